"""maskflownet_amd.config / run (the host policy) / the new listers of readers: everything a training run decides without a device.

The settings files under tests/golden/reference_config and the log excerpts (the first 200 lines of each) under
tests/golden/reference_logs are the reference's own; tests/golden/reference_splits.json records its KITTI and HD1K validation index
lists and the first 160 entries of its Sintel split."""
import glob
import json
import os
import re

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CONFIGS = sorted(glob.glob(os.path.join(GOLDEN, "reference_config", "*.yaml")))
LOGS = sorted(glob.glob(os.path.join(GOLDEN, "reference_logs", "*.log")))
SCHEDULE = [[4, 1e-4], [7, 5e-5]]


def _cfg(name):
    from maskflownet_amd import config
    return config.load(os.path.join(GOLDEN, "reference_config", name))


def _splits():
    with open(os.path.join(GOLDEN, "reference_splits.json")) as f:
        return json.load(f)


# ---- config ----------------------------------------------------------------------------------------------------------------------------
def test_every_reference_settings_file_parses():
    from maskflownet_amd import config
    assert len(CONFIGS) == 13
    for path in CONFIGS:
        cfg = config.load(path)
        assert isinstance(cfg.get(), dict) and cfg.get()
        if os.path.basename(path).startswith("MaskFlownet"):
            assert getattr(cfg.network, "class").value in ("MaskFlownet", "MaskFlownet_S")
        else:
            assert cfg.dataset.value in ("chairs", "sintel", "kitti", "things3d")
            assert cfg.validation_steps.value == 2500 and cfg.checkpoint_steps.value == 5000


def test_settings_come_out_as_written():
    s = _cfg("MaskFlownet_S.yaml")
    assert getattr(s.network, "class").value == "MaskFlownet_S"
    assert s.optimizer.learning_rate.value == [[400000, 1e-4], [600000, 5e-5], [800000, 2.5e-5], [1000000, 1.25e-5], [1200000, 6.25e-6]]
    assert all(isinstance(lr, float) for _, lr in s.optimizer.learning_rate.value)
    assert s.optimizer.q.get(None) is None and s.network.mw.get([.005, .01, .02, .08, .32]) == [.005, .01, .02, .08, .32]
    k = _cfg("MaskFlownet_kitti.yaml")
    assert getattr(k.network, "class").value == "MaskFlownet" and k.optimizer.q.value == 0.4
    assert k.optimizer.learning_rate.value[0] == [50000, 3e-5] and k.optimizer.learning_rate.value[-1] == [300000, 0.5e-6]
    assert len(k.optimizer.learning_rate.value) == 12
    mixed = _cfg("sintel_kitti2015_hd1k.yaml")
    assert (mixed.dataset.value, mixed.kitti.value, mixed.hd1k.value, mixed.target_shape.value) == ("sintel", 1, 1, [320, 768])
    plain = _cfg("sintel.yaml")
    assert plain.kitti.get(0) == 0 and plain.hd1k.get(0) == 0 and plain.train_all.get(False) is False
    assert _cfg("chairs.yaml").target_shape.value == [320, 448] and _cfg("kitti.yaml").target_shape.value == [320, 896]
    t = _cfg("things3d.yaml")
    assert t.sub_type.value == "clean" and t.target_shape.value == [384, 768] and t.orig_shape.get([540, 960]) == [540, 960]


def test_reader_is_null_safe_and_value_raises():
    from maskflownet_amd.config import Reader
    cfg = Reader({"a": {"b": 1, "none": None}, "leaf": 3, "zero": 0, "no": False})
    assert cfg.a.b.value == 1 and cfg.a.b.get(7) == 1
    assert cfg.x.y.z.get("d") == "d" and cfg.a.none.get(5) == 5 and cfg.a.none.below.get(6) == 6 and cfg.leaf.below.get(2) == 2
    assert cfg.zero.get(9) == 0 and cfg.no.get(True) is False          # present, falsy values are values
    assert cfg.x.get() is None
    for missing in (cfg.x, cfg.a.c, cfg.a.none, cfg.leaf.below.further):
        with pytest.raises(KeyError):
            missing.value
    with pytest.raises(KeyError, match=r"a\.c"):
        cfg.a.c.value


# ---- RunPolicy -------------------------------------------------------------------------------------------------------------------------
def test_policy_schedule_validation_and_checkpoints():
    from maskflownet_amd.run import RunPolicy
    p = RunPolicy(3, 3, SCHEDULE)
    assert [p.learning_rate(s) for s in range(1, 9)] == [1e-4] * 4 + [5e-5] * 3 + [None]
    assert [p.ends(s) for s in range(1, 9)] == [False] * 7 + [True]
    assert [s for s in range(1, 8) if p.validates(s)] == [1, 3, 6]
    assert [s for s in range(1, 8) if p.checkpoints(s)] == [3, 6]
    nested = RunPolicy(3, 2, SCHEDULE)
    assert [s for s in range(1, 8) if nested.checkpoints(s)] == [6]
    assert [s for s in range(1, 121) if p.logs(s)] == list(range(1, 21)) + [50, 100]
    assert p.validates(0) and p.validates(1)          # steps <= 1


def test_policy_on_the_chairs_schedule():
    """MaskFlownet_S.yaml's schedule with chairs.yaml's cadences: boundaries train at their own rate, the run ends past the last one."""
    from maskflownet_amd.run import RunPolicy
    sched = _cfg("MaskFlownet_S.yaml").optimizer.learning_rate.value
    p = RunPolicy(2500, 5000, sched)
    assert p.learning_rate(400000) == 1e-4 and p.learning_rate(400001) == 5e-5
    assert not p.ends(1200000) and p.ends(1200001)
    assert p.checkpoints(5000) and not p.checkpoints(2500) and p.validates(2500)


class _Unreadable:
    """What a training step returns: anything that would bring it to the host raises."""

    def _no(self, *a, **k):
        raise AssertionError("a training value was read on a step that logs nothing")
    cpu = numpy = item = tolist = mean = __float__ = __array__ = __iter__ = __len__ = __bool__ = __int__ = __index__ = _no


class _Readable:
    def __init__(self, v):
        self.v, self.reads = v, 0

    def cpu(self):
        self.reads += 1
        return self

    def numpy(self):
        return np.array([self.v, self.v + 2.0], np.float32)


def _loop(tmp_path, policy, logged_only=True, validate=True):
    from maskflownet_amd import run
    os.makedirs(tmp_path / "weights", exist_ok=True)
    log = run.RunLog(str(tmp_path / "run.log"))
    seen = {"train": [], "validate": [], "save": [], "values": []}

    def train(steps, lr):
        seen["train"].append((steps, lr))
        if logged_only and not policy.logs(steps):
            return {"epe": _Unreadable()}
        seen["values"].append(_Readable(float(steps)))
        return {"epe": seen["values"][-1]}

    def val():
        seen["validate"].append(loop.steps)
        return {"chairs": 1.5, "sintel.clean": 2.5}

    def save(prefix):
        seen["save"].append(prefix)
        for suffix in run.CHECKPOINT_SUFFIXES:
            open(prefix + suffix, "w").close()
    loop = run.RunLoop(policy, log, train, val if validate else None, save, str(tmp_path / "weights" / "abcJan01-0000"))
    return loop, log, seen


def test_loop_reads_training_values_on_logged_steps_only(tmp_path):
    from maskflownet_amd.run import RunPolicy
    policy = RunPolicy(1000, 1000, [[120, 1e-4]])
    loop, log, seen = _loop(tmp_path, policy)
    assert loop.run() == 120 and loop.steps == 120 and not loop.step() and loop.steps == 120
    log.close()
    assert [s for s, _ in seen["train"]] == list(range(1, 121)) and {lr for _, lr in seen["train"]} == {1e-4}
    assert [v.reads for v in seen["values"]] == [1] * 22            # steps 1..20, 50, 100: read once each
    lines = open(tmp_path / "run.log").read().splitlines()
    train_lines = [l for l in lines if "total_time=" in l]
    assert [int(re.search(r"steps=(\d+),", l).group(1)) for l in train_lines] == list(range(1, 21)) + [50, 100]
    # the first line: the moving average of one value v is v * 1 / (1e-8 * 0.95 + 1); np.mean([1, 3]) = 2
    first = re.match(r"^\[.*\] steps=1, epe=(\S+), total_time=0\.00$", train_lines[0])
    assert first and float(first.group(1)) == 2.0 / (1e-8 * 0.95 + 1)
    assert seen["validate"] == [1] and seen["save"] == []
    assert sum("chairs=1.5, sintel.clean=2.5" in l for l in lines) == 1


def test_loop_runs_the_policy_of_the_issue(tmp_path):
    from maskflownet_amd.run import RunPolicy
    loop, log, seen = _loop(tmp_path, RunPolicy(3, 3, SCHEDULE), logged_only=False)
    assert loop.run() == 7
    assert seen["train"] == [(s, 1e-4) for s in (1, 2, 3, 4)] + [(s, 5e-5) for s in (5, 6, 7)]
    assert seen["validate"] == [1, 3, 6]
    assert [os.path.basename(p) for p in seen["save"]] == ["abcJan01-0000_3", "abcJan01-0000_6"]
    nested, _, seen2 = _loop(tmp_path / "nested", RunPolicy(3, 2, SCHEDULE), logged_only=False)
    nested.run()
    assert [os.path.basename(p) for p in seen2["save"]] == ["abcJan01-0000_6"]
    capped, _, seen3 = _loop(tmp_path / "capped", RunPolicy(3, 3, SCHEDULE), logged_only=False)
    assert capped.run(max_steps=2) == 2 and capped.run(max_steps=100) == 7
    silent, _, seen4 = _loop(tmp_path / "silent", RunPolicy(3, 3, SCHEDULE), logged_only=False, validate=False)
    silent.run()
    assert seen4["validate"] == [] and len(seen4["save"]) == 2      # validationSize 0: no line, the checkpoint all the same


def test_rotation_keeps_the_last_three(tmp_path):
    from maskflownet_amd import run
    loop, log, seen = _loop(tmp_path, run.RunPolicy(1, 1, [[5, 1e-4]], keep=3), logged_only=False)
    assert loop.run() == 5
    left = sorted(os.listdir(tmp_path / "weights"))
    assert left == sorted("abcJan01-0000_%d%s" % (s, x) for s in (3, 4, 5) for x in run.CHECKPOINT_SUFFIXES)
    assert [os.path.basename(p) for p in loop.checkpoints] == ["abcJan01-0000_%d" % s for s in (3, 4, 5)]
    assert run.RunPolicy(1, 1, SCHEDULE).rotate(list("abcde")) == (list("cde"), list("ab"))
    assert run.RunPolicy(1, 1, SCHEDULE).rotate(list("ab")) == (list("ab"), [])
    # the loop's state carries the list: a resumed loop goes on rotating
    state = loop.state()
    again, _, _ = _loop(tmp_path, run.RunPolicy(1, 1, [[6, 1e-4]], keep=3), logged_only=False)
    again.set_state(state)
    assert again.run() == 6
    assert sorted(os.listdir(tmp_path / "weights")) == sorted("abcJan01-0000_%d%s" % (s, x) for s in (4, 5, 6) for x in run.CHECKPOINT_SUFFIXES)


def test_moving_averages():
    from maskflownet_amd.run import DictMovingAverage, MovingAverage
    m = MovingAverage()
    assert (m.sum, m.weight, m.ratio) == (0, 1e-8, 0.95)
    s, w = 0.0, 1e-8
    for v in (3.0, 1.0, 4.0, 1.0, 5.0):
        m.update(v)
        s, w = s * 0.95 + v, w * 0.95 + 1
        assert m.average == s / w
    d = DictMovingAverage()
    d.update({"epe": 2.0})
    d.update({"epe": 4.0, "loss": 1.0})
    assert d.average == {"epe": (2.0 * 0.95 + 4.0) / ((1e-8 * 0.95 + 1) * 0.95 + 1), "loss": 1.0 / (1e-8 * 0.95 + 1)}


# ---- log, lookup, id, formats ------------------------------------------------------------------------------------------------------------
STAMP = re.compile(r"^\[\d{4}/\d\d/\d\d \d\d:\d\d:\d\d\] ")


def test_run_log_lines_and_backup(tmp_path, capsys):
    import datetime
    from maskflownet_amd import run
    path = str(tmp_path / "a.log")
    log = run.RunLog(path)
    log.log("start=0, train=8, val=2, host=h, batch=2")
    log.log("x=1")
    log.close()
    assert not os.path.exists(path + ".bak") and capsys.readouterr().out == ""
    first = open(path).read()
    assert all(STAMP.match(l) for l in first.splitlines()) and first.splitlines()[1].endswith("] x=1")
    stamp = datetime.datetime.strptime(first[:22], "[%Y/%m/%d %H:%M:%S] ")
    utc = datetime.datetime.now(datetime.timezone.utc).replace(tzinfo=None)
    assert abs((stamp - utc).total_seconds() - 8 * 3600) < 120          # UTC+8, whatever the machine's zone
    log = run.RunLog(path, screen=True)
    log.log("start=3")
    log.close()
    assert open(path + ".bak").read() == first and open(path).read().startswith(first) and len(open(path).read().splitlines()) == 3
    assert STAMP.match(capsys.readouterr().out) is not None


def _header_by_hand(path):
    with open(path) as f:
        lines = [f.readline(), f.readline()]
    out = {}
    for ln in lines:
        out.update(item.split("=", 1) for item in ln[ln.index("] ") + 2:].strip().split(", "))
    return out


@pytest.mark.parametrize("path", LOGS, ids=[os.path.basename(p) for p in LOGS])
def test_read_log_on_the_reference_logs(path):
    from maskflownet_amd import run
    assert len(LOGS) == 4 and len(open(path).read().splitlines()) <= 200
    val, info = run.read_log(path)
    assert len(info) == 1 and val == []
    want = _header_by_hand(path)
    assert info[0] == want
    for key in ("start", "train", "val", "batch", "config", "checkpoint"):
        assert key in info[0], key
    assert info[0]["start"] == "0" and int(info[0]["train"]) > 0 and info[0]["config"].startswith("'MaskFlownet")
    # the training lines of the excerpt are the steps the policy logs
    lines = open(path).read().splitlines()
    assert all(STAMP.match(l) for l in lines)
    logged = [int(re.search(r"\] steps=(\d+),", l).group(1)) for l in lines if "total_time=" in l]
    policy = run.RunPolicy(2500, 5000, [[10 ** 7, 1e-4]])
    assert logged == [s for s in range(1, max(logged) + 1) if policy.logs(s)] and max(logged) > 2500
    validated = sorted({int(re.search(r"\] steps=(\d+),", l).group(1)) for l in lines[2:] if "total_time=" not in l})
    # the validation at steps <= 1 is in the two November logs; the two September ones were written by a revision of the script without it
    assert [s for s in validated if s > 1] == [s for s in range(2, max(logged) + 1) if policy.validates(s)]
    assert (validated[0] == 1) == ("Nov" in os.path.basename(path))


def test_read_log_merges_the_line_after_every_start(tmp_path):
    from maskflownet_amd import run
    path = str(tmp_path / "r.log")
    log = run.RunLog(path)
    log.log(run.format_start(0, 8, 2, "h", 2))
    log.log(run.format_arguments({"config": "a.yaml", "batch": 8, "checkpoint": None, "tag": "t1"}))
    log.log(run.format_train(1, {"epe": 3.25}, 0.0))
    log.log("val_epe=2.0, steps=1")
    log.log("not a record")
    log.log(run.format_start(3, 8, 2, "h", 2))
    log.log(run.format_arguments({"config": "a.yaml", "checkpoint": "abc:3"}))
    log.close()
    val, info = run.read_log(path)
    assert val == [{"val_epe": "2.0", "steps": "1"}]
    assert info == [{"start": "0", "train": "8", "val": "2", "host": "h", "batch": "8", "config": "'a.yaml'", "checkpoint": "None", "tag": "'t1'"},
                    {"start": "3", "train": "8", "val": "2", "host": "h", "batch": "2", "config": "'a.yaml'", "checkpoint": "'abc:3'"}]


def test_find_log_and_checkpoints(tmp_path):
    from maskflownet_amd import run
    root = str(tmp_path)
    os.makedirs(tmp_path / "logs" / "val")
    os.makedirs(tmp_path / "weights")
    for name in ("5adNov03-0005.log", "5adNov03-0005.log.bak", "771Sep25-0735.log", "notes.txt", "val"):
        if name != "val":
            open(tmp_path / "logs" / name, "w").close()
    for rid, steps in (("5adNov03-0005", (5000, 10000, 995000)), ("771Sep25-0735", (5000,))):
        for s in steps:
            for x in run.CHECKPOINT_SUFFIXES:
                open(tmp_path / "weights" / ("%s_%d%s" % (rid, s, x)), "w").close()
    assert run.find_log(root, "5ad") == (os.path.join(root, "logs", "5adNov03-0005.log"), "5adNov03-0005")
    assert run.find_log(root, "5adNov03") == run.find_log(root, "5adNov03-0005") == run.find_log(root, "5ad")
    assert run.find_log(root, "771")[1] == "771Sep25-0735"
    for missing in ("zzz", "5adNov03-0005.log", "adNov"):
        with pytest.raises(ValueError, match="Not found"):
            run.find_log(root, missing)
    found = run.find_checkpoints(root, "5adNov03-0005")
    assert [s for _, s in found] == [5000, 10000, 995000]                # by number, not by name
    assert found[0][0] == os.path.join(root, "weights", "5adNov03-0005_5000.params")
    assert run.find_checkpoints(root, "nothing") == []
    latest = run.resolve_checkpoint(root, "5ad")
    assert latest == (os.path.join(root, "logs", "5adNov03-0005.log"), "5adNov03-0005", os.path.join(root, "weights", "5adNov03-0005_995000.params"), 995000)
    assert run.resolve_checkpoint(root, "5ad:10000")[2:] == (os.path.join(root, "weights", "5adNov03-0005_10000.params"), 10000)
    with pytest.raises(ValueError, match="no checkpoint of steps 7"):
        run.resolve_checkpoint(root, "5ad:7")


def test_run_id_and_formats():
    import datetime
    import hashlib
    from maskflownet_amd import run
    now = datetime.datetime(2019, 11, 3, 0, 5, 59)
    rid = run.run_id("msragpux04", now, "0,1")
    assert rid == hashlib.sha224(b"msragpux04Nov03-00050,1").hexdigest()[:3] + "Nov03-0005"
    assert re.match(r"^[0-9a-f]{3}[A-Z][a-z]{2}\d\d-\d{4}$", run.run_id())
    assert run.run_id("a", now, "0") != run.run_id("b", now, "0")
    assert run.format_start(0, 394, 79, "msragpux04", 4) == "start=0, train=394, val=79, host=msragpux04, batch=4"
    assert run.format_arguments({"batch": 8, "config": "MaskFlownet_S.yaml", "clear_steps": True, "checkpoint": None}) == \
        "batch=8, config='MaskFlownet_S.yaml', clear_steps=True, checkpoint=None"
    assert run.format_train(50, {"epe": 19.756858747915913}, 0.2749) == "steps=50, epe=19.756858747915913, total_time=0.27"
    assert run.format_validation(1, {"sintel.clean": 2.8726730346679688, "sintel.final": 4.583795547485352}) == \
        "steps=1, sintel.clean=2.8726730346679688, sintel.final=4.583795547485352"
    assert run.format_validation(1, {}) == "steps=1"


def test_cli_arguments():
    from maskflownet_amd import train
    a = train.parser().parse_args(["net.yaml"])
    assert (a.config, a.dataset_cfg, a.shard, a.checkpoint, a.clear_steps, a.network, a.debug, a.valid, a.predict, a.resize, a.batch) == \
        ("net.yaml", "chairs.yaml", 1, None, False, "MaskFlownet", False, False, False, "", 8)
    a = train.parser().parse_args(["net.yaml", "--dataset_cfg", "d.yaml", "-s", "4", "-g", "2", "-c", "abc:3", "--clear_steps", "--debug",
                                   "--resize", "448,1024", "--batch", "2", "--data", "data.yaml", "--root", "runs", "--seed", "5", "--valid"])
    assert (a.shard, a.gpu_device, a.checkpoint, a.clear_steps, a.debug, a.resize, a.batch, a.data, a.root, a.seed, a.valid) == \
        (4, "2", "abc:3", True, True, "448,1024", 2, "data.yaml", "runs", 5, True)
    assert train.device_of("3") == "cuda:3"
    with pytest.raises(NotImplementedError, match="GradientBuckets"):
        train.device_of("0,1")
    with pytest.raises(NotImplementedError, match="GradientBuckets"):
        train.main(["net.yaml", "-g", "0,1,2,3"])


# ---- listers ---------------------------------------------------------------------------------------------------------------------------
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").close()


def test_things3d_lists(tmp_path):
    from maskflownet_amd import readers
    root = str(tmp_path)
    for camera in ("left", "right"):
        for direction in ("into_future", "into_past"):
            for n in (6, 15):
                _touch(os.path.join(root, "train", "flow", camera, direction, "%07d.flo" % n))
    flows = lambda camera, direction: os.path.join(root, "train", "flow", camera, direction)
    clean = readers.things3d_entries(root, "clean")
    assert len(clean) == 8
    # the four camera x direction lists, in the reference's order
    assert [os.path.dirname(e[2]) for e in clean[::2]] == [flows("left", "into_future"), flows("left", "into_past"),
                                                            flows("right", "into_future"), flows("right", "into_past")]
    img = lambda sub, camera, n: os.path.join(root, "train", "image_" + sub, camera, "%07d.png" % n)
    by_flow = {e[2]: e for e in clean}
    assert by_flow[os.path.join(flows("left", "into_future"), "0000006.flo")][:2] == (img("clean", "left", 6), img("clean", "left", 7))
    assert by_flow[os.path.join(flows("left", "into_past"), "0000006.flo")][:2] == (img("clean", "left", 6), img("clean", "left", 5))
    assert by_flow[os.path.join(flows("right", "into_past"), "0000015.flo")][:2] == (img("clean", "right", 15), img("clean", "right", 14))
    final = readers.things3d_entries(root, "final")
    assert [e[2] for e in final] == [e[2] for e in clean] and all("image_final" in e[0] and "image_final" in e[1] for e in final)
    assert readers.things3d_entries(root, "mixed") == clean + final
    with pytest.raises(ValueError, match="sub_type"):
        readers.things3d_entries(root, "albedo")


def test_kitti_parts_against_the_recorded_lists():
    from maskflownet_amd import readers
    lists = _splits()["kitti"]
    assert len(lists["2012"]) == 39 and len(lists["2015"]) == 40 and lists["2015"][-1] == 199
    for edition, n in (("2012", 194), ("2015", 200)):
        valid = lists[edition]
        assert valid == sorted(set(valid))
        got = {part: readers.kitti_indices(n, valid, part) for part in ("train", "valid", "mixed")}
        assert got["mixed"] == list(range(n)) and got["valid"] == valid
        assert got["train"] == [k for k in range(n) if k not in set(valid)] and len(got["train"]) == n - len(valid)
    # the reference's count of a 200-file directory is 199: its own validation index 199 is then never read
    assert readers.kitti_indices(199, lists["2015"], "valid") == lists["2015"][:-1]
    assert readers.kitti_indices(4, [1, 3], "train") == [0, 2] and readers.kitti_indices(4, [3, 1], "valid") == [3]
    with pytest.raises(ValueError, match="part"):
        readers.kitti_indices(4, [], "test")


def test_kitti_count(tmp_path):
    from maskflownet_amd import readers
    for k in range(5):
        _touch(str(tmp_path / ("%06d_10.png" % k)))
    _touch(str(tmp_path / "readme.txt"))
    assert readers.kitti_count(str(tmp_path)) == 5 and readers.kitti_count(str(tmp_path), follow_reference=True) == 4


def test_hd1k_skips_the_first_map_of_every_sequence(tmp_path):
    from maskflownet_amd import readers
    names = ["000000_0010", "000000_0011", "000000_0012", "000001_0010", "000001_0011", "000002_0010", "000003_0010", "000003_0011"]
    for n in names:
        _touch(str(tmp_path / (n + ".png")))
    # position 5 (000002_0010, the recorded validation index) aside, every map but a sequence's first stands for (frame - 1, frame)
    assert _splits()["hd1k"] == [5]
    assert readers.hd1k_names(str(tmp_path), [5], "mixed") == ["000000_0010", "000000_0011", "000001_0010", "000003_0010"]
    assert readers.hd1k_names(str(tmp_path), [5], "train") == ["000000_0010", "000000_0011", "000001_0010", "000003_0010"]
    assert readers.hd1k_names(str(tmp_path), [5], "valid") == []           # a part of one map: it is its sequence's first
    assert readers.hd1k_names(str(tmp_path), [4], "train") == ["000000_0010", "000000_0011", "000003_0010"]   # 000001_0010 is now first of what is left
    assert readers.hd1k_names(str(tmp_path), [5], "mixed", samples=3) == ["000000_0010", "000000_0011"]
    # what hd1k_samples reads for a name: frames F and F + 1 and the flow map of F
    assert readers.hd1k_names(str(tmp_path), [], "mixed")[-1] == "000003_0010"


def _sintel_tree(root, order):
    for part, kinds in (("training", ("clean", "final")), ("test", ("clean", "final"))):
        for kind in kinds:
            for seq, frames in order:
                for i in frames:
                    _touch(os.path.join(root, part, kind, seq, "frame_%04d.png" % i))
                _touch(os.path.join(root, part, kind, seq, "notes.txt"))


def test_sintel_split_is_consumed_in_listing_order(tmp_path, monkeypatch):
    from maskflownet_amd import readers
    root = str(tmp_path)
    seqs = [("market_2", (1, 2, 3)), ("alley_1", (1, 2, 3, 4)), ("cave_4", (7, 8))]
    _sintel_tree(root, seqs)
    real = os.listdir

    def listed(path):          # the walk follows os.listdir's order, whatever it is: here neither sorted nor reversed
        got = real(path)
        if os.path.basename(path) in ("clean", "final"):
            assert sorted(got) == sorted(s for s, _ in seqs)
            return [s for s, _ in seqs]
        return got
    monkeypatch.setattr(os, "listdir", listed)
    split = [1, 2, 2, 1, 1, 2]       # market_2: 1, 2; alley_1: 2, 1, 1; cave_4: 2
    got = readers.sintel_entries(root, split)
    pairs = [("market_2", 1), ("market_2", 2), ("alley_1", 1), ("alley_1", 2), ("alley_1", 3), ("cave_4", 7)]
    for subset in ("clean", "final"):      # the split starts anew for every subset
        assert got["training"][subset] == pairs and got["test"][subset] == pairs
        assert got["training1"][subset] == [pairs[0], pairs[3], pairs[4]]
        assert got["training2"][subset] == [pairs[1], pairs[2], pairs[5]]
    assert set(got) == {"training", "training1", "training2", "test"}
    prefix = _splits()["sintel_split_prefix"]
    assert set(prefix) == {1, 2} and readers.sintel_entries(root, prefix)["training2"]["clean"] == []     # the recorded prefix opens with 1s
    with pytest.raises(ValueError, match="more training pairs"):
        readers.sintel_entries(root, split[:5])
    assert readers.sintel_entries(root, None, parts=("test",), subsets=("final",)) == {"test": {"final": pairs}}


def test_read_split_and_chairs_split(tmp_path):
    from maskflownet_amd import readers
    (tmp_path / "s.txt").write_text("1\n1\n2\n1\n2\n")
    (tmp_path / "t.txt").write_text("1.000000000000000000e+00 2.000000000000000000e+00\n1\n")
    assert readers.read_split(str(tmp_path / "s.txt")) == [1, 1, 2, 1, 2] and readers.read_split(str(tmp_path / "t.txt")) == [1, 2, 1]
    assert readers.chairs_split([1, 1, 2, 1, 2]) == ([1, 2, 4], [3, 5])


def test_sintel_branch_slot_table():
    from maskflownet_amd import run
    assert run.sintel_slots(0, 0) == ["sintel"] * 4
    assert run.sintel_slots(1, 1) == ["sintel", "sintel", "kitti", "hd1k"]
    assert run.sintel_slots(2, 0) == ["sintel", "sintel", "kitti", "kitti"]
    with pytest.raises(ValueError, match="do not fit"):
        run.sintel_slots(3, 2)


def test_augmenter_state_round_trip():
    """state() / set_state(): the draws (and for colour the Philox key and call counter) continue where the state was taken."""
    import pickle
    from maskflownet_amd import augment
    geo, col = augment.presets("kitti", 2, (64, 64), (64, 64), seed=3)
    geo.draw(), col.draw()
    col.calls = 41
    sg, sc = pickle.loads(pickle.dumps((geo.state(), col.state())))
    want_g, want_c = [geo.table() for _ in range(3)], [col.table(col.draw()) for _ in range(3)]
    geo2, col2 = augment.presets("kitti", 2, (64, 64), (64, 64), seed=99)
    assert col2.seed != col.seed
    geo2.set_state(sg), col2.set_state(sc)
    assert (col2.seed, col2.calls) == (col.seed, 41)
    for w in want_g:
        assert (geo2.table().view(np.uint32) == w.view(np.uint32)).all()
    for w in want_c:
        assert (col2.table(col2.draw()).view(np.uint32) == w.view(np.uint32)).all()
