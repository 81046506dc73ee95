"""maskflownet_amd.run on the MI355X: a training run from settings files, resume, clear_steps, the head-stack start, mixed batch slots,
and the --valid / --predict modes of `python -m maskflownet_amd.train`.

Every test builds its own tiny dataset tree with the project's writers: 64 x 64 samples, crop 64 x 64, batch 2 (the size
tests/test_data_feed.py trains at); the run of the first test -- schedule [[4, 1e-4], [7, 5e-5]], validation and checkpoint every 3
steps, seed 0, MaskFlownet_S -- is made once and its checkpoints serve the tests after it."""
import os
import re
import types

import numpy as np
import pytest

from tests import data_ref

pytestmark = pytest.mark.gpu

SCHEDULE = [[4, 1e-4], [7, 5e-5]]
STAMP = r"^\[\d{4}/\d\d/\d\d \d\d:\d\d:\d\d\] "


# ---- synthetic trees ---------------------------------------------------------------------------------------------------------------------
def _pair(rng, H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 127 + 60 * np.sin(xx / 9.0)[..., None] + 50 * np.cos(yy / 7.0)[..., None] + rng.uniform(-15, 15, (H, W, 3))
    img1 = np.clip(base, 0, 255).astype(np.uint8)
    img2 = np.clip(np.roll(base, 2, axis=1) + rng.uniform(-3, 3, (H, W, 3)), 0, 255).astype(np.uint8)
    flow = (np.stack([np.full((H, W), 2.0), np.zeros((H, W))], axis=-1) + rng.standard_normal((H, W, 2)) * 0.25).astype(np.float32)
    return img1, img2, flow


def _write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6 %d %d 255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def _chairs_tree(root, rng, n_train=8, n_valid=2):
    from maskflownet_amd import io
    os.makedirs(os.path.join(root, "data"))
    split = [1] * n_train + [2] * n_valid
    split[2], split[-1] = split[-1], split[2]          # the validation samples are not simply the last ones
    for k in range(1, len(split) + 1):
        a, b, f = _pair(rng, 64, 64)
        _write_ppm(os.path.join(root, "data", "%05d_img1.ppm" % k), a)
        _write_ppm(os.path.join(root, "data", "%05d_img2.ppm" % k), b)
        io.write_flo(os.path.join(root, "data", "%05d_flow.flo" % k), f)
    with open(os.path.join(root, "train_val.txt"), "w") as f:
        f.write("".join("%d\n" % v for v in split))
    return {"root": os.path.join(root, "data"), "split": os.path.join(root, "train_val.txt")}


def _sintel_tree(root, rng, split_of_pass, H=64, W=64):
    """Two sequences of three frames per pass (two pairs each); the split file has one entry per training pair of a pass."""
    from maskflownet_amd import io
    for seq in ("alley_1", "cave_4"):
        for kind in ("clean", "final", "flow", "invalid"):
            os.makedirs(os.path.join(root, "training", kind, seq))
        for kind in ("clean", "final"):
            os.makedirs(os.path.join(root, "test", kind, seq))
        for i in (1, 2, 3):
            a, b, f = _pair(rng, H, W)
            for part in ("training", "test"):
                io.write_png(os.path.join(root, part, "clean", seq, "frame_%04d.png" % i), a)
                io.write_png(os.path.join(root, part, "final", seq, "frame_%04d.png" % i), b)
            if i < 3:
                io.write_flo(os.path.join(root, "training", "flow", seq, "frame_%04d.flo" % i), f)
                io.write_png(os.path.join(root, "training", "invalid", seq, "frame_%04d.png" % i), ((rng.uniform(size=(H, W)) < 0.1) * 255).astype(np.uint8))
    with open(os.path.join(root, "split.txt"), "w") as f:
        f.write(" ".join(str(v) for v in split_of_pass) + "\n")
    return {"root": root, "split": os.path.join(root, "split.txt")}


def _flow_png(rng, H, W):
    _, _, f = _pair(rng, H, W)
    valid = rng.uniform(size=(H, W)) > 0.2
    return np.concatenate([np.round(f * 64 + 32768).astype(np.uint16), valid[..., None].astype(np.uint16)], axis=-1)


def _kitti_tree(root, rng, pairs=4, H=64, W=64, valid=(1,)):
    from maskflownet_amd import io
    for sub in ("image", "flow_occ", "testing"):
        os.makedirs(os.path.join(root, sub))
    for k in range(pairs):
        a, b, _ = _pair(rng, H, W)
        for sub in ("image", "testing"):
            io.write_png(os.path.join(root, sub, "%06d_10.png" % k), a)
            io.write_png(os.path.join(root, sub, "%06d_11.png" % k), b)
        io.write_png(os.path.join(root, "flow_occ", "%06d_10.png" % k), _flow_png(rng, H, W))
    return {"image": os.path.join(root, "image"), "flow_occ": os.path.join(root, "flow_occ"), "testing": os.path.join(root, "testing"),
            "valid": list(valid)}


def _hd1k_tree(root, rng, H=180, W=280):
    from maskflownet_amd import io
    for sub in ("image", "flow_occ"):
        os.makedirs(os.path.join(root, sub))
    for frame in (10, 11, 12, 13):
        io.write_png(os.path.join(root, "image", "000000_%04d.png" % frame), _pair(rng, H, W)[0])
        if frame < 13:
            io.write_png(os.path.join(root, "flow_occ", "000000_%04d.png" % frame), _flow_png(rng, H, W))
    return {"image": os.path.join(root, "image"), "flow_occ": os.path.join(root, "flow_occ"), "valid": []}


def _yaml(path, tree):
    import yaml
    with open(path, "w") as f:
        yaml.safe_dump(tree, f)
    return str(path)


def _settings(folder, cls="MaskFlownet_S", dataset="chairs", validation=3, checkpoint=3, **more):
    os.makedirs(folder, exist_ok=True)
    net = _yaml(os.path.join(folder, cls + ".yaml"), {"optimizer": {"learning_rate": SCHEDULE}, "network": {"class": cls}})
    ds = {"dataset": dataset, "validation_steps": validation, "checkpoint_steps": checkpoint, "orig_shape": [64, 64], "target_shape": [64, 64]}
    ds.update(more)
    return net, _yaml(os.path.join(folder, "%s_%s.yaml" % (dataset, cls)), ds)


def _watch(run):
    """What the network is fed (a forward pre-hook, as tests/test_data_feed.py takes it) and the learning rate the Trainer steps at, per
    step of the run."""
    import torch
    seen = types.SimpleNamespace(fed={}, lr={})
    run.net.register_forward_pre_hook(lambda mod, args: seen.fed.__setitem__(run.steps, torch.cat(args, 0).cpu().numpy()))
    inner = run.trainer.step

    def step(batch_size):
        seen.lr[run.steps] = run.trainer.learning_rate
        return inner(batch_size)
    run.trainer.step = step
    return seen


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _equal_to_file(named, path, prefix=""):
    from maskflownet_amd import io
    got = io.load_params(path)
    return all((_bits(p.detach().cpu().numpy()) == _bits(got[prefix + k])).all() for k, p in named)


@pytest.fixture(scope="module")
def s_run(tmp_path_factory):
    from maskflownet_amd import config, run
    base = tmp_path_factory.mktemp("run")
    rng = np.random.default_rng(0)
    data = {"chairs": _chairs_tree(str(base / "chairs"), rng)}
    net_cfg, ds_cfg = _settings(str(base / "cfg"), batch_size=2)
    root = str(base / "root")
    r = run.TrainingRun(config.load(net_cfg), config.load(ds_cfg), data, root, seed=0, batch=2)
    seen = _watch(r)
    last = r.run()
    r.close()
    return types.SimpleNamespace(run=r, seen=seen, last=last, root=root, data=data, net_cfg=net_cfg, ds_cfg=ds_cfg, base=base,
                                 log=open(os.path.join(root, "logs", r.run_id + ".log")).read().splitlines())


def test_gpu_run_from_files(s_run):
    from maskflownet_amd import io, network, run
    r = s_run.run
    assert s_run.last == 7 and r.steps == 7 and not r.step()
    assert (r.batch_size, r.orig_shape, r.target_shape, r.train_size, r.validation_size) == (2, [64, 64], [64, 64], 8, 2)
    assert r.network_class == "MaskFlownet_S" and all(s is r.slots[0] for s in r.slots)
    log = s_run.log
    assert all(re.match(STAMP, l) for l in log)
    assert re.search(r"\] start=0, train=8, val=2, host=\S+, batch=2$", log[0]) and re.search(r"\] seed=0, checkpoint=None, clear_steps=False$", log[1])
    train = [re.search(r"\] steps=(\d+), epe=(\S+), total_time=(\d+\.\d\d)$", l) for l in log if "total_time=" in l]
    assert [int(m.group(1)) for m in train] == [1, 2, 3, 4, 5, 6, 7] and all(np.isfinite(float(m.group(2))) for m in train)
    val = [re.search(r"\] steps=(\d+), chairs=(\S+)$", l) for l in log[2:] if "total_time=" not in l]
    assert [int(m.group(1)) for m in val] == [1, 3, 6] and all(np.isfinite(float(m.group(2))) and float(m.group(2)) > 0 for m in val)
    assert len(log) == 2 + 7 + 3
    weights = sorted(os.listdir(os.path.join(s_run.root, "weights")))
    assert weights == sorted("%s_%d%s" % (r.run_id, s, x) for s in (3, 6) for x in run.CHECKPOINT_SUFFIXES)
    assert s_run.seen.lr == {1: 1e-4, 2: 1e-4, 3: 1e-4, 4: 1e-4, 5: 5e-5, 6: 5e-5, 7: 5e-5}
    assert sorted(s_run.seen.fed) == [1, 2, 3, 4, 5, 6, 7] and s_run.seen.fed[1].shape == (4, 3, 64, 64)
    assert run.find_checkpoints(s_run.root, r.run_id)[-1][1] == 6
    params = io.load_params(os.path.join(s_run.root, "weights", "%s_3.params" % r.run_id))
    inference = network.MaskFlownetS(network.from_reference_keys(params), 1, 64, 64)
    assert set(params) == set(network.random_params(0)) and inference is not None


def test_gpu_resume_continues_the_run(s_run):
    from maskflownet_amd import config, io, run, training
    first = s_run.run
    prefix = os.path.join(s_run.root, "weights", "%s_3" % first.run_id)
    r = run.TrainingRun(config.load(s_run.net_cfg), config.load(s_run.ds_cfg), s_run.data, s_run.root, seed=123, batch=2,
                        checkpoint="%s:3" % first.run_id[:3])
    assert r.run_id == first.run_id and r.steps == 3 and r.trainer.num_update == 3
    assert _equal_to_file(training.reference_named_parameters(r.net), prefix + ".params")
    assert _equal_to_file(r.trainer.mean.items(), prefix + ".states", "mean:") and _equal_to_file(r.trainer.var.items(), prefix + ".states", "var:")
    assert any(bool(v.any()) for v in r.trainer.var.values())
    assert [os.path.basename(p) for p in r.loop.checkpoints] == ["%s_3" % first.run_id]
    seen = _watch(r)
    assert r.run() == 7
    r.close()
    assert sorted(seen.fed) == [4, 5, 6, 7] and seen.lr == {4: 1e-4, 5: 5e-5, 6: 5e-5, 7: 5e-5}
    for s in (4, 5, 6, 7):       # sampler and both augmenters continue: the network is fed the uninterrupted run's batch
        assert (seen.fed[s].view(np.uint32) == s_run.seen.fed[s].view(np.uint32)).all(), "step %d" % s
    log = open(os.path.join(s_run.root, "logs", r.run_id + ".log")).read().splitlines()
    assert log[:len(s_run.log)] == s_run.log and open(os.path.join(s_run.root, "logs", r.run_id + ".log.bak")).read().splitlines() == s_run.log
    more = log[len(s_run.log):]
    assert re.search(r"\] start=3, train=8, val=2, host=\S+, batch=2$", more[0])
    assert [int(re.search(r"steps=(\d+)", l).group(1)) for l in more[2:]] == [4, 5, 6, 6, 7]
    assert len(run.read_log(os.path.join(s_run.root, "logs", r.run_id + ".log"))[1]) == 2
    assert sorted(os.listdir(os.path.join(s_run.root, "weights"))) == sorted("%s_%d%s" % (r.run_id, s, x) for s in (3, 6) for x in run.CHECKPOINT_SUFFIXES)


def test_gpu_clear_steps_starts_a_new_run(s_run):
    from maskflownet_amd import config, run, training
    first = s_run.run
    prefix = os.path.join(s_run.root, "weights", "%s_3" % first.run_id)
    r = run.TrainingRun(config.load(s_run.net_cfg), config.load(s_run.ds_cfg), s_run.data, s_run.root, seed=0, batch=2,
                        checkpoint="%s:3" % first.run_id, clear_steps=True)
    assert r.run_id != first.run_id and r.steps == 0 and r.trainer.num_update == 0 and r.loop.checkpoints == []
    assert _equal_to_file(training.reference_named_parameters(r.net), prefix + ".params")
    assert not any(bool(v.any()) for v in r.trainer.mean.values()) and not any(bool(v.any()) for v in r.trainer.var.values())
    seen = _watch(r)
    assert r.run(max_steps=1) == 1 and sorted(seen.fed) == [1]
    r.close()
    assert (seen.fed[1].view(np.uint32) == s_run.seen.fed[1].view(np.uint32)).all()      # seed 0 again: the first run's first batch
    log = open(os.path.join(s_run.root, "logs", r.run_id + ".log")).read().splitlines()
    assert re.search(r"\] start=0, ", log[0]) and re.search(r"\] steps=1, epe=", log[2]) and re.search(r"\] steps=1, chairs=", log[3])


def test_gpu_head_stack_start(s_run):
    """MaskFlownet, clear_steps, chairs: the S checkpoint fills the head alone, and the head stays frozen."""
    from maskflownet_amd import config, run
    first = s_run.run
    net_cfg, ds_cfg = _settings(str(s_run.base / "cfg_full"), cls="MaskFlownet", batch_size=2)
    r = run.TrainingRun(config.load(net_cfg), config.load(ds_cfg), s_run.data, s_run.root, seed=1, batch=2,
                        checkpoint="%s:3" % first.run_id, clear_steps=True)
    path = os.path.join(s_run.root, "weights", "%s_3.params" % first.run_id)
    head = [(k.replace("__", "."), p) for k, p in r.net.head.P.items()]
    assert r.network_class == "MaskFlownet" and len(head) == 142 and _equal_to_file(head, path)
    assert not any(k.startswith("MaskFlownet_S.") for k in r.trainer.names) and not any(p.requires_grad for _, p in head)
    before = {k: p.detach().clone() for k, p in r.net.P.items()}
    assert r.run(max_steps=2) == 2
    r.close()
    assert _equal_to_file(head, path)
    assert any(bool((p.detach() != before[k]).any()) for k, p in r.net.P.items())


def test_gpu_mixed_slots(tmp_path):
    """The 'sintel' branch with kitti: 1, hd1k: 1: slot k of every batch is cut from data set k at the sampler's draw, with its mask."""
    from maskflownet_amd import config, run
    rng = np.random.default_rng(5)
    data = {"sintel": _sintel_tree(str(tmp_path / "sintel"), rng, [1, 2, 1, 1]),
            "kitti": {"2015": _kitti_tree(str(tmp_path / "kitti15"), rng)}, "hd1k": _hd1k_tree(str(tmp_path / "hd1k"), rng)}
    net_cfg, ds_cfg = _settings(str(tmp_path / "cfg"), dataset="sintel", validation=100, checkpoint=100, kitti=1, hd1k=1)
    r = run.TrainingRun(config.load(net_cfg), config.load(ds_cfg), data, str(tmp_path / "root"), seed=2, batch=2)
    sintel, kitti, hd1k = r.slots[0], r.slots[2], r.slots[3]
    assert len(r.slots) == 4 and r.slots[1] is sintel and kitti is not sintel and hd1k is not kitti and r.batch_size == 4
    assert (len(sintel), len(kitti), len(hd1k)) == (6, 4, 2) and r.train_size == 12         # 3 of 4 pairs per pass; 4 pairs; 3 maps less the first
    assert {kitti.shape(i) for i in range(4)} == {(436, 1024)} and {hd1k.shape(i) for i in range(2)} == {(436, 1024)}
    assert sorted(r.validation_sets) == ["sintel.clean", "sintel.final"] and r.validation_size == 2
    batches, inner = [], r.feeder.next

    def next_batch():
        batches.append((inner(), r.feeder.last_draw))
        return batches[-1][0]
    r.feeder.next = next_batch
    assert r.run(max_steps=2) == 2
    r.close()
    assert len(batches) == 2 and batches[0][1] != batches[1][1]
    for batch, draw in batches:
        assert batch[3] is not None and tuple(batch[3].shape) == (4, 1, 64, 64)
        want = data_ref.gather_batch([ds.host(d[0]) for ds, d in zip(r.slots, draw)], (64, 64), [d[1:] for d in draw], True)
        for name, g, w in zip(("img1", "img2", "label", "mask"), batch, want):
            assert (_bits(g.cpu().numpy()) == _bits(w)).all(), name
        assert draw[0][0] != draw[1][0]                                 # the two Sintel slots share one permutation
        assert any(d[1] or d[2] for d in draw[2:])                      # the resized sets leave room for the crop
    log = open(os.path.join(str(tmp_path / "root"), "logs", r.run_id + ".log")).read().splitlines()
    assert re.search(r"\] start=0, train=12, val=2, ", log[0]) and re.search(r"\] steps=1, sintel.clean=\S+, sintel.final=\S+$", log[3])


def _lookup_data(base, rng):
    return {"sintel": _sintel_tree(str(base / "sintel"), rng, [1, 2, 2, 1]),
            "kitti": {"2012": _kitti_tree(str(base / "kitti12"), rng, pairs=2, H=70, W=100, valid=[0]),
                      "2015": _kitti_tree(str(base / "kitti15"), rng, pairs=2, H=64, W=90, valid=[1])}}


def test_gpu_valid_mode(s_run, tmp_path):
    from maskflownet_amd import data as mfn_data, readers, run, train, training
    tree = _lookup_data(tmp_path, np.random.default_rng(6))
    rid = s_run.run.run_id
    assert train.main([s_run.net_cfg, "--data", _yaml(tmp_path / "data.yaml", tree), "--root", s_run.root, "-c", rid + ":3", "--valid",
                       "--batch", "2"]) == 0
    lines = open(os.path.join(s_run.root, "logs", "val", rid + ".val.log")).read().splitlines()
    got = dict(re.search(STAMP + r"steps=3, (\S+)=(\S+)$", l).groups() for l in lines)
    # the same sets, built here from the listers and the readers
    sets = {}
    entries = readers.sintel_entries(tree["sintel"]["root"], readers.read_split(tree["sintel"]["split"]), parts=("training",))
    for div in ("training2", "training"):
        for subset in ("clean", "final"):
            ds = mfn_data.DeviceDataset("cuda")
            ds.extend(readers.sintel_samples(tree["sintel"]["root"], subset, entries[div][subset]))
            sets["sintel.%s.%s" % (div, subset)] = ds
    for edition in ("2012", "2015"):
        ds = mfn_data.DeviceDataset("cuda")
        for a, b, fo in readers.kitti_samples(tree["kitti"][edition]["image"], tree["kitti"][edition]["flow_occ"], range(2)):
            ds.append_raw(a, b, fo, resize=(1224, 370))
        sets["kitti." + edition] = ds
    assert [len(sets[k]) for k in sets] == [2, 2, 4, 4, 2, 2]
    net, full = run._build_net(None, "MaskFlownet_S", os.path.join(s_run.root, "weights", rid + "_3.params"), "cuda:0")
    want = training.Validation(sets, 2, full=full).run(net, kitti=True)
    expect = {}
    for name, r in want.items():
        expect[name + ":epe"] = repr(r["epe"])
        if name.startswith("kitti."):
            expect[name + ":kitti"] = repr(r["fl"])
    assert got == expect and len(lines) == 8 and all(np.isfinite(float(v)) for v in got.values())


def test_gpu_predict_mode(s_run, tmp_path):
    import torch
    from maskflownet_amd import io, ops, predict, train
    tree = _lookup_data(tmp_path, np.random.default_rng(7))
    rid = s_run.run.run_id
    assert train.main([s_run.net_cfg, "--data", _yaml(tmp_path / "data.yaml", tree), "--root", s_run.root, "-c", rid + ":3", "--predict",
                       "--resize", "128,192"]) == 0
    flows = os.path.join(s_run.root, "flows")
    params = io.load_params(os.path.join(s_run.root, "weights", rid + "_3.params"))
    made = sorted(os.path.relpath(os.path.join(d, f), flows) for d, _, fs in os.walk(flows) for f in fs)
    assert made == sorted([os.path.join(rid + "_3_sintel", "final", seq, "frame_%04d.flo" % i) for seq in ("alley_1", "cave_4") for i in (1, 2)]
                          + [os.path.join(rid + "_3_kitti", ed, "%06d_10.png" % k) for ed in ("2012", "2015") for k in (0, 1)])

    def flow_of(p, a, b):
        out = p.do_batch_u8(torch.stack([a, b]), 0, 1, 1, warped=False)
        return np.flip(out["flow"][0].cpu().numpy().transpose(1, 2, 0), axis=-1)
    # KITTI: the frames resized to 128 x 192 in BGR order, the flow at that size, quantised as predict.py:63-66 does
    p = predict.Predictor(params, 1, 128, 192, resize=(128, 192))
    for edition in ("2012", "2015"):
        for k in (0, 1):
            raw = [io.read_png(os.path.join(tree["kitti"][edition]["testing"], "%06d_%d.png" % (k, t)))[..., 2::-1] for t in (10, 11)]
            a, b = (ops.cv_resize_u8(torch.from_numpy(np.ascontiguousarray(x)).cuda(), (128, 192)) for x in raw)
            flow = flow_of(p, a, b)
            png = io.read_png(os.path.join(flows, rid + "_3_kitti", edition, "%06d_10.png" % k))
            assert png.dtype == np.uint16 and png.shape == (128, 192, 3) and (png[..., 2] == 1).all()
            assert (png[..., :2] == (64.0 * (flow.astype(np.float64) + 512.0)).astype(np.uint16)).all() and np.abs(flow).max() < 500
    # Sintel test/final: the network at 128 x 192, the flow at the frames' own 64 x 64
    p = predict.Predictor(params, 1, 64, 64, resize=(128, 192))
    for seq in ("alley_1", "cave_4"):
        for i in (1, 2):
            a, b = (torch.from_numpy(io.read_png(os.path.join(tree["sintel"]["root"], "test", "final", seq, "frame_%04d.png" % n))[..., :3].copy()).cuda()
                    for n in (i, i + 1))
            got = io.read_flo(os.path.join(flows, rid + "_3_sintel", "final", seq, "frame_%04d.flo" % i))
            assert got.shape == (64, 64, 2) and (got.view(np.uint32) == np.ascontiguousarray(flow_of(p, a, b)).view(np.uint32)).all()
