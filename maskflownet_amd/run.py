"""Training runs from the reference's settings files: the run loop, its log, checkpoints and resume.

The reference's main.py puts its readers, augmenters, pipeline and logger together at module level; this module is that script as a
library, in two layers:

* the HOST POLICY, importable and testable without a device: `RunLog` (logger.py), `read_log` / `find_log` / `find_checkpoints`
  (path.py, relative to a run root), `MovingAverage` / `DictMovingAverage` (main.py:427-457), `RunPolicy` -- the loop's decisions as
  pure functions of the step number --, `run_id`, the message formats, and `RunLoop`, the loop of main.py:511-556 over three callables
  (train one batch, validate, save a checkpoint);
* the DEVICE BINDING: `load_datasets` (the dataset table of main.py:190-365 into data.DeviceDataset), `TrainingRun` (net, loss, Trainer,
  augmenters, Feeder, Validation and RunLog behind a RunLoop), `validate_checkpoint` (main.py:163-187) and `predict_checkpoint`
  (predict.py:8-66).  `python -m maskflownet_amd.train` is the command line on top.

A run root holds what the reference keeps next to its sources: logs/<run_id>.log, logs/val/, logs/debug/, weights/<run_id>_<steps>.params
/ .states / .run, flows/.

What a step of the loop costs the hot path (Feeder.next -> training.train_batch): a few host comparisons, two timer reads and one
set_learning_rate; a step that logs nothing reads nothing back from the device and allocates nothing on it."""
import datetime
import hashlib
import os
import pickle
import re
import shutil
import socket
from timeit import default_timer

import numpy as np

from .training import learning_rate_at

TIMEZONE_HOURS = 8            # logger.py:6: the reference's logs are stamped in UTC+8 wherever they run


def local_time():
    return datetime.datetime.now(datetime.timezone.utc).replace(tzinfo=None) + datetime.timedelta(hours=TIMEZONE_HOURS)


class RunLog:
    """logger.py's FileLog: an append-only file of lines '[%Y/%m/%d %H:%M:%S] msg' stamped at UTC+8 and flushed one by one; a file that
    exists is copied to <path>.bak before it is appended to; screen=True echoes every line."""

    def __init__(self, path, screen=False):
        if os.path.exists(path):
            shutil.copy(path, path + ".bak")
        self.path, self.screen = path, bool(screen)
        self._f = open(path, "a")

    @staticmethod
    def timestamp():
        return local_time().strftime("[%Y/%m/%d %H:%M:%S] ")

    def log(self, msg, end="\n"):
        line = self.timestamp() + msg + end
        self._f.write(line)
        self._f.flush()
        if self.screen:
            print(line, end="", flush=True)

    def close(self):
        self._f.close()


# ---- path.py: logs and checkpoints of a run root ---------------------------------------------------------------------------------------
def _list_dir(folder, pattern):
    rx = re.compile(pattern)
    for f in sorted(os.listdir(folder)):
        m = rx.match(f)
        if m is not None:
            yield (os.path.join(folder, f),) + m.groups()


def find_log(root, prefix):
    """-> (log file, run id) of the run whose id begins with `prefix`: the files of root/logs that match ^(prefix(.*\\d)?)\\.log$, so a
    prefix is completed up to a final digit ('5ad' finds '5adNov03-0005.log').  Of several matches the first in sorted order is taken
    (the reference takes os.listdir's first); none raises ValueError."""
    hits = list(_list_dir(os.path.join(root, "logs"), r"^(%s(.*\d)?)\.log$" % re.escape(prefix)))
    if not hits:
        raise ValueError("Not found {}".format(prefix))
    return hits[0][:2]


def find_checkpoints(root, run_id):
    """-> [(path of the .params file, steps)] of root/weights/<run_id>*_<steps>.params, ascending by step number."""
    hits = _list_dir(os.path.join(root, "weights"), r"^%s.*_(\d+)\.params$" % re.escape(run_id))
    return sorted(((p, int(s)) for p, s in hits), key=lambda t: t[1])


def resolve_checkpoint(root, checkpoint):
    """'prefix' or 'prefix:steps' (main.py:83-100) -> (log file, run id, .params path, steps): the run's latest checkpoint, or the one of
    the given step number."""
    prefix, _, steps = checkpoint.partition(":")
    log_file, rid = find_log(root, prefix)
    found = find_checkpoints(root, rid)
    if steps:
        found = [t for t in found if t[1] == int(steps)]
    if not found:
        raise ValueError("no checkpoint%s of run %s under %s" % (" of steps " + steps if steps else "", rid, os.path.join(root, "weights")))
    return (log_file, rid) + found[-1]


def read_log(fname):
    """path.py:33-53 -> (val, exp_info).  Every line's message is split at ', ' into k=v items (at the first '='; the values stay
    strings).  A line with a 'start' key opens a record of exp_info and the line that FOLLOWS it is merged into the record -- the
    header pair of a run, so a key of the second line (its 'batch', the validation batch) replaces the first's; a file that a resumed
    run appended to has one record per start.  Lines with a 'val_epe' key are collected in val.  A line that does not split into k=v
    items is skipped (the reference re-reads the previous line's items there)."""
    val, exp_info, in_start = [], [], False
    with open(fname) as f:
        for ln in f:
            p = ln.find("] ")
            items = ln[p + 2:].strip().split(", ")
            if not all("=" in item for item in items):
                continue
            kvs = dict(item.split("=", 1) for item in items)
            if "val_epe" in kvs:
                val.append(kvs)
            elif "start" in kvs:
                exp_info.append(kvs)
                in_start = True
            elif in_start:
                exp_info[-1].update(kvs)
                in_start = False
    return val, exp_info


# ---- main.py:427-457 -------------------------------------------------------------------------------------------------------------------
class MovingAverage:
    def __init__(self, ratio=0.95):
        self.sum, self.weight, self.ratio = 0, 1e-8, ratio

    def update(self, v):
        self.sum = self.sum * self.ratio + v
        self.weight = self.weight * self.ratio + 1

    @property
    def average(self):
        return self.sum / self.weight


class DictMovingAverage:
    def __init__(self, ratio=0.95):
        self.sum, self.weight, self.ratio = {}, {}, ratio

    def update(self, v):
        for key in v:
            if key not in self.sum:
                self.sum[key], self.weight[key] = 0, 1e-8
            self.sum[key] = self.sum[key] * self.ratio + v[key]
            self.weight[key] = self.weight[key] * self.ratio + 1

    @property
    def average(self):
        return {key: self.sum[key] / self.weight[key] for key in self.sum}


class RunPolicy:
    """The decisions of the loop of main.py:511-556 as pure functions of `steps`, the counter AFTER its increment at the top of an
    iteration (the first iteration of a fresh run is steps = 1).  The reference's quirks are kept: steps <= 1 validates whatever the
    cadence; a checkpoint is written only inside the validation branch, so only at steps that both cadences divide; the training line
    and the moving average see the first twenty steps and every fiftieth, nothing else."""

    def __init__(self, validation_steps, checkpoint_steps, lr_schedule, keep=3):
        self.validation_steps, self.checkpoint_steps, self.keep = int(validation_steps), int(checkpoint_steps), int(keep)
        self.lr_schedule = [[int(b), float(lr)] for b, lr in lr_schedule]
        if self.validation_steps < 1 or self.checkpoint_steps < 1 or self.keep < 1 or not self.lr_schedule:
            raise ValueError("RunPolicy: cadences and keep must be >= 1 and the schedule non-empty")

    def learning_rate(self, steps):
        """The step's learning rate, or None: the run ends BEFORE this step (pipeline.py:65-75, main.py:515-516)."""
        return learning_rate_at(self.lr_schedule, steps)

    def ends(self, steps):
        return self.learning_rate(steps) is None

    def logs(self, steps):
        return steps <= 20 or steps % 50 == 0

    def validates(self, steps):
        return steps % self.validation_steps == 0 or steps <= 1

    def checkpoints(self, steps):
        return self.validates(steps) and steps % self.checkpoint_steps == 0

    def rotate(self, checkpoints):
        """-> (kept, dropped) of the list of checkpoint prefixes after one was appended: the last `keep` stay (main.py:552-556)."""
        n = max(0, len(checkpoints) - self.keep)
        return list(checkpoints[n:]), list(checkpoints[:n])


CHECKPOINT_SUFFIXES = (".params", ".states", ".run")


def run_id(host=None, now=None, device=""):
    """main.py:113-116: sha224(host + '%b%d-%H%M' + device)[:3] followed by the same '%b%d-%H%M' (UTC+8)."""
    stamp = (now if now is not None else local_time()).strftime("%b%d-%H%M")
    uid = (host if host is not None else socket.gethostname()) + stamp + device
    return hashlib.sha224(uid.encode()).hexdigest()[:3] + stamp


def format_start(start, train, val, host, batch):
    return "start={}, train={}, val={}, host={}, batch={}".format(start, train, val, host, batch)


def format_arguments(arguments):
    return ", ".join("{}={}".format(k, repr(v)) for k, v in arguments.items())


def format_train(steps, averages, total_time):
    return "steps={}{}, total_time={:.2f}".format(steps, "".join(", {}={}".format(k, v) for k, v in averages.items()), total_time)


def format_validation(steps, result):
    return "steps={}{}".format(steps, "".join(", {}={}".format(k, v) for k, v in result.items()))


def _host_mean(v):
    """np.mean of a returned value on the host (pipeline.py:115): the one place where a training value leaves the device."""
    if hasattr(v, "cpu"):
        v = v.cpu().numpy()
    return float(np.mean(np.asarray(v)))


class RunLoop:
    """The loop of main.py:511-556 over three callables, so that it runs without a device:

        train(steps, lr) -> {name: per-sample values}      one batch fed, augmented and trained at learning rate lr
        validate()       -> {set name: value}              None (the argument) where there is nothing to validate on (validationSize 0)
        save(prefix)                                        writes prefix + each of CHECKPOINT_SUFFIXES

    `step()` is one iteration and returns False, having done nothing, where the schedule has ended.  What train returns is read on
    the host (`_host_mean`) only on a step that logs; on every other step it is dropped unread."""

    def __init__(self, policy, log, train, validate, save, weights_prefix, steps=0, timer=default_timer):
        self.policy, self.log, self.train, self.validate, self.save = policy, log, train, validate, save
        self.weights_prefix, self.steps, self.timer = weights_prefix, int(steps), timer
        self.total_time, self.train_avg = MovingAverage(), DictMovingAverage()
        self.checkpoints = []
        self.last_validation = None
        self._t1 = None

    def step(self):
        p = self.policy
        self.steps += 1
        steps = self.steps
        lr = p.learning_rate(steps)
        if lr is None:
            self.steps -= 1        # the reference exits here; the counter stays at the last step that ran
            return False
        t0 = self.timer()
        if self._t1 is not None:
            self.total_time.update(t0 - self._t1)
        self._t1 = t0
        train_log = self.train(steps, lr)
        if p.logs(steps):
            self.train_avg.update({k: _host_mean(v) for k, v in train_log.items()})
            self.log.log(format_train(steps, self.train_avg.average, self.total_time.average))
        if p.validates(steps):
            if self.validate is not None:
                self.last_validation = self.validate()
                self.log.log(format_validation(steps, self.last_validation))
            if steps % p.checkpoint_steps == 0:
                prefix = "{}_{}".format(self.weights_prefix, steps)
                self.checkpoints.append(prefix)
                self.save(prefix)           # sees the list with itself in it: a resumed run rotates as the first would have
                self.checkpoints, dropped = p.rotate(self.checkpoints)
                for old in dropped:
                    for suffix in CHECKPOINT_SUFFIXES:
                        try:
                            os.remove(old + suffix)
                        except OSError as e:
                            self.log.log("Remove failed " + str(e))
        return True

    def run(self, max_steps=None):
        """Until the schedule ends, or for at most max_steps iterations.  -> the number of the last step that ran."""
        n = 0
        while (max_steps is None or n < max_steps) and self.step():
            n += 1
        return self.steps

    def state(self):
        return {"steps": self.steps, "checkpoints": list(self.checkpoints),
                "total_time": (self.total_time.sum, self.total_time.weight),
                "train_avg": (dict(self.train_avg.sum), dict(self.train_avg.weight))}

    def set_state(self, state):
        self.steps, self.checkpoints = int(state["steps"]), list(state["checkpoints"])
        self.total_time.sum, self.total_time.weight = state["total_time"]
        self.train_avg.sum, self.train_avg.weight = dict(state["train_avg"][0]), dict(state["train_avg"][1])


# ---- the dataset table of main.py:190-365 ----------------------------------------------------------------------------------------------
def _need(data, *keys):
    node = data
    for k in keys:
        node = node.get(k) if isinstance(node, dict) else None
        if node is None:
            raise KeyError("the data file has no entry '%s' (INTEGRATION.md: the data file)" % ".".join(str(k) for k in keys))
    return node


def _take(items, samples):
    """The first `samples` items; a negative count takes all (the reference's [:samples] with its default -1 drops the last one)."""
    items = list(items)
    return items if samples is None or samples < 0 else items[:samples]


def sintel_slots(num_kitti, num_hd1k, batch_size=4):
    """main.py:244-260: which data set fills which batch slot of the 'sintel' branch."""
    n = batch_size - num_kitti - num_hd1k
    if min(n, num_kitti, num_hd1k) < 0:
        raise ValueError("sintel_slots: kitti=%d and hd1k=%d do not fit a batch of %d" % (num_kitti, num_hd1k, batch_size))
    return ["sintel"] * n + ["kitti"] * num_kitti + ["hd1k"] * num_hd1k


HD1K_CROP = ((50, 50), (100, 100))       # hd1k.py:16, :51


def _kitti_set(ds, data, edition, part, resize, samples, crop=None):
    from . import readers
    flow_dir = _need(data, "kitti", edition, "flow_occ")
    n = readers.kitti_count(flow_dir)
    if samples is not None and samples >= 0:
        n = min(n, samples)
    idx = readers.kitti_indices(n, list(_need(data, "kitti", edition, "valid")), part)
    for a, b, fo in readers.kitti_samples(_need(data, "kitti", edition, "image"), flow_dir, idx):
        ds.append_raw(a, b, fo, crop=crop, resize=resize)
    return ds


def _sintel_sets(data, device, division, samples):
    """{pass: DeviceDataset} of one division ('training', 'training1', 'training2') of Sintel."""
    from . import readers
    from .data import DeviceDataset
    root = _need(data, "sintel", "root")
    entries = readers.sintel_entries(root, readers.read_split(_need(data, "sintel", "split")), parts=("training",))
    out = {}
    for subset, ent in entries[division].items():
        ds = DeviceDataset(device)
        ds.extend(readers.sintel_samples(root, subset, _take(ent, samples)))
        out[subset] = ds
    return out


def load_datasets(dataset_cfg, data, device, samples=-1, shard=1, flow_dtype=None, network_class="MaskFlownet"):
    """The four branches of main.py:197-365 -> (slots, validation, batch_size, orig_shape): one data.DeviceDataset per batch slot (the
    same object where slots share a set), {name: DeviceDataset} to validate on, the training batch and the crop the sampler cuts.

    dataset_cfg: a config.Reader of the reference's dataset files (`dataset`, `orig_shape`, `train_all`, `kitti`, `hd1k`,
    `resize_shape`, `sub_type`; `batch_size` is this project's addition and overrides the branch's batch).  data: the user's mapping
    of roots, split files and validation index lists.  samples: at most that many per set, -1 = all (--debug: 32);
    shard: every shard-th FlyingThings3D sample; flow_dtype: None = float16 for things3d (main.py:297), float32 otherwise.
    network_class picks the Sintel division the 'chairs' branch validates on: 'training' for MaskFlownet_S, 'training2' for MaskFlownet.

    Deviations: a negative `samples` takes every sample (`_take`); KITTI directories are counted by readers.kitti_count; the Sintel
    validation sets of the 'chairs' branch are loaded only where the data file has a `sintel` entry."""
    from . import readers
    from .data import DeviceDataset
    name = dataset_cfg.dataset.value
    dtype = flow_dtype or ("float16" if name == "things3d" else "float32")
    new = lambda: DeviceDataset(device, flow_dtype=dtype)
    validation = {}
    if name == "kitti":
        batch_size, orig_shape = 4, list(dataset_cfg.orig_shape.get([370, 1224]))
        resize = (orig_shape[1], orig_shape[0])
        part = "mixed" if dataset_cfg.train_all.get(False) else "train"
        train = new()
        for edition in ("2012", "2015"):
            _kitti_set(train, data, edition, part, resize, samples)
        slots = [train] * batch_size
        for edition, key in (("2012", "kitti.12"), ("2015", "kitti.15")):
            validation[key] = _kitti_set(new(), data, edition, "valid", resize, samples)
    elif name == "sintel":
        batch_size, orig_shape = 4, [436, 1024]
        num_kitti, num_hd1k = int(dataset_cfg.kitti.get(0)), int(dataset_cfg.hd1k.get(0))
        root = _need(data, "sintel", "root")
        entries = readers.sintel_entries(root, readers.read_split(_need(data, "sintel", "split")), parts=("training",))
        train = new()
        for subset, ent in entries["training" if dataset_cfg.train_all.get(False) else "training1"].items():
            train.extend(readers.sintel_samples(root, subset, _take(ent, samples)))
        sets = {"sintel": train}
        resize = (1024, int(dataset_cfg.resize_shape.get(436)))
        if num_kitti > 0:
            sets["kitti"] = _kitti_set(new(), data, "2015", "mixed", resize, samples)
        if num_hd1k > 0:
            flow_dir = _need(data, "hd1k", "flow_occ")
            sets["hd1k"] = new()
            names = readers.hd1k_names(flow_dir, data["hd1k"].get("valid", (5,)), "mixed", samples)
            for a, b, fo in readers.hd1k_samples(_need(data, "hd1k", "image"), flow_dir, names):
                sets["hd1k"].append_raw(a, b, fo, crop=HD1K_CROP, premultiply=True, normalize=True, resize=resize)
        slots = [sets[k] for k in sintel_slots(num_kitti, num_hd1k, int(dataset_cfg.batch_size.get(batch_size)))]
        for subset, ds in _sintel_sets(data, device, "training2", samples).items():
            validation["sintel." + subset] = ds
    elif name == "things3d":
        batch_size, orig_shape = 4, [540, 960]
        entries = readers.things3d_entries(_need(data, "things3d", "root"), dataset_cfg.sub_type.get("clean"))
        train = new()
        train.extend(readers.things3d_samples(_take(entries, samples)[::max(1, int(shard))]))
        slots = [train] * batch_size
        _, valid = readers.chairs_split(readers.read_split(_need(data, "chairs", "split")))
        validation["chairs"] = DeviceDataset(device)
        validation["chairs"].extend(readers.chairs_samples(_need(data, "chairs", "root"), _take(valid, samples)))
    elif name == "chairs":
        batch_size, orig_shape = 8, [384, 512]
        root = _need(data, "chairs", "root")
        train_idx, valid = readers.chairs_split(readers.read_split(_need(data, "chairs", "split")))
        train = new()
        train.extend(readers.chairs_samples(root, _take(train_idx, samples)))
        slots = [train] * batch_size
        validation["chairs"] = new()
        validation["chairs"].extend(readers.chairs_samples(root, _take(valid, samples)))
        if isinstance(data.get("sintel"), dict):
            division = "training2" if network_class == "MaskFlownet" else "training"
            for subset, ds in _sintel_sets(data, device, division, samples).items():
                validation["sintel." + subset] = ds
    else:
        raise NotImplementedError("dataset %r" % (name,))
    if name != "sintel":
        slots = slots[:1] * int(dataset_cfg.batch_size.get(batch_size))
    batch_size = len(slots)
    orig_shape = [int(v) for v in dataset_cfg.orig_shape.get(orig_shape)]
    return slots, validation, batch_size, orig_shape


# ---- the device binding ----------------------------------------------------------------------------------------------------------------
class TrainingRun:
    """main.py from its line 59 on, for one device: a training run built from a network settings file and a dataset settings file
    (config.Reader each), the user's `data` mapping and a run root.

    network: 'MaskFlownet_S' or 'MaskFlownet'; None takes `network.class` of the settings (default 'MaskFlownet', pipeline.py:24).
    checkpoint: 'prefix' or 'prefix:steps' of a run under the same root (resolve_checkpoint).  Which of the reference's three load
    modes applies (main.py:126-143): for the class MaskFlownet with clear_steps on the 'chairs' dataset the checkpoint is a
    MaskFlownet_S one and fills the head alone (training.load_head); otherwise it fills the whole net.  The head of a MaskFlownet is
    always frozen (MaskFlownetTrainable; the reference freezes it only when it loads a checkpoint and would otherwise train a random
    head).  Without clear_steps the run CONTINUES: same run id and log file, the trainer's states, and -- what the reference loses at a
    restart -- the step counter, the sampler's and both augmenters' random state, the moving averages and the checkpoint list, from
    the checkpoint's .run file.  With clear_steps the steps start at 1 under a new run id and nothing but weights is taken.
    debug: 32 samples per set and the log under logs/debug.  arguments: what the second header line records (the command line's)."""

    def __init__(self, network_cfg, dataset_cfg, data, root, network=None, seed=0, checkpoint=None, clear_steps=False, debug=False,
                 device="cuda:0", shard=1, batch=8, arguments=None, screen=False):
        import torch
        from . import augment, network as net_mod, training
        from .data import BatchSampler, Feeder
        self.root, self.seed, self.debug = root, int(seed), bool(debug)
        self.network_class = network or getattr(network_cfg.network, "class").get("MaskFlownet")
        if self.network_class not in ("MaskFlownet_S", "MaskFlownet"):
            raise NotImplementedError("network class %r" % (self.network_class,))
        full = self.network_class == "MaskFlownet"
        self.dataset = dataset_cfg.dataset.value
        for sub in ("logs", os.path.join("logs", "val"), os.path.join("logs", "debug"), "weights", "flows"):
            os.makedirs(os.path.join(root, sub), exist_ok=True)

        steps, self.tag, self.checkpoint = 0, None, None
        if checkpoint is not None:
            log_file, rid, self.checkpoint, steps = resolve_checkpoint(root, checkpoint)
            if clear_steps:
                steps = 0
            else:
                info = read_log(log_file)[1]
                if info and "tag" in info[-1]:
                    import ast
                    self.tag = ast.literal_eval(info[-1]["tag"])
        if checkpoint is None or clear_steps:
            # two runs started on one host and device within a minute would share the reference's id, and with it log and weights:
            # the hashed string then gets a counter behind the device, which changes the three-letter tag alone
            self.run_id, n = run_id(device=str(device)), 0
            while os.path.exists(os.path.join(root, "logs", "debug" if debug else "", self.run_id + ".log")):
                n += 1
                self.run_id = run_id(device="%s#%d" % (device, n))
        else:
            self.run_id = rid

        schedule = dataset_cfg.optimizer.learning_rate.get(None) or network_cfg.optimizer.learning_rate.value
        self.policy = RunPolicy(dataset_cfg.validation_steps.value, dataset_cfg.checkpoint_steps.value, schedule)

        self.net = (training.MaskFlownetTrainable if full else training.MaskFlownetSTrainable)(net_mod.random_params(self.seed, full=full)).to(device)
        mw = network_cfg.network.mw.get(None)
        q = network_cfg.optimizer.q.get(None)
        self.loss_fn = training.FusedMultiscaleEpe(q=q, weights=tuple(mw)) if (mw is not None and len(mw) == 5) else training.FusedMultiscaleEpe(q=q)
        self.trainer = training.Trainer(training.reference_named_parameters(self.net), "adam", {"learning_rate": 1e-4})
        if self.checkpoint is not None:
            if full and clear_steps and self.dataset == "chairs":
                training.load_head(self.checkpoint, self.net)
            else:
                training.load_checkpoint(self.checkpoint[:-len(".params")], self.net)
            if not clear_steps:
                self.trainer.load_states(self.checkpoint[:-len(".params")] + ".states")

        self.slots, self.validation_sets, self.batch_size, self.orig_shape = load_datasets(
            dataset_cfg, data, device, samples=32 if debug else -1, shard=shard, network_class=self.network_class)
        self.target_shape = [int(v) for v in dataset_cfg.target_shape.get([s + (64 - s) % 64 for s in self.orig_shape])]
        self.geo_aug, self.color_aug = augment.presets(self.dataset, self.batch_size, tuple(self.orig_shape), tuple(self.target_shape), seed=self.seed)
        self.feeder = Feeder(BatchSampler(self.slots, self.orig_shape, seed=self.seed))
        self.validation = training.Validation(self.validation_sets, batch, full=full)
        distinct = {id(ds): ds for ds in self.slots}
        self.train_size = sum(len(ds) for ds in distinct.values())
        self.validation_size = sum(len(ds) for ds in self.validation_sets.values())

        self.log = RunLog(os.path.join(root, "logs", "debug" if debug else "", self.run_id + ".log"), screen=screen)
        self.loop = RunLoop(self.policy, self.log, self._train, self._validate if self.validation_size > 0 else None, self.save,
                            os.path.join(root, "weights", self.run_id), steps=steps)
        if self.checkpoint is not None and not clear_steps:
            self._load_run_state(self.checkpoint[:-len(".params")] + ".run", steps)
        self.log.log(format_start(self.loop.steps, self.train_size, self.validation_size, socket.gethostname(), self.batch_size))
        self.log.log(format_arguments(arguments if arguments is not None else {"seed": self.seed, "checkpoint": checkpoint, "clear_steps": bool(clear_steps)}))
        torch.cuda.synchronize(device)        # the sets are resident before the first step is timed

    @property
    def steps(self):
        return self.loop.steps

    def _train(self, steps, lr):
        from . import training
        self.trainer.set_learning_rate(lr)
        img1, img2, label, mask = self.feeder.next()
        _, epe = training.train_batch(self.net, self.loss_fn, self.trainer, img1, img2, label, mask, self.geo_aug, self.color_aug)
        return {"epe": epe}

    def _validate(self):
        return self.validation.run(self.net)

    def save(self, prefix):
        """pipeline.py:52-54's .params and .states, and the .run file that lets a restart continue this run."""
        from . import training
        training.save_checkpoint(prefix, self.net, self.trainer)
        state = {"version": 1, "loop": self.loop.state(), "sampler": self.feeder.sampler.state(), "geo_aug": self.geo_aug.state(),
                 "color_aug": self.color_aug.state()}
        with open(prefix + ".run.tmp", "wb") as f:
            pickle.dump(state, f)
        os.replace(prefix + ".run.tmp", prefix + ".run")

    def _load_run_state(self, path, steps):
        with open(path, "rb") as f:
            state = pickle.load(f)
        if state.get("version") != 1 or state["loop"]["steps"] != steps:
            raise ValueError("%s: not the run state of step %d" % (path, steps))
        self.loop.set_state(state["loop"])
        self.feeder.sampler.set_state(state["sampler"])
        self.geo_aug.set_state(state["geo_aug"])
        self.color_aug.set_state(state["color_aug"])

    def step(self):
        """One iteration of main.py:513-556; False where the schedule has ended."""
        return self.loop.step()

    def run(self, max_steps=None):
        return self.loop.run(max_steps)

    def close(self):
        self.log.close()


def _build_net(network_cfg, network, params_path, device):
    from . import network as net_mod, training
    cls = network or getattr(network_cfg.network, "class").get("MaskFlownet")
    full = cls == "MaskFlownet"
    net = (training.MaskFlownetTrainable if full else training.MaskFlownetSTrainable)(net_mod.random_params(0, full=full)).to(device)
    training.load_checkpoint(params_path[:-len(".params")], net)
    return net, full


KITTI_VALID_SHAPE = (370, 1224)       # main.py:176
SINTEL_PREDICT_SIZE = (448, 1024)     # predict.py:10
KITTI_PREDICT_SIZE = (512, 1152)      # predict.py:44


def validation_sets(data, device, samples=-1):
    """The sets of the --valid mode (main.py:166-184): every Sintel pass of 'training2' and 'training', KITTI 2012 and 2015 (all pairs)
    resized to 370 x 1224 -- the reference hands its (370, 1224) to cv2.resize, which reads it as (width, height); here it is (H, W),
    the size its comment and every other call mean.  Sets whose data-file entry is missing are left out."""
    from .data import DeviceDataset
    sets = {}
    if isinstance(data.get("sintel"), dict):
        for div in ("training2", "training"):
            for subset, ds in _sintel_sets(data, device, div, samples).items():
                sets["sintel.%s.%s" % (div, subset)] = ds
    for edition in ("2012", "2015"):
        if isinstance(data.get("kitti"), dict) and isinstance(data["kitti"].get(edition), dict):
            sets["kitti." + edition] = _kitti_set(DeviceDataset(device), data, edition, "mixed", KITTI_VALID_SHAPE[::-1], samples)
    return sets


def validate_checkpoint(network_cfg, data, root, checkpoint, network=None, batch=8, resize=None, device="cuda:0", screen=True):
    """--valid (main.py:163-187): the checkpoint's net on validation_sets(data), logged to root/logs/val/<run_id>.val.log as
    'steps=N, <set>:epe=V' and, for KITTI, also 'steps=N, <set>:kitti=V'.  One Validation.run(kitti=True) yields both KITTI figures;
    the reference runs each KITTI set twice.  -> {set: {"epe", "fl"}}."""
    from . import training
    _, rid, params, steps = resolve_checkpoint(root, checkpoint)
    net, full = _build_net(network_cfg, network, params, device)
    os.makedirs(os.path.join(root, "logs", "val"), exist_ok=True)
    log = RunLog(os.path.join(root, "logs", "val", rid + ".val.log"), screen=screen)
    result = training.Validation(validation_sets(data, device), batch, full=full, resize=resize).run(net, kitti=True)
    for name, r in result.items():
        log.log("steps={}, {}:epe={}".format(steps, name, r["epe"]))
        if name.startswith("kitti."):
            log.log("steps={}, {}:kitti={}".format(steps, name, r["fl"]))
    log.close()
    return result


def kitti_test_pairs(image_dir):
    """How many pairs %06d_10.png / %06d_11.png, counted from 0 without a gap, a KITTI testing directory holds (the reference takes
    (len(os.listdir) - 1) // 2, one fewer than a directory of nothing but pairs holds)."""
    n = 0
    while all(os.path.exists(os.path.join(image_dir, "%06d_%d.png" % (n, t))) for t in (10, 11)):
        n += 1
    return n


def predict_checkpoint(network_cfg, data, root, checkpoint, network=None, resize=None, device="cuda:0"):
    """--predict (predict.py:8-66), batch 1 through predict.Predictor.  Sintel test/final: the network runs at 448 x 1024 (or `resize`)
    and the flow of every pair, at the frames' own size, goes to root/flows/<ckpt>_sintel/final/<sequence>/frame_XXXX.flo.  KITTI
    testing, both editions: the frames are resized on the device to 512 x 1152 (ops.cv_resize_u8; (H, W) -- the reference hands the pair
    to cv2.resize as (width, height)) in cv2.imread's BGR order, and the flow at that size goes to <ckpt>_kitti/<edition>/%06d_10.png
    in KITTI's 16-bit format (io.write_kitti_flow).  -> the list of files written."""
    import torch
    from . import io, ops, readers
    from .predict import Predictor
    _, rid, params_path, steps = resolve_checkpoint(root, checkpoint)
    cls = network or getattr(network_cfg.network, "class").get("MaskFlownet")
    full = cls == "MaskFlownet"
    params = io.load_params(params_path)
    name = os.path.basename(params_path)[:-len(".params")]
    prefix = os.path.join(root, "flows", name)
    written, predictors = [], {}

    def flow_of(a, b, size):
        """(u, v) flow (H,W,2) of two uint8 (H,W,3) device frames, the network at `size`."""
        key = (tuple(a.shape[:2]), tuple(size))
        if key not in predictors:
            predictors[key] = Predictor(params, 1, a.shape[0], a.shape[1], full=full, resize=size, device=device)
        out = predictors[key].do_batch_u8(torch.stack([a, b]), 0, 1, 1, warped=False)
        return np.ascontiguousarray(np.flip(out["flow"][0].cpu().numpy().transpose(1, 2, 0), axis=-1))

    if isinstance(data.get("sintel"), dict):
        sroot = _need(data, "sintel", "root")
        size = tuple(resize) if resize else SINTEL_PREDICT_SIZE
        entries = readers.sintel_entries(sroot, None, parts=("test",), subsets=("final",))["test"]["final"]
        for (seq, i), (a, b) in zip(entries, readers.sintel_test_pairs(sroot, "final", entries)):
            folder = os.path.join(prefix + "_sintel", "final", seq)
            os.makedirs(folder, exist_ok=True)
            a, b = (torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in (a, b))
            written.append(os.path.join(folder, "frame_%04d.flo" % i))
            io.write_flo(written[-1], flow_of(a, b, size))
    size = tuple(resize) if resize else KITTI_PREDICT_SIZE
    for edition in ("2012", "2015"):
        if not (isinstance(data.get("kitti"), dict) and isinstance(data["kitti"].get(edition), dict) and data["kitti"][edition].get("testing")):
            continue
        image_dir = data["kitti"][edition]["testing"]
        folder = os.path.join(prefix + "_kitti", edition)
        os.makedirs(folder, exist_ok=True)
        for k in range(kitti_test_pairs(image_dir)):
            raw = [io.read_png(os.path.join(image_dir, "%06d_%d.png" % (k, t)))[..., 2::-1] for t in (10, 11)]
            a, b = (ops.cv_resize_u8(torch.from_numpy(np.ascontiguousarray(x)).to(device), size) for x in raw)
            written.append(os.path.join(folder, "%06d_10.png" % k))
            io.write_kitti_flow(written[-1], flow_of(a, b, size))
    return written
