"""Times run.TrainingRun.step() against a hand-written loop of Feeder.next() + training.train_batch() over the SAME objects, at the
reference's Chairs shapes: batch 8, 384x512 cropped to 320x448, MaskFlownet_S, on a synthetic Chairs tree written to a temporary directory.

    python tools/train_loop_time.py [--json PATH]

Five windows each, alternating.  A window is 200 steps on which the loop neither logs, validates nor writes a checkpoint; every fiftieth
step logs, so a window is four segments of 49 steps and one of 4, each between two device synchronisations, with the logged step run
untimed between segments (the bare loop runs one untimed step there too).  Then the cost of one validation of 8 samples, one checkpoint
and one logged step.  Prints one JSON object."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maskflownet_amd import config, io, run, training  # noqa: E402

import argparse  # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None, help="also write the result here")
args = ap.parse_args()
base = tempfile.mkdtemp()
rng = np.random.default_rng(0)
H, W = 384, 512
os.makedirs(os.path.join(base, "chairs"))
split = [1] * 16 + [2] * 8
for k in range(1, len(split) + 1):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    b = 127 + 60 * np.sin(xx / 9.0)[..., None] + 50 * np.cos(yy / 7.0)[..., None] + rng.uniform(-15, 15, (H, W, 3))
    for name, img in (("img1", b), ("img2", np.roll(b, 2, axis=1))):
        with open(os.path.join(base, "chairs", "%05d_%s.ppm" % (k, name)), "wb") as f:
            f.write(b"P6 %d %d 255\n" % (W, H))
            f.write(np.clip(img, 0, 255).astype(np.uint8).tobytes())
    io.write_flo(os.path.join(base, "chairs", "%05d_flow.flo" % k),
                 (np.stack([np.full((H, W), 2.0), np.zeros((H, W))], -1) + rng.standard_normal((H, W, 2)) * 0.25).astype(np.float32))
with open(os.path.join(base, "split.txt"), "w") as f:
    f.write("".join("%d\n" % v for v in split))
import yaml  # noqa: E402
net_cfg, ds_cfg = os.path.join(base, "net.yaml"), os.path.join(base, "ds.yaml")
yaml.safe_dump({"optimizer": {"learning_rate": [[10 ** 6, 1e-4]]}, "network": {"class": "MaskFlownet_S"}}, open(net_cfg, "w"))
yaml.safe_dump({"dataset": "chairs", "validation_steps": 10 ** 6, "checkpoint_steps": 10 ** 6, "target_shape": [320, 448]}, open(ds_cfg, "w"))
data = {"chairs": {"root": os.path.join(base, "chairs"), "split": os.path.join(base, "split.txt")}}

r = run.TrainingRun(config.load(net_cfg), config.load(ds_cfg), data, os.path.join(base, "root"), seed=0, batch=8)
assert r.batch_size == 8 and r.target_shape == [320, 448]


def bare_step():
    img1, img2, label, mask = r.feeder.next()
    training.train_batch(r.net, r.loss_fn, r.trainer, img1, img2, label, mask, r.geo_aug, r.color_aug)


def timed(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def loop_segment(n):
    for _ in range(n):
        assert not r.policy.logs(r.steps + 1) and not r.policy.validates(r.steps + 1)
    return timed(r.step, n)


def to_next_segment():
    """Run (untimed) up to and including the next logged step."""
    while True:
        r.step()
        if r.steps % 50 == 0:
            return


for _ in range(20):      # steps 1..20: logged, step 1 validates; also the warm-up of every plan
    r.step()
print("warm-up done at step", r.steps, flush=True)
to_next_segment()         # step 50
windows = {"run_loop": [], "bare_loop": []}
for w in range(5):
    for kind in ("run_loop", "bare_loop"):
        total = 0.0
        for seg in (49, 49, 49, 49, 4):
            if kind == "run_loop":
                total += loop_segment(seg)
                to_next_segment()
            else:
                total += timed(bare_step, seg)
                bare_step()      # the untimed step between segments, as the run loop has its logged one
        windows[kind].append(total)
        print(kind, w, "%.4f s / 200 steps = %.3f ms per step" % (total, total * 5), flush=True)

torch.cuda.synchronize()
t = time.perf_counter(); r._validate(); torch.cuda.synchronize(); first_val = time.perf_counter() - t
vals = []
for _ in range(3):
    t = time.perf_counter(); r._validate(); torch.cuda.synchronize(); vals.append(time.perf_counter() - t)
saves = []
for k in range(3):
    t = time.perf_counter(); r.save(os.path.join(base, "root", "weights", "probe_%d" % k)); saves.append(time.perf_counter() - t)
logged = []
for _ in range(3):        # a logged step: the step plus the read of its EPE and the line
    while (r.steps + 1) % 50:
        r.step()
    logged.append(timed(r.step, 1))
result = {"windows_s_per_200_steps": windows, "validation_8_samples_s": vals, "validation_after_training_steps_first_s": first_val,
          "checkpoint_s": saves, "logged_step_s": logged, "steps": r.steps, "device": torch.cuda.get_device_name(0)}
r.close()
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps(result))
