"""Times the assembly of a training batch on the GPU, at the shapes the reference trains at: data.Feeder.next() (the draws, one table
upload, one launch of batch_gather_kernel), the kernel alone (ops.batch_gather on a fixed table into fixed outputs), a torch
device-to-device copy_ that moves the same number of bytes, and the host path a user has without the feature: the numpy statement of
main.py:466-486 (crop, transpose, flip, negate, stack) on host arrays plus the upload of the four arrays.

    python tools/batch_gather_time.py [--iters 100 --windows 7 --host-iters 15] [--json PATH]

Device events around windows of --iters back-to-back calls, the variants alternating window by window; the median window with the
fastest and the slowest.  The host path is a host clock around work that ends in a device synchronise.  Bytes are the algorithm's: per
output pixel 3 + 3 + (8 or 4) + (1 where the source has a mask) read, 3 + 3 + 8 + (1 in a call with a mask) written, from the shapes.
The copy_ is of half that count (a copy reads and writes each byte), so that it moves the same total.  Prints a markdown report."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maskflownet_amd import data, ops  # noqa: E402

PEAK = 8e12   # bytes / s

# name, N, crop, source size, label dtype, mask, samples held
WORKLOADS = [
    ("chairs: N=8, 384x512 uncropped, fp32, no mask", 8, (384, 512), (384, 512), "float32", False, 16),
    ("sintel: N=4, 436x1024 of 436x1024, fp32, mask", 4, (436, 1024), (436, 1024), "float32", True, 8),
    ("sintel: N=4, 436x1024 of 436x1024, fp16, mask", 4, (436, 1024), (436, 1024), "float16", True, 8),
    ("mixed:  N=4, 436x1024 of 448x1100, fp32, mask", 4, (436, 1024), (448, 1100), "float32", True, 8),
    ("mixed:  N=4, 436x1024 of 448x1100, fp16, mask", 4, (436, 1024), (448, 1100), "float16", True, 8),
]


def windows(variants, iters, nwin, warm=5):
    """{name: [us per call of each window]}; the variants alternate window by window."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(nwin):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / iters)
    return out


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}


def host_batch(samples, crop, draw, with_mask):
    """main.py:466-486 in numpy on host arrays: -> img1, img2, label, mask or None."""
    Hc, Wc = crop
    rows = []
    for (i, y0, x0, flip) in draw:
        arrs = [a for a in samples[i] if a is not None]
        cut = [np.transpose(a[y0:y0 + Hc, x0:x0 + Wc], (2, 0, 1)) for a in arrs]
        if flip:
            cut = [a[:, :, ::-1] for a in cut]
            cut[2] = np.stack([-cut[2][0, :, :], cut[2][1, :, :]], axis=0)
        rows.append(cut)
    out = [np.stack(x, axis=0) for x in zip(*rows)]
    out[2] = out[2].astype("float32")                       # pipeline.py:99
    return out if with_mask else out[:3] + [None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host-iters", type=int, default=15)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    rng = np.random.default_rng(0)
    results = []
    for name, N, crop, (Hs, Ws), kind, mask, held in WORKLOADS:
        samples = []
        ds = data.DeviceDataset("cuda", flow_dtype=kind)
        for _ in range(held):
            s = (rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8), rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8),
                 (rng.standard_normal((Hs, Ws, 2)) * 10).astype(kind), rng.integers(0, 2, (Hs, Ws, 1), dtype=np.uint8) * 255 if mask else None)
            samples.append(s)
            ds.append(*s)
        sampler = data.BatchSampler([ds] * N, crop, seed=1)
        feed = data.Feeder(sampler)
        batch = feed.next()
        # the feeder's batch is the host statement's on the same draw, bit for bit, at the size that is timed
        want = host_batch(samples, crop, feed.last_draw, mask)
        for g, w in zip(batch, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert (g.cpu().numpy().reshape(-1).view(np.uint8) == np.ascontiguousarray(w).reshape(-1).view(np.uint8)).all(), name
        rows = ops.batch_gather_rows([ds.sample(d[0]) for d in feed.last_draw], crop, [(d[1], d[2]) for d in feed.last_draw],
                                     [d[3] for d in feed.last_draw])
        outs = list(batch)
        px = N * crop[0] * crop[1]
        nbytes = px * ((6 + (8 if kind == "float32" else 4) + (1 if mask else 0)) + (6 + 8 + (1 if mask else 0)))
        src, dst = (torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        dev = windows({"Feeder.next()": feed.next, "batch_gather_kernel alone": lambda: ops.batch_gather(rows, crop, mask, out=outs),
                       "torch copy_, same bytes moved": lambda: dst.copy_(src)}, a.iters, a.windows)
        # the host path: the draws, the numpy statement, the upload, a synchronise
        host_sampler = data.BatchSampler([ds] * N, crop, seed=1)
        host_ms = []
        for k in range(a.host_iters + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            up = [None if t is None else torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in host_batch(samples, crop, host_sampler.draw(), mask)]
            torch.cuda.synchronize()
            if k >= 2:
                host_ms.append((time.perf_counter() - t0) * 1e3)
            del up
        results.append({"workload": name, "bytes": nbytes, "device": {k: summary(v) for k, v in dev.items()},
                        "host_ms": {"median": statistics.median(host_ms), "min": min(host_ms), "max": max(host_ms)}})
        del ds, feed, rows, outs, batch, src, dst
    print("## Batch assembly: %d windows of %d calls, us per call: median (min - max); host path: %d batches, ms\n" % (a.windows, a.iters, a.host_iters))
    print("| workload | MB read + written | Feeder.next() us | kernel alone us | kernel TB/s | of 8 TB/s | copy_ of the same bytes us | copy_ TB/s | "
          "kernel / copy_ rate | host numpy + upload ms |\n|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        f, k, c = (r["device"][n] for n in ("Feeder.next()", "batch_gather_kernel alone", "torch copy_, same bytes moved"))
        rate = lambda v: r["bytes"] / v["median_us"] / 1e6
        print("| %s | %.1f | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.2f | %.3f | %.1f (%.1f - %.1f) | %.2f | %.2f | %.1f (%.1f - %.1f) |" % (
            r["workload"], r["bytes"] / 1e6, f["median_us"], f["min_us"], f["max_us"], k["median_us"], k["min_us"], k["max_us"], rate(k),
            rate(k) * 1e12 / PEAK, c["median_us"], c["min_us"], c["max_us"], rate(c), rate(k) / rate(c), r["host_ms"]["median"], r["host_ms"]["min"],
            r["host_ms"]["max"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
