"""Times the trainer's update on the GPU over the parameter set of MaskFlownet-S (142 tensors, 10.5 M parameters): training.Trainer.step
-- one launch of mfn_multi_adam_update (kernels/optimizer.h), the 1 / batch_size inside it -- against the step train_step composes for a
torch optimizer: the bucket scale (GradientBuckets.finish: one mul_ per bucket), or without buckets one mul_ per gradient, then
torch.optim.Adam.step().  The gradients are fixed random values; no forward or backward runs.

Device events around windows of --iters back-to-back steps, --windows windows per variant, the variants alternating; the median window
is reported with the fastest and the slowest.  The kernel alone (ops.multi_adam_update on the trainer's table, no Python around it but
the call) is timed the same way, with its 28 bytes per parameter as a fraction of 8 TB/s.  --other-so PATH times the same kernel of a
second build of the library in the same process, window by window next to the shipped one: the measurement of MFN_ADAM_NT (the
non-temporal accesses to mean and var against plain ones) builds that library with -DMFN_ADAM_NT=0 or =1.

    python tools/optimizer_time.py [--iters 200 --windows 9] [--other-so PATH --other-name plain] [--json PATH]

Prints a markdown report."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maskflownet_amd import _abi, _lib, network, ops, training  # noqa: E402

PEAK = 8e12   # bytes / s


def windows(variants, iters, nwin, warm=5):
    """{name: [us per step of each window]}; the variants alternate window by window."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--other-so", default=None)
    ap.add_argument("--other-name", default="other build")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    P = network.random_params(0)
    g = torch.Generator(device="cuda").manual_seed(0)

    def fresh():
        return training.MaskFlownetSTrainable(P).cuda()

    # the fused step
    net_f = fresh()
    tr = training.Trainer(training.reference_named_parameters(net_f), "adam", {"learning_rate": 1e-4})
    for b in tr.buckets.buckets:
        b.copy_(1e-3 * torch.randn(b.shape, device="cuda", generator=g))
    n_params = sum(p.numel() for p in tr.params)
    # the composed steps: with buckets (one scale per bucket) and without (one per gradient), then torch's Adam
    net_b = fresh()
    gb = training.GradientBuckets(list(net_b.parameters()))
    opt_b = torch.optim.Adam(net_b.parameters(), lr=1e-4)
    for b in gb.buckets:
        b.copy_(1e-3 * torch.randn(b.shape, device="cuda", generator=g))
    net_p = fresh()
    opt_p = torch.optim.Adam(net_p.parameters(), lr=1e-4)
    for p in net_p.parameters():
        p.grad = 1e-3 * torch.randn(p.shape, device="cuda", generator=g)
    inv = 1.0 / a.batch

    def composed_buckets():
        gb.finish(a.batch)
        opt_b.step()

    def composed_plain():
        for p in net_p.parameters():
            p.grad.mul_(inv)
        opt_p.step()

    steps = windows({"Trainer.step (fused)": lambda: tr.step(a.batch), "bucket scale + torch.optim.Adam": composed_buckets,
                     "142 mul_ + torch.optim.Adam": composed_plain}, a.iters, a.windows)
    # the kernel alone, the shipped build and (optionally) a second build on the same table
    table, hp = tr._table, (tr.lr_t(), 0.9, 0.999, 1e-8, 0.0, inv, -1.0)
    kernels = {"multi_adam_update (shipped build)": lambda: ops.multi_adam_update(table, *hp)}
    if a.other_so:
        other = ops.OpSet(_abi.bind(ctypes.CDLL(os.path.abspath(a.other_so)), "mfn_", product=True), ops.TorchAdapter(), _lib.check)
        kernels["multi_adam_update (%s)" % a.other_name] = lambda: other.multi_adam_update(table, *hp)
    kern = windows(kernels, a.iters, a.windows)
    nbytes = 28 * n_params
    res = {"tensors": len(tr.params), "parameters": n_params, "bytes": nbytes, "blocks": table.n_blocks, "iters": a.iters, "windows": a.windows,
           "steps": {k: summary(v) for k, v in steps.items()}, "kernel": {k: summary(v) for k, v in kern.items()}}
    print("## Adam step over MaskFlownet-S: %d tensors, %d parameters, %.1f MB moved (28 bytes per parameter), %d blocks; %d windows of %d "
          "steps, us per step: median (min - max)\n" % (len(tr.params), n_params, nbytes / 1e6, table.n_blocks, a.windows, a.iters))
    print("| step | us |\n|---|---|")
    for k, v in res["steps"].items():
        print("| %s | %.1f (%.1f - %.1f) |" % (k, v["median_us"], v["min_us"], v["max_us"]))
    print("\n| kernel alone | us | TB/s | of 8 TB/s |\n|---|---|---|---|")
    for k, v in res["kernel"].items():
        print("| %s | %.1f (%.1f - %.1f) | %.2f | %.3f |" % (k, v["median_us"], v["min_us"], v["max_us"], nbytes / v["median_us"] / 1e6,
                                                           nbytes / v["median_us"] * 1e6 / PEAK))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
