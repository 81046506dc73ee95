"""Times the multiscale training loss on the GPU, forward + backward: training.FusedMultiscaleEpe (kernels/loss.h, two launches
forward, one per scale backward) against training.MultiscaleEpe, the composition of mfn_upsample_fwd / _bwd and torch
element-wise and reduction kernels under torch autograd -- for the sqrt form (q None) and the robust form (q 0.4).

Device events around windows of --iters back-to-back rounds, --windows windows per variant, the variants alternating; the median
window is reported with the fastest and the slowest.  A round is: loss = module(label, mask, *preds); loss.sum().backward(), the five
predictions being leaves whose .grad is dropped between rounds.  The fused entries are also timed one by one (the forward's two
launches; each scale's backward launch, through req = null for the others) with their algorithmic bytes (kernels/loss.h: label and mask
once, 12 N H W, plus the prediction read / its gradient written) and the fraction of 8 TB/s those bytes are.

    python tools/loss_time.py [--batch 8 --shape 384 512] [--json PATH]

Prints a markdown report.  MFN_HIP_SO selects a measurement build of the library (maskflownet_amd/_lib.py)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maskflownet_amd import ops, training  # noqa: E402

PEAK = 8e12   # bytes / s


def windows(variants, iters, nwin, warm=10):
    """{name: [us per round of each window]}; the variants alternate window by window."""
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shape", type=int, nargs=2, default=(384, 512))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    N, (H, W) = a.batch, a.shape
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    scales, weights = training.MultiscaleEpe().scales, training.MultiscaleEpe().weights
    label = 4 * torch.randn((N, 2, H, W), device=dev, generator=g)
    mask = (torch.rand((N, 1, H, W), device=dev, generator=g) > 0.1).float()
    preds = [(4 * torch.randn((N, 2, H // f, W // f), device=dev, generator=g)).requires_grad_(True) for f in scales]

    def round_of(mod):
        def fn():
            for p in preds:
                p.grad = None
            mod(label, mask, *preds).sum().backward()
        return fn

    res = {"shape": {"N": N, "H": H, "W": W, "scales": list(scales)}, "library": os.environ.get("MFN_HIP_SO") or "shipped build",
           "iters": a.iters, "windows": a.windows, "forward_backward": {}, "agreement": {}, "kernels": {}}
    for form, q in (("sqrt", None), ("robust q=0.4", 0.4)):
        fused, comp = training.FusedMultiscaleEpe(q=q), training.MultiscaleEpe(q=q)
        got = {}
        for name, mod in (("fused", fused), ("composed", comp)):        # the two agree (losses; gradients relative to the largest element)
            round_of(mod)()
            got[name] = (mod(label, mask, *preds).detach(), [p.grad.clone() for p in preds])
        res["agreement"][form] = {"loss max rel diff": float(((got["fused"][0] - got["composed"][0]).abs() / got["composed"][0].abs()).max()),
                                  "gradient max diff / max |gradient|": max(float((x - y).abs().max() / y.abs().max())
                                                                             for x, y in zip(got["fused"][1], got["composed"][1]))}
        w = windows({"FusedMultiscaleEpe": round_of(fused), "MultiscaleEpe (composed)": round_of(comp)}, a.iters, a.windows)
        res["forward_backward"][form] = {k: summary(v) for k, v in w.items()}

        # the fused entries one by one
        dp = [p.detach() for p in preds]
        _, sums = ops.multiscale_epe(dp, label, mask, scales, weights, 1e-8, q)
        gloss = torch.ones(N, device=dev)
        outs = [torch.empty_like(p) for p in dp]
        variants = {"forward (partial + final)": lambda: ops.multiscale_epe(dp, label, mask, scales, weights, 1e-8, q)}
        nbytes = {"forward (partial + final)": 12 * N * H * W + sum(p.numel() * 4 for p in dp)}
        for i, f in enumerate(scales):
            reqs = ["write" if j == i else "null" for j in range(len(scales))]
            out = [o if j == i else None for j, o in enumerate(outs)]
            key = "backward f = %d" % f
            variants[key] = (lambda r=reqs, o=out: ops.multiscale_epe_backward(gloss, dp, label, mask, scales, weights, sums, 1e-8, q, reqs=r, out=o))
            nbytes[key] = 12 * N * H * W + 2 * dp[i].numel() * 4
        variants["backward, all scales"] = lambda: ops.multiscale_epe_backward(gloss, dp, label, mask, scales, weights, sums, 1e-8, q, out=outs)
        nbytes["backward, all scales"] = sum(nbytes["backward f = %d" % f] for f in scales)
        w = windows(variants, a.iters, max(3, a.windows // 2))
        res["kernels"][form] = {k: dict(summary(v), bytes=nbytes[k]) for k, v in w.items()}

    print("## multiscale loss, forward + backward, N = %d, %d x %d, scales %s, %s; %d windows of %d rounds, us per round: median (min - max)\n"
          % (N, H, W, list(scales), res["library"], a.windows, a.iters))
    print("| form | variant | us |\n|---|---|---|")
    for form, d in res["forward_backward"].items():
        for k, v in d.items():
            print("| %s | %s | %.1f (%.1f - %.1f) |" % (form, k, v["median_us"], v["min_us"], v["max_us"]))
    print("\n| form | fused entry | us | algorithmic bytes | TB/s | of 8 TB/s |\n|---|---|---|---|---|---|")
    for form, d in res["kernels"].items():
        for k, v in d.items():
            print("| %s | %s | %.1f (%.1f - %.1f) | %.1f MB | %.2f | %.3f |" % (form, k, v["median_us"], v["min_us"], v["max_us"], v["bytes"] / 1e6,
                                                                              v["bytes"] / v["median_us"] / 1e6, v["bytes"] / v["median_us"] * 1e6 / PEAK))
    for form, d in res["agreement"].items():
        print("\nfused against composed, %s: " % form + ", ".join("%s %.3g" % kv for kv in d.items()))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
