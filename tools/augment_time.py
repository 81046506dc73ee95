"""Times the augmentation of a training batch on the GPU: the library's launches (augment_geometry, augment_color_mean,
augment_color) against the same result composed from the operators the package had before them -- GridGenerator(affine) +
BilinearSampler twice, torch element-wise glue, torch.randn -- as augmentation.py:295-338 and :213-225 compose it.

Device events around windows of --iters back-to-back rounds, --windows windows per variant, the variants alternating; the median
window is reported with the fastest and the slowest.  The tables are uploaded once, outside the windows, for both variants.
Bytes (kernels/augment.h): geometry 4 N (9 Ho Wo + 9 Ht Wt); colour mean 4 * 2N * 3 H W read; colour the same read and written.

    python tools/augment_time.py [--batch 8 --orig 384 512 --target 320 448] [--json PATH]

Prints a markdown report.  MFN_HIP_SO selects a measurement build of the library (maskflownet_amd/_lib.py)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maskflownet_amd import _lib, augment, ops  # noqa: E402

PEAK = 8e12   # bytes / s


def windows(variants, iters, nwin, warm=20):
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
    ap.add_argument("--orig", type=int, nargs=2, default=(384, 512))
    ap.add_argument("--target", type=int, nargs=2, default=(320, 448))
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    N, (Ho, Wo), (Ht, Wt) = a.batch, a.orig, a.target
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    im1, im2 = (torch.rand((N, 3, Ho, Wo), device=dev, generator=g) for _ in range(2))
    flow = 4 * torch.randn((N, 2, Ho, Wo), device=dev, generator=g)
    mask = torch.ones((N, 1, 1, 1), device=dev)
    geo, col = augment.presets("chairs", N, (Ho, Wo), (Ht, Wt), seed=0)
    gtab_h, ctab_h = geo.table(), col.table(col.draw())
    gtab, ctab = (torch.from_numpy(t).to(dev) for t in (gtab_h, ctab_h))
    sigma, seed = 0.03, col.seed

    # ---- the library ---------------------------------------------------------------------------------------------------------------
    def lib_geometry():
        return ops.augment_geometry(im1, im2, flow, mask, gtab, (Ht, Wt), label_order=1)

    g1, g2, gl, gm = lib_geometry()

    def lib_mean():
        return ops.augment_color_mean(g1, g2, ctab, sigma, seed, 5)

    mean = lib_mean()

    def lib_color():
        return ops.augment_color(g1, g2, ctab, sigma, seed, 5, mean=mean)

    def lib_all():
        o1, o2, lab, m = ops.augment_geometry(im1, im2, flow, mask, gtab, (Ht, Wt), label_order=1)
        return ops.augment_color(o1, o2, ctab, sigma, seed, 5), lab, m

    def lib_all_centralize():   # with the consumer of the colour kernel's output behind it, as training.augment_batch runs them
        both, lab, m = lib_all()
        return ops.preprocess_pair(both[:N], both[N:], Ht, Wt, mean=ops.pair_mean(both[:N], both[N:])), lab, m

    # ---- the composition from the earlier operators ----------------------------------------------------------------------------------
    t = gtab
    theta1, theta2 = t[:, 0:6].contiguous(), t[:, 6:12].contiguous()
    rt = t[:, 14:16, None, None]
    shift = t[:, 16:18, None, None]
    inv2, fac = t[:, 18:22].reshape(N, 2, 2), t[:, 22:26].reshape(N, 2, 2)
    ident = ops.GridGenerator(torch.tensor([[1., 0, 0, 0, 1, 0]], device=dev), "affine", (Ht, Wt)).reshape(1, 2, -1).expand(N, 2, -1).contiguous()
    c = ctab
    M, cc, ch, br = c[:, 0:9].reshape(N, 3, 3), c[:, 9:12, None, None], c[:, 12:15, None, None], c[:, 15, None, None, None]
    mask_plane = mask.expand(N, 1, Ho, Wo)

    def comp_geometry():
        grid = ops.GridGenerator(theta1, "affine", (Ht, Wt))
        ft = torch.relu(grid.amax((2, 3), keepdim=True) - 1) - torch.relu(-1 - grid.amin((2, 3), keepdim=True))
        grid = (grid - ft).clamp(-1, 1)
        s = ops.BilinearSampler(torch.cat([im1, mask_plane, (flow - shift) * mask_plane], 1), grid)
        m = s[:, 3:4]
        f = s[:, 4:6] / m.clamp(min=1e-8)
        grid2 = ops.GridGenerator(theta2, "affine", (Ht, Wt)) - ft + rt
        o2 = ops.BilinearSampler(im2, grid2)
        lab = torch.baddbmm(torch.bmm(fac, ident), inv2, f.reshape(N, 2, -1)).reshape(N, 2, Ht, Wt).flip(1)
        return s[:, :3].contiguous(), o2, lab, m.contiguous()

    def comp_color_one(img):
        x = torch.bmm(M, img.reshape(N, 3, -1)).reshape(N, 3, Ht, Wt) + torch.randn((N, 3, Ht, Wt), device=dev) * sigma
        mu = x.mean((2, 3), keepdim=True)
        return ((x - mu) * cc + (mu * ch + br)).clamp(0, 1)

    def comp_color():
        return torch.cat([comp_color_one(g1), comp_color_one(g2)], 0)

    def comp_all():
        o1, o2, lab, m = comp_geometry()
        return torch.cat([comp_color_one(o1), comp_color_one(o2)], 0), lab, m

    # ---- the two agree (sigma = 0 for this: the two noise generators differ) -----------------------------------------------------------
    sigma, keep = 0.0, sigma
    (lb, ll, lm), (cb, cl, cm) = lib_all(), comp_all()
    agree = {"images": float((lb - cb).abs().max()), "mask": float((lm - cm).abs().max()),
             "flow (median |diff|)": float((ll - cl).abs().median()), "flow (max |diff|)": float((ll - cl).abs().max())}
    sigma = keep

    res = {"shape": {"N": N, "orig": [Ho, Wo], "target": [Ht, Wt]}, "library": os.environ.get("MFN_HIP_SO") or "shipped build",
           "iters": a.iters, "windows": a.windows, "agreement_sigma0": agree}
    by = {"augment_geometry": 4 * N * 9 * (Ho * Wo + Ht * Wt), "augment_color_mean (2 launches)": 4 * 2 * N * 3 * Ht * Wt,
          "augment_color": 2 * 4 * 2 * N * 3 * Ht * Wt}
    w = windows({"augment_geometry": lib_geometry, "augment_color_mean (2 launches)": lib_mean, "augment_color": lib_color,
                 "composition: geometry": comp_geometry, "composition: colour": comp_color}, a.iters, a.windows)
    res["stages"] = {k: dict(summary(v), bytes=by.get(k)) for k, v in w.items()}
    w = windows({"library: geometry + mean + colour": lib_all, "composition: all": comp_all}, a.iters, a.windows)
    res["whole"] = {k: summary(v) for k, v in w.items()}
    res["store_policy"] = {}
    for pol in (-1, 0, 1, 2):
        _lib.set_tuning(store_policy=pol)
        w = windows({"augment_geometry": lib_geometry, "augment_color": lib_color, "geometry + mean + colour": lib_all,
                     "... + pair_mean + preprocess_pair": lib_all_centralize}, a.iters, max(3, a.windows // 2))
        res["store_policy"][str(pol)] = {k: summary(v) for k, v in w.items()}
    _lib.set_tuning(store_policy=-1)

    print("## N = %d, %d x %d -> %d x %d, %s; %d windows of %d rounds, us per round: median (min - max)\n" % (N, Ho, Wo, Ht, Wt, res["library"], a.windows, a.iters))
    print("| stage | us | bytes | TB/s | of 8 TB/s |\n|---|---|---|---|---|")
    for k, v in res["stages"].items():
        bw = ("%.1f MB | %.2f | %.2f" % (v["bytes"] / 1e6, v["bytes"] / v["median_us"] / 1e6, v["bytes"] / v["median_us"] * 1e6 / PEAK)) if v["bytes"] else "- | - | -"
        print("| %s | %.1f (%.1f - %.1f) | %s |" % (k, v["median_us"], v["min_us"], v["max_us"], bw))
    print("\n| whole | us |\n|---|---|")
    for k, v in res["whole"].items():
        print("| %s | %.1f (%.1f - %.1f) |" % (k, v["median_us"], v["min_us"], v["max_us"]))
    print("\n| store.policy | " + " | ".join(next(iter(res["store_policy"].values()))) + " |\n|---|---|---|---|---|")
    for pol, d in res["store_policy"].items():
        print("| %s | " % pol + " | ".join("%.1f (%.1f - %.1f)" % (v["median_us"], v["min_us"], v["max_us"]) for v in d.values()) + " |")
    print("\nlibrary against composition at sigma = 0, max |difference|: " + ", ".join("%s %.3g" % kv for kv in agree.items()))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
