"""Times the ingest of one KITTI and one HD1K sample on the GPU (kernels/ingest.h): the kernels that turn the uploaded raw arrays into
the stored sample -- mfn_ingest_minmax (HD1K only), mfn_ingest_image twice, mfn_ingest_flow_occ -- against that sample's own
host-to-device copy (two uint8 images and the uint16 flow map from pinned memory), in the same session.  The condition the path was
built to: the kernels of a sample take less time than its copy, so ingest stays upload-bound.

    KITTI  375 x 1242, crop (370, 1224), no resize                              (main.py:325: kitti.read_dataset(..., crop = (370, 1224)))
    KITTI  375 x 1242 -> 436 x 1024                                             (main.py:251: kitti.read_dataset(resize = (1024, 436)))
    HD1K   1080 x 2560, margins (50, 100), stretch, premultiply -> 436 x 1024   (main.py:258: hd1k.read_dataset(resize = (1024, 436)))

Device events around windows of --iters back-to-back rounds, --windows windows per variant, the variants alternating; the median window
is reported with the fastest and the slowest.  Tables are uploaded once, outside the windows.  Bytes (the least the algorithm moves):
every window byte read once (twice for the images with the stretch: the min/max pass), every stored byte written once.

    python tools/ingest_time.py [--iters 200 --windows 7] [--json PATH]

Prints a markdown report."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maskflownet_amd import ops  # noqa: E402

PEAK = 8e12   # bytes / s of HBM

WORKLOADS = {
    "KITTI 375x1242 -> 370x1224": dict(raw=(375, 1242), window=(5, 0, 370, 1224), dst=(370, 1224), premultiply=False, normalize=False),
    "KITTI 375x1242 -> 436x1024": dict(raw=(375, 1242), window=(0, 0, 375, 1242), dst=(436, 1024), premultiply=False, normalize=False),
    "HD1K 1080x2560 -> 436x1024": dict(raw=(1080, 2560), window=(50, 100, 980, 2360), dst=(436, 1024), premultiply=True, normalize=True),
}


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


def measure(name, w, flow_dtype, iters, nwin):
    H, W = w["raw"]
    y0, x0, h, wd = w["window"]
    Hd, Wd = w["dst"]
    rng = np.random.default_rng(0)
    pad16 = lambda n: (n + 15) & ~15
    img_bytes, fo_bytes = H * W * 3, H * W * 6
    offs = [0, pad16(img_bytes), 2 * pad16(img_bytes)]
    total = offs[2] + pad16(fo_bytes)
    stage = torch.zeros(total, dtype=torch.uint8).pin_memory()
    host = stage.numpy()
    host[:img_bytes] = rng.integers(0, 256, img_bytes, dtype=np.uint8)
    host[offs[1]:offs[1] + img_bytes] = rng.integers(0, 256, img_bytes, dtype=np.uint8)
    fo = np.zeros((H, W, 3), np.uint16)
    fo[..., :2] = rng.integers(32768 - 8000, 32768 + 8000, (H, W, 2))
    fo[..., 2] = rng.random((H, W)) < 0.3
    host[offs[2]:offs[2] + fo_bytes] = fo.reshape(-1).view(np.uint8)
    raw = torch.empty(total, dtype=torch.uint8, device="cuda")
    r1, r2 = (raw[o:o + img_bytes].view(H, W, 3) for o in offs[:2])
    rf = raw[offs[2]:offs[2] + fo_bytes].view(torch.uint16).view(H, W, 3)
    item = 2 if flow_dtype == "float16" else 4
    o1, o2 = (torch.empty((Hd, Wd, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    of = torch.empty((Hd, Wd, 2), dtype=getattr(torch, flow_dtype), device="cuda")
    om = torch.empty((Hd, Wd, 1), dtype=torch.uint8, device="cuda")
    mm = torch.empty(2, dtype=torch.int32, device="cuda")
    tables = ops.ingest_tables((h, wd), (Hd, Wd), like=raw)

    def copy():
        raw.copy_(stage, non_blocking=True)

    def minmax():
        ops.ingest_minmax(r1, r2, w["window"], out=mm)

    def images():
        use = mm if w["normalize"] else None
        ops.ingest_image(r1, w["window"], (Hd, Wd), tables, bgr=True, minmax=use, out=o1)
        ops.ingest_image(r2, w["window"], (Hd, Wd), tables, bgr=True, minmax=use, out=o2)

    def flow():
        ops.ingest_flow_occ(rf, w["window"], (Hd, Wd), tables, premultiply=w["premultiply"], flow_dtype=flow_dtype, out_flow=of, out_mask=om)

    def kernels():
        if w["normalize"]:
            minmax()
        images()
        flow()

    copy()
    minmax()
    variants = {"host-to-device copy": copy, "kernels of one sample": kernels, "ingest_image x 2": images, "ingest_flow_occ": flow}
    if w["normalize"]:
        variants["ingest_minmax (2 launches)"] = minmax
    t = windows(variants, iters, nwin)
    win_img, win_fo = h * wd * 3, h * wd * 6
    by = {"host-to-device copy": total, "ingest_image x 2": 2 * (win_img + Hd * Wd * 3), "ingest_flow_occ": win_fo + Hd * Wd * (2 * item + 1),
          "ingest_minmax (2 launches)": 2 * win_img}
    by["kernels of one sample"] = by["ingest_image x 2"] + by["ingest_flow_occ"] + (by["ingest_minmax (2 launches)"] if w["normalize"] else 0)
    res = {k: dict(summary(v), bytes=by[k]) for k, v in t.items()}
    margin = res["host-to-device copy"]["median_us"] / res["kernels of one sample"]["median_us"]
    return {"workload": name, "flow_dtype": flow_dtype, "stages": res, "copy_over_kernels": margin,
            "condition_met": bool(res["kernels of one sample"]["median_us"] < res["host-to-device copy"]["median_us"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "windows": a.windows, "runs": []}
    print("device: %s, torch %s; %d windows of %d rounds, us per round: median (min - max)\n" % (out["device"], out["torch"], a.windows, a.iters))
    for name, w in WORKLOADS.items():
        for flow_dtype in ("float32", "float16"):
            r = measure(name, w, flow_dtype, a.iters, a.windows)
            out["runs"].append(r)
            print("## %s, flow stored as %s\n" % (name, flow_dtype))
            print("| stage | us | bytes | GB/s | of 8 TB/s |\n|---|---|---|---|---|")
            for k, v in r["stages"].items():
                gbs = v["bytes"] / v["median_us"] / 1e3
                print("| %s | %.1f (%.1f - %.1f) | %.2f MB | %.0f | %s |" % (k, v["median_us"], v["min_us"], v["max_us"], v["bytes"] / 1e6, gbs,
                                                                          "-" if k.startswith("host") else "%.3f" % (gbs * 1e9 / PEAK)))
            print("\ncopy / kernels = %.1f: the kernels %s less time than the sample's own copy\n" % (r["copy_over_kernels"], "take" if r["condition_met"] else "DO NOT take"))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
