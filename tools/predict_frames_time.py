"""Times prediction on a frame sequence end to end on the GPU, host conversion, uploads and downloads included:

    predict          Predictor.predict(frames[:-1], frames[1:]): every HWC uint8 image converted on the host (/ 255, transpose) and
                     uploaded as float32 CHW, every inner frame twice; flow, occlusion mask and warped image downloaded
    predict+color    the same, and the flows coloured on the device afterwards from the downloaded arrays (uploaded again): what a
                     caller of predict() has to do for the picture
    frames           Predictor.predict_frames(frames): every frame uploaded once as bytes; flow and occlusion mask downloaded
    frames+color     predict_frames(frames, color=True): the colours made on the device from the batch's flow buffer, downloaded too

A window is one pass over the sequence, ended by the last download (a host clock around work that ends in a device synchronise);
the variants alternate window by window and the median window is reported with the fastest and the slowest.  PCIe bytes per pair are
counted from the shapes.  Seeded synthetic frames and parameters: the time does not depend on the values.

    python tools/predict_frames_time.py [--size 436,1024 --batch 4 --frames 32 --windows 9] [--json PATH]

Prints a markdown report."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maskflownet_amd import network, ops, predict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="436,1024")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    H, W = (int(v) for v in args.size.split(","))
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(args.frames)]
    p = predict.Predictor(network.random_params(0), args.batch, H, W)
    pairs = args.frames - 1

    def colour(flows):
        for f in flows:
            net_order = torch.from_numpy(np.ascontiguousarray(f[..., ::-1].transpose(2, 0, 1))[None]).cuda()
            ops.flow_color(net_order).cpu()

    variants = {
        "predict": lambda: [o[0] for o in p.predict(frames[:-1], frames[1:])],
        "predict+color": lambda: colour([o[0] for o in p.predict(frames[:-1], frames[1:])]),
        "frames": lambda: [o[0] for o in p.predict_frames(frames)],
        "frames+color": lambda: [o[3] for o in p.predict_frames(frames, color=True)],
    }
    px = H * W
    pcie = {   # bytes per pair: host -> device, device -> host
        "predict": (2 * 3 * px * 4, (2 + 1 + 3) * px * 4),
        "predict+color": (2 * 3 * px * 4 + 2 * px * 4, (2 + 1 + 3) * px * 4 + 3 * px),
        "frames": (3 * px * args.frames / pairs, (2 + 1) * px * 4),
        "frames+color": (3 * px * args.frames / pairs, (2 + 1) * px * 4 + 3 * px),
    }
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / pairs)
    report = {"size": [H, W], "batch": args.batch, "frames": args.frames, "windows": args.windows, "device": torch.cuda.get_device_name(0),
              "variants": {k: {"median_ms_per_pair": statistics.median(v), "min_ms_per_pair": min(v), "max_ms_per_pair": max(v),
                               "h2d_bytes_per_pair": pcie[k][0], "d2h_bytes_per_pair": pcie[k][1]} for k, v in times.items()}}
    print("| variant | ms per pair (median of %d windows) | fastest | slowest | MB up per pair | MB down per pair |" % args.windows)
    print("|---|---|---|---|---|---|")
    for k, r in report["variants"].items():
        print("| %s | %.3f | %.3f | %.3f | %.2f | %.2f |" % (k, r["median_ms_per_pair"], r["min_ms_per_pair"], r["max_ms_per_pair"],
                                                              r["h2d_bytes_per_pair"] / 1e6, r["d2h_bytes_per_pair"] / 1e6))
    print("\n%dx%d, batch %d, %d frames (%d pairs), %s" % (H, W, args.batch, args.frames, pairs, report["device"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
