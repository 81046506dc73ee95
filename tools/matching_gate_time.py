#!/usr/bin/env python3
"""The matching gate's kernels (kernels/gate.h) next to the torch element-wise kernels they replace, and a training step with
LibraryBackend(fused_matching=...) off and on.  usage: matching_gate_time.py [report.md]   env: ITERS=200 STEPS=10 ROUNDS=3

Part 1, per gated level of cfg2 (batch 8, 384 x 512: levels 5..2): forward + backward of the gate, all three gradients, one upstream
gradient (what the trainable networks run).
  library   the kernels' own time: mfn_profile_* (device events around every launch), summed over the gate's launches, per call;
            and the region between two device events around ITERS forward + backward calls (kernels AND the gaps between them)
  torch     the composition of training.py, leaky_relu(raw * sigmoid(mask) + tradeoff, 0.1) and its autograd backward: the same
            region figure (its kernels are not the library's to instrument)
Part 2: wall time (host clock around STEPS steps ending in a device synchronise) of training.train_step on MaskFlownetSTrainable,
batch 8, 384 x 512, FusedMultiscaleEpe, torch Adam; flag off and on alternate, ROUNDS times each, after a warm-up of both."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from maskflownet_amd import _lib, hotpath, network, ops, training  # noqa: E402

ITERS, STEPS, ROUNDS = (int(os.environ.get(k, d)) for k, d in (("ITERS", "200"), ("STEPS", "10"), ("ROUNDS", "3")))
lib = _lib.lib()
lines = []


def say(s=""):
    print(s)
    lines.append(s)


def kernel_ms(substr):
    c, ms = ctypes.c_int(0), ctypes.c_double(0)
    lib.profile_query(substr.encode(), ctypes.byref(c), ctypes.byref(ms))
    return c.value, ms.value


def region_us(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def gate_level(level):
    N, C, H, W = hotpath.level_shapes(*hotpath.CONFIGS["cfg2"][:3])[level]
    g = torch.Generator(device="cuda").manual_seed(level)
    raw, trade, gout = (torch.randn(N, C, H, W, device="cuda", generator=g) for _ in range(3))
    mask = torch.randn(N, 1, H, W, device="cuda", generator=g) * 2
    o = ops.default_ops()
    out = torch.empty_like(raw)
    grads = (torch.empty_like(raw), torch.empty_like(mask), torch.empty_like(raw))

    def library():
        o.matching_gate(raw, mask, trade, out=out)
        o.matching_gate_backward(gout, out, raw, mask, out=grads)

    leaves = [t.clone().requires_grad_(True) for t in (raw, mask, trade)]

    def composed():
        y = torch.nn.functional.leaky_relu(leaves[0] * torch.sigmoid(leaves[1]) + leaves[2], 0.1)
        torch.autograd.grad(y, leaves, gout)
    lib_region = region_us(library, ITERS)
    torch_region = region_us(composed, ITERS)
    torch.cuda.synchronize()
    lib.profile_reset()
    lib.profile_enable(1)
    for _ in range(ITERS):
        library()
    torch.cuda.synchronize()
    lib.profile_enable(0)
    (nf, fms), (nb, bms), (nj, jms) = kernel_ms("matching_gate_fwd"), kernel_ms("matching_gate_bwd_v"), kernel_ms("matching_gate_bwd_join")
    plan = "%d slices" % (lib.matching_gate_bwd_workspace_bytes(N, C, H, W) // (N * H * W * 4) or 1)
    say("| %d | %dx%dx%dx%d | %s | %.1f | %.1f | %.1f | %.1f | %.1f |" % (
        level, N, C, H, W, plan, fms * 1e3 / nf, (bms + jms) * 1e3 / nb, (fms + bms + jms) * 1e3 / nf, lib_region, torch_region))


def steps_ms(net, opt, loss_fn, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        training.train_step(net, loss_fn, opt, *batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    say("device: %s; torch %s; %s" % (torch.cuda.get_device_name(0), torch.__version__, lib.version_string().decode()))
    say()
    say("Gate forward + backward per call, microseconds (ITERS = %d)" % ITERS)
    say()
    say("| level | shape | backward plan | fwd kernel | bwd kernels | fwd + bwd kernels | library, event region | torch composition, event region |")
    say("|---|---|---|---|---|---|---|---|")
    for level in (5, 4, 3, 2):
        gate_level(level)
    say()
    N, H, W = 8, 384, 512
    params = network.random_params(0)
    g = torch.Generator().manual_seed(1)
    batch = [t.cuda() for t in (torch.rand(N, 3, H, W, generator=g) - 0.5, torch.rand(N, 3, H, W, generator=g) - 0.5,
                                torch.randn(N, 2, H, W, generator=g) * 3, (torch.rand(N, 1, H, W, generator=g) > 0.1).float())]
    runs = {}
    for flag in (False, True):
        net = training.MaskFlownetSTrainable(params, backend=training.LibraryBackend(fused_matching=flag)).cuda()
        runs[flag] = (net, torch.optim.Adam(net.parameters(), lr=1e-5), training.FusedMultiscaleEpe())
        steps_ms(*runs[flag], batch, 3)     # warm-up
    say("training.train_step, MaskFlownetSTrainable, batch %d, %d x %d, milliseconds per step (%d steps per figure, off / on alternating)" % (N, H, W, STEPS))
    say()
    say("| round | fused_matching=False | fused_matching=True |")
    say("|---|---|---|")
    for r in range(ROUNDS):
        off = steps_ms(*runs[False], batch, STEPS)
        on = steps_ms(*runs[True], batch, STEPS)
        say("| %d | %.2f | %.2f |" % (r + 1, off, on))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
