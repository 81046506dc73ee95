"""layer.matching_level / layer._MatchingLevelFn: one pyramid level's matching step (MaskFlownet.py:230-236), differentiable on the
library -- deformable convolution, gate (kernels/gate.h), cost volume with its fused LeakyReLU, and their backward kernels.

Reference: the oracle chain that tests/test_mxnet_binding.py::_matching_level states forward (oracle.deformable_convolution on
offsets_from_flow, the gate of tests/gate_ref.py, oracle.correlation) and its backward functions, in fp64 (acceptance) and in fp32 (the
twin).  Bar: parity_cases.check_fp64_bound on both outputs and all seven input gradients.  M is composed stage by stage:
ref_numpy.deformable_convolution_bound -> matching_bound -> correlation_bound forward; correlation_backward_bound (on M of warp) ->
gate_ref's bounds (on M of raw and M of the cost volume's gradient) -> deformable_convolution_shared_backward_bound backward.  Both
LeakyReLU kinks of the backward are read from the outputs the library computed, by the library and by both references alike.  Flows
lie on the exact_positions grid, so that every sample position is the same number in fp32 and fp64.

The chain through the OpSet (no torch) runs on the emulation here and on the MI355X under -m gpu; the autograd function, its
needs_input_grad patterns and the no-grad form are GPU tests."""
import numpy as np
import pytest

from oracle import ref as oracle
from oracle import ref_numpy
from tests import gate_ref as gr
from tests import parity_cases as pc
from tests.fp64_env import Env, exact_positions

U = 2.0 ** -24
SCALE = 20.0
CASES = {"gated": ((1, 32, 6, 8), 8.0, 4, True), "ungated": ((2, 48, 4, 8), 16.0, 2, False)}
NAMES = ("c1", "c2", "flow", "weight", "bias", "mask", "tradeoff")
_CACHE = {}


def leaky(v, dtype):
    return np.maximum(v, (dtype(0.1) * v).astype(dtype))


def inputs(case):
    if case not in _CACHE:
        (N, C, H, W), stride, md, gated = CASES[case]
        rng = np.random.default_rng([N, C, H, W, md])
        a = {"c1": pc.feat(rng, (N, C, H, W)), "c2": pc.feat(rng, (N, C, H, W)),
             # flows on a 2^-10 (stride 8: x 2.5) / 2^-9 (stride 16: x 1.25) grid: the offsets land on exact_positions' 2^-11 grid
             "flow": exact_positions(pc.flow_field(rng, N, H, W) * np.float32(stride / SCALE), 2.0 ** -10 if stride == 8.0 else 2.0 ** -9),
             "weight": pc.msra_weight(rng, C, C), "bias": (rng.standard_normal(C) * 0.1).astype(np.float32),
             "mask": (rng.standard_normal((N, 1, H, W)) * 2).astype(np.float32) if gated else None,
             "tradeoff": rng.standard_normal((N, C, H, W)).astype(np.float32) if gated else None,
             "gcorr": rng.standard_normal((N, (2 * md + 1) ** 2, H, W)).astype(np.float32),
             "gwarp": rng.standard_normal((N, C, H, W)).astype(np.float32)}
        off = oracle.offsets_from_flow(a["flow"], SCALE, stride)
        assert (off == exact_positions(off)).all()
        fwd = {}
        for dt in (np.float64, np.float32):
            o = oracle.offsets_from_flow(a["flow"], SCALE, stride, dtype=dt)
            raw = oracle.deformable_convolution(a["c2"], o, a["weight"], a["bias"], kernel=(3, 3), pad=(1, 1), dtype=dt)
            warp = gr.forward(raw, a["mask"], a["tradeoff"], True, dtype=dt)
            corr = leaky(oracle.correlation(a["c1"], warp, max_displacement=md, pad_size=md, dtype=dt), dt)
            fwd[dt] = (o, raw, warp, corr)
        Mraw = ref_numpy.deformable_convolution_bound(a["c2"], off, a["weight"], a["bias"])
        Mwarp = ref_numpy.matching_bound(Mraw, a["mask"], a["tradeoff"])
        _CACHE[case] = (a, fwd, (Mraw, Mwarp, ref_numpy.correlation_bound(a["c1"], Mwarp, md)))
    return _CACHE[case]


def reference_backward(case, yw, yc, seed_warp, dt):
    """The seven gradients of the oracle chain in `dt`, the kinks from the given outputs."""
    (N, C, H, W), stride, md, gated = CASES[case]
    a, fwd, _ = inputs(case)
    off, raw, warp, _ = fwd[dt]
    gc = a["gcorr"].astype(dt)
    gpre = np.where(yc > 0, gc, (gc * dt(0.1)).astype(dt)).astype(dt)
    g1, g2 = oracle.correlation_backward(gpre, a["c1"], warp, max_displacement=md, pad_size=md, dtype=dt)
    graw, gmask, gtr = gr.backward(a["gwarp"], yw, raw, a["mask"], True, g2, dtype=dt) if seed_warp else gr.backward(g2, yw, raw, a["mask"], True, dtype=dt)
    gx, goff, gw, gb = oracle.deformable_convolution_backward(graw, a["c2"], off, a["weight"], with_bias=True, kernel=(3, 3), pad=(1, 1), dtype=dt)
    gflow = (goff.reshape(N, 9, 2, H, W).sum(axis=1) * dt(SCALE / stride)).astype(dt)
    return [g1, gx, gflow, gw, gb, gmask, gtr if gated else None]


def bound_backward(case, yw, seed_warp):
    (N, C, H, W), stride, md, gated = CASES[case]
    a, _, (Mraw, Mwarp, _) = inputs(case)
    M1, M2 = ref_numpy.correlation_backward_bound(a["gcorr"], a["c1"], Mwarp, md)
    Mgraw, Mgmask, Mgtr = gr.backward(a["gwarp"], yw, Mraw, a["mask"], True, M2, magnitude=True) if seed_warp else \
        gr.backward(M2, yw, Mraw, a["mask"], True, magnitude=True)
    Mgx, Mgflow, Mgw, Mgb = ref_numpy.deformable_convolution_shared_backward_bound(Mgraw, a["c2"], a["flow"], SCALE, stride, a["weight"])
    return [M1, Mgx, Mgflow, Mgw, Mgb, Mgmask, Mgtr if gated else None]


def check_outputs(case, corr, warp, what):
    _, fwd, (_, Mwarp, Mcorr) = inputs(case)
    for nm, got, i, M in (("warp", warp, 2, Mwarp), ("corr", corr, 3, Mcorr)):
        pc.assert_magnitude_bound(M, fwd[np.float64][i], "%s %s" % (what, nm))
        e_lib, e_ref = pc.check_fp64_bound(got, fwd[np.float64][i], fwd[np.float32][i], M, "%s %s" % (what, nm))
        print("%s %s: e_lib %.2f ulp, e_twin %.2f ulp of M" % (what, nm, e_lib / U, e_ref / U))


def check_gradients(case, grads, yw, yc, seed_warp, what, wanted=(True,) * 7):
    want64, ref32, M = (reference_backward(case, yw, yc, seed_warp, np.float64), reference_backward(case, yw, yc, seed_warp, np.float32),
                        bound_backward(case, yw, seed_warp))
    for nm, g, w64, r32, m, need in zip(NAMES, grads, want64, ref32, M, wanted):
        if w64 is None or not need:
            assert g is None, "%s: a gradient of %s came back" % (what, nm)
            continue
        pc.assert_magnitude_bound(m, w64, "%s g%s" % (what, nm))
        e_lib, e_ref = pc.check_fp64_bound(g, w64, r32, m, "%s gradient of %s" % (what, nm))
        print("%s g%s: e_lib %.2f ulp, e_twin %.2f ulp of M" % (what, nm, e_lib / U, e_ref / U))


# ---- the chain through the OpSet: what _MatchingLevelFn runs, on the emulation and on the GPU -----------------------------------
def check_opset_chain(env, case, seed_warp):
    (N, C, H, W), stride, md, gated = CASES[case]
    a, _, _ = inputs(case)
    o, d = env.ops, {k: (None if v is None else env.dev(v)) for k, v in inputs(case)[0].items()}
    with env.launches() as L:
        raw = o.deformable_convolution_shared(d["c2"], d["flow"], SCALE, stride, d["weight"], d["bias"])
        warp = o.matching_gate(raw, d["mask"], d["tradeoff"])
        corr = o.Correlation(d["c1"], warp, kernel_size=1, max_displacement=md, stride1=1, stride2=1, pad_size=md, activation="leaky")
        g1, g2 = o.Correlation_backward(o.LeakyReLU_backward(d["gcorr"], corr), d["c1"], warp, kernel_size=1, max_displacement=md, stride1=1,
                                        stride2=1, pad_size=md)
        graw, gmask, gtr = o.matching_gate_backward(d["gwarp"] if seed_warp else g2, warp, raw, d["mask"], out_grad2=g2 if seed_warp else None)
        gx, gfl, gw, gb = o.deformable_convolution_shared_backward(graw, d["c2"], d["flow"], SCALE, stride, d["weight"])
    L.expect(["matching_gate_fwd_v4", "matching_gate_bwd_v4"] + (["matching_gate_bwd_join"] if gated else []), what=case)
    host = lambda t: None if t is None else np.array(env.host(t))
    yw, yc = host(warp), host(corr)
    what = "%s, OpSet chain, %s" % (case, "both heads" if seed_warp else "corr alone")
    check_outputs(case, yc, yw, what)
    check_gradients(case, [host(g) for g in (g1, gx, gfl, gw, gb, gmask, gtr if gated else None)], yw, yc, seed_warp, what)


@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


@pytest.mark.parametrize("case,seed_warp", [("gated", True), ("ungated", True), ("gated", False)])
def test_emu_opset_chain_against_fp64(emu, case, seed_warp):
    check_opset_chain(emu, case, seed_warp)


@pytest.mark.gpu
@pytest.mark.parametrize("case,seed_warp", [("gated", True), ("ungated", True), ("gated", False)])
def test_gpu_opset_chain_against_fp64(gpu, case, seed_warp):
    check_opset_chain(gpu, case, seed_warp)


# ---- the autograd function and the public entry (GPU) -----------------------------------------------------------------------------
def _tensors(case, requires):
    import torch
    a, _, _ = inputs(case)
    return {k: (None if a[k] is None else torch.from_numpy(a[k]).cuda().requires_grad_(k in requires)) for k in a}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_no_grad_form_is_the_inference_form_bit_for_bit(gpu, case):
    import torch
    from maskflownet_amd import layer, ops
    (N, C, H, W), stride, md, gated = CASES[case]
    t = _tensors(case, ())
    corr, warp = layer.matching_level(t["c1"], t["c2"], t["flow"], t["weight"], t["bias"], t["mask"], t["tradeoff"], SCALE, stride, md)
    want_warp = ops.default_ops().deformable_matching(t["c2"], t["flow"], SCALE, stride, t["weight"], t["bias"], t["mask"], t["tradeoff"])
    want_corr = ops.Correlation(t["c1"], want_warp, pad_size=md, kernel_size=1, max_displacement=md, stride1=1, stride2=1, activation="leaky")
    assert torch.equal(warp, want_warp) and torch.equal(corr, want_corr)
    assert not corr.requires_grad and not warp.requires_grad
    with torch.no_grad():         # requires_grad inputs under no_grad: still the inference form
        t2 = _tensors(case, NAMES)
        corr2, _ = layer.matching_level(t2["c1"], t2["c2"], t2["flow"], t2["weight"], t2["bias"], t2["mask"], t2["tradeoff"], SCALE, stride, md)
    assert torch.equal(corr2, want_corr)
    out = torch.empty_like(corr)
    got, _ = layer.matching_level(t["c1"], t["c2"], t["flow"], t["weight"], t["bias"], t["mask"], t["tradeoff"], SCALE, stride, md, out=out)
    assert got is out and torch.equal(out, want_corr)
    t3 = _tensors(case, ("weight",))
    with pytest.raises(RuntimeError, match="inference-time"):
        layer.matching_level(t3["c1"], t3["c2"], t3["flow"], t3["weight"], t3["bias"], t3["mask"], t3["tradeoff"], SCALE, stride, md, out=out)


PATTERNS = {"everything": NAMES, "the frozen head's": ("flow", "weight", "bias", "mask", "tradeoff"), "only weight": ("weight",)}


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("case,seed_warp", [("gated", True), ("ungated", True), ("gated", False)])
def test_gpu_autograd_against_fp64(gpu, case, seed_warp, pattern):
    import torch
    from maskflownet_amd import layer
    (N, C, H, W), stride, md, gated = CASES[case]
    t = _tensors(case, PATTERNS[pattern])
    with gpu.launches() as L:
        corr, warp = layer.matching_level(t["c1"], t["c2"], t["flow"], t["weight"], t["bias"], t["mask"], t["tradeoff"], SCALE, stride, md)
        heads, seeds = [corr], [t["gcorr"]]
        if seed_warp:
            heads.append(warp)
            seeds.append(t["gwarp"])
        torch.autograd.backward(heads, seeds)
    assert L.count("matching_gate_fwd") == 1 and L.count("matching_gate_bwd_v") == 1
    yw, yc = warp.detach().cpu().numpy(), corr.detach().cpu().numpy()
    what = "%s, autograd, %s, %s" % (case, "both heads" if seed_warp else "corr alone", pattern)
    check_outputs(case, yc, yw, what)
    grads = [None if (t[k] is None or t[k].grad is None) else t[k].grad.cpu().numpy() for k in NAMES]
    check_gradients(case, grads, yw, yc, seed_warp, what, wanted=[k in PATTERNS[pattern] for k in NAMES])


@pytest.mark.gpu
def test_gpu_forward_matching_is_differentiable(gpu):
    """DeformableConv2D.forward_matching under autograd: the gate's own kernels, the gradients of the same chain without the cost volume."""
    import torch
    from maskflownet_amd import layer
    (N, C, H, W), stride, md, gated = CASES["gated"]
    a, fwd, (Mraw, Mwarp, _) = inputs("gated")
    t = _tensors("gated", ("c2", "flow", "mask", "tradeoff"))
    blk = layer.DeformableConv2D(C, 3, padding=1, in_channels=C).cuda()
    with torch.no_grad():
        blk.weight.copy_(t["weight"])
        blk.bias.copy_(t["bias"])
    with gpu.launches() as L:
        warp = blk.forward_matching(t["c2"], t["flow"], SCALE, stride, t["mask"], t["tradeoff"])
        warp.backward(t["gwarp"])
    assert L.count("matching_gate_fwd_v4") == 1 and L.count("matching_gate_bwd_v4") == 1
    yw = warp.detach().cpu().numpy()
    pc.check_fp64_bound(yw, fwd[np.float64][2], fwd[np.float32][2], Mwarp, "forward_matching under autograd")
    refs = []
    for dt in (np.float64, np.float32):
        off, raw, _, _ = fwd[dt]
        graw, gmask, gtr = gr.backward(a["gwarp"], yw, raw, a["mask"], True, dtype=dt)
        gx, goff, gw, gb = oracle.deformable_convolution_backward(graw, a["c2"], off, a["weight"], with_bias=True, kernel=(3, 3), pad=(1, 1), dtype=dt)
        refs.append([gx, (goff.reshape(N, 9, 2, H, W).sum(axis=1) * dt(SCALE / stride)).astype(dt), gw, gb, gmask, gtr])
    Mgraw, Mgmask, Mgtr = gr.backward(a["gwarp"], yw, Mraw, a["mask"], True, magnitude=True)
    M = list(ref_numpy.deformable_convolution_shared_backward_bound(Mgraw, a["c2"], a["flow"], SCALE, stride, a["weight"])) + [Mgmask, Mgtr]
    got = [t["c2"].grad, t["flow"].grad, blk.weight.grad, blk.bias.grad, t["mask"].grad, t["tradeoff"].grad]
    for nm, g, w64, r32, m in zip(("c2", "flow", "weight", "bias", "mask", "tradeoff"), got, refs[0], refs[1], M):
        pc.check_fp64_bound(g.cpu().numpy(), w64, r32, m, "forward_matching gradient of %s" % nm)
    with torch.no_grad():     # the no-grad branch is the single fused launch, as before
        with gpu.launches() as L:
            blk.forward_matching(t["c2"], t["flow"], SCALE, stride, t["mask"], t["tradeoff"])
        assert L.count("matching_gate") == 0
