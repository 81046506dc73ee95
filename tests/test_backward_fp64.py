"""fp64 acceptance of the backward kernels, per element.

Every case runs the library, the fp32 oracle (the MXNet-faithful loops of oracle/mfn_ref_body.inc), the fp64 oracle and the
magnitude bound M (oracle/ref_numpy.*_bound: per element, the sum of |terms|) on the same seeded inputs, and asserts
parity_cases.check_fp64_bound: max |got - fp64| / M within 4x the fp32 oracle's + 16 ulp, exact zeros where no term exists,
finite outputs.  Output gradients are plain N(0,1) and graded (10^U(-6,0) per pixel, one image at 1e-3): an error in a small
element is invisible to the global check_close bar.  Each case runs under both arithmetics of its operator (ARITH_FP32 and the
default) and asserts the kernel it reached, so that a plan change cannot move it onto a fallback unnoticed.

CPU half: the real kernel sources on the emulation (tests/emu) at small shapes that take the same kernels.  `-m gpu`: the
bench pyramids (CFG2: 384x512 at batch 8, CFG3: 448x1024 at batch 4).  MFN_BWD_FP64_REPORT=<file> appends the maxima per
case and arithmetic to <file>."""
import os

import numpy as np
import pytest

from oracle import ref as oracle
from oracle import ref_numpy
from tests import parity_cases as pc
from tests.fp64_env import Env, deform_offsets, exact_positions, per_image as _per_image

ARITHS = [0, -1]                # ARITH_FP32, ARITH_DEFAULT
GOUTS = ["plain", "graded"]
_CACHE = {}
_RESULTS = []


def _gout(rng, shape, kind):
    return pc.graded_gout(rng, shape) if kind == "graded" else rng.standard_normal(shape).astype(np.float32)


def _cached(key, make):
    """The oracle results (fp32, fp64, M) of one input set, shared by the runs under both arithmetics."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _seq_sum(parts):
    acc = parts[0].copy()
    for p in parts[1:]:
        acc += p              # the oracle's order: gw += (one image's sum), image after image, in its own precision
    return acc


def _dc_oracle(go, x, off, w, dtype):
    r = _per_image(lambda g, xx, o: oracle.deformable_convolution_backward(g, xx, o, w, with_bias=True, kernel=(3, 3), pad=(1, 1),
                                                                           dtype=dtype), go, x, off)
    return (np.concatenate([a[0] for a in r]), np.concatenate([a[1] for a in r]), _seq_sum([a[2] for a in r]),
            _seq_sum([a[3] for a in r]))


def _check(what, arith, got, want64, ref32, M, base=None):
    e_lib, e_ref = pc.check_fp64_bound(got, want64, ref32, M, what=what, base=base)
    _RESULTS.append((what, arith, e_lib, e_ref))
    return e_lib, e_ref


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def case_corr_bwd(env, arith, shape, md, gkind, req="write", seed=0):
    N, C, H, W = shape
    D = 2 * md + 1
    rng = np.random.default_rng(700 + seed)
    f1, f2 = pc.feat(rng, shape), pc.feat(rng, shape)
    go = _gout(rng, (N, D * D, H, W), gkind)

    def make():
        kw = dict(max_displacement=md, pad_size=md)
        r32 = _per_image(lambda g, a, b: oracle.correlation_backward(g, a, b, **kw), go, f1, f2)
        r64 = _per_image(lambda g, a, b: oracle.correlation_backward(g, a, b, dtype=np.float64, **kw), go, f1, f2)
        cat = lambda r, k: np.concatenate([a[k] for a in r])
        return (cat(r32, 0), cat(r32, 1)), (cat(r64, 0), cat(r64, 1)), ref_numpy.correlation_backward_bound(go, f1, f2, md)

    ref32, want64, M = _cached(("corr", shape, md, gkind, seed), make)
    env.set_arith("corr", arith)
    # req 'add': the caller's values at the gradient's own scale (an N(0,1) base under a graded gradient would leave the sum's
    # rounding, not the kernel, as the measured error)
    base = [(rng.standard_normal(shape) * m).astype(np.float32) for m in M] if req == "add" else [None, None]
    with env.launches() as L:
        if req == "add":
            g1, g2 = env.ops.Correlation_backward(env.dev(go), env.dev(f1), env.dev(f2), 1, md, 1, 1, md, True, req1="add", req2="add",
                                                  g1=env.dev(base[0].copy()), g2=env.dev(base[1].copy()))
        else:
            g1, g2 = env.ops.Correlation_backward(env.dev(go), env.dev(f1), env.dev(f2), 1, md, 1, 1, md, True)
    what = "corr bwd %s md=%d %s %s" % (shape, md, gkind, req)
    L.expect(["corr_bwd_lds"], what=what)
    for g, w64, r32, m, b, nm in zip((g1, g2), want64, ref32, M, base, ("g1", "g2")):
        _check("%s %s" % (what, nm), arith, env.host(g), w64, r32, m, base=b)


def _dc_inputs(N, Cin, Cout, H, W, gkind, seed):
    rng = np.random.default_rng(800 + seed)
    x = pc.feat(rng, (N, Cin, H, W))
    w = pc.msra_weight(rng, Cout, Cin)
    return rng, x, w, _gout(rng, (N, Cout, H, W), gkind)


def case_deform_bwd(env, arith, N, Cin, Cout, H, W, kind, gkind, input_kernel="dc_bwd_input_pix", seed=0, tuning=None):
    """mfn_deform_conv_bwd (the drop-in DeformableConvolution backward), all four gradients."""
    rng, x, w, go = _dc_inputs(N, Cin, Cout, H, W, gkind, seed)
    off = deform_offsets(rng, N, H, W, kind)

    def make():
        return _dc_oracle(go, x, off, w, np.float32), _dc_oracle(go, x, off, w, np.float64), \
            ref_numpy.deformable_convolution_backward_bound(go, x, off, w)

    ref32, want64, M = _cached(("deform", (N, Cin, Cout, H, W), kind, gkind, seed), make)
    env.set_arith("deform", arith)
    if tuning:
        env.set_tuning(**tuning)
    try:
        with env.launches() as L:
            got = env.ops.DeformableConvolution_backward(env.dev(go), env.dev(x), env.dev(off), env.dev(w), kernel=(3, 3), pad=(1, 1))
    finally:
        if tuning:
            env.set_tuning(**{k: 0 for k in tuning})
    what = "deform bwd %s %s %s %s" % ((N, Cin, Cout, H, W), kind, gkind, input_kernel)
    wk = "dc_bwd_weight_pc" if Cout <= 96 else "dc_bwd_weight_mfma"
    L.expect([input_kernel, wk], what=what)
    for g, w64, r32, m, nm in zip(got, want64, ref32, M, ("gx", "goffset", "gw", "gbias")):
        _check("%s %s" % (what, nm), arith, env.host(g), w64, r32, m)


def case_deform_flow_bwd(env, arith, N, C, H, W, gkind, scale=20.0, stride=8.0, seed=0):
    """mfn_deform_conv_shared_bwd in flow mode: d/dflow = scale / stride * sum over the taps, against the summed bound."""
    rng, x, w, go = _dc_inputs(N, C, C, H, W, gkind, 50 + seed)
    # flows on a 2^-10 grid below 2^7: flow * 20 / 8 (and flow * 2.5) are exact, the offsets on the exact_positions grid
    fl = exact_positions(pc.flow_field(rng, N, H, W) * np.float32(stride / scale), 2.0 ** -10)
    off = oracle.offsets_from_flow(fl, scale, stride)
    assert (off == exact_positions(off)).all()
    f = np.float32(scale) / np.float32(stride)

    def make():
        r32, r64 = _dc_oracle(go, x, off, w, np.float32), _dc_oracle(go, x, off, w, np.float64)
        r32 = (r32[0], (r32[1].reshape(N, 9, 2, H, W).sum(axis=1) * f).astype(np.float32), r32[2], r32[3])
        r64 = (r64[0], r64[1].reshape(N, 9, 2, H, W).sum(axis=1) * (scale / stride), r64[2], r64[3])
        return r32, r64, ref_numpy.deformable_convolution_shared_backward_bound(go, x, fl, scale, stride, w)

    ref32, want64, M = _cached(("flow", (N, C, H, W), gkind, seed), make)
    env.set_arith("deform", arith)
    with env.launches() as L:
        got = env.ops.deformable_convolution_shared_backward(env.dev(go), env.dev(x), env.dev(fl), scale, stride, env.dev(w))
    what = "deform flow bwd %s %s" % ((N, C, H, W), gkind)
    L.expect(["dc_bwd_input_pix", "dc_bwd_weight_pc"], absent=["offsets_from_flow"], what=what)
    for g, w64, r32, m, nm in zip(got, want64, ref32, M, ("gx", "gflow", "gw", "gbias")):
        _check("%s %s" % (what, nm), arith, env.host(g), w64, r32, m)


def case_warp_bwd(env, shape, clip, gkind, seed=0):
    N, C, H, W = shape
    rng = np.random.default_rng(900 + seed)
    x = rng.standard_normal(shape).astype(np.float32)
    fl = pc.flow_field(rng, N, H, W, sigma=3.0)
    go = _gout(rng, shape, gkind)

    def make():
        # The kernel forms its sample positions as MXNet does, grid = (flow + index) / ((size-1)/2) - 1 then back, in fp32: the
        # fp64 arbiter and M are evaluated at those positions (ref_numpy.warp_backward_at, pinned to the C oracle by
        # tests/test_oracle_warp.py), so that the fp32 oracle's error -- same positions -- is arithmetic only.
        pos = ref_numpy.warp_positions(fl, clip, np.float32)
        return (oracle.warp_backward(go, x, fl, clip_grid=clip), ref_numpy.warp_backward_at(go, x, pos),
                ref_numpy.warp_backward_at(go, x, pos, bound=True))

    ref32, want64, M = _cached(("warp", shape, clip, gkind, seed), make)
    with env.launches() as L:
        got = env.ops.warp_backward(env.dev(go), env.dev(x), env.dev(fl), clip_grid=clip)
    what = "warp bwd %s clip=%s %s" % (shape, clip, gkind)
    L.expect(["warp_bwd"], what=what)
    for g, w64, r32, m, nm in zip(got, want64, ref32, M, ("gx", "gflow")):
        _check("%s %s" % (what, nm), None, env.host(g), w64, r32, m)


def _torch_conv_grads(x, w, b, gpre, dtype):
    import torch
    F = torch.nn.functional
    tx = torch.tensor(x, dtype=dtype, requires_grad=True)
    tw = torch.tensor(w, dtype=dtype, requires_grad=True)
    tb = torch.tensor(b, dtype=dtype, requires_grad=True) if b is not None else None
    F.conv2d(tx, tw, tb, padding=1).backward(torch.tensor(gpre, dtype=dtype))
    return tx.grad.numpy(), tw.grad.numpy(), tb.grad.numpy() if tb is not None else None


def case_conv_bwd(env, arith, N, Cin, Cout, H, W, gkind, leaky=False, kernels=(), seed=0):
    """mfn_conv2d_bwd, 3x3 / stride 1 / pad 1: want64 = torch fp64 autograd, ref32 = the same in fp32, M = the fp64 autograd on
    |x|, |W| and |the gradient behind the LeakyReLU|."""
    import torch
    rng = np.random.default_rng(1000 + seed)
    x = pc.feat(rng, (N, Cin, H, W))
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (1.01 * Cin * 9))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    go = _gout(rng, (N, Cout, H, W), gkind)
    env.set_arith("conv", arith)
    y = env.ops.Convolution(env.dev(x), env.dev(w), env.dev(b), pad=(1, 1), activation="leaky" if leaky else None)
    y64 = torch.nn.functional.conv2d(torch.tensor(x, dtype=torch.float64), torch.tensor(w, dtype=torch.float64),
                                     torch.tensor(b, dtype=torch.float64), padding=1).numpy()
    slope = np.where(y64 > 0, 1.0, 0.1) if leaky else 1.0

    def make():
        g64 = go.astype(np.float64) * slope
        g32 = np.where(y64 > 0, go, np.float32(0.1) * go).astype(np.float32) if leaky else go
        return (_torch_conv_grads(x, w, b, g32, torch.float32), _torch_conv_grads(x, w, b, g64, torch.float64),
                _torch_conv_grads(np.abs(x), np.abs(w), np.abs(b), np.abs(g64), torch.float64))

    ref32, want64, M = _cached(("conv", (N, Cin, Cout, H, W), leaky, gkind, seed), make)
    with env.launches() as L:
        got = env.ops.Convolution_backward(env.dev(go), env.dev(x), env.dev(w), output=y if leaky else None, pad=(1, 1),
                                           activation="leaky" if leaky else None)
    what = "conv bwd %s leaky=%s %s" % ((N, Cin, Cout, H, W), leaky, gkind)
    L.expect(kernels, what=what)
    for g, w64, r32, m, nm in zip(got, want64, ref32, M, ("gx", "gw", "gbias")):
        _check("%s %s" % (what, nm), arith, env.host(g), w64, r32, m)


def conv_kernels(arith, dcm):
    """Kernels of a 3x3 / stride 1 / dilation 1 backward with W % 16 == 0: the weight gradient on the bf16 x 3 matrix-core kernel under
    the default arithmetic (the fp32 MFMA one under ARITH_FP32), the data gradient on dc_mma_kernel<CONV> where the plan takes it."""
    if arith == 0:
        return ("conv_wgrad",)
    return ("conv_wgrad_bf16x3",) + (("conv3x3_dcm",) if dcm else ())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MFN_BWD_FP64_REPORT")
    if path and _RESULTS:
        with open(path, "a") as f:
            for what, arith, e_lib, e_ref in _RESULTS:
                f.write("%-80s arith %-7s max e_lib %.3e   max e_ref32 %.3e   ratio %.3f\n" % (
                    what, {0: "fp32", -1: "default", None: "-"}[arith], e_lib, e_ref, e_lib / e_ref if e_ref > 0 else 0.0))


# ---- CPU half: the emulation at small shapes that take the same kernels -----------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture
def _emu_defaults(emu):
    yield
    from tests.emu import emu_ops
    emu_ops.set_tuning(corr_gram=-1, dc_mma=-1, conv_mma=-1, bwd_off=0, conv_dcm=0)


@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("arith", ARITHS)
def test_emu_correlation_backward(emu, _emu_defaults, arith, gkind):
    case_corr_bwd(emu, arith, (2, 5, 6, 16), 4, gkind)
    case_corr_bwd(emu, arith, (1, 4, 7, 32), 2, gkind, seed=1)
    case_corr_bwd(emu, arith, (1, 3, 5, 8), 4, gkind, req="add", seed=2)


@pytest.mark.parametrize("kind", ["smooth", "rough", "far"])
@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("arith", ARITHS)
def test_emu_deform_backward(emu, _emu_defaults, arith, gkind, kind):
    case_deform_bwd(emu, arith, 2, 4, 8, 9, 16, kind, gkind)


@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("arith", ARITHS)
def test_emu_deform_backward_per_tap(emu, _emu_defaults, arith, gkind):
    """Per-tap offsets: the lane = pixel kernel's tap-by-tap strips, and the tap-by-tap kernel alone (bwd.off=1)."""
    case_deform_bwd(emu, arith, 1, 4, 8, 7, 16, "pertap", gkind)
    case_deform_bwd(emu, arith, 1, 4, 8, 7, 16, "pertap", gkind, input_kernel="dc_bwd_input_tile", tuning=dict(bwd_off=1))


@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("arith", ARITHS)
def test_emu_deform_flow_backward(emu, _emu_defaults, arith, gkind):
    case_deform_flow_bwd(emu, arith, 1, 4, 5, 8, gkind)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("gkind", GOUTS)
def test_emu_warp_backward(emu, gkind, clip):
    case_warp_bwd(emu, (2, 3, 8, 11), clip, gkind)


@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("arith", ARITHS)
def test_emu_conv_backward(emu, _emu_defaults, arith, gkind):
    case_conv_bwd(emu, arith, 1, 8, 32, 8, 16, gkind, kernels=conv_kernels(arith, False))
    emu.set_tuning(conv_dcm=2)   # the plan's >= 384-tile threshold, forced at a small shape
    case_conv_bwd(emu, arith, 2, 37, 32, 6, 16, gkind, leaky=True, kernels=conv_kernels(arith, True), seed=1)


# ---- GPU half: the bench shapes ---------------------------------------------------------------------------------------------------
CFG2 = [(8, 196, 6, 8), (8, 128, 12, 16), (8, 96, 24, 32), (8, 64, 48, 64), (8, 32, 96, 128)]      # levels 6..2 of 384x512, N=8
CFG3 = [(4, 196, 7, 16), (4, 128, 14, 32), (4, 96, 28, 64), (4, 64, 56, 128), (4, 32, 112, 256)]   # levels 6..2 of 448x1024, N=4
LEVEL = {6: 0, 5: 1, 4: 2, 3: 3, 2: 4}
PYR = {"cfg2": CFG2, "cfg3": CFG3}


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


@pytest.fixture
def _gpu_defaults(gpu):
    yield
    from maskflownet_amd import _lib
    _lib.set_arithmetic(all=-1)
    _lib.set_tuning(bwd_off=0)


def _lv(cfg, level):
    return PYR[cfg][LEVEL[level]]


@pytest.mark.gpu
@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("cfg,level,md", [(c, l, 4) for c in PYR for l in (6, 5, 4, 3, 2)] + [(c, l, 2) for c in PYR for l in (3, 2)])
def test_gpu_correlation_backward(gpu, _gpu_defaults, cfg, level, md, gkind):
    for arith in ARITHS:
        case_corr_bwd(gpu, arith, _lv(cfg, level), md, gkind)
    if level == 3 and md == 4:
        case_corr_bwd(gpu, -1, _lv(cfg, level), md, gkind, req="add")


@pytest.mark.gpu
@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("cfg,level,kind", [(c, l, "smooth") for c in PYR for l in (5, 4, 3, 2)]
                         + [(c, l, k) for c in PYR for l in (4, 2) for k in ("rough", "far")])
def test_gpu_deform_backward(gpu, _gpu_defaults, cfg, level, kind, gkind):
    N, C, H, W = _lv(cfg, level)
    for arith in ARITHS:
        case_deform_bwd(gpu, arith, N, C, C, H, W, kind, gkind)


@pytest.mark.gpu
@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("cfg", list(PYR))
def test_gpu_deform_backward_per_tap(gpu, _gpu_defaults, cfg, gkind):
    """Per-tap offsets at level 3: the lane = pixel kernel's tap-by-tap strips, and the tap-by-tap kernel alone (bwd.off=1)."""
    N, C, H, W = _lv(cfg, 3)
    for arith in ARITHS:
        case_deform_bwd(gpu, arith, N, C, C, H, W, "pertap", gkind)
        case_deform_bwd(gpu, arith, N, C, C, H, W, "pertap", gkind, input_kernel="dc_bwd_input_tile", tuning=dict(bwd_off=1))


@pytest.mark.gpu
@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("cfg,level", [(c, l) for c in PYR for l in (4, 2)])
def test_gpu_deform_flow_backward(gpu, _gpu_defaults, cfg, level, gkind):
    N, C, H, W = _lv(cfg, level)
    for arith in ARITHS:
        case_deform_flow_bwd(gpu, arith, N, C, H, W, gkind)


@pytest.mark.gpu
@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("shape", [(8, 3, 384, 512), (4, 3, 448, 1024)])
def test_gpu_warp_backward(gpu, shape, clip, gkind):
    case_warp_bwd(gpu, shape, clip, gkind)


GPU_CONV = [   # (N, Cin, Cout, H, W, leaky, data gradient on dc_mma_kernel<CONV>)
    (1, 8, 32, 8, 16, False, False),           # tests/test_frow_backward.py GPU_CONV_CASES that take conv_wgrad_bf16x3
    (3, 35, 64, 5, 16, False, False),
    (2, 64, 32, 48, 64, True, False),
    (8, 64, 32, 48, 64, True, True),           # a level-3 decoder layer at batch 8: 768 pixel tiles, the data gradient on the matrix-core kernel
    (8, 96, 64, 24, 32, True, False),          # level 4 at batch 8: 192 tiles
]


@pytest.mark.gpu
@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("case", GPU_CONV, ids=lambda c: "x".join(map(str, c[:5])) + ("_leaky" if c[5] else ""))
def test_gpu_conv_backward(gpu, _gpu_defaults, case, gkind):
    N, Cin, Cout, H, W, leaky, dcm = case
    for arith in ARITHS:
        case_conv_bwd(gpu, arith, N, Cin, Cout, H, W, gkind, leaky=leaky, kernels=conv_kernels(arith, dcm))
