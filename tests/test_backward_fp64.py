"""fp64 acceptance of the backward kernels, per element.

Every case runs the library, the fp32 oracle (the MXNet-faithful loops of oracle/mfn_ref_body.inc), the fp64 oracle and the
magnitude bound M (oracle/ref_numpy.*_bound: per element, the sum of |terms|) on the same seeded inputs, and asserts
parity_cases.check_fp64_bound: max |got - fp64| / M within 4x the fp32 oracle's + 16 ulp, exact zeros where no term exists,
finite outputs.  Output gradients are plain N(0,1) and graded (10^U(-6,0) per pixel, one image at 1e-3): an error in a small
element is invisible to the global check_close bar.  Each case runs under both arithmetics of its operator (ARITH_FP32 and the
default) and asserts the kernel it reached, so that a plan change cannot move it onto a fallback unnoticed.

CPU half: the real kernel sources on the emulation (tests/emu) at small shapes that take the same kernels.  `-m gpu`: the
bench pyramids (CFG2: 384x512 at batch 8, CFG3: 448x1024 at batch 4); the convolution backward's routes at the smallest shapes that
reach their production kernels.  MFN_BWD_FP64_REPORT=<file> appends the maxima per case and arithmetic to <file>.

mfn_conv2d_bwd, route -> case (EMU_CONV_ROUTES on the emulation, GPU_CONV_ROUTES on the GPU; each asserts its kernels and that no other
kernel of the same family ran):
  data gradient   ConvBwdData::S2d     s2d_8, s2d_32, s2d_add / _nwn / _wna                   upfeat_96, upflow_64, upfeat_96_add
                  ConvBwdData::Conv    conv_t3_adj11, conv_t4_p0, conv_add / _nwn / _wna      transposed_3x3_adj11
                  ConvBwdData::Flip    test_emu_conv_backward, flip_*, head*                  test_gpu_conv_backward, dilated_*, w36_*, head_3
                  ConvBwdData::Deconv  deconv_adj11 / 01 / 00, deconv_add / _nwn / _wna       conv3a_s2*, conv6a_s2
  weight gradient conv_wgrad*          test_emu_conv_backward, flip_d2_w16, flip_d4_w16, head test_gpu_conv_backward, dilated_d4, head_3
                  DcBwdW::PcSlabs      flip_w12_pc, flip_nwn, generic4_wgrad                  w36_pc, w36_nwn
                  DcBwdW::Mfma         every strided and transposed case, flip_d*_w12         the same, dilated_d2_w36
                  DcBwdW::Generic      generic2_wgrad (path.generic = 2)                      -
  bias            channel_sum          nearly every case                                      the same
                  channel_sum_partial + channel_sum_final   flip_bias_partial, flip_wna      upflow_64
(DcBwdW::Pc, the same kernel summing through atomics where the slabs do not fit, cannot be reached from mfn_conv2d_bwd: its workspace
always holds the slabs.)  path.generic = 4 moves a call off S2d and off conv_wgrad: generic4_s2d, generic4_wgrad."""
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
def case_corr_bwd(env, arith, shape, md, gkind, req="write", seed=0, kernels=("corr_bwd_lds",), reqs=None):
    """reqs: (req of g1, req of g2), 'write' or 'null' each, in place of `req` for both: a gradient that is not asked for comes back None."""
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
        elif reqs is not None:
            g1, g2 = env.ops.Correlation_backward(env.dev(go), env.dev(f1), env.dev(f2), 1, md, 1, 1, md, True, req1=reqs[0], req2=reqs[1])
        else:
            g1, g2 = env.ops.Correlation_backward(env.dev(go), env.dev(f1), env.dev(f2), 1, md, 1, 1, md, True)
    what = "corr bwd %s md=%d %s %s" % (shape, md, gkind, req if reqs is None else "/".join(reqs))
    L.expect(list(kernels), what=what)
    for g, w64, r32, m, b, nm, rq in zip((g1, g2), want64, ref32, M, base, ("g1", "g2"), reqs or (req, req)):
        if rq == "null":
            assert g is None, "%s %s: req null, but an output came back" % (what, nm)
            continue
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


def case_deform_flow_bwd(env, arith, N, C, H, W, gkind, scale=20.0, stride=8.0, seed=0, kernels=None, req=("write",) * 4):
    """mfn_deform_conv_shared_bwd in flow mode: d/dflow = scale / stride * sum over the taps, against the summed bound.  kernels: the
    call's launches where they are not the bench levels'; req: (gx, gflow, gw, gbias), 'write' or 'null' each."""
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
        got = env.ops.deformable_convolution_shared_backward(env.dev(go), env.dev(x), env.dev(fl), scale, stride, env.dev(w), req=tuple(req))
    what = "deform flow bwd %s %s%s" % ((N, C, H, W), gkind, "" if tuple(req) == ("write",) * 4 else " req=" + "".join(r[0] for r in req))
    if kernels is None:
        L.expect(["dc_bwd_input_pix", "dc_bwd_weight_pc"], absent=["offsets_from_flow"], what=what)
    else:
        L.expect(list(kernels), what=what)
    for g, w64, r32, m, nm, rq in zip(got, want64, ref32, M, ("gx", "gflow", "gw", "gbias"), req):
        if rq == "null":
            assert g is None, "%s %s: req null, but an output came back" % (what, nm)
            continue
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


def _torch_conv(tx, tw, tb, geo):
    import torch
    F = torch.nn.functional
    if geo["transposed"]:
        return F.conv_transpose2d(tx, tw, tb, stride=geo["stride"], padding=geo["pad"], output_padding=geo["adj"], dilation=geo["dilate"])
    return F.conv2d(tx, tw, tb, stride=geo["stride"], padding=geo["pad"], dilation=geo["dilate"])


def _torch_conv_grads(x, w, b, gpre, dtype, geo):
    """torch autograd of conv2d / conv_transpose2d on the CPU: (gx, gw, gbias or None)."""
    import torch
    tx = torch.tensor(x, dtype=dtype, requires_grad=True)
    tw = torch.tensor(w, dtype=dtype, requires_grad=True)
    tb = torch.tensor(b, dtype=dtype, requires_grad=True) if b is not None else None
    _torch_conv(tx, tw, tb, geo).backward(torch.tensor(gpre, dtype=dtype))
    return tx.grad.numpy(), tw.grad.numpy(), tb.grad.numpy() if tb is not None else None


WWW = ("write", "write", "write")


def _conv_geo(kernel=(3, 3), stride=(1, 1), pad=(1, 1), dilate=(1, 1), transposed=False, adj=(0, 0)):
    return dict(kernel=tuple(kernel), stride=tuple(stride), pad=tuple(pad), dilate=tuple(dilate), transposed=bool(transposed), adj=tuple(adj))


def _conv_out_hw(H, W, geo):
    ext = [d * (k - 1) + 1 for d, k in zip(geo["dilate"], geo["kernel"])]
    if geo["transposed"]:
        return tuple((v - 1) * s - 2 * p + e + a for v, s, p, e, a in zip((H, W), geo["stride"], geo["pad"], ext, geo["adj"]))
    return tuple((v + 2 * p - e) // s + 1 for v, s, p, e in zip((H, W), geo["stride"], geo["pad"], ext))


def _conv_problem(N, Cin, Cout, H, W, gkind, seed, geo, bias=True):
    """Seeded inputs of one layer: features, weights in the operator's own layout, bias (or None), the output gradient."""
    rng = np.random.default_rng(1000 + seed)
    kh, kw = geo["kernel"]
    x = pc.feat(rng, (N, Cin, H, W))
    wshape = (Cin, Cout, kh, kw) if geo["transposed"] else (Cout, Cin, kh, kw)
    w = (rng.standard_normal(wshape) * np.sqrt(2.0 / (1.01 * Cin * kh * kw))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    go = _gout(rng, (N, Cout) + _conv_out_hw(H, W, geo), gkind)
    return rng, x, w, b if bias else None, go


def _conv_refs(x, w, b, go, geo, y64=None):
    """(ref32, want64, M): torch autograd in fp32, in fp64, and in fp64 on the absolute values; y64: the fp64 pre-activation of a fused
    LeakyReLU, whose sign gives the slope."""
    import torch
    g64 = go.astype(np.float64) * (1.0 if y64 is None else np.where(y64 > 0, 1.0, 0.1))
    g32 = go if y64 is None else np.where(y64 > 0, go, np.float32(0.1) * go).astype(np.float32)
    ab = None if b is None else np.abs(b)
    return (_torch_conv_grads(x, w, b, g32, torch.float32, geo), _torch_conv_grads(x, w, b, g64, torch.float64, geo),
            _torch_conv_grads(np.abs(x), np.abs(w), ab, np.abs(g64), torch.float64, geo))


def case_conv_bwd(env, arith, N, Cin, Cout, H, W, gkind, leaky=False, kernels=(), seed=0, kernel=(3, 3), stride=(1, 1), pad=(1, 1),
                  dilate=(1, 1), transposed=False, adj=(0, 0), bias=True, req=WWW, absent=(), tuning=None, zeros=False):
    """mfn_conv2d_bwd of any geometry: want64 = torch fp64 autograd of conv2d / conv_transpose2d, ref32 = the same in fp32, M = the fp64
    autograd on |x|, |W|, |b| and |the gradient behind the LeakyReLU| (the slope from the sign of the fp64 pre-activation).  req 'add':
    the caller's values are N(0,1) * M; req 'null': the output comes back None.  zeros: the case is there for its structural zeros."""
    import torch
    geo = _conv_geo(kernel, stride, pad, dilate, transposed, adj)
    rng, x, w, b, go = _conv_problem(N, Cin, Cout, H, W, gkind, seed, geo, bias)
    env.set_arith("conv", arith)
    okw = dict(kernel=geo["kernel"], stride=geo["stride"], pad=geo["pad"], dilate=geo["dilate"], no_bias=b is None)
    if transposed:
        okw["adj"] = geo["adj"]
    fwd, bwd = (env.ops.Deconvolution, env.ops.Deconvolution_backward) if transposed else (env.ops.Convolution, env.ops.Convolution_backward)
    y = y64 = None
    if leaky:
        t64 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)
        y64 = _torch_conv(t64(x), t64(w), t64(b), geo).numpy()
        y = fwd(env.dev(x), env.dev(w), env.dev(b) if b is not None else None, activation="leaky", **okw)
        # the kernel takes the slope from ITS forward output: an input whose pre-activation rounds across zero would measure that, not the backward
        assert ((env.host(y) > 0) == (y64 > 0)).all(), "the forward output and the fp64 pre-activation differ in sign: take another seed"

    make = lambda: _conv_refs(x, w, b, go, geo, y64)
    ref32, want64, M = _cached(("conv", (N, Cin, Cout, H, W), leaky, gkind, seed, tuple(sorted(geo.items())), b is not None), make)
    what = " ".join(p for p in ("deconv bwd" if transposed else "conv bwd", str((N, Cin, Cout, H, W)), _geo_name(geo), "leaky=%s" % leaky, gkind,
                                "" if b is not None else "no bias", "" if tuple(req) == WWW else "req=" + "".join(r[0] for r in req)) if p)
    names = ("gx", "gw", "gbias")
    for m, w64, nm in zip(M, want64, names):
        if m is not None:
            pc.assert_magnitude_bound(m, w64, what="%s %s" % (what, nm))
    if zeros:
        assert (M[1] == 0).sum() > 0, "%s: the case has lost its structural zeros" % what
    base = [(rng.standard_normal(m.shape) * m).astype(np.float32) if (r == "add" and m is not None) else None for r, m in zip(req, M)]
    out = tuple(env.dev(a.copy()) if a is not None else None for a in base)
    if tuning:
        env.set_tuning(**tuning)
    try:
        with env.launches() as L:
            got = bwd(env.dev(go), env.dev(x), env.dev(w), output=y, activation="leaky" if leaky else None, req=req,
                      out=out if any(o is not None for o in out) else None, **okw)
    finally:
        if tuning:
            env.set_tuning(**{k: 0 for k in tuning})
    L.expect(kernels, absent=absent, what=what)
    for g, w64, r32, m, r, b0, nm in zip(got, want64, ref32, M, req, base, names):
        if r == "null" or m is None:
            assert g is None, "%s %s: req null / no bias, but an output came back" % (what, nm)
            continue
        _check("%s %s" % (what, nm), arith, env.host(g), w64, r32, m, base=b0)


def _geo_name(geo):
    """'' for 3x3 / stride 1 / pad 1 / dilation 1 (the cases that were here first keep their names in the report)."""
    dflt = dict(kernel=(3, 3), stride=(1, 1), pad=(1, 1), dilate=(1, 1), transposed=False, adj=(0, 0))
    short = dict(kernel="k", stride="s", pad="p", dilate="d", adj="adj")
    parts = ["%s%s" % (short[k], "x".join(map(str, v)) if k == "adj" else v[0]) for k, v in geo.items() if k in short and v != dflt[k]]
    return " ".join(parts)


def conv_kernels(arith, dcm):
    """Kernels of a 3x3 / stride 1 / dilation 1 backward with W % 16 == 0: the weight gradient on the bf16 x 3 matrix-core kernel under
    the default arithmetic (the fp32 MFMA one under ARITH_FP32), the data gradient on dc_mma_kernel<CONV> where the plan takes it."""
    if arith == 0:
        return ("conv_wgrad",)
    return ("conv_wgrad_bf16x3",) + (("conv3x3_dcm",) if dcm else ())


# The kernels mfn_conv2d_bwd chooses among, by what they compute.  A case names the ones its route reaches; every other one of the same family
# must not have run, so that two routes cannot be mistaken for each other.
DATA_KERNELS = ("conv_s2d", "conv_s2d_weights", "conv_flip_weights", "conv_generic", "conv3x3_mfma", "conv3x3_row_mfma", "conv3x3_bf16x3",
                "conv3x3_dcm", "conv3x3_few", "deconv_as_conv3x3_mfma", "deconv_as_conv3x3_row_mfma", "deconv_as_conv3x3_bf16x3", "deconv4x4_mfma")
WGRAD_KERNELS = ("conv_wgrad", "conv_wgrad_bf16x3", "dc_bwd_weight_mfma", "dc_bwd_weight_pc", "dc_bwd_weight_reduce", "dc_bwd_weight")
BIAS_KERNELS = ("channel_sum", "channel_sum_partial", "channel_sum_final")
S2D, FLIP = ("conv_s2d", "conv_s2d_weights"), ("conv_flip_weights",)
PC = ("dc_bwd_weight_pc", "dc_bwd_weight_reduce")
SUM1, SUM2 = ("channel_sum",), ("channel_sum_partial", "channel_sum_final")
T4 = dict(transposed=True, kernel=(4, 4), stride=(2, 2), pad=(1, 1))            # the network's transposed convolution
T3 = dict(transposed=True, kernel=(3, 3), stride=(2, 2), pad=(1, 1), adj=(1, 1))
S2 = dict(stride=(2, 2))
D2, D4 = dict(dilate=(2, 2), pad=(2, 2)), dict(dilate=(4, 4), pad=(4, 4))
AAA, NWN, WNA = ("add", "add", "add"), ("null", "write", "null"), ("write", "null", "add")


def conv_route(env, arith, data, wgrad, bias, req=WWW, has_bias=True):
    """(kernels, absent) of a case: `data` / `wgrad` are (under ARITH_FP32, under the default arithmetic) or one tuple for both; an output
    that is not requested launches none of its family.  The GPU's launch counters match names by substring: there a name inside an
    expected one cannot be asked to be absent."""
    pick = lambda k: k[0 if arith == 0 else 1] if k and isinstance(k[0], tuple) else k
    want = (pick(data) if req[0] != "null" else ()) + (pick(wgrad) if req[1] != "null" else ()) + (bias if req[2] != "null" and has_bias else ())
    absent = [k for k in DATA_KERNELS + WGRAD_KERNELS + BIAS_KERNELS if k not in want and (env.emu or not any(k in e for e in want))]
    return want, absent


def run_conv_route(env, arith, gkind, case):
    shape, kw, data, wgrad, bias = case
    kw = dict(kw)
    kernels, absent = conv_route(env, arith, data, wgrad, bias, kw.get("req", WWW), kw.get("bias", True))
    case_conv_bwd(env, arith, *shape, gkind, kernels=kernels, absent=absent, seed=3, **kw)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MFN_BWD_FP64_REPORT")
    if path and _RESULTS:
        with open(path, "a") as f:
            for what, arith, e_lib, e_ref in _RESULTS:
                f.write("%-80s arith %-7s max e_lib %.3e   max e_ref32 %.3e   ratio %.3f\n" % (
                    what, {0: "fp32", -1: "default", None: "-"}[arith], e_lib, e_ref, e_lib / e_ref if e_ref > 0 else 0.0))


# ---- the rule sees what the global bar cannot (no kernel involved) ---------------------------------------------------------------
def _library_sized(N, Cin, Cout, H, W, geo):
    """A graded layer's references and a library-sized result (the fp64 gradients rounded to fp32)."""
    _, x, w, b, go = _conv_problem(N, Cin, Cout, H, W, "graded", 7, geo)
    ref32, want64, M = _conv_refs(x, w, b, go, geo)
    good = [a.astype(np.float32) for a in want64]
    for g, w64, r32, m, nm in zip(good, want64, ref32, M, ("gx", "gw", "gbias")):
        pc.assert_magnitude_bound(m, w64)
        pc.check_close(g, w64, tol=2e-5)
        pc.check_fp64_bound(g, w64, r32, m, what="untouched " + nm)
    return x, w, b, go, ref32, want64, M, good


def _accepted_globally_rejected_per_element(name, bad, want64, ref32, M):
    pc.check_close(bad, want64, tol=2e-5, what=name)
    with pytest.raises(AssertionError):
        pc.check_fp64_bound(bad, want64, ref32, M, what=name)


@pytest.mark.parametrize("layer", ["strided", "transposed"])
def test_per_element_rule_sees_what_the_global_bar_cannot(layer):
    """A strided and a transposed layer under the graded gradient, library-sized.  (a) One weight element loses what the quiet image (the
    one scaled by 1e-3) adds to it: among the elements where that is at most 1e-5 of max |gw|, half of what check_close(2e-5) lets through,
    the one where it is largest against M.  (b) One gx element of the quietest pixel moves by 2^-12 M.  parity_cases.check_close(2e-5),
    the bar of case_conv_backward, accepts both; check_fp64_bound raises on both."""
    import torch
    geo = _conv_geo(stride=(2, 2)) if layer == "strided" else _conv_geo(**T4)
    x, w, b, go, ref32, want64, M, good = _library_sized(2, 16, 8, 12, 16, geo)
    quiet = go.copy()
    quiet[1:] = 0
    share = _torch_conv_grads(x, w, b, quiet, torch.float64, geo)[1]                # the quiet image's share of gw
    gw0 = np.abs(share)
    ok = (gw0 > 0) & (gw0 <= 1e-5 * np.abs(want64[1]).max())
    assert ok.any()
    e = np.unravel_index(np.argmax(np.where(ok, gw0 / M[1], 0.0)), gw0.shape)
    assert gw0[e] / M[1][e] > 2.0 ** -16                                             # far above any fp32 rounding
    a = good[1].copy()
    a[e] = np.float32(want64[1][e] - share[e])
    _accepted_globally_rejected_per_element("dropped tap", a, want64[1], ref32[1], M[1])
    c = good[0].copy()
    q = np.unravel_index(np.argmin(np.where(M[0] > 0, M[0], np.inf)), M[0].shape)
    assert M[0][q] < 1e-3 * np.abs(want64[0]).max()                                  # a quiet pixel: 2^-12 M there is nothing to the global bar
    c[q] = np.float32(want64[0][q] + 2.0 ** -12 * M[0][q])
    _accepted_globally_rejected_per_element("quiet pixel", c, want64[0], ref32[0], M[0])


def test_per_element_rule_sees_a_nonzero_structural_zero():
    """Dilation 4 on four rows: the kernel rows 0 and 2 only ever read padding.  1e-30 in one of those weight gradients passes
    check_close(2e-5) and is rejected by check_fp64_bound."""
    x, w, b, go, ref32, want64, M, good = _library_sized(1, 4, 8, 4, 12, _conv_geo(**D4))
    assert (M[1][:, :, (0, 2)] == 0).all() and (M[1][:, :, 1] > 0).all()
    bad = good[1].copy()
    bad[3, 2, 0, 1] = np.float32(1e-30)
    _accepted_globally_rejected_per_element("nonzero structural zero", bad, want64[1], ref32[1], M[1])


# ---- CPU half: the emulation at small shapes that take the same kernels -----------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture
def _emu_defaults(emu):
    yield
    from tests.emu import emu_ops
    emu_ops.set_tuning(corr_gram=-1, dc_mma=-1, conv_mma=-1, bwd_off=0, conv_dcm=0, path_generic=0)


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


MM, BF = ("conv3x3_mfma",), ("conv3x3_bf16x3",)
DECONV11 = (("deconv_as_conv3x3_mfma",), ("deconv_as_conv3x3_bf16x3",))
GEN, WMFMA, WOWN = ("conv_generic",), ("dc_bwd_weight_mfma",), (("conv_wgrad",), ("conv_wgrad_bf16x3",))
# (N, Cin, Cout, H, W), geometry / requests, data-gradient kernels, weight-gradient kernels, bias kernels
EMU_CONV_ROUTES = {
    "deconv_adj11": ((1, 8, 16, 12, 16), S2, DECONV11, WMFMA, SUM1),
    "deconv_adj01": ((2, 8, 16, 13, 18), dict(S2, leaky=True), GEN, WMFMA, SUM1),
    "deconv_adj00": ((1, 8, 16, 13, 17), S2, GEN, WMFMA, SUM1),
    "s2d_8": ((2, 8, 4, 4, 8), dict(T4, leaky=True), (S2D + MM, S2D + BF), WMFMA, SUM1),
    "s2d_32": ((2, 32, 16, 6, 8), dict(T4, leaky=True), (S2D + MM, S2D + BF), WMFMA, SUM1),
    "conv_t3_adj11": ((1, 16, 8, 6, 8), dict(T3, leaky=True), (("conv3x3_row_mfma",), BF), WMFMA, SUM1),   # its forward: the adj-aware workspace query
    "conv_t4_p0": ((1, 16, 8, 6, 8), dict(T4, pad=(0, 0)), GEN, WMFMA, SUM1),
    "flip_d2_w16": ((1, 4, 8, 12, 16), dict(D2, leaky=True), (FLIP + MM, FLIP + BF), ("conv_wgrad",), SUM1),
    "flip_d2_w12": ((1, 4, 8, 12, 12), dict(D2, leaky=True), (FLIP + MM, FLIP + BF), WMFMA, SUM1),
    "flip_d4_w16": ((1, 4, 8, 4, 16), dict(D4, zeros=True), (FLIP + MM, FLIP + BF), ("conv_wgrad",), SUM1),
    "flip_d4_w12": ((1, 4, 8, 4, 12), dict(D4, zeros=True), (FLIP + MM, FLIP + BF), WMFMA, SUM1),
    # W % 8 != 0 and the two-stage bias sum (more than 4096 output pixels), one small shape each in place of one (2, 4, 6, 40, 52)
    "flip_w12_pc": ((2, 4, 6, 8, 12), dict(leaky=True), (FLIP + MM, FLIP + BF), PC, SUM1),
    "flip_bias_partial": ((1, 4, 2, 65, 64), {}, FLIP + ("conv3x3_few",), WOWN, SUM2),
    "head": ((2, 8, 2, 8, 8), {}, (FLIP + MM, FLIP + BF), ("conv_wgrad",), SUM1),
    "head_no_bias": ((2, 8, 2, 8, 8), dict(bias=False), (FLIP + MM, FLIP + BF), ("conv_wgrad",), SUM1),
    # the request modes, once per data route
    "deconv_add": ((1, 8, 16, 12, 16), dict(S2, req=AAA), DECONV11, WMFMA, SUM1),
    "deconv_nwn": ((1, 8, 16, 12, 16), dict(S2, req=NWN), DECONV11, WMFMA, SUM1),
    "deconv_wna": ((2, 8, 16, 13, 18), dict(S2, leaky=True, req=WNA), GEN, WMFMA, SUM1),
    "s2d_add": ((2, 8, 4, 4, 8), dict(T4, leaky=True, req=AAA), (S2D + MM, S2D + BF), WMFMA, SUM1),
    "s2d_nwn": ((2, 8, 4, 4, 8), dict(T4, req=NWN), (S2D + MM, S2D + BF), WMFMA, SUM1),
    "s2d_wna": ((2, 8, 4, 4, 8), dict(T4, req=WNA), (S2D + MM, S2D + BF), WMFMA, SUM1),
    "conv_add": ((1, 16, 8, 6, 8), dict(T3, req=AAA), (("conv3x3_row_mfma",), BF), WMFMA, SUM1),
    "conv_nwn": ((1, 16, 8, 6, 8), dict(T4, pad=(0, 0), req=NWN), GEN, WMFMA, SUM1),
    "conv_wna": ((1, 16, 8, 6, 8), dict(T3, leaky=True, req=WNA), (("conv3x3_row_mfma",), BF), WMFMA, SUM1),
    "flip_d4_w12_add": ((1, 4, 8, 4, 12), dict(D4, zeros=True, req=AAA), (FLIP + MM, FLIP + BF), WMFMA, SUM1),   # the structural zeros keep the base
    "flip_d4_w16_add": ((1, 4, 8, 4, 16), dict(D4, zeros=True, req=AAA), (FLIP + MM, FLIP + BF), ("conv_wgrad",), SUM1),
    "flip_nwn": ((2, 4, 6, 8, 12), dict(req=NWN), (FLIP + MM, FLIP + BF), PC, SUM1),
    "flip_wna": ((1, 4, 2, 65, 64), dict(req=WNA), FLIP + ("conv3x3_few",), WOWN, SUM2),
    # path.generic = 4: off S2d (the Conv route's generic kernel) and off conv_wgrad; path.generic = 2: the generic deformable weight gradient
    "generic4_s2d": ((2, 8, 4, 4, 8), dict(T4, leaky=True, tuning=dict(path_generic=4)), GEN, WMFMA, SUM1),
    "generic4_wgrad": ((1, 8, 32, 8, 16), dict(tuning=dict(path_generic=4)), FLIP + GEN, PC, SUM1),
    "generic2_wgrad": ((1, 4, 8, 12, 12), dict(D2, tuning=dict(path_generic=2)), (FLIP + MM, FLIP + BF), ("dc_bwd_weight",), SUM1),
}


@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", list(EMU_CONV_ROUTES))
def test_emu_conv_backward_routes(emu, _emu_defaults, name, arith, gkind):
    run_conv_route(emu, arith, gkind, EMU_CONV_ROUTES[name])


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


# The smallest shapes that reach each route's production kernels (kernel names from the emulation's dry run of the same calls).
GPU_CONV_ROUTES = {
    "conv3a_s2": ((2, 32, 64, 48, 64), dict(S2, leaky=True), DECONV11, WMFMA, SUM1),                        # adj (1, 1)
    "conv6a_s2": ((2, 128, 196, 12, 16), dict(S2, leaky=True), DECONV11, WMFMA, SUM1),
    "conv3a_s2_47x63": ((2, 32, 64, 47, 63), S2, GEN, WMFMA, SUM1),                                          # adj (0, 0)
    "conv3a_s2_48x63": ((2, 32, 64, 48, 63), dict(S2, leaky=True), GEN, WMFMA, SUM1),                        # adj (1, 0)
    "conv3a_s2_wna": ((2, 32, 64, 48, 64), dict(S2, req=WNA), DECONV11, WMFMA, SUM1),
    "upfeat_96": ((2, 96, 16, 12, 16), dict(T4, leaky=True), (S2D + MM, S2D + BF), WMFMA, SUM1),
    "upflow_64": ((2, 64, 2, 24, 32), T4, (S2D + MM, S2D + BF), WMFMA, SUM2),
    "upfeat_96_add": ((2, 96, 16, 12, 16), dict(T4, req=AAA), (S2D + MM, S2D + BF), WMFMA, SUM1),
    "transposed_3x3_adj11": ((2, 64, 32, 12, 16), dict(T3, leaky=True), (("conv3x3_row_mfma",), BF), WMFMA, SUM1),
    "dilated_d4": ((1, 128, 128, 24, 32), dict(D4, leaky=True), (FLIP + MM, FLIP + BF), ("conv_wgrad",), SUM1),
    "dilated_d2_w36": ((1, 64, 64, 24, 36), dict(D2, leaky=True), (FLIP + MM, FLIP + BF), WMFMA, SUM1),
    "dilated_d4_h4_add": ((1, 128, 128, 4, 32), dict(D4, zeros=True, req=AAA), (FLIP + MM, FLIP + BF), ("conv_wgrad",), SUM1),
    "w36_pc": ((2, 64, 32, 24, 36), dict(leaky=True), (FLIP + MM, FLIP + BF), PC, SUM1),
    "w36_nwn": ((2, 64, 32, 24, 36), dict(req=NWN), (FLIP + MM, FLIP + BF), PC, SUM1),
    "head_3": ((2, 64, 3, 24, 32), {}, (FLIP + MM, FLIP + BF), WOWN, SUM1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("gkind", GOUTS)
@pytest.mark.parametrize("name", list(GPU_CONV_ROUTES))
def test_gpu_conv_backward_routes(gpu, _gpu_defaults, name, gkind):
    for arith in ARITHS:
        run_conv_route(gpu, arith, gkind, GPU_CONV_ROUTES[name])
