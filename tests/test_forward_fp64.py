"""fp64 acceptance of the forward kernels, per element (the forward twin of tests/test_backward_fp64.py).

Every case runs the library, the fp32 oracle, the fp64 oracle and the magnitude bound M (oracle/ref_numpy.*_bound: per output element
the sum of |terms|) on the same seeded inputs, and asserts parity_cases.check_fp64_bound: max |got - fp64| / M within 4x the fp32
oracle's + 16 ulp, exact zeros where no term exists (a displacement that leaves the image, taps and samples outside), finite outputs.
Inputs are plain pc.feat features, 'graded-pixel' (10^U(-6,0) per pixel, one image at 1e-3) and 'graded-channel' (10^U(-6,0) per
channel): an error in a small element is invisible to the global check_close bar.  A fused LeakyReLU is compared with leaky(fp64)
under the same M (1-Lipschitz, keeps zeros).  Graded cases run without a bias (it would swamp M), and once with one scaled by 1e-7.
Each case runs under both arithmetics of its operator where the plan depends on it and asserts the kernel it reached.

CPU half: the real kernel sources on the emulation (tests/emu) at small shapes that take the same kernels.  `-m gpu`: the bench
pyramids (CFG2: 384x512 at batch 8, CFG3: 448x1024 at batch 4).  MFN_FWD_FP64_REPORT=<file> appends the maxima per case and
arithmetic to <file>.

Kernels the forward calls cannot reach, so no case names them: conv_s2d and conv_s2d_weights (stages of the transposed convolution's
BACKWARD only: the S2d cases of tests/test_backward_fp64.py)."""
import os

import numpy as np
import pytest

from oracle import ref as oracle
from oracle import ref_numpy
from tests import parity_cases as pc
from tests.fp64_env import Env, deform_offsets, exact_positions, per_image

ARITHS = [0, -1]                # ARITH_FP32, ARITH_DEFAULT
KINDS = ["plain", "graded-pixel", "graded-channel"]
_CACHE = {}
_RESULTS = []
SENTINEL = np.float32(-12345.5)


def _cached(key, make):
    """The oracle results (fp32, fp64, M) of one input set, shared by the runs under both arithmetics."""
    if key not in _CACHE:
        if len(_CACHE) > 6:
            _CACHE.clear()
        _CACHE[key] = make()
    return _CACHE[key]


def _check(what, arith, got, want64, ref32, M):
    e_lib, e_ref = pc.check_fp64_bound(got, want64, ref32, M, what=what)
    print("%-96s arith %-7s max e_lib %.3e   max e_ref32 %.3e" % (what, {0: "fp32", -1: "default", None: "-"}[arith], e_lib, e_ref))
    _RESULTS.append((what, arith, e_lib, e_ref))


def _leaky32(a):
    return np.where(a > 0, a, np.float32(0.1) * a).astype(np.float32)


def _leaky64(a):
    return np.where(a > 0, a, 0.1 * a)


class _tuned:
    """env.set_tuning(**kw) for the length of a block."""

    def __init__(self, env, kw):
        self.env, self.kw = env, kw or {}

    def __enter__(self):
        if self.kw:
            self.env.set_tuning(**self.kw)

    def __exit__(self, *exc):
        if self.kw:
            self.env.set_tuning(**{k: (-1 if k == "corr_variant" else 0) for k in self.kw})
        return False


# ---- correlation ---------------------------------------------------------------------------------------------------------------
def case_corr(env, arith, shape, md, kind, kernels, tuning=None, forms=("plain", "leaky", "into"), seed=0):
    N, C, H, W = shape
    D2 = (2 * md + 1) ** 2
    rng = np.random.default_rng(1700 + seed)
    f1, f2 = pc.graded_feat(rng, shape, kind), pc.graded_feat(rng, shape, kind)   # graded independently

    def make():
        kw = dict(max_displacement=md, pad_size=md)
        r32 = np.concatenate(per_image(lambda a, b: oracle.correlation(a, b, **kw), f1, f2))
        r64 = np.concatenate(per_image(lambda a, b: oracle.correlation(a, b, dtype=np.float64, **kw), f1, f2))
        M = ref_numpy.correlation_bound(f1, f2, md)
        # structural zeros: exactly the displacements that leave the image (no feature is 0)
        outside = sum(H * W - max(H - abs(dy), 0) * max(W - abs(dx), 0) for dy in range(-md, md + 1) for dx in range(-md, md + 1))
        assert int((M == 0).sum()) == N * outside
        return r32, r64, M

    ref32, want64, M = _cached(("corr", shape, md, kind, seed), make)
    env.set_arith("corr", arith)
    okw = dict(kernel_size=1, max_displacement=md, stride1=1, stride2=1, pad_size=md, is_multiply=True)
    d1, d2 = env.dev(f1), env.dev(f2)
    for form in forms:
        what = "corr %s md=%d %s %s %s" % (shape, md, kind, "+".join(kernels), form)
        with _tuned(env, tuning), env.launches() as L:
            if form == "into":   # the cost volume in its channel slice of a concat buffer
                c0, extra = 4, 7
                buf = env.dev(np.full((N, c0 + D2 + extra, H, W), SENTINEL, np.float32))
                env.ops.Correlation(d1, d2, activation="leaky", out=buf[:, c0:c0 + D2], **okw)
                full = env.host(buf)
                assert (full[:, :c0].view(np.uint32) == SENTINEL.view(np.uint32)).all() and \
                    (full[:, c0 + D2:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), "%s: wrote outside the slice" % what
                got = full[:, c0:c0 + D2]
            else:
                got = env.host(env.ops.Correlation(d1, d2, activation="leaky" if form == "leaky" else None, **okw))
        L.expect(kernels, what=what)
        if form == "plain":
            _check(what, arith, got, want64, ref32, M)
        else:
            _check(what, arith, got, _leaky64(want64), _leaky32(ref32), M)


# ---- deformable convolution ----------------------------------------------------------------------------------------------------
def _dc_oracles(x, off, w, b):
    r32 = np.concatenate(per_image(lambda xx, o: oracle.deformable_convolution(xx, o, w, b, kernel=(3, 3), pad=(1, 1)), x, off))
    r64 = np.concatenate(per_image(lambda xx, o: oracle.deformable_convolution(xx, o, w, b, kernel=(3, 3), pad=(1, 1), dtype=np.float64), x, off))
    Mz = np.concatenate(per_image(lambda xx, o: ref_numpy.deformable_convolution_bound(xx, o, w, None), x, off))
    return r32, r64, Mz


def _bias(rng, C, kind, bias):
    """plain: the usual bias; graded: none, or ('small') one scaled by 1e-7."""
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    if kind == "plain":
        return b
    return (b * np.float32(1e-7)).astype(np.float32) if bias == "small" else None


def _structural(what, got, Mz, b):
    """Outputs whose taps all fall outside: exactly the bias (exactly 0 without one)."""
    z = Mz == 0
    want = np.broadcast_to((b if b is not None else np.zeros(got.shape[1], np.float32))[None, :, None, None], got.shape)
    assert (got[z] == want[z]).all(), "%s: %d outputs without a tap inside differ from the bias" % (what, int((got[z] != want[z]).sum()))
    return int(z.sum())


def _names(kernel):
    """One kernel name, or the list of a call's launches."""
    return [kernel] if isinstance(kernel, str) else list(kernel)


def case_deform(env, arith, N, C, H, W, okind, kind, kernel, bias="usual", tuning=None, packed=False, seed=0):
    """The drop-in DeformableConvolution at offsets of `okind` on the exact_positions grid."""
    rng = np.random.default_rng(1800 + seed)
    x = pc.graded_feat(rng, (N, C, H, W), kind)
    w = pc.msra_weight(rng, C, C)
    b = _bias(rng, C, kind, bias)
    off = deform_offsets(rng, N, H, W, okind)
    r32, r64, Mz = _cached(("deform", (N, C, H, W), okind, kind, bias, seed), lambda: _dc_oracles(x, off, w, b))
    M = Mz + (np.abs(b.astype(np.float64))[None, :, None, None] if b is not None else 0.0)
    env.set_arith("deform", arith)
    what = "deform %s %s %s bias=%s %s%s" % ((N, C, H, W), okind, kind, bias if b is not None else "no", "+".join(_names(kernel)), " packed" if packed else "")
    kw = dict(kernel=(3, 3), pad=(1, 1), num_filter=C, no_bias=b is None)
    xd, od, wd, bd = env.dev(x), env.dev(off), env.dev(w), env.dev(b) if b is not None else None
    with _tuned(env, tuning):
        with env.launches() as L:
            got = env.host(env.ops.DeformableConvolution(xd, od, wd, bd, **kw))
        L.expect(_names(kernel), what=what)
        if packed:   # weights packed once give the per-call path's bits
            pk = env.ops.pack_deform_weights(wd, (N, C, H, W), kernel=(3, 3), pad=(1, 1))
            np.testing.assert_array_equal(env.host(env.ops.DeformableConvolution(xd, od, wd, bd, packed=pk, **kw)), got)
    nz = _structural(what, got, Mz, b)
    if okind in ("outside", "far"):
        assert nz > 0, what
    _check(what, arith, got, r64, r32, M)


def case_deform_flow(env, arith, N, C, H, W, kind, kernel, bias="usual", scale=20.0, stride=8.0, seed=0):
    """The fused-offset call (deformable_convolution_shared: the drop-in call's bits) and deformable_matching with mask, tradeoff and
    LeakyReLU, under a flow on a 2^-10 grid (flow * 20 / 8 exact: offsets on the exact_positions grid)."""
    rng = np.random.default_rng(1900 + seed)
    x = pc.graded_feat(rng, (N, C, H, W), kind)
    w = pc.msra_weight(rng, C, C)
    b = _bias(rng, C, kind, bias)
    fl = exact_positions(pc.flow_field(rng, N, H, W) * np.float32(stride / scale), 2.0 ** -10)
    off = oracle.offsets_from_flow(fl, scale, stride)
    assert (off == exact_positions(off)).all()
    mask = (rng.standard_normal((N, 1, H, W)) * 2).astype(np.float32)
    unit = rng.standard_normal((N, C, H, W))

    def make():
        r32, r64, Mz = _dc_oracles(x, off, w, b)
        Mb = Mz + (np.abs(b.astype(np.float64))[None, :, None, None] if b is not None else 0.0)
        tr = (unit * Mb).astype(np.float32)     # a tradeoff at each output's own scale: N(0,1) would swamp the graded outputs
        sig32 = np.float32(1) / (np.float32(1) + np.exp(-mask, dtype=np.float32))
        m32 = _leaky32(r32 * sig32 + tr)
        m64 = _leaky64(r64 / (1.0 + np.exp(-mask.astype(np.float64))) + tr.astype(np.float64))
        return r32, r64, Mz, Mb, tr, m32, m64, ref_numpy.matching_bound(Mb, mask, tr)

    r32, r64, Mz, Mb, tr, m32, m64, Mm = _cached(("flow", (N, C, H, W), kind, bias, seed), make)
    env.set_arith("deform", arith)
    what = "deform %s flow %s bias=%s %s" % ((N, C, H, W), kind, bias if b is not None else "no", "+".join(_names(kernel)))
    xd, fd, wd, bd = env.dev(x), env.dev(fl), env.dev(w), env.dev(b) if b is not None else None
    with env.launches() as L:
        got = env.host(env.ops.deformable_convolution_shared(xd, fd, scale, stride, wd, bd))
    L.expect(_names(kernel), absent=["offsets_from_flow", "offsets_from_flow_v4"], what=what + " shared")
    dropin = env.host(env.ops.DeformableConvolution(xd, env.dev(off), wd, bd, kernel=(3, 3), pad=(1, 1), num_filter=C, no_bias=b is None))
    np.testing.assert_array_equal(got, dropin, err_msg=what + ": the fused-offset call differs from the drop-in call")
    _structural(what, got, Mz, b)
    _check(what + " shared", arith, got, r64, r32, Mb)
    with env.launches() as L:
        got = env.host(env.ops.deformable_matching(xd, fd, scale, stride, wd, bd, env.dev(mask), env.dev(tr), leaky=True))
    L.expect(_names(kernel), what=what + " matching")
    _check(what + " matching", arith, got, m64, m32, Mm)


# ---- warp ----------------------------------------------------------------------------------------------------------------------
def case_warp(env, shape, clip, kind, pair=False, seed=0):
    """warp() (pair: GridGenerator('warp') + BilinearSampler, the clip applied to the grid in between) at the sample positions the
    grid arithmetic gives in fp32 -- the kernels' and the fp32 oracle's --, so that the fp32 oracle's error is arithmetic only."""
    N, C, H, W = shape
    rng = np.random.default_rng(2000 + seed)
    x = pc.graded_feat(rng, shape, kind)
    fl = pc.flow_field(rng, N, H, W, sigma=3.0)

    def make():
        pos = ref_numpy.warp_positions(fl, clip, np.float32)
        M = ref_numpy.warp_at(x, pos, bound=True)
        assert clip or (M == 0).any()      # samples outside: structural zeros
        return oracle.warp(x, fl, clip_grid=clip), ref_numpy.warp_at(x, pos), M

    ref32, want64, M = _cached(("warp", shape, clip, kind, seed), make)
    what = "%s %s clip=%s %s" % ("sampler pair" if pair else "warp", shape, clip, kind)
    with env.launches() as L:
        if pair:
            grid = env.ops.GridGenerator(env.dev(np.ascontiguousarray(fl[:, ::-1])), "warp")
            if clip:
                grid = env.dev(np.clip(env.host(grid), np.float32(-1), np.float32(1)))
            got = env.host(env.ops.BilinearSampler(env.dev(x), grid))
        else:
            got = env.host(env.ops.warp(env.dev(x), env.dev(fl), clip_grid=clip))
    L.expect(["grid_generator_warp", "bilinear_sampler"] if pair else ["warp_fwd_fast"], what=what)
    _check(what, None, got, want64, ref32, M)


# ---- convolution / deconvolution -----------------------------------------------------------------------------------------------
def _torch_conv(x, w, b, dtype, transposed, kw):
    import torch
    F = torch.nn.functional
    t = lambda a: None if a is None else torch.tensor(a, dtype=dtype)
    stride, pad, dil = kw.get("stride", (1, 1)), kw.get("pad", (1, 1) if transposed else (0, 0)), kw.get("dilate", (1, 1))
    if transposed:
        return F.conv_transpose2d(t(x), t(w), t(b), stride=stride, padding=pad, output_padding=kw.get("adj", (0, 0)), dilation=dil).numpy()
    return F.conv2d(t(x), t(w), t(b), stride=stride, padding=pad, dilation=dil).numpy()


def case_conv(env, arith, N, Cin, Cout, H, W, kind, kernels, leaky=False, bias="usual", transposed=False, tuning=None, seed=0, **kw):
    """Convolution / Deconvolution: want64 / ref32 / M = torch on the CPU in fp64 / fp32 / fp64 of |x|, |W|, |b|."""
    import torch
    rng = np.random.default_rng(2100 + seed)
    k = tuple(kw.get("kernel", (4, 4) if transposed else (3, 3)))
    x = pc.graded_feat(rng, (N, Cin, H, W), kind)
    w = (rng.standard_normal(((Cin, Cout) if transposed else (Cout, Cin)) + k) * np.sqrt(2.0 / (1.01 * Cin * (4 if transposed else k[0] * k[1])))).astype(np.float32)
    b = _bias(rng, Cout, kind, bias)
    if transposed:
        kw = dict(dict(stride=(2, 2), pad=(1, 1)), **kw)

    def make():
        ab = None if b is None else np.abs(b)
        return (_torch_conv(x, w, b, torch.float32, transposed, kw), _torch_conv(x, w, b, torch.float64, transposed, kw),
                _torch_conv(np.abs(x), np.abs(w), ab, torch.float64, transposed, kw))

    ref32, want64, M = _cached(("conv", (N, Cin, Cout, H, W), kind, bias, transposed, seed, tuple(sorted(kw.items()))), make)
    env.set_arith("conv", arith)
    op = env.ops.Deconvolution if transposed else env.ops.Convolution
    what = "%s %s %s %s leaky=%d bias=%s %s" % ("deconv" if transposed else "conv", (N, Cin, Cout, H, W), ",".join("%s=%s" % (a, v[0]) for a, v in sorted(kw.items())),
                                                kind, leaky, bias if b is not None else "no", "+".join(kernels))
    with _tuned(env, tuning), env.launches() as L:
        got = env.host(op(env.dev(x), env.dev(w), env.dev(b) if b is not None else None, num_filter=Cout, no_bias=b is None,
                          activation="leaky" if leaky else None, **kw))
    L.expect(kernels, what=what)
    if leaky:
        _check(what, arith, got, _leaky64(want64), _leaky32(ref32), M)
    else:
        _check(what, arith, got, want64, ref32, M)


def conv_runs(kind):
    """(leaky, bias) runs of one layer per input kind: plain -- no activation, the usual bias; graded-pixel -- with and without the
    fused LeakyReLU, no bias, and once a bias scaled by 1e-7; graded-channel -- LeakyReLU, no bias."""
    return {"plain": [(False, "usual")], "graded-pixel": [(False, "none"), (True, "none"), (True, "small")], "graded-channel": [(True, "none")]}[kind]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("MFN_FWD_FP64_REPORT")
    if path and _RESULTS:
        with open(path, "a") as f:
            for what, arith, e_lib, e_ref in _RESULTS:
                f.write("%-100s arith %-7s max e_lib %.3e   max e_ref32 %.3e   ratio %.3f\n" % (
                    what, {0: "fp32", -1: "default", None: "-"}[arith], e_lib, e_ref, e_lib / e_ref if e_ref > 0 else 0.0))


# ---- the rule sees what the global bar cannot (no kernel involved) ---------------------------------------------------------------
def test_per_element_rule_sees_what_the_global_bar_cannot():
    """A graded cost volume, library-sized (the fp64 result rounded to fp32), with (a) the 1e-3 image's outputs scaled by 1 + 1e-3,
    (b) one 4 x 8 tile of a quiet region zeroed, (c) 1e-30 in one structural zero: pc.check_close(tol=1e-5) passes each,
    check_fp64_bound raises on each."""
    shape, md = (2, 8, 12, 16), 4
    rng = np.random.default_rng(11)
    f1, f2 = pc.graded_feat(rng, shape, "graded-pixel"), pc.graded_feat(rng, shape, "graded-pixel")
    ref32 = oracle.correlation(f1, f2, max_displacement=md, pad_size=md)
    want64 = oracle.correlation(f1, f2, max_displacement=md, pad_size=md, dtype=np.float64)
    M = ref_numpy.correlation_bound(f1, f2, md)
    good = want64.astype(np.float32)
    pc.check_close(good, ref32, tol=1e-5)
    pc.check_fp64_bound(good, want64, ref32, M, what="untouched")
    top = np.abs(want64).max()
    a = good.copy()
    a[0] *= np.float32(1 + 1e-3)
    b = good.copy()
    ch = 40                                       # displacement (0, 0): no structural zero in the tile
    tiles = [(y, x) for y in range(0, 12, 4) for x in range(0, 16, 8)]
    y0, x0 = min(tiles, key=lambda t: np.abs(want64[0, ch, t[0]:t[0] + 4, t[1]:t[1] + 8]).max())
    assert 0 < np.abs(want64[0, ch, y0:y0 + 4, x0:x0 + 8]).max() < 1e-6 * top and (M[0, ch, y0:y0 + 4, x0:x0 + 8] > 0).all()
    b[0, ch, y0:y0 + 4, x0:x0 + 8] = 0.0
    c = good.copy()
    z = tuple(np.argwhere(M == 0)[0])
    c[z] = np.float32(1e-30)
    for name, bad in (("scaled image", a), ("zeroed tile", b), ("nonzero structural zero", c)):
        pc.check_close(bad, ref32, tol=1e-5, what=name)
        with pytest.raises(AssertionError):
            pc.check_fp64_bound(bad, want64, ref32, M, what=name)


# ---- CPU half: the emulation at small shapes that take the same kernels -----------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture
def _emu_defaults(emu):
    yield
    from tests.emu import emu_ops
    emu_ops.set_tuning(corr_gram=-1, dc_mma=-1, conv_mma=-1, conv_dcm=0, corr_variant=-1, corr_rows=0, corr_direct=0, dc_mt=0, dc_pt=0, dc_nw=0,
                       conv_pt=0)


# (tuning, shape, md, kernels): a forced corr.variant runs the same kernel under both arithmetics -- those run once
EMU_CORR_FORCED = [
    (dict(corr_variant=48, corr_direct=2), (1, 32, 10, 24), 4, ["corr_gram_v48"]),                    # 32 channels, 6-row items
    (dict(corr_variant=48, corr_direct=2, corr_rows=8), (2, 32, 13, 20), 4, ["corr_gram_v48"]),       # 8-row items, odd H
    (dict(corr_variant=48, corr_direct=2, corr_rows=2), (1, 64, 9, 24), 4, ["corr_gram_v48c2"]),      # 64 channels: the two-chunk K loop
    (dict(corr_variant=46, corr_direct=2, corr_rows=6), (1, 32, 7, 36), 2, ["corr_gram_v46"]),        # the fp32 matrix instruction, md = 2
    (dict(corr_variant=44, corr_direct=2), (1, 96, 5, 16), 4, ["corr_gramk"]),
    (dict(corr_variant=45, corr_direct=2), (1, 64, 4, 24), 2, ["corr_gramk"]),
    (dict(corr_variant=26, corr_direct=2), (1, 12, 6, 40), 4, ["corr_dma_v26"]),
    (dict(corr_direct=1), (2, 30, 6, 8), 4, ["corr_direct"]),
    (dict(corr_variant=6, corr_direct=2), (2, 32, 7, 16), 4, ["corr_tiled_v6", "corr_reduce"]),       # channel slices + reduce
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tuning,shape,md,kernels", EMU_CORR_FORCED, ids=lambda v: "+".join(v) if isinstance(v, list) else None)
def test_emu_correlation_kernels(emu, _emu_defaults, tuning, shape, md, kernels, kind):
    forms = ("plain", "leaky", "into") if kind == "graded-pixel" else ("plain",)
    case_corr(emu, -1, shape, md, kind, kernels, tuning=tuning, forms=forms)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arith", ARITHS)
def test_emu_correlation_plan(emu, _emu_defaults, arith, kind):
    """The plan's own choice at small shapes: a coarse-level band under the default arithmetic (the direct kernel under ARITH_FP32),
    the row-pair kernel where neither applies."""
    case_corr(emu, arith, (1, 96, 5, 16), 4, kind, ["corr_gramk"] if arith else ["corr_direct"], forms=("plain", "leaky"))
    case_corr(emu, arith, (1, 12, 6, 40), 2, kind, ["corr_dma_v26"], forms=("plain",), seed=1)


EMU_DC_KERNEL = {0: "dc_lds", -1: "dc_mma"}


@pytest.mark.parametrize("okind", ["smooth", "rough", "far", "outside", "pertap"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arith", ARITHS)
def test_emu_deform(emu, _emu_defaults, arith, kind, okind):
    case_deform(emu, arith, 1, 32, 8, 16, okind, kind, EMU_DC_KERNEL[arith], packed=okind == "smooth")
    if kind != "plain" and okind == "smooth":
        case_deform(emu, arith, 1, 32, 8, 16, okind, kind, EMU_DC_KERNEL[arith], bias="small")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arith", ARITHS)
def test_emu_deform_flow_and_matching(emu, _emu_defaults, arith, kind):
    case_deform_flow(emu, arith, 1, 32, 6, 8, kind, EMU_DC_KERNEL[arith])
    if kind == "graded-pixel":
        case_deform_flow(emu, arith, 1, 32, 6, 8, kind, EMU_DC_KERNEL[arith], bias="small")


# dc_mma_kernel's tilings (filter tiles per wave, pixel tiles per block, waves per block) and a channel count they divide
EMU_DCM_TILINGS = [(1, 4, 4, 32), (2, 3, 12, 64), (2, 2, 4, 64), (3, 1, 6, 96), (1, 1, 8, 128), (1, 1, 4, 64), (1, 1, 2, 32), (1, 1, 1, 48)]


@pytest.mark.parametrize("mt,pt,nw,C", EMU_DCM_TILINGS)
def test_emu_deform_matrix_core_tilings(emu, _emu_defaults, mt, pt, nw, C):
    """Every tiling of tests/test_emu_parity.py DCM_TILINGS once, graded-pixel input."""
    case_deform(emu, -1, 1, C, 6, 8, "smooth", "graded-pixel", "dc_mma", tuning=dict(dc_mt=mt, dc_pt=pt, dc_nw=nw))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clip", [False, True])
def test_emu_warp(emu, kind, clip):
    case_warp(emu, (2, 3, 8, 12), clip, kind)
    case_warp(emu, (2, 3, 8, 12), clip, kind, pair=True)


# (N, Cin, Cout, H, W, geometry, transposed, tuning, kernels under ARITH_FP32, kernels under the default arithmetic)
P1 = dict(pad=(1, 1))
EMU_CONV = [
    (1, 8, 32, 8, 16, P1, False, None, ["conv3x3_mfma"], ["conv3x3_bf16x3"]),
    (1, 6, 10, 11, 19, dict(pad=(1, 1), stride=(2, 2)), False, None, ["conv3x3_row_mfma"], ["conv3x3_bf16x3"]),      # stride 2
    (2, 37, 32, 6, 16, P1, False, dict(conv_dcm=2), ["conv3x3_mfma"], ["conv3x3_dcm"]),                                # dc_mma_kernel<CONV>
    (1, 20, 40, 5, 16, dict(pad=(2, 2), dilate=(2, 2)), False, None, ["conv3x3_mfma"], ["conv3x3_bf16x3"]),           # dilated
    (2, 6, 8, 7, 9, dict(kernel=(1, 1)), False, None, ["conv_generic"], ["conv_generic"]),
    (2, 37, 2, 6, 16, P1, False, None, ["conv3x3_few"], ["conv3x3_few"]),                                              # the two-filter head
    (2, 37, 1, 6, 16, P1, False, None, ["conv3x3_few"], ["conv3x3_few"]),                                              # the one-filter head
    (2, 9, 16, 5, 8, {}, True, None, ["deconv_as_conv3x3_mfma"], ["deconv_as_conv3x3_bf16x3"]),                       # 4x4 / stride 2 / pad 1
    (1, 4, 10, 6, 9, dict(pad=(0, 0)), True, None, ["deconv4x4_mfma"], ["deconv4x4_mfma"]),                           # 4x4 / stride 2, another padding
    # 3x3 / stride 2 / pad 1 / adj (1, 1), the strided layers' data gradient as a forward call: a packing kernel only with this adj, and the
    # workspace query takes none
    (1, 16, 8, 6, 8, dict(kernel=(3, 3), pad=(1, 1), adj=(1, 1)), True, None, ["deconv_as_conv3x3_mfma"], ["deconv_as_conv3x3_bf16x3"]),
]


def _conv_id(c):
    return "%s%s" % ("x".join(map(str, c[:5])), "_T" if c[6] else "") + "".join("_%s%d" % (k[0], v[0]) for k, v in sorted(c[5].items()))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", EMU_CONV, ids=_conv_id)
def test_emu_conv(emu, _emu_defaults, case, arith, kind):
    N, Cin, Cout, H, W, geo, transposed, tuning, k32, kdef = case
    if arith == 0 and k32 == kdef and kind != "graded-pixel":
        return   # one kernel under both arithmetics: the second pass repeats the first (graded-pixel still runs both)
    for leaky, bias in conv_runs(kind):
        case_conv(emu, arith, N, Cin, Cout, H, W, kind, k32 if arith == 0 else kdef, leaky=leaky, bias=bias, transposed=transposed,
                  tuning=tuning, **geo)


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
    _lib.set_tuning(corr_variant=-1, corr_rows=0, corr_direct=0, conv_dcm=0)


def _lv(cfg, level):
    return PYR[cfg][LEVEL[level]]


def plan_corr_kernel(cfg, level, md, arith):
    """The plan's cost-volume kernel per level: under the default arithmetic the Gram band (corr_gram_kernel at levels 2 and 3,
    corr_gramk_kernel at the coarse ones); under ARITH_FP32 the band on the fp32 matrix instruction at level 2, the FMA kernels above."""
    if arith != 0:
        return {2: "corr_gram_v48", 3: "corr_gram_v48c2"}.get(level, "corr_gramk")
    if level == 4:
        return "corr_dma_v31" if (cfg, md) == ("cfg3", 4) else "corr_dma_v26"
    return {2: "corr_gram_v46", 3: "corr_dma_v20", 5: "corr_dma_v26", 6: "corr_direct"}[level]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("md", [4, 2])
@pytest.mark.parametrize("cfg,level", [(c, l) for c in PYR for l in (6, 5, 4, 3, 2)])
def test_gpu_correlation_plan(gpu, _gpu_defaults, cfg, level, md, kind):
    forms = ("plain", "leaky", "into") if kind == "graded-pixel" else ("plain", "leaky")
    for arith in ARITHS:
        case_corr(gpu, arith, _lv(cfg, level), md, kind, [plan_corr_kernel(cfg, level, md, arith)], forms=forms)


GPU_CORR_FORCED = [
    (dict(corr_variant=48, corr_rows=8), (8, 32, 96, 128), 4, ["corr_gram_v48"]),          # the other item height
    (dict(corr_variant=48, corr_rows=6), (4, 32, 112, 256), 2, ["corr_gram_v48"]),
    (dict(corr_variant=48), (4, 64, 56, 128), 2, ["corr_gram_v48c2"]),
    (dict(corr_variant=46), (8, 32, 96, 128), 4, ["corr_gram_v46"]),
    (dict(corr_variant=44), (8, 128, 12, 16), 4, ["corr_gramk"]),
    (dict(corr_variant=45), (4, 96, 28, 64), 2, ["corr_gramk"]),
    (dict(corr_variant=16), (8, 32, 96, 128), 4, ["corr_dma_v16"]),
    (dict(corr_direct=1), (8, 196, 6, 8), 4, ["corr_direct"]),
    (dict(corr_variant=6, corr_direct=2), (8, 128, 12, 16), 4, ["corr_tiled_v6", "corr_reduce"]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tuning,shape,md,kernels", GPU_CORR_FORCED, ids=lambda v: "+".join(v) if isinstance(v, list) else None)
def test_gpu_correlation_kernels(gpu, _gpu_defaults, tuning, shape, md, kernels, kind):
    case_corr(gpu, -1, shape, md, kind, kernels, tuning=tuning, forms=("plain", "leaky", "into") if kind == "graded-pixel" else ("plain",))


GPU_DC_KERNEL = {0: "dc_lds", -1: "dc_mma"}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg,level,okind", [(c, l, "smooth") for c in PYR for l in (5, 4, 3, 2)]
                         + [(c, l, k) for c, l in (("cfg2", 4), ("cfg3", 2)) for k in ("rough", "far", "outside", "pertap")])
def test_gpu_deform(gpu, _gpu_defaults, cfg, level, okind, kind):
    N, C, H, W = _lv(cfg, level)
    for arith in ARITHS:
        case_deform(gpu, arith, N, C, H, W, okind, kind, GPU_DC_KERNEL[arith], packed=okind == "smooth")
        if kind == "graded-pixel" and okind == "smooth":
            case_deform(gpu, arith, N, C, H, W, okind, kind, GPU_DC_KERNEL[arith], bias="small")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg,level", [(c, l) for c in PYR for l in (5, 3, 2)])
def test_gpu_deform_flow_and_matching(gpu, _gpu_defaults, cfg, level, kind):
    N, C, H, W = _lv(cfg, level)
    for arith in ARITHS:
        case_deform_flow(gpu, arith, N, C, H, W, kind, GPU_DC_KERNEL[arith])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("shape", [(8, 3, 384, 512), (4, 3, 448, 1024)])
def test_gpu_warp(gpu, shape, clip, kind):
    case_warp(gpu, shape, clip, kind)
    case_warp(gpu, shape, clip, kind, pair=True)


GPU_CONV = [
    (8, 64, 32, 48, 64, P1, False, None, ["conv3x3_mfma"], ["conv3x3_dcm"]),                                           # a level-3 decoder layer
    (8, 96, 64, 24, 32, P1, False, None, ["conv3x3_mfma"], ["conv3x3_bf16x3"]),                                        # level 4
    (8, 64, 96, 48, 64, dict(pad=(1, 1), stride=(2, 2)), False, None, ["conv3x3_row_mfma"], ["conv3x3_bf16x3"]),      # conv4a
    (4, 128, 128, 56, 128, dict(pad=(4, 4), dilate=(4, 4)), False, None, ["conv3x3_mfma"], ["conv3x3_bf16x3"]),       # dc_conv3
    (8, 32, 32, 96, 128, dict(kernel=(1, 1)), False, None, ["conv_generic"], ["conv_generic"]),
    (4, 579, 2, 112, 256, P1, False, None, ["conv3x3_few"], ["conv3x3_few"]),                                          # pred_flow2
    (8, 529, 1, 12, 16, P1, False, None, ["conv3x3_few", "conv3x3_few_reduce"], ["conv3x3_few", "conv3x3_few_reduce"]),   # pred_mask5
    (8, 529, 16, 6, 8, {}, True, None, ["deconv_as_conv3x3_mfma"], ["deconv_as_conv3x3_bf16x3"]),                     # upfeat5
    (4, 563, 16, 56, 128, {}, True, None, ["deconv_as_conv3x3_mfma"], ["deconv_as_conv3x3_bf16x3"]),                  # upfeat2
    (8, 64, 16, 24, 32, dict(pad=(0, 0)), True, None, ["deconv4x4_mfma"], ["deconv4x4_mfma"]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", GPU_CONV, ids=_conv_id)
def test_gpu_conv(gpu, _gpu_defaults, case, kind):
    N, Cin, Cout, H, W, geo, transposed, tuning, k32, kdef = case
    for arith in ARITHS:
        for leaky, bias in conv_runs(kind):
            case_conv(gpu, arith, N, Cin, Cout, H, W, kind, k32 if arith == 0 else kdef, leaky=leaky, bias=bias, transposed=transposed,
                      tuning=tuning, **geo)
