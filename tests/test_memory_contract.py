"""Where every kernel reads and writes: each call once through the plain OpSet and twice through tests/guarded.py (every buffer between
guard bands, every workspace a fresh allocation of exactly the queried size holding a NaN pattern).

Per case:
  (a) status OK and the guarded runs reached the plain run's kernels in the same order (and the kernels the case names: Launches.expect);
  (b) every band is intact (guarded.verify);
  (c) deterministic routes: the guarded results are the plain run's bits.  Routes the header promises "up to summation order" (gx and
      goffset of the deformable backward; weight -- and with it bias -- gradients summed through atomics: more than 96 filters, W % 4 != 0,
      no slabs) meet parity_cases.check_fp64_bound unchanged, against the oracles of tests/test_backward_fp64.py.  Three more results are
      scattered through fp32 atomics and the header says nothing about their bits (found here: their bits change from call to call): gx
      of mfn_warp_bwd, gdata of mfn_bilinear_sampler_bwd, and both gradients of mfn_correlation_bwd outside the reference geometry
      (corr_bwd_scatter).  They answer to the same bound, M being the sum of |terms| (the same gradient of absolute values);
  (d) no NaN in any result (a read of an input's band or of a workspace's stale contents that reaches a result);
  (e) a gradient whose req is null, given as a real banded buffer (the raw-ABI calls of the backward cases), keeps its fill;
  (f) the second guarded call, whose workspaces hold another stale pattern, gives the first one's bits on the deterministic routes.
Shapes, tunings and kernel names come from the tables of the fp64 and dispatch files; inputs are their `plain` kind: this file is
about addresses, not arithmetic.  The CPU half runs the table on the emulation, the GPU half (-m gpu) the same table at the same shapes.
The self-tests at the end show, with a fake operator in numpy, that each defect the harness is there for fails it."""
import ctypes

import numpy as np
import pytest

from oracle import ref as oracle
from oracle import ref_numpy
from maskflownet_amd.ops import OpSet
from tests import guarded as G
from tests import parity_cases as pc
from tests import test_backward_fp64 as tb
from tests import test_forward_fp64 as tf
from tests.fp64_env import Env, deform_offsets, exact_positions
from tests.test_dispatch_table import CORR_BWD_REQS, DC_BWD_REQS, DC_BWD_SHAPES
from tests.test_emu_parity import DEFAULT_TUNING

SENTINEL = tf.SENTINEL
REQ = {0: "null", 1: "write", 3: "add"}
DCM_TILINGS = tf.EMU_DCM_TILINGS
CASES = {}


class Case:
    """call(env) -> device array or tuple (None: no output); kernels: names the launch record must hold; exact: per result, whether the
    route is deterministic (default: all); refs() -> per result None or (want64, ref32, M, base) for check_fp64_bound; after(results):
    further asserts on the host results (fills that must survive)."""

    def __init__(self, call, kernels=(), tuning=None, exact=None, refs=None, after=None):
        self.call, self.kernels, self.tuning, self.exact, self.refs, self.after = call, tuple(kernels), dict(tuning or {}), exact, refs, after
        self._refs = None

    def references(self):
        if self._refs is None:
            self._refs = self.refs()
        return self._refs


def case(name, *a, **kw):
    assert name not in CASES, name
    CASES[name] = Case(*a, **kw)


def dest(env, values):
    """A destination holding `values`: banded on a guarded env."""
    values = np.ascontiguousarray(values, np.float32)
    return env.filled(values) if hasattr(env, "filled") else env.dev(values.copy())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, what):
    assert a.shape == b.shape, what
    diff = np.flatnonzero(_bits(a).ravel() != _bits(b).ravel())
    assert diff.size == 0, "%s: %d of %d elements differ in their bits (first at flat index %d: %r against %r)" % (
        what, diff.size, a.size, diff[0], a.ravel()[diff[0]], b.ravel()[diff[0]])


def contract(env, name, c):
    try:
        env.set_tuning(**c.tuning)
        with env.launches() as L0:
            res = c.call(env)
        L0.expect(c.kernels, what=name + " (plain)")
        l0, r0 = G.launch_list(env, L0), G.to_host(env, res)
        g1, g2 = G.guarded_env(env), G.guarded_env(env)
        g2.ad.calls = 0x4000                                   # another stale pattern than the first guarded call's
        r1, l1 = G.run_guarded(g1, c.call, expect=c.kernels, what=name + " (guarded)")            # (b) inside
        r2, l2 = G.run_guarded(g2, c.call, expect=c.kernels, what=name + " (guarded, second call)")
    finally:
        env.set_tuning(**DEFAULT_TUNING)
    assert l1 == l0 and l2 == l0, "%s: the guarded call took another route: %s, plain %s" % (name, l1, l0)      # (a)
    assert g1.ad.last_stale != g2.ad.last_stale or g1.ad.last_stale is None
    assert len(r0) == len(r1) == len(r2)
    exact = c.exact if c.exact is not None else (True,) * len(r0)
    refs = c.references() if not all(exact) else (None,) * len(r0)
    for i, (a0, a1, a2, ex, ref) in enumerate(zip(r0, r1, r2, exact, refs)):
        what = "%s result %d" % (name, i)
        if a0 is None:
            assert a1 is None and a2 is None, what
            continue
        for run, a in (("plain", a0), ("guarded", a1), ("guarded, second call", a2)):
            assert not np.isnan(a).any(), "%s (%s): %d NaN" % (what, run, int(np.isnan(a).sum()))               # (d)
        if ex:
            _same_bits(a1, a0, what + ": guarded against plain")                                                # (c)
            _same_bits(a2, a1, what + ": second guarded call against the first")                                # (f)
        else:
            want64, ref32, M, base = ref
            for run, a in (("plain", a0), ("guarded", a1), ("guarded, second call", a2)):
                pc.check_fp64_bound(a, want64, ref32, M, what="%s (%s)" % (what, run), base=base)               # (c), up to summation order
    if c.after:
        for run, r in (("plain", r0), ("guarded", r1), ("guarded, second call", r2)):
            c.after(r, "%s (%s)" % (name, run))                                                                 # (e)


def _rng(seed):
    return np.random.default_rng(4200 + seed)


def _kept(fill):
    def after(results, what, idx):
        for i in idx:
            assert (_bits(results[i]) == _bits(np.float32(fill))).all(), "%s: result %d, req null, was touched" % (what, i)
    return after


NULL_FILL = np.float32(-777.25)


# ---- correlation forward -----------------------------------------------------------------------------------------------------------
def corr_case(name, shape, md, kernels, tuning=None, form="plain", c0=4, extra=7, ws=None, **geo):
    N, C, H, W = shape
    rng = _rng(1)
    f1, f2 = pc.feat(rng, shape), pc.feat(rng, shape)
    kw = dict(kernel_size=1, max_displacement=md, stride1=1, stride2=1, pad_size=md, is_multiply=True)
    kw.update(geo)

    def call(env):
        if ws is not None:   # the case is there for its workspace: the query must say so
            q = env.ops.ns.correlation_workspace_bytes(N, C, H, W, md, kw["kernel_size"], kw["stride1"], kw["stride2"], kw["pad_size"], 1)
            assert (q > 0) == ws, "%s: mfn_correlation_workspace_bytes = %d" % (name, q)
        d1, d2 = env.dev(f1), env.dev(f2)
        if form != "into":
            return env.ops.Correlation(d1, d2, activation="leaky" if form == "leaky" else None, **kw)
        tc, th, tw = env.ops.correlation_out_shape(H, W, kw["kernel_size"], md, kw["stride1"], kw["stride2"], kw["pad_size"])
        buf = dest(env, np.full((N, c0 + tc + extra, th, tw), SENTINEL, np.float32))
        env.ops.Correlation(d1, d2, activation="leaky", out=buf[:, c0:c0 + tc], **kw)
        return buf

    def after(results, what):
        D2 = results[0].shape[1] - c0 - extra
        assert (_bits(results[0][:, :c0]) == _bits(SENTINEL)).all() and (_bits(results[0][:, c0 + D2:]) == _bits(SENTINEL)).all(), \
            "%s: wrote outside the slice" % what
        assert (_bits(results[0][:, c0:c0 + D2]) != _bits(SENTINEL)).all(), "%s: slice elements left unwritten" % what

    case(name, call, kernels, tuning, after=after if form == "into" else None)


for _i, (_t, _s, _md, _k) in enumerate(tf.EMU_CORR_FORCED):
    corr_case("corr_forced_%d_%s" % (_i, "+".join(_k)), _s, _md, _k, tuning=_t, ws=True if "corr_reduce" in _k else None)
    if _i in (0, 4, 8):   # the band, the coarse-level band, slices + reduce: also into a concat slice
        corr_case("corr_forced_%d_%s_into" % (_i, "+".join(_k)), _s, _md, _k, tuning=_t, form="into")
for _a in tf.ARITHS:   # the plan's own forms (test_emu_correlation_plan)
    corr_case("corr_plan_96_arith%d" % _a, (1, 96, 5, 16), 4, ["corr_gramk"] if _a else ["corr_direct"], tuning=dict(corr_gram=_a), form="leaky")
    corr_case("corr_plan_12_arith%d" % _a, (1, 12, 6, 40), 2, ["corr_dma_v26"], tuning=dict(corr_gram=_a))
for _C in (16, 32):   # tests/test_emu_parity.py test_correlation_channel_slices_and_reduce
    corr_case("corr_sliced_reduce_C%d" % _C, (2, _C, 7, 16), 4, ["corr_tiled_v6", "corr_reduce"], tuning=dict(corr_variant=6, corr_direct=2), ws=True)
corr_case("corr_level5_tuned_sliced", (8, 128, 12, 16), 4, ["corr_tiled_v6", "corr_reduce"], tuning=dict(corr_variant=6), ws=True)
corr_case("corr_direct", (2, 30, 6, 8), 4, ["corr_direct"], tuning=dict(corr_direct=1))
corr_case("corr_generic_k3_s2", (2, 3, 9, 10), 2, ["corr_generic"], kernel_size=3, stride1=2, pad_size=3)
corr_case("corr_into_unaligned_slice", (2, 5, 5, 6), 4, ["corr_generic"], form="into", c0=3)      # 3 * 30 floats: no multiple of 16 bytes
corr_case("corr_odd_width", (1, 3, 5, 7), 4, ["corr_generic"])
corr_case("corr_w30", (2, 8, 20, 30), 2, ["corr_generic"])


# ---- correlation backward (raw ABI: a req-null gradient is a real buffer) ------------------------------------------------------------
def corr_bwd_case(name, shape, md, req, kernels, tuning=None, exact=True, **geo):
    N, C, H, W = shape
    rng = _rng(2)
    f1, f2 = pc.feat(rng, shape), pc.feat(rng, shape)
    kw = dict(kernel_size=1, stride1=1, stride2=1, pad_size=md)
    kw.update(geo)
    tc, th, tw = oracle.correlation_out_shape(H, W, md, kw["kernel_size"], kw["stride1"], kw["stride2"], kw["pad_size"])
    go = rng.standard_normal((N, tc, th, tw)).astype(np.float32)
    base = [rng.standard_normal(shape).astype(np.float32) if r == 3 else np.full(shape, NULL_FILL if r == 0 else np.nan, np.float32) for r in req]

    def call(env):
        ad = env.ops.ad
        g, a, b = (ad.prepare(env.dev(v)) for v in (go, f1, f2))
        g1, g2 = dest(env, base[0]), dest(env, base[1])
        env.ops.check(env.ops.ns.correlation_bwd(ad.ptr(g), ad.ptr(a), ad.ptr(b), ad.ptr(g1), ad.ptr(g2), N, C, H, W, md, kw["kernel_size"],
                                                 kw["stride1"], kw["stride2"], kw["pad_size"], 1, req[0], req[1], ad.stream(a)))
        return g1, g2

    def refs():   # M: the sum of |terms| = the same gradient of the absolute values (the operator is bilinear in gout and the other feature map)
        okw = dict(max_displacement=md, **kw)
        r32, r64 = oracle.correlation_backward(go, f1, f2, **okw), oracle.correlation_backward(go, f1, f2, dtype=np.float64, **okw)
        M = oracle.correlation_backward(np.abs(go), np.abs(f1), np.abs(f2), dtype=np.float64, **okw)
        return [None if r == 0 else (r64[i], r32[i], M[i], base[i] if r == 3 else None) for i, r in enumerate(req)]

    null = [i for i, r in enumerate(req) if r == 0]
    case(name, call, kernels, tuning, exact=tuple(exact or r == 0 for r in req), refs=refs, after=lambda r, what: _kept(NULL_FILL)(r, what, null))


for _r in CORR_BWD_REQS:
    _n = "".join(REQ[r][0] for r in _r)
    corr_bwd_case("corr_bwd_lds_%s" % _n, (2, 5, 6, 16), 4, _r, ["corr_bwd_lds"])
    corr_bwd_case("corr_bwd_block_%s" % _n, (2, 5, 6, 16), 4, _r, ["corr_bwd_block"], tuning=dict(bwd_off=4))
    corr_bwd_case("corr_bwd_gather_%s" % _n, (2, 3, 5, 7), 4, _r, ["corr_bwd_gather"])                # W % 4 != 0
    # any other geometry: the scatter kernel, which adds through atomics -- the header promises its bits nothing, so it answers to the bound
    corr_bwd_case("corr_bwd_generic_%s" % _n, (2, 3, 9, 10), 2, _r, ["corr_bwd_scatter"], exact=False, kernel_size=3, stride1=2, pad_size=3)


# ---- deformable convolution forward --------------------------------------------------------------------------------------------------
def deform_case(name, N, C, H, W, kernels, tuning=None, Cout=None, packed=False, groups=1, dg=1, entry="dropin", mask=True, tradeoff=True):
    Cout = Cout or C
    rng = _rng(3)
    x = pc.feat(rng, (N, C, H, W))
    w = pc.msra_weight(rng, Cout, C // groups)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    off = np.concatenate([deform_offsets(rng, N, H, W, "smooth") for _ in range(dg)], axis=1)
    fl = exact_positions(pc.flow_field(rng, N, H, W) * np.float32(8.0 / 20.0), 2.0 ** -10)
    m = (rng.standard_normal((N, 1, H, W)) * 2).astype(np.float32) if mask else None
    tr = rng.standard_normal((N, Cout, H, W)).astype(np.float32) if tradeoff else None
    geo = dict(kernel=(3, 3), pad=(1, 1), num_group=groups)

    def call(env):
        xd, wd, bd = env.dev(x), env.dev(w), env.dev(b)
        pk = None
        if packed:   # the packed buffer: exactly mfn_deform_conv_packed_weight_bytes, banded, stale inside
            pk = env.ops.pack_deform_weights(wd, (N, C, H, W), num_deformable_group=dg, **geo)
            assert pk.nbytes == env.ops.ns.deform_conv_packed_weight_bytes(N, C, H, W, Cout, 3, 3, 1, 1, 1, 1, 1, 1, groups, dg)
        if entry == "dropin":
            return env.ops.DeformableConvolution(xd, env.dev(off), wd, bd, num_filter=Cout, num_deformable_group=dg, packed=pk, **geo)
        if entry == "shared":
            return env.ops.deformable_convolution_shared(xd, env.dev(fl), 20.0, 8.0, wd, bd, num_group=groups, packed=pk)
        return env.ops.deformable_matching(xd, env.dev(fl), 20.0, 8.0, wd, bd, env.dev(m) if mask else None, env.dev(tr) if tradeoff else None,
                                           leaky=True, num_group=groups, packed=pk)

    case(name, call, kernels, tuning)


for _mt, _pt, _nw, _C in DCM_TILINGS:
    deform_case("deform_mma_mt%d_pt%d_nw%d_C%d" % (_mt, _pt, _nw, _C), 1, _C, 6, 8, ["dc_mma"], tuning=dict(dc_mma=-1, dc_mt=_mt, dc_pt=_pt, dc_nw=_nw))
deform_case("deform_lds_fp32", 1, 32, 8, 16, ["dc_lds"], tuning=dict(dc_mma=0))
deform_case("deform_lds_fp32_w7", 1, 32, 6, 7, ["dc_lds"], tuning=dict(dc_mma=0))
deform_case("deform_split_k", 1, 32, 4, 8, ["dc_lds", "dc_reduce"], tuning=dict(dc_mma=0, dc_pt=1, dc_ksb=2))
deform_case("deform_split_k_matching", 1, 32, 4, 8, ["dc_lds", "dc_reduce"], tuning=dict(dc_mma=0, dc_pt=1, dc_ksb=2), entry="matching")
deform_case("deform_generic_groups2", 2, 4, 6, 7, ["dc_generic"], Cout=6, groups=2)
deform_case("deform_generic_dg2", 2, 4, 6, 7, ["dc_generic"], Cout=6, dg=2)
deform_case("deform_packed_mma", 1, 32, 6, 8, ["dc_mma"], tuning=dict(dc_mma=-1), packed=True)
deform_case("deform_packed_lds", 1, 32, 6, 8, ["dc_lds"], tuning=dict(dc_mma=0), packed=True)
for _a in tf.ARITHS:
    deform_case("deform_shared_arith%d" % _a, 1, 32, 6, 8, [tf.EMU_DC_KERNEL[_a]], tuning=dict(dc_mma=_a), entry="shared")
    for _m, _t in ((True, True), (False, False), (True, False)):
        deform_case("deform_matching_arith%d_mask%d_tradeoff%d" % (_a, _m, _t), 1, 32, 6, 8, [tf.EMU_DC_KERNEL[_a]], tuning=dict(dc_mma=_a),
                    entry="matching", mask=_m, tradeoff=_t)
deform_case("deform_matching_w7", 1, 8, 5, 7, ["dc_lds"], entry="matching")
deform_case("deform_shared_packed", 1, 32, 6, 8, ["dc_mma"], tuning=dict(dc_mma=-1), entry="shared", packed=True)


# ---- deformable convolution backward (raw ABI) ---------------------------------------------------------------------------------------
def deform_bwd_case(name, N, Cin, Cout, H, W, req, kernels, tuning=None, bias=True, flow=False, no_ws=False, okind="smooth"):
    """mfn_deform_conv_bwd (flow: mfn_deform_conv_shared_bwd), 3x3 / pad 1.  gx and goffset: up to summation order, always; gw and gbias:
    deterministic where the weight launch adds its slabs in a fixed order (DcBwdW::PcSlabs) or no atomics are involved (Generic)."""
    req = list(req)
    if not bias:
        req[3] = 0
    rng, x, w, go = tb._dc_inputs(N, Cin, Cout, H, W, "plain", 11)
    scale, stride = 20.0, 8.0
    if flow:
        fl = exact_positions(pc.flow_field(rng, N, H, W) * np.float32(stride / scale), 2.0 ** -10)
        off = oracle.offsets_from_flow(fl, scale, stride)
    else:
        fl, off = None, deform_offsets(rng, N, H, W, okind)
    second = fl if flow else off
    shapes = (x.shape, second.shape, w.shape, (Cout,))
    base = [rng.standard_normal(s).astype(np.float32) if r == 3 else np.full(s, NULL_FILL if r == 0 else np.nan, np.float32) for r, s in zip(req, shapes)]
    slabs = "dc_bwd_weight_reduce" in kernels
    w_exact = slabs or "dc_bwd_weight" in kernels
    b_exact = slabs or "dc_bwd_bias" in kernels

    def call(env):
        ops, ad = env.ops, env.ops.ad
        g, xd, sd, wd = (ad.prepare(env.dev(v)) for v in (go, x, second, w))
        grads = [dest(env, v) for v in base]
        if flow:
            need = ops.ns.deform_conv_shared_bwd_workspace_bytes(N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1)
        else:
            need = ops.ns.deform_conv_bwd_workspace_bytes(N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
        # the slabs of the weight gradient's shape (W % 4 == 0, at most 96 filters), whatever the requests; flow: the offsets and their gradient too
        offs = 2 * ((N * 18 * H * W * 4 + 255) // 256 * 256) if flow else 0
        assert need >= offs and (need > offs) == (W % 4 == 0 and Cout <= 96), "%s: the query answers %d bytes" % (name, need)
        ws = ops._workspace(xd, need) if need and not no_ws else None
        wsp, wsb = (ad.ptr(ws), ad.nbytes(ws)) if ws is not None else (None, 0)
        gp = [ad.ptr(v) for v in grads]
        if flow:
            ops.check(ops.ns.deform_conv_shared_bwd(ad.ptr(g), ad.ptr(xd), ad.ptr(sd), scale, stride, ad.ptr(wd), *gp, N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1,
                                                    1, *req, wsp, wsb, ad.stream(xd)))
        else:
            ops.check(ops.ns.deform_conv_bwd(ad.ptr(g), ad.ptr(xd), ad.ptr(sd), ad.ptr(wd), *gp, N, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, *req,
                                             wsp, wsb, ad.stream(xd)))
        return tuple(grads)

    def refs():
        r32, r64 = tb._dc_oracle(go, x, off, w, np.float32), tb._dc_oracle(go, x, off, w, np.float64)
        if flow:
            f = np.float32(scale) / np.float32(stride)
            r32 = (r32[0], (r32[1].reshape(N, 9, 2, H, W).sum(axis=1) * f).astype(np.float32), r32[2], r32[3])
            r64 = (r64[0], r64[1].reshape(N, 9, 2, H, W).sum(axis=1) * (scale / stride), r64[2], r64[3])
            M = ref_numpy.deformable_convolution_shared_backward_bound(go, x, fl, scale, stride, w)
        else:
            M = ref_numpy.deformable_convolution_backward_bound(go, x, off, w)
        return [None if r == 0 else (r64[i], r32[i], M[i], base[i] if r == 3 else None) for i, r in enumerate(req)]

    null = [i for i, r in enumerate(req) if r == 0]
    exact = tuple(r == 0 or ex for r, ex in zip(req, (False, False, w_exact, b_exact)))
    case(name, call, kernels, tuning, exact=exact, refs=refs, after=lambda r, what: _kept(NULL_FILL)(r, what, null))


def _dc_kernels(req, inp, wk):
    """Kernels of a deformable backward by its requests: the input route's, the weight route's (the bias rides on the weight launch, or has
    its own where there is none or the generic one)."""
    k = []
    if req[0] or req[1]:
        k += [inp]
    if req[2]:
        k += list(wk)
    if req[3] and (not req[2] or wk == ("dc_bwd_weight",)):
        k += ["dc_bwd_bias"]
    return k


PCS, PCA, MFMA, WGEN = ("dc_bwd_weight_pc", "dc_bwd_weight_reduce"), ("dc_bwd_weight_pc",), ("dc_bwd_weight_mfma",), ("dc_bwd_weight",)
# weight route -> (N, Cin, Cout, H, W), input kernel there, tuning, workspace withheld
DC_BWD_ROUTES = {
    "PcSlabs": ((1, 4, 4, 5, 16), "dc_bwd_input_pix", {}, False, PCS),
    "Pc": ((1, 4, 4, 5, 16), "dc_bwd_input_pix", {}, True, PCA),                        # no workspace: the same kernel through atomics
    "Mfma": ((1, 2, 4, 4, 6), "dc_bwd_input_tile", {}, False, MFMA),                    # W % 4 != 0
    "Generic": ((1, 4, 4, 5, 16), "dc_bwd_input", dict(path_generic=2), False, WGEN),
}
for _route, (_shape, _inp, _tune, _nows, _wk) in DC_BWD_ROUTES.items():
    for _r in DC_BWD_REQS:
        _n = "".join(REQ[r][0] for r in _r)
        if _route == "Pc" and not _r[2]:
            continue    # without a weight request no weight route: the PcSlabs case of the same requests
        deform_bwd_case("deform_bwd_%s_%s" % (_route, _n), *_shape, _r, _dc_kernels(_r, _inp, _wk), tuning=_tune, no_ws=_nows)
    deform_bwd_case("deform_bwd_%s_no_bias" % _route, *_shape, (1, 1, 1, 1), _dc_kernels((1, 1, 1, 0), _inp, _wk), tuning=_tune, no_ws=_nows, bias=False)
deform_bwd_case("deform_bwd_tile_switch", 1, 4, 4, 4, 16, (1, 1, 1, 1), ["dc_bwd_input_tile"] + list(PCS), tuning=dict(bwd_off=1))
deform_bwd_case("deform_bwd_pertap", 1, 4, 8, 7, 16, (1, 1, 1, 1), ["dc_bwd_input_pix"] + list(PCS), okind="pertap")
# the branch shapes of the dispatch record at N <= 2 below the pyramid's sizes: every one whose query asks for slabs (3x3 / pad 1, W % 4 == 0, at
# most 96 filters), and one that asks for none (100 filters)
_small = lambda s: s[5] == dict(k=3, pad=1) and 0 < s[0] <= 2 and s[3] * s[4] <= 400 and s[1] * s[2] <= 1600
_BRANCH = [s for s in DC_BWD_SHAPES if _small(s) and s[4] % 4 == 0 and s[2] <= 96] + [s for s in DC_BWD_SHAPES if _small(s) and s[2] > 96][:1]
for _s in _BRANCH:
    _N, _Ci, _Co, _H, _W, _ = _s
    _slabs = _W % 4 == 0 and _Co <= 96
    _pix = _W % 4 == 0 and _Ci % 4 == 0
    deform_bwd_case("deform_bwd_branch_%dx%dx%dx%dx%d" % _s[:5], _N, _Ci, _Co, _H, _W, (1, 1, 1, 1),
                    ["dc_bwd_input_pix" if _pix else "dc_bwd_input_tile"] + list(PCS if _slabs else MFMA))
assert len(_BRANCH) >= 10 and _BRANCH[-1][2] > 96
# more than 256 tile x channel-block items: the weight kernel's blocks take two 8x4 tiles each (tpb = 2 in dc_bwd_plan) and the last block a
# single one (29 x 9 = 261 tiles, 131 blocks); the slabs are per block, so this is the slab indexing no small shape reaches.  Weights and
# bias only: the input gradient's kernel does not touch the workspace
deform_bwd_case("deform_bwd_two_tiles_per_block", 1, 4, 4, 116, 72, (0, 0, 1, 1), list(PCS))
deform_bwd_case("deform_shared_bwd_flow", 1, 4, 4, 5, 8, (1, 1, 1, 1), ["dc_bwd_input_pix"] + list(PCS), flow=True)
deform_bwd_case("deform_shared_bwd_flow_add", 1, 4, 20, 5, 8, (3, 3, 3, 3), ["dc_bwd_input_pix"] + list(PCS), flow=True)
deform_bwd_case("deform_shared_bwd_composed", 1, 4, 4, 5, 8, (1, 3, 1, 1), ["offsets_from_flow_v4", "dc_bwd_input_pix", "offsets_from_flow_bwd"] + list(PCS),
                tuning=dict(bwd_off=2), flow=True)
deform_bwd_case("deform_shared_bwd_composed_null_flow", 1, 4, 4, 5, 8, (1, 0, 1, 1), ["offsets_from_flow_v4", "dc_bwd_input_pix"] + list(PCS),
                tuning=dict(bwd_off=2), flow=True)


# ---- convolution / deconvolution forward -----------------------------------------------------------------------------------------------
def _conv_inputs(N, Cin, Cout, H, W, geo, transposed, seed=0):
    rng = _rng(5 + seed)
    k = tuple(geo.get("kernel", (4, 4) if transposed else (3, 3)))
    x = pc.feat(rng, (N, Cin, H, W))
    w = (rng.standard_normal(((Cin, Cout) if transposed else (Cout, Cin)) + k) * np.sqrt(2.0 / (1.01 * Cin * k[0] * k[1]))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    return x, w, b


def conv_case(name, N, Cin, Cout, H, W, geo, transposed, kernels, tuning, packed=False, leaky=False):
    x, w, b = _conv_inputs(N, Cin, Cout, H, W, geo, transposed)
    geo = dict(dict(stride=(2, 2), pad=(1, 1)) if transposed else {}, **geo)

    def call(env):
        op = env.ops.Deconvolution if transposed else env.ops.Convolution
        wd, pk = env.dev(w), None
        if packed:
            pgeo = {k: v for k, v in geo.items() if k != "adj"}
            pk = env.ops.pack_conv_weights(wd, (N, Cin, H, W), transposed=transposed, **dict(dict(kernel=(4, 4) if transposed else (3, 3)), **pgeo))
        return op(env.dev(x), wd, env.dev(b), num_filter=Cout, activation="leaky" if leaky else None, packed=pk, **geo)

    case(name, call, kernels, tuning)


for _c in tf.EMU_CONV:
    _N, _Ci, _Co, _H, _W, _geo, _tr, _tune, _k32, _kdef = _c
    for _a, _k in ((0, _k32), (-1, _kdef)):
        if _a == -1 and _k32 == _kdef:
            continue   # one kernel under both arithmetics
        conv_case("conv_%s_arith%d" % (tf._conv_id(_c), _a), _N, _Ci, _Co, _H, _W, _geo, _tr, _k, dict(_tune or {}, conv_mma=_a), leaky=_tr)
# both packed layouts: the fp32 MFMA kernels' and the bf16 x 3 kernels', and the transposed layer's
conv_case("conv_packed_mfma", 1, 8, 32, 8, 16, tf.P1, False, ["conv3x3_mfma"], dict(conv_mma=0), packed=True)
conv_case("conv_packed_bf16x3", 1, 8, 32, 8, 16, tf.P1, False, ["conv3x3_bf16x3"], dict(conv_mma=-1), packed=True)
conv_case("conv_packed_dcm", 2, 37, 32, 6, 16, tf.P1, False, ["conv3x3_dcm"], dict(conv_mma=-1, conv_dcm=2), packed=True)
conv_case("deconv_packed", 2, 9, 16, 5, 8, {}, True, ["deconv_as_conv3x3_mfma"], dict(conv_mma=0), packed=True)


def conv_concat_case(name, arith, kernels):
    """x = concat(conv(x), x) in place (MaskFlownet.py:219): out = buf[:, :Cout], x = buf[:, Cout:Cout + Cin]; three more channels behind
    them hold a fill that must survive, as must x."""
    N, Cin, Cout, H, W, tail = 2, 8, 32, 8, 16, 3
    x, w, b = _conv_inputs(N, Cin, Cout, H, W, tf.P1, False, seed=1)
    start = np.full((N, Cout + Cin + tail, H, W), SENTINEL, np.float32)
    start[:, Cout:Cout + Cin] = x

    def call(env):
        buf = dest(env, start)
        env.ops.Convolution(buf[:, Cout:Cout + Cin], env.dev(w), env.dev(b), num_filter=Cout, activation="leaky", out=buf[:, :Cout], **tf.P1)
        return buf

    def after(results, what):
        assert (_bits(results[0][:, Cout:]) == _bits(start[:, Cout:])).all(), "%s: the input slice or the channels behind it changed" % what

    case(name, call, kernels, dict(conv_mma=arith), after=after)


conv_concat_case("conv_concat_in_place_arith0", 0, ["conv3x3_mfma"])
conv_concat_case("conv_concat_in_place_arith-1", -1, ["conv3x3_bf16x3"])


# ---- convolution backward: every entry of EMU_CONV_ROUTES ---------------------------------------------------------------------------------
def conv_bwd_case(name, arith, route):
    shape, kw, data, wgrad, bias_k = route
    kw = dict(kw)
    N, Cin, Cout, H, W = shape
    req, has_bias, leaky, tuning = kw.pop("req", tb.WWW), kw.pop("bias", True), kw.pop("leaky", False), kw.pop("tuning", None)
    kw.pop("zeros", None)
    geo = tb._conv_geo(**kw)
    rng, x, w, b, go = tb._conv_problem(N, Cin, Cout, H, W, "plain", 3, geo, has_bias)
    shapes = (x.shape, w.shape, (Cout,))
    rq = [tb_req for tb_req in ({"null": 0, "write": 1, "add": 3}[r] for r in req)]
    if b is None:
        rq[2] = 0
    # the raw ABI: a gradient whose req is null (or the bias gradient of a layer without bias) is a real buffer that must keep its fill
    base = [rng.standard_normal(s).astype(np.float32) if r == 3 else np.full(s, NULL_FILL if r == 0 else np.nan, np.float32) for r, s in zip(rq, shapes)]
    okw = dict(kernel=geo["kernel"], stride=geo["stride"], pad=geo["pad"], dilate=geo["dilate"], no_bias=b is None)
    if geo["transposed"]:
        okw["adj"] = geo["adj"]
    (kh, kw_), (sh, sw), (ph, pw), (dh, dw), (ah, aw) = geo["kernel"], geo["stride"], geo["pad"], geo["dilate"], geo["adj"]
    dims = (N, Cin, H, W, Cout, kh, kw_, sh, sw, ph, pw, dh, dw, 1, int(geo["transposed"]), ah, aw, 1 if leaky else 0)

    class _Names:     # conv_route only asks whether this is the emulation
        emu = True
    kernels, _ = tb.conv_route(_Names, arith, data, wgrad, bias_k, req, has_bias)
    w_atomics = "dc_bwd_weight_mfma" in kernels     # the weight gradient through atomics (W % 4 != 0 here): up to summation order

    def call(env):
        ops, ad = env.ops, env.ops.ad
        fwd = ops.Deconvolution if geo["transposed"] else ops.Convolution
        xd, wd, god = (ad.prepare(env.dev(v)) for v in (x, w, go))
        y = fwd(xd, wd, env.dev(b) if b is not None else None, activation="leaky", **okw) if leaky else None
        grads = [dest(env, v) for v in base]
        need = ops.ns.conv2d_bwd_workspace_bytes(*dims)
        ws = ops._workspace(xd, need) if need else None
        ops.check(ops.ns.conv2d_bwd(ad.ptr(god), ad.ptr(xd), ad.ptr(wd), ad.ptr(y) if y is not None else None, *(ad.ptr(g) for g in grads), *dims, *rq,
                                    ad.ptr(ws) if ws is not None else None, ad.nbytes(ws) if ws is not None else 0, ad.stream(xd)))
        return tuple(grads)

    def refs():
        import torch
        y64 = None
        if leaky:
            t64 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)
            y64 = tb._torch_conv(t64(x), t64(w), t64(b), geo).numpy()
        ref32, want64, M = tb._conv_refs(x, w, b, go, geo, y64)
        return [None if r == 0 else (w64, r32, m, bs if r == 3 else None) for r, w64, r32, m, bs in zip(rq, want64, ref32, M, base)]

    null = [i for i, r in enumerate(rq) if r == 0]
    case(name, call, kernels, dict(tuning or {}, conv_mma=arith), exact=(True, not w_atomics or rq[1] == 0, True), refs=refs,
         after=lambda r, what: _kept(NULL_FILL)(r, what, null))


for _name, _route in tb.EMU_CONV_ROUTES.items():
    for _a in tb.ARITHS:
        conv_bwd_case("conv_bwd_%s_arith%d" % (_name, _a), _a, _route)


# ---- everything without a workspace ------------------------------------------------------------------------------------------------------
def simple_case(name, make, kernels=(), tuning=None):
    """make(rng) -> call, or (call, exact, refs) where a result is scattered through atomics."""
    made = make(_rng(7))
    call, exact, refs = made if isinstance(made, tuple) else (made, None, None)
    case(name, call, kernels, tuning, exact=exact, refs=refs)


def _warp(clip, backward):
    def make(rng):
        shape = (2, 3, 8, 11)
        x, fl, go = rng.standard_normal(shape).astype(np.float32), pc.flow_field(rng, 2, 8, 11, sigma=3.0), rng.standard_normal(shape).astype(np.float32)
        if not backward:
            return lambda env: env.ops.warp(env.dev(x), env.dev(fl), clip_grid=clip)

        def refs():   # gx is scattered through atomics, as MXNet's kernel does: the bound of tests/test_backward_fp64.py case_warp_bwd
            pos = ref_numpy.warp_positions(fl, clip, np.float32)
            return [(ref_numpy.warp_backward_at(go, x, pos)[0], oracle.warp_backward(go, x, fl, clip_grid=clip)[0],
                     ref_numpy.warp_backward_at(go, x, pos, bound=True)[0], None), None]
        return (lambda env: env.ops.warp_backward(env.dev(go), env.dev(x), env.dev(fl), clip_grid=clip)), (False, True), refs
    return make


for _clip in (False, True):
    simple_case("warp_fwd_clip%d" % _clip, _warp(_clip, False), ["warp_fwd_fast"])
    simple_case("warp_bwd_clip%d" % _clip, _warp(_clip, True), ["warp_bwd"])


def _grid_warp(rng):
    fl = (rng.standard_normal((2, 2, 6, 9)) * 2).astype(np.float32)
    return lambda env: env.ops.GridGenerator(env.dev(fl), "warp")


def _grid_affine(rng):
    theta = rng.standard_normal((2, 6)).astype(np.float32)
    return lambda env: env.ops.GridGenerator(env.dev(theta), "affine", target_shape=(5, 7))


def _sampler(backward):
    def make(rng):
        x = rng.standard_normal((1, 2, 6, 9)).astype(np.float32)
        grid = (rng.uniform(-1.2, 1.2, (1, 2, 5, 7))).astype(np.float32)       # oH, oW != iH, iW; some samples outside
        go = rng.standard_normal((1, 2, 5, 7)).astype(np.float32)
        if not backward:
            return lambda env: env.ops.BilinearSampler(env.dev(x), env.dev(grid))

        def refs():   # gdata is scattered through atomics; its terms are gout times bilinear weights >= 0: M is the gradient of |gout|
            return [(oracle.bilinear_sampler_backward(go, x, grid, dtype=np.float64)[0], oracle.bilinear_sampler_backward(go, x, grid)[0],
                     oracle.bilinear_sampler_backward(np.abs(go), x, grid, dtype=np.float64)[0], None), None]
        return (lambda env: env.ops.BilinearSampler_backward(env.dev(go), env.dev(x), env.dev(grid))), (False, True), refs
    return make


def _grid_bwd(rng):
    go = rng.standard_normal((2, 2, 6, 9)).astype(np.float32)
    return lambda env: env.ops.GridGenerator_backward(env.dev(go))


def _null_req_bwd(sampler, req):
    """mfn_warp_bwd / mfn_bilinear_sampler_bwd through the raw ABI with one req null: that gradient is a real buffer and keeps its fill."""
    def make(rng):
        N, C, H, W = 2, 3, 8, 11
        x, go = rng.standard_normal((N, C, H, W)).astype(np.float32), rng.standard_normal((N, C, H, W)).astype(np.float32)
        second = rng.uniform(-1.2, 1.2, (N, 2, H, W)).astype(np.float32) if sampler else pc.flow_field(rng, N, H, W, sigma=3.0)
        base = [np.full(s, NULL_FILL if r == 0 else np.nan, np.float32) for r, s in zip(req, (x.shape, second.shape))]

        def call(env):
            ops, ad = env.ops, env.ops.ad
            g, xd, sd = (ad.prepare(env.dev(v)) for v in (go, x, second))
            grads = [dest(env, v) for v in base]
            if sampler:
                ops.check(ops.ns.bilinear_sampler_bwd(ad.ptr(g), ad.ptr(xd), ad.ptr(sd), ad.ptr(grads[0]), ad.ptr(grads[1]), N, C, H, W, H, W, *req, ad.stream(xd)))
            else:
                ops.check(ops.ns.warp_bwd(ad.ptr(g), ad.ptr(xd), ad.ptr(sd), ad.ptr(grads[0]), ad.ptr(grads[1]), N, C, H, W, 0, *req, ad.stream(xd)))
            return tuple(grads)

        def refs():
            if sampler:
                r = (oracle.bilinear_sampler_backward(go, x, second, dtype=np.float64)[0], oracle.bilinear_sampler_backward(go, x, second)[0],
                     oracle.bilinear_sampler_backward(np.abs(go), x, second, dtype=np.float64)[0], None)
            else:
                pos = ref_numpy.warp_positions(second, False, np.float32)
                r = (ref_numpy.warp_backward_at(go, x, pos)[0], oracle.warp_backward(go, x, second, clip_grid=False)[0],
                     ref_numpy.warp_backward_at(go, x, pos, bound=True)[0], None)
            return [r if req[0] else None, None]
        return call, (req[0] == 0, True), refs
    return make


for _req in ((1, 0), (0, 1)):
    for _smp in (False, True):
        _nm = "%s_bwd_req_%s" % ("bilinear_sampler" if _smp else "warp", "".join(REQ[r][0] for r in _req))
        simple_case(_nm, _null_req_bwd(_smp, _req), ["bilinear_sampler_bwd" if _smp else "warp_bwd"])
        CASES[_nm].after = (lambda null: lambda r, what: _kept(NULL_FILL)(r, what, null))([i for i, r in enumerate(_req) if r == 0])
simple_case("grid_generator_warp", _grid_warp, ["grid_generator_warp"])
simple_case("grid_generator_affine", _grid_affine, ["grid_generator_affine"])
simple_case("bilinear_sampler_fwd", _sampler(False), ["bilinear_sampler"])
simple_case("bilinear_sampler_bwd", _sampler(True), ["bilinear_sampler_bwd"])
simple_case("grid_generator_bwd", _grid_bwd, ["grid_generator_warp_bwd"])


def _upsample(factor, backward):
    def make(rng):
        H, W = 5, 7
        if backward:
            go = rng.standard_normal((1, 2, H * factor, W * factor)).astype(np.float32)
            return lambda env: env.ops.Upsample_backward(env.dev(go), factor)
        x = rng.standard_normal((1, 2, H, W)).astype(np.float32)
        return lambda env: env.ops.Upsample(env.dev(x), factor)
    return make


for _f in (1, 2, 8, 16):
    simple_case("upsample_fwd_x%d" % _f, _upsample(_f, False), ["upsample_v1" if _f < 8 else "upsample_v4"])
    simple_case("upsample_bwd_x%d" % _f, _upsample(_f, True), ["upsample_bwd" if _f < 8 else "upsample_bwd_block"])


def _leaky(n):
    def make(rng):
        go, y = rng.standard_normal((n,)).astype(np.float32), rng.standard_normal((n,)).astype(np.float32)
        return lambda env: env.ops.LeakyReLU_backward(env.dev(go), env.dev(y))
    return make


for _n in (1, 3, 4, 1023, 1025):
    simple_case("leaky_relu_bwd_n%d" % _n, _leaky(_n), ["leaky_bwd"])


def _offsets(W, backward):
    def make(rng):
        if backward:
            go = rng.standard_normal((2, 18, 5, W)).astype(np.float32)
            return lambda env: env.ops.offsets_from_flow_backward(env.dev(go), 20.0, 16.0)
        fl = rng.standard_normal((2, 2, 5, W)).astype(np.float32)
        return lambda env: env.ops.offsets_from_flow(env.dev(fl), 20.0, 16.0)
    return make


simple_case("offsets_from_flow_w6", _offsets(6, False), ["offsets_from_flow"])
simple_case("offsets_from_flow_w8", _offsets(8, False), ["offsets_from_flow_v4"])
simple_case("offsets_from_flow_bwd_w6", _offsets(6, True), ["offsets_from_flow_bwd"])
simple_case("offsets_from_flow_bwd_w8", _offsets(8, True), ["offsets_from_flow_bwd"])


# ---- predict entries ---------------------------------------------------------------------------------------------------------------------
def _resize(Hin, Win, Hout, Wout, sub, flow):
    def make(rng):
        C = 2 if flow else 3
        x, m = rng.standard_normal((2, C, Hin, Win)).astype(np.float32), rng.standard_normal((2, C)).astype(np.float32)
        return lambda env: env.ops.bilinear_resize(env.dev(x), Hout, Wout, sub=env.dev(m) if sub else None, flow_rescale=flow)
    return make


for _nm, _hw in (("up", (5, 7, 9, 13)), ("down", (9, 13, 5, 6)), ("equal", (5, 7, 5, 7))):
    simple_case("resize_%s" % _nm, _resize(*_hw, False, False), ["resize_copy_v1" if _nm == "equal" else "resize_v1"])
    simple_case("resize_%s_sub" % _nm, _resize(*_hw, True, False), ["resize_copy_v1" if _nm == "equal" else "resize_v1"])
    simple_case("resize_%s_flow_rescale" % _nm, _resize(*_hw, False, True), ["resize_copy_v1" if _nm == "equal" else "resize_v1"])


def _pair(rng):
    a, b = rng.uniform(0, 255, (2, 3, 9, 13)).astype(np.float32), rng.uniform(0, 255, (2, 3, 9, 13)).astype(np.float32)
    return a, b


def _preprocess(rng):
    a, b = _pair(rng)
    m = rng.uniform(100, 150, (2, 3)).astype(np.float32)
    return lambda env: env.ops.preprocess_pair(env.dev(a), env.dev(b), 6, 10, mean=env.dev(m))


def _pair_mean(rng):
    a, b = _pair(rng)

    def call(env):
        assert env.ops.ns.pair_mean_workspace_bytes(2, 3, 9, 13) > 0
        return env.ops.pair_mean(env.dev(a), env.dev(b))
    return call


def _metrics(rng):
    f, l = (rng.standard_normal((2, 2, 9, 13)) * 4).astype(np.float32), (rng.standard_normal((2, 2, 9, 13)) * 4).astype(np.float32)
    m = (rng.uniform(0, 1, (2, 1, 9, 13)) > 0.3).astype(np.float32)

    def call(env):
        assert env.ops.ns.flow_metrics_workspace_bytes(2, 9, 13) > 0
        return env.ops.flow_metric_sums(env.dev(f), env.dev(l), env.dev(m))
    return call


simple_case("preprocess_pair", _preprocess, ["resize_v1"])
simple_case("pair_mean", _pair_mean, ["pair_mean_partial", "pair_mean_final"])
simple_case("flow_metrics", _metrics, ["flow_metrics_partial", "flow_metrics_final"])


# ---- the two halves ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    """The emulation, with the predict entries bound as well: the library exports them, the suite's namespace leaves them out because the
    oracle has no twin of them -- this file needs no oracle for them."""
    import copy
    import types
    from maskflownet_amd import _abi
    env = copy.copy(Env(emu=True))
    ns = types.SimpleNamespace(**vars(env.ops.ns))      # a namespace of this file's own: the suite's shared one stays as it is
    for name in ("pair_mean_workspace_bytes", "pair_mean", "preprocess_pair", "bilinear_resize_fwd", "flow_metrics_workspace_bytes", "flow_metrics"):
        fn = getattr(ctypes.CDLL(ns._cdll._name), "mfn_emu_" + name)
        fn.restype, fn.argtypes = _abi.PRODUCT_ONLY[name]
        setattr(ns, name, fn)
    env.ops = OpSet(ns, env.ops.ad, env.ops.check)
    return env


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


@pytest.mark.parametrize("name", list(CASES))
def test_emu_memory_contract(emu, name):
    contract(emu, name, CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_memory_contract(gpu, name):
    contract(gpu, name, CASES[name])


# ---- the harness fails for each defect it is there for (no kernel involved) -----------------------------------------------------------------
class _NoLaunches:
    log = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def expect(self, names, absent=(), what=""):
        pass


class FakeEnv:
    """The emulation's adapter without its library: what a fake operator written in numpy needs.  dev() puts an input between two finite
    neighbours, so that the PLAIN run of an operator that reads past its input still gives finite numbers."""
    emu = True

    def __init__(self):
        from tests.emu.emu_ops import NumpyAdapter

        class Roomy(NumpyAdapter):     # the plain run's outputs with room around them: the defective stores land in memory the test owns
            def empty(self, like, shape):
                n = int(np.prod(shape))
                return np.full(n + 32, np.nan, np.float32)[16:16 + n].reshape(shape)

        self.ops = OpSet(None, Roomy(), None)
        self.host = lambda a: a
        self.set_tuning = lambda **kw: None
        self.launches = _NoLaunches

    def dev(self, a):
        big = np.ones(a.size + 32, np.float32)
        big[16:16 + a.size] = a.ravel()
        return big[16:16 + a.size].reshape(a.shape)


def _raw(ad, a, first, count):
    """`count` floats from `first` floats behind a's first element, wherever that is."""
    return np.ctypeslib.as_array(ctypes.cast(ad.ptr(a) + 4 * first, ctypes.POINTER(ctypes.c_float)), (count,))


NEED = 256   # bytes of workspace the fake operator asks for


def fake_operator(defect):
    """y = 2 x through a workspace, plus a gradient buffer whose req is null."""
    x = np.arange(1, 41, dtype=np.float32).reshape(1, 2, 4, 5)
    n = x.size

    def call(env):
        ad = env.ops.ad
        xx = ad.prepare(env.dev(x))
        out = ad.empty(xx, xx.shape)
        null = dest(env, np.full((7,), NULL_FILL, np.float32))
        ws = env.ops._workspace(xx, NEED)
        if defect == "stale workspace":
            out.reshape(-1)[0] = ws[5]                          # read before anything was written there
        ws[:n] = xx.reshape(-1)
        out.reshape(-1)[...] = 2 * ws[:n] + (out.reshape(-1) if defect == "stale workspace" else 0) * 0
        if defect == "store past the end":
            _raw(ad, out, n, 1)[0] = 1.0
        if defect == "store before the start":
            _raw(ad, out, -1, 1)[0] = 1.0
        if defect == "store at byte need of the workspace":
            _raw(ad, ws, NEED // 4, 1)[0] = 1.0
        if defect == "input band read":
            out.reshape(-1)[n - 1] *= _raw(ad, xx, n, 1)[0]       # the float behind the input, multiplied into a result
        if defect == "req-null buffer touched":
            null[3] = 0.0
        return out, null

    return Case(call, after=lambda r, what: _kept(NULL_FILL)(r, what, [1]))


DEFECTS = ["store past the end", "store before the start", "store at byte need of the workspace", "input band read", "stale workspace",
           "req-null buffer touched"]


def test_harness_passes_the_sound_operator():
    contract(FakeEnv(), "fake operator", fake_operator(None))


@pytest.mark.parametrize("defect", DEFECTS)
def test_harness_fails_for(defect):
    with pytest.raises(AssertionError) as e:
        contract(FakeEnv(), "fake operator", fake_operator(defect))
    want = {"store past the end": "band after", "store before the start": "band before", "store at byte need of the workspace": "bytes[256]",
            "input band read": "NaN", "stale workspace": "NaN", "req-null buffer touched": "req null"}[defect]
    assert want in str(e.value), str(e.value)
