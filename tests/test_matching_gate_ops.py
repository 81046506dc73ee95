"""The matching module's gate on its own (maskflownet_amd/csrc/kernels/gate.h: mfn_matching_gate_fwd / _bwd, ops.matching_gate /
matching_gate_backward), one table on the emulation (CPU) and on the MI355X (-m gpu).

Reference: tests/gate_ref.py (fp64, its fp32 twin, the magnitude bounds M).  Bars: parity_cases.assert_magnitude_bound on every M,
parity_cases.check_fp64_bound on the forward and on each of the three gradients (4 x the twin's error + 16 * 2^-24 of M per element,
exact zeros where M == 0, finite), bit-identical replays, the launch record names the route taken and not the other one, and each
(shape, route) once through test_memory_contract.contract (guard bands, the workspace of exactly the queried size holding stale NaN).
Masks are uniform in +-12: saturated sigmoids in every case.  The backward's y is the twin's forward with a few elements set to
exactly 0 (that side takes the slope, as mfn_leaky_relu_bwd does); kernel and reference read the kink from the same y."""
import ctypes

import numpy as np
import pytest

from tests import gate_ref as gr
from tests import parity_cases as pc
from tests import test_memory_contract as mc
from tests.fp64_env import Env

U = 2.0 ** -24
# (N, C, H, W): (what it exercises, channel slices of the backward plan -- gate_plan of kernels/gate.h worked out by hand:
# blocks = N * ceil(H W / 1024), slices = min(ceil(512 / blocks), ceil(C / 4)), channels per slice = ceil(C / slices), renormalised)
SHAPES = {
    (1, 1, 1, 1): ("a single element", 1),
    (2, 5, 3, 7): ("the scalar route, odd C, the image stride", 2),
    (1, 37, 4, 8): ("the vector route, C divisible by no split", 10),
    (2, 32, 5, 12): ("pixels no multiple of a wave", 8),
    (1, 3, 2, 132): ("a row longer than a wave's span", 1),
    (1, 8, 33, 68): ("more pixels than one block", 2),
    (2, 196, 6, 8): ("level 6 of the full model at its real size: the channel-split plan", 49),
}
ALL_REQS = ("write", "write", "write")


def ws_bytes(shape):
    N, C, H, W = shape
    return SHAPES[shape][1] * N * H * W * 4 if SHAPES[shape][1] > 1 else 0


def make_inputs(shape, mask=True, tradeoff=True, leaky=True, gout2=False, seed=0):
    N, C, H, W = shape
    rng = np.random.default_rng([N, C, H, W, seed])
    a = {"raw": pc.graded_feat(rng, shape, "graded-pixel"), "leaky": leaky,
         "mask": rng.uniform(-12.0, 12.0, (N, 1, H, W)).astype(np.float32) if mask else None,
         "tradeoff": (-0.5 * pc.graded_feat(rng, shape, "graded-pixel")).astype(np.float32) if tradeoff else None,
         "gout": pc.graded_gout(rng, shape), "gout2": pc.graded_gout(rng, shape) if gout2 else None}
    y = gr.forward(a["raw"], a["mask"], a["tradeoff"], leaky, dtype=np.float32)
    y.reshape(-1)[::5] = 0.0                       # exactly 0: the slope side
    a["y"] = y
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


_REFS = {}


def references(key, a):
    """Once per input set, shared by the emulation and the GPU side, never modified."""
    if key not in _REFS:
        f = (a["raw"], a["mask"], a["tradeoff"], a["leaky"])
        b = (a["gout"], a["y"], a["raw"], a["mask"], a["leaky"], a["gout2"])
        r = {"f64": gr.forward(*f), "f32": gr.forward(*f, dtype=np.float32), "fM": gr.forward(*f, magnitude=True),
             "b64": gr.backward(*b), "b32": gr.backward(*b, dtype=np.float32), "bM": gr.backward(*b, magnitude=True)}
        for v in r.values():
            for arr in (v if isinstance(v, tuple) else (v,)):
                if arr is not None:
                    arr.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def dev(env, a):
    return None if a is None else env.dev(a)


def run_fwd(env, a):
    return np.array(env.host(env.ops.matching_gate(env.dev(a["raw"]), dev(env, a["mask"]), dev(env, a["tradeoff"]), leaky=a["leaky"])))


def run_bwd(env, a, req=ALL_REQS, out=None):
    g = env.ops.matching_gate_backward(env.dev(a["gout"]), env.dev(a["y"]), env.dev(a["raw"]), dev(env, a["mask"]), leaky=a["leaky"],
                                       out_grad2=dev(env, a["gout2"]), req=req, out=out)
    return [None if v is None else np.array(env.host(v)) for v in g]


def routes(shape):
    v = "v4" if shape[3] % 4 == 0 else "v1"
    o = "v1" if v == "v4" else "v4"
    return v, o


def check_case(env, shape, mask, tradeoff, leaky, gout2, req):
    a = make_inputs(shape, mask, tradeoff, leaky, gout2)
    key = (shape, mask, tradeoff, leaky, gout2)
    what = "%s mask=%d tradeoff=%d leaky=%d gout2=%d req=%s" % (shape, mask, tradeoff, leaky, gout2, req)
    ref = references(key, a)
    v, o = routes(shape)
    # ---- forward
    with env.launches() as L:
        out = run_fwd(env, a)
    L.expect(["matching_gate_fwd_" + v], absent=["matching_gate_fwd_" + o], what=what)
    np.testing.assert_array_equal(out.view(np.uint32), run_fwd(env, a).view(np.uint32))
    pc.assert_magnitude_bound(ref["fM"], ref["f64"], what)
    e_lib, e_ref = pc.check_fp64_bound(out, ref["f64"], ref["f32"], ref["fM"], what + " forward")
    print("%s forward: e_lib %.2f ulp, e_twin %.2f ulp of M" % (what, e_lib / U, e_ref / U))
    # ---- backward
    names = ("raw", "mask", "tradeoff")
    reqs = {"write": ALL_REQS, "add": ("add",) * 3, "null": ("null",) * 3}.get(req) or tuple("write" if n == req else "null" for n in names)
    live = [r != "null" and (n != "mask" or mask) for n, r in zip(names, reqs)]
    bases = [None] * 3          # req add: bases of the order of M element by element, so that the addition's rounding stays of M's order
    if req == "add":
        rng = np.random.default_rng(11)
        bases = [None if M is None else (rng.standard_normal(M.shape) * M).astype(np.float32) for M in ref["bM"]]

    def once():
        d = [None if b is None else mc.dest(env, b) for b in bases] if req == "add" else None
        return run_bwd(env, a, reqs, d)
    with env.launches() as L:
        got = once()
    if any(live):
        L.expect(["matching_gate_bwd_" + v], absent=["matching_gate_bwd_" + o], what=what)
        assert (L.count("matching_gate_bwd_join") == 1) == (live[1] and SHAPES[shape][1] > 1), what
    else:
        assert sum(L.count("matching_gate_bwd_" + k) for k in ("v4", "v1", "join")) == 0, what + ": a launch with every req null"
    for g, g2 in zip(got, once()):
        assert (g is None) == (g2 is None)
        if g is not None:
            np.testing.assert_array_equal(g.view(np.uint32), g2.view(np.uint32))
    for n, lv, g, w64, r32, M, base in zip(names, live, got, ref["b64"], ref["b32"], ref["bM"], bases):
        if not lv:
            assert g is None, "%s: gradient of %s with req null" % (what, n)
            continue
        pc.assert_magnitude_bound(M, w64, what + " g" + n)
        e_lib, e_ref = pc.check_fp64_bound(g, w64, r32, M, what + " g" + n, base=base)
        print("%s g%s: e_lib %.2f ulp, e_twin %.2f ulp of M" % (what, n, e_lib / U, e_ref / U))


COMBO_SHAPES = [(2, 5, 3, 7), (2, 196, 6, 8)]
REQ_SHAPES = [(1, 37, 4, 8), (2, 5, 3, 7)]
PARAMS = [(s, True, True, True, False, "write") for s in SHAPES]
PARAMS += [(s, m, t, l, True, "write") for s in COMBO_SHAPES for m in (True, False) for t in (True, False) for l in (True, False)]
PARAMS += [(s, True, True, True, i % 2 == 0, r) for s in REQ_SHAPES for i, r in enumerate(("add", "raw", "mask", "tradeoff", "null"))]
IDS = ["%dx%dx%dx%d-m%d-t%d-l%d-g%d-%s" % (s + (m, t, l, g, r)) for s, m, t, l, g, r in PARAMS]


@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


@pytest.mark.parametrize("shape,mask,tradeoff,leaky,gout2,req", PARAMS, ids=IDS)
def test_emu_gate_against_fp64(emu, shape, mask, tradeoff, leaky, gout2, req):
    check_case(emu, shape, mask, tradeoff, leaky, gout2, req)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mask,tradeoff,leaky,gout2,req", PARAMS, ids=IDS)
def test_gpu_gate_against_fp64(gpu, shape, mask, tradeoff, leaky, gout2, req):
    check_case(gpu, shape, mask, tradeoff, leaky, gout2, req)


# ---- the reference itself: the two-sigmoid product against autograd, and why it is not s * (1 - s) ------------------------------
def test_reference_equals_autograd_and_the_two_sigmoid_form_holds_on_saturated_masks():
    import torch
    a = make_inputs((2, 5, 3, 7), gout2=True)
    t = {k: torch.from_numpy(np.asarray(a[k], np.float64)).requires_grad_(k in ("raw", "mask", "tradeoff")) for k in ("raw", "mask", "tradeoff", "gout", "gout2")}
    out = torch.nn.functional.leaky_relu(t["raw"] * torch.sigmoid(t["mask"]) + t["tradeoff"], 0.1)
    np.testing.assert_allclose(gr.forward(a["raw"], a["mask"], a["tradeoff"]), out.detach().numpy(), rtol=1e-12)
    out.backward(t["gout"] + t["gout2"])
    graw, gmask, gtr = gr.backward(a["gout"], out.detach().numpy(), a["raw"], a["mask"], True, a["gout2"])
    for g, k in ((graw, "raw"), (gmask, "mask"), (gtr, "tradeoff")):
        np.testing.assert_allclose(g, t[k].grad.numpy(), rtol=1e-9, atol=1e-300)
    m = np.random.default_rng(0).uniform(-12, 12, 4096).astype(np.float32)
    s, sn = gr._sig(m, np.float32)
    s64, sn64 = gr._sig(m.astype(np.float64), np.float64)
    two = np.abs((s * sn).astype(np.float64) - s64 * sn64) / (s64 * sn64)
    one_minus = np.abs((s * (np.float32(1) - s)).astype(np.float64) - s64 * sn64) / (s64 * sn64)
    assert two.max() <= 5 * U * 2 and one_minus.max() > 1e3 * U      # ulp = 2^-23 of the term's magnitude


# ---- the raw ABI with every pointer 4 bytes past a 16-byte boundary: the scalar route on a W % 4 == 0 shape ---------------------
def check_misaligned(env):
    shape = (1, 5, 3, 8)
    N, C, H, W = shape
    a = make_inputs(shape, gout2=True)
    ad, ns = env.ops.ad, env.ops.ns
    keep = []

    def off(values=None, n=None):
        n = values.size if values is not None else n
        host = np.full(n + 1, np.nan, np.float32)
        if values is not None:
            host[1:] = values.reshape(-1)
        buf = ad.prepare(env.dev(host))
        keep.append(buf)
        view = buf[1:]
        assert ad.ptr(view) % 16 == 4
        return view
    raw, mask, tr, gout, gout2, y = (off(a[k]) for k in ("raw", "mask", "tradeoff", "gout", "gout2", "y"))
    out, graw, gmask, gtr = off(n=a["raw"].size), off(n=a["raw"].size), off(n=a["mask"].size), off(n=a["raw"].size)
    nb = ns.matching_gate_bwd_workspace_bytes(N, C, H, W)
    assert nb == 2 * N * H * W * 4                   # blocks = 1, slices = min(512, ceil(5 / 4)) = 2
    ws = off(n=nb // 4)
    with env.launches() as L:
        env.ops.check(ns.matching_gate_fwd(ad.ptr(raw), ad.ptr(mask), ad.ptr(tr), 1, ad.ptr(out), N, C, H, W, ad.stream(raw)))
        env.ops.check(ns.matching_gate_bwd(ad.ptr(gout), ad.ptr(gout2), ad.ptr(y), ad.ptr(raw), ad.ptr(mask), 1, ad.ptr(graw), ad.ptr(gmask),
                                           ad.ptr(gtr), N, C, H, W, 1, 1, 1, ad.ptr(ws), nb, ad.stream(raw)))
    L.expect(["matching_gate_fwd_v1", "matching_gate_bwd_v1", "matching_gate_bwd_join"], absent=["matching_gate_fwd_v4", "matching_gate_bwd_v4"],
             what="misaligned")
    ref = references(("misaligned",), a)
    pc.check_fp64_bound(np.array(env.host(out)).reshape(shape), ref["f64"], ref["f32"], ref["fM"], "misaligned forward")
    for g, w64, r32, M in zip((graw, gmask, gtr), ref["b64"], ref["b32"], ref["bM"]):
        pc.check_fp64_bound(np.array(env.host(g)).reshape(M.shape), w64, r32, M, "misaligned backward")


def test_emu_misaligned_pointers_take_the_scalar_route(emu):
    check_misaligned(emu)


@pytest.mark.gpu
def test_gpu_misaligned_pointers_take_the_scalar_route(gpu):
    check_misaligned(gpu)


# ---- memory contract: each (shape, route) plain and twice between guard bands, the workspace of exactly the queried size --------
def _contract_case(shape):
    a = make_inputs(shape, gout2=True, seed=1)
    N, C, H, W = shape
    v, _ = routes(shape)

    def call(env):
        assert env.ops.ns.matching_gate_bwd_workspace_bytes(N, C, H, W) == ws_bytes(shape)
        out = env.ops.matching_gate(env.dev(a["raw"]), env.dev(a["mask"]), env.dev(a["tradeoff"]))
        return (out,) + env.ops.matching_gate_backward(env.dev(a["gout"]), env.dev(a["y"]), env.dev(a["raw"]), env.dev(a["mask"]),
                                                       out_grad2=env.dev(a["gout2"]))
    return mc.Case(call, ["matching_gate_fwd_" + v, "matching_gate_bwd_" + v] + (["matching_gate_bwd_join"] if SHAPES[shape][1] > 1 else []))


def _null_req_case(req):
    """The raw ABI with one req null: that gradient is a real (banded) buffer and keeps its fill."""
    shape = (2, 5, 3, 8)
    N, C, H, W = shape
    a = make_inputs(shape, seed=2)
    shapes = (shape, (N, 1, H, W), shape)

    def call(env):
        ops, ad = env.ops, env.ops.ad
        gout, y, raw, mask = (ad.prepare(env.dev(a[k])) for k in ("gout", "y", "raw", "mask"))
        grads = [mc.dest(env, np.full(s, mc.NULL_FILL if r == 0 else np.nan, np.float32)) for r, s in zip(req, shapes)]
        nb = ops.ns.matching_gate_bwd_workspace_bytes(N, C, H, W) if req[1] else 0
        ws = ops._workspace(gout, nb) if nb else None
        ops.check(ops.ns.matching_gate_bwd(ad.ptr(gout), None, ad.ptr(y), ad.ptr(raw), ad.ptr(mask), 1, *[ad.ptr(g) for g in grads], N, C, H, W,
                                           *req, ad.ptr(ws) if nb else None, ad.nbytes(ws) if nb else 0, ad.stream(gout)))
        return tuple(grads)
    null = [i for i, r in enumerate(req) if r == 0]
    return mc.Case(call, ["matching_gate_bwd_v4"], after=lambda r, what: mc._kept(mc.NULL_FILL)(r, what, null))


CONTRACT = {"%dx%dx%dx%d %s" % (s + (routes(s)[0],)): _contract_case(s) for s in SHAPES}
CONTRACT.update({"req null %s" % "".join(mc.REQ[r][0] for r in req): _null_req_case(req) for req in ((0, 1, 1), (1, 0, 1), (1, 1, 0))})


@pytest.mark.parametrize("name", list(CONTRACT))
def test_emu_memory_contract(emu, name):
    mc.contract(emu, name, CONTRACT[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONTRACT))
def test_gpu_memory_contract(gpu, name):
    mc.contract(gpu, name, CONTRACT[name])


# ---- argument checks: every error returns its code before any launch ---------------------------------------------------------------
def test_new_entries_fail_before_any_launch():
    from maskflownet_amd import _lib
    _lib.build()
    lib = _lib.lib()
    one = ctypes.c_void_p(16)                     # never dereferenced
    big = 1 << 20

    def fwd(raw=one, mask=one, tr=one, act=1, out=one, N=1, C=8, H=4, W=4):
        return lib.matching_gate_fwd(raw, mask, tr, act, out, N, C, H, W, None)

    def bwd(gout=one, gout2=None, y=one, raw=one, mask=one, act=1, graw=one, gmask=one, gtr=one, N=1, C=8, H=4, W=4, req=(1, 1, 1), ws=one, wsb=big):
        return lib.matching_gate_bwd(gout, gout2, y, raw, mask, act, graw, gmask, gtr, N, C, H, W, *req, ws, wsb, None)
    for call in (fwd, bwd):
        assert call(N=-1) == -2 and call(C=0) == -2 and call(H=0) == -2 and call(W=-3) == -2
        assert call(act=2) == -3 and b"activation" in lib.last_error()
        assert call(act=-1) == -3
        assert call(raw=None) == -1 and b"NULL" in lib.last_error()
        assert call(N=70000) == -4
    assert fwd(out=None) == -1
    assert fwd(raw=None, mask=None, tr=None, out=None, N=0) == 0
    assert bwd(gout=None) == -1 and bwd(y=None) == -1
    assert bwd(graw=None) == -1 and bwd(gmask=None) == -1 and bwd(gtr=None) == -1
    for bad in ((2, 1, 1), (1, -1, 1), (1, 1, 4)):
        assert bwd(req=bad) == -3 and b"req" in lib.last_error()
    assert bwd(mask=None) == -3 and b"no mask" in lib.last_error()                     # a mask gradient without a mask
    need = lib.matching_gate_bwd_workspace_bytes(1, 8, 4, 4)
    assert need == 2 * 16 * 4                                                           # two slices of four channels, 16 pixels
    assert bwd(ws=None, wsb=0) == -5 and b"workspace" in lib.last_error()
    assert bwd(wsb=need - 4) == -5
    assert bwd(ws=ctypes.c_void_p(18)) == -6
    assert bwd(req=(0, 0, 0), gout=None, y=None, raw=None, graw=None, gmask=None, gtr=None, ws=None, wsb=0) == 0   # nothing to do
    assert bwd(gout=None, y=None, raw=None, mask=None, graw=None, gmask=None, gtr=None, N=0, req=(1, 0, 1), ws=None, wsb=0) == 0
    assert lib.matching_gate_bwd_workspace_bytes(8, 32, 96, 128) == 6 * 8 * 96 * 128 * 4  # level 2 at batch 8: 96 blocks of pixels, 6 slices of 6 channels
    assert lib.matching_gate_bwd_workspace_bytes(8, 32, 384, 512) == 0                  # 1536 blocks of pixels: no split, no workspace
    assert lib.matching_gate_bwd_workspace_bytes(8, 196, 6, 8) == 49 * 8 * 48 * 4       # level 6 of the full model
    assert lib.matching_gate_bwd_workspace_bytes(0, 8, 4, 4) == 0 and lib.matching_gate_bwd_workspace_bytes(1, 0, 4, 4) == 0


def test_ops_shape_errors_and_cpu_tensors():
    import torch
    from maskflownet_amd import ops
    from tests.emu import emu_ops
    o = emu_ops.emu_ops()
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ValueError, match="mask must be"):
        o.matching_gate(z(1, 4, 2, 2), z(1, 2, 2, 2))
    with pytest.raises(ValueError, match="tradeoff must be"):
        o.matching_gate(z(1, 4, 2, 2), None, z(1, 3, 2, 2))
    with pytest.raises(ValueError, match="out has shape"):
        o.matching_gate(z(1, 4, 2, 2), out=z(1, 4, 2, 3))
    with pytest.raises(ValueError, match="raw must be 4-D"):
        o.matching_gate(z(4, 2, 2))
    with pytest.raises(ValueError, match="output has shape"):
        o.matching_gate_backward(z(1, 4, 2, 2), z(1, 4, 2, 3), z(1, 4, 2, 2))
    with pytest.raises(ValueError, match="mask must be"):
        o.matching_gate_backward(z(1, 4, 2, 2), z(1, 4, 2, 2), z(1, 4, 2, 2), z(1, 1, 2, 3))
    with pytest.raises(ValueError, match="needs the buffer"):
        o.matching_gate_backward(z(1, 4, 2, 2), z(1, 4, 2, 2), z(1, 4, 2, 2), z(1, 1, 2, 2), req=("add", "write", "write"))
    with pytest.raises(ValueError, match="needs raw"):
        o.matching_gate_backward(z(1, 4, 2, 2), z(1, 4, 2, 2), None, z(1, 1, 2, 2))
    graw, gmask, gtr = o.matching_gate_backward(z(1, 4, 2, 2), z(1, 4, 2, 2), None, None)     # no mask: raw is not needed, no gmask
    assert gmask is None and graw.shape == gtr.shape == (1, 4, 2, 2)
    t = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.matching_gate(t(1, 4, 2, 2), t(1, 1, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.matching_gate_backward(t(1, 4, 2, 2), t(1, 4, 2, 2), t(1, 4, 2, 2), t(1, 1, 2, 2))
