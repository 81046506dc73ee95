"""The fused multiscale training loss (maskflownet_amd/csrc/kernels/loss.h: mfn_multiscale_epe_fwd / _bwd, ops.multiscale_epe,
training.FusedMultiscaleEpe), sqrt and robust form.

Reference: tests/loss_ref.py -- the fp32 oracle's Upsample output taken as given, everything after it in fp64 (acceptance) or fp32 (the
twin).  Bars: gradients parity_cases.check_fp64_bound (4 x the twin's error + 16 * 2^-24 of M per element, exact zeros where M == 0,
finite, non-vacuous); sums and loss |got - fp64| <= 64 * 2^-24 * M, the bar of test_gpu_flow_metrics for the same kind of sum.  M: the
same expressions over absolute values.  The kernel tables run on the emulation here and under -m gpu on the MI355X."""
import ctypes

import numpy as np
import pytest

from tests import loss_ref as lr
from tests import parity_cases as pc
from tests import test_memory_contract as mc
from tests.fp64_env import Env

U = 2.0 ** -24
DEFAULT_SCALES, DEFAULT_WEIGHTS = (64, 32, 16, 8, 4), (.005, .01, .02, .08, .32)
FORMS = {"sqrt": (None, 1e-8), "q0.4": (0.4, 1e-8), "q0.4 eps0.01": (0.4, 0.01)}
MASKS = ("ones", "sparse", "scalar")

# name: (N, label (H, W), scales, weights)
CASES = {}
for _f in (1, 2, 3, 4, 8):
    CASES["f%d" % _f] = (2, (3 * _f, 5 * _f), (_f,), (.32,))          # f = 1, 2, 3: W % 4 != 0, the scalar route
for _f in (16, 32, 64):
    CASES["f%d" % _f] = (2, (2 * _f, 3 * _f), (_f,), (.32,))
CASES["training call"] = (2, (128, 192), DEFAULT_SCALES, DEFAULT_WEIGHTS)
CASES["degenerate 1x1"] = (1, (4, 4), (4,), (.32,))                    # every footprint is all edge clamp
CASES["degenerate 1x4"] = (1, (4, 16), (4,), (.32,))
CASES["mixed width"] = (2, (9, 15), (3, 1), (.32, .08))                # two different factors in one call, W % 4 != 0
CASES["W=1"] = (1, (3, 1), (1,), (.32,))


def bwd_kernel(f):
    return "multiscale_epe_bwd_t%d" % (1 if f <= 4 else (64 if f <= 16 else 256))      # loss_bwd_threads (kernels/loss.h)


def make_inputs(case, mask_kind, kind="plain", seed=0):
    N, (H, W), scales, weights = CASES[case]
    rng = np.random.default_rng([len(case), N, H, W, seed])
    if kind == "plain":
        preds = [(4 * rng.standard_normal((N, 2, H // f, W // f))).astype(np.float32) for f in scales]
        label = (4 * rng.standard_normal((N, 2, H, W))).astype(np.float32)
    else:
        preds = [4 * pc.graded_feat(rng, (N, 2, H // f, W // f), kind) for f in scales]
        label = 4 * pc.graded_feat(rng, (N, 2, H, W), kind)
    mask = {"ones": np.ones((N, 1, H, W), np.float32), "sparse": (rng.uniform(size=(N, 1, H, W)) < 0.3).astype(np.float32),
            "scalar": np.array([1.0, 0.5], np.float32)[:N].reshape(N, 1, 1, 1) if N > 1 else np.full((1, 1, 1, 1), 0.5, np.float32)}[mask_kind]
    if mask_kind == "sparse":
        mask[:, 0, 0, 0] = 1.0            # no sample without a valid pixel (that is the NaN rule's test)
    gloss = rng.uniform(0.5, 1.5, N).astype(np.float32)
    return preds, label, mask, gloss, scales, weights


_REFS = {}


def references(key, preds, label, mask, gloss, scales, weights, eps, q):
    """Computed once per input set, shared by the emulation and the GPU side, never modified."""
    if key not in _REFS:
        a = (preds, label, mask, scales, weights, eps, q)
        _REFS[key] = {"loss64": lr.loss(*a), "lossM": lr.loss(*a, magnitude=True),
                      "g64": lr.grads(gloss, *a), "g32": lr.grads(gloss, *a, dtype=np.float32), "gM": lr.grads(gloss, *a, magnitude=True)}
        for v in _REFS[key].values():
            for arr in v:
                arr.setflags(write=False)
    return _REFS[key]


def check_sums(got_loss, got_sums, ref, what):
    (l64, s64), (lM, sM) = ref["loss64"], ref["lossM"]
    for name, g, w, m in (("loss", got_loss, l64, lM), ("sums", got_sums, s64, sM)):
        assert np.isfinite(g).all(), "%s %s" % (what, name)
        ratio = float((np.abs(g.astype(np.float64) - w) / (64 * U * m)).max())
        print("%s %s: max |got - fp64| / (64 * 2^-24 * M) = %.3f" % (what, name, ratio))
        assert ratio <= 1.0, "%s %s: %.3f of the 64-ulp bar" % (what, name, ratio)


def run(env, preds, label, mask, gloss, scales, weights, eps, q, reqs=None, out=None):
    dp, dl, dm, dg = [env.dev(p) for p in preds], env.dev(label), env.dev(mask), env.dev(gloss)
    loss, sums = env.ops.multiscale_epe(dp, dl, dm, scales, weights, eps, q)
    gp = env.ops.multiscale_epe_backward(dg, dp, dl, dm, scales, weights, sums, eps, q, reqs=reqs, out=out)
    return np.array(env.host(loss)), np.array(env.host(sums)), [None if g is None else np.array(env.host(g)) for g in gp]


def check_case(env, case, form, mask_kind, kind="plain"):
    q, eps = FORMS[form]
    preds, label, mask, gloss, scales, weights = make_inputs(case, mask_kind, kind)
    what = "%s %s %s %s" % (case, form, mask_kind, kind)
    with env.launches() as L:
        loss, sums, gp = run(env, preds, label, mask, gloss, scales, weights, eps, q)
    W = label.shape[3]
    L.expect(["multiscale_epe_partial_v4" if W % 4 == 0 else "multiscale_epe_partial_v1", "multiscale_epe_final"] + [bwd_kernel(f) for f in scales],
             absent=["multiscale_epe_partial_v1" if W % 4 == 0 else "multiscale_epe_partial_v4"], what=what)
    loss2, sums2, gp2 = run(env, preds, label, mask, gloss, scales, weights, eps, q)                       # determinism: bit-identical replays
    for a, b in zip([loss, sums] + gp, [loss2, sums2] + gp2):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    ref = references((case, form, mask_kind, kind), preds, label, mask, gloss, scales, weights, eps, q)
    check_sums(loss, sums, ref, what)
    np.testing.assert_array_equal(sums[:, -1], ref["loss64"][1][:, -1].astype(np.float32))              # msum: exact for these masks
    for f, g, w64, r32, M in zip(scales, gp, ref["g64"], ref["g32"], ref["gM"]):
        pc.assert_magnitude_bound(M, w64, what)
        e_lib, e_ref = pc.check_fp64_bound(g, w64, r32, M, "%s gradient of scale %d" % (what, f))
        print("%s scale %d: e_lib %.2f ulp, e_twin %.2f ulp of M" % (what, f, e_lib / U, e_ref / U))


PARAMS = [(c, fm, m, "plain") for c in CASES for fm in FORMS for m in MASKS] + [("f4", fm, "ones", "graded-pixel") for fm in FORMS]


@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


@pytest.mark.parametrize("case,form,mask_kind,kind", PARAMS)
def test_emu_loss_against_fp64(emu, case, form, mask_kind, kind):
    check_case(emu, case, form, mask_kind, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("case,form,mask_kind,kind", PARAMS)
def test_gpu_loss_against_fp64(gpu, case, form, mask_kind, kind):
    check_case(gpu, case, form, mask_kind, kind)


# ---- CPU: the reference itself ---------------------------------------------------------------------------------------------------
def _up64(p, f):
    import torch
    return lr.upsample_torch(torch.from_numpy(np.asarray(p, np.float64)), f).numpy()


@pytest.mark.parametrize("form", ["sqrt", "q0.4"])
@pytest.mark.parametrize("mask_kind", MASKS)
def test_reference_equals_the_literal_composition(form, mask_kind):
    """loss_ref.loss / grads against EpeLossWithMask / MultiscaleEpe written out in torch, fp64, and its autograd -- on the same fp64
    upsampled values (the fp32 oracle's differ from them by roundings of u, which the kernels' contract takes as given)."""
    import torch
    q, eps = FORMS[form]
    preds, label, mask, gloss, scales, weights = make_inputs("mixed width", mask_kind)
    tp = [torch.from_numpy(p.astype(np.float64)).requires_grad_(True) for p in preds]
    total = lr.composed(tp, torch.from_numpy(label.astype(np.float64)), torch.from_numpy(mask.astype(np.float64)), scales, weights, eps, q)
    (total * torch.from_numpy(gloss.astype(np.float64))).sum().backward()
    got, _ = lr.loss(preds, label, mask, scales, weights, eps, q, up=_up64)
    np.testing.assert_allclose(got, total.detach().numpy(), rtol=1e-13)
    for g, t in zip(lr.grads(gloss, preds, label, mask, scales, weights, eps, q, up=_up64), tp):
        np.testing.assert_allclose(g, t.grad.numpy(), rtol=1e-11, atol=1e-13 * np.abs(t.grad.numpy()).max())
    for p, f in zip(preds, scales):                                   # the fp32 oracle's Upsample against this statement: 4 products, 3 sums
        bound = 8 * U * _up64(np.abs(p), f) + 1e-30
        assert (np.abs(lr.oracle_upsample(p, f) - _up64(p, f)) <= bound).all()


def test_composed_module_with_q_equals_the_reference():
    """training.MultiscaleEpe(q=0.4) over the torch fp64 backend of tests/test_training_step.py."""
    import torch
    from maskflownet_amd import training
    from tests.test_training_step import TorchBackend
    preds, label, mask, gloss, scales, weights = make_inputs("mixed width", "sparse")
    mod = training.MultiscaleEpe(scales, weights, 1e-8, backend=TorchBackend(), q=0.4)
    tp = [torch.from_numpy(p.astype(np.float64)) for p in preds]
    got = mod(torch.from_numpy(label.astype(np.float64)), torch.from_numpy(mask.astype(np.float64)), *tp).numpy()
    want, _ = lr.loss(preds, label, mask, scales, weights, 1e-8, 0.4, up=_up64)
    np.testing.assert_allclose(got, want, rtol=1e-13)
    assert training.MultiscaleEpe().q is None and training.FusedMultiscaleEpe().scales == training.MultiscaleEpe().scales


# ---- sharp checks of the shared upsample arithmetic ---------------------------------------------------------------------------------
def check_sharp(env, f):
    case = "f%d" % f
    N, (H, W), scales, weights = CASES[case]
    preds, _, _, gloss, _, _ = make_inputs(case, "ones")
    u = lr.oracle_upsample(preds[0], f)
    mask = np.ones((N, 1, H, W), np.float32)
    _, _, gp = run(env, preds, u, mask, gloss, scales, weights, 1e-8, 0.4)
    assert (gp[0] == 0).all(), "robust-form gradient with label == Upsample(p): %d non-zero elements" % int((gp[0] != 0).sum())
    loss, sums, _ = run(env, preds, u, mask, gloss, scales, weights, 1e-8, None)
    want = weights[0] * np.sqrt(np.float32(1e-8)).astype(np.float64)
    assert (np.abs(loss - want) <= 64 * U * want).all(), (loss, want)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    up_or_down = np.where((yy + xx) % 2 == 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    label = np.nextafter(u, np.broadcast_to(up_or_down, u.shape)).astype(np.float32)
    _, _, gp = run(env, preds, label, mask, gloss, scales, weights, 1e-8, 0.4)
    a = (preds, label, mask, scales, weights, 1e-8, 0.4)
    w64, r32, M = lr.grads(gloss, *a)[0], lr.grads(gloss, *a, dtype=np.float32)[0], lr.grads(gloss, *a, magnitude=True)[0]
    pc.check_fp64_bound(gp[0], w64, r32, M, "label one ulp off on a checkerboard, f=%d" % f)
    big = np.abs(w64) > 2.0 ** -10 * M                  # (at f = 64 the 16 129 alternating terms of an element cancel to far below M)
    assert (big.any() or f > 4) and (np.sign(gp[0])[big] == np.sign(w64)[big]).all()


@pytest.mark.parametrize("f", [3, 4, 64])
def test_emu_upsampled_value_is_the_oracles(emu, f):
    check_sharp(emu, f)


@pytest.mark.gpu
@pytest.mark.parametrize("f", [3, 4, 64])
def test_gpu_upsampled_value_is_the_oracles(gpu, f):
    check_sharp(gpu, f)


# ---- edge behaviour -----------------------------------------------------------------------------------------------------------------
def check_structural_zeros_and_req(env, form):
    """f = 4, label 12 x 20, full-resolution rows 0..7 masked out: the footprints of input rows 0 and 1 (rows <= 3 and 1..7) hold no valid
    pixel.  req write, add (base scaled by M) and null."""
    q, eps = FORMS[form]
    preds, label, mask, gloss, scales, weights = make_inputs("f4", "sparse")
    mask[:, :, :8] = 0
    a = (preds, label, mask, scales, weights, eps, q)
    w64, r32, M = lr.grads(gloss, *a)[0], lr.grads(gloss, *a, dtype=np.float32)[0], lr.grads(gloss, *a, magnitude=True)[0]
    assert (M[:, :, :2] == 0).all() and (M[:, :, 2:] > 0).any()
    _, _, gp = run(env, *a[:3], gloss, *a[3:])
    pc.check_fp64_bound(gp[0], w64, r32, M, "structural zeros, write, " + form)
    base = (np.random.default_rng(5).standard_normal(M.shape) * np.maximum(M, 1e-3)).astype(np.float32)
    _, _, gp = run(env, *a[:3], gloss, *a[3:], reqs=["add"], out=[mc.dest(env, base)])
    pc.check_fp64_bound(gp[0], w64, r32, M, "structural zeros, add, " + form, base=base)
    np.testing.assert_array_equal(gp[0][:, :, :2], base[:, :, :2])
    # null through the raw ABI: a real buffer, untouched
    dp, dl, dm, dg = env.dev(preds[0]), env.dev(label), env.dev(mask), env.dev(gloss)
    _, sums = env.ops.multiscale_epe([dp], dl, dm, scales, weights, eps, q)
    buf = env.dev(np.full(preds[0].shape, mc.NULL_FILL, np.float32))
    ad, N, H, W = env.ops.ad, label.shape[0], label.shape[2], label.shape[3]
    with env.launches() as L:
        rc = env.ops.ns.multiscale_epe_bwd(ad.ptr(dg), (ctypes.c_void_p * 1)(ad.ptr(dp)), (ctypes.c_int * 1)(4), (ctypes.c_float * 1)(.32), 1, ad.ptr(dl),
                                           ad.ptr(dm), 0, eps, int(q is not None), float(q or 0), ad.ptr(sums), (ctypes.c_void_p * 1)(ad.ptr(buf)),
                                           (ctypes.c_int * 1)(0), N, H, W, ad.stream(dl))
    assert rc == 0 and L.count("multiscale_epe_bwd_t1") == 0
    assert (np.array(env.host(buf)).view(np.uint32) == np.float32(mc.NULL_FILL).view(np.uint32)).all()
    assert env.ops.multiscale_epe_backward(dg, [dp], dl, dm, scales, weights, sums, eps, q, reqs=["null"]) == (None,)


def check_nan_rule(env, form):
    q, eps = FORMS[form]
    preds, label, mask, gloss, scales, weights = make_inputs("mixed width", "sparse")
    mask[0] = 0
    loss, sums, gp = run(env, preds, label, mask, gloss, scales, weights, eps, q)
    assert np.isnan(loss[0]) and all(np.isnan(g[0]).all() for g in gp)
    one = ([p[1:] for p in preds], label[1:], mask[1:], scales, weights, eps, q)
    ref = {"loss64": lr.loss(*one), "lossM": lr.loss(*one, magnitude=True)}
    check_sums(loss[1:], sums[1:], ref, "NaN rule, the other sample, " + form)
    for g, w64, r32, M in zip(gp, lr.grads(gloss[1:], *one), lr.grads(gloss[1:], *one, dtype=np.float32), lr.grads(gloss[1:], *one, magnitude=True)):
        pc.check_fp64_bound(g[1:], w64, r32, M, "NaN rule, the other sample, " + form)


@pytest.mark.parametrize("form", ["sqrt", "q0.4"])
def test_emu_structural_zeros_and_req(emu, form):
    check_structural_zeros_and_req(emu, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sqrt", "q0.4"])
def test_gpu_structural_zeros_and_req(gpu, form):
    check_structural_zeros_and_req(gpu, form)


@pytest.mark.parametrize("form", ["sqrt", "q0.4"])
def test_emu_nan_rule(emu, form):
    check_nan_rule(emu, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sqrt", "q0.4"])
def test_gpu_nan_rule(gpu, form):
    check_nan_rule(gpu, form)


# ---- memory contract: each route plain and twice between guard bands, the workspace of exactly the queried size ---------------------
def _contract_case(case, form, mask_kind, ws_bytes):
    q, eps = FORMS[form]
    preds, label, mask, gloss, scales, weights = make_inputs(case, mask_kind, seed=1)
    N, _, H, W = label.shape

    def call(env):
        assert env.ops.ns.multiscale_epe_workspace_bytes(N, H, W, len(scales)) == ws_bytes
        dp, dl, dm, dg = [env.dev(p) for p in preds], env.dev(label), env.dev(mask), env.dev(gloss)
        loss, sums = env.ops.multiscale_epe(dp, dl, dm, scales, weights, eps, q)
        return (loss, sums) + env.ops.multiscale_epe_backward(dg, dp, dl, dm, scales, weights, sums, eps, q)
    kernels = ["multiscale_epe_partial_v4" if W % 4 == 0 else "multiscale_epe_partial_v1", "multiscale_epe_final"] + [bwd_kernel(f) for f in scales]
    return mc.Case(call, kernels)


CONTRACT = {                                                                             # workspace: N * ceil(H W / 2048) * (S + 1) * 4 bytes
    "v4, t1": _contract_case("f4", "sqrt", "sparse", 2 * 1 * 2 * 4),
    "v1, t1 (f = 3)": _contract_case("f3", "q0.4", "ones", 2 * 1 * 2 * 4),
    "v4, t64": _contract_case("f8", "q0.4", "scalar", 2 * 1 * 2 * 4),
    "v4, t256": _contract_case("f32", "sqrt", "sparse", 2 * 3 * 2 * 4),
    "training call": _contract_case("training call", "q0.4", "sparse", 2 * 12 * 6 * 4),
    "mixed width": _contract_case("mixed width", "sqrt", "scalar", 2 * 1 * 3 * 4),
}


@pytest.mark.parametrize("name", list(CONTRACT))
def test_emu_memory_contract(emu, name):
    mc.contract(emu, name, CONTRACT[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONTRACT))
def test_gpu_memory_contract(gpu, name):
    mc.contract(gpu, name, CONTRACT[name])


# ---- argument checks: every error returns its code before any launch ------------------------------------------------------------------
def test_new_entries_fail_before_any_launch():
    from maskflownet_amd import _lib
    _lib.build()
    lib = _lib.lib()
    one = ctypes.c_void_p(16)                     # never dereferenced
    P = lambda *v: (ctypes.c_void_p * len(v))(*v)
    I = lambda *v: (ctypes.c_int * len(v))(*v)
    Fl = lambda *v: (ctypes.c_float * len(v))(*v)
    big = 1 << 20

    def fwd(preds=P(16), factors=I(4), weights=Fl(.32), S=1, label=one, mask=one, robust=0, q=0.0, loss=one, sums=one, N=1, H=8, W=8, ws=one, wsb=big):
        return lib.multiscale_epe_fwd(preds, factors, weights, S, label, mask, 0, 1e-8, robust, q, loss, sums, N, H, W, ws, wsb, None)

    def bwd(preds=P(16), factors=I(4), weights=Fl(.32), S=1, gloss=one, label=one, mask=one, robust=0, q=0.0, sums=one, gp=P(16), reqs=I(1), N=1, H=8, W=8):
        return lib.multiscale_epe_bwd(gloss, preds, factors, weights, S, label, mask, 0, 1e-8, robust, q, sums, gp, reqs, N, H, W, None)
    for call in (fwd, bwd):
        assert call(H=9) == -2 and b"multiple" in lib.last_error()
        assert call(W=10) == -2
        assert call(H=0) == -2 and call(N=-1) == -2
        assert call(S=0) == -3 and b"n_scales" in lib.last_error()
        assert call(S=9) == -3
        assert call(factors=I(0)) == -3 and b"factor" in lib.last_error()
        assert call(factors=I(-2)) == -3
        assert call(robust=1, q=0.0) == -3 and b"q > 0" in lib.last_error()
        assert call(robust=1, q=-0.4) == -3
        assert call(label=None) == -1 and b"NULL" in lib.last_error()
        assert call(mask=None) == -1 and call(sums=None) == -1
        assert call(preds=P(None)) == -1
        assert call(preds=None) == -1 and call(factors=None) == -1 and call(weights=None) == -1
    assert fwd(loss=None) == -1
    assert fwd(ws=None, wsb=0) == -5 and b"workspace" in lib.last_error()
    assert fwd(H=64, W=64, wsb=2 * 2 * 4 - 4) == -5                # two slices of 2048 pixels, S + 1 = 2 floats each
    assert fwd(preds=P(None), label=None, mask=None, loss=None, sums=None, N=0, ws=None, wsb=0) == 0
    assert bwd(gloss=None) == -1
    assert bwd(gp=P(None)) == -1 and bwd(gp=None) == -1 and bwd(reqs=None) == -1
    assert bwd(reqs=I(2)) == -3 and b"req" in lib.last_error()
    assert bwd(gp=P(None), reqs=I(0)) == 0                         # req null: the gradient pointer may be NULL, nothing is launched
    assert bwd(preds=P(None), gp=P(None), gloss=None, label=None, mask=None, sums=None, N=0) == 0
    assert lib.multiscale_epe_workspace_bytes(2, 128, 192, 5) == 2 * 12 * 6 * 4
    assert lib.multiscale_epe_workspace_bytes(0, 8, 8, 1) == 0 and lib.multiscale_epe_workspace_bytes(1, 8, 8, 9) == 0


def test_ops_shape_errors_and_cpu_tensors():
    import torch
    from maskflownet_amd import ops, training
    from tests.emu import emu_ops
    o = emu_ops.emu_ops()
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ValueError, match="label must be"):
        o.multiscale_epe([z(1, 2, 2, 2)], z(1, 3, 8, 8), z(1, 1, 8, 8), (4,), (.32,))
    with pytest.raises(ValueError, match="mask must have shape"):
        o.multiscale_epe([z(1, 2, 2, 2)], z(1, 2, 8, 8), z(1, 1, 8, 4), (4,), (.32,))
    with pytest.raises(ValueError, match="prediction of scale 4"):
        o.multiscale_epe([z(1, 2, 2, 3)], z(1, 2, 8, 8), z(1, 1, 8, 8), (4,), (.32,))
    with pytest.raises(ValueError, match="prediction of scale 3"):
        o.multiscale_epe([z(1, 2, 2, 2)], z(1, 2, 8, 8), z(1, 1, 8, 8), (3,), (.32,))
    with pytest.raises(ValueError, match="one scale and one weight"):
        o.multiscale_epe([z(1, 2, 2, 2)], z(1, 2, 8, 8), z(1, 1, 8, 8), (4, 2), (.32,))
    with pytest.raises(ValueError, match="q must be positive"):
        o.multiscale_epe([z(1, 2, 2, 2)], z(1, 2, 8, 8), z(1, 1, 8, 8), (4,), (.32,), q=0.0)
    with pytest.raises(ValueError, match="gloss must be"):
        o.multiscale_epe_backward(z(2), [z(1, 2, 2, 2)], z(1, 2, 8, 8), z(1, 1, 8, 8), (4,), (.32,), z(1, 2))
    with pytest.raises(ValueError, match="needs the buffer"):
        o.multiscale_epe_backward(z(1), [z(1, 2, 2, 2)], z(1, 2, 8, 8), z(1, 1, 8, 8), (4,), (.32,), z(1, 2), reqs=["add"])
    t = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.multiscale_epe([t(1, 2, 2, 2)], t(1, 2, 8, 8), t(1, 1, 8, 8), (4,), (.32,))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.multiscale_epe_backward(t(1), [t(1, 2, 2, 2)], t(1, 2, 8, 8), t(1, 1, 8, 8), (4,), (.32,), t(1, 2))
    with pytest.raises(RuntimeError, match="no CPU"):
        training.FusedMultiscaleEpe(q=0.4)(t(1, 2, 64, 64), t(1, 1, 64, 64), *[t(1, 2, 64 // f, 64 // f) for f in DEFAULT_SCALES])


# ---- end to end on the GPU -----------------------------------------------------------------------------------------------------------
def _net_batch():
    import torch
    from maskflownet_amd import network, training
    from tests.test_training_step import _batch
    net = training.MaskFlownetSTrainable(network.random_params(0)).cuda()
    return net, [t.cuda() for t in _batch(2, 64, 64, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["sqrt", "q0.4"])
def test_gpu_fused_module_against_the_composed_one_and_fp64(form):
    import torch
    from maskflownet_amd import training
    q, eps = FORMS[form]
    net, (im1, im2, label, mask) = _net_batch()
    with torch.no_grad():
        preds = [p.contiguous() for p in net(im1, im2)[0]]
    losses, grads = {}, {}
    for name, mod in (("fused", training.FusedMultiscaleEpe(q=q)), ("composed", training.MultiscaleEpe(q=q))):
        ps = [p.clone().requires_grad_(True) for p in preds]
        loss = mod(label, mask, *ps)
        loss.sum().backward()
        losses[name], grads[name] = loss.detach().cpu().numpy(), [p.grad.cpu().numpy() for p in ps]
    assert all(g is not None for g in grads["fused"])
    a = ([p.cpu().numpy() for p in preds], label.cpu().numpy(), mask.cpu().numpy(), DEFAULT_SCALES, DEFAULT_WEIGHTS, eps, q)
    (l64, _), (lM, _) = lr.loss(*a), lr.loss(*a, magnitude=True)
    for name in losses:
        ratio = (np.abs(losses[name] - l64) / (64 * U * lM)).max()
        print("%s %s loss: %.3f of the 64-ulp bar" % (form, name, ratio))
        assert ratio <= 1.0, name
    gl = np.ones(2, np.float32)
    for f, g, w64, r32, M in zip(DEFAULT_SCALES, grads["fused"], lr.grads(gl, *a), lr.grads(gl, *a, dtype=np.float32), lr.grads(gl, *a, magnitude=True)):
        e_lib, e_ref = pc.check_fp64_bound(g, w64, r32, M, "%s fused gradient of scale %d" % (form, f))
        print("%s scale %d: e_lib %.2f ulp, e_twin %.2f ulp of M" % (form, f, e_lib / U, e_ref / U))


@pytest.mark.gpu
def test_gpu_four_steps_with_the_fused_robust_loss_lower_it():
    import torch
    from maskflownet_amd import training
    net, (im1, im2, label, mask) = _net_batch()
    loss_fn, opt = training.FusedMultiscaleEpe(q=0.4), torch.optim.Adam(net.parameters(), lr=1e-4)
    first = training.train_step(net, loss_fn, opt, im1, im2, label, mask)
    for _ in range(3):
        last = training.train_step(net, loss_fn, opt, im1, im2, label, mask)
    assert torch.isfinite(last).all() and last.sum().item() < first.sum().item()


@pytest.mark.gpu
def test_gpu_train_batch_with_the_fused_robust_loss():
    import torch
    from maskflownet_amd import augment, network, training
    from tests.test_augment_pipeline import _inputs, N, H, W
    im1, im2, label = (torch.from_numpy(a).cuda() for a in _inputs())
    net = training.MaskFlownetSTrainable(network.random_params(0)).cuda()
    geo, col = augment.presets("chairs", N, (H, W), (H, W), seed=3)
    loss, epe = training.train_batch(net, training.FusedMultiscaleEpe(q=0.4), torch.optim.Adam(net.parameters(), lr=1e-4), im1, im2, label, None, geo, col)
    assert loss.shape == (N,) and epe.shape == (N,) and torch.isfinite(loss).all() and torch.isfinite(epe).all()
