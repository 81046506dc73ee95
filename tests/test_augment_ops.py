"""The augmentation kernels of the training batch (maskflownet_amd/csrc/kernels/augment.h) and the host side that feeds them
(maskflownet_amd/augment.py).

Reference: tests/augment_ref.py, the header restated in numpy -- fp32 positions / grids / taps by definition, blends in fp64 (acceptance)
or fp32 (the twin).  Bars: parity_cases.check_fp64_bound with M = the same expression over absolute values (4 x the fp32 statement's
error + 16 * 2^-24, exact zeros where M == 0); means: 64 * 2^-24 * sum|terms| / n.  The kernel tables run on the emulation here and
under -m gpu on the MI355X.

The gamma step.  powf(v, e) of a clipped value v is judged on its own: M is the fp64 power itself, the input is the kernel's own
clipped value (its output with gamma off: the same instructions up to the clip).  Judging the whole chain against a power of the fp64
chain cannot work: where the chain cancels to v ~ 1e-6 its absolute error of ~1e-7 is a relative error of 0.1 of v and of v^e, whatever
computes it (the bar would be vacuous), and a pixel the fp64 chain clips to 0 that fp32 leaves at 1e-8 has M == 0 and a non-zero result."""
import ctypes

import numpy as np
import pytest

from tests import augment_ref as ar
from tests import parity_cases as pc
from tests import test_memory_contract as mc
from tests.fp64_env import Env

U = 2.0 ** -24


# ---- CPU: the reference itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_reference_philox_reproduces_the_published_vectors(ctr, key, want):
    assert tuple(int(v) for v in ar.philox4x32_10(*ctr, *key)) == want


NORMAL_SEED = 1


def test_reference_normals_are_standard_normal():
    n = 2 ** 18
    z = ar.normals([5], n, NORMAL_SEED, 3)[0]
    z32 = ar.normals([5], n, NORMAL_SEED, 3, np.float32)[0]
    print("2^18 normals: mean %.3e (bar %.3e), var - 1 %.3e (bar %.3e)" % (z.mean(), 5 / np.sqrt(n), z.var() - 1, 5 * np.sqrt(2 / n)))
    assert np.isfinite(z).all() and np.isfinite(z32).all()
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert np.abs(z32 - z).max() < 1e-5
    assert not np.array_equal(z, ar.normals([5], n, NORMAL_SEED, 4)[0]) and not np.array_equal(z, ar.normals([6], n, NORMAL_SEED, 3)[0])


def _chairs(batch, orig, target, seed=0):
    from maskflownet_amd import augment
    return augment.presets("chairs", batch, orig, target, seed=seed)


def geo_inputs(rng, N, Ho, Wo, kind="plain", mask_kind="plane"):
    if kind == "plain":
        i1, i2 = (rng.uniform(0, 1, (N, 3, Ho, Wo)).astype(np.float32) for _ in range(2))
        fl = (4 * rng.standard_normal((N, 2, Ho, Wo))).astype(np.float32)
    else:
        i1, i2 = (pc.graded_feat(rng, (N, 3, Ho, Wo), kind) for _ in range(2))
        fl = 4 * pc.graded_feat(rng, (N, 2, Ho, Wo), kind)
    mask = {"plane": np.ones((N, 1, Ho, Wo), np.float32), "const": np.ones((N, 1, 1, 1), np.float32),
            "sparse": (rng.uniform(size=(N, 1, Ho, Wo)) < 0.3).astype(np.float32)}[mask_kind]
    return i1, i2, fl, mask


@pytest.mark.parametrize("mask_kind", ["sparse", "plane"])
def test_reference_geometry_agrees_with_the_oracle_composition(mask_kind):
    """augment_ref.geometry against augmentation.py:305-338 composed literally from the oracle's GridGenerator(affine) and BilinearSampler
    in fp64 (grids, force translation by max / min over the grid, clip, concat, sample, divide, re-project).

    The only difference is where the sample positions are rounded.  With u = 2^-24, per axis of size S: xn carries <= 3.5 u (the
    rounded step times x <= 2: 2 u; the product: u; the sum into [-1,1]: u/2); a xn + b yn with |a| + |b| <= 1: 3.5 u + two products
    (u/2 each) + the sum (u/2) = 5 u; + t (a value < 2): u; - ft: u/2; (g + 1): u -- 7.5 u on g + 1, times (S-1)/2 = 3.75 u S pixels,
    plus the rounding of the product with (float)(S-1): u S.  That is < 4.75 u S pixels per axis in the worst case; the bar takes
    8 u max(Ho, Wo) pixels for the displacement, times the largest difference between neighbouring input samples (a bilinear surface
    moves by at most that per pixel of displacement), plus 16 u M for the fp64 roundings' order and the closed-form force translation.

    The flow's tolerance is divided by m': with the sparse mask it is loose wherever m' is small (there the quotient really is that
    sensitive to the positions); with the dense mask m' = 1 at every pixel and the flow's bar bites everywhere."""
    from oracle import ref as oracle
    from maskflownet_amd import augment
    N, (Ho, Wo), (Ht, Wt) = 2, (13, 18), (8, 12)
    rng = np.random.default_rng(11)
    geo, _ = _chairs(N, (Ho, Wo), (Ht, Wt), seed=5)
    tab = geo.table()
    i1, i2, fl, mask = geo_inputs(rng, N, Ho, Wo, mask_kind=mask_kind)
    t = tab.astype(np.float64)
    grid = oracle.grid_generator_affine(t[:, :6], (Ht, Wt), dtype=np.float64)
    ft = np.maximum(grid.max(axis=(2, 3), keepdims=True) - 1, 0) + np.minimum(grid.min(axis=(2, 3), keepdims=True) + 1, 0)
    assert np.abs(ft[:, :, 0, 0] - t[:, ar.AG_FT:ar.AG_FT + 2]).max() < 4 * U          # the closed form against the max / min over the grid
    grid = np.clip(grid - ft, -1, 1)
    shift = t[:, ar.AG_FSHIFT:ar.AG_FSHIFT + 2, None, None]
    cat = np.concatenate([i1, mask, (fl - shift) * mask], axis=1).astype(np.float64)
    s = oracle.bilinear_sampler(cat, grid, dtype=np.float64)
    o1, m, f = s[:, :3], s[:, 3:4], s[:, 4:6] / np.maximum(s[:, 3:4], 1e-8)
    grid2 = oracle.grid_generator_affine(t[:, 6:12], (Ht, Wt), dtype=np.float64) - ft + t[:, ar.AG_RT:ar.AG_RT + 2, None, None]
    o2 = oracle.bilinear_sampler(i2.astype(np.float64), grid2, dtype=np.float64)
    ident = oracle.grid_generator_affine(np.array([[1., 0, 0, 0, 1, 0]]), (Ht, Wt), dtype=np.float64)[0].reshape(2, -1)
    inv2, fac = t[:, ar.AG_INV2:ar.AG_INV2 + 4].reshape(N, 2, 2), t[:, ar.AG_FACTOR:ar.AG_FACTOR + 4].reshape(N, 2, 2)
    of = (inv2 @ f.reshape(N, 2, -1) + fac @ ident[None]).reshape(N, 2, Ht, Wt)
    got = ar.geometry(i1, i2, fl, mask, tab, (Ht, Wt))
    M = ar.geometry(i1, i2, fl, mask, tab, (Ht, Wt), magnitude=True)

    def step(a):
        return max(np.abs(np.diff(a, axis=2)).max(), np.abs(np.diff(a, axis=3)).max())
    px = 8 * U * max(Ho, Wo)
    den = np.maximum(got[3], 1e-8)
    scale = np.abs(inv2).sum(axis=2)[:, :, None, None]
    # f = S((flow - shift) mask) / m': numerator and denominator both move; |f| <= max |flow - shift|, a weighted mean of it
    tols = [px * step(i1), px * step(i2), px * scale * (step((fl - shift) * mask) + np.abs(fl - shift).max() * step(mask)) / den, px * step(mask)]
    for name, a, b, tol, m_ in zip(("img1", "img2", "flow", "mask"), got, (o1, o2, of, m), tols, M):
        err = np.abs(a - b) - 16 * U * m_
        print("%s: max |ref - oracle composition| %.3e, tolerance (least) %.3e" % (name, np.abs(a - b).max(), np.min(tol)))
        assert (err <= tol).all(), name


def test_host_parameters_of_the_chairs_preset():
    geo, col = _chairs(4, (384, 512), (320, 448), seed=2)
    corners = np.array([[x, y, 1.0] for x in (-1, 1) for y in (-1, 1)])
    for _ in range(250):       # 250 x batch 4 = 1 000 draws
        d = geo.draw()
        for k, (lo, hi) in geo.ranges().items():
            assert (d[k] >= lo).all() and (d[k] <= hi).all(), k
        t = geo.table(d).astype(np.float64)
        g = np.einsum("nij,cj->nci", t[:, :6].reshape(-1, 2, 3), corners) - t[:, None, ar.AG_FT:ar.AG_FT + 2]
        assert g.min() >= -1 - 1e-6 and g.max() <= 1 + 1e-6, (g.min(), g.max())
        c = col.draw()
        for k, (lo, hi) in col.ranges().items():
            assert (np.asarray(c[k]) >= lo).all() and (np.asarray(c[k]) <= hi).all(), k
        assert np.isfinite(col.table(c)).all()


def _identity_geo(N, shape):
    from maskflownet_amd import augment
    return augment.GeometryAugmentation((0, 0), (1, 1), 0, shape, shape, N, aspect_range=(1, 1), relative_angle=0.25, relative_scale=(1, 1),
                                        relative_translation=0.25)


def test_degenerate_ranges_give_the_identity_tables():
    t = _identity_geo(3, (64, 128)).table()
    want = np.zeros(26, np.float32)
    want[[0, 4, 6, 10, 18, 21]] = 1
    np.testing.assert_array_equal(t, np.tile(want, (3, 1)))


def test_flow_reprojection_closes_the_loop():
    """img2 = img1 smooth, flow 0, mask 1, the relative transform on: warping img2' by flow_out reproduces img1' where every tap lies
    inside.  The residual is calibrated by a control: inv2 / factor built from the relative rotation with its sign flipped."""
    from oracle import ref as oracle
    from maskflownet_amd import augment
    N, (Ho, Wo), (Ht, Wt) = 2, (64, 96), (48, 64)
    yy, xx = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    img = np.stack([0.5 + 0.2 * np.sin(2 * np.pi * xx / p) + 0.2 * np.cos(2 * np.pi * yy / q) for p, q in ((32, 40), (48, 36), (64, 52))])
    img = np.tile(img[None], (N, 1, 1, 1)).astype(np.float32)
    flow, mask = np.zeros((N, 2, Ho, Wo), np.float32), np.ones((N, 1, 1, 1), np.float32)
    geo = augment.GeometryAugmentation((-17, 17), (0.5, 1 / 0.9), 0.1, (Ht, Wt), (Ho, Wo), N, aspect_range=(0.9, 1 / 0.9),
                                       relative_angle=1.0, relative_scale=(0.96, 1 / 0.96), relative_translation=0.25, seed=3)
    d = geo.draw()
    d["rel_rotation"] = np.array([0.12, -0.1])               # a relative rotation of ~6 degrees: a few pixels at the border
    tab = geo.table(d)
    flipped = tab.copy()
    d2 = dict(d, rel_rotation=-d["rel_rotation"])
    flipped[:, ar.AG_INV2:] = geo.table(d2)[:, ar.AG_INV2:]

    def residual(table):
        o1, o2, f, _ = ar.geometry(img, img, flow, mask, table, (Ht, Wt))
        back = oracle.warp(o2, f[:, ::-1], dtype=np.float64)      # the oracle's warp takes (dy, dx)
        ok = ar.all_taps_inside(tab, (Ho, Wo), (Ht, Wt))
        fy, fx = f[:, 1] + np.arange(Ht)[None, :, None], f[:, 0] + np.arange(Wt)[None, None, :]
        ok &= (fy >= 0) & (fy <= Ht - 1) & (fx >= 0) & (fx <= Wt - 1)
        return np.abs(back - o1)[np.broadcast_to(ok[:, None], o1.shape)].mean(), 1 - ok.mean()
    r, out = residual(tab)
    rc, _ = residual(flipped)
    print("re-projection residual %.3e, control (rotation flipped) %.3e, excluded %.1f %%" % (r, rc, 100 * out))
    assert out <= 0.25 and 10 * r <= rc


def test_new_entries_fail_before_any_launch():
    from maskflownet_amd import _lib
    _lib.build()
    lib = _lib.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: argument checks come first
    geo = lambda *a: lib.augment_geometry(*a)
    assert geo(None, one, one, one, 1, one, one, one, one, one, 1, 8, 8, 4, 4, 0, None) == -1 and b"NULL" in lib.last_error()
    assert geo(one, one, one, one, 1, None, one, one, one, one, 1, 8, 8, 4, 4, 0, None) == -1
    assert geo(one, one, one, one, 1, one, one, one, one, None, 1, 8, 8, 4, 4, 0, None) == -1
    assert geo(one, one, one, one, 1, one, one, one, one, one, 1, 8, 8, 1, 4, 0, None) == -2 and b"target" in lib.last_error()
    assert geo(one, one, one, one, 1, one, one, one, one, one, 1, 8, 8, 4, 1, 0, None) == -2
    assert geo(one, one, one, one, 1, one, one, one, one, one, 1, 0, 8, 4, 4, 0, None) == -2
    assert geo(one, one, one, one, 1, one, one, one, one, one, -1, 8, 8, 4, 4, 0, None) == -2
    assert geo(None, None, None, None, 1, None, None, None, None, None, 0, 8, 8, 4, 4, 0, None) == 0
    assert lib.augment_color_mean_workspace_bytes(1, 52, 100) == 2 * 2 * 3 * 4     # ceil(5200 / 4096) = 2 slices, two images, three channels
    assert lib.augment_color_mean_workspace_bytes(0, 8, 8) == 0
    assert lib.augment_color_mean(one, None, one, 0.0, 0, 0, one, 1, 8, 8, one, 1 << 20, None) == -1
    assert lib.augment_color_mean(one, one, one, 0.0, 0, 0, None, 1, 8, 8, one, 1 << 20, None) == -1
    assert lib.augment_color_mean(one, one, one, 0.0, 0, 0, one, 1, 0, 8, one, 1 << 20, None) == -2
    assert lib.augment_color_mean(one, one, one, 0.0, 0, 0, one, 1, 8, 8, None, 0, None) == -5
    assert lib.augment_color_mean(one, one, one, 0.0, 0, 0, one, 1, 52, 100, one, 2 * 2 * 3 * 4 - 4, None) == -5 and b"workspace" in lib.last_error()
    assert lib.augment_color_mean(None, None, None, 0.0, 0, 0, None, 0, 8, 8, None, 0, None) == 0
    assert lib.augment_color(one, one, one, None, 0.0, 0, 0, 0, 0, one, 1, 8, 8, None) == -1
    assert lib.augment_color(one, one, one, one, 0.0, 0, 0, 0, 0, None, 1, 8, 8, None) == -1
    assert lib.augment_color(one, one, one, one, 0.0, 0, 0, 0, 0, one, 1, 8, -8, None) == -2
    assert lib.augment_color(None, None, None, None, 0.0, 0, 0, 0, 0, None, 0, 8, 8, None) == 0


def test_module_imports_without_a_gpu_and_the_ops_refuse_cpu_tensors():
    import torch
    from maskflownet_amd import augment, ops, training
    assert callable(augment.GeometryAugmentation) and callable(augment.ColorAugmentation) and callable(training.train_batch)
    geo, col = augment.presets("kitti", 2, (8, 8), (8, 8))
    x, f = torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        geo(x, x, f, torch.ones(2, 1, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU"):
        col(x, x)
    t = torch.zeros(2, 26)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_color_mean(x, x, t)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.augment_geometry(x, x, f, x[:, :1], t, (8, 8))


# ---- the kernel tables: the emulation here, the MI355X under -m gpu ------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


def _draw(N, rot=0.0, aspect=1.0, scale=1.0, shift=(0.0, 0.0), rel_rot=0.0, rel_scale=1.0, rel_t=(0.0, 0.0)):
    full = lambda v, s: np.broadcast_to(np.asarray(v, np.float64), s).copy()
    return {"rotation": full(rot, (N,)), "aspect": full(aspect, (N,)), "scale": full(scale, (N,)), "shift_unit": np.zeros((N, 2)),
            "shift": full(shift, (N, 2)), "rel_rotation": full(rel_rot, (N,)), "rel_scale": full(rel_scale, (N,)),
            "rel_translation": full(rel_t, (N, 2))}


def _table_rot(N, orig, target):
    from maskflownet_amd import augment
    return augment.geometry_table(_draw(N, rot=np.deg2rad(17.0), aspect=0.9, scale=0.8, shift=(0.05, -0.04), rel_rot=0.07, rel_scale=1.03,
                                        rel_t=(0.06, -0.05)), orig, target)


def _table_small(N, orig, target):
    from maskflownet_amd import augment
    return augment.geometry_table(_draw(N, rot=-0.2, aspect=1.05, scale=0.7, shift=(-0.03, 0.02), rel_rot=-0.05, rel_scale=0.97,
                                        rel_t=(-0.04, 0.03)), orig, target)


def _table_shifted(N, orig, target):
    """A translation that needs a force translation; half of it is then taken away again, so that the first grid leaves [-1,1] and the
    clip acts on a band of pixels; the second grid, moved further by rt, samples the zero padding."""
    from maskflownet_amd import augment
    t = augment.geometry_table(_draw(N, rot=0.1, scale=1.0, shift=(0.5, -0.4), rel_rot=0.1, rel_t=(0.3, 0.2)), orig, target)
    assert (np.abs(t[:, ar.AG_FT:ar.AG_FT + 2]) > 0.1).all()
    t[:, ar.AG_FT:ar.AG_FT + 2] *= np.float32(0.5)
    unclipped = t.copy()
    g = ar.grids(t[0], *target)
    x_raw = (t[0, 0] * g[4] + t[0, 1] * g[5]) + t[0, 2] - t[0, ar.AG_FT]
    assert (x_raw > 1.05).any() and not ar.all_taps_inside(unclipped, orig, target).all()
    return t


def _table_identity(N, orig, target):
    return _identity_geo(N, target).table()


GEO_CASES = {"rot17 Wt%4==0": (2, (13, 18), (8, 12), _table_rot), "scalar stores": (1, (9, 11), (7, 9), _table_small),
             "clip and padding": (2, (16, 20), (16, 20), _table_shifted), "identity": (1, (64, 128), (64, 128), _table_identity),
             "Wt%64==0": (1, (70, 132), (64, 128), _table_rot)}


def check_geometry(env, case, mask_kind, kind):
    N, orig, target, make = GEO_CASES[case]
    tab = make(N, orig, target)
    rng = np.random.default_rng([len(case), N, orig[0]])
    i1, i2, fl, mask = geo_inputs(rng, N, *orig, kind=kind, mask_kind=mask_kind)
    dev = [env.dev(a) for a in (i1, i2, fl, mask, tab)]
    with env.launches() as L:
        got = [np.array(env.host(a)) for a in env.ops.augment_geometry(*dev, target, label_order=0)]
        flipped = [np.array(env.host(a)) for a in env.ops.augment_geometry(*dev, target, label_order=1)]
    t2d = target[1] % 16 == 0 and target[0] % 4 == 0         # the plan of augment_geometry_launch (kernels/augment.h)
    L.expect(["augment_geometry_t2d" if t2d else ("augment_geometry_v4" if target[1] % 4 == 0 else "augment_geometry_v1")], what=case)
    for k in (0, 1, 3):
        np.testing.assert_array_equal(flipped[k], got[k])
    np.testing.assert_array_equal(flipped[2], got[2][:, ::-1])          # label_order = 1 is exactly the channel swap
    want64 = ar.geometry(i1, i2, fl, mask, tab, target)
    ref32 = ar.geometry(i1, i2, fl, mask, tab, target, dtype=np.float32)
    M = ar.geometry(i1, i2, fl, mask, tab, target, magnitude=True)
    if mask_kind == "sparse":
        m = want64[3]
        assert (m == 0).any() and ((m > 0) & (m < 0.05)).any()         # the 1e-8 floor and values next to it are reached
    for name, g, w, r, m in zip(("img1", "img2", "flow", "mask"), got, want64, ref32, M):
        what = "geometry %s %s %s: %s" % (case, mask_kind, kind, name)
        pc.assert_magnitude_bound(m, w, what)
        e_lib, e_ref = pc.check_fp64_bound(g, w, r, m, what)
        print("%s: e_lib %.3e, e_ref32 %.3e, bit-equal to the fp32 statement: %s" % (what, e_lib, e_ref, np.array_equal(g, r)))
    if case == "identity" and mask_kind != "sparse":                     # the op returns its inputs
        for g, a in zip(got[:3], (i1, i2, fl)):                          # ... up to the fp32 positions (the bound of the oracle test above)
            step = max(np.abs(np.diff(a, axis=2)).max(), np.abs(np.diff(a, axis=3)).max())
            assert (np.abs(g - a) <= 8 * U * max(orig) * step + 16 * U * np.abs(a)).all()


GEO_PARAMS = [(c, m, k) for c in GEO_CASES for m in ("plane", "const", "sparse") for k in ("plain", "graded-pixel")]


@pytest.mark.parametrize("case,mask_kind,kind", GEO_PARAMS)
def test_emu_geometry_against_fp64(emu, case, mask_kind, kind):
    check_geometry(emu, case, mask_kind, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("case,mask_kind,kind", GEO_PARAMS)
def test_gpu_geometry_against_fp64(gpu, case, mask_kind, kind):
    check_geometry(gpu, case, mask_kind, kind)


def check_geometry_taps(env):
    """One-hot planes, one per source pixel of 6 x 8 (16 samples x 3 channels): the set of non-zero outputs is exactly the reference's."""
    N, orig, target = 16, (6, 8), (7, 9)
    tab = _table_small(N, orig, target)
    eye = np.eye(48, dtype=np.float32).reshape(N, 3, 6, 8)
    fl, mask = np.zeros((N, 2, 6, 8), np.float32), np.ones((N, 1, 1, 1), np.float32)
    got = [np.array(env.host(a)) for a in env.ops.augment_geometry(*(env.dev(a) for a in (eye, eye, fl, mask, tab)), target)]
    ref32 = ar.geometry(eye, eye, fl, mask, tab, target, dtype=np.float32)
    for k in (0, 1):
        assert (ref32[k] != 0).any()
        np.testing.assert_array_equal(got[k] != 0, ref32[k] != 0)
        np.testing.assert_array_equal(got[k], ref32[k])                 # the weights themselves


def test_emu_geometry_taps_are_the_references(emu):
    check_geometry_taps(emu)


@pytest.mark.gpu
def test_gpu_geometry_taps_are_the_references(gpu):
    check_geometry_taps(gpu)


def _views(env, shapes, misalign):
    """Destinations inside fills of 7.0; the one named by `misalign` starts 4 bytes past a 16-byte boundary."""
    bufs, views = [], []
    for k, s in enumerate(shapes):
        n = int(np.prod(s))
        if env.emu:
            raw = np.full(n + 40, 7.0, np.float32)
            lo = (-raw.ctypes.data % 64) // 4 + 16 + (1 if k == misalign else 0)
        else:
            import torch
            raw = torch.full((n + 40,), 7.0, device="cuda:0")
            assert raw.data_ptr() % 64 == 0
            lo = 16 + (1 if k == misalign else 0)
        v = raw[lo:lo + n].reshape(s) if env.emu else raw[lo:lo + n].view(s)
        assert env.ops.ad.ptr(v) % 16 == (4 if k == misalign else 0)
        bufs.append((raw, lo, n))
        views.append(v)
    return bufs, views


def check_geometry_misaligned(env):
    N, orig, target, make = GEO_CASES["rot17 Wt%4==0"]
    tab = make(N, orig, target)
    ins = [env.dev(a) for a in geo_inputs(np.random.default_rng(8), N, *orig)] + [env.dev(tab)]
    shapes = [(N, 3) + target, (N, 3) + target, (N, 2) + target, (N, 1) + target]
    with env.launches() as L:
        aligned = [np.array(env.host(a)) for a in env.ops.augment_geometry(*ins, target)]
    L.expect(["augment_geometry_v4"], absent=["augment_geometry_v1"])
    bufs, views = _views(env, shapes, misalign=2)
    with env.launches() as L:
        env.ops.augment_geometry(*ins, target, out=tuple(views))
    L.expect(["augment_geometry_v1"], absent=["augment_geometry_v4"])
    for (raw, lo, n), v, a in zip(bufs, views, aligned):
        np.testing.assert_array_equal(np.array(env.host(v)), a)
        flat = np.array(env.host(raw))
        assert (flat[:lo] == 7.0).all() and (flat[lo + n:] == 7.0).all()


def test_emu_geometry_into_a_misaligned_destination(emu):
    check_geometry_misaligned(emu)


@pytest.mark.gpu
def test_gpu_geometry_into_a_misaligned_destination(gpu):
    check_geometry_misaligned(gpu)


# ---- colour --------------------------------------------------------------------------------------------------------------------------
SEED, OFFSET = 0x9E3779B97F4A7C15, (1 << 32) + 5      # both halves of the key and of the offset in use
COLOR_SHAPES = [(2, 3, 5, 7), (1, 3, 52, 100), (2, 3, 64, 128)]
COLOR_PARAMS = [(s, sg, g, e) for s in COLOR_SHAPES for sg in (0.0, 0.04) for g in (False, True) for e in (False, True)]


def color_inputs(shape, eigen):
    from maskflownet_amd import augment
    rng = np.random.default_rng([shape[0], shape[2], int(eigen)])
    a, b = (rng.uniform(0, 1, shape).astype(np.float32) for _ in range(2))
    col = augment.ColorAugmentation((-0.4, 0.8), 0.1, (0.8, 1.4), shape[0], shape[2:], (0, 0.04), 0.5, 0.5, gamma_range=(-0.5, 0.5),
                                    eigen_aug=eigen, seed=shape[3])
    return a, b, col.table(col.draw())


def check_color(env, shape, sigma, gamma, eigen):
    a, b, tab = color_inputs(shape, eigen)
    da, db, dt = env.dev(a), env.dev(b), env.dev(tab)
    what = "colour %s sigma=%g gamma=%s eigen=%s" % (shape, sigma, gamma, eigen)
    with env.launches() as L:
        mean_d = env.ops.augment_color_mean(da, db, dt, sigma, SEED, OFFSET)
        again = env.ops.augment_color_mean(da, db, dt, sigma, SEED, OFFSET)
    L.expect(["augment_color_mean_partial", "augment_color_mean_final"], what=what)
    mean = np.array(env.host(mean_d))
    np.testing.assert_array_equal(np.array(env.host(again)), mean)                     # bit-identical when repeated
    want, bound = ar.color_mean(a, b, tab, sigma, SEED, OFFSET)
    print("%s: means max err / bound = %.3f" % (what, (np.abs(mean - want) / bound).max()))
    assert (np.abs(mean - want) <= bound).all()

    def run(g, seed=SEED, offset=OFFSET, mean=None):
        return np.array(env.host(env.ops.augment_color(da, db, dt, sigma, seed, offset, spin=eigen, gamma=g, mean=mean)))
    pre = run(False, mean=mean_d)
    for own_mean, label in ((mean, "the kernel's means"), (None, "end to end")):
        got = pre if own_mean is not None else run(False)
        w64 = ar.color(a, b, tab, sigma, SEED, OFFSET, spin=eigen, mean=own_mean)
        r32 = ar.color(a, b, tab, sigma, SEED, OFFSET, spin=eigen, mean=own_mean, dtype=np.float32)
        M = ar.color(a, b, tab, sigma, SEED, OFFSET, spin=eigen, mean=own_mean, magnitude=True)
        pc.assert_magnitude_bound(M, w64, what)
        e_lib, e_ref = pc.check_fp64_bound(got, w64, r32, M, "%s (%s)" % (what, label))
        print("%s (%s): e_lib %.3e, e_ref32 %.3e" % (what, label, e_lib, e_ref))
    np.testing.assert_array_equal(run(False), pre)                                      # the default mean is augment_color_mean's
    assert (pre == 0).any() and (pre == 1).any() and pre.min() >= 0 and pre.max() <= 1  # clipped pixels are exactly 0 / 1
    out = pre
    if gamma:
        out = run(True, mean=mean_d)
        e_lib, e_ref = pc.check_fp64_bound(out, ar.gamma(pre, tab), ar.gamma(pre, tab, np.float32), ar.gamma(pre, tab), what + " (powf)")
        print("%s (powf of the kernel's clipped values): e_lib %.3e, e_ref32 %.3e" % (what, e_lib, e_ref))
        np.testing.assert_array_equal(out[pre == 0], 0)
        np.testing.assert_array_equal(out[pre == 1], 1)                                 # ... and powf keeps them so
        np.testing.assert_array_equal(run(True), out)
    other = run(gamma, mean=mean_d, seed=SEED + 1, offset=OFFSET + 1)
    if sigma == 0:
        np.testing.assert_array_equal(other, out)                                       # no generator: seed and offset do not matter
        np.testing.assert_array_equal(np.array(env.host(env.ops.augment_color_mean(da, db, dt, sigma, 1, 2))), mean)
    else:
        assert (run(gamma, mean=mean_d, offset=OFFSET + 1) != out).mean() > 0.5          # another offset: other noise
        assert (other != out).mean() > 0.5
        np.testing.assert_array_equal(run(gamma, mean=mean_d), out)                      # the same offset: the same bits


@pytest.mark.parametrize("shape,sigma,gamma,eigen", COLOR_PARAMS)
def test_emu_color_against_fp64(emu, shape, sigma, gamma, eigen):
    check_color(emu, shape, sigma, gamma, eigen)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,sigma,gamma,eigen", COLOR_PARAMS)
def test_gpu_color_against_fp64(gpu, shape, sigma, gamma, eigen):
    check_color(gpu, shape, sigma, gamma, eigen)


def check_device_normals(env):
    """The kernels' normals themselves: M = 0, sigma = 1/8, mean 0, channel 0, brightness 0 leave clip(+-z / 8, 0, 1) with cc = +-1 --
    every step but the generator exact -- so z = 8 (out+ - out-), against fp64 Box-Muller of the same Philox words, M = r."""
    shape = (1, 3, 52, 100)
    a = np.random.default_rng(0).uniform(0, 1, shape).astype(np.float32)
    zero = env.dev(np.zeros((2, 3), np.float32))
    outs = []
    for cc in (1.0, -1.0):
        tab = np.zeros((1, 26), np.float32)
        tab[0, ar.AC_CC:ar.AC_CC + 3], tab[0, ar.AC_E] = cc, 1.0
        outs.append(np.array(env.host(env.ops.augment_color(env.dev(a), env.dev(a), env.dev(tab), 0.125, SEED, OFFSET, mean=zero))))
    assert ((outs[0] == 0) | (outs[1] == 0)).all() and max(outs[0].max(), outs[1].max()) < 1
    z = 8.0 * (outs[0].astype(np.float64) - outs[1])
    planes, npix = list(range(6)), 52 * 100
    z64 = ar.normals(planes, npix, SEED, OFFSET).reshape(z.shape)
    z32 = ar.normals(planes, npix, SEED, OFFSET, np.float32).reshape(z.shape)
    r = ar.normals(planes, npix, SEED, OFFSET, magnitude=True).reshape(z.shape)
    e_lib, e_ref = pc.check_fp64_bound(z, z64, z32, r, "device normals")
    print("device normals: e_lib %.3e, e_ref32 (numpy fp32 statement) %.3e, ratio %.2f" % (e_lib, e_ref, e_lib / e_ref))


def test_emu_normals_against_fp64(emu):
    check_device_normals(emu)


@pytest.mark.gpu
def test_gpu_normals_against_fp64(gpu):
    check_device_normals(gpu)


# ---- memory contract: each op plain and twice between guard bands, workspaces of exactly the queried size ---------------------------------
def _contract_cases():
    N, orig, target, make = GEO_CASES["rot17 Wt%4==0"]
    g_in = list(geo_inputs(np.random.default_rng(21), N, *orig, mask_kind="sparse")) + [make(N, orig, target)]
    g_const = list(geo_inputs(np.random.default_rng(22), 1, 9, 11, mask_kind="const")) + [_table_small(1, (9, 11), (7, 9))]
    a, b, tab = color_inputs((1, 3, 52, 100), True)
    a2, b2, tab2 = color_inputs((2, 3, 5, 7), False)

    def mean_call(env):
        assert env.ops.ns.augment_color_mean_workspace_bytes(1, 52, 100) == 48
        return env.ops.augment_color_mean(env.dev(a), env.dev(b), env.dev(tab), 0.04, SEED, OFFSET)
    return {
        "augment_geometry": mc.Case(lambda env: env.ops.augment_geometry(*(env.dev(x) for x in g_in), target), ["augment_geometry_v4"]),
        "augment_geometry const mask": mc.Case(lambda env: env.ops.augment_geometry(*(env.dev(x) for x in g_const), (7, 9), label_order=1),
                                               ["augment_geometry_v1"]),
        "augment_color_mean": mc.Case(mean_call, ["augment_color_mean_partial", "augment_color_mean_final"]),
        "augment_color": mc.Case(lambda env: env.ops.augment_color(env.dev(a), env.dev(b), env.dev(tab), 0.04, SEED, OFFSET, spin=True, gamma=True),
                                 ["augment_color_mean_partial", "augment_color_mean_final", "augment_color_v4"]),
        "augment_color scalar": mc.Case(lambda env: env.ops.augment_color(env.dev(a2), env.dev(b2), env.dev(tab2), 0.0), ["augment_color_v1"]),
    }


CONTRACT = _contract_cases()


@pytest.mark.parametrize("name", list(CONTRACT))
def test_emu_memory_contract(emu, name):
    mc.contract(emu, name, CONTRACT[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONTRACT))
def test_gpu_memory_contract(gpu, name):
    mc.contract(gpu, name, CONTRACT[name])
