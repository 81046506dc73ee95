"""dc_mma_kernel's K-slice reduction and epilogue (kernels/deform_conv_mma.h): every wave of a pixel tile sums a slab of the tile's
filter rows over the K slices (slice order 0..KW-1) and stores it, 16 bytes per lane.

The summation order is the one the kernel always had, so every output is pinned BIT FOR BIT: tests/golden/dc_mma_reduce_store_v1.json
holds a SHA-256 of the output bytes of every case below, recorded by tools/make_dc_mma_golden.py on the emulation (tests/emu)
of the kernel as it was when tile mt was summed and stored by slice mt % KW alone.  Every case also stays within the fp64 acceptance
bound of tests/test_forward_fp64.py (parity_cases.check_fp64_bound) and gives the same bytes when the call is repeated.

Cases -- the smallest shapes at which the slab split can go wrong:
  * every tiling of tests/test_emu_parity.py DCM_TILINGS (KW in {1, 2, 4, 6, 8}, MT in {1, 2, 3}, PT in {1, 2, 3, 4}) on 1 x C x 6 x 8
    (fused call, raw and packed weights) and 2 x C x 5 x 12 (drop-in call without a bias: ragged tile rows and columns, the store tail
    ox + 3 >= W, W = 12 where a quad straddles the tile edge);
  * ragged filters: Cout = C - 24 and (one or two filter tiles per wave; three tiles per wave need three tiles) Cout = 40, with a
    bias -- a slab's rows lie partly or wholly past Cout;
  * the matching epilogue, mask / tradeoff / LeakyReLU together on every tiling, each alone on two K-sliced tilings;
  * the CONV form on its K-sliced tiling (2, 3, 4) with Cin = 56 (no multiple of 16), input and output channel slices of one concat
    buffer (x_nstride, out_nstride), with and without a bias;
  * the window tiers on a K-sliced tiling: a gradient flow the small window holds, one only the big window holds, one that leaves
    lanes outside both, a flow without any coherence (parity_cases.wild_flow, its absurd values at 1000 pixels), per-tap offsets.
Uneven slabs do not exist: 32 MT filter rows divide by KW for every (MT, KW) of DCM_TILINGS, and the kernel refuses to compile for
a tiling where they would not (static_assert in DcmGeom).  out_nstride reaches dc_mma_kernel through the CONV form only: the
deformable calls of the C ABI take dense outputs, no slice.

The `gpu` twins run the same cases through the C ABI on the device: the fp64 bound and the repeated call (the device's bits are not
the emulation's -- expf, contraction --; its bit identity with the previous kernel is measured on bench.py --dump-outputs,
profiles/dc_mma_fixed_cost.md)."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import ref as oracle
from oracle import ref_numpy
from tests import parity_cases as pc
from tests.fp64_env import Env, exact_positions, per_image
from tests.test_emu_parity import DCM_TILINGS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dc_mma_reduce_store_v1.json")
K33 = dict(kernel=(3, 3), pad=(1, 1))
SENTINEL = np.float32(-12345.5)


def _leaky32(a):
    return np.where(a > 0, a, np.float32(0.1) * a).astype(np.float32)


def _leaky64(a):
    return np.where(a > 0, a, 0.1 * a)


def _flow(rng, N, H, W):
    """a flow on a 2^-10 grid: flow * 20 / 8 is exact, the offsets lie on the exact_positions grid (tests/fp64_env.py)"""
    return exact_positions(pc.flow_field(rng, N, H, W) * np.float32(8.0 / 20.0), 2.0 ** -10)


def _dc_oracles(x, off, w, b):
    kw = dict(kernel=(3, 3), pad=(1, 1))
    r32 = np.concatenate(per_image(lambda xx, o: oracle.deformable_convolution(xx, o, w, b, **kw), x, off))
    r64 = np.concatenate(per_image(lambda xx, o: oracle.deformable_convolution(xx, o, w, b, dtype=np.float64, **kw), x, off))
    M = np.concatenate(per_image(lambda xx, o: ref_numpy.deformable_convolution_bound(xx, o, w, None), x, off))
    if b is not None:
        M = M + np.abs(b.astype(np.float64))[None, :, None, None]
    return r32, r64, M


def _inputs(seed, N, C, Cout, H, W, bias=True):
    rng = np.random.default_rng(seed)
    x = pc.feat(rng, (N, C, H, W))
    w = pc.msra_weight(rng, Cout, C)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32) if bias else None
    return rng, x, w, b


def run_fused(env, N, C, H, W, seed, flow=None, packed=False):
    """deformable_convolution_shared (flow mode); packed: the weights packed once must give the raw call's bits."""
    rng, x, w, b = _inputs(seed, N, C, C, H, W)
    fl = _flow(rng, N, H, W) if flow is None else exact_positions(np.asarray(flow, np.float32) * np.float32(8.0 / 20.0), 2.0 ** -10)
    off = oracle.offsets_from_flow(fl, 20.0, 8.0)
    xd, fd, wd, bd = env.dev(x), env.dev(fl), env.dev(w), env.dev(b)
    call = lambda: env.host(env.ops.deformable_convolution_shared(xd, fd, 20.0, 8.0, wd, bd))
    got = call()
    if packed:
        pk = env.ops.pack_deform_weights(wd, (N, C, H, W), **K33)
        np.testing.assert_array_equal(env.host(env.ops.deformable_convolution_shared(xd, fd, 20.0, 8.0, wd, bd, packed=pk)), got)
    return got, call, lambda: _dc_oracles(x, off, w, b)


def run_dropin(env, N, C, Cout, H, W, seed, bias=True, pertap=False):
    """DeformableConvolution with the offset tensor: nine equal offsets per pixel (the reference's call), or per-tap offsets."""
    rng, x, w, b = _inputs(seed, N, C, Cout, H, W, bias)
    if pertap:
        off = (rng.standard_normal((N, 18, H, W)) * 1.5).astype(np.float32)
        off[:, :, 0, 0] = np.float32(3.0 * max(H, W))
        off = exact_positions(off)
    else:
        off = oracle.offsets_from_flow(_flow(rng, N, H, W), 20.0, 8.0)
    xd, od, wd, bd = env.dev(x), env.dev(off), env.dev(w), env.dev(b) if b is not None else None
    call = lambda: env.host(env.ops.DeformableConvolution(xd, od, wd, bd, num_filter=Cout, no_bias=b is None, **K33))
    return call(), call, lambda: _dc_oracles(x, off, w, b)


def run_matching(env, N, C, H, W, seed, mask=True, add=True, leaky=True):
    rng, x, w, b = _inputs(seed, N, C, C, H, W)
    fl = _flow(rng, N, H, W)
    off = oracle.offsets_from_flow(fl, 20.0, 8.0)
    m = (rng.standard_normal((N, 1, H, W)) * 2).astype(np.float32) if mask else None
    tr = rng.standard_normal((N, C, H, W)).astype(np.float32) if add else None
    d = lambda a: env.dev(a) if a is not None else None
    xd, fd, wd, bd, md, td = env.dev(x), env.dev(fl), env.dev(w), env.dev(b), d(m), d(tr)
    call = lambda: env.host(env.ops.deformable_matching(xd, fd, 20.0, 8.0, wd, bd, md, td, leaky=leaky))

    def oracles():
        r32, r64, M = _dc_oracles(x, off, w, b)
        if m is not None:
            r32 = r32 * (np.float32(1) / (np.float32(1) + np.exp(-m, dtype=np.float32)))
            r64 = r64 / (1.0 + np.exp(-m.astype(np.float64)))
        if tr is not None:
            r32, r64 = r32 + tr, r64 + tr.astype(np.float64)
        if leaky:
            r32, r64 = _leaky32(r32), _leaky64(r64)
        return r32.astype(np.float32), r64, ref_numpy.matching_bound(M, m, tr)

    return call(), call, oracles


def run_conv_slices(env, N, Cin, Cout, H, W, seed, bias=True):
    """x = concat(conv(x), x): the CONV form reads the channel suffix of a concat buffer whose prefix is not written yet (NaN: never
    read) and writes the prefix; packed weights, fused LeakyReLU."""
    import torch
    rng = np.random.default_rng(seed)
    x = pc.feat(rng, (N, Cin, H, W))
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (1.01 * Cin * 9))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32) if bias else None
    full = np.full((N, Cout + Cin + 3, H, W), np.float32(np.nan))
    full[:, Cout:Cout + Cin] = x
    full[:, Cout + Cin:] = SENTINEL
    wd, bd = env.dev(w), env.dev(b) if b is not None else None
    pk = env.ops.pack_conv_weights(wd, (N, Cin, H, W), **K33)

    def call():
        buf = env.dev(full)
        env.ops.Convolution(buf[:, Cout:Cout + Cin], wd, bd, pad=(1, 1), num_filter=Cout, no_bias=b is None, out=buf[:, :Cout],
                            activation="leaky", packed=pk)
        h = env.host(buf)
        np.testing.assert_array_equal(h[:, Cout:Cout + Cin], x)
        assert (h[:, Cout + Cin:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), "wrote outside the slice"
        return np.ascontiguousarray(h[:, :Cout])

    def oracles():
        F = torch.nn.functional
        t = lambda a, dt: None if a is None else torch.tensor(a, dtype=dt)
        cv = lambda xx, ww, bb, dt: F.conv2d(t(xx, dt), t(ww, dt), t(bb, dt), padding=1).numpy()
        return (_leaky32(cv(x, w, b, torch.float32)), _leaky64(cv(x, w, b, torch.float64)),
                cv(np.abs(x), np.abs(w), None if b is None else np.abs(b), torch.float64))

    return call(), call, oracles


def _cases():
    """id -> (tuning, kernel, run(env) -> (got, call, oracles))"""
    out = {}
    for mt, pt, nw, C in DCM_TILINGS:
        tag = "t%d_%d_%d" % (mt, pt, nw)
        tune = dict(dc_mma=1, dc_mt=mt, dc_pt=pt, dc_nw=nw)
        out[tag + "-fused-packed-1x%dx6x8" % C] = (tune, "dc_mma", lambda e, C=C: run_fused(e, 1, C, 6, 8, 11, packed=True))
        out[tag + "-dropin-nobias-2x%dx5x12" % C] = (tune, "dc_mma", lambda e, C=C: run_dropin(e, 2, C, C, 5, 12, 12, bias=False))
        out[tag + "-cout%d-1x%dx6x8" % (C - 24, C)] = (tune, "dc_mma", lambda e, C=C: run_dropin(e, 1, C, C - 24, 6, 8, 13))
        if mt <= 2 and C != 64:   # (C = 64: C - 24 is 40)
            out[tag + "-cout40-1x%dx6x8" % C] = (tune, "dc_mma", lambda e, C=C: run_dropin(e, 1, C, 40, 6, 8, 14))
        out[tag + "-matching-1x%dx6x8" % C] = (tune, "dc_mma", lambda e, C=C: run_matching(e, 1, C, 6, 8, 15))
    for mt, pt, nw, C in [(1, 1, 4, 64), (2, 2, 4, 64)]:
        tag = "t%d_%d_%d" % (mt, pt, nw)
        tune = dict(dc_mma=1, dc_mt=mt, dc_pt=pt, dc_nw=nw)
        for nm, opt in (("mask", dict(add=False, leaky=False)), ("add", dict(mask=False, leaky=False)), ("leaky", dict(mask=False, add=False)),
                        ("all", dict())):
            out[tag + "-matching-%s-2x%dx5x12" % (nm, C)] = (tune, "dc_mma", lambda e, C=C, opt=opt: run_matching(e, 2, C, 5, 12, 16, **opt))
    conv = dict(conv_dcm=2)   # Cout = 64, four 16-channel groups (the last with 8 channels): the K-sliced (2, 3, 4) tiling
    out["conv_t2_3_12-slices-2x56x5x12"] = (conv, "conv3x3_dcm", lambda e: run_conv_slices(e, 2, 56, 64, 5, 12, 17))
    out["conv_t2_3_12-slices-nobias-1x56x6x8"] = (conv, "conv3x3_dcm", lambda e: run_conv_slices(e, 1, 56, 64, 6, 8, 18, bias=False))
    tune = dict(dc_mma=1, dc_mt=1, dc_pt=1, dc_nw=4)
    for nm, (gy, gx) in (("small-window", (0.0, 0.6)), ("big-window", (1.1, 0.9)), ("lanes-outside", (2.5, 2.5))):
        out["t1_1_4-tier-%s-1x64x8x16" % nm] = (tune, "dc_mma", lambda e, gy=gy, gx=gx: run_fused(e, 1, 64, 8, 16, 19, flow=pc.gradient_flow(1, 8, 16, gy, gx)))
    # (wild_flow's 1e9 and -3e38 clipped to 1000 pixels: far outside every window all the same, and the fp64 oracle's bound can take them)
    out["t1_1_4-tier-wild-1x64x9x16"] = (tune, "dc_mma", lambda e: run_fused(e, 1, 64, 9, 16, 20,
                                                                             flow=np.clip(pc.wild_flow(np.random.default_rng(31), 1, 9, 16), -1000.0, 1000.0)))
    out["t1_1_4-tier-pertap-1x64x5x12"] = (tune, "dc_mma", lambda e: run_dropin(e, 1, 64, 64, 5, 12, 21, pertap=True))
    return out


CASES = _cases()
RESET = dict(dc_mma=-1, dc_mt=0, dc_pt=0, dc_nw=0, conv_dcm=0)


def sha(a):
    a = np.ascontiguousarray(a, np.float32)
    return hashlib.sha256(("%s|" % (a.shape,)).encode() + a.tobytes()).hexdigest()


def run_case(env, cid):
    """(output, the call for a second run, the oracles) of case `cid` under its tuning, which is reset afterwards."""
    tune, kernel, run = CASES[cid]
    env.set_tuning(**tune)
    try:
        with env.launches() as L:
            got, call, oracles = run(env)
        L.expect([kernel], what=cid)
        again = call()
    finally:
        env.set_tuning(**RESET)
    return got, again, oracles


def _check(env, cid, golden):
    got, again, oracles = run_case(env, cid)
    assert got.tobytes() == again.tobytes(), "%s: two runs of the same call differ" % cid
    if golden is not None:
        assert cid in golden, "%s: no golden hash (tools/make_dc_mma_golden.py)" % cid
        assert sha(got) == golden[cid], "%s: the output's bits are not those of the kernel the golden hashes were recorded from" % cid
    ref32, want64, M = oracles()
    e_lib, e_ref = pc.check_fp64_bound(got, want64, ref32, M, what=cid)
    print("%-48s max e_lib %.3e   max e_ref32 %.3e" % (cid, e_lib, e_ref))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["sha256"]


@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


def test_slabs_of_the_shipped_tilings_are_even():
    """32 MT filter rows over KW waves: no shipped tiling leaves a remainder (the docstring's claim)."""
    for mt, pt, nw, _ in DCM_TILINGS:
        assert (32 * mt) % (nw // pt) == 0, (mt, pt, nw)
    assert {nw // pt for _, pt, nw, _ in DCM_TILINGS} == {1, 2, 4, 6, 8}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_emu_bits_of_the_previous_kernel_fp64_bound_and_repeat(emu, golden, cid):
    _check(emu, cid, golden)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_gpu_fp64_bound_and_repeat(gpu, cid):
    _check(gpu, cid, None)
