"""dc_mma_kernel's two ways of feeding the weight operand (kernels/deform_conv_mma.h): through stage buffers in LDS, or from memory
straight into registers (the AREG form: two register sets, requests hipcc does not count, no stage buffers, no block barrier in the
K loop).  Both run the same six products in the same order, so every output must be BIT FOR BIT the same.

The plan takes the AREG form at every tiling that has it -- (1, 4, 1), (3, 1, 6), (1, 1, 8): the network's levels 2, 4 and 5 --; bit 4
of the tuning key dc.off switches it off.  Level 3's (2, 3, 4) has none (its registers do not fit three waves per SIMD without
spills), nor have (2, 2, 2) and (1, 1, 4): there the bit must change nothing.  Per case: the call with and without the bit,
`array_equal` between the two, the plan's choice read back after each call (mfn_debug_last_dc_plan: tiling and form -- both forms
launch as `dc_mma` with the same grid, block and LDS request, so the launch record cannot tell them apart), the default call
repeated, and -- for the cases of tests/test_dc_mma_reduce_store.py on these tilings -- the SHA-256 of
tests/golden/dc_mma_reduce_store_v1.json (recorded from the kernel before either form existed) for both.

Cases, for each of the four tilings of the network's levels:
  * N = 2 on 6 x 8 (a ragged tile) and 8 x 24 (a block whose last pixel tiles are missing), drop-in and fused call;
  * channels giving ONE and TWO 16-channel groups per K slice (C = 16 / 32, 64 / 128, 96 / 192, 128 / 256): one group is where the
    prefetch of the next group's first operand runs past the slice, two where it crosses a group boundary inside the slice and a
    wrong wait count would show;
  * a Cout that is no multiple of 32;
  * the four gather tiers with the flows of tests/test_dc_mma_reduce_store.py (small window, big window, lanes outside the window,
    per-tap offsets: that tier reads the packed weights with plain loads in the AREG form), on the tiling with one K slice, the one
    with eight and the one whose K slices are shared by three pixel tiles;
and one drop-in case on each of (2, 2, 2) and (1, 1, 4).
The device runs every case.  The emulation runs every lane as a thread: measured there, the four fused two-group 8 x 24 cases take
40-115 s each (2 x 256 x 8 x 24 on (1, 1, 8): 114 s) and a repeated call adds half to every case (the whole file 8 minutes), so the
emulation leaves those four out -- two groups per slice run on 6 x 8 -- and repeats the call on the small tier cases only (its loads
are synchronous: a repeat can show nothing there that the first call did not).
A CPU test pins that the shipped library holds the AREG form of exactly the three tilings, without scratch."""
import json

import numpy as np
import pytest

from tests import parity_cases as pc
from tests import test_dc_mma_reduce_store as rs
from tests.fp64_env import Env

TILINGS = [(1, 4, 4, (16, 32)), (2, 3, 12, (64, 128)), (3, 1, 6, (96, 192)), (1, 1, 8, (128, 256))]   # mt, pt, nw, C (one / two groups per slice)
AREG_TILINGS = {(1, 4, 4), (3, 1, 6), (1, 1, 8)}   # (mt, pt, nw) the AREG form is built for
LDS_FORM, PLAN_FORM = 4, 0   # dc.off: the AREG form switched off / the plan
RESET = dict(rs.RESET, dc_off=0)


def _cases():
    """id -> (tuning, run(env) -> (got, call, oracles), golden id or None)"""
    out = {}
    for mt, pt, nw, cs in TILINGS:
        tag = "t%d_%d_%d" % (mt, pt, nw)
        tune = dict(dc_mma=1, dc_mt=mt, dc_pt=pt, dc_nw=nw)
        for C in cs:
            out[tag + "-dropin-2x%dx6x8" % C] = (tune, lambda e, C=C: rs.run_dropin(e, 2, C, C, 6, 8, 41), None)
            out[tag + "-fused-2x%dx8x24" % C] = (tune, lambda e, C=C: rs.run_fused(e, 2, C, 8, 24, 42), None)
        C = cs[0]
        cout = C - 24 if C > 32 else 8
        out[tag + "-cout%d-2x%dx6x8" % (cout, C)] = (tune, lambda e, C=C, cout=cout: rs.run_dropin(e, 2, C, cout, 6, 8, 43), None)
        for cid in sorted(rs.CASES):
            if cid.startswith(tag + "-"):
                out["golden-" + cid] = (rs.CASES[cid][0], rs.CASES[cid][2], cid)
    for mt, pt, nw, C in ((1, 4, 4, 32), (1, 1, 8, 128), (2, 3, 12, 64)):
        tag = "t%d_%d_%d" % (mt, pt, nw)
        tune = dict(dc_mma=1, dc_mt=mt, dc_pt=pt, dc_nw=nw)
        for nm, (gy, gx) in (("small-window", (0.0, 0.6)), ("big-window", (1.1, 0.9)), ("lanes-outside", (2.5, 2.5))):
            out[tag + "-tier-%s-1x%dx8x16" % (nm, C)] = (tune, lambda e, C=C, gy=gy, gx=gx: rs.run_fused(e, 1, C, 8, 16, 19, flow=pc.gradient_flow(1, 8, 16, gy, gx)), None)
        out[tag + "-tier-pertap-1x%dx5x12" % C] = (tune, lambda e, C=C: rs.run_dropin(e, 1, C, C, 5, 12, 21, pertap=True), None)
    for mt, pt, nw, C in ((2, 2, 4, 64), (1, 1, 4, 64)):   # tilings without the form
        out["t%d_%d_%d-dropin-2x%dx6x8" % (mt, pt, nw, C)] = (dict(dc_mma=1, dc_mt=mt, dc_pt=pt, dc_nw=nw), lambda e, C=C: rs.run_dropin(e, 2, C, C, 6, 8, 41), None)
    return out


CASES = _cases()
EMU_CASES = sorted(c for c in CASES if not any(c.endswith("-fused-2x%dx8x24" % t[3][1]) for t in TILINGS))


def _last_plan(env):
    """(mt, pt, nw, areg) of the thread's last dc_mma launch"""
    import ctypes
    if env.emu:
        ns = env.ops.ns
    else:
        from maskflownet_amd import _lib
        ns = _lib.lib()
    v = [ctypes.c_int(-1) for _ in range(4)]
    assert ns.debug_last_dc_plan(*[ctypes.byref(x) for x in v]) == 0
    mt, pt, kw, areg = (x.value for x in v)
    return mt, pt, pt * kw, areg


def _check(env, cid, golden):
    tune, run, gid = CASES[cid]
    tiling = (tune["dc_mt"], tune["dc_pt"], tune["dc_nw"])
    got = {}
    try:
        for form in (LDS_FORM, PLAN_FORM):
            env.set_tuning(**dict(tune, dc_off=form))
            with env.launches() as L:
                out, call, _ = run(env)
            L.expect(["dc_mma"], what="%s dc_off=%d" % (cid, form))
            want_areg = int(form == PLAN_FORM and tiling in AREG_TILINGS)
            assert _last_plan(env) == tiling + (want_areg,), "%s dc_off=%d: planned %s" % (cid, form, _last_plan(env))
            got[form] = out
        again = call() if not env.emu or "-tier-" in cid else out   # the plan's form once more
    finally:
        env.set_tuning(**RESET)
    np.testing.assert_array_equal(got[PLAN_FORM], got[LDS_FORM], err_msg="%s: the two forms differ" % cid)
    np.testing.assert_array_equal(again, got[PLAN_FORM], err_msg="%s: two runs of the same call differ" % cid)
    assert np.isfinite(got[PLAN_FORM]).all() and np.abs(got[PLAN_FORM]).max() > 0
    if golden is not None and gid is not None:
        assert gid in golden, gid
        for form in (LDS_FORM, PLAN_FORM):
            assert rs.sha(got[form]) == golden[gid], "%s dc_off=%d: not the bits of the kernel the golden hashes were recorded from" % (cid, form)


@pytest.fixture(scope="module")
def golden():
    with open(rs.GOLDEN) as f:
        return json.load(f)["sha256"]


@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


def test_the_cases_cover_the_golden_record_of_these_tilings():
    assert sum(1 for c in CASES.values() if c[2]) >= 4 * 4
    assert {c[2].split("-")[0] for c in CASES.values() if c[2]} == {"t%d_%d_%d" % t[:3] for t in TILINGS}


def test_the_library_ships_the_areg_form_of_these_tilings_without_scratch():
    """hipcc's resource remarks of the shipped library list dc_mma_kernel<.., AREG = true> for exactly these tilings, each without
    scratch or spills: a spill could move a register that an uncounted request is still to fill."""
    import subprocess
    from maskflownet_amd import _lib
    _lib.build()
    seen = set()
    for mangled, r in _lib.kernel_resources().items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        if "dc_mma_kernel<" in name and name.split(">")[0].endswith("false, true"):
            mt, pt, kw = (int(v) for v in name.split("<")[1].split(",")[:3])
            seen.add((mt, pt, pt * kw))
            assert r.get("ScratchSize [bytes/lane]") == "0" and r.get("VGPRs Spill") == "0", (name, r)
    assert seen == AREG_TILINGS, seen


@pytest.mark.parametrize("cid", EMU_CASES)
def test_emu_both_forms_give_the_same_bits(emu, golden, cid):
    _check(emu, cid, golden)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", sorted(CASES))
def test_gpu_both_forms_give_the_same_bits(gpu, cid):
    _check(gpu, cid, None)
