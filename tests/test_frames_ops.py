"""The operators of maskflownet_amd/csrc/kernels/frames.h: the joint mean and the network's input batch straight from uint8 HWC frames,
and the colour picture of a flow [flow_vis-ext, unpinned].

References: tests/flowviz_ref.py (the numpy statements) and, for preprocess_pair_u8, the float operator preprocess_pair fed the floats
byte / 255 of predict._chw01 -- bit for bit.
Bars: pair_mean_u8 -- bit-identical to np.float32(np.float64(sum) / np.float64(255 * 2 * H * W)) (integer sums have no order);
preprocess_pair_u8 -- torch.equal; flow_color -- every byte in {floor(x - d), floor(x + d)} for the fp64 x = 255 * col and d = 0.01:
the fp32 chain's error in x is bounded by about 4e-3 (atan2f to a few ulp times the 54 steps of fk times the wheel's largest step
64/255, plus a handful of roundings), d is 2.5 times that; a numpy fp32 run differs from fp64 by 1.6e-4 at most."""
import ctypes

import numpy as np
import pytest

from tests import flowviz_ref as fv

DELTA = 0.01


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_reference_colour_statement_anchors_and_known_colours():
    w = fv.wheel()
    assert w.shape == (55, 3)
    for k, rgb in {0: (255, 0, 0), 14: (255, 238, 0), 15: (255, 255, 0), 21: (0, 255, 0), 25: (0, 255, 255), 27: (0, 209, 255),
                   36: (0, 0, 255), 49: (255, 0, 255), 54: (255, 0, 43)}.items():
        assert tuple(w[k]) == rgb, (k, w[k])

    def lone(u, v):   # one pixel of flow (u, v): it is its own maximum
        return tuple(fv.flow_color(np.array([v, u], np.float32).reshape(1, 2, 1, 1))[0, 0, 0])
    assert lone(0.0, 0.0) == (255, 255, 255)
    assert lone(3.0, 0.0) == (255, 0, 0)         # rightward
    assert lone(-3.0, 0.0) == (0, 209, 255)      # leftward
    assert lone(0.0, 3.0) == (255, 229, 0)       # downward
    assert lone(0.0, -3.0) == (88, 0, 255)       # upward
    assert tuple(fv.flow_color(np.array([0.0, 3.0], np.float32).reshape(1, 2, 1, 1), bgr=True)[0, 0, 0]) == (0, 0, 255)
    bad = np.zeros((1, 2, 1, 2), np.float32)
    bad[0, :, 0, 0] = (1.0, 2.0)           # (v, u)
    bad[0, :, 0, 1] = (np.nan, 100.0)      # not finite: black, and no part of the maximum
    got = fv.flow_color(bad)
    assert tuple(got[0, 0, 1]) == (0, 0, 0) and fv.rad_max_of(bad)[0] == np.sqrt(5.0)
    assert tuple(got[0, 0, 0]) == tuple(fv.flow_color(bad[:, :, :, :1])[0, 0, 0])


def test_reference_colour_statement_fp32_twin():
    """The fp32 statement stays within a small fraction of the bar of the fp64 one: the bar has room for the kernel's own atan2f."""
    flow = (2.0 * np.random.default_rng(3).standard_normal((2, 2, 13, 9))).astype(np.float32)
    for rad_max in (None, 3.0):
        x64 = fv.flow_color_x(flow, rad_max)
        x32 = fv.flow_color_x(flow, rad_max, dtype=np.float32)
        clear = np.abs(x64["rad"] - 1.0) > 1e-5
        d = np.abs(x32["x"].astype(np.float64) - x64["x"])[clear].max()
        print("rad_max=%s: max |x fp32 - x fp64| = %.2e" % (rad_max, d))
        assert d <= DELTA / 10


def _lib():
    from maskflownet_amd import _lib
    _lib.build()
    return _lib.lib()


def test_frames_entries_fail_before_any_launch():
    lib = _lib()
    one = ctypes.c_void_p(16)    # never dereferenced: argument checks come first
    big = ctypes.c_size_t(1 << 20)
    F, H, W = 3, 5, 7
    # pair_mean_u8(frames, F, H, W, a0, b0, N, mean, ws, ws_bytes, stream)
    assert lib.pair_mean_u8(None, F, H, W, 0, 1, 2, one, one, big, None) == -1 and b"NULL" in lib.last_error()
    assert lib.pair_mean_u8(one, F, H, W, 0, 1, 2, None, one, big, None) == -1
    assert lib.pair_mean_u8(one, F, H, W, -1, 1, 2, one, one, big, None) == -2 and b"a0" in lib.last_error()
    assert lib.pair_mean_u8(one, F, H, W, 0, -1, 2, one, one, big, None) == -2 and b"b0" in lib.last_error()
    assert lib.pair_mean_u8(one, F, H, W, 2, 0, 2, one, one, big, None) == -2 and b"a0 + N" in lib.last_error()    # a0 + N == F + 1
    assert lib.pair_mean_u8(one, F, H, W, 0, 2, 2, one, one, big, None) == -2 and b"b0 + N" in lib.last_error()    # b0 + N == F + 1
    assert lib.pair_mean_u8(one, F, 0, W, 0, 1, 2, one, one, big, None) == -2 and b"H=" in lib.last_error()
    assert lib.pair_mean_u8(one, F, H, 0, 0, 1, 2, one, one, big, None) == -2 and b"W=" in lib.last_error()
    assert lib.pair_mean_u8(one, F, H, W, 0, 1, -1, one, one, big, None) == -2 and b"N=" in lib.last_error()
    need = lib.pair_mean_u8_workspace_bytes(2, H, W)
    assert lib.pair_mean_u8(one, F, H, W, 0, 1, 2, one, one, need - 1, None) == -5
    assert lib.pair_mean_u8(one, F, H, W, 0, 1, 2, one, None, big, None) == -5
    assert lib.pair_mean_u8(None, F, H, W, 0, 1, 0, None, None, 0, None) == 0      # N == 0: nothing to do, nothing touched
    # preprocess_pair_u8(frames, F, H, W, a0, b0, N, mean_or_null, out, Hout, Wout, stream)
    assert lib.preprocess_pair_u8(None, F, H, W, 0, 1, 2, one, one, 8, 8, None) == -1
    assert lib.preprocess_pair_u8(one, F, H, W, 0, 1, 2, None, None, 8, 8, None) == -1
    assert lib.preprocess_pair_u8(one, F, H, W, -1, 1, 2, None, one, 8, 8, None) == -2 and b"a0" in lib.last_error()
    assert lib.preprocess_pair_u8(one, F, H, W, 0, -2, 2, None, one, 8, 8, None) == -2 and b"b0" in lib.last_error()
    assert lib.preprocess_pair_u8(one, F, H, W, 2, 0, 2, None, one, 8, 8, None) == -2 and b"a0 + N" in lib.last_error()
    assert lib.preprocess_pair_u8(one, F, H, W, 0, 2, 2, None, one, 8, 8, None) == -2 and b"b0 + N" in lib.last_error()
    assert lib.preprocess_pair_u8(one, F, 0, W, 0, 1, 2, None, one, 8, 8, None) == -2
    assert lib.preprocess_pair_u8(one, F, H, 0, 0, 1, 2, None, one, 8, 8, None) == -2
    assert lib.preprocess_pair_u8(one, F, H, W, 0, 1, 2, None, one, 0, 8, None) == -2 and b"Hout" in lib.last_error()
    assert lib.preprocess_pair_u8(one, F, H, W, 0, 1, 2, None, one, 8, 0, None) == -2 and b"Wout" in lib.last_error()
    assert lib.preprocess_pair_u8(None, F, H, W, 0, 1, 0, None, None, 8, 8, None) == 0
    # flow_color(flow, rgb, N, H, W, rad_max, bgr, ws, ws_bytes, stream)
    assert lib.flow_color(None, one, 1, H, W, -1.0, 0, one, big, None) == -1
    assert lib.flow_color(one, None, 1, H, W, -1.0, 0, one, big, None) == -1
    assert lib.flow_color(one, one, -1, H, W, -1.0, 0, one, big, None) == -2
    assert lib.flow_color(one, one, 1, 0, W, -1.0, 0, one, big, None) == -2 and b"H=" in lib.last_error()
    assert lib.flow_color(one, one, 1, H, 0, 3.0, 0, one, big, None) == -2 and b"W=" in lib.last_error()
    need = lib.flow_color_workspace_bytes(1, H, W)
    assert lib.flow_color(one, one, 1, H, W, -1.0, 0, one, need - 1, None) == -5
    assert lib.flow_color(one, one, 1, H, W, 3.0, 0, None, big, None) == -5
    assert lib.flow_color(None, None, 0, H, W, -1.0, 0, None, 0, None) == 0


def test_frames_workspace_formulas():
    """pair_mean_u8: three 32-bit partial sums per pair and slice of 4096 of its 2 H W pixels; flow_color: one fp32 maximum per image and
    slice of 4096 of its H W pixels, and one per image."""
    lib = _lib()
    assert lib.pair_mean_u8_workspace_bytes(1, 52, 100) == 1 * 3 * 3 * 4       # 10400 pixels: three slices
    assert lib.pair_mean_u8_workspace_bytes(3, 1, 1) == 3 * 1 * 3 * 4
    assert lib.flow_color_workspace_bytes(1, 52, 100) == 1 * (2 + 1) * 4       # 5200 pixels: two slices
    assert lib.flow_color_workspace_bytes(3, 1, 1) == 3 * (1 + 1) * 4
    assert lib.pair_mean_u8_workspace_bytes(0, 5, 7) == 0 and lib.flow_color_workspace_bytes(1, 0, 7) == 0


def test_frames_ops_refuse_cpu_tensors():
    import torch
    from maskflownet_amd import ops
    _lib()
    frames = torch.zeros(3, 5, 7, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.pair_mean_u8(frames, 0, 1, 2)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.preprocess_pair_u8(frames, 0, 1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.flow_color(torch.zeros(1, 2, 5, 7))


def test_predict_module_has_the_frame_entries_without_a_gpu():
    import maskflownet_amd.predict as predict
    assert all(callable(getattr(predict.Predictor, m)) for m in ("do_batch_u8", "predict_frames"))
    assert callable(predict.main)
    from maskflownet_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("pair_mean_u8", "preprocess_pair_u8", "flow_color"))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def frames_a():
    """(3,13,9,3): frame 0 holds all 256 byte values (351 bytes), the rest random."""
    fr = np.random.default_rng(11).integers(0, 256, (3, 13, 9, 3), dtype=np.uint8)
    fr[0].reshape(-1)[:256] = np.random.default_rng(12).permutation(256).astype(np.uint8)
    return fr


def frames_b():
    """(3,5,7,3): a frame is 105 bytes, no multiple of 4 -- frame 1 starts at a misaligned address."""
    return np.random.default_rng(13).integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)


PAIRS = [(2, 0, 1), (1, 1, 2)]     # (N, a0, b0)


@pytest.mark.gpu
@pytest.mark.parametrize("which,out,with_mean", [("a", (4, 3), True), ("a", (8, 12), True), ("b", (5, 7), True), ("b", (5, 7), False)])
@pytest.mark.parametrize("n,a0,b0", PAIRS)
def test_preprocess_pair_u8_is_preprocess_pair_on_the_chw01_floats(which, out, with_mean, n, a0, b0):
    import torch
    from maskflownet_amd import ops
    fr = frames_a() if which == "a" else frames_b()
    dev = torch.from_numpy(fr).cuda()
    fl = torch.from_numpy(fv.chw01(fr)).cuda()
    mean = torch.from_numpy(fv.pair_mean_u8(fr, a0, b0, n)).cuda()
    im1, im2 = fl[a0:a0 + n].contiguous(), fl[b0:b0 + n].contiguous()
    if with_mean:
        want = ops.preprocess_pair(im1, im2, out[0], out[1], mean=mean)
        got = ops.preprocess_pair_u8(dev, a0, b0, n, out[0], out[1], mean=mean)
    else:     # the float operator has no form without a mean: the unpack is the floats themselves
        assert out == fr.shape[1:3]
        want = torch.cat([im1, im2])
        got = ops.preprocess_pair_u8(dev, a0, b0, n, out[0], out[1])
    assert got.shape == (2 * n, 3) + out and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert torch.equal(ops.preprocess_pair_u8(dev, a0, b0, n, out[0], out[1], mean=mean if with_mean else None), got)


def mean_cases():
    big = np.random.default_rng(14).integers(0, 256, (2, 52, 100, 3), dtype=np.uint8)     # 2 H W = 10400 pixels: three slices
    return {"a": frames_a(), "b": frames_b(), "big": big, "ones": np.full((2, 52, 100, 3), 255, np.uint8)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a", "b", "big", "ones"])
def test_pair_mean_u8_bits(which):
    import torch
    from maskflownet_amd import ops
    fr = mean_cases()[which]
    dev = torch.from_numpy(fr).cuda()
    for n, a0, b0 in (PAIRS if fr.shape[0] == 3 else [(1, 0, 1), (1, 1, 0)]):
        got = ops.pair_mean_u8(dev, a0, b0, n).cpu().numpy()
        want = fv.pair_mean_u8(fr, a0, b0, n)
        assert got.shape == (n, 3) and got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        if which == "ones":
            assert (got == 1.0).all()


def check_colours(got, flow, rad_max, bgr):
    """got (N,H,W,3) uint8 against the fp64 statement: every byte one of the two that x +- DELTA allows; under a fixed rad_max a pixel with
    |rad - 1| <= 1e-5 may have taken either branch."""
    ref = fv.flow_color_x(flow, rad_max, bgr)
    lo, hi = fv.allowed(ref["x"], DELTA)
    ok = (got == lo) | (got == hi)
    if rad_max is not None:
        near = (np.abs(ref["rad"] - 1.0) <= 1e-5)[..., None]
        assert near.mean() < 0.01, "the inputs sit on the branch: %d pixels" % near.sum()      # a statement about the reference alone
        lo2, hi2 = fv.allowed(ref["other"], DELTA)
        ok |= near & ((got == lo2) | (got == hi2))
    fin = ref["finite"][..., None]
    ok = np.where(fin, ok, got == 0)
    worst = np.abs(got.astype(np.float64) - (np.floor(ref["x"]))).max()
    print("flow_color %s rad_max=%s bgr=%s: %d of %d bytes differ from floor(x fp64), largest difference %g"
          % (flow.shape, rad_max, bgr, int((got != np.clip(np.floor(ref["x"]), 0, 255)).sum()), got.size, worst))
    assert ok.all(), "%d bytes outside {floor(x - d), floor(x + d)}" % int((~ok).sum())


def colour_flows():
    rng = np.random.default_rng(15)
    small, mid = [(2.0 * rng.standard_normal(s)).astype(np.float32) for s in ((1, 2, 5, 7), (2, 2, 13, 9))]
    big = (2.0 * rng.standard_normal((1, 2, 52, 100))).astype(np.float32)
    big[0, :, 51, 37] = (30.0, -40.0)      # the largest radius, in the last 100 pixels: the second slice of 4096
    return {"small": small, "mid": mid, "big": big}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["small", "mid", "big"])
@pytest.mark.parametrize("rad_max,bgr", [(None, False), (3.0, False), (None, True)])
def test_flow_color_against_the_fp64_statement(which, rad_max, bgr):
    import torch
    from maskflownet_amd import ops
    flow = colour_flows()[which]
    if rad_max is not None:
        share = (fv.flow_color_x(flow, rad_max)["rad"] > 1.0).mean()
        assert 0.1 < share < 0.6, share        # both branches are exercised
    dev = torch.from_numpy(flow).cuda()
    got = ops.flow_color(dev, rad_max=rad_max, bgr=bgr)
    assert got.dtype == torch.uint8 and got.shape == (flow.shape[0],) + flow.shape[2:] + (3,)
    check_colours(got.cpu().numpy(), flow, rad_max, bgr)
    assert torch.equal(ops.flow_color(dev, rad_max=rad_max, bgr=bgr), got)


@pytest.mark.gpu
def test_flow_color_zero_flow_and_a_nan_pixel():
    import torch
    from maskflownet_amd import ops
    zero = torch.zeros(1, 2, 5, 7, device="cuda")
    assert (ops.flow_color(zero) == 255).all()
    flow = colour_flows()["mid"].copy()
    flow[1, 0, 4, 3] = np.nan
    flow[0, 1, 12, 8] = np.inf
    got = ops.flow_color(torch.from_numpy(flow).cuda()).cpu().numpy()
    assert tuple(got[1, 4, 3]) == (0, 0, 0) and tuple(got[0, 12, 8]) == (0, 0, 0)
    check_colours(got, flow, None, False)      # the maxima are those of the finite pixels


# ---- the memory contract: guard bytes around every buffer, a workspace of exactly the queried size ------------------------------------
GUARD = 4096      # bytes on each side


class Banded:
    """A device buffer of `nbytes` bytes in the middle of a larger allocation; the bytes around it hold 0xA5 and are compared afterwards.
    offset: the view's address modulo 16 (the allocation itself is 256-byte aligned)."""

    def __init__(self, torch, nbytes, fill, offset=0):
        self.torch, self.n, self.off = torch, int(nbytes), int(offset)
        self.raw = torch.full((2 * GUARD + self.n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.view = self.raw[GUARD + self.off:GUARD + self.off + self.n]
        self.view.fill_(fill)

    def intact(self):
        lo, hi = self.raw[:GUARD + self.off], self.raw[GUARD + self.off + self.n:]
        return bool((lo == 0xA5).all()) and bool((hi == 0xA5).all())


def exact_ops(torch, made):
    """default_ops() with OpSet._workspace replaced: a fresh banded buffer of exactly the queried size, holding 0xFF (NaN as floats)."""
    from maskflownet_amd import ops as ops_mod

    class Exact(ops_mod.OpSet):
        def _workspace(self, like, nbytes):
            assert nbytes % 4 == 0 and nbytes > 0
            made.append(Banded(torch, nbytes, 0xFF))
            return made[-1].view.view(torch.float32)

    base = ops_mod.default_ops()
    return Exact(base.ns, base.ad, base.check)


@pytest.mark.gpu
def test_frames_ops_stay_inside_their_buffers():
    """Each op once between guard bytes, at the shapes where a vector store of 3-byte pixels or a misaligned wide load would overrun first:
    the (3,5,7,3) frames (105 bytes each) placed so that frame 0 is misaligned too, and a (1,2,5,7) flow."""
    import torch
    fr = frames_b()
    made = []
    ops = exact_ops(torch, made)
    for offset in (0, 1):
        fb = Banded(torch, fr.size, 0, offset)
        fb.view.copy_(torch.from_numpy(fr.reshape(-1)).cuda())
        frames = fb.view.view(3, 5, 7, 3)
        mean_b = Banded(torch, 2 * 3 * 4, 0xFF)
        mean = ops.pair_mean_u8(frames, 0, 1, 2, out=mean_b.view.view(torch.float32).view(2, 3))
        np.testing.assert_array_equal(mean.cpu().numpy().view(np.uint32), fv.pair_mean_u8(fr, 0, 1, 2).view(np.uint32))
        assert made[-1].n == ops.ns.pair_mean_u8_workspace_bytes(2, 5, 7)
        outs = []
        for hw in ((5, 7), (8, 12), (4, 3)):
            ob = Banded(torch, 4 * 3 * hw[0] * hw[1] * 4, 0xFF)
            out = ops.preprocess_pair_u8(frames, 0, 1, 2, hw[0], hw[1], mean=mean, out=ob.view.view(torch.float32).view(4, 3, *hw))
            assert not torch.isnan(out).any()       # every element written
            outs.append(ob)
        torch.cuda.synchronize()
        assert fb.intact() and mean_b.intact() and all(o.intact() for o in outs)
    flow = colour_flows()["small"]
    for rad_max in (None, 3.0):
        fl_b = Banded(torch, flow.size * 4, 0)
        fl_b.view.view(torch.float32).copy_(torch.from_numpy(flow.reshape(-1)).cuda())
        rgb_b = Banded(torch, 5 * 7 * 3, 0x5A)
        got = ops.flow_color(fl_b.view.view(torch.float32).view(1, 2, 5, 7), rad_max=rad_max, out=rgb_b.view.view(1, 5, 7, 3))
        check_colours(got.cpu().numpy(), flow, rad_max, False)
        assert made[-1].n == ops.ns.flow_color_workspace_bytes(1, 5, 7)
        torch.cuda.synchronize()
        assert fl_b.intact() and rgb_b.intact()
    assert all(w.intact() for w in made) and len(made) == 4
