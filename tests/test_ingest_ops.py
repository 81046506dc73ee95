"""mfn_ingest_minmax / mfn_ingest_image / mfn_ingest_flow_occ (kernels/ingest.h) against the numpy statement of tests/ingest_ref.py, bit
for bit -- uint8 as bytes, fp32 as uint32, fp16 as uint16, every element -- and never against the code under test.

The same cases run on the emulation (the kernels' own source on the CPU) and, marked gpu, on the product library, through the C ABI.
Every source is a 16-byte aligned array padded to a multiple of 16 bytes (the read contract).  Every output is a view inside a larger
byte buffer whose bands carry a fixed pattern, verified after the call; the interior is pre-filled with the complement of the
expected bytes, so an element the kernel did not write differs from the expectation wherever it lies (the harness of
tests/test_batch_gather.py).

The last tests compare ingest_ref's convention with torch.nn.functional.interpolate(mode="bilinear", align_corners=False), an
implementation written by somebody else; the two differ only in how they round the sampling position."""
import ctypes

import numpy as np
import pytest

from tests import ingest_ref
from tests.fp64_env import Env

BAND = 4096          # bytes on each side of an output, a multiple of 16
BAND_BYTE = 0xA5


@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
def _device_bytes(env, host_u8):
    """A 16-byte aligned byte buffer holding host_u8 on env's side."""
    if env.emu:
        raw = np.zeros(host_u8.size + 32, np.uint8)
        start = (-raw.ctypes.data) % 16
        buf = raw[start:start + host_u8.size]
        buf[...] = host_u8
        return buf
    import torch
    buf = torch.empty(host_u8.size, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.copy_(torch.from_numpy(np.ascontiguousarray(host_u8)))
    return buf


def _typed(env, buf, dtype, shape):
    if env.emu:
        return buf.view(dtype).reshape(shape)
    import torch
    return buf.view(getattr(torch, np.dtype(dtype).name)).view(shape)


def _source(env, a):
    """A source array under the read contract: 16-byte aligned, padded to a multiple of 16 bytes."""
    a = np.ascontiguousarray(a)
    padded = np.zeros((a.nbytes + 15) & ~15, np.uint8)
    padded[:a.nbytes] = a.reshape(-1).view(np.uint8)
    return _typed(env, _device_bytes(env, padded)[:a.nbytes], a.dtype, a.shape)


class _Out:
    """An output tensor as a view between two bands, pre-filled with the complement of what is expected."""

    def __init__(self, env, expected):
        self.env, self.expected = env, np.ascontiguousarray(expected)
        want = self.expected.reshape(-1).view(np.uint8)
        host = np.full(2 * BAND + want.size, BAND_BYTE, np.uint8)
        host[BAND:BAND + want.size] = ~want
        self.buf = _device_bytes(env, host)
        self.view = _typed(env, self.buf[BAND:BAND + want.size], self.expected.dtype, self.expected.shape)

    def check(self, what):
        got = self.buf if self.env.emu else self.buf.cpu().numpy()
        want = self.expected.reshape(-1).view(np.uint8)
        inner = got[BAND:BAND + want.size]
        bad = np.flatnonzero(inner != want)
        assert bad.size == 0, "%s: %d of %d bytes differ, the first at byte %d (got 0x%02x, expected 0x%02x)" % (
            what, bad.size, want.size, bad[0], inner[bad[0]], want[bad[0]])
        assert (got[:BAND] == BAND_BYTE).all(), "%s: the band before the tensor changed" % what
        assert (got[BAND + want.size:] == BAND_BYTE).all(), "%s: the band behind the tensor changed" % what
        return inner.copy()


# ---- images -------------------------------------------------------------------------------------------------------------------------
def run_image(env, src, window, dst_hw, bgr=False, stretch=False, other=None):
    """One call against ingest_ref.image (with stretch: min/max over `src` and `other` by mfn_ingest_minmax first) -> the output."""
    y0, x0, h, w = window
    what = "image %s window %s -> %s bgr=%d stretch=%d" % (src.shape[:2], window, dst_hw, bgr, stretch)
    dsrc = _source(env, src)
    lut = minmax = None
    if stretch:
        other = src if other is None else other
        want_mm = ingest_ref.minmax(src, other, window)
        mm = _Out(env, np.array(want_mm, np.int32))
        with env.launches() as L:
            minmax = env.ops.ingest_minmax(dsrc, _source(env, other), window, out=mm.view)
        assert L.count("ingest_minmax_kernel") == 1 and L.count("ingest_minmax_init_kernel") == 1
        mm.check("minmax of " + what)
        lut = ingest_ref.stretch_lut(*want_mm)
    expected = ingest_ref.image(src, window, dst_hw, bgr, lut)
    assert expected.shape == (dst_hw[0], dst_hw[1], 3) and expected.dtype == np.uint8
    out = _Out(env, expected)
    tables = env.ops.ingest_tables((h, w), dst_hw)
    with env.launches() as L:
        env.ops.ingest_image(dsrc, window, dst_hw, tables, bgr=bgr, minmax=minmax, out=out.view)
    assert L.count("ingest_image_kernel") == 1, "one call is one launch of ingest_image_kernel"
    if env.emu:
        assert L.log == ["ingest_image_kernel"], L.log
    return out.check(what).reshape(expected.shape)


def _img(rng, H, W, lo=0, hi=256):
    return rng.integers(lo, hi, (H, W, 3), dtype=np.uint8)


def case_image_window(env):
    """13x21 at (3, 5) of 17x29 -> 9x31: shrinks in y, grows in x; the 93-byte rows exercise the 16-byte stores' tails."""
    rng = np.random.default_rng(1)
    for bgr in (False, True):
        run_image(env, _img(rng, 17, 29), (3, 5, 13, 21), (9, 31), bgr=bgr)


def case_image_single_row_and_column(env):
    rng = np.random.default_rng(2)
    run_image(env, _img(rng, 1, 7), (0, 0, 1, 7), (5, 3))
    run_image(env, _img(rng, 6, 1), (0, 0, 6, 1), (4, 4))


def case_image_equal_sizes_copy(env):
    """11x19 -> 11x19 is the source bytes, with bgr the reversed ones."""
    rng = np.random.default_rng(3)
    src = _img(rng, 14, 23)
    win = (2, 3, 11, 19)
    assert (run_image(env, src, win, (11, 19)) == src[2:13, 3:22]).all()
    assert (run_image(env, src, win, (11, 19), bgr=True) == src[2:13, 3:22, ::-1]).all()


def case_image_many_blocks(env):
    """37x53 -> 70x150: 31 500 bytes, eight blocks, the last one partly idle."""
    rng = np.random.default_rng(4)
    run_image(env, _img(rng, 37, 53), (0, 0, 37, 53), (70, 150), bgr=True)


def case_image_odd_origin(env):
    """Window origins whose first byte sits at an odd address, and at 1, 2 and 3 modulo 4."""
    rng = np.random.default_rng(5)
    src = _img(rng, 17, 29)
    for y0, x0 in ((1, 2), (1, 0), (2, 1), (3, 2), (1, 1)):
        assert 3 * (y0 * 29 + x0) % 4 in (1, 2, 3)
        run_image(env, src, (y0, x0, 9, 20), (7, 27))
    assert 3 * (1 * 29 + 2) % 2 == 1


def case_image_stretch(env):
    """HD1K's lookup: a random min / max pair over two images (the extremes in different images), and the constant pair -> 0."""
    rng = np.random.default_rng(6)
    a, b = _img(rng, 37, 53, 41, 200), _img(rng, 37, 53, 41, 200)
    a[20, 30, 1], b[5, 7, 2] = 23, 231
    a[0, 0, 0] = 3                                   # outside the window: must not count
    win = (1, 2, 35, 50)
    for src, other in ((a, b), (b, a)):
        run_image(env, src, win, (20, 64), bgr=True, stretch=True, other=other)
    run_image(env, a, win, (35, 50), stretch=True, other=b)
    flat = np.full((9, 12, 3), 77, np.uint8)
    assert (run_image(env, flat, (0, 0, 9, 12), (5, 17), stretch=True) == 0).all()


# ---- flow and validity ----------------------------------------------------------------------------------------------------------------
def _flow_src(rng, H, W, valid, span=20000):
    """uint16 (H, W, 3) in file order: R, G around 32768, B = 1 with probability `valid`."""
    a = np.zeros((H, W, 3), np.uint16)
    a[..., :2] = rng.integers(32768 - span, 32768 + span, (H, W, 2))
    a[..., 2] = rng.random((H, W)) < valid
    return a


def run_flow(env, src, window, dst_hw, premultiply=False, flow_dtype=np.float32):
    y0, x0, h, w = window
    what = "flow %s window %s -> %s premultiply=%d %s" % (src.shape[:2], window, dst_hw, premultiply, np.dtype(flow_dtype).name)
    want_flow, want_mask = ingest_ref.flow_occ(src, window, dst_hw, premultiply, flow_dtype)
    assert want_flow.dtype == flow_dtype and want_flow.shape == dst_hw + (2,) and want_mask.shape == dst_hw + (1,)
    of, om = _Out(env, want_flow), _Out(env, want_mask)
    tables = env.ops.ingest_tables((h, w), dst_hw)
    with env.launches() as L:
        env.ops.ingest_flow_occ(_source(env, src), window, dst_hw, tables, premultiply=premultiply, flow_dtype=np.dtype(flow_dtype).name,
                                out_flow=of.view, out_mask=om.view)
    assert L.count("ingest_flow_occ_kernel") == 1, "one call is one launch of ingest_flow_occ_kernel"
    if env.emu:
        assert L.log == ["ingest_flow_occ_kernel"], L.log
    flow = of.check("flow of " + what).view(flow_dtype).reshape(want_flow.shape)
    return flow, om.check("mask of " + what).reshape(want_mask.shape)


def case_flow_sparse(env):
    """11x19 -> 16x24 with 30 % valid pixels: both branches of the denominator run; premultiply off and on; fp32 and fp16."""
    rng = np.random.default_rng(11)
    src = _flow_src(rng, 15, 26, 0.3)
    win = (2, 4, 11, 19)
    empty = float((ingest_ref.resize_f32((src[2:13, 4:23, 2] & 0xFF).astype(np.float32), (16, 24)) == 0).mean())
    assert 0.05 < empty < 0.5, empty          # about a fifth of the destination has occ_r == 0, the rest has not
    for pre in (False, True):
        for dt in (np.float32, np.float16):
            run_flow(env, src, win, (16, 24), pre, dt)


def case_flow_all_and_none_valid(env):
    rng = np.random.default_rng(12)
    for valid in (1.0, 0.0):
        src = _flow_src(rng, 11, 19, valid)
        for pre in (False, True):
            flow, mask = run_flow(env, src, (0, 0, 11, 19), (16, 24), pre)
            assert (mask == (255 if valid else 0)).all()
        if not valid:
            assert (flow == 0).all()          # premultiplied: 0 / 1


def case_flow_equal_sizes(env):
    """Equal sizes are the readers' resize=None branch: scale 1, division by 1, occ * 255."""
    rng = np.random.default_rng(13)
    src = _flow_src(rng, 13, 22, 0.5)
    win = (1, 2, 11, 19)
    for pre in (False, True):
        flow, mask = run_flow(env, src, win, (11, 19), pre)
        want_flow, want_mask = ingest_ref.flow_occ_unresized(src, win, pre)
        assert (flow == want_flow).all() and (mask == want_mask).all()
        run_flow(env, src, win, (11, 19), pre, np.float16)


def case_flow_extreme_words(env):
    """Raw words 0 and 65535, B values above 255 (only the low byte counts), flows that leave fp16's range (inf, as numpy's astype) and
    flows among its subnormals."""
    rng = np.random.default_rng(14)
    src = _flow_src(rng, 11, 19, 0.6)
    src[0, 0, :2], src[0, 1, :2], src[5, 9, :2], src[10, 18, :2] = 0, 65535, (0, 65535), (65535, 0)
    src[0, :2, 2], src[5, 9, 2], src[10, 18, 2] = 1, 1, 1
    src[..., 2] += (rng.integers(0, 200, (11, 19)) * 256).astype(np.uint16)       # high bytes: ignored
    assert (src[..., 2] > 255).any()
    for dt in (np.float32, np.float16):
        flow, mask = run_flow(env, src, (0, 0, 11, 19), (16, 24), False, dt)
        plain, _ = ingest_ref.flow_occ((src & np.array([0xFFFF, 0xFFFF, 0xFF], np.uint16)).astype(np.uint16), (0, 0, 11, 19), (16, 24), False, dt)
        assert (flow.view(np.uint8) == plain.view(np.uint8)).all()
    # few valid pixels, not premultiplied (KITTI): a sum of flows over a small resized validity leaves fp16's range
    sparse = _flow_src(rng, 11, 19, 0.08)
    for dt in (np.float32, np.float16):
        flow, _ = run_flow(env, sparse, (0, 0, 11, 19), (40, 56), False, dt)
    assert np.isinf(flow).any(), "the case was meant to leave fp16's range"
    # +-1/64 px everywhere: the blends that cross zero land among fp16's subnormals
    tiny = np.ones((11, 19, 3), np.uint16)
    tiny[..., :2] = 32768 + rng.choice((-1, 1), (11, 19, 2))
    small, _ = run_flow(env, tiny, (0, 0, 11, 19), (60, 80), True, np.float16)
    bits = small.view(np.uint16) & 0x7FFF
    assert ((bits > 0) & (bits < 0x0400)).any(), "the case was meant to reach fp16's subnormals"


def case_flow_many_blocks(env):
    """37x53 -> 64x40: 2 560 pixels, three blocks; and an odd pixel count (a tail of three pixels, rows that end inside a quad)."""
    rng = np.random.default_rng(15)
    src = _flow_src(rng, 37, 53, 0.4)
    for dt in (np.float32, np.float16):
        run_flow(env, src, (0, 0, 37, 53), (64, 40), False, dt)
        run_flow(env, src, (3, 5, 30, 41), (33, 37), True, dt)


CASES = {f.__name__[5:]: f for f in (case_image_window, case_image_single_row_and_column, case_image_equal_sizes_copy, case_image_many_blocks,
                                     case_image_odd_origin, case_image_stretch, case_flow_sparse, case_flow_all_and_none_valid,
                                     case_flow_equal_sizes, case_flow_extreme_words, case_flow_many_blocks)}


@pytest.mark.parametrize("name", list(CASES))
def test_emu_ingest(emu, name):
    CASES[name](emu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_ingest(gpu, name):
    CASES[name](gpu)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _argument_errors(ns, launches):
    A, B, T = 4096, 8192, 16384        # never dereferenced: the checks come before any launch
    host = (ctypes.c_ulonglong * 4 * 64)()
    tag = ctypes.c_ulonglong()

    def refused(rc, code, text=None):
        assert rc == code, (rc, code, ns.last_error())
        assert ns.last_error(), "a refusal leaves last_error set"
        assert text is None or text in ns.last_error(), ns.last_error()

    def build(sh=13, sw=21, dh=9, dw=31, buf=ctypes.addressof(host), nbytes=32 * 40, ptag=ctypes.byref(tag)):
        return ns.ingest_build_tables(sh, sw, dh, dw, buf, nbytes, ptag)

    def image(src=A, H=17, W=29, pitch=87, y0=3, x0=5, h=13, w=21, tab=T, nbytes=32 * 40, tg=None, bgr=0, mm=None, dst=B, dh=9, dw=31):
        return ns.ingest_image(src, H, W, pitch, y0, x0, h, w, tab, nbytes, tag.value if tg is None else tg, bgr, mm, dst, dh, dw, None)

    def flow(src=A, H=17, W=29, pitch=87, y0=3, x0=5, h=13, w=21, tab=T, nbytes=32 * 40, tg=None, pre=0, ft=0, fl=B, mask=B, dh=9, dw=31):
        return ns.ingest_flow_occ(src, H, W, pitch, y0, x0, h, w, tab, nbytes, tag.value if tg is None else tg, pre, ft, fl, mask, dh, dw, None)

    def minmax(a=A, b=B, H=17, W=29, pitch=87, y0=3, x0=5, h=13, w=21, out=T):
        return ns.ingest_minmax(a, b, H, W, pitch, y0, x0, h, w, out, None)

    with launches() as L:
        assert ns.ingest_tables_bytes(9, 31) == 32 * 40 and ns.ingest_tables_bytes(0, 31) == 0 and ns.ingest_tables_bytes(9, -1) == 0
        assert build() == 0
        # the first column of 21 -> 31: position (0.5 * 21 / 31 - 0.5) < 0 clamps to source 0 with coefficients (1, 0) / (2048, 0)
        assert np.frombuffer(host, np.int32, 2, 0).tolist() == [0, 1] and np.frombuffer(host, np.float32, 2, 8).tolist() == [1.0, 0.0]
        assert np.frombuffer(host, np.int32, 2, 16).tolist() == [2048, 0]
        for k in ("buf", "ptag"):
            refused(build(**{k: None}), -1, b"NULL")
        for kw in (dict(sh=0), dict(sw=-1), dict(dh=0), dict(dw=0)):
            refused(build(**kw), -2)
        refused(build(nbytes=32 * 40 - 1), -2, b"1280 bytes needed")
        refused(build(buf=ctypes.addressof(host) + 4), -6)
        assert build() == 0
        for call in (image, flow):
            # a window outside the image, on every side
            for kw in (dict(y0=-1), dict(x0=-1), dict(y0=5), dict(x0=9), dict(h=15, tg=0), dict(w=25, tg=0)):
                refused(call(**kw), -2, b"leaves")
            for kw in (dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(dh=0), dict(dw=-3)):
                refused(call(**kw), -2)
            refused(call(pitch=86), -2, b"pitch")
            refused(call(src=None), -1, b"NULL")
            refused(call(tab=None), -1, b"NULL")
            refused(call(nbytes=32 * 39), -2, b"1280 bytes expected")
            refused(call(tg=tag.value ^ 1), -2, b"re-run")
            refused(call(dh=10, nbytes=32 * 41), -2, b"re-run")          # the tag carries the sizes the tables were built for
            refused(call(h=12), -2, b"re-run")
            refused(call(src=A + 8), -6, b"16-byte")
            refused(call(tab=T + 8), -6, b"16-byte")
        refused(image(dst=None), -1, b"NULL")                             # null outputs
        refused(flow(fl=None), -1, b"NULL")
        refused(flow(mask=None), -1, b"NULL")
        refused(minmax(out=None), -1, b"NULL")
        refused(image(dst=B + 4), -6)
        refused(flow(fl=B + 4), -6)
        refused(flow(mask=B + 1), -6)
        refused(image(mm=T + 2), -6)
        refused(image(bgr=2), -3)
        refused(flow(pre=-1), -3)
        refused(flow(ft=2), -3)
        # a flow window with a side of 1: the reference's scale is x / 0
        assert ns.ingest_build_tables(1, 21, 9, 31, ctypes.addressof(host), 32 * 40, ctypes.byref(tag)) == 0
        refused(flow(h=1), -2, b"at least 2")
        assert ns.ingest_build_tables(13, 1, 9, 31, ctypes.addressof(host), 32 * 40, ctypes.byref(tag)) == 0
        refused(flow(w=1), -2, b"at least 2")
        for kw in (dict(a=None), dict(b=None)):
            refused(minmax(**kw), -1, b"NULL")
        for kw in (dict(y0=5), dict(x0=9), dict(h=0), dict(pitch=80)):
            refused(minmax(**kw), -2)
        refused(minmax(a=A + 4), -6)
        refused(ns.png_unfilter(None, 2, 5, 1), -1, b"NULL")
        refused(ns.png_unfilter(A, 2, 5, 0), -2)
        refused(ns.png_unfilter(A, -1, 5, 1), -2)
    return L


def test_emu_argument_errors_launch_nothing(emu):
    L = _argument_errors(emu.ops.ns, emu.launches)
    assert L.log == [], L.log


def test_product_argument_errors_fail_before_any_launch():
    """The same table on the product library, without a GPU: every call returns its own (negative) code, so none reached a launch."""
    import contextlib
    from maskflownet_amd import _lib
    _lib.build()
    _argument_errors(_lib.lib(), lambda: contextlib.nullcontext())


@pytest.mark.gpu
def test_gpu_argument_errors_launch_nothing(gpu):
    L = _argument_errors(gpu.ops.ns, gpu.launches)
    assert sum(L.count(k) for k in ("ingest_image_kernel", "ingest_flow_occ_kernel", "ingest_minmax_kernel", "ingest_minmax_init_kernel")) == 0


def test_ops_wrappers_allocate_and_refuse(emu):
    """The wrappers with destinations of their own, cv_resize_u8, the tables' cache, and their refusals."""
    import torch
    from maskflownet_amd import ops
    o = emu.ops
    rng = np.random.default_rng(21)
    src, fsrc = _img(rng, 12, 17), _flow_src(rng, 12, 17, 0.5)
    dsrc, dfsrc = _source(emu, src), _source(emu, fsrc)
    got = o.cv_resize_u8(dsrc, (9, 20))
    assert got.dtype == np.uint8 and (got == ingest_ref.image(src, (0, 0, 12, 17), (9, 20))).all()
    tables = o.ingest_tables((12, 17), (9, 20))
    assert o.ingest_tables((12, 17), (9, 20)) is tables and o.ingest_tables((12, 17), (9, 21)) is not tables
    for name, dt in (("float32", np.float32), ("float16", np.float16)):
        flow, mask = o.ingest_flow_occ(dfsrc, None, (9, 20), tables, flow_dtype=name)
        want_flow, want_mask = ingest_ref.flow_occ(fsrc, (0, 0, 12, 17), (9, 20), False, dt)
        assert flow.dtype == dt and (flow.view(np.uint8) == want_flow.view(np.uint8)).all() and (mask == want_mask).all()
    assert o.ingest_minmax(dsrc, dsrc).tolist() == list(ingest_ref.minmax(src, src, (0, 0, 12, 17)))
    with pytest.raises(TypeError, match="uint8 expected"):
        o.ingest_image(dfsrc, None, (9, 20), tables)
    with pytest.raises(TypeError, match="uint16 expected"):
        o.ingest_flow_occ(dsrc, None, (9, 20), tables)
    with pytest.raises(ValueError, match="expected \\(9, 20, 3\\)"):
        o.ingest_image(dsrc, None, (9, 20), tables, out=np.zeros((9, 21, 3), np.uint8))
    with pytest.raises(ValueError, match="flow_dtype"):
        o.ingest_flow_occ(dfsrc, None, (9, 20), tables, flow_dtype="float64")
    with pytest.raises(RuntimeError, match="re-run"):
        o.ingest_image(dsrc, (0, 0, 11, 17), (9, 20), tables)
    with pytest.raises(RuntimeError, match="leaves"):
        o.ingest_image(dsrc, (2, 0, 12, 17), (9, 20), tables)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.ingest_image(torch.zeros(12, 17, 3, dtype=torch.uint8), None, (9, 20), tables)


# ---- the convention against somebody else's implementation (CPU) ----------------------------------------------------------------------
SIZES = (((13, 21), (9, 31)), ((37, 53), (64, 40)), ((37, 53), (70, 150)), ((1, 7), (5, 3)), ((6, 1), (4, 4)), ((11, 19), (11, 19)))


def _interpolate(a_hwc, dst_hw):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a_hwc, dtype=np.float32)).permute(2, 0, 1)[None]
    out = torch.nn.functional.interpolate(t, size=tuple(dst_hw), mode="bilinear", align_corners=False)
    return out[0].permute(1, 2, 0).numpy().astype(np.float64)


@pytest.mark.parametrize("src_hw,dst_hw", SIZES)
def test_convention_uint8_against_torch_interpolate(src_hw, dst_hw):
    """The fixed-point path stays strictly within one grey level of torch's bilinear interpolation of the same image."""
    rng = np.random.default_rng(31)
    src = _img(rng, *src_hw)
    got = ingest_ref.image(src, (0, 0) + src_hw, dst_hw).astype(np.float64)
    worst = float(np.abs(got - _interpolate(src, dst_hw)).max())
    print("uint8 path %s -> %s: worst |delta| = %.4f grey levels" % (src_hw, dst_hw, worst))
    assert worst < 1.0, worst


@pytest.mark.parametrize("src_hw,dst_hw", SIZES)
def test_convention_float_against_torch_interpolate(src_hw, dst_hw):
    """The float path: |delta| <= 2^-20 * max(H, W, H', W') * (max - min of the source)."""
    rng = np.random.default_rng(32)
    src = (rng.standard_normal(src_hw) * 40).astype(np.float32)
    got = ingest_ref.resize_f32(src, dst_hw).astype(np.float64)
    worst = float(np.abs(got - _interpolate(src[..., None], dst_hw)[..., 0]).max())
    bound = 2.0 ** -20 * max(src_hw + dst_hw) * float(src.max() - src.min())
    print("float path %s -> %s: worst |delta| = %.3e, bound %.3e" % (src_hw, dst_hw, worst, bound))
    assert worst <= bound, (worst, bound)
    exact = ingest_ref.resize_f64(src, dst_hw)
    assert float(np.abs(got - exact).max()) <= bound
