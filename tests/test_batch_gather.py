"""mfn_batch_gather (kernels/batch.h): one training batch cut out of resident samples, against the numpy statement of
tests/data_ref.py, bit for bit -- uint8 as bytes, fp32 as uint32, every element.

The same cases run on the emulation (the kernel's own source on the CPU) and, marked gpu, on the product library.  Every source is a
16-byte aligned array padded to a multiple of 16 bytes (the read contract).  Every output is a view inside a larger byte buffer whose
bands carry a fixed pattern, verified after the call; the interior is pre-filled with the complement of the expected bytes, so an
element the kernel did not write differs from the expectation wherever it lies."""
import ctypes

import numpy as np
import pytest

from tests import data_ref
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
def _aligned_bytes(n, offset=0):
    """n writable bytes in host memory starting `offset` bytes behind a 16-byte boundary."""
    raw = np.zeros(n + 32, np.uint8)
    start = (-raw.ctypes.data) % 16 + offset
    return raw[start:start + n]


def _device_bytes(env, host_u8, offset=0):
    """A byte buffer holding host_u8 on env's side, its first byte `offset` bytes behind a 16-byte boundary."""
    if env.emu:
        buf = _aligned_bytes(host_u8.size, offset)
        buf[...] = host_u8
        return buf
    import torch
    full = torch.empty(host_u8.size + 16, dtype=torch.uint8, device="cuda")
    assert full.data_ptr() % 16 == 0
    buf = full[offset:offset + host_u8.size]
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

    def __init__(self, env, expected, offset=0):
        self.env, self.expected = env, np.ascontiguousarray(expected)
        want = self.expected.reshape(-1).view(np.uint8)
        host = np.full(2 * BAND + want.size, BAND_BYTE, np.uint8)
        host[BAND:BAND + want.size] = ~want
        self.buf = _device_bytes(env, host, offset)
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


def run_case(env, samples, crop, draws, with_mask=True, label_offset=0):
    """One call against data_ref; -> the four outputs' bytes.  draws: [(y0, x0, flip)]."""
    expected = data_ref.gather_batch(samples, crop, draws, with_mask)
    dev = [tuple(None if a is None else _source(env, a) for a in s) for s in samples]
    rows = env.ops.batch_gather_rows(dev, crop, [(d[0], d[1]) for d in draws], [d[2] for d in draws])
    outs = [_Out(env, e, label_offset if k == 2 else 0) if e is not None else None for k, e in enumerate(expected)]
    with env.launches() as L:
        res = env.ops.batch_gather(rows, crop, with_mask, out=[None if o is None else o.view for o in outs])
    assert L.count("batch_gather_kernel") == 1, "one call is one launch of batch_gather_kernel"
    if env.emu:
        assert L.log == ["batch_gather_kernel"], L.log
    assert (res[3] is None) == (not with_mask)
    return [None if o is None else o.check("%s of crop %s" % (n, crop)) for o, n in zip(outs, ("img1", "img2", "label", "mask"))]


def make_sample(rng, H, W, flow_dtype=np.float32, mask=True):
    img1, img2 = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
    flow = (rng.standard_normal((H, W, 2)) * 20).astype(flow_dtype)
    return img1, img2, flow, (rng.integers(0, 2, (H, W, 1), dtype=np.uint8) * 255 if mask else None)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def case_mixed(env):
    """Four slots of four sizes: crops at the origin and at the far edge of both axes with odd x0, both flips, both label types, one
    slot without a mask."""
    rng = np.random.default_rng(1)
    sizes, kinds, masks = ((9, 14), (11, 13), (7, 10), (8, 23)), (np.float32, np.float16, np.float16, np.float32), (True, True, False, True)
    samples = [make_sample(rng, h, w, k, m) for (h, w), k, m in zip(sizes, kinds, masks)]
    out = run_case(env, samples, (7, 10), [(0, 0, 0), (4, 3, 1), (0, 0, 1), (1, 13, 0)])
    assert (out[3].reshape(4, -1)[2] == 255).all()


def case_narrow(env):
    """The byte path alone: Hc * Wc odd, so every plane but the first starts off a dword boundary."""
    rng = np.random.default_rng(2)
    samples = [make_sample(rng, 5, 9, np.float32), make_sample(rng, 5, 9, np.float16)]
    for Wc in (1, 2, 3, 5):
        run_case(env, samples, (3, Wc), [(2, 9 - Wc, 1), (1, 3, 0)])


def case_wide(env):
    """Rows longer than a wave's reach, both store paths, a one-pixel tail, source offset 3 mod 4 (x0 = 37), both flips."""
    rng = np.random.default_rng(3)
    samples = [make_sample(rng, 4, 300, np.float32), make_sample(rng, 4, 300, np.float16)]
    for Wc in (260, 261):
        for flips in ((0, 1), (1, 0)):
            run_case(env, samples, (3, Wc), [(1, 37, flips[0]), (0, 37, flips[1])])


def case_uncropped(env):
    """The FlyingChairs form: the crop is the sample."""
    rng = np.random.default_rng(4)
    samples = [make_sample(rng, 8, 16, np.float32, mask=False) for _ in range(2)]
    run_case(env, samples, (8, 16), [(0, 0, 0), (0, 0, 1)], with_mask=False)


def case_no_mask_call(env):
    """A call without a mask over samples that have one: no mask output exists (NULL), nothing else changes."""
    rng = np.random.default_rng(5)
    samples = [make_sample(rng, 6, 12), make_sample(rng, 6, 12)]
    for Wc in (8, 7):
        out = run_case(env, samples, (4, Wc), [(1, 3, 1), (2, 0, 0)], with_mask=False)
        assert out[3] is None


def case_half_every_value(env):
    """Every fp16 bit pattern that is no NaN, widened exactly, plain and flipped, through both store paths."""
    bits = np.arange(1 << 16, dtype=np.uint32)
    bits = bits[((bits & 0x7C00) != 0x7C00) | ((bits & 0x3FF) == 0)].astype(np.uint16)     # NaNs left out by construction
    assert bits.size == 65536 - 2 * 1023
    flow = np.zeros(128 * 256 * 2, np.uint16)
    flow[:bits.size] = bits
    flow = flow.view(np.float16).reshape(128, 256, 2)
    assert not np.isnan(flow.astype(np.float32)).any()
    rng = np.random.default_rng(6)
    img1, img2, _, _ = make_sample(rng, 128, 256, mask=False)
    samples = [(img1, img2, flow, None)] * 2
    run_case(env, samples, (128, 256), [(0, 0, 0), (0, 0, 1)], with_mask=False)
    run_case(env, samples, (127, 255), [(1, 1, 0), (0, 0, 1)], with_mask=False)


def case_float_specials(env):
    """+-0.0, subnormals and +-inf in an fp32 label, plain and flipped: the flip changes the sign bit and nothing else."""
    rng = np.random.default_rng(7)
    img1, img2, flow, mask = make_sample(rng, 4, 8)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000], np.uint32).view(np.float32)
    flow[0, :, 0], flow[1, :, 1], flow[2, :, 0], flow[3, :, 1] = special, special, special[::-1], special[::-1]
    samples = [(img1, img2, flow, mask)] * 2
    for Wc, off in ((8, 0), (8, 4), (7, 0)):
        out = run_case(env, samples, (4, Wc), [(0, 0, 0), (0, 0, 1)], label_offset=off)
        lab = out[2].view(np.uint32).reshape(2, 2, 4, Wc)
        # the flipped slot's column x is source column Wc - 1 - x
        assert (lab[1, 0, :, ::-1] == (flow.view(np.uint32)[:, :Wc, 0] ^ 0x80000000)).all()
        assert (lab[1, 1, :, ::-1] == flow.view(np.uint32)[:, :Wc, 1]).all()


def case_paths_agree(env):
    """The same sources through the dword path (Wc = 8) and the byte path (Wc = 7): equal over the columns both hold; the dword path
    with a label tensor that is only 4-byte aligned (single-dword label stores) gives the same bytes as with a 16-byte aligned one."""
    rng = np.random.default_rng(8)
    samples = [make_sample(rng, 6, 21, np.float32), make_sample(rng, 6, 21, np.float16)]
    draws = [(1, 5, 0), (2, 13, 1)]
    wide = run_case(env, samples, (4, 8), draws)
    for off in (4, 8, 12):
        again = run_case(env, samples, (4, 8), draws, label_offset=off)
        assert all((a == b).all() for a, b in zip(wide, again))
    # seven columns from the same origin: the plain slot keeps columns 0..6, the flipped slot's column x is the wide one's x + 1
    narrow = run_case(env, samples, (4, 7), draws)
    for w, n, C, item in zip(wide, narrow, (3, 3, 2, 1), (1, 1, 4, 1)):
        w = w.reshape(2, C, 4, 8, item)
        n = n.reshape(2, C, 4, 7, item)
        assert (n[0] == w[0, :, :, :7]).all() and (n[1] == w[1, :, :, 1:]).all()


CASES = {f.__name__[5:]: f for f in (case_mixed, case_narrow, case_wide, case_uncropped, case_no_mask_call, case_half_every_value,
                                     case_float_specials, case_paths_agree)}


@pytest.mark.parametrize("name", list(CASES))
def test_emu_batch_gather(emu, name):
    CASES[name](emu)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_batch_gather(gpu, name):
    CASES[name](gpu)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _argument_errors(ns, launches):
    P = lambda *v: (ctypes.c_void_p * len(v))(*v)
    I = lambda *v: (ctypes.c_int * len(v))(*v)
    host = (ctypes.c_ulonglong * 16)()
    tag = ctypes.c_ulonglong()
    A, B = 4096, 8192        # never dereferenced: the table is built from host arrays, and the checks come before any launch

    def build(N=2, img1=P(A, B), img2=P(A, B), flow=P(A, B), mask=P(A, None), Hs=I(9, 11), Ws=I(14, 13), lt=I(0, 1), y0=I(0, 4), x0=I(1, 3),
              flip=I(0, 1), Hc=7, Wc=10, buf=ctypes.addressof(host), nbytes=128, ptag=ctypes.byref(tag)):
        return ns.batch_gather_build_rows(N, img1, img2, flow, mask, Hs, Ws, lt, y0, x0, flip, Hc, Wc, buf, nbytes, ptag)

    def gather(table=A, nbytes=128, tg=None, N=2, Hc=7, Wc=10, with_mask=1, img1=A, img2=A, label=A, mask=A):
        return ns.batch_gather(table, nbytes, tag.value if tg is None else tg, N, Hc, Wc, with_mask, img1, img2, label, mask, None)

    def refused(rc, code, text=None):
        assert rc == code, (rc, code, ns.last_error())
        assert ns.last_error(), "a refusal leaves last_error set"
        assert text is None or text in ns.last_error(), ns.last_error()

    with launches() as L:
        assert ns.batch_gather_rows_bytes(2) == 128 and ns.batch_gather_rows_bytes(0) == 0 and ns.batch_gather_rows_bytes(-3) == 0
        assert build() == 0
        first = np.frombuffer(host, np.uint64, 4, 0).tolist(), np.frombuffer(host, np.int32, 6, 32).tolist()
        assert first == ([A, A, A, A], [9, 14, 0, 1, 0, 0])
        second = np.frombuffer(host, np.uint64, 4, 64).tolist(), np.frombuffer(host, np.int32, 6, 96).tolist()
        assert second == ([B, B, B, 0], [11, 13, 4, 3, 1, 1])
        # MFN_E_NULL
        for k in ("img1", "img2", "flow", "Hs", "Ws", "lt", "y0", "x0", "flip", "buf", "ptag"):
            refused(build(**{k: None}), -1, b"NULL")
        for k in ("img1", "img2", "flow"):
            refused(build(**{k: P(A, None)}), -1, b"slot 1")
        assert build(mask=None) == 0                                        # no slot has a mask
        # MFN_E_SHAPE
        for kw in (dict(N=0), dict(N=-1), dict(Hc=0), dict(Wc=0), dict(Wc=-10), dict(Hs=I(9, 0)), dict(Ws=I(-14, 13))):
            refused(build(**kw), -2)
        for kw in (dict(y0=I(-1, 4)), dict(y0=I(3, 4)), dict(y0=I(0, 5)), dict(x0=I(-1, 3)), dict(x0=I(5, 3)), dict(x0=I(1, 4)), dict(Hc=10),
                   dict(Wc=14)):
            refused(build(**kw), -2, b"leaves")
        assert build(y0=I(2, 4), x0=I(4, 3)) == 0                           # the far edges themselves are inside
        refused(build(nbytes=127), -2, b"128 bytes needed")
        # MFN_E_ALIGN
        for k in ("img1", "img2", "flow", "mask"):
            refused(build(**{k: P(A, B + 8)}), -6, b"16-byte")
            refused(build(**{k: P(A + 4, B)}), -6, b"slot 0")
        refused(build(buf=ctypes.addressof(host) + 4), -6)
        # MFN_E_PARAM
        for kw in (dict(lt=I(0, 2)), dict(lt=I(-1, 1)), dict(flip=I(2, 0)), dict(flip=I(0, -1))):
            refused(build(**kw), -3)
        assert build() == 0
        # the launch entry
        for k in ("table", "img1", "img2", "label", "mask"):
            refused(gather(**{k: None}), -1, b"NULL")
        for kw in (dict(N=0), dict(Hc=0), dict(Wc=-1)):
            refused(gather(**kw), -2)
        refused(gather(nbytes=64), -2, b"128 bytes expected")
        refused(gather(nbytes=192), -2)
        refused(gather(tg=tag.value ^ 1), -2, b"re-run")
        refused(gather(Hc=8), -2, b"re-run")                                # the tag carries the crop the rows were checked against
        refused(gather(Wc=9), -2, b"re-run")
        refused(gather(N=1, nbytes=64), -2, b"re-run")
        for k in ("img1", "img2", "label", "mask"):
            for off in (1, 2, 3):
                refused(gather(**{k: A + off}), -6, b"4-byte")
        refused(gather(table=A + 4), -6)
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
    assert L.count("batch_gather_kernel") == 0


def test_ops_refuse_wrong_arrays_and_cpu_tensors(emu):
    import torch
    from maskflownet_amd import ops
    o = emu.ops
    rng = np.random.default_rng(9)
    img1, img2, flow, mask = (_source(emu, a) for a in make_sample(rng, 6, 8))
    with pytest.raises(TypeError, match="uint8 expected"):
        o.batch_gather_rows([(img1.astype(np.float32), img2, flow, mask)], (4, 4), [(0, 0)], [0])
    with pytest.raises(TypeError, match="float32 or float16 expected"):
        o.batch_gather_rows([(img1, img2, flow.astype(np.float64), mask)], (4, 4), [(0, 0)], [0])
    with pytest.raises(ValueError, match="expected \\(6, 8, 2\\)"):
        o.batch_gather_rows([(img1, img2, flow[:5], mask)], (4, 4), [(0, 0)], [0])
    with pytest.raises(ValueError, match="must be contiguous"):
        o.batch_gather_rows([(img1, np.asfortranarray(img2), flow, mask)], (4, 4), [(0, 0)], [0])
    with pytest.raises(ValueError, match="one origin and one flip per sample"):
        o.batch_gather_rows([(img1, img2, flow, mask)], (4, 4), [(0, 0), (1, 1)], [0])
    with pytest.raises(RuntimeError, match="leaves"):
        o.batch_gather_rows([(img1, img2, flow, mask)], (4, 4), [(3, 0)], [0])
    rows = o.batch_gather_rows([(img1, img2, flow, mask)], (4, 4), [(2, 4)], [1])
    with pytest.raises(ValueError, match="out label"):
        o.batch_gather(rows, (4, 4), True, out=[np.zeros((1, 3, 4, 4), np.uint8)] * 2 + [np.zeros((1, 2, 4, 5), np.float32), np.zeros((1, 1, 4, 4), np.uint8)])
    with pytest.raises(ValueError, match="out mask is missing"):
        o.batch_gather(rows, (4, 4), True, out=[np.zeros((1, 3, 4, 4), np.uint8)] * 2 + [np.zeros((1, 2, 4, 4), np.float32), None])
    with pytest.raises(RuntimeError, match="re-run"):
        o.batch_gather(rows, (4, 8), False)
    got = o.batch_gather(rows, (4, 4), True)         # destinations of the op's own
    want = data_ref.gather_batch([tuple(np.array(a) for a in (img1, img2, flow, mask))], (4, 4), [(2, 4, 1)], True)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g.reshape(-1).view(np.uint8) == w.reshape(-1).view(np.uint8)).all()
    t = torch.zeros(6, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.batch_gather_rows([(t, t, torch.zeros(6, 8, 2), None)], (4, 4), [(0, 0)], [0])
