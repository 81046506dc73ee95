"""The operators of maskflownet_amd/csrc/kernels/validate.h: a validation batch read through the rows of a resident data set.

Each is held, bit for bit, to the operator the suite already trusts, run on the same bytes gathered into one tensor:
    val_pair_mean         == pair_mean_u8 on the images stacked as (2N,H,W,3) frames
    val_preprocess        == preprocess_pair_u8 on those frames, with the same mean or none
    val_flow_metric_sums  == flow_metric_sums on the label materialised in numpy as [..., ::-1] -> CHW fp32 (an fp16 label widens
                             exactly) and the mask as astype(float32) / float32(255)
The same cases run on the emulation (the kernels' own source on the CPU) and, marked gpu, on the product library.  The sources are
separate arrays under the read contract (16-byte aligned, padded to a multiple of 16 bytes) inside one arena, apart from each other
(the gaps hold 0xEE) and in another order than the slots, so a kernel that takes the batch for one contiguous tensor fails.  The
calls run inside tests/guarded.py's guard bands, every workspace exactly of the queried size."""
import numpy as np
import pytest

from maskflownet_amd import _abi
from maskflownet_amd.ops import BatchRows, OpSet
from tests.fp64_env import Env
from tests.guarded import guarded_env, run_guarded
from tests.test_batch_gather import _device_bytes, _typed

SHAPES = [(1, 1), (5, 7), (64, 64), (17, 241), (100, 180)]      # planes of 1, 35, 4096, 4097 and 18000 pixels: the slice is 4096
_TWINS = ("pair_mean_u8_workspace_bytes", "pair_mean_u8", "preprocess_pair_u8", "flow_metrics_workspace_bytes", "flow_metrics")


def _with_reference_entries(env):
    """The emulation compiles the whole dispatch file, the reference operators included; emu_ops binds only what the oracle has a twin
    of.  Bind the three that this file compares against, in a namespace of this file's own: the suite's shared one stays as it is."""
    import copy
    import ctypes
    import types
    env = copy.copy(env)
    ns = types.SimpleNamespace(**vars(env.ops.ns))
    for name in _TWINS:
        fn = getattr(ctypes.CDLL(ns._cdll._name), "mfn_emu_" + name)
        fn.restype, fn.argtypes = _abi.PRODUCT_ONLY[name]
        setattr(ns, name, fn)
    env.ops = OpSet(ns, env.ops.ad, env.ops.check)
    return env


@pytest.fixture(scope="module")
def emu():
    return _with_reference_entries(Env(emu=True))


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


# ---- sources ------------------------------------------------------------------------------------------------------------------------
def place(env, samples, seed):
    """The arrays of `samples` ([(img1, img2, flow, mask or None)], host) as views into one arena on env's side, each under the read
    contract, 48 to 112 bytes of 0xEE apart; the slots from the last to the first, and within a slot image 2, the mask, the flow and
    image 1 in an order that `seed` rotates.  -> the samples as device views."""
    flat = [(s, k, a) for s, smp in enumerate(samples) for k, a in enumerate(smp) if a is not None]
    within = {k: (j + seed) % 4 for j, k in enumerate((1, 3, 2, 0))}
    order = sorted(range(len(flat)), key=lambda j: (-flat[j][0], within[flat[j][1]]))
    offs, total = {}, 64
    for j in order:
        s, k, a = flat[j]
        offs[(s, k)] = total
        total += ((a.nbytes + 15) & ~15) + 48 + 16 * int(j % 5)
    host = np.full(total, 0xEE, np.uint8)
    for s, k, a in flat:
        o = offs[(s, k)]
        host[o:o + ((a.nbytes + 15) & ~15)] = 0          # the pad the contract allows a kernel to read
        host[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf = _device_bytes(env, host)
    out = []
    for s, smp in enumerate(samples):
        out.append(tuple(None if a is None else _typed(env, buf[offs[(s, k)]:offs[(s, k)] + a.nbytes], a.dtype, a.shape)
                         for k, a in enumerate(smp)))
    first = [offs[(s, 0)] for s in range(len(samples))]
    assert first == sorted(first, reverse=True)          # the slots do not follow each other in memory
    return out


def make_samples(rng, N, H, W, flow_dtype=np.float32, masks="bytes", images="random"):
    """masks: 'bytes' (drawn from {0, 1, 128, 254, 255}), 'valid' (all 255), 'mixed' (slot 1 of 3 has none: a NULL pointer)."""
    out = []
    for n in range(N):
        if images == "extremes" and n > 0:          # an all-0 and an all-255 pair
            img1 = img2 = np.full((H, W, 3), 0 if n == 1 else 255, np.uint8)
        else:
            img1, img2 = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
        flow = (rng.standard_normal((H, W, 2)) * 20).astype(flow_dtype)
        if masks == "valid":
            mask = np.full((H, W, 1), 255, np.uint8)
        elif masks == "mixed" and n == 1:
            mask = None
        else:
            mask = rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), (H, W, 1))
        out.append((img1, img2, flow, mask))
    return out


def whole_rows(ops, dev, H, W):
    return ops.batch_gather_rows(dev, (H, W), [(0, 0)] * len(dev), [0] * len(dev))


def frames_of(samples):
    """(2N,H,W,3): images 1 then images 2 -- pair n is (frames[n], frames[N + n])."""
    return np.stack([s[0] for s in samples] + [s[1] for s in samples])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def frames_on(env, fr):
    return _typed(env, _device_bytes(env, np.ascontiguousarray(fr).reshape(-1)), np.uint8, fr.shape)


# ---- the joint mean --------------------------------------------------------------------------------------------------------------------
def case_mean(env, N, H, W):
    rng = np.random.default_rng(100 + 7 * N + H)
    samples = make_samples(rng, N, H, W, images="extremes")
    g = guarded_env(env)
    dev = place(env, samples, seed=N + W)
    (got,), launches = run_guarded(g, lambda g: g.ops.val_pair_mean(whole_rows(g.ops, dev, H, W), 0, N),
                                   expect=("val_pair_mean_partial", "pair_mean_u8_final"), what="val_pair_mean")
    if env.emu:
        assert launches == ["val_pair_mean_partial", "pair_mean_u8_final"], launches
    (want,), _ = run_guarded(g, lambda g: g.ops.pair_mean_u8(frames_on(env, frames_of(samples)), 0, N, N))
    exact = np.stack([np.float32(np.float64(np.concatenate([s[0].reshape(-1, 3), s[1].reshape(-1, 3)]).sum(0, dtype=np.int64))
                                 / np.float64(255 * 2 * H * W)) for s in samples]).astype(np.float32)
    assert got.shape == (N, 3) and same_bits(got, want), (got, want)
    assert same_bits(got, exact)
    if N == 3:
        assert (got[1] == 0.0).all() and (got[2] == 1.0).all()


MEAN_CASES = [(N, H, W) for N in (1, 3) for H, W in SHAPES]


@pytest.mark.parametrize("N,H,W", MEAN_CASES)
def test_emu_val_pair_mean_is_pair_mean_u8(emu, N, H, W):
    case_mean(emu, N, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,W", MEAN_CASES)
def test_gpu_val_pair_mean_is_pair_mean_u8(gpu, N, H, W):
    case_mean(gpu, N, H, W)


# ---- the network's input batch -----------------------------------------------------------------------------------------------------------
PRE_CASES = [((5, 7), (8, 12), "val_resize_v4"),           # Wout % 4 == 0; the taps are bytes either way
             ((5, 7), (7, 9), "val_resize_v1"),            # the scalar path
             ((12, 16), (12, 16), "val_unpack_v4"),        # equal sizes: the unpack, dword loads
             ((5, 7), (5, 7), "val_unpack_v1"),            # its byte path (35 pixels)
             ((12, 16), (64, 64), "val_resize_v4"),
             ((100, 180), (128, 192), "val_resize_v4")]


def case_preprocess(env, src, dst, kernel, with_mean):
    (H, W), (Ho, Wo) = src, dst
    N = 3 if H < 100 else 2
    rng = np.random.default_rng(200 + H + Ho)
    samples = make_samples(rng, N, H, W)
    mean = rng.random((N, 3)).astype(np.float32) if with_mean else None
    g = guarded_env(env)
    dev = place(env, samples, seed=H + Wo)
    md = None if mean is None else env.dev(mean)
    (got,), launches = run_guarded(g, lambda g: g.ops.val_preprocess(whole_rows(g.ops, dev, H, W), 0, N, Ho, Wo, mean=md),
                                   expect=(kernel,), what="val_preprocess")
    if env.emu:
        assert launches == [kernel], launches
    (want,), _ = run_guarded(g, lambda g: g.ops.preprocess_pair_u8(frames_on(env, frames_of(samples)), 0, N, N, Ho, Wo, mean=md))
    assert got.shape == (2 * N, 3, Ho, Wo) and not np.isnan(got).any()
    assert np.array_equal(got, want) and same_bits(got, want)
    if (Ho, Wo) == (H, W) and mean is None:     # the unpack is the floats byte / 255 themselves
        fr = frames_of(samples)
        assert np.array_equal(got, (fr.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("with_mean", [True, False])
@pytest.mark.parametrize("src,dst,kernel", PRE_CASES)
def test_emu_val_preprocess_is_preprocess_pair_u8(emu, src, dst, kernel, with_mean):
    case_preprocess(emu, src, dst, kernel, with_mean)


@pytest.mark.gpu
@pytest.mark.parametrize("with_mean", [True, False])
@pytest.mark.parametrize("src,dst,kernel", PRE_CASES)
def test_gpu_val_preprocess_is_preprocess_pair_u8(gpu, src, dst, kernel, with_mean):
    case_preprocess(gpu, src, dst, kernel, with_mean)


# ---- the metric sums -----------------------------------------------------------------------------------------------------------------------
def materialised(samples):
    """What the host path hands flow_metric_sums: the label flipped to (dy, dx) as CHW fp32 (pipeline.py:176), the mask / 255 (:175)."""
    label = np.stack([np.ascontiguousarray(s[2].astype(np.float32)[..., ::-1].transpose(2, 0, 1)) for s in samples])
    H, W = label.shape[2:]
    mask = np.stack([np.ones((1, H, W), np.float32) if s[3] is None else
                     (s[3].astype(np.float32) / np.float32(255)).transpose(2, 0, 1) for s in samples])
    return label, np.ascontiguousarray(mask)


def flow_for(rng, label):
    """label + noise of 1 px; every 11th pixel pushed 10 px away (past the 3 px / 5 % bar wherever |label| < 200), every 7th exactly at
    the label (zero error)."""
    flow = label + rng.standard_normal(label.shape).astype(np.float32)
    flat, lab = flow.reshape(label.shape[0], 2, -1), label.reshape(label.shape[0], 2, -1)
    flat[:, :, ::7] = lab[:, :, ::7]
    flat[:, 0, 3::11] = lab[:, 0, 3::11] + np.float32(10.0)
    return flow


def case_metrics(env, H, W, flow_dtype, masks, zero_slot=None):
    N = 3
    rng = np.random.default_rng(300 + H + (flow_dtype == np.float16))
    samples = make_samples(rng, N, H, W, flow_dtype=flow_dtype, masks=masks)
    if zero_slot is not None:
        samples[zero_slot][3][...] = 0
    label, mask = materialised(samples)
    flow = flow_for(rng, label)
    g = guarded_env(env)
    dev = place(env, samples, seed=W + len(masks))
    fd = env.dev(flow)
    (got,), launches = run_guarded(g, lambda g: g.ops.val_flow_metric_sums(whole_rows(g.ops, dev, H, W), 0, N, fd),
                                   expect=("val_flow_metrics_partial", "flow_metrics_final"), what="val_flow_metric_sums")
    if env.emu:
        assert launches == ["val_flow_metrics_partial", "flow_metrics_final"], launches
    (want,), _ = run_guarded(g, lambda g: g.ops.flow_metric_sums(fd, env.dev(label), env.dev(mask)))
    assert got.shape == (N, 3) and same_bits(got, want), (got, want)
    # the cases are what they claim to be
    if H * W >= 35:
        assert (want[:, 2] > 0).all() or masks != "valid", want       # outliers counted
    if masks == "valid" or masks == "mixed":
        assert want[1, 1] == H * W                                    # all valid: the slot without a mask counts every pixel
    if zero_slot is not None:
        assert (got[zero_slot].view(np.uint32) == 0).all()            # s1 = +0.0: the division is the caller's
    return got


METRIC_CASES = [(H, W, dt, m) for H, W in SHAPES for dt in ("float32", "float16") for m in ("bytes", "valid", "mixed")]


@pytest.mark.parametrize("H,W,dt,masks", METRIC_CASES)
def test_emu_val_flow_metric_sums_is_flow_metric_sums(emu, H, W, dt, masks):
    case_metrics(emu, H, W, np.dtype(dt).type, masks)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,dt,masks", METRIC_CASES)
def test_gpu_val_flow_metric_sums_is_flow_metric_sums(gpu, H, W, dt, masks):
    case_metrics(gpu, H, W, np.dtype(dt).type, masks)


def test_emu_a_slot_whose_mask_is_all_zero(emu):
    case_metrics(emu, 17, 241, np.float16, "bytes", zero_slot=2)


@pytest.mark.gpu
def test_gpu_a_slot_whose_mask_is_all_zero(gpu):
    case_metrics(gpu, 17, 241, np.float16, "bytes", zero_slot=2)


def case_window(env):
    """A window of a longer table: rows [1, 3) of four give the results of those slots alone."""
    H, W = 5, 7
    rng = np.random.default_rng(400)
    samples = make_samples(rng, 4, H, W, masks="mixed")
    label, _ = materialised(samples)
    flow = flow_for(rng, label)
    g = guarded_env(env)
    dev = place(env, samples, seed=4)

    def both(g, first, n, smp):
        rows = whole_rows(g.ops, smp, H, W)
        return (g.ops.val_pair_mean(rows, first, n), g.ops.val_preprocess(rows, first, n, 8, 12),
                g.ops.val_flow_metric_sums(rows, first, n, env.dev(flow[1:3])))
    window, _ = run_guarded(g, lambda g: both(g, 1, 2, dev))
    alone, _ = run_guarded(g, lambda g: both(g, 0, 2, dev[1:3]))
    assert all(same_bits(a, b) for a, b in zip(window, alone))


def test_emu_a_window_of_a_longer_table(emu):
    case_window(emu)


@pytest.mark.gpu
def test_gpu_a_window_of_a_longer_table(gpu):
    case_window(gpu)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _argument_errors(ns, launches):
    A = 4096        # never dereferenced: argument checks come first
    big = 1 << 20
    N, H, W = 2, 5, 7

    def refused(rc, code, text=None):
        assert rc == code, (rc, code, ns.last_error())
        assert ns.last_error(), "a refusal leaves last_error set"
        assert text is None or text in ns.last_error(), ns.last_error()

    with launches() as L:
        # val_pair_mean(rows, N, H, W, mean, workspace, workspace_bytes, stream)
        need = ns.val_pair_mean_workspace_bytes(N, H, W)
        assert need == N * 1 * 3 * 4 and ns.val_pair_mean_workspace_bytes(1, 52, 100) == 3 * 3 * 4      # 10400 pixels: three slices
        assert ns.val_pair_mean_workspace_bytes(0, H, W) == 0 and ns.val_pair_mean_workspace_bytes(N, 0, W) == 0
        refused(ns.val_pair_mean(None, N, H, W, A, A, big, None), -1, b"NULL")
        refused(ns.val_pair_mean(A, N, H, W, None, A, big, None), -1, b"NULL")
        refused(ns.val_pair_mean(A, -1, H, W, A, A, big, None), -3, b"N=")
        refused(ns.val_pair_mean(A, N, 0, W, A, A, big, None), -3, b"H=")
        refused(ns.val_pair_mean(A, N, H, 0, A, A, big, None), -3, b"W=")
        refused(ns.val_pair_mean(A, N, H, W, A, A, need - 1, None), -5)
        refused(ns.val_pair_mean(A, N, H, W, A, None, big, None), -5)
        refused(ns.val_pair_mean(A + 4, N, H, W, A, A, big, None), -6, b"8-byte")
        refused(ns.val_pair_mean(A, N, H, W, A + 2, A, big, None), -6, b"4-byte")
        assert ns.val_pair_mean(None, 0, H, W, None, None, 0, None) == 0            # N == 0: nothing to do, nothing touched
        # val_preprocess(rows, N, H, W, mean_or_null, out, Hout, Wout, stream)
        refused(ns.val_preprocess(None, N, H, W, A, A, 8, 12, None), -1, b"NULL")
        refused(ns.val_preprocess(A, N, H, W, None, None, 8, 12, None), -1, b"NULL")
        refused(ns.val_preprocess(A, -2, H, W, None, A, 8, 12, None), -3, b"N=")
        refused(ns.val_preprocess(A, N, 0, W, None, A, 8, 12, None), -3, b"H=")
        refused(ns.val_preprocess(A, N, H, -1, None, A, 8, 12, None), -3, b"W=")
        refused(ns.val_preprocess(A, N, H, W, None, A, 0, 12, None), -3, b"Hout")
        refused(ns.val_preprocess(A, N, H, W, None, A, 8, 0, None), -3, b"Wout")
        refused(ns.val_preprocess(A, N, H, W, A + 1, A, 8, 12, None), -6)
        refused(ns.val_preprocess(A, N, H, W, None, A + 3, 8, 12, None), -6)
        assert ns.val_preprocess(None, 0, H, W, None, None, 8, 12, None) == 0
        # val_flow_metrics(rows, flow, N, H, W, sums, workspace, workspace_bytes, stream)
        need = ns.val_flow_metrics_workspace_bytes(N, H, W)
        assert need == N * 1 * 3 * 4 and ns.val_flow_metrics_workspace_bytes(1, 52, 100) == 2 * 3 * 4    # 5200 pixels: two slices
        assert ns.val_flow_metrics_workspace_bytes(-1, H, W) == 0
        refused(ns.val_flow_metrics(None, A, N, H, W, A, A, big, None), -1, b"NULL")
        refused(ns.val_flow_metrics(A, None, N, H, W, A, A, big, None), -1, b"NULL")
        refused(ns.val_flow_metrics(A, A, N, H, W, None, A, big, None), -1, b"NULL")
        refused(ns.val_flow_metrics(A, A, -1, H, W, A, A, big, None), -3, b"N=")
        refused(ns.val_flow_metrics(A, A, N, 0, W, A, A, big, None), -3, b"H=")
        refused(ns.val_flow_metrics(A, A, N, H, 0, A, A, big, None), -3, b"W=")
        refused(ns.val_flow_metrics(A, A, N, H, W, A, A, need - 1, None), -5)
        refused(ns.val_flow_metrics(A, A, N, H, W, A, None, big, None), -5)
        refused(ns.val_flow_metrics(A, A + 1, N, H, W, A, A, big, None), -6)
        assert ns.val_flow_metrics(None, None, 0, H, W, None, None, 0, None) == 0
    return L


def test_emu_argument_errors_launch_nothing(emu):
    L = _argument_errors(emu.ops.ns, emu.launches)
    assert L.log == [], L.log


def test_product_argument_errors_fail_before_any_launch():
    """The same list on the product library, without a GPU: every call returns its own (negative) code, so none reached a launch."""
    import contextlib
    from maskflownet_amd import _lib
    _lib.build()
    _argument_errors(_lib.lib(), lambda: contextlib.nullcontext())


@pytest.mark.gpu
def test_gpu_argument_errors_launch_nothing(gpu):
    L = _argument_errors(gpu.ops.ns, gpu.launches)
    assert L.count("val_") == 0 and L.count("_final") == 0


def test_rows_that_are_not_whole_samples_are_refused_before_any_launch(emu):
    """A flipped slot, a crop off the origin, a crop of another size: the host copy of the table says so, nothing is launched."""
    o = emu.ops
    rng = np.random.default_rng(500)
    dev = place(emu, make_samples(rng, 2, 6, 8), seed=5)
    flow = np.zeros((2, 2, 6, 8), np.float32)
    calls = (lambda r, n: o.val_pair_mean(r, 0, n), lambda r, n: o.val_preprocess(r, 0, n, 8, 8),
             lambda r, n: o.val_flow_metric_sums(r, 0, n, flow[:n]))
    with emu.launches() as L:
        for rows, text in ((o.batch_gather_rows(dev, (6, 8), [(0, 0), (0, 0)], [0, 1]), "row 1 .* flipped"),
                           (o.batch_gather_rows(dev, (5, 8), [(0, 0), (1, 0)], [0, 0]), "row 0 is a 5x8 crop"),
                           (o.batch_gather_rows(dev, (6, 7), [(0, 1), (0, 0)], [0, 0]), "row 0 is a 6x7 crop at \\(0, 1\\)")):
            for call in calls:
                with pytest.raises(ValueError, match=text):
                    call(rows, 2)
        good = o.batch_gather_rows(dev, (6, 8), [(0, 0), (0, 0)], [0, 1])
        assert o.val_pair_mean(good, 0, 1).shape == (1, 3)                       # the window stops in front of the flipped row
    assert L.log == ["val_pair_mean_partial", "pair_mean_u8_final"], L.log          # the one call that was not refused
    whole = o.batch_gather_rows(dev, (6, 8), [(0, 0), (0, 0)], [0, 0])
    with pytest.raises(ValueError, match="leave a table of 2"):
        o.val_pair_mean(whole, 1, 2)
    with pytest.raises(ValueError, match="flow must have shape"):
        o.val_flow_metric_sums(whole, 0, 2, flow[:, :, :5])
    with pytest.raises(ValueError, match="mean must have shape"):
        o.val_preprocess(whole, 0, 2, 8, 8, mean=np.zeros((1, 3), np.float32))
    with pytest.raises(TypeError, match="batch_gather_rows"):
        o.val_pair_mean(whole.buf, 0, 2)


def test_val_ops_refuse_cpu_tensors():
    import torch
    from maskflownet_amd import _lib, ops
    _lib.build()
    img = torch.zeros(5, 7, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.batch_gather_rows([(img, img, torch.zeros(5, 7, 2), None)], (5, 7), [(0, 0)], [0])
    rows = BatchRows(torch.zeros(16), 64, 0, 1, (5, 7), [(img, img, torch.zeros(5, 7, 2), None)], [(0, 0)], [0])
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.val_pair_mean(rows, 0, 1)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.val_preprocess(rows, 0, 1, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.val_flow_metric_sums(rows, 0, 1, torch.zeros(1, 2, 5, 7))


def test_packers_write_again_into_a_buffer_of_the_same_layout_only(emu):
    """pack_conv_weights / pack_deform_weights with out=: the same buffer, the same tag, the new weights' layout -- and a buffer laid
    out for other dims is refused."""
    o = emu.ops
    rng = np.random.default_rng(600)
    wa, wb = (rng.standard_normal((16, 16, 3, 3)).astype(np.float32) for _ in range(2))
    for pack in (lambda w, shape, out=None: o.pack_conv_weights(w, shape, kernel=(3, 3), pad=(1, 1), out=out),
                 lambda w, shape, out=None: o.pack_deform_weights(w, shape, kernel=(3, 3), pad=(1, 1), out=out)):
        pa = pack(wa, (2, 16, 8, 8))
        fresh_b = pack(wb, (2, 16, 8, 8))
        bytes_a = np.array(pa.buf).copy()
        again = pack(wb, (2, 16, 8, 8), out=pa)
        assert again.buf is pa.buf and again.tag == pa.tag == fresh_b.tag and again.dims == pa.dims
        assert np.array_equal(pa.buf.view(np.uint32), fresh_b.buf.view(np.uint32))
        assert not np.array_equal(pa.buf.view(np.uint32), bytes_a.view(np.uint32))
        with pytest.raises(ValueError, match="laid out for"):
            pack(wb, (2, 16, 8, 16), out=pa)
        with pytest.raises(TypeError, match="PackedDeformWeights"):
            pack(wb, (2, 16, 8, 8), out=pa.buf)
