"""The operators around the network when it predicts on images of any size (maskflownet_amd/csrc/kernels/predict.h):
align-corners bilinear resize [MXNet-ext, unpinned], pair preprocessing, the joint mean and the flow metrics.

Reference: tests/predict_ref.py, a numpy statement in fp64 (acceptance) and fp32 (the kernel's bit-level twin).
Bars: resize -- parity_cases.check_fp64_bound with M = sum over the four taps of |weight * (value - sub)|;
reductions -- 64 * 2^-24 * sum|terms|, what a summation with at most 62 additions per term (the library's has 46) and a
handful of roundings per term cannot exceed; the outlier count -- exact, on inputs asserted to stay clear of the thresholds."""
import ctypes

import numpy as np
import pytest

from tests import parity_cases as pc
from tests import predict_ref as pr

U = 2.0 ** -24


# ---- CPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,out", [((3, 5), (7, 13)), ((13, 9), (4, 3)), ((5, 7), (1, 9)), ((6, 6), (6, 11)), ((2, 2), (64, 64)),
                                    ((1, 1), (64, 64))])
def test_reference_resize_is_align_corners_bilinear(hw, out):
    import torch
    x = np.random.default_rng(0).standard_normal((2, 3) + hw).astype(np.float32)
    got = pr.resize(x, *out)
    ref = torch.nn.functional.interpolate(torch.from_numpy(x).double(), size=out, mode="bilinear", align_corners=True).numpy()
    d = np.abs(got - ref).max()
    print("%s -> %s: max |predict_ref - torch fp64| = %.2e" % (hw, out, d))
    assert d <= 1e-5


def test_positions_are_fp32_by_definition():
    """At 375x1242 -> 384x1280 the operator (fp32 positions, fp64 blend) and an fp64-position bilinear resize differ by ~3e-4 on
    N(0,1) data: (int)p and the lambdas of a few output columns land on the other side of an input sample.  The positions are
    therefore part of the semantics; no tolerance on the blend could absorb a reference that forms them in fp64."""
    import torch
    x = np.random.default_rng(0).standard_normal((2, 3, 375, 1242)).astype(np.float32)
    got = pr.resize(x, 384, 1280)
    ref = torch.nn.functional.interpolate(torch.from_numpy(x).double(), size=(384, 1280), mode="bilinear", align_corners=True).numpy()
    own64 = pr.resize(x, 384, 1280, axis_fn=pr.axis64)
    d_torch, d_own = np.abs(got - ref).max(), np.abs(got - own64).max()
    print("375x1242 -> 384x1280: fp32 vs fp64 positions: %.2e (torch fp64), %.2e (own fp64 positions)" % (d_torch, d_own))
    assert d_torch > 1e-5 and d_own > 1e-5
    assert d_torch < 1e-2 and np.abs(own64 - ref).max() <= 1e-9    # ... and it is the positions, nothing else
    i0, ip, l0, l1 = pr.axis(375, 384)
    assert (i0 + ip).max() == 374 and l1.min() >= 0.0 and l1.max() < 1.0   # fp32 positions stay inside the image


def test_size_rounding():
    from maskflownet_amd import predict
    assert [predict.round_up_64(s) for s in (436, 1024, 375, 1242, 64, 1)] == [448, 1024, 384, 1280, 64, 64]
    assert predict.network_size(436, 1024) == (448, 1024) and predict.network_size(375, 1242) == (384, 1280)
    assert predict.network_size(100, 180, resize=(256, 320)) == (256, 320)
    with pytest.raises(ValueError):
        predict.round_up_64(0)


def test_predict_module_imports_without_a_gpu():
    import maskflownet_amd.predict as predict
    assert callable(predict.Predictor) and all(hasattr(predict.Predictor, m) for m in ("do_batch", "predict", "validate"))
    from maskflownet_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("bilinear_resize", "preprocess_pair", "flow_metrics", "pair_mean"))


def test_new_ops_refuse_cpu_tensors():
    import torch
    from maskflownet_amd import ops
    x = torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.bilinear_resize(x, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.preprocess_pair(x, x, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.flow_metrics(x, x, x[:, :1])


def test_new_entries_fail_before_any_launch():
    from maskflownet_amd import _lib
    _lib.build()
    lib = _lib.lib()
    one = ctypes.c_void_p(16)   # never dereferenced: argument checks come first
    assert lib.pair_mean(None, one, one, 1, 3, 8, 8, one, 1 << 20, None) == -1 and b"NULL" in lib.last_error()
    assert lib.pair_mean(one, one, None, 1, 3, 8, 8, one, 1 << 20, None) == -1
    assert lib.pair_mean(one, one, one, 1, 3, 0, 8, one, 1 << 20, None) == -2
    assert lib.pair_mean(one, one, one, 1, 0, 8, 8, one, 1 << 20, None) == -2
    assert lib.pair_mean(one, one, one, 1, 3, 8, 8, None, 0, None) == -5          # no workspace
    assert lib.pair_mean(one, one, one, 1, 3, 436, 1024, one, 3 * 218 * 4 - 4, None) == -5 and b"workspace" in lib.last_error()
    assert lib.pair_mean_workspace_bytes(1, 3, 436, 1024) == 3 * 218 * 4         # ceil(2 * 436 * 1024 / 4096) slices per (n, c)
    assert lib.pair_mean_workspace_bytes(1, 3, 1, 1) == 3 * 4 and lib.pair_mean_workspace_bytes(0, 3, 8, 8) == 0
    assert lib.preprocess_pair(one, None, one, one, 1, 3, 8, 8, 64, 64, None) == -1
    assert lib.preprocess_pair(one, one, None, one, 1, 3, 8, 8, 64, 64, None) == -1
    assert lib.preprocess_pair(one, one, one, one, 1, 3, 8, 8, 0, 64, None) == -2
    assert lib.preprocess_pair(one, one, one, one, -1, 3, 8, 8, 64, 64, None) == -2
    assert lib.bilinear_resize_fwd(None, None, one, 1, 3, 8, 8, 4, 4, 0, None) == -1
    assert lib.bilinear_resize_fwd(one, None, None, 1, 3, 8, 8, 4, 4, 0, None) == -1
    assert lib.bilinear_resize_fwd(one, None, one, 1, 3, 8, 8, 4, 0, 0, None) == -2
    assert lib.bilinear_resize_fwd(one, None, one, 1, 3, 8, -8, 4, 4, 0, None) == -2
    assert lib.bilinear_resize_fwd(one, None, one, 1, 3, 8, 8, 4, 4, 1, None) == -2 and b"flow_rescale" in lib.last_error()
    assert lib.flow_metrics(one, one, None, one, 1, 8, 8, one, 1 << 20, None) == -1
    assert lib.flow_metrics(one, one, one, None, 1, 8, 8, one, 1 << 20, None) == -1
    assert lib.flow_metrics(one, one, one, one, 1, 8, 0, one, 1 << 20, None) == -2
    assert lib.flow_metrics(one, one, one, one, 1, 8, 8, one, 8, None) == -5
    assert lib.flow_metrics_workspace_bytes(3, 52, 100) == 3 * 2 * 3 * 4          # ceil(5200 / 4096) = 2 slices, three sums
    # an empty batch is no error and touches nothing
    assert lib.pair_mean(None, None, None, 0, 3, 8, 8, None, 0, None) == 0
    assert lib.bilinear_resize_fwd(None, None, None, 0, 3, 8, 8, 4, 4, 0, None) == 0


# ---- GPU: resize -----------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


RESIZE_CASES = [((2, 3, 3, 5), (7, 13)),        # Wout % 4 != 0: scalar stores
                ((2, 3, 13, 9), (4, 3)),        # downscale
                ((1, 2, 5, 7), (1, 9)),         # Hout = 1: r = 0
                ((1, 3, 6, 8), (6, 12)),        # identity on one axis
                ((1, 1, 1, 1), (8, 8)),
                ((1, 3, 436, 1024), (448, 1024)),   # the Sintel size ...
                ((1, 3, 448, 1024), (436, 1024))]   # ... and back: the last row has ip = 0


def _resize_input(shape, kind, seed):
    rng = np.random.default_rng(seed)
    x = pc.graded_feat(rng, shape, kind)
    sub = (0.5 * rng.standard_normal(shape[:2])).astype(np.float32)
    if kind != "plain":
        sub *= np.float32(1e-4)     # a mean of the order of the quiet regions, so that value - sub keeps their grading
    return x, sub


def _check_resize(got, x, out_hw, sub, what, flow=False):
    want64 = pr.resize(x, *out_hw, sub=sub, flow_rescale=flow)
    ref32 = pr.resize(x, *out_hw, sub=sub, dtype=np.float32, flow_rescale=flow)
    M = pr.resize(x, *out_hw, sub=sub, flow_rescale=flow, magnitude=True)
    pc.assert_magnitude_bound(M, want64, what)
    e_lib, e_ref = pc.check_fp64_bound(got, want64, ref32, M, what)
    print("%s: e_lib %.3e, e_ref32 %.3e, bit-equal to the fp32 statement: %s" % (what, e_lib, e_ref, np.array_equal(got, ref32)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "graded-pixel"])
@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("shape,out_hw", RESIZE_CASES)
def test_gpu_resize_against_fp64(shape, out_hw, with_sub, kind):
    from maskflownet_amd import ops
    x, sub = _resize_input(shape, kind, seed=shape[2] * 31 + out_hw[1])
    got = ops.bilinear_resize(_dev(x), *out_hw, sub=_dev(sub) if with_sub else None).cpu().numpy()
    assert got.shape == shape[:2] + out_hw
    _check_resize(got, x, out_hw, sub if with_sub else None, "resize %s -> %s %s sub=%s" % (shape, out_hw, kind, with_sub))


@pytest.mark.gpu
@pytest.mark.parametrize("with_sub", [False, True])
def test_gpu_resize_into_a_misaligned_view(with_sub):
    """Wout % 4 == 0 but the destination starts 4 bytes past a 16-byte boundary: scalar stores, same values, nothing around them."""
    import torch
    from maskflownet_amd import ops
    shape, out_hw = (1, 3, 6, 8), (6, 12)
    x, sub = _resize_input(shape, "plain", seed=5)
    s = _dev(sub) if with_sub else None
    n = 3 * 6 * 12
    buf = torch.full((n + 2,), 7.0, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + n].view(1, 3, 6, 12)
    assert view.data_ptr() % 16 == 4
    ops.bilinear_resize(_dev(x), *out_hw, sub=s, out=view)
    aligned = ops.bilinear_resize(_dev(x), *out_hw, sub=s)
    assert torch.equal(view, aligned) and buf[0].item() == 7.0 and buf[-1].item() == 7.0
    _check_resize(view.cpu().numpy(), x, out_hw, sub if with_sub else None, "misaligned view sub=%s" % with_sub)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 3, 6, 8)])      # plane % 4 != 0 (scalar) and == 0 (16-byte accesses)
def test_gpu_resize_to_the_same_size_is_a_copy(shape):
    from maskflownet_amd import ops
    x, sub = _resize_input(shape, "graded-pixel", seed=9)
    np.testing.assert_array_equal(ops.bilinear_resize(_dev(x), *shape[2:]).cpu().numpy(), x)
    np.testing.assert_array_equal(ops.bilinear_resize(_dev(x), *shape[2:], sub=_dev(sub)).cpu().numpy(),
                                  x - sub[:, :, None, None])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "graded-pixel"])
def test_gpu_resize_flow_mode(kind):
    """(2,2,64,128) -> (52,100): channel 0 * 52/64, channel 1 * 100/128 after the blend, one separately rounded multiply."""
    from maskflownet_amd import ops
    shape, out_hw = (2, 2, 64, 128), (52, 100)
    x, _ = _resize_input(shape, kind, seed=3)
    got = ops.bilinear_resize(_dev(x), *out_hw, flow_rescale=True).cpu().numpy()
    sy, sx = pr.flow_scales(64, 128, 52, 100)
    assert (sy, sx) == (np.float32(52 / 64), np.float32(100 / 128))
    plain32 = pr.resize(x, *out_hw, dtype=np.float32)
    np.testing.assert_array_equal(got, plain32 * np.array([sy, sx], np.float32).reshape(1, 2, 1, 1))
    _check_resize(got, x, out_hw, None, "flow mode %s" % kind, flow=True)
    with pytest.raises(ValueError, match="flow_rescale"):
        ops.bilinear_resize(_dev(np.zeros((1, 3, 4, 4), np.float32)), 8, 8, flow_rescale=True)


@pytest.mark.gpu
@pytest.mark.parametrize("hw,out_hw", [((3, 5), (7, 13)), ((13, 9), (4, 3)), ((5, 7), (1, 9)), ((6, 8), (6, 12)), ((12, 16), (11, 15))])
def test_gpu_resize_taps_are_the_references(hw, out_hw):
    """One-hot inputs, one plane per input pixel: the set of non-zero outputs is exactly the reference's -- a tap shifted by one
    sample moves that set."""
    from maskflownet_amd import ops
    H, W = hw
    x = np.eye(H * W, dtype=np.float32).reshape(H * W, 1, H, W)
    got = ops.bilinear_resize(_dev(x), *out_hw).cpu().numpy()
    ref32 = pr.resize(x, *out_hw, dtype=np.float32)
    np.testing.assert_array_equal(got != 0, ref32 != 0)
    np.testing.assert_array_equal(got, ref32)      # weights of 0/1-valued planes: the lambdas themselves


# ---- GPU: preprocess_pair ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3])
def test_gpu_preprocess_pair_is_resize_of_the_centralized_images(N):
    import torch
    from maskflownet_amd import ops
    rng = np.random.default_rng(N)
    im1, im2 = (rng.uniform(0, 1, (N, 3, 52, 100)).astype(np.float32) for _ in range(2))
    d1, d2 = _dev(im1), _dev(im2)
    mean = ops.pair_mean(d1, d2)
    out = ops.preprocess_pair(d1, d2, 64, 128, mean=mean)
    assert tuple(out.shape) == (2 * N, 3, 64, 128)
    assert torch.equal(out[:N], ops.bilinear_resize(d1, 64, 128, sub=mean))
    assert torch.equal(out[N:], ops.bilinear_resize(d2, 64, 128, sub=mean))
    assert torch.equal(ops.preprocess_pair(d1, d2, 64, 128), out)            # the default mean is pair_mean's
    _check_resize(out[N:].cpu().numpy(), im2, (64, 128), mean.cpu().numpy(), "preprocess_pair N=%d image 2" % N)
    same = ops.preprocess_pair(d1, d2, 52, 100, mean=mean)                     # no resize: exactly x - mean
    assert torch.equal(same, torch.cat([d1, d2]) - torch.cat([mean, mean])[:, :, None, None])


# ---- GPU: pair_mean ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 5, 7), (3, 3, 52, 100), (1, 3, 436, 1024)])
def test_gpu_pair_mean_bound_and_determinism(shape):
    import torch
    from maskflownet_amd import ops
    rng = np.random.default_rng(shape[2])
    im1, im2 = (rng.uniform(0, 1, shape).astype(np.float32) for _ in range(2))
    if shape[2] == 436:
        im1[:, 1] += np.float32(1e3)    # a large common offset: the image content sits in the low bits of every partial sum
        im2[:, 1] -= np.float32(1e3)    # ... and cancels between the two images
    want, bound = pr.pair_mean(im1, im2)
    d1, d2 = _dev(im1), _dev(im2)
    got = ops.pair_mean(d1, d2)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print("pair_mean %s: max err / bound = %.3f" % (shape, (err / bound).max()))
    assert (err <= bound).all(), (err, bound)
    assert torch.equal(ops.pair_mean(d1, d2), got)


@pytest.mark.gpu
def test_gpu_reductions_refuse_a_small_workspace_and_launch_nothing():
    import torch
    from maskflownet_amd import _lib
    lib = _lib.lib()
    N, C, H, W = 1, 3, 52, 100
    x = torch.rand(N, C, H, W, device="cuda:0")
    need = lib.pair_mean_workspace_bytes(N, C, H, W)
    assert need == N * C * 3 * 4
    ws = torch.full((need // 4,), 5.0, device="cuda:0")
    mean = torch.full((N, C), 5.0, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.pair_mean(x.data_ptr(), x.data_ptr(), mean.data_ptr(), N, C, H, W, ws.data_ptr(), need - 4, stream) == -5
    f = torch.rand(N, 2, H, W, device="cuda:0")
    sums = torch.full((N, 3), 5.0, device="cuda:0")
    need_m = lib.flow_metrics_workspace_bytes(N, H, W)
    assert lib.flow_metrics(f.data_ptr(), f.data_ptr(), x.data_ptr(), sums.data_ptr(), N, H, W, ws.data_ptr(), need_m - 4, stream) == -5
    torch.cuda.synchronize()
    assert (mean == 5.0).all() and (ws == 5.0).all() and (sums == 5.0).all()
    assert lib.pair_mean(x.data_ptr(), x.data_ptr(), mean.data_ptr(), N, C, H, W, ws.data_ptr(), need, stream) == 0
    torch.cuda.synchronize()
    assert torch.allclose(mean, x.mean(dim=(2, 3)), atol=1e-6)


# ---- GPU: flow_metrics ---------------------------------------------------------------------------------------------------------
# seeds for which the fp64 reference keeps every pixel clear of both thresholds (searched on the CPU; asserted below)
METRIC_SEEDS = {(2, 5, 7): 0, (3, 52, 100): 4}


def metric_inputs(N, H, W, seed):
    """Labels spanning 0.1 .. 200 px, flows = label + an error of a few px: |d| lies on both sides of 3 px and |d| / |label| on
    both sides of 0.05."""
    rng = np.random.default_rng([seed, N, H, W])
    label = (rng.standard_normal((N, 2, H, W)) * 10.0 ** rng.uniform(-1.0, 2.3, (N, 1, H, W))).astype(np.float32)
    flow = (label + 3.0 * rng.standard_normal((N, 2, H, W))).astype(np.float32)
    masks = {"ones": np.ones((N, 1, H, W), np.float32), "binary": (rng.uniform(size=(N, 1, H, W)) < 0.6).astype(np.float32)}
    masks["zero-sample"] = masks["binary"].copy()
    masks["zero-sample"][0] = 0.0
    return flow, label, masks


def metric_margins(flow, label):
    r = pr.flow_metrics(flow, label, np.ones_like(flow[:, :1]))
    return np.abs(r["norm_d"] - 3.0).min(), np.abs(r["ratio"] - 0.05).min()


@pytest.mark.parametrize("N,H,W", sorted(METRIC_SEEDS))
def test_metric_inputs_stay_clear_of_the_thresholds(N, H, W):
    flow, label, _ = metric_inputs(N, H, W, METRIC_SEEDS[(N, H, W)])
    m3, m05 = metric_margins(flow, label)
    r = pr.flow_metrics(flow, label, np.ones_like(flow[:, :1]))
    frac = r["sums"][:, 2] / r["sums"][:, 1]
    print("(%d,%d,%d): margins %.2e (3 px), %.2e (0.05); outlier fractions %s" % (N, H, W, m3, m05, frac))
    assert m3 > 1e-4 and m05 > 1e-6
    assert ((frac > 0.1) & (frac < 0.9)).all()                      # both outcomes occur in every sample
    d, ratio = r["norm_d"], r["ratio"]
    assert ((d > 3.0) & (ratio <= 0.05)).any() and ((d <= 3.0) & (ratio > 0.05)).any()    # each condition decides somewhere


@pytest.mark.gpu
@pytest.mark.parametrize("mask_kind", ["ones", "binary", "zero-sample"])
@pytest.mark.parametrize("N,H,W", sorted(METRIC_SEEDS))
def test_gpu_flow_metrics(N, H, W, mask_kind):
    import torch
    from maskflownet_amd import ops
    flow, label, masks = metric_inputs(N, H, W, METRIC_SEEDS[(N, H, W)])
    m3, m05 = metric_margins(flow, label)
    assert m3 > 1e-4 and m05 > 1e-6            # fp32 moves |d| by < 1e-6 and the ratio by < 1e-7: no pixel can change sides
    mask = masks[mask_kind]
    ref = pr.flow_metrics(flow, label, mask)
    df, dl, dm = _dev(flow), _dev(label), _dev(mask)
    sums = ops.flow_metric_sums(df, dl, dm)
    got = sums.cpu().numpy().astype(np.float64)
    e0, e1 = np.abs(got[:, 0] - ref["sums"][:, 0]), np.abs(got[:, 1] - ref["sums"][:, 1])
    print("flow_metrics (%d,%d,%d) %s: err/bound epe %s, mask %s" % (N, H, W, mask_kind, e0 / np.maximum(64 * U * ref["M_epe"], 1e-300),
                                                                    e1 / np.maximum(64 * U * ref["M_mask"], 1e-300)))
    assert (e0 <= 64 * U * ref["M_epe"]).all() and (e1 <= 64 * U * ref["M_mask"]).all()
    np.testing.assert_array_equal(got[:, 2], ref["sums"][:, 2])
    assert torch.equal(ops.flow_metric_sums(df, dl, dm), sums)
    epe, fl = ops.flow_metrics(df, dl, dm)
    epe, fl = epe.cpu().numpy(), fl.cpu().numpy()
    k = 1 if mask_kind == "zero-sample" else 0
    if k:
        assert (got[0] == 0.0).all() and np.isnan(epe[0]) and np.isnan(fl[0])
    np.testing.assert_allclose(epe[k:], ref["sums"][k:, 0] / ref["sums"][k:, 1], rtol=1e-5)
    np.testing.assert_allclose(fl[k:], ref["sums"][k:, 2] / ref["sums"][k:, 1], rtol=1e-6)
