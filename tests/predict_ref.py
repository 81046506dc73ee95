"""numpy statement of the operators of maskflownet_amd/csrc/kernels/predict.h (test infrastructure only).

[MXNet-ext, unpinned] contrib.BilinearResize2D of MXNet 1.5 (align_corners) as include/mfn_hip.h restates it: the positions and
the four lambdas are fp32 BY DEFINITION (`axis`), the blend runs in the dtype asked for -- float64 for the acceptance
reference, float32 for the bit-level twin of the kernel (numpy rounds every product and sum separately, as the kernel does
with fp contraction off)."""
import numpy as np


def axis(n_in, n_out):
    """(i0, ip, l0, l1) per output index, all arithmetic in fp32 exactly as the header writes it."""
    r = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    o = np.arange(n_out, dtype=np.float32)
    p = (r * o).astype(np.float32)
    i0 = p.astype(np.int32)
    ip = (i0 < n_in - 1).astype(np.int32)
    l1 = (p - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, ip, l0, l1


def axis64(n_in, n_out):
    """The same positions in fp64: NOT the operator -- what the fp32 positions are compared against."""
    r = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    p = r * np.arange(n_out, dtype=np.float64)
    i0 = np.minimum(p.astype(np.int64), n_in - 1)
    ip = (i0 < n_in - 1).astype(np.int64)
    return i0, ip, 1.0 - (p - i0), p - i0


def flow_scales(Hin, Win, Hout, Wout):
    return np.float32(float(Hout) / float(Hin)), np.float32(float(Wout) / float(Win))


def resize(x, Hout, Wout, sub=None, dtype=np.float64, flow_rescale=False, axis_fn=axis, magnitude=False):
    """x (N,C,Hin,Win) -> (N,C,Hout,Wout) in `dtype`.  sub (N,C): subtracted from every tap before the blend.  flow_rescale:
    channel 0 * Hout/Hin, channel 1 * Wout/Win (fp32 factors) after the blend.  magnitude=True returns instead
    M = sum over the four taps of |weight * (value - sub)| (* the factor), the scale of the rounding errors."""
    N, C, H, W = x.shape
    v = x.astype(dtype)
    if sub is not None:
        v = v - np.asarray(sub).astype(dtype).reshape(N, C, 1, 1)
    if (H, W) == (Hout, Wout):
        out = np.abs(v) if magnitude else v
    else:
        h0, hp, a0, a1 = axis_fn(H, Hout)
        w0, wp, b0, b1 = axis_fn(W, Wout)
        a0, a1 = a0.astype(dtype)[:, None], a1.astype(dtype)[:, None]
        b0, b1 = b0.astype(dtype), b1.astype(dtype)
        if magnitude:
            v = np.abs(v)
        top, bot = v[:, :, h0], v[:, :, h0 + hp]
        out = a0 * (b0 * top[:, :, :, w0] + b1 * top[:, :, :, w0 + wp]) + a1 * (b0 * bot[:, :, :, w0] + b1 * bot[:, :, :, w0 + wp])
    if flow_rescale:
        assert C == 2
        sy, sx = flow_scales(H, W, Hout, Wout)
        out = out * np.array([sy, sx]).astype(dtype).reshape(1, 2, 1, 1)
    return out.astype(dtype)


def pair_mean(im1, im2):
    """(mean64 (N,C), bound (N,C)): the joint mean of the pair in fp64 and 64 * 2^-24 * sum|x| / n, what a summation in which no
    term passes through more than 62 fp32 additions (plus the division) cannot miss it by."""
    a, b = im1.astype(np.float64), im2.astype(np.float64)
    n = 2 * a.shape[2] * a.shape[3]
    mean = (a.sum(axis=(2, 3)) + b.sum(axis=(2, 3))) / n
    mag = (np.abs(a).sum(axis=(2, 3)) + np.abs(b).sum(axis=(2, 3))) / n
    return mean, 64.0 * 2.0 ** -24 * mag


EPS = 1e-8


def flow_metrics(flow, label, mask):
    """fp64: dict(sums (N,3), norm_d, ratio (N,H,W)) of mfn_flow_metrics; flow / label (N,2,H,W), mask (N,1,H,W)."""
    f, l, m = flow.astype(np.float64), label.astype(np.float64), mask.astype(np.float64)[:, 0]
    d = np.sqrt(((f - l) ** 2).sum(axis=1))
    ratio = d / (np.sqrt((l ** 2).sum(axis=1)) + EPS)
    out = (d > 3.0) & (ratio > 0.05)
    sums = np.stack([(m * np.sqrt(((f - l) ** 2).sum(axis=1) + EPS)).sum(axis=(1, 2)), m.sum(axis=(1, 2)),
                     (m * out).sum(axis=(1, 2))], axis=1)
    return {"sums": sums, "norm_d": d, "ratio": ratio, "M_epe": (m * d).sum(axis=(1, 2)), "M_mask": m.sum(axis=(1, 2))}
