"""The numpy statement of kernels/ingest.h, written from the specification and independently of the kernels: what the reference's
readers (reader/kitti.py:57-74, reader/hd1k.py:51-78) compute with cv2, with OpenCV's INTER_LINEAR restated from its generic path.

Tables are computed here, position in float64 rounded once to float32, fixed coefficients in int64; `taps(..., exact=True)` is the
float64 variant (position and coefficients never rounded) that the convention cross-check uses."""
import numpy as np


def taps(src, dst, exact=False):
    """-> s, s1 (int64), c0, c1 (float32, or float64 with exact), i0, i1 (int64) per destination index."""
    d = np.arange(dst, dtype=np.float64)
    pos = (d + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5
    f = pos if exact else pos.astype(np.float32)
    s = np.floor(f)
    f = f - s                                  # stays float32 (or float64)
    s = s.astype(np.int64)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    f = np.where(low | high, f.dtype.type(0), f)
    s1 = np.minimum(s + 1, src - 1)
    c0, c1 = f.dtype.type(1) - f, f
    i0 = np.rint(c0 * f.dtype.type(2048)).astype(np.int64)       # numpy's rint: half to even
    i1 = np.rint(c1 * f.dtype.type(2048)).astype(np.int64)
    return s, s1, c0, c1, i0, i1


def stretch_lut(mn, mx):
    """hd1k.py:56 per value: uint8((v - mn) * (255.0 / (mx - mn))) in float64; the constant pair maps to 0 (the one departure)."""
    lut = np.zeros(256, np.uint8)
    mn, mx = int(mn), int(mx)
    if mx > mn:
        v = np.arange(mn, mx + 1, dtype=np.uint8)
        lut[mn:mx + 1] = ((v - np.uint8(mn)).astype(np.float64) * (np.float64(255.0) / np.float64(mx - mn))).astype(np.uint8)
    return lut


def minmax(img1, img2, window):
    y0, x0, h, w = window
    a, b = img1[y0:y0 + h, x0:x0 + w], img2[y0:y0 + h, x0:x0 + w]
    return min(int(a.min()), int(b.min())), max(int(a.max()), int(b.max()))


def image(src, window, dst_hw, bgr=False, lut=None):
    """uint8 (H, W, 3) window -> uint8 (H', W', 3): reversal, lookup, OpenCV's fixed-point bilinear."""
    y0, x0, h, w = window
    Hd, Wd = dst_hw
    S = src[y0:y0 + h, x0:x0 + w]
    if bgr:
        S = S[..., ::-1]
    if lut is not None:
        S = lut[S]
    S = S.astype(np.int64)
    xs, xs1, _, _, i0, i1 = taps(w, Wd)
    ys, ys1, _, _, j0, j1 = taps(h, Hd)
    hor = S[:, xs] * i0[None, :, None] + S[:, xs1] * i1[None, :, None]          # (h, Wd, 3)
    v = ((j0[:, None, None] * (hor[ys] >> 4)) >> 16) + ((j1[:, None, None] * (hor[ys1] >> 4)) >> 16)
    return np.clip((v + 2) >> 2, 0, 255).astype(np.uint8)


def _resize_f32(a, ys, ys1, d0, d1, xs, xs1, c0, c1):
    """(h, w) float32 -> (Hd, Wd) float32, horizontal then vertical, every product and sum rounded to float32."""
    hor = (a[:, xs] * c0[None, :]).astype(np.float32) + (a[:, xs1] * c1[None, :]).astype(np.float32)
    hor = hor.astype(np.float32)
    out = (hor[ys] * d0[:, None]).astype(np.float32) + (hor[ys1] * d1[:, None]).astype(np.float32)
    return out.astype(np.float32)


def resize_f32(a, dst_hw):
    """(h, w) float32 -> (H', W') float32 with the float coefficients: the float path of cv2.resize."""
    a = np.asarray(a, np.float32)
    xs, xs1, c0, c1, _, _ = taps(a.shape[1], dst_hw[1])
    ys, ys1, d0, d1, _, _ = taps(a.shape[0], dst_hw[0])
    return _resize_f32(a, ys, ys1, d0, d1, xs, xs1, c0, c1)


def flow_occ(src_u16, window, dst_hw, premultiply=False, flow_dtype=np.float32):
    """uint16 (H, W, 3) window in file order (R = u, G = v, B = valid) -> flow (H', W', 2) (u, v), mask (H', W', 1) uint8."""
    y0, x0, h, w = window
    Hd, Wd = dst_hw
    S = src_u16[y0:y0 + h, x0:x0 + w]
    u = ((S[..., 0].astype(np.float32) - np.float32(32768)) / np.float32(64)).astype(np.float32)
    v = ((S[..., 1].astype(np.float32) - np.float32(32768)) / np.float32(64)).astype(np.float32)
    occ = (S[..., 2] & 0xFF).astype(np.float32)
    if premultiply:
        u, v = (u * occ).astype(np.float32), (v * occ).astype(np.float32)
    xs, xs1, c0, c1, _, _ = taps(w, Wd)
    ys, ys1, d0, d1, _, _ = taps(h, Hd)
    args = (ys, ys1, d0, d1, xs, xs1, c0, c1)
    ur, vr, orr = _resize_f32(u, *args), _resize_f32(v, *args), _resize_f32(occ, *args)
    sx = np.float32(Wd - 1) / np.float32(w - 1)
    sy = np.float32(Hd - 1) / np.float32(h - 1)
    ur, vr = (ur * sx).astype(np.float32), (vr * sy).astype(np.float32)
    den = (orr + (orr == 0).astype(np.float32)).astype(np.float32)
    with np.errstate(over="ignore"):
        flow = np.stack([(ur / den).astype(np.float32), (vr / den).astype(np.float32)], -1).astype(flow_dtype)
    mask = ((orr * np.float32(255)).astype(np.float32).astype(np.int64) & 0xFF).astype(np.uint8)[..., None]
    return flow, mask


def flow_occ_unresized(src_u16, window, premultiply=False):
    """The readers' resize=None branch (kitti.py:61-63, 74; hd1k.py:57-60, 78), for the equal-size case."""
    y0, x0, h, w = window
    S = src_u16[y0:y0 + h, x0:x0 + w]
    flow = (S[..., 0:2].astype(np.float32) - 32768.) / 64.
    occ = S[..., 2:3].astype(np.uint8)
    if premultiply:
        flow = flow * occ
    return flow.astype(np.float32), occ * np.uint8(255)


def resize_f64(a, dst_hw):
    """(h, w[, C]) -> (H', W'[, C]) in float64 with exact positions and coefficients: the convention itself, no rounding."""
    a = np.asarray(a, np.float64)
    h, w = a.shape[:2]
    xs, xs1, c0, c1, _, _ = taps(w, dst_hw[1], exact=True)
    ys, ys1, d0, d1, _, _ = taps(h, dst_hw[0], exact=True)
    ex = (slice(None),) + (None,) * (a.ndim - 2)
    hor = a[:, xs] * c0[(None,) + ex] + a[:, xs1] * c1[(None,) + ex]
    return hor[ys] * d0[ex + (None,)] + hor[ys1] * d1[ex + (None,)]


def window_of(shape_hw, crop):
    """(y0, x0, h, w) of the readers' crops: (h, w) = the bottom h rows and the left w columns (kitti.py:57-60);
    ((top, bottom), (left, right)) = margins (hd1k.py:51); None = everything."""
    H, W = shape_hw
    if crop is None:
        return 0, 0, H, W
    if isinstance(crop[0], (tuple, list)):
        (t, b), (l, r) = crop
        return t, l, H - t - b, W - l - r
    return H - crop[0], 0, crop[0], crop[1]


def sample(img1, img2, flow_occ_u16, crop=None, resize=None, bgr=True, premultiply=False, normalize=False, flow_dtype=np.float32):
    """What DeviceDataset.append_raw stores: (img1, img2, flow, mask)."""
    win = window_of(img1.shape[:2], crop)
    dst = (win[2], win[3]) if resize is None else (resize[1], resize[0])
    lut = stretch_lut(*minmax(img1, img2, win)) if normalize else None
    flow, mask = flow_occ(flow_occ_u16, win, dst, premultiply, flow_dtype)
    return image(img1, win, dst, bgr, lut), image(img2, win, dst, bgr, lut), flow, mask
