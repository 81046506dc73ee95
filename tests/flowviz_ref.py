"""The numpy statements of kernels/frames.h, written from the specification and independently of the kernels.

[flow_vis-ext, unpinned] flow_color_x restates flow_vis.flow_to_color(flow_uv, convert_to_bgr=...) without clip_flow -- the call of the
reference's predict_new_data.py:155,:158 -- from memory; flow_vis itself is not available to these tests:

    wheel (55 rows of R,G,B; segments RY=15, YG=6, GC=4, CB=11, BM=13, MR=6, in this order)
    un = u / (rad_max + 1e-5);  vn = v / (rad_max + 1e-5);  rad = sqrt(un^2 + vn^2)
    a  = atan2(-vn, -un) / pi;  fk = (a + 1) / 2 * 54;  k0 = floor(fk);  k1 = k0 + 1, 55 -> 0;  f = fk - k0
    col = (1 - f) * wheel[k0]/255 + f * wheel[k1]/255;   col = rad <= 1 ? 1 - rad * (1 - col) : col * 0.75
    byte = floor(255 * col)   (bgr: channels reversed);  a pixel whose flow is not finite is (0, 0, 0)

in float64 (the statement the kernel is held to) or float32 (every operation rounded, as the kernel works)."""
import numpy as np

SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))


def wheel():
    """(55, 3) int: the Middlebury colour wheel."""
    rows = []
    for name, n in SEGMENTS:
        up = np.floor(255 * np.arange(n) / n).astype(np.int64)
        full, zero = np.full(n, 255, np.int64), np.zeros(n, np.int64)
        rows.append({"RY": (full, up, zero), "YG": (255 - up, full, zero), "GC": (zero, full, up),
                     "CB": (zero, 255 - up, full), "BM": (up, zero, full), "MR": (full, zero, 255 - up)}[name])
    return np.concatenate([np.stack(r, axis=1) for r in rows], axis=0)


def rad_max_of(flow, dtype=np.float64):
    """(N,) the largest finite sqrt(u*u + v*v) of each image of flow (N,2,H,W) (0 where none is finite)."""
    f = np.asarray(flow, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        rad = np.sqrt(f[:, 1] * f[:, 1] + f[:, 0] * f[:, 0])
    rad = np.where(np.isfinite(rad), rad, dtype(0))
    return rad.reshape(rad.shape[0], -1).max(axis=1).astype(dtype)


def flow_color_x(flow, rad_max=None, bgr=False, dtype=np.float64):
    """flow (N,2,H,W) fp32 in network order (channel 0 = v, channel 1 = u) -> dict(x (N,H,W,3): 255 * col before the floor, in RGB or
    BGR order; other: the same through the OTHER branch of `rad <= 1`; rad (N,H,W): the normalised radius; finite (N,H,W))."""
    T = dtype
    f = np.asarray(flow, np.float32)
    finite = np.isfinite(f).all(axis=1)
    rm = rad_max_of(f, T) if rad_max is None else np.full(f.shape[0], rad_max, T)
    den = (rm + T(1e-5)).astype(T).reshape(-1, 1, 1)
    v = np.where(finite, f[:, 0], 0).astype(T) / den
    u = np.where(finite, f[:, 1], 0).astype(T) / den
    rad = np.sqrt(u * u + v * v).astype(T)
    a = (np.arctan2(-v, -u) / T(np.pi)).astype(T)
    fk = ((a + T(1)) / T(2) * T(54)).astype(T)
    k0 = np.floor(fk).astype(np.int64)
    k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
    fr = (fk - k0.astype(T)).astype(T)[..., None]
    w = (wheel().astype(T) / T(255)).astype(T)
    col = ((T(1) - fr) * w[k0] + fr * w[k1]).astype(T)
    inside = (T(1) - rad[..., None] * (T(1) - col)).astype(T)
    outside = (col * T(0.75)).astype(T)
    le = (rad <= 1)[..., None]
    x = T(255) * np.where(le, inside, outside)
    other = T(255) * np.where(le, outside, inside)
    if bgr:
        x, other = x[..., ::-1], other[..., ::-1]
    return {"x": x.astype(T), "other": other.astype(T), "rad": rad, "finite": finite}


def flow_color(flow, rad_max=None, bgr=False, dtype=np.float64):
    """-> (N,H,W,3) uint8."""
    r = flow_color_x(flow, rad_max, bgr, dtype)
    return np.where(r["finite"][..., None], np.clip(np.floor(r["x"]), 0, 255), 0).astype(np.uint8)


def allowed(x, delta):
    """The two bytes a value x before the floor may become when it is known to +- delta."""
    return (np.clip(np.floor(x - delta), 0, 255).astype(np.int64), np.clip(np.floor(x + delta), 0, 255).astype(np.int64))


def pair_mean_u8(frames, a0, b0, n):
    """(n,3) float32: np.float32(np.float64(sum) / np.float64(255 * 2 * H * W)) over the bytes of frames[a0+k] and frames[b0+k]."""
    fr = np.asarray(frames)
    assert fr.dtype == np.uint8 and fr.ndim == 4 and fr.shape[3] == 3
    H, W = fr.shape[1:3]
    out = np.empty((n, 3), np.float32)
    for k in range(n):
        s = fr[a0 + k].astype(np.int64).sum(axis=(0, 1)) + fr[b0 + k].astype(np.int64).sum(axis=(0, 1))
        out[k] = np.float32(np.float64(s) / np.float64(255 * 2 * H * W))
    return out


def chw01(frames):
    """(F,H,W,3) uint8 -> (F,3,H,W) float32 byte / 255: predict._chw01 per frame."""
    return np.ascontiguousarray((np.asarray(frames).astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))
