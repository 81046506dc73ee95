"""numpy statement of maskflownet_amd/csrc/kernels/augment.h (test infrastructure only).

Grid positions, the two grids, the taps and their weights are fp32 BY DEFINITION, formed exactly as the header writes them (as
predict_ref.axis is for the resize); the blends and everything behind them run in the dtype asked for -- float64 for the acceptance
reference, float32 for the twin of the kernel (numpy rounds every product and sum separately, as the kernels do with fp contraction
off).  magnitude=True returns M, the same expression over absolute values: the scale of the rounding errors
(parity_cases.check_fp64_bound)."""
import numpy as np

F = np.float32
U24 = 2.0 ** -24
AG_THETA1, AG_THETA2, AG_FT, AG_RT, AG_FSHIFT, AG_INV2, AG_FACTOR, AG_K = 0, 6, 12, 14, 16, 18, 22, 26
AC_M, AC_CC, AC_CHANNEL, AC_BRIGHTNESS, AC_E, AC_SPIN, AC_K = 0, 9, 12, 15, 16, 17, 26


# ---- Philox4x32-10 and the normals -------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or ints) and key words -> four uint32 arrays (Salmon et al., SC'11)."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & np.uint64(0xFFFFFFFF) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1, mask = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF, np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def noise_words(planes, npix, seed, offset):
    """The Philox blocks of `planes` (ints) for npix pixels: uint32 (len(planes), ceil(npix / 4), 4)."""
    q = np.arange((npix + 3) // 4, dtype=np.uint64)[None, :]
    pl = np.asarray(planes, np.uint64)[:, None]
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    return np.stack(philox4x32_10(q, pl, offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32), axis=-1)


def box_muller(words, dtype=np.float64, magnitude=False):
    """words (..., 4) -> normals (..., 4).  float32: the header's statement; float64: the same uniforms (exact in either format) through
    an fp64 logarithm, square root, 2 pi and sine / cosine.  magnitude: r, the radius each normal is a fraction of."""
    x = np.asarray(words, np.uint32)
    out = np.empty(x.shape, dtype)
    for h in range(2):
        a, b = (x[..., 2 * h] >> np.uint32(8)), (x[..., 2 * h + 1] >> np.uint32(8))
        if dtype == np.float32:
            u1 = (a.astype(F) + F(1)) * F(U24)
            u2 = b.astype(F) * F(U24)
            r = np.sqrt(F(-2) * np.log(u1))
            ang = F(6.2831855) * u2
        else:
            u1, u2 = (a.astype(np.float64) + 1.0) * U24, b.astype(np.float64) * U24
            r = np.sqrt(-2.0 * np.log(u1))
            ang = 2.0 * np.pi * u2
        out[..., 2 * h] = r if magnitude else r * np.cos(ang)
        out[..., 2 * h + 1] = r if magnitude else r * np.sin(ang)
    return out


def normals(planes, npix, seed, offset, dtype=np.float64, magnitude=False):
    """(len(planes), npix) normals of the given planes."""
    z = box_muller(noise_words(planes, npix, seed, offset), dtype, magnitude)
    return z.reshape(len(planes), -1)[:, :npix]


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def positions(Ht, Wt):
    """(xn (Wt,), yn (Ht,)) in fp32: -1 + i * (float)(2 / (size - 1)), product and sum rounded separately."""
    xn = F(-1) + np.arange(Wt, dtype=F) * F(2.0 / (Wt - 1))
    yn = F(-1) + np.arange(Ht, dtype=F) * F(2.0 / (Ht - 1))
    return xn.astype(F), yn.astype(F)


def grids(row, Ht, Wt):
    """The two grids of one sample in fp32: (g1x, g1y, g2x, g2y, xn, yn), each (Ht, Wt)."""
    t = np.asarray(row, F)
    xn, yn = positions(Ht, Wt)
    xn, yn = np.broadcast_to(xn[None, :], (Ht, Wt)), np.broadcast_to(yn[:, None], (Ht, Wt))
    th1, th2, ft, rt = t[AG_THETA1:], t[AG_THETA2:], t[AG_FT:], t[AG_RT:]
    clip = lambda v: np.minimum(np.maximum(v, F(-1)), F(1))
    g1x = clip(((th1[0] * xn + th1[1] * yn) + th1[2]) - ft[0])
    g1y = clip(((th1[3] * xn + th1[4] * yn) + th1[5]) - ft[1])
    g2x = (((th2[0] * xn + th2[1] * yn) + th2[2]) - ft[0]) + rt[0]
    g2y = (((th2[3] * xn + th2[4] * yn) + th2[5]) - ft[1]) + rt[1]
    assert all(a.dtype == F for a in (g1x, g1y, g2x, g2y))
    return g1x, g1y, g2x, g2y, xn, yn


def taps(gx, gy, H, W):
    """sampler_taps of warp.h in fp32: (idx (4,...) flat offsets into a plane, clamped; w (4,...) weights, 0 for taps outside)."""
    y_real = (gy + F(1)) * F(H - 1) / F(2)
    x_real = (gx + F(1)) * F(W - 1) / F(2)
    fy, fx = np.floor(y_real), np.floor(x_real)
    ty = np.minimum(np.maximum(fy, F(-2)), F(H + 1)).astype(np.int64)
    tx = np.minimum(np.maximum(fx, F(-2)), F(W + 1)).astype(np.int64)
    wy, wx = F(1) - (y_real - fy), F(1) - (x_real - fx)
    y0, y1 = (ty >= 0) & (ty <= H - 1), (ty + 1 >= 0) & (ty + 1 <= H - 1)
    x0, x1 = (tx >= 0) & (tx <= W - 1), (tx + 1 >= 0) & (tx + 1 <= W - 1)
    z = F(0)
    w = np.stack([np.where(y0 & x0, wy * wx, z), np.where(y0 & x1, wy * (F(1) - wx), z),
                  np.where(y1 & x0, (F(1) - wy) * wx, z), np.where(y1 & x1, (F(1) - wy) * (F(1) - wx), z)]).astype(F)
    cy0, cy1 = np.clip(ty, 0, H - 1), np.clip(ty + 1, 0, H - 1)
    cx0, cx1 = np.clip(tx, 0, W - 1), np.clip(tx + 1, 0, W - 1)
    idx = np.stack([cy0 * W + cx0, cy0 * W + cx1, cy1 * W + cx0, cy1 * W + cx1])
    return idx, w


def tap_values(plane, idx, w, dtype):
    """The four tap values of a (H, W) plane (or a scalar: a constant plane); a tap of weight 0 is 0."""
    plane = np.asarray(plane)
    v = plane.reshape(-1)[idx] if plane.ndim else np.broadcast_to(plane, idx.shape)
    return np.where(w != 0, v, 0).astype(dtype)


def blend(v, w, dtype, magnitude=False):
    w = w.astype(dtype)
    p = np.abs(v * w) if magnitude else v * w
    return ((p[0] + p[1]) + p[2]) + p[3]


def geometry(img1, img2, flow, mask, table, target_shape, label_order=0, dtype=np.float64, magnitude=False):
    """-> (img1', img2', flow_out, mask') of augment_geometry_kernel in `dtype`, or their magnitudes M."""
    N, _, Ho, Wo = img1.shape
    Ht, Wt = target_shape
    table = np.asarray(table, F)
    o1, o2 = np.empty((N, 3, Ht, Wt), dtype), np.empty((N, 3, Ht, Wt), dtype)
    of, om = np.empty((N, 2, Ht, Wt), dtype), np.empty((N, 1, Ht, Wt), dtype)
    for n in range(N):
        row = table[n].astype(dtype)
        g1x, g1y, g2x, g2y, xn, yn = grids(table[n], Ht, Wt)
        i1, w1 = taps(g1x, g1y, Ho, Wo)
        i2, w2 = taps(g2x, g2y, Ho, Wo)
        for c in range(3):
            o1[n, c] = blend(tap_values(img1[n, c], i1, w1, dtype), w1, dtype, magnitude)
            o2[n, c] = blend(tap_values(img2[n, c], i2, w2, dtype), w2, dtype, magnitude)
        mk = mask[n, 0] if mask.shape[2:] == (Ho, Wo) else mask[n, 0, 0, 0]
        mv = tap_values(mk, i1, w1, dtype)
        ms = blend(mv, w1, dtype)                      # the mask itself (not its magnitude) divides in either mode
        om[n, 0] = blend(mv, w1, dtype, magnitude)
        den = np.maximum(ms, dtype(1e-8) if dtype == np.float64 else F(1e-8))
        f = []
        for c in range(2):
            v = (tap_values(flow[n, c], i1, w1, dtype) - row[AG_FSHIFT + c]) * mv
            f.append(blend(v, w1, dtype, magnitude) / den)
        xg, yg = xn.astype(dtype), yn.astype(dtype)
        iv, fa = row[AG_INV2:AG_INV2 + 4], row[AG_FACTOR:AG_FACTOR + 4]
        if magnitude:
            iv, fa, xg, yg = np.abs(iv), np.abs(fa), np.abs(xg), np.abs(yg)
        ou = (iv[0] * f[0] + iv[1] * f[1]) + (fa[0] * xg + fa[1] * yg)
        ov = (iv[2] * f[0] + iv[3] * f[1]) + (fa[2] * xg + fa[3] * yg)
        of[n, 0], of[n, 1] = (ov, ou) if label_order else (ou, ov)
    assert all(a.dtype == dtype for a in (o1, o2, of, om))
    return o1, o2, of, om


def all_taps_inside(table, orig_shape, target_shape):
    """(N, Ht, Wt) bool: every tap of BOTH grids lies inside the source (no zero padding, no weight-0 tap but an exact one)."""
    Ho, Wo = orig_shape
    out = []
    for row in np.asarray(table, F):
        g1x, g1y, g2x, g2y, _, _ = grids(row, *target_shape)
        ok = np.ones(g1x.shape, bool)
        for gx, gy in ((g1x, g1y), (g2x, g2y)):
            yr, xr = (gy + F(1)) * F(Ho - 1) / F(2), (gx + F(1)) * F(Wo - 1) / F(2)
            ok &= (yr >= 0) & (yr <= Ho - 1) & (xr >= 0) & (xr <= Wo - 1)
        out.append(ok)
    return np.stack(out)


# ---- colour ------------------------------------------------------------------------------------------------------------------------
def color_a(img1, img2, table, sigma=0.0, seed=0, offset=0, dtype=np.float64, magnitude=False):
    """a = M rgb + z * sigma for both images: (2N,3,H,W) in `dtype` (the fp64 form uses the fp64 normals), or its magnitude."""
    N, _, H, W = img1.shape
    tab = np.asarray(table, F).astype(dtype)
    x = np.concatenate([img1, img2]).astype(dtype)
    sg = np.asarray(sigma, F).astype(dtype)
    out = np.empty((2 * N, 3, H, W), dtype)
    for kn in range(2 * N):
        M = tab[kn % N, AC_M:AC_M + 9].reshape(3, 3)
        if magnitude:
            M = np.abs(M)
        for i in range(3):
            out[kn, i] = (M[i, 0] * x[kn, 0] + M[i, 1] * x[kn, 1]) + M[i, 2] * x[kn, 2]
        if float(sigma) != 0.0:
            z = normals([kn * 3 + i for i in range(3)], H * W, seed, offset, dtype).reshape(3, H, W)
            out[kn] = out[kn] + (np.abs(z * sg) if magnitude else z * sg)
    assert out.dtype == dtype
    return out


def color_mean(img1, img2, table, sigma=0.0, seed=0, offset=0):
    """(mean64 (2N,3), bound (2N,3)): the means in fp64 and 64 * 2^-24 * sum|terms| / n (at most 46 additions per term, the roundings of a
    term itself and those of its normal)."""
    a = color_a(img1, img2, table, sigma, seed, offset)
    mag = color_a(img1, img2, table, sigma, seed, offset, magnitude=True)
    return a.mean(axis=(2, 3)), 64.0 * U24 * mag.mean(axis=(2, 3))


def color(img1, img2, table, sigma=0.0, seed=0, offset=0, spin=False, mean=None, dtype=np.float64, magnitude=False):
    """The colour kernel up to and including the clip (the gamma step is `gamma`): (2N,3,H,W).  mean (2N,3): given (the kernel's own,
    fp32 values), or this statement's own -- the mean of `a` in fp64, rounded to `dtype`.  The magnitude is the chain of absolute
    terms (the clip is exact and takes no part in it)."""
    N = img1.shape[0]
    tab = np.asarray(table, F).astype(dtype)
    a = color_a(img1, img2, table, sigma, seed, offset, dtype)
    if mean is None:
        mean = a.astype(np.float64).mean(axis=(2, 3))
    mean = np.asarray(mean).astype(dtype)
    if magnitude:
        a, mean, tab = color_a(img1, img2, table, sigma, seed, offset, dtype, magnitude=True), np.abs(mean), np.abs(tab)
    out = np.empty_like(a)
    for kn in range(2 * N):
        t = tab[kn % N]
        m = mean[kn][:, None, None]
        v = ((a[kn] + m) if magnitude else (a[kn] - m)) * t[AC_CC:AC_CC + 3, None, None]
        if spin:
            S = t[AC_SPIN:AC_SPIN + 9].reshape(3, 3)
            v = np.stack([(S[i, 0] * v[0] + S[i, 1] * v[1]) + S[i, 2] * v[2] for i in range(3)])
        v = v + (m * t[AC_CHANNEL:AC_CHANNEL + 3, None, None] + t[AC_BRIGHTNESS])
        out[kn] = v if magnitude else np.minimum(np.maximum(v, dtype(0)), dtype(1))
    assert out.dtype == dtype
    return out


def gamma(v, table, dtype=np.float64):
    """powf(v, e) per sample of a (2N,3,H,W) batch of clipped values; its magnitude is the fp64 value itself."""
    N = v.shape[0] // 2
    e = np.asarray(table, F)[:, AC_E].astype(dtype)
    return np.power(v.astype(dtype), np.concatenate([e, e])[:, None, None, None])


def centralize(batch):
    """pipeline.py:85-87 on a (2N,3,H,W) batch in fp64."""
    b = np.asarray(batch, np.float64)
    N = b.shape[0] // 2
    mean = (b[:N].mean(axis=(2, 3)) + b[N:].mean(axis=(2, 3))) / 2
    return b - np.concatenate([mean, mean])[:, :, None, None], mean
