"""Independent fp64 numpy statement of the hot-path operators (TEST INFRASTRUCTURE ONLY).

Written from the mathematical definitions in SURVEY.md section 8(a) -- not from the MXNet
loop nests -- and vectorised differently from oracle/mfn_ref_body.inc, so that a slip in
either restatement shows up as a disagreement (tests/test_oracle_*.py).  Small cases only.

  correlation : out[n,(dy+r)*D+(dx+r),y,x] = 1/C * sum_c f1[n,c,y,x] * f2[n,c,y+dy,x+dx]   (zero outside)
                (/root/reference/network/MaskFlownet.py:193-195, :440-441)
  warp        : out[n,c,y,x] = bilinear(x[n,c], y+flow[n,0,y,x], x+flow[n,1,y,x]), taps outside = 0,
                Smooth variant clamps the sample position to the image
                (/root/reference/network/layer.py:14-18, :26-30)
  deform conv : out[n,o,y,x] = b[o] + sum_{c,i,j} W[o,c,i,j] * S(x[n,c], y*s-p+i*d+dy_k, x*s-p+j*d+dx_k)
                S = 0 if coord < 0 or >= dim, clamp-to-last inside [dim-1, dim)
                (/root/reference/network/layer.py:117-124)
"""
import numpy as np


def correlation(f1, f2, max_displacement=4, stride2=1):
    f1 = np.asarray(f1, np.float64)
    f2 = np.asarray(f2, np.float64)
    N, C, H, W = f1.shape
    r = max_displacement // stride2
    D = 2 * r + 1
    md = r * stride2
    f2p = np.zeros((N, C, H + 2 * md, W + 2 * md))
    f2p[:, :, md:md + H, md:md + W] = f2
    out = np.zeros((N, D * D, H, W))
    for iy in range(D):
        for ix in range(D):
            dy, dx = (iy - r) * stride2, (ix - r) * stride2
            shifted = f2p[:, :, md + dy:md + dy + H, md + dx:md + dx + W]
            out[:, iy * D + ix] = (f1 * shifted).sum(axis=1) / C
    return out


def _tap(img, yy, xx):
    """img (C,H,W); integer index arrays yy,xx (H',W'); zero outside."""
    C, H, W = img.shape
    ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
    v = img[:, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
    return v * ok[None]


def warp(x, flow_yx, clip_grid=False):
    x = np.asarray(x, np.float64)
    flow = np.asarray(flow_yx, np.float64)
    N, C, H, W = x.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros_like(x)
    for n in range(N):
        py = ys + flow[n, 0]
        px = xs + flow[n, 1]
        if clip_grid:  # grid.clip(-1,1) == clamp the sample position to [0, size-1]
            py = np.clip(py, 0, H - 1)
            px = np.clip(px, 0, W - 1)
        y0 = np.floor(py).astype(np.int64)
        x0 = np.floor(px).astype(np.int64)
        ay = py - y0
        ax = px - x0
        out[n] = (_tap(x[n], y0, x0) * ((1 - ay) * (1 - ax))[None]
                  + _tap(x[n], y0, x0 + 1) * ((1 - ay) * ax)[None]
                  + _tap(x[n], y0 + 1, x0) * (ay * (1 - ax))[None]
                  + _tap(x[n], y0 + 1, x0 + 1) * (ay * ax)[None])
    return out


def _dc_sample(img, hy, wx):
    """DeformableConvolution's sampling rule on img (C,H,W) at float coords hy,wx (Ho,Wo)."""
    C, H, W = img.shape
    valid = (hy >= 0) & (wx >= 0) & (hy < H) & (wx < W)
    hl = np.floor(hy).astype(np.int64)
    wl = np.floor(wx).astype(np.int64)
    lh = hy - hl
    lw = wx - wl
    top = hl >= H - 1
    lef = wl >= W - 1
    hl = np.where(top, H - 1, hl)
    wl = np.where(lef, W - 1, wl)
    hh = np.where(top, H - 1, hl + 1)
    wh = np.where(lef, W - 1, wl + 1)
    lh = np.where(top, 0.0, lh)
    lw = np.where(lef, 0.0, lw)
    hl, hh, wl, wh = (np.clip(a, 0, b) for a, b in ((hl, H - 1), (hh, H - 1), (wl, W - 1), (wh, W - 1)))
    v = ((1 - lh) * (1 - lw))[None] * img[:, hl, wl] + ((1 - lh) * lw)[None] * img[:, hl, wh] \
        + (lh * (1 - lw))[None] * img[:, hh, wl] + (lh * lw)[None] * img[:, hh, wh]
    return v * valid[None]


def deformable_convolution(x, offset, weight, bias=None, kernel=(3, 3), stride=(1, 1), dilate=(1, 1),
                           pad=(1, 1), num_group=1, num_deformable_group=1):
    x = np.asarray(x, np.float64)
    offset = np.asarray(offset, np.float64)
    weight = np.asarray(weight, np.float64)
    N, Cin, H, W = x.shape
    Cout = weight.shape[0]
    kh, kw = kernel
    sh, sw = stride
    dh, dw = dilate
    ph, pw = pad
    Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    ys, xs = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    cpg = Cin // num_group
    opg = Cout // num_group
    cpd = Cin // num_deformable_group
    out = np.zeros((N, Cout, Ho, Wo))
    for n in range(N):
        col = np.zeros((Cin, kh, kw, Ho, Wo))
        for dg in range(num_deformable_group):
            for i in range(kh):
                for j in range(kw):
                    k = i * kw + j
                    oy = offset[n, dg * 2 * kh * kw + 2 * k]
                    ox = offset[n, dg * 2 * kh * kw + 2 * k + 1]
                    hy = ys * sh - ph + i * dh + oy
                    wx = xs * sw - pw + j * dw + ox
                    col[dg * cpd:(dg + 1) * cpd, i, j] = _dc_sample(x[n, dg * cpd:(dg + 1) * cpd], hy, wx)
        for g in range(num_group):
            wg = weight[g * opg:(g + 1) * opg].reshape(opg, cpg * kh * kw)
            cg = col[g * cpg:(g + 1) * cpg].reshape(cpg * kh * kw, Ho * Wo)
            out[n, g * opg:(g + 1) * opg] = (wg @ cg).reshape(opg, Ho, Wo)
        if bias is not None:
            out[n] += np.asarray(bias, np.float64)[:, None, None]
    return out


def offsets_from_flow(flow_yx, scale, stride, taps=9):
    f = np.asarray(flow_yx, np.float64) * scale / stride
    return np.tile(f, (1, taps, 1, 1))


def upsample(img, factor):
    """out[f*i+a] interpolates linearly between in[i] and in[i+1] (edge replicated)."""
    img = np.asarray(img, np.float64)
    N, C, H, W = img.shape
    f = factor
    p = np.pad(img, ((0, 0), (0, 0), (0, 1), (0, 1)), mode="edge")
    out = np.zeros((N, C, H * f, W * f))
    for a in range(f):
        for b in range(f):
            wy, wx = a / f, b / f
            out[:, :, a::f, b::f] = ((1 - wy) * (1 - wx) * p[:, :, :H, :W] + (1 - wy) * wx * p[:, :, :H, 1:W + 1]
                                     + wy * (1 - wx) * p[:, :, 1:H + 1, :W] + wy * wx * p[:, :, 1:H + 1, 1:W + 1])
    return out


# ---- magnitude bounds of the backward pass ---------------------------------------------------------------------------------
# M: per gradient element, the sum of the absolute values of the terms that element is made of (the C oracle's terms, under its
# border rules).  |exact - computed| <= (terms) * eps * M for any summation order, so |got - want64| / M is the error a kernel
# makes per element, whatever that element's own magnitude.  A bilinear derivative (b - a) * coef is taken as |coef||a| + |coef||b|.
def correlation_backward_bound(gout, f1, f2, max_displacement=4):
    """M of CorrelationBackward (kernel 1, strides 1, pad = md, multiply): (M1, M2) for (g1, g2)."""
    ga = np.abs(np.asarray(gout, np.float64))
    a1 = np.abs(np.asarray(f1, np.float64))
    a2 = np.abs(np.asarray(f2, np.float64))
    N, C, H, W = a1.shape
    md = max_displacement
    D = 2 * md + 1
    a2p = np.zeros((N, C, H + 2 * md, W + 2 * md))
    a2p[:, :, md:md + H, md:md + W] = a2
    m1 = np.zeros((N, C, H, W))
    m2p = np.zeros((N, C, H + 2 * md, W + 2 * md))
    for iy in range(D):
        for ix in range(D):
            g = ga[:, iy * D + ix][:, None]
            m1 += g * a2p[:, :, iy:iy + H, ix:ix + W]
            m2p[:, :, iy:iy + H, ix:ix + W] += g * a1
    return m1 / C, m2p[:, :, md:md + H, md:md + W] / C


def _dc_corners(hy, wx, H, W):
    """The C oracle's sampling rule at (hy, wx): valid mask, clamped corner rows / columns, fractions (0 where clamped)."""
    valid = (hy >= 0) & (wx >= 0) & (hy < H) & (wx < W)
    hs = np.where(valid, hy, 0.0)
    ws = np.where(valid, wx, 0.0)
    hl = np.floor(hs).astype(np.int64)
    wl = np.floor(ws).astype(np.int64)
    top, lef = hl >= H - 1, wl >= W - 1
    hl, wl = np.where(top, H - 1, hl), np.where(lef, W - 1, wl)
    hh, wh = np.where(top, H - 1, hl + 1), np.where(lef, W - 1, wl + 1)
    lh, lw = np.where(top, 0.0, hs - hl), np.where(lef, 0.0, ws - wl)
    return valid, hl, hh, wl, wh, lh, lw


def deformable_convolution_backward_bound(gout, x, offset, weight, kernel=(3, 3), pad=(1, 1)):
    """M of DeformableConvolution's backward (stride 1, dilation 1, one group, one deformable group): (Mgx, Mgoffset, Mgw, Mgbias).
    Column gradient M: |W|^T |gout|; gx: its scatter with the bilinear weights; goffset: times the derivative's corner terms;
    gw: |gout| . columns of |x|; gbias: sum |gout|."""
    import scipy.sparse as sp
    ga = np.abs(np.asarray(gout, np.float64))
    xa = np.abs(np.asarray(x, np.float64))
    off = np.asarray(offset, np.float64)
    wa = np.abs(np.asarray(weight, np.float64))
    N, Cin, H, W = xa.shape
    Cout = wa.shape[0]
    kh, kw = kernel
    ph, pw = pad
    K = kh * kw
    Ho, Wo = H + 2 * ph - kh + 1, W + 2 * pw - kw + 1
    P = Ho * Wo
    assert wa.shape == (Cout, Cin, kh, kw) and off.shape == (N, 2 * K, Ho, Wo) and ga.shape == (N, Cout, Ho, Wo)
    ys, xs = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    wt = wa.reshape(Cout, Cin * K).T                                   # (Cin*K, Cout)
    mgx = np.zeros((N, Cin, H * W))
    mgoff = np.zeros((N, 2 * K, P))
    mgw = np.zeros((Cin, K, Cout))
    for n in range(N):
        g = ga[n].reshape(Cout, P)
        mcol = (wt @ g).reshape(Cin, K, P)
        xn = xa[n].reshape(Cin, H * W)
        rows, cols, vals = [], [], []
        for k in range(K):
            i, j = divmod(k, kw)
            hy = (ys - ph + i + off[n, 2 * k]).ravel()
            wx = (xs - pw + j + off[n, 2 * k + 1]).ravel()
            valid, hl, hh, wl, wh, lh, lw = _dc_corners(hy, wx, H, W)
            v = valid.astype(np.float64)
            a, b, c, d = xn[:, hl * W + wl], xn[:, hl * W + wh], xn[:, hh * W + wl], xn[:, hh * W + wh]
            cw = ((1 - lh) * (1 - lw) * v, (1 - lh) * lw * v, lh * (1 - lw) * v, lh * lw * v)
            colabs = cw[0] * a + cw[1] * b + cw[2] * c + cw[3] * d        # (Cin, P): columns of |x|
            mgw[:, k] += colabs @ g.T
            dh = ((1 - lw) * (a + c) + lw * (b + d)) * v                 # d/dh: (1-lw)(c - a) + lw (d - b)
            dw = ((1 - lh) * (a + b) + lh * (c + d)) * v                 # d/dw: (1-lh)(b - a) + lh (d - c)
            mgoff[n, 2 * k] = (mcol[:, k] * dh).sum(axis=0)
            mgoff[n, 2 * k + 1] = (mcol[:, k] * dw).sum(axis=0)
            for idx, wgt in zip((hl * W + wl, hl * W + wh, hh * W + wl, hh * W + wh), cw):
                rows.append(idx)
                cols.append(k * P + np.arange(P))
                vals.append(wgt)
        A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, K * P))
        mgx[n] = (A @ mcol.reshape(Cin, K * P).T).T
    mgb = ga.sum(axis=(0, 2, 3))
    return (mgx.reshape(N, Cin, H, W), mgoff.reshape(N, 2 * K, Ho, Wo),
            mgw.transpose(2, 0, 1).reshape(Cout, Cin, kh, kw), mgb)


def deformable_convolution_shared_backward_bound(gout, x, flow_yx, scale, stride, weight, kernel=(3, 3), pad=(1, 1)):
    """M of the flow-mode backward: offsets = repeat(flow * scale / stride) over the taps, d/dflow = scale / stride * sum over
    the taps of d/doffset; (Mgx, Mgflow, Mgw, Mgbias)."""
    K = kernel[0] * kernel[1]
    fl = np.asarray(flow_yx, np.float32)
    off = np.repeat((fl * np.float32(scale) / np.float32(stride))[:, None], K, axis=1).reshape(fl.shape[0], 2 * K, *fl.shape[2:])
    mgx, mgoff, mgw, mgb = deformable_convolution_backward_bound(gout, x, off, weight, kernel, pad)
    N, _, H, W = mgoff.shape
    return mgx, mgoff.reshape(N, K, 2, H, W).sum(axis=1) * (abs(float(scale)) / abs(float(stride))), mgw, mgb


def warp_positions(flow_yx, clip_grid=False, dtype=np.float64):
    """The sample positions of Reconstruction2D[Smooth] as GridGenerator('warp') + BilinearSampler form them, in `dtype`:
    grid = (flow + index) / ((size-1)/2) - 1 [clipped], real = (grid + 1) * (size-1) / 2.  Returns (y_real, x_real, y_in, x_in):
    y_in / x_in say where the unclipped grid lies inside [-1, 1] (the clip's gradient mask)."""
    fl = np.asarray(flow_yx, dtype)
    N, _, H, W = fl.shape
    t = np.dtype(dtype).type
    nx, ny = t((W - 1) / 2.0), t((H - 1) / 2.0)
    ys, xs = np.meshgrid(np.arange(H).astype(dtype), np.arange(W).astype(dtype), indexing="ij")
    gxr = (fl[:, 1] + xs) / nx - t(1)
    gyr = (fl[:, 0] + ys) / ny - t(1)
    gxc, gyc = (np.clip(gxr, t(-1), t(1)), np.clip(gyr, t(-1), t(1))) if clip_grid else (gxr, gyr)
    yr = (gyc + t(1)) * t(H - 1) / t(2)
    xr = (gxc + t(1)) * t(W - 1) / t(2)
    one = np.ones_like(gxr, dtype=bool)
    y_in = (gyr >= -1) & (gyr <= 1) if clip_grid else one
    x_in = (gxr >= -1) & (gxr <= 1) if clip_grid else one
    return (yr.astype(np.float64), xr.astype(np.float64), y_in, x_in)


def warp_backward_at(gout, x, positions, bound=False):
    """fp64 BilinearSampler backward at given sample positions (warp_positions), composed with GridGenerator('warp')'s backward:
    (gx, gflow).  bound=True: the magnitude bound M instead -- |gout| times the bilinear weights for gx; for gflow the terms of
    the derivative as MXNet's sampler (and warp_bwd_kernel) forms it, -(tr - br + (tl - tr - bl + br) * wx) for d/dy, each as
    |coef| |value| (the form is exact, but rounds at the scale of all four corners); d/dflow is zero where the clip cuts the grid."""
    g_all = np.asarray(gout, np.float64)
    x_all = np.asarray(x, np.float64)
    if bound:
        g_all, x_all = np.abs(g_all), np.abs(x_all)
    yr_all, xr_all, yin_all, xin_all = positions
    N, C, H, W = x_all.shape
    gx = np.zeros((N, C, H * W))
    gf = np.zeros((N, 2, H, W))
    for n in range(N):
        yr, xr = yr_all[n].ravel(), xr_all[n].ravel()
        y0 = np.floor(yr).astype(np.int64)
        x0 = np.floor(xr).astype(np.int64)
        wy = 1.0 - (yr - y0)
        wx = 1.0 - (xr - x0)
        g = g_all[n].reshape(C, H * W)
        xn = x_all[n].reshape(C, H * W)
        vals = []
        for dy, dx, wgt in ((0, 0, wy * wx), (0, 1, wy * (1 - wx)), (1, 0, (1 - wy) * wx), (1, 1, (1 - wy) * (1 - wx))):
            yy, xx = y0 + dy, x0 + dx
            ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = np.where(ok, yy * W + xx, 0)
            np.add.at(gx[n], (slice(None), idx[ok]), g[:, ok] * wgt[ok])
            vals.append(np.where(ok, xn[:, idx], 0.0))
        tl, tr, bl, br = vals
        if bound:   # the terms of BilinearSampler's own form, tr - br + (tl - tr - bl + br) * wx (it cancels tr, br as wx -> 1)
            d_y = tr + br + wx * (tl + tr + bl + br)
            d_x = bl + br + wy * (tl + tr + bl + br)
        else:
            d_y = wx * (bl - tl) + (1 - wx) * (br - tr)
            d_x = wy * (tr - tl) + (1 - wy) * (br - bl)
        gf[n, 0] = np.where(yin_all[n], (g * d_y).sum(axis=0).reshape(H, W), 0.0)
        gf[n, 1] = np.where(xin_all[n], (g * d_x).sum(axis=0).reshape(H, W), 0.0)
    return gx.reshape(N, C, H, W), gf


def warp_backward_bound(gout, x, flow_yx, clip_grid=False, positions_dtype=np.float64):
    """M of Reconstruction2D[Smooth]'s backward: (Mgx, Mgflow), at the sample positions the grid arithmetic gives in
    `positions_dtype` (float64: the fp64 oracle's; float32: the fp32 kernels' and the fp32 oracle's)."""
    return warp_backward_at(gout, x, warp_positions(flow_yx, clip_grid, positions_dtype), bound=True)


# ---- magnitude bounds of the forward pass ------------------------------------------------------------------------------------
# M as above, per output element.  Every forward operator here is a sum of products whose interpolation weights are >= 0, so M is
# the operator itself on the absolute values of its inputs, at the SAME sample positions.  A fused LeakyReLU is 1-Lipschitz and
# keeps zeros: its output is compared with leaky(want64) under the same M.
def correlation_bound(f1, f2, max_displacement=4):
    """M of Correlation (kernel 1, strides 1, pad = md, multiply): the cost volume of |f1|, |f2|; zero exactly where the
    displacement leaves the image."""
    return correlation(np.abs(np.asarray(f1, np.float64)), np.abs(np.asarray(f2, np.float64)), max_displacement)


def deformable_convolution_bound(x, offset, weight, bias=None, kernel=(3, 3), stride=(1, 1), dilate=(1, 1), pad=(1, 1),
                                 num_group=1, num_deformable_group=1):
    """M of DeformableConvolution: the operator on |x|, |W|, |b| at the same offsets (the bilinear weights are >= 0); without a
    bias, zero exactly where every tap of an output falls outside the image."""
    return deformable_convolution(np.abs(np.asarray(x, np.float64)), offset, np.abs(np.asarray(weight, np.float64)),
                                  None if bias is None else np.abs(np.asarray(bias, np.float64)), kernel, stride, dilate, pad,
                                  num_group, num_deformable_group)


def matching_bound(m_dc, mask=None, tradeoff=None):
    """M of the matching epilogue deform * sigmoid(mask) + tradeoff: M_dc * sigmoid(mask) + |tradeoff|."""
    m = np.asarray(m_dc, np.float64)
    if mask is not None:
        m = m * (1.0 / (1.0 + np.exp(-np.asarray(mask, np.float64))))
    if tradeoff is not None:
        m = m + np.abs(np.asarray(tradeoff, np.float64))
    return m


def warp_at(x, positions, bound=False):
    """fp64 BilinearSampler forward at given sample positions (warp_positions): the forward twin of warp_backward_at.  Corners
    outside the image contribute nothing.  bound=True: the magnitude bound M, the same sum on |x|."""
    x_all = np.asarray(x, np.float64)
    if bound:
        x_all = np.abs(x_all)
    yr_all, xr_all = positions[0], positions[1]
    N, C, H, W = x_all.shape
    out = np.zeros((N, C) + yr_all.shape[1:])
    for n in range(N):
        yr, xr = yr_all[n], xr_all[n]
        y0 = np.floor(yr).astype(np.int64)
        x0 = np.floor(xr).astype(np.int64)
        wy = 1.0 - (yr - y0)
        wx = 1.0 - (xr - x0)
        for dy, dx, wgt in ((0, 0, wy * wx), (0, 1, wy * (1 - wx)), (1, 0, (1 - wy) * wx), (1, 1, (1 - wy) * (1 - wx))):
            out[n] += _tap(x_all[n], y0 + dy, x0 + dx) * wgt[None]
    return out
