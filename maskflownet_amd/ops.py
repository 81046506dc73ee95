"""Operator front-end: the MXNet operator signatures of the hot path, on top of the C ABI.

Mirrors the operators /root/reference reaches (same names, argument meaning, shape inference and
error conditions), so the parity tests read like MXNet operator tests:

    Correlation(data1, data2, kernel_size, max_displacement, stride1, stride2, pad_size, is_multiply)
        -- network/MaskFlownet.py:193-195, :440-441
    GridGenerator(data, transform_type, target_shape) / BilinearSampler(data, grid)
        -- network/layer.py:17-18, :29-30; augmentation.py:60-64, 306-321
    DeformableConvolution(data, offset, weight, bias, kernel, stride, dilate, pad, num_filter,
                          num_group, num_deformable_group, no_bias)  -- network/layer.py:117-124
plus the fused forms the hot path actually wants: warp() (GridGenerator+clip+BilinearSampler in
one kernel) and deformable_convolution_shared() (offset builder of MaskFlownet.py:230 folded in).

`OpSet` is array-library agnostic: an adapter supplies raw addresses, allocation and the stream.
The module-level functions bind it to torch-ROCm tensors (torch is plumbing: device memory and
streams) and libmfn_hip.so.  There is no CPU implementation behind these functions.
"""
import ctypes

from . import _lib

_REQ = {"null": 0, None: 0, "write": 1, "add": 3}  # MXNet OpReqType


class OpSet:
    def __init__(self, ns, adapter, check):
        self.ns = ns
        self.ad = adapter
        self.check = check
        self._ws = {}
        self._retired = []

    # ---- helpers -------------------------------------------------------------------------------
    def _in(self, *arrs):
        return [self.ad.prepare(a) for a in arrs]

    def _workspace(self, like, nbytes):
        key = self.ad.device_key(like)
        ws = self._ws.get(key)
        if ws is None or self.ad.nbytes(ws) < nbytes:
            if ws is not None:
                # a hipGraph captured earlier (hotpath.capture, or a user's own capture) still holds the old
                # pointer: the superseded buffer must outlive it, so it is parked instead of freed -- until the owner of
                # those graphs says they are gone (release_retired)
                self._retired.append(ws)
            ws = self.ad.empty_bytes(like, max(int(nbytes), 1 << 20))
            self._ws[key] = ws
        return ws

    def release_retired(self):
        """Free the workspaces superseded by larger ones.  Call it when no hipGraph captured BEFORE the growth is alive any
        more (such a graph holds the old pointer); returns how many buffers were dropped."""
        n = len(self._retired)
        del self._retired[:]
        return n

    def _upload(self, like, host, nbytes):
        """`nbytes` (a multiple of 4) of a ctypes host buffer in a fresh device buffer next to `like`: a table built on the host."""
        buf = self.ad.empty_bytes(like, max(nbytes, 8))
        if nbytes:
            if hasattr(self.ad, "torch"):    # one host-to-device copy on the tensors' device, ordered on the current stream
                t = self.ad.torch
                buf[:nbytes // 4].copy_(t.frombuffer(host, dtype=t.float32, count=nbytes // 4))
            else:                            # host arrays (the emulation): the bytes themselves
                ctypes.memmove(self.ad.ptr(buf), ctypes.addressof(host), nbytes)
        return buf

    def _out(self, out, like, shape, what):
        """A caller-supplied destination goes to the kernel as it is: it must already be what the kernel writes --
        float32, contiguous NCHW of exactly `shape`, on the inputs' device (no silent copy, no reshaping)."""
        shape = tuple(int(v) for v in shape)
        if out is None:
            return self.ad.empty(like, shape)
        if self.ad.shape(out) != shape:
            raise ValueError("%s: out has shape %s, expected %s" % (what, self.ad.shape(out), shape))
        self.ad.require_destination(out, like, what)
        return out

    # ---- Correlation ---------------------------------------------------------------------------
    def correlation_out_shape(self, H, W, kernel_size=1, max_displacement=1, stride1=1, stride2=1, pad_size=0):
        c, h, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.check(self.ns.correlation_out_shape(H, W, max_displacement, kernel_size, stride1, stride2, pad_size,
                                                 ctypes.byref(c), ctypes.byref(h), ctypes.byref(w)))
        return c.value, h.value, w.value

    def Correlation(self, data1, data2, kernel_size=1, max_displacement=1, stride1=1, stride2=1, pad_size=0,
                    is_multiply=True, out=None, activation=None):
        """activation="leaky": LeakyReLU(0.1) fused into the epilogue (the reference applies it to every cost
        volume, MaskFlownet.py:217); bit-identical to the separate elementwise op."""
        if activation not in (None, "leaky"):
            raise ValueError("Correlation: activation must be None or 'leaky'")
        d1, d2 = self._in(data1, data2)
        if self.ad.ndim(d1) != 4 or self.ad.shape(d1) != self.ad.shape(d2):
            raise ValueError("Correlation: data1 and data2 must be 4-D with identical shapes, got %s and %s"
                             % (self.ad.shape(d1), self.ad.shape(d2)))
        N, C, H, W = self.ad.shape(d1)
        tc, th, tw = self.correlation_out_shape(H, W, kernel_size, max_displacement, stride1, stride2, pad_size)
        if out is None:
            out = self.ad.empty(d1, (N, tc, th, tw))
        elif self.ad.shape(out) != (N, tc, th, tw):
            raise ValueError("Correlation: out has shape %s, expected %s" % (self.ad.shape(out), (N, tc, th, tw)))
        # `out` may be a channel slice of the decoder's concat buffer (x = concat(corr, c1, feat, flow),
        # MaskFlownet.py:235): dense per image, images a whole (Ctot, h, w) apart
        st = self.ad.elem_strides(out)
        dims, want = (tc, th, tw), (th * tw, tw, 1)
        dense_img = all(d <= 1 or a == b for d, a, b in zip(dims, st[1:], want))  # size-1 dims: any stride
        if N * tc * th * tw != 0 and (not dense_img or (N > 1 and st[0] < tc * th * tw)):
            raise ValueError("Correlation: out must be contiguous or a channel slice buf[:, c0:c0+%d] of a contiguous "
                             "NCHW buffer (strides %s)" % (tc, st))
        args = (N, C, H, W, int(max_displacement), int(kernel_size), int(stride1), int(stride2), int(pad_size),
                int(bool(is_multiply)))
        nbytes = self.ns.correlation_workspace_bytes(*args)
        ws = self._workspace(d1, nbytes) if nbytes else None
        self.check(self.ns.correlation_fwd_into(self.ad.ptr(d1), self.ad.ptr(d2), self.ad.ptr(out),
                                                int(st[0]) if N > 1 else 0, *args,
                                                1 if activation == "leaky" else 0,
                                                self.ad.ptr(ws) if ws is not None else None,
                                                self.ad.nbytes(ws) if ws is not None else 0, self.ad.stream(d1)))
        return out

    def Correlation_backward(self, out_grad, data1, data2, kernel_size=1, max_displacement=1, stride1=1, stride2=1,
                             pad_size=0, is_multiply=True, req1="write", req2="write", g1=None, g2=None):
        """Gradients of Correlation w.r.t. data1 / data2 (MXNet CorrelationBackward)."""
        go, d1, d2 = self._in(out_grad, data1, data2)
        N, C, H, W = self.ad.shape(d1)
        tc, th, tw = self.correlation_out_shape(H, W, kernel_size, max_displacement, stride1, stride2, pad_size)
        if self.ad.shape(go) != (N, tc, th, tw):
            raise ValueError("Correlation_backward: out_grad shape %s, expected %s" % (self.ad.shape(go), (N, tc, th, tw)))
        r1, r2 = _REQ[req1], _REQ[req2]
        if g1 is None and r1:
            g1 = self.ad.empty(d1, (N, C, H, W))
        if g2 is None and r2:
            g2 = self.ad.empty(d1, (N, C, H, W))
        self.check(self.ns.correlation_bwd(self.ad.ptr(go), self.ad.ptr(d1), self.ad.ptr(d2),
                                           self.ad.ptr(g1) if r1 else None, self.ad.ptr(g2) if r2 else None, N, C, H, W,
                                           int(max_displacement), int(kernel_size), int(stride1), int(stride2),
                                           int(pad_size), int(bool(is_multiply)), r1, r2, self.ad.stream(d1)))
        return g1, g2

    # ---- warp ------------------------------------------------------------------------------------
    def warp(self, x, flow, clip_grid=False, out=None):
        """layer.py Reconstruction2D (clip_grid=False) / Reconstruction2DSmooth (True), fused.
        flow: (N,2,H,W), channel 0 = dy, channel 1 = dx."""
        xx, fl = self._in(x, flow)
        if self.ad.ndim(xx) != 4:
            raise ValueError("warp: x must be 4-D")
        N, C, H, W = self.ad.shape(xx)
        if self.ad.shape(fl) != (N, 2, H, W):
            raise ValueError("warp: flow must have shape %s, got %s" % ((N, 2, H, W), self.ad.shape(fl)))
        out = self._out(out, xx, (N, C, H, W), "warp")
        self.check(self.ns.warp_fwd(self.ad.ptr(xx), self.ad.ptr(fl), self.ad.ptr(out), N, C, H, W,
                                    int(bool(clip_grid)), self.ad.stream(xx)))
        return out

    def warp_backward(self, out_grad, x, flow, clip_grid=False, req_x="write", req_flow="write", gx=None, gflow=None):
        """Gradients of warp() w.r.t. x and flow (BilinearSamplerBackward + GridGenerator 'warp' backward + flip)."""
        go, xx, fl = self._in(out_grad, x, flow)
        N, C, H, W = self.ad.shape(xx)
        rx, rf = _REQ[req_x], _REQ[req_flow]
        if gx is None and rx:
            gx = self.ad.empty(xx, (N, C, H, W))
        if gflow is None and rf:
            gflow = self.ad.empty(xx, (N, 2, H, W))
        self.check(self.ns.warp_bwd(self.ad.ptr(go), self.ad.ptr(xx), self.ad.ptr(fl), self.ad.ptr(gx) if rx else None,
                                    self.ad.ptr(gflow) if rf else None, N, C, H, W, int(bool(clip_grid)), rx, rf,
                                    self.ad.stream(xx)))
        return gx, gflow

    def GridGenerator(self, data, transform_type, target_shape=None):
        (d,) = self._in(data)
        if transform_type == "warp":
            if self.ad.ndim(d) != 4 or self.ad.shape(d)[1] != 2:
                raise ValueError("GridGenerator(warp): data must be (N,2,H,W)")
            N, _, H, W = self.ad.shape(d)
            grid = self.ad.empty(d, (N, 2, H, W))
            self.check(self.ns.grid_generator_warp(self.ad.ptr(d), self.ad.ptr(grid), N, H, W, self.ad.stream(d)))
            return grid
        if transform_type == "affine":
            if target_shape is None or len(target_shape) != 2:
                raise ValueError("GridGenerator(affine): target_shape=(H,W) is required")
            shp = self.ad.shape(d)
            if len(shp) != 2 or shp[1] != 6:
                raise ValueError("GridGenerator(affine): data must be (N,6)")
            H, W = int(target_shape[0]), int(target_shape[1])
            grid = self.ad.empty(d, (shp[0], 2, H, W))
            self.check(self.ns.grid_generator_affine(self.ad.ptr(d), self.ad.ptr(grid), shp[0], H, W,
                                                     self.ad.stream(d)))
            return grid
        raise ValueError("GridGenerator: transform_type must be 'affine' or 'warp'")

    def BilinearSampler(self, data, grid):
        d, g = self._in(data, grid)
        if self.ad.ndim(d) != 4 or self.ad.ndim(g) != 4 or self.ad.shape(g)[1] != 2 or \
                self.ad.shape(g)[0] != self.ad.shape(d)[0]:
            raise ValueError("BilinearSampler: data (N,C,H,W) and grid (N,2,H',W') expected")
        N, C, iH, iW = self.ad.shape(d)
        _, _, oH, oW = self.ad.shape(g)
        out = self.ad.empty(d, (N, C, oH, oW))
        self.check(self.ns.bilinear_sampler_fwd(self.ad.ptr(d), self.ad.ptr(g), self.ad.ptr(out), N, C, iH, iW, oH,
                                                oW, self.ad.stream(d)))
        return out

    def BilinearSampler_backward(self, out_grad, data, grid, req_data="write", req_grid="write", gdata=None, ggrid=None):
        """Gradients of BilinearSampler w.r.t. data and grid (BilinearSamplerBackward of MXNet's bilinear_sampler.cc)."""
        go, d, g = self._in(out_grad, data, grid)
        N, C, iH, iW = self.ad.shape(d)
        _, _, oH, oW = self.ad.shape(g)
        rd, rg = _REQ[req_data], _REQ[req_grid]
        if gdata is None and rd:
            gdata = self.ad.empty(d, (N, C, iH, iW))
        if ggrid is None and rg:
            ggrid = self.ad.empty(d, (N, 2, oH, oW))
        self.check(self.ns.bilinear_sampler_bwd(self.ad.ptr(go), self.ad.ptr(d), self.ad.ptr(g),
                                                self.ad.ptr(gdata) if rd else None, self.ad.ptr(ggrid) if rg else None,
                                                N, C, iH, iW, oH, oW, rd, rg, self.ad.stream(d)))
        return gdata, ggrid

    def GridGenerator_backward(self, out_grad, transform_type="warp", req="write", gdata=None):
        """Gradient of GridGenerator('warp') w.r.t. its flow input: grad / ((size - 1) / 2) per channel."""
        if transform_type != "warp":
            raise NotImplementedError("GridGenerator backward: only transform_type='warp' (the affine grids of "
                                      "augmentation.py are never differentiated)")
        (go,) = self._in(out_grad)
        N, two, H, W = self.ad.shape(go)
        if two != 2:
            raise ValueError("GridGenerator(warp) backward: out_grad must be (N,2,H,W)")
        r = _REQ[req]
        if gdata is None and r:
            gdata = self.ad.empty(go, (N, 2, H, W))
        self.check(self.ns.grid_generator_warp_bwd(self.ad.ptr(go), self.ad.ptr(gdata) if r else None, N, H, W, r,
                                                   self.ad.stream(go)))
        return gdata

    # ---- DeformableConvolution -----------------------------------------------------------------------
    @staticmethod
    def _pair(v):
        if isinstance(v, (tuple, list)):
            if len(v) != 2:
                raise ValueError("2-D kernel/stride/pad/dilate expected, got %r" % (v,))
            return int(v[0]), int(v[1])
        return int(v), int(v)

    def deform_conv_out_shape(self, H, W, kernel, stride=(1, 1), pad=(0, 0), dilate=(1, 1)):
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(self._pair, (kernel, stride, pad, dilate))
        ho, wo = ctypes.c_int(), ctypes.c_int()
        self.check(self.ns.deform_conv_out_shape(H, W, kh, kw, sh, sw, ph, pw, dh, dw, ctypes.byref(ho),
                                                 ctypes.byref(wo)))
        return ho.value, wo.value

    def DeformableConvolution(self, data, offset, weight, bias=None, kernel=(3, 3), stride=(1, 1), dilate=(1, 1),
                              pad=(0, 0), num_filter=None, num_group=1, num_deformable_group=1, no_bias=False,
                              layout="NCHW", out=None, packed=None):
        """packed: a PackedDeformWeights from pack_deform_weights() for these constant weights (inference);
        the per-call re-layout of `weight` is skipped, results are bit-identical."""
        if layout not in (None, "NCHW"):
            raise ValueError("DeformableConvolution: only layout='NCHW' is supported")
        if no_bias:
            bias = None
        elif bias is None:
            raise ValueError("DeformableConvolution: bias is required unless no_bias=True")
        x, off, w = self._in(data, offset, weight)
        b = self._in(bias)[0] if bias is not None else None
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(self._pair, (kernel, stride, pad, dilate))
        if self.ad.ndim(x) != 4:
            raise ValueError("DeformableConvolution: data must be 4-D")
        N, Cin, H, W = self.ad.shape(x)
        Cout = self.ad.shape(w)[0]
        if num_filter is not None and int(num_filter) != Cout:
            raise ValueError("DeformableConvolution: num_filter=%s but weight has %d filters" % (num_filter, Cout))
        if Cin % num_group or Cout % num_group or Cin % num_deformable_group:
            raise ValueError("DeformableConvolution: channels must divide num_group / num_deformable_group")
        if self.ad.shape(w) != (Cout, Cin // num_group, kh, kw):
            raise ValueError("DeformableConvolution: weight shape %s, expected %s"
                             % (self.ad.shape(w), (Cout, Cin // num_group, kh, kw)))
        Ho, Wo = self.deform_conv_out_shape(H, W, (kh, kw), (sh, sw), (ph, pw), (dh, dw))
        exp_off = (N, 2 * kh * kw * num_deformable_group, Ho, Wo)
        if self.ad.shape(off) != exp_off:
            raise ValueError("DeformableConvolution: offset shape %s, expected %s" % (self.ad.shape(off), exp_off))
        if b is not None and self.ad.shape(b) != (Cout,):
            raise ValueError("DeformableConvolution: bias shape %s, expected (%d,)" % (self.ad.shape(b), Cout))
        out = self._out(out, x, (N, Cout, Ho, Wo), "DeformableConvolution")
        nbytes = self.ns.deform_conv_workspace_bytes(N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, num_group,
                                                     num_deformable_group)
        ws = self._workspace(x, nbytes)
        dims = (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, num_group, num_deformable_group)
        if packed is not None:
            packed.require(dims)
            self.check(self.ns.deform_conv_fwd_packed(self.ad.ptr(x), self.ad.ptr(off), self.ad.ptr(packed.buf),
                                                      packed.nbytes, packed.tag, self.ad.ptr(b) if b is not None else None,
                                                      self.ad.ptr(out), *dims, self.ad.ptr(ws), self.ad.nbytes(ws),
                                                      self.ad.stream(x)))
            return out
        self.check(self.ns.deform_conv_fwd(self.ad.ptr(x), self.ad.ptr(off), self.ad.ptr(w),
                                           self.ad.ptr(b) if b is not None else None, self.ad.ptr(out), *dims,
                                           self.ad.ptr(ws), self.ad.nbytes(ws), self.ad.stream(x)))
        return out

    def pack_deform_weights(self, weight, data_shape, kernel=(3, 3), stride=(1, 1), dilate=(1, 1), pad=(0, 0),
                            num_group=1, num_deformable_group=1, out=None):
        """Lay constant DeformableConvolution weights out once for inputs of `data_shape` (N,Cin,H,W);
        mfn_deform_conv_pack_weights.  The layout depends on the shape and on set_tuning(): re-pack after
        changing either (a stale pack is refused, never silently used).  out: a PackedDeformWeights of the same dims whose
        buffer is written again (new weights at an address a captured graph holds)."""
        (w,) = self._in(weight)
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(self._pair, (kernel, stride, pad, dilate))
        N, Cin, H, W = (int(v) for v in data_shape)
        Cout = self.ad.shape(w)[0]
        if self.ad.shape(w) != (Cout, Cin // num_group, kh, kw):
            raise ValueError("pack_deform_weights: weight shape %s, expected %s"
                             % (self.ad.shape(w), (Cout, Cin // num_group, kh, kw)))
        dims = (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, int(num_group), int(num_deformable_group))
        nbytes = self.ns.deform_conv_packed_weight_bytes(*dims)
        if not nbytes:
            raise ValueError("pack_deform_weights: bad shape %s" % (dims,))
        buf = self._pack_buffer(w, nbytes, dims, out, "pack_deform_weights")
        tag = ctypes.c_ulonglong()
        self.check(self.ns.deform_conv_pack_weights(self.ad.ptr(w), *dims, self.ad.ptr(buf), nbytes,
                                                    ctypes.byref(tag), self.ad.stream(w)))
        return PackedDeformWeights(buf, nbytes, dims, tag.value)

    def DeformableConvolution_backward(self, out_grad, data, offset, weight, kernel=(3, 3), stride=(1, 1),
                                       dilate=(1, 1), pad=(0, 0), num_group=1, num_deformable_group=1, no_bias=False,
                                       req=("write", "write", "write", "write"), out=None):
        """Gradients w.r.t. (data, offset, weight, bias) -- MXNet DeformableConvolutionOp::Backward.
        out: optional (gx, goffset, gweight, gbias) buffers to write/add into (required for req "add"; lets a
        training step keep its parameter gradients in one flat all-reduce bucket)."""
        go, x, off, w = self._in(out_grad, data, offset, weight)
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(self._pair, (kernel, stride, pad, dilate))
        N, Cin, H, W = self.ad.shape(x)
        Cout = self.ad.shape(w)[0]
        rq = [_REQ[r] for r in req]
        if no_bias:
            rq[3] = 0
        want = (self.ad.shape(x), self.ad.shape(off), self.ad.shape(w), (Cout,))
        given = tuple(out) if out is not None else (None, None, None, None)
        if len(given) != 4:
            raise ValueError("DeformableConvolution_backward: out must be (gx, goffset, gweight, gbias)")
        grads = []
        for i, (g, shp) in enumerate(zip(given, want)):
            if not rq[i]:
                grads.append(None)
            elif g is None:
                if rq[i] == _REQ["add"]:
                    raise ValueError("DeformableConvolution_backward: req 'add' needs the buffer to add into (out[%d])" % i)
                grads.append(self.ad.empty(x, shp))
            else:
                self.ad.require_destination(g, x, "DeformableConvolution_backward")   # written in place: no silent copy
                if self.ad.shape(g) != tuple(shp):
                    raise ValueError("DeformableConvolution_backward: out[%d] has shape %s, expected %s"
                                     % (i, self.ad.shape(g), tuple(shp)))
                grads.append(g)
        gx, goff, gw, gb = grads
        p = lambda a: self.ad.ptr(a) if a is not None else None
        nbytes = self.ns.deform_conv_bwd_workspace_bytes(N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, num_group,
                                                         num_deformable_group)
        ws = self._workspace(x, nbytes) if nbytes else None   # per-block slabs of the weight / bias gradient
        self.check(self.ns.deform_conv_bwd(self.ad.ptr(go), self.ad.ptr(x), self.ad.ptr(off), self.ad.ptr(w), p(gx),
                                           p(goff), p(gw), p(gb), N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw,
                                           num_group, num_deformable_group, rq[0], rq[1], rq[2], rq[3],
                                           self.ad.ptr(ws) if ws is not None else None,
                                           self.ad.nbytes(ws) if ws is not None else 0, self.ad.stream(x)))
        return gx, goff, gw, gb

    def deformable_convolution_shared_backward(self, out_grad, data, flow, flow_scale, flow_stride, weight, kernel=(3, 3),
                                               dilate=(1, 1), pad=(1, 1), num_group=1, no_bias=False,
                                               req=("write", "write", "write", "write"), out=None):
        """Gradients of deformable_convolution_shared w.r.t. (data, flow, weight, bias): the fused call's backward
        (mfn_deform_conv_shared_bwd).  d/dflow = flow_scale / flow_stride * sum over the taps of the offset gradient.
        out: optional (gx, gflow, gweight, gbias) buffers (required for req "add")."""
        go, x, fl, w = self._in(out_grad, data, flow, weight)
        (kh, kw), (ph, pw), (dh, dw) = map(self._pair, (kernel, pad, dilate))
        N, Cin, H, W = self.ad.shape(x)
        Cout = self.ad.shape(w)[0]
        if self.ad.shape(fl) != (N, 2, H, W):
            raise ValueError("deformable_convolution_shared_backward: flow must be (N,2,H,W) = %s, got %s"
                             % ((N, 2, H, W), self.ad.shape(fl)))
        rq = [_REQ[r] for r in req]
        if no_bias:
            rq[3] = 0
        want = (self.ad.shape(x), self.ad.shape(fl), self.ad.shape(w), (Cout,))
        given = tuple(out) if out is not None else (None, None, None, None)
        if len(given) != 4:
            raise ValueError("deformable_convolution_shared_backward: out must be (gx, gflow, gweight, gbias)")
        grads = []
        for i, (g, shp) in enumerate(zip(given, want)):
            if not rq[i]:
                grads.append(None)
            elif g is None:
                if rq[i] == _REQ["add"]:
                    raise ValueError("deformable_convolution_shared_backward: req 'add' needs the buffer to add into (out[%d])" % i)
                grads.append(self.ad.empty(x, shp))
            else:
                self.ad.require_destination(g, x, "deformable_convolution_shared_backward")   # written in place: no silent copy
                if self.ad.shape(g) != tuple(shp):
                    raise ValueError("deformable_convolution_shared_backward: out[%d] has shape %s, expected %s"
                                     % (i, self.ad.shape(g), tuple(shp)))
                grads.append(g)
        gx, gfl, gw, gb = grads
        p = lambda a: self.ad.ptr(a) if a is not None else None
        nbytes = self.ns.deform_conv_shared_bwd_workspace_bytes(N, Cin, H, W, Cout, kh, kw, ph, pw, dh, dw, num_group)
        ws = self._workspace(x, nbytes)
        self.check(self.ns.deform_conv_shared_bwd(self.ad.ptr(go), self.ad.ptr(x), self.ad.ptr(fl), float(flow_scale),
                                                  float(flow_stride), self.ad.ptr(w), p(gx), p(gfl), p(gw), p(gb), N, Cin, H, W,
                                                  Cout, kh, kw, ph, pw, dh, dw, num_group, rq[0], rq[1], rq[2], rq[3],
                                                  self.ad.ptr(ws), self.ad.nbytes(ws), self.ad.stream(x)))
        return gx, gfl, gw, gb

    def offsets_from_flow_backward(self, offset_grad, scale, stride, taps=9, req="write", out=None):
        """Gradient of offsets_from_flow: (N,2,H,W) = scale / stride * sum over the taps."""
        (go,) = self._in(offset_grad)
        N, c, H, W = self.ad.shape(go)
        if c != 2 * taps:
            raise ValueError("offsets_from_flow_backward: offset gradient must be (N,%d,H,W)" % (2 * taps))
        if req == "add" and out is None:
            raise ValueError("offsets_from_flow_backward: req 'add' needs the buffer to add into")
        out = self._out(out, go, (N, 2, H, W), "offsets_from_flow_backward")
        self.check(self.ns.offsets_from_flow_bwd(self.ad.ptr(go), self.ad.ptr(out), N, H, W, int(taps), float(scale),
                                                 float(stride), _REQ[req], self.ad.stream(go)))
        return out

    def deformable_convolution_shared(self, data, flow, flow_scale, flow_stride, weight, bias=None, kernel=(3, 3),
                                      dilate=(1, 1), pad=(1, 1), num_group=1, out=None, packed=None):
        """DeformableConvolution with offset = repeat9(flow*flow_scale/flow_stride) (MaskFlownet.py:230)
        without materialising the offset tensor.  packed: see DeformableConvolution."""
        x, fl, w = self._in(data, flow, weight)
        b = self._in(bias)[0] if bias is not None else None
        (kh, kw), (ph, pw), (dh, dw) = map(self._pair, (kernel, pad, dilate))
        N, Cin, H, W = self.ad.shape(x)
        Cout = self.ad.shape(w)[0]
        if self.ad.shape(w) != (Cout, Cin // num_group, kh, kw):
            raise ValueError("deformable_convolution_shared: bad weight shape %s" % (self.ad.shape(w),))
        if self.ad.shape(fl) != (N, 2, H, W):
            raise ValueError("deformable_convolution_shared: flow must be %s" % ((N, 2, H, W),))
        out = self._out(out, x, (N, Cout, H, W), "deformable_convolution_shared")
        nbytes = self.ns.deform_conv_workspace_bytes(N, Cin, H, W, Cout, kh, kw, 1, 1, ph, pw, dh, dw, num_group, 1)
        ws = self._workspace(x, nbytes)
        if packed is not None:
            packed.require((N, Cin, H, W, Cout, kh, kw, 1, 1, ph, pw, dh, dw, num_group, 1))
            self.check(self.ns.deform_conv_shared_fwd_packed(
                self.ad.ptr(x), self.ad.ptr(fl), float(flow_scale), float(flow_stride), self.ad.ptr(packed.buf),
                packed.nbytes, packed.tag, self.ad.ptr(b) if b is not None else None, self.ad.ptr(out), N, Cin, H, W, Cout,
                kh, kw,
                ph, pw, dh, dw, num_group, self.ad.ptr(ws), self.ad.nbytes(ws), self.ad.stream(x)))
            return out
        self.check(self.ns.deform_conv_shared_fwd(self.ad.ptr(x), self.ad.ptr(fl), float(flow_scale),
                                                  float(flow_stride), self.ad.ptr(w),
                                                  self.ad.ptr(b) if b is not None else None, self.ad.ptr(out), N, Cin,
                                                  H, W, Cout, kh, kw, ph, pw, dh, dw, num_group, self.ad.ptr(ws),
                                                  self.ad.nbytes(ws), self.ad.stream(x)))
        return out

    def Upsample(self, img, factor, out=None):
        """MaskFlownet.py:35-62 Upsample(factor): (N,C,H,W) -> (N,C,H*factor,W*factor)."""
        (x,) = self._in(img)
        if self.ad.ndim(x) != 4:
            raise ValueError("Upsample: data must be 4-D")
        N, C, H, W = self.ad.shape(x)
        factor = int(factor)
        if factor < 1:
            raise ValueError("Upsample: factor must be >= 1")
        out = self._out(out, x, (N, C, H * factor, W * factor), "Upsample")
        self.check(self.ns.upsample_fwd(self.ad.ptr(x), self.ad.ptr(out), N, C, H, W, factor, self.ad.stream(x)))
        return out

    # ---- prediction on images of any size (network/pipeline.py:85-87, :117-147, :176-182) ---------------------------------
    def bilinear_resize(self, data, height, width, sub=None, flow_rescale=False, out=None):
        """contrib.BilinearResize2D(data, height, width) of MXNet 1.5 (align_corners; pipeline.py:129-130, :140, :142):
        (N,C,Hin,Win) -> (N,C,height,width), positions and blend in fp32.  sub (N,C): subtracted from every tap before the
        blend (centralize, then resize).  flow_rescale (C == 2): channel 0 * height/Hin, channel 1 * width/Win after the blend."""
        (x,) = self._in(data)
        if self.ad.ndim(x) != 4:
            raise ValueError("bilinear_resize: data must be 4-D")
        N, C, Hin, Win = self.ad.shape(x)
        m = None
        if sub is not None:
            (m,) = self._in(sub)
            if self.ad.shape(m) != (N, C):
                raise ValueError("bilinear_resize: sub must have shape %s, got %s" % ((N, C), self.ad.shape(m)))
        if flow_rescale and C != 2:
            raise ValueError("bilinear_resize: flow_rescale needs a (N,2,H,W) flow, got C=%d" % C)
        out = self._out(out, x, (N, C, int(height), int(width)), "bilinear_resize")
        self.check(self.ns.bilinear_resize_fwd(self.ad.ptr(x), self.ad.ptr(m) if m is not None else None, self.ad.ptr(out), N, C,
                                               Hin, Win, int(height), int(width), int(bool(flow_rescale)), self.ad.stream(x)))
        return out

    def pair_mean(self, img1, img2, out=None):
        """rgb_mean of PipelineFlownet.centralize (pipeline.py:86): (N,C) joint mean of the pair, fixed summation order."""
        a, b = self._in(img1, img2)
        if self.ad.ndim(a) != 4 or self.ad.shape(a) != self.ad.shape(b):
            raise ValueError("pair_mean: img1 and img2 must be 4-D with identical shapes, got %s and %s"
                             % (self.ad.shape(a), self.ad.shape(b)))
        N, C, H, W = self.ad.shape(a)
        out = self._out(out, a, (N, C), "pair_mean")
        ws = self._workspace(a, self.ns.pair_mean_workspace_bytes(N, C, H, W))
        self.check(self.ns.pair_mean(self.ad.ptr(a), self.ad.ptr(b), self.ad.ptr(out), N, C, H, W, self.ad.ptr(ws),
                                     self.ad.nbytes(ws), self.ad.stream(a)))
        return out

    def preprocess_pair(self, img1, img2, height, width, mean=None, out=None):
        """centralize + BilinearResize2D of both images in one launch (pipeline.py:120-130): -> (2N,C,height,width) with image 1
        in rows [0,N) and image 2 in rows [N,2N), the network's input batch.  mean: (N,C), default pair_mean(img1, img2)."""
        a, b = self._in(img1, img2)
        if self.ad.ndim(a) != 4 or self.ad.shape(a) != self.ad.shape(b):
            raise ValueError("preprocess_pair: img1 and img2 must be 4-D with identical shapes, got %s and %s"
                             % (self.ad.shape(a), self.ad.shape(b)))
        N, C, H, W = self.ad.shape(a)
        if mean is None:
            mean = self.pair_mean(a, b)
        (m,) = self._in(mean)
        if self.ad.shape(m) != (N, C):
            raise ValueError("preprocess_pair: mean must have shape %s, got %s" % ((N, C), self.ad.shape(m)))
        out = self._out(out, a, (2 * N, C, int(height), int(width)), "preprocess_pair")
        self.check(self.ns.preprocess_pair(self.ad.ptr(a), self.ad.ptr(b), self.ad.ptr(m), self.ad.ptr(out), N, C, H, W,
                                           int(height), int(width), self.ad.stream(a)))
        return out

    def flow_metric_sums(self, flow, label, mask, out=None):
        """(N,3) per-sample sums of mfn_flow_metrics: sum mask * sqrt(|flow-label|^2 + 1e-8), sum mask, sum mask * outlier."""
        f, l, m = self._in(flow, label, mask)
        if self.ad.ndim(f) != 4 or self.ad.shape(f)[1] != 2 or self.ad.shape(l) != self.ad.shape(f):
            raise ValueError("flow_metrics: flow and label must both be (N,2,H,W), got %s and %s" % (self.ad.shape(f), self.ad.shape(l)))
        N, _, H, W = self.ad.shape(f)
        if self.ad.shape(m) != (N, 1, H, W):
            raise ValueError("flow_metrics: mask must have shape %s, got %s" % ((N, 1, H, W), self.ad.shape(m)))
        out = self._out(out, f, (N, 3), "flow_metrics")
        ws = self._workspace(f, self.ns.flow_metrics_workspace_bytes(N, H, W))
        self.check(self.ns.flow_metrics(self.ad.ptr(f), self.ad.ptr(l), self.ad.ptr(m), self.ad.ptr(out), N, H, W, self.ad.ptr(ws),
                                        self.ad.nbytes(ws), self.ad.stream(f)))
        return out

    def flow_metrics(self, flow, label, mask):
        """-> (epe, fl), each (N,): EpeLossWithMask (MaskFlownet.py:576-583) and the KITTI outlier ratio (pipeline.py:182); flow and
        label in network order (channel 0 = dy).  A sample whose mask is all zero gives nan, as the reference's 0 / 0 does."""
        s = self.flow_metric_sums(flow, label, mask)
        return s[:, 0] / s[:, 1], s[:, 2] / s[:, 1]

    # ---- augmentation of the training batch (augmentation.py:168-339, as pipeline.py:100-101 applies it) --------------------------
    def augment_geometry(self, img1, img2, flow, mask, table, target_shape, label_order=0, out=None):
        """GeometryAugmentation.hybrid_forward (augmentation.py:295-338) in one launch.  img1, img2 (N,3,Ho,Wo); flow (N,2,Ho,Wo)
        as (u, v); mask (N,1,Ho,Wo) or (N,1,1,1) (a constant plane, never materialised); table (N,26) per kernels/augment.h.
        -> (img1', img2', flow', mask') at target_shape; label_order=1 writes the flow as (dy, dx) (pipeline.py:105).
        out: the four destinations."""
        a, b, f, m, t = self._in(img1, img2, flow, mask, table)
        if self.ad.ndim(a) != 4 or self.ad.shape(a)[1] != 3 or self.ad.shape(b) != self.ad.shape(a):
            raise ValueError("augment_geometry: img1 and img2 must both be (N,3,H,W), got %s and %s" % (self.ad.shape(a), self.ad.shape(b)))
        N, _, Ho, Wo = self.ad.shape(a)
        if self.ad.shape(f) != (N, 2, Ho, Wo):
            raise ValueError("augment_geometry: flow must have shape %s, got %s" % ((N, 2, Ho, Wo), self.ad.shape(f)))
        if self.ad.shape(m) not in ((N, 1, Ho, Wo), (N, 1, 1, 1)):
            raise ValueError("augment_geometry: mask must have shape %s or %s, got %s" % ((N, 1, Ho, Wo), (N, 1, 1, 1), self.ad.shape(m)))
        if self.ad.shape(t) != (N, 26):
            raise ValueError("augment_geometry: table must have shape %s, got %s" % ((N, 26), self.ad.shape(t)))
        Ht, Wt = (int(v) for v in target_shape)
        o = out if out is not None else (None,) * 4
        if len(o) != 4:
            raise ValueError("augment_geometry: out must hold four destinations")
        o1 = self._out(o[0], a, (N, 3, Ht, Wt), "augment_geometry img1")
        o2 = self._out(o[1], a, (N, 3, Ht, Wt), "augment_geometry img2")
        of = self._out(o[2], a, (N, 2, Ht, Wt), "augment_geometry flow")
        om = self._out(o[3], a, (N, 1, Ht, Wt), "augment_geometry mask")
        self.check(self.ns.augment_geometry(self.ad.ptr(a), self.ad.ptr(b), self.ad.ptr(f), self.ad.ptr(m),
                                            int(self.ad.shape(m) == (N, 1, Ho, Wo)), self.ad.ptr(t), self.ad.ptr(o1), self.ad.ptr(o2),
                                            self.ad.ptr(of), self.ad.ptr(om), N, Ho, Wo, Ht, Wt, int(bool(label_order)),
                                            self.ad.stream(a)))
        return o1, o2, of, om

    def _color_args(self, what, img1, img2, table):
        a, b, t = self._in(img1, img2, table)
        if self.ad.ndim(a) != 4 or self.ad.shape(a)[1] != 3 or self.ad.shape(b) != self.ad.shape(a):
            raise ValueError("%s: img1 and img2 must both be (N,3,H,W), got %s and %s" % (what, self.ad.shape(a), self.ad.shape(b)))
        if self.ad.shape(t) != (self.ad.shape(a)[0], 26):
            raise ValueError("%s: table must have shape %s, got %s" % (what, (self.ad.shape(a)[0], 26), self.ad.shape(t)))
        return a, b, t

    def augment_color_mean(self, img1, img2, table, sigma=0.0, seed=0, offset=0, out=None):
        """The per (image, sample, channel) mean of augmentation.py:216 over a = M rgb + noise * sigma: -> (2N,3), fixed summation
        order.  seed, offset: the 64-bit Philox key and the call counter; sigma == 0 uses neither."""
        a, b, t = self._color_args("augment_color_mean", img1, img2, table)
        N, _, H, W = self.ad.shape(a)
        out = self._out(out, a, (2 * N, 3), "augment_color_mean")
        ws = self._workspace(a, self.ns.augment_color_mean_workspace_bytes(N, H, W))
        self.check(self.ns.augment_color_mean(self.ad.ptr(a), self.ad.ptr(b), self.ad.ptr(t), float(sigma), int(seed) & (2 ** 64 - 1),
                                              int(offset) & (2 ** 64 - 1), self.ad.ptr(out), N, H, W, self.ad.ptr(ws), self.ad.nbytes(ws),
                                              self.ad.stream(a)))
        return out

    def augment_color(self, img1, img2, table, sigma=0.0, seed=0, offset=0, spin=False, gamma=False, mean=None, out=None):
        """ColorAugmentation.hybrid_forward (augmentation.py:213-225) for both images: -> (2N,3,H,W), images 1 first.  mean: (2N,3),
        default augment_color_mean with the same table, sigma, seed and offset."""
        a, b, t = self._color_args("augment_color", img1, img2, table)
        N, _, H, W = self.ad.shape(a)
        if mean is None:
            mean = self.augment_color_mean(a, b, t, sigma, seed, offset)
        (m,) = self._in(mean)
        if self.ad.shape(m) != (2 * N, 3):
            raise ValueError("augment_color: mean must have shape %s, got %s" % ((2 * N, 3), self.ad.shape(m)))
        out = self._out(out, a, (2 * N, 3, H, W), "augment_color")
        self.check(self.ns.augment_color(self.ad.ptr(a), self.ad.ptr(b), self.ad.ptr(t), self.ad.ptr(m), float(sigma),
                                         int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), int(bool(spin)), int(bool(gamma)),
                                         self.ad.ptr(out), N, H, W, self.ad.stream(a)))
        return out

    # ---- the fused multiscale training loss (MaskFlownet.py:563-611 as pipeline.py:42-44 builds it) --------------------------------
    def _loss_args(self, what, preds, label, mask, scales, weights, q):
        preds = self._in(*preds)
        l, m = self._in(label, mask)
        scales, weights = [int(f) for f in scales], [float(w) for w in weights]
        S = len(preds)
        if not 1 <= S <= 8 or len(scales) != S or len(weights) != S:
            raise ValueError("%s: 1..8 predictions with one scale and one weight each, got %d predictions, %d scales, %d weights"
                             % (what, S, len(scales), len(weights)))
        if self.ad.ndim(l) != 4 or self.ad.shape(l)[1] != 2:
            raise ValueError("%s: label must be (N,2,H,W), got %s" % (what, self.ad.shape(l)))
        N, _, H, W = self.ad.shape(l)
        if self.ad.shape(m) not in ((N, 1, H, W), (N, 1, 1, 1)):
            raise ValueError("%s: mask must have shape %s or %s, got %s" % (what, (N, 1, H, W), (N, 1, 1, 1), self.ad.shape(m)))
        for p, f in zip(preds, scales):
            if f < 1 or H % f or W % f or self.ad.shape(p) != (N, 2, H // f, W // f):
                raise ValueError("%s: the prediction of scale %d must have shape (N,2,H/%d,W/%d) of label %s, got %s"
                                 % (what, f, f, f, self.ad.shape(l), self.ad.shape(p)))
        if q is not None and not float(q) > 0:
            raise ValueError("%s: q must be positive (or None for the sqrt form), got %r" % (what, q))
        scalar = int(self.ad.shape(m) != (N, 1, H, W))
        host = ((ctypes.c_void_p * S)(*[self.ad.ptr(p) for p in preds]), (ctypes.c_int * S)(*scales), (ctypes.c_float * S)(*weights))
        return preds, l, m, scales, host, scalar, (N, H, W)

    def multiscale_epe(self, preds, label, mask, scales, weights, eps=1e-8, q=None):
        """MultiscaleEpe(scales, weights, match='upsampling', eps, q) of MaskFlownet.py:585-611 in two launches: preds[s]
        (N,2,H/scales[s],W/scales[s]), label (N,2,H,W), mask (N,1,H,W) or (N,1,1,1) -> (loss (N,), sums (N,S+1): the S masked sums
        and sum(mask)).  q=None: sqrt(dy^2 + dx^2 + eps); q: (|dy| + |dx| + eps)^q.  No full-resolution tensor is written."""
        preds, l, m, scales, (pp, ff, ww), scalar, (N, H, W) = self._loss_args("multiscale_epe", preds, label, mask, scales, weights, q)
        S = len(preds)
        loss = self.ad.empty(l, (N,))
        sums = self.ad.empty(l, (N, S + 1))
        ws = self._workspace(l, self.ns.multiscale_epe_workspace_bytes(N, H, W, S))
        self.check(self.ns.multiscale_epe_fwd(pp, ff, ww, S, self.ad.ptr(l), self.ad.ptr(m), scalar, float(eps), int(q is not None),
                                              float(q or 0.0), self.ad.ptr(loss), self.ad.ptr(sums), N, H, W, self.ad.ptr(ws),
                                              self.ad.nbytes(ws), self.ad.stream(l)))
        return loss, sums

    def multiscale_epe_backward(self, gloss, preds, label, mask, scales, weights, sums, eps=1e-8, q=None, reqs=None, out=None):
        """Gradients of multiscale_epe's loss with respect to the predictions: gloss (N,), sums as the forward returned them ->
        a tuple with one (N,2,h,w) gradient per prediction (None where req is 'null').  reqs: 'write' / 'add' / 'null' per
        prediction (default all 'write'); out: the destinations ('add' needs them)."""
        what = "multiscale_epe_backward"
        preds, l, m, scales, (pp, ff, ww), scalar, (N, H, W) = self._loss_args(what, preds, label, mask, scales, weights, q)
        S = len(preds)
        g, sm = self._in(gloss, sums)
        if self.ad.shape(g) != (N,) or self.ad.shape(sm) != (N, S + 1):
            raise ValueError("%s: gloss must be %s and sums %s, got %s and %s" % (what, (N,), (N, S + 1), self.ad.shape(g), self.ad.shape(sm)))
        reqs = ["write"] * S if reqs is None else list(reqs)
        out = [None] * S if out is None else list(out)
        if len(reqs) != S or len(out) != S:
            raise ValueError("%s: reqs and out must have one entry per prediction" % what)
        gp = []
        for s in range(S):
            if _REQ[reqs[s]] == 0:
                gp.append(None)
                continue
            if _REQ[reqs[s]] == _REQ["add"] and out[s] is None:
                raise ValueError("%s: req 'add' needs the buffer to add into" % what)
            gp.append(self._out(out[s], l, self.ad.shape(preds[s]), what))
        gptr = (ctypes.c_void_p * S)(*[None if t is None else self.ad.ptr(t) for t in gp])
        rr = (ctypes.c_int * S)(*[_REQ[r] for r in reqs])
        self.check(self.ns.multiscale_epe_bwd(self.ad.ptr(g), pp, ff, ww, S, self.ad.ptr(l), self.ad.ptr(m), scalar, float(eps),
                                              int(q is not None), float(q or 0.0), self.ad.ptr(sm), gptr, rr, N, H, W, self.ad.stream(l)))
        return tuple(gp)

    # ---- the trainer's Adam step (MXNet's adam_update, pipeline.py:27 and :114) ---------------------------------------------------
    def _adam_tensors(self, what, weight, grad, mean, var):
        """The four tensors of one parameter as they are (updated in place: no copy may come between)."""
        ts = [self.ad.prepare_strided(t) for t in (weight, grad, mean, var)]
        shape = self.ad.shape(ts[0])
        n = 1
        for d in shape:
            n *= int(d)
        dense, st = [], 1
        for d in reversed(shape):
            dense.insert(0, st)
            st *= int(d)
        for name, t in zip(("weight", "grad", "mean", "var"), ts):
            if self.ad.shape(t) != shape:
                raise ValueError("%s: %s has shape %s, weight %s" % (what, name, self.ad.shape(t), shape))
            if n and any(d > 1 and a != b for d, a, b in zip(shape, self.ad.elem_strides(t), dense)):
                raise ValueError("%s: %s must be contiguous (strides %s)" % (what, name, self.ad.elem_strides(t)))
        return ts, n

    @staticmethod
    def _adam_scalars(lr, beta1, beta2, epsilon, wd, rescale_grad, clip_gradient):
        clip = -1.0 if clip_gradient is None else float(clip_gradient)
        return (float(lr), float(beta1), float(beta2), float(epsilon), float(wd), float(rescale_grad), clip)

    def adam_update(self, weight, grad, mean, var, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, wd=0.0, rescale_grad=1.0,
                    clip_gradient=-1.0):
        """mx.nd.adam_update(weight, grad, mean, var, out=weight, ...): weight, mean and var are updated IN PLACE (mfn_adam_update).
        lr carries the bias corrections, as MXNet's Adam.update hands it over.  clip_gradient < 0 (or None): no clipping."""
        (w, g, m, v), n = self._adam_tensors("adam_update", weight, grad, mean, var)
        self.check(self.ns.adam_update(self.ad.ptr(w), self.ad.ptr(g), self.ad.ptr(m), self.ad.ptr(v), n,
                                       *self._adam_scalars(lr, beta1, beta2, epsilon, wd, rescale_grad, clip_gradient), self.ad.stream(w)))
        return weight

    def multi_adam_table(self, weights, grads, means, vars, lr_mults=None, wd_mults=None):
        """The device-resident table of mfn_multi_adam_update over these tensors (lists of equal length; lr_mults / wd_mults: one
        float per tensor, default 1): built on the host by mfn_multi_adam_build_table, uploaded once.  It holds addresses: a tensor
        that moved needs a new table (AdamTable.stale)."""
        what = "multi_adam_table"
        T = len(weights)
        if not T or not (len(grads) == len(means) == len(vars) == T):
            raise ValueError("%s: one grad, mean and var per weight and at least one tensor, got %d / %d / %d / %d"
                             % (what, T, len(grads), len(means), len(vars)))
        for name, mult in (("lr_mults", lr_mults), ("wd_mults", wd_mults)):
            if mult is not None and len(mult) != T:
                raise ValueError("%s: %s must have one entry per tensor" % (what, name))
        rows = [self._adam_tensors(what, *q) for q in zip(weights, grads, means, vars)]
        ptrs = tuple(tuple(self.ad.ptr(t) for t in ts) for ts, _ in rows)
        counts = (ctypes.c_longlong * T)(*[n for _, n in rows])
        cols = [(ctypes.c_void_p * T)(*[p[k] for p in ptrs]) for k in range(4)]
        lm = None if lr_mults is None else (ctypes.c_float * T)(*[float(x) for x in lr_mults])
        wm = None if wd_mults is None else (ctypes.c_float * T)(*[float(x) for x in wd_mults])
        nbytes = self.ns.multi_adam_table_bytes(T, counts)
        host = (ctypes.c_ulonglong * max(1, (nbytes + 7) // 8))()
        nb, tag = ctypes.c_int(), ctypes.c_ulonglong()
        self.check(self.ns.multi_adam_build_table(T, *cols, counts, lm, wm, ctypes.addressof(host), nbytes, ctypes.byref(nb), ctypes.byref(tag)))
        return AdamTable(self._upload(rows[0][0][0], host, nbytes), nbytes, tag.value, T, nb.value, ptrs, [n for _, n in rows])

    def multi_adam_update(self, table, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, wd=0.0, rescale_grad=1.0, clip_gradient=-1.0):
        """adam_update over every tensor of `table` (multi_adam_table) in one launch, in place; a tensor's lr and wd are scaled by
        its lr_mult and wd_mult."""
        self.check(self.ns.multi_adam_update(self.ad.ptr(table.buf), table.nbytes, table.tag, table.n_tensors, table.n_blocks,
                                             *self._adam_scalars(lr, beta1, beta2, epsilon, wd, rescale_grad, clip_gradient),
                                             self.ad.stream(table.buf)))

    # ---- one training batch out of a device-resident data set (main.py:466-486) -----------------------------------------------------
    _BATCH_LABEL = {"float32": 0, "float16": 1}

    def _raw(self, a, what, dtypes, shape=None):
        """A uint8 / float16 / float32 device array as it is (the adapters' prepare insists on float32): -> its dtype's name.  Dense
        and C-ordered; `shape`, where given, is what it must have."""
        if hasattr(self.ad, "torch") and not isinstance(a, self.ad.torch.Tensor):
            raise TypeError("%s: expected a torch.Tensor on a ROCm device, got %r" % (what, type(a)))
        if getattr(a, "is_cuda", True) is False:
            raise RuntimeError("maskflownet_amd ops run on the MI355X only: %s is on %s (there is no CPU fallback)" % (what, a.device))
        name = str(getattr(a, "dtype", type(a))).split(".")[-1]
        if name not in dtypes:
            raise TypeError("%s: %s expected, got %s" % (what, " or ".join(dtypes), name))
        got = self.ad.shape(a)
        if shape is not None and got != tuple(shape):
            raise ValueError("%s: shape %s, expected %s" % (what, got, tuple(shape)))
        st = 1
        for d, have in zip(reversed(got), reversed(self.ad.elem_strides(a))):
            if d > 1 and have != st:
                raise ValueError("%s must be contiguous (strides %s)" % (what, self.ad.elem_strides(a)))
            st *= int(d)
        return name

    def batch_gather_rows(self, samples, crop_shape, origins, flips):
        """The device-resident table of mfn_batch_gather for one batch: one slot per entry of `samples`, each (img1, img2, flow, mask
        or None) of device arrays in the readers' HWC layout -- img1, img2 uint8 (Hs,Ws,3), flow float32 or float16 (Hs,Ws,2), mask uint8
        (Hs,Ws) or (Hs,Ws,1); origins: (y0, x0) per slot; flips: 0 / 1 per slot.  Built and checked on the host by
        mfn_batch_gather_build_rows (a crop that leaves its source, a source that is not 16-byte aligned: refused), uploaded once.
        Every source must be readable up to the next multiple of 16 bytes of its size (data.DeviceDataset pads it so)."""
        what = "batch_gather_rows"
        N = len(samples)
        Hc, Wc = (int(v) for v in crop_shape)
        if not N or len(origins) != N or len(flips) != N:
            raise ValueError("%s: one origin and one flip per sample and at least one sample, got %d / %d / %d" % (what, N, len(origins), len(flips)))
        ptrs, Hs, Ws, lt = [[], [], [], []], [], [], []
        for n, smp in enumerate(samples):
            img1, img2, flow, mask = smp
            self._raw(img1, "%s: img1 of slot %d" % (what, n), ("uint8",))
            shp = self.ad.shape(img1)
            if len(shp) != 3 or shp[2] != 3:
                raise ValueError("%s: img1 of slot %d has shape %s, expected (Hs, Ws, 3)" % (what, n, shp))
            h, w = int(shp[0]), int(shp[1])
            self._raw(img2, "%s: img2 of slot %d" % (what, n), ("uint8",), (h, w, 3))
            lt.append(self._BATCH_LABEL[self._raw(flow, "%s: flow of slot %d" % (what, n), ("float32", "float16"), (h, w, 2))])
            if mask is not None:
                self._raw(mask, "%s: mask of slot %d" % (what, n), ("uint8",), (h, w, 1) if len(self.ad.shape(mask)) == 3 else (h, w))
            for col, a in zip(ptrs, (img1, img2, flow, mask)):
                col.append(None if a is None else self.ad.ptr(a))
            Hs.append(h)
            Ws.append(w)
        ints = lambda v: (ctypes.c_int * N)(*[int(x) for x in v])
        cols = [(ctypes.c_void_p * N)(*c) for c in ptrs]
        nbytes = self.ns.batch_gather_rows_bytes(N)
        host = (ctypes.c_ulonglong * (nbytes // 8))()
        tag = ctypes.c_ulonglong()
        self.check(self.ns.batch_gather_build_rows(N, *cols, ints(Hs), ints(Ws), ints(lt), ints([o[0] for o in origins]),
                                                   ints([o[1] for o in origins]), ints(flips), Hc, Wc, ctypes.addressof(host), nbytes,
                                                   ctypes.byref(tag)))
        return BatchRows(self._upload(samples[0][0], host, nbytes), nbytes, tag.value, N, (Hc, Wc), samples, origins, flips)

    def batch_gather(self, rows, crop_shape, with_mask, out=None):
        """One batch in one launch (mfn_batch_gather): -> (img1, img2 (N,3,Hc,Wc) uint8, label (N,2,Hc,Wc) float32 in the readers' (u, v)
        order, mask (N,1,Hc,Wc) uint8 or None), exactly what main.py:466-486 stacks on the host.  out[n,c,y,x] = src_n[y0 + y,
        x0 + (flip ? Wc-1-x : x), c]; with flip the label's channel 0 is negated; a slot without a mask writes 255.  with_mask False:
        no mask is written or returned.  out: the four destinations (the last one None without a mask), used as they are."""
        what = "batch_gather"
        N = rows.N
        Hc, Wc = (int(v) for v in crop_shape)
        shapes = ((N, 3, Hc, Wc), (N, 3, Hc, Wc), (N, 2, Hc, Wc), (N, 1, Hc, Wc))
        kinds = ("uint8", "uint8", "float32", "uint8")
        if out is None:
            dt = (lambda k: getattr(self.ad.torch, k)) if hasattr(self.ad, "torch") else (lambda k: k)
            out = []
            for shape, kind in zip(shapes, kinds):
                if shape[1] == 1 and not with_mask:
                    out.append(None)
                    continue
                nb = N * shape[1] * Hc * Wc * (4 if kind == "float32" else 1)
                out.append(self.ad.empty_bytes(rows.buf, nb).view(dt(kind))[:nb // (4 if kind == "float32" else 1)].reshape(shape))
        else:
            out = list(out)
            if len(out) != 4:
                raise ValueError("%s: out must be (img1, img2, label, mask or None)" % what)
            for o, shape, kind, name in zip(out, shapes, kinds, ("img1", "img2", "label", "mask")):
                if o is not None:
                    self._raw(o, "%s: out %s" % (what, name), (kind,), shape)
                elif name != "mask" or with_mask:
                    raise ValueError("%s: out %s is missing" % (what, name))
        i1, i2, lab, msk = out
        self.check(self.ns.batch_gather(self.ad.ptr(rows.buf), rows.nbytes, rows.tag, N, Hc, Wc, int(bool(with_mask)), self.ad.ptr(i1),
                                        self.ad.ptr(i2), self.ad.ptr(lab), self.ad.ptr(msk) if with_mask else None,
                                        self.ad.stream(rows.buf)))
        return i1, i2, lab, (msk if with_mask else None)

    # ---- a validation batch read through the rows of a resident data set (pipeline.py:149-187; kernels/validate.h) -------------------
    def _val_rows(self, rows, first, n, what):
        """The window [first, first + n) of a table of batch_gather_rows, checked on the host before any launch: every slot the whole
        (H, W) sample, unflipped.  -> (address of row `first`, H, W)."""
        if not isinstance(rows, BatchRows):
            raise TypeError("%s: rows must come from batch_gather_rows, got %r" % (what, type(rows)))
        if getattr(rows.buf, "is_cuda", True) is False:
            raise RuntimeError("maskflownet_amd ops run on the MI355X only: %s: the table is on %s (there is no CPU fallback)"
                               % (what, rows.buf.device))
        first, n = int(first), int(n)
        if first < 0 or n < 0 or first + n > rows.N:
            raise ValueError("%s: rows [%d, %d) leave a table of %d" % (what, first, first + n, rows.N))
        if len(rows.origins) != rows.N or len(rows.flips) != rows.N:
            raise ValueError("%s: the table carries no host copy of its origins and flips" % what)
        H, W = rows.crop_shape
        for k in range(first, first + n):
            shp = tuple(int(v) for v in self.ad.shape(rows.samples[k][0])[:2])
            if shp != (H, W) or rows.origins[k] != (0, 0) or rows.flips[k] != 0:
                raise ValueError("%s: row %d is a %dx%d crop at %s%s of a %dx%d sample; a validation slot is the whole sample, unflipped"
                                 % (what, k, H, W, rows.origins[k], " flipped" if rows.flips[k] else "", shp[0], shp[1]))
        return self.ad.ptr(rows.buf) + first * BatchRows.ROW_BYTES, H, W

    def val_pair_mean(self, rows, first, n, out=None):
        """pair_mean_u8 for the n slots from row `first` of a table of batch_gather_rows, read where the samples lie: rgb_mean of
        pipeline.py:86 on bytes / 255 -> (n,3), exact; the bits of pair_mean_u8 on the same images (mfn_val_pair_mean)."""
        what = "val_pair_mean"
        table, H, W = self._val_rows(rows, first, n, what)
        n = int(n)
        out = self._out(out, rows.buf, (n, 3), what)
        ws = self._workspace(rows.buf, self.ns.val_pair_mean_workspace_bytes(n, H, W))
        self.check(self.ns.val_pair_mean(table, n, H, W, self.ad.ptr(out), self.ad.ptr(ws), self.ad.nbytes(ws), self.ad.stream(rows.buf)))
        return out

    def val_preprocess(self, rows, first, n, height, width, mean=None, out=None):
        """preprocess_pair_u8 for those slots (pipeline.py:208, :120-130): -> (2n,3,height,width), image 1 of slot k in row k, image 2 in
        row n + k; the bits of preprocess_pair_u8 on the same images.  mean (n,3): subtracted from every tap; None subtracts nothing."""
        what = "val_preprocess"
        table, H, W = self._val_rows(rows, first, n, what)
        n = int(n)
        m = None
        if mean is not None:
            (m,) = self._in(mean)
            if self.ad.shape(m) != (n, 3):
                raise ValueError("%s: mean must have shape %s, got %s" % (what, (n, 3), self.ad.shape(m)))
        out = self._out(out, rows.buf, (2 * n, 3, int(height), int(width)), what)
        self.check(self.ns.val_preprocess(table, n, H, W, self.ad.ptr(m) if m is not None else None, self.ad.ptr(out), int(height),
                                          int(width), self.ad.stream(rows.buf)))
        return out

    def val_flow_metric_sums(self, rows, first, n, flow, out=None):
        """flow_metric_sums of flow (n,2,H,W), network order, against those slots' stored labels and masks (pipeline.py:175-176, :146,
        :182): the label's (u, v) flipped to (dy, dx), fp16 widened exactly, the mask byte / 255 (all valid without one) -> (n,3); the
        bits of flow_metric_sums on the materialised fp32 tensors (mfn_val_flow_metrics)."""
        what = "val_flow_metric_sums"
        table, H, W = self._val_rows(rows, first, n, what)
        n = int(n)
        (f,) = self._in(flow)
        if self.ad.shape(f) != (n, 2, H, W):
            raise ValueError("%s: flow must have shape %s, got %s" % (what, (n, 2, H, W), self.ad.shape(f)))
        out = self._out(out, f, (n, 3), what)
        ws = self._workspace(f, self.ns.val_flow_metrics_workspace_bytes(n, H, W))
        self.check(self.ns.val_flow_metrics(table, self.ad.ptr(f), n, H, W, self.ad.ptr(out), self.ad.ptr(ws), self.ad.nbytes(ws),
                                            self.ad.stream(f)))
        return out

    # ---- raw decoded KITTI / HD1K arrays into stored samples (reader/kitti.py:57-74, reader/hd1k.py:51-78) ---------------------------
    _INGEST_FLOW = {"float32": 0, "float16": 1}

    def _like(self, like):
        """A device array to allocate next to: `like`, or (torch) an empty tensor on the current ROCm device."""
        if like is None and hasattr(self.ad, "torch"):
            like = self.ad.torch.empty(0, device="cuda")
        return like

    def _raw_out(self, like, shape, kind, out, what):
        """The destination of an ingest op: `out` as it is (dtype, shape and density checked), or a fresh dense array."""
        if out is not None:
            self._raw(out, what, (kind,), shape)
            return out
        item = {"uint8": 1, "int32": 4, "float32": 4, "float16": 2}[kind]
        n = 1
        for d in shape:
            n *= int(d)
        dt = getattr(self.ad.torch, kind) if hasattr(self.ad, "torch") else kind
        return self.ad.empty_bytes(like, max(n * item, 4)).view(dt)[:n].reshape(tuple(shape))

    def ingest_tables(self, src_hw, dst_hw, like=None):
        """The device-resident resampling tables of mfn_ingest_image / mfn_ingest_flow_occ for a (h, w) window and a (H', W')
        destination: OpenCV's INTER_LINEAR positions and coefficients per destination column and row, built on the host by
        mfn_ingest_build_tables, uploaded once and cached per pair of sizes (and device / stream)."""
        h, w = (int(v) for v in src_hw)
        Hd, Wd = (int(v) for v in dst_hw)
        like = self._like(like)
        key = (h, w, Hd, Wd, self.ad.device_key(like))
        if not hasattr(self, "_ingest_cache"):
            self._ingest_cache = {}
        tab = self._ingest_cache.get(key)
        if tab is None:
            nbytes = self.ns.ingest_tables_bytes(Hd, Wd)
            host = (ctypes.c_ulonglong * max(1, nbytes // 8))()
            tag = ctypes.c_ulonglong()
            self.check(self.ns.ingest_build_tables(h, w, Hd, Wd, ctypes.addressof(host), nbytes, ctypes.byref(tag)))
            tab = IngestTables(self._upload(like, host, nbytes), nbytes, tag.value, (h, w), (Hd, Wd))
            self._ingest_cache[key] = tab
        return tab

    def _ingest_src(self, src, window, kind, what):
        self._raw(src, what, (kind,))
        shp = self.ad.shape(src)
        if len(shp) != 3 or shp[2] != 3:
            raise ValueError("%s has shape %s, expected (H, W, 3)" % (what, shp))
        y0, x0, h, w = ((0, 0, shp[0], shp[1]) if window is None else (int(v) for v in window))
        return int(shp[0]), int(shp[1]), y0, x0, h, w

    def ingest_minmax(self, img1, img2, window=None, out=None):
        """min and max over the window (y0, x0, h, w) of both uint8 (H, W, 3) images, all channels (hd1k.py:55) -> int32 (2,) on the
        device (mfn_ingest_minmax); what ingest_image's `minmax` takes."""
        what = "ingest_minmax"
        H, W, y0, x0, h, w = self._ingest_src(img1, window, "uint8", what + ": img1")
        self._raw(img2, what + ": img2", ("uint8",), (H, W, 3))
        out = self._raw_out(img1, (2,), "int32", out, what + ": out")
        self.check(self.ns.ingest_minmax(self.ad.ptr(img1), self.ad.ptr(img2), H, W, 3 * W, y0, x0, h, w, self.ad.ptr(out), self.ad.stream(img1)))
        return out

    def ingest_image(self, src, window, dst_hw, tables, bgr=False, minmax=None, out=None):
        """The window (y0, x0, h, w) of a uint8 (H, W, 3) device array -> uint8 (H', W', 3): channel reversal (bgr), HD1K's contrast
        stretch (minmax: ingest_minmax's result), cv2.resize's fixed-point bilinear (mfn_ingest_image).  tables: ingest_tables((h, w),
        (H', W')).  The source must be readable up to the next multiple of 16 bytes of its size."""
        what = "ingest_image"
        H, W, y0, x0, h, w = self._ingest_src(src, window, "uint8", what + ": src")
        Hd, Wd = (int(v) for v in dst_hw)
        if minmax is not None:
            self._raw(minmax, what + ": minmax", ("int32",), (2,))
        out = self._raw_out(src, (Hd, Wd, 3), "uint8", out, what + ": out")
        self.check(self.ns.ingest_image(self.ad.ptr(src), H, W, 3 * W, y0, x0, h, w, self.ad.ptr(tables.buf), tables.nbytes, tables.tag, int(bool(bgr)),
                                        None if minmax is None else self.ad.ptr(minmax), self.ad.ptr(out), Hd, Wd, self.ad.stream(src)))
        return out

    def ingest_flow_occ(self, src_u16, window, dst_hw, tables, premultiply=False, flow_dtype="float32", out_flow=None, out_mask=None):
        """The window of a uint16 (H, W, 3) device array in the file's order (R = u, G = v, B = valid) -> (flow (H', W', 2) in (u, v)
        order, float32 or float16; mask (H', W', 1) uint8): kitti.py:61-72, with premultiply hd1k.py:57-76 (mfn_ingest_flow_occ)."""
        what = "ingest_flow_occ"
        if flow_dtype not in self._INGEST_FLOW:
            raise ValueError("%s: flow_dtype must be 'float32' or 'float16', got %r" % (what, flow_dtype))
        H, W, y0, x0, h, w = self._ingest_src(src_u16, window, "uint16", what + ": src")
        Hd, Wd = (int(v) for v in dst_hw)
        out_flow = self._raw_out(src_u16, (Hd, Wd, 2), flow_dtype, out_flow, what + ": out_flow")
        out_mask = self._raw_out(src_u16, (Hd, Wd, 1), "uint8", out_mask, what + ": out_mask")
        self.check(self.ns.ingest_flow_occ(self.ad.ptr(src_u16), H, W, 3 * W, y0, x0, h, w, self.ad.ptr(tables.buf), tables.nbytes, tables.tag,
                                           int(bool(premultiply)), self._INGEST_FLOW[flow_dtype], self.ad.ptr(out_flow), self.ad.ptr(out_mask), Hd,
                                           Wd, self.ad.stream(src_u16)))
        return out_flow, out_mask

    # ---- prediction on uint8 frame sequences, the colour picture of a flow (predict_new_data.py:152-158) -----------------------------
    def _frames(self, frames, a0, b0, n, what):
        self._raw(frames, what + ": frames", ("uint8",))
        shp = self.ad.shape(frames)
        if len(shp) != 4 or shp[3] != 3:
            raise ValueError("%s: frames has shape %s, expected (F, H, W, 3)" % (what, shp))
        return tuple(int(v) for v in shp[:3]) + (int(a0), int(b0), int(n))

    def pair_mean_u8(self, frames, a0, b0, n, out=None):
        """rgb_mean of PipelineFlownet.centralize (pipeline.py:86) for the n pairs (frames[a0+k], frames[b0+k]) of a uint8 (F,H,W,3)
        device array read as bytes / 255: -> (n,3), exact (integer sums; mfn_pair_mean_u8), not the bits of pair_mean on floats."""
        what = "pair_mean_u8"
        F, H, W, a0, b0, n = self._frames(frames, a0, b0, n, what)
        out = self._out(out, frames, (n, 3), what)
        ws = self._workspace(frames, self.ns.pair_mean_u8_workspace_bytes(n, H, W))
        self.check(self.ns.pair_mean_u8(self.ad.ptr(frames), F, H, W, a0, b0, n, self.ad.ptr(out), self.ad.ptr(ws), self.ad.nbytes(ws),
                                        self.ad.stream(frames)))
        return out

    def preprocess_pair_u8(self, frames, a0, b0, n, height, width, mean=None, out=None):
        """preprocess_pair reading the bytes of a uint8 (F,H,W,3) device array, every tap (float)byte / 255.f (pipeline.py:208,
        :120-130): -> (2n,3,height,width), frames[a0+k] in row k and frames[b0+k] in row n + k; the bits of preprocess_pair on those
        floats.  mean (n,3): subtracted from every tap; None subtracts nothing.  height == H and width == W unpacks."""
        what = "preprocess_pair_u8"
        F, H, W, a0, b0, n = self._frames(frames, a0, b0, n, what)
        m = None
        if mean is not None:
            (m,) = self._in(mean)
            if self.ad.shape(m) != (n, 3):
                raise ValueError("%s: mean must have shape %s, got %s" % (what, (n, 3), self.ad.shape(m)))
        out = self._out(out, frames, (2 * n, 3, int(height), int(width)), what)
        self.check(self.ns.preprocess_pair_u8(self.ad.ptr(frames), F, H, W, a0, b0, n, self.ad.ptr(m) if m is not None else None,
                                              self.ad.ptr(out), int(height), int(width), self.ad.stream(frames)))
        return out

    def flow_color(self, flow, rad_max=None, bgr=False, out=None):
        """flow_vis.flow_to_color(flow, convert_to_bgr=bgr) of predict_new_data.py:155,:158 ([flow_vis-ext, unpinned]; mfn_flow_color):
        flow (N,2,H,W) in network order (channel 0 = dy) -> uint8 (N,H,W,3).  rad_max: the radius that saturates the colours, one for
        all images; None takes each image's own largest finite radius."""
        what = "flow_color"
        (f,) = self._in(flow)
        if self.ad.ndim(f) != 4 or self.ad.shape(f)[1] != 2:
            raise ValueError("%s: flow must be (N,2,H,W), got %s" % (what, self.ad.shape(f)))
        if rad_max is not None and not float(rad_max) >= 0.0:
            raise ValueError("%s: rad_max must be >= 0 or None, got %r" % (what, rad_max))
        N, _, H, W = self.ad.shape(f)
        out = self._raw_out(f, (N, H, W, 3), "uint8", out, what + ": out")
        ws = self._workspace(f, self.ns.flow_color_workspace_bytes(N, H, W))
        self.check(self.ns.flow_color(self.ad.ptr(f), self.ad.ptr(out), N, H, W, -1.0 if rad_max is None else float(rad_max), int(bool(bgr)),
                                      self.ad.ptr(ws), self.ad.nbytes(ws), self.ad.stream(f)))
        return out

    def cv_resize_u8(self, img, dst_hw, out=None):
        """cv2.resize(img, (W', H')) of a uint8 (H, W, 3) device array, INTER_LINEAR (kitti.py:105-106, the test-set images)."""
        shp = self.ad.shape(img)
        if len(shp) != 3:
            raise ValueError("cv_resize_u8: img has shape %s, expected (H, W, 3)" % (shp,))
        return self.ingest_image(img, None, dst_hw, self.ingest_tables(shp[:2], dst_hw, like=img), out=out)

    def Upsample_backward(self, out_grad, factor, req="write", out=None):
        """Adjoint of Upsample(factor): (N,C,H*f,W*f) -> (N,C,H,W) (mfn_upsample_bwd)."""
        (go,) = self._in(out_grad)
        factor = int(factor)
        N, C, Hf, Wf = self.ad.shape(go)
        if factor < 1 or Hf % factor or Wf % factor:
            raise ValueError("Upsample_backward: out_grad %s is no multiple of factor %d" % ((Hf, Wf), factor))
        if _REQ[req] == _REQ["add"] and out is None:
            raise ValueError("Upsample_backward: req 'add' needs the buffer to add into")
        out = self._out(out, go, (N, C, Hf // factor, Wf // factor), "Upsample_backward")
        self.check(self.ns.upsample_bwd(self.ad.ptr(go), self.ad.ptr(out), N, C, Hf // factor, Wf // factor, factor, _REQ[req],
                                        self.ad.stream(go)))
        return out

    def LeakyReLU_backward(self, out_grad, output, slope=0.1, out=None):
        """gin = gout * (y > 0 ? 1 : slope) from the forward OUTPUT y (the fused activations' gradient side)."""
        go, y = self._in(out_grad, output)
        if self.ad.shape(go) != self.ad.shape(y):
            raise ValueError("LeakyReLU_backward: out_grad %s vs output %s" % (self.ad.shape(go), self.ad.shape(y)))
        out = self._out(out, go, self.ad.shape(go), "LeakyReLU_backward")
        n = 1
        for d in self.ad.shape(go):
            n *= d
        self.check(self.ns.leaky_relu_bwd(self.ad.ptr(go), self.ad.ptr(y), self.ad.ptr(out), n, float(slope), self.ad.stream(go)))
        return out

    def _conv_backward(self, what, transposed, out_grad, data, weight, output, kernel, stride, dilate, pad, adj, num_group,
                       no_bias, activation, req, out):
        if activation not in (None, "leaky"):
            raise ValueError("%s: activation must be None or 'leaky'" % what)
        if activation == "leaky" and output is None:
            raise ValueError("%s: the forward output is needed for activation='leaky'" % what)
        go, x, w = self._in(out_grad, data, weight)
        y = self._in(output)[0] if output is not None else None
        (kh, kw), (sh, sw), (ph, pw), (dh, dw), (ah, aw) = map(self._pair, (kernel, stride, pad, dilate, adj))
        N, Cin, H, W = self.ad.shape(x)
        g = int(num_group)
        Cout = self.ad.shape(w)[1] * g if transposed else self.ad.shape(w)[0]
        Ho, Wo = self.conv_out_shape(H, W, (kh, kw), (sh, sw), (ph, pw), (dh, dw), transposed, (ah, aw))
        if self.ad.shape(go) != (N, Cout, Ho, Wo):
            raise ValueError("%s: out_grad has shape %s, expected %s" % (what, self.ad.shape(go), (N, Cout, Ho, Wo)))
        rq = [_REQ[r] for r in req]
        if no_bias:
            rq[2] = 0
        want = (self.ad.shape(x), self.ad.shape(w), (Cout,))
        given = tuple(out) if out is not None else (None, None, None)
        if len(given) != 3:
            raise ValueError("%s: out must be (gx, gweight, gbias)" % what)
        grads = []
        for i, (gbuf, shp) in enumerate(zip(given, want)):
            if not rq[i]:
                grads.append(None)
            elif gbuf is None:
                if rq[i] == _REQ["add"]:
                    raise ValueError("%s: req 'add' needs the buffer to add into (out[%d])" % (what, i))
                grads.append(self.ad.empty(x, shp))
            else:
                self.ad.require_destination(gbuf, x, what)
                if self.ad.shape(gbuf) != tuple(shp):
                    raise ValueError("%s: out[%d] has shape %s, expected %s" % (what, i, self.ad.shape(gbuf), tuple(shp)))
                grads.append(gbuf)
        gx, gw, gb = grads
        act = 1 if activation == "leaky" else 0
        dims = (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, g, int(bool(transposed)), ah, aw, act)
        nbytes = self.ns.conv2d_bwd_workspace_bytes(*dims)
        ws = self._workspace(x, nbytes) if nbytes else None
        p = lambda a: self.ad.ptr(a) if a is not None else None
        self.check(self.ns.conv2d_bwd(self.ad.ptr(go), self.ad.ptr(x), self.ad.ptr(w), p(y), p(gx), p(gw), p(gb), *dims,
                                      rq[0], rq[1], rq[2], p(ws), self.ad.nbytes(ws) if ws is not None else 0, self.ad.stream(x)))
        return gx, gw, gb

    def Convolution_backward(self, out_grad, data, weight, output=None, kernel=(3, 3), stride=(1, 1), dilate=(1, 1), pad=(0, 0),
                             num_group=1, no_bias=False, activation=None, req=("write", "write", "write"), out=None):
        """Gradients of Convolution w.r.t. (data, weight, bias) -- mfn_conv2d_bwd; `output` = the forward result, needed when
        the forward fused activation='leaky'."""
        return self._conv_backward("Convolution_backward", False, out_grad, data, weight, output, kernel, stride, dilate, pad,
                                   (0, 0), num_group, no_bias, activation, req, out)

    def Deconvolution_backward(self, out_grad, data, weight, output=None, kernel=(4, 4), stride=(2, 2), dilate=(1, 1),
                               pad=(1, 1), adj=(0, 0), num_group=1, no_bias=False, activation=None,
                               req=("write", "write", "write"), out=None):
        """Gradients of Deconvolution w.r.t. (data, weight, bias)."""
        return self._conv_backward("Deconvolution_backward", True, out_grad, data, weight, output, kernel, stride, dilate, pad,
                                   adj, num_group, no_bias, activation, req, out)

    def deformable_matching(self, data, flow, flow_scale, flow_stride, weight, bias=None, mask=None, tradeoff=None,
                            leaky=True, kernel=(3, 3), dilate=(1, 1), pad=(1, 1), num_group=1, out=None, packed=None):
        """MaskFlownet.py:230-233 in one launch: LeakyReLU(0.1)(deform(data, repeat9(flow*scale/stride)) *
        sigmoid(mask) + tradeoff); mask (N,1,H,W), tradeoff (N,Cout,H,W), both optional."""
        x, fl, w = self._in(data, flow, weight)
        b = self._in(bias)[0] if bias is not None else None
        m = self._in(mask)[0] if mask is not None else None
        tr = self._in(tradeoff)[0] if tradeoff is not None else None
        (kh, kw), (ph, pw), (dh, dw) = map(self._pair, (kernel, pad, dilate))
        N, Cin, H, W = self.ad.shape(x)
        Cout = self.ad.shape(w)[0]
        if self.ad.shape(w) != (Cout, Cin // num_group, kh, kw):
            raise ValueError("deformable_matching: bad weight shape %s" % (self.ad.shape(w),))
        if self.ad.shape(fl) != (N, 2, H, W):
            raise ValueError("deformable_matching: flow must be %s" % ((N, 2, H, W),))
        if m is not None and self.ad.shape(m) != (N, 1, H, W):
            raise ValueError("deformable_matching: mask must be %s" % ((N, 1, H, W),))
        if tr is not None and self.ad.shape(tr) != (N, Cout, H, W):
            raise ValueError("deformable_matching: tradeoff must be %s" % ((N, Cout, H, W),))
        out = self._out(out, x, (N, Cout, H, W), "deformable_matching")
        nbytes = self.ns.deform_conv_workspace_bytes(N, Cin, H, W, Cout, kh, kw, 1, 1, ph, pw, dh, dw, num_group, 1)
        ws = self._workspace(x, nbytes)
        if packed is not None:
            packed.require((N, Cin, H, W, Cout, kh, kw, 1, 1, ph, pw, dh, dw, num_group, 1))
        p = lambda a: self.ad.ptr(a) if a is not None else None
        self.check(self.ns.deform_conv_matching_fwd(
            self.ad.ptr(x), self.ad.ptr(fl), float(flow_scale), float(flow_stride), self.ad.ptr(w),
            self.ad.ptr(packed.buf) if packed is not None else None, packed.nbytes if packed is not None else 0,
            packed.tag if packed is not None else 0, p(b), p(m), p(tr), 1 if leaky else 0, self.ad.ptr(out), N, Cin, H, W,
            Cout, kh, kw, ph, pw, dh, dw, num_group, self.ad.ptr(ws), self.ad.nbytes(ws), self.ad.stream(x)))
        return out

    def _gate_args(self, what, raw, mask, shape=None):
        """(N, C, H, W) of the gate's tensors; mask must be (N,1,H,W)."""
        if self.ad.ndim(raw) != 4 or (shape is not None and self.ad.shape(raw) != shape):
            raise ValueError("%s: raw must be 4-D%s, got %s" % (what, "" if shape is None else " %s" % (shape,), self.ad.shape(raw)))
        N, C, H, W = self.ad.shape(raw)
        if mask is not None and self.ad.shape(mask) != (N, 1, H, W):
            raise ValueError("%s: mask must be %s" % (what, (N, 1, H, W)))
        return N, C, H, W

    def matching_gate(self, raw, mask=None, tradeoff=None, leaky=True, out=None):
        """MaskFlownet.py:231-233 on the deformable convolution's output: LeakyReLU(0.1)(raw * sigmoid(mask) + tradeoff); mask
        (N,1,H,W), tradeoff (N,C,H,W), both optional -- the training form of deformable_matching's epilogue (mfn_matching_gate_fwd),
        which keeps `raw` for the backward pass."""
        (r,) = self._in(raw)
        m = self._in(mask)[0] if mask is not None else None
        tr = self._in(tradeoff)[0] if tradeoff is not None else None
        N, C, H, W = self._gate_args("matching_gate", r, m)
        if tr is not None and self.ad.shape(tr) != (N, C, H, W):
            raise ValueError("matching_gate: tradeoff must be %s" % ((N, C, H, W),))
        out = self._out(out, r, (N, C, H, W), "matching_gate")
        p = lambda a: self.ad.ptr(a) if a is not None else None
        self.check(self.ns.matching_gate_fwd(self.ad.ptr(r), p(m), p(tr), 1 if leaky else 0, self.ad.ptr(out), N, C, H, W,
                                             self.ad.stream(r)))
        return out

    def matching_gate_backward(self, out_grad, output, raw, mask=None, leaky=True, out_grad2=None,
                               req=("write", "write", "write"), out=None):
        """Gradients of matching_gate w.r.t. (raw, mask, tradeoff) from the forward OUTPUT (mfn_matching_gate_bwd); out_grad2: a
        second upstream gradient, added to out_grad first.  The mask gradient's channel sum is added in a fixed order: the same
        bits on every call.  `raw` may be None when no mask gradient is asked for.  out: optional (graw, gmask, gtradeoff)
        buffers (required for req "add")."""
        what = "matching_gate_backward"
        go, y = self._in(out_grad, output)
        go2 = self._in(out_grad2)[0] if out_grad2 is not None else None
        m = self._in(mask)[0] if mask is not None else None
        r = self._in(raw)[0] if raw is not None else None
        N, C, H, W = self._gate_args(what, go, m)
        for name, a in (("output", y), ("raw", r), ("out_grad2", go2)):
            if a is not None and self.ad.shape(a) != (N, C, H, W):
                raise ValueError("%s: %s has shape %s, expected %s" % (what, name, self.ad.shape(a), (N, C, H, W)))
        rq = [_REQ[v] for v in req]
        if len(rq) != 3:
            raise ValueError("%s: req must be (raw, mask, tradeoff)" % what)
        if m is None:
            rq[1] = 0
        elif rq[1] and r is None:
            raise ValueError("%s: the mask gradient needs raw" % what)
        want = ((N, C, H, W), (N, 1, H, W), (N, C, H, W))
        given = tuple(out) if out is not None else (None, None, None)
        if len(given) != 3:
            raise ValueError("%s: out must be (graw, gmask, gtradeoff)" % what)
        grads = []
        for i, (g, shp) in enumerate(zip(given, want)):
            if not rq[i]:
                grads.append(None)
            elif g is None:
                if rq[i] == _REQ["add"]:
                    raise ValueError("%s: req 'add' needs the buffer to add into (out[%d])" % (what, i))
                grads.append(self.ad.empty(go, shp))
            else:
                self.ad.require_destination(g, go, what)   # written in place: no silent copy
                if self.ad.shape(g) != shp:
                    raise ValueError("%s: out[%d] has shape %s, expected %s" % (what, i, self.ad.shape(g), shp))
                grads.append(g)
        p = lambda a: self.ad.ptr(a) if a is not None else None
        nbytes = self.ns.matching_gate_bwd_workspace_bytes(N, C, H, W) if rq[1] else 0
        ws = self._workspace(go, nbytes) if nbytes else None
        self.check(self.ns.matching_gate_bwd(self.ad.ptr(go), p(go2), self.ad.ptr(y), p(r), p(m), 1 if leaky else 0, p(grads[0]),
                                             p(grads[1]), p(grads[2]), N, C, H, W, rq[0], rq[1], rq[2], p(ws),
                                             self.ad.nbytes(ws) if ws is not None else 0, self.ad.stream(go)))
        return tuple(grads)

    # ---- Convolution / Deconvolution (nn.Conv2D / nn.Conv2DTranspose of MaskFlownet.py:79-163) ----
    def conv_out_shape(self, H, W, kernel, stride=(1, 1), pad=(0, 0), dilate=(1, 1), transposed=False, adj=(0, 0)):
        (kh, kw), (sh, sw), (ph, pw), (dh, dw), (ah, aw) = map(self._pair, (kernel, stride, pad, dilate, adj))
        ho, wo = ctypes.c_int(), ctypes.c_int()
        self.check(self.ns.conv2d_out_shape(H, W, kh, kw, sh, sw, ph, pw, dh, dw, int(bool(transposed)), ah, aw,
                                            ctypes.byref(ho), ctypes.byref(wo)))
        return ho.value, wo.value

    def _conv(self, what, transposed, data, weight, bias, kernel, stride, dilate, pad, adj, num_filter, num_group, no_bias,
              out, activation, packed):
        if activation not in (None, "leaky"):
            raise ValueError("%s: activation must be None or 'leaky'" % what)
        if no_bias:
            bias = None
        elif bias is None:
            raise ValueError("%s: bias is required unless no_bias=True" % what)
        (w,) = self._in(weight)
        b = self._in(bias)[0] if bias is not None else None
        (kh, kw), (sh, sw), (ph, pw), (dh, dw), (ah, aw) = map(self._pair, (kernel, stride, pad, dilate, adj))
        if self.ad.ndim(data) != 4:
            raise ValueError("%s: data must be 4-D" % what)
        # `data` may be the channel suffix buf[:, c0:] of a concat buffer: dense per image, images further apart
        xst, xsh = self.ad.elem_strides(data), self.ad.shape(data)
        if xsh[0] > 1 and all(d <= 1 or a == e for d, a, e in zip(xsh[1:], xst[1:], (xsh[2] * xsh[3], xsh[3], 1))) \
                and xst[0] > xsh[1] * xsh[2] * xsh[3]:
            x, x_nstride = self.ad.prepare_strided(data), int(xst[0])
        else:
            (x,), x_nstride = self._in(data), 0
        N, Cin, H, W = self.ad.shape(x)
        g = int(num_group)
        if transposed:
            if self.ad.ndim(w) != 4 or self.ad.shape(w)[0] != Cin:
                raise ValueError("%s: weight shape %s, expected (%d, num_filter/num_group, %d, %d)" % (what, self.ad.shape(w), Cin, kh, kw))
            Cout = self.ad.shape(w)[1] * g
            want_w = (Cin, Cout // g, kh, kw)
        else:
            Cout = self.ad.shape(w)[0]
            want_w = (Cout, Cin // g, kh, kw)
        if num_filter is not None and int(num_filter) != Cout:
            raise ValueError("%s: num_filter=%s but weight has %d filters" % (what, num_filter, Cout))
        if Cin % g or Cout % g:
            raise ValueError("%s: channels must divide num_group" % what)
        if self.ad.shape(w) != want_w:
            raise ValueError("%s: weight shape %s, expected %s" % (what, self.ad.shape(w), want_w))
        if b is not None and self.ad.shape(b) != (Cout,):
            raise ValueError("%s: bias shape %s, expected (%d,)" % (what, self.ad.shape(b), Cout))
        Ho, Wo = self.conv_out_shape(H, W, (kh, kw), (sh, sw), (ph, pw), (dh, dw), transposed, (ah, aw))
        shape = (N, Cout, Ho, Wo)
        if out is None:
            out = self.ad.empty(x, shape)
            nstride = 0
        else:
            # `out` may be a channel slice of a concat buffer (x = concat(conv(x), x), MaskFlownet.py:219): dense per
            # image, images a whole (Ctot, h, w) apart
            if self.ad.shape(out) != shape:
                raise ValueError("%s: out has shape %s, expected %s" % (what, self.ad.shape(out), shape))
            st = self.ad.elem_strides(out)
            dense_img = all(d <= 1 or a == e for d, a, e in zip(shape[1:], st[1:], (Ho * Wo, Wo, 1)))
            if N * Cout * Ho * Wo != 0 and (not dense_img or (N > 1 and st[0] < Cout * Ho * Wo)):
                raise ValueError("%s: out must be contiguous or a channel slice buf[:, c0:c0+%d] of a contiguous NCHW "
                                 "buffer (strides %s)" % (what, Cout, st))
            nstride = int(st[0]) if N > 1 else 0
        dims = (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, g, int(bool(transposed)))
        p = lambda a: self.ad.ptr(a) if a is not None else None
        if packed is not None:
            packed.require(dims)
            # plain-layout weights = the generic or the few-filter kernel; the latter wants scratch for the partial sums of its
            # channel blocks on the coarse levels (0 bytes otherwise; the MFMA plans' figure is the re-layout they do not need)
            nbytes = self.ns.conv2d_workspace_bytes(*dims) if packed.tag == 0x4d43ffff00000000 else 0
            ws = self._workspace(x, nbytes) if nbytes else None
            self.check(self.ns.conv2d_fwd(p(x), x_nstride, None, self.ad.ptr(packed.buf), packed.nbytes, packed.tag, p(b),
                                          self.ad.ptr(out), nstride, *dims, ah, aw, 1 if activation == "leaky" else 0, p(ws),
                                          self.ad.nbytes(ws) if ws is not None else 0, self.ad.stream(x)))
            return out
        nbytes = self.ns.conv2d_workspace_bytes(*dims)
        ws = self._workspace(x, nbytes) if nbytes else None
        self.check(self.ns.conv2d_fwd(p(x), x_nstride, p(w), None, 0, 0, p(b), self.ad.ptr(out), nstride, *dims, ah, aw,
                                      1 if activation == "leaky" else 0, p(ws), self.ad.nbytes(ws) if ws is not None else 0,
                                      self.ad.stream(x)))
        return out

    def Convolution(self, data, weight, bias=None, kernel=(3, 3), stride=(1, 1), dilate=(1, 1), pad=(0, 0), num_filter=None,
                    num_group=1, no_bias=False, layout="NCHW", out=None, activation=None, packed=None):
        """MXNet Convolution (2-D, NCHW).  activation='leaky': the LeakyReLU(0.1) every conv() of the reference is followed
        by (MaskFlownet.py:165-173), fused; out: optional destination, e.g. a channel slice of a concat buffer."""
        if layout not in (None, "NCHW"):
            raise ValueError("Convolution: only layout='NCHW' is supported")
        return self._conv("Convolution", False, data, weight, bias, kernel, stride, dilate, pad, (0, 0), num_filter, num_group,
                          no_bias, out, activation, packed)

    def Deconvolution(self, data, weight, bias=None, kernel=(4, 4), stride=(2, 2), dilate=(1, 1), pad=(1, 1), adj=(0, 0),
                      num_filter=None, num_group=1, no_bias=False, layout="NCHW", out=None, activation=None, packed=None):
        """MXNet Deconvolution (2-D, NCHW; weight (Cin, num_filter/num_group, kh, kw)) -- nn.Conv2DTranspose of deconv(),
        MaskFlownet.py:175-183."""
        if layout not in (None, "NCHW"):
            raise ValueError("Deconvolution: only layout='NCHW' is supported")
        return self._conv("Deconvolution", True, data, weight, bias, kernel, stride, dilate, pad, adj, num_filter, num_group,
                          no_bias, out, activation, packed)

    def _pack_buffer(self, like, nbytes, dims, out, what):
        """Where a pack entry writes: a fresh buffer, or the one of `out`, which must have been laid out for the same dims."""
        if out is None:
            return self.ad.empty_bytes(like, nbytes)
        if not isinstance(out, PackedDeformWeights):
            raise TypeError("%s: out must be a PackedDeformWeights, got %r" % (what, type(out)))
        out.require(dims)
        if out.nbytes != int(nbytes):
            raise ValueError("%s: out holds %d bytes, this layout takes %d (tuning changed since it was packed)" % (what, out.nbytes, nbytes))
        return out.buf

    def pack_conv_weights(self, weight, data_shape, kernel=(3, 3), stride=(1, 1), dilate=(1, 1), pad=(0, 0), num_group=1,
                          transposed=False, out=None):
        """Lay constant Convolution / Deconvolution weights out once for inputs of `data_shape` (mfn_conv2d_pack_weights).  out: as
        pack_deform_weights."""
        (w,) = self._in(weight)
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = map(self._pair, (kernel, stride, pad, dilate))
        N, Cin, H, W = (int(v) for v in data_shape)
        g = int(num_group)
        Cout = self.ad.shape(w)[1] * g if transposed else self.ad.shape(w)[0]
        dims = (N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, g, int(bool(transposed)))
        nbytes = self.ns.conv2d_packed_weight_bytes(*dims)
        if not nbytes:
            raise ValueError("pack_conv_weights: bad shape %s" % (dims,))
        buf = self._pack_buffer(w, nbytes, dims, out, "pack_conv_weights")
        tag = ctypes.c_ulonglong()
        self.check(self.ns.conv2d_pack_weights(self.ad.ptr(w), *dims, self.ad.ptr(buf), nbytes, ctypes.byref(tag),
                                               self.ad.stream(w)))
        return PackedDeformWeights(buf, nbytes, dims, tag.value)

    def offsets_from_flow(self, flow, scale, stride, taps=9, out=None):
        (fl,) = self._in(flow)
        N, two, H, W = self.ad.shape(fl)
        if two != 2:
            raise ValueError("offsets_from_flow: flow must be (N,2,H,W)")
        out = self._out(out, fl, (N, 2 * taps, H, W), "offsets_from_flow")
        self.check(self.ns.offsets_from_flow(self.ad.ptr(fl), self.ad.ptr(out), N, H, W, int(taps), float(scale),
                                             float(stride), self.ad.stream(fl)))
        return out


class PackedDeformWeights:
    """Opaque device buffer made by OpSet.pack_deform_weights for one (shape, hyper-parameter) tuple."""

    def __init__(self, buf, nbytes, dims, tag):
        self.buf, self.nbytes, self.dims, self.tag = buf, int(nbytes), tuple(dims), int(tag)

    def require(self, dims):
        if tuple(int(d) for d in dims) != self.dims:
            raise ValueError("packed DeformableConvolution weights were laid out for %s, called with %s"
                             % (self.dims, tuple(dims)))


class AdamTable:
    """Opaque device buffer made by OpSet.multi_adam_table: the tensors' addresses and counts, the launch's blocks, the layout tag."""

    def __init__(self, buf, nbytes, tag, n_tensors, n_blocks, ptrs, counts):
        self.buf, self.nbytes, self.tag, self.n_tensors, self.n_blocks = buf, int(nbytes), int(tag), int(n_tensors), int(n_blocks)
        self.ptrs, self.counts = tuple(ptrs), tuple(counts)

    def stale(self, ptrs):
        """Whether any of these (weight, grad, mean, var) address rows differs from the ones the table was built from."""
        return tuple(tuple(r) for r in ptrs) != self.ptrs


class BatchRows:
    """Opaque device table made by OpSet.batch_gather_rows: one 64-byte row per batch slot and the tag that binds it to (N, Hc, Wc).
    It holds addresses: `samples` keeps the sources alive as long as the table is.  `origins` and `flips` are the host's copy of what the
    rows say: the validate ops check a window of the table against them before any launch."""
    ROW_BYTES = 64

    def __init__(self, buf, nbytes, tag, N, crop_shape, samples, origins=(), flips=()):
        self.buf, self.nbytes, self.tag, self.N, self.crop_shape = buf, int(nbytes), int(tag), int(N), tuple(crop_shape)
        self.samples = list(samples)
        self.origins, self.flips = [(int(o[0]), int(o[1])) for o in origins], [int(f) for f in flips]


class IngestTables:
    """Opaque device tables made by OpSet.ingest_tables: 32 bytes per destination column and row, and the tag that binds them to the
    window size and the destination size."""

    def __init__(self, buf, nbytes, tag, src_hw, dst_hw):
        self.buf, self.nbytes, self.tag, self.src_hw, self.dst_hw = buf, int(nbytes), int(tag), tuple(src_hw), tuple(dst_hw)


class TorchAdapter:
    """torch-ROCm tensors as device buffers; launches go to torch's current stream."""

    def __init__(self):
        import torch
        self.torch = torch

    def prepare(self, a):
        t = self.torch
        if not isinstance(a, t.Tensor):
            raise TypeError("expected a torch.Tensor on a ROCm device, got %r" % type(a))
        if not a.is_cuda:
            raise RuntimeError("maskflownet_amd ops run on the MI355X only: tensor is on %s (there is no CPU "
                               "fallback)" % a.device)
        if a.dtype != t.float32:
            raise TypeError("float32 expected, got %s" % a.dtype)
        return a if a.is_contiguous() else a.contiguous()

    def require_destination(self, out, like, what):
        t = self.torch
        if not isinstance(out, t.Tensor) or out.dtype != t.float32:
            raise TypeError("%s: out must be a float32 torch.Tensor" % what)
        if out.device != like.device:
            raise RuntimeError("%s: out lives on %s, the inputs on %s" % (what, out.device, like.device))
        if not out.is_contiguous():
            raise ValueError("%s: out must be contiguous (strides %s)" % (what, tuple(out.stride())))

    def prepare_strided(self, a):
        """A float32 device tensor used in place through its strides (no .contiguous() copy)."""
        t = self.torch
        if not isinstance(a, t.Tensor) or not a.is_cuda or a.dtype != t.float32:
            raise TypeError("expected a float32 torch.Tensor on a ROCm device")
        return a

    def ptr(self, a):
        return a.data_ptr()

    def shape(self, a):
        return tuple(a.shape)

    def ndim(self, a):
        return a.dim()

    def elem_strides(self, a):
        return tuple(a.stride())

    def empty(self, like, shape):
        return self.torch.empty(shape, dtype=self.torch.float32, device=like.device)

    def empty_bytes(self, like, nbytes):
        return self.torch.empty((int(nbytes) + 3) // 4, dtype=self.torch.float32, device=like.device)

    def nbytes(self, a):
        return a.numel() * a.element_size()

    def device_key(self, a):
        return (a.device.index, self.torch.cuda.current_stream(a.device).cuda_stream)

    def stream(self, a):
        return self.torch.cuda.current_stream(a.device).cuda_stream


_default = None


def default_ops():
    """The product OpSet: libmfn_hip.so + torch tensors.  Raises if the library is not built."""
    global _default
    if _default is None:
        _default = OpSet(_lib.lib(), TorchAdapter(), _lib.check)
    return _default


def Correlation(*a, **k):
    return default_ops().Correlation(*a, **k)


def GridGenerator(*a, **k):
    return default_ops().GridGenerator(*a, **k)


def BilinearSampler(*a, **k):
    return default_ops().BilinearSampler(*a, **k)


def DeformableConvolution(*a, **k):
    return default_ops().DeformableConvolution(*a, **k)


def warp(*a, **k):
    return default_ops().warp(*a, **k)


def deformable_convolution_shared(*a, **k):
    return default_ops().deformable_convolution_shared(*a, **k)


def matching_gate(*a, **k):
    return default_ops().matching_gate(*a, **k)


def matching_gate_backward(*a, **k):
    return default_ops().matching_gate_backward(*a, **k)


def offsets_from_flow(*a, **k):
    return default_ops().offsets_from_flow(*a, **k)


def offsets_from_flow_backward(*a, **k):
    return default_ops().offsets_from_flow_backward(*a, **k)


def deformable_convolution_shared_backward(*a, **k):
    return default_ops().deformable_convolution_shared_backward(*a, **k)


def Upsample(*a, **k):
    return default_ops().Upsample(*a, **k)


def bilinear_resize(*a, **k):
    return default_ops().bilinear_resize(*a, **k)


def pair_mean(*a, **k):
    return default_ops().pair_mean(*a, **k)


def preprocess_pair(*a, **k):
    return default_ops().preprocess_pair(*a, **k)


def flow_metric_sums(*a, **k):
    return default_ops().flow_metric_sums(*a, **k)


def flow_metrics(*a, **k):
    return default_ops().flow_metrics(*a, **k)


def augment_geometry(*a, **k):
    return default_ops().augment_geometry(*a, **k)


def augment_color_mean(*a, **k):
    return default_ops().augment_color_mean(*a, **k)


def augment_color(*a, **k):
    return default_ops().augment_color(*a, **k)


def multiscale_epe(*a, **k):
    return default_ops().multiscale_epe(*a, **k)


def multiscale_epe_backward(*a, **k):
    return default_ops().multiscale_epe_backward(*a, **k)


def adam_update(*a, **k):
    return default_ops().adam_update(*a, **k)


def multi_adam_table(*a, **k):
    return default_ops().multi_adam_table(*a, **k)


def multi_adam_update(*a, **k):
    return default_ops().multi_adam_update(*a, **k)


def batch_gather_rows(*a, **k):
    return default_ops().batch_gather_rows(*a, **k)


def batch_gather(*a, **k):
    return default_ops().batch_gather(*a, **k)


def val_pair_mean(*a, **k):
    return default_ops().val_pair_mean(*a, **k)


def val_preprocess(*a, **k):
    return default_ops().val_preprocess(*a, **k)


def val_flow_metric_sums(*a, **k):
    return default_ops().val_flow_metric_sums(*a, **k)


def ingest_tables(*a, **k):
    return default_ops().ingest_tables(*a, **k)


def ingest_minmax(*a, **k):
    return default_ops().ingest_minmax(*a, **k)


def ingest_image(*a, **k):
    return default_ops().ingest_image(*a, **k)


def ingest_flow_occ(*a, **k):
    return default_ops().ingest_flow_occ(*a, **k)


def cv_resize_u8(*a, **k):
    return default_ops().cv_resize_u8(*a, **k)


def pair_mean_u8(*a, **k):
    return default_ops().pair_mean_u8(*a, **k)


def preprocess_pair_u8(*a, **k):
    return default_ops().preprocess_pair_u8(*a, **k)


def flow_color(*a, **k):
    return default_ops().flow_color(*a, **k)


def Convolution(*a, **k):
    return default_ops().Convolution(*a, **k)


def Deconvolution(*a, **k):
    return default_ops().Deconvolution(*a, **k)
