"""The training step of MaskFlownet-S with EVERY layer's forward and backward on libmfn_hip.so.

Caller of the hot path on the training side: /root/reference/network/pipeline.py:89-114 (`train_batch`: forward under
autograd, `MultiscaleEpe` loss, `loss.backward()`, `trainer.step`) over /root/reference/network/MaskFlownet.py:197-315
(`MaskFlownet_S.hybrid_forward`).  MXNet's autograd is torch's here (device memory, tape and the optimizer are plumbing);
what the tape calls is the library:

* convolutions / transposed convolutions with their fused LeakyReLU: `mfn_conv2d_fwd` / `mfn_conv2d_bwd` (`_ConvFn`),
* cost volumes, the deformable matching step, `Upsample`: the autograd functions of `layer.py`
  (`mfn_correlation_fwd/_bwd`, `mfn_deform_conv_shared_fwd/_bwd`, `mfn_upsample_fwd/_bwd`),
* concatenation and the composed loss's arithmetic: torch element-wise glue, as the reference's are MXNet's.  So is, by default,
  the gating `warp * sigmoid(mask) + tradeoff` with its LeakyReLU; `LibraryBackend(fused_matching=True)` runs a level's whole
  matching step -- deformable convolution, gate, cost volume and its activation -- as one autograd function on the library
  (`layer.matching_level`: `mfn_matching_gate_fwd/_bwd` between the kernels above) and keeps the LeakyReLU of the cost volumes
  that stand alone in their epilogue: no torch leaky_relu kernel is left in a step, and of torch's sigmoid only the occlusion
  masks the networks hand out (`MaskFlownet.py:303-305`, `:309`), which are no part of a matching step.

`network.MaskFlownetS` is the inference form of the same graph (pre-allocated concat buffers, packed weights, one
hipGraph); the parameter names are shared (`network.random_params`, the reference checkpoint's keys).
"""
import numpy as np
import torch
from torch import nn

from . import layer, ops
from .network import CONTEXT, DECODER, MD, PYRAMID, SCALE, STRIDES, UPFEAT


class _ConvFn(torch.autograd.Function):
    """Convolution / Deconvolution + bias [+ LeakyReLU(0.1)] in one launch; backward through mfn_conv2d_bwd (which undoes the
    fused activation from the saved output)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, dilation, act, transposed):
        o = ops.default_ops()
        x = x.contiguous()
        if transposed:
            y = o.Deconvolution(x, w, b, kernel=(4, 4), stride=(2, 2), pad=(1, 1), activation="leaky" if act else None)
        else:
            y = o.Convolution(x, w, b, kernel=(3, 3), stride=(stride, stride), dilate=(dilation, dilation),
                              pad=(dilation, dilation), activation="leaky" if act else None)
        ctx.save_for_backward(x, w, y)
        ctx.cfg = (stride, dilation, act, transposed)
        return y

    @staticmethod
    def backward(ctx, gout):
        x, w, y = ctx.saved_tensors
        stride, dilation, act, transposed = ctx.cfg
        o = ops.default_ops()
        need = ctx.needs_input_grad
        req = tuple("write" if need[i] else "null" for i in range(3))
        gout = gout.contiguous()
        if transposed:
            gx, gw, gb = o.Deconvolution_backward(gout, x, w, output=y, kernel=(4, 4), stride=(2, 2), pad=(1, 1),
                                                  activation="leaky" if act else None, req=req)
        else:
            gx, gw, gb = o.Convolution_backward(gout, x, w, output=y, kernel=(3, 3), stride=(stride, stride),
                                                dilate=(dilation, dilation), pad=(dilation, dilation),
                                                activation="leaky" if act else None, req=req)
        return gx, gw, gb, None, None, None, None


class LibraryBackend:
    """The differentiable layer set of the network, every member's forward AND backward a libmfn_hip.so call.  (The tests pass
    a pure-torch implementation of the same four members to check the gradients of the composition.)
    fused_matching=True (opt-in; the default waits for the measurement cited in DESIGN.md 4.4): the backend also has
    matching_level -- a pyramid level's matching step as one differentiable call, layer.matching_level --, which the networks
    use where a backend offers it, and its correlation keeps the LeakyReLU in the kernel's epilogue under autograd too."""

    def __init__(self, fused_matching=False):
        self._up = {}
        self.fused_matching = bool(fused_matching)
        if self.fused_matching:      # members of the instance: a backend without the flag has none of them
            self.matching_level = self._matching_level
            self.correlation = self._leaky_correlation

    def conv(self, x, w, b, stride=1, dilation=1, act=True, transposed=False):
        return _ConvFn.apply(x, w, b, stride, dilation, act, transposed)

    def correlation(self, a, b, md):     # MaskFlownet.py:193-195 + the LeakyReLU around every call (:217)
        return layer.correlation(a.contiguous(), b.contiguous(), md, leaky=True)

    def deform(self, x, flow, w, b, scale, stride):   # MaskFlownet.py:230: deform(x, repeat9(flow * scale / stride))
        return layer._SharedDeformConvFn.apply(x.contiguous(), flow.contiguous(), w, b, scale, stride,
                                               {"kernel": (3, 3), "dilate": (1, 1), "pad": (1, 1), "num_group": 1}, None)

    def _matching_level(self, c1, c2, flow, w, b, scale, stride, md, mask=None, tradeoff=None):
        """MaskFlownet.py:230-236 (gated) / :460-463 (the cascade: the LeakyReLU alone) -> (corr, warp)."""
        return layer.matching_level(c1, c2, flow, w, b, mask, tradeoff, scale, stride, md)

    def _leaky_correlation(self, a, b, md):
        if layer._any_grad(a, b):
            return layer._LeakyCorrelationFn.apply(a.contiguous(), b.contiguous(), md)
        return layer.correlation(a.contiguous(), b.contiguous(), md, leaky=True)

    def upsample(self, x, factor):
        if factor not in self._up:
            self._up[factor] = layer.Upsample(factor)
        return self._up[factor](x.contiguous())

    def warp(self, x, flow):             # layer.py:14-18 (Reconstruction2D); only ever called on the frozen head's outputs
        return ops.warp(x.contiguous(), flow.contiguous(), clip_grid=False)


def _key(name):
    return name.replace(".", "__")


class MaskFlownetSTrainable(nn.Module):
    """MaskFlownet_S.hybrid_forward (MaskFlownet.py:197-315) as a differentiable module on the library.
    forward(im1, im2) -> ([flow6 .. flow2] x scale, [sigmoid(mask2)]) = the reference's (predictions, occlusion_masks)."""

    def __init__(self, params, backend=None, dtype=torch.float32):
        super().__init__()
        self.P = nn.ParameterDict({_key(k): nn.Parameter(torch.as_tensor(np.ascontiguousarray(v)).to(dtype))
                                   for k, v in params.items()})
        self.B = backend if backend is not None else LibraryBackend()

    def _p(self, name):
        return self.P[_key(name + ".weight")], self.P[_key(name + ".bias")]

    def conv(self, name, x, stride=1, dilation=1, act=True, transposed=False):
        w, b = self._p(name)
        return self.B.conv(x, w, b, stride, dilation, act, transposed)

    def forward(self, im1, im2):
        r = self.run(im1, im2)
        return r["predictions"], [r["occlusion"]]

    def run(self, im1, im2):
        """forward() with what MaskFlownet_S hands to the cascade (`srcs`, MaskFlownet.py:305-314) kept: the pyramid c[l] (both
        images as one batch), the flows per level (network units) and mask2."""
        N = im1.shape[0]
        x = torch.cat([im1, im2], 0)
        c = {}
        for l in range(1, 7):                        # both images as one batch through the shared pyramid
            for k, s in (("a", 2), ("b", 1), ("c", 1)):
                x = self.conv("conv%d%s" % (l, k), x, stride=s)
            c[l] = x
        preds, flows = [], {}
        flow = mask = feat = None
        level = getattr(self.B, "matching_level", None)      # LibraryBackend(fused_matching=True): the matching step in one call
        for l in (6, 5, 4, 3, 2):
            c1, c2 = c[l][:N], c[l][N:]
            if l == 6:
                x = self.B.correlation(c1, c2, MD)
            else:
                flow_up, mask_up = self.B.upsample(flow, 2), self.B.upsample(mask, 2)
                trade = self.conv("conv%df" % l, feat, act=False)
                w, b = self._p("deform%d" % l)
                # MaskFlownet.py:230-233: deform(c2, repeat9(flow * scale / stride)) * sigmoid(mask) + tradeoff, LeakyReLU
                if level is not None:
                    corr, _ = level(c1, c2, flow_up, w, b, SCALE, float(STRIDES[l]), MD, mask=mask_up, tradeoff=trade)
                else:
                    warp = self.B.deform(c2, flow_up, w, b, SCALE, float(STRIDES[l]))
                    warp = torch.nn.functional.leaky_relu(warp * torch.sigmoid(mask_up) + trade, 0.1)
                    corr = self.B.correlation(c1, warp, MD)
                x = torch.cat([corr, c1, feat, flow_up], 1)
            for k in range(len(DECODER)):            # x = concat(conv(x), x)
                x = torch.cat([self.conv("conv%d_%d" % (l, k), x), x], 1)
            if l > 2:
                d = torch.cat([self.conv("pred_flow%d" % l, x, act=False), self.conv("pred_mask%d" % l, x, act=False)], 1)
            else:
                d = self.conv("pred_flow2", x, act=False)
            flow = d[:, :2].contiguous() if l == 6 else flow_up + d[:, :2]
            if l > 2:
                mask = d[:, 2:3].contiguous()
                feat = self.conv("upfeat%d" % (l - 1), x, transposed=True)
                preds.append(flow)
                flows[l] = flow
        y = x
        for i, (_, dil) in enumerate(CONTEXT):
            y = self.conv("dc_conv%d" % (i + 1), y, dilation=dil)
        flow = flow + self.conv("dc_conv7", y, act=False)
        preds.append(flow)
        flows[2] = flow
        return {"predictions": [f * SCALE for f in preds], "occlusion": torch.sigmoid(mask_up),      # MaskFlownet.py:303-305
                "c": c, "flows": flows, "mask2": mask_up}


class MaskFlownetTrainable(nn.Module):
    """The full MaskFlownet (MaskFlownet.hybrid_forward, MaskFlownet.py:436-545) for its training stage: the S head frozen
    (`fix_head`, :413-415, main.py:139) and run without a tape, the cascade -- second pyramid over (image 1 | 0) and (warped image 2 |
    occlusion mask - 0.5), per level a deformable warp by the cascade's own flow, two md = 2 cost volumes, decoder, flow head, the
    context network -- differentiable on the library.  `params`: the head under 'MaskFlownet_S.<block>', the cascade under '<block>'.
    forward -> ([gflow6 .. gflow2] x scale, [the head's occlusion mask])."""

    def __init__(self, params, backend=None, dtype=torch.float32):
        super().__init__()
        from .network import HEAD
        self.B = backend if backend is not None else LibraryBackend()
        self.head = MaskFlownetSTrainable({k[len(HEAD):]: v for k, v in params.items() if k.startswith(HEAD)}, self.B, dtype)
        for q in self.head.parameters():
            q.requires_grad_(False)
        self.P = nn.ParameterDict({_key(k): nn.Parameter(torch.as_tensor(np.ascontiguousarray(v)).to(dtype))
                                   for k, v in params.items() if not k.startswith(HEAD)})

    def conv(self, name, x, stride=1, dilation=1, act=True, transposed=False):
        return self.B.conv(x, self.P[_key(name + ".weight")], self.P[_key(name + ".bias")], stride, dilation, act, transposed)

    def forward(self, im1, im2):
        from .network import MD_CASCADE
        N = im1.shape[0]
        with torch.no_grad():
            h = self.head.run(im1, im2)
            warped = self.B.warp(im2, self.B.upsample(h["flows"][2], 4) * SCALE)                       # :311
            mask0 = torch.sigmoid(self.B.upsample(h["mask2"], 4)) - 0.5                                 # :309-310
            x = torch.cat([torch.cat([im1, torch.zeros_like(mask0)], 1), torch.cat([warped, mask0], 1)], 0)   # c30, c40 (:312-313)
        d = {}
        for l in range(1, 7):                        # the second pyramid, both 4-channel inputs as one batch
            for k, s in (("x", 2), ("y", 1), ("z", 1)):
                x = self.conv("conv%d%s" % (l, k), x, stride=s)
            d[l] = x
        preds = []
        flow = feat = None
        level = getattr(self.B, "matching_level", None)
        for l in (6, 5, 4, 3, 2):
            c1 = h["c"][l][:N]
            c2 = c1 if l in (2, 3) else h["c"][l][N:]          # c2s = [c21, c12, c13, c24, c25, c26] (:307)
            c3, c4 = d[l][:N], d[l][N:]
            flow_in = h["flows"][6] if l == 6 else self.B.upsample(flow, 2)                              # :457
            w, b = self.P[_key("deform%d.weight" % l)], self.P[_key("deform%d.bias" % l)]
            if level is not None:                # no mask, no trade-off: the gate is the LeakyReLU alone
                cu, _ = level(c1, c2, flow_in, w, b, SCALE, float(STRIDES[l]), MD_CASCADE)
            else:
                warp = torch.nn.functional.leaky_relu(self.B.deform(c2, flow_in, w, b, SCALE, float(STRIDES[l])), 0.1)   # :460-461
                cu = self.B.correlation(c1, warp, MD_CASCADE)
            cv = self.B.correlation(c3, c4, MD_CASCADE)
            x = torch.cat([cu, cv, flow_in], 1) if l == 6 else torch.cat([c1, feat, cu, cv, flow_in, h["flows"][l]], 1)   # :466, :480
            for k in range(len(DECODER)):
                x = torch.cat([self.conv("conv%d_%d" % (l, k), x), x], 1)
            flow = flow_in + self.conv("pred_flow%d" % l, x, act=False)
            if l > 2:
                feat = self.conv("upfeat%d" % (l - 1), x, transposed=True)
                preds.append(flow)
        y = x
        for i, (_, dil) in enumerate(CONTEXT):
            y = self.conv("dc_conv%d" % (i + 1), y, dilation=dil)
        flow = flow + self.conv("dc_conv7", y, act=False)
        preds.append(flow)
        return [f * SCALE for f in preds], [h["occlusion"]]


class MultiscaleEpe(nn.Module):
    """MaskFlownet.py:585-611 with match='upsampling' (pipeline.py:42-44): sum_s w_s * EpeLossWithMask(Upsample(s)(pred_s) ,
    label, mask); EpeLossWithMask (:563-583) = sum(sqrt(sum_c (p - l)^2 + eps) * mask) / sum(mask) per sample, or with q (the
    `optimizer.q` of the Sintel / KITTI schedules, :577-578) sum((sum_c |p - l| + eps)^q * mask) / sum(mask).
    `label` in pixels, as the predictions (flow x scale).  Composed from Upsample and torch element-wise kernels: the torch twin
    of FusedMultiscaleEpe."""

    def __init__(self, scales=(64, 32, 16, 8, 4), weights=(.005, .01, .02, .08, .32), eps=1e-8, backend=None, q=None):
        super().__init__()
        self.scales, self.weights, self.eps = tuple(scales), tuple(weights), float(eps)
        self.q = None if q is None else float(q)
        self.B = backend if backend is not None else LibraryBackend()

    def forward(self, label, mask, *preds):
        total = 0.
        for p, w, s in zip(preds, self.weights, self.scales):
            if self.q is None:
                e = torch.sqrt(((self.B.upsample(p, s) - label) ** 2).sum(1) + self.eps) * mask[:, 0]
            else:
                e = ((self.B.upsample(p, s) - label).abs().sum(1) + self.eps) ** self.q * mask[:, 0]
            total = total + w * e.flatten(1).sum(1) / mask.flatten(1).sum(1)
        return total


class _FusedEpeFn(torch.autograd.Function):
    """mfn_multiscale_epe_fwd / _bwd: nothing but the predictions, label, mask and the (N, S+1) sums is kept for backward."""

    @staticmethod
    def forward(ctx, label, mask, cfg, *preds):
        scales, weights, eps, q = cfg
        preds = tuple(p.contiguous() for p in preds)
        loss, sums = ops.multiscale_epe(preds, label, mask, scales, weights, eps, q)
        ctx.save_for_backward(label, mask, sums, *preds)
        ctx.cfg = cfg
        return loss

    @staticmethod
    def backward(ctx, gloss):
        label, mask, sums, *preds = ctx.saved_tensors
        scales, weights, eps, q = ctx.cfg
        reqs = ["write" if need else "null" for need in ctx.needs_input_grad[3:]]
        gp = ops.multiscale_epe_backward(gloss.contiguous(), preds, label, mask, scales, weights, sums, eps, q, reqs=reqs)
        return (None, None, None) + tuple(gp)


class FusedMultiscaleEpe(nn.Module):
    """MultiscaleEpe on the library's fused kernels (kernels/loss.h): the same defaults, call `(label, mask, *preds)`, per-sample
    return value and `.scales`; forward is two launches, backward one per scale, and no full-resolution tensor is written or kept.
    q=None: the sqrt form; q (0.4 in the Sintel / KITTI schedules): the robust form.  Gradients reach the predictions only."""

    def __init__(self, scales=(64, 32, 16, 8, 4), weights=(.005, .01, .02, .08, .32), eps=1e-8, q=None):
        super().__init__()
        self.scales, self.weights, self.eps = tuple(scales), tuple(weights), float(eps)
        self.q = None if q is None else float(q)

    def forward(self, label, mask, *preds):
        n = len(preds)
        return _FusedEpeFn.apply(label, mask, (self.scales[:n], self.weights[:n], self.eps, self.q), *preds)


class GradientBuckets:
    """The training step's gradient exchange (/root/reference/network/pipeline.py:27 kvstore='device', :95 batch
    shards, :114 `trainer.step(batch_size)`): every parameter gradient of the network (142 tensors, 42.06 MB for MaskFlownet-S)
    lives in one of `n_buckets` flat fp32 buffers -- `p.grad` is a VIEW into its bucket, autograd accumulates in place -- laid
    out in REVERSE registration order, which is roughly the order backward completes them (context network and decoders first,
    the image pyramid last).  A post-accumulate hook per parameter counts its bucket down; the bucket whose last gradient
    arrives is all-reduced (sum) at once with async_op=True, so the collective of the decoders' gradients travels over
    RCCL / xGMI while backward is still in the pyramid.  finish() waits for the handles and applies 1 / global_batch.
    Four buckets of ~10.5 MB: large enough for xGMI's per-link bandwidth, few enough launches, early enough first launch.
    Without a process group (or world 1) only the 1 / global_batch remains.
    align: every view starts on a multiple of `align` elements of its bucket (4 = 16 bytes, what Trainer's kernel wants for its
    16-byte accesses; the padding stays zero and travels with the bucket).  1 packs the views back to back."""

    def __init__(self, params, n_buckets=4, dist=None, align=1):
        params = [p for p in params if p.requires_grad]
        self.dist = dist if (dist is not None and dist.is_initialized() and dist.get_world_size() > 1) else None
        order = list(reversed(params))
        total = sum(p.numel() for p in order)
        target = (total + n_buckets - 1) // max(1, n_buckets)
        groups, cur, size = [], [], 0
        for p in order:
            cur.append(p)
            size += p.numel()
            if size >= target and len(groups) < n_buckets - 1:
                groups.append(cur)
                cur, size = [], 0
        if cur:
            groups.append(cur)
        align = max(1, int(align))
        pad = lambda n: (n + align - 1) // align * align
        self.buckets, self.members, self._of, self._hooks = [], groups, {}, []
        self.offsets = []        # per bucket: the element offset of each member's view
        for bi, grp in enumerate(groups):
            flat = torch.zeros(sum(pad(p.numel()) for p in grp), dtype=grp[0].dtype, device=grp[0].device)
            off, offs = 0, []
            for p in grp:
                p.grad = flat[off:off + p.numel()].view_as(p)
                offs.append(off)
                off += pad(p.numel())
                self._of[p] = bi
                self._hooks.append(p.register_post_accumulate_grad_hook(self._arrived))
            self.buckets.append(flat)
            self.offsets.append(offs)
        self._left = [len(g) for g in groups]
        self._handles = []
        self.launch_order = []   # bucket indices in the order their all-reduce was launched by the last backward (tests read it)

    def zero(self):
        """Before a step's backward (instead of opt.zero_grad(set_to_none=True), which would drop the views)."""
        for b in self.buckets:
            b.zero_()
        self._left = [len(g) for g in self.members]
        self._handles, self.launch_order = [], []

    def _arrived(self, p):
        bi = self._of[p]
        b = self.buckets[bi]
        if p.grad is None or not (b.data_ptr() <= p.grad.data_ptr() < b.data_ptr() + b.numel() * b.element_size()):
            raise RuntimeError("a parameter's .grad no longer views its gradient bucket (zero the buckets with GradientBuckets.zero())")
        self._left[bi] -= 1
        if self._left[bi] == 0:
            self.launch_order.append(bi)
            if self.dist is not None:
                self._handles.append(self.dist.all_reduce(self.buckets[bi], op=self.dist.ReduceOp.SUM, async_op=True))

    def finish(self, global_batch=None, scale=True):
        """Behind backward: every bucket reduced (whatever arrived late is launched now), then trainer.step's 1 / batch_size.
        scale=False leaves the sums as they are: Trainer hands 1 / batch_size to its kernel as rescale_grad instead."""
        for bi, left in enumerate(self._left):
            if left > 0:   # parameters that took no gradient this step (frozen branches): their bucket still has to travel
                self._left[bi] = 0
                self.launch_order.append(bi)
                if self.dist is not None:
                    self._handles.append(self.dist.all_reduce(self.buckets[bi], op=self.dist.ReduceOp.SUM, async_op=True))
        for h in self._handles:
            h.wait()
        self._handles = []
        if scale:
            for b in self.buckets:
                b.mul_(1.0 / float(global_batch))

    def nbytes(self):
        return sum(b.numel() * b.element_size() for b in self.buckets)


def reference_named_parameters(net):
    """[(the reference's parameter name, parameter)] of a module in registration order: the trainable networks keep 'conv1a.weight'
    as P['conv1a__weight'] and the frozen head of the full model under `head` ('MaskFlownet_S.conv1a.weight'); any other module's
    names are taken as they are (layer.DeformableConv2D: 'weight', 'bias')."""
    from .network import HEAD
    if isinstance(net, MaskFlownetTrainable):
        return [(HEAD + k, p) for k, p in reference_named_parameters(net.head)] + [(k.replace("__", "."), p) for k, p in net.P.items()]
    if isinstance(net, MaskFlownetSTrainable):
        return [(k.replace("__", "."), p) for k, p in net.P.items()]
    return list(net.named_parameters())


def learning_rate_at(schedule, steps):
    """pipeline.py:65-75: the learning rate of the first entry [boundary, lr] of the schedule (config.optimizer.learning_rate) that
    `steps` has not passed -- `steps > boundary` moves on, so a boundary step still trains at its own entry's rate --, or None past
    the last entry (the reference's set_learning_rate returns False there and the run ends)."""
    i = 0
    while i < len(schedule) and steps > schedule[i][0]:
        i += 1
    return float(schedule[i][1]) if i < len(schedule) else None


_ADAM_DEFAULTS = {"learning_rate": 0.001, "beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8, "wd": 0.0, "clip_gradient": None}
_STATE_KEY = "trainer:adam"      # the float64 array of save_states: num_update, then the hyper-parameters in this order
_STATE_FIELDS = ("num_update", "learning_rate", "beta1", "beta2", "epsilon", "wd", "clip_gradient")


class Trainer:
    """gluon.Trainer(params, 'adam', {'learning_rate': 1e-4}) of pipeline.py:27 with MXNet's arithmetic, the whole step one launch of
    mfn_multi_adam_update (kernels/optimizer.h).  named_params: {name: parameter} or (name, parameter) pairs, the names the
    reference's (reference_named_parameters); only parameters with requires_grad are taken -- `fix_head` (main.py:139): a frozen
    head and its would-be state are never touched.  optimizer_params: learning_rate, beta1 (0.9), beta2 (0.999), epsilon (1e-8),
    wd (0), clip_gradient (None), MXNet's names and defaults; lr_mult / wd_mult: {name: factor}, default 1.
    The trainer owns a GradientBuckets(align=4) over its parameters (`.buckets`: p.grad is a view, zero them with buckets.zero())
    and flat zero-initialised mean and var buffers in the same layout.  step(batch_size): the exchange is finished unscaled, num_update
    advances (one count for all parameters: every one is updated at every step, so MXNet's per-index counts are equal), lr_t =
    lr * sqrt(1 - beta2^t) / (1 - beta1^t) is formed in Python doubles as Adam.update does, and the kernel gets rescale_grad =
    1 / batch_size; then every updated parameter's version counter advances (the kernel writes through raw pointers, and caches such
    as layer.DeformableConv2D._packed key on it)."""

    def __init__(self, named_params, optimizer="adam", optimizer_params=None, n_buckets=4, dist=None):
        if optimizer != "adam":
            raise ValueError("Trainer: only 'adam' (pipeline.py:27) is implemented, got %r" % (optimizer,))
        hp = dict(_ADAM_DEFAULTS)
        hp.update(optimizer_params or {})
        unknown = sorted(set(hp) - set(_ADAM_DEFAULTS) - {"lr_mult", "wd_mult"})
        if unknown:
            raise ValueError("Trainer: unknown optimizer parameters %s" % unknown)
        self._lr_mult, self._wd_mult = dict(hp.pop("lr_mult", None) or {}), dict(hp.pop("wd_mult", None) or {})
        self._hp = hp
        pairs = list(named_params.items()) if hasattr(named_params, "items") else list(named_params)
        pairs = [(k, p) for k, p in pairs if p.requires_grad]
        if not pairs:
            raise ValueError("Trainer: no parameter with requires_grad")
        self.names, self.params = [k for k, _ in pairs], [p for _, p in pairs]
        if len(set(self.names)) != len(self.names):
            raise ValueError("Trainer: parameter names must be unique")
        for k, p in pairs:
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise ValueError("Trainer: parameter %s must be a contiguous float32 tensor" % k)
        self.buckets = GradientBuckets(self.params, n_buckets=n_buckets, dist=dist, align=4)
        self._mean = [torch.zeros_like(b) for b in self.buckets.buckets]
        self._var = [torch.zeros_like(b) for b in self.buckets.buckets]
        where = {}
        for bi, (grp, offs) in enumerate(zip(self.buckets.members, self.buckets.offsets)):
            for p, off in zip(grp, offs):
                where[p] = (bi, off)
        view = lambda flats, p: flats[where[p][0]][where[p][1]:where[p][1] + p.numel()].view_as(p)
        self.mean = {k: view(self._mean, p) for k, p in pairs}      # views into the flat buffers, by name
        self.var = {k: view(self._var, p) for k, p in pairs}
        self.num_update = 0
        self._table = None

    # ---- gluon.Trainer's surface ---------------------------------------------------------------------------------------------
    @property
    def learning_rate(self):
        return self._hp["learning_rate"]

    def set_learning_rate(self, lr):
        self._hp["learning_rate"] = float(lr)

    def lr_t(self, t=None):
        """What Adam.update hands to the operator at update count t (default: the next step's), rounded once to fp32."""
        t = self.num_update + 1 if t is None else int(t)
        coef1 = 1.0 - self._hp["beta1"] ** t
        coef2 = 1.0 - self._hp["beta2"] ** t
        return float(np.float32(self._hp["learning_rate"] * np.sqrt(coef2) / coef1))

    def _rows(self):
        return [(p, p.grad, self.mean[k], self.var[k]) for k, p in zip(self.names, self.params)]

    def step(self, batch_size):
        """trainer.step(batch_size), pipeline.py:114."""
        rows = self._rows()
        for k, (p, g, _, _) in zip(self.names, rows):
            if g is None or g.shape != p.shape or not g.is_contiguous():
                raise RuntimeError("Trainer.step: the gradient of %s no longer views its bucket (zero the gradients with trainer.buckets.zero())" % k)
        self.buckets.finish(scale=False)
        ptrs = [tuple(t.data_ptr() for t in r) for r in rows]
        if self._table is None or self._table.stale(ptrs):      # rebuilt and uploaded only when an address in it changed
            self._table = ops.multi_adam_table(*zip(*rows), lr_mults=[self._lr_mult.get(k, 1.0) for k in self.names],
                                               wd_mults=[self._wd_mult.get(k, 1.0) for k in self.names])
        self.num_update += 1
        hp = self._hp
        ops.multi_adam_update(self._table, self.lr_t(self.num_update), hp["beta1"], hp["beta2"], hp["epsilon"], hp["wd"],
                              1.0 / float(batch_size), hp["clip_gradient"])
        for p in self.params:
            torch.autograd.graph.increment_version(p)

    def save_states(self, path):
        """trainer.save_states (pipeline.py:54).  MXNet's .states is a pickle of MXNet objects; this file is the project's own: the
        NDArray-list container of io.save_params with 'mean:<name>' and 'var:<name>' per parameter and one float64 array
        'trainer:adam' = (num_update, learning_rate, beta1, beta2, epsilon, wd, clip_gradient or -1)."""
        from . import io
        out = {}
        for k in self.names:
            out["mean:" + k] = self.mean[k].detach().cpu().numpy()
            out["var:" + k] = self.var[k].detach().cpu().numpy()
        hp = self._hp
        clip = -1.0 if hp["clip_gradient"] is None else float(hp["clip_gradient"])
        out[_STATE_KEY] = np.array([self.num_update, hp["learning_rate"], hp["beta1"], hp["beta2"], hp["epsilon"], hp["wd"], clip], np.float64)
        io.save_params(path, out)

    def load_states(self, path):
        """trainer.load_states (main.py:143): refuses missing names, unexpected names and wrong shapes before it changes anything."""
        from . import io
        got = io.load_params(path)
        want = [pre + k for k in self.names for pre in ("mean:", "var:")] + [_STATE_KEY]
        missing = [k for k in want if k not in got]
        unexpected = [k for k in got if k not in set(want)]
        if missing:
            raise KeyError("load_states: %s lacks %s" % (path, missing))
        if unexpected:
            raise KeyError("load_states: %s has entries without a parameter here: %s" % (path, unexpected))
        for k, p in zip(self.names, self.params):
            for pre in ("mean:", "var:"):
                if tuple(got[pre + k].shape) != tuple(p.shape) or got[pre + k].dtype != np.float32:
                    raise ValueError("load_states: %s%s is %s %s, the parameter %s float32" % (pre, k, got[pre + k].dtype, got[pre + k].shape, tuple(p.shape)))
        st = got[_STATE_KEY]
        if st.shape != (len(_STATE_FIELDS),) or st.dtype != np.float64:
            raise ValueError("load_states: %s must be %d float64 values" % (_STATE_KEY, len(_STATE_FIELDS)))
        for k in self.names:
            self.mean[k].copy_(torch.from_numpy(got["mean:" + k]))
            self.var[k].copy_(torch.from_numpy(got["var:" + k]))
        self.num_update = int(st[0])
        for name, v in zip(_STATE_FIELDS[1:], st[1:]):
            self._hp[name] = float(v)
        if self._hp["clip_gradient"] < 0:
            self._hp["clip_gradient"] = None


def save_checkpoint(prefix, net, trainer):
    """pipeline.py:52-54: network.save_parameters(prefix + '.params') under the reference's names, trainer.save_states(prefix + '.states')."""
    from . import io
    io.save_params(prefix + ".params", {k: p.detach().cpu().numpy() for k, p in reference_named_parameters(net)})
    trainer.save_states(prefix + ".states")


def load_checkpoint(prefix, net, trainer=None):
    """pipeline.py:56-57 and main.py:143: the parameters of prefix + '.params' into `net` (in place: their addresses, and with them
    the trainer's table, stay), then the trainer's states of prefix + '.states'."""
    from . import io
    got = io.load_params(prefix + ".params")
    own = reference_named_parameters(net)
    missing = [k for k, _ in own if k not in got]
    unexpected = [k for k in got if k not in {k for k, _ in own}]
    if missing or unexpected:
        raise KeyError("load_checkpoint: %s.params lacks %s and has %s without a parameter" % (prefix, missing, unexpected))
    with torch.no_grad():
        for k, p in own:
            if tuple(got[k].shape) != tuple(p.shape):
                raise ValueError("load_checkpoint: %s has shape %s, the parameter %s" % (k, got[k].shape, tuple(p.shape)))
            p.copy_(torch.from_numpy(np.ascontiguousarray(got[k])))
    if trainer is not None:
        trainer.load_states(prefix + ".states")


def load_head(path, net):
    """MaskFlownet.load_head (MaskFlownet.py:410-411, main.py:133): a MaskFlownet_S checkpoint -- `path` is its .params file -- into the
    frozen head of a MaskFlownetTrainable, in place; the cascade keeps what it has.  Refuses missing names, unexpected names and wrong
    shapes before it changes anything."""
    from . import io
    if not isinstance(net, MaskFlownetTrainable):
        raise TypeError("load_head: a MaskFlownetTrainable is expected, got %r" % type(net))
    got = io.load_params(path)
    own = reference_named_parameters(net.head)
    missing = [k for k, _ in own if k not in got]
    unexpected = [k for k in got if k not in {k for k, _ in own}]
    if missing or unexpected:
        raise KeyError("load_head: %s lacks %s and has %s without a parameter in the head" % (path, missing, unexpected))
    for k, p in own:
        if tuple(got[k].shape) != tuple(p.shape):
            raise ValueError("load_head: %s has shape %s, the parameter %s" % (k, got[k].shape, tuple(p.shape)))
    with torch.no_grad():
        for k, p in own:
            p.copy_(torch.from_numpy(np.ascontiguousarray(got[k])))


def train_step(net, loss_fn, opt, im1, im2, label, mask, buckets=None, global_batch=None):
    """pipeline.py:95-114: forward, loss, `loss.backward()` (the per-sample losses summed), the gradient exchange, and
    `trainer.step(batch_size)` -- the optimizer sees (sum over the GLOBAL batch of the per-sample gradients) / global_batch.
    buckets: a GradientBuckets over net.parameters() (its all-reduces start inside backward); None = one device, the gradients
    scaled in place.  global_batch defaults to this call's batch (one device).  Returns the per-sample loss of the local shard.
    opt: a torch optimizer, or a Trainer -- then its own buckets carry the gradients (`buckets` must be None or those) and the step is
    opt.step(global_batch): MXNet's Adam in one launch, the 1 / global_batch inside it."""
    gb = int(global_batch if global_batch is not None else im1.shape[0])
    if isinstance(opt, Trainer):
        if buckets is not None and buckets is not opt.buckets:
            raise ValueError("train_step: a Trainer brings its own gradient buckets")
        opt.buckets.zero()
        preds, _ = net(im1, im2)
        loss = loss_fn(label, mask, *preds)
        loss.sum().backward()
        opt.step(gb)
        return loss.detach()
    if buckets is not None:
        buckets.zero()
    else:
        opt.zero_grad(set_to_none=True)
    preds, _ = net(im1, im2)
    loss = loss_fn(label, mask, *preds)
    loss.sum().backward()
    if buckets is not None:
        buckets.finish(gb)
    else:
        for p in net.parameters():
            if p.grad is not None:
                p.grad.mul_(1.0 / gb)
    opt.step()
    return loss.detach()


def augment_batch(img1, img2, label, mask, geo_aug, color_aug):
    """pipeline.py:99-105 on the device: `/ 255`, the geometry augmenter (the flow comes back flipped to the network's (dy, dx) order,
    :105), the colour augmenter, `centralize` (ops.pair_mean + ops.preprocess_pair at equal size: x - rgb_mean).  img1, img2: (N,3,H,W)
    uint8 or float in 0..255; label: (N,2,H,W) in the reader's (u, v) order; mask: (N,1,H,W) or (N,1,1,1) in 0..255, None = all valid
    (:93-94).  -> (batch (2N,3,Ht,Wt) with images 1 first, label (N,2,Ht,Wt), mask (N,1,Ht,Wt))."""
    N = img1.shape[0]
    if mask is None:
        mask = torch.full((N, 1, 1, 1), 255.0, device=img1.device)
    im1, im2, msk = (t.to(torch.float32) / 255.0 for t in (img1, img2, mask))
    im1, im2, lab, msk = geo_aug(im1, im2, label.to(torch.float32), msk, label_order=1)
    both = color_aug(im1, im2)
    H, W = both.shape[2:]
    return ops.preprocess_pair(both[:N], both[N:], H, W, mean=ops.pair_mean(both[:N], both[N:])), lab, msk


def train_batch(net, loss_fn, opt, img1, img2, label, mask, geo_aug, color_aug, buckets=None, global_batch=None):
    """pipeline.py:89-115: augment_batch, then train_step itself; the finest prediction of its one forward pass is picked up by a
    forward hook that lives for this call.  Returns (the per-sample loss of the local shard, the masked end-point error of :107 per
    sample)."""
    x, lab, msk = augment_batch(img1, img2, label, mask, geo_aug, color_aug)
    N = lab.shape[0]
    finest = []

    def keep(mod, args, out):   # the trainable networks return (predictions, coarse to fine; further outputs): train_step's `preds, _ = net(..)`
        preds = out[0]
        if not isinstance(preds, (list, tuple)) or not torch.is_tensor(preds[-1]):
            raise TypeError("train_batch: net must return (a sequence of flow predictions, coarse to fine; ...), as the trainable networks do")
        finest.append(preds[-1].detach())
    hook = net.register_forward_hook(keep)
    try:
        loss = train_step(net, loss_fn, opt, x[:N], x[N:], lab, msk, buckets=buckets, global_batch=global_batch)
    finally:
        hook.remove()
    epe, _ = ops.flow_metrics(ops.Upsample(finest[-1], loss_fn.scales[-1]), lab, msk)
    return loss, epe


class Validation:
    """`validation_datasets` of the reference's main.py:193-362 and the body of its `validate()` (:157-161), for sets that are resident
    on the device: Validation(sets, batch, full=False, resize=None) with sets = {name: data.DeviceDataset}.  One predict.Predictor is
    kept per distinct sample shape -- built, packed and captured at the first run that meets the shape; every later run puts the
    net's current weights under its captured graph in place (Predictor.load_weights) and validates every set where it lies
    (Predictor.validate_dataset).  full: the net is a MaskFlownetTrainable (frozen head and cascade), else a MaskFlownetSTrainable."""

    def __init__(self, sets, batch, full=False, resize=None):
        self.sets, self.batch, self.full, self.resize = dict(sets), int(batch), bool(full), resize
        self.predictors = {}      # (H, W) -> Predictor

    def run(self, net, kitti=False):
        """-> {name: epe}, or {name: {"epe", "fl"}} with kitti=True (pipeline.py:183-187's two return types), for the net as it is now.
        The weights are read behind the work enqueued on the current stream (the optimizer step) and every set is finished when this
        returns, so the caller may step the optimizer at once."""
        from .predict import Predictor
        named = dict(reference_named_parameters(net))
        groups = {}               # name -> {(H, W): [indices]}
        for name, ds in self.sets.items():
            by_shape = groups.setdefault(name, {})
            for i in range(len(ds)):
                by_shape.setdefault(ds.shape(i), []).append(i)
        fresh = set()
        for name, by_shape in groups.items():
            for shape in by_shape:
                if shape not in self.predictors:
                    host = {k: p.detach().to("cpu", torch.float32).numpy() for k, p in named.items()}
                    self.predictors[shape] = Predictor(host, self.batch, shape[0], shape[1], full=self.full, resize=self.resize,
                                                       device=self.sets[name].device)
                    fresh.add(shape)
        for shape, p in self.predictors.items():
            if shape not in fresh:
                p.load_weights(named)
        out = {}
        for name, by_shape in groups.items():
            per = np.zeros((len(self.sets[name]), 2), np.float32)
            for shape, idx in by_shape.items():
                per[idx] = self.predictors[shape].validate_dataset(self.sets[name], idx)["per_sample"]
            epe, fl = float(np.mean(per[:, 0])), float(np.mean(per[:, 1]))
            out[name] = {"epe": epe, "fl": fl} if kitti else epe
        return out
