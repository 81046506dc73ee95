"""Prediction on images of any size: what PipelineFlownet does around the network, on the device.

The caller of the network at inference time, /root/reference/network/pipeline.py: `centralize` (:85-87), `do_batch_mx`
(:117-132), `do_batch` (:134-147), `validate` (:149-187) and `predict` (:189-223).  MaskFlownetS / MaskFlownet accept only
heights and widths that are multiples of 64; the reference feeds them anything by

    centralize by the pair's joint RGB mean  ->  BilinearResize2D up to the next multiple of 64 (a resize, not a pad)
    ->  network  ->  Upsample(4)  ->  BilinearResize2D back, flow components * (H / H64, W / W64)
    ->  Reconstruction2DSmooth of image 2  ->  masked EPE / KITTI outlier ratio

and `Predictor` is that sequence: four HIP kernels of csrc/kernels/predict.h (joint mean, centralize + resize of both
images straight into the network's input batch, resize back, metric sums) plus Upsample and warp, enqueued on the
network's own stream around one replay of its hipGraph, one synchronisation per batch.  The resize arithmetic is MXNet
1.5's (align_corners, fp32 positions; include/mfn_hip.h), not torch's.
"""
import numpy as np

from . import network
from .ops import default_ops


def round_up_64(s):
    """s + (64 - s % 64) % 64 (pipeline.py:123-124): the size the network runs at."""
    s = int(s)
    if s < 1:
        raise ValueError("image sizes must be >= 1, got %d" % s)
    return s + (64 - s % 64) % 64


def network_size(H, W, resize=None):
    """(H64, W64): the next multiples of 64, or `resize` as given (pipeline.py:122-127)."""
    if resize is not None:
        return int(resize[0]), int(resize[1])
    return round_up_64(H), round_up_64(W)


def _chw01(img):
    """HWC uint8 (-> / 255, pipeline.py:208) or float in [0,1] -> CHW float32."""
    a = np.asarray(img)
    if a.ndim != 3:
        raise ValueError("an HWC image is expected, got shape %s" % (a.shape,))
    a = a.astype(np.float32) / np.float32(255.0) if a.dtype == np.uint8 else a.astype(np.float32)
    return np.ascontiguousarray(a.transpose(2, 0, 1))


class Predictor:
    """Predictor(params, batch, H, W): flow, occlusion mask and warped image 2 for (batch,3,H,W) pairs of any H, W >= 1.
    full=True runs network.MaskFlownet (params with the 'MaskFlownet_S.' head), else network.MaskFlownetS; resize=(H', W')
    runs the network at that size instead of the next multiples of 64."""

    def __init__(self, params, batch, H, W, full=False, resize=None, device="cuda:0"):
        import torch
        self.torch, self.ops = torch, default_ops()
        self.N, self.H, self.W, self.full = int(batch), int(H), int(W), bool(full)
        if self.N < 1 or self.H < 1 or self.W < 1:
            raise ValueError("Predictor: batch, H and W must be >= 1, got %d, %d, %d" % (self.N, self.H, self.W))
        self.H64, self.W64 = network_size(self.H, self.W, resize)
        self.resized = (self.H64, self.W64) != (self.H, self.W)
        self.net = (network.MaskFlownet if full else network.MaskFlownetS)(params, self.N, self.H64, self.W64, device)
        self.dev, self.stream = self.net.dev, self.net.stream
        N, H, W = self.N, self.H, self.W
        with torch.cuda.stream(self.stream):
            e = lambda *shape: torch.empty(*shape, device=self.dev)
            self.b = {"im1": e(N, 3, H, W), "im2": e(N, 3, H, W), "mean": e(N, 3), "occ64": e(N, 1, self.H64, self.W64),
                      "warped": e(N, 3, H, W), "label": e(N, 2, H, W), "mask": e(N, 1, H, W), "sums": e(N, 3)}
            if self.resized:
                self.b["flow"] = e(N, 2, H, W)
                self.b["occ"] = e(N, 1, H, W)
            self.net.b["im"].zero_()        # the forward that capture() runs first reads it: finite flows, in-range gathers
        self.net.capture()
        self.net.synchronize()

    def _load(self, dst, src, n, what):
        t = self.torch
        src = t.as_tensor(src)
        if src.dtype != t.float32:
            raise TypeError("%s: float32 expected, got %s" % (what, src.dtype))
        want = (n,) + tuple(dst.shape[1:])
        if tuple(src.shape) != want:
            src = src.expand(want)          # e.g. the reference's (n,1,1,1) all-valid mask; anything else raises here
        dst[:n].copy_(src.to(self.dev, non_blocking=True))
        if n < self.N:                      # a short batch: repeat its last sample
            dst[n:].copy_(dst[n - 1:n].expand((self.N - n,) + tuple(dst.shape[1:])))

    def do_batch(self, img1, img2, label=None, mask=None):
        """img1, img2: (n,3,H,W) in [0,1], n <= batch (numpy or torch, any device); label (n,2,H,W) in network order
        (channel 0 = dy, as after pipeline.py:176), mask (n,1,H,W) or broadcastable, default all valid.
        -> dict(flow (n,2,H,W), occ_mask (n,1,H,W), warped (n,3,H,W), epe (n,), fl (n,)); epe / fl are None without a label.
        The tensors are this object's buffers: the next call overwrites them."""
        t, ops, b, net, N = self.torch, self.ops, self.b, self.net, self.N
        n = int(img1.shape[0])
        if not 1 <= n <= N:
            raise ValueError("do_batch: %d pairs for a Predictor of batch %d" % (n, N))
        with t.cuda.stream(self.stream):
            self._load(b["im1"], img1, n, "img1")
            self._load(b["im2"], img2, n, "img2")
            ops.pair_mean(b["im1"], b["im2"], out=b["mean"])
            ops.preprocess_pair(b["im1"], b["im2"], self.H64, self.W64, mean=b["mean"], out=net.b["im"])
            net.replay()
            flow64 = net.b["gflow_full" if self.full else "flow_full"]                     # Upsample(4)(flows[-1]), pipeline.py:137
            ops.Upsample(net.b["occlusion"], 4, out=b["occ64"])                            # :138
            if self.resized:                                                               # :139-142
                flow = ops.bilinear_resize(flow64, self.H, self.W, flow_rescale=True, out=b["flow"])
                occ = ops.bilinear_resize(b["occ64"], self.H, self.W, out=b["occ"])
            else:
                flow, occ = flow64, b["occ64"]
            ops.warp(b["im2"], flow, clip_grid=True, out=b["warped"])                      # Reconstruction2DSmooth, :143
            epe = fl = None
            if label is not None:
                self._load(b["label"], label, n, "label")
                if mask is None:
                    b["mask"].fill_(1.0)
                else:
                    self._load(b["mask"], mask, n, "mask")
                ops.flow_metric_sums(flow, b["label"], b["mask"], out=b["sums"])
                epe, fl = (b["sums"][:n, 0] / b["sums"][:n, 1]), (b["sums"][:n, 2] / b["sums"][:n, 1])
        self.stream.synchronize()
        return {"flow": flow[:n], "occ_mask": occ[:n], "warped": b["warped"][:n], "epe": epe, "fl": fl}

    def _batches(self, *lists):
        size = len(lists[0])
        if any(len(l) != size for l in lists):
            raise ValueError("lists of different lengths: %s" % ([len(l) for l in lists],))
        for j in range(0, size, self.N):
            yield [l[j:j + self.N] for l in lists]

    def predict(self, img1s, img2s):
        """Generator over lists of HWC images (uint8, or float in [0,1]): per pair (flow (H,W,2) in (u,v) order -- what
        io.write_flo takes --, occ_mask (H,W,1), warped (H,W,3)) as numpy arrays (pipeline.py:189-223)."""
        for im1, im2 in self._batches(img1s, img2s):
            out = self.do_batch(np.stack([_chw01(a) for a in im1]), np.stack([_chw01(a) for a in im2]))
            flow = np.flip(out["flow"].cpu().numpy().transpose(0, 2, 3, 1), axis=-1)
            occ = out["occ_mask"].cpu().numpy().transpose(0, 2, 3, 1)
            warped = out["warped"].cpu().numpy().transpose(0, 2, 3, 1)
            for k in range(len(im1)):
                yield np.ascontiguousarray(flow[k]), np.ascontiguousarray(occ[k]), np.ascontiguousarray(warped[k])

    def validate(self, img1s, img2s, labels, masks=None, return_type="epe"):
        """Mean over the set of the per-pair masked EPE (return_type='epe') or KITTI outlier ratio (anything else),
        pipeline.py:149-187.  labels: HWC (u,v) flows, flipped to the network's (dy,dx) here (:176); masks: HW1 uint8 (255 =
        valid, / 255 as :175) or float, default all valid."""
        vals = []
        if masks is None:
            masks = [None] * len(labels)
        for im1, im2, lab, msk in self._batches(img1s, img2s, labels, masks):
            lab = np.stack([np.ascontiguousarray(np.asarray(l, np.float32).transpose(2, 0, 1)[::-1]) for l in lab])
            m = None if msk[0] is None else np.stack([_chw01(x) for x in msk])
            out = self.do_batch(np.stack([_chw01(a) for a in im1]), np.stack([_chw01(a) for a in im2]), lab, m)
            vals.append((out["epe"] if return_type == "epe" else out["fl"]).cpu().numpy())
        return float(np.mean(np.concatenate(vals)))
