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

Frame sequences (the reference's predict_new_data.py: an image pair or the consecutive frames of a video, :100-118, :152-158)
stay bytes until they are on the device: `do_batch_u8` / `predict_frames` upload every uint8 HWC frame once, take the joint mean
and the network's input batch straight from the bytes (csrc/kernels/frames.h) and can colour the flows there
(flow_vis.flow_to_color, restated and unpinned); `python -m maskflownet_amd.predict` is the command line on top of them.
"""
import weakref

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
        self.frames_uploaded = 0            # frames that predict_frames sent to the device: one per frame of the sequence
        self._val_key, self._val_ds = None, lambda: None      # validate_dataset's table: which set and selection it was built for
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

    # ---- uint8 frame sequences on the device (predict_new_data.py:100-118, :152-158) ------------------------------------------------
    def _rows_u8(self, frames, f0, n, height, width, mean, dst):
        """dst[k] <- frames[f0 + min(k, n - 1)] through preprocess_pair_u8 with mean[min(k, n - 1)], for every row of dst: the first n
        rows and the last of them repeated.  A launch of m pairs writes 2m adjacent rows with ONE set of m means, so a launch here is
        (x, x, m): rows [s, s + m) and the same again in [s + m, s + 2m), which a later launch overwrites or, for the last frame, is
        the repeat asked for.  About log2(n) + (rows - n) / 2 launches; no frame is copied."""
        ops, rows, s = self.ops, int(dst.shape[0]), 0
        while s < rows:
            if s >= n - 1:                       # the last frame and its repeats: identical rows, two per launch
                r, x, m = min(s, rows - 2), f0 + n - 1, 1
            else:                                # the second copy stays inside dst and in front of the last frame's row
                r, x, m = s, f0 + s, min(n - 1 - s, (rows - s) // 2)
            ops.preprocess_pair_u8(frames, x, x, m, height, width, mean=None if mean is None else mean[x - f0:x - f0 + m],
                                   out=dst[r:r + 2 * m])
            s = r + 2 if s >= n - 1 else s + m

    def _fill_u8(self, frames, a0, b0, n, height, width, mean, dst):
        """dst (2N,3,height,width) <- the n pairs (frames[a0+k], frames[b0+k]), image 1 in rows [0,N), image 2 in rows [N,2N); a short
        batch repeats its last pair (index arithmetic, one launch for a full batch)."""
        if n == self.N:
            self.ops.preprocess_pair_u8(frames, a0, b0, n, height, width, mean=mean, out=dst)
        else:
            self._rows_u8(frames, a0, n, height, width, mean, dst[:self.N])
            self._rows_u8(frames, b0, n, height, width, mean, dst[self.N:])

    def _enqueue_u8(self, frames, a0, b0, n, label, mask, warped):
        t, ops, b, net, N = self.torch, self.ops, self.b, self.net, self.N
        a0, b0, n = int(a0), int(b0), int(n)
        if not isinstance(frames, t.Tensor) or frames.dtype != t.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (self.H, self.W, 3):
            raise ValueError("do_batch_u8: frames must be a uint8 (F,%d,%d,3) device tensor, got %s %s"
                             % (self.H, self.W, getattr(frames, "dtype", type(frames)), tuple(getattr(frames, "shape", ()))))
        if not 1 <= n <= N:
            raise ValueError("do_batch_u8: %d pairs for a Predictor of batch %d" % (n, N))
        with t.cuda.stream(self.stream):
            ops.pair_mean_u8(frames, a0, b0, n, out=b["mean"][:n])                         # pipeline.py:86 on bytes / 255 (:208)
            self._fill_u8(frames, a0, b0, n, self.H64, self.W64, b["mean"], net.b["im"])   # :120-130
            net.replay()
            flow64 = net.b["gflow_full" if self.full else "flow_full"]
            ops.Upsample(net.b["occlusion"], 4, out=b["occ64"])
            if self.resized:
                flow = ops.bilinear_resize(flow64, self.H, self.W, flow_rescale=True, out=b["flow"])
                occ = ops.bilinear_resize(b["occ64"], self.H, self.W, out=b["occ"])
            else:
                flow, occ = flow64, b["occ64"]
            if warped:
                if "im12" not in b:            # image 1 and image 2 as floats, one (2N,3,H,W) buffer: what one unpack launch writes
                    b["im12"] = t.empty(2 * N, 3, self.H, self.W, device=self.dev)
                self._fill_u8(frames, a0, b0, n, self.H, self.W, None, b["im12"])
                ops.warp(b["im12"][N:], flow, clip_grid=True, out=b["warped"])
            epe = fl = None
            if label is not None:
                self._load(b["label"], label, n, "label")
                if mask is None:
                    b["mask"].fill_(1.0)
                else:
                    self._load(b["mask"], mask, n, "mask")
                ops.flow_metric_sums(flow, b["label"], b["mask"], out=b["sums"])
                epe, fl = (b["sums"][:n, 0] / b["sums"][:n, 1]), (b["sums"][:n, 2] / b["sums"][:n, 1])
        return flow, {"flow": flow[:n], "occ_mask": occ[:n], "warped": b["warped"][:n] if warped else None, "epe": epe, "fl": fl}

    def do_batch_u8(self, frames, a0, b0, n, label=None, mask=None, warped=True):
        """do_batch on bytes that are already on the device.  frames: (F,H,W,3) uint8 device tensor, HWC; the n <= batch pairs are
        (frames[a0+k], frames[b0+k]) -- a video passes b0 = a0 + 1, two stacked lists b0 = a0 + n.  The joint mean is the exact one of
        ops.pair_mean_u8 (one fp32 rounding away from do_batch's on the same images); everything after it is do_batch's sequence.
        warped=False skips the unpacking of the frames into floats and the warp, and returns None for it.  -> do_batch's dict."""
        out = self._enqueue_u8(frames, a0, b0, n, label, mask, warped)[1]
        self.stream.synchronize()
        return out

    def predict_frames(self, frames, color=False, rad_max=None, bgr=False, warped=False):
        """Generator over an iterable of HWC uint8 frames (predict_video_flow, predict_new_data.py:100-118): per consecutive pair
        (flow (H,W,2) in (u,v) order, occ_mask (H,W,1), warped (H,W,3) or None), with color=True followed by the colour picture
        (H,W,3) uint8 of the flow (flow_vis.flow_to_color, :155,:158; rad_max, bgr as ops.flow_color).  Every frame crosses to the device
        once, as bytes (self.frames_uploaded counts them): a batch's last frame stays there as the first of the next.  One
        synchronisation per batch."""
        t, N = self.torch, self.N
        if "frames" not in self.b:
            with t.cuda.stream(self.stream):
                self.b["frames"] = t.empty(N + 1, self.H, self.W, 3, dtype=t.uint8, device=self.dev)
                self.b["rgb"] = t.empty(N, self.H, self.W, 3, dtype=t.uint8, device=self.dev)
        fb, have, new = self.b["frames"], 0, []     # have: 1 once slot 0 holds the frame that opens the next batch

        def run(new):
            nonlocal have
            host = np.stack([self._frame_u8(f) for f in new])
            n = have + len(new) - 1                 # pairs: slots (k, k + 1)
            with t.cuda.stream(self.stream):
                fb[have:have + len(new)].copy_(t.from_numpy(host), non_blocking=True)
                self.frames_uploaded += len(new)
                flow_all, out = self._enqueue_u8(fb, 0, 1, n, None, None, warped)
                rgb = self.ops.flow_color(flow_all, rad_max=rad_max, bgr=bgr, out=self.b["rgb"]) if color else None
            self.stream.synchronize()
            flow = np.flip(out["flow"].cpu().numpy().transpose(0, 2, 3, 1), axis=-1)
            occ = out["occ_mask"].cpu().numpy().transpose(0, 2, 3, 1)
            wrp = out["warped"].cpu().numpy().transpose(0, 2, 3, 1) if warped else None
            pic = rgb[:n].cpu().numpy() if color else None
            with t.cuda.stream(self.stream):
                fb[0].copy_(fb[n])                  # the carry-over, device to device; ordered behind the kernels that read slot 0
            have = 1
            for k in range(n):
                res = (np.ascontiguousarray(flow[k]), np.ascontiguousarray(occ[k]), np.ascontiguousarray(wrp[k]) if warped else None)
                yield res + (pic[k].copy(),) if color else res

        for f in frames:
            new.append(f)
            if have + len(new) == N + 1:
                yield from run(new)
                new = []
        if have + len(new) >= 2:
            yield from run(new)
        elif not have:
            raise ValueError("predict_frames: at least two frames are needed, got %d" % len(new))

    def _frame_u8(self, img):
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.shape != (self.H, self.W, 3):
            raise ValueError("predict_frames: a uint8 (%d,%d,3) frame is expected, got %s %s" % (self.H, self.W, a.dtype, a.shape))
        return a

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

    # ---- validation during training: the net being trained, on a data set that is resident on the device ---------------------------
    def load_weights(self, named_params, wait_stream=None):
        """The network's weights replaced in place under its captured graph (network.MaskFlownetS.load_weights): no allocation, no
        capture.  named_params: a dict, or (name, parameter) pairs as training.reference_named_parameters returns them; device
        tensors are read where they are.  wait_stream (default: the device's current stream) is the stream whose work wrote them --
        the optimizer step: an event recorded there is waited for by the network's stream before the first copy.  Does not
        synchronise: anything that overwrites the parameters next must be ordered behind the network's stream (validate_dataset
        returns after a synchronisation)."""
        t = self.torch
        params = dict(named_params)
        ev = t.cuda.Event()
        ev.record(wait_stream if wait_stream is not None else t.cuda.current_stream(self.dev))
        self.stream.wait_event(ev)
        self.net.load_weights(params)
        return self

    def _val_table(self, ds, indices):
        """One table for the whole set: ceil(S / N) * N rows, the short last batch padded with its last row; uploaded once and kept
        while the data set and the selection stay the same."""
        idx = tuple(range(len(ds))) if indices is None else tuple(int(i) for i in indices)
        if not idx:
            raise ValueError("validate_dataset: no samples")
        key = (id(ds), idx)
        if self._val_key != key or self._val_ds() is not ds:
            for i in idx:
                if ds.shape(i) != (self.H, self.W):
                    raise ValueError("validate_dataset: sample %d is %dx%d, this Predictor was built for %dx%d" % ((i,) + ds.shape(i) + (self.H, self.W)))
            pad = idx + idx[-1:] * (-len(idx) % self.N)
            samples = [ds.sample(i) for i in pad]
            with self.torch.cuda.stream(self.stream):
                rows = self.ops.batch_gather_rows(samples, (self.H, self.W), [(0, 0)] * len(pad), [0] * len(pad))
                sums = self.torch.empty(len(idx), 3, device=self.dev)
            self._val_key, self._val_ds, self._val_rows, self._val_sums = key, weakref.ref(ds), rows, sums
        return len(idx), self._val_rows, self._val_sums

    def validate_dataset(self, ds, indices=None):
        """PipelineFlownet.validate (pipeline.py:149-187) over the samples `indices` (default: all) of a data.DeviceDataset whose
        samples have this Predictor's (H, W), without a host copy of any of them: per batch the joint mean, the network's input batch,
        one replay, the way back to (H, W) and the metric sums of the batch's slots are enqueued on the network's stream, reading
        images, labels (flipped to (dy, dx), :176) and masks (/ 255, :175; all valid where the set has none) where they lie
        (kernels/validate.h).  The warp is skipped: validate never reads it.  One synchronisation and one (S,3) download per set.
        -> {"epe", "fl": the set's means as floats, "per_sample": (S,2) float32 numpy of (epe, fl)}."""
        t, ops, b, net, N = self.torch, self.ops, self.b, self.net, self.N
        S, rows, sums = self._val_table(ds, indices)
        self.stream.wait_stream(t.cuda.current_stream(self.dev))      # the data set's uploads and ingest kernels were enqueued there
        with t.cuda.stream(self.stream):
            for j in range(0, S, N):
                n = min(N, S - j)
                ops.val_pair_mean(rows, j, N, out=b["mean"])                                   # pipeline.py:86 on bytes / 255 (:208)
                ops.val_preprocess(rows, j, N, self.H64, self.W64, mean=b["mean"], out=net.b["im"])   # :120-130
                net.replay()
                flow = net.b["gflow_full" if self.full else "flow_full"]                       # Upsample(4)(flows[-1]), :137
                if self.resized:                                                               # :139-141
                    flow = ops.bilinear_resize(flow, self.H, self.W, flow_rescale=True, out=b["flow"])
                ops.val_flow_metric_sums(rows, j, n, flow[:n], out=sums[j:j + n])              # :175-182
            per = t.stack([sums[:, 0] / sums[:, 1], sums[:, 2] / sums[:, 1]], dim=1)
        self.stream.synchronize()
        per = per.cpu().numpy()
        return {"epe": float(np.mean(per[:, 0])), "fl": float(np.mean(per[:, 1])), "per_sample": per}


# ---- command line: the reference's predict_new_data.py for an image pair or a directory of frames ---------------------------------
def _read_bgr(path):
    """A .png or .ppm file as cv2.imread hands it to the reference (predict_new_data.py:152-153): (H,W,3) uint8 in BGR order."""
    from . import io
    a = io.read_ppm(path) if path.lower().endswith(".ppm") else io.read_png(path)
    if a.dtype != np.uint8:
        raise ValueError("%s: an 8-bit image is expected, got %s" % (path, a.dtype))
    if a.ndim == 2:
        a = a[..., None]
    if a.shape[2] in (1, 2):                # gray (+ alpha): cv2.imread's three equal channels
        a = np.repeat(a[..., :1], 3, axis=2)
    return np.ascontiguousarray(a[..., 2::-1])


def main(argv=None):
    """python -m maskflownet_amd.predict OUT --params FILE [--full] [--resize H,W] [--batch B] [--rad_max R]
    (--image_1 A --image_2 B | --frames DIR): the colour picture of the flow of an image pair as the PNG file OUT, or of every
    consecutive pair of the sorted .png / .ppm files of DIR as OUT/%06d.png.  Video containers are not read: there is no decoder."""
    import argparse
    import os
    from . import io
    ap = argparse.ArgumentParser(prog="python -m maskflownet_amd.predict", description=main.__doc__)
    ap.add_argument("out", help="destination: a PNG file (image pair) or a directory (frames)")
    ap.add_argument("--params", required=True, help="checkpoint in MXNet's NDArray-list format")
    ap.add_argument("--full", action="store_true", help="MaskFlownet (default: MaskFlownet-S)")
    ap.add_argument("--resize", default="", help="H,W the network runs at (default: the next multiples of 64)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rad_max", type=float, default=None, help="flow radius that saturates the colours (default: each picture's largest)")
    ap.add_argument("--image_1")
    ap.add_argument("--image_2")
    ap.add_argument("--frames", help="directory of .png / .ppm frames, taken in sorted order")
    args = ap.parse_args(argv)
    if (args.frames is None) == (args.image_1 is None) or (args.image_1 is None) != (args.image_2 is None):
        ap.error("give --image_1 and --image_2, or --frames")
    resize = [int(s) for s in args.resize.split(",")] if args.resize else None
    if args.frames is not None:
        names = sorted(f for f in os.listdir(args.frames) if f.lower().endswith((".png", ".ppm")))
        paths = [os.path.join(args.frames, f) for f in names]
    else:
        paths = [args.image_1, args.image_2]
    if len(paths) < 2:
        ap.error("at least two frames are needed, found %d" % len(paths))
    first = _read_bgr(paths[0])
    batch = max(1, min(args.batch, len(paths) - 1))
    p = Predictor(network.from_reference_keys(io.load_params(args.params)), batch, first.shape[0], first.shape[1], full=args.full, resize=resize)
    frames = (first if k == 0 else _read_bgr(q) for k, q in enumerate(paths))
    pictures = (out[3] for out in p.predict_frames(frames, color=True, rad_max=args.rad_max, bgr=False))
    if args.frames is None:
        io.write_png(args.out, next(pictures))
    else:
        os.makedirs(args.out, exist_ok=True)
        for k, pic in enumerate(pictures):
            io.write_png(os.path.join(args.out, "%06d.png" % k), pic)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
