"""The training set resident in HBM, and batches cut from it by one kernel.

The loader of the reference's main.py:421-509 -- `index_generator`, `iterate_data`, `batch_samples` -- crops, flips, transposes and
stacks every batch in Python threads and uploads it.  Here the samples are uploaded once, as the readers return them (HWC), and
`Feeder.next()` is one small table upload plus one launch of `batch_gather_kernel` (kernels/batch.h, `ops.batch_gather`), which
writes the bytes `batch_samples` would have stacked.  The result is what `training.train_batch` takes.

    ds = data.DeviceDataset("cuda", flow_dtype="float16")
    for a, b, f in pairs:                                   # io.read_ppm / io.read_flo, or any reader: host HWC arrays
        ds.append(a, b, f)
    feed = data.Feeder(data.BatchSampler([ds] * 8, (384, 512), seed=0))
    img1, img2, label, mask = feed.next()

KITTI and HD1K are not stored as read: the reference's readers crop, stretch, resize and normalise every sample with cv2 at load time
(reader/kitti.py:57-74, reader/hd1k.py:51-78).  `DeviceDataset.append_raw` takes the decoded files as they are (readers.py) and runs
that stage on the device, straight into the arena (kernels/ingest.h):

    kitti = data.DeviceDataset("cuda")
    for a, b, fo in readers.kitti_samples(image_dir, flow_dir, indices):
        kitti.append_raw(a, b, fo, crop=(370, 1224))         # main.py:325's kitti.read_dataset(..., crop = (370, 1224))

All randomness is the sampler's: a batch is a function of (seed, step), and `BatchSampler.state()` / `set_state()` continue a run
where a checkpoint left it.
"""
import numpy as np
import torch

from . import ops

_FLOW = {"float32": (np.float32, torch.float32), "float16": (np.float16, torch.float16)}


def _pad16(n):
    return (int(n) + 15) & ~15


class DeviceDataset:
    """Samples (img1, img2, flow[, mask]) in device memory, in the readers' HWC layout.

    They live in chunked byte arenas: a list of `chunk_bytes` torch.uint8 tensors (1 GiB by default), a sample never straddles a
    chunk, every array starts 16-byte aligned and is padded to a multiple of 16 bytes (the read contract of mfn_batch_gather), and an
    address never moves once handed out.  Uploads go through one reused pinned staging buffer.  flow_dtype "float16" halves the
    labels' footprint, as the reference stores FlyingThings3D (main.py:297); the kernel widens them exactly."""

    def __init__(self, device, flow_dtype="float32", chunk_bytes=1 << 30):
        if flow_dtype not in _FLOW:
            raise ValueError("DeviceDataset: flow_dtype must be 'float32' or 'float16', got %r" % (flow_dtype,))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceDataset lives on the MI355X: device is %s (there is no CPU fallback)" % self.device)
        self.flow_dtype = flow_dtype
        self.chunk_bytes = _pad16(chunk_bytes)
        self.has_mask = None          # decided by the first sample; True / False afterwards
        self._chunks, self._used = [], 0
        self._samples = []            # (img1, img2, flow, mask or None): views into the chunks
        self._stage, self._staged = None, None
        self._raw, self._minmax = None, None      # append_raw: the uploaded raw arrays (reused), HD1K's min / max words
        self._nbytes = 0

    # ---- the arena ---------------------------------------------------------------------------------------------------------
    def _reserve(self, total):
        if total > self.chunk_bytes:
            raise ValueError("DeviceDataset: a sample of %d bytes does not fit a chunk of %d" % (total, self.chunk_bytes))
        if not self._chunks or self._used + total > self.chunk_bytes:
            chunk = torch.empty(self.chunk_bytes, dtype=torch.uint8, device=self.device)
            if chunk.data_ptr() % 16:
                raise RuntimeError("DeviceDataset: the allocator returned a chunk that is not 16-byte aligned")
            self._chunks.append(chunk)
            self._used = 0
        off = self._used
        self._used += total
        return self._chunks[-1], off

    def _staging(self, total):
        if self._staged is not None:
            self._staged.synchronize()        # the previous upload has left the buffer
        if self._stage is None or self._stage.numel() < total:
            self._stage = torch.zeros(max(total, 1 << 20), dtype=torch.uint8).pin_memory()
        return self._stage

    def append(self, img1, img2, flow, mask=None):
        """One sample from host arrays: img1, img2 uint8 (H,W,3), flow (H,W,2) float32 or float16, mask uint8 (H,W) or (H,W,1) --
        either every sample of a data set has a mask or none has.  -> its index."""
        img1, img2 = (np.ascontiguousarray(a) for a in (img1, img2))
        if img1.dtype != np.uint8 or img1.ndim != 3 or img1.shape[2] != 3 or min(img1.shape[:2]) < 1:
            raise ValueError("DeviceDataset.append: img1 must be uint8 (H, W, 3), got %s %s" % (img1.dtype, img1.shape))
        H, W = img1.shape[:2]
        if img2.dtype != np.uint8 or img2.shape != (H, W, 3):
            raise ValueError("DeviceDataset.append: img2 must be uint8 %s, got %s %s" % ((H, W, 3), img2.dtype, img2.shape))
        flow = np.asarray(flow)
        if flow.dtype not in (np.float32, np.float16) or flow.shape != (H, W, 2):
            raise ValueError("DeviceDataset.append: flow must be float32 or float16 %s, got %s %s" % ((H, W, 2), flow.dtype, flow.shape))
        flow = np.ascontiguousarray(flow, dtype=_FLOW[self.flow_dtype][0])
        parts = [img1, img2, flow]
        if mask is not None:
            mask = np.ascontiguousarray(mask)
            if mask.dtype != np.uint8 or mask.shape not in ((H, W), (H, W, 1)):
                raise ValueError("DeviceDataset.append: mask must be uint8 %s, got %s %s" % ((H, W, 1), mask.dtype, mask.shape))
            parts.append(mask.reshape(H, W, 1))
        if self.has_mask is not None and self.has_mask != (mask is not None):
            raise ValueError("DeviceDataset.append: this data set %s masks" % ("has" if self.has_mask else "has no"))
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            total += _pad16(a.nbytes)
        stage = self._staging(total)
        host = stage.numpy()
        for a, o in zip(parts, offs):
            host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        chunk, base = self._reserve(total)
        chunk[base:base + total].copy_(stage[:total], non_blocking=True)
        self._staged = torch.cuda.Event()
        self._staged.record(torch.cuda.current_stream(self.device))
        views = []
        for a, o in zip(parts, offs):
            v = chunk[base + o:base + o + a.nbytes]
            if a.dtype != np.uint8:
                v = v.view(_FLOW[self.flow_dtype][1])
            views.append(v.view(a.shape))
        self.has_mask = mask is not None
        self._samples.append(tuple(views) if mask is not None else (views[0], views[1], views[2], None))
        self._nbytes += total
        return len(self._samples) - 1

    @staticmethod
    def _window(H, W, crop):
        """(y0, x0, h, w) of the readers' crops: (h, w) = the bottom h rows and the left w columns (kitti.py:57-60);
        ((top, bottom), (left, right)) = margins (hd1k.py:51)."""
        if crop is None:
            return 0, 0, H, W
        if isinstance(crop[0], (tuple, list)):
            (t, b), (l, r) = ((int(v) for v in side) for side in crop)
            win = (t, l, H - t - b, W - l - r)
            if min(t, b, l, r) < 0:
                raise ValueError("DeviceDataset.append_raw: negative crop margins %s" % (crop,))
        else:
            h, w = (int(v) for v in crop)
            win = (H - h, 0, h, w)
        if win[0] < 0 or win[2] < 1 or win[3] < 1 or win[1] + win[3] > W:
            raise ValueError("DeviceDataset.append_raw: crop %s does not fit a %dx%d sample" % (crop, H, W))
        return win

    def append_raw(self, img1, img2, flow_occ_u16, *, crop=None, resize=None, bgr=True, premultiply=False, normalize=False):
        """One KITTI / HD1K sample from its decoded files (io.read_png: RGB order): img1, img2 uint8 (H,W,3), flow_occ_u16 uint16
        (H,W,3) with R = u, G = v, B = valid.  What the reference's readers do on the host with cv2 runs here on the device, from
        the uploaded raw arrays straight into the stored sample (kernels/ingest.h): crop -- (h, w): the bottom h rows and the left w
        columns (kitti.py:57-60); ((top, bottom), (left, right)): margins (hd1k.py:51) --, channel reversal to cv2.imread's BGR
        (bgr), HD1K's min/max stretch of both images (normalize, hd1k.py:54-56), cv2.resize to resize = (W', H') (None: the window's
        size), the flow's re-scaling and its division by the resized validity, with HD1K's multiplication by the validity first
        (premultiply, hd1k.py:60), and the mask uint8(validity * 255).  The flow is stored in the data set's flow_dtype.  -> its index."""
        img1, img2, fo = (np.ascontiguousarray(a) for a in (img1, img2, flow_occ_u16))
        if img1.dtype != np.uint8 or img1.ndim != 3 or img1.shape[2] != 3 or min(img1.shape[:2]) < 1:
            raise ValueError("DeviceDataset.append_raw: img1 must be uint8 (H, W, 3), got %s %s" % (img1.dtype, img1.shape))
        H, W = img1.shape[:2]
        if img2.dtype != np.uint8 or img2.shape != (H, W, 3):
            raise ValueError("DeviceDataset.append_raw: img2 must be uint8 %s, got %s %s" % ((H, W, 3), img2.dtype, img2.shape))
        if fo.dtype != np.uint16 or fo.shape != (H, W, 3):
            raise ValueError("DeviceDataset.append_raw: flow_occ_u16 must be uint16 %s, got %s %s" % ((H, W, 3), fo.dtype, fo.shape))
        if self.has_mask is False:
            raise ValueError("DeviceDataset.append_raw: this data set has no masks")
        win = self._window(H, W, crop)
        if min(win[2:]) < 2:
            raise ValueError("DeviceDataset.append_raw: a window of %dx%d: both sides must be at least 2" % win[2:])
        Hd, Wd = (win[2], win[3]) if resize is None else (int(resize[1]), int(resize[0]))
        if min(Hd, Wd) < 1:
            raise ValueError("DeviceDataset.append_raw: resize %s" % (resize,))
        # the raw arrays: pinned staging, one copy into a reused device buffer (kernels of the previous call are ahead on the stream)
        offs, total = [], 0
        for a in (img1, img2, fo):
            offs.append(total)
            total += _pad16(a.nbytes)
        stage = self._staging(total)
        host = stage.numpy()
        for a, o in zip((img1, img2, fo), offs):
            host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        if self._raw is None or self._raw.numel() < total:
            self._raw = torch.empty(total, dtype=torch.uint8, device=self.device)
        self._raw[:total].copy_(stage[:total], non_blocking=True)
        self._staged = torch.cuda.Event()
        self._staged.record(torch.cuda.current_stream(self.device))
        r1, r2 = (self._raw[o:o + img1.nbytes].view(H, W, 3) for o in offs[:2])
        rf = self._raw[offs[2]:offs[2] + fo.nbytes].view(torch.uint16).view(H, W, 3)
        # the stored sample: two images, the flow, the mask at the destination size
        np_flow, torch_flow = _FLOW[self.flow_dtype]
        sizes = [Hd * Wd * 3, Hd * Wd * 3, Hd * Wd * 2 * np.dtype(np_flow).itemsize, Hd * Wd]
        starts, need = [], 0
        for n in sizes:
            starts.append(need)
            need += _pad16(n)
        chunk, base = self._reserve(need)
        parts = [chunk[base + o:base + o + n] for o, n in zip(starts, sizes)]
        v1, v2 = parts[0].view(Hd, Wd, 3), parts[1].view(Hd, Wd, 3)
        vf, vm = parts[2].view(torch_flow).view(Hd, Wd, 2), parts[3].view(Hd, Wd, 1)
        tables = ops.ingest_tables(win[2:], (Hd, Wd), like=chunk)
        mm = None
        if normalize:
            if self._minmax is None:
                self._minmax = torch.empty(2, dtype=torch.int32, device=self.device)
            mm = ops.ingest_minmax(r1, r2, win, out=self._minmax)
        ops.ingest_image(r1, win, (Hd, Wd), tables, bgr=bgr, minmax=mm, out=v1)
        ops.ingest_image(r2, win, (Hd, Wd), tables, bgr=bgr, minmax=mm, out=v2)
        ops.ingest_flow_occ(rf, win, (Hd, Wd), tables, premultiply=premultiply, flow_dtype=self.flow_dtype, out_flow=vf, out_mask=vm)
        self.has_mask = True
        self._samples.append((v1, v2, vf, vm))
        self._nbytes += need
        return len(self._samples) - 1

    def extend(self, samples):
        """append() for each (img1, img2, flow) or (img1, img2, flow, mask) of an iterable."""
        for s in samples:
            self.append(*s)

    # ---- what it holds -----------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self._samples)

    def shape(self, i):
        """(H, W) of sample i."""
        return tuple(self._samples[i][0].shape[:2])

    @property
    def nbytes(self):
        """Bytes of device memory the samples occupy, padding included (the chunks reserve more)."""
        return self._nbytes

    def sample(self, i):
        """The device views (img1, img2, flow, mask or None) of sample i: what ops.batch_gather_rows takes.  Their addresses are fixed for
        the data set's lifetime."""
        return self._samples[i]

    def host(self, i):
        """Sample i copied back: numpy (img1, img2, flow, mask or None)."""
        return tuple(None if v is None else v.cpu().numpy() for v in self._samples[i])


class BatchSampler:
    """Which sample, which crop and which flip every slot of every batch gets: the draws of `iterate_data` (main.py:466-478).

    slots: one data set per batch slot (`training_datasets` of main.py, each repeated batch_size // len times; the same data set in
    every slot is a plain batch).  The slots of one data set share one `index_generator`: an epoch permutation without replacement,
    reshuffled when it is used up.  Per sample, in this order: the next index; `y0 = space and randint(space)` with
    space = Hs - Hc, the same for x0; one flip bit.  All draws come from one numpy.random.default_rng(seed), so the sequence is a
    function of the seed; state() / set_state() save and restore it (picklable) for checkpoints.  Only len() and shape(i) of a data
    set are used."""

    def __init__(self, slots, crop_shape, seed=0):
        self.slots = list(slots)
        if not self.slots:
            raise ValueError("BatchSampler: at least one slot")
        self.crop_shape = (int(crop_shape[0]), int(crop_shape[1]))
        if min(self.crop_shape) < 1:
            raise ValueError("BatchSampler: crop_shape %s" % (self.crop_shape,))
        self._sets = []               # the distinct data sets, in order of first appearance
        self._set_of = []             # slot -> index into _sets
        for ds in self.slots:
            k = next((j for j, d in enumerate(self._sets) if d is ds), None)
            if k is None:
                k = len(self._sets)
                self._sets.append(ds)
            self._set_of.append(k)
        self._rng = np.random.default_rng(seed)
        self._perm = [np.zeros(0, np.int64) for _ in self._sets]
        self._pos = [0] * len(self._sets)

    def _next_index(self, k):
        if self._pos[k] >= len(self._perm[k]):
            n = len(self._sets[k])
            if n < 1:
                raise ValueError("BatchSampler: data set %d is empty" % k)
            self._perm[k] = self._rng.permutation(n)
            self._pos[k] = 0
        i = int(self._perm[k][self._pos[k]])
        self._pos[k] += 1
        return i

    def draw(self):
        """-> [(index, y0, x0, flip)] for the slots of the next batch."""
        Hc, Wc = self.crop_shape
        out = []
        for n, k in enumerate(self._set_of):
            i = self._next_index(k)
            Hs, Ws = self._sets[k].shape(i)
            if Hs < Hc or Ws < Wc:
                raise ValueError("BatchSampler: sample %d of slot %d is %dx%d, smaller than the crop %dx%d" % (i, n, Hs, Ws, Hc, Wc))
            y0 = int(self._rng.integers(Hs - Hc)) if Hs > Hc else 0
            x0 = int(self._rng.integers(Ws - Wc)) if Ws > Wc else 0
            out.append((i, y0, x0, int(self._rng.integers(2))))
        return out

    def state(self):
        return {"rng": self._rng.bit_generator.state, "perm": [p.copy() for p in self._perm], "pos": list(self._pos)}

    def set_state(self, state):
        if len(state["perm"]) != len(self._sets):
            raise ValueError("BatchSampler.set_state: the state is of %d data sets, this sampler has %d" % (len(state["perm"]), len(self._sets)))
        self._rng.bit_generator.state = state["rng"]
        self._perm = [np.array(p, np.int64) for p in state["perm"]]
        self._pos = [int(p) for p in state["pos"]]


class Feeder:
    """Batches for training.train_batch: `next()` -> (img1, img2 (N,3,Hc,Wc) uint8, label (N,2,Hc,Wc) float32 in the readers' (u, v)
    order, mask (N,1,Hc,Wc) uint8 or None).  The mask is None when no slot's data set has one (main.py:526-531); a slot without one
    among slots with one is all valid (255).  One table upload and one launch on torch's current stream per batch.  `last_draw` keeps
    the batch's [(index, y0, x0, flip)]."""

    def __init__(self, sampler):
        self.sampler = sampler
        for ds in sampler.slots:
            if not isinstance(ds, DeviceDataset):
                raise TypeError("Feeder: every slot must be a DeviceDataset, got %r" % type(ds))
        self.last_draw = None
        self._rows = None

    def next(self):
        draw = self.sampler.draw()
        samples = [ds.sample(d[0]) for ds, d in zip(self.sampler.slots, draw)]
        self._rows = ops.batch_gather_rows(samples, self.sampler.crop_shape, [(d[1], d[2]) for d in draw], [d[3] for d in draw])
        self.last_draw = draw
        return ops.batch_gather(self._rows, self.sampler.crop_shape, any(bool(ds.has_mask) for ds in self.sampler.slots))

    __next__ = next

    def __iter__(self):
        return self
