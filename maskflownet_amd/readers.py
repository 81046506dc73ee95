"""File-level readers of KITTI, HD1K and Sintel: which files make a sample, decoded by io.py and nothing more.

The reference's readers (/root/reference/reader/kitti.py, reader/hd1k.py, reader/sintel.py) also crop, stretch, resize and normalise
every sample on the host with cv2; here that stage is `data.DeviceDataset.append_raw` (kernels/ingest.h), and these generators yield
what it takes -- for Sintel, whose samples are stored as read, what `append` takes.  Which samples train and which validate is the
CALLER's argument (`indices`, `names`, `entries`): the reference's index lists and split file are not part of this package.

    ds = data.DeviceDataset("cuda")
    for a, b, fo in readers.kitti_samples(image_dir, flow_dir, range(200)):
        ds.append_raw(a, b, fo, crop=(370, 1224))

The LISTERS restate which files the reference's readers pick, given the caller's lists: `read_split` / `chairs_split` / `chairs_samples`
(FlyingChairs), `things3d_entries` / `things3d_samples` (the FlyingThings3D subset), `kitti_indices` / `kitti_count` (the `parts` filter),
`hd1k_names` (the first map of every sequence is skipped), `sintel_entries` (the split consumed in listing order).  `run.load_datasets`
puts them together as main.py:190-365 does.
"""
import os

from . import io


def kitti_samples(image_dir, flow_dir, indices):
    """KITTI 2012 / 2015 (kitti.py:54-56): per index k the frames image_dir/%06d_10.png and %06d_11.png and the 16-bit flow map
    flow_dir/%06d_10.png -> (img1, img2 uint8 (H,W,3) RGB, flow_occ uint16 (H,W,3) with R = u, G = v, B = valid)."""
    for k in indices:
        yield (io.read_png(os.path.join(image_dir, "%06d_10.png" % k)), io.read_png(os.path.join(image_dir, "%06d_11.png" % k)),
               io.read_png(os.path.join(flow_dir, "%06d_10.png" % k)))


def hd1k_samples(image_dir, flow_dir, names):
    """HD1K (hd1k.py:43-53): names are the flow maps' stems "SSSSSS_FFFF" (sequence, first frame); the pair is the frames FFFF and
    FFFF + 1 of the sequence -> as kitti_samples.  append_raw(..., crop=((50, 50), (100, 100)), premultiply=True, normalize=True,
    resize=...) is the reference's reading."""
    for name in names:
        seq, frame = name.rsplit("_", 1)
        nxt = "%s_%0*d" % (seq, len(frame), int(frame) + 1)
        yield (io.read_png(os.path.join(image_dir, name + ".png")), io.read_png(os.path.join(image_dir, nxt + ".png")),
               io.read_png(os.path.join(flow_dir, name + ".png")))


def sintel_samples(root, subset, entries):
    """Sintel training pairs (sintel.py:29-40): entries are (sequence, frame number i); subset "clean" or "final" ->
    (img1, img2 uint8 (H,W,3), flow float32 (H,W,2) (u, v), mask uint8 (H,W,1) = 255 - invalid): what DeviceDataset.append takes."""
    for seq, i in entries:
        frame = lambda kind, n, ext: os.path.join(root, "training", kind, seq, "frame_%04d.%s" % (n, ext))
        yield (io.read_png(frame(subset, i, "png"))[..., :3], io.read_png(frame(subset, i + 1, "png"))[..., :3],
               io.read_flo(frame("flow", i, "flo")), io.read_sintel_invalid(frame("invalid", i, "png")))


def read_split(path):
    """A split file -- one integer per white-space separated entry, as FlyingChairs_train_val.txt (1 = training, 2 = validation) and
    the Sintel split (sintel.py:17) -- -> [int]."""
    with open(path) as f:
        return [int(float(tok)) for tok in f.read().split()]


def chairs_split(split):
    """(training, validation) sample numbers of FlyingChairs from its split entries: sample k (1-based, chairs/trainval.py) trains where
    entry k - 1 is 1 and validates otherwise."""
    train = [k + 1 for k, v in enumerate(split) if v == 1]
    valid = [k + 1 for k, v in enumerate(split) if v != 1]
    return train, valid


def chairs_samples(root, indices):
    """FlyingChairs (main.py:340-342): per sample number k root/%05d_img1.ppm, %05d_img2.ppm, %05d_flow.flo ->
    (img1, img2 uint8 (H,W,3), flow float32 (H,W,2)): what DeviceDataset.append takes."""
    for k in indices:
        yield (io.read_ppm(os.path.join(root, "%05d_img1.ppm" % k)), io.read_ppm(os.path.join(root, "%05d_img2.ppm" % k)),
               io.read_flo(os.path.join(root, "%05d_flow.flo" % k)))


def things3d_entries(root, sub_type="clean"):
    """The FlyingThings3D subset's training pairs (things3d.py:9-36) -> [(image 1, image 2, flow)] paths.  Per sub_type ('clean',
    'final'; 'mixed' = both), camera (left, right) and direction (into_future, into_past), in this order, every file of
    root/train/flow/<camera>/<direction> in os.listdir order: image 1 is the frame of the flow's number in
    root/train/image_<sub_type>/<camera>, image 2 its neighbour -- the next frame into the future, the previous one into the past.
    Images are PNG files, flows Middlebury .flo: no PFM reader is needed."""
    if sub_type not in ("clean", "final", "mixed"):
        raise ValueError("things3d_entries: sub_type must be 'clean', 'final' or 'mixed', got %r" % (sub_type,))
    out = []
    for sub in (("clean", "final") if sub_type == "mixed" else (sub_type,)):
        for camera in ("left", "right"):
            for direction, step in (("into_future", 1), ("into_past", -1)):
                images = os.path.join(root, "train", "image_" + sub, camera)
                flows = os.path.join(root, "train", "flow", camera, direction)
                for name in os.listdir(flows):
                    stem, ext = os.path.splitext(name)
                    if ext != ".flo":
                        continue
                    number = stem[-7:]
                    out.append((os.path.join(images, stem + ".png"),
                                os.path.join(images, stem[:-7] + "%07d" % (int(number) + step) + ".png"),
                                os.path.join(flows, name)))
    return out


def things3d_samples(entries):
    """The entries of things3d_entries decoded -> (img1, img2 uint8 (H,W,3) in cv2.imread's BGR order (main.py:291-294), flow float32
    (H,W,2)): what DeviceDataset.append takes."""
    for a, b, f in entries:
        yield (io.read_png(a)[..., 2::-1], io.read_png(b)[..., 2::-1], io.read_flo(f))


def kitti_indices(n, valid, part="mixed"):
    """Which of the pairs 0 .. n - 1 of a KITTI edition belong to `part` (kitti.py:42-53): 'valid' = the indices of `valid`, 'train' =
    the others, 'mixed' = all.  `valid` is walked once in its own order, as the reference walks it, so it must ascend; an entry that is
    out of order or >= n is never met and then stops every later one from matching."""
    if part not in ("train", "valid", "mixed"):
        raise ValueError("kitti_indices: part must be 'train', 'valid' or 'mixed', got %r" % (part,))
    out, ind = [], 0
    for k in range(int(n)):
        if ind < len(valid) and valid[ind] == k:
            ind += 1
            if part == "train":
                continue
        elif part == "valid":
            continue
        out.append(k)
    return out


def kitti_count(flow_dir, follow_reference=False):
    """How many pairs a KITTI flow directory holds.  The reference takes len(os.listdir(flow_dir)) - 1 files (kitti.py:41), which drops
    the LAST pair of a directory that holds nothing but its flow maps: a real KITTI 2015 flow_occ directory of 200 files gives 199
    there, and pair 000199 -- a member of the reference's own 2015 validation list -- is never read.  This function counts the files
    named %06d_10.png and does NOT follow the reference: 200 files are 200 pairs.  follow_reference=True gives the reference's count
    (for reproducing its logged set sizes)."""
    n = sum(1 for f in os.listdir(flow_dir) if len(f) == 13 and f.endswith("_10.png") and f[:6].isdigit())
    return max(n - 1, 0) if follow_reference else n


def hd1k_names(flow_dir, valid=(5,), part="mixed", samples=-1):
    """The flow maps of HD1K that make a sample (hd1k.py:26-50) -> their stems "SSSSSS_FFFF", the FIRST frame's, as hd1k_samples takes
    them.  The files of flow_dir are taken in sorted order (the reference takes os.listdir's, which is sorted on the file systems it
    ran on; its sequence rule needs a sequence's maps adjacent).  Position k of the list is filtered by `valid` / `part` exactly as
    kitti_indices does; of what is left, the first map of every sequence -- the first one whose sequence number differs from the
    previous kept one's -- is skipped, and a map SSSSSS_FFFF stands for the pair (FFFF - 1, FFFF) with the flow map of FFFF - 1.
    samples: at most that many positions are looked at (-1: all; the reference looks at one fewer than the directory holds, this
    function at all of them, see kitti_count)."""
    files = sorted(f for f in os.listdir(flow_dir) if f.endswith(".png"))
    n = len(files) if samples is None or samples < 0 else min(len(files), int(samples))
    out, previous = [], None
    for k in kitti_indices(n, list(valid), part):
        seq, frame = files[k][:-4].rsplit("_", 1)
        first = seq != previous
        previous = seq
        if first:
            continue
        out.append("%s_%0*d" % (seq, len(frame), int(frame) - 1))
    return out


def sintel_entries(root, split, parts=("training", "test"), subsets=("clean", "final")):
    """Sintel's pairs by division (sintel.py:12-44) -> {'training': {subset: [(sequence, frame)]}, 'training1': ..., 'training2': ...,
    'test': ...}.  Per subset the sequences are walked in os.listdir order and the frames of a sequence in ascending order; every
    frame but the last opens a pair.  `split` (read_split of the caller's split file; None where only 'test' is asked for) is consumed
    one entry per training pair in that walk, anew for every subset: entry 1 puts the pair into 'training1', 2 into 'training2'.  So a
    split file belongs to one listing order, as the reference's does."""
    import re
    pattern = re.compile(r"frame_(\d+)\.png$")
    out = {}
    for part in parts:
        out[part] = {}
        if part == "training":
            out["training1"], out["training2"] = {}, {}
        for subset in subsets:
            base = os.path.join(root, part, subset)
            out[part][subset] = []
            if part == "training":
                out["training1"][subset], out["training2"][subset] = [], []
            c = 0
            for seq in os.listdir(base):
                frames = sorted(int(m.group(1)) for m in map(pattern.match, os.listdir(os.path.join(base, seq))) if m)
                for i in frames[:-1]:
                    out[part][subset].append((seq, i))
                    if part == "training":
                        if split is None or c >= len(split):
                            raise ValueError("sintel_entries: the split has %d entries, the tree more training pairs"
                                             % (0 if split is None else len(split)))
                        if split[c] not in (1, 2):
                            raise ValueError("sintel_entries: split entry %d is %r, expected 1 or 2" % (c, split[c]))
                        out["training%d" % split[c]][subset].append((seq, i))
                        c += 1
    return out


def sintel_test_pairs(root, subset, entries):
    """The frames of Sintel's test pairs (predict.py:25) -> (img1, img2 uint8 (H,W,3)) per (sequence, frame) entry."""
    for seq, i in entries:
        frame = lambda n: os.path.join(root, "test", subset, seq, "frame_%04d.png" % n)
        yield io.read_png(frame(i))[..., :3], io.read_png(frame(i + 1))[..., :3]
