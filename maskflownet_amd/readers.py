"""File-level readers of KITTI, HD1K and Sintel: which files make a sample, decoded by io.py and nothing more.

The reference's readers (/root/reference/reader/kitti.py, reader/hd1k.py, reader/sintel.py) also crop, stretch, resize and normalise
every sample on the host with cv2; here that stage is `data.DeviceDataset.append_raw` (kernels/ingest.h), and these generators yield
what it takes -- for Sintel, whose samples are stored as read, what `append` takes.  Which samples train and which validate is the
CALLER's argument (`indices`, `names`, `entries`): the reference's index lists and split file are not part of this package.

    ds = data.DeviceDataset("cuda")
    for a, b, fo in readers.kitti_samples(image_dir, flow_dir, range(200)):
        ds.append_raw(a, b, fo, crop=(370, 1224))
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
