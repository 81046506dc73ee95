"""What one training batch is, stated in numpy: the expected value of tests/test_batch_gather.py and tests/test_data_feed.py.

Per sample: cut the crop out of every HWC array, move the channels to the front, and where the flip bit is set reverse the W axis of
all of them and negate the first channel of the label; then stack the samples.  A label kept as float16 is widened to float32 first
(exact).  A sample without a mask, in a batch with one, is all valid: 255."""
import numpy as np


def gather_sample(img1, img2, flow, mask, crop_shape, y0, x0, flip):
    """-> [img1 (3,Hc,Wc) uint8, img2, label (2,Hc,Wc) float32, mask (1,Hc,Wc) uint8 or None] of one sample."""
    Hc, Wc = crop_shape
    H, W = img1.shape[:2]
    assert 0 <= y0 and y0 + Hc <= H and 0 <= x0 and x0 + Wc <= W, "the crop leaves the sample"
    arrs = [np.asarray(img1), np.asarray(img2), np.asarray(flow).astype(np.float32)]
    if mask is not None:
        arrs.append(np.asarray(mask).reshape(H, W, 1))
    cut = [np.transpose(a[y0:y0 + Hc, x0:x0 + Wc], (2, 0, 1)) for a in arrs]
    if flip:
        cut = [a[:, :, ::-1] for a in cut]
        cut[2] = np.stack([-cut[2][0], cut[2][1]], axis=0)
    cut = [np.ascontiguousarray(a) for a in cut]
    return cut if mask is not None else cut + [None]


def gather_batch(samples, crop_shape, draws, with_mask):
    """samples: [(img1, img2, flow, mask or None)]; draws: [(y0, x0, flip)] -> (img1, img2, label, mask or None), stacked NCHW."""
    Hc, Wc = crop_shape
    rows = [gather_sample(*s, crop_shape, *d) for s, d in zip(samples, draws)]
    out = [np.stack([r[k] for r in rows], axis=0) for k in range(3)]
    if not with_mask:
        return out[0], out[1], out[2], None
    masks = [r[3] if r[3] is not None else np.full((1, Hc, Wc), 255, np.uint8) for r in rows]
    return out[0], out[1], out[2], np.stack(masks, axis=0)
