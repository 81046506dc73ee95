"""The two augmenters of the training batch, on the device.

Callers on the reference's side: /root/reference/network/pipeline.py:100-101 (`geo_aug(img1, img2, label, mask)`, then
`color_aug(img1, img2)`), configured per dataset by /root/reference/main.py:389-419.  The classes keep the constructor arguments of
/root/reference/augmentation.py:168-171 (`ColorAugmentation`) and :229-231 (`GeometryAugmentation`); the bodies are this project's:

* the per-sample scalars are drawn on the HOST from a seeded numpy generator (`draw()`), a few dozen numbers per step;
* the parameter tables of csrc/kernels/augment.h are formed from them in fp64 and rounded once to fp32 (`geometry_table`,
  `color_table`) -- the `_unit` matrix, the two scale clamps of :278-279, pad_x / pad_y, the relative transform and its inverse; the
  reference's `force_translation` (:307, a max / min over the whole grid on the device) in closed form: the extremes of the affine
  function a x + b y + t over [-1,1]^2 are t +- (|a| + |b|);
* one upload of the table and one library call (`ops.augment_geometry`), resp. two (`ops.augment_color_mean`, `ops.augment_color`):
  neither the grids, nor the concatenated (img1 | mask | flow * mask) tensor, nor the noise exist in memory.

`ColorAugmentation` keeps a 64-bit call counter, the offset of the Philox counter: every call draws fresh noise, and the same seed
reproduces a run bit for bit.  There is no CPU implementation behind the calls."""
import math

import numpy as np

AG_THETA1, AG_THETA2, AG_FT, AG_RT, AG_FSHIFT, AG_INV2, AG_FACTOR, AG_K = 0, 6, 12, 14, 16, 18, 22, 26
AC_M, AC_CC, AC_CHANNEL, AC_BRIGHTNESS, AC_E, AC_SPIN, AC_K = 0, 9, 12, 15, 16, 17, 26


def _pair(r):
    try:
        r = tuple(float(v) for v in r)
    except TypeError:
        r = (-float(r), float(r))
    if len(r) != 2:
        raise ValueError("expected a range (low, high), got %r" % (r,))
    return r


def _upload(table, like):
    import torch
    return torch.from_numpy(np.ascontiguousarray(table, np.float32)).to(like.device, non_blocking=False)


def relative_matrices(rotation, scale, target_shape):
    """(R (N,2,2), R_inverse (N,2,2)) of augmentation.py:253-269: the second image's extra rotation / zoom in grid units (the
    target's aspect ratio enters R) and its inverse in pixels."""
    A = (target_shape[0] - 1) / (target_shape[1] - 1)
    c, s = np.cos(rotation), np.sin(rotation)
    R = np.stack([scale * c, -scale * s * A, scale * s / A, scale * c], axis=1).reshape(-1, 2, 2)
    Ri = np.stack([c / scale, s / scale, -s / scale, c / scale], axis=1).reshape(-1, 2, 2)
    return R, Ri


def geometry_table(d, orig_shape, target_shape):
    """The (N, 26) fp32 table of augment_geometry_kernel from the drawn scalars `d` (GeometryAugmentation.draw), in fp64 throughout."""
    Ho, Wo = (int(v) for v in orig_shape)
    Ht, Wt = (int(v) for v in target_shape)
    rot, aspect = np.asarray(d["rotation"], np.float64), np.asarray(d["aspect"], np.float64)
    N = rot.shape[0]
    u00, u01, u10, u11 = (Wt - 1) / (Wo - 1), (Wt - 1) / (Ho - 1), (Ht - 1) / (Wo - 1), (Ht - 1) / (Ho - 1)
    c, s, ar = np.cos(rot), np.sin(rot), np.abs(rot)
    scale = np.minimum(d["scale"], (Wo - 1) / (aspect * ((Ht - 1) * np.sin(ar) + (Wt - 1) * np.cos(ar))))   # the source's width ...
    scale = np.minimum(scale, (Ho - 1) / ((Ht - 1) * np.cos(ar) + (Wt - 1) * np.sin(ar)))                 # ... and height hold the crop
    pad_x, pad_y = 1 - scale * u00, 1 - scale * u11
    tx = d["shift_unit"][:, 0] * pad_x + d["shift"][:, 0]
    ty = d["shift_unit"][:, 1] * pad_y + d["shift"][:, 1]
    lin = np.stack([scale * aspect * c * u00, -scale * aspect * s * u10, scale * s * u01, scale * c * u11], axis=1).reshape(N, 2, 2)
    linv = np.stack([c / (scale * aspect), s / (scale * aspect), -s / scale, c / scale], axis=1).reshape(N, 2, 2)
    R, Ri = relative_matrices(np.asarray(d["rel_rotation"], np.float64), np.asarray(d["rel_scale"], np.float64), (Ht, Wt))
    lin2 = lin @ R
    t = np.stack([tx, ty], axis=1)
    ext = np.abs(lin).sum(axis=2)                                    # the first grid spans t - ext .. t + ext per coordinate
    ft = np.maximum(t + ext - 1, 0) + np.minimum(t - ext + 1, 0)
    rt = np.asarray(d["rel_translation"], np.float64)
    tab = np.zeros((N, AG_K), np.float64)
    tab[:, AG_THETA1:AG_THETA1 + 6] = np.concatenate([lin, t[:, :, None]], axis=2).reshape(N, 6)
    tab[:, AG_THETA2:AG_THETA2 + 6] = np.concatenate([lin2, t[:, :, None]], axis=2).reshape(N, 6)
    tab[:, AG_FT:AG_FT + 2] = ft
    tab[:, AG_RT:AG_RT + 2] = rt
    tab[:, AG_FSHIFT:AG_FSHIFT + 2] = rt * np.array([(Wo - 1) / 2, (Ho - 1) / 2])
    tab[:, AG_INV2:AG_INV2 + 4] = (Ri @ linv).reshape(N, 4)
    tab[:, AG_FACTOR:AG_FACTOR + 4] = ((Ri - np.eye(2)) @ np.diag([(Wt - 1) / 2, (Ht - 1) / 2])).reshape(N, 4)
    return tab.astype(np.float32)


class GeometryAugmentation:
    """augmentation.py:229-339.  __call__(img1, img2, flow, mask) -> (img1', img2', flow', mask') at target_shape; images in [0,1],
    flow (N,2,H,W) in the reader's (u, v) order, mask (N,1,H,W) or (N,1,1,1).  label_order=1 returns the flow as (dy, dx)."""

    def __init__(self, angle_range, zoom_range, translation_range, target_shape, orig_shape, batch_size, aspect_range=None,
                 relative_angle=None, relative_scale=None, relative_translation=None, seed=0):
        self._angle_range = tuple(v / 180 * math.pi for v in angle_range)
        self._scale_range = _pair(zoom_range)
        self._translation_range = tuple(2 * v for v in _pair(translation_range))      # grid units span 2
        self._target_shape = tuple(int(v) for v in target_shape)
        self._orig_shape = tuple(int(v) for v in orig_shape)
        if min(self._target_shape) < 2 or min(self._orig_shape) < 2:
            raise ValueError("GeometryAugmentation: every side must be >= 2, got %s -> %s" % (self._orig_shape, self._target_shape))
        self._batch_size = int(batch_size)
        self._aspect_range = None if aspect_range is None else _pair(aspect_range)
        self._relative = relative_angle is not None
        self._relative_angle = tuple(v * relative_angle for v in self._angle_range) if self._relative else (0.0, 0.0)
        self._relative_scale = _pair(relative_scale) if (self._relative and relative_scale is not None) else (1.0, 1.0)
        self._relative_translation = (tuple(v * relative_translation for v in self._translation_range)
                                      if (self._relative and relative_translation is not None) else None)
        self.rng = np.random.default_rng(seed)
        self.last_table = None

    def ranges(self):
        """name -> (low, high) of every scalar draw() returns."""
        one = (1.0, 1.0)
        return {"rotation": self._angle_range, "aspect": self._aspect_range or one, "scale": self._scale_range, "shift_unit": (-1.0, 1.0),
                "shift": self._translation_range, "rel_rotation": self._relative_angle, "rel_scale": self._relative_scale,
                "rel_translation": self._relative_translation or (0.0, 0.0)}

    def draw(self):
        """One step's scalars, (batch,) or (batch, 2) each, uniform in ranges()."""
        N, r = self._batch_size, self.ranges()
        shape = {"shift_unit": (N, 2), "shift": (N, 2), "rel_translation": (N, 2)}
        return {k: self.rng.uniform(lo, hi, shape.get(k, (N,))) for k, (lo, hi) in r.items()}

    def table(self, d=None):
        return geometry_table(self.draw() if d is None else d, self._orig_shape, self._target_shape)

    def state(self):
        """What the next call's draws depend on (picklable): the numpy bit generator's state.  set_state() continues from it."""
        return {"rng": self.rng.bit_generator.state}

    def set_state(self, state):
        self.rng.bit_generator.state = state["rng"]

    def __call__(self, img1, img2, flow, mask, label_order=0, out=None):
        from . import ops
        if tuple(img1.shape) != (self._batch_size, 3) + self._orig_shape:
            raise ValueError("GeometryAugmentation: images of shape %s expected, got %s" % ((self._batch_size, 3) + self._orig_shape, tuple(img1.shape)))
        self.last_table = self.table()
        return ops.augment_geometry(img1, img2, flow, mask, _upload(self.last_table, img1), self._target_shape, label_order=label_order, out=out)


def color_table(d, eigen_aug=False):
    """The (N, 26) fp32 table of the colour kernels from the drawn scalars `d` (ColorAugmentation.draw), in fp64 throughout."""
    alpha, theta = np.asarray(d["alpha"], np.float64), np.asarray(d["theta"], np.float64)
    N = alpha.shape[0]
    su, sw = alpha * np.cos(theta), alpha * np.sin(theta)
    # saturation / hue: a rotation by theta and a stretch by alpha of the chroma plane of YIQ, written out in RGB (:198-200)
    base = np.array([[0.299, 0.587, 0.114]] * 3)
    cu = np.array([[0.701, -0.587, -0.114], [-0.299, 0.413, -0.114], [-0.300, -0.588, 0.886]])
    cw = np.array([[0.168, 0.330, -0.497], [-0.328, 0.035, 0.292], [1.250, -1.050, -0.203]])
    M = base[None] + su[:, None, None] * cu[None] + sw[:, None, None] * cw[None]
    tab = np.zeros((N, AC_K), np.float64)
    tab[:, AC_M:AC_M + 9] = M.reshape(N, 9)
    tab[:, AC_CC:AC_CC + 3] = np.asarray(d["contrast"], np.float64)[:, None] * d["channel"]
    tab[:, AC_CHANNEL:AC_CHANNEL + 3] = d["channel"]
    tab[:, AC_BRIGHTNESS] = d["brightness"]
    tab[:, AC_E] = np.exp(d["gamma"]) if d.get("gamma") is not None else 1.0
    spin = np.tile(np.eye(3).reshape(1, 9), (N, 1))
    if eigen_aug:      # three successive plane rotations (:203-208)
        c, s = np.cos(d["spin_angle"]), np.sin(d["spin_angle"])
        c0, c1, c2, s0, s1, s2 = c[:, 0], c[:, 1], c[:, 2], s[:, 0], s[:, 1], s[:, 2]
        spin = np.stack([c0 * c1, s1 * c2 + s0 * c1 * s2, s1 * s2 - s0 * c1 * c2,
                         -c0 * s1, c1 * c2 - s0 * s1 * s2, c1 * s2 + s0 * s1 * c2,
                         s0, -c0 * s2, c0 * c2], axis=1)
    tab[:, AC_SPIN:AC_SPIN + 9] = spin
    return tab.astype(np.float32)


class ColorAugmentation:
    """augmentation.py:168-227.  __call__(img1, img2) -> (2N,3,H,W): both augmented images in one buffer, images 1 first (the layout
    `ops.preprocess_pair` and the trainable networks' torch.cat([im1, im2], 0) use)."""

    def __init__(self, contrast_range, brightness_sigma, channel_range, batch_size, shape, noise_range, saturation, hue,
                 gamma_range=None, eigen_aug=False, seed=0):
        self._contrast_range = _pair(contrast_range)
        self._brightness_sigma = float(brightness_sigma)
        self._channel_range = _pair(channel_range)
        self._batch_size = int(batch_size)
        self._shape = tuple(int(v) for v in shape)
        self._noise_range = _pair(noise_range)
        self._gamma_range = None if gamma_range is None else _pair(gamma_range)
        self._eigen_aug = bool(eigen_aug)
        self._saturation, self._hue = float(saturation), float(hue)
        self.rng = np.random.default_rng(seed)
        self.seed = int(self.rng.integers(0, 2 ** 63)) * 2 + int(self.rng.integers(0, 2))     # the 64-bit Philox key
        self.calls = 0                                                                          # the 64-bit Philox offset
        self.last_table = self.last_sigma = self.last_offset = None

    def ranges(self):
        """name -> (low, high) of every uniformly drawn scalar of draw() (the brightness is normal)."""
        r = {"contrast": tuple(v + 1 for v in self._contrast_range), "channel": self._channel_range, "noise_sigma": self._noise_range,
             "alpha": (1 - self._saturation, 1 + self._saturation), "theta": (-self._hue * math.pi, self._hue * math.pi)}
        if self._gamma_range is not None:
            r["gamma"] = self._gamma_range
        if self._eigen_aug:
            r["spin_angle"] = (-math.pi, math.pi)
        return r

    def draw(self):
        N = self._batch_size
        shape = {"channel": (N, 3), "noise_sigma": (), "spin_angle": (N, 3)}
        d = {k: self.rng.uniform(lo, hi, shape.get(k, (N,))) for k, (lo, hi) in self.ranges().items()}
        d["brightness"] = self.rng.normal(0.0, self._brightness_sigma, (N,))
        return d

    def table(self, d):
        return color_table(d, self._eigen_aug)

    def state(self):
        """What the next call's draws and noise depend on (picklable): the numpy bit generator's state, the Philox key and the call
        counter.  set_state() continues from it."""
        return {"rng": self.rng.bit_generator.state, "seed": int(self.seed), "calls": int(self.calls)}

    def set_state(self, state):
        self.rng.bit_generator.state = state["rng"]
        self.seed, self.calls = int(state["seed"]), int(state["calls"])

    def __call__(self, img1, img2, out=None):
        from . import ops
        if tuple(img1.shape) != (self._batch_size, 3) + self._shape:
            raise ValueError("ColorAugmentation: images of shape %s expected, got %s" % ((self._batch_size, 3) + self._shape, tuple(img1.shape)))
        d = self.draw()
        self.last_table, self.last_sigma, self.last_offset = self.table(d), float(np.float32(d["noise_sigma"])), self.calls
        self.calls = (self.calls + 1) & (2 ** 64 - 1)
        return ops.augment_color(img1, img2, _upload(self.last_table, img1), sigma=self.last_sigma, seed=self.seed, offset=self.last_offset,
                                 spin=self._eigen_aug, gamma=self._gamma_range is not None, out=out)


def presets(dataset, batch, orig_shape, target_shape, seed=0):
    """(geo_aug, color_aug) as main.py:389-419 configures them for 'sintel', 'kitti' or any other dataset (the chairs / things default)."""
    if dataset == "sintel":
        color = dict(contrast_range=(-0.4, 0.8), brightness_sigma=0.1, channel_range=(0.8, 1.4), noise_range=(0, 0), saturation=0.5, hue=0.5)
        geo = dict(angle_range=(-17, 17), zoom_range=(1 / 1.5, 1 / 0.9), aspect_range=(0.9, 1 / 0.9), translation_range=0.1,
                   relative_angle=0.25, relative_scale=(0.96, 1 / 0.96), relative_translation=0.25)
    elif dataset == "kitti":
        color = dict(contrast_range=(-0.2, 0.4), brightness_sigma=0.05, channel_range=(0.9, 1.2), noise_range=(0, 0.02), saturation=0.25,
                     hue=0.1, gamma_range=(-0.5, 0.5))
        geo = dict(angle_range=(-5, 5), zoom_range=(1 / 1.25, 1 / 0.95), aspect_range=(0.95, 1 / 0.95), translation_range=0.05,
                   relative_angle=0.25, relative_scale=(0.98, 1 / 0.98), relative_translation=0.25)
    else:
        color = dict(contrast_range=(-0.4, 0.8), brightness_sigma=0.1, channel_range=(0.8, 1.4), noise_range=(0, 0.04), saturation=0.5, hue=0.5)
        geo = dict(angle_range=(-17, 17), zoom_range=(0.5, 1 / 0.9), aspect_range=(0.9, 1 / 0.9), translation_range=0.1,
                   relative_angle=0.25, relative_scale=(0.96, 1 / 0.96), relative_translation=0.25)
    geo_aug = GeometryAugmentation(target_shape=target_shape, orig_shape=orig_shape, batch_size=batch, seed=[seed, 0], **geo)
    color_aug = ColorAugmentation(batch_size=batch, shape=target_shape, eigen_aug=False, seed=[seed, 1], **color)
    return geo_aug, color_aug
