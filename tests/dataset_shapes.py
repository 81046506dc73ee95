"""The resolutions the reference trains and predicts at, and every library call MaskFlownet_S and the full MaskFlownet make at one of
them: the workloads as data, for tests/test_dataset_plans.py.

RESOLUTIONS holds numbers only (crop height and width, global batch), each with the place in the reference it is read from.  A
training batch is divided evenly over the cards (main.py:371-372), so the per-card batch is global / 1, 2, 4, 8 wherever that divides;
prediction runs one pair at a time (predict.py:26, :58) on images resized up to multiples of 64 (network/pipeline.py:122-125).

calls(N, H, W, full) derives the call list from maskflownet_amd.network's tables (PYRAMID, DECODER, CONTEXT, UPFEAT, MD, MD_CASCADE,
STRIDES), in the order of network.MaskFlownetS._forward / MaskFlownet._forward and training.MaskFlownet[S]Trainable.  selfcheck()
compares it with network.layer_shapes*() and with hotpath.HotPathWorkload(...).calls()."""
from collections import namedtuple

from maskflownet_amd import hotpath, network
from maskflownet_amd.network import CONTEXT, DEC_SUM, DECODER, HEAD, MD, MD_CASCADE, PYRAMID, STRIDES, UPFEAT

# (name, stage, global batch, H, W, where the numbers stand in the reference)
RESOLUTIONS = [
    ("chairs", "train", 8, 320, 448, "network/config/chairs.yaml:10-11 target_shape; main.py:331 batch_size"),
    ("kitti", "train", 4, 320, 896, "network/config/kitti.yaml:10-11; main.py:198"),
    ("sintel", "train", 4, 384, 768, "network/config/sintel.yaml:10-11; main.py:221"),
    ("things3d", "train", 4, 384, 768, "network/config/things3d.yaml:13-14; main.py:271"),
    ("sintel_kitti_hd1k", "train", 4, 320, 768, "network/config/sintel_kitti2015_hd1k.yaml:16-17; main.py:221"),
    ("kitti", "predict", 1, 384, 1280, "main.py:176 read_resize (370, 1224), rounded up to 64 by network/pipeline.py:122-125"),
    ("sintel", "predict", 1, 448, 1024, "predict.py:10 sintel_resize"),
    ("hd1k", "predict", 1, 1088, 2560, "HD1K frames are 1080 x 2560 (read uncropped for prediction); network/pipeline.py:122-125 rounds up to 64"),
]
CARDS = (1, 2, 4, 8)

Entry = namedtuple("Entry", "name stage N H W source")


def entries():
    """One Entry per (resolution, per-card batch): distinct (stage, N, H, W) only, the first dataset naming it."""
    out, seen = [], set()
    for name, stage, batch, H, W, src in RESOLUTIONS:
        for cards in (CARDS if stage == "train" else (1,)):
            if batch % cards:
                continue     # main.py:371 asserts the division
            key = (stage, batch // cards, H, W)
            if key not in seen:
                seen.add(key)
                out.append(Entry("%s/%d" % (name, cards) if stage == "train" else name, stage, batch // cards, H, W, src))
    return out


# op: conv | deconv | corr | offsets | deform_dropin | deform_shared | warp | upsample
# param: the parameter block ('conv3a', 'MaskFlownet_S.deform4', ...) or None; wshape: its weight shape
# hot: the name of the call in hotpath.HotPathWorkload.calls(), hot_mode the mode it belongs to (None: both)
# dims: conv / deconv (N, Cin, Cout, H, W); corr / deform / warp / upsample / offsets (N, C, H, W)
# geo: conv: kernel, stride, pad, dilate, act; corr: md; deform / offsets: stride; upsample: factor
# req: what the trainer asks of the call's backward ('write' / 'null' per output), None where it issues none
Call = namedtuple("Call", "op param wshape hot hot_mode dims geo req")
W3 = ("write", "write", "write")


def _conv(scope, name, N, cin, cout, h, w, stride=1, dilate=1, act=True, transposed=False, gx=True, train=True, layer=True):
    k = 4 if transposed else 3
    geo = dict(kernel=(k, k), stride=(2, 2) if transposed else (stride, stride), pad=(1, 1) if transposed else (dilate, dilate),
               dilate=(dilate, dilate), act=act)
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    req = ("write" if gx else "null", "write", "write") if train else None
    return Call("deconv" if transposed else "conv", scope + name if layer else None, wshape, None, None, (N, cin, cout, h, w), geo, req)


def _pyramid(scope, N, H, W, cin, letters, train):
    h, w = H, W
    for l in range(1, 7):
        for i, k in enumerate(letters):
            yield _conv(scope, "conv%d%s" % (l, k), 2 * N, cin, PYRAMID[l], h, w, stride=2 if i == 0 else 1, gx=(l, i) != (1, 0), train=train)
            if i == 0:
                h, w = (h + 1) // 2, (w + 1) // 2
            cin = PYRAMID[l]


def _decoder(scope, l, N, c, h, w, train, masks):
    """conv{l}_0..4 (densely connected), the flow [and mask] head, upfeat{l-1}; the inference form's one three-filter head besides."""
    for k, ch in enumerate(DECODER):
        yield _conv(scope, "conv%d_%d" % (l, k), N, c, ch, h, w, train=train)
        c += ch
    yield _conv(scope, "pred_flow%d" % l, N, c, 2, h, w, act=False, train=train)
    if l > 2:
        if masks:
            yield _conv(scope, "pred_mask%d" % l, N, c, 1, h, w, act=False, train=train)
            yield _conv(scope, "heads%d" % l, N, c, 3, h, w, act=False, train=False, layer=False)     # network.MaskFlownetS: both heads in one call
        yield _conv(scope, "upfeat%d" % (l - 1), N, c, UPFEAT, h, w, transposed=True, train=train)
    return c


def _context(scope, N, c, h, w, train):
    for i, (ch, dil) in enumerate(CONTEXT):
        yield _conv(scope, "dc_conv%d" % (i + 1), N, c, ch, h, w, dilate=dil, train=train)
        c = ch
    yield _conv(scope, "dc_conv7", N, c, 2, h, w, act=False, train=train)


def _deform(scope, l, N, h, w, hot, req):
    C = PYRAMID[l]
    wshape, dims, geo = (C, C, 3, 3), (N, C, h, w), dict(stride=float(STRIDES[l]))
    yield Call("offsets", None, None, "offsets" + hot, "dropin", (N, 2, h, w), geo, None)
    yield Call("deform_dropin", None, wshape, "deform" + hot, "dropin", dims, geo, req)
    yield Call("deform_shared", scope + "deform%d" % l, wshape, "deform" + hot, "fused", dims, geo, req)


def calls(N, H, W, full=False):
    """Every library call of MaskFlownet_S at batch N and H x W (full: of MaskFlownet, the head -- frozen, so without a backward --
    followed by the cascade), in forward order."""
    if H % 64 or W % 64:
        raise ValueError("H and W must be multiples of 64")
    scope, train = (HEAD, False) if full else ("", True)
    out = list(_pyramid(scope, N, H, W, 3, "abc", train))
    WW = ("write", "write") if train else None
    W4 = ("write",) * 4 if train else None
    for l in (6, 5, 4, 3, 2):
        h, w, C = H // STRIDES[l], W // STRIDES[l], PYRAMID[l]
        if l < 6:
            out.append(Call("upsample", None, None, None, None, (N, 2, h // 2, w // 2), dict(factor=2), None))
            out.append(Call("upsample", None, None, None, None, (N, 1, h // 2, w // 2), dict(factor=2), None))
            out.append(_conv(scope, "conv%df" % l, N, UPFEAT, C, h, w, act=False, train=train))
            out += _deform(scope, l, N, h, w, "%d" % l, W4)
        out.append(Call("corr", None, None, "corr%d" % l, None, (N, C, h, w), dict(md=MD), WW))
        out += _decoder(scope, l, N, 81 if l == 6 else 81 + C + UPFEAT + 2, h, w, train, masks=True)
    out += _context(scope, N, DEC_SUM + 81 + PYRAMID[2] + UPFEAT + 2, H // 4, W // 4, train)
    out.append(Call("upsample", None, None, None, None, (N, 2, H // 4, W // 4), dict(factor=4), None))
    out.append(Call("warp", None, None, "warp", None, (N, 3, H, W), {}, None))
    if not full:
        return out
    out.append(Call("upsample", None, None, None, None, (N, 1, H // 4, W // 4), dict(factor=4), None))
    out += _pyramid("", N, H, W, 4, "xyz", True)
    for l in (6, 5, 4, 3, 2):
        h, w, C = H // STRIDES[l], W // STRIDES[l], PYRAMID[l]
        if l < 6:
            out.append(Call("upsample", None, None, None, None, (N, 2, h // 2, w // 2), dict(factor=2), None))
        # the features come from the frozen head: no gradient to them; the level-6 flow is the head's as well
        out += _deform("", l, N, h, w, "_u%d" % l, ("null", "null" if l == 6 else "write", "write", "write"))
        out.append(Call("corr", None, None, "corr_u%d" % l, None, (N, C, h, w), dict(md=MD_CASCADE), ("null", "write")))
        out.append(Call("corr", None, None, "corr_v%d" % l, None, (N, C, h, w), dict(md=MD_CASCADE), ("write", "write")))
        out += _decoder("", l, N, network.cascade_input_channels(l), h, w, True, masks=False)
    out += _context("", N, DEC_SUM + network.cascade_input_channels(2), H // 4, W // 4, True)
    out.append(Call("upsample", None, None, None, None, (N, 2, H // 4, W // 4), dict(factor=4), None))
    return out


class _Recorder:
    """Stands in for an OpSet: notes (operator family, shape of the first tensor, md or stride) of every call."""
    FAMILY = {"Correlation": "corr", "DeformableConvolution": "deform_dropin", "deformable_convolution_shared": "deform_shared",
              "deformable_matching": "deform_shared", "offsets_from_flow": "offsets", "warp": "warp", "Correlation_backward": "corr_bwd",
              "DeformableConvolution_backward": "deform_dropin_bwd", "deformable_convolution_shared_backward": "deform_shared_bwd"}

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        fam = self.FAMILY[name]

        def call(*a, **kw):
            first = a[1] if fam.endswith("_bwd") else a[0]      # backward calls take the output gradient first
            if fam in ("corr", "corr_bwd"):
                extra = a[4 if fam == "corr_bwd" else 3]        # max_displacement
            elif fam in ("warp",):
                extra = None
            elif fam == "offsets":
                extra = float(a[2])
            elif fam in ("deform_shared", "deform_shared_bwd"):
                extra = float(a[4 if fam.endswith("_bwd") else 3])
            else:
                extra = None
            self.log.append((fam, tuple(first.shape), extra))
        return call


class _NumpyBuffers:
    def __init__(self):
        import contextlib
        self.ops, self.launching = _Recorder(), contextlib.nullcontext

    def to_device(self, a):
        return a

    def empty(self, shape):
        import numpy as np
        return np.empty(tuple(shape), np.float32)

    def zeros(self, n):
        import numpy as np
        return np.zeros(int(n), np.float32)

    def view(self, flat, off, shape):
        import numpy as np
        return flat[off:off + int(np.prod(shape))].reshape(shape)

    def synchronize(self):
        pass


def hot_path_calls(N, H, W, kind, mode):
    """[(name, family, shape, md or stride)] of the enumeration's hot-path subset, as HotPathWorkload.calls() orders a pass of `kind`."""
    want = [c for c in calls(N, H, W, full=kind == "full") if c.hot is not None and c.hot_mode in (None, mode)]
    fwd = []
    for c in want:
        extra = c.geo["md"] if c.op == "corr" else c.geo["stride"] if c.op in ("offsets", "deform_shared") else None
        fwd.append((c.hot, c.op, c.dims, extra))
    # HotPathWorkload lists the S pass's warp before the cascade; the network issues the same calls in that order too
    if kind != "train":
        return fwd
    bwd = []
    for l in (2, 3, 4, 5, 6):    # finest level first
        for c in want:
            if c.hot == "corr%d" % l:
                bwd.append(("corr_bwd%d" % l, "corr_bwd", c.dims, c.geo["md"]))
        for c in want:
            if c.hot == "deform%d" % l:
                bwd.append(("deform_bwd%d" % l, c.op + "_bwd", c.dims, c.geo["stride"] if c.op == "deform_shared" else None))
    return fwd + bwd


def selfcheck(N=1, H=64, W=128):
    """The enumeration against network.layer_shapes*() (every block exactly once, with its weight shape) and against
    hotpath.HotPathWorkload(...).calls() (the same operators on the same shapes in the same order, every kind and mode)."""
    for full, shapes in ((False, network.layer_shapes()), (True, network.layer_shapes_full())):
        got = [(c.param, tuple(c.wshape)) for c in calls(N, H, W, full) if c.param is not None]
        assert len(got) == len(set(n for n, _ in got)), "a block is listed twice"
        assert sorted(got) == sorted((n, tuple(ws)) for n, ws, _ in shapes), set(got) ^ set((n, tuple(ws)) for n, ws, _ in shapes)
    for kind in hotpath.KINDS:
        for mode in ("dropin", "fused"):
            bufs = _NumpyBuffers()
            wl = hotpath.HotPathWorkload((N, H, W, kind), mode=mode, buffers=bufs, prepack=False)
            names = []
            for name, fn in wl.calls():
                names.append(name)
                fn()
            got = [(n,) + r for n, r in zip(names, bufs.ops.log, strict=True)]
            want = hot_path_calls(N, H, W, kind, mode)
            assert got == want, "%s %s:\n%s\n%s" % (kind, mode, got, want)
    return True
