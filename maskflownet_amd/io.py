"""Flow and checkpoint IO next to the hot path -- host side only, numpy.

* Middlebury `.flo`: b'PIEH' (the float 202021.25), int32 width, int32 height, then H*W (u, v) float32 pairs, little
  endian (/root/reference/reader/chairs/flo.py:4-25 hard-codes the 512x384 header; reader/sintel.py:46-73 reads the
  general one).  `.flo` stores (u, v) = (dx, dy); the network uses channel 0 = dy (pipeline.py:105,176,219), so
  `flo_to_network` / `network_to_flo` do the flip and the HWC <-> CHW move.
* Binary PPM (`P6`), the FlyingChairs images: `P6`, width, height, maxval as decimal text separated by white space
  (`#` comments allowed), ONE white-space byte, then H*W RGB triples.  reader/chairs/ppm.py accepts only the literal
  header `P6 512 384 255\n`; `read_ppm` reads any size at maxval 255.
* MXNet `.params` (`save_parameters`, pipeline.py:52-63): an NDArray list -- uint64 magic 0x112, uint64 reserved,
  uint64 count, count x NDArray, uint64 name count, names as uint64 length + bytes.  An NDArray (V2, magic 0xF993FAC9)
  is int32 storage type (0 = dense), shape as uint32 ndim + int64 dims, context (int32 dev_type, int32 dev_id), int32
  dtype flag, raw little-endian data; V1 (0xF993FAC8) has no storage type; older files start with the uint32 ndim and
  carry uint32 dims.  Restated from MXNet 1.x `src/ndarray/ndarray.cc`; MXNet cannot run here and the reference's
  weights are absent (.MISSING_LARGE_BLOBS), so the reader is pinned by tests/golden/mxnet_v2.params -- assembled byte
  by byte from that layout by tests/golden/make_params_fixture.py, independently of the writer below -- and by round
  trips.
* PNG, the frames of Sintel / KITTI / HD1K, Sintel's invalid masks and KITTI's 16-bit flow maps (cv2.imread of
  /root/reference/reader/kitti.py:54-56 and reader/hd1k.py:51-53, skimage.io.imread of reader/sintel.py:79): the
  8-byte signature, then chunks of uint32 length, 4-byte type, data, CRC-32 of type and data, all big endian.  IHDR:
  width, height, bit depth, colour type (0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGBA), compression, filter,
  interlace.  The IDAT chunks together are one zlib stream of scanlines, each a filter-type byte (None, Sub, Up,
  Average, Paeth) followed by the filtered bytes; 16-bit samples are big endian.  Restated from the PNG specification
  on `zlib` alone; the filters are reversed by mfn_png_unfilter, host C++ inside the library.  `read_png` returns the
  FILE's channel order (RGB), not cv2's BGR.  `write_kitti_flow` is the benchmark submission writer of
  /root/reference/predict.py:63-66.
"""
import struct
import zlib

import numpy as np

FLO_TAG = 202021.25
_LIST_MAGIC = 0x112
_V1, _V2, _V3 = 0xF993FAC8, 0xF993FAC9, 0xF993FACA
_DTYPES = {0: np.float32, 1: np.float64, 2: np.float16, 3: np.uint8, 4: np.int32, 5: np.int8, 6: np.int64}
_FLAGS = {np.dtype(v): k for k, v in _DTYPES.items()}


def read_flo(path):
    """-> (H, W, 2) float32, last axis (u, v) = (dx, dy)."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) != 12:
            raise ValueError("%s: truncated .flo header" % path)
        tag, w, h = struct.unpack("<fii", head)
        if tag != FLO_TAG:
            raise ValueError("%s: bad .flo tag %r (expected 'PIEH' = %r)" % (path, tag, FLO_TAG))
        if w <= 0 or h <= 0 or w > 99999 or h > 99999:
            raise ValueError("%s: implausible .flo size %dx%d" % (path, w, h))
        data = np.fromfile(f, dtype="<f4", count=2 * w * h)
    if data.size != 2 * w * h:
        raise ValueError("%s: truncated .flo payload" % path)
    return data.reshape(h, w, 2).astype(np.float32, copy=False)


def read_ppm(path):
    """Binary PPM (P6, maxval 255) of any size -> (H, W, 3) uint8, as reader/chairs/ppm.py returns it for 512x384."""
    with open(path, "rb") as f:
        buf = f.read()
    pos, fields = 0, []
    while len(fields) < 4:
        while pos < len(buf) and buf[pos:pos + 1].isspace():
            pos += 1
        if buf[pos:pos + 1] == b"#":                 # a comment runs to the end of its line
            while pos < len(buf) and buf[pos:pos + 1] != b"\n":
                pos += 1
            continue
        end = pos
        while end < len(buf) and not buf[end:end + 1].isspace():
            end += 1
        if end == pos:
            raise ValueError("%s: truncated PPM header" % path)
        fields.append(buf[pos:end])
        pos = end
    if fields[0] != b"P6":
        raise ValueError("%s: bad PPM magic %r (expected b'P6')" % (path, fields[0][:8]))
    try:
        w, h, maxval = (int(v) for v in fields[1:])
    except ValueError:
        raise ValueError("%s: bad PPM header fields %r" % (path, fields[1:])) from None
    if maxval != 255:
        raise ValueError("%s: PPM maxval %d (only 255 is read)" % (path, maxval))
    if w <= 0 or h <= 0 or w > 99999 or h > 99999:
        raise ValueError("%s: implausible PPM size %dx%d" % (path, w, h))
    pos += 1                                          # the single white-space byte behind maxval
    if len(buf) - pos < 3 * w * h:
        raise ValueError("%s: truncated PPM payload (%d of %d bytes)" % (path, max(0, len(buf) - pos), 3 * w * h))
    return np.frombuffer(buf, np.uint8, 3 * w * h, pos).reshape(h, w, 3).copy()


_PNG_SIG = b"\x89PNG\r\n\x1a\n"
_PNG_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def read_png(path):
    """-> (H, W) for gray, (H, W, C) otherwise, uint8 or uint16, in the file's channel order.  Colour types 0, 2, 4, 6 at bit
    depths 8 and 16, all five row filters, any number of IDAT chunks; interlaced and palette files raise."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:8] != _PNG_SIG:
        raise ValueError("%s: not a PNG file (signature %r)" % (path, buf[:8]))
    pos, head, idat, ended = 8, None, [], False
    while pos + 12 <= len(buf) and not ended:
        (n,) = struct.unpack_from(">I", buf, pos)
        kind, data = buf[pos + 4:pos + 8], buf[pos + 8:pos + 8 + n]
        if len(data) != n or pos + 12 + n > len(buf):
            raise ValueError("%s: truncated %r chunk" % (path, kind))
        if struct.unpack_from(">I", buf, pos + 8 + n)[0] != (zlib.crc32(kind + data) & 0xFFFFFFFF):
            raise ValueError("%s: bad CRC of a %r chunk" % (path, kind))
        pos += 12 + n
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif kind == b"IDAT":
            idat.append(data)
        elif kind == b"IEND":
            ended = True
    if head is None or not idat or not ended:
        raise ValueError("%s: a PNG file needs IHDR, IDAT and IEND chunks" % path)
    w, h, depth, ctype, comp, filt, lace = head
    if w <= 0 or h <= 0 or w > 99999 or h > 99999:
        raise ValueError("%s: implausible PNG size %dx%d" % (path, w, h))
    if ctype == 3:
        raise ValueError("%s: palette PNG files are not read" % path)
    if lace != 0:
        raise ValueError("%s: interlaced PNG files are not read" % path)
    if ctype not in _PNG_CHANNELS or depth not in (8, 16) or comp != 0 or filt != 0:
        raise ValueError("%s: PNG colour type %d at bit depth %d (compression %d, filter %d) is not read" % (path, ctype, depth, comp, filt))
    C, item = _PNG_CHANNELS[ctype], depth // 8
    row = w * C * item
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if raw.size != h * (row + 1):
        raise ValueError("%s: %d bytes of image data, %d expected" % (path, raw.size, h * (row + 1)))
    raw = raw.copy()
    from . import _lib
    _lib.check(_lib.lib().png_unfilter(raw.ctypes.data, h, row, C * item), "png_unfilter")
    px = np.ascontiguousarray(raw.reshape(h, row + 1)[:, 1:])
    out = px if item == 1 else px.view(">u2").astype(np.uint16)
    return out.reshape((h, w) if C == 1 else (h, w, C))


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, array):
    """8-bit or 16-bit gray (H, W), gray + alpha (H, W, 2), RGB (H, W, 3) or RGBA (H, W, 4); filter None, one IDAT."""
    a = np.asarray(array)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 2, 3, 4)) or min(a.shape[:2]) < 1:
        raise ValueError("write_png: expected uint8 or uint16 (H, W) or (H, W, 1..4), got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    C = 1 if a.ndim == 2 else a.shape[2]
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[C]
    rows = np.ascontiguousarray(a.reshape(h, w * C).astype(">u2" if a.dtype == np.uint16 else np.uint8)).view(np.uint8).reshape(h, -1)
    raw = np.zeros((h, rows.shape[1] + 1), np.uint8)
    raw[:, 1:] = rows
    with open(path, "wb") as f:
        f.write(_PNG_SIG + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8 * a.dtype.itemsize, ctype, 0, 0, 0))
                + _png_chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _png_chunk(b"IEND", b""))


def write_kitti_flow(path, flow_hw2_uv):
    """KITTI's 16-bit flow map of a prediction, (H, W, 2) in (u, v) order (predict.py:63-66): R = uint16(64.0 * (u + 512)), G the
    same of v, both evaluated in float64 and truncated, B = 1 (numpy evaluates the reference's expression in float32 for a float32
    flow, which can round u + 512 before the truncation; float64 is the exact quantisation).  Values outside the format's range
    (-512 .. 511.98) saturate."""
    fl = np.asarray(flow_hw2_uv, np.float64)
    if fl.ndim != 3 or fl.shape[2] != 2:
        raise ValueError("write_kitti_flow: expected (H, W, 2), got %s" % (fl.shape,))
    pred = np.ones(fl.shape[:2] + (3,), np.uint16)
    pred[..., 0:2] = np.clip(64.0 * (fl + 512.0), 0.0, 65535.0).astype(np.uint16)
    write_png(path, pred)


def read_sintel_invalid(path):
    """Sintel's invalid map as the reference's mask (reader/sintel.py:80-81): 255 - gray[..., None], uint8 (H, W, 1)."""
    gray = read_png(path)
    if gray.ndim != 2 or gray.dtype != np.uint8:
        raise ValueError("%s: an 8-bit gray PNG expected, got %s %s" % (path, gray.dtype, gray.shape))
    return 255 - gray[..., None]


def write_flo(path, flow_hw2):
    a = np.ascontiguousarray(flow_hw2, dtype="<f4")
    if a.ndim != 3 or a.shape[2] != 2:
        raise ValueError("write_flo: expected (H, W, 2), got %s" % (a.shape,))
    with open(path, "wb") as f:
        f.write(struct.pack("<fii", FLO_TAG, a.shape[1], a.shape[0]))
        a.tofile(f)


def flo_to_network(flow_hw2):
    """(H, W, 2) (u, v) -> (2, H, W) with channel 0 = dy, as the network and mfn_warp_fwd expect."""
    return np.ascontiguousarray(np.asarray(flow_hw2)[..., ::-1].transpose(2, 0, 1))


def network_to_flo(flow_2hw):
    return np.ascontiguousarray(np.asarray(flow_2hw).transpose(1, 2, 0)[..., ::-1])


def _read_ndarray(buf, pos):
    (magic,) = struct.unpack_from("<I", buf, pos)
    if magic in (_V2, _V3):
        pos += 4
        (stype,) = struct.unpack_from("<i", buf, pos)
        pos += 4
        if stype != 0:
            raise ValueError("sparse NDArray (storage type %d) is not supported" % stype)
        (ndim,) = struct.unpack_from("<I" if magic == _V2 else "<i", buf, pos)
        pos += 4
        dims = struct.unpack_from("<%dq" % ndim, buf, pos)
        pos += 8 * ndim
    elif magic == _V1:
        pos += 4
        (ndim,) = struct.unpack_from("<I", buf, pos)
        pos += 4
        dims = struct.unpack_from("<%dq" % ndim, buf, pos)
        pos += 8 * ndim
    else:  # legacy: the first word is ndim, dims are uint32
        ndim = magic
        if ndim > 16:
            raise ValueError("not an MXNet NDArray (first word 0x%x)" % magic)
        pos += 4
        dims = struct.unpack_from("<%dI" % ndim, buf, pos)
        pos += 4 * ndim
    if ndim == 0:
        return np.zeros((0,), np.float32), pos
    pos += 8  # context: dev_type, dev_id
    (flag,) = struct.unpack_from("<i", buf, pos)
    pos += 4
    if flag not in _DTYPES:
        raise ValueError("unknown MXNet dtype flag %d" % flag)
    dt = np.dtype(_DTYPES[flag]).newbyteorder("<")
    n = int(np.prod(dims, dtype=np.int64))
    arr = np.frombuffer(buf, dtype=dt, count=n, offset=pos).reshape(dims).copy()
    return arr, pos + n * dt.itemsize


def load_params(path):
    """MXNet NDArray-list file -> {name: ndarray}.  Gluon prefixes ('arg:' / 'aux:') are stripped, so the structural
    keys of save_parameters ('deform5.weight', 'conv1a.0.weight', ...) come back as they are."""
    buf = open(path, "rb").read()
    magic, _reserved, count = struct.unpack_from("<QQQ", buf, 0)
    if magic != _LIST_MAGIC:
        raise ValueError("%s: not an MXNet NDArray list (magic 0x%x)" % (path, magic))
    pos, arrays = 24, []
    for _ in range(count):
        a, pos = _read_ndarray(buf, pos)
        arrays.append(a)
    (nnames,) = struct.unpack_from("<Q", buf, pos)
    pos += 8
    names = []
    for _ in range(nnames):
        (ln,) = struct.unpack_from("<Q", buf, pos)
        pos += 8
        names.append(buf[pos:pos + ln].decode())
        pos += ln
    if nnames not in (0, count):
        raise ValueError("%s: %d names for %d arrays" % (path, nnames, count))
    if not names:
        names = [str(i) for i in range(count)]
    strip = lambda k: k.split(":", 1)[1] if k[:4] in ("arg:", "aux:") else k
    return {strip(k): a for k, a in zip(names, arrays)}


def save_params(path, params):
    """Writer of the same format (V2 dense NDArrays on cpu(0)); used to pin load_params by round trips."""
    with open(path, "wb") as f:
        f.write(struct.pack("<QQQ", _LIST_MAGIC, 0, len(params)))
        for a in params.values():
            a = np.ascontiguousarray(a)
            if a.dtype not in _FLAGS:
                raise ValueError("dtype %s has no MXNet flag" % a.dtype)
            f.write(struct.pack("<IiI", _V2, 0, a.ndim))
            f.write(struct.pack("<%dq" % a.ndim, *a.shape))
            f.write(struct.pack("<iii", 1, 0, _FLAGS[a.dtype]))
            f.write(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes())
        f.write(struct.pack("<Q", len(params)))
        for k in params:
            kb = k.encode()
            f.write(struct.pack("<Q", len(kb)))
            f.write(kb)


def load_into(module, params, strict=True):
    """Copy checkpoint arrays into a torch module that uses the reference's parameter names (layer.DeformableConv2D:
    '<prefix>weight' / '<prefix>bias').  Blocks built the way the reference builds them -- DeformableConv2D with
    in_channels=0, MaskFlownet.py:155-158: weight creation deferred to the first forward -- are materialised here from
    the checkpoint's weight shape first, so that their parameters exist to be loaded (and are seen by an optimizer
    built afterwards).  strict: every parameter must be in the checkpoint AND every checkpoint key must match a
    parameter.  Returns (missing, unexpected)."""
    import torch
    from .layer import DeformableConv2D
    for name, mod in module.named_modules():
        if isinstance(mod, DeformableConv2D) and mod.weight is None:
            key = (name + "." if name else "") + "weight"
            if key in params:
                w = params[key]
                if w.ndim != 4 or w.shape[0] != mod._channels or tuple(w.shape[2:]) != tuple(mod._kwargs["kernel"]):
                    raise ValueError("%s: checkpoint shape %s does not fit DeformableConv2D(%d, kernel %s)"
                                     % (key, w.shape, mod._channels, mod._kwargs["kernel"]))
                mod._materialize(int(w.shape[1]) * mod._kwargs["num_group"], torch.device("cpu"))
    own = dict(module.named_parameters())
    missing = [k for k in own if k not in params]
    unexpected = [k for k in params if k not in own]
    if strict and missing:
        raise KeyError("checkpoint lacks %s" % missing)
    if strict and unexpected:
        raise KeyError("checkpoint keys without a parameter: %s" % unexpected)
    with torch.no_grad():
        for k, p in own.items():
            if k in params:
                if tuple(p.shape) != tuple(params[k].shape):
                    raise ValueError("%s: checkpoint shape %s, module shape %s" % (k, params[k].shape, tuple(p.shape)))
                p.copy_(torch.from_numpy(np.ascontiguousarray(params[k])))
    return missing, unexpected
