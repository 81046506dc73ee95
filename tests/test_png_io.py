"""maskflownet_amd/io.py's PNG codec (read_png on zlib + mfn_png_unfilter, write_png, write_kitti_flow, read_sintel_invalid), on the CPU.

The decoder is tested against an ENCODER of this file's own: forward filtering of a row needs only the original bytes of the row and
of the one above, so each of the five filters is a few numpy lines that share nothing with the decoder; chunks and CRCs are written
here too.  Every row gets a randomly chosen filter and the zlib stream is split over two IDAT chunks."""
import struct
import zlib

import numpy as np
import pytest

from maskflownet_amd import _lib, io


@pytest.fixture(scope="module", autouse=True)
def built():
    _lib.build()


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _filter_row(kind, cur, up, bpp):
    """One scanline filtered forwards (PNG specification, section 9): cur, up int64 arrays of the row's original bytes."""
    def shifted(row):                        # the byte one pixel to the left; zeros in front of the first pixel
        out = np.zeros_like(row)
        out[bpp:] = row[:max(row.size - bpp, 0)]
        return out
    left, upleft = shifted(cur), shifted(up)
    if kind == 0:
        pred = np.zeros_like(cur)
    elif kind == 1:
        pred = left
    elif kind == 2:
        pred = up
    elif kind == 3:
        pred = (left + up) // 2
    else:
        p = left + up - upleft
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
        pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    return ((cur - pred) % 256).astype(np.uint8)


def encode_png(array, filters, split=True, interlace=0, ctype=None):
    a = np.asarray(array)
    h, w = a.shape[:2]
    C = 1 if a.ndim == 2 else a.shape[2]
    item = a.dtype.itemsize
    rows = a.reshape(h, w * C).astype(">u2" if item == 2 else np.uint8).view(np.uint8).reshape(h, -1).astype(np.int64)
    bpp = C * item
    raw = bytearray()
    for y in range(h):
        up = rows[y - 1] if y else np.zeros_like(rows[0])
        raw.append(int(filters[y]))
        raw += _filter_row(int(filters[y]), rows[y], up, bpp).tobytes()
    z = zlib.compress(bytes(raw), 9)
    cut = len(z) // 2 if split else len(z)
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[C] if ctype is None else ctype
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8 * item, ctype, 0, 0, interlace))
    out += _chunk(b"tEXt", b"Comment\x00an ancillary chunk the reader skips")
    out += _chunk(b"IDAT", z[:cut]) + (_chunk(b"IDAT", z[cut:]) if split else b"") + _chunk(b"IEND", b"")
    return out


def _random_image(rng, h, w, C, dtype):
    hi = 256 if dtype == np.uint8 else 65536
    a = rng.integers(0, hi, (h, w, C), dtype=dtype)
    if h > 2 and w > 2:                      # smooth stretches too: filters whose predictions are mostly right
        a[h // 2:] = (np.arange(w)[None, :, None] * 3 + np.arange(h - h // 2)[:, None, None] * 5) % hi
    return a[..., 0] if C == 1 else a


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
@pytest.mark.parametrize("C", (1, 3, 2, 4))
@pytest.mark.parametrize("hw", ((1, 1), (7, 5), (33, 17)))
def test_read_png_decodes_every_filter(tmp_path, hw, C, dtype):
    rng = np.random.default_rng(hw[0] * 100 + C * 10 + np.dtype(dtype).itemsize)
    a = _random_image(rng, hw[0], hw[1], C, dtype)
    plans = [rng.integers(0, 5, hw[0])] + [np.full(hw[0], k) for k in range(5)]
    for n, filters in enumerate(plans):
        path = tmp_path / ("f%d.png" % n)
        path.write_bytes(encode_png(a, filters))
        got = io.read_png(str(path))
        assert got.dtype == dtype and got.shape == a.shape, (got.dtype, got.shape)
        assert (got == a).all(), "filters %s" % (filters,)


def test_read_png_refuses_what_it_does_not_read(tmp_path):
    a = np.zeros((4, 4, 3), np.uint8)
    good = encode_png(a, [0] * 4)
    cases = {"interlaced": encode_png(a, [0] * 4, interlace=1), "palette": encode_png(a[..., 0], [0] * 4, ctype=3),
             "not a PNG": b"P6 4 4 255\n" + bytes(48), "bad CRC": good[:40] + bytes([good[40] ^ 1]) + good[41:], "truncated": good[:-20]}
    for text, blob in cases.items():
        path = tmp_path / "bad.png"
        path.write_bytes(blob)
        with pytest.raises(ValueError, match={"interlaced": "interlaced", "palette": "palette", "not a PNG": "not a PNG", "bad CRC": "CRC",
                                              "truncated": "truncated|needs"}[text]):
            io.read_png(str(path))
    rows = bytearray(4 * 13)                 # four scanlines of a filter byte and twelve data bytes
    rows[13] = 7                             # the second row's filter type
    blob = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 4, 4, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(bytes(rows))) + _chunk(b"IEND", b"")
    (tmp_path / "filter.png").write_bytes(blob)
    with pytest.raises(RuntimeError, match="row 1"):
        io.read_png(str(tmp_path / "filter.png"))


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
@pytest.mark.parametrize("C", (1, 2, 3, 4))
def test_write_png_round_trip(tmp_path, C, dtype):
    rng = np.random.default_rng(C)
    a = _random_image(rng, 9, 14, C, dtype)
    io.write_png(str(tmp_path / "a.png"), a)
    got = io.read_png(str(tmp_path / "a.png"))
    assert got.dtype == dtype and got.shape == a.shape and (got == a).all()
    with pytest.raises(ValueError, match="write_png"):
        io.write_png(str(tmp_path / "b.png"), a.astype(np.float32))


def test_pil_files_are_read_and_written_files_open_in_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for C in (3, 1):
        a = _random_image(rng, 21, 34, C, np.uint8)
        Image.fromarray(a).save(str(tmp_path / "pil.png"))          # PIL picks its own filters per row
        assert (io.read_png(str(tmp_path / "pil.png")) == a).all()
        io.write_png(str(tmp_path / "own.png"), a)
        assert (np.asarray(Image.open(str(tmp_path / "own.png"))) == a).all()


def test_write_kitti_flow_round_trip(tmp_path):
    """predict.py:63-66: the file decodes (kitti.py:61-63) to the flow quantised to 1/64 px, truncating, with every pixel valid."""
    rng = np.random.default_rng(6)
    flow = (rng.standard_normal((12, 19, 2)) * 60).astype(np.float32)
    flow[0, 0], flow[0, 1], flow[0, 2] = (-512, 511.984375), (0, -0.01), (1 / 64, 1 / 128)
    io.write_kitti_flow(str(tmp_path / "000000_10.png"), flow)
    raw = io.read_png(str(tmp_path / "000000_10.png"))
    assert raw.dtype == np.uint16 and raw.shape == (12, 19, 3) and (raw[..., 2] == 1).all()
    want = np.floor(64.0 * (flow.astype(np.float64) + 512.0))
    assert (raw[..., :2] == want).all()
    decoded = (raw[..., :2].astype(np.float32) - 32768.) / 64.
    assert (decoded == np.floor(flow.astype(np.float64) * 64) / 64).all()
    with pytest.raises(ValueError, match="write_kitti_flow"):
        io.write_kitti_flow(str(tmp_path / "x.png"), flow[..., 0])


def test_read_sintel_invalid(tmp_path):
    rng = np.random.default_rng(7)
    gray = (rng.random((10, 13)) < 0.3).astype(np.uint8) * 255
    io.write_png(str(tmp_path / "frame_0001.png"), gray)
    mask = io.read_sintel_invalid(str(tmp_path / "frame_0001.png"))
    assert mask.dtype == np.uint8 and mask.shape == (10, 13, 1) and (mask[..., 0] == 255 - gray).all()
    io.write_png(str(tmp_path / "rgb.png"), np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="gray"):
        io.read_sintel_invalid(str(tmp_path / "rgb.png"))
