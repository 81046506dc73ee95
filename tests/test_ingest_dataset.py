"""DeviceDataset.append_raw, the readers and the feeder over ingested samples, on the GPU: what is stored is tests/ingest_ref.py's
statement of the reference's readers (reader/kitti.py:57-74, reader/hd1k.py:51-78), bit for bit in all four parts; batches cut from
such a data set next to a Sintel-style one are tests/data_ref.py's batches."""
import numpy as np
import pytest

from tests import data_ref, ingest_ref


def _raw_sample(rng, H, W, valid=0.4):
    img1, img2 = (rng.integers(30, 220, (H, W, 3), dtype=np.uint8) for _ in range(2))
    fo = np.zeros((H, W, 3), np.uint16)
    fo[..., :2] = rng.integers(32768 - 6000, 32768 + 6000, (H, W, 2))
    fo[..., 2] = rng.random((H, W)) < valid
    return img1, img2, fo


def _same(got, want, what):
    for g, w, part in zip(got, want, ("img1", "img2", "flow", "mask")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))
        assert bad.size == 0, "%s: %s differs in %d bytes, the first at %d" % (what, part, bad.size, bad[0])


STYLES = {
    # kitti.read_dataset(resize=..., crop=(h, w)): the bottom rows and the left columns, BGR, plain flow
    "kitti": dict(crop=(18, 30), resize=(24, 16), bgr=True, premultiply=False, normalize=False),
    "kitti_uncropped_unresized": dict(crop=None, resize=None, bgr=True, premultiply=False, normalize=False),
    # hd1k.read_dataset(resize=..., normalize=True, crop=(top/bottom, left/right)): margins, the stretch, flow * occ
    "hd1k": dict(crop=((1, 1), (2, 2)), resize=(24, 16), bgr=True, premultiply=True, normalize=True),
    "identity": dict(crop=None, resize=None, bgr=False, premultiply=False, normalize=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("flow_dtype", ("float32", "float16"))
@pytest.mark.parametrize("style", list(STYLES))
def test_gpu_append_raw_stores_the_readers_samples(style, flow_dtype):
    from maskflownet_amd.data import DeviceDataset
    kw = STYLES[style]
    rng = np.random.default_rng(sorted(STYLES).index(style))
    ds = DeviceDataset("cuda", flow_dtype=flow_dtype, chunk_bytes=1 << 20)
    raws = [_raw_sample(rng, 20, 33), _raw_sample(rng, 20, 33, valid=1.0), _raw_sample(rng, 21, 35, valid=0.1)]
    for k, raw in enumerate(raws):
        assert ds.append_raw(*raw, **kw) == k
    assert len(ds) == 3 and ds.has_mask is True
    for k, raw in enumerate(raws):
        want = ingest_ref.sample(*raw, flow_dtype=np.dtype(flow_dtype).type, **kw)
        if kw["resize"] is not None:
            assert ds.shape(k) == (16, 24)
        _same(ds.host(k), want, "%s sample %d" % (style, k))


@pytest.mark.gpu
def test_gpu_append_raw_refuses_what_does_not_fit():
    from maskflownet_amd.data import DeviceDataset
    rng = np.random.default_rng(9)
    img1, img2, fo = _raw_sample(rng, 20, 33)
    ds = DeviceDataset("cuda")
    with pytest.raises(ValueError, match="uint16"):
        ds.append_raw(img1, img2, fo.astype(np.float32))
    with pytest.raises(ValueError, match="img2"):
        ds.append_raw(img1, img2[:19], fo)
    with pytest.raises(ValueError, match="does not fit"):
        ds.append_raw(img1, img2, fo, crop=(21, 30))
    with pytest.raises(ValueError, match="does not fit"):
        ds.append_raw(img1, img2, fo, crop=((10, 10), (2, 2)))
    with pytest.raises(ValueError, match="at least 2"):
        ds.append_raw(img1, img2, fo, crop=(1, 30))
    assert len(ds) == 0
    plain = DeviceDataset("cuda")
    plain.append(img1, img2, np.zeros((20, 33, 2), np.float32))
    with pytest.raises(ValueError, match="no masks"):
        plain.append_raw(img1, img2, fo)


@pytest.mark.gpu
def test_gpu_feeder_mixes_an_ingested_and_a_stored_data_set():
    """main.py:244-260's mixed batch: one slot from a data set built by append_raw (KITTI), one from append with masks (Sintel)."""
    from maskflownet_amd.data import BatchSampler, DeviceDataset, Feeder
    rng = np.random.default_rng(10)
    kitti, sintel = DeviceDataset("cuda", flow_dtype="float16"), DeviceDataset("cuda")
    for _ in range(3):
        kitti.append_raw(*_raw_sample(rng, 22, 37), crop=(20, 36), resize=(40, 24))
        img1, img2 = (rng.integers(0, 256, (26, 44, 3), dtype=np.uint8) for _ in range(2))
        sintel.append(img1, img2, (rng.standard_normal((26, 44, 2)) * 9).astype(np.float32), rng.integers(0, 2, (26, 44, 1), dtype=np.uint8) * 255)
    hosts = {id(kitti): [kitti.host(i) for i in range(3)], id(sintel): [sintel.host(i) for i in range(3)]}
    slots = [kitti, sintel, kitti, sintel]
    feed = Feeder(BatchSampler(slots, (24, 32), seed=3))
    for _ in range(3):
        got = feed.next()
        draw = feed.last_draw
        samples = [hosts[id(ds)][d[0]] for ds, d in zip(slots, draw)]
        want = data_ref.gather_batch(samples, (24, 32), [d[1:] for d in draw], True)
        for g, w, name in zip(got, want, ("img1", "img2", "label", "mask")):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and (g.view(np.uint8) == w.view(np.uint8)).all(), name


@pytest.mark.gpu
def test_gpu_readers_feed_append_raw(tmp_path):
    """readers.kitti_samples / hd1k_samples / sintel_samples over directories of files written by io.write_png and io.write_flo."""
    from maskflownet_amd import io, readers
    from maskflownet_amd.data import DeviceDataset
    rng = np.random.default_rng(11)
    images, flows = tmp_path / "image_2", tmp_path / "flow_occ"
    images.mkdir()
    flows.mkdir()
    raws = {}
    for k in (0, 3):
        raws[k] = _raw_sample(rng, 20, 33)
        io.write_png(str(images / ("%06d_10.png" % k)), raws[k][0])
        io.write_png(str(images / ("%06d_11.png" % k)), raws[k][1])
        io.write_png(str(flows / ("%06d_10.png" % k)), raws[k][2])
    ds = DeviceDataset("cuda")
    for s in readers.kitti_samples(str(images), str(flows), [3, 0]):
        ds.append_raw(*s, crop=(18, 30), resize=(24, 16))
    for i, k in enumerate((3, 0)):
        _same(ds.host(i), ingest_ref.sample(*raws[k], crop=(18, 30), resize=(24, 16)), "kitti file %d" % k)
    # HD1K: the flow map's stem names the first frame, the second is the next one
    himg, hflow = tmp_path / "hd1k_image", tmp_path / "hd1k_flow"
    himg.mkdir()
    hflow.mkdir()
    raw = _raw_sample(rng, 20, 33)
    io.write_png(str(himg / "000002_0009.png"), raw[0])
    io.write_png(str(himg / "000002_0010.png"), raw[1])
    io.write_png(str(hflow / "000002_0009.png"), raw[2])
    kw = dict(crop=((1, 1), (2, 2)), resize=(24, 16), premultiply=True, normalize=True)
    hd = DeviceDataset("cuda")
    for s in readers.hd1k_samples(str(himg), str(hflow), ["000002_0009"]):
        hd.append_raw(*s, **kw)
    _same(hd.host(0), ingest_ref.sample(*raw, **kw), "hd1k file")
    # Sintel: stored as read, mask = 255 - invalid
    root = tmp_path / "sintel"
    for kind in ("clean", "flow", "invalid"):
        (root / "training" / kind / "alley_1").mkdir(parents=True)
    f1, f2 = (rng.integers(0, 256, (12, 20, 3), dtype=np.uint8) for _ in range(2))
    flow = rng.standard_normal((12, 20, 2)).astype(np.float32)
    invalid = (rng.random((12, 20)) < 0.2).astype(np.uint8) * 255
    io.write_png(str(root / "training" / "clean" / "alley_1" / "frame_0007.png"), f1)
    io.write_png(str(root / "training" / "clean" / "alley_1" / "frame_0008.png"), f2)
    io.write_flo(str(root / "training" / "flow" / "alley_1" / "frame_0007.flo"), flow)
    io.write_png(str(root / "training" / "invalid" / "alley_1" / "frame_0007.png"), invalid)
    st = DeviceDataset("cuda")
    st.extend(readers.sintel_samples(str(root), "clean", [("alley_1", 7)]))
    _same(st.host(0), (f1, f2, flow, (255 - invalid)[..., None]), "sintel entry")


def test_readers_decode_without_a_gpu(tmp_path):
    """The readers themselves are host code: the same KITTI directory read back on the CPU."""
    from maskflownet_amd import io, readers
    rng = np.random.default_rng(12)
    raw = _raw_sample(rng, 9, 14)
    for name, a in (("000005_10.png", raw[0]), ("000005_11.png", raw[1])):
        io.write_png(str(tmp_path / name), a)
    (tmp_path / "flow").mkdir()
    io.write_png(str(tmp_path / "flow" / "000005_10.png"), raw[2])
    (got,) = list(readers.kitti_samples(str(tmp_path), str(tmp_path / "flow"), [5]))
    assert all(g.dtype == w.dtype and (g == w).all() for g, w in zip(got, raw))
