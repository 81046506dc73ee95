"""maskflownet_amd.predict on uint8 frames end to end (GPU): Predictor.do_batch_u8 / predict_frames and the command line, at the fixture
sizes of tests/test_predict_pipeline.py (100x180 -> 128x192, MaskFlownet-S, seeded parameters) and against that file's CPU reference
path fed bytes / 255, within that file's bars."""
import os

import numpy as np
import pytest

from oracle import network_ref as nr
from tests import predict_ref as pr
from tests import test_predict_pipeline as tp

pytestmark = pytest.mark.gpu

H, W = tp.H, tp.W


def to_bytes(im):
    """(n,3,H,W) in [0,1] -> (n,H,W,3) uint8, round(255 * image)."""
    return np.ascontiguousarray(np.round(im * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))


@pytest.fixture(scope="module")
def small(oracle):
    """Frames, parameters, the CPU result on bytes / 255 and one Predictor of batch 2: made once, left unchanged."""
    from maskflownet_amd import predict
    im1, im2 = tp.images(2)
    frames = np.concatenate([to_bytes(im1), to_bytes(im2)])          # pair k is (frames[k], frames[2 + k])
    fl = (frames.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
    P = nr.Params(seed=7)
    ref = tp.cpu_path(nr.Net, P, np.ascontiguousarray(fl[:2]), np.ascontiguousarray(fl[2:]), oracle)
    rng = np.random.default_rng(5)
    label = (ref["flow"] + 2.0 * rng.standard_normal(ref["flow"].shape)).astype(np.float32)
    mask = (rng.uniform(size=(2, 1, H, W)) < 0.7).astype(np.float32)
    for a in list(ref.values()) + [frames]:
        a.setflags(write=False)
    return {"frames": frames, "P": P, "ref": ref, "label": label, "mask": mask, "p": predict.Predictor(P.store, 2, H, W)}


def test_do_batch_u8_against_the_cpu_reference_path(small):
    import torch
    ref, p = small["ref"], small["p"]
    dev = torch.from_numpy(small["frames"].copy()).cuda()
    got = tp.to_np(p.do_batch_u8(dev, 0, 2, 2, small["label"], small["mask"]))
    assert got["flow"].shape == (2, 2, H, W) and got["occ_mask"].shape == (2, 1, H, W) and got["warped"].shape == (2, 3, H, W)
    d = nr.epe_delta({"flow_full": got["flow"]}, {"flow_full": ref["flow"]})
    m = pr.flow_metrics(ref["flow"], small["label"], small["mask"])["sums"]
    epe_ref = m[:, 0] / m[:, 1]
    e_warp = np.abs(got["warped"] - ref["warped"]).max() / np.abs(ref["warped"]).max()
    e_occ = np.abs(got["occ_mask"] - ref["occ_mask"]).max()
    e_epe = np.abs(got["epe"] - epe_ref).max() / epe_ref.min()
    print("do_batch_u8 %dx%d vs CPU path: %r; warped %.2e (rel), occ_mask %.2e, epe %.2e (rel)" % (H, W, d, e_warp, e_occ, e_epe))
    assert d["mean_flow_px"] > 0.1
    assert d["epe_delta_rel"] <= 1e-4, d
    assert e_warp <= 5e-4
    assert e_occ <= 1e-4
    assert e_epe <= 1e-4
    again = tp.to_np(p.do_batch_u8(dev, 0, 2, 2, small["label"], small["mask"]))
    for k in got:
        np.testing.assert_array_equal(again[k], got[k], err_msg=k)
    bare = p.do_batch_u8(dev, 0, 2, 2, warped=False)
    assert bare["warped"] is None and bare["epe"] is None and bare["fl"] is None
    np.testing.assert_array_equal(bare["flow"].cpu().numpy(), got["flow"])
    # a short batch repeats its last pair by index arithmetic: the pair's result is the one it has in a full batch
    short = tp.to_np(p.do_batch_u8(dev, 1, 3, 1))
    for k in ("flow", "occ_mask", "warped"):
        np.testing.assert_array_equal(short[k][0], got[k][1], err_msg=k)
    with pytest.raises(ValueError):
        p.do_batch_u8(dev, 0, 1, 3)
    with pytest.raises(Exception, match="a0 \\+ N"):
        p.do_batch_u8(dev, 3, 0, 2)


def test_predict_frames_uploads_every_frame_once(small):
    """4 frames, batch 2: pairs (0,1), (1,2) and the short batch (2,3); bit-identical to do_batch_u8 on the explicit pairs."""
    import torch
    from maskflownet_amd import ops
    p, frames = small["p"], small["frames"]
    before = p.frames_uploaded
    outs = list(p.predict_frames(iter(frames), color=True, warped=True))
    assert p.frames_uploaded - before == 4 and len(outs) == 3
    dev = torch.from_numpy(frames.copy()).cuda()
    first = tp.to_np(p.do_batch_u8(dev, 0, 1, 2))
    last = tp.to_np(p.do_batch_u8(dev, 2, 3, 1))
    for k, (flow, occ, warped, rgb) in enumerate(outs):
        want = first if k < 2 else last
        j = k if k < 2 else 0
        assert flow.shape == (H, W, 2) and occ.shape == (H, W, 1) and warped.shape == (H, W, 3) and rgb.shape == (H, W, 3)
        assert flow.dtype == occ.dtype == warped.dtype == np.float32 and rgb.dtype == np.uint8
        np.testing.assert_array_equal(flow[..., 0], want["flow"][j, 1])      # (u, v): the network's (dy, dx) reversed
        np.testing.assert_array_equal(flow[..., 1], want["flow"][j, 0])
        np.testing.assert_array_equal(occ[..., 0], want["occ_mask"][j, 0])
        np.testing.assert_array_equal(warped, want["warped"][j].transpose(1, 2, 0))
        net_order = torch.from_numpy(np.ascontiguousarray(flow[..., ::-1].transpose(2, 0, 1))[None]).cuda()
        np.testing.assert_array_equal(rgb, ops.flow_color(net_order)[0].cpu().numpy())
    assert np.abs(outs[2][0] - outs[0][0]).max() > 1e-3                       # the third pair is another pair
    plain = list(p.predict_frames(list(frames[:3])))                          # no colours, no warp: 3-tuples
    assert len(plain) == 2 and len(plain[0]) == 3 and plain[0][2] is None
    np.testing.assert_array_equal(plain[1][0], outs[1][0])
    fixed = list(p.predict_frames(list(frames[:2]), color=True, rad_max=3.0, bgr=True))
    net_order = torch.from_numpy(np.ascontiguousarray(fixed[0][0][..., ::-1].transpose(2, 0, 1))[None]).cuda()
    np.testing.assert_array_equal(fixed[0][3], ops.flow_color(net_order, rad_max=3.0, bgr=True)[0].cpu().numpy())
    with pytest.raises(ValueError):
        list(p.predict_frames([frames[0]]))


def test_command_line_writes_the_device_colours(small, tmp_path):
    from maskflownet_amd import io, predict
    frames = small["frames"]
    params = str(tmp_path / "net.params")
    io.save_params(params, small["P"].store)
    src = tmp_path / "frames"
    os.makedirs(src)
    for k in range(3):
        io.write_png(str(src / ("f%02d.png" % k)), frames[k])
    bgr = [np.ascontiguousarray(f[..., ::-1]) for f in frames[:3]]           # what cv2.imread hands the reference
    # a directory of three frames: two pictures, from a Predictor of batch 2 like the fixture's
    out_dir = tmp_path / "out"
    assert predict.main([str(out_dir), "--params", params, "--frames", str(src)]) == 0
    want = [o[3] for o in small["p"].predict_frames(bgr, color=True)]
    assert sorted(os.listdir(out_dir)) == ["000000.png", "000001.png"]
    for k in range(2):
        np.testing.assert_array_equal(io.read_png(str(out_dir / ("%06d.png" % k))), want[k])
    # an image pair with one scale given: one picture, from a Predictor of batch 1
    out = tmp_path / "pair.png"
    assert predict.main([str(out), "--params", params, "--image_1", str(src / "f00.png"), "--image_2", str(src / "f01.png"),
                         "--rad_max", "4.5"]) == 0
    one = predict.Predictor(small["P"].store, 1, H, W)
    (flow, occ, warped, rgb), = one.predict_frames(bgr[:2], color=True, rad_max=4.5)
    got = io.read_png(str(out))
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, rgb)
    assert warped is None and one.frames_uploaded == 2
