"""maskflownet_amd.predict.Predictor end to end (GPU): images whose size is no multiple of 64 through centralize -> resize ->
network (one hipGraph) -> Upsample(4) -> resize back + rescale -> clipped warp -> masked EPE, against the same sequence on the CPU:
numpy centralize, tests/predict_ref.py's fp32 resize, oracle/network_ref.py with the oracle's operators."""
import numpy as np
import pytest

from oracle import network_ref as nr
from tests import predict_ref as pr

pytestmark = pytest.mark.gpu

H, W, H64, W64 = 100, 180, 128, 192
OFFSET = np.array([0.45, 0.5, 0.4], np.float32).reshape(1, 3, 1, 1)


def images(N, seed=20260925):
    """nr.synthetic_pair with a per-channel constant added back: centralizing is no no-op, the images lie in [0, 1]."""
    c1, c2 = nr.synthetic_pair(N, H, W, seed=seed)
    return np.clip(c1 + OFFSET, 0.0, 1.0).astype(np.float32), np.clip(c2 + OFFSET, 0.0, 1.0).astype(np.float32)


def centralize(im1, im2):
    mean = np.concatenate([im1, im2], axis=2).mean(axis=(2, 3), dtype=np.float64).astype(np.float32).reshape(-1, 3, 1, 1)
    return im1 - mean, im2 - mean


def cpu_path(net_cls, params, im1, im2, oracle):
    """The reference's do_batch on the CPU -> dict(flow, occ_mask, warped) at H x W."""
    c1, c2 = centralize(im1, im2)
    out = net_cls(params, nr.OracleMatching(), "cpu").forward(pr.resize(c1, H64, W64, dtype=np.float32),
                                                               pr.resize(c2, H64, W64, dtype=np.float32))
    head = out.get("head", out)
    flow = pr.resize(out["flow_full"], H, W, dtype=np.float32, flow_rescale=True)
    occ = pr.resize(oracle.upsample(np.ascontiguousarray(head["occlusion"]), 4), H, W, dtype=np.float32)
    return {"flow": flow, "occ_mask": occ, "warped": oracle.warp(im2, flow, clip_grid=True)}


def to_np(out):
    return {k: (v.cpu().numpy().copy() if v is not None else None) for k, v in out.items()}


@pytest.fixture(scope="module")
def small(oracle):
    """Parameters, inputs and the CPU result of the MaskFlownet-S case, computed once and left unchanged."""
    im1, im2 = images(2)
    P = nr.Params(seed=7)
    ref = cpu_path(nr.Net, P, im1, im2, oracle)       # creates every parameter
    rng = np.random.default_rng(5)
    label = (ref["flow"] + 2.0 * rng.standard_normal(ref["flow"].shape)).astype(np.float32)
    mask = (rng.uniform(size=(2, 1, H, W)) < 0.7).astype(np.float32)
    for a in ref.values():
        a.setflags(write=False)
    return {"im1": im1, "im2": im2, "P": P, "ref": ref, "label": label, "mask": mask}


def test_predictor_against_the_cpu_reference_path(small):
    from maskflownet_amd import predict
    ref = small["ref"]
    p = predict.Predictor(small["P"].store, 2, H, W)
    assert (p.H64, p.W64) == (H64, W64) and p.resized
    got = to_np(p.do_batch(small["im1"], small["im2"], small["label"], small["mask"]))
    assert got["flow"].shape == (2, 2, H, W) and got["occ_mask"].shape == (2, 1, H, W) and got["warped"].shape == (2, 3, H, W)
    d = nr.epe_delta({"flow_full": got["flow"]}, {"flow_full": ref["flow"]})
    m = pr.flow_metrics(ref["flow"], small["label"], small["mask"])["sums"]
    epe_ref = m[:, 0] / m[:, 1]
    e_warp = np.abs(got["warped"] - ref["warped"]).max() / np.abs(ref["warped"]).max()
    e_occ = np.abs(got["occ_mask"] - ref["occ_mask"]).max()
    e_epe = np.abs(got["epe"] - epe_ref).max() / epe_ref.min()
    print("Predictor %dx%d vs CPU path: %r; warped %.2e (rel), occ_mask %.2e, epe %.2e (rel)" % (H, W, d, e_warp, e_occ, e_epe))
    assert d["mean_flow_px"] > 0.1
    assert d["epe_delta_rel"] <= 1e-4, d
    assert e_warp <= 5e-4
    assert e_occ <= 1e-4
    assert e_epe <= 1e-4
    assert got["fl"].shape == (2,) and np.isfinite(got["fl"]).all()
    again = to_np(p.do_batch(small["im1"], small["im2"], small["label"], small["mask"]))     # the captured graph, a second time
    for k in got:
        np.testing.assert_array_equal(again[k], got[k], err_msg=k)
    without = p.do_batch(small["im1"], small["im2"])
    assert without["epe"] is None and without["fl"] is None
    np.testing.assert_array_equal(without["flow"].cpu().numpy(), got["flow"])


def test_full_model_predictor_flow(oracle):
    from maskflownet_amd import predict
    im1, im2 = images(1, seed=11)
    P = nr.Params(seed=11)
    ref = cpu_path(nr.NetFull, P, im1, im2, oracle)
    got = to_np(predict.Predictor(P.store, 1, H, W, full=True).do_batch(im1, im2))
    d = nr.epe_delta({"flow_full": got["flow"]}, {"flow_full": ref["flow"]})
    print("full-model Predictor vs CPU path: %r" % (d,))
    assert d["mean_flow_px"] > 0.1 and d["epe_delta_rel"] <= 1e-4, d


def test_no_resize_is_the_network_on_the_centralized_pair(small):
    """128 x 192: preprocessing only centralizes (exactly x - mean), no resize back: the network's own flow, bit for bit."""
    import torch
    from maskflownet_amd import network, ops, predict
    rng = np.random.default_rng(2)
    im1, im2 = (rng.uniform(0, 1, (2, 3, H64, W64)).astype(np.float32) for _ in range(2))
    p = predict.Predictor(small["P"].store, 2, H64, W64)
    assert not p.resized
    flow = p.do_batch(im1, im2)["flow"].clone()
    d1, d2 = torch.from_numpy(im1).cuda(), torch.from_numpy(im2).cuda()
    mean = ops.pair_mean(d1, d2)[:, :, None, None]
    net = network.MaskFlownetS(small["P"].store, 2, H64, W64)
    assert torch.equal(net(d1 - mean, d2 - mean)["flow_full"], flow)


def test_predict_generator_short_last_batch_and_flo_round_trip(small, tmp_path):
    from maskflownet_amd import io, predict
    im1, im2 = images(3, seed=4)
    u8 = lambda a: [np.ascontiguousarray(np.round(x * 255.0).astype(np.uint8).transpose(1, 2, 0)) for x in a]
    a, b = u8(im1), u8(im2)
    p = predict.Predictor(small["P"].store, 2, H, W)
    outs = list(p.predict(a, b))                       # batches (0, 1) and (2, padding)
    assert len(outs) == 3
    for flow, occ, warped in outs:
        assert flow.shape == (H, W, 2) and occ.shape == (H, W, 1) and warped.shape == (H, W, 3)
        assert flow.dtype == occ.dtype == warped.dtype == np.float32
    first = list(p.predict([a[2], a[0]], [b[2], b[0]]))[0]
    for x, y in zip(outs[2], first):
        np.testing.assert_array_equal(x, y)             # a pair's result does not depend on its place or on the padding
    assert np.abs(outs[2][0] - outs[0][0]).max() > 1e-3   # ... and the third pair is another pair
    # (u, v) order: the last axis is the network's (dy, dx) reversed
    raw = p.do_batch(np.stack([x.transpose(2, 0, 1) for x in a[:2]]).astype(np.float32) / np.float32(255.0),
                     np.stack([x.transpose(2, 0, 1) for x in b[:2]]).astype(np.float32) / np.float32(255.0))["flow"].cpu().numpy()
    np.testing.assert_array_equal(outs[1][0][..., 0], raw[1, 1])
    np.testing.assert_array_equal(outs[1][0][..., 1], raw[1, 0])
    path = str(tmp_path / "pair2.flo")
    io.write_flo(path, outs[2][0])
    np.testing.assert_array_equal(io.read_flo(path), outs[2][0])
    # validate(): labels in (u, v) order, flipped inside; the mean over the set of the per-pair figures
    labels = [f + 1.0 for f, _, _ in outs]
    masks = [np.full((H, W, 1), 255, np.uint8)] * 3
    epe = p.validate(a, b, labels, masks)
    assert abs(epe - np.sqrt(2.0 + 1e-8)) <= 1e-5 * np.sqrt(2.0), epe     # |(1, 1)| at every pixel
    assert p.validate(a, b, labels, return_type="fl") == 0.0                # nowhere above 3 px
