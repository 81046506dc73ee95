"""Validation during training (GPU): predict.Predictor.validate_dataset on a data.DeviceDataset, the weights of a captured network
replaced in place (network.MaskFlownetS.load_weights, Predictor.load_weights), and training.Validation on top of both.

Bars.  validate_dataset against do_batch_u8 on the same frames stacked, the label and the mask handed over as the fp32 tensors the host
path makes: bit-identical per sample, the short batch included (the kernels of validate.h give the bits of the operators do_batch_u8
runs; tests/test_validate_ops.py).  Against Predictor.validate on host lists: 1e-4 relative, the bar tests/test_predict_frames.py holds
the byte path to -- the joint mean of the float path is one fp32 rounding away from the exact one.  A refreshed network against a
freshly built one: bit-identical flows."""
import numpy as np
import pytest

from oracle import network_ref as nr
from tests.test_predict_pipeline import H, W, images

pytestmark = pytest.mark.gpu

S, BATCH = 3, 2          # one full batch and one short batch


def reference_params(seed, full=False):
    """nr.Params(seed) with every layer of the model drawn: a layer's draw depends on (seed, name, shape) alone."""
    from maskflownet_amd import network
    P = nr.Params(seed=seed)
    for name, ws, bs in (network.layer_shapes_full() if full else network.layer_shapes()):
        P.get(name + ".weight", ws)
        P.get(name + ".bias", bs)
    return dict(P.store)


@pytest.fixture(scope="module")
def data():
    """S samples of 100 x 180 as the readers store them, resident on the device, and the same on the host; left unchanged."""
    import torch
    from maskflownet_amd import data as mdata
    im1, im2 = images(S)
    u8 = lambda a: np.ascontiguousarray(np.round(a * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))
    img1, img2 = u8(im1), u8(im2)
    rng = np.random.default_rng(17)
    flow = (3.0 * rng.standard_normal((S, H, W, 2))).astype(np.float32)               # (u, v)
    mask = rng.choice(np.array([0, 128, 255, 255, 255], np.uint8), (S, H, W, 1))
    ds = mdata.DeviceDataset("cuda")
    for k in range(S):
        ds.append(img1[k], img2[k], flow[k], mask[k])
    torch.cuda.synchronize()
    for a in (img1, img2, flow, mask):
        a.setflags(write=False)
    return {"ds": ds, "img1": img1, "img2": img2, "flow": flow, "mask": mask, "P": reference_params(7)}


@pytest.fixture(scope="module")
def predictor(data):
    from maskflownet_amd import predict
    return predict.Predictor(data["P"], BATCH, H, W)


def test_validate_dataset_is_do_batch_u8_per_sample_and_validate_for_the_set(data, predictor):
    import torch
    p = predictor
    got = p.validate_dataset(data["ds"])
    per = got["per_sample"]
    assert per.shape == (S, 2) and per.dtype == np.float32 and np.isfinite(per).all()
    assert got["epe"] == float(np.mean(per[:, 0])) and got["fl"] == float(np.mean(per[:, 1]))
    # the same frames stacked, the label flipped to (dy, dx) as CHW fp32 and the mask / 255: what the host path uploads
    frames = torch.from_numpy(np.concatenate([data["img1"], data["img2"]])).cuda()
    label = np.ascontiguousarray(data["flow"][..., ::-1].transpose(0, 3, 1, 2))
    mask = np.ascontiguousarray((data["mask"].astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    want = []
    for j in range(0, S, BATCH):
        n = min(BATCH, S - j)
        out = p.do_batch_u8(frames, j, S + j, n, label=label[j:j + n], mask=mask[j:j + n], warped=False)
        want.append(np.stack([out["epe"].cpu().numpy(), out["fl"].cpu().numpy()], axis=1))
    want = np.concatenate(want)
    print("per sample (epe, fl):", per.tolist(), "do_batch_u8:", want.tolist())
    assert np.array_equal(per.view(np.uint32), want.view(np.uint32))
    assert (per[:, 1] > 0).any() and (per[:, 1] < 1).any()         # the outlier ratio is exercised
    # the host path of today
    host = p.validate(list(data["img1"]), list(data["img2"]), list(data["flow"]), list(data["mask"]))
    print("set epe: validate_dataset %.9g, validate %.9g" % (got["epe"], host))
    assert abs(got["epe"] - host) <= 1e-4 * abs(host)
    host_fl = p.validate(list(data["img1"]), list(data["img2"]), list(data["flow"]), list(data["mask"]), return_type="fl")
    assert abs(got["fl"] - host_fl) <= 1e-4 * abs(host_fl) + 1.0 / (H * W)      # one pixel may change sides of the outlier bar
    # again: the same bits
    again = p.validate_dataset(data["ds"])
    assert np.array_equal(again["per_sample"].view(np.uint32), per.view(np.uint32)) and again["epe"] == got["epe"]
    # a selection, in another order
    some = p.validate_dataset(data["ds"], indices=[2, 0])
    assert np.array_equal(some["per_sample"].view(np.uint32), per[[2, 0]].view(np.uint32))


def test_a_set_without_masks_counts_every_pixel(data, predictor):
    from maskflownet_amd import data as mdata
    ds = mdata.DeviceDataset("cuda", flow_dtype="float16")
    for k in range(2):
        ds.append(data["img1"][k], data["img2"][k], data["flow"][k])
    assert ds.has_mask is False
    got = predictor.validate_dataset(ds)
    half = [f.astype(np.float16).astype(np.float32) for f in data["flow"][:2]]
    host = predictor.validate(list(data["img1"][:2]), list(data["img2"][:2]), half)
    assert abs(got["epe"] - host) <= 1e-4 * abs(host)


def test_a_sample_of_another_size_is_refused(data, predictor):
    from maskflownet_amd import data as mdata
    ds = mdata.DeviceDataset("cuda")
    ds.append(data["img1"][0], data["img2"][0], data["flow"][0], data["mask"][0])
    ds.append(data["img1"][1][:, :-4], data["img2"][1][:, :-4], data["flow"][1][:, :-4], data["mask"][1][:, :-4])
    with pytest.raises(ValueError, match="sample 1 is 100x176"):
        predictor.validate_dataset(ds)
    assert predictor.validate_dataset(ds, indices=[0])["per_sample"].shape == (1, 2)
    with pytest.raises(ValueError, match="no samples"):
        predictor.validate_dataset(ds, indices=[])


def test_one_synchronisation_and_one_download_per_set(data, predictor, monkeypatch):
    import torch
    counts = {"sync": 0, "cpu": 0}
    stream_sync, device_sync, to_cpu = torch.cuda.Stream.synchronize, torch.cuda.synchronize, torch.Tensor.cpu

    def count(key, fn):
        def wrapped(*a, **k):
            counts[key] += 1
            return fn(*a, **k)
        return wrapped
    predictor.validate_dataset(data["ds"])          # the table is built and uploaded by the first call
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", count("sync", stream_sync))
    monkeypatch.setattr(torch.cuda, "synchronize", count("sync", device_sync))
    monkeypatch.setattr(torch.Tensor, "cpu", count("cpu", to_cpu))
    rows = predictor._val_rows
    got = predictor.validate_dataset(data["ds"])
    monkeypatch.undo()
    assert counts == {"sync": 1, "cpu": 1}, counts
    assert predictor._val_rows is rows and rows.N == 4       # one table for the set: ceil(3 / 2) * 2 rows, kept
    assert got["per_sample"].shape == (S, 2)


# ---- new weights under the captured graph ----------------------------------------------------------------------------------------------
def _addresses(net):
    return {k: v.data_ptr() for k, v in net.P.items()}, {k: pk.buf.data_ptr() for k, pk in net._packed.items()}


@pytest.mark.parametrize("full", [False, True])
def test_load_weights_is_a_fresh_predictor_at_the_old_addresses(data, full):
    import torch
    from maskflownet_amd import predict
    A, B = reference_params(7, full), reference_params(8, full)
    frames = torch.from_numpy(np.concatenate([data["img1"][:BATCH], data["img2"][:BATCH]])).cuda()
    flow_of = lambda p: p.do_batch_u8(frames, 0, BATCH, BATCH, warped=False)["flow"].cpu().numpy().copy()
    p = predict.Predictor(A, BATCH, H, W, full=full)
    flow_a = flow_of(p)
    where = _addresses(p.net)
    assert len(where[1]) > 60
    fresh_b = flow_of(predict.Predictor(B, BATCH, H, W, full=full))
    assert p.load_weights({k: torch.from_numpy(v).cuda() for k, v in B.items()}) is p       # device tensors, read where they are
    flow_b = flow_of(p)
    assert np.array_equal(flow_b.view(np.uint32), fresh_b.view(np.uint32))
    assert not np.array_equal(flow_b, flow_a)
    assert _addresses(p.net) == where
    # refusals come before any write
    short = dict(B)
    gone = sorted(short)[5]
    del short[gone]
    with pytest.raises(KeyError, match=r"missing keys \['"):
        p.load_weights(short)
    with pytest.raises(KeyError, match=r"unknown keys \['"):
        p.load_weights(dict(A, **{"no_such_layer.weight": np.zeros(3, np.float32)}))
    bad = dict(A)
    last = sorted(bad)[-1]
    bad[last] = np.zeros(tuple(bad[last].shape) + (2,), np.float32)
    with pytest.raises(ValueError, match="shape"):
        p.load_weights(bad)
    assert np.array_equal(flow_of(p).view(np.uint32), flow_b.view(np.uint32))
    p.load_weights(list(A.items()))                                                          # (name, array) pairs, host arrays
    assert np.array_equal(flow_of(p).view(np.uint32), flow_a.view(np.uint32))
    assert _addresses(p.net) == where


# ---- the training loop's validate() ---------------------------------------------------------------------------------------------------
def _exported(net):
    from maskflownet_amd import training
    return {k: q.detach().cpu().numpy().copy() for k, q in training.reference_named_parameters(net)}


@pytest.mark.parametrize("full", [False, True])
def test_validation_follows_the_net_being_trained(full):
    """At (2,64,128), the shape tests/test_training_step.py trains at: the EPE of Validation.run before and after one optimizer step, each
    against a fresh Predictor built from the parameters the net exports at that moment."""
    import torch
    from maskflownet_amd import data as mdata, network, predict, training
    N, Hs, Ws = 2, 64, 128
    rng = np.random.default_rng(23)
    ds = mdata.DeviceDataset("cuda")
    for k in range(N):
        a = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
        ds.append(a, np.roll(a, (2, -3), (0, 1)), (3.0 * rng.standard_normal((Hs, Ws, 2))).astype(np.float32),
                  rng.choice(np.array([0, 255, 255], np.uint8), (Hs, Ws, 1)))
    params = network.random_params(9, full=full)
    net = (training.MaskFlownetTrainable if full else training.MaskFlownetSTrainable)(params).cuda()
    val = training.Validation({"a": ds}, batch=N, full=full)
    fresh = lambda: predict.Predictor(_exported(net), N, Hs, Ws, full=full).validate_dataset(ds)
    before = val.run(net)
    assert set(before) == {"a"} and before["a"] == fresh()["epe"]
    g = torch.Generator().manual_seed(4)
    im1 = (torch.rand(N, 3, Hs, Ws, generator=g) - 0.5).cuda()
    im2 = torch.roll(im1, shifts=(2, -3), dims=(2, 3))
    label, mask = (torch.randn(N, 2, Hs, Ws, generator=g) * 3.0).cuda(), torch.ones(N, 1, Hs, Ws).cuda()
    opt = torch.optim.Adam([q for q in net.parameters() if q.requires_grad], lr=1e-3)
    training.train_step(net, training.MultiscaleEpe(), opt, im1, im2, label, mask)
    after = val.run(net, kitti=True)                        # no synchronisation of ours between the step and the refresh
    want = fresh()
    print("epe before %.9g, after one step %.9g" % (before["a"], after["a"]["epe"]))
    assert after["a"] == {"epe": want["epe"], "fl": want["fl"]}
    assert after["a"]["epe"] != before["a"]
    assert list(val.predictors) == [(Hs, Ws)]               # one Predictor per sample shape, built once
