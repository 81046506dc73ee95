"""training.train_batch (pipeline.py:89-115): /255, geometry, colour, centralize, one training step -- on the MI355X.

The batch the network is fed is checked against tests/augment_ref.py plus a numpy centralize; the bars are those of
tests/test_augment_ops.py.  The colour stage is compared on the geometry stage's own output (the chain through both stages is
ill-conditioned where the colour arithmetic clips), the centralize on the colour stage's."""
import numpy as np
import pytest

from tests import augment_ref as ar
from tests import parity_cases as pc
from tests import predict_ref

U = 2.0 ** -24
N, H, W = 2, 64, 128


def _inputs(seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 127 + 60 * np.sin(xx / 9.0)[None, None] + 50 * np.cos(yy / 7.0)[None, None] + rng.uniform(-15, 15, (N, 3, H, W))
    im1 = np.clip(base, 0, 255).astype(np.uint8)
    im2 = np.clip(np.roll(base, 2, axis=3) + rng.uniform(-3, 3, (N, 3, H, W)), 0, 255).astype(np.uint8)
    label = np.concatenate([np.full((N, 1, H, W), 2.0), np.zeros((N, 1, H, W))], axis=1).astype(np.float32)     # (u, v): 2 px to the right
    return im1, im2, label


def test_train_batch_signature():
    import inspect
    from maskflownet_amd import training
    assert list(inspect.signature(training.train_batch).parameters) == ["net", "loss_fn", "opt", "img1", "img2", "label", "mask", "geo_aug",
                                                                        "color_aug", "buckets", "global_batch"]


def _run(steps=2, seed=3, replay=None):
    """replay: the parameters another run had after each of its steps; this run continues every step but the first from them."""
    import torch
    from maskflownet_amd import augment, network, training
    im1, im2, label = (torch.from_numpy(a).cuda() for a in _inputs())
    net = training.MaskFlownetSTrainable(network.random_params(0)).cuda()
    loss_fn, opt = training.MultiscaleEpe(), torch.optim.Adam(net.parameters(), lr=1e-4)
    geo, col = augment.presets("chairs", N, (H, W), (H, W), seed=seed)
    before = [p.detach().clone() for p in net.parameters()]
    out, fed, after = [], [], []
    hook = net.register_forward_pre_hook(lambda mod, args: fed.append(torch.cat(args, 0).cpu().numpy()))     # what the network is fed
    for step in range(steps):
        if replay is not None and step > 0:
            with torch.no_grad():
                for p, q in zip(net.parameters(), replay[step - 1]):
                    p.copy_(q)
        loss, epe = training.train_batch(net, loss_fn, opt, im1, im2, label, None, geo, col)
        out.append((loss.cpu().numpy(), epe.cpu().numpy(), geo.last_table.copy(), col.last_table.copy(), col.last_sigma, col.last_offset, fed[-1]))
        after.append([p.detach().clone() for p in net.parameters()])
    hook.remove()
    moved = sum(int((a != p.detach()).any()) for a, p in zip(before, net.parameters()))
    return out, moved, after


@pytest.mark.gpu
def test_gpu_train_batch_runs_two_steps_and_reproduces():
    """Two steps, twice from the same seeds.  Everything train_batch adds (the drawn tables, the noise offset, the batch the network
    is fed) and the forward pass (loss, EPE) reproduce bit for bit in both steps.  The one thing that does not is older than
    train_batch: the backward pass sums its weight gradients through fp32 atomics ("up to summation order", include/mfn_hip.h; their
    bits change from call to call, tests/test_memory_contract.py), so two runs hold parameters that differ in the last bits after
    step 1 (measured: the second step's EPE 11.847165 against 11.847166).  The second run therefore continues its second step from
    the first run's parameters after step 1: on equal parameters the second step is asserted bit for bit as well."""
    out, moved, after = _run()
    for loss, epe, *_ in out:
        assert loss.shape == (N,) and epe.shape == (N,) and np.isfinite(loss).all() and np.isfinite(epe).all()
    assert moved > 100                                                     # the parameters change
    assert not np.array_equal(out[0][2], out[1][2]) and not np.array_equal(out[0][3], out[1][3]) and out[1][5] == out[0][5] + 1
    assert (out[0][6] != out[1][6]).mean() > 0.5                            # the second step's augmented images differ from the first's
    out2, _, _ = _run(replay=after)
    for step, (a, b) in enumerate(zip(out, out2)):
        for k in (0, 1, 2, 3, 6):                                          # loss, EPE, both tables, the batch the network was fed
            np.testing.assert_array_equal(a[k], b[k], err_msg="step %d, item %d" % (step, k))
        assert a[4:6] == b[4:6]                                            # sigma and the noise offset


@pytest.mark.gpu
def test_gpu_augmented_batch_is_the_references():
    import torch
    from maskflownet_amd import augment, ops, training
    im1, im2, label = _inputs()
    d1, d2, dl = (torch.from_numpy(a).cuda() for a in (im1, im2, label))
    batches = []
    for step in range(2):
        geo, col = augment.presets("chairs", N, (H, W), (H, W), seed=3)
        for _ in range(step + 1):                                          # the second round replays step 1, then looks at step 2
            x, lab, msk = training.augment_batch(d1, d2, dl, None, geo, col)
        batches.append(x.cpu().numpy())
        f1, f2 = (a.astype(np.float32) / np.float32(255) for a in (im1, im2))
        mask = np.ones((N, 1, 1, 1), np.float32)
        args = (f1, f2, label, mask, geo.last_table, (H, W))
        want, ref32, M = (ar.geometry(*args, label_order=1, **kw) for kw in ({}, {"dtype": np.float32}, {"magnitude": True}))
        g = [t.cpu().numpy() for t in ops.augment_geometry(*(torch.from_numpy(a).cuda() for a in args[:5]), (H, W), label_order=1)]
        for name, k, got in (("label", 2, lab.cpu().numpy()), ("mask", 3, msk.cpu().numpy())):
            np.testing.assert_array_equal(got, g[k])
            pc.check_fp64_bound(got, want[k], ref32[k], M[k], "step %d %s" % (step, name))
        for k in (0, 1):
            pc.check_fp64_bound(g[k], want[k], ref32[k], M[k], "step %d image %d after the geometry" % (step, k + 1))
        cargs = (g[0], g[1], col.last_table, col.last_sigma, col.seed, col.last_offset)
        both = ops.augment_color(torch.from_numpy(g[0]).cuda(), torch.from_numpy(g[1]).cuda(), torch.from_numpy(col.last_table).cuda(),
                                 col.last_sigma, col.seed, col.last_offset).cpu().numpy()
        pc.check_fp64_bound(both, ar.color(*cargs), ar.color(*cargs, dtype=np.float32), ar.color(*cargs, magnitude=True), "step %d colour" % step)
        cen, mean = ar.centralize(both)
        _, mean_bound = predict_ref.pair_mean(both[:N], both[N:])              # 64 * 2^-24 * sum|x| / n
        bound = np.concatenate([mean_bound, mean_bound])[:, :, None, None] + 2 * U * (np.abs(both) + np.abs(np.concatenate([mean, mean]))[:, :, None, None])
        assert (np.abs(x.cpu().numpy() - cen) <= bound).all(), "step %d: centralize" % step     # the mean's bound + the subtraction's rounding
    assert (batches[0] != batches[1]).mean() > 0.5                          # the second step's images differ from the first's
