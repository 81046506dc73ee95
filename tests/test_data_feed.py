"""maskflownet_amd.data: the resident data set, the sampler's draws and the feeder's batches; io.read_ppm.

CPU: the sampler (its draws are host arithmetic over len() and shape(i) of a data set) and the PPM reader.  GPU: the arena, Feeder.next()
against tests/data_ref.py on the draws it reports, bit for bit, and two training steps fed by it against the same two steps fed by
batches assembled on the host."""
import pickle

import numpy as np
import pytest

from tests import data_ref


class _Shapes:
    """What BatchSampler uses of a data set: len() and shape(i)."""

    def __init__(self, shapes):
        self.shapes = list(shapes)

    def __len__(self):
        return len(self.shapes)

    def shape(self, i):
        return self.shapes[i]


def test_import_needs_no_gpu():
    import maskflownet_amd.data as data
    assert {"DeviceDataset", "BatchSampler", "Feeder"} <= set(dir(data))
    with pytest.raises(RuntimeError, match="no CPU"):
        data.DeviceDataset("cpu")
    with pytest.raises(ValueError, match="flow_dtype"):
        data.DeviceDataset("cuda", flow_dtype="bfloat16")


def test_sampler_epochs_have_every_index_once():
    from maskflownet_amd.data import BatchSampler
    a, b = _Shapes([(8, 8)] * 5), _Shapes([(8, 8)] * 3)
    s = BatchSampler([a, a, b], (8, 8), seed=1)       # two slots share a's index generator, as batch_size // len(iqs) of main.py:484
    drawn = {0: [], 1: []}
    for step in range(15):                             # 30 draws of a = 6 epochs, 15 of b = 5 epochs
        d = s.draw()
        assert len(d) == 3 and all(len(t) == 4 for t in d)
        drawn[0] += [d[0][0], d[1][0]]
        drawn[1].append(d[2][0])
        assert all(t[1] == 0 and t[2] == 0 for t in d)     # space 0: the crop is the sample
    assert np.bincount(drawn[0], minlength=5).tolist() == [6] * 5 and np.bincount(drawn[1], minlength=3).tolist() == [5] * 3
    for k, n in ((0, 5), (1, 3)):                      # every epoch on its own is a permutation
        for e in range(len(drawn[k]) // n):
            assert sorted(drawn[k][e * n:(e + 1) * n]) == list(range(n))
    assert len({tuple(drawn[0][e * 5:(e + 1) * 5]) for e in range(6)}) > 1      # and they are reshuffled


@pytest.mark.parametrize("space", [0, 1, 5])
def test_sampler_crops_stay_in_range_and_reach_both_ends(space):
    from maskflownet_amd.data import BatchSampler
    ds = _Shapes([(10 + space, 7 + space)] * 4)
    s = BatchSampler([ds], (10, 7), seed=2)
    ys, xs, flips = set(), set(), set()
    for _ in range(200):
        (i, y0, x0, flip), = s.draw()
        ys.add(y0), xs.add(x0), flips.add(flip)
    # `space and randint(space)`: 0 .. space - 1, and 0 where there is no space
    want = set(range(space)) if space else {0}
    assert ys == want and xs == want and flips == {0, 1}


def test_sampler_refuses_a_sample_smaller_than_the_crop():
    from maskflownet_amd.data import BatchSampler
    with pytest.raises(ValueError, match="smaller than the crop"):
        BatchSampler([_Shapes([(9, 9)])], (10, 8)).draw()
    with pytest.raises(ValueError, match="empty"):
        BatchSampler([_Shapes([])], (4, 4)).draw()
    with pytest.raises(ValueError, match="at least one slot"):
        BatchSampler([], (4, 4))


def test_sampler_reproduces_from_its_seed_and_its_state():
    from maskflownet_amd.data import BatchSampler
    a, b = _Shapes([(12, 20), (9, 14), (16, 16), (8, 30), (11, 13), (10, 10), (9, 9)]), _Shapes([(20, 20)] * 3)
    run = lambda s, n: [s.draw() for _ in range(n)]
    one, two, other = (BatchSampler([a, b, a], (8, 9), seed=k) for k in (7, 7, 8))
    first = run(one, 11)
    assert first == run(two, 11) and first != run(other, 11)
    state = pickle.loads(pickle.dumps(one.state()))     # mid-epoch of both data sets: 22 draws of 7, 11 of 3
    rest = run(one, 9)
    fresh = BatchSampler([a, b, a], (8, 9), seed=123)
    fresh.set_state(state)
    assert run(fresh, 9) == rest
    with pytest.raises(ValueError, match="data sets"):
        BatchSampler([a], (8, 9)).set_state(state)


def _ppm(path, w, h, rgb, header=None):
    with open(path, "wb") as f:
        f.write(header if header is not None else b"P6 %d %d 255\n" % (w, h))
        f.write(rgb.tobytes())


def test_read_ppm(tmp_path):
    from maskflownet_amd import io
    rng = np.random.default_rng(0)
    for w, h in ((512, 384), (5, 3)):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        _ppm(tmp_path / "a.ppm", w, h, rgb)
        got = io.read_ppm(str(tmp_path / "a.ppm"))
        assert got.dtype == np.uint8 and got.shape == (h, w, 3) and (got == rgb).all() and got.flags["WRITEABLE"]
    _ppm(tmp_path / "c.ppm", 5, 3, rgb, b"P6\n# a comment\n5 3\n255\n")
    assert (io.read_ppm(str(tmp_path / "c.ppm")) == rgb).all()
    rgb[0, 0, 0] = 10                                   # a payload that begins with a white-space byte stays a payload
    _ppm(tmp_path / "d.ppm", 5, 3, rgb)
    assert (io.read_ppm(str(tmp_path / "d.ppm")) == rgb).all()
    for name, header, payload, err in (("magic", b"P5 5 3 255\n", rgb, "magic"), ("maxval", b"P6 5 3 65535\n", rgb, "maxval"),
                                       ("short", b"P6 5 3 255\n", rgb[:2], "truncated"), ("header", b"P6 5", rgb[:0], "truncated"),
                                       ("fields", b"P6 five 3 255\n", rgb, "header fields")):
        _ppm(tmp_path / (name + ".ppm"), 5, 3, payload, header)
        with pytest.raises(ValueError, match=err):
            io.read_ppm(str(tmp_path / (name + ".ppm")))


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------
def _samples(rng, shapes, flow_dtype, mask):
    out = []
    for H, W in shapes:
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = 127 + 60 * np.sin(xx / 9.0)[..., None] + 50 * np.cos(yy / 7.0)[..., None] + rng.uniform(-15, 15, (H, W, 3))
        img1 = np.clip(base, 0, 255).astype(np.uint8)
        img2 = np.clip(np.roll(base, 2, axis=1) + rng.uniform(-3, 3, (H, W, 3)), 0, 255).astype(np.uint8)
        flow = (np.stack([np.full((H, W), 2.0), np.zeros((H, W))], axis=-1) + rng.standard_normal((H, W, 2)) * 0.25).astype(flow_dtype)
        out.append((img1, img2, flow, (rng.uniform(size=(H, W, 1)) > 0.1).astype(np.uint8) * 255 if mask else None))
    return out


@pytest.mark.gpu
def test_gpu_device_dataset_round_trip_across_chunks():
    import torch
    from maskflownet_amd.data import DeviceDataset
    rng = np.random.default_rng(1)
    shapes = [(40, 61), (33, 50), (40, 61), (17, 23), (33, 50), (40, 61), (17, 23)]
    host = _samples(rng, shapes, np.float32, True)
    ds = DeviceDataset("cuda", flow_dtype="float16", chunk_bytes=64 << 10)
    early = []
    addresses = lambda i: tuple(v.data_ptr() for v in ds.sample(i))
    for k, s in enumerate(host):
        assert ds.append(*s) == k
        early.append(addresses(k))
    assert len(ds) == 7 and ds.has_mask is True and [ds.shape(i) for i in range(7)] == shapes
    assert len(ds._chunks) > 1, "64 KiB chunks roll over within seven samples"
    assert ds.nbytes == sum(sum((a.nbytes // (2 if a.dtype == np.float32 else 1) + 15) & ~15 for a in s) for s in host)
    spans = [(c.data_ptr(), c.data_ptr() + c.numel()) for c in ds._chunks]
    for i, s in enumerate(host):
        assert addresses(i) == early[i]                               # nothing moved while the arena grew
        assert all(a % 16 == 0 for a in addresses(i))
        lo, hi = min(addresses(i)), max(a + ((v.numel() * v.element_size() + 15) & ~15) for a, v in zip(addresses(i), ds.sample(i)))
        assert sum(1 for b, e in spans if b <= lo and hi <= e) == 1     # a sample lies inside one chunk, padding included
        got = ds.host(i)
        assert got[2].dtype == np.float16
        for g, w in zip(got, (s[0], s[1], s[2].astype(np.float16), s[3])):
            assert g.shape == w.shape and (g.reshape(-1).view(np.uint8) == np.ascontiguousarray(w).reshape(-1).view(np.uint8)).all()
    with pytest.raises(ValueError, match="has masks"):
        ds.append(*host[0][:3])
    with pytest.raises(ValueError, match="does not fit a chunk"):
        ds.append(*_samples(rng, [(200, 200)], np.float32, True)[0])
    assert len(ds) == 7
    torch.cuda.synchronize()


def _two_datasets(seed=2):
    from maskflownet_amd.data import DeviceDataset
    rng = np.random.default_rng(seed)
    host_a = _samples(rng, [(80, 96), (64, 64), (70, 101)], np.float32, True)
    host_b = _samples(rng, [(64, 77), (91, 64)], np.float32, False)
    a, b = DeviceDataset("cuda", flow_dtype="float16"), DeviceDataset("cuda")
    a.extend(host_a)
    b.extend(host_b)
    host_a = [(s[0], s[1], s[2].astype(np.float16), s[3]) for s in host_a]   # what the data set holds
    return (a, host_a), (b, host_b)


def _reference_batch(hosts, draw, crop, with_mask):
    return data_ref.gather_batch([h[d[0]] for h, d in zip(hosts, draw)], crop, [d[1:] for d in draw], with_mask)


@pytest.mark.gpu
def test_gpu_feeder_batches_are_the_reference_batches():
    from maskflownet_amd.data import BatchSampler, Feeder
    (a, host_a), (b, host_b) = _two_datasets()
    feed = Feeder(BatchSampler([a, b, a], (64, 64), seed=4))
    seen = []
    for step, batch in zip(range(5), feed):
        draw = feed.last_draw
        seen.append(draw)
        want = _reference_batch((host_a, host_b, host_a), draw, (64, 64), True)
        for name, g, w in zip(("img1", "img2", "label", "mask"), batch, want):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert (g.reshape(-1).view(np.uint8) == w.reshape(-1).view(np.uint8)).all(), "step %d: %s" % (step, name)
        assert (batch[3][1] == 255).all()                                 # the slot whose data set has no mask is all valid
    assert len({tuple(d) for d in seen}) == 5 and {t[3] for d in seen for t in d} == {0, 1}
    only_b = Feeder(BatchSampler([b, b], (64, 64), seed=4))
    img1, img2, label, mask = only_b.next()
    assert mask is None and img1.shape == (2, 3, 64, 64) and label.dtype.is_floating_point      # main.py:526-531: no data set has a mask
    want = _reference_batch((host_b, host_b), only_b.last_draw, (64, 64), False)
    assert (label.cpu().numpy().view(np.uint32) == want[2].view(np.uint32)).all()


def _train_two_steps(fed_by_feeder, pinned=None):
    """Two train_batch steps at 64 x 64, batch 2, with a Trainer, fed by a Feeder or by batches assembled on the host from the same
    draws.  pinned: the gradients another run's two updates consumed; this run's updates then consume those instead of its own (see the
    test below)."""
    import torch
    from maskflownet_amd import augment, network, training
    from maskflownet_amd.data import BatchSampler, Feeder
    (a, host_a), (b, host_b) = _two_datasets(seed=3)
    sampler = BatchSampler([a, b], (64, 64), seed=6)
    feed = Feeder(sampler)
    net = training.MaskFlownetSTrainable(network.random_params(0)).cuda()
    loss_fn = training.MultiscaleEpe()
    trainer = training.Trainer(training.reference_named_parameters(net), "adam", {"learning_rate": 1e-4})
    geo, col = augment.presets("chairs", 2, (64, 64), (64, 64), seed=3)
    fed, out, params, states, grads, own = [], [], [], [], [], []
    inner = trainer.step

    def step(batch_size):       # entered after backward: the gradients the update is about to read
        own.append([p.grad.detach().clone() for p in trainer.params])
        if pinned is not None:
            for p, g in zip(trainer.params, pinned[len(grads)]):
                p.grad.copy_(g)
        grads.append([p.grad.detach().clone() for p in trainer.params])
        return inner(batch_size)
    trainer.step = step
    hook = net.register_forward_pre_hook(lambda mod, args: fed.append(torch.cat(args, 0).cpu().numpy()))
    for _ in range(2):
        if fed_by_feeder:
            batch = feed.next()
            draw = feed.last_draw
        else:
            draw = sampler.draw()
            batch = tuple(torch.from_numpy(t).cuda() for t in _reference_batch((host_a, host_b), draw, (64, 64), True))
        states.append(pickle.dumps(sampler.state()))
        loss, epe = training.train_batch(net, loss_fn, trainer, *batch, geo, col)
        out.append((draw, [t.cpu().numpy() for t in batch], fed[-1], loss.cpu().numpy(), epe.cpu().numpy()))
        params.append([p.detach().clone() for p in trainer.params] + [trainer.mean[k].clone() for k in trainer.names] + [trainer.var[k].clone() for k in trainer.names])
    hook.remove()
    return out, params, states, grads, own


@pytest.mark.gpu
def test_gpu_training_fed_by_the_feeder_is_training_fed_from_the_host():
    """Two steps fed by a Feeder against the same two steps fed by tensors assembled with data_ref from the same draws and uploaded,
    the augmenters seeded alike: the draws, the four tensors of each batch, what the network is fed, loss and EPE agree bit for bit in
    both steps, and so do all parameters and the trainer's mean and var after each step.

    One quantity between the batch and the parameters does not reproduce on this library, whoever feeds it: the backward pass sums
    some weight gradients through fp32 atomics (include/mfn_hip.h "up to summation order"; tests/test_augment_pipeline.py meets the
    same thing and continues its second run from the first one's parameters).  Measured on the MI355X with each run consuming its
    own gradients and everything before them bit-identical: 19 of 142 parameter tensors differed in their last bits after step 1
    and 100 after step 2.  So the feeder-fed run's two updates consume the gradients the host-fed run's updates consumed (its own
    are recorded first and must agree with them to what a reordered fp32 sum can differ by: a weight gradient here sums at most
    2 * 64 * 64 = 8192 terms, and 8192 * 2^-24 = 4.9e-4 of the largest term bounds any two orders of summation, so 1e-3 of each
    tensor's largest gradient is asserted); with that one input pinned, parameter and state bits must be equal, with no replay of
    parameters in between."""
    from maskflownet_amd.data import BatchSampler, Feeder
    ref, ref_params, _, ref_grads, _ = _train_two_steps(False)
    got, got_params, states, _, own = _train_two_steps(True, pinned=ref_grads)
    for step, (r, g) in enumerate(zip(ref, got)):
        assert r[0] == g[0], "step %d: the draws" % step
        for k, name in enumerate(("img1", "img2", "label", "mask")):
            assert (r[1][k].reshape(-1).view(np.uint8) == g[1][k].reshape(-1).view(np.uint8)).all(), "step %d: %s" % (step, name)
        assert (r[2].view(np.uint32) == g[2].view(np.uint32)).all(), "step %d: what the network was fed" % step
        assert (r[3].view(np.uint32) == g[3].view(np.uint32)).all(), "step %d: loss %s against %s" % (step, g[3], r[3])
        assert (r[4].view(np.uint32) == g[4].view(np.uint32)).all(), "step %d: EPE %s against %s" % (step, g[4], r[4])
        assert np.isfinite(g[3]).all() and np.isfinite(g[4]).all()
    assert ref[0][0] != ref[1][0]
    for step in range(2):
        worst = max(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() for a, b in zip(own[step], ref_grads[step]))
        differ = sum(int(not (a == b).all()) for a, b in zip(own[step], ref_grads[step]))
        print("step %d: %d of %d gradient tensors differ between the runs in their bits, at most %.2e of a tensor's largest gradient"
              % (step + 1, differ, len(own[step]), worst))
        assert worst <= 1e-3, worst
        differ = sum(int(not (p == q).all()) for p, q in zip(ref_params[step], got_params[step]))
        assert differ == 0, "step %d: %d of %d parameter / mean / var tensors differ" % (step + 1, differ, len(ref_params[step]))
    assert any(bool((p != q).any()) for p, q in zip(ref_params[0], ref_params[1]))          # the steps do move the parameters
    # the sampler's state after step 1, restored into a fresh sampler, reproduces step 2's batch
    (a, host_a), (b, host_b) = _two_datasets(seed=3)
    fresh = BatchSampler([a, b], (64, 64), seed=99)
    fresh.set_state(pickle.loads(states[0]))
    feed = Feeder(fresh)
    batch = feed.next()
    assert feed.last_draw == got[1][0]
    for k in range(4):
        assert (batch[k].cpu().numpy().reshape(-1).view(np.uint8) == got[1][1][k].reshape(-1).view(np.uint8)).all()
