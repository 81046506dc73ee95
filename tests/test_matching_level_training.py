"""training.LibraryBackend(fused_matching=True): both trainable networks with a pyramid level's matching step as one autograd function
on the library (layer.matching_level: mfn_deform_conv_shared_fwd/_bwd, mfn_matching_gate_fwd/_bwd, mfn_correlation_fwd_act/_bwd,
mfn_leaky_relu_bwd).  The two gradient tests of tests/test_training_step.py with the flag set: the same sizes (1 x 128 x 128), the same
reference (its TorchBackend: every layer in differentiable torch, fp64 on the CPU), the same GRAD_TOL and the same 1e-4 loss bar.  A
training step with the flag launches the gate's kernels 4 (MaskFlownet-S) / 5 (the cascade) times per direction, no torch leaky_relu
and no torch sigmoid in a matching step, forward or backward; a backend without matching_level takes the composed path, as before.

What is left of torch's sigmoid in a step is counted exactly: the occlusion masks the networks hand out, which no matching step
contains -- sigmoid(mask2) of MaskFlownet_S (MaskFlownet.py:303-305: one launch, its gradient never asked for) and, in the full model,
the head's and the cascade's input plane sigmoid(Upsample(4)(mask2)) - 0.5 (:309: two launches, under no_grad).  Running those through
the gate's kernel instead would make "no torch sigmoid at all" true and the gate's launch count 5 / 7 instead of 4 / 5: the two
figures cannot both hold for a graph that has these outputs, and the count per level is the one kept."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.fp64_env import Launches                                               # noqa: E402
from tests.test_training_step import GRAD_TOL, TorchBackend, _batch               # noqa: E402

N, H, W = 1, 128, 128


def _params(seed, bias_seed, full=False):
    from maskflownet_amd import network
    params = network.random_params(seed, full=full)
    rng = np.random.default_rng(bias_seed)
    for k in params:                      # biases off zero, so that no LeakyReLU sits on its kink
        if k.endswith(".bias"):
            params[k] = (rng.standard_normal(params[k].shape) * 0.05).astype(np.float32)
    return params


def _compare(lib_net, loss, ref_net, rl, what):
    assert abs(loss.item() - rl.item()) <= 1e-4 * abs(rl.item())
    errs = []
    for k, p in lib_net.P.items():
        g, r = p.grad.detach().cpu().double(), ref_net.P[k].grad
        assert g.shape == r.shape and torch.isfinite(g).all(), k
        errs.append(((g - r).abs().max().item() / max(r.abs().max().item(), 1e-12), k))
    errs.sort(reverse=True)
    print("%s, relative gradient errors, worst first:" % what, ["%s %.1e" % (k, e) for e, k in errs[:8]], "median %.1e" % errs[len(errs) // 2][0])
    assert errs[0][0] <= GRAD_TOL, errs[:5]


def _torch_ops(prof):
    """aten operators of a profiled region that are a sigmoid or a leaky_relu, forward or backward, on any thread."""
    return {e.key: e.count for e in prof.key_averages() if "sigmoid" in e.key or "leaky_relu" in e.key}


def _profiled_step(net, batch):
    """One train_step under the library's launch record and torch's operator profiler -> (gate launches forward, backward, torch ops)."""
    from torch.profiler import ProfilerActivity, profile
    from maskflownet_amd import training
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    im1, im2, label, mask = (t.cuda() for t in batch)
    with Launches(False) as L, profile(activities=[ProfilerActivity.CPU]) as prof:
        loss = training.train_step(net, training.MultiscaleEpe(), opt, im1, im2, label, mask)
        torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    return L.count("matching_gate_fwd"), L.count("matching_gate_bwd_v"), _torch_ops(prof)


def test_parameter_gradients_match_a_torch_statement_of_the_graph():
    from maskflownet_amd import training
    params = _params(7, 3)
    im1, im2, label, mask = _batch(N, H, W, 2)
    lib_net = training.MaskFlownetSTrainable(params, backend=training.LibraryBackend(fused_matching=True)).cuda()
    preds, _ = lib_net(im1.cuda(), im2.cuda())
    loss = training.MultiscaleEpe()(label.cuda(), mask.cuda(), *preds).sum()
    loss.backward()
    tb = TorchBackend()
    ref_net = training.MaskFlownetSTrainable(params, backend=tb, dtype=torch.float64)
    rpreds, _ = ref_net(im1.double(), im2.double())
    rl = training.MultiscaleEpe(backend=tb)(label.double(), mask.double(), *rpreds).sum()
    rl.backward()
    _compare(lib_net, loss, ref_net, rl, "MaskFlownet-S, fused matching")


def test_full_model_cascade_forward_and_gradients():
    from maskflownet_amd import network, training
    params = _params(11, 5, full=True)
    im1, im2, label, mask = _batch(N, H, W, 6)
    ref = network.MaskFlownet(params, N, H, W)(im1, im2)
    lib_net = training.MaskFlownetTrainable(params, backend=training.LibraryBackend(fused_matching=True)).cuda()
    preds, _ = lib_net(im1.cuda(), im2.cuda())
    for a, b in zip(preds, ref["predictions"]):
        assert (a.detach() - b).abs().max().item() <= 2e-5 * max(b.abs().max().item(), 1e-3)
    loss = training.MultiscaleEpe()(label.cuda(), mask.cuda(), *preds).sum()
    loss.backward()
    assert all(q.grad is None for q in lib_net.head.parameters())
    tb = TorchBackend()
    ref_net = training.MaskFlownetTrainable(params, backend=tb, dtype=torch.float64)
    rpreds, _ = ref_net(im1.double(), im2.double())
    rl = training.MultiscaleEpe(backend=tb)(label.double(), mask.double(), *rpreds).sum()
    rl.backward()
    _compare(lib_net, loss, ref_net, rl, "full model, fused matching")


def test_a_step_with_the_flag_runs_the_gate_kernels_and_no_torch_sigmoid_or_leaky_relu_in_a_matching_step():
    from maskflownet_amd import network, training
    B = training.LibraryBackend(fused_matching=True)
    net = training.MaskFlownetSTrainable(network.random_params(9), backend=B).cuda()
    fwd, bwd, torch_ops = _profiled_step(net, _batch(N, H, W, 4))
    assert (fwd, bwd) == (4, 4), (fwd, bwd)
    assert torch_ops == {"aten::sigmoid": 1}, torch_ops      # the occlusion output alone; no leaky_relu, nothing backward
    full = training.MaskFlownetTrainable(network.random_params(9, full=True), backend=training.LibraryBackend(fused_matching=True)).cuda()
    fwd, bwd, torch_ops = _profiled_step(full, _batch(N, H, W, 4))
    assert (fwd, bwd) == (5, 5), (fwd, bwd)       # the cascade's five levels; the frozen head runs the inference form (no gate launch)
    assert torch_ops == {"aten::sigmoid": 2}, torch_ops      # the head's occlusion output and the cascade's input plane, both without a tape


def test_a_backend_without_matching_level_takes_the_composed_path():
    from maskflownet_amd import network, training
    B = training.LibraryBackend()
    assert not B.fused_matching and not hasattr(B, "matching_level")
    assert hasattr(training.LibraryBackend(fused_matching=True), "matching_level")
    net = training.MaskFlownetSTrainable(network.random_params(9)).cuda()
    assert not hasattr(net.B, "matching_level")
    fwd, bwd, torch_ops = _profiled_step(net, _batch(N, 64, 64, 4))
    assert (fwd, bwd) == (0, 0)
    assert torch_ops.get("aten::sigmoid", 0) >= 5 and torch_ops.get("aten::leaky_relu", 0) >= 4, torch_ops     # today's composition
