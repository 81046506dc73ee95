"""mfn_matching_level (maskflownet_amd/mxnet_ops.py) trains: forward under mx.autograd.record() and backward through the MXNet stub
of tests/fake_mxnet, against the operator chain of MaskFlownet.py:227-236 stated on the oracle (the chain of
tests/test_mxnet_binding.py::_matching_level, and its backward functions, with tests/gate_ref.py between them).

The stub's tape carries a gradient for each output (autograd.backward(heads, head_grads)), so both heads are seeded -- corr and warp --
and the gate's two-gradient path runs here as well as at the OpSet level; one case seeds corr alone (what the trainable networks do:
warp is used by the cost volume only), where the stub hands zeros over for warp's gradient.  The LeakyReLU kinks of the reference chain
are taken from the operator's own outputs, as its backward takes them.  Tolerances: those tests/test_mxnet_binding.py uses for these
kernels' gradients -- parity_cases.check_close at 2e-5 of each tensor's largest element (test_upsample_and_fused_leaky_correlation_train's
for the cost volume's backward, _deform_fwd_bwd's for req 'add')."""
import numpy as np
import pytest

from tests import gate_ref as gr
from tests import parity_cases as pc
from tests.test_mxnet_binding import _matching_level, cpu_binding, gpu_binding   # noqa: F401  (fixtures)

TOL = 2e-5


def _level(mx, oracle, ctx, N, C, H, W, stride, gated, seed=0, grad_req="write", seed_warp=True, md=4):
    rng = np.random.default_rng(900 + seed)
    c1, c2 = pc.feat(rng, (N, C, H, W)), pc.feat(rng, (N, C, H, W))
    w = pc.msra_weight(rng, C, C)
    b = (rng.standard_normal((C,)) * 0.1).astype(np.float32)
    fl = (pc.flow_field(rng, N, H, W, sigma=2.0) * np.float32(stride / 20.0)).astype(np.float32)
    mask = (rng.standard_normal((N, 1, H, W)) * 2).astype(np.float32) if gated else None
    trade = rng.standard_normal((N, C, H, W)).astype(np.float32) if gated else None
    D = 2 * md + 1
    gcorr = (rng.standard_normal((N, D * D, H, W)) / 8).astype(np.float32)
    gwarp = (rng.standard_normal((N, C, H, W)) / 8).astype(np.float32) if seed_warp else None
    host = [c1, c2, fl, w, b] + ([mask, trade] if gated else [])
    names = ["c1", "c2", "flow", "weight", "bias"] + (["mask", "tradeoff"] if gated else [])
    arrs = [mx.nd.array(a, ctx=ctx) for a in host]
    for a in arrs:
        a.attach_grad(grad_req)
        if grad_req == "add":
            a.grad[:] = mx.nd.array(np.full(a.shape, 0.5, np.float32), ctx=ctx)
    base = np.float32(0.5 if grad_req == "add" else 0.0)
    with mx.autograd.record():
        got_corr, got_warp = mx.nd.Custom(*arrs, op_type="mfn_matching_level", scale=20.0, stride=stride, max_displacement=md,
                                          gated=gated, tradeoff=gated)
    # ---- forward, as _matching_level states it
    off = oracle.offsets_from_flow(fl, 20.0, stride)
    raw = oracle.deformable_convolution(c2, off, w, b, kernel=(3, 3), pad=(1, 1))
    warp = gr.forward(raw, mask, trade, True, dtype=np.float32)
    corr = oracle.correlation(c1, warp, max_displacement=md, pad_size=md)
    corr = np.where(corr > 0, corr, np.float32(0.1) * corr).astype(np.float32)
    yw, yc = got_warp.asnumpy(), got_corr.asnumpy()
    pc.check_close(yw, warp, what="matching level under record(): warped features")
    pc.check_close(yc, corr, what="matching level under record(): cost volume")
    # ---- backward
    heads, grads = [got_corr], [mx.nd.array(gcorr, ctx=ctx)]
    if seed_warp:
        heads.append(got_warp)
        grads.append(mx.nd.array(gwarp, ctx=ctx))
    mx.autograd.backward(heads, grads)
    gpre = np.where(yc > 0, gcorr, np.float32(0.1) * gcorr).astype(np.float32)
    g1, g2 = oracle.correlation_backward(gpre, c1, warp, max_displacement=md, pad_size=md)
    graw, gmask, gtr = gr.backward(g2 if gwarp is None else gwarp, yw, raw, mask, True, None if gwarp is None else g2, dtype=np.float32)
    gx, goff, gw, gb = oracle.deformable_convolution_backward(graw, c2, off, w, with_bias=True, pad=(1, 1))
    gflow = (goff.reshape(N, 9, 2, H, W).sum(1) * np.float32(20.0 / stride)).astype(np.float32)
    want = [g1, gx, gflow, gw, gb] + ([gmask, gtr] if gated else [])
    for a, g, nm in zip(arrs, want, names):
        pc.check_close(a.grad.asnumpy() - base, g, tol=TOL, what="matching level backward, gradient of %s (%s, gated=%s)" % (nm, grad_req, gated))


@pytest.mark.parametrize("gated", [False, True])
def test_matching_level_trains_through_the_stub(cpu_binding, oracle, gated):
    mx, m = cpu_binding
    _level(mx, oracle, mx.cpu(), 1, 32, 6, 8, 8.0, gated)
    _level(mx, oracle, mx.cpu(), 2, 48, 4, 8, 16.0, gated, seed=1, md=2)


def test_matching_level_corr_seeded_alone_and_grad_req_add(cpu_binding, oracle):
    mx, m = cpu_binding
    _level(mx, oracle, mx.cpu(), 1, 32, 6, 8, 8.0, True, seed=2, seed_warp=False)
    _level(mx, oracle, mx.cpu(), 2, 48, 4, 8, 16.0, True, seed=3, grad_req="add", md=2)
    _level(mx, oracle, mx.cpu(), 1, 32, 6, 8, 8.0, False, seed=4, grad_req="add")


def test_inference_outputs_are_unchanged_and_dependencies_declared(cpu_binding, oracle):
    """The registered operator's outputs stay what tests/test_mxnet_binding.py checks; backward asks for out_grad + in_data + out_data."""
    mx, m = cpu_binding
    _matching_level(mx, oracle, mx.cpu(), 1, 32, 6, 8, 8.0, True)
    prop = mx.operator.get_registered("mfn_matching_level")(scale="20.0", stride="8", gated="True", tradeoff="True")
    assert prop.declare_backward_dependency([0, 1], [2, 3, 4, 5, 6, 7, 8], [9, 10]) == list(range(11))


def test_frozen_inputs_get_req_null(cpu_binding, oracle):
    """Only the weight attached: every other req is null, the mask gradient with it -- no recomputed convolution, no gate workspace."""
    mx, m = cpu_binding
    from tests.emu import emu_ops
    rng = np.random.default_rng(5)
    N, C, H, W = 1, 32, 6, 8
    host = [pc.feat(rng, (N, C, H, W)), pc.feat(rng, (N, C, H, W)), (pc.flow_field(rng, N, H, W) * np.float32(0.4)).astype(np.float32),
            pc.msra_weight(rng, C, C), np.zeros(C, np.float32), rng.standard_normal((N, 1, H, W)).astype(np.float32),
            rng.standard_normal((N, C, H, W)).astype(np.float32)]
    arrs = [mx.nd.array(a) for a in host]
    arrs[3].attach_grad()
    with mx.autograd.record():
        corr, warp = mx.nd.Custom(*arrs, op_type="mfn_matching_level", scale=20.0, stride=8.0, max_displacement=4, gated=True, tradeoff=True)
    emu_ops.launch_log()
    corr.backward(mx.nd.array(np.ones(corr.shape, np.float32)))
    log = [k for k in emu_ops.launch_log().split(";") if k]
    assert "matching_gate_bwd_v4" in log and "matching_gate_bwd_join" not in log, log
    assert np.isfinite(arrs[3].grad.asnumpy()).all() and np.abs(arrs[3].grad.asnumpy()).max() > 0


@pytest.mark.gpu
def test_gpu_matching_level_trains(gpu_binding, oracle):
    """One cfg2 level (level 3 of a 384 x 512 input: 64 channels, 48 x 64, stride 8, gated) at batch 2."""
    mx, m = gpu_binding
    _level(mx, oracle, mx.gpu(0), 2, 64, 48, 64, 8.0, True, seed=7)
