"""Reference of the fused multiscale training loss (maskflownet_amd/csrc/kernels/loss.h), numpy / torch-CPU.

MaskFlownet.py:563-611 (EpeLossWithMask, MultiscaleEpe with match='upsampling') as pipeline.py:42-44 builds it.  The upsampled
prediction u is `oracle.ref.upsample(p, f)` in fp32 -- the project's bit-exact contract for Upsample, taken as given (the loss's
gradient is steep or discontinuous at u == label, so an ulp of u is not an error of the loss kernels to be bounded but part of
their definition); everything after it runs in `dtype`: fp64 for acceptance, fp32 for the twin whose error sets the bar.  The
adjoint of Upsample is torch autograd over edge pad + conv_transpose2d with the triangle kernel (`upsample_torch`, the statement
tests/test_training_step.py uses).  magnitude=True evaluates the same expressions over absolute values (M of
parity_cases.check_fp64_bound)."""
import numpy as np
import torch

F = torch.nn.functional


def upsample_torch(x, f):
    """MaskFlownet.py:35-62 on a torch tensor, differentiable."""
    if f == 1:
        return x
    N, C, H, W = x.shape
    xi = F.pad(x.reshape(N * C, 1, H, W), (0, 1, 0, 1), mode="replicate")
    wk = 2 * f - 1
    c = wk // 2
    k1 = 1 - (c - torch.arange(wk, dtype=x.dtype)).abs() / (c + 1)
    y = F.conv_transpose2d(xi, (k1[:, None] * k1[None, :])[None, None], stride=f, padding=f - 1)[:, :, :-1, :-1]
    return y.reshape(N, C, H * f, W * f)


def upsample_adjoint(g, f, dtype=np.float64):
    """The adjoint of Upsample(f) applied to g (N,C,H,W) -> (N,C,H/f,W/f), by autograd."""
    g = torch.from_numpy(np.ascontiguousarray(g, dtype))
    N, C, H, W = g.shape
    x = torch.zeros((N, C, H // f, W // f), dtype=g.dtype, requires_grad=True)
    upsample_torch(x, f).backward(g)
    return x.grad.numpy()


def oracle_upsample(p, f):
    from oracle import ref
    ref.build()
    return ref.upsample(np.ascontiguousarray(p, np.float32), int(f))


def _pixel(u, label, eps, q, dtype):
    """(L, dL/ddy, dL/ddx, |dL/ddy|, |dL/ddx|) per pixel, in dtype."""
    d = u.astype(dtype) - label.astype(dtype)
    dy, dx = d[:, 0], d[:, 1]
    eps = dtype(eps)
    if q is None:
        r = np.sqrt((dy * dy + dx * dx) + eps)
        return r, dy / r, dx / r, np.abs(dy) / r, np.abs(dx) / r
    a = (np.abs(dy) + np.abs(dx)) + eps
    t = dtype(q) * np.power(a, dtype(q) - dtype(1))
    return np.power(a, dtype(q)), t * np.sign(dy), t * np.sign(dx), t * np.abs(np.sign(dy)), t * np.abs(np.sign(dx))


def _msum(mask, dtype):
    return mask.astype(dtype).reshape(mask.shape[0], -1).sum(1)     # (N,1,1,1): the value itself (the reference's broadcast)


def loss(preds, label, mask, scales, weights, eps=1e-8, q=None, dtype=np.float64, magnitude=False, up=oracle_upsample):
    """-> (loss (N,), sums (N, S+1)).  magnitude: the sums of |terms| (sums: themselves, every term is >= 0 for mask >= 0)."""
    N = label.shape[0]
    m = mask.astype(dtype)[:, 0]
    if magnitude:
        m = np.abs(m)
    msum = _msum(mask, dtype)
    sums = np.zeros((N, len(preds) + 1), dtype)
    total = np.zeros(N, dtype)
    for s, (p, f, w) in enumerate(zip(preds, scales, weights)):
        L = _pixel(up(p, f), label, eps, q, dtype)[0]
        sums[:, s] = (L * m).reshape(N, -1).sum(1)
        term = dtype(w) * sums[:, s] / msum
        total = total + (np.abs(term) if magnitude else term)
    sums[:, -1] = _msum(np.abs(mask) if magnitude else mask, dtype)
    return total, sums


def grads(gloss, preds, label, mask, scales, weights, eps=1e-8, q=None, dtype=np.float64, magnitude=False, up=oracle_upsample):
    """-> [gp_s (N,2,h,w)]: gloss[n] * w_s / msum[n] * Upsample^T(mask * dL/dd)."""
    N, _, H, W = label.shape
    m = np.broadcast_to(mask.astype(dtype), (N, 1, H, W))
    msum = _msum(mask, dtype)
    out = []
    for p, f, w in zip(preds, scales, weights):
        _, gy, gx, ay, ax = _pixel(up(p, f), label, eps, q, dtype)
        g = np.stack([ay, ax] if magnitude else [gy, gx], 1) * (np.abs(m) if magnitude else m)
        coef = np.asarray(gloss, dtype) * dtype(w) / msum
        if magnitude:
            coef = np.abs(coef)
        out.append((coef[:, None, None, None] * upsample_adjoint(g, f, dtype)).astype(dtype))
    return out


def composed(preds, label, mask, scales, weights, eps=1e-8, q=None):
    """The literal composition in torch (fp64 tensors in, differentiable): EpeLossWithMask per scale times its weight, added."""
    def epe(pred):
        if q is not None:
            e = ((pred - label).abs().sum(1) + eps) ** q
        else:
            e = torch.sqrt(((pred - label) ** 2).sum(1) + eps)
        e = e * mask.squeeze(1)
        return e.flatten(1).sum(1) / mask.flatten(1).sum(1)
    return sum(epe(upsample_torch(p, f)) * w for p, f, w in zip(preds, scales, weights))
