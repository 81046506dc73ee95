"""Reference statements of the trainer's Adam step (maskflownet_amd/csrc/kernels/optimizer.h: MXNet 1.5's `adam_update` operator as
Adam.update calls it), in numpy.  TEST INFRASTRUCTURE ONLY.

    g  = rescale_grad * grad + wd * w
    g  = clip_gradient >= 0 ? min(max(g, -clip), clip) : g
    m' = beta1 * m + (1 - beta1) * g
    v' = beta2 * v + (1 - beta2) * (g * g)
    w' = w - (lr * m') / (sqrt(v') + epsilon)

adam_step(dtype=np.float32): the twin -- every scalar is an fp32 value, 1 - beta is formed in fp32, every product, sum, quotient and
root is one numpy operation on fp32 arrays and therefore rounded once, in the header's order.  adam_step(dtype=np.float64): the same
expression on the same fp32 INPUTS (tensors and scalars, 1 - beta included: the kernel's contract takes them as given), evaluated in
fp64.  adam_magnitude: M, the same expression over absolute values -- every sum of signed terms becomes the sum of their magnitudes;
the quotient's denominator sqrt(v') + epsilon is a sum of non-negative terms and stays what it is (the fp64 value), so that M bounds
|w'| element by element.  lr_t: the learning rate Adam.update hands to the operator."""
import math

import numpy as np


def lr_t(lr, beta1, beta2, t):
    """python/mxnet/optimizer/optimizer.py, Adam.update: coef1 = 1 - beta1**t; coef2 = 1 - beta2**t; lr *= sqrt(coef2) / coef1 -- in
    Python doubles; the operator receives it as a float (rounded once to fp32 here)."""
    coef1 = 1.0 - beta1 ** t
    coef2 = 1.0 - beta2 ** t
    return float(np.float32(lr * math.sqrt(coef2) / coef1))


def _scalars(dtype, lr, beta1, beta2, epsilon, wd, rescale_grad, lr_mult, wd_mult):
    f = np.float32
    lr_, wd_ = f(lr) * f(lr_mult), f(wd) * f(wd_mult)                # one fp32 product each, as the kernel forms them
    omb1, omb2 = f(1.0) - f(beta1), f(1.0) - f(beta2)                # formed in fp32
    return [dtype(x) for x in (lr_, f(beta1), f(beta2), f(epsilon), wd_, f(rescale_grad), omb1, omb2)]


def _clip(g, clip, dtype):
    if clip is None or clip < 0:
        return g
    c = dtype(np.float32(clip))
    return np.minimum(np.maximum(g, -c), c)                          # numpy's minimum / maximum pass a NaN through, as the kernel does


def adam_step(w, grad, m, v, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, wd=0.0, rescale_grad=1.0, clip_gradient=-1.0, lr_mult=1.0,
              wd_mult=1.0, dtype=np.float32):
    """-> (w', m', v') as `dtype` arrays; the inputs are not modified."""
    lr_, b1, b2, eps, wd_, rs, omb1, omb2 = _scalars(dtype, lr, beta1, beta2, epsilon, wd, rescale_grad, lr_mult, wd_mult)
    w, grad, m, v = (np.asarray(a, np.float32).astype(dtype) for a in (w, grad, m, v))
    with np.errstate(all="ignore"):
        g = rs * grad + wd_ * w
        g = _clip(g, clip_gradient, dtype)
        m1 = b1 * m + omb1 * g
        v1 = b2 * v + omb2 * (g * g)
        w1 = w - (lr_ * m1) / (np.sqrt(v1) + eps)
    for a in (w1, m1, v1):
        assert a.dtype == dtype
    return w1, m1, v1


def adam_magnitude(w, grad, m, v, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, wd=0.0, rescale_grad=1.0, clip_gradient=-1.0, lr_mult=1.0,
                   wd_mult=1.0):
    """-> (M_w, M_m, M_v), fp64: adam_step over absolute values; the quotient's denominator is the fp64 statement's own."""
    d = np.float64
    lr_, b1, b2, eps, wd_, rs, omb1, omb2 = _scalars(d, lr, beta1, beta2, epsilon, wd, rescale_grad, lr_mult, wd_mult)
    _, _, v64 = adam_step(w, grad, m, v, lr, beta1, beta2, epsilon, wd, rescale_grad, clip_gradient, lr_mult, wd_mult, dtype=d)
    w, grad, m, v = (np.abs(np.asarray(a, np.float32).astype(d)) for a in (w, grad, m, v))
    with np.errstate(all="ignore"):
        Mg = abs(rs) * grad + abs(wd_) * w
        Mg = _clip(Mg, clip_gradient, d)
        Mm = b1 * m + omb1 * Mg
        Mv = b2 * v + omb2 * (Mg * Mg)
        Mw = w + (abs(lr_) * Mm) / (np.sqrt(v64) + eps)
    return Mw, Mm, Mv


def torch_adam_step(w, grad, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in fp64, for the comparison of the two optimizers' arithmetic:
    the denominator is sqrt(v') / sqrt(1 - beta2^t) + eps and the step lr / (1 - beta1^t)."""
    w, grad, m, v = (np.asarray(a, np.float64) for a in (w, grad, m, v))
    m1 = beta1 * m + (1 - beta1) * grad
    v1 = beta2 * v + (1 - beta2) * grad * grad
    denom = np.sqrt(v1) / math.sqrt(1 - beta2 ** t) + eps
    return w - (lr / (1 - beta1 ** t)) * m1 / denom, m1, v1
