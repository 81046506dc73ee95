"""The matching module's gate (maskflownet_amd/csrc/kernels/gate.h) stated in numpy, forward and backward, independent of the
kernels: fp64 (acceptance), an fp32 twin of the same formulae (every product and sum rounded to fp32, the two-sigmoid product
included, channels added one after another) and the magnitude bounds M of tests/parity_cases.check_fp64_bound.

    s = 1 / (1 + exp(-mask))          s' = 1 / (1 + exp(+mask))          (s' on its own: 1 - s has no correct bit on a saturated mask)
    out       = act(raw * s + tradeoff)                                   M = |raw| s + |tradeoff|
    gp        = act ? g * (y > 0 ? 1 : 0.1) : g,   g = gout (+ gout2)     the kink is taken from the GIVEN y, as the kernel takes it
    gtradeoff = gp                                                        M = |g|
    graw      = gp * s                                                    M = |g| s
    gmask     = s s' sum_c gp raw                                         M = s s' sum_c |gp raw|
"""
import numpy as np


def _sig(x, dtype):
    one = dtype(1)
    with np.errstate(over="ignore"):
        return (one / (one + np.exp(-x))).astype(dtype), (one / (one + np.exp(x))).astype(dtype)


def forward(raw, mask=None, tradeoff=None, leaky=True, dtype=np.float64, magnitude=False):
    raw = np.asarray(raw, dtype)
    v = np.abs(raw) if magnitude else raw
    if mask is not None:
        v = (v * _sig(np.asarray(mask, dtype), dtype)[0]).astype(dtype)
    if tradeoff is not None:
        t = np.asarray(tradeoff, dtype)
        v = (v + (np.abs(t) if magnitude else t)).astype(dtype)
    if leaky and not magnitude:
        v = np.maximum(v, (dtype(0.1) * v).astype(dtype))
    return v


def backward(gout, y, raw, mask=None, leaky=True, gout2=None, dtype=np.float64, magnitude=False):
    """-> (graw, gmask or None, gtradeoff); magnitude=True: the bounds M of the three."""
    g = np.asarray(gout, dtype)
    if magnitude:
        g = np.abs(g)
    if gout2 is not None:
        g2 = np.asarray(gout2, dtype)
        g = (g + (np.abs(g2) if magnitude else g2)).astype(dtype)
    gp = g
    if leaky and not magnitude:      # M keeps slope 1 everywhere: it bounds either side of the kink
        gp = np.where(np.asarray(y) > 0, g, (g * dtype(0.1)).astype(dtype)).astype(dtype)
    if mask is None:
        return gp, None, gp
    s, sn = _sig(np.asarray(mask, dtype), dtype)
    graw = (gp * s).astype(dtype)
    if raw is None:
        return graw, None, gp
    r = np.asarray(raw, dtype)
    terms = (gp * (np.abs(r) if magnitude else r)).astype(dtype)
    acc = np.zeros(terms[:, :1].shape, dtype)
    for c in range(terms.shape[1]):  # one after another, each sum rounded (fp32 twin)
        acc = (acc + terms[:, c:c + 1]).astype(dtype)
    return graw, ((s * sn).astype(dtype) * acc).astype(dtype), gp
