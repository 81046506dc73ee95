"""What the fp64 acceptance files (tests/test_backward_fp64.py, tests/test_forward_fp64.py) share: the two sides of the suite (the
emulation on the CPU, the library on the GPU) behind one interface, the record of which kernels a call reached, the oracle's loops
image by image on parallel threads, and sample positions that are exact in fp32."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import parity_cases as pc

_OPS = {"corr": ("correlation", "corr_gram"), "deform": ("deformable_convolution", "dc_mma"), "conv": ("convolution", "conv_mma")}
_THREADS = max(1, min(16, len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))


def per_image(fn, *arrays):
    """fn on each image (the oracle's loops hold no state across images; ctypes calls run in parallel threads)."""
    N = arrays[0].shape[0]
    with ThreadPoolExecutor(_THREADS) as ex:
        return list(ex.map(lambda n: fn(*(a[n:n + 1] for a in arrays)), range(N)))


class Launches:
    """Which kernels a call reached: emu_ops.launch_log() on the emulation, the library's profile counters on the GPU."""

    def __init__(self, emu):
        self.emu = emu

    def __enter__(self):
        if self.emu:
            from tests.emu import emu_ops
            emu_ops.launch_log()
        else:
            import torch
            from maskflownet_amd import _lib
            torch.cuda.synchronize()
            _lib.lib().profile_reset()
            _lib.lib().profile_enable(1)
        return self

    def __exit__(self, *exc):
        if self.emu:
            from tests.emu import emu_ops
            self.log = [k for k in emu_ops.launch_log().split(";") if k]
        else:
            import torch
            from maskflownet_amd import _lib
            torch.cuda.synchronize()
            _lib.lib().profile_enable(0)
        return False

    def count(self, name):
        if self.emu:
            return self.log.count(name)
        import ctypes
        from maskflownet_amd import _lib
        c, ms = ctypes.c_int(0), ctypes.c_double(0)
        _lib.lib().profile_query(name.encode(), ctypes.byref(c), ctypes.byref(ms))
        return c.value

    def expect(self, names, absent=(), what=""):
        for nm in names:
            assert self.count(nm) >= 1, "%s: kernel %s did not run%s" % (what, nm, (" (ran: %s)" % self.log) if self.emu else "")
        for nm in absent:
            assert self.count(nm) == 0, "%s: kernel %s ran" % (what, nm)


class Env:
    """One side of the suite: the OpSet, host <-> device moves, the arithmetic switch, the launch check."""

    def __init__(self, emu):
        self.emu = emu
        if emu:
            from tests.emu import emu_ops
            self.ops = emu_ops.emu_ops()
            self.dev = self.host = lambda a: a
        else:
            import torch
            assert torch.cuda.is_available(), "these tests need the MI355X"
            from maskflownet_amd import ops as o
            self.ops = o.default_ops()
            self.dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            self.host = lambda t: t.detach().cpu().numpy()

    def set_arith(self, op, mode):
        if self.emu:
            from tests.emu import emu_ops
            emu_ops.set_tuning(**{_OPS[op][1]: mode})
        else:
            from maskflownet_amd import _lib
            _lib.set_arithmetic(**{_OPS[op][0]: mode})

    def set_tuning(self, **kw):
        if self.emu:
            from tests.emu import emu_ops
            emu_ops.set_tuning(**kw)
        else:
            from maskflownet_amd import _lib
            _lib.set_tuning(**kw)

    def launches(self):
        return Launches(self.emu)


def exact_positions(a, step=2.0 ** -11):
    """Offsets (or flows) on a 2^-11 grid below 2^10 pixels: tap + offset, its fraction and the bilinear weights are then exact in
    fp32, so the fp32 oracle's and the kernels' sample positions are the fp64 oracle's, and the fp32 oracle's error (the bar) is
    arithmetic only.  (Offsets rounded in fp32 would put samples on the other side of a lattice line now and then: the derivative
    of the interpolation jumps there, by the order of M.)  Values beyond 2^10 pixels (far outside the image) are left alone."""
    a = np.asarray(a, np.float32)
    return np.where(np.abs(a) < 1024, np.round(a / step) * step, a).astype(np.float32)


def deform_offsets(rng, N, H, W, kind):
    """shared (one (dy, dx) per pixel over the nine taps) 'smooth' / 'rough' / 'far' offsets of parity_cases.shared_offsets;
    'pertap': independent offsets per tap of sigma 1.5 px, some far outside; on the exact_positions grid."""
    if kind != "pertap":
        return exact_positions(pc.shared_offsets(rng, N, H, W, kind))
    off = (rng.standard_normal((N, 18, H, W)) * 1.5).astype(np.float32)
    off[:, :, 0, 0] = np.float32(3.0 * max(H, W))
    return exact_positions(off)
