"""Guard bands around every buffer a call touches, and workspaces of exactly the queried size (tests/test_memory_contract.py).

The fp64 acceptance files pin WHAT a kernel computes; this helper makes visible WHERE it reads and writes, without provoking a fault:
every buffer is a view in the middle of a larger allocation that the test owns, so a stray access lands in memory that is mapped and
watched.  It wraps either side of fp64_env.Env (the emulation's NumpyAdapter, the product's TorchAdapter).

    genv = guarded_env(env)                      # env.ops with a GuardedAdapter and per-call exact workspaces
    results, launches = run_guarded(genv, call)  # call(genv) -> array or tuple; bands verified after the (synchronised) call

GuardedAdapter: BAND floats on each side of every buffer it prepares or hands out, views 64-byte aligned as the plain buffers are (so
dispatch does not change).
  inputs (prepare)                  bands of quiet NaN: a read that leaves the tensor and reaches a result poisons it
  outputs, gradients (empty)        bands of BAND_BITS (no NaN, compared as uint32), interior NaN: an unwritten element shows
  packed weights, workspaces        bands of BAND_BITS, interior of a "stale" NaN bit pattern that differs from the input bands' and
  (empty_bytes)                     from call to call: a result that depends on what the workspace held before shows as NaN
GuardedOpSet overrides OpSet._workspace only: a fresh allocation of exactly `nbytes` per call (no 1 MB floor, no reuse, no rounding: the
64-byte aligned view covers every alignment the header asks for), and `nbytes` itself is the size the library is told.

Reach.  The bands see every WRITE up to BAND floats (16 KiB) before or after a buffer, bit for bit.  Of READS they see only those whose
value reaches a result (NaN).  A write further away, and a read whose value is discarded (masked out, multiplied by an exact zero weight
is still seen: NaN * 0 = NaN; selected away is not), are outside this harness: they are the job of the sanitized stand-alone run of the
emulation (tools/emu_bounds), where every buffer is a heap block of its exact size."""
import numpy as np

from maskflownet_amd.ops import OpSet

BAND = 4096                    # floats on each side: a multiple of 16, so an aligned allocation gives an aligned view
BAND_BITS = 0x4B1D4B1D         # outputs', workspaces' and packed buffers' bands (1.03e7 as a float: no NaN)
INPUT_BAND_BITS = 0x7FC00000   # inputs' bands: the quiet NaN
STALE_BITS = 0x7FE10000        # | call counter: the interior of a fresh workspace / packed buffer (a quiet NaN with a payload)
NAN_BITS = 0x7FC00000          # interior of an output


class _NumpyMem:
    def alloc(self, like, n):
        raw = np.empty(n + 16, np.float32)
        return raw[(-raw.ctypes.data % 64) // 4:][:n]

    def fill(self, flat, bits):
        flat.view(np.uint32)[...] = np.uint32(bits)

    def bits(self, flat):
        return flat.view(np.uint32)

    def store(self, flat, a):
        flat[...] = np.asarray(a, np.float32).reshape(-1)

    def ptr(self, flat):
        return flat.ctypes.data


class _TorchMem:
    def __init__(self, torch):
        self.torch = torch

    def alloc(self, like, n):
        return self.torch.empty(n, dtype=self.torch.float32, device=like.device)

    def fill(self, flat, bits):
        flat.view(self.torch.int32).fill_(int(bits))     # every pattern here is below 2^31

    def bits(self, flat):
        return flat.view(self.torch.int32).cpu().numpy().view(np.uint32)

    def store(self, flat, a):
        flat.copy_(a.reshape(-1))

    def ptr(self, flat):
        return flat.data_ptr()


class _Rec:
    def __init__(self, name, flat, n, band_bits):
        self.name, self.flat, self.n, self.band_bits = name, flat, n, band_bits


class GuardedAdapter:
    """Delegates to `inner` (NumpyAdapter or TorchAdapter); see the module docstring."""

    def __init__(self, inner):
        self.inner = inner
        self.mem = _TorchMem(inner.torch) if hasattr(inner, "torch") else _NumpyMem()
        self.records = []
        self._mine = {}          # data pointer of a view -> its record
        self._exact = {}         # data pointer of an empty_bytes view -> the byte count asked for
        self.calls = 0           # empty_bytes calls so far: the stale pattern's payload
        self.last_stale = None

    def __getattr__(self, name):     # ptr, shape, ndim, elem_strides, require_destination, prepare_strided, device_key, stream
        return getattr(self.inner, name)

    def _banded(self, like, shape, name, band_bits, interior_bits=None):
        n = 1
        for d in shape:
            n *= int(d)
        flat = self.mem.alloc(like, n + 2 * BAND)
        assert self.mem.ptr(flat) % 64 == 0
        self.mem.fill(flat[:BAND], band_bits)
        self.mem.fill(flat[BAND + n:], band_bits)
        if interior_bits is not None:
            self.mem.fill(flat[BAND:BAND + n], interior_bits)
        rec = _Rec("%s#%d %s" % (name, len(self.records), tuple(shape)), flat, n, band_bits)
        self.records.append(rec)
        view = flat[BAND:BAND + n].reshape(tuple(int(d) for d in shape))
        self._mine[self.inner.ptr(view)] = rec
        return view, rec

    def prepare(self, a):
        a = self.inner.prepare(a)
        if self.inner.ptr(a) in self._mine or 0 in self.inner.shape(a):
            return a                  # a result of an earlier guarded call, used as an input: it has its bands
        view, rec = self._banded(a, self.inner.shape(a), "input", INPUT_BAND_BITS)
        self.mem.store(rec.flat[BAND:BAND + rec.n], a)
        return view

    def empty(self, like, shape):
        return self._banded(like, shape, "output", BAND_BITS, NAN_BITS)[0]

    def filled(self, like, values):
        """A banded destination holding `values` (a host array): req 'add' bases, req-null fills, concat buffers."""
        values = np.ascontiguousarray(values, np.float32)
        view, rec = self._banded(like, values.shape, "destination", BAND_BITS)
        self.mem.store(rec.flat[BAND:BAND + rec.n], values if isinstance(self.mem, _NumpyMem) else self.mem.torch.from_numpy(values).to(like.device))
        return view

    def empty_bytes(self, like, nbytes):
        nbytes = int(nbytes)
        assert nbytes % 4 == 0, "a byte count that is no multiple of 4: %d" % nbytes
        self.last_stale = STALE_BITS | (self.calls & 0xFFFF)
        self.calls += 1
        view, _ = self._banded(like, (nbytes // 4,), "bytes[%d]" % nbytes, BAND_BITS, self.last_stale)
        self._exact[self.inner.ptr(view)] = nbytes
        return view

    def nbytes(self, a):
        return self._exact.get(self.inner.ptr(a), self.inner.nbytes(a))

    def verify(self):
        """Every band bit for bit; names the buffer, the side and the first offset (in floats from the buffer's first / past its last
        element) that changed."""
        for rec in self.records:
            for side, lo, hi in (("before", 0, BAND), ("after", BAND + rec.n, 2 * BAND + rec.n)):
                got = self.mem.bits(rec.flat[lo:hi])
                bad = np.flatnonzero(got != np.uint32(rec.band_bits))
                if bad.size:
                    first = int(bad[-1]) - BAND if side == "before" else int(bad[0])
                    at = int(bad[-1] if side == "before" else bad[0])
                    raise AssertionError("%s: the band %s the buffer changed at float offset %d (%d floats changed; 0x%08x -> 0x%08x)"
                                         % (rec.name, side, first, bad.size, rec.band_bits, int(got[at])))


class GuardedOpSet(OpSet):
    def _workspace(self, like, nbytes):
        return self.ad.empty_bytes(like, int(nbytes))    # fresh, exact, stale-filled; adapter.nbytes() answers `nbytes` itself


class GuardedEnv:
    """An fp64_env.Env whose ops hand out guarded buffers (the same library, the same moves, tuning and launch record)."""

    def __init__(self, env):
        self.env, self.emu = env, env.emu
        self.ad = GuardedAdapter(env.ops.ad)
        self.ops = GuardedOpSet(env.ops.ns, self.ad, env.ops.check)
        self.dev, self.host = env.dev, env.host
        self.set_tuning, self.launches = env.set_tuning, env.launches

    def filled(self, values):
        """A banded device buffer holding `values`."""
        return self.ad.filled(self.dev(np.zeros(1, np.float32)), values)

    def verify(self):
        self.ad.verify()


def guarded_env(env):
    return GuardedEnv(env)


def launch_list(env, L):
    """The launches a fp64_env.Launches block saw, in order: the emulation's log name by name; on the GPU the library's record, (name,
    count) in order of first launch."""
    if env.emu:
        return list(L.log)
    import ctypes
    from maskflownet_amd import _lib
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.lib().profile_dump(buf, len(buf))
    return [tuple(line.split(" ")[:2]) for line in buf.value.decode().splitlines() if line]


def to_host(env, res):
    """A call's results on the host: a tuple of arrays (None kept)."""
    res = res if isinstance(res, (tuple, list)) else (res,)
    return tuple(None if r is None else np.array(env.host(r)) for r in res)


def run_guarded(genv, call, expect=(), what=""):
    """call(genv) under the launch record; -> (results on the host, launch list), after every band was verified.  Leaving the launch
    record synchronises the device: the bands are read after the kernels have finished.  expect: kernels the record must hold."""
    with genv.launches() as L:
        res = call(genv)
    L.expect(expect, what=what)
    launches = launch_list(genv, L)
    out = to_host(genv, res)
    genv.verify()
    return out, launches
