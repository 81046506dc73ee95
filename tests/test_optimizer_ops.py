"""The trainer's Adam step (maskflownet_amd/csrc/kernels/optimizer.h: mfn_adam_update, mfn_multi_adam_update and its host-built table;
ops.adam_update / multi_adam_table / multi_adam_update; training.Trainer, learning_rate_at, save_checkpoint / load_checkpoint).

Reference: tests/optimizer_ref.py -- MXNet 1.5's adam_update as Adam.update calls it, in fp32 (every operation rounded: the twin) and
in fp64, M the same expression over absolute values.  Bars: on the emulation w, m and v are the twin's bits; on the GPU
parity_cases.check_fp64_bound per element (4 x the twin's own error + 16 * 2^-24 of M, exact zeros where M == 0, finite,
non-vacuous), and the test prints whether the result was the twin's bits as well.  The kernel tables run on the emulation here and
under -m gpu on the MI355X."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import optimizer_ref as orf
from tests import parity_cases as pc
from tests import test_memory_contract as mc
from tests.fp64_env import Env

U = 2.0 ** -24
CHUNK = 4096                                                   # ADAM_CHUNK (kernels/optimizer.h): 256 threads, four quads each
# every count the issue names, in an order that puts a one-element tensor between two multi-block ones
COUNTS = (2 * CHUNK + 7, 1, CHUNK + 1, 3, 4, 5, CHUNK - 1, CHUNK)
LR_MULTS = (1.0, 0.5, 2.0, 1.0, 0.25, 1.0, 3.0, 1.0)
WD_MULTS = (1.0, 0.0, 1.0, 2.0, 1.0, 0.5, 1.0, 0.0)
FORMS = ("multi", "multi-views", "single", "single-views")
ONES = (1.0,) * len(COUNTS)
# name: (t, wd, clip, lr_mults, wd_mults).  The learning rate is lr_t(1e-4, t); rescale_grad is 1 / 3 (a batch of three).
ARITH = {
    "t1": (1, 0.0, None, ONES, ONES),
    "t2 wd": (2, 1e-2, None, ONES, WD_MULTS),
    "t1000 clip lr_mult": (1000, 0.0, 1.0, LR_MULTS, ONES),
    "t2 wd clip mults": (2, 1e-2, 1e-3, LR_MULTS, WD_MULTS),
}
BETA1, BETA2, EPS, RESCALE = 0.9, 0.999, 1e-8, 1.0 / 3.0


def graded(rng, n):
    """Signed values whose magnitudes are graded over 1e-9 .. 1e3: g * g stays above 1e-18, far from the denormal range."""
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-9.0, 3.0, n)).astype(np.float32)


def make_inputs(arith, seed=0):
    """-> [(w, grad, m, v)] per tensor of COUNTS.  t == 1 starts from zero state; later steps from a state of the gradients' scale."""
    t = ARITH[arith][0]
    rng = np.random.default_rng([len(arith), t, seed])
    out = []
    for n in COUNTS:
        w = (0.1 * rng.standard_normal(n)).astype(np.float32)
        g = graded(rng, n)
        if t == 1:
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        else:
            m = (0.1 * graded(rng, n)).astype(np.float32)
            v = (graded(rng, n).astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
        out.append((w, g, m, v))
    return out


def hyper(arith):
    t, wd, clip, _, _ = ARITH[arith]
    return dict(lr=orf.lr_t(1e-4, BETA1, BETA2, t), beta1=BETA1, beta2=BETA2, epsilon=EPS, wd=wd, rescale_grad=RESCALE,
                clip_gradient=-1.0 if clip is None else clip)


_REFS = {}


def references(key, tensors, hp, lr_mults, wd_mults):
    """Computed once per input set, shared by the emulation and the GPU side, never modified."""
    if key not in _REFS:
        rows = []
        for q, lm, wm in zip(tensors, lr_mults, wd_mults):
            kw = dict(hp, lr_mult=lm, wd_mult=wm)
            r32, r64, M = orf.adam_step(*q, **kw), orf.adam_step(*q, dtype=np.float64, **kw), orf.adam_magnitude(*q, **kw)
            for a in r32 + r64 + M:
                a.setflags(write=False)
            rows.append((r32, r64, M))
        _REFS[key] = rows
    return _REFS[key]


def flat_views(env, tensors, fill=None):
    """The tensors as views at UNPADDED offsets of one flat device buffer per kind (w, grad, m, v): with these counts some views
    start on 16 bytes and take the 16-byte route while their neighbours take the one-element route.  -> ([(w, g, m, v) views], flats)."""
    total = sum(COUNTS)
    flats = []
    for k in range(4):
        host = np.concatenate([q[k] for q in tensors])
        flats.append(fill(host) if fill is not None else env.dev(host.copy()))
    views, off = [], 0
    for n in COUNTS:
        views.append(tuple(f[off:off + n] for f in flats))
        off += n
    assert off == total
    return views, flats


def run(env, form, tensors, hp, lr_mults, wd_mults, fill=None):
    """One step in place on fresh device copies -> [(w', m', v') on the host] per tensor."""
    o = env.ops
    if form.endswith("views"):
        dev, _ = flat_views(env, tensors, fill)
        aligned = [sum(COUNTS[:i]) % 4 == 0 for i in range(len(COUNTS))]
        assert any(aligned) and not all(aligned)
    else:
        dev = [tuple((fill(a) if fill is not None else env.dev(a.copy())) for a in q) for q in tensors]
    if form.startswith("multi"):
        table = o.multi_adam_table(*zip(*dev), lr_mults=lr_mults, wd_mults=wd_mults)
        assert table.n_tensors == len(COUNTS) and table.n_blocks == sum((n + CHUNK - 1) // CHUNK for n in COUNTS)
        o.multi_adam_update(table, **hp)
    else:
        for (w, g, m, v), lm, wm in zip(dev, lr_mults, wd_mults):   # the operator itself has no multipliers: they go into lr and wd
            f = np.float32
            o.adam_update(w, g, m, v, **dict(hp, lr=float(f(hp["lr"]) * f(lm)), wd=float(f(hp["wd"]) * f(wm))))
    return [tuple(np.array(env.host(a)) for a in (w, m, v)) for w, _, m, v in dev]


def check_case(env, form, arith):
    _, _, _, lr_mults, wd_mults = ARITH[arith]
    tensors, hp = make_inputs(arith), hyper(arith)
    what = "%s, %s" % (form, arith)
    with env.launches() as L:
        got = run(env, form, tensors, hp, lr_mults, wd_mults)
    kernel, other = ("multi_adam_update", "adam_update") if form.startswith("multi") else ("adam_update", "multi_adam_update")
    assert L.count(kernel) >= 1, "%s: kernel %s did not run" % (what, kernel)
    if env.emu:                                     # (the GPU's record matches names by substring)
        assert L.log.count(kernel) == (1 if form.startswith("multi") else len(COUNTS)) and L.log.count(other) == 0, L.log
    got2 = run(env, form, tensors, hp, lr_mults, wd_mults)                               # determinism: bit-identical replays
    refs = references(arith, tensors, hp, lr_mults, wd_mults)
    same = total = 0
    for n, g, g2, (r32, r64, M) in zip(COUNTS, got, got2, refs):
        for name, a, a2, t32, w64, m in zip(("w", "m", "v"), g, g2, r32, r64, M):
            tag = "%s, tensor of %d, %s" % (what, n, name)
            np.testing.assert_array_equal(a.view(np.uint32), a2.view(np.uint32), err_msg=tag)
            pc.assert_magnitude_bound(m, w64, tag)
            if env.emu:                             # the same operations in the same order: the twin's bits
                np.testing.assert_array_equal(a.view(np.uint32), t32.view(np.uint32), err_msg=tag)
            if n >= 3:                              # (one element cannot show that the bar can fail)
                pc.check_fp64_bound(a, w64, t32, m, tag)
            else:
                assert np.abs(a.astype(np.float64) - w64).max() <= (4 * np.abs(t32 - w64) + 16 * U * m).max(), tag
            same += int((a.view(np.uint32) == t32.view(np.uint32)).sum())
            total += a.size
    print("%s: %d of %d elements of w, m, v have the bits of the fp32 statement" % (what, same, total))
    if arith == "t1000 clip lr_mult":               # the clip has work on both sides and in between
        gs = np.concatenate([np.float32(RESCALE) * q[1] for q in tensors])
        assert (gs > 1.0).any() and (gs < -1.0).any() and (np.abs(gs) < 1.0).any()


PARAMS = [(f, a) for f in FORMS for a in ARITH]


@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


@pytest.mark.parametrize("form,arith", PARAMS)
def test_emu_adam_against_the_statement(emu, form, arith):
    check_case(emu, form, arith)


@pytest.mark.gpu
@pytest.mark.parametrize("form,arith", PARAMS)
def test_gpu_adam_against_the_statement(gpu, form, arith):
    check_case(gpu, form, arith)


# ---- CPU: the reference itself ---------------------------------------------------------------------------------------------------
def test_reference_statement_rounds_every_operation_and_differs_from_torch():
    """The fp32 statement against an element-by-element evaluation with Python's own fp32 roundings, lr_t against Adam.update's
    lines, and the two optimizers: three steps at lr 1e-4 on g = 1e-6 * randn end more than 0.5 lr apart in some weight."""
    import math
    f = np.float32
    rng = np.random.default_rng(1)
    w, g, m, v = (0.1 * rng.standard_normal(64)).astype(f), graded(rng, 64), (0.1 * graded(rng, 64)).astype(f), (graded(rng, 64) ** 2).astype(f)
    hp = dict(lr=orf.lr_t(1e-4, BETA1, BETA2, 7), wd=1e-2, rescale_grad=RESCALE, clip_gradient=1.0, lr_mult=0.5, wd_mult=2.0)
    w1, m1, v1 = orf.adam_step(w, g, m, v, **hp)
    lr, wd, rs, b1, b2, eps, c = f(f(hp["lr"]) * f(0.5)), f(f(1e-2) * f(2.0)), f(RESCALE), f(BETA1), f(BETA2), f(EPS), f(1.0)
    for i in range(64):
        gi = f(f(rs * g[i]) + f(wd * w[i]))
        gi = min(max(gi, -c), c)
        mi = f(f(b1 * m[i]) + f(f(f(1.0) - b1) * gi))
        vi = f(f(b2 * v[i]) + f(f(f(1.0) - b2) * f(gi * gi)))
        wi = f(w[i] - f(f(lr * mi) / f(f(np.sqrt(vi)) + eps)))
        assert (mi, vi, wi) == (m1[i], v1[i], w1[i]), i
    assert orf.lr_t(1e-4, 0.9, 0.999, 1) == float(f(1e-4 * math.sqrt(1 - 0.999) / (1 - 0.9)))
    assert abs(orf.lr_t(1e-4, 0.9, 0.999, 10 ** 6) - 1e-4) < 1e-11
    rng = np.random.default_rng(0)
    w0, grads = rng.standard_normal(4096).astype(f), [(1e-6 * rng.standard_normal(4096)).astype(f) for _ in range(3)]
    a, b = (w0, np.zeros_like(w0), np.zeros_like(w0)), (w0.astype(np.float64), 0.0 * w0, 0.0 * w0)
    for t, gr in enumerate(grads, 1):
        wa, ma, va = orf.adam_step(a[0], gr, a[1], a[2], lr=orf.lr_t(1e-4, 0.9, 0.999, t))
        a = (wa, ma, va)
        b = orf.torch_adam_step(b[0], gr, b[1], b[2], t, 1e-4)
    assert np.abs(a[0] - b[0]).max() > 0.5 * 1e-4


SCHEDULE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sintel_lr_schedule.json")))["learning_rate"]


def test_learning_rate_at_follows_the_reference_schedule():
    """pipeline.py:65-75 on the reference's MaskFlownet_S_sintel.yaml schedule (tests/golden/sintel_lr_schedule.json): at every
    boundary, one step either side of it, and past the end."""
    from maskflownet_amd import training
    assert len(SCHEDULE) == 18 and SCHEDULE[0] == [100000, 5.0e-5] and SCHEDULE[-1] == [1000000, 1.25e-7]
    assert training.learning_rate_at(SCHEDULE, 0) == 5.0e-5
    for i, (boundary, lr) in enumerate(SCHEDULE):
        assert training.learning_rate_at(SCHEDULE, boundary - 1) == lr
        assert training.learning_rate_at(SCHEDULE, boundary) == lr                       # strict comparison: steps > boundary moves on
        nxt = SCHEDULE[i + 1][1] if i + 1 < len(SCHEDULE) else None
        assert training.learning_rate_at(SCHEDULE, boundary + 1) == nxt
    assert training.learning_rate_at(SCHEDULE, 10 ** 7) is None and training.learning_rate_at([], 0) is None


def _cpu_params(sizes=((3, 5), (7,), (2, 2, 3, 3), (1,), (6, 4), (9,)), frozen=()):
    import torch
    g = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in sizes]
    for i in frozen:
        ps[i].requires_grad_(False)
    return ps


def test_gradient_buckets_align_and_default_layout():
    """align=1 (the default) keeps the back-to-back layout: every view starts where the previous one ended, the bucket has no
    padding; align=4 starts every view on 16 bytes and the padding is zero."""
    from maskflownet_amd import training
    ps = _cpu_params()
    for kw in ({}, {"align": 1}):
        gb = training.GradientBuckets(ps, n_buckets=2, **kw)
        assert sum(b.numel() for b in gb.buckets) == sum(p.numel() for p in ps)
        for flat, grp, offs in zip(gb.buckets, gb.members, gb.offsets):
            off = 0
            for p, o in zip(grp, offs):
                assert o == off and p.grad.data_ptr() == flat.data_ptr() + 4 * off and p.grad.shape == p.shape
                off += p.numel()
            assert off == flat.numel()
        assert [id(p) for grp in gb.members for p in grp] == [id(p) for p in reversed(ps)]
    gb = training.GradientBuckets(ps, n_buckets=2, align=4)
    for flat, grp, offs in zip(gb.buckets, gb.members, gb.offsets):
        assert flat.data_ptr() % 16 == 0 and flat.numel() == sum((p.numel() + 3) // 4 * 4 for p in grp)
        for p, o in zip(grp, offs):
            assert o % 4 == 0 and p.grad.data_ptr() % 16 == 0 and p.grad.data_ptr() == flat.data_ptr() + 4 * o
        for p in grp:
            p.grad.fill_(1.0)
        assert flat.sum().item() == sum(p.numel() for p in grp)                         # the padding stayed zero


def _gloo_worker(rank, port, q):
    import torch
    import torch.distributed as dist
    from maskflownet_amd import training
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=2)
    try:
        out = {}
        for scale in (False, True):
            ps = _cpu_params()
            gb = training.GradientBuckets(ps, n_buckets=2, dist=dist, align=4)
            gb.zero()
            sum((p * float(rank + 1)).sum() for p in ps).backward()
            gb.finish(8, scale=scale) if scale else gb.finish(scale=False)
            out[scale] = [p.grad.clone().numpy() for p in ps]
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_finish_without_scale_leaves_the_gloo_sum():
    """World 2 over gloo: rank r's gradients are r + 1 everywhere, so the all-reduced sum is 3; finish(scale=False) leaves it, the
    default divides by the global batch."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank in (0, 1):
        for g in res[rank][False]:
            assert (g == 3.0).all()
        for g in res[rank][True]:
            assert (g == np.float32(3.0) * np.float32(1.0 / 8)).all()


# ---- structure: guard bands, determinism, NaN, n == 0 ---------------------------------------------------------------------------------
def _contract_case(form, arith):
    _, _, _, lr_mults, wd_mults = ARITH[arith]
    tensors, hp = make_inputs(arith, seed=1), hyper(arith)

    def call(env):
        """Every tensor (or flat buffer) and the table between guard bands on a guarded env; -> every w', m', v' and the gradients."""
        o = env.ops
        fill = lambda a: mc.dest(env, a)
        if form.endswith("views"):
            dev, flats = flat_views(env, tensors, fill)
            res = tuple(flats)
        else:
            dev = [tuple(fill(a) for a in q) for q in tensors]
            res = tuple(a for q in dev for a in q)
        if form.startswith("multi"):
            o.multi_adam_update(o.multi_adam_table(*zip(*dev), lr_mults=lr_mults, wd_mults=wd_mults), **hp)
        else:
            for w, g, m, v in dev:
                o.adam_update(w, g, m, v, **hp)
        return res
    return mc.Case(call, ["multi_adam_update" if form.startswith("multi") else "adam_update"])


CONTRACT = {"multi": _contract_case("multi", "t2 wd clip mults"), "multi-views": _contract_case("multi-views", "t2 wd clip mults"),
            "single": _contract_case("single", "t1000 clip lr_mult"), "single-views": _contract_case("single-views", "t2 wd")}


@pytest.mark.parametrize("name", list(CONTRACT))
def test_emu_memory_contract(emu, name):
    mc.contract(emu, name, CONTRACT[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONTRACT))
def test_gpu_memory_contract(gpu, name):
    mc.contract(gpu, name, CONTRACT[name])


def check_nan_and_empty(env):
    """A NaN gradient poisons exactly its own element of w, m and v -- in a 16-byte quad, in the scalar tail and on the one-element
    route --, every other element keeps the bits of the clean run; n == 0 succeeds."""
    arith = "t2 wd"
    _, _, _, lr_mults, wd_mults = ARITH[arith]
    tensors, hp = make_inputs(arith), hyper(arith)
    clean = run(env, "multi-views", tensors, hp, lr_mults, wd_mults)
    spots = {0: [5, CHUNK + 2, 2 * CHUNK + 6], 1: [0], 2: [CHUNK], 6: [17, CHUNK - 2]}       # tensor -> elements
    dirty = [tuple(a.copy() for a in q) for q in tensors]
    for ti, idx in spots.items():
        dirty[ti][1][idx] = np.nan
    got = run(env, "multi-views", dirty, hp, lr_mults, wd_mults)
    for ti, (g, c) in enumerate(zip(got, clean)):
        bad = np.zeros(COUNTS[ti], bool)
        bad[spots.get(ti, [])] = True
        for a, b in zip(g, c):
            assert np.isnan(a[bad]).all() and not np.isnan(a[~bad]).any(), ti
            np.testing.assert_array_equal(a[~bad].view(np.uint32), b[~bad].view(np.uint32))
    z = env.dev(np.zeros(0, np.float32))
    with env.launches() as L:
        env.ops.adam_update(z, z, z, z, 1e-4)
        assert env.ops.ns.adam_update(None, None, None, None, 0, 1e-4, .9, .999, 1e-8, 0., 1., -1., None) == 0
        nb, tag = ctypes.c_int(-1), ctypes.c_ulonglong()
        assert env.ops.ns.multi_adam_build_table(0, None, None, None, None, None, None, None, None, 0, ctypes.byref(nb), ctypes.byref(tag)) == 0
        assert nb.value == 0
        assert env.ops.ns.multi_adam_update(None, 0, tag.value, 0, 0, 1e-4, .9, .999, 1e-8, 0., 1., -1., None) == 0
        w = env.dev(np.ones(3, np.float32))                  # a table whose only tensors are empty: no block, no launch
        table = env.ops.multi_adam_table([z, z], [z, z], [z, z], [z, z])
        assert table.n_blocks == 0
        env.ops.multi_adam_update(table, 1e-4)
    assert L.count("adam_update") == 0 and (not env.emu or L.log == [])
    assert (np.array(env.host(w)) == 1).all()


def test_emu_nan_gradient_and_empty_tensors(emu):
    check_nan_and_empty(emu)


@pytest.mark.gpu
def test_gpu_nan_gradient_and_empty_tensors(gpu):
    check_nan_and_empty(gpu)


# ---- argument checks: every error returns its code before any launch ------------------------------------------------------------------
def _argument_errors(ns, launches):
    one = ctypes.c_void_p(16)                     # never dereferenced
    P = lambda *v: (ctypes.c_void_p * len(v))(*v)
    LL = lambda *v: (ctypes.c_longlong * len(v))(*v)

    def single(w=one, g=one, m=one, v=one, n=8, lr=1e-4, b1=.9, b2=.999, eps=1e-8, wd=0., rs=1., clip=-1.):
        return ns.adam_update(w, g, m, v, n, lr, b1, b2, eps, wd, rs, clip, None)

    host = (ctypes.c_ulonglong * 64)()
    nb, tag = ctypes.c_int(), ctypes.c_ulonglong()

    def build(T=2, w=P(16, 32), g=P(16, 32), m=P(16, 32), v=P(16, 32), counts=LL(5, CHUNK + 1), buf=ctypes.addressof(host), nbytes=2 * 64 + 3 * 8,
              pnb=ctypes.byref(nb), ptag=ctypes.byref(tag)):
        return ns.multi_adam_build_table(T, w, g, m, v, counts, None, None, buf, nbytes, pnb, ptag)

    def multi(table=one, nbytes=2 * 64 + 3 * 8, tg=None, T=2, B=3, b1=.9, b2=.999, eps=1e-8):
        return ns.multi_adam_update(table, nbytes, tag.value if tg is None else tg, T, B, 1e-4, b1, b2, eps, 0., 1., -1., None)

    with launches() as L:
        assert single(n=-1) == -2 and b"n=-1" in ns.last_error()
        for k in "wgmv":
            assert single(**{k: None}) == -1 and b"NULL" in ns.last_error()
        assert single(w=ctypes.c_void_p(18)) == -6
        for call in (single, multi):
            assert call(b1=1.0) == -3 and b"beta" in ns.last_error()
            assert call(b1=-0.1) == -3 and call(b2=1.0) == -3 and call(b2=-1e-3) == -3 and call(b1=float("nan")) == -3
            assert call(eps=-1e-8) == -3 and b"epsilon" in ns.last_error()
        assert single(w=None, g=None, m=None, v=None, n=0) == 0
        assert ns.multi_adam_table_bytes(2, LL(5, CHUNK + 1)) == 2 * 64 + 3 * 8
        assert ns.multi_adam_table_bytes(2, LL(5, -1)) == 0 and ns.multi_adam_table_bytes(0, LL(5)) == 0 and ns.multi_adam_table_bytes(1, None) == 0
        assert build(counts=LL(5, -1)) == -2 and b"count -1 of tensor 1" in ns.last_error()
        assert build(T=-1) == -2
        assert build(w=P(16, None)) == -1 and b"tensor 1" in ns.last_error()
        assert build(g=None) == -1 and build(counts=None) == -1 and build(pnb=None) == -1 and build(ptag=None) == -1
        assert build(m=P(18, 32)) == -6
        assert build(nbytes=2 * 64 + 3 * 8 - 8) == -5 and build(buf=None) == -5
        assert build(w=P(None, 32), counts=LL(0, CHUNK + 1), nbytes=2 * 64 + 2 * 8) == 0 and nb.value == 2      # an empty tensor may be NULL
        assert build() == 0 and nb.value == 3
        blocks = np.frombuffer(host, np.uint32, 6, 2 * 64)
        assert blocks.tolist() == [0, 0, 1, 0, 1, 1]                                    # {tensor, chunk} per block
        assert multi(table=None) == -1
        assert multi(tg=tag.value ^ 1) == -5 and b"re-run" in ns.last_error()
        assert multi(T=3) == -5 and multi(B=4) == -5                                     # the tag carries both counts
        assert multi(nbytes=2 * 64 + 3 * 8 + 8) == -5 and multi(nbytes=0) == -5
        assert multi(T=-1) == -2
    return L


def test_emu_argument_errors_launch_nothing(emu):
    L = _argument_errors(emu.ops.ns, emu.launches)
    assert L.log == [], L.log


def test_product_argument_errors_fail_before_any_launch():
    """The same table on libmfn_hip.so, without a GPU: every call returns its own (negative) code, so none reached a launch."""
    import contextlib
    from maskflownet_amd import _lib
    _lib.build()
    _argument_errors(_lib.lib(), lambda: contextlib.nullcontext())


def test_ops_shape_errors_and_cpu_tensors():
    import torch
    from maskflownet_amd import _lib, ops, training
    from tests.emu import emu_ops
    _lib.build()
    o = emu_ops.emu_ops()
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ValueError, match="grad has shape"):
        o.adam_update(z(4), z(5), z(4), z(4), 1e-4)
    with pytest.raises(ValueError, match="must be contiguous"):
        o.adam_update(z(4, 4)[:, ::2], z(4, 2), z(4, 2), z(4, 2), 1e-4)
    with pytest.raises(ValueError, match="one grad, mean and var per weight"):
        o.multi_adam_table([z(4)], [z(4), z(4)], [z(4)], [z(4)])
    with pytest.raises(ValueError, match="lr_mults must have one entry"):
        o.multi_adam_table([z(4)], [z(4)], [z(4)], [z(4)], lr_mults=[1.0, 2.0])
    w, g, m, v = z(8), z(8), z(8), z(8)
    table = o.multi_adam_table([w], [g], [m], [v])
    assert not table.stale([[a.ctypes.data for a in (w, g, m, v)]]) and table.stale([[a.ctypes.data for a in (w, g, m, z(8))]])
    t = torch.zeros(4)
    with pytest.raises(TypeError, match="ROCm device"):
        ops.adam_update(t, t, t, t, 1e-4)
    with pytest.raises(ValueError, match="only 'adam'"):
        training.Trainer({"a": torch.nn.Parameter(t)}, "sgd")
    with pytest.raises(ValueError, match="unknown optimizer parameters"):
        training.Trainer({"a": torch.nn.Parameter(t)}, "adam", {"momentum": 0.9})
    with pytest.raises(ValueError, match="no parameter with requires_grad"):
        training.Trainer({"a": torch.nn.Parameter(t, requires_grad=False)})


# ---- the trainer, on the GPU -----------------------------------------------------------------------------------------------------------
def _statement_check(what, before, grads, mean, var, after, lr, batch, hp=None, names=None):
    """after[k] against adam_step applied to the snapshot (before, grads, mean, var), parameter by parameter, under the kernel rule."""
    hp = dict(dict(beta1=BETA1, beta2=BETA2, epsilon=EPS, wd=0.0, clip_gradient=-1.0), **(hp or {}))
    same = total = 0
    worst = 0.0
    for k in (names or list(before)):
        q = (before[k].ravel(), grads[k].ravel(), mean[k].ravel(), var[k].ravel())
        kw = dict(hp, lr=lr, rescale_grad=1.0 / batch)
        r32, r64, M = orf.adam_step(*q, **kw), orf.adam_step(*q, dtype=np.float64, **kw), orf.adam_magnitude(*q, **kw)
        got = after[k].ravel()
        if got.size >= 3 and (M[0] > 0).any():
            e_lib, _ = pc.check_fp64_bound(got, r64[0], r32[0], M[0], "%s, %s" % (what, k))
            worst = max(worst, e_lib)
        else:
            assert (np.abs(got.astype(np.float64) - r64[0]) <= 4 * np.abs(r32[0] - r64[0]) + 16 * U * M[0]).all(), k
        same += int((got.view(np.uint32) == r32[0].view(np.uint32)).sum())
        total += got.size
    print("%s: %d of %d weights have the bits of the fp32 statement; largest error %.2f ulp of M" % (what, same, total, worst / U))
    return same, total


def _snap(d):
    return {k: t.detach().cpu().numpy().copy() for k, t in d.items()}


@pytest.mark.gpu
def test_gpu_three_steps_follow_mxnet_and_leave_torch():
    """Fidelity: three Trainer.steps at lr 1e-4 on fixed gradients 1e-6 * randn equal the MXNet statement step by step, and end more
    than 0.5 lr away from torch.optim.Adam on the same gradients in some weight (the two reference statements alone: 1.97 lr)."""
    import torch
    from maskflownet_amd import training
    g = torch.Generator().manual_seed(0)
    shapes = {"a.weight": (16, 8, 3, 3), "a.bias": (16,), "b.weight": (CHUNK + 5,), "c.weight": (3, 7)}
    params = {k: torch.nn.Parameter(torch.randn(*s, generator=g).cuda()) for k, s in shapes.items()}
    twins = {k: torch.nn.Parameter(p.detach().clone()) for k, p in params.items()}
    grads = [{k: (1e-6 * torch.randn(*s, generator=g)).cuda() for k, s in shapes.items()} for _ in range(3)]
    tr = training.Trainer(params, "adam", {"learning_rate": 1e-4})
    opt = torch.optim.Adam(list(twins.values()), lr=1e-4)
    for t, gr in enumerate(grads, 1):
        tr.buckets.zero()
        for k, p in params.items():
            p.grad.copy_(gr[k])
            twins[k].grad = gr[k].clone()
        before, mean, var = _snap(params), _snap(tr.mean), _snap(tr.var)
        assert tr.lr_t() == orf.lr_t(1e-4, BETA1, BETA2, t)
        tr.step(1)
        opt.step()
        assert tr.num_update == t
        _statement_check("step %d" % t, before, _snap(gr), mean, var, _snap(params), orf.lr_t(1e-4, BETA1, BETA2, t), 1)
    far = max((params[k].detach() - twins[k].detach()).abs().max().item() for k in params)
    print("Trainer against torch.optim.Adam after three steps: %.3f lr" % (far / 1e-4))
    assert far > 0.5 * 1e-4


def _net_batch(seed=0):
    from maskflownet_amd import network, training
    from tests.test_training_step import _batch
    net = training.MaskFlownetSTrainable(network.random_params(seed)).cuda()
    return net, [t.cuda() for t in _batch(2, 64, 64, 6)]


def _hook_step(trainer, log):
    """Snapshots parameters, the UNSCALED buckets' views and the state when step is entered (after backward): what the update reads."""
    inner = trainer.step

    def step(batch_size):
        named = dict(zip(trainer.names, trainer.params))
        log.append({"before": _snap(named), "grads": _snap({k: p.grad for k, p in named.items()}), "mean": _snap(trainer.mean),
                    "var": _snap(trainer.var), "batch": batch_size, "lr": trainer.lr_t()})
        inner(batch_size)
        log[-1]["after"] = _snap(named)
    trainer.step = step


@pytest.mark.gpu
def test_gpu_train_step_with_a_trainer_and_resume(tmp_path):
    """train_step of MaskFlownetSTrainable at 64 x 64, batch 2, with a Trainer: the parameters after each step are the statement applied
    to what the step read (the backward's atomics never enter); two steps with set_learning_rate in between use lr_t of t = 1, 2;
    save_checkpoint / load_checkpoint into a fresh net and trainer, then one more step on saved gradients: bit-identical parameters."""
    import torch
    from maskflownet_amd import training
    net, (im1, im2, label, mask) = _net_batch()
    loss_fn = training.FusedMultiscaleEpe()
    tr = training.Trainer(training.reference_named_parameters(net), "adam", {"learning_rate": 1e-4})
    assert len(tr.names) == 142 and "conv1a.weight" in tr.names and all(p.grad.data_ptr() % 16 == 0 for p in tr.params)
    log = []
    _hook_step(tr, log)
    training.train_step(net, loss_fn, tr, im1, im2, label, mask)
    tr.set_learning_rate(5e-5)
    assert tr.learning_rate == 5e-5
    loss = training.train_step(net, loss_fn, tr, im1, im2, label, mask)
    assert torch.isfinite(loss).all() and len(log) == 2 and tr.num_update == 2
    assert log[0]["lr"] == orf.lr_t(1e-4, BETA1, BETA2, 1) and log[1]["lr"] == orf.lr_t(5e-5, BETA1, BETA2, 2) and log[0]["batch"] == 2
    assert any(np.abs(g).max() > 0 for g in log[1]["grads"].values())
    for i, s in enumerate(log):
        _statement_check("train_step %d" % (i + 1), s["before"], s["grads"], s["mean"], s["var"], s["after"], s["lr"], 2)
    # resume: the uninterrupted run takes a third step on fixed gradients; the resumed one starts from the checkpoint
    prefix = str(tmp_path / "ckpt")
    training.save_checkpoint(prefix, net, tr)
    fixed = {k: torch.from_numpy(g).cuda() for k, g in log[1]["grads"].items()}

    def third(trainer):
        trainer.buckets.zero()
        for k, p in zip(trainer.names, trainer.params):
            p.grad.copy_(fixed[k])
        trainer.step(2)
    third(tr)
    net2, _ = _net_batch(seed=1)
    tr2 = training.Trainer(training.reference_named_parameters(net2), "adam", {"learning_rate": 1e-3})
    training.load_checkpoint(prefix, net2, tr2)
    assert tr2.num_update == 2 and tr2.learning_rate == 5e-5
    third(tr2)
    for (k, p), (_, p2) in zip(training.reference_named_parameters(net), training.reference_named_parameters(net2)):
        assert torch.equal(p.detach(), p2.detach()), k
    for k in tr.names:
        assert torch.equal(tr.mean[k], tr2.mean[k]) and torch.equal(tr.var[k], tr2.var[k]), k
    # load_states refuses a missing name, an unexpected one and a wrong shape, and changes nothing then
    from maskflownet_amd import io
    states = io.load_params(prefix + ".states")
    assert states["trainer:adam"].dtype == np.float64 and states["trainer:adam"][0] == 2 and "mean:conv1a.weight" in states
    kept = tr2.mean["conv1a.weight"].clone()
    for name, change, err in (("missing", lambda d: d.pop("var:conv1a.weight"), KeyError), ("unexpected", lambda d: d.update({"mean:nobody": np.zeros(1, np.float32)}), KeyError),
                              ("shape", lambda d: d.update({"mean:conv1a.weight": np.zeros((2, 2), np.float32)}), ValueError)):
        bad = dict(states)
        change(bad)
        io.save_params(str(tmp_path / (name + ".states")), bad)
        with pytest.raises(err):
            tr2.load_states(str(tmp_path / (name + ".states")))
        assert torch.equal(tr2.mean["conv1a.weight"], kept) and tr2.num_update == 3


@pytest.mark.gpu
def test_gpu_frozen_parameters_and_their_state_are_never_touched():
    """fix_head (main.py:139): a Trainer over the full model takes the cascade only; the head's parameters keep their bits through a
    step, the trainer holds no state under their names, and a parameter frozen by hand in the S network is left alone as well."""
    import torch
    from maskflownet_amd import network, training
    net = training.MaskFlownetTrainable(network.random_params(3, full=True)).cuda()
    named = training.reference_named_parameters(net)
    head = {k: p.detach().clone() for k, p in named if k.startswith(network.HEAD)}
    assert len(head) == 142 and all(not p.requires_grad for k, p in named if k in head)
    tr = training.Trainer(named, "adam", {"learning_rate": 1e-2})
    assert not any(k.startswith(network.HEAD) for k in tr.names) and len(tr.names) == len(named) - 142
    assert set(tr.mean) == set(tr.names) == set(tr.var)
    g = torch.Generator(device="cuda").manual_seed(0)
    tr.buckets.zero()
    for b in tr.buckets.buckets:
        b.copy_(torch.randn(b.shape, device="cuda", generator=g))
    before = {k: p.detach().clone() for k, p in named}
    tr.step(1)
    for k, p in named:
        assert torch.equal(p.detach(), before[k]) == (k in head), k
    net_s = training.MaskFlownetSTrainable(network.random_params(4)).cuda()
    named_s = training.reference_named_parameters(net_s)
    dict(named_s)["conv3b.weight"].requires_grad_(False)
    tr = training.Trainer(named_s, "adam", {"learning_rate": 1e-2})
    assert "conv3b.weight" not in tr.names and len(tr.names) == 141 and dict(named_s)["conv3b.weight"].grad is None
    before = {k: p.detach().clone() for k, p in named_s}
    for b in tr.buckets.buckets:
        b.fill_(1.0)
    tr.step(1)
    for k, p in named_s:
        assert torch.equal(p.detach(), before[k]) == (k == "conv3b.weight"), k


@pytest.mark.gpu
def test_gpu_a_trained_deformable_layer_repacks_its_weights():
    """layer.DeformableConv2D._packed keys its packed weights on weight._version, which a kernel writing through raw pointers does
    not advance: Trainer.step advances it.  After one step the layer gives the output of a fresh layer built from the updated weights;
    the same update without the version bump (the raw operator) leaves it on the old output."""
    import torch
    from maskflownet_amd import layer, ops, training
    g = torch.Generator().manual_seed(0)
    lay = layer.DeformableConv2D(16, 3, padding=1, in_channels=16).cuda()
    x, off = torch.randn(1, 16, 8, 8, generator=g).cuda(), torch.randn(1, 18, 8, 8, generator=g).cuda()

    def fresh():
        other = layer.DeformableConv2D(16, 3, padding=1, in_channels=16).cuda()
        with torch.no_grad():
            other.weight.copy_(lay.weight)
            other.bias.copy_(lay.bias)
            return other(x, off)
    with torch.no_grad():
        y0 = lay(x, off)
    assert torch.equal(y0, fresh())
    tr = training.Trainer(lay.named_parameters(), "adam", {"learning_rate": 1e-2})
    tr.buckets.zero()
    lay(x, off).square().sum().backward()
    version = lay.weight._version
    tr.step(1)
    assert lay.weight._version > version
    with torch.no_grad():
        y1 = lay(x, off)
    assert torch.equal(y1, fresh()) and not torch.equal(y1, y0)
    # the trap itself: the same kernel through the raw operator moves the weights and not the counter
    ops.adam_update(lay.weight.detach(), lay.weight.grad, tr.mean["weight"], tr.var["weight"], 1e-2)
    with torch.no_grad():
        stale = lay(x, off)
        assert torch.equal(stale, y1) and not torch.equal(stale, fresh())
        torch.autograd.graph.increment_version(lay.weight)
        assert torch.equal(lay(x, off), fresh())
