"""The plans the library takes at the reference's training and prediction resolutions, each one executed against fp64.

The plans are functions of N, C, H and W.  tests/dataset_shapes.py lists the reference's resolutions with their per-card batches and
every call MaskFlownet_S and the full MaskFlownet make at one.  In the emulation's dry-run mode (tests/test_dispatch_table.py) every
one of those calls is planned under ARITH_DEFAULT and ARITH_FP32 -- forward everywhere, the trainer's backward calls with its
requests at the training entries -- and reduced to a signature: the operator, the return code, the ordered launches as (kernel name,
block dims, dynamic LDS bytes) and, where a call launches dc_mma_kernel, the tiling mfn_debug_last_dc_plan reports.  The grid is
left out: it counts the work, and a plan that is kept at a smaller N and H runs the same template instance on the same block shape.

tests/data/dataset_plans_v1.json maps every distinct signature to ONE witness, with the arithmetics the datasets take it under:
  bench   a CFG2 / CFG3 level or a GPU_CONV / GPU_CONV_ROUTES row that the `-m gpu` halves of tests/test_forward_fp64.py and
          tests/test_backward_fp64.py already run, named in the record;
  case    a call of this file: the dataset call's channel counts and W, the smallest N and the smallest H with H % 8 unchanged that
          keep the signature (a dry-run search); "gpu_only" where the emulation of that shape is too slow for the CPU half.
On the CPU: every signature the datasets take has a witness, every witness planned in dry-run yields exactly its signature under every
arithmetic recorded for it, and the record has no entry no dataset call takes.  Rebuild it with

    MFN_DATASET_PLANS=write python -m pytest tests/test_dataset_plans.py -q -m "not gpu" -k ledger

and review the diff like tests/data/dispatch_v1.json.

What a signature does not hold.  The grid and the tensor extents are left out, so one signature covers every call that reaches the
same kernel instance with the same block and LDS request: the witness of `corr_dma_v22, 960 threads, 153 600 B` is the 32-channel
level 2 of the 320 x 768 crop, and the 64-channel (4, 64, 40, 96) call that shares the signature is executed by no witness.  A kernel
that loops over the channels in chunks runs more trips there; the same holds wherever a signature is shared across channel counts or
widths (the failure message of the ledger lists the calls behind each signature).

Every case witness then runs through the cases of the two fp64 files (imported, not copied) under parity_cases.check_fp64_bound, the
launches of its signature asserted from the launch record, inputs plain and graded per pixel: all of them on the GPU (`-m gpu`), on
the emulation those whose emulated run takes under about 20 s here (EMU_LEFT_OUT lists the others with their measured times).
On the emulation the launch record holds exact kernel names.  On the GPU the library's launch counters match a name by substring and
say only that at least one such launch happened ("conv3x3_mfma" is met by "deconv_as_conv3x3_mfma" too), and neither side records
block sizes or LDS bytes of a real run: that the recorded signature is what runs rests on the ledger's dry run and on the library
planning a call with the same code in both builds (maskflownet_amd/csrc/api_impl.inc)."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import ref as oracle
from tests import dataset_shapes as ds
from tests import parity_cases as pc
from tests import test_backward_fp64 as bwd64
from tests import test_forward_fp64 as fwd64
from tests.emu import emu_ops
from tests.fp64_env import Env
from tests.test_dispatch_table import _buf, _bufs, _conv_bwd_call, _corr_bwd_call, _corr_call, _dc_bwd_call, _status
from tests.test_emu_parity import DEFAULT_TUNING

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "dataset_plans_v1.json")
ARITHS = (-1, 0)                       # ARITH_DEFAULT, ARITH_FP32
REQ = {"w": 1, "n": 0, "a": 3}        # MFN_REQ_WRITE / _NULL / _ADD
DCM_KERNELS = ("dc_mma",)        # conv3x3_dcm is the same kernel, but its launcher reports no plan


# ---- a call as a key: a flat list, JSON as it stands ---------------------------------------------------------------------------------
# ["corr", N, C, H, W, md]                    ["corr_bwd", N, C, H, W, md, "wn"]
# ["conv" | "deconv", N, Cin, Cout, H, W, stride, dilate, act]        3x3 / pad = dilate; 4x4 / stride 2 / pad 1 transposed
# ["conv_bwd" | "deconv_bwd", N, Cin, Cout, H, W, stride, dilate, act, "nww"]
# ["deform_dropin" | "deform_shared", N, C, H, W]                      ["deform_shared_bwd", N, C, H, W, "nwww"]
# ["warp", N, C, H, W]    ["upsample", N, C, H, W, factor]    ["offsets", N, H, W]
def _req(req):
    return "".join(r[0] for r in req)


def keys_of(call, backward):
    """The ledger keys of one enumerated call: its forward, and with `backward` what the trainer asks of its backward."""
    d, g = list(call.dims), call.geo
    if call.op in ("conv", "deconv"):
        out = [[call.op] + d + [g["stride"][0], g["dilate"][0], int(g["act"])]]
        if backward and call.req:
            out.append([call.op + "_bwd"] + d + [g["stride"][0], g["dilate"][0], int(g["act"]), _req(call.req)])
        return out
    if call.op == "corr":
        return [["corr"] + d + [g["md"]]] + ([["corr_bwd"] + d + [g["md"], _req(call.req)]] if backward and call.req else [])
    if call.op == "deform_shared":
        return [[call.op] + d] + ([["deform_shared_bwd"] + d + [_req(call.req)]] if backward and call.req else [])
    if call.op == "offsets":
        return [["offsets", d[0], d[2], d[3]]]
    if call.op == "upsample":
        return [["upsample"] + d + [g["factor"]]]
    return [[call.op] + d]     # deform_dropin (the trainer's backward is the flow-shared one), warp


def dataset_keys():
    """{key (as a tuple): [the dataset entries that make the call]} over every table entry, both networks."""
    out = {}
    for e in ds.entries():
        for full in (False, True):
            for c in ds.calls(e.N, e.H, e.W, full):
                for k in keys_of(c, e.stage == "train"):
                    out.setdefault(tuple(k), [])
                    tag = "%s %s %dx%dx%d%s" % (e.name, e.stage, e.N, e.H, e.W, " full" if full else "")
                    if tag not in out[tuple(k)]:
                        out[tuple(k)].append(tag)
    return out


# ---- planning a key in dry-run mode ----------------------------------------------------------------------------------------------------
def _arr(tag, *shape):
    return _buf(tag, int(np.prod(shape)))[:int(np.prod(shape))].reshape(shape)


def _conv_geo(op, stride, dilate):
    if op.startswith("deconv"):
        return dict(kernel=(4, 4), stride=(2, 2), pad=(1, 1))
    return dict(kernel=(3, 3), stride=(stride, stride), pad=(dilate, dilate), dilate=(dilate, dilate))


def _plan(ops, key):
    """Issue the call of `key` (dry-run is on: nothing is computed, buffers are uninitialised) -> its return code."""
    ns, op = ops.ns, key[0]
    if op == "corr":
        return _corr_call(ns, tuple(key[1:5]), key[5])[0]
    if op == "corr_bwd":
        return _corr_bwd_call(ns, tuple(key[1:5]), key[5], [REQ[r] for r in key[6]])[0]
    if op in ("conv", "deconv"):
        N, Cin, Cout, H, W, stride, dilate, act = key[1:]
        geo = _conv_geo(op, stride, dilate)
        Ho, Wo = ops.conv_out_shape(H, W, geo["kernel"], geo["stride"], geo["pad"], geo.get("dilate", (1, 1)), op == "deconv")
        k = geo["kernel"][0]
        w = _arr("w", Cin, Cout, k, k) if op == "deconv" else _arr("w", Cout, Cin, k, k)
        fn = ops.Deconvolution if op == "deconv" else ops.Convolution
        return _status(lambda: fn(_arr("x", N, Cin, H, W), w, _arr("b", Cout), out=_arr("out", N, Cout, Ho, Wo),
                                  activation="leaky" if act else None, **geo))
    if op in ("conv_bwd", "deconv_bwd"):
        N, Cin, Cout, H, W, stride, dilate, act, req = key[1:]
        geo = _conv_geo(op, stride, dilate)
        kw = dict(k=geo["kernel"][0], stride=geo["stride"], pad=geo["pad"], dilate=geo.get("dilate", (1, 1)), transposed=int(op == "deconv_bwd"))
        return _conv_bwd_call(ns, (N, Cin, Cout, H, W, kw), act, [REQ[r] for r in req])[0]
    if op in ("deform_dropin", "deform_shared"):
        N, C, H, W = key[1:]
        x, w, b, out = _arr("x", N, C, H, W), _arr("w", C, C, 3, 3), _arr("b", C), _arr("out", N, C, H, W)
        if op == "deform_shared":
            return _status(lambda: ops.deformable_convolution_shared(x, _arr("fl", N, 2, H, W), 20.0, 8.0, w, b, out=out))
        return _status(lambda: ops.DeformableConvolution(x, _arr("off", N, 18, H, W), w, b, kernel=(3, 3), pad=(1, 1), num_filter=C, out=out))
    if op == "deform_shared_bwd":
        N, C, H, W, req = key[1:]
        return _dc_bwd_call(ns, (N, C, C, H, W, dict(k=3, pad=1)), [REQ[r] for r in req], True)[0]
    if op == "warp":
        N, C, H, W = key[1:]
        return _status(lambda: ops.warp(_arr("x", N, C, H, W), _arr("fl", N, 2, H, W), clip_grid=False, out=_arr("out", N, C, H, W)))
    if op == "upsample":
        N, C, H, W, f = key[1:]
        return _status(lambda: ops.Upsample(_arr("x", N, C, H, W), f, out=_arr("out", N, C, H * f, W * f)))
    if op == "offsets":
        N, H, W = key[1:]
        return _status(lambda: ops.offsets_from_flow(_arr("fl", N, 2, H, W), 20.0, 8.0, out=_arr("off", N, 18, H, W)))
    raise KeyError(op)


_SIG = {}


def signature(ops, key, arith):
    """'op | rc | name bx by bz lds; ... [| dc plan mt pt kw areg]' of the call under one arithmetic."""
    ck = (tuple(key), arith)
    if ck not in _SIG:
        emu_ops.set_tuning(corr_gram=arith, dc_mma=arith, conv_mma=arith)
        emu_ops.dry_launches()
        rc = _plan(ops, list(key))
        recs = emu_ops.dry_launches()
        sig = "%s | %d | %s" % (key[0], rc, "; ".join("%s %d %d %d %d" % (r[0], r[4], r[5], r[6], r[7]) for r in recs))
        if any(r[0] in DCM_KERNELS for r in recs):
            v = [ctypes.c_int(-1) for _ in range(4)]
            assert ops.ns.debug_last_dc_plan(*[ctypes.byref(x) for x in v]) == 0
            sig += " | dc plan %d %d %d %d" % tuple(x.value for x in v)
        _SIG[ck] = sig
    return _SIG[ck]


def kernels_of(sig):
    return [rec.split(" ")[0] for rec in sig.split(" | ")[2].split("; ") if rec]


@pytest.fixture
def dry_ops():
    ops = emu_ops.emu_ops()
    emu_ops.set_tuning(**DEFAULT_TUNING)
    emu_ops.dry_run(True)
    emu_ops.dry_launches()
    try:
        yield ops
    finally:
        emu_ops.dry_run(False)
        emu_ops.launch_log()
        emu_ops.set_tuning(**DEFAULT_TUNING)
        _bufs.clear()


# ---- what the existing `-m gpu` fp64 tests run ----------------------------------------------------------------------------------------
def _route_key(shape, kw):
    """A GPU_CONV_ROUTES row of tests/test_backward_fp64.py as a key, or None where its geometry is none of the network's."""
    kw = dict(kw)
    req = _req(kw.get("req", bwd64.WWW))
    if kw.get("transposed"):
        if kw.get("kernel") != (4, 4) or kw.get("pad", (1, 1)) != (1, 1) or not kw.get("bias", True):
            return None
        return ["deconv_bwd"] + list(shape) + [2, 1, int(bool(kw.get("leaky"))), req]
    d = kw.get("dilate", (1, 1))[0]
    if kw.get("pad", (1, 1))[0] != d or not kw.get("bias", True):
        return None
    return ["conv_bwd"] + list(shape) + [kw.get("stride", (1, 1))[0], d, int(bool(kw.get("leaky"))), req]


def bench_keys():
    """{key: name} of the calls the GPU halves of the two fp64 files make, both arithmetics each (the names say where)."""
    out = {}
    for cfg, pyr in fwd64.PYR.items():
        for level in (6, 5, 4, 3, 2):
            s = list(pyr[fwd64.LEVEL[level]])
            for md in (4, 2):
                out[tuple(["corr"] + s + [md])] = "test_gpu_correlation_plan %s level %d md=%d" % (cfg, level, md)
            if level != 6:
                out[tuple(["deform_dropin"] + s)] = "test_gpu_deform %s level %d" % (cfg, level)
            if level in (5, 3, 2):
                out[tuple(["deform_shared"] + s)] = "test_gpu_deform_flow_and_matching %s level %d" % (cfg, level)
            out[tuple(["corr_bwd"] + s + [4, "ww"])] = "test_gpu_correlation_backward %s level %d md=4" % (cfg, level)
            if level in (3, 2):
                out[tuple(["corr_bwd"] + s + [2, "ww"])] = "test_gpu_correlation_backward %s level %d md=2" % (cfg, level)
            if level in (4, 2):
                out[tuple(["deform_shared_bwd"] + s + ["wwww"])] = "test_gpu_deform_flow_backward %s level %d" % (cfg, level)
    for shape in ((8, 3, 384, 512), (4, 3, 448, 1024)):
        out[tuple(["warp"] + list(shape))] = "test_gpu_warp %s" % (shape,)
    for row in fwd64.GPU_CONV:
        N, Cin, Cout, H, W, geo, transposed = row[:7]
        rid = fwd64._conv_id(row)
        if transposed and not geo:
            for act in (0, 1):
                out[("deconv", N, Cin, Cout, H, W, 2, 1, act)] = "test_gpu_conv " + rid
        elif not transposed and geo.get("kernel", (3, 3)) == (3, 3) and geo.get("pad") == geo.get("dilate", (1, 1)):
            for act in (0, 1) if Cout > 3 else (0,):     # conv_runs: with and without the LeakyReLU; the heads have none
                out[("conv", N, Cin, Cout, H, W, geo.get("stride", (1, 1))[0], geo.get("dilate", (1, 1))[0], act)] = "test_gpu_conv " + rid
    for N, Cin, Cout, H, W, leaky, _ in bwd64.GPU_CONV:
        out[("conv_bwd", N, Cin, Cout, H, W, 1, 1, int(leaky), "www")] = "test_gpu_conv_backward %s" % "x".join(map(str, (N, Cin, Cout, H, W)))
    for name, (shape, kw, _, _, _) in bwd64.GPU_CONV_ROUTES.items():
        k = _route_key(shape, kw)
        if k is not None:
            out[tuple(k)] = "test_gpu_conv_backward_routes " + name
    return out


# ---- the witness of a signature ---------------------------------------------------------------------------------------------------------
def _hw_pos(key):
    return (4, 5) if key[0].startswith(("conv", "deconv")) else (2, 3) if key[0] == "offsets" else (3, 4)


def _with(key, N, H):
    k = list(key)
    k[1], k[_hw_pos(key)[0]] = N, H
    return k


def reduce_witness(ops, key, ariths, sigs):
    """The smallest (N, H) with H % 8 kept whose plan is `sigs` under every arithmetic of `ariths`; the channel counts and W stay."""
    N0, H0 = key[1], key[_hw_pos(key)[0]]
    best = None
    for N in range(1, N0 + 1):
        for H in range(H0 % 8 or 8, H0 + 1, 8):
            if best is not None and (N * H, N) >= best[0]:
                break
            if all(signature(ops, _with(key, N, H), a) == s for a, s in zip(ariths, sigs)):
                best = ((N * H, N), N, H)
                break
    assert best is not None, key
    return _with(key, best[1], best[2])


def ledger(ops):
    """{signature: dict(ariths, calls = the dataset calls that take it)} over every dataset key."""
    out = {}
    for key, tags in dataset_keys().items():
        for a in ARITHS:
            e = out.setdefault(signature(ops, key, a), dict(ariths=[], calls=[]))
            if a not in e["ariths"]:
                e["ariths"].append(a)
            e["calls"].append((key, a, tags))
    return out


def build_record(ops):
    bench = bench_keys()
    bench_sigs = {}
    for key, name in bench.items():
        for a in ARITHS:
            bench_sigs.setdefault(signature(ops, key, a), {})[a] = name
    rec = []
    for sig, e in sorted(ledger(ops).items()):
        ariths = sorted(e["ariths"])
        if all(a in bench_sigs.get(sig, {}) for a in ariths):
            key = next(k for k, n in bench.items() if n == bench_sigs[sig][ariths[0]])
            if all(signature(ops, key, a) == sig for a in ariths):
                rec.append(dict(signature=sig, ariths=ariths, bench=bench_sigs[sig][ariths[0]], key=list(key)))
                continue
        # the smallest dataset call taking it under every one of its arithmetics
        keys = sorted({k for k, a, _ in e["calls"]}, key=lambda k: (np.prod([v for v in k[1:] if isinstance(v, int)]), k))
        keys = [k for k in keys if all(signature(ops, k, a) == sig for a in ariths)]
        assert keys, "no single dataset call takes %s under all of %s" % (sig, ariths)
        r = dict(signature=sig, ariths=ariths, case=reduce_witness(ops, keys[0], ariths, [sig] * len(ariths)))
        if _wid(r) in EMU_LEFT_OUT:
            r["gpu_only"] = "the smallest shape that keeps the signature; its emulated run takes longer than about 20 s"
        rec.append(r)
    return rec


def _write(rec):
    with open(RECORD, "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rec) + "\n]\n")


def _read():
    with open(RECORD) as f:
        return json.load(f)


def test_the_enumeration_lists_every_layer_and_every_hot_path_call():
    assert ds.selfcheck()
    assert ds.selfcheck(2, 128, 192)
    names = [e.name for e in ds.entries()]
    assert len(names) == len(set(names)) and {e.stage for e in ds.entries()} == {"train", "predict"}
    assert all(e.N == 1 for e in ds.entries() if e.stage == "predict")


def test_ledger_every_dataset_plan_has_a_witness_that_takes_it(dry_ops):
    if os.environ.get("MFN_DATASET_PLANS") == "write":
        _write(build_record(dry_ops))
    rec = {r["signature"]: r for r in _read()}
    assert len(rec) == len(_read()), "a signature is recorded twice"
    led = ledger(dry_ops)
    orphans = ["%s under arithmetic %s:\n    %s" % (sig, sorted(set(e["ariths"]) - set(rec.get(sig, {}).get("ariths", []))),
                                                   "\n    ".join("%s  %s" % (list(k), ", ".join(t[:3])) for k, t in list({k: t for k, _, t in e["calls"]}.items())[:6]))
               for sig, e in sorted(led.items()) if sig not in rec or set(e["ariths"]) - set(rec[sig]["ariths"])]
    assert not orphans, "%d dataset plans have no witness:\n%s" % (len(orphans), "\n".join(orphans))
    stale = [sig for sig, r in rec.items() if sig not in led or set(r["ariths"]) - set(led[sig]["ariths"])]
    assert not stale, "%d recorded plans that no dataset call takes:\n%s" % (len(stale), "\n".join(stale))
    bench = bench_keys()
    for sig, r in rec.items():
        key = r["key"] if "bench" in r else r["case"]
        if "bench" in r:
            assert bench.get(tuple(key)) == r["bench"], "%s is not what %s runs" % (key, r["bench"])
        for a in r["ariths"]:
            got = signature(dry_ops, key, a)
            assert got == sig, "witness %s under arithmetic %d plans\n  %s\nrecorded for\n  %s" % (key, a, got, sig)


# ---- the witnesses against fp64 -----------------------------------------------------------------------------------------------------------
def _witnesses():
    return [r for r in _read() if "case" in r]


def _wid(r):
    return "-".join(str(v) for v in r["case"]) + "-a" + "".join("d" if a else "f" for a in r["ariths"])


KINDS = ("plain", "graded-pixel")
# case_conv_bwd takes the LeakyReLU's slope from the library's forward output and refuses a seed under which a pre-activation rounds
# across zero ("take another seed").  Seed 3, the routes' seed, puts one of conv2a's 143 360 at 1.9e-8 of its magnitude bound, below
# fp32's resolution (torch's own fp32 convolution flips that sign too): these two witnesses take seed 4.
SEEDS = {"conv_bwd-1-16-32-80-224-2-1-1-www-af": 4, "conv_bwd-1-16-32-80-224-2-1-1-www-ad": 4}
GKIND = {"plain": "plain", "graded-pixel": "graded"}
FULL_REQ = {"w": "write", "n": "null", "a": "add"}


def run_witness(env, r, kind):
    """The witness call through the fp64 case of its operator, under every arithmetic recorded for it, its launches asserted."""
    key, kernels = r["case"], kernels_of(r["signature"])
    op = key[0]
    for arith in r["ariths"]:
        if op == "corr":
            fwd64.case_corr(env, arith, tuple(key[1:5]), key[5], kind, kernels, forms=("plain", "leaky", "into") if kind != "plain" else ("plain", "leaky"))
        elif op == "corr_bwd":
            bwd64.case_corr_bwd(env, arith, tuple(key[1:5]), key[5], GKIND[kind], kernels=kernels, reqs=tuple(FULL_REQ[c] for c in key[6]))
        elif op in ("conv", "deconv"):
            N, Cin, Cout, H, W, stride, dilate, act = key[1:]
            geo = _conv_geo(op, stride, dilate)
            for leaky, bias in ((bool(act), "usual"),) if kind == "plain" else ((bool(act), "none"), (bool(act), "small")):
                fwd64.case_conv(env, arith, N, Cin, Cout, H, W, kind, kernels, leaky=leaky, bias=bias, transposed=op == "deconv", **geo)
        elif op in ("conv_bwd", "deconv_bwd"):
            N, Cin, Cout, H, W, stride, dilate, act, req = key[1:]
            geo = _conv_geo(op, stride, dilate)
            geo.setdefault("dilate", (1, 1))
            bwd64.case_conv_bwd(env, arith, N, Cin, Cout, H, W, GKIND[kind], leaky=bool(act), kernels=kernels, transposed=op == "deconv_bwd",
                                req=tuple(FULL_REQ[c] for c in req), seed=SEEDS.get(_wid(r), 3), **geo)
        elif op == "deform_dropin":
            fwd64.case_deform(env, arith, *key[1:], "smooth", kind, kernels, packed=True)
        elif op == "deform_shared":
            fwd64.case_deform_flow(env, arith, *key[1:], kind, kernels)
        elif op == "deform_shared_bwd":
            bwd64.case_deform_flow_bwd(env, arith, *key[1:5], GKIND[kind], kernels=kernels, req=tuple(FULL_REQ[c] for c in key[5]))
        elif op == "warp":
            fwd64.case_warp(env, tuple(key[1:]), False, kind)
        elif op == "upsample":      # bit-identical to the fp32 oracle: the same products in the same order
            with env.launches() as L:
                pc.case_upsample(env.ops, oracle, env.dev, env.host, tuple(key[1:5]), key[5])
            L.expect(kernels, what=str(key))
        elif op == "offsets":       # one multiplication and one division: the oracle's bits
            N, H, W = key[1:]
            fl = pc.flow_field(np.random.default_rng(5), N, H, W)
            with env.launches() as L:
                got = env.host(env.ops.offsets_from_flow(env.dev(fl), 20.0, 8.0))
            L.expect(kernels, what=str(key))
            np.testing.assert_array_equal(got, oracle.offsets_from_flow(fl, 20.0, 8.0))
        else:
            raise KeyError(op)


@pytest.fixture(scope="module")
def gpu():
    return Env(emu=False)


@pytest.fixture
def _gpu_defaults(gpu):
    yield
    from maskflownet_amd import _lib
    _lib.set_arithmetic(all=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r", _witnesses(), ids=_wid)
def test_gpu_witness(gpu, _gpu_defaults, r, kind):
    n = len(bwd64._RESULTS)
    run_witness(gpu, r, kind)
    for what, arith, e_lib, e_ref in bwd64._RESULTS[n:]:     # the forward cases print theirs themselves
        print("%-96s arith %-7s max e_lib %.3e   max e_ref32 %.3e" % (what, {0: "fp32", -1: "default", None: "-"}[arith], e_lib, e_ref))


# Witnesses whose emulated run takes longer than about 20 s here: they run on the GPU only, and the ledger test covers their plans on the
# CPU.  Seconds of one graded-pixel run of run_witness on the emulation, under every arithmetic of the witness, its oracle included, alone
# on the eight cores (three, above 60 s, on two cores of their own: the emulator keeps a process on one core, so that costs the oracle only).
EMU_LEFT_OUT = {
    "deform_shared_bwd-1-128-2-24-nwww-adf": 20.4,
    "conv_bwd-1-16-32-80-224-2-1-1-www-af": 20.6,
    "corr-1-64-32-96-4-ad": 21.7,
    "deform_shared_bwd-1-64-8-56-nwww-adf": 23.2,
    "deform_dropin-1-196-5-7-adf": 24.4,
    "corr-1-128-34-80-2-ad": 29.4,
    "conv_bwd-1-404-64-5-12-1-1-1-www-af": 29.4,
    "conv_bwd-1-404-64-5-12-1-1-1-www-ad": 30.6,
    "corr-1-128-34-80-4-ad": 32.6,
    "conv_bwd-1-308-96-5-12-1-1-1-www-ad": 34.6,
    "deform_shared-1-196-5-7-adf": 35.3,
    "conv_bwd-1-308-96-5-12-1-1-1-www-af": 38.4,
    "conv_bwd-2-64-64-40-56-1-1-1-www-ad": 51.1,
    "conv_bwd-8-16-96-20-28-1-1-0-www-ad": 53.5,
    "conv_bwd-2-32-64-80-112-2-1-1-www-ad": 56.9,
    "conv-1-16-32-56-640-1-1-0-af": 62.6,
    "conv_bwd-2-16-32-80-224-1-1-0-www-ad": 63.6,
    "conv_bwd-2-32-64-80-112-2-1-1-www-af": 71.4,
    "conv_bwd-2-16-32-80-224-1-1-0-www-af": 71.9,
    "conv-1-32-2-56-640-1-1-0-ad": 76.7,
}
# The largest witnesses take minutes each on the emulation: their runs, on two cores of their own, were ended unfinished after this long.
EMU_UNFINISHED_AFTER = {
    "conv-1-16-64-104-320-1-1-0-af": 75.0,
    "conv-2-358-96-80-224-1-1-1-af": 75.0,
    "conv-2-64-64-48-128-1-1-1-ad": 75.0,
    "conv-2-96-96-44-160-1-1-1-ad": 75.0,
    "conv-8-32-64-80-224-2-1-1-af": 75.0,
    "conv_bwd-1-16-16-152-224-1-1-1-www-ad": 75.0,
    "conv_bwd-1-16-16-152-224-1-1-1-www-af": 75.0,
    "conv_bwd-1-518-32-64-192-1-1-1-www-ad": 75.0,
    "conv_bwd-1-550-2-56-112-1-1-0-www-af": 75.0,
    "conv_bwd-1-550-2-64-192-1-1-0-www-ad": 75.0,
    "conv_bwd-15-64-64-40-56-1-1-1-www-ad": 75.0,
    "conv_bwd-2-16-32-152-448-2-1-1-www-af": 75.0,
    "conv_bwd-2-550-32-32-96-1-1-1-www-af": 75.0,
    "conv_bwd-2-64-32-80-224-1-1-1-www-af": 75.0,
    "conv_bwd-4-64-64-32-96-1-1-1-www-ad": 75.0,
    "conv_bwd-7-134-128-32-56-1-1-1-www-ad": 75.0,
    "conv_bwd-7-582-2-32-56-1-1-0-www-ad": 75.0,
    "conv_bwd-7-64-64-32-56-1-1-1-www-ad": 75.0,
    "conv_bwd-8-16-96-20-28-1-1-0-www-af": 75.0,
    "conv_bwd-8-166-128-20-28-1-1-1-www-ad": 75.0,
    "conv_bwd-8-166-128-20-28-1-1-1-www-af": 75.0,
    "conv_bwd-8-518-64-20-28-1-1-1-www-ad": 75.0,
    "conv_bwd-8-518-64-20-28-1-1-1-www-af": 75.0,
    "conv_bwd-8-582-32-20-28-1-1-1-www-ad": 75.0,
    "conv_bwd-8-582-32-20-28-1-1-1-www-af": 75.0,
    "conv_bwd-8-614-2-20-28-1-1-0-www-ad": 75.0,
    "conv_bwd-8-614-2-20-28-1-1-0-www-af": 75.0,
    "conv_bwd-8-643-1-20-28-1-1-0-www-af": 75.0,
    "conv_bwd-8-96-96-20-28-1-1-1-www-ad": 75.0,
    "conv_bwd-8-96-96-20-28-1-1-1-www-af": 75.0,
    "deconv-1-582-16-104-320-2-1-1-af": 75.0,
    "deconv_bwd-1-614-16-20-56-2-1-1-www-ad": 75.0,
    "deconv_bwd-1-614-16-20-56-2-1-1-www-af": 75.0,
    "deconv_bwd-4-582-16-32-96-2-1-1-www-ad": 75.0,
    "deconv_bwd-8-643-16-20-28-2-1-1-www-af": 75.0,
    "deform_dropin-3-196-5-12-adf": 75.0,
    "deform_shared-3-196-5-12-adf": 75.0,
}
EMU_LEFT_OUT.update(EMU_UNFINISHED_AFTER)


@pytest.fixture(scope="module")
def emu():
    return Env(emu=True)


@pytest.fixture
def _emu_defaults(emu):
    yield
    emu_ops.set_tuning(corr_gram=-1, dc_mma=-1, conv_mma=-1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("r", [r for r in _witnesses() if _wid(r) not in EMU_LEFT_OUT], ids=_wid)
def test_emu_witness(emu, _emu_defaults, r, kind):
    run_witness(emu, r, kind)


def test_the_record_says_which_witnesses_run_on_the_gpu_only():
    assert set(EMU_LEFT_OUT) == {_wid(r) for r in _witnesses() if "gpu_only" in r}
    assert all(t > 20.0 for t in EMU_LEFT_OUT.values()) and all(t >= 60.0 for t in EMU_UNFINISHED_AFTER.values())
