"""Which kernel a call dispatches to, with what launch geometry, against a record (tests/data/dispatch_v1.json).

The CPU emulation compiles the product's own argument checking and planning code (maskflownet_amd/csrc/api_impl.inc).  In its dry-run
mode a launch is recorded (name, grid, block, dynamic shared bytes) and no kernel body runs, so the plans of the bench-size levels,
which the emulation cannot execute in reasonable time, are pinned here on the CPU: per call the return code, the workspace / packed
bytes the size queries answer, and the list of launches.

The record is data, taken from the code BEFORE a change to the plans and compared entry for entry afterwards.  When a pull request
changes a plan on purpose, rebuild it with

    MFN_DISPATCH_RECORD=write python -m pytest tests/test_dispatch_table.py -q

and review the diff of the JSON file like code.  corr.variant values that name no kernel (40..43, 47) are not in the record: they
are asserted separately (the library chooses, as tuning.h promises for every value a key does not list)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests.emu import emu_ops
from tests.test_emu_parity import DCM_TILINGS, DEFAULT_TUNING
from tests.test_gpu_parity import CFG2, CFG3, CONV_LAYERS, DEFORM_LEVELS

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "dispatch_v1.json")
RECORD_BWD = os.path.join(os.path.dirname(RECORD), "dispatch_bwd_v1.json")   # the backward entry points, same format

# shapes the emulation tests run (tests/test_emu_parity.py), every kernel family among them
SMALL = [(1, 6, 10, 20), (1, 6, 10, 72), (1, 20, 6, 40), (1, 48, 5, 32), (1, 32, 10, 24), (2, 32, 13, 20), (1, 32, 16, 16),
         (1, 64, 9, 24), (2, 196, 6, 8), (1, 96, 5, 16), (1, 64, 4, 24), (1, 12, 6, 40), (1, 9, 18, 20), (2, 5, 9, 28), (2, 7, 6, 64),
         (4, 4, 32, 16), (2, 32, 7, 16), (1, 37, 12, 16), (1, 16, 24, 32), (2, 30, 6, 8), (1, 200, 3, 4), (1, 5, 12, 16), (2, 5, 6, 8)]
CORR_TUNINGS = ([{}] + [{"corr_variant": v} for v in (6, 16, 20, 22, 26, 31, 44, 45, 46, 48)] + [{"corr_form": v} for v in (16, 20, 46, 48)]
                + [{"corr_direct": v} for v in (0, 1, 2)] + [{"corr_rows": v} for v in (0, 6, 8)] + [{"path_generic": 1}])
UNLISTED_VARIANTS = (40, 41, 42, 43, 47)
# the facts only a run knows, on shapes whose plan has channel slices, a direct kernel, a Gram band, a coarse-level band
FACT_SHAPES = [(8, 196, 6, 8), (8, 128, 12, 16), (8, 32, 96, 128), (4, 64, 56, 128), (2, 32, 7, 16), (2, 30, 6, 8), (1, 6, 10, 72)]
FACT_TUNINGS = [{}, {"corr_direct": 2}, {"corr_direct": 1}, {"corr_variant": 6}, {"corr_variant": 16}]
FACTS = ("no_ws", "ws_short", "d1+4", "d2+4", "out+4", "nstride+2")

DC_TUNINGS = ([{}] + [{"dc_pt": pt, "dc_ksb": ksb} for pt, ksb in ((1, 1), (4, 1), (2, 1), (2, 2), (1, 2), (1, 0))]
              + [{"dc_ksb": 2}, {"dc_nw": 8, "dc_pt": 1}, {"dc_off": 1}, {"dc_off": 2}, {"dc_pt": 4}, {"path_generic": 2}]
              + [{"dc_mt": mt, "dc_pt": pt, "dc_nw": nw} for mt, pt, nw, _ in DCM_TILINGS])
CONV_TUNINGS = ([{}] + [{"conv_mt": mt, "conv_pt": pt} for mt, pt in ((1, 4), (2, 4), (3, 4), (4, 4), (1, 1), (2, 1))]
                + [{"conv_pt": 1}, {"conv_pt": 4}, {"conv_dcm": 1}, {"conv_dcm": 2}, {"path_generic": 4}])


def _name(tune):
    return ",".join("%s=%d" % kv for kv in sorted(tune.items())) or "default"


def _status(call):
    """Return code of an OpSet call (its check raises on a non-zero status)."""
    try:
        call()
        return 0
    except RuntimeError as e:
        return int(re.match(r"mfn_emu status (-?\d+)", str(e)).group(1))


_bufs = {}


def _buf(tag, n):
    """n + 8 uninitialised floats, 64-byte aligned (no kernel body runs in a dry run); one buffer per tag, grown on demand."""
    b = _bufs.get(tag)
    if b is None or b.size < n + 24:
        b = _bufs[tag] = np.empty(n + 24, np.float32)
    return b[(-b.ctypes.data % 64) // 4:]


def _corr_call(ns, shape, md, fact=None, kernel=1, s1=1, s2=1, pad=None):
    N, C, H, W = shape
    pad = md if pad is None else pad
    geo = (md, kernel, s1, s2, pad, 1)
    tc, th, tw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = ns.correlation_out_shape(H, W, md, kernel, s1, s2, pad, ctypes.byref(tc), ctypes.byref(th), ctypes.byref(tw))
    if rc:
        return [rc, 0]
    img = tc.value * th.value * tw.value
    need = ns.correlation_workspace_bytes(N, C, H, W, *geo)
    d1, d2, out, ws = _buf("d1", N * C * H * W), _buf("d2", N * C * H * W), _buf("out", N * (img + 2)), _buf("ws", need // 4)
    off = lambda a, name: a.ctypes.data + (4 if fact == name + "+4" else 0)
    ws_ptr, ws_bytes = (ws.ctypes.data, need) if need else (None, 0)
    if fact == "no_ws":
        ws_ptr, ws_bytes = None, 0
    if fact == "ws_short" and need:
        ws_bytes = need - 1
    nstride = img + 2 if fact == "nstride+2" else 0
    rc = ns.correlation_fwd_into(off(d1, "d1"), off(d2, "d2"), off(out, "out"), nstride, N, C, H, W, *geo, 0, ws_ptr, ws_bytes, None)
    return [rc, need]


def _dc_call(ops, N, C, H, W, stride, fused):
    dims = (N, C, H, W, C, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
    x, w, b = _buf("x", N * C * H * W)[:N * C * H * W].reshape(N, C, H, W), _buf("w", C * C * 9)[:C * C * 9].reshape(C, C, 3, 3), _buf("b", C)[:C]
    if fused:
        fl = _buf("fl", N * 2 * H * W)[:N * 2 * H * W].reshape(N, 2, H, W)
        rc = _status(lambda: ops.deformable_convolution_shared(x, fl, 20.0, stride, w, b))
    else:
        off = _buf("off", N * 18 * H * W)[:N * 18 * H * W].reshape(N, 18, H, W)
        rc = _status(lambda: ops.DeformableConvolution(x, off, w, b, kernel=(3, 3), pad=(1, 1), num_filter=C))
    return [rc, ops.ns.deform_conv_workspace_bytes(*dims), ops.ns.deform_conv_packed_weight_bytes(*dims)]


def _conv_call(ops, N, Cin, Cout, H, W, kw):
    (sh, sw), (ph, pw), (dh, dw) = kw.get("stride", (1, 1)), kw.get("pad", (0, 0)), kw.get("dilate", (1, 1))
    dims = (N, Cin, H, W, Cout, 3, 3, sh, sw, ph, pw, dh, dw, 1, 0)
    x, w, b = _buf("x", N * Cin * H * W)[:N * Cin * H * W].reshape(N, Cin, H, W), _buf("w", Cout * Cin * 9)[:Cout * Cin * 9].reshape(Cout, Cin, 3, 3), _buf("b", Cout)[:Cout]
    rc = _status(lambda: ops.Convolution(x, w, b, num_filter=Cout, activation="leaky", **kw))
    return [rc, ops.ns.conv2d_workspace_bytes(*dims), ops.ns.conv2d_packed_weight_bytes(*dims)]


def _with_launches(entry):
    return entry + [";".join(" ".join(str(v) for v in rec) for rec in emu_ops.dry_launches())]


def _entries(ops, corr_tunings=CORR_TUNINGS):
    """(kind, settings, case, [rc, bytes.., launches]) of every call of the record, in a fixed order."""
    ns = ops.ns
    levels = [(s, md) for md in (4, 2) for s in CFG2 + CFG3 + SMALL]
    for arith in (-1, 0, 1):
        for tune in corr_tunings:
            emu_ops.set_tuning(**dict(DEFAULT_TUNING, corr_gram=arith, **tune))
            head = "corr", "arith=%d %s" % (arith, _name(tune))
            for shape, md in levels:
                yield head + ("%s md=%d" % (shape, md), _with_launches(_corr_call(ns, shape, md)))
            yield head + ("(1, 3, 5, 7) md=4 odd width", _with_launches(_corr_call(ns, (1, 3, 5, 7), 4)))
            yield head + ("(2, 8, 20, 30) md=2 W%4", _with_launches(_corr_call(ns, (2, 8, 20, 30), 2)))
            yield head + ("(2, 3, 9, 10) kernel=3 s1=2", _with_launches(_corr_call(ns, (2, 3, 9, 10), 2, kernel=3, s1=2, pad=3)))
            yield head + ("(8, 32, 96, 128) kernel=3 s1=2", _with_launches(_corr_call(ns, (8, 32, 96, 128), 4, kernel=3, s1=2, pad=5)))
            yield head + ("(2, 3, 9, 10) s2=2", _with_launches(_corr_call(ns, (2, 3, 9, 10), 4, s2=2)))
    if corr_tunings is not CORR_TUNINGS:
        return
    for arith in (-1, 0):
        for tune in FACT_TUNINGS:
            emu_ops.set_tuning(**dict(DEFAULT_TUNING, corr_gram=arith, **tune))
            for shape in FACT_SHAPES:
                for fact in FACTS:
                    yield "corr run facts", "arith=%d %s" % (arith, _name(tune)), "%s md=4 %s" % (shape, fact), _with_launches(_corr_call(ns, shape, 4, fact))
    for arith in (-1, 0):
        for tune in DC_TUNINGS:
            emu_ops.set_tuning(**dict(DEFAULT_TUNING, dc_mma=arith, **tune))
            for C, H, W, stride in DEFORM_LEVELS:
                for N, fused in ((2, True), (2, False), (8, True), (8, False)):
                    yield ("dc", "arith=%d %s" % (arith, _name(tune)), "N=%d C=%d %dx%d fused=%d" % (N, C, H, W, fused),
                           _with_launches(_dc_call(ops, N, C, H, W, stride, fused)))
        for tune in CONV_TUNINGS:
            emu_ops.set_tuning(**dict(DEFAULT_TUNING, conv_mma=arith, **tune))
            for N, Cin, Cout, H, W, kw in CONV_LAYERS:
                yield ("conv", "arith=%d %s" % (arith, _name(tune)), "N=%d %d->%d %dx%d %s" % (N, Cin, Cout, H, W, _name({k: v[0] for k, v in kw.items()})),
                       _with_launches(_conv_call(ops, N, Cin, Cout, H, W, kw)))


# ---- the backward entry points (tests/data/dispatch_bwd_v1.json) ----
W_, A_, N_ = 1, 3, 0   # MFN_REQ_WRITE / _ADD / _NULL
CORR_BWD_TUNINGS = [{}, {"bwd_off": 4}]
CORR_BWD_REQS = [(W_, W_), (W_, N_), (N_, A_)]
DC_BWD_TUNINGS = [{}, {"bwd_off": 1}, {"bwd_off": 2}, {"bwd_off": 3}, {"path_generic": 2}]
# (x, offset / flow, w, bias): all write, all add, weights only (the conv2d_bwd use), input + offset only, bias without weights
DC_BWD_REQS = [(W_, W_, W_, W_), (A_, A_, A_, A_), (N_, N_, W_, N_), (W_, W_, N_, N_), (W_, W_, N_, W_), (N_, N_, N_, W_)]
_K3 = dict(k=3, pad=1)
# (N, Cin, Cout, H, W, geometry): the network's levels at N = 2 and 8, the shapes tests/test_emu_parity.py runs the backward on, and
# one shape per remaining branch (ragged channel blocks, W % 4, Cin % 4, more than 96 filters, stride 2, groups 2, a 5x5 kernel)
DC_BWD_SHAPES = ([(N, C, C, H, W, _K3) for N in (2, 8) for C, H, W, _ in DEFORM_LEVELS]
                 + [(2, 4, 6, 6, 7, g) for g in (_K3, dict(k=3, pad=1, stride=2), dict(k=3, pad=2, dilate=2), dict(k=3, pad=1, groups=2),
                                                 dict(k=3, pad=1, dg=2), dict(k=1, pad=0))]
                 + [(N, Ci, Co, H, W, _K3) for N, Ci, Co, H, W in
                    [(1, 36, 34, 5, 18), (2, 5, 70, 3, 9), (1, 34, 4, 7, 19), (1, 4, 4, 11, 19), (1, 4, 4, 11, 20), (1, 36, 36, 9, 16),
                     (1, 20, 40, 9, 16), (1, 8, 8, 9, 16), (2, 8, 8, 13, 28), (1, 36, 40, 5, 16), (1, 8, 100, 5, 8), (1, 4, 4, 4, 16),
                     (1, 2, 4, 9, 17), (1, 4, 4, 5, 16), (1, 4, 4, 4, 8), (1, 4, 20, 5, 8), (1, 36, 4, 4, 8), (1, 4, 4, 5, 8), (0, 4, 4, 5, 8)]]
                 + [(1, 4, 6, 4, 5, dict(k=3, pad=2, dilate=2)), (1, 4, 4, 6, 8, dict(k=5, pad=2)), (2, 8, 8, 8, 16, dict(k=3, pad=1, stride=2))])
DC_BWD_FACT_SHAPES = [s for s in DC_BWD_SHAPES if s[0] == 8] + [(1, 4, 20, 5, 8, _K3), (1, 36, 40, 5, 16, _K3)]
DC_BWD_FACTS = ("no_ws", "ws_short", "ws+4", "x+4", "w+4")
CONV_BWD_TUNINGS = [{}, {"path_generic": 4}, {"conv_dcm": 1}]
# CONV_LAYERS, then: the network's transposed convolution, two transposed layers that are not that shape, strided convolutions whose
# data gradient has adj 0 / 1 / mixed
CONV_BWD_LAYERS = ([(N, Ci, Co, H, W, dict(kw, k=3)) for N, Ci, Co, H, W, kw in CONV_LAYERS]
                   + [(2, 32, 16, 12, 16, dict(k=4, stride=(2, 2), pad=(1, 1), transposed=1)),
                      (1, 16, 8, 12, 16, dict(k=3, stride=(2, 2), pad=(1, 1), transposed=1, adj=(1, 1))),
                      (1, 16, 8, 6, 8, dict(k=4, stride=(2, 2), transposed=1)),
                      (1, 8, 16, 13, 17, dict(k=3, stride=(2, 2), pad=(1, 1))), (1, 8, 16, 14, 18, dict(k=3, stride=(2, 2), pad=(1, 1))),
                      (1, 8, 16, 13, 18, dict(k=3, stride=(2, 2), pad=(1, 1)))])


def _ptr(a, shift=False):
    return a.ctypes.data + (4 if shift else 0)


def _corr_bwd_call(ns, shape, md, req, fact=None, kernel=1, s1=1, s2=1, pad=None):
    N, C, H, W = shape
    pad = md if pad is None else pad
    tc, th, tw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = ns.correlation_out_shape(H, W, md, kernel, s1, s2, pad, ctypes.byref(tc), ctypes.byref(th), ctypes.byref(tw))
    if rc:
        return [rc]
    n_in = N * C * H * W
    go, d1, d2, g1, g2 = _buf("go", N * tc.value * th.value * tw.value), _buf("d1", n_in), _buf("d2", n_in), _buf("g1", n_in), _buf("g2", n_in)
    return [ns.correlation_bwd(_ptr(go), _ptr(d1), _ptr(d2), _ptr(g1, fact == "g1+4") if req[0] else None, _ptr(g2) if req[1] else None,
                               N, C, H, W, md, kernel, s1, s2, pad, 1, req[0], req[1], None)]


def _dc_bwd_call(ns, shape, req, shared, fact=None):
    """mfn_deform_conv_bwd, or mfn_deform_conv_shared_bwd with the same tensors (the flow in place of the offsets)."""
    N, Cin, Cout, H, W, g = shape
    k, pad, stride, dil, groups, dg = g["k"], g["pad"], g.get("stride", 1), g.get("dilate", 1), g.get("groups", 1), g.get("dg", 1)
    Ho, Wo = ((v + 2 * pad - (dil * (k - 1) + 1)) // stride + 1 for v in (H, W))
    geo = (k, k, pad, pad, dil, dil, groups) if shared else (k, k, stride, stride, pad, pad, dil, dil, groups, dg)
    query = ns.deform_conv_shared_bwd_workspace_bytes if shared else ns.deform_conv_bwd_workspace_bytes
    need = query(N, Cin, H, W, Cout, *geo)
    n_x, n_off, n_w = N * Cin * H * W, N * 2 * k * k * dg * Ho * Wo, Cout * (Cin // groups) * k * k
    go, x, off, w, ws = _buf("go", N * Cout * Ho * Wo), _buf("x", n_x), _buf("off", n_off), _buf("w", n_w), _buf("ws", need // 4)
    gx, goff, gw, gb = _buf("gx", n_x), _buf("goff", n_off), _buf("gw", n_w), _buf("gb", Cout)
    ws_ptr, ws_bytes = (_ptr(ws, fact == "ws+4"), need) if need else (None, 0)
    if fact == "no_ws":
        ws_ptr, ws_bytes = None, 0
    if fact == "ws_short" and need:
        ws_bytes = need - 1
    grads = [_ptr(a) if r else None for a, r in zip((gx, goff, gw, gb), req)]
    head = (_ptr(go), _ptr(x, fact == "x+4"), _ptr(off)) + ((20.0, 4.0) if shared else ()) + (_ptr(w, fact == "w+4"),)
    fn = ns.deform_conv_shared_bwd if shared else ns.deform_conv_bwd
    return [fn(*head, *grads, N, Cin, H, W, Cout, *geo, *req, ws_ptr, ws_bytes, None), need]


def _conv_bwd_call(ns, layer, act, req, fact=None):
    N, Cin, Cout, H, W, kw = layer
    k, (sh, sw), (ph, pw), (dh, dw) = kw["k"], kw.get("stride", (1, 1)), kw.get("pad", (0, 0)), kw.get("dilate", (1, 1))
    tr, (ah, aw) = kw.get("transposed", 0), kw.get("adj", (0, 0))
    geo = (k, k, sh, sw, ph, pw, dh, dw, 1, tr, ah, aw, act)
    ho, wo = ctypes.c_int(), ctypes.c_int()
    rc = ns.conv2d_out_shape(H, W, *geo[:8], tr, ah, aw, ctypes.byref(ho), ctypes.byref(wo))
    if rc:
        return [rc, 0]
    need = ns.conv2d_bwd_workspace_bytes(N, Cin, H, W, Cout, *geo)
    n_x, n_y, n_w = N * Cin * H * W, N * Cout * ho.value * wo.value, Cout * Cin * k * k
    go, x, w, y, ws = _buf("go", n_y), _buf("x", n_x), _buf("w", n_w), _buf("y", n_y), _buf("ws", need // 4)
    gx, gw, gb = _buf("gx", n_x), _buf("gw", n_w), _buf("gb", Cout)
    grads = [_ptr(a) if r else None for a, r in zip((gx, gw, gb), req)]
    return [ns.conv2d_bwd(_ptr(go), _ptr(x, fact == "x+4"), _ptr(w), _ptr(y) if act else None, *grads, N, Cin, H, W, Cout, *geo, *req,
                          _ptr(ws), need, None), need]


def _geo_name(g):
    return _name({k: (v if isinstance(v, int) else v[0]) for k, v in g.items()})


def _bwd_entries(ns):
    """As _entries, for the backward calls."""
    req_name = lambda req: "req=" + "".join("nw.a"[r] for r in req)
    levels = [(s, md) for md in (4, 2) for s in CFG2 + CFG3 + SMALL]
    for tune in CORR_BWD_TUNINGS:
        emu_ops.set_tuning(**dict(DEFAULT_TUNING, **tune))
        call = lambda *a, **kw: _with_launches(_corr_bwd_call(ns, *a, **kw))
        for req in CORR_BWD_REQS:
            head = "corr_bwd", "%s %s" % (_name(tune), req_name(req))
            for shape, md in levels:
                yield head + ("%s md=%d" % (shape, md), call(shape, md, req))
            yield head + ("(8, 32, 96, 128) md=4 g1+4", call((8, 32, 96, 128), 4, req, "g1+4"))
            yield head + ("(2, 30, 6, 8) md=2 g1+4", call((2, 30, 6, 8), 2, req, "g1+4"))
            yield head + ("(2, 8, 20, 30) md=2 W%4", call((2, 8, 20, 30), 2, req))
            yield head + ("(2, 3, 9, 10) kernel=3 s1=2", call((2, 3, 9, 10), 2, req, kernel=3, s1=2, pad=3))
            yield head + ("(2, 3, 9, 10) s2=2", call((2, 3, 9, 10), 4, req, s2=2))
    shape_name = lambda s: "N=%d %d->%d %dx%d %s" % (s[:5] + (_geo_name(s[5]),))
    fused_ok = lambda s: s[5].get("stride", 1) == 1 and s[5].get("dg", 1) == 1   # the flow-shared call has neither parameter
    for tune in DC_BWD_TUNINGS:
        emu_ops.set_tuning(**dict(DEFAULT_TUNING, **tune))
        for shared in (False, True):
            for req in DC_BWD_REQS:
                head = "dc_shared_bwd" if shared else "dc_bwd", "%s %s" % (_name(tune), req_name(req))
                for shape in DC_BWD_SHAPES:
                    if not shared or fused_ok(shape):
                        yield head + (shape_name(shape), _with_launches(_dc_bwd_call(ns, shape, req, shared)))
            for req in DC_BWD_REQS[:2]:
                head = "dc_shared_bwd run facts" if shared else "dc_bwd run facts", "%s %s" % (_name(tune), req_name(req))
                for shape in DC_BWD_FACT_SHAPES:
                    for fact in DC_BWD_FACTS:
                        yield head + ("%s %s" % (shape_name(shape), fact), _with_launches(_dc_bwd_call(ns, shape, req, shared, fact)))
    for arith in (-1, 0):
        for tune in CONV_BWD_TUNINGS:
            emu_ops.set_tuning(**dict(DEFAULT_TUNING, conv_mma=arith, **tune))
            for act in (0, 1):
                for req in ((W_, W_, W_), (A_, W_, W_), (N_, W_, W_)):
                    head = "conv_bwd", "arith=%d %s act=%d %s" % (arith, _name(tune), act, req_name(req))
                    for layer in CONV_BWD_LAYERS:
                        yield head + (shape_name(layer), _with_launches(_conv_bwd_call(ns, layer, act, req)))
                    for layer in CONV_BWD_LAYERS[:9]:   # x at +4: from conv_wgrad to the deformable weight gradient
                        yield head + (shape_name(layer) + " x+4", _with_launches(_conv_bwd_call(ns, layer, act, req, "x+4")))


def _flat(entries):
    return {"%s %s %s" % (kind, settings, case): value for kind, settings, case, value in entries}


def _write_record(entries, path=RECORD):
    """The record holds every distinct outcome once; a row per (kind, settings) indexes into them, one index per case of that kind."""
    outcomes, cases, rows = [], {}, []
    for kind, settings, case, value in entries:
        if not rows or rows[-1][:2] != [kind, settings]:
            rows.append([kind, settings, []])
        if len(rows[-1][2]) == len(cases.setdefault(kind, [])):
            cases[kind].append(case)
        assert cases[kind][len(rows[-1][2])] == case
        if value not in outcomes:
            outcomes.append(value)
        rows[-1][2].append(outcomes.index(value))
    lines = lambda items: "[\n" + ",\n".join("  " + json.dumps(i) for i in items) + "\n ]"
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write('{"cases": {\n%s\n },\n "outcomes": %s,\n "rows": %s}\n'
                % (",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in cases.items()), lines(outcomes), lines(rows)))


def _read_record(path=RECORD):
    with open(path) as f:
        rec = json.load(f)
    return {"%s %s %s" % (kind, settings, case): rec["outcomes"][i]
            for kind, settings, idx in rec["rows"] for case, i in zip(rec["cases"][kind], idx, strict=True)}


@pytest.fixture()
def dry_ops():
    ops = emu_ops.emu_ops()
    emu_ops.dry_run(True)
    emu_ops.dry_launches()
    try:
        yield ops
    finally:
        emu_ops.dry_run(False)
        emu_ops.launch_log()
        emu_ops.set_tuning(**DEFAULT_TUNING)
        _bufs.clear()


def _check_record(entries, path):
    if os.environ.get("MFN_DISPATCH_RECORD") == "write":
        _write_record(entries, path)
    got, want = _flat(entries), _read_record(path)
    assert len(got) == len(entries)
    assert list(got) == list(want)
    diff = ["%s: recorded %s, got %s" % (k, want[k], got[k]) for k in want if got[k] != want[k]]
    assert not diff, "%d of %d entries differ:\n%s" % (len(diff), len(want), "\n".join(diff[:40]))
    assert sum(1 for v in want.values() if v[-1]) > len(want) * 9 // 10   # a record of launches, not of refusals


def test_dispatch_matches_the_record(dry_ops):
    _check_record(list(_entries(dry_ops)), RECORD)


def test_backward_dispatch_matches_the_record(dry_ops):
    """The backward entry points: correlation_bwd, deform_conv_bwd, deform_conv_shared_bwd, conv2d_bwd (tests/data/dispatch_bwd_v1.json)."""
    _check_record(list(_bwd_entries(dry_ops.ns)), RECORD_BWD)


def test_unlisted_corr_variants_leave_the_choice_to_the_library(dry_ops):
    """corr.variant = 40 / 41 / 42 / 43 / 47 name kernels that are gone: every call is planned as with corr.variant = -1."""
    default = _flat(_entries(dry_ops, [{}]))
    assert any("corr_gram_v48 " in v[-1] for v in default.values()) and any("corr_gramk " in v[-1] for v in default.values())
    for variant in UNLISTED_VARIANTS:
        tune = {"corr_variant": variant}
        got = _flat(_entries(dry_ops, [tune]))
        assert {k.replace(_name(tune), "default"): v for k, v in got.items()} == default, variant


def test_tall_image_leaves_the_gram_kernel_only_beyond_its_block_range(dry_ops):
    """(1, 32, 400000, 8) under corr.variant = 48: 8-row items make 50 000 blocks, inside the range of the Gram-band kernel's magic
    divisions, and it runs; corr.rows = 6 makes 66 667, beyond it (corr_gram_range_ok), and the plan falls back to the tiled kernel --
    which is also its own choice at this shape.  tests/test_gpu_parity.py runs the three calls."""
    got = {}
    for name, tune in (("rows8", dict(corr_variant=48)), ("rows6", dict(corr_variant=48, corr_rows=6)), ("plan", {})):
        emu_ops.set_tuning(**dict(DEFAULT_TUNING, **tune))
        assert _corr_call(dry_ops.ns, (1, 32, 400000, 8), 4)[0] == 0
        got[name] = [(r[0], r[1]) for r in emu_ops.dry_launches()]
    assert got["rows8"] == [("corr_gram_v48", 50000)]
    assert got["rows6"] == got["plan"] == [("corr_tiled_v6", 12500)]
