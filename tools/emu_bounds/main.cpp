// emu_bounds -- the kernel sources on the CPU emulation (tests/emu/emu_api.cpp) under AddressSanitizer / UBSan, called through the
// mfn_emu_* entries with every buffer a heap block of exactly its tensor or queried size.  A stand-alone program: nothing is loaded into
// Python, nothing is preloaded, no GPU is involved.  tests/test_memory_contract.py sees writes next to a buffer and reads that reach a
// result; here the sanitizer sees every access outside a block at any distance, discarded over-reads and the emulated LDS included.
// The list is one call per kernel family and route of that test, driven by the tables below; built and run by tools/emu_bounds.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define mfn_last_error mfn_emu_last_error
#define mfn_set_tuning mfn_emu_set_tuning
#define mfn_set_arithmetic mfn_emu_set_arithmetic
#define mfn_correlation_out_shape mfn_emu_correlation_out_shape
#define mfn_correlation_workspace_bytes mfn_emu_correlation_workspace_bytes
#define mfn_correlation_fwd_into mfn_emu_correlation_fwd_into
#define mfn_correlation_bwd mfn_emu_correlation_bwd
#define mfn_warp_fwd mfn_emu_warp_fwd
#define mfn_warp_bwd mfn_emu_warp_bwd
#define mfn_grid_generator_warp mfn_emu_grid_generator_warp
#define mfn_grid_generator_affine mfn_emu_grid_generator_affine
#define mfn_bilinear_sampler_fwd mfn_emu_bilinear_sampler_fwd
#define mfn_bilinear_sampler_bwd mfn_emu_bilinear_sampler_bwd
#define mfn_grid_generator_warp_bwd mfn_emu_grid_generator_warp_bwd
#define mfn_deform_conv_workspace_bytes mfn_emu_deform_conv_workspace_bytes
#define mfn_deform_conv_fwd mfn_emu_deform_conv_fwd
#define mfn_deform_conv_shared_fwd mfn_emu_deform_conv_shared_fwd
#define mfn_deform_conv_packed_weight_bytes mfn_emu_deform_conv_packed_weight_bytes
#define mfn_deform_conv_pack_weights mfn_emu_deform_conv_pack_weights
#define mfn_deform_conv_fwd_packed mfn_emu_deform_conv_fwd_packed
#define mfn_deform_conv_matching_fwd mfn_emu_deform_conv_matching_fwd
#define mfn_deform_conv_bwd_workspace_bytes mfn_emu_deform_conv_bwd_workspace_bytes
#define mfn_deform_conv_bwd mfn_emu_deform_conv_bwd
#define mfn_deform_conv_shared_bwd_workspace_bytes mfn_emu_deform_conv_shared_bwd_workspace_bytes
#define mfn_deform_conv_shared_bwd mfn_emu_deform_conv_shared_bwd
#define mfn_offsets_from_flow_bwd mfn_emu_offsets_from_flow_bwd
#define mfn_upsample_fwd mfn_emu_upsample_fwd
#define mfn_upsample_bwd mfn_emu_upsample_bwd
#define mfn_leaky_relu_bwd mfn_emu_leaky_relu_bwd
#define mfn_offsets_from_flow mfn_emu_offsets_from_flow
#define mfn_pair_mean_workspace_bytes mfn_emu_pair_mean_workspace_bytes
#define mfn_pair_mean mfn_emu_pair_mean
#define mfn_preprocess_pair mfn_emu_preprocess_pair
#define mfn_bilinear_resize_fwd mfn_emu_bilinear_resize_fwd
#define mfn_flow_metrics_workspace_bytes mfn_emu_flow_metrics_workspace_bytes
#define mfn_flow_metrics mfn_emu_flow_metrics
#define mfn_multiscale_epe_workspace_bytes mfn_emu_multiscale_epe_workspace_bytes
#define mfn_multiscale_epe_fwd mfn_emu_multiscale_epe_fwd
#define mfn_multiscale_epe_bwd mfn_emu_multiscale_epe_bwd
#define mfn_adam_update mfn_emu_adam_update
#define mfn_multi_adam_table_bytes mfn_emu_multi_adam_table_bytes
#define mfn_multi_adam_build_table mfn_emu_multi_adam_build_table
#define mfn_multi_adam_update mfn_emu_multi_adam_update
#define mfn_batch_gather_rows_bytes mfn_emu_batch_gather_rows_bytes
#define mfn_batch_gather_build_rows mfn_emu_batch_gather_build_rows
#define mfn_batch_gather mfn_emu_batch_gather
#define mfn_ingest_tables_bytes mfn_emu_ingest_tables_bytes
#define mfn_ingest_build_tables mfn_emu_ingest_build_tables
#define mfn_ingest_minmax mfn_emu_ingest_minmax
#define mfn_ingest_image mfn_emu_ingest_image
#define mfn_ingest_flow_occ mfn_emu_ingest_flow_occ
#define mfn_png_unfilter mfn_emu_png_unfilter
#define mfn_conv2d_out_shape mfn_emu_conv2d_out_shape
#define mfn_conv2d_workspace_bytes mfn_emu_conv2d_workspace_bytes
#define mfn_conv2d_packed_weight_bytes mfn_emu_conv2d_packed_weight_bytes
#define mfn_conv2d_pack_weights mfn_emu_conv2d_pack_weights
#define mfn_conv2d_fwd mfn_emu_conv2d_fwd
#define mfn_conv2d_bwd_workspace_bytes mfn_emu_conv2d_bwd_workspace_bytes
#define mfn_conv2d_bwd mfn_emu_conv2d_bwd
#include "../../include/mfn_hip.h"
extern "C" int mfn_emu_test_launch_log(char *buf, int cap);

// A heap block of exactly `bytes` bytes, 64-byte aligned (the alignment the plans ask about), freed at the end of the call's scope.
struct Block {
  void *p = nullptr;
  size_t bytes = 0;
  explicit Block(size_t b) : bytes(b) {
    if (b && posix_memalign(&p, 64, b)) abort();
  }
  Block(const Block &) = delete;
  ~Block() { free(p); }
  float *f() const { return (float *)p; }
};
static unsigned g_seed = 12345u;
static float rnd() {   // uniform in [-1, 1)
  g_seed = g_seed * 1664525u + 1013904223u;
  return (float)(g_seed >> 8) * (2.0f / 16777216.0f) - 1.0f;
}
struct Tensor : Block {
  size_t n;
  explicit Tensor(size_t count, float scale = 1.f, bool fill = true) : Block(count * sizeof(float)), n(count) {
    for (size_t i = 0; fill && i < n; ++i) f()[i] = rnd() * scale;
  }
};

struct KV { const char *key; int value; };
static int g_failed = 0, g_calls = 0;
static std::vector<std::string> g_touched;
static void tune(const std::vector<KV> &kv) {
  for (const KV &t : kv) {
    int rc;
    if (!strcmp(t.key, "correlation") || !strcmp(t.key, "deformable_convolution") || !strcmp(t.key, "convolution")) rc = mfn_set_arithmetic(t.key, t.value);
    else rc = mfn_set_tuning(t.key, t.value);
    if (rc) { printf("  setting %s=%d refused: %s\n", t.key, t.value, mfn_last_error()); ++g_failed; }
    g_touched.push_back(t.key);
  }
}
static void untune() {
  for (const std::string &k : g_touched) {
    if (k == "correlation" || k == "deformable_convolution" || k == "convolution") mfn_set_arithmetic(k.c_str(), -1);
    else mfn_set_tuning(k.c_str(), k == "corr.variant" ? -1 : 0);
  }
  g_touched.clear();
}
static void report(const char *what, int rc) {
  char log[4096];
  mfn_emu_test_launch_log(log, sizeof(log));
  ++g_calls;
  if (rc) { ++g_failed; printf("%-44s status %d: %s\n", what, rc, mfn_last_error()); }
  else printf("%-44s ok   %s\n", what, log);
  fflush(stdout);
  untune();
}

// ---- correlation ------------------------------------------------------------------------------------------------------------------------
struct CorrRow { const char *name; std::vector<KV> t; int N, C, H, W, md, k, s1, pad, c0; };
static void corr_fwd(const CorrRow &r) {
  tune(r.t);
  int tc, th, tw;
  if (mfn_correlation_out_shape(r.H, r.W, r.md, r.k, r.s1, 1, r.pad, &tc, &th, &tw)) return report(r.name, -1);
  const size_t in = (size_t)r.N * r.C * r.H * r.W, img = (size_t)th * tw, extra = r.c0 ? 7 : 0;
  Tensor d1(in), d2(in), out((size_t)r.N * (r.c0 + tc + extra) * img, 1.f, false);
  const size_t need = mfn_correlation_workspace_bytes(r.N, r.C, r.H, r.W, r.md, r.k, r.s1, 1, r.pad, 1);
  Block ws(need);
  report(r.name, mfn_correlation_fwd_into(d1.f(), d2.f(), out.f() + r.c0 * img, r.c0 ? (long long)((r.c0 + tc + extra) * img) : 0, r.N, r.C, r.H,
                                          r.W, r.md, r.k, r.s1, 1, r.pad, 1, MFN_ACT_LEAKY_0_1, ws.p, need, nullptr));
}
struct CorrBwdRow { const char *name; std::vector<KV> t; int N, C, H, W, md, k, s1, pad, req1, req2; };
static void corr_bwd(const CorrBwdRow &r) {
  tune(r.t);
  int tc, th, tw;
  if (mfn_correlation_out_shape(r.H, r.W, r.md, r.k, r.s1, 1, r.pad, &tc, &th, &tw)) return report(r.name, -1);
  const size_t in = (size_t)r.N * r.C * r.H * r.W;
  Tensor go((size_t)r.N * tc * th * tw), d1(in), d2(in), g1(r.req1 ? in : 0), g2(r.req2 ? in : 0);
  report(r.name, mfn_correlation_bwd(go.f(), d1.f(), d2.f(), g1.f(), g2.f(), r.N, r.C, r.H, r.W, r.md, r.k, r.s1, 1, r.pad, 1, r.req1, r.req2, nullptr));
}

// ---- deformable convolution -------------------------------------------------------------------------------------------------------------
enum { DROPIN, PACKED, SHARED, MATCHING };
struct DcRow { const char *name; std::vector<KV> t; int N, Cin, Cout, H, W, groups, dg, entry; };
static void dc_fwd(const DcRow &r) {
  tune(r.t);
  const size_t px = (size_t)r.H * r.W;
  Tensor x((size_t)r.N * r.Cin * px), off((size_t)r.N * 18 * r.dg * px, 1.5f), fl((size_t)r.N * 2 * px, 0.6f), w((size_t)r.Cout * (r.Cin / r.groups) * 9, 0.1f),
      b(r.Cout), mask((size_t)r.N * px), tr((size_t)r.N * r.Cout * px), out((size_t)r.N * r.Cout * px, 1.f, false);
  const size_t need = mfn_deform_conv_workspace_bytes(r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1, 1, r.groups, r.dg);
  Block ws(need);
  int rc;
  if (r.entry == PACKED) {
    const size_t pb = mfn_deform_conv_packed_weight_bytes(r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1, 1, r.groups, r.dg);
    Block packed(pb);
    unsigned long long tag = 0;
    rc = mfn_deform_conv_pack_weights(w.f(), r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1, 1, r.groups, r.dg, packed.p, pb, &tag, nullptr);
    if (!rc) rc = mfn_deform_conv_fwd_packed(x.f(), off.f(), packed.p, pb, tag, b.f(), out.f(), r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1, 1, r.groups,
                                             r.dg, ws.p, need, nullptr);
  } else if (r.entry == SHARED) {
    rc = mfn_deform_conv_shared_fwd(x.f(), fl.f(), 20.f, 8.f, w.f(), b.f(), out.f(), r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, r.groups, ws.p, need, nullptr);
  } else if (r.entry == MATCHING) {
    rc = mfn_deform_conv_matching_fwd(x.f(), fl.f(), 20.f, 8.f, w.f(), nullptr, 0, 0, b.f(), mask.f(), tr.f(), 1, out.f(), r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1,
                                      1, 1, 1, r.groups, ws.p, need, nullptr);
  } else {
    rc = mfn_deform_conv_fwd(x.f(), off.f(), w.f(), b.f(), out.f(), r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1, 1, r.groups, r.dg, ws.p, need, nullptr);
  }
  report(r.name, rc);
}
struct DcBwdRow { const char *name; std::vector<KV> t; int N, Cin, Cout, H, W, flow, no_ws, req[4]; };
static void dc_bwd(const DcBwdRow &r) {
  tune(r.t);
  const size_t px = (size_t)r.H * r.W, nx = (size_t)r.N * r.Cin * px, nw = (size_t)r.Cout * r.Cin * 9, no = (size_t)r.N * (r.flow ? 2 : 18) * px;
  Tensor go((size_t)r.N * r.Cout * px), x(nx), off(no, r.flow ? 0.6f : 1.5f), w(nw, 0.1f);
  Tensor gx(r.req[0] ? nx : 0), goff(r.req[1] ? no : 0), gw(r.req[2] ? nw : 0), gb(r.req[3] ? r.Cout : 0);
  size_t need = r.flow ? mfn_deform_conv_shared_bwd_workspace_bytes(r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1)
                       : mfn_deform_conv_bwd_workspace_bytes(r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1);
  if (r.no_ws) need = 0;
  Block ws(need);
  int rc;
  if (r.flow)
    rc = mfn_deform_conv_shared_bwd(go.f(), x.f(), off.f(), 20.f, 8.f, w.f(), gx.f(), goff.f(), gw.f(), gb.f(), r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1,
                                    r.req[0], r.req[1], r.req[2], r.req[3], ws.p, need, nullptr);
  else
    rc = mfn_deform_conv_bwd(go.f(), x.f(), off.f(), w.f(), gx.f(), goff.f(), gw.f(), gb.f(), r.N, r.Cin, r.H, r.W, r.Cout, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, r.req[0],
                             r.req[1], r.req[2], r.req[3], ws.p, need, nullptr);
  report(r.name, rc);
}

// ---- convolution / deconvolution ----------------------------------------------------------------------------------------------------------
struct ConvRow { const char *name; std::vector<KV> t; int N, Cin, Cout, H, W, k, s, p, d, tr, adj, packed, act, bwd, req[3]; };
static void conv(const ConvRow &r) {
  tune(r.t);
  int Ho, Wo;
  if (mfn_conv2d_out_shape(r.H, r.W, r.k, r.k, r.s, r.s, r.p, r.p, r.d, r.d, r.tr, r.adj, r.adj, &Ho, &Wo)) return report(r.name, -1);
  const size_t nx = (size_t)r.N * r.Cin * r.H * r.W, nw = (size_t)r.Cin * r.Cout * r.k * r.k, ny = (size_t)r.N * r.Cout * Ho * Wo;
  Tensor x(nx), w(nw, 0.1f), b(r.Cout), y(ny, 1.f, false);
  int rc;
  {
    size_t need = mfn_conv2d_workspace_bytes(r.N, r.Cin, r.H, r.W, r.Cout, r.k, r.k, r.s, r.s, r.p, r.p, r.d, r.d, 1, r.tr);
    if (r.packed) {
      const size_t pb = mfn_conv2d_packed_weight_bytes(r.N, r.Cin, r.H, r.W, r.Cout, r.k, r.k, r.s, r.s, r.p, r.p, r.d, r.d, 1, r.tr);
      Block packed(pb);
      unsigned long long tag = 0;
      rc = mfn_conv2d_pack_weights(w.f(), r.N, r.Cin, r.H, r.W, r.Cout, r.k, r.k, r.s, r.s, r.p, r.p, r.d, r.d, 1, r.tr, packed.p, pb, &tag, nullptr);
      if (tag != 0x4d43ffff00000000ull) need = 0;   // packed for a matrix-core plan: no re-layout scratch
      Block ws(need);
      if (!rc) rc = mfn_conv2d_fwd(x.f(), 0, nullptr, packed.p, pb, tag, b.f(), y.f(), 0, r.N, r.Cin, r.H, r.W, r.Cout, r.k, r.k, r.s, r.s, r.p, r.p, r.d, r.d, 1,
                                   r.tr, r.adj, r.adj, r.act, ws.p, need, nullptr);
    } else {
      Block ws(need);
      rc = mfn_conv2d_fwd(x.f(), 0, w.f(), nullptr, 0, 0, b.f(), y.f(), 0, r.N, r.Cin, r.H, r.W, r.Cout, r.k, r.k, r.s, r.s, r.p, r.p, r.d, r.d, 1, r.tr, r.adj, r.adj,
                          r.act, ws.p, need, nullptr);
    }
  }
  if (!rc && r.bwd) {
    Tensor go(ny), gx(r.req[0] ? nx : 0), gw(r.req[1] ? nw : 0), gb(r.req[2] ? r.Cout : 0);
    const size_t need = mfn_conv2d_bwd_workspace_bytes(r.N, r.Cin, r.H, r.W, r.Cout, r.k, r.k, r.s, r.s, r.p, r.p, r.d, r.d, 1, r.tr, r.adj, r.adj, r.act);
    Block ws(need);
    rc = mfn_conv2d_bwd(go.f(), x.f(), w.f(), r.act ? y.f() : nullptr, gx.f(), gw.f(), gb.f(), r.N, r.Cin, r.H, r.W, r.Cout, r.k, r.k, r.s, r.s, r.p, r.p, r.d, r.d, 1,
                        r.tr, r.adj, r.adj, r.act, r.req[0], r.req[1], r.req[2], ws.p, need, nullptr);
  }
  report(r.name, rc);
}

// ---- entries without a workspace, and the predict entries ---------------------------------------------------------------------------------
static void others() {
  {
    const int N = 2, C = 3, H = 8, W = 11;
    const size_t n = (size_t)N * C * H * W, nf = (size_t)N * 2 * H * W;
    for (int clip = 0; clip < 2; ++clip) {
      Tensor x(n), fl(nf, 3.f), out(n, 1.f, false), go(n), gx(n, 1.f, false), gf(nf, 1.f, false);
      report(clip ? "warp_fwd clip" : "warp_fwd", mfn_warp_fwd(x.f(), fl.f(), out.f(), N, C, H, W, clip, nullptr));
      report(clip ? "warp_bwd clip" : "warp_bwd", mfn_warp_bwd(go.f(), x.f(), fl.f(), gx.f(), gf.f(), N, C, H, W, clip, 1, 1, nullptr));
    }
  }
  {
    Tensor fl(2 * 2 * 6 * 9, 2.f), grid(2 * 2 * 6 * 9, 1.f, false), theta(2 * 6), ga(2 * 2 * 5 * 7, 1.f, false), gflow(2 * 2 * 6 * 9, 1.f, false);
    report("grid_generator_warp", mfn_grid_generator_warp(fl.f(), grid.f(), 2, 6, 9, nullptr));
    report("grid_generator_affine", mfn_grid_generator_affine(theta.f(), ga.f(), 2, 5, 7, nullptr));
    report("grid_generator_warp_bwd", mfn_grid_generator_warp_bwd(fl.f(), gflow.f(), 2, 6, 9, 1, nullptr));
    Tensor d(1 * 2 * 6 * 9), g(1 * 2 * 5 * 7, 1.2f), out(1 * 2 * 5 * 7, 1.f, false), go(1 * 2 * 5 * 7), gd(1 * 2 * 6 * 9, 1.f, false), gg(1 * 2 * 5 * 7, 1.f, false);
    report("bilinear_sampler_fwd", mfn_bilinear_sampler_fwd(d.f(), g.f(), out.f(), 1, 2, 6, 9, 5, 7, nullptr));
    report("bilinear_sampler_bwd", mfn_bilinear_sampler_bwd(go.f(), d.f(), g.f(), gd.f(), gg.f(), 1, 2, 6, 9, 5, 7, 1, 1, nullptr));
  }
  for (int f : {1, 2, 8, 16}) {
    const int H = 5, W = 7;
    Tensor x(2 * H * W), out((size_t)2 * H * f * W * f, 1.f, false), gx(2 * H * W, 1.f, false);
    char name[64];
    snprintf(name, sizeof(name), "upsample_fwd x%d", f);
    report(name, mfn_upsample_fwd(x.f(), out.f(), 1, 2, H, W, f, nullptr));
    Tensor go((size_t)2 * H * f * W * f);
    snprintf(name, sizeof(name), "upsample_bwd x%d", f);
    report(name, mfn_upsample_bwd(go.f(), gx.f(), 1, 2, H, W, f, 1, nullptr));
  }
  for (size_t n : {(size_t)1, (size_t)3, (size_t)4, (size_t)1023, (size_t)1025}) {
    Tensor go(n), y(n), gi(n, 1.f, false);
    char name[64];
    snprintf(name, sizeof(name), "leaky_relu_bwd n=%zu", n);
    report(name, mfn_leaky_relu_bwd(go.f(), y.f(), gi.f(), n, 0.1f, nullptr));
  }
  for (int W : {6, 8}) {
    Tensor fl(2 * 2 * 5 * W), off(2 * 18 * 5 * W, 1.f, false), goff(2 * 18 * 5 * W), gfl(2 * 2 * 5 * W, 1.f, false);
    report(W == 6 ? "offsets_from_flow W=6" : "offsets_from_flow W=8", mfn_offsets_from_flow(fl.f(), off.f(), 2, 5, W, 9, 20.f, 16.f, nullptr));
    report(W == 6 ? "offsets_from_flow_bwd W=6" : "offsets_from_flow_bwd W=8", mfn_offsets_from_flow_bwd(goff.f(), gfl.f(), 2, 5, W, 9, 20.f, 16.f, 1, nullptr));
  }
  {
    const int N = 2, C = 3, H = 9, W = 13;
    Tensor a((size_t)N * C * H * W, 100.f), b((size_t)N * C * H * W, 100.f), mean(N * C, 1.f, false), out((size_t)2 * N * C * 6 * 10, 1.f, false);
    const size_t need = mfn_pair_mean_workspace_bytes(N, C, H, W);
    Block ws(need);
    report("pair_mean", mfn_pair_mean(a.f(), b.f(), mean.f(), N, C, H, W, ws.p, need, nullptr));
    report("preprocess_pair", mfn_preprocess_pair(a.f(), b.f(), mean.f(), out.f(), N, C, H, W, 6, 10, nullptr));
    Tensor up((size_t)N * C * 12 * 17, 1.f, false), down((size_t)N * C * 5 * 6, 1.f, false), same((size_t)N * C * H * W, 1.f, false);
    report("bilinear_resize up, sub", mfn_bilinear_resize_fwd(a.f(), mean.f(), up.f(), N, C, H, W, 12, 17, 0, nullptr));
    report("bilinear_resize down", mfn_bilinear_resize_fwd(a.f(), nullptr, down.f(), N, C, H, W, 5, 6, 0, nullptr));
    report("bilinear_resize equal", mfn_bilinear_resize_fwd(a.f(), nullptr, same.f(), N, C, H, W, H, W, 0, nullptr));
    report("bilinear_resize equal, sub", mfn_bilinear_resize_fwd(a.f(), mean.f(), same.f(), N, C, H, W, H, W, 0, nullptr));
    Tensor fl((size_t)N * 2 * H * W, 4.f), lab((size_t)N * 2 * H * W, 4.f), mask((size_t)N * H * W), sums(N * 3, 1.f, false), flup((size_t)N * 2 * 12 * 17, 1.f, false);
    report("bilinear_resize flow rescale", mfn_bilinear_resize_fwd(fl.f(), nullptr, flup.f(), N, 2, H, W, 12, 17, 1, nullptr));
    const size_t need2 = mfn_flow_metrics_workspace_bytes(N, H, W);
    Block ws2(need2);
    report("flow_metrics", mfn_flow_metrics(fl.f(), lab.f(), mask.f(), sums.f(), N, H, W, ws2.p, need2, nullptr));
  }
  // the fused multiscale loss: forward v4 / v1, backward with 1, 64 and 256 threads per input pixel, plane and per-sample mask, both forms
  struct LossRow { const char *name; int N, h, w, f0, f1, scalar_mask, robust; };
  for (const LossRow &r : {LossRow{"multiscale_epe v4, t1 + t64", 2, 2, 4, 4, 8, 0, 0}, LossRow{"multiscale_epe v1, t1 (f = 3, 1)", 2, 3, 5, 3, 1, 0, 1},
                           LossRow{"multiscale_epe v4, t256 + t64, scalar mask", 1, 1, 2, 32, 16, 1, 1}, LossRow{"multiscale_epe W = 1", 1, 3, 1, 1, 1, 1, 0}}) {
    const int H = r.h * r.f0, W = r.w * r.f0, fs[2] = {r.f0, r.f1};
    Tensor p0((size_t)r.N * 2 * r.h * r.w, 4.f), p1((size_t)r.N * 2 * (H / r.f1) * (W / r.f1), 4.f), lab((size_t)r.N * 2 * H * W, 4.f);
    Tensor mask(r.scalar_mask ? (size_t)r.N : (size_t)r.N * H * W), loss(r.N, 1.f, false), sums(r.N * 3, 1.f, false), gloss(r.N);
    Tensor g0(p0.n, 1.f, false), g1(p1.n);
    for (size_t i = 0; i < mask.n; ++i) mask.f()[i] = mask.f()[i] > 0.4f ? 0.f : 1.f;
    const float *preds[2] = {p0.f(), p1.f()};
    float *gp[2] = {g0.f(), g1.f()};
    const float wts[2] = {0.32f, 0.08f};
    const int reqs[2] = {MFN_REQ_WRITE, MFN_REQ_ADD};
    const size_t need = mfn_multiscale_epe_workspace_bytes(r.N, H, W, 2);
    Block ws(need);
    char name[96];
    snprintf(name, sizeof(name), "%s fwd", r.name);
    report(name, mfn_multiscale_epe_fwd(preds, fs, wts, 2, lab.f(), mask.f(), r.scalar_mask, 1e-8f, r.robust, 0.4f, loss.f(), sums.f(), r.N, H, W, ws.p,
                                        need, nullptr));
    snprintf(name, sizeof(name), "%s bwd", r.name);
    report(name, mfn_multiscale_epe_bwd(gloss.f(), preds, fs, wts, 2, lab.f(), mask.f(), r.scalar_mask, 1e-8f, r.robust, 0.4f, sums.f(), gp, reqs, r.N, H,
                                        W, nullptr));
  }
  // the trainer's Adam step: every count around a block of 4096 elements, each tensor a heap block of its exact size (the 16-byte
  // route with its scalar tail), then the same tensors one float into blocks one float longer (the one-element route), single and multi
  {
    const long long counts[8] = {2 * 4096 + 7, 1, 4097, 3, 4, 5, 4095, 4096};
    for (int shift = 0; shift < 2; ++shift) {
      std::vector<Tensor *> own;
      float *w[8], *m[8], *v[8];
      const float *g[8];
      for (int i = 0; i < 8; ++i) {
        Tensor *t[4];
        for (int k = 0; k < 4; ++k) own.push_back(t[k] = new Tensor((size_t)counts[i] + shift));
        for (size_t e = 0; e < t[3]->n; ++e) t[3]->f()[e] = fabsf(t[3]->f()[e]);
        w[i] = t[0]->f() + shift; g[i] = t[1]->f() + shift; m[i] = t[2]->f() + shift; v[i] = t[3]->f() + shift;
      }
      char name[96];
      for (int i = 0; i < 8; ++i) {
        snprintf(name, sizeof(name), "adam_update n = %lld%s", counts[i], shift ? ", unaligned" : "");
        report(name, mfn_adam_update(w[i], g[i], m[i], v[i], counts[i], 1e-4f, 0.9f, 0.999f, 1e-8f, 1e-2f, 0.5f, 1.f, nullptr));
      }
      const size_t need = mfn_multi_adam_table_bytes(8, counts);
      Block table(need);
      int nb = 0;
      unsigned long long tag = 0;
      int rc = mfn_multi_adam_build_table(8, w, g, m, v, counts, nullptr, nullptr, table.p, need, &nb, &tag);
      snprintf(name, sizeof(name), "multi_adam_update, 8 tensors%s", shift ? ", unaligned" : "");
      report(name, rc ? rc : mfn_multi_adam_update(table.p, need, tag, 8, nb, 1e-4f, 0.9f, 0.999f, 1e-8f, 1e-2f, 0.5f, 1.f, nullptr));
      for (Tensor *t : own) delete t;
    }
  }
  // one training batch out of resident samples (kernels/batch.h): every source array a heap block of exactly its size rounded up to 16 bytes
  // (the read contract), every output of exactly its size; both store paths, crops on all four source edges, both flips, both label
  // types, a slot without a mask, a call without one, and a label tensor 12 bytes into its block (single-dword label stores, ends exact)
  {
    struct Src { int Hs, Ws, lt, y0, x0, flip, has_mask; };
    struct Row { const char *name; int Hc, Wc, with_mask, label_off; std::vector<Src> s; };
    const std::vector<Row> rows = {
        {"batch_gather 7x10 mixed, byte path", 7, 10, 1, 0, {{9, 14, 0, 0, 0, 0, 1}, {11, 13, 1, 4, 3, 1, 1}, {7, 10, 1, 0, 0, 1, 0}, {8, 23, 0, 1, 13, 0, 1}}},
        {"batch_gather 7x12 mixed, dword path", 7, 12, 1, 0, {{9, 14, 0, 0, 0, 0, 1}, {11, 13, 1, 4, 1, 1, 1}, {7, 12, 1, 0, 0, 1, 0}, {8, 23, 0, 1, 11, 0, 1}}},
        {"batch_gather 7x12, label at 12 mod 16", 7, 12, 1, 12, {{9, 14, 0, 2, 2, 1, 1}, {7, 12, 1, 0, 0, 0, 0}}},
        {"batch_gather 3x5 at the last pixel, no mask", 3, 5, 0, 0, {{5, 9, 0, 2, 4, 1, 1}, {5, 9, 1, 2, 4, 0, 0}}},
        {"batch_gather 3x260 of 300 at 37", 3, 260, 1, 0, {{4, 300, 0, 1, 37, 0, 1}, {3, 300, 1, 0, 40, 1, 1}}},
        {"batch_gather 3x261 of 300 at 37", 3, 261, 1, 0, {{4, 300, 1, 1, 37, 1, 1}, {3, 300, 0, 0, 39, 0, 0}}},
        {"batch_gather 8x16 uncropped", 8, 16, 0, 0, {{8, 16, 0, 0, 0, 0, 0}, {8, 16, 1, 0, 0, 1, 0}}},
    };
    for (const Row &r : rows) {
      const int N = (int)r.s.size();
      std::vector<Block *> own;
      auto bytes16 = [&](size_t n) {
        Block *b = new Block((n + 15) & ~(size_t)15);
        for (size_t i = 0; i < b->bytes; ++i) ((unsigned char *)b->p)[i] = (unsigned char)(rnd() * 127.f);
        own.push_back(b);
        return (const void *)b->p;
      };
      std::vector<const void *> i1(N), i2(N), fl(N), mk(N);
      std::vector<int> Hs(N), Ws(N), lt(N), y0(N), x0(N), flip(N);
      for (int n = 0; n < N; ++n) {
        const Src &q = r.s[n];
        const size_t px = (size_t)q.Hs * q.Ws;
        i1[n] = bytes16(3 * px); i2[n] = bytes16(3 * px); fl[n] = bytes16((q.lt ? 4 : 8) * px);
        mk[n] = q.has_mask ? bytes16(px) : nullptr;
        Hs[n] = q.Hs; Ws[n] = q.Ws; lt[n] = q.lt; y0[n] = q.y0; x0[n] = q.x0; flip[n] = q.flip;
      }
      const size_t need = mfn_batch_gather_rows_bytes(N), plane = (size_t)r.Hc * r.Wc;
      Block table(need), o1(3 * N * plane), o2(3 * N * plane), lab(8 * N * plane + r.label_off), om(r.with_mask ? N * plane : 0);
      unsigned long long tag = 0;
      int rc = mfn_batch_gather_build_rows(N, i1.data(), i2.data(), fl.data(), mk.data(), Hs.data(), Ws.data(), lt.data(), y0.data(), x0.data(),
                                           flip.data(), r.Hc, r.Wc, table.p, need, &tag);
      report(r.name, rc ? rc : mfn_batch_gather(table.p, need, tag, N, r.Hc, r.Wc, r.with_mask, (unsigned char *)o1.p, (unsigned char *)o2.p,
                                                (float *)((char *)lab.p + r.label_off), (unsigned char *)om.p, nullptr));
      for (Block *b : own) delete b;
    }
  }
  // raw arrays into stored samples (kernels/ingest.h): every source a heap block of exactly its size rounded up to 16 bytes (the read
  // contract), every output and table of exactly its size; windows at odd byte offsets and against the array's last row and column,
  // image sizes that end inside a 16-byte piece, pixel counts that end inside a quad, both flow types, the stretch
  {
    struct Row { const char *name; int H, W, y0, x0, h, w, Hd, Wd, bgr, stretch, pre, f16; };
    const std::vector<Row> rows = {
        {"ingest 13x21 of 17x29 -> 9x31", 17, 29, 3, 5, 13, 21, 9, 31, 1, 0, 0, 0},
        {"ingest last rows / columns, stretch, fp16", 17, 29, 4, 8, 13, 21, 7, 27, 0, 1, 1, 1},
        {"ingest 2x2 -> 5x3", 2, 2, 0, 0, 2, 2, 5, 3, 0, 1, 0, 1},
        {"ingest equal sizes", 11, 19, 0, 0, 11, 19, 11, 19, 1, 0, 1, 0},
        {"ingest 37x53 -> 70x150", 37, 53, 0, 0, 37, 53, 70, 150, 0, 1, 0, 0},
    };
    for (const Row &r : rows) {
      auto bytes16 = [&](size_t n) {
        Block *b = new Block((n + 15) & ~(size_t)15);
        for (size_t i = 0; i < b->bytes; ++i) ((unsigned char *)b->p)[i] = (unsigned char)(rnd() * 127.f + 128.f);
        return b;
      };
      const size_t px = (size_t)r.H * r.W, dpx = (size_t)r.Hd * r.Wd, need = mfn_ingest_tables_bytes(r.Hd, r.Wd);
      Block *i1 = bytes16(3 * px), *i2 = bytes16(3 * px), *fo = bytes16(6 * px);
      Block tab(need), mm(8), o1(3 * dpx), o2(3 * dpx), fl((r.f16 ? 4 : 8) * dpx), mk(dpx);
      unsigned long long tag = 0;
      int rc = mfn_ingest_build_tables(r.h, r.w, r.Hd, r.Wd, tab.p, need, &tag);
      if (!rc && r.stretch) rc = mfn_ingest_minmax((const unsigned char *)i1->p, (const unsigned char *)i2->p, r.H, r.W, 3 * r.W, r.y0, r.x0, r.h, r.w, (unsigned *)mm.p, nullptr);
      if (!rc) rc = mfn_ingest_image((const unsigned char *)i1->p, r.H, r.W, 3 * r.W, r.y0, r.x0, r.h, r.w, tab.p, need, tag, r.bgr, r.stretch ? (const unsigned *)mm.p : nullptr,
                                     (unsigned char *)o1.p, r.Hd, r.Wd, nullptr);
      if (!rc) rc = mfn_ingest_image((const unsigned char *)i2->p, r.H, r.W, 3 * r.W, r.y0, r.x0, r.h, r.w, tab.p, need, tag, r.bgr, r.stretch ? (const unsigned *)mm.p : nullptr,
                                     (unsigned char *)o2.p, r.Hd, r.Wd, nullptr);
      if (!rc) rc = mfn_ingest_flow_occ((const unsigned short *)fo->p, r.H, r.W, 3 * r.W, r.y0, r.x0, r.h, r.w, tab.p, need, tag, r.pre, r.f16, fl.p, (unsigned char *)mk.p,
                                        r.Hd, r.Wd, nullptr);
      report(r.name, rc);
      delete i1; delete i2; delete fo;
    }
  }
  // the PNG row filters (host code of the library): scanlines of every filter type, one and eight bytes per pixel, a row shorter than
  // a pixel, the buffer a heap block of exactly rows * (1 + row_bytes) bytes; then a filter type that does not exist
  {
    struct Row { const char *name; long long rows, row_bytes; int bpp; };
    for (const Row &r : {Row{"png_unfilter 11 x 37, 1 byte per pixel", 11, 37, 1}, Row{"png_unfilter 10 x 40, 8 bytes per pixel", 10, 40, 8},
                         Row{"png_unfilter 7 x 3, 6 bytes per pixel", 7, 3, 6}, Row{"png_unfilter 1 x 1", 1, 1, 1}, Row{"png_unfilter no rows", 0, 5, 3}}) {
      Block raw((size_t)(r.rows * (r.row_bytes + 1)));
      for (size_t i = 0; i < raw.bytes; ++i) ((unsigned char *)raw.p)[i] = (unsigned char)(rnd() * 127.f + 128.f);
      for (long long y = 0; y < r.rows; ++y) ((unsigned char *)raw.p)[y * (r.row_bytes + 1)] = (unsigned char)((y + 4) % 5);
      report(r.name, mfn_png_unfilter((unsigned char *)raw.p, r.rows, r.row_bytes, r.bpp));
    }
    Block raw(2 * 6);
    memset(raw.p, 0, raw.bytes);
    ((unsigned char *)raw.p)[6] = 5;
    report("png_unfilter refuses filter type 5", mfn_png_unfilter((unsigned char *)raw.p, 2, 5, 1) == MFN_E_PARAM ? 0 : -1);
  }
}

int main() {
  const std::vector<KV> D2 = {{"corr.direct", 2}};
  const std::vector<CorrRow> corr = {
      {"corr gram v48", {{"corr.variant", 48}, {"corr.direct", 2}}, 1, 32, 10, 24, 4, 1, 1, 4, 0},
      {"corr gram v48 rows 8, into a slice", {{"corr.variant", 48}, {"corr.direct", 2}, {"corr.rows", 8}}, 2, 32, 13, 20, 4, 1, 1, 4, 4},
      {"corr gram v48c2", {{"corr.variant", 48}, {"corr.direct", 2}, {"corr.rows", 2}}, 1, 64, 9, 24, 4, 1, 1, 4, 0},
      {"corr gram v46", {{"corr.variant", 46}, {"corr.direct", 2}, {"corr.rows", 6}}, 1, 32, 7, 36, 2, 1, 1, 2, 0},
      {"corr gramk v44", {{"corr.variant", 44}, {"corr.direct", 2}}, 1, 96, 5, 16, 4, 1, 1, 4, 0},
      {"corr gramk v45", {{"corr.variant", 45}, {"corr.direct", 2}}, 1, 64, 4, 24, 2, 1, 1, 2, 0},
      {"corr dma v26", {{"corr.variant", 26}, {"corr.direct", 2}}, 1, 12, 6, 40, 4, 1, 1, 4, 0},
      {"corr direct", {{"corr.direct", 1}}, 2, 30, 6, 8, 4, 1, 1, 4, 0},
      {"corr tiled v6 + reduce", {{"corr.variant", 6}, {"corr.direct", 2}}, 2, 32, 7, 16, 4, 1, 1, 4, 0},
      {"corr tiled v6 + reduce, into a slice", {{"corr.variant", 6}, {"corr.direct", 2}}, 2, 16, 7, 16, 4, 1, 1, 4, 4},
      {"corr plan fp32 (1,96,5,16)", {{"correlation", 0}}, 1, 96, 5, 16, 4, 1, 1, 4, 0},
      {"corr generic k3 s1=2", {}, 2, 3, 9, 10, 2, 3, 2, 3, 0},
      {"corr unaligned slice", {}, 2, 5, 5, 6, 4, 1, 1, 4, 3},
      {"corr odd width", {}, 1, 3, 5, 7, 4, 1, 1, 4, 0},
      {"corr W=30", {}, 2, 8, 20, 30, 2, 1, 1, 2, 0},
  };
  for (const CorrRow &r : corr) corr_fwd(r);
  const std::vector<CorrBwdRow> cbwd = {
      {"corr_bwd lds ww", {}, 2, 5, 6, 16, 4, 1, 1, 4, 1, 1},
      {"corr_bwd lds wn", {}, 2, 5, 6, 16, 4, 1, 1, 4, 1, 0},
      {"corr_bwd block na", {{"bwd.off", 4}}, 2, 5, 6, 16, 4, 1, 1, 4, 0, 3},
      {"corr_bwd block ww", {{"bwd.off", 4}}, 2, 5, 6, 16, 4, 1, 1, 4, 1, 1},
      {"corr_bwd gather W=7 ww", {}, 2, 3, 5, 7, 4, 1, 1, 4, 1, 1},
      {"corr_bwd gather W=7 na", {}, 2, 3, 5, 7, 4, 1, 1, 4, 0, 3},
      {"corr_bwd generic ww", {}, 2, 3, 9, 10, 2, 3, 2, 3, 1, 1},
  };
  for (const CorrBwdRow &r : cbwd) corr_bwd(r);
  const std::vector<DcRow> dc = {
      {"dc_mma 1x4x4 C32", {{"dc.mt", 1}, {"dc.pt", 4}, {"dc.nw", 4}}, 1, 32, 32, 6, 8, 1, 1, DROPIN},
      {"dc_mma 2x3x12 C64", {{"dc.mt", 2}, {"dc.pt", 3}, {"dc.nw", 12}}, 1, 64, 64, 6, 8, 1, 1, DROPIN},
      {"dc_mma 3x1x6 C96", {{"dc.mt", 3}, {"dc.pt", 1}, {"dc.nw", 6}}, 1, 96, 96, 6, 8, 1, 1, DROPIN},
      {"dc_mma 1x1x1 C48", {{"dc.mt", 1}, {"dc.pt", 1}, {"dc.nw", 1}}, 1, 48, 48, 6, 8, 1, 1, DROPIN},
      {"dc_mma packed", {}, 1, 32, 32, 6, 8, 1, 1, PACKED},
      {"dc_mma shared", {}, 1, 32, 32, 6, 8, 1, 1, SHARED},
      {"dc_mma matching", {}, 1, 32, 32, 6, 8, 1, 1, MATCHING},
      {"dc_lds fp32", {{"deformable_convolution", 0}}, 1, 32, 32, 8, 16, 1, 1, DROPIN},
      {"dc_lds fp32 W=7", {{"deformable_convolution", 0}}, 1, 32, 32, 6, 7, 1, 1, SHARED},
      {"dc_lds fp32 packed", {{"deformable_convolution", 0}}, 1, 32, 32, 6, 8, 1, 1, PACKED},
      {"dc_lds split K", {{"deformable_convolution", 0}, {"dc.pt", 1}, {"dc.ksb", 2}}, 1, 32, 32, 4, 8, 1, 1, DROPIN},
      {"dc_lds split K matching", {{"deformable_convolution", 0}, {"dc.pt", 1}, {"dc.ksb", 2}}, 1, 32, 32, 4, 8, 1, 1, MATCHING},
      {"dc generic groups 2", {}, 2, 4, 6, 6, 7, 2, 1, DROPIN},
      {"dc generic deformable groups 2", {}, 2, 4, 6, 6, 7, 1, 2, DROPIN},
  };
  for (const DcRow &r : dc) dc_fwd(r);
  const std::vector<DcBwdRow> dcb = {
      {"dc_bwd pix + pc slabs", {}, 1, 4, 4, 5, 16, 0, 0, {1, 1, 1, 1}},
      {"dc_bwd pix + pc slabs add", {}, 1, 4, 4, 5, 16, 0, 0, {3, 3, 3, 3}},
      {"dc_bwd weights only", {}, 1, 4, 4, 5, 16, 0, 0, {0, 0, 1, 0}},
      {"dc_bwd pc atomics (no workspace)", {}, 1, 4, 4, 5, 16, 0, 1, {1, 1, 1, 1}},
      {"dc_bwd tile + mfma W=17", {}, 1, 2, 4, 9, 17, 0, 0, {1, 1, 1, 1}},
      {"dc_bwd generic", {{"path.generic", 2}}, 1, 4, 4, 5, 16, 0, 0, {1, 1, 1, 1}},
      {"dc_bwd tile (bwd.off=1)", {{"bwd.off", 1}}, 1, 4, 4, 4, 16, 0, 0, {1, 1, 1, 1}},
      {"dc_bwd 100 filters", {}, 1, 8, 100, 5, 8, 0, 0, {1, 1, 1, 1}},
      {"dc_bwd ragged blocks (1,36,40,5,16)", {}, 1, 36, 40, 5, 16, 0, 0, {1, 1, 1, 1}},
      // 261 tiles of 8x4 pixels: two per block of the weight kernel, one in the last (tpb = 2, nblk = 131 in dc_bwd_plan); slabs per block
      {"dc_bwd pc slabs, two tiles per block", {}, 1, 4, 4, 116, 72, 0, 0, {0, 0, 1, 1}},
      {"dc_shared_bwd flow mode", {}, 1, 4, 4, 5, 8, 1, 0, {1, 1, 1, 1}},
      {"dc_shared_bwd composed", {{"bwd.off", 2}}, 1, 4, 4, 5, 8, 1, 0, {1, 3, 1, 1}},
      {"dc_shared_bwd composed W=17", {}, 1, 2, 4, 9, 17, 1, 0, {1, 1, 1, 1}},
  };
  for (const DcBwdRow &r : dcb) dc_bwd(r);
  const std::vector<KV> F32 = {{"convolution", 0}}, DCM = {{"conv.dcm", 2}}, G4 = {{"path.generic", 4}}, G2 = {{"path.generic", 2}};
  const std::vector<ConvRow> convs = {
      //                                      N  Cin Cout H   W  k  s  p  d tr adj packed act bwd req
      {"conv3x3 bf16x3 + bwd", {}, 1, 8, 32, 8, 16, 3, 1, 1, 1, 0, 0, 0, 1, 1, {1, 1, 1}},
      {"conv3x3 mfma + bwd", F32, 1, 8, 32, 8, 16, 3, 1, 1, 1, 0, 0, 0, 1, 1, {1, 1, 1}},
      {"conv3x3 stride 2 + bwd (deconv adj11)", {}, 1, 8, 16, 12, 16, 3, 2, 1, 1, 0, 0, 0, 0, 1, {1, 1, 1}},
      {"conv3x3 stride 2 fp32 + bwd (adj00)", F32, 1, 8, 16, 13, 17, 3, 2, 1, 1, 0, 0, 0, 0, 1, {1, 1, 1}},
      {"conv3x3 dcm + bwd", DCM, 2, 37, 32, 6, 16, 3, 1, 1, 1, 0, 0, 0, 1, 1, {1, 1, 1}},
      {"conv3x3 dilated + bwd (flip, wgrad)", {}, 1, 4, 8, 12, 16, 3, 1, 2, 2, 0, 0, 0, 1, 1, {1, 1, 1}},
      {"conv3x3 dilated W=12 + bwd (flip, mfma)", F32, 1, 4, 8, 12, 12, 3, 1, 2, 2, 0, 0, 0, 1, 1, {3, 3, 3}},
      {"conv 1x1 generic", {}, 2, 6, 8, 7, 9, 1, 1, 0, 1, 0, 0, 0, 0, 0, {0, 0, 0}},
      {"conv3x3 few (2 filters) + bwd", {}, 2, 37, 2, 6, 16, 3, 1, 1, 1, 0, 0, 0, 0, 1, {1, 1, 1}},
      {"conv3x3 W=12 + bwd (pc slabs)", {}, 2, 4, 6, 8, 12, 3, 1, 1, 1, 0, 0, 0, 1, 1, {1, 1, 1}},
      {"conv3x3 65x64 + bwd (two-stage bias)", {}, 1, 4, 2, 65, 64, 3, 1, 1, 1, 0, 0, 0, 0, 1, {1, 0, 3}},
      {"conv3x3 + bwd path.generic=4", G4, 1, 8, 32, 8, 16, 3, 1, 1, 1, 0, 0, 0, 0, 1, {1, 1, 1}},
      {"conv3x3 dilated + bwd path.generic=2", G2, 1, 4, 8, 12, 12, 3, 1, 2, 2, 0, 0, 0, 0, 1, {1, 1, 1}},
      {"deconv 4x4 + bwd (s2d)", {}, 2, 8, 4, 4, 8, 4, 2, 1, 1, 1, 0, 0, 1, 1, {1, 1, 1}},
      {"deconv 4x4 fp32 + bwd (s2d 32)", F32, 2, 32, 16, 6, 8, 4, 2, 1, 1, 1, 0, 0, 1, 1, {3, 3, 3}},
      {"deconv 4x4 as conv3x3", {}, 2, 9, 16, 5, 8, 4, 2, 1, 1, 1, 0, 0, 1, 0, {0, 0, 0}},
      {"deconv 4x4 pad 0 + bwd (generic)", {}, 1, 16, 8, 6, 8, 4, 2, 0, 1, 1, 0, 0, 0, 1, {1, 1, 1}},
      {"deconv 3x3 adj 1 + bwd", {}, 1, 16, 8, 6, 8, 3, 2, 1, 1, 1, 1, 0, 1, 1, {1, 1, 1}},
      {"deconv 3x3 adj 1 fp32", F32, 1, 16, 8, 6, 8, 3, 2, 1, 1, 1, 1, 0, 0, 0, {0, 0, 0}},
      {"conv3x3 packed bf16x3", {}, 1, 8, 32, 8, 16, 3, 1, 1, 1, 0, 0, 1, 1, 0, {0, 0, 0}},
      {"conv3x3 packed mfma", F32, 1, 8, 32, 8, 16, 3, 1, 1, 1, 0, 0, 1, 1, 0, {0, 0, 0}},
      {"conv3x3 packed dcm", DCM, 2, 37, 32, 6, 16, 3, 1, 1, 1, 0, 0, 1, 1, 0, {0, 0, 0}},
      {"deconv 4x4 packed", F32, 2, 9, 16, 5, 8, 4, 2, 1, 1, 1, 0, 1, 1, 0, {0, 0, 0}},
  };
  for (const ConvRow &r : convs) conv(r);
  others();
  printf("%d calls, %d refused or failed\n", g_calls, g_failed);
  return g_failed ? 1 : 0;
}
