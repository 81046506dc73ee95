// api_impl.inc -- argument checking and kernel dispatch behind include/mfn_hip.h.
// Included by api.hip (product, symbols mfn_*) and by tests/emu/emu_api.cpp (kernel-logic
// emulation for the CPU-only CI, symbols mfn_emu_*; test infrastructure only).
// MFN_API(name) expands to the exported symbol.

#include <atomic>
#include <initializer_list>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "kernels/correlation.h"
#include "kernels/correlation_direct.h"
#include "kernels/correlation_gram.h"
#include "kernels/correlation_gramk.h"
#include "kernels/conv_wgrad.h"
#include "kernels/deform_conv.h"
#include "kernels/deform_conv_mma.h"
#include "kernels/warp.h"
#include "kernels/upsample.h"
#include "kernels/predict.h"
#include "kernels/frames.h"
#include "kernels/augment.h"
#include "kernels/loss.h"
#include "kernels/gate.h"
#include "kernels/optimizer.h"
#include "kernels/batch.h"
#include "kernels/validate.h"
#include "kernels/ingest.h"
#include "kernels/backward.h"
#include "kernels/dc_backward.h"
#include "kernels/conv.h"
#include "tuning.h"

namespace mfn {

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
static int hipfail(int rc, const char *what) {
  if (rc == 0) return 0;
  snprintf(g_err, sizeof(g_err), "%s: HIP error %d (%s)", what, rc, hipGetErrorString((hipError_t)rc));
  return rc;
}
static inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p % a) == 0; }

Tuning g_tuning;
// Arithmetic of the three GEMM-shaped operators (include/mfn_hip.h "Arithmetic"): ONE setting per process (atomic), read by whichever
// thread makes the call.  (Round 5 kept it per thread: torch runs backward on its autograd thread and MXNet every operator on
// custom-op worker threads, so the caller's choice never reached the kernels launched there -- ADVICE r05.)
// -1 = the library's compiled-in default (the bf16 x 3 matrix-core kernels wherever one exists for the shape), 0 = fp32 FMA
// kernels everywhere, 1 = as the default (kept distinct so that tests can say "the matrix-core kernel or an error").
struct Arith { std::atomic<int> corr{-1}, deform{-1}, conv{-1}; };
static Arith t_arith;
void *g_timeline = nullptr;  // measurement only (mfn_debug_set_timeline)
static thread_local int t_last_dc_plan[4] = {0, 0, 0, 0};  // mt, pt, kw, areg of this thread's last dc_mma launch (mfn_debug_last_dc_plan)
// One reading of the process-wide settings.  Every exported entry point that plans takes it once (each atomic loaded once) and passes
// it down, so that a call is planned from one set of values and every plan below is a function of its arguments.
struct Settings { Tuning t; int corr, deform, conv; };
static Settings settings_now() { return Settings{g_tuning, t_arith.corr.load(), t_arith.deform.load(), t_arith.conv.load()}; }

// ---- correlation ---------------------------------------------------------------------------------
static int corr_shape(int H, int W, int md, int kernel, int s1, int s2, int pad, int *tc, int *th, int *tw) {
  if (H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "correlation: H=%d W=%d must be positive", H, W);
  if (md < 0 || kernel < 1 || s1 < 1 || s2 < 1 || pad < 0)
    return fail(MFN_E_PARAM, "correlation: bad parameter (max_displacement=%d kernel_size=%d stride1=%d stride2=%d pad_size=%d)",
                md, kernel, s1, s2, pad);
  if ((kernel % 2) == 0) return fail(MFN_E_PARAM, "correlation: kernel size should be odd number (got %d)", kernel);
  const int Hp = H + 2 * pad, Wp = W + 2 * pad;
  const int border = md + (kernel - 1) / 2;
  const int th_ = (int)ceilf((float)(Hp - border * 2) / (float)s1);
  const int tw_ = (int)ceilf((float)(Wp - border * 2) / (float)s1);
  if (th_ < 1 || tw_ < 1)
    return fail(MFN_E_SHAPE, "correlation: Correlation cannot be done with current settings. Neighborhood and kernel don't fit in blob");
  const int r = md / s2, gw = 2 * r + 1;
  if (tc) *tc = gw * gw;
  if (th) *th = th_;
  if (tw) *tw = tw_;
  return 0;
}

// What corr_plan (below) decides for a forward call and corr_fwd_common executes.
struct CorrPlan {
  CorrFamily family;
  const CorrForm *form;   // Tiled / Dma / Gram / GramK: the template point (channel groups, row split, terms, f2 rows)
  int D;                  // displacements per axis (every family but Generic: 9 or 5)
  int tile_w, tile_h;     // Tiled / Dma: pixels per tile
  int slices;             // Tiled / Dma: channel slices over blockIdx.y; > 1: partial sums in the workspace + corr_reduce
  int rows;               // Gram: output rows per work item
  int store_policy;
  size_t ws_bytes;        // workspace the launch uses
};
template <int D>
static int corr_tile_launch(const CorrParams &p, const CorrPlan &pl, hipStream_t s) {
  if (pl.family == CorrFamily::Dma) return corr_dma_form<D>(p, *pl.form, s);
  return pl.tile_w == 16 ? corr_tiled_form<D, 16>(p, s) : corr_tiled_form<D, 8>(p, s);
}

}  // namespace mfn

using namespace mfn;

extern "C" {

const char *MFN_API(last_error)(void) { return g_err; }

int MFN_API(correlation_out_shape)(int H, int W, int md, int kernel, int s1, int s2, int pad, int *tc, int *th,
                                   int *tw) {
  return corr_shape(H, W, md, kernel, s1, s2, pad, tc, th, tw);
}

// ---- correlation forward: one plan -----------------------------------------------------------------
// Does the plan give this level to corr_gramk_kernel (the coarse levels' Gram band, channels over the waves of a block), and
// with how many f2 rows per block?  Same box, back to back in a graph (profiles/r04_corr_gramk.txt), 384x512 at batch 8 /
// 448x1024 at batch 4: level 6 (24 / 32 f1 blocks of 8 x 2 px) 7.85 -> 3.4 us / 7.58 -> 3.4 with two rows per block;
// level 5 (96 / 112) 7.18 -> 3.4 / 7.17 -> 3.9; level 4 (384 / 448) 7.02 -> 5.95 / 9.13 -> 7.0 with half the window per
// block; level 3 (1536 / 1792 blocks) loses (9.65 -> 12.0 us: every f2 row is converted by five blocks) and keeps its kernel.
// MFN_ARITH_FP32 keeps the fp32-FMA kernels everywhere.  Returns the form or nullptr.
static const CorrForm *corr_gramk_plan(int N, int C, int H, int W, const Settings &st) {
  if (st.corr == 0 || C <= 32 || !corr_gramk_shape_ok(C, W)) return nullptr;
  const long nb = (long)N * cdiv(H, 2) * cdiv(W, 8);
  return nb <= 160 ? &kCorrForms[kCorrGramK2] : (nb <= 512 ? &kCorrForms[kCorrGramKHalf] : nullptr);
}

// The tile kernel of a level by its count of 32x4-pixel tiles.
// >= 400 tiles (level 2): the single-buffered LDS-DMA form (16) keeps every block of the launch resident (17.0 vs 18.6 us
// for the double-buffered ring at 384x512).  128-399 tiles (level 3): two channel groups per block, reduced through LDS
// in the same launch (9.7 us; 13.6 with one group).  Fewer tiles than that leave CUs idle and the work of one tile is
// what ONE CU can pull through its LDS and VALU: the displacement rows of a tile are spread over blockIdx.z (variant 26:
// one row pair per block and 4 channel groups; 31: two row pairs, 2 groups) as long as the launch still fits one round
// of 256 CUs -- level 4 (48 tiles) 12.4 -> 7.1 us, level 5 (24 half-filled tiles) 13.0 (band kernel) -> 7.2 us,
// 448x1024: level 4 (56 tiles) 12.7 -> 9.3, level 5 15.3 -> 7.2 us.  At 192 tiles the split loses (10.8-20 us vs 9.7).
static const CorrForm *corr_tile_form(int N, int H, int W, int D) {
  const long t32 = (long)N * cdiv(W, 32) * cdiv(H, 4);
  const int nw = (D + 1) / 2;   // row-pair waves of a tile
  if (W < 16) return &kCorrForms[kCorrTiled];
  if (t32 * nw <= 256) return &kCorrForms[kCorrDmaRows1];
  if (W < 32) return &kCorrForms[kCorrTiled];
  if (t32 * ((nw + 1) / 2) <= 256) return &kCorrForms[kCorrDmaRows2];
  return &kCorrForms[t32 >= 400 ? kCorrDma1 : (t32 >= 128 ? kCorrDma2 : kCorrDma3)];
}

// Cache policy of a kernel's output stores (mfn_rt.h: mfn_store4_stream), from measurements of every kernel INSIDE the
// pass (bench.py --tuning store_dc=..,store_corr=.., `kernels` and `roofline`): cost volumes of 4 MB and more are written
// through (level 2: 17.4 -> 15.6 us inside the pass, 17-21 -> 14.8 us back to back; level 3: 12.4 -> 11.6 us); the
// deformable conv's output stays plain because the next kernel reads it on the same XCD; smaller outputs and the
// latency-bound coarse levels lose a little with any policy.
static int store_policy_for(const Settings &st, size_t out_bytes, int preferred, int family_override, size_t below = (size_t)-1) {
  if (family_override >= 0) return family_override;
  if (st.t.store_policy >= 0) return st.t.store_policy;
  return (out_bytes >= ((size_t)4 << 20) && out_bytes < below) ? preferred : 0;
}

// aligned16 (f1, f2, out and the distance between output images allow 16-byte accesses) and ws_bytes (of a 16-byte aligned workspace,
// 0 = none) are what only the run knows; a size query plans an aligned call that brings all the workspace the plan wants.
static CorrPlan corr_plan(const Settings &st, int N, int C, int H, int W, int md, int kernel, int s1, int s2, int pad, int is_multiply,
                          bool aligned16 = true, size_t ws_bytes = (size_t)-1) {
  CorrPlan pl;
  memset(&pl, 0, sizeof(pl));
  pl.family = CorrFamily::Generic;
  pl.D = 2 * (md / s2) + 1;
  const int D = pl.D;
  if ((st.t.path_generic & 1) || kernel != 1 || s1 != 1 || s2 != 1 || pad != md || !is_multiply || (D != 9 && D != 5) || W % 4 != 0 ||
      !aligned16)
    return pl;
  const size_t out_elems = (size_t)N * D * D * H * W;   // pad == md, stride 1: one output pixel per input pixel
  const CorrForm *form = corr_form(st.t.corr_variant);   // nullptr: the library chooses
  const bool chosen = form == nullptr;
  const CorrForm *gramk = chosen ? corr_gramk_plan(N, C, H, W, st) : nullptr;
  // the tiniest levels (level 6): direct kernel, L1/L2-resident operands, channel slices inside the block
  if (corr_direct_shape_ok(W, D) && (st.t.corr_direct == 1 || (st.t.corr_direct == 0 && (long)H * W < 180 && chosen && !gramk))) {
    pl.family = CorrFamily::Direct;
    pl.store_policy = store_policy_for(st, out_elems * 4, 2, -1);
    return pl;
  }
  if (chosen) form = gramk ? gramk : corr_tile_form(N, H, W, D);
  if (chosen && !gramk && C == 32 && W % 8 == 0 && form == &kCorrForms[kCorrDma1]) {
    // level 2 (32 channels, >= 400 tiles): the Gram band on the matrix cores.  Same box, same session (profiles/
    // r04_corr_gram_experiments.md section 7): level 2 of 384x512 at batch 8 back to back 10.45 against 13.2 us, rocprofv3 average
    // 12.65 against 15.6 us, inside the pass 12.3-12.5 us = 0.57-0.58 of 8 TB/s against 14.2 us = 0.50; 448x1024 at batch 4 13.7
    // against 17.6 us; on buffers rotated through more than the Infinity Cache a tie (17.95 against 17.3-17.8 us).
    // Under MFN_ARITH_FP32 the same band on the fp32 matrix instruction (form 46: raw operands, an fmaf chain over the channels
    // in order, bitwise): 12.5 us against corr_dma_kernel's 14.0 back to back (corr.form = 16 keeps the latter)
    const CorrForm *asked = corr_form(st.t.corr_form);
    if (st.corr != 0) form = asked && asked->family == CorrFamily::Gram ? asked : &kCorrForms[kCorrGramBf16];
    else if (asked != &kCorrForms[kCorrDma1]) form = &kCorrForms[kCorrGramF32];
  }
  // level 3 (64 channels, 128-399 tiles): the same band with a two-chunk K loop (form 48 only; corr.form = 20 keeps corr_dma_kernel's
  // two channel groups: 9.95 -> 8.30 us back to back at 384x512 / batch 8, 10.04 -> 8.37 at 448x1024 / batch 4, profiles/r06_corr_l3.txt)
  if (chosen && !gramk && C == 64 && W % 8 == 0 && form == &kCorrForms[kCorrDma2] && st.corr != 0 &&
      corr_form(st.t.corr_form) != &kCorrForms[kCorrDma2])
    form = &kCorrForms[kCorrGramBf16];
  pl.form = form;
  if (form->family == CorrFamily::Gram) {   // its own tiling, no channel slices; 64 channels: the bf16 form's two-chunk K loop only
    pl.rows = corr_gram_rows(N, H, W, st.t.corr_rows, C);
    if ((C == 32 || (C == 64 && form->terms == 5 && W % 8 == 0)) && corr_gram_range_ok(N, H, W, pl.rows)) {
      pl.family = CorrFamily::Gram;
      pl.store_policy = store_policy_for(st, out_elems * 4, 2, -1);
      return pl;
    }
  }
  if (form->family == CorrFamily::GramK && corr_gramk_shape_ok(C, W)) {   // coarse levels: channels over the waves of a block
    pl.family = CorrFamily::GramK;
    pl.store_policy = st.t.store_policy >= 0 ? st.t.store_policy : 0;
    return pl;
  }
  if (form->family != CorrFamily::Tiled && form->family != CorrFamily::Dma)   // asked for, but not a level that kernel takes
    form = corr_tile_form(N, H, W, D);
  if (W < 32 && !(form->row_pairs && W >= 16)) form = &kCorrForms[kCorrTiled];   // the 32x4-tile kernels want full-width tiles
  else if (form->family == CorrFamily::Tiled) form = &kCorrForms[kCorrDma1];      // corr_tiled_kernel only runs below 32 columns
  pl.form = form;
  pl.family = form->family;
  pl.tile_w = form->family == CorrFamily::Dma ? 32 : (W >= 16 ? 16 : 8);
  pl.tile_h = form->family == CorrFamily::Dma ? 4 : 256 / pl.tile_w;
  const long tiles = (long)N * cdiv(W, pl.tile_w) * cdiv(H, pl.tile_h);
  int slices = 1;  // few tiles, many channels: split channels until every CU has a block
  if (tiles < 128 && form->groups == 1)  // the grouped tile kernels split the channels inside the block instead
    while (tiles * slices < 256 && C / (slices * 2) >= 8 && slices < 32) slices *= 2;
  if (slices > C / 4) slices = C / 4 > 0 ? C / 4 : 1;
  if (slices > 1 && ws_bytes < (size_t)slices * out_elems * sizeof(float))
    slices = 1;  // no (or too small a) workspace: single pass over all channels, still correct
  pl.slices = slices;
  pl.ws_bytes = slices > 1 ? (size_t)slices * out_elems * sizeof(float) : 0;
  pl.store_policy = store_policy_for(st, out_elems * 4, 2, -1);
  return pl;
}

size_t MFN_API(correlation_workspace_bytes)(int N, int C, int H, int W, int md, int kernel, int s1, int s2, int pad,
                                            int is_multiply) {
  if (N <= 0 || C <= 0 || corr_shape(H, W, md, kernel, s1, s2, pad, nullptr, nullptr, nullptr)) return 0;
  return corr_plan(settings_now(), N, C, H, W, md, kernel, s1, s2, pad, is_multiply).ws_bytes;
}

static int corr_fwd_common(const Settings &st, const float *d1, const float *d2, float *out, int N, int C, int H, int W, int md, int kernel,
                           int s1, int s2, int pad, int is_multiply, int act, void *workspace, size_t ws_bytes,
                           void *stream, long long out_batch_stride = 0) {
  if (N != 0 && (!d1 || !d2 || !out)) return fail(MFN_E_NULL, "correlation_fwd: NULL tensor pointer");
  if (act != 0 && act != 1) return fail(MFN_E_PARAM, "correlation_fwd: activation must be MFN_ACT_NONE or MFN_ACT_LEAKY_0_1");
  if (N < 0 || C <= 0) return fail(MFN_E_SHAPE, "correlation_fwd: N=%d C=%d", N, C);
  int tc, th, tw;
  int rc = corr_shape(H, W, md, kernel, s1, s2, pad, &tc, &th, &tw);
  if (rc) return rc;
  if (!aligned(d1, 4) || !aligned(d2, 4) || !aligned(out, 4)) return fail(MFN_E_ALIGN, "correlation_fwd: unaligned pointer");
  const int r = md / s2;
  // MXNet reads the padded temporaries unchecked: the displaced window must stay inside them
  if ((th - 1) * s1 + md + r * s2 + kernel - 1 >= H + 2 * pad || (tw - 1) * s1 + md + r * s2 + kernel - 1 >= W + 2 * pad ||
      md - r * s2 < 0)
    return fail(MFN_E_PARAM, "correlation_fwd: displaced window leaves the padded input (pad_size=%d < max_displacement=%d?)", pad, md);
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  // out may be a channel slice of a wider (N, Ctot, h, w) buffer: images then sit out_batch_stride elements apart
  const size_t img_elems = (size_t)tc * th * tw;
  if (out_batch_stride != 0 && (out_batch_stride < 0 || (size_t)out_batch_stride < img_elems))
    return fail(MFN_E_PARAM, "correlation_fwd: out_batch_stride=%lld is smaller than one image of the output (%zu)",
                out_batch_stride, img_elems);
  const size_t onst = out_batch_stride ? (size_t)out_batch_stride : img_elems;
  const CorrPlan pl = corr_plan(st, N, C, H, W, md, kernel, s1, s2, pad, is_multiply,
                                aligned(d1, 16) && aligned(d2, 16) && aligned(out, 16) && onst % 4 == 0,
                                workspace && aligned(workspace, 16) ? ws_bytes : 0);
  const bool d9 = pl.D == 9;
  switch (pl.family) {
    case CorrFamily::Generic: {
      CorrGenericParams g{d1, d2, out, N, C, H, W, md, kernel, s1, s2, pad, is_multiply ? 1 : 0, tc, th, tw, r, pl.D, act, onst};
      return hipfail(corr_generic_launch(g, s), "correlation_fwd(generic)");
    }
    case CorrFamily::Direct: {
      CorrDirectParams dp;
      memset(&dp, 0, sizeof(dp));
      dp.f1 = d1; dp.f2 = d2; dp.out = out; dp.out_nstride = onst; dp.st_policy = pl.store_policy;
      dp.N = N; dp.C = C; dp.H = H; dp.W = W;
      dp.sumelems = (float)C;
      dp.inv_sumelems = 1.0f / (float)C;
      dp.exact_div = (C & (C - 1)) != 0;
      dp.leaky = act;
      dp.max_slices = 32;  // measured: 7.9 us at level 6 (8x196x6x8) against 9.2 us with 49 four-channel slices
      return hipfail(d9 ? corr_direct_launch<9>(dp, s) : corr_direct_launch<5>(dp, s), "correlation_fwd(direct)");
    }
    case CorrFamily::Gram: {
      CorrGramParams gp;
      memset(&gp, 0, sizeof(gp));
      gp.f1 = d1; gp.f2 = d2; gp.out = out; gp.out_nstride = onst;
      gp.N = N; gp.H = H; gp.W = W; gp.C = C;
      gp.rows = pl.rows;
      gp.store_policy = pl.store_policy;   // full lines, written through like every other cost volume >= 4 MB
      gp.leaky = act;
      gp.xcd_swizzle = 1;
      gp.inv_c = 1.0f / (float)C;
      gp.timeline = (unsigned long long *)g_timeline;
      return hipfail(d9 ? corr_gram_form<9>(gp, *pl.form, s) : corr_gram_form<5>(gp, *pl.form, s), "correlation_fwd(gram)");
    }
    case CorrFamily::GramK: {
      CorrGramKParams kp;
      memset(&kp, 0, sizeof(kp));
      kp.f1 = d1; kp.f2 = d2; kp.out = out; kp.out_nstride = onst;
      kp.N = N; kp.C = C; kp.H = H; kp.W = W;
      kp.store_policy = pl.store_policy;
      kp.leaky = act;
      kp.xcd_swizzle = 1;
      kp.sumelems = (float)C;
      kp.inv_sumelems = 1.0f / (float)C;
      kp.exact_div = (C & (C - 1)) != 0;
      return hipfail(d9 ? corr_gramk_form<9>(kp, *pl.form, s) : corr_gramk_form<5>(kp, *pl.form, s), "correlation_fwd(gramk)");
    }
    default: break;   // Tiled / Dma
  }
  CorrParams p;
  p.f1 = d1; p.f2 = d2; p.out = out; p.out_nstride = onst;
  p.N = N; p.C = C; p.H = H; p.W = W;
  p.tiles_x = p.tiles_y = 0;
  p.sumelems = (float)C;
  p.inv_sumelems = 1.0f / (float)C;
  p.exact_div = (C & (C - 1)) != 0;  // 1/C is exact only for powers of two
  p.xcd_swizzle = 1;
  p.nt_store = pl.store_policy;
  p.leaky = act;
  p.timeline = (unsigned long long *)g_timeline;
  p.nslices = pl.slices;
  p.slice_channels = pl.slices > 1 ? ((cdiv(C, pl.slices) + 3) / 4) * 4 : C;
  p.partial = (float *)workspace;
  rc = d9 ? corr_tile_launch<9>(p, pl, s) : corr_tile_launch<5>(p, pl, s);
  if (rc) return hipfail(rc, "correlation_fwd");
  if (pl.slices > 1) {
    CorrReduceParams rp{(const float *)workspace, out, (size_t)N * img_elems / 4, pl.slices, p.inv_sumelems, p.sumelems, p.exact_div, act,
                        img_elems / 4, onst / 4};
    rc = corr_reduce_launch(rp, s);
  }
  return hipfail(rc, "correlation_fwd");
}

int MFN_API(correlation_fwd_ws)(const float *d1, const float *d2, float *out, int N, int C, int H, int W, int md,
                                int kernel, int s1, int s2, int pad, int is_multiply, void *workspace,
                                size_t ws_bytes, void *stream) {
  return corr_fwd_common(settings_now(), d1, d2, out, N, C, H, W, md, kernel, s1, s2, pad, is_multiply, 0, workspace, ws_bytes, stream);
}

int MFN_API(correlation_fwd_act)(const float *d1, const float *d2, float *out, int N, int C, int H, int W, int md,
                                 int kernel, int s1, int s2, int pad, int is_multiply, int activation, void *workspace,
                                 size_t ws_bytes, void *stream) {
  return corr_fwd_common(settings_now(), d1, d2, out, N, C, H, W, md, kernel, s1, s2, pad, is_multiply, activation, workspace, ws_bytes,
                         stream);
}

int MFN_API(correlation_fwd_into)(const float *d1, const float *d2, float *out, long long out_batch_stride, int N, int C,
                                  int H, int W, int md, int kernel, int s1, int s2, int pad, int is_multiply,
                                  int activation, void *workspace, size_t ws_bytes, void *stream) {
  return corr_fwd_common(settings_now(), d1, d2, out, N, C, H, W, md, kernel, s1, s2, pad, is_multiply, activation, workspace, ws_bytes,
                         stream, out_batch_stride);
}

int MFN_API(correlation_fwd)(const float *d1, const float *d2, float *out, int N, int C, int H, int W, int md,
                             int kernel, int s1, int s2, int pad, int is_multiply, void *stream) {
  return corr_fwd_common(settings_now(), d1, d2, out, N, C, H, W, md, kernel, s1, s2, pad, is_multiply, 0, nullptr, 0, stream);
}

// ---- warp -------------------------------------------------------------------------------------------
int MFN_API(warp_fwd)(const float *x, const float *flow, float *out, int N, int C, int H, int W, int clip,
                      void *stream) {
  if (N != 0 && (!x || !flow || !out)) return fail(MFN_E_NULL, "warp_fwd: NULL tensor pointer");
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "warp_fwd: N=%d C=%d H=%d W=%d", N, C, H, W);
  if (!aligned(x, 4) || !aligned(flow, 4) || !aligned(out, 4)) return fail(MFN_E_ALIGN, "warp_fwd: unaligned pointer");
  if (N == 0) return 0;
  WarpParams p{x, flow, out, N, C, H, W, clip ? 1 : 0, store_policy_for(settings_now(), (size_t)N * C * H * W * 4, 1, -1)};
  return hipfail(warp_fwd_launch(p, (hipStream_t)stream), "warp_fwd");
}

int MFN_API(grid_generator_warp)(const float *flow_xy, float *grid, int N, int H, int W, void *stream) {
  if (N != 0 && (!flow_xy || !grid)) return fail(MFN_E_NULL, "grid_generator_warp: NULL tensor pointer");
  if (N < 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "grid_generator_warp: N=%d H=%d W=%d", N, H, W);
  GridWarpParams p{flow_xy, grid, N, H, W};
  return hipfail(grid_warp_launch(p, (hipStream_t)stream), "grid_generator_warp");
}

int MFN_API(grid_generator_affine)(const float *theta, float *grid, int N, int H, int W, void *stream) {
  if (N != 0 && (!theta || !grid)) return fail(MFN_E_NULL, "grid_generator_affine: NULL tensor pointer");
  if (N < 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "grid_generator_affine: N=%d H=%d W=%d", N, H, W);
  GridAffineParams p{theta, grid, N, H, W};
  return hipfail(grid_affine_launch(p, (hipStream_t)stream), "grid_generator_affine");
}

int MFN_API(bilinear_sampler_fwd)(const float *data, const float *grid, float *out, int N, int C, int iH, int iW,
                                  int oH, int oW, void *stream) {
  if (N != 0 && (!data || !grid || !out)) return fail(MFN_E_NULL, "bilinear_sampler_fwd: NULL tensor pointer");
  if (N < 0 || C <= 0 || iH <= 0 || iW <= 0 || oH <= 0 || oW <= 0)
    return fail(MFN_E_SHAPE, "bilinear_sampler_fwd: bad shape");
  SamplerParams p{data, grid, out, N, C, iH, iW, oH, oW};
  return hipfail(bilinear_sampler_launch(p, (hipStream_t)stream), "bilinear_sampler_fwd");
}

// ---- deformable convolution -----------------------------------------------------------------------------
int MFN_API(deform_conv_out_shape)(int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                   int *Ho, int *Wo) {
  if (H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "deform_conv: H=%d W=%d must be positive", H, W);
  if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || dh < 1 || dw < 1)
    return fail(MFN_E_PARAM, "deform_conv: bad kernel/stride/pad/dilate");
  const int ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
  const int wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
  if (H + 2 * ph < dh * (kh - 1) + 1 || W + 2 * pw < dw * (kw - 1) + 1 || ho < 1 || wo < 1)
    return fail(MFN_E_SHAPE, "deform_conv: kernel size exceed input");
  if (Ho) *Ho = ho;
  if (Wo) *Wo = wo;
  return 0;
}

static bool dc_mfma_ok(const Settings &st, int kh, int kw, int groups, int dg) {
  return (st.t.path_generic & 2) == 0 && kh == 3 && kw == 3 && groups == 1 && dg == 1;
}

// ---- launch plan of the MFMA path: tiling, K split and workspace layout -----------------------------------
struct DcPlan {
  int mt, pt, nw, ksb, mgroups, ncp_pad, cps_per_slice;
  int mma;   // 0: exact fp32 (dc_lds_kernel); 2: the bf16 x 3 matrix-core kernel (dc_mma_kernel, deform_conv_mma.h)
  int kw, ring, groups, gps;   // mma == 2: K slices per pixel tile, window ring depth, 16-channel groups (per slice)
  int areg;   // mma == 2: the weight operand from memory to registers (dc_mma_kernel's AREG form) instead of through LDS
  int tile_w, tiles_x, tiles_y, ntiles;
  size_t wt_bytes, partial_bytes, mg_words;
};
// the (filter tiles per wave, pixel tiles per block, K slices) the library has dc_mma_kernel instantiated for
#ifndef MFN_DCM_CONFIGS   // measurement builds instantiate fewer
#define MFN_DCM_CONFIGS(X) X(1, 4, 1) X(2, 3, 4) X(2, 2, 2) X(3, 1, 6) X(1, 1, 8) X(1, 1, 4) X(1, 1, 2) X(1, 1, 1)
#endif
// ... and those it has the AREG form of (the tilings the plan gives the network's four levels)
#ifndef MFN_DCM_AREG_CONFIGS
#define MFN_DCM_AREG_CONFIGS(X) X(1, 4, 1) X(3, 1, 6) X(1, 1, 8)
#endif
static bool dcm_areg_config_ok(int mt, int pt, int kw) {
#define X(a, b, c) if (mt == a && pt == b && kw == c) return true;
  MFN_DCM_AREG_CONFIGS(X)
#undef X
  return false;
}
static bool dcm_config_ok(int mt, int pt, int kw) {
#define X(a, b, c) if (mt == a && pt == b && kw == c) return true;
  MFN_DCM_CONFIGS(X)
#undef X
  return false;
}
// mma_shape: the call has the operator shape dc_mma_kernel takes (dcm_shape_ok)
static DcPlan dc_plan(const Settings &st, int Cin, int Cout, int N, int Ho, int Wo, bool mma_shape) {
  DcPlan pl;
  memset(&pl, 0, sizeof(pl));
  const long P = (long)N * Ho * Wo;
  const int mtiles = (Cout + 31) / 32;
  int mt = 1;  // one 32-filter tile per wave, the filter tiles spread over workgroups (blockIdx.z)
  // 32-pixel tiles: 4x8 (default) or 2x16 output pixels (small source windows), or 32 consecutive flattened
  // pixels for images narrower than 8 columns
  pl.tile_w = Wo >= 8 ? 8 : 0;
  if (pl.tile_w) {
    pl.tiles_x = (Wo + pl.tile_w - 1) / pl.tile_w;
    pl.tiles_y = (Ho + 32 / pl.tile_w - 1) / (32 / pl.tile_w);
    pl.ntiles = N * pl.tiles_y * pl.tiles_x;
  } else {
    pl.tiles_x = pl.tiles_y = 0;
    pl.ntiles = (int)((P + 31) / 32);
  }
  const long tiles = pl.ntiles;
  if (mma_shape && st.deform != 0) {
    // ---- dc_mma_kernel: B operands shared by the MT filter tiles of a wave; K slices in whole 16-channel groups ----
    pl.mma = 2;
    pl.groups = Cin / 16;
    pl.ring = 3;
    // measured per level of the 384x512 batch-8 pass (profiles/r05_dcm_sweep.txt): level 2 three 4-wave blocks per CU in one round
    // (1, 4, 1); level 3 (two filter tiles) 256 blocks of 12 waves, the three pixel tiles of a K slice sharing its weights (2, 3, 4);
    // level 4 all three filter tiles in the wave, six one-group K slices (3, 1, 6); level 5 eight K slices, the filter tiles over
    // workgroups (1, 1, 8).  Anything else: one pixel tile, as many one-group K slices as divide the groups.
    int cmt = 1, cpt = 1, ckw = pl.groups % 8 == 0 ? 8 : (pl.groups % 4 == 0 ? 4 : (pl.groups % 2 == 0 ? 2 : 1));
    if (mtiles == 1 && tiles >= 1024) { cpt = 4; ckw = 1; }
    else if (mtiles == 2 && tiles >= 384 && pl.groups % 4 == 0) {
      cmt = 2; cpt = 3; ckw = 4;
      // 12-wave blocks: one per CU.  More than 256 of them (448x1024 at batch 4: 299) run in two rounds -- 30.9 us at level 3 against
      // 18 for the 256 blocks of 384x512.  Then 4-wave blocks of two pixel tiles x two K slices, two per CU (six-wave blocks do not
      // pair up: their waves land 2-2-1-1 on the SIMDs and a second block finds no room -- measured 34.1 us)
      if ((tiles + 2) / 3 > 256 && (tiles + 1) / 2 <= 512) { cpt = 2; ckw = 2; }
    }
    else if (mtiles == 3 && pl.groups % 6 == 0) { cmt = 3; ckw = 6; }
    else if (tiles >= 1024) { cpt = 4; ckw = 1; }
    if (st.t.dc_mt > 0 && st.t.dc_pt > 0 && st.t.dc_nw > 0) {     // measurement: an explicit (mt, pt, waves per block)
      cmt = st.t.dc_mt; cpt = st.t.dc_pt; ckw = st.t.dc_nw / (cpt > 0 ? cpt : 1);
    }
    if (!dcm_config_ok(cmt, cpt, ckw) || pl.groups % ckw != 0 || cmt > mtiles) { cmt = 1; cpt = 1; ckw = 1; }
    pl.mt = cmt; pl.pt = cpt; pl.kw = ckw; pl.nw = cpt * ckw; pl.ksb = 1;
    // the weight operand from memory to registers wherever that form exists: it won at each of its tilings
    // (profiles/dc_mma_a_operand.md).  dc.off bit 4 forces the LDS form (A/B runs and tests; the packed layout is the same); a
    // tiling without the form keeps the LDS kernel whatever the bits say
    pl.areg = dcm_areg_config_ok(cmt, cpt, ckw) && !(st.t.dc_off & 4);
    pl.mgroups = (mtiles + cmt - 1) / cmt;
    pl.gps = pl.groups / ckw;
    pl.mg_words = (size_t)(pl.groups * 9 + dcm_kc(cmt, ckw)) * (3 * cmt * 256);
    pl.wt_bytes = (pl.mgroups * pl.mg_words * sizeof(float) + 255) / 256 * 256;
    pl.partial_bytes = 0;
    return pl;
  }
  // sweep r01 (tools/sweep_dc.py): one 32-filter tile per wave and the filter tiles spread over workgroups wins at
  // every level -- fp32 MFMA and VALU share the same ALUs on gfx950, so what counts is resident waves, and a
  // (1, pt) block needs the fewest registers.
  pl.mt = mt;
  pl.mma = 0;
  pl.mgroups = (mtiles + mt - 1) / mt;
  const int ncp = (Cin + 1) / 2;
  int pt = st.t.dc_pt;
  if (!(pt == 1 || pt == 2 || pt == 4)) {
    // cycles of the slowest SIMD: residency rounds (3 blocks of 4 waves per CU) x [channel pairs per wave x (576 MFMA +
    // ~170 VALU) + setup + epilogue] -- the measured per-block phases (profiles/r01b_deform_pmc_and_timelines.md);
    // ties go to more pixel tiles per block (they share a weight stage)
    double best = 1e30;
    pt = 1;
    for (int cand = 1; cand <= 4; cand <<= 1) {
      const double blocks = (double)((tiles + cand - 1) / cand) * pl.mgroups;
      const double rounds = blocks <= 768.0 ? 1.0 : (double)(long)((blocks + 767.0) / 768.0);
      const double pairs = (double)ncp * cand / 4.0;
      const double cost = rounds * (pairs * 745.0 + 10700.0);
      if (cost <= best) { best = cost; pt = cand; }
    }
  }
  pl.pt = pt;
  // 8-wave blocks (twice the in-block K slices) where the whole launch is at most one block per CU and every wave still
  // gets a few channel pairs: the coarsest level (192 blocks, 64 pairs) is a latency chain per wave, not a throughput job
  int nw = st.t.dc_nw;
  if (nw != 4 && nw != 8) nw = (mt == 1 && pt == 1 && ((tiles + pt - 1) / pt) * pl.mgroups <= 256 && ncp >= 32) ? 8 : 4;
  if (nw == 8 && !(mt == 1 && pt == 1)) nw = 4;  // the only 8-wave instantiation
  pl.nw = nw;
  const int kw = nw / pt, kc = dc_kc(mt, kw);
  int ksb = st.t.dc_ksb;
  if (ksb <= 0) {  // few pixel tiles (coarse levels): split K across workgroups until the chip is covered
    ksb = 1;
    const long blocks0 = ((tiles + pt - 1) / pt) * pl.mgroups;
    while (blocks0 * ksb < 64 && ncp / (kw * ksb * 2) >= 2 * kc && ksb < 16) ksb *= 2;
  }
  pl.ksb = ksb;
  const int S = kw * ksb;
  pl.cps_per_slice = (((ncp + S - 1) / S + kc - 1) / kc) * kc;
  pl.ncp_pad = S * pl.cps_per_slice + kc;
  pl.wt_bytes = (((size_t)pl.mgroups * pl.ncp_pad * (18 * 32 * mt) * sizeof(float)) + 255) / 256 * 256;
  pl.partial_bytes = ksb > 1 ? (size_t)ksb * Cout * P * sizeof(float) : 0;
  return pl;
}
// does this call have the operator shape of dc_mma_kernel?  (the tensors' alignment is checked at the launch: the size queries
// cannot know it, and an unaligned call falls back to the exact kernel with the layout it was packed for refused loudly)
static bool dc_mma_shape(int N, int Cin, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int dg) {
  int Ho = 0, Wo = 0;
  if (N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1 || ph < 0 || pw < 0) return false;
  Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
  Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
  return dcm_shape_ok(N, Cin, H, W, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg);
}

// what a packed filter bank depends on; handed to the caller by pack_weights and checked by the *_packed calls
static unsigned long long dc_layout_tag(const DcPlan &pl) {
  if (pl.mma == 2)   // [mg][group][step][term][filter tile]: the tiles per wave, the M-groups and the padding (one chunk: mt, kw) decide it
    return 0x4d46000000000000ull | (2ull << 44) | ((unsigned long long)pl.mt << 40) | ((unsigned long long)pl.mgroups << 32) |
           ((unsigned long long)dcm_kc(pl.mt, pl.kw) << 24) | (unsigned long long)(unsigned)pl.groups;
  return 0x4d46000000000000ull | ((unsigned long long)pl.mma << 44) | ((unsigned long long)pl.mt << 40) | ((unsigned long long)pl.mgroups << 32) |
         (unsigned long long)(unsigned)pl.ncp_pad;
}
static const unsigned long long kDcPlainTag = 0x4d46ffff00000000ull;  // plain copy of w (shapes the MFMA path skips)

// the filter bank in the layout of the plan's kernel
static int dc_pack(const DcPlan &pl, const float *w, float *packed, int Cin, int Cout, hipStream_t s) {
  if (pl.mma == 2) return dcm_pack_launch(DcmPackParams{w, packed, Cin, Cout, pl.mt, pl.mgroups, pl.groups, pl.mg_words}, s);
  PackParams pp{w, packed, Cin, Cout, 32 * pl.mt, pl.mgroups, pl.ncp_pad, 9};
  return dc_pack_launch(pp, s);
}

size_t MFN_API(deform_conv_workspace_bytes)(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw,
                                            int ph, int pw, int dh, int dw, int groups, int deform_groups) {
  const Settings st = settings_now();
  (void)groups; (void)deform_groups;
  int Ho, Wo;
  if (N <= 0 || Cin <= 0 || Cout <= 0 || MFN_API(deform_conv_out_shape)(H, W, kh, kw, sh, sw, ph, pw, dh, dw, &Ho, &Wo))
    return 0;
  if (!dc_mfma_ok(st, kh, kw, groups, deform_groups)) return 0;  // generic kernel needs no workspace
  // the larger of the two plans: a call whose x / out are not 16-byte aligned (a view at an odd offset) cannot take the matrix-core
  // kernel and runs the fp32 kernel's plan instead (dc_run), with the same workspace
  const bool mma = dc_mma_shape(N, Cin, H, W, kh, kw, sh, sw, ph, pw, dh, dw, groups, deform_groups);
  const DcPlan pl = dc_plan(st, Cin, Cout, N, Ho, Wo, mma);
  size_t need = pl.wt_bytes + pl.partial_bytes;
  if (mma) {
    const DcPlan alt = dc_plan(st, Cin, Cout, N, Ho, Wo, false);
    if (alt.wt_bytes + alt.partial_bytes > need) need = alt.wt_bytes + alt.partial_bytes;
  }
  return need;
}

static size_t dc_packed_bytes(const Settings &st, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                              int dh, int dw, int groups, int deform_groups) {
  int Ho, Wo;
  if (N <= 0 || Cin <= 0 || Cout <= 0 || groups < 1 || Cin % groups ||
      MFN_API(deform_conv_out_shape)(H, W, kh, kw, sh, sw, ph, pw, dh, dw, &Ho, &Wo))
    return 0;
  if (!dc_mfma_ok(st, kh, kw, groups, deform_groups)) return (size_t)Cout * (Cin / groups) * kh * kw * sizeof(float);
  return dc_plan(st, Cin, Cout, N, Ho, Wo, dc_mma_shape(N, Cin, H, W, kh, kw, sh, sw, ph, pw, dh, dw, groups, deform_groups)).wt_bytes;
}
size_t MFN_API(deform_conv_packed_weight_bytes)(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw,
                                                int ph, int pw, int dh, int dw, int groups, int deform_groups) {
  return dc_packed_bytes(settings_now(), N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, deform_groups);
}

int MFN_API(deform_conv_pack_weights)(const float *w, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh,
                                      int sw, int ph, int pw, int dh, int dw, int groups, int deform_groups,
                                      void *packed, size_t packed_bytes, unsigned long long *layout_tag,
                                      void *stream) {
  const Settings st = settings_now();
  if (!w || !packed || !layout_tag) return fail(MFN_E_NULL, "deform_conv_pack_weights: NULL pointer");
  const size_t need = dc_packed_bytes(st, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, deform_groups);
  if (!need) return fail(MFN_E_SHAPE, "deform_conv_pack_weights: bad shape");
  if (packed_bytes < need) return fail(MFN_E_WORKSPACE, "deform_conv_pack_weights: %zu bytes required (got %zu)", need, packed_bytes);
  if (!aligned(packed, 16)) return fail(MFN_E_ALIGN, "deform_conv_pack_weights: packed buffer must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (!dc_mfma_ok(st, kh, kw, groups, deform_groups)) {
    *layout_tag = kDcPlainTag;
    return hipfail(dc_copy_launch(w, (float *)packed, need / sizeof(float), s), "deform_conv_pack_weights");
  }
  int Ho, Wo;
  MFN_API(deform_conv_out_shape)(H, W, kh, kw, sh, sw, ph, pw, dh, dw, &Ho, &Wo);
  const DcPlan pl = dc_plan(st, Cin, Cout, N, Ho, Wo, dc_mma_shape(N, Cin, H, W, kh, kw, sh, sw, ph, pw, dh, dw, groups, deform_groups));
  *layout_tag = dc_layout_tag(pl);
  return hipfail(dc_pack(pl, w, (float *)packed, Cin, Cout, s), "deform_conv_pack_weights");
}

// packed == nullptr: stateless operator call, the filter bank is re-packed into the head of the workspace
// (MXNet hands the operator its weights on every call).  packed != nullptr: the caller packed it once with
// mfn_deform_conv_pack_weights (inference: weights are constants) and the workspace only holds partial sums.
static int dc_run(const Settings &st, DeformParams &p, const void *packed, size_t packed_bytes, unsigned long long tag, void *workspace,
                  size_t ws_bytes, hipStream_t s, const char *what) {
  if (!dc_mfma_ok(st, p.kh, p.kw, p.groups, p.dg)) {
    if (packed) {  // plain copy of w for shapes the MFMA path does not take
      if (tag != kDcPlainTag)
        return fail(MFN_E_WORKSPACE, "%s: packed weights were laid out under another tuning (re-run mfn_deform_conv_pack_weights)", what);
      p.w = (const float *)packed;
    }
    return hipfail(dc_generic_launch(p, s), what);
  }
  // The matrix-core kernel moves 16 bytes per lane: x and out have to be 16-byte aligned.  A call that hands raw weights (the
  // operator's signature) and tensors at an odd offset -- a view -- takes the fp32 kernel's plan instead, BEFORE anything is packed;
  // weights packed for the matrix-core layout cannot follow and are refused below (MFN_E_ALIGN).
  bool mma_shape = dcm_shape_ok(p.N, p.Cin, p.H, p.W, p.Ho, p.Wo, p.kh, p.kw, p.sh, p.sw, p.ph, p.pw, p.dh, p.dw, p.groups, p.dg);
  if (mma_shape && !packed && (!aligned(p.x, 16) || !aligned(p.out, 16))) mma_shape = false;
  const DcPlan pl = dc_plan(st, p.Cin, p.Cout, p.N, p.Ho, p.Wo, mma_shape);
  const size_t need = (packed ? 0 : pl.wt_bytes) + pl.partial_bytes;
  if (need && (!workspace || ws_bytes < need))
    return fail(MFN_E_WORKSPACE, "%s: workspace of %zu bytes required (got %zu)", what, need, workspace ? ws_bytes : (size_t)0);
  if (need && !aligned(workspace, 16)) return fail(MFN_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  int rc;
  char *partial_base = (char *)workspace;
  if (packed) {
    if (packed_bytes < pl.wt_bytes || tag != dc_layout_tag(pl))
      return fail(MFN_E_WORKSPACE, "%s: packed weights (%zu bytes, layout %llx) do not match this shape/tuning (%zu bytes, layout %llx): "
                  "re-run mfn_deform_conv_pack_weights", what, packed_bytes, tag, pl.wt_bytes, dc_layout_tag(pl));
    if (!aligned(packed, 16)) return fail(MFN_E_ALIGN, "%s: packed weights must be 16-byte aligned", what);
    p.wt = (const float *)packed;
  } else {
    rc = dc_pack(pl, p.w, (float *)workspace, p.Cin, p.Cout, s);
    if (rc) return hipfail(rc, what);
    p.wt = (const float *)workspace;
    partial_base += pl.wt_bytes;
  }
  p.allow_fast = (st.t.dc_off & 2) ? 0 : 1;
  p.timeline = (unsigned long long *)g_timeline;
  p.stage_window = (st.t.dc_off & 1) ? 0 : 1;
  {
    // blockIdx.x -> tile range per XCD: the dispatch order is x fastest, so with several filter groups (grid z) block
    // (x, z) still runs on XCD x % 8 as long as gridDim.x is a multiple of 8
    const int tiles_ = pl.tile_w ? pl.ntiles : cdiv(p.N * p.Ho * p.Wo, 32);
    const int gx_ = cdiv(tiles_, pl.pt);
    p.xcd = pl.ksb == 1 && (pl.mgroups == 1 || gx_ % 8 == 0);
  }
  // plain: the warped features are read next by the correlation of the same level, whose block order puts image k on the
  // same XCD as this kernel's -- written through (nt) they would leave that L2 (level-2 correlation +1 us inside the pass)
  p.st_policy = store_policy_for(st, (size_t)p.N * p.Cout * p.Ho * p.Wo * 4, 0, -1);
  p.vec_store = (p.Wo % 4 == 0) && aligned(p.out, 16) && aligned(workspace, 16) && pl.wt_bytes % 16 == 0;
  p.ncp_pad = pl.ncp_pad;
  p.cps_per_slice = pl.cps_per_slice;
  p.ksb = pl.ksb;
  p.mgroups = pl.mgroups;
  p.tile_w = pl.tile_w; p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.ntiles = pl.ntiles;
  p.inv_tpi = pl.tile_w ? 1.0f / (float)(pl.tiles_y * pl.tiles_x) : 0.f;
  p.inv_tiles_x = pl.tile_w ? 1.0f / (float)pl.tiles_x : 0.f;
  p.partial = pl.ksb > 1 ? (float *)partial_base : nullptr;
  rc = -1000;
  if (pl.mma == 2) {
    // rows of 16 bytes (W % 4 == 0 is part of the shape) at 16-byte aligned tensors: the window transfers and the stores are 16 bytes wide
    if (!aligned(p.x, 16) || !aligned(p.out, 16) || !aligned(p.wt, 16))
      return fail(MFN_E_ALIGN, "%s: x, out and the packed weights must be 16-byte aligned for the matrix-core layout these weights were packed in "
                  "(pass the raw weights, or pack under mfn_set_arithmetic(\"deformable_convolution\", MFN_ARITH_FP32))", what);
    p.dcm_groups = pl.groups;
    p.dcm_gps = pl.gps;
    p.xcd = pl.mgroups == 1 || cdiv(pl.ntiles, pl.pt) % 8 == 0;
    t_last_dc_plan[0] = pl.mt; t_last_dc_plan[1] = pl.pt; t_last_dc_plan[2] = pl.kw; t_last_dc_plan[3] = pl.areg;
#define X(a, b, c) else if (pl.areg && pl.mt == a && pl.pt == b && pl.kw == c) rc = dc_mma_launch<a, b, c, 3, false, true>(p, s);
    if (false) {}
    MFN_DCM_AREG_CONFIGS(X)
#undef X
#define X(a, b, c) else if (pl.mt == a && pl.pt == b && pl.kw == c) rc = dc_mma_launch<a, b, c, 3>(p, s);
    MFN_DCM_CONFIGS(X)
#undef X
    if (rc == -1000) return fail(MFN_E_UNSUPPORTED, "%s: no matrix-core kernel for mt=%d pt=%d kw=%d", what, pl.mt, pl.pt, pl.kw);
    return hipfail(rc, what);
  }
  if (pl.nw == 8) rc = dc_lds_launch<1, 1, 8>(p, s, "dc_lds");
  else if (pl.pt == 1) rc = dc_lds_launch<1, 1>(p, s, "dc_lds");
  else if (pl.pt == 2) rc = dc_lds_launch<1, 2>(p, s, "dc_lds");
  else if (pl.pt == 4) rc = dc_lds_launch<1, 4>(p, s, "dc_lds");
  if (rc == -1000) return fail(MFN_E_UNSUPPORTED, "%s: no kernel for mt=%d pt=%d", what, pl.mt, pl.pt);
  if (rc) return hipfail(rc, what);
  if (pl.ksb > 1) {
    DcReduceParams rp{p.partial, p.bias, p.out, (size_t)p.Cout * p.P, pl.ksb, p.Cout, (size_t)p.Ho * p.Wo,
                      p.ep_mask, p.ep_add, p.ep_leaky};
    rc = dc_reduce_launch(rp, s);
  }
  return hipfail(rc, what);
}

static int dc_check(const char *what, const void *x, const void *w, const void *out, int N, int Cin, int H, int W,
                    int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int dg,
                    int *Ho, int *Wo) {
  if (!w || (N != 0 && (!x || !out))) return fail(MFN_E_NULL, "%s: NULL tensor pointer", what);
  if (N < 0 || Cin <= 0 || Cout <= 0) return fail(MFN_E_SHAPE, "%s: N=%d Cin=%d Cout=%d", what, N, Cin, Cout);
  if (groups < 1 || dg < 1) return fail(MFN_E_PARAM, "%s: num_group=%d num_deformable_group=%d", what, groups, dg);
  if (Cin % groups) return fail(MFN_E_SHAPE, "%s: input num_filter must divide group size", what);
  if (Cout % groups) return fail(MFN_E_SHAPE, "%s: output num_filter must divide group size", what);
  if (Cin % dg) return fail(MFN_E_SHAPE, "%s: input num_filter must divide deformable group size", what);
  if ((size_t)H * W >= ((size_t)1 << 30) || (size_t)N * Cin * H * W >= ((size_t)1 << 31))
    return fail(MFN_E_UNSUPPORTED, "%s: input tensor too large for 32-bit element offsets", what);
  int rc = MFN_API(deform_conv_out_shape)(H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo);
  if (rc) return rc;
  if ((size_t)N * *Ho * *Wo >= ((size_t)1 << 31) - 64) return fail(MFN_E_UNSUPPORTED, "%s: too many output pixels", what);
  return 0;
}

static int dc_fwd_common(const Settings &st, const char *what, const float *x, const float *offset, const float *w, const void *packed,
                         size_t packed_bytes, unsigned long long tag, const float *bias, float *out, int N, int Cin, int H, int W, int Cout,
                         int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int dg,
                         void *workspace, size_t ws_bytes, void *stream) {
  int Ho, Wo;
  int rc = dc_check(what, x, packed ? packed : (const void *)w, out, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg, &Ho, &Wo);
  if (rc) return rc;
  if (N != 0 && !offset) return fail(MFN_E_NULL, "%s: NULL offset", what);
  if (N == 0) return 0;
  DeformParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.offset = offset; p.flow = nullptr; p.flow_scale = 1.f; p.flow_stride = 1.f;
  p.w = w; p.wt = nullptr; p.bias = bias; p.out = out;
  p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.CoutP = Cout; p.Ho = Ho; p.Wo = Wo;
  p.kh = kh; p.kw = kw; p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw; p.dh = dh; p.dw = dw;
  p.groups = groups; p.dg = dg; p.P = N * Ho * Wo; p.allow_fast = 1;
  return dc_run(st, p, packed, packed_bytes, tag, workspace, ws_bytes, (hipStream_t)stream, what);
}

static int dc_shared_common(const Settings &st, const char *what, const float *x, const float *flow, float flow_scale, float flow_stride,
                            const float *w, const void *packed, size_t packed_bytes, unsigned long long tag,
                            const float *bias, const float *ep_mask, const float *ep_add, int ep_act, float *out, int N, int Cin, int H, int W, int Cout, int kh, int kw, int ph, int pw, int dh, int dw,
                            int groups, void *workspace, size_t ws_bytes, void *stream) {
  int Ho, Wo;
  int rc = dc_check(what, x, packed ? packed : (const void *)w, out, N, Cin, H, W, Cout, kh, kw, 1, 1, ph, pw, dh, dw, groups, 1, &Ho, &Wo);
  if (rc) return rc;
  if (N != 0 && !flow) return fail(MFN_E_NULL, "%s: NULL flow", what);
  if (Ho != H || Wo != W)
    return fail(MFN_E_SHAPE, "%s: flow is sampled on the input grid, needs Ho==H and Wo==W (got %dx%d vs %dx%d)", what, Ho, Wo, H, W);
  if (flow_stride == 0.f) return fail(MFN_E_PARAM, "%s: flow_stride must be non-zero", what);
  if (N == 0) return 0;
  DeformParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.offset = nullptr; p.flow = flow; p.flow_scale = flow_scale; p.flow_stride = flow_stride;
  p.w = w; p.wt = nullptr; p.bias = bias; p.out = out;
  p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.CoutP = Cout; p.Ho = Ho; p.Wo = Wo;
  p.kh = kh; p.kw = kw; p.sh = 1; p.sw = 1; p.ph = ph; p.pw = pw; p.dh = dh; p.dw = dw;
  p.groups = groups; p.dg = 1; p.P = N * Ho * Wo; p.allow_fast = 1;
  p.ep_mask = ep_mask; p.ep_add = ep_add; p.ep_leaky = ep_act;
  return dc_run(st, p, packed, packed_bytes, tag, workspace, ws_bytes, (hipStream_t)stream, what);
}

int MFN_API(deform_conv_fwd)(const float *x, const float *offset, const float *w, const float *bias, float *out,
                             int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                             int dh, int dw, int groups, int dg, void *workspace, size_t ws_bytes, void *stream) {
  return dc_fwd_common(settings_now(), "deform_conv_fwd", x, offset, w, nullptr, 0, 0, bias, out, N, Cin, H, W, Cout, kh, kw, sh, sw, ph,
                       pw, dh, dw, groups, dg, workspace, ws_bytes, stream);
}

int MFN_API(deform_conv_fwd_packed)(const float *x, const float *offset, const void *packed, size_t packed_bytes,
                                    unsigned long long layout_tag, const float *bias, float *out, int N, int Cin, int H, int W, int Cout, int kh,
                                    int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int dg,
                                    void *workspace, size_t ws_bytes, void *stream) {
  if (!packed) return fail(MFN_E_NULL, "deform_conv_fwd_packed: NULL packed weights");
  return dc_fwd_common(settings_now(), "deform_conv_fwd_packed", x, offset, nullptr, packed, packed_bytes, layout_tag, bias, out, N, Cin, H, W,
                       Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg, workspace, ws_bytes, stream);
}

int MFN_API(deform_conv_shared_fwd)(const float *x, const float *flow, float flow_scale, float flow_stride,
                                    const float *w, const float *bias, float *out, int N, int Cin, int H, int W,
                                    int Cout, int kh, int kw, int ph, int pw, int dh, int dw, int groups,
                                    void *workspace, size_t ws_bytes, void *stream) {
  return dc_shared_common(settings_now(), "deform_conv_shared_fwd", x, flow, flow_scale, flow_stride, w, nullptr, 0, 0, bias, nullptr, nullptr, 0, out, N, Cin,
                          H, W, Cout, kh, kw, ph, pw, dh, dw, groups, workspace, ws_bytes, stream);
}

int MFN_API(deform_conv_shared_fwd_packed)(const float *x, const float *flow, float flow_scale, float flow_stride,
                                           const void *packed, size_t packed_bytes, unsigned long long layout_tag,
                                           const float *bias, float *out, int N, int Cin, int H, int W, int Cout, int kh, int kw, int ph, int pw,
                                           int dh, int dw, int groups, void *workspace, size_t ws_bytes, void *stream) {
  if (!packed) return fail(MFN_E_NULL, "deform_conv_shared_fwd_packed: NULL packed weights");
  return dc_shared_common(settings_now(), "deform_conv_shared_fwd_packed", x, flow, flow_scale, flow_stride, nullptr, packed,
                          packed_bytes, layout_tag, bias, nullptr, nullptr, 0, out, N, Cin, H, W, Cout, kh, kw, ph, pw, dh, dw,
                          groups, workspace, ws_bytes, stream);
}

int MFN_API(deform_conv_matching_fwd)(const float *x, const float *flow, float flow_scale, float flow_stride,
                                      const float *w, const void *packed, size_t packed_bytes,
                                      unsigned long long layout_tag, const float *bias, const float *mask,
                                      const float *tradeoff, int activation, float *out, int N, int Cin, int H, int W,
                                      int Cout, int kh, int kw, int ph, int pw, int dh, int dw, int groups,
                                      void *workspace, size_t ws_bytes, void *stream) {
  if (!w && !packed) return fail(MFN_E_NULL, "deform_conv_matching_fwd: neither weights nor packed weights");
  if (activation != 0 && activation != 1)
    return fail(MFN_E_PARAM, "deform_conv_matching_fwd: activation must be MFN_ACT_NONE or MFN_ACT_LEAKY_0_1");
  return dc_shared_common(settings_now(), "deform_conv_matching_fwd", x, flow, flow_scale, flow_stride, packed ? nullptr : w, packed,
                          packed ? packed_bytes : 0, layout_tag, bias, mask, tradeoff, activation, out, N, Cin, H, W, Cout, kh,
                          kw, ph, pw, dh, dw, groups, workspace, ws_bytes, stream);
}

static int offsets_from_flow_run(const Settings &st, const float *flow, float *offset, int N, int H, int W, int taps, float scale, float stride,
                                 hipStream_t s) {
  OffsetsParams p{flow, offset, N, H, W, taps, scale, stride, store_policy_for(st, (size_t)N * 2 * taps * H * W * 4, 2, -1)};
  return hipfail(offsets_from_flow_launch(p, s), "offsets_from_flow");
}
int MFN_API(offsets_from_flow)(const float *flow, float *offset, int N, int H, int W, int taps, float scale,
                               float stride, void *stream) {
  if (N != 0 && (!flow || !offset)) return fail(MFN_E_NULL, "offsets_from_flow: NULL tensor pointer");
  if (N < 0 || H <= 0 || W <= 0 || taps < 1) return fail(MFN_E_SHAPE, "offsets_from_flow: bad shape");
  if (stride == 0.f) return fail(MFN_E_PARAM, "offsets_from_flow: stride must be non-zero");
  return offsets_from_flow_run(settings_now(), flow, offset, N, H, W, taps, scale, stride, (hipStream_t)stream);
}

int MFN_API(upsample_fwd)(const float *x, float *out, int N, int C, int H, int W, int factor, void *stream) {
  if (N != 0 && (!x || !out)) return fail(MFN_E_NULL, "upsample_fwd: NULL tensor pointer");
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "upsample_fwd: N=%d C=%d H=%d W=%d", N, C, H, W);
  if (factor < 1) return fail(MFN_E_PARAM, "upsample_fwd: factor=%d must be >= 1", factor);
  if ((size_t)H * factor >= ((size_t)1 << 30) || (size_t)W * factor >= ((size_t)1 << 30))
    return fail(MFN_E_UNSUPPORTED, "upsample_fwd: output plane too large");
  if (N == 0) return 0;
  UpsampleParams p{x, out, N, C, H, W, factor, store_policy_for(settings_now(), (size_t)N * C * H * W * factor * factor * 4, 2, -1)};
  return hipfail(upsample_launch(p, (hipStream_t)stream), "upsample_fwd");
}

// ---- prediction on images of any size: joint mean, centralize + resize, metrics (kernels/predict.h) -------------------
// sizes every resize entry accepts: positive, planes and output elements inside what one launch indexes
static int resize_dims(const char *what, int N, int C, int Hin, int Win, int Hout, int Wout) {
  if (N < 0 || C <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0)
    return fail(MFN_E_SHAPE, "%s: N=%d C=%d Hin=%d Win=%d Hout=%d Wout=%d", what, N, C, Hin, Win, Hout, Wout);
  if ((size_t)2 * N * C >= ((size_t)1 << 31) || (size_t)Hin * Win >= ((size_t)1 << 31) ||
      (size_t)2 * N * C * Hout * Wout >= ((size_t)1 << 32))
    return fail(MFN_E_UNSUPPORTED, "%s: tensor too large", what);
  return 0;
}
static int resize_run(const Settings &st, const char *what, const float *x, const float *x2, const float *sub, float *out, int planes,
                      int planes_a, int Hin, int Win, int Hout, int Wout, int flow, hipStream_t s) {
  ResizeParams p{};
  p.x = x; p.x2 = x2; p.sub = sub; p.out = out;
  p.planes = planes; p.planes_a = planes_a;
  p.Hin = Hin; p.Win = Win; p.Hout = Hout; p.Wout = Wout;
  p.ry = Hout > 1 ? (float)(Hin - 1) / (float)(Hout - 1) : 0.f;
  p.rx = Wout > 1 ? (float)(Win - 1) / (float)(Wout - 1) : 0.f;
  p.flow = flow;
  p.sy = (float)((double)Hout / (double)Hin);
  p.sx = (float)((double)Wout / (double)Win);
  p.st_policy = store_policy_for(st, (size_t)planes * Hout * Wout * 4, 2, -1);
  return hipfail(resize_launch(p, s), what);
}
// the reductions' shapes: slices of 4096 elements, at most 4096 of them per result, results over blockIdx.y
static int reduce_dims(const char *what, size_t results, size_t elems) {
  if (results > 65535 || (elems + PRED_SLICE - 1) / PRED_SLICE > (size_t)PRED_MAX_SLICES) return fail(MFN_E_UNSUPPORTED, "%s: tensor too large", what);
  return 0;
}

size_t MFN_API(pair_mean_workspace_bytes)(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * C * pred_slices((size_t)2 * H * W) * sizeof(float);
}

int MFN_API(pair_mean)(const float *im1, const float *im2, float *mean, int N, int C, int H, int W, void *workspace,
                       size_t workspace_bytes, void *stream) {
  if (N != 0 && (!im1 || !im2 || !mean)) return fail(MFN_E_NULL, "pair_mean: NULL tensor pointer");
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "pair_mean: N=%d C=%d H=%d W=%d", N, C, H, W);
  if (N == 0) return 0;
  const size_t plane = (size_t)H * W;
  if (int rc = reduce_dims("pair_mean", (size_t)N * C, 2 * plane)) return rc;
  const int slices = pred_slices(2 * plane);
  const size_t need = (size_t)N * C * slices * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(MFN_E_WORKSPACE, "pair_mean: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (!aligned(workspace, 4)) return fail(MFN_E_ALIGN, "pair_mean: workspace must be 4-byte aligned");
  PairMeanParams p{im1, im2, (float *)workspace, mean, plane, N * C, slices,
                   (plane % 4 == 0 && aligned(im1, 16) && aligned(im2, 16)) ? 1 : 0};
  return hipfail(pair_mean_launch(p, (hipStream_t)stream), "pair_mean");
}

int MFN_API(preprocess_pair)(const float *im1, const float *im2, const float *mean, float *out, int N, int C, int H, int W,
                             int Hout, int Wout, void *stream) {
  if (N != 0 && (!im1 || !im2 || !mean || !out)) return fail(MFN_E_NULL, "preprocess_pair: NULL tensor pointer");
  if (int rc = resize_dims("preprocess_pair", N, C, H, W, Hout, Wout)) return rc;
  if (N == 0) return 0;
  return resize_run(settings_now(), "preprocess_pair", im1, im2, mean, out, 2 * N * C, N * C, H, W, Hout, Wout, 0, (hipStream_t)stream);
}

int MFN_API(bilinear_resize_fwd)(const float *x, const float *sub_or_null, float *out, int N, int C, int Hin, int Win, int Hout,
                                 int Wout, int flow_rescale, void *stream) {
  if (N != 0 && (!x || !out)) return fail(MFN_E_NULL, "bilinear_resize_fwd: NULL tensor pointer");
  if (int rc = resize_dims("bilinear_resize_fwd", N, C, Hin, Win, Hout, Wout)) return rc;
  if (flow_rescale && C != 2) return fail(MFN_E_SHAPE, "bilinear_resize_fwd: flow_rescale needs C == 2 (dy, dx), got C=%d", C);
  if (N == 0) return 0;
  return resize_run(settings_now(), "bilinear_resize_fwd", x, nullptr, sub_or_null, out, N * C, N * C, Hin, Win, Hout, Wout,
                    flow_rescale ? 1 : 0, (hipStream_t)stream);
}

size_t MFN_API(flow_metrics_workspace_bytes)(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * pred_slices((size_t)H * W) * 3 * sizeof(float);
}

int MFN_API(flow_metrics)(const float *flow, const float *label, const float *mask, float *sums, int N, int H, int W,
                          void *workspace, size_t workspace_bytes, void *stream) {
  if (N != 0 && (!flow || !label || !mask || !sums)) return fail(MFN_E_NULL, "flow_metrics: NULL tensor pointer");
  if (N < 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "flow_metrics: N=%d H=%d W=%d", N, H, W);
  if (N == 0) return 0;
  const size_t plane = (size_t)H * W;
  if (int rc = reduce_dims("flow_metrics", N, plane)) return rc;
  const int slices = pred_slices(plane);
  const size_t need = (size_t)N * slices * 3 * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(MFN_E_WORKSPACE, "flow_metrics: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (!aligned(workspace, 4)) return fail(MFN_E_ALIGN, "flow_metrics: workspace must be 4-byte aligned");
  FlowMetricsParams p{flow, label, mask, (float *)workspace, sums, plane, N, slices};
  return hipfail(flow_metrics_launch(p, (hipStream_t)stream), "flow_metrics");
}

// ---- prediction on uint8 frame sequences, the colour picture of a flow (kernels/frames.h) -----------------------------------
// what every frames entry accepts: positive sizes, both index ranges inside [0, F), a frame inside what one launch indexes
static int frames_dims(const char *what, int F, int H, int W, int a0, int b0, int N) {
  if (N < 0) return fail(MFN_E_SHAPE, "%s: N=%d is negative", what, N);
  if (F < 0) return fail(MFN_E_SHAPE, "%s: F=%d is negative", what, F);
  if (H < 1 || W < 1) return fail(MFN_E_SHAPE, "%s: H=%d W=%d must be >= 1", what, H, W);
  if (a0 < 0) return fail(MFN_E_SHAPE, "%s: a0=%d is negative", what, a0);
  if (b0 < 0) return fail(MFN_E_SHAPE, "%s: b0=%d is negative", what, b0);
  if ((long long)a0 + N > F) return fail(MFN_E_SHAPE, "%s: a0 + N = %lld leaves the F=%d frames", what, (long long)a0 + N, F);
  if ((long long)b0 + N > F) return fail(MFN_E_SHAPE, "%s: b0 + N = %lld leaves the F=%d frames", what, (long long)b0 + N, F);
  if ((size_t)H * W * 3 >= ((size_t)1 << 31)) return fail(MFN_E_UNSUPPORTED, "%s: frame too large", what);
  return 0;
}

size_t MFN_API(pair_mean_u8_workspace_bytes)(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * pred_slices((size_t)2 * H * W) * 3 * sizeof(unsigned);
}

int MFN_API(pair_mean_u8)(const unsigned char *frames, int F, int H, int W, int a0, int b0, int N, float *mean, void *workspace,
                          size_t workspace_bytes, void *stream) {
  if (N != 0 && (!frames || !mean)) return fail(MFN_E_NULL, "pair_mean_u8: NULL tensor pointer");
  if (int rc = frames_dims("pair_mean_u8", F, H, W, a0, b0, N)) return rc;
  if (N == 0) return 0;
  const size_t plane = (size_t)H * W;
  if (int rc = reduce_dims("pair_mean_u8", (size_t)N, 2 * plane)) return rc;
  const int slices = pred_slices(2 * plane);
  const size_t need = (size_t)N * slices * 3 * sizeof(unsigned);
  if (!workspace || workspace_bytes < need)
    return fail(MFN_E_WORKSPACE, "pair_mean_u8: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (!aligned(workspace, 4) || !aligned(mean, 4)) return fail(MFN_E_ALIGN, "pair_mean_u8: mean and workspace must be 4-byte aligned");
  PairMeanU8Params p{frames, (unsigned *)workspace, mean, plane, 255.0 * (double)(2 * plane), a0, b0, N, slices};
  return hipfail(pair_mean_u8_launch(p, (hipStream_t)stream), "pair_mean_u8");
}

int MFN_API(preprocess_pair_u8)(const unsigned char *frames, int F, int H, int W, int a0, int b0, int N, const float *mean_or_null,
                                float *out, int Hout, int Wout, void *stream) {
  if (N != 0 && (!frames || !out)) return fail(MFN_E_NULL, "preprocess_pair_u8: NULL tensor pointer");
  if (int rc = frames_dims("preprocess_pair_u8", F, H, W, a0, b0, N)) return rc;
  if (Hout < 1 || Wout < 1) return fail(MFN_E_SHAPE, "preprocess_pair_u8: Hout=%d Wout=%d must be >= 1", Hout, Wout);
  if (int rc = resize_dims("preprocess_pair_u8", N, 3, H, W, Hout, Wout)) return rc;
  if (N == 0) return 0;
  if (!aligned(out, 4) || !aligned(mean_or_null, 4)) return fail(MFN_E_ALIGN, "preprocess_pair_u8: mean and out must be 4-byte aligned");
  FramesPreParams p{};
  p.frames = frames; p.mean = mean_or_null; p.out = out;
  p.a0 = a0; p.b0 = b0; p.N = N;
  p.H = H; p.W = W; p.Hout = Hout; p.Wout = Wout;
  p.ry = Hout > 1 ? (float)(H - 1) / (float)(Hout - 1) : 0.f;
  p.rx = Wout > 1 ? (float)(W - 1) / (float)(Wout - 1) : 0.f;
  p.st_policy = store_policy_for(settings_now(), (size_t)6 * N * Hout * Wout * 4, 2, -1);
  return hipfail(frames_pre_launch(p, (hipStream_t)stream), "preprocess_pair_u8");
}

size_t MFN_API(flow_color_workspace_bytes)(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * (pred_slices((size_t)H * W) + 1) * sizeof(float);
}

int MFN_API(flow_color)(const float *flow, unsigned char *rgb, int N, int H, int W, float rad_max, int bgr, void *workspace,
                        size_t workspace_bytes, void *stream) {
  if (N != 0 && (!flow || !rgb)) return fail(MFN_E_NULL, "flow_color: NULL tensor pointer");
  if (N < 0 || H < 1 || W < 1) return fail(MFN_E_SHAPE, "flow_color: N=%d H=%d W=%d", N, H, W);
  if (rad_max != rad_max) return fail(MFN_E_PARAM, "flow_color: rad_max is NaN");
  if (N == 0) return 0;
  const size_t plane = (size_t)H * W;
  if ((size_t)N * plane * 3 >= ((size_t)1 << 32)) return fail(MFN_E_UNSUPPORTED, "flow_color: tensor too large");
  if (int rc = reduce_dims("flow_color", (size_t)N, plane)) return rc;
  const int slices = pred_slices(plane);
  const size_t need = (size_t)N * (slices + 1) * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(MFN_E_WORKSPACE, "flow_color: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (!aligned(workspace, 4) || !aligned(flow, 4)) return fail(MFN_E_ALIGN, "flow_color: flow and workspace must be 4-byte aligned");
  FlowColorParams p{flow, rgb, (float *)workspace, (float *)workspace + (size_t)N * slices, rad_max, N, H, W, slices, bgr ? 1 : 0};
  return hipfail(flow_color_launch(p, (hipStream_t)stream), "flow_color");
}

// ---- augmentation of the training batch: geometry, colour (kernels/augment.h) ---------------------------------------------
static int augment_color_dims(const char *what, int N, int H, int W) {
  if (N < 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "%s: N=%d H=%d W=%d", what, N, H, W);
  if ((size_t)2 * N > 65535 || (size_t)6 * N * (size_t)H * W >= ((size_t)1 << 32)) return fail(MFN_E_UNSUPPORTED, "%s: tensor too large", what);
  return reduce_dims(what, (size_t)2 * N, (size_t)H * W);
}
static AugNoise augment_noise(unsigned long long seed, unsigned long long offset) {
  return AugNoise{(unsigned)seed, (unsigned)(seed >> 32), (unsigned)offset, (unsigned)(offset >> 32)};
}

int MFN_API(augment_geometry)(const float *img1, const float *img2, const float *flow, const float *mask, int mask_is_plane,
                              const float *table, float *out1, float *out2, float *flow_out, float *mask_out, int N, int Ho, int Wo,
                              int Ht, int Wt, int label_order, void *stream) {
  if (N != 0 && (!img1 || !img2 || !flow || !mask || !table || !out1 || !out2 || !flow_out || !mask_out))
    return fail(MFN_E_NULL, "augment_geometry: NULL tensor pointer");
  if (N < 0 || Ho <= 0 || Wo <= 0 || Ht < 2 || Wt < 2)
    return fail(MFN_E_SHAPE, "augment_geometry: N=%d Ho=%d Wo=%d Ht=%d Wt=%d (a target side must be >= 2)", N, Ho, Wo, Ht, Wt);
  if ((size_t)Ho * Wo >= ((size_t)1 << 31) || (size_t)N * Ht * Wt >= ((size_t)1 << 31))
    return fail(MFN_E_UNSUPPORTED, "augment_geometry: tensor too large");
  if (N == 0) return 0;
  AugGeoParams p{};
  p.img1 = img1; p.img2 = img2; p.flow = flow; p.mask = mask; p.tab = table;
  p.o1 = out1; p.o2 = out2; p.oflow = flow_out; p.omask = mask_out;
  p.N = N; p.Ho = Ho; p.Wo = Wo; p.Ht = Ht; p.Wt = Wt;
  p.mask_plane = mask_is_plane ? 1 : 0;
  p.label_order = label_order ? 1 : 0;
  p.sx = (float)(2.0 / (Wt - 1));
  p.sy = (float)(2.0 / (Ht - 1));
  p.st_policy = store_policy_for(settings_now(), (size_t)N * 9 * Ht * Wt * 4, 2, -1);
  return hipfail(augment_geometry_launch(p, (hipStream_t)stream), "augment_geometry");
}

size_t MFN_API(augment_color_mean_workspace_bytes)(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)2 * N * pred_slices((size_t)H * W) * 3 * sizeof(float);
}

int MFN_API(augment_color_mean)(const float *img1, const float *img2, const float *table, float sigma, unsigned long long seed,
                                unsigned long long offset, float *mean, int N, int H, int W, void *workspace, size_t workspace_bytes,
                                void *stream) {
  if (N != 0 && (!img1 || !img2 || !table || !mean)) return fail(MFN_E_NULL, "augment_color_mean: NULL tensor pointer");
  if (int rc = augment_color_dims("augment_color_mean", N, H, W)) return rc;
  if (N == 0) return 0;
  const size_t plane = (size_t)H * W;
  const int slices = pred_slices(plane);
  const size_t need = (size_t)2 * N * slices * 3 * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(MFN_E_WORKSPACE, "augment_color_mean: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (!aligned(workspace, 4)) return fail(MFN_E_ALIGN, "augment_color_mean: workspace must be 4-byte aligned");
  AugColorParams p{};
  p.img1 = img1; p.img2 = img2; p.tab = table; p.partial = (float *)workspace; p.mean = mean;
  p.plane = plane; p.N = N; p.slices = slices; p.sigma = sigma; p.noise = augment_noise(seed, offset);
  return hipfail(augment_color_mean_launch(p, (hipStream_t)stream), "augment_color_mean");
}

int MFN_API(augment_color)(const float *img1, const float *img2, const float *table, const float *mean, float sigma,
                           unsigned long long seed, unsigned long long offset, int use_spin, int use_gamma, float *out, int N, int H,
                           int W, void *stream) {
  if (N != 0 && (!img1 || !img2 || !table || !mean || !out)) return fail(MFN_E_NULL, "augment_color: NULL tensor pointer");
  if (int rc = augment_color_dims("augment_color", N, H, W)) return rc;
  if (N == 0) return 0;
  AugColorParams p{};
  p.img1 = img1; p.img2 = img2; p.tab = table; p.mean_in = mean; p.out = out;
  p.plane = (size_t)H * W; p.N = N; p.sigma = sigma; p.noise = augment_noise(seed, offset);
  p.spin = use_spin ? 1 : 0; p.gamma = use_gamma ? 1 : 0;
  p.st_policy = store_policy_for(settings_now(), (size_t)6 * N * H * W * 4, 2, -1);
  return hipfail(augment_color_launch(p, (hipStream_t)stream), "augment_color");
}

// ---- backward (SURVEY.md 8 a7) -------------------------------------------------------------------------------
static bool req_ok(int r) { return r == MFN_REQ_NULL || r == MFN_REQ_WRITE || r == MFN_REQ_ADD; }

// What corr_bwd_plan decides for a backward call and mfn_correlation_bwd launches (a new kernel family: a member here, a case there).
enum class CorrBwdFamily { Lds, Block, Gather, Scatter };
struct CorrBwdPlan { CorrBwdFamily family; dim3 grid; int rows; size_t lds_bytes; int store_policy; };
// aligned16: gout, both feature maps and the requested gradients allow 16-byte accesses; out_elems: elements of gout
static CorrBwdPlan corr_bwd_plan(const Settings &st, int N, int C, int H, int W, int md, int kernel, int s1, int s2, int pad, int is_multiply,
                                 int req1, int req2, bool aligned16, size_t out_elems) {
  const size_t in_elems = (size_t)N * C * H * W;
  const int D = 2 * (md / s2) + 1, cq = (C + 3) / 4;
  const unsigned parts = (req1 && req2) ? 2u : 1u;   // both gradients requested: one block row each
  CorrBwdPlan pl{CorrBwdFamily::Scatter, dim3((unsigned)((out_elems + 255) / 256)), 0, 0, store_policy_for(st, in_elems * 4, 2, -1)};
  if (kernel != 1 || s1 != 1 || s2 != 1 || pad != md || !is_multiply) return pl;
  pl.family = CorrBwdFamily::Gather;
  pl.grid = dim3((unsigned)((in_elems + 255) / 256));
  if (W % 4 != 0 || (D != 9 && D != 5) || !aligned16) return pl;
  pl.family = CorrBwdFamily::Block;
  pl.grid = dim3((unsigned)(((size_t)N * cq * H * (W / 4) + 255) / 256), parts);
  if ((st.t.bwd_off & 4) == 0 && (W == 8 || W == 16 || W == 32 || W == 64 || W == 128 || W == 256)) {
    // the other feature map's rows through LDS (kernels/backward.h: corr_bwd_lds_kernel), a block row per gradient.  Measured
    // at the five levels of cfg2 against corr_bwd_block_kernel (both gradients, us): 14.5 / 15.1 / 20.5 / 29.9 / 54.6 before
    pl.family = CorrBwdFamily::Lds;
    pl.rows = 256 / (W / 4);
    pl.grid = dim3((unsigned)(N * cq * cdiv(H, pl.rows)), parts);
    pl.lds_bytes = corr_bwd_lds_bytes(H, W, D / 2);
  }
  return pl;
}

int MFN_API(correlation_bwd)(const float *gout, const float *d1, const float *d2, float *g1, float *g2, int N, int C,
                             int H, int W, int md, int kernel, int s1, int s2, int pad, int is_multiply, int req1,
                             int req2, void *stream) {
  const Settings st = settings_now();
  if (N != 0 && (!gout || !d1 || !d2)) return fail(MFN_E_NULL, "correlation_bwd: NULL tensor pointer");
  if (N != 0 && ((req1 && !g1) || (req2 && !g2))) return fail(MFN_E_NULL, "correlation_bwd: NULL gradient output");
  if (!req_ok(req1) || !req_ok(req2)) return fail(MFN_E_PARAM, "correlation_bwd: req must be 0 (null), 1 (write) or 3 (add)");
  if (N < 0 || C <= 0) return fail(MFN_E_SHAPE, "correlation_bwd: N=%d C=%d", N, C);
  int tc, th, tw;
  int rc = corr_shape(H, W, md, kernel, s1, s2, pad, &tc, &th, &tw);
  if (rc) return rc;
  if (N == 0 || (!req1 && !req2)) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int r = md / s2, D = 2 * r + 1;
  const bool al16 = aligned(gout, 16) && aligned(d1, 16) && aligned(d2, 16) && (!g1 || aligned(g1, 16)) && (!g2 || aligned(g2, 16));
  const CorrBwdPlan pl = corr_bwd_plan(st, N, C, H, W, md, kernel, s1, s2, pad, is_multiply, req1, req2, al16, (size_t)N * tc * th * tw);
  const CorrBwdParams p{gout, d1, d2, g1, g2, N, C, H, W, md, D, req1, req2, pl.store_policy};
  switch (pl.family) {
    case CorrBwdFamily::Lds: {
      const CorrBwdLdsParams lp{p, pl.rows, cdiv(H, pl.rows)};
      rc = D == 9 ? launch("corr_bwd_lds", corr_bwd_lds_kernel<4>, pl.grid, dim3(256), pl.lds_bytes, s, lp)
                  : launch("corr_bwd_lds", corr_bwd_lds_kernel<2>, pl.grid, dim3(256), pl.lds_bytes, s, lp);
      break;
    }
    case CorrBwdFamily::Block: rc = launch("corr_bwd_block", corr_bwd_block_kernel<0>, pl.grid, dim3(256), 0, s, p); break;
    case CorrBwdFamily::Gather: rc = launch("corr_bwd_gather", corr_bwd_gather_kernel, pl.grid, dim3(256), 0, s, p); break;
    case CorrBwdFamily::Scatter: {
      const size_t in_elems = (size_t)N * C * H * W;
      if (req1 == MFN_REQ_WRITE && (rc = fill_zero_launch(g1, in_elems, s))) break;
      if (req2 == MFN_REQ_WRITE && (rc = fill_zero_launch(g2, in_elems, s))) break;
      const CorrBwdGenericParams gp{gout, d1, d2, g1, g2, N, C, H, W, md, kernel, s1, s2, pad, is_multiply ? 1 : 0, tc, th, tw, r, D, req1, req2};
      rc = launch("corr_bwd_scatter", corr_bwd_scatter_kernel, pl.grid, dim3(256), 0, s, gp);
    }
  }
  return hipfail(rc, "correlation_bwd");
}

int MFN_API(warp_bwd)(const float *gout, const float *x, const float *flow, float *gx, float *gflow, int N, int C, int H,
                      int W, int clip, int req_x, int req_flow, void *stream) {
  if (N != 0 && (!gout || !x || !flow)) return fail(MFN_E_NULL, "warp_bwd: NULL tensor pointer");
  if (N != 0 && ((req_x && !gx) || (req_flow && !gflow))) return fail(MFN_E_NULL, "warp_bwd: NULL gradient output");
  if (!req_ok(req_x) || !req_ok(req_flow)) return fail(MFN_E_PARAM, "warp_bwd: req must be 0 (null), 1 (write) or 3 (add)");
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "warp_bwd: N=%d C=%d H=%d W=%d", N, C, H, W);
  if (N == 0 || (!req_x && !req_flow)) return 0;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (req_x == MFN_REQ_WRITE && (rc = fill_zero_launch(gx, (size_t)N * C * H * W, s))) return hipfail(rc, "warp_bwd");
  WarpBwdParams p{gout, x, flow, gx, gflow, N, C, H, W, clip ? 1 : 0, req_x, req_flow};
  const size_t total = (size_t)N * H * W;
  return hipfail(launch("warp_bwd", warp_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p), "warp_bwd");
}

int MFN_API(bilinear_sampler_bwd)(const float *gout, const float *data, const float *grid, float *gdata, float *ggrid,
                                  int N, int C, int iH, int iW, int oH, int oW, int req_data, int req_grid, void *stream) {
  if (N != 0 && (!gout || !data || !grid)) return fail(MFN_E_NULL, "bilinear_sampler_bwd: NULL tensor pointer");
  if (N != 0 && ((req_data && !gdata) || (req_grid && !ggrid))) return fail(MFN_E_NULL, "bilinear_sampler_bwd: NULL gradient output");
  if (!req_ok(req_data) || !req_ok(req_grid)) return fail(MFN_E_PARAM, "bilinear_sampler_bwd: req must be 0 (null), 1 (write) or 3 (add)");
  if (N < 0 || C <= 0 || iH <= 0 || iW <= 0 || oH <= 0 || oW <= 0) return fail(MFN_E_SHAPE, "bilinear_sampler_bwd: bad shape");
  if (N == 0 || (!req_data && !req_grid)) return 0;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (req_data == MFN_REQ_WRITE && (rc = fill_zero_launch(gdata, (size_t)N * C * iH * iW, s))) return hipfail(rc, "bilinear_sampler_bwd");
  SamplerBwdParams p{gout, data, grid, gdata, ggrid, N, C, iH, iW, oH, oW, req_data, req_grid};
  const size_t total = (size_t)N * oH * oW;
  return hipfail(launch("bilinear_sampler_bwd", bilinear_sampler_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p),
                 "bilinear_sampler_bwd");
}

int MFN_API(grid_generator_warp_bwd)(const float *ggrid, float *gflow_xy, int N, int H, int W, int req, void *stream) {
  if (N != 0 && (!ggrid || (req && !gflow_xy))) return fail(MFN_E_NULL, "grid_generator_warp_bwd: NULL tensor pointer");
  if (!req_ok(req)) return fail(MFN_E_PARAM, "grid_generator_warp_bwd: req must be 0 (null), 1 (write) or 3 (add)");
  if (N < 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "grid_generator_warp_bwd: N=%d H=%d W=%d", N, H, W);
  if (N == 0 || !req) return 0;
  GridWarpBwdParams p{ggrid, gflow_xy, N, H, W, req};
  const size_t total = (size_t)N * 2 * H * W;
  return hipfail(launch("grid_generator_warp_bwd", grid_warp_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                        (hipStream_t)stream, p), "grid_generator_warp_bwd");
}

// What dc_bwd_plan decides for a backward call of the deformable convolution and dc_bwd_exec launches, top to bottom.
enum class DcBwdIn { None, Pix, Tile, Generic };
enum class DcBwdW { None, PcSlabs, Pc, Mfma, Generic };
struct DcBwdPlan {
  DcBwdIn in;                  // input / offset gradient: dc_bwd_input_pix_kernel | dc_bwd_input_tile_kernel | dc_bwd_input_kernel
  int tiles_x, tiles_y;        // Pix / Tile: DCI_TW x DCI_TH pixel tiles of an image
  int pblocks, ksplit, xcd;    // Pix: channel blocks, filter slices over blockIdx.z, block order by XCD
  int cchunk;                  // Generic: input channels per thread
  DcBwdW w;                    // weight gradient: dc_bwd_weight_pc_kernel, its blocks' partial sums in workspace slabs (+ reduce launch) or
                               // added to gw through atomics | dc_bwd_weight_mfma_kernel | dc_bwd_weight_kernel
  int tx, ty, ntiles, cblocks, mtot, tpb, nblk;   // Pc*: 8x4-pixel tiles, channel blocks, filter tiles, tiles per block, blocks per channel block
  int mto, slices;             // Mfma: filter tiles per block, pixel slices
  bool bias_launch;            // dc_bwd_bias_kernel; otherwise the weight launch sums the bias as well (or none is requested)
  bool zero[4];                // write-mode gx, goffset, gw, gbias that accumulate through atomics start from zero: cleared by fill_zero4, or ...
  bool pc_zeroes;              // ... (gx, goffset) by the PcSlabs blocks on their way in: that launch then runs first, no fill launch
  bool flow_ok;                // flow mode wanted and every kernel of the call reads the flow field in place of an offset tensor
  size_t slab_bytes, ws_bytes; // the Pc slabs (weights' + bias'); what a size query answers
};
// p: shape and requests (Ho / Wo filled in).  What only a run knows: flow mode wanted (mfn_deform_conv_shared_bwd), 16-byte alignment of
// x and w, usable bytes of a 16-byte aligned workspace; a size query plans an aligned call that brings all the workspace the plan wants.
static DcBwdPlan dc_bwd_plan(const Settings &st, const DcBwdParams &p, bool flow = false, bool x16 = true, bool w16 = true,
                             size_t ws_bytes = (size_t)-1) {
  DcBwdPlan pl{};
  const int N = p.N, Cin = p.Cin, H = p.H, W = p.W, Cout = p.Cout, T = p.kh * p.kw;
  const bool fast = p.groups == 1 && p.dg == 1 && (st.t.path_generic & 2) == 0;
  const bool same = p.sh == 1 && p.sw == 1 && p.Ho == H && p.Wo == W && H < 65536 && W < 65536;
  // the shared-offset kernels' conditions that the host can see (the offsets themselves are judged per strip on the device)
  const bool shared = p.kh == 3 && p.kw == 3 && p.dh == 1 && p.dw == 1 && p.groups == 1 && p.dg == 1 && same;
  const bool fits30 = (size_t)N * Cin * H * W < ((size_t)1 << 30);
  // ---- weight gradient.  Pc: in the forward's orientation (kernels/dc_backward.h), columns produced as the forward kernel does, pixels
  // as the reduction dimension.  Up to three filter tiles: with four (level 5: one 4x8 tile per block) the per-block slab and the
  // reduce launch cost more than the per-tap kernel's atomics (37 against 25 us)
  const bool pc_shape = shared && W % 4 == 0 && Cout <= 96 && fits30;
  pl.tx = cdiv(W, 8); pl.ty = cdiv(H, 4); pl.ntiles = N * pl.tx * pl.ty; pl.cblocks = cdiv(Cin, 32); pl.mtot = cdiv(Cout, 32);
  pl.tpb = cdiv(pl.ntiles * pl.cblocks, 256);
  if (pl.tpb < 1) pl.tpb = 1;
  pl.nblk = cdiv(pl.ntiles, pl.tpb);
  pl.slab_bytes = ((size_t)pl.cblocks * pl.nblk * pl.mtot * 32 * 288 + (size_t)pl.nblk * pl.mtot * 32) * sizeof(float);
  pl.ws_bytes = pc_shape ? pl.slab_bytes : 0;   // whatever the requests and path.generic (kept from round 2)
  const bool w_fast = p.req_w && fast && T <= 25;
  if (w_fast && pc_shape && x16) pl.w = ws_bytes >= pl.slab_bytes ? DcBwdW::PcSlabs : DcBwdW::Pc;
  else if (w_fast) {
    // fp32-MFMA weight gradient: pixels are the reduction dimension, partial sums meet in gw through atomics.
    // blocks = slices * jgroups * ogroups; every block ends with 32 x 32 atomics per wave into the same gw, so the
    // block count trades parallelism against atomic traffic
    // measured (tools/bwd_levels.py, cfg2): 512 blocks -- 27 / 62 / 84 / 142 us at levels 5..2 against 42 / 65 / 113 / 178 with 1024
    pl.w = DcBwdW::Mfma;
    pl.mto = Cout > 32 ? 2 : 1;
    const int tiles = cdiv((int)((size_t)N * p.Ho * p.Wo), 32), jgroups = cdiv(cdiv(Cin * T, 32), 4), ogroups = cdiv(Cout, pl.mto * 32);
    pl.slices = 512 / (jgroups * ogroups);
    pl.slices = pl.slices < 1 ? 1 : (pl.slices > tiles ? tiles : pl.slices);
  } else if (p.req_w) pl.w = DcBwdW::Generic;
  pl.bias_launch = p.req_bias && (pl.w == DcBwdW::None || pl.w == DcBwdW::Generic);
  const bool w_atomics = pl.w == DcBwdW::Pc || pl.w == DcBwdW::Mfma;
  pl.zero[0] = p.req_x == MFN_REQ_WRITE;
  pl.zero[1] = p.req_offset == MFN_REQ_WRITE;
  pl.zero[2] = w_atomics && p.req_w == MFN_REQ_WRITE;
  pl.zero[3] = w_atomics && p.req_bias == MFN_REQ_WRITE;
  pl.pc_zeroes = pl.w == DcBwdW::PcSlabs && (pl.zero[0] || pl.zero[1]);
  // ---- input / offset gradient.  Tile: fp32-MFMA column gradient + LDS-privatised scatter (kernels/backward.h), every tap of every
  // strip.  Pix: lane = pixel (kernels/dc_backward.h), 8x16-pixel regions x 16 channels, two blocks per CU, all nine taps in one pass
  // where they share one offset per pixel (the reference's only use); tiles that do not qualify are done tap by tap by the same blocks
  const bool tile_ok = fast && same && T <= 9;
  const bool pix_ok = tile_ok && shared && (st.t.bwd_off & 1) == 0 && W % 4 == 0 && Cin % 4 == 0 && x16 && w16 && fits30 &&
                      (size_t)Cout * H * W < ((size_t)1 << 29) && (size_t)Cout * Cin * 9 < ((size_t)1 << 29);
  pl.tiles_x = cdiv(W, DCI_TW); pl.tiles_y = cdiv(H, DCI_TH);
  if (!p.req_x && !p.req_offset) pl.in = DcBwdIn::None;
  else if (pix_ok) {
    pl.in = DcBwdIn::Pix;
    const int tiles8 = N * pl.tiles_x * pl.tiles_y;
    pl.pblocks = cdiv(Cin, DCP_CB);
    pl.xcd = (pl.pblocks == 1 || tiles8 % 8 == 0) ? 1 : 0;
    // fewer blocks than the chip has CUs (coarse levels): the filters are split over blockIdx.z (chunks of 16) up to ONE
    // block per CU -- every slice repeats everything behind the K loop, and two such blocks on a CU slow each other
    // (level 5, same box: 256 slots 35.4-36.9 us, 512 slots 37.9-38.2, 128 slots 40.3)
    pl.ksplit = 256 / (tiles8 * pl.pblocks);
    pl.ksplit = pl.ksplit < 1 ? 1 : (pl.ksplit > cdiv(Cout, DCP_KO) ? cdiv(Cout, DCP_KO) : pl.ksplit);
  } else if (tile_ok) pl.in = DcBwdIn::Tile;
  else {
    pl.in = DcBwdIn::Generic;   // enough threads to fill the chip: the input channels of a pixel over several threads when pixels are few
    const long px = (long)N * p.Ho * p.Wo;
    long want = (65536 + px - 1) / px;
    want = want < 1 ? 1 : (want > Cin ? Cin : want);
    pl.cchunk = (int)((Cin + want - 1) / want);
  }
  pl.flow_ok = flow && (st.t.bwd_off & 2) == 0 && pix_ok && (!p.req_w || pc_shape);
  return pl;
}
static size_t dc_bwd_ws_bytes(const Settings &st, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                              int dh, int dw, int groups, int dg) {
  DcBwdParams p{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, Cin, H, W, Cout, 0, 0, kh, kw, sh, sw, ph, pw,
                dh, dw, groups, dg, 0, 0, 0, 0, 1};
  if (N <= 0 || Cin <= 0 || Cout <= 0 || MFN_API(deform_conv_out_shape)(H, W, kh, kw, sh, sw, ph, pw, dh, dw, &p.Ho, &p.Wo)) return 0;
  return dc_bwd_plan(st, p).ws_bytes;
}
// workspace of the backward: the weight gradient's per-block slabs (the column gradient is formed on the fly)
size_t MFN_API(deform_conv_bwd_workspace_bytes)(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                                                int dh, int dw, int groups, int dg) {
  return dc_bwd_ws_bytes(settings_now(), N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, dg);
}

// flow mode of the backward (mfn_deform_conv_shared_bwd): the kernels of kernels/dc_backward.h read the flow field in place of an
// offset tensor and write d/dflow in place of goffset (p.goffset).  Only where the plan says they take the whole call (flow_ok).
struct DcFlowArgs { const float *flow; float scale, stride; };
static int dc_bwd_weight_pc(const DcBwdPlan &pl, const DcBwdParams &p, float *slabs, const DcFlowArgs *fl, float *const zero[2],
                            const size_t zero_n[2], hipStream_t s) {
  DcBwdWPParams wp{p.gout, p.x, p.offset, p.gw, p.req_bias ? p.gbias : nullptr, p.N, p.Cin, p.H, p.W, p.Cout, p.ph, p.pw, pl.tx, pl.ty, pl.ntiles,
                   1.f / (float)(pl.tx * pl.ty), 1.f / (float)pl.tx, pl.tpb, slabs,
                   slabs ? slabs + (size_t)pl.cblocks * pl.nblk * pl.mtot * 32 * 288 : nullptr,
                   (p.req_x || p.req_offset) ? nullptr : (unsigned long long *)((unsigned long long)g_timeline & ~1ull),
                   fl ? fl->flow : nullptr, fl ? fl->scale : 0.f, fl ? fl->stride : 1.f,
                   {zero ? zero[0] : nullptr, zero ? zero[1] : nullptr}, {zero ? zero_n[0] : 0, zero ? zero_n[1] : 0}};
  const dim3 grid(pl.nblk, pl.cblocks);
  const size_t lds2 = dc_bwd_weight_pc_lds_bytes(pl.mtot);   // producer / consumer waves (eight per block)
  int rc = pl.mtot == 1 ? launch("dc_bwd_weight_pc", dc_bwd_weight_pc_kernel<1>, grid, dim3(512), lds2, s, wp)
         : pl.mtot == 2 ? launch("dc_bwd_weight_pc", dc_bwd_weight_pc_kernel<2>, grid, dim3(512), lds2, s, wp)
                        : launch("dc_bwd_weight_pc", dc_bwd_weight_pc_kernel<3>, grid, dim3(512), lds2, s, wp);
  if (rc || !slabs) return rc;
  // the blocks' partial sums are added in block order
  const int wblocks = (int)(((size_t)p.Cout * p.Cin * 9 + 15) / 16), bblocks = p.req_bias ? cdiv(p.Cout, 16) : 0;
  DcBwdWRParams rp{slabs, wp.bias_slabs, p.gw, p.gbias, p.Cin, p.Cout, pl.mtot, pl.nblk, p.req_w == MFN_REQ_ADD ? 1 : 0,
                   p.req_bias == MFN_REQ_ADD ? 1 : 0, wblocks};
  return launch("dc_bwd_weight_reduce", dc_bwd_weight_reduce_kernel, dim3((unsigned)(wblocks + bblocks)), dim3(256), 256 * sizeof(float), s, rp);
}
// the launches of a plan, in order; returns a HIP status.  fl: flow mode (pl.flow_ok)
static int dc_bwd_exec(const DcBwdPlan &pl, DcBwdParams p, void *workspace, const DcFlowArgs *fl, hipStream_t s) {
  const size_t oplane = (size_t)p.Ho * p.Wo;
  const int T = p.kh * p.kw;
  float *const slabs = pl.w == DcBwdW::PcSlabs ? (float *)workspace : nullptr;
  float *const zp[4] = {pl.zero[0] ? p.gx : nullptr, pl.zero[1] ? p.goffset : nullptr, pl.zero[2] ? p.gw : nullptr, pl.zero[3] ? p.gbias : nullptr};
  const size_t zn[4] = {(size_t)p.N * p.Cin * p.H * p.W, fl ? (size_t)p.N * 2 * oplane : (size_t)p.N * 2 * T * p.dg * oplane,
                        (size_t)p.Cout * p.Cin * T, (size_t)p.Cout};
  int rc = pl.pc_zeroes ? dc_bwd_weight_pc(pl, p, slabs, fl, zp, zn, s) : fill_zero4_launch(zp, zn, s);   // one launch for all of them
  if (rc) return rc;
  unsigned long long *const timeline = (unsigned long long *)((unsigned long long)g_timeline & ~1ull);
  switch (pl.in) {
    case DcBwdIn::None: break;
    case DcBwdIn::Pix: {
      DcBwdPParams pp{p.gout, p.x, p.offset, p.w, p.gx, p.goffset, p.N, p.Cin, p.H, p.W, p.Cout, p.ph, p.pw, pl.tiles_x, pl.tiles_y,
                      1.f / (float)(pl.tiles_x * pl.tiles_y), 1.f / (float)pl.tiles_x, p.req_x, p.req_offset, pl.xcd, timeline,
                      (int)((unsigned long long)g_timeline & 1ull), fl ? fl->flow : nullptr, fl ? p.goffset : nullptr, fl ? fl->scale : 0.f,
                      fl ? fl->stride : 1.f};
      rc = launch("dc_bwd_input_pix", dc_bwd_input_pix_kernel, dim3(p.N * pl.tiles_x * pl.tiles_y, pl.pblocks, pl.ksplit), dim3(256),
                  dc_bwd_input_pix_lds_bytes(), s, pp);
      break;
    }
    case DcBwdIn::Tile: {
      DcBwdIParams ip{p.gout, p.x, p.offset, p.w, p.gx, p.goffset, p.N, p.Cin, p.H, p.W, p.Cout, p.kh, p.kw, p.ph, p.pw, p.dh, p.dw, T,
                      pl.tiles_x, pl.tiles_y, p.req_x, p.req_offset, timeline};
      rc = launch("dc_bwd_input_tile", dc_bwd_input_tile_kernel, dim3(p.N * pl.tiles_x * pl.tiles_y, cdiv(p.Cin, 32)), dim3(256),
                  dc_bwd_input_lds_bytes(), s, ip);
      break;
    }
    case DcBwdIn::Generic: {
      p.cchunk = pl.cchunk;
      const size_t total = (size_t)p.N * oplane * ((p.Cin + p.cchunk - 1) / p.cchunk);
      rc = launch("dc_bwd_input", dc_bwd_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    }
  }
  if (rc) return rc;
  switch (pl.w) {
    case DcBwdW::None: break;
    case DcBwdW::PcSlabs:
    case DcBwdW::Pc:
      if (!pl.pc_zeroes) rc = dc_bwd_weight_pc(pl, p, slabs, fl, nullptr, nullptr, s);
      break;
    case DcBwdW::Mfma: {
      DcBwdWParams wp{p.gout, p.x, p.offset, p.gw, p.req_bias ? p.gbias : nullptr, p.N, p.Cin, p.H, p.W, p.Cout, p.Ho, p.Wo, p.kh, p.kw, p.sh, p.sw,
                      p.ph, p.pw, p.dh, p.dw, (int)((size_t)p.N * oplane), p.Cin * T, T, 1};
      rc = pl.mto == 2 ? dc_bwd_weight_mfma_launch<2>(wp, pl.slices, s) : dc_bwd_weight_mfma_launch<1>(wp, pl.slices, s);
      break;
    }
    case DcBwdW::Generic:
      rc = launch("dc_bwd_weight", dc_bwd_weight_kernel, dim3(p.Cin * T * cdiv(p.Cout / p.groups, DC_BW_OC)), dim3(256),
                  (size_t)DC_BW_OC * 256 * sizeof(float), s, p);
  }
  if (!rc && pl.bias_launch) rc = launch("dc_bwd_bias", dc_bwd_bias_kernel, dim3(p.Cout), dim3(256), 256 * sizeof(float), s, p);
  return rc;
}

// the checks every backward call of the deformable convolution makes (p.Ho / p.Wo filled in), then its requests and gradient pointers
static int dc_bwd_dims(const char *what, DcBwdParams &p) {
  return dc_check(what, p.x, p.w, p.gout, p.N, p.Cin, p.H, p.W, p.Cout, p.kh, p.kw, p.sh, p.sw, p.ph, p.pw, p.dh, p.dw, p.groups, p.dg, &p.Ho, &p.Wo);
}
static int dc_bwd_reqs(const DcBwdParams &p) {
  if (!req_ok(p.req_x) || !req_ok(p.req_offset) || !req_ok(p.req_w) || !req_ok(p.req_bias))
    return fail(MFN_E_PARAM, "deform_conv_bwd: req must be 0 (null), 1 (write) or 3 (add)");
  if ((p.N != 0 && ((p.req_x && !p.gx) || (p.req_offset && !p.goffset))) || (p.req_w && !p.gw) || (p.req_bias && !p.gbias))
    return fail(MFN_E_NULL, "deform_conv_bwd: NULL gradient output");
  return 0;
}
static int dc_bwd_empty(const DcBwdParams &p, hipStream_t s) {   // empty batch: the parameter gradients are zero
  int rc = p.req_w == MFN_REQ_WRITE ? fill_zero_launch(p.gw, (size_t)p.Cout * (p.Cin / p.groups) * p.kh * p.kw, s) : 0;
  if (!rc && p.req_bias == MFN_REQ_WRITE) rc = fill_zero_launch(p.gbias, (size_t)p.Cout, s);
  return hipfail(rc, "deform_conv_bwd");
}
static int dc_bwd_run(const Settings &st, DcBwdParams p, void *workspace, size_t ws_bytes, hipStream_t s) {
  int rc = dc_bwd_dims("deform_conv_bwd", p);
  if (rc) return rc;
  if (p.N != 0 && !p.offset) return fail(MFN_E_NULL, "deform_conv_bwd: NULL offset");
  if ((rc = dc_bwd_reqs(p))) return rc;
  if (p.N == 0) return dc_bwd_empty(p, s);
  const DcBwdPlan pl = dc_bwd_plan(st, p, false, aligned(p.x, 16), aligned(p.w, 16), workspace && aligned(workspace, 16) ? ws_bytes : 0);
  return hipfail(dc_bwd_exec(pl, p, workspace, nullptr, s), "deform_conv_bwd");
}

int MFN_API(deform_conv_bwd)(const float *gout, const float *x, const float *offset, const float *w, float *gx,
                             float *goffset, float *gw, float *gbias, int N, int Cin, int H, int W, int Cout, int kh,
                             int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int dg, int req_x,
                             int req_offset, int req_w, int req_bias, void *workspace, size_t ws_bytes, void *stream) {
  const DcBwdParams p{gout, x, offset, w, gx, goffset, gw, gbias, N, Cin, H, W, Cout, 0, 0, kh, kw, sh, sw, ph, pw, dh, dw,
                      groups, dg, req_x, req_offset, req_w, req_bias, 1};
  return dc_bwd_run(settings_now(), p, workspace, ws_bytes, (hipStream_t)stream);
}

// gradient of mfn_offsets_from_flow
static int offsets_from_flow_bwd_run(const float *goffset, float *gflow, int N, int H, int W, int taps, float scale, float stride, int req,
                                     hipStream_t s) {
  const size_t total = (size_t)N * 2 * H * W;
  if (!total) return 0;
  OffsetsBwdParams p{goffset, gflow, N, H, W, taps, scale, stride, req};
  return hipfail(launch("offsets_from_flow_bwd", offsets_from_flow_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p),
                 "offsets_from_flow_bwd");
}
int MFN_API(offsets_from_flow_bwd)(const float *goffset, float *gflow, int N, int H, int W, int taps, float scale, float stride,
                                   int req, void *stream) {
  if (N != 0 && (!goffset || !gflow)) return fail(MFN_E_NULL, "offsets_from_flow_bwd: NULL tensor pointer");
  if (N < 0 || H <= 0 || W <= 0 || taps < 1) return fail(MFN_E_SHAPE, "offsets_from_flow_bwd: bad shape");
  if (stride == 0.f) return fail(MFN_E_PARAM, "offsets_from_flow_bwd: stride must be non-zero");
  if (req != MFN_REQ_WRITE && req != MFN_REQ_ADD) return fail(MFN_E_PARAM, "offsets_from_flow_bwd: req must be 1 (write) or 3 (add)");
  return offsets_from_flow_bwd_run(goffset, gflow, N, H, W, taps, scale, stride, req, (hipStream_t)stream);
}

// Backward of the fused call (mfn_deform_conv_shared_fwd): where the plan has no flow mode the offsets and their gradient live in the
// workspace, [offset N x 2T x H x W][goffset, the same][workspace of mfn_deform_conv_bwd]
static size_t dc_shared_bwd_off_bytes(int N, int H, int W, int kh, int kw) {
  return ((size_t)N * 2 * kh * kw * H * W * sizeof(float) + 255) / 256 * 256;
}
size_t MFN_API(deform_conv_shared_bwd_workspace_bytes)(int N, int Cin, int H, int W, int Cout, int kh, int kw, int ph, int pw,
                                                       int dh, int dw, int groups) {
  if (N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || kh <= 0 || kw <= 0) return 0;
  return 2 * dc_shared_bwd_off_bytes(N, H, W, kh, kw) + dc_bwd_ws_bytes(settings_now(), N, Cin, H, W, Cout, kh, kw, 1, 1, ph, pw, dh, dw, groups, 1);
}
int MFN_API(deform_conv_shared_bwd)(const float *gout, const float *x, const float *flow, float flow_scale, float flow_stride,
                                    const float *w, float *gx, float *gflow, float *gw, float *gbias, int N, int Cin, int H,
                                    int W, int Cout, int kh, int kw, int ph, int pw, int dh, int dw, int groups, int req_x,
                                    int req_flow, int req_w, int req_bias, void *workspace, size_t ws_bytes, void *stream) {
  const Settings st = settings_now();
  if (N != 0 && !flow) return fail(MFN_E_NULL, "deform_conv_shared_bwd: NULL flow");
  if (flow_stride == 0.f) return fail(MFN_E_PARAM, "deform_conv_shared_bwd: flow_stride must be non-zero");
  if (!req_ok(req_flow)) return fail(MFN_E_PARAM, "deform_conv_shared_bwd: req must be 0 (null), 1 (write) or 3 (add)");
  if (N != 0 && req_flow && !gflow) return fail(MFN_E_NULL, "deform_conv_shared_bwd: NULL gradient output");
  DcBwdParams p{gout, x, nullptr, w, gx, gflow, gw, gbias, N, Cin, H, W, Cout, 0, 0, kh, kw, 1, 1, ph, pw, dh, dw, groups, 1,
                req_x, req_flow, req_w, req_bias, 1};
  int rc = dc_bwd_dims("deform_conv_shared_bwd", p);
  if (rc) return rc;
  if (p.Ho != H || p.Wo != W)
    return fail(MFN_E_SHAPE, "deform_conv_shared_bwd: the flow-shared form needs Ho == H and Wo == W (got %dx%d -> %dx%d)", H, W, p.Ho, p.Wo);
  const size_t ob = dc_shared_bwd_off_bytes(N, H, W, kh, kw);
  if (N != 0 && (!workspace || ws_bytes < 2 * ob || !aligned(workspace, 16)))
    return fail(MFN_E_PARAM, "deform_conv_shared_bwd: workspace of mfn_deform_conv_shared_bwd_workspace_bytes (16-byte aligned) required");
  if ((rc = dc_bwd_reqs(p))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return dc_bwd_empty(p, s);
  float *off = (float *)workspace, *goff = (float *)((char *)workspace + ob);
  void *inner = (char *)workspace + 2 * ob;   // 16-byte aligned, as the workspace is
  const bool x16 = aligned(x, 16), w16 = aligned(w, 16);
  const DcBwdPlan pl = dc_bwd_plan(st, p, true, x16, w16, ws_bytes - 2 * ob);
  if (pl.flow_ok) {   // the lane = pixel kernels take the flow field itself: no offsets, no per-tap offset gradient
    const DcFlowArgs fl{flow, flow_scale, flow_stride};
    return hipfail(dc_bwd_exec(pl, p, inner, &fl, s), "deform_conv_bwd");
  }
  if ((rc = offsets_from_flow_run(st, flow, off, N, H, W, kh * kw, flow_scale, flow_stride, s))) return rc;
  p.offset = off; p.goffset = goff; p.req_offset = req_flow ? MFN_REQ_WRITE : MFN_REQ_NULL;
  rc = hipfail(dc_bwd_exec(dc_bwd_plan(st, p, false, x16, w16, ws_bytes - 2 * ob), p, inner, nullptr, s), "deform_conv_bwd");
  if (rc || !req_flow) return rc;
  return offsets_from_flow_bwd_run(goff, gflow, N, H, W, kh * kw, flow_scale, flow_stride, req_flow, s);
}

// ---- Convolution / Deconvolution (SURVEY.md 8 f-4b) ---------------------------------------------------------------
struct ConvPlan {
  int few;    // 1: conv_few_kernel (3x3 / stride 1 / pad 1 / dilation 1 with <= 4 filters: the prediction heads); plain weights
  int mfma;   // 0: generic kernel (or `few`)
  int mma;    // 1: bf16 x 3 operand split on the matrix cores (conv.mma; 3x3 kinds, measured variant, not the default)
  int mt, pt, mgroups, ncp_pad, cps_per_slice, kc;
  int tiles_x, tiles_y, ntiles;
  size_t wt_bytes;
  // dcm: dc_mma_kernel<mt, pt, kw, 3, CONV> (the matrix-core deformable kernel's plain-convolution form): 16-channel groups (the last one
  // zero padded), groups per K slice, words of one M-group of the packed weights
  int dcm, kw, groups16, gps;
  size_t mg_words;
};
// the (filter tiles per wave, pixel tiles per block, K slices) dc_mma_kernel<.., CONV = true> is instantiated for
#ifndef MFN_DCMC_CONFIGS
#define MFN_DCMC_CONFIGS(X) X(1, 4, 1) X(2, 4, 1) X(3, 4, 1) X(2, 3, 4)
#endif
// which MFMA family: 1 = 3x3 convolution, 2 = 4x4 transposed (masked taps), 3 = the network's 4x4 / stride 2 / pad 1
// transposed convolution as a 3x3 convolution with 4*Cout pseudo-filters on the input grid (conv.h, shuffle2)
struct ConvGeo { int sh, sw, ph, pw, dh, dw, adj_h, adj_w; };
static int conv_kind(int kh, int kw, int transposed, const ConvGeo &g) {
  if (!transposed && kh == 3 && kw == 3) return 1;
  if (transposed && kh == 4 && kw == 4) {
    if (g.sh == 2 && g.sw == 2 && g.ph == 1 && g.pw == 1 && g.dh == 1 && g.dw == 1 && !g.adj_h && !g.adj_w) return 3;
    return 2;
  }
  // 4 = the data gradient of the pyramid's 3x3 / stride 2 / pad 1 convolutions: a 3x3 / stride 2 / pad 1 / adj 1 transposed
  // convolution (output exactly 2H x 2W), run like 3 -- output row 2y+py takes input rows {y} (py = 0: kernel row 1) or
  // {y, y+1} (py = 1: kernel rows 2, 0); the generic kernel took 2.3 ms per such layer in the training step
  if (transposed && kh == 3 && kw == 3 && g.sh == 2 && g.sw == 2 && g.ph == 1 && g.pw == 1 && g.dh == 1 && g.dw == 1 && g.adj_h == 1 &&
      g.adj_w == 1)
    return 4;
  return 0;
}
// Ho / Wo: the output grid the kernel's pixel tiles cover (kind 3: the INPUT grid), Cout: its filter count (kind 3: 4x)
static ConvPlan conv_plan(const Settings &st, int N, int Cin, int Cout, int Ho, int Wo, int kh, int kw, int groups, int kind) {
  ConvPlan pl;
  memset(&pl, 0, sizeof(pl));
  if (!kind || groups != 1 || Wo < 8 || (st.t.path_generic & 4)) return pl;
  if (kind == 3) { kh = kw = 3; }
  pl.mfma = 1;
  pl.tiles_x = (Wo + 7) / 8;
  pl.tiles_y = (Ho + 3) / 4;
  pl.ntiles = N * pl.tiles_y * pl.tiles_x;
  const int mtiles = (Cout + 31) / 32;
  const int T = kh * kw;
  int mt = kind == 2 ? 1 : (mtiles >= 4 ? 4 : mtiles);
  if (kind != 2 && mtiles > 4 && mtiles % 4 != 0 && mtiles % 3 == 0) mt = 3;
  int pt = 4;
  // few pixel tiles (coarse pyramid levels): one pixel tile per block with four in-block K slices, and one 32-filter tile
  // per wave so that the filter tiles spread over more workgroups
  if ((long)((pl.ntiles + 3) / 4) * ((mtiles + mt - 1) / mt) < 256) {
    pt = 1;
    if (mt > 2) mt = 2;   // four K slices' weight chunks share the stage buffers: two filter tiles per wave at most
    while (mt > 1 && (long)pl.ntiles * ((mtiles + mt - 1) / mt) < 512) --mt;
    // three filter tiles as 2 + 1 leave every other block with half the work: one tile per wave (profiles/r04_conv_plan_sweep.txt:
    // conv3_2 251 -> 228 us, conv4a / 4b / 4c 31 / 44 / 42 -> 26 / 36 / 36)
    if (mt == 2 && mtiles == 3) mt = 1;
  }
  if (st.t.conv_mt >= 1 && st.t.conv_mt <= 4 && kind != 2) mt = st.t.conv_mt;
  if (st.t.conv_pt == 1 || st.t.conv_pt == 4) pt = st.t.conv_pt;
  if (pt == 1 && mt > 2) mt = 2;
  pl.mma = (st.conv != 0 && kind != 2 && T == 9) ? 1 : 0;   // the bf16 x 3 form unless the thread asked for fp32 FMA chains
  if (pl.mma) {   // the instantiations of the bf16 x 3 form: (1,1), (1,4), (2,4), (4,4)
    if (pt == 1) mt = 1;
    else if (mt == 3) mt = 2;
  }
  pl.mt = mt;
  pl.pt = pt;
  pl.mgroups = (mtiles + mt - 1) / mt;
  const int RL = 32 * mt;
  pl.kc = pl.mma ? conv_kc_mma(mt, pt) : conv_kc(mt, pt, T);
  const int ks = 4 / pt, ncp = (Cin + 1) / 2;
  pl.cps_per_slice = (((ncp + ks - 1) / ks + pl.kc - 1) / pl.kc) * pl.kc;
  pl.ncp_pad = ks * pl.cps_per_slice + pl.kc;
  pl.wt_bytes = (((size_t)pl.mgroups * pl.ncp_pad * (pl.mma ? mt * DC_PAIR_W_BF16 : T * 2 * RL) * sizeof(float)) + 255) / 256 * 256;
  return pl;
}
// Plain 3x3 / stride 1 / pad 1 / dilation 1 convolutions with whole 32-filter tiles on images of at least 384 pixel tiles (levels 2 and 3
// of the 384x512 batch-8 network): dc_mma_kernel's CONV form.  Measured against conv_mfma_kernel's bf16 x 3 form, same boxes
// (profiles/r05_conv_dcm.txt): level-2 decoder layers 1.2-1.6x, level 3 1.6-1.8x, level 4 (192 tiles) no gain -- left where it was.
static bool conv_dcm_plan(const Settings &st, ConvPlan &pl, int N, int Cin, int Cout, int H, int W) {
  if (st.t.conv_dcm == 1 || st.conv == 0 || (st.t.path_generic & 4) || st.t.conv_mt || st.t.conv_pt) return false;
  if (Cout < 32 || W % 4 != 0 || W < 8) return false;   // (a 16-filter layer would fill half a tile)
  const int tiles_x = (W + 7) / 8, tiles_y = (H + 3) / 4;
  const long tiles = (long)N * tiles_y * tiles_x;
  if (tiles < 384 && st.t.conv_dcm != 2) return false;
  memset(&pl, 0, sizeof(pl));
  pl.dcm = 1;
  pl.tiles_x = tiles_x; pl.tiles_y = tiles_y; pl.ntiles = (int)tiles;
  pl.groups16 = (Cin + 15) / 16;
  // filter tiles per wave: the B operand of a pixel tile costs ~2.5 units per M-group that forms it and a filter tile ~4.2 (from the
  // level-2 layers: one tile per wave 150 TFLOP/s, three 199); a filter count that is no multiple of 32 * mt pads the last M-group with
  // zero filters (the data gradients of the decoder: 131, 259, 387 ... filters)
  const int mtiles = (Cout + 31) / 32;
  int mt = 1, pt = 4, kw = 1;
  double best = 1e30;
  for (int cand = 3; cand >= 1; --cand) {
    const double cost = (double)((mtiles + cand - 1) / cand) * (2.45 + 4.2 * cand);
    if (cost < best - 1e-9) { best = cost; mt = cand; }
  }
  // few tiles and two filter tiles (level 3's 64-filter layers): three pixel tiles x four K slices, as the deformable convolution there
  if (tiles < 1024 && mt == 2 && pl.groups16 % 4 == 0) { pt = 3; kw = 4; }
  if (st.t.dc_pt > 0 && kw == 1) pt = st.t.dc_pt;   // measurement (a build that instantiates it: MFN_DCMC_CONFIGS)
  pl.mt = mt; pl.pt = pt; pl.kw = kw;
  pl.mgroups = (mtiles + mt - 1) / mt;
  pl.gps = pl.groups16 / kw;
  pl.mg_words = (size_t)(pl.groups16 * 9 + dcm_kc(mt, kw)) * (3 * mt * 256);
  pl.wt_bytes = (pl.mgroups * pl.mg_words * sizeof(float) + 255) / 256 * 256;
  return true;
}
static unsigned long long conv_layout_tag(const ConvPlan &pl, int T, int kind) {
  if (pl.dcm)
    return 0x4d44000000000000ull | ((unsigned long long)pl.mt << 40) | ((unsigned long long)pl.mgroups << 32) |
           ((unsigned long long)dcm_kc(pl.mt, pl.kw) << 24) | (unsigned long long)(unsigned)pl.groups16;
  return 0x4d43000000000000ull | ((unsigned long long)pl.mma << 47) | ((unsigned long long)(kind & 1) << 46) | ((unsigned long long)((kind >> 1) & 1) << 45) | ((unsigned long long)T << 40) |
         ((unsigned long long)pl.mt << 36) | ((unsigned long long)pl.mgroups << 28) | ((unsigned long long)(kind == 4) << 27) |
         (unsigned long long)(unsigned)pl.ncp_pad;
}
static const unsigned long long kConvPlainTag = 0x4d43ffff00000000ull;

int MFN_API(conv2d_out_shape)(int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int transposed,
                              int adj_h, int adj_w, int *Ho, int *Wo) {
  if (H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "conv2d: H=%d W=%d must be positive", H, W);
  if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1 || ph < 0 || pw < 0)
    return fail(MFN_E_PARAM, "conv2d: bad kernel / stride / dilate / pad");
  int ho, wo;
  if (transposed) {
    if (adj_h < 0 || adj_w < 0 || adj_h >= sh || adj_w >= sw) return fail(MFN_E_PARAM, "Deconvolution: adj must be smaller than stride");
    ho = (H - 1) * sh - 2 * ph + dh * (kh - 1) + 1 + adj_h;
    wo = (W - 1) * sw - 2 * pw + dw * (kw - 1) + 1 + adj_w;
  } else {
    if (adj_h || adj_w) return fail(MFN_E_PARAM, "Convolution: adj is a Deconvolution parameter");
    const int eh = dh * (kh - 1) + 1, ew = dw * (kw - 1) + 1;
    if (H + 2 * ph < eh || W + 2 * pw < ew) return fail(MFN_E_SHAPE, "Convolution: kernel size exceed input");
    ho = (H + 2 * ph - eh) / sh + 1;
    wo = (W + 2 * pw - ew) / sw + 1;
  }
  if (ho < 1 || wo < 1) return fail(MFN_E_SHAPE, "conv2d: empty output");
  if (Ho) *Ho = ho;
  if (Wo) *Wo = wo;
  return 0;
}

static int conv_dims(const char *what, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                     int dw, int groups, int transposed, int adj_h, int adj_w, int *Ho, int *Wo) {
  if (N < 0 || Cin <= 0 || Cout <= 0) return fail(MFN_E_SHAPE, "%s: N=%d Cin=%d Cout=%d", what, N, Cin, Cout);
  if (groups < 1 || Cin % groups || Cout % groups) return fail(MFN_E_SHAPE, "%s: channels must divide num_group=%d", what, groups);
  if ((size_t)H * W >= ((size_t)1 << 29) || (size_t)N * Cin * H * W >= ((size_t)1 << 31))
    return fail(MFN_E_UNSUPPORTED, "%s: input tensor too large for 32-bit element offsets", what);
  return MFN_API(conv2d_out_shape)(H, W, kh, kw, sh, sw, ph, pw, dh, dw, transposed, adj_h, adj_w, Ho, Wo);
}

// kernel family + plan of a call; CoutK / HoK / WoK / T describe the problem the MFMA kernel sees (kind 3: the pseudo
// 3x3 convolution on the input grid), pack_mode is conv_pack_weights_kernel's `transposed`
struct ConvSetup { int kind, T, CoutK, HoK, WoK, pack_mode; ConvPlan pl; };
static ConvSetup conv_setup(const Settings &st, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                            int groups, int transposed, int adj_h, int adj_w, int Ho, int Wo, bool allow_dcm = true) {
  ConvSetup cs;
  const ConvGeo g{sh, sw, ph, pw, dh, dw, adj_h, adj_w};
  cs.kind = conv_kind(kh, kw, transposed, g);
  if (cs.kind >= 3) { cs.T = 9; cs.CoutK = 4 * Cout; cs.HoK = H; cs.WoK = W; cs.pack_mode = cs.kind == 3 ? 2 : 3; }
  else { cs.T = kh * kw; cs.CoutK = Cout; cs.HoK = Ho; cs.WoK = Wo; cs.pack_mode = transposed ? 1 : 0; }
  cs.pl = conv_plan(st, N, Cin, cs.CoutK, cs.HoK, cs.WoK, kh, kw, groups, cs.kind);
  // the prediction heads: a channel reduction with 1-4 filters does not belong on a 32-filter matrix tile
  if (cs.kind == 1 && Cout <= 4 && groups == 1 && sh == 1 && sw == 1 && ph == 1 && pw == 1 && dh == 1 && dw == 1 && conv_few_shape_ok(W) &&
      !(st.t.path_generic & 4) && st.t.conv_mt == 0 && st.t.conv_pt == 0) {
    memset(&cs.pl, 0, sizeof(cs.pl));
    cs.pl.few = 1;
  }
  if (allow_dcm && cs.kind == 1 && !cs.pl.few && cs.pl.mfma &&
      dcm_conv_shape_ok(N, (size_t)Cin * H * W, H, W, kh, kw, sh, sw, ph, pw, dh, dw, groups))
    conv_dcm_plan(st, cs.pl, N, Cin, Cout, H, W);
  if (cs.pl.dcm) cs.pl.mfma = 1;
  return cs;
}

static size_t conv_packed_bytes(const ConvSetup &cs, int Cin, int Cout, int kh, int kw, int groups) {
  return cs.pl.mfma ? cs.pl.wt_bytes : (((size_t)Cout * (Cin / groups) * kh * kw * sizeof(float)) + 15) / 16 * 16;
}
size_t MFN_API(conv2d_packed_weight_bytes)(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                                           int dh, int dw, int groups, int transposed) {
  int Ho, Wo;
  if (conv_dims("conv2d", N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, 0, 0, &Ho, &Wo)) return 0;
  return conv_packed_bytes(conv_setup(settings_now(), N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, 0, 0, Ho, Wo), Cin, Cout,
                           kh, kw, groups);
}
// workspace of a forward call that is given `w` instead of a packed buffer (adj: a Deconvolution's; the size query has none)
static size_t conv_ws_bytes(const Settings &st, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                            int groups, int transposed, int adj_h = 0, int adj_w = 0) {
  int Ho, Wo;
  if (conv_dims("conv2d", N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, &Ho, &Wo)) return 0;
  const ConvSetup cs = conv_setup(st, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, Ho, Wo);
  if (cs.pl.few) return conv_few_workspace_bytes(N, Cin, H, W, Cout);   // partial sums of the channel blocks (coarse levels)
  if (cs.pl.dcm) {   // a call whose tensors are not 16-byte aligned packs for conv_mfma_kernel instead: room for either
    const ConvSetup c2 = conv_setup(st, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, Ho, Wo, false);
    return cs.pl.wt_bytes > c2.pl.wt_bytes ? cs.pl.wt_bytes : c2.pl.wt_bytes;
  }
  return cs.pl.mfma ? cs.pl.wt_bytes : 0;   // the re-laid-out weights
}
size_t MFN_API(conv2d_workspace_bytes)(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                                       int dh, int dw, int groups, int transposed) {
  const Settings st = settings_now();
  size_t need = conv_ws_bytes(st, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed);
  // the query has no adj, the call does, and the kernel family depends on it: room for every adj the call accepts
  int Ho, Wo;
  if (!transposed || conv_dims("conv2d", N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, 0, 0, &Ho, &Wo)) return need;
  for (int ah = 0; ah < sh; ++ah)
    for (int aw = 0; aw < sw; ++aw) {
      if (!ah && !aw) continue;
      const size_t b = conv_ws_bytes(st, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, ah, aw);
      need = need > b ? need : b;
    }
  return need;
}

int MFN_API(conv2d_pack_weights)(const float *w, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph,
                                 int pw, int dh, int dw, int groups, int transposed, void *packed, size_t packed_bytes,
                                 unsigned long long *layout_tag, void *stream) {
  int Ho, Wo;
  int rc = conv_dims("conv2d_pack_weights", N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, 0, 0, &Ho, &Wo);
  if (rc) return rc;
  if (!w || !packed || !layout_tag) return fail(MFN_E_NULL, "conv2d_pack_weights: NULL pointer");
  if (!aligned(packed, 16)) return fail(MFN_E_ALIGN, "conv2d_pack_weights: packed buffer must be 16-byte aligned");
  const ConvSetup cs = conv_setup(settings_now(), N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, 0, 0, Ho, Wo);
  const size_t need = conv_packed_bytes(cs, Cin, Cout, kh, kw, groups);
  if (packed_bytes < need) return fail(MFN_E_WORKSPACE, "conv2d_pack_weights: %zu bytes required (got %zu)", need, packed_bytes);
  if (!cs.pl.mfma) {
    *layout_tag = kConvPlainTag;
    return hipfail(dc_copy_launch(w, (float *)packed, (size_t)Cout * (Cin / groups) * kh * kw, (hipStream_t)stream), "conv2d_pack_weights");
  }
  *layout_tag = conv_layout_tag(cs.pl, cs.T, cs.kind);
  if (cs.pl.dcm)
    return hipfail(dcm_pack_launch(DcmPackParams{w, (float *)packed, Cin, Cout, cs.pl.mt, cs.pl.mgroups, cs.pl.groups16, cs.pl.mg_words},
                                   (hipStream_t)stream), "conv2d_pack_weights");
  ConvPackParams pp{w, (float *)packed, Cin, cs.CoutK, 32 * cs.pl.mt, cs.pl.mgroups, cs.pl.ncp_pad, cs.T, cs.pack_mode};
  return hipfail(cs.pl.mma ? conv_pack_bf16_launch(pp, (hipStream_t)stream) : conv_pack_launch(pp, (hipStream_t)stream), "conv2d_pack_weights");
}

static int conv_fwd_common(const Settings &st, const float *x, long long in_batch_stride, const float *w_or_null, const void *packed_or_null,
                           size_t packed_bytes, unsigned long long layout_tag, const float *bias_or_null, float *out,
                           long long out_batch_stride, int N,
                           int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                           int transposed, int adj_h, int adj_w, int activation, void *workspace, size_t workspace_bytes,
                           void *stream) {
  const char *what = transposed ? "conv2d_transpose_fwd" : "conv2d_fwd";
  int Ho, Wo;
  int rc = conv_dims(what, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, &Ho, &Wo);
  if (rc) return rc;
  if ((!w_or_null && !packed_or_null) || (N != 0 && (!x || !out))) return fail(MFN_E_NULL, "%s: NULL tensor pointer", what);
  if (activation != MFN_ACT_NONE && activation != MFN_ACT_LEAKY_0_1) return fail(MFN_E_PARAM, "%s: unknown activation %d", what, activation);
  if (N == 0) return 0;
  const size_t dense = (size_t)Cout * Ho * Wo;
  const size_t onst = out_batch_stride > 0 ? (size_t)out_batch_stride : dense;
  if (onst < dense) return fail(MFN_E_SHAPE, "%s: out_batch_stride %lld is smaller than one output image (%zu)", what, out_batch_stride, dense);
  const size_t xdense = (size_t)Cin * H * W;
  const size_t xnst = in_batch_stride > 0 ? (size_t)in_batch_stride : xdense;
  if (xnst < xdense) return fail(MFN_E_SHAPE, "%s: in_batch_stride %lld is smaller than one input image (%zu)", what, in_batch_stride, xdense);
  if ((size_t)N * xnst >= ((size_t)1 << 31)) return fail(MFN_E_UNSUPPORTED, "%s: input buffer too large for 32-bit element offsets", what);
  if (!aligned(x, 4) || !aligned(out, 4)) return fail(MFN_E_ALIGN, "%s: pointers must be 4-byte aligned", what);
  hipStream_t s = (hipStream_t)stream;
  ConvParams p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.w = w_or_null; p.bias = bias_or_null; p.out = out;
  p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout; p.Ho = Ho; p.Wo = Wo;
  p.kh = kh; p.kw = kw; p.sh = sh; p.sw = sw; p.ph = ph; p.pw = pw; p.dh = dh; p.dw = dw; p.groups = groups;
  p.transposed = transposed ? 1 : 0;
  p.out_nstride = onst;
  p.x_nstride = xnst;
  p.leaky = activation == MFN_ACT_LEAKY_0_1;
  // the matrix-core deformable kernel's convolution form wants 16-byte rows in both tensors and offsets below 2^32 bytes; a call that is
  // given `w` (packed here, per call) and does not qualify takes conv_mfma_kernel, one with weights PACKED for it is refused
  const bool dcm_call_ok = aligned(x, 16) && aligned(out, 16) && xnst % 4 == 0 && onst % 4 == 0 && (size_t)N * xnst < ((size_t)1 << 30);
  ConvSetup cs = conv_setup(st, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, Ho, Wo);
  if (cs.pl.dcm && !dcm_call_ok) {
    if (packed_or_null)
      return fail(MFN_E_ALIGN, "%s: weights packed for the matrix-core convolution need x / out 16-byte aligned with batch strides that are multiples of 4 "
                  "(and N * in_batch_stride < 2^30)", what);
    cs = conv_setup(st, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, Ho, Wo, false);
  }
  const ConvPlan &pl = cs.pl;
  if (!pl.mfma) {
    if (packed_or_null) {
      if (layout_tag != kConvPlainTag) return fail(MFN_E_WORKSPACE, "%s: packed weights were laid out for another plan", what);
      p.w = (const float *)packed_or_null;
    }
    if (pl.few && aligned(x, 16) && aligned(out, 16) && xnst % 4 == 0 && onst % 4 == 0)
      return hipfail(conv_few_launch(p, workspace, workspace_bytes, s), what);
    return hipfail(conv_generic_launch(p, s), what);
  }
  if (packed_or_null) {
    if (packed_bytes < pl.wt_bytes || layout_tag != conv_layout_tag(pl, cs.T, cs.kind))
      return fail(MFN_E_WORKSPACE, "%s: packed weights (%zu bytes, layout %llx) do not match this shape/tuning (%zu bytes, layout %llx): "
                  "re-run mfn_conv2d_pack_weights", what, packed_bytes, layout_tag, pl.wt_bytes, conv_layout_tag(pl, cs.T, cs.kind));
    if (!aligned(packed_or_null, 16)) return fail(MFN_E_ALIGN, "%s: packed weights must be 16-byte aligned", what);
    p.wt = (const float *)packed_or_null;
  } else {
    if (!workspace || workspace_bytes < pl.wt_bytes)
      return fail(MFN_E_WORKSPACE, "%s: workspace of %zu bytes required (got %zu)", what, pl.wt_bytes, workspace ? workspace_bytes : (size_t)0);
    if (!aligned(workspace, 16)) return fail(MFN_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
    if (pl.dcm) rc = dcm_pack_launch(DcmPackParams{w_or_null, (float *)workspace, Cin, Cout, pl.mt, pl.mgroups, pl.groups16, pl.mg_words}, s);
    else {
      ConvPackParams pp{w_or_null, (float *)workspace, Cin, cs.CoutK, 32 * pl.mt, pl.mgroups, pl.ncp_pad, cs.T, cs.pack_mode};
      rc = pl.mma ? conv_pack_bf16_launch(pp, s) : conv_pack_launch(pp, s);
    }
    if (rc) return hipfail(rc, what);
    p.wt = (const float *)workspace;
  }
  if (pl.dcm) {
    DeformParams q;
    memset(&q, 0, sizeof(q));
    q.x = x; q.wt = p.wt; q.bias = bias_or_null; q.out = out;
    q.N = N; q.Cin = Cin; q.H = H; q.W = W; q.Cout = Cout; q.CoutP = Cout; q.Ho = Ho; q.Wo = Wo;
    q.kh = q.kw = 3; q.sh = q.sw = q.ph = q.pw = q.dh = q.dw = q.groups = q.dg = 1;
    q.P = N * Ho * Wo;
    q.allow_fast = 1;
    q.timeline = (unsigned long long *)g_timeline;
    q.ep_leaky = p.leaky;
    q.mgroups = pl.mgroups;
    q.tile_w = 8; q.tiles_x = pl.tiles_x; q.tiles_y = pl.tiles_y; q.ntiles = pl.ntiles;
    q.inv_tpi = 1.0f / (float)(pl.tiles_y * pl.tiles_x);
    q.inv_tiles_x = 1.0f / (float)pl.tiles_x;
    q.dcm_groups = pl.groups16; q.dcm_gps = pl.gps;
    q.x_nstride = xnst; q.out_nstride = onst;
    q.xcd = pl.mgroups == 1 || cdiv(pl.ntiles, pl.pt) % 8 == 0;
    q.st_policy = 0;   // the next layer reads it
    rc = -1000;
#define X(a, b, c) if (pl.mt == a && pl.pt == b && pl.kw == c) rc = dc_mma_launch<a, b, c, 3, true>(q, s, "conv3x3_dcm");
    MFN_DCMC_CONFIGS(X)
#undef X
    if (rc == -1000) return fail(MFN_E_UNSUPPORTED, "%s: no matrix-core convolution for mt=%d pt=%d kw=%d", what, pl.mt, pl.pt, pl.kw);
    return hipfail(rc, what);
  }
  if (cs.kind >= 3) {   // the kernel sees a 3x3 / stride 1 / pad 1 convolution with 4*Cout filters on the input grid
    p.Cout = cs.CoutK; p.Ho = H; p.Wo = W;
    p.sh = p.sw = 1; p.ph = p.pw = 1; p.dh = p.dw = 1;
    p.shuffle2 = 1;
  }
  p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.ntiles = pl.ntiles;
  p.inv_tpi = 1.0f / (float)(pl.tiles_y * pl.tiles_x);
  p.inv_tiles_x = 1.0f / (float)pl.tiles_x;
  p.ncp_pad = pl.ncp_pad; p.cps_per_slice = pl.cps_per_slice; p.mgroups = pl.mgroups;
  {
    const int gx_ = cdiv(pl.ntiles, pl.pt);
    p.xcd = (pl.mgroups == 1 || gx_ % 8 == 0);
  }
  p.st_policy = 0;   // the next layer reads it
  rc = -1000;
  // one global_load_dwordx3 per kernel row where the three taps of a row are adjacent floats (conv.h ROW3)
  // (measured: a gain only for strided convolutions -- conv1a 30 -> 22 us, conv2a 24 -> 19 us; with stride 1 the lanes'
  // overlapping 12-byte loads are slower than three dword gathers: dc_conv1 1239 -> 1450 us)
  const bool row3 = cs.kind != 2 && p.dw == 1 && p.pw <= 1 && W >= 3 &&
                    (p.sw >= 2);
#define MFN_CONV_CASE(MT_, PT_)                                                                                              \
  if (cs.kind != 2 && pl.mt == MT_ && pl.pt == PT_)                                                                          \
    rc = row3 ? conv_mfma_launch<MT_, PT_, 3, 3, false, true>(p, s, cs.kind >= 3 ? "deconv_as_conv3x3_row_mfma" : "conv3x3_row_mfma") \
              : conv_mfma_launch<MT_, PT_, 3, 3, false, false>(p, s, cs.kind >= 3 ? "deconv_as_conv3x3_mfma" : "conv3x3_mfma");
  if (!pl.mma) {
    MFN_CONV_CASE(1, 1) MFN_CONV_CASE(1, 4) MFN_CONV_CASE(2, 1) MFN_CONV_CASE(2, 4)
    MFN_CONV_CASE(3, 4) MFN_CONV_CASE(4, 4)
  }
#undef MFN_CONV_CASE
#define MFN_CONV_MMA_CASE(MT_, PT_)                                                                                         \
  if (pl.mma && cs.kind != 2 && pl.mt == MT_ && pl.pt == PT_)                                                                \
    rc = conv_mfma_launch<MT_, PT_, 3, 3, false, false, 1>(p, s, cs.kind >= 3 ? "deconv_as_conv3x3_bf16x3" : "conv3x3_bf16x3");
  MFN_CONV_MMA_CASE(1, 1) MFN_CONV_MMA_CASE(1, 4) MFN_CONV_MMA_CASE(2, 4) MFN_CONV_MMA_CASE(4, 4)
#undef MFN_CONV_MMA_CASE
  if (cs.kind == 2 && pl.pt == 1) rc = conv_mfma_launch<1, 1, 4, 4, true>(p, s, "deconv4x4_mfma");
  if (cs.kind == 2 && pl.pt == 4) rc = conv_mfma_launch<1, 4, 4, 4, true>(p, s, "deconv4x4_mfma");
  if (rc == -1000) return fail(MFN_E_UNSUPPORTED, "%s: no kernel for mt=%d pt=%d", what, pl.mt, pl.pt);
  return hipfail(rc, what);
}

int MFN_API(conv2d_fwd)(const float *x, long long in_batch_stride, const float *w_or_null, const void *packed_or_null,
                        size_t packed_bytes, unsigned long long layout_tag, const float *bias_or_null, float *out,
                        long long out_batch_stride, int N,
                        int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                        int transposed, int adj_h, int adj_w, int activation, void *workspace, size_t workspace_bytes,
                        void *stream) {
  return conv_fwd_common(settings_now(), x, in_batch_stride, w_or_null, packed_or_null, packed_bytes, layout_tag, bias_or_null, out,
                         out_batch_stride, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, activation,
                         workspace, workspace_bytes, stream);
}

// ---- backward of the f rows (round 3): Upsample, LeakyReLU, Convolution / Deconvolution -------------------------------
int MFN_API(upsample_bwd)(const float *gout, float *gx, int N, int C, int H, int W, int factor, int req, void *stream) {
  if (!req_ok(req)) return fail(MFN_E_PARAM, "upsample_bwd: req must be 0 (null), 1 (write) or 3 (add)");
  if (N != 0 && req && (!gout || !gx)) return fail(MFN_E_NULL, "upsample_bwd: NULL tensor pointer");
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "upsample_bwd: N=%d C=%d H=%d W=%d", N, C, H, W);
  if (factor < 1) return fail(MFN_E_PARAM, "upsample_bwd: factor=%d must be >= 1", factor);
  if ((size_t)H * factor >= ((size_t)1 << 30) || (size_t)W * factor >= ((size_t)1 << 30))
    return fail(MFN_E_UNSUPPORTED, "upsample_bwd: output plane too large");
  if (N == 0 || !req) return 0;
  UpsampleBwdParams p{gout, gx, N, C, H, W, factor, req == MFN_REQ_ADD ? 1 : 0};
  const size_t total = (size_t)N * C * H * W;
  if (factor >= 8 && total < ((size_t)1 << 31))   // a block per input pixel: the footprint is (2f-1)^2 >= 225 outputs
    return hipfail(launch("upsample_bwd_block", upsample_bwd_block_kernel, dim3((unsigned)total), dim3(256), 256 * sizeof(float),
                          (hipStream_t)stream, p), "upsample_bwd");
  return hipfail(launch("upsample_bwd", upsample_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p),
                 "upsample_bwd");
}

// ---- the fused multiscale training loss (kernels/loss.h) --------------------------------------------------------------------
// what both directions accept; the host arrays are read here and travel to the kernels by value
static int loss_dims(const char *what, const float *const *preds, const int *factors, const float *weights, int n_scales, int N, int H,
                     int W, int robust, float q) {
  if (n_scales < 1 || n_scales > MFN_LOSS_MAX_SCALES)
    return fail(MFN_E_PARAM, "%s: n_scales=%d must be in 1..%d", what, n_scales, MFN_LOSS_MAX_SCALES);
  if (!preds || !factors || !weights) return fail(MFN_E_NULL, "%s: NULL host array (preds, factors, weights)", what);
  if (N < 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "%s: N=%d H=%d W=%d", what, N, H, W);
  for (int s = 0; s < n_scales; ++s) {
    if (factors[s] < 1) return fail(MFN_E_PARAM, "%s: factor %d of scale %d must be >= 1", what, factors[s], s);
    if (factors[s] > LOSS_MAX_FACTOR) return fail(MFN_E_UNSUPPORTED, "%s: factor %d of scale %d is above %d", what, factors[s], s, LOSS_MAX_FACTOR);
    if (H % factors[s] || W % factors[s])
      return fail(MFN_E_SHAPE, "%s: H=%d W=%d is no multiple of the factor %d of scale %d", what, H, W, factors[s], s);
  }
  if (robust && !(q > 0.f)) return fail(MFN_E_PARAM, "%s: the robust form needs q > 0 (got %g)", what, (double)q);
  if (N > 65535 || (size_t)H * W > (size_t)LOSS_SLICE * LOSS_MAX_SLICES) return fail(MFN_E_UNSUPPORTED, "%s: tensor too large", what);
  return 0;
}

size_t MFN_API(multiscale_epe_workspace_bytes)(int N, int H, int W, int n_scales) {
  if (N <= 0 || H <= 0 || W <= 0 || n_scales < 1 || n_scales > MFN_LOSS_MAX_SCALES) return 0;
  return (size_t)N * loss_slices((size_t)H * W) * (n_scales + 1) * sizeof(float);
}

int MFN_API(multiscale_epe_fwd)(const float *const *preds, const int *factors, const float *weights, int n_scales, const float *label,
                                const float *mask, int mask_is_scalar, float eps, int robust, float q, float *loss, float *sums, int N,
                                int H, int W, void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = loss_dims("multiscale_epe_fwd", preds, factors, weights, n_scales, N, H, W, robust, q)) return rc;
  if (N == 0) return 0;
  if (!label || !mask || !loss || !sums) return fail(MFN_E_NULL, "multiscale_epe_fwd: NULL tensor pointer");
  for (int s = 0; s < n_scales; ++s)
    if (!preds[s]) return fail(MFN_E_NULL, "multiscale_epe_fwd: prediction %d is NULL", s);
  const int slices = loss_slices((size_t)H * W);
  const size_t need = (size_t)N * slices * (n_scales + 1) * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(MFN_E_WORKSPACE, "multiscale_epe_fwd: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (!aligned(workspace, 4)) return fail(MFN_E_ALIGN, "multiscale_epe_fwd: workspace must be 4-byte aligned");
  LossFwdParams p{};
  for (int s = 0; s < n_scales; ++s) { p.pred[s] = preds[s]; p.f[s] = factors[s]; p.magic[s] = mfn_make_magic((unsigned)factors[s]); p.w[s] = weights[s]; }
  p.S = n_scales; p.label = label; p.mask = mask; p.partial = (float *)workspace; p.sums = sums; p.loss = loss;
  p.N = N; p.H = H; p.W = W; p.slices = slices; p.mask_scalar = mask_is_scalar ? 1 : 0; p.robust = robust ? 1 : 0;
  p.eps = eps; p.q = q;
  return hipfail(multiscale_epe_fwd_launch(p, (hipStream_t)stream), "multiscale_epe_fwd");
}

int MFN_API(multiscale_epe_bwd)(const float *gloss, const float *const *preds, const int *factors, const float *weights, int n_scales,
                                const float *label, const float *mask, int mask_is_scalar, float eps, int robust, float q,
                                const float *sums, float *const *gpreds, const int *reqs, int N, int H, int W, void *stream) {
  if (int rc = loss_dims("multiscale_epe_bwd", preds, factors, weights, n_scales, N, H, W, robust, q)) return rc;
  if (!gpreds || !reqs) return fail(MFN_E_NULL, "multiscale_epe_bwd: NULL host array (gpreds, reqs)");
  bool any = false;
  for (int s = 0; s < n_scales; ++s) {
    if (!req_ok(reqs[s])) return fail(MFN_E_PARAM, "multiscale_epe_bwd: req of scale %d must be 0 (null), 1 (write) or 3 (add)", s);
    if (N != 0 && reqs[s] && (!preds[s] || !gpreds[s])) return fail(MFN_E_NULL, "multiscale_epe_bwd: prediction %d or its gradient is NULL", s);
    any = any || reqs[s];
  }
  if (N == 0 || !any) return 0;
  if (!gloss || !label || !mask || !sums) return fail(MFN_E_NULL, "multiscale_epe_bwd: NULL tensor pointer");
  for (int s = 0; s < n_scales; ++s) {
    if (!reqs[s]) continue;
    LossBwdParams p{};
    p.pred = preds[s]; p.gpred = gpreds[s]; p.f = factors[s]; p.magic = mfn_make_magic((unsigned)factors[s]); p.add = reqs[s] == MFN_REQ_ADD ? 1 : 0; p.w = weights[s];
    p.label = label; p.mask = mask; p.gloss = gloss; p.sums = sums; p.S1 = n_scales + 1;
    p.N = N; p.H = H; p.W = W; p.h = H / factors[s]; p.wd = W / factors[s];
    p.mask_scalar = mask_is_scalar ? 1 : 0; p.robust = robust ? 1 : 0; p.eps = eps; p.q = q;
    if (int rc = hipfail(multiscale_epe_bwd_launch(p, (hipStream_t)stream), "multiscale_epe_bwd")) return rc;
  }
  return 0;
}

// ---- the trainer's Adam step (kernels/optimizer.h) ---------------------------------------------------------------------------
// what both forms accept of the operator's scalars
static int adam_hyper(const char *what, float beta1, float beta2, float epsilon) {
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
    return fail(MFN_E_PARAM, "%s: beta1=%g and beta2=%g must be in [0, 1)", what, (double)beta1, (double)beta2);
  if (!(epsilon >= 0.f)) return fail(MFN_E_PARAM, "%s: epsilon=%g must be >= 0", what, (double)epsilon);
  return 0;
}
// blocks of a table over these counts, or -1 (a negative count, or more blocks than a launch has)
static long long adam_count_blocks(int n_tensors, const long long *counts) {
  unsigned long long nb = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (counts[i] < 0) return -1;
    nb += adam_blocks_of((unsigned long long)counts[i]);
    if (nb > 0x7FFFFFFFull) return -1;
  }
  return (long long)nb;
}

int MFN_API(adam_update)(float *weight, const float *grad, float *mean, float *var, long long n, float lr, float beta1, float beta2,
                         float epsilon, float wd, float rescale_grad, float clip_gradient, void *stream) {
  if (n < 0) return fail(MFN_E_SHAPE, "adam_update: n=%lld", n);
  if (int rc = adam_hyper("adam_update", beta1, beta2, epsilon)) return rc;
  if (n == 0) return 0;
  if (!weight || !grad || !mean || !var) return fail(MFN_E_NULL, "adam_update: NULL tensor pointer");
  if (!aligned(weight, 4) || !aligned(grad, 4) || !aligned(mean, 4) || !aligned(var, 4))
    return fail(MFN_E_ALIGN, "adam_update: pointers must be 4-byte aligned");
  if (adam_blocks_of((unsigned long long)n) > 0x7FFFFFFFull) return fail(MFN_E_UNSUPPORTED, "adam_update: n=%lld is more than one launch covers", n);
  AdamTensor t{};
  t.w = weight; t.g = grad; t.m = mean; t.v = var; t.n = (unsigned long long)n; t.lr_mult = 1.f; t.wd_mult = 1.f;
  t.aligned16 = adam_aligned16(weight, grad, mean, var) ? 1u : 0u;
  return hipfail(adam_update_launch(t, AdamHyper{lr, beta1, beta2, epsilon, wd, rescale_grad, clip_gradient}, (hipStream_t)stream), "adam_update");
}

size_t MFN_API(multi_adam_table_bytes)(int n_tensors, const long long *counts) {
  if (n_tensors <= 0 || !counts) return 0;
  const long long nb = adam_count_blocks(n_tensors, counts);
  return nb < 0 ? 0 : adam_table_bytes((unsigned)n_tensors, (unsigned long long)nb);
}

int MFN_API(multi_adam_build_table)(int n_tensors, float *const *weights, const float *const *grads, float *const *means,
                                    float *const *vars, const long long *counts, const float *lr_mults, const float *wd_mults,
                                    void *table_host, size_t table_bytes, int *n_blocks, unsigned long long *tag) {
  if (n_tensors < 0) return fail(MFN_E_SHAPE, "multi_adam_build_table: n_tensors=%d", n_tensors);
  if (!n_blocks || !tag) return fail(MFN_E_NULL, "multi_adam_build_table: NULL output (n_blocks, tag)");
  if (n_tensors == 0) {
    *n_blocks = 0;
    *tag = adam_table_tag(0, 0);
    return 0;
  }
  if (!weights || !grads || !means || !vars || !counts) return fail(MFN_E_NULL, "multi_adam_build_table: NULL host array");
  const long long nb = adam_count_blocks(n_tensors, counts);
  if (nb < 0) {
    for (int i = 0; i < n_tensors; ++i)
      if (counts[i] < 0) return fail(MFN_E_SHAPE, "multi_adam_build_table: count %lld of tensor %d", counts[i], i);
    return fail(MFN_E_UNSUPPORTED, "multi_adam_build_table: more blocks than one launch has");
  }
  for (int i = 0; i < n_tensors; ++i) {
    if (counts[i] == 0) continue;
    if (!weights[i] || !grads[i] || !means[i] || !vars[i]) return fail(MFN_E_NULL, "multi_adam_build_table: tensor %d has a NULL pointer", i);
    if (!aligned(weights[i], 4) || !aligned(grads[i], 4) || !aligned(means[i], 4) || !aligned(vars[i], 4))
      return fail(MFN_E_ALIGN, "multi_adam_build_table: the pointers of tensor %d must be 4-byte aligned", i);
  }
  const size_t need = adam_table_bytes((unsigned)n_tensors, (unsigned long long)nb);
  if (!table_host || table_bytes < need)
    return fail(MFN_E_WORKSPACE, "multi_adam_build_table: a table of %zu bytes needed, %zu given", need, table_host ? table_bytes : (size_t)0);
  if (!aligned(table_host, 8)) return fail(MFN_E_ALIGN, "multi_adam_build_table: the table must be 8-byte aligned");
  char *out = (char *)table_host;
  unsigned block = 0;
  for (int i = 0; i < n_tensors; ++i) {
    AdamTensor t{};
    t.w = weights[i]; t.g = grads[i]; t.m = means[i]; t.v = vars[i]; t.n = (unsigned long long)counts[i];
    t.lr_mult = lr_mults ? lr_mults[i] : 1.f;
    t.wd_mult = wd_mults ? wd_mults[i] : 1.f;
    t.aligned16 = adam_aligned16(weights[i], grads[i], means[i], vars[i]) ? 1u : 0u;
    t.first_block = block;
    memcpy(out + (size_t)i * sizeof(AdamTensor), &t, sizeof(t));
    const unsigned chunks = (unsigned)adam_blocks_of(t.n);
    for (unsigned c = 0; c < chunks; ++c, ++block) {
      const AdamBlock b{(unsigned)i, c};
      memcpy(out + (size_t)n_tensors * sizeof(AdamTensor) + (size_t)block * sizeof(AdamBlock), &b, sizeof(b));
    }
  }
  *n_blocks = (int)nb;
  *tag = adam_table_tag((unsigned)n_tensors, (unsigned)nb);
  return 0;
}

int MFN_API(multi_adam_update)(const void *table_dev, size_t table_bytes, unsigned long long tag, int n_tensors, int n_blocks, float lr,
                               float beta1, float beta2, float epsilon, float wd, float rescale_grad, float clip_gradient, void *stream) {
  if (n_tensors < 0 || n_blocks < 0) return fail(MFN_E_SHAPE, "multi_adam_update: n_tensors=%d n_blocks=%d", n_tensors, n_blocks);
  if (int rc = adam_hyper("multi_adam_update", beta1, beta2, epsilon)) return rc;
  if (tag != adam_table_tag((unsigned)n_tensors, (unsigned)n_blocks))
    return fail(MFN_E_WORKSPACE, "multi_adam_update: the table (tag %llx) was not built for %d tensors in %d blocks (tag %llx): "
                "re-run mfn_multi_adam_build_table", tag, n_tensors, n_blocks, adam_table_tag((unsigned)n_tensors, (unsigned)n_blocks));
  if (n_tensors == 0 || n_blocks == 0) return 0;
  const size_t need = adam_table_bytes((unsigned)n_tensors, (unsigned long long)n_blocks);
  if (!table_dev) return fail(MFN_E_NULL, "multi_adam_update: NULL table");
  if (table_bytes != need) return fail(MFN_E_WORKSPACE, "multi_adam_update: a table of %zu bytes expected, %zu given", need, table_bytes);
  if (!aligned(table_dev, 8)) return fail(MFN_E_ALIGN, "multi_adam_update: the table must be 8-byte aligned");
  return hipfail(multi_adam_update_launch(table_dev, (unsigned)n_tensors, (unsigned)n_blocks,
                                          AdamHyper{lr, beta1, beta2, epsilon, wd, rescale_grad, clip_gradient}, (hipStream_t)stream),
                 "multi_adam_update");
}

// ---- one training batch out of a device-resident data set (kernels/batch.h) ---------------------------------------------------
size_t MFN_API(batch_gather_rows_bytes)(int N) { return batch_rows_bytes(N); }

int MFN_API(batch_gather_build_rows)(int N, const void *const *img1, const void *const *img2, const void *const *flow,
                                     const void *const *mask, const int *Hs, const int *Ws, const int *label_type, const int *y0,
                                     const int *x0, const int *flip, int Hc, int Wc, void *rows_host, size_t rows_bytes,
                                     unsigned long long *tag) {
  const char *what = "batch_gather_build_rows";
  if (N <= 0 || Hc <= 0 || Wc <= 0) return fail(MFN_E_SHAPE, "%s: N=%d Hc=%d Wc=%d", what, N, Hc, Wc);
  if (N > 65535 || (long long)Hc * Wc > 0x7FFFFFFFll) return fail(MFN_E_UNSUPPORTED, "%s: N=%d, crop %dx%d is more than one launch covers", what, N, Hc, Wc);
  if (!img1 || !img2 || !flow || !Hs || !Ws || !label_type || !y0 || !x0 || !flip) return fail(MFN_E_NULL, "%s: NULL host array", what);
  if (!rows_host || !tag) return fail(MFN_E_NULL, "%s: NULL output (rows_host, tag)", what);
  if (rows_bytes < batch_rows_bytes(N)) return fail(MFN_E_SHAPE, "%s: a table of %zu bytes needed, %zu given", what, batch_rows_bytes(N), rows_bytes);
  if (!aligned(rows_host, 8)) return fail(MFN_E_ALIGN, "%s: the table must be 8-byte aligned", what);
  for (int n = 0; n < N; ++n) {
    const void *m = mask ? mask[n] : nullptr;
    if (!img1[n] || !img2[n] || !flow[n]) return fail(MFN_E_NULL, "%s: slot %d has a NULL img1, img2 or flow", what, n);
    if (!aligned(img1[n], 16) || !aligned(img2[n], 16) || !aligned(flow[n], 16) || !aligned(m, 16))
      return fail(MFN_E_ALIGN, "%s: the source arrays of slot %d must be 16-byte aligned", what, n);
    if (label_type[n] != BATCH_LABEL_F32 && label_type[n] != BATCH_LABEL_F16)
      return fail(MFN_E_PARAM, "%s: label type %d of slot %d (0 = fp32, 1 = fp16)", what, label_type[n], n);
    if (flip[n] != 0 && flip[n] != 1) return fail(MFN_E_PARAM, "%s: flip %d of slot %d (0 or 1)", what, flip[n], n);
    if (Hs[n] <= 0 || Ws[n] <= 0) return fail(MFN_E_SHAPE, "%s: slot %d is %dx%d", what, n, Hs[n], Ws[n]);
    if (y0[n] < 0 || x0[n] < 0 || (long long)y0[n] + Hc > Hs[n] || (long long)x0[n] + Wc > Ws[n])
      return fail(MFN_E_SHAPE, "%s: the crop %dx%d at (%d, %d) leaves the %dx%d source of slot %d", what, Hc, Wc, y0[n], x0[n], Hs[n], Ws[n], n);
  }
  for (int n = 0; n < N; ++n) {
    BatchRow r{};
    r.img1 = (const unsigned char *)img1[n]; r.img2 = (const unsigned char *)img2[n]; r.flow = flow[n];
    r.mask = (const unsigned char *)(mask ? mask[n] : nullptr);
    r.Hs = Hs[n]; r.Ws = Ws[n]; r.y0 = y0[n]; r.x0 = x0[n];
    r.flip = (unsigned)flip[n]; r.label_type = (unsigned)label_type[n];
    memcpy((char *)rows_host + (size_t)n * sizeof(BatchRow), &r, sizeof(r));
  }
  *tag = batch_rows_tag(N, Hc, Wc);
  return 0;
}

int MFN_API(batch_gather)(const void *rows_dev, size_t rows_bytes, unsigned long long tag, int N, int Hc, int Wc, int with_mask,
                          unsigned char *img1, unsigned char *img2, float *label, unsigned char *mask, void *stream) {
  if (N <= 0 || Hc <= 0 || Wc <= 0) return fail(MFN_E_SHAPE, "batch_gather: N=%d Hc=%d Wc=%d", N, Hc, Wc);
  if (!rows_dev || !img1 || !img2 || !label) return fail(MFN_E_NULL, "batch_gather: NULL table or output");
  if (with_mask && !mask) return fail(MFN_E_NULL, "batch_gather: NULL mask output in a call with a mask");
  if (N > 65535 || (long long)Hc * Wc > 0x7FFFFFFFll) return fail(MFN_E_UNSUPPORTED, "batch_gather: N=%d, crop %dx%d is more than one launch covers", N, Hc, Wc);
  if (rows_bytes != batch_rows_bytes(N)) return fail(MFN_E_SHAPE, "batch_gather: a table of %zu bytes expected for N=%d, %zu given", batch_rows_bytes(N), N, rows_bytes);
  if (tag != batch_rows_tag(N, Hc, Wc))
    return fail(MFN_E_SHAPE, "batch_gather: the table (tag %llx) was not built for N=%d and a %dx%d crop: re-run mfn_batch_gather_build_rows", tag, N, Hc, Wc);
  if (!aligned(rows_dev, 8)) return fail(MFN_E_ALIGN, "batch_gather: the table must be 8-byte aligned");
  if (!aligned(img1, 4) || !aligned(img2, 4) || !aligned(label, 4) || (with_mask && !aligned(mask, 4)))
    return fail(MFN_E_ALIGN, "batch_gather: the output tensors must be 4-byte aligned");
  BatchGatherParams p{};
  p.rows = (const BatchRow *)rows_dev;
  p.img1 = img1; p.img2 = img2; p.label = (unsigned *)label; p.mask = with_mask ? mask : nullptr;
  p.N = N; p.Hc = Hc; p.Wc = Wc;
  p.label16 = aligned(label, 16) ? 1u : 0u;
  return hipfail(batch_gather_launch(p, (hipStream_t)stream), "batch_gather");
}

// ---- a validation batch read through the rows of a resident data set (kernels/validate.h) -----------------------------------------
// what every validate entry accepts: a table for N >= 0 slots of H x W >= 1 x 1, inside what one launch indexes
static int val_dims(const char *what, const void *rows, int N, int H, int W) {
  if (N < 0) return fail(MFN_E_PARAM, "%s: N=%d is negative", what, N);
  if (H < 1 || W < 1) return fail(MFN_E_PARAM, "%s: H=%d W=%d must be >= 1", what, H, W);
  if (N > 32767 || (size_t)H * W * 3 >= ((size_t)1 << 31)) return fail(MFN_E_UNSUPPORTED, "%s: N=%d of %dx%d is more than one launch covers", what, N, H, W);
  if (!aligned(rows, 8)) return fail(MFN_E_ALIGN, "%s: the table must be 8-byte aligned", what);
  return 0;
}

size_t MFN_API(val_pair_mean_workspace_bytes)(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * pred_slices((size_t)2 * H * W) * 3 * sizeof(unsigned);
}

int MFN_API(val_pair_mean)(const void *rows_dev, int N, int H, int W, float *mean, void *workspace, size_t workspace_bytes, void *stream) {
  if (N != 0 && (!rows_dev || !mean)) return fail(MFN_E_NULL, "val_pair_mean: NULL table or mean");
  if (int rc = val_dims("val_pair_mean", rows_dev, N, H, W)) return rc;
  if (N == 0) return 0;
  const size_t plane = (size_t)H * W;
  if (int rc = reduce_dims("val_pair_mean", (size_t)N, 2 * plane)) return rc;
  const int slices = pred_slices(2 * plane);
  const size_t need = (size_t)N * slices * 3 * sizeof(unsigned);
  if (!workspace || workspace_bytes < need)
    return fail(MFN_E_WORKSPACE, "val_pair_mean: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (!aligned(workspace, 4) || !aligned(mean, 4)) return fail(MFN_E_ALIGN, "val_pair_mean: mean and workspace must be 4-byte aligned");
  ValPairMeanParams p{(const BatchRow *)rows_dev,
                      PairMeanU8Params{nullptr, (unsigned *)workspace, mean, plane, 255.0 * (double)(2 * plane), 0, 0, N, slices}};
  return hipfail(val_pair_mean_launch(p, (hipStream_t)stream), "val_pair_mean");
}

int MFN_API(val_preprocess)(const void *rows_dev, int N, int H, int W, const float *mean_or_null, float *out, int Hout, int Wout,
                            void *stream) {
  if (N != 0 && (!rows_dev || !out)) return fail(MFN_E_NULL, "val_preprocess: NULL table or out");
  if (int rc = val_dims("val_preprocess", rows_dev, N, H, W)) return rc;
  if (Hout < 1 || Wout < 1) return fail(MFN_E_PARAM, "val_preprocess: Hout=%d Wout=%d must be >= 1", Hout, Wout);
  if (int rc = resize_dims("val_preprocess", N, 3, H, W, Hout, Wout)) return rc;
  if (N == 0) return 0;
  if (!aligned(out, 4) || !aligned(mean_or_null, 4)) return fail(MFN_E_ALIGN, "val_preprocess: mean and out must be 4-byte aligned");
  ValPreParams p{};
  p.rows = (const BatchRow *)rows_dev; p.mean = mean_or_null; p.out = out;
  p.N = N; p.H = H; p.W = W; p.Hout = Hout; p.Wout = Wout;
  p.ry = Hout > 1 ? (float)(H - 1) / (float)(Hout - 1) : 0.f;
  p.rx = Wout > 1 ? (float)(W - 1) / (float)(Wout - 1) : 0.f;
  p.st_policy = store_policy_for(settings_now(), (size_t)6 * N * Hout * Wout * 4, 2, -1);
  return hipfail(val_pre_launch(p, (hipStream_t)stream), "val_preprocess");
}

size_t MFN_API(val_flow_metrics_workspace_bytes)(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * pred_slices((size_t)H * W) * 3 * sizeof(float);
}

int MFN_API(val_flow_metrics)(const void *rows_dev, const float *flow, int N, int H, int W, float *sums, void *workspace,
                              size_t workspace_bytes, void *stream) {
  if (N != 0 && (!rows_dev || !flow || !sums)) return fail(MFN_E_NULL, "val_flow_metrics: NULL table, flow or sums");
  if (int rc = val_dims("val_flow_metrics", rows_dev, N, H, W)) return rc;
  if (N == 0) return 0;
  const size_t plane = (size_t)H * W;
  if (int rc = reduce_dims("val_flow_metrics", N, plane)) return rc;
  const int slices = pred_slices(plane);
  const size_t need = (size_t)N * slices * 3 * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(MFN_E_WORKSPACE, "val_flow_metrics: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (!aligned(workspace, 4) || !aligned(flow, 4) || !aligned(sums, 4))
    return fail(MFN_E_ALIGN, "val_flow_metrics: flow, sums and workspace must be 4-byte aligned");
  ValMetricsParams p{(const BatchRow *)rows_dev, FlowMetricsParams{flow, nullptr, nullptr, (float *)workspace, sums, plane, N, slices}};
  return hipfail(val_flow_metrics_launch(p, (hipStream_t)stream), "val_flow_metrics");
}

// ---- raw decoded arrays into stored samples (kernels/ingest.h) -------------------------------------------------------------------
size_t MFN_API(ingest_tables_bytes)(int dst_h, int dst_w) { return ingest_tables_bytes(dst_h, dst_w); }

int MFN_API(ingest_build_tables)(int src_h, int src_w, int dst_h, int dst_w, void *tables_host, size_t tables_bytes,
                                 unsigned long long *tag) {
  const char *what = "ingest_build_tables";
  if (src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1) return fail(MFN_E_SHAPE, "%s: source %dx%d, destination %dx%d", what, src_h, src_w, dst_h, dst_w);
  if (!tables_host || !tag) return fail(MFN_E_NULL, "%s: NULL output (tables_host, tag)", what);
  if (tables_bytes < ingest_tables_bytes(dst_h, dst_w))
    return fail(MFN_E_SHAPE, "%s: tables of %zu bytes needed, %zu given", what, ingest_tables_bytes(dst_h, dst_w), tables_bytes);
  if (!aligned(tables_host, 8)) return fail(MFN_E_ALIGN, "%s: the tables must be 8-byte aligned", what);
  ingest_build_tables((IngestTap *)tables_host, src_h, src_w, dst_h, dst_w);
  *tag = ingest_tables_tag(src_h, src_w, dst_h, dst_w);
  return 0;
}

// The window (y0, x0, h, w) of an (H, W, 3) array with `pitch` elements per row: sizes, pitch, the window inside the array.
static int ingest_window(const char *what, int H, int W, long long pitch, int y0, int x0, int h, int w, int min_side) {
  if (H < 1 || W < 1 || h < 1 || w < 1) return fail(MFN_E_SHAPE, "%s: array %dx%d, window %dx%d", what, H, W, h, w);
  if (pitch < 3ll * W) return fail(MFN_E_SHAPE, "%s: a pitch of %lld elements is less than a row of %d pixels (%lld)", what, pitch, W, 3ll * W);
  if (y0 < 0 || x0 < 0 || (long long)y0 + h > H || (long long)x0 + w > W)
    return fail(MFN_E_SHAPE, "%s: the window %dx%d at (%d, %d) leaves the %dx%d array", what, h, w, y0, x0, H, W);
  if (h < min_side || w < min_side) return fail(MFN_E_SHAPE, "%s: a window of %dx%d: both sides must be at least %d", what, h, w, min_side);
  if ((long long)H * pitch > 0x7FFFFFFFll) return fail(MFN_E_UNSUPPORTED, "%s: an array of %d rows of %lld elements is too large", what, H, pitch);
  return 0;
}
static int ingest_tables_ok(const char *what, const void *tables, size_t bytes, unsigned long long tag, int h, int w, int dst_h, int dst_w) {
  if (dst_h < 1 || dst_w < 1) return fail(MFN_E_SHAPE, "%s: destination %dx%d", what, dst_h, dst_w);
  if ((long long)dst_h * dst_w > 0x1FFFFFFFll) return fail(MFN_E_UNSUPPORTED, "%s: a destination of %dx%d is more than one launch covers", what, dst_h, dst_w);
  if (!tables) return fail(MFN_E_NULL, "%s: NULL tables", what);
  if (bytes != ingest_tables_bytes(dst_h, dst_w))
    return fail(MFN_E_SHAPE, "%s: tables of %zu bytes expected for a %dx%d destination, %zu given", what, ingest_tables_bytes(dst_h, dst_w), dst_h, dst_w, bytes);
  if (tag != ingest_tables_tag(h, w, dst_h, dst_w))
    return fail(MFN_E_SHAPE, "%s: the tables (tag %llx) were not built for a %dx%d window and a %dx%d destination: re-run mfn_ingest_build_tables", what, tag,
                h, w, dst_h, dst_w);
  if (!aligned(tables, 16)) return fail(MFN_E_ALIGN, "%s: the tables must be 16-byte aligned", what);
  return 0;
}

int MFN_API(ingest_minmax)(const unsigned char *img1, const unsigned char *img2, int H, int W, long long pitch, int y0, int x0, int h,
                           int w, unsigned *minmax, void *stream) {
  const char *what = "ingest_minmax";
  if (!img1 || !img2 || !minmax) return fail(MFN_E_NULL, "%s: NULL array or output", what);
  if (int rc = ingest_window(what, H, W, pitch, y0, x0, h, w, 1)) return rc;
  if (!aligned(img1, 16) || !aligned(img2, 16)) return fail(MFN_E_ALIGN, "%s: the arrays must be 16-byte aligned", what);
  if (!aligned(minmax, 4)) return fail(MFN_E_ALIGN, "%s: the output must be 4-byte aligned", what);
  IngestMinmaxParams p{};
  p.img1 = img1; p.img2 = img2; p.pitch = pitch; p.y0 = y0; p.x0 = x0; p.h = h; p.w = w; p.out = minmax;
  return hipfail(ingest_minmax_launch(p, (hipStream_t)stream), what);
}

int MFN_API(ingest_image)(const unsigned char *src, int H, int W, long long pitch, int y0, int x0, int h, int w, const void *tables_dev,
                          size_t tables_bytes, unsigned long long tag, int bgr, const unsigned *minmax_or_null, unsigned char *dst,
                          int dst_h, int dst_w, void *stream) {
  const char *what = "ingest_image";
  if (!src || !dst) return fail(MFN_E_NULL, "%s: NULL array or output", what);
  if (int rc = ingest_window(what, H, W, pitch, y0, x0, h, w, 1)) return rc;
  if (int rc = ingest_tables_ok(what, tables_dev, tables_bytes, tag, h, w, dst_h, dst_w)) return rc;
  if (bgr != 0 && bgr != 1) return fail(MFN_E_PARAM, "%s: bgr %d (0 or 1)", what, bgr);
  if (!aligned(src, 16) || !aligned(dst, 16)) return fail(MFN_E_ALIGN, "%s: the array and the output must be 16-byte aligned", what);
  if (!aligned(minmax_or_null, 4)) return fail(MFN_E_ALIGN, "%s: the min/max words must be 4-byte aligned", what);
  IngestImageParams p{};
  p.src = src + (long long)y0 * pitch + 3ll * x0;
  p.pitch = pitch;
  p.cols = (const IngestTap *)tables_dev; p.rows = p.cols + dst_w;
  p.minmax = minmax_or_null; p.dst = dst; p.Hd = dst_h; p.Wd = dst_w; p.bgr = (unsigned)bgr;
  return hipfail(ingest_image_launch(p, (hipStream_t)stream), what);
}

int MFN_API(ingest_flow_occ)(const unsigned short *src, int H, int W, long long pitch, int y0, int x0, int h, int w,
                             const void *tables_dev, size_t tables_bytes, unsigned long long tag, int premultiply, int flow_type,
                             void *flow, unsigned char *mask, int dst_h, int dst_w, void *stream) {
  const char *what = "ingest_flow_occ";
  if (!src || !flow || !mask) return fail(MFN_E_NULL, "%s: NULL array or output", what);
  if (int rc = ingest_window(what, H, W, pitch, y0, x0, h, w, 2)) return rc;
  if (int rc = ingest_tables_ok(what, tables_dev, tables_bytes, tag, h, w, dst_h, dst_w)) return rc;
  if (premultiply != 0 && premultiply != 1) return fail(MFN_E_PARAM, "%s: premultiply %d (0 or 1)", what, premultiply);
  if (flow_type != INGEST_FLOW_F32 && flow_type != INGEST_FLOW_F16) return fail(MFN_E_PARAM, "%s: flow type %d (0 = fp32, 1 = fp16)", what, flow_type);
  if (!aligned(src, 16) || !aligned(flow, 16) || !aligned(mask, 16)) return fail(MFN_E_ALIGN, "%s: the array and the outputs must be 16-byte aligned", what);
  IngestFlowParams p{};
  p.src = src + (long long)y0 * pitch + 3ll * x0;
  p.pitch = pitch;
  p.cols = (const IngestTap *)tables_dev; p.rows = p.cols + dst_w;
  p.flow = flow; p.mask = mask; p.Hd = dst_h; p.Wd = dst_w;
  p.premultiply = (unsigned)premultiply; p.flow_type = (unsigned)flow_type;
  p.sx = (float)(dst_w - 1) / (float)(w - 1);
  p.sy = (float)(dst_h - 1) / (float)(h - 1);
  return hipfail(ingest_flow_occ_launch(p, (hipStream_t)stream), what);
}

int MFN_API(png_unfilter)(unsigned char *raw, long long rows, long long row_bytes, int bytes_per_pixel) {
  if (rows < 0 || row_bytes < 0 || bytes_per_pixel < 1 || bytes_per_pixel > 8)
    return fail(MFN_E_SHAPE, "png_unfilter: rows=%lld row_bytes=%lld bytes_per_pixel=%d", rows, row_bytes, bytes_per_pixel);
  if (rows != 0 && !raw) return fail(MFN_E_NULL, "png_unfilter: NULL buffer");
  const long long bad = png_unfilter(raw, rows, row_bytes, bytes_per_pixel);
  if (bad) return fail(MFN_E_PARAM, "png_unfilter: row %lld has a filter type that is none of 0..4", bad - 1);
  return 0;
}

int MFN_API(leaky_relu_bwd)(const float *gout, const float *y, float *gin, size_t n, float slope, void *stream) {
  if (n != 0 && (!gout || !y || !gin)) return fail(MFN_E_NULL, "leaky_relu_bwd: NULL tensor pointer");
  return hipfail(leaky_bwd_launch(LeakyBwdParams{gout, y, gin, n, slope}, (hipStream_t)stream), "leaky_relu_bwd");
}

// ---- the matching module's gate, forward and backward (kernels/gate.h) ---------------------------------------------------------
static int gate_dims(const char *what, int N, int C, int H, int W, int activation) {
  if (N < 0 || C <= 0 || H <= 0 || W <= 0) return fail(MFN_E_SHAPE, "%s: N=%d C=%d H=%d W=%d", what, N, C, H, W);
  if (activation != MFN_ACT_NONE && activation != MFN_ACT_LEAKY_0_1) return fail(MFN_E_PARAM, "%s: activation=%d", what, activation);
  if (N > GATE_MAX_GRID_YZ || cdiv(C, GATE_FWD_CH) > GATE_MAX_GRID_YZ || (size_t)H * W > ((size_t)1 << 30))
    return fail(MFN_E_UNSUPPORTED, "%s: tensor too large", what);
  return 0;
}
// the 16-byte route: W % 4 == 0 and every pointer given 16-byte aligned (NULL counts as aligned)
static bool gate_vec4(int W, std::initializer_list<const void *> ptrs) {
  bool ok = W % 4 == 0;
  for (const void *q : ptrs) ok = ok && aligned(q, 16);
  return ok;
}

int MFN_API(matching_gate_fwd)(const float *raw, const float *mask, const float *tradeoff, int activation, float *out, int N, int C, int H,
                               int W, void *stream) {
  if (int rc = gate_dims("matching_gate_fwd", N, C, H, W, activation)) return rc;
  if (N == 0) return 0;
  if (!raw || !out) return fail(MFN_E_NULL, "matching_gate_fwd: NULL tensor pointer");
  const GateFwdParams p{raw, mask, tradeoff, out, N, C, H * W, activation == MFN_ACT_LEAKY_0_1 ? 1 : 0};
  return hipfail(matching_gate_fwd_launch(p, gate_vec4(W, {raw, mask, tradeoff, out}), (hipStream_t)stream), "matching_gate_fwd");
}

size_t MFN_API(matching_gate_bwd_workspace_bytes)(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return gate_bwd_ws_bytes(N, C, (size_t)H * W);
}

int MFN_API(matching_gate_bwd)(const float *gout, const float *gout2, const float *y, const float *raw, const float *mask, int activation,
                               float *graw, float *gmask, float *gtradeoff, int N, int C, int H, int W, int req_raw, int req_mask,
                               int req_tradeoff, void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = gate_dims("matching_gate_bwd", N, C, H, W, activation)) return rc;
  if (!req_ok(req_raw) || !req_ok(req_mask) || !req_ok(req_tradeoff))
    return fail(MFN_E_PARAM, "matching_gate_bwd: every req must be 0 (null), 1 (write) or 3 (add)");
  if (req_mask && !mask) return fail(MFN_E_PARAM, "matching_gate_bwd: a mask gradient is asked for and no mask is given");
  if (N == 0 || (!req_raw && !req_mask && !req_tradeoff)) return 0;
  if (!gout || (activation && !y) || (req_mask && !raw)) return fail(MFN_E_NULL, "matching_gate_bwd: NULL tensor pointer (gout, y, raw)");
  if ((req_raw && !graw) || (req_mask && !gmask) || (req_tradeoff && !gtradeoff))
    return fail(MFN_E_NULL, "matching_gate_bwd: NULL gradient pointer with a req that is not null");
  const GatePlan pl = gate_plan(N, C, (size_t)H * W);
  const size_t need = req_mask ? gate_bwd_ws_bytes(N, C, (size_t)H * W) : 0;
  if (need && (!workspace || workspace_bytes < need))
    return fail(MFN_E_WORKSPACE, "matching_gate_bwd: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (need && !aligned(workspace, 4)) return fail(MFN_E_ALIGN, "matching_gate_bwd: workspace must be 4-byte aligned");
  GateBwdParams p{};
  p.gout = gout; p.gout2 = gout2; p.y = activation ? y : nullptr; p.raw = req_mask ? raw : nullptr; p.mask = mask;
  p.graw = req_raw ? graw : nullptr; p.gmask = req_mask ? gmask : nullptr; p.gtradeoff = req_tradeoff ? gtradeoff : nullptr;
  p.partial = need ? (float *)workspace : nullptr;
  p.N = N; p.C = C; p.HW = H * W; p.leaky = activation == MFN_ACT_LEAKY_0_1 ? 1 : 0; p.cps = pl.cps; p.splits = pl.splits;
  p.add_raw = req_raw == MFN_REQ_ADD; p.add_mask = req_mask == MFN_REQ_ADD; p.add_tradeoff = req_tradeoff == MFN_REQ_ADD;
  const bool vec4 = gate_vec4(W, {gout, gout2, p.y, p.raw, mask, p.graw, p.gmask, p.gtradeoff, p.partial});
  return hipfail(matching_gate_bwd_launch(p, vec4, (hipStream_t)stream), "matching_gate_bwd");
}

// What conv_bwd_plan decides for mfn_conv2d_bwd and the call executes.  Workspace: [gpre: the gradient before the fused LeakyReLU]
// [zero offsets of the weight-gradient call] [flipped weights] [gx temporary] [s2d] [inner: the forward call's packed weights, the
// weight gradient's slabs]
enum class ConvBwdData { S2d, Conv, Flip, Deconv };
struct ConvBwdPlan {
  size_t gpre, zoff, wflip, gxtmp, s2d, inner, total;
  int Ho, Wo;
  // data gradient, a forward call (N, Cin', H', W') -> (N, Cin, H, W).  S2d: the network's transposed convolution (4x4 / stride 2 / pad 1,
  // no adj) as a 3x3 convolution of the pixel-unshuffled output gradient (kernels/backward.h conv_s2d_kernel) on the MFMA kernels |
  // Conv: a transposed layer's, Convolution(gpre, w) | Flip: stride 1, convolution of gpre with the flipped, transposed filters |
  // Deconv: strided, Deconvolution(gpre, w) with THIS call's adj (odd input sizes: adj != 0; the kernel family depends on it)
  ConvBwdData data;
  struct { int Cin, H, W, kh, kw, sh, sw, ph, pw, dh, dw, transposed, adj_h, adj_w; } d;
  bool wgrad_own;   // the convolution's own weight-gradient kernel (conv_wgrad.h); else the deformable weight gradient with zero offsets
};
// al16: gpre and x are 16-byte aligned, which conv_wgrad needs and the size query cannot know: the scratch serves either weight gradient
static int conv_bwd_plan(const Settings &st, ConvBwdPlan &q, const char *what, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw,
                         int ph, int pw, int dh, int dw, int groups, int transposed, int adj_h, int adj_w, int activation, int req_x,
                         bool al16 = true) {
  memset(&q, 0, sizeof(q));
  int rc = conv_dims(what, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, &q.Ho, &q.Wo);
  if (rc) return rc;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t out_elems = (size_t)N * Cout * q.Ho * q.Wo, in_elems = (size_t)N * Cin * H * W;
  q.gpre = activation == MFN_ACT_LEAKY_0_1 ? up(out_elems * 4) : 0;
  // the weight gradient is a deformable-conv weight gradient with zero offsets: "output" grid = the conv's output (transposed: input) grid
  const size_t wplane = transposed ? (size_t)H * W : (size_t)q.Ho * q.Wo;
  q.zoff = up((size_t)N * 2 * kh * kw * wplane * 4);
  q.wflip = up((size_t)Cout * Cin * kh * kw * 4);
  q.gxtmp = req_x == MFN_REQ_ADD ? up(in_elems * 4) : 0;
  q.d = {Cout, q.Ho, q.Wo, kh, kw, sh, sw, ph, pw, dh, dw, 0, 0, 0};
  size_t wg;
  if (transposed && kh == 4 && kw == 4 && sh == 2 && sw == 2 && ph == 1 && pw == 1 && dh == 1 && dw == 1 && !adj_h && !adj_w &&
      !(st.t.path_generic & 4)) {
    q.data = ConvBwdData::S2d;
    q.s2d = up(out_elems * 4);                                  // (N, 4 Cout, H, W)
    q.wflip = up((size_t)Cin * 4 * Cout * 9 * 4);               // (Cin, 4 Cout, 3, 3)
    q.d = {4 * Cout, H, W, 3, 3, 1, 1, 1, 1, 1, 1, 0, 0, 0};
  } else if (transposed) q.data = ConvBwdData::Conv;
  else if (sh == 1 && sw == 1) {
    q.data = ConvBwdData::Flip;
    q.d.ph = dh * (kh - 1) - ph; q.d.pw = dw * (kw - 1) - pw;
  } else {
    q.data = ConvBwdData::Deconv;
    q.d.transposed = 1;
    q.d.adj_h = H - ((q.Ho - 1) * sh - 2 * ph + dh * (kh - 1) + 1); q.d.adj_w = W - ((q.Wo - 1) * sw - 2 * pw + dw * (kw - 1) + 1);
  }
  size_t inner = conv_ws_bytes(st, N, q.d.Cin, q.d.H, q.d.W, Cin, q.d.kh, q.d.kw, q.d.sh, q.d.sw, q.d.ph, q.d.pw, q.d.dh, q.d.dw, 1, q.d.transposed,
                               q.d.adj_h, q.d.adj_w);
  if (transposed) wg = dc_bwd_ws_bytes(st, N, Cout, q.Ho, q.Wo, Cin, kh, kw, sh, sw, ph, pw, dh, dw, 1, 1);
  else {
    wg = dc_bwd_ws_bytes(st, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, 1, 1);
    if (conv_wgrad_shape_ok(Cin, Cout, H, W, kh, kw, sh, sw, ph, pw, dh, dw) && !(st.t.path_generic & 4)) {
      q.wgrad_own = al16;
      size_t slab = conv_wgrad_plan(N, Cin, Cout, H, W).slab_bytes;
      if (conv_wgrad_mma_ok(W, dh)) { const size_t s2 = conv_wgrad_plan(N, Cin, Cout, H, W, true).slab_bytes; slab = slab > s2 ? slab : s2; }
      wg = wg > slab ? wg : slab;
    }
  }
  q.inner = up(inner > wg ? inner : wg);
  q.total = q.gpre + q.zoff + q.wflip + q.gxtmp + q.s2d + q.inner;
  return 0;
}

size_t MFN_API(conv2d_bwd_workspace_bytes)(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                                           int dh, int dw, int groups, int transposed, int adj_h, int adj_w, int activation) {
  ConvBwdPlan q;
  if (N <= 0 || conv_bwd_plan(settings_now(), q, "conv2d_bwd_workspace_bytes", N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed,
                              adj_h, adj_w, activation, MFN_REQ_ADD))
    return 0;
  return q.total;
}

// Backward of mfn_conv2d_fwd (groups == 1), composed from the library's own kernels:
//   gpre = gout * LeakyReLU'(y)                                        (activation == MFN_ACT_LEAKY_0_1: y = the forward output)
//   gx   = a forward call of the plan's data-gradient route
//   gw   = conv_wgrad, or the deformable convolution's weight gradient with zero offsets (bilinear sampling at integer positions is the
//          pixel itself, out-of-range taps are zero in both operators); for the transposed operator the roles of x and gpre swap
//   gb   = sum of gpre over (n, pixel)
int MFN_API(conv2d_bwd)(const float *gout, const float *x, const float *w, const float *y_or_null, float *gx, float *gw,
                        float *gbias, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                        int dh, int dw, int groups, int transposed, int adj_h, int adj_w, int activation, int req_x, int req_w,
                        int req_bias, void *workspace, size_t ws_bytes, void *stream) {
  const Settings st = settings_now();
  const char *what = transposed ? "conv2d_transpose_bwd" : "conv2d_bwd";
  if (!req_ok(req_x) || !req_ok(req_w) || !req_ok(req_bias)) return fail(MFN_E_PARAM, "%s: req must be 0 (null), 1 (write) or 3 (add)", what);
  if (groups != 1) return fail(MFN_E_UNSUPPORTED, "%s: num_group=%d (the reference's blocks use 1)", what, groups);
  if (activation != MFN_ACT_NONE && activation != MFN_ACT_LEAKY_0_1) return fail(MFN_E_PARAM, "%s: unknown activation %d", what, activation);
  ConvBwdPlan q;   // gpre is gout or the head of the (16-byte aligned) workspace
  int rc = conv_bwd_plan(st, q, what, N, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, transposed, adj_h, adj_w, activation, req_x,
                         aligned(x, 16) && (activation == MFN_ACT_LEAKY_0_1 || aligned(gout, 16)));
  if (rc) return rc;
  if (!w || (N != 0 && (!gout || !x))) return fail(MFN_E_NULL, "%s: NULL tensor pointer", what);
  if (activation == MFN_ACT_LEAKY_0_1 && N != 0 && !y_or_null) return fail(MFN_E_NULL, "%s: the forward output is needed for the fused LeakyReLU", what);
  if ((N != 0 && req_x && !gx) || (req_w && !gw) || (req_bias && !gbias)) return fail(MFN_E_NULL, "%s: NULL gradient output", what);
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    if (req_w == MFN_REQ_WRITE && (rc = fill_zero_launch(gw, (size_t)Cout * Cin * kh * kw, s))) return hipfail(rc, what);
    if (req_bias == MFN_REQ_WRITE && (rc = fill_zero_launch(gbias, (size_t)Cout, s))) return hipfail(rc, what);
    return 0;
  }
  if (!workspace || ws_bytes < q.total) return fail(MFN_E_WORKSPACE, "%s: workspace of %zu bytes required (got %zu)", what, q.total, workspace ? ws_bytes : (size_t)0);
  if (!aligned(workspace, 16)) return fail(MFN_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  char *base = (char *)workspace;
  float *gpre_buf = (float *)base; base += q.gpre;
  float *zoff = (float *)base; base += q.zoff;
  float *wflip = (float *)base; base += q.wflip;
  float *gxtmp = (float *)base; base += q.gxtmp;
  float *s2d = (float *)base; base += q.s2d;
  void *inner = base;
  const int Ho = q.Ho, Wo = q.Wo;
  const size_t out_elems = (size_t)N * Cout * Ho * Wo, in_elems = (size_t)N * Cin * H * W;
  const float *gpre = gout;
  if (activation == MFN_ACT_LEAKY_0_1) {
    if ((rc = leaky_bwd_launch(LeakyBwdParams{gout, y_or_null, gpre_buf, out_elems, 0.1f}, s))) return hipfail(rc, what);
    gpre = gpre_buf;
  }
  if (req_x) {
    const float *src = gpre, *wsrc = w;
    if (q.data == ConvBwdData::S2d) {
      const size_t nt = (size_t)N * 4 * Cout * H * W, nw3 = (size_t)Cin * 4 * Cout * 9;
      if ((rc = launch("conv_s2d", conv_s2d_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, S2dParams{gpre, s2d, N, Cout, H, W})))
        return hipfail(rc, what);
      if ((rc = launch("conv_s2d_weights", conv_s2d_weights_kernel, dim3((unsigned)((nw3 + 255) / 256)), dim3(256), 0, s,
                       S2dWeightParams{w, wflip, Cin, Cout})))
        return hipfail(rc, what);
      src = s2d; wsrc = wflip;
    } else if (q.data == ConvBwdData::Flip) {
      if ((rc = conv_flip_weights_launch(FlipParams{w, wflip, Cout, Cin, kh, kw}, s))) return hipfail(rc, what);
      wsrc = wflip;
    }
    rc = conv_fwd_common(st, src, 0, wsrc, nullptr, 0, 0, nullptr, req_x == MFN_REQ_ADD ? gxtmp : gx, 0, N, q.d.Cin, q.d.H, q.d.W, Cin, q.d.kh, q.d.kw,
                         q.d.sh, q.d.sw, q.d.ph, q.d.pw, q.d.dh, q.d.dw, 1, q.d.transposed, q.d.adj_h, q.d.adj_w, MFN_ACT_NONE, inner, q.inner, stream);
    if (rc) return rc;
    if (req_x == MFN_REQ_ADD && (rc = accumulate_launch(gx, gxtmp, in_elems, s))) return hipfail(rc, what);
  }
  if (req_w && q.wgrad_own) {
    if ((rc = conv_wgrad_launch(gpre, x, gw, inner, N, Cin, Cout, H, W, dh, req_w == MFN_REQ_ADD ? 1 : 0, s, st.conv != 0))) return hipfail(rc, what);
  } else if (req_w) {
    const size_t wplane = transposed ? (size_t)H * W : (size_t)Ho * Wo;
    if ((rc = fill_zero_launch(zoff, (size_t)N * 2 * kh * kw * wplane, s))) return hipfail(rc, what);
    // (gout', x') of the deformable weight gradient: Convolution (gpre, x); Deconvolution (x, gpre) -- gw comes out as
    // (Cout, Cin, kh, kw) resp. (Cin, Cout, kh, kw), the operators' own layouts
    const DcBwdParams wp = transposed ? DcBwdParams{x, gpre, zoff, w, nullptr, nullptr, gw, nullptr, N, Cout, Ho, Wo, Cin, 0, 0, kh, kw, sh, sw, ph, pw,
                                                    dh, dw, 1, 1, MFN_REQ_NULL, MFN_REQ_NULL, req_w, MFN_REQ_NULL, 1}
                                      : DcBwdParams{gpre, x, zoff, w, nullptr, nullptr, gw, nullptr, N, Cin, H, W, Cout, 0, 0, kh, kw, sh, sw, ph, pw,
                                                    dh, dw, 1, 1, MFN_REQ_NULL, MFN_REQ_NULL, req_w, MFN_REQ_NULL, 1};
    if ((rc = dc_bwd_run(st, wp, inner, q.inner, s))) return rc;
  }
  if (req_bias) {
    // slices of the (n, pixel) range over blockIdx.y; their partial sums sit in the zero-offset buffer, which is free by now
    const size_t plane = (size_t)Ho * Wo, span = (size_t)N * plane;
    int S = (int)((span + 4095) / 4096);
    if (S > 64) S = 64;
    while (S > 1 && (size_t)Cout * S * sizeof(float) > q.zoff) --S;
    if (S > 1) {
      const int vec = plane % 4 == 0 && aligned(gpre, 16);
      size_t chunk = (span + S - 1) / S;
      chunk = (chunk + 3) / 4 * 4;
      ChanSumPartParams pp{gpre, zoff, N, Cout, S, plane, chunk, vec};
      if ((rc = launch("channel_sum_partial", channel_sum_partial_kernel, dim3(Cout, S), dim3(256), 256 * sizeof(float), s, pp))) return hipfail(rc, what);
      ChanSumFinalParams fp{zoff, gbias, Cout, S, req_bias == MFN_REQ_ADD ? 1 : 0};
      if ((rc = launch("channel_sum_final", channel_sum_final_kernel, dim3((unsigned)cdiv(Cout, 256)), dim3(256), 0, s, fp))) return hipfail(rc, what);
    } else {
      ChanSumParams cp{gpre, gbias, N, Cout, plane, req_bias == MFN_REQ_ADD ? 1 : 0};
      if ((rc = launch("channel_sum", channel_sum_kernel, dim3(Cout), dim3(256), 256 * sizeof(float), s, cp))) return hipfail(rc, what);
    }
  }
  return 0;
}

int MFN_API(debug_set_timeline)(void *device_buffer) {
  g_timeline = device_buffer;
  return 0;
}

static std::atomic<int> *arith_slot(const char *op) {
  if (!op) return nullptr;
  if (!strcmp(op, "correlation")) return &t_arith.corr;
  if (!strcmp(op, "deformable_convolution")) return &t_arith.deform;
  if (!strcmp(op, "convolution")) return &t_arith.conv;
  return nullptr;
}
int MFN_API(set_arithmetic)(const char *op, int mode) {
  if (mode < -1 || mode > 1) return fail(MFN_E_PARAM, "set_arithmetic: mode %d is none of MFN_ARITH_DEFAULT / _FP32 / _BF16X3", mode);
  if (op && !strcmp(op, "all")) { t_arith.corr = mode; t_arith.deform = mode; t_arith.conv = mode; return 0; }
  std::atomic<int> *slot = arith_slot(op);
  if (!slot) return fail(MFN_E_PARAM, "set_arithmetic: unknown operator '%s'", op ? op : "(null)");
  *slot = mode;
  return 0;
}
int MFN_API(get_arithmetic)(const char *op, int *mode) {
  std::atomic<int> *slot = arith_slot(op);
  if (!slot || !mode) return fail(MFN_E_PARAM, "get_arithmetic: unknown operator '%s'", op ? op : "(null)");
  *mode = *slot;
  return 0;
}

int MFN_API(debug_last_dc_plan)(int *mt, int *pt, int *kw, int *areg) {
  if (mt) *mt = t_last_dc_plan[0];
  if (pt) *pt = t_last_dc_plan[1];
  if (kw) *kw = t_last_dc_plan[2];
  if (areg) *areg = t_last_dc_plan[3];
  return 0;
}

int MFN_API(set_tuning)(const char *key, int value) {
  int *slot = key ? g_tuning.slot(key) : nullptr;
  if (!slot) return fail(MFN_E_PARAM, "set_tuning: unknown key '%s'", key ? key : "(null)");
  *slot = value;
  return 0;
}
int MFN_API(get_tuning)(const char *key, int *value) {
  int *slot = key ? g_tuning.slot(key) : nullptr;
  if (!slot || !value) return fail(MFN_E_PARAM, "get_tuning: unknown key '%s'", key ? key : "(null)");
  *value = *slot;
  return 0;
}

}  // extern "C"
