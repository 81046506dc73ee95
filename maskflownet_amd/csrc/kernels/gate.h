// gate.h -- the matching module's gate on its own, forward and backward: the training form of dc_epilogue (deform_conv.h).
//
// Replaces network/MaskFlownet.py:231-233 (and :249-251, :267-269, :285-287) where a level is trained through:
//   warp = raw * sigmoid(mask) + tradeoff;  warp = LeakyReLU(0.1)(warp)          raw: the deformable convolution's output
// with s = 1 / (1 + expf(-mask)), mask (N,1,H,W) and tradeoff (N,C,H,W) each optional, everything contiguous NCHW fp32.
// At inference the deformable convolution applies dc_epilogue itself (mfn_deform_conv_matching_fwd); training needs `raw`
// on the tape, so the gate is a pass of its own here.  The forward calls dc_epilogue per element: one statement of the
// arithmetic for both.
//
// Backward, from the upstream gradient(s) g = gout (+ gout2, added first), the saved OUTPUT y, raw and mask:
//   gp        = act ? g * (y > 0 ? 1 : 0.1) : g                    (the rule of leaky_bwd_kernel, from the output)
//   gtradeoff = gp
//   graw      = gp * s                                             (gp without a mask)
//   gmask     = s * s' * sum_c gp[n,c,h,w] * raw[n,c,h,w]          s' = 1 / (1 + expf(+mask)) = sigmoid(-mask)
// s' is evaluated on its own: 1 - s has no correct bit left on a saturated mask.  Every product and sum is rounded separately
// (fp contraction off), so the statement in tests/gate_ref.py is the same arithmetic.
//
// A thread owns VEC consecutive pixels of one image (VEC = 4 with 16-byte loads and stores where W % 4 == 0 and every pointer
// is 16-byte aligned, VEC = 1 otherwise) and walks a slice of the channels, so mask, s and s' are read and formed once per
// slice and the channel sum is a serial sum in a register: no atomics, a fixed order.
//   bytes: forward 2 (3 with a tradeoff) tensor passes; backward gout, y, raw in and graw, gtradeoff out: 5 passes (6 with gout2),
//   the (N,1,H,W) planes are 1 / C of one.  Level 2 (98 k pixels x 32 channels: 12.6 MB per tensor pass) is bandwidth.
// Plan (gate_plan, from N, C, H, W alone, so that the workspace query and the call agree): the pixels alone give
// N * ceil(H W / 1024) blocks; a level with fewer than GATE_TARGET_BLOCKS of them (level 6 of the full model: 384 pixels x 196
// channels, one block per image) splits the channels over grid.y into slices of at least GATE_MIN_CH channels.  The slices'
// partial sums go to the workspace [slice][N][H W], every element written, and matching_gate_bwd_join_kernel adds them in
// slice order and applies s * s'.  GATE_TARGET_BLOCKS = 512 is two blocks for each of the 256 CUs: a reasoned figure, not a
// measured one (profiles/matching_gate.md records what was measured).
#pragma once
#include "../mfn_rt.h"
#include "deform_conv.h"

namespace mfn {

enum { GATE_FWD_CH = 8, GATE_MIN_CH = 4, GATE_TARGET_BLOCKS = 512, GATE_MAX_GRID_YZ = 65535 };

template <int VEC>
__device__ __forceinline__ void gate_load(float (&d)[VEC], const float *src) {
  if constexpr (VEC == 4) {
    const float4 a = *reinterpret_cast<const float4 *>(src);
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  } else {
    d[0] = src[0];
  }
}
template <int VEC>
__device__ __forceinline__ void gate_store(float *dst, const float (&v)[VEC], int add) {
  if constexpr (VEC == 4) {
    float4 o = make_float4(v[0], v[1], v[2], v[3]);
    if (add) {
      const float4 a = *reinterpret_cast<const float4 *>(dst);
      o = make_float4(a.x + v[0], a.y + v[1], a.z + v[2], a.w + v[3]);
    }
    *reinterpret_cast<float4 *>(dst) = o;
  } else {
    dst[0] = add ? dst[0] + v[0] : v[0];
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
// dc_epilogue on values held in registers: it takes its mask and its addend through pointers, and only the address of a local
// that is named outright (not selected against nullptr) lets the compiler keep that local in a register
__device__ __forceinline__ float gate_value(float v, float m, float t, bool has_m, bool has_t, int leaky) {
  if (has_m) return has_t ? dc_epilogue(v, &m, &t, leaky, 0, 0) : dc_epilogue(v, &m, nullptr, leaky, 0, 0);
  return has_t ? dc_epilogue(v, nullptr, &t, leaky, 0, 0) : dc_epilogue(v, nullptr, nullptr, leaky, 0, 0);
}

struct GateFwdParams { const float *raw, *mask, *tradeoff; float *out; int N, C, HW, leaky; };

// grid (ceil(HW / VEC / 256), ceil(C / GATE_FWD_CH), N)
template <int VEC>
__global__ __launch_bounds__(256) void matching_gate_fwd_kernel(GateFwdParams p) {
  const size_t q0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * VEC;   // VEC == 4 only with W % 4 == 0: HW % 4 == 0
  if (q0 >= (size_t)p.HW) return;
  const int n = blockIdx.z, c0 = blockIdx.y * GATE_FWD_CH, c1 = min(c0 + GATE_FWD_CH, p.C);
  float m[VEC] = {}, t[VEC] = {}, v[VEC];
  if (p.mask) gate_load<VEC>(m, p.mask + (size_t)n * p.HW + q0);
  for (int c = c0; c < c1; ++c) {
    const size_t e = ((size_t)n * p.C + c) * p.HW + q0;
    gate_load<VEC>(v, p.raw + e);
    if (p.tradeoff) gate_load<VEC>(t, p.tradeoff + e);
    MFN_UNROLL
    for (int j = 0; j < VEC; ++j) v[j] = gate_value(v[j], m[j], t[j], p.mask != nullptr, p.tradeoff != nullptr, p.leaky);
    gate_store<VEC>(p.out + e, v, 0);
  }
}

inline int matching_gate_fwd_launch(GateFwdParams p, bool vec4, hipStream_t stream) {
  const int vec = vec4 ? 4 : 1;
  const dim3 grid((unsigned)(((size_t)p.HW / vec + 255) / 256), (unsigned)cdiv(p.C, GATE_FWD_CH), (unsigned)p.N);
  return vec4 ? launch("matching_gate_fwd_v4", matching_gate_fwd_kernel<4>, grid, dim3(256), 0, stream, p)
              : launch("matching_gate_fwd_v1", matching_gate_fwd_kernel<1>, grid, dim3(256), 0, stream, p);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
struct GatePlan { int cps, splits; };   // channels per slice, slices (grid.y)
inline GatePlan gate_plan(int N, int C, size_t HW) {
  const size_t blocks = (size_t)N * ((HW + 1023) / 1024);
  int want = 1;
  if (blocks < GATE_TARGET_BLOCKS) want = (int)((GATE_TARGET_BLOCKS + blocks - 1) / blocks);
  const int most = cdiv(C, GATE_MIN_CH);
  const int cps = cdiv(C, want < most ? want : most);
  return GatePlan{cps, cdiv(C, cps)};   // no empty slice
}
inline size_t gate_bwd_ws_bytes(int N, int C, size_t HW) {
  const GatePlan pl = gate_plan(N, C, HW);
  return pl.splits > 1 ? (size_t)pl.splits * N * HW * sizeof(float) : 0;
}

struct GateBwdParams {
  const float *gout, *gout2, *y, *raw, *mask;   // gout2, mask: or nullptr; y: read with leaky only; raw: read for gmask only
  float *graw, *gmask, *gtradeoff;              // nullptr: req null
  float *partial;                               // splits > 1 and gmask: [splits][N][HW]
  int N, C, HW, leaky, cps, splits, add_raw, add_mask, add_tradeoff;
};

// grid (ceil(HW / VEC / 256), splits, N)
template <int VEC>
__global__ __launch_bounds__(256) void matching_gate_bwd_kernel(GateBwdParams p) {
#pragma clang fp contract(off)
  const size_t q0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (q0 >= (size_t)p.HW) return;
  const int n = blockIdx.z, sp = blockIdx.y, c0 = sp * p.cps, c1 = min(c0 + p.cps, p.C);
  const size_t pix = (size_t)n * p.HW + q0;
  float s[VEC], sn[VEC], acc[VEC], g[VEC], u[VEC];
  MFN_UNROLL
  for (int j = 0; j < VEC; ++j) { s[j] = 1.f; sn[j] = 0.f; acc[j] = 0.f; }
  if (p.mask) {
    gate_load<VEC>(u, p.mask + pix);
    MFN_UNROLL
    for (int j = 0; j < VEC; ++j) { s[j] = 1.f / (1.f + expf(-u[j])); sn[j] = 1.f / (1.f + expf(u[j])); }
  }
  for (int c = c0; c < c1; ++c) {
    const size_t e = ((size_t)n * p.C + c) * p.HW + q0;
    gate_load<VEC>(g, p.gout + e);
    if (p.gout2) {
      gate_load<VEC>(u, p.gout2 + e);
      MFN_UNROLL
      for (int j = 0; j < VEC; ++j) g[j] = g[j] + u[j];
    }
    if (p.leaky) {
      gate_load<VEC>(u, p.y + e);
      MFN_UNROLL
      for (int j = 0; j < VEC; ++j) g[j] = u[j] > 0.f ? g[j] : g[j] * 0.1f;
    }
    if (p.gtradeoff) gate_store<VEC>(p.gtradeoff + e, g, p.add_tradeoff);
    if (p.gmask) {
      gate_load<VEC>(u, p.raw + e);
      MFN_UNROLL
      for (int j = 0; j < VEC; ++j) acc[j] = acc[j] + g[j] * u[j];
    }
    if (p.graw) {
      if (p.mask) {
        MFN_UNROLL
        for (int j = 0; j < VEC; ++j) g[j] = g[j] * s[j];
      }
      gate_store<VEC>(p.graw + e, g, p.add_raw);
    }
  }
  if (!p.gmask) return;
  if (p.splits > 1) {
    gate_store<VEC>(p.partial + ((size_t)sp * p.N + n) * p.HW + q0, acc, 0);
  } else {
    MFN_UNROLL
    for (int j = 0; j < VEC; ++j) acc[j] = (s[j] * sn[j]) * acc[j];
    gate_store<VEC>(p.gmask + pix, acc, p.add_mask);
  }
}

// the slices' partial sums in slice order, then s * s': one thread per pixel of the (N,1,H,W) plane
__global__ __launch_bounds__(256) void matching_gate_bwd_join_kernel(GateBwdParams p) {
#pragma clang fp contract(off)
  const size_t plane = (size_t)p.N * p.HW, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  float acc = p.partial[i];
  for (int sp = 1; sp < p.splits; ++sp) acc = acc + p.partial[(size_t)sp * plane + i];
  const float m = p.mask[i];
  const float v = ((1.f / (1.f + expf(-m))) * (1.f / (1.f + expf(m)))) * acc;
  p.gmask[i] = p.add_mask ? p.gmask[i] + v : v;
}

inline int matching_gate_bwd_launch(GateBwdParams p, bool vec4, hipStream_t stream) {
  const int vec = vec4 ? 4 : 1;
  const dim3 grid((unsigned)(((size_t)p.HW / vec + 255) / 256), (unsigned)p.splits, (unsigned)p.N);
  const int rc = vec4 ? launch("matching_gate_bwd_v4", matching_gate_bwd_kernel<4>, grid, dim3(256), 0, stream, p)
                      : launch("matching_gate_bwd_v1", matching_gate_bwd_kernel<1>, grid, dim3(256), 0, stream, p);
  if (rc || !p.gmask || p.splits == 1) return rc;
  const size_t plane = (size_t)p.N * p.HW;
  return launch("matching_gate_bwd_join", matching_gate_bwd_join_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, stream, p);
}

}  // namespace mfn
