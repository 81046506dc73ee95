// upsample.h -- Upsample(factor) of the flow / mask between pyramid levels.
//
// Replaces the Gluon block at /root/reference/network/MaskFlownet.py:35-62 (call sites :228-229, :246-247, :264-265,
// :282-283, :308, :311): edge-pad one row/column at the bottom/right, Deconvolution with the separable triangle
// kernel k[a] = 1 - |f-1-a|/f (kernel 2f-1, stride f, pad f-1), drop the last row/column.  Semantics as
// oracle/mfn_ref_body.inc upsample.  Written as a gather: output (oy,ox) has at most 2x2 contributing inputs,
//   iy0 = oy / f with weight 1 - r/f  and  iy0 + 1 (clamped to H-1: the edge pad) with weight r/f,   r = oy % f,
// accumulated in the oracle's raster order with separately rounded multiplies and adds (fp contraction off), so
// results are bit-identical.
// HBM-bound: 4*N*C*H*W*(1 + f*f) bytes; one thread writes 4 adjacent outputs with one 16-byte store.
#pragma once
#include "../mfn_rt.h"

namespace mfn {

struct UpsampleParams {
  const float *x;
  float *out;
  int N, C, H, W, f;
  int st_policy;  // cache policy of the output stores (mfn_store4_stream)
};

// hipcc contracts a*b+c into FMAs by default (and HIP's __fmul_rn / __fadd_rn are plain operators, not barriers);
// the oracle (gcc -ffp-contract=off) rounds every product and sum separately, so contraction is switched off here.
__device__ __forceinline__ float upsample_tri(int cc, int a) {
#pragma clang fp contract(off)
  return 1.f - fabsf((float)(cc - a)) / (float)(cc + 1);  // the reference's _kernel2d entry, same rounding
}

// One output pixel, in three steps that upsample_kernel and the fused multiscale loss (loss.h) share: the loss recomputes
// Upsample(f)(p) per pixel and has to get upsample_kernel's bits (its gradient is discontinuous where the difference to the
// label changes sign), so the arithmetic lives here once.  `tri(a)` supplies upsample_tri(f - 1, a) -- computed on the spot
// here, read from a table of exactly those values in loss.h -- and `div(o)` is o / f (a plain or a multiply-shift division:
// integers, exact either way).  Row part: the two input rows and their weights.
struct UpsampleRow { size_t o0, o1; float ka0, ka1; int i0, i1, ry; };
template <class Tri, class Div>
__device__ __forceinline__ UpsampleRow upsample_row(int H, int W, int f, int oy, Tri tri, Div div) {
  UpsampleRow r;
  r.i0 = div(oy);
  r.ry = oy - r.i0 * f;
  r.i1 = min(r.i0 + 1, H - 1);
  r.ka0 = tri(r.ry + f - 1);                  // row iy0
  r.ka1 = r.ry ? tri(r.ry - 1) : 0.f;         // row iy0 + 1 (absent when r == 0)
  r.o0 = (size_t)r.i0 * W;
  r.o1 = (size_t)r.i1 * W;
  return r;
}
// Column part: the two input columns and their weights.
struct UpsampleCol { int ix0, ix1; float kb0, kb1; int rx; };
template <class Tri, class Div>
__device__ __forceinline__ UpsampleCol upsample_col(int W, int f, int ox, Tri tri, Div div) {
  UpsampleCol c;
  c.ix0 = div(ox);
  c.rx = ox - c.ix0 * f;
  c.ix1 = min(c.ix0 + 1, W - 1);
  c.kb0 = tri(c.rx + f - 1);
  c.kb1 = c.rx ? tri(c.rx - 1) : 0.f;
  return c;
}
// The blend: dst += v * (ka * kb) in raster order of the contributing inputs; no contraction into FMAs.  `ld(rs, cs)` supplies the
// input at (row rs ? i1 : i0, column cs ? ix1 : ix0) -- from the plane in global memory here, from a staged patch in loss.h.
template <class Ld>
__device__ __forceinline__ float upsample_blend(Ld ld, const UpsampleRow &r, const UpsampleCol &c) {
#pragma clang fp contract(off)
  float acc = ld(0, 0) * (r.ka0 * c.kb0);
  if (c.rx) acc = acc + ld(0, 1) * (r.ka0 * c.kb1);
  if (r.ry) {
    acc = acc + ld(1, 0) * (r.ka1 * c.kb0);
    if (c.rx) acc = acc + ld(1, 1) * (r.ka1 * c.kb1);
  }
  return acc;
}
// ld of a plane in global memory
struct UpsamplePlane {
  const float *src;
  const UpsampleRow &r;
  const UpsampleCol &c;
  __device__ __forceinline__ float operator()(int rs, int cs) const { return src[(rs ? r.o1 : r.o0) + (cs ? c.ix1 : c.ix0)]; }
};

template <int VEC>
__global__ __launch_bounds__(256) void upsample_kernel(UpsampleParams p) {
#pragma clang fp contract(off)
  const int f = p.f;
  const int Hout = p.H * f, Wout = p.W * f;
  const int wv = Wout / VEC;
  const size_t total = (size_t)p.N * p.C * Hout * wv;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int xv = (int)(idx % wv);
  const int oy = (int)((idx / wv) % Hout);
  const size_t nc = idx / ((size_t)wv * Hout);
  const float *src = p.x + nc * (size_t)p.H * p.W;
  auto tri = [f](int a) { return upsample_tri(f - 1, a); };
  auto div = [f](int o) { return o / f; };
  const UpsampleRow row = upsample_row(p.H, p.W, f, oy, tri, div);
  float o[VEC];
  MFN_UNROLL
  for (int k = 0; k < VEC; ++k) {
    const UpsampleCol col = upsample_col(p.W, f, xv * VEC + k, tri, div);
    o[k] = upsample_blend(UpsamplePlane{src, row, col}, row, col);
  }
  float *dst = p.out + nc * (size_t)Hout * Wout + (size_t)oy * Wout + (size_t)xv * VEC;
  if (VEC == 4) {
    mfn_store4_stream(dst, o[0], o[1 % VEC], o[2 % VEC], o[3 % VEC], p.st_policy);
  } else {
    MFN_UNROLL
    for (int k = 0; k < VEC; ++k) dst[k] = o[k];
  }
}

inline int upsample_launch(UpsampleParams p, hipStream_t stream) {
  const int Wout = p.W * p.f;
  const bool vec4 = (Wout % 4 == 0) && (((uintptr_t)p.out) % 16 == 0);
  const size_t total = (size_t)p.N * p.C * p.H * p.f * (vec4 ? Wout / 4 : Wout);
  if (total == 0) return 0;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (vec4) return launch("upsample_v4", upsample_kernel<4>, grid, dim3(256), 0, stream, p);
  return launch("upsample_v1", upsample_kernel<1>, grid, dim3(256), 0, stream, p);
}

}  // namespace mfn
