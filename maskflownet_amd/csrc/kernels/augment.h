// augment.h -- the two augmenters of the training batch on the device.
//
// Replaces the device side of /root/reference/augmentation.py:229-339 (GeometryAugmentation: :295-338 in one launch) and :168-227
// (ColorAugmentation: :213-225 in a reduction and one element-wise launch), as /root/reference/network/pipeline.py:100-101 calls
// them.  The per-sample scalars are drawn and turned into two small tables on the host (maskflownet_amd/augment.py); the kernels
// read the tables.  Every fp32 expression below is evaluated as written, left to right, every product and sum rounded separately
// (fp contraction off); tests/augment_ref.py restates this text in numpy.
//
// ---- geometry: per target pixel (n, y, x) of Ht x Wt (both >= 2), sources of Ho x Wo --------------------------------------------
// table row of sample n (AG_K floats): theta1[6] theta2[6] ft[2] rt[2] fshift[2] inv2[4] factor[4]  (offsets AG_*)
//   xn  = -1.f + (float)x * sx          sx = (float)(2.0 / (Wt-1))                     (grid_affine_kernel's positions)
//   yn  = -1.f + (float)y * sy          sy = (float)(2.0 / (Ht-1))
//   g1x = clip(((theta1[0]*xn + theta1[1]*yn) + theta1[2]) - ft[0], -1, 1)             clip(v) = fminf(fmaxf(v, -1.f), 1.f)
//   g1y = clip(((theta1[3]*xn + theta1[4]*yn) + theta1[5]) - ft[1], -1, 1)
//   g2x = (((theta2[0]*xn + theta2[1]*yn) + theta2[2]) - ft[0]) + rt[0]                not clipped: the sampler pads with zeros
//   g2y = (((theta2[3]*xn + theta2[4]*yn) + theta2[5]) - ft[1]) + rt[1]
//   t1 = sampler_taps(g1x, g1y, Ho, Wo), t2 = sampler_taps(g2x, g2y, Ho, Wo)           (warp.h: BilinearSampler's taps, once per grid)
//   S(v; t) = ((v00*w00 + v01*w01) + v10*w10) + v11*w11      a tap whose weight is 0 contributes the value 0.f (never loaded into the sum)
//   img1'[c] = S(img1[n,c]; t1)         img2'[c] = S(img2[n,c]; t2)         m' = S(mask[n]; t1)
//   f'[c]    = S(v; t1) with v_tap = (flow[n,c]_tap - fshift[c]) * mask_tap            (c = 0: u, c = 1: v, the reader's order)
//   f[c]     = f'[c] / fmaxf(m', 1e-8f)
//   out_u    = (inv2[0]*f[0] + inv2[1]*f[1]) + (factor[0]*xn + factor[1]*yn)
//   out_v    = (inv2[2]*f[0] + inv2[3]*f[1]) + (factor[2]*xn + factor[3]*yn)
//   flow_out = (out_u, out_v), or (out_v, out_u) with label_order = 1 (labels.flip(axis=1) of pipeline.py:105)
// A mask of shape (N,1,1,1) is read as a constant plane (every tap is mask[n]); it is never materialised, neither are the two
// grids nor the concatenated (img1 | mask | flow * mask) tensor of :305.  A thread reuses its two tap sets for all channels.
// Where Wt % 16 == 0 and Ht % 4 == 0 a thread owns one pixel and a wave is a 2-D tile of 16 x 4 pixels, the tile form of
// warp_fwd_fast_kernel: under a rotation the wave's taps stay within a few source rows, and the 64 lanes of a gather are on adjacent
// addresses.  Elsewhere a wave is a strip of one row, and a thread owns four adjacent pixels where Wt % 4 == 0 and every destination
// is 16-byte aligned (16-byte stores), one pixel otherwise.  Measured at 8 x 384x512 -> 320x448 (profiles/augment_kernels.md):
// 16 x 4 tile of single pixels 23 us, 64 x 4 tile of four-pixel threads 31 us (removed), strip of four-pixel threads 47 us.
// Traffic: 4 * N * (9 * Ho*Wo gathered at most + 9 * Ht*Wt written) bytes.
//
// ---- noise: Philox4x32-10, key (seed_lo, seed_hi), counter (q, plane, offset_lo, offset_hi) --------------------------------------
//   plane = (k*N + n)*3 + c  (k = 0: image 1, 1: image 2),  q = pixel index / 4: one block x[0..3] gives the normals of pixels 4q..4q+3
//   u1 = ((float)(x[0]>>8) + 1.f) * 2^-24  in (0,1]     u2 = (float)(x[1]>>8) * 2^-24     r = sqrtf(-2.f * logf(u1))
//   z0 = r * cosf(6.2831855f * u2)      z1 = r * sinf(6.2831855f * u2)      z2, z3 the same from x[2], x[3]
// logf / sinf / cosf are the accurate ones.  The noise never exists in memory: both colour kernels regenerate it.  sigma == 0 runs no
// generator code: the result does not depend on seed or offset.
//
// ---- colour: table row of sample n (AC_K floats): M[9] cc[3] channel[3] brightness e spin[9]  (offsets AC_*) ----------------------
//   a[i] = (M[3i]*r + M[3i+1]*g) + M[3i+2]*b          (r, g, b) the pixel of image k;  sigma != 0:  a[i] = a[i] + z[i]*sigma
//   mean[k,n,i] = (sum over the plane of a[i]) / (float)(H*W)
//       fixed order, no atomics: a block of 256 threads takes a slice of 4096 pixels, thread t the quads 4*(j*256 + t) .. +3 of it for
//       j = 0..3 (16 pixels in ascending order, added one by one to a sum that starts at 0.f: 16 additions, the first one exact),
//       an 8-level tree in LDS joins the threads (8 additions), one partial sum per slice and channel goes to the workspace; a
//       second kernel sums up to 4096 partials the same way (at most 16 + 8): no term passes through more than 48 additions, of
//       which the two onto 0.f round nothing -- the 46 of pair_mean's bound; bit-identical from run to run.
//   v[i] = (a[i] - mean[i]) * cc[i]                                                      cc = contrast * channel
//   spin:  v[i] = (spin[3i]*v[0] + spin[3i+1]*v[1]) + spin[3i+2]*v[2]                    (eigen_aug; from the three v of the line above)
//   v[i] = v[i] + (mean[i]*channel[i] + brightness)
//   v[i] = fminf(fmaxf(v[i], 0.f), 1.f)
//   gamma: v[i] = powf(v[i], e)                                                          e = exp(gamma), formed on the host
// out: (2N,3,H,W), images 1 in [0,N), images 2 in [N,2N).  Traffic: 4 * 2N*3*H*W bytes read by each kernel, the same written once.
#pragma once
#include "../mfn_rt.h"
#include "predict.h"
#include "warp.h"

namespace mfn {

enum { AG_THETA1 = 0, AG_THETA2 = 6, AG_FT = 12, AG_RT = 14, AG_FSHIFT = 16, AG_INV2 = 18, AG_FACTOR = 22, AG_K = 26 };
enum { AC_M = 0, AC_CC = 9, AC_CHANNEL = 12, AC_BRIGHTNESS = 15, AC_E = 16, AC_SPIN = 17, AC_K = 26 };

// ---- geometry ---------------------------------------------------------------------------------------------------------------------
struct AugGeoParams {
  const float *img1, *img2;   // (N,3,Ho,Wo)
  const float *flow;          // (N,2,Ho,Wo): (u, v)
  const float *mask;          // (N,1,Ho,Wo), or (N,1,1,1) with mask_plane == 0
  const float *tab;           // (N, AG_K)
  float *o1, *o2, *oflow, *omask;
  int N, Ho, Wo, Ht, Wt;
  int mask_plane;
  int label_order;
  float sx, sy;               // (float)(2.0 / (Wt-1)), (float)(2.0 / (Ht-1))
  int st_policy;              // cache policy of the output stores
};
#ifndef MFN_AUG_1D
#define MFN_AUG_1D 0   // measurement hook (profiles/augment_kernels.md): 1 = a wave is a strip of one row everywhere
#endif
#ifndef MFN_AUG_VEC1
#define MFN_AUG_VEC1 0   // measurement hook (the same): 1 = one pixel per thread and 4-byte stores everywhere
#endif

// the four tap values of a plane; a tap of weight 0 is 0.f.  PAIRS (Wo >= 2): two 8-byte loads instead of four gathers (warp.h)
template <bool PAIRS>
__device__ __forceinline__ void ag_gather(const float *pl, const Taps &t, float (&v)[4]) {
  if (PAIRS) {
    const f2u a = mfn_load2u(pl + t.p0), b = mfn_load2u(pl + t.p1);
    v[0] = t.w00 != 0.f ? (t.sel0 ? a.y : a.x) : 0.f;
    v[1] = t.w01 != 0.f ? (t.sel1 ? a.x : a.y) : 0.f;
    v[2] = t.w10 != 0.f ? (t.sel0 ? b.y : b.x) : 0.f;
    v[3] = t.w11 != 0.f ? (t.sel1 ? b.x : b.y) : 0.f;
  } else {
    v[0] = t.w00 != 0.f ? pl[t.i00] : 0.f;
    v[1] = t.w01 != 0.f ? pl[t.i01] : 0.f;
    v[2] = t.w10 != 0.f ? pl[t.i10] : 0.f;
    v[3] = t.w11 != 0.f ? pl[t.i11] : 0.f;
  }
}
__device__ __forceinline__ float ag_blend(const float (&v)[4], const Taps &t) {
#pragma clang fp contract(off)
  return ((v[0] * t.w00 + v[1] * t.w01) + v[2] * t.w10) + v[3] * t.w11;
}
__device__ __forceinline__ float ag_clip1(float v) { return fminf(fmaxf(v, -1.f), 1.f); }

template <int VEC, bool PAIRS, bool T2D>
__global__ __launch_bounds__(256) void augment_geometry_kernel(AugGeoParams p) {
#pragma clang fp contract(off)
  const int wv = p.Wt / VEC;   // VEC == 4 only with Wt % 4 == 0
  int xv, y, n;
  static_assert(!T2D || VEC == 1, "the 2-D tile is the one-pixel form's");
  if (T2D) {   // a wave is a tile of 16 x 4 pixels (Wt % 16 == 0, Ht % 4 == 0); the waves are numbered tile row by tile row
    const size_t bw = (size_t)(wv >> 4), bh = (size_t)(p.Ht >> 2);
    const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (size_t)p.N * bh * bw) return;
    const size_t rest = w / bw;
    xv = (int)(w - rest * bw) * 16 + (int)(threadIdx.x & 15u);
    y = (int)(rest % bh) * 4 + (int)((threadIdx.x >> 4) & 3u);
    n = (int)(rest / bh);
  } else {
    const size_t total = (size_t)p.N * p.Ht * wv;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    xv = (int)(idx % wv);
    y = (int)((idx / wv) % p.Ht);
    n = (int)(idx / ((size_t)wv * p.Ht));
  }
  const float *tb = p.tab + (size_t)n * AG_K;
  const size_t iplane = (size_t)p.Ho * p.Wo, oplane = (size_t)p.Ht * p.Wt;
  const float *s1 = p.img1 + (size_t)n * 3 * iplane, *s2 = p.img2 + (size_t)n * 3 * iplane;
  const float *fl = p.flow + (size_t)n * 2 * iplane;
  const float *mk = p.mask + (p.mask_plane ? (size_t)n * iplane : (size_t)n);
  const float yn = -1.f + (float)y * p.sy;
  float r[9][VEC];   // img1'[3], img2'[3], flow_out[2], m'
  MFN_UNROLL
  for (int k = 0; k < VEC; ++k) {
    const int x = xv * VEC + k;
    const float xn = -1.f + (float)x * p.sx;
    const float g1x = ag_clip1(((tb[AG_THETA1 + 0] * xn + tb[AG_THETA1 + 1] * yn) + tb[AG_THETA1 + 2]) - tb[AG_FT + 0]);
    const float g1y = ag_clip1(((tb[AG_THETA1 + 3] * xn + tb[AG_THETA1 + 4] * yn) + tb[AG_THETA1 + 5]) - tb[AG_FT + 1]);
    const float g2x = (((tb[AG_THETA2 + 0] * xn + tb[AG_THETA2 + 1] * yn) + tb[AG_THETA2 + 2]) - tb[AG_FT + 0]) + tb[AG_RT + 0];
    const float g2y = (((tb[AG_THETA2 + 3] * xn + tb[AG_THETA2 + 4] * yn) + tb[AG_THETA2 + 5]) - tb[AG_FT + 1]) + tb[AG_RT + 1];
    const Taps t1 = sampler_taps(g1x, g1y, p.Ho, p.Wo), t2 = sampler_taps(g2x, g2y, p.Ho, p.Wo);
    float v[4], m[4];
    MFN_UNROLL
    for (int c = 0; c < 3; ++c) {
      ag_gather<PAIRS>(s1 + (size_t)c * iplane, t1, v);
      r[c][k] = ag_blend(v, t1);
      ag_gather<PAIRS>(s2 + (size_t)c * iplane, t2, v);
      r[3 + c][k] = ag_blend(v, t2);
    }
    if (p.mask_plane) {
      ag_gather<PAIRS>(mk, t1, m);
    } else {
      const float mv = mk[0];
      m[0] = t1.w00 != 0.f ? mv : 0.f;
      m[1] = t1.w01 != 0.f ? mv : 0.f;
      m[2] = t1.w10 != 0.f ? mv : 0.f;
      m[3] = t1.w11 != 0.f ? mv : 0.f;
    }
    const float ms = ag_blend(m, t1);
    const float den = fmaxf(ms, 1e-8f);
    float f[2];
    MFN_UNROLL
    for (int c = 0; c < 2; ++c) {
      ag_gather<PAIRS>(fl + (size_t)c * iplane, t1, v);
      const float sh = tb[AG_FSHIFT + c];
      MFN_UNROLL
      for (int j = 0; j < 4; ++j) v[j] = (v[j] - sh) * m[j];
      f[c] = ag_blend(v, t1) / den;
    }
    const float ou = (tb[AG_INV2 + 0] * f[0] + tb[AG_INV2 + 1] * f[1]) + (tb[AG_FACTOR + 0] * xn + tb[AG_FACTOR + 1] * yn);
    const float ov = (tb[AG_INV2 + 2] * f[0] + tb[AG_INV2 + 3] * f[1]) + (tb[AG_FACTOR + 2] * xn + tb[AG_FACTOR + 3] * yn);
    r[6][k] = p.label_order ? ov : ou;
    r[7][k] = p.label_order ? ou : ov;
    r[8][k] = ms;
  }
  const size_t pix = (size_t)y * p.Wt + (size_t)xv * VEC;
  MFN_UNROLL
  for (int c = 0; c < 9; ++c) {
    float *dst = c < 3   ? p.o1 + ((size_t)n * 3 + c) * oplane
                 : c < 6 ? p.o2 + ((size_t)n * 3 + (c - 3)) * oplane
                 : c < 8 ? p.oflow + ((size_t)n * 2 + (c - 6)) * oplane
                         : p.omask + (size_t)n * oplane;
    if (VEC == 4) mfn_store4_stream(dst + pix, r[c][0], r[c][1 % VEC], r[c][2 % VEC], r[c][3 % VEC], p.st_policy);
    else mfn_store1_stream(dst + pix, r[c][0], p.st_policy);
  }
}

inline int augment_geometry_launch(AugGeoParams p, hipStream_t stream) {
  if ((size_t)p.N * p.Ht * p.Wt == 0) return 0;
  const bool pairs = p.Wo >= 2;
  const bool t2d = !MFN_AUG_1D && p.Wt % 16 == 0 && p.Ht % 4 == 0;   // one pixel per thread: a whole number of 16 x 4 waves
  const bool vec4 = !t2d && !MFN_AUG_VEC1 && p.Wt % 4 == 0 && ((uintptr_t)p.o1 | (uintptr_t)p.o2 | (uintptr_t)p.oflow | (uintptr_t)p.omask) % 16 == 0;
  const size_t total = (size_t)p.N * p.Ht * (vec4 ? p.Wt / 4 : p.Wt);   // threads
  const dim3 grid((unsigned)((total + 255) / 256));
  if (t2d) return pairs ? launch("augment_geometry_t2d", augment_geometry_kernel<1, true, true>, grid, dim3(256), 0, stream, p)
                        : launch("augment_geometry_t2d", augment_geometry_kernel<1, false, true>, grid, dim3(256), 0, stream, p);
  if (vec4) return pairs ? launch("augment_geometry_v4", augment_geometry_kernel<4, true, false>, grid, dim3(256), 0, stream, p)
                         : launch("augment_geometry_v4", augment_geometry_kernel<4, false, false>, grid, dim3(256), 0, stream, p);
  return pairs ? launch("augment_geometry_v1", augment_geometry_kernel<1, true, false>, grid, dim3(256), 0, stream, p)
               : launch("augment_geometry_v1", augment_geometry_kernel<1, false, false>, grid, dim3(256), 0, stream, p);
}

// ---- noise ------------------------------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11); the high words from 64-bit products
__host__ __device__ __forceinline__ void ag_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                                   unsigned (&x)[4]) {
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}
struct AugNoise { unsigned seed_lo, seed_hi, off_lo, off_hi; };
// the normals of pixels 4q .. 4q+3 of a plane
__device__ __forceinline__ void ag_normals(unsigned q, unsigned plane, const AugNoise &s, float (&z)[4]) {
#pragma clang fp contract(off)
  unsigned x[4];
  ag_philox(q, plane, s.off_lo, s.off_hi, s.seed_lo, s.seed_hi, x);
  MFN_UNROLL
  for (int h = 0; h < 2; ++h) {
    const float u1 = ((float)(x[2 * h] >> 8) + 1.f) * 5.9604644775390625e-8f;
    const float u2 = (float)(x[2 * h + 1] >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.f * logf(u1));
    const float a = 6.2831855f * u2;
    z[2 * h] = r * cosf(a);
    z[2 * h + 1] = r * sinf(a);
  }
}

// ---- colour -----------------------------------------------------------------------------------------------------------------------
struct AugColorParams {
  const float *img1, *img2;   // (N,3,H,W)
  const float *tab;           // (N, AC_K)
  float *partial;             // (2N, slices, 3)       mean kernels
  float *mean;                // (2N, 3): written by the mean kernels
  const float *mean_in;       // (2N, 3): read by the colour kernel
  float *out;                 // (2N,3,H,W)            colour kernel
  size_t plane;               // H * W
  int N, slices;
  float sigma;
  AugNoise noise;
  int spin, gamma;
  int st_policy;
};

// a[0..2] of the four pixels 4q .. 4q+3 of image kn (= k*N + n); px[c][j]: channel c of pixel 4q+j
__device__ __forceinline__ void ag_color_a(const AugColorParams &p, const float *tb, int kn, unsigned q, const float (&px)[3][4],
                                           float (&a)[3][4]) {
#pragma clang fp contract(off)
  MFN_UNROLL
  for (int i = 0; i < 3; ++i) {
    MFN_UNROLL
    for (int j = 0; j < 4; ++j)
      a[i][j] = (tb[AC_M + 3 * i] * px[0][j] + tb[AC_M + 3 * i + 1] * px[1][j]) + tb[AC_M + 3 * i + 2] * px[2][j];
  }
  if (p.sigma != 0.f) {
    MFN_UNROLL
    for (int i = 0; i < 3; ++i) {
      float z[4];
      ag_normals(q, (unsigned)kn * 3u + (unsigned)i, p.noise, z);
      MFN_UNROLL
      for (int j = 0; j < 4; ++j) a[i][j] = a[i][j] + z[j] * p.sigma;
    }
  }
}
// the quad's pixels of the three channel planes; VEC: plane % 4 == 0 and 16-byte aligned images.  Pixels past the plane read 0.f
template <bool VEC>
__device__ __forceinline__ void ag_load_quad(const float *src, size_t plane, size_t pix, float (&px)[3][4]) {
  MFN_UNROLL
  for (int c = 0; c < 3; ++c) {
    if (VEC) {
      const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)c * plane + pix);
      px[c][0] = v.x; px[c][1] = v.y; px[c][2] = v.z; px[c][3] = v.w;
    } else {
      MFN_UNROLL
      for (int j = 0; j < 4; ++j) px[c][j] = pix + j < plane ? src[(size_t)c * plane + pix + j] : 0.f;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void augment_color_mean_partial_kernel(AugColorParams p) {
  MFN_DYN_SHARED(float, red);   // [3][256]
  const int sl = blockIdx.x, kn = blockIdx.y;
  const int n = kn < p.N ? kn : kn - p.N;
  const float *src = (kn < p.N ? p.img1 : p.img2) + (size_t)n * 3 * p.plane;
  const float *tb = p.tab + (size_t)n * AC_K;
  const size_t base = (size_t)sl * PRED_SLICE;
  float s[3] = {0.f, 0.f, 0.f};
  MFN_UNROLL
  for (int k = 0; k < PRED_RUN / 4; ++k) {
    const size_t pix = base + 4 * ((size_t)k * 256 + threadIdx.x);
    if (pix < p.plane) {
      float px[3][4], a[3][4];
      ag_load_quad<VEC>(src, p.plane, pix, px);
      ag_color_a(p, tb, kn, (unsigned)(pix / 4), px, a);
      MFN_UNROLL
      for (int j = 0; j < 4; ++j) {
        if (VEC || pix + j < p.plane) { s[0] += a[0][j]; s[1] += a[1][j]; s[2] += a[2][j]; }
      }
    }
  }
  for (int i = 0; i < 3; ++i) {   // one tree per channel, each on its own 256 floats
    red[i * 256 + threadIdx.x] = s[i];
    pred_block_tree(red + i * 256);
  }
  if (threadIdx.x < 3) p.partial[((size_t)kn * p.slices + sl) * 3 + threadIdx.x] = red[threadIdx.x * 256];
}
__global__ __launch_bounds__(256) void augment_color_mean_final_kernel(AugColorParams p) {
  MFN_DYN_SHARED(float, red);
  const int kn = blockIdx.x, run = pred_run2(p.slices);
  const float *part = p.partial + (size_t)kn * p.slices * 3;
  float s[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < run; ++k) {
    const int q = (int)threadIdx.x * run + k;
    if (q < p.slices) { s[0] += part[q * 3]; s[1] += part[q * 3 + 1]; s[2] += part[q * 3 + 2]; }
  }
  for (int i = 0; i < 3; ++i) {
    red[i * 256 + threadIdx.x] = s[i];
    pred_block_tree(red + i * 256);
  }
  if (threadIdx.x < 3) p.mean[(size_t)kn * 3 + threadIdx.x] = red[threadIdx.x * 256] / (float)p.plane;
}

template <bool VEC>
__global__ __launch_bounds__(256) void augment_color_kernel(AugColorParams p) {
#pragma clang fp contract(off)
  const size_t quads = (p.plane + 3) / 4;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)2 * p.N * quads) return;
  const int kn = (int)(idx / quads);
  const size_t pix = (idx - (size_t)kn * quads) * 4;
  const int n = kn < p.N ? kn : kn - p.N;
  const float *src = (kn < p.N ? p.img1 : p.img2) + (size_t)n * 3 * p.plane;
  const float *tb = p.tab + (size_t)n * AC_K;
  float px[3][4], v[3][4];
  ag_load_quad<VEC>(src, p.plane, pix, px);
  ag_color_a(p, tb, kn, (unsigned)(pix / 4), px, v);
  const float bright = tb[AC_BRIGHTNESS], e = tb[AC_E];
  float mean[3], add[3];
  MFN_UNROLL
  for (int i = 0; i < 3; ++i) {
    mean[i] = p.mean_in[(size_t)kn * 3 + i];
    add[i] = mean[i] * tb[AC_CHANNEL + i] + bright;
  }
  MFN_UNROLL
  for (int j = 0; j < 4; ++j) {
    float w[3];
    MFN_UNROLL
    for (int i = 0; i < 3; ++i) w[i] = (v[i][j] - mean[i]) * tb[AC_CC + i];
    if (p.spin) {
      const float w0 = w[0], w1 = w[1], w2 = w[2];
      MFN_UNROLL
      for (int i = 0; i < 3; ++i) w[i] = (tb[AC_SPIN + 3 * i] * w0 + tb[AC_SPIN + 3 * i + 1] * w1) + tb[AC_SPIN + 3 * i + 2] * w2;
    }
    MFN_UNROLL
    for (int i = 0; i < 3; ++i) {
      float o = w[i] + add[i];
      o = fminf(fmaxf(o, 0.f), 1.f);
      if (p.gamma) o = powf(o, e);
      v[i][j] = o;
    }
  }
  float *dst = p.out + (size_t)kn * 3 * p.plane + pix;
  MFN_UNROLL
  for (int i = 0; i < 3; ++i) {
    if (VEC) {
      mfn_store4_stream(dst + (size_t)i * p.plane, v[i][0], v[i][1], v[i][2], v[i][3], p.st_policy);
    } else {
      MFN_UNROLL
      for (int j = 0; j < 4; ++j)
        if (pix + j < p.plane) dst[(size_t)i * p.plane + j] = v[i][j];
    }
  }
}

inline bool augment_color_vec(const AugColorParams &p, const float *out_or_null) {
  return p.plane % 4 == 0 && ((uintptr_t)p.img1 | (uintptr_t)p.img2 | (uintptr_t)out_or_null) % 16 == 0;
}
inline int augment_color_mean_launch(AugColorParams p, hipStream_t stream) {
  if (p.N == 0) return 0;
  const dim3 grid((unsigned)p.slices, (unsigned)(2 * p.N));
  const int rc = augment_color_vec(p, nullptr)
                     ? launch("augment_color_mean_partial", augment_color_mean_partial_kernel<true>, grid, dim3(256), 3 * 256 * sizeof(float), stream, p)
                     : launch("augment_color_mean_partial", augment_color_mean_partial_kernel<false>, grid, dim3(256), 3 * 256 * sizeof(float), stream, p);
  if (rc) return rc;
  return launch("augment_color_mean_final", augment_color_mean_final_kernel, dim3((unsigned)(2 * p.N)), dim3(256), 3 * 256 * sizeof(float), stream, p);
}
inline int augment_color_launch(AugColorParams p, hipStream_t stream) {
  const size_t total = (size_t)2 * p.N * ((p.plane + 3) / 4);
  if (total == 0) return 0;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (augment_color_vec(p, p.out)) return launch("augment_color_v4", augment_color_kernel<true>, grid, dim3(256), 0, stream, p);
  return launch("augment_color_v1", augment_color_kernel<false>, grid, dim3(256), 0, stream, p);
}

}  // namespace mfn
