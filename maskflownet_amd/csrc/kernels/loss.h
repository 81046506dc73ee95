// loss.h -- the multiscale end-point-error training loss, forward and backward, fused.
//
// Replaces the composition of /root/reference/network/MaskFlownet.py:563-611 (EpeLossWithMask, MultiscaleEpe with
// match='upsampling') as network/pipeline.py:42-44 builds it and :82 calls it: per scale s with factor f_s, weight w_s and
// prediction p_s (N,2,H/f_s,W/f_s)
//   u_s = Upsample(f_s)(p_s)                     d = u_s - label
//   L   = sqrt(d_y^2 + d_x^2 + eps)              or (|d_y| + |d_x| + eps)^q   (optimizer.q of the Sintel / KITTI schedules)
//   sum_s[n] = sum_pix mask[n,pix] * L           msum[n] = sum mask[n]        loss[n] = sum_s w_s * sum_s[n] / msum[n]
// mask: a plane (N,1,H,W), or one value per sample (N,1,1,1): the reference's broadcast then gives msum[n] = mask[n] and a
// numerator over all pixels.  msum == 0 is the reference's 0 / 0 for that sample.
//
// u_s is never written: both directions recompute it per pixel through upsample_row / upsample_col / upsample_blend
// (upsample.h), the arithmetic of upsample_kernel itself, so it has upsample_kernel's bits.  That matters: with eps = 1e-8
// dL/dd is sign(d) (robust form) or has slope 1e4 (sqrt form) at d = 0, and an ulp of u decides an O(1) part of a term.
// Everything here is evaluated as written, every product and sum rounded separately (fp contraction off).
//
// Forward: one pass over the full-resolution pixels for all scales of the call.  A block of 256 threads takes a slice of 2048
// pixels, a thread 8 of them (two 16-byte loads per label channel and mask where W % 4 == 0 and the pointers are aligned,
// scalar loads otherwise); the 2 x 2 taps of every prediction come from the small, cache-resident tensors.  The S + 1 sums
// meet in LDS in one fixed 8-level tree, a partial per slice goes to the workspace, a second kernel (one block per sample)
// adds up to 4096 partials the same way and forms the loss.  No atomics; no term passes through more than 40 additions;
// bit-identical from run to run.
//   bytes: 12 * N * H * W (label and mask, once) + the predictions (1.33 / 16 * 8 * N * H * W at the default scales)
//          = 18.9 MB + 1.0 MB at N = 8, 384 x 512; partial sums 4 * N * slices * (S + 1), written and read once.
//
// Backward (gradients of the predictions only; nothing is saved by the forward but `sums`):
//   gp_s[n,c,iy,ix] = gloss[n] * w_s / msum[n] * sum_footprint k_y k_x * mask * dL/dd_c
//   dL/dd_c = d_c / sqrt(..)   or   q * (..)^(q-1) * sign(d_c), sign(0) = 0
// Owner computes: the (2f-1)^2 triangle footprint of an input pixel -- the clamped extra row / column of the edge pad lands on
// the last input row / column, as in upsample_bwd_kernel -- is walked by T threads that recompute d from p_s and label, both
// channels at once; T = 1 (f <= 4: 49 terms), 8 x 8 (f <= 16: 961 terms) or 16 x 16 (f = 64: 16 129 terms) threads, each with a
// strided share of the footprint's rows and columns, their partial sums joined in LDS in a fixed order.  The triangle weights
// come from a table of upsample_tri's values that every block builds in LDS (2f - 1 floats), divisions by f are multiply-shift:
// a term costs no IEEE division but the loss's own.  One launch per scale.  No atomics, fixed order, bit-identical replays;
// masked-out pixels add no term.
//   bytes: the algorithmic minimum is the forward's (label and mask once per scale: 5 * 18.9 MB at the training shape); every
//   full-resolution pixel lies in the footprint of (2 - 1/f)^2 input pixels, so label and mask are re-read 2.25 (f = 2) to 3.9
//   (f = 64) times per scale, out of L2: neighbouring footprints overlap and a scale's working set per block row is a few rows.
#pragma once
#include "../mfn_rt.h"
#include "upsample.h"

namespace mfn {

enum { LOSS_MAX_SCALES = 8, LOSS_MAX_FACTOR = 512, LOSS_RUN = 8, LOSS_SLICE = 256 * LOSS_RUN, LOSS_MAX_SLICES = 256 * 16 };

// L and dL/dd of one pixel
__device__ __forceinline__ float loss_value(float dy, float dx, float eps, int robust, float q) {
#pragma clang fp contract(off)
  if (robust) return powf((fabsf(dy) + fabsf(dx)) + eps, q);
  return sqrtf((dy * dy + dx * dx) + eps);
}
__device__ __forceinline__ void loss_slope(float dy, float dx, float eps, int robust, float q, float &gy, float &gx) {
#pragma clang fp contract(off)
  if (robust) {
    const float t = q * powf((fabsf(dy) + fabsf(dx)) + eps, q - 1.f);
    gy = dy > 0.f ? t : (dy < 0.f ? -t : 0.f);
    gx = dx > 0.f ? t : (dx < 0.f ? -t : 0.f);
  } else {
    const float r = sqrtf((dy * dy + dx * dx) + eps);
    gy = dy / r;
    gx = dx / r;
  }
}
// The 2f - 1 triangle weights of a factor, upsample_tri's own values, once per block into LDS: every weight of the block is
// then a lookup instead of an IEEE division (eight of them per term otherwise).  The caller places the barrier.
__device__ __forceinline__ void loss_fill_tri(float *tab, int f) {
  for (int a = threadIdx.x; a < 2 * f - 1; a += 256) tab[a] = upsample_tri(f - 1, a);
}

struct LossFwdParams {
  const float *pred[LOSS_MAX_SCALES];   // (N,2,H/f,W/f)
  int f[LOSS_MAX_SCALES];
  unsigned magic[LOSS_MAX_SCALES];      // mfn_make_magic(f): x / f for x < H, W (exact while x * f < 2^32; f <= min(H, W) and H * W <= 2^23 here)
  float w[LOSS_MAX_SCALES];
  int S;
  const float *label, *mask;            // (N,2,H,W); (N,1,H,W) or (N)
  float *partial;                       // (N, slices, S+1)
  float *sums;                          // (N, S+1): the S masked sums, msum
  float *loss;                          // (N)
  int N, H, W, slices, mask_scalar, robust;
  float eps, q;
};

template <int VEC>
__global__ __launch_bounds__(256) void multiscale_epe_partial_kernel(LossFwdParams p) {
#pragma clang fp contract(off)
  MFN_DYN_SHARED(float, red);   // [S+1][256], then the scales' weight tables
  float *tabs = red + (p.S + 1) * 256;
  {
    int off = 0;
    for (int s = 0; s < p.S; ++s) {
      loss_fill_tri(tabs + off, p.f[s]);
      off += 2 * p.f[s] - 1;
    }
  }
  __syncthreads();
  const int sl = blockIdx.x, n = blockIdx.y;
  const size_t plane = (size_t)p.H * p.W;
  const float *ly = p.label + (size_t)n * 2 * plane, *lx = ly + plane;
  const float *mk = p.mask_scalar ? nullptr : p.mask + (size_t)n * plane;
  const float mconst = p.mask_scalar ? p.mask[n] : 0.f;
  const size_t base = (size_t)sl * LOSS_SLICE;
  float acc[LOSS_MAX_SCALES + 1];
  MFN_UNROLL
  for (int s = 0; s <= LOSS_MAX_SCALES; ++s) acc[s] = 0.f;
  for (int k = 0; k < LOSS_RUN / VEC; ++k) {
    const size_t q0 = base + ((size_t)k * 256 + threadIdx.x) * VEC;
    if (q0 >= plane) continue;
    const int oy = (int)(q0 / p.W), ox0 = (int)(q0 - (size_t)oy * p.W);   // VEC == 4 only with W % 4 == 0: one row
    float vy[VEC], vx[VEC], m[VEC];
    if (VEC == 4) {
      const float4 a = *reinterpret_cast<const float4 *>(ly + q0), b = *reinterpret_cast<const float4 *>(lx + q0);
      vy[0] = a.x; vy[1 % VEC] = a.y; vy[2 % VEC] = a.z; vy[3 % VEC] = a.w;
      vx[0] = b.x; vx[1 % VEC] = b.y; vx[2 % VEC] = b.z; vx[3 % VEC] = b.w;
      if (mk) {
        const float4 c = *reinterpret_cast<const float4 *>(mk + q0);
        m[0] = c.x; m[1 % VEC] = c.y; m[2 % VEC] = c.z; m[3 % VEC] = c.w;
      } else {
        m[0] = m[1 % VEC] = m[2 % VEC] = m[3 % VEC] = mconst;
      }
    } else {
      vy[0] = ly[q0]; vx[0] = lx[q0]; m[0] = mk ? mk[q0] : mconst;
    }
    MFN_UNROLL
    for (int j = 0; j < VEC; ++j) acc[LOSS_MAX_SCALES] += m[j];
    int off = 0;
    MFN_UNROLL
    for (int s = 0; s < LOSS_MAX_SCALES; ++s) {
      if (s < p.S) {
        const int f = p.f[s], h = p.H / f, w = p.W / f;
        const float *tab = tabs + off;
        const unsigned magic = p.magic[s];
        auto tri = [tab](int a) { return tab[a]; };
        auto div = [magic](int o) { return (int)mfn_div_magic((unsigned)o, magic); };
        const float *py = p.pred[s] + (size_t)n * 2 * h * w, *px = py + (size_t)h * w;
        const UpsampleRow row = upsample_row(h, w, f, oy, tri, div);
        // the four pixels of a quad mostly share their 2 x 2 taps (always where f % 4 == 0): loaded once, reused where the cell is the same
        const UpsampleCol col0 = upsample_col(w, f, ox0, tri, div);
        float ty[2][2], tx[2][2];
        MFN_UNROLL
        for (int rs = 0; rs < 2; ++rs) {
          MFN_UNROLL
          for (int cs = 0; cs < 2; ++cs) {
            ty[rs][cs] = UpsamplePlane{py, row, col0}(rs, cs);
            tx[rs][cs] = UpsamplePlane{px, row, col0}(rs, cs);
          }
        }
        MFN_UNROLL
        for (int j = 0; j < VEC; ++j) {
          const UpsampleCol col = j ? upsample_col(w, f, ox0 + j, tri, div) : col0;
          const bool same = col.ix0 == col0.ix0;
          auto ldy = [&](int rs, int cs) { return same ? ty[rs][cs] : UpsamplePlane{py, row, col}(rs, cs); };
          auto ldx = [&](int rs, int cs) { return same ? tx[rs][cs] : UpsamplePlane{px, row, col}(rs, cs); };
          const float dy = upsample_blend(ldy, row, col) - vy[j], dx = upsample_blend(ldx, row, col) - vx[j];
          acc[s] += m[j] * loss_value(dy, dx, p.eps, p.robust, p.q);
        }
        off += 2 * f - 1;
      }
    }
  }
  MFN_UNROLL
  for (int s = 0; s < LOSS_MAX_SCALES; ++s)
    if (s < p.S) red[s * 256 + threadIdx.x] = acc[s];
  red[p.S * 256 + threadIdx.x] = acc[LOSS_MAX_SCALES];
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {   // one tree for the S + 1 sums, each on its own 256 floats
    if ((int)threadIdx.x < st)
      for (int s = 0; s <= p.S; ++s) red[s * 256 + threadIdx.x] += red[s * 256 + threadIdx.x + st];
    __syncthreads();
  }
  if ((int)threadIdx.x <= p.S) p.partial[((size_t)n * p.slices + sl) * (p.S + 1) + threadIdx.x] = red[threadIdx.x * 256];
}

__global__ __launch_bounds__(256) void multiscale_epe_final_kernel(LossFwdParams p) {
#pragma clang fp contract(off)
  MFN_DYN_SHARED(float, red);   // [S+1][256]
  const int n = blockIdx.x, S1 = p.S + 1, run = (p.slices + 255) / 256;
  const float *part = p.partial + (size_t)n * p.slices * S1;
  for (int s = 0; s < S1; ++s) {
    float v = 0.f;
    for (int k = 0; k < run; ++k) {
      const int i = (int)threadIdx.x * run + k;
      if (i < p.slices) v += part[(size_t)i * S1 + s];
    }
    red[s * 256 + threadIdx.x] = v;
  }
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if ((int)threadIdx.x < st)
      for (int s = 0; s < S1; ++s) red[s * 256 + threadIdx.x] += red[s * 256 + threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float msum = p.mask_scalar ? p.mask[n] : red[p.S * 256];
    float total = 0.f;
    for (int s = 0; s < p.S; ++s) {
      p.sums[(size_t)n * S1 + s] = red[s * 256];
      total = total + p.w[s] * red[s * 256] / msum;
    }
    p.sums[(size_t)n * S1 + p.S] = msum;
    p.loss[n] = total;
  }
}

inline int loss_slices(size_t plane) { return (int)((plane + LOSS_SLICE - 1) / LOSS_SLICE); }

inline int multiscale_epe_fwd_launch(LossFwdParams p, hipStream_t stream) {
  if (p.N == 0) return 0;
  bool vec4 = p.W % 4 == 0 && ((uintptr_t)p.label) % 16 == 0 && (p.mask_scalar || ((uintptr_t)p.mask) % 16 == 0);
  const dim3 grid((unsigned)p.slices, (unsigned)p.N);
  size_t tabs = 0;
  for (int s = 0; s < p.S; ++s) tabs += 2 * p.f[s] - 1;
  const size_t red = (size_t)(p.S + 1) * 256 * sizeof(float), lds = red + tabs * sizeof(float);
  const int rc = vec4 ? launch("multiscale_epe_partial_v4", multiscale_epe_partial_kernel<4>, grid, dim3(256), lds, stream, p)
                      : launch("multiscale_epe_partial_v1", multiscale_epe_partial_kernel<1>, grid, dim3(256), lds, stream, p);
  if (rc) return rc;
  return launch("multiscale_epe_final", multiscale_epe_final_kernel, dim3((unsigned)p.N), dim3(256), red, stream, p);
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
struct LossBwdParams {
  const float *pred;                    // (N,2,h,w) of this scale
  float *gpred;
  int f, add;
  unsigned magic;                       // mfn_make_magic(f)
  float w;
  const float *label, *mask, *gloss, *sums;   // sums: (N, S1), msum in column S1 - 1
  int S1;
  int N, H, W, h, wd, mask_scalar, robust;
  float eps, q;
};

// TY x TX threads per input pixel (thread (ly, lx) takes the footprint's rows ly, ly + TY, .. and columns lx, lx + TX, ..),
// 256 / (TY TX) pixels per block
template <int TY, int TX>
__global__ __launch_bounds__(256) void multiscale_epe_bwd_kernel(LossBwdParams p) {
#pragma clang fp contract(off)
  constexpr int T = TY * TX;
  constexpr int P = 256 / T;    // input pixels per block
  MFN_DYN_SHARED(float, tab);   // [2f-1] weights, then [18][P] the pixels' 3 x 3 x 2 input patches, then [2][256] partial sums (T > 1)
  const int f = p.f;
  float *patch = tab + (2 * f - 1), *red = patch + 18 * P;
  loss_fill_tri(tab, f);
  const unsigned magic = p.magic;
  auto tri = [tab](int a) { return tab[a]; };
  auto div = [magic](int o) { return (int)mfn_div_magic((unsigned)o, magic); };
  const size_t total = (size_t)p.N * p.h * p.wd;
  const size_t idx = (size_t)blockIdx.x * (256 / T) + threadIdx.x / T;
  const int lane = (int)threadIdx.x % T, lyy = lane / TX, lxx = lane % TX;
  const int pix = (int)threadIdx.x / T;
  const bool live = idx < total;
  float sy = 0.f, sx = 0.f;
  const int ix = (int)(idx % p.wd), iy = (int)((idx / p.wd) % p.h), n = (int)(idx / ((size_t)p.wd * p.h));
  if (live) {   // entry (c, dy, dx) of the patch: p[n, c, clamp(iy + dy - 1), clamp(ix + dx - 1)]; every tap of the footprint is one of them
    const float *src = p.pred + (size_t)n * 2 * p.h * p.wd;
    for (int k = lane; k < 18; k += T) {
      const int c = k / 9, dy = (k - c * 9) / 3, dx = k - c * 9 - dy * 3;
      patch[k * P + pix] = src[((size_t)c * p.h + min(max(iy + dy - 1, 0), p.h - 1)) * p.wd + min(max(ix + dx - 1, 0), p.wd - 1)];
    }
  }
  __syncthreads();
  if (live) {
    const size_t plane = (size_t)p.H * p.W;
    const float *ly = p.label + (size_t)n * 2 * plane, *lx = ly + plane;
    const float *mk = p.mask_scalar ? nullptr : p.mask + (size_t)n * plane;
    const float mconst = p.mask_scalar ? p.mask[n] : 0.f;
    // the footprint of input pixel (iy, ix), as upsample_bwd_kernel has it: input line i receives the weight of output line o's
    // upper tap when o / f == i and that of its lower tap when min(o / f + 1, lines - 1) == i (the edge pad: both on the last line)
    const int oy_lo = max((iy - 1) * f + 1, 0), oy_hi = min((iy + 1) * f - 1, p.H - 1);
    const int ox_lo = max((ix - 1) * f + 1, 0), ox_hi = min((ix + 1) * f - 1, p.W - 1);
    for (int oy = oy_lo + lyy; oy <= oy_hi; oy += TY) {
      const UpsampleRow row = upsample_row(p.h, p.wd, f, oy, tri, div);
      float wy = 0.f;
      if (row.i0 == iy) wy += row.ka0;
      if (row.ry && row.i1 == iy) wy += row.ka1;
      const size_t qrow = (size_t)oy * p.W;
      for (int ox = ox_lo + lxx; ox <= ox_hi; ox += TX) {
        const float m = mk ? mk[qrow + ox] : mconst;
        if (m != 0.f) {
          const UpsampleCol col = upsample_col(p.wd, f, ox, tri, div);
          float wx = 0.f;
          if (col.ix0 == ix) wx += col.kb0;
          if (col.rx && col.ix1 == ix) wx += col.kb1;
          auto ldy = [&](int rs, int cs) { return patch[(((rs ? row.i1 : row.i0) - iy + 1) * 3 + ((cs ? col.ix1 : col.ix0) - ix + 1)) * P + pix]; };
          auto ldx = [&](int rs, int cs) { return patch[(9 + ((rs ? row.i1 : row.i0) - iy + 1) * 3 + ((cs ? col.ix1 : col.ix0) - ix + 1)) * P + pix]; };
          const float dy = upsample_blend(ldy, row, col) - ly[qrow + ox], dx = upsample_blend(ldx, row, col) - lx[qrow + ox];
          float gy, gx;
          loss_slope(dy, dx, p.eps, p.robust, p.q, gy, gx);
          const float km = (wy * wx) * m;
          sy += km * gy;
          sx += km * gx;
        }
      }
    }
  }
  if (T > 1) {   // the pixel's TY x TX partial sums meet in LDS in a fixed order: every row's TX values, then the TY row sums
    red[threadIdx.x] = sy;
    red[256 + threadIdx.x] = sx;
    __syncthreads();
    if (lxx == 0) {
      for (int j = 1; j < TX; ++j) {
        sy += red[threadIdx.x + j];
        sx += red[256 + threadIdx.x + j];
      }
      red[threadIdx.x] = sy;
      red[256 + threadIdx.x] = sx;
    }
    __syncthreads();
    if (lane == 0) {
      for (int j = 1; j < TY; ++j) {
        sy += red[threadIdx.x + j * TX];
        sx += red[256 + threadIdx.x + j * TX];
      }
    }
  }
  if (live && lane == 0) {
    const float coef = p.gloss[n] * p.w / p.sums[(size_t)n * p.S1 + p.S1 - 1];
    const size_t hw = (size_t)p.h * p.wd;
    float *gy = p.gpred + (size_t)n * 2 * hw + (idx - (size_t)n * hw), *gx = gy + hw;
    const float vy = coef * sy, vx = coef * sx;
    *gy = p.add ? *gy + vy : vy;
    *gx = p.add ? *gx + vx : vx;
  }
}

inline int loss_bwd_threads(int f) { return f <= 4 ? 1 : (f <= 16 ? 64 : 256); }

inline int multiscale_epe_bwd_launch(LossBwdParams p, hipStream_t stream) {
  const size_t total = (size_t)p.N * p.h * p.wd;
  if (total == 0) return 0;
  const int T = loss_bwd_threads(p.f);
  const dim3 grid((unsigned)((total + 256 / T - 1) / (256 / T)));
  const size_t lds = (size_t)(2 * p.f - 1 + 18 * (256 / T) + (T > 1 ? 512 : 0)) * sizeof(float);
  if (T == 1) return launch("multiscale_epe_bwd_t1", multiscale_epe_bwd_kernel<1, 1>, grid, dim3(256), lds, stream, p);
  if (T == 64) return launch("multiscale_epe_bwd_t64", multiscale_epe_bwd_kernel<8, 8>, grid, dim3(256), lds, stream, p);
  return launch("multiscale_epe_bwd_t256", multiscale_epe_bwd_kernel<16, 16>, grid, dim3(256), lds, stream, p);
}

}  // namespace mfn
