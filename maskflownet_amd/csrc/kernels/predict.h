// predict.h -- what surrounds the network when it predicts on images of any size.
//
// Replaces the device side of PipelineFlownet.centralize / do_batch_mx / do_batch / validate of
// /root/reference/network/pipeline.py:85-87, :117-147, :176-182:
//   pair_mean      rgb_mean = concat(img1, img2, dim=2).mean(axis=(2,3))                                   (:86)
//   resize         img - rgb_mean, contrib.BilinearResize2D to the next multiple of 64                     (:120-130)
//                  BilinearResize2D back * [H/H64, W/W64] for the flow, plain for the occlusion mask       (:139-142)
//   flow_metrics   EpeLossWithMask (MaskFlownet.py:576-583) and the KITTI outlier ratio                    (:146, :182)
//
// [MXNet-ext, unpinned] BilinearResize2D of MXNet 1.5 (bilinear_resize.cc, align_corners), restated per axis:
//   r  = (out > 1) ? (float)(in-1) / (float)(out-1) : 0.f          p  = r * (float)o      (one fp32 multiply)
//   i0 = (int)p      ip = (i0 < in-1) ? 1 : 0                      l1 = p - (float)i0     l0 = 1.f - l1
//   out = h0*(w0*x[i0][j0] + w1*x[i0][j0+jp]) + h1*(w0*x[i0+ip][j0] + w1*x[i0+ip][j0+jp])
// positions and lambdas in fp32 exactly as written (they are the semantics: an fp64 position moves the result by up to 4e-4 of
// the data range at 375x1242); every product and sum rounded separately (fp contraction off), so the result is the
// expression evaluated in IEEE fp32 -- bit-identical to a numpy fp32 statement of it.  Equal input and output size: a copy.
//
// All four kernels are HBM-bound, one pass over their inputs:
//   resize         4*planes*(Hin*Win + Hout*Wout) bytes        one thread writes 4 adjacent outputs with one 16-byte store
//   pair_mean      8*N*C*H*W bytes                             (+ 4*N*C*slices of partial sums, twice)
//   flow_metrics   20*N*H*W bytes                              (+ 12*N*slices, twice)
// The two reductions run in a fixed order through a caller-supplied workspace, without atomics: a block of 256 threads
// takes a slice of 4096 elements, every thread sums a run of 16 of them (15 additions), an 8-level tree in LDS joins the
// threads (8), one partial sum per slice goes to the workspace; a second kernel, one block per result, sums up to 4096
// partials the same way (15 + 8).  No term passes through more than 46 additions, whatever the image size, and the order
// is a function of the shape alone: bit-identical from run to run.
#pragma once
#include "../mfn_rt.h"

namespace mfn {

enum { PRED_RUN = 16, PRED_SLICE = 256 * PRED_RUN, PRED_MAX_SLICES = 256 * PRED_RUN };

// ---- align-corners bilinear resize [MXNet-ext, unpinned] ---------------------------------------------------------------
struct ResizeParams {
  const float *x;     // planes [0, planes_a) of (Hin, Win)
  const float *x2;    // planes [planes_a, planes): the second image of a pair (preprocess_pair), else unused
  const float *sub;   // optional, one value per plane of ONE input (plane % planes_a): subtracted from every tap before the blend
  float *out;         // (planes, Hout, Wout)
  int planes, planes_a;
  int Hin, Win, Hout, Wout;
  float ry, rx;       // (float)(in-1) / (float)(out-1), 0 for out == 1: formed once on the host in IEEE fp32
  int flow;           // planes alternate (dy, dx): the blend * sy / * sx, one separately rounded multiply (pipeline.py:140-141)
  float sy, sx;       // (float)((double)Hout / (double)Hin), the same of the widths
  int st_policy;      // cache policy of the output stores (mfn_store4_stream)
};

template <int VEC>
__global__ __launch_bounds__(256) void resize_kernel(ResizeParams p) {
#pragma clang fp contract(off)
  const int wv = (p.Wout + VEC - 1) / VEC;
  const size_t total = (size_t)p.planes * p.Hout * wv;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int xv = (int)(idx % wv);
  const int oy = (int)((idx / wv) % p.Hout);
  const int pl = (int)(idx / ((size_t)wv * p.Hout));
  const int pa = pl < p.planes_a ? pl : pl - p.planes_a;
  const float *src = (pl < p.planes_a ? p.x : p.x2) + (size_t)pa * p.Hin * p.Win;
  const float m = p.sub ? p.sub[pa] : 0.f;
  const float scale = p.flow ? ((pl & 1) ? p.sx : p.sy) : 1.f;
  const float py = p.ry * (float)oy;
  const int i0 = min((int)py, p.Hin - 1);      // (int)py <= Hin-1 already (|r*(out-1) - (in-1)| << 1): this only guards the load
  const int ip = i0 < p.Hin - 1 ? 1 : 0;
  const float h1 = py - (float)i0, h0 = 1.f - h1;
  const float *r0 = src + (size_t)i0 * p.Win;
  const float *r1 = r0 + (size_t)ip * p.Win;
  float o[VEC];
  MFN_UNROLL
  for (int k = 0; k < VEC; ++k) {
    const int ox = min(xv * VEC + k, p.Wout - 1);   // VEC == 4 only with Wout % 4 == 0: never clamps there
    const float px = p.rx * (float)ox;
    const int j0 = min((int)px, p.Win - 1);
    const int jp = j0 < p.Win - 1 ? 1 : 0;
    const float w1 = px - (float)j0, w0 = 1.f - w1;
    float a = r0[j0], b = r0[j0 + jp], c = r1[j0], d = r1[j0 + jp];
    if (p.sub) { a = a - m; b = b - m; c = c - m; d = d - m; }
    float v = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d);
    if (p.flow) v = v * scale;
    o[k] = v;
  }
  float *dst = p.out + ((size_t)pl * p.Hout + oy) * p.Wout + (size_t)xv * VEC;
  if (VEC == 4) {
    mfn_store4_stream(dst, o[0], o[1 % VEC], o[2 % VEC], o[3 % VEC], p.st_policy);
  } else {
    dst[0] = o[0];
  }
}

// equal sizes: out = x (- sub) (* scale, which is 1.f for equal sizes), element by element
template <int VEC>
__global__ __launch_bounds__(256) void resize_copy_kernel(ResizeParams p) {
#pragma clang fp contract(off)
  const size_t plane = (size_t)p.Hin * p.Win;
  const size_t pv = plane / VEC;                  // VEC == 4 only with plane % 4 == 0
  const size_t total = (size_t)p.planes * pv;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int pl = (int)(idx / pv);
  const size_t q = (idx - (size_t)pl * pv) * VEC;
  const int pa = pl < p.planes_a ? pl : pl - p.planes_a;
  const float *src = (pl < p.planes_a ? p.x : p.x2) + (size_t)pa * plane + q;
  const float m = p.sub ? p.sub[pa] : 0.f;
  float *dst = p.out + (size_t)pl * plane + q;
  if (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4 *>(src);
    float a = v.x, b = v.y, c = v.z, d = v.w;
    if (p.sub) { a = a - m; b = b - m; c = c - m; d = d - m; }
    mfn_store4_stream(dst, a, b, c, d, p.st_policy);
  } else {
    dst[0] = p.sub ? src[0] - m : src[0];
  }
}

inline int resize_launch(ResizeParams p, hipStream_t stream) {
  if ((size_t)p.planes * p.Hout * p.Wout == 0) return 0;
  const bool al_out = ((uintptr_t)p.out) % 16 == 0;
  if (p.Hin == p.Hout && p.Win == p.Wout) {
    const size_t plane = (size_t)p.Hin * p.Win;
    const bool vec4 = plane % 4 == 0 && al_out && ((uintptr_t)p.x) % 16 == 0 && (p.planes == p.planes_a || ((uintptr_t)p.x2) % 16 == 0);
    const size_t total = (size_t)p.planes * (vec4 ? plane / 4 : plane);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec4) return launch("resize_copy_v4", resize_copy_kernel<4>, grid, dim3(256), 0, stream, p);
    return launch("resize_copy_v1", resize_copy_kernel<1>, grid, dim3(256), 0, stream, p);
  }
  const bool vec4 = p.Wout % 4 == 0 && al_out;
  const size_t total = (size_t)p.planes * p.Hout * (vec4 ? p.Wout / 4 : p.Wout);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (vec4) return launch("resize_v4", resize_kernel<4>, grid, dim3(256), 0, stream, p);
  return launch("resize_v1", resize_kernel<1>, grid, dim3(256), 0, stream, p);
}

// ---- the two fixed-order reductions ------------------------------------------------------------------------------------
// red[0] = the sum of the block's 256 values, in the order of an 8-level tree
__device__ __forceinline__ void pred_block_tree(float *red) {
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
}
inline int pred_slices(size_t elems) { return (int)((elems + PRED_SLICE - 1) / PRED_SLICE); }
__host__ __device__ __forceinline__ int pred_run2(int slices) { return (slices + 255) / 256; }   // partial sums per thread of the second stage: <= PRED_RUN

// joint mean of an image pair: the sequence of (n, c) is plane (n, c) of im1 followed by plane (n, c) of im2
struct PairMeanParams {
  const float *im1, *im2;
  float *partial;     // (planes, slices)
  float *mean;        // (planes)
  size_t plane;       // H * W
  int planes, slices, vec;
};
__global__ __launch_bounds__(256) void pair_mean_partial_kernel(PairMeanParams p) {
  MFN_DYN_SHARED(float, red);
  const int sl = blockIdx.x, pl = blockIdx.y;
  const float *a = p.im1 + (size_t)pl * p.plane, *b = p.im2 + (size_t)pl * p.plane;
  const size_t total = 2 * p.plane, base = (size_t)sl * PRED_SLICE;
  float s = 0.f;
  if (p.vec) {   // plane % 4 == 0 and 16-byte aligned images: a quad never straddles the two planes
    MFN_UNROLL
    for (int k = 0; k < PRED_RUN / 4; ++k) {
      const size_t q = base + 4 * ((size_t)k * 256 + threadIdx.x);
      if (q < total) {
        const float4 v = *reinterpret_cast<const float4 *>(q < p.plane ? a + q : b + (q - p.plane));
        s += (v.x + v.y) + (v.z + v.w);
      }
    }
  } else {
    MFN_UNROLL
    for (int k = 0; k < PRED_RUN; ++k) {
      const size_t q = base + (size_t)k * 256 + threadIdx.x;
      if (q < total) s += q < p.plane ? a[q] : b[q - p.plane];
    }
  }
  red[threadIdx.x] = s;
  pred_block_tree(red);
  if (threadIdx.x == 0) p.partial[(size_t)pl * p.slices + sl] = red[0];
}
__global__ __launch_bounds__(256) void pair_mean_final_kernel(PairMeanParams p) {
  MFN_DYN_SHARED(float, red);
  const int pl = blockIdx.x, run = pred_run2(p.slices);
  const float *part = p.partial + (size_t)pl * p.slices;
  float s = 0.f;
  for (int k = 0; k < run; ++k) {
    const int q = (int)threadIdx.x * run + k;
    if (q < p.slices) s += part[q];
  }
  red[threadIdx.x] = s;
  pred_block_tree(red);
  if (threadIdx.x == 0) p.mean[pl] = red[0] / (float)(2.0 * (double)p.plane);
}
inline int pair_mean_launch(PairMeanParams p, hipStream_t stream) {
  if (p.planes == 0) return 0;
  const int rc = launch("pair_mean_partial", pair_mean_partial_kernel, dim3((unsigned)p.slices, (unsigned)p.planes), dim3(256),
                        256 * sizeof(float), stream, p);
  if (rc) return rc;
  return launch("pair_mean_final", pair_mean_final_kernel, dim3((unsigned)p.planes), dim3(256), 256 * sizeof(float), stream, p);
}

// masked end-point error and outlier sums per sample; flow / label in network order (channel 0 = dy)
struct FlowMetricsParams {
  const float *flow, *label;   // (N, 2, H, W)
  const float *mask;           // (N, 1, H, W)
  float *partial;              // (N, slices, 3)
  float *sums;                 // (N, 3): sum mask * sqrt(|d|^2 + eps), sum mask, sum mask * [|d| > 3 and |d| / (|label| + eps) > 0.05]
  size_t plane;
  int N, slices;
};
// one pixel's terms of the three sums: flow (fy, fx), label (ly, lx), mask m.  The one statement of this arithmetic: every kernel
// that makes these sums (here and in validate.h) adds its pixels through it, in the same order, and so gives the same bits.
__device__ __forceinline__ void flow_metrics_term(float fy, float fx, float ly, float lx, float m, float &s0, float &s1, float &s2) {
  const float eps = 1e-8f;
  const float dy = fy - ly, dx = fx - lx;
  const float sq = dy * dy + dx * dx;
  const float nd = sqrtf(sq), nl = sqrtf(ly * ly + lx * lx);
  s0 += m * sqrtf(sq + eps);
  s1 += m;
  s2 += (nd > 3.f && nd / (nl + eps) > 0.05f) ? m : 0.f;
}
// the block's three sums joined, one tree per sum, each on its own 256 floats: -> partial[0..3)
__device__ __forceinline__ void flow_metrics_block_sums(float *red, float s0, float s1, float s2, float *partial) {
  float s[3] = {s0, s1, s2};
  for (int j = 0; j < 3; ++j) {
    red[j * 256 + threadIdx.x] = s[j];
    pred_block_tree(red + j * 256);
  }
  if (threadIdx.x < 3) partial[threadIdx.x] = red[threadIdx.x * 256];
}
__global__ __launch_bounds__(256) void flow_metrics_partial_kernel(FlowMetricsParams p) {
  MFN_DYN_SHARED(float, red);   // [3][256]
  const int sl = blockIdx.x, n = blockIdx.y;
  const float *f = p.flow + (size_t)n * 2 * p.plane, *l = p.label + (size_t)n * 2 * p.plane, *mk = p.mask + (size_t)n * p.plane;
  const size_t base = (size_t)sl * PRED_SLICE;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  MFN_UNROLL
  for (int k = 0; k < PRED_RUN; ++k) {
    const size_t q = base + (size_t)k * 256 + threadIdx.x;
    if (q < p.plane) flow_metrics_term(f[q], f[p.plane + q], l[q], l[p.plane + q], mk[q], s0, s1, s2);
  }
  flow_metrics_block_sums(red, s0, s1, s2, p.partial + ((size_t)n * p.slices + sl) * 3);
}
__global__ __launch_bounds__(256) void flow_metrics_final_kernel(FlowMetricsParams p) {
  MFN_DYN_SHARED(float, red);
  const int n = blockIdx.x, run = pred_run2(p.slices);
  const float *part = p.partial + (size_t)n * p.slices * 3;
  float s[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < run; ++k) {
    const int q = (int)threadIdx.x * run + k;
    if (q < p.slices) { s[0] += part[q * 3]; s[1] += part[q * 3 + 1]; s[2] += part[q * 3 + 2]; }
  }
  for (int j = 0; j < 3; ++j) {
    red[j * 256 + threadIdx.x] = s[j];
    pred_block_tree(red + j * 256);
  }
  if (threadIdx.x < 3) p.sums[(size_t)n * 3 + threadIdx.x] = red[threadIdx.x * 256];
}
inline int flow_metrics_launch(FlowMetricsParams p, hipStream_t stream) {
  if (p.N == 0) return 0;
  const int rc = launch("flow_metrics_partial", flow_metrics_partial_kernel, dim3((unsigned)p.slices, (unsigned)p.N), dim3(256),
                        3 * 256 * sizeof(float), stream, p);
  if (rc) return rc;
  return launch("flow_metrics_final", flow_metrics_final_kernel, dim3((unsigned)p.N), dim3(256), 3 * 256 * sizeof(float), stream, p);
}

}  // namespace mfn
