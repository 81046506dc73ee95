// validate.h -- a validation batch read where the data set lies: pairs, labels and masks through a BatchRow table.
//
// Replaces, for samples that are resident in HBM as the readers store them (data.DeviceDataset), what PipelineFlownet.validate of the
// reference's network/pipeline.py:149-187 does to a batch on the host before and after the network, and the uploads in between:
//   val_pair_mean      rgb_mean of :86 on the bytes / 255 of :208                                    = pair_mean_u8 (frames.h)
//   val_preprocess     `/ 255`, HWC -> CHW, - rgb_mean, BilinearResize2D of both images (:120-130)   = preprocess_pair_u8 (frames.h)
//   val_flow_metrics   the label flipped to (v, u) (:176), the mask byte / 255 (:175), EpeLossWithMask and the KITTI outlier sums
//                      (:146, :182)                                                                  = flow_metrics (predict.h)
// Each gives the BITS of the operator named on the right run on the same bytes gathered into one tensor: the arithmetic is that
// operator's, statement for statement (fp contraction as there), the reductions are its slices of PRED_SLICE, runs of PRED_RUN and
// trees, and the second stages are its own kernels.  Only where a byte comes from differs.
//
// The slots are rows of the table of batch.h (mfn_batch_gather_build_rows), device resident: blockIdx.y is the slot (the image, for
// val_preprocess), so the row is a wave-uniform read; its pointers are cast to the global address space once (bg_ld*).  Every slot is
// the whole sample: Hs == H, Ws == W, y0 == x0 == 0, flip == 0 -- the caller checks that on the host copy of the table before any
// launch (ops.py), the kernels do not look at those fields.
//
// READ CONTRACT (batch.h's).  Every source starts at a 16-byte aligned address and is readable up to the next multiple of 16 bytes
// of its size.  Dword loads are taken at addresses that are multiples of 4 and begin inside the array's own bytes; everything else
// is read byte by byte.  Nothing outside that extent is touched.
//
// HBM-bound single passes: val_pair_mean 6*N*H*W bytes, val_preprocess 6*N*H*W + 24*N*Hout*Wout, val_flow_metrics (8 + 8|4 + 1)*N*H*W.
// No LDS beyond the reduction trees, no atomics, fixed summation order.
#pragma once
#include "../mfn_rt.h"
#include "batch.h"
#include "frames.h"

namespace mfn {

typedef const MFN_BATCH_GLOBAL unsigned char *val_bytes;   // a source array, as the table names it, in the global address space
__device__ __forceinline__ val_bytes val_global(const void *p) { return (val_bytes)p; }
__device__ __forceinline__ unsigned val_ld32(val_bytes p) { return *(const MFN_BATCH_GLOBAL unsigned *)p; }

// ---- the joint mean of the slots' pairs, exact: the first stage of pair_mean_u8 over two arrays --------------------------------------
struct ValPairMeanParams {
  const BatchRow *rows;
  PairMeanU8Params fin;   // partial (N, slices, 3), mean (N, 3), plane, denom, N, slices: the second stage is pair_mean_u8_final_kernel
};
// the pixel sequence of slot n: the H*W pixels of img1 followed by those of img2; a thread sums a run of 16 of them
__global__ __launch_bounds__(256) void val_pair_mean_partial_kernel(ValPairMeanParams p) {
  MFN_DYN_SHARED(unsigned, red);   // [3][256]
  const int sl = blockIdx.x, n = blockIdx.y;
  const BatchRow r = p.rows[n];    // wave-uniform: indexed by the block
  const val_bytes fa = val_global(r.img1), fb = val_global(r.img2);
  const size_t plane = p.fin.plane, total = 2 * plane;
  const size_t q0 = (size_t)sl * PRED_SLICE + (size_t)threadIdx.x * PRED_RUN;
  unsigned s[3] = {0u, 0u, 0u};
  if (q0 < total) {
    const bool first = q0 < plane;
    const val_bytes src = first ? fa + 3 * q0 : fb + 3 * (q0 - plane);
    const size_t end = first ? plane : total;   // where the run's image ends
    if (q0 + PRED_RUN <= end && ((uintptr_t)src & 3) == 0) {   // 48 bytes inside one image from an aligned address: 12 words
      MFN_UNROLL
      for (int k = 0; k < 3 * PRED_RUN / 4; ++k) {
        const unsigned v = val_ld32(src + 4 * k);
        s[(4 * k) % 3] += v & 255u;
        s[(4 * k + 1) % 3] += (v >> 8) & 255u;
        s[(4 * k + 2) % 3] += (v >> 16) & 255u;
        s[(4 * k + 3) % 3] += v >> 24;
      }
    } else {
      for (int k = 0; k < PRED_RUN; ++k) {
        const size_t q = q0 + k;
        if (q < total) {
          const val_bytes px = q < plane ? fa + 3 * q : fb + 3 * (q - plane);
          s[0] += px[0]; s[1] += px[1]; s[2] += px[2];
        }
      }
    }
  }
  for (int c = 0; c < 3; ++c) {
    red[c * 256 + threadIdx.x] = s[c];
    frames_block_tree(red + c * 256, [](unsigned a, unsigned b) { return a + b; });
  }
  if (threadIdx.x < 3) p.fin.partial[((size_t)n * p.fin.slices + sl) * 3 + threadIdx.x] = red[threadIdx.x * 256];
}
inline int val_pair_mean_launch(ValPairMeanParams p, hipStream_t stream) {
  if (p.fin.N == 0) return 0;
  const int rc = launch("val_pair_mean_partial", val_pair_mean_partial_kernel, dim3((unsigned)p.fin.slices, (unsigned)p.fin.N), dim3(256),
                        3 * 256 * sizeof(unsigned), stream, p);
  if (rc) return rc;
  return launch("pair_mean_u8_final", pair_mean_u8_final_kernel, dim3((unsigned)p.fin.N), dim3(256), 3 * 256 * sizeof(unsigned long long),
                stream, p.fin);
}

// ---- / 255, HWC -> CHW, - mean, align-corners bilinear resize of both images: frames_resize_kernel / frames_unpack_kernel per slot -----
struct ValPreParams {
  const BatchRow *rows;
  const float *mean;   // (N, 3) or NULL: no subtraction
  float *out;          // (2N, 3, Hout, Wout): image 1 of slot n in row n, image 2 in row N + n
  int N, H, W, Hout, Wout;
  float ry, rx;        // as ResizeParams
  int st_policy;
};
// blockIdx.y: the image of the output batch; -> its slot and its bytes
__device__ __forceinline__ val_bytes val_image(const ValPreParams &p, int img, int &n) {
  n = img < p.N ? img : img - p.N;
  const BatchRow r = p.rows[n];
  return val_global(img < p.N ? r.img1 : r.img2);
}

template <int VEC>
__global__ __launch_bounds__(256) void val_resize_kernel(ValPreParams p) {
#pragma clang fp contract(off)
  const int wv = (p.Wout + VEC - 1) / VEC;
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= (unsigned)p.Hout * (unsigned)wv) return;
  const int xv = (int)(idx % (unsigned)wv), oy = (int)(idx / (unsigned)wv);
  const int img = blockIdx.y;
  int n;
  const val_bytes src = val_image(p, img, n);
  float m[3] = {0.f, 0.f, 0.f};
  if (p.mean) { m[0] = p.mean[n * 3]; m[1] = p.mean[n * 3 + 1]; m[2] = p.mean[n * 3 + 2]; }
  const float py = p.ry * (float)oy;
  const int i0 = min((int)py, p.H - 1);
  const int ip = i0 < p.H - 1 ? 1 : 0;
  const float h1 = py - (float)i0, h0 = 1.f - h1;
  const val_bytes r0 = src + (size_t)i0 * p.W * 3;
  const val_bytes r1 = r0 + (size_t)ip * p.W * 3;
  float o[3][VEC];
  MFN_UNROLL
  for (int k = 0; k < VEC; ++k) {
    const int ox = min(xv * VEC + k, p.Wout - 1);   // VEC == 4 only with Wout % 4 == 0: never clamps there
    const float px = p.rx * (float)ox;
    const int j0 = min((int)px, p.W - 1);
    const int jp = j0 < p.W - 1 ? 1 : 0;
    const float w1 = px - (float)j0, w0 = 1.f - w1;
    MFN_UNROLL
    for (int c = 0; c < 3; ++c) {
      float a = (float)r0[j0 * 3 + c] / 255.f, b = (float)r0[(j0 + jp) * 3 + c] / 255.f;
      float cc = (float)r1[j0 * 3 + c] / 255.f, d = (float)r1[(j0 + jp) * 3 + c] / 255.f;
      if (p.mean) { a = a - m[c]; b = b - m[c]; cc = cc - m[c]; d = d - m[c]; }
      o[c][k] = h0 * (w0 * a + w1 * b) + h1 * (w0 * cc + w1 * d);
    }
  }
  MFN_UNROLL
  for (int c = 0; c < 3; ++c) {
    float *dst = p.out + (((size_t)img * 3 + c) * p.Hout + oy) * p.Wout + (size_t)xv * VEC;
    if (VEC == 4) {
      mfn_store4_stream(dst, o[c][0], o[c][1 % VEC], o[c][2 % VEC], o[c][3 % VEC], p.st_policy);
    } else {
      dst[0] = o[c][0];
    }
  }
}

// equal sizes: out = byte / 255 (- mean), a pure unpack into float CHW
template <int VEC>
__global__ __launch_bounds__(256) void val_unpack_kernel(ValPreParams p) {
#pragma clang fp contract(off)
  const size_t plane = (size_t)p.H * p.W;
  const size_t pv = plane / VEC;                  // VEC == 4 only with plane % 4 == 0
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= pv) return;
  const size_t q = idx * VEC;
  const int img = blockIdx.y;
  int n;
  const val_bytes src = val_image(p, img, n) + q * 3;   // VEC == 4: 12 * idx bytes behind a 16-byte aligned address, a multiple of 4
  float m[3] = {0.f, 0.f, 0.f};
  if (p.mean) { m[0] = p.mean[n * 3]; m[1] = p.mean[n * 3 + 1]; m[2] = p.mean[n * 3 + 2]; }
  unsigned char by[3 * VEC];
  if (VEC == 4 && ((uintptr_t)src & 3) == 0) {    // 12 bytes inside the image from an aligned address: 3 words
    MFN_UNROLL
    for (int k = 0; k < 3 * VEC / 4; ++k) {
      const unsigned v = val_ld32(src + 4 * k);
      by[4 * k] = (unsigned char)(v & 255u); by[4 * k + 1] = (unsigned char)((v >> 8) & 255u);
      by[4 * k + 2] = (unsigned char)((v >> 16) & 255u); by[4 * k + 3] = (unsigned char)(v >> 24);
    }
  } else {
    MFN_UNROLL
    for (int k = 0; k < 3 * VEC; ++k) by[k] = src[k];
  }
  MFN_UNROLL
  for (int c = 0; c < 3; ++c) {
    float o[VEC];
    MFN_UNROLL
    for (int k = 0; k < VEC; ++k) {
      const float x = (float)by[3 * k + c] / 255.f;
      o[k] = p.mean ? x - m[c] : x;
    }
    float *dst = p.out + ((size_t)img * 3 + c) * plane + q;
    if (VEC == 4) {
      mfn_store4_stream(dst, o[0], o[1 % VEC], o[2 % VEC], o[3 % VEC], p.st_policy);
    } else {
      dst[0] = o[0];
    }
  }
}

// the store rules of frames_pre_launch: 16-byte stores when the row length (the plane, for the unpack) is a multiple of 4 and out is aligned
inline int val_pre_launch(ValPreParams p, hipStream_t stream) {
  if ((size_t)p.N * p.Hout * p.Wout == 0) return 0;
  const bool al_out = ((uintptr_t)p.out) % 16 == 0;
  if (p.H == p.Hout && p.W == p.Wout) {
    const size_t plane = (size_t)p.H * p.W;
    const bool vec4 = plane % 4 == 0 && al_out;
    const dim3 grid((unsigned)(((vec4 ? plane / 4 : plane) + 255) / 256), 2u * (unsigned)p.N);
    if (vec4) return launch("val_unpack_v4", val_unpack_kernel<4>, grid, dim3(256), 0, stream, p);
    return launch("val_unpack_v1", val_unpack_kernel<1>, grid, dim3(256), 0, stream, p);
  }
  const bool vec4 = p.Wout % 4 == 0 && al_out;
  const size_t items = (size_t)p.Hout * (vec4 ? p.Wout / 4 : p.Wout);
  const dim3 grid((unsigned)((items + 255) / 256), 2u * (unsigned)p.N);
  if (vec4) return launch("val_resize_v4", val_resize_kernel<4>, grid, dim3(256), 0, stream, p);
  return launch("val_resize_v1", val_resize_kernel<1>, grid, dim3(256), 0, stream, p);
}

// ---- masked end-point error and outlier sums per slot: the first stage of flow_metrics with the label and the mask as stored ---------
struct ValMetricsParams {
  const BatchRow *rows;
  FlowMetricsParams fin;   // flow (N,2,H,W), partial (N, slices, 3), sums (N,3), plane, N, slices: the second stage is flow_metrics_final_kernel
};
__global__ __launch_bounds__(256) void val_flow_metrics_partial_kernel(ValMetricsParams p) {
  MFN_DYN_SHARED(float, red);   // [3][256]
  const int sl = blockIdx.x, n = blockIdx.y;
  const BatchRow r = p.rows[n];    // wave-uniform: indexed by the block
  const size_t plane = p.fin.plane;
  const float *f = p.fin.flow + (size_t)n * 2 * plane;
  const unsigned char *lab = (const unsigned char *)r.flow;
  const val_bytes mk = val_global(r.mask);
  const bool half = r.label_type == BATCH_LABEL_F16, masked = r.mask != nullptr;
  const size_t base = (size_t)sl * PRED_SLICE;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  MFN_UNROLL
  for (int k = 0; k < PRED_RUN; ++k) {
    const size_t q = base + (size_t)k * 256 + threadIdx.x;
    if (q < plane) {
      unsigned u, v;   // the stored pair is (u, v) = (dx, dy): channel 0 of the network order is v
      if (half) {
        const unsigned w = bg_ld32(lab + 4 * q);
        u = bg_half_bits(w & 0xffffu);
        v = bg_half_bits(w >> 16);
      } else {
        const bg_u32x2 w = bg_ld64(lab + 8 * q);
        u = w.x;
        v = w.y;
      }
      const float m = masked ? (float)mk[q] / 255.f : 1.f;
      flow_metrics_term(f[q], f[plane + q], __builtin_bit_cast(float, v), __builtin_bit_cast(float, u), m, s0, s1, s2);
    }
  }
  flow_metrics_block_sums(red, s0, s1, s2, p.fin.partial + ((size_t)n * p.fin.slices + sl) * 3);
}
inline int val_flow_metrics_launch(ValMetricsParams p, hipStream_t stream) {
  if (p.fin.N == 0) return 0;
  const int rc = launch("val_flow_metrics_partial", val_flow_metrics_partial_kernel, dim3((unsigned)p.fin.slices, (unsigned)p.fin.N),
                        dim3(256), 3 * 256 * sizeof(float), stream, p);
  if (rc) return rc;
  return launch("flow_metrics_final", flow_metrics_final_kernel, dim3((unsigned)p.fin.N), dim3(256), 3 * 256 * sizeof(float), stream, p.fin);
}

}  // namespace mfn
