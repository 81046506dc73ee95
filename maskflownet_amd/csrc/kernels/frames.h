// frames.h -- prediction on uint8 frame sequences, and the colour picture of a flow.
//
// Replaces the arithmetic of the reference's predict_new_data.py around `pipe.predict(prev_frames, new_frames)` (:152-158) for
// frames that are already on the device as bytes:
//   pair_mean_u8         PipelineFlownet.centralize's joint mean (pipeline.py:86) of frames / 255 (pipeline.py:208), from the bytes
//   preprocess_pair_u8   `/ 255`, HWC -> CHW, - rgb_mean, BilinearResize2D of both images (pipeline.py:208, :120-130) in one launch
//   flow_color           flow_vis.flow_to_color(flow, convert_to_bgr=...) (predict_new_data.py:155, :158)
//
// Frames layout.  frames: (F, H, W, 3) uint8, HWC.  A batch of N pairs is two first indices: pair n is (frames[a0+n], frames[b0+n]);
// a video passes b0 = a0 + 1, two stacked lists b0 = a0 + N.  No index table.  A frame's first byte is 4-byte aligned only when
// a0*H*W*3 is: every wider-than-byte load below is taken where the ADDRESS is a multiple of 4 and the bytes lie inside one frame,
// else the same bytes are read one by one.
//
// pair_mean_u8 is EXACT: the 2*H*W bytes of (n, c) are summed as integers (32-bit partial sums per slice of 4096 pixels, at most
// 4096 * 255; a 64-bit final sum), through a caller-supplied workspace in a fixed order, no atomics, two stages like
// pair_mean_*_kernel, then mean = (float)((double)sum / (255.0 * 2*H*W)) with the denominator formed in double.  The result is
// order-independent and bit-identical to np.float32(np.float64(sum) / np.float64(255 * 2 * H * W)).  It is NOT the bits of
// mfn_pair_mean on byte / 255 floats: that one is an fp32 sum of rounded quotients (within its 64 * 2^-24 bound of this one).
//
// preprocess_pair_u8 is resize_kernel / resize_copy_kernel of predict.h with the tap (float)byte / 255.f -- one IEEE division, the
// value predict._chw01 makes on the host -- and everything after it the same expressions in the same order (fp contraction off):
// bit-identical to mfn_preprocess_pair on those floats with the same mean.  One thread makes 4 adjacent outputs of all three
// channels: a tap's three bytes are neighbours in memory.
//
// [flow_vis-ext, unpinned] flow_color restates flow_vis.flow_to_color (without clip_flow) from memory; flow_vis is not part of the
// reference tree.  Compare against flow_vis itself before relying on the last bit of a colour.  In fp32, per pixel, with the flow in
// network order (channel 0 = dy = v, channel 1 = dx = u):
//   wheel: 55 rows of (R, G, B), segments RY=15, YG=6, GC=4, CB=11, BM=13, MR=6 in this order:
//     RY (255, floor(255 i/15), 0)       YG (255 - floor(255 i/6), 255, 0)    GC (0, 255, floor(255 i/4))
//     CB (0, 255 - floor(255 i/11), 255) BM (floor(255 i/13), 0, 255)         MR (255, 0, 255 - floor(255 i/6))
//   un = u / (rad_max + 1e-5);  vn = v / (rad_max + 1e-5);  rad = sqrt(un^2 + vn^2)
//   a = atan2(-vn, -un) / pi;  fk = (a + 1) / 2 * 54;  k0 = floor(fk);  k1 = k0 + 1, 55 -> 0;  f = fk - k0
//   col = (1 - f) * wheel[k0]/255 + f * wheel[k1]/255;   col = rad <= 1 ? 1 - rad * (1 - col) : col * 0.75
//   byte = floor(255 * col), channels reversed with bgr;  a pixel whose flow is not finite is written (0, 0, 0)
// rad_max: the argument when it is >= 0 (one scale for a whole video), else the image's own maximum of sqrtf(u*u + v*v) over its
// finite values (0 for none) -- contraction off, the bits of numpy fp32 --, found in the fixed-order two-stage pattern of
// flow_metrics over slices of 4096 pixels.  A maximum does not depend on the order; the pattern keeps the workspace contract.
//
// All kernels are HBM-bound, one pass: pair_mean_u8 6*N*H*W bytes, preprocess_pair_u8 6*N*H*W + 24*N*Hout*Wout,
// flow_color 8*N*H*W (twice with its own maximum) + 3*N*H*W.
#pragma once
#include "../mfn_rt.h"
#include "predict.h"

namespace mfn {

// red[0] = the block's 256 values joined in the order of an 8-level tree
template <class T, class Op>
__device__ __forceinline__ void frames_block_tree(T *red, Op op) {
  __syncthreads();
  for (int st = 128; st >= 1; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + st]);
    __syncthreads();
  }
}

// ---- the joint mean of a pair of byte frames, exact ------------------------------------------------------------------------------
struct PairMeanU8Params {
  const unsigned char *frames;
  unsigned *partial;   // (N, slices, 3)
  float *mean;         // (N, 3)
  size_t plane;        // H * W
  double denom;        // 255.0 * 2 * H * W
  int a0, b0, N, slices;
};
// the pixel sequence of pair n: the H*W pixels of frame a0+n followed by those of frame b0+n; a thread sums a run of 16 of them
__global__ __launch_bounds__(256) void pair_mean_u8_partial_kernel(PairMeanU8Params p) {
  MFN_DYN_SHARED(unsigned, red);   // [3][256]
  const int sl = blockIdx.x, n = blockIdx.y;
  const unsigned char *fa = p.frames + (size_t)(p.a0 + n) * p.plane * 3, *fb = p.frames + (size_t)(p.b0 + n) * p.plane * 3;
  const size_t total = 2 * p.plane;
  const size_t q0 = (size_t)sl * PRED_SLICE + (size_t)threadIdx.x * PRED_RUN;
  unsigned s[3] = {0u, 0u, 0u};
  if (q0 < total) {
    const bool first = q0 < p.plane;
    const unsigned char *src = first ? fa + 3 * q0 : fb + 3 * (q0 - p.plane);
    const size_t end = first ? p.plane : total;   // where the run's frame ends
    if (q0 + PRED_RUN <= end && ((uintptr_t)src & 3) == 0) {   // 48 bytes inside one frame from an aligned address: 12 words
      const unsigned *w = reinterpret_cast<const unsigned *>(src);
      MFN_UNROLL
      for (int k = 0; k < 3 * PRED_RUN / 4; ++k) {
        const unsigned v = w[k];
        s[(4 * k) % 3] += v & 255u;
        s[(4 * k + 1) % 3] += (v >> 8) & 255u;
        s[(4 * k + 2) % 3] += (v >> 16) & 255u;
        s[(4 * k + 3) % 3] += v >> 24;
      }
    } else {
      for (int k = 0; k < PRED_RUN; ++k) {
        const size_t q = q0 + k;
        if (q < total) {
          const unsigned char *px = q < p.plane ? fa + 3 * q : fb + 3 * (q - p.plane);
          s[0] += px[0]; s[1] += px[1]; s[2] += px[2];
        }
      }
    }
  }
  for (int c = 0; c < 3; ++c) {
    red[c * 256 + threadIdx.x] = s[c];
    frames_block_tree(red + c * 256, [](unsigned a, unsigned b) { return a + b; });
  }
  if (threadIdx.x < 3) p.partial[((size_t)n * p.slices + sl) * 3 + threadIdx.x] = red[threadIdx.x * 256];
}
__global__ __launch_bounds__(256) void pair_mean_u8_final_kernel(PairMeanU8Params p) {
  MFN_DYN_SHARED(unsigned long long, red);   // [3][256]
  const int n = blockIdx.x;
  const unsigned *part = p.partial + (size_t)n * p.slices * 3;
  unsigned long long s[3] = {0ull, 0ull, 0ull};
  for (int q = (int)threadIdx.x; q < p.slices; q += 256) { s[0] += part[q * 3]; s[1] += part[q * 3 + 1]; s[2] += part[q * 3 + 2]; }
  for (int c = 0; c < 3; ++c) {
    red[c * 256 + threadIdx.x] = s[c];
    frames_block_tree(red + c * 256, [](unsigned long long a, unsigned long long b) { return a + b; });
  }
  if (threadIdx.x < 3) p.mean[(size_t)n * 3 + threadIdx.x] = (float)((double)red[threadIdx.x * 256] / p.denom);
}
inline int pair_mean_u8_launch(PairMeanU8Params p, hipStream_t stream) {
  if (p.N == 0) return 0;
  const int rc = launch("pair_mean_u8_partial", pair_mean_u8_partial_kernel, dim3((unsigned)p.slices, (unsigned)p.N), dim3(256),
                        3 * 256 * sizeof(unsigned), stream, p);
  if (rc) return rc;
  return launch("pair_mean_u8_final", pair_mean_u8_final_kernel, dim3((unsigned)p.N), dim3(256), 3 * 256 * sizeof(unsigned long long),
                stream, p);
}

// ---- / 255, HWC -> CHW, - mean, align-corners bilinear resize of both images [MXNet-ext, unpinned] ---------------------------------
struct FramesPreParams {
  const unsigned char *frames;
  const float *mean;   // (N, 3) or NULL: no subtraction
  float *out;          // (2N, 3, Hout, Wout): image 1 of pair n in row n, image 2 in row N + n
  int a0, b0, N;
  int H, W, Hout, Wout;
  float ry, rx;        // as ResizeParams
  int st_policy;
};
__device__ __forceinline__ const unsigned char *frames_image(const FramesPreParams &p, int img, size_t frame_bytes) {
  return p.frames + (size_t)(img < p.N ? p.a0 + img : p.b0 + (img - p.N)) * frame_bytes;
}

template <int VEC>
__global__ __launch_bounds__(256) void frames_resize_kernel(FramesPreParams p) {
#pragma clang fp contract(off)
  const int wv = (p.Wout + VEC - 1) / VEC;
  const size_t total = (size_t)2 * p.N * p.Hout * wv;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int xv = (int)(idx % wv);
  const int oy = (int)((idx / wv) % p.Hout);
  const int img = (int)(idx / ((size_t)wv * p.Hout));
  const int n = img < p.N ? img : img - p.N;
  const unsigned char *src = frames_image(p, img, (size_t)p.H * p.W * 3);
  float m[3] = {0.f, 0.f, 0.f};
  if (p.mean) { m[0] = p.mean[n * 3]; m[1] = p.mean[n * 3 + 1]; m[2] = p.mean[n * 3 + 2]; }
  const float py = p.ry * (float)oy;
  const int i0 = min((int)py, p.H - 1);
  const int ip = i0 < p.H - 1 ? 1 : 0;
  const float h1 = py - (float)i0, h0 = 1.f - h1;
  const unsigned char *r0 = src + (size_t)i0 * p.W * 3;
  const unsigned char *r1 = r0 + (size_t)ip * p.W * 3;
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
__global__ __launch_bounds__(256) void frames_unpack_kernel(FramesPreParams p) {
#pragma clang fp contract(off)
  const size_t plane = (size_t)p.H * p.W;
  const size_t pv = plane / VEC;                  // VEC == 4 only with plane % 4 == 0
  const size_t total = (size_t)2 * p.N * pv;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int img = (int)(idx / pv);
  const size_t q = (idx - (size_t)img * pv) * VEC;
  const int n = img < p.N ? img : img - p.N;
  const unsigned char *src = frames_image(p, img, plane * 3) + q * 3;
  float m[3] = {0.f, 0.f, 0.f};
  if (p.mean) { m[0] = p.mean[n * 3]; m[1] = p.mean[n * 3 + 1]; m[2] = p.mean[n * 3 + 2]; }
  unsigned char by[3 * VEC];
  if (VEC == 4 && ((uintptr_t)src & 3) == 0) {    // 12 bytes inside the frame from an aligned address: 3 words
    const unsigned *w = reinterpret_cast<const unsigned *>(src);
    MFN_UNROLL
    for (int k = 0; k < 3 * VEC / 4; ++k) {
      const unsigned v = w[k];
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

// the store rules of resize_launch: 16-byte stores when the row length (the plane, for the unpack) is a multiple of 4 and out is aligned
inline int frames_pre_launch(FramesPreParams p, hipStream_t stream) {
  if ((size_t)p.N * p.Hout * p.Wout == 0) return 0;
  const bool al_out = ((uintptr_t)p.out) % 16 == 0;
  if (p.H == p.Hout && p.W == p.Wout) {
    const size_t plane = (size_t)p.H * p.W;
    const bool vec4 = plane % 4 == 0 && al_out;
    const size_t total = (size_t)2 * p.N * (vec4 ? plane / 4 : plane);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec4) return launch("frames_unpack_v4", frames_unpack_kernel<4>, grid, dim3(256), 0, stream, p);
    return launch("frames_unpack_v1", frames_unpack_kernel<1>, grid, dim3(256), 0, stream, p);
  }
  const bool vec4 = p.Wout % 4 == 0 && al_out;
  const size_t total = (size_t)2 * p.N * p.Hout * (vec4 ? p.Wout / 4 : p.Wout);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (vec4) return launch("frames_resize_v4", frames_resize_kernel<4>, grid, dim3(256), 0, stream, p);
  return launch("frames_resize_v1", frames_resize_kernel<1>, grid, dim3(256), 0, stream, p);
}

// ---- the Middlebury colour wheel picture of a flow [flow_vis-ext, unpinned] --------------------------------------------------------
enum { FLOW_WHEEL = 55 };
struct FlowColorParams {
  const float *flow;    // (N, 2, H, W), channel 0 = v, channel 1 = u
  unsigned char *rgb;   // (N, H, W, 3)
  float *partial;       // (N, slices): the slices' maxima
  float *radmax;        // (N): the images' maxima; both unused with rad_max >= 0
  float rad_max;        // >= 0: the scale of every image; < 0: each image's own maximum
  int N, H, W, slices, bgr;
};
__global__ __launch_bounds__(256) void flow_radmax_partial_kernel(FlowColorParams p) {
#pragma clang fp contract(off)
  MFN_DYN_SHARED(float, red);
  const int sl = blockIdx.x, n = blockIdx.y;
  const size_t plane = (size_t)p.H * p.W, base = (size_t)sl * PRED_SLICE;
  const float *f = p.flow + (size_t)n * 2 * plane;
  float m = 0.f;
  MFN_UNROLL
  for (int k = 0; k < PRED_RUN; ++k) {
    const size_t q = base + (size_t)k * 256 + threadIdx.x;
    if (q < plane) {
      const float v = f[q], u = f[plane + q];
      const float r = sqrtf(u * u + v * v);
      if (r <= 3.4028234663852886e38f && r > m) m = r;   // a NaN or infinite radius is ignored
    }
  }
  red[threadIdx.x] = m;
  frames_block_tree(red, [](float a, float b) { return b > a ? b : a; });
  if (threadIdx.x == 0) p.partial[(size_t)n * p.slices + sl] = red[0];
}
__global__ __launch_bounds__(256) void flow_radmax_final_kernel(FlowColorParams p) {
  MFN_DYN_SHARED(float, red);
  const int n = blockIdx.x;
  const float *part = p.partial + (size_t)n * p.slices;
  float m = 0.f;
  for (int q = (int)threadIdx.x; q < p.slices; q += 256) m = part[q] > m ? part[q] : m;
  red[threadIdx.x] = m;
  frames_block_tree(red, [](float a, float b) { return b > a ? b : a; });
  if (threadIdx.x == 0) p.radmax[n] = red[0];
}

// row k of the wheel, channel c
__device__ __forceinline__ int flow_wheel_entry(int k, int c) {
  int r, g, b;
  if (k < 15) { r = 255; g = 255 * k / 15; b = 0; }
  else if (k < 21) { r = 255 - 255 * (k - 15) / 6; g = 255; b = 0; }
  else if (k < 25) { r = 0; g = 255; b = 255 * (k - 21) / 4; }
  else if (k < 36) { r = 0; g = 255 - 255 * (k - 25) / 11; b = 255; }
  else if (k < 49) { r = 255 * (k - 36) / 13; g = 0; b = 255; }
  else { r = 255; g = 0; b = 255 - 255 * (k - 49) / 6; }
  return c == 0 ? r : c == 1 ? g : b;
}

// one thread: 4 adjacent pixels of a row, 12 bytes -- three word stores where the row has all four and the address is a multiple of 4
__global__ __launch_bounds__(256) void flow_color_kernel(FlowColorParams p) {
#pragma clang fp contract(off)
  MFN_DYN_SHARED(float, wheel);   // [55][3], each entry / 255
  if (threadIdx.x < 3 * FLOW_WHEEL) wheel[threadIdx.x] = (float)flow_wheel_entry((int)threadIdx.x / 3, (int)threadIdx.x % 3) / 255.f;
  __syncthreads();
  const int wq = (p.W + 3) / 4;
  const size_t total = (size_t)p.N * p.H * wq;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int xq = (int)(idx % wq);
  const int y = (int)((idx / wq) % p.H);
  const int n = (int)(idx / ((size_t)wq * p.H));
  const size_t plane = (size_t)p.H * p.W;
  const int x0 = xq * 4, cnt = min(4, p.W - x0);
  const float *pv = p.flow + (size_t)n * 2 * plane + (size_t)y * p.W + x0, *pu = pv + plane;
  float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
  if (cnt == 4 && (((uintptr_t)pv | (uintptr_t)pu) & 15) == 0) {
    const float4 a = *reinterpret_cast<const float4 *>(pv), b = *reinterpret_cast<const float4 *>(pu);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    u[0] = b.x; u[1] = b.y; u[2] = b.z; u[3] = b.w;
  } else {
    MFN_UNROLL
    for (int k = 0; k < 4; ++k)
      if (k < cnt) { v[k] = pv[k]; u[k] = pu[k]; }
  }
  const float den = (p.rad_max >= 0.f ? p.rad_max : p.radmax[n]) + 1e-5f;
  const float big = 3.4028234663852886e38f;
  unsigned char by[12];
  MFN_UNROLL
  for (int k = 0; k < 4; ++k) {
    const bool finite = fabsf(u[k]) <= big && fabsf(v[k]) <= big;
    const float un = (finite ? u[k] : 0.f) / den, vn = (finite ? v[k] : 0.f) / den;
    const float rad = sqrtf(un * un + vn * vn);
    const float a = atan2f(-vn, -un) / 3.14159265358979323846f;
    const float fk = (a + 1.f) / 2.f * (float)(FLOW_WHEEL - 1);
    const float fl = floorf(fk);
    const int k0 = min(max((int)fl, 0), FLOW_WHEEL - 1);   // fk lies in [0, 54]: the clamp only guards the LDS index
    const int k1 = k0 + 1 == FLOW_WHEEL ? 0 : k0 + 1;
    const float f = fk - fl;
    unsigned char q[3];
    MFN_UNROLL
    for (int c = 0; c < 3; ++c) {
      float col = (1.f - f) * wheel[k0 * 3 + c] + f * wheel[k1 * 3 + c];
      col = rad <= 1.f ? 1.f - rad * (1.f - col) : col * 0.75f;
      const float x = floorf(255.f * col);
      q[c] = finite ? (unsigned char)(int)fminf(fmaxf(x, 0.f), 255.f) : (unsigned char)0;
    }
    by[3 * k] = p.bgr ? q[2] : q[0];
    by[3 * k + 1] = q[1];
    by[3 * k + 2] = p.bgr ? q[0] : q[2];
  }
  unsigned char *dst = p.rgb + (((size_t)n * p.H + y) * p.W + x0) * 3;
  if (cnt == 4 && ((uintptr_t)dst & 3) == 0) {
    unsigned *w = reinterpret_cast<unsigned *>(dst);
    MFN_UNROLL
    for (int k = 0; k < 3; ++k)
      w[k] = (unsigned)by[4 * k] | ((unsigned)by[4 * k + 1] << 8) | ((unsigned)by[4 * k + 2] << 16) | ((unsigned)by[4 * k + 3] << 24);
  } else {
    MFN_UNROLL
    for (int k = 0; k < 12; ++k)
      if (k < 3 * cnt) dst[k] = by[k];
  }
}
inline int flow_color_launch(FlowColorParams p, hipStream_t stream) {
  if (p.N == 0) return 0;
  if (!(p.rad_max >= 0.f)) {
    int rc = launch("flow_radmax_partial", flow_radmax_partial_kernel, dim3((unsigned)p.slices, (unsigned)p.N), dim3(256),
                    256 * sizeof(float), stream, p);
    if (rc) return rc;
    rc = launch("flow_radmax_final", flow_radmax_final_kernel, dim3((unsigned)p.N), dim3(256), 256 * sizeof(float), stream, p);
    if (rc) return rc;
  }
  const size_t total = (size_t)p.N * p.H * ((p.W + 3) / 4);
  return launch("flow_color", flow_color_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 3 * FLOW_WHEEL * sizeof(float) + 12,
                stream, p);
}

}  // namespace mfn
