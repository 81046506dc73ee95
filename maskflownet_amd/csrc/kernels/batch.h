// batch.h -- one training batch cut out of a device-resident data set, one launch.
//
// Replaces what iterate_data / batch_samples of the reference's main.py:466-486 do to the N samples of one batch on the host, and
// the upload that follows: per sample a crop, the HWC -> CHW transpose, the optional reversal of the W axis with the sign of the
// label's first channel, and np.stack.  The bytes are the same:
//
//   out[n, c, y, x] = src_n[y0_n + y, x0_n + (flip_n ? Wc - 1 - x : x), c]
//
// for img1, img2 (3 channels, uint8), the label (2 channels, fp32 out, (u, v) as the readers give it) and the mask (1 channel,
// uint8).  A label stored as fp16 is widened exactly (subnormals, +-0, +-inf; a NaN keeps sign and payload bits << 13).  With flip
// the label's channel 0 has its SIGN BIT flipped (numpy's unary minus: +0.0 -> -0.0).  A slot without a mask, in a call with one,
// writes 255 (all valid, pipeline.py:94); a call without a mask touches no mask pointer.
//
// The slots are described by a device-resident table of BatchRow, 64 bytes each, built and checked on the host
// (mfn_batch_gather_build_rows) and uploaded by the caller: sizes, crop, flip and label type differ from slot to slot (a mixed
// Sintel / KITTI / HD1K batch has one data set per slot).  blockIdx.y is the slot, so the row is a wave-uniform read.
//
// READ CONTRACT.  Every source array starts at a 16-byte aligned address and is readable up to the next multiple of 16 bytes of
// its size.  The kernel reads aligned dwords (8 bytes for fp32 labels) that begin inside the array's own bytes, so nothing outside
// that extent is touched; the crop's byte offset 3 * (y * Ws + x) has any alignment and is handled by funnel shifts.
//
// Two instances, the same bytes:
//   QUAD  (Wc % 4 == 0: every shape the reference trains at)  a thread owns four consecutive x of one output row: 12 source bytes
//         per image (three or four aligned dwords, shifted into place) become one dword store per colour plane; eight label values
//         become two 16-byte stores (four dword stores each when the label tensor is not 16-byte aligned); four mask bytes one dword.
//         Consecutive lanes read consecutive 12-byte groups and write consecutive dwords.  Plane bases are dword aligned because
//         Hc * Wc % 4 == 0 and the tensors are.
//   BYTE  (any Wc)  a thread owns one output pixel; byte loads and byte stores.
// No reuse, no LDS, no atomics: per output pixel 6 + 8 (or 4) + 1 bytes read and 6 + 8 + 1 written.
#pragma once
#include "../mfn_rt.h"

namespace mfn {

enum { BATCH_THREADS = 256, BATCH_LABEL_F32 = 0, BATCH_LABEL_F16 = 1 };

// One slot of a batch; the table's layout is part of its tag.
struct BatchRow {
  const unsigned char *img1, *img2;   // (Hs, Ws, 3) uint8
  const void *flow;                   // (Hs, Ws, 2) fp32 or fp16
  const unsigned char *mask;          // (Hs, Ws, 1) uint8 or NULL
  int Hs, Ws, y0, x0;
  unsigned flip, label_type;
  unsigned pad_[2];
};
static_assert(sizeof(BatchRow) == 64, "the table's layout is part of its tag");

struct BatchGatherParams {
  const BatchRow *rows;
  unsigned char *img1, *img2;   // (N, 3, Hc, Wc)
  unsigned *label;              // (N, 2, Hc, Wc) fp32, moved as bit patterns
  unsigned char *mask;          // (N, 1, Hc, Wc) or NULL (a call without a mask)
  int N, Hc, Wc;
  unsigned items;               // per slot: Hc * Wc / 4 (QUAD) or Hc * Wc (BYTE)
  unsigned label16;             // the label tensor is 16-byte aligned
};

// The rows' pointers come out of a table in memory: cast to the global address space once, as kernels/optimizer.h does.
#if defined(MFN_EMU)
#define MFN_BATCH_GLOBAL
#else
#define MFN_BATCH_GLOBAL __attribute__((address_space(1)))
#endif
#if defined(MFN_EMU)
struct alignas(8) bg_u32x2 { unsigned x, y; };
struct alignas(16) bg_u32x4 { unsigned x, y, z, w; };
#else
typedef unsigned bg_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned bg_u32x4 __attribute__((ext_vector_type(4)));
#endif

__device__ __forceinline__ unsigned bg_ld8(const unsigned char *p) { return *(const MFN_BATCH_GLOBAL unsigned char *)p; }
__device__ __forceinline__ unsigned bg_ld16(const unsigned char *p) { return *(const MFN_BATCH_GLOBAL unsigned short *)p; }
__device__ __forceinline__ unsigned bg_ld32(const unsigned char *p) { return *(const MFN_BATCH_GLOBAL unsigned *)p; }
__device__ __forceinline__ bg_u32x2 bg_ld64(const unsigned char *p) { return *(const MFN_BATCH_GLOBAL bg_u32x2 *)p; }
// the dword that starts `sh` bits into lo (sh in {0, 8, 16, 24}); hi is not looked at when sh == 0
__device__ __forceinline__ unsigned bg_funnel(unsigned lo, unsigned hi, unsigned sh) {
  return (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
}
__device__ __forceinline__ unsigned bg_byte(const unsigned (&d)[3], int i) { return (d[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// fp16 bits -> the fp32 bits of the same value
__device__ __forceinline__ unsigned bg_half_bits(unsigned h) {
  const unsigned s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 31u) return s | 0x7f800000u | (m << 13);
  if (e != 0u) return s | ((e + 112u) << 23) | (m << 13);
  return s | (unsigned)mfn_f2i((float)m * 5.9604644775390625e-08f);   // m * 2^-24: exact, and normal in fp32 (0 for m == 0)
}

// 12 bytes at `p` (any alignment; p - (p & 3) .. is inside the array's extent): the three dwords they make
__device__ __forceinline__ void bg_load12(const unsigned char *p, unsigned (&d)[3]) {
  const unsigned sh = ((unsigned)(uintptr_t)p & 3u) * 8u;
  const unsigned char *q = p - (sh >> 3);
  const unsigned w0 = bg_ld32(q), w1 = bg_ld32(q + 4), w2 = bg_ld32(q + 8);
  const unsigned w3 = sh ? bg_ld32(q + 12) : 0u;   // a fourth dword only where the twelve bytes reach into it
  d[0] = bg_funnel(w0, w1, sh);
  d[1] = bg_funnel(w1, w2, sh);
  d[2] = bg_funnel(w2, w3, sh);
}
// four pixels of three interleaved channels -> one dword per plane, output x ascending in the bytes
__device__ __forceinline__ void bg_image_quad(const unsigned char *src, unsigned char *dst, size_t plane, bool flip) {
  unsigned d[3];
  bg_load12(src, d);
  MFN_UNROLL
  for (int c = 0; c < 3; ++c) {
    const unsigned b0 = bg_byte(d, c), b1 = bg_byte(d, 3 + c), b2 = bg_byte(d, 6 + c), b3 = bg_byte(d, 9 + c);
    const unsigned w = flip ? (b3 | (b2 << 8) | (b1 << 16) | (b0 << 24)) : (b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
    *reinterpret_cast<unsigned *>(dst + (size_t)c * plane) = w;
  }
}
__device__ __forceinline__ void bg_store4(unsigned *dst, unsigned a, unsigned b, unsigned c, unsigned d, bool wide) {
  if (wide) {
    *reinterpret_cast<bg_u32x4 *>(dst) = bg_u32x4{a, b, c, d};
  } else {
    dst[0] = a; dst[1] = b; dst[2] = c; dst[3] = d;
  }
}

template <bool QUAD>
__global__ __launch_bounds__(BATCH_THREADS) void batch_gather_kernel(BatchGatherParams p) {
  const unsigned n = blockIdx.y;
  const unsigned item = blockIdx.x * BATCH_THREADS + threadIdx.x;
  if (n >= (unsigned)p.N || item >= p.items) return;
  const BatchRow r = p.rows[n];                 // wave-uniform: indexed by the block
  const bool flip = r.flip != 0u;
  const size_t plane = (size_t)p.Hc * p.Wc;
  if (QUAD) {
    const unsigned wq = (unsigned)p.Wc >> 2;
    const unsigned y = item / wq, x = (item - y * wq) * 4u;
    // the four source pixels are consecutive either way: from xs upwards, output x ascending (plain) or descending (flip)
    const size_t spix = (size_t)(r.y0 + (int)y) * r.Ws + (size_t)(r.x0 + (flip ? p.Wc - 4 - (int)x : (int)x));
    const size_t opix = (size_t)y * p.Wc + x;
    bg_image_quad(r.img1 + 3 * spix, p.img1 + (size_t)n * 3 * plane + opix, plane, flip);
    bg_image_quad(r.img2 + 3 * spix, p.img2 + (size_t)n * 3 * plane + opix, plane, flip);
    unsigned u[4], v[4];
    if (r.label_type == BATCH_LABEL_F16) {
      const unsigned char *f = (const unsigned char *)r.flow + 4 * spix;    // dword aligned: one (u, v) pair per dword
      MFN_UNROLL
      for (int k = 0; k < 4; ++k) {
        const unsigned w = bg_ld32(f + 4 * k);
        u[k] = bg_half_bits(w & 0xffffu);
        v[k] = bg_half_bits(w >> 16);
      }
    } else {
      const unsigned char *f = (const unsigned char *)r.flow + 8 * spix;    // 8-byte aligned
      MFN_UNROLL
      for (int k = 0; k < 4; ++k) {
        const bg_u32x2 w = bg_ld64(f + 8 * k);
        u[k] = w.x;
        v[k] = w.y;
      }
    }
    unsigned *lab = p.label + (size_t)n * 2 * plane + opix;
    if (flip) {
      bg_store4(lab, u[3] ^ 0x80000000u, u[2] ^ 0x80000000u, u[1] ^ 0x80000000u, u[0] ^ 0x80000000u, p.label16 != 0u);
      bg_store4(lab + plane, v[3], v[2], v[1], v[0], p.label16 != 0u);
    } else {
      bg_store4(lab, u[0], u[1], u[2], u[3], p.label16 != 0u);
      bg_store4(lab + plane, v[0], v[1], v[2], v[3], p.label16 != 0u);
    }
    if (p.mask) {
      unsigned m = 0xffffffffu;
      if (r.mask) {
        const unsigned char *s = r.mask + spix;
        const unsigned sh = ((unsigned)(uintptr_t)s & 3u) * 8u;
        const unsigned w0 = bg_ld32(s - (sh >> 3)), w1 = sh ? bg_ld32(s - (sh >> 3) + 4) : 0u;
        m = bg_funnel(w0, w1, sh);
        if (flip) m = (m >> 24) | ((m >> 8) & 0xff00u) | ((m << 8) & 0xff0000u) | (m << 24);
      }
      *reinterpret_cast<unsigned *>(p.mask + (size_t)n * plane + opix) = m;
    }
  } else {
    const unsigned y = item / (unsigned)p.Wc, x = item - y * (unsigned)p.Wc;
    const size_t spix = (size_t)(r.y0 + (int)y) * r.Ws + (size_t)(r.x0 + (flip ? p.Wc - 1 - (int)x : (int)x));
    const size_t opix = (size_t)y * p.Wc + x;
    unsigned char *o1 = p.img1 + (size_t)n * 3 * plane + opix, *o2 = p.img2 + (size_t)n * 3 * plane + opix;
    MFN_UNROLL
    for (int c = 0; c < 3; ++c) {
      o1[(size_t)c * plane] = (unsigned char)bg_ld8(r.img1 + 3 * spix + c);
      o2[(size_t)c * plane] = (unsigned char)bg_ld8(r.img2 + 3 * spix + c);
    }
    unsigned u, v;
    if (r.label_type == BATCH_LABEL_F16) {
      const unsigned char *f = (const unsigned char *)r.flow + 4 * spix;
      u = bg_half_bits(bg_ld16(f));
      v = bg_half_bits(bg_ld16(f + 2));
    } else {
      const unsigned char *f = (const unsigned char *)r.flow + 8 * spix;
      u = bg_ld32(f);
      v = bg_ld32(f + 4);
    }
    unsigned *lab = p.label + (size_t)n * 2 * plane + opix;
    lab[0] = flip ? u ^ 0x80000000u : u;
    lab[plane] = v;
    if (p.mask) p.mask[(size_t)n * plane + opix] = r.mask ? (unsigned char)bg_ld8(r.mask + spix) : (unsigned char)255;
  }
}

// ---- the table: host side --------------------------------------------------------------------------------------------------
inline size_t batch_rows_bytes(int N) { return N > 0 ? (size_t)N * sizeof(BatchRow) : 0; }
// What a table has to carry to be used with (N, Hc, Wc): the layout's version and the crop it was checked against.
inline unsigned long long batch_rows_tag(int N, int Hc, int Wc) {
  unsigned long long t = (0xBA7C0001ull << 32) ^ ((unsigned long long)sizeof(BatchRow) << 24);
  t ^= ((unsigned long long)(unsigned)N * 0x9E3779B97F4A7C15ull) >> 7;
  t ^= ((unsigned long long)(unsigned)Hc * 0xC2B2AE3D27D4EB4Full) >> 11;
  t ^= ((unsigned long long)(unsigned)Wc * 0x165667B19E3779F9ull) >> 13;
  return t;
}

inline int batch_gather_launch(BatchGatherParams p, hipStream_t stream) {
  const bool quad = (p.Wc & 3) == 0;
  const size_t plane = (size_t)p.Hc * p.Wc;
  p.items = (unsigned)(quad ? plane / 4 : plane);
  const dim3 grid((p.items + BATCH_THREADS - 1) / BATCH_THREADS, (unsigned)p.N);
  if (quad) return launch("batch_gather_kernel", batch_gather_kernel<true>, grid, dim3(BATCH_THREADS), 0, stream, p);
  return launch("batch_gather_kernel", batch_gather_kernel<false>, grid, dim3(BATCH_THREADS), 0, stream, p);
}

}  // namespace mfn
