// ingest.h -- raw decoded KITTI / HD1K / Sintel arrays turned into stored samples inside the data set's arena.
//
// Replaces what the reference's readers do to every sample at load time on the host, with cv2 (reader/kitti.py:57-74,
// reader/hd1k.py:51-78): crop, (HD1K) min/max contrast stretch of both images, cv2.resize of the images, bilinear resize of flow and
// validity, re-scaling of the flow, division of the flow by the resized validity (the sparse-flow normalisation), quantisation of the
// mask -- and, here, the narrowing of the flow to fp16 where the data set stores it so.  No intermediate tensor.
//
// Every kernel reads a WINDOW of a raw HWC array: base pointer, row pitch in elements, origin (y0, x0) and size (h, w) in pixels.
// READ CONTRACT (as kernels/batch.h): the base is 16-byte aligned and readable up to the next multiple of 16 bytes of the array's size.
// The image and flow kernels read single elements inside the window; the min/max kernel reads aligned dwords that begin inside the
// array's own bytes (the window's origin has any alignment: bytes of a dword outside the window's row are masked out).  Destinations
// are dense, 16-byte aligned sample parts.  Plain C++ and vector stores; the only atomics are the vector atomicMin / atomicMax of the
// min/max kernel.
//
// RESAMPLING is OpenCV's INTER_LINEAR (half-pixel centres, edge replicate, no antialiasing), restated from its generic, non-IPP path.
// Positions and coefficients come from two host-built tables (ingest_build_tables below), one IngestTap per destination column and one
// per destination row; the kernels apply the coefficients and never derive them.  For destination index d of `dst` over a source of
// `src`:
//     scale = double(src) / double(dst);  f = float((d + 0.5) * scale - 0.5)   (product and difference in double, one rounding)
//     s = floor(f);  f = float(f - s);   s < 0: s = 0, f = 0;   s >= src - 1: s = src - 1, f = 0;   s1 = min(s + 1, src - 1)
//     c0 = 1.0f - f, c1 = f;   i0 = rint(c0 * 2048), i1 = rint(c1 * 2048) (half to even)
//
// ingest_image_kernel   uint8 HWC-3 window -> uint8 HWC-3 (H', W'): optional channel reversal (cv2.imread's BGR), optional 256-entry
//     lookup (HD1K's stretch), then OpenCV's fixed-point bilinear:  h = S[s] * i0 + S[s1] * i1 (int32) per source row,
//     v = ((j0 * (h_s >> 4)) >> 16) + ((j1 * (h_s1 >> 4)) >> 16),  out = saturate_u8((v + 2) >> 2).  At equal sizes: a copy.
//     The lookup is built per block in LDS from the two words the min/max kernel left, in double as numpy does (hd1k.py:56):
//     lut[v] = uint8((v - mn) * (255.0 / (mx - mn))), truncating.  THE ONE DEPARTURE: a constant pair (mx == mn) makes the reference
//     divide by zero (NaN, an undefined cast); here it maps to 0.
// ingest_minmax_kernel  min and max over both image windows, all channels (hd1k.py:55), into two device words.
// ingest_flow_occ_kernel  uint16 HWC-3 window in FILE order (R = u, G = v, B = valid) -> flow (H', W', 2) in (u, v) order, fp32 or
//     fp16, and mask (H', W', 1) uint8, one pass.  Every fp32 operation rounded separately (fp contraction off).  Per source pixel
//         u = (float(R) - 32768) / 64, v likewise, occ = float(B & 0xFF);   premultiply (hd1k.py:60): u *= occ, v *= occ
//     all three resized with the float coefficients, horizontal first (S[s] * c0 + S[s1] * c1: mul, mul, add), then vertical; then
//         u_r *= sx, v_r *= sy      with sx = float(W' - 1) / float(W - 1), sy = float(H' - 1) / float(H - 1) from the host (kitti.py:68-69)
//         den = occ_r + (occ_r == 0 ? 1 : 0);  u_o = u_r / den, v_o = v_r / den                                        (kitti.py:71)
//         mask = uint8(occ_r * 255), truncating; a value above 255 (a valid byte above 1) keeps its low 8 bits         (kitti.py:72)
//     fp16 storage: IEEE round to nearest even of u_o, v_o, overflow to inf (numpy's astype).  At equal sizes this is the reference's
//     resize=None branch: scale 1, division by 1, occ * 255 (a premultiplied -0.0 may come out as +0.0).
//
// Shape: a thread owns 16 consecutive bytes of the dense destination image (one aligned 16-byte store; the tail of the image byte by
// byte), or four consecutive pixels of flow and mask (16-byte flow stores, one dword of mask; the tail pixel by pixel); consecutive
// lanes own consecutive pieces, so a wave's stores are contiguous.  The two or four source rows a piece needs are read straight from
// global memory (no LDS staging: not measured to pay).
#pragma once
#include "../mfn_rt.h"

namespace mfn {

enum { INGEST_THREADS = 256, INGEST_FLOW_F32 = 0, INGEST_FLOW_F16 = 1, INGEST_MINMAX_BLOCKS = 512 };

// One destination index of one axis; the table's layout is part of its tag.
struct IngestTap {
  int s, s1;        // the two source indices
  float c0, c1;     // float coefficients
  int i0, i1;       // fixed-point coefficients (int16 range)
  int pad_[2];
};
static_assert(sizeof(IngestTap) == 32, "the table's layout is part of its tag");

struct IngestImageParams {
  const unsigned char *src;       // window origin: base + y0 * pitch + 3 * x0
  long long pitch;                // bytes per source row
  const IngestTap *cols, *rows;   // Wd and Hd entries
  const unsigned *minmax;         // {min, max} or NULL: no lookup
  unsigned char *dst;             // (Hd, Wd, 3), 16-byte aligned
  int Hd, Wd;
  unsigned bgr;
  unsigned long long nbytes;      // Hd * Wd * 3
};

struct IngestMinmaxParams {
  const unsigned char *img1, *img2;   // array bases (16-byte aligned)
  long long pitch;
  int y0, x0, h, w;
  unsigned row_dwords;                // an upper bound of the aligned dwords one window row touches
  unsigned long long items;           // 2 * h * row_dwords
  unsigned *out;                      // {min, max}
};

struct IngestFlowParams {
  const unsigned short *src;      // window origin: base + y0 * pitch + 3 * x0
  long long pitch;                // elements per source row
  const IngestTap *cols, *rows;
  void *flow;                     // (Hd, Wd, 2) fp32 or fp16, 16-byte aligned
  unsigned char *mask;            // (Hd, Wd, 1), 16-byte aligned
  int Hd, Wd;
  unsigned premultiply, flow_type;
  float sx, sy;
  unsigned long long npix;        // Hd * Wd
};

#if defined(MFN_EMU)
struct alignas(16) ig_u32x4 { unsigned x, y, z, w; };
static inline void ig_atomic_min(unsigned *p, unsigned v) {
  std::atomic_ref<unsigned> a(*p);
  for (unsigned cur = a.load(); v < cur && !a.compare_exchange_weak(cur, v);) {}
}
static inline void ig_atomic_max(unsigned *p, unsigned v) {
  std::atomic_ref<unsigned> a(*p);
  for (unsigned cur = a.load(); v > cur && !a.compare_exchange_weak(cur, v);) {}
}
#else
typedef unsigned ig_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void ig_atomic_min(unsigned *p, unsigned v) { atomicMin(p, v); }
__device__ __forceinline__ void ig_atomic_max(unsigned *p, unsigned v) { atomicMax(p, v); }
#endif

// fp32 -> the fp16 bits of the nearest value, ties to even, overflow to inf, subnormal results exact (integer arithmetic: the same
// bits on every build)
__device__ __forceinline__ unsigned ig_half_bits(float f) {
  const unsigned x = (unsigned)mfn_f2i(f), sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a >= 0x7f800000u) return sign | 0x7c00u | (a > 0x7f800000u ? 0x200u | ((a >> 13) & 0x3ffu) : 0u);   // inf, NaN (quiet, payload kept)
  if (a >= 0x477ff000u) return sign | 0x7c00u;                                                             // >= 65520: rounds to inf
  if (a >= 0x38800000u) {                                                                                  // normal in fp16
    const unsigned m = a - 0x38000000u;                       // exponent rebased (127 -> 15)
    return sign | ((m + 0xfffu + ((m >> 13) & 1u)) >> 13);
  }
  if (a < 0x33000000u) return sign;                                                                        // < 2^-25: 0
  const unsigned e = a >> 23, m = (a & 0x7fffffu) | 0x800000u, sh = 126u - e;                              // value = m * 2^(e - 150); fp16 subnormal unit 2^-24
  const unsigned q = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
}

// ---- the image -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(INGEST_THREADS) void ingest_image_kernel(IngestImageParams p) {
  MFN_DYN_SHARED(unsigned char, lut);   // 256 entries
  const bool use_lut = p.minmax != nullptr;
  if (use_lut) {   // wave-uniform
    const unsigned mn = p.minmax[0], mx = p.minmax[1];
    const unsigned v = threadIdx.x;
    unsigned o = 0u;
    if (mx > mn && v >= mn && v <= mx) o = (unsigned)(int)((double)(v - mn) * (255.0 / (double)(mx - mn))) & 0xffu;
    lut[v] = (unsigned char)o;
    __syncthreads();
  }
  const unsigned long long b0 = ((unsigned long long)blockIdx.x * INGEST_THREADS + threadIdx.x) * 16ull;
  if (b0 >= p.nbytes) return;
  const unsigned rowb = 3u * (unsigned)p.Wd;
  unsigned y = (unsigned)(b0 / rowb), xb = (unsigned)(b0 - (unsigned long long)y * rowb);
  unsigned x = xb / 3u, c = xb - 3u * x;
  IngestTap ty = p.rows[y], tx = p.cols[x];
  const unsigned n = p.nbytes - b0 < 16ull ? (unsigned)(p.nbytes - b0) : 16u;
  unsigned word[4] = {0u, 0u, 0u, 0u};
  MFN_UNROLL
  for (unsigned k = 0; k < 16u; ++k) {
    if (k < n) {
      const unsigned cs = p.bgr ? 2u - c : c;
      const unsigned char *r0 = p.src + (long long)ty.s * p.pitch + cs, *r1 = p.src + (long long)ty.s1 * p.pitch + cs;
      unsigned a00 = r0[3 * tx.s], a01 = r0[3 * tx.s1], a10 = r1[3 * tx.s], a11 = r1[3 * tx.s1];
      if (use_lut) { a00 = lut[a00]; a01 = lut[a01]; a10 = lut[a10]; a11 = lut[a11]; }
      const int h0 = (int)a00 * tx.i0 + (int)a01 * tx.i1, h1 = (int)a10 * tx.i0 + (int)a11 * tx.i1;
      const int v = ((ty.i0 * (h0 >> 4)) >> 16) + ((ty.i1 * (h1 >> 4)) >> 16);
      int o = (v + 2) >> 2;
      o = o < 0 ? 0 : (o > 255 ? 255 : o);
      word[k >> 2] |= (unsigned)o << (8u * (k & 3u));
      if (++c == 3u) {
        c = 0u;
        if (++x == (unsigned)p.Wd) {
          x = 0u;
          ++y;
          if (k + 1u < n) ty = p.rows[y];
        }
        if (k + 1u < n) tx = p.cols[x];
      }
    }
  }
  unsigned char *d = p.dst + b0;
  if (n == 16u) {
    *reinterpret_cast<ig_u32x4 *>(d) = ig_u32x4{word[0], word[1], word[2], word[3]};
  } else {
    for (unsigned k = 0; k < n; ++k) d[k] = (unsigned char)(word[k >> 2] >> (8u * (k & 3u)));
  }
}

// ---- min and max of both windows -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ingest_minmax_init_kernel(unsigned *out) {
  if (blockIdx.x == 0 && threadIdx.x < 2) out[threadIdx.x] = threadIdx.x == 0 ? 255u : 0u;
}

__global__ __launch_bounds__(INGEST_THREADS) void ingest_minmax_kernel(IngestMinmaxParams p) {
  int lo = 255, hi = 0;
  const unsigned long long stride = (unsigned long long)gridDim.x * INGEST_THREADS;
  const unsigned long long per_img = (unsigned long long)p.h * p.row_dwords;
  for (unsigned long long it = (unsigned long long)blockIdx.x * INGEST_THREADS + threadIdx.x; it < p.items; it += stride) {
    const unsigned img = it >= per_img ? 1u : 0u;
    const unsigned long long r = it - (img ? per_img : 0ull);
    const unsigned y = (unsigned)(r / p.row_dwords), k = (unsigned)(r - (unsigned long long)y * p.row_dwords);
    const unsigned char *base = img ? p.img2 : p.img1;
    // the row's bytes [a, e) as offsets from the (16-byte aligned) base; dword k of the aligned dwords that cover them
    const unsigned long long a = (unsigned long long)(p.y0 + (int)y) * (unsigned long long)p.pitch + 3ull * (unsigned)p.x0, e = a + 3ull * (unsigned)p.w;
    const unsigned long long q = (a & ~3ull) + 4ull * k;
    if (q < e) {   // begins inside the row's bytes or in the (at most three) bytes of the array in front of them
      const unsigned wv = *reinterpret_cast<const unsigned *>(base + q);
      MFN_UNROLL
      for (unsigned j = 0; j < 4u; ++j) {
        if (q + j >= a && q + j < e) {
          const int b = (int)((wv >> (8u * j)) & 0xffu);
          lo = b < lo ? b : lo;
          hi = b > hi ? b : hi;
        }
      }
    }
  }
  // wave, then block (LDS), then one atomic pair per block, and only where it still improves the words: they move one way only, so a
  // stale reading can cost an atomic but never lose one (every wave issuing its own pair: 100 us of contention on two addresses for
  // HD1K's 13.9 MB, profiles/ingest.md)
  lo = mfn_wave_min_i32(lo);
  hi = mfn_wave_max_i32(hi);
  MFN_DYN_SHARED(int, red);   // [2][waves]
  const unsigned wave = threadIdx.x >> 6, waves = INGEST_THREADS / 64;
  if (MFN_LANE_ID() == 0) { red[wave] = lo; red[waves + wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (unsigned k = 1; k < waves; ++k) {
      lo = red[k] < lo ? red[k] : lo;
      hi = red[waves + k] > hi ? red[waves + k] : hi;
    }
    if ((unsigned)lo < p.out[0]) ig_atomic_min(p.out, (unsigned)lo);
    if ((unsigned)hi > p.out[1]) ig_atomic_max(p.out + 1, (unsigned)hi);
  }
}

// ---- flow and validity -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ingest_flow_pixel(const IngestFlowParams &p, const IngestTap &ty, const IngestTap &tx, float &uo, float &vo,
                                                  unsigned &mo) {
#pragma clang fp contract(off)
  float hu[2], hv[2], ho[2];
  MFN_UNROLL
  for (int r = 0; r < 2; ++r) {
    const unsigned short *row = p.src + (long long)(r ? ty.s1 : ty.s) * p.pitch;
    float u[2], v[2], o[2];
    MFN_UNROLL
    for (int k = 0; k < 2; ++k) {
      const unsigned short *q = row + 3 * (k ? tx.s1 : tx.s);
      u[k] = ((float)q[0] - 32768.f) / 64.f;
      v[k] = ((float)q[1] - 32768.f) / 64.f;
      o[k] = (float)(q[2] & 0xffu);
      if (p.premultiply) { u[k] = u[k] * o[k]; v[k] = v[k] * o[k]; }
    }
    const float u0 = u[0] * tx.c0, u1 = u[1] * tx.c1, v0 = v[0] * tx.c0, v1 = v[1] * tx.c1, o0 = o[0] * tx.c0, o1 = o[1] * tx.c1;
    hu[r] = u0 + u1; hv[r] = v0 + v1; ho[r] = o0 + o1;
  }
  const float ua = hu[0] * ty.c0, ub = hu[1] * ty.c1, va = hv[0] * ty.c0, vb = hv[1] * ty.c1, oa = ho[0] * ty.c0, ob = ho[1] * ty.c1;
  float ur = ua + ub, vr = va + vb;
  const float orr = oa + ob;
  ur = ur * p.sx;
  vr = vr * p.sy;
  const float den = orr + (orr == 0.f ? 1.f : 0.f);
  uo = ur / den;
  vo = vr / den;
  const float m = orr * 255.f;
  mo = (unsigned)(int)m & 0xffu;
}

__global__ __launch_bounds__(INGEST_THREADS) void ingest_flow_occ_kernel(IngestFlowParams p) {
#pragma clang fp contract(off)
  const unsigned long long p0 = ((unsigned long long)blockIdx.x * INGEST_THREADS + threadIdx.x) * 4ull;
  if (p0 >= p.npix) return;
  const unsigned n = p.npix - p0 < 4ull ? (unsigned)(p.npix - p0) : 4u;
  unsigned y = (unsigned)(p0 / (unsigned)p.Wd), x = (unsigned)(p0 - (unsigned long long)y * (unsigned)p.Wd);
  IngestTap ty = p.rows[y];
  unsigned fu[4] = {0u, 0u, 0u, 0u}, fv[4] = {0u, 0u, 0u, 0u}, mw = 0u;
  MFN_UNROLL
  for (unsigned k = 0; k < 4u; ++k) {
    if (k < n) {
      const IngestTap tx = p.cols[x];
      float uo, vo;
      unsigned mo;
      ingest_flow_pixel(p, ty, tx, uo, vo, mo);
      fu[k] = (unsigned)mfn_f2i(uo);
      fv[k] = (unsigned)mfn_f2i(vo);
      if (p.flow_type == INGEST_FLOW_F16) { fu[k] = ig_half_bits(uo); fv[k] = ig_half_bits(vo); }
      mw |= mo << (8u * k);
      if (++x == (unsigned)p.Wd) {
        x = 0u;
        ++y;
        if (k + 1u < n) ty = p.rows[y];
      }
    }
  }
  if (p.flow_type == INGEST_FLOW_F16) {
    unsigned *d = reinterpret_cast<unsigned *>(p.flow) + p0;   // one (u, v) pair per dword
    if (n == 4u) *reinterpret_cast<ig_u32x4 *>(d) = ig_u32x4{fu[0] | (fv[0] << 16), fu[1] | (fv[1] << 16), fu[2] | (fv[2] << 16), fu[3] | (fv[3] << 16)};
    else for (unsigned k = 0; k < n; ++k) d[k] = fu[k] | (fv[k] << 16);
  } else {
    unsigned *d = reinterpret_cast<unsigned *>(p.flow) + 2ull * p0;
    if (n == 4u) {
      *reinterpret_cast<ig_u32x4 *>(d) = ig_u32x4{fu[0], fv[0], fu[1], fv[1]};
      *reinterpret_cast<ig_u32x4 *>(d + 4) = ig_u32x4{fu[2], fv[2], fu[3], fv[3]};
    } else {
      for (unsigned k = 0; k < n; ++k) { d[2u * k] = fu[k]; d[2u * k + 1u] = fv[k]; }
    }
  }
  if (n == 4u) *reinterpret_cast<unsigned *>(p.mask + p0) = mw;
  else for (unsigned k = 0; k < n; ++k) p.mask[p0 + k] = (unsigned char)(mw >> (8u * k));
}

// ---- the tables: host side -------------------------------------------------------------------------------------------------
inline size_t ingest_tables_bytes(int Hd, int Wd) { return Hd > 0 && Wd > 0 ? ((size_t)Hd + (size_t)Wd) * sizeof(IngestTap) : 0; }
// What a table has to carry to be used with a (h, w) window and a (Hd, Wd) destination: the layout's version and the four sizes.
inline unsigned long long ingest_tables_tag(int h, int w, int Hd, int Wd) {
  unsigned long long t = (0x16E57001ull << 32) ^ ((unsigned long long)sizeof(IngestTap) << 24);
  t ^= ((unsigned long long)(unsigned)h * 0x9E3779B97F4A7C15ull) >> 7;
  t ^= ((unsigned long long)(unsigned)w * 0xC2B2AE3D27D4EB4Full) >> 11;
  t ^= ((unsigned long long)(unsigned)Hd * 0x165667B19E3779F9ull) >> 13;
  t ^= ((unsigned long long)(unsigned)Wd * 0xD6E8FEB86659FD93ull) >> 17;
  return t;
}
inline void ingest_fill_taps(IngestTap *t, int src, int dst) {
#pragma clang fp contract(off)
  const double scale = (double)src / (double)dst;
  for (int d = 0; d < dst; ++d) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    IngestTap e{};
    e.s = s;
    e.s1 = s + 1 < src - 1 ? s + 1 : src - 1;
    e.c0 = 1.0f - f;
    e.c1 = f;
    e.i0 = (int)nearbyintf(e.c0 * 2048.f);   // the default rounding mode: half to even
    e.i1 = (int)nearbyintf(e.c1 * 2048.f);
    t[d] = e;
  }
}
// columns first (Wd entries), then rows (Hd entries)
inline void ingest_build_tables(IngestTap *t, int h, int w, int Hd, int Wd) {
  ingest_fill_taps(t, w, Wd);
  ingest_fill_taps(t + Wd, h, Hd);
}

inline int ingest_image_launch(IngestImageParams p, hipStream_t stream) {
  p.nbytes = (unsigned long long)p.Hd * (unsigned long long)p.Wd * 3ull;
  const unsigned long long chunks = (p.nbytes + 15ull) / 16ull;
  const dim3 grid((unsigned)((chunks + INGEST_THREADS - 1) / INGEST_THREADS));
  return launch("ingest_image_kernel", ingest_image_kernel, grid, dim3(INGEST_THREADS), 256, stream, p);
}

inline int ingest_minmax_launch(IngestMinmaxParams p, hipStream_t stream) {
  // a row's 3 w bytes at any alignment lie in at most (3 w + 3) / 4 + 1 aligned dwords
  p.row_dwords = (unsigned)((3ull * (unsigned)p.w + 3ull) / 4ull + 1ull);
  p.items = 2ull * (unsigned)p.h * p.row_dwords;
  if (int rc = launch("ingest_minmax_init_kernel", ingest_minmax_init_kernel, dim3(1), dim3(64), 0, stream, p.out)) return rc;
  unsigned long long blocks = (p.items + INGEST_THREADS - 1) / INGEST_THREADS;
  if (blocks > INGEST_MINMAX_BLOCKS) blocks = INGEST_MINMAX_BLOCKS;
  return launch("ingest_minmax_kernel", ingest_minmax_kernel, dim3((unsigned)blocks), dim3(INGEST_THREADS), 2 * (INGEST_THREADS / 64) * sizeof(int), stream, p);
}

inline int ingest_flow_occ_launch(IngestFlowParams p, hipStream_t stream) {
  p.npix = (unsigned long long)p.Hd * (unsigned long long)p.Wd;
  const unsigned long long quads = (p.npix + 3ull) / 4ull;
  const dim3 grid((unsigned)((quads + INGEST_THREADS - 1) / INGEST_THREADS));
  return launch("ingest_flow_occ_kernel", ingest_flow_occ_kernel, grid, dim3(INGEST_THREADS), 0, stream, p);
}

// ---- PNG row filters (host code; maskflownet_amd/io.py read_png) -------------------------------------------------------------
// `raw` holds `rows` scanlines of 1 + row_bytes bytes as zlib returned them: the filter type, then the filtered bytes.  Reverses the
// five filters of the PNG specification in place (the reconstructed bytes replace the filtered ones; the type bytes stay).  bpp: bytes
// per complete pixel, at least 1.  -> 0, or 1 + the row whose filter type is none of 0..4.
inline long long png_unfilter(unsigned char *raw, long long rows, long long row_bytes, int bpp) {
  const long long stride = row_bytes + 1;
  for (long long y = 0; y < rows; ++y) {
    unsigned char *cur = raw + y * stride + 1;
    const unsigned char *up = y ? cur - stride : nullptr;
    switch (cur[-1]) {
      case 0: break;
      case 1:
        for (long long i = bpp; i < row_bytes; ++i) cur[i] = (unsigned char)(cur[i] + cur[i - bpp]);
        break;
      case 2:
        if (up) for (long long i = 0; i < row_bytes; ++i) cur[i] = (unsigned char)(cur[i] + up[i]);
        break;
      case 3:
        for (long long i = 0; i < row_bytes; ++i) {
          const unsigned a = i >= bpp ? cur[i - bpp] : 0u, b = up ? up[i] : 0u;
          cur[i] = (unsigned char)(cur[i] + ((a + b) >> 1));
        }
        break;
      case 4:
        for (long long i = 0; i < row_bytes; ++i) {
          const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
          const int pp = a + b - c, pa = pp > a ? pp - a : a - pp, pb = pp > b ? pp - b : b - pp, pc = pp > c ? pp - c : c - pp;
          const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
          cur[i] = (unsigned char)(cur[i] + pr);
        }
        break;
      default: return 1 + y;
    }
  }
  return 0;
}

}  // namespace mfn
