// optimizer.h -- the trainer's Adam step, in place, one launch for every tensor of a step.
//
// Replaces `self.trainer.step(batch_size)` of /root/reference/network/pipeline.py:114 for the trainer :27 builds
// (gluon.Trainer(params, 'adam', {'learning_rate': 1e-4})): MXNet 1.5's `adam_update` operator (src/operator/optimizer_op-inl.h,
// AdamUpdate), which python/mxnet/optimizer/optimizer.py Adam.update calls with lr = lr * sqrt(1 - beta2^t) / (1 - beta1^t) -- both
// bias corrections folded into the learning rate on the host, so the denominator below is sqrt(var) + epsilon, not torch's
// sqrt(var) / sqrt(1 - beta2^t) + eps.  Per element, in this evaluation order, every product, sum, quotient and root rounded
// separately in fp32 (fp contraction off); tests/optimizer_ref.py restates this text in numpy:
//
//   g  = rescale_grad * grad + wd * w                     (wd == 0 still evaluates the product: 0 * inf = NaN, as MXNet)
//   g  = clip_gradient >= 0 ? min(max(g, -clip), clip) : g   (by comparisons: a NaN passes through, as mshadow_op::clip)
//   m' = beta1 * m + (1.0f - beta1) * g                   (1.0f - beta1 is formed in fp32)
//   v' = beta2 * v + (1.0f - beta2) * (g * g)
//   w' = w - (lr * m') / (sqrtf(v') + epsilon)
//
// No special case for NaN or inf: they propagate per element.  In the multi-tensor form lr and wd are lr * lr_mult and wd * wd_mult
// of the element's tensor (one fp32 product each, as Optimizer._get_lr / _get_wd hand them to the operator).
//
// One body, two instances.  A block of 256 threads owns one chunk of 4096 consecutive elements of ONE tensor: four quads per
// thread, quad k of thread t at element 4 * (256 k + t) of the chunk, so that a wave's request is 1 KiB of consecutive bytes.
//   adam_update_kernel<false>: the tensor's descriptor travels in the kernel arguments, blockIdx.x is the chunk.
//   adam_update_kernel<true>:  a device-resident table (built on the host by mfn_multi_adam_build_table, uploaded by the caller)
//     holds n_tensors descriptors followed by one {tensor, chunk} pair per block.  Both reads are indexed by blockIdx.x or by
//     what the first returned: wave-uniform, two dependent loads, no search in any thread.
// A tensor whose four pointers are 16-byte aligned moves 16 bytes per access, with a one-element route for the last n % 4
// elements; any other tensor takes the one-element route throughout (sixteen elements per thread, element 256 k + t).  Every
// element is read and written by exactly one thread: no atomics, no workspace, bit-identical from run to run.
//   bytes: 28 per element (w, grad, m, v read; w, m, v written): 294 MB for the 10.5 M parameters of MaskFlownet-S.
// m and v are not read again before the next step, w is read by the next forward: MFN_ADAM_NT chooses the cache policy of the
// accesses to m and v (profiles/trainer_adam.md has both measurements).
#pragma once
#include "../mfn_rt.h"

#ifndef MFN_ADAM_NT
#define MFN_ADAM_NT 0   // 0: plain accesses to m and v (measured faster: 44.9 against 48.2 us), 1: non-temporal (nt).  w and grad are always plain.
#endif

namespace mfn {

enum { ADAM_THREADS = 256, ADAM_QUADS = 4, ADAM_CHUNK = ADAM_THREADS * ADAM_QUADS * 4 };

struct AdamHyper { float lr, beta1, beta2, epsilon, wd, rescale_grad, clip_gradient; };

// One tensor of a step; 64 bytes, the table's first part.
struct AdamTensor {
  float *w;
  const float *g;
  float *m, *v;
  unsigned long long n;
  float lr_mult, wd_mult;
  unsigned aligned16;       // all four pointers are 16-byte aligned
  unsigned first_block;     // of the launch (multi-tensor form)
  unsigned pad_[2];
};
// One block of the multi-tensor launch; the table's second part.
struct AdamBlock { unsigned tensor, chunk; };
static_assert(sizeof(AdamTensor) == 64 && sizeof(AdamBlock) == 8, "the table's layout is part of its tag");

struct f32x4a { float x, y, z, w; } __attribute__((aligned(16)));

// The tensors' pointers come out of a table in memory, so hipcc cannot know that they point to global memory and would emit
// flat_load / flat_store (an aperture check per access, both wait counters): they are cast to the global address space once.
#if defined(MFN_EMU)
#define MFN_ADAM_GLOBAL
#else
#define MFN_ADAM_GLOBAL __attribute__((address_space(1)))
#endif
typedef MFN_ADAM_GLOBAL float adam_gf;

template <bool NT> __device__ __forceinline__ f32x4a adam_load4(const adam_gf *p) {
#if defined(MFN_EMU)
  return *reinterpret_cast<const f32x4a *>(p);
#else
  typedef float v4 __attribute__((ext_vector_type(4)));
  const MFN_ADAM_GLOBAL v4 *q = reinterpret_cast<const MFN_ADAM_GLOBAL v4 *>(p);
  const v4 r = NT ? __builtin_nontemporal_load(q) : *q;
  return f32x4a{r.x, r.y, r.z, r.w};
#endif
}
template <bool NT> __device__ __forceinline__ void adam_store4(adam_gf *p, const f32x4a &a) {
#if defined(MFN_EMU)
  *reinterpret_cast<f32x4a *>(p) = a;
#else
  typedef float v4 __attribute__((ext_vector_type(4)));
  const v4 r = {a.x, a.y, a.z, a.w};
  MFN_ADAM_GLOBAL v4 *q = reinterpret_cast<MFN_ADAM_GLOBAL v4 *>(p);
  if (NT) __builtin_nontemporal_store(r, q);
  else *q = r;
#endif
}
template <bool NT> __device__ __forceinline__ float adam_load1(const adam_gf *p) {
#if defined(MFN_EMU)
  return *p;
#else
  return NT ? __builtin_nontemporal_load(p) : *p;
#endif
}
template <bool NT> __device__ __forceinline__ void adam_store1(adam_gf *p, float a) {
#if defined(MFN_EMU)
  *p = a;
#else
  if (NT) __builtin_nontemporal_store(a, p);
  else *p = a;
#endif
}

// The expression of the header comment, one element.  omb1 = 1.0f - beta1, omb2 = 1.0f - beta2.
__device__ __forceinline__ void adam_element(float &w, float grad, float &m, float &v, const AdamHyper &h, float lr, float wd, float omb1,
                                             float omb2) {
#pragma clang fp contract(off)
  float g = h.rescale_grad * grad + wd * w;
  if (h.clip_gradient >= 0.f) g = g > h.clip_gradient ? h.clip_gradient : (g < -h.clip_gradient ? -h.clip_gradient : g);
  m = h.beta1 * m + omb1 * g;
  v = h.beta2 * v + omb2 * (g * g);
  w = w - (lr * m) / (sqrtf(v) + h.epsilon);
}

// One chunk of one tensor.  All of a thread's loads are issued before its arithmetic.
__device__ __forceinline__ void adam_chunk(const AdamTensor &t, unsigned chunk, const AdamHyper &h) {
#pragma clang fp contract(off)
  constexpr bool NT = MFN_ADAM_NT != 0;
  const float lr = h.lr * t.lr_mult, wd = h.wd * t.wd_mult;
  const float omb1 = 1.0f - h.beta1, omb2 = 1.0f - h.beta2;
  const unsigned long long base = (unsigned long long)chunk * ADAM_CHUNK, n = t.n;
  if (base >= n) return;
  const unsigned long long left = n - base;
  const unsigned len = left < (unsigned long long)ADAM_CHUNK ? (unsigned)left : (unsigned)ADAM_CHUNK;   // elements of this chunk
  adam_gf *w = (adam_gf *)t.w + base, *m = (adam_gf *)t.m + base, *v = (adam_gf *)t.v + base;
  const adam_gf *g = (const adam_gf *)t.g + base;
  if (t.aligned16) {   // base is a multiple of 4096 elements: the chunk's pointers are as aligned as the tensor's
    f32x4a W[ADAM_QUADS], G[ADAM_QUADS], M[ADAM_QUADS], V[ADAM_QUADS];
    MFN_UNROLL
    for (int k = 0; k < ADAM_QUADS; ++k) {
      const unsigned e = 4u * ((unsigned)k * ADAM_THREADS + threadIdx.x);
      if (e + 4u <= len) {
        W[k] = adam_load4<false>(w + e);
        G[k] = adam_load4<false>(g + e);
        M[k] = adam_load4<NT>(m + e);
        V[k] = adam_load4<NT>(v + e);
      }
    }
    MFN_UNROLL
    for (int k = 0; k < ADAM_QUADS; ++k) {
      const unsigned e = 4u * ((unsigned)k * ADAM_THREADS + threadIdx.x);
      if (e + 4u <= len) {
        adam_element(W[k].x, G[k].x, M[k].x, V[k].x, h, lr, wd, omb1, omb2);
        adam_element(W[k].y, G[k].y, M[k].y, V[k].y, h, lr, wd, omb1, omb2);
        adam_element(W[k].z, G[k].z, M[k].z, V[k].z, h, lr, wd, omb1, omb2);
        adam_element(W[k].w, G[k].w, M[k].w, V[k].w, h, lr, wd, omb1, omb2);
        adam_store4<false>(w + e, W[k]);
        adam_store4<NT>(m + e, M[k]);
        adam_store4<NT>(v + e, V[k]);
      }
    }
    const unsigned e = (len & ~3u) + threadIdx.x;   // the last len % 4 elements (only the tensor's last chunk has any)
    if (threadIdx.x < (len & 3u)) {
      float w1 = w[e], m1 = adam_load1<NT>(m + e), v1 = adam_load1<NT>(v + e);
      adam_element(w1, g[e], m1, v1, h, lr, wd, omb1, omb2);
      w[e] = w1;
      adam_store1<NT>(m + e, m1);
      adam_store1<NT>(v + e, v1);
    }
  } else {
    MFN_UNROLL
    for (int k = 0; k < ADAM_QUADS * 4; ++k) {
      const unsigned e = (unsigned)k * ADAM_THREADS + threadIdx.x;
      if (e < len) {
        float w1 = w[e], m1 = adam_load1<NT>(m + e), v1 = adam_load1<NT>(v + e);
        adam_element(w1, g[e], m1, v1, h, lr, wd, omb1, omb2);
        w[e] = w1;
        adam_store1<NT>(m + e, m1);
        adam_store1<NT>(v + e, v1);
      }
    }
  }
}

struct AdamParams {
  AdamTensor one;               // MULTI == false: the tensor itself
  const AdamTensor *tensors;    // MULTI == true: the table's descriptors ...
  const AdamBlock *blocks;      // ... and its blocks
  unsigned n_tensors, n_blocks;
  AdamHyper h;
};

template <bool MULTI>
__global__ __launch_bounds__(ADAM_THREADS) void adam_update_kernel(AdamParams p) {
  if (MULTI) {
    if (blockIdx.x >= p.n_blocks) return;
    const AdamBlock b = p.blocks[blockIdx.x];      // wave-uniform: indexed by the block
    if (b.tensor >= p.n_tensors) return;
    const AdamTensor t = p.tensors[b.tensor];      // wave-uniform: indexed by what the block read
    adam_chunk(t, b.chunk, p.h);
  } else {
    adam_chunk(p.one, blockIdx.x, p.h);
  }
}

// ---- the table: host side --------------------------------------------------------------------------------------------------
inline unsigned long long adam_blocks_of(unsigned long long n) { return (n + ADAM_CHUNK - 1) / ADAM_CHUNK; }
inline size_t adam_table_bytes(unsigned n_tensors, unsigned long long n_blocks) {
  return (size_t)n_tensors * sizeof(AdamTensor) + (size_t)n_blocks * sizeof(AdamBlock);
}
// What a table of this shape has to carry: the layout's version (descriptor and block sizes, chunk length) and both counts.
inline unsigned long long adam_table_tag(unsigned n_tensors, unsigned n_blocks) {
  unsigned long long t = 0xADA30001ull << 32;
  t ^= ((unsigned long long)sizeof(AdamTensor) << 24) ^ ((unsigned long long)sizeof(AdamBlock) << 16) ^ (unsigned long long)ADAM_CHUNK;
  t ^= ((unsigned long long)n_tensors * 0x9E3779B97F4A7C15ull) >> 7;
  t ^= ((unsigned long long)n_blocks * 0xC2B2AE3D27D4EB4Full) >> 11;
  return t;
}
inline bool adam_aligned16(const void *a, const void *b, const void *c, const void *d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15u) == 0;
}

inline int adam_update_launch(const AdamTensor &t, const AdamHyper &h, hipStream_t stream) {
  if (t.n == 0) return 0;
  AdamParams p{};
  p.one = t;
  p.h = h;
  return launch("adam_update", adam_update_kernel<false>, dim3((unsigned)adam_blocks_of(t.n)), dim3(ADAM_THREADS), 0, stream, p);
}
inline int multi_adam_update_launch(const void *table, unsigned n_tensors, unsigned n_blocks, const AdamHyper &h, hipStream_t stream) {
  if (n_blocks == 0) return 0;
  AdamParams p{};
  p.tensors = reinterpret_cast<const AdamTensor *>(table);
  p.blocks = reinterpret_cast<const AdamBlock *>(reinterpret_cast<const char *>(table) + (size_t)n_tensors * sizeof(AdamTensor));
  p.n_tensors = n_tensors;
  p.n_blocks = n_blocks;
  p.h = h;
  return launch("multi_adam_update", adam_update_kernel<true>, dim3(n_blocks), dim3(ADAM_THREADS), 0, stream, p);
}

}  // namespace mfn
