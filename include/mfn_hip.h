/*
 * mfn_hip.h -- C ABI of libmfn_hip.so: the MI355X (gfx950) implementation of MaskFlownet's
 * per-pyramid-level matching hot path.  This is the drop-in boundary: every entry point
 * replaces one MXNet operator call made by /root/reference (file:line cited per function)
 * and is what a ctypes / MXNet-CustomOp binding on the reference side binds to
 * (INTEGRATION.md shows the stubs).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch/MXNet types cross the boundary.
 *   - every tensor is a contiguous fp32 NCHW buffer in DEVICE memory, owned by the caller.
 *     Outputs are fully overwritten unless a `req` argument says otherwise.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls only
 *     enqueue work; they never synchronise and never allocate device memory.
 *   - return value: 0 = ok; < 0 = bad argument (MFN_E_*); > 0 = a hipError_t from the
 *     launch.  mfn_last_error() returns a thread-local description of the last failure.
 *     Nothing throws across the boundary.
 *   - the operator entry points are re-entrant and keep no per-call state: any number of host threads may call
 *     them concurrently on their own streams.  What arithmetic a call uses is the process's setting
 *     (mfn_set_arithmetic: one atomic value per operator, read by whichever thread makes the call).  The process-global MEASUREMENT state is the exception and is not
 *     part of the drop-in surface: mfn_set_tuning (tilings / code paths only) / mfn_profile_* / mfn_debug_set_timeline
 *     write plain globals that every launch reads -- call them only while no other thread is inside the library.
 *   - flow tensors use the network's channel order: channel 0 = dy (vertical),
 *     channel 1 = dx (horizontal)   (/root/reference/network/pipeline.py:105,
 *     /root/reference/network/layer.py:17).
 */
#ifndef MFN_HIP_H
#define MFN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFN_ABI_VERSION 1

/* status codes (< 0); > 0 are hipError_t values */
#define MFN_OK 0
#define MFN_E_NULL (-1)        /* a required pointer is NULL */
#define MFN_E_SHAPE (-2)       /* a dimension is non-positive or inconsistent */
#define MFN_E_PARAM (-3)       /* an operator parameter is outside what MXNet accepts */
#define MFN_E_UNSUPPORTED (-4) /* valid for MXNet, not implemented by this library */
#define MFN_E_WORKSPACE (-5)   /* workspace missing or too small */
#define MFN_E_ALIGN (-6)       /* a pointer is not 4-byte aligned */

/* OpReqType of MXNet (include/mxnet/op_attr_types.h) for gradient outputs */
#define MFN_REQ_NULL 0
#define MFN_REQ_WRITE 1
#define MFN_REQ_ADD 3

int mfn_abi_version(void);
const char *mfn_version_string(void);
/* Thread-local text for the last non-zero status returned on this thread ("" if none). */
const char *mfn_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Correlation  -- replaces F.Correlation(data1, data2, kernel_size, max_displacement, stride1,
 * stride2, pad_size, is_multiply) at /root/reference/network/MaskFlownet.py:193-195 (md=4) and
 * :440-441 (md=2).  Semantics: MXNet src/operator/correlation.cc:
 *   out[n, (dy/s2 + r)*D + (dx/s2 + r), i, j] =
 *       1/(K*K*C) * sum_{h,w<K} sum_c pad(data1)[n,c,y1+h,x1+w] * pad(data2)[n,c,y1+dy+h,x1+dx+w]
 *   r = max_displacement/stride2, D = 2r+1, y1 = i*stride1 + max_displacement (padded coords).
 * data1,data2: (N,C,H,W); out: (N, D*D, top_h, top_w) from mfn_correlation_out_shape.
 * The reference configuration (kernel_size=1, strides 1, pad_size == max_displacement) runs
 * the LDS-tiled kernel; any other valid configuration runs a generic kernel.
 * ------------------------------------------------------------------------------------------- */
int mfn_correlation_out_shape(int H, int W, int max_displacement, int kernel_size, int stride1,
                              int stride2, int pad_size, int *top_channels, int *top_h, int *top_w);
int mfn_correlation_fwd(const float *data1, const float *data2, float *out, int N, int C, int H,
                        int W, int max_displacement, int kernel_size, int stride1, int stride2,
                        int pad_size, int is_multiply, void *stream);
/* Same operator with a scratch buffer: levels with few pixels and many channels (L6..L3 of the
 * pyramid) are split into channel slices across workgroups, partial sums go to `workspace` and a
 * second kernel reduces them in a fixed order (deterministic).  workspace may be NULL / too small:
 * the call then runs the single-pass kernel.  mfn_correlation_workspace_bytes returns the size the
 * heuristic wants (0 when slicing would not be used). */
size_t mfn_correlation_workspace_bytes(int N, int C, int H, int W, int max_displacement, int kernel_size,
                                       int stride1, int stride2, int pad_size, int is_multiply);
int mfn_correlation_fwd_ws(const float *data1, const float *data2, float *out, int N, int C, int H,
                           int W, int max_displacement, int kernel_size, int stride1, int stride2,
                           int pad_size, int is_multiply, void *workspace, size_t workspace_bytes,
                           void *stream);
/* Fused epilogue: the reference applies LeakyReLU(0.1) to every cost volume right
 * away (/root/reference/network/MaskFlownet.py:217,231,249,267,285: self.leakyRELU(self.corr(...))).
 * activation: MFN_ACT_NONE or MFN_ACT_LEAKY_0_1 (max(v, 0.1 v), applied after the 1/C normalisation,
 * bit-identical to the separate elementwise op).  Otherwise identical to mfn_correlation_fwd_ws. */
#define MFN_ACT_NONE 0
#define MFN_ACT_LEAKY_0_1 1
int mfn_correlation_fwd_act(const float *data1, const float *data2, float *out, int N, int C, int H,
                            int W, int max_displacement, int kernel_size, int stride1, int stride2,
                            int pad_size, int is_multiply, int activation, void *workspace,
                            size_t workspace_bytes, void *stream);
/* Rest of f-1: the cost volume written straight into its channel slice of the decoder's concat buffer
 * (/root/reference/network/MaskFlownet.py:235,253,271,289: x = concat(corr, c1, feat, flow)) -- no concat copy.
 * out points at channel c0 of image 0 of a contiguous (N, Ctot, h, w) buffer; out_batch_stride = Ctot*h*w elements
 * (0 = dense, i.e. D*D*h*w).  Must be >= one output image; the 16-byte-store kernels need out 16-byte aligned and
 * the stride a multiple of 4 (otherwise the generic kernel runs).  Otherwise identical to mfn_correlation_fwd_act. */
int mfn_correlation_fwd_into(const float *data1, const float *data2, float *out, long long out_batch_stride,
                             int N, int C, int H, int W, int max_displacement, int kernel_size, int stride1,
                             int stride2, int pad_size, int is_multiply, int activation, void *workspace,
                             size_t workspace_bytes, void *stream);
/* Backward of the same call site (training, /root/reference/network/pipeline.py:112-113).
 * g1/g2: (N,C,H,W); req1/req2 in {MFN_REQ_NULL, MFN_REQ_WRITE, MFN_REQ_ADD}.  The reference configuration's kernels add in a
 * fixed order (bit-identical from run to run); any other valid configuration runs a scatter kernel that accumulates with fp32
 * atomics: the same results up to summation order. */
int mfn_correlation_bwd(const float *gout, const float *data1, const float *data2, float *g1,
                        float *g2, int N, int C, int H, int W, int max_displacement,
                        int kernel_size, int stride1, int stride2, int pad_size, int is_multiply,
                        int req1, int req2, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Warp -- replaces the operator pair of /root/reference/network/layer.py:14-18
 * (Reconstruction2D) and :26-30 (Reconstruction2DSmooth):
 *     grid = GridGenerator(flow.flip(axis=1), 'warp') [.clip(-1, 1)];  out = BilinearSampler(x, grid)
 * fused into one kernel.  x,out: (N,C,H,W); flow_yx: (N,2,H,W).  clip_grid=1 is the Smooth
 * variant (border replicate).  Semantics: MXNet grid_generator-inl.h (kWarp) +
 * bilinear_sampler.cc, including the fp32 normalise/denormalise
 * round trip and per-tap zero padding.
 * ------------------------------------------------------------------------------------------- */
int mfn_warp_fwd(const float *x, const float *flow_yx, float *out, int N, int C, int H, int W,
                 int clip_grid, void *stream);
/* gx: (N,C,H,W) data gradient, gflow_yx: (N,2,H,W) flow gradient (NULL / MFN_REQ_NULL to skip,
 * which is what block_grad=True in layer.py:15-16 does).  gx is scattered with fp32 atomics (as MXNet's GPU kernel does): its
 * bit-level results can differ from run to run by summation order; gflow_yx is deterministic. */
int mfn_warp_bwd(const float *gout, const float *x, const float *flow_yx, float *gx,
                 float *gflow_yx, int N, int C, int H, int W, int clip_grid, int req_x,
                 int req_flow, void *stream);
/* The two MXNet operators on their own (also used by /root/reference/augmentation.py:60-64,
 * 306-321,333).  flow_xy/grid: (N,2,H,W) channel 0 = x.  theta: (N,6) row-major 2x3. */
int mfn_grid_generator_warp(const float *flow_xy, float *grid, int N, int H, int W, void *stream);
int mfn_grid_generator_affine(const float *theta, float *grid, int N, int H, int W, void *stream);
int mfn_bilinear_sampler_fwd(const float *data, const float *grid, float *out, int N, int C,
                             int iH, int iW, int oH, int oW, void *stream);
/* Backward of the operator pair (what MXNet's autograd reaches where the reference differentiates a warp it built
 * from the two operators: c40 of /root/reference/network/MaskFlownet.py:311, block_grad=False).  gdata: (N,C,iH,iW),
 * ggrid: (N,2,oH,oW) channel 0 = x; gflow_xy = ggrid / ((size-1)/2).  req in {MFN_REQ_NULL, _WRITE, _ADD}.  gdata is scattered
 * with fp32 atomics: the same results up to summation order from run to run; ggrid is deterministic. */
int mfn_bilinear_sampler_bwd(const float *gout, const float *data, const float *grid, float *gdata,
                             float *ggrid, int N, int C, int iH, int iW, int oH, int oW,
                             int req_data, int req_grid, void *stream);
int mfn_grid_generator_warp_bwd(const float *ggrid, float *gflow_xy, int N, int H, int W, int req,
                                void *stream);

/* ---------------------------------------------------------------------------------------------
 * DeformableConvolution -- replaces F.contrib.DeformableConvolution(x, offset, weight[, bias],
 * kernel, stride, dilate, pad, num_filter, num_group, num_deformable_group, no_bias) at
 * /root/reference/network/layer.py:117-124 (kwargs :91-95).  Semantics: MXNet
 * contrib/nn/deformable_im2col.* + contrib/deformable_convolution-inl.h:
 *   out[n,o,y,x] = bias[o] + sum_{c,i,j} w[o,c,i,j] * S(x[n,c], y*sh-ph+i*dh + off[n,2k,y,x],
 *                                                        x*sw-pw+j*dw + off[n,2k+1,y,x]),  k=i*kw+j
 *   S = 0 when a coordinate is < 0 or >= dim; bilinear with clamp-to-last inside [dim-1, dim).
 * x: (N,Cin,H,W); offset: (N, 2*kh*kw*deform_groups, Ho, Wo); w: (Cout, Cin/groups, kh, kw);
 * bias: (Cout) or NULL (no_bias); out: (N,Cout,Ho,Wo).
 * The im2col buffer is never materialised: the gather feeds fp32 MFMA tiles directly.
 * `workspace` holds the re-laid-out weights and, for coarse levels whose reduction dimension is
 * split across workgroups, the partial sums (mfn_deform_conv_workspace_bytes); it is scratch,
 * valid only for the duration of the call's stream work.
 * ------------------------------------------------------------------------------------------- */
int mfn_deform_conv_out_shape(int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                              int dw, int *Ho, int *Wo);
size_t mfn_deform_conv_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh,
                                       int sw, int ph, int pw, int dh, int dw, int groups,
                                       int deform_groups);
int mfn_deform_conv_fwd(const float *x, const float *offset, const float *w,
                        const float *bias_or_null, float *out, int N, int Cin, int H, int W,
                        int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                        int groups, int deform_groups, void *workspace, size_t workspace_bytes,
                        void *stream);
/* Fused form of the reference's call pattern /root/reference/network/MaskFlownet.py:230,248,266,
 * 284: offset = repeat9(flow * flow_scale / flow_stride) is never built; every tap of pixel
 * (y,x) uses (flow[n,0,y,x], flow[n,1,y,x]) * flow_scale / flow_stride.  Same result as
 * mfn_offsets_from_flow + mfn_deform_conv_fwd.  Requires stride 1 (Ho=H, Wo=W). */
int mfn_deform_conv_shared_fwd(const float *x, const float *flow_yx, float flow_scale,
                               float flow_stride, const float *w, const float *bias_or_null,
                               float *out, int N, int Cin, int H, int W, int Cout, int kh, int kw,
                               int ph, int pw, int dh, int dw, int groups, void *workspace,
                               size_t workspace_bytes, void *stream);
/* Inference: a Gluon block (/root/reference/network/layer.py:97-124) owns constant weights, so
 * their re-layout can be done once instead of on every call.  mfn_deform_conv_pack_weights writes
 * the layout the kernels stream (an opaque function of the 15 shape ints and of mfn_set_tuning;
 * mfn_deform_conv_packed_weight_bytes gives its size) and the *_packed entry points take it in
 * place of `w`, with the layout tag pack_weights returned; their workspace then only holds split-K
 * partial sums (the value returned by mfn_deform_conv_workspace_bytes is always enough).  Results
 * are bit-identical to the unpacked calls.  A tag that does not match the layout the current
 * shape/tuning needs is refused with MFN_E_WORKSPACE, never silently used. */
size_t mfn_deform_conv_packed_weight_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw,
                                           int sh, int sw, int ph, int pw, int dh, int dw,
                                           int groups, int deform_groups);
int mfn_deform_conv_pack_weights(const float *w, int N, int Cin, int H, int W, int Cout, int kh,
                                 int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                                 int deform_groups, void *packed, size_t packed_bytes,
                                 unsigned long long *layout_tag, void *stream);
int mfn_deform_conv_fwd_packed(const float *x, const float *offset, const void *packed,
                               size_t packed_bytes, unsigned long long layout_tag,
                               const float *bias_or_null, float *out, int N,
                               int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw,
                               int ph, int pw, int dh, int dw, int groups, int deform_groups,
                               void *workspace, size_t workspace_bytes, void *stream);
int mfn_deform_conv_shared_fwd_packed(const float *x, const float *flow_yx, float flow_scale,
                                      float flow_stride, const void *packed, size_t packed_bytes,
                                      unsigned long long layout_tag, const float *bias_or_null, float *out, int N, int Cin, int H,
                                      int W, int Cout, int kh, int kw, int ph, int pw, int dh,
                                      int dw, int groups, void *workspace, size_t workspace_bytes,
                                      void *stream);
/* The whole warp step of the matching module in one launch, for
 * /root/reference/network/MaskFlownet.py:230-233 (and :248-251, :266-269, :284-287):
 *   warp = deform(c2, repeat9(flow*scale/stride)); warp = warp * sigmoid(mask) + tradeoff; warp = LeakyReLU(0.1)(warp)
 * mask: (N,1,H,W) or NULL; tradeoff: (N,Cout,H,W) (the conv5f(feat) term) or NULL; activation: MFN_ACT_*.
 * Give either `w` (re-packed on every call into workspace) or `packed` + layout tag (see above).
 * Elementwise results equal the separate ops' (sigmoid = 1/(1+expf(-m)) in fp32). */
int mfn_deform_conv_matching_fwd(const float *x, const float *flow_yx, float flow_scale, float flow_stride,
                                 const float *w_or_null, const void *packed_or_null, size_t packed_bytes,
                                 unsigned long long layout_tag, const float *bias_or_null,
                                 const float *mask_or_null, const float *tradeoff_or_null, int activation,
                                 float *out, int N, int Cin, int H, int W, int Cout, int kh, int kw, int ph,
                                 int pw, int dh, int dw, int groups, void *workspace, size_t workspace_bytes,
                                 void *stream);
/* Backward (training).  gx,goffset,gw,gbias as the forward's x,offset,w,bias; req_* per output
 * (MFN_REQ_NULL skips it and the pointer may be NULL).  The column gradient is formed on the fly.
 * Scratch (mfn_deform_conv_bwd_workspace_bytes; 0 for shapes other than 3x3 / stride 1 / dilation 1
 * / one group): the per-block partial sums of the weight / bias gradient, which a second kernel
 * adds in a fixed order.  workspace may be NULL or smaller (parameter gradients through atomics:
 * same results up to summation order).  Tiles whose nine taps share one offset
 * (MaskFlownet.py:230) take all taps in one pass, the others tap by tap, in the same launch.  gx and goffset are accumulated with fp32 atomics (as MXNet's GPU kernels do): their
 * bit-level results can differ from run to run by summation order; with the workspace gw and gbias
 * are deterministic. */
size_t mfn_deform_conv_bwd_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw,
                                           int sh, int sw, int ph, int pw, int dh, int dw,
                                           int groups, int deform_groups);
int mfn_deform_conv_bwd(const float *gout, const float *x, const float *offset, const float *w,
                        float *gx, float *goffset, float *gw, float *gbias_or_null, int N, int Cin,
                        int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                        int dh, int dw, int groups, int deform_groups, int req_x, int req_offset,
                        int req_w, int req_bias, void *workspace, size_t workspace_bytes,
                        void *stream);
/* Backward of the fused call mfn_deform_conv_shared_fwd (training with the offsets never built by the caller):
 * gflow (N,2,H,W) = d loss / d flow_yx = flow_scale / flow_stride * sum over the taps of the offset gradient; gx, gw, gbias
 * and the req_* as mfn_deform_conv_bwd.  The workspace (mfn_deform_conv_shared_bwd_workspace_bytes, required, 16-byte
 * aligned) has room for the offsets and their gradient: shapes outside the lane = pixel kernels (3x3, pad 1, one group,
 * W % 4 == 0, Cin % 4 == 0, Cout <= 96) are composed as mfn_offsets_from_flow -> mfn_deform_conv_bwd ->
 * mfn_offsets_from_flow_bwd; inside, the kernels read the flow field and write gflow themselves.  mfn_offsets_from_flow_bwd
 * is the gradient of mfn_offsets_from_flow on its own (req: MFN_REQ_WRITE or MFN_REQ_ADD). */
size_t mfn_deform_conv_shared_bwd_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int ph,
                                                  int pw, int dh, int dw, int groups);
int mfn_deform_conv_shared_bwd(const float *gout, const float *x, const float *flow_yx, float flow_scale,
                               float flow_stride, const float *w, float *gx, float *gflow, float *gw,
                               float *gbias, int N, int Cin, int H, int W, int Cout, int kh, int kw, int ph,
                               int pw, int dh, int dw, int groups, int req_x, int req_flow, int req_w,
                               int req_bias, void *workspace, size_t workspace_bytes, void *stream);
int mfn_offsets_from_flow_bwd(const float *goffset, float *gflow_yx, int N, int H, int W, int taps,
                              float flow_scale, float flow_stride, int req, void *stream);

/* Upsample(factor) of flow / mask between pyramid levels -- replaces the Gluon block
 * /root/reference/network/MaskFlownet.py:35-62 (edge pad + Deconvolution with the triangle kernel
 * 1-|f-1-a|/f, kernel 2f-1, stride f, pad f-1, last row/column dropped; call sites :228-229 ... :311).
 * x: (N,C,H,W) -> out: (N,C,H*factor,W*factor); factor 1 copies.  Bit-identical to the fp32 oracle. */
int mfn_upsample_fwd(const float *x, float *out, int N, int C, int H, int W, int factor, void *stream);
/* Its backward (the block is linear; on the gradient path of every level: flow5 = Upsample(2)(flow6), MaskFlownet.py:228):
 * gout: (N,C,H*factor,W*factor) -> gx: (N,C,H,W); req: MFN_REQ_*.  What MXNet's autograd computes through the
 * pad / Deconvolution / slice chain of :51-62. */
int mfn_upsample_bwd(const float *gout, float *gx, int N, int C, int H, int W, int factor, int req, void *stream);
/* LeakyReLU(slope) backward from the forward OUTPUT y: gin = gout * (y > 0 ? 1 : slope) -- the gradient side of the fused
 * activations (mfn_correlation_fwd_act, mfn_conv2d_fwd activation = MFN_ACT_LEAKY_0_1; nn.LeakyReLU(0.1) of
 * /root/reference/network/MaskFlownet.py:76,217).  gin may alias gout. */
int mfn_leaky_relu_bwd(const float *gout, const float *y, float *gin, size_t n, float slope, void *stream);
/* The gate of the matching module on its own, for training through a pyramid level (kernels/gate.h) -- replaces
 * network/MaskFlownet.py:231-233 (and :249-251, :267-269, :285-287), the part of mfn_deform_conv_matching_fwd after the
 * deformable convolution, whose output `raw` the backward pass needs:
 *   out = act(raw * s + tradeoff),  s = 1 / (1 + expf(-mask))
 * raw, tradeoff, out: (N,C,H,W); mask: (N,1,H,W); mask and tradeoff each optional; activation: MFN_ACT_*.  Per element the
 * arithmetic of mfn_deform_conv_matching_fwd's epilogue (the same device function).
 * Backward, from g = gout (+ gout2: an optional second upstream gradient, added first), the forward OUTPUT y, raw and mask:
 *   gp        = activation ? g * (y > 0 ? 1 : 0.1) : g                 (the rule of mfn_leaky_relu_bwd)
 *   gtradeoff = gp
 *   graw      = gp * s                                                  (gp without a mask)
 *   gmask     = s * s' * sum_c gp[n,c,h,w] * raw[n,c,h,w],   s' = 1 / (1 + expf(+mask)), evaluated on its own (not 1 - s:
 *               no bit of that is right on a saturated mask)
 * req_* per output (MFN_REQ_NULL skips it and the pointer may be NULL); req_mask other than null without a mask is
 * MFN_E_PARAM.  y is read with MFN_ACT_LEAKY_0_1 only, raw for gmask only: either may be NULL otherwise.  All three reqs
 * null, or N == 0: nothing is launched.
 * Deterministic: the channel sum of gmask is added in a fixed order that depends on (N, C, H, W) alone, without atomics --
 * bit-identical from call to call.  Levels with few pixels split the channels over blocks; their partial sums need
 * mfn_matching_gate_bwd_workspace_bytes of scratch (0 where one block row per image suffices) when req_mask is not null: a
 * shorter workspace is MFN_E_WORKSPACE before any launch, there is no other route.  16-byte loads and stores where
 * W % 4 == 0 and every pointer is 16-byte aligned, scalar ones otherwise; same results.  No output may alias an input or
 * another output. */
int mfn_matching_gate_fwd(const float *raw, const float *mask_or_null, const float *tradeoff_or_null, int activation,
                          float *out, int N, int C, int H, int W, void *stream);
size_t mfn_matching_gate_bwd_workspace_bytes(int N, int C, int H, int W);
int mfn_matching_gate_bwd(const float *gout, const float *gout2_or_null, const float *y, const float *raw,
                          const float *mask_or_null, int activation, float *graw, float *gmask, float *gtradeoff,
                          int N, int C, int H, int W, int req_raw, int req_mask, int req_tradeoff,
                          void *workspace, size_t workspace_bytes, void *stream);
/* Offset builder of /root/reference/network/MaskFlownet.py:230:
 *   offset[n, 2k+t, y, x] = flow_yx[n, t, y, x] * scale / stride   for k < taps. */
int mfn_offsets_from_flow(const float *flow_yx, float *offset, int N, int H, int W, int taps,
                          float scale, float stride, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Prediction on images of any size -- replace the device side of PipelineFlownet in
 * /root/reference/network/pipeline.py: centralize (:85-87), do_batch_mx (:117-132), do_batch (:134-147) and the
 * metrics of validate (:176-182).  maskflownet_amd/predict.py composes them around the network's hipGraph.
 *
 * [MXNet-ext, unpinned] contrib.BilinearResize2D of MXNet 1.5 (bilinear_resize.cc, align_corners), per axis:
 *   r = (out > 1) ? (float)(in-1)/(float)(out-1) : 0.f;  p = r * (float)o;  i0 = (int)p;  ip = (i0 < in-1) ? 1 : 0;
 *   l1 = p - (float)i0;  l0 = 1.f - l1;
 *   out = h0*(w0*x[i0][j0] + w1*x[i0][j0+jp]) + h1*(w0*x[i0+ip][j0] + w1*x[i0+ip][j0+jp])
 * with positions, lambdas and the blend in fp32, every operation rounded separately; equal sizes copy.
 *
 * The two reductions (joint mean, metrics) run in a fixed order through the caller's workspace, without atomics: results
 * are bit-identical from run to run and no term passes through more than 46 additions, so that
 * |result - exact| <= 64 * 2^-24 * sum |terms| (/ n for the mean).  A missing or too small workspace is MFN_E_WORKSPACE. */
/* rgb_mean of pipeline.py:86: mean[n,c] = (sum im1[n,c] + sum im2[n,c]) / (2 H W); im1, im2: (N,C,H,W), mean: (N,C). */
size_t mfn_pair_mean_workspace_bytes(int N, int C, int H, int W);
int mfn_pair_mean(const float *im1, const float *im2, float *mean, int N, int C, int H, int W, void *workspace,
                  size_t workspace_bytes, void *stream);
/* pipeline.py:120, :129-130 in one launch: out[0:N] = resize(im1 - mean), out[N:2N] = resize(im2 - mean);
 * out: (2N,C,Hout,Wout), the network's input batch.  The mean is subtracted from every tap before the blend (the
 * reference's order: centralize, then resize); Hout == H and Wout == W gives exactly x - mean. */
int mfn_preprocess_pair(const float *im1, const float *im2, const float *mean, float *out, int N, int C, int H, int W,
                        int Hout, int Wout, void *stream);
/* contrib.BilinearResize2D (pipeline.py:129-130, :140, :142): x (N,C,Hin,Win) -> out (N,C,Hout,Wout).
 * sub_or_null: (N,C), subtracted from every tap before the blend.  flow_rescale != 0 (C == 2, else MFN_E_SHAPE): channel 0
 * * (float)((double)Hout/Hin), channel 1 * (float)((double)Wout/Win) after the blend, one rounding (pipeline.py:140-141). */
int mfn_bilinear_resize_fwd(const float *x, const float *sub_or_null, float *out, int N, int C, int Hin, int Win, int Hout,
                            int Wout, int flow_rescale, void *stream);
/* EpeLossWithMask (/root/reference/network/MaskFlownet.py:576-583, pipeline.py:146) and the KITTI outlier ratio
 * (pipeline.py:182) as sums; the caller divides.  flow, label: (N,2,H,W) in network order (channel 0 = dy), mask: (N,1,H,W).
 * sums (N,3): sum mask * sqrt(|flow-label|^2 + 1e-8), sum mask,
 *             sum mask * [|flow-label| > 3 and |flow-label| / (|label| + 1e-8) > 0.05],  |v| = sqrt(v_y^2 + v_x^2). */
size_t mfn_flow_metrics_workspace_bytes(int N, int H, int W);
int mfn_flow_metrics(const float *flow, const float *label, const float *mask, float *sums, int N, int H, int W,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Prediction on uint8 frame sequences and the colour picture of a flow -- replace the arithmetic of the
 * reference's /root/reference/predict_new_data.py around `pipe.predict(prev_frames, new_frames)` (:152-158) for frames that are on
 * the device as bytes.  kernels/frames.h spells out every expression.
 * frames: (F,H,W,3) uint8, HWC.  A batch of N pairs is two first indices: pair n is (frames[a0+n], frames[b0+n]) -- a video passes
 * b0 = a0 + 1, two stacked lists b0 = a0 + N.  No alignment is asked of `frames`: wider-than-byte loads are taken only where the
 * address allows them.
 * Errors before any launch: a NULL tensor (MFN_E_NULL); N, a0 or b0 < 0, a0 + N > F, b0 + N > F, H, W, Hout or Wout < 1
 * (MFN_E_SHAPE, the message names the argument); a missing or short workspace (MFN_E_WORKSPACE); a float pointer that is not 4-byte
 * aligned (MFN_E_ALIGN).  N == 0 succeeds and touches nothing. */
/* rgb_mean of pipeline.py:86 for the images bytes / 255 of pipeline.py:208, EXACT: per (n, c) the 2 H W bytes are summed as integers
 * (fixed order through the workspace, no atomics) and mean[n,c] = (float)((double)sum / (255.0 * 2 H W)): order-independent,
 * bit-identical to np.float32(np.float64(sum) / np.float64(255 * 2 * H * W)).  Not the bits of mfn_pair_mean on byte / 255 floats,
 * which sums rounded quotients in fp32.  mean: (N,3). */
size_t mfn_pair_mean_u8_workspace_bytes(int N, int H, int W);
int mfn_pair_mean_u8(const unsigned char *frames, int F, int H, int W, int a0, int b0, int N, float *mean, void *workspace,
                     size_t workspace_bytes, void *stream);
/* pipeline.py:208 (`/ 255`, HWC -> CHW), :120 and :129-130 in one launch: mfn_preprocess_pair reading byte taps, each
 * (float)byte / 255.f.  out: (2N,3,Hout,Wout), image 1 in rows [0,N), image 2 in rows [N,2N).  Bit-identical to
 * mfn_preprocess_pair on the floats byte / 255.f with the same mean.  mean_or_null: (N,3), NULL subtracts nothing.  Hout == H and
 * Wout == W unpacks the bytes into float CHW (- mean). */
int mfn_preprocess_pair_u8(const unsigned char *frames, int F, int H, int W, int a0, int b0, int N, const float *mean_or_null,
                           float *out, int Hout, int Wout, void *stream);
/* [flow_vis-ext, unpinned] flow_vis.flow_to_color(flow_uv, convert_to_bgr=bgr) of predict_new_data.py:155,:158 (no clip_flow),
 * restated from memory in kernels/frames.h: the Middlebury colour wheel (55 colours), hue from the direction, saturation from
 * |flow| / (rad_max + 1e-5), in fp32.  flow: (N,2,H,W) in network order (channel 0 = dy); rgb: (N,H,W,3) uint8, channels reversed
 * with bgr != 0.  rad_max >= 0: the scale of every image (one scale for a video); rad_max < 0: each image's own maximum of
 * sqrtf(u*u + v*v) over its finite values, found through the workspace in a fixed order; NaN: MFN_E_PARAM.  A pixel whose flow is
 * not finite is written (0,0,0).  The workspace is asked for in both forms. */
size_t mfn_flow_color_workspace_bytes(int N, int H, int W);
int mfn_flow_color(const float *flow, unsigned char *rgb, int N, int H, int W, float rad_max, int bgr, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Augmentation of the training batch -- replace the device side of the two augmenters that
 * /root/reference/network/pipeline.py:100-101 applies before every step: GeometryAugmentation
 * (/root/reference/augmentation.py:229-339) and ColorAugmentation (:168-227).  The per-sample scalars are drawn on the host
 * (maskflownet_amd/augment.py) and reach the kernels as one small fp32 table per call; maskflownet_amd/csrc/kernels/augment.h
 * names the table offsets and spells out every fp32 expression in evaluation order (fp contraction off). */
/* augmentation.py:295-338 in one launch, per target pixel: both affine grids (never stored), the clip of the first, the bilinear
 * samples of img1 | mask | (flow - shift) * mask through the first and of img2 through the second, flow / max(mask, 1e-8), the
 * 2x2 re-projection and the grid term.  img1, img2: (N,3,Ho,Wo); flow: (N,2,Ho,Wo) as (u, v); mask: (N,1,Ho,Wo) with
 * mask_is_plane != 0, else (N,1,1,1) read as a constant plane; table: (N,26).  out1, out2: (N,3,Ht,Wt); flow_out: (N,2,Ht,Wt), written
 * as (v, u) = (dy, dx) with label_order = 1 (pipeline.py:105); mask_out: (N,1,Ht,Wt).  Ht, Wt >= 2, else MFN_E_SHAPE. */
int mfn_augment_geometry(const float *img1, const float *img2, const float *flow, const float *mask, int mask_is_plane,
                         const float *table, float *out1, float *out2, float *flow_out, float *mask_out, int N, int Ho, int Wo,
                         int Ht, int Wt, int label_order, void *stream);
/* F.mean of augmentation.py:216 for both images: mean[k,n,c] over the plane of a = M rgb + z * sigma (:213-215), M the
 * saturation / hue matrix of :198-200 from table (N,26), z the Philox4x32-10 normals of key `seed`, counter (pixel / 4,
 * (k N + n) 3 + c, offset) -- regenerated, never stored; sigma == 0 runs no generator.  mean: (2N,3).  Fixed summation order
 * through the caller's workspace as mfn_pair_mean: bit-identical from run to run, at most 46 additions per term. */
size_t mfn_augment_color_mean_workspace_bytes(int N, int H, int W);
int mfn_augment_color_mean(const float *img1, const float *img2, const float *table, float sigma, unsigned long long seed,
                           unsigned long long offset, float *mean, int N, int H, int W, void *workspace, size_t workspace_bytes,
                           void *stream);
/* augmentation.py:213-225 element-wise: a as above with the same seed and offset, (a - mean) * contrast * channel, the optional
 * 3x3 spin (eigen_aug, :220), + (mean * channel + brightness), clip(0, 1), the optional powf(., exp(gamma)) (:224).
 * out: (2N,3,H,W), images 1 in [0,N), images 2 in [N,2N): the network's input batch layout. */
int mfn_augment_color(const float *img1, const float *img2, const float *table, const float *mean, float sigma,
                      unsigned long long seed, unsigned long long offset, int use_spin, int use_gamma, float *out, int N, int H,
                      int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The multiscale training loss, fused -- replaces EpeLossWithMask and MultiscaleEpe(match='upsampling') of
 * /root/reference/network/MaskFlownet.py:563-611 as /root/reference/network/pipeline.py:42-44 builds them (eps 1e-8, q from
 * optimizer.q: None for the chairs / things schedules, 0.4 for Sintel and KITTI) and :82 calls them.  Per scale s of n_scales,
 * with factor f_s, weight w_s and prediction p_s (N,2,H/f_s,W/f_s):
 *   d = Upsample(f_s)(p_s) - label;   L = sqrt(d_y^2 + d_x^2 + eps),  or (|d_y| + |d_x| + eps)^q with robust != 0;
 *   sums[n,s] = sum_pix mask[n,pix] * L;   sums[n,n_scales] = msum[n] = sum mask[n];   loss[n] = sum_s w_s * sums[n,s] / msum[n].
 * label: (N,2,H,W); mask: (N,1,H,W), or with mask_is_scalar != 0 (N,1,1,1): msum[n] = mask[n], the numerator over all pixels (the
 * reference's broadcast).  msum == 0 gives that sample the reference's 0 / 0.  The upsampled value is recomputed per pixel with
 * mfn_upsample_fwd's own arithmetic (its bits) and never stored; kernels/loss.h spells out every expression (fp contraction off).
 * preds, factors, weights (and gpreds, reqs) are HOST arrays of n_scales <= MFN_LOSS_MAX_SCALES entries, copied by value into
 * the launches: no allocation, no synchronisation, capturable.  Fixed-order reductions through the caller's workspace, no
 * atomics: bit-identical from run to run, |sum - exact| <= 64 * 2^-24 * sum |terms|.
 * Errors before any launch: n_scales outside 1..8, a factor < 1, q <= 0 with robust (MFN_E_PARAM); H or W no multiple of a
 * factor (MFN_E_SHAPE); a NULL array or tensor (MFN_E_NULL); a missing or short workspace (MFN_E_WORKSPACE). */
#define MFN_LOSS_MAX_SCALES 8
size_t mfn_multiscale_epe_workspace_bytes(int N, int H, int W, int n_scales);
int mfn_multiscale_epe_fwd(const float *const *preds, const int *factors, const float *weights, int n_scales,
                           const float *label, const float *mask, int mask_is_scalar, float eps, int robust, float q,
                           float *loss, float *sums, int N, int H, int W, void *workspace, size_t workspace_bytes, void *stream);
/* Gradients of the predictions (none of label or mask): gpreds[s] (N,2,H/f_s,W/f_s) =
 *   gloss[n] * w_s / msum[n] * sum over the (2 f_s - 1)^2 footprint of k_y k_x * mask * dL/dd_c,
 * dL/dd_c = d_c / sqrt(..), or q * (..)^(q-1) * sign(d_c) with sign(0) = 0; d recomputed from preds and label, msum read from
 * the forward's sums (N, n_scales + 1).  reqs[s]: MFN_REQ_* per prediction (MFN_REQ_NULL: gpreds[s] may be NULL and is not
 * touched).  One launch per scale, owner computes, no atomics: bit-identical from run to run.  Pixels with mask == 0 add no
 * term: an input pixel whose whole footprint is masked out gets exactly 0. */
int mfn_multiscale_epe_bwd(const float *gloss, const float *const *preds, const int *factors, const float *weights, int n_scales,
                           const float *label, const float *mask, int mask_is_scalar, float eps, int robust, float q,
                           const float *sums, float *const *gpreds, const int *reqs, int N, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The trainer's Adam step -- replaces `self.trainer.step(batch_size)` of /root/reference/network/pipeline.py:114
 * for the trainer of :27, gluon.Trainer(params, 'adam', {'learning_rate': 1e-4}).  mfn_adam_update is MXNet 1.5's `adam_update`
 * operator (src/operator/optimizer_op-inl.h, AdamUpdate) with its own signature, in place on n fp32 elements:
 *   g  = rescale_grad * grad + wd * weight;   g = clip_gradient >= 0 ? clip(g, -clip_gradient, clip_gradient) : g;
 *   mean = beta1 * mean + (1 - beta1) * g;    var = beta2 * var + (1 - beta2) * g * g;
 *   weight = weight - lr * mean / (sqrt(var) + epsilon)
 * kernels/optimizer.h spells out the evaluation order (every operation rounded in fp32, fp contraction off).  The bias corrections
 * are the caller's, folded into lr as MXNet's Adam.update does: lr * sqrt(1 - beta2^t) / (1 - beta1^t).  NaN and inf propagate per
 * element.  Every element is owned by one thread: no atomics, no workspace, bit-identical from run to run.
 * Errors before any launch: n < 0 (MFN_E_SHAPE); a NULL pointer with n > 0 (MFN_E_NULL); beta1 or beta2 outside [0, 1),
 * epsilon < 0 (MFN_E_PARAM); a pointer that is not 4-byte aligned (MFN_E_ALIGN).  n == 0 succeeds without a launch. */
int mfn_adam_update(float *weight, const float *grad, float *mean, float *var, long long n, float lr, float beta1, float beta2,
                    float epsilon, float wd, float rescale_grad, float clip_gradient, void *stream);
/* All tensors of a step in ONE launch.  A table says where they are: per tensor the four pointers, the count, lr_mult and wd_mult (the
 * tensor's lr is lr * lr_mult, its wd wd * wd_mult; NULL arrays mean 1) and whether all four pointers are 16-byte aligned (such
 * tensors move 16 bytes per access, the others one element), then one entry per block of 4096 elements.  The two host-only entries
 * size and fill the table in a caller-owned HOST buffer (8-byte aligned) from HOST arrays of DEVICE pointers; the caller uploads the
 * bytes as they are: the library allocates nothing and synchronises nothing.  mfn_multi_adam_build_table returns the launch's block
 * count and a layout tag; mfn_multi_adam_update refuses a tag or byte count that does not fit n_tensors and n_blocks
 * (MFN_E_WORKSPACE).  A tensor whose address or size changed needs a new table.  counts[i] == 0 is allowed (its pointers may be
 * NULL); a negative count is MFN_E_SHAPE, a NULL pointer of a non-empty tensor MFN_E_NULL.  mfn_multi_adam_table_bytes returns 0
 * for arguments the builder refuses.  n_tensors == 0 succeeds without a launch. */
size_t mfn_multi_adam_table_bytes(int n_tensors, const long long *counts);
int mfn_multi_adam_build_table(int n_tensors, float *const *weights, const float *const *grads, float *const *means,
                               float *const *vars, const long long *counts, const float *lr_mults, const float *wd_mults,
                               void *table_host, size_t table_bytes, int *n_blocks, unsigned long long *tag);
int mfn_multi_adam_update(const void *table_dev, size_t table_bytes, unsigned long long tag, int n_tensors, int n_blocks, float lr,
                          float beta1, float beta2, float epsilon, float wd, float rescale_grad, float clip_gradient, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One training batch cut out of a device-resident data set -- replaces what iterate_data and batch_samples
 * of the reference's main.py:466-486 do to the N samples of a batch on the host (crop, HWC -> CHW, the reversed W axis with the
 * negated first label channel, np.stack) and the upload of the result.  One launch, the same bytes:
 *   out[n, c, y, x] = src_n[y0_n + y, x0_n + (flip_n ? Wc - 1 - x : x), c]
 * Sources per slot n, HWC and contiguous: img1, img2 uint8 (Hs,Ws,3); flow (Hs,Ws,2), fp32 (label_type 0) or fp16 (1, widened
 * exactly); mask uint8 (Hs,Ws,1) or NULL.  Sizes, crop origin, flip and label type are per slot.  Outputs, contiguous NCHW:
 * img1, img2 (N,3,Hc,Wc) uint8; label (N,2,Hc,Wc) fp32 in the readers' (u, v) order, channel 0 with its sign bit flipped where
 * flip is set (+0.0 -> -0.0); mask (N,1,Hc,Wc) uint8 when with_mask != 0 -- a slot whose mask is NULL writes 255 -- and not
 * touched (may be NULL) otherwise.
 * READ CONTRACT: every source array starts at a 16-byte aligned address and is readable up to the next multiple of 16 bytes of
 * its size; the kernel reads aligned words inside that extent and nothing outside it.
 * mfn_batch_gather_build_rows checks the slots and fills a caller-owned HOST table (8-byte aligned, mfn_batch_gather_rows_bytes(N)
 * bytes: 64 per slot) from HOST arrays of DEVICE addresses (`mask` may be NULL: no slot has one); the caller uploads the bytes as
 * they are, once per step: the library allocates nothing and synchronises nothing.  The tag binds the table to (N, Hc, Wc).
 * Errors before any launch: a NULL required pointer or array, a NULL img1 / img2 / flow of a slot (MFN_E_NULL); N, Hc, Wc, Hs or
 * Ws <= 0, a crop that leaves its source (y0 < 0, y0 + Hc > Hs, x0 < 0, x0 + Wc > Ws), a table byte count or tag that does not
 * fit (MFN_E_SHAPE); a source address that is not 16-byte aligned, an output tensor that is not 4-byte aligned, a table that is
 * not 8-byte aligned (MFN_E_ALIGN); a label type other than 0 / 1, a flip other than 0 / 1 (MFN_E_PARAM); N > 65535 or
 * Hc * Wc >= 2^31 (MFN_E_UNSUPPORTED).  mfn_batch_gather_rows_bytes returns 0 for N <= 0. */
size_t mfn_batch_gather_rows_bytes(int N);
int mfn_batch_gather_build_rows(int N, const void *const *img1, const void *const *img2, const void *const *flow,
                                const void *const *mask, const int *Hs, const int *Ws, const int *label_type, const int *y0,
                                const int *x0, const int *flip, int Hc, int Wc, void *rows_host, size_t rows_bytes,
                                unsigned long long *tag);
int mfn_batch_gather(const void *rows_dev, size_t rows_bytes, unsigned long long tag, int N, int Hc, int Wc, int with_mask,
                     unsigned char *img1, unsigned char *img2, float *label, unsigned char *mask, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A validation batch read where the data set lies -- replaces what PipelineFlownet.validate of
 * /root/reference/network/pipeline.py:149-187 does to a batch on the host around the network, and its uploads, for samples that are
 * resident on the device as the readers store them.  rows_dev: N rows of a table made by mfn_batch_gather_build_rows, on the device
 * (a window of a longer table is the address of its first row: rows are 64 bytes).  Every slot is the whole H x W sample: the caller
 * has checked Hs == H, Ws == W, y0 == x0 == 0 and flip == 0 on its host copy; the kernels read the pointers and the label type only.
 * READ CONTRACT: that of mfn_batch_gather.  kernels/validate.h names, for each entry, the operator whose bits it gives.
 * Errors before any launch: a NULL table or tensor (MFN_E_NULL); N < 0, H, W, Hout or Wout < 1 (MFN_E_PARAM); a missing or short
 * workspace (MFN_E_WORKSPACE); a table that is not 8-byte aligned, a float pointer that is not 4-byte aligned (MFN_E_ALIGN);
 * N > 32767 or a sample of 2^31 bytes (MFN_E_UNSUPPORTED).  N == 0 succeeds and touches nothing. */
/* rgb_mean of pipeline.py:86 on the bytes / 255 of :208 for the N slots' (img1, img2): exact integer sums, mean (N,3); the bits of
 * mfn_pair_mean_u8 on the same bytes. */
size_t mfn_val_pair_mean_workspace_bytes(int N, int H, int W);
int mfn_val_pair_mean(const void *rows_dev, int N, int H, int W, float *mean, void *workspace, size_t workspace_bytes, void *stream);
/* pipeline.py:208 (`/ 255`, HWC -> CHW), :120 and :129-130 in one launch: out (2N,3,Hout,Wout), image 1 of slot n in row n, image 2
 * in row N + n; mean_or_null (N,3), NULL subtracts nothing; Hout == H and Wout == W unpacks.  The bits of mfn_preprocess_pair_u8 on
 * the same bytes. */
int mfn_val_preprocess(const void *rows_dev, int N, int H, int W, const float *mean_or_null, float *out, int Hout, int Wout,
                       void *stream);
/* pipeline.py:175-176 and :146, :182: the sums of mfn_flow_metrics, (N,3), of flow (N,2,H,W) in network order (channel 0 = dy)
 * against each slot's stored HWC (u, v) label -- fp32, or fp16 widened exactly; channel 0 of the network order is the stored v -- under
 * its mask (float)byte / 255.f, 1.f for a slot without one.  The reduction is mfn_flow_metrics's: the bits of that entry on the
 * label and mask materialised as fp32 tensors. */
size_t mfn_val_flow_metrics_workspace_bytes(int N, int H, int W);
int mfn_val_flow_metrics(const void *rows_dev, const float *flow, int N, int H, int W, float *sums, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Raw decoded KITTI / HD1K arrays turned into stored samples -- replaces what the reference's readers do to
 * every sample at load time on the host with cv2: /root/reference/reader/kitti.py:57-74 and reader/hd1k.py:51-78 (crop, HD1K's
 * min/max stretch, cv2.resize of the images, bilinear resize of flow and validity, flow re-scaling, the division by the resized
 * validity, mask quantisation), and cv2.resize of the test images (kitti.py:105-106).  kernels/ingest.h spells out every expression.
 * Every entry reads a WINDOW (y0, x0, h, w) of an (H, W, 3) array with `pitch` elements per row (pitch >= 3 W).
 * READ CONTRACT: the array starts at a 16-byte aligned address and is readable up to the next multiple of 16 bytes of its size;
 * nothing outside that extent is touched.  Outputs are dense and 16-byte aligned.
 * The resampling is OpenCV's INTER_LINEAR (half-pixel centres, edge replicate, no antialiasing) restated from its generic path; its
 * positions and coefficients come from tables that the host-only entry below fills in a caller-owned HOST buffer (8-byte aligned,
 * 32 bytes per destination column and row) for one (window size, destination size); the caller uploads the bytes as they are
 * (16-byte aligned on the device), once per pair of sizes.  The tag binds the tables to the four sizes; an entry refuses tables
 * whose byte count or tag does not fit its own sizes (MFN_E_SHAPE).
 * Errors before any launch: a NULL array, output or table (MFN_E_NULL); a size < 1, a pitch below 3 W, a window that leaves its
 * array, a flow window with a side < 2 -- the reference's flow scale is x / 0 there -- (MFN_E_SHAPE); an address that is not
 * aligned as stated (MFN_E_ALIGN); bgr, premultiply or flow_type outside their values (MFN_E_PARAM). */
size_t mfn_ingest_tables_bytes(int dst_h, int dst_w);
int mfn_ingest_build_tables(int src_h, int src_w, int dst_h, int dst_w, void *tables_host, size_t tables_bytes,
                            unsigned long long *tag);
/* hd1k.py:55: minmax[0] = the minimum, minmax[1] = the maximum over both windows, all channels.  Two launches (the words' initial
 * values, then per-block reductions folded in with vector atomicMin / atomicMax): no workspace, no synchronisation. */
int mfn_ingest_minmax(const unsigned char *img1, const unsigned char *img2, int H, int W, long long pitch, int y0, int x0, int h,
                      int w, unsigned *minmax, void *stream);
/* uint8 window -> dst (dst_h, dst_w, 3) uint8: the channels reversed with bgr != 0 (cv2.imread's order, kitti.py:54), then with
 * minmax_or_null != NULL hd1k.py:56's stretch uint8((v - min) * (255.0 / (max - min))) in double (min == max, where the reference
 * divides by zero, gives 0), then cv2.resize's fixed-point bilinear (kitti.py:66).  At equal sizes: the source bytes. */
int mfn_ingest_image(const unsigned char *src, int H, int W, long long pitch, int y0, int x0, int h, int w, const void *tables_dev,
                     size_t tables_bytes, unsigned long long tag, int bgr, const unsigned *minmax_or_null, unsigned char *dst,
                     int dst_h, int dst_w, void *stream);
/* uint16 window in the file's channel order (R = u, G = v, B = valid) -> flow (dst_h, dst_w, 2) in (u, v) order, fp32
 * (flow_type 0) or fp16 (1: round to nearest even), and mask (dst_h, dst_w, 1) uint8: kitti.py:61-72, with premultiply != 0
 * hd1k.py:57-76.  At equal sizes the readers' resize=None branch. */
int mfn_ingest_flow_occ(const unsigned short *src, int H, int W, long long pitch, int y0, int x0, int h, int w,
                        const void *tables_dev, size_t tables_bytes, unsigned long long tag, int premultiply, int flow_type,
                        void *flow, unsigned char *mask, int dst_h, int dst_w, void *stream);
/* Host code, no GPU: reverses the five row filters of a PNG image in place (what cv2.imread of kitti.py:54-56 and skimage.io.imread
 * of reader/sintel.py:79 do inside libpng).  raw: `rows` scanlines of 1 + row_bytes bytes as inflated, the filter type first;
 * bytes_per_pixel: 1..8.  A filter type above 4: MFN_E_PARAM. */
int mfn_png_unfilter(unsigned char *raw, long long rows, long long row_bytes, int bytes_per_pixel);

/* ---------------------------------------------------------------------------------------------
 * Convolution / Deconvolution -- replace the Gluon blocks of
 * /root/reference/network/MaskFlownet.py:79-163: nn.Conv2D(channels, kernel_size=3, strides, padding, dilation)
 * [+ LeakyReLU(0.1)] of conv() / predict_flow() / predict_mask() (:165-191) and nn.Conv2DTranspose(channels, 4, 2, 1)
 * [+ LeakyReLU(0.1)] of deconv() (:175-183), i.e. MXNet's Convolution / Deconvolution operators:
 *   Convolution:   out[n,o,y,x] = b[o] + sum_{c,i,j} w[o,c,i,j] * x[n,c, y*sh-ph+i*dh, x*sw-pw+j*dw]      (zero outside)
 *   Deconvolution: out[n,o,y,x] = b[o] + sum_{c,i,j} w[c,o,i,j] * x[n,c,(y+ph-i*dh)/sh,(x+pw-j*dw)/sw]   (exact divisions only)
 * x: (N,Cin,H,W); w: (Cout,Cin/groups,kh,kw), transposed: (Cin,Cout/groups,kh,kw); out: (N,Cout,Ho,Wo) from
 * mfn_conv2d_out_shape.  3x3 convolutions and 4x4 transposed convolutions with groups == 1 run fused gather + matrix-core
 * implicit GEMM kernels (no im2col buffer; arithmetic per mfn_set_arithmetic("convolution", ..): the default is fp32-EQUIVALENT --
 * operands as three bf16 terms, see "Arithmetic" --, MFN_ARITH_FP32 the bit-exact fp32 MFMA chain); every other parameter set
 * runs a generic kernel.
 * activation: MFN_ACT_NONE | MFN_ACT_LEAKY_0_1 (fused, bit-identical to the separate elementwise op).
 * out_batch_stride / in_batch_stride: elements between consecutive output / input images (0 = dense): a layer writes
 * straight into its channel slice of the decoder's concat buffer and the next layer reads the buffer's channel suffix
 * (x = concat(conv(x), x), MaskFlownet.py:219-223) -- no concat copies.
 * Weights: give `w` (re-laid-out into `workspace` on every call, mfn_conv2d_workspace_bytes) or a buffer made once by
 * mfn_conv2d_pack_weights + its layout tag (mfn_conv2d_packed_weight_bytes; a tag that does not match the plan of the
 * current shape / tuning is refused, never silently used).  3x3 / stride 1 / pad 1 layers with >= 32 filters on large images are
 * packed for the deformable convolution's matrix-core kernel (kernels/deform_conv_mma.h, CONV form): a call with such a buffer needs
 * x and out 16-byte aligned and batch strides that are multiples of 4 elements (MFN_E_ALIGN otherwise; a call that gives `w` picks
 * the other kernel by itself).  mfn_conv2d_workspace_bytes takes no adj: for a transposed call its answer suffices for every adj
 * the call accepts (adj_h < sh, adj_w < sw; the kernel family depends on adj).
 * ------------------------------------------------------------------------------------------- */
int mfn_conv2d_out_shape(int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int transposed,
                         int adj_h, int adj_w, int *Ho, int *Wo);
size_t mfn_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph,
                                  int pw, int dh, int dw, int groups, int transposed);
size_t mfn_conv2d_packed_weight_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph,
                                      int pw, int dh, int dw, int groups, int transposed);
int mfn_conv2d_pack_weights(const float *w, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw,
                            int ph, int pw, int dh, int dw, int groups, int transposed, void *packed,
                            size_t packed_bytes, unsigned long long *layout_tag, void *stream);
int mfn_conv2d_fwd(const float *x, long long in_batch_stride, const float *w_or_null, const void *packed_or_null,
                   size_t packed_bytes, unsigned long long layout_tag, const float *bias_or_null, float *out,
                   long long out_batch_stride, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                   int dw, int groups, int transposed, int adj_h, int adj_w, int activation, void *workspace,
                   size_t workspace_bytes, void *stream);

/* Backward of mfn_conv2d_fwd (num_group == 1): what autograd runs for the Conv2D / Conv2DTranspose blocks of
 * /root/reference/network/MaskFlownet.py:79-163 in network/pipeline.py:112-113.  gout: (N,Cout,Ho,Wo); y: the forward output
 * (only read when activation = MFN_ACT_LEAKY_0_1, NULL otherwise); gx: (N,Cin,H,W); gw: the weight's own layout; gbias: (Cout).
 * req_*: MFN_REQ_NULL / WRITE / ADD per gradient.  workspace: mfn_conv2d_bwd_workspace_bytes (16-byte aligned).
 * The weight gradient runs on the deformable convolution's weight-gradient kernels with zero offsets; where those sum
 * through fp32 atomics (filters > 96 per call or widths that are no multiple of 4) its last bits vary from run to run. */
size_t mfn_conv2d_bwd_workspace_bytes(int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph,
                                      int pw, int dh, int dw, int groups, int transposed, int adj_h, int adj_w,
                                      int activation);
int mfn_conv2d_bwd(const float *gout, const float *x, const float *w, const float *y_or_null, float *gx, float *gw,
                   float *gbias, int N, int Cin, int H, int W, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                   int dh, int dw, int groups, int transposed, int adj_h, int adj_w, int activation, int req_x, int req_w,
                   int req_bias, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Stream plumbing for the host side (no reference equivalent: MXNet's engine does this).
 * A hot-path pass is ~10 short launches; capturing it once into a hipGraph and replaying it
 * removes the per-launch host cost.  Capture is plain hipStreamBeginCapture on `stream`.
 * ------------------------------------------------------------------------------------------- */
int mfn_graph_begin_capture(void *stream);
int mfn_graph_end_capture(void *stream, void **graph_exec_out);
int mfn_graph_launch(void *graph_exec, void *stream);
int mfn_graph_destroy(void *graph_exec);

/* Built-in kernel timer: while enabled, every launch made by this library on this thread is
 * bracketed by HIP events on ITS OWN stream (hipExtLaunchKernelGGL start/stop events) and
 * accumulated per kernel name.  Used by bench.py for the roofline line. */
int mfn_profile_enable(int on);
int mfn_profile_reset(void);
/* Records taken until the next call carry the suffix "@tag" (NULL / "" clears it): tells the launches of one operator
 * call apart inside a fully profiled pass. */
int mfn_profile_tag(const char *tag);
/* Synchronises the recorded events, then reports launches and summed milliseconds of every
 * kernel whose name contains `name_substr`.  Returns the number of matching launches. */
int mfn_profile_query(const char *name_substr, int *launches, double *total_ms);
/* Writes up to `cap` bytes of "name launches total_ms\n" lines into buf; returns bytes needed. */
int mfn_profile_dump(char *buf, int cap);

/* ---------------------------------------------------------------------------------------------
 * Arithmetic.  The three GEMM-shaped operators (Correlation, DeformableConvolution, Convolution / Deconvolution) exist in
 * two arithmetics; which one a call uses is ONE setting per process (atomic; default compiled in) that every thread's calls read --
 * the thread that launches a kernel is often not the one that chose: torch runs backward on its autograd thread, MXNet runs every
 * CustomOp on worker threads.  Set it before the calls it should govern; it is not one of the measurement knobs below:
 *   MFN_ARITH_DEFAULT  the library's choice: the bf16 x 3 matrix-core kernels wherever one exists for the call's shape
 *                      (level shapes of the network), the fp32 kernels elsewhere.
 *   MFN_ARITH_FP32     fp32 FMA chains everywhere (v_fma_f32 / v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32): the accumulation order of an fp32
 *                      inner product, bit-reproducible against itself across tilings of K only within one kernel.
 *   MFN_ARITH_BF16X3   as the default.
 * bf16 x 3: every fp32 operand is written exactly as hi + mid + lo with three bf16 terms (24 significant bits) and SIX of the
 * nine partial products -- those of weight >= 2^-16 -- are accumulated in fp32 by v_mfma_f32_*_bf16.  I/O stays fp32.  The
 * dropped products are <= 2^-24 of a product each (~1 ulp per product, not per sum).  The acceptance rule is asserted per ELEMENT
 * in tests/test_forward_fp64.py and tests/test_backward_fp64.py (parity_cases.check_fp64_bound): with M the sum of the absolute
 * values of the terms an element is made of, "max |got - fp64| / M within 4 x the fp32 oracle's on the same input + 16 * 2^-24,
 * and exactly 0 where no term exists", on plain and on graded inputs (pixels and channels six orders of magnitude apart), per kernel
 * and arithmetic.  tests/test_gpu_parity.py keeps the per-TENSOR form: "maximum error against the fp64 oracle within 1.25 x
 * (deformable convolution) / 1.5 x (cost volumes) / 2 x (convolutions) of the fp32 kernel's on the same input, and <= 1e-5 of
 * max|ref|" (observed: 0.7-1.1 x).  It is
 * fp32-EQUIVALENT, not the bit pattern of an FMA chain.  Divergence on non-finite inputs: an +-inf operand splits into
 * inf + NaN (inf - bf16(inf)), so outputs that an FMA chain would make +-inf come back NaN; NaN inputs give NaN either way;
 * values beyond bf16's range do not exist (bf16 has fp32's exponent); fp32 denormal operands lose their low terms (flushed), an
 * absolute error below 2^-126 per product.  Which OUTPUTS a non-finite input pixel reaches: under the default arithmetic the
 * deformable convolution's taps outside the image read zeros, so exactly the outputs whose valid taps touch the pixel (MXNet's
 * set); the fp32 kernel (MFN_ARITH_FP32, dc_lds_kernel) multiplies border-clamped reads by zero weights, so a non-finite pixel
 * within three rows / columns of the border also poisons neighbouring outputs whose taps fall outside the image
 * (tests/test_gpu_parity.py::test_deform_numeric_range_edge_cases).
 * Layouts packed by mfn_deform_conv_pack_weights / mfn_conv2d_pack_weights depend on the arithmetic in force when they were packed;
 * a call under another arithmetic refuses them (layout tag) instead of misreading them.
 * Like mfn_set_tuning, mfn_set_arithmetic must not race with calls in flight: a call is planned from one reading of the settings,
 * but a size query and the run that follows it are two readings.
 * op: "correlation" | "deformable_convolution" | "convolution" | "all".  Unknown op / mode: MFN_E_PARAM. */
#define MFN_ARITH_DEFAULT (-1)
#define MFN_ARITH_FP32 0
#define MFN_ARITH_BF16X3 1
int mfn_set_arithmetic(const char *op, int mode);
int mfn_get_arithmetic(const char *op, int *mode);

/* Kernel-selection knobs for tuning sweeps: tilings and code paths only, never arithmetic (process-global, NOT thread-safe,
 * not part of the drop-in surface: set them before the first operator call or while no other thread is inside the library).
 * Unknown keys return MFN_E_PARAM.  Keys: see maskflownet_amd/csrc/tuning.h. */
/* Measurement only: when non-NULL, instrumented kernels write 4 x uint64 wall-clock stamps (100 MHz)
 * per workgroup into this device buffer (caller sizes it: 32 bytes x workgroups). */
int mfn_debug_set_timeline(void *device_buffer);
/* Measurement and tests only: the tiling the calling thread's last deformable-convolution launch on dc_mma_kernel was planned with --
 * filter tiles per wave, pixel tiles per block, K slices, and whether the weight operand went from memory to registers (the AREG
 * form, 1) or through LDS (0).  All zero before the first such launch.  Any pointer may be NULL. */
int mfn_debug_last_dc_plan(int *mt, int *pt, int *kw, int *areg);
int mfn_set_tuning(const char *key, int value);
int mfn_get_tuning(const char *key, int *value);

#ifdef __cplusplus
}
#endif
#endif /* MFN_HIP_H */
