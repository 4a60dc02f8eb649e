/* ctgan_hip.h - C-ABI of libctgan_hip.so: the MI355X (gfx950) kernels behind the CT-WGAN
 * adversarial step of biuyq/CT-GAN.
 *
 * The reference has no native code and no FFI: its operator library (the tflib/ops modules) bottoms out
 * in TensorFlow-1.2.1 graph nodes.  Each entry point below replaces one of those TF call sites
 * (cited per function; TF/ = CT-GANs/tensorflow_generative_model/).  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - All tensors are fp32 unless stated; activations are logically NCHW like the reference but
 *    described with explicit element strides, so the physical layout may be NHWC (channels-last,
 *    what the fast kernels want) or NCHW (image inputs / sample outputs).
 *  - The library never allocates or frees caller-visible memory; workspaces are caller-provided
 *    (size from ctgan_conv2d_workspace_bytes).
 *  - Every call is asynchronous on the caller's hipStream_t (`stream`, passed as void*); no
 *    internal device synchronisation; safe under hipGraph stream capture.
 *  - Return 0 on success, negative CTGAN_E_* on failure; ctgan_last_error() gives a thread-local
 *    message.  No C++ exception crosses the ABI.
 */
#ifndef CTGAN_HIP_H
#define CTGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTGAN_OK 0
#define CTGAN_E_BADARG (-1)
#define CTGAN_E_UNSUPPORTED (-2)
#define CTGAN_E_LAUNCH (-3)

#define CTGAN_ABI_VERSION 1

typedef void* ctgan_stream_t; /* hipStream_t */

/* Geometry of one TF 'SAME' convolution  y[n,k,p,q] = sum_{r,s,c} x[n,c,p*stride-pad_t+r,
 * q*stride-pad_l+s] * w[r,s,c,k]  (w is HWIO, contiguous: tflib `name.Filters`).
 * The same descriptor drives the forward op, its data gradient and its weight gradient.
 * A Deconv2D is described by the descriptor of the strided conv it is the adjoint of
 * (x side = the large / output side of the deconv). */
typedef struct ctgan_conv_desc {
    int32_t N, C, H, W;   /* x: batch, channels, height, width                                */
    int32_t K, R, S;      /* y channels, filter height, filter width                           */
    int32_t P, Q;         /* y height, width ( = ceil(H/stride), ceil(W/stride) under SAME )   */
    int32_t stride;       /* 1 or 2                                                            */
    int32_t pad_t, pad_l; /* leading SAME pads (trailing pads are implied by P,Q)              */
    int32_t x_up;         /* 1: x is read through a nearest-neighbour 2x upsample (H,W are the */
                          /*    upsampled sizes; the physical tensor is H/2 x W/2)  (K10)      */
    int32_t reserved;
    int64_t xs[4];        /* x element strides for (n, c, h, w)                                */
    int64_t ys[4];        /* y element strides for (n, k, p, q)                                */
} ctgan_conv_desc;

enum { CTGAN_CONV_FWD = 0, CTGAN_CONV_DGRAD = 1, CTGAN_CONV_WGRAD = 2 };
enum { CTGAN_EPI_RELU = 1, CTGAN_IN_RELU = 2,    /* relu on the result / on the gathered input (conv(relu(x))) */
       CTGAN_RESID_UP = 8 };                      /* fwd: `resid` is the dense channels-last [N,K,P/2,Q/2] tensor and is added
                                                    * through a nearest-2x upsample (UpsampleConv shortcut, :100-107,130) */
enum { CTGAN_DGRAD_W_REPACKED = 1 };

/* ---- library ------------------------------------------------------------------------------ */
int ctgan_version(void);
const char* ctgan_last_error(void);
/* which kernel variant the last conv call on this thread dispatched to (for tests/profiles)   */
const char* ctgan_last_kernel(void);
/* ... and its device symbol as rocprofv3 prints it (e.g. "conv16_kernel<3, 2, 2, 32, false, false>"); the variant name when the
   launcher does not record one.  bench.py keys its per-kernel roofline table by it (cross-checked against profiles/).            */
const char* ctgan_last_symbol(void);
/* (test / A-B switches and launch introspection live in ctgan_hip_debug.h - not part of this ABI)                              */

/* Optional epilogue extension of ctgan_conv2d_fwd / ctgan_conv2d_dgrad: tf.nn.dropout (:173-177) applied to the
 * RESULT inside the kernel, y *= floor(keep + u)/keep, where u is what ctgan_rng_uniform(.., seed, stream_id, ctr)
 * writes at the same physical offset (i.e. exactly ctgan_dropout_rng of the result, without the extra pass).  The
 * forward uses it for a dropout that follows a conv; the backward for the dropout mask a data gradient is multiplied
 * with.  drop_keep outside (0,1) = no dropout.  CTGAN_E_UNSUPPORTED unless the pipelined kernel with the 16-B
 * epilogue serves the call (caller then applies ctgan_dropout_rng itself).
 * Row ranges (forward only, dense channels-last result): n_ranges > 0 splits the batch into consecutive sample ranges
 * [0, range_end[0]), [range_end[0], range_end[1]), ... each with its own keep probability (outside (0,1) = none) and
 * stream id, the draws indexed from the range's first element - exactly the dropout each range would get as a tensor of
 * its own.  Lets several passes that use the same weights (dropout passes, clean pass, gradient-penalty pass) share one
 * launch per layer.                                                                                                      */
#define CTGAN_DROP_RANGES 3
typedef struct ctgan_epilogue_ext {
    float drop_keep;
    uint64_t drop_seed, drop_stream_id;
    const uint64_t* drop_ctr;
    int32_t n_ranges;
    int32_t range_end[CTGAN_DROP_RANGES];
    float range_keep[CTGAN_DROP_RANGES];
    uint64_t range_stream_id[CTGAN_DROP_RANGES];
    /* forward only (ctgan_conv2d_fwd, ctgan_conv2d16_fwd): the result is kept only where out_mask > 0 (strides of y; after the
     * bias, before resid - the order of the dgrad epilogue's mask).  Used by the double backward of the gradient penalty, where the
     * conv that follows multiplies its input with a constant ReLU mask (TF/CT_gan_cifar_resnet.py:284-286 through :109-141).  NULL = none. */
    const float* out_mask;
    /* 16-bit slice kernels only (ctgan_conv2d16_fwd / ctgan_conv2d16_dgrad, mma = CTGAN_MMA_BF16 / CTGAN_MMA_F16, dense channels-last
     * result): act = 1 applies the LeakyReLU + dropout pair of the DCGAN critics (TF/CT_gan_cifar.py:86-98, TF/CT_gan_mnist.py:94-106:
     * tf.nn.dropout(LeakyReLU(conv))) to the result r after bias / mask / resid / relu:
     *     out = r * (ref > 0 ? 1 : act_alpha) * floor(keep + u) / keep,   ref = act_ref ? act_ref[same offset] : r
     * with keep / Philox stream from drop_keep / drop_stream_id or, with n_ranges > 0, from the sample range of the row (draws indexed
     * from the range's first element) - bit for bit ctgan_lrelu_dropout_rng(2) run on the plain result.  act_ref = the forward result
     * gives the pair's backward (the data gradient's epilogue) and its application to a cotangent (the penalty's double backward).      */
    int32_t act;
    float act_alpha;
    const float* act_ref;
    /* ctgan_conv2d_fwd, many -> few convs on the one-pixel-per-lane kernel only (3x3, <= 4 output channels, 32-pixel rows; the generator's
     * output stage tanh(Conv2D(relu(Batchnorm(h)))), TF/CT_gan_cifar_resnet.py:164-166, evaluated without a tape): training-mode batch norm of
     * the INPUT applied while it is staged - x' = (x - in_bn_mean[g][c]) * in_bn_rstd[g][c] * in_bn_scale[c] + in_bn_offset[c], g = sample /
     * (N / in_bn_groups), then CTGAN_IN_RELU if set; the SAME zero padding stays zero - and out_tanh: tanh of the result.  The arithmetic of
     * ctgan_bn_apply followed by the conv and ctgan_tanh_fwd.  in_bn_mean == NULL and out_tanh == 0: off.                                   */
    const float* in_bn_mean;
    const float* in_bn_rstd;
    const float* in_bn_scale;
    const float* in_bn_offset;
    int32_t in_bn_groups;
    int32_t out_tanh;
    /* ... and on ctgan_conv2d16_fwd (mma = CTGAN_MMA_F32X3, stride 1, launches the fragment-streaming halo kernel takes with tiles inside one image,
     * CTGAN_IN_RELU set): the same batch norm while the halo patch is staged - the generator's Conv2 layers (TF/CT_gan_cifar_resnet.py:134-141) without
     * a tape.  in_bn_labels (int32 per sample, or NULL): conditional batch norm - in_bn_scale / in_bn_offset are [n_labels][C] tables.  */
    const int32_t* in_bn_labels;
} ctgan_epilogue_ext;
/* Weight gradient of ONE filter over several (x, dy) pairs of the same geometry and strides (the uses of the filter in
 * different passes of a step: the dropout passes and the gradient-penalty double backward,
 * TF/CT_gan_cifar_resnet.py:284,335-336 sum them in tf.gradients): dw = sum_s wgrad(xs[s], dys[s]) in one launch + one
 * fixed-order reduction.  d->N is ignored (Ns[s] rows per segment); seg_flags[s] = CTGAN_IN_RELU (x -> relu(x)) |
 * CTGAN_WGRAD_SEG_BIAS (dys[s] contributes to db).  Returns CTGAN_E_UNSUPPORTED for shapes outside the pipelined
 * kernel (caller falls back to ctgan_conv2d_wgrad per segment).                                               */
#define CTGAN_WGRAD_MAX_SEGS 3
#define CTGAN_WGRAD_SEG_BIAS 4
size_t ctgan_conv2d_wgrad_multi_workspace_bytes(const ctgan_conv_desc* d, int32_t nseg, const int32_t* Ns);
int ctgan_conv2d_wgrad_multi(const ctgan_conv_desc* d, int32_t nseg, const float* const* xs, const float* const* dys,
                             const int32_t* Ns, const int32_t* seg_flags, float* dw, float* db, void* ws,
                             size_t ws_bytes, ctgan_stream_t stream);
/* Several such weight gradients (different filters / geometries) at once: the deferred weight gradients of a step are
 * independent of each other, so they share ONE launch per tile configuration (workgroup -> problem table in the kernel
 * arguments, at most CTGAN_WGRAD_GROUP_MAX problems per launch) and ONE launch for all their split-K reductions.
 * Validates every group before the first launch: CTGAN_E_UNSUPPORTED means nothing ran (fall back per group).   */
#define CTGAN_WGRAD_GROUP_MAX 8      /* problems per grouped kernel launch */
#define CTGAN_WGRAD_GROUP_LIMIT 32   /* groups per call */
#define CTGAN_REDUCE_BATCH 16        /* reductions per launch */
typedef struct ctgan_wgrad_group {
    ctgan_conv_desc d;               /* d.N ignored, as in ctgan_conv2d_wgrad_multi */
    int32_t nseg;
    int32_t Ns[CTGAN_WGRAD_MAX_SEGS];
    int32_t seg_flags[CTGAN_WGRAD_MAX_SEGS];
    const float* xs[CTGAN_WGRAD_MAX_SEGS];
    const float* dys[CTGAN_WGRAD_MAX_SEGS];
    float* dw;
    float* db;                       /* NULL unless a segment carries CTGAN_WGRAD_SEG_BIAS */
    /* optional finished addends (grouped launch only): dw = (sum over segments) + add_dw, db likewise - the weight gradient another
       launch already produced for the same filter.  May alias dw / db (in-place accumulation).  add_db is ignored when db is NULL. */
    const float* add_dw;
    const float* add_db;
} ctgan_wgrad_group;
/* phases = CTGAN_WGRAD_GROUP_GEMM | CTGAN_WGRAD_GROUP_REDUCE for the whole call, or the two phases of the grouped launch separately
   (bench.py times the GEMM launches alone, as rocprofv3 reports them): the grouped weight-gradient kernels write the split-K slabs, the
   batched reduction sums them into dw / db in a fixed order.                                                                    */
enum { CTGAN_WGRAD_GROUP_GEMM = 1, CTGAN_WGRAD_GROUP_REDUCE = 2,
       /* optional: restrict the GEMM phase to the launch of one tile configuration (bit CTGAN_WGRAD_GROUP_TILE0 << t, t = 0..3) */
       CTGAN_WGRAD_GROUP_TILE0 = 16, CTGAN_WGRAD_GROUP_TILE_MASK = 16 | 32 | 64 | 128 };
size_t ctgan_conv2d_wgrad_group_workspace_bytes(const ctgan_wgrad_group* groups, int32_t n);
int ctgan_conv2d_wgrad_group(const ctgan_wgrad_group* groups, int32_t n, void* ws, size_t ws_bytes, int phases,
                             ctgan_stream_t stream);
/* The same grouped call on the 16-bit family - mma = CTGAN_MMA_F32X3 (fp32 accuracy on the bf16 matrix cores at 6/16 of the fp32 MFMA's
   cost: the hybrid fp32 mode's weight gradients) or CTGAN_MMA_BF16 / CTGAN_MMA_F16 (the small weight gradients of the mixed-precision configs):
   every segment of every group is one problem of ONE launch of 128x128-tile workgroups with a common pixels-per-split, then one batched
   reduction (add_dw / add_db as above).  Members: C and K multiples of 128, power-of-two pixel grid (split mode; Q % 4 == 0 otherwise), unit channel stride of x, dense
   channels-last dy, no x_up; workspace_bytes returns 0 and the call CTGAN_E_UNSUPPORTED (nothing launched) if a member does not
   qualify - the caller then uses ctgan_conv2d_wgrad_group for it.  phases as CTGAN_WGRAD_GROUP_GEMM | CTGAN_WGRAD_GROUP_REDUCE; with
   CTGAN_WGRAD_GROUP_TILE0 << 0 / << 1 the GEMM phase launches only the filter-column / only the slice kernel.                  */
size_t ctgan_conv2d16_wgrad_group_workspace_bytes(const ctgan_wgrad_group* groups, int32_t n, int mma);
int ctgan_conv2d16_wgrad_group(const ctgan_wgrad_group* groups, int32_t n, int mma, void* ws, size_t ws_bytes, int phases,
                               ctgan_stream_t stream);
/* the launch (0..3) of a grouped call that problem g rides in; -1 if it does not qualify */
int ctgan_conv2d_wgrad_group_tile(const ctgan_wgrad_group* g);
/* ---- convolution family  (replaces tf.nn.conv2d TF/tflib/ops/conv2d.py:106-112,
 *      tf.nn.conv2d_transpose TF/tflib/ops/deconv2d.py:97-103, tf.matmul
 *      TF/tflib/ops/linear.py:132-137 (as 1x1 conv on a 1x1 image), and the conv gradient nodes
 *      tf.gradients / compute_gradients generate, TF/CT_gan_cifar_resnet.py:284,335-336) ------- */
size_t ctgan_conv2d_workspace_bytes(const ctgan_conv_desc* d, int op);
/* y = conv(x,w) [+ bias[k]] [+ resid (same strides as y)] [relu if flags&CTGAN_EPI_RELU]; ext (NULL = none): the
 * epilogue extension above                                                                     */
int ctgan_conv2d_fwd(const ctgan_conv_desc* d, const float* x, const float* w, const float* bias, const float* resid,
                     float* y, int flags, const ctgan_epilogue_ext* ext, ctgan_stream_t stream);
/* dx = adjoint of conv w.r.t. x, applied to dy [+ bias[c]] (dx has the strides d->xs; x_up must
 * be 0).  With bias this is Deconv2D's forward (TF/tflib/ops/deconv2d.py:97-110).               */
/* epilogue: dx = (conv^T(dy,w) + bias) [kept only where mask > 0: the ReLU backward of conv(relu(x)),
 * mask = x] [+ resid] [times the dropout mask of ext; NULL = none].  mask and resid have the strides of dx. */
int ctgan_conv2d_dgrad(const ctgan_conv_desc* d, const float* dy, const float* w, const float* bias,
                       const float* mask, const float* resid, float* dx, void* ws, size_t ws_bytes, int flags,
                       const ctgan_epilogue_ext* ext, ctgan_stream_t stream);
/* wt[r',s',k,c] = w[R-1-r',S-1-s',c,k]: the rotated, I/O-swapped filter the data gradient multiplies
 * with.  Callers that run several dgrads per weight update repack once and pass
 * CTGAN_DGRAD_W_REPACKED (then `w` is wt and no workspace is needed).                            */
int ctgan_conv2d_repack_filter(const ctgan_conv_desc* d, const float* w, float* wt, ctgan_stream_t stream);
/* ---- Layernorm, fused (csrc/layernorm.hip) ----------------------------------------------------------------------------------
 * TF/tflib/ops/layernorm.py:6-20 (tf.nn.moments over the non-batch axes + tf.nn.batch_normalization, eps 1e-5) for dense
 * tensors with the channel axis fastest ([N,H,W,C] or [N,C]); D = elements per sample, C = channels (scale / offset size).
 *   fwd : y = (x - mean) * rstd * scale[c] + offset[c]; mean / rstd [N] are returned for the backward passes
 *   bwd : gx (and, when gscale / goffset != NULL, the parameter gradients) from the gradient gy of y
 *   bwd2: the adjoint of bwd - the gradient penalty differentiates the critic twice (LS/wgan_LSUN_Bedrooms128.py:256-262):
 *         given the cotangent u of gx returns the cotangents of gy, x and scale (NULL = not wanted)
 * Supported when C % 4 == 0 and 1024 % C == 0 (ctgan_layernorm_supported); otherwise CTGAN_E_UNSUPPORTED and the caller
 * composes the operator from ctgan_sample_sum / ctgan_mul / ctgan_rsqrt / ctgan_channel_affine.  ws: scratch of
 * ctgan_layernorm_workspace_bytes(N, D, C) bytes.  N (and, for the label-conditioned maps and the by-label row sum, n_labels)
 * above 65535 is CTGAN_E_UNSUPPORTED too, returned before any launch: they are the y / z extents of the launch grids.      */
int ctgan_layernorm_supported(int64_t D, int32_t C);
size_t ctgan_layernorm_workspace_bytes(int32_t N, int64_t D, int32_t C);
/* relu != 0: y = relu(Layernorm(x)) (the critics' Normalize -> nonlinearity, LS/wgan_LSUN_Bedrooms128.py:122-128) in the same
 * pass; the backward maps then take that y as `ymask` (NULL = no fused ReLU) and read gy as gy * (y > 0).                   */
int ctgan_layernorm_fwd(const float* x, const float* scale, const float* offset, float* y, float* mean, float* rstd, int32_t N,
                        int64_t D, int32_t C, float eps, int32_t relu, void* ws, size_t ws_bytes, ctgan_stream_t stream);
int ctgan_layernorm_bwd(const float* gy, const float* x, const float* scale, const float* mean, const float* rstd,
                        const float* ymask, float* gx, float* gscale, float* goffset, int32_t N, int64_t D, int32_t C, void* ws,
                        size_t ws_bytes, ctgan_stream_t stream);
int ctgan_layernorm_bwd2(const float* u, const float* gy, const float* x, const float* scale, const float* mean,
                         const float* rstd, const float* ymask, float* cot_gy, float* cot_x, float* cot_scale, int32_t N,
                         int64_t D, int32_t C, void* ws, size_t ws_bytes, ctgan_stream_t stream);
/* Label-conditioned twins (LS/tflib/ops/layernorm.py:21-30; the "vanilla" conditional critic of TF/CT_gan_cifar_resnet.py:70-87):
 * scale / offset are row-major [n_labels, C] tables and sample n uses row labels[n] (int32 [N], device memory).  A label is
 * clamped to [0, n_labels) inside the kernels, so no label can index outside the tables.  gscale / goffset / cot_scale are
 * [n_labels, C]: per (label, channel) the fixed-order fp64 sum over the samples that carry the label (no float atomics, identical
 * bits run to run), a written zero row for a label absent from the batch.  Same support predicate (ctgan_layernorm_supported) and
 * workspace (ctgan_layernorm_workspace_bytes) as the unconditional maps; tables whose rows all equal one vector give y, gx,
 * cot_gy and cot_x equal to the unconditional results bit for bit.                                                        */
int ctgan_layernorm_cond_fwd(const float* x, const float* scale, const float* offset, const int32_t* labels, int32_t n_labels,
                             float* y, float* mean, float* rstd, int32_t N, int64_t D, int32_t C, float eps, int32_t relu, void* ws,
                             size_t ws_bytes, ctgan_stream_t stream);
int ctgan_layernorm_cond_bwd(const float* gy, const float* x, const float* scale, const float* mean, const float* rstd,
                             const float* ymask, const int32_t* labels, int32_t n_labels, float* gx, float* gscale, float* goffset,
                             int32_t N, int64_t D, int32_t C, void* ws, size_t ws_bytes, ctgan_stream_t stream);
int ctgan_layernorm_cond_bwd2(const float* u, const float* gy, const float* x, const float* scale, const float* mean,
                              const float* rstd, const float* ymask, const int32_t* labels, int32_t n_labels, float* cot_gy,
                              float* cot_x, float* cot_scale, int32_t N, int64_t D, int32_t C, void* ws, size_t ws_bytes,
                              ctgan_stream_t stream);
/* The table side of the composed conditional operator (channel counts outside the fused kernels): out [N, C] = table[labels[n]]
 * and its adjoint out [n_labels, C] = the by-label sum of rows [N, C] (same fixed-order fp64 reduction as above, labels clamped). */
int ctgan_layernorm_rows_gather(const float* table, const int32_t* labels, int32_t n_labels, float* out, int32_t N, int32_t C,
                                ctgan_stream_t stream);
int ctgan_layernorm_rows_sum_by_label(const float* rows, const int32_t* labels, int32_t n_labels, float* out, int32_t N, int32_t C,
                                      ctgan_stream_t stream);
/* ---- 16-bit matrix-core family (csrc/igemm16.hip): BASELINE.json configs[1] "bf16" and configs[4] "fp16 MFMA conv" ----
 * The same three operators (tf.nn.conv2d TF/tflib/ops/conv2d.py:106-112, tf.nn.conv2d_transpose / the data gradient
 * TF/tflib/ops/deconv2d.py:91-103, the filter gradient tf.gradients derives) computed as mixed precision: operands rounded
 * (nearest-even) to bf16 or fp16 on their way into LDS, v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulation; activations,
 * gradients and master weights stay fp32 in caller memory.  The filter operand is a packed 16-bit image built once per
 * weight version by ctgan_conv2d16_pack_filter (FWD: [K][(r,s,c)]; DGRAD: per output-parity phase [C][(t,u,k)] with the taps
 * of that phase only, rotated).  `mma` = CTGAN_MMA_BF16 | CTGAN_MMA_F16.  Shapes outside the family (few-channel layers, odd
 * extents, x_up) return CTGAN_E_UNSUPPORTED: the caller uses the fp32 entry points above for those layers.
 * Epilogues as the fp32 family: fwd  y = [relu](conv(x | relu(x)) + bias + resid);  dgrad  dx = (conv^T(dy) + bias)
 * [kept where mask > 0] [+ resid].  flags = CTGAN_EPI_RELU | CTGAN_IN_RELU.  The bias gradient is not fused here
 * (ctgan_colsum).                                                                                                     */
/* CTGAN_MMA_F32X3: fp32 arithmetic on the bf16 matrix cores.  Every fp32 operand is split exactly into three bf16 terms
 * (x = h + m + l, nearest-even at each level: 24 significand bits) while it is staged, and a product is the six bf16 MFMAs
 * hh + hm + mh + mm + hl + lh accumulated in fp32 - the dropped terms are below 2^-24 relative, i.e. the result carries fp32
 * rounding accuracy (measured against an fp64 reference it is as close as the fp32 MFMA family), at 6/16 of the fp32 MFMA's
 * cycle cost.  The packed filter holds the three planes one after the other.                                               */
enum { CTGAN_MMA_BF16 = 1, CTGAN_MMA_F16 = 2, CTGAN_MMA_F32X3 = 3 };
int ctgan_conv2d16_supported(const ctgan_conv_desc* d, int op, int mma);        /* op = CTGAN_CONV_{FWD,DGRAD,WGRAD}; 1 / 0 */
/* 1 where CTGAN_MMA_F32X3 is the faster fp32 path for this launch (stride-1 convs / data gradients on whole-row or whole-image
 * 128x128 tiles, stride-2 convs / data gradients, weight gradients over >= 32k pixels - each only when the launch fills the chip):
 * the caller may route such layers through ctgan_conv2d16_{fwd,dgrad,wgrad} with mma = CTGAN_MMA_F32X3 and keep every other layer
 * on the fp32 MFMA entry points - the results carry fp32 accuracy either way.  A forward launch with prefers = 1 and stride 1 also
 * accepts CTGAN_RESID_UP.                                                                                                    */
int ctgan_conv2d16_x3_prefers(const ctgan_conv_desc* d, int op);
/* 1 when ctgan_conv2d16_fwd (mma = CTGAN_MMA_F32X3, CTGAN_IN_RELU) takes this forward launch with the input batch norm on load
 * (ctgan_epilogue_ext::in_bn_*): stride 1 on the fragment-streaming halo kernel with every tile inside one image.  The launcher asks
 * the same function, so a caller that gets 1 here never computes the moments for a launch that is then refused.                   */
int ctgan_conv2d16_bn_in_takes(const ctgan_conv_desc* d);
/* 1 when the filter-column weight-gradient kernel (csrc/wgrad16c.hip) takes this problem over `rows` samples in mode mma - geometry, the
 * strides of x in d->xs (images dense in memory) and the 32-bit offset limits; callers that queue weight gradients for
 * ctgan_conv2d16_wgrad_group use it to tell the problems the grouped launch runs on that kernel from those it would run on the slice tiles. */
int ctgan_conv2d16_wgrad_col_takes(const ctgan_conv_desc* d, int mma, int32_t rows);
size_t ctgan_conv2d16_filter_elems(const ctgan_conv_desc* d, int op, int mma);  /* 16-bit elements of the packed filter     */
int ctgan_conv2d16_pack_filter(const ctgan_conv_desc* d, int op, int mma, const float* w, void* wp, ctgan_stream_t stream);
/* n packs in one launch (all images of one weight version): descs[i] / ops[i] (CTGAN_CONV_FWD | CTGAN_CONV_DGRAD) / ws[i] -> wps[i] */
int ctgan_conv2d16_pack_batch(const ctgan_conv_desc* descs, const int32_t* ops, int32_t n, int mma, const float* const* ws,
                              void* const* wps, ctgan_stream_t stream);
/* ws (optional, ctgan_conv2d16_workspace_bytes(d, op) bytes): slabs for a K split of launches whose pixel x channel tiles cannot
 * fill the chip (8x8 / 4x4 layers at batch 64); NULL = never split.                                                      */
size_t ctgan_conv2d16_workspace_bytes(const ctgan_conv_desc* d, int op);
/* ext (NULL = none) with the epilogue dropout of ctgan_conv2d_fwd (same ext, same draws): mma = CTGAN_MMA_F32X3 on launches the halo-patch
 * kernel takes (ctgan_conv2d16_x3_prefers, stride 1); CTGAN_E_UNSUPPORTED otherwise - the caller then uses ctgan_conv2d_fwd.       */
int ctgan_conv2d16_fwd(const ctgan_conv_desc* d, int mma, const float* x, const void* wp, const float* bias, const float* resid,
                       float* y, int flags, const ctgan_epilogue_ext* ext, void* ws, size_t ws_bytes, ctgan_stream_t stream);
/* ext (NULL = none) with the epilogue dropout of ctgan_conv2d_dgrad (dx multiplied by the mask of ext's dropout, same draws at the same
 * physical offsets): mma = CTGAN_MMA_F32X3, stride 1, dense channels-last dx, launches the halo-patch kernels take; CTGAN_E_UNSUPPORTED
 * otherwise - the caller then uses ctgan_conv2d_dgrad.                                                                             */
int ctgan_conv2d16_dgrad(const ctgan_conv_desc* d, int mma, const float* dy, const void* wp, const float* bias,
                         const float* mask, const float* resid, float* dx, int flags, const ctgan_epilogue_ext* ext, void* ws,
                         size_t ws_bytes, ctgan_stream_t stream);
size_t ctgan_conv2d16_wgrad_workspace_bytes(const ctgan_conv_desc* d, int mma);
/* db != NULL: the bias gradient db[K] = sum over pixels of dy fused into the same launch (the workgroups of the first tile row sum the dy
 * tiles they stage; fixed-order reduction): replaces the separate ctgan_colsum pass.  db NULL = the filter gradient alone.         */
int ctgan_conv2d16_wgrad(const ctgan_conv_desc* d, int mma, const float* x, const float* dy, float* dw, float* db, void* ws,
                         size_t ws_bytes, int flags, ctgan_stream_t stream);
/* flags of ctgan_conv2d16_wgrad besides CTGAN_IN_RELU: launch only the split-K GEMM (slabs stay in ws) / only the reduction of
   slabs a GEMM-only call left there - bench.py times the two kernels apart, as rocprofv3 lists them                               */
enum { CTGAN_WGRAD16_GEMM_ONLY = 0x100, CTGAN_WGRAD16_REDUCE_ONLY = 0x200 };
/* dw[r,s,c,k] = sum_{n,p,q} x[..] * dy[n,k,p,q]   (HWIO, contiguous; deterministic split-K);
 * db[k] = sum_{n,p,q} dy[n,k,p,q] when db != NULL (tf.nn.bias_add gradient, fused when possible) */
int ctgan_conv2d_wgrad(const ctgan_conv_desc* d, const float* x, const float* dy, float* dw, float* db,
                       void* ws, size_t ws_bytes, int flags /* CTGAN_IN_RELU: x -> relu(x) */,
                       ctgan_stream_t stream);
/* Patch expansion for convs with very few input channels (first critic conv, TF/CT_gan_cifar_resnet.py:
 * 144,150; TF/CT_gan_cifar.py:84; TF/CT_gan_mnist.py:92): cols[n,p,q,(r*S+s)*C+c] = x[n,c,p*st-pt+r,q*st-pl+s]
 * (zero outside the image and for columns >= R*S*C; cols is channels-last [N,P,Q,cpad], contiguous).
 * col2im is its adjoint (dx has the strides d->xs).                                              */
int ctgan_im2col(const ctgan_conv_desc* d, const float* x, int32_t cpad, float* cols, ctgan_stream_t stream);
int ctgan_col2im(const ctgan_conv_desc* d, const float* cols, int32_t cpad, float* dx, ctgan_stream_t stream);
/* out[j] = sum_i x[i*ld + j], i<rows, j<cols (bias gradient; tf.nn.bias_add grad)             */
int ctgan_colsum(const float* x, int64_t rows, int32_t cols, int64_t ld, float* out,
                 void* ws, size_t ws_bytes, ctgan_stream_t stream);
size_t ctgan_colsum_workspace_bytes(int64_t rows, int32_t cols);

/* ---- elementwise / layout (K9-K12, K19 of SURVEY 2.1) -------------------------------------- */
/* y = x>0 ? x : alpha*x   (tf.nn.relu alpha=0; LeakyReLU tf.maximum(alpha*x,x) alpha=0.2)     */
int ctgan_lrelu_fwd(const float* x, float* y, int64_t n, float alpha, ctgan_stream_t stream);
/* gx = ref>0 ? gy : alpha*gy  (ref = forward input or output; same sign)                      */
int ctgan_lrelu_bwd(const float* gy, const float* ref, float* gx, int64_t n, float alpha,
                    ctgan_stream_t stream);
/* gx = scale * (ref>0 ? gy : alpha*gy): backward of y = dropout(relu(z)) computed in a conv epilogue, where
 * ref = y (y > 0 iff z > 0 and the element was kept) and scale = 1/keep                          */
int ctgan_lrelu_bwd_scaled(const float* gy, const float* ref, float* gx, int64_t n, float alpha, float scale,
                           ctgan_stream_t stream);
/* tf.nn.dropout: y = x/keep * floor(keep + u)  (TF/CT_gan_cifar_resnet.py:173-177); the
 * backward is the same call on the gradient.  keep in (0,1]; keep = 1 returns x itself
 * (floor(1 + u) would be 2 in float for u = 1 - 2^-24, the largest uniform draw) - here and
 * in the ctgan_*dropout_rng* entry points.                                                    */
int ctgan_dropout(const float* x, const float* u, float* y, int64_t n, float keep,
                  ctgan_stream_t stream);
int ctgan_tanh_fwd(const float* x, float* y, int64_t n, ctgan_stream_t stream);
int ctgan_tanh_bwd(const float* gy, const float* y, float* gx, int64_t n, ctgan_stream_t stream);
int ctgan_sigmoid_fwd(const float* x, float* y, int64_t n, ctgan_stream_t stream);
int ctgan_sigmoid_bwd(const float* gy, const float* y, float* gx, int64_t n, ctgan_stream_t stream);
/* out = a*x + b*y  (residual add; y may be NULL => out = a*x)                                  */
int ctgan_axpby(const float* x, const float* y, float* out, int64_t n, float a, float b,
                ctgan_stream_t stream);
/* generic 4-D strided copy (NCHW <-> NHWC repack): y[i0,i1,i2,i3] = x[i0,i1,i2,i3]            */
int ctgan_copy4d(const float* x, const int64_t xs[4], float* y, const int64_t ys[4],
                 const int32_t dims[4], ctgan_stream_t stream);
/* y[n,c,p,q] = scale * sum of the 2x2 window of x  (mean-pool: scale=.25,
 * TF/CT_gan_cifar_resnet.py:91,96; also the adjoint of upsample2 with scale=1)                 */
int ctgan_pool2(const float* x, const int64_t xs[4], float* y, const int64_t ys[4],
                const int32_t ydims[4] /* n,c,p,q */, float scale, ctgan_stream_t stream);
/* y[n,c,h,w] = scale * x[n,c,h/2,w/2]  (nearest 2x upsample, TF/CT_gan_cifar_resnet.py:102-105;
 * also the adjoint of pool2)                                                                   */
int ctgan_upsample2(const float* x, const int64_t xs[4], float* y, const int64_t ys[4],
                    const int32_t ydims[4] /* n,c,h,w */, float scale, ctgan_stream_t stream);
/* Filters of a conv fused with its 2x resampling (exact algebra, fewer multiplies):
 *   ConvMeanPool (TF/CT_gan_cifar_resnet.py:89-92): pool2(conv_RxS(x, w))  = conv_{(R+1)x(S+1), stride 2}(x, spread(w)/4)
 *   UpsampleConv (:100-107):   conv_RxS(upsample2(x), w) = conv2d_transpose_{(R+1)x(S+1), stride 2}(x, flipped spread(w))
 * spread: out[u,v,c,k] = scale * sum_{a,b in {0,1}} w[u-a, v-b, c, k]   (w is [R,S,C,K], out [(R+1),(S+1),C,K]);
 * flip != 0 writes the rotated, I/O-swapped filter out[R-u, S-v, k, c] instead ([(R+1),(S+1),K,C]).        */
int ctgan_filter_spread(const float* w, float* out, int32_t R, int32_t S, int32_t C, int32_t K, float scale,
                        int32_t flip, ctgan_stream_t stream);
/* the adjoint map (weight gradient back to the RxS filter): out[r,s,c,k] = scale * sum_{a,b} W[r+a, s+b, c, k],
 * W = w4 (flip == 0) or its un-flipped view W[u,v,c,k] = w4[R-u, S-v, k, c] (flip != 0)                      */
int ctgan_filter_fold(const float* w4, float* out, int32_t R, int32_t S, int32_t C, int32_t K, float scale,
                      int32_t flip, ctgan_stream_t stream);
/* All derived filters of one weight update in a single launch (per CTGAN_FILTER_BATCH jobs): every job reads an
 * HWIO filter src[R,S,C,K] and writes one derived layout.  `jobs` is a HOST array; it travels in the kernel
 * arguments, so the call is hipGraph-capture safe.
 *   CTGAN_FILTER_ROTATE      dst[R,S,K,C]            = what ctgan_conv2d_repack_filter writes for a stride-1 conv
 *   CTGAN_FILTER_PHASES      dst[4][ceil(R/2)][ceil(S/2)][K][C] = ... for a stride-2 conv with pads (pad_t, pad_l)
 *   CTGAN_FILTER_SPREAD      dst[(R+1),(S+1),C,K]    = ctgan_filter_spread(scale, flip = 0)
 *   CTGAN_FILTER_SPREAD_FLIP dst[(R+1),(S+1),K,C]    = ctgan_filter_spread(scale, flip = 1)                  */
#define CTGAN_FILTER_ROTATE 0
#define CTGAN_FILTER_PHASES 1
#define CTGAN_FILTER_SPREAD 2
#define CTGAN_FILTER_SPREAD_FLIP 3
/* pre = CTGAN_FILTER_SPREAD / _SPREAD_FLIP with kind = ROTATE / PHASES: the layout is taken OF the spread filter
 * (pre_scale = its scale; its taps are (R+1) x (S+1), and for _SPREAD_FLIP its channel roles are swapped) straight from
 * src, bit-identical to running the spread job first and the layout job on its output - but independent of it.          */
#define CTGAN_FILTER_BATCH 40
typedef struct ctgan_filter_job {
    const float* src;
    float* dst;
    int32_t R, S, C, K;
    int32_t kind;
    int32_t pad_t, pad_l;
    float scale;
    int32_t pre;
    float pre_scale;
} ctgan_filter_job;
int ctgan_filter_batch(const ctgan_filter_job* jobs, int32_t n, ctgan_stream_t stream);
/* Several ctgan_filter_fold calls in one launch: dst[R,S,C,K] = scale * fold(src [(R+1),(S+1),C,K] or, flip, [(R+1),(S+1),K,C]). */
#define CTGAN_FOLD_BATCH 16
typedef struct ctgan_fold_job {
    const float* src;
    float* dst;
    int32_t R, S, C, K;
    float scale;
    int32_t flip;
} ctgan_fold_job;
int ctgan_filter_fold_batch(const ctgan_fold_job* jobs, int32_t n, ctgan_stream_t stream);
/* ---- Layernorm primitives (TF/tflib/ops/layernorm.py:6-20: tf.nn.moments over (C,H,W) per sample +
 *      tf.nn.batch_normalization with per-channel scale/offset).  The operator is composed of these linear /
 *      elementwise maps so that its first AND second derivatives (gradient penalty through a layer-normalised
 *      critic, config[4]) are compositions of the same kernels. ---------------------------------------------- */
int ctgan_mul(const float* x, const float* y, float* out, int64_t n, ctgan_stream_t stream);           /* out = x*y    */
int ctgan_rsqrt(const float* x, float* y, int64_t n, float eps, ctgan_stream_t stream);               /* 1/sqrt(x+eps) */
/* y[i] = scale * sum_j x[i][j] for a dense [n][m] tensor (per-sample reduction, fixed order)                    */
int ctgan_sample_sum(const float* x, float* y, int32_t n, int64_t m, float scale, ctgan_stream_t stream);
/* y[i][j] = scale * v[i]  (its adjoint)                                                                         */
int ctgan_sample_bcast(const float* v, float* y, int32_t n, int64_t m, float scale, ctgan_stream_t stream);
/* channels-last x [rows][c]: y = x*scale[c] + offset[c] (offset may be NULL)                                    */
int ctgan_channel_affine(const float* x, const float* scale, const float* offset, float* y, int64_t rows, int32_t c,
                         ctgan_stream_t stream);
/* y[n,c] = scale * sum_{hw} x[n,hw,c]  (tf.reduce_mean(axis=[2,3]) :179) on channels-last x    */
int ctgan_spatial_sum(const float* x, float* y, int32_t n, int32_t hw, int32_t c, float scale,
                      ctgan_stream_t stream);
/* y[n,hw,c] = scale * g[n,c]  (its adjoint)                                                    */
int ctgan_spatial_bcast(const float* g, float* y, int32_t n, int32_t hw, int32_t c, float scale,
                        ctgan_stream_t stream);
/* real = 2*((int/denom)-.5) + noise   (TF/CT_gan_cifar_resnet.py:201-202; noise may be NULL:
 * TF/CT_gan_cifar.py:103 with denom 255)                                                       */
int ctgan_real_prep(const int32_t* x_int, const float* noise, float* y, int64_t n, float denom,
                    ctgan_stream_t stream);
/* score-sample pixels (TF/CT_gan_cifar_resnet.py:355-357): out[n,hw,c] (uint8, NHWC) = trunc((x[n,c,hw] + 1) * scale)
 * clamped to [0, 255], x fp32 NCHW; add, then multiply, each rounded in fp32.  A non-finite x gives 0.  scale > 0.  */
int ctgan_pixels_u8(const float* x, uint8_t* out, int64_t n, int32_t c, int32_t hw, float scale,
                    ctgan_stream_t stream);
/* out[b,:] = real[b,:] + alpha[b]*(fake[b,:]-real[b,:])   (:282-283)                           */
int ctgan_interpolate(const float* real, const float* fake, const float* alpha, float* out,
                      int32_t b, int32_t d, ctgan_stream_t stream);

/* ---- batch norm (K13/K14): training-mode statistics over (n,h,w) per channel, biased variance,
 *      eps added inside rsqrt; `groups` independent row groups of n/groups samples each model the
 *      reference's per-tower statistics (TF/CT_gan_cifar_resnet.py:196-199,316-321).
 *      x is channels-last [n, hw, c].  scale/offset are [n_labels, c] gathered by labels[n]
 *      (cond_batchnorm.py:12-16) or [c] when labels == NULL (batchnorm.py:23-30).  ---------- */
int ctgan_bn_stats(const float* x, int32_t n, int32_t hw, int32_t c, int32_t groups, float eps,
                   float* mean /*[groups,c]*/, float* rstd /*[groups,c]*/,
                   void* ws, size_t ws_bytes, ctgan_stream_t stream);
/* The same with every partial sum in fp64 (ctgan_bn_stats keeps short per-thread sums in fp32 on its vector path): for eps as small
 * as 1e-6, where sum x^2 / n - mean^2 of a channel whose spread is far below its mean must not lose the variance to rounding.    */
int ctgan_bn_stats_f64(const float* x, int32_t n, int32_t hw, int32_t c, int32_t groups, float eps,
                       float* mean /*[groups,c]*/, float* rstd /*[groups,c]*/,
                       void* ws, size_t ws_bytes, ctgan_stream_t stream);
int ctgan_bn_apply(const float* x, const float* mean, const float* rstd, const float* scale,
                   const float* offset, const int32_t* labels, float* y, int32_t n, int32_t hw,
                   int32_t c, int32_t groups, int32_t relu, ctgan_stream_t stream);
/* backward of y = [relu]( xhat*scale + offset ): gy -> gx, gscale, goffset                     */
int ctgan_bn_bwd(const float* gy, const float* x, const float* mean, const float* rstd,
                 const float* scale, const float* offset, const int32_t* labels,
                 float* gx, float* gscale, float* goffset, int32_t n, int32_t hw, int32_t c,
                 int32_t groups, int32_t n_labels, int32_t relu, void* ws, size_t ws_bytes,
                 ctgan_stream_t stream);
size_t ctgan_bn_workspace_bytes(int32_t n, int32_t hw, int32_t c, int32_t groups, int32_t n_labels);

/* ---- batch norm of the self-trained MNIST score classifier (LS/tflib/ops/batchnorm.py:30-69) ---- */
/* ctgan_bn_stats_f64 for one statistic group that also moves the moving statistics in place (:62-65):
 *   moving <- (it/(it+1)) moving + (1/(it+1)) batch,  in fp32, it = *it read on the DEVICE (a float scalar), no special case at 0;
 * batch_var = biased variance * cnt/max(cnt-1, 1), cnt = n*hw (what tf.nn.fused_batch_norm returns in training), from the fp64 sums.
 * moving_mean == moving_var == NULL: statistics only.  ws as ctgan_bn_stats.                                                        */
int ctgan_bn_stats_moving(const float* x, int32_t n, int32_t hw, int32_t c, float eps, float* mean /*[c]*/, float* rstd /*[c]*/,
                          float* moving_mean /*[c]*/, float* moving_var /*[c]*/, const float* it, void* ws, size_t ws_bytes,
                          ctgan_stream_t stream);
/* Statistics of the inference-mode "blend" (:32-38): per sample and channel the biased moments m, v over hw, then in fp32
 *   mean[n][c] = m/B + ((B-1)/B) moving_mean[c],  var alike,  rstd[n][c] = 1/sqrt(var + eps),  B = n (the rows of the call).       */
int ctgan_bn_blend_stats(const float* x, int32_t n, int32_t hw, int32_t c, float eps, const float* moving_mean,
                         const float* moving_var, float* mean /*[n,c]*/, float* rstd /*[n,c]*/, void* ws, size_t ws_bytes,
                         ctgan_stream_t stream);
/* y = [shortcut +] alpha * [relu]((x - mean) * rstd * scale + offset) and, with elu_out, elu_out = elu(y), in one pass.
 * per_sample: mean / rstd are [n,c] (ctgan_bn_blend_stats), else [c].  shortcut and elu_out may be NULL.                            */
int ctgan_bn_apply_ex(const float* x, const float* mean, const float* rstd, int32_t per_sample, const float* scale,
                      const float* offset, const float* shortcut, float alpha, float* y, float* elu_out, int32_t relu, int32_t n,
                      int32_t hw, int32_t c, ctgan_stream_t stream);
/* ctgan_bn_bwd (one group, no labels, no ReLU) of the gradient gy_scale * gy: the factor rides on the reduced totals and the gain,
 * not on a pass over gy.  ws: ctgan_bn_workspace_bytes(n, hw, c, 1, 1).                                                            */
int ctgan_bn_bwd_scaled(const float* gy, const float* x, const float* mean, const float* rstd, const float* scale,
                        const float* offset, float gy_scale, float* gx, float* gscale, float* goffset, int32_t n, int32_t hw,
                        int32_t c, void* ws, size_t ws_bytes, ctgan_stream_t stream);

/* ---- batch norm with the following activation folded in, and the gate on its own (csrc/bn_act.hip): the hidden layers of the DCGAN-style
 *      64x64 nets, conv -> Batchnorm -> LeakyReLU | tanh | gate (TF/CT_gan_64x64.py:237-273, :325-353, :375-399, :435-467).
 *      z = (x - mean) rstd scale + offset with mean / rstd [groups, c] from ctgan_bn_stats and scale / offset [c];
 *      LRELU: y = z > 0 ? z : alpha z;  TANH: y = tanh(z);  GATE: y[.., j] = sigmoid(z[.., 2j]) tanh(z[.., 2j+1]), y and gy [n, hw, c/2]
 *      (c even; :95-96, :333).  ReLU stays with ctgan_bn_apply / ctgan_bn_bwd.  ---------- */
#define CTGAN_ACT_LRELU 0
#define CTGAN_ACT_TANH 1
#define CTGAN_ACT_GATE 2
int ctgan_bn_act_apply(const float* x, const float* mean, const float* rstd, const float* scale, const float* offset, float* y,
                       int32_t n, int32_t hw, int32_t c, int32_t groups, int32_t act, float alpha, ctgan_stream_t stream);
/* gy -> gx, gscale [c], goffset [c] with g = act'(z) gy recomputed from x and the coefficients in both passes (three launches, as
 * ctgan_bn_bwd).  ws: ctgan_bn_workspace_bytes(n, hw, c, groups, 1).                                                             */
int ctgan_bn_act_bwd(const float* gy, const float* x, const float* mean, const float* rstd, const float* scale, const float* offset,
                     float* gx, float* gscale, float* goffset, int32_t n, int32_t hw, int32_t c, int32_t groups, int32_t act,
                     float alpha, void* ws, size_t ws_bytes, ctgan_stream_t stream);
/* The gate without a normalisation, over flat pairs: y[j] = sigmoid(x[2j]) tanh(x[2j+1]), j < n_out - a dense channels-last tensor
 * with an even channel count (or rows [n, c]) -> half the channels.  One launch each way.                                         */
int ctgan_gate_fwd(const float* x, float* y, int64_t n_out, ctgan_stream_t stream);
int ctgan_gate_bwd(const float* gy, const float* x, float* gx, int64_t n_out, ctgan_stream_t stream);

/* ---- ELU and the global-norm clip of the score classifier (csrc/score.hip) ---- */
/* y = x > 0 ? x : expm1(x)                                                                      */
int ctgan_elu_fwd(const float* x, float* y, int64_t n, ctgan_stream_t stream);
/* gx = [add +] (y > 0 ? gy : gy * (y + 1)),  y the forward OUTPUT; add may be NULL             */
int ctgan_elu_bwd(const float* gy, const float* y, const float* add, float* gx, int64_t n, ctgan_stream_t stream);
/* norm[0] = sqrt(sum g^2): two-stage, fp64 partials in a fixed order (the same bits on every run) */
size_t ctgan_global_norm_workspace_bytes(int64_t n);
int ctgan_global_norm(const float* g, int64_t n, float* norm, void* ws, size_t ws_bytes, ctgan_stream_t stream);
/* g *= clip / max(norm[0], clip) in place, norm read on the device (tf.clip_by_global_norm with use_norm) */
int ctgan_clip_by_norm(float* g, int64_t n, const float* norm, float clip, ctgan_stream_t stream);

/* ---- fused loss heads (K16-K20) ------------------------------------------------------------- */
/* slopes[b] = ||g[b,:]||_2 ; gp = lambda*mean((slopes-1)^2)   (TF/CT_gan_cifar_resnet.py:285-286); gp == NULL: slopes only */
int ctgan_gp_fwd(const float* g, int32_t b, int32_t d, float lambda, float* slopes, float* gp,
                 ctgan_stream_t stream);
/* gg[b,:] = gout * lambda*2*(s-1)/(s*B) * g[b,:]                                               */
int ctgan_gp_bwd(const float* g, const float* slopes, const float* gout, int32_t b, int32_t d,
                 float lambda, float* gg, ctgan_stream_t stream);
/* ctgan_gp_bwd that also takes the penalty's value in the same launch: gp[0] = lambda*mean((slopes-1)^2) (gp may be NULL) and, with
 * out5 != NULL, out5[0] += gp, out5[4] += gp - the two sums of ctgan_tail_critic_heads_fwd (cost; wgan + ct + gp) that contain the
 * penalty, for a step whose loss heads ran before dD/dx_hat existed (the hand-scheduled critic step: TF/CT_gan_cifar_resnet.py:284-286,
 * :295-300 evaluated after the merged backward).                                                                               */
int ctgan_gp_bwd_mean(const float* g, const float* slopes, const float* gout, int32_t b, int32_t d, float lambda, float* gg, float* gp,
                      float* out5, ctgan_stream_t stream);
/* CT_i = l2*(d-d_)^2 + l2*0.1*mean_j (f-f_)^2 ; ct = mean_i max(CT_i - M, 0)   (:288-291)      */
int ctgan_ct_fwd(const float* d, const float* d_, const float* f, const float* f_, int32_t b,
                 int32_t nf, float lambda2, float M, float* ct_i, float* ct, ctgan_stream_t stream);
int ctgan_ct_bwd(const float* d, const float* d_, const float* f, const float* f_,
                 const float* ct_i, const float* gout, int32_t b, int32_t nf, float lambda2, float M,
                 float* gd, float* gd_, float* gf, float* gf_, ctgan_stream_t stream);
/* loss = mean_i CE(logits[i,:], labels[i]); probs saved for backward; correct = #argmax==label  */
int ctgan_softmax_ce_fwd(const float* logits, const int32_t* labels, int32_t b, int32_t ncls,
                         float* probs, float* loss, float* n_correct, ctgan_stream_t stream);
int ctgan_softmax_ce_bwd(const float* probs, const int32_t* labels, const float* gout, int32_t b,
                         int32_t ncls, float* glogits, ctgan_stream_t stream);
/* out = sign_a*mean(x[0:na]) + sign_b*mean(x[na:na+nb])  (WGAN critic / generator cost :244,322) */
int ctgan_mean_diff_fwd(const float* x, int32_t na, int32_t nb, float sa, float sb, float* out,
                        ctgan_stream_t stream);
int ctgan_mean_diff_bwd(const float* gout, int32_t na, int32_t nb, float sa, float sb, float* gx,
                        ctgan_stream_t stream);
/* Loss heads of the scripts' other MODE branches over critic outputs (TF/CT_gan_mnist.py:165-195, TF/CT_gan_64x64.py:521-537).
 * kind CTGAN_LOSS_BCE_D / CTGAN_LOSS_LS_D: d [2B] with rows [0,B) = D(real), [B,2B) = D(fake);
 *   BCE_D = (mean_i bce(d_fake_i, 0) + mean_i bce(d_real_i, 1)) / 2,  bce(x, z) = max(x,0) - x z + log1p(exp(-|x|))
 *   LS_D  = (mean_i (d_real_i - 1)^2 + mean_i d_fake_i^2) / 2
 * kind CTGAN_LOSS_BCE_G / CTGAN_LOSS_LS_G: d [B] = D(fake);  BCE_G = mean_i bce(d_i, 1),  LS_G = mean_i (d_i - 1)^2.
 * fwd: out[0] = the cost (one workgroup, fixed-order reduction).  bwd: gd = gout[0] * d cost / d d (for BCE (sigmoid(x) - z) / n,
 * finite for any finite logit).                                                                                                   */
/* Hinge objective (Lim & Ye 2017; Miyato et al. 2018; NOT in the reference), hinge(t) = t >= 0 ? t : 0, so its derivative at t == 0 is 1:
 * kind CTGAN_LOSS_HINGE_D: d [2B] as above;  HINGE_D = mean_i hinge(1 - d_real_i) + mean_i hinge(1 + d_fake_i)  (no 1/2 in front)
 * kind CTGAN_LOSS_HINGE_G: d [B] = D(fake);  HINGE_G = -mean_i d_i.                                                               */
enum { CTGAN_LOSS_BCE_D = 0, CTGAN_LOSS_BCE_G = 1, CTGAN_LOSS_LS_D = 2, CTGAN_LOSS_LS_G = 3, CTGAN_LOSS_HINGE_D = 4, CTGAN_LOSS_HINGE_G = 5 };
int ctgan_gan_loss_fwd(const float* d, int32_t B, int32_t kind, float* out, ctgan_stream_t stream);
int ctgan_gan_loss_bwd(const float* d, const float* gout, int32_t B, int32_t kind, float* gd, ctgan_stream_t stream);

/* All loss heads of one critic step over the batched dropout passes (TF/CT_gan_cifar_resnet.py:244-248,288-291):
 * d [3B], f [3B,nf], a [3B,ncls] (a may be NULL) with rows [0,B) = real pass 1, [B,2B) = fake pass 1, [2B,3B) = real
 * pass 2.  out[5] = {wgan + ct + gp + acgan_scale*acgan, wgan, ct, acgan, wgan + ct + gp} with gp = the step's gradient
 * penalty scalar (device pointer, may be NULL = 0; :284-286, :304); ct_i [B] and probs [B,ncls] are kept for the
 * backward, which writes the full gradients gd [3B], gf [3B,nf], ga [3B,ncls] given gout[n_gout] = upstream
 * gradients of the four outputs (n_gout = 4) or of the summed cost only (n_gout = 1).  One launch each instead of ~25. */
int ctgan_critic_heads_fwd(const float* d, const float* f, const float* a, const int32_t* labels, const float* gp,
                           int32_t B, int32_t nf, int32_t ncls, float lambda2, float M, float acgan_scale, float* ct_i,
                           float* probs, float* out, ctgan_stream_t stream);
int ctgan_critic_heads_bwd(const float* d, const float* f, const float* probs, const int32_t* labels, const float* ct_i,
                           const float* gout, int32_t n_gout, int32_t B, int32_t nf, int32_t ncls, float lambda2,
                           float M, float acgan_scale, float* gd, float* gf, float* ga, ctgan_stream_t stream);
/* The critic's output head fused around those loss heads (TF/CT_gan_cifar_resnet.py:179-186): y = the last residual
 * block's relu(dropout(.)) output, dense channels-last [n][hw][nf].
 *   tail_heads_fwd: f [n,nf] = mean over hw (:180; of relu(y) when relu != 0, :179), d [n] = f.w_out + b_out (:181, w_out [nf,1]; NULL = skip),
 *                   a [n,ncls] = f.w_ac + b_ac (:183, w_ac [nf,ncls]; NULL = skip) - one launch for reduce_mean + 2 Linear.
 *   tail_heads_bwd: given the saved d, f, probs, ct_i of ctgan_critic_heads_fwd and gout as in ctgan_critic_heads_bwd, writes
 *                   gy [3B][hw][nf] = the gradient w.r.t. the last block's PRE-activation (head gradients pushed through both
 *                   Linear layers, the mean and the relu/dropout mask y > 0 with its 1/keep = mask_scale) and the head
 *                   weight gradients gw_out [nf], gb_out [1], gw_ac [nf,ncls], gb_ac [ncls] - one launch instead of nine.
 *   gp_head_grad / gp_head_wgrad: the gradient-penalty branch needs only dD/dz (:284): gz = (y > 0) * w_out / hw *
 *                   mask_scale, and in the double backward gw_out[j] = mask_scale / hw * sum_{y > 0} gg[.,.,j].            */
int ctgan_tail_heads_fwd(const float* y, int32_t n, int32_t hw, int32_t nf, int32_t relu, const float* w_out,
                         const float* b_out, const float* w_ac, const float* b_ac, int32_t ncls, float* f, float* d,
                         float* a, ctgan_stream_t stream);
/* tail_heads_fwd on the 3B rows of a critic step (relu = 0) + ctgan_critic_heads_fwd in two launches: the workgroup of
 * real sample i owns both of its dropout passes (rows i and 2B+i) and writes ct_i[i], probs[i,:] and ce_i[i] (scratch
 * [B]); a one-workgroup kernel then takes the batch means into out[5].                                                */
/* ... with two optional reductions folded into the same two launches (slopes = NULL, y_clean = NULL: neither, gp is only read):
 *   slopes != NULL (gp then non-NULL): the gradient penalty's batch mean gp[0] = gp_lambda * mean((slopes - 1)^2) (:286) is taken by the
 *     one-workgroup kernel and written to gp[0] before it enters out[] (pair with ctgan_gp_fwd(.., gp = NULL));
 *   y_clean != NULL ([2B][hw][nf], real rows then fake rows, the dropout-free pass :228): a_clean [2B,ncls] = class head of its rows
 *     (relu'd first when clean_relu; f_clean [2B,nf] scratch) by extra workgroups of the rows launch, and the accuracies acc[2]
 *     (:249-266, as ctgan_accuracy2) by the one-workgroup kernel.                                                              */
int ctgan_tail_critic_heads_fwd(const float* y, int32_t B, int32_t hw, int32_t nf, const float* w_out, const float* b_out,
                                const float* w_ac, const float* b_ac, int32_t ncls, const int32_t* labels, float* gp,
                                const float* slopes, float gp_lambda, const float* y_clean, int32_t clean_relu, float* f_clean,
                                float* a_clean, float* acc, float lambda2, float M, float acgan_scale, float* f, float* d, float* a,
                                float* ct_i, float* probs, float* ce_i, float* out, ctgan_stream_t stream);
/* n_gp > 0: also writes gz_gp = ctgan_gp_head_grad(y_gp) for the n_gp rows of the penalty pass (the seeds of BOTH backward chains in
 * one launch - the hand-scheduled critic step, critic_schedule.py, runs them as one chain); y_gp = NULL, n_gp = 0, gz_gp = NULL: none. */
int ctgan_tail_heads_bwd(const float* y, const float* d, const float* f, const float* probs, const int32_t* labels, const float* ct_i,
                         const float* gout, int32_t n_gout, int32_t B, int32_t hw, int32_t nf, int32_t ncls, float lambda2, float M,
                         float acgan_scale, float mask_scale, const float* w_out, const float* w_ac, float* gy, float* gw_out,
                         float* gb_out, float* gw_ac, float* gb_ac, const float* y_gp, int32_t n_gp, float* gz_gp, ctgan_stream_t stream);
/* Generator-step loss on the critic's output head (TF/CT_gan_cifar_resnet.py:321-330): cost = -mean(d) + ac_scale * CE(a, labels)
 * with f, d, a as in ctgan_tail_heads_fwd (two launches), and its backward straight to the gradient w.r.t. the last critic
 * conv's result (both Linear data gradients, the mean's broadcast, the relu/dropout mask) in one launch; the critic's weights
 * get no gradient in the generator step.                                                                                    */
int ctgan_gen_heads_fwd(const float* y, int32_t n, int32_t hw, int32_t nf, const float* w_out, const float* b_out,
                        const float* w_ac, const float* b_ac, int32_t ncls, const int32_t* labels, float ac_scale, float* f,
                        float* d, float* a, float* probs, float* out, ctgan_stream_t stream);
int ctgan_gen_heads_bwd(const float* y, const float* probs, const int32_t* labels, const float* gout, int32_t n, int32_t hw,
                        int32_t nf, int32_t ncls, float ac_scale, float mask_scale, const float* w_out, const float* w_ac,
                        float* gy, ctgan_stream_t stream);
/* Round 5 (the hand-scheduled critic step, critic_schedule.py): launches folded into their neighbours.
 *   ctgan_gp_head_wgrad      : accumulate != 0 ADDS onto gw (the head weight's gradient from the dropout passes) instead of writing it;
 *   ctgan_gp_finish          : ga [b, c*h*w] (NCHW, in place) += scale * upsample2(gs [b,c,h/2,w/2], element strides gs_strides[4]) and
 *                              slopes[b] = ||ga[b,:]||_2 - dD/dx_hat = gradient through the first conv + gradient through the pooled 1x1
 *                              shortcut (:146-153, :284-285) in one launch instead of upsample + add + ctgan_gp_fwd.                      */
int ctgan_gp_finish(float* ga, const float* gs, const int64_t* gs_strides, int32_t b, int32_t c, int32_t h, int32_t w, float scale, float* slopes,
                    ctgan_stream_t stream);
int ctgan_gp_head_grad(const float* y, const float* w_out, int32_t n, int32_t hw, int32_t nf, float mask_scale,
                       float* gz, ctgan_stream_t stream);
int ctgan_gp_head_wgrad(const float* gg, const float* y, int32_t n, int32_t hw, int32_t nf, float mask_scale, float* gw,
                        float* ws /* 64 * nf floats */, int accumulate, ctgan_stream_t stream);
/* ---- Projection head (Miyato & Koyama 2018; NOT in the reference): D(x, y) = f . (w_out + E[y]) + b_out with a label table
 * emb = E [n_labels, nf] (row-major; 4-byte alignment is enough: it lives in the optimizer's flat bucket) - the output head above with a PER-ROW weight vector, so every entry point below is its
 * twin without the `_proj` with w_out + emb[label of the row] wherever the twin reads w_out: same launches, same grids for the rows, same
 * summation orders (a zero table gives the twin's bits).  There is no class head and there are no clean rows in these forms.
 * labels are int32 in [0, n_labels); a label outside that range is the CALLER's error (as for ctgan_rows_gather): it is not checked and
 * makes the kernels read outside emb.  No kernel writes through a label: g_emb is indexed by class.
 *   tail_critic_heads_fwd_proj : labels [B]; row r of the 3B rows [real, fake, real'] reads labels[r % B].  gp / slopes / gp_lambda as in
 *                                ctgan_tail_critic_heads_fwd.  out[5] = {cost, wgan, ct, 0, wgan + ct + gp}.
 *   tail_heads_bwd_proj        : as ctgan_tail_heads_bwd; penalty row i (n_gp <= B rows) reads labels[i]; additionally
 *                                g_emb [n_labels, nf]: g_emb[c][j] = sum over the rows r with labels[r % B] = c of f[r][j] * gd[r], in ascending
 *                                row order by one wave per element (no atomics: the same bits on every run).  Every element is written; the
 *                                row of a class no sample carries is exact zeros.  sum_c g_emb[c] = gw_out up to rounding.
 *   gen_heads_fwd_proj / _bwd_proj : labels [n], one per row; cost = -mean(d); gy = (y > 0) (-gout / n) (w_out + emb[label]) / hw * mask_scale.
 *   gp_head_grad_proj          : labels [n], one per row; gz = (y > 0) (w_out + emb[label]) / hw * mask_scale.
 *   gp_head_wgrad_proj         : its adjoint: gw [nf] as ctgan_gp_head_wgrad and g_emb[c][j] = the same sum over the rows of label c; accumulate != 0
 *                                ADDS onto both.  Any nf % 4 == 0 up to 1024; ws = n * nf floats.  Two launches: per-row partial sums, then
 *                                their sum over the rows in ascending order (for n = 64 the additions are ctgan_gp_head_wgrad's, in its order). */
int ctgan_tail_critic_heads_fwd_proj(const float* y, int32_t B, int32_t hw, int32_t nf, const float* w_out, const float* b_out,
                                     const float* emb, int32_t n_labels, const int32_t* labels, float* gp, const float* slopes,
                                     float gp_lambda, float lambda2, float M, float* f, float* d, float* ct_i, float* out,
                                     ctgan_stream_t stream);
int ctgan_tail_heads_bwd_proj(const float* y, const float* d, const float* f, const int32_t* labels, const float* ct_i, const float* gout,
                              int32_t n_gout, int32_t B, int32_t hw, int32_t nf, float lambda2, float M, float mask_scale,
                              const float* w_out, const float* emb, int32_t n_labels, float* gy, float* gw_out, float* gb_out, float* g_emb,
                              const float* y_gp, int32_t n_gp, float* gz_gp, ctgan_stream_t stream);
int ctgan_gen_heads_fwd_proj(const float* y, int32_t n, int32_t hw, int32_t nf, const float* w_out, const float* b_out, const float* emb,
                             int32_t n_labels, const int32_t* labels, float* f, float* d, float* out, ctgan_stream_t stream);
/* ---- Hinge objective (NOT in the reference): the ResNet critic's fused output stage for L_D = mean_i hinge(1 - D(x_i)) + mean_i hinge(1 +
 * D(G(z_i))) [+ acgan_scale * CE(class head of the real rows)], hinge(t) = t >= 0 ? t : 0 - the row workgroup and the one-workgroup finish of
 * ctgan_tail_critic_heads_fwd / ctgan_tail_heads_bwd without the consistency and penalty parts.  ONE entry pair: the projection table
 * emb [n_labels,nf] (a row's weight is w_out + emb[labels[r % B]]) and the class head w_ac [nf,ncls], b_ac are optional operands, NULL = absent;
 * both non-NULL: CTGAN_E_BADARG.  y [2B][hw][nf] dense channels-last = relu(dropout(z)), rows [0,B) real, [B,2B) fake; labels [B] (needed with
 * either operand; a label outside the table is the caller's error, as for the _proj entries).  nf % 4 == 0, nf <= 1024, y / gy 16-byte aligned.
 *   fwd (two launches): f [2B,nf] = mean_hw y, d [2B], a [2B,ncls]; probs [B,ncls] and ce_i [B] on the real rows; acc[2] as ctgan_accuracy2 on a
 *     (the step's own, dropped-out rows); out[5] = {hinge + acgan_scale * acgan, hinge, hinge_real, hinge_fake, acgan}.  Without the class head
 *     a, probs, ce_i, acc are not touched and acgan = 0.
 *   bwd (one launch), gout = device scalar: gd_r = -gout [1 - d_r >= 0] / B (real rows), +gout [1 + d_r >= 0] / B (fake rows);
 *     ga = gout acgan_scale (probs - onehot) / B on the real rows; gy = (y > 0) (gd_r (w_out + emb[label]) + W_ac ga_r) / hw * mask_scale;
 *     gw_out [nf] = sum_r f_r gd_r, gb_out [1] = sum_r gd_r, gw_ac [nf,ncls], gb_ac [ncls], g_emb [n_labels,nf] (every element written; a class
 *     no row carries gets exact zeros).  Every sum: one wave, lanes over the rows in ascending order, no atomics - the same bits on every run. */
int ctgan_tail_hinge_heads_fwd(const float* y, int32_t B, int32_t hw, int32_t nf, const float* w_out, const float* b_out, const float* emb,
                               int32_t n_labels, const float* w_ac, const float* b_ac, int32_t ncls, const int32_t* labels, float acgan_scale,
                               float* f, float* d, float* a, float* probs, float* ce_i, float* acc, float* out, ctgan_stream_t stream);
int ctgan_tail_hinge_heads_bwd(const float* y, const float* d, const float* f, const float* probs, const int32_t* labels, const float* gout,
                               int32_t B, int32_t hw, int32_t nf, int32_t ncls, float acgan_scale, float mask_scale, const float* w_out,
                               const float* emb, int32_t n_labels, const float* w_ac, float* gy, float* gw_out, float* gb_out, float* g_emb,
                               float* gw_ac, float* gb_ac, ctgan_stream_t stream);
int ctgan_gen_heads_bwd_proj(const float* y, const int32_t* labels, const float* gout, int32_t n, int32_t hw, int32_t nf, float mask_scale,
                             const float* w_out, const float* emb, int32_t n_labels, float* gy, ctgan_stream_t stream);
int ctgan_gp_head_grad_proj(const float* y, const float* w_out, const float* emb, const int32_t* labels, int32_t n_labels, int32_t n,
                            int32_t hw, int32_t nf, float mask_scale, float* gz, ctgan_stream_t stream);
int ctgan_gp_head_wgrad_proj(const float* gg, const float* y, const int32_t* labels, int32_t n_labels, int32_t n, int32_t hw, int32_t nf,
                             float mask_scale, float* gw, float* g_emb, float* ws /* n * nf floats */, int accumulate,
                             ctgan_stream_t stream);
/* ACGAN accuracies of the clean critic pass (:249-266): logits [2B,ncls] (real rows, then fake rows); acc[2]   */
int ctgan_accuracy2(const float* logits, const int32_t* labels, int32_t B, int32_t ncls, float* acc,
                    ctgan_stream_t stream);

/* ---- optimizer (K21): tf.train.AdamOptimizer on a flat buffer
 *      (TF/CT_gan_cifar_resnet.py:333-338).  `state` = device float[4]: {lr, beta1^t, beta2^t, skipped};
 *      the kernel reads lr and the running beta powers from it (graph-replay safe) and
 *      ctgan_adam_advance multiplies the powers after all buckets of a step are applied.  An element whose scaled gradient is not
 *      finite (NaN / inf: an overflow of the fp16 matrix-core mode, a degenerate input) keeps its weight and slots unchanged - one
 *      inf would otherwise poison m, v and theta for good, also at lr = 0 (build-only safeguard; TF would propagate it) - and
 *      state[3] is incremented by one per skipped element (float accumulator, exact to 2^24), so the caller can see it.
 *
 *      Every update entry point (ctgan_adam_step, ctgan_rmsprop_step and their _packed forms) takes two optional operands, both
 *      build-only (NOT in the reference) and both fused into the one launch; all argument rules are checked before any launch.
 *      avg, avg_rate - generator weight averaging (Yazici et al. 2019).  avg == NULL with avg_rate == 0: no average.  avg != NULL with
 *        avg_rate in (0, 1]: after the update - after the clip, and also for an element whose non-finite gradient was skipped -
 *        avg = avg + avg_rate * (theta - avg), two fp32 roundings, identical in the plain and the packed form; theta, the slots, the
 *        bucket and state come out bit-identical to the call without it.  avg == NULL with any other rate, or avg != NULL with a rate
 *        outside (0, 1] (NaN included): CTGAN_E_BADARG.  The packed forms also want a non-NULL avg 16-byte aligned (CTGAN_E_UNSUPPORTED).
 *      scaler - the dynamic loss scale of the fp16 matrix-core mode, device float[4] {S, found, good, skipped} (see
 *        ctgan_grads_nonfinite below).  NULL: none.  Otherwise grad_scale / scaler[0] stands for grad_scale - exact, S being a power of
 *        two: bit-identical to the call without a scaler given that quotient - and, when scaler[1] != 0, the WHOLE update is dropped:
 *        no theta, m, v, ms changes (the RMSProp clip still clips, the average still moves towards the weights as they are, the packed
 *        forms still write the bucket) and state[3] does not count its elements.  The per-element skip stays in place on the steps
 *        that are applied.                                                                                                    ------ */
int ctgan_adam_step(float* theta, const float* g, float* m, float* v, int64_t n, float* state, float beta1, float beta2, float eps,
                    float grad_scale, float* avg, float avg_rate, const float* scaler, ctgan_stream_t stream);
int ctgan_adam_advance(float* state, float beta1, float beta2, ctgan_stream_t stream);
/* tf.train.RMSPropOptimizer (decay rho, momentum 0, not centered) on a flat buffer, with an optional fused weight clip
 * (TF/CT_gan_mnist.py:134-143, TF/CT_gan_64x64.py:548-558):  ms += (g^2 - ms) (1 - rho);  theta = clip(theta - lr g / sqrt(ms + eps))
 * with g = grad * grad_scale, lr = state[0] (graph-replay safe), clip(x) = min(max(x, -clip), clip) when clip > 0 (no clip otherwise).
 * TF creates the ms slot at ONES: the caller initialises it so.  A non-finite scaled gradient leaves the element's ms unchanged and its
 * weight only clipped, and adds one to state[3], as ctgan_adam_step.  avg, avg_rate, scaler: as ctgan_adam_step.  The packed form =
 * ctgan_pack + the update in one launch (n_tensors <= 64, 16-byte aligned flat buffers), bit-identical to ctgan_pack +
 * ctgan_rmsprop_step.                                                                                                             */
int ctgan_rmsprop_step(float* theta, const float* g, float* ms, int64_t n, float* state, float rho, float eps, float clip,
                       float grad_scale, float* avg, float avg_rate, const float* scaler, ctgan_stream_t stream);
int ctgan_rmsprop_step_packed(const float* const* srcs, const int64_t* dst_offs, const int64_t* counts, int32_t n_tensors, float* flat,
                              float* theta, float* ms, float* state, float rho, float eps, float clip, float grad_scale, float* avg,
                              float avg_rate, const float* scaler, ctgan_stream_t stream);
/* End of a step in one launch.  scaler == NULL (growth_interval, min_scale, max_scale ignored): ctgan_adam_advance(state) and, with
 * rng_ctr != NULL, ctgan_rng_advance(rng_ctr, rng_by).  scaler != NULL, the end of a step under the dynamic loss scale - applied
 * (scaler[1] == 0): the beta powers advance, good += 1, and at growth_interval in a row S = min(2 S, max_scale), good = 0; dropped: the
 * beta powers stay, S = max(S / 2, min_scale), good = 0, skipped += 1; either way found = 0 and rng_ctr advances.  Then
 * growth_interval >= 1 and min_scale <= max_scale, both powers of two (CTGAN_E_BADARG otherwise).                                 */
int ctgan_step_advance(float* state, float beta1, float beta2, uint64_t* rng_ctr, uint64_t rng_by, float* scaler, int64_t growth_interval,
                       float min_scale, float max_scale, ctgan_stream_t stream);
/* ctgan_pack + ctgan_adam_step in one launch (n_tensors <= 64, 16-byte aligned flat buffers; CTGAN_E_UNSUPPORTED otherwise):
 * compute_gradients' bucket and apply_gradients (TF/CT_gan_cifar_resnet.py:335-338) of a single-rank step.  flat receives the
 * packed gradients as ctgan_pack writes them; theta/m/v are updated with bit-identical arithmetic to the two-launch form.        */
int ctgan_adam_step_packed(const float* const* srcs, const int64_t* dst_offs, const int64_t* counts, int32_t n_tensors, float* flat,
                           float* theta, float* m, float* v, float* state, float beta1, float beta2, float eps, float grad_scale, float* avg,
                           float avg_rate, const float* scaler, ctgan_stream_t stream);
/* flat[dst_offs[i] : dst_offs[i] + counts[i]] = srcs[i][0:counts[i]] (srcs[i] == NULL: zeros), i < n_tensors, in one
 * launch per 64 tensors.  The three arrays are HOST arrays (the pointers are device pointers); they are passed to
 * the kernel by value, so the call is hipGraph-capture safe.  This is the gradient bucket of compute_gradients
 * (TF/CT_gan_cifar_resnet.py:335-336) without one copy per variable.                                   */
int ctgan_pack(const float* const* srcs, const int64_t* dst_offs, const int64_t* counts, int32_t n_tensors,
               float* flat, ctgan_stream_t stream);
/* Swap the contents of two disjoint fp32 buffers of n elements in one launch (16-byte accesses when both pointers are 16-byte
 * aligned, with the n % 4 last elements one by one; element by element otherwise; n == 0: nothing is launched; overlapping
 * buffers: CTGAN_E_BADARG): the weights and their average change places without either address changing.                         */
int ctgan_exchange(float* a, float* b, int64_t n, ctgan_stream_t stream);
/* The scan of the dynamic loss scale.  scaler = device float[4] {S, found, good, skipped}: S the power-of-two scale the step's backward
 * is seeded with (the caller reads scaler[0] as the seed), found != 0 once this step's gradients held a NaN / inf, good = updates
 * applied in a row since S last changed, skipped = updates dropped so far (float counts, exact to 2^24).  A step is three launches -
 * this scan, an update with `scaler`, ctgan_step_advance with `scaler` - all stream-ordered, none reads the host.
 * ctgan_grads_nonfinite: scaler[1] = 1 if any element of the n_tensors (<= 64) sources is NaN or +-inf (raw bits: +-FLT_MAX, denormals
 * and -0 are finite); a NULL source is all zeros.  One source = the flat bucket after the all-reduce.  16-byte loads between a
 * source's first and last 16-byte boundary.  ctgan_grads_nonfinite_blocks: grid.x of that launch (its workgroups hold 256 threads,
 * each reads one 16-byte item per trip; grid.y = n_tensors), for the largest count and the number of sources.                         */
unsigned ctgan_grads_nonfinite_blocks(int64_t max_count, int32_t n_tensors);
int ctgan_grads_nonfinite(const float* const* srcs, const int64_t* counts, int32_t n_tensors, float* scaler, ctgan_stream_t stream);

/* ---- RNG: Philox4x32-10 counter-based streams (tf.random_uniform / tf.random_normal /
 *      dropout masks :157,202,277,319).  counter base is read from device memory
 *      (`ctr[0]`, advanced by ctgan_rng_advance) so captured graphs draw fresh numbers. -------- */
/* tf.nn.dropout with its mask drawn inside the kernel: y[i] = x[i]/keep * floor(keep + u_i), where u_i is what
 * ctgan_rng_uniform(out, n, seed, stream_id, ctr, 0, 1) writes to out[i].  The backward (and its backward) is the
 * same call on the gradient with the same (seed, stream_id, ctr) - no mask tensor is stored.              */
int ctgan_dropout_rng(const float* x, float* y, int64_t n, float keep, uint64_t seed, uint64_t stream_id,
                      const uint64_t* ctr, ctgan_stream_t stream);
/* ctgan_dropout_rng followed by ctgan_lrelu_bwd(., ref, alpha = 0) in one pass: y (NULL = not wanted) = dropout(x),
 * y_masked = y where ref > 0, else 0.  x, ref, y, y_masked share one physical layout.                        */
int ctgan_dropout_rng_mask(const float* x, const float* ref, float* y, float* y_masked, int64_t n, float keep, uint64_t seed,
                           uint64_t stream_id, const uint64_t* ctr, ctgan_stream_t stream);
/* LeakyReLU + dropout in one pass (TF/CT_gan_cifar.py:84-98, TF/CT_gan_mnist.py:92-100: `dropout(LeakyReLU(conv))`): y = x * (ref > 0 ? 1 :
 * alpha) / keep * floor(keep + u_i), draws as ctgan_dropout_rng.  Forward: ref = x.  Backward (and its backward): x = the arriving gradient,
 * ref = the forward result (kept values carry the pre-activation's sign, dropped ones are multiplied by 0).  One physical layout.     */
int ctgan_lrelu_dropout_rng(const float* x, const float* ref, float* y, int64_t n, float alpha, float keep, uint64_t seed,
                            uint64_t stream_id, const uint64_t* ctr, ctgan_stream_t stream);
/* The same over TWO tensors laid end to end: elements [0, n1) draw stream_id, elements [n1, n) draw stream_id2 indexed from n1 (n1 % 4 == 0) -
 * each part gets the draws a launch of its own would make (TF/CT_gan_cifar.py:84-98 evaluated once on [real, fake, real | x_hat]).        */
int ctgan_lrelu_dropout_rng2(const float* x, const float* ref, float* y, int64_t n, int64_t n1, float alpha, float keep, uint64_t seed,
                             uint64_t stream_id, uint64_t stream_id2, const uint64_t* ctr, ctgan_stream_t stream);
int ctgan_rng_uniform(float* out, int64_t n, uint64_t seed, uint64_t stream_id, const uint64_t* ctr,
                      float lo, float hi, ctgan_stream_t stream);
int ctgan_rng_normal(float* out, int64_t n, uint64_t seed, uint64_t stream_id, const uint64_t* ctr,
                     ctgan_stream_t stream);
/* labels = (int32)(u*nlab), u~U[0,1)   (tf.cast(tf.random_uniform*10, int32) :319)             */
int ctgan_rng_labels(int32_t* out, int64_t n, int32_t nlab, uint64_t seed, uint64_t stream_id,
                     const uint64_t* ctr, ctgan_stream_t stream);
int ctgan_rng_advance(uint64_t* ctr, uint64_t by, ctgan_stream_t stream);
/* Critic-step input preparation in one launch (TF/CT_gan_cifar_resnet.py:201-202,226,277-283): rf [2b,d] = [real ; fake]
 * with real = 2*(x_int/denom - .5) + U[lo,hi) (stream sid_deq, element i), interp [b,d] = real + alpha*(fake - real) with
 * alpha[row] = U[0,1) (stream sid_alpha, element row) - the same draws as ctgan_rng_uniform on [b,d] and [b,1] tensors
 * followed by ctgan_real_prep, ctgan_interpolate and a concat.  d % 4 == 0.                                              */
int ctgan_critic_prep(const int32_t* x_int, const float* fake, int32_t b, int32_t d, uint64_t seed, uint64_t sid_deq,
                      uint64_t sid_alpha, const uint64_t* ctr, float lo, float hi, float denom, float* rf, float* interp,
                      ctgan_stream_t stream);
/* ctgan_critic_prep without the interpolation (the hinge objective's critic step has no x_hat): rf [2b,d] = [2*(x_int/denom - .5) + U[lo,hi) ;
 * fake] in one launch, the draws those of ctgan_rng_uniform on [b,d] at (seed, stream_id, ctr).  d % 4 == 0, 16-byte aligned pointers.       */
int ctgan_real_fake_prep(const int32_t* x_int, const float* fake, int32_t b, int32_t d, uint64_t seed, uint64_t stream_id,
                         const uint64_t* ctr, float lo, float hi, float denom, float* rf, ctgan_stream_t stream);
/* dst [n_src + n_extra rows] = tf.nn.dropout([src ; src[0:n_extra]], keep) in one launch (input of the critic tail for the
 * two dropout passes, pass 2 on the real half only, :226-227); draws as ctgan_dropout_rng on the concatenated tensor;
 * keep = 1: plain concat.  rows_cat_bwd: the concat's adjoint gsrc[r] = g[r] + g[n_src + r] (r < n_extra).                */
int ctgan_rows_cat_dropout(const float* src, int64_t n_src, int64_t n_extra, int64_t row_elems, float keep, uint64_t seed,
                           uint64_t stream_id, const uint64_t* ctr, float* dst, ctgan_stream_t stream);
int ctgan_rows_cat_bwd(const float* g, int64_t n_src, int64_t n_extra, int64_t row_elems, float* gsrc, ctgan_stream_t stream);
/* The same with n_pass further rows behind the concat that pass straight through: g = [a (n_src) ; a' (n_extra) ; c (n_pass)] ->
 * gsrc [n_src + n_pass rows] = [a + a' ; c].  One launch for the step from the critic tail's merged backward (rows real, fake |
 * real' | x_hat: the two dropout passes of :226-227 and the penalty pass of :283-284) to the trunk's (rows real, fake, x_hat).  */
int ctgan_rows_cat_bwd2(const float* g, int64_t n_src, int64_t n_extra, int64_t n_pass, int64_t row_elems, float* gsrc,
                        ctgan_stream_t stream);
/* General form: dst = concatenation of up to CTGAN_ROW_SEGMENTS row segments of src (segment i = rows [src_row0,
 * src_row0 + rows)), each with its own tf.nn.dropout (keep >= 1: none) whose Philox element index is counted from dst row
 * index_row0 (<= the segment's first dst row): segments that share index_row0 and stream_id reproduce the dropout of their
 * own concatenated tensor.  Builds the inputs of all critic tails of a step (dropout passes, clean pass, gradient-penalty
 * pass) in one launch.                                                                                                     */
#define CTGAN_ROW_SEGMENTS 6
typedef struct ctgan_row_segment {
    int64_t src_row0, rows;
    float keep;
    uint64_t stream_id;
    int64_t index_row0;
} ctgan_row_segment;
int ctgan_rows_gather_dropout(const float* src, const ctgan_row_segment* segs, int32_t nseg, int64_t row_elems, uint64_t seed,
                              const uint64_t* ctr, float* dst, ctgan_stream_t stream);


/* ---- semi-supervised CT classifier (csrc/ssl.hip; TH/ = CT-GANs/Theano_classifier) ---------------------------------------
 * Weight-normalised dense layer (TH/nn.py:398-430; the generator's l2normalize, :250-264): w[i,j] = theta[i,j] * s[j] * rnorm[j],
 * rnorm[j] = 1 / sqrt(eps + sum_i theta[i,j]^2) over the [in, out] row-major theta.  eps = 0 for the classifier's DenseLayer,
 * 1e-6 for l2normalize.  The backward takes the saved rnorm:  d_j = sum_i gw_ij theta_ij,  gs_j = d_j rnorm_j (gs may be NULL),
 * gtheta_ij = s_j rnorm_j (gw_ij - theta_ij d_j rnorm_j^2).                                                                 */
int ctgan_wn_fwd(const float* theta, const float* s, int32_t in, int32_t out, float eps, float* w, float* rnorm,
                 ctgan_stream_t stream);
int ctgan_wn_bwd(const float* gw, const float* theta, const float* s, const float* rnorm, int32_t in, int32_t out, float* gtheta,
                 float* gs, ctgan_stream_t stream);
/* Epilogue of a dense layer followed by a GaussianNoiseLayer (TH/nn.py:428-430, :232-244) in one launch after the GEMM:
 * a = y + bias (bias may be NULL), relu != 0: a = max(a, 0); h = a + sigma * N(0,1).  Element (r, c) of the [rows, cols]
 * tensor draws value (row_offset + r) * cols + c of the stream ctgan_rng_normal(., seed, stream_id, ctr) writes, so a pass that
 * is a row block of a stacked batch draws what a launch of its own would.  sigma = 0: no draw (deterministic pass).  `a` (may be
 * NULL) receives the pre-noise activation.  bias = NULL, relu = 0 is the input noise site x + sigma N.  No noise tensor is
 * written.  The backward: gz = gh + ga (either may be NULL) kept where y + bias > 0 (relu != 0), gb_j = sum_i gz_ij (may be NULL). */
int ctgan_dense_noise_fwd(const float* y, const float* bias, int64_t rows, int32_t cols, int32_t relu, float sigma, uint64_t seed,
                          uint64_t stream_id, const uint64_t* ctr, int64_t row_offset, float* h, float* a, ctgan_stream_t stream);
int ctgan_dense_noise_bwd(const float* gh, const float* ga, const float* y, const float* bias, int64_t rows, int32_t cols,
                          int32_t relu, float* gz, float* gb, ctgan_stream_t stream);
/* Data-dependent init of one weight-normalised layer (TH/nn.py:421-426), in place on the pre-activation y = x W [rows, cols]:
 * y <- (y - mean_j) / stdv_j (then relu), stdv_j the root mean square of the centred column; s_j <- s_j / stdv_j,
 * b_j <- -mean_j / stdv_j.                                                                                                   */
int ctgan_wn_init(float* y, int64_t rows, int32_t cols, int32_t relu, float* s, float* b, ctgan_stream_t stream);
/* Loss head of the classifier step (TH/CT_MNIST.py:70-90) over logits [4b, nc] = [labelled ; unlabelled ; unlabelled, second
 * noisy pass ; generated]:  out4 = { loss_lab, loss_unl, CT, train_err },  ct_i [b] = mean_k (softmax(unl) - softmax(unl2))^2,
 * CT = mean_i max(lam2 ct_i - m, 0), loss_unl = (CT - mean lse(unl) + mean softplus(lse(unl)) + mean softplus(lse(fake))) / 2.
 * Max-subtracted log-sum-exp, softplus(t) = max(t,0) + log1p(exp(-|t|)).  The backward writes the [4b, nc] cotangent of
 * gout[0] * loss_lab + gout[1] * loss_unl (gout: device float[>= 2]).                                                        */
int ctgan_ssl_head_fwd(const float* logits, const int32_t* labels, int32_t b, int32_t nc, float lam2, float m, float* out4,
                       float* ct_i, ctgan_stream_t stream);
int ctgan_ssl_head_bwd(const float* logits, const int32_t* labels, const float* gout, int32_t b, int32_t nc, float lam2, float m,
                       float* glogits, ctgan_stream_t stream);
/* Feature matching (TH/CT_MNIST.py:92-94) over f [2b, c] = [f(G(z)) ; f(x)]: diff_j = mean_i f_ij - mean_i f_(b+i)j,
 * loss = mean_j diff_j^2; the backward: gf = +-gout * 2 diff_j / (c b).                                                      */
int ctgan_featmatch_fwd(const float* f, int32_t b, int32_t c, float* loss, float* diff, ctgan_stream_t stream);
int ctgan_featmatch_bwd(const float* diff, const float* gout, int32_t b, int32_t c, float* gf, ctgan_stream_t stream);
/* Batch norm of a [b, c] activation with batch statistics, an offset and no gain (TH/nn.py:194-216, batch_norm(g=None)):
 * xhat = (x - mean_j) rstd_j, rstd_j = 1 / sqrt(eps + var_j); y = xhat + offset_j, act = 1: y = softplus(xhat + offset_j).     */
int ctgan_bn2d_fwd(const float* x, const float* offset, int32_t b, int32_t c, float eps, int32_t act, float* y, float* xhat,
                   float* rstd, ctgan_stream_t stream);
int ctgan_bn2d_bwd(const float* gy, const float* xhat, const float* offset, const float* rstd, int32_t b, int32_t c, int32_t act,
                   float* gx, float* goffset, ctgan_stream_t stream);
/* Theano-form Adam (TH/nn.py:30-47) on flat buffers with the parameter average of TH/CT_MNIST.py:104-105 fused:
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; theta -= lr (m / (1 - b1^t)) / sqrt(v / (1 - b2^t) + eps) - eps INSIDE the
 * root -; avg += avg_rate (theta - avg) (avg may be NULL).  state = {lr, b1^t, b2^t, skipped} as ctgan_adam_step's.           */
int ctgan_adam_theano_step(float* theta, const float* g, float* m, float* v, float* avg, int64_t n, float* state, float beta1,
                           float beta2, float eps, float avg_rate, ctgan_stream_t stream);


/* ---- convolutional semi-supervised CT classifier (csrc/ssl_conv.hip; TH/CT_CIFAR.py) -----------------------------------------
 * Weight norm of a filter whose output axis is in the middle (TH/nn.py:70-81, Deconv2DLayer): theta [outer, out, inner] row-major
 * (a [k,k,out,in] transposed-conv filter: outer = k k, inner = in), w[a,o,i] = theta[a,o,i] * s[o] * rnorm[o],
 * rnorm[o] = 1 / sqrt(eps + sum_{a,i} theta[a,o,i]^2).  The backward has the contract of ctgan_wn_bwd (saved rnorm, gs may be NULL). */
int ctgan_wn_mid_fwd(const float* theta, const float* s, int32_t outer, int32_t out, int32_t inner, float eps, float* w, float* rnorm,
                     ctgan_stream_t stream);
int ctgan_wn_mid_bwd(const float* gw, const float* theta, const float* s, const float* rnorm, int32_t outer, int32_t out,
                     int32_t inner, float* gtheta, float* gs, ctgan_stream_t stream);
/* Data-dependent init of a weight-normalised conv / NIN / dense layer (TH/nn.py:85-95) in place on the channels-last
 * pre-activation y [rows = N H W, cols = C]: m_c the column mean, inv_c = init_stdv / sqrt(mean_i (y_ic - m_c)^2);
 * y <- act((y - m_c) inv_c) - no b is added in this pass -; g_c <- g_c inv_c; b_c <- -m_c inv_c.
 * act: 0 identity, 1 LeakyReLU with `slope`, 2 tanh.                                                                           */
int ctgan_wn_init_map(float* y, int64_t rows, int32_t cols, int32_t act, float slope, float init_stdv, float* g, float* b,
                      ctgan_stream_t stream);
/* Feature consistency (TH/CT_CIFAR.py:120) over the features f [4b, fdim] of [labelled ; unlabelled ; unlabelled, second pass ;
 * generated]: out2[0] = mean_{i,j} (f[b+i,j] - f[2b+i,j])^2; with logits [4b, nc] (may be NULL) out2[1] = train_err2 =
 * mean_{i<b} (max_k logits[i,k] <= 0) (:128), else 0.  The backward writes the [4b, fdim] cotangent of gout[0] * out2[0].       */
int ctgan_featcons_fwd(const float* f, const float* logits, int32_t b, int32_t fdim, int32_t nc, float* out2, ctgan_stream_t stream);
int ctgan_featcons_bwd(const float* f, const float* gout, int32_t b, int32_t fdim, float* gf, ctgan_stream_t stream);
/* L1 feature matching (TH/CT_CIFAR.py:152-156) over f [2b, c]: diff_j = mean_i f_ij - mean_i f_(b+i)j, loss = mean_j |diff_j|;
 * the backward: gf = +-gout sign(diff_j) / (c b), zero where diff_j = 0.                                                        */
int ctgan_featmatch_l1_fwd(const float* f, int32_t b, int32_t c, float* loss, float* diff, ctgan_stream_t stream);
int ctgan_featmatch_l1_bwd(const float* diff, const float* gout, int32_t b, int32_t c, float* gf, ctgan_stream_t stream);
/* Augmenting gather (TH/CT_CIFAR.py:48, :211-265): output row r is a win x win window of image idx[r] of the uint8 set
 * data [n_data, channels, size, size], reflect-padded by `pad` through index arithmetic, flipped horizontally or not, each byte
 * converted through the 256-entry float table `lut`.  In the reference's orientation out[c,y,x] = P'[c, oy + y, ox + x] with P'
 * the padded image after the flip.  augment != 0: flip = u[3r] > 0.5, oy = min(int((2 pad + 1) u[3r+1]), 2 pad), ox the same of
 * u[3r+2], u the stream ctgan_rng_uniform(., seed, stream_id, ctr) writes (win <= size); augment == 0: off_y, off_x, flip as given
 * (the window must lie inside the padded image).  rot180 != 0 writes the window rotated by 180 degrees; channels_last != 0 writes
 * rows of [win, win, channels], else [channels, win, win].  An index outside [0, n_data) reads nothing and writes NaN.         */
int ctgan_aug_gather(const uint8_t* data, const int32_t* idx, int32_t n_data, int32_t rows, int32_t channels, int32_t size,
                     int32_t pad, int32_t win, int32_t augment, int32_t off_y, int32_t off_x, int32_t flip, int32_t rot180,
                     int32_t channels_last, const float* lut, uint64_t seed, uint64_t stream_id, const uint64_t* ctr, float* out,
                     ctgan_stream_t stream);


/* ---- temporal-ensembling CT classifier (csrc/ssl_te.hip; TH/CT_CIFAR-10_TE.py) ------------------------------------------------
 * Loss head of the classifier step (:102-126) over logits [3b, nc] and features [3b, fdim] = [labelled ; unlabelled ; generated],
 * the consistency term taken against the rows idx[i] (int32 [b]) of the device tables targets [n, nc] (raw ensembled logits,
 * softmaxed here) and targets2 [n, fdim], read by index inside the kernel:  ct_i = mean_k (softmax(unl_i) - softmax(t_i))_k^2,
 * ctf_i = mean_j (f_ij - t2_ij)^2, CT_i = lam2 (ct_i + feat_w ctf_i) - m, CT_ = mean_i max(CT_i, 0),
 * loss_unl = (CT_ - mean lse(unl) + mean softplus(lse(unl)) + mean softplus(lse(fake))) / 2;
 * out8 = { loss_lab, loss_unl, CT_, train_err, train_err2, mean ct, mean ctf, 0 }.  The same launch stores the unlabelled logits
 * and feature rows into pred[idx[i]] [n, nc] and pred2[idx[i]] [n, fdim] (:300-302) with plain stores: the indices of a batch
 * are distinct by contract (slices of a permutation); duplicates are memory-safe, the surviving row unspecified.  Numerics as
 * ctgan_ssl_head_fwd.  A label outside [0, nc) makes loss_lab NaN and reads nothing; an index outside [0, n) makes loss_unl, CT_,
 * mean ct and mean ctf NaN and reads and writes no table row.  Fixed-order reductions, no atomics.  The backward writes the
 * cotangents glogits [3b, nc] and gfeat [3b, fdim] of gout[0] * loss_lab + gout[1] * loss_unl (gout: device float[>= 2]),
 * recomputed from the logits, features and target rows (the targets are constants); gfeat is exactly 0 on the labelled and
 * generated rows; an unlabelled row with an index outside [0, n) gets NaN.                                                     */
int ctgan_te_head_fwd(const float* logits, const float* feat, const int32_t* labels, const int32_t* idx, const float* targets,
                      const float* targets2, int32_t b, int32_t nc, int32_t fdim, int32_t n, float lam2, float feat_w, float m,
                      float* out8, float* pred, float* pred2, ctgan_stream_t stream);
int ctgan_te_head_bwd(const float* logits, const float* feat, const int32_t* labels, const int32_t* idx, const float* targets,
                      const float* targets2, const float* gout, int32_t b, int32_t nc, int32_t fdim, int32_t n, float lam2,
                      float feat_w, float m, float* glogits, float* gfeat, ctgan_stream_t stream);
/* Epoch-end update of one table triple of n elements (:305-309, :273-274): ens = decay ens + (1 - decay) pred,
 * targets = ens inv_corr with inv_corr = 1 / (1 - decay^(epoch + 1)) formed by the caller in double precision, pred = 0.
 * float4 accesses where the three pointers are 16-byte aligned, a scalar tail.                                                  */
int ctgan_te_ensemble_update(float* ens, float* targets, float* pred, int64_t n, float decay, float inv_corr, ctgan_stream_t stream);


/* ---- classifier score of CIFAR-10 samples (csrc/score_cifar.hip; score_cifar.py) ------------------------------------------------
 * The path between a generator and the score of TF/tflib/inception_score.py:60-69 under the CT classifier (ct_cifar.py), kept on
 * the device.
 * Generator output x [n, channels size size] (NCHW flat) -> the classifier's internal input: out logical [n, channels, size, size],
 * channels-last, rotated by 180 degrees, out = lut[byte] with byte what ctgan_pixels_u8 computes for that element - bit-equal to
 * ctgan_pixels_u8 -> NHWC to NCHW -> ctgan_aug_gather(rows 0..n-1, win = size, offsets (pad, pad), no flip, rot180, channels_last). */
int ctgan_score_input(const float* x, int64_t n, int32_t channels, int32_t size, float scale, const float* lut, float* out,
                      ctgan_stream_t stream);
/* Streaming score statistic over the logits [m, classes] of the chunk of global rows [r0, r0 + m) of n, n >= splits.  Row g
 * belongs to split k with k n / splits <= g < (k + 1) n / splits (integer division: score_from_probabilities' slices).  Caller-owned,
 * caller-zeroed state: acc double [splits, classes + 1], cnt int64 [2 classes].  Per row in fp64: lp = z - max - log sum exp(z - max),
 * p = exp(lp); acc[k, j] += p_j; acc[k, classes] += sum_j p_j lp_j (a p that underflowed to 0 adds exactly 0; a non-finite logit
 * makes the row's terms NaN); cnt[argmax] += 1 (first maximum, as numpy.argmax) and, with labels (int32 [m], may be NULL),
 * cnt[classes + label] += 1 where argmax == label.  One workgroup per split; fp64 partials per thread, an LDS tree in a fixed
 * order, one thread adds into acc with plain loads and stores; integer adds for cnt.  Successive chunks are ordered by the stream.
 * classes > 32: CTGAN_E_UNSUPPORTED, nothing is launched.                                                                         */
int ctgan_score_accum(const float* logits, int64_t m, int32_t classes, int64_t r0, int64_t n, int32_t splits, const int32_t* labels,
                      double* acc, int64_t* cnt, ctgan_stream_t stream);
/* acc -> out double [2 + splits]: out[2 + k] = exp(acc[k, classes] / n_k - sum_j m_j log m_j), m_j = acc[k, j] / n_k (a term with
 * m_j = 0 is 0), n_k the split's length; out[0] their mean, out[1] their population standard deviation.  One workgroup.          */
int ctgan_score_finish(const double* acc, int64_t n, int32_t splits, int32_t classes, double* out, ctgan_stream_t stream);
/* Streaming raw moments of a feature layer (csrc/moments.hip), for the classifier Frechet distance of score_cifar.py: f fp32 [m, d]
 * row-major; s1[a] += sum_i f[i, a], s2[a, b] += sum_i f[i, a] f[i, b] in fp64, s2 the full symmetric [d, d].  Caller-owned,
 * caller-zeroed state, 8-byte aligned; successive chunks are ordered by the stream.  The fp32 -> fp64 conversions and the fp64
 * products are exact: the only roundings are those of the sums.  One workgroup per pair (ti <= tj) of 16-column tiles on
 * v_mfma_f64_16x16x4_f64, four waves with a fixed quarter of the rows each, folded through LDS in wave order; every state element
 * has one owning workgroup, which adds with a plain load and store (no atomics): the same chunking gives the same bits, and s2 is
 * exactly symmetric.  m == 0: nothing is launched.  d > 1024: CTGAN_E_UNSUPPORTED, nothing is launched.                          */
int ctgan_moments_accum(const float* f, int64_t m, int32_t d, double* s1, double* s2, ctgan_stream_t stream);
/* The same moments segmented by a label column, for the per-class Frechet distance of score_cifar.py: labels int32 [m]; caller-owned,
 * caller-zeroed state cnt int64 [classes], s1 double [classes, d], s2 double [classes, d, d], 8-byte aligned.  With R_c the chunk's
 * rows of label c in ascending row order: cnt[c] += |R_c|, s1[c] += sum f_i, s2[c] += sum f_i f_i^T over R_c.  A label outside
 * [0, classes) belongs to no class and adds to nothing (the caller sees it in cnt).  One launch, grid (tile pairs, classes): every
 * workgroup compacts its class's rows into an LDS list (wave ballots, a prefix over the waves: stable), then runs the loop of
 * ctgan_moments_accum through the list - one body, a row indirection the only difference.  Contract: after a call the state of
 * class c holds the bits ctgan_moments_accum leaves from the [|R_c|, d] array of those rows gathered in order; an absent class's
 * state is not touched.  No atomics, one owner per state element.  m == 0: nothing is launched.
 * m > ctgan_class_moments_max_rows() (8192, the LDS list), classes > 32 or d > 1024: CTGAN_E_UNSUPPORTED, nothing is launched.    */
int ctgan_class_moments_max_rows(void);
int ctgan_class_moments_accum(const float* f, const int32_t* labels, int64_t m, int32_t d, int32_t classes, int64_t* cnt, double* s1,
                              double* s2, ctgan_stream_t stream);
/* conf[labels[i], argmax(logits[i, :])] += 1 over logits fp32 [m, classes], labels int32 [m], into the caller-owned, caller-zeroed
 * conf int64 [classes, classes] (conditioned label x predicted class).  The argmax is ctgan_score_accum's (first maximum, as
 * numpy.argmax); a row with a label outside [0, classes) is ignored.  LDS integer counters per workgroup, then integer adds: exact
 * in any order.  m == 0: nothing is launched.  classes > 32: CTGAN_E_UNSUPPORTED, nothing is launched.                           */
int ctgan_confusion_accum(const float* logits, const int32_t* labels, int64_t m, int32_t classes, int64_t* conf, ctgan_stream_t stream);
/* The k-nearest-neighbour manifold estimate in a feature space (csrc/knn.hip), for the precision and recall of score_cifar.py.  The
 * squared distance is d2(i, j) = max(0, |a_i|^2 + |b_j|^2 - 2 a_i . b_j), every term in fp64 over the fp32 features widened exactly; the
 * dot products and both norms run on v_mfma_f64_16x16x4_f64 through the same k-ordered chain, so two bit-identical rows are at
 * d2 == 0.0 exactly and bit-identical rows of b give bit-identical distances.  A workgroup owns 64 rows of a and streams b through
 * LDS; no [m, n] array, no atomics, one owner per output element: two runs give the same bits.  Features are finite by precondition;
 * a NaN distance compares false - never a neighbour, never covering.
 * ctgan_knn_radii: f fp32 [n, d] row-major -> r2 fp64 [n], r2[i] the squared distance from row i to its k-th nearest OTHER row (self
 * is excluded by index: a bit-identical duplicate elsewhere counts, at distance 0).  k < 1 or n < k + 1: CTGAN_E_BADARG;
 * k > ctgan_knn_max_k() (8) or d > 1024: CTGAN_E_UNSUPPORTED; nothing is launched either way.
 * ctgan_knn_cover: a fp32 [m, d], b fp32 [n, d], r2_b fp64 [n] or NULL -> covered int32 [m] = 1 iff some j has d2(i, j) <= r2_b[j]
 * (not written, and may be NULL, when r2_b is NULL), nn_d2 fp64 [m] = min_j d2(i, j), nn_idx int32 [m] = the LOWEST j attaining it
 * (all distances NaN: +inf and -1).  m == 0: nothing is launched.  n < 1: CTGAN_E_BADARG.  d > 1024: CTGAN_E_UNSUPPORTED.        */
int ctgan_knn_max_k(void);
int ctgan_knn_radii(const float* f, int64_t n, int32_t d, int32_t k, double* r2, ctgan_stream_t stream);
int ctgan_knn_cover(const float* a, int64_t m, const float* b, int64_t n, int32_t d, const double* r2_b, int32_t* covered, double* nn_d2,
                    int32_t* nn_idx, ctgan_stream_t stream);
/* The all-pairs polynomial-kernel sums of the unbiased kernel distance of score_cifar.py (csrc/kid.hip).  a fp32 [m, d], b fp32 [n, d]
 * row-major -> sums fp64 [ceil(m / T), ceil(n / T)] row-major, T = ctgan_kernel_tile() (64):
 *   sums[p][q] = sum over i in [T p, min(T p + T, m)), j in [T q, min(T q + T, n)) of (gamma a_i . b_j + coef0)^3,
 * without the pairs i == j (by global index) when exclude_diag != 0 - the caller passes a == b then, and m != n is CTGAN_E_BADARG.
 * Every term is fp64 over the fp32 features widened exactly: the dot products run on v_mfma_f64_16x16x4_f64 (exact products, only the
 * sums round), then v = gamma dot + coef0 and v v v in fp64.  Padded rows and the excluded diagonal are masked by index.  The grid is
 * (tiles of a) x (slabs of consecutive tiles of b), the slab length chosen so that few rows of a still fill the chip; every element of
 * sums has one owning workgroup and one summation order that does not depend on the slab length: the same bits for every grid shape
 * and every run.  No atomics, no [m, n] array.  m < 1, n < 1, d < 1, more than 2^30 rows or a null pointer: CTGAN_E_BADARG;
 * d > 1024: CTGAN_E_UNSUPPORTED; nothing is launched either way.                                                                  */
int ctgan_kernel_tile(void);
int ctgan_kernel_tile_sums(const float* a, int64_t m, const float* b, int64_t n, int32_t d, double gamma, double coef0, int32_t exclude_diag,
                           double* sums, ctgan_stream_t stream);
/* The same three kernels per class of CLASS-SORTED operands, one launch for every class (csrc/knn.hip, csrc/kid.hip), for the per-class
 * precision, recall and kernel distance of score_cifar.py.  An operand's rows of class 0 come first, then class 1, ..., in their original
 * order inside a class; seg int32 [classes + 1], device-resident, holds the segment starts: class c is rows [seg[c], seg[c + 1]) and
 * rows at or behind seg[classes] belong to no class and are never read as operands.  (A kernel clamps what it reads of seg into
 * [0, rows]: a wrong array gives wrong numbers, never an access outside the operand.)  No count is needed on the host: the grid is
 * ceil(rows of a / 64) + classes workgroups, each scans seg for its (class, tile of the class's rows of a), and a surplus workgroup
 * returns at once.  The bodies are the pooled kernels' on the segment's bases and counts, so class c receives the BITS the pooled entry
 * point leaves from the gathered rows of class c; no atomics, one owner per output element, the same bits on every run.
 * ctgan_knn_radii_seg: f fp32 [n, d], seg -> r2 fp64 [n] in sorted order: the squared distance of row i to its k-th nearest other row OF
 * ITS OWN CLASS; +inf for a row whose class has fewer than k + 1 rows (the selection never fills; the caller masks such classes); rows
 * at or behind seg[classes] are not written.  n == 0: nothing is launched.
 * ctgan_knn_cover_seg: row i of class c of a [m, d] against the rows of class c of b [n, d] only, r2_b fp64 [n] (sorted order) or NULL ->
 * covered int32 [m], nn_d2 fp64 [m], nn_idx int32 [m] as ctgan_knn_cover, nn_idx counting from the start of the class's segment of b.
 * A class with no rows in b: covered 0, nn_d2 +inf, nn_idx -1, and nothing of b or r2_b is read (n == 0 is such a call, b may be NULL).
 * m == 0: nothing is launched.
 * ctgan_kernel_tile_sums_seg: class c's tile matrix [ceil(m_c / T), ceil(n_c / T)] of ctgan_kernel_tile_sums is stored row-major at
 * sums[toff[c] : toff[c + 1]]; toff int64 [classes + 1], device-resident, the caller's exclusive prefix sums of
 * ceil(m_c / T) ceil(n_c / T); sums holds at least toff[classes] elements ((ceil(m / T) + classes) (ceil(n / T) + 1) always suffices)
 * and elements no class owns are not written.  exclude_diag != 0 drops i == j by the index INSIDE the class and needs a == b,
 * seg_a == seg_b, m == n (else CTGAN_E_BADARG).  grid.y is the slab count at the pooled bound ceil(n / T); a workgroup whose slab
 * starts past its class's tiles returns.
 * All three: classes outside 1..32 or d > 1024 (radii: k > ctgan_knn_max_k()): CTGAN_E_UNSUPPORTED for the upper limits,
 * CTGAN_E_BADARG below 1; a null pointer or an fp64 / int64 array that is not 8-byte aligned: CTGAN_E_BADARG; nothing is launched.
 * ctgan_segment_sums: out[s] = the fp64 sum of vals[off[s] : off[s + 1]], off int64 [segments + 1]: one workgroup per segment, thread
 * t of 256 adds elements t, t + 256, ... in index order, then an LDS tree - one fixed order that does not depend on the grid: the
 * same bits on every run.  An empty segment gives 0.  It turns the ragged tile sums into per-class totals (a cumsum difference would
 * round against the total of all classes).  segments == 0: nothing is launched.                                                   */
int ctgan_knn_radii_seg(const float* f, const int32_t* seg, int32_t classes, int64_t n, int32_t d, int32_t k, double* r2, ctgan_stream_t stream);
int ctgan_knn_cover_seg(const float* a, const int32_t* seg_a, int64_t m, const float* b, const int32_t* seg_b, int64_t n, int32_t classes, int32_t d,
                        const double* r2_b, int32_t* covered, double* nn_d2, int32_t* nn_idx, ctgan_stream_t stream);
int ctgan_kernel_tile_sums_seg(const float* a, const int32_t* seg_a, int64_t m, const float* b, const int32_t* seg_b, int64_t n, int32_t classes,
                               int32_t d, double gamma, double coef0, int32_t exclude_diag, const int64_t* toff, double* sums, ctgan_stream_t stream);
int ctgan_segment_sums(const double* vals, const int64_t* off, int32_t segments, double* out, ctgan_stream_t stream);

/* ---- differentiable augmentation of the critic's inputs (csrc/diffaug.hip; Zhao et al. 2020 - NOT in the reference) --------------
 * The policy `color,translation,cutout` on flat NCHW fp32 images [n, c, h, w], one workgroup per image.  Exactly one of x (fp32) and
 * x_int (int32 pixels, forward only: converted on load as 2 (v / denom - .5), bit-equal to ctgan_real_prep followed by this call) is
 * given.  policy is a bit mask: 1 colour, 2 translation, 4 cutout; 0 copies.  Image r takes values 8r .. 8r+7 of the uniform stream
 * ctgan_rng_uniform(., seed, stream_id, ctr) writes: u0..u2 brightness b = u0 - .5, saturation s = 2 u1, contrast q = u2 + .5; u3, u4
 * the shift ty = min(int((2 S_h + 1) u3), 2 S_h) - S_h with S_h = int(h/8 + .5) (tx: u4, w); u5, u6 the centre of the cut rectangle
 * oy = min(int(n_h u5), n_h - 1), rows [oy - k_h/2, oy - k_h/2 + k_h) clipped to the image, k_h = int(h/2 + .5),
 * n_h = h + (1 - k_h % 2) (columns: u6, w).  A bit that is off fixes its parameters at the identity.
 * adjoint = 0, the forward: x1 = x + b; x2 = s x1 + (1-s) mean_c(x1); x3 = q x2 + (1-q) (mean(x) + b);
 *   y[c,i,j] = x3[c,i-ty,j-tx] where that pixel exists and (i,j) is not cut, else 0.
 * adjoint = 1 (input: the gradient g of y): gt[c,i,j] = g[c,i+ty,j+tx] where that pixel exists and is not cut, else 0;
 *   gx = q (s gt + (1-s) mean_c(gt)) + (1-q) mean(gt).
 * adjoint = 2: the forward without the brightness (b = 0) - the linear part of T, which is the adjoint of the adjoint.
 * The image mean is summed in one fixed order (per lane serially, then an LDS tree; diffaug.hip's header): the same bits on every run.
 * params (may be NULL) [n, 8] receives per image (b, s, q, ty, tx, y0, x0, policy): y0 / x0 the first cut row / column, h / w when
 * nothing is cut.  A null y, both or neither of x / x_int, x_int with adjoint = 1, n, c, h, w < 1, c > 16, policy > 7,
 * stream_id >= 2^32 or denom == 0: CTGAN_E_BADARG, nothing is launched.                                                           */
int ctgan_diffaug(const float* x, const int32_t* x_int, float denom, float* y, int32_t n, int32_t c, int32_t h, int32_t w,
                  uint32_t policy, int32_t adjoint, uint64_t seed, uint64_t stream_id, const uint64_t* ctr, float* params,
                  ctgan_stream_t stream);

/* ---- spectral normalisation of the weight matrices of a flat parameter bucket (csrc/spectral.hip; Miyato et al. 2018 - NOT in the
 * reference) -------------------------------------------------------------------------------------------------------------------
 * A job is one normalised parameter: `K x N` floats at bucket offset `off`, read row-major as M[K, N]; its state is u[N], v[K] and
 * sigma.  The jobs of a bucket are described ONCE by a table of ctgan_spectral_table_words(njobs) int64 words that
 * ctgan_spectral_table_fill writes on the host (off / K / N: int64 [njobs], ascending and non-overlapping inside a bucket of `total`
 * floats) and the caller copies to the device: per job its offsets into the packed u (sum of the N before it), v (sum of the K) and
 * sigma (its index) arrays, its rows per slice and the prefix that flattens (job, row slice) into one grid; word 0 is njobs, word 1
 * the slice count `nslices` the two operators are given back, ctgan_spectral_scratch_bytes(table) the scratch both need (floats, no
 * alignment beyond 4 bytes; not preserved between calls).  N > ctgan_spectral_max_n() (4096): CTGAN_E_UNSUPPORTED from the fill,
 * so before any launch; K is unbounded (the slices of a bucket: fewer than 2^31).  eps = 1e-12.
 * ctgan_spectral_normalize, iterate != 0: three launches -
 *   t = M u;  v = t / max(|t|, eps);  s = M^T v;  sigma = |s|;  u <- s / max(sigma, eps);  theta_bar = M / max(sigma, eps) inside
 *   a job and a copy of theta outside one.  iterate == 0: the last launch alone (u, v, sigma are read only).
 * ctgan_spectral_grad: two launches - over each job, gbar <- (gbar - <gbar, Mbar> v u^T) / max(sigma, eps), Mbar the job's part of
 *   theta_bar; elements no job owns are not touched.
 * Dynamic loss scale: scaler (the float[4] state of the update launches) and hold (one float) are both given or both NULL.  With
 *   them ctgan_spectral_grad also copies the flag scaler[1] into hold[0]; ctgan_spectral_normalize given that hold (may be NULL)
 *   skips the iteration when hold[0] != 0 - the update in between was dropped, there is no new weight version - and only rewrites
 *   theta_bar from the unchanged sigma: u, v, sigma and theta_bar keep their bits.  Only one of the two: CTGAN_E_BADARG.
 * Every sum has one fixed order relative to its job: the same bits on every run, at any offset and in any company.  theta and
 * theta_bar are 16-byte aligned and distinct; the table is 8-byte aligned; a null pointer or njobs < 1: CTGAN_E_BADARG.          */
int ctgan_spectral_max_n(void);
int64_t ctgan_spectral_table_words(int32_t njobs);
int ctgan_spectral_table_fill(const int64_t* off, const int64_t* K, const int64_t* N, int32_t njobs, int64_t total, int64_t* table);
size_t ctgan_spectral_scratch_bytes(const int64_t* table);
int ctgan_spectral_normalize(const float* theta, float* theta_bar, int64_t total, const int64_t* table, int32_t njobs, int64_t nslices,
                             float* u, float* v, float* sigma, float* scratch, int32_t iterate, const float* hold, ctgan_stream_t stream);
int ctgan_spectral_grad(float* gbar, const float* theta_bar, const int64_t* table, int32_t njobs, int64_t nslices, const float* u,
                        const float* v, const float* sigma, float* scratch, const float* scaler, float* hold, ctgan_stream_t stream);

/* ---- self-attention core and its gated residual (csrc/attention.hip; NOT in the reference) ----------------------------------
 * Dense rows: q, k [n, N, dk], v, out, gout [n, N, dv], lse, delta [n, N], all fp32; q, k, v, out, gout 16-byte aligned.
 * ctgan_attention_fwd: out[b, i, :] = sum_j softmax_j(q[b, i] . k[b, j]) v[b, j, :] (no 1 / sqrt(dk) scale; the row maximum is
 *   subtracted before exp), lse[b, i] = log sum_j exp(q[b, i] . k[b, j]); lse may be NULL (no backward will follow).  One launch.
 * ctgan_attention_bwd: P = exp(S - lse), delta_i = gout_i . out_i, dS = P o (gout v^T - delta); gq = dS k, gk = dS^T q,
 *   gv = P^T gout.  Two launches: one over query blocks owns gq (and writes delta, the [n, N] scratch of the second), one over key
 *   blocks owns gk and gv.
 * The [N, N] scores exist in registers and LDS only; products on the exact-fp32 MFMA; no atomics, the same bits on every run, an
 * image's rows independent of the rest of the launch.  N a multiple of 16 (at least 16), dk a multiple of 4 in [4, 64], dv a
 * multiple of 16 in [16, 128]: anything else CTGAN_E_BADARG naming the operand.
 * ctgan_attn_residual_fwd: y = x + gamma[0] o over n elements (gamma is read on the device).
 * ctgan_attn_residual_bwd: go = gamma[0] gy, ggamma[0] = sum gy o in one fixed order (fp64 partial sums in `part`, 8-byte aligned,
 *   ctgan_attn_residual_parts() doubles, then a plain store); the gradient of x is gy itself.  Two launches.                    */
int ctgan_attention_fwd(const float* q, const float* k, const float* v, float* out, float* lse, int64_t n, int32_t N, int32_t dk, int32_t dv,
                        ctgan_stream_t stream);
int ctgan_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout, float* gq,
                        float* gk, float* gv, float* delta, int64_t n, int32_t N, int32_t dk, int32_t dv, ctgan_stream_t stream);
int ctgan_attn_residual_parts(void);
int ctgan_attn_residual_fwd(const float* x, const float* o, const float* gamma, float* y, int64_t n, ctgan_stream_t stream);
int ctgan_attn_residual_bwd(const float* gy, const float* o, const float* gamma, float* go, float* ggamma, double* part, int64_t n,
                            ctgan_stream_t stream);
/* The second derivative: the backward of ctgan_attention_bwd, with a, b, c the cotangents of gq, gk, gv (shaped like them,
 * 16-byte aligned, never NULL: the host passes zeros for an absent one) and lse, delta the rows that ctgan_attention_bwd read / wrote.
 *   T = a k^T + q b^T, dP = gout v^T, tau_i = sum_j P T, Pc = P c, rho_i = sum_j P T dP - 2 tau_i delta_i + gout_i . (Pc)_i,
 *   W = P o (T - tau), Sbar = P o (T o dP - dP tau - T delta + gout c^T - rho), dS = P o (dP - delta);
 *   dq = Sbar k + dS b, dgout = W v + Pc, dk = Sbar^T q + dS^T a, dv = W^T gout.
 * Two launches: one over query blocks (a first key sweep for tau, rho, Pc, a second for dq and dgout; tau, rho go to the [n, N] scratch
 * rows `tau`, `rho`), one over key blocks for dk and dv.  The same shape contract and the same properties as the first derivative.
 * ctgan_attn_residual_bwd2: the backward of ctgan_attn_residual_bwd with cgo / cgg the cotangents of go / ggamma: dgy = gamma[0] cgo +
 *   cgg[0] o, d_o = cgg[0] gy, dgamma[0] = sum cgo gy (the partial sums of ctgan_attn_residual_bwd).  gamma and cgg are read on the
 *   device; cgg may be NULL (zero), then d_o may be NULL and is not written.  Two launches.                                       */
int ctgan_attention_bwd2(const float* q, const float* k, const float* v, const float* lse, const float* delta, const float* gout, const float* a,
                         const float* b, const float* c, float* dq, float* dk, float* dv, float* dgout, float* tau, float* rho, int64_t n,
                         int32_t N, int32_t dk_width, int32_t dv_width, ctgan_stream_t stream);
int ctgan_attn_residual_bwd2(const float* cgo, const float* gy, const float* o, const float* gamma, const float* cgg, float* dgy, float* d_o,
                             float* dgamma, double* part, int64_t n, ctgan_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CTGAN_HIP_H */
