/* mdd_hip.h -- C ABI of libmdd_hip.so: the MI355X (gfx950) engine for the hot path of
 * kushal-bhargav/multimodal_dataset_distillation: distill.py's inner `syn_steps` unrolled
 * training + bi-trajectory matching loop.
 *
 * Plain pointers and sizes only; all `*_dev` pointers are DEVICE pointers (hipMalloc'ed /
 * torch.Tensor.data_ptr()), `stream` is a hipStream_t cast to void* (NULL = default stream).
 * Every function returns 0 on success; on failure it returns non-zero and `mdd_last_error()`
 * describes it.  HIP out-of-memory is reported with the substring "out of memory" so the
 * reference's OOM handling (distill.py:525-545, 568-575 matches on that substring) keeps
 * working when the Python host re-raises it as RuntimeError.
 *
 * Reference interface each entry point replaces (file:line in /root/reference):
 *   mdd_engine_create / _param_*     student construction CLIPModel_full + ReparamModule x2
 *                                    distill.py:440-442, reparam_module.py:18-75 (flatten order)
 *   mdd_img_forward                  img_student_net(x, flat_param=theta)   distill.py:524
 *                                    -> ReparamModule.forward reparam_module.py:148-159
 *                                    -> ImageEncoder.forward networks.py:678-682 (timm nfnet_l0)
 *   mdd_txt_forward                  txt_student_net(y, flat_param=theta)   distill.py:537
 *                                    -> ProjectionHead.forward networks.py:639-646
 *   mdd_contrastive                  x/||x||, y/||y||, syn_lr_img * x @ y.T, symmetric CE
 *                                    distill.py:533,546-551
 *   mdd_img_backward / mdd_txt_backward
 *                                    torch.autograd.grad(loss, theta, create_graph=True)
 *                                    distill.py:562-567
 *   mdd_*_tangent_forward/backward   the double-backward that grand_loss.backward() performs
 *                                    through those gradients, distill.py:606
 *   mdd_flat_*                       theta' = theta - lr*g (:582-583), sum-MSE (:588-595),
 *                                    SGD momentum step (:233-241, :611-613)
 *   mdd_unrolled_match               the whole iteration distill.py:509-606 in one call
 */
#ifndef MDD_HIP_H
#define MDD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDD_DTYPE_F32 0  /* fp32 storage + exact-fp32 MFMA (parity mode)                    */
#define MDD_DTYPE_BF16 1 /* bf16 activations/weights, bf16 MFMA, fp32 accumulate, fp32 theta */
#define MDD_DTYPE_BF16X2 2 /* fp32 storage; every contraction operand split into hi+lo bf16 (16
                              significand bits), bf16 MFMA with fp32 accumulate: the fast mode that
                              meets the 1e-3 parity bar                        */
#define MDD_DTYPE_F32_BF16OPS 3 /* experiment: fp32 storage, operands rounded to ONE bf16 (hi only):
                                   separates stash rounding from MFMA operand rounding            */

typedef struct mdd_engine mdd_engine;

typedef struct mdd_config {
  const char* variant; /* "nfnet_l0" | "nfnet_l1" | "nfnet_tiny" | "nf_resnet50" | "nf_resnet_tiny" | "nf_regnet_b1" |
                          "nf_regnet_tiny" | "vit_b16" | "vit_tiny16" | "vit_tiny16_cls" | "vit_micro" | "vit_micro_cls" |
                          "clip_vit_b32" | "clip_vit_micro" | "clip_vit_nano" */
  int32_t batch;       /* pairs per inner step (mini_batch_size, distill.py:511)          */
  int32_t num_queries; /* rows of image_syn / text_syn (distill.py:630)                    */
  int32_t image_size;  /* square input, multiple of 32                                     */
  int32_t d_txt;       /* text embedding dim (768 for BERT, networks.py:824)               */
  int32_t syn_steps;   /* number of activation stashes kept (unroll depth)                 */
  int32_t dtype;       /* MDD_DTYPE_*                                                      */
  int32_t keep_steps;  /* activation stash policy of mdd_unrolled_match: the first keep_steps inner
                          steps keep their forward/backward activations in HBM for the reverse sweep;
                          the others share ONE stash slot and are recomputed (forward + inner
                          gradient at the kept theta_k) when the sweep reaches them.  < 0 or
                          >= syn_steps: keep every step (no recompute).  Workspace shrinks from
                          syn_steps+1 to keep_steps+2 activation sets.              */
} mdd_config;

const char* mdd_last_error(void);
/* ABI version of this header: 2 = round 2 (mdd_config.keep_steps, MDD_DTYPE_BF16X2 / _F32_BF16OPS,
 * profile kind 4); 3 = + mdd_comm_* / mdd_allreduce_syn_grads; 4 = + the ViT building-block ops; 5 = + mdd_engine_set_pass_precision; 6 = + mdd_op_conv2d_wgrad2, mdd_set_pipe_kernels; 7 = + mdd_op_maxpool2d_3s2; 8 = + mdd_set_group8_kernels, mdd_op_mid_se; 9 = + mdd_set_se_fused; 10 = + mdd_op_linear, mdd_op_pool_se; 11 = + mdd_op_weight_std, mdd_op_text_head,
 * mdd_op_contrastive refuses what its kernels cannot take; 12 = + mdd_op_image_edge, mdd_op_vit_glue, mdd_op_lin_pack,
 * mdd_op_resid, mdd_flat_dot / _scale_out / _sub_inplace / _lambda_init / _match_finalize / _d2f / _accum_f2d; 13 = +
 * in-engine dropout masks (mdd_iter_args.drop_p / drop_iteration / drop_seed, mdd_txt_forward_rng, mdd_op_dropout_mask,
 * mdd_sizeof_iter_args); still 13 (new symbols only, no struct changed): + mdd_op_quick_gelu / mdd_op_quick_gelu_bwd and the
 * CLIP ViT variants; still 13 (new symbols only, no struct changed): + the frozen CLIP text tower (mdd_text_tower_*,
 * mdd_op_attention_causal, mdd_op_token_embed, mdd_op_eot_gather); still 13: + the frozen BERT text tower over packed
 * sequences (mdd_text_tower_encode_varlen, mdd_op_attention_varlen, mdd_op_bert_embed).  mdd_text_tower_config gained
 * max_tokens at its end: a binding compares mdd_sizeof_text_tower_config() with its own struct, as it does
 * mdd_sizeof_iter_args(); still 13 (new symbol only): + mdd_set_skip_unused_param_grads.  A binding built against
 * another version must refuse to load. */
#define MDD_ABI_VERSION 13
int mdd_version(void);
/* The wide bf16 pointwise contractions (>= 768 channels in and out, >= 8192 rows: the ViT linears) run on 256 x 256-tile
 * pipelined kernels; 0 routes them to the general kernels instead (process-wide; returns the previous setting).  For the
 * parity tests, which compare an iteration both ways, and for A/B timing. */
int mdd_set_pipe_kernels(int enable);
/* The bf16 grouped 3x3 convolutions with 8 channels per group (NF-RegNet's conv2): forward and data gradient run on a
 * dedicated kernel (csrc/conv_g8.hip) for the geometries where it measured faster (1, the default); 0 routes them all to
 * the general kernels, 2 routes every such geometry to the dedicated kernel (process-wide; returns the previous setting).
 * For the parity tests, which run the same geometry both ways, and for A/B timing. */
int mdd_set_group8_kernels(int enable);
/* The NFNet image walker applies the squeeze-excite gate, the residual add and the next pre-activation in conv3's forward
 * epilogue (1, the default); 0 = conv3 writes C3 and a separate elementwise kernel applies the gate (process-wide; returns
 * the previous setting).  Both give the same bits in the forward passes.  For the parity tests, which run a pass both
 * ways, and for A/B timing. */
int mdd_set_se_fused(int enable);
/* mdd_unrolled_match does not compute the parameter gradients that nothing reads (1, the default): the Hessian-vector
 * product of reverse step 0, after which lambda is dead, and the inner gradient of a step the stash policy recomputes,
 * whose g_k is kept from the forward sweep.  The data gradients of those passes run launch for launch as before.  0 = every
 * backward pass computes its parameter gradients (process-wide; returns the previous setting).  The op-level entry points
 * (mdd_img_backward, mdd_img_tangent_backward, mdd_txt_*) always compute them.  For the parity tests and for A/B timing. */
int mdd_set_skip_unused_param_grads(int enable);

/* ---- engine lifetime and memory (the caller owns device memory: PyTorch caching allocator) */
int mdd_engine_create(const mdd_config* cfg, mdd_engine** out);
void mdd_engine_destroy(mdd_engine* e);
int64_t mdd_engine_workspace_bytes(const mdd_engine* e);
int mdd_engine_bind_workspace(mdd_engine* e, void* ws_dev, int64_t bytes, void* stream);

/* ---- parameter table in reference flatten order (reparam_module.py:28-39).  which: 0 = image
 * encoder, 1 = text projection.  shape4 is right-padded with 1s; ndim in *ndim. */
int64_t mdd_engine_param_numel(const mdd_engine* e, int which);
int mdd_engine_param_count(const mdd_engine* e, int which);
int mdd_engine_param_info(const mdd_engine* e, int which, int index, char* name, int name_cap,
                          int64_t* shape4, int* ndim, int64_t* offset);
int mdd_engine_feature_dim(const mdd_engine* e);
/* named stash buffer lookup for tests: byte offset into the bound workspace */
int mdd_engine_find_buffer(const mdd_engine* e, const char* name, int slot, int64_t* byte_offset,
                           int64_t* elems, int* is_float32);

/* ---- image encoder passes (slot = inner step index whose activations are kept) */
int mdd_img_forward(mdd_engine* e, int slot, const float* theta_dev, const float* image_syn_dev,
                    const int64_t* idx_dev, float* feat_out_dev, void* stream);
/* gtheta = J_theta^T feat_bar.  If dimage_accum_dev != NULL also
 * dimage_accum[idx] += coef*mul * J_image^T feat_bar.  stash != 0 keeps the backward signals of
 * this slot for the tangent pass (the inner-gradient call); stash == 0 leaves them untouched (a
 * second backward through the same forward, as the outer backward of distill.py:606 performs). */
int mdd_img_backward(mdd_engine* e, int slot, const float* theta_dev, const float* feat_bar_dev,
                     float* gtheta_out_dev, float* dimage_accum_dev, const int64_t* idx_dev,
                     const float* coef_dev, float mul, int stash, void* stream);
int mdd_img_tangent_forward(mdd_engine* e, int slot, const float* theta_dev,
                            const float* theta_dot_dev, float* feat_dot_out_dev, void* stream);
/* dimage_accum[idx] += coef*mul * d/d(image) ; coef_dev may be NULL (=1) */
int mdd_img_tangent_backward(mdd_engine* e, int slot, const float* theta_dev,
                             const float* theta_dot_dev, const float* feat_bar_dot_dev,
                             float* htheta_out_dev, float* dimage_accum_dev,
                             const int64_t* idx_dev, const float* coef_dev, float mul,
                             void* stream);

/* ---- text projection passes; drop_mask_dev: [batch, feat] already scaled by 1/(1-p), or NULL */
int mdd_txt_forward(mdd_engine* e, int slot, const float* theta_dev, const float* text_syn_dev,
                    const int64_t* idx_dev, const float* drop_mask_dev, float* feat_out_dev,
                    void* stream);
/* The same pass with the dropout mask DRAWN BY THE ENGINE (reference networks.py:636,643: Dropout(p) in train mode).
 * Nothing is stored: the slot remembers (p, seed, step, iteration, idx_dev) and mdd_txt_backward, mdd_txt_tangent_forward
 * and mdd_txt_tangent_backward of that slot draw the same mask again, so idx_dev must stay valid until the last of them.
 * The mask (normative; tests/dropout_refs.py restates it): Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53,
 * 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85), key = (seed low word, seed high word), counter = (column / 4, sample,
 * step, iteration), output word column % 4 belongs to `column`; sample = (uint32_t)idx_dev[row], or row when idx_dev is
 * NULL (a shard that runs some rows of a minibatch draws exactly those rows of the unsharded mask); u = (word >> 8) *
 * 2^-24, keep iff u >= p, mask = keep ? 1.0f / (1.0f - p) : 0.  p in [0, 1), 0 = no dropout; anything else (NaN too) is
 * "invalid argument" before anything is launched.  The call keeps no state of its own: the same arguments give the same
 * mask on any engine. */
int mdd_txt_forward_rng(mdd_engine* e, int slot, const float* theta_dev, const float* text_syn_dev,
                        const int64_t* idx_dev, float p, uint64_t seed, uint32_t step, uint32_t iteration,
                        float* feat_out_dev, void* stream);
/* That mask itself, [n, d] fp32 (to inspect it, or to inject it through drop_mask_dev / mdd_iter_args.drop_masks);
 * idx_dev int64 [n] or NULL.  Same argument checks. */
int mdd_op_dropout_mask(float p, uint64_t seed, uint32_t step, uint32_t iteration, int n, int d,
                        const int64_t* idx_dev, float* out_dev, void* stream);
int mdd_txt_backward(mdd_engine* e, int slot, const float* theta_dev, const float* feat_bar_dev,
                     float* gtheta_out_dev, float* dtext_accum_dev, const int64_t* idx_dev,
                     const float* coef_dev, float mul, int stash, void* stream);
int mdd_txt_tangent_forward(mdd_engine* e, int slot, const float* theta_dev,
                            const float* theta_dot_dev, float* feat_dot_out_dev, void* stream);
int mdd_txt_tangent_backward(mdd_engine* e, int slot, const float* theta_dev,
                             const float* theta_dot_dev, const float* feat_bar_dot_dev,
                             float* htheta_out_dev, float* dtext_accum_dev, const int64_t* idx_dev,
                             const float* coef_dev, float mul, void* stream);

/* ---- contrastive head: loss + d/dx, d/dy, d/dscale; tangent variant when x_dot/y_dot given.
 * scale_dev NULL => scale_const is used (upstream distill_original.py:430 behaviour). */
int mdd_contrastive(mdd_engine* e, const float* x_dev, const float* y_dev, const float* scale_dev,
                    float scale_const, float* loss_dev, float* xbar_dev, float* ybar_dev,
                    float* sbar_dev, void* stream);
int mdd_contrastive_tangent(mdd_engine* e, const float* x_dev, const float* y_dev,
                            const float* x_dot_dev, const float* y_dot_dev, const float* scale_dev,
                            float scale_const, float* xbar_dot_dev, float* ybar_dot_dev,
                            float* sbar_dot_dev, void* stream);

/* The same head without an engine, for any row count: sample-sharded runs (SURVEY 8e mode B, what
 * `--distributed` / nn.DataParallel does at distill.py:443-445, 515-517) evaluate it on the all-gathered
 * [n, d] features of every rank.  x_dot/y_dot NULL: loss, xbar, ybar, sbar; non-NULL: their directional
 * derivatives into the same output pointers (loss unused).  work: mdd_op_contrastive_workspace_floats(n, d).
 * Refused with "invalid argument" before anything is launched (mdd_contrastive / _tangent refuse the same): d > 4096 (the
 * feature-gradient kernel keeps 16 x 256 features of a row in registers), n > 4092 (the cross-entropy kernel's (4 n + 16)
 * floats of LDS must fit the 64 KiB a workgroup may ask for), an n whose n * n does not fit an int. */
int64_t mdd_op_contrastive_workspace_floats(int n, int d);
int mdd_op_contrastive(int n, int d, const float* x_dev, const float* y_dev, const float* x_dot_dev,
                       const float* y_dot_dev, const float* scale_dev, float scale_const, float* work_dev,
                       float* loss_dev, float* xbar_dev, float* ybar_dev, float* sbar_dev, void* stream);

/* ---- flat fp32 parameter streams */
int mdd_flat_axpy(float* out_dev, const float* x_dev, const float* g_dev, const float* lr_dev,
                  float sign, int64_t n, void* stream);       /* out = x + sign*lr*g */
int mdd_flat_sqdist(const float* a_dev, const float* b_dev, double* out_dev, int64_t n,
                    void* stream);                             /* out[0] += sum (a-b)^2 */
int mdd_flat_sgd_momentum(float* p_dev, const float* g_dev, float* buf_dev, float lr, float mom,
                          int first, int64_t n, void* stream);
/* the same step, a no-op when skip_flag_dev[0] != 0: the reference leaves its loop on a NaN loss BEFORE the
 * optimiser steps (distill.py:599-613); with the decision taken on the device the host can enqueue the next
 * iteration without first reading this one's loss back */
int mdd_flat_sgd_momentum_guarded(float* p_dev, const float* g_dev, float* buf_dev, float lr,
                                  float mom, int first, int64_t n, const float* skip_flag_dev,
                                  void* stream);

/* the reverse sweep's kernels over the same streams (the vector kernels move float4: 16-byte aligned pointers) */
int mdd_flat_dot(const float* a_dev, const float* b_dev, double* out_dev, double sign, int64_t n,
                 void* stream);                                /* out[0] += sign * <a, b>, accumulated in double */
int mdd_flat_scale_out(float* y_dev, const float* x_dev, const float* coef_dev, float mul, int64_t n,
                       void* stream);                          /* y = coef[0] * mul * x; coef a device scalar or NULL (= 1) */
int mdd_flat_sub_inplace(float* y_dev, const float* x_dev, int64_t n, void* stream);       /* y -= x */
/* lam = (float)(2 / dist0[0]) * (thK - tgt): d grand_loss / d theta_K (distill.py:588-597), dist0 a device double */
int mdd_flat_lambda_init(float* lam_dev, const float* thK_dev, const float* tgt_dev, const double* dist0_dev, int64_t n,
                         void* stream);
/* s4 = {img_numer, img_denom, txt_numer, txt_denom} (double) -> out3 = {s0/s1 + s2/s3, s0/s1, s2/s3} (distill.py:596-598) */
int mdd_flat_match_finalize(const double* s4_dev, float* out3_dev, void* stream);
/* the scalar hand-overs: out[i] = (accum ? out[i] : 0) + (float)(in[i] * mul) for i < n, 1 <= n <= 64 (one wave; out is
 * not read when accum == 0);  out[0] += sign * (double)in[0] */
int mdd_flat_d2f(float* out_dev, const double* in_dev, float mul, int accum, int n, void* stream);
int mdd_flat_accum_f2d(double* out_dev, const float* in_dev, double sign, void* stream);

/* ---- one whole outer iteration (reference distill.py:509-606) */
typedef struct mdd_iter_args {
  const float* image_syn;    /* [num_queries,3,S,S] fp32 NCHW                                  */
  const float* text_syn;     /* [num_queries,d_txt]                                            */
  const float* lr_img;       /* device scalar syn_lr_img (also the logit scale, distill.py:548) */
  const float* lr_txt;       /* device scalar syn_lr_txt                                       */
  const float* theta0_img;   /* expert start  (distill.py:473-476)                             */
  const float* theta0_txt;
  const float* target_img;   /* expert target (distill.py:469-472)                             */
  const float* target_txt;
  const int64_t* perms;      /* [syn_steps, batch] minibatch indices (distill.py:510-511)      */
  const float* drop_masks;   /* [syn_steps, batch, feat] or NULL                               */
  int32_t syn_steps;
  int32_t use_lr_as_scale;   /* 1: fork behaviour (:548); 0: use logit_scale_const             */
  float logit_scale_const;
  float* grad_image_syn;     /* out, same shape as image_syn (overwritten)                     */
  float* grad_text_syn;      /* out                                                            */
  float* grad_lr;            /* out [2]: d/d lr_img, d/d lr_txt                                */
  float* losses;             /* out [3 + syn_steps]: grand, img, txt, contrastive per step     */
  /* used when drop_masks == NULL and drop_p > 0: the engine draws step k's mask itself (mdd_txt_forward_rng with
   * step = k, idx = perms + k * batch) in the forward, the inner gradient, both tangent passes and the recomputed
   * steps of keep_steps.  drop_p outside [0, 1), or drop_masks together with drop_p > 0: "invalid argument" */
  float drop_p;
  uint32_t drop_iteration;   /* the outer iteration: counter word 3                            */
  uint64_t drop_seed;
} mdd_iter_args;
/* sizeof(mdd_iter_args) as the library was built: a binding checks its own layout against it */
size_t mdd_sizeof_iter_args(void);
int mdd_unrolled_match(mdd_engine* e, const mdd_iter_args* a, void* stream);

/* ---- per-kernel HIP-event timing of the contraction launches (bench.py roofline accounting).
 * kind: 0 = conv_gemm 128x32 tile, 1 = conv_gemm 256x64, 2 = conv_gemm 128x128, 3 = conv_wgrad (the
 * contraction kernel alone), 4 = the split-M reduce kernel that follows each conv_wgrad.
 * out4 = {launches, total milliseconds, algorithmic FLOPs, algorithmic bytes} since enable. */
int mdd_engine_profile(mdd_engine* e, int enable);
/* fp32-storage engines (MDD_DTYPE_F32 / _BF16X2 / _F32_BF16OPS): operand arithmetic of the image encoder's
 * contractions per pass -- F (reference distill.py:524), B (:562-567), T-F and T-B (what :606 differentiates):
 * 0 = the engine's own mode, 1 = split-bf16 (hi + lo), 2 = one bf16 per operand, 3 = exact fp32 MFMA, 4 = one fp16 per
 * operand (experiment: what an fp16-storage engine's matrix cores would see).  Used for the
 * per-pass error attribution and for mixed parity-grade modes. */
int mdd_engine_set_pass_precision(mdd_engine* e, int fwd, int bwd, int tan_fwd, int tan_bwd);
int mdd_engine_profile_read(mdd_engine* e, int kind, double* out4);
/* one CSV row per contraction launch since enable (geometry, ms, TFLOP/s, GB/s) */
int mdd_engine_profile_dump(mdd_engine* e, const char* path);

/* ---- single-op entry points (parity tests; NHWC activations, dtype = MDD_DTYPE_*) */
int mdd_op_conv2d(int dtype, int transposed, int nimg, int hin, int win, int cin, int cout, int k,
                  int stride, int pad, int groups, const void* a_dev, const void* w_packed_dev,
                  const float* bias_dev, void* out_dev, void* stream);
int mdd_op_conv2d_wgrad(int dtype, int nimg, int hin, int win, int cin, int cout, int k, int stride,
                        int pad, int groups, const void* dy_dev, const void* x_dev,
                        float* dw_packed_dev, float* dbias_dev, void* stream);
/* the engine's form of the weight gradient: an optional second pair (tangent pass: dW_t = dy1^T x1 + dy2^T x2) and
 * a split-M workspace of ws_floats floats (partial tiles are summed by a second kernel into dw, which is then
 * OVERWRITTEN; without a workspace the partials are added into dw with fp32 atomics).  The bias gradient is the
 * column sum of dy1 (added into dbias). */
int mdd_op_conv2d_wgrad2(int dtype, int nimg, int hin, int win, int cin, int cout, int k, int stride,
                         int pad, int groups, const void* dy1_dev, const void* x1_dev, const void* dy2_dev,
                         const void* x2_dev, float* dw_packed_dev, float* dbias_dev, float* ws_dev,
                         long long ws_floats, void* stream);
/* MaxPool2d(3, stride 2, padding 1) on NHWC [n, h, w, c] (the NF-ResNet stem's pool); ho = (h - 1) / 2 + 1, the same
 * for w.  c must be a multiple of 4 (MDD_DTYPE_F32) or 8 (MDD_DTYPE_BF16).  idx: [n, ho, wo, c] bytes, ky*3 + kx of
 * the FIRST maximum of each window (PyTorch's rule: taps in row-major order, a tap wins when greater or NaN;
 * padding is -inf).
 *   mode 0  forward:  x [n, h, w, c] -> y [n, ho, wo, c], writes idx
 *   mode 1  tangent:  x = x_t [n, h, w, c] -> y = y_t [n, ho, wo, c], the element at idx
 *   mode 2  backward (and tangent backward, the index being fixed): x = dy [n, ho, wo, c] -> y = dx [n, h, w, c],
 *           each input element gathers the windows whose index points at it (no atomics) */
int mdd_op_maxpool2d_3s2(int dtype, int mode, int n, int h, int w, int c, const void* x_dev, void* y_dev,
                         void* idx_dev, void* stream);

/* Squeeze-excite in the MIDDLE of a block (NF-RegNet: on the mid channels between conv2 and conv3, followed by the
 * activation): a3 = silu(ga * gate * c2), c2 / a3 NHWC [n, hw, c] in the storage type, gate [n, c] fp32.  c must be a
 * multiple of 4 (MDD_DTYPE_F32) or 8 (MDD_DTYPE_BF16).  Tangent operands (`_t`) come all together or not at all; with
 * them ONLY the `_t` outputs are written (the primal ones are inputs then: they hold the primal call's results).
 *   mode 0  forward:  out = a3                                      (tangent: out_t)
 *   mode 1  backward: out = c2bar = ga*gate*dsilu(u)*a3bar, u = ga*gate*c2 (+ qbar / hw per (image, channel) when qbar
 *           [n, c] is given: the pooled path's share), zbar [n, c] = (ga * sum_hw c2*dsilu(u)*a3bar) * gate*(1-gate)
 *           (tangent: out_t, zbar_t; qbar_t in the place of qbar) */
int mdd_op_mid_se(int dtype, int mode, int n, int hw, int c, float ga, const void* c2, const void* c2_t, const float* gate,
                  const float* gate_t, const void* a3bar, const void* a3bar_t, const float* qbar, void* out, void* out_t,
                  float* zbar, float* zbar_t, void* stream);

/* The small-batch linear layers (csrc/linear.hip): squeeze-excite fc1 / fc2, the pooled-feature -> conv3 shortcut, the
 * text head.  n = batch, k = in features, j = out features; x [n, k], W [j, k], b [j], dy [n, j], all fp32 row-major
 * (form 3: W in wdtype).  A call is a TANGENT call when out_t is given (forms 0, 1, 3) or when dy_t or x_t is given
 * (forms 2, 4); it writes the tangent result only, and every tangent operand may be null on its own (= 0).
 *   form 0  forward:  out = y [n, j] = act(x W^T + b), act 0 none / 1 ReLU / 2 sigmoid, b may be null.
 *           tangent: out holds the stashed post-activation y (an input), out_t = act'(y) * (x_t W^T + x W_t^T + b_t)
 *   form 1  dgrad:    out = dx [n, k] = dy W, times [relu_of [n, k] > 0] when relu_of is given
 *           tangent: out_t = (dy_t W + dy W_t), masked the same way
 *   form 2  wgrad:    out = dW [j, k] = dy^T x, db [j] = column sums of dy (db may be null)
 *           tangent: out = dy_t^T x + dy^T x_t, db = column sums of dy_t
 *   form 3  typed-weight forward: out = alpha * (x W^T) + b with W (and W_t) in wdtype = MDD_DTYPE_F32 or _BF16
 *           tangent: out_t = alpha * (x_t W^T + x W_t^T) + b_t
 *   form 4  form 2, ADDED into out and db
 * route 0 = the engine's route (the one-workgroup-per-tile matrix-core kernel); route 1 = the route retrieval and the
 * caption decode take (no scratch: the LDS-tiled kernel, unsplit) -- form 0 only, primal, act 0, no bias.
 * wdtype is MDD_DTYPE_F32 except in form 3; alpha is read by form 3 only. */
int mdd_op_linear(int form, int route, int wdtype, int n, int k, int j, int act, float alpha, const float* x,
                  const float* x_t, const void* W, const void* W_t, const float* b, const float* b_t, const float* dy,
                  const float* dy_t, const float* relu_of, float* out, float* out_t, float* db, void* stream);

/* The pooled / squeeze-excite kernels of the NFNet image path (csrc/elementwise.hip).  Activations are NHWC
 * [n, h, w, c] in the storage type (dtype = MDD_DTYPE_F32 or _BF16; c a multiple of 4 or 8), hw = h * w; the per-(image,
 * channel) operand v and the pooled outputs are [n, c] fp32.  Tangent operands (`_t`) come all together or not at all;
 * with them ONLY the `_t` outputs are written.
 *   op 0  out [n, c] fp32 = mean_hw a                                            (linear: no tangent form)
 *   op 1  out [n, c] fp32 = mean_hw silu(a) ;  op 2  the same with relu          (tangent: out_t)
 *   op 3  out = v / hw * dsilu(a), v = the gradient of op 1's output ;  op 4  v / hw * [a > 0]      (tangent: out_t)
 *   op 5  a = c3, b = sc, v = gate: out = x' = c3 * gate * ga + sc, out2 = beta * silu(x') (out2 may be null)
 *         (tangent: out_t, out2_t)
 *   op 6  a = xbar, b = c3, v = gate: out [n, c] fp32 = zbar = (ga * sum_hw xbar * c3) * gate * (1 - gate),
 *         out2 = c3bar = xbar * gate * ga                                          (tangent: out_t, out2_t)
 *   op 7  AvgPool2d(2, 2, ceil_mode, count_include_pad = False): a [n, h, w, c] -> out [n, ceil(h/2), ceil(w/2), c]
 *   op 8  its backward: a = dout [n, ceil(h/2), ceil(w/2), c] -> out = din [n, h, w, c]          (7, 8: no tangent form) */
int mdd_op_pool_se(int dtype, int op, int n, int h, int w, int c, float ga, float beta, const void* a, const void* a_t,
                   const void* b, const void* b_t, const float* v, const float* v_t, void* out, void* out_t, void* out2,
                   void* out2_t, void* stream);

/* Weight standardisation of every convolution of a net in one launch (csrc/ws.hip), as the engine runs it: the descriptors
 * are built from `convs` (host memory) exactly as the engine builds them from its conv table, scale = gamma / sqrt(fan_in),
 * fan_in = cin / groups * k * k.  theta (fp32): per conv the weight OIHW [cout, cin / groups, k, k], then the gain [cout].
 * Packed buffers (dtype = MDD_DTYPE_F32 or _BF16 storage): conv i starts at the prefix sum of cout * k * k * cin_pad / groups
 * in both layouts, wf [cout][k * k][cin_pad / groups] and wt [groups][cin_pad / groups][k * k][cout / groups]; lanes of the
 * padded channels are never written.  cin_pad / groups and cout / groups must be whole 16-byte chunks of dtype.
 *   mode 0  forward: writes wf and wt.  Tangent call (theta_t given): writes wf_t and wt_t, and wf / wt again when that
 *           pair is given (both or neither)
 *   mode 1  backward: dwf (fp32, wf layout; padded lanes are not read) -> gtheta in theta's layout: the gradient of the
 *           weights and of the gains.  Tangent call (theta_t and dwf_t given): gtheta receives the tangent of that gradient
 * The call returns after the launch has completed (the descriptor array lives for the call only). */
typedef struct mdd_ws_conv {
  int32_t cout, cin, k, groups, cin_pad;
} mdd_ws_conv;
int mdd_op_weight_std(int dtype, int mode, int nconv, const mdd_ws_conv* convs_host, float gamma, float eps,
                      const float* theta, const float* theta_t, void* wf, void* wt, void* wf_t, void* wt_t,
                      const float* dwf, const float* dwf_t, float* gtheta, void* stream);

/* The pointwise, LayerNorm and row kernels of the text head (csrc/head.hip), fp32 [n, d] row-major.  A call is a TANGENT
 * call when out_t is given: the `_t` operands of a, b, c (and out2_t) are then required, gamma_t / beta_t may be null (= 0),
 * and ONLY the `_t` outputs are written (ops 0 - 2; op 3 see there).
 *   op 0  gelu:      a = p -> out = g = GELU(p) (erf)
 *   op 1  gelu_bwd:  a = p, b = rbar, c = gbar -> out = pbar = rbar + gbar * GELU'(p)
 *   op 2  ln_fwd:    a = f, b = p, mask [n, d] or null (= 1) -> out2 = r = f * mask + p, out = y = LN(r) * gamma + beta.
 *                    Tangent call: out2 holds the stashed r (read), out2_t = r_t, out_t = y_t
 *   op 3  ln_bwd:    a = ybar, b = r, mask or null, gamma -> out = rbar, out2 = fbar = rbar * mask, dgamma [d], dbeta [d];
 *                    stats: 4 n floats of scratch.  Tangent call: out_t = rbar_t, out2_t = fbar_t, and dgamma / dbeta
 *                    receive the TANGENTS of the parameter gradients (as the engine's gradient vector does)
 *   op 4  gather_rows:        out [n, d] = a[idx[r], :], idx int64 [n] or null (= the identity)
 *   op 5  scatter_rows_axpy:  out[idx[r], :] += coef[0] * mul * a[r, :], coef a device scalar or null (= 1); the rows of idx
 *                             are distinct
 * eps is read by ops 2 and 3, mul by op 5. */
int mdd_op_text_head(int op, int n, int d, float eps, float mul, const float* a, const float* a_t, const float* b,
                     const float* b_t, const float* c, const float* c_t, const float* mask, const float* gamma,
                     const float* gamma_t, const float* beta, const float* beta_t, const int64_t* idx, const float* coef,
                     float* out, float* out_t, float* out2, float* out2_t, float* dgamma, float* dbeta, float* stats,
                     void* stream);

/* The kernels at the two ends of every image pass: image_syn -> the first activation tensor, and the first layer's data
 * gradient -> grad_image_syn (csrc/elementwise.hip, csrc/vit.hip, csrc/nfres.hip).  image / dimage are fp32 NCHW
 * [nq, 3, h, w]; idx int64 [n] names the row of image / dimage that sample r reads / adds to, or is null (= the identity);
 * activations are in the storage type (dtype = MDD_DTYPE_F32 or _BF16).  The accumulating ops add
 * coef[0] * mul * (...) into dimage[idx[r]] (coef a device scalar or null = 1) WITHOUT atomics: the rows of idx must be
 * distinct, as the engine's are within a step; rows of dimage that idx does not name are not touched.  Operands an op
 * does not list must be null, parameters it does not list 0.
 *   op 0  gather:    image -> out NHWC [n, h, w, c]; c = cpad >= 3 (the engine passes 8), channels 3 .. c - 1 are written +0
 *   op 1  scatter:   a = x0bar [n, h, w, c] -> dimage[idx[r], ch, y, x] += coef * mul * x0bar[r, y, x, ch], ch < 3 (channels
 *                    3 .. c - 1 are not read)
 *   op 2  stem dgrad: the data gradient of Conv2d(3, cout, 3, stride 2, padding 1) straight into dimage: h = w = s,
 *                    c = cout, a = dy1 [n, s/2, s/2, cout], wt1 = the packed data-gradient weight [8][9][cout] in the storage
 *                    type (input channels 3 .. 7 are not read), optionally a2 = dy2, wt2 (the tangent pass: both or neither):
 *                    dimage[idx[r]] += coef * mul * (dgrad(dy1, wt1) + dgrad(dy2, wt2)).  "invalid argument" when the
 *                    kernel does not take the shape (s % 8 != 0, cout not 8 or 16: the engine then runs the implicit-GEMM data
 *                    gradient and op 1)
 *   op 3  patchify:  image -> out [n * (s/p)^2, 3 p p], h = w = s, c = 3, k = p, s % p == 0; row (r, py, px), column
 *                    ch * p * p + dy * p + dx = image[idx[r], ch, py * p + dy, px * p + dx]
 *   op 4  unpatchify_accum: a = colsbar in that layout -> dimage += coef * mul * (the same map backwards)
 *   op 5  im2col:    a = NHWC [n, h, w, c] (c = cpad, whole 16-byte chunks) -> out col [n * ho * wo, k * k * c], column
 *                    (ty * k + tx) * c + ch = a[r, oy * stride - pad + ty, ox * stride - pad + tx, ch], +0 outside the image;
 *                    ho = (h + 2 pad - k) / stride + 1, the same for wo.  No idx. */
int mdd_op_image_edge(int dtype, int op, int n, int h, int w, int c, int k, int stride, int pad, float mul,
                      const float* image, const int64_t* idx, const float* coef, const void* a, const void* wt1,
                      const void* a2, const void* wt2, void* out, float* dimage, void* stream);

/* The ViT's token glue (csrc/vit.hip).  Activations [n, tok, dim] in the storage type, cls [dim] / pos [tok, dim] and
 * dcls / dpos fp32.  A call is a TANGENT call when a_t is given (ops 0, 1, 4 only): every `_t` operand of the op is then
 * required and ONLY the `_t` outputs are written (op 1: see there).  Operands an op does not list must be null.
 *   op 0  embed:       a = pe [n, tok - 1, dim], cls, pos -> out = x0: x0[r, 0] = cls + pos[0], x0[r, 1 + p] = pe[r, p] + pos[1 + p]
 *                      (tangent: a_t, cls_t, pos_t -> out_t)
 *   op 1  embed_bwd:   a = xbar [n, tok, dim] -> out = pebar [n, tok - 1, dim] = xbar[:, 1:], dpos [tok, dim] = sum_r xbar[r],
 *                      dcls [dim] = sum_r xbar[r, 0].  dpos and dcls are OVERWRITTEN (they are slices of the flat gradient).
 *                      Tangent call (a_t -> out_t; out may be null): dpos / dcls receive the sums of xbar_t, the TANGENTS of
 *                      the parameter gradients
 *   op 2  cls_gather:  a = x [n, tok, dim] -> out [n, dim] = x[:, 0]
 *   op 3  cls_scatter: a = in [n, dim] -> out = xbar [n, tok, dim]: xbar[:, 0] = in, every other row written +0
 *   op 4  add2:        out = a + b over n * tok * dim elements, a multiple of the 16-byte chunk (tangent: a_t, b_t -> out_t)
 *   op 5  act_to_f32:  a (storage type) -> out fp32, n * tok * dim elements ;  op 6  f32_to_act: a fp32 -> out (storage type) */
int mdd_op_vit_glue(int dtype, int op, int n, int tok, int dim, const void* a, const void* a_t, const void* b, const void* b_t,
                    const float* cls, const float* cls_t, const float* pos, const float* pos_t, void* out, void* out_t,
                    float* dcls, float* dpos, void* stream);

/* The packed operands of every linear of a ViT in one launch (csrc/vit.hip k_lin_pack_all), as the engine runs it: the
 * descriptors are built from `shapes` (host memory: nlin pairs {out, in}) exactly as the engine builds them from its table
 * of linears.  theta (fp32): per linear the weight [out][in], then the bias [out], which is never read.  Packed buffers
 * (storage type): linear i starts at the prefix sum of out * in in both, wf = W as stored [out][in], wt = W^T [in][out];
 * every element of both is written.  Tangent call (theta_t given): wf_t and wt_t are required and receive the same packing
 * of theta_t, and wf / wt are WRITTEN AGAIN from theta (all four buffers are outputs).
 * The call returns after the launch has completed (the descriptor array lives for the call only). */
int mdd_op_lin_pack(int dtype, int nlin, const int32_t* shapes_host, const float* theta, const float* theta_t, void* wf,
                    void* wt, void* wf_t, void* wt_t, void* stream);

/* The residual sum of a block without squeeze-excite (csrc/nfres.hip, csrc/nfreg.hip) over `elems` elements of the storage
 * type, a multiple of the 16-byte chunk:  xo = x' = alpha * c3 + sc,  ao = beta * act(x') (ao may be null).
 *   op 0  act = ReLU (NF-ResNet) ;  op 1  act = SiLU (NF-RegNet)
 *         Tangent call (c3_t given: sc_t and xo_t required): ONLY xo_t and, when ao_t is given, ao_t are written (ao is then
 *         the stashed primal; ReLU's tangent is beta * [x' > 0] * x'_t with x' recomputed from c3 and sc)
 *   op 2  xo = alpha * c3 (no other operand) */
int mdd_op_resid(int dtype, int op, int64_t elems, float alpha, float beta, const void* c3, const void* c3_t, const void* sc,
                 const void* sc_t, void* xo, void* xo_t, void* ao, void* ao_t, void* stream);

/* ---- synthetic-set evaluation: retrieval ranks.
 * Replaces the per-row host loops of reference epoch.py:140-156 (image->text: argsort of one similarity
 * row, position of the best ground-truth caption), :163-192 (text->image) and itm_eval epoch.py:219-237.
 * img_feat [n_img, dim], txt_feat [n_txt, dim]: un-normalised fp32 embeddings (normalised here as
 * epoch.py:126/:148 do); scale = exp(log(1/0.07)) in the reference (epoch.py:106-107).
 * img2txt: CSR lists of ground-truth caption ids per image (dataset.img2txt); txt2img[n_txt].
 * scores_ws: n_img*n_txt floats, left holding the scaled similarity matrix; norm_ws: n_img+n_txt floats.
 * rank_*: 0-based ranks = number of strictly better-scoring candidates.  All pointers device memory. */
int mdd_retrieval_ranks(const float* img_feat, const float* txt_feat, const int* img2txt_off,
                        const int* img2txt_idx, const int* txt2img, int n_img, int n_txt, int dim,
                        float scale, float* scores_ws, float* norm_ws, int* rank_i2t, int* rank_t2i,
                        void* stream);

/* ---- caption decode of the synthetic text embeddings: for every query row the index
 * of the most cosine-similar bank row.  Replaces reference distill.py:89-95 (`nearest_neighbor`: one
 * sklearn cosine_similarity + np.argmax per query against all ~145k train caption embeddings), called at
 * distill.py:244 and :374.  Ties resolve to the lowest index (np.argmax).
 * query [n_query, dim], bank [n_bank, dim] fp32; scores_ws n_query*n_bank floats (left holding the cosine
 * matrix); norm_ws n_query+n_bank floats; idx_out [n_query].  All device memory. */
int mdd_nearest_neighbor(const float* query, const float* bank, int n_query, int n_bank, int dim,
                         float* scores_ws, float* norm_ws, int* idx_out, void* stream);

/* ---- RCCL all-reduce of the synthetic-set gradient (SURVEY 8b `allreduce_syn_grads`; mode A's one exchange
 * per outer iteration -- north_star: "RCCL all-reduce of the matching-loss gradient over xGMI").  The reference
 * has no counterpart (its only multi-GPU code is nn.DataParallel, distill.py:443-445).  RCCL is bound at run
 * time from the librccl.so.1 the process already holds (torch's), else /opt/rocm's; every entry fails with
 * "mdd: RCCL unavailable" when there is none.  One communicator per rank = per GPU:
 *   rank 0: mdd_comm_unique_id(id)  ->  the host moves the MDD_COMM_ID_BYTES to every rank (any channel)
 *   all   : mdd_comm_create(id, rank, world, device_id, &c)          (collective: returns when all joined)
 *   all   : mdd_allreduce_syn_grads(c, buf, n, average, stream)      (in place, fp32 sum; average != 0 then
 *           divides by world in the same stream order: bit-identical to all_reduce(SUM) + div_(world)) */
#define MDD_COMM_ID_BYTES 128
typedef struct mdd_comm mdd_comm;
int mdd_comm_unique_id(void* id_out);
int mdd_comm_create(const void* id, int rank, int world, int device_id, mdd_comm** out);
void mdd_comm_destroy(mdd_comm* c);
int mdd_comm_world(const mdd_comm* c);
int mdd_allreduce_syn_grads(mdd_comm* c, float* buf_dev, int64_t n, int average, void* stream);

/* ---- ViT building blocks (BASELINE configs[4]: ViT-B/16 image encoder; csrc/vit.hip).
 * The operators of timm 0.6.7's VisionTransformer block (what the reference reaches through timm / clip,
 * networks.py:661,668) that the NFNet path does not have, each as forward, backward and -- when the `*_t` tangent
 * pointers are non-NULL -- the tangent of either (the double backward of distill.py:606).  A tangent call reads the
 * primal operands and writes ONLY the `*_t` outputs.  dtype: MDD_DTYPE_F32 or MDD_DTYPE_BF16 = the storage type of
 * the activation tensors (`void*`); parameters, scores and probabilities are fp32.  Row-major, 16-byte aligned.
 *   layernorm      y = (x - mean) * rstd * gamma + beta over rows of `dim`            (eps 1e-6 in ViT)
 *   layernorm_bwd  dx (+ `res` when non-NULL: the gradient arriving over the residual connection), and dgamma / dbeta
 *                  ACCUMULATED (+=, fp32 atomics) into the caller's zeroed/partial sums
 *   gelu           a = GELU(c) (exact, erf);  gelu_bwd  cbar = abar * GELU'(c)
 *   quick_gelu     a = c * sigmoid(1.702 c) (CLIP's QuickGELU);  quick_gelu_bwd  cbar = abar * QuickGELU'(c)
 *   softmax        p = softmax(scale * s) over `cols` of each row (row stride ld); softmax_bwd  ds = scale*p*(dp - <p,dp>);
 *                  dtype = the storage type of the score tensors (the engine's bf16 mode keeps them in bf16: the matrix-core
 *                  contractions round them to bf16 anyway)
 *   bgemm          C[b] = alpha * A[b] B[b] for b = (o < outer, q < inner), every operand addressed by element strides
 *                  (transposes and the head slices of a fused qkv tensor need no copy).  bf16 dtype: a_is_f32 /
 *                  c_is_f32 say which of A, C are fp32 tensors (scores, probabilities); B is always activation-typed.
 *                  dtype MDD_DTYPE_BF16X2: fp32 tensors throughout, every product as hi*hi + hi*lo + lo*hi of split-bf16
 *                  operands on the matrix cores (the engine's bf16x2 mode); MDD_DTYPE_F32: exact fp32 FMA. */
typedef struct mdd_bgemm_desc {
  int32_t m, n, k, outer, inner;
  int64_t a_row, a_col, b_row, b_col, c_row, c_col;               /* A(i,kk) = A[i*a_row + kk*a_col], B(kk,j) = B[kk*b_row + j*b_col] */
  int64_t a_outer, a_inner, b_outer, b_inner, c_outer, c_inner;   /* batch strides in elements */
  float alpha;
} mdd_bgemm_desc;
/* Fused multi-head attention of the bf16 ViT path (csrc/attn.hip): head dimension 64, tokens <= 224; qkv is the fused
 * [n, tokens, 3, heads, 64] tensor, dout / out the [n, tokens, heads, 64] attention output (modes 0, 1) or, for the
 * gradient modes, out = d qkv in qkv's layout.  Nothing of size tokens x tokens leaves the CU: every mode recomputes
 * the score tiles it needs and exchanges per-row statistics [n, heads, tokens] (m, l: softmax max / sum, written by
 * mode 0; r = rowsum(P S_t), written by mode 1; D = rowsum(P dP) = rowsum(O dO), by mode 2 from o and dout; D_t, by
 * mode 3 from o, o_t, dout, dout_t).
 *   0  O = softmax(scale Q K^T) V          1  O_t (tangent along qkv_t)          2  dQ = dS K      (r_tan: dS K_t, accum)
 *   3  dQ_t part: dS_t K                   4  dV = P^T dO, dK = dS^T Q           (r_tan: dS^T Q_t; skip0: dK part only; accum)
 *   5  dV_t = P_t^T dO + P^T dO_t          6  dK_t part: dS_t^T Q
 * A full tangent of the backward is 3, 2(r_tan, accum), 5, 6, 4(r_tan, skip0, accum) on d qkv_t. */
int mdd_op_attention(int mode, int n, int tokens, int heads, float scale, const void* qkv, const void* qkv_t,
                     const void* dout, const void* dout_t, const void* o, const void* o_t, void* out, float* m, float* l,
                     float* r, float* D, float* D_t, int r_tan, int accum, int skip0, void* stream);
int mdd_op_layernorm(int dtype, int rows, int dim, float eps, const void* x, const void* x_t, const float* gamma,
                     const float* gamma_t, const float* beta, const float* beta_t, void* y, void* y_t, void* stream);
/* LayerNorm of a residual sum in one pass: s = a + b (stored in the storage type, normalised as stored), y = LN(s).
 * Tangent call (gamma_t given): s is the stashed primal sum (read), s_t = a_t + b_t (stored), y_t the tangent. */
int mdd_op_add_layernorm(int dtype, int rows, int dim, float eps, const void* a, const void* a_t, const void* b,
                         const void* b_t, void* s, void* s_t, const float* gamma, const float* gamma_t, const float* beta,
                         const float* beta_t, void* y, void* y_t, void* stream);
int mdd_op_layernorm_bwd(int dtype, int rows, int dim, float eps, const void* x, const void* x_t, const void* dy,
                         const void* dy_t, const float* gamma, const float* gamma_t, const void* res,
                         const void* res_t, void* dx, void* dx_t, float* dgamma, float* dgamma_t, float* dbeta,
                         float* dbeta_t, void* stream);
int mdd_op_gelu(int dtype, int64_t n, const void* c, const void* c_t, void* a, void* a_t, void* stream);
int mdd_op_gelu_bwd(int dtype, int64_t n, const void* c, const void* c_t, const void* abar, const void* abar_t,
                    void* cbar, void* cbar_t, void* stream);
int mdd_op_quick_gelu(int dtype, int64_t n, const void* c, const void* c_t, void* a, void* a_t, void* stream);
int mdd_op_quick_gelu_bwd(int dtype, int64_t n, const void* c, const void* c_t, const void* abar, const void* abar_t,
                          void* cbar, void* cbar_t, void* stream);
int mdd_op_softmax(int dtype, int64_t rows, int cols, int ld, float scale, const void* s, const void* s_t, void* p,
                   void* p_t, void* stream);
int mdd_op_softmax_bwd(int dtype, int64_t rows, int cols, int ld, float scale, const void* p, const void* p_t,
                       const void* dp, const void* dp_t, void* ds, void* ds_t, void* stream);
int mdd_op_bgemm(int dtype, int a_is_f32, int c_is_f32, const mdd_bgemm_desc* d, const void* A, const void* A_t,
                 const void* B, const void* B_t, void* C, void* C_t, void* stream);

/* ---- the frozen text towers that write the caption caches (csrc/text_tower.hip, csrc/attn_causal.hip,
 * csrc/attn_varlen.hip; DESIGN.md sections 13 and 14), which the reference reaches through textprocess /
 * textprocess_train (networks.py:700-735, distill.py:107-144): OpenAI CLIP's encode_text (clip/model.py) for
 * --text_encoder clip, and transformers' BertModel("bert-base-uncased") -> last_hidden_state[:, 0] for --text_encoder bert
 * (the default), computed over PACKED sequences: total = sum(len) token rows and cu_seqlens, no padding row.  Forward only.
 *
 * Causal multi-head attention, head dimension 64, 1 <= tokens <= 128: qkv is the fused [n, tokens, 3, heads, 64] tensor,
 * out [n, tokens, heads, 64], both in the storage type (dtype = MDD_DTYPE_F32: exact fp32 FMA; MDD_DTYPE_BF16: bf16 matrix
 * cores, maximum / denominator / accumulation in fp32).  out[i] = softmax(scale * q_i . K[0..i]) V[0..i]: keys after the
 * query are never part of the maximum, the denominator or the sum.  Nothing of size tokens x tokens leaves the CU. */
int mdd_op_attention_causal(int dtype, int n, int tokens, int heads, float scale, const void* qkv, void* out, void* stream);
/* out[r, t, :] = table[clamp(ids[r, t], 0, vocab - 1), :] + pos[t, :], summed in fp32 and stored in the storage type.
 * ids int32 [n, ctx] (device), table [vocab, width] and pos [ctx, width] fp32; width a multiple of the 16-byte chunk of
 * dtype.  The clamp keeps every read inside the table; refusing such ids is the caller's job. */
int mdd_op_token_embed(int dtype, int n, int ctx, int width, int vocab, const int32_t* ids, const float* table,
                       const float* pos, void* out, void* stream);
/* out [n, width] fp32 = x[r, e_r, :] (+ b[r, e_r, :] when b is given, added in fp32), e_r = the FIRST position of the
 * largest id of row r (torch.argmax; CLIP's end-of-text token has the largest id).  x, b [n, ctx, width] in the storage
 * type. */
int mdd_op_eot_gather(int dtype, int n, int ctx, int width, const int32_t* ids, const void* x, const void* b, float* out,
                      void* stream);

/* Bidirectional multi-head attention over packed sequences of different lengths (BERT's key-padding mask without the
 * padding), head dimension 64: qkv [total, 3, heads, 64], out [total, heads, 64] in the storage type; cu_seqlens int32
 * [n + 1] on the device, cu[0] = 0, cu[n] = total, 1 <= len_r = cu[r + 1] - cu[r] <= max_len <= 512.
 * out[cu[r] + i] = softmax(scale * q_i . K_r) V_r over the keys of sequence r only: the keys of other sequences are never
 * loaded, and the LDS rows beyond len_r take no part in the maximum or the denominator (their probabilities are exact
 * zeros).  K and V are streamed through LDS in stages of 128 keys: the LDS of a workgroup does not depend on max_len.
 * dtype as for mdd_op_attention_causal.  Whatever cu_seqlens holds, no row outside [0, total) is read or written (the
 * kernel clamps; a length above max_len is cut to max_len). */
int mdd_op_attention_varlen(int dtype, int n, int total, int heads, float scale, const void* qkv, const int32_t* cu_seqlens,
                            int max_len, void* out, void* stream);
/* BERT's embedding sum over packed rows, before its LayerNorm: out[row, :] = (word[id, :] + pos[t, :]) + type0[:] in fp32,
 * stored in the storage type (one rounding); id = clamp(ids[row], 0, vocab - 1), t = clamp(row - cu[r], 0, positions - 1)
 * for the sequence r that holds the row.  ids int32 [total], cu_seqlens int32 [n + 1] (device); word [vocab, width], pos
 * [positions, width], type0 [width] (row 0 of the token-type table) fp32; width a multiple of the 16-byte chunk. */
int mdd_op_bert_embed(int dtype, int n, int total, int width, int vocab, int positions, const int32_t* ids,
                      const int32_t* cu_seqlens, const float* word, const float* pos, const float* type0, void* out,
                      void* stream);

typedef struct mdd_text_tower mdd_text_tower;
typedef struct mdd_text_tower_config {
  const char* variant; /* "clip_text_b32" | "clip_text_micro" | "clip_text_nano" |
                          "bert_base_uncased" | "bert_micro" | "bert_nano" */
  int32_t max_batch;   /* sequences per mdd_text_tower_encode / _encode_varlen call                 */
  int32_t dtype;       /* MDD_DTYPE_F32 | MDD_DTYPE_BF16: storage and arithmetic of the blocks       */
  int32_t max_tokens;  /* BERT: packed token rows per call, which the workspace is planned from; 0 = max_batch *
                          context.  The CLIP variants compute whole contexts and ignore it.          */
} mdd_text_tower_config;
size_t mdd_sizeof_text_tower_config(void);   /* sizeof(mdd_text_tower_config) of the library */
/* create makes no GPU call: a tower that is only asked for its tables works without a GPU */
int mdd_text_tower_create(const mdd_text_tower_config* cfg, mdd_text_tower** out);
void mdd_text_tower_destroy(mdd_text_tower* t);
/* the tower's own flat fp32 parameter vector.  CLIP: names as the `clip` package registers them, under "model.".  BERT:
 * the `transformers` names of BertModel, bare ("embeddings.word_embeddings.weight", "encoder.layer.0.attention.self.
 * query.weight", ...), every parameter but pooler.* (bert_base_uncased: 108,891,648 elements); a layer's query, key and
 * value weights (and their biases) lie next to each other, which makes them one [3 D, D] linear.  Weights are matched BY
 * NAME (the flat order is this table's, not that of any whole-model parameter list) */
int64_t mdd_text_tower_param_numel(const mdd_text_tower* t);
int mdd_text_tower_param_count(const mdd_text_tower* t);
int mdd_text_tower_param_info(const mdd_text_tower* t, int index, char* name, int name_cap, int64_t* shape4, int* ndim,
                              int64_t* offset);
int mdd_text_tower_feature_dim(const mdd_text_tower* t);
/* CLIP: the context length every sequence has; BERT: the length of the position table (the longest sequence) */
int mdd_text_tower_context(const mdd_text_tower* t);
int mdd_text_tower_vocab(const mdd_text_tower* t);
int64_t mdd_text_tower_workspace_bytes(const mdd_text_tower* t);
int mdd_text_tower_bind_workspace(mdd_text_tower* t, void* ws_dev, int64_t bytes, void* stream);
/* theta_dev: the flat fp32 vector of the table above.  The linears are cast and packed and every other parameter is copied
 * into the workspace here, once: theta_dev is not read after the work enqueued by this call has run. */
int mdd_text_tower_load(mdd_text_tower* t, const float* theta_dev, void* stream);
/* ids_dev int32 [n, context], 1 <= n <= max_batch -> out_dev fp32 [n, feature_dim]; enqueues only (no host
 * synchronisation).  Ids outside [0, vocab) are clamped by the embedding kernel. */
int mdd_text_tower_encode(mdd_text_tower* t, const int32_t* ids_dev, int n, float* out_dev, void* stream);
/* BERT towers (a CLIP tower returns "invalid argument", as mdd_text_tower_encode does on a BERT tower): ids_packed_dev
 * int32 [total] -- the sequences one after another, each starting with its [CLS] token -- and cu_seqlens_dev int32 [n + 1]
 * as for mdd_op_attention_varlen; 1 <= n <= max_batch, n <= total <= max_tokens, max_len >= the longest sequence and <=
 * context -> out_dev fp32 [n, feature_dim], the last layer's [CLS] rows (last_hidden_state[:, 0]; the pooler is not part
 * of the tower).  Enqueues only. */
int mdd_text_tower_encode_varlen(mdd_text_tower* t, const int32_t* ids_packed_dev, const int32_t* cu_seqlens_dev, int n,
                                 int total, int max_len, float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDD_HIP_H */
