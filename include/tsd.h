/* tsd.h - C ABI of libtsd.so, the MI355X-native Tiny-Stable-Diffusion hot path.
 *
 * This header is the drop-in boundary: plain C scalars and pointers only,
 * no structs by value, no callbacks, so the reference's host language (Mojo, via
 * sys.ffi.DLHandle / external_call) or any other FFI can bind it.  The reference has no
 * FFI of its own; each entry point below replaces one Mojo struct's `forward()` and cites it
 * (paths relative to the reference repo lrmantovani10/Stable-Diffusion.mojo).
 *
 * Conventions
 *   - Host tensors are float32 in the reference's own layouts (`Matrix._data`,
 *     helpers/utils.mojo:805-811): images/activations CHW, token tensors (T, D), batched
 *     tensors contiguous [B][...] (`Matrix_Array`, helpers/utils.mojo:464-468).
 *   - The caller owns every input and output buffer; the library never keeps a caller pointer
 *     after return and never mutates an input (the reference's accidental aliasing,
 *     SURVEY.md App.A D14/D16, is not reproduced).
 *   - Arithmetic on the device is fp16 storage / fp32 accumulate (MFMA) - the "_f32" suffix
 *     names the boundary dtype, not the compute precision.
 *   - Every function returns 0 (TSD_OK) or a negative tsd_status; `tsd_last_error()` gives
 *     the thread-local message.  The reference prints and returns a null Matrix on shape
 *     errors (e.g. helpers/utils.mojo:1955-1957); a shim maps non-zero to that convention.
 *   - Calls on one context are serialised on that context's HIP stream; the host-pointer
 *     entry points are synchronous on return.  Distinct contexts may be used from distinct
 *     threads/processes (one per GPU).
 *   - There is NO CPU fallback: every compute entry point fails with TSD_E_HIP when no gfx950
 *     device is usable.
 */
#ifndef TSD_H
#define TSD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSD_VERSION 100 /* 0.1.0 */

typedef enum tsd_status {
  TSD_OK = 0,
  TSD_E_ARG = -1,   /* null pointer / bad enum / bad handle */
  TSD_E_SHAPE = -2, /* shape the path does not support (reference: "Returning null matrix") */
  TSD_E_ALLOC = -3,
  TSD_E_HIP = -4, /* HIP runtime error or no usable GPU */
  TSD_E_RCCL = -5,
  TSD_E_STATE = -6, /* call order violated (e.g. forward before weights set) */
  TSD_E_NONFINITE = -7 /* inf / NaN reached a tensor that leaves the device (fp16 activation overflow or non-finite input):
                        * reported by the next synchronisation point, see tsd_debug_nonfinite_count */
} tsd_status;

typedef struct tsd_ctx tsd_ctx;         /* one per GPU: device, stream, workspace arena */
typedef struct tsd_model tsd_model;     /* device-resident packed weights of one model */
typedef struct tsd_session tsd_session; /* device-resident denoise loop state (latents, context, schedule) */

/* ---- introspection ------------------------------------------------------------------- */
int tsd_version(void);
const char* tsd_last_error(void);
int tsd_device_count(void); /* number of visible HIP devices (0 if none / no driver) */

/* ---- context ------------------------------------------------------------------------- */
int tsd_ctx_create(int device, tsd_ctx** out);
int tsd_ctx_destroy(tsd_ctx* ctx);
int tsd_ctx_synchronize(tsd_ctx* ctx);
/* hipEvent timing on the context's own stream (bench.py: torch.cuda.Event would not see it). */
int tsd_ctx_timer_start(tsd_ctx* ctx);
int tsd_ctx_timer_stop(tsd_ctx* ctx, float* elapsed_ms);
/* Per-kernel-class timing with hipEvent pairs around every launch on the context stream (profiling pass
 * only - adds one event pair per launch).  Classes: 0 dense GEMM, 1 conv3x3 implicit GEMM, 2 flash attention,
 * 3 GroupNorm, 4 LayerNorm, 5 tiny-M linear, 6 elementwise/layout, 7 row softmax.  nclass <= 8. */
int tsd_ctx_profile_begin(tsd_ctx* ctx);
int tsd_ctx_profile_end(tsd_ctx* ctx, float* ms_per_class, int* launches_per_class, int nclass);
/* Per-launch records of the current profiling pass (call BEFORE profile_end, which resets):
 * rec[i] = {class, M, N, K, batch} (GEMM-class launches; Sq,Sk,d,B*H for attention), ms[i]; returns the count. */
int tsd_ctx_profile_records(tsd_ctx* ctx, int* rec, float* ms, int cap);

/* ---- op level: one export per reference op struct (host fp32 in/out) ------------------ */

/* `Conv2D.forward` helpers/utils.mojo:1738-1811.  x (C,H,W) [only the first `I` channels are
 * read, :1771], w (O,I,k,k) OIHW (:1718), bias (O) or NULL, symmetric zero padding
 * (pad_h,pad_w) (:1744-1747), stride (:1750-1758).  y (O,Ho,Wo), Ho=(H+2*pad_h-k)/stride_h+1.
 * k in {1,3}. */
int tsd_conv2d_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, const float* w, const float* bias, int I,
                   int O, int k, int pad_h, int pad_w, int stride_h, int stride_w, float* y);

/* `Matrix.pad` helpers/utils.mojo:1383-1413 (zero pad; the encoder's (0,1),(0,1), vae.mojo:115-116). */
int tsd_pad_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, int top, int bottom, int left, int right,
                float* y);

/* `GroupNorm.forward` helpers/utils.mojo:1845-1885: y=(x-mu)/(sigma+eps)*gamma over each of
 * `groups` groups of the first `num_channels` channels; population sigma; eps added to sigma
 * (:1871-1873).  y has `num_channels` channels. */
int tsd_groupnorm_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, int groups, int num_channels, float eps,
                      float gamma, float* y);

/* `LayerNorm.forward` helpers/utils.mojo:2052-2061, build semantics (SURVEY.md App.A D8):
 * per-row normalisation of x (M,C) with the GroupNorm formula, eps = 1e-5 in the reference. */
int tsd_layernorm_f32(tsd_ctx* ctx, const float* x, int M, int C, float eps, float* y);

/* EXTENSION (not reference behaviour): the norms real, PyTorch-trained checkpoints assume -
 * y = (x - mu) / sqrt(var + eps) * weight[c] + bias[c] (population variance, eps inside the root, per-channel affine;
 * weight / bias may be NULL = ones / zeros), i.e. torch.nn.GroupNorm / LayerNorm.  The reference's GroupNorm has a
 * scalar gamma, an unused beta and eps added to sigma (helpers/utils.mojo:1833-1834,1871-1873); its LayerNorm has no
 * parameters (:2052-2061).  `silu` != 0 fuses x*sigmoid(x) after the GroupNorm. */
int tsd_groupnorm_affine_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, int groups, float eps,
                             const float* weight, const float* bias, int silu, float* y);
int tsd_layernorm_affine_f32(tsd_ctx* ctx, const float* x, int M, int C, float eps, const float* weight,
                             const float* bias, float* y);

/* `SiLU.forward` helpers/utils.mojo:1892-1902 / `Gelu.forward` :1908-1919 (tanh approximation). */
int tsd_silu_f32(tsd_ctx* ctx, const float* x, int64_t n, float* y);
int tsd_gelu_tanh_f32(tsd_ctx* ctx, const float* x, int64_t n, float* y);

/* `Linear.forward` helpers/utils.mojo:1954-1976: y (M,N) = x (M,K) . w(N,K)^T + bias(N)|NULL. */
int tsd_linear_f32(tsd_ctx* ctx, const float* x, int M, int K, const float* w, const float* bias, int N, float* y);

/* `Matrix.matmul` helpers/utils.mojo:1549-1569: c[b] (M,N) = a[b] (M,K) . bmat[b or 0] (K,N),
 * `b_batch` is 1 (broadcast, :770-777) or `batch`. */
int tsd_matmul_f32(tsd_ctx* ctx, const float* a, const float* bmat, int batch, int b_batch, int M, int K, int N,
                   float* c);

/* `Upsample.forward` helpers/utils.mojo:1989-2010, build semantics (App.A D1): nearest x2. */
int tsd_upsample_nearest2x_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, float* y);

/* `Softmax(dim=2)` as used by attention (helpers/utils.mojo:411-448, helpers/attention.mojo:59),
 * build semantics (App.A D6): softmax over the last axis of x (rows, cols). */
int tsd_softmax_lastdim_f32(tsd_ctx* ctx, const float* x, int64_t rows, int cols, float* y);

/* `Self_Attention.forward` helpers/attention.mojo:26-65.  x (T,D); w_in (3D,D), b_in (3D)|NULL;
 * w_out (D,D), b_out (D)|NULL; heads; causal must be 0 on this path (CLIP only). */
int tsd_self_attention_f32(tsd_ctx* ctx, const float* x, int T, int D, int heads, const float* w_in,
                           const float* b_in, const float* w_out, const float* b_out, int causal, float* y);

/* `Cross_Attention.forward` helpers/attention.mojo:96-118.  x (Tq,D), context (Tk,Dc);
 * wq (D,D), wk/wv (D,Dc), wo (D,D); biases (D)|NULL. */
int tsd_cross_attention_f32(tsd_ctx* ctx, const float* x, int Tq, int D, const float* context, int Tk, int Dc,
                            int heads, const float* wq, const float* bq, const float* wk, const float* bk,
                            const float* wv, const float* bv, const float* wo, const float* bo, float* y);

/* `get_time_embedding` helpers/utils.mojo:353-370, build semantics (App.A D9): out[320] =
 * [cos(t f_i), sin(t f_i)], f_i = 10000^(-i/160).  Runs on the device like the rest of the path. */
int tsd_time_embedding_f32(tsd_ctx* ctx, float t, float* out320);

/* ---- block level (host fp32 in/out; weights passed per call, reference field order) ---- */

/* `Time_Embedding.forward` diffusion.mojo:17-21: (320) -> (1280). */
int tsd_time_embedding_mlp_f32(tsd_ctx* ctx, const float* t320, const float* w1, const float* b1,
                               const float* w2, const float* b2, float* out1280);

/* `Unet_Residual_Block.forward` diffusion.mojo:54-72.  x (Cx>=cin,H,W), time (1280).
 * conv1_w (cout,cin,3,3), lin_w (cout,1280), conv2_w (cout,cout,3,3), skip_w (cout,cin,1,1)
 * [used iff cin != cout; may be NULL otherwise].  y (cout,H,W). */
int tsd_unet_residual_block_f32(tsd_ctx* ctx, const float* x, int Cx, int H, int W, const float* time, int cin,
                                int cout, const float* conv1_w, const float* conv1_b, const float* lin_w,
                                const float* lin_b, const float* conv2_w, const float* conv2_b,
                                const float* skip_w, const float* skip_b, float* y);

/* `Unet_Attention_Block.forward` diffusion.mojo:112-147.  x (C,H,W) with C = n_head*n_embed,
 * context (Tk,Dc).  Weights in struct-field order (diffusion.mojo:87-98); `w` is an array of
 * 16 pointers (nw = 16): conv_in_w, conv_in_b, sa_in_w, sa_out_w, sa_out_b, ca_q_w, ca_k_w, ca_v_w,
 * ca_out_w, ca_out_b, geglu1_w, geglu1_b, geglu2_w, geglu2_b, conv_out_w, conv_out_b. */
int tsd_unet_attention_block_f32(tsd_ctx* ctx, const float* x, int n_head, int n_embed, int H, int W,
                                 const float* context, int Tk, int Dc, const float* const* w, int nw, float* y);

/* VAE `Res_Block.forward` vae.mojo:57-67 (GroupNorm 16 groups, no time input). */
int tsd_vae_res_block_f32(tsd_ctx* ctx, const float* x, int H, int W, int cin, int cout, const float* conv1_w,
                          const float* conv1_b, const float* conv2_w, const float* conv2_b, const float* skip_w,
                          const float* skip_b, float* y);

/* VAE `Attention_Block.forward` vae.mojo:17-27 (GroupNorm 32, one head, biases on). */
int tsd_vae_attention_block_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, const float* w_in,
                                const float* b_in, const float* w_out, const float* b_out, float* y);

/* ---- module level: device-resident weights (the measured path) ------------------------ */

/* TSD_MODEL_DIFFUSION_SD15: the full-size (860 M parameter) UNet of BASELINE.json configs[4] - the 12-encoder /
 * bottleneck / 12-decoder layout the reference's 23-layer graph (diffusion.mojo:177-201) was trimmed from, built from
 * the reference's own blocks (Unet_Residual_Block diffusion.mojo:34-72, Unet_Attention_Block :87-147, Upsample
 * :149-160 followed by a 3x3 conv).  It is not defined by the reference: throughput stress configuration only; every
 * entry point that takes a Diffusion accepts it.
 * TSD_MODEL_DIFFUSION_SD15_TORCH: the same graph with the norm semantics of PyTorch-trained SD-1.x checkpoints (extension,
 * see tsd_groupnorm_affine_f32): every GroupNorm / LayerNorm carries per-channel weight and bias parameters (appended
 * after the kind-5 parameter list as `<block>.layerN.weight` / `.bias`, N = the norm's field position in the reference
 * struct), eps sits inside the root, and the output layer's GroupNorm has 32 groups.
 * TSD_MODEL_CLIP_TORCH: the CLIP text encoder (clip.mojo:74-109) with torch LayerNorms - weight and bias of the two
 * LayerNorms of every layer (`playerN.layer1`, `playerN.layer3`) and of the final one (`layernorm`) appended to the
 * kind-4 parameter list; this is exactly Hugging Face's CLIPTextModel (the ViT-L/14 text tower SD-1.x conditions on).
 * TSD_MODEL_DECODER_TORCH / TSD_MODEL_ENCODER_TORCH: the VAE graphs (vae.mojo:94-112,194-219) with the trained VAE's
 * norms - 32 groups in the residual blocks (the reference declares 16, vae.mojo:42-43), per-channel weight / bias of
 * every GroupNorm appended to the kind-2 / kind-3 list (`lN.group_norm1`, `lN.group_norm2`, `lN.group_norm`, and
 * `lN` for the stand-alone norm), eps inside the root: the layout of diffusers' AutoencoderKL decoder / encoder. */
typedef enum tsd_model_kind { TSD_MODEL_DIFFUSION = 1, TSD_MODEL_DECODER = 2, TSD_MODEL_ENCODER = 3, TSD_MODEL_CLIP = 4, TSD_MODEL_DIFFUSION_SD15 = 5, TSD_MODEL_DIFFUSION_SD15_TORCH = 6, TSD_MODEL_CLIP_TORCH = 7, TSD_MODEL_DECODER_TORCH = 8, TSD_MODEL_ENCODER_TORCH = 9, TSD_MODEL_CONTROLNET_SD15 = 10, TSD_MODEL_CONTROLNET_SD15_TORCH = 11, TSD_MODEL_DIFFUSION_SD2 = 16, TSD_MODEL_CLIP_SD2 = 17, TSD_MODEL_IP_ADAPTER_SD15 = 20, TSD_MODEL_CLIP_VISION_H = 22, TSD_MODEL_IP_ADAPTER_PLUS_SD15 = 24 } tsd_model_kind;
/* TSD_MODEL_CONTROLNET_SD15 (EXTENSION: Zhang et al. 2023; the layout of diffusers' ControlNetModel): the control network of the full-size
 * UNet.  Parameters in this order: `time_embed.layer1/2`; the hint encoder `hint.conv1 .. hint.conv8` (3x3 convolutions 3->16, 16->16,
 * 16->32 stride 2, 32->32, 32->96 stride 2, 96->96, 96->256 stride 2, 256->320; SiLU after each but the last, the last initialised to
 * zero); `unet.layer1 .. unet.layer21`, the full-size UNet's 18 encoder and 3 bottleneck steps under the UNet's own names; the zero convolutions
 * `zero.skip1 .. zero.skip12` (1x1, one per skip the encoder pushes: 320 x4, 640 x3, 1280 x5 channels) and `zero.mid` (1x1, 1280), all
 * initialised to zero.  TSD_MODEL_CONTROLNET_SD15_TORCH: the same with the norm parameters of kind 6 appended last, so the shared
 * indices equal kind 10's.  tsd_flop_count returns -1 for both and tsd_model_lora_add refuses them (TSD_E_ARG). */

/* Parameter inventory in struct-field DFS order: `Diffusion`
 * diffusion.mojo:299-302, `Decoder` vae.mojo:194-219, `Encoder` vae.mojo:94-112.  No GPU needed. */
int tsd_model_param_count(int kind);
int tsd_model_param_info(int kind, int index, char* name, int name_cap, int64_t shape[4], int* ndim, int* used,
                         float* init_bound);

int tsd_model_create(tsd_ctx* ctx, int kind, tsd_model** out);
int tsd_model_destroy(tsd_model* m);
/* Upload one parameter (float32, reference layout: conv OIHW, linear (out,in), bias (out)). */
int tsd_model_set_param(tsd_model* m, int index, const float* data, int64_t numel);
/* Synthetic init on the device (the reference random-initialises in every __init__,
 * helpers/utils.mojo:1716-1727,1938-1945): U(+-init_bound) from the counter RNG
 * value = f(seed, kind*4096+index, element) - bit-identical to tsd/rng.py. */
int tsd_model_init_random(tsd_model* m, uint64_t seed);
/* The packed fp16/fp32 weight blob (one device allocation) - what multi-GPU broadcasts. */
int tsd_model_packed_blob(tsd_model* m, void** device_ptr, size_t* bytes);
int tsd_model_mark_loaded(tsd_model* m); /* after an external write (RCCL broadcast) into the blob */
/* Build the model's derived device buffers now (K-tile-major weight copies, the fused kernels' weight streams, im2col input
 * weights - rebuilt per rank, never broadcast) and wait for them; otherwise the first forward builds them.  Lets a multi-GPU host
 * time that step next to the broadcast (bench.py `derived_buffers_s`).  TSD_E_STATE if a used parameter was never set. */
int tsd_model_prepare(tsd_model* m);

/* ---- LoRA adapters (EXTENSION: the reference can only random-initialise) ----------------------------------------------------------
 * A model keeps the packed fp16 weights only, so a low-rank adapter is MERGED on the device, in the weights' own layout:
 *     W'[o][c] = rn16( W[o][c] + scale * sum_j up[o - row0][j] * down[j][c] )     row0 <= o < row0 + rows
 * fp32 operands and accumulation on the exact-fp32 matrix instruction, ONE rounding to fp16 (nearest-even).  `index` names a weight
 * matrix (conv kernel or linear weight); up [rows][rank] and down [rank][cols] are host fp32 in reference coordinates: cols = I for a
 * linear layer, I * k * k (i * k * k + tap, the flattened [I][k][k]) for a convolution.  Synchronous.
 * The first add on a parameter snapshots its packed bytes (the base); repeated adds on one parameter stack, each costing one rounding -
 * two stacked adapters are not bit-equal to one merge of their sum.  tsd_model_lora_clear restores every touched parameter bit for
 * bit and frees the snapshots; tsd_model_lora_count is the number of parameters that currently differ from their base.
 * Both move the parameter generation like tsd_model_set_param, so an open session rebuilds its hoisted buffers on its next step.
 * tsd_model_set_param(index) makes the new value the base of that parameter (its snapshot is dropped); tsd_model_init_random and
 * tsd_model_mark_loaded drop every snapshot.
 * Errors leave the weights, the snapshots and the count exactly as they were: TSD_E_ARG (NULL pointer, a bias / norm parameter, a
 * parameter the forward never reads, rank outside 1..1024, a non-finite scale), TSD_E_SHAPE (row range outside the parameter),
 * TSD_E_STATE (the parameter was never set), TSD_E_NONFINITE (a merged weight leaves fp16, or up / down hold inf / NaN). */
int tsd_model_lora_add(tsd_model* m, int index, int row0, int rows, const float* up, const float* down, int rank, float scale);
int tsd_model_lora_clear(tsd_model* m);
int tsd_model_lora_count(tsd_model* m);
/* Parameter `index` as the forward reads it, unpacked to the reference layout in fp32 (numel must match): every weight is exactly an
 * fp16 value - there are no fp32 masters -, biases and norm parameters are the fp32 that was set; a parameter the forward never
 * reads comes back as zeros.  TSD_E_STATE if it was never set. */
int tsd_model_get_param(tsd_model* m, int index, float* out, int64_t numel);
/* Op level, host fp32 in/out, synchronous: the merge above on w [O][I] (k = 0; interleave != 0: packed with the GEGLU row interleave)
 * or [O][I][k][k] (k = 1, 3), packed as a model packs it, merged by the same kernel and returned unpacked - every value of out is
 * exactly an fp16.  TSD_E_NONFINITE when a merged value is not finite. */
int tsd_lora_merge_f32(tsd_ctx* ctx, const float* w, int O, int I, int k, int interleave, int row0, int rows, const float* up,
                       const float* down, int rank, float scale, float* out);

/* `Diffusion.forward` diffusion.mojo:309-318, batched.  latents [B,4,L,L], context [B,T,768],
 * time_emb [B,320] (= get_time_embedding(t) per sample) -> out [B,4,L,L]. */
int tsd_diffusion_forward(tsd_model* m, const float* latents, const float* context, const float* time_emb, int B,
                          int L, int T, float* out);
/* `Decoder.forward` vae.mojo:221-250, batched.  latents [B,4,L,L] -> images [B,3,8L,8L] (raw decoder
 * output; pipeline.mojo:127's rescale is tsd_rescale_images_f32). */
int tsd_decoder_forward(tsd_model* m, const float* latents, int B, int L, float* images);
/* `Encoder.forward` vae.mojo:131-159 (+ metrics_evals :118-129), batched.  images [B,3,S,S] in
 * [-1,1], noise [B,4,S/8,S/8] -> latents [B,4,S/8,S/8]. */
int tsd_encoder_forward(tsd_model* m, const float* images, const float* noise, int B, int S, float* latents);
/* Rectangular forms of the three forwards; the square entries above are their LH == LW == L (SH == SW == S) case, the same launches
 * and the same bits.  latents / out [B,4,LH,LW], images [B,3,8LH,8LW] (encoder: images [B,3,SH,SW], noise and latents
 * [B,4,SH/8,SW/8]).  Per side the square rules: LH and LW multiples of 8 (16 for the full-size UNet kinds), SH and SW multiples of 64;
 * TSD_E_SHAPE otherwise, before any launch or copy. */
int tsd_diffusion_forward_hw(tsd_model* m, const float* latents, const float* context, const float* time_emb, int B,
                             int LH, int LW, int T, float* out);
int tsd_decoder_forward_hw(tsd_model* m, const float* latents, int B, int LH, int LW, float* images);
/* ---- ControlNet (EXTENSION): spatial conditioning of the full-size UNet ------------------------------------------------------------
 * The control network `cn` (kinds 10 / 11) sees the UNet's inputs and a hint image, hint [B,3,8LH,8LW] fp32 with the values as given:
 *     h = conv_in(latents) + hint_encoder(hint), then the UNet's encoder and bottleneck on the ControlNet's own weights;
 *     r_i = zero_i(h_i) for the 12 tensors the encoder pushes as skips (i = 0..11, in push order) and the bottleneck output (i = 12).
 * tsd_controlnet_forward_hw returns the 13 residuals as fp32 CHW, residuals_out[i] = [B,C_i,H_i,W_i] with (C_i, side) = (320, L) x3,
 * (320, L/2), (640, L/2) x2, (640, L/4), (1280, L/4) x2, (1280, L/8) x4.
 * tsd_diffusion_forward_control_hw is tsd_diffusion_forward_hw of `unet` (kinds 5 / 6) with skip_i + scale[b] * r_i in place of every
 * skip and of the bottleneck output.  Both forwards run inside one plan of one context: the two models must belong to the same tsd_ctx
 * (TSD_E_ARG otherwise, as for a `unet` that is not full-size or a `cn` that is no ControlNet).  On the device the residuals are fp16
 * NHWC and the injection is ONE launch between the bottleneck and the first decoder block,
 *     x = rn16(fmaf(scale[b], (float)r, (float)x))            fp32, one rounding to fp16, in place
 * which also re-emits the GroupNorm statistics the producers of those tensors emitted, so no decoder block gains a statistics pass.  A
 * sample whose scale is exactly 0 is neither read nor written by it: its output is the uncontrolled forward's.  Shapes as for
 * tsd_diffusion_forward_hw (LH, LW multiples of 16), TSD_E_SHAPE otherwise. */
int tsd_controlnet_forward_hw(tsd_model* cn, const float* latents, const float* context, const float* time_emb, const float* hint, int B,
                              int LH, int LW, int T, float* const* residuals_out);
int tsd_diffusion_forward_control_hw(tsd_model* unet, tsd_model* cn, const float* latents, const float* context, const float* time_emb,
                                     const float* hint, const float* scale, int B, int LH, int LW, int T, float* eps_out);
/* The hint encoder alone: hint [B,3,8LH,8LW] -> features_out fp32 [B,320,LH,LW].  It depends on the hint only. */
int tsd_controlnet_hint_hw(tsd_model* cn, const float* hint, int B, int LH, int LW, float* features_out);
/* ControlNet in a lockstep denoise session on a full-size UNet.  hint: host fp32 [B,3,8LH,8LW] (the session's B and sides; the entry
 * takes no shape, so the caller owns it - the Python wrapper checks it); scale: one fp32 for every sample; cond_only != 0: under CFG the
 * uncond half gets scale 0; control is applied on steps first_step <= i <= last_step (last_step < 0: to the end of the list).  cn == NULL
 * turns control off.  Call after upload().  The hint encoder runs here, once, and its features stay on the device; the per-sample scale
 * vector is built and uploaded here; the ControlNet's time projections and context K / V^T follow the session's hoist exactly as the
 * UNet's do (built here and at every later upload() when it is on, per step when off).  A step inside the window runs the ControlNet
 * forward at the UNet's batch (2B under CFG) on the step's latents, timestep and contexts and then the controlled UNet forward, with no
 * copy from the host and no allocation; a step outside it, and every step after set_control(NULL), enqueues the launches and gives the
 * bits of a session without control.  The control stays across upload()s until it is turned off.  Samplers, prediction types, seeds,
 * inpainting and guidance rescale compose unchanged: only the forward differs.
 * TSD_E_ARG: the session's UNet is not full-size, cn is no ControlNet or lives on another context, a scale that is not finite, a bad
 * window.  TSD_E_STATE: before upload(); on a slot session; and tsd_session_slots_open on a session with control (per-slot control is
 * not supported).  tsd_session_control_active: 1 while a ControlNet is set. */
int tsd_session_set_control(tsd_session* s, tsd_model* cn, const float* hint, float scale, int cond_only, int first_step, int last_step);
int tsd_session_control_active(tsd_session* s);
/* Op level, host fp16 in/out, synchronous: the injection launch alone over a table of n <= 16 tensors.  x[i] / r[i] / y_out[i]: fp16 bits
 * [B][HW[i]][C[i]] (C a multiple of 8, at most 2048); scale [B]; partial_out[i]: fp32 [B][nslab[i]][groups[i]][2], the (sum, sum of
 * squares) of the rounded y over slab s = rows [s * ceil(HW / nslab), ...) and group g, summed in fp32 in a fixed order.  groups[i] == 0:
 * no statistics for that entry (partial_out[i] is ignored; nslab[i] only cuts the work).  Here every sample is computed, a scale of 0
 * included (y == x).  A sample's y and partials are the same bits run to run and in every batch position. */
int tsd_control_inject_f16(tsd_ctx* ctx, int n, const void* const* x, const void* const* r, int B, const int* HW, const int* C,
                           const int* groups, const int* nslab, const float* scale, void* const* y_out, float* const* partial_out);
/* ---- IP-Adapter (EXTENSION: Ye et al. 2023; the layout of the published ip-adapter_sd15 files): image-prompt tokens through decoupled
 * cross attention.  In every cross-attention block of the full-size SD-1.x UNet a second key / value pair reads N image tokens and its
 * attention result joins the text result before the shared output projection:
 *     ao = Attn(q, K_text, V_text) + s_b * Attn(q, K_ip, V_ip)        K_ip = tok . Wk_ip^T,  V_ip = tok . Wv_ip^T,  tok [N][768]
 * TSD_MODEL_IP_ADAPTER_SD15 (20; the numbers 12 - 15, 18 and 19 stay reserved and refused) holds, under the published names: `image_proj.proj.weight` [N*768][1024] and `.bias`,
 * `image_proj.norm.weight` / `.bias` [768], and for each of the 16 cross-attention blocks of the full-size step table, in the table's
 * order (6 encoder, 1 bottleneck, 9 decoder blocks), `ip_adapter.<i>.to_k_ip.weight` and `ip_adapter.<i>.to_v_ip.weight` [C][768] with no
 * bias, <i> the odd number the published files give the block (1 .. 11 the encoder, 31 the bottleneck, 13 .. 29 the decoder).  N = 4.
 * The 16 to_k_ip matrices are contiguous in the packed blob and the 16 to_v_ip matrices follow them, so K_ip and V_ip^T of all blocks are
 * one GEMM (two where the fused form does not apply) over the tokens staged as 16 fp16 rows per sample, rows N .. 15 zero.
 * tsd_flop_count returns -1 and tsd_model_lora_add refuses the kind.  Callers bring the 1024-wide image embedding -
 * tsd_clip_vision_forward below computes it from pixels - or the tokens themselves.  The "plus" files are a kind of their own, with
 * their resampler: TSD_MODEL_IP_ADAPTER_PLUS_SD15, "IP-Adapter Plus" below.
 * tsd_ip_adapter_project: embeds [B][1024] -> tokens_out [B][N][768] = LayerNorm(Linear(embeds)) per token (eps 1e-5); every value is
 * exactly an fp16.
 * tsd_diffusion_forward_ip_hw: tsd_diffusion_forward_hw of `unet` (kinds 5 / 6; TSD_E_ARG for the Tiny-SD graph, the SD-2.x kind and a
 * ControlNet in that place) with the adapter `ip` on tokens [B][N][768], 1 <= N <= 16, scaled per sample by ip_scale [B]; and, when
 * cn != NULL, with the ControlNet `cn` on hint / control_scale as in tsd_diffusion_forward_control_hw - both in one plan (the adapter does
 * not apply to the ControlNet's own blocks).  ip == NULL: no adapter (tokens, N, ip_scale are ignored), the launches of the plain or the
 * controlled entry.  With an adapter every attention block runs op by op and gains ONE launch between its cross-attention core and
 * out_proj (k_ip_attn_add, csrc/kernels_ipattn.hip):
 *     O <- rn16( f32(O) + s_b * (sum_j p_j V_ip[j]) / sum_j p_j ),   p_j = rn16( exp(scale (q . K_ip[j]) - max_j) ),  j < N
 * A sample whose scale is exactly 0 is neither read nor written by it.  All models on one tsd_ctx. */
int tsd_ip_adapter_project(tsd_model* ip, const float* embeds, int B, float* tokens_out);
/* ---- IP-Adapter Plus (EXTENSION: the layout of the published ip-adapter-plus_sd15 / ip-adapter-plus-face_sd15 files): the same adapter
 * behind a Perceiver resampler.  TSD_MODEL_IP_ADAPTER_PLUS_SD15 (24; 12 - 15, 18, 19, 21 and 23 stay reserved and refused) holds, under the
 * published names and in the module's state-dict order: `image_proj.latents` [1][16][768] (kept as fp16), `image_proj.proj_in.weight`
 * [768][1280] and `.bias`, `image_proj.proj_out.weight` [768][768] and `.bias`, `image_proj.norm_out.weight` / `.bias`; per layer L = 0 .. 3
 * `image_proj.layers.L.0.norm1` and `.0.norm2` (weight / bias), `.0.to_q.weight` [768][768], `.0.to_kv.weight` [1536][768] (K rows first),
 * `.0.to_out.weight` [768][768], `.1.0.weight` / `.bias` (the feed-forward LayerNorm), `.1.1.weight` [3072][768], `.1.3.weight` [768][3072],
 * none of these linears with a bias; then the 32 `ip_adapter.<i>.to_k_ip.weight` / `.to_v_ip.weight` entries exactly as kind 20 lists and
 * packs them: 83 parameters, 49 087 488 elements.  The layout is written from memory of the published module, not checked against a
 * real file.  tsd_flop_count, tsd_model_lora_add and tsd_model_context_width answer as for kind 20.
 * tsd_ip_adapter_resample: hidden fp32 [B][S][1280] (tsd_clip_vision_forward's hidden_out at S = 257) -> tokens_out fp32 [B][16][768],
 * every value exactly an fp16.  For one sample, LayerNorms torch's with eps 1e-5:
 *     x = hidden . proj_in^T + b_in;  lat = latents;  four times:  xn = LN(x; norm1), ln = LN(lat; norm2), q = ln . Wq^T,
 *     k | v = concat(ln, xn) . Wkv^T, per head of 64 columns (12 heads) a = softmax(q k^T / 8) v over all S + 16 keys (no mask),
 *     lat = a . Wo^T + lat,  lat = gelu_erf(LN(lat; ff_norm) . W1^T) . W2^T + lat;   tokens = LN(lat . proj_out^T + b_out; norm_out)
 * (the 16 latent keys stand in front of the S image keys: softmax does not depend on the order, and the pad behind a sample's keys stays
 * at one end).  Existing kernels only, about 2 B + 8 launches a layer; activations are fp16, sums fp32; a sample's bits do not depend on B
 * or on its batch position.  1 <= B <= 16 and 1 <= S <= 1024, TSD_E_SHAPE otherwise; TSD_E_ARG for a kind-20 model, and
 * tsd_ip_adapter_project on a kind-24 model is TSD_E_ARG with a message that names this entry; a refusal leaves tokens_out untouched.
 * Host in, host out, synchronous.  A non-finite value in `hidden` (or an fp16 overflow on the way) is not looked for at the entry: it
 * spreads through the norms and GEMMs, tokens_out is written with the resulting inf / NaN, the launch that writes it counts them and the
 * call returns TSD_E_NONFINITE - the convention of every entry whose output leaves the device (tsd_debug_nonfinite_count).
 * The tokens go where kind 20's go: tsd_diffusion_forward_ip_hw and tsd_session_set_ip_adapter take a kind-24 model wherever they take
 * kind 20, with N the caller's (16 in use); tsd_clip_vision_forward below gives `hidden`. */
int tsd_ip_adapter_resample(tsd_model* ip, const float* hidden, int B, int S, float* tokens_out);
int tsd_diffusion_forward_ip_hw(tsd_model* unet, tsd_model* ip, const float* tokens, int N, const float* ip_scale, tsd_model* cn,
                                const float* hint, const float* control_scale, const float* latents, const float* context,
                                const float* time_emb, int B, int LH, int LW, int T, float* eps_out);
/* Op level, host fp16 in/out, synchronous: the launch alone.  q / o [B][S][H*d], k_ip [B][16][H*d] (rows >= N are not read),
 * vt_ip [B][H*d][16] (columns >= N do not reach the result), scale [B]; d in {40, 80, 160}, 1 <= N <= 16, S a multiple of 4;
 * softmax_scale multiplies the scores (1 / sqrt(d) in the graph).  o_out receives o updated; a sample with scale 0 comes back as it went. */
int tsd_ip_attn_add_f16(tsd_ctx* ctx, const void* q, const void* k_ip, const void* vt_ip, const void* o, const float* scale, int B, int H,
                        int d, int S, int N, float softmax_scale, void* o_out);
/* IP-Adapter in a lockstep denoise session on a full-size SD-1.x UNet.  tokens: host fp32 [B][N][768] for the conditional half;
 * uncond_tokens: the same shape for the unconditional half - required when the session runs CFG (callers pass the projection of a zero
 * embedding, which is NOT zero tokens), ignored otherwise; scale: one fp32 for every sample of both halves; the adapter applies on steps
 * first_step <= i <= last_step (last_step < 0: to the end).  ip == NULL turns it off.  Call after upload().  The tokens are staged and
 * K_ip / V_ip^T of all 16 blocks are projected here, ONCE (they do not depend on the step), and the per-sample scale vector is built and
 * uploaded here; every step() inside the window runs the adapted forward with no host copy and no allocation; upload() rebuilds nothing
 * of it; a step outside the window and every step after set_ip_adapter(NULL) enqueues the launches and gives the bits of a session
 * without an adapter.  It composes with tsd_session_set_control, seeds, inpainting, guidance rescale, every sampler and prediction type
 * and the hoist.  New parameters of `ip` (tsd_model_set_param) take effect at the next set_ip_adapter.
 * TSD_E_ARG: the session's UNet is not kind 5 / 6, ip is no IP-Adapter or lives on another context, N outside 1 .. 16, a scale that is not
 * finite, a bad window, no uncond_tokens under CFG.  TSD_E_STATE: before upload(); on a slot session; and tsd_session_slots_open on a
 * session with an adapter (per-slot adapters are not supported).  tsd_session_ip_adapter_active: 1 while an adapter is set. */
int tsd_session_set_ip_adapter(tsd_session* s, tsd_model* ip, const float* tokens, const float* uncond_tokens, int N, float scale,
                               int first_step, int last_step);
int tsd_session_ip_adapter_active(tsd_session* s);
/* Replay entry of launch_ip_attn_add with the conventions of tsd_debug_attn_run (test infrastructure: tests/ipadapter_ref.py holds the
 * kernel to an fp64 reference, element-wise).  One int64 per argument: pitches and per-sample strides in elements, SCALE the bits of a
 * float.  Operand slots: inputs Q [B][S][ldq], K [B][16][ldk], V^T [B][H*d][ldvt], S (fp32 [B]) and OIN, the payload O starts from (not
 * a device operand of its own); output O [B][S][ldo], updated in place.  host_in == NULL only sizes.  info[TSD_PI_CHANGED]: guard and
 * pitch-gap elements the launch changed.  The shapes the launcher refuses (d, N, S % 4, misaligned pitches) are sized and left to it. */
enum tsd_ipattn_desc_field {
  TSD_PD_VERSION = 0, TSD_PD_B, TSD_PD_H, TSD_PD_D, TSD_PD_S, TSD_PD_N, TSD_PD_LDQ, TSD_PD_LDK, TSD_PD_LDVT, TSD_PD_LDO,
  TSD_PD_SQB, TSD_PD_SKB, TSD_PD_SVTB, TSD_PD_SOB, TSD_PD_SCALE,
  TSD_PD_COUNT
};
#define TSD_PD_VERSION_1 1
enum tsd_ipattn_operand { TSD_PO_Q = 0, TSD_PO_K, TSD_PO_VT, TSD_PO_S, TSD_PO_OIN, TSD_PO_O, TSD_PO_COUNT };
enum tsd_ipattn_info { TSD_PI_CHANGED = 0, TSD_PI_COUNT };
int tsd_debug_ip_attn_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out, int64_t* ext,
                          int64_t* info);
/* Time `iters` launches of k_ip_attn_add on synthetic device data: B samples (<= 16, all at scale 1), S queries, N image tokens. */
int tsd_debug_ip_attn_bench(tsd_ctx* ctx, int B, int H, int d, int S, int N, int iters, float* ms);
int tsd_encoder_forward_hw(tsd_model* m, const float* images, const float* noise, int B, int SH, int SW, float* latents);
/* ---- CLIP vision encoder (EXTENSION: OpenCLIP ViT-H/14 as Hugging Face ships it in the `image_encoder/` folder of h94/IP-Adapter, a
 * CLIPVisionModelWithProjection): the 1024-wide image embedding the ip-adapter_sd15 files were trained against, from pixels.
 * TSD_MODEL_CLIP_VISION_H (22; the numbers 12 - 15, 18, 19, 21 and 23 stay reserved and refused): width 1280, 16 heads of 80, 32 pre-LN
 * layers, erf-GELU MLP of 5120, 14x14 patches of a 224x224 crop (256 patches + 1 class token = 257 tokens), `post_layernorm` on the class
 * row, a bias-free 1280 -> 1024 projection.  Parameters, in this order: `embeddings.class_embedding` [1280],
 * `embeddings.patch_embedding.weight` [1280][588] (the flattened HF conv weight [1280][3][14][14]; no bias; K zero-padded to 640 in the
 * packed blob: the GEMM wants whole 64-deep K tiles), `embeddings.position_embedding.weight` [257][1280] (kept as fp16),
 * `pre_layrnorm.weight` / `.bias` (HF's spelling), per layer N = 0 .. 31 `layers.N.ln1`, `layers.N.in_proj` ([3840][1280] with bias, q | k | v
 * stacked), `layers.N.out_proj`, `layers.N.ln2`, `layers.N.fc1` (1280 -> 5120), `layers.N.fc2` (5120 -> 1280), then `post_layernorm` and
 * `visual_projection.weight` [1024][1280] (no bias).  LayerNorms are torch's (eps 1e-5).  tsd_model_lora_add refuses the kind,
 * tsd_model_context_width returns TSD_E_ARG for it, tsd_flop_count(kind, 0, 0) returns the GFLOP of ONE image: 32 x (four linears on 257
 * rows + 4 * 257^2 * 1280 for the attention core) + the patch GEMM + the projection.
 *
 * The image front end (k_clip_image_patches, csrc/kernels_vision.hip) is the float-valued form of HF's CLIPImageProcessor: images fp32
 * [B][3][H][W] on the 0 .. 255 scale (the scale of the VAE encoder's input), 8 <= H, W <= 2048 (TSD_E_SHAPE otherwise) ->
 *   resize: shortest edge to 224, the other edge to int(224 * long / short); PIL's separable antialiased bicubic (Keys, a = -0.5),
 *           horizontal pass first.  Per axis scale = n_in / n_out, fs = max(scale, 1), support = 2 fs; output xx has
 *           center = (xx + 0.5) scale, lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), n_in) and the
 *           weights w((x - center + 0.5) / fs), x in [lo, hi), divided by their sum.  The host builds the two tables in double, rounds
 *           every weight to fp32 once and keeps them on the context per (H, W);
 *   centre crop to 224 x 224: top = (RH - 224) / 2, left = (RW - 224) / 2 (integer division);
 *   normalise: (v / 255 - mean_c) / std_c, mean (0.48145466, 0.4578275, 0.40821073), std (0.26862954, 0.26130258, 0.27577711),
 *           evaluated as one fma with 1 / (255 std_c) and -mean_c / std_c, rounded ONCE to fp16;
 * -> patch rows fp16 [B * 256][592]: row b * 256 + py * 16 + px, column c * 196 + kh * 14 + kw (the flattening of the HF conv weight),
 * columns 588 .. 591 zero.  fp32 sums in tap order; no atomics; a sample's bits do not depend on B or on its batch position.
 * NOT reproduced: the rounding to uint8 that PIL applies after resizing an 8-bit image (CLIPImageProcessor on a uint8 input) - after the
 * normalisation at most 0.5 / 255 / std = 7.5e-3 per element.  A 224 x 224 input is resized by the identity (every coefficient row is
 * 0, 1, 0, 0), so a caller who resizes to 224 x 224 themselves gets HF's numbers.
 * tsd_clip_image_patches_f16: host in, host out (fp16 bits [B * 256][592]), synchronous; 1 <= B <= 64.
 * tsd_clip_vision_forward: images as above, 1 <= B <= 16 -> image_embeds fp32 [B][1024] (HF's `image_embeds`) and, when hidden_out is
 * not NULL, the input of the last layer fp32 [B][257][1280] (HF's `hidden_states[-2]`, no post-LayerNorm: what the "plus" adapters read).
 * hidden_out costs one conversion launch and a copy, nothing when NULL; image_embeds are the same bits either way. */
int tsd_clip_image_patches_f16(tsd_ctx* ctx, const float* images, int B, int H, int W, void* patches_out);
int tsd_clip_vision_forward(tsd_model* m, const float* images, int B, int H, int W, float* image_embeds, float* hidden_out);
/* Replay entry of the front-end launch with the conventions of tsd_debug_ip_attn_run (test infrastructure: tests/clipvision_ref.py holds
 * the kernel to an fp64 reference, element-wise).  One int64 per argument; LD is the pitch of the patch rows in elements (>= 592, a
 * multiple of 8; columns 588 .. LD - 1 are written as zero).  Operand slots: input IMG fp32 [B][3][H][W]; output OUT fp16 [B * 256][LD].
 * host_in == NULL only sizes.  info[TSD_VI_CHANGED]: guard elements the launch changed; TAPS_H / TAPS_V: the longest coefficient row of
 * the horizontal / vertical table; ROWS: the most source rows one patch stages; LDS: bytes of LDS of the launch. */
enum tsd_imgpatch_desc_field { TSD_VD_VERSION = 0, TSD_VD_B, TSD_VD_H, TSD_VD_W, TSD_VD_LD, TSD_VD_COUNT };
#define TSD_VD_VERSION_1 1
enum tsd_imgpatch_operand { TSD_VO_IMG = 0, TSD_VO_OUT, TSD_VO_COUNT };
enum tsd_imgpatch_info { TSD_VI_CHANGED = 0, TSD_VI_TAPS_H, TSD_VI_TAPS_V, TSD_VI_ROWS, TSD_VI_LDS, TSD_VI_COUNT };
int tsd_debug_image_patches_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out, int64_t* ext,
                                int64_t* info);

/* `CLIP.forward` clip.mojo:90-109 (the step before the hot path), intended semantics
 * (App.A D3/D8/D15/D20): tokens [B][T] int32 ids (T <= 77; rows are zero-padded to 77 like clip.mojo:91-93)
 * -> context [B][77][768] fp32, the `context` input of tsd_diffusion_forward / tsd_session_upload.
 * Token embedding + learned position table, 12 x (LayerNorm, causal 12-head self-attention, +res, LayerNorm,
 * Linear 768->3072, quick-GELU x*sigmoid(1.702x), Linear 3072->768, +res), final LayerNorm. */
int tsd_clip_forward(tsd_model* m, const int32_t* tokens, int B, int T, float* context);
/* Kinds 12 - 15 are reserved and refused (TSD_E_ARG), like every number that names no kind.
 * TSD_MODEL_DIFFUSION_SD2 (16): the UNet of the Stable Diffusion 2.x checkpoints - the full-size graph of kind 6 (torch norm semantics,
 * erf-GELU) on a second step table: every attention block has head dimension 64 (5 / 10 / 20 / 20 heads at C = 320 / 640 / 1280 / 1280)
 * and its k_proj / v_proj read a 1024-wide context.  Parameter names and order are kind 6's, the norm parameters last.  Sessions, samplers,
 * seeds, v-prediction, CFG, guidance rescale, inpainting, slots and the hoist work as on kind 6; a ControlNet (an SD-1.x network) is refused.
 * TSD_MODEL_CLIP_SD2 (17): the OpenCLIP-H text encoder as diffusers ships it for SD-2.x: width 1024, 16 heads of 64, 23 layers, erf-GELU
 * MLP, torch LayerNorms and the final LayerNorm, 77 positions, vocabulary 49408; parameter names are kind 7's.
 * tsd_model_context_width: the width of the context rows a UNet (or ControlNet) model reads and of the rows a text encoder writes - 768,
 * or 1024 for the SD-2.x kinds - so callers can size `context` ([B][T][width] fp32 everywhere); TSD_E_ARG (negative) for a VAE model. */
int tsd_model_context_width(const tsd_model* m);

/* ---- prompt tokenizer (host only, no GPU): `Tokenizer` + `bpe_encode`, helpers/utils.mojo:229-327, over the
 * tokenizer_clip.bin wire format of tokenizer_creation.py:43-48 (u32 max_token_length; per token f32 score, u32 length,
 * bytes).  pipeline.mojo:37-51: Tokenizer(49408, buf); ids = bpe_encode(prompt.replace(" ", "</w>"), tokenizer). ---- */
typedef struct tsd_tokenizer tsd_tokenizer;
int tsd_tokenizer_create(const char* path, int vocab_size, tsd_tokenizer** out);
int tsd_tokenizer_create_from_memory(const void* data, size_t bytes, int vocab_size, tsd_tokenizer** out);
int tsd_tokenizer_destroy(tsd_tokenizer* t);
/* `Tokenizer.find` :270-287 (with `wrap` :200-209): id of `token`, -1 when absent. */
int tsd_tokenizer_find(const tsd_tokenizer* t, const char* token);
/* vocabulary entry `id` -> bytes (NUL-terminated, truncated to cap) and score */
int tsd_tokenizer_token(const tsd_tokenizer* t, int id, char* out, int cap, float* score);
/* `bpe_encode` :289-327. ids may be NULL to query the count; *complete = 0 when an unknown character ended it early. */
int tsd_tokenizer_encode(const tsd_tokenizer* t, const char* text, int32_t* ids, int cap, int* n_out, int* complete);
/* pipeline.mojo:127 `rescale((-1,1),(0,255),clamp=True)` (helpers/utils.mojo:577-597). */
int tsd_rescale_images_f32(tsd_ctx* ctx, const float* x, int64_t n, float* y);

/* ---- samplers (EXTENSION: the reference has `DDPMSampler` only, sampler.mojo:5-124) ------------------------------------
 * DDPM, DDIM(eta) and DPM-Solver++(2M) are one per-element update with per-step scalars,
 *     e  = (eps - eps_uncond) * cfg_scale + eps_uncond        (pipeline.mojo:117-119; e = eps without eps_uncond)
 *     x0 = (x - sigma_t e) / alpha_t                          alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t)
 *     x' = c_x x + c_e e + c_h h + c_n z                      h = the x0 of the previous step, z ~ N(0,1)
 *     h' = x0
 * TSD_SAMPLER_DDPM: Ho et al. 2020, eq. 7 (posterior mean and variance; what `DDPMSampler.step` sampler.mojo:75-109 computes).
 * TSD_SAMPLER_DDIM: Song et al. 2021, eq. 12 with sigma = eta * (eq. 16); eta = 0 is deterministic, eta = 1 is DDPM.
 * TSD_SAMPLER_DPMPP_2M: Lu et al. 2022, algorithm 2 (DPM-Solver++(2M), data prediction); first order (D = x0) on the first step,
 *   on the step onto the clean sample and whenever no valid history exists.  Takes no noise.
 * TSD_SPACING_LEADING: timesteps i * (N // n), the reference's (sampler.mojo:40-43).  TSD_SPACING_TRAILING:
 *   round(N - k N/n) - 1, k = 0..n-1: starts at N - 1, what few-step sampling needs.  The previous timestep of step i is entry
 *   i + 1 of the list; after the last entry comes the clean sample (abar = 1). */
typedef enum tsd_sampler_kind { TSD_SAMPLER_DDPM = 0, TSD_SAMPLER_DDIM = 1, TSD_SAMPLER_DPMPP_2M = 2 } tsd_sampler_kind;
typedef enum tsd_timestep_spacing { TSD_SPACING_LEADING = 0, TSD_SPACING_TRAILING = 1 } tsd_timestep_spacing;
/* Host only, no GPU (like tsd_model_param_info).  The timestep list with the first `start_step` entries dropped (`set_strength`):
 * writes min(count, cap) entries (timesteps may be NULL) and returns the count; < 0 on a bad argument. */
int tsd_sampler_timesteps(int spacing, int n_train, int n_infer, int start_step, int* timesteps, int cap);
/* Host only, no GPU.  The scalars of step i of that list, computed in double from the fp32 alphas_cumprod table (sampler.mojo:28-32):
 * out[8] = { t, t_prev (-1 = the clean sample), alpha_t, sigma_t, c_x, c_e, c_h, c_n }.  eta is read by DDIM only; have_history by
 * DPM-Solver++(2M) only (0 = first order).  A session with DDIM or DPM-Solver++(2M) steps with exactly these scalars rounded to
 * float; a DDPM session keeps the reference's fp32 scalar arithmetic and update order (`DDPMSampler.step`), which this entry's
 * DDPM row restates in double. */
int tsd_sampler_coeffs(int kind, double eta, int spacing, int n_train, int n_infer, int start_step, int i, int have_history,
                       double out[8]);
/* Op level, host fp32 in/out like the other ops: one update of n elements with caller-given scalars
 * c[6] = { alpha_t, sigma_t, c_x, c_e, c_h, c_n } - the kernel a DDIM / DPM-Solver++(2M) session launches.  eps_uncond, hist,
 * noise and hist_out may be NULL (the term / the output is skipped).  x_out and hist_out may alias nothing. */
int tsd_sampler_step_f32(tsd_ctx* ctx, const float* x, const float* eps, const float* eps_uncond, float cfg_scale,
                         const float* hist, const float* noise, int64_t n, const float* c, float* x_out, float* hist_out);
/* ---- v-prediction and zero-terminal-SNR schedules (EXTENSION; Salimans & Ho 2022; Lin et al. 2023, section 3.1 and algorithm 1) ----
 * TSD_PRED_V: the model output means v = alpha_t e - sigma_t x0, hence x0 = alpha_t x - sigma_t v and e = sigma_t x + alpha_t v, and the
 * update is
 *     v  = (v_c - v_u) * cfg_scale + v_u                      the same combine
 *     x' = c_x x + c_v v + c_h h + c_n z                      the same arithmetic, v in place of e
 *     h' = alpha_t x - sigma_t v                              the data prediction: two products and a difference, no division
 * for all three samplers: under TSD_PRED_V a DDPM session runs this update as well, with the posterior's scalars in double rounded once
 * to float (the fp32 `DDPMSampler.step` kernel restates a reference that has no v-prediction and stays the epsilon path only), and it
 * takes noise on every step with c_n != 0.
 * Zero-terminal-SNR table: from the fp32 alphas_cumprod table ac[], in double, s_i = sqrt(ac[i]),
 *     s'_i = (s_i - s_{N-1}) * s_0 / (s_0 - s_{N-1}),   ac'[i] = (float)(s'_i^2)           one rounding to float per entry
 * so ac'[N-1] is exactly 0, ac'[0] equals ac[0] to rounding and the table strictly decreases.  diffusers (rescale_zero_terminal_snr)
 * goes back through fp32 betas and a second cumprod: its table differs from this one in the last bits.  Needs n_train >= 2.
 * At a timestep with abar = 0 (the first of a trailing list on that table) alpha_t = 0, sigma_t = 1, x0 = -v: the v rows are finite
 * there (DPM-Solver++(2M)'s step is the DDIM(0) step; the step after it is first order, c_h = 0), the epsilon rows do not exist.
 * Epsilon-prediction on the zero-terminal-SNR table is therefore allowed only while no timestep of the list has abar = 0 (leading
 * spacing, or a start_step that drops it): TSD_E_ARG otherwise. */
typedef enum tsd_prediction_type { TSD_PRED_EPSILON = 0, TSD_PRED_V = 1 } tsd_prediction_type;
/* Host only, no GPU.  The alphas_cumprod table of n_train entries: zero_terminal_snr = 0 the table every session used so far (bitwise),
 * 1 its rescale above.  Writes min(n_train, cap) entries (out may be NULL) and returns n_train; < 0 on a bad argument. */
int tsd_sampler_alphas_cumprod(int n_train, int zero_terminal_snr, float* out, int cap);
/* Host only, no GPU.  tsd_sampler_coeffs for a prediction type and a table choice; (TSD_PRED_EPSILON, 0) returns tsd_sampler_coeffs'
 * doubles.  Under TSD_PRED_V out[5] multiplies v.  TSD_E_ARG for unknown values and for the refused combination above. */
int tsd_sampler_coeffs_ex(int kind, double eta, int spacing, int n_train, int n_infer, int start_step, int i, int have_history,
                          int prediction, int zero_terminal_snr, double out[8]);
/* Op level, host fp32 in/out: the v update on n elements with caller-given scalars c[6] = { alpha_t, sigma_t, c_x, c_v, c_h, c_n } - the
 * kernel a v-prediction session launches; the twin of tsd_sampler_step_f32, with the same optional pointers.  With the same c[2..5]
 * its x_out is bitwise tsd_sampler_step_f32's; hist_out is alpha_t x - sigma_t v. */
int tsd_sampler_step_v_f32(tsd_ctx* ctx, const float* x, const float* v, const float* v_uncond, float cfg_scale, const float* hist,
                           const float* noise, int64_t n, const float* c, float* x_out, float* hist_out);
/* Op level, host fp32 in/out, synchronous: the update of step i of a DDPM session with this schedule (spacing, n_train, n_infer,
 * start_step as in tsd_sampler_coeffs) on n elements - the kernel and the fp32 scalars of `DDPMSampler.step` the session launches.
 * eps_uncond and noise may be NULL; like the session, the noise is added only on a step that does not land on t = 0. */
int tsd_ddpm_step_f32(tsd_ctx* ctx, const float* x, const float* eps, const float* eps_uncond, float cfg_scale, const float* noise,
                      int64_t n, int spacing, int n_train, int n_infer, int start_step, int i, float* x_out);

/* ---- guidance rescale (EXTENSION: the reference combines cond and uncond with a fixed formula, pipeline.mojo:117-119) ----------
 * Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", eq. 15-16 (diffusers: guidance_rescale).  Per
 * sample, with c the conditional and u the unconditional eps, n = 4*L*L elements, s the guidance scale and phi in [0, 1]:
 *     e_i   = (c_i - u_i) * s + u_i                      the update's own combine: three fp32 roundings
 *     var_c = sum c^2 / n - (sum c / n)^2, var_e likewise over e                 sums and moments in fp64
 *     g     = phi * sqrt(var_c / var_e) + (1 - phi)      in fp64, rounded once to fp32
 *     c'_i  = g * c_i,  u'_i = g * u_i                   one fp32 rounding each
 * and the sampler update then runs on c', u' unchanged: its combine gives g * e up to rounding, and the DPM-Solver++(2M) history is the
 * x0 of the rescaled prediction.  g = 1 exactly (the sample passes through) when var_e is not finite, var_e <= 0 or var_c is not
 * finite; a var_c below zero counts as zero.  A sample's g is bitwise the same run to run, at every B and in every position of the
 * batch.  phi = 0 leaves a sample unread and unwritten. */
/* Op level, host fp32 in/out, synchronous: eps / eps_uncond / the outputs [B][chw], cfg_scale [B], phi [B], g_out [B] or NULL (1 for a
 * sample with phi = 0).  The outputs may be the inputs.  TSD_E_SHAPE for B outside 1..16 or chw <= 0; TSD_E_ARG for a phi that is not
 * finite or outside [0, 1] and for a cfg_scale that is not finite.  Non-finite inputs are not counted here (the update counts them). */
int tsd_cfg_rescale_f32(tsd_ctx* ctx, const float* eps, const float* eps_uncond, int B, int64_t chw, const float* cfg_scale,
                        const float* phi, float* eps_out, float* eps_uncond_out, float* g_out);

/* ---- masked denoising / inpainting (EXTENSION: the reference has txt2img and img2img only) ---------------------------------
 * The classic 4-channel inpainting: after each sampler update the known region of the latents is replaced by the original
 * latents, noised to the timestep the update has just reached,
 *     k  = a_prev * known + s_prev * noise                    a_prev = sqrt(abar_prev), s_prev = sqrt(1 - abar_prev)
 *     x' = m * x + (1 - m) * k                                m = 1: regenerate, m = 0: keep
 * every product, sum and difference one fp32 rounding in this order, so m = 1 returns x and m = 0 returns k bitwise (finite operands).
 * TSD_MASK_AREA: a latent cell's mask is the mean of its 8x8 pixel block.  TSD_MASK_ANY: 1 if any pixel of the block is >= 0.5,
 * else 0 - a cell that touches a masked pixel is regenerated. */
typedef enum tsd_mask_mode { TSD_MASK_AREA = 0, TSD_MASK_ANY = 1 } tsd_mask_mode;
/* Op level, host fp32 in/out, synchronous.  mask_px [B][8L][8L] -> mask_lat [B][L][L].  Every value must be finite and in [0, 1]
 * (TSD_E_ARG, like an unknown mode); TSD_E_SHAPE for B <= 0 or L <= 0. */
int tsd_latent_mask_f32(tsd_ctx* ctx, const float* mask_px, int B, int L, int mode, float* mask_lat);
/* The same for a rectangular mask: mask_px [B][8LH][8LW] -> mask_lat [B][LH][LW]; LH == LW gives the bits of the entry above. */
int tsd_latent_mask_hw_f32(tsd_ctx* ctx, const float* mask_px, int B, int LH, int LW, int mode, float* mask_lat);
/* Op level, host fp32 in/out, synchronous: the blend above on x / known / noise / x_out CHW [B][4][hw] and mask [B][hw] (one mask
 * value serves the 4 channels) - the kernel a session with inpainting launches after its sampler update.  noise may be NULL (k =
 * a_prev * known).  x_out may be x.  A non-finite output is counted (TSD_E_NONFINITE): an inf in x under m = 0 comes out as NaN. */
int tsd_inpaint_blend_f32(tsd_ctx* ctx, const float* x, const float* mask, const float* known, const float* noise, int B,
                          int64_t hw, float a_prev, float s_prev, float* x_out);

/* ---- seeded noise (EXTENSION: the reference draws from Mojo's stdlib PRNG) ------------------------------------------------------
 * N(0,1) as a pure function of (seed, stream id, element counter j), computed on the device in fp32:
 *     base = seed * 0x9E3779B97F4A7C15 + stream * 0xBF58476D1CE4E5B9        (uint64, wrapping; the rule of tsd_model_init_random)
 *     k1 = mix64(base + 2j) >> 40, k2 = mix64(base + 2j + 1) >> 40          (24 bits each; mix64 = the splitmix64 finaliser)
 *     z  = sqrt(-2 ln((k1 + 1) 2^-24)) * cos(pi k2 2^-23)                   |z| <= 5.77
 * tsd/rng.py normal_counter is the float64 host twin; the device value is within 14 * 2^-24 relative of it (csrc/counter_rng.h), not
 * bitwise equal: logf and cospif are the device library's. */
/* Op level, host out, synchronous: out[e] = z at counter offset + e of the stream (seed, stream), e < n.  TSD_E_SHAPE for n <= 0. */
int tsd_normal_fill_f32(tsd_ctx* ctx, uint64_t seed, uint64_t stream, uint64_t offset, int64_t n, float* out);

/* ---- device-resident denoise loop (pipeline.mojo:57-127 + sampler.mojo:15-124) --------- */

/* B samples, latent side L, T context tokens; cfg != 0 runs the UNet on 2B (cond + uncond,
 * SURVEY.md App.A D10).  `decoder` may be NULL when only latents are wanted. */
int tsd_session_create(tsd_model* diffusion, tsd_model* decoder, int B, int L, int T, int cfg, tsd_session** out);
/* A session of rectangular latents [.,4,LH,LW] (images [.,3,8LH,8LW]); tsd_session_create is its LH == LW == L case.  LH and LW are
 * multiples of 8 (16 for the full-size UNet kinds), TSD_E_SHAPE otherwise.  One session has one shape: every entry below keeps its
 * signature, and where its comment says L,L the tensor is LH,LW - latents, noise, known [.,4,LH,LW], masks [.,LH,LW], images
 * [.,3,8LH,8LW] - and L*L is LH*LW.  The seeded-noise counter is the element's index inside its sample, (c*LH + y)*LW + x. */
int tsd_session_create_hw(tsd_model* diffusion, tsd_model* decoder, int B, int LH, int LW, int T, int cfg, tsd_session** out);
int tsd_session_shape(tsd_session* s, int* LH, int* LW); /* the session's latent sides */
int tsd_session_destroy(tsd_session* s);
/* `DDPMSampler.__init__` + `set_inference_timesteps` sampler.mojo:15-44 (+ `set_strength` :67-73 via
 * start_step: the first `start_step` timesteps are dropped).  beta 0.00085..0.012 scaled-linear. */
int tsd_session_set_schedule(tsd_session* s, int num_training_steps, int num_inference_steps, int start_step);
/* Choose the sampler (see "samplers" above; default TSD_SAMPLER_DDPM / TSD_SPACING_LEADING = the reference).  eta is read by DDIM
 * only.  Rebuilds the timestep list and invalidates the upload exactly as tsd_session_set_schedule does: step() returns
 * TSD_E_STATE until upload().  DPM-Solver++(2M) keeps the previous step's x0 on the device; it is valid for step i only if the
 * previous call on the session was step(i - 1) since the last upload() / add_noise() / set_*() - otherwise step i runs first order.
 * With DDPM or DDIM(eta > 0) and no uploaded noise the update is noiseless; DPM-Solver++(2M) ignores the noise. */
int tsd_session_set_sampler(tsd_session* s, int kind, float eta, int spacing);
/* What the model output means (a tsd_prediction_type) and which alphas_cumprod table the session runs on (zero_terminal_snr 0 / 1; see
 * "v-prediction" above).  Session configuration like set_sampler: rebuilds the table and the step plans and invalidates the upload
 * (TSD_E_STATE until upload() / slots_open()); it persists across uploads; the default is (TSD_PRED_EPSILON, 0), with which a session
 * enqueues the launches and computes the bits it always did.  Everything that reads the table follows it: add_noise*, the inpainting
 * blend's scalars (lockstep and per slot) and slot_start's noise at the start - at the index of abar = 0, add_noise leaves exactly the
 * noise.  All slots share it.  Guidance rescale is unchanged: it scales the model output whatever it means.
 * TSD_E_ARG for unknown values, and from whichever of set_schedule, set_sampler and set_prediction completes epsilon-prediction on a
 * timestep list with abar = 0; a refused call leaves the session as it was. */
int tsd_session_set_prediction(tsd_session* s, int prediction, int zero_terminal_snr);
int tsd_session_prediction(tsd_session* s, int* prediction, int* zero_terminal_snr);
int tsd_session_num_steps(tsd_session* s);
int tsd_session_timestep(tsd_session* s, int i); /* i-th timestep of the schedule */
/* Upload state.  latents [B,4,LH,LW] (L,L below: the session's LH,LW); context [B,T,768]; uncond_context [B,T,768] or NULL;
 * noise [nsteps,B,4,L,L] ~ N(0,1) (an input: App.A D19) or NULL for a noiseless update. */
int tsd_session_upload(tsd_session* s, const float* latents, const float* context, const float* uncond_context,
                       const float* noise, float cfg_scale);
/* Enqueue step i: time embedding -> Diffusion.forward (x1 or x2 with CFG combine) -> DDPMSampler.step
 * (sampler.mojo:75-109), or the update of the sampler chosen with tsd_session_set_sampler.  Asynchronous on the context stream. */
int tsd_session_step(tsd_session* s, int i);
/* `add_noise` sampler.mojo:111-124 at timestep index i (img2img), noise [B,4,L,L] host. */
int tsd_session_add_noise(tsd_session* s, int i, const float* noise);
/* Masked denoising (see "masked denoising" above) for the steps of the current upload: mask [B][L][L] (1 = regenerate, 0 = keep),
 * known [B,4,L,L] (the original latents), noise [B,4,L,L] or NULL for a noiseless known region; all host, copied into buffers the
 * session owns; synchronous.  While it is on, step(i) launches the blend in place on the latents after its sampler update, with the
 * scalars of the timestep the update lands on: entry i + 1 of the list (tsd_sampler_coeffs(..., i + 1, ...) out[2], out[3] rounded to
 * float), (1, 0) after the last entry - the same for all three samplers.  mask == NULL turns it off (known and noise are ignored).
 * It belongs to one upload: TSD_E_STATE before tsd_session_upload; upload(), set_schedule and set_sampler turn it off.  TSD_E_ARG,
 * with the previous state unchanged, for a mask value that is not finite or outside [0, 1], for a missing known and for inf / NaN in
 * known or noise.  The latents are not modified; like add_noise it drops the DPM-Solver++(2M) history (the next step runs first order)
 * and the decoded images.  A session that never calls it enqueues exactly the launches it enqueued before. */
int tsd_session_set_inpaint(tsd_session* s, const float* mask, const float* known, const float* noise);
int tsd_session_inpaint_active(tsd_session* s); /* 1 / 0; < 0 on a NULL session */
/* Seeded device-side noise (see "seeded noise" above) for the steps of the current upload, one seed per sample: seeds [B] host, NULL
 * turns it off.  While it is on, a DDPM step (t > 0) and a DDIM(eta > 0) step draw their noise inside the update kernel from stream
 * 16 + i of seeds[b] - i the step index, the counter the element's index inside its sample (c*L + y)*L + x - with no noise buffer and no
 * extra launch; the result is bitwise that of a session whose uploaded noise[i][b] is tsd_normal_fill_f32(seeds[b], 16 + i, 0, 4*L*L).
 * A sample's noise depends on its seed alone, never on B or on its slot in the batch.  DPM-Solver++(2M) takes no noise and ignores it.
 * It belongs to one upload: TSD_E_STATE before tsd_session_upload and when that upload carried a noise tensor (one source of noise per
 * upload); upload(), set_schedule and set_sampler turn it off.  Like add_noise it drops the DPM-Solver++(2M) history and the decoded
 * images.  A session that never calls it enqueues exactly the launches, and computes the bits, it did before. */
int tsd_session_set_seeds(tsd_session* s, const uint64_t* seeds);
int tsd_session_seeds_active(tsd_session* s); /* 1 / 0; < 0 on a NULL session */
/* Replace the latents by stream 2 of each sample's seed (txt2img's initial latents; asynchronous).  TSD_E_STATE without seeds. */
int tsd_session_seed_latents(tsd_session* s);
/* tsd_session_add_noise at timestep index i with stream 4 of each sample's seed instead of a host tensor: the same scalars, the same
 * kernel.  TSD_E_STATE without seeds, TSD_E_ARG for an index outside the schedule. */
int tsd_session_add_noise_seeded(tsd_session* s, int i);
/* tsd_session_set_inpaint whose noise is stream 4 of each sample's seed (the values add_noise_seeded used), filled into the session's
 * buffer on the device.  Validation and state rules are set_inpaint's; TSD_E_STATE for a mask without seeds.  mask == NULL turns
 * inpainting off. */
int tsd_session_set_inpaint_seeded(tsd_session* s, const float* mask, const float* known);
/* Guidance rescale (see "guidance rescale" above) for the steps of the current upload, one phi for the batch; 0 turns it off.  While
 * phi > 0, step(i) enqueues two short launches between the forward and the sampler update that scale every sample's cond and uncond
 * eps in place by its g - no host-to-device copy, no allocation, no synchronisation - with all three samplers, with or without seeds,
 * inpainting and the hoist.  It belongs to one upload: TSD_E_STATE before tsd_session_upload and on a session created with cfg = 0;
 * upload(), set_schedule and set_sampler turn it off.  TSD_E_ARG for a phi that is not finite or outside [0, 1].  It touches neither
 * the latents, the history nor the decoded images.  With phi = 0, or never called, a session enqueues exactly the launches, and
 * computes the bits, it did before. */
int tsd_session_set_guidance_rescale(tsd_session* s, float phi);
int tsd_session_guidance_rescale(tsd_session* s, float* phi); /* *phi = the value in force (0 = off, also before upload()) */
int tsd_session_decode(tsd_session* s); /* Decoder.forward on the current latents (async) */
int tsd_session_download_latents(tsd_session* s, float* latents);
int tsd_session_download_images(tsd_session* s, int rescale_0_255, float* images);

/* ---- slot sessions (EXTENSION: the reference denoises one prompt from step 0 to the end, pipeline.mojo:86-124) ------------------------
 * Continuous batching: each of the B samples of a session is a SLOT holding its own request - context, seed, guidance scale - and its
 * own index into the session's timestep list.  One advance() runs ONE UNet forward over all samples and gives every active slot the
 * sampler update of its own index; a slot that has finished is refilled by slot_start while the others keep going.  Each entry point
 * stands in for the body of `pipeline.generate`'s loop (pipeline.mojo:86-124: time embedding, Diffusion.forward, the CFG combine :117-119,
 * DDPMSampler.step), per sample.  All slots share the session's sampler, spacing and timestep list.  Noise is always the seeded noise
 * above: streams 2 / 4 / 16 + i of the slot's seed.  A slot's latents are bit for bit those of a lockstep session of the same B running
 * the same request in the same sample position (upload + set_seeds + seed_latents | add_noise_seeded + step start_index..n-1).
 * Inpainting is per slot: tsd_session_slot_set_inpaint gives one request a mask and known latents, and the update launch of an advance
 * blends them in (no extra launch); the lockstep set_inpaint* stay refused in slot mode.
 * A session that never calls slots_open enqueues exactly the launches, and computes the bits, it did before. */
/* Enter slot mode, after set_sampler / set_schedule and in place of upload(): sizes the workspace and the hoisted buffers by upload()'s
 * planning pass, zeroes the latents and the context, marks all B slots idle.  upload(), set_schedule and set_sampler leave slot mode.
 * In slot mode step, add_noise*, set_seeds, seed_latents, set_inpaint*, decode, download_latents and download_images return
 * TSD_E_STATE. */
int tsd_session_slots_open(tsd_session* s);
/* Put a request into slot b (idle, done or active: an active slot's request is replaced).  context [T,768]; uncond_context [T,768]
 * (NULL only without CFG); latents [4,L,L] or NULL = stream 2 of `seed` (tsd_session_seed_latents' rule); with latents and
 * noise_at_start != 0 they are noised to timesteps[start_index] with stream 4 of `seed` (tsd_session_add_noise_seeded's scalars and
 * kernel, img2img).  The slot's next step is start_index; its DPM-Solver++(2M) history is dropped.  Synchronous.  Every refusal comes
 * before the first copy and leaves all slots as they were: TSD_E_ARG for b or start_index out of range, a missing uncond_context on a
 * CFG session, inf / NaN in a host tensor or in cfg_scale; TSD_E_STATE outside slot mode.  Other slots' buffers are never touched: with
 * the step invariants hoisted, only this sample's context K / V^T are rebuilt, in place. */
int tsd_session_slot_start(tsd_session* s, int b, const float* context, const float* uncond_context, const float* latents,
                           int noise_at_start, uint64_t seed, int start_index, float cfg_scale);
/* One tick, asynchronous like tsd_session_step: one forward over all samples, then every ACTIVE slot b takes the update of its index
 * i_b with its own cfg_scale, its noise from stream 16 + i_b of its seed (where the sampler takes noise) and its own DPM-Solver++(2M)
 * history; i_b grows by one, a slot that reaches tsd_session_num_steps becomes done and sets bit b of *finished_mask (may be NULL).
 * Idle and done slots ride through the forward: their output is ignored, their latents and history are not written and they are not
 * counted as non-finite.  The per-slot scalars travel as kernel arguments: no host-to-device copy, no allocation.  TSD_E_STATE with no
 * active slot or outside slot mode; otherwise tsd_session_step's guards (a parameter change rebuilds the invariants of all samples). */
int tsd_session_advance(tsd_session* s, uint32_t* finished_mask);
/* *index = the slot's next schedule index (num_steps when done), *state = 0 idle, 1 active, 2 done; either may be NULL. */
int tsd_session_slot_state(tsd_session* s, int b, int* index, int* state);
/* Masked denoising for the request of ACTIVE slot b - right after slot_start, or mid-flight: mask [L,L] in [0,1] (1 = regenerate, 0 = keep)
 * and known [4,L,L], the original latents, are copied into sample b's region of the session's inpainting buffers; the noise they are
 * re-noised with is stream 4 of the slot's seed, filled on the device - the values tsd_session_set_inpaint_seeded fills for that sample
 * and slot_start(noise_at_start) adds.  From then on the update of every advance holds the slot's known region at the timestep ITS step
 * reaches (entry i_b + 1 of the list, the clean sample after the last), inside the update kernel: an advance with inpainting slots
 * enqueues the launches of one without.  The slot's latents are bit for bit sample b of a lockstep session running set_inpaint_seeded with
 * this mask.  mask == NULL turns the slot's inpainting off.  Either way the slot's DPM-Solver++(2M) history is dropped.  slot_start and
 * slots_open turn it off: a refilled slot never inherits a mask.  Synchronous.  Every refusal comes before the first copy and leaves all
 * slots as they were: TSD_E_ARG for b out of range, a mask value that is not finite or not in [0, 1], a missing `known`, inf / NaN in
 * `known`; TSD_E_STATE outside slot mode and on an idle or done slot.  Other slots' buffers are never written. */
int tsd_session_slot_set_inpaint(tsd_session* s, int b, const float* mask, const float* known);
int tsd_session_slot_inpaint_active(tsd_session* s, int b); /* 1 / 0; < 0 on error (NULL session, outside slot mode, b out of range) */
/* Guidance rescale for the request of ACTIVE slot b, per request like cfg_scale: an advance with some active slot at phi > 0 enqueues
 * the two launches of tsd_session_set_guidance_rescale with a per-sample table; idle and done slots and slots at phi = 0 are neither
 * read nor written by them, and an advance with no such slot enqueues what it always did.  The slot's latents are bit for bit sample b
 * of a lockstep session running its request with the same phi.  slot_start and slots_open clear it: a refilled slot never inherits
 * it.  TSD_E_ARG for b out of range and a phi that is not finite or outside [0, 1]; TSD_E_STATE outside slot mode, on an idle or done
 * slot and on a session created with cfg = 0.  The latents and the history are not touched. */
int tsd_session_slot_set_guidance_rescale(tsd_session* s, int b, float phi);
int tsd_session_slot_guidance_rescale(tsd_session* s, int b, float* phi); /* *phi = the active slot's value, 0 otherwise */
/* One slot's latents [4,L,L] (synchronises).  TSD_E_STATE on an idle slot.  tsd_session_download_latents' finite check, on that slot's
 * buffer only: inf / NaN there returns TSD_E_NONFINITE and latches the session until slots_open() or upload(). */
int tsd_session_slot_download(tsd_session* s, int b, float* latents);
int tsd_session_slots_active(tsd_session* s); /* number of active slots (0 outside slot mode); < 0 on a NULL session */

/* ---- multi-GPU: RCCL over xGMI (one process per GPU) ----------------------------------- */
/* unique_id: 128 bytes from tsd_dist_unique_id on rank 0, shared out-of-band (e.g. torch.distributed). */
int tsd_dist_unique_id(void* id128);
/* A context holds at most one communicator: TSD_E_STATE, and nothing changes, on a context that already has one (tsd_dist_finalize
 * first).  tsd_ctx_destroy finalizes a communicator that is still live. */
int tsd_dist_init(tsd_ctx* ctx, int rank, int nranks, const void* id128);
int tsd_dist_broadcast_weights(tsd_model* m, int root); /* ncclBroadcast of the packed blob */
/* ranks of the communicator tsd_dist_init created (ncclCommCount): what RCCL itself holds, not what the caller passed in */
int tsd_dist_comm_count(tsd_ctx* ctx, int* nranks);
int tsd_dist_finalize(tsd_ctx* ctx);

/* ---- debug / tuning -------------------------------------------------------------------- */
/* Every switch below belongs to ONE context: the library keeps no process-global mutable state besides the thread-local error
 * string and the ledger of device resources (tsd_debug_device_ledger below: counters behind a mutex that no call reads to decide
 * anything), so two contexts (one per GPU, each driven by its own host thread) may run different settings side by side.  The
 * TSD_* environment variables named here are read once, by tsd_ctx_create, into that context.  A denoise session sizes its
 * workspace for the settings active at upload(): after a tsd_debug_set_* call that CHANGES a setting of its context, step() /
 * decode() fail with TSD_E_STATE until upload() is called again (setting the value that is already there changes nothing).
 * Every tsd_debug_set_* returns the previous setting, always >= 0; an out-of-range value is ignored; the only negative
 * return is TSD_E_ARG (-1) for a NULL context.
 * Non-finite results are sticky per SESSION: once a session download has returned TSD_E_NONFINITE, every later step(), decode()
 * and download of that session returns it again until upload() replaces the session's state. */
/* split-K hand-offs that timed out or paired blocks on different XCDs since the context was created (must be 0);
 * 1 when workgroups map to XCDs round-robin (the precondition of the L2-local split-K hand-off). */
int tsd_debug_splitk_errors(tsd_ctx* ctx);
int tsd_debug_xcd_round_robin(void);
/* Non-finite values (inf / NaN) written to caller-visible tensors on this context since the last report: the path stores
 * activations as fp16 (|x| <= 65504) where the reference computes in fp32 (helpers/utils.mojo:12-15), so an overflow is possible
 * and must never be silent.  Every kernel that produces a tensor that leaves the device counts what it writes; the synchronous
 * entry points, tsd_ctx_synchronize and the session downloads return TSD_E_NONFINITE when the count is non-zero (and clear it).
 * This call reads the count without failing (reset != 0 clears it); < 0 on error.  Synchronises the context's stream. */
int tsd_debug_nonfinite_count(tsd_ctx* ctx, int reset);
/* Test infrastructure: fill the context's whole workspace arena and whole staging buffer, as allocated now, with `byte` (0..255), on the
 * context's stream; a region that is not allocated yet is skipped.  Both are per-call scratch (DESIGN.md "Workspace rule"): no result
 * of any later call may depend on the byte.  Nothing else is touched - not the split-K hand-off flags, not the status words, not a
 * table, a model or a session.  TSD_E_ARG for a NULL context or a byte outside 0..255.  Does not synchronise.
 * TSD_DEBUG_POISON=<byte> in the environment of tsd_ctx_create is the same statement about FRESH allocations: those selected by
 * TSD_DEBUG_POISON_WHAT (default 31: 1 arena, 2 derived weights, 4 session state, 8 every buffer a session allocates or grows
 * later - context K/V, noise, time table and rows, control, IP-Adapter K/V - 16 staging) are filled with the byte when allocated. */
int tsd_debug_scribble(tsd_ctx* ctx, int byte);
/* Test infrastructure: the session's raw latent buffer [B,4,L,L] as it is on the device - in any mode, idle slots included, with no
 * finite check and no effect on the session's state.  Synchronises. */
int tsd_debug_session_latents(tsd_session* s, float* latents);
/* A/B switch for the fused attention-block kernels of the 64x64 level (kernels_chain.hip): 0 = op-by-op graph, 1 = fused
 * (default; TSD_CHAIN=0 in the environment has the same effect).  Returns the previous setting. */
int tsd_debug_set_fused_attention(tsd_ctx* ctx, int on);
/* Time one GEMM (conv = 0: M = B*H*W, K = Cin) or conv3x3 problem on synthetic device data with tile
 * configuration `cfg` (< 0: dispatcher's choice); average ms per launch over `iters` launches. */
int tsd_debug_gemm_bench(tsd_ctx* ctx, int conv, int B, int H, int W, int Cin, int N, int stride, int ups, int cfg,
                         int iters, float* ms);

/* Run one problem with tile configuration `cfg` and with `ref_cfg`; max |difference| and max |reference|. */
int tsd_debug_gemm_check(tsd_ctx* ctx, int conv, int B, int H, int W, int Cin, int N, int stride, int ups, int cfg,
                         int ref_cfg, float* max_abs_diff, float* max_abs_ref);
/* ---- GEMM / conv3x3 launch descriptors (test infrastructure: tests/gemm_ref.py holds every launch to an fp64 reference) ----
 * One internal GEMM launch as int64 fields, one per GemmArgs field (csrc/common.h).  Pitches and strides are in elements.
 * K0: the dense concat split (K when there is no second source).  PAD: top/left padding; HO / WO carry what an asymmetric pad
 * implies.  W_KTS: 1 when the launch reads the K-tile-major weight copy.  OUT_SCALE: the float's bits.  ALIAS: bit 0 R == C
 * (in-place residual), bit 1 A1 == A0, bit 2 A2 == A1.  SK_BIG: the context's long-K split setting at the launch.  CFG / WAYS:
 * tile configuration and split-K slices that ran (written by the dispatcher). */
enum tsd_gemm_desc_field {
  TSD_GD_VERSION = 0, TSD_GD_CONV, TSD_GD_M, TSD_GD_N, TSD_GD_K, TSD_GD_K0,
  TSD_GD_LDA0, TSD_GD_LDA1, TSD_GD_LDA2, TSD_GD_LDW, TSD_GD_LDW1, TSD_GD_LDR, TSD_GD_LDC,
  TSD_GD_BATCH, TSD_GD_SA, TSD_GD_SW, TSD_GD_SC, TSD_GD_SR,
  TSD_GD_HS, TSD_GD_WS, TSD_GD_HO, TSD_GD_WO, TSD_GD_CIN, TSD_GD_STRIDE, TSD_GD_PAD, TSD_GD_UPS,
  TSD_GD_CIN1, TSD_GD_CIN2, TSD_GD_W_KTS,
  TSD_GD_EPI, TSD_GD_OUT_SCALE, TSD_GD_ROWVEC_LD, TSD_GD_ROWS_PER_BATCH,
  TSD_GD_VT, TSD_GD_VT_N0, TSD_GD_VT_LD, TSD_GD_VT_S, TSD_GD_VT_SB,
  TSD_GD_GN_GROUPS, TSD_GD_GN_RPS, TSD_GD_GN_NSLAB, TSD_GD_RPS_HINT, TSD_GD_SK_BIG, TSD_GD_ALIAS,
  TSD_GD_CFG, TSD_GD_WAYS,
  TSD_GD_COUNT
};
#define TSD_GD_VERSION_1 1
/* Operand slots of tsd_debug_gemm_run: inputs A0 A1 A2 W Wt1 R (fp16) bias rowvec (fp32); outputs C (fp16, fp32 under
 * EPI_OUT_F32), Vt (fp16), GroupNorm partials (fp32). */
enum tsd_gemm_operand { TSD_GO_A0 = 0, TSD_GO_A1, TSD_GO_A2, TSD_GO_W, TSD_GO_WT1, TSD_GO_R, TSD_GO_BIAS, TSD_GO_ROWVEC, TSD_GO_C,
                        TSD_GO_VT, TSD_GO_GN, TSD_GO_COUNT };
/* on != 0: clear the list and record the descriptor of every GEMM launch enqueued on this context from now on (planning passes
 * do not count); on == 0: stop.  Returns the number of descriptors held. */
int tsd_debug_gemm_record(tsd_ctx* ctx, int on);
/* Copy recorded descriptor i (n >= TSD_GD_COUNT fields) into desc; returns TSD_GD_COUNT. */
int tsd_debug_gemm_recorded(tsd_ctx* ctx, int i, int64_t* desc, int n);
/* Run one launch described by desc on caller operands (host_in[TSD_GO_A0 .. TSD_GO_ROWVEC]; NULL for unused slots) and return
 * its outputs (host_out[TSD_GO_C .. TSD_GO_GN] at index slot - TSD_GO_C).  Every operand is passed in its device layout - element
 * i of slot s at offset i, ext[s] elements - except W under W_KTS, which is row-major [N][K] (the entry builds the K-tile-major
 * copy).  host_in == NULL only sizes (ctx may be NULL): ext[TSD_GO_COUNT] receives every slot's extent (0 = unused).
 * cfg < 0: the dispatcher's choice (split-K included, SK_BIG applied for the call); cfg >= 0: that tile configuration, no split.
 * Inputs and outputs sit between 4 KiB guard bands of a NaN pattern; outputs are pre-filled with it (C with R when ALIAS bit 0).
 * info[0] configuration, [1] split-K slices that ran, [2] guard / pitch-gap elements the launch changed.  The outputs are
 * returned even when the launch is refused (its status is the return value). */
int tsd_debug_gemm_run(tsd_ctx* ctx, const int64_t* desc, int n, int cfg, const void* const* host_in, void* const* host_out,
                       int64_t* ext, int64_t* info);
/* The host plan of the launch desc describes (csrc/gemm_plan.cpp: what launch_gemm acts on), without running it: plan[TSD_GP_COUNT]
 * receives the tile configuration that would run and its split-K slices (what tsd_debug_gemm_run reports as info[0], info[1]), the conv
 * variant (0 plain, 1 halo-x, 2 fused 1x1 skip, 3 upsample fold), the tile and one wave's sub-tile, the K the launch executes (4 * CIN
 * under the upsample fold), the split-K workspace in floats, the LDS bytes, and the GroupNorm statistics slabs per sample the tile can
 * emit for the descriptor's GN_RPS / GN_GROUPS (0: none).  cfg as in tsd_debug_gemm_run.  No device is touched: ctx == NULL plans under
 * the options of the environment (the defaults when no TSD_* variable is set) and the descriptor's SK_BIG.  TSD_E_ARG for a tile
 * configuration the build does not have, or one without the variant the launch needs. */
enum tsd_gemm_plan_field { TSD_GP_CFG = 0, TSD_GP_WAYS, TSD_GP_VARIANT, TSD_GP_BM, TSD_GP_BN, TSD_GP_BMW, TSD_GP_BNW, TSD_GP_K,
                           TSD_GP_WS_FLOATS, TSD_GP_LDS_BYTES, TSD_GP_GN_NSLAB, TSD_GP_COUNT };
int tsd_debug_gemm_plan(tsd_ctx* ctx, const int64_t* desc, int n, int cfg, int64_t* plan);
/* ---- GroupNorm / LayerNorm launch descriptors (test infrastructure: tests/norm_ref.py holds every statistics path of
 * csrc/kernels_norm.hip to an fp64 reference) ----
 * One int64 per argument of launch_groupnorm / launch_gn_stats / launch_gn_finalize / launch_layernorm.  EPS and GAMMA hold the bits
 * of a float.  C0 < C: channels [C0, C) come from the second source (X1, pitch LD1).  HAS_W / HAS_B / TORCH_RSTD: the NormAffine
 * extension (none set: reference semantics, no NormAffine passed).  STATS (groupnorm mode only): where the statistics come from -
 * 0 the launch's own pass over x, 1 one table of NSLAB producer partials per sample (PART0, [B][NSLAB][GROUPS][2]), 2 a GnComposite
 * of NSLAB slabs: G0 fine groups in PART0 ([B][NSLAB][G0][2]), G1 in PART1 (G1 == 0: no second table), COMB fine groups per group.
 * gn_finalize mode reads PART0 [B][NSLAB][GROUPS][2] and no x.  layernorm mode: ROWS rows of C channels, x at pitch LD0, y at LDY. */
enum tsd_norm_desc_field {
  TSD_ND_VERSION = 0, TSD_ND_MODE, TSD_ND_B, TSD_ND_HW, TSD_ND_C, TSD_ND_C0, TSD_ND_LD0, TSD_ND_LD1, TSD_ND_LDY, TSD_ND_GROUPS,
  TSD_ND_EPS, TSD_ND_GAMMA, TSD_ND_SILU, TSD_ND_HAS_W, TSD_ND_HAS_B, TSD_ND_TORCH_RSTD,
  TSD_ND_STATS, TSD_ND_NSLAB, TSD_ND_G0, TSD_ND_G1, TSD_ND_COMB, TSD_ND_ROWS,
  TSD_ND_COUNT
};
#define TSD_ND_VERSION_1 1
enum tsd_norm_mode { TSD_NM_GROUPNORM = 0, TSD_NM_GN_STATS, TSD_NM_GN_FINALIZE, TSD_NM_LAYERNORM };
/* Operand slots: inputs X0 X1 (fp16) PART0 PART1 W BIAS (fp32); outputs Y (fp16), STATS (fp32 [B][GROUPS][2] (mean, scale)). */
enum tsd_norm_operand { TSD_NO_X0 = 0, TSD_NO_X1, TSD_NO_PART0, TSD_NO_PART1, TSD_NO_W, TSD_NO_BIAS, TSD_NO_Y, TSD_NO_STATS, TSD_NO_COUNT };
/* info: guard / pitch-gap elements the launches changed, then the plan the GroupNorm launch took (all 0 when it was refused, and
 * for layernorm): the slab count the statistics were finished from, whether the launch ran its own statistics pass, k_gn_prereduce,
 * the separate k_gn_finalize launch, whether the composite was accepted, pixels per statistics slab and per apply block, pixel
 * lanes per block. */
enum tsd_norm_info { TSD_NI_CHANGED = 0, TSD_NI_NSLAB, TSD_NI_OWN_PASS, TSD_NI_PREREDUCE, TSD_NI_FINALIZE, TSD_NI_COMPOSITE,
                     TSD_NI_SLAB_PIXELS, TSD_NI_APPLY_PIXELS, TSD_NI_PL, TSD_NI_COUNT };
/* Run the launch described by desc (n >= TSD_ND_COUNT fields) on caller operands in their device layout (host_in[TSD_NO_X0 ..
 * TSD_NO_BIAS], NULL for unused slots) and return its outputs (host_out[slot - TSD_NO_Y]).  host_in == NULL only sizes (ctx may be
 * NULL, no device is touched): ext[TSD_NO_COUNT] receives every slot's extent (0 = unused) and, when info is given, info[] the plan
 * under the default options.  A descriptor that cannot be sized is refused before any launch.  Every operand sits between 4 KiB
 * guard bands of a NaN pattern and the outputs are pre-filled with it; they are returned even when the launch is refused (its
 * status is the return value). */
int tsd_debug_norm_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out, int64_t* ext,
                       int64_t* info);
/* ---- attention-core / row-softmax launch descriptors (test infrastructure: tests/attn_ref.py holds flash_attn_kernel<40,1>, <40,2>,
 * <80,1>, <160,1>, flash_attn8_kernel<40> and the k_softmax_rows kernels to an fp64 reference, element-wise) ----
 * One int64 per argument of launch_flash_attention: pitches and batch strides in elements, SCALE the bits of a float.  KERNEL: the d = 40
 * kernel mode of tsd_debug_set_attn_qb for this call (0 = by shape); DIAG: tsd_debug_set_attn_diag for this call.  Both are restored.
 * softmax_rows mode: ROWS rows of COLS columns at pitch LD; DTYPE 0 = fp32 (launch_softmax_rows_f32: dense, LD == COLS, X -> O), 1 = fp16
 * in place (launch_softmax_rows_f16; with CAUSAL > 0 launch_softmax_rows_f16_causal, period CAUSAL, columns [kept, ZERO_TO) zeroed).
 *
 * The V^T pad-column contract.  The kernels stream V^T in 8-column chunks and the last key tile reads every chunk that starts below
 * Skv = min(round_up(Sk, 8), ldvt): columns [Sk, Skv) reach the P.V MFMA with P = 0, and 0 x NaN = NaN, so they must hold FINITE values
 * (columns >= Skv, the K pitch gap and K rows >= Sk are never read).  Every producer of a V^T operand writes them (csrc/, read for this):
 *   - cross-attention, Sk = T (77), pitch Tp = round_up(T, 8).  The context is converted by launch_f32_to_f16_rows with rows_dst = Tp,
 *     which writes rows [T, Tp) as zeros (kernels_elementwise.hip k_f32_to_f16_rows; called at api_ops.cpp:482 and :604, by
 *     tsd_diffusion_forward and by session_put_context, session.cpp - the session's context).  Every V^T GEMM then computes all Tp columns from those rows: the swapped-operand
 *     GEMMs with N = Tp (api_ops.cpp:489, graph.cpp:276-281 and :474-479) and the fused K | V^T GEMM over M = B * Tp rows with vt_S = Tp
 *     (graph.cpp:462-468, which also builds the session's hoisted context V^T, session_build_invariants).  Columns [T, Tp) hold W_v . 0 (+ b_v):
 *     finite, whatever the arena held.
 *   - self-attention, Sk = S = H * W.  The fused q | k | V^T GEMM (graph.cpp:236-242, :391-397) and the fused block head (graph.cpp:217-225)
 *     run only where Sp == S (no pad columns).  Otherwise g_unet_attn zeroes the whole V^T buffer before the swapped-operand GEMM writes its
 *     S columns (graph.cpp:232); tsd_self_attention_f32 and the VAE block refuse T % 8 != 0 (api_ops.cpp:435, graph.cpp:415).
 * No path leaves arena contents there.  tests/test_gpu_attn_ref.py runs the core with 0 and with +-60000 in those columns (same bits) and
 * tsd_cross_attention_f32 at T = 77 on an arena filled with an fp16 NaN pattern and with zeros (same bits, finite). */
enum tsd_attn_desc_field {
  TSD_AD_VERSION = 0, TSD_AD_MODE, TSD_AD_B, TSD_AD_H, TSD_AD_D, TSD_AD_SQ, TSD_AD_SK, TSD_AD_LDQ, TSD_AD_LDK, TSD_AD_LDVT, TSD_AD_LDO,
  TSD_AD_SQB, TSD_AD_SKB, TSD_AD_SVTB, TSD_AD_SOB, TSD_AD_SCALE, TSD_AD_KERNEL, TSD_AD_DIAG,
  TSD_AD_ROWS, TSD_AD_COLS, TSD_AD_LD, TSD_AD_DTYPE, TSD_AD_CAUSAL, TSD_AD_ZERO_TO,
  TSD_AD_COUNT
};
#define TSD_AD_VERSION_1 1
/* Version 2 has the fields of version 1 and admits head dimension 64 (flash_attn_kernel<64, 1>, TSD_AK_64).  A version-1 descriptor keeps
 * what it always did with d = 64: it is sized, the run is refused with the launcher's status, reports kernel 0 and writes nothing. */
#define TSD_AD_VERSION_2 2
enum tsd_attn_mode { TSD_AM_ATTN = 0, TSD_AM_SOFTMAX_ROWS };
/* Operand slots: inputs Q [B][Sq][ldq], K [B][Sk][ldk], V^T [B][H*d][ldvt] (fp16), X (softmax_rows input: fp32, or the fp16 rows the
 * launch overwrites); output O (attention: [B][Sq][ldo] fp16; softmax_rows: the rows, in X's type and layout). */
enum tsd_attn_operand { TSD_AO_Q = 0, TSD_AO_K, TSD_AO_VT, TSD_AO_X, TSD_AO_O, TSD_AO_COUNT };
enum tsd_attn_kernel { TSD_AK_NONE = 0, TSD_AK_40_1, TSD_AK_40_2, TSD_AK_40_8W, TSD_AK_80, TSD_AK_160, TSD_AK_64 };
/* info: guard / pitch-gap elements the launch changed; the kernel that ran (tsd_attn_kernel; softmax_rows: 1 k_softmax_rows<float>,
 * 2 k_softmax_rows<half_t>, 3 / 4 k_softmax_rows_h8<1> / <2>); workgroups that took the exact repeat in this launch; the diag and xcd_map
 * values passed to the kernel. */
enum tsd_attn_info { TSD_AI_CHANGED = 0, TSD_AI_KERNEL, TSD_AI_EXACT_WGS, TSD_AI_DIAG, TSD_AI_XCD_MAP, TSD_AI_COUNT };
/* Run the launch described by desc (n >= TSD_AD_COUNT fields) on caller operands in their device layout (host_in[TSD_AO_Q .. TSD_AO_X],
 * NULL for unused slots) through launch_flash_attention / launch_softmax_rows_* and return its output (host_out[0]).  host_in == NULL only
 * sizes (ctx may be NULL, no device is touched): ext[TSD_AO_COUNT] receives every slot's extent (0 = unused) and, when info is given,
 * info[TSD_AI_KERNEL / DIAG / XCD_MAP] what the dispatcher chooses under the default options (with the descriptor's KERNEL and DIAG).  A
 * descriptor that cannot be sized is refused before any launch; the shapes the launchers refuse (head dimension, misaligned pitches, empty
 * sequence: sized as one row) are sized and left to them.  Every operand sits between 4 KiB guard bands of a NaN pattern and O is
 * pre-filled with it (fp16 softmax_rows: with X); the output is returned even when the launch is refused (its status is the return
 * value). */
int tsd_debug_attn_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out, int64_t* ext,
                       int64_t* info);
/* ---- fused attention-block head / tail launch descriptors (test infrastructure: tests/chain_ref.py holds attn_chain_kernel<KIND_HEAD>,
 * attn_chain_kernel<KIND_TAIL> and the two weight-stream packers of csrc/kernels_chain.hip to an fp64 reference, element-wise) ----
 * One int64 per argument of launch_attn_tail / launch_attn_head (AttnTailArgs / AttnHeadArgs, csrc/common.h): B samples of S token rows
 * (M = B * S), T context keys, pitches and per-sample strides in elements, SCALE and EPS the bits of a float.  C, D, HEADS are the
 * block's width, head dimension and head count: the kernels exist for 320 / 40 / 8 only and every other value is refused by the launch,
 * not by the sizing.  GN (tail, 0 / 1): emit the output's GroupNorm(32) partials, one slab per 32 rows (nslab = S / 32).  LDW_*: the
 * pitch of each row-major weight (tail: SO, Q, CO, 1, 2, OUT; head: C, IN).  The entry builds the packed weight stream itself
 * (launch_attn_tail_pack / launch_attn_head_pack, into a guarded scratch operand) from the caller's row-major weights.
 *
 * The tail's pad contract for the context operands (csrc/kernels_chain.hip, the context staging): K rows >= T are never read - their
 * lanes fetch at PAD_OFF, beyond the buffer descriptor, which returns zeros; V^T is staged in 8-column chunks and every chunk that starts
 * below round_up(T, 8) is read whole: columns [T, round_up(T, 8)) reach the P.V MFMA with P = 0, and 0 x NaN = NaN, so they must hold
 * FINITE values; columns >= round_up(T, 8) (and the pitch gaps of K) are never read.  The producers of the context V^T write those
 * columns (see the attention entry's note above: the context is padded with zero rows to round_up(T, 8)). */
enum tsd_chain_desc_field {
  TSD_CD_VERSION = 0, TSD_CD_MODE, TSD_CD_B, TSD_CD_S, TSD_CD_T, TSD_CD_C, TSD_CD_D, TSD_CD_HEADS,
  TSD_CD_LD_AO, TSD_CD_LD_TOK, TSD_CD_LD_X, TSD_CD_LD_OUT, TSD_CD_LDK, TSD_CD_SKB, TSD_CD_LDVT, TSD_CD_SVTB, TSD_CD_SCALE, TSD_CD_EPS,
  TSD_CD_GN, TSD_CD_LD_QK, TSD_CD_LD_VT, TSD_CD_S_VT,
  TSD_CD_LDW_SO, TSD_CD_LDW_Q, TSD_CD_LDW_CO, TSD_CD_LDW_1, TSD_CD_LDW_2, TSD_CD_LDW_OUT, TSD_CD_LDW_C, TSD_CD_LDW_IN,
  TSD_CD_COUNT
};
#define TSD_CD_VERSION_1 1
enum tsd_chain_mode { TSD_CM_HEAD = 0, TSD_CM_TAIL };
/* Operand slots, in the device layout.  Tail inputs: AO, TOK, X [M][ld] fp16; KC [B][>= T][LDK]; VT [B][C][LDVT]; WSO, WQ, WCO, WOUT
 * [C][ldw], W1 [8C][ldw] and B1 [8C] in the interleaved (a, g) row order of k_pack_linear (row 2q = "a" unit q, row 2q + 1 = gate q), W2
 * [C][ldw] of 4C columns (fp16); BSO, BCO, B1, B2, BOUT fp32.  Head inputs: X; GN_STATS [B][32][2] fp32 (mean, 1 / (sigma + eps)); WC
 * [C][ldw], WIN [3C][ldw] (fp16); B_IN fp32.  Tail outputs: OUT [M][LD_OUT] fp16, GN_PART [B][S / 32][32][2] fp32 (GN = 1).  Head
 * outputs: HTOK [M][LD_TOK], QK [M][LD_QK] (q | k), HVT [B][C][LD_VT] at stride S_VT (fp16). */
enum tsd_chain_operand {
  TSD_CO_AO = 0, TSD_CO_TOK, TSD_CO_X, TSD_CO_KC, TSD_CO_VT, TSD_CO_WSO, TSD_CO_WQ, TSD_CO_WCO, TSD_CO_W1, TSD_CO_W2, TSD_CO_WOUT,
  TSD_CO_BSO, TSD_CO_BCO, TSD_CO_B1, TSD_CO_B2, TSD_CO_BOUT, TSD_CO_GN_STATS, TSD_CO_WC, TSD_CO_WIN, TSD_CO_B_IN,
  TSD_CO_OUT, TSD_CO_GN_PART, TSD_CO_HTOK, TSD_CO_QK, TSD_CO_HVT, TSD_CO_COUNT
};
/* info: guard / pitch-gap elements the launches changed; 1 when the fused kernel was launched (0: the packer or the launcher refused). */
enum tsd_chain_info { TSD_CI_CHANGED = 0, TSD_CI_RAN, TSD_CI_COUNT };
/* Run the launch described by desc (n >= TSD_CD_COUNT fields) on caller operands (host_in[TSD_CO_AO .. TSD_CO_B_IN], NULL for unused
 * slots) through launch_attn_tail / launch_attn_head and return its outputs (host_out[slot - TSD_CO_OUT]).  host_in == NULL only sizes
 * (ctx may be NULL, no device is touched): ext[TSD_CO_COUNT] receives every slot's extent (0 = unused).  A descriptor that cannot be
 * sized is refused before any launch; what the launchers refuse (S % 64, T outside 1 .. 80, pitches below 320 or no multiple of 8, LDVT
 * < round_up(T, 8), LD_VT < S, C / D / HEADS other than 320 / 40 / 8, the fused path switched off by tsd_debug_set_fused_attention) is
 * sized and left to them.  Every operand sits between 4 KiB guard bands of a NaN pattern and the outputs are pre-filled with it; they are
 * returned even when the launch is refused (its status is the return value). */
int tsd_debug_chain_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out, int64_t* ext,
                        int64_t* info);
/* ---- elementwise / layout / packing launch descriptors (test infrastructure: tests/elem_ref.py holds the time path, the activations,
 * the boundary conversions and the packers of csrc/kernels_elementwise.hip to an fp64 reference, element-wise) ----
 * One descriptor is one launch of the launch_* function its MODE names; the other fields are that function's arguments (unused ones 0).
 * Pitches in elements, SCALE and T_BITS the bits of a float.  Per mode (X, W, BIAS: inputs; Y: output):
 *   SMALL_LINEAR      launch_small_linear: X fp32 [B][LDX], W fp16 [N][LDW], BIAS fp32 [N] (HAS_BIAS) -> Y fp32 [B][LDY]; K, SILU
 *   TIME_EMBEDDING    launch_time_embedding: X fp32 [B] (HAS_T; else the scalar T_BITS for every row) -> Y fp32 [B][320]
 *   GEGLU_ERF         launch_geglu_erf_f16: X fp16 [ROWS][2 COLS] ((a, gate) interleaved) -> Y fp16 [ROWS][COLS]
 *   QUICK_GELU        launch_quick_gelu_f16: X fp16 [N], in place (Y starts as X)
 *   UNARY             launch_unary_f32: OP 0 silu, 1 gelu-tanh, 2 to-pixel; X fp32 [N] -> Y fp32 [N]
 *   CLIP_EMBED        launch_clip_embed: X int32 tokens [B T], W fp16 table [V][D], BIAS fp32 positions [T][D] -> Y fp16 [B T][D]
 *   CHW_TO_NHWC       launch_chw_f32_to_nhwc_f16: X fp32 [B][C][H W] -> Y fp16 [B H W][CDST]; CUSE, SCALE
 *   IM2COL3X3         launch_chw_f32_to_im2col3x3_f16: X fp32 [B][C][H W] -> Y fp16 [B H W][64]; SCALE
 *   NHWC_TO_CHW       launch_nhwc_f16_to_chw_f32 (DTYPE 1) / launch_nhwc_f32_to_chw_f32 (DTYPE 0): X [B H W][LD] -> Y fp32 [B][C][H W]
 *   F32_TO_F16_ROWS   launch_f32_to_f16_rows: X fp32 [ROWS][COLS] -> Y fp16 [ROWS_DST][LD], zero padded
 *   F16_TO_F32_ROWS   launch_f16_to_f32_rows: X fp16 [ROWS][LD] -> Y fp32 [ROWS][COLS]
 *   TRANSPOSE_TO_F16  launch_transpose_f32_to_f16: X fp32 [B][K][N] -> Y fp16 [B][NPAD][KPAD]
 *   PACK_CONV         launch_pack_conv: X fp32 [O][I][KSIZE][KSIZE] -> Y fp16 [OPAD][KSIZE KSIZE][IPAD]
 *   PACK_LINEAR       launch_pack_linear: X fp32 [N][K] -> Y fp16 [N][KPAD]; INTERLEAVE
 *   PACK_BIAS         launch_pack_bias: X fp32 [N] -> Y fp32 [NPAD]; INTERLEAVE
 *   PACK_IM2COL_W     launch_pack_im2col_w: X fp16 [O][9][IPAD] -> Y fp16 [O][64]; C
 *   ENCODER_SAMPLE    launch_encoder_sample: X fp32 moments [B][HW][LD], W fp32 noise [B][4][HW] -> Y fp32 [B][4][HW] */
enum tsd_elem_desc_field {
  TSD_ED_VERSION = 0, TSD_ED_MODE, TSD_ED_B, TSD_ED_K, TSD_ED_N, TSD_ED_LDX, TSD_ED_LDW, TSD_ED_LDY, TSD_ED_SILU, TSD_ED_HAS_BIAS,
  TSD_ED_HAS_T, TSD_ED_T_BITS, TSD_ED_ROWS, TSD_ED_COLS, TSD_ED_OP, TSD_ED_T, TSD_ED_V, TSD_ED_D,
  TSD_ED_C, TSD_ED_H, TSD_ED_W, TSD_ED_HW, TSD_ED_CUSE, TSD_ED_CDST, TSD_ED_SCALE, TSD_ED_DTYPE, TSD_ED_LD, TSD_ED_ROWS_DST,
  TSD_ED_KPAD, TSD_ED_NPAD, TSD_ED_O, TSD_ED_I, TSD_ED_KSIZE, TSD_ED_OPAD, TSD_ED_IPAD, TSD_ED_INTERLEAVE,
  TSD_ED_COUNT
};
#define TSD_ED_VERSION_1 1
enum tsd_elem_mode {
  TSD_EM_SMALL_LINEAR = 0, TSD_EM_TIME_EMBEDDING, TSD_EM_GEGLU_ERF, TSD_EM_QUICK_GELU, TSD_EM_UNARY, TSD_EM_CLIP_EMBED,
  TSD_EM_CHW_TO_NHWC, TSD_EM_IM2COL3X3, TSD_EM_NHWC_TO_CHW, TSD_EM_F32_TO_F16_ROWS, TSD_EM_F16_TO_F32_ROWS, TSD_EM_TRANSPOSE_TO_F16,
  TSD_EM_PACK_CONV, TSD_EM_PACK_LINEAR, TSD_EM_PACK_BIAS, TSD_EM_PACK_IM2COL_W, TSD_EM_ENCODER_SAMPLE, TSD_EM_COUNT
};
/* Operand slots: inputs X, W, BIAS; output Y.  Elements are 2 or 4 bytes as the mode states (token ids: int32 in a 4-byte slot). */
enum tsd_elem_operand { TSD_EO_X = 0, TSD_EO_W, TSD_EO_BIAS, TSD_EO_Y, TSD_EO_COUNT };
/* info: guard / pitch-gap elements the launch changed; the change of the context's non-finite count across the launch (the count is
 * cleared afterwards, as tsd_debug_nonfinite_count(ctx, 1) does); SMALL_LINEAR: the k_small_linear<NB> instance that ran and its K
 * passes (0 when the launch was refused). */
enum tsd_elem_info { TSD_EI_CHANGED = 0, TSD_EI_NONFINITE, TSD_EI_NB, TSD_EI_PASSES, TSD_EI_COUNT };
/* Run the launch described by desc (n >= TSD_ED_COUNT fields) on caller operands in their device layout (host_in[TSD_EO_X .. TSD_EO_BIAS],
 * NULL for unused slots) and return its output (host_out[0]).  host_in == NULL only sizes (ctx may be NULL, no device is touched):
 * ext[TSD_EO_COUNT] receives every slot's extent (0 = unused).  A descriptor that cannot be sized is refused before any launch; what the
 * launchers refuse (B > 16, K % 8, misaligned pitches, B K beyond the LDS, widths that are no multiple of their vector) is sized and left
 * to them.  Every operand sits between 4 KiB guard bands of a NaN pattern and Y is pre-filled with it (QUICK_GELU: with X); the output is
 * returned even when the launch is refused (its status is the return value). */
int tsd_debug_elem_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out, int64_t* ext,
                       int64_t* info);
/* GroupNorm launches enqueued on this context since the last reset, per statistics path: counts[0] all, [1] own statistics pass,
 * [2] one producer table finished inside the apply blocks, [3] one producer table finished by the k_gn_finalize launch,
 * [4] k_gn_prereduce, [5] composite accepted, [6] k_gn_finalize launches (any source), [7] composites offered.  n >= 8; reset != 0
 * clears them. */
int tsd_debug_gn_path_counts(tsd_ctx* ctx, int64_t* counts, int n, int reset);
/* The -DTSD_JITTER build (`make jitter`: random wave-level delays where waves meet) shows that it detects a hazard: n (1 .. 64) launches
 * of a two-wave kernel in which wave 0 reads an LDS word that wave 1 writes, with a jitter point in each wave and no barrier between
 * the two accesses (csrc/kernels_elementwise.hip, k_jitter_selftest: in bounds, nothing waits).  Returns the number of DISTINCT words the
 * launches stored - 2 when both orders occurred, 1 on a build that keeps one schedule.  The shipped library has no such kernel: there
 * the entry launches nothing and returns TSD_E_ARG ("not supported in this build"), like a tile configuration the build does not have. */
int tsd_debug_jitter_selftest(tsd_ctx* ctx, int n);
/* Attention blocks that run op by op (C = 640 / 1280) fold GEGLU's second linear into the output 1x1 convolution at tsd_model_prepare:
 * wf [C][5C] fp16 = [W_out . W_2 | W_out], bf [C] = W_out . b_2 + b_out.  Copies block `block`'s (index into the UNet's layers; NULL
 * pointers only ask) and returns C, 0 when that block does not fold.  tsd_model_prepare returns TSD_E_NONFINITE when a folded weight
 * leaves fp16. */
int tsd_debug_model_fold(tsd_model* m, int block, void* wf, float* bf);
/* UNet layer 10 reads the channel concat of ONE tensor with itself (diffusion.mojo:253-256).  With TSD_FOLD_DUP (default 1, read by
 * tsd_ctx_create) tsd_model_prepare adds the two input-channel halves of its conv1 and 1x1 skip weights - exact sum, one rounding to
 * fp16, nearest-even - and the block runs as cin/2 -> cout with GroupNorm(groups/2).  tsd_debug_model_dup_fold copies the folded conv1
 * [Opad][9][cin/2] and skip [Opad][cin/2] fp16 weights (NULL pointers only ask) and returns cin/2, 0 when the model does not fold;
 * tsd_model_prepare returns TSD_E_NONFINITE when a sum leaves fp16.  tsd_debug_dup_fold_host is that arithmetic on host memory (no
 * device needed): out[r][t][c] = w[r][t][c] + w[r][t][half + c] for c < half, 0 for half <= c < ldo, on fp16 bit patterns
 * w [rows][taps][ldw], out [rows][taps][ldo]; returns the number of sums that are not finite, < 0 on a bad argument. */
int tsd_debug_model_dup_fold(tsd_model* m, void* conv1_w, void* skip_w);
int64_t tsd_debug_dup_fold_host(const void* w, int rows, int taps, int ldw, int half, void* out, int ldo);
/* The residual blocks behind a nearest-2x upsample (layers 15 and 20 of the 23-layer UNet) run conv1 over the upsampled grid.  Its nine
 * taps read 2 x 2 source pixels per output pixel, so tsd_model_prepare sums the taps that share one: four 2x2 kernels, one per output
 * parity q = 2 py + px, rows {0},{1,2} for parity 0 and {0,1},{2} for parity 1, columns alike - exact sum, one rounding to fp16,
 * nearest-even - and with TSD_UPS_FOLD (default 1; tsd_debug_set_ups_fold returns the previous value) the launch executes K = 4 Cin on
 * them where the source plane is a multiple of 256 pixels (TSD_GD_UPS = 2 in its descriptor, which still states the 3x3 problem).
 * tsd_debug_ups_fold_host is the arithmetic on host memory (no device needed): fp16 bit patterns w [O][3][3][Ipad] with row pitch
 * ldw >= 9 Ipad -> out [4][O][2][2][Ipad]; returns the number of sums that are not finite, < 0 on a bad argument.
 * tsd_debug_model_ups_fold copies the device copy of residual block `block` (index into the UNet's layers; NULL only asks): per parity
 * that matrix K-tile-major, [4 Ipad / 64][Opad][64]; returns Ipad, 0 when the block does not fold.  tsd_model_prepare returns
 * TSD_E_NONFINITE when a sum leaves fp16. */
int64_t tsd_debug_ups_fold_host(const void* w, int O, int Ipad, int ldw, void* out);
int tsd_debug_model_ups_fold(tsd_model* m, int block, void* out);
int tsd_debug_set_ups_fold(tsd_ctx* ctx, int on);
/* Raw packed bytes of parameter `index` (the device layout: fp16 [N][Kpad] / [Opad][k*k][Ipad], fp32 biases).  out == NULL asks for
 * the size; returns the byte count (0 for a parameter the forward never reads), TSD_E_ARG when cap is too small. */
int tsd_debug_model_packed_param(tsd_model* m, int index, void* out, size_t cap);
/* tsd_debug_gemm_bench for the fused attention core: Q,K [B][S][H*d], V^T [B][H*d][Sk]. */
int tsd_debug_attn_bench(tsd_ctx* ctx, int B, int H, int d, int Sq, int Sk, int iters, float* ms);
/* The fused attention core runs an optimistic softmax pass (reference fixed after the first key tile) and repeats a
 * workgroup exactly when one of its rows overflowed fp16: number of workgroups that repeated since the last reset
 * (reset != 0 clears the counter); < 0 on error.  Synchronises the context's stream. */
int tsd_debug_attn_exact_passes(tsd_ctx* ctx, int reset);
/* Kernel of the d = 40 attention core: 0 = chosen by shape (default), 1 = 32 queries per wave, 2 = 64 (4-wave workgroups),
 * 3 = the 8-wave two-group kernel (64 queries per wave, 512 per workgroup).
 * All compute every row with the same instruction sequence: bitwise equal results as long as no workgroup takes the exact
 * repeat (there the repeat and the reference moves are decided per workgroup / per wave, i.e. over different row sets).  The
 * default choice depends on the layer shape only, never on the batch.  Returns the previous mode. */
int tsd_debug_set_attn_qb(tsd_ctx* ctx, int mode);
/* Self-attention (Sq == Sk): the optimistic softmax reference is max(row maximum of key tile 0, row maximum over the query's
 * own 32-key block) + headroom; on = 0 restores the tile-0-only reference (to measure what the second reference saves on
 * peaked score distributions).  Returns the previous setting. */
int tsd_debug_set_attn_diag(tsd_ctx* ctx, int on);
/* Residual blocks whose skip path is a 1x1 convolution at the block's own resolution (diffusion.mojo:70-72, vae.mojo:65-67) run it
 * inside the second 3x3 convolution as extra K (on = 1, default); on = 0 runs it as its own GEMM + residual add (the round-2 path,
 * kept for A/B and for the equivalence test).  Returns the previous setting. */
int tsd_debug_set_res_fuse_skip(tsd_ctx* ctx, int on);
/* Self-attention input projection (helpers/attention.mojo:29-31): q | k (token-major) and V^T (channel-major, what the attention
 * kernel reads) come from ONE GEMM over in_proj's 3C rows whose tiles beyond column 2C store transposed (on = 1, default; needs
 * H*W % 32 == 0); on = 0 runs the q/k GEMM and the swapped-operand V^T GEMM as two launches.  Environment: TSD_QKV_FUSE.  Returns
 * the previous setting. */
int tsd_debug_set_qkv_fuse(tsd_ctx* ctx, int on);
/* A denoise session computes what a step's UNet forward derives from the timestep and the context alone - the time MLP and the time
 * projections of every schedule entry, the context K / V^T of all attention blocks - once per tsd_session_upload, with the launches
 * the step would make, and its steps read them (on = 1, default): five launches per step fewer, the same bits.  A parameter set
 * after upload() makes the next step rebuild them.  on = 0: every step computes them again.  Like every tsd_debug_set_* call a
 * change asks the context's sessions for a new upload().  Environment: TSD_SESSION_HOIST.  Returns the previous setting. */
int tsd_debug_set_session_hoist(tsd_ctx* ctx, int on);
/* TSD_CONTROL_STATS (default 1): 0 makes the ControlNet injection discard the statistics of the tensors it rewrites, so every consumer
 * runs its own statistics pass - the A/B of the statistics hand-over.  Returns the previous value. */
int tsd_debug_set_control_stats(tsd_ctx* ctx, int on);
/* info[6] of a session: [0] 1 when the steps of the current upload() read the hoisted buffers, [1] device address of the time table,
 * [2] of the context K and [3] V^T buffers, [4] bytes allocated for them, [5] times they have been built (uploads + rebuilds). */
int tsd_debug_session_hoist_info(tsd_session* s, int64_t* info);
/* What this board sustains on the matrix pipe: a register-resident dense fp16 MFMA loop (no LDS, no memory) run for about
 * `ms_target` ms at 4 waves per SIMD; reports the achieved TFLOP/s and the shader clock (GHz) during the run.  The nominal
 * dense peak assumes the boost clock; under matrix-pipe load the board's power limit sets the clock. */
int tsd_debug_mfma_sustained(tsd_ctx* ctx, float ms_target, float* tflops, float* clock_ghz);
/* The ledger of device resources: what the library as a whole - every context, model and session of the process - holds on the device
 * now, and what it has ever allocated and released.  Every device allocation, event and stream the library makes or releases is recorded
 * as the runtime reports it; the ledger only counts and never changes what a call does.  LIVE fields go up and down; the others are
 * monotone.  ALLOCS_LIVE == ALLOCS_TOTAL - FREES_TOTAL.  FREES_UNKNOWN counts releases of a pointer, event or stream the ledger does not
 * hold (a double or a foreign release), RELEASE_ERRORS releases the runtime refused: both must stay 0.  A step of a session that keeps
 * its "no allocation" promise leaves ALLOCS_TOTAL and FREES_TOTAL where they were.  What RCCL allocates for a communicator is its own
 * and is not counted.  Writes the first min(n, TSD_DL_COUNT) fields to out and returns TSD_DL_COUNT; TSD_E_ARG for a NULL out or n < 0.
 * Needs no device; safe from any thread. */
enum tsd_device_ledger_field {
  TSD_DL_ALLOCS_LIVE = 0, TSD_DL_BYTES_LIVE, TSD_DL_EVENTS_LIVE, TSD_DL_STREAMS_LIVE, TSD_DL_CTX_LIVE, TSD_DL_MODELS_LIVE,
  TSD_DL_SESSIONS_LIVE, TSD_DL_ALLOCS_TOTAL, TSD_DL_FREES_TOTAL, TSD_DL_FREES_UNKNOWN, TSD_DL_RELEASE_ERRORS, TSD_DL_COUNT
};
/* debug */ int tsd_debug_device_ledger(int64_t* out, int n);

/* ---- FreeU (EXTENSION: Si et al. 2023, "FreeU: Free Lunch in Diffusion U-Net"; diffusers' `enable_freeu`) on the full-size UNets
 * (kinds 5 / 6 / 16).  In front of every decoder concat the two inputs are re-weighted in place: the backbone half of the hidden tensor
 * is scaled up, the lowest spatial frequencies of the popped skip are scaled down.  No weights, no training.
 * Number the decoder residual blocks j = 0 .. 11 in pop order (flat layers 22, 23, 24, 26, 28, 30, 33, 35, 37, 40, 42, 44 of the step
 * tables); block j sees the hidden tensor h [B][H*W][Ch] and the popped skip r [B][H*W][Cr], fp16 NHWC, and a table gives it (b_j, s_j).
 *   skip (s_j != 1; otherwise r is neither read nor written): diffusers' fourier_filter(r, threshold = 1, scale = s_j) - the four bins
 *     (fy, fx) in {0, -1}^2 of each (sample, channel) plane's 2-D DFT times s_j - evaluated without a transform: with
 *     cy[y] = cos(2 pi y / H), sy[y] = sin(2 pi y / H), cx / sx likewise over W, cxy = cy cx - sy sx, sxy = sy cx + cy sx,
 *       S0 = sum r, Ay = sum r cy, By = sum r sy, Ax = sum r cx, Bx = sum r sx, Axy = sum r cxy, Bxy = sum r sxy   (over the plane)
 *       P = (S0 + Ay cy + By sy + Ax cx + Bx sx + Axy cxy + Bxy sxy) / (H W),   r' = rn16(r + (s_j - 1) P)
 *     fp32 sums in a fixed order, one rounding to fp16; the four tables are built on the host in double, rounded once to fp32 and kept on
 *     the context per (H, W) (released with it).
 *   hidden (b_j != 1; otherwise h is neither read nor written), channels c < Ch / 2 only - the other half is never written:
 *     TSD_FREEU_CONSTANT (diffusers): h' = rn16(b_j h).
 *     TSD_FREEU_MODULATED (the "v2" form of the authors' repository): m[p] = (1 / Ch) sum_c h[p][c] over all Ch channels, lo / hi its
 *     per-sample minimum / maximum over the pixels, n[p] = (m[p] - lo) / (hi - lo), h' = rn16(((b_j - 1) n[p] + 1) h).  Where hi == lo,
 *     n = 0 (h stays as it is): the published code divides by zero there - a deliberate deviation.
 * One launch per decoder block with an active entry, one more in the modulated mode; no atomics, no synchronisation; a sample's bits do
 * not depend on B or on its batch position.  A ControlNet's injection runs before FreeU, as in diffusers.  The GroupNorm statistics the
 * producers of a rewritten tensor emitted are dropped: the block's first GroupNorm runs its own statistics pass.
 * FreeU is state of the UNet MODEL: tsd_diffusion_forward_hw, _control_hw, _ip_hw, sessions and slot sessions of the model all run it.
 * tsd_model_set_freeu: b, s fp32 [TSD_FREEU_BLOCKS]; both NULL turns it off, and so does a table of all ones: an off model enqueues
 * exactly the launches it did before and gives the bits it gave.  It takes effect on the next forward, also the next step() / advance()
 * of an open session, which needs no upload(): the workspace a forward needs does not depend on the table.  TSD_E_ARG: a kind other
 * than 5 / 6 / 16 (Tiny-SD, ControlNets, adapters, encoders), a non-finite b or s, an unknown mode, exactly one of b, s NULL; the
 * model's table stays as it was.
 * tsd_model_freeu: 1 when a table is active, 0 when off (negative: TSD_E_ARG, a NULL model or a wrong kind); b, s ([12]) and mode are
 * filled when not NULL - ones and TSD_FREEU_CONSTANT when off.
 * tsd_freeu_f16: the launch alone on host fp16 tensors, synchronous: h [B][H][W][Ch], r [B][H][W][Cr] -> h_out, r_out (either pair may be
 * NULL together: that tensor is skipped).  1 <= B <= 64, H, W >= 2, Ch a multiple of 16, Cr of 8 (TSD_E_SHAPE). */
#define TSD_FREEU_BLOCKS 12
enum { TSD_FREEU_CONSTANT = 0, TSD_FREEU_MODULATED = 1 };
int tsd_model_set_freeu(tsd_model* unet, const float* b, const float* s, int mode);
int tsd_model_freeu(tsd_model* unet, float* b, float* s, int* mode);
int tsd_freeu_f16(tsd_ctx* ctx, const void* h, const void* r, int B, int H, int W, int Ch, int Cr, float b, float s, int mode, void* h_out,
                  void* r_out);
/* The same launch on operands with pitches and guard bands (test infrastructure: tests/test_gpu_freeu.py).  h / r: host fp16 buffers of
 * guard + B * H * W * ld + guard elements (ldh >= Ch, ldr >= Cr, pitches and guard multiples of 8, guard >= 0); the launch is given the
 * address behind the leading guard.  h_out / r_out receive the WHOLE buffers back, guards and pitch gaps included: what the launch may
 * write is columns < Ch / 2 of h and < Cr of r, nothing else. */
int tsd_debug_freeu_run(tsd_ctx* ctx, const void* h, const void* r, int B, int H, int W, int Ch, int Cr, int ldh, int ldr, int guard, float b,
                        float s, int mode, void* h_out, void* r_out);

/* ---- census -------------------------------------------------------------------------- */
/* Algorithmic GFLOP (2*MAC of conv + linear + attention core) of one forward per sample
 * (SURVEY.md Appendix B): kind, latent side L, context tokens T. */
double tsd_flop_count(int kind, int L, int T);

#ifdef __cplusplus
}
#endif
#endif /* TSD_H */
