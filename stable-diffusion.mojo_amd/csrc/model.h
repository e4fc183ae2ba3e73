// model.h - parameter inventory, packed device weights and resolved weight trees.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"

enum ParamKind { P_CONV_W = 0, P_CONV_B = 1, P_LIN_W = 2, P_LIN_B = 3 };

struct ParamSpec {
  std::string name;
  int64_t shape[4] = {0, 0, 0, 0};
  int ndim = 0;
  int kind = 0;
  bool used = true;
  float bound = 0.f;  // synthetic-init bound (0 -> zeros)
  float offset = 0.f; // synthetic init = offset + U(+-bound) (norm weights: 1 + ...)
  // packing
  int Opad = 0, Kpad = 0;  // conv: Opad rows, Kpad = Ipad ; linear: Kpad
  int interleave = 0;      // GEGLU (a,g) row interleave (diffusion.mojo:138-141)
  int region = 0;          // 0 normal; dense contiguous tables: 1 time-proj weights, 2 time-proj biases, 3 k_proj, 4 v_proj
  size_t off = 0, bytes = 0;
  int64_t numel() const {
    int64_t n = 1;
    for (int i = 0; i < ndim; i++) n *= shape[i];
    return n;
  }
  // P_LIN_W as the packer sees it: [rows][cols]; a 3-d entry is [1][rows][cols] (the resampler's `latents`)
  int rows() const { return (int)shape[ndim == 3 ? 1 : 0]; }
  int cols() const { return (int)shape[ndim == 3 ? 2 : 1]; }
};

// layer tables (diffusion.mojo:177-201, vae.mojo:94-112,194-219)
enum LayerKind { L_CONV, L_CONV_S2, L_RES, L_ATTN, L_UP, L_GN, L_SILU, L_UPCONV };
struct LayerDef { int kind; int a, b, c, d; };
extern const LayerDef UNET_LAYERS[23];
extern const LayerDef DECODER_LAYERS[26];
extern const LayerDef ENCODER_LAYERS[19];
// full-size UNet (TSD_MODEL_DIFFUSION_SD15): flat layer list with the skip-connection plumbing of each step
enum { U_POP = 1, U_PUSH = 2 };  // input = concat(x, popped skip) ; output pushed as a skip
struct UNetStep { LayerDef l; int flags; };
constexpr int SD15_N = 45;
extern const UNetStep SD15_STEPS[SD15_N];
// SD-2.x UNet (TSD_MODEL_DIFFUSION_SD2): SD15_STEPS with every attention block {L_ATTN, C / 64, 64} - the same kinds, widths and flags
extern const UNetStep SD2_STEPS[SD15_N];
static inline bool is_sd2_unet_kind(int kind) { return kind == TSD_MODEL_DIFFUSION_SD2; }
static inline const UNetStep* full_unet_steps(int kind) { return is_sd2_unet_kind(kind) ? SD2_STEPS : SD15_STEPS; }
static inline bool is_full_unet_kind(int kind) {
  return kind == TSD_MODEL_DIFFUSION_SD15 || kind == TSD_MODEL_DIFFUSION_SD15_TORCH || kind == TSD_MODEL_DIFFUSION_SD2;
}
static inline bool is_diffusion_kind(int kind) { return kind == TSD_MODEL_DIFFUSION || is_full_unet_kind(kind); }
static inline bool is_clip_kind(int kind) { return kind == TSD_MODEL_CLIP || kind == TSD_MODEL_CLIP_TORCH || kind == TSD_MODEL_CLIP_SD2; }
static inline bool is_torch_clip_kind(int kind) { return kind == TSD_MODEL_CLIP_TORCH || kind == TSD_MODEL_CLIP_SD2; }
static inline bool is_decoder_kind(int kind) { return kind == TSD_MODEL_DECODER || kind == TSD_MODEL_DECODER_TORCH; }
static inline bool is_encoder_kind(int kind) { return kind == TSD_MODEL_ENCODER || kind == TSD_MODEL_ENCODER_TORCH; }
static inline bool is_vae_torch_kind(int kind) { return kind == TSD_MODEL_DECODER_TORCH || kind == TSD_MODEL_ENCODER_TORCH; }
// ControlNet of the full-size UNet (kinds 10 / 11): SD15_STEPS[0, SD15_ENC_N) - the encoder and the bottleneck - on weights of its own, a
// hint encoder in front and one 1x1 "zero" convolution per pushed skip and for the bottleneck output (graph.cpp g_controlnet_forward)
constexpr int SD15_ENC_N = 21;  // the first U_POP step: 18 encoder steps (12 of them push) and the three of the bottleneck
constexpr int CN_HINT_N = 8;
struct HintConvDef { int cin, cout, stride; };
extern const HintConvDef CN_HINT_CONVS[CN_HINT_N];
static inline bool is_controlnet_kind(int kind) { return kind == TSD_MODEL_CONTROLNET_SD15 || kind == TSD_MODEL_CONTROLNET_SD15_TORCH; }
static inline bool is_torch_unet_kind(int kind) {
  return kind == TSD_MODEL_DIFFUSION_SD15_TORCH || kind == TSD_MODEL_CONTROLNET_SD15_TORCH || kind == TSD_MODEL_DIFFUSION_SD2;
}
// IP-Adapter of the SD-1.x full-size UNet (kind 20): the image projection and one to_k_ip / to_v_ip pair per cross-attention block of
// SD15_STEPS, in the table's order; no graph of its own - the UNet's forward reads its projected keys / values (graph.h IpKV)
constexpr int IP_SD15_TOKENS = 4, IP_EMBED_DIM = 1024, IP_CTX_DIM = 768;
// IP-Adapter Plus (kind 24): the same 16 pairs behind a Perceiver resampler - 16 learned queries read the CLIP vision encoder's
// hidden_states[-2] ([S][1280], S = 257 in use) through 4 layers of cross attention (12 heads of 64) and a 768 -> 3072 -> 768
// feed-forward (graph.cpp g_ip_resample); the UNet side is kind 20's at N = 16
constexpr int IPP_TOKENS = 16, IPP_DEPTH = 4, IPP_HEADS = 12, IPP_DHEAD = 64, IPP_EMBED = 1280, IPP_FF = 3072, IPP_MAX_S = 1024;
static inline bool is_ip_plus_kind(int kind) { return kind == TSD_MODEL_IP_ADAPTER_PLUS_SD15; }
static inline bool is_ip_adapter_kind(int kind) { return kind == TSD_MODEL_IP_ADAPTER_SD15 || is_ip_plus_kind(kind); }
// `ip_adapter.<index>` of the published files for the t-th cross-attention block of SD15_STEPS (6 down, 1 mid, 9 up): the files count
// diffusers' attention processors - down blocks, then up blocks, then the mid block - and the cross-attention ones are the odd numbers
static inline int ip_adapter_published_index(int t) { return t < 6 ? 2 * t + 1 : (t == 6 ? 31 : 2 * t - 1); }
// CLIP vision encoder (kind 22): OpenCLIP ViT-H/14 as the `image_encoder/` folder of the IP-Adapter files holds it (graph.cpp g_clip_vision_forward)
constexpr int CV_WIDTH = 1280, CV_HEADS = 16, CV_LAYERS = 32, CV_MLP = 5120, CV_TOKENS = 257, CV_EMBED = 1024;
static inline bool is_clip_vision_kind(int kind) { return kind == TSD_MODEL_CLIP_VISION_H; }
// 1 .. 11, 16, 17, 20, 22 and 24; 12 .. 15, 18, 19, 21 and 23 are reserved and refused
static inline bool is_model_kind(int kind) {
  return (kind >= TSD_MODEL_DIFFUSION && kind <= TSD_MODEL_CONTROLNET_SD15_TORCH) || kind == TSD_MODEL_DIFFUSION_SD2 || kind == TSD_MODEL_CLIP_SD2 ||
         is_ip_adapter_kind(kind) || kind == TSD_MODEL_CLIP_VISION_H;
}

std::vector<ParamSpec> build_param_specs(int model_kind);

struct ResW {
  ConvW conv1, conv2, skip;
  LinW time;       // UNet only (kept for the op-level path; the model path uses the concatenated table)
  int cin = 0, cout = 0, groups = 32;
  int groups_in = 0;  // groups of the FIRST GroupNorm when they differ from `groups` (0: the same) - the folded duplicate-concat block only
  bool has_skip = false;
  int time_off = 0;  // column offset into the concatenated time projection [B][6720]
  NormAffine gn1, gn2;  // torch-norm extension (kind 6): per-channel affine of the two GroupNorms (w == nullptr: reference)
  float eps = 1e-5f;    // GroupNorm epsilon (helpers/utils.mojo:1821-1826 default); 1e-6 in a trained VAE (kinds 8, 9)
};
struct AttnW {  // Unet_Attention_Block, diffusion.mojo:87-98
  int n_head = 0, n_embed = 0, C = 0, d_ctx = 768;
  ConvW conv_in, conv_out;
  LinW sa_in, sa_out, ca_q, ca_k, ca_v, ca_out, geglu1, geglu2;
  int kv_off = 0;  // row offset of this block in the concatenated k_proj / v_proj tables
  NormAffine gn, ln[3];  // torch-norm extension (kind 6)
  bool gelu_erf = false; // kind 6: exact GELU in the GEGLU gate (torch.nn.functional.gelu)
  // derived: the six tail matrices re-packed as the tile stream of the fused tail kernel (kernels_chain.hip); nullptr when
  // the block is not eligible or the model's parameters changed since the last model_check_ready()
  const half_t* tail_stream = nullptr;
  const half_t* head_stream = nullptr;  // same for conv_in + in_proj (fused head kernel)
  // derived, blocks that run op by op (C = 640 / 1280): `conv_out(geglu2(h) + r) + x` (diffusion.mojo:143-146) is linear in [h | r], so the two
  // GEMMs run as ONE over the channel concat with folded weights [C][4C + C] (row-major and K-tile-major) and bias conv_out.w . geglu2.b + conv_out.b
  const half_t* fold_w = nullptr; const half_t* fold_w_tm = nullptr; const float* fold_b = nullptr;
};
// true when the fused tail kernel can run this block's weights (reference norms, tanh GELU, C = 8 x 40)
bool attn_tail_weights_ok(const AttnW& w);
bool attn_head_weights_ok(const AttnW& w);
struct VaeAttnW {  // vae.mojo:9-11
  int C = 0;
  LinW in_proj, out_proj;
  NormAffine gn;  // torch-norm extension (kinds 8, 9)
  float eps = 1e-5f;
};

struct UNetW {
  LinW t1, t2;       // Time_Embedding
  LinW tproj;        // concatenated layer3 of the 9 residual blocks: [6720][1280]
  LinW kproj_all, vproj_all;  // concatenated cross-attention k_proj / v_proj of the 9 attention blocks: [6720][768]
  ConvW conv1, conv4, conv7, final_conv;
  // derived: the input convolution's weights as a [Opad][64] matrix over K = (tap, cin) for cin < 8 (model_check_ready): the 4-channel
  // latent is gathered to im2col rows at the boundary and the convolution runs as ONE 64-deep K tile instead of nine padded taps
  const half_t* conv_in_im2col = nullptr;
  std::vector<ResW> res;    // indexed by flat layer position (23 entries, or SD15_N)
  std::vector<AttnW> attn;
  std::vector<ConvW> conv;  // full-size UNet only: input, downsample and upsample convolutions
  // derived (TSD_FOLD_DUP): layer 10 reads concat(x, x) of ONE tensor (diffusion.mojo:253-256), so GroupNorm(32) over [x | x] is
  // [g | g] with g = GroupNorm(16)(x) and conv1 / the 1x1 skip over the concat are convolutions of the single tensor with the two
  // input-channel halves of their weights added (exact sum, one rounding to fp16): an ordinary cin/2 -> cout block.  res_dup shares
  // everything else with res[9]; res_dup_on is false when the block does not qualify or the parameters changed since
  // model_check_ready().  Decided from the graph's structure, never from the data.
  ResW res_dup;
  bool res_dup_on = false;
  // ControlNet kinds only: the hint encoder, the zero convolutions in push order and the one of the bottleneck output
  ConvW hint[CN_HINT_N];
  std::vector<ConvW> zero;
  ConvW zero_mid;
  NormAffine final_gn;      // torch-norm extension (kind 6)
  int final_groups = 320;   // UNet_Output_Layer's GroupNorm (diffusion.mojo:287-291); 32 with torch norms
};
struct VaeW {
  std::vector<ConvW> conv;      // indexed by layer (1-based position - 1)
  const half_t* conv_in_im2col = nullptr;  // derived: the first convolution (3 or 4 input channels) as [Opad][64] im2col weights
  std::vector<ResW> res;
  std::vector<VaeAttnW> attn;
  std::vector<NormAffine> gn;   // stand-alone GroupNorm layers (torch-norm extension)
  float gn_eps = 1e-5f;         // their epsilon (1e-6 in a trained VAE)
};

struct ClipLayerW { LinW in_proj, out_proj, l4, l5; NormAffine ln1, ln2; };  // ClipPlayer clip.mojo:23-34 (its LayerNorms have no parameters)
constexpr int CLIP_MAX_LAYERS = 23;
struct ClipW {
  int D = 768, H = 12, n_layer = 12;  // width, heads (of 64) and layers: 1024 / 16 / 23 for TSD_MODEL_CLIP_SD2
  bool gelu_erf = false;              // the MLP's activation: quick-GELU (clip.mojo:49-50), or torch's exact GELU (OpenCLIP)
  const half_t* tok = nullptr;  // [49408][D] fp16
  const float* pos = nullptr;   // [77][D] fp32
  ClipLayerW layer[CLIP_MAX_LAYERS];
  NormAffine final_ln;  // torch-norm extension (kind 7)
};

struct IpResampleLayerW { NormAffine norm1, norm2, ff_norm; LinW to_q, to_kv, to_out, ff1, ff2; };  // no biases
struct IpAdapterW {  // kinds 20 / 24
  int n_tokens = IP_SD15_TOKENS;  // 4; 16 for kind 24
  LinW proj;        // image_proj.proj: [n_tokens * 768][1024], with bias (kind 20 only)
  NormAffine norm;  // image_proj.norm: LayerNorm(768) weight / bias, torch semantics (kind 20 only)
  // kind 24 only: the resampler.  latents [16][768] fp16, proj_in [768][1280] and proj_out [768][768] with bias, norm_out, four layers
  const half_t* latents = nullptr;
  LinW proj_in, proj_out;
  NormAffine norm_out;
  IpResampleLayerW layer[IPP_DEPTH];
  // to_k_ip / to_v_ip of the 16 blocks, contiguous in the blob in the step table's order ([12480][768] each, as kproj_all / vproj_all):
  // they live in tsd_model::unet.kproj_all / vproj_all so that g_unet_ctx_kv projects the image tokens exactly as it projects a context
  int n_blocks = 0;
  int kv_off[SD15_N] = {};  // per flat layer position: row offset of the block in the two tables (as AttnW::kv_off)
  int C[SD15_N] = {};       // per flat layer position: the block's width, 0 where the step is no attention block
};

struct ClipVisionLayerW { NormAffine ln1, ln2; LinW in_proj, out_proj, fc1, fc2; };
struct ClipVisionW {  // kind 22
  const float* cls = nullptr;   // [1280] fp32
  LinW patch;                   // [1280][588 -> 640], no bias
  const half_t* pos = nullptr;  // [257][1280] fp16
  NormAffine pre_ln, post_ln;
  ClipVisionLayerW layer[CV_LAYERS];
  LinW proj;                    // [1024][1280], no bias
};

struct PlanKey { int B, L, T; bool operator<(const PlanKey& o) const { return B != o.B ? B < o.B : (L != o.L ? L < o.L : T < o.T); } };

struct tsd_model {
  tsd_ctx* ctx = nullptr;
  int kind = 0;
  std::vector<ParamSpec> params;
  std::map<std::string, int> index;
  char* blob = nullptr;
  size_t blob_bytes = 0;
  std::vector<char> loaded;
  bool ready = false;
  unsigned gen = 0;  // parameter generation: moves whenever `ready` is cleared (set_param, init_random, mark_loaded); a denoise session
                     // remembers the one its step-invariant buffers were built from
  UNetW unet;
  VaeW vae;
  ClipW clip;
  IpAdapterW ip;
  ClipVisionW vision;
  std::map<PlanKey, size_t> plans;  // workspace high-water mark per problem shape
  char* derived = nullptr;          // derived device buffers rebuilt by model_check_ready(): fused-tail weight streams
  size_t derived_bytes = 0;
  // low-rank adapters (tsd_model_lora_add): parameter index -> device copy of its packed bytes as they were before the first merge (the
  // base).  tsd_model_lora_clear copies them back bit for bit; set_param drops the entry of its parameter (the new value is the new base),
  // init_random / mark_loaded drop all of them.
  std::map<int, char*> lora_base;
  // FreeU (tsd_model_set_freeu; full-size UNets only): (b_j, s_j) of the twelve decoder residual blocks in pop order.  Read by
  // unet_full_steps when the forward is enqueued; off (or all ones): the forward enqueues what it always did.
  bool freeu_on = false;
  int freeu_mode = 0;
  float freeu_b[TSD_FREEU_BLOCKS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, freeu_s[TSD_FREEU_BLOCKS] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
};

int model_resolve(tsd_model* m);                      // fill unet / vae from the packed blob
ConvW model_conv(const tsd_model* m, const std::string& prefix);
LinW model_lin(const tsd_model* m, const std::string& prefix, bool use_bias);
int model_check_ready(tsd_model* m);
// width of the context rows: what a UNet / ControlNet's k_proj reads, what a text encoder writes; 0 for a VAE
static inline int model_context_width(const tsd_model* m) {
  if (is_diffusion_kind(m->kind) || is_controlnet_kind(m->kind)) return m->unet.kproj_all.K;
  return is_clip_kind(m->kind) ? m->clip.D : 0;
}
static inline int clip_kind_width(int kind) { return kind == TSD_MODEL_CLIP_SD2 ? 1024 : 768; }
static inline int clip_kind_layers(int kind) { return kind == TSD_MODEL_CLIP_SD2 ? 23 : 12; }
