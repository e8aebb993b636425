// Host runtime + C-ABI of libagenda_hip.so (see include/agenda_hip.h for the contract).
// Owns: bf16 re-laid weights, an activation arena, cross-attention K/V caches, heat-map
// accumulators; walks the SD UNet / VAE-decoder graphs as stream-ordered HIP kernel launches.
#include "../../include/agenda_hip.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

// ---------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------
static thread_local char g_err[2048] = "";
// C ABI entry points are the only default-visibility symbols of the library (built with -fvisibility=hidden)
#define AGD_API extern "C" __attribute__((visibility("default")))
extern "C" void agd_set_error(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
#define CK(expr) do { if ((expr) != 0) return -1; } while (0)
#define FAIL(...) do { agd_set_error(__VA_ARGS__); return -1; } while (0)

struct WMat { bf16_t* w = nullptr; int N = 0, Cin = 0, Cpad = 0, taps = 0;
              int sc_cols = 0;                                   // conv2 with its block's conv_shortcut appended: rows are [taps x Cpad | sc_cols] (igemm_halo.h shortcut loop)
              bf16_t* wfrag = nullptr; int wfrag_ni = 0; };   // the matrix once more in MFMA fragment order (igemm_wreg.h), column ranges of wfrag_ni x 16
// cpart: per-(M tile, channel) partial sums the producing igemm launch leaves for a following GroupNorm
// ([B*H*W / cpart_bm][C] float2; cpart_bm = 0: none were produced -> the GroupNorm runs its own statistics pass)
// normed / normed_gamma: a GroupNorm of this activation that its producer already applied (split-K slab pass, igemm.hip splitk_reduce_gn_kernel):
// the consumer whose norm weights are `normed_gamma` reads `normed` instead of running the GroupNorm kernels
struct Act { bf16_t* p = nullptr; int B = 0, H = 0, W = 0, C = 0; float* cpart = nullptr; int cpart_bm = 0;
             bf16_t* normed = nullptr; const float* normed_gamma = nullptr;
             long long n() const { return (long long)B * H * W * C; } };
// the GroupNorm that will read a resnet's output next, when it reads that tensor alone (no concat): lets a split-K conv2 normalise in its slab pass
struct NextGn { const float* gamma = nullptr; const float* beta = nullptr; float eps = 0.f; int silu = 0; };

struct Arena {
  char* base = nullptr; size_t cap = 0, off = 0, peak = 0;
  void* alloc(size_t bytes) {
    size_t a = (off + 255) & ~(size_t)255;
    if (a + bytes > cap) { agd_set_error("activation arena exhausted: need %zu + %zu > %zu bytes (raise workspace_bytes)", a, bytes, cap); return nullptr; }
    off = a + bytes; if (off > peak) peak = off;
    return base + a;
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
};

enum { PC_CONV3 = 0, PC_GEMM, PC_ATTN_SELF, PC_ATTN_CROSS, PC_GN, PC_LN, PC_ELEM, PC_HEAT, PC_VAE_ATTN, PC_OTHER, PC_TOUCH };
static const char* kClassNames[AGD_N_CLASSES] = {"igemm_conv3x3", "igemm_linear_1x1", "attn_self_flash", "attn_cross_daam",
                                                 "groupnorm", "layernorm", "elementwise", "heatmap", "vae_attn_softmax", "other", "weight_touch"};

// device buffer that only grows (capacity in bytes); the old block is freed when a larger one is needed
struct DBuf {
  void* p = nullptr; size_t cap = 0;
  template <typename T> T* as() const { return (T*)p; }
  int ensure(size_t bytes) {
    if (p && bytes <= cap) return 0;
    if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); p = nullptr; cap = 0; }
    const size_t want = bytes ? bytes : 256;
    if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; agd_set_error("hipMalloc(%zu) failed", want); return -1; }
    cap = want;
    return 0;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct XLayer {
  std::string name; int C = 0, heads = 0, level = 0; bool mid = false;
  bool cn = false;                                    // a ControlNet layer: K/V and the pre-multiplied form like the UNet's, never recorded
  WMat wkv; DBuf kvb; bf16_t* kv = nullptr; DBuf accb; float* acc = nullptr; int acc_h = 0, acc_w = 0;
  int acc_heads = 0;                                  // slices in acc per image: `heads`, or fewer = head-group sums (layers at latent resolution)
  DBuf wqTb, wkvTb, woTb; WMat wqT, wkvT, woT;        // transposed weights for the input-gradient GEMMs (built on first backward)
  // attn2 against per-image pre-multiplied context matrices (xattn_pre.hip; the C = 1280 blocks): load-time parts (to_q transposed, Wq . norm2.bias)
  // and the per-prompt-batch products K'' / cs / bs / V'' (agd_set_context)
  bf16_t* pm_wqT = nullptr; float* pm_wqb = nullptr; bool pm_ready = false;
  DBuf pm_kppb, pm_vppb, pm_csb; bf16_t* pm_kpp = nullptr; bf16_t* pm_vpp = nullptr; float* pm_kcs = nullptr; float* pm_kbs = nullptr;
};

// one GLIGEN GatedSelfAttentionDense ("<pre>transformer_blocks.0.fuser."): fused q/k/v and k/v, the tanh gates, the to_out / ff.net.2 biases
// pre-scaled by them (agd_finalize), and the per-call grounding K/V [B2][max_objs][2C] bf16 (agd_gligen_set)
struct Fuser {
  std::string pre; int C = 0, heads = 0;
  WMat wqkv, wkv; float ta = 0.f, td = 0.f; float* bo_s = nullptr; float* b2_s = nullptr;
  DBuf gkvb;
};

// one attn2 layer's IP-Adapter parts ("<pre>transformer_blocks.0.attn2.to_k_ip / to_v_ip.weight" bf16 [C][cross_attention_dim]) and its per-call
// pre-multiplied matrices K'' [B2][cols][C], V'' [B2][C][cols] (bf16), cs | bs [2][B2][cols] (ipadapter.hip)
struct IpaLayer {
  std::string pre; int C = 0, heads = 0, cols = 0;
  DBuf wk, wv, kppb, vppb, csbsb;
};

// agd_set_option("tblock_fuse"): the fused row-panel kernels of the transformer blocks (tblock.hip).  Read by tblock_plan() alone.
enum : int {
  TBF_FF            = 1 << 0,    // C = 320: norm3 -> GEGLU -> ff.net.2 + residual in one launch
  TBF_ATTN2         = 1 << 1,    // C = 320: the attn2 chain, norm2 -> to_q -> attention (+ DAAM record) -> to_out + residual in one launch
  TBF_ATTN1_OUT     = 1 << 2,    // attn1.to_out + residual in front of the attn2 chain, same launch
  TBF_FF_PROJ       = 1 << 3,    // proj_out + residual behind the fused feed-forward, same launch
  TBF_QKV           = 1 << 4,    // C = 320: proj_in -> norm1 -> q / k / v in one launch (the qkv chain)
  TBF_ATTN2_640     = 1 << 5,    // the attn2 chain for the C = 640 blocks too
  TBF_LAZY_DUP      = 1 << 6,    // the CFG-shared prefix's duplication inside the fused kernels (no copy launches)
  TBF_QKV_GN        = 1 << 7,    // the GroupNorm applied inside the qkv chain (no fold launch)
  TBF_QKV_640       = 1 << 8,    // the qkv chain with the GroupNorm inside for the C = 640 blocks too (off: measured slower than the three launches it replaces)
  TBF_FF_PREMUL     = 1 << 9,    // ff.net.2 / proj_out pre-multiplied inside the feed-forward launch
  TBF_ATTN2_ROWS32  = 1 << 10,   // 32-row panels for the C = 640 attn2 chain where 64-row panels would fill half the chip
  TBF_QKV_ROWS64    = 1 << 11,   // the C = 320 qkv chain on 64-row panels (two co-resident four-wave workgroups per CU)
  TBF_QKV_SCHED2    = 1 << 12,   // the qkv chain on qkv_chain2_kernel's schedule (same results bit for bit)
  TBF_DEFAULT       = 0x1fff & ~TBF_QKV_640,   // 7935
};

struct ProfEv { int cls; double flops, bytes; hipEvent_t a, b; };   // algorithmic flop / HBM bytes of the launch

// What ONE model evaluation runs beside the UNet (resolve_cond() -> CallCond::at(i) -> unet_walk).  Default: the plain UNet.
struct EvalCond {
  float cn_scale = 0.f;    // != 0: the ControlNet runs after the mid block, its residuals times cn_scale land on the skips and the mid output
  bool grounded = false;   // the GLIGEN fusers run in the UNet's transformer blocks
  float ad_scale = 0.f;    // != 0: the T2I-Adapter's features times ad_scale are added to the down blocks' outputs
  bool ipa = false;        // the IP-Adapter's image branch runs beside every UNet attn2
  bool pag = false;        // the perturbed branch of Perturbed-Attention Guidance: the applied self-attention layers pass their value rows through
  int dc = 0;              // DeepCache: 0 = the plain walk, DC_CAPTURE = the plain walk + the capture of U_{b+1}'s hidden-state input, DC_SHALLOW = the shallow walk on the cached one
  int dc_branch = 0;       // b of the above
};
enum : int { DC_CAPTURE = 1, DC_SHALLOW = 2 };

struct agd_ctx {
  int device = 0; agd_config cfg{}; std::string err;
  std::unordered_map<std::string, WMat> W;
  std::unordered_map<std::string, float*> V;
  std::unordered_map<std::string, int> Vn;
  std::vector<void*> owned;
  Arena arena; bf16_t* zero_page = nullptr;
  float* stage = nullptr; size_t stage_bytes = 0;
  bool finalized = false;
  // time embedding
  WMat tproj_all; float* tproj_bias = nullptr; float* tproj_out = nullptr; int tproj_total = 0;
  const float* tproj_cur = nullptr;                 // time_emb_proj outputs of the forward being walked
  int tproj_cur_ld = 0;                             // 0: one timestep for every image; tproj_total: one row per image (agd_unet_forward_ts)
  float* tsteps_buf = nullptr; int tsteps_cap = 0;   // agd_denoise: embeddings of ALL steps, computed up front
  std::unordered_map<std::string, int> tproj_off;
  float* temb_buf = nullptr;   // [dim | 4dim | 4dim] fp32 scratch
  float* t_dev = nullptr;
  // cross attention
  std::vector<XLayer> xl; std::unordered_map<std::string, int> xl_idx;
  DBuf ctxb; bf16_t* ctx_bf16 = nullptr; int ctx_B2 = 0, ctx_T = 0;
  // recorder
  int rec_mode = 0, rec_is_train = 0, rec_T_cfg = 0, rec_T = 0, rec_B = 0, rec_L = 0, rec_Lh = 0, rec_Lw = 0;   // rec_T: rows the accumulators were sized for (set by record_reset); rec_L: hook.py's square side
  DBuf hook_sumb, hook_scratchb, hook_headsb, hook_storeb;     // hook_heads: per-head probabilities of one call; hook_store: kept per-call maps (train mode)
  struct HookRec { size_t off; int Bp, T, N; };
  std::vector<HookRec> hook_recs; size_t hook_store_used = 0;
  DBuf bwd_wsb;                                                 // attention-backward workspace
  float* hook_sum = nullptr; float* hook_scratch = nullptr; int hook_count = 0, hook_Bp = 0, hook_T = 0;
  // DAAM states of a forward that covers only part of the rec_B images the accumulators hold (agd_denoise_panorama: one state per (panorama,
  // view), a chunk of views per forward): recorded image j of the forward is state rec_base + j, and the forward records iff it has rec_call
  // images.  0 / 0 = every other entry point: state j, rec_B images.
  int rec_base = 0, rec_call = 0;
  int pano_B = 0, pano_Lh = 0, pano_Lw = 0, pano_stride = 0;        // the last agd_denoise_panorama that recorded (agd_daam_global_panorama reads its geometry)
  DBuf pano_ctxb;                                                // agd_denoise_panorama: the prompts' bf16 context [2 B][T][D], kept while the tiled one is in place
  DBuf reg_xb;                                                   // agd_denoise_regions' region buffer [R][B][C][Lh][Lw] (scratch: no state)
  DBuf pano_viewb, pano_hmb;                                     // agd_denoise_panorama's views [V][B][C][win][win]; agd_daam_global_panorama's per-view maps
  // denoise scratch
  DBuf latb, epsb, vae_imgb, plmsb, dpmb;
  bf16_t* lat_bf16 = nullptr; float* eps_nhwc = nullptr;
  SplitKWs splitk;                                    // split-K partial slabs of this ctx (stream-ordered reuse)
  int opt_cfg_share = 1;                              // agd_set_option("cfg_shared_prefix")
  int opt_ln_fold = 1;                                // agd_set_option("ln_fold"): LayerNorm folded into the GEMMs around it
  int opt_gn_fused = 1;                               // agd_set_option("gn_fused_stats"): GroupNorm statistics from the producing igemm's epilogue
  int opt_warm = 3;                                   // agd_set_option("weight_warm"): in-kernel cold-weight warm-up: 1 = W-major launches (per-XCD slices), 3 = A-major launches too
  int opt_gn_proj_fold = 1;                           // agd_set_option("gn_proj_fold"): the transformers' GroupNorm folded into per-image proj_in matrices (1: C <= 320, 2: C <= 640)
  int opt_p8 = 1;                                     // agd_set_option("igemm8p"): 256-row 8-wave / 8-phase igemm for launches with enough tiles (igemm8p.h)
  int opt_halo = 1;                                   // agd_set_option("conv_halo"): 3x3 stride-1 convs through the row-halo kernel (igemm_halo.h)
  int opt_tb_fuse = TBF_DEFAULT;                       // agd_set_option("tblock_fuse"): the TBF_* bits above
  int opt_ups4 = 7; /* see agd_set_option */                                   // agd_set_option("upsample_phases"): the UNet's nearest-2x upsampling convs as four 2x2 phase convs on the un-upsampled map (one launch, 4/9 of the MACs)
  int opt_ffproj = 1;                                 // agd_set_option("ff_proj_fuse"): ff.net.2 and proj_out as ONE GEMM with the pre-multiplied matrix [Wp W2 | Wp] over [hidden | h] (blocks whose feed-forward is not the fused row-panel kernel)
  int opt_sc_fuse = 3;                                // agd_set_option("shortcut_fuse"): a UNet resnet's 1x1 conv_shortcut runs as extra K of its conv2 launch where that is an unsplit row-halo launch
  int opt_wreg = 3;                                   // agd_set_option("wreg_mask"): weight-streaming kernel (igemm_wreg.h) for bit 0: the C = 1280 GEGLU at 1024 <= M <= 4096 (the 16 x 16 blocks), bit 1: proj_in / proj_out of the C = 640 blocks
  int opt_kg2 = 1;                                    // agd_set_option("igemm_kgroups"): two K groups of waves per workgroup on the one-workgroup-per-CU 1x1 launches of the small maps
  int opt_side = 0;                                   // agd_set_option("side_stream"): a resnet's 1x1 conv_shortcut runs on a second stream beside norm1 / conv1 / norm2
  hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int opt_smap = 1;                                   // agd_set_option("conv_smap"): 3x3 convs of the 8 x 8 maps through the whole-images-resident kernel (igemm_smap.h)
  int opt_reduce_gn = 1;                              // agd_set_option("reduce_gn"): split-K slab sum + the GroupNorm that reads it as one launch (igemm.hip splitk_reduce_gn_kernel)
  int opt_xcd_block = 1;                              // agd_set_option("xcd_block"): the igemm tile grid cut into one block per XCD that minimises the XCD's L2 working set (igemm.hip pick_xcd_block)
  int opt_pc = 49;                                    // agd_set_option("igemm_pc"): producer / consumer igemm (igemm_pc.h) -- bit 0: 1x1 launches on 64 x 160 tiles, bit 1: 3x3 convs of the 16 x 16 maps;
                                                      // bit 4: the row-halo producer / consumer kernel (igemm_pch.h) for 3x3 convs whose 128 x 160 tiles (x K slices) fit one wave of workgroups;
                                                      // bit 5: the 1x1 launches of one 128 x 160 tile per CU (M = 8192, N = 640) on igemm_pc.h's 128-row form
  // safety checker (agd_safety_configure): the CLIP vision tower's config, its fp32 concept rows (special-care rows first, L2-normalised at finalize)
  agd_vision_config vis{}; bool vis_on = false; float* vis_concepts = nullptr;
  // the IP-Adapter's image encoder (agd_image_encoder_begin .. commit, after agd_finalize): weights "image_encoder.*"; ienc_state 0 none, 1 loading, 2 ready
  agd_vision_config ienc{}; int ienc_state = 0;
  int opt_xpre = 1;                                   // agd_set_option("attn2_premul"): attn2 of the C = 1280 blocks as two GEMMs against per-image pre-multiplied context matrices (xattn_pre.hip)
  int opt_touch = 3;                                  // agd_set_option("weight_touch"): n > 0 = stream 1x1 weight matrices of >= n MB through the caches right before their launch
  unsigned* touch_sink = nullptr;
  // ControlNet (agd_controlnet_configure): weights "controlnet.*", its transformer layers in xl with cn = true, its own stacked time_emb_proj
  // (offsets in tproj_off under its "controlnet." prefixes), the zero convs' biases back to back (cn_zb: as loaded, cn_zbs: times cn_zscale)
  agd_controlnet_config cnc{}; bool cn_on = false;
  WMat cn_tproj_all; float* cn_tproj_bias = nullptr; float* cn_tproj_out = nullptr; int cn_tproj_total = 0;
  int cn_nres = 0; float* cn_zb = nullptr; float* cn_zbs = nullptr; int cn_zb_total = 0; std::vector<int> cn_zb_off; float cn_zscale = NAN;
  DBuf cn_embb; int cn_emb_B2 = 0, cn_emb_Lh = 0, cn_emb_Lw = 0, cn_emb_rep = 0;      // the conditioning embedding [B2][Lh][Lw][C0] bf16 (agd_controlnet_set_cond)
  std::vector<float> cn_sched;                                         // agd_controlnet_set_schedule: one scale per model evaluation
  // inpainting (agd_inpaint_set): ip_mode 0 = none, 1 = the 9-channel UNet input (mask + masked-image latents in ip_condb), 2 = the 4-channel
  // blend (image latents in ip_condb, the noise in ip_noiseb, (sa, sb) per model evaluation in ip_sched); all fp32 NCHW for ip_B images
  int ip_mode = 0, ip_B = 0, ip_Lh = 0, ip_Lw = 0, ip_Cm = 0, ip_Cc = 0;
  DBuf ip_maskb, ip_condb, ip_noiseb;
  std::vector<float> ip_sched;
  // InstructPix2Pix (agd_ip2p_set_hw): the image latents fp32 NCHW [i2_B][vae latent channels][i2_Lh][i2_Lw] in i2_latb, unscaled, and the
  // image guidance scale; i2_prep_*: the shape agd_ip2p_prepare_hw left there (agd_ip2p_set_hw with a null pointer installs those)
  bool i2_on = false; int i2_B = 0, i2_Lh = 0, i2_Lw = 0; float i2_scale = 1.f;
  int i2_prep_B = 0, i2_prep_Lh = 0, i2_prep_Lw = 0;
  DBuf i2_latb;
  // LoRA (agd_lora_add / agd_lora_set_scale / agd_lora_clear): per target its fp32 factors and a bf16 copy of its base matrix (merge descriptors
  // on the host and in lora_descb), merged into the raw matrices and re-derived in place; lora_scratch: 8 C C bf16 for derive_tblock
  std::vector<std::string> lora_keys; std::vector<LoraMergeD> lora_d; int lora_tiles = 0;
  DBuf lora_descb; bf16_t* lora_scratch = nullptr; size_t lora_scratch_n = 0;
  float lora_scale = 0.f; bool lora_dirty = false;
  bool ctx_stale = false;                             // the raw matrices changed after agd_set_context: the projected context must be rebuilt
  // GLIGEN (agd_gligen_configure): one Fuser per UNet transformer block (gl_idx: block prefix -> index), the PositionNet output of the call
  // (gl_objb [gl_B2][max_objs][cross_attention_dim] bf16), one flag per model evaluation
  agd_gligen_config glc{}; bool gl_on = false;
  std::vector<Fuser> gl_f; std::unordered_map<std::string, int> gl_idx;
  DBuf gl_objb; int gl_B2 = 0; std::vector<int> gl_sched;
  // T2I-Adapter (agd_adapter_configure): weights "adapter.*"; the per-call UNSCALED features fp32 NHWC [ad_B][Lh >> i][Lw >> i][channels[i]]
  // (agd_adapter_set_cond_hw), one scale per model evaluation;
  // ad_adds: adds launched with / without GroupNorm partial sums
  agd_adapter_config adc{}; bool ad_on = false;
  DBuf ad_featb[AGD_MAX_LEVELS]; int ad_B = 0, ad_Lh = 0, ad_Lw = 0;
  std::vector<float> ad_sched; long long ad_adds[2] = {0, 0};
  // IP-Adapter (agd_ip_adapter_begin .. commit, after agd_finalize): the image projection and, per UNet attn2 layer (ipa_idx: block prefix ->
  // index), to_k_ip / to_v_ip; ipa_t: what agd_ip_adapter_tensor has received so far (name -> shape).  Per call (agd_ip_adapter_set): the
  // projected tokens fp32 [ipa_B2][ipa_nt][cross_attention_dim], every layer's pre-multiplied matrices and the scale; ipa_stale: a LoRA scale
  // change rewrote to_q / to_out after they were built; ipa_counts: score / add launches
  bool ipa_loading = false, ipa_on = false; int ipa_E = 0, ipa_nt = 0;
  DBuf ipa_projw, ipa_projb, ipa_ng, ipa_nb;
  std::unordered_map<std::string, std::vector<long long>> ipa_t;
  std::vector<IpaLayer> ipa_l; std::unordered_map<std::string, int> ipa_idx;
  DBuf ipa_embb, ipa_tokb, ipa_kipb, ipa_vipb, ipa_wqbb;
  int ipa_B2 = 0; float ipa_scale = 0.f; bool ipa_stale = false; long long ipa_counts[2] = {0, 0};
  // FreeU (agd_freeu_set / agd_freeu_clear): persistent; unet_walk re-weights the resnet inputs of up blocks 0 and 1 (freeu_apply).
  // fu_counts: launches that left GroupNorm partial sums / that left none
  bool fu_on = false; float fu_s[2] = {1.f, 1.f}, fu_b[2] = {1.f, 1.f}; long long fu_counts[2] = {0, 0};
  // guidance_rescale (agd_guidance_rescale_set / _clear): phi > 0 = set; the step lambdas of the two-branch loops read it (guidance_factor).
  // gr_factb: the [batch] factors of the evaluation in flight; gr_count: factor launches since create
  float gr_phi = 0.f; DBuf gr_factb; long long gr_count = 0;
  // Perturbed-Attention Guidance (agd_pag_set / agd_pag_clear): one scale per model evaluation (non-empty = set) and the applied self-attention
  // layers as transformer prefixes ("unet.mid_block.attentions.0."); pag_counts: perturbed walks / perturbed self-attention layers launched
  std::vector<float> pag_sched; std::unordered_set<std::string> pag_layers; long long pag_counts[2] = {0, 0};
  // DeepCache (agd_deepcache_set / agd_deepcache_clear): one flag per model evaluation (1 = full, 0 = shallow; non-empty = set) and the branch b.
  // dc_buf: the persistent slot outside the arena (unet_walk releases the arena at its start) -- the hidden state that entered U_{b+1} at the
  // last capture, bf16 [rows][Lh][Lw][C], and behind it (256-byte aligned) its GroupNorm partial sums; dc_act describes it (cpart_bm == 0: no
  // sums were left, the consumer runs its own statistics pass).  dc_valid: the slot holds a capture of (dc_rows, dc_Lh, dc_Lw, dc_b).
  // dc_counts: full evaluations that captured / shallow evaluations
  std::vector<int> dc_sched; int dc_branch = 0; long long dc_counts[2] = {0, 0};
  // Semantic Guidance (agd_sega_set / agd_sega_clear): sega_K > 0 = set; the descriptor's arrays, copied -- coef, w_mom, w_add [n][K], add_mom [n],
  // q [K].  sega_momb: the momentum fp32 [B][HW][4], zeroed at the start of every call; sega_thrb: the thresholds [B][K][4] of the evaluation
  // in flight.  sega_counts: concept walks / folds
  int sega_K = 0, sega_n = 0; float sega_mu = 0.f, sega_beta = 0.f; std::vector<float> sega_coef, sega_wmom, sega_wadd, sega_addmom; std::vector<double> sega_q;
  DBuf sega_momb, sega_thrb; long long sega_counts[2] = {0, 0};
  DBuf dc_buf; Act dc_act; bool dc_valid = false; int dc_rows = 0, dc_Lh = 0, dc_Lw = 0, dc_b = 0;
  // profiling
  EvalCond cur;                                       // the forward being walked (unet_walk sets it; tblock_plan, down_mid_walk and adapter_add read it)
  bool prof_on = false; std::vector<ProfEv> prof; std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
  long long launches[AGD_N_CLASSES] = {0};
};

static int fail_ctx(agd_ctx* c) { if (c) c->err = g_err; return -1; }
// frees everything an IP-Adapter holds (weights and per-call state); the caller has synchronised
static void ipa_release(agd_ctx* c) {
  for (auto& l : c->ipa_l) { l.wk.release(); l.wv.release(); l.kppb.release(); l.vppb.release(); l.csbsb.release(); }
  c->ipa_l.clear(); c->ipa_idx.clear(); c->ipa_t.clear();
  for (DBuf* b : {&c->ipa_projw, &c->ipa_projb, &c->ipa_ng, &c->ipa_nb, &c->ipa_embb, &c->ipa_tokb, &c->ipa_kipb, &c->ipa_vipb, &c->ipa_wqbb}) b->release();
  c->ipa_loading = c->ipa_on = false; c->ipa_E = c->ipa_nt = 0;
  c->ipa_B2 = 0; c->ipa_scale = 0.f; c->ipa_stale = c->cur.ipa = false; c->ipa_counts[0] = c->ipa_counts[1] = 0;
}
static inline int rec_images(const agd_ctx* c) { return c->rec_call > 0 ? c->rec_call : c->rec_B; }   // images a recording forward must have
#define API_CK(c, expr) do { if ((expr) != 0) return fail_ctx(c); } while (0)

struct ProfScope {
  agd_ctx* c; hipStream_t st; bool on; size_t idx;
  ProfScope(agd_ctx* c_, hipStream_t st_, int cls, double flops, double bytes = 0) : c(c_), st(st_), on(c_ && c_->prof_on), idx(0) {
    if (c) c->launches[cls]++;
    if (!on) return;
    auto get = [&]() { if (c->ev_used == c->ev_pool.size()) { hipEvent_t e; hipEventCreate(&e); c->ev_pool.push_back(e); } return c->ev_pool[c->ev_used++]; };
    ProfEv pe; pe.cls = cls; pe.flops = flops; pe.bytes = bytes; pe.a = get(); pe.b = get();
    hipEventRecord(pe.a, st);
    idx = c->prof.size(); c->prof.push_back(pe);
  }
  ~ProfScope() { if (on) hipEventRecord(c->prof[idx].b, st); }
};

// frees a dmalloc'd block before agd_destroy (load-time scratch); the caller has synchronised
static void dfree(agd_ctx* c, void* p) {
  if (!p) return;
  if (c) { auto it = std::find(c->owned.begin(), c->owned.end(), p); if (it != c->owned.end()) c->owned.erase(it); }
  (void)hipFree(p);
}
template <typename T> static T* dmalloc(agd_ctx* c, size_t n) {
  void* p = nullptr;
  if (hipMalloc(&p, n * sizeof(T) ? n * sizeof(T) : 256) != hipSuccess) { agd_set_error("hipMalloc(%zu) failed", n * sizeof(T)); return nullptr; }
  if (c) c->owned.push_back(p);
  return (T*)p;
}

// the smallest row tile a producer leaves GroupNorm partial sums on: every partial-sum table (an activation's below, DeepCache's slot) is sized for it
static const int kMinStatTile = 64;
// stats: the activation will be written by an igemm launch and read by a GroupNorm -> room for the producer's partial sums
static Act alloc_act(agd_ctx* c, int B, int H, int W, int C, bool stats = false) {
  Act a; a.B = B; a.H = H; a.W = W; a.C = C;
  a.p = (bf16_t*)c->arena.alloc((size_t)a.n() * 2);
  if (a.p && stats && c->opt_gn_fused && ((long long)H * W) % kMinStatTile == 0) {
    a.cpart = (float*)c->arena.alloc((size_t)((long long)B * H * W / kMinStatTile) * C * 2 * sizeof(float));     // worst case: 64-row tiles
    if (!a.cpart) a.p = nullptr;
  }
  return a;
}

// ---------------------------------------------------------------------------------------
// op wrappers
// ---------------------------------------------------------------------------------------
struct GemmOpt {
  const float* bias = nullptr; const float* rowadd = nullptr; int rowadd_ld = 0;
  const bf16_t* residual = nullptr; int ldr = 0; int geglu = 0; int act = 0; int out_f32 = 0; int ldo = 0;
  int stride = 1, up = 1; float alpha = 1.f;
  int* query_cfg = nullptr;                                                              // igemm_query only: {BM, BN, splits}
  Act* out_act = nullptr;                                                                // output feeds a GroupNorm: leave per-channel partial sums in it
  int rows_per_image = 0;                                                                // for out_act on linear-shaped launches (B=1, W=M): rows of one image
  float* rowstat_out = nullptr; int rowstat_slots = 0;                                   // producer side of the LayerNorm fold
  const float* ln_stats = nullptr; int ln_slots = 0; const float* ln_cs = nullptr; float ln_invC = 0.f, ln_eps = 0.f;   // consumer side
  int warm = 0;                 // benches: request the in-kernel cold-weight warm-up (the walk sets it through the ctx option)
  int halo = 0;                 // benches: allow the row-halo 3x3 kernel (the walk sets it through the ctx option)
  int want_rowstat = 0;         // igemm_query only: the launch will be a LayerNorm row-statistics producer (changes the kernel family)
  int p8 = 0;                   // benches: 1 = allow the 8-phase kernel, 2 / 3 = force its 256- / 160-wide tile (the walk sets it through the ctx option)
  int w_per_image = 0;          // 1x1 launches: image i multiplies with w.w + i * N * K (GroupNorm folded into per-image matrices)
  // the GroupNorm(+SiLU) that reads this launch's output next, for split-K launches (IgemmP::gn_y): *gn_fused = 1 when the slab-sum pass did it
  const float* gn_gamma = nullptr; const float* gn_beta = nullptr; bf16_t* gn_y = nullptr; int gn_groups = 0; float gn_eps = 0.f; int gn_silu = 0, gn_keep_out = 0; int* gn_fused = nullptr;
  int kg2 = 0;                  // benches / tests: two K groups of waves per workgroup on the 64-row 1x1 tiles (the walk sets it through the ctx option)
  int smap = 0;                 // benches / tests: allow the 8 x 8 whole-images-resident 3x3 kernel (the walk sets it through the ctx option)
  int xcd_block = 0;            // benches / tests: XCD-aware tile blocks (IgemmP::xcd_block; the walk sets it through the ctx option)
  int pc = 0;                   // benches / tests: producer / consumer kernel mask (IgemmP::pc; the walk sets it through the ctx option)
  int wreg = 0;                 // benches / tests: weight-streaming kernel for this launch when the WMat carries a fragment-order copy (bit 0 plain, bit 1 GEGLU)
  const bf16_t* sc0 = nullptr; const bf16_t* sc1 = nullptr; int sc_C0 = 0, sc_C1 = 0;   // the block's 1x1 conv_shortcut as extra K of this 3x3 launch (WMat::sc_cols)
  int ups4 = 0;                 // > 0: phase-decomposed upsampling conv (IgemmP::ups4 = Cout; ksize 2, the merged [4 Cout][4][Cin] matrix, hout / wout = the input size)
  int* can_fuse_sc = nullptr;   // query only: *can_fuse_sc = 1 when this launch could take a shortcut that way (nothing is launched)
  int pad = -1;                 // -1: 1 for 3x3, 0 for 1x1
  int hout = 0, wout = 0;       // >0: override (asymmetric (0,1,0,1) padding of the VAE encoder's stride-2 convs)
  int prof_cls = -1;            // >= 0: the profiler class of this launch (default: PC_CONV3 / PC_GEMM by kernel size)
};
static const int kTextExtraRows = 256;   // room for tokenizer.add_tokens() (learned tokens)

// streams `n16` 16-byte words through the memory hierarchy and keeps nothing
__global__ __launch_bounds__(256) void touch_kernel(const u32x4* __restrict__ p, long long n16, unsigned* __restrict__ sink) {
  unsigned a = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) { const u32x4 v = p[i]; a |= v[0] ^ v[1] ^ v[2] ^ v[3]; }
  if (a == 0x9E3779B9u) *sink = a;
}
static int run_conv(agd_ctx* c, hipStream_t st, const bf16_t* s0, int C0, const bf16_t* s1, int C1, int B, int Hin, int Win,
                    const WMat& w, int ksize, void* out, const GemmOpt& o, const bf16_t* zero_page) {
  IgemmP p{};
  p.src0 = s0; p.src1 = s1; p.C0 = C0; p.C1 = C1; p.Hin = Hin; p.Win = Win;
  p.ksize = ksize; p.stride = o.stride; p.pad = o.pad >= 0 ? o.pad : (ksize == 3 ? 1 : 0); p.up = o.up;
  p.Hout = o.hout > 0 ? o.hout : (Hin * o.up + 2 * p.pad - ksize) / o.stride + 1;
  p.Wout = o.wout > 0 ? o.wout : (Win * o.up + 2 * p.pad - ksize) / o.stride + 1;
  p.W = w.w; p.bias = o.bias; p.bias_mode = o.bias ? 1 : 0; p.rowadd = o.rowadd; p.rowadd_ld = o.rowadd_ld;
  p.residual = o.residual; p.N = w.N; p.K = w.taps * w.Cpad; p.M = B * p.Hout * p.Wout; p.ups4 = o.ups4;
  if (o.sc0) {
    if (w.sc_cols != o.sc_C0 + o.sc_C1 || w.sc_cols < 64) FAIL("conv: weight carries %d shortcut columns, the launch %d + %d", w.sc_cols, o.sc_C0, o.sc_C1);
    p.sc0 = o.sc0; p.sc1 = o.sc1; p.sc_C0 = o.sc_C0; p.sc_C1 = o.sc_C1; p.K += w.sc_cols;
  }
  const int nout = o.geglu ? w.N / 2 : w.N;
  p.ldr = o.ldr ? o.ldr : nout; p.out = out; p.out_f32 = o.out_f32; p.ldo = o.ldo ? o.ldo : nout;
  p.alpha = o.alpha; p.geglu = o.geglu; p.act = o.act; p.batch = 1; p.zero_page = zero_page; p.ws = c ? &c->splitk : nullptr;
  p.rowstat_out = o.rowstat_out; p.rowstat_slots = o.rowstat_slots;
  p.ln_stats = o.ln_stats; p.ln_slots = o.ln_slots; p.ln_cs = o.ln_cs; p.ln_invC = o.ln_invC; p.ln_eps = o.ln_eps;
  if (o.w_per_image) { p.w_per_image = 1; p.sW = (long long)w.N * w.taps * w.Cpad; }
  if (o.wreg && w.wfrag) { p.Wfrag = w.wfrag; p.wfrag_ni = w.wfrag_ni; p.wreg = o.wreg; p.wreg_mmin = 1; p.wreg_mmax = 1 << 30; }
  if (o.gn_y && c && c->opt_reduce_gn) { p.gn_gamma = o.gn_gamma; p.gn_beta = o.gn_beta; p.gn_y = o.gn_y; p.gn_groups = o.gn_groups; p.gn_eps = o.gn_eps; p.gn_silu = o.gn_silu;
                                         p.gn_keep_out = o.gn_keep_out; p.gn_fused = o.gn_fused; }
  p.halo = (c && c->opt_halo) || o.halo;
  p.smap = (c && c->opt_smap) || o.smap;
  p.kg2 = (c && c->opt_kg2) || o.kg2;
  p.pc = (c ? c->opt_pc : 0) | o.pc;
  p.xcd_block = (c ? c->opt_xcd_block : 0) | o.xcd_block;
  p.p8 = o.p8 < 0 ? 0 : o.p8 ? o.p8 : c ? c->opt_p8 : 0;          // before any igemm_query: the tile shape depends on it (-1: not for this launch)
  if (o.query_cfg) { if (o.want_rowstat && !p.rowstat_out) { p.rowstat_out = (float*)16; p.rowstat_slots = 0; } return igemm_query(p, o.query_cfg); }   // (nothing is launched)
  if (o.out_act) {
    o.out_act->cpart_bm = 0;
    if (o.out_act->cpart && !o.out_f32 && !o.geglu) {
      int cfg[3] = {0, 0, 0};
      if (igemm_query(p, cfg) != 0) {                      // (a shortcut-fusion query on a launch that cannot take the shortcut: "no", not an error)
        if (o.can_fuse_sc) { *o.can_fuse_sc = 0; return 0; }
        return -1;
      }
      const int rpi = o.rows_per_image > 0 ? o.rows_per_image : p.Hout * p.Wout;
      // split-K launches keep the separate statistics kernel: a reduce pass that also emits partial sums was measured
      // slower than the two it replaces (+5.7 ms per batch, tools/ab_option.py)
      if (cfg[2] == 1 && cfg[0] > 0 && rpi % cfg[0] == 0) { p.colstat_out = o.out_act->cpart; p.colstat_rows = rpi; o.out_act->cpart_bm = cfg[0]; }
    }
  }
  // (asked AFTER the column-statistics decision above: the query must see the launch exactly as it will run -- a statistics producer never splits K,
  //  which can change the tile the launcher picks)
  if (o.can_fuse_sc) { *o.can_fuse_sc = igemm_can_fuse_shortcut(p) ? 1 : 0; return 0; }
  if (w.taps != ksize * ksize || w.Cpad != C0 + C1) FAIL("conv: weight [N=%d taps=%d Cpad=%d] does not match input C=%d+%d ksize=%d", w.N, w.taps, w.Cpad, C0, C1, ksize);
  // algorithmic HBM bytes: every input pixel / weight read once, the output written once (+ the residual read)
  const double in_b = 2.0 * B * Hin * Win * (double)(C0 + C1), w_b = 2.0 * p.N * (double)p.K;
  const double out_b = (double)p.M * nout * (o.out_f32 ? 4.0 : 2.0) + (o.residual ? 2.0 * p.M * nout : 0.0);
  // W-major launches (weights >= 1.5x the activations) warm their weights inside the kernel; the launcher's rule restated here
  const bool wmaj = ksize == 1 && w_b > 1.5 * in_b && w_b >= (double)(1 << 20);
  if (c && c->opt_warm) p.warm = c->opt_warm == 1 ? 1 : 3;      // 1: W-major launches only; 3: also A-major launches with >= 1 MB of weights (the launcher decides)
  if (o.warm) p.warm = o.warm;
  if (c && c->opt_touch > 0 && ksize == 1 && p.M <= 8192 && w_b >= c->opt_touch * 1e6 && !(c->opt_warm && wmaj) && c->opt_warm != 3) {
    // the weights arrive cold (1.7 GB per forward against 256 MB of Infinity Cache): a full-rate streaming read in front of the launch
    // costs less than the tile-by-tile cold misses inside it (tools/kb_cold.py; in situ 575.5 -> 572.3 ms per batch, tools/ab_option.py;
    // touching the 3x3 matrices of the 16x16 maps as well gave the gain back)
    if (!c->touch_sink) c->touch_sink = dmalloc<unsigned>(c, 64);
    if (c->touch_sink) { ProfScope pt(c, st, PC_TOUCH, 0, w_b);
      hipLaunchKernelGGL(touch_kernel, dim3(1024), dim3(256), 0, st, (const u32x4*)w.w, (long long)(w_b / 16), c->touch_sink); }
  }
  ProfScope ps(c, st, o.prof_cls >= 0 ? o.prof_cls : (ksize != 1 ? PC_CONV3 : PC_GEMM), 2.0 * p.M * (double)p.N * p.K, in_b + w_b + out_b + 2.0 * B * Hin * Win * (double)(o.sc_C0 + o.sc_C1));
  return launch_igemm(p, st);
}

static int run_gn(agd_ctx* c, hipStream_t st, const bf16_t* x0, int C0, const bf16_t* x1, int C1, int B, int HW,
                  const float* gamma, const float* beta, int groups, float eps, int silu, bf16_t* y,
                  const Act* a0 = nullptr, const Act* a1 = nullptr) {
  GroupNormP g{}; g.x0 = x0; g.x1 = x1; g.C0 = C0; g.C1 = C1; g.y = y; g.gamma = gamma; g.beta = beta;
  g.B = B; g.HW = HW; g.groups = groups; g.eps = eps; g.silu = silu;
  if (c->opt_gn_fused && a0 && a0->cpart_bm > 0 && (!x1 || (a1 && a1->cpart_bm > 0))) {      // every source brought its partial sums
    g.part0 = a0->cpart; g.bm0 = a0->cpart_bm;
    if (x1) { g.part1 = a1->cpart; g.bm1 = a1->cpart_bm; }
  }
  if (groupnorm_check(B, C0, C1, HW, groups)) return -1;                 // before the workspace geometry divides by C / 8
  const long long wsf = groupnorm_ws_floats(B, C0 + C1, HW, groups);
  const size_t mk = c->arena.mark();
  g.ws = (float*)c->arena.alloc((size_t)wsf * 4);
  if (!g.ws) return -1;
  ProfScope ps(c, st, PC_GN, 0, 4.0 * B * HW * (double)(C0 + C1));       // one read + one write of the activation
  const int rc = launch_groupnorm(g, st);
  c->arena.release(mk);   // stream-ordered: later kernels that reuse this memory run after the norm
  return rc;
}

static const WMat* getW(agd_ctx* c, const std::string& k) {
  auto it = c->W.find(k);
  if (it == c->W.end()) { agd_set_error("missing weight '%s'", k.c_str()); return nullptr; }
  return &it->second;
}
static const float* getV(agd_ctx* c, const std::string& k) {
  auto it = c->V.find(k);
  if (it == c->V.end()) { agd_set_error("missing tensor '%s'", k.c_str()); return nullptr; }
  return it->second;
}
#define GETW(var, key) const WMat* var = getW(c, key); if (!var) return -1
#define GETV(var, key) const float* var = getV(c, key); if (!var) return -1

// ResnetBlock2D (norm1-silu-conv1 (+temb) - norm2-silu-conv2 + shortcut)
static int resnet(agd_ctx* c, hipStream_t st, const std::string& pre, const Act& x0, const Act* x1, int Cout, float eps,
                  bool has_temb, int groups, Act& out, const NextGn* next = nullptr) {
  const int B = x0.B, H = x0.H, Wd = x0.W, HW = H * Wd;
  const int C1 = x1 ? x1->C : 0, Cin = x0.C + C1;
  out = alloc_act(c, B, H, Wd, Cout, true); if (!out.p) return -1;
  bf16_t* out_normed = nullptr;
  if (next && next->gamma && c->opt_reduce_gn) { out_normed = (bf16_t*)c->arena.alloc((size_t)out.n() * 2); if (!out_normed) return -1; }   // lives as long as `out`
  const size_t mk = c->arena.mark();
  // the 1x1 conv_shortcut depends on the block's input alone: with the option on it runs on a second stream beside norm1 / conv1 / norm2
  // (those launches are one workgroup per CU or fewer on the small maps); unsplit launches only -- the split-K workspace is the main stream's
  bf16_t* side_out = nullptr;
  const bool has_sc = c->W.count(pre + "conv_shortcut.weight") != 0;
  if (has_sc && c->opt_side && (c->opt_side == 1 || HW <= c->opt_side)) {        // 1: every level; else: maps of at most that many pixels
    GETW(ws, pre + "conv_shortcut.weight"); GETV(bs, pre + "conv_shortcut.bias");
    GemmOpt os; os.bias = bs; int cfg[3] = {0, 0, 0}; os.query_cfg = cfg;
    CK(run_conv(c, st, x0.p, x0.C, x1 ? x1->p : nullptr, C1, B, H, Wd, *ws, 1, nullptr, os, c->zero_page));
    if (cfg[2] == 1) {
      if (!c->side) {
        if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) FAIL("side stream");
      }
      side_out = (bf16_t*)c->arena.alloc((size_t)B * HW * Cout * 2); if (!side_out) return -1;
      os.query_cfg = nullptr;
      if (hipEventRecord(c->ev_fork, st) != hipSuccess || hipStreamWaitEvent(c->side, c->ev_fork, 0) != hipSuccess) FAIL("side stream fork");
      CK(run_conv(c, c->side, x0.p, x0.C, x1 ? x1->p : nullptr, C1, B, H, Wd, *ws, 1, side_out, os, c->zero_page));
      if (hipEventRecord(c->ev_join, c->side) != hipSuccess) FAIL("side stream join");
    }
  }
  Act n1 = alloc_act(c, B, H, Wd, Cin); if (!n1.p) return -1;
  GETV(g1, pre + "norm1.weight"); GETV(b1, pre + "norm1.bias");
  const bf16_t* n1p = n1.p;
  if (!x1 && x0.normed && x0.normed_gamma == g1) n1p = x0.normed;      // the producer's slab pass already applied this very norm
  else CK(run_gn(c, st, x0.p, x0.C, x1 ? x1->p : nullptr, C1, B, HW, g1, b1, groups, eps, 1, n1.p, &x0, x1));
  Act h = alloc_act(c, B, H, Wd, Cout, true); if (!h.p) return -1;
  GETW(w1, pre + "conv1.weight"); GETV(cb1, pre + "conv1.bias");
  GemmOpt o1; o1.bias = cb1; o1.out_act = &h;
  if (has_temb) {
    auto it = c->tproj_off.find(pre);
    if (it == c->tproj_off.end()) FAIL("no time_emb_proj for %s", pre.c_str());
    o1.rowadd = c->tproj_cur + it->second; o1.rowadd_ld = c->tproj_cur_ld;
  }
  Act n2 = alloc_act(c, B, H, Wd, Cout); if (!n2.p) return -1;
  GETV(g2, pre + "norm2.weight"); GETV(b2, pre + "norm2.bias");
  // conv1's output is read by norm2 and by nothing else: a split-K launch's slab-sum pass normalises straight into n2 (h is not written)
  int gn_done = 0;
  o1.gn_gamma = g2; o1.gn_beta = b2; o1.gn_y = n2.p; o1.gn_groups = groups; o1.gn_eps = eps; o1.gn_silu = 1; o1.gn_keep_out = 0; o1.gn_fused = &gn_done;
  CK(run_conv(c, st, n1p, Cin, nullptr, 0, B, H, Wd, *w1, 3, h.p, o1, c->zero_page));
  if (!gn_done) CK(run_gn(c, st, h.p, Cout, nullptr, 0, B, HW, g2, b2, groups, eps, 1, n2.p, &h));
  const bf16_t* res = x0.p;
  // conv_shortcut as extra K of conv2 (igemm_halo.h shortcut loop): one launch, the shortcut's output never exists -- where conv2 is an unsplit row-halo launch
  bool fuse_sc = false;
  if (has_sc && !side_out && (c->opt_sc_fuse & (H == 8 && Wd == 8 ? 2 : 1)) && c->W.count(pre + "conv2.sc")) {
    GETW(w2q, pre + "conv2.sc");
    int can = 0; GemmOpt q; q.can_fuse_sc = &can; q.sc0 = x0.p; q.sc_C0 = x0.C; q.sc1 = x1 ? x1->p : nullptr; q.sc_C1 = C1;
    q.out_act = &out;                                    // the launch below as it will run (its output leaves GroupNorm partial sums)
    CK(run_conv(c, st, n2.p, Cout, nullptr, 0, B, H, Wd, *w2q, 3, nullptr, q, c->zero_page));
    fuse_sc = can != 0;
  }
  if (fuse_sc) {
    GETW(w2s, pre + "conv2.sc"); GETV(cbs, pre + "conv2.sc.bias");
    GemmOpt o2; o2.bias = cbs; o2.out_act = &out; o2.sc0 = x0.p; o2.sc_C0 = x0.C; o2.sc1 = x1 ? x1->p : nullptr; o2.sc_C1 = C1;
    int gn2_done = 0;
    if (out_normed) {      // (as below: a split-K launch's slab pass also applies the GroupNorm that reads this output next)
      o2.gn_gamma = next->gamma; o2.gn_beta = next->beta; o2.gn_y = out_normed; o2.gn_groups = groups; o2.gn_eps = next->eps; o2.gn_silu = next->silu;
      o2.gn_keep_out = 1; o2.gn_fused = &gn2_done;
    }
    CK(run_conv(c, st, n2.p, Cout, nullptr, 0, B, H, Wd, *w2s, 3, out.p, o2, c->zero_page));
    if (gn2_done) { out.normed = out_normed; out.normed_gamma = next->gamma; }
    c->arena.release(mk);
    return 0;
  }
  if (side_out) {
    if (hipStreamWaitEvent(st, c->ev_join, 0) != hipSuccess) FAIL("side stream wait");
    res = side_out;
  } else if (has_sc) {
    GETW(ws, pre + "conv_shortcut.weight"); GETV(bs, pre + "conv_shortcut.bias");
    GemmOpt os; os.bias = bs;
    CK(run_conv(c, st, x0.p, x0.C, x1 ? x1->p : nullptr, C1, B, H, Wd, *ws, 1, h.p, os, c->zero_page));  // h is free again
    res = h.p;
  } else if (x1 || x0.C != Cout) {
    FAIL("resnet %s: channel change %d->%d without conv_shortcut", pre.c_str(), Cin, Cout);
  }
  GETW(w2, pre + "conv2.weight"); GETV(cb2, pre + "conv2.bias");
  GemmOpt o2; o2.bias = cb2; o2.residual = res; o2.out_act = &out;
  int gn2_done = 0;
  if (out_normed) {      // the next GroupNorm reads this output alone: a split-K launch's slab pass writes the output AND its normalised copy
    o2.gn_gamma = next->gamma; o2.gn_beta = next->beta; o2.gn_y = out_normed; o2.gn_groups = groups; o2.gn_eps = next->eps; o2.gn_silu = next->silu;
    o2.gn_keep_out = 1; o2.gn_fused = &gn2_done;
  }
  CK(run_conv(c, st, n2.p, Cout, nullptr, 0, B, H, Wd, *w2, 3, out.p, o2, c->zero_page));
  if (gn2_done) { out.normed = out_normed; out.normed_gamma = next->gamma; }
  c->arena.release(mk);
  return 0;
}

static int run_attention(agd_ctx* c, hipStream_t st, int cls, AttnP& a) {
  const double fl = 4.0 * a.B * a.H * (double)a.Nq * a.Nk * a.D;
  // q read + o written + k/v read once per (batch, head); the recorder's read-modify-write of its fp32 rows on top
  double by = 2.0 * a.B * a.H * (double)a.D * (2.0 * a.Nq + 2.0 * a.Nk);
  if (a.record_mode == 1) by += 8.0 * (a.B - a.rec_b0) * a.H * (double)a.rec_T * a.Nq;
  else if (a.record_mode == 2 || a.record_mode == 3) by += 8.0 * (a.B - a.rec_b0) * (double)a.rec_T * a.Nq;
  ProfScope ps(c, st, cls, fl, by);
  return launch_attention(a, st);
}

// DAAM's recording rule, for an attn2 call of B2 images (a CFG pair per recorded image) on a qh x qw query map: the recorder is on, the layer
// is not the mid block's and has accumulators of this map's size, and the images are the ones they were sized for.  factor = sqrt(latent
// h * w / N) = Lh / qh; recorded iff factor != 8; the conditional half only.
static inline bool daam_records(const agd_ctx* c, const XLayer& xl, int B2, int qh, int qw) {
  return c->rec_mode == 1 && !xl.mid && xl.acc && c->rec_Lh / qh != 8 && qh == xl.acc_h && qw == xl.acc_w && B2 / 2 == rec_images(c);
}

// cross-attention attn2 body shared by the UNet walk and the agd_cross_attn seam
// qh x qw: the query map (N = qh * qw); the seam passes the square side of its token count
static int cross_attention(agd_ctx* c, hipStream_t st, XLayer& xl, const bf16_t* q, int B2, int N, int qh, int qw, bf16_t* out, bool record,
                           const float* mask = nullptr) {
  const int C = xl.C, D = C / xl.heads, T = c->ctx_T;
  if (xl.cn) record = false;                           // DAAM and hook.py see the UNet's layers only
  AttnP a{}; a.q = q; a.k = xl.kv; a.v = xl.kv + C; a.o = out;
  a.ldq = C; a.ldk = 2 * C; a.ldv = 2 * C; a.ldo = C;
  a.sq = (long long)N * C; a.sk = (long long)T * 2 * C; a.sv = a.sk; a.so = a.sq;
  a.B = B2; a.H = xl.heads; a.D = D; a.Nq = N; a.Nk = T; a.scale = 1.0f / sqrtf((float)D);
  a.record_mode = 0; a.mask = mask;
  const int side = qh;                                 // (hook.py mode: square maps only)
  bool hook_call = false;
  // a context beyond 96 tokens: DAAM records through attention_long.hip (per-head rows, final probabilities over several key tiles);
  // whatever does not record runs the flash kernel, which walks key tiles already
  const bool long_ctx = T > 96;
  if (long_ctx && record && c->rec_mode == 2) FAIL("the hook.py recorder takes contexts of at most 96 tokens (this one has %d)", T);
  if (record && daam_records(c, xl, B2, qh, qw)) {
    if (long_ctx) {
      if (mask) FAIL("attention_mask together with daam recording is not supported beyond 96 tokens (this context has %d)", T);
      if (xl.acc_heads < xl.heads || c->rec_T > T)
        FAIL("%s: the daam accumulators hold %d of %d head rows and %d token rows, this context has %d tokens: reset after agd_set_context (agd_record_reset)",
             xl.name.c_str(), xl.acc_heads, xl.heads, c->rec_T, T);
    }
    a.rec_b0 = B2 / 2; a.rec_T = c->rec_T;
    a.rec_head_stride = (long long)c->rec_T * N; a.rec_img_stride = a.rec_head_stride * xl.acc_heads;
    a.rec = xl.acc + (size_t)c->rec_base * a.rec_img_stride;
    if (xl.acc_heads < xl.heads) {                   // latent-resolution layer: head-group sums (attention.hip RECORD 2)
      if (mask) FAIL("attention_mask together with daam recording at latent resolution is not supported");
      a.record_mode = 3; a.rec_hpb = xl.heads / xl.acc_heads;
    } else a.record_mode = 1;
  } else if (record && c->rec_mode == 2 && c->hook_scratch) {
    const int b0 = c->rec_is_train ? 0 : B2 / 2;
    if (B2 - b0 == c->hook_Bp) {
      if (qh != qw) FAIL("the hook.py recorder takes square maps only (h = w = sqrt(N)); this call's map is %d x %d", qh, qw);
      if (T != c->hook_T || side > c->rec_L) FAIL("hook recorder was reset for %d tokens / latent side %d but this call has %d tokens / side %d: call clear() (agd_record_reset) after changing the context", c->hook_T, c->rec_L, T, side);
      // per-head probabilities of this call (plain read-modify-write rows, like the DAAM accumulators), then an ORDERED
      // head mean (hook.py:55): reproducible run to run, unlike float atomics across the head workgroups
      const size_t nh = (size_t)c->hook_Bp * xl.heads * T * N;
      CK(c->hook_headsb.ensure(nh * 4));
      if (hipMemsetAsync(c->hook_headsb.p, 0, nh * 4, st) != hipSuccess) FAIL("memset hook heads");
      a.record_mode = 1; a.rec_b0 = b0; a.rec = c->hook_headsb.as<float>(); a.rec_T = T;
      a.rec_head_stride = (long long)T * N; a.rec_img_stride = a.rec_head_stride * xl.heads;
      hook_call = true;
    }
  }
  if (long_ctx && a.record_mode != 0) {
    const double fl = 6.0 * a.B * a.H * (double)a.Nq * a.Nk * a.D;      // Q K^T twice (attention_long.hip's two passes), P V once
    const double by = 2.0 * a.B * a.H * (double)a.D * (2.0 * a.Nq + 3.0 * a.Nk) + 8.0 * (a.B - a.rec_b0) * a.H * (double)a.rec_T * a.Nq;
    ProfScope ps(c, st, PC_ATTN_CROSS, fl, by);
    CK(launch_attention_long(a, st));
  } else CK(run_attention(c, st, PC_ATTN_CROSS, a));
  if (hook_call) {
    ProfScope ps(c, st, PC_HEAT, 0);
    CK(launch_hook_headmean(c->hook_headsb.as<float>(), c->hook_Bp, xl.heads, T, N, c->hook_scratch, st));
    if (c->rec_is_train) {
      // hook.py:110-112 `self.cross_attn_maps.append(maps)`: training reads every per-call map (finetune_sd_token.py:1043-1045),
      // so they are kept (device memory, grown geometrically, earlier maps carried over)
      const size_t bytes = (size_t)c->hook_Bp * T * N * 4, need = c->hook_store_used + bytes;
      if (need > c->hook_storeb.cap) {
        DBuf bigger; CK(bigger.ensure(need * 2 > ((size_t)64 << 20) ? need * 2 : ((size_t)64 << 20)));
        if (c->hook_store_used && hipMemcpyAsync(bigger.p, c->hook_storeb.p, c->hook_store_used, hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("hook store copy");
        hipStreamSynchronize(st);
        c->hook_storeb.release(); c->hook_storeb = bigger;
      }
      if (hipMemcpyAsync((char*)c->hook_storeb.p + c->hook_store_used, c->hook_scratch, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("hook store");
      c->hook_recs.push_back({c->hook_store_used, c->hook_Bp, T, N});
      c->hook_store_used = need;
    }
    CK(launch_hook_accum(c->hook_scratch, c->hook_Bp, T, side, c->rec_L, c->hook_sum, st));
    c->hook_count++;
  }
  return 0;
}

// GLIGEN's GatedSelfAttentionDense on the B x HW rows of h, in place:  h += tanh(alpha_attn) to_out(attn(norm1(h) | grounding K/V));
// h += tanh(alpha_dense) ff.net.2(GEGLU(norm2(h))).  The attention is attention.hip's second-K/V-source form: the HW visual keys of the image,
// then its max_objs grounding keys (norm1 and K/V of the objects were computed once per call) as one extra masked tile.  Both gates go on
// the GEMM accumulators (alpha) with the biases pre-scaled, the residual operand = h.  qkv [B HW][3C] and att [B HW][C] are the caller's
// scratch; last(A, K, w, o) runs the gated ff.net.2 launch (transformer(): the GEMM that also leaves norm2's row statistics).
static int fuser_rows(agd_ctx* c, hipStream_t st, const Fuser& f, bf16_t* h, int B, int HW, bf16_t* qkv, bf16_t* att,
                      const std::function<int(const bf16_t*, int, const WMat&, const GemmOpt&)>& last) {
  const int C = f.C, D = C / f.heads, M = B * HW, NO = c->glc.max_objs;
  if (B != c->gl_B2) FAIL("gligen: the grounding objects are set for %d rows, this forward has %d (agd_gligen_set)", c->gl_B2, B);
  const std::string t = f.pre + "transformer_blocks.0.fuser.";
  bf16_t* n = (bf16_t*)c->arena.alloc((size_t)M * C * 2); bf16_t* ff = (bf16_t*)c->arena.alloc((size_t)M * 4 * C * 2);
  if (!n || !ff) return -1;
  GETV(g1, t + "norm1.weight"); GETV(b1, t + "norm1.bias"); GETV(g2, t + "norm2.weight"); GETV(b2, t + "norm2.bias");
  GETW(wo, t + "attn.to_out.0.weight"); GETW(w1, t + "ff.net.0.proj.weight"); GETV(bb1, t + "ff.net.0.proj.bias"); GETW(w2, t + "ff.net.2.weight");
  { ProfScope ps(c, st, PC_LN, 0, 4.0 * M * (double)C); CK(launch_layernorm(h, n, g1, b1, M, C, 1e-5f, st)); }
  { GemmOpt o; CK(run_conv(c, st, n, C, nullptr, 0, 1, 1, M, f.wqkv, 1, qkv, o, c->zero_page)); }
  AttnP a{}; a.q = qkv; a.k = qkv + C; a.v = qkv + 2 * C; a.o = att;
  a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C; a.sq = a.sk = a.sv = (long long)HW * 3 * C; a.so = (long long)HW * C;
  a.B = B; a.H = f.heads; a.D = D; a.Nq = HW; a.Nk = HW; a.scale = 1.0f / sqrtf((float)D);
  a.k2 = f.gkvb.as<bf16_t>(); a.v2 = a.k2 + C; a.ldk2 = a.ldv2 = 2 * C; a.sk2 = a.sv2 = (long long)NO * 2 * C; a.Nk2 = NO;
  { const double fl = 4.0 * B * f.heads * (double)HW * (HW + NO) * D, by = 2.0 * B * (double)C * (4.0 * HW + 2.0 * NO);
    ProfScope ps(c, st, PC_ATTN_SELF, fl, by); CK(launch_attention(a, st)); }
  { GemmOpt o; o.bias = f.bo_s; o.alpha = f.ta; o.residual = h; CK(run_conv(c, st, att, C, nullptr, 0, 1, 1, M, *wo, 1, h, o, c->zero_page)); }
  { ProfScope ps(c, st, PC_LN, 0, 4.0 * M * (double)C); CK(launch_layernorm(h, n, g2, b2, M, C, 1e-5f, st)); }
  { GemmOpt o; o.bias = bb1; o.geglu = 1; CK(run_conv(c, st, n, C, nullptr, 0, 1, 1, M, *w1, 1, ff, o, c->zero_page)); }
  GemmOpt o; o.bias = f.b2_s; o.alpha = f.td; o.residual = h;
  return last(ff, 4 * C, *w2, o);
}

// the second half of a [2B'] activation := its first half (CFG: both halves saw identical inputs so far)
static int dup_half(agd_ctx* c, hipStream_t st, bf16_t* p, long long half_elems) {
  ProfScope ps(c, st, PC_ELEM, 0);
  if (hipMemcpyAsync(p + half_elems, p, (size_t)half_elems * 2, hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("dup_half copy failed");
  return 0;
}

// Transformer2DModel with one BasicTransformerBlock: transformer() allocates, tblock_plan() decides which form every stage takes,
// the tb_*() stages launch what the plan says and decide nothing themselves
enum TbHead  { HEAD_GN,            // GroupNorm pass (or the producing resnet's normalised copy), proj_in GEMM
               HEAD_FOLD,          // fold launch (the GroupNorm into per-image proj_in matrices), proj_in GEMM on the raw x
               HEAD_QKV,           // fold launch, then proj_in -> h -> norm1 -> q / k / v in one launch (the qkv chain, tblock.hip)
               HEAD_QKV_GN };      // the qkv chain alone, applying the GroupNorm itself (C = 320; C = 640 under TBF_QKV_640)
enum TbDup   { DUP_NONE, DUP_COPY,   // copy launches behind attn1.to_out
               DUP_LAZY };         // inside the fused kernels (the chain reads input row m % M', the feed-forward's proj_out stage adds block-input row m % M')
enum TbAttn2 { ATTN2_CHAIN,        // norm2 -> to_q -> attention (+ DAAM record) -> to_out + residual in one launch (tblock.hip)
               ATTN2_PREMUL,       // the C = 1280 blocks: S GEMM + softmax + recorder, then the output GEMM, against per-image pre-multiplied context matrices (xattn_pre.hip)
               ATTN2_KERNELS };    // to_q, cross_attention() (the processor seam), to_out
enum TbFf    { FF_FUSED,           // norm3 (folded) -> GEGLU -> ff.net.2 + residual in one launch, the 4C-wide hidden activation stays in LDS (tblock.hip); proj_out a GEMM
               FF_FUSED_PROJ,      // ... with proj_out + residual (+ the next GroupNorm's partial sums) behind it, same launch
               FF_FUSED_PREMUL,    // ... with ff.net.2 and proj_out pre-multiplied (as FF_FFPROJ does for the other blocks): no intermediate h3
               FF_FFPROJ,          // GEGLU GEMM, then ff.net.2 and proj_out as ONE GEMM (opt "ff_proj_fuse")
               FF_PLAIN };         // GEGLU, ff.net.2 and proj_out GEMMs

struct TBlockPlan {
  // LayerNorm folded into the GEMMs around it (opt "ln_fold"): the GEMM that writes h also emits per-row (sum, sum of squares) of its bf16
  // outputs per N tile; the GEMM that would read LayerNorm(h) reads h itself with W diag(gamma) and finishes  rstd (acc - mean colsum) +
  // (bias + W beta)  in its epilogue.  The three LayerNorm launches (and their read + write of the activation) per block disappear; h is
  // still rounded to bf16 exactly once.
  bool fold;
  bool x_normed;                   // the producing resnet's slab pass already applied this block's GroupNorm (x.normed)
  bool gfold;                      // the GroupNorm goes into per-image proj_in matrices: every head but HEAD_GN and C = 640's HEAD_QKV_GN
  TbHead head; int qkv_rows64, qkv_sched2;      // (QkvChainP::rows64 / sched2)
  bool attn1_in_chain;             // attn1.to_out + residual run inside the attn2 chain launch, not as a GEMM of their own
  TbDup dup;
  const Fuser* fuser;              // GLIGEN: this evaluation runs the block's fuser (between the duplication and attn2)
  const IpaLayer* ipa;             // IP-Adapter: this forward runs the block's image branch (scores on attn2's input, the add on its output)
  XLayer* xl;                      // the block's attn2 layer (null: not registered -- the attn2 stage refuses)
  TbAttn2 attn2; int chain_rows32;              // (AttnChainP::rows32)
  bool daam;                       // attn2 records into the DAAM accumulators (the chain and pre-multiplied forms; cross_attention() asks daam_records() itself)
  TbFf ff;
  bool wreg_proj;                  // proj_in / proj_out GEMMs through the weight-streaming kernel (opt "wreg_mask" bit 1)
  // the GEMM that writes h leaves the row statistics its reader folds a LayerNorm with: proj_in for norm1; attn1.to_out, or the fuser's last
  // GEMM, for norm2 (the attn2 chain takes its own); attn2's last launch for norm3 (the fused feed-forward takes its own)
  bool stats_head, stats_attn1, stats_attn2;
  bool stats_ipa;                  // IP-Adapter: the add stage takes norm3's statistics from the rows (in place of stats_attn2)
  // Not here, because they shape one launch and choose no path: consume()'s weight-streaming form of the C = 1280 GEGLU (opt "wreg_mask" bit 0,
  // by M) and the fused feed-forward's partial sums for the next GroupNorm (where `out` has room for them)
};

static const float kTbLnEps = 1e-5f;

// one block's walk: its inputs, its buffers and where the residual stream stands
struct TBlock {
  agd_ctx* c; hipStream_t st; const std::string& pre; const std::string t; const Act& x; Act& out; int heads, groups;
  int C, HW, Bs, B;                 // Bs: batch of the shared part (B / 2 under dup)
  const float* gn_g = nullptr; const float* gn_b = nullptr; const WMat* w_in = nullptr; const float* b_in = nullptr;     // norm, proj_in
  bf16_t* ln = nullptr;             // [M][C] normalised rows: the GroupNorm's output, then the unfolded LayerNorms'
  bf16_t* h = nullptr; bf16_t* qkv = nullptr; bf16_t* att = nullptr;
  const bf16_t* xres;               // residual of proj_out
  int M; const int Mshared;         // rows until the duplication point (Mshared), B * HW after it
  float* stats = nullptr; int slots = 0;        // row statistics of the current h
  bf16_t* ipaP = nullptr;           // IP-Adapter: the image branch's probabilities [M][cols] between its two stages
  TBlock(agd_ctx* c_, hipStream_t st_, const std::string& pre_, const Act& x_, Act& out_, int heads_, int groups_, int dup)
    : c(c_), st(st_), pre(pre_), t(pre_ + "transformer_blocks.0."), x(x_), out(out_), heads(heads_), groups(groups_), C(x_.C), HW(x_.H * x_.W),
      Bs(x_.B), B(dup ? 2 * x_.B : x_.B), xres(x_.p), M(x_.B * x_.H * x_.W), Mshared(M) {}

  // h = A . W^T (+ bias, + residual), and with want_stats its row statistics
  // (shaped: launched as [images][H][W] instead of one row of M pixels -- the per-image forms of the epilogue need the image of a row)
  int produce(const bf16_t* A, int K, const WMat& w, GemmOpt o, bool shaped, bool want_stats) {
    const int gb_ = shaped ? M / HW : 1, gh_ = shaped ? x.H : 1, gw_ = shaped ? x.W : M;
    stats = nullptr; slots = 0;
    if (want_stats) {
      int cfg[3] = {0, 0, 0}; GemmOpt qo = o; qo.query_cfg = cfg; qo.want_rowstat = 1;
      CK(run_conv(c, st, A, K, nullptr, 0, gb_, gh_, gw_, w, 1, h, qo, c->zero_page));
      slots = (w.N + cfg[1] - 1) / cfg[1];
      stats = (float*)c->arena.alloc((size_t)B * HW * slots * 2 * sizeof(float)); if (!stats) return -1;   // B*HW rows: room for the CFG duplicate
      o.rowstat_out = stats; o.rowstat_slots = slots;
    }
    return run_conv(c, st, A, K, nullptr, 0, gb_, gh_, gw_, w, 1, h, o, c->zero_page);
  }
  // outp = LayerNorm(h) . W^T (+ bias) [GEGLU]: folded, or the LayerNorm kernel followed by the plain GEMM
  int consume(bool fold, const std::string& lnkey, const std::string& wkey, const float* bias, int geglu, bf16_t* outp) {
    if (fold) {
      const std::string k = wkey + ".lnfold";
      GETW(wf, k); GETV(cs, k + ".cs"); GETV(bf, k + ".bias");
      GemmOpt o; o.bias = bf; o.geglu = geglu; o.ln_stats = stats; o.ln_slots = slots; o.ln_cs = cs; o.ln_invC = 1.0f / (float)C; o.ln_eps = kTbLnEps;
      if (geglu && C == 1280 && M >= 1024 && M <= 4096 && (c->opt_wreg & 1) && wf->wfrag) o.wreg = 2;
      return run_conv(c, st, h, C, nullptr, 0, 1, 1, M, *wf, 1, outp, o, c->zero_page);
    }
    GETV(g, lnkey + ".weight"); GETV(b, lnkey + ".bias");
    { ProfScope ps(c, st, PC_LN, 0, 4.0 * M * (double)C); CK(launch_layernorm(h, ln, g, b, M, C, kTbLnEps, st)); }
    GETW(w, wkey); GemmOpt o; o.bias = bias; o.geglu = geglu;
    return run_conv(c, st, ln, C, nullptr, 0, 1, 1, M, *w, 1, outp, o, c->zero_page);
  }
};

// dup != 0 (first transformer of a CFG forward, agd_denoise only): x holds B' = batch/2 images whose unconditional and
// conditional rows are still IDENTICAL (same latents, same timestep; the text context enters at attn2).  GroupNorm,
// proj_in, norm1 and the self-attention run once on B' rows; the result is duplicated right before the first
// cross-attention and the block returns 2B' rows.  Bit-identical to running both halves (every op here is
// row- or image-local), at half the cost for the most expensive attention call of the forward.
// GLIGEN (c->cur.grounded, a UNet block with a fuser): the fuser runs between attn1's residual add and attn2.  The CFG halves diverge there
// (the unconditional half sees null objects only), so the shared prefix is duplicated BEFORE the fuser (DUP_COPY) and attn1.to_out stays a
// GEMM of its own.  norm2's statistics for whatever attn2 form follows come from the fuser's last GEMM (the gated ff.net.2 is a produce()
// launch).  Evaluations without the flag take the same plan as a model without fusers.
static TBlockPlan tblock_plan(const TBlock& s, int dup) {
  agd_ctx* c = s.c; const Act& x = s.x; const std::string& pre = s.pre; const std::string& t = s.t;
  const int C = s.C, HW = s.HW, heads = s.heads, groups = s.groups;
  auto tb = [c](int bit) { return (c->opt_tb_fuse & bit) != 0; };
  auto has = [c](const std::string& key) { return c->W.count(key) != 0; };
  TBlockPlan p{};
  p.fold = c->opt_ln_fold == 1 || (c->opt_ln_fold == 2 && C <= 320) || (c->opt_ln_fold == 3 && C <= 640);
  p.x_normed = x.normed && x.normed_gamma == s.gn_g;
  p.wreg_proj = C == 640 && (c->opt_wreg & 2);
  // --- head ---
  // The transformer's GroupNorm has no activation behind it: where the producer of x left its per-tile channel sums, the norm is folded
  // into per-image proj_in matrices (norm.hip gn_fold_weight_kernel) and proj_in reads the raw x -- no read + write of the activation by
  // a GroupNorm kernel.  Default C <= 320 (the 64 x 64 maps: the fold launch takes 8.5 us against the 17 us apply pass; in situ 522.4 -> 521.3 ms
  // per batch, tools/ab_option.py); at C = 640 the fold (16.8 us, 6.5 MB of matrices) costs more than the 10.8 us pass it replaces.
  const bool sums = c->opt_gn_fused && x.cpart && x.cpart_bm > 0 && HW % x.cpart_bm == 0;
  p.gfold = c->opt_gn_proj_fold && sums && C <= (c->opt_gn_proj_fold >= 2 ? 640 : 320) && HW % 128 == 0;
  if (p.gfold) {
    const bool qkv = tb(TBF_QKV) && C == 320 && s.w_in->N == C && has(t + "attn1.qkv.frag");
    // the chain takes the GroupNorm's statistics from the partial sums and normalises the rows in its LDS panel: no fold launch either
    const bool gn_inside = qkv && tb(TBF_QKV_GN) && groups <= 32 && has(pre + "proj_in.frag");
    p.head = gn_inside ? HEAD_QKV_GN : qkv ? HEAD_QKV : HEAD_FOLD;
    p.qkv_rows64 = qkv && tb(TBF_QKV_ROWS64) && HW % 64 == 0;
  } else if (C == 640 && tb(TBF_QKV) && tb(TBF_QKV_640) && tb(TBF_QKV_GN) && sums && HW % 64 == 0 && groups <= 32 && !p.x_normed && !dup &&
             has(pre + "proj_in.frag") && has(t + "attn1.qkv.frag")) {
    // C = 640 (the 32 x 32 maps): no fold, the chain takes the raw rows (measured 71 us against 65 for the three launches it replaces --
    // 128 workgroups each streaming 3.3 MB of weights)
    p.head = HEAD_QKV_GN;
  } else p.head = HEAD_GN;
  p.qkv_sched2 = tb(TBF_QKV_SCHED2);
  // --- feed-forward: the row-panel kernel where its shape is built (C = 320) ---
  const bool ff_fused = tb(TBF_FF) && p.fold && C == 320 && has(t + "ff.w1.frag");
  if (ff_fused) {
    const bool proj = tb(TBF_FF_PROJ) && has(pre + "proj_out.frag");
    p.ff = !proj ? FF_FUSED : tb(TBF_FF_PREMUL) && has(t + "ff.w2p.frag") ? FF_FUSED_PREMUL : FF_FUSED_PROJ;
  } else p.ff = c->opt_ffproj && has(pre + "ffproj.weight") ? FF_FFPROJ : FF_PLAIN;
  // --- attn2: the pre-multiplied form where agd_set_context built its products; the chain steps aside exactly there.  The chain's shape: 8 heads,
  // <= 96 keys, whole 128-row (C = 640: 64-row) tiles per image.  The hook.py recorder (per-head maps of every call) keeps the kernels. ---
  auto itx = c->xl_idx.find(t + "attn2");
  p.xl = itx == c->xl_idx.end() ? nullptr : &c->xl[itx->second];
  p.daam = p.xl && daam_records(c, *p.xl, s.B, x.H, x.W);
  const bool premul = p.xl && p.xl->pm_ready && c->opt_xpre && p.fold && HW % 64 == 0 && c->rec_mode != 2 && c->ctx_T <= XATTN_TP && !dup &&
                      (!p.daam || p.xl->acc_heads == p.xl->heads);
  const bool chain = !premul && tb(TBF_ATTN2) && (C == 320 || (C == 640 && tb(TBF_ATTN2_640))) && heads == 8 && HW % (C == 320 ? 128 : 64) == 0 &&
                     c->ctx_T <= 96 && c->rec_mode != 2 && has(t + "attn2.to_q.frag");
  p.attn2 = premul ? ATTN2_PREMUL : chain ? ATTN2_CHAIN : ATTN2_KERNELS;
  p.chain_rows32 = tb(TBF_ATTN2_ROWS32);
  // --- between them: the duplication of the CFG-shared prefix, the fuser, and where attn1.to_out runs ---
  if (c->cur.grounded) { auto itf = c->gl_idx.find(pre); if (itf != c->gl_idx.end()) p.fuser = &c->gl_f[itf->second]; }
  if (c->cur.ipa) { auto iti = c->ipa_idx.find(pre); if (iti != c->ipa_idx.end()) p.ipa = &c->ipa_l[iti->second]; }
  const bool lazy = dup && tb(TBF_LAZY_DUP) && chain && C == 320 && (p.ff == FF_FUSED_PROJ || p.ff == FF_FUSED_PREMUL) && !p.fuser && !p.ipa;
  p.dup = !dup ? DUP_NONE : lazy ? DUP_LAZY : DUP_COPY;
  p.attn1_in_chain = chain && tb(TBF_ATTN1_OUT) && p.dup != DUP_COPY && has(t + "attn1.to_out.frag") && !p.fuser && !p.ipa;
  // (with the image branch the add stage takes norm3's statistics itself, from the rows as they are after the add: attn2's last launch leaves none)
  p.stats_head = p.fold; p.stats_attn1 = p.fold && !chain; p.stats_attn2 = p.fold && !ff_fused && !p.ipa; p.stats_ipa = p.fold && !ff_fused && p.ipa;
  return p;
}

// IP-Adapter (c->cur.ipa, a UNet block): the image branch reads attn2's INPUT rows, so -- as with the fuser -- that input must exist in
// memory with all B rows: attn1.to_out stays a GEMM of its own and a CFG-shared prefix is duplicated by copies.  Whatever attn2 form the plan
// picked then runs unchanged and in place, and the add lands on its output.  norm3's row statistics must describe h AFTER the add, so attn2's
// last launch leaves none (stats_attn2 off) and tb_ip_adapter_add takes them from the rows (stats_ipa: one slot, launch_rowstat_bf16).
// launch parameters of the qkv chain; wb / radd: the fold launch's per-image matrices and rows (HEAD_QKV)
static int qkv_chain_params(const TBlock& s, const TBlockPlan& p, const bf16_t* wb, const float* radd, QkvChainP& qp) {
  agd_ctx* c = s.c; const Act& x = s.x; const int C = s.C;
  GETW(fqkv, s.t + "attn1.qkv.frag"); GETV(g1, s.t + "norm1.weight"); GETV(b1, s.t + "norm1.bias");
  qp.x = x.p; qp.wbf = wb; qp.wb_stride = (long long)s.w_in->N * C; qp.rowadd = radd; qp.rowadd_stride = C; qp.h = s.h; qp.gamma = g1; qp.beta = b1; qp.ln_eps = kTbLnEps;
  qp.wqkvf = fqkv->w; qp.qkv = s.qkv; qp.M = s.M; qp.HW = s.HW; qp.rows64 = p.qkv_rows64; qp.sched2 = p.qkv_sched2;
  if (p.head == HEAD_QKV_GN) {
    GETW(fpi, s.pre + "proj_in.frag");
    if (!s.b_in) FAIL("proj_in without bias");
    qp.wbf = fpi->w; qp.wb_stride = 0; qp.rowadd = s.b_in; qp.rowadd_stride = 0;
    qp.gn_part = x.cpart; qp.gn_bm = x.cpart_bm; qp.gn_groups = s.groups; qp.gn_eps = 1e-6f; qp.gn_gamma = s.gn_g; qp.gn_beta = s.gn_b;
  }
  return 0;
}

// GroupNorm + proj_in -> h (HEAD_QKV / HEAD_QKV_GN: + norm1 and attn1's q / k / v)
static int tb_head(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c; hipStream_t st = s.st; const Act& x = s.x; const WMat* w = s.w_in; const int C = s.C;
  if (p.head == HEAD_GN) {
    if (p.x_normed) s.ln = x.normed;
    else CK(run_gn(c, st, x.p, C, nullptr, 0, s.Bs, s.HW, s.gn_g, s.gn_b, s.groups, 1e-6f, 0, s.ln, &x));
    GemmOpt o; o.bias = s.b_in;
    if (p.wreg_proj) o.wreg = 1;
    return s.produce(s.ln, C, *w, o, false, p.stats_head);
  }
  if (p.gfold) { if (w->taps != 1 || w->Cpad != C) FAIL("gn_proj_fold: proj_in weight [N=%d taps=%d Cpad=%d] is not a 1x1 over %d channels", w->N, w->taps, w->Cpad, C); }
  else if (w->taps != 1 || w->Cpad != C || w->N != C || !s.b_in) FAIL("qkv chain: proj_in weight [N=%d taps=%d Cpad=%d] is not a biased 1x1 over %d channels", w->N, w->taps, w->Cpad, C);
  bf16_t* wb = nullptr; float* radd = nullptr;
  if (p.head != HEAD_QKV_GN) {
    wb = (bf16_t*)c->arena.alloc((size_t)s.Bs * w->N * C * 2);
    radd = (float*)c->arena.alloc((size_t)s.Bs * w->N * sizeof(float));
    if (!wb || !radd) return -1;
    ProfScope ps(c, st, PC_GN, 0, 2.0 * s.Bs * (double)w->N * C * 2);
    CK(launch_gn_fold_weight(x.cpart, x.cpart_bm, s.Bs, s.HW, C, s.groups, 1e-6f, s.gn_g, s.gn_b, w->w, s.b_in, w->N, wb, radd, st, p.head == HEAD_QKV ? C / 64 : 0));
  }
  if (p.head == HEAD_FOLD) {
    WMat wi = *w; wi.w = wb;
    GemmOpt o; o.rowadd = radd; o.rowadd_ld = w->N; o.w_per_image = 1;
    return s.produce(x.p, C, wi, o, true, p.stats_head);
  }
  QkvChainP qp{}; CK(qkv_chain_params(s, p, wb, radd, qp));
  s.stats = nullptr; s.slots = 0;                        // norm1's statistics come from the rows themselves
  ProfScope ps(c, st, PC_GEMM, 8.0 * s.M * (double)C * C, 2.0 * s.M * (double)C * 5.0 + 2.0 * (p.gfold ? s.Bs + 3.0 : 4.0) * C * (double)C);
  return launch_qkv_chain(qp, C, st);
}

static int tb_self_attention(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c; const std::string& t = s.t; const int C = s.C, HW = s.HW, D = C / s.heads;
  if (p.head == HEAD_GN || p.head == HEAD_FOLD) CK(s.consume(p.fold, t + "norm1", t + "attn1.qkv", nullptr, 0, s.qkv));
  AttnP a{}; a.q = s.qkv; a.k = s.qkv + C; a.v = s.qkv + 2 * C; a.o = s.att;
  a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C; a.sq = a.sk = a.sv = (long long)HW * 3 * C; a.so = (long long)HW * C;
  a.B = s.Bs; a.H = s.heads; a.D = D; a.Nq = HW; a.Nk = HW; a.scale = 1.0f / sqrtf((float)D);
  if (c->cur.pag && c->pag_layers.count(s.pre)) {          // the perturbed branch: the attention map is the identity, the output is the value rows
    const double M = (double)s.Bs * HW;
    ProfScope ps(c, s.st, PC_ELEM, 0, 4.0 * M * C);
    CK(launch_pag_v_rows(s.qkv, s.att, s.Bs * HW, C, s.st));
    c->pag_counts[1]++;
  } else CK(run_attention(c, s.st, PC_ATTN_SELF, a));
  if (p.attn1_in_chain) return 0;
  GETW(wo, t + "attn1.to_out.0.weight"); GETV(bo, t + "attn1.to_out.0.bias");
  GemmOpt oo; oo.bias = bo; oo.residual = s.h;
  return s.produce(s.att, C, *wo, oo, false, p.stats_attn1);
}

// the halves of a CFG-shared prefix diverge from here on (text context)
static int tb_duplicate(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c; hipStream_t st = s.st; const int C = s.C, M = s.Mshared;
  if (p.dup == DUP_NONE) return 0;
  s.M = s.B * s.HW;
  if (p.dup == DUP_LAZY) return 0;
  CK(dup_half(c, st, s.h, (long long)M * C));
  if (p.stats_attn1) { ProfScope ps(c, st, PC_ELEM, 0);
    if (hipMemcpyAsync(s.stats + (size_t)M * s.slots * 2, s.stats, (size_t)M * s.slots * 2 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("dup stats copy failed"); }
  Act x2 = alloc_act(c, s.B, s.x.H, s.x.W, C); if (!x2.p) return -1;
  { ProfScope ps(c, st, PC_ELEM, 0);
    if (hipMemcpyAsync(x2.p, s.x.p, (size_t)M * C * 2, hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("dup copy failed"); }
  CK(dup_half(c, st, x2.p, (long long)M * C));
  s.xres = x2.p;
  return 0;
}

static int tb_fuser(TBlock& s, const TBlockPlan& p) {
  return fuser_rows(s.c, s.st, *p.fuser, s.h, s.B, s.HW, s.qkv, s.att,
                    [&](const bf16_t* A, int K, const WMat& w, const GemmOpt& o) { return s.produce(A, K, w, o, false, p.stats_attn1); });
}

// the two IP-Adapter stages on B images of HW rows (transformer() and agd_ip_adapter_block)
static int ipa_scores_rows(agd_ctx* c, hipStream_t st, const IpaLayer& l, const bf16_t* h, int B, int HW, bf16_t* P) {
  if (B != c->ipa_B2) FAIL("ip_adapter: the image tokens are set for %d rows, this forward has %d (agd_ip_adapter_set)", c->ipa_B2, B);
  IpaScoreP sp{}; sp.h = h; sp.kpp = l.kppb.as<bf16_t>(); sp.cs = l.csbsb.as<float>(); sp.bs = sp.cs + (size_t)B * l.cols; sp.P = P;
  sp.B = B; sp.HW = HW; sp.C = l.C; sp.H = l.heads; sp.nt = c->ipa_nt; sp.colsP = l.cols; sp.eps = 1e-5f;
  const double M = (double)B * HW;
  ProfScope ps(c, st, PC_ATTN_CROSS, 2.0 * M * l.cols * l.C, 2.0 * M * l.C + 2.0 * B * (double)l.cols * l.C + 2.0 * M * l.cols);
  return launch_ipa_scores(sp, st);
}
static int ipa_add_rows(agd_ctx* c, hipStream_t st, const IpaLayer& l, bf16_t* h, int B, int HW, const bf16_t* P) {
  IpaAddP ap{}; ap.h = h; ap.P = P; ap.vpp = l.vppb.as<bf16_t>(); ap.B = B; ap.HW = HW; ap.C = l.C; ap.colsP = l.cols; ap.s = c->ipa_scale;
  const double M = (double)B * HW;
  ProfScope ps(c, st, PC_ATTN_CROSS, 2.0 * M * l.cols * l.C, 4.0 * M * l.C + 2.0 * B * (double)l.cols * l.C + 2.0 * M * l.cols);
  return launch_ipa_add(ap, st);
}
static int tb_ip_adapter_scores(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c;
  if (s.C != p.ipa->C) FAIL("ip_adapter: %s has %d channels, its to_k_ip / to_v_ip were loaded for %d", s.pre.c_str(), s.C, p.ipa->C);
  s.ipaP = (bf16_t*)c->arena.alloc((size_t)s.M * p.ipa->cols * 2); if (!s.ipaP) return -1;
  CK(ipa_scores_rows(c, s.st, *p.ipa, s.h, s.B, s.HW, s.ipaP));
  c->ipa_counts[0]++;
  return 0;
}
static int tb_ip_adapter_add(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c;
  CK(ipa_add_rows(c, s.st, *p.ipa, s.h, s.B, s.HW, s.ipaP));
  c->ipa_counts[1]++;
  if (p.stats_ipa) {                                     // norm3's folded consumer reads statistics of the rows as they are NOW
    s.slots = 1; s.stats = (float*)c->arena.alloc((size_t)s.M * 2 * sizeof(float)); if (!s.stats) return -1;
    ProfScope ps(c, s.st, PC_LN, 0, 2.0 * s.M * (double)s.C);
    CK(launch_rowstat_bf16(s.h, s.stats, s.M, s.C, s.st));
  }
  return 0;
}

static int tb_attn2_chain(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c; const std::string& t = s.t; const XLayer& xl = *p.xl; const int C = s.C, HW = s.HW, B = s.B, M = s.M, heads = s.heads;
  GETW(fq, t + "attn2.to_q.frag"); GETW(fo, t + "attn2.to_out.frag");
  GETV(g2, t + "norm2.weight"); GETV(b2, t + "norm2.bias"); GETV(bo, t + "attn2.to_out.0.bias");
  const int T = c->ctx_T, D = C / heads;
  AttnChainP ap{}; ap.h = s.h; ap.out = s.h; ap.gamma = g2; ap.beta = b2; ap.ln_eps = kTbLnEps; ap.wqf = fq->w; ap.wof = fo->w; ap.bo = bo;
  ap.kv = xl.kv; ap.ldkv = 2 * C; ap.skv = (long long)T * 2 * C; ap.M = M; ap.HW = HW; ap.T = T; ap.scale = 1.0f / sqrtf((float)D);
  double rec_bytes = 0;
  if (p.daam) {
    ap.record = 1; ap.rec_b0 = B / 2; ap.rec_T = c->rec_T; ap.rec_hpb = heads / xl.acc_heads;
    ap.rec_head_stride = (long long)c->rec_T * HW; ap.rec_img_stride = ap.rec_head_stride * xl.acc_heads;
    ap.rec = xl.acc + (size_t)c->rec_base * ap.rec_img_stride;
    rec_bytes = 8.0 * (B - ap.rec_b0) * xl.acc_heads * (double)c->rec_T * HW;
  }
  if (p.attn1_in_chain || p.dup == DUP_LAZY) {           // the chain's input is not its output: the residual stream continues in a second buffer
    ap.out = (bf16_t*)c->arena.alloc((size_t)M * C * 2); if (!ap.out) return -1;
  }
  if (p.attn1_in_chain) {                                // h1 = attn1.to_out(att) + h is computed (and stored) by the chain itself
    GETW(f1o, t + "attn1.to_out.frag"); GETV(bo1, t + "attn1.to_out.0.bias");
    ap.o1 = s.att; ap.wo1f = f1o->w; ap.bo1 = bo1;
  }
  if (p.dup == DUP_LAZY) ap.src_rows = s.Mshared;
  ap.rows32 = p.chain_rows32;
  if (p.stats_attn2) {                                   // the GEGLU consumer of the LayerNorm fold reads one slot of row statistics
    s.slots = 1; s.stats = (float*)c->arena.alloc((size_t)M * 2 * sizeof(float)); if (!s.stats) return -1;
    ap.rowstat_out = s.stats;
  }
  const double gemms = p.attn1_in_chain ? 6.0 : 4.0;
  ProfScope ps(c, s.st, PC_ATTN_CROSS, gemms * M * (double)C * C + 4.0 * B * heads * (double)HW * T * D, gemms * M * (double)C + gemms * C * (double)C + 4.0 * B * (double)T * C + rec_bytes);
  CK(launch_attn_chain(ap, C, heads, s.st));
  s.h = ap.out;
  return 0;
}

static int tb_attn2_premul(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c; const XLayer& xl = *p.xl; const int C = s.C, HW = s.HW, B = s.B, M = s.M, heads = s.heads;
  if (!s.stats || s.slots <= 0) FAIL("attn2_premul: the GEMM in front of attn2 left no row statistics for norm2");
  GETV(bo, s.t + "attn2.to_out.0.bias");
  const int HT = heads * XATTN_TP;
  bf16_t* P = (bf16_t*)c->arena.alloc((size_t)M * HT * 2); if (!P) return -1;
  XattnSP sp{}; sp.x = s.h; sp.ln_stats = s.stats; sp.ln_slots = s.slots; sp.ln_invC = 1.0f / (float)C; sp.ln_eps = kTbLnEps;
  sp.kpp = xl.pm_kpp; sp.kcs = xl.pm_kcs; sp.kbs = xl.pm_kbs; sp.P = P; sp.M = M; sp.HW = HW; sp.C = C; sp.H = heads; sp.T = c->ctx_T;
  double rec_bytes = 0;
  if (p.daam) {
    sp.rec_b0 = B / 2; sp.rec_T = c->rec_T; sp.rec_head_stride = (long long)c->rec_T * HW; sp.rec_img_stride = sp.rec_head_stride * xl.acc_heads;
    sp.rec = xl.acc + (size_t)c->rec_base * sp.rec_img_stride;
    rec_bytes = 8.0 * (B - sp.rec_b0) * heads * (double)c->rec_T * HW;
  }
  { ProfScope ps(c, s.st, PC_ATTN_CROSS, 2.0 * M * (double)HT * C, 2.0 * M * (double)C + 2.0 * B * (double)HT * C + 2.0 * M * (double)HT + rec_bytes);
    CK(launch_xattn_s(sp, s.st)); }
  WMat wv; wv.w = xl.pm_vpp; wv.N = C; wv.Cin = HT; wv.Cpad = HT; wv.taps = 1;
  GemmOpt oo; oo.bias = bo; oo.residual = s.h; oo.w_per_image = 1;
  return s.produce(P, HT, wv, oo, true, p.stats_attn2);
}

static int tb_attn2(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c; const std::string& t = s.t;
  if (!p.xl) FAIL("cross-attn layer %s not registered", (t + "attn2").c_str());
  if (c->ctx_B2 != s.B) FAIL("context batch %d != unet batch %d (call agd_set_context)", c->ctx_B2, s.B);
  if (p.attn2 == ATTN2_CHAIN) return tb_attn2_chain(s, p);
  if (p.attn2 == ATTN2_PREMUL) return tb_attn2_premul(s, p);
  CK(s.consume(p.fold, t + "norm2", t + "attn2.to_q.weight", nullptr, 0, s.qkv));
  CK(cross_attention(c, s.st, *p.xl, s.qkv, s.B, s.HW, s.x.H, s.x.W, s.att, true));
  GETW(wo, t + "attn2.to_out.0.weight"); GETV(bo, t + "attn2.to_out.0.bias");
  GemmOpt oo; oo.bias = bo; oo.residual = s.h;
  return s.produce(s.att, s.C, *wo, oo, false, p.stats_attn2);
}

static int tb_ff_fused(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c; const std::string& t = s.t; Act& out = s.out; const int C = s.C, M = s.M;
  GETW(f1, t + "ff.w1.frag"); GETW(f2, t + "ff.w2.frag");
  const std::string k = t + "ff.net.0.proj.weight.lnfold";
  GETV(cs, k + ".cs"); GETV(bf, k + ".bias"); GETV(b2, t + "ff.net.2.bias");
  FFusedP fp{}; fp.h = s.h; fp.out = s.h; fp.w1f = f1->w; fp.cs1 = cs; fp.b1 = bf; fp.w2f = f2->w; fp.b2 = b2; fp.M = M; fp.ln_eps = kTbLnEps;
  const bool proj = p.ff != FF_FUSED;
  if (proj) {
    GETW(fpw, s.pre + "proj_out.frag"); GETV(bp, s.pre + "proj_out.bias");
    fp.wpf = fpw->w; fp.bp = bp; fp.xres = s.xres; fp.pout = out.p;
    if (p.ff == FF_FUSED_PREMUL) {
      GETW(f2p, t + "ff.w2p.frag"); GETV(bcp, s.pre + "ffproj.bias");
      fp.w2f = f2p->w; fp.bp = bcp; fp.premul = 1;
    }
    if (p.dup == DUP_LAZY) fp.xres_rows = s.Mshared;     // xres is still the B'-row block input
    out.cpart_bm = 0;
    if (out.cpart && c->opt_gn_fused && s.HW % 128 == 0) { fp.colstat = out.cpart; out.cpart_bm = 128; }
  }
  ProfScope ps(c, s.st, PC_GEMM, 2.0 * M * (double)C * (proj ? 13.0 : 12.0) * C, (proj ? 8.0 : 4.0) * M * (double)C + 2.0 * (proj ? 13.0 : 12.0) * C * (double)C);
  return launch_ff_fused(fp, C, s.st);
}

// GEGLU feed-forward and proj_out
static int tb_feed_forward(TBlock& s, const TBlockPlan& p) {
  agd_ctx* c = s.c; hipStream_t st = s.st; const std::string& t = s.t; const int C = s.C, M = s.M;
  if (p.ff == FF_FUSED || p.ff == FF_FUSED_PROJ || p.ff == FF_FUSED_PREMUL) CK(tb_ff_fused(s, p));
  else {
    bf16_t* ff = (bf16_t*)c->arena.alloc((size_t)M * 4 * C * 2); if (!ff) return -1;
    GETV(b1, t + "ff.net.0.proj.bias");
    CK(s.consume(p.fold, t + "norm3", t + "ff.net.0.proj.weight", b1, 1, ff));
    if (p.ff == FF_FFPROJ) {
      // proj_out(ff.net.2(g) + h) + x = [Wp W2 | Wp] . [g | h] + (Wp b2 + bp) + x: one launch over the channel concat of the hidden activation and the residual stream
      // with the matrix pre-multiplied at load time -- h3 is never formed, the proj_out launch (its 5 - 10 MB output pass and epilogue) disappears
      GETW(wc, s.pre + "ffproj.weight"); GETV(bc, s.pre + "ffproj.bias");
      GemmOpt o; o.bias = bc; o.residual = s.xres; o.out_act = &s.out; o.rows_per_image = s.HW;
      return run_conv(c, st, ff, 4 * C, s.h, C, 1, 1, M, *wc, 1, s.out.p, o, c->zero_page);
    }
    GETW(w2, t + "ff.net.2.weight"); GETV(b2, t + "ff.net.2.bias");
    GemmOpt o2; o2.bias = b2; o2.residual = s.h;
    CK(run_conv(c, st, ff, 4 * C, nullptr, 0, 1, 1, M, *w2, 1, s.h, o2, c->zero_page));
  }
  if (p.ff != FF_FUSED && p.ff != FF_PLAIN) return 0;    // proj_out ran inside the feed-forward's last launch
  GETW(w, s.pre + "proj_out.weight"); GETV(b, s.pre + "proj_out.bias");
  GemmOpt o; o.bias = b; o.residual = s.xres; o.out_act = &s.out; o.rows_per_image = s.HW;
  if (p.wreg_proj) o.wreg = 1;
  return run_conv(c, st, s.h, C, nullptr, 0, 1, 1, M, *w, 1, s.out.p, o, c->zero_page);
}

static int transformer(agd_ctx* c, hipStream_t st, const std::string& pre, const Act& x, int heads, int groups, Act& out, int dup = 0) {
  TBlock s(c, st, pre, x, out, heads, groups, dup);
  const int B = s.B, HW = s.HW, C = s.C;
  out = alloc_act(c, B, x.H, x.W, C, true); if (!out.p) return -1;
  const size_t mk = c->arena.mark();
  Act n = alloc_act(c, B, x.H, x.W, C); if (!n.p) return -1;
  Act h = alloc_act(c, B, x.H, x.W, C); if (!h.p) return -1;
  s.ln = n.p; s.h = h.p;
  s.qkv = (bf16_t*)c->arena.alloc((size_t)B * HW * 3 * C * 2); if (!s.qkv) return -1;
  s.att = (bf16_t*)c->arena.alloc((size_t)B * HW * C * 2); if (!s.att) return -1;
  GETV(gg, pre + "norm.weight"); GETV(gb, pre + "norm.bias"); GETW(w_in, pre + "proj_in.weight"); GETV(b_in, pre + "proj_in.bias");
  s.gn_g = gg; s.gn_b = gb; s.w_in = w_in; s.b_in = b_in;
  const TBlockPlan p = tblock_plan(s, dup);
  CK(tb_head(s, p));
  CK(tb_self_attention(s, p));
  CK(tb_duplicate(s, p));
  if (p.fuser) CK(tb_fuser(s, p));
  if (p.ipa) CK(tb_ip_adapter_scores(s, p));
  CK(tb_attn2(s, p));
  if (p.ipa) CK(tb_ip_adapter_add(s, p));
  CK(tb_feed_forward(s, p));
  c->arena.release(mk);
  return 0;
}

// time embeddings of n <= 25 timesteps (inference: one timestep serves every batch row); scratch = n * 9 * dim floats,
// out = [n][tproj_total]: every resnet's time_emb_proj(silu(temb)) from one stacked matrix
// cn: the ControlNet's own time_embedding and stacked time_emb_proj (out = [n][cn_tproj_total])
static int time_embed(agd_ctx* c, hipStream_t st, const float* ts, int n, float* scratch, float* out, bool cn = false) {
  const int dim = c->cfg.block_out_channels[0], td = dim * 4;
  const std::string pre = cn ? "controlnet." : "unet.";
  ProfScope ps(c, st, PC_ELEM, 0);
  float* e0 = scratch; float* e1 = e0 + (size_t)n * dim; float* e2 = e1 + (size_t)n * td;
  for (int i = 0; i < n; ++i) CK(launch_timestep_embed(ts[i], e0 + (size_t)i * dim, dim, st));
  GETW(w1, pre + "time_embedding.linear_1.weight"); GETV(b1, pre + "time_embedding.linear_1.bias");
  GETW(w2, pre + "time_embedding.linear_2.weight"); GETV(b2, pre + "time_embedding.linear_2.bias");
  CK(launch_small_linear(e0, w1->w, b1, e1, n, td, w1->Cpad, 0, 1, st));     // linear_1 + SiLU
  CK(launch_small_linear(e1, w2->w, b2, e2, n, td, w2->Cpad, 0, 0, st));     // linear_2 -> temb
  if (cn) CK(launch_small_linear(e2, c->cn_tproj_all.w, c->cn_tproj_bias, out, n, c->cn_tproj_total, td, 1, 0, st));
  else CK(launch_small_linear(e2, c->tproj_all.w, c->tproj_bias, out, n, c->tproj_total, td, 1, 0, st));
  return 0;
}

// conv_in, the down blocks and the mid block of a UNet-shaped model under the weight prefix u ("unet." or "controlnet."); on_sample(a) sees
// every res sample in order (conv_in, each resnet / transformer output, each downsampler: the UNet's skips); h = the mid block's output.
// conv_in_res: added in conv_in's epilogue (the ControlNet's conditioning embedding).  shared: rows [0,B2/2) and [B2/2,B2) of xin (and of
// conv_in_res) are identical -- everything ahead of the first attn2 runs on B2/2 rows.
// T2I-Adapter (the UNet's walk with c->cur.ad_scale != 0): after the last layer of level i and before on_sample sees it, h becomes h + ad_scale * feature i
// in a fresh activation (adapter_add) -- the sum is the level's last skip and the input of the downsampler / the mid block.
static int adapter_add(agd_ctx* c, hipStream_t st, int level, const Act& h, Act& out);
static int down_mid_walk(agd_ctx* c, hipStream_t st, const std::string& u, const bf16_t* xin, int B2, int Lh, int Lw, bool shared,
                         const bf16_t* conv_in_res, const std::function<int(const Act&)>& on_sample, Act& h, int stop_layer = -1) {
  const agd_config& g = c->cfg;
  const int nl = g.n_levels, G = g.norm_num_groups;
  const int Bh = shared ? B2 / 2 : B2;
  const bool inject = c->cur.ad_scale != 0.f && u == "unet.";
  h = alloc_act(c, B2, Lh, Lw, g.block_out_channels[0], true); if (!h.p) return -1;
  { GETW(w, u + "conv_in.weight"); GETV(b, u + "conv_in.bias"); GemmOpt o; o.bias = b; o.out_act = &h; o.residual = conv_in_res;
    CK(run_conv(c, st, xin, 64, nullptr, 0, Bh, Lh, Lw, *w, 3, h.p, o, c->zero_page)); }
  if (shared) {                                                             // the skip connection needs all B2 rows (and their partial sums)
    CK(dup_half(c, st, h.p, (long long)Bh * Lh * Lw * h.C));
    if (h.cpart_bm > 0) {
      const size_t nb = (size_t)((long long)Bh * Lh * Lw / h.cpart_bm) * h.C * 2 * sizeof(float);
      if (hipMemcpyAsync((char*)h.cpart + nb, h.cpart, nb, hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("dup partials copy failed");
    }
  }
  CK(on_sample(h));
  for (int i = 0; i < nl; ++i) {
    const int co = g.block_out_channels[i];
    for (int j = 0; j < g.layers_per_block; ++j) {
      const bool first = shared && i == 0 && j == 0;
      const bool add_here = inject && j + 1 == g.layers_per_block;       // the adapter's feature i lands on this layer's output
      Act hin = h; if (first) hin.B = Bh;
      // the GroupNorm that reads this resnet's output alone: the block's transformer, the next resnet of an attention-free level, or mid_block
      NextGn ng; std::string nk; 
      if (g.down_cross[i]) { nk = u + "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".norm."; ng.eps = 1e-6f; ng.silu = 0; }
      else if (j + 1 < g.layers_per_block) { nk = u + "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j + 1) + ".norm1."; ng.eps = 1e-5f; ng.silu = 1; }
      else if (i == nl - 1) { nk = u + "mid_block.resnets.0.norm1."; ng.eps = 1e-5f; ng.silu = 1; }
      if (!nk.empty()) { auto ig = c->V.find(nk + "weight"), ib = c->V.find(nk + "bias"); if (ig != c->V.end() && ib != c->V.end()) { ng.gamma = ig->second; ng.beta = ib->second; } }
      // (no NextGn where the add follows the resnet directly -- the attention-free level: a normalised copy of the un-added tensor would be stale)
      const bool no_ng = first || (add_here && !g.down_cross[i]);
      Act r; CK(resnet(c, st, u + "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".", hin, nullptr, co, 1e-5f, true, G, r, no_ng ? nullptr : &ng));
      h = r;
      if (g.down_cross[i]) {
        Act a; CK(transformer(c, st, u + "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", h, g.num_heads[i], G, a, first ? 1 : 0));
        h = a;
      }
      if (add_here) { Act s; CK(adapter_add(c, st, i, h, s)); h = s; }
      CK(on_sample(h));
      if (i == 0 && j == stop_layer) return 0;                             // DeepCache's shallow walk: s_0 .. s_{b+1} exist, nothing deeper runs
    }
    if (i != nl - 1) {
      const std::string k = u + "down_blocks." + std::to_string(i) + ".downsamplers.0.conv.";
      GETW(w, k + "weight"); GETV(b, k + "bias");
      Act d = alloc_act(c, B2, h.H / 2, h.W / 2, co, true); if (!d.p) return -1;
      GemmOpt o; o.bias = b; o.stride = 2; o.out_act = &d;
      CK(run_conv(c, st, h.p, co, nullptr, 0, B2, h.H, h.W, *w, 3, d.p, o, c->zero_page));
      h = d; CK(on_sample(h));
    }
  }
  { const int cm = g.block_out_channels[nl - 1];
    NextGn ngm; { auto ig = c->V.find(u + "mid_block.attentions.0.norm.weight"), ib = c->V.find(u + "mid_block.attentions.0.norm.bias");
                  if (ig != c->V.end() && ib != c->V.end()) { ngm.gamma = ig->second; ngm.beta = ib->second; ngm.eps = 1e-6f; ngm.silu = 0; } }
    Act r; CK(resnet(c, st, u + "mid_block.resnets.0.", h, nullptr, cm, 1e-5f, true, G, r, &ngm)); h = r;
    Act a; CK(transformer(c, st, u + "mid_block.attentions.0.", h, g.num_heads[nl - 1], G, a)); h = a;
    Act r2; CK(resnet(c, st, u + "mid_block.resnets.1.", h, nullptr, cm, 1e-5f, true, G, r2)); h = r2; }
  return 0;
}

// h + c->cur.ad_scale * feature `level` into a fresh activation, with the GroupNorm partial sums of the sum on 64-row tiles where the consumer takes
// them (norm.hip gn_part_ok: HW % bm == 0, C % 8 == 0, the 65536 index bound) and cpart_bm = 0 -- the norm's own statistics pass -- elsewhere
static int adapter_add(agd_ctx* c, hipStream_t st, int level, const Act& h, Act& out) {
  const int HW = h.H * h.W;
  if (level >= c->adc.n_channels || h.C != c->adc.channels[level] || h.H != (c->ad_Lh >> level) || h.W != (c->ad_Lw >> level) || c->ad_B < 1 || h.B % c->ad_B)
    FAIL("adapter: feature %d is set for %d images at %d x %d x %d, down block %d gives %d rows of %d x %d x %d", level, c->ad_B, c->ad_Lh >> level, c->ad_Lw >> level,
         level < c->adc.n_channels ? c->adc.channels[level] : 0, level, h.B, h.H, h.W, h.C);
  out = alloc_act(c, h.B, h.H, h.W, h.C, true); if (!out.p) return -1;
  const int bm = (out.cpart && HW % 64 == 0 && (long long)(h.C / c->cfg.norm_num_groups) * (HW / 64) < 65536) ? 64 : 0;
  out.cpart_bm = bm;
  const double rows = (double)h.B * HW;
  ProfScope ps(c, st, PC_ELEM, 0, rows * h.C * (2.0 + 4.0 + 2.0) + (bm ? rows / bm * h.C * 8.0 : 0.0));
  CK(launch_adapter_add(h.p, c->ad_featb[level].as<float>(), out.p, bm ? out.cpart : nullptr, bm, h.B, HW, h.C, c->ad_B, c->cur.ad_scale, st));
  c->ad_adds[bm ? 0 : 1]++;
  return 0;
}

// The ControlNet forward (diffusers ControlNetModel.forward, SD-1.x) at timestep t: its own time embedding, conv_in(x) + the cached
// conditioning embedding (conv_in's residual operand), the UNet's down / mid code under the "controlnet." weights, and a 1x1 zero conv
// per res sample and on the mid output, every result times `scale` (igemm alpha on the accumulator + the bias pre-scaled by cn_zbs).
// skips / h given (inside unet_walk, after the UNet's mid block): each zero conv runs as soon as its res sample exists, with the UNet's
//   skip k as its residual operand, into a FRESH activation allocated ahead of the ControlNet's own arena mark, and skip k is repointed to
//   it -- the launch leaves the GroupNorm partial sums of the injected tensor, while the old Act's partial sums and normed copy describe
//   the un-injected one.  The mid residual goes into *h the same way.  The ControlNet keeps no skip list of its own.
// skips == nullptr: the scaled residuals go to res_out as fp32 instead, back to back, NHWC or NCHW (agd_controlnet_residuals).
static int controlnet_walk(agd_ctx* c, hipStream_t st, const bf16_t* xin, int B2, int Lh, int Lw, float t, float scale, bool cfg_shared,
                           std::vector<Act>* skips, Act* h_unet, float* res_out, int nhwc) {
  const agd_config& g = c->cfg;
  if (!c->cn_on) FAIL("controlnet: none loaded (agd_controlnet_configure before agd_finalize)");
  if (c->ctx_stale) FAIL("the context is stale: a LoRA scale change rewrote the weights it was projected with (call agd_set_context)");
  if (c->cn_emb_B2 != B2 || c->cn_emb_Lh != Lh || c->cn_emb_Lw != Lw)
    FAIL("controlnet: the conditioning image is set for %d rows at latent sides %d x %d, this forward has %d rows at %d x %d (agd_controlnet_set_cond)",
         c->cn_emb_B2, c->cn_emb_Lh, c->cn_emb_Lw, B2, Lh, Lw);
  if (skips && ((int)skips->size() != c->cn_nres || !h_unet)) FAIL("controlnet: %zu UNet skips for %d ControlNet res samples", skips->size(), c->cn_nres);
  std::vector<Act> inj;
  if (skips) {
    for (const Act& s : *skips) { inj.push_back(alloc_act(c, s.B, s.H, s.W, s.C, true)); if (!inj.back().p) return -1; }
    inj.push_back(alloc_act(c, h_unet->B, h_unet->H, h_unet->W, h_unet->C, true)); if (!inj.back().p) return -1;
  }
  if (!(scale == c->cn_zscale)) {                       // (the biases are rewritten only when the scale changes; stream-ordered)
    ProfScope ps(c, st, PC_ELEM, 0);
    CK(launch_controlnet_scale_bias(c->cn_zb, c->cn_zbs, c->cn_zb_total, scale, st));
    c->cn_zscale = scale;
  }
  const size_t mk = c->arena.mark();
  const float* tp_save = c->tproj_cur; const int ld_save = c->tproj_cur_ld;
  CK(time_embed(c, st, &t, 1, c->temb_buf, c->cn_tproj_out, true));
  c->tproj_cur = c->cn_tproj_out; c->tproj_cur_ld = 0;
  const std::string u = "controlnet.";
  int k = 0; long long res_off = 0;
  auto zero_conv = [&](const Act& s) -> int {
    const std::string key = u + (k < c->cn_nres ? "controlnet_down_blocks." + std::to_string(k) + "." : std::string("controlnet_mid_block."));
    GETW(w, key + "weight");
    if (w->N != s.C || w->Cpad != s.C) FAIL("controlnet: '%sweight' is [%d, %d], res sample %d has %d channels", key.c_str(), w->N, w->Cin, k, s.C);
    GemmOpt o; o.bias = c->cn_zbs + c->cn_zb_off[k]; o.alpha = scale;
    if (skips) {
      Act& base = k < c->cn_nres ? (*skips)[k] : *h_unet;
      if (base.B != s.B || base.H != s.H || base.W != s.W || base.C != s.C) FAIL("controlnet: res sample %d does not match the UNet's", k);
      Act& dst = inj[k];
      o.residual = base.p; o.out_act = &dst;
      CK(run_conv(c, st, s.p, s.C, nullptr, 0, s.B, s.H, s.W, *w, 1, dst.p, o, c->zero_page));
      base = dst;                                       // (fresh partial sums, no normed copy)
    } else {
      float* dst = res_out + res_off;
      o.out_f32 = 1;
      if (nhwc) CK(run_conv(c, st, s.p, s.C, nullptr, 0, s.B, s.H, s.W, *w, 1, dst, o, c->zero_page));
      else {
        float* tmp = (float*)c->arena.alloc((size_t)s.n() * 4); if (!tmp) return -1;
        CK(run_conv(c, st, s.p, s.C, nullptr, 0, s.B, s.H, s.W, *w, 1, tmp, o, c->zero_page));
        ProfScope ps(c, st, PC_ELEM, 0);
        CK(launch_nchw_from_nhwc_f32(tmp, s.C, dst, s.B, s.C, s.H * s.W, st));
      }
      res_off += s.n();
    }
    ++k;
    return 0;
  };
  // the CFG halves see the same latents and the same conditioning rows up to the first attn2 (as in the UNet) when the embedding was set
  // with an even repeat
  const bool shared = cfg_shared && (B2 % 2) == 0 && g.down_cross[0] && c->opt_cfg_share && c->cn_emb_rep % 2 == 0;
  Act h;
  CK(down_mid_walk(c, st, u, xin, B2, Lh, Lw, shared, c->cn_embb.as<bf16_t>(), zero_conv, h));
  CK(zero_conv(h));
  c->tproj_cur = tp_save; c->tproj_cur_ld = ld_save;
  c->arena.release(mk);
  return 0;
}

// FreeU on the inputs of one resnet of up block `blk` (0 or 1): ho = h with its first C / 2 channels times b, so = sk with its lowest four
// frequencies times s, both in FRESH activations written by one launch (freeu.hip) -- the old Acts may still be a ControlNet's or a recorder's
// operand, and their partial sums / normed copies describe the un-weighted tensors.  b == 1 / s == 1 leaves that tensor (and its Act) alone;
// both 1 launches nothing.  The outputs carry the GroupNorm partial sums of their bf16-rounded values on 64-row tiles where the concat norm
// takes them (as adapter_add), cpart_bm = 0 -- the norm's own statistics pass -- elsewhere.
static int freeu_apply(agd_ctx* c, hipStream_t st, int blk, const Act& h, const Act& sk, Act& ho, Act& so) {
  const float b = c->fu_b[blk], s = c->fu_s[blk];
  ho = h; so = sk;
  if (b == 1.f && s == 1.f) return 0;
  if (h.B != sk.B || h.H != sk.H || h.W != sk.W) FAIL("freeu: up block %d joins %d x %d x %d with a skip of %d x %d x %d", blk, h.B, h.H, h.W, sk.B, sk.H, sk.W);
  const int HW = h.H * h.W;
  if (b != 1.f) { ho = alloc_act(c, h.B, h.H, h.W, h.C, true); if (!ho.p) return -1; }
  if (s != 1.f) { so = alloc_act(c, sk.B, sk.H, sk.W, sk.C, true); if (!so.p) return -1; }
  const bool stats = (b == 1.f || ho.cpart) && (s == 1.f || so.cpart) && HW % 64 == 0 &&
                     (long long)(std::max(h.C, sk.C) / c->cfg.norm_num_groups) * (HW / 64) < 65536;
  if (b != 1.f) ho.cpart_bm = stats ? 64 : 0;
  if (s != 1.f) so.cpart_bm = stats ? 64 : 0;
  const double rows = (double)h.B * HW, ch = (b != 1.f ? h.C : 0) + (s != 1.f ? 1.5 * sk.C : 0);          // (the filter reads its map twice)
  ProfScope ps(c, st, PC_ELEM, 0, rows * ch * 4.0 + (stats ? rows / 64 * ch * 8.0 : 0.0));
  CK(launch_freeu(h.p, b != 1.f ? ho.p : nullptr, stats ? ho.cpart : nullptr, h.C, sk.p, s != 1.f ? so.p : nullptr, stats ? so.cpart : nullptr, sk.C,
                  h.B, h.H, h.W, b, s, st));
  c->fu_counts[stats ? 0 : 1]++;
  return 0;
}

// DeepCache: the bytes the slot needs for a capture of `rows` rows at Lh x Lw -- the widest tensor that can enter the last up block (its own
// channels, or the previous block's through the upsampler) and the partial sums of kMinStatTile-row tiles, alloc_act's own worst case: a
// table that fits the activation it came from fits here, so a capture cannot run out of room in the middle of an evaluation
static size_t deepcache_slot_bytes(const agd_ctx* c, int rows, int Lh, int Lw, size_t* part_off) {
  const agd_config& g = c->cfg;
  const int C = std::max(g.block_out_channels[0], g.block_out_channels[g.n_levels > 1 ? 1 : 0]);
  const size_t act = ((size_t)rows * Lh * Lw * C * 2 + 255) & ~(size_t)255;
  if (part_off) *part_off = act;
  return act + ((size_t)rows * Lh * Lw / kMinStatTile + 1) * C * 2 * sizeof(float);
}
static void deepcache_invalidate(agd_ctx* c) { c->dc_valid = false; }
// h (the hidden state about to enter U_{b+1}) and its partial sums into the slot, one launch; dc_act then describes the copy.  The slot was
// sized before the call's first launch (deepcache_reserve); a tensor that does not fit is refused, never written.
static int deepcache_capture(agd_ctx* c, hipStream_t st, const Act& h, int branch) {
  size_t part_off = 0;
  const size_t need = deepcache_slot_bytes(c, h.B, h.H, h.W, &part_off);
  const long long nb = h.n() * 2;
  const long long pb = h.cpart_bm > 0 ? (long long)((long long)h.B * h.H * h.W / h.cpart_bm) * h.C * 2 * (long long)sizeof(float) : 0;
  if (!c->dc_buf.p || c->dc_buf.cap < need || (size_t)nb > part_off || (size_t)pb > need - part_off || (pb > 0 && !h.cpart))
    FAIL("deepcache: the slot holds %zu bytes, the capture of %d x %d x %d x %d needs %lld + %lld", c->dc_buf.cap, h.B, h.H, h.W, h.C, nb, pb);
  c->dc_valid = false;
  char* base = c->dc_buf.as<char>();
  { ProfScope ps(c, st, PC_ELEM, 0, 2.0 * (double)(nb + pb));
    CK(launch_deepcache_capture(h.p, base, nb, h.cpart, base + part_off, pb, st)); }
  Act a; a.p = (bf16_t*)base; a.B = h.B; a.H = h.H; a.W = h.W; a.C = h.C; a.cpart_bm = h.cpart_bm; a.cpart = pb > 0 ? (float*)(base + part_off) : nullptr;
  c->dc_act = a; c->dc_valid = true; c->dc_rows = h.B; c->dc_Lh = h.H; c->dc_Lw = h.W; c->dc_b = branch;
  c->dc_counts[0]++;
  return 0;
}
static int deepcache_reserve(agd_ctx* c, int rows, int Lh, int Lw) { return c->dc_buf.ensure(deepcache_slot_bytes(c, rows, Lh, Lw, nullptr)); }

// x: [B2][Lh*Lw][64] bf16 (latent channels zero-padded) -> eps [B2][Lh*Lw][out_channels] fp32 NHWC
// tproj_row: this timestep's time_emb_proj outputs when the caller computed them up front (agd_denoise), else nullptr
// cfg_shared: rows [0,B2/2) and [B2/2,B2) of xin are identical (agd_denoise): share everything ahead of the first attn2
// tproj_ld: 0 = tproj_row serves every image; tproj_total = tproj_row holds one row per image (per-sample timesteps, training)
// DeepCache (ec.dc): DC_SHALLOW runs conv_in and layers 0 .. b of down block 0, then enters the last up block at layer lpb - b - 1 with h taken
// from the context's slot (dc_act) -- the same up loop entered later, so the CFG-shared prefix, the recorders and FreeU ride along; DC_CAPTURE is
// the plain walk, launch for launch, plus one capture launch in front of that layer (before FreeU touches h).
// ec: what this evaluation runs beside the UNet -- one element of the CallCond that resolve_cond() built for the call before its first launch
// (nothing is refused here any more); it becomes c->cur, where tblock_plan (fusers, image branch) and down_mid_walk / adapter_add (features) read it
static int unet_walk(agd_ctx* c, hipStream_t st, const bf16_t* xin, int B2, int Lh, int Lw, float t, float* eps_out,
                     const float* tproj_row = nullptr, bool cfg_shared = false, int tproj_ld = 0, const EvalCond& ec = EvalCond()) {
  const agd_config& g = c->cfg;
  c->cur = ec;
  if (c->ctx_stale) FAIL("the context is stale: a LoRA scale change rewrote the weights it was projected with (call agd_set_context)");
  const int nl = g.n_levels, G = g.norm_num_groups;
  const std::string u = "unet.";
  c->arena.release(0);
  c->tproj_cur_ld = tproj_row ? tproj_ld : 0;
  if (tproj_row) c->tproj_cur = tproj_row;
  else { CK(time_embed(c, st, &t, 1, c->temb_buf, c->tproj_out)); c->tproj_cur = c->tproj_out; }
  std::vector<Act> skips;
  const bool shared = cfg_shared && (B2 % 2) == 0 && g.down_cross[0] && c->opt_cfg_share;
  Act h;
  const int lpb = g.layers_per_block;
  const bool shallow = ec.dc == DC_SHALLOW;
  const int dc_j = ec.dc ? lpb - ec.dc_branch - 1 : -1;              // the last up block's layer U_{b+1}
  if (ec.dc && (ec.dc_branch < 0 || ec.dc_branch > lpb - 1)) FAIL("deepcache: branch %d (this UNet has branches 0 .. %d)", ec.dc_branch, lpb - 1);
  if (shallow) {
    if (!c->dc_valid || c->dc_rows != B2 || c->dc_Lh != Lh || c->dc_Lw != Lw || c->dc_b != ec.dc_branch)
      FAIL("deepcache: a shallow evaluation of %d rows at %d x %d, branch %d, without a valid cache (a full evaluation that captures comes first)", B2, Lh, Lw, ec.dc_branch);
    c->dc_counts[1]++;
  }
  CK(down_mid_walk(c, st, u, xin, B2, Lh, Lw, shared, nullptr, [&](const Act& a) { skips.push_back(a); return 0; }, h, shallow ? ec.dc_branch : -1));
  if (shallow) h = c->dc_act;
  if (ec.cn_scale != 0.f) {
    if (c->tproj_cur_ld != 0) FAIL("controlnet: per-image timesteps are not supported");
    CK(controlnet_walk(c, st, xin, B2, Lh, Lw, t, ec.cn_scale, cfg_shared, &skips, &h, nullptr, 0));
  }
  for (int i = shallow ? nl - 1 : 0; i < nl; ++i) {
    const int lvl = nl - 1 - i, co = g.block_out_channels[lvl];
    for (int j = shallow ? dc_j : 0; j < g.layers_per_block + 1; ++j) {
      if (ec.dc == DC_CAPTURE && i == nl - 1 && j == dc_j) CK(deepcache_capture(c, st, h, ec.dc_branch));
      Act sk = skips.back(); skips.pop_back();
      NextGn ngu;
      if (g.down_cross[lvl]) { const std::string nk = u + "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".norm.";
        auto ig = c->V.find(nk + "weight"), ib = c->V.find(nk + "bias"); if (ig != c->V.end() && ib != c->V.end()) { ngu.gamma = ig->second; ngu.beta = ib->second; ngu.eps = 1e-6f; ngu.silu = 0; } }
      Act hf = h, skf = sk;
      if (c->fu_on && i < 2) CK(freeu_apply(c, st, i, h, sk, hf, skf));       // (off: the plain walk, launch for launch)
      Act r; CK(resnet(c, st, u + "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".", hf, &skf, co, 1e-5f, true, G, r, &ngu));
      h = r;
      if (g.down_cross[lvl]) {
        Act a; CK(transformer(c, st, u + "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", h, g.num_heads[lvl], G, a));
        h = a;
      }
    }
    if (i != nl - 1) {
      const std::string k = u + "up_blocks." + std::to_string(i) + ".upsamplers.0.conv.";
      GETW(w, k + "weight"); GETV(b, k + "bias");
      Act d = alloc_act(c, B2, h.H * 2, h.W * 2, co, true); if (!d.p) return -1;
      if ((c->opt_ups4 & 1) && c->W.count(k + "phases") && (long long)B2 * h.H * h.W >= ((c->opt_ups4 & 4) ? 512 : 2048)) {
        // conv3x3(nearest2x(x)) = four 2x2 convs on x, one per output phase, with the taps that coincide pre-summed (misc.hip upsample_phase_weight_kernel): 4/9 of the MACs
        GETW(w4, k + "phases"); GETV(b4, k + "phases.bias");
        GemmOpt o; o.bias = b4; o.out_act = &d; o.ups4 = co; o.hout = h.H; o.wout = h.W; o.ldo = co; o.pad = 0;
        if (c->opt_ups4 & 8) o.p8 = -1;                    // (A/B: keep the phase convs on the 4-wave kernel)
        CK(run_conv(c, st, h.p, co, nullptr, 0, B2, h.H, h.W, *w4, 2, d.p, o, c->zero_page));
      } else {
      GemmOpt o; o.bias = b; o.up = 2; o.out_act = &d;
      CK(run_conv(c, st, h.p, co, nullptr, 0, B2, h.H, h.W, *w, 3, d.p, o, c->zero_page));
      }
      h = d;
    }
  }
  { Act n = alloc_act(c, B2, Lh, Lw, h.C); if (!n.p) return -1;
    GETV(gg, u + "conv_norm_out.weight"); GETV(gb, u + "conv_norm_out.bias");
    CK(run_gn(c, st, h.p, h.C, nullptr, 0, B2, Lh * Lw, gg, gb, G, 1e-5f, 1, n.p, &h));
    GETW(w, u + "conv_out.weight"); GETV(b, u + "conv_out.bias");
    GemmOpt o; o.bias = b; o.out_f32 = 1; o.ldo = g.out_channels;
    CK(run_conv(c, st, n.p, h.C, nullptr, 0, B2, Lh, Lw, *w, 3, eps_out, o, c->zero_page)); }
  return 0;
}

// AutoencoderKL mid-block attention: single head over N = Lh*Lw tokens, C channels, through batched GEMMs
static int vae_mid_attention(agd_ctx* c, hipStream_t st, const std::string& a, int G, int B, int Lh, int Lw, int top, Act& h) {
    const int N = Lh * Lw, C = top, M = B * N;
    Act out = alloc_act(c, B, Lh, Lw, C, true); if (!out.p) return -1;
    const size_t mk = c->arena.mark();
    Act n = alloc_act(c, B, Lh, Lw, C); if (!n.p) return -1;
    GETV(gg, a + "group_norm.weight"); GETV(gb, a + "group_norm.bias");
    CK(run_gn(c, st, h.p, C, nullptr, 0, B, N, gg, gb, G, 1e-6f, 0, n.p, &h));
    bf16_t* q = (bf16_t*)c->arena.alloc((size_t)M * C * 2); bf16_t* k = (bf16_t*)c->arena.alloc((size_t)M * C * 2);
    bf16_t* vT = (bf16_t*)c->arena.alloc((size_t)M * C * 2); bf16_t* att = (bf16_t*)c->arena.alloc((size_t)M * C * 2);
    float* S = (float*)c->arena.alloc((size_t)B * N * N * 4); bf16_t* P = (bf16_t*)c->arena.alloc((size_t)B * N * N * 2);
    if (!q || !k || !vT || !att || !S || !P) return -1;
    GETW(wq, a + "to_q.weight"); GETV(bq, a + "to_q.bias"); GETW(wk, a + "to_k.weight"); GETV(bk, a + "to_k.bias");
    GETW(wv, a + "to_v.weight"); GETV(bv, a + "to_v.bias"); GETW(wo, a + "to_out.0.weight"); GETV(bo, a + "to_out.0.bias");
    { GemmOpt o; o.bias = bq; CK(run_conv(c, st, n.p, C, nullptr, 0, 1, 1, M, *wq, 1, q, o, c->zero_page)); }
    { GemmOpt o; o.bias = bk; CK(run_conv(c, st, n.p, C, nullptr, 0, 1, 1, M, *wk, 1, k, o, c->zero_page)); }
    { // V^T[b] = Wv . X[b]^T  -> [C][N], bias per output row
      IgemmP p{}; p.src0 = wv->w; p.C0 = C; p.Hin = 1; p.Win = C; p.Hout = 1; p.Wout = C; p.ksize = 1; p.stride = 1; p.up = 1;
      p.W = n.p; p.bias = bv; p.bias_mode = 2; p.out = vT; p.ldo = N; p.ldr = N; p.M = C; p.N = N; p.K = C; p.alpha = 1.f;
      p.batch = B; p.sA0 = 0; p.sW = (long long)N * C; p.sO = (long long)C * N; p.zero_page = c->zero_page;
      ProfScope ps(c, st, PC_GEMM, 2.0 * B * C * (double)N * C); CK(launch_igemm(p, st)); }
    { // S[b] = scale * Q[b] K[b]^T  (fp32)
      IgemmP p{}; p.src0 = q; p.C0 = C; p.Hin = 1; p.Win = N; p.Hout = 1; p.Wout = N; p.ksize = 1; p.stride = 1; p.up = 1;
      p.W = k; p.out = S; p.out_f32 = 1; p.ldo = N; p.ldr = N; p.M = N; p.N = N; p.K = C; p.alpha = 1.0f / sqrtf((float)C);
      p.batch = B; p.sA0 = (long long)N * C; p.sW = (long long)N * C; p.sO = (long long)N * N; p.zero_page = c->zero_page;
      ProfScope ps(c, st, PC_VAE_ATTN, 2.0 * B * N * (double)N * C); CK(launch_igemm(p, st)); }
    { ProfScope ps(c, st, PC_VAE_ATTN, 0); CK(launch_softmax_rows(S, P, B * N, N, st)); }
    { // O[b] = P[b] V[b]  via V^T as the [N=C][K=N] operand
      IgemmP p{}; p.src0 = P; p.C0 = N; p.Hin = 1; p.Win = N; p.Hout = 1; p.Wout = N; p.ksize = 1; p.stride = 1; p.up = 1;
      p.W = vT; p.out = att; p.ldo = C; p.ldr = C; p.M = N; p.N = C; p.K = N; p.alpha = 1.f;
      p.batch = B; p.sA0 = (long long)N * N; p.sW = (long long)C * N; p.sO = (long long)N * C; p.zero_page = c->zero_page;
      ProfScope ps(c, st, PC_VAE_ATTN, 2.0 * B * N * (double)N * C); CK(launch_igemm(p, st)); }
    { GemmOpt o; o.bias = bo; o.residual = h.p; o.out_act = &out; o.rows_per_image = N; CK(run_conv(c, st, att, C, nullptr, 0, 1, 1, M, *wo, 1, out.p, o, c->zero_page)); }
    c->arena.release(mk);
    h = out;
  return 0;
}

// AutoencoderKL.decode: z [B][Lh*Lw][64] bf16 (already divided by scaling factor) -> fp32 NHWC [B][8Lh*8Lw][ldo=4]
static int vae_walk(agd_ctx* c, hipStream_t st, const bf16_t* zin, int B, int Lh, int Lw, float* img_out) {
  const agd_config& g = c->cfg;
  const int nl = g.vae_n_levels, G = g.vae_norm_num_groups;
  const std::string v = "vae.";
  c->arena.release(0);
  const int top = g.vae_block_out_channels[nl - 1];
  // post_quant_conv (1x1, 4->4) written into a zeroed 64-channel buffer so conv_in sees padded input
  bf16_t* pq = (bf16_t*)c->arena.alloc((size_t)B * Lh * Lw * 64 * 2); if (!pq) return -1;
  if (hipMemsetAsync(pq, 0, (size_t)B * Lh * Lw * 64 * 2, st) != hipSuccess) FAIL("memset pq");
  { GETW(w, v + "post_quant_conv.weight"); GETV(b, v + "post_quant_conv.bias"); GemmOpt o; o.bias = b; o.ldo = 64;
    CK(run_conv(c, st, zin, 64, nullptr, 0, B, Lh, Lw, *w, 1, pq, o, c->zero_page)); }
  Act h = alloc_act(c, B, Lh, Lw, top, true); if (!h.p) return -1;
  { GETW(w, v + "decoder.conv_in.weight"); GETV(b, v + "decoder.conv_in.bias"); GemmOpt o; o.bias = b; o.out_act = &h;
    CK(run_conv(c, st, pq, 64, nullptr, 0, B, Lh, Lw, *w, 3, h.p, o, c->zero_page)); }
  { Act r; CK(resnet(c, st, v + "decoder.mid_block.resnets.0.", h, nullptr, top, 1e-6f, false, G, r)); h = r; }
  CK(vae_mid_attention(c, st, v + "decoder.mid_block.attentions.0.", G, B, Lh, Lw, top, h));
  { Act r; CK(resnet(c, st, v + "decoder.mid_block.resnets.1.", h, nullptr, top, 1e-6f, false, G, r)); h = r; }
  for (int i = 0; i < nl; ++i) {
    const int co = g.vae_block_out_channels[nl - 1 - i];
    for (int j = 0; j < g.vae_layers_per_block + 1; ++j) {
      Act r; CK(resnet(c, st, v + "decoder.up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".", h, nullptr, co, 1e-6f, false, G, r));
      h = r;
    }
    if (i != nl - 1) {
      const std::string k = v + "decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv.";
      GETW(w, k + "weight"); GETV(b, k + "bias");
      Act d = alloc_act(c, B, h.H * 2, h.W * 2, co, true); if (!d.p) return -1;
      if ((c->opt_ups4 & 2) && c->W.count(k + "phases")) {              // four 2x2 phase convs on the un-upsampled map (as in the UNet walk)
        GETW(w4, k + "phases"); GETV(b4, k + "phases.bias");
        GemmOpt o; o.bias = b4; o.out_act = &d; o.ups4 = co; o.hout = h.H; o.wout = h.W; o.ldo = co; o.pad = 0;
        if (c->opt_ups4 & 8) o.p8 = -1;
        CK(run_conv(c, st, h.p, co, nullptr, 0, B, h.H, h.W, *w4, 2, d.p, o, c->zero_page));
      } else {
      GemmOpt o; o.bias = b; o.up = 2; o.out_act = &d;
      CK(run_conv(c, st, h.p, co, nullptr, 0, B, h.H, h.W, *w, 3, d.p, o, c->zero_page));
      }
      h = d;
    }
  }
  { Act n = alloc_act(c, B, h.H, h.W, h.C); if (!n.p) return -1;
    GETV(gg, v + "decoder.conv_norm_out.weight"); GETV(gb, v + "decoder.conv_norm_out.bias");
    CK(run_gn(c, st, h.p, h.C, nullptr, 0, B, h.H * h.W, gg, gb, G, 1e-6f, 1, n.p, &h));
    GETW(w, v + "decoder.conv_out.weight"); GETV(b, v + "decoder.conv_out.bias");
    GemmOpt o; o.bias = b; o.out_f32 = 1; o.ldo = 4;
    CK(run_conv(c, st, n.p, h.C, nullptr, 0, B, h.H, h.W, *w, 3, img_out, o, c->zero_page)); }
  return 0;
}

// AutoencoderKL.encode: x [B][Sh*Sw][64] bf16 (3 image channels zero-padded) -> moments fp32 NHWC [B][Lh*Lw][2*lc]
static int vae_encode_walk(agd_ctx* c, hipStream_t st, const bf16_t* xin, int B, int Sh, int Sw, float* moments) {
  const agd_config& g = c->cfg;
  const int nl = g.vae_n_levels, G = g.vae_norm_num_groups, lc = g.vae_latent_channels;
  const std::string v = "vae.";
  c->arena.release(0);
  Act h = alloc_act(c, B, Sh, Sw, g.vae_block_out_channels[0], true); if (!h.p) return -1;
  { GETW(w, v + "encoder.conv_in.weight"); GETV(b, v + "encoder.conv_in.bias"); GemmOpt o; o.bias = b; o.out_act = &h;
    CK(run_conv(c, st, xin, 64, nullptr, 0, B, Sh, Sw, *w, 3, h.p, o, c->zero_page)); }
  for (int i = 0; i < nl; ++i) {
    const int co = g.vae_block_out_channels[i];
    for (int j = 0; j < g.vae_layers_per_block; ++j) {
      Act r; CK(resnet(c, st, v + "encoder.down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".", h, nullptr, co, 1e-6f, false, G, r));
      h = r;
    }
    if (i != nl - 1) {   // Downsample2D(padding=0) after F.pad(x, (0,1,0,1)): taps beyond the bottom/right edge read zeros
      const std::string k = v + "encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv.";
      GETW(w, k + "weight"); GETV(b, k + "bias");
      Act d = alloc_act(c, B, h.H / 2, h.W / 2, co, true); if (!d.p) return -1;
      GemmOpt o; o.bias = b; o.stride = 2; o.pad = 0; o.hout = h.H / 2; o.wout = h.W / 2; o.out_act = &d;
      CK(run_conv(c, st, h.p, co, nullptr, 0, B, h.H, h.W, *w, 3, d.p, o, c->zero_page));
      h = d;
    }
  }
  const int top = g.vae_block_out_channels[nl - 1], Lh = h.H, Lw = h.W;
  { Act r; CK(resnet(c, st, v + "encoder.mid_block.resnets.0.", h, nullptr, top, 1e-6f, false, G, r)); h = r; }
  CK(vae_mid_attention(c, st, v + "encoder.mid_block.attentions.0.", G, B, Lh, Lw, top, h));
  { Act r; CK(resnet(c, st, v + "encoder.mid_block.resnets.1.", h, nullptr, top, 1e-6f, false, G, r)); h = r; }
  Act n = alloc_act(c, B, Lh, Lw, top); if (!n.p) return -1;
  GETV(gg, v + "encoder.conv_norm_out.weight"); GETV(gb, v + "encoder.conv_norm_out.bias");
  CK(run_gn(c, st, h.p, top, nullptr, 0, B, Lh * Lw, gg, gb, G, 1e-6f, 1, n.p, &h));
  // conv_out (top -> 2*lc) into a zeroed 64-channel buffer, then quant_conv 1x1 (2*lc -> 2*lc) in fp32 out
  bf16_t* co64 = (bf16_t*)c->arena.alloc((size_t)B * Lh * Lw * 64 * 2); if (!co64) return -1;
  if (hipMemsetAsync(co64, 0, (size_t)B * Lh * Lw * 64 * 2, st) != hipSuccess) FAIL("memset enc");
  { GETW(w, v + "encoder.conv_out.weight"); GETV(b, v + "encoder.conv_out.bias"); GemmOpt o; o.bias = b; o.ldo = 64;
    CK(run_conv(c, st, n.p, top, nullptr, 0, B, Lh, Lw, *w, 3, co64, o, c->zero_page)); }
  { GETW(w, v + "quant_conv.weight"); GETV(b, v + "quant_conv.bias"); GemmOpt o; o.bias = b; o.out_f32 = 1; o.ldo = 2 * lc;
    CK(run_conv(c, st, co64, 64, nullptr, 0, B, Lh, Lw, *w, 1, moments, o, c->zero_page)); }
  return 0;
}

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
AGD_API const char* agd_version(void) { return "agenda_hip 0.1 (gfx950)"; }
AGD_API const char* agd_last_error(agd_ctx* c) { return (c && !c->err.empty()) ? c->err.c_str() : g_err; }
AGD_API const char* agd_profile_class_name(int cls) { return (cls >= 0 && cls < AGD_N_CLASSES) ? kClassNames[cls] : ""; }

AGD_API agd_ctx* agd_create(int device_id, const agd_config* cfg) {
  if (!cfg || cfg->struct_size != (int)sizeof(agd_config)) { agd_set_error("agd_create: bad config (struct_size %d != %zu)", cfg ? cfg->struct_size : -1, sizeof(agd_config)); return nullptr; }
  if (cfg->n_levels < 1 || cfg->n_levels > AGD_MAX_LEVELS || cfg->vae_n_levels < 1 || cfg->vae_n_levels > AGD_MAX_LEVELS) { agd_set_error("agd_create: bad level count"); return nullptr; }
  for (int i = 0; i < cfg->n_levels; ++i)
    if (cfg->block_out_channels[i] % 64) { agd_set_error("agd_create: UNet channels must be multiples of 64"); return nullptr; }
  for (int i = 0; i < cfg->vae_n_levels; ++i)
    if (cfg->vae_block_out_channels[i] % 64) { agd_set_error("agd_create: VAE channels must be multiples of 64"); return nullptr; }
  if (cfg->cross_attention_dim % 64) { agd_set_error("agd_create: cross_attention_dim must be a multiple of 64"); return nullptr; }
  if (hipSetDevice(device_id) != hipSuccess) { agd_set_error("hipSetDevice(%d) failed", device_id); return nullptr; }
  agd_ctx* c = new agd_ctx(); c->device = device_id; c->cfg = *cfg;
  const size_t ws = cfg->workspace_bytes > 0 ? (size_t)cfg->workspace_bytes : ((size_t)8 << 30);
  if (hipMalloc((void**)&c->arena.base, ws) != hipSuccess) { agd_set_error("arena hipMalloc(%zu) failed", ws); delete c; return nullptr; }
  c->arena.cap = ws;
  c->zero_page = dmalloc<bf16_t>(c, 2048);
  c->t_dev = dmalloc<float>(c, 64);
  if (!c->zero_page || !c->t_dev) { delete c; return nullptr; }
  hipMemset(c->zero_page, 0, 4096);
  return c;
}

AGD_API void agd_destroy(agd_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipDeviceSynchronize();
  for (void* p : c->owned) hipFree(p);
  for (auto& xl : c->xl) { xl.kvb.release(); xl.accb.release(); }
  c->pano_viewb.release(); c->pano_hmb.release(); c->reg_xb.release(); c->pano_ctxb.release(); c->i2_latb.release();
  c->ctxb.release(); c->hook_sumb.release(); c->hook_scratchb.release(); c->hook_headsb.release(); c->hook_storeb.release(); c->bwd_wsb.release();
  for (auto& xl : c->xl) { xl.wqTb.release(); xl.wkvTb.release(); xl.woTb.release(); xl.pm_kppb.release(); xl.pm_vppb.release(); xl.pm_csb.release(); }
  c->latb.release(); c->epsb.release(); c->vae_imgb.release(); c->plmsb.release(); c->dpmb.release(); c->gr_factb.release(); c->sega_momb.release(); c->sega_thrb.release(); c->dc_buf.release(); c->cn_embb.release(); c->lora_descb.release();
  for (auto& f : c->gl_f) f.gkvb.release();
  c->gl_objb.release();
  for (auto& b : c->ad_featb) b.release();
  ipa_release(c);
  if (c->side) { hipStreamDestroy(c->side); hipEventDestroy(c->ev_fork); hipEventDestroy(c->ev_join); }
  if (c->splitk.p) hipFree(c->splitk.p);
  if (c->arena.base) hipFree(c->arena.base);
  if (c->stage) hipFree(c->stage);
  if (c->tsteps_buf) hipFree(c->tsteps_buf);
  for (auto e : c->ev_pool) hipEventDestroy(e);
  delete c;
}

static bool ends_with(const std::string& s, const char* suf) { const size_t n = strlen(suf); return s.size() >= n && s.compare(s.size() - n, n, suf) == 0; }

AGD_API int agd_load_tensor(agd_ctx* c, const char* name, const void* ptr, int dtype, int ndim, const long long* shape) {
  if (!c || !name || !ptr || !shape) { agd_set_error("agd_load_tensor: null argument"); return fail_ctx(c); }
  if (dtype != 0) { agd_set_error("agd_load_tensor: only float32 (dtype 0) supported"); return fail_ctx(c); }
  hipSetDevice(c->device);
  long long n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i];
  const size_t bytes = (size_t)n * 4;
  if (bytes > c->stage_bytes) {
    if (c->stage) hipFree(c->stage);
    if (hipMalloc((void**)&c->stage, bytes) != hipSuccess) { c->stage = nullptr; c->stage_bytes = 0; agd_set_error("stage alloc failed"); return fail_ctx(c); }
    c->stage_bytes = bytes;
  }
  if (hipMemcpy(c->stage, ptr, bytes, hipMemcpyDefault) != hipSuccess) { agd_set_error("copy of '%s' failed", name); return fail_ctx(c); }
  const std::string k(name);
  if (k.compare(0, 11, "controlnet.") == 0 && !c->cn_on) { agd_set_error("'%s': call agd_controlnet_configure before loading ControlNet weights", name); return fail_ctx(c); }
  if (k.compare(0, 8, "adapter.") == 0 && !c->ad_on) { agd_set_error("'%s': call agd_adapter_configure before loading T2I-Adapter weights", name); return fail_ctx(c); }
  if ((k.compare(0, 18, "unet.position_net.") == 0 || k.find(".fuser.") != std::string::npos) && !c->gl_on) {
    agd_set_error("'%s': call agd_gligen_configure before loading GLIGEN weights", name); return fail_ctx(c); }
  // the safety checker keeps everything but its encoder-layer matrices in fp32 as loaded (embeddings, the 14 x 14 patch conv, the
  // projection, the concept rows); agd_finalize checks their sizes and builds the padded patch matrix
  const bool vis_f32 = (k.compare(0, 7, "safety.") == 0 || k.compare(0, 14, "image_encoder.") == 0) && !(ndim == 2 && k.find(".encoder.layers.") != std::string::npos);
  if (ndim == 1 || vis_f32 || (ndim == 0 && c->gl_on)) {            // (0-d: GLIGEN's alpha_attn / alpha_dense)
    float* d = dmalloc<float>(c, (size_t)n); if (!d) return fail_ctx(c);
    hipMemcpy(d, c->stage, bytes, hipMemcpyDeviceToDevice);
    c->V[k] = d; c->Vn[k] = (int)n;
  } else if (ndim == 2 || ndim == 4) {
    WMat w; w.N = (int)shape[0]; w.Cin = (int)shape[1]; w.taps = ndim == 4 ? (int)(shape[2] * shape[3]) : 1;
    if (w.taps != 1 && w.taps != 9) { agd_set_error("'%s': only 1x1 / 3x3 kernels", name); return fail_ctx(c); }
    w.Cpad = (w.Cin + 63) / 64 * 64;
    const bool is_tok_emb = ends_with(k, "token_embedding.weight");
    w.w = dmalloc<bf16_t>(c, (size_t)(w.N + (is_tok_emb ? kTextExtraRows : 0)) * w.taps * w.Cpad); if (!w.w) return fail_ctx(c);
    if (is_tok_emb) hipMemset(w.w + (size_t)w.N * w.Cpad, 0, (size_t)kTextExtraRows * w.Cpad * 2);
    const int geglu_bn = ends_with(k, "ff.net.0.proj.weight") ? 16 : 0;   // [8 values | 8 gates] per 16 rows (igemm_epilogue.h)
    if (geglu_bn && (w.N % 256)) { agd_set_error("'%s': GEGLU projection rows %d not a multiple of 256", name, w.N); return fail_ctx(c); }
    API_CK(c, launch_convert_weight(c->stage, w.w, w.N, w.Cin, w.taps, w.Cpad, geglu_bn, 0));
    hipDeviceSynchronize();
    c->W[k] = w;
  } else { agd_set_error("'%s': unsupported ndim %d", name, ndim); return fail_ctx(c); }
  return 0;
}

// alloc = false: `out` is an earlier concatenation of the same parts, rewritten in place
static int concat_rows(agd_ctx* c, const std::vector<const WMat*>& parts, WMat& out, bool alloc = true) {
  if (alloc) {
    out = WMat(); out.Cin = parts[0]->Cin; out.Cpad = parts[0]->Cpad; out.taps = parts[0]->taps;
    for (auto* p : parts) { if (p->Cpad != out.Cpad || p->taps != out.taps) FAIL("concat_rows: mismatched K"); out.N += p->N; }
    out.w = dmalloc<bf16_t>(c, (size_t)out.N * out.taps * out.Cpad); if (!out.w) return -1;
  } else {
    int n = 0; for (auto* p : parts) { if (p->Cpad != out.Cpad || p->taps != out.taps) FAIL("concat_rows: mismatched K"); n += p->N; }
    if (n != out.N || !out.w) FAIL("concat_rows: %d rows do not match the earlier %d", n, out.N);
  }
  size_t off = 0;
  for (auto* p : parts) { const size_t nb = (size_t)p->N * p->taps * p->Cpad; hipMemcpy(out.w + off, p->w, nb * 2, hipMemcpyDeviceToDevice); off += nb; }
  return 0;
}

// q_proj / k_proj / v_proj of every layer of a CLIP encoder as one [3H][H] matrix + bias ("<prefix><l>.self_attn.qkv.*");
// alloc = false (agd_lora_set_scale, the text encoder): the fused matrices are rewritten in place from the current q / k / v (biases unchanged)
static int fuse_clip_qkv(agd_ctx* c, const std::string& prefix, int layers, bool alloc = true) {
  for (int l = 0; l < layers; ++l) {
    const std::string a = prefix + std::to_string(l) + ".self_attn.";
    const WMat* q = getW(c, a + "q_proj.weight"); const WMat* k = getW(c, a + "k_proj.weight"); const WMat* v = getW(c, a + "v_proj.weight");
    const float* bq = getV(c, a + "q_proj.bias"); const float* bk = getV(c, a + "k_proj.bias"); const float* bv = getV(c, a + "v_proj.bias");
    if (!q || !k || !v || !bq || !bk || !bv) return -1;
    if (!alloc) {
      auto it = c->W.find(a + "qkv.weight"); if (it == c->W.end()) FAIL("derived form '%sqkv.weight' missing", a.c_str());
      if (concat_rows(c, {q, k, v}, it->second, false)) return -1;
      continue;
    }
    WMat qkv; if (concat_rows(c, {q, k, v}, qkv)) return -1; c->W[a + "qkv.weight"] = qkv;
    float* b = dmalloc<float>(c, (size_t)3 * q->N); if (!b) return -1;
    hipMemcpy(b, bq, (size_t)q->N * 4, hipMemcpyDeviceToDevice); hipMemcpy(b + q->N, bk, (size_t)q->N * 4, hipMemcpyDeviceToDevice);
    hipMemcpy(b + 2 * q->N, bv, (size_t)q->N * 4, hipMemcpyDeviceToDevice);
    c->V[a + "qkv.bias"] = b; c->Vn[a + "qkv.bias"] = 3 * q->N;
  }
  return 0;
}

// A CLIP vision tower with its projection (transformers CLIPVisionModelWithProjection), under the weight names of its owner: the safety
// checker's ("safety.vision_model.vision_model.", config c->vis) or the IP-Adapter's image encoder ("image_encoder.vision_model.", c->ienc)
struct VisTower { const agd_vision_config* v; std::string pre, proj, patch; const char* what; };
static VisTower safety_tower(agd_ctx* c) { return {&c->vis, "safety.vision_model.vision_model.", "safety.visual_projection.weight", "safety.patch_matrix", "safety"}; }
static VisTower image_tower(agd_ctx* c) { return {&c->ienc, "image_encoder.vision_model.", "image_encoder.visual_projection.weight", "image_encoder.patch_matrix", "image encoder"}; }
// an fp32 vision tensor of exactly n elements
static const float* getV_n(agd_ctx* c, const std::string& k, long long n, const char* what = "safety") {
  const float* p = getV(c, k); if (!p) return nullptr;
  if (c->Vn[k] != n) { agd_set_error("'%s' has %d elements, the %s config needs %lld", k.c_str(), c->Vn[k], what, n); return nullptr; }
  return p;
}

// checks every tensor of the tower against its config, fuses q/k/v per layer and builds the zero-padded patch matrix
static int finalize_vision(agd_ctx* c, const VisTower& t) {
  const agd_vision_config& v = *t.v;
  const char* kVisPre = t.pre.c_str(); const char* what = t.what;
  const std::string E = t.pre + "embeddings.";
  const int H = v.hidden, ps = v.patch_size, g = v.image_size / ps, K = 3 * ps * ps, P = v.projection_dim;
  const float* pw = getV_n(c, E + "patch_embedding.weight", (long long)H * K, what); if (!pw) return -1;
  if (!getV_n(c, E + "class_embedding", H, what) || !getV_n(c, E + "position_embedding.weight", (long long)(g * g + 1) * H, what)) return -1;
  for (const char* ln : {"pre_layrnorm.", "post_layernorm."})
    for (const char* wb : {"weight", "bias"}) if (!getV_n(c, std::string(kVisPre) + ln + wb, H, what)) return -1;
  if (!getV_n(c, t.proj, (long long)P * H, what)) return -1;
  for (int l = 0; l < v.layers; ++l) {
    const std::string L = std::string(kVisPre) + "encoder.layers." + std::to_string(l) + ".";
    for (const char* m : {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2"}) {
      const WMat* w = getW(c, L + m + ".weight"); if (!w) return -1;
      const bool fc1 = !strcmp(m, "mlp.fc1"), fc2 = !strcmp(m, "mlp.fc2");
      const int want_n = fc1 ? v.intermediate : H, want_k = fc2 ? v.intermediate : H;
      if (w->N != want_n || w->Cin != want_k) FAIL("'%s%s.weight' is [%d, %d], the %s config needs [%d, %d]", L.c_str(), m, w->N, w->Cin, what, want_n, want_k);
      if (!getV_n(c, L + m + ".bias", want_n, what)) return -1;
    }
    for (const char* ln : {"layer_norm1.", "layer_norm2."})
      for (const char* wb : {"weight", "bias"}) if (!getV_n(c, L + ln + wb, H, what)) return -1;
  }
  if (fuse_clip_qkv(c, std::string(kVisPre) + "encoder.layers.", v.layers)) return -1;
  // the 14 x 14 / 14 conv as a [H][Kpad] GEMM matrix, K = 3 ps ps zero-padded to the 64-multiple the implicit GEMM steps in
  { WMat w; w.N = H; w.Cin = K; w.taps = 1; w.Cpad = (K + 63) / 64 * 64;
    w.w = dmalloc<bf16_t>(c, (size_t)w.N * w.Cpad); if (!w.w) return -1;
    if (launch_convert_weight(pw, w.w, w.N, K, 1, w.Cpad, 0, 0)) return -1;
    c->W[t.patch] = w; }
  return 0;
}

static int finalize_safety(agd_ctx* c) {
  const agd_vision_config& v = c->vis;
  const int P = v.projection_dim, n = v.n_special + v.n_concepts;
  if (finalize_vision(c, safety_tower(c))) return -1;
  const float* sp = getV_n(c, "safety.special_care_embeds", (long long)v.n_special * P); if (!sp) return -1;
  const float* cp = getV_n(c, "safety.concept_embeds", (long long)v.n_concepts * P); if (!cp) return -1;
  // concept rows, L2-normalised once (cosine_distance normalises both sides; the image side is normalised per call)
  std::vector<float> rows((size_t)n * P);
  if (hipMemcpy(rows.data(), sp, (size_t)v.n_special * P * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(rows.data() + (size_t)v.n_special * P, cp, (size_t)v.n_concepts * P * 4, hipMemcpyDeviceToHost) != hipSuccess) FAIL("safety: concept read failed");
  for (int i = 0; i < n; ++i) {
    double ss = 0; for (int j = 0; j < P; ++j) ss += (double)rows[(size_t)i * P + j] * rows[(size_t)i * P + j];
    const double inv = 1.0 / std::max(std::sqrt(ss), 1e-12);
    for (int j = 0; j < P; ++j) rows[(size_t)i * P + j] = (float)(rows[(size_t)i * P + j] * inv);
  }
  c->vis_concepts = dmalloc<float>(c, rows.size()); if (!c->vis_concepts) return -1;
  if (hipMemcpy(c->vis_concepts, rows.data(), rows.size() * 4, hipMemcpyHostToDevice) != hipSuccess) FAIL("safety: concept upload failed");
  return 0;
}

// ControlNet res samples (SD-1.x: 12): conv_in, layers_per_block per level, a downsampler per level but the last; their channel counts
static std::vector<int> controlnet_res_channels(const agd_config& g) {
  std::vector<int> ch{g.block_out_channels[0]};
  for (int i = 0; i < g.n_levels; ++i) {
    for (int j = 0; j < g.layers_per_block; ++j) ch.push_back(g.block_out_channels[i]);
    if (i != g.n_levels - 1) ch.push_back(g.block_out_channels[i]);
  }
  return ch;
}

static int finalize_controlnet(agd_ctx* c) {
  const agd_config& g = c->cfg;
  const agd_controlnet_config& e = c->cnc;
  const std::string u = "controlnet.", E = u + "controlnet_cond_embedding.";
  // ControlNetConditioningEmbedding: conv_in 3 -> e0, per step (c -> c, c -> c' stride 2) as blocks.0 .. blocks.{2 (n - 1) - 1}, conv_out e_last -> C0
  auto want = [&](const std::string& k, int n, int cin) -> int {
    const WMat* w = getW(c, k + ".weight"); if (!w) return -1;
    if (w->N != n || w->Cin != cin || w->taps != 9) FAIL("'%s.weight' is [%d, %d, %d taps], the ControlNet config needs [%d, %d, 3x3]", k.c_str(), w->N, w->Cin, w->taps, n, cin);
    auto b = c->Vn.find(k + ".bias"); if (b == c->Vn.end() || b->second != n) FAIL("'%s.bias' missing or not %d long", k.c_str(), n);
    return 0;
  };
  CK(want(E + "conv_in", e.emb_channels[0], 3));
  for (int i = 0; i + 1 < e.n_emb; ++i) {
    CK(want(E + "blocks." + std::to_string(2 * i), e.emb_channels[i], e.emb_channels[i]));
    CK(want(E + "blocks." + std::to_string(2 * i + 1), e.emb_channels[i + 1], e.emb_channels[i]));
  }
  CK(want(E + "conv_out", g.block_out_channels[0], e.emb_channels[e.n_emb - 1]));
  const std::vector<int> ch = controlnet_res_channels(g);
  c->cn_nres = (int)ch.size();
  std::vector<std::string> keys;
  for (int k = 0; k < c->cn_nres; ++k) keys.push_back(u + "controlnet_down_blocks." + std::to_string(k));
  keys.push_back(u + "controlnet_mid_block");
  std::vector<int> n_of(ch); n_of.push_back(g.block_out_channels[g.n_levels - 1]);
  c->cn_zb_off.clear(); int total = 0;
  for (size_t k = 0; k < keys.size(); ++k) {
    const WMat* w = getW(c, keys[k] + ".weight"); if (!w) return -1;
    if (w->N != n_of[k] || w->Cin != n_of[k] || w->taps != 1) FAIL("'%s.weight' is [%d, %d, %d taps], the UNet needs a 1x1 [%d, %d]", keys[k].c_str(), w->N, w->Cin, w->taps, n_of[k], n_of[k]);
    auto b = c->Vn.find(keys[k] + ".bias"); if (b == c->Vn.end() || b->second != n_of[k]) FAIL("'%s.bias' missing or not %d long", keys[k].c_str(), n_of[k]);
    c->cn_zb_off.push_back(total); total += n_of[k];
  }
  c->cn_zb = dmalloc<float>(c, total); c->cn_zbs = dmalloc<float>(c, total); if (!c->cn_zb || !c->cn_zbs) return -1;
  for (size_t k = 0; k < keys.size(); ++k)
    if (hipMemcpy(c->cn_zb + c->cn_zb_off[k], c->V[keys[k] + ".bias"], (size_t)n_of[k] * 4, hipMemcpyDeviceToDevice) != hipSuccess) FAIL("controlnet: bias copy failed");
  c->cn_zb_total = total; c->cn_zscale = NAN;
  return 0;
}

// T2I-Adapter "full_adapter": the config must fit the UNet it feeds, and every matrix of adapter.conv_in / adapter.body.{i}.in_conv /
// adapter.body.{i}.resnets.{j}.block1 (3x3) / block2 (1x1) must be present with the config's shape
static int finalize_adapter(agd_ctx* c) {
  const agd_config& g = c->cfg;
  const agd_adapter_config& e = c->adc;
  if (e.n_channels != g.n_levels) FAIL("adapter: channels has %d entries, the UNet has %d levels", e.n_channels, g.n_levels);
  for (int i = 0; i < e.n_channels; ++i)
    if (e.channels[i] != g.block_out_channels[i]) FAIL("adapter: channels[%d] = %d, the UNet's block_out_channels[%d] = %d", i, e.channels[i], i, g.block_out_channels[i]);
  const int vf = 1 << (g.vae_n_levels - 1);
  if (e.downscale_factor != vf) FAIL("adapter: downscale_factor = %d, the VAE's scale factor is %d", e.downscale_factor, vf);
  auto want = [&](const std::string& k, int n, int cin, int taps) -> int {
    const WMat* w = getW(c, k + ".weight"); if (!w) return -1;
    if (w->N != n || w->Cin != cin || w->taps != taps) FAIL("'%s.weight' is [%d, %d, %d taps], the adapter config needs [%d, %d, %d taps]", k.c_str(), w->N, w->Cin, w->taps, n, cin, taps);
    auto b = c->Vn.find(k + ".bias"); if (b == c->Vn.end() || b->second != n) FAIL("'%s.bias' missing or not %d long", k.c_str(), n);
    return 0;
  };
  const std::string A = "adapter.adapter.";
  CK(want(A + "conv_in", e.channels[0], e.in_channels * e.downscale_factor * e.downscale_factor, 9));
  for (int i = 0; i < e.n_channels; ++i) {
    const std::string Bk = A + "body." + std::to_string(i) + ".";
    const int cin = i ? e.channels[i - 1] : e.channels[0], co = e.channels[i];
    if (cin != co) CK(want(Bk + "in_conv", co, cin, 1));
    for (int j = 0; j < e.num_res_blocks; ++j) {
      CK(want(Bk + "resnets." + std::to_string(j) + ".block1", co, co, 9));
      CK(want(Bk + "resnets." + std::to_string(j) + ".block2", co, co, 1));
    }
  }
  return 0;
}

// The transformer blocks, in the order agd_finalize registers their cross-attention layers (daam's: up, down, mid), the ControlNet's after
// them: (prefix "...attentions.<j>.", level)
static std::vector<std::pair<std::string, int>> transformer_prefixes(agd_ctx* c) {
  const agd_config& g = c->cfg;
  std::vector<std::pair<std::string, int>> tf;
  const int nl = g.n_levels;
  for (int i = 0; i < nl; ++i) { const int lvl = nl - 1 - i;
    if (g.down_cross[lvl]) for (int j = 0; j < g.layers_per_block + 1; ++j) tf.push_back({"unet.up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", lvl}); }
  for (int i = 0; i < nl; ++i)
    if (g.down_cross[i]) for (int j = 0; j < g.layers_per_block; ++j) tf.push_back({"unet.down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", i});
  tf.push_back({"unet.mid_block.attentions.0.", nl - 1});
  if (c->cn_on) {                                   // the ControlNet's blocks: after every recorder layer (xl order is daam's for the UNet's)
    for (int i = 0; i < nl; ++i)
      if (g.down_cross[i]) for (int j = 0; j < g.layers_per_block; ++j) tf.push_back({"controlnet.down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", i});
    tf.push_back({"controlnet.mid_block.attentions.0.", nl - 1});
  }
  return tf;
}

// Every form one transformer block derives from its raw matrices: the fused QKV, the cross K/V (and its XLayer), the pre-multiplied attn2
// parts, the three LayerNorm folds, [Wp W2 | Wp] with Wp b2 + bp, and the fragment orders.  alloc = true (agd_finalize) allocates them;
// alloc = false (agd_lora_set_scale) rewrites the same blocks in place from the current raw matrices through the same launches, so the two
// cannot drift.  scratch: nullptr = load-time blocks, allocated and freed here; else 8 C C bf16 of room the caller owns.
static int derive_tblock(agd_ctx* c, const std::string& pre, int level, bool alloc, bf16_t* scratch) {
  const agd_config& g = c->cfg;
  // the destination of a derived matrix / vector: a fresh block at finalize, the existing one when rewritten
  auto wbuf = [&](const std::string& key, size_t n) -> bf16_t* {
    if (alloc) return dmalloc<bf16_t>(c, n);
    auto it = c->W.find(key);
    if (it == c->W.end() || !it->second.w) { agd_set_error("derived form '%s' missing", key.c_str()); return nullptr; }
    return it->second.w;
  };
  auto vbuf = [&](const std::string& key, size_t n) -> float* {
    if (alloc) return dmalloc<float>(c, n);
    auto it = c->V.find(key);
    if (it == c->V.end() || !it->second) { agd_set_error("derived form '%s' missing", key.c_str()); return nullptr; }
    return it->second;
  };
  {
    const std::string t = pre + "transformer_blocks.0.";
    const WMat* q = getW(c, t + "attn1.to_q.weight"); const WMat* k = getW(c, t + "attn1.to_k.weight"); const WMat* v = getW(c, t + "attn1.to_v.weight");
    if (!q || !k || !v) return fail_ctx(c);
    if (alloc) { WMat qkv; API_CK(c, concat_rows(c, {q, k, v}, qkv)); c->W[t + "attn1.qkv"] = qkv; }
    else { auto it = c->W.find(t + "attn1.qkv"); if (it == c->W.end()) FAIL("derived form '%sattn1.qkv' missing", t.c_str());
      API_CK(c, concat_rows(c, {q, k, v}, it->second, false)); }
    const WMat* ck = getW(c, t + "attn2.to_k.weight"); const WMat* cv = getW(c, t + "attn2.to_v.weight");
    if (!ck || !cv) return fail_ctx(c);
    XLayer xl_new; XLayer* xp = &xl_new;
    if (alloc) {
      XLayer& xl = xl_new; xl.name = t + "attn2"; xl.C = q->N; xl.level = level; xl.heads = g.num_heads[level];
      xl.mid = pre.find("mid_block") != std::string::npos;
      xl.cn = pre.compare(0, 11, "controlnet.") == 0;
      API_CK(c, concat_rows(c, {ck, cv}, xl.wkv));
      if (xl.C % xl.heads) { agd_set_error("%s: C %d not divisible by heads %d", xl.name.c_str(), xl.C, xl.heads); return fail_ctx(c); }
    } else {
      auto it = c->xl_idx.find(t + "attn2"); if (it == c->xl_idx.end()) FAIL("cross-attn layer %sattn2 not registered", t.c_str());
      xp = &c->xl[it->second];
      API_CK(c, concat_rows(c, {ck, cv}, xp->wkv, false));
      xp->wqT.w = nullptr; xp->wkvT.w = nullptr; xp->woT.w = nullptr;     // the backward's transposes: rebuilt (same buffers) on next use
    }
    XLayer& xl = *xp;
    // pre-multiplied attn2 (xattn_pre.hip) where it saves work: H x 80 padded token columns <= C / 2, i.e. head dim >= 160 (SD-1.x: the C = 1280 blocks)
    { const WMat* wq2 = getW(c, t + "attn2.to_q.weight"); const WMat* wo2 = getW(c, t + "attn2.to_out.0.weight");
      auto be2 = c->V.find(t + "norm2.bias");
      const int C2 = xl.C, D2 = C2 / xl.heads;
      // (option bit 1, off by default: also where the columns equal C -- head dim 80, the C = 640 blocks: no fewer MACs, but three full-chip launches instead of the
      //  half-chip chain kernel)
      if (wq2 && wo2 && be2 != c->V.end() && D2 % 8 == 0 && C2 % 160 == 0 && C2 % 64 == 0 && (xl.heads * XATTN_TP) % 64 == 0 && xl.heads * XATTN_TP <= C2 &&
          wq2->taps == 1 && wq2->N == C2 && wq2->Cpad == C2 && wo2->taps == 1 && wo2->N == C2 && wo2->Cpad == C2) {
        if (alloc) { xl.pm_wqT = dmalloc<bf16_t>(c, (size_t)C2 * C2); xl.pm_wqb = dmalloc<float>(c, C2); }
        if (!xl.pm_wqT || !xl.pm_wqb) return fail_ctx(c);
        API_CK(c, launch_transpose_bf16(wq2->w, C2, C2, xl.pm_wqT, 0));
        API_CK(c, launch_matvec_bf16(wq2->w, be2->second, xl.pm_wqb, C2, C2, 0));       // (Wq beta)[(h,d)]
      } }
    if (alloc) { c->xl_idx[xl.name] = (int)c->xl.size(); c->xl.push_back(xl); }
    // LayerNorm folded into the three GEMMs it feeds: W' = W diag(gamma), colsum(W'), bias' = bias + W beta
    struct Fold { const char* w; const char* bias; const char* ln; int geglu; };
    const Fold folds[3] = {{"attn1.qkv", nullptr, "norm1", 0}, {"attn2.to_q.weight", nullptr, "norm2", 0}, {"ff.net.0.proj.weight", "ff.net.0.proj.bias", "norm3", 16}};
    for (const Fold& f : folds) {
      const WMat* w = getW(c, t + f.w); const float* ga = getV(c, t + f.ln + ".weight"); const float* be = getV(c, t + f.ln + ".bias");
      if (!w || !ga || !be) return fail_ctx(c);
      const float* b0 = f.bias ? getV(c, t + f.bias) : nullptr;
      if (f.bias && !b0) return fail_ctx(c);
      if (w->taps != 1 || w->Cpad != w->Cin) { agd_set_error("%s: cannot fold LayerNorm (padded K)", (t + f.w).c_str()); return fail_ctx(c); }
      const std::string k = t + f.w + ".lnfold";
      WMat wf = *w; wf.w = wbuf(k, (size_t)w->N * w->Cpad);
      float* cs = vbuf(k + ".cs", w->N); float* bf = vbuf(k + ".bias", w->N);
      if (!wf.w || !cs || !bf) return fail_ctx(c);
      API_CK(c, launch_ln_fold_weight(w->w, ga, be, b0, w->N, w->Cpad, f.geglu, wf.w, cs, bf, 0));
      if (alloc) { c->W[k] = wf; c->V[k + ".cs"] = cs; c->V[k + ".bias"] = bf; c->Vn[k + ".cs"] = w->N; c->Vn[k + ".bias"] = w->N; }
    }
    if (q->N == 1280) {                                 // the C = 1280 GEGLU matrix once more in igemm_wreg.h's fragment order (option wreg_mask bit 0)
      auto it = c->W.find(t + "ff.net.0.proj.weight.lnfold");
      if (it != c->W.end() && it->second.taps == 1 && it->second.N % 256 == 0) {
        WMat& wm_ = it->second;
        if (alloc) wm_.wfrag = dmalloc<bf16_t>(c, (size_t)wm_.N * wm_.Cpad);
        if (!wm_.wfrag) return fail_ctx(c);
        API_CK(c, launch_frag_order_w(wm_.w, wm_.wfrag, wm_.N, wm_.Cpad, 4, wm_.Cpad, 0)); wm_.wfrag_ni = 4;
      }
    }
    // ff.net.2 and proj_out pre-multiplied: [Wp W2 | Wp] (rows of 5 C) and Wp b2 + bp, for the blocks whose feed-forward runs as separate launches
    { const WMat* w2 = getW(c, t + "ff.net.2.weight"); const WMat* wp = getW(c, pre + "proj_out.weight");
      auto b2 = c->V.find(t + "ff.net.2.bias"); auto bp = c->V.find(pre + "proj_out.bias");
      if (w2 && wp && b2 != c->V.end() && bp != c->V.end() && w2->taps == 1 && wp->taps == 1 && wp->N == q->N && wp->Cpad == q->N && w2->N == q->N && w2->Cpad == 4 * q->N) {
        const int C = q->N;
        bf16_t* w2t = alloc ? dmalloc<bf16_t>(c, (size_t)4 * C * C) : scratch;
        WMat wc = *wp; wc.N = C; wc.taps = 1; wc.Cpad = 5 * C; wc.Cin = 5 * C; wc.wfrag = nullptr; wc.wfrag_ni = 0; wc.sc_cols = 0;
        wc.w = wbuf(pre + "ffproj.weight", (size_t)C * 5 * C); float* bc = vbuf(pre + "ffproj.bias", C);
        if (!w2t || !wc.w || !bc) return fail_ctx(c);
        API_CK(c, launch_transpose_bf16(w2->w, C, 4 * C, w2t, 0));                       // W2 [C][4C] -> [4C][C]
        { WMat wt; wt.w = w2t; wt.N = 4 * C; wt.Cin = C; wt.Cpad = C; wt.taps = 1;        // (Wp W2)[n][k] = sum_j Wp[n][j] W2T[k][j]: Wp's rows as the activation rows
          GemmOpt o; o.ldo = 5 * C;
          API_CK(c, run_conv(c, 0, wp->w, C, nullptr, 0, 1, 1, C, wt, 1, wc.w, o, c->zero_page)); }
        if (hipMemcpy2D(wc.w + 4 * C, (size_t)5 * C * 2, wp->w, (size_t)C * 2, (size_t)C * 2, C, hipMemcpyDeviceToDevice) != hipSuccess) { agd_set_error("finalize: ff/proj matrix assembly failed"); return fail_ctx(c); }
        std::vector<unsigned short> hw((size_t)C * C); std::vector<float> hb2(C), hbp(C);
        if (hipMemcpy(hw.data(), wp->w, (size_t)C * C * 2, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hb2.data(), b2->second, C * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hbp.data(), bp->second, C * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { agd_set_error("finalize: ff/proj bias read failed"); return fail_ctx(c); }
        for (int n = 0; n < C; ++n) {
          double a = hbp[n];
          for (int j = 0; j < C; ++j) { unsigned u = (unsigned)hw[(size_t)n * C + j] << 16; float f; memcpy(&f, &u, 4); a += (double)f * hb2[j]; }
          hbp[n] = (float)a;
        }
        if (hipMemcpy(bc, hbp.data(), C * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { agd_set_error("finalize: ff/proj bias write failed"); return fail_ctx(c); }
        if (alloc) { c->W[pre + "ffproj.weight"] = wc; c->V[pre + "ffproj.bias"] = bc; c->Vn[pre + "ffproj.bias"] = C; }
        if (C == 320) {                                   // the fused feed-forward kernel's form of it: Wp W2 alone, in ff.net.2's fragment order
          bf16_t* tmpc = alloc ? dmalloc<bf16_t>(c, (size_t)C * 4 * C) : scratch + (size_t)4 * C * C; WMat f2p = *w2; f2p.wfrag = nullptr; f2p.wfrag_ni = 0;
          f2p.w = wbuf(t + "ff.w2p.frag", (size_t)C * 4 * C);
          if (!tmpc || !f2p.w) return fail_ctx(c);
          if (hipMemcpy2D(tmpc, (size_t)4 * C * 2, wc.w, (size_t)5 * C * 2, (size_t)4 * C * 2, C, hipMemcpyDeviceToDevice) != hipSuccess) { agd_set_error("finalize: Wp W2 copy failed"); return fail_ctx(c); }
          API_CK(c, launch_frag_order_w(tmpc, f2p.w, C, 4 * C, C / 64, 128, 0));
          if (alloc) c->W[t + "ff.w2p.frag"] = f2p;
          hipDeviceSynchronize(); if (alloc) dfree(c, tmpc);          // load-time scratch
        }
        hipDeviceSynchronize(); if (alloc) dfree(c, w2t);
      } }
    // fused row-panel kernels (tblock.hip, C = 320 blocks): the matrices once more in MFMA fragment order
    if (q->N == 320 || q->N == 640) {                 // (C = 640: the attn2 chain only -- a wave's GEMM tile is 80 columns whatever C: NI = 5)
      const int C = q->N;
      const WMat* w1 = getW(c, t + "ff.net.0.proj.weight.lnfold"); const WMat* w2 = getW(c, t + "ff.net.2.weight");
      if (!w1 || !w2) return fail_ctx(c);
      if (C == 320 && w1->N == 8 * C && w1->Cpad == C && w2->N == C && w2->Cpad == 4 * C && w2->taps == 1) {
        WMat f1 = *w1, f2 = *w2;
        f1.w = wbuf(t + "ff.w1.frag", (size_t)w1->N * C); f2.w = wbuf(t + "ff.w2.frag", (size_t)C * 4 * C);
        if (!f1.w || !f2.w) return fail_ctx(c);
        API_CK(c, launch_frag_order_w1(w1->w, f1.w, C, 4 * C, 0));
        API_CK(c, launch_frag_order_w(w2->w, f2.w, C, 4 * C, C / 64, 128, 0));
        if (alloc) { c->W[t + "ff.w1.frag"] = f1; c->W[t + "ff.w2.frag"] = f2; }
        const WMat* wp = getW(c, pre + "proj_out.weight");
        if (!wp) return fail_ctx(c);
        if (wp->N == C && wp->Cpad == C && wp->taps == 1) {
          WMat fp_ = *wp; fp_.w = wbuf(pre + "proj_out.frag", (size_t)C * C); if (!fp_.w) return fail_ctx(c);
          API_CK(c, launch_frag_order_w(wp->w, fp_.w, C, C, C / 64, C, 0));
          if (alloc) c->W[pre + "proj_out.frag"] = fp_;
        }

      }
      if (C == 640) {                                   // proj_in / proj_out once more in igemm_wreg.h's fragment order (option wreg_mask bit 1)
        for (const char* nm : {"proj_in.weight", "proj_out.weight"}) {
          auto it = c->W.find(pre + nm); if (it == c->W.end()) { agd_set_error("finalize: missing weight '%s%s'", pre.c_str(), nm); return fail_ctx(c); }
          WMat& wm_ = it->second;
          if (wm_.taps == 1 && wm_.N % 128 == 0 && wm_.Cpad % 64 == 0) {
            if (alloc) wm_.wfrag = dmalloc<bf16_t>(c, (size_t)wm_.N * wm_.Cpad);
            if (!wm_.wfrag) return fail_ctx(c);
            API_CK(c, launch_frag_order_w(wm_.w, wm_.wfrag, wm_.N, wm_.Cpad, 2, wm_.Cpad, 0)); wm_.wfrag_ni = 2;
          }
        }
      }
      { const WMat* wi = getW(c, pre + "proj_in.weight");
        if (!wi) return fail_ctx(c);
        if (wi->N == C && wi->Cpad == C && wi->taps == 1) {
          WMat fi = *wi; fi.w = wbuf(pre + "proj_in.frag", (size_t)C * C); if (!fi.w) return fail_ctx(c);
          API_CK(c, launch_frag_order_w(wi->w, fi.w, C, C, 5, C, 0));
          if (alloc) c->W[pre + "proj_in.frag"] = fi;
        } }
      const WMat* wq = getW(c, t + "attn2.to_q.weight"); const WMat* wo = getW(c, t + "attn2.to_out.0.weight");
      if (!wq || !wo) return fail_ctx(c);
      if (wq->N == C && wq->Cpad == C && wq->taps == 1 && wo->N == C && wo->Cpad == C && wo->taps == 1 && xl.heads == 8) {
        WMat fq = *wq, fo = *wo;
        fq.w = wbuf(t + "attn2.to_q.frag", (size_t)C * C); fo.w = wbuf(t + "attn2.to_out.frag", (size_t)C * C);
        if (!fq.w || !fo.w) return fail_ctx(c);
        API_CK(c, launch_frag_order_w(wq->w, fq.w, C, C, 5, C, 0));
        API_CK(c, launch_frag_order_w(wo->w, fo.w, C, C, 5, C, 0));
        if (alloc) { c->W[t + "attn2.to_q.frag"] = fq; c->W[t + "attn2.to_out.frag"] = fo; }
        { const WMat* wqkv = getW(c, t + "attn1.qkv"); if (!wqkv) return fail_ctx(c);
          if (wqkv->N == 3 * C && wqkv->Cpad == C && wqkv->taps == 1) {
            WMat fqkv = *wqkv; fqkv.w = wbuf(t + "attn1.qkv.frag", (size_t)3 * C * C); if (!fqkv.w) return fail_ctx(c);
            API_CK(c, launch_frag_order_w(wqkv->w, fqkv.w, 3 * C, C, 5, C, 0));
            if (alloc) c->W[t + "attn1.qkv.frag"] = fqkv;
          } }
        const WMat* wo1 = getW(c, t + "attn1.to_out.0.weight");
        if (!wo1) return fail_ctx(c);
        if (wo1->N == C && wo1->Cpad == C && wo1->taps == 1) {
          WMat f1o = *wo1; f1o.w = wbuf(t + "attn1.to_out.frag", (size_t)C * C); if (!f1o.w) return fail_ctx(c);
          API_CK(c, launch_frag_order_w(wo1->w, f1o.w, C, C, 5, C, 0));
          if (alloc) c->W[t + "attn1.to_out.frag"] = f1o;
        }
      }
    }
  }
  return 0;
}

// GLIGEN: PositionNet linears.{0,2,4} = [512][positive_len + 8 F], [512][512], [cross_attention_dim][512] and the two null features; in every
// UNet transformer block a fuser whose linear maps cross_attention_dim -> C, with q / k / v / to_out [C][C], GEGLU [8C][C], ff.net.2 [C][4C]
static int finalize_gligen(agd_ctx* c) {
  const agd_gligen_config& e = c->glc;
  const int Dc = c->cfg.cross_attention_dim, Pin = e.positive_len + 8 * e.fourier_freqs;
  auto want = [&](const std::string& k, int n, int cin) -> int {
    const WMat* w = getW(c, k + ".weight"); if (!w) return -1;
    if (w->N != n || w->Cin != cin || w->taps != 1) FAIL("'%s.weight' is [%d, %d], GLIGEN needs [%d, %d]", k.c_str(), w->N, w->Cin, n, cin);
    return 0;
  };
  auto wantv = [&](const std::string& k, int n) -> int {
    auto it = c->Vn.find(k); if (it == c->Vn.end() || it->second != n) FAIL("'%s' missing or not %d long", k.c_str(), n);
    return 0;
  };
  const std::string P = "unet.position_net.";
  CK(want(P + "linears.0", 512, Pin)); CK(wantv(P + "linears.0.bias", 512));
  CK(want(P + "linears.2", 512, 512)); CK(wantv(P + "linears.2.bias", 512));
  CK(want(P + "linears.4", Dc, 512)); CK(wantv(P + "linears.4.bias", Dc));
  CK(wantv(P + "null_positive_feature", e.positive_len)); CK(wantv(P + "null_position_feature", 8 * e.fourier_freqs));
  if (getW(c, P + "linears.0.weight")->Cpad != Pin) FAIL("gligen: positive_len + %d = %d is not a multiple of 64", 8 * e.fourier_freqs, Pin);
  c->gl_f.clear(); c->gl_idx.clear();
  for (auto& pr : transformer_prefixes(c)) {
    if (pr.first.compare(0, 5, "unet.") != 0) continue;
    const std::string t = pr.first + "transformer_blocks.0.fuser.";
    const WMat* q = getW(c, t + "attn.to_q.weight"); if (!q) return -1;
    Fuser f; f.pre = pr.first; f.C = q->N; f.heads = c->cfg.num_heads[pr.second];
    const int C = f.C;
    if (C % f.heads) FAIL("gligen: %s C %d not divisible by %d heads", t.c_str(), C, f.heads);
    CK(want(t + "linear", C, Dc)); CK(wantv(t + "linear.bias", C));
    CK(want(t + "attn.to_q", C, C)); CK(want(t + "attn.to_k", C, C)); CK(want(t + "attn.to_v", C, C));
    CK(want(t + "attn.to_out.0", C, C)); CK(wantv(t + "attn.to_out.0.bias", C));
    CK(want(t + "ff.net.0.proj", 8 * C, C)); CK(wantv(t + "ff.net.0.proj.bias", 8 * C));
    CK(want(t + "ff.net.2", C, 4 * C)); CK(wantv(t + "ff.net.2.bias", C));
    for (const char* n : {"norm1", "norm2"}) { CK(wantv(t + n + ".weight", C)); CK(wantv(t + n + ".bias", C)); }
    CK(wantv(t + "alpha_attn", 1)); CK(wantv(t + "alpha_dense", 1));
    CK(concat_rows(c, {q, getW(c, t + "attn.to_k.weight"), getW(c, t + "attn.to_v.weight")}, f.wqkv));
    CK(concat_rows(c, {getW(c, t + "attn.to_k.weight"), getW(c, t + "attn.to_v.weight")}, f.wkv));
    float al[2];
    if (hipMemcpy(&al[0], c->V[t + "alpha_attn"], 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&al[1], c->V[t + "alpha_dense"], 4, hipMemcpyDeviceToHost) != hipSuccess) FAIL("gligen: gate read failed");
    f.ta = tanhf(al[0]); f.td = tanhf(al[1]);
    std::vector<float> bo(C), b2(C);
    if (hipMemcpy(bo.data(), c->V[t + "attn.to_out.0.bias"], (size_t)C * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(b2.data(), c->V[t + "ff.net.2.bias"], (size_t)C * 4, hipMemcpyDeviceToHost) != hipSuccess) FAIL("gligen: bias read failed");
    for (int i = 0; i < C; ++i) { bo[i] *= f.ta; b2[i] *= f.td; }
    f.bo_s = dmalloc<float>(c, C); f.b2_s = dmalloc<float>(c, C); if (!f.bo_s || !f.b2_s) return -1;
    if (hipMemcpy(f.bo_s, bo.data(), (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(f.b2_s, b2.data(), (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess) FAIL("gligen: bias write failed");
    c->gl_idx[f.pre] = (int)c->gl_f.size(); c->gl_f.push_back(f);
  }
  return 0;
}

AGD_API int agd_finalize(agd_ctx* c) {
  if (!c) return -1;
  hipSetDevice(c->device);
  const agd_config& g = c->cfg;
  // ---- transformer blocks: fused QKV + cross K/V weights, recorder layers (daam order: up, down, mid), every derived form
  for (auto& pr : transformer_prefixes(c)) API_CK(c, derive_tblock(c, pr.first, pr.second, true, nullptr));
  // ---- the UNet's upsampling convs once more as the merged phase matrices [4 Cout][4 taps][Cin] (+ the bias four times)
  { std::vector<std::string> keys;
    const std::string tail = "upsamplers.0.conv.weight";
    for (auto& kv : c->W) if (kv.first.size() > tail.size() && kv.first.compare(kv.first.size() - tail.size(), tail.size(), tail) == 0)
      keys.push_back(kv.first.substr(0, kv.first.size() - 6));                 // "... .conv." (UNet and VAE decoder)
    for (const std::string& k : keys) {
      const WMat* w = getW(c, k + "weight"); auto bi = c->V.find(k + "bias");
      if (!w || bi == c->V.end()) return fail_ctx(c);
      if (w->taps != 9 || (w->Cpad & 63) || (w->N % 160 && w->N % 128)) continue;
      WMat w4 = *w; w4.N = 4 * w->N; w4.taps = 4; w4.wfrag = nullptr; w4.wfrag_ni = 0; w4.sc_cols = 0;
      w4.w = dmalloc<bf16_t>(c, (size_t)w4.N * 4 * w->Cpad); float* b4 = dmalloc<float>(c, w4.N);
      if (!w4.w || !b4) return fail_ctx(c);
      API_CK(c, launch_upsample_phase_weight(w->w, w4.w, w->N, w->Cpad, 0));
      for (int ph = 0; ph < 4; ++ph)
        if (hipMemcpy(b4 + (size_t)ph * w->N, bi->second, w->N * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess) { agd_set_error("finalize: phase bias copy failed"); return fail_ctx(c); }
      c->W[k + "phases"] = w4; c->V[k + "phases.bias"] = b4; c->Vn[k + "phases.bias"] = w4.N;
    } }
  // ---- UNet resnets with a conv_shortcut: conv2's matrix once more with the shortcut's columns appended to every row, and the two biases summed
  { std::vector<std::string> pres;
    const std::string tail = "conv_shortcut.weight";
    for (auto& kv : c->W) if ((kv.first.compare(0, 5, "unet.") == 0 || kv.first.compare(0, 11, "controlnet.") == 0) && kv.first.size() > tail.size() && kv.first.compare(kv.first.size() - tail.size(), tail.size(), tail) == 0)
      pres.push_back(kv.first.substr(0, kv.first.size() - tail.size()));
    for (const std::string& pre : pres) {
      const WMat* w2 = getW(c, pre + "conv2.weight"); const WMat* ws = getW(c, pre + "conv_shortcut.weight");
      auto b2 = c->V.find(pre + "conv2.bias"); auto bs = c->V.find(pre + "conv_shortcut.bias");
      if (!w2 || !ws || b2 == c->V.end() || bs == c->V.end()) return fail_ctx(c);
      if (w2->taps != 9 || ws->taps != 1 || w2->N != ws->N || (ws->Cpad & 63) || (w2->Cpad & 63)) continue;
      const size_t k2 = (size_t)9 * w2->Cpad, ks = (size_t)ws->Cpad;
      WMat f = *w2; f.sc_cols = (int)ks; f.wfrag = nullptr; f.wfrag_ni = 0;
      f.w = dmalloc<bf16_t>(c, (size_t)f.N * (k2 + ks)); float* fb = dmalloc<float>(c, f.N);
      if (!f.w || !fb) return fail_ctx(c);
      if (hipMemcpy2D(f.w, (k2 + ks) * 2, w2->w, k2 * 2, k2 * 2, f.N, hipMemcpyDeviceToDevice) != hipSuccess ||
          hipMemcpy2D(f.w + k2, (k2 + ks) * 2, ws->w, ks * 2, ks * 2, f.N, hipMemcpyDeviceToDevice) != hipSuccess) { agd_set_error("finalize: shortcut weight concat failed"); return fail_ctx(c); }
      std::vector<float> ha(f.N), hb(f.N);
      if (hipMemcpy(ha.data(), b2->second, f.N * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hb.data(), bs->second, f.N * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { agd_set_error("finalize: bias read failed"); return fail_ctx(c); }
      for (int i = 0; i < f.N; ++i) ha[i] += hb[i];
      if (hipMemcpy(fb, ha.data(), f.N * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { agd_set_error("finalize: bias write failed"); return fail_ctx(c); }
      c->W[pre + "conv2.sc"] = f; c->V[pre + "conv2.sc.bias"] = fb; c->Vn[pre + "conv2.sc.bias"] = f.N;
    } }
  // ---- all time_emb_proj stacked into one [sum Cout][4*dim] matrix; the ControlNet's (its own time embedding feeds them) into a second one
  for (const bool cn : {false, true}) {
    if (cn && !c->cn_on) break;
    WMat& all = cn ? c->cn_tproj_all : c->tproj_all; float*& bias = cn ? c->cn_tproj_bias : c->tproj_bias;
    float*& out = cn ? c->cn_tproj_out : c->tproj_out; int& total_out = cn ? c->cn_tproj_total : c->tproj_total;
    std::vector<const WMat*> parts; std::vector<std::string> pres; int total = 0;
    for (auto& kv : c->W)
      if (ends_with(kv.first, "time_emb_proj.weight") && (kv.first.compare(0, 11, "controlnet.") == 0) == cn) pres.push_back(kv.first.substr(0, kv.first.size() - strlen("time_emb_proj.weight")));
    std::sort(pres.begin(), pres.end());
    for (auto& p : pres) { const WMat* w = getW(c, p + "time_emb_proj.weight"); parts.push_back(w); c->tproj_off[p] = total; total += w->N; }
    if (!parts.empty()) {
      API_CK(c, concat_rows(c, parts, all)); total_out = total;
      bias = dmalloc<float>(c, total); out = dmalloc<float>(c, total);
      if (!bias || !out) return fail_ctx(c);
      for (auto& p : pres) { const float* b = getV(c, p + "time_emb_proj.bias"); if (!b) return fail_ctx(c);
        hipMemcpy(bias + c->tproj_off[p], b, (size_t)c->Vn[p + "time_emb_proj.bias"] * 4, hipMemcpyDeviceToDevice); }
    } else if (cn) { agd_set_error("finalize: the ControlNet has no time_emb_proj weights"); return fail_ctx(c); }
  }
  { const int dim = g.block_out_channels[0];
    c->temb_buf = dmalloc<float>(c, (size_t)dim * 9); if (!c->temb_buf) return fail_ctx(c); }
  // ---- CLIP text encoder: fused q/k/v projection per layer
  API_CK(c, fuse_clip_qkv(c, "text.encoder.layers.", g.text_layers));
  // ---- safety checker: the vision tower's fused q/k/v, the zero-padded patch matrix, the normalised concept rows
  if (c->vis_on) API_CK(c, finalize_safety(c));
  // ---- ControlNet: the conditioning embedding's shapes, the zero convs' biases back to back
  if (c->cn_on) API_CK(c, finalize_controlnet(c));
  // ---- GLIGEN: the PositionNet's shapes, every fuser's fused projections, gates and pre-scaled biases
  if (c->gl_on) API_CK(c, finalize_gligen(c));
  // ---- T2I-Adapter: the config against the UNet's, every matrix's shape
  if (c->ad_on) API_CK(c, finalize_adapter(c));
  hipDeviceSynchronize();
  c->finalized = true;
  return 0;
}

static hipStream_t S(void* s) { return (hipStream_t)s; }
static int need_final(agd_ctx* c) { if (!c) { agd_set_error("null ctx"); return -1; } if (!c->finalized) { agd_set_error("agd_finalize not called"); return -1; } hipSetDevice(c->device); return 0; }

static int project_context(agd_ctx* c, hipStream_t st, int batch2, int tokens);
AGD_API int agd_set_context(agd_ctx* c, const float* ctx_emb, int batch2, int tokens, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  const int Dc = c->cfg.cross_attention_dim;
  if (tokens > AGD_MAX_CONTEXT_TOKENS) { agd_set_error("set_context: tokens %d > %d unsupported", tokens, AGD_MAX_CONTEXT_TOKENS); return fail_ctx(c); }
  if (batch2 < 1 || tokens < 1) { agd_set_error("set_context: batch2 %d tokens %d", batch2, tokens); return fail_ctx(c); }
  // buffers only ever grow (capacity-tracked); a shorter/smaller context reuses the same blocks
  API_CK(c, c->ctxb.ensure((size_t)batch2 * tokens * Dc * 2)); c->ctx_bf16 = c->ctxb.as<bf16_t>();
  for (auto& xl : c->xl) { API_CK(c, xl.kvb.ensure((size_t)batch2 * tokens * 2 * xl.C * 2)); xl.kv = xl.kvb.as<bf16_t>(); }
  c->ctx_B2 = batch2; c->ctx_T = tokens;
  deepcache_invalidate(c);                              // (a captured hidden state belongs to the context it was computed under)
  API_CK(c, launch_f32_to_bf16(ctx_emb, c->ctx_bf16, (long long)batch2 * tokens * Dc, st));
  API_CK(c, project_context(c, st, batch2, tokens));
  return 0;
}
// the per-layer K/V rows (and, where that form runs, the pre-multiplied attn2 products) of the bf16 context [batch2][tokens][Dc] in ctx_bf16
static int project_context(agd_ctx* c, hipStream_t st, int batch2, int tokens) {
  const int Dc = c->cfg.cross_attention_dim;
  for (auto& xl : c->xl) { API_CK(c, xl.kvb.ensure((size_t)batch2 * tokens * 2 * xl.C * 2)); xl.kv = xl.kvb.as<bf16_t>(); }
  c->ctx_B2 = batch2; c->ctx_T = tokens;
  for (auto& xl : c->xl) {
    GemmOpt o;
    API_CK(c, run_conv(c, st, c->ctx_bf16, Dc, nullptr, 0, 1, 1, batch2 * tokens, xl.wkv, 1, xl.kv, o, c->zero_page));
    // the context products of the pre-multiplied attn2 form, once per prompt batch (xattn_pre.hip)
    xl.pm_ready = false;
    if (c->opt_xpre && xl.pm_wqT && tokens <= XATTN_TP && ((c->opt_xpre & 2) || xl.heads * XATTN_TP * 2 <= xl.C)) {
      const std::string t = xl.name.substr(0, xl.name.size() - 5);          // "...transformer_blocks.0."
      const WMat* wo2 = getW(c, t + "attn2.to_out.0.weight"); const float* g2 = getV(c, t + "norm2.weight");
      if (!wo2 || !g2) { agd_set_error("%s: pre-multiplied form without attn2.to_out.0.weight / norm2.weight", xl.name.c_str()); return fail_ctx(c); }
      const size_t HT = (size_t)xl.heads * XATTN_TP;
      API_CK(c, xl.pm_kppb.ensure((size_t)batch2 * HT * xl.C * 2)); API_CK(c, xl.pm_vppb.ensure((size_t)batch2 * HT * xl.C * 2)); API_CK(c, xl.pm_csb.ensure((size_t)batch2 * HT * 2 * sizeof(float)));
      xl.pm_kpp = xl.pm_kppb.as<bf16_t>(); xl.pm_vpp = xl.pm_vppb.as<bf16_t>(); xl.pm_kcs = xl.pm_csb.as<float>(); xl.pm_kbs = xl.pm_kcs + (size_t)batch2 * HT;
      XattnPremulP pm{}; pm.kv = xl.kv; pm.ldkv = 2 * xl.C; pm.skv = (long long)tokens * 2 * xl.C; pm.wqT = xl.pm_wqT; pm.wo = wo2->w; pm.gamma = g2; pm.wqb = xl.pm_wqb;
      pm.B = batch2; pm.T = tokens; pm.C = xl.C; pm.H = xl.heads; pm.scale = 1.0f / sqrtf((float)(xl.C / xl.heads));
      pm.kpp = xl.pm_kpp; pm.kcs = xl.pm_kcs; pm.kbs = xl.pm_kbs; pm.vpp = xl.pm_vpp;
      { ProfScope ps(c, st, PC_ATTN_CROSS, 8.0 * batch2 * (double)HT * xl.C * (xl.C / xl.heads) / 2.0, 4.0 * batch2 * (double)HT * xl.C);
        API_CK(c, launch_xattn_premul(pm, st)); }
      xl.pm_ready = true;
    }
  }
  c->ctx_stale = false;
  return 0;
}

static int ensure_lat(agd_ctx* c, int B2, int Lh, int Lw) {
  const size_t need = (size_t)B2 * Lh * Lw * 64;
  const int oc = c->cfg.out_channels > 4 ? c->cfg.out_channels : 4;
  CK(c->latb.ensure(need * 2)); CK(c->epsb.ensure((size_t)B2 * Lh * Lw * oc * 4));
  c->lat_bf16 = c->latb.as<bf16_t>(); c->eps_nhwc = c->epsb.as<float>();
  return 0;
}

static int embed_all_timesteps(agd_ctx* c, hipStream_t st, const float* timesteps, int n, const float** out);
// ---- the conditioning of a call ------------------------------------------------------------------------------------------------------
// What a whole call runs beside the UNet, resolved ONCE by resolve_cond() before the call's first launch: the per-evaluation ControlNet
// scales, GLIGEN flags, T2I-Adapter scales and inpainting-blend (sa, sb) pairs -- each nullptr when none -- and the IP-Adapter's image branch.
struct CallCond {
  const float* cn = nullptr; const int* gl = nullptr; const float* ad = nullptr; const float* blend = nullptr; bool ipa = false;
  const float* pag = nullptr;                                      // the PAG scales: the loop runs a third walk where pag[i] > 0 (at(i) stays the main walk's)
  // DeepCache's flags (1 = full, 0 = shallow) of the call's dc_n evaluations at branch dc_b: a full evaluation captures iff the next one is shallow
  const int* dc = nullptr; int dc_n = 0, dc_b = 0;
  bool sega = false;                                               // a Semantic Guidance state: the loop runs the concept walk, the threshold and the fold
  EvalCond at(int i) const {
    EvalCond e; e.cn_scale = cn ? cn[i] : 0.f; e.grounded = gl && gl[i]; e.ad_scale = ad ? ad[i] : 0.f; e.ipa = ipa;
    if (dc) { e.dc = !dc[i] ? DC_SHALLOW : (i + 1 < dc_n && !dc[i + 1]) ? DC_CAPTURE : 0; e.dc_branch = dc_b; }
    return e;
  }
};
// who resolves: agd_unet_forward_hw, agd_unet_forward_ts_hw, run_eval_loop, run_ip2p_loop, agd_denoise_panorama, agd_deepcache_forward_hw,
// agd_denoise_regions
enum Caller { CALL_UNET_FORWARD, CALL_UNET_FORWARD_TS, CALL_EVAL_LOOP, CALL_IP2P_LOOP, CALL_PANORAMA, CALL_DC_FORWARD, CALL_REGIONS };
enum CondState { ST_CN, ST_GL, ST_INP, ST_I2P, ST_AD, ST_IPA, ST_PAG, ST_DC, ST_SEGA, N_COND_STATES };                       // the states a call can meet, in the order of a row's cells
// One row per refusing party: a state (self) that, when set, refuses to run beside others in the callers that consult it, or an entry point
// that runs the UNet alone (self < 0: it refuses whenever it is the caller).  with[s]: nullptr = allowed beside state s, else the refusal.
// Rows are looked at top to bottom, the first set cell wins.  Whatever is not here is allowed: ControlNet + GLIGEN, GLIGEN + either
// inpainting, agd_unet_forward_hw beside an inpainting / InstructPix2Pix state (it does not read them), an idle IP-Adapter beside anything.
struct ConflictRow { int self; unsigned callers; const char* with[N_COND_STATES]; };
static const ConflictRow kConflicts[] = {
  { ST_INP, 1u << CALL_EVAL_LOOP, {   // inpaint
    "inpaint: a ControlNet schedule is set; ControlNet inpainting is not implemented", nullptr, nullptr, nullptr, nullptr, nullptr } },
  { ST_I2P, 1u << CALL_IP2P_LOOP, {   // ip2p
    "ip2p: a ControlNet schedule is set; ControlNet with InstructPix2Pix is not implemented (clear it first)",
    "ip2p: a GLIGEN schedule is set; GLIGEN with InstructPix2Pix is not implemented (clear it first)",
    "ip2p: an inpainting state is set; inpainting with InstructPix2Pix is not implemented (agd_inpaint_clear first)",
    nullptr,
    "ip2p: a T2I-Adapter schedule is set; the T2I-Adapter with InstructPix2Pix is not implemented (clear it first)",
    "ip2p: an IP-Adapter image is set; ip2p runs without it (agd_ip_adapter_clear first)" } },
  { ST_AD, 1u << CALL_UNET_FORWARD | 1u << CALL_EVAL_LOOP, {   // adapter
    "adapter: a ControlNet schedule is set; the T2I-Adapter with a ControlNet is not implemented (clear one of them)",
    "adapter: a GLIGEN schedule is set; the T2I-Adapter with GLIGEN is not implemented (clear one of them)",
    "adapter: an inpainting state is set; the T2I-Adapter with inpainting is not implemented (agd_inpaint_clear first)",
    "adapter: an InstructPix2Pix state is set; the T2I-Adapter with InstructPix2Pix is not implemented (agd_ip2p_clear first)",
    nullptr, nullptr } },
  { ST_IPA, 1u << CALL_UNET_FORWARD | 1u << CALL_EVAL_LOOP, {   // ip_adapter
    "ip_adapter: a ControlNet schedule is set; the IP-Adapter with a ControlNet is not implemented (clear one of them)",
    "ip_adapter: a GLIGEN schedule is set; the IP-Adapter with GLIGEN is not implemented (clear one of them)",
    "ip_adapter: an inpainting state is set; the IP-Adapter with inpainting is not implemented (agd_inpaint_clear first)",
    "ip_adapter: an InstructPix2Pix state is set; the IP-Adapter with InstructPix2Pix is not implemented (agd_ip2p_clear first)",
    "ip_adapter: a T2I-Adapter schedule is set; the IP-Adapter with a T2I-Adapter is not implemented (clear one of them)",
    nullptr } },
  { -1, 1u << CALL_UNET_FORWARD_TS, {   // unet_forward_ts (it reads neither an inpainting nor an InstructPix2Pix state)
    "unet_forward_ts: a ControlNet schedule is set; per-image timesteps run the UNet alone (clear it first)",
    "unet_forward_ts: a GLIGEN schedule is set; per-image timesteps run the UNet alone (clear it first)",
    nullptr, nullptr,
    "unet_forward_ts: a T2I-Adapter schedule is set; per-image timesteps run the UNet alone (clear it first)",
    "unet_forward_ts: an IP-Adapter image is set; unet_forward_ts runs without it (agd_ip_adapter_clear first)" } },
  { -1, 1u << CALL_PANORAMA, {   // denoise_panorama
    "denoise_panorama: a ControlNet schedule is set; ControlNet on a panorama is not implemented (clear it first)",
    "denoise_panorama: a GLIGEN schedule is set; GLIGEN on a panorama is not implemented (clear it first)",
    "denoise_panorama: an inpainting state is set; inpainting on a panorama is not implemented (agd_inpaint_clear first)",
    "denoise_panorama: an InstructPix2Pix state is set; InstructPix2Pix on a panorama is not implemented (agd_ip2p_clear first)",
    "denoise_panorama: a T2I-Adapter schedule is set; the T2I-Adapter on a panorama is not implemented (clear it first)",
    "denoise_panorama: an IP-Adapter image is set; denoise_panorama runs without it (agd_ip_adapter_clear first)" } },
};
// Perturbed-Attention Guidance's row and column of the table, consulted after it (so whatever kConflicts refuses keeps its message).  They
// stand apart because tests/test_conditioning_gpu.py counts kConflicts' cells against a recording made before PAG existed, in which every
// cell above is refused somewhere; the rows above leave their ST_PAG cell empty (nullptr).
static const ConflictRow kPagConflicts[] = {
  { ST_PAG, 1u << CALL_UNET_FORWARD | 1u << CALL_EVAL_LOOP | 1u << CALL_IP2P_LOOP, {   // pag
    "pag: a ControlNet schedule is set; Perturbed-Attention Guidance with a ControlNet is not implemented (clear one of them)",
    "pag: a GLIGEN schedule is set; Perturbed-Attention Guidance with GLIGEN is not implemented (clear one of them)",
    "pag: an inpainting state is set; Perturbed-Attention Guidance with inpainting is not implemented (agd_inpaint_clear or agd_pag_clear first)",
    "pag: an InstructPix2Pix state is set; Perturbed-Attention Guidance with InstructPix2Pix is not implemented (agd_ip2p_clear or agd_pag_clear first)",
    "pag: a T2I-Adapter schedule is set; Perturbed-Attention Guidance with a T2I-Adapter is not implemented (clear one of them)",
    "pag: an IP-Adapter image is set; Perturbed-Attention Guidance with an IP-Adapter is not implemented (agd_ip_adapter_clear or agd_pag_clear first)",
    nullptr } },
  { -1, 1u << CALL_UNET_FORWARD_TS, { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
    "unet_forward_ts: a Perturbed-Attention Guidance schedule is set; per-image timesteps run the UNet alone (agd_pag_clear first)" } },
  { -1, 1u << CALL_PANORAMA, { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
    "denoise_panorama: a Perturbed-Attention Guidance schedule is set; Perturbed-Attention Guidance on a panorama is not implemented (agd_pag_clear first)" } },
};
// DeepCache's rows, consulted last, in a table of their own for the same reason (the tables above leave their ST_DC cell empty).  The shallow
// walk runs the plain UNet alone: nothing that injects into, or runs beside, the layers it skips.  agd_unet_forward_hw does not read the state.
static const ConflictRow kDcConflicts[] = {
  { ST_DC, 1u << CALL_EVAL_LOOP | 1u << CALL_IP2P_LOOP, {   // deepcache
    "deepcache: a ControlNet schedule is set; DeepCache with a ControlNet is not implemented (clear one of them)",
    "deepcache: a GLIGEN schedule is set; DeepCache with GLIGEN is not implemented (clear one of them)",
    "deepcache: an inpainting state is set; DeepCache with inpainting is not implemented (agd_inpaint_clear or agd_deepcache_clear first)",
    "deepcache: an InstructPix2Pix state is set; DeepCache with InstructPix2Pix is not implemented (agd_ip2p_clear or agd_deepcache_clear first)",
    "deepcache: a T2I-Adapter schedule is set; DeepCache with a T2I-Adapter is not implemented (clear one of them)",
    "deepcache: an IP-Adapter image is set; DeepCache with an IP-Adapter is not implemented (agd_ip_adapter_clear or agd_deepcache_clear first)",
    "deepcache: a Perturbed-Attention Guidance schedule is set; DeepCache with Perturbed-Attention Guidance is not implemented (agd_pag_clear or agd_deepcache_clear first)",
    nullptr } },
  { -1, 1u << CALL_DC_FORWARD, {   // deepcache_forward (it reads neither an inpainting nor an InstructPix2Pix state, nor a DeepCache schedule)
    "deepcache_forward: a ControlNet schedule is set; DeepCache with a ControlNet is not implemented (clear it first)",
    "deepcache_forward: a GLIGEN schedule is set; DeepCache with GLIGEN is not implemented (clear it first)",
    nullptr, nullptr,
    "deepcache_forward: a T2I-Adapter schedule is set; DeepCache with a T2I-Adapter is not implemented (clear it first)",
    "deepcache_forward: an IP-Adapter image is set; DeepCache with an IP-Adapter is not implemented (agd_ip_adapter_clear first)",
    "deepcache_forward: a Perturbed-Attention Guidance schedule is set; DeepCache with Perturbed-Attention Guidance is not implemented (agd_pag_clear first)",
    nullptr } },
  { -1, 1u << CALL_UNET_FORWARD_TS, { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
    "unet_forward_ts: a DeepCache schedule is set; per-image timesteps run the UNet alone (agd_deepcache_clear first)" } },
  { -1, 1u << CALL_PANORAMA, { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
    "denoise_panorama: a DeepCache schedule is set; DeepCache on a panorama is not implemented (agd_deepcache_clear first)" } },
};
// agd_denoise_regions' row, consulted after the three tables above, in a table of its own for the same reason: it runs the UNet alone on its
// R x batch rows and reads none of these states.
static const ConflictRow kRegionConflicts[] = {
  { -1, 1u << CALL_REGIONS, {   // denoise_regions
    "denoise_regions: a ControlNet schedule is set; ControlNet with region prompts is not implemented (clear it first)",
    "denoise_regions: a GLIGEN schedule is set; GLIGEN with region prompts is not implemented (clear it first)",
    "denoise_regions: an inpainting state is set; inpainting with region prompts is not implemented (agd_inpaint_clear first)",
    "denoise_regions: an InstructPix2Pix state is set; InstructPix2Pix with region prompts is not implemented (agd_ip2p_clear first)",
    "denoise_regions: a T2I-Adapter schedule is set; the T2I-Adapter with region prompts is not implemented (clear it first)",
    "denoise_regions: an IP-Adapter image is set; denoise_regions runs without it (agd_ip_adapter_clear first)",
    "denoise_regions: a Perturbed-Attention Guidance schedule is set; Perturbed-Attention Guidance with region prompts is not implemented (agd_pag_clear first)",
    "denoise_regions: a DeepCache schedule is set; DeepCache with region prompts is not implemented (agd_deepcache_clear first)" } },
};
// Semantic Guidance's rows, consulted last, in a table of their own for the same reason (the tables above leave their ST_SEGA cell empty).  The
// concept walk runs the plain UNet on K B rows of its own context: nothing that is set for 2 B rows, or that runs a walk of its own, beside it.
#define SEGA_NULL8 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr
static const ConflictRow kSegaConflicts[] = {
  { ST_SEGA, 1u << CALL_UNET_FORWARD | 1u << CALL_EVAL_LOOP | 1u << CALL_IP2P_LOOP, {   // sega
    "sega: a ControlNet schedule is set; Semantic Guidance with a ControlNet is not implemented (clear one of them)",
    "sega: a GLIGEN schedule is set; Semantic Guidance with GLIGEN is not implemented (clear one of them)",
    "sega: an inpainting state is set; Semantic Guidance with inpainting is not implemented (agd_inpaint_clear or agd_sega_clear first)",
    "sega: an InstructPix2Pix state is set; Semantic Guidance with InstructPix2Pix is not implemented (agd_ip2p_clear or agd_sega_clear first)",
    "sega: a T2I-Adapter schedule is set; Semantic Guidance with a T2I-Adapter is not implemented (clear one of them)",
    "sega: an IP-Adapter image is set; Semantic Guidance with an IP-Adapter is not implemented (agd_ip_adapter_clear or agd_sega_clear first)",
    "sega: a Perturbed-Attention Guidance schedule is set; Semantic Guidance with Perturbed-Attention Guidance is not implemented (agd_pag_clear or agd_sega_clear first)",
    "sega: a DeepCache schedule is set; Semantic Guidance with DeepCache is not implemented (agd_deepcache_clear or agd_sega_clear first)",
    nullptr } },
  { -1, 1u << CALL_UNET_FORWARD_TS, { SEGA_NULL8,
    "unet_forward_ts: a Semantic Guidance state is set; per-image timesteps run the UNet alone (agd_sega_clear first)" } },
  { -1, 1u << CALL_PANORAMA, { SEGA_NULL8,
    "denoise_panorama: a Semantic Guidance state is set; Semantic Guidance on a panorama is not implemented (agd_sega_clear first)" } },
  { -1, 1u << CALL_DC_FORWARD, { SEGA_NULL8,
    "deepcache_forward: a Semantic Guidance state is set; DeepCache with Semantic Guidance is not implemented (agd_sega_clear first)" } },
  { -1, 1u << CALL_REGIONS, { SEGA_NULL8,
    "denoise_regions: a Semantic Guidance state is set; Semantic Guidance with region prompts is not implemented (agd_sega_clear first)" } },
};
// an InstructPix2Pix UNet reads the latent channels and the VAE's latent channels
static int ip2p_check_unet(agd_ctx* c, const char* what) {
  const agd_config& g = c->cfg;
  if (g.in_channels != g.out_channels + g.vae_latent_channels || g.in_channels > 64)
    FAIL("%s: the UNet takes %d input channels, InstructPix2Pix needs %d latent + %d image-latent channels", what, g.in_channels, g.out_channels, g.vae_latent_channels);
  return 0;
}
// The conditioning of the call `who` makes: n model evaluations on `rows` images at latent size Lh x Lw (agd_unet_forward_hw: its UNet rows;
// a loop: its batch, the UNet then runs 2 rows of them under CFG).  Everything that can refuse does so here, before the first launch, in this
// order: (a) which states are set, (b) the conflict table, (c) whether each state that runs fits this call.  *out: what the call then runs.
static int resolve_cond(agd_ctx* c, Caller who, int n, int rows, int Lh, int Lw, CallCond* out) {
  *out = CallCond();
  const int B2 = who == CALL_UNET_FORWARD || who == CALL_DC_FORWARD ? rows : 2 * rows;
  // (a) a schedule counts once it is non-empty, all zeros too; the IP-Adapter only with rows and a non-zero scale (idle otherwise)
  bool set[N_COND_STATES];
  set[ST_CN] = !c->cn_sched.empty(); set[ST_GL] = !c->gl_sched.empty(); set[ST_INP] = c->ip_mode != 0; set[ST_I2P] = c->i2_on;
  set[ST_AD] = !c->ad_sched.empty(); set[ST_IPA] = c->ipa_B2 > 0 && c->ipa_scale != 0.f; set[ST_PAG] = !c->pag_sched.empty();
  set[ST_DC] = !c->dc_sched.empty(); set[ST_SEGA] = c->sega_K > 0;
  for (const ConflictRow* t : {kConflicts, kPagConflicts, kDcConflicts, kRegionConflicts, kSegaConflicts}) {   // (b) rows top to bottom, the first set cell wins
    const size_t rows = t == kConflicts ? sizeof(kConflicts) / sizeof(kConflicts[0]) : t == kPagConflicts ? sizeof(kPagConflicts) / sizeof(kPagConflicts[0])
                                        : t == kDcConflicts ? sizeof(kDcConflicts) / sizeof(kDcConflicts[0])
                                        : t == kRegionConflicts ? sizeof(kRegionConflicts) / sizeof(kRegionConflicts[0]) : sizeof(kSegaConflicts) / sizeof(kSegaConflicts[0]);
    for (size_t k = 0; k < rows; ++k) {
      const ConflictRow& r = t[k];
      if (!((r.callers >> who) & 1) || (r.self >= 0 && !set[r.self])) continue;
      for (int s = 0; s < N_COND_STATES; ++s) if (set[s] && r.with[s]) FAIL("%s", r.with[s]);
    }
  }
  // (c) a context beyond 96 tokens runs the plain UNet in the fused loops, agd_unet_forward_hw and agd_deepcache_forward_hw, recorded by DAAM alone
  if (c->ctx_T > 96) {
    const int T = c->ctx_T;
    if (c->rec_mode == 2) FAIL("long context: the hook.py recorder takes contexts of at most 96 tokens (this one has %d)", T);
    if (who == CALL_UNET_FORWARD_TS) FAIL("unet_forward_ts: a context of %d tokens is not supported (at most 96)", T);
    if (who == CALL_PANORAMA) FAIL("denoise_panorama: a context of %d tokens is not supported (at most 96)", T);
    if (who == CALL_REGIONS) FAIL("denoise_regions: a context of %d tokens is not supported (at most 96)", T);
    static const struct { int st; const char* what; } kLong[] = {
      {ST_CN, "a ControlNet schedule"}, {ST_GL, "a GLIGEN schedule"}, {ST_INP, "an inpainting state"}, {ST_I2P, "an InstructPix2Pix state"},
      {ST_AD, "a T2I-Adapter schedule"}, {ST_IPA, "an IP-Adapter image"}, {ST_SEGA, "a Semantic Guidance state"} };
    for (const auto& k : kLong) {
      if (!set[k.st] || (k.st == ST_INP && who != CALL_EVAL_LOOP) || (k.st == ST_I2P && who != CALL_IP2P_LOOP)) continue;   // (only where the caller reads the state)
      FAIL("long context: %s is set; a context of %d tokens (over 96) runs the plain UNet only (clear it first)", k.what, T);
    }
  }
  // the entry points that run the UNet alone have refused every state they read; the latents must be all the UNet takes
  if (who == CALL_PANORAMA && c->cfg.in_channels != c->cfg.out_channels)
    FAIL("denoise_panorama: the UNet takes %d input channels (an inpainting UNet), the latents have %d", c->cfg.in_channels, c->cfg.out_channels);
  if (who == CALL_REGIONS && c->cfg.in_channels != c->cfg.out_channels)
    FAIL("denoise_regions: the UNet takes %d input channels (an inpainting UNet), the latents have %d", c->cfg.in_channels, c->cfg.out_channels);
  if (who == CALL_UNET_FORWARD_TS || who == CALL_PANORAMA || who == CALL_REGIONS) return 0;
  if (who == CALL_IP2P_LOOP) {
    CK(ip2p_check_unet(c, "ip2p"));
    if (c->i2_B != rows || c->i2_Lh != Lh || c->i2_Lw != Lw)
      FAIL("ip2p: the state holds %d images at latent sides %d x %d, this call runs %d at %d x %d", c->i2_B, c->i2_Lh, c->i2_Lw, rows, Lh, Lw);
    return 0;
  }
  // a schedule's length is the call's evaluations; what it reads must exist for exactly these rows and sizes once any entry is non-zero
  auto any = [](const auto& v) { for (auto x : v) if (x != 0) return true; return false; };
  if (set[ST_CN]) {
    if ((int)c->cn_sched.size() != n) FAIL("controlnet: the schedule has %zu scales, this call runs %d model evaluations (agd_controlnet_set_schedule)", c->cn_sched.size(), n);
    if (any(c->cn_sched) && (c->cn_emb_B2 != B2 || c->cn_emb_Lh != Lh || c->cn_emb_Lw != Lw))
      FAIL("controlnet: no conditioning image set for %d rows at latent sides %d x %d (agd_controlnet_set_cond has %d rows at %d x %d)", B2, Lh, Lw, c->cn_emb_B2, c->cn_emb_Lh, c->cn_emb_Lw);
    out->cn = c->cn_sched.data();
  }
  if (set[ST_GL]) {
    if ((int)c->gl_sched.size() != n) FAIL("gligen: the schedule has %zu flags, this call runs %d model evaluations (agd_gligen_set_schedule)", c->gl_sched.size(), n);
    if (any(c->gl_sched) && c->gl_B2 != B2) FAIL("gligen: the grounding objects are set for %d rows, this call runs %d (agd_gligen_set)", c->gl_B2, B2);
    out->gl = c->gl_sched.data();
  }
  if (who == CALL_EVAL_LOOP && !set[ST_INP] && c->cfg.in_channels != c->cfg.out_channels)
    FAIL("denoise: the UNet takes %d input channels, the latents have %d: an inpainting UNet needs agd_inpaint_set first, an InstructPix2Pix UNet agd_ip2p_set_hw",
         c->cfg.in_channels, c->cfg.out_channels);
  if (who == CALL_EVAL_LOOP && set[ST_INP]) {
    if (c->ip_B != rows || c->ip_Lh != Lh || c->ip_Lw != Lw)
      FAIL("inpaint: the state holds %d images at latent sides %d x %d, this call runs %d at %d x %d", c->ip_B, c->ip_Lh, c->ip_Lw, rows, Lh, Lw);
    if (c->ip_mode == 2) {
      if ((int)c->ip_sched.size() != 2 * n) FAIL("inpaint: the blend schedule has %zu entries, this call runs %d model evaluations (agd_inpaint_set_schedule)", c->ip_sched.size() / 2, n);
      out->blend = c->ip_sched.data();
    }
  }
  if (set[ST_AD]) {                                                // features for ad_B images serve rows a multiple of it (row image b reads feature image b % ad_B)
    if ((int)c->ad_sched.size() != n) FAIL("adapter: the schedule has %zu scales, this call runs %d model evaluations (agd_adapter_set_schedule)", c->ad_sched.size(), n);
    if (any(c->ad_sched) && (c->ad_B < 1 || rows % c->ad_B || c->ad_Lh != Lh || c->ad_Lw != Lw))
      FAIL("adapter: the features are set for %d images at latent sides %d x %d, this call runs %d rows at %d x %d (agd_adapter_set_cond_hw)", c->ad_B, c->ad_Lh, c->ad_Lw, rows, Lh, Lw);
    out->ad = c->ad_sched.data();
  }
  if (set[ST_IPA]) {
    if (c->ipa_stale) FAIL("ip_adapter: a LoRA scale change rewrote to_q / to_out after the image products were built (call agd_ip_adapter_set again)");
    if (c->ipa_B2 != B2) FAIL("ip_adapter: the image tokens are set for %d rows, this call runs %d (agd_ip_adapter_set)", c->ipa_B2, B2);
    out->ipa = true;
  }
  if (set[ST_PAG]) {
    if ((int)c->pag_sched.size() != n) FAIL("pag: the schedule has %zu scales, this call runs %d model evaluations (agd_pag_set)", c->pag_sched.size(), n);
    out->pag = c->pag_sched.data();
  }
  if (set[ST_SEGA]) {
    if (c->sega_n != n) FAIL("sega: the schedule covers %d model evaluations, this call runs %d (agd_sega_set)", c->sega_n, n);
    if (c->cfg.out_channels != 4) FAIL("sega: the UNet has %d output channels; the Semantic Guidance kernels read rows of 4 (out_channels = 4)", c->cfg.out_channels);
    if (who == CALL_UNET_FORWARD && (rows % (2 + c->sega_K) || rows < 2 + c->sega_K))
      FAIL("sega: unet_forward on %d rows; %d concepts take (2 + K) B = a multiple of %d rows", rows, c->sega_K, 2 + c->sega_K);
    out->sega = true;
  }
  if (set[ST_DC] && who == CALL_EVAL_LOOP) {
    if ((int)c->dc_sched.size() != n) FAIL("deepcache: the schedule has %zu flags, this call runs %d model evaluations (agd_deepcache_set)", c->dc_sched.size(), n);
    if (c->dc_branch > c->cfg.layers_per_block - 1) FAIL("deepcache: branch %d (this UNet has branches 0 .. %d)", c->dc_branch, c->cfg.layers_per_block - 1);
    if (!std::all_of(c->dc_sched.begin(), c->dc_sched.end(), [](int f) { return f != 0; })) {   // (all full: the plain call, nothing reserved)
      CK(deepcache_reserve(c, B2, Lh, Lw));
      out->dc = c->dc_sched.data(); out->dc_n = n; out->dc_b = c->dc_branch;
    }
  }
  return 0;
}
// A non-recording side walk of `rows` images against context rows [row0, row0 + rows) of what agd_set_context projected (PanoCtx::point's
// arithmetic).  Perturbed-Attention Guidance's perturbed walk: in a loop the [cond x B] half of [uncond x B | cond x B], in
// agd_unet_forward_hw all of it.  Semantic Guidance's concept walk: the K B rows from row 2 B on.  Nothing is recorded, and the engine is put
// back as it was when the walk ends, on an error too.  count: the feature's walk counter, advanced once.
struct SideWalk {
  struct Saved { bf16_t* kv; bf16_t* kpp; bf16_t* vpp; float* kcs; float* kbs; };
  agd_ctx* c; int B2, mode; std::vector<Saved> saved;
  SideWalk(agd_ctx* c_, int row0, int rows, long long* count) : c(c_), B2(c_->ctx_B2), mode(c_->rec_mode) {
    const size_t off = (size_t)row0;
    if (off) {
      saved.reserve(c->xl.size());
      for (auto& xl : c->xl) {
        saved.push_back({xl.kv, xl.pm_kpp, xl.pm_vpp, xl.pm_kcs, xl.pm_kbs});
        xl.kv += off * c->ctx_T * 2 * xl.C;
        if (!xl.pm_ready) continue;
        const size_t HT = (size_t)xl.heads * XATTN_TP;
        xl.pm_kpp += off * HT * xl.C; xl.pm_vpp += off * HT * xl.C; xl.pm_kcs += off * HT; xl.pm_kbs += off * HT;
      }
    }
    c->ctx_B2 = rows; c->rec_mode = 0; ++*count;
  }
  ~SideWalk() {
    for (size_t k = 0; k < saved.size(); ++k) {
      XLayer& xl = c->xl[k]; const Saved& v = saved[k];
      xl.kv = v.kv; xl.pm_kpp = v.kpp; xl.pm_vpp = v.vpp; xl.pm_kcs = v.kcs; xl.pm_kbs = v.kbs;
    }
    c->ctx_B2 = B2; c->rec_mode = mode; c->cur.pag = false;
  }
};
// Semantic Guidance (sega.hip).  SegaMain: the main walk of an evaluation sees the first `rows` = 2 B rows of the (2 + K) B-row context (they
// are its head: no pointer moves), so the shared prefix and the recorders' conditional half are what they are without the state; rows == 0:
// nothing changes.  The engine is put back when the walk ends, on an error too.
struct SegaMain {
  agd_ctx* c; int B2;
  SegaMain(agd_ctx* c_, int rows) : c(c_), B2(c_->ctx_B2) { if (rows) c->ctx_B2 = rows; }
  ~SegaMain() { c->ctx_B2 = B2; }
};
// evaluation i's scalars for the kernels
static SegaEvalP sega_eval(const agd_ctx* c, int i, int HW) {
  SegaEvalP p{};
  for (int k = 0; k < c->sega_K; ++k) {
    p.coef[k] = c->sega_coef[(size_t)i * c->sega_K + k]; p.w_mom[k] = c->sega_wmom[(size_t)i * c->sega_K + k]; p.w_add[k] = c->sega_wadd[(size_t)i * c->sega_K + k];
    sega_rank(c->sega_q[k], HW, &p.lo[k], &p.f[k]);
  }
  return p;
}
// What follows the main walk of evaluation i of a Semantic Guidance call on `batch` images: lat_bf16 rows [0, 2 B) hold the main walk's input,
// eps rows [0, 2 B) its output.  walk_always: agd_unet_forward_hw returns the concept rows, so it walks them whatever the coefficients.
static int sega_after_main(agd_ctx* c, hipStream_t st, int i, int batch, int Lh, int Lw, float t, const float* tproj_row, const EvalCond& ec, bool walk_always) {
  const int K = c->sega_K, HW = Lh * Lw, B2 = 2 * batch;
  const long long ne = (long long)batch * HW * 4;
  const SegaEvalP p = sega_eval(c, i, HW);
  bool any = false;
  for (int k = 0; k < K; ++k) any = any || p.coef[k] != 0.f;
  float* thr = c->sega_thrb.as<float>();
  if (any || walk_always) {
    // e_k: the conditional rows again (K copies of their input), concept k's B rows against context rows [(2 + k) B, (3 + k) B), into eps
    // rows [2 B, (2 + K) B); nothing is recorded
    bf16_t* xin_k = c->lat_bf16 + (size_t)B2 * HW * 64;
    { ProfScope ps(c, st, PC_ELEM, 0); CK(launch_tile_rows(c->lat_bf16 + (size_t)batch * HW * 64, xin_k, 1, batch, K, (size_t)HW * 64 * 2, st)); }
    { SideWalk sw(c, B2, K * batch, &c->sega_counts[0]);
      CK(unet_walk(c, st, xin_k, K * batch, Lh, Lw, t, c->eps_nhwc + 2 * ne, tproj_row, false, 0, ec)); }
  }
  ProfScope ps(c, st, PC_ELEM, 0);
  if (any) CK(launch_sega_threshold(c->eps_nhwc, batch, K, c->cfg.out_channels, HW, p, thr, st));
  CK(launch_sega_fold(c->eps_nhwc, c->sega_momb.as<float>(), thr, batch, K, c->cfg.out_channels, HW, p, c->sega_mu, c->sega_beta, c->sega_addmom[i], st));
  c->sega_counts[1]++;
  return 0;
}
// a Semantic Guidance call's buffers for `batch` images, the momentum zeroed
static int sega_begin(agd_ctx* c, hipStream_t st, int batch, int Lh, int Lw) {
  const size_t ne = (size_t)batch * Lh * Lw * 4;
  if (c->ctx_B2 != (2 + c->sega_K) * batch)
    FAIL("sega: the context holds %d rows; %d concepts on %d images take (2 + K) B = %d: [uncond x B | cond x B | concept_0 x B | ...] (agd_set_context)",
         c->ctx_B2, c->sega_K, batch, (2 + c->sega_K) * batch);
  CK(ensure_lat(c, (2 + c->sega_K) * batch, Lh, Lw));
  CK(c->sega_momb.ensure(ne * sizeof(float))); CK(c->sega_thrb.ensure((size_t)batch * c->sega_K * 4 * sizeof(float)));
  if (hipMemsetAsync(c->sega_momb.p, 0, ne * sizeof(float), st) != hipSuccess) FAIL("sega: momentum clear failed");
  return 0;
}
// the UNet input of one CFG evaluation: the latents (txt2img) or latents | mask | masked-image latents (9-channel inpainting), both CFG halves
static int prep_unet_input(agd_ctx* c, hipStream_t st, const float* latents, int batch, int HW) {
  ProfScope ps(c, st, PC_ELEM, 0);
  if (c->ip_mode == 1)
    return launch_prep_inpaint(latents, c->ip_maskb.as<float>(), c->ip_condb.as<float>(), c->lat_bf16, batch, c->cfg.out_channels, c->ip_Cm, c->ip_Cc, HW, 64, 2, st);
  return launch_prep_latents(latents, c->lat_bf16, batch, c->cfg.out_channels, HW, 64, 2, 1.0f, st);
}
// the 4-channel blend after the step of evaluation i (sab = (sa, sb) of that evaluation)
static int inpaint_blend(agd_ctx* c, hipStream_t st, float* latents, int batch, int HW, const float* sab) {
  ProfScope ps(c, st, PC_ELEM, 0);
  return launch_inpaint_blend(latents, c->ip_condb.as<float>(), c->ip_noiseb.as<float>(), c->ip_maskb.as<float>(), batch, c->cfg.out_channels, HW,
                              sab[0], sab[1], st);
}
// a latent size of a _hw entry point: both sides positive; a rectangular one must halve exactly at every UNet level (the 64-pixel rule
// per axis).  Square sizes keep the acceptance the one-side entry points always had.
static int check_latent_hw(agd_ctx* c, const char* what, int Lh, int Lw) {
  const int f = 1 << (c->cfg.n_levels - 1);
  if (Lh < 1 || Lw < 1 || (Lh != Lw && (Lh % f || Lw % f))) FAIL("%s: latent size %d x %d (each side a positive multiple of %d)", what, Lh, Lw, f);
  return 0;
}

AGD_API int agd_unet_forward_hw(agd_ctx* c, const float* sample, int batch2, int Lh, int Lw, float timestep, float* out, void* stream) {
  API_CK(c, need_final(c));
  API_CK(c, check_latent_hw(c, "unet_forward", Lh, Lw));
  hipStream_t st = S(stream);
  API_CK(c, ensure_lat(c, batch2, Lh, Lw));
  const int Cl = c->cfg.in_channels;
  CallCond cc; API_CK(c, resolve_cond(c, CALL_UNET_FORWARD, 1, batch2, Lh, Lw, &cc));
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_prep_latents(sample, c->lat_bf16, batch2, Cl, Lh * Lw, 64, 1, 1.0f, st)); }
  EvalCond ec = cc.at(0);
  if (cc.sega) {                                                   // one Semantic Guidance evaluation on (2 + K) B rows: the folded pair, then the concept rows
    const int batch = batch2 / (2 + c->sega_K);
    API_CK(c, sega_begin(c, st, batch, Lh, Lw));
    { SegaMain sm(c, 2 * batch);
      API_CK(c, unet_walk(c, st, c->lat_bf16, 2 * batch, Lh, Lw, timestep, c->eps_nhwc, nullptr, false, 0, ec)); }
    API_CK(c, sega_after_main(c, st, 0, batch, Lh, Lw, timestep, nullptr, ec, true));
  } else if (cc.pag && cc.pag[0] > 0.f) {                                  // every row is the perturbed branch, against the caller's context as it is; nothing is recorded
    ec.pag = true;
    SideWalk pw(c, 0, c->ctx_B2, &c->pag_counts[0]);
    API_CK(c, unet_walk(c, st, c->lat_bf16, batch2, Lh, Lw, timestep, c->eps_nhwc, nullptr, false, 0, ec));
  } else {
    API_CK(c, unet_walk(c, st, c->lat_bf16, batch2, Lh, Lw, timestep, c->eps_nhwc, nullptr, false, 0, ec));
  }
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_nchw_from_nhwc_f32(c->eps_nhwc, c->cfg.out_channels, out, batch2, c->cfg.out_channels, Lh * Lw, st)); }
  return 0;
}
AGD_API int agd_unet_forward(agd_ctx* c, const float* sample, int batch2, int L, float timestep, float* out, void* stream) {
  return agd_unet_forward_hw(c, sample, batch2, L, L, timestep, out, stream);
}

// the training call `unet(noisy, timesteps[bsz], encoder_hidden_states)` (finetune_sd_token.py:1027): one timestep PER IMAGE
// (host array of batch2 floats): every image gets its own time-embedding row in the resnets' row add
AGD_API int agd_unet_forward_ts_hw(agd_ctx* c, const float* sample, int batch2, int Lh, int Lw, const float* timesteps, float* out, void* stream) {
  API_CK(c, need_final(c));
  API_CK(c, check_latent_hw(c, "unet_forward_ts", Lh, Lw));
  if (!timesteps || batch2 < 1) { agd_set_error("unet_forward_ts: bad arguments"); return fail_ctx(c); }
  CallCond cc; API_CK(c, resolve_cond(c, CALL_UNET_FORWARD_TS, 1, batch2, Lh, Lw, &cc));
  hipStream_t st = S(stream);
  API_CK(c, ensure_lat(c, batch2, Lh, Lw));
  const int Cl = c->cfg.in_channels;
  const float* tp_all = nullptr;
  API_CK(c, embed_all_timesteps(c, st, timesteps, batch2, &tp_all));
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_prep_latents(sample, c->lat_bf16, batch2, Cl, Lh * Lw, 64, 1, 1.0f, st)); }
  API_CK(c, unet_walk(c, st, c->lat_bf16, batch2, Lh, Lw, timesteps[0], c->eps_nhwc, tp_all, false, c->tproj_total));
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_nchw_from_nhwc_f32(c->eps_nhwc, c->cfg.out_channels, out, batch2, c->cfg.out_channels, Lh * Lw, st)); }
  return 0;
}
AGD_API int agd_unet_forward_ts(agd_ctx* c, const float* sample, int batch2, int L, const float* timesteps, float* out, void* stream) {
  return agd_unet_forward_ts_hw(c, sample, batch2, L, L, timesteps, out, stream);
}

// eps strides for cfg_ddim: NCHW eps handled by transposing through the NHWC kernel's stride form
AGD_API int agd_cfg_ddim_step_hw(agd_ctx* c, const float* eps, float* latents, int batch, int Lh, int Lw, float guidance, float alpha_t,
                                 float alpha_prev, void* stream) {
  API_CK(c, need_final(c));
  API_CK(c, check_latent_hw(c, "cfg_ddim_step", Lh, Lw));
  hipStream_t st = S(stream);
  API_CK(c, ensure_lat(c, 2 * batch, Lh, Lw));
  // NCHW eps -> NHWC scratch (tiny), then the fused kernel
  const int C = c->cfg.out_channels, HW = Lh * Lw;
  // reuse nchw_from_nhwc in the reverse direction: treat eps as "NHWC with ldc=HW" is not valid; do an explicit pass
  float* tmp = c->eps_nhwc;
  // out[b][p][c] = eps[b][c][p]  == nchw_from_nhwc with (C,HW) swapped
  API_CK(c, launch_nchw_from_nhwc_f32(eps, HW, tmp, 2 * batch, HW, C, st));
  ProfScope ps(c, st, PC_ELEM, 0);
  API_CK(c, launch_cfg_ddim(tmp, C, latents, batch, C, HW, guidance, alpha_t, alpha_prev, c->cfg.prediction_type, nullptr, st));
  return 0;
}
AGD_API int agd_cfg_ddim_step(agd_ctx* c, const float* eps, float* latents, int batch, int L, float guidance, float alpha_t,
                                 float alpha_prev, void* stream) {
  return agd_cfg_ddim_step_hw(c, eps, latents, batch, L, L, guidance, alpha_t, alpha_prev, stream);
}

// time embeddings of every model evaluation of a denoise loop, 8 timesteps per launch (the stacked time_emb_proj matrix is
// ~50 MB of weights: streamed ceil(n/8) times instead of once per step); returns [n][tproj_total] in *out
static int embed_all_timesteps(agd_ctx* c, hipStream_t st, const float* timesteps, int n, const float** out) {
  const int dim0 = c->cfg.block_out_channels[0];
  const size_t per_step = (size_t)c->tproj_total + (size_t)9 * dim0;         // (scratch: 9 dim floats per row of a chunk; chunk <= n rows at a time)
  if (c->tsteps_cap < n) {
    if (c->tsteps_buf) { hipDeviceSynchronize(); hipFree(c->tsteps_buf); }
    c->tsteps_buf = nullptr; c->tsteps_cap = 0;
    if (hipMalloc((void**)&c->tsteps_buf, per_step * n * sizeof(float)) != hipSuccess) FAIL("denoise: time-embedding buffer alloc failed");
    c->tsteps_cap = n;
  }
  float* tp_all = c->tsteps_buf;                                  // [n][tproj_total]
  float* tscratch = c->tsteps_buf + (size_t)c->tproj_total * n;
  const int chunk = (size_t)25 * 4 * dim0 * 4 <= 160 * 1024 ? 25 : 8;      // rows per launch: the 4 dim-wide fp32 rows of a chunk sit in LDS (misc.hip small_linear_kernel)
  for (int s0 = 0; s0 < n; s0 += chunk) {
    const int m = n - s0 < chunk ? n - s0 : chunk;
    CK(time_embed(c, st, timesteps + s0, m, tscratch, tp_all + (size_t)s0 * c->tproj_total));
  }
  *out = tp_all;
  return 0;
}

// guidance_rescale inside a step lambda (under the step's ProfScope): state clear -> *f = nullptr and no launch (the plain step, launch for
// launch); set -> one launch that reduces this evaluation's eps to a factor per image (guidance.hip), which the step kernel multiplies in.
static int guidance_factor(agd_ctx* c, hipStream_t st, const float* eps, int batch, int Cl, int HW, float guidance, const float** f) {
  *f = nullptr;
  if (!(c->gr_phi > 0.f)) return 0;
  CK(c->gr_factb.ensure((size_t)batch * sizeof(float)));
  CK(launch_guidance_factor(eps, c->cfg.out_channels, batch, Cl, HW, guidance, c->gr_phi, c->gr_factb.as<float>(), st));
  c->gr_count++;
  *f = c->gr_factb.as<float>();
  return 0;
}
// a loop that cannot rescale refuses a set state before its first launch
static int refuse_guidance_rescale(agd_ctx* c, const char* loop) {
  if (c->gr_phi > 0.f) FAIL("%s: guidance rescale (phi = %g) is set; this loop does not apply it (agd_guidance_rescale_clear)", loop, (double)c->gr_phi);
  return 0;
}
static int check_guidance_rescale(agd_ctx* c, const char* what, int Cl, int HW) {
  if (c->gr_phi > 0.f && (long long)Cl * HW < 2) FAIL("%s: guidance rescale needs at least 2 values per image (C * HW = %lld)", what, (long long)Cl * HW);
  return 0;
}

// The uncond walk of an InstructPix2Pix evaluation runs `rows` images against the first `rows` context rows -- the [uncond x B] half of the
// [uncond x B | cond x B] agd_set_context projected -- and records nothing.  The engine is put back as it was when the walk ends, on an error too.
struct Ip2pUncond {
  agd_ctx* c; int B2, mode;
  Ip2pUncond(agd_ctx* c_, int rows) : c(c_), B2(c_->ctx_B2), mode(c_->rec_mode) { c->ctx_B2 = rows; c->rec_mode = 0; }
  ~Ip2pUncond() { c->ctx_B2 = B2; c->rec_mode = mode; }
};
// The InstructPix2Pix evaluation loop (ip2p.hip): per evaluation the 8-channel input of the three branches, walk A on rows [0, B) (uncond:
// zero image latents, the negative prompt), walk B on rows [B, 3 B) (the usual [uncond | cond] pair, both with the image latents: the
// shared prefix and the recorders' conditional half apply unchanged), the fold of the three outputs into rows [B, 3 B), then step(i, eps)
// on those rows with the text scale.
template <class Step>
static int run_ip2p_loop(agd_ctx* c, hipStream_t st, float* latents, int batch, int Lh, int Lw, int n, const float* timesteps, Step&& step) {
  const int B2 = 2 * batch, HW = Lh * Lw, oc = c->cfg.out_channels;
  CK(refuse_guidance_rescale(c, "the InstructPix2Pix denoise loop"));
  CallCond cc; CK(resolve_cond(c, CALL_IP2P_LOOP, n, batch, Lh, Lw, &cc));
  if (c->ctx_B2 != B2) FAIL("denoise: context batch %d != 2*batch %d", c->ctx_B2, B2);
  CK(ensure_lat(c, 3 * batch, Lh, Lw));
  const float* tp_all = nullptr;
  CK(embed_all_timesteps(c, st, timesteps, n, &tp_all));
  const long long ne = (long long)batch * HW * oc;                 // one branch of eps
  bf16_t* xin_b = c->lat_bf16 + (size_t)batch * HW * 64;
  float* eps_b = c->eps_nhwc + ne;
  for (int i = 0; i < n; ++i) {
    const float* tp = tp_all + (size_t)i * c->tproj_total;
    { ProfScope ps(c, st, PC_ELEM, 0);
      CK(launch_prep_ip2p(latents, c->i2_latb.as<float>(), c->lat_bf16, batch, oc, c->cfg.vae_latent_channels, HW, 64, st)); }
    { Ip2pUncond un(c, batch);
      CK(unet_walk(c, st, c->lat_bf16, batch, Lh, Lw, timesteps[i], c->eps_nhwc, tp, false)); }
    CK(unet_walk(c, st, xin_b, B2, Lh, Lw, timesteps[i], eps_b, tp, true));
    { ProfScope ps(c, st, PC_ELEM, 0); CK(launch_ip2p_fold(c->eps_nhwc, ne, c->i2_scale, st)); }
    CK(step(i, eps_b));
  }
  return 0;
}

// The CFG evaluation loop of every fused denoise call: n model evaluations on `batch` images at Lh x Lw, `latents` updated in place.  Per
// evaluation i: the UNet input from the latents, the walk under that evaluation's time embedding and conditioning (cc.at(i)), then
// step(i, eps) -- the scheduler's kernel, eps [uncond | cond] -> latents -- then the inpainting blend when a blend schedule is set.  With an
// InstructPix2Pix state the three-branch loop above runs instead.  Every refusal comes before the first launch.
template <class Step>
static int run_eval_loop(agd_ctx* c, hipStream_t st, float* latents, int batch, int Lh, int Lw, int n, const float* timesteps, Step&& step) {
  if (c->i2_on) return run_ip2p_loop(c, st, latents, batch, Lh, Lw, n, timesteps, step);
  const int B2 = 2 * batch, HW = Lh * Lw;
  CK(ensure_lat(c, B2, Lh, Lw));
  if (c->sega_K == 0 && c->ctx_B2 != B2) FAIL("denoise: context batch %d != 2*batch %d", c->ctx_B2, B2);
  CallCond cc; CK(resolve_cond(c, CALL_EVAL_LOOP, n, batch, Lh, Lw, &cc));
  if (cc.sega) {                                                   // Semantic Guidance: a K B-row concept walk where a concept is active, the fold at every evaluation
    CK(refuse_guidance_rescale(c, "the Semantic Guidance denoise loop"));
    CK(sega_begin(c, st, batch, Lh, Lw));
  }
  struct DcLoop { agd_ctx* c; DcLoop(agd_ctx* c_) : c(c_) { deepcache_invalidate(c); } ~DcLoop() { deepcache_invalidate(c); } } dc_loop(c);   // a cache never outlives, or enters, a loop
  if (cc.pag) {                                                    // Perturbed-Attention Guidance: a third, B-row walk where its scale is > 0
    CK(refuse_guidance_rescale(c, "the Perturbed-Attention Guidance denoise loop"));
    CK(ensure_lat(c, 3 * batch, Lh, Lw));
  }
  const float* tp_all = nullptr;                                   // all timesteps are known up front: embed them now
  CK(embed_all_timesteps(c, st, timesteps, n, &tp_all));
  const long long ne = (long long)batch * HW * c->cfg.out_channels;   // one branch of eps
  for (int i = 0; i < n; ++i) {
    CK(prep_unet_input(c, st, latents, batch, HW));
    { SegaMain sm(c, cc.sega ? B2 : 0);
      CK(unet_walk(c, st, c->lat_bf16, B2, Lh, Lw, timesteps[i], c->eps_nhwc, tp_all + (size_t)i * c->tproj_total, true, 0, cc.at(i))); }
    if (cc.sega) CK(sega_after_main(c, st, i, batch, Lh, Lw, timesteps[i], tp_all + (size_t)i * c->tproj_total, cc.at(i), false));
    if (cc.pag && cc.pag[i] > 0.f) {
      // e_p: the conditional rows again (a copy of their input, the conditional half of the context) with the applied layers perturbed,
      // into eps rows [2 B, 3 B); then d = p (e_c - e_p) lands on both rows the step kernel reads
      bf16_t* xin_p = c->lat_bf16 + (size_t)B2 * HW * 64;
      { ProfScope ps(c, st, PC_ELEM, 0);
        if (hipMemcpyAsync(xin_p, c->lat_bf16 + (size_t)batch * HW * 64, (size_t)batch * HW * 64 * 2, hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("pag: input copy failed"); }
      { EvalCond ep = cc.at(i); ep.pag = true;
        SideWalk pw(c, batch, batch, &c->pag_counts[0]);
        CK(unet_walk(c, st, xin_p, batch, Lh, Lw, timesteps[i], c->eps_nhwc + 2 * ne, tp_all + (size_t)i * c->tproj_total, false, 0, ep)); }
      { ProfScope ps(c, st, PC_ELEM, 0); CK(launch_pag_fold(c->eps_nhwc, ne, cc.pag[i], st)); }
    }
    CK(step(i, c->eps_nhwc));
    if (cc.blend) CK(inpaint_blend(c, st, latents, batch, HW, cc.blend + 2 * i));
  }
  return 0;
}

AGD_API int agd_denoise_hw(agd_ctx* c, float* latents, int batch, int Lh, int Lw, int n_steps, const float* timesteps, const float* alpha_t,
                           const float* alpha_prev, float guidance, void* stream) {
  API_CK(c, need_final(c));
  API_CK(c, check_latent_hw(c, "denoise", Lh, Lw));
  hipStream_t st = S(stream);
  const int Cl = c->cfg.out_channels, HW = Lh * Lw;                          // Cl: the latent channels (a 9-channel UNet's input has more)
  API_CK(c, check_guidance_rescale(c, "denoise", Cl, HW));
  API_CK(c, run_eval_loop(c, st, latents, batch, Lh, Lw, n_steps, timesteps, [&](int s, const float* eps) {
    ProfScope ps(c, st, PC_ELEM, 0);
    const float* f; CK(guidance_factor(c, st, eps, batch, Cl, HW, guidance, &f));
    return launch_cfg_ddim(eps, c->cfg.out_channels, latents, batch, Cl, HW, guidance, alpha_t[s], alpha_prev[s], c->cfg.prediction_type, f, st);
  }));
  return 0;
}
AGD_API int agd_denoise(agd_ctx* c, float* latents, int batch, int L, int n_steps, const float* timesteps, const float* alpha_t,
                           const float* alpha_prev, float guidance, void* stream) {
  return agd_denoise_hw(c, latents, batch, L, L, n_steps, timesteps, alpha_t, alpha_prev, guidance, stream);
}

// ---- MultiDiffusion panorama (diffusers 0.21.2 StableDiffusionPanoramaPipeline [upstream-knowledge]; panorama.hip) ------------------
// While agd_denoise_panorama runs, the context is the prompts' [uncond x B | cond x B] tiled to [uncond x n B | cond x n B] (UNet batch order of a
// forward: view-major, panorama-minor) and projected ONCE per call -- exactly what agd_set_context on the tiled embeddings gives, so no step
// projects the text again.  When the loop ends (on an error too) the prompts' own context is put back and projected again: the engine is
// left as agd_set_context left it.
struct PanoCtx {
  agd_ctx* c; hipStream_t st; int B2, n = 0; bool tiled = false;
  PanoCtx(agd_ctx* c_, hipStream_t st_) : c(c_), st(st_), B2(c_->ctx_B2) {}
  int tile(int B, int n_) {
    const size_t row = (size_t)c->ctx_T * c->cfg.cross_attention_dim * 2;
    CK(c->pano_ctxb.ensure((size_t)B2 * row));
    if (hipMemcpyAsync(c->pano_ctxb.p, c->ctx_bf16, (size_t)B2 * row, hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("denoise_panorama: context copy failed");
    tiled = true; n = n_;
    CK(c->ctxb.ensure((size_t)2 * B * n * row)); c->ctx_bf16 = c->ctxb.as<bf16_t>();
    { ProfScope ps(c, st, PC_ELEM, 0); CK(launch_tile_rows(c->pano_ctxb.p, c->ctx_bf16, 2, B, n, row, st)); }
    return project_context(c, st, 2 * B * n, c->ctx_T);
  }
  // a forward of m <= n views per panorama: rows [(n - m) B, (n + m) B) of the tiled context are [uncond x m B | cond x m B] (the tiles of a half are equal)
  void point(int B, int m) {
    const size_t R = (size_t)2 * B * n, off = (size_t)(n - m) * B;
    for (auto& xl : c->xl) {
      xl.kv = xl.kvb.as<bf16_t>() + off * c->ctx_T * 2 * xl.C;
      if (!xl.pm_ready) continue;
      const size_t HT = (size_t)xl.heads * XATTN_TP;
      xl.pm_kpp = xl.pm_kppb.as<bf16_t>() + off * HT * xl.C; xl.pm_vpp = xl.pm_vppb.as<bf16_t>() + off * HT * xl.C;
      xl.pm_kcs = xl.pm_csb.as<float>() + off * HT; xl.pm_kbs = xl.pm_csb.as<float>() + R * HT + off * HT;
    }
    c->ctx_B2 = 2 * B * m;
  }
  ~PanoCtx() {
    c->rec_base = 0; c->rec_call = 0;
    if (!tiled) return;
    const size_t row = (size_t)c->ctx_T * c->cfg.cross_attention_dim * 2;
    (void)hipMemcpyAsync(c->ctx_bf16, c->pano_ctxb.p, (size_t)B2 * row, hipMemcpyDeviceToDevice, st);
    const std::string keep = g_err;                               // an error of the loop stays the one reported
    if (project_context(c, st, B2, c->ctx_T) != 0) c->ctx_stale = true;
    else agd_set_error("%s", keep.c_str());
  }
};
// accepted panorama sizes: each latent side a multiple of the stride and at least the window, the window itself on the stride grid (every
// canvas element is then covered: count > 0 everywhere) and a latent size the UNet takes
static int check_panorama(agd_ctx* c, const char* what, int Lh, int Lw, int window, int stride, int* nbh, int* nbw) {
  if (window < 1 || stride < 1 || window % stride || Lh < window || Lw < window || Lh % stride || Lw % stride)
    FAIL("%s: latent size %d x %d with window %d and stride %d (each side a multiple of the stride and at least the window)", what, Lh, Lw, window, stride);
  CK(check_latent_hw(c, what, window, window));
  return pano_view_grid(Lh, Lw, window, stride, nbh, nbw);
}

// The DDIM loop of a panorama: canvas [batch][4][Lh][Lw] fp32 in place.  Per step every view (window x window at (i stride, j stride), view
// v = i nbw + j) is gathered, run through the CFG UNet and stepped on its own, `view_batch` views per panorama per forward (<= 0: all of
// them); then every canvas element becomes the mean of the stepped views that cover it, summed in view order.  The context set by
// agd_set_context is the [2 batch, T, D] of the prompts; it is tiled per view here, once.  With the DAAM recorder on, the state of
// (panorama p, view v) is image v * batch + p of an agd_record_reset_hw(ctx, batch * views, window, window).
AGD_API int agd_denoise_panorama(agd_ctx* c, float* canvas, int batch, int Lh, int Lw, int window, int stride, int view_batch, int n_steps,
                                 const float* timesteps, const float* alpha_t, const float* alpha_prev, float guidance, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  int nbh = 0, nbw = 0;
  API_CK(c, check_panorama(c, "denoise_panorama", Lh, Lw, window, stride, &nbh, &nbw));
  if (batch < 1 || n_steps < 1 || !canvas || !timesteps || !alpha_t || !alpha_prev) { agd_set_error("denoise_panorama: batch %d, steps %d or a null argument", batch, n_steps); return fail_ctx(c); }
  API_CK(c, refuse_guidance_rescale(c, "denoise_panorama"));
  CallCond cc; API_CK(c, resolve_cond(c, CALL_PANORAMA, n_steps, batch, window, window, &cc));
  if (c->rec_mode == 2) { agd_set_error("denoise_panorama: the hook.py recorder is installed; a panorama records through the DAAM recorder only"); return fail_ctx(c); }
  const int V = nbh * nbw, n = (view_batch < 1 || view_batch > V) ? V : view_batch;
  const int Cl = c->cfg.out_channels, HW = window * window;
  if (c->ctx_B2 != 2 * batch) { agd_set_error("denoise_panorama: context batch %d != 2*batch %d", c->ctx_B2, 2 * batch); return fail_ctx(c); }
  if (c->rec_mode == 1 && (c->rec_B != batch * V || c->rec_Lh != window || c->rec_Lw != window)) {
    agd_set_error("denoise_panorama: the recorder holds %d images at %d x %d, this call records %d panoramas x %d views at %d x %d (agd_record_reset_hw(ctx, batch * views, window, window))",
                  c->rec_B, c->rec_Lh, c->rec_Lw, batch, V, window, window);
    return fail_ctx(c);
  }
  c->pano_B = 0;
  if (c->rec_mode == 1) { c->pano_B = batch; c->pano_Lh = Lh; c->pano_Lw = Lw; c->pano_stride = stride; }
  API_CK(c, ensure_lat(c, 2 * batch * n, window, window));
  const size_t img = (size_t)Cl * HW;
  API_CK(c, c->pano_viewb.ensure((size_t)batch * V * img * sizeof(float)));
  float* views = c->pano_viewb.as<float>();                         // [V][batch][Cl][window][window]
  const float* tp_all = nullptr;
  API_CK(c, embed_all_timesteps(c, st, timesteps, n_steps, &tp_all));
  PanoCtx pc(c, st);
  API_CK(c, pc.tile(batch, n));
  for (int s = 0; s < n_steps; ++s) {
    for (int v0 = 0; v0 < V; v0 += n) {
      const int m = V - v0 < n ? V - v0 : n;
      float* vb = views + (size_t)v0 * batch * img;
      { ProfScope ps(c, st, PC_ELEM, 0, 8.0 * batch * m * (double)img);
        API_CK(c, launch_window_gather(canvas, vb, batch, Cl, Lh, Lw, window, stride, v0, m, 1, batch, st)); }
      pc.point(batch, m);
      c->rec_base = v0 * batch; c->rec_call = m * batch;
      API_CK(c, prep_unet_input(c, st, vb, batch * m, HW));
      API_CK(c, unet_walk(c, st, c->lat_bf16, 2 * batch * m, window, window, timesteps[s], c->eps_nhwc, tp_all + (size_t)s * c->tproj_total, true));
      { ProfScope ps(c, st, PC_ELEM, 0);
        API_CK(c, launch_cfg_ddim(c->eps_nhwc, c->cfg.out_channels, vb, batch * m, Cl, HW, guidance, alpha_t[s], alpha_prev[s], c->cfg.prediction_type, nullptr, st)); }
    }
    ProfScope ps(c, st, PC_ELEM, 0, 4.0 * batch * (double)img * V + 4.0 * batch * (double)Cl * Lh * Lw);
    API_CK(c, launch_window_mean(views, canvas, batch, Cl, Lh, Lw, window, stride, 1, batch, st));
  }
  return 0;
}

// ---- Region-based MultiDiffusion (Bar-Tal et al. 2023, region_based.py of its repository [upstream-knowledge], parity-unpinned; regions.hip) ----
// The DDIM loop of R regions on ONE canvas [batch][4][Lh][Lw] fp32, in place.  Per step: the spread hands the canvas to every region (for
// the first d->bootstrapping steps a foreground region sees a noised constant-colour background outside its mask), the CFG UNet runs the
// 2 R batch rows in one forward against the context [uncond x R batch | cond x R batch] set by agd_set_context, the DDIM step updates the
// R batch rows, and the masked mean writes the canvas.  Row (region r, image p) = r * batch + p; with the DAAM recorder on that is also its
// state of an agd_record_reset_hw(ctx, R * batch, Lh, Lw).  Nothing of the call is kept in the context.
static int check_regions_desc(const agd_regions_desc* d, int n_steps) {
  if (!d) FAIL("denoise_regions: null descriptor");
  if (d->struct_size != (int)sizeof(agd_regions_desc)) FAIL("denoise_regions: descriptor struct_size %d, this library has %zu", d->struct_size, sizeof(agd_regions_desc));
  const int R = d->regions;
  if (R < 1 || R > AGD_MAX_REGIONS) FAIL("denoise_regions: %d regions (1 .. %d)", R, AGD_MAX_REGIONS);
  if (d->bootstrapping < 0 || d->bootstrapping > n_steps) FAIL("denoise_regions: bootstrapping %d outside 0 .. %d (the call's steps)", d->bootstrapping, n_steps);
  if (!d->masks) FAIL("denoise_regions: null masks");
  if (d->bootstrapping > 0 && R > 1) {
    if (d->n_backgrounds < 1) FAIL("denoise_regions: %d backgrounds for %d bootstrapped steps (at least 1)", d->n_backgrounds, d->bootstrapping);
    if (!d->noise || !d->backgrounds || !d->idx || !d->sqrt_ac) FAIL("denoise_regions: null noise, backgrounds, idx or sqrt_ac with %d bootstrapped steps", d->bootstrapping);
    for (int s = 0; s < d->bootstrapping; ++s)
      for (int r = 1; r < R; ++r) {
        const int k = d->idx[s * (R - 1) + (r - 1)];
        if (k < 0 || k >= d->n_backgrounds) FAIL("denoise_regions: background index %d (step %d, region %d) outside 0 .. %d", k, s, r, d->n_backgrounds - 1);
      }
  }
  return 0;
}
AGD_API int agd_denoise_regions(agd_ctx* c, float* canvas, int batch, int Lh, int Lw, const agd_regions_desc* d, int n_steps,
                                const float* timesteps, const float* alpha_t, const float* alpha_prev, float guidance, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  API_CK(c, check_latent_hw(c, "denoise_regions", Lh, Lw));
  if (batch < 1 || n_steps < 1 || !canvas || !timesteps || !alpha_t || !alpha_prev) { agd_set_error("denoise_regions: batch %d, steps %d or a null argument", batch, n_steps); return fail_ctx(c); }
  API_CK(c, check_regions_desc(d, n_steps));
  const int R = d->regions, rows = R * batch;
  API_CK(c, refuse_guidance_rescale(c, "denoise_regions"));
  CallCond cc; API_CK(c, resolve_cond(c, CALL_REGIONS, n_steps, rows, Lh, Lw, &cc));
  if (c->rec_mode == 2) { agd_set_error("denoise_regions: the hook.py recorder is installed; region prompts record through the DAAM recorder only"); return fail_ctx(c); }
  if (c->ctx_B2 != 2 * rows) { agd_set_error("denoise_regions: context batch %d != 2 * regions * batch = 2 * %d * %d", c->ctx_B2, R, batch); return fail_ctx(c); }
  if (c->rec_mode == 1 && (c->rec_B != rows || c->rec_Lh != Lh || c->rec_Lw != Lw)) {
    agd_set_error("denoise_regions: the recorder holds %d images at %d x %d, this call records %d regions x %d images at %d x %d (agd_record_reset_hw(ctx, regions * batch, Lh, Lw))",
                  c->rec_B, c->rec_Lh, c->rec_Lw, R, batch, Lh, Lw);
    return fail_ctx(c);
  }
  const int Cl = c->cfg.out_channels; const long long HW = (long long)Lh * Lw;
  API_CK(c, ensure_lat(c, 2 * rows, Lh, Lw));
  const size_t img = (size_t)Cl * HW;
  API_CK(c, c->reg_xb.ensure((size_t)rows * img * sizeof(float)));
  float* x = c->reg_xb.as<float>();                                 // [R][batch][Cl][Lh][Lw]
  const float* tp_all = nullptr;
  API_CK(c, embed_all_timesteps(c, st, timesteps, n_steps, &tp_all));
  for (int s = 0; s < n_steps; ++s) {
    const bool boot = s < d->bootstrapping && R > 1;
    RegionIdx ri = {};
    if (boot) for (int r = 1; r < R; ++r) ri.v[r] = d->idx[s * (R - 1) + (r - 1)];
    { ProfScope ps(c, st, PC_ELEM, 0, (boot ? 16.0 : 8.0) * rows * (double)img);
      API_CK(c, launch_region_spread(canvas, x, d->masks, d->noise, d->backgrounds, R, batch, Cl, HW, d->n_backgrounds, boot, ri,
                                     boot ? d->sqrt_ac[2 * s] : 0.f, boot ? d->sqrt_ac[2 * s + 1] : 0.f, st)); }
    API_CK(c, prep_unet_input(c, st, x, rows, (int)HW));
    API_CK(c, unet_walk(c, st, c->lat_bf16, 2 * rows, Lh, Lw, timesteps[s], c->eps_nhwc, tp_all + (size_t)s * c->tproj_total, true));
    { ProfScope ps(c, st, PC_ELEM, 0);
      API_CK(c, launch_cfg_ddim(c->eps_nhwc, c->cfg.out_channels, x, rows, Cl, (int)HW, guidance, alpha_t[s], alpha_prev[s], c->cfg.prediction_type, nullptr, st)); }
    ProfScope ps(c, st, PC_ELEM, 0, 4.0 * rows * (double)img + 4.0 * rows * (double)HW + 4.0 * batch * (double)img);
    API_CK(c, launch_region_mean(x, d->masks, canvas, R, batch, Cl, HW, st));
  }
  return 0;
}

// The denoise loop under the reference's ACTUAL scheduler: `pipeline(prompt, num_inference_steps=20)` at
// data_generation.py:59 runs the checkpoint's PNDMScheduler (skip_prk_steps, i.e. PLMS) -- n_evals = steps + 1 model
// evaluations, the second timestep evaluated twice [upstream-knowledge: diffusers 0.21.2 PNDMScheduler.step_plms].
// Per evaluation i the host passes the UNet timestep and the two coefficients of `_get_prev_sample`
// (prev = sample_coeff[i] * sample + eps_coeff[i] * model_output); the linear-multistep weights are applied here:
//   i = 0: e0                       (the sample is kept: evaluation 1 restarts from it)
//   i = 1: (e1 + e0) / 2 from the KEPT sample (e1 is not added to the history)
//   then : (3 e - h1) / 2 ; (23 e - 16 h1 + 5 h2) / 12 ; (55 e - 59 h1 + 37 h2 - 9 h3) / 24
AGD_API int agd_denoise_plms_hw(agd_ctx* c, float* latents, int batch, int Lh, int Lw, int n_evals, const float* timesteps, const float* sample_coeff,
                             const float* eps_coeff, float guidance, void* stream) {
  API_CK(c, need_final(c));
  API_CK(c, check_latent_hw(c, "denoise_plms", Lh, Lw));
  hipStream_t st = S(stream);
  if (c->cfg.prediction_type != 0) { agd_set_error("denoise_plms: epsilon prediction only"); return fail_ctx(c); }
  if (n_evals < 2) { agd_set_error("denoise_plms: needs >= 2 model evaluations (got %d)", n_evals); return fail_ctx(c); }
  const int Cl = c->cfg.out_channels, HW = Lh * Lw;
  const size_t n1 = (size_t)batch * Cl * HW;
  API_CK(c, check_guidance_rescale(c, "denoise_plms", Cl, HW));
  API_CK(c, c->plmsb.ensure(n1 * 5 * sizeof(float)));            // 4 history slots + the kept sample
  float* hist[4]; for (int k = 0; k < 4; ++k) hist[k] = c->plmsb.as<float>() + n1 * k;
  float* kept = c->plmsb.as<float>() + n1 * 4;                    // the blend rewrites `latents` only: the kept sample stays unblended
  int n_hist = 0, head = 0;                                       // hist[(head - 1 - k) & 3] = k-th newest stored eps
  API_CK(c, run_eval_loop(c, st, latents, batch, Lh, Lw, n_evals, timesteps, [&](int i, const float* eps) {
    float w[4] = {1.f, 0.f, 0.f, 0.f};
    const float* h[3] = {nullptr, nullptr, nullptr};
    const float* src = latents; float* store = nullptr;
    if (i == 1) {                                                 // PLMS second call: average with e0, restart from the kept sample
      w[0] = 0.5f; w[1] = 0.5f; h[0] = hist[(head - 1) & 3]; src = kept;
    } else {
      if (i == 0 && hipMemcpyAsync(kept, latents, n1 * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("plms: keep sample");
      store = hist[head & 3];
      for (int k = 0; k < 3 && k < n_hist; ++k) h[k] = hist[(head - 1 - k) & 3];
      if (n_hist == 1) { w[0] = 1.5f; w[1] = -0.5f; }
      else if (n_hist == 2) { w[0] = 23.f / 12.f; w[1] = -16.f / 12.f; w[2] = 5.f / 12.f; }
      else if (n_hist >= 3) { w[0] = 55.f / 24.f; w[1] = -59.f / 24.f; w[2] = 37.f / 24.f; w[3] = -9.f / 24.f; }
    }
    ProfScope ps(c, st, PC_ELEM, 0);
    const float* f; CK(guidance_factor(c, st, eps, batch, Cl, HW, guidance, &f));
    CK(launch_cfg_plms(eps, c->cfg.out_channels, latents, src, h[0], h[1], h[2], store, batch, Cl, HW, guidance, w, sample_coeff[i],
                       eps_coeff[i], f, st));
    if (store) { ++head; if (n_hist < 3) ++n_hist; }
    return 0;
  }));
  return 0;
}
AGD_API int agd_denoise_plms(agd_ctx* c, float* latents, int batch, int L, int n_evals, const float* timesteps, const float* sample_coeff,
                             const float* eps_coeff, float guidance, void* stream) {
  return agd_denoise_plms_hw(c, latents, batch, L, L, n_evals, timesteps, sample_coeff, eps_coeff, guidance, stream);
}

// The denoise loop under DPM-Solver++ (2M) [upstream-knowledge: diffusers 0.21.2 DPMSolverMultistepScheduler, algorithm_type
// "dpmsolver++", midpoint]: one model evaluation per step.  The host scheduler (agenda_amd/scheduler.py dpm_program) passes, per
// evaluation i, the UNet timestep (fractional with Karras sigmas) and coeffs[5 i ..]: cx, ce, a, b0, b1 with
//   x0 = cx x + ce m  (m: CFG-combined model output; eps or v is folded into cx / ce),  x = a x + b0 x0 + b1 x0_prev
// so first / second order, the lower-order final step and the prediction type are all host decisions.  x0 ping-pongs between the
// two halves of the context-owned dpmb buffer: evaluation i reads slot (i - 1) & 1 and writes slot i & 1.
AGD_API int agd_denoise_dpm_hw(agd_ctx* c, float* latents, int batch, int Lh, int Lw, int n_evals, const float* timesteps, const float* coeffs,
                            float guidance, void* stream) {
  API_CK(c, need_final(c));
  API_CK(c, check_latent_hw(c, "denoise_dpm", Lh, Lw));
  hipStream_t st = S(stream);
  if (n_evals < 1 || !timesteps || !coeffs) { agd_set_error("denoise_dpm: needs >= 1 model evaluation and host timesteps / coeffs (got %d)", n_evals); return fail_ctx(c); }
  const int Cl = c->cfg.out_channels, HW = Lh * Lw;
  const size_t n1 = (size_t)batch * Cl * HW;
  API_CK(c, check_guidance_rescale(c, "denoise_dpm", Cl, HW));
  API_CK(c, c->dpmb.ensure(n1 * 2 * sizeof(float)));
  float* slot[2] = {c->dpmb.as<float>(), c->dpmb.as<float>() + n1};
  API_CK(c, run_eval_loop(c, st, latents, batch, Lh, Lw, n_evals, timesteps, [&](int i, const float* eps) {
    const float* prev = i > 0 ? slot[(i - 1) & 1] : nullptr;
    float* store = i + 1 < n_evals ? slot[i & 1] : nullptr;     // the last x0 has no reader
    ProfScope ps(c, st, PC_ELEM, 0);
    const float* f; CK(guidance_factor(c, st, eps, batch, Cl, HW, guidance, &f));
    return launch_cfg_dpm(eps, c->cfg.out_channels, latents, prev, store, batch, Cl, HW, guidance, coeffs + (size_t)5 * i, f, st);
  }));
  return 0;
}
AGD_API int agd_denoise_dpm(agd_ctx* c, float* latents, int batch, int L, int n_evals, const float* timesteps, const float* coeffs,
                            float guidance, void* stream) {
  return agd_denoise_dpm_hw(c, latents, batch, L, L, n_evals, timesteps, coeffs, guidance, stream);
}

AGD_API int agd_vae_decode_hw(agd_ctx* c, const float* latents, int batch, int Lh, int Lw, unsigned char* out_u8, float* out_f32, void* stream) {
  API_CK(c, need_final(c));
  if (Lh < 1 || Lw < 1) { agd_set_error("vae_decode: latent size %d x %d", Lh, Lw); return fail_ctx(c); }
  hipStream_t st = S(stream);
  API_CK(c, ensure_lat(c, batch, Lh, Lw));
  const int sh = c->cfg.vae_n_levels - 1;
  const long long npix = (long long)batch * (Lh << sh) * (Lw << sh);
  { ProfScope ps(c, st, PC_ELEM, 0);
    API_CK(c, launch_prep_latents(latents, c->lat_bf16, batch, c->cfg.vae_latent_channels, Lh * Lw, 64, 1, 1.0f / c->cfg.vae_scaling_factor, st)); }
  API_CK(c, c->vae_imgb.ensure((size_t)npix * 4 * 4));     // grows once per (batch, size); stream-ordered reuse, no sync
  float* img = c->vae_imgb.as<float>();
  int rc = vae_walk(c, st, c->lat_bf16, batch, Lh, Lw, img);
  if (rc == 0 && out_u8) { ProfScope ps(c, st, PC_ELEM, 0); rc = launch_image_u8(img, 4, out_u8, npix, c->cfg.vae_out_channels, st); }
  if (rc == 0 && out_f32) {
    // [npix][4] -> [npix][3] : "NCHW from NHWC" with HW=1 does exactly that per pixel
    rc = launch_nchw_from_nhwc_f32(img, 4, out_f32, (int)npix, c->cfg.vae_out_channels, 1, st);
  }
  return rc ? fail_ctx(c) : 0;
}
AGD_API int agd_vae_decode(agd_ctx* c, const float* latents, int batch, int L, unsigned char* out_u8, float* out_f32, void* stream) {
  return agd_vae_decode_hw(c, latents, batch, L, L, out_u8, out_f32, stream);
}

// ---- options --------------------------------------------------------------------------
AGD_API int agd_set_option(agd_ctx* c, const char* name, int value) {
  if (!c || !name) { agd_set_error("set_option: null argument"); return fail_ctx(c); }
  if (!strcmp(name, "cfg_shared_prefix")) { c->opt_cfg_share = value != 0; return 0; }
  if (!strcmp(name, "ln_fold")) { c->opt_ln_fold = value; return 0; }       // 0 off, 1 on; 2 / 3: only blocks with C <= 320 / 640 (A/B)
  if (!strcmp(name, "gn_fused_stats")) { c->opt_gn_fused = value != 0; return 0; }
  if (!strcmp(name, "weight_touch")) { c->opt_touch = value < 0 ? 0 : value; return 0; }
  if (!strcmp(name, "weight_warm")) { c->opt_warm = value; return 0; }
  if (!strcmp(name, "conv_halo")) { c->opt_halo = value != 0; return 0; }
  if (!strcmp(name, "gn_proj_fold")) { c->opt_gn_proj_fold = value < 0 ? 0 : value; return 0; }   // 0 off, 1: blocks with C <= 320, 2: C <= 640 (A/B)
  if (!strcmp(name, "tblock_fuse")) { c->opt_tb_fuse = value < 0 ? 0 : value; return 0; }   // the TBF_* bits
  if (!strcmp(name, "reduce_gn")) { c->opt_reduce_gn = value != 0; return 0; }
  if (!strcmp(name, "xcd_block")) { c->opt_xcd_block = value != 0; return 0; }
  if (!strcmp(name, "igemm_pc")) { c->opt_pc = value < 0 ? 0 : value; return 0; }
  if (!strcmp(name, "attn2_premul")) { c->opt_xpre = value < 0 ? 0 : value; return 0; }     // takes effect at the next agd_set_context (the products are built there)
  if (!strcmp(name, "conv_smap")) { c->opt_smap = value != 0; return 0; }
  if (!strcmp(name, "side_stream")) { c->opt_side = value < 0 ? 0 : value; return 0; }
  if (!strcmp(name, "igemm_kgroups")) { c->opt_kg2 = value != 0; return 0; }
  if (!strcmp(name, "upsample_phases")) { c->opt_ups4 = value & 15; return 0; }      // bit 0: the UNet's upsamplers from 16 x 16 maps up, bit 1: the VAE decoder's, bit 2: the UNet's 8 x 8 -> 16 x 16 one too
  if (!strcmp(name, "ff_proj_fuse")) { c->opt_ffproj = value != 0; return 0; }
  if (!strcmp(name, "shortcut_fuse")) { c->opt_sc_fuse = value & 3; return 0; }      // bit 0: row-halo launches (64 x 64 .. 16 x 16 maps), bit 1: the 8 x 8 whole-images launches
  if (!strcmp(name, "wreg_mask")) { c->opt_wreg = value & 3; return 0; }
  if (!strcmp(name, "igemm8p")) { c->opt_p8 = value < 0 ? 0 : value; return 0; }   // 0 off, 1 on (the launcher decides per launch); tests: 2 / 3 / 4 force the 256-wide / 160-wide / any legal tile
  agd_set_error("set_option: unknown option '%s'", name);
  return fail_ctx(c);
}

// ---- recorder -------------------------------------------------------------------------
AGD_API int agd_record_config(agd_ctx* c, int mode, int is_train, int rec_tokens) {
  if (!c) return -1;
  if (mode < 0 || mode > 2) { agd_set_error("record_config: mode %d", mode); return fail_ctx(c); }
  c->rec_mode = mode; c->rec_is_train = is_train; c->rec_T_cfg = rec_tokens;   // takes effect at the next agd_record_reset
  return 0;
}

// hook.py recorder state for `rows` kept batch rows (B' of hook.py:48-55) at latent side L: running sum, per-call scratch
static int hook_reset_rows(agd_ctx* c, int rows, int L, hipStream_t st) {
  const int Tc = c->ctx_T > 0 ? c->ctx_T : c->cfg.max_tokens;
  const size_t n = (size_t)rows * Tc * L * L;
  CK(c->hook_sumb.ensure(n * 4)); CK(c->hook_scratchb.ensure(n * 4));
  c->hook_sum = c->hook_sumb.as<float>(); c->hook_scratch = c->hook_scratchb.as<float>();
  c->hook_Bp = rows; c->hook_T = Tc;
  if (hipMemsetAsync(c->hook_sum, 0, n * 4, st) != hipSuccess) FAIL("memset hook");
  c->hook_count = 0; c->hook_recs.clear(); c->hook_store_used = 0;
  return 0;
}

// `hooker.clear()` with the number of recorded batch rows given explicitly (training calls the UNet without CFG: any batch)
AGD_API int agd_hook_reset(agd_ctx* c, int rows, int L, void* stream) {
  API_CK(c, need_final(c));
  if (c->rec_mode != 2) { agd_set_error("hook_reset: recorder is not in hook.py mode (agd_record_config(2, ..))"); return fail_ctx(c); }
  if (rows < 1 || L < 1) { agd_set_error("hook_reset: rows %d latent side %d", rows, L); return fail_ctx(c); }
  if (c->ctx_T > 96) { agd_set_error("hook_reset: the hook.py recorder takes contexts of at most 96 tokens (this one has %d)", c->ctx_T); return fail_ctx(c); }
  API_CK(c, hook_reset_rows(c, rows, L, S(stream)));
  c->rec_B = c->rec_is_train ? (rows + 1) / 2 : rows; c->rec_L = c->rec_Lh = c->rec_Lw = L;
  return 0;
}

AGD_API int agd_record_reset_hw(agd_ctx* c, int batch, int Lh, int Lw, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (batch < 1 || Lh < 1 || Lw < 1) { agd_set_error("record_reset: batch %d latent size %d x %d", batch, Lh, Lw); return fail_ctx(c); }
  if (c->rec_mode == 2 && Lh != Lw) { agd_set_error("record_reset: the hook.py recorder takes square latents only (got %d x %d)", Lh, Lw); return fail_ctx(c); }
  const int T = c->rec_T_cfg > 0 ? c->rec_T_cfg : c->cfg.max_tokens;
  const bool long_ctx = c->ctx_T > 96;                 // attention_long.hip records per-head rows only: no head-group sums at any level
  if (c->rec_mode == 2 && long_ctx) { agd_set_error("record_reset: the hook.py recorder takes contexts of at most 96 tokens (this one has %d)", c->ctx_T); return fail_ctx(c); }
  if (c->rec_mode == 1 && long_ctx && T > c->ctx_T) { agd_set_error("record_reset: rec_tokens %d > the context's %d tokens", T, c->ctx_T); return fail_ctx(c); }
  c->rec_T = T;
  if (c->rec_mode == 1) {
    for (auto& xl : c->xl) {
      if (xl.mid || xl.cn) continue;
      // daam: a layer's maps are (Lh / f) x (Lw / f) with f = sqrt(Lh * Lw / N) = 2^level; f == 8 is not recorded
      const int h = Lh >> xl.level, w = Lw >> xl.level;
      if (h < 1 || w < 1 || (Lh / h) == 8) { xl.acc = nullptr; xl.acc_h = xl.acc_w = 0; continue; }
      // capacity-tracked: a larger batch / token count / side than the block was allocated for reallocates it
      // daam averages clamp(bicubic(map), 0) over every (layer, head) map.  At latent resolution the resize is the identity and the
      // clamp cannot fire (sums of probabilities), so heads are summed in the recording kernel: down to 1/8 of the state and traffic
      xl.acc_heads = xl.heads;
      if (xl.level == 0 && !long_ctx) {   // heads per workgroup: as many as still leave >= 256 workgroups (UNet batch x head groups x 128-query tiles)
        int hpb = xl.heads;
        while (hpb > 1 && hpb % 2 == 0 && (long long)2 * batch * (xl.heads / hpb) * ((h * w + 127) / 128) < 256) hpb /= 2;
        xl.acc_heads = xl.heads / hpb;
      }
      const size_t n = (size_t)batch * xl.acc_heads * T * h * w;
      API_CK(c, xl.accb.ensure(n * 4)); xl.acc = xl.accb.as<float>(); xl.acc_h = h; xl.acc_w = w;
      if (hipMemsetAsync(xl.acc, 0, n * 4, st) != hipSuccess) { agd_set_error("memset acc"); return fail_ctx(c); }
    }
  } else if (c->rec_mode == 2) {
    API_CK(c, hook_reset_rows(c, c->rec_is_train ? 2 * batch : batch, Lh, st));   // `batch` = images; UNet batch is 2*batch under CFG
  }
  c->rec_B = batch; c->rec_L = Lh; c->rec_Lh = Lh; c->rec_Lw = Lw; c->pano_B = 0;
  return 0;
}
AGD_API int agd_record_reset(agd_ctx* c, int batch, int L, void* stream) {
  return agd_record_reset_hw(c, batch, L, L, stream);
}

AGD_API int agd_daam_global(agd_ctx* c, int img, int rows, float* out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  std::vector<HeatLayer> hl; int total = 0;
  for (auto& xl : c->xl) {
    if (!xl.acc || xl.mid) continue;
    HeatLayer h; h.acc = xl.acc; h.h = xl.acc_h; h.w = xl.acc_w; h.heads = xl.acc_heads;
    h.head_stride = (long long)c->rec_T * xl.acc_h * xl.acc_w; h.img_stride = h.head_stride * xl.acc_heads;
    hl.push_back(h); total += xl.heads;                            // the mean is over (layer, head) maps either way
  }
  if (hl.empty() || c->rec_mode != 1) { agd_set_error("No heat maps found. Did you forget to call `with trace(...)`?"); c->err = g_err; return -2; }
  if (rows > c->rec_T || img >= c->rec_B) { agd_set_error("daam_global: rows %d > recorded %d or img %d >= %d", rows, c->rec_T, img, c->rec_B); return fail_ctx(c); }
  { ProfScope ps(c, st, PC_HEAT, 0); API_CK(c, launch_daam_global(hl.data(), (int)hl.size(), total, rows, c->rec_Lh, c->rec_Lw, img, out, st)); }
  return 0;
}

// The heat map of a whole panorama (this project's definition; daam has no panorama support): the per-view global map of each of panorama
// `img`'s views -- launch_daam_global at window x window, unchanged -- then the overlap mean of the views, exactly as the latents are fused.
// out [rows][Lh][Lw] at the canvas size of the last agd_denoise_panorama, whose recorder state it reads: batch * views images, (panorama p,
// view v) at v * batch + p.
AGD_API int agd_daam_global_panorama(agd_ctx* c, int img, int rows, float* out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  const int win = c->rec_Lh, batch = c->pano_B, Lh = c->pano_Lh, Lw = c->pano_Lw, stride = c->pano_stride;
  if (c->rec_mode != 1 || win < 1 || c->rec_Lw != win || batch < 1) { agd_set_error("No heat maps found. Did you forget to call `with trace(...)`?"); c->err = g_err; return -2; }
  int nbh = 0, nbw = 0;
  API_CK(c, check_panorama(c, "daam_global_panorama", Lh, Lw, win, stride, &nbh, &nbw));
  const int V = nbh * nbw;
  if (batch < 1 || c->rec_B != batch * V || img < 0 || img >= batch || rows < 1 || rows > c->rec_T) {
    agd_set_error("daam_global_panorama: panorama %d of %d with %d views and %d rows, the recorder holds %d images and %d rows", img, batch, V, rows, c->rec_B, c->rec_T);
    return fail_ctx(c);
  }
  const size_t per = (size_t)rows * win * win;
  API_CK(c, c->pano_hmb.ensure((size_t)V * per * sizeof(float)));
  float* hm = c->pano_hmb.as<float>();                              // [V][rows][win][win]
  for (int v = 0; v < V; ++v) {
    const int rc = agd_daam_global(c, v * batch + img, rows, hm + (size_t)v * per, stream);
    if (rc != 0) return rc;
  }
  ProfScope ps(c, st, PC_HEAT, 0, 4.0 * V * (double)per + 4.0 * rows * (double)Lh * Lw);
  API_CK(c, launch_window_mean(hm, out, 1, rows, Lh, Lw, win, stride, V, 1, st));
  return 0;
}

AGD_API int agd_hook_count(agd_ctx* c) { return c ? c->hook_count : 0; }

AGD_API int agd_hook_last_map(agd_ctx* c, float* out, int n_query, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (c->hook_count == 0 || !c->hook_scratch) { agd_set_error("No heat maps found."); c->err = g_err; return -2; }
  const size_t n = (size_t)c->hook_Bp * c->hook_T * n_query;
  if (hipMemcpyAsync(out, c->hook_scratch, n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { agd_set_error("hook_last_map copy"); return fail_ctx(c); }
  return 0;
}

AGD_API int agd_hook_global(agd_ctx* c, float* out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (c->hook_count == 0 || !c->hook_sum) { agd_set_error("No heat maps found."); c->err = g_err; return -2; }
  const long long n = (long long)c->hook_Bp * c->hook_T * c->rec_L * c->rec_L;
  hipMemcpyAsync(out, c->hook_sum, (size_t)n * 4, hipMemcpyDeviceToDevice, st);
  API_CK(c, launch_scale(out, n, 1.0f / (float)c->hook_count, st));
  return 0;
}

// The processor seam: one `Attention` module call of the UNet, hook.py:83-122 in full.
//   layer "...attn2" + ctx_emb        -> cross-attention (is_cross, hook.py:95-99), feeds the recorder when record != 0
//   layer "...attn1" + ctx_emb NULL   -> self-attention (encoder_hidden_states = hidden_states), records nothing
//   attn_mask: additive fp32 [batch2][keys] or NULL (hook.py:92 prepare_attention_mask -> hook.py:108 get_attention_scores)
// Output is to_out[0](attention) + bias (to_out[1] is Dropout(0)); the residual is the caller's (BasicTransformerBlock).
AGD_API int agd_attn_processor(agd_ctx* c, const char* layer, const float* hidden, const float* ctx_emb, const float* attn_mask,
                               int batch2, int n_query, int tokens, float* out, int record, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!layer || !hidden || !out || batch2 < 1 || n_query < 1) { agd_set_error("attn_processor: bad argument"); return fail_ctx(c); }
  std::string name(layer);
  if (name.compare(0, 5, "unet.") != 0) name = "unet." + name;
  const bool is_attn2 = ends_with(name, "attn2"), is_attn1 = ends_with(name, "attn1");
  if (!is_attn1 && !is_attn2) { agd_set_error("attn_processor: unknown layer '%s' (neither an attn1 nor an attn2 module)", layer); return fail_ctx(c); }
  const std::string t = name.substr(0, name.size() - 5);
  auto it = c->xl_idx.find(t + "attn2");
  if (it == c->xl_idx.end()) { agd_set_error("attn_processor: unknown layer '%s'", layer); return fail_ctx(c); }
  XLayer& xl = c->xl[it->second];
  const int C = xl.C, M = batch2 * n_query;
  if (is_attn2) {
    // cross-attention needs the text context (a self-attention call on attn2 would feed C-wide rows to a ctx_dim-wide to_k)
    if (ctx_emb) API_CK(c, agd_set_context(c, ctx_emb, batch2, tokens, stream));
    else if (c->ctx_T <= 0) { agd_set_error("attn_processor: attn2 called without encoder_hidden_states and no context set"); return fail_ctx(c); }
    if (c->ctx_B2 != batch2) { agd_set_error("attn_processor: context batch %d != %d", c->ctx_B2, batch2); return fail_ctx(c); }
    if (record && c->ctx_T > 96) { agd_set_error("attn_processor: recording takes contexts of at most 96 tokens (this one has %d)", c->ctx_T); return fail_ctx(c); }
  } else if (ctx_emb) {
    agd_set_error("attn_processor: attn1 is the self-attention module (encoder_hidden_states must be NULL)"); return fail_ctx(c);
  }
  c->arena.release(0);
  bf16_t* x = (bf16_t*)c->arena.alloc((size_t)M * C * 2);
  bf16_t* q = (bf16_t*)c->arena.alloc((size_t)M * (is_attn2 ? 1 : 3) * C * 2);
  bf16_t* att = (bf16_t*)c->arena.alloc((size_t)M * C * 2);
  if (!x || !q || !att) return fail_ctx(c);
  API_CK(c, launch_f32_to_bf16(hidden, x, (long long)M * C, st));
  const std::string an = t + (is_attn2 ? "attn2." : "attn1.");
  const WMat* wo = getW(c, an + "to_out.0.weight"); const float* bo = getV(c, an + "to_out.0.bias");
  if (!wo || !bo) return fail_ctx(c);
  if (is_attn2) {
    const WMat* wq = getW(c, an + "to_q.weight"); if (!wq) return fail_ctx(c);
    { GemmOpt o; API_CK(c, run_conv(c, st, x, C, nullptr, 0, 1, 1, M, *wq, 1, q, o, c->zero_page)); }
    const int qs = (int)lrintf(sqrtf((float)n_query));      // the seam's query maps are square (hook.py's _unravel_attn)
    API_CK(c, cross_attention(c, st, xl, q, batch2, n_query, qs, qs, att, record != 0, attn_mask));
  } else {
    const WMat* wqkv = getW(c, t + "attn1.qkv"); if (!wqkv) return fail_ctx(c);
    { GemmOpt o; API_CK(c, run_conv(c, st, x, C, nullptr, 0, 1, 1, M, *wqkv, 1, q, o, c->zero_page)); }
    AttnP a{}; a.q = q; a.k = q + C; a.v = q + 2 * C; a.o = att;
    a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C; a.sq = a.sk = a.sv = (long long)n_query * 3 * C; a.so = (long long)n_query * C;
    a.B = batch2; a.H = xl.heads; a.D = C / xl.heads; a.Nq = n_query; a.Nk = n_query; a.scale = 1.0f / sqrtf((float)(C / xl.heads));
    a.mask = attn_mask;
    API_CK(c, run_attention(c, st, PC_ATTN_SELF, a));
  }
  { GemmOpt o; o.bias = bo; o.out_f32 = 1; API_CK(c, run_conv(c, st, att, C, nullptr, 0, 1, 1, M, *wo, 1, out, o, c->zero_page)); }
  return 0;
}

// ---- training-mode seam -------------------------------------------------------------------
AGD_API int agd_hook_num_maps(agd_ctx* c) { return c ? (int)c->hook_recs.size() : 0; }

// hook.py:110-112: the k-th map appended since the last clear() (train mode keeps them all): dims = {B', T, n_query}
AGD_API int agd_hook_map_dims(agd_ctx* c, int k, int* dims) {
  if (!c || !dims || k < 0 || k >= (int)c->hook_recs.size()) { agd_set_error("hook_map: no recorded map %d (have %d; is_train keeps per-call maps)", k, c ? (int)c->hook_recs.size() : 0); return fail_ctx(c); }
  dims[0] = c->hook_recs[k].Bp; dims[1] = c->hook_recs[k].T; dims[2] = c->hook_recs[k].N;
  return 0;
}
AGD_API int agd_hook_map(agd_ctx* c, int k, float* out, void* stream) {
  API_CK(c, need_final(c));
  if (k < 0 || k >= (int)c->hook_recs.size()) { agd_set_error("hook_map: no recorded map %d (have %d)", k, (int)c->hook_recs.size()); return fail_ctx(c); }
  const auto& r = c->hook_recs[k];
  if (hipMemcpyAsync(out, (const char*)c->hook_storeb.p + r.off, (size_t)r.Bp * r.T * r.N * 4, hipMemcpyDeviceToDevice, S(stream)) != hipSuccess) { agd_set_error("hook_map copy"); return fail_ctx(c); }
  return 0;
}

// finetune_sd_token.py:1046-1066 for ONE recorded map [B][T][P] (P = h*w): loss_out [B][2] = {bg, fg} terms of each sample
// (already times coef = reg_weight / #samples with an object), dmap [B][T][P] (may be NULL) = their gradient w.r.t. the map.
// obj/fg/bg_idx: device int [B], obj < 0 skips the sample (no object in the image, :1048).
AGD_API int agd_op_attn_reg_loss(const float* map, int B, int T, int P, const int* obj_idx, const int* fg_idx, const int* bg_idx, float coef,
                                 float* loss_out, float* dmap, void* stream) {
  if (!map || !obj_idx || !fg_idx || !bg_idx || !loss_out || B < 0 || T < 1 || P < 1) { agd_set_error("attn_reg_loss: bad argument"); return -1; }
  CK(launch_attn_reg_loss(map, B, T, P, obj_idx, fg_idx, bg_idx, coef, loss_out, dmap, S(stream)));
  return 0;
}

static int transposed(agd_ctx* c, hipStream_t st, const WMat& w, DBuf& buf, WMat& out) {
  if (out.w) return 0;
  const int K = w.taps * w.Cpad;
  CK(buf.ensure((size_t)w.N * K * 2));
  CK(launch_transpose_bf16(w.w, w.N, K, buf.as<bf16_t>(), st));
  out.w = buf.as<bf16_t>(); out.N = K; out.Cin = w.N; out.Cpad = w.N; out.taps = 1;
  return 0;
}

// Backward of one cross-attention call of the seam (hook.py:91-120) w.r.t. its inputs:
//   d_out  [B2, N, C] fp32 or NULL: gradient of the returned hidden_states
//   d_map  [B', T, N] fp32 or NULL: gradient of the recorded head-mean map (hook.py:55; B' = B2 in train mode, the
//          conditional half B2/2 otherwise, hook.py:48-49) -- e.g. from agd_op_attn_reg_loss
//   -> d_hidden [B2, N, C] and d_ctx [B2, T, ctx_dim] fp32 (either may be NULL)
// P is recomputed from Q = to_q(hidden) and the cached K/V of `ctx_emb` (bf16 operands, fp32 arithmetic, like the forward).
AGD_API int agd_attn_processor_backward(agd_ctx* c, const char* layer, const float* hidden, const float* ctx_emb, const float* d_out,
                                        const float* d_map, int is_train, int batch2, int n_query, int tokens, float* d_hidden, float* d_ctx,
                                        void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!layer || !hidden || (!d_out && !d_map) || batch2 < 1 || n_query < 1) { agd_set_error("attn_processor_backward: bad argument"); return fail_ctx(c); }
  std::string name(layer);
  if (name.compare(0, 5, "unet.") != 0) name = "unet." + name;
  auto it = c->xl_idx.find(name);
  if (it == c->xl_idx.end() || !ends_with(name, "attn2")) { agd_set_error("attn_processor_backward: unknown cross-attention layer '%s'", layer); return fail_ctx(c); }
  XLayer& xl = c->xl[it->second];
  if (ctx_emb) API_CK(c, agd_set_context(c, ctx_emb, batch2, tokens, stream));
  if (c->ctx_B2 != batch2 || c->ctx_T < 1) { agd_set_error("attn_processor_backward: context batch %d != %d", c->ctx_B2, batch2); return fail_ctx(c); }
  if (c->ctx_T > 96) { agd_set_error("attn_processor_backward: takes contexts of at most 96 tokens (this one has %d)", c->ctx_T); return fail_ctx(c); }
  const int C = xl.C, H = xl.heads, D = C / H, T = c->ctx_T, M = batch2 * n_query, Dc = c->cfg.cross_attention_dim;
  const std::string t = xl.name.substr(0, xl.name.size() - 5);
  const WMat* wq = getW(c, t + "attn2.to_q.weight"); const WMat* wo = getW(c, t + "attn2.to_out.0.weight");
  if (!wq || !wo) return fail_ctx(c);
  API_CK(c, transposed(c, st, *wq, xl.wqTb, xl.wqT)); API_CK(c, transposed(c, st, xl.wkv, xl.wkvTb, xl.wkvT)); API_CK(c, transposed(c, st, *wo, xl.woTb, xl.woT));
  API_CK(c, c->bwd_wsb.ensure((size_t)attention_backward_ws_floats(batch2, H, D, n_query, T) * 4));
  c->arena.release(0);
  bf16_t* x = (bf16_t*)c->arena.alloc((size_t)M * C * 2); bf16_t* q = (bf16_t*)c->arena.alloc((size_t)M * C * 2);
  bf16_t* dy = d_out ? (bf16_t*)c->arena.alloc((size_t)M * C * 2) : nullptr; bf16_t* dO = d_out ? (bf16_t*)c->arena.alloc((size_t)M * C * 2) : nullptr;
  bf16_t* dq = (bf16_t*)c->arena.alloc((size_t)M * C * 2); bf16_t* dkv = (bf16_t*)c->arena.alloc((size_t)batch2 * T * 2 * C * 2);
  if (!x || !q || !dq || !dkv || (d_out && (!dy || !dO))) return fail_ctx(c);
  API_CK(c, launch_f32_to_bf16(hidden, x, (long long)M * C, st));
  { GemmOpt o; API_CK(c, run_conv(c, st, x, C, nullptr, 0, 1, 1, M, *wq, 1, q, o, c->zero_page)); }                  // Q = to_q(hidden), hook.py:93
  if (d_out) {                                                                                                       // dO = d_out . Wo  (hook.py:118)
    API_CK(c, launch_f32_to_bf16(d_out, dy, (long long)M * C, st));
    GemmOpt o; API_CK(c, run_conv(c, st, dy, C, nullptr, 0, 1, 1, M, xl.woT, 1, dO, o, c->zero_page));
  }
  API_CK(c, launch_attention_backward(q, xl.kv, dO, d_map, is_train ? 0 : batch2 / 2, batch2, H, D, n_query, T, 1.0f / sqrtf((float)D), dq, dkv,
                                      c->bwd_wsb.as<float>(), st));
  if (d_hidden) { GemmOpt o; o.out_f32 = 1; API_CK(c, run_conv(c, st, dq, C, nullptr, 0, 1, 1, M, xl.wqT, 1, d_hidden, o, c->zero_page)); }          // dX = dQ . Wq
  if (d_ctx) { GemmOpt o; o.out_f32 = 1; API_CK(c, run_conv(c, st, dkv, 2 * C, nullptr, 0, 1, 1, batch2 * T, xl.wkvT, 1, d_ctx, o, c->zero_page)); } // dCtx = [dK | dV] . Wkv
  (void)Dc;
  return 0;
}

AGD_API int agd_cross_attn(agd_ctx* c, const char* layer, const float* hidden, const float* ctx_emb, int batch2, int n_query,
                           int tokens, float* out, int record, void* stream) {
  return agd_attn_processor(c, layer, hidden, ctx_emb, nullptr, batch2, n_query, tokens, out, record, stream);
}

// ---- profiling ------------------------------------------------------------------------
AGD_API int agd_profile_begin(agd_ctx* c) {
  if (!c) return -1;
  c->prof.clear(); c->ev_used = 0; c->prof_on = true;
  for (int i = 0; i < AGD_N_CLASSES; ++i) c->launches[i] = 0;
  return 0;
}
// per class: Sum of HIP-event ms, algorithmic flop and HBM bytes, launches, and roof_ms = Sum over launches of
// max(flop / mfma_peak, bytes / hbm_peak) -- the time the launch's BINDING roof allows (short-K GEMMs are HBM-bound)
AGD_API int agd_profile_end_ex(agd_ctx* c, double mfma_peak_flops, double hbm_peak_bytes, double* ms, double* flops, double* bytes,
                               double* roof_ms, double* roof_ms_hbm_bound, long long* launches) {
  if (!c || !ms || !flops || !bytes || !roof_ms || !launches) return -1;
  hipSetDevice(c->device);
  hipDeviceSynchronize();
  for (int i = 0; i < AGD_N_CLASSES; ++i) { ms[i] = 0; flops[i] = 0; bytes[i] = 0; roof_ms[i] = 0; launches[i] = c->launches[i]; if (roof_ms_hbm_bound) roof_ms_hbm_bound[i] = 0; }
  for (auto& pe : c->prof) {
    float t = 0; hipEventElapsedTime(&t, pe.a, pe.b);
    ms[pe.cls] += t; flops[pe.cls] += pe.flops; bytes[pe.cls] += pe.bytes;
    const double tm = mfma_peak_flops > 0 ? pe.flops / mfma_peak_flops * 1e3 : 0, th = hbm_peak_bytes > 0 ? pe.bytes / hbm_peak_bytes * 1e3 : 0;
    roof_ms[pe.cls] += tm > th ? tm : th;
    if (roof_ms_hbm_bound && th > tm) roof_ms_hbm_bound[pe.cls] += th;
  }
  c->prof_on = false; c->prof.clear(); c->ev_used = 0;
  return 0;
}
AGD_API int agd_profile_end(agd_ctx* c, double* ms, double* flops, long long* launches) {
  double by[AGD_N_CLASSES], rf[AGD_N_CLASSES];
  return agd_profile_end_ex(c, 0, 0, ms, flops, by, rf, nullptr, launches);
}

// ---------------------------------------------------------------------------------------
// single-op entry points (fp32 in/out; temp device buffers per call; used by parity tests)
// ---------------------------------------------------------------------------------------
struct Tmp {
  std::vector<void*> v;
  template <typename T> T* get(size_t n) { void* p = nullptr; if (hipMalloc(&p, n * sizeof(T) + 256) != hipSuccess) { agd_set_error("tmp alloc failed"); return nullptr; } v.push_back(p); return (T*)p; }
  ~Tmp() { for (void* p : v) hipFree(p); }
};
static bf16_t* op_zero_page() {
  static bf16_t* z = nullptr;
  if (!z) { hipMalloc((void**)&z, 4096); hipMemset(z, 0, 4096); }
  return z;
}

// NCHW fp32 <-> NHWC bf16 (padded) helpers built from the library kernels
static int to_nhwc_bf16(const float* x, bf16_t* y, int B, int C, int HW, int Cpad, hipStream_t st) { return launch_prep_latents(x, y, B, C, HW, Cpad, 1, 1.0f, st); }

AGD_API int agd_op_conv2d_ex(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int H, int W, int Cout,
                                int ksize, int stride, int pad, int upsample, int flags, void* stream);
AGD_API int agd_op_conv2d(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int H, int W, int Cout,
                             int ksize, int stride, int pad, int upsample, void* stream) {
  return agd_op_conv2d_ex(x, w, bias, y, B, Cin, H, W, Cout, ksize, stride, pad, upsample, 0, stream);
}
// flags bit 0: 3x3 stride-1 launches take the row-halo kernel (igemm_halo.h) where it applies; bits 1..3: the 8-phase kernel
// (igemm8p.h) -- 2 = where the launcher would pick it, 4 / 8 = force its 256- / 160-wide tile
AGD_API int agd_op_conv2d_ex(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int H, int W, int Cout,
                                int ksize, int stride, int pad, int upsample, int flags, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (pad != (ksize == 3 ? 1 : 0)) { agd_set_error("op_conv2d: pad must be 1 for 3x3, 0 for 1x1"); return -1; }
  const int Cpad = (Cin + 63) / 64 * 64, taps = ksize * ksize, up = upsample ? 2 : 1;
  const int Ho = (H * up + 2 * pad - ksize) / stride + 1, Wo = (W * up + 2 * pad - ksize) / stride + 1;
  bf16_t* xb = tmp.get<bf16_t>((size_t)B * H * W * Cpad); bf16_t* wb = tmp.get<bf16_t>((size_t)Cout * taps * Cpad);
  float* yn = tmp.get<float>((size_t)B * Ho * Wo * Cout);
  if (!xb || !wb || !yn) return -1;
  CK(to_nhwc_bf16(x, xb, B, Cin, H * W, Cpad, st));
  CK(launch_convert_weight(w, wb, Cout, Cin, taps, Cpad, 0, st));
  WMat wm; wm.w = wb; wm.N = Cout; wm.Cin = Cin; wm.Cpad = Cpad; wm.taps = taps;
  GemmOpt o; o.bias = bias; o.stride = stride; o.up = up; o.out_f32 = 1; o.halo = flags & 1; o.p8 = (flags & 4) ? 2 : (flags & 8) ? 3 : (flags & 2) ? 1 : 0;
  o.smap = (flags & 16) ? 1 : 0;
  o.pc = ((flags >> 7) & 15) | ((flags >> 8) & 48); // the producer / consumer kernels (igemm_pc.h, igemm_pch.h): IgemmP::pc mask bits 0..3 in bits 7..10, bits 4 / 5 in bits 12 / 13
  o.xcd_block = (flags >> 11) & 1;                   // XCD-aware tile blocks (igemm.hip pick_xcd_block)
  if ((flags & 64) && upsample && ksize == 3 && stride == 1) {     // the upsampling conv as four 2x2 phase convs (IgemmP::ups4); bf16 output (that form's only one), widened afterwards
    bf16_t* w4 = tmp.get<bf16_t>((size_t)4 * Cout * 4 * Cpad); float* b4 = tmp.get<float>((size_t)4 * Cout); bf16_t* yb = tmp.get<bf16_t>((size_t)B * Ho * Wo * Cout);
    if (!w4 || !b4 || !yb) return -1;
    CK(launch_upsample_phase_weight(wb, w4, Cout, Cpad, st));
    for (int ph = 0; ph < 4; ++ph) {
      if (bias) { if (hipMemcpyAsync(b4 + (size_t)ph * Cout, bias, Cout * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) { agd_set_error("op_conv2d: bias copy"); return -1; } }
      else if (hipMemsetAsync(b4 + (size_t)ph * Cout, 0, Cout * sizeof(float), st) != hipSuccess) { agd_set_error("op_conv2d: bias clear"); return -1; }
    }
    WMat wm4; wm4.w = w4; wm4.N = 4 * Cout; wm4.Cin = Cin; wm4.Cpad = Cpad; wm4.taps = 4;
    GemmOpt o4; o4.bias = b4; o4.ups4 = Cout; o4.hout = H; o4.wout = W; o4.ldo = Cout; o4.pad = 0; o4.p8 = o.p8;
    CK(run_conv(nullptr, st, xb, Cpad, nullptr, 0, B, H, W, wm4, 2, yb, o4, op_zero_page()));
    CK(launch_bf16_to_f32(yb, yn, (long long)B * Ho * Wo * Cout, st));
  } else
  CK(run_conv(nullptr, st, xb, Cpad, nullptr, 0, B, H, W, wm, ksize, yn, o, op_zero_page()));
  CK(launch_nchw_from_nhwc_f32(yn, Cout, y, B, Cout, Ho * Wo, st));
  hipStreamSynchronize(st);
  return 0;
}

AGD_API int agd_op_linear(const float* x, const float* w, const float* bias, const float* residual, float* y, int M, int K, int N,
                             int geglu, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  const int flags = geglu; geglu &= 1;            // bit 0: GEGLU; bits 1..3: the 8-phase kernel, as in agd_op_conv2d_ex
  if (K % 64) { agd_set_error("op_linear: K must be a multiple of 64"); return -1; }
  const int Nout = geglu ? N / 2 : N;
  bf16_t* xb = tmp.get<bf16_t>((size_t)M * K); bf16_t* wb = tmp.get<bf16_t>((size_t)N * K);
  bf16_t* rb = residual ? tmp.get<bf16_t>((size_t)M * Nout) : nullptr;
  if (!xb || !wb || (residual && !rb)) return -1;
  CK(launch_f32_to_bf16(x, xb, (long long)M * K, st));
  CK(launch_convert_weight(w, wb, N, K, 1, K, geglu ? 16 : 0, st));
  if (residual) CK(launch_f32_to_bf16(residual, rb, (long long)M * Nout, st));
  WMat wm; wm.w = wb; wm.N = N; wm.Cin = K; wm.Cpad = K; wm.taps = 1;
  GemmOpt o; o.bias = bias; o.residual = rb; o.geglu = geglu; o.out_f32 = 1; o.p8 = (flags & 4) ? 2 : (flags & 8) ? 3 : (flags & 2) ? 1 : 0;
  o.kg2 = (flags & 32) ? 1 : 0;                      // two K groups of waves per workgroup where the launcher's 64-row unsplit tiles apply
  o.pc = ((flags >> 7) & 15) | ((flags >> 8) & 48); // the producer / consumer kernel (igemm_pc.h): IgemmP::pc mask bits 0..3 in bits 7..10, bits 4 / 5 in bits 12 / 13
  o.xcd_block = (flags >> 11) & 1;                   // XCD-aware tile blocks (igemm.hip pick_xcd_block)
  if (flags & 16) {                                  // the weight-streaming kernel (igemm_wreg.h); bf16 output (that kernel's only form), widened afterwards
    const int ni = geglu ? 4 : 2;
    if (N % (ni * 64)) { agd_set_error("op_linear: the weight-streaming kernel needs N %% %d == 0", ni * 64); return -1; }
    wm.wfrag = tmp.get<bf16_t>((size_t)N * K); bf16_t* yb = tmp.get<bf16_t>((size_t)M * Nout); if (!wm.wfrag || !yb) return -1;
    CK(launch_frag_order_w(wb, wm.wfrag, N, K, ni, K, st));
    wm.wfrag_ni = ni; o.wreg = (flags & 64) ? 7 : 3; o.out_f32 = 0;
    CK(run_conv(nullptr, st, xb, K, nullptr, 0, 1, 1, M, wm, 1, yb, o, op_zero_page()));
    CK(launch_bf16_to_f32(yb, y, (long long)M * Nout, st));
    hipStreamSynchronize(st);
    return 0;
  }
  CK(run_conv(nullptr, st, xb, K, nullptr, 0, 1, 1, M, wm, 1, y, o, op_zero_page()));
  hipStreamSynchronize(st);
  return 0;
}

// GroupNorm(+SiLU) reaching every form of launch_groupnorm: one source or the channel concat x0 | x1 (x1 null with C1 = 0), and optional
// host-supplied partial-sum tables in the layout igemm's colstat_out leaves ([(b * HW / bm + tile) * Cs + ch] * 2 floats: sum and sum of
// squares of the source's bf16 values over the tile's bm pixels).  *path (may be null): 1 the partial-sum kernel ran, 2 the two-kernel path.
AGD_API int agd_op_groupnorm_ex(const float* x0, const float* x1, const float* gamma, const float* beta, float* y, int B, int C0, int C1, int HW,
                                int groups, float eps, int silu, const float* part0, int bm0, const float* part1, int bm1, int* path, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (path) *path = 0;
  if (groupnorm_check(B, C0, C1, HW, groups)) return -1;
  if (!x0 || !gamma || !beta || !y || (C1 > 0) != (x1 != nullptr)) { agd_set_error("op_groupnorm: null operand, or x1 and C1 = %d disagree", C1); return -1; }
  const int C = C0 + C1;
  const long long wsf = groupnorm_ws_floats(B, C, HW, groups);
  if (wsf < 0) return -1;
  bf16_t* xb0 = tmp.get<bf16_t>((size_t)B * HW * C0); bf16_t* xb1 = C1 ? tmp.get<bf16_t>((size_t)B * HW * C1) : nullptr;
  bf16_t* yb = tmp.get<bf16_t>((size_t)B * HW * C);
  float* ws = tmp.get<float>((size_t)wsf); float* yf = tmp.get<float>((size_t)B * HW * C);
  if (!xb0 || (C1 && !xb1) || !yb || !ws || !yf) return -1;
  CK(to_nhwc_bf16(x0, xb0, B, C0, HW, C0, st));
  if (C1) CK(to_nhwc_bf16(x1, xb1, B, C1, HW, C1, st));
  GroupNormP g{}; g.x0 = xb0; g.x1 = xb1; g.C0 = C0; g.C1 = C1; g.y = yb; g.gamma = gamma; g.beta = beta; g.B = B; g.HW = HW; g.groups = groups; g.eps = eps; g.silu = silu; g.ws = ws;
  g.part0 = part0; g.bm0 = bm0; g.part1 = part1; g.bm1 = bm1; g.path = path;
  CK(launch_groupnorm(g, st));
  CK(launch_bf16_to_f32(yb, yf, (long long)B * HW * C, st));
  CK(launch_nchw_from_nhwc_f32(yf, C, y, B, C, HW, st));
  hipStreamSynchronize(st);
  return 0;
}
AGD_API int agd_op_groupnorm(const float* x, const float* gamma, const float* beta, float* y, int B, int C, int HW, int groups,
                                float eps, int silu, void* stream) {
  return agd_op_groupnorm_ex(x, nullptr, gamma, beta, y, B, C, 0, HW, groups, eps, silu, nullptr, 0, nullptr, 0, nullptr, stream);
}

// GroupNorm folded into the projection behind it (launch_gn_fold_weight), piece by piece: the statistics come from the partial-sum table
// `part` (layout as in agd_op_groupnorm_ex, bm pixels per tile).  wb [B][N][C] and rowadd [B][N]: the row-major fold; with frag_ni > 0 also
// wb_frag = the kernel's fragment-ordered Wb and wb_frag_ref = launch_frag_order_w (NI = frag_ni, KC = C) of each image's row-major Wb, both
// [B][N * C] in storage order; y (may be null, then x may be) [B * HW][N]: the raw activation x (NCHW, rounded to bf16) through the per-image
// matrices plus rowadd, as the transformer's proj_in runs it.  Everything fp32 (bf16 values widened exactly).
AGD_API int agd_op_gn_fold(const float* x, const float* part, int bm, int B, int C, int HW, int groups, float eps, const float* gamma, const float* beta,
                           const float* w, const float* bias, int N, int frag_ni, float* wb, float* rowadd, float* wb_frag, float* wb_frag_ref,
                           float* y, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (groupnorm_check(B, C, 0, HW, groups)) return -1;
  if (N < 1 || N > 65536 || !part || !gamma || !beta || !w || !wb || !rowadd || (frag_ni > 0 && (!wb_frag || !wb_frag_ref)) || (y && !x)) { agd_set_error("op_gn_fold: bad arguments (N %d)", N); return -1; }
  if (y && (C % 64 || HW % 64)) { agd_set_error("op_gn_fold: the projection needs C %% 64 == 0 and HW %% 64 == 0 (C %d HW %d)", C, HW); return -1; }
  const size_t nw = (size_t)B * N * C;
  bf16_t* w16 = tmp.get<bf16_t>((size_t)N * C); bf16_t* wbb = tmp.get<bf16_t>(nw); float* radd = tmp.get<float>((size_t)B * N);
  if (!w16 || !wbb || !radd) return -1;
  CK(launch_convert_weight(w, w16, N, C, 1, C, 0, st));
  CK(launch_gn_fold_weight(part, bm, B, HW, C, groups, eps, gamma, beta, w16, bias, N, wbb, radd, st, 0));
  CK(launch_bf16_to_f32(wbb, wb, (long long)nw, st));
  if (hipMemcpyAsync(rowadd, radd, (size_t)B * N * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) { agd_set_error("op_gn_fold: rowadd copy"); return -1; }
  if (frag_ni > 0) {
    bf16_t* wf = tmp.get<bf16_t>(nw); bf16_t* wr = tmp.get<bf16_t>(nw); float* radd2 = tmp.get<float>((size_t)B * N);
    if (!wf || !wr || !radd2) return -1;
    CK(launch_gn_fold_weight(part, bm, B, HW, C, groups, eps, gamma, beta, w16, bias, N, wf, radd2, st, frag_ni));
    for (int b = 0; b < B; ++b) CK(launch_frag_order_w(wbb + (size_t)b * N * C, wr + (size_t)b * N * C, N, C, frag_ni, C, st));
    CK(launch_bf16_to_f32(wf, wb_frag, (long long)nw, st));
    CK(launch_bf16_to_f32(wr, wb_frag_ref, (long long)nw, st));
  }
  if (y) {
    bf16_t* xb = tmp.get<bf16_t>((size_t)B * HW * C); if (!xb) return -1;
    CK(to_nhwc_bf16(x, xb, B, C, HW, C, st));
    WMat wi; wi.w = wbb; wi.N = N; wi.Cin = C; wi.Cpad = C; wi.taps = 1;
    GemmOpt o; o.rowadd = radd; o.rowadd_ld = N; o.w_per_image = 1; o.out_f32 = 1;
    CK(run_conv(nullptr, st, xb, C, nullptr, 0, B, 1, HW, wi, 1, y, o, op_zero_page()));
  }
  hipStreamSynchronize(st);
  return 0;
}

// conv3x3 (+bias) -> GroupNorm(+SiLU) as the graph walk chains them: with fused != 0 the conv launch leaves per-channel partial
// sums and the GroupNorm skips its statistics pass; with fused == 0 the two-kernel GroupNorm runs on the same conv output.
// y_nchw fp32 [B, Cout, H, W].  (Test entry point for the producer-statistics path.)
AGD_API int agd_op_conv_groupnorm(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, float* y, int B,
                                  int Cin, int H, int W, int Cout, int groups, float eps, int silu, int fused, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (Cin < 1 || H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) { agd_set_error("op_conv_groupnorm: bad shape Cin=%d H=%d W=%d", Cin, H, W); return -1; }
  if (groupnorm_check(B, Cout, 0, H * W, groups)) return -1;
  const int Cpad = (Cin + 63) / 64 * 64, HW = H * W;
  bf16_t* xb = tmp.get<bf16_t>((size_t)B * HW * Cpad); bf16_t* wb = tmp.get<bf16_t>((size_t)Cout * 9 * Cpad);
  bf16_t* hb = tmp.get<bf16_t>((size_t)B * HW * Cout); bf16_t* yb = tmp.get<bf16_t>((size_t)B * HW * Cout);
  float* part = tmp.get<float>((size_t)((long long)B * HW / 64 + 1) * Cout * 2); float* yf = tmp.get<float>((size_t)B * HW * Cout);
  float* ws = tmp.get<float>((size_t)groupnorm_ws_floats(B, Cout, HW, groups));
  if (!xb || !wb || !hb || !yb || !part || !yf || !ws) return -1;
  CK(to_nhwc_bf16(x, xb, B, Cin, HW, Cpad, st));
  CK(launch_convert_weight(w, wb, Cout, Cin, 9, Cpad, 0, st));
  IgemmP p{};
  p.src0 = xb; p.C0 = Cpad; p.Hin = H; p.Win = W; p.Hout = H; p.Wout = W; p.ksize = 3; p.stride = 1; p.pad = 1; p.up = 1;
  p.W = wb; p.bias = bias; p.bias_mode = bias ? 1 : 0; p.N = Cout; p.K = 9 * Cpad; p.M = B * HW; p.ldr = Cout; p.out = hb; p.ldo = Cout;
  p.alpha = 1.f; p.batch = 1; p.zero_page = op_zero_page();
  p.p8 = (fused & 4) ? 2 : (fused & 8) ? 3 : (fused & 2) ? 1 : 0; fused &= 1;      // bits 1..3: the 8-phase kernel, as in agd_op_conv2d_ex
  int bm = 0;
  if (fused) {
    int cfg[3] = {0, 0, 0};
    CK(igemm_query(p, cfg));
    bm = cfg[0];
    if (cfg[2] != 1 || bm < 1 || HW % bm || HW % 64) { agd_set_error("op_conv_groupnorm: shape not eligible for producer statistics (tile %d, splits %d)", cfg[0], cfg[2]); return -1; }
    p.colstat_out = part; p.colstat_rows = HW;
  }
  CK(launch_igemm(p, st));
  GroupNormP g{}; g.x0 = hb; g.C0 = Cout; g.y = yb; g.gamma = gamma; g.beta = beta; g.B = B; g.HW = HW; g.groups = groups; g.eps = eps; g.silu = silu; g.ws = ws;
  if (fused) { g.part0 = part; g.bm0 = bm; }
  CK(launch_groupnorm(g, st));
  CK(launch_bf16_to_f32(yb, yf, (long long)B * HW * Cout, st));
  CK(launch_nchw_from_nhwc_f32(yf, Cout, y, B, Cout, HW, st));
  hipStreamSynchronize(st);
  return 0;
}

// One launch_igemm call stated field by field (include/agenda_hip.h agd_igemm_desc).  (Test entry point: every gather and epilogue form, every
// kernel family, with the family and slab pass that ran reported back.)
static_assert(AGD_IGEMM_GENERAL == IGEMM_RAN_GENERAL && AGD_IGEMM_HALO == IGEMM_RAN_HALO && AGD_IGEMM_PCH == IGEMM_RAN_PCH && AGD_IGEMM_PC == IGEMM_RAN_PC &&
              AGD_IGEMM_8P == IGEMM_RAN_8P && AGD_IGEMM_SMAP == IGEMM_RAN_SMAP && AGD_IGEMM_WREG == IGEMM_RAN_WREG && AGD_IGEMM_SLAB_PLAIN == IGEMM_SLAB_PLAIN &&
              AGD_IGEMM_SLAB_GN == IGEMM_SLAB_GN, "the public family codes restate the launcher's");
AGD_API int agd_op_igemm(agd_igemm_desc* d, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (!d || d->struct_size != (int)sizeof(agd_igemm_desc)) { agd_set_error("op_igemm: descriptor size mismatch"); return -1; }
  d->cfg[0] = d->cfg[1] = d->cfg[2] = 0; d->ran[0] = d->ran[1] = 0; d->gn_fused = 0; d->can_fuse_sc = -1;
  if (d->images < 1 || d->H < 1 || d->W < 1 || d->N < 1 || d->K < 1 || d->stride < 1 || d->up < 1 || d->ksize < 1 || !d->src0 || !d->w || !d->out ||
      d->n_src0 < 1 || d->n_w < 1 || d->n_out < 1 || (d->src1 != nullptr) != (d->n_src1 > 0) || (d->sc0 != nullptr) != (d->n_sc0 > 0) ||
      (d->sc1 != nullptr) != (d->n_sc1 > 0) || (d->residual != nullptr) != (d->n_res > 0)) { agd_set_error("op_igemm: bad descriptor (shape, or a pointer and its element count disagree)"); return -1; }
  const int Hout = d->hout > 0 ? d->hout : (d->H * d->up + 2 * d->pad - d->ksize) / d->stride + 1;
  const int Wout = d->wout > 0 ? d->wout : (d->W * d->up + 2 * d->pad - d->ksize) / d->stride + 1;
  if (Hout < 1 || Wout < 1) { agd_set_error("op_igemm: empty output map"); return -1; }
  {  // every buffer the launch walks must cover what the descriptor says of it
    const long long nb = d->batch > 1 ? d->batch - 1 : 0, px = (long long)d->images * d->H * d->W, M_ = (long long)d->images * Hout * Wout;
    const long long nout = d->geglu ? d->N / 2 : d->N, nkk = (long long)d->N * d->K;
    const long long w_need = d->w_per_image ? (long long)(d->images - 1) * (d->sW ? d->sW : nkk) + nkk : nb * d->sW + nkk;
    if (d->sA0 < 0 || d->sA1 < 0 || d->sW < 0 || d->sO < 0 || d->sR < 0 || d->C0 < 0 || d->C1 < 0 || d->sc_C0 < 0 || d->sc_C1 < 0 || d->ldo < nout || (d->residual && d->ldr < nout) ||
        nb * d->sA0 + px * d->C0 > d->n_src0 || (d->src1 && nb * d->sA1 + px * d->C1 > d->n_src1) || (d->C1 > 0 && !d->src1) ||
        (d->sc0 && M_ * d->sc_C0 > d->n_sc0) || (d->sc1 && M_ * d->sc_C1 > d->n_sc1) || (d->sc_C0 > 0 && !d->sc0) || (d->sc_C1 > 0 && !d->sc1) ||
        w_need > d->n_w || nb * d->sO + (M_ - 1) * d->ldo + nout > d->n_out || (d->residual && nb * d->sR + (M_ - 1) * d->ldr + nout > d->n_res) ||
        (d->gn_y && d->ldo != d->N)) { agd_set_error("op_igemm: a buffer is smaller than the descriptor's shape and strides need"); return -1; }
  }
  auto to_bf = [&](const float* x, long long n) -> bf16_t* {
    if (!x) return nullptr;
    bf16_t* b = tmp.get<bf16_t>((size_t)n);
    if (b && launch_f32_to_bf16(x, b, n, st)) return nullptr;
    return b;
  };
  bf16_t* s0 = to_bf(d->src0, d->n_src0); bf16_t* s1 = to_bf(d->src1, d->n_src1);
  bf16_t* c0 = to_bf(d->sc0, d->n_sc0); bf16_t* c1 = to_bf(d->sc1, d->n_sc1); bf16_t* rb = to_bf(d->residual, d->n_res);
  if (!s0 || (d->src1 && !s1) || (d->sc0 && !c0) || (d->sc1 && !c1) || (d->residual && !rb)) return -1;
  // the matrices: rounded (and, GEGLU, interleaved as the loader interleaves them) one [N][K] matrix at a time
  const long long nk = (long long)d->N * d->K;
  if (d->n_w % nk) { agd_set_error("op_igemm: n_w is not a whole number of [N][K] matrices"); return -1; }
  bf16_t* wb = tmp.get<bf16_t>((size_t)d->n_w); if (!wb) return -1;
  for (long long i = 0; i < d->n_w / nk; ++i) CK(launch_convert_weight(d->w + i * nk, wb + i * nk, d->N, d->K, 1, d->K, d->geglu ? 16 : 0, st));
  bf16_t* ob = nullptr; bf16_t* gb = nullptr;
  if (!d->out_f32) { ob = to_bf(d->out, d->n_out); if (!ob) return -1; }
  const long long n_gn = (long long)d->images * Hout * Wout * d->N;
  if (d->gn_y) { gb = to_bf(d->gn_y, n_gn); if (!gb) return -1; }
  IgemmP p{};
  p.src0 = s0; p.src1 = s1; p.C0 = d->C0; p.C1 = d->C1; p.Hin = d->H; p.Win = d->W; p.Hout = Hout; p.Wout = Wout;
  p.ksize = d->ksize; p.stride = d->stride; p.pad = d->pad; p.up = d->up;
  p.sc0 = c0; p.sc1 = c1; p.sc_C0 = d->sc_C0; p.sc_C1 = d->sc_C1;
  p.W = wb; p.bias = d->bias; p.bias_mode = d->bias_mode; p.rowadd = d->rowadd; p.rowadd_ld = d->rowadd_ld; p.residual = rb; p.ldr = d->ldr;
  p.out = d->out_f32 ? (void*)d->out : (void*)ob; p.out_f32 = d->out_f32; p.ldo = d->ldo;
  p.M = d->images * Hout * Wout; p.N = d->N; p.K = d->K; p.alpha = d->alpha; p.geglu = d->geglu; p.act = d->act;
  p.batch = d->batch > 0 ? d->batch : 1; p.sA0 = d->sA0; p.sA1 = d->sA1; p.sW = d->sW; p.sO = d->sO; p.sR = d->sR;
  p.zero_page = op_zero_page();
  p.w_per_image = d->w_per_image; if (p.w_per_image && !p.sW) p.sW = nk;
  p.rowstat_out = d->rowstat; p.rowstat_slots = d->rowstat_slots;
  p.ln_stats = d->ln_stats; p.ln_slots = d->ln_slots; p.ln_cs = d->ln_cs; p.ln_invC = d->ln_invC; p.ln_eps = d->ln_eps;
  p.colstat_out = d->colstat; p.colstat_rows = d->colstat_rows;
  p.gn_gamma = d->gn_gamma; p.gn_beta = d->gn_beta; p.gn_y = gb; p.gn_groups = d->gn_groups; p.gn_eps = d->gn_eps; p.gn_silu = d->gn_silu;
  p.gn_keep_out = d->gn_keep_out; p.gn_fused = &d->gn_fused;
  p.halo = d->halo; p.p8 = d->p8; p.smap = d->smap; p.pc = d->pc; p.kg2 = d->kg2; p.xcd_block = d->xcd_block;
  if (d->wreg) {      // the fragment-order copy the weight-streaming kernel reads, as agd_op_linear makes it
    const int ni = d->geglu ? 4 : 2;
    if (d->N % (ni * 64) || d->n_w != nk) { agd_set_error("op_igemm: the weight-streaming kernel needs one matrix with N %% %d == 0", ni * 64); return -1; }
    bf16_t* wf = tmp.get<bf16_t>((size_t)nk); if (!wf) return -1;
    CK(launch_frag_order_w(wb, wf, d->N, d->K, ni, d->K, st));
    p.Wfrag = wf; p.wfrag_ni = ni; p.wreg = d->wreg; p.wreg_mmin = 1; p.wreg_mmax = 1 << 30;
  }
  (void)igemm_query(p, d->cfg);                              // (a refused query leaves zeros; the launch below states the reason)
  if (p.sc0) d->can_fuse_sc = igemm_can_fuse_shortcut(p) ? 1 : 0;
  p.ran = d->ran;
  const int rc = launch_igemm(p, st);
  if (rc) { hipStreamSynchronize(st); return rc; }
  if (ob) CK(launch_bf16_to_f32(ob, d->out, d->n_out, st));
  if (gb) CK(launch_bf16_to_f32(gb, d->gn_y, n_gn, st));
  if (hipStreamSynchronize(st) != hipSuccess) { agd_set_error("op_igemm: the launch failed"); return -1; }
  return 0;
}

// *inst (may be null): which layernorm_kernel<LPR, MAXV> ran, as 100 * LPR + MAXV (6404, 1605 or 1610)
AGD_API int agd_op_layernorm_ex(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps, int* inst, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (inst) *inst = 0;
  if (layernorm_check(rows, C)) return -1;
  bf16_t* xb = tmp.get<bf16_t>((size_t)rows * C); bf16_t* yb = tmp.get<bf16_t>((size_t)rows * C);
  if (!xb || !yb) return -1;
  CK(launch_f32_to_bf16(x, xb, (long long)rows * C, st));
  CK(launch_layernorm(xb, yb, gamma, beta, rows, C, eps, st, inst));
  CK(launch_bf16_to_f32(yb, y, (long long)rows * C, st));
  hipStreamSynchronize(st);
  return 0;
}
AGD_API int agd_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps, void* stream) {
  return agd_op_layernorm_ex(x, gamma, beta, y, rows, C, eps, nullptr, stream);
}

// y = x + ff.net.2(GEGLU(ff.net.0(LayerNorm(x)))) through the fused row-panel kernel (tblock.hip); w1 [8C][C] (values then gates),
// b1 [8C], w2 [C][4C], b2 [C], x / y [M][C] fp32 (x is rounded to bf16 first, as the residual stream is stored)
AGD_API int agd_op_ff_fused(const float* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                            const float* b2, float* y, int M, int C, float eps, void* stream) {
  return agd_op_ff_fused_ex(x, gamma, beta, w1, b1, w2, b2, y, M, C, eps, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, stream);
}
// agd_op_ff_fused reaching every form of launch_ff_fused.  wp != null: the proj_out stage -- pout [M][C] = (x + FF(x)) . wp^T + bp + xres, xres
// [xres_rows > 0 ? xres_rows : M][C] (output row m adds row m % xres_rows), y is then not written (may be null); premul: w2 is the caller's
// Wp W2 [C][4C] and bp the caller's Wp b2 + bp (b2 is not read).  colstat (optional, with wp): [ceil(M / 128)][C][2] device floats, left as the
// kernel writes them.  inplace: the launch runs with out == h, as the transformer runs it.
AGD_API int agd_op_ff_fused_ex(const float* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                               const float* b2, float* y, int M, int C, float eps, const float* wp, const float* bp, const float* xres,
                               int xres_rows, float* pout, int premul, float* colstat, int inplace, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (C != 320) { agd_set_error("op_ff_fused: C = %d (320 only)", C); return -1; }
  if (M < 1 || xres_rows < 0 || !x || !gamma || !beta || !w1 || !b1 || !w2 || !b2 || (!wp && !y)) { agd_set_error("op_ff_fused: bad arguments (M %d xres_rows %d)", M, xres_rows); return -1; }
  if (colstat && !wp) { agd_set_error("op_ff_fused: colstat belongs to the proj_out stage"); return -1; }
  const int H8 = 8 * C, H4 = 4 * C;
  const long long xr_rows = xres_rows > 0 ? xres_rows : M;
  bf16_t* xb = tmp.get<bf16_t>((size_t)M * C); bf16_t* yb = tmp.get<bf16_t>((size_t)M * C);
  bf16_t* w1b = tmp.get<bf16_t>((size_t)H8 * C); bf16_t* w1l = tmp.get<bf16_t>((size_t)H8 * C); bf16_t* w1f = tmp.get<bf16_t>((size_t)H8 * C);
  bf16_t* w2b = tmp.get<bf16_t>((size_t)C * H4); bf16_t* w2f = tmp.get<bf16_t>((size_t)C * H4);
  float* cs = tmp.get<float>(H8); float* bf = tmp.get<float>(H8);
  if (!xb || !yb || !w1b || !w1l || !w1f || !w2b || !w2f || !cs || !bf) return -1;
  CK(launch_f32_to_bf16(x, xb, (long long)M * C, st));
  CK(launch_convert_weight(w1, w1b, H8, C, 1, C, 16, st));
  CK(launch_ln_fold_weight(w1b, gamma, beta, b1, H8, C, 16, w1l, cs, bf, st));
  CK(launch_frag_order_w1(w1l, w1f, C, H4, st));
  CK(launch_convert_weight(w2, w2b, C, H4, 1, H4, 0, st));
  CK(launch_frag_order_w(w2b, w2f, C, H4, C / 64, 128, st));
  FFusedP fp{}; fp.h = xb; fp.out = inplace ? xb : yb; fp.w1f = w1f; fp.cs1 = cs; fp.b1 = bf; fp.w2f = w2f; fp.b2 = b2; fp.M = M; fp.ln_eps = eps;
  bf16_t* pb = nullptr;
  fp.premul = premul ? 1 : 0; fp.xres_rows = xres_rows; fp.colstat = colstat; fp.bp = bp;
  if (wp) {
    bf16_t* wpb = tmp.get<bf16_t>((size_t)C * C); bf16_t* wpf = tmp.get<bf16_t>((size_t)C * C); pb = tmp.get<bf16_t>((size_t)M * C);
    if (!wpb || !wpf || !pb) return -1;
    CK(launch_convert_weight(wp, wpb, C, C, 1, C, 0, st));
    CK(launch_frag_order_w(wpb, wpf, C, C, C / 64, C, st));
    fp.wpf = wpf; fp.pout = pout ? pb : nullptr;
    if (xres) {
      bf16_t* xrb = tmp.get<bf16_t>((size_t)xr_rows * C); if (!xrb) return -1;
      CK(launch_f32_to_bf16(xres, xrb, xr_rows * C, st));
      fp.xres = xrb;
    }
  }
  CK(launch_ff_fused(fp, C, st));
  if (wp) CK(launch_bf16_to_f32(pb, pout, (long long)M * C, st));
  else CK(launch_bf16_to_f32(fp.out, y, (long long)M * C, st));
  hipStreamSynchronize(st);
  return 0;
}

// y = x + to_out(attention(to_q(LayerNorm(x)), k, v)) through the fused row-panel kernel (tblock.hip): x / y [B * HW][C] fp32, wq / wo
// [C][C], bo [C], kv [B][T][2C] (projected context: K columns then V columns); probs_sum (optional) [B][T][HW] = probabilities summed
// over the heads (the recorder's head-group form, all images recording)
AGD_API int agd_op_attn_chain(const float* x, const float* gamma, const float* beta, const float* wq, const float* kv, const float* wo,
                              const float* bo, float* y, float* probs_sum, int B, int HW, int T, int C, int heads, float eps, void* stream) {
  hipStream_t st = S(stream);
  const int rows32 = (heads >> 8) & 1; heads &= 255;     // (bit 8 of `heads`: the 32-row panel form of the C = 640 kernel, tests)
  if (probs_sum && B > 0 && T > 0 && HW > 0 && hipMemsetAsync(probs_sum, 0, (size_t)B * T * HW * 4, st) != hipSuccess) { agd_set_error("memset probs"); return -1; }
  return agd_op_attn_chain_ex(x, gamma, beta, wq, kv, wo, bo, y, B, HW, T, C, heads, eps, nullptr, nullptr, nullptr, nullptr, 0, nullptr, probs_sum, 8, 0, T, T,
                              rows32, 0, stream);
}
// agd_op_attn_chain reaching every form of launch_attn_chain.  o1 != null: the prologue h1 = o1 . wo1^T + bo1 + x runs first (o1 has x's rows);
// h1 (optional) receives it -- the kernel overwrites its stored h1 with the final rows, so the entry takes it from a launch of its own with
// to_out's matrix and bias zeroed, whose output is h1 bit for bit (0 + 0 + h1, rounded again to the bf16 value it already is).  src_rows > 0:
// x / o1 hold src_rows rows and output row m reads input row m % src_rows.  rowstat (optional): [B * HW][2] device floats.  rec (optional): the
// recorder rows [B - rec_b0][8 / rec_hpb][rec_rows][HW] device floats, ADDED to as the kernel does (never zeroed here); token rows >= rec_T are
// left alone (rec_T <= rec_rows).  inplace: out == h.
AGD_API int agd_op_attn_chain_ex(const float* x, const float* gamma, const float* beta, const float* wq, const float* kv, const float* wo,
                                 const float* bo, float* y, int B, int HW, int T, int C, int heads, float eps, const float* o1, const float* wo1,
                                 const float* bo1, float* h1, int src_rows, float* rowstat, float* rec, int rec_hpb, int rec_b0, int rec_T,
                                 int rec_rows, int rows32, int inplace, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (C != 320 && C != 640) { agd_set_error("op_attn_chain: C %d", C); return -1; }
  if (B < 1 || HW < 1 || (long long)B * HW >= (1LL << 31) || T < 0 || src_rows < 0 || !x || !gamma || !beta || !wq || !kv || !wo || !bo || !y) { agd_set_error("op_attn_chain: bad arguments (B %d HW %d T %d src_rows %d)", B, HW, T, src_rows); return -1; }
  if (o1 && (!wo1 || !bo1)) { agd_set_error("op_attn_chain: the prologue needs wo1 and bo1"); return -1; }
  if (h1 && !o1) { agd_set_error("op_attn_chain: h1 is the prologue's"); return -1; }
  if (rec && (rec_b0 < 0 || rec_b0 > B || rec_T < 1 || rec_T > rec_rows)) { agd_set_error("op_attn_chain: recorder rows b0 %d T %d of %d", rec_b0, rec_T, rec_rows); return -1; }
  const long long M = (long long)B * HW, Min = src_rows > 0 ? src_rows : M;
  bf16_t* xb = tmp.get<bf16_t>((size_t)Min * C); bf16_t* yb = tmp.get<bf16_t>((size_t)M * C); bf16_t* kvb = tmp.get<bf16_t>((size_t)B * T * 2 * C);
  bf16_t* wqb = tmp.get<bf16_t>((size_t)C * C); bf16_t* wqf = tmp.get<bf16_t>((size_t)C * C);
  bf16_t* wob = tmp.get<bf16_t>((size_t)C * C); bf16_t* wof = tmp.get<bf16_t>((size_t)C * C);
  if (!xb || !yb || !kvb || !wqb || !wqf || !wob || !wof) return -1;
  CK(launch_f32_to_bf16(x, xb, Min * C, st));
  if (T > 0) CK(launch_f32_to_bf16(kv, kvb, (long long)B * T * 2 * C, st));
  CK(launch_convert_weight(wq, wqb, C, C, 1, C, 0, st)); CK(launch_frag_order_w(wqb, wqf, C, C, 5, C, st));
  CK(launch_convert_weight(wo, wob, C, C, 1, C, 0, st)); CK(launch_frag_order_w(wob, wof, C, C, 5, C, st));
  AttnChainP ap{}; ap.h = xb; ap.out = inplace ? xb : yb; ap.gamma = gamma; ap.beta = beta; ap.ln_eps = eps; ap.wqf = wqf; ap.wof = wof; ap.bo = bo;
  ap.rows32 = rows32; ap.src_rows = src_rows;
  ap.kv = kvb; ap.ldkv = 2 * C; ap.skv = (long long)T * 2 * C; ap.M = (int)M; ap.HW = HW; ap.T = T; ap.scale = 1.0f / sqrtf((float)(heads > 0 ? C / heads : C));
  if (o1) {
    bf16_t* o1b = tmp.get<bf16_t>((size_t)Min * C); bf16_t* w1b = tmp.get<bf16_t>((size_t)C * C); bf16_t* w1f = tmp.get<bf16_t>((size_t)C * C);
    if (!o1b || !w1b || !w1f) return -1;
    CK(launch_f32_to_bf16(o1, o1b, Min * C, st));
    CK(launch_convert_weight(wo1, w1b, C, C, 1, C, 0, st)); CK(launch_frag_order_w(w1b, w1f, C, C, 5, C, st));
    ap.o1 = o1b; ap.wo1f = w1f; ap.bo1 = bo1;
  }
  if (h1) {                                              // (nothing recorded, no statistics: the launch below is the one under test)
    bf16_t* zw = tmp.get<bf16_t>((size_t)C * C); float* zb = tmp.get<float>(C); bf16_t* hb = tmp.get<bf16_t>((size_t)M * C);
    if (!zw || !zb || !hb) return -1;
    if (hipMemsetAsync(zw, 0, (size_t)C * C * 2, st) != hipSuccess || hipMemsetAsync(zb, 0, (size_t)C * 4, st) != hipSuccess) { agd_set_error("op_attn_chain: memset"); return -1; }
    AttnChainP a1 = ap; a1.wof = zw; a1.bo = zb; a1.out = inplace ? xb : hb;
    CK(launch_attn_chain(a1, C, heads, st));
    CK(launch_bf16_to_f32(a1.out, h1, M * C, st));
  }
  ap.rowstat_out = rowstat;
  if (rec) {
    const int slices = (rec_hpb >= 1 && rec_hpb <= 8 && 8 % rec_hpb == 0) ? 8 / rec_hpb : 1;       // (any other head group: the launcher refuses)
    ap.record = 1; ap.rec = rec; ap.rec_b0 = rec_b0; ap.rec_T = rec_T; ap.rec_hpb = rec_hpb;
    ap.rec_head_stride = (long long)rec_rows * HW; ap.rec_img_stride = ap.rec_head_stride * slices;
  }
  CK(launch_attn_chain(ap, C, heads, st));
  CK(launch_bf16_to_f32(ap.out, y, M * C, st));
  hipStreamSynchronize(st);
  return 0;
}

// The block head as ONE launch (tblock.hip launch_qkv_chain): GroupNorm -> proj_in -> h -> norm1 -> q | k | v.  x [M][C] = the raw rows of M / HW images
// (NHWC), part = the caller's partial-sum table of those rows (layout as agd_op_groupnorm_ex, bm pixels per tile), w_in [C][C] + b_in, wqkv [3C][C]
// (q rows, k rows, v rows); h [M][C], qkv [M][3C].  flags bit 0: the GroupNorm is applied inside the kernel (the plain proj_in matrix in fragment
// order); clear: it is folded into per-image matrices by launch_gn_fold_weight, written in the chain's fragment order (column ranges of 80: NI = 5
// whatever C).  bit 1: rows64, bit 2: sched2.
AGD_API int agd_op_qkv_chain(const float* x, const float* gn_gamma, const float* gn_beta, int groups, float gn_eps, const float* part, int bm,
                             const float* w_in, const float* b_in, const float* gamma, const float* beta, float ln_eps, const float* wqkv, float* h,
                             float* qkv, int M, int HW, int C, int flags, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (M < 1 || HW < 1 || groups < 1 || bm < 1 || C < 64 || C > 1280 || C % 64) { agd_set_error("op_qkv_chain: bad shape (M %d HW %d C %d groups %d bm %d)", M, HW, C, groups, bm); return -1; }
  if (!x || !gn_gamma || !gn_beta || !part || !w_in || !b_in || !gamma || !beta || !wqkv || !h || !qkv) { agd_set_error("op_qkv_chain: bad arguments"); return -1; }
  const int B = M / HW > 0 ? M / HW : 1;
  const size_t MC = (size_t)M * C;
  bf16_t* xb = tmp.get<bf16_t>(MC); bf16_t* hb = tmp.get<bf16_t>(MC); bf16_t* qb = tmp.get<bf16_t>(3 * MC);
  bf16_t* wib = tmp.get<bf16_t>((size_t)C * C); bf16_t* wqb = tmp.get<bf16_t>((size_t)3 * C * C); bf16_t* wqf = tmp.get<bf16_t>((size_t)3 * C * C);
  if (!xb || !hb || !qb || !wib || !wqb || !wqf) return -1;
  CK(launch_f32_to_bf16(x, xb, (long long)MC, st));
  CK(launch_convert_weight(w_in, wib, C, C, 1, C, 0, st));
  CK(launch_convert_weight(wqkv, wqb, 3 * C, C, 1, C, 0, st));
  QkvChainP qp{}; qp.x = xb; qp.h = hb; qp.qkv = qb; qp.gamma = gamma; qp.beta = beta; qp.ln_eps = ln_eps; qp.M = M; qp.HW = HW;
  qp.rows64 = (flags >> 1) & 1; qp.sched2 = (flags >> 2) & 1;
  if (C != 320 && C != 640) return launch_qkv_chain(qp, C, st);                          // (refused there, by name; the re-layouts below need C % 80 == 0)
  CK(launch_frag_order_w(wqb, wqf, 3 * C, C, 5, C, st));
  qp.wqkvf = wqf;
  if (flags & 1) {
    bf16_t* wif = tmp.get<bf16_t>((size_t)C * C); if (!wif) return -1;
    CK(launch_frag_order_w(wib, wif, C, C, 5, C, st));
    qp.wbf = wif; qp.wb_stride = 0; qp.rowadd = b_in; qp.rowadd_stride = 0;
    qp.gn_part = part; qp.gn_bm = bm; qp.gn_groups = groups; qp.gn_eps = gn_eps; qp.gn_gamma = gn_gamma; qp.gn_beta = gn_beta;
  } else {
    bf16_t* wb = tmp.get<bf16_t>((size_t)B * C * C); float* radd = tmp.get<float>((size_t)B * C); if (!wb || !radd) return -1;
    CK(launch_gn_fold_weight(part, bm, B, HW, C, groups, gn_eps, gn_gamma, gn_beta, wib, b_in, C, wb, radd, st, 5));
    qp.wbf = wb; qp.wb_stride = (long long)C * C; qp.rowadd = radd; qp.rowadd_stride = C;
  }
  CK(launch_qkv_chain(qp, C, st));
  CK(launch_bf16_to_f32(hb, h, (long long)MC, st));
  CK(launch_bf16_to_f32(qb, qkv, (long long)(3 * MC), st));
  hipStreamSynchronize(st);
  return 0;
}

// x + to_out(attention(to_q(LayerNorm(x)), k, v)) through the pre-multiplied form (xattn_pre.hip): x [B][HW][C] fp32, wq / wo [C][C], bo [C], kv [B][T][2C];
// probs (optional) [B][heads][T][HW] = every head's probabilities (the recorder's per-(image, head) rows, all images recording)
AGD_API int agd_op_xattn_premul(const float* x, const float* gamma, const float* beta, const float* wq, const float* kv, const float* wo,
                                const float* bo, float* y, float* probs, int B, int HW, int T, int C, int heads, float eps, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  const long long M = (long long)B * HW;
  if (heads < 1 || C % heads || (C / heads) % 8 || C % 160 || C % 64 || HW % 64 || T < 1 || T > XATTN_TP || (heads * XATTN_TP) % 64) { agd_set_error("op_xattn_premul: C %d heads %d HW %d T %d", C, heads, HW, T); return -1; }
  const size_t HT = (size_t)heads * XATTN_TP;
  bf16_t* xb = tmp.get<bf16_t>((size_t)M * C); bf16_t* yb = tmp.get<bf16_t>((size_t)M * C); bf16_t* kvb = tmp.get<bf16_t>((size_t)B * T * 2 * C);
  bf16_t* wqb = tmp.get<bf16_t>((size_t)C * C); bf16_t* wqT = tmp.get<bf16_t>((size_t)C * C); bf16_t* wob = tmp.get<bf16_t>((size_t)C * C);
  float* wqbeta = tmp.get<float>(C); float* rst = tmp.get<float>((size_t)M * 2);
  bf16_t* kpp = tmp.get<bf16_t>((size_t)B * HT * C); bf16_t* vpp = tmp.get<bf16_t>((size_t)B * HT * C); float* kcs = tmp.get<float>((size_t)B * HT * 2);
  bf16_t* P = tmp.get<bf16_t>((size_t)M * HT);
  if (!xb || !yb || !kvb || !wqb || !wqT || !wob || !wqbeta || !rst || !kpp || !vpp || !kcs || !P) return -1;
  CK(launch_f32_to_bf16(x, xb, M * C, st));
  CK(launch_f32_to_bf16(kv, kvb, (long long)B * T * 2 * C, st));
  CK(launch_convert_weight(wq, wqb, C, C, 1, C, 0, st)); CK(launch_transpose_bf16(wqb, C, C, wqT, st));
  CK(launch_convert_weight(wo, wob, C, C, 1, C, 0, st));
  CK(launch_matvec_bf16(wqb, beta, wqbeta, C, C, st));
  CK(launch_rowstat_bf16(xb, rst, (int)M, C, st));
  XattnPremulP pm{}; pm.kv = kvb; pm.ldkv = 2 * C; pm.skv = (long long)T * 2 * C; pm.wqT = wqT; pm.wo = wob; pm.gamma = gamma; pm.wqb = wqbeta;
  pm.B = B; pm.T = T; pm.C = C; pm.H = heads; pm.scale = 1.0f / sqrtf((float)(C / heads)); pm.kpp = kpp; pm.kcs = kcs; pm.kbs = kcs + (size_t)B * HT; pm.vpp = vpp;
  CK(launch_xattn_premul(pm, st));
  XattnSP sp{}; sp.x = xb; sp.ln_stats = rst; sp.ln_slots = 1; sp.ln_invC = 1.0f / (float)C; sp.ln_eps = eps; sp.kpp = kpp; sp.kcs = pm.kcs; sp.kbs = pm.kbs; sp.P = P;
  sp.M = (int)M; sp.HW = HW; sp.C = C; sp.H = heads; sp.T = T;
  if (probs) {
    if (hipMemsetAsync(probs, 0, (size_t)B * heads * T * HW * 4, st) != hipSuccess) { agd_set_error("memset probs"); return -1; }
    sp.rec = probs; sp.rec_b0 = 0; sp.rec_T = T; sp.rec_head_stride = (long long)T * HW; sp.rec_img_stride = sp.rec_head_stride * heads;
  }
  CK(launch_xattn_s(sp, st));
  WMat wv; wv.w = vpp; wv.N = C; wv.Cin = (int)HT; wv.Cpad = (int)HT; wv.taps = 1;
  GemmOpt oo; oo.bias = bo; oo.residual = xb; oo.w_per_image = 1;
  CK(run_conv(nullptr, st, P, (int)HT, nullptr, 0, B, 1, HW, wv, 1, yb, oo, op_zero_page()));
  CK(launch_bf16_to_f32(yb, y, M * C, st));
  hipStreamSynchronize(st);
  return 0;
}

// The stages of agd_op_xattn_premul and of the IP-Adapter branch (ipadapter.hip) one at a time (tests/test_premul_ops_gpu.py).  Context-free; fp32 in
// and out, bf16 quantities rounded / widened by launch_f32_to_bf16 / launch_bf16_to_f32; every output buffer the kernels write into is first filled
// with the byte 0x7F (bf16 0x7F7F, fp32 0x7F7F7F7F: huge finite values), so an element a kernel leaves out shows.  What a launcher refuses
// comes back as -1 with its message.
static size_t opn(long long n) { return n > 0 ? (size_t)n : 0; }
static int op_fill(void* p, size_t bytes, hipStream_t st) {
  if (bytes && hipMemsetAsync(p, 0x7F, bytes, st) != hipSuccess) { agd_set_error("op: memset failed"); return -1; }
  return 0;
}
// the context products exactly as agd_op_xattn_premul builds them: kv [B][T][2C], wq / wo [C][C] -> kpp [B][heads][80][C], cs / bs [B][heads][80],
// vpp [B][C][heads][80], the padding included
AGD_API int agd_op_xattn_context(const float* kv, const float* wq, const float* wo, const float* gamma, const float* beta, float* kpp, float* cs,
                                 float* bs, float* vpp, int B, int T, int C, int heads, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (!kv || !wq || !wo || !gamma || !beta || !kpp || !cs || !bs || !vpp || B < 1 || T < 1 || C < 1 || heads < 1) { agd_set_error("op_xattn_context: bad arguments (B %d T %d C %d heads %d)", B, T, C, heads); return -1; }
  const size_t HT = (size_t)heads * XATTN_TP, CC = (size_t)C * C;
  bf16_t* kvb = tmp.get<bf16_t>((size_t)B * T * 2 * C); bf16_t* wqb = tmp.get<bf16_t>(CC); bf16_t* wqT = tmp.get<bf16_t>(CC); bf16_t* wob = tmp.get<bf16_t>(CC);
  float* wqbeta = tmp.get<float>(C); bf16_t* kb = tmp.get<bf16_t>((size_t)B * HT * C); bf16_t* vb = tmp.get<bf16_t>((size_t)B * HT * C);
  if (!kvb || !wqb || !wqT || !wob || !wqbeta || !kb || !vb) return -1;
  CK(launch_f32_to_bf16(kv, kvb, (long long)B * T * 2 * C, st));
  CK(launch_convert_weight(wq, wqb, C, C, 1, C, 0, st)); CK(launch_transpose_bf16(wqb, C, C, wqT, st));
  CK(launch_convert_weight(wo, wob, C, C, 1, C, 0, st));
  CK(launch_matvec_bf16(wqb, beta, wqbeta, C, C, st));
  CK(op_fill(kb, (size_t)B * HT * C * 2, st)); CK(op_fill(vb, (size_t)B * HT * C * 2, st)); CK(op_fill(cs, (size_t)B * HT * 4, st)); CK(op_fill(bs, (size_t)B * HT * 4, st));
  XattnPremulP pm{}; pm.kv = kvb; pm.ldkv = 2 * C; pm.skv = (long long)T * 2 * C; pm.wqT = wqT; pm.wo = wob; pm.gamma = gamma; pm.wqb = wqbeta;
  pm.B = B; pm.T = T; pm.C = C; pm.H = heads; pm.scale = 1.0f / sqrtf((float)(C / heads > 0 ? C / heads : 1)); pm.kpp = kb; pm.kcs = cs; pm.kbs = bs; pm.vpp = vb;
  CK(launch_xattn_premul(pm, st));
  CK(launch_bf16_to_f32(kb, kpp, (long long)B * HT * C, st));
  CK(launch_bf16_to_f32(vb, vpp, (long long)B * HT * C, st));
  hipStreamSynchronize(st);
  return 0;
}
// launch_xattn_s alone on the caller's K'' / cs / bs: x [B * HW][C], stats (optional) [B * HW][slots][2] = the row's (sum, sum of squares) in slots
// partial sums (NULL: one slot from launch_rowstat_bf16), kpp [B][heads][80][C], cs / bs [B][heads][80] -> P [B * HW][heads * 80].  rec (optional):
// [B - rec_b0][heads][rec_rows][HW] device floats the launch ADDS to (never zeroed here): images >= rec_b0, token rows < rec_T <= rec_rows.
AGD_API int agd_op_xattn_scores(const float* x, const float* stats, int slots, const float* kpp, const float* cs, const float* bs, float* P, float* rec,
                                int rec_b0, int rec_T, int rec_rows, int B, int HW, int T, int C, int heads, float eps, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (!x || !kpp || !cs || !bs || !P || B < 1 || HW < 1 || C < 1 || heads < 1 || (stats && slots < 1)) { agd_set_error("op_xattn_scores: bad arguments (B %d HW %d C %d heads %d slots %d)", B, HW, C, heads, slots); return -1; }
  if (rec && (rec_b0 < 0 || rec_b0 >= B || rec_T < 1 || rec_T > rec_rows || rec_T > XATTN_TP)) { agd_set_error("op_xattn_scores: recorder rows b0 %d T %d of %d", rec_b0, rec_T, rec_rows); return -1; }
  const long long M = (long long)B * HW; const size_t HT = (size_t)heads * XATTN_TP;
  if (M >= (1LL << 31)) { agd_set_error("op_xattn_scores: %lld rows", M); return -1; }
  bf16_t* xb = tmp.get<bf16_t>((size_t)M * C); bf16_t* kb = tmp.get<bf16_t>((size_t)B * HT * C); bf16_t* Pb = tmp.get<bf16_t>((size_t)M * HT);
  float* rst = stats ? nullptr : tmp.get<float>((size_t)M * 2);
  if (!xb || !kb || !Pb || (!stats && !rst)) return -1;
  CK(launch_f32_to_bf16(x, xb, M * C, st));
  CK(launch_f32_to_bf16(kpp, kb, (long long)B * HT * C, st));
  if (!stats) CK(launch_rowstat_bf16(xb, rst, (int)M, C, st));
  CK(op_fill(Pb, (size_t)M * HT * 2, st));
  XattnSP sp{}; sp.x = xb; sp.ln_stats = stats ? stats : rst; sp.ln_slots = stats ? slots : 1; sp.ln_invC = 1.0f / (float)C; sp.ln_eps = eps;
  sp.kpp = kb; sp.kcs = cs; sp.kbs = bs; sp.P = Pb; sp.M = (int)M; sp.HW = HW; sp.C = C; sp.H = heads; sp.T = T;
  if (rec) { sp.rec = rec; sp.rec_b0 = rec_b0; sp.rec_T = rec_T; sp.rec_head_stride = (long long)rec_rows * HW; sp.rec_img_stride = sp.rec_head_stride * heads; }
  CK(launch_xattn_s(sp, st));
  CK(launch_bf16_to_f32(Pb, P, M * (long long)HT, st));
  hipStreamSynchronize(st);
  return 0;
}
// launch_ipa_linear: y [R][N] = x [R][K] . bf16(w [N][K])^T (+ bias [N], optional)
AGD_API int agd_op_ipa_linear(const float* x, const float* w, const float* bias, float* y, int R, int N, int K, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (!x || !w || !y) { agd_set_error("op_ipa_linear: bad arguments"); return -1; }
  bf16_t* wb = tmp.get<bf16_t>(opn((long long)N * K)); if (!wb) return -1;
  CK(launch_f32_to_bf16(w, wb, (long long)opn((long long)N * K), st));
  CK(op_fill(y, opn((long long)R * N) * 4, st));
  CK(launch_ipa_linear(x, wb, bias, y, R, N, K, st));
  hipStreamSynchronize(st);
  return 0;
}
// launch_ipa_layernorm on a copy of x [rows][C] -> y
AGD_API int agd_op_ipa_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps, void* stream) {
  hipStream_t st = S(stream);
  if (!x || !gamma || !beta || !y) { agd_set_error("op_ipa_layernorm: bad arguments"); return -1; }
  const size_t bytes = opn((long long)rows * C) * 4;
  if (bytes && hipMemcpyAsync(y, x, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) { agd_set_error("op_ipa_layernorm: copy failed"); return -1; }
  CK(launch_ipa_layernorm(y, gamma, beta, rows, C, eps, st));
  hipStreamSynchronize(st);
  return 0;
}
// the Wq . beta mat-vec and launch_ipa_premul as agd_ip_adapter_set runs them: kip / vip [B][nt][C] fp32, wq / wo [C][C] -> kpp [B][colsP][C],
// cs / bs [B][colsP], vpp [B][C][colsP]
AGD_API int agd_op_ipa_context(const float* kip, const float* vip, const float* wq, const float* wo, const float* gamma, const float* beta, float* kpp,
                               float* cs, float* bs, float* vpp, int B, int C, int heads, int nt, int colsP, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (!kip || !vip || !wq || !wo || !gamma || !beta || !kpp || !cs || !bs || !vpp || B < 1 || C < 1 || heads < 1 || nt < 1 || colsP < 1) { agd_set_error("op_ipa_context: bad arguments (B %d C %d heads %d tokens %d cols %d)", B, C, heads, nt, colsP); return -1; }
  const size_t CC = (size_t)C * C, n = (size_t)B * colsP * C;
  bf16_t* wqb = tmp.get<bf16_t>(CC); bf16_t* wob = tmp.get<bf16_t>(CC); float* wqbeta = tmp.get<float>(C); bf16_t* kb = tmp.get<bf16_t>(n); bf16_t* vb = tmp.get<bf16_t>(n);
  if (!wqb || !wob || !wqbeta || !kb || !vb) return -1;
  CK(launch_convert_weight(wq, wqb, C, C, 1, C, 0, st)); CK(launch_convert_weight(wo, wob, C, C, 1, C, 0, st));
  CK(launch_matvec_bf16(wqb, beta, wqbeta, C, C, st));
  CK(op_fill(kb, n * 2, st)); CK(op_fill(vb, n * 2, st)); CK(op_fill(cs, (size_t)B * colsP * 4, st)); CK(op_fill(bs, (size_t)B * colsP * 4, st));
  IpaPremulP pm{}; pm.kip = kip; pm.vip = vip; pm.wq = wqb; pm.wo = wob; pm.gamma = gamma; pm.wqb = wqbeta;
  pm.B = B; pm.C = C; pm.H = heads; pm.nt = nt; pm.colsP = colsP; pm.scale = 1.0f / sqrtf((float)(C / heads > 0 ? C / heads : 1));
  pm.kpp = kb; pm.cs = cs; pm.bs = bs; pm.vpp = vb;
  CK(launch_ipa_premul(pm, st));
  CK(launch_bf16_to_f32(kb, kpp, (long long)n, st));
  CK(launch_bf16_to_f32(vb, vpp, (long long)n, st));
  hipStreamSynchronize(st);
  return 0;
}
// launch_ipa_scores: h [B * HW][C], kpp [B][colsP][C], cs / bs [B][colsP] -> P.  P is the CALLER's [B * HW + guard_rows][colsP] floats (bf16 values):
// rounded to bf16, handed to the kernel and widened back whole, so rows the kernel must not touch come back as they went in
AGD_API int agd_op_ipa_scores(const float* h, const float* kpp, const float* cs, const float* bs, float* P, int B, int HW, int C, int heads, int nt,
                              int colsP, float eps, int guard_rows, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (!h || !kpp || !cs || !bs || !P || B < 1 || HW < 1 || C < 1 || colsP < 1 || guard_rows < 0) { agd_set_error("op_ipa_scores: bad arguments (B %d HW %d C %d cols %d)", B, HW, C, colsP); return -1; }
  const long long M = (long long)B * HW, np = (M + guard_rows) * colsP;
  bf16_t* hb = tmp.get<bf16_t>((size_t)M * C); bf16_t* kb = tmp.get<bf16_t>((size_t)B * colsP * C); bf16_t* Pb = tmp.get<bf16_t>((size_t)np);
  if (!hb || !kb || !Pb) return -1;
  CK(launch_f32_to_bf16(h, hb, M * C, st)); CK(launch_f32_to_bf16(kpp, kb, (long long)B * colsP * C, st)); CK(launch_f32_to_bf16(P, Pb, np, st));
  IpaScoreP sp{}; sp.h = hb; sp.kpp = kb; sp.cs = cs; sp.bs = bs; sp.P = Pb; sp.B = B; sp.HW = HW; sp.C = C; sp.H = heads; sp.nt = nt; sp.colsP = colsP; sp.eps = eps;
  CK(launch_ipa_scores(sp, st));
  CK(launch_bf16_to_f32(Pb, P, np, st));
  hipStreamSynchronize(st);
  return 0;
}
// launch_ipa_add: h += s P V''^T.  h is the CALLER's [B * HW + guard_rows][C] floats, updated in place through bf16 as above; P [B * HW][colsP],
// vpp [B][C][colsP]
AGD_API int agd_op_ipa_add(float* h, const float* P, const float* vpp, int B, int HW, int C, int colsP, float s, int guard_rows, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (!h || !P || !vpp || B < 1 || HW < 1 || C < 1 || colsP < 1 || guard_rows < 0) { agd_set_error("op_ipa_add: bad arguments (B %d HW %d C %d cols %d)", B, HW, C, colsP); return -1; }
  const long long M = (long long)B * HW, nh = (M + guard_rows) * C;
  bf16_t* hb = tmp.get<bf16_t>((size_t)nh); bf16_t* Pb = tmp.get<bf16_t>((size_t)M * colsP); bf16_t* vb = tmp.get<bf16_t>((size_t)B * C * colsP);
  if (!hb || !Pb || !vb) return -1;
  CK(launch_f32_to_bf16(h, hb, nh, st)); CK(launch_f32_to_bf16(P, Pb, M * colsP, st)); CK(launch_f32_to_bf16(vpp, vb, (long long)B * C * colsP, st));
  IpaAddP ap{}; ap.h = hb; ap.P = Pb; ap.vpp = vb; ap.B = B; ap.HW = HW; ap.C = C; ap.colsP = colsP; ap.s = s;
  CK(launch_ipa_add(ap, st));
  CK(launch_bf16_to_f32(hb, h, nh, st));
  hipStreamSynchronize(st);
  return 0;
}

AGD_API int agd_op_attention(const float* q, const float* k, const float* v, float* o, int B, int H, int D, int Nq, int Nk,
                                float scale, float* probs_out, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  const int C = H * D;
  bf16_t* qb = tmp.get<bf16_t>((size_t)B * Nq * C); bf16_t* kb = tmp.get<bf16_t>((size_t)B * Nk * C);
  bf16_t* vb = tmp.get<bf16_t>((size_t)B * Nk * C); bf16_t* ob = tmp.get<bf16_t>((size_t)B * Nq * C);
  if (!qb || !kb || !vb || !ob) return -1;
  CK(launch_f32_to_bf16(q, qb, (long long)B * Nq * C, st));
  CK(launch_f32_to_bf16(k, kb, (long long)B * Nk * C, st));
  CK(launch_f32_to_bf16(v, vb, (long long)B * Nk * C, st));
  AttnP a{}; a.q = qb; a.k = kb; a.v = vb; a.o = ob; a.ldq = a.ldk = a.ldv = a.ldo = C;
  a.sq = (long long)Nq * C; a.so = a.sq; a.sk = (long long)Nk * C; a.sv = a.sk;
  a.B = B; a.H = H; a.D = D; a.Nq = Nq; a.Nk = Nk; a.scale = scale;
  if (probs_out) {
    if (hipMemsetAsync(probs_out, 0, (size_t)B * H * Nk * Nq * 4, st) != hipSuccess) { agd_set_error("memset probs"); return -1; }
    a.record_mode = 1; a.rec_b0 = 0; a.rec = probs_out; a.rec_T = Nk;
    a.rec_head_stride = (long long)Nk * Nq; a.rec_img_stride = a.rec_head_stride * H;
  }
  CK(launch_attention(a, st));
  CK(launch_bf16_to_f32(ob, o, (long long)B * Nq * C, st));
  hipStreamSynchronize(st);
  return 0;
}

// Every instantiation of attention.hip's attn_kernel through one context-free entry (tests/test_attention_ops_gpu.py).  q [B][Nq][H*D],
// k / v [B][Nk][H*D], mask [B][Nk] (additive, or NULL), k2 / v2 [B][Nk2][H*D] (the second K/V source, or both NULL): packed fp32, rounded to
// bf16 here.  layout: how the bf16 operands lie in memory when the kernel reads them --
//   0  packed: q, k, v (and k2, v2) each [.][H*D], pitch C
//   1  q | k | v are the column blocks of ONE [B][N][3C] buffer (pitch 3C, batch stride N * 3C; needs Nq == Nk) -- UNet / CLIP self-attention
//   2  k | v are the column blocks of ONE [B][Nk][2C] buffer (pitch 2C) -- cross-attention; q packed
//   (layouts 1 and 2 keep the second source as the k2 | v2 column blocks of one [B][Nk2][2C] buffer, as GLIGEN's fuser does)
// record: 0 = none; 1 = every head's probabilities, probs_out [B][H][Nk][Nq]; 2 = their sum over the heads, probs_out [B][Nk][Nq].  probs_out
// is zeroed here; batch rows >= rec_b0 and token rows < rec_T are then recorded, every other row stays zero.
// Every refusal of this entry comes before any allocation or launch; the launcher's own (mask + causal, a second source with a mask, causal
// order or recording, Nk2 outside 1..64, head-summed recording with a mask) come back as errors before its launch.  Syncs.
AGD_API int agd_op_attention_ex(const float* q, const float* k, const float* v, float* o, int B, int H, int D, int Nq, int Nk, float scale,
                                int causal, const float* mask, const float* k2, const float* v2, int Nk2, int layout, float* probs_out,
                                int record, int rec_b0, int rec_T, void* stream) {
  if (D != 32 && D != 40 && D != 64 && D != 80 && D != 128 && D != 160) { agd_set_error("attention_ex: unsupported head dim D=%d", D); return -1; }
  if (B < 1 || H < 1 || Nq < 1 || Nk < 1) { agd_set_error("attention_ex: bad shape B=%d H=%d Nq=%d Nk=%d", B, H, Nq, Nk); return -1; }
  if (!q || !k || !v || !o) { agd_set_error("attention_ex: q, k, v and o are required"); return -1; }
  if (layout < 0 || layout > 2) { agd_set_error("attention_ex: layout=%d (0 packed, 1 fused q|k|v rows, 2 fused k|v rows)", layout); return -1; }
  if (layout == 1 && Nq != Nk) { agd_set_error("attention_ex: layout=1 (fused q|k|v rows) needs Nq == Nk (got Nq=%d Nk=%d)", Nq, Nk); return -1; }
  if (record < 0 || record > 2 || (record != 0) != (probs_out != nullptr)) { agd_set_error("attention_ex: record=%d needs probs_out, and probs_out needs record 1 or 2", record); return -1; }
  if (record && Nk > 96) { agd_set_error("attention_ex: recording needs Nk <= 96 (got Nk=%d)", Nk); return -1; }
  if (record && (rec_b0 < 0 || rec_b0 > B)) { agd_set_error("attention_ex: rec_b0=%d outside [0, %d]", rec_b0, B); return -1; }
  if (record && (rec_T < 1 || rec_T > Nk)) { agd_set_error("attention_ex: rec_T=%d outside [1, %d]", rec_T, Nk); return -1; }
  if ((k2 != nullptr) != (v2 != nullptr)) { agd_set_error("attention_ex: k2 and v2 come together"); return -1; }
  if (!k2 && Nk2 != 0) { agd_set_error("attention_ex: Nk2=%d without a second source", Nk2); return -1; }
  hipStream_t st = S(stream); Tmp tmp;
  const int C = H * D;
  const long long nq = (long long)B * Nq * C, nk = (long long)B * Nk * C, nk2 = k2 ? (long long)B * (Nk2 > 0 ? Nk2 : 0) * C : 0;
  bf16_t* qb = tmp.get<bf16_t>((size_t)nq); bf16_t* kb = tmp.get<bf16_t>((size_t)nk); bf16_t* vb = tmp.get<bf16_t>((size_t)nk);
  bf16_t* ob = tmp.get<bf16_t>((size_t)nq);
  bf16_t* k2b = k2 ? tmp.get<bf16_t>((size_t)nk2 + 8) : nullptr; bf16_t* v2b = k2 ? tmp.get<bf16_t>((size_t)nk2 + 8) : nullptr;
  bf16_t* fused = layout ? tmp.get<bf16_t>((size_t)(layout == 1 ? 3 : 2) * nk) : nullptr;
  bf16_t* fused2 = (layout && k2) ? tmp.get<bf16_t>((size_t)2 * nk2 + 8) : nullptr;
  if (!qb || !kb || !vb || !ob || (k2 && (!k2b || !v2b)) || (layout && !fused) || (layout && k2 && !fused2)) return -1;
  CK(launch_f32_to_bf16(q, qb, nq, st));
  CK(launch_f32_to_bf16(k, kb, nk, st));
  CK(launch_f32_to_bf16(v, vb, nk, st));
  if (nk2 > 0) { CK(launch_f32_to_bf16(k2, k2b, nk2, st)); CK(launch_f32_to_bf16(v2, v2b, nk2, st)); }
  // column block `col` of a [rows][wide * C] buffer <- packed [rows][C]
  auto place = [&](bf16_t* dst, int wide, int col, const bf16_t* src, long long rows) {
    if (rows < 1) return 0;
    if (hipMemcpy2DAsync(dst + (size_t)col * C, (size_t)wide * C * 2, src, (size_t)C * 2, (size_t)C * 2, (size_t)rows, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      agd_set_error("attention_ex: layout copy failed"); return -1; }
    return 0;
  };
  AttnP a{}; a.q = qb; a.k = kb; a.v = vb; a.o = ob; a.ldq = a.ldk = a.ldv = a.ldo = C;
  a.sq = (long long)Nq * C; a.so = a.sq; a.sk = (long long)Nk * C; a.sv = a.sk;
  if (layout == 1) {
    CK(place(fused, 3, 0, qb, (long long)B * Nq)); CK(place(fused, 3, 1, kb, (long long)B * Nk)); CK(place(fused, 3, 2, vb, (long long)B * Nk));
    a.q = fused; a.k = fused + C; a.v = fused + 2 * C; a.ldq = a.ldk = a.ldv = 3 * C; a.sq = a.sk = a.sv = (long long)Nk * 3 * C;
  } else if (layout == 2) {
    CK(place(fused, 2, 0, kb, (long long)B * Nk)); CK(place(fused, 2, 1, vb, (long long)B * Nk));
    a.k = fused; a.v = fused + C; a.ldk = a.ldv = 2 * C; a.sk = a.sv = (long long)Nk * 2 * C;
  }
  a.B = B; a.H = H; a.D = D; a.Nq = Nq; a.Nk = Nk; a.scale = scale; a.causal = causal ? 1 : 0; a.mask = mask;
  if (k2) {
    a.k2 = k2b; a.v2 = v2b; a.ldk2 = a.ldv2 = C; a.sk2 = a.sv2 = (long long)Nk2 * C; a.Nk2 = Nk2;
    if (layout) {
      CK(place(fused2, 2, 0, k2b, (long long)B * Nk2)); CK(place(fused2, 2, 1, v2b, (long long)B * Nk2));
      a.k2 = fused2; a.v2 = fused2 + C; a.ldk2 = a.ldv2 = 2 * C; a.sk2 = a.sv2 = (long long)Nk2 * 2 * C;
    }
  }
  if (record) {
    const long long rows = (record == 1 ? (long long)B * H : (long long)B) * Nk * Nq;
    if (hipMemsetAsync(probs_out, 0, (size_t)rows * 4, st) != hipSuccess) { agd_set_error("memset probs"); return -1; }
    a.record_mode = record == 1 ? 1 : 3; a.rec_hpb = record == 1 ? 0 : H; a.rec_b0 = rec_b0; a.rec_T = rec_T;
    a.rec_head_stride = (long long)Nk * Nq; a.rec_img_stride = record == 1 ? a.rec_head_stride * H : a.rec_head_stride;
    a.rec = probs_out + (long long)rec_b0 * a.rec_img_stride;      // the kernel indexes the recording rows from rec_b0
  }
  CK(launch_attention(a, st));
  CK(launch_bf16_to_f32(ob, o, nq, st));
  hipStreamSynchronize(st);
  return 0;
}

// attention_long.hip alone (tests/test_attention_long_gpu.py): per-head recording at 97 .. AGD_MAX_CONTEXT_TOKENS keys.  Operands as
// agd_op_attention_ex (packed fp32, rounded to bf16 here); layout 0 packed, 2 = k | v as the column blocks of one [B][Nk][2C] buffer, as the
// engine's projected context lies.  probs_inout [B][H][Nk][Nq] is ADDED to (the caller zeroes it, or launches twice for 2 p): batch rows
// >= rec_b0 and token rows < rec_T only.  Every refusal comes before any allocation or launch.  Syncs.
AGD_API int agd_op_attention_long(const float* q, const float* k, const float* v, float* o, int B, int H, int D, int Nq, int Nk, float scale,
                                  int layout, float* probs_inout, int rec_b0, int rec_T, void* stream) {
  if (D != 32 && D != 40 && D != 64 && D != 80 && D != 128 && D != 160) { agd_set_error("attention_long: unsupported head dim D=%d", D); return -1; }
  if (Nk <= 96 || Nk > AGD_MAX_CONTEXT_TOKENS) { agd_set_error("attention_long: Nk=%d keys outside [97, %d]", Nk, AGD_MAX_CONTEXT_TOKENS); return -1; }
  if (B < 1 || H < 1 || Nq < 1) { agd_set_error("attention_long: bad shape B=%d H=%d Nq=%d Nk=%d", B, H, Nq, Nk); return -1; }
  if (!q || !k || !v || !o || !probs_inout) { agd_set_error("attention_long: q, k, v, o and probs_inout are required"); return -1; }
  if (layout != 0 && layout != 2) { agd_set_error("attention_long: layout=%d (0 packed, 2 fused k|v rows)", layout); return -1; }
  if (rec_b0 < 0 || rec_b0 > B) { agd_set_error("attention_long: rec_b0=%d outside [0, %d]", rec_b0, B); return -1; }
  if (rec_T < 1 || rec_T > Nk) { agd_set_error("attention_long: rec_T=%d outside [1, %d]", rec_T, Nk); return -1; }
  hipStream_t st = S(stream); Tmp tmp;
  const int C = H * D;
  const long long nq = (long long)B * Nq * C, nk = (long long)B * Nk * C;
  bf16_t* qb = tmp.get<bf16_t>((size_t)nq); bf16_t* kb = tmp.get<bf16_t>((size_t)nk); bf16_t* vb = tmp.get<bf16_t>((size_t)nk);
  bf16_t* ob = tmp.get<bf16_t>((size_t)nq);
  bf16_t* fused = layout ? tmp.get<bf16_t>((size_t)2 * nk) : nullptr;
  if (!qb || !kb || !vb || !ob || (layout && !fused)) return -1;
  CK(launch_f32_to_bf16(q, qb, nq, st));
  CK(launch_f32_to_bf16(k, kb, nk, st));
  CK(launch_f32_to_bf16(v, vb, nk, st));
  AttnP a{}; a.q = qb; a.k = kb; a.v = vb; a.o = ob; a.ldq = a.ldk = a.ldv = a.ldo = C;
  a.sq = (long long)Nq * C; a.so = a.sq; a.sk = (long long)Nk * C; a.sv = a.sk;
  if (layout == 2) {
    for (int col = 0; col < 2; ++col)
      if (hipMemcpy2DAsync(fused + (size_t)col * C, (size_t)2 * C * 2, col ? vb : kb, (size_t)C * 2, (size_t)C * 2, (size_t)B * Nk, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        agd_set_error("attention_long: layout copy failed"); return -1; }
    a.k = fused; a.v = fused + C; a.ldk = a.ldv = 2 * C; a.sk = a.sv = (long long)Nk * 2 * C;
  }
  a.B = B; a.H = H; a.D = D; a.Nq = Nq; a.Nk = Nk; a.scale = scale;
  a.record_mode = 1; a.rec_b0 = rec_b0; a.rec_T = rec_T;
  a.rec_head_stride = (long long)Nk * Nq; a.rec_img_stride = a.rec_head_stride * H;
  a.rec = probs_inout + (long long)rec_b0 * a.rec_img_stride;      // the kernel indexes the recording rows from rec_b0
  CK(launch_attention_long(a, st));
  CK(launch_bf16_to_f32(ob, o, nq, st));
  hipStreamSynchronize(st);
  return 0;
}

// as agd_op_attention with the probabilities summed over the heads: probs_sum_out [B][Nk][Nq] (attention.hip RECORD 2)
AGD_API int agd_op_attention_headsum(const float* q, const float* k, const float* v, float* o, int B, int H, int D, int Nq, int Nk,
                                     float scale, float* probs_sum_out, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  const int C = H * D;
  if (!probs_sum_out) { agd_set_error("attention_headsum: probs_sum_out is required"); return -1; }
  bf16_t* qb = tmp.get<bf16_t>((size_t)B * Nq * C); bf16_t* kb = tmp.get<bf16_t>((size_t)B * Nk * C);
  bf16_t* vb = tmp.get<bf16_t>((size_t)B * Nk * C); bf16_t* ob = tmp.get<bf16_t>((size_t)B * Nq * C);
  if (!qb || !kb || !vb || !ob) return -1;
  CK(launch_f32_to_bf16(q, qb, (long long)B * Nq * C, st));
  CK(launch_f32_to_bf16(k, kb, (long long)B * Nk * C, st));
  CK(launch_f32_to_bf16(v, vb, (long long)B * Nk * C, st));
  AttnP a{}; a.q = qb; a.k = kb; a.v = vb; a.o = ob; a.ldq = a.ldk = a.ldv = a.ldo = C;
  a.sq = (long long)Nq * C; a.so = a.sq; a.sk = (long long)Nk * C; a.sv = a.sk;
  a.B = B; a.H = H; a.D = D; a.Nq = Nq; a.Nk = Nk; a.scale = scale;
  if (hipMemsetAsync(probs_sum_out, 0, (size_t)B * Nk * Nq * 4, st) != hipSuccess) { agd_set_error("memset probs"); return -1; }
  a.record_mode = 3; a.rec_hpb = H; a.rec_b0 = 0; a.rec = probs_sum_out; a.rec_T = Nk; a.rec_img_stride = (long long)Nk * Nq;
  CK(launch_attention(a, st));
  CK(launch_bf16_to_f32(ob, o, (long long)B * Nq * C, st));
  hipStreamSynchronize(st);
  return 0;
}

// train.hip's attention backward in isolation: q [B][N][H*D], kv [B][T][2*H*D] (K columns then V columns), d_o [B][N][H*D] (gradient of the
// per-head attention output, BEFORE to_out; may be NULL), d_map [B - b0][T][N] (gradient of the head-mean map of batch rows >= b0; may be
// NULL) -> dq [B][N][H*D], dkv [B][T][2*H*D].  Operands rounded to bf16, fp32 arithmetic, bf16 results returned as fp32.
AGD_API int agd_op_attention_backward(const float* q, const float* kv, const float* d_o, const float* d_map, int b0, int B, int H, int D, int N,
                                      int T, float scale, float* dq, float* dkv, void* stream) {
  // every refusal comes before any allocation or launch (the shapes first: an empty tensor arrives as a null pointer)
  if (D != 32 && D != 40 && D != 64 && D != 80 && D != 128 && D != 160) { agd_set_error("attention_backward: unsupported head dim D=%d", D); return -1; }
  if (T < 1 || T > 96) { agd_set_error("attention_backward: T=%d keys unsupported (1..96)", T); return -1; }
  if (B < 1 || H < 1 || N < 1) { agd_set_error("attention_backward: bad shape B=%d H=%d N=%d", B, H, N); return -1; }
  if (b0 < 0 || b0 > B) { agd_set_error("attention_backward: b0=%d outside [0, %d]", b0, B); return -1; }
  if (!q || !kv || !dq || !dkv) { agd_set_error("attention_backward: q, kv, dq and dkv are required"); return -1; }
  if (!d_o && !d_map) { agd_set_error("attention_backward: d_o and d_map are both null (no gradient to propagate)"); return -1; }
  hipStream_t st = S(stream); Tmp tmp;
  const int C = H * D;
  const long long nq = (long long)B * N * C, nkv = (long long)B * T * 2 * C;
  bf16_t* qb = tmp.get<bf16_t>((size_t)nq); bf16_t* kvb = tmp.get<bf16_t>((size_t)nkv);
  bf16_t* dob = d_o ? tmp.get<bf16_t>((size_t)nq) : nullptr;
  bf16_t* dqb = tmp.get<bf16_t>((size_t)nq); bf16_t* dkvb = tmp.get<bf16_t>((size_t)nkv);
  float* part = tmp.get<float>((size_t)attention_backward_ws_floats(B, H, D, N, T));
  if (!qb || !kvb || (d_o && !dob) || !dqb || !dkvb || !part) return -1;
  CK(launch_f32_to_bf16(q, qb, nq, st));
  CK(launch_f32_to_bf16(kv, kvb, nkv, st));
  if (d_o) CK(launch_f32_to_bf16(d_o, dob, nq, st));
  CK(launch_attention_backward(qb, kvb, dob, d_map, b0, B, H, D, N, T, scale, dqb, dkvb, part, st));
  CK(launch_bf16_to_f32(dqb, dq, nq, st));
  CK(launch_bf16_to_f32(dkvb, dkv, nkv, st));
  hipStreamSynchronize(st);
  return 0;
}

// hook.py:55 in isolation: heads [Bp][H][T][N] fp32 -> map [Bp][T][N] = the mean over the heads, summed in head order
AGD_API int agd_op_hook_headmean(const float* heads, int Bp, int H, int T, int N, float* map, void* stream) {
  if (!heads || !map || Bp < 1 || H < 1 || T < 1 || N < 1) { agd_set_error("hook_headmean: bad argument Bp=%d H=%d T=%d N=%d", Bp, H, T, N); return -1; }
  hipStream_t st = S(stream);
  CK(launch_hook_headmean(heads, Bp, H, T, N, map, st));
  hipStreamSynchronize(st);
  return 0;
}

AGD_API int agd_op_bicubic_clamp_mean(const float* maps, int n_maps, int T, int side, int S_, float* out, void* stream) {
  hipStream_t st = S(stream);
  // n_maps accumulators of [T][side][side]: treat as one layer with n_maps "heads"
  HeatLayer h; h.acc = maps; h.h = h.w = side; h.heads = n_maps; h.head_stride = (long long)T * side * side; h.img_stride = 0;
  CK(launch_daam_global(&h, 1, n_maps, T, S_, S_, 0, out, st));
  hipStreamSynchronize(st);
  return 0;
}

// panorama.hip in isolation: canvas [B][C][Lh][Lw] -> views [v0, v0 + n) of every panorama as [B * n][C][win][win] (view-major within a
// panorama), and views [B * V][C][win][win] -> canvas as the overlap mean (sum in ascending view order / number of covering views)
AGD_API int agd_op_window_gather(const float* canvas, float* views, int B, int C, int Lh, int Lw, int window, int stride, int v0, int n, void* stream) {
  int nbh = 0, nbw = 0;
  if (pano_view_grid(Lh, Lw, window, stride, &nbh, &nbw)) return -1;
  if (!canvas || !views) { agd_set_error("op_window_gather: null argument"); return -1; }
  return launch_window_gather(canvas, views, B, C, Lh, Lw, window, stride, v0, n, n, 1, S(stream));
}
AGD_API int agd_op_window_mean(const float* views, float* canvas, int B, int C, int Lh, int Lw, int window, int stride, void* stream) {
  int nbh = 0, nbw = 0;
  if (pano_view_grid(Lh, Lw, window, stride, &nbh, &nbw)) return -1;
  if (!canvas || !views) { agd_set_error("op_window_mean: null argument"); return -1; }
  return launch_window_mean(views, canvas, B, C, Lh, Lw, window, stride, (long long)nbh * nbw, 1, S(stream));
}
// regions.hip in isolation (include/agenda_hip.h states the layouts); idx is a host array of R - 1 indices, NULL = a step that is not bootstrapped
AGD_API int agd_op_region_masks(const void* px, int px_f32, int per_image, float* masks, int R, int B, int H, int W, int Lh, int Lw, void* stream) {
  return launch_region_masks(px, px_f32, per_image, masks, R, B, H, W, Lh, Lw, S(stream));
}
AGD_API int agd_op_region_spread(const float* canvas, float* x, const float* masks, const float* noise, const float* bgs, int R, int B, int C, int Lh,
                                 int Lw, int n_bg, const int* idx, float sa, float sb, void* stream) {
  if (Lh < 1 || Lw < 1 || R < 1 || R > AGD_MAX_REGIONS) { agd_set_error("op_region_spread: %d regions (1 .. %d) at latent size %d x %d", R, AGD_MAX_REGIONS, Lh, Lw); return -1; }
  RegionIdx ri = {};
  if (idx) for (int r = 1; r < R; ++r) ri.v[r] = idx[r - 1];
  return launch_region_spread(canvas, x, masks, noise, bgs, R, B, C, (long long)Lh * Lw, n_bg, idx != nullptr, ri, sa, sb, S(stream));
}
AGD_API int agd_op_region_mean(const float* x, const float* masks, float* canvas, int R, int B, int C, int Lh, int Lw, void* stream) {
  if (Lh < 1 || Lw < 1) { agd_set_error("op_region_mean: latent size %d x %d", Lh, Lw); return -1; }
  return launch_region_mean(x, masks, canvas, R, B, C, (long long)Lh * Lw, S(stream));
}

#ifdef AGD_EXPERIMENTS   // the micro-benchmark entry points exist only in the experiments library (make exp): tools/kb*.py
// ---------------------------------------------------------------------------------------
// kernel micro-benchmarks (random bf16 operands; HIP-event timing on the launch stream)
// ---------------------------------------------------------------------------------------
__global__ void fill_random_bf16(bf16_t* p, long long n, unsigned seed, float scale) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u ^ seed; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    p[i] = f2bf(((float)(h & 0xFFFF) / 32768.0f - 1.0f) * scale);
  }
}
static void fill_rand(bf16_t* p, long long n, unsigned seed, float scale) {
  hipLaunchKernelGGL(fill_random_bf16, dim3(4096), dim3(256), 0, 0, p, n, seed, scale);
}

AGD_API int agd_bench_conv(int B, int H, int W, int C0, int C1, int Cout, int ksize, int stride, int up, int geglu,
                              int with_residual, int iters, double* ms_out) {
  Tmp tmp;
  const int Ctot = C0 + C1, taps = ksize * ksize, pad = ksize == 3 ? 1 : 0;
  const int Ho = (H * up + 2 * pad - ksize) / stride + 1, Wo = (W * up + 2 * pad - ksize) / stride + 1;
  const long long M = (long long)B * Ho * Wo;
  const int Nout = (geglu & 1) ? Cout / 2 : Cout;
  bf16_t* x0 = tmp.get<bf16_t>((size_t)B * H * W * C0); bf16_t* x1 = C1 ? tmp.get<bf16_t>((size_t)B * H * W * C1) : nullptr;
  bf16_t* w = tmp.get<bf16_t>((size_t)Cout * taps * Ctot); bf16_t* y = tmp.get<bf16_t>((size_t)M * Nout);
  bf16_t* r = with_residual ? tmp.get<bf16_t>((size_t)M * Nout) : nullptr;
  float* bias = tmp.get<float>(Cout);
  if (!x0 || !w || !y || !bias || (C1 && !x1) || (with_residual && !r)) return -1;
  fill_rand(x0, (long long)B * H * W * C0, 1, 1.0f); if (x1) fill_rand(x1, (long long)B * H * W * C1, 2, 1.0f);
  fill_rand(w, (long long)Cout * taps * Ctot, 3, 0.05f); if (r) fill_rand(r, M * Nout, 4, 1.0f);
  hipMemset(bias, 0, Cout * 4);
  WMat wm; wm.w = w; wm.N = Cout; wm.Cin = Ctot; wm.Cpad = Ctot; wm.taps = taps;
  // geglu bit 1 = GEGLU; bit 2 = also emit LayerNorm row statistics (producer); bit 4 = LayerNorm-folded consumer epilogue
  const int mode = geglu; geglu &= 1;
  GemmOpt o; o.bias = bias; o.stride = stride; o.up = up; o.geglu = geglu; o.residual = r; o.halo = (mode & 8) ? 1 : 0;
  o.p8 = (mode & 32) ? 2 : (mode & 64) ? 3 : (mode & 16) ? 1 : 0;
  o.smap = (mode & 256) ? 1 : 0;
  o.kg2 = (mode & 512) ? 1 : 0;
  o.pc = ((mode >> 11) & 15) | ((mode >> 12) & 48);  // producer / consumer kernels (igemm_pc.h, igemm_pch.h): IgemmP::pc mask bits 0..3 in bits 11..14, bit 4 in bit 16
  o.xcd_block = (mode >> 15) & 1;                    // XCD-aware tile blocks
  if (mode & 128) {                                  // weight-streaming kernel (igemm_wreg.h): the matrix once more in fragment order
    const int ni = geglu ? 4 : 2;
    wm.wfrag = tmp.get<bf16_t>((size_t)Cout * taps * Ctot); if (!wm.wfrag) return -1;
    if (taps != 1 || C1) { agd_set_error("bench: wreg is for plain 1x1 launches"); return -1; }
    CK(launch_frag_order_w(w, wm.wfrag, Cout, Ctot, ni, Ctot, 0));
    wm.wfrag_ni = ni; o.wreg = (mode & 1024) ? 7 : 3;
  }
  float* stats = nullptr; float* cs = nullptr;
  if (mode & 6) {
    int cfg[3] = {0, 0, 0}; GemmOpt qo = o; qo.query_cfg = cfg; qo.want_rowstat = (mode & 2) ? 1 : 0;
    CK(run_conv(nullptr, 0, x0, C0, x1, C1, B, H, W, wm, ksize, y, qo, op_zero_page()));
    const int slots = (mode & 2) ? (Cout + cfg[1] - 1) / cfg[1] : 2;
    stats = tmp.get<float>((size_t)M * slots * 2); cs = tmp.get<float>(Cout);
    if (!stats || !cs) return -1;
    hipMemset(stats, 0, (size_t)M * slots * 2 * 4); hipMemset(cs, 0, Cout * 4);
    if (mode & 2) { o.rowstat_out = stats; o.rowstat_slots = slots; }
    if (mode & 4) { o.ln_stats = stats; o.ln_slots = slots; o.ln_cs = cs; o.ln_invC = 1.0f / Ctot; o.ln_eps = 1e-5f; }
  }
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  for (int i = 0; i < 2; ++i) CK(run_conv(nullptr, 0, x0, C0, x1, C1, B, H, W, wm, ksize, y, o, op_zero_page()));
  hipEventRecord(a, 0);
  for (int i = 0; i < iters; ++i) CK(run_conv(nullptr, 0, x0, C0, x1, C1, B, H, W, wm, ksize, y, o, op_zero_page()));
  hipEventRecord(b, 0); hipEventSynchronize(b);
  float t = 0; hipEventElapsedTime(&t, a, b);
  *ms_out = t / iters;
  hipEventDestroy(a); hipEventDestroy(b);
  return 0;
}

// One 1x1 / 3x3 launch with COLD weights, as inside the UNet walk (1.7 GB of weights per forward against 256 MB of Infinity Cache):
// every iteration first overwrites a 1 GiB scratch (evicts L2 + Infinity Cache), rewrites the activation (hot, as after its
// producer), then times [optional streaming touch of the weight matrix] + the launch.  warm: 0 = cold weights, 1 = touch then launch
// (both timed), 2 = weights left hot (no flush of them: the touch runs untimed).  ms_out = mean of the timed regions.
AGD_API int agd_bench_conv_cold(int B, int H, int W, int C0, int Cout, int ksize, int geglu, int with_residual, int warm, int iters, double* ms_out) {
  Tmp tmp;
  const int taps = ksize * ksize;
  const long long M = (long long)B * H * W;
  const int Nout = geglu ? Cout / 2 : Cout;
  const size_t xn = (size_t)M * C0, wn = (size_t)Cout * taps * C0, flush_bytes = (size_t)1 << 30;
  bf16_t* x0 = tmp.get<bf16_t>(xn); bf16_t* xs = tmp.get<bf16_t>(xn); bf16_t* w = tmp.get<bf16_t>(wn); bf16_t* y = tmp.get<bf16_t>((size_t)M * Nout);
  bf16_t* r = with_residual ? tmp.get<bf16_t>((size_t)M * Nout) : nullptr;
  float* bias = tmp.get<float>(Cout); char* scratch = tmp.get<char>(flush_bytes); unsigned* sink = tmp.get<unsigned>(64);
  if (!x0 || !xs || !w || !y || !bias || !scratch || !sink || (with_residual && !r)) return -1;
  fill_rand(xs, (long long)xn, 1, 1.0f); fill_rand(w, (long long)wn, 3, 0.05f); if (r) fill_rand(r, M * Nout, 4, 1.0f);
  hipMemset(bias, 0, Cout * 4);
  WMat wm; wm.w = w; wm.N = Cout; wm.Cin = C0; wm.Cpad = C0; wm.taps = taps;
  GemmOpt o; o.bias = bias; o.geglu = geglu; o.residual = r; o.warm = warm == 3 ? 3 : 0;      // warm 3: cold weights, in-kernel warm-up
  o.halo = 1; o.p8 = 1; o.smap = 1;                                                             // the walk's dispatch options (ctx defaults)
  // the intervening layer (warm >= 4): conv3x3 640 -> 640 on 8 x 32 x 32
  bf16_t* ix = tmp.get<bf16_t>((size_t)8 * 1024 * 640); bf16_t* iy = tmp.get<bf16_t>((size_t)8 * 1024 * 640); bf16_t* iw = tmp.get<bf16_t>((size_t)640 * 9 * 640);
  if (!ix || !iy || !iw) return -1;
  fill_rand(ix, (long long)8 * 1024 * 640, 11, 1.0f); fill_rand(iw, (long long)640 * 9 * 640, 12, 0.05f);
  WMat iwm; iwm.w = iw; iwm.N = 640; iwm.Cin = 640; iwm.Cpad = 640; iwm.taps = 9;
  GemmOpt io; io.bias = bias;
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  double tot = 0;
  for (int i = 0; i < iters + 1; ++i) {
    hipMemsetAsync(scratch, i, flush_bytes, 0);
    hipMemcpyAsync(x0, xs, xn * 2, hipMemcpyDeviceToDevice, 0);
    if (r) hipMemcpyAsync(y, r, (size_t)M * Nout * 2, hipMemcpyDeviceToDevice, 0);       // touches the residual / output lines
    if (warm == 2 || warm >= 4) hipLaunchKernelGGL(touch_kernel, dim3(1024), dim3(256), 0, 0, (const u32x4*)w, (long long)(wn * 2 / 16), sink);
    // warm 4 / 5 / 6: the touch is followed by 1 / 2 / 4 intervening launches of a typical layer (an L1 3x3 conv: ~100 MB through the
    // caches each) before the timed launch: does the Infinity Cache still hold the matrix?
    for (int k = 0; k < (warm == 4 ? 1 : warm == 5 ? 2 : warm == 6 ? 4 : 0); ++k) CK(run_conv(nullptr, 0, ix, 640, nullptr, 0, 8, 32, 32, iwm, 3, iy, io, op_zero_page()));
    hipEventRecord(a, 0);
    if (warm == 1) hipLaunchKernelGGL(touch_kernel, dim3(1024), dim3(256), 0, 0, (const u32x4*)w, (long long)(wn * 2 / 16), sink);
    CK(run_conv(nullptr, 0, x0, C0, nullptr, 0, B, H, W, wm, ksize, y, o, op_zero_page()));
    hipEventRecord(b, 0); hipEventSynchronize(b);
    float t = 0; hipEventElapsedTime(&t, a, b);
    if (i > 0) tot += t;
  }
  *ms_out = tot / iters;
  hipEventDestroy(a); hipEventDestroy(b);
  return 0;
}

// fused row-panel kernels (tblock.hip) at C = 320: kind 0 = feed-forward, 1 = attn2 chain (B images of HW tokens, 77 keys, the upper half of the
// images recording head-summed probabilities, as in a CFG forward)
AGD_API int agd_bench_tblock(int kind, int B, int HW, int iters, double* ms_out) {
  Tmp tmp;
  const int C = (kind == 4 || kind == 5) ? 640 : 320, T = 77; const long long M = (long long)B * HW;      // kind 4 / 5: the attn2 chain at C = 640 (plain / from attn1.to_out)
  if (kind == 4 || kind == 5) kind = kind == 4 ? 1 : 3;
  bf16_t* h = tmp.get<bf16_t>((size_t)M * C); bf16_t* o = tmp.get<bf16_t>((size_t)M * C);
  bf16_t* w1 = tmp.get<bf16_t>((size_t)8 * C * C); bf16_t* w1f = tmp.get<bf16_t>((size_t)8 * C * C);
  bf16_t* w2 = tmp.get<bf16_t>((size_t)4 * C * C); bf16_t* w2f = tmp.get<bf16_t>((size_t)4 * C * C);
  bf16_t* kv = tmp.get<bf16_t>((size_t)B * T * 2 * C);
  const int rslices = C == 640 ? 8 : 1;                 // recorder slices per image: per-head rows below latent resolution, one head-summed slice at it
  float* vec = tmp.get<float>((size_t)16 * C + 64); float* rec = tmp.get<float>((size_t)B * rslices * T * HW);
  if (!h || !o || !w1 || !w1f || !w2 || !w2f || !kv || !vec || !rec) return -1;
  fill_rand(h, M * C, 1, 1.0f); fill_rand(w1, 8LL * C * C, 2, 0.05f); fill_rand(w2, 4LL * C * C, 3, 0.03f); fill_rand(kv, (long long)B * T * 2 * C, 4, 1.0f);
  hipMemset(vec, 0, ((size_t)16 * C + 64) * 4); hipMemset(rec, 0, (size_t)B * rslices * T * HW * 4);
  FFusedP fp{}; AttnChainP ap{};
  if (kind == 0) {
    CK(launch_frag_order_w1(w1, w1f, C, 4 * C, 0)); CK(launch_frag_order_w(w2, w2f, C, 4 * C, C / 64, 128, 0));
    fp.h = h; fp.out = o; fp.w1f = w1f; fp.cs1 = vec; fp.b1 = vec + 8 * C; fp.w2f = w2f; fp.b2 = vec; fp.M = (int)M; fp.ln_eps = 1e-5f;
  } else {
    CK(launch_frag_order_w(w1, w1f, C, C, 5, C, 0)); CK(launch_frag_order_w(w2, w2f, C, C, 5, C, 0));
    ap.h = h; ap.out = o; ap.gamma = vec; ap.beta = vec; ap.ln_eps = 1e-5f; ap.wqf = w1f; ap.wof = w2f; ap.bo = vec; ap.kv = kv; ap.ldkv = 2 * C; ap.skv = (long long)T * 2 * C;
    ap.M = (int)M; ap.HW = HW; ap.T = T; ap.scale = 1.0f / sqrtf((float)(C / 8));
    ap.record = 1; ap.rec = rec; ap.rec_b0 = B / 2; ap.rec_T = T; ap.rec_hpb = 8 / rslices; ap.rec_head_stride = (long long)T * HW; ap.rec_img_stride = (long long)rslices * T * HW;
  }
  bf16_t* o2 = nullptr; float* cst = nullptr;
  if (kind == 2) {                                   // feed-forward + proj_out stage (+ column statistics)
    o2 = tmp.get<bf16_t>((size_t)M * C); cst = tmp.get<float>((size_t)(M / 128 + 1) * C * 2); if (!o2 || !cst) return -1;
    bf16_t* wpf = tmp.get<bf16_t>((size_t)C * C); if (!wpf) return -1;
    CK(launch_frag_order_w(w2, wpf, C, C, C / 64, C, 0));          // (any matrix will do)
    CK(launch_frag_order_w1(w1, w1f, C, 4 * C, 0)); CK(launch_frag_order_w(w2, w2f, C, 4 * C, C / 64, 128, 0));
    fp.h = h; fp.out = o; fp.w1f = w1f; fp.cs1 = vec; fp.b1 = vec + 8 * C; fp.w2f = w2f; fp.b2 = vec; fp.M = (int)M; fp.ln_eps = 1e-5f;
    fp.wpf = wpf; fp.bp = vec; fp.xres = o2; fp.pout = o; fp.colstat = cst;
  }
  if (kind == 3) {                                   // attn2 chain starting at attn1.to_out
    o2 = tmp.get<bf16_t>((size_t)M * C); bf16_t* wo1f = tmp.get<bf16_t>((size_t)C * C); if (!o2 || !wo1f) return -1;
    fill_rand(o2, M * C, 9, 1.0f);
    CK(launch_frag_order_w(w2, wo1f, C, C, 5, C, 0));
    ap.o1 = o2; ap.wo1f = wo1f; ap.bo1 = vec;
  }
  QkvChainP qp{};
  const bool qkvk = kind >= 6 && kind <= 9;            // (8 / 9: the same on round 6's schedule) the block head (GroupNorm inside -> proj_in -> norm1 -> q / k / v); 7: two co-resident 64-row workgroups per CU
  if (qkvk) {
    bf16_t* qkv = tmp.get<bf16_t>((size_t)M * 3 * C); float* part = tmp.get<float>((size_t)B * (HW / 128) * C * 2); float* gv = tmp.get<float>((size_t)4 * C);
    if (!qkv || !part || !gv) return -1;
    hipMemset(part, 0x3C, (size_t)B * (HW / 128) * C * 2 * 4); hipMemset(gv, 0x3C, (size_t)4 * C * 4);    // 0x3C3C3C3C = 0.0115f: finite, non-zero everywhere
    CK(launch_frag_order_w(w2, w2f, C, C, 5, C, 0)); CK(launch_frag_order_w(w1, w1f, 3 * C, C, 5, C, 0));
    qp.x = h; qp.wbf = w2f; qp.wb_stride = 0; qp.rowadd = gv; qp.rowadd_stride = 0; qp.h = o; qp.gamma = gv + C; qp.beta = gv + 2 * C; qp.ln_eps = 1e-5f;
    qp.wqkvf = w1f; qp.qkv = qkv; qp.M = (int)M; qp.HW = HW; qp.rows64 = kind == 7 || kind == 9; qp.sched2 = kind >= 8;
    qp.gn_part = part; qp.gn_bm = 128; qp.gn_groups = 32; qp.gn_eps = 1e-6f; qp.gn_gamma = gv + 3 * C; qp.gn_beta = gv;
  }
  auto run = [&]() { return qkvk ? launch_qkv_chain(qp, C, 0) : (kind == 0 || kind == 2) ? launch_ff_fused(fp, C, 0) : launch_attn_chain(ap, C, 8, 0); };
  hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
  for (int i = 0; i < 2; ++i) CK(run());
  hipEventRecord(a, 0);
  for (int i = 0; i < iters; ++i) CK(run());
  hipEventRecord(b, 0); hipEventSynchronize(b);
  float t = 0; hipEventElapsedTime(&t, a, b);
  *ms_out = t / iters;
  hipEventDestroy(a); hipEventDestroy(b);
  return 0;
}

AGD_API int agd_bench_attention(int B, int H, int D, int Nq, int Nk, int record, int iters, double* ms_out) {
  Tmp tmp;
  const int C = H * D;
  const bool self = (Nq == Nk);
  // self: packed qkv rows [3C]; cross: q [C], kv [2C]
  bf16_t* q = tmp.get<bf16_t>((size_t)B * Nq * (self ? 3 * C : C)); bf16_t* kv = self ? nullptr : tmp.get<bf16_t>((size_t)B * Nk * 2 * C);
  bf16_t* o = tmp.get<bf16_t>((size_t)B * Nq * C);
  float* rec = record ? tmp.get<float>((size_t)B * H * Nk * Nq) : nullptr;     // record: 1 per-head rows, 2 head-summed rows
  if (!q || !o || (!self && !kv) || (record && !rec)) return -1;
  fill_rand(q, (long long)B * Nq * (self ? 3 * C : C), 5, 1.0f); if (kv) fill_rand(kv, (long long)B * Nk * 2 * C, 6, 1.0f);
  if (rec) hipMemset(rec, 0, (size_t)B * H * Nk * Nq * 4);
  AttnP a{};
  if (self) { a.q = q; a.k = q + C; a.v = q + 2 * C; a.ldq = a.ldk = a.ldv = 3 * C; a.sq = a.sk = a.sv = (long long)Nq * 3 * C; }
  else { a.q = q; a.k = kv; a.v = kv + C; a.ldq = C; a.ldk = a.ldv = 2 * C; a.sq = (long long)Nq * C; a.sk = a.sv = (long long)Nk * 2 * C; }
  a.o = o; a.ldo = C; a.so = (long long)Nq * C; a.B = B; a.H = H; a.D = D; a.Nq = Nq; a.Nk = Nk; a.scale = 1.0f / sqrtf((float)D);
  // record: 1 per-head rows; 2, 3, 4 = head-group sums with 8, 4, 2 heads per workgroup
  if (record) { a.record_mode = record >= 2 ? 3 : 1; a.rec_hpb = record >= 2 ? (16 >> record < H ? 16 >> record : H) : 0; a.rec_b0 = B / 2; a.rec = rec;
                a.rec_T = Nk; a.rec_head_stride = (long long)Nk * Nq; a.rec_img_stride = a.rec_head_stride * (record >= 2 ? H / a.rec_hpb : H); }
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  for (int i = 0; i < 2; ++i) CK(launch_attention(a, 0));
  hipEventRecord(e0, 0);
  for (int i = 0; i < iters; ++i) CK(launch_attention(a, 0));
  hipEventRecord(e1, 0); hipEventSynchronize(e1);
  float t = 0; hipEventElapsedTime(&t, e0, e1);
  *ms_out = t / iters;
  hipEventDestroy(e0); hipEventDestroy(e1);
  return 0;
}

// GroupNorm(+SiLU) of a [B][HW][C0 (+ C1 concatenated)] activation; fused_stats != 0 takes the one-kernel path that reads the
// producing igemm launches' per-(128-row tile, channel) partial sums (here: arbitrary values -- timing only)
AGD_API int agd_bench_groupnorm_ex(int B, int HW, int C0, int C1, int fused_stats, int iters, double* ms_out) {
  Tmp tmp;
  const int C = C0 + C1;
  if (B < 1 || HW < 1 || C0 < 8 || C1 < 0 || iters < 1 || !ms_out) { agd_set_error("bench_groupnorm: bad arguments"); return -1; }
  if (groupnorm_check(B, C0, C1, HW, 32)) return -1;
  bf16_t* x0 = tmp.get<bf16_t>((size_t)B * HW * C0); bf16_t* x1 = C1 ? tmp.get<bf16_t>((size_t)B * HW * C1) : nullptr;
  bf16_t* y = tmp.get<bf16_t>((size_t)B * HW * C);
  float* ws = tmp.get<float>((size_t)groupnorm_ws_floats(B, C, HW, 32)); float* g = tmp.get<float>(2 * C);
  if (!x0 || (C1 && !x1) || !y || !ws || !g) return -1;
  fill_rand(x0, (long long)B * HW * C0, 7, 1.0f); if (C1) fill_rand(x1, (long long)B * HW * C1, 8, 1.0f);
  hipMemset(g, 0, 2 * C * 4);
  GroupNormP p{}; p.x0 = x0; p.x1 = x1; p.C0 = C0; p.C1 = C1; p.y = y; p.gamma = g; p.beta = g + C; p.B = B; p.HW = HW; p.groups = 32; p.eps = 1e-5f; p.silu = 1; p.ws = ws;
  if (fused_stats) {
    if (HW % 128) { agd_set_error("bench_groupnorm: fused_stats needs HW %% 128 == 0"); return -1; }
    const size_t n0 = (size_t)B * (HW / 128) * C0 * 2, n1 = (size_t)B * (HW / 128) * C1 * 2;
    float* p0 = tmp.get<float>(n0); float* p1 = C1 ? tmp.get<float>(n1) : nullptr;
    if (!p0 || (C1 && !p1)) return -1;
    hipMemset(p0, 0, n0 * 4); if (C1) hipMemset(p1, 0, n1 * 4);
    p.part0 = p0; p.part1 = p1; p.bm0 = 128; p.bm1 = C1 ? 128 : 0;
  }
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  for (int i = 0; i < 2; ++i) CK(launch_groupnorm(p, 0));
  hipEventRecord(e0, 0);
  for (int i = 0; i < iters; ++i) CK(launch_groupnorm(p, 0));
  hipEventRecord(e1, 0); hipEventSynchronize(e1);
  float t = 0; hipEventElapsedTime(&t, e0, e1);
  *ms_out = t / iters;
  hipEventDestroy(e0); hipEventDestroy(e1);
  return 0;
}
AGD_API int agd_bench_groupnorm(int B, int HW, int C, int iters, double* ms_out) { return agd_bench_groupnorm_ex(B, HW, C, 0, 0, iters, ms_out); }
#endif  // AGD_EXPERIMENTS


// ---------------------------------------------------------------------------------------
// export entry points
// ---------------------------------------------------------------------------------------
namespace {
struct PilCoeffs { int in = 0, out = 0, ksize = 0; int* bounds = nullptr; int* kk = nullptr; };
double pil_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
// Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc (PRECISION_BITS = 22), cached per (in, out)
const PilCoeffs* pil_coeffs(int in_size, int out_size) {
  static std::vector<PilCoeffs> cache;
  for (auto& c : cache) if (c.in == in_size && c.out == out_size) return &c;
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  std::vector<int> bounds(2 * out_size), kk((size_t)out_size * ksize, 0);
  std::vector<double> w(ksize);
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5); if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5); if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) { w[x] = pil_bicubic((x + xmin - center + 0.5) * ss); ww += w[x]; }
    for (int x = 0; x < xmax; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
    }
    bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
  }
  PilCoeffs c; c.in = in_size; c.out = out_size; c.ksize = ksize;
  if (hipMalloc((void**)&c.bounds, bounds.size() * 4) != hipSuccess || hipMalloc((void**)&c.kk, kk.size() * 4) != hipSuccess) return nullptr;
  hipMemcpy(c.bounds, bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(c.kk, kk.data(), kk.size() * 4, hipMemcpyHostToDevice);
  cache.push_back(c);
  return &cache.back();
}
}  // namespace

AGD_API int agd_op_heatmap_u8(const float* hm, int n, int npix, unsigned char* out, void* stream) {
  CK(launch_heatmap_u8(hm, n, npix, out, S(stream)));
  return 0;
}

// in [n][H][W][C] uint8 -> out [n][oh][ow][C], == PIL Image.resize((ow, oh)) per image (default BICUBIC)
AGD_API int agd_op_resize_u8_pil(const unsigned char* in, int n, int H, int W, int C, int oh, int ow, unsigned char* out, void* stream) {
  hipStream_t st = S(stream);
  const unsigned char* src = in;
  unsigned char* tmp = nullptr;
  if (W != ow) {                                            // horizontal pass first
    const PilCoeffs* ch = pil_coeffs(W, ow); if (!ch) FAIL("resize: coefficient upload failed");
    unsigned char* dst = out;
    if (H != oh) { if (hipMalloc((void**)&tmp, (size_t)n * H * ow * C) != hipSuccess) FAIL("resize: tmp alloc"); dst = tmp; }
    CK(launch_pil_resample(src, dst, ch->bounds, ch->kk, ch->ksize, (long long)n * H, W, ow, C, st));
    src = dst;
  }
  if (H != oh) {                                            // then vertical
    const PilCoeffs* cv = pil_coeffs(H, oh); if (!cv) FAIL("resize: coefficient upload failed");
    CK(launch_pil_resample(src, out, cv->bounds, cv->kk, cv->ksize, n, H, oh, ow * C, st));
  } else if (W == ow) {
    hipMemcpyAsync(out, in, (size_t)n * H * W * C, hipMemcpyDeviceToDevice, st);
  }
  hipStreamSynchronize(st);
  if (tmp) hipFree(tmp);
  return 0;
}

AGD_API int agd_op_stack_heatmaps(const unsigned char* obj, const unsigned char* fg, const unsigned char* bg, long long npix,
                                     unsigned char* rgb, unsigned char* inv, void* stream) {
  CK(launch_stack_heatmaps(obj, fg, bg, npix, rgb, inv, S(stream)));
  return 0;
}


// ---------------------------------------------------------------------------------------
// CLIP text encoder: `pipeline.text_encoder(input_ids)[0]`
// ---------------------------------------------------------------------------------------
AGD_API int agd_text_set_embedding_row(agd_ctx* c, int token_id, const float* row) {
  API_CK(c, need_final(c));
  const WMat* te = getW(c, "text.embeddings.token_embedding.weight"); if (!te) return fail_ctx(c);
  if (token_id < 0 || token_id >= te->N + kTextExtraRows) { agd_set_error("text: token id %d out of range (vocab %d + %d)", token_id, te->N, kTextExtraRows); return fail_ctx(c); }
  Tmp tmp; float* d = tmp.get<float>(te->Cpad); if (!d) return fail_ctx(c);
  if (hipMemcpy(d, row, (size_t)te->Cin * 4, hipMemcpyDefault) != hipSuccess) { agd_set_error("text: row copy failed"); return fail_ctx(c); }
  API_CK(c, launch_f32_to_bf16(d, te->w + (size_t)token_id * te->Cpad, te->Cin, 0));
  hipDeviceSynchronize();
  return 0;
}

// The layer loop of a CLIP encoder (transformers CLIPEncoder: pre-LN, fused q/k/v, attention with head dim H / heads,
// out_proj + residual, pre-LN, fc1 + quick_gelu / gelu, fc2 + residual) over the residual stream x bf16 [B T][H] in place;
// shared by the text encoder (causal) and the safety checker's vision tower (causal = 0, T = 257).  h / qkv / att / ff are
// scratch of [B T] rows x H / 3H / H / inter.  prof_cls >= 0 times every launch under that class (the text path keeps its classes).
struct ClipEnc { std::string prefix; int layers, H, heads, inter, act; float eps; int causal; int prof_cls; };
static int clip_encoder_layers(agd_ctx* c, hipStream_t st, const ClipEnc& e, int B, int T, bf16_t* x, bf16_t* h, bf16_t* qkv, bf16_t* att,
                               bf16_t* ff) {
  const int H = e.H, D = H / e.heads, M = B * T;
  auto ln = [&](const float* g, const float* b) {
    if (e.prof_cls < 0) return launch_layernorm(x, h, g, b, M, H, e.eps, st);
    ProfScope ps(c, st, e.prof_cls, 0, 4.0 * M * (double)H);
    return launch_layernorm(x, h, g, b, M, H, e.eps, st);
  };
  for (int l = 0; l < e.layers; ++l) {
    const std::string L = e.prefix + std::to_string(l) + ".";
    const float* g1 = getV(c, L + "layer_norm1.weight"); const float* b1 = getV(c, L + "layer_norm1.bias");
    const float* g2 = getV(c, L + "layer_norm2.weight"); const float* b2 = getV(c, L + "layer_norm2.bias");
    const WMat* wqkv = getW(c, L + "self_attn.qkv.weight"); const float* bqkv = getV(c, L + "self_attn.qkv.bias");
    const WMat* wo = getW(c, L + "self_attn.out_proj.weight"); const float* bo = getV(c, L + "self_attn.out_proj.bias");
    const WMat* w1 = getW(c, L + "mlp.fc1.weight"); const float* bf1 = getV(c, L + "mlp.fc1.bias");
    const WMat* w2 = getW(c, L + "mlp.fc2.weight"); const float* bf2 = getV(c, L + "mlp.fc2.bias");
    if (!g1 || !b1 || !g2 || !b2 || !wqkv || !bqkv || !wo || !bo || !w1 || !bf1 || !w2 || !bf2) return -1;
    if (ln(g1, b1)) return -1;
    { GemmOpt o; o.bias = bqkv; o.prof_cls = e.prof_cls; if (run_conv(c, st, h, H, nullptr, 0, 1, 1, M, *wqkv, 1, qkv, o, c->zero_page)) return -1; }
    { AttnP a{}; a.q = qkv; a.k = qkv + H; a.v = qkv + 2 * H; a.o = att; a.ldq = a.ldk = a.ldv = 3 * H; a.ldo = H;
      a.sq = a.sk = a.sv = (long long)T * 3 * H; a.so = (long long)T * H; a.B = B; a.H = e.heads; a.D = D; a.Nq = T; a.Nk = T;
      a.scale = 1.0f / sqrtf((float)D); a.causal = e.causal;
      if (run_attention(c, st, PC_OTHER, a)) return -1; }
    { GemmOpt o; o.bias = bo; o.residual = x; o.prof_cls = e.prof_cls; if (run_conv(c, st, att, H, nullptr, 0, 1, 1, M, *wo, 1, x, o, c->zero_page)) return -1; }
    if (ln(g2, b2)) return -1;
    { GemmOpt o; o.bias = bf1; o.act = e.act == 0 ? 2 : 3; o.prof_cls = e.prof_cls; if (run_conv(c, st, h, H, nullptr, 0, 1, 1, M, *w1, 1, ff, o, c->zero_page)) return -1; }
    { GemmOpt o; o.bias = bf2; o.residual = x; o.prof_cls = e.prof_cls; if (run_conv(c, st, ff, e.inter, nullptr, 0, 1, 1, M, *w2, 1, x, o, c->zero_page)) return -1; }
  }
  return 0;
}

AGD_API int agd_text_encode(agd_ctx* c, const int* input_ids, int B, int T, float* out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  const agd_config& g = c->cfg;
  if (g.text_layers <= 0) { agd_set_error("text encoder not configured"); return fail_ctx(c); }
  const int H = g.text_hidden, M = B * T;
  if (T > g.text_max_pos || T > 96) { agd_set_error("text: %d tokens unsupported (max %d)", T, g.text_max_pos < 96 ? g.text_max_pos : 96); return fail_ctx(c); }
  const std::string tx = "text.";
  const WMat* te = getW(c, tx + "embeddings.token_embedding.weight"); const WMat* pe = getW(c, tx + "embeddings.position_embedding.weight");
  if (!te || !pe) return fail_ctx(c);
  c->arena.release(0);
  int* ids = (int*)c->arena.alloc((size_t)M * 4);
  bf16_t* x = (bf16_t*)c->arena.alloc((size_t)M * H * 2); bf16_t* h = (bf16_t*)c->arena.alloc((size_t)M * H * 2);
  bf16_t* qkv = (bf16_t*)c->arena.alloc((size_t)M * 3 * H * 2); bf16_t* att = (bf16_t*)c->arena.alloc((size_t)M * H * 2);
  bf16_t* ff = (bf16_t*)c->arena.alloc((size_t)M * g.text_intermediate * 2);
  if (!ids || !x || !h || !qkv || !att || !ff) return fail_ctx(c);
  if (hipMemcpyAsync(ids, input_ids, (size_t)M * 4, hipMemcpyDefault, st) != hipSuccess) { agd_set_error("text: ids copy failed"); return fail_ctx(c); }
  API_CK(c, launch_embed_gather(ids, te->w, pe->w, x, B, T, H, te->N + kTextExtraRows, st));
  const ClipEnc enc{tx + "encoder.layers.", g.text_layers, H, g.text_heads, g.text_intermediate, g.text_act, g.text_eps, 1, -1};
  API_CK(c, clip_encoder_layers(c, st, enc, B, T, x, h, qkv, att, ff));
  { const float* gf = getV(c, tx + "final_layer_norm.weight"); const float* bfn = getV(c, tx + "final_layer_norm.bias");
    if (!gf || !bfn) return fail_ctx(c);
    API_CK(c, launch_layernorm(x, h, gf, bfn, M, H, g.text_eps, st));
    API_CK(c, launch_bf16_to_f32(h, out, (long long)M * H, st)); }
  return 0;
}


// ---------------------------------------------------------------------------------------
// Safety checker (`pipeline.safety_checker`, data_generation.py:59-62): StableDiffusionSafetyChecker's CLIP vision tower + cosines
// ---------------------------------------------------------------------------------------
// what both towers need of their config; the head dim (64, or 80 for the image encoder) is the caller's check
static int check_vision_config(const agd_vision_config* v, const char* who) {
  if (v->hidden < 64 || v->hidden > 2048 || v->hidden % 64 || v->heads < 1 || v->hidden % v->heads)
    FAIL("%s: hidden %d / heads %d unsupported (hidden a multiple of 64 up to 2048, head dim 64)", who, v->hidden, v->heads);
  if (v->layers < 1 || v->intermediate < 64 || v->intermediate % 64 || v->act < 0 || v->act > 1)
    FAIL("%s: layers %d / intermediate %d / act %d unsupported", who, v->layers, v->intermediate, v->act);
  if (v->patch_size < 1 || v->image_size < v->patch_size || v->image_size % v->patch_size || v->image_size > 4096)
    FAIL("%s: image_size %d / patch_size %d unsupported", who, v->image_size, v->patch_size);
  if (v->projection_dim < 1 || v->hidden + v->projection_dim + 4 > 16384 || v->n_special < 0 || v->n_concepts < 0)
    FAIL("%s: projection_dim %d / %d special / %d concepts unsupported", who, v->projection_dim, v->n_special, v->n_concepts);
  for (int i = 0; i < 3; ++i) if (!(v->std[i] > 0.f)) FAIL("%s: image_std[%d] = %g", who, i, v->std[i]);
  return 0;
}

AGD_API int agd_safety_configure(agd_ctx* c, const agd_vision_config* v) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  if (!v || v->struct_size != (int)sizeof(agd_vision_config)) {
    agd_set_error("agd_safety_configure: bad config (struct_size %d != %zu)", v ? v->struct_size : -1, sizeof(agd_vision_config)); return fail_ctx(c); }
  if (c->finalized) { agd_set_error("agd_safety_configure: call it before agd_finalize"); return fail_ctx(c); }
  API_CK(c, check_vision_config(v, "agd_safety_configure"));
  if (v->hidden / v->heads != 64)
    { agd_set_error("agd_safety_configure: hidden %d / heads %d unsupported (hidden a multiple of 64 up to 2048, head dim 64)", v->hidden, v->heads); return fail_ctx(c); }
  if (v->n_special + v->n_concepts < 1)
    { agd_set_error("agd_safety_configure: projection_dim %d / %d special / %d concepts unsupported", v->projection_dim, v->n_special, v->n_concepts); return fail_ctx(c); }
  c->vis = *v; c->vis_on = true;
  return 0;
}

// The vision path shared by agd_safety_scores_hw and agd_image_embeds: CLIPImageProcessor on uint8 NHWC images (device), the patch
// embedding, class / position embeddings + pre_layrnorm, the encoder layers, then the pooled head -- post_layernorm(CLS),
// visual_projection, and either the cosines against `concepts` (n rows) or the projected embeddings themselves (emb_out), or both.
static int vision_embed(agd_ctx* c, hipStream_t st, const VisTower& tw, const unsigned char* images, int B, int ih, int iw, float* pixels_out,
                        const float* concepts, int n, float* cos_out, float* emb_out) {
  const agd_vision_config& v = *tw.v;
  const char* kVisPre = tw.pre.c_str();
  const int R = v.image_size, ps = v.patch_size, g = R / ps, np = g * g, T = np + 1, H = v.hidden, M = B * T;
  const std::string E = tw.pre + "embeddings.";
  const WMat* pw = getW(c, tw.patch);
  const float* cls = getV(c, E + "class_embedding"); const float* pos = getV(c, E + "position_embedding.weight");
  const float* g0 = getV(c, std::string(kVisPre) + "pre_layrnorm.weight"); const float* b0 = getV(c, std::string(kVisPre) + "pre_layrnorm.bias");
  const float* gp = getV(c, std::string(kVisPre) + "post_layernorm.weight"); const float* bp = getV(c, std::string(kVisPre) + "post_layernorm.bias");
  const float* wp = getV(c, tw.proj);
  if (!pw || !cls || !pos || !g0 || !b0 || !gp || !bp || !wp) return fail_ctx(c);
  // scratch from the activation arena only (like agd_text_encode): the recorder accumulators, the cached context and the scheduler's
  // buffers are context-owned allocations this call never touches
  c->arena.release(0);
  // CLIPImageProcessor geometry: the shortest edge resized to image_size, the long one to int(image_size * long / short), then the
  // image_size x image_size center crop at ((rh - R) / 2, (rw - R) / 2)
  const int rh = ih <= iw ? R : (int)((long long)R * ih / iw), rw = ih <= iw ? (int)((long long)R * iw / ih) : R;
  const bool resize = rh != ih || rw != iw, crop = rh != R || rw != R;
  unsigned char* tmp = nullptr; unsigned char* img = nullptr; unsigned char* cropped = nullptr;
  if (resize) {
    tmp = (unsigned char*)c->arena.alloc((size_t)B * ih * rw * 3); img = (unsigned char*)c->arena.alloc((size_t)B * rh * rw * 3);
    if (!tmp || !img) return fail_ctx(c);
  }
  if (crop) { cropped = (unsigned char*)c->arena.alloc((size_t)B * R * R * 3); if (!cropped) return fail_ctx(c); }
  bf16_t* rows = (bf16_t*)c->arena.alloc((size_t)B * np * pw->Cpad * 2); float* pe = (float*)c->arena.alloc((size_t)B * np * H * 4);
  bf16_t* x = (bf16_t*)c->arena.alloc((size_t)M * H * 2); bf16_t* h = (bf16_t*)c->arena.alloc((size_t)M * H * 2);
  bf16_t* qkv = (bf16_t*)c->arena.alloc((size_t)M * 3 * H * 2); bf16_t* att = (bf16_t*)c->arena.alloc((size_t)M * H * 2);
  bf16_t* ff = (bf16_t*)c->arena.alloc((size_t)M * v.intermediate * 2);
  if (!rows || !pe || !x || !h || !qkv || !att || !ff) return fail_ctx(c);
  // CLIPImageProcessor: PIL BICUBIC resize, horizontal pass then vertical (Pillow's order; a pass whose axis keeps its size is skipped
  // in both Pillow and here); the coefficient tables are built and uploaded once per (in, out) and cached
  const unsigned char* src = images;
  if (resize) {
    const unsigned char* hsrc = images; unsigned char* hdst = rh != ih ? tmp : img;
    if (rw != iw) {
      const PilCoeffs* cf = pil_coeffs(iw, rw); if (!cf) FAIL("safety: resize coefficient upload failed");
      ProfScope ps_(c, st, PC_OTHER, 0, (double)B * ih * (iw + rw) * 3);
      API_CK(c, launch_pil_resample(images, hdst, cf->bounds, cf->kk, cf->ksize, (long long)B * ih, iw, rw, 3, st));
      hsrc = hdst;
    }
    if (rh != ih) {
      const PilCoeffs* cf = pil_coeffs(ih, rh); if (!cf) FAIL("safety: resize coefficient upload failed");
      ProfScope ps_(c, st, PC_OTHER, 0, (double)B * rw * (ih + rh) * 3);
      API_CK(c, launch_pil_resample(hsrc, img, cf->bounds, cf->kk, cf->ksize, B, ih, rh, rw * 3, st));
    }
    src = img;
  }
  if (crop) {
    const int top = (rh - R) / 2, left = (rw - R) / 2;
    ProfScope ps_(c, st, PC_OTHER, 0, 2.0 * B * R * R * 3);
    for (int b = 0; b < B; ++b)
      if (hipMemcpy2DAsync(cropped + (size_t)b * R * R * 3, (size_t)R * 3, src + (((size_t)b * rh + top) * rw + left) * 3, (size_t)rw * 3,
                           (size_t)R * 3, R, hipMemcpyDeviceToDevice, st) != hipSuccess) FAIL("safety: center crop copy failed");
    src = cropped;
  }
  const VisNorm nm{v.mean[0], v.mean[1], v.mean[2], v.std[0], v.std[1], v.std[2]};
  { ProfScope ps_(c, st, PC_OTHER, 0, (double)B * R * R * 3 + 2.0 * B * np * pw->Cpad);
    API_CK(c, launch_vis_patchify(src, B, R, ps, pw->Cpad, nm, rows, pixels_out, st)); }
  { GemmOpt o; o.out_f32 = 1; o.prof_cls = PC_OTHER; API_CK(c, run_conv(c, st, rows, pw->Cpad, nullptr, 0, 1, 1, B * np, *pw, 1, pe, o, c->zero_page)); }
  { ProfScope ps_(c, st, PC_OTHER, 0, 4.0 * B * np * H + 2.0 * M * H);
    API_CK(c, launch_vis_embed_ln(pe, cls, pos, g0, b0, B, np, H, v.eps, x, st)); }
  const ClipEnc enc{std::string(kVisPre) + "encoder.layers.", v.layers, H, v.heads, v.intermediate, v.act, v.eps, 0, PC_OTHER};
  API_CK(c, clip_encoder_layers(c, st, enc, B, T, x, h, qkv, att, ff));
  { ProfScope ps_(c, st, PC_OTHER, 2.0 * B * (double)v.projection_dim * (H + n), 4.0 * (double)v.projection_dim * (H + n));
    API_CK(c, launch_vis_pooled_head(x, B, T, H, gp, bp, v.eps, wp, v.projection_dim, concepts, n, cos_out, emb_out, st)); }
  return 0;
}

AGD_API int agd_safety_scores_hw(agd_ctx* c, const unsigned char* images, int B, int ih, int iw, float* cos_out, float* pixels_out, void* stream) {
  API_CK(c, need_final(c));
  if (!c->vis_on) { agd_set_error("safety checker not configured (agd_safety_configure before agd_finalize)"); return fail_ctx(c); }
  if (B < 1 || ih < 1 || iw < 1 || !images || !cos_out) { agd_set_error("safety_scores: batch %d size %d x %d / null buffer", B, ih, iw); return fail_ctx(c); }
  return vision_embed(c, S(stream), safety_tower(c), images, B, ih, iw, pixels_out, c->vis_concepts, c->vis.n_special + c->vis.n_concepts, cos_out, nullptr);
}
AGD_API int agd_safety_scores(agd_ctx* c, const unsigned char* images, int B, int side, float* cos_out, float* pixels_out, void* stream) {
  return agd_safety_scores_hw(c, images, B, side, side, cos_out, pixels_out, stream);
}


// `vae.encode(image).latent_dist` moments: image fp32 NCHW [B,3,S,S] in [-1,1] -> mean, logvar fp32 NCHW [B,lc,L,L]
AGD_API int agd_vae_encode_hw(agd_ctx* c, const float* image, int batch, int h, int w, float* mean_out, float* logvar_out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  const int lc = c->cfg.vae_latent_channels, f = 1 << (c->cfg.vae_n_levels - 1), Lh = h / f, Lw = w / f;
  if (h < 1 || w < 1 || h % f || h % 8 || w % f || w % 8) { agd_set_error("vae_encode: size %d x %d not divisible", h, w); return fail_ctx(c); }
  const size_t hw = (size_t)Lh * Lw;
  Tmp tmp;
  bf16_t* x = tmp.get<bf16_t>((size_t)batch * h * w * 64); float* mom = tmp.get<float>((size_t)batch * hw * 2 * lc);
  float* mom_nchw = tmp.get<float>((size_t)batch * hw * 2 * lc);
  if (!x || !mom || !mom_nchw) return fail_ctx(c);
  API_CK(c, launch_prep_latents(image, x, batch, c->cfg.vae_out_channels, h * w, 64, 1, 1.0f, st));
  API_CK(c, vae_encode_walk(c, st, x, batch, h, w, mom));
  API_CK(c, launch_nchw_from_nhwc_f32(mom, 2 * lc, mom_nchw, batch, 2 * lc, (int)hw, st));
  for (int b = 0; b < batch; ++b) {
    hipMemcpyAsync(mean_out + (size_t)b * lc * hw, mom_nchw + (size_t)b * 2 * lc * hw, (size_t)lc * hw * 4, hipMemcpyDeviceToDevice, st);
    hipMemcpyAsync(logvar_out + (size_t)b * lc * hw, mom_nchw + ((size_t)b * 2 + 1) * lc * hw, (size_t)lc * hw * 4, hipMemcpyDeviceToDevice, st);
  }
  hipStreamSynchronize(st);
  return 0;
}
AGD_API int agd_vae_encode(agd_ctx* c, const float* image, int batch, int side, float* mean_out, float* logvar_out, void* stream) {
  return agd_vae_encode_hw(c, image, batch, side, side, mean_out, logvar_out, stream);
}

// ---------------------------------------------------------------------------------------
// ControlNet (diffusers ControlNetModel + StableDiffusionControlNetPipeline, SD-1.x): the walk is controlnet_walk inside unet_walk
// ---------------------------------------------------------------------------------------
AGD_API int agd_controlnet_configure(agd_ctx* c, const agd_controlnet_config* e) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  if (!e || e->struct_size != (int)sizeof(agd_controlnet_config)) {
    agd_set_error("agd_controlnet_configure: bad config (struct_size %d != %zu)", e ? e->struct_size : -1, sizeof(agd_controlnet_config)); return fail_ctx(c); }
  if (c->finalized) { agd_set_error("agd_controlnet_configure: call it before agd_finalize"); return fail_ctx(c); }
  if (e->n_emb < 2 || e->n_emb > AGD_CN_MAX_EMB) { agd_set_error("agd_controlnet_configure: %d embedding channel counts (2 .. %d)", e->n_emb, AGD_CN_MAX_EMB); return fail_ctx(c); }
  for (int i = 0; i < e->n_emb; ++i)
    if (e->emb_channels[i] < 1 || e->emb_channels[i] > 4096) { agd_set_error("agd_controlnet_configure: embedding channels[%d] = %d", i, e->emb_channels[i]); return fail_ctx(c); }
  c->cnc = *e; c->cn_on = true;
  return 0;
}

// the conditioning embedding, once per call: conv_in (+ SiLU), per step a 3x3 (+ SiLU) and a stride-2 3x3 (+ SiLU), conv_out -- 2 n_emb igemm
// launches (SD-1.x: eight).  The 3-channel image is zero-padded to 64 channels like the VAE encoder's input; maps whose width is not a
// multiple of 64 (16 / 32 / 96 by default) are written with a 64-multiple row stride into zeroed buffers, so every conv reads whole
// 64-channel chunks.  It runs on the `batch` distinct images only; the other repeat - 1 row blocks are copies.
AGD_API int agd_controlnet_set_cond_hw(agd_ctx* c, const float* cond, int batch, int ih, int iw, int repeat, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!c->cn_on) { agd_set_error("controlnet_set_cond: no ControlNet loaded"); return fail_ctx(c); }
  const agd_controlnet_config& e = c->cnc;
  const int sh = e.n_emb - 1, Lh = ih >> sh, Lw = iw >> sh, C0 = c->cfg.block_out_channels[0];
  if (!cond || batch < 1 || repeat < 1 || Lh < 1 || Lw < 1 || (Lh << sh) != ih || (Lw << sh) != iw)
    { agd_set_error("controlnet_set_cond: batch %d / repeat %d / size %d x %d (each side a multiple of %d)", batch, repeat, ih, iw, 1 << sh); return fail_ctx(c); }
  const int B2 = batch * repeat;
  c->cn_emb_B2 = 0; c->cn_emb_Lh = c->cn_emb_Lw = 0;               // (unset until the embedding below is complete)
  c->arena.release(0);
  // ping-pong scratch: the largest map of the chain -- the padded input (H x W x 64) or any intermediate output (Ho x Wo x its padded width)
  size_t big = (size_t)batch * ih * iw * 64;
  { long long h = ih, w = iw;
    auto out_elems = [&](int ch) -> size_t { const size_t ld = (size_t)(ch + 63) / 64 * 64; return (size_t)batch * (size_t)h * (size_t)w * ld; };
    big = std::max(big, out_elems(e.emb_channels[0]));
    for (int i = 0; i + 1 < e.n_emb; ++i) { big = std::max(big, out_elems(e.emb_channels[i])); h /= 2; w /= 2; big = std::max(big, out_elems(e.emb_channels[i + 1])); } }
  big *= 2;
  bf16_t* buf[2] = {(bf16_t*)c->arena.alloc(big), (bf16_t*)c->arena.alloc(big)};
  if (!buf[0] || !buf[1]) return fail_ctx(c);
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_controlnet_cond_prep(cond, buf[0], batch, ih * iw, 64, e.bgr, st)); }
  API_CK(c, c->cn_embb.ensure((size_t)B2 * Lh * Lw * C0 * 2));
  const std::string E = "controlnet.controlnet_cond_embedding.";
  int cur = 0, H = ih, W = iw, Cin = 64;
  auto conv = [&](const std::string& k, int stride, bool last) -> int {
    GETW(w, E + k + ".weight"); GETV(b, E + k + ".bias");
    if (w->Cpad != Cin) FAIL("controlnet_set_cond: '%s' reads %d channels, the map has %d", k.c_str(), w->Cpad, Cin);
    const int Ho = H / stride, Wo = W / stride, ld = last ? w->N : (w->N + 63) / 64 * 64;
    if (last ? w->N != C0 : (size_t)batch * Ho * Wo * ld * 2 > big) FAIL("controlnet_set_cond: '%s' output [%d x %d x %d] does not fit its buffer", k.c_str(), Ho, Wo, ld);
    bf16_t* out = last ? c->cn_embb.as<bf16_t>() : buf[cur ^ 1];
    if (!last && ld != w->N && hipMemsetAsync(out, 0, (size_t)batch * Ho * Wo * ld * 2, st) != hipSuccess) FAIL("controlnet_set_cond: memset");
    GemmOpt o; o.bias = b; o.act = last ? 0 : 1; o.stride = stride; o.ldo = ld;
    CK(run_conv(c, st, buf[cur], Cin, nullptr, 0, batch, H, W, *w, 3, out, o, c->zero_page));
    cur ^= 1; H = Ho; W = Wo; Cin = ld;
    return 0;
  };
  API_CK(c, conv("conv_in", 1, false));
  for (int i = 0; i + 1 < e.n_emb; ++i) {
    API_CK(c, conv("blocks." + std::to_string(2 * i), 1, false));
    API_CK(c, conv("blocks." + std::to_string(2 * i + 1), 2, false));
  }
  API_CK(c, conv("conv_out", 1, true));
  { const size_t blk = (size_t)batch * Lh * Lw * C0;               // rows r and r + batch are the same image
    ProfScope ps(c, st, PC_ELEM, 0);
    for (int r = 1; r < repeat; ++r)
      if (hipMemcpyAsync(c->cn_embb.as<bf16_t>() + r * blk, c->cn_embb.as<bf16_t>(), blk * 2, hipMemcpyDeviceToDevice, st) != hipSuccess)
        { agd_set_error("controlnet_set_cond: row copy failed"); return fail_ctx(c); } }
  c->cn_emb_B2 = B2; c->cn_emb_Lh = Lh; c->cn_emb_Lw = Lw; c->cn_emb_rep = repeat;
  return 0;
}
AGD_API int agd_controlnet_set_cond(agd_ctx* c, const float* cond, int batch, int side, int repeat, void* stream) {
  return agd_controlnet_set_cond_hw(c, cond, batch, side, side, repeat, stream);
}

// agd_controlnet_set_schedule / agd_adapter_set_schedule: n finite scales, one per model evaluation (n = 0 clears) for a loaded model
static int set_scale_schedule(agd_ctx* c, const char* what, const char* model, bool loaded, const float* scales, int n, std::vector<float>* sched) {
  if (n < 0 || (n > 0 && !scales)) { agd_set_error("%s: %d scales", what, n); return fail_ctx(c); }
  if (n > 0 && !loaded) { agd_set_error("%s: no %s loaded", what, model); return fail_ctx(c); }
  for (int i = 0; i < n; ++i) if (!std::isfinite(scales[i])) { agd_set_error("%s: scale %d is %g", what, i, scales[i]); return fail_ctx(c); }
  sched->assign(scales, scales + n);
  return 0;
}
AGD_API int agd_controlnet_set_schedule(agd_ctx* c, const float* scales, int n) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  return set_scale_schedule(c, "controlnet_set_schedule", "ControlNet", c->cn_on, scales, n, &c->cn_sched);
}

AGD_API int agd_controlnet_residuals_hw(agd_ctx* c, const float* sample, int batch2, int Lh, int Lw, float timestep, float scale, int nhwc,
                                        float* out, long long* n_out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!c->cn_on) { agd_set_error("controlnet_residuals: no ControlNet loaded"); return fail_ctx(c); }
  const int sh = c->cfg.n_levels - 1;
  if (batch2 < 1 || Lh < 1 || Lw < 1 || (Lh >> sh) < 1 || (Lw >> sh) < 1) { agd_set_error("controlnet_residuals: batch2 %d latent size %d x %d", batch2, Lh, Lw); return fail_ctx(c); }
  API_CK(c, check_latent_hw(c, "controlnet_residuals", Lh, Lw));
  long long n = 0;
  { long long h = Lh, w = Lw; int k = 0;
    const std::vector<int> ch = controlnet_res_channels(c->cfg);
    n += (long long)batch2 * ch[k++] * h * w;
    for (int i = 0; i < c->cfg.n_levels; ++i) {
      for (int j = 0; j < c->cfg.layers_per_block; ++j) n += (long long)batch2 * ch[k++] * h * w;
      if (i != c->cfg.n_levels - 1) { h /= 2; w /= 2; n += (long long)batch2 * ch[k++] * h * w; }
    }
    n += (long long)batch2 * c->cfg.block_out_channels[c->cfg.n_levels - 1] * h * w; }
  if (n_out) *n_out = n;
  if (!out) return 0;
  if (!sample) { agd_set_error("controlnet_residuals: null sample"); return fail_ctx(c); }
  API_CK(c, ensure_lat(c, batch2, Lh, Lw));
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_prep_latents(sample, c->lat_bf16, batch2, c->cfg.in_channels, Lh * Lw, 64, 1, 1.0f, st)); }
  c->arena.release(0);
  API_CK(c, controlnet_walk(c, st, c->lat_bf16, batch2, Lh, Lw, timestep, scale, false, nullptr, nullptr, out, nhwc));
  return 0;
}
AGD_API int agd_controlnet_residuals(agd_ctx* c, const float* sample, int batch2, int L, float timestep, float scale, int nhwc,
                                     float* out, long long* n_out, void* stream) {
  return agd_controlnet_residuals_hw(c, sample, batch2, L, L, timestep, scale, nhwc, out, n_out, stream);
}

// ---------------------------------------------------------------------------------------
// T2I-Adapter (diffusers T2IAdapter "full_adapter" + StableDiffusionAdapterPipeline): the network runs once per call here; the per-evaluation
// adds are adapter_add inside down_mid_walk
// ---------------------------------------------------------------------------------------
AGD_API int agd_adapter_configure(agd_ctx* c, const agd_adapter_config* e) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  if (!e || e->struct_size != (int)sizeof(agd_adapter_config)) {
    agd_set_error("agd_adapter_configure: bad config (struct_size %d != %zu)", e ? e->struct_size : -1, sizeof(agd_adapter_config)); return fail_ctx(c); }
  if (c->finalized) { agd_set_error("agd_adapter_configure: call it before agd_finalize"); return fail_ctx(c); }
  if (e->n_channels < 1 || e->n_channels > AGD_MAX_LEVELS) { agd_set_error("agd_adapter_configure: %d channel counts (1 .. %d)", e->n_channels, AGD_MAX_LEVELS); return fail_ctx(c); }
  for (int i = 0; i < e->n_channels; ++i)
    if (e->channels[i] < 64 || e->channels[i] % 64 || e->channels[i] > 4096) { agd_set_error("agd_adapter_configure: channels[%d] = %d (a multiple of 64)", i, e->channels[i]); return fail_ctx(c); }
  if (e->in_channels < 1 || e->in_channels > 4 || e->num_res_blocks < 1 || e->num_res_blocks > 16 || e->downscale_factor < 1 || e->downscale_factor > 16) {
    agd_set_error("agd_adapter_configure: in_channels %d, num_res_blocks %d, downscale_factor %d", e->in_channels, e->num_res_blocks, e->downscale_factor); return fail_ctx(c); }
  c->adc = *e; c->ad_on = true;
  return 0;
}

// The adapter, once per call, on the arena: front end (pixel unshuffle, channels zero-padded to a 64-multiple), conv_in, then per block the 2x2
// average pool, the 1x1 in_conv and the resnets x + block2(relu(block1(x))) -- block2 takes x as its residual operand, and the block's last
// block2 writes the feature as fp32 (the bf16 copy the next block reads is rounded from it).
AGD_API int agd_adapter_set_cond_hw(agd_ctx* c, const void* image, int image_f32, int batch, int ih, int iw, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!c->ad_on) { agd_set_error("adapter_set_cond: no T2I-Adapter loaded (agd_adapter_configure before agd_finalize)"); return fail_ctx(c); }
  const agd_adapter_config& e = c->adc;
  const int r = e.downscale_factor, f = r << (e.n_channels - 1);
  if (!image || batch < 1 || ih < f || iw < f || ih % f || iw % f) {
    agd_set_error("adapter_set_cond: batch %d / size %d x %d (each side a positive multiple of %d)", batch, ih, iw, f); return fail_ctx(c); }
  const int Lh = ih / r, Lw = iw / r;
  c->ad_B = 0; c->ad_Lh = c->ad_Lw = 0;                            // (unset until every feature below is complete)
  c->arena.release(0);
  const int Cpad = (e.in_channels * r * r + 63) / 64 * 64;
  bf16_t* x0 = (bf16_t*)c->arena.alloc((size_t)batch * Lh * Lw * Cpad * 2); if (!x0) return fail_ctx(c);
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_adapter_front(image, image_f32, batch, ih, iw, e.in_channels, r, Cpad, x0, st)); }
  const std::string A = "adapter.adapter.";
  auto conv = [&](const std::string& k, const bf16_t* src, int Cin, int H, int W, int ks, const bf16_t* residual, void* out, int out_f32) -> int {
    GETW(w, A + k + ".weight"); GETV(b, A + k + ".bias");
    GemmOpt o; o.bias = b; o.residual = residual; o.out_f32 = out_f32;
    return run_conv(c, st, src, Cin, nullptr, 0, batch, H, W, *w, ks, out, o, c->zero_page);
  };
  int H = Lh, W = Lw;
  Act a = alloc_act(c, batch, H, W, e.channels[0]); if (!a.p) return fail_ctx(c);
  API_CK(c, conv("conv_in", x0, Cpad, H, W, 3, nullptr, a.p, 0));
  for (int i = 0; i < e.n_channels; ++i) {
    const std::string Bk = "body." + std::to_string(i) + ".";
    const int co = e.channels[i];
    if (i > 0) {
      Act d = alloc_act(c, batch, H / 2, W / 2, a.C); if (!d.p) return fail_ctx(c);
      { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_adapter_avgpool(a.p, d.p, batch, H, W, a.C, st)); }
      a = d; H /= 2; W /= 2;
    }
    if (a.C != co) {
      Act d = alloc_act(c, batch, H, W, co); if (!d.p) return fail_ctx(c);
      API_CK(c, conv(Bk + "in_conv", a.p, a.C, H, W, 1, nullptr, d.p, 0));
      a = d;
    }
    const size_t n = (size_t)batch * H * W * co;
    API_CK(c, c->ad_featb[i].ensure(n * 4));
    for (int j = 0; j < e.num_res_blocks; ++j) {
      const std::string R = Bk + "resnets." + std::to_string(j) + ".";
      const bool last = j + 1 == e.num_res_blocks;
      Act t = alloc_act(c, batch, H, W, co), y = alloc_act(c, batch, H, W, co); if (!t.p || !y.p) return fail_ctx(c);
      API_CK(c, conv(R + "block1", a.p, co, H, W, 3, nullptr, t.p, 0));
      { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_adapter_relu(t.p, (long long)n, st)); }
      if (!last) API_CK(c, conv(R + "block2", t.p, co, H, W, 1, a.p, y.p, 0));
      else {
        API_CK(c, conv(R + "block2", t.p, co, H, W, 1, a.p, c->ad_featb[i].p, 1));
        if (i + 1 < e.n_channels) { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_f32_to_bf16(c->ad_featb[i].as<float>(), y.p, (long long)n, st)); }
      }
      a = y;
    }
  }
  c->ad_B = batch; c->ad_Lh = Lh; c->ad_Lw = Lw;
  return 0;
}

AGD_API int agd_adapter_features(agd_ctx* c, float* out) {
  API_CK(c, need_final(c));
  if (!c->ad_on || c->ad_B < 1) { agd_set_error("adapter_features: no features set (agd_adapter_set_cond_hw)"); return fail_ctx(c); }
  if (!out) { agd_set_error("adapter_features: null out"); return fail_ctx(c); }
  if (hipDeviceSynchronize() != hipSuccess) { agd_set_error("adapter_features: sync failed"); return fail_ctx(c); }   // (agd_adapter_set_cond_hw ran on the caller's stream)
  size_t off = 0;
  for (int i = 0; i < c->adc.n_channels; ++i) {
    const int C = c->adc.channels[i], hw = (c->ad_Lh >> i) * (c->ad_Lw >> i);
    API_CK(c, launch_nchw_from_nhwc_f32(c->ad_featb[i].as<float>(), C, out + off, c->ad_B, C, hw, 0));
    off += (size_t)c->ad_B * C * hw;
  }
  if (hipStreamSynchronize(0) != hipSuccess) { agd_set_error("adapter_features: sync failed"); return fail_ctx(c); }
  return 0;
}

AGD_API int agd_adapter_set_schedule(agd_ctx* c, const float* scales, int n) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  return set_scale_schedule(c, "adapter_set_schedule", "T2I-Adapter", c->ad_on, scales, n, &c->ad_sched);
}

AGD_API int agd_adapter_clear(agd_ctx* c) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  c->ad_sched.clear(); c->ad_B = 0; c->ad_Lh = c->ad_Lw = 0; c->cur.ad_scale = 0.f;
  return 0;
}

AGD_API int agd_adapter_add_counts(agd_ctx* c, long long* counts) {
  if (!c || !counts) { agd_set_error("adapter_add_counts: null argument"); return fail_ctx(c); }
  counts[0] = c->ad_adds[0]; counts[1] = c->ad_adds[1];
  return 0;
}

// ---------------------------------------------------------------------------------------
// FreeU (diffusers >= 0.22 enable_freeu / disable_freeu [upstream-knowledge]): persistent state that every later unet_walk reads (freeu_apply)
// ---------------------------------------------------------------------------------------
AGD_API int agd_freeu_set(agd_ctx* c, float s1, float s2, float b1, float b2) {
  API_CK(c, need_final(c));
  const float v[4] = {s1, s2, b1, b2}; const char* nm[4] = {"s1", "s2", "b1", "b2"};
  for (int i = 0; i < 4; ++i) if (!std::isfinite(v[i])) { agd_set_error("freeu_set: %s = %g (a finite number)", nm[i], (double)v[i]); return fail_ctx(c); }
  if (c->cfg.n_levels < 2) { agd_set_error("freeu_set: the UNet has %d level(s); FreeU re-weights up blocks 0 and 1", c->cfg.n_levels); return fail_ctx(c); }
  c->fu_s[0] = s1; c->fu_s[1] = s2; c->fu_b[0] = b1; c->fu_b[1] = b2;
  c->fu_on = !(s1 == 1.f && s2 == 1.f && b1 == 1.f && b2 == 1.f);
  deepcache_invalidate(c);
  return 0;
}

AGD_API int agd_freeu_clear(agd_ctx* c) {
  if (!c) { agd_set_error("freeu_clear: null context"); return -1; }
  c->fu_on = false; c->fu_s[0] = c->fu_s[1] = c->fu_b[0] = c->fu_b[1] = 1.f;
  deepcache_invalidate(c);
  return 0;
}

AGD_API int agd_freeu_counts(agd_ctx* c, long long* counts) {
  if (!c || !counts) { agd_set_error("freeu_counts: null argument"); return fail_ctx(c); }
  counts[0] = c->fu_counts[0]; counts[1] = c->fu_counts[1];
  return 0;
}

// The production kernel on fp32 NCHW device tensors (the test seam): inputs rounded to bf16 NHWC, one launch_freeu as the UNet walk issues it
// (with the partial sums where H W % 64 == 0), outputs widened back.  b == 1 / s == 1: that output is the bf16-rounded input.
AGD_API int agd_op_freeu(const float* hidden_nchw, const float* skip_nchw, float* hidden_out, float* skip_out, int B, int Ch, int Cs, int H, int W,
                         float b, float s, void* stream) {
  hipStream_t st = S(stream); Tmp tmp;
  if (!hidden_nchw || !skip_nchw || !hidden_out || !skip_out) { agd_set_error("op_freeu: null argument"); return -1; }
  if (B < 1 || H < 1 || W < 1 || Ch < 8 || Ch % 8 || Cs < 8 || Cs % 8 || (long long)H * W >= (1ll << 24) || (long long)B * H * W * std::max(Ch, Cs) >= (1ll << 31)) {
    agd_set_error("op_freeu: %d maps of %d x %d, %d backbone / %d skip channels (multiples of 8)", B, H, W, Ch, Cs); return -1; }
  if (!std::isfinite(b) || !std::isfinite(s)) { agd_set_error("op_freeu: b = %g, s = %g (finite numbers)", (double)b, (double)s); return -1; }
  const int HW = H * W; const size_t nh = (size_t)B * HW * Ch, ns = (size_t)B * HW * Cs;
  bf16_t* hb = tmp.get<bf16_t>(nh); bf16_t* sb = tmp.get<bf16_t>(ns); bf16_t* ho = tmp.get<bf16_t>(nh); bf16_t* so = tmp.get<bf16_t>(ns);
  float* hf = tmp.get<float>(nh); float* sf = tmp.get<float>(ns);
  float* hp = nullptr; float* sp = nullptr;
  if (HW % 64 == 0) { hp = tmp.get<float>(nh / 64 * 2); sp = tmp.get<float>(ns / 64 * 2); if (!hp || !sp) return -1; }
  if (!hb || !sb || !ho || !so || !hf || !sf) return -1;
  CK(to_nhwc_bf16(hidden_nchw, hb, B, Ch, HW, Ch, st));
  CK(to_nhwc_bf16(skip_nchw, sb, B, Cs, HW, Cs, st));
  if (b != 1.f || s != 1.f) CK(launch_freeu(hb, b != 1.f ? ho : nullptr, hp, Ch, sb, s != 1.f ? so : nullptr, sp, Cs, B, H, W, b, s, st));
  CK(launch_bf16_to_f32(b != 1.f ? ho : hb, hf, (long long)nh, st));
  CK(launch_bf16_to_f32(s != 1.f ? so : sb, sf, (long long)ns, st));
  CK(launch_nchw_from_nhwc_f32(hf, Ch, hidden_out, B, Ch, HW, st));
  CK(launch_nchw_from_nhwc_f32(sf, Cs, skip_out, B, Cs, HW, st));
  hipStreamSynchronize(st);
  return 0;
}

// ---------------------------------------------------------------------------------------
// guidance_rescale (diffusers 0.21.2 StableDiffusionPipeline.__call__(guidance_rescale=phi) -> rescale_noise_cfg [upstream-knowledge]): state
// that the step lambdas of agd_denoise_hw / agd_denoise_plms_hw / agd_denoise_dpm_hw read (guidance_factor)
// ---------------------------------------------------------------------------------------
AGD_API int agd_guidance_rescale_set(agd_ctx* c, float phi) {
  API_CK(c, need_final(c));
  if (!std::isfinite(phi) || phi < 0.f || phi > 1.f) { agd_set_error("guidance_rescale_set: guidance rescale phi = %g (a number in [0, 1])", (double)phi); return fail_ctx(c); }
  c->gr_phi = phi;
  return 0;
}

AGD_API int agd_guidance_rescale_clear(agd_ctx* c) {
  if (!c) { agd_set_error("guidance_rescale_clear: null context"); return -1; }
  c->gr_phi = 0.f;
  return 0;
}

AGD_API int agd_guidance_rescale_counts(agd_ctx* c, long long* launches) {
  if (!c || !launches) { agd_set_error("guidance_rescale_counts: null argument"); return fail_ctx(c); }
  *launches = c->gr_count;
  return 0;
}

// ---- Perturbed-Attention Guidance (pag.hip) -------------------------------------------------------------------------------------------
// scales: one per model evaluation of the next call(s); layers: attn1 module names in config.py's spelling (self_attn_layer_names)
AGD_API int agd_pag_set(agd_ctx* c, const float* scales, int n, const char* const* layers, int n_layers) {
  API_CK(c, need_final(c));
  if (!scales || n < 1 || n_layers < 0 || (n_layers > 0 && !layers)) { agd_set_error("pag_set: %d scales, %d layers or a null argument", n, n_layers); return fail_ctx(c); }
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(scales[i]) || scales[i] < 0.f) { agd_set_error("pag_set: scale %d is %g (every scale a finite number >= 0)", i, (double)scales[i]); return fail_ctx(c); }
  std::unordered_set<std::string> pres;
  static const char kTail[] = "transformer_blocks.0.attn1";
  for (int k = 0; k < n_layers; ++k) {
    const std::string name = layers[k] ? layers[k] : "";
    const size_t tl = sizeof(kTail) - 1;
    bool ok = name.size() > tl && name.compare(name.size() - tl, tl, kTail) == 0;
    std::string pre;
    if (ok) {
      pre = "unet." + name.substr(0, name.size() - tl);                      // "unet.mid_block.attentions.0."
      auto it = c->xl_idx.find(pre + "transformer_blocks.0.attn2");
      ok = it != c->xl_idx.end() && !c->xl[it->second].cn;
    }
    if (!ok) { agd_set_error("pag_set: '%s' is not a self-attention layer of this UNet (e.g. mid_block.attentions.0.transformer_blocks.0.attn1)", name.c_str()); return fail_ctx(c); }
    pres.insert(pre);
  }
  c->pag_sched.assign(scales, scales + n); c->pag_layers.swap(pres);
  return 0;
}

AGD_API int agd_pag_clear(agd_ctx* c) {
  if (!c) { agd_set_error("pag_clear: null context"); return -1; }
  c->pag_sched.clear(); c->pag_layers.clear();
  return 0;
}

AGD_API int agd_pag_counts(agd_ctx* c, long long* walks, long long* layers) {
  if (!c || !walks || !layers) { agd_set_error("pag_counts: null argument"); return fail_ctx(c); }
  *walks = c->pag_counts[0]; *layers = c->pag_counts[1];
  return 0;
}

// The production kernels alone (the test seams), on device memory
AGD_API int agd_op_pag_v_rows(agd_ctx* c, const void* qkv, void* att, int M, int C, void* stream) {
  hipStream_t st = S(stream);                                       // (c may be null: it only keeps the error text)
  API_CK(c, launch_pag_v_rows((const bf16_t*)qkv, (bf16_t*)att, M, C, st));
  hipStreamSynchronize(st);
  return 0;
}
// ---- Semantic Guidance (sega.hip) -------------------------------------------------------------------------------------------------------
AGD_API int agd_sega_set(agd_ctx* c, const agd_sega_desc* d) {
  API_CK(c, need_final(c));
  if (!d || d->struct_size != (int)sizeof(agd_sega_desc)) { agd_set_error("sega_set: descriptor struct_size %d, this library has %zu", d ? d->struct_size : -1, sizeof(agd_sega_desc)); return fail_ctx(c); }
  const int K = d->concepts, n = d->n_evals;
  if (K < 1 || K > AGD_MAX_EDIT_CONCEPTS) { agd_set_error("sega_set: %d concepts (1 .. %d)", K, AGD_MAX_EDIT_CONCEPTS); return fail_ctx(c); }
  if (n < 1 || !d->coef || !d->q || !d->w_mom || !d->w_add || !d->add_mom) { agd_set_error("sega_set: %d evaluations or a null array", n); return fail_ctx(c); }
  if (!std::isfinite(d->mom_scale) || !std::isfinite(d->mom_beta)) { agd_set_error("sega_set: momentum scale %g, beta %g (finite numbers)", (double)d->mom_scale, (double)d->mom_beta); return fail_ctx(c); }
  for (int k = 0; k < K; ++k)
    if (!(d->q[k] >= 0.0 && d->q[k] <= 1.0)) { agd_set_error("sega_set: q[%d] is %g (a quantile in [0, 1])", k, d->q[k]); return fail_ctx(c); }
  for (long long j = 0; j < (long long)n * K; ++j)
    if (!std::isfinite(d->coef[j]) || !std::isfinite(d->w_mom[j]) || !std::isfinite(d->w_add[j])) {
      agd_set_error("sega_set: evaluation %lld, concept %lld: coef %g, w_mom %g, w_add %g (finite numbers)", j / K, j % K, (double)d->coef[j], (double)d->w_mom[j], (double)d->w_add[j]); return fail_ctx(c); }
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(d->add_mom[i])) { agd_set_error("sega_set: add_mom[%d] is %g (a finite number)", i, (double)d->add_mom[i]); return fail_ctx(c); }
  c->sega_coef.assign(d->coef, d->coef + (size_t)n * K); c->sega_wmom.assign(d->w_mom, d->w_mom + (size_t)n * K);
  c->sega_wadd.assign(d->w_add, d->w_add + (size_t)n * K); c->sega_addmom.assign(d->add_mom, d->add_mom + n); c->sega_q.assign(d->q, d->q + K);
  c->sega_K = K; c->sega_n = n; c->sega_mu = d->mom_scale; c->sega_beta = d->mom_beta;
  return 0;
}
AGD_API int agd_sega_clear(agd_ctx* c) {
  if (!c) { agd_set_error("sega_clear: null context"); return -1; }
  c->sega_K = 0; c->sega_n = 0; c->sega_coef.clear(); c->sega_wmom.clear(); c->sega_wadd.clear(); c->sega_addmom.clear(); c->sega_q.clear();
  return 0;
}
AGD_API int agd_sega_counts(agd_ctx* c, long long* walks, long long* folds) {
  if (!c || !walks || !folds) { agd_set_error("sega_counts: null argument"); return fail_ctx(c); }
  *walks = c->sega_counts[0]; *folds = c->sega_counts[1];
  return 0;
}
static int sega_op_scalars(const char* what, int K, int HW, const float* coef, const double* q, const float* w_mom, const float* w_add, SegaEvalP* p) {
  if (K < 1 || K > AGD_MAX_EDIT_CONCEPTS || HW < 1 || !coef) { agd_set_error("%s: %d concepts (1 .. %d), %d pixels or a null array", what, K, AGD_MAX_EDIT_CONCEPTS, HW); return -1; }
  *p = SegaEvalP{};
  for (int k = 0; k < K; ++k) {
    p->coef[k] = coef[k]; p->w_mom[k] = w_mom ? w_mom[k] : 0.f; p->w_add[k] = w_add ? w_add[k] : 0.f;
    if (q) {
      if (!(q[k] >= 0.0 && q[k] <= 1.0)) { agd_set_error("%s: q[%d] is %g (a quantile in [0, 1])", what, k, q[k]); return -1; }
      sega_rank(q[k], HW, &p->lo[k], &p->f[k]);
    }
  }
  return 0;
}
AGD_API int agd_op_sega_threshold(agd_ctx* c, const float* eps, int B, int K, int HW, const float* coef, const double* q, float* thr, void* stream) {
  hipStream_t st = S(stream);
  if (!q) { agd_set_error("op_sega_threshold: null q"); return fail_ctx(c); }
  SegaEvalP p; API_CK(c, sega_op_scalars("op_sega_threshold", K, HW, coef, q, nullptr, nullptr, &p));
  API_CK(c, launch_sega_threshold(eps, B, K, 4, HW, p, thr, st));
  return 0;
}
AGD_API int agd_op_sega_fold(agd_ctx* c, float* eps, float* m, const float* thr, int B, int K, int HW, const float* coef, const float* w_mom,
                             const float* w_add, float add_mom, float mom_scale, float mom_beta, void* stream) {
  hipStream_t st = S(stream);
  if (!w_mom || !w_add) { agd_set_error("op_sega_fold: null weights"); return fail_ctx(c); }
  SegaEvalP p; API_CK(c, sega_op_scalars("op_sega_fold", K, HW, coef, nullptr, w_mom, w_add, &p));
  API_CK(c, launch_sega_fold(eps, m, thr, B, K, 4, HW, p, mom_scale, mom_beta, add_mom, st));
  return 0;
}
AGD_API int agd_op_pag_fold(agd_ctx* c, float* eps, long long n, float p, void* stream) {
  hipStream_t st = S(stream);
  API_CK(c, launch_pag_fold(eps, n, p, st));
  hipStreamSynchronize(st);
  return 0;
}

// ---- DeepCache (deepcache.hip; the upstream DeepCacheSDHelper's uniform schedule [upstream-knowledge]) ---------------------------------
// One flag per model evaluation of the next fused loop (1 = the full walk, 0 = the shallow walk at `branch`), counted from evaluation 0 of the
// call whatever its scheduler.  flags[0] must be full; every flag 1 is the plain call.
AGD_API int agd_deepcache_set(agd_ctx* c, const int* full_flags, int n, int branch) {
  API_CK(c, need_final(c));
  if (!full_flags || n < 1) { agd_set_error("deepcache_set: %d flags or a null argument", n); return fail_ctx(c); }
  const int lpb = c->cfg.layers_per_block;
  if (branch < 0 || branch > lpb - 1) { agd_set_error("deepcache_set: branch %d (this UNet has branches 0 .. %d: the layers of its first down block)", branch, lpb - 1); return fail_ctx(c); }
  for (int i = 0; i < n; ++i)
    if (full_flags[i] != 0 && full_flags[i] != 1) { agd_set_error("deepcache_set: flag %d is %d (1 = full, 0 = shallow)", i, full_flags[i]); return fail_ctx(c); }
  if (full_flags[0] != 1) { agd_set_error("deepcache_set: flag 0 is shallow; the first evaluation of a call has no cache to read and must be full"); return fail_ctx(c); }
  c->dc_sched.assign(full_flags, full_flags + n); c->dc_branch = branch;
  deepcache_invalidate(c);
  return 0;
}

AGD_API int agd_deepcache_clear(agd_ctx* c) {
  if (!c) { agd_set_error("deepcache_clear: null context"); return -1; }
  c->dc_sched.clear(); c->dc_branch = 0;
  deepcache_invalidate(c);
  return 0;
}

AGD_API int agd_deepcache_counts(agd_ctx* c, long long* out) {
  if (!c || !out) { agd_set_error("deepcache_counts: null argument"); return fail_ctx(c); }
  out[0] = c->dc_counts[0]; out[1] = c->dc_counts[1];
  return 0;
}

// One evaluation of a DeepCache pair outside a loop (the test and tool seam; agd_unet_forward_hw's arguments).  shallow == 0: the plain forward
// plus the capture for `branch`; shallow == 1: the shallow walk on what the last such call captured for the same (rows, Lh, Lw, branch) --
// refused on the host when there is none, or when agd_set_context, a LoRA scale change, agd_freeu_set / _clear or agd_deepcache_clear came between.
AGD_API int agd_deepcache_forward_hw(agd_ctx* c, const float* sample, int rows, int Lh, int Lw, float timestep, int branch, int shallow, float* out, void* stream) {
  API_CK(c, need_final(c));
  API_CK(c, check_latent_hw(c, "deepcache_forward", Lh, Lw));
  if (!sample || !out || rows < 1 || (shallow != 0 && shallow != 1)) { agd_set_error("deepcache_forward: %d rows, shallow %d or a null argument", rows, shallow); return fail_ctx(c); }
  const int lpb = c->cfg.layers_per_block;
  if (branch < 0 || branch > lpb - 1) { agd_set_error("deepcache_forward: branch %d (this UNet has branches 0 .. %d: the layers of its first down block)", branch, lpb - 1); return fail_ctx(c); }
  CallCond cc; API_CK(c, resolve_cond(c, CALL_DC_FORWARD, 1, rows, Lh, Lw, &cc));
  if (shallow && (!c->dc_valid || c->dc_rows != rows || c->dc_Lh != Lh || c->dc_Lw != Lw || c->dc_b != branch)) {
    agd_set_error("deepcache_forward: a shallow evaluation of %d rows at %d x %d, branch %d, without a valid cache (%s)", rows, Lh, Lw, branch,
                  c->dc_valid ? "the captured one has another shape or branch" : "none was captured since the last invalidating call");
    return fail_ctx(c);
  }
  hipStream_t st = S(stream);
  API_CK(c, ensure_lat(c, rows, Lh, Lw));
  if (!shallow) API_CK(c, deepcache_reserve(c, rows, Lh, Lw));
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_prep_latents(sample, c->lat_bf16, rows, c->cfg.in_channels, Lh * Lw, 64, 1, 1.0f, st)); }
  EvalCond ec = cc.at(0); ec.dc = shallow ? DC_SHALLOW : DC_CAPTURE; ec.dc_branch = branch;
  API_CK(c, unet_walk(c, st, c->lat_bf16, rows, Lh, Lw, timestep, c->eps_nhwc, nullptr, false, 0, ec));
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_nchw_from_nhwc_f32(c->eps_nhwc, c->cfg.out_channels, out, rows, c->cfg.out_channels, Lh * Lw, st)); }
  return 0;
}

// The capture kernel alone (the test seam): two device regions of bytes0 / bytes1 bytes, copied as the walk's capture launch copies them
AGD_API int agd_op_deepcache_capture(agd_ctx* c, const void* src0, void* dst0, long long bytes0, const void* src1, void* dst1, long long bytes1, void* stream) {
  hipStream_t st = S(stream);
  API_CK(c, launch_deepcache_capture(src0, dst0, bytes0, src1, dst1, bytes1, st));
  hipStreamSynchronize(st);
  return 0;
}

// The production kernel alone (the test seam): eps [2 B][HW][ldc] fp32 on the device, as the step kernels read it -> factor [B] on the device
AGD_API int agd_op_guidance_rescale(agd_ctx* c, const float* eps, int ldc, int B, int C, int HW, float guidance, float phi, float* factor, void* stream) {
  hipStream_t st = S(stream);                                       // (c may be null: it only keeps the error text)
  API_CK(c, launch_guidance_factor(eps, ldc, B, C, HW, guidance, phi, factor, st));
  hipStreamSynchronize(st);
  return 0;
}

// ---------------------------------------------------------------------------------------
// Inpainting (diffusers StableDiffusionInpaintPipeline): the mask front end once per call, then a state the three fused loops read
// ---------------------------------------------------------------------------------------
AGD_API int agd_inpaint_prepare_hw(agd_ctx* c, const void* image, int image_f32, const void* mask, int mask_f32, int batch, int h, int w,
                                   float* image_out, float* masked_out, float* mask_lat_out, void* stream) {
  API_CK(c, need_final(c));
  if (!image || !mask) { agd_set_error("inpaint_prepare: null image or mask"); return fail_ctx(c); }
  const int f = 1 << (c->cfg.vae_n_levels - 1);
  ProfScope ps(c, S(stream), PC_ELEM, 0);
  API_CK(c, launch_inpaint_front(image, image_f32 != 0, mask, mask_f32 != 0, batch, h, w, f, image_out, masked_out, mask_lat_out, S(stream)));
  return 0;
}
AGD_API int agd_inpaint_prepare(agd_ctx* c, const void* image, int image_f32, const void* mask, int mask_f32, int batch, int side,
                                float* image_out, float* masked_out, float* mask_lat_out, void* stream) {
  return agd_inpaint_prepare_hw(c, image, image_f32, mask, mask_f32, batch, side, side, image_out, masked_out, mask_lat_out, stream);
}

AGD_API int agd_inpaint_set_hw(agd_ctx* c, const float* mask, int mask_channels, const float* cond, int cond_channels, const float* noise,
                               int batch, int Lh, int Lw, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  const int Cl = c->cfg.out_channels, Cin = c->cfg.in_channels;
  if (!mask || !cond || batch < 1 || Lh < 1 || Lw < 1) { agd_set_error("inpaint_set: null mask / cond, or batch %d latent size %d x %d", batch, Lh, Lw); return fail_ctx(c); }
  int mode = 0;
  if (Cin == Cl) {
    if (mask_channels != 1 || cond_channels != Cl || !noise)
      { agd_set_error("inpaint_set: the %d-channel UNet blends: needs a 1-channel mask, %d-channel image latents and the noise (got %d, %d%s)",
                      Cin, Cl, mask_channels, cond_channels, noise ? "" : ", no noise"); return fail_ctx(c); }
    mode = 2;
  } else {
    if (mask_channels < 1 || cond_channels < 1 || Cl + mask_channels + cond_channels != Cin || Cin > 64 || noise)
      { agd_set_error("inpaint_set: %d latent + %d mask + %d masked-latent channels do not make the UNet's %d input channels%s", Cl, mask_channels,
                      cond_channels, Cin, noise ? " (and a concatenating UNet takes no noise)" : ""); return fail_ctx(c); }
    mode = 1;
  }
  c->ip_mode = 0; c->ip_sched.clear();
  const size_t hw = (size_t)Lh * Lw, nm = (size_t)batch * mask_channels * hw, nc = (size_t)batch * cond_channels * hw;
  API_CK(c, c->ip_maskb.ensure(nm * 4)); API_CK(c, c->ip_condb.ensure(nc * 4));
  if (hipMemcpyAsync(c->ip_maskb.p, mask, nm * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(c->ip_condb.p, cond, nc * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { agd_set_error("inpaint_set: copy failed"); return fail_ctx(c); }
  if (noise) {
    API_CK(c, c->ip_noiseb.ensure(nc * 4));
    if (hipMemcpyAsync(c->ip_noiseb.p, noise, nc * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { agd_set_error("inpaint_set: copy failed"); return fail_ctx(c); }
  }
  c->ip_mode = mode; c->ip_B = batch; c->ip_Lh = Lh; c->ip_Lw = Lw; c->ip_Cm = mask_channels; c->ip_Cc = cond_channels;
  return 0;
}
AGD_API int agd_inpaint_set(agd_ctx* c, const float* mask, int mask_channels, const float* cond, int cond_channels, const float* noise,
                            int batch, int L, void* stream) {
  return agd_inpaint_set_hw(c, mask, mask_channels, cond, cond_channels, noise, batch, L, L, stream);
}

AGD_API int agd_inpaint_set_schedule(agd_ctx* c, const float* sa_sb, int n) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  if (c->ip_mode != 2) { agd_set_error("inpaint_set_schedule: no blend state (agd_inpaint_set on a UNet that takes the latent channels only)"); return fail_ctx(c); }
  if (n < 1 || !sa_sb) { agd_set_error("inpaint_set_schedule: %d entries", n); return fail_ctx(c); }
  for (int i = 0; i < 2 * n; ++i) if (!std::isfinite(sa_sb[i])) { agd_set_error("inpaint_set_schedule: entry %d is %g", i / 2, sa_sb[i]); return fail_ctx(c); }
  c->ip_sched.assign(sa_sb, sa_sb + 2 * n);
  return 0;
}

AGD_API int agd_inpaint_clear(agd_ctx* c) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  c->ip_mode = 0; c->ip_B = c->ip_Lh = c->ip_Lw = c->ip_Cm = c->ip_Cc = 0; c->ip_sched.clear();
  return 0;
}

// ---------------------------------------------------------------------------------------
// InstructPix2Pix (diffusers StableDiffusionInstructPix2PixPipeline): the image front end and VAE encode once per call, then a state the
// three fused loops read (run_ip2p_loop)
// ---------------------------------------------------------------------------------------
AGD_API int agd_ip2p_prepare_hw(agd_ctx* c, const void* image, int image_f32, int batch, int h, int w, float* latents_out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  const int lc = c->cfg.vae_latent_channels, f = 1 << (c->cfg.vae_n_levels - 1);
  if (!image || batch < 1) { agd_set_error("ip2p_prepare: null image or batch %d", batch); return fail_ctx(c); }
  if (h < 1 || w < 1 || h % f || h % 8 || w % f || w % 8) { agd_set_error("ip2p_prepare: size %d x %d (each side a positive multiple of %d)", h, w, f > 8 ? f : 8); return fail_ctx(c); }
  const int Lh = h / f, Lw = w / f;
  const size_t nl = (size_t)batch * lc * Lh * Lw;
  c->i2_on = false; c->i2_prep_B = 0;                              // the buffer below is the state's: a state set earlier ends here
  Tmp tmp;
  float* x = tmp.get<float>((size_t)batch * 3 * h * w); float* logvar = tmp.get<float>(nl);
  if (!x || !logvar) return fail_ctx(c);
  API_CK(c, c->i2_latb.ensure(nl * 4));
  { ProfScope ps(c, st, PC_ELEM, 0); API_CK(c, launch_ip2p_front(image, image_f32 != 0, batch, h, w, x, st)); }
  if (agd_vae_encode_hw(c, x, batch, h, w, c->i2_latb.as<float>(), logvar, stream) != 0) return -1;      // synchronizes the stream
  if (latents_out && hipMemcpyAsync(latents_out, c->i2_latb.p, nl * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { agd_set_error("ip2p_prepare: copy failed"); return fail_ctx(c); }
  c->i2_prep_B = batch; c->i2_prep_Lh = Lh; c->i2_prep_Lw = Lw;
  return 0;
}

AGD_API int agd_ip2p_set_hw(agd_ctx* c, const float* image_latents, int batch, int Lh, int Lw, float image_guidance, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  API_CK(c, ip2p_check_unet(c, "ip2p_set"));
  if (batch < 1 || Lh < 1 || Lw < 1) { agd_set_error("ip2p_set: batch %d latent size %d x %d", batch, Lh, Lw); return fail_ctx(c); }
  if (!std::isfinite(image_guidance)) { agd_set_error("ip2p_set: image guidance scale %g", image_guidance); return fail_ctx(c); }
  c->i2_on = false;
  if (!image_latents) {
    if (c->i2_prep_B != batch || c->i2_prep_Lh != Lh || c->i2_prep_Lw != Lw)
      { agd_set_error("ip2p_set: no image latents given and agd_ip2p_prepare_hw left %d images at %d x %d, not %d at %d x %d", c->i2_prep_B, c->i2_prep_Lh, c->i2_prep_Lw, batch, Lh, Lw); return fail_ctx(c); }
  } else {
    const size_t nl = (size_t)batch * c->cfg.vae_latent_channels * Lh * Lw;
    c->i2_prep_B = 0;
    API_CK(c, c->i2_latb.ensure(nl * 4));
    if (hipMemcpyAsync(c->i2_latb.p, image_latents, nl * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { agd_set_error("ip2p_set: copy failed"); return fail_ctx(c); }
  }
  c->i2_on = true; c->i2_B = batch; c->i2_Lh = Lh; c->i2_Lw = Lw; c->i2_scale = image_guidance;
  return 0;
}

AGD_API int agd_ip2p_clear(agd_ctx* c) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  c->i2_on = false; c->i2_B = c->i2_Lh = c->i2_Lw = 0; c->i2_scale = 1.f; c->i2_prep_B = 0;
  return 0;
}

// ---------------------------------------------------------------------------------------
// LoRA (diffusers load_lora_weights / cross_attention_kwargs={"scale": s}): low-rank updates of the UNet transformer blocks' linears and
// the text encoder's, merged into the raw matrices on the device (lora.hip) and every form derived from them rewritten in place
// (derive_tblock, fuse_clip_qkv) -- the denoise loop then runs the same kernels on the same buffers
// ---------------------------------------------------------------------------------------
static const char* kLoraUnetTargets[] = {"transformer_blocks.0.attn1.to_q.weight", "transformer_blocks.0.attn1.to_k.weight", "transformer_blocks.0.attn1.to_v.weight",
                                         "transformer_blocks.0.attn1.to_out.0.weight", "transformer_blocks.0.attn2.to_q.weight", "transformer_blocks.0.attn2.to_k.weight",
                                         "transformer_blocks.0.attn2.to_v.weight", "transformer_blocks.0.attn2.to_out.0.weight", "transformer_blocks.0.ff.net.0.proj.weight",
                                         "transformer_blocks.0.ff.net.2.weight", "proj_in.weight", "proj_out.weight"};
static const char* kLoraTextTargets[] = {"self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.out_proj.weight",
                                         "mlp.fc1.weight", "mlp.fc2.weight"};
static const char* kTextLayers = "text.encoder.layers.";

// the UNet transformer block (prefix) a target key belongs to; "" for a text-encoder target or no target at all
static std::string lora_block_of(agd_ctx* c, const std::string& key) {
  for (auto& pr : transformer_prefixes(c)) {
    if (pr.first.compare(0, 5, "unet.") != 0 || key.compare(0, pr.first.size(), pr.first) != 0) continue;
    for (const char* s : kLoraUnetTargets) if (key.compare(pr.first.size(), std::string::npos, s) == 0) return pr.first;
  }
  return "";
}
static bool lora_text_target(agd_ctx* c, const std::string& key) {
  for (int l = 0; l < c->cfg.text_layers; ++l) {
    const std::string L = std::string(kTextLayers) + std::to_string(l) + ".";
    if (key.compare(0, L.size(), L) != 0) continue;
    for (const char* s : kLoraTextTargets) if (key.compare(L.size(), std::string::npos, s) == 0) return true;
  }
  return false;
}

// rewrites, in place, every derived form of the blocks the LoRA touches (and the text encoder's fused q/k/v)
static int lora_rederive(agd_ctx* c) {
  bool text = false;
  for (const std::string& k : c->lora_keys) if (k.compare(0, 5, "text.") == 0) text = true;
  for (auto& pr : transformer_prefixes(c)) {
    if (pr.first.compare(0, 5, "unet.") != 0) continue;              // the ControlNet's blocks: never a LoRA target
    bool hit = false;
    for (const std::string& k : c->lora_keys) if (k.compare(0, pr.first.size(), pr.first) == 0) { hit = true; break; }
    if (hit) CK(derive_tblock(c, pr.first, pr.second, false, c->lora_scratch));
  }
  if (text) CK(fuse_clip_qkv(c, kTextLayers, c->cfg.text_layers, false));
  return 0;
}

AGD_API int agd_lora_add(agd_ctx* c, const char* target_key, const float* down, const float* up, int rank, float alpha) {
  API_CK(c, need_final(c));
  if (!target_key || !down || !up) { agd_set_error("agd_lora_add: null argument"); return fail_ctx(c); }
  const std::string k(target_key);
  for (const char* refused : {"controlnet.", "safety.", "vae."})
    if (k.compare(0, strlen(refused), refused) == 0) { agd_set_error("agd_lora_add: '%s': LoRA on the %.*s is not supported", target_key, (int)strlen(refused) - 1, refused); return fail_ctx(c); }
  const std::string block = lora_block_of(c, k);
  if (block.empty() && !lora_text_target(c, k)) { agd_set_error("agd_lora_add: '%s' is not a LoRA target (transformer-block linears, proj_in / proj_out, text-encoder q/k/v/out_proj/fc1/fc2)", target_key); return fail_ctx(c); }
  auto it = c->W.find(k);
  if (it == c->W.end()) { agd_set_error("agd_lora_add: no weight '%s' loaded", target_key); return fail_ctx(c); }
  const WMat& w = it->second;
  if (w.taps != 1) { agd_set_error("agd_lora_add: '%s' is not a linear / 1x1 matrix", target_key); return fail_ctx(c); }
  if (rank < 1 || rank > 4096 || !(alpha > 0.f) || !std::isfinite(alpha)) { agd_set_error("agd_lora_add: '%s': rank %d / alpha %g", target_key, rank, (double)alpha); return fail_ctx(c); }
  for (const std::string& o : c->lora_keys) if (o == k) { agd_set_error("agd_lora_add: '%s' already has a LoRA (one adapter at a time: agd_lora_clear first)", target_key); return fail_ctx(c); }
  // room the in-place re-derivation of this block needs ([4C][C] transposed W2 + [C][4C] Wp W2), held from here on: set_scale allocates nothing
  if (!block.empty()) {
    const WMat* q = getW(c, block + "transformer_blocks.0.attn1.to_q.weight"); if (!q) return fail_ctx(c);
    const size_t need = (size_t)8 * q->N * q->N;
    if (need > c->lora_scratch_n) {
      hipDeviceSynchronize(); dfree(c, c->lora_scratch); c->lora_scratch = nullptr; c->lora_scratch_n = 0;
      c->lora_scratch = dmalloc<bf16_t>(c, need); if (!c->lora_scratch) return fail_ctx(c);
      c->lora_scratch_n = need;
    }
  }
  LoraMergeD d{};
  d.N = w.N; d.Cin = w.Cin; d.Cpad = w.Cpad; d.r = rank; d.geglu = ends_with(k, "ff.net.0.proj.weight") ? 16 : 0; d.coef = alpha / (float)rank;
  d.dst = w.w;
  float* dn = dmalloc<float>(c, (size_t)rank * w.Cin); float* upd = dmalloc<float>(c, (size_t)w.N * rank); bf16_t* base = dmalloc<bf16_t>(c, (size_t)w.N * w.Cpad);
  if (!dn || !upd || !base) { dfree(c, dn); dfree(c, upd); dfree(c, base); return fail_ctx(c); }
  // the target's first touch: its base matrix is still what was loaded (a target takes one LoRA at a time)
  if (hipMemcpy(dn, down, (size_t)rank * w.Cin * 4, hipMemcpyDefault) != hipSuccess || hipMemcpy(upd, up, (size_t)w.N * rank * 4, hipMemcpyDefault) != hipSuccess ||
      hipMemcpy(base, w.w, (size_t)w.N * w.Cpad * 2, hipMemcpyDeviceToDevice) != hipSuccess) {
    dfree(c, dn); dfree(c, upd); dfree(c, base); agd_set_error("agd_lora_add: '%s': factor upload failed", target_key); return fail_ctx(c); }
  d.down = dn; d.up = upd; d.base = base; d.tile0 = c->lora_tiles;
  c->lora_keys.push_back(k); c->lora_d.push_back(d); c->lora_tiles += lora_merge_tiles(d.N, d.Cpad);
  API_CK(c, c->lora_descb.ensure(c->lora_d.size() * sizeof(LoraMergeD)));
  if (hipMemcpy(c->lora_descb.p, c->lora_d.data(), c->lora_d.size() * sizeof(LoraMergeD), hipMemcpyHostToDevice) != hipSuccess) { agd_set_error("agd_lora_add: descriptor upload failed"); return fail_ctx(c); }
  c->lora_dirty = true;                                // the new target is still at its base: the next set_scale merges everything
  return 0;
}

// s = 0 copies the base matrices back; a repeated s does nothing.  Synchronous: the merge and re-derivation run on the null stream after
// `stream` has drained.  Allocates nothing.
static int lora_apply(agd_ctx* c, float s, hipStream_t st) {
  if (hipStreamSynchronize(st) != hipSuccess) FAIL("lora: stream sync failed");
  c->lora_dirty = true;                                // until the whole rewrite has succeeded
  CK(launch_lora_merge(c->lora_descb.as<LoraMergeD>(), (int)c->lora_d.size(), c->lora_tiles, s, s == 0.f ? 1 : 0, 0));
  CK(lora_rederive(c));
  if (hipDeviceSynchronize() != hipSuccess) FAIL("lora: merge failed");
  c->lora_scale = s; c->lora_dirty = false; c->ctx_stale = true;
  deepcache_invalidate(c);
  if (c->ipa_B2 > 0) c->ipa_stale = true;               // K'' / V'' of the image tokens were built from the old to_q / to_out
  return 0;
}

AGD_API int agd_lora_set_scale(agd_ctx* c, float s, void* stream) {
  API_CK(c, need_final(c));
  if (!std::isfinite(s)) { agd_set_error("agd_lora_set_scale: scale %g", (double)s); return fail_ctx(c); }
  if (c->lora_d.empty()) { agd_set_error("agd_lora_set_scale: no LoRA loaded (agd_lora_add)"); return fail_ctx(c); }
  if (!c->lora_dirty && s == c->lora_scale) return 0;
  API_CK(c, lora_apply(c, s, S(stream)));
  return 0;
}

AGD_API int agd_lora_clear(agd_ctx* c) {
  API_CK(c, need_final(c));
  if (c->lora_d.empty()) return 0;
  API_CK(c, lora_apply(c, 0.f, 0));                    // the base matrices back, every derived form from them
  for (auto& d : c->lora_d) { dfree(c, (void*)d.down); dfree(c, (void*)d.up); dfree(c, (void*)d.base); }
  dfree(c, c->lora_scratch); c->lora_scratch = nullptr; c->lora_scratch_n = 0;
  c->lora_descb.release();
  c->lora_keys.clear(); c->lora_d.clear(); c->lora_tiles = 0; c->lora_scale = 0.f; c->lora_dirty = false;
  return 0;
}

AGD_API int agd_lora_count(agd_ctx* c) { return c ? (int)c->lora_d.size() : 0; }
AGD_API float agd_lora_scale(agd_ctx* c) { return c ? c->lora_scale : 0.f; }

// ---------------------------------------------------------------------------------------
// GLIGEN (diffusers PositionNet + GatedSelfAttentionDense + StableDiffusionGLIGENPipeline): the fusers run inside transformer()
// ---------------------------------------------------------------------------------------
AGD_API int agd_gligen_configure(agd_ctx* c, const agd_gligen_config* e) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  if (!e || e->struct_size != (int)sizeof(agd_gligen_config)) {
    agd_set_error("agd_gligen_configure: bad config (struct_size %d != %zu)", e ? e->struct_size : -1, sizeof(agd_gligen_config)); return fail_ctx(c); }
  if (c->finalized) { agd_set_error("agd_gligen_configure: call it before agd_finalize"); return fail_ctx(c); }
  if (e->max_objs < 1 || e->max_objs > 64) { agd_set_error("agd_gligen_configure: max_objs %d (1 .. 64: one key tile)", e->max_objs); return fail_ctx(c); }
  if (e->fourier_freqs < 1 || e->fourier_freqs > 64 || e->positive_len < 1 || e->positive_len > 8192) {
    agd_set_error("agd_gligen_configure: positive_len %d / fourier_freqs %d", e->positive_len, e->fourier_freqs); return fail_ctx(c); }
  c->glc = *e; c->gl_on = true;
  return 0;
}

// the PositionNet (Fourier embedding + null replacement + concat in one launch, then three igemm linears with SiLU between them) and, per
// fuser, linear -> norm1 -> K / V of the grounding rows.  Everything runs on the batch2 * max_objs object rows.
AGD_API int agd_gligen_set(agd_ctx* c, const float* boxes, const float* pos_emb, const float* masks, int batch2, void* stream) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  if (!c->gl_on) { agd_set_error("gligen_set: no GLIGEN UNet loaded (agd_gligen_configure before agd_finalize)"); return fail_ctx(c); }
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!boxes || !pos_emb || !masks || batch2 < 1) { agd_set_error("gligen_set: bad arguments (batch2 %d)", batch2); return fail_ctx(c); }
  if (c->ctx_B2 > 0 && batch2 != c->ctx_B2) { agd_set_error("gligen_set: %d rows, the context holds %d (agd_set_context)", batch2, c->ctx_B2); return fail_ctx(c); }
  const agd_gligen_config& e = c->glc;
  const int rows = batch2 * e.max_objs, Dc = c->cfg.cross_attention_dim, Pin = e.positive_len + 8 * e.fourier_freqs;
  c->gl_B2 = 0;                                                    // (unset until every block's K/V is written)
  c->arena.release(0);
  bf16_t* in = (bf16_t*)c->arena.alloc((size_t)rows * Pin * 2);
  bf16_t* h1 = (bf16_t*)c->arena.alloc((size_t)rows * 512 * 2); bf16_t* h2 = (bf16_t*)c->arena.alloc((size_t)rows * 512 * 2);
  if (!in || !h1 || !h2) return fail_ctx(c);
  API_CK(c, c->gl_objb.ensure((size_t)rows * Dc * 2));
  bf16_t* objs = c->gl_objb.as<bf16_t>();
  const std::string P = "unet.position_net.";
  { const float* np_ = getV(c, P + "null_positive_feature"); const float* nx = getV(c, P + "null_position_feature");
    if (!np_ || !nx) return fail_ctx(c);
    ProfScope ps(c, st, PC_ELEM, 0);
    API_CK(c, launch_gligen_posnet_input(boxes, pos_emb, masks, np_, nx, in, rows, e.positive_len, e.fourier_freqs, Pin, st)); }
  auto lin = [&](const std::string& k, const bf16_t* A, int K, bf16_t* out, int act) -> int {
    GETW(w, k + ".weight"); GETV(b, k + ".bias");
    GemmOpt o; o.bias = b; o.act = act;
    return run_conv(c, st, A, K, nullptr, 0, 1, 1, rows, *w, 1, out, o, c->zero_page);
  };
  API_CK(c, lin(P + "linears.0", in, Pin, h1, 1));
  API_CK(c, lin(P + "linears.2", h1, 512, h2, 1));
  API_CK(c, lin(P + "linears.4", h2, 512, objs, 0));
  for (Fuser& f : c->gl_f) {
    const size_t mk = c->arena.mark();
    const int C = f.C;
    const std::string t = f.pre + "transformer_blocks.0.fuser.";
    bf16_t* o = (bf16_t*)c->arena.alloc((size_t)rows * C * 2); bf16_t* n = (bf16_t*)c->arena.alloc((size_t)rows * C * 2);
    if (!o || !n) return fail_ctx(c);
    API_CK(c, lin(t + "linear", objs, Dc, o, 0));
    const float* g1 = getV(c, t + "norm1.weight"); const float* b1 = getV(c, t + "norm1.bias"); if (!g1 || !b1) return fail_ctx(c);
    { ProfScope ps(c, st, PC_LN, 0, 4.0 * rows * (double)C); API_CK(c, launch_layernorm(o, n, g1, b1, rows, C, 1e-5f, st)); }
    API_CK(c, f.gkvb.ensure((size_t)rows * 2 * C * 2));
    { GemmOpt go; API_CK(c, run_conv(c, st, n, C, nullptr, 0, 1, 1, rows, f.wkv, 1, f.gkvb.p, go, c->zero_page)); }
    c->arena.release(mk);
  }
  c->gl_B2 = batch2;
  return 0;
}

AGD_API int agd_gligen_set_schedule(agd_ctx* c, const int* flags, int n) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  if (n < 0 || (n > 0 && !flags)) { agd_set_error("gligen_set_schedule: %d flags", n); return fail_ctx(c); }
  if (n > 0 && !c->gl_on) { agd_set_error("gligen_set_schedule: no GLIGEN UNet loaded"); return fail_ctx(c); }
  c->gl_sched.assign(flags, flags + n);
  return 0;
}

AGD_API int agd_gligen_clear(agd_ctx* c) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  c->gl_sched.clear(); c->gl_B2 = 0; c->cur.grounded = false;
  return 0;
}

AGD_API int agd_gligen_objs(agd_ctx* c, float* out) {
  API_CK(c, need_final(c));
  if (!c->gl_on || c->gl_B2 < 1) { agd_set_error("gligen_objs: no grounding objects set (agd_gligen_set)"); return fail_ctx(c); }
  if (!out) { agd_set_error("gligen_objs: null out"); return fail_ctx(c); }
  if (hipDeviceSynchronize() != hipSuccess) { agd_set_error("gligen_objs: sync failed"); return fail_ctx(c); }   // (agd_gligen_set ran on the caller's stream)
  API_CK(c, launch_bf16_to_f32(c->gl_objb.as<bf16_t>(), out, (long long)c->gl_B2 * c->glc.max_objs * c->cfg.cross_attention_dim, 0));
  if (hipStreamSynchronize(0) != hipSuccess) { agd_set_error("gligen_objs: sync failed"); return fail_ctx(c); }
  return 0;
}

// a UNet transformer block as callers name it ("down_blocks.0.attentions.0", with or without "unet." and the trailing dot) -> its weight prefix
static std::string unet_block_prefix(const char* block_name) {
  std::string pre(block_name);
  if (pre.compare(0, 5, "unet.") != 0) pre = "unet." + pre;
  if (pre.back() != '.') pre += ".";
  return pre;
}
AGD_API int agd_gligen_fuser(agd_ctx* c, const char* block_name, const float* x, int batch2, int h, int w, float* out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!c->gl_on) { agd_set_error("gligen_fuser: no GLIGEN UNet loaded"); return fail_ctx(c); }
  if (!block_name || !x || !out || batch2 < 1 || h < 1 || w < 1) { agd_set_error("gligen_fuser: bad arguments"); return fail_ctx(c); }
  const std::string pre = unet_block_prefix(block_name);
  auto it = c->gl_idx.find(pre);
  if (it == c->gl_idx.end()) { agd_set_error("gligen_fuser: no fuser in block '%s'", block_name); return fail_ctx(c); }
  const Fuser& f = c->gl_f[it->second];
  const int HW = h * w, M = batch2 * HW, C = f.C;
  c->arena.release(0);
  bf16_t* hb = (bf16_t*)c->arena.alloc((size_t)M * C * 2); bf16_t* qkv = (bf16_t*)c->arena.alloc((size_t)M * 3 * C * 2);
  bf16_t* att = (bf16_t*)c->arena.alloc((size_t)M * C * 2);
  if (!hb || !qkv || !att) return fail_ctx(c);
  API_CK(c, launch_f32_to_bf16(x, hb, (long long)M * C, st));
  API_CK(c, fuser_rows(c, st, f, hb, batch2, HW, qkv, att, [&](const bf16_t* A, int K, const WMat& wm, const GemmOpt& o) {
    return run_conv(c, st, A, K, nullptr, 0, 1, 1, M, wm, 1, hb, o, c->zero_page); }));
  API_CK(c, launch_bf16_to_f32(hb, out, (long long)M * C, st));
  return 0;
}

// ---------------------------------------------------------------------------------------
// IP-Adapter (diffusers >= 0.24 load_ip_adapter / ip_adapter_image [upstream-knowledge]; ipadapter.hip): loaded into a finalised context like
// a LoRA; once per call the image projection and every attn2 layer's pre-multiplied image matrices, then two stages per transformer block
// (tb_ip_adapter_scores / tb_ip_adapter_add).  agd_attn_processor and agd_cross_attn (the seam) stay text-only.
// ---------------------------------------------------------------------------------------
static const char* kIpaProj[4] = {"image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias"};
static const char* kIpaK = "transformer_blocks.0.attn2.to_k_ip.weight";
static const char* kIpaV = "transformer_blocks.0.attn2.to_v_ip.weight";

AGD_API int agd_ip_adapter_begin(agd_ctx* c, int embed_dim, int n_tokens) {
  API_CK(c, need_final(c));
  if (c->ipa_on || c->ipa_loading) { agd_set_error("agd_ip_adapter_begin: an IP-Adapter is already loaded (one adapter at a time: agd_ip_adapter_unload first)"); return fail_ctx(c); }
  if (embed_dim < 1 || embed_dim > 8192 || n_tokens < 1 || n_tokens > 16) { agd_set_error("agd_ip_adapter_begin: embed_dim %d (1 .. 8192) / n_tokens %d (1 .. 16)", embed_dim, n_tokens); return fail_ctx(c); }
  for (auto& pr : transformer_prefixes(c)) {
    if (pr.first.compare(0, 5, "unet.") != 0) continue;            // the ControlNet's attn2 layers take no image branch
    auto it = c->xl_idx.find(pr.first + "transformer_blocks.0.attn2");
    if (it == c->xl_idx.end()) { agd_set_error("agd_ip_adapter_begin: cross-attn layer of %s not registered", pr.first.c_str()); ipa_release(c); return fail_ctx(c); }
    const XLayer& xl = c->xl[it->second];
    IpaLayer l; l.pre = pr.first; l.C = xl.C; l.heads = xl.heads; l.cols = (xl.heads * n_tokens + 15) / 16 * 16;
    if (l.cols > IPA_MAX_COLS || l.C % 8) {
      agd_set_error("agd_ip_adapter_begin: %s: %d heads x %d tokens (at most %d columns) / C %d", pr.first.c_str(), xl.heads, n_tokens, IPA_MAX_COLS, l.C); ipa_release(c); return fail_ctx(c); }
    c->ipa_idx[l.pre] = (int)c->ipa_l.size(); c->ipa_l.push_back(l);
  }
  c->ipa_E = embed_dim; c->ipa_nt = n_tokens; c->ipa_loading = true;
  return 0;
}

AGD_API int agd_ip_adapter_tensor(agd_ctx* c, const char* name, const void* ptr, int dtype, int ndim, const long long* shape) {
  API_CK(c, need_final(c));
  if (!c->ipa_loading) { agd_set_error("agd_ip_adapter_tensor: call agd_ip_adapter_begin first"); return fail_ctx(c); }
  if (!name || !ptr || !shape) { agd_set_error("agd_ip_adapter_tensor: null argument"); return fail_ctx(c); }
  if (dtype != 0) { agd_set_error("agd_ip_adapter_tensor: only float32 (dtype 0) supported"); return fail_ctx(c); }
  if (ndim < 1 || ndim > 2) { agd_set_error("agd_ip_adapter_tensor: '%s': ndim %d (1 or 2)", name, ndim); return fail_ctx(c); }
  std::string k(name);
  DBuf* dst = nullptr; bool mat = false;
  for (int i = 0; i < 4; ++i) if (k == kIpaProj[i]) { dst = i == 0 ? &c->ipa_projw : i == 1 ? &c->ipa_projb : i == 2 ? &c->ipa_ng : &c->ipa_nb; mat = i == 0; }
  if (!dst) {
    if (k.compare(0, 5, "unet.") != 0) k = "unet." + k;
    for (auto& l : c->ipa_l) {
      if (k == l.pre + kIpaK) { dst = &l.wk; mat = true; }
      else if (k == l.pre + kIpaV) { dst = &l.wv; mat = true; }
    }
  }
  if (!dst) { agd_set_error("agd_ip_adapter_tensor: '%s' is not an IP-Adapter tensor (image_proj.proj / norm, <unet block>.transformer_blocks.0.attn2.to_k_ip / to_v_ip.weight)", name); return fail_ctx(c); }
  if ((ndim == 2) != mat) { agd_set_error("agd_ip_adapter_tensor: '%s': ndim %d", name, ndim); return fail_ctx(c); }
  long long n = 1; for (int i = 0; i < ndim; ++i) { if (shape[i] < 1 || shape[i] > (1 << 24)) { agd_set_error("agd_ip_adapter_tensor: '%s': bad shape", name); return fail_ctx(c); } n *= shape[i]; }
  if (n > (1ll << 28)) { agd_set_error("agd_ip_adapter_tensor: '%s': %lld elements", name, n); return fail_ctx(c); }
  const size_t bytes = (size_t)n * 4;
  if (bytes > c->stage_bytes) {
    if (c->stage) hipFree(c->stage);
    if (hipMalloc((void**)&c->stage, bytes) != hipSuccess) { c->stage = nullptr; c->stage_bytes = 0; agd_set_error("stage alloc failed"); return fail_ctx(c); }
    c->stage_bytes = bytes;
  }
  if (hipMemcpy(c->stage, ptr, bytes, hipMemcpyDefault) != hipSuccess) { agd_set_error("copy of '%s' failed", name); return fail_ctx(c); }
  API_CK(c, dst->ensure(mat ? (size_t)n * 2 : bytes));
  if (mat) API_CK(c, launch_f32_to_bf16(c->stage, dst->as<bf16_t>(), n, 0));
  else if (hipMemcpy(dst->p, c->stage, bytes, hipMemcpyDeviceToDevice) != hipSuccess) { agd_set_error("copy of '%s' failed", name); return fail_ctx(c); }
  if (hipDeviceSynchronize() != hipSuccess) { agd_set_error("agd_ip_adapter_tensor: '%s': upload failed", name); return fail_ctx(c); }
  c->ipa_t[k] = std::vector<long long>(shape, shape + ndim);
  return 0;
}

AGD_API int agd_ip_adapter_commit(agd_ctx* c) {
  API_CK(c, need_final(c));
  if (!c->ipa_loading) { agd_set_error("agd_ip_adapter_commit: call agd_ip_adapter_begin first"); return fail_ctx(c); }
  const long long Dc = c->cfg.cross_attention_dim, E = c->ipa_E, nt = c->ipa_nt;
  std::string bad;
  auto want = [&](const std::string& k, std::vector<long long> shp) {
    auto it = c->ipa_t.find(k);
    if (it == c->ipa_t.end()) { bad += (bad.empty() ? "" : ", ") + k + " (missing)"; return; }
    if (it->second != shp) {
      std::string g, w; for (long long v : it->second) g += (g.empty() ? "" : ", ") + std::to_string(v); for (long long v : shp) w += (w.empty() ? "" : ", ") + std::to_string(v);
      bad += (bad.empty() ? "" : ", ") + k + " ([" + g + "], expected [" + w + "])";
    }
  };
  want(kIpaProj[0], {nt * Dc, E}); want(kIpaProj[1], {nt * Dc}); want(kIpaProj[2], {Dc}); want(kIpaProj[3], {Dc});
  for (auto& l : c->ipa_l) { want(l.pre + kIpaK, {l.C, Dc}); want(l.pre + kIpaV, {l.C, Dc}); }
  if (!bad.empty()) { agd_set_error("agd_ip_adapter_commit: %s", bad.c_str()); return fail_ctx(c); }
  c->ipa_loading = false; c->ipa_on = true;
  return 0;
}

AGD_API int agd_ip_adapter_unload(agd_ctx* c) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  hipSetDevice(c->device);
  if (hipDeviceSynchronize() != hipSuccess) { agd_set_error("agd_ip_adapter_unload: sync failed"); return fail_ctx(c); }
  ipa_release(c);
  return 0;
}

AGD_API int agd_ip_adapter_set(agd_ctx* c, const float* image_embeds, int batch2, float scale, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!c->ipa_on) { agd_set_error("ip_adapter_set: no IP-Adapter loaded (agd_ip_adapter_begin .. agd_ip_adapter_commit)"); return fail_ctx(c); }
  if (!image_embeds || batch2 < 1 || batch2 > 4096) { agd_set_error("ip_adapter_set: bad arguments (batch2 %d)", batch2); return fail_ctx(c); }
  if (!std::isfinite(scale)) { agd_set_error("ip_adapter_set: scale %g", (double)scale); return fail_ctx(c); }
  if (c->lora_dirty) { agd_set_error("ip_adapter_set: a LoRA was added and not merged yet (agd_lora_set_scale first)"); return fail_ctx(c); }
  const int Dc = c->cfg.cross_attention_dim, E = c->ipa_E, nt = c->ipa_nt, rows = batch2 * nt;
  c->ipa_B2 = 0;                                                   // (unset until every layer's matrices are written)
  int Cmax = 0; for (auto& l : c->ipa_l) Cmax = std::max(Cmax, l.C);
  API_CK(c, c->ipa_embb.ensure((size_t)batch2 * E * 4)); API_CK(c, c->ipa_tokb.ensure((size_t)rows * Dc * 4));
  API_CK(c, c->ipa_kipb.ensure((size_t)rows * Cmax * 4)); API_CK(c, c->ipa_vipb.ensure((size_t)rows * Cmax * 4)); API_CK(c, c->ipa_wqbb.ensure((size_t)Cmax * 4));
  if (hipMemcpyAsync(c->ipa_embb.p, image_embeds, (size_t)batch2 * E * 4, hipMemcpyDefault, st) != hipSuccess) { agd_set_error("ip_adapter_set: copy of the embeddings failed"); return fail_ctx(c); }
  float* tok = c->ipa_tokb.as<float>();
  { ProfScope ps(c, st, PC_OTHER, 2.0 * batch2 * (double)nt * Dc * E);
    API_CK(c, launch_ipa_linear(c->ipa_embb.as<float>(), c->ipa_projw.as<bf16_t>(), c->ipa_projb.as<float>(), tok, batch2, nt * Dc, E, st));
    API_CK(c, launch_ipa_layernorm(tok, c->ipa_ng.as<float>(), c->ipa_nb.as<float>(), rows, Dc, 1e-5f, st)); }
  for (auto& l : c->ipa_l) {
    const std::string t = l.pre + "transformer_blocks.0.";
    const WMat* wq = getW(c, t + "attn2.to_q.weight"); const WMat* wo = getW(c, t + "attn2.to_out.0.weight");
    const float* g2 = getV(c, t + "norm2.weight"); const float* b2 = getV(c, t + "norm2.bias");
    if (!wq || !wo || !g2 || !b2) return fail_ctx(c);
    const int C = l.C;
    if (wq->taps != 1 || wq->N != C || wq->Cpad != C || wo->taps != 1 || wo->N != C || wo->Cpad != C) {
      agd_set_error("ip_adapter_set: %s: to_q / to_out are not [%d][%d]", t.c_str(), C, C); return fail_ctx(c); }
    API_CK(c, l.kppb.ensure((size_t)batch2 * l.cols * C * 2)); API_CK(c, l.vppb.ensure((size_t)batch2 * l.cols * C * 2)); API_CK(c, l.csbsb.ensure((size_t)2 * batch2 * l.cols * 4));
    ProfScope ps(c, st, PC_OTHER, 4.0 * rows * (double)C * Dc + 4.0 * batch2 * (double)l.cols * C * (C / l.heads));
    API_CK(c, launch_ipa_linear(tok, l.wk.as<bf16_t>(), nullptr, c->ipa_kipb.as<float>(), rows, C, Dc, st));
    API_CK(c, launch_ipa_linear(tok, l.wv.as<bf16_t>(), nullptr, c->ipa_vipb.as<float>(), rows, C, Dc, st));
    API_CK(c, launch_matvec_bf16(wq->w, b2, c->ipa_wqbb.as<float>(), C, C, st));           // (Wq beta2)[(h,d)] from the merged to_q
    IpaPremulP pm{}; pm.kip = c->ipa_kipb.as<float>(); pm.vip = c->ipa_vipb.as<float>(); pm.wq = wq->w; pm.wo = wo->w; pm.gamma = g2; pm.wqb = c->ipa_wqbb.as<float>();
    pm.B = batch2; pm.C = C; pm.H = l.heads; pm.nt = nt; pm.colsP = l.cols; pm.scale = 1.0f / sqrtf((float)(C / l.heads));
    pm.kpp = l.kppb.as<bf16_t>(); pm.cs = l.csbsb.as<float>(); pm.bs = pm.cs + (size_t)batch2 * l.cols; pm.vpp = l.vppb.as<bf16_t>();
    API_CK(c, launch_ipa_premul(pm, st));
  }
  c->ipa_B2 = batch2; c->ipa_scale = scale; c->ipa_stale = false;
  return 0;
}

AGD_API int agd_ip_adapter_clear(agd_ctx* c) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  c->ipa_B2 = 0; c->ipa_scale = 0.f; c->ipa_stale = c->cur.ipa = false; c->ipa_counts[0] = c->ipa_counts[1] = 0;
  return 0;
}

AGD_API int agd_ip_adapter_tokens(agd_ctx* c, float* out) {
  API_CK(c, need_final(c));
  if (!c->ipa_on || c->ipa_B2 < 1) { agd_set_error("ip_adapter_tokens: no image tokens set (agd_ip_adapter_set)"); return fail_ctx(c); }
  if (!out) { agd_set_error("ip_adapter_tokens: null out"); return fail_ctx(c); }
  if (hipDeviceSynchronize() != hipSuccess) { agd_set_error("ip_adapter_tokens: sync failed"); return fail_ctx(c); }   // (agd_ip_adapter_set ran on the caller's stream)
  if (hipMemcpy(out, c->ipa_tokb.p, (size_t)c->ipa_B2 * c->ipa_nt * c->cfg.cross_attention_dim * 4, hipMemcpyDefault) != hipSuccess) {
    agd_set_error("ip_adapter_tokens: copy failed"); return fail_ctx(c); }
  return 0;
}

AGD_API int agd_ip_adapter_block(agd_ctx* c, const char* block_name, const float* x, int batch2, int h, int w, float* out, void* stream) {
  API_CK(c, need_final(c));
  hipStream_t st = S(stream);
  if (!c->ipa_on || c->ipa_B2 < 1) { agd_set_error("ip_adapter_block: no image tokens set (agd_ip_adapter_set)"); return fail_ctx(c); }
  if (!block_name || !x || !out || batch2 < 1 || h < 1 || w < 1) { agd_set_error("ip_adapter_block: bad arguments"); return fail_ctx(c); }
  if (c->ipa_stale) { agd_set_error("ip_adapter_block: a LoRA scale change rewrote to_q / to_out after the image products were built (call agd_ip_adapter_set again)"); return fail_ctx(c); }
  const std::string pre = unet_block_prefix(block_name);
  auto it = c->ipa_idx.find(pre);
  if (it == c->ipa_idx.end()) { agd_set_error("ip_adapter_block: no attn2 layer in block '%s'", block_name); return fail_ctx(c); }
  const IpaLayer& l = c->ipa_l[it->second];
  const long long HW = (long long)h * w, M = batch2 * HW;
  if (M >= (1ll << 28)) { agd_set_error("ip_adapter_block: %d rows of %d x %d", batch2, h, w); return fail_ctx(c); }
  c->arena.release(0);
  bf16_t* hb = (bf16_t*)c->arena.alloc((size_t)M * l.C * 2); bf16_t* P = (bf16_t*)c->arena.alloc((size_t)M * l.cols * 2);
  if (!hb || !P) return fail_ctx(c);
  API_CK(c, launch_f32_to_bf16(x, hb, M * l.C, st));
  API_CK(c, ipa_scores_rows(c, st, l, hb, batch2, (int)HW, P));
  API_CK(c, ipa_add_rows(c, st, l, hb, batch2, (int)HW, P));
  API_CK(c, launch_bf16_to_f32(hb, out, M * l.C, st));
  return 0;
}

AGD_API int agd_ip_adapter_counts(agd_ctx* c, long long* counts) {
  if (!c || !counts) { agd_set_error("ip_adapter_counts: null argument"); return fail_ctx(c); }
  counts[0] = c->ipa_counts[0]; counts[1] = c->ipa_counts[1];
  return 0;
}

// ---------------------------------------------------------------------------------------
// The IP-Adapter's image encoder (transformers CLIPVisionModelWithProjection: image_embeds = visual_projection(post_layernorm(CLS))):
// the safety checker's vision path (vision_embed) under its own weights, loaded after agd_finalize.  Head dim 64 or 80 (OpenCLIP ViT-H/14).
// ---------------------------------------------------------------------------------------
AGD_API int agd_image_encoder_begin(agd_ctx* c, const agd_vision_config* v) {
  API_CK(c, need_final(c));
  if (!v || v->struct_size != (int)sizeof(agd_vision_config)) {
    agd_set_error("agd_image_encoder_begin: bad config (struct_size %d != %zu)", v ? v->struct_size : -1, sizeof(agd_vision_config)); return fail_ctx(c); }
  if (c->ienc_state != 0) { agd_set_error("agd_image_encoder_begin: an image encoder is already loaded or half loaded (one per context: agd_image_encoder_unload first)"); return fail_ctx(c); }
  API_CK(c, check_vision_config(v, "agd_image_encoder_begin"));
  const int d = v->hidden / v->heads;
  if (d != 64 && d != 80) { agd_set_error("agd_image_encoder_begin: hidden %d / heads %d: head dim %d unsupported (64 or 80)", v->hidden, v->heads, d); return fail_ctx(c); }
  if (v->n_special != 0 || v->n_concepts != 0) { agd_set_error("agd_image_encoder_begin: an image encoder has no concept rows (n_special = n_concepts = 0)"); return fail_ctx(c); }
  c->ienc = *v; c->ienc_state = 1;
  return 0;
}
AGD_API int agd_image_encoder_tensor(agd_ctx* c, const char* name, const void* ptr, int dtype, int ndim, const long long* shape) {
  API_CK(c, need_final(c));
  if (c->ienc_state != 1) { agd_set_error("agd_image_encoder_tensor: call agd_image_encoder_begin first (and not after agd_image_encoder_commit)"); return fail_ctx(c); }
  if (!name || strncmp(name, "image_encoder.", 14) != 0) { agd_set_error("agd_image_encoder_tensor: '%s' does not start with \"image_encoder.\"", name ? name : "(null)"); return fail_ctx(c); }
  if (ndim < 1 || ndim > 4) { agd_set_error("agd_image_encoder_tensor: '%s': ndim %d", name, ndim); return fail_ctx(c); }
  if (c->W.count(name) || c->V.count(name)) { agd_set_error("agd_image_encoder_tensor: '%s' was loaded already", name); return fail_ctx(c); }
  return agd_load_tensor(c, name, ptr, dtype, ndim, shape);
}
AGD_API int agd_image_encoder_commit(agd_ctx* c) {
  API_CK(c, need_final(c));
  if (c->ienc_state != 1) { agd_set_error("agd_image_encoder_commit: call agd_image_encoder_begin first"); return fail_ctx(c); }
  API_CK(c, finalize_vision(c, image_tower(c)));
  if (hipDeviceSynchronize() != hipSuccess) { agd_set_error("agd_image_encoder_commit: sync failed"); return fail_ctx(c); }
  c->ienc_state = 2;
  return 0;
}
// frees every "image_encoder.*" tensor (the loaded ones, the fused q/k/v and the patch matrix): after a failed load, so that it can be tried
// again, or to drop a committed encoder
AGD_API int agd_image_encoder_unload(agd_ctx* c) {
  if (!c) { agd_set_error("null ctx"); return -1; }
  hipSetDevice(c->device);
  if (hipDeviceSynchronize() != hipSuccess) { agd_set_error("agd_image_encoder_unload: sync failed"); return fail_ctx(c); }
  std::vector<void*> gone;
  for (auto it = c->W.begin(); it != c->W.end();)
    if (it->first.compare(0, 14, "image_encoder.") == 0) { gone.push_back(it->second.w); gone.push_back(it->second.wfrag); it = c->W.erase(it); } else ++it;
  for (auto it = c->V.begin(); it != c->V.end();)
    if (it->first.compare(0, 14, "image_encoder.") == 0) { gone.push_back(it->second); c->Vn.erase(it->first); it = c->V.erase(it); } else ++it;
  for (void* p : gone) {
    auto o = std::find(c->owned.begin(), c->owned.end(), p);
    if (o != c->owned.end()) { hipFree(p); c->owned.erase(o); }
  }
  c->ienc = agd_vision_config{}; c->ienc_state = 0;
  return 0;
}
AGD_API int agd_image_embeds(agd_ctx* c, const unsigned char* images, int batch, int h, int w, float* out, void* stream) {
  API_CK(c, need_final(c));
  if (c->ienc_state != 2) { agd_set_error("image_embeds: no image encoder loaded (agd_image_encoder_begin .. agd_image_encoder_commit)"); return fail_ctx(c); }
  if (batch < 1 || h < 1 || w < 1 || !images || !out) { agd_set_error("image_embeds: batch %d size %d x %d / null buffer", batch, h, w); return fail_ctx(c); }
  return vision_embed(c, S(stream), image_tower(c), images, batch, h, w, nullptr, nullptr, 0, nullptr, out);
}
