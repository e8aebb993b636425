/* agenda_hip.h -- C ABI of libagenda_hip.so: the MI355X (gfx950) implementation of the AGenDA
 * data-generation hot path (Stable-Diffusion UNet denoise loop + DAAM cross-attention heat maps +
 * VAE decode).
 *
 * The reference (humansensinglab/AGenDA) has no FFI: the path sits behind three PYTHON surfaces
 * (SURVEY.md §8b).  Each entry point below names the reference interface it stands under:
 *   - diffusers `StableDiffusionPipeline.__call__`   reference data_generation/data_generation.py:59
 *   - `daam.trace(pipe)` / `compute_global_heat_map`  reference data_generation/data_generation.py:57,64
 *   - diffusers attention-processor protocol          reference data_generation/hook.py:83-122
 * The Python shim in agenda_amd/ binds these with ctypes.
 *
 * Conventions: plain pointers + sizes, no torch types.  Every call returns 0 on success, nonzero on
 * error (message via agd_last_error).  Tensors are caller-owned DEVICE pointers unless noted; the
 * library owns only its weights, workspace and heat-map accumulators.  `stream` is a hipStream_t
 * (NULL = default stream); calls are stream-ordered with no hidden syncs except where noted.
 * One ctx per GPU per process; calls on one ctx must be serialised by the caller.
 */
/* Image sizes: every entry point that takes one latent side (or pixel side) has a `_hw` form taking (height, width); the one-side
 * form is that call with h == w.  Rectangular latents must halve exactly at every UNet level (a multiple of 64 pixels per axis). */
#ifndef AGENDA_HIP_H
#define AGENDA_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct agd_ctx agd_ctx;

#define AGD_MAX_LEVELS 8

/* Architecture description == the fields of unet/config.json + vae/config.json that
 * `StableDiffusionPipeline.from_pretrained` (data_generation.py:30) reads. */
typedef struct agd_config {
  int struct_size;                 /* sizeof(agd_config), ABI guard */
  int in_channels, out_channels, n_levels;
  int block_out_channels[AGD_MAX_LEVELS];
  int down_cross[AGD_MAX_LEVELS];  /* 1 = CrossAttnDownBlock2D at this level */
  int num_heads[AGD_MAX_LEVELS];
  int layers_per_block, cross_attention_dim, use_linear_projection, norm_num_groups;
  int vae_latent_channels, vae_out_channels, vae_n_levels;
  int vae_block_out_channels[AGD_MAX_LEVELS];
  int vae_layers_per_block, vae_norm_num_groups;
  float vae_scaling_factor;
  int max_tokens;                  /* 77 */
  int prediction_type;             /* 0 epsilon, 1 v_prediction */
  long long workspace_bytes;       /* activation arena; 0 = default (8 GiB) */
  /* CLIP text encoder (`pipeline.text_encoder`, data_generation.py:47-52); text_layers == 0: none loaded */
  int text_hidden, text_layers, text_heads, text_intermediate, text_vocab, text_max_pos;
  int text_act;                    /* 0 quick_gelu (SD-1.x CLIP ViT-L/14), 1 gelu (OpenCLIP, SD-2.x) */
  float text_eps;
} agd_config;

/* ---- lifetime ------------------------------------------------------------------------- */
agd_ctx* agd_create(int device_id, const agd_config* cfg);
void agd_destroy(agd_ctx* ctx);
const char* agd_last_error(agd_ctx* ctx);          /* ctx may be NULL (last global error) */

/* ---- weights: names are the diffusers state-dict keys, UNet keys prefixed "unet.", VAE keys
 * "vae." (`pipeline.unet` / `pipeline.vae`, data_generation.py:30).  `ptr` may be host or
 * device memory; dtype 0 = float32.  Synchronous. */
int agd_load_tensor(agd_ctx* ctx, const char* name, const void* ptr, int dtype, int ndim, const long long* shape);
int agd_finalize(agd_ctx* ctx);                    /* after the last agd_load_tensor */

/* ---- text context: `encoder_hidden_states` [2B, T, ctx_dim] fp32, rows [0,B) unconditional,
 * [B,2B) conditional (CFG order assumed by hook.py:48-49).  Projects K/V of every attn2 once.
 * T <= AGD_MAX_CONTEXT_TOKENS.  Up to 96 tokens everything runs as it always has.  Beyond (long and weighted prompts: 152 / 227 / 302 rows)
 * attn2 runs to_q, attention, to_out as separate launches, DAAM records per-head rows at every level through csrc/attention_long.hip --
 * call agd_record_reset AFTER agd_set_context, rec_tokens up to T -- and the fused loops (img2img, LoRA, FreeU, guidance_rescale, PAG,
 * DeepCache, rectangular sizes included), agd_unet_forward_hw and agd_deepcache_forward_hw take it.  Refused by name with such a context: the
 * hook.py recorder, recording through agd_attn_processor / agd_cross_attn, agd_attn_processor_backward, agd_unet_forward_ts*,
 * agd_denoise_panorama, agd_denoise_regions, and a set ControlNet, GLIGEN, inpainting, InstructPix2Pix, T2I-Adapter or IP-Adapter state. */
#define AGD_MAX_CONTEXT_TOKENS 320
int agd_set_context(agd_ctx* ctx, const float* ctx_emb, int batch2, int tokens, void* stream);

/* ---- `text_encoder(input_ids)[0]` (CLIPTextModel.last_hidden_state): ids int32 [B, T] (host or device) ->
 * out fp32 [B, T, text_hidden].  Weights: "text." + transformers state-dict key.  Rows of the token embedding can
 * be (over)written -- the learned-token injection of data_generation.py:45-52 -- ids up to text_vocab + 255. */
int agd_text_encode(agd_ctx* ctx, const int* input_ids, int batch, int tokens, float* out, void* stream);
int agd_text_set_embedding_row(agd_ctx* ctx, int token_id, const float* row);

/* ---- the safety checker (`pipeline.safety_checker`, a StableDiffusionSafetyChecker: the CLIP ViT vision tower + visual_projection +
 * cosine_distance against its concept embeddings; data_generation.py:59-62 skips the images it flags).  Configured by
 * agd_safety_configure BEFORE agd_finalize; weights through agd_load_tensor as "safety." + diffusers state-dict key
 * ("safety.vision_model.vision_model.…", "safety.visual_projection.weight", "safety.concept_embeds", "safety.special_care_embeds").
 * agd_finalize fuses q/k/v per layer, zero-pads the patch matrix and L2-normalises the concept rows. */
typedef struct agd_vision_config {
  int struct_size;                 /* sizeof(agd_vision_config), ABI guard */
  int hidden, layers, heads, intermediate, image_size, patch_size, projection_dim;
  int n_special, n_concepts;       /* rows of special_care_embeds / concept_embeds */
  int act;                         /* 0 quick_gelu, 1 gelu */
  float eps;
  float mean[3], std[3];           /* CLIPImageProcessor image_mean / image_std (rescale 1/255 before them) */
} agd_vision_config;
int agd_safety_configure(agd_ctx* ctx, const agd_vision_config* vcfg);
/* images: uint8 [B,S,S,3] DEVICE (the decoded images) -> PIL-bicubic resize to image_size, rescale, normalize, the tower:
 * cos_out fp32 [B, n_special + n_concepts] (device; special-care cosines first); pixels_out (may be NULL) fp32 [B,3,image_size,image_size]
 * = the processor's pixel_values.  Stream-ordered; leaves the recorder accumulators, the context and the scheduler state untouched. */
int agd_safety_scores(agd_ctx* ctx, const unsigned char* images, int batch, int side, float* cos_out, float* pixels_out, void* stream);
/* the same on [batch][h][w][3] images of any size: CLIPImageProcessor's shortest-edge resize to image_size, then the center crop */
int agd_safety_scores_hw(agd_ctx* ctx, const unsigned char* images, int batch, int h, int w, float* cos_out, float* pixels_out, void* stream);

/* ---- ControlNet (diffusers ControlNetModel, SD-1.x: the UNet's down blocks + mid block, a conditioning embedding and 1x1 zero convs).
 * Configured by agd_controlnet_configure BEFORE agd_finalize; weights through agd_load_tensor as "controlnet." + diffusers state-dict key.
 * Its block layout, heads and cross-attention width are the UNet's (the host refuses anything else).  Its transformer layers are never
 * recorded (DAAM and the hook.py recorder see the UNet's layers only). */
#define AGD_CN_MAX_EMB 8
typedef struct agd_controlnet_config {
  int struct_size;                 /* sizeof(agd_controlnet_config), ABI guard */
  int n_emb;                       /* len(conditioning_embedding_out_channels), 2 .. AGD_CN_MAX_EMB */
  int emb_channels[AGD_CN_MAX_EMB];
  int bgr;                         /* controlnet_conditioning_channel_order == "bgr": the image's channels are flipped first */
} agd_controlnet_config;
int agd_controlnet_configure(agd_ctx* ctx, const agd_controlnet_config* cncfg);
/* the conditioning image cond fp32 [batch,3,S,S] (device) in [0,1] -> the embedding, computed once and kept for batch * repeat UNet rows
 * (repeat 2: [cond; cond], the CFG doubling); S = latent side << (n_emb - 1). */
int agd_controlnet_set_cond(agd_ctx* ctx, const float* cond, int batch, int side, int repeat, void* stream);
int agd_controlnet_set_cond_hw(agd_ctx* ctx, const float* cond, int batch, int h, int w, int repeat, void* stream);   /* [batch][3][h][w] */
/* per-model-evaluation conditioning scales (controlnet_conditioning_scale x the guidance window), host array of n floats, consumed by the
 * next agd_denoise / agd_denoise_plms / agd_denoise_dpm (n must equal its evaluation count) or agd_unet_forward (n = 1).  A scale of
 * exactly 0 skips the ControlNet for that evaluation.  n = 0 clears the schedule: the UNet runs alone. */
int agd_controlnet_set_schedule(agd_ctx* ctx, const float* scales, int n);
/* one ControlNet forward: the 13 (SD-1.x) scaled residuals, down residuals in res-sample order then the mid residual, written back to back
 * into out fp32 (device) per residual as [batch2][C][h][w] (nhwc = 0) or [batch2][h][w][C] (nhwc = 1); returns the float count in *n_out.
 * out = NULL: only the count.  The conditioning embedding must be set for batch2 rows. */
int agd_controlnet_residuals(agd_ctx* ctx, const float* sample, int batch2, int latent_side, float timestep, float scale, int nhwc,
                             float* out, long long* n_out, void* stream);
int agd_controlnet_residuals_hw(agd_ctx* ctx, const float* sample, int batch2, int latent_h, int latent_w, float timestep, float scale, int nhwc,
                                float* out, long long* n_out, void* stream);

/* ---- inpainting (diffusers StableDiffusionInpaintPipeline).  A 9-channel UNet (in_channels = latent + 1 + latent) reads
 * latents | mask | masked-image latents every evaluation; a UNet that takes the latent channels only is blended after every scheduler
 * step instead.  The state is set once per call and cleared explicitly; without it every loop runs plain txt2img. */
/* the front end, once per call, device pointers: image uint8 NHWC [batch,S,S,3] (image_f32 = 0: x / 255, then 2 x - 1) or fp32 NCHW
 * [batch,3,S,S] already in [-1,1] (image_f32 = 1); mask uint8 [batch,S,S] (mask_f32 = 0: / 255) or fp32 [batch,S,S] in [0,1], binarized
 * (m < 0.5 -> 0, else 1).  Writes, each may be NULL: image_out fp32 NCHW [batch,3,S,S], masked_out = image * (m < 0.5), mask_lat_out fp32
 * [batch,1,L,L] with L = S / the VAE's downscale f and latent pixel (i, j) = mask pixel (f i, f j). */
int agd_inpaint_prepare(agd_ctx* ctx, const void* image, int image_f32, const void* mask, int mask_f32, int batch, int side,
                        float* image_out, float* masked_out, float* mask_lat_out, void* stream);
int agd_inpaint_prepare_hw(agd_ctx* ctx, const void* image, int image_f32, const void* mask, int mask_f32, int batch, int h, int w,
                           float* image_out, float* masked_out, float* mask_lat_out, void* stream);   /* mask_lat [batch][1][h/8][w/8] */
/* the state, copied from device fp32 NCHW tensors of `batch` images (both CFG halves read them): mask [batch,mask_channels,L,L] and cond
 * [batch,cond_channels,L,L].  A 9-channel UNet: cond = the masked-image latents, latent + mask_channels + cond_channels must equal
 * in_channels, noise = NULL.  A UNet of latent input channels: cond = the image latents, mask_channels = 1, noise [batch,latent,L,L] (the
 * draw that started the loop), and a blend schedule must follow.  The next loop must run on `batch` images at latent side L. */
int agd_inpaint_set(agd_ctx* ctx, const float* mask, int mask_channels, const float* cond, int cond_channels, const float* noise,
                    int batch, int latent_side, void* stream);
int agd_inpaint_set_hw(agd_ctx* ctx, const float* mask, int mask_channels, const float* cond, int cond_channels, const float* noise,
                       int batch, int latent_h, int latent_w, void* stream);
/* the blend's (sa, sb) per model evaluation, host array of 2 n floats; n must equal the next loop's evaluation count.  After the step of
 * evaluation i: x = (1 - m) (sa_i image_latents + sb_i noise) + m x. */
int agd_inpaint_set_schedule(agd_ctx* ctx, const float* sa_sb, int n);
int agd_inpaint_clear(agd_ctx* ctx);

/* ---- InstructPix2Pix (diffusers StableDiffusionInstructPix2PixPipeline).  An 8-channel UNet (in_channels = latent + the VAE's latent
 * channels) reads latents | image latents.  With a state set, every evaluation of agd_denoise_hw / agd_denoise_plms_hw / agd_denoise_dpm_hw
 * runs three branches against the [uncond | cond] context of agd_set_context -- uncond: negative prompt, zero image latents; image: negative
 * prompt, image latents; text: prompt, image latents -- and combines them on the device as
 *   e = e_uncond + guidance (e_text - e_image) + image_guidance (e_image - e_uncond)
 * before the scheduler's step; `guidance` of those calls is the text scale.  The recorders see the text branch only.  ControlNet and GLIGEN
 * schedules, an inpainting state and agd_denoise_panorama are refused while the state is set; without it every loop runs as before. */
/* the front end, once per call, device pointers: image uint8 NHWC [batch,h,w,3] (image_f32 = 0: x / 255, then 2 x - 1) or fp32 NCHW
 * [batch,3,h,w] already in [-1,1] (image_f32 = 1).  Runs the VAE encoder and keeps the posterior mean (`latent_dist.mode()`, NOT multiplied
 * by the scaling factor) on the device; also written to latents_out fp32 NCHW [batch,lc,h/f,w/f] when that is non-NULL.  Ends a state set earlier. */
int agd_ip2p_prepare_hw(agd_ctx* ctx, const void* image, int image_f32, int batch, int h, int w, float* latents_out, void* stream);
/* the state: image latents fp32 NCHW [batch,lc,Lh,Lw] (device; copied), or NULL for the ones agd_ip2p_prepare_hw left (same batch and
 * size).  The next loop must run `batch` images at Lh x Lw. */
int agd_ip2p_set_hw(agd_ctx* ctx, const float* image_latents, int batch, int latent_h, int latent_w, float image_guidance, void* stream);
int agd_ip2p_clear(agd_ctx* ctx);

/* ---- T2I-Adapter (diffusers T2IAdapter "full_adapter" + StableDiffusionAdapterPipeline): a small convolutional network runs ONCE per call
 * on the conditioning image -- PixelUnshuffle(downscale_factor), conv_in 3x3, then per entry of channels[] an AdapterBlock (2x2 average pool
 * from the second block on, a 1x1 in_conv where the width changes, num_res_blocks x [x + conv1x1(relu(conv3x3(x)))]) -- and the output of
 * block i, independent of the timestep, is added to the output of UNet down block i at every evaluation: after the block's last resnet /
 * transformer, before that state becomes a skip and before the downsampler (the last, attention-free block: after the block, the same tensor
 * being its last skip and the mid block's input).  Configured by agd_adapter_configure BEFORE agd_finalize; weights through agd_load_tensor
 * as "adapter." + diffusers state-dict key ("adapter.adapter.conv_in.weight", "adapter.adapter.body.1.in_conv.weight", ...).  agd_finalize
 * needs len(channels) == n_levels, channels[i] == block_out_channels[i] and downscale_factor == the VAE's downscale. */
typedef struct agd_adapter_config {
  int struct_size;                 /* sizeof(agd_adapter_config), ABI guard */
  int in_channels;                 /* channels of the conditioning image (3, or 1 for sketch-style adapters) */
  int n_channels;                  /* len(channels), 1 .. AGD_MAX_LEVELS */
  int channels[AGD_MAX_LEVELS];
  int num_res_blocks;
  int downscale_factor;
} agd_adapter_config;
int agd_adapter_configure(agd_ctx* ctx, const agd_adapter_config* acfg);
/* the conditioning image, device pointer: uint8 NHWC [batch,h,w,in_channels] (image_f32 = 0: x / 255) or fp32 NCHW [batch,in_channels,h,w]
 * already in [0,1] (image_f32 = 1).  Runs the adapter once and keeps its UNSCALED features as fp32 for `batch` images at latent size
 * h / downscale_factor x w / downscale_factor; UNet row image b reads feature image b % batch (both CFG halves the same features). */
int agd_adapter_set_cond_hw(agd_ctx* ctx, const void* image, int image_f32, int batch, int h, int w, void* stream);
/* the features of the last agd_adapter_set_cond_hw, back to back, each fp32 NCHW [batch][channels[i]][Lh >> i][Lw >> i] (device; syncs) */
int agd_adapter_features(agd_ctx* ctx, float* out);
/* per-model-evaluation scales (adapter_conditioning_scale where the features are added, 0 where they are not), host array of n floats,
 * consumed by the next agd_denoise_hw / agd_denoise_plms_hw / agd_denoise_dpm_hw (n must equal its evaluation count) or agd_unet_forward
 * (n = 1).  A scale of exactly 0 runs the plain UNet for that evaluation; n = 0 clears the schedule.  While a schedule is set, ControlNet and
 * GLIGEN schedules, inpainting and InstructPix2Pix states, agd_denoise_panorama and agd_unet_forward_ts are refused. */
int agd_adapter_set_schedule(agd_ctx* ctx, const float* scales, int n);
int agd_adapter_clear(agd_ctx* ctx);                 /* the schedule and the per-call features */
/* seam for tests: the adds launched since agd_create -- counts[0] with GroupNorm partial sums left for the next norm, counts[1] without
 * (maps with no legal statistics tile, or "gn_fused_stats" off: the norm runs its own statistics pass) */
int agd_adapter_add_counts(agd_ctx* ctx, long long* counts);

/* ---- IP-Adapter (image prompts; diffusers >= 0.24 load_ip_adapter / ip_adapter_image, the SD-1.x "ip-adapter_sd15" family): an image
 * projection turns CLIP image embeddings into n_tokens extra context tokens, and every UNet attn2 adds a second cross-attention over them:
 *   out = to_out(attn(q, K_text, V_text) + scale * attn(q, to_k_ip(tokens), to_v_ip(tokens))).
 * Loaded AFTER agd_finalize, like a LoRA; one adapter at a time.  The ControlNet's attn2 layers take no image branch.
 * agd_ip_adapter_begin(embed_dim, n_tokens), then agd_ip_adapter_tensor per tensor (fp32, host or device): "image_proj.proj.weight"
 * [n_tokens * cross_attention_dim, embed_dim], "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias", and per UNet
 * transformer block "<block prefix>transformer_blocks.0.attn2.to_k_ip.weight" / "...to_v_ip.weight" [C, cross_attention_dim] (the block
 * prefix with or without "unet."); agd_ip_adapter_commit names whatever is missing or misshapen.  agd_ip_adapter_unload frees everything. */
int agd_ip_adapter_begin(agd_ctx* ctx, int embed_dim, int n_tokens);
int agd_ip_adapter_tensor(agd_ctx* ctx, const char* name, const void* ptr, int dtype, int ndim, const long long* shape);
int agd_ip_adapter_commit(agd_ctx* ctx);
int agd_ip_adapter_unload(agd_ctx* ctx);
/* once per call, AFTER agd_lora_set_scale: image_embeds fp32 [batch2][embed_dim] (rows [0,B) the unconditional half -- the caller passes
 * zeros there, which the projection turns into non-zero tokens), a finite scale.  Runs the image projection and builds, per attn2 layer, the
 * pre-multiplied per-image matrices from the CURRENT to_q / to_out; a later agd_lora_set_scale makes them stale and the next forward refuses
 * until agd_ip_adapter_set runs again.  With tokens set and scale != 0, agd_denoise* and agd_unet_forward(_hw) on batch2 rows run the image
 * branch in every UNet transformer block; agd_unet_forward_ts*, agd_denoise_panorama and any call with a ControlNet, GLIGEN or T2I-Adapter
 * schedule, an inpainting state or an InstructPix2Pix state are refused.  Scale 0 or nothing set: exactly the plain UNet, launch for launch.
 * agd_attn_processor / agd_cross_attn stay text-only; DAAM and the hook.py recorder see the text branch only. */
int agd_ip_adapter_set(agd_ctx* ctx, const float* image_embeds, int batch2, float scale, void* stream);
int agd_ip_adapter_clear(agd_ctx* ctx);              /* the per-call state and the counts; the weights stay loaded */
int agd_ip_adapter_tokens(agd_ctx* ctx, float* out); /* the projected tokens fp32 [batch2][n_tokens][cross_attention_dim] (host or device; syncs) */
/* seam for tests: x + scale * to_out_weight . attn_ip(norm2(x)) of one block on x fp32 [batch2][h*w][C] (device), any map shape */
int agd_ip_adapter_block(agd_ctx* ctx, const char* block_name, const float* x, int batch2, int h, int w, float* out, void* stream);
/* seam for tests: the score / add launches of the block walk since the last agd_ip_adapter_clear (or load) */
int agd_ip_adapter_counts(agd_ctx* ctx, long long* counts);

/* ---- the IP-Adapter's image encoder (a transformers CLIPVisionModelWithProjection: image_embeds = visual_projection(post_layernorm(CLS));
 * the published SD-1.5 adapters use OpenCLIP ViT-H/14: hidden 1280, 32 layers, 16 heads of 80, MLP 5120, gelu, patch 14, 224 px,
 * projection 1024).  It runs the safety checker's vision path (CLIPImageProcessor front end, patch embedding, encoder, pooled head) under
 * its own weights, loaded AFTER agd_finalize: agd_image_encoder_begin(vcfg) with n_special = n_concepts = 0 and head dim 64 or 80, then
 * agd_image_encoder_tensor per tensor (fp32; names "image_encoder." + the transformers key: "image_encoder.vision_model.embeddings.…",
 * "image_encoder.visual_projection.weight"), then agd_image_encoder_commit (checks every shape, fuses q/k/v).  One encoder per context;
 * agd_image_encoder_unload frees it, and is also how a load that failed part way (a refused tensor or commit) is cleared before it is
 * tried again.  agd_image_embeds: uint8 NHWC [batch,h,w,3] (device) -> fp32 [batch][projection_dim] (device). */
int agd_image_encoder_begin(agd_ctx* ctx, const agd_vision_config* vcfg);
int agd_image_encoder_tensor(agd_ctx* ctx, const char* name, const void* ptr, int dtype, int ndim, const long long* shape);
int agd_image_encoder_commit(agd_ctx* ctx);
int agd_image_encoder_unload(agd_ctx* ctx);
int agd_image_embeds(agd_ctx* ctx, const unsigned char* images, int batch, int h, int w, float* out, void* stream);

/* ---- GLIGEN (diffusers StableDiffusionGLIGENPipeline, a UNet of attention_type "gated"): a PositionNet turns per-object phrase
 * embeddings and boxes into grounding tokens, and a GatedSelfAttentionDense ("fuser") in every transformer block, after attn1's residual
 * add, attends over the block's rows plus those tokens:  x += tanh(alpha_attn) attn(norm1([x; o]))[:N];  x += tanh(alpha_dense) ff(norm2(x)).
 * Configured by agd_gligen_configure BEFORE agd_finalize; weights through agd_load_tensor under their diffusers keys ("unet.position_net.*",
 * "unet.<block>.transformer_blocks.0.fuser.*"; the 0-d alpha_attn / alpha_dense included).  agd_finalize fuses each fuser's q/k/v and k/v
 * and pre-scales its to_out and ff.net.2 biases by the tanh gates (the gates themselves go on the GEMM accumulators). */
typedef struct agd_gligen_config {
  int struct_size;                 /* sizeof(agd_gligen_config), ABI guard */
  int max_objs;                    /* 30 */
  int positive_len;                /* PositionNet positive_len (the UNet's cross_attention_dim) */
  int fourier_freqs;               /* 8 */
} agd_gligen_config;
int agd_gligen_configure(agd_ctx* ctx, const agd_gligen_config* gcfg);
/* the per-call objects, device fp32: boxes [batch2][max_objs][4] (x0, y0, x1, y1 in [0,1]), pos_emb [batch2][max_objs][positive_len],
 * masks [batch2][max_objs] (1 = a real object, 0 = null; the CFG unconditional half all null).  Runs the PositionNet and, for every fuser,
 * linear -> norm1 -> K/V of the max_objs grounding rows, kept per block ([batch2][max_objs][2C] bf16) for the next forwards on batch2 rows. */
int agd_gligen_set(agd_ctx* ctx, const float* boxes, const float* pos_emb, const float* masks, int batch2, void* stream);
/* one flag per model evaluation (1 = the fusers run), host array of n ints, consumed by the next agd_denoise / agd_denoise_plms /
 * agd_denoise_dpm (n must equal its evaluation count) or agd_unet_forward (n = 1).  A flag of 0 runs exactly the plain UNet.
 * n = 0 clears the schedule. */
int agd_gligen_set_schedule(agd_ctx* ctx, const int* flags, int n);
int agd_gligen_clear(agd_ctx* ctx);                  /* the schedule and the per-call objects */
/* seams for tests: the PositionNet output of the current call, out fp32 [batch2][max_objs][cross_attention_dim] (device; syncs), and one
 * fuser forward on rows x fp32 [batch2][h*w][C] -> out (device; the block's name as "down_blocks.0.attentions.0", "unet." optional) */
int agd_gligen_objs(agd_ctx* ctx, float* out);
int agd_gligen_fuser(agd_ctx* ctx, const char* block_name, const float* x, int batch2, int h, int w, float* out, void* stream);

/* ---- `unet(sample, t, encoder_hidden_states).sample`: sample/out fp32 NCHW [B2,4,L,L] */
int agd_unet_forward(agd_ctx* ctx, const float* sample, int batch2, int latent_side, float timestep, float* out,
                     void* stream);
int agd_unet_forward_hw(agd_ctx* ctx, const float* sample, int batch2, int latent_h, int latent_w, float timestep, float* out, void* stream);
/* the same with one timestep PER IMAGE (host array of batch2 floats): the training call `unet(noisy_latents, timesteps, ehs)` of
 * finetune_sd_token.py:1027, where `timesteps` is a [bsz] tensor */
int agd_unet_forward_ts(agd_ctx* ctx, const float* sample, int batch2, int latent_side, const float* timesteps, float* out, void* stream);
int agd_unet_forward_ts_hw(agd_ctx* ctx, const float* sample, int batch2, int latent_h, int latent_w, const float* timesteps, float* out,
                           void* stream);

/* ---- CFG combine + DDIM (eta 0) step on fp32 NCHW latents [B,4,L,L] in place;
 * eps is [2B,4,L,L] NCHW.  (`scheduler.step` inside pipeline.__call__) */
int agd_cfg_ddim_step(agd_ctx* ctx, const float* eps, float* latents, int batch, int latent_side, float guidance,
                      float alpha_t, float alpha_prev, void* stream);
int agd_cfg_ddim_step_hw(agd_ctx* ctx, const float* eps, float* latents, int batch, int latent_h, int latent_w, float guidance,
                         float alpha_t, float alpha_prev, void* stream);

/* ---- the whole denoise loop of `pipeline(prompt, num_inference_steps=..)` on device:
 * latents [B,4,L,L] fp32 in/out; per-step timesteps and alpha_cumprod (t, prev) from the host
 * scheduler.  Heat-map recording follows agd_record_config. */
int agd_denoise(agd_ctx* ctx, float* latents, int batch, int latent_side, int n_steps, const float* timesteps,
                const float* alpha_t, const float* alpha_prev, float guidance, void* stream);
int agd_denoise_hw(agd_ctx* ctx, float* latents, int batch, int latent_h, int latent_w, int n_steps, const float* timesteps,
                   const float* alpha_t, const float* alpha_prev, float guidance, void* stream);

/* ---- the same loop under the scheduler the reference actually runs: data_generation.py:59 calls the pipeline with the
 * checkpoint's default PNDMScheduler (skip_prk_steps: PLMS) x 20.  n_evals = steps + 1 model evaluations; per evaluation the
 * UNet timestep and the two `_get_prev_sample` coefficients (prev = sample_coeff * sample + eps_coeff * model_output) come
 * from the host scheduler (agenda_amd/scheduler.py PNDMScheduler); the multistep weights are applied on the device. */
int agd_denoise_plms(agd_ctx* ctx, float* latents, int batch, int latent_side, int n_evals, const float* timesteps,
                     const float* sample_coeff, const float* eps_coeff, float guidance, void* stream);
int agd_denoise_plms_hw(agd_ctx* ctx, float* latents, int batch, int latent_h, int latent_w, int n_evals, const float* timesteps,
                        const float* sample_coeff, const float* eps_coeff, float guidance, void* stream);

/* ---- the same loop under DPM-Solver++ (2M) (agenda_amd/scheduler.py DPMSolverMultistepScheduler, epsilon or v-prediction, with
 * or without Karras sigmas): n_evals = steps model evaluations.  Per evaluation i the host passes the UNet timestep (fractional
 * with Karras sigmas) and coeffs[5 i + 0..4] = cx, ce, a, b0, b1: x0 = cx * sample + ce * model_output, then
 * sample = a * sample + b0 * x0 + b1 * x0 of evaluation i - 1.  The previous x0 lives in a context-owned buffer. */
int agd_denoise_dpm(agd_ctx* ctx, float* latents, int batch, int latent_side, int n_evals, const float* timesteps,
                    const float* coeffs, float guidance, void* stream);
int agd_denoise_dpm_hw(agd_ctx* ctx, float* latents, int batch, int latent_h, int latent_w, int n_evals, const float* timesteps,
                       const float* coeffs, float guidance, void* stream);

/* ---- `vae.decode(latents / scaling_factor)` + image post-process.
 * out_u8: [B, 8L, 8L, 3] uint8 (may be NULL); out_f32: [B, 8L, 8L, 3] fp32 in [-1,1] (may be NULL) */
int agd_vae_decode(agd_ctx* ctx, const float* latents, int batch, int latent_side, unsigned char* out_u8,
                   float* out_f32, void* stream);
int agd_vae_decode_hw(agd_ctx* ctx, const float* latents, int batch, int latent_h, int latent_w, unsigned char* out_u8,
                      float* out_f32, void* stream);   /* images [batch][8 latent_h][8 latent_w][3] */

/* ---- `vae.encode(image).latent_dist` (img2img front end; anchors: finetune_sd.py:764-765):
 * image fp32 NCHW [B,3,S,S] in [-1,1] -> mean and logvar fp32 NCHW [B,4,S/8,S/8].  Syncs. */
int agd_vae_encode(agd_ctx* ctx, const float* image, int batch, int side, float* mean_out, float* logvar_out, void* stream);
int agd_vae_encode_hw(agd_ctx* ctx, const float* image, int batch, int h, int w, float* mean_out, float* logvar_out, void* stream);

/* ---- per-ctx options (no environment variables steer the library).  "cfg_shared_prefix" (default 1): agd_denoise runs the
 * layers ahead of the first cross-attention once for the identical unconditional / conditional halves (bit-identical to 0).
 * "ln_fold", "gn_fused_stats" (default 1): LayerNorm / GroupNorm statistics produced by the GEMM that writes the activation.
 * "gn_proj_fold" (default 1; 0 off, 2: also C = 640): the GroupNorm in front of a transformer's proj_in (no activation in between) is
 * folded into per-image proj_in matrices where C <= 320 and the producer left its statistics; proj_in then reads the un-normalised activation.
 * "weight_touch" (default 3; 0 off): 1x1 weight matrices of at least that many MB are streamed through the caches by a read-only
 * kernel right in front of the launch that uses them (the UNet's 1.7 GB of weights never stay in the 256 MB Infinity Cache).
 * "conv_halo" (default 1): 3x3 stride-1 convolutions run the row-halo kernel (one LDS image of the tile's pixel rows serves the three
 * horizontal taps) where its geometry applies.
 * "weight_warm" (default 3; 0 off): the first workgroups of a launch stream its weight matrix through the caches before their main
 * loops -- 1: only launches whose weights outweigh their activations (each XCD its own slice, into its L2); 3: every launch with
 * >= 1 MB of weights and 1024 <= M <= 32768 (the touch launches then disappear).
 * "igemm8p" (default 1): launches with enough 256-row tiles (wide 1x1 projections, 3x3 convs with N a multiple of 256, the
 * upsampling convs) run the 8-wave / 8-phase implicit-GEMM kernel (igemm8p.h); 0 = the 4-wave kernels everywhere; tests: 2 / 3 / 4
 * force its 256-wide / 160-wide / any legal tile.
 * "tblock_fuse" (default 1791): fused row-panel kernels of the transformer blocks at C = 320 (tblock.hip) -- bit 0: norm3 -> GEGLU ->
 * ff.net.2 + residual as one launch, bit 1: norm2 -> to_q -> cross-attention (+ recorder) -> to_out + residual as one launch, bit 2: that
 * launch starts at attn1.to_out + residual, bit 3: the feed-forward launch ends with proj_out + residual (+ the next GroupNorm's sums), bit 4: proj_in (GroupNorm folded) -> norm1 ->
 * q / k / v projections as one launch, bit 5: the attn2 chain (bits 1, 2) for the C = 640 blocks of the 32 x 32 maps as well (64-row panels), bit 6: under `cfg_shared_prefix` the duplication of the shared rows happens inside the fused kernels (no copy launches), bit 7: the bit-4 launch applies the transformer's GroupNorm itself (statistics from the producer's partial sums, rows normalised in its LDS panel) instead of reading per-image folded matrices from a fold launch, bit 8 (not in the default: measured slower): that launch, GroupNorm inside, for the C = 640 blocks too, bit 9: inside the feed-forward launch (bits 0, 3) ff.net.2 and proj_out are pre-multiplied (Wp W2 at load time; the proj_out stage adds Wp . h on the same accumulators -- no intermediate h3), bit 10: the attn2 chain of the C = 640 blocks on 32-row panels where 64-row panels give fewer than 200 workgroups (M = 8192: 256 workgroups instead of 128).
 * "reduce_gn" (default 1): the slab-sum pass of a split-K conv also applies the GroupNorm (+ SiLU) that reads its output next (conv1 -> norm2 of a
 * ResnetBlock2D; conv2 -> the following module's norm where that reads this output alone); 0 = separate statistics / apply launches.
 * "conv_smap" (default 1): 3x3 convs of the 8 x 8 maps run the whole-images-resident kernel (igemm_smap.h).
 * "upsample_phases" (default 7; bit 0: the UNet's from 16 x 16 maps up, bit 1: the VAE decoder's, bit 2: the UNet's 8 x 8 -> 16 x 16 one): nearest-2x upsampling convs run as four 2x2 phase convs on the un-upsampled map in one launch (taps that coincide pre-summed at load
 * time, pixel-shuffled output rows: 4/9 of the MACs); 0 = the 3x3 conv with the upsample folded into its gather.
 * "ff_proj_fuse" (default 1): ff.net.2 (+ residual) and proj_out (+ block residual) as one GEMM with the pre-multiplied matrix [Wp W2 | Wp] over [hidden | h], in the transformer
 * blocks whose feed-forward is not the fused row-panel kernel; 0 = two launches.
 * "shortcut_fuse" (default 3): a UNet ResnetBlock2D's 1x1 conv_shortcut runs as extra K of its conv2 launch (the shortcut's output is never stored) -- bit 0: where conv2 is a
 * row-halo launch (the 64 x 64 .. 16 x 16 maps), bit 1: the 8 x 8 whole-images launches; 0 = its own launch, added as conv2's residual.
 * "wreg_mask" (default 3): the weight-streaming kernel (igemm_wreg.h: weight fragments straight to registers) for bit 0 = the GEGLU projection of the C = 1280 blocks at 16 x 16,
 * bit 1 = proj_in / proj_out of the C = 640 transformer blocks.
 * "igemm_kgroups" (default 1): the unsplit 1x1 launches on 64 x 64 tiles (8 x 8 maps: at most one workgroup per CU) run two K groups of four waves per workgroup.
 * "igemm_pc" (default 49): producer / consumer implicit GEMM (csrc/igemm_pc.h: loader waves issue the ring's LDS-DMA pieces, consumer waves read fragments one K step ahead and run the MFMAs) --
 * bit 0: the 1x1 launches on 64 x 160 tiles (one workgroup per CU: the 16 x 16 / 8 x 8 maps), bits 1 - 3 (measured slower, off): 3x3 convs of the 16 x 16 / 8 x 8 maps,
 * bit 4: the row-halo producer / consumer kernel (csrc/igemm_pch.h) for the 3x3 stride-1 convs whose 128 x 160 tiles (x K slices) make at most one workgroup per CU (the
 * 32 x 32 and 16 x 16 maps at UNet batch 8), fused conv_shortcut included; same tiles and summation order as the row-halo kernel: bit-identical;
 * bit 5: the plain 1x1 launches of one 128 x 160 tile per CU (M = 8192, N = 640: ff.net.2 + proj_out of the 32 x 32 blocks) on igemm_pc.h's 128-row form; bit-identical.
 * "xcd_block" (default 1): the igemm tile grid is cut into one a x b block of tiles per XCD, (a, b) minimising the XCD's L2 working set, instead of tiles / 8 consecutive tiles of the
 * A-major / W-major walk (same tiles, same results bit for bit).
 * "attn2_premul" (default 1, bit 1 -- also the head-dim-80 blocks -- off: a tie; read at the next agd_set_context): attn2 of the blocks with head dim >= 160 (SD-1.x: C = 1280, the 16 x 16 and 8 x 8 maps) runs against per-image
 * PRE-MULTIPLIED context matrices built once per agd_set_context (csrc/xattn_pre.hip; hook.py:91-120): S = LN(h) . K'' with K'' = gamma scale (k Wq), softmax + recorder in that GEMM's
 * epilogue, out = P . V'' + bo + h with V'' = Wo v -- two launches instead of to_q, the attention kernel and to_out; 0 = the kernel chain.  The hook.py recorder keeps the chain.
 * "side_stream" (default 0; measured slower, kept for the A/B): a resnet's 1x1 conv_shortcut runs on a second stream beside norm1 / conv1 / norm2. */
int agd_set_option(agd_ctx* ctx, const char* name, int value);

/* ---- heat-map recording (daam.trace / hook.py UNetCrossAttentionHooker state)
 * mode 0 off; 1 DAAM (per-layer/head time sums, mid block excluded, conditional half);
 * 2 HOOK (hook.py: head-mean per call, every attn2 incl. mid; is_train=1 keeps all batch rows).
 * rec_tokens: token rows recorded (<= tokens; rows beyond len(prompt)+2 are never read by daam); takes effect at the
 * next agd_record_reset, which (re)sizes the accumulators for it.
 * A context beyond 96 tokens (agd_set_context): mode 1 only, rec_tokens up to the context's T (larger is refused by agd_record_reset), the
 * accumulators hold per-head rows at every level (no head-group sums at latent resolution) and are written by csrc/attention_long.hip.
 * Accumulators sized before the context was set, for head-group sums or for more rows than it has, make the next recording call fail
 * by name ("reset after agd_set_context"); mode 2 is refused by agd_record_reset / agd_hook_reset and by the calls themselves. */
int agd_record_config(agd_ctx* ctx, int mode, int is_train, int rec_tokens);
int agd_record_reset(agd_ctx* ctx, int batch, int latent_side, void* stream);   /* hooker.clear() / new trace */
/* DAAM: layer accumulators of (latent_h / f) x (latent_w / f), f = 2^level; agd_daam_global then writes [rows][latent_h][latent_w].
 * The hook.py recorder (mode 2) takes square latents only. */
int agd_record_reset_hw(agd_ctx* ctx, int batch, int latent_h, int latent_w, void* stream);
/* daam `compute_global_heat_map()` for image `img`: out [rows, S, S] fp32 (rows <= rec_tokens). Stream-ordered. */
int agd_daam_global(agd_ctx* ctx, int img, int rows, float* out, void* stream);
/* hook.py `compute_global_heat_map()`: out [B', T, S, S]; returns -2 if nothing was recorded. Stream-ordered. */
int agd_hook_global(agd_ctx* ctx, float* out, void* stream);
int agd_hook_count(agd_ctx* ctx);
/* the map hook.py:110-112 appends for the most recent recorded call: out [B', T, h, w] (h*w = n_query). Stream-ordered. */
int agd_hook_last_map(agd_ctx* ctx, float* out, int n_query, void* stream);

/* ---- the processor seam, hook.py:83-122 in full: one call of the diffusers attention-processor protocol
 * `proc(attn, hidden_states, encoder_hidden_states=None, attention_mask=None)` for the UNet `Attention` module
 * `layer` (module path, e.g. "down_blocks.0.attentions.0.transformer_blocks.0.attn2" or "...attn1").
 *   ctx_emb != NULL on an attn2 module: cross-attention (is_cross_attn, hook.py:94-99); record != 0 feeds the recorder
 *   ctx_emb == NULL on an attn1 module: self-attention (encoder_hidden_states = hidden_states); records nothing
 *   attn_mask: additive fp32 [B2, keys] (hook.py:92 `prepare_attention_mask`, broadcast over heads and queries) or NULL
 * hidden/out fp32 [B2, N, C]; ctx_emb fp32 [B2, T, ctx_dim].  Returns to_out[0](softmax(scale QK^T + mask) V) + bias. */
int agd_attn_processor(agd_ctx* ctx, const char* layer, const float* hidden, const float* ctx_emb, const float* attn_mask,
                       int batch2, int n_query, int tokens, float* out, int record, void* stream);
/* the same for an attn2 module without a mask (kept for callers of the round-1 ABI) */
int agd_cross_attn(agd_ctx* ctx, const char* layer, const float* hidden, const float* ctx_emb, int batch2,
                   int n_query, int tokens, float* out, int record, void* stream);

/* ---- training-mode seam (what finetune_sd_token.py does with hook.py's recorder)
 * With agd_record_config(2, is_train = 1) every recorded attn2 call keeps its head-mean map [B', T, n_query] on the device
 * (hook.py:110-112 `cross_attn_maps.append`), in call order, until the next agd_record_reset (`hooker.clear()`,
 * finetune_sd_token.py:1024,1069). */
int agd_hook_reset(agd_ctx* ctx, int rows, int latent_side, void* stream);   /* clear() with B' given explicitly (no CFG pairing) */
int agd_hook_num_maps(agd_ctx* ctx);
int agd_hook_map_dims(agd_ctx* ctx, int k, int* dims3);                 /* {B', T, n_query} of the k-th kept map */
int agd_hook_map(agd_ctx* ctx, int k, float* out, void* stream);        /* out [B', T, n_query] fp32; stream-ordered */
/* The attention regulariser of finetune_sd_token.py:1046-1066 on ONE recorded map [B, T, P = h*w]: per sample the object /
 * foreground / background token rows are min-max normalised (+1e-8), L1-normalised, and compared:
 *   bg = coef * mean|(1 - o^)/sum(1 - o^) - b~| ,  fg = coef * mean|o^/sum(o^) - f~|      (coef = reg_weight / #object samples)
 * loss_out [B][2] = {bg, fg}; dmap [B, T, P] (may be NULL) = d(bg + fg)/d map (min/max paths included, as torch autograd).
 * obj/fg/bg_idx: device int [B]; obj_idx < 0 skips the sample (:1048).  Stream-ordered. */
int agd_op_attn_reg_loss(const float* map, int B, int T, int P, const int* obj_idx, const int* fg_idx, const int* bg_idx, float coef,
                         float* loss_out, float* dmap, void* stream);
/* Backward of one cross-attention call of the seam (hook.py:91-120) w.r.t. its inputs: given d_out [B2, N, C] (gradient of the
 * returned hidden_states; may be NULL) and/or d_map [B', T, N] (gradient of the recorded map; B' = B2 if is_train else B2/2;
 * may be NULL) -> d_hidden [B2, N, C] and d_ctx [B2, T, ctx_dim] fp32 (either may be NULL).  ctx_emb NULL = the cached context. */
int agd_attn_processor_backward(agd_ctx* ctx, const char* layer, const float* hidden, const float* ctx_emb, const float* d_out,
                                const float* d_map, int is_train, int batch2, int n_query, int tokens, float* d_hidden, float* d_ctx,
                                void* stream);

/* ---- single-op entry points (fp32 in/out, converted to the bf16 NHWC compute layout inside);
 * used by the parity tests, mirror torch.nn.functional signatures the oracle uses. */
int agd_op_conv2d(const float* x_nchw, const float* w, const float* bias, float* y_nchw, int B, int Cin, int H, int W,
                  int Cout, int ksize, int stride, int pad, int upsample, void* stream);
/* flags bit 0: 3x3 stride-1 launches take the row-halo kernel where it applies; bit 4: 8 x 8 maps take the whole-images-resident kernel
   (igemm_smap.h); bits 1..3: the 256-row 8-wave / 8-phase kernel --
   2 = where the launcher would pick it, 4 / 8 = force its 256- / 160-wide tile (agd_op_linear: the same bits in `geglu`, bit 0 = GEGLU,
   bit 4 = the weight-streaming 1x1 kernel, igemm_wreg.h: the matrix in fragment order straight to registers, bf16 output) */
int agd_op_conv2d_ex(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int H, int W, int Cout,
                     int ksize, int stride, int pad, int upsample, int flags, void* stream);
int agd_op_linear(const float* x, const float* w, const float* bias, const float* residual, float* y, int M, int K,
                  int N, int geglu, void* stream);
/* BasicTransformerBlock's feed-forward tail as ONE launch (tblock.hip): y = x + ff.net.2(GEGLU(ff.net.0(norm3(x)))), the op sequence
 * diffusers runs behind reference data_generation/data_generation.py:59; x / y [M][C] fp32, w1 [8C][C] (value rows then gate rows),
 * b1 [8C], w2 [C][4C], b2 [C]; C = 320 (the 64 x 64 maps' blocks) */
int agd_op_ff_fused(const float* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* y, int M, int C, float eps, void* stream);
/* BasicTransformerBlock's attn2 section as ONE launch (tblock.hip): y = x + to_out(softmax(scale to_q(norm2(x)) k^T) v), the processor body of
 * reference data_generation/hook.py:91-120 with the LayerNorm in front and the residual behind it; x / y [B * HW][C] fp32, kv [B][T][2C] =
 * the projected context (to_k columns then to_v columns), probs_sum (optional) [B][T][HW] = the probabilities summed over the heads;
 * C = 320 (HW a multiple of 128) or C = 640 (HW a multiple of 64), 8 heads, T <= 96 */
int agd_op_attn_chain(const float* x, const float* gamma, const float* beta, const float* wq, const float* kv, const float* wo,
                      const float* bo, float* y, float* probs_sum, int B, int HW, int T, int C, int heads, float eps, void* stream);
/* The three row-panel chains of csrc/tblock.hip reaching EVERY form of their launchers, for per-kernel tests.  Context-free; inputs fp32,
 * rounded to bf16 by the entry; outputs bf16 widened exactly; weights converted and put into fragment order by the library's own kernels, as
 * the loader does; whatever a launcher refuses comes back as -1 with its message.
 *
 * agd_op_ff_fused_ex: agd_op_ff_fused plus the proj_out stage -- wp [C][C] != NULL: pout [M][C] = (x + FF(x)) wp^T + bp + xres, with xres
 * [xres_rows > 0 ? xres_rows : M][C] (output row m adds row m % xres_rows) and y not written (may be NULL).  premul: w2 is the caller's product
 * Wp W2 [C][4C] and bp the caller's Wp b2 + bp.  colstat (optional, with wp): [ceil(M / 128)][C][2] device floats = per-(128-row tile, channel)
 * sum and sum of squares of the bf16 pout.  inplace: the launch writes over its own input rows (out == h).
 *
 * agd_op_attn_chain_ex: agd_op_attn_chain plus the attn1.to_out prologue (o1, wo1 [C][C], bo1: h1 = o1 wo1^T + bo1 + x is formed first and is
 * the chain's input; h1 (optional) [B * HW][C] receives it), src_rows > 0 (x / o1 hold src_rows rows, output row m reads row m % src_rows),
 * rowstat (optional) [B * HW][2] = (sum, sum of squares) of each bf16 output row, and the recorder as the kernel sees it: rec (optional)
 * [B - rec_b0][8 / rec_hpb][rec_rows][HW] device floats that the launch ADDS to (never zeroed here): images >= rec_b0, head groups of rec_hpb
 * in {1, 2, 4, 8}, token rows < rec_T <= rec_rows.  rows32: allow the 32-row panels of C = 640.  inplace: out == h.
 *
 * agd_op_qkv_chain: GroupNorm -> proj_in -> h -> norm1 -> q | k | v as one launch.  x [M][C] raw rows of M / HW images (NHWC), part = the
 * caller's partial-sum table of those rows (layout of agd_op_groupnorm_ex, bm pixels per tile), w_in [C][C], b_in [C], wqkv [3C][C] (q, k, v
 * rows); h [M][C], qkv [M][3C].  flags bit 0: the GroupNorm is applied inside the kernel, clear: folded into per-image matrices
 * (launch_gn_fold_weight in the chain's fragment order); bit 1: 64-row panels (C = 320); bit 2: the second schedule.  C = 320 or 640. */
int agd_op_ff_fused_ex(const float* x, const float* gamma, const float* beta, const float* w1, const float* b1, const float* w2,
                       const float* b2, float* y, int M, int C, float eps, const float* wp, const float* bp, const float* xres,
                       int xres_rows, float* pout, int premul, float* colstat, int inplace, void* stream);
int agd_op_attn_chain_ex(const float* x, const float* gamma, const float* beta, const float* wq, const float* kv, const float* wo,
                         const float* bo, float* y, int B, int HW, int T, int C, int heads, float eps, const float* o1, const float* wo1,
                         const float* bo1, float* h1, int src_rows, float* rowstat, float* rec, int rec_hpb, int rec_b0, int rec_T,
                         int rec_rows, int rows32, int inplace, void* stream);
int agd_op_qkv_chain(const float* x, const float* gn_gamma, const float* gn_beta, int groups, float gn_eps, const float* part, int bm,
                     const float* w_in, const float* b_in, const float* gamma, const float* beta, float ln_eps, const float* wqkv, float* h,
                     float* qkv, int M, int HW, int C, int flags, void* stream);
/* the same function through the pre-multiplied form of the C = 1280 blocks (csrc/xattn_pre.hip; hook.py:91-120 behind norm2): the context products
 * K'' = gamma scale (k Wq), V'' = Wo v are built first, then S = LN-folded x K''^T -> softmax -> P V''^T + bo + x as two GEMMs.
 * probs (may be NULL): [B][heads][T][HW], every head's probabilities (the recorder's per-(image, head) rows).  Needs HW % 64 == 0, T <= 80,
 * head dim % 8 == 0, C % 160 == 0 and C % 64 == 0 (i.e. C a multiple of 320), heads x 80 a multiple of 64. */
int agd_op_xattn_premul(const float* x, const float* gamma, const float* beta, const float* wq, const float* kv, const float* wo,
                        const float* bo, float* y, float* probs, int B, int HW, int T, int C, int heads, float eps, void* stream);
/* The stages of agd_op_xattn_premul (csrc/xattn_pre.hip) and of the IP-Adapter branch (csrc/ipadapter.hip) one launcher at a time, for per-kernel
 * tests.  Context-free, device pointers, fp32 in and out; bf16 quantities are rounded / widened on the device; every output the kernels write
 * is pre-filled with the byte 0x7F so an element a kernel leaves out shows; a launcher's refusal comes back as -1 with its message.
 *
 * agd_op_xattn_context: kv [B][T][2C], wq / wo [C][C], gamma / beta [C] -> kpp [B][heads][80][C] (K''), cs / bs [B][heads][80], vpp [B][C][heads][80]
 * (V''), built by the launches agd_op_xattn_premul makes, the zero padding of token rows >= T included.
 * agd_op_xattn_scores: launch_xattn_s alone on the caller's K'' / cs / bs -> P [B * HW][heads * 80].  stats (may be NULL: one slot, computed here)
 * [B * HW][slots][2] = partial (sum, sum of squares) of each row of x.  rec (may be NULL) [B - rec_b0][heads][rec_rows][HW] is ADDED to (never zeroed
 * here): images >= rec_b0, token rows < rec_T <= rec_rows.
 * agd_op_ipa_linear / agd_op_ipa_layernorm / agd_op_ipa_scores / agd_op_ipa_add: one launcher each.  agd_op_ipa_context: the Wq . beta mat-vec and
 * launch_ipa_premul -> kpp [B][colsP][C], cs / bs [B][colsP], vpp [B][C][colsP].  agd_op_ipa_scores writes into the CALLER's P
 * [B * HW + guard_rows][colsP] and agd_op_ipa_add updates the CALLER's h [B * HW + guard_rows][C] in place (both through bf16), so rows the kernel
 * must not touch come back as they went in. */
int agd_op_xattn_context(const float* kv, const float* wq, const float* wo, const float* gamma, const float* beta, float* kpp, float* cs,
                         float* bs, float* vpp, int B, int T, int C, int heads, void* stream);
int agd_op_xattn_scores(const float* x, const float* stats, int slots, const float* kpp, const float* cs, const float* bs, float* P, float* rec,
                        int rec_b0, int rec_T, int rec_rows, int B, int HW, int T, int C, int heads, float eps, void* stream);
int agd_op_ipa_linear(const float* x, const float* w, const float* bias, float* y, int R, int N, int K, void* stream);
int agd_op_ipa_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps, void* stream);
int agd_op_ipa_context(const float* kip, const float* vip, const float* wq, const float* wo, const float* gamma, const float* beta, float* kpp,
                       float* cs, float* bs, float* vpp, int B, int C, int heads, int nt, int colsP, void* stream);
int agd_op_ipa_scores(const float* h, const float* kpp, const float* cs, const float* bs, float* P, int B, int HW, int C, int heads, int nt,
                      int colsP, float eps, int guard_rows, void* stream);
int agd_op_ipa_add(float* h, const float* P, const float* vpp, int B, int HW, int C, int colsP, float s, int guard_rows, void* stream);
int agd_op_groupnorm(const float* x_nchw, const float* gamma, const float* beta, float* y_nchw, int B, int C, int HW,
                     int groups, float eps, int silu, void* stream);
/* agd_op_groupnorm reaching EVERY form of the GroupNorm launcher, for per-kernel tests: one source, or the channel concat x0 | x1 (both NCHW
 * fp32, rounded to bf16 by the entry; x1 NULL with C1 = 0), and optional partial-sum tables made by the caller in the layout the producing
 * GEMM's epilogue leaves: part[((b * (HW / bm) + tile) * Cs + ch) * 2 + {0, 1}] = sum / sum of squares of source channel ch's bf16 values
 * over the bm pixels of tile `tile` of image b (Cs = C0 for part0 / bm0, C1 for part1 / bm1; device fp32; NULL / 0: none).  With tables for
 * every source and a shape the one-kernel form supports, the statistics pass is skipped; otherwise the two-kernel form runs.  *path (may be
 * NULL): 1 = the partial-sum kernel ran, 2 = the two-kernel path.  Refused (-1, nothing computed or allocated), like every GroupNorm entry:
 * C0 + C1 < 8 or > 4096, C0 + C1 or C0 not a multiple of 8, groups < 1 or > 64 or not dividing C0 + C1. */
int agd_op_groupnorm_ex(const float* x0_nchw, const float* x1_nchw, const float* gamma, const float* beta, float* y_nchw, int B, int C0,
                        int C1, int HW, int groups, float eps, int silu, const float* part0, int bm0, const float* part1, int bm1,
                        int* path, void* stream);
/* The GroupNorm folded into the projection behind it (Transformer2DModel norm -> proj_in), piece by piece: per image,
 * wb [B][N][C] = bf16(W gamma rstd) and rowadd [B][N] = bias + W beta - wb mu, statistics from `part` (layout above, bm pixels per tile).
 * frag_ni > 0: also wb_frag = the kernel's MFMA-fragment-ordered matrices and wb_frag_ref = the library's fragment re-layout of each
 * image's row-major wb, both [B][N * C] in storage order (N % (16 frag_ni) == 0).  y (may be NULL) [B * HW][N]: the RAW activation x (NCHW,
 * rounded to bf16) times image i's matrix plus image i's row, as the transformer's proj_in runs (C % 64 == 0, HW % 64 == 0).  All fp32
 * (bf16 values widened exactly); w [N][C], bias (may be NULL) [N].  C <= 1024, HW % bm == 0. */
int agd_op_gn_fold(const float* x_nchw, const float* part, int bm, int B, int C, int HW, int groups, float eps, const float* gamma,
                   const float* beta, const float* w, const float* bias, int N, int frag_ni, float* wb, float* rowadd, float* wb_frag,
                   float* wb_frag_ref, float* y, void* stream);
/* conv3x3(+bias) -> GroupNorm(+SiLU), chained as the graph walk chains them; fused != 0: the conv launch emits the per-channel
 * partial sums and the GroupNorm skips its statistics pass (the production path), fused == 0: the two-kernel GroupNorm. */
int agd_op_conv_groupnorm(const float* x_nchw, const float* w, const float* bias, const float* gamma, const float* beta, float* y_nchw,
                          int B, int Cin, int H, int W, int Cout, int groups, float eps, int silu, int fused, void* stream);
/* One implicit-GEMM launch stated field by field (igemm.hip launch_igemm): the entry fills the launcher's descriptor itself, so no ctx option
 * stands between a test and the launcher.  Every pointer is a device pointer.  Activations, weights and the residual are fp32 and are rounded
 * to bf16 by the entry (n_* = their element counts); bias / rowadd / ln_stats / ln_cs / gn_gamma / gn_beta are handed to the launch AS GIVEN
 * (address and all).  Outputs go into caller-allocated, caller-pre-filled buffers of the full pitch: `out` fp32 [n_out] (a bf16 launch gets
 * the buffer's values rounded to bf16 first and its result widened exactly afterwards, so a pre-filled bf16-exact sentinel survives where
 * the launch stores nothing), `gn_y` alike, `rowstat` / `colstat` fp32 tables written in place.  M = images * Hout * Wout; a linear layer is
 * images = 1, H = 1, W = rows.  w: [N][K] (w_per_image: [images][N][K]; batch > 1: as sW says), k = tap * (C0 + C1) + c, then the sc_C0 + sc_C1
 * shortcut columns; geglu: rows [values ; gates], interleaved by the entry as the loader does.
 * Returned in the struct: cfg = igemm_query's {BM, BN, K splits} (zeros where the query refuses), ran = {kernel family, slab pass} (AGD_IGEMM_*),
 * gn_fused, can_fuse_sc = igemm_can_fuse_shortcut of this launch (-1 without shortcut sources).  0, or -1 with the error text set. */
enum { AGD_IGEMM_NONE = 0, AGD_IGEMM_GENERAL = 1, AGD_IGEMM_HALO = 2, AGD_IGEMM_PCH = 3, AGD_IGEMM_PC = 4, AGD_IGEMM_8P = 5, AGD_IGEMM_SMAP = 6,
       AGD_IGEMM_WREG = 7 };
enum { AGD_IGEMM_SLAB_NONE = 0, AGD_IGEMM_SLAB_PLAIN = 1, AGD_IGEMM_SLAB_GN = 2 };
typedef struct agd_igemm_desc {
  int struct_size;                 /* sizeof(agd_igemm_desc), ABI guard */
  int images, H, W, C0, C1;        /* two NHWC sources [images][H][W][C0 | C1] */
  int ksize, stride, pad, up, hout, wout;   /* hout / wout > 0: override the output size (the asymmetric pad-0 stride-2 form) */
  int sc_C0, sc_C1;                /* conv_shortcut sources' channels */
  int N, K, w_per_image;
  int bias_mode, rowadd_ld, ldr, geglu, act, out_f32, ldo;
  int batch;
  int rowstat_slots, ln_slots, colstat_rows;
  int gn_groups, gn_silu, gn_keep_out;
  int halo, p8, smap, pc, kg2, wreg, xcd_block;
  float alpha, ln_invC, ln_eps, gn_eps;
  long long sA0, sA1, sW, sO, sR;
  long long n_src0, n_src1, n_sc0, n_sc1, n_w, n_res, n_out;
  const float* src0; const float* src1; const float* sc0; const float* sc1; const float* w;
  const float* bias; const float* rowadd; const float* residual;
  const float* ln_stats; const float* ln_cs; const float* gn_gamma; const float* gn_beta;
  float* out; float* gn_y; float* rowstat; float* colstat;
  int cfg[3]; int ran[2]; int gn_fused; int can_fuse_sc;     /* out */
} agd_igemm_desc;
int agd_op_igemm(agd_igemm_desc* d, void* stream);
int agd_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps,
                     void* stream);
/* the same; *inst (may be NULL) = which instantiation of the LayerNorm kernel ran, as 100 * lanes per row + vectors per lane (6404, 1605, 1610).
 * Both refuse rows < 1, C < 8, C % 8 != 0 and C > 2048. */
int agd_op_layernorm_ex(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps, int* inst,
                        void* stream);
/* q [B,Nq,H*D], k/v [B,Nk,H*D] fp32 -> o [B,Nq,H*D]; probs_out (may be NULL): [B,H,Nk,Nq] fp32, needs Nk<=96 */
int agd_op_attention(const float* q, const float* k, const float* v, float* o, int B, int H, int D, int Nq, int Nk,
                     float scale, float* probs_out, void* stream);
/* agd_op_attention reaching EVERY form of the attention kernel (causal order, an additive mask, a second K/V source, the fused operand
 * layouts of the production callers, partial recording), for per-kernel tests.  All operands packed fp32, rounded to bf16 by the entry:
 * q / o [B,Nq,H*D], k / v [B,Nk,H*D]; mask (may be NULL) [B,Nk] additive, broadcast over heads and queries; k2 / v2 (both or neither)
 * [B,Nk2,H*D], 1 <= Nk2 <= 64, attended after the Nk keys.  layout: the memory layout the entry builds for the kernel -- 0 packed rows of
 * pitch C; 1 q | k | v as the column blocks of one [B,N,3C] buffer (Nq == Nk); 2 k | v as the column blocks of one [B,Nk,2C] buffer (with
 * 1 and 2, k2 | v2 likewise share one [B,Nk2,2C] buffer).  The values, and so the result, do not depend on the layout.
 * record: 0 none (probs_out NULL); 1 probs_out [B,H,Nk,Nq] = every head's probabilities; 2 probs_out [B,Nk,Nq] = their sum over the
 * heads.  probs_out is zeroed first; only batch rows >= rec_b0 (0 .. B) and token rows < rec_T (1 .. Nk) are recorded.  Recording needs
 * Nk <= 96.  D in {32,40,64,80,128,160}.  Refused with a message, before anything is launched: the above, mask + causal, a second source
 * together with a mask, causal order or recording, and head-summed recording with a mask.  Syncs. */
int agd_op_attention_ex(const float* q, const float* k, const float* v, float* o, int B, int H, int D, int Nq, int Nk, float scale,
                        int causal, const float* mask, const float* k2, const float* v2, int Nk2, int layout, float* probs_out,
                        int record, int rec_b0, int rec_T, void* stream);
/* The recording kernel for contexts beyond 96 tokens alone (csrc/attention_long.hip: two passes over 64-key tiles, so that the recorded
 * probabilities are divided by the row sum over ALL keys).  Operands as agd_op_attention_ex; 97 <= Nk <= AGD_MAX_CONTEXT_TOKENS; layout 0
 * packed or 2 (k | v as the column blocks of one [B,Nk,2C] buffer).  probs_inout [B,H,Nk,Nq] is ADDED to, as the DAAM accumulators are (the
 * caller zeroes it): batch rows >= rec_b0 (0 .. B) and token rows < rec_T (1 .. Nk) only; the rest is not touched.  Refusals come with a
 * message, before anything is launched.  Syncs. */
int agd_op_attention_long(const float* q, const float* k, const float* v, float* o, int B, int H, int D, int Nq, int Nk, float scale,
                          int layout, float* probs_inout, int rec_b0, int rec_T, void* stream);
/* same, the probabilities summed over the heads (the recording form of the daam layers at latent resolution): probs_sum_out [B,Nk,Nq] */
int agd_op_attention_headsum(const float* q, const float* k, const float* v, float* o, int B, int H, int D, int Nq, int Nk,
                             float scale, float* probs_sum_out, void* stream);
/* The attention backward of the training seam in isolation (what agd_attn_processor_backward runs between its GEMMs): recompute
 * P = softmax(scale q k^T) per head, then the gradient of  sum(O . d_o) + sum(mean_heads(P)[b0:] . d_map)  w.r.t. q and kv.
 * q / d_o / dq [B,N,H*D], kv / dkv [B,T,2*H*D] (K columns, then V columns), d_map [B-b0,T,N]; d_o is the gradient of the per-head
 * attention output (before to_out).  d_o or d_map may be NULL, not both.  D in {32,40,64,80,128,160}, 1 <= T <= 96, 0 <= b0 <= B.
 * Operands are rounded to bf16, the arithmetic is fp32, dq / dkv are the bf16 results as fp32.  Syncs. */
int agd_op_attention_backward(const float* q, const float* kv, const float* d_o, const float* d_map, int b0, int B, int H, int D,
                              int N, int T, float scale, float* dq, float* dkv, void* stream);
/* hook.py:55 `maps.mean(dim=1)` in isolation: heads [Bp,H,T,N] fp32 -> map [Bp,T,N] = (heads summed in order h = 0, 1, ...) * (1/H).  Syncs. */
int agd_op_hook_headmean(const float* heads, int Bp, int H, int T, int N, float* map, void* stream);
int agd_op_bicubic_clamp_mean(const float* maps, int n_maps, int T, int side, int S, float* out, void* stream);

/* ---- export path on device, bit-exact with the reference's host code:
 * heat map fp32 [n][npix] -> uint8 by per-map min-max (+1e-8), x255, truncation   (data_generation.py:82-84) */
int agd_op_heatmap_u8(const float* hm, int n, int npix, unsigned char* out, void* stream);
/* uint8 [n][H][W][C] -> [n][oh][ow][C], identical to PIL `Image.resize((ow, oh))` (default BICUBIC) per image
 * (data_generation.py:60,85).  Syncs. */
int agd_op_resize_u8_pil(const unsigned char* in, int n, int H, int W, int C, int oh, int ow, unsigned char* out, void* stream);
/* rgb [npix][3] = [obj, fg, 255 - bg]; inv [npix] = 255 - bg (may be NULL)        (postprocess_heatmap.py:44-48) */
int agd_op_stack_heatmaps(const unsigned char* obj, const unsigned char* fg, const unsigned char* bg, long long npix,
                          unsigned char* rgb, unsigned char* inv, void* stream);

/* ---- LoRA (diffusers load_lora_weights + cross_attention_kwargs={"scale": s}): one adapter of low-rank updates on the UNet transformer
 * blocks' linears (attn1 / attn2 to_q, to_k, to_v, to_out.0; ff.net.0.proj; ff.net.2; proj_in; proj_out) and the text encoder's (q/k/v/out_proj,
 * fc1, fc2), merged on the device: W = bf16(float(W_base) + s * (alpha / rank) * up @ down), then every form finalize derived from W is
 * rewritten in place.  Call after agd_finalize.
 * agd_lora_add: target_key = the engine key agd_load_tensor saw ("unet.<diffusers key>", "text.encoder.layers.<l>.self_attn.q_proj.weight", ...;
 *   "controlnet.", "safety." and "vae." keys are refused); down fp32 [rank][in], up fp32 [out][rank] (host or device; 1x1-conv factors
 *   flattened).  Stages the factors and a bf16 copy of the target's base matrix (first touch); the weights stay at the base until
 *   agd_lora_set_scale.  A target takes one LoRA at a time.
 * agd_lora_set_scale: merges at scale s and re-derives (synchronous; allocates nothing).  s equal to the current scale: no work; s = 0: the
 *   base matrices.  Afterwards the projected context is stale: agd_unet_forward / the fused loops fail until agd_set_context runs again.
 * agd_lora_clear: the base matrices back (re-derived), the LoRA state freed. */
int agd_lora_add(agd_ctx* ctx, const char* target_key, const float* down, const float* up, int rank, float alpha);
int agd_lora_set_scale(agd_ctx* ctx, float s, void* stream);
int agd_lora_clear(agd_ctx* ctx);
int agd_lora_count(agd_ctx* ctx);                    /* targets staged */
float agd_lora_scale(agd_ctx* ctx);                  /* the scale the weights hold now */

/* ---- MultiDiffusion panorama (diffusers 0.21.2 StableDiffusionPanoramaPipeline [upstream-knowledge]; csrc/panorama.hip)
 * Views of a latent canvas Lh x Lw: nbh x nbw windows of `window` x `window` at (i stride, j stride), nbh = (Lh - window) / stride + 1,
 * view v = i * nbw + j (diffusers get_views order).
 * agd_op_window_gather: canvas fp32 [B][C][Lh][Lw] -> views [v0, v0 + n) of every panorama, fp32 [B * n][C][window][window], view-major
 *   within a panorama.  agd_op_window_mean: views [B * V][C][window][window] -> canvas, every element the fp32 sum of the views that cover it
 *   in ascending view order divided by their number (0 where no view covers it): a gather, deterministic, no atomics.  Both take any
 *   window / stride with each side at least the window.
 * agd_denoise_panorama: the DDIM loop on a canvas [batch][4][Lh][Lw] in place.  Per step every view is gathered, run through the CFG UNet
 *   and stepped on its own, view_batch views of every panorama per UNet call (<= 0: all views); then one overlap mean writes the canvas.
 *   Sizes: Lh, Lw multiples of `stride` and at least `window`, `window` a multiple of `stride`.  The context (agd_set_context) is the
 *   [2 * batch, T, D] of the prompts; the loop tiles its projections per view once per call.  A ControlNet schedule, a GLIGEN schedule or an
 *   inpainting state being set is an error.  DAAM: after agd_record_reset_hw(ctx, batch * views, window, window) the loop records one state
 *   per (panorama p, view v), image v * batch + p, for any view_batch (agd_daam_global reads one view's map).
 * agd_daam_global_panorama: out [rows][Lh][Lw] of panorama `img` of the last agd_denoise_panorama = the overlap mean of its views' global
 *   maps (each the agd_daam_global map at window x window).  This definition is this project's: daam has no panorama support. */
int agd_op_window_gather(const float* canvas, float* views, int B, int C, int Lh, int Lw, int window, int stride, int v0, int n, void* stream);
int agd_op_window_mean(const float* views, float* canvas, int B, int C, int Lh, int Lw, int window, int stride, void* stream);
int agd_denoise_panorama(agd_ctx* ctx, float* canvas, int batch, int Lh, int Lw, int window, int stride, int view_batch, int n_steps,
                         const float* timesteps, const float* alpha_t, const float* alpha_prev, float guidance, void* stream);
int agd_daam_global_panorama(agd_ctx* ctx, int img, int rows, float* out, void* stream);

/* ---- Region-based MultiDiffusion (Bar-Tal et al. 2023; the MultiDiffusion repository's region_based.py [upstream-knowledge], parity-unpinned:
 * diffusers 0.21.2 has no such pipeline; csrc/regions.hip).  R regions share ONE latent canvas [batch][4][Lh][Lw]; region 0 is the background.
 * Row (region r, image p) is r * batch + p everywhere: the latent masks [R][batch][Lh * Lw] fp32 (one value per latent pixel), the UNet batch
 * within a CFG half, the context rows and the DAAM states.  At most AGD_MAX_REGIONS regions.
 * agd_op_region_masks (seam for tests, and the pipeline's mask front end): pixel masks on the device, uint8 (set: > 127; px_f32 = 0) or fp32
 *   (set: > 0.5; px_f32 = 1), [per_image ? B : 1][R - 1][H][W] -> masks.  H / Lh and W / Lw must be whole; latent (y, x) reads pixel
 *   (y H / Lh, x W / Lw) (torch's nearest sample); row 0 is max(0, 1 - the sum of the foreground rows).  R = 1 reads no pixels.
 * agd_op_region_spread (seam for tests): x [R][B][C][Lh * Lw] from canvas [B][C][Lh * Lw].  idx == NULL (a step past the bootstrapping
 *   phase): every region is the canvas.  Else idx is a HOST array of R - 1 background indices in 0 .. n_bg - 1 and, for r >= 1,
 *   x = canvas m + (sa bgs[idx[r - 1]] + sb noise) (1 - m) with bgs [n_bg][C][Lh * Lw] and noise [B][C][Lh * Lw]; region 0 is the canvas.
 * agd_op_region_mean (seam for tests): canvas = sum_r m_r x_r / sum_r m_r, both sums in ascending r in fp32, one division per element; the
 *   sum itself (0) where no mask covers the element.  Deterministic, no atomics; any channel count.
 * agd_denoise_regions: the DDIM loop on the canvas in place.  Per step s: spread (bootstrapped while s < bootstrapping, with the step's
 *   sqrt_ac pair and idx row), the CFG UNet on the 2 R batch rows in ONE forward -- the context set by agd_set_context must hold
 *   [uncond x R batch | cond x R batch] -- the DDIM step on the R batch rows, then the masked mean.  Stateless: everything the call reads
 *   comes in the descriptor and nothing is kept.  With the DAAM recorder on it must hold R batch images at Lh x Lw
 *   (agd_record_reset_hw(ctx, R * batch, Lh, Lw)); agd_daam_global(ctx, r * batch + p, ...) is region r's map of image p.
 *   Refused by name before the first launch: a ControlNet, GLIGEN or T2I-Adapter schedule, an IP-Adapter image, either inpainting state, an
 *   InstructPix2Pix state, a Perturbed-Attention Guidance or DeepCache schedule, a guidance rescale, the hook.py recorder, a context over 96
 *   tokens, an inpainting UNet, and a bad descriptor.  FreeU and LoRA belong to the UNet and apply unchanged. */
#define AGD_MAX_REGIONS 8
typedef struct agd_regions_desc {
  int struct_size;                 /* sizeof(agd_regions_desc), ABI guard */
  int regions;                     /* R >= 1 */
  int bootstrapping;               /* 0 .. n_steps: the first steps whose foreground regions see a background outside their mask */
  int n_backgrounds;               /* N >= 1 when bootstrapping > 0 and R > 1 */
  const float* masks;              /* device [R][batch][Lh * Lw] */
  const float* noise;              /* device [batch][4][Lh][Lw]: the call's initial latents */
  const float* backgrounds;        /* device [N][4][Lh][Lw]: encoded constant-colour images, times the scaling factor */
  const int* idx;                  /* host [bootstrapping][R - 1], each in 0 .. N - 1 */
  const float* sqrt_ac;            /* host [bootstrapping][2]: (sqrt(ac_t), sqrt(1 - ac_t)) of the step */
} agd_regions_desc;
int agd_op_region_masks(const void* px, int px_f32, int per_image, float* masks, int R, int B, int H, int W, int Lh, int Lw, void* stream);
int agd_op_region_spread(const float* canvas, float* x, const float* masks, const float* noise, const float* bgs, int R, int B, int C, int Lh,
                         int Lw, int n_bg, const int* idx, float sa, float sb, void* stream);
int agd_op_region_mean(const float* x, const float* masks, float* canvas, int R, int B, int C, int Lh, int Lw, void* stream);
int agd_denoise_regions(agd_ctx* ctx, float* canvas, int batch, int Lh, int Lw, const agd_regions_desc* desc, int n_steps,
                        const float* timesteps, const float* alpha_t, const float* alpha_prev, float guidance, void* stream);

/* ---- FreeU (Si et al. 2023; diffusers >= 0.22 enable_freeu(s1, s2, b1, b2) / disable_freeu [upstream-knowledge]; csrc/freeu.hip): a
 * training-free re-weighting of the UNet decoder.  In up block i in {0, 1}, for every resnet of the block and immediately before its concat,
 *   hidden[:, : C / 2] *= b_i           (the first half of the backbone's channels)
 *   skip = fourier_filter(skip, 1, s_i) (the centred 2 x 2 block of the shifted 2-D spectrum times s_i: the frequencies {-1, 0} x {-1, 0})
 * with (b, s) = (b1, s1) in block 0 and (b2, s2) in block 1; the upsamplers, the transformers and every other block are untouched, and with a
 * ControlNet the filtered skip is the one with the residual added.  The filter runs as a rank-4 projection (seven real sums per image and
 * channel, no transform), any map size; both tensors of a resnet are written by ONE launch into fresh activations.
 * agd_freeu_set: persistent context state after agd_finalize, read by every later UNet evaluation (agd_unet_forward*, agd_denoise*,
 *   the InstructPix2Pix loop, agd_denoise_panorama) beside any conditioning state; needs finite values and at least two UNet levels.  A b of
 *   exactly 1 skips that block's scale, an s of exactly 1 its filter; all four 1 is agd_freeu_clear.  Suggested: SD-1.4 (0.9, 0.2, 1.2, 1.4),
 *   SD-1.5 (0.9, 0.2, 1.5, 1.6), SD-2.1 (0.9, 0.2, 1.4, 1.6).
 * agd_freeu_clear: the plain UNet again, launch for launch (bit-identical results).
 * agd_freeu_counts (seam for tests): the FreeU launches since agd_create -- counts[0] those that left GroupNorm partial sums for the concat
 *   norm, counts[1] those that left none (maps whose pixel count is no multiple of 64, or "gn_fused_stats" off).
 * agd_op_freeu (seam for tests): the production kernel on fp32 NCHW device tensors hidden [B][Ch][H][W] / skip [B][Cs][H][W], rounded to
 *   bf16 on the way in; the outputs are the bf16 results widened (b == 1 / s == 1: the rounded input itself).  Ch, Cs multiples of 8. */
int agd_freeu_set(agd_ctx* ctx, float s1, float s2, float b1, float b2);
int agd_freeu_clear(agd_ctx* ctx);
int agd_freeu_counts(agd_ctx* ctx, long long* counts);
int agd_op_freeu(const float* hidden_nchw, const float* skip_nchw, float* hidden_out, float* skip_out, int B, int Ch, int Cs, int H, int W,
                 float b, float s, void* stream);

/* ---- guidance_rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed"; diffusers 0.21.2
 * StableDiffusionPipeline.__call__(guidance_rescale=phi) -> rescale_noise_cfg [upstream-knowledge]; csrc/guidance.hip).  After the CFG combine
 *   m = eps_u + g (eps_c - eps_u),   f_b = 1 + phi (std(eps_c[b]) / std(m[b]) - 1),   m' = f_b m
 * with std over the (C, H, W) values of image b jointly, unbiased; m' is what the scheduler step sees (PLMS keeps m' in its history).  One
 * extra launch per model evaluation -- one workgroup per image, mean-shifted fp32 sums in a fixed order, so f_b is bit-identical between runs
 * and between an image alone and the same image in a batch -- and one multiply inside the step kernel.  std(m[b]) == 0 gives f_b = 1 (upstream
 * divides by zero there).
 * agd_guidance_rescale_set: context state after agd_finalize, read by agd_denoise* (DDIM), agd_denoise_plms* and agd_denoise_dpm* at every
 *   evaluation, until cleared; phi must be a finite number in [0, 1]; 0 is agd_guidance_rescale_clear.  The InstructPix2Pix loop and
 *   agd_denoise_panorama refuse a set state before their first launch; agd_cfg_ddim_step* never rescales.
 * agd_guidance_rescale_clear: the plain loops again, launch for launch (bit-identical results).
 * agd_guidance_rescale_counts (seam for tests): the factor launches since agd_create.
 * agd_op_guidance_rescale (seam for tests): the factor kernel alone on device memory -- eps fp32 [2 B][HW][ldc], rows [0, B) unconditional and
 *   [B, 2 B) conditional, channels c < C of every ldc-wide row -> factor [B].  C * HW >= 2.  ctx may be NULL (it only keeps the error text). */
int agd_guidance_rescale_set(agd_ctx* ctx, float phi);
int agd_guidance_rescale_clear(agd_ctx* ctx);
int agd_guidance_rescale_counts(agd_ctx* ctx, long long* launches);
int agd_op_guidance_rescale(agd_ctx* ctx, const float* eps, int ldc, int B, int C, int HW, float guidance, float phi, float* factor, void* stream);

/* ---- Perturbed-Attention Guidance (Ahn et al. 2024, "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance"; diffusers >= 0.30
 * StableDiffusionPAGPipeline [upstream-knowledge]; csrc/pag.hip).  Where its scale p_i is > 0, model evaluation i runs a third UNet branch on
 * the conditional rows (same latents, timestep and text context) in which every applied self-attention layer computes to_out(to_v(norm1(h)))
 * -- the attention map replaced by the identity -- and the step sees
 *   eps = e_u + s (e_c - e_u) + p_i (e_c - e_p).
 * The branch is one extra B-row walk; it records nothing (the DAAM / hook.py recorders see the main walk's conditional half as without PAG)
 * and takes its K/V from the conditional half of what agd_set_context projected.  q and k of a perturbed layer are still computed and ignored.
 * agd_pag_set: context state after agd_finalize, until cleared.  scales: one finite p_i >= 0 per model evaluation of the calls to come
 *   (agd_denoise*, agd_denoise_plms*, agd_denoise_dpm* check n against their evaluations; an evaluation with p_i == 0 is the plain one, launch
 *   for launch).  layers: n_layers attn1 module names ("mid_block.attentions.0.transformer_blocks.0.attn1"); a name that is no self-attention
 *   layer of this UNet is refused by name; n_layers == 0 perturbs nothing (the third walk still runs).  With the state set,
 *   agd_unet_forward_hw under a schedule of length 1 with p_0 > 0 runs ALL its rows as the perturbed branch against the context as it is,
 *   recording nothing.  Refused by name before the first launch: a ControlNet, GLIGEN or T2I-Adapter schedule, an active IP-Adapter, either
 *   inpainting state, an InstructPix2Pix state, agd_denoise_panorama, agd_unet_forward_ts*, and a set guidance rescale.
 * agd_pag_clear: the plain loops again, launch for launch (bit-identical results).
 * agd_pag_counts (seam for tests): perturbed walks run, and perturbed self-attention layers launched, since agd_create.
 * agd_op_pag_v_rows (seam for tests): att[m][0:C] = qkv[m][2C:3C] on device bf16 memory, rows of 3 C -> rows of C; C % 8 != 0 is refused.
 * agd_op_pag_fold (seam for tests): eps fp32 [3][n] on the device (uncond | cond | perturbed), in place: d = p (e_c - e_p) with the product
 *   rounded on its own, e_u += d, e_c += d.  For both seams ctx may be NULL (it only keeps the error text). */
int agd_pag_set(agd_ctx* ctx, const float* scales, int n, const char* const* layers, int n_layers);
int agd_pag_clear(agd_ctx* ctx);
int agd_pag_counts(agd_ctx* ctx, long long* walks, long long* layers);
int agd_op_pag_v_rows(agd_ctx* ctx, const void* qkv, void* att, int M, int C, void* stream);
int agd_op_pag_fold(agd_ctx* ctx, float* eps, long long n, float p, void* stream);

/* ---- DeepCache (Ma, Fang, Wang 2024, "DeepCache: Accelerating Diffusion Models for Free"; the upstream DeepCacheSDHelper's uniform schedule
 * [upstream-knowledge]; csrc/deepcache.hip).  Number the UNet's skip tensors in the order the down path makes them: s_0 = conv_in's output,
 * s_1 .. s_lpb the outputs of the layers of down block 0 (lpb = layers_per_block), then the downsampler's, and so on; U_k is the up layer that
 * consumes s_k, so U_lpb .. U_0 are layers 0 .. lpb of the last up block.  A SHALLOW evaluation at branch b runs the time embedding, conv_in
 * and layers 0 .. b of down block 0, then U_{b+1} .. U_0 and conv_norm_out / conv_out; the hidden-state input of U_{b+1} is the one that entered
 * that layer at the most recent FULL evaluation, kept with its GroupNorm partial sums in a slot of the context outside the activation arena.
 * A full evaluation is the plain walk, launch for launch, plus -- when the next evaluation is shallow -- one copy launch into the slot.
 * The recorders (DAAM, hook.py) see exactly the attn2 layers that run; FreeU acts inside the shallow walk where it touches the last up block.
 * agd_deepcache_set: context state after agd_finalize, until cleared.  full_flags: one flag per model evaluation of the calls to come (1 = full,
 *   0 = shallow), counted from evaluation 0 of the call (agd_denoise*, agd_denoise_plms* with its extra evaluation, agd_denoise_dpm* check n
 *   against their evaluations); full_flags[0] must be 1; all ones is the plain call, bit for bit, and captures nothing.  branch: 0 ..
 *   layers_per_block - 1, anything else is refused by name.  Refused by name before the first launch: a ControlNet, GLIGEN or T2I-Adapter
 *   schedule, an active IP-Adapter, either inpainting state, an InstructPix2Pix state, a Perturbed-Attention Guidance schedule,
 *   agd_denoise_panorama and agd_unet_forward_ts*.  agd_unet_forward_hw does not read the state.
 * agd_deepcache_clear: the plain loops again, launch for launch.
 * agd_deepcache_counts (seam for tests): out[0] = full evaluations that captured, out[1] = shallow evaluations, since agd_create.
 * agd_deepcache_forward_hw (seam for tests and tools; agd_unet_forward_hw's arguments): shallow == 0 is the plain forward plus a capture for
 *   `branch`, shallow == 1 the shallow walk on that capture.  A capture is valid for one (rows, Lh, Lw, branch); a fused loop invalidates it at
 *   its start and its end, and so do agd_set_context, a LoRA scale change, agd_freeu_set / agd_freeu_clear, agd_deepcache_set and
 *   agd_deepcache_clear.  shallow == 1 without a valid capture is refused on the host; nothing is launched.  It does not read the schedule.
 *   A loop that is refused (a conflicting state, a wrong schedule length) fails before it invalidates anything: it leaves the schedule, the
 *   counters and a capture made through this seam as they were.
 * agd_op_deepcache_capture (seam for tests): the capture launch alone on two device regions of bytes0 / bytes1 bytes (either may be 0), each
 *   16-byte aligned, copied bit for bit.  ctx may be NULL (it only keeps the error text). */
int agd_deepcache_set(agd_ctx* ctx, const int* full_flags, int n, int branch);
int agd_deepcache_clear(agd_ctx* ctx);
int agd_deepcache_counts(agd_ctx* ctx, long long* out);
int agd_deepcache_forward_hw(agd_ctx* ctx, const float* sample, int rows, int Lh, int Lw, float timestep, int branch, int shallow, float* out, void* stream);
int agd_op_deepcache_capture(agd_ctx* ctx, const void* src0, void* dst0, long long bytes0, const void* src1, void* dst1, long long bytes1, void* stream);

/* ---- Semantic Guidance (Brack et al. 2023, "SEGA: Instructing Text-to-Image Models using Semantic Guidance"; diffusers 0.21.2
 * SemanticStableDiffusionPipeline [upstream-knowledge]; csrc/sega.hip).  Up to AGD_MAX_EDIT_CONCEPTS edit concepts, shared by the images of a
 * call, each with a UNet branch of its own.  Evaluation i counts the model evaluations of a call from 0 (PLMS's extra evaluation has its own
 * index).  For concept k, in fp32 and in this operation order:
 *   v_k = (e_k - e_u) * coef[i][k]
 *   thr = quantile(|v_k| over the HW latent pixels, q[k]) per image and channel: p = q (HW - 1) in double, lo = floor(p), f = float(p - lo),
 *         a, b the lo-th and min(lo + 1, HW - 1)-th smallest values, thr = min(b, a + f (b - a))
 *   G_k = v_k where |v_k| >= thr, else 0;  a concept with coef[i][k] == 0 contributes exactly 0 and its eps rows are not read
 *   g = sum_k w_mom[i][k] G_k + mom_scale m;   added = sum_k w_add[i][k] G_k + add_mom[i] mom_scale m;   m <- mom_beta m + (1 - mom_beta) g
 * with the momentum m fp32, one value per image and latent element, zero at the start of every fused loop (and of every agd_unet_forward_hw).
 * `added` lands on both e_u and e_c, so the schedulers' two-way step kernels compute e_u + s (e_c - e_u) + added unchanged.
 * agd_sega_set: context state after agd_finalize, until cleared; the descriptor's host arrays are copied.  coef, w_mom, w_add: [n_evals][concepts],
 *   add_mom: [n_evals], q: [concepts] in [0, 1]; every number finite.  With the state set, agd_set_context must hold (2 + K) B rows:
 *   [uncond x B | cond x B | concept_0 x B | ... | concept_{K-1} x B]; the loops refuse any other row count by name.  Per evaluation of
 *   agd_denoise*, agd_denoise_plms*, agd_denoise_dpm* (n_evals is checked against theirs): the main 2 B-row walk exactly as without the state
 *   (it sees a context of 2 B rows: shared prefix and recorders unchanged); where any coef[i][k] != 0 one non-recording walk of K B rows
 *   against context rows [2 B, (2 + K) B) on K copies of the conditional rows' input, into eps rows [2 B, (2 + K) B); the threshold launch
 *   (skipped with the walk) and the fold launch (every evaluation: momentum outlives cool-down); then the step.
 *   agd_unet_forward_hw with the state set and n_evals == 1 runs one such evaluation on its (2 + K) B sample rows -- the concept walk always
 *   runs there, on copies of the conditional rows -- and returns all rows: the folded pair, then the concept rows as the walk left them.
 *   Refused by name before the first launch: a ControlNet, GLIGEN or T2I-Adapter schedule, either inpainting state, an InstructPix2Pix state,
 *   a Perturbed-Attention Guidance or DeepCache schedule, an active IP-Adapter, a set guidance rescale, agd_denoise_panorama,
 *   agd_denoise_regions, agd_deepcache_forward_hw, agd_unet_forward_ts*, a context over 96 tokens, and out_channels != 4.
 * agd_sega_clear: the plain loops again, launch for launch (bit-identical results).
 * agd_sega_counts (seam for tests): concept walks and folds run since agd_create.
 * agd_op_sega_threshold (seam for tests): eps fp32 [(2 + K) B][HW][4] on the device, coef / q host arrays of K -> thr fp32 [B][K][4] on the
 *   device.  One workgroup per (image, concept): radix select on the bit patterns of |v| with integer LDS atomics (two runs give equal bits);
 *   the patterns are staged in LDS up to 9216 pixels and re-read through L2 beyond.  Any HW >= 1.
 * agd_op_sega_fold (seam for tests): the fold alone, eps rows [0, 2 B) and m [B][HW][4] updated in place, the concept rows left as they are.
 *   For both seams ctx may be NULL (it only keeps the error text). */
#define AGD_MAX_EDIT_CONCEPTS 8
typedef struct agd_sega_desc {
  int struct_size;                 /* sizeof(agd_sega_desc), ABI guard */
  int concepts;                    /* K: 1 .. AGD_MAX_EDIT_CONCEPTS */
  int n_evals;                     /* model evaluations of the calls to come */
  float mom_scale, mom_beta;       /* edit_momentum_scale, edit_mom_beta */
  const float* coef;               /* [n_evals][concepts] */
  const double* q;                 /* [concepts] */
  const float* w_mom;              /* [n_evals][concepts] */
  const float* w_add;              /* [n_evals][concepts] */
  const float* add_mom;            /* [n_evals] */
} agd_sega_desc;
int agd_sega_set(agd_ctx* ctx, const agd_sega_desc* desc);
int agd_sega_clear(agd_ctx* ctx);
int agd_sega_counts(agd_ctx* ctx, long long* walks, long long* folds);
int agd_op_sega_threshold(agd_ctx* ctx, const float* eps, int B, int K, int HW, const float* coef, const double* q, float* thr, void* stream);
int agd_op_sega_fold(agd_ctx* ctx, float* eps, float* m, const float* thr, int B, int K, int HW, const float* coef, const float* w_mom,
                     const float* w_add, float add_mom, float mom_scale, float mom_beta, void* stream);

/* ---- per-kernel-class timing (HIP events on the launch stream) */
#define AGD_N_CLASSES 11
int agd_profile_begin(agd_ctx* ctx);
int agd_profile_end(agd_ctx* ctx, double* ms, double* flops, long long* launches);  /* arrays of AGD_N_CLASSES; syncs */
/* the same plus, per class, the algorithmic HBM bytes and roof_ms = Sum over launches of max(flop / mfma_peak_flops,
 * bytes / hbm_peak_bytes) [ms]: the time each launch's BINDING roof allows (bench.py's per-class roofline fractions);
 * roof_ms_hbm_bound (may be NULL): the part of roof_ms that came from launches whose binding roof is HBM. */
int agd_profile_end_ex(agd_ctx* ctx, double mfma_peak_flops, double hbm_peak_bytes, double* ms, double* flops, double* bytes,
                       double* roof_ms, double* roof_ms_hbm_bound, long long* launches);
const char* agd_profile_class_name(int cls);

#ifdef AGD_EXPERIMENTS
/* Only in the experiments library (`make -C agenda_amd/csrc exp` -> agenda_amd/libagenda_hip_exp.so); the product library exports none of these. */
/* ---- kernel micro-benchmarks (tools/kbench.py): random bf16 operands, HIP-event timing of `iters` launches -> ms per launch */
int agd_bench_conv(int B, int H, int W, int C0, int C1, int Cout, int ksize, int stride, int up, int geglu, int with_residual,
                   int iters, double* ms_out);
int agd_bench_attention(int B, int H, int D, int Nq, int Nk, int record, int iters, double* ms_out);
/* one launch with cold weights (caches flushed per iteration); warm: 0 cold, 1 streaming touch of the weights timed with the launch, 2 weights hot */
int agd_bench_conv_cold(int B, int H, int W, int C0, int Cout, int ksize, int geglu, int with_residual, int warm, int iters, double* ms_out);
int agd_bench_groupnorm(int B, int HW, int C, int iters, double* ms_out);
int agd_bench_groupnorm_ex(int B, int HW, int C0, int C1, int fused_stats, int iters, double* ms_out);
#endif /* AGD_EXPERIMENTS */

const char* agd_version(void);

#ifdef __cplusplus
}
#endif
#endif
