"""Architecture configs for the Stable-Diffusion UNet / VAE decoder on the AGenDA generation path.

The reference never spells these out: it loads them from the checkpoint's ``unet/config.json`` /
``vae/config.json`` via ``StableDiffusionPipeline.from_pretrained`` (reference
data_generation/data_generation.py:30).  The values below restate the public SD-1.x / SD-2.1
configs [upstream-knowledge, SURVEY.md §8a/§8d] and give every parameter the diffusers
state-dict key so a real checkpoint maps 1:1 (`agd_load_tensor`).
"""
from __future__ import annotations

from dataclasses import dataclass, field, asdict
from typing import Dict, List, Tuple


@dataclass
class UNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    # True = CrossAttnDownBlock2D / CrossAttnUpBlock2D at that level
    down_cross: Tuple[bool, ...] = (True, True, True, False)
    layers_per_block: int = 2
    # diffusers' `attention_head_dim` is in fact the NUMBER of heads for SD-1.x/2.x
    num_heads: Tuple[int, ...] = (8, 8, 8, 8)
    cross_attention_dim: int = 768
    use_linear_projection: bool = False
    norm_num_groups: int = 32
    time_embed_dim_mult: int = 4

    @property
    def up_cross(self) -> Tuple[bool, ...]:
        return tuple(reversed(self.down_cross))


@dataclass
class VAEConfig:
    latent_channels: int = 4
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.18215


@dataclass
class SchedulerConfig:
    """DDIM as configured for SD [upstream-knowledge, SURVEY.md §8a row S1]."""
    num_train_timesteps: int = 1000
    beta_start: float = 0.00085
    beta_end: float = 0.012
    steps_offset: int = 1
    set_alpha_to_one: bool = False
    prediction_type: str = "epsilon"  # "v_prediction" for SD-2.1 768
    skip_prk_steps: bool = True       # PNDM only: SD checkpoints set it (pure PLMS); False (Runge-Kutta warm-up) is refused, not ignored
    # DPMSolverMultistepScheduler only (any other value of the solver keys is refused, not ignored)
    use_karras_sigmas: bool = False
    timestep_spacing: str = "linspace"   # DPM's own spacing; DDIM's is ddim_timestep_spacing below, PNDM always runs "leading"
    algorithm_type: str = "dpmsolver++"
    solver_order: int = 2
    solver_type: str = "midpoint"
    lower_order_final: bool = True
    # DDIMScheduler only (img2img's DDIM table follows them; PNDM and DPM-Solver++ refuse anything but these defaults, by name)
    ddim_timestep_spacing: str = "leading"   # "leading" | "trailing" | "linspace"
    rescale_betas_zero_snr: bool = False     # Lin et al. 2023: the last timestep carries pure noise (alphas_cumprod[-1] == 0)


@dataclass
class TextConfig:
    """CLIP text encoder (`pipeline.text_encoder`; transformers CLIPTextConfig fields). Defaults = SD-1.x ViT-L/14."""
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    vocab_size: int = 49408
    max_position_embeddings: int = 77
    hidden_act: str = "quick_gelu"       # "gelu" for the OpenCLIP encoder of SD-2.x
    layer_norm_eps: float = 1e-5


@dataclass
class SafetyConfig:
    """The safety checker (`pipeline.safety_checker`, diffusers StableDiffusionSafetyChecker): its CLIP vision tower under the
    transformers CLIPVisionConfig field names, the CLIPConfig `projection_dim`, the concept counts, and the CLIPImageProcessor
    settings of `feature_extractor/preprocessor_config.json`.  Defaults = the SD-1.x checker (ViT-L/14 at 224 px, 3 special-care
    and 17 concept embeddings)."""
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    num_channels: int = 3
    image_size: int = 224
    patch_size: int = 14
    hidden_act: str = "quick_gelu"
    layer_norm_eps: float = 1e-5
    projection_dim: int = 768
    n_special: int = 3
    n_concepts: int = 17
    # CLIPImageProcessor (resize shortest edge -> center crop -> rescale -> normalize, PIL BICUBIC)
    size: int = 224
    crop_size: int = 224
    resample: int = 3
    rescale_factor: float = 1 / 255
    image_mean: Tuple[float, float, float] = (0.48145466, 0.4578275, 0.40821073)
    image_std: Tuple[float, float, float] = (0.26862954, 0.26130258, 0.27577711)


# transformers CLIPVisionConfig / CLIPConfig defaults: what a key missing from safety_checker/config.json means
_CLIP_VISION_DEFAULTS = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, num_channels=3,
                             image_size=224, patch_size=32, hidden_act="quick_gelu", layer_norm_eps=1e-5)
_CLIP_PROJECTION_DIM_DEFAULT = 512


def _edge(v, what: str) -> int:
    """`size` / `crop_size` of a preprocessor config: an int, {"shortest_edge": n} or {"height": n, "width": n}."""
    if isinstance(v, bool):
        raise ValueError(f"preprocessor {what}: {v!r} is not a size")
    if isinstance(v, (int, float)):
        return int(v)
    if isinstance(v, dict):
        if "shortest_edge" in v and len(v) == 1:
            return int(v["shortest_edge"])
        if set(v) == {"height", "width"} and v["height"] == v["width"]:
            return int(v["height"])
    raise ValueError(f"preprocessor {what} {v!r} is not supported (an int, {{'shortest_edge': n}} or a square {{'height', 'width'}})")


def safety_config_from_json(clip_cfg: dict, preprocessor: dict, n_special: int = 3, n_concepts: int = 17) -> SafetyConfig:
    """SafetyConfig from `safety_checker/config.json` (a CLIPConfig: `vision_config`, else the older `vision_config_dict`, and the
    top-level `projection_dim`) and `feature_extractor/preprocessor_config.json`.  Preprocessor settings other than resize ->
    center crop -> rescale by 1/255 -> normalize with BICUBIC (resample 3) are refused, not ignored: the device front end runs
    exactly that chain."""
    vis = clip_cfg.get("vision_config") or clip_cfg.get("vision_config_dict") or {}
    v = {k: vis.get(k, d) for k, d in _CLIP_VISION_DEFAULTS.items()}
    pp = dict(preprocessor)
    for flag in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
        if not pp.get(flag, True):
            raise ValueError(f"preprocessor_config: {flag}=False is not supported (the checker runs resize -> center crop -> rescale -> normalize)")
    if int(pp.get("resample", 3)) != 3:
        raise ValueError(f"preprocessor_config: resample={pp['resample']} is not supported (only 3, BICUBIC)")
    rf = float(pp.get("rescale_factor", 1 / 255))
    if abs(rf - 1 / 255) > 1e-12:
        raise ValueError(f"preprocessor_config: rescale_factor={rf} is not supported (only 1/255)")
    for k in ("do_pad", "do_flip_channel_order", "do_reduce_labels"):
        if pp.get(k):
            raise ValueError(f"preprocessor_config: {k}=True is not supported")
    size = _edge(pp.get("size", 224), "size")
    crop = _edge(pp.get("crop_size", 224), "crop_size")
    if size != crop:
        raise ValueError(f"preprocessor_config: size {size} != crop_size {crop} is not supported (square images: the crop must be the identity)")
    if crop != v["image_size"]:
        raise ValueError(f"preprocessor_config: crop_size {crop} != vision image_size {v['image_size']}")
    mean = tuple(float(x) for x in pp.get("image_mean", SafetyConfig.image_mean))
    std = tuple(float(x) for x in pp.get("image_std", SafetyConfig.image_std))
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("preprocessor_config: image_mean / image_std must have 3 entries")
    return SafetyConfig(projection_dim=int(clip_cfg.get("projection_dim", _CLIP_PROJECTION_DIM_DEFAULT)), n_special=n_special,
                        n_concepts=n_concepts, size=size, crop_size=crop, resample=3, rescale_factor=rf, image_mean=mean, image_std=std, **v)


@dataclass
class SDConfig:
    name: str = "sd15"
    unet: UNetConfig = field(default_factory=UNetConfig)
    vae: VAEConfig = field(default_factory=VAEConfig)
    sched: SchedulerConfig = field(default_factory=SchedulerConfig)
    max_tokens: int = 77
    vae_scale_factor: int = 8
    default_sample_size: int = 64
    text: "TextConfig | None" = None     # None: no device text encoder (synthetic / external embeddings)
    safety: "SafetyConfig | None" = None  # None: no safety checker (nothing is blacked out)

    def to_dict(self):
        return asdict(self)


def sd15() -> SDConfig:
    return SDConfig(name="sd15")


def sd21() -> SDConfig:
    return SDConfig(
        name="sd21",
        unet=UNetConfig(num_heads=(5, 10, 20, 20), cross_attention_dim=1024, use_linear_projection=True),
        sched=SchedulerConfig(prediction_type="v_prediction"),
        default_sample_size=96,
    )


def tiny(cross_dim: int = 64) -> SDConfig:
    """Small config (same topology, 64-multiples of channels) for fast CPU/GPU plumbing tests."""
    return SDConfig(
        name="tiny",
        unet=UNetConfig(block_out_channels=(64, 128, 128, 128), num_heads=(2, 2, 2, 2),
                        cross_attention_dim=cross_dim),
        vae=VAEConfig(block_out_channels=(64, 64, 128, 128)),
        default_sample_size=16,
    )


def tiny40() -> SDConfig:
    """Small config with SD-1.x head dims 40/80 (C=320/640 at 8 heads) but only two levels."""
    return SDConfig(
        name="tiny40",
        unet=UNetConfig(block_out_channels=(320, 640), down_cross=(True, False), num_heads=(8, 8),
                        cross_attention_dim=128, layers_per_block=1),
        vae=VAEConfig(block_out_channels=(64, 128), layers_per_block=1),
        default_sample_size=16,
    )


def tiny21() -> SDConfig:
    """SD-2.1-style small config: linear proj_in/out, head dim 64, v-prediction (run it at latent 24 to get
    the ragged 768-px-like token counts 576 / 144 / 36 / 9)."""
    return SDConfig(
        name="tiny21",
        unet=UNetConfig(block_out_channels=(64, 128, 128, 128), num_heads=(1, 2, 2, 2), cross_attention_dim=128,
                        use_linear_projection=True),
        vae=VAEConfig(block_out_channels=(64, 64, 128, 128)),
        sched=SchedulerConfig(prediction_type="v_prediction"),
        default_sample_size=24,
    )


CONFIGS = {"sd15": sd15, "sd21": sd21, "tiny": tiny, "tiny40": tiny40, "tiny21": tiny21}


def inpaint_variant(cfg: SDConfig) -> SDConfig:
    """`cfg` with an inpainting UNet: in_channels = latents + mask + masked-image latents (9 for SD); everything else unchanged."""
    import copy
    out = copy.deepcopy(cfg)
    out.unet.in_channels = out.unet.out_channels + 1 + out.vae.latent_channels
    out.name = cfg.name + "-inpaint"
    return out


def ip2p_variant(cfg: SDConfig) -> SDConfig:
    """`cfg` with an InstructPix2Pix UNet: in_channels = latents + image latents (8 for SD); everything else unchanged."""
    import copy
    out = copy.deepcopy(cfg)
    out.unet.in_channels = out.unet.out_channels + out.vae.latent_channels
    out.name = cfg.name + "-ip2p"
    return out


def inpaint_flavour(cfg: SDConfig) -> str:
    """How a UNet inpaints [upstream-knowledge: diffusers 0.21.2 StableDiffusionInpaintPipeline]: "concat" when it takes latents + mask +
    masked-image latents (in_channels = out_channels + 1 + the VAE's latent channels: 9 for SD), "blend" when it takes the latents only
    (the latents are blended with the noised image latents after every step).  Any other width raises."""
    u = cfg.unet
    if u.in_channels == u.out_channels:
        return "blend"
    if u.in_channels == u.out_channels + 1 + cfg.vae.latent_channels:
        return "concat"
    raise ValueError(f"inpainting needs a UNet of {u.out_channels} or {u.out_channels + 1 + cfg.vae.latent_channels} input channels "
                     f"(latents, or latents + mask + masked-image latents), this one takes {u.in_channels}")


def text_param_shapes(t: TextConfig) -> Dict[str, tuple]:
    """transformers CLIPTextModel state-dict keys (without the `text_model.` prefix of transformers 4.x)."""
    H, I = t.hidden_size, t.intermediate_size
    p: Dict[str, tuple] = {"embeddings.token_embedding.weight": (t.vocab_size, H),
                           "embeddings.position_embedding.weight": (t.max_position_embeddings, H)}
    for l in range(t.num_hidden_layers):
        L = f"encoder.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            p[L + f"self_attn.{n}.weight"] = (H, H)
            p[L + f"self_attn.{n}.bias"] = (H,)
        for n in ("layer_norm1", "layer_norm2"):
            p[L + n + ".weight"] = (H,)
            p[L + n + ".bias"] = (H,)
        p[L + "mlp.fc1.weight"] = (I, H); p[L + "mlp.fc1.bias"] = (I,)
        p[L + "mlp.fc2.weight"] = (H, I); p[L + "mlp.fc2.bias"] = (H,)
    p["final_layer_norm.weight"] = (H,)
    p["final_layer_norm.bias"] = (H,)
    return p


def safety_param_shapes(s: SafetyConfig) -> Dict[str, tuple]:
    """diffusers StableDiffusionSafetyChecker state-dict keys (`vision_model` is a transformers CLIPVisionModel, hence the doubled
    `vision_model.vision_model.` prefix)."""
    H, I, P = s.hidden_size, s.intermediate_size, s.projection_dim
    g = s.image_size // s.patch_size
    V = "vision_model.vision_model."
    p: Dict[str, tuple] = {V + "embeddings.class_embedding": (H,),
                           V + "embeddings.patch_embedding.weight": (H, s.num_channels, s.patch_size, s.patch_size),
                           V + "embeddings.position_embedding.weight": (g * g + 1, H),
                           V + "pre_layrnorm.weight": (H,), V + "pre_layrnorm.bias": (H,)}
    for l in range(s.num_hidden_layers):
        L = V + f"encoder.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            p[L + f"self_attn.{n}.weight"] = (H, H)
            p[L + f"self_attn.{n}.bias"] = (H,)
        for n in ("layer_norm1", "layer_norm2"):
            p[L + n + ".weight"] = (H,)
            p[L + n + ".bias"] = (H,)
        p[L + "mlp.fc1.weight"] = (I, H); p[L + "mlp.fc1.bias"] = (I,)
        p[L + "mlp.fc2.weight"] = (H, I); p[L + "mlp.fc2.bias"] = (H,)
    p[V + "post_layernorm.weight"] = (H,)
    p[V + "post_layernorm.bias"] = (H,)
    p["visual_projection.weight"] = (P, H)
    p["concept_embeds"] = (s.n_concepts, P)
    p["special_care_embeds"] = (s.n_special, P)
    p["concept_embeds_weights"] = (s.n_concepts,)
    p["special_care_embeds_weights"] = (s.n_special,)
    return p


# ------------------------------------------------------------------------------------------
# Parameter inventory: diffusers state-dict key -> shape
# ------------------------------------------------------------------------------------------
def _resnet(p: Dict[str, tuple], pre: str, cin: int, cout: int, temb: int | None):
    p[pre + "norm1.weight"] = (cin,)
    p[pre + "norm1.bias"] = (cin,)
    p[pre + "conv1.weight"] = (cout, cin, 3, 3)
    p[pre + "conv1.bias"] = (cout,)
    if temb:
        p[pre + "time_emb_proj.weight"] = (cout, temb)
        p[pre + "time_emb_proj.bias"] = (cout,)
    p[pre + "norm2.weight"] = (cout,)
    p[pre + "norm2.bias"] = (cout,)
    p[pre + "conv2.weight"] = (cout, cout, 3, 3)
    p[pre + "conv2.bias"] = (cout,)
    if cin != cout:
        p[pre + "conv_shortcut.weight"] = (cout, cin, 1, 1)
        p[pre + "conv_shortcut.bias"] = (cout,)


def _transformer(p: Dict[str, tuple], pre: str, c: int, ctx: int, linear_proj: bool):
    p[pre + "norm.weight"] = (c,)
    p[pre + "norm.bias"] = (c,)
    pw = (c, c) if linear_proj else (c, c, 1, 1)
    p[pre + "proj_in.weight"] = pw
    p[pre + "proj_in.bias"] = (c,)
    t = pre + "transformer_blocks.0."
    for n in ("norm1", "norm2", "norm3"):
        p[t + n + ".weight"] = (c,)
        p[t + n + ".bias"] = (c,)
    for a, kd in (("attn1", c), ("attn2", ctx)):
        p[t + a + ".to_q.weight"] = (c, c)
        p[t + a + ".to_k.weight"] = (c, kd)
        p[t + a + ".to_v.weight"] = (c, kd)
        p[t + a + ".to_out.0.weight"] = (c, c)
        p[t + a + ".to_out.0.bias"] = (c,)
    p[t + "ff.net.0.proj.weight"] = (8 * c, c)
    p[t + "ff.net.0.proj.bias"] = (8 * c,)
    p[t + "ff.net.2.weight"] = (c, 4 * c)
    p[t + "ff.net.2.bias"] = (c,)
    p[pre + "proj_out.weight"] = pw
    p[pre + "proj_out.bias"] = (c,)


def unet_param_shapes(cfg: UNetConfig) -> Dict[str, tuple]:
    p: Dict[str, tuple] = {}
    boc = cfg.block_out_channels
    temb = boc[0] * cfg.time_embed_dim_mult
    p["conv_in.weight"] = (boc[0], cfg.in_channels, 3, 3)
    p["conv_in.bias"] = (boc[0],)
    p["time_embedding.linear_1.weight"] = (temb, boc[0])
    p["time_embedding.linear_1.bias"] = (temb,)
    p["time_embedding.linear_2.weight"] = (temb, temb)
    p["time_embedding.linear_2.bias"] = (temb,)
    ch = boc[0]
    for i, co in enumerate(boc):
        for j in range(cfg.layers_per_block):
            _resnet(p, f"down_blocks.{i}.resnets.{j}.", ch, co, temb)
            ch = co
            if cfg.down_cross[i]:
                _transformer(p, f"down_blocks.{i}.attentions.{j}.", co, cfg.cross_attention_dim,
                             cfg.use_linear_projection)
        if i != len(boc) - 1:
            p[f"down_blocks.{i}.downsamplers.0.conv.weight"] = (co, co, 3, 3)
            p[f"down_blocks.{i}.downsamplers.0.conv.bias"] = (co,)
    mid = boc[-1]
    _resnet(p, "mid_block.resnets.0.", mid, mid, temb)
    _transformer(p, "mid_block.attentions.0.", mid, cfg.cross_attention_dim, cfg.use_linear_projection)
    _resnet(p, "mid_block.resnets.1.", mid, mid, temb)
    rev = list(reversed(boc))
    ch = rev[0]
    for i, co in enumerate(rev):
        prev_out = ch
        in_ch = rev[min(i + 1, len(rev) - 1)]
        for j in range(cfg.layers_per_block + 1):
            skip = in_ch if j == cfg.layers_per_block else co
            rin = prev_out if j == 0 else co
            _resnet(p, f"up_blocks.{i}.resnets.{j}.", rin + skip, co, temb)
            if cfg.up_cross[i]:
                _transformer(p, f"up_blocks.{i}.attentions.{j}.", co, cfg.cross_attention_dim,
                             cfg.use_linear_projection)
        ch = co
        if i != len(rev) - 1:
            p[f"up_blocks.{i}.upsamplers.0.conv.weight"] = (co, co, 3, 3)
            p[f"up_blocks.{i}.upsamplers.0.conv.bias"] = (co,)
    p["conv_norm_out.weight"] = (boc[0],)
    p["conv_norm_out.bias"] = (boc[0],)
    p["conv_out.weight"] = (cfg.out_channels, boc[0], 3, 3)
    p["conv_out.bias"] = (cfg.out_channels,)
    return p


def vae_decoder_param_shapes(cfg: VAEConfig) -> Dict[str, tuple]:
    """Keys of `AutoencoderKL` that `decode()` touches (post_quant_conv + decoder.*), with the
    diffusers>=0.18 attention naming (`to_q/to_k/to_v/to_out.0/group_norm`)."""
    p: Dict[str, tuple] = {}
    lc = cfg.latent_channels
    p["post_quant_conv.weight"] = (lc, lc, 1, 1)
    p["post_quant_conv.bias"] = (lc,)
    rev = list(reversed(cfg.block_out_channels))
    top = rev[0]
    p["decoder.conv_in.weight"] = (top, lc, 3, 3)
    p["decoder.conv_in.bias"] = (top,)
    _resnet(p, "decoder.mid_block.resnets.0.", top, top, None)
    a = "decoder.mid_block.attentions.0."
    p[a + "group_norm.weight"] = (top,)
    p[a + "group_norm.bias"] = (top,)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        p[a + n + ".weight"] = (top, top)
        p[a + n + ".bias"] = (top,)
    _resnet(p, "decoder.mid_block.resnets.1.", top, top, None)
    ch = top
    for i, co in enumerate(rev):
        for j in range(cfg.layers_per_block + 1):
            _resnet(p, f"decoder.up_blocks.{i}.resnets.{j}.", ch, co, None)
            ch = co
        if i != len(rev) - 1:
            p[f"decoder.up_blocks.{i}.upsamplers.0.conv.weight"] = (co, co, 3, 3)
            p[f"decoder.up_blocks.{i}.upsamplers.0.conv.bias"] = (co,)
    p["decoder.conv_norm_out.weight"] = (ch,)
    p["decoder.conv_norm_out.bias"] = (ch,)
    p["decoder.conv_out.weight"] = (cfg.out_channels, ch, 3, 3)
    p["decoder.conv_out.bias"] = (cfg.out_channels,)
    return p


def vae_encoder_param_shapes(cfg: VAEConfig) -> Dict[str, tuple]:
    """Keys of `AutoencoderKL` that `encode()` touches (encoder.* + quant_conv) -- the img2img front end."""
    p: Dict[str, tuple] = {}
    lc, boc = cfg.latent_channels, cfg.block_out_channels
    p["encoder.conv_in.weight"] = (boc[0], cfg.out_channels, 3, 3)
    p["encoder.conv_in.bias"] = (boc[0],)
    ch = boc[0]
    for i, co in enumerate(boc):
        for j in range(cfg.layers_per_block):
            _resnet(p, f"encoder.down_blocks.{i}.resnets.{j}.", ch, co, None)
            ch = co
        if i != len(boc) - 1:
            p[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"] = (co, co, 3, 3)
            p[f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"] = (co,)
    _resnet(p, "encoder.mid_block.resnets.0.", ch, ch, None)
    a = "encoder.mid_block.attentions.0."
    p[a + "group_norm.weight"] = (ch,)
    p[a + "group_norm.bias"] = (ch,)
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        p[a + n + ".weight"] = (ch, ch)
        p[a + n + ".bias"] = (ch,)
    _resnet(p, "encoder.mid_block.resnets.1.", ch, ch, None)
    p["encoder.conv_norm_out.weight"] = (ch,)
    p["encoder.conv_norm_out.bias"] = (ch,)
    p["encoder.conv_out.weight"] = (2 * lc, ch, 3, 3)
    p["encoder.conv_out.bias"] = (2 * lc,)
    p["quant_conv.weight"] = (2 * lc, 2 * lc, 1, 1)
    p["quant_conv.bias"] = (2 * lc,)
    return p


def cross_attn_layer_names(cfg: UNetConfig, include_mid: bool = True) -> List[str]:
    """Module paths of every `attn2`, in daam's locator order (up blocks, then down blocks, then
    mid) [upstream-knowledge, SURVEY.md §8a row D1]."""
    names = []
    n = len(cfg.block_out_channels)
    for i in range(n):
        if cfg.up_cross[i]:
            for j in range(cfg.layers_per_block + 1):
                names.append(f"up_blocks.{i}.attentions.{j}.transformer_blocks.0.attn2")
    for i in range(n):
        if cfg.down_cross[i]:
            for j in range(cfg.layers_per_block):
                names.append(f"down_blocks.{i}.attentions.{j}.transformer_blocks.0.attn2")
    if include_mid:
        names.append("mid_block.attentions.0.transformer_blocks.0.attn2")
    return names


def self_attn_layer_names(cfg) -> List[str]:
    """Module paths of every `attn1` of the UNet's transformer blocks: `cross_attn_layer_names`' spelling and order with attn1 in place of
    attn2.  cfg: a UNetConfig or an SDConfig."""
    ucfg = getattr(cfg, "unet", cfg)
    return [n[:-len("attn2")] + "attn1" for n in cross_attn_layer_names(ucfg)]


def resolve_pag_layers(cfg, layers) -> List[str]:
    """diffusers' `pag_applied_layers` [upstream-knowledge: diffusers 0.30 PAGMixin]: every string is `re.search`ed against the module names
    of the UNet's self-attention layers; the result is the matched names in `self_attn_layer_names`' order, each once.  A string that
    matches no layer is a ValueError naming it."""
    import re
    if isinstance(layers, str):
        layers = [layers]
    names = self_attn_layer_names(cfg)
    hit = set()
    for pat in layers:
        if not isinstance(pat, str):
            raise ValueError(f"pag_applied_layers takes strings, got {pat!r}")
        found = [n for n in names if re.search(pat, n) is not None]
        if not found:
            raise ValueError(f"Cannot find PAG layer to set attention processor for: {pat}")
        hit.update(found)
    return [n for n in names if n in hit]


def pag_schedule(timesteps, pag_scale: float, pag_adaptive_scale: float = 0.0) -> List[float]:
    """The PAG scale of every model evaluation [upstream-knowledge: diffusers 0.30 PAGMixin._get_pag_scale]:
    p_i = max(0, pag_scale - pag_adaptive_scale (1000 - t_i)); constant pag_scale when the adaptive scale is 0."""
    p, a = float(pag_scale), float(pag_adaptive_scale)
    if not a:
        return [p] * len(timesteps)
    return [max(0.0, p - a * (1000.0 - float(t))) for t in timesteps]


MAX_EDIT_CONCEPTS = 8          # AGD_MAX_EDIT_CONCEPTS


def sega_per_concept(name: str, value, K: int, default=None) -> list:
    """A per-concept argument of Semantic Guidance: a scalar (for every concept) or a list of K, as upstream; None is `default`."""
    if value is None:
        value = default
    if isinstance(value, (list, tuple)):
        if len(value) != K:
            raise ValueError(f"{name} has {len(value)} entries for {K} editing concepts (a scalar, or one entry per concept)")
        return list(value)
    return [value] * K


def sega_schedule(n_evaluations: int, concepts: int, reverse_editing_direction=False, edit_guidance_scale=5, edit_threshold=0.9,
                  edit_warmup_steps=10, edit_cooldown_steps=None, edit_weights=None) -> dict:
    """The host scalars of a Semantic Guidance call [upstream-knowledge: diffusers 0.21.2 SemanticStableDiffusionPipeline; parity-unpinned], one
    row per model evaluation i counted from 0 (PNDM's extra evaluation and img2img's shortened grid count as they run).  Concept k is active at
    i iff i < cooldown_k (None: always); coef[i][k] = sign_k scale_k if active else 0; w_mom[i] = softmax_k(weight_k if active else 0) over all
    K; with W = {k : i >= warmup_k}: w_add = w_mom and add_mom = 1 if W is everything, both 0 if W is empty, else w_add = the softmax of the
    same values over W alone (0 elsewhere) and add_mom = 0.  Computed in float64, rounded to fp32.  Returns {"concepts", "n_evals", "coef",
    "w_mom", "w_add" ([n][K] lists), "add_mom" ([n]), "q" ([K], float64), "walks", "folds"} -- walks: the evaluations with a non-zero coef."""
    import math
    import struct
    K, n = concepts, n_evaluations
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"n_evaluations={n!r}: a call runs at least one model evaluation")
    if isinstance(K, bool) or not isinstance(K, int) or K < 1 or K > MAX_EDIT_CONCEPTS:
        raise ValueError(f"editing_prompt: {K!r} editing concepts (1 .. {MAX_EDIT_CONCEPTS})")
    rev = sega_per_concept("reverse_editing_direction", reverse_editing_direction, K, False)
    scale = [float(x) for x in sega_per_concept("edit_guidance_scale", edit_guidance_scale, K, 5)]
    q = [float(x) for x in sega_per_concept("edit_threshold", edit_threshold, K, 0.9)]
    warm = sega_per_concept("edit_warmup_steps", edit_warmup_steps, K, 10)
    cool = sega_per_concept("edit_cooldown_steps", edit_cooldown_steps, K, None)
    wts = [float(x) for x in sega_per_concept("edit_weights", edit_weights, K, 1.0)]
    for k in range(K):
        if not math.isfinite(scale[k]):
            raise ValueError(f"edit_guidance_scale={scale[k]!r} for concept {k}: a finite number")
        if not (0.0 <= q[k] <= 1.0):
            raise ValueError(f"edit_threshold={q[k]!r} for concept {k}: a quantile in [0, 1]")
        if not math.isfinite(wts[k]):
            raise ValueError(f"edit_weights={wts[k]!r} for concept {k}: a finite number")
        if isinstance(warm[k], bool) or not isinstance(warm[k], int) or warm[k] < 0:
            raise ValueError(f"edit_warmup_steps={warm[k]!r} for concept {k}: an integer >= 0")
        if cool[k] is not None and (isinstance(cool[k], bool) or not isinstance(cool[k], int) or cool[k] < 0):
            raise ValueError(f"edit_cooldown_steps={cool[k]!r} for concept {k}: None or an integer >= 0")

    def f32(x: float) -> float:
        return struct.unpack("f", struct.pack("f", x))[0]

    def softmax(vals):
        mx = max(vals)
        e = [math.exp(v - mx) for v in vals]
        s = sum(e)
        return [x / s for x in e]

    coef, w_mom, w_add, add_mom = [], [], [], []
    for i in range(n):
        active = [cool[k] is None or i < cool[k] for k in range(K)]
        coef.append([f32((-1.0 if rev[k] else 1.0) * scale[k]) if active[k] else 0.0 for k in range(K)])
        vals = [wts[k] if active[k] else 0.0 for k in range(K)]
        wm = softmax(vals)
        W = [k for k in range(K) if i >= warm[k]]
        if len(W) == K:
            wa, am = wm, 1.0
        elif not W:
            wa, am = [0.0] * K, 0.0
        else:
            sub = softmax([vals[k] for k in W])
            wa = [0.0] * K
            for j, k in enumerate(W):
                wa[k] = sub[j]
            am = 0.0
        w_mom.append([f32(x) for x in wm]); w_add.append([f32(x) for x in wa]); add_mom.append(am)
    return {"concepts": K, "n_evals": n, "coef": coef, "w_mom": w_mom, "w_add": w_add, "add_mom": add_mom, "q": q,
            "walks": sum(1 for row in coef if any(c != 0.0 for c in row)), "folds": n}


def deepcache_schedule(n_evaluations: int, cache_interval: int) -> List[int]:
    """DeepCache's uniform schedule [upstream-knowledge: DeepCacheSDHelper, skip_mode "uniform"; parity-unpinned]: one flag per model
    evaluation of a call, counted from 0 whatever the scheduler (PNDM's extra evaluation and img2img's tail of the grid included) --
    1 = the full UNet, 0 = the shallow walk on the cached features; evaluation i is full iff i % cache_interval == 0."""
    if isinstance(n_evaluations, bool) or not isinstance(n_evaluations, int) or n_evaluations < 1:
        raise ValueError(f"n_evaluations={n_evaluations!r}: a call runs at least one model evaluation")
    if isinstance(cache_interval, bool) or not isinstance(cache_interval, int) or cache_interval < 1:
        raise ValueError(f"cache_interval={cache_interval!r}: DeepCache takes an integer interval >= 1")
    return [1 if i % cache_interval == 0 else 0 for i in range(n_evaluations)]


# ==========================================================================================
# ControlNet (diffusers ControlNetModel) [upstream-knowledge: diffusers 0.21.2]
# ==========================================================================================
@dataclass
class ControlNetConfig:
    """The parts of a diffusers ControlNet `config.json` the device path implements: the conditioning embedding's channel steps and
    the channel order of the control image.  Everything else must equal the UNet's (`controlnet_config_from_json` checks it)."""
    conditioning_embedding_out_channels: Tuple[int, ...] = (16, 32, 96, 256)
    conditioning_channel_order: str = "rgb"

    def to_json(self, unet: UNetConfig) -> dict:
        """A diffusers-shaped `config.json` for this ControlNet next to `unet`."""
        boc = unet.block_out_channels
        return {"_class_name": "ControlNetModel", "in_channels": unet.in_channels, "conditioning_channels": 3,
                "block_out_channels": list(boc),
                "down_block_types": ["CrossAttnDownBlock2D" if x else "DownBlock2D" for x in unet.down_cross],
                "layers_per_block": unet.layers_per_block, "attention_head_dim": list(unet.num_heads),
                "cross_attention_dim": unet.cross_attention_dim, "use_linear_projection": unet.use_linear_projection,
                "norm_num_groups": unet.norm_num_groups, "only_cross_attention": False, "upcast_attention": False,
                "class_embed_type": None, "addition_embed_type": None, "global_pool_conditions": False,
                "controlnet_conditioning_channel_order": self.conditioning_channel_order,
                "conditioning_embedding_out_channels": list(self.conditioning_embedding_out_channels)}


def controlnet_config_from_json(cj: dict, unet: UNetConfig) -> ControlNetConfig:
    """`ControlNetModel.from_pretrained(dir).config` -> ControlNetConfig.  Raises ValueError for what the device path does not implement:
    global pooling, class / addition embeddings, conditioning_channels != 3, and a block, head or cross-attention layout unlike the UNet's."""
    if cj.get("global_pool_conditions", False):
        raise ValueError("ControlNet global_pool_conditions=True (the shuffle ControlNets) is not implemented")
    for k in ("class_embed_type", "addition_embed_type", "encoder_hid_dim", "encoder_hid_dim_type", "projection_class_embeddings_input_dim"):
        if cj.get(k) is not None:
            raise ValueError(f"ControlNet {k}={cj.get(k)!r} is not implemented")
    if cj.get("num_class_embeds") is not None:
        raise ValueError(f"ControlNet num_class_embeds={cj.get('num_class_embeds')!r} is not implemented")
    tlpb = cj.get("transformer_layers_per_block", 1)
    if any(int(v) != 1 for v in (tlpb if isinstance(tlpb, (list, tuple)) else [tlpb])):
        raise ValueError(f"ControlNet transformer_layers_per_block={tlpb!r} is not implemented (one transformer block per attention)")
    if int(cj.get("conditioning_channels", 3)) != 3:
        raise ValueError(f"ControlNet conditioning_channels={cj.get('conditioning_channels')} is not implemented (3: an RGB control image)")
    order = cj.get("controlnet_conditioning_channel_order", "rgb")
    if order not in ("rgb", "bgr"):
        raise ValueError(f"ControlNet controlnet_conditioning_channel_order={order!r}")
    for k in ("only_cross_attention", "upcast_attention", "resnet_time_scale_shift", "act_fn", "flip_sin_to_cos", "freq_shift",
              "norm_eps", "downsample_padding", "mid_block_scale_factor"):
        want = {"only_cross_attention": False, "upcast_attention": False, "resnet_time_scale_shift": "default", "act_fn": "silu",
                "flip_sin_to_cos": True, "freq_shift": 0, "norm_eps": 1e-5, "downsample_padding": 1, "mid_block_scale_factor": 1}[k]
        v = cj.get(k, want)
        if isinstance(v, (list, tuple)):
            v = list(v)
            if any(x != want for x in v):
                raise ValueError(f"ControlNet {k}={cj.get(k)!r} is not implemented")
        elif v != want:
            raise ValueError(f"ControlNet {k}={v!r} is not implemented")
    ahd = cj.get("num_attention_heads") or cj.get("attention_head_dim", 8)
    heads = tuple(ahd) if isinstance(ahd, (list, tuple)) else (ahd,) * len(cj.get("block_out_channels", ()))
    got = {"in_channels": cj.get("in_channels", 4), "block_out_channels": tuple(cj.get("block_out_channels", ())),
           "down_cross": tuple("CrossAttn" in t for t in cj.get("down_block_types", ())),
           "layers_per_block": cj.get("layers_per_block", 2), "num_heads": heads,
           "cross_attention_dim": cj.get("cross_attention_dim", 1280), "use_linear_projection": cj.get("use_linear_projection", False),
           "norm_num_groups": cj.get("norm_num_groups", 32)}
    for k, v in got.items():
        if v != getattr(unet, k):
            raise ValueError(f"ControlNet {k}={v!r} differs from the UNet's {getattr(unet, k)!r}; only ControlNets shaped like their UNet are implemented")
    emb = tuple(cj.get("conditioning_embedding_out_channels", (16, 32, 96, 256)))
    if not 2 <= len(emb) <= 8 or any(int(c) < 1 for c in emb):
        raise ValueError(f"ControlNet conditioning_embedding_out_channels={emb!r} is not implemented (2 .. 8 positive entries)")
    return ControlNetConfig(conditioning_embedding_out_channels=tuple(int(c) for c in emb), conditioning_channel_order=order)


def controlnet_res_channels(unet: UNetConfig) -> List[int]:
    """Channel counts of the ControlNet's down-block res samples, in order (SD-1.x: 12): conv_in, each resnet / transformer output,
    each downsampler."""
    boc = unet.block_out_channels
    ch = [boc[0]]
    for i, co in enumerate(boc):
        ch += [co] * unet.layers_per_block
        if i != len(boc) - 1:
            ch.append(co)
    return ch


def controlnet_param_shapes(unet: UNetConfig, cn: ControlNetConfig) -> Dict[str, tuple]:
    """diffusers ControlNetModel state-dict keys and shapes: the UNet's conv_in, time embedding, down blocks and mid block, the
    conditioning embedding (conv_in, blocks.0 .. blocks.{2 (n - 1) - 1}, conv_out: 2 n 3x3 convs) and the 1x1 zero convs."""
    full = unet_param_shapes(unet)
    p = {k: v for k, v in full.items() if k.startswith(("conv_in.", "time_embedding.", "down_blocks.", "mid_block."))}
    emb = cn.conditioning_embedding_out_channels
    e = "controlnet_cond_embedding."
    p[e + "conv_in.weight"] = (emb[0], 3, 3, 3)
    p[e + "conv_in.bias"] = (emb[0],)
    for i in range(len(emb) - 1):
        p[e + f"blocks.{2 * i}.weight"] = (emb[i], emb[i], 3, 3)
        p[e + f"blocks.{2 * i}.bias"] = (emb[i],)
        p[e + f"blocks.{2 * i + 1}.weight"] = (emb[i + 1], emb[i], 3, 3)
        p[e + f"blocks.{2 * i + 1}.bias"] = (emb[i + 1],)
    p[e + "conv_out.weight"] = (unet.block_out_channels[0], emb[-1], 3, 3)
    p[e + "conv_out.bias"] = (unet.block_out_channels[0],)
    for k, c in enumerate(controlnet_res_channels(unet)):
        p[f"controlnet_down_blocks.{k}.weight"] = (c, c, 1, 1)
        p[f"controlnet_down_blocks.{k}.bias"] = (c,)
    mid = unet.block_out_channels[-1]
    p["controlnet_mid_block.weight"] = (mid, mid, 1, 1)
    p["controlnet_mid_block.bias"] = (mid,)
    return p


def controlnet_keep_schedule(n: int, start: float = 0.0, end: float = 1.0) -> List[float]:
    """StableDiffusionControlNetPipeline's `controlnet_keep` [upstream-knowledge]: evaluation i of n keeps the ControlNet unless
    i / n < control_guidance_start or (i + 1) / n > control_guidance_end."""
    if not 0.0 <= start < end <= 1.0:
        raise ValueError(f"control guidance window [{start}, {end}] must satisfy 0 <= start < end <= 1")
    return [1.0 - float(i / n < start or (i + 1) / n > end) for i in range(n)]


# ==========================================================================================
# T2I-Adapter (diffusers T2IAdapter, "full_adapter") [upstream-knowledge: diffusers 0.21.2]
# ==========================================================================================
@dataclass
class AdapterConfig:
    """A diffusers T2IAdapter `config.json`: `T2IAdapter(in_channels, channels, num_res_blocks, downscale_factor, adapter_type)`.  The
    defaults are the published SD-1.5 full adapters (canny / sketch take in_channels=1, depth / seg / pose 3)."""
    in_channels: int = 3
    channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    num_res_blocks: int = 2
    downscale_factor: int = 8
    adapter_type: str = "full_adapter"

    def to_json(self) -> dict:
        return {"_class_name": "T2IAdapter", "in_channels": self.in_channels, "channels": list(self.channels),
                "num_res_blocks": self.num_res_blocks, "downscale_factor": self.downscale_factor, "adapter_type": self.adapter_type}


def adapter_config_from_json(cj: dict) -> AdapterConfig:
    """`T2IAdapter.from_pretrained(dir).config` -> AdapterConfig.  Only "full_adapter" is implemented ("light_adapter" and the SDXL
    "full_adapter_xl" raise NotImplementedError)."""
    kind = cj.get("adapter_type", "full_adapter")
    if kind != "full_adapter":
        raise NotImplementedError(f"T2IAdapter adapter_type={kind!r} is not implemented (only 'full_adapter')")
    ch = tuple(int(c) for c in cj.get("channels", (320, 640, 1280, 1280)))
    if not ch or any(c < 1 for c in ch):
        raise ValueError(f"T2IAdapter channels={cj.get('channels')!r}")
    return AdapterConfig(in_channels=int(cj.get("in_channels", 3)), channels=ch, num_res_blocks=int(cj.get("num_res_blocks", 2)),
                         downscale_factor=int(cj.get("downscale_factor", 8)), adapter_type=kind)


def adapter_config_for(unet: UNetConfig, in_channels: int = 3) -> AdapterConfig:
    """The full adapter that fits `unet`: one block per UNet level at that level's width."""
    return AdapterConfig(in_channels=in_channels, channels=tuple(unet.block_out_channels))


def adapter_param_shapes(unet: UNetConfig, acfg: AdapterConfig) -> Dict[str, tuple]:
    """diffusers T2IAdapter (FullAdapter) state-dict keys and shapes: `adapter.conv_in` (3x3 on the pixel-unshuffled image), per entry
    of `channels` an AdapterBlock `adapter.body.{i}` -- `in_conv` (1x1) only where the width changes, then `num_res_blocks` resnets of
    `block1` (3x3) and `block2` (1x1).  `unet` only has to agree with it (the engine checks channels[i] == block_out_channels[i])."""
    del unet
    p: Dict[str, tuple] = {}
    ch = acfg.channels
    p["adapter.conv_in.weight"] = (ch[0], acfg.in_channels * acfg.downscale_factor ** 2, 3, 3)
    p["adapter.conv_in.bias"] = (ch[0],)
    for i, co in enumerate(ch):
        cin = ch[i - 1] if i else ch[0]
        b = f"adapter.body.{i}."
        if cin != co:
            p[b + "in_conv.weight"] = (co, cin, 1, 1)
            p[b + "in_conv.bias"] = (co,)
        for j in range(acfg.num_res_blocks):
            p[b + f"resnets.{j}.block1.weight"] = (co, co, 3, 3)
            p[b + f"resnets.{j}.block1.bias"] = (co,)
            p[b + f"resnets.{j}.block2.weight"] = (co, co, 1, 1)
            p[b + f"resnets.{j}.block2.bias"] = (co,)
    return p


def adapter_schedule(n: int, scale: float = 1.0, factor: float = 1.0) -> List[float]:
    """One scale per model evaluation: `adapter_conditioning_scale` on evaluations i < int(adapter_conditioning_factor * n), 0 (the plain
    UNet) on the rest.  n counts evaluations, so PNDM's repeated one counts."""
    if not 0.0 <= factor <= 1.0:
        raise ValueError(f"adapter_conditioning_factor {factor} must lie in [0, 1]")
    k = int(factor * n)
    return [float(scale) if i < k else 0.0 for i in range(n)]
