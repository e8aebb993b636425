"""IP-Adapter weight files -> the engine's tensors (`StableDiffusionPipeline.load_ip_adapter`, agd_ip_adapter_*).

[upstream-knowledge: the IP-Adapter paper (Ye et al. 2023) and the diffusers >= 0.24 loaders (`load_ip_adapter`, `ImageProjection`,
`IPAdapterAttnProcessor`)]
  file keys      `.safetensors`: flat "image_proj.proj.weight|bias", "image_proj.norm.weight|bias", "ip_adapter.{k}.to_k_ip.weight",
                 "ip_adapter.{k}.to_v_ip.weight"; `.bin`: a torch.load dict {"image_proj": {...}, "ip_adapter": {...}} with the same inner keys
  k numbering    k = 2 i + 1, i counting the attn2 layers in `unet.attn_processors` order: all of down_blocks, then all of up_blocks, then
                 mid_block last (k = 31 at SD-1.5); the even k are the attn1 processors, which carry no weights
  projection     tokens = LayerNorm(Linear(image_embeds).reshape(B, n_tok, cross_attention_dim)), n_tok = proj rows / cross_attention_dim;
                 under CFG the unconditional rows are the projection of zeros_like(image_embeds) -- not zero tokens
Supported: the plain SD-1.x / SD-2.x adapters ("ip-adapter_sd15", "ip-adapter_sd15_light": 4 tokens).  "plus" / "full-face" files (a
Resampler or MLP projection), FaceID files (LoRA keys), SDXL shapes, more than one adapter and list-valued scales are refused by name."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple, Union

import torch

from .config import SDConfig, UNetConfig

WEIGHT_NAMES = ("ip-adapter_sd15.safetensors", "ip-adapter_sd15.bin", "ip_adapter.safetensors", "ip_adapter.bin")
PROJ_KEYS = ("image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias")
REFUSED_PIPELINES = ("StableDiffusionControlNetPipeline", "StableDiffusionAdapterPipeline", "StableDiffusionGLIGENPipeline",
                     "StableDiffusionInpaintPipeline", "StableDiffusionInstructPix2PixPipeline", "StableDiffusionPanoramaPipeline",
                     "StableDiffusionRegionPipeline")


def attn2_blocks(ucfg: UNetConfig) -> List[str]:
    """The UNet's transformer-block prefixes ("down_blocks.0.attentions.0." ...) in `unet.attn_processors` order: down, up, mid."""
    n = len(ucfg.block_out_channels)
    out = [f"down_blocks.{i}.attentions.{j}." for i in range(n) if ucfg.down_cross[i] for j in range(ucfg.layers_per_block)]
    out += [f"up_blocks.{i}.attentions.{j}." for i in range(n) if ucfg.up_cross[i] for j in range(ucfg.layers_per_block + 1)]
    return out + ["mid_block.attentions.0."]


def key_indices(ucfg: UNetConfig) -> Dict[int, str]:
    """File index k -> transformer-block prefix (k = 2 i + 1)."""
    return {2 * i + 1: pre for i, pre in enumerate(attn2_blocks(ucfg))}


def block_channels(ucfg: UNetConfig, pre: str) -> int:
    boc = ucfg.block_out_channels
    if pre.startswith("mid_block"):
        return boc[-1]
    lvl = int(pre.split(".")[1])
    return boc[lvl] if pre.startswith("down_blocks") else tuple(reversed(boc))[lvl]


def ip_adapter_param_shapes(ucfg: UNetConfig, embed_dim: int, n_tokens: int = 4) -> Dict[str, tuple]:
    """The flat file keys of a plain IP-Adapter for `ucfg`."""
    D = ucfg.cross_attention_dim
    p = {PROJ_KEYS[0]: (n_tokens * D, embed_dim), PROJ_KEYS[1]: (n_tokens * D,), PROJ_KEYS[2]: (D,), PROJ_KEYS[3]: (D,)}
    for k, pre in key_indices(ucfg).items():
        c = block_channels(ucfg, pre)
        p[f"ip_adapter.{k}.to_k_ip.weight"] = (c, D)
        p[f"ip_adapter.{k}.to_v_ip.weight"] = (c, D)
    return p


def make_ip_adapter_weights(cfg: SDConfig, seed: int = 888, embed_dim: int = 1024, n_tokens: int = 4, bias_std: float = 0.05,
                            perturb_norm: float = 0.1) -> Dict[str, torch.Tensor]:
    """Random IP-Adapter weights for `cfg.unet` in the file's own (flat) key naming, bf16-representable: matrices N(0, 1/fan_in), the
    LayerNorm gamma ~ 1, small biases."""
    g = torch.Generator("cpu").manual_seed(seed)
    sd = {}
    for k, shp in ip_adapter_param_shapes(cfg.unet, embed_dim, n_tokens).items():
        if len(shp) == 2:
            w = torch.randn(shp, generator=g) / math.sqrt(shp[1])
        elif k.endswith("norm.weight"):
            w = 1.0 + perturb_norm * torch.randn(shp, generator=g)
        else:
            w = bias_std * torch.randn(shp, generator=g)
        sd[k] = w.to(torch.bfloat16).to(torch.float32)
    return sd


def write_ip_adapter(path: str, sd: Dict[str, torch.Tensor]) -> str:
    """Writes flat-keyed weights as the file format `path`'s extension names: `.safetensors` (flat keys) or `.bin` (nested dict)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if path.endswith(".safetensors"):
        from safetensors.torch import save_file
        save_file({k: t.contiguous() for k, t in sd.items()}, path)
    elif path.endswith(".bin"):
        nested: Dict[str, Dict[str, torch.Tensor]] = {"image_proj": {}, "ip_adapter": {}}
        for k, t in sd.items():
            top, rest = k.split(".", 1)
            nested.setdefault(top, {})[rest] = t
        torch.save(nested, path)
    else:
        raise ValueError(f"IP-Adapter: '{path}' is neither a .safetensors nor a .bin file")
    return path


def load_ip_adapter_state_dict(path_or_dict: Union[str, os.PathLike, Dict], subfolder: Optional[str] = None,
                               weight_name: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """Flat-keyed weights from a dict (flat or nested), a file, or a local directory (`subfolder` / `weight_name` in it).  Local only."""
    if isinstance(path_or_dict, (list, tuple)):
        raise ValueError("IP-Adapter: more than one adapter is not supported (pass one path or one state dict)")
    if isinstance(path_or_dict, dict):
        sd = path_or_dict
    else:
        path = os.fspath(path_or_dict)
        if isinstance(weight_name, (list, tuple)) or isinstance(subfolder, (list, tuple)):
            raise ValueError("IP-Adapter: more than one adapter is not supported (weight_name / subfolder must be single names)")
        if os.path.isdir(path):
            base = os.path.join(path, subfolder) if subfolder else path
            names = [weight_name] if weight_name else list(WEIGHT_NAMES)
            for n in names:
                if os.path.isfile(os.path.join(base, n)):
                    path = os.path.join(base, n)
                    break
            else:
                raise FileNotFoundError(f"IP-Adapter: no {' or '.join(names)} in {base} (local directories and files only)")
        elif not os.path.isfile(path):
            raise FileNotFoundError(f"IP-Adapter: {path} does not exist (local directories and files only)")
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(path, device="cpu")
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
    flat: Dict[str, torch.Tensor] = {}
    for k, v in sd.items():
        if isinstance(v, dict):
            for k2, t in v.items():
                flat[f"{k}.{k2}"] = t
        else:
            flat[k] = v
    return flat


def to_engine_tensors(sd: Dict[str, torch.Tensor], cfg: SDConfig) -> Tuple[Dict[str, torch.Tensor], int, int]:
    """Flat file keys -> ({engine name: fp32 tensor}, embed_dim, n_tokens); every unsupported file is refused by name."""
    u = cfg.unet
    D = u.cross_attention_dim
    for k in sd:
        if k.startswith("image_proj.latents") or ".layers." in k or k.startswith(("image_proj.proj_in", "image_proj.proj_out", "image_proj.norm_out")):
            raise ValueError(f"IP-Adapter: key '{k}' belongs to a Resampler projection (an IP-Adapter 'plus' / 'plus-face' file): not supported")
        if k.startswith(("image_proj.ff.", "image_proj.proj.0.", "image_proj.proj.2.")):
            raise ValueError(f"IP-Adapter: key '{k}' belongs to an MLP projection (an IP-Adapter 'full-face' file): not supported")
        if "lora" in k or k.startswith("image_proj.perceiver"):
            raise ValueError(f"IP-Adapter: key '{k}' belongs to an IP-Adapter FaceID file: not supported")
    for k in PROJ_KEYS:
        if k not in sd:
            raise ValueError(f"IP-Adapter: key '{k}' is missing")
    pw = sd[PROJ_KEYS[0]]
    idx = key_indices(u)
    ks = sorted(int(k.split(".")[1]) for k in sd if k.startswith("ip_adapter.") and k.endswith(".to_k_ip.weight"))
    if ks and sd[f"ip_adapter.{ks[0]}.to_k_ip.weight"].shape[1] == 2048 and D != 2048:
        raise ValueError(f"IP-Adapter: to_k_ip takes 2048-wide tokens (an SDXL adapter), this UNet's cross_attention_dim is {D}: not supported")
    if pw.ndim != 2 or pw.shape[0] % D:
        raise ValueError(f"IP-Adapter: image_proj.proj.weight {tuple(pw.shape)} is not [n_tokens * {D}, embed_dim] for this UNet "
                         f"(cross_attention_dim {D}; an SDXL adapter has 2048)")
    if ks != sorted(idx):
        raise ValueError(f"IP-Adapter: the file holds attn2 indices {ks[:3]}..{ks[-3:] if ks else []} ({len(ks)} layers), this UNet has "
                         f"{len(idx)} (k = 1, 3, .., {max(idx)}); an SDXL adapter has 70")
    n_tokens, embed_dim = int(pw.shape[0] // D), int(pw.shape[1])
    out = {k: sd[k].detach().to("cpu", torch.float32) for k in PROJ_KEYS}
    for k, pre in idx.items():
        for n in ("to_k_ip", "to_v_ip"):
            fk = f"ip_adapter.{k}.{n}.weight"
            if fk not in sd:
                raise ValueError(f"IP-Adapter: key '{fk}' is missing")
            t = sd[fk]
            want = (block_channels(u, pre), D)
            if tuple(t.shape) != want:
                raise ValueError(f"IP-Adapter: key '{fk}' is {tuple(t.shape)}, block {pre} needs {want}")
            out[f"{pre}transformer_blocks.0.attn2.{n}.weight"] = t.detach().to("cpu", torch.float32)
    extra = [k for k in sd if k not in PROJ_KEYS and not (k.startswith("ip_adapter.") and k.endswith(("to_k_ip.weight", "to_v_ip.weight")))]
    if extra:
        raise ValueError(f"IP-Adapter: cannot place key '{extra[0]}'")
    return out, embed_dim, n_tokens


def project_tokens(sd: Dict[str, torch.Tensor], image_embeds: torch.Tensor, cross_dim: int) -> torch.Tensor:
    """ImageProjection.forward on the host (fp32): [B, E] -> [B, n_tok, cross_dim]."""
    import torch.nn.functional as F
    h = F.linear(image_embeds.float(), sd[PROJ_KEYS[0]].float(), sd[PROJ_KEYS[1]].float())
    return F.layer_norm(h.reshape(image_embeds.shape[0], -1, cross_dim), (cross_dim,), sd[PROJ_KEYS[2]].float(), sd[PROJ_KEYS[3]].float(), 1e-5)


def cfg_image_embeds(embeds: torch.Tensor, batch: int, prompt_batch: int, images_per_prompt: int, embed_dim: int) -> torch.Tensor:
    """`ip_adapter_image_embeds` -> the [2B, E] rows [negative; positive] of a call of `batch` images: [B, E], [1, E] (one image for every
    prompt) or [prompt_batch, E] (one per prompt) positive rows get zeros as their negative rows; [2B, E] is taken as [neg; pos]."""
    if isinstance(embeds, (list, tuple)):
        if len(embeds) != 1:
            raise ValueError("ip_adapter_image_embeds: more than one adapter is not supported (pass one tensor)")
        embeds = embeds[0]
    e = torch.as_tensor(embeds).detach().to(torch.float32)
    if e.ndim == 3 and e.shape[1] == 1:
        e = e[:, 0]
    if e.ndim != 2 or e.shape[1] != embed_dim:
        raise ValueError(f"ip_adapter_image_embeds: shape {tuple(e.shape)}, expected [rows, {embed_dim}]")
    n = e.shape[0]
    if n == 2 * batch:
        return e.contiguous()
    if n == batch:
        pos = e
    elif n == 1:
        pos = e.expand(batch, -1)
    elif n == prompt_batch:
        pos = e.repeat_interleave(images_per_prompt, 0)
    else:
        raise ValueError(f"ip_adapter_image_embeds: {n} rows for {batch} images (1, {prompt_batch} (one per prompt), {batch}, or {2 * batch} as [neg; pos])")
    return torch.cat([torch.zeros_like(pos), pos], 0).contiguous()


# ---- the image encoder (a transformers CLIPVisionModelWithProjection directory: config.json + model.safetensors) ---------------------
ENCODER_WEIGHT_NAMES = ("model.safetensors", "pytorch_model.bin")


def image_encoder_config(**tower):
    """The tower's description as a `config.SafetyConfig` without concept rows (the safety checker's tower has the same fields).
    Defaults: OpenCLIP ViT-H/14, the encoder of the published SD-1.5 adapters [upstream-knowledge]."""
    from .config import SafetyConfig
    kw = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, hidden_act="gelu", projection_dim=1024,
              n_special=0, n_concepts=0)
    kw.update(tower)
    return SafetyConfig(**kw)


def image_encoder_config_from_json(cj: dict, preprocessor: Optional[dict] = None):
    """transformers CLIPVisionConfig `config.json` (+ an optional CLIPImageProcessor `preprocessor_config.json`) -> the tower's config."""
    v = cj.get("vision_config", cj)
    kw = {k: v[k] for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size",
                            "hidden_act", "layer_norm_eps") if k in v}
    kw["projection_dim"] = cj.get("projection_dim", v.get("projection_dim", 1024))
    if "image_size" in kw:
        kw["size"] = kw["crop_size"] = kw["image_size"]
    if preprocessor:
        for src, dst in (("image_mean", "image_mean"), ("image_std", "image_std")):
            if src in preprocessor:
                kw[dst] = tuple(preprocessor[src])
    return image_encoder_config(**kw)


def image_encoder_param_shapes(scfg) -> Dict[str, tuple]:
    """The transformers CLIPVisionModelWithProjection state-dict keys ("vision_model.…", "visual_projection.weight")."""
    from .config import safety_param_shapes
    out = {}
    for k, shp in safety_param_shapes(scfg).items():
        if k.startswith("vision_model.vision_model."):
            out[k[len("vision_model."):]] = shp
        elif k == "visual_projection.weight":
            out[k] = shp
    return out


def make_image_encoder_weights(scfg, seed: int = 99) -> Dict[str, torch.Tensor]:
    """Random image-encoder weights for `scfg` (image_encoder_config) under the transformers keys, bf16-representable: linears and the
    patch conv N(0, 1/fan_in), class / position embeddings N(0, 0.02), LayerNorm gamma ~ 1, small biases."""
    g = torch.Generator("cpu").manual_seed(seed)
    sd = {}
    for k, shp in image_encoder_param_shapes(scfg).items():
        if "embedding" in k and "patch" not in k:
            w = torch.randn(shp, generator=g) * 0.02
        elif k.endswith(".weight") and len(shp) >= 2:
            w = torch.randn(shp, generator=g) / math.sqrt(math.prod(shp[1:]))
        elif k.endswith(".weight"):
            w = 1.0 + 0.1 * torch.randn(shp, generator=g)
        else:
            w = 0.05 * torch.randn(shp, generator=g)
        sd[k] = w.to(torch.bfloat16).to(torch.float32)
    return sd


def write_image_encoder(path: str, scfg, sd: Dict[str, torch.Tensor]) -> str:
    """Writes a transformers-shaped CLIPVisionModelWithProjection directory: config.json + model.safetensors."""
    import json
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    cj = {"architectures": ["CLIPVisionModelWithProjection"], "model_type": "clip_vision_model", "hidden_size": scfg.hidden_size,
          "intermediate_size": scfg.intermediate_size, "num_hidden_layers": scfg.num_hidden_layers, "num_attention_heads": scfg.num_attention_heads,
          "image_size": scfg.image_size, "patch_size": scfg.patch_size, "hidden_act": scfg.hidden_act, "layer_norm_eps": scfg.layer_norm_eps,
          "projection_dim": scfg.projection_dim, "num_channels": 3}
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cj, f)
    save_file({k: t.contiguous() for k, t in sd.items()}, os.path.join(path, "model.safetensors"))
    return path


def load_image_encoder(path: str):
    """(tower config, state dict) of a local CLIPVisionModelWithProjection directory."""
    import json
    if not os.path.isfile(os.path.join(path, "config.json")):
        raise FileNotFoundError(f"IP-Adapter image encoder: no config.json in {path} (a local transformers CLIPVisionModelWithProjection directory)")
    with open(os.path.join(path, "config.json")) as f:
        cj = json.load(f)
    pre = None
    if os.path.isfile(os.path.join(path, "preprocessor_config.json")):
        with open(os.path.join(path, "preprocessor_config.json")) as f:
            pre = json.load(f)
    for n in ENCODER_WEIGHT_NAMES:
        fp = os.path.join(path, n)
        if os.path.isfile(fp):
            if n.endswith(".safetensors"):
                from safetensors.torch import load_file
                sd = load_file(fp, device="cpu")
            else:
                sd = torch.load(fp, map_location="cpu", weights_only=True)
            break
    else:
        raise FileNotFoundError(f"IP-Adapter image encoder: no {' or '.join(ENCODER_WEIGHT_NAMES)} in {path}")
    scfg = image_encoder_config_from_json(cj, pre)
    want = image_encoder_param_shapes(scfg)
    sd = {k: v for k, v in sd.items() if not k.endswith("position_ids")}
    for k, shp in want.items():
        if k not in sd:
            raise ValueError(f"IP-Adapter image encoder: key '{k}' is missing in {path}")
        if tuple(sd[k].shape) != tuple(shp):
            raise ValueError(f"IP-Adapter image encoder: key '{k}' is {tuple(sd[k].shape)}, config.json needs {tuple(shp)}")
    return scfg, {k: sd[k] for k in want}


def find_image_encoder(adapter_path, subfolder: Optional[str], folder: Optional[str]) -> Optional[str]:
    """The encoder directory `load_ip_adapter` reads: `folder` itself if it is a directory, else `folder` beside the weights (under the
    adapter directory's subfolder, then under the directory).  None: nothing found (the encoder is optional)."""
    if not folder:
        return None
    cands = [folder]
    if isinstance(adapter_path, (str, os.PathLike)):
        base = os.fspath(adapter_path)
        base = base if os.path.isdir(base) else os.path.dirname(os.path.abspath(base))
        cands = ([os.path.join(base, subfolder, folder)] if subfolder else []) + [os.path.join(base, folder)] + cands
    for c in cands:
        if os.path.isfile(os.path.join(c, "config.json")):
            return c
    return None


def prepare_ip_adapter_image(image) -> torch.Tensor:
    """`ip_adapter_image` -> uint8 [n, H, W, 3]: a PIL image, a uint8 [H,W,3] / [n,H,W,3] array or tensor, or a list of same-sized ones."""
    import numpy as np
    items = list(image) if isinstance(image, (list, tuple)) else [image]
    if not items:
        raise ValueError("ip_adapter_image: an empty list")
    out = []
    for it in items:
        if hasattr(it, "convert"):                                  # PIL
            it = np.asarray(it.convert("RGB"))
        t = torch.as_tensor(np.asarray(it) if not torch.is_tensor(it) else it)
        if t.dtype != torch.uint8 or t.ndim not in (3, 4) or t.shape[-1] != 3:
            raise ValueError(f"ip_adapter_image: expected PIL images or uint8 [H,W,3] / [n,H,W,3], got {t.dtype} {tuple(t.shape)}")
        out.append(t[None] if t.ndim == 3 else t)
    if len({tuple(t.shape[1:]) for t in out}) != 1:
        raise ValueError("ip_adapter_image: the images of one call must share one size")
    return torch.cat(out, 0).contiguous()
