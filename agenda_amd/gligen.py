"""GLIGEN box-grounded txt2img: diffusers' `StableDiffusionGLIGENPipeline` (0.21.2 semantics) over the device engine.

A GLIGEN UNet (`attention_type: "gated"`) carries a PositionNet and, in every transformer block, a GatedSelfAttentionDense ("fuser") that
runs after attn1's residual add.  The PositionNet turns per-object phrase embeddings and boxes into 30 grounding tokens once per call
(`agd_gligen_set`); each fuser's K/V of those tokens is cached per block, and the fused denoise loops run the fusers on the evaluations the
scheduled-sampling rule enables (`agd_gligen_set_schedule`).  An evaluation without grounding runs exactly the plain UNet.  DAAM and the
hook.py hooker see attn2 only, as with diffusers.  Rules restated from the published pipeline are marked [upstream-knowledge].

Beyond diffusers (labelled so below): `gligen_phrases` / `gligen_boxes` may be a list of layouts, one per image of the call.
Not implemented, and refused: `gligen_inpaint_image`, GLIGEN with ControlNet, inpainting or img2img, the "gated-text-image" UNet, LoRA on the
fusers or the PositionNet.
"""
from __future__ import annotations

import json
import math
import os
import warnings
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from .config import SDConfig, cross_attn_layer_names
from .pipeline import StableDiffusionPipeline, refuse_deepcache, refuse_long_prompt, refuse_pag, refuse_sega

MAX_OBJS = 30                 # [upstream-knowledge] StableDiffusionGLIGENPipeline.__call__: max_objs = 30
FOURIER_FREQS = 8             # [upstream-knowledge] PositionNet(fourier_freqs=8)
POSNET_HIDDEN = 512


def is_gligen_key(key: str) -> bool:
    """A UNet state-dict key of the GLIGEN parts (the PositionNet or a fuser)."""
    return key.startswith("position_net.") or ".fuser." in key


def attention_type_of(unet_json: dict) -> str:
    """`attention_type` of a UNet config.json: "default" (absent) or "gated"; "gated-text-image" and anything else are refused."""
    at = unet_json.get("attention_type", "default")
    if at not in ("default", "gated"):
        raise ValueError(f"unet attention_type {at!r} is not supported (GLIGEN runs 'gated' UNets; 'gated-text-image' is not implemented)")
    return at


def transformer_blocks(ucfg) -> List[str]:
    """The UNet's transformer-block prefixes ("down_blocks.0.attentions.0." ...), one fuser each."""
    return [n[: -len("transformer_blocks.0.attn2")] for n in cross_attn_layer_names(ucfg, include_mid=True)]


def gligen_param_shapes(ucfg) -> Dict[str, tuple]:
    """The GLIGEN keys of a gated UNet [upstream-knowledge: PositionNet(positive_len = out_dim = cross_attention_dim) and
    GatedSelfAttentionDense(C, cross_attention_dim, heads, C / heads) as `transformer_blocks.0.fuser`]."""
    D, p = ucfg.cross_attention_dim, {}
    p["position_net.linears.0.weight"] = (POSNET_HIDDEN, D + 8 * FOURIER_FREQS)
    p["position_net.linears.0.bias"] = (POSNET_HIDDEN,)
    p["position_net.linears.2.weight"] = (POSNET_HIDDEN, POSNET_HIDDEN)
    p["position_net.linears.2.bias"] = (POSNET_HIDDEN,)
    p["position_net.linears.4.weight"] = (D, POSNET_HIDDEN)
    p["position_net.linears.4.bias"] = (D,)
    p["position_net.null_positive_feature"] = (D,)
    p["position_net.null_position_feature"] = (8 * FOURIER_FREQS,)
    boc = ucfg.block_out_channels
    for pre in transformer_blocks(ucfg):
        if pre.startswith("mid_block"):
            c = boc[-1]
        elif pre.startswith("down_blocks"):
            c = boc[int(pre.split(".")[1])]
        else:
            c = tuple(reversed(boc))[int(pre.split(".")[1])]
        f = pre + "transformer_blocks.0.fuser."
        p[f + "linear.weight"] = (c, D)
        p[f + "linear.bias"] = (c,)
        for n in ("to_q", "to_k", "to_v"):
            p[f + f"attn.{n}.weight"] = (c, c)
        p[f + "attn.to_out.0.weight"] = (c, c)
        p[f + "attn.to_out.0.bias"] = (c,)
        p[f + "ff.net.0.proj.weight"] = (8 * c, c)
        p[f + "ff.net.0.proj.bias"] = (8 * c,)
        p[f + "ff.net.2.weight"] = (c, 4 * c)
        p[f + "ff.net.2.bias"] = (c,)
        for n in ("norm1", "norm2"):
            p[f + n + ".weight"] = (c,)
            p[f + n + ".bias"] = (c,)
        p[f + "alpha_attn"] = ()
        p[f + "alpha_dense"] = ()
    return p


def make_gligen_weights(cfg: SDConfig, seed: int = 777, alpha_attn: float = 0.7, alpha_dense: float = 0.5, bias_std: float = 0.05,
                        perturb_norm: float = 0.1) -> Dict[str, torch.Tensor]:
    """Random PositionNet + fuser weights for `cfg.unet`, bf16-representable: matrices N(0, 1/fan_in), LayerNorm gamma ~ 1, small biases,
    null features N(0, 0.5).  The gates are NOT zero (a freshly initialised GLIGEN has tanh(0) = 0 and would hide a broken fuser)."""
    g = torch.Generator("cpu").manual_seed(seed)
    sd = {}
    for k, shp in gligen_param_shapes(cfg.unet).items():
        last = k.split(".")[-1]
        if last == "alpha_attn":
            w = torch.tensor(alpha_attn)
        elif last == "alpha_dense":
            w = torch.tensor(alpha_dense)
        elif "null_" in k:
            w = 0.5 * torch.randn(shp, generator=g)
        elif k.endswith(".weight") and len(shp) == 2:
            w = torch.randn(shp, generator=g) / math.sqrt(shp[1])
        elif k.endswith(".weight"):
            w = 1.0 + perturb_norm * torch.randn(shp, generator=g)
        else:
            w = bias_std * torch.randn(shp, generator=g)
        sd[k] = w.to(torch.bfloat16).to(torch.float32)
    return sd


# ---- the pipeline's per-call preparation [upstream-knowledge: StableDiffusionGLIGENPipeline.__call__, diffusers 0.21.2] ------------------
def check_layout(phrases: Sequence[str], boxes: Sequence[Sequence[float]]) -> Tuple[List[str], List[List[float]]]:
    """One image's objects: equal counts (ValueError), boxes [x0, y0, x1, y1] inside [0, 1] with x0 <= x1 and y0 <= y1 (ValueError), more than
    30 cut to the first 30 with a warning."""
    phrases, boxes = list(phrases), [list(map(float, b)) for b in boxes]
    if len(phrases) != len(boxes):
        raise ValueError(f"length of gligen_phrases ({len(phrases)}) and gligen_boxes ({len(boxes)}) must be the same")
    for b in boxes:
        if len(b) != 4:
            raise ValueError(f"a GLIGEN box is [x0, y0, x1, y1], got {b}")
        if not all(0.0 <= v <= 1.0 for v in b):
            raise ValueError(f"GLIGEN box {b} lies outside [0, 1] (boxes are normalised to the image)")
        if b[0] > b[2] or b[1] > b[3]:
            raise ValueError(f"GLIGEN box {b} has x0 > x1 or y0 > y1")
    if len(boxes) > MAX_OBJS:
        warnings.warn(f"More that {MAX_OBJS} objects found. Only first {MAX_OBJS} objects will be processed.", FutureWarning)
        phrases, boxes = phrases[:MAX_OBJS], boxes[:MAX_OBJS]
    return phrases, boxes


def layouts_for(gligen_phrases, gligen_boxes, batch: int) -> List[Tuple[List[str], List[List[float]]]]:
    """The call's layout per image: diffusers' one layout for every image, or (an extension beyond diffusers) a list of `batch` layouts,
    one per image, so that one batch can hold a different layout per seed."""
    if gligen_phrases is None or gligen_boxes is None:
        raise ValueError("StableDiffusionGLIGENPipeline needs gligen_phrases and gligen_boxes")
    per_image = len(gligen_phrases) > 0 and isinstance(gligen_phrases[0], (list, tuple))
    if not per_image:
        lay = check_layout(gligen_phrases, gligen_boxes)
        return [lay] * batch
    if len(gligen_phrases) != batch or len(gligen_boxes) != batch:
        raise ValueError(f"per-image GLIGEN layouts: {len(gligen_phrases)} phrase lists and {len(gligen_boxes)} box lists for {batch} images")
    return [check_layout(p, b) for p, b in zip(gligen_phrases, gligen_boxes)]


def first_eos(ids: torch.Tensor, eos_id: int) -> torch.Tensor:
    """The pooled row of each sequence: the first EOS position.  CLIPTextModel's pooler_output takes argmax(input_ids), which is the first EOS
    because EOS is the largest id of the CLIP vocabulary [upstream-knowledge]; the rule here holds for any tokenizer."""
    return (ids == eos_id).to(torch.int64).argmax(dim=1)


def object_tensors(layouts, pooled: Dict[str, torch.Tensor], cross_dim: int):
    """boxes [2B, 30, 4], text_embeddings [2B, 30, D], masks [2B, 30]: zero beyond each image's n_objs, masks[:n_objs] = 1, then the CFG
    doubling with the unconditional half all null (masks[:B] = 0) [upstream-knowledge]."""
    B = len(layouts)
    boxes = torch.zeros(B, MAX_OBJS, 4)
    emb = torch.zeros(B, MAX_OBJS, cross_dim)
    masks = torch.zeros(B, MAX_OBJS)
    for i, (ph, bx) in enumerate(layouts):
        n = len(bx)
        if n:
            boxes[i, :n] = torch.tensor(bx)
            emb[i, :n] = torch.stack([pooled[p] for p in ph])
            masks[i, :n] = 1
    boxes, emb, masks = torch.cat([boxes] * 2), torch.cat([emb] * 2), torch.cat([masks] * 2)
    masks[:B] = 0
    return boxes, emb, masks


def grounding_flags(beta: float, n_evals: int) -> List[int]:
    """[upstream-knowledge] num_grounding_steps = int(beta * len(timesteps)); the fusers run for loop indices i < num_grounding_steps."""
    k = int(beta * n_evals)
    return [1 if i < k else 0 for i in range(n_evals)]


class StableDiffusionGLIGENPipeline(StableDiffusionPipeline):
    """`StableDiffusionGLIGENPipeline`: `pipe(prompt, gligen_phrases=[...], gligen_boxes=[[x0, y0, x1, y1], ...],
    gligen_scheduled_sampling_beta=0.3)`; everything else is StableDiffusionPipeline's."""
    _gligen = True

    def __init__(self, cfg: SDConfig, unet_sd, vae_sd, controlnet=None, **kw):
        if controlnet is not None:
            raise ValueError("GLIGEN with a ControlNet is not implemented")
        if cfg.unet.in_channels != cfg.unet.out_channels:
            raise ValueError("GLIGEN on an inpainting UNet is not implemented")
        want = gligen_param_shapes(cfg.unet)
        missing = sorted(k for k in want if k not in unet_sd)
        if missing:
            raise ValueError(f"not a GLIGEN UNet: {len(missing)} position_net / fuser weights missing (first: {missing[0]})")
        self._gl_sd = {k: v for k, v in unet_sd.items() if is_gligen_key(k)}
        self._gl_pending = None
        super().__init__(cfg, {k: v for k, v in unet_sd.items() if not is_gligen_key(k)}, vae_sd, **kw)

    def _load_extra(self):
        self.engine.gligen_configure(self.cfg.unet.cross_attention_dim, MAX_OBJS, FOURIER_FREQS)
        self.engine.load_state_dict(self._gl_sd, "unet.")

    # ---- construction -------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, cfg: Union[str, SDConfig] = "sd15", seed: int = 1234, device=0, workspace_bytes: int = 0,
                       weights_device: str = "cpu", keep_weights: bool = False, scheduler: str = "DDIMScheduler", gligen=True, **kw):
        """Random UNet / VAE weights plus random PositionNet and fusers with non-zero gates (gligen=True; or a state dict of GLIGEN keys)."""
        from . import config as _config, synthetic
        cfg = _config.CONFIGS[cfg]() if isinstance(cfg, str) else cfg
        usd = synthetic.make_unet_weights(cfg, seed, device=weights_device, **kw)
        vsd = synthetic.make_vae_weights(cfg, seed + 1, device=weights_device, **kw)
        usd.update(make_gligen_weights(cfg, seed + 3) if gligen is True else gligen)
        pipe = cls(cfg, usd, vsd, device=device, workspace_bytes=workspace_bytes, scheduler=scheduler)
        if keep_weights:
            pipe.synthetic_weights = (usd, vsd)
        return pipe

    @classmethod
    def from_pretrained(cls, path: str, **kw):
        """A checkpoint whose unet/config.json has `attention_type: "gated"`."""
        with open(os.path.join(path, "unet", "config.json")) as f:
            at = attention_type_of(json.load(f))
        if at != "gated":
            raise ValueError(f"{path}: the UNet is not a GLIGEN UNet (attention_type {at!r}, StableDiffusionGLIGENPipeline needs 'gated')")
        return super().from_pretrained(path, **kw)

    def save_pretrained(self, save_directory: str):
        """StableDiffusionPipeline.save_pretrained (the UNet's weights, fusers and PositionNet included, are re-exported as loaded) with
        `attention_type: "gated"` and the pipeline's `_class_name`."""
        super().save_pretrained(save_directory)
        uc = os.path.join(save_directory, "unet", "config.json")
        with open(uc) as f:
            uj = json.load(f)
        uj["attention_type"] = "gated"
        with open(uc, "w") as f:
            json.dump(uj, f, indent=2)
        mi = os.path.join(save_directory, "model_index.json")
        with open(mi) as f:
            mj = json.load(f)
        mj["_class_name"] = "StableDiffusionGLIGENPipeline"
        with open(mi, "w") as f:
            json.dump(mj, f, indent=2)

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, weight_name: Optional[str] = None, **kwargs):
        """LoRA on the UNet's own attention and the text encoder as StableDiffusionPipeline; keys that name the fusers or the PositionNet are
        refused (the fusers' fused forms are derived once at load)."""
        from . import lora
        sd = lora.load_lora_state_dict(pretrained_model_name_or_path_or_dict, weight_name)
        bad = [k for k in sd if "fuser" in k or "position_net" in k]
        if bad:
            raise ValueError(f"LoRA on the GLIGEN fusers / PositionNet is not supported ({len(bad)} keys, first: {bad[0]})")
        return super().load_lora_weights(sd, **kwargs)

    # ---- objects ------------------------------------------------------------------------
    def _eos_id(self) -> int:
        tok = self.tokenizer
        eid = getattr(tok, "eos_token_id", None)
        return int(eid) if eid is not None else int(tok.vocab[tok.eos_token])

    def _phrase_ids(self, phrases: List[str]) -> torch.Tensor:
        te = self.text_encoder
        if hasattr(te, "_ids"):
            return te._ids(phrases).to(torch.int64)
        return torch.tensor([self.tokenizer.encode(p) for p in phrases], dtype=torch.int64)

    def pooled_phrase_embeddings(self, phrases: Sequence[str]) -> Dict[str, torch.Tensor]:
        """[upstream-knowledge] each phrase's `text_encoder(...).pooler_output`: the final-LayerNorm row at its first EOS.  The encoder runs at
        the full token length; it is causal, so that row equals the one of the `padding=True` encode diffusers runs."""
        uniq = list(dict.fromkeys(phrases))
        if not uniq:
            return {}
        hidden = self.text_encoder(uniq).detach().float().cpu()
        idx = first_eos(self._phrase_ids(uniq), self._eos_id())
        rows = hidden[torch.arange(len(uniq)), idx]
        return {p: rows[i] for i, p in enumerate(uniq)}

    # ---- txt2img ------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, gligen_scheduled_sampling_beta: float = 0.3,
                 gligen_phrases=None, gligen_boxes=None, gligen_inpaint_image=None, negative_prompt=None, num_images_per_prompt: int = 1,
                 eta: float = 0.0, generator=None, latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None,
                 output_type: str = "pil", cross_attention_kwargs: Optional[dict] = None, guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 max_embeddings_multiples: Optional[int] = None, editing_prompt=None, editing_prompt_embeddings=None, sem_guidance=None):
        refuse_pag("StableDiffusionGLIGENPipeline", pag_scale, pag_adaptive_scale)
        refuse_sega("StableDiffusionGLIGENPipeline", editing_prompt, editing_prompt_embeddings, sem_guidance)
        refuse_deepcache("StableDiffusionGLIGENPipeline", getattr(self, "_deepcache", None))
        refuse_long_prompt("StableDiffusionGLIGENPipeline", max_embeddings_multiples, prompt_embeds)
        if gligen_inpaint_image is not None:
            raise ValueError("gligen_inpaint_image (GLIGEN inpainting) is not implemented")
        if eta != 0.0:
            raise ValueError("eta != 0 is not implemented (the fused DDIM step is deterministic)")
        if prompt_embeds is not None:
            batch = prompt_embeds.shape[0] // 2
        else:
            batch = (1 if isinstance(prompt, str) else len(prompt)) * num_images_per_prompt
        layouts = layouts_for(gligen_phrases, gligen_boxes, batch)
        pooled = self.pooled_phrase_embeddings([p for ph, _ in layouts for p in ph])
        objs = object_tensors(layouts, pooled, self.cfg.unet.cross_attention_dim)
        self._gl_pending = (objs, float(gligen_scheduled_sampling_beta))
        self.last_layouts = layouts
        try:
            return super().__call__(prompt, height=height, width=width, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                    negative_prompt=negative_prompt, generator=generator, latents=latents, prompt_embeds=prompt_embeds,
                                    output_type=output_type, num_images_per_prompt=num_images_per_prompt,
                                    cross_attention_kwargs=cross_attention_kwargs, guidance_rescale=guidance_rescale)
        finally:
            self._gl_pending = None
            self.engine.gligen_clear()

    def grounding_schedule(self, num_inference_steps: int, beta: float) -> List[int]:
        """One flag per model evaluation of this pipeline's scheduler (PNDM: steps + 1 evaluations)."""
        from .controlnet import evaluation_count
        return grounding_flags(beta, evaluation_count(self.scheduler, num_inference_steps))

    def _denoise(self, lat, num_inference_steps, guidance_scale):
        if self._gl_pending is None:
            raise RuntimeError("the GLIGEN pipeline's loop runs from __call__ (it needs the phrases and boxes)")
        (boxes, emb, masks), beta = self._gl_pending
        if boxes.shape[0] != 2 * lat.shape[0]:
            raise ValueError(f"GLIGEN objects for {boxes.shape[0] // 2} images, latents for {lat.shape[0]}")
        self.engine.gligen_set(boxes, emb, masks)
        self.engine.gligen_set_schedule(self.grounding_schedule(num_inference_steps, beta))
        super()._denoise(lat, num_inference_steps, guidance_scale)

    def img2img(self, *a, **kw):
        raise ValueError("GLIGEN img2img is not implemented")
