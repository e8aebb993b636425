"""`StableDiffusionPipeline`-shaped surface over libagenda_hip.so.

Mirrors what the reference touches on `diffusers.StableDiffusionPipeline`
(reference data_generation/data_generation.py:30-31,47-52,59): `from_pretrained`, `.to("cuda")`,
`.tokenizer`, `.text_encoder`, `.unet`, `.vae`, `.scheduler`, `set_progress_bar_config`,
`__call__(prompt, num_inference_steps=, generator=).images[0]`.

Differences that are deliberate:
 * batched prompts/seeds per call (the reference runs batch 1);
 * DDIM (eta 0) instead of the checkpoint's default scheduler (BASELINE.json's metric);
 * initial latents come from a CPU `torch.Generator` (or are passed explicitly) so the CPU oracle
   and the GPU run share them; a CUDA generator cannot be reproduced on the host;
 * the safety checker runs when the checkpoint has one (`safety_checker/` + `feature_extractor/`, agenda_amd/safety.py);
   synthetic pipelines and checkpoints without it black nothing out.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .config import SDConfig, CONFIGS, UNetConfig, VAEConfig, SchedulerConfig, cross_attn_layer_names
from .scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler, SCHEDULERS, scheduler_config_from_json,
                        scheduler_config_to_json)
from .text import SimpleTokenizer, SyntheticTextEncoder


_KEEP = object()        # from_pretrained(safety_checker=...) not given: load the checkpoint's own checker


@dataclass
class UNetOutput:
    """diffusers' UNet2DConditionOutput: `unet(...).sample`."""
    sample: torch.Tensor


@dataclass
class PipelineOutput:
    images: list
    latents: Optional[torch.Tensor] = None
    nsfw_content_detected: Optional[list] = None


def _hw(L) -> Tuple[int, int]:
    """A latent (or pixel) size given as one side (square) or as an (h, w) pair."""
    if isinstance(L, (tuple, list)):
        h, w = L
        return int(h), int(w)
    return int(L), int(L)


def check_guidance_rescale(guidance_rescale: float) -> None:
    """`guidance_rescale` is Lin et al.'s phi: a finite number in [0, 1].  Refused here, before a call does any device work."""
    phi = float(guidance_rescale)
    if not (math.isfinite(phi) and 0.0 <= phi <= 1.0):
        raise ValueError(f"guidance_rescale={guidance_rescale!r}: guidance rescale takes a number in [0, 1]")


def check_pag(pag_scale: float, pag_adaptive_scale: float = 0.0, guidance_rescale: float = 0.0) -> None:
    """`pag_scale` / `pag_adaptive_scale`: finite numbers >= 0, the adaptive scale only beside a pag_scale > 0, and no guidance rescale with
    them (diffusers rescales against the text branch, which the fold has overwritten).  Refused here, before a call does any device work."""
    p, a = float(pag_scale), float(pag_adaptive_scale)
    if not (math.isfinite(p) and p >= 0.0):
        raise ValueError(f"pag_scale={pag_scale!r}: Perturbed-Attention Guidance takes a finite scale >= 0")
    if not (math.isfinite(a) and a >= 0.0):
        raise ValueError(f"pag_adaptive_scale={pag_adaptive_scale!r}: Perturbed-Attention Guidance takes a finite adaptive scale >= 0")
    if a > 0.0 and not p > 0.0:
        raise ValueError(f"pag_adaptive_scale={pag_adaptive_scale!r} needs pag_scale > 0 (got pag_scale={pag_scale!r})")
    if p > 0.0 and guidance_rescale:
        raise ValueError(f"guidance_rescale={guidance_rescale!r} with pag_scale={pag_scale!r}: guidance rescale beside Perturbed-Attention "
                         "Guidance is not implemented (the text branch it rescales to is folded away); leave one of them 0")


def refuse_pag(pipeline: str, pag_scale: float, pag_adaptive_scale: float = 0.0) -> None:
    """The pipelines that run beside something the perturbed branch does not carry refuse a non-zero scale by name."""
    if pag_scale or pag_adaptive_scale:
        raise ValueError(f"pag_scale={pag_scale!r}, pag_adaptive_scale={pag_adaptive_scale!r}: Perturbed-Attention Guidance is not implemented "
                         f"for {pipeline} (StableDiffusionPipeline's txt2img and img2img run it); leave both 0")


def check_sega(editing_prompt=None, editing_prompt_embeddings=None, reverse_editing_direction=False, edit_guidance_scale=5,
               edit_warmup_steps=10, edit_cooldown_steps=None, edit_threshold=0.9, edit_momentum_scale=0.1, edit_mom_beta=0.4,
               edit_weights=None, sem_guidance=None, pag_scale: float = 0.0, guidance_rescale: float = 0.0, deepcache=None, ip_adapter=None,
               ip_adapter_image=None, ip_adapter_image_embeds=None, max_embeddings_multiples=None) -> Optional[dict]:
    """Semantic Guidance's arguments (diffusers 0.21.2 SemanticStableDiffusionPipeline [upstream-knowledge]), decided from the call's
    arguments alone, before any device work.  No editing prompt: None (the plain call).  Else the concepts -- {"K", "prompts" (a list, or
    None), "embeds" ([K, T, D], or None), "args" (`config.sega_schedule`'s keywords), "mu", "beta"} -- after every refusal: both forms of the
    concepts, more than 8 of them, a per-concept list whose length is not K, a threshold outside [0, 1], upstream's `sem_guidance`, and what
    the concept walk does not run beside (pag_scale, guidance_rescale, an enabled DeepCache, an active IP-Adapter, weighted prompts)."""
    from .config import MAX_EDIT_CONCEPTS, sega_schedule
    if sem_guidance is not None:
        raise ValueError("sem_guidance: precomputed guidance vectors are not implemented (the engine computes the guidance of every "
                         "evaluation on the device); leave it None")
    if editing_prompt is not None and editing_prompt_embeddings is not None:
        raise ValueError("editing_prompt and editing_prompt_embeddings are both given; pass the concepts in one form")
    if editing_prompt is None and editing_prompt_embeddings is None:
        return None
    if editing_prompt is not None:
        prompts = [editing_prompt] if isinstance(editing_prompt, str) else list(editing_prompt)
        if not all(isinstance(p, str) for p in prompts):
            raise ValueError(f"editing_prompt={editing_prompt!r}: a string or a list of strings")
        K, embeds, name = len(prompts), None, "editing_prompt"
    else:
        embeds, prompts, name = editing_prompt_embeddings, None, "editing_prompt_embeddings"
        if not torch.is_tensor(embeds) or embeds.ndim != 3:
            raise ValueError("editing_prompt_embeddings: a tensor [K, T, D], one row of tokens per concept")
        K = embeds.shape[0]
    if K < 1 or K > MAX_EDIT_CONCEPTS:
        raise ValueError(f"{name}: {K} editing concepts (1 .. {MAX_EDIT_CONCEPTS})")
    args = dict(reverse_editing_direction=reverse_editing_direction, edit_guidance_scale=edit_guidance_scale, edit_threshold=edit_threshold,
                edit_warmup_steps=edit_warmup_steps, edit_cooldown_steps=edit_cooldown_steps, edit_weights=edit_weights)
    sega_schedule(1, K, **args)                                # (every per-concept refusal, by the argument's name)
    mu, beta = float(edit_momentum_scale), float(edit_mom_beta)
    if not math.isfinite(mu):
        raise ValueError(f"edit_momentum_scale={edit_momentum_scale!r}: a finite number")
    if not math.isfinite(beta):
        raise ValueError(f"edit_mom_beta={edit_mom_beta!r}: a finite number")
    if pag_scale:
        raise ValueError(f"pag_scale={pag_scale!r} with {name}: Semantic Guidance beside Perturbed-Attention Guidance is not implemented; leave one out")
    if guidance_rescale:
        raise ValueError(f"guidance_rescale={guidance_rescale!r} with {name}: guidance rescale beside Semantic Guidance is not implemented; leave one out")
    refuse_deepcache("StableDiffusionPipeline", deepcache, f"{name} (Semantic Guidance)")
    if (ip_adapter_image is not None or ip_adapter_image_embeds is not None) and ip_adapter is not None and ip_adapter["scale"] != 0.0:
        raise ValueError(f"an active IP-Adapter (scale {ip_adapter['scale']!r}) with {name}: Semantic Guidance beside an image prompt is not "
                         "implemented; leave the image prompt out or set_ip_adapter_scale(0)")
    if max_embeddings_multiples is not None:
        raise ValueError(f"max_embeddings_multiples={max_embeddings_multiples!r} with {name}: Semantic Guidance with weighted / long prompts "
                         "is not implemented; leave it None")
    return {"K": K, "prompts": prompts, "embeds": embeds, "args": args, "mu": mu, "beta": beta}


def refuse_sega(pipeline: str, editing_prompt=None, editing_prompt_embeddings=None, sem_guidance=None) -> None:
    """The pipelines that run beside something the concept walk does not carry refuse Semantic Guidance's arguments by name."""
    for name, v in (("editing_prompt", editing_prompt), ("editing_prompt_embeddings", editing_prompt_embeddings), ("sem_guidance", sem_guidance)):
        if v is not None:
            raise ValueError(f"{name}: Semantic Guidance is not implemented for {pipeline} (StableDiffusionPipeline's txt2img and img2img "
                             "run it); leave it None")


def check_deepcache(cache_interval, cache_branch_id, layers_per_block: int, skip_mode: str = "uniform") -> None:
    """`enable_deepcache`'s arguments: an integer interval >= 1, a branch among the layers of the first down block, the uniform schedule."""
    for name, v in (("cache_interval", cache_interval), ("cache_branch_id", cache_branch_id)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name}={v!r}: DeepCache takes an integer")
    if cache_interval < 1:
        raise ValueError(f"cache_interval={cache_interval!r}: DeepCache takes an interval >= 1 (1 = every evaluation is full)")
    if not 0 <= cache_branch_id <= layers_per_block - 1:
        raise ValueError(f"cache_branch_id={cache_branch_id!r}: this UNet has branches 0 .. {layers_per_block - 1} (the layers of its first "
                         "down block); deeper branches are not implemented")
    if skip_mode != "uniform":
        raise ValueError(f"skip_mode={skip_mode!r}: only the 'uniform' DeepCache schedule is implemented")


def refuse_deepcache(pipeline: str, deepcache, what: str = "") -> None:
    """The pipelines (and call arguments) that run beside something the shallow walk does not carry refuse an enabled DeepCache by name.
    `deepcache`: the pipeline's state, None or (cache_interval, cache_branch_id); interval 1 sets nothing and is never refused."""
    if deepcache is not None and deepcache[0] > 1:
        raise ValueError(f"DeepCache (cache_interval={deepcache[0]}, cache_branch_id={deepcache[1]}) is enabled: it is not implemented for "
                         f"{pipeline}{' with ' + what if what else ''} (StableDiffusionPipeline's txt2img and img2img run it); "
                         "call disable_deepcache() first")


LONG_CONTEXT = 96      # tokens up to which every pipeline, recorder and adapter runs; beyond, StableDiffusionPipeline's txt2img / img2img only


def refuse_long_prompt(pipeline: str, max_embeddings_multiples, prompt_embeds) -> None:
    """The pipelines that run something beside the plain UNet refuse weighted / long prompts by name: the argument, and given
    prompt_embeds of more than 96 tokens (the engine's fused attn2 forms and their recorders stop there)."""
    if max_embeddings_multiples is not None:
        raise ValueError(f"max_embeddings_multiples={max_embeddings_multiples!r}: weighted and long prompts are not implemented for {pipeline} "
                         "(StableDiffusionPipeline's txt2img and img2img run them); leave it None")
    if prompt_embeds is not None and prompt_embeds.shape[1] > LONG_CONTEXT:
        raise ValueError(f"prompt_embeds of {prompt_embeds.shape[1]} tokens: a context over {LONG_CONTEXT} tokens is not implemented for {pipeline} "
                         "(StableDiffusionPipeline's txt2img and img2img run it)")


def refuse_deepcache_beside(deepcache, pag_scale: float, ip_adapter, ip_adapter_image, ip_adapter_image_embeds) -> None:
    """What a txt2img / img2img call can carry that the shallow walk does not, decided from the call's arguments alone, before any device
    work: a non-zero pag_scale, and an image prompt for a loaded IP-Adapter whose scale is not 0 (`ip_adapter`: the pipeline's adapter
    state, None = none loaded -- the call then fails on that by itself; scale 0 or no image leaves the adapter idle, which is allowed)."""
    if pag_scale:
        refuse_deepcache("StableDiffusionPipeline", deepcache, f"pag_scale={pag_scale!r}")
    if (ip_adapter_image is not None or ip_adapter_image_embeds is not None) and ip_adapter is not None and ip_adapter["scale"] != 0.0:
        refuse_deepcache("StableDiffusionPipeline", deepcache, f"an active IP-Adapter (scale {ip_adapter['scale']!r})")


class DeepCacheSDHelper:
    """The upstream `DeepCache.DeepCacheSDHelper` [upstream-knowledge], parity-unpinned: `set_params`, `enable`, `disable` forwarded to the
    pipeline's enable_deepcache / disable_deepcache, so a script written for the upstream helper runs unchanged."""

    def __init__(self, pipe=None):
        self.pipe = pipe
        self.params = dict(cache_interval=1, cache_branch_id=0, skip_mode="uniform")

    def set_params(self, cache_interval: int = 1, cache_branch_id: int = 0, skip_mode: str = "uniform"):
        check_deepcache(cache_interval, cache_branch_id, self.pipe.cfg.unet.layers_per_block, skip_mode)
        self.params = dict(cache_interval=cache_interval, cache_branch_id=cache_branch_id, skip_mode=skip_mode)

    def enable(self, pipe=None):
        if pipe is not None:
            self.pipe = pipe
        self.pipe.enable_deepcache(**self.params)

    def disable(self):
        self.pipe.disable_deepcache()


def check_image_size(height: int, width: int, multiple: int = 64) -> None:
    """The pipelines' size rule: each side a positive multiple of 64, applied per axis (height and width may differ)."""
    if not all(isinstance(v, int) and v > 0 and v % multiple == 0 for v in (height, width)):
        raise ValueError(f"height and width must each be a positive multiple of {multiple}, got height={height}, width={width}")


def _floats(xs):
    """A sequence of numbers as a ctypes float array (one element when empty: the engine is given a valid pointer and a length of 0)."""
    xs = [float(x) for x in xs]
    return (C.c_float * max(len(xs), 1))(*xs)


def _make_cfg(cfg: SDConfig, workspace_bytes: int) -> _lib.AgdConfig:
    a = _lib.AgdConfig()
    a.struct_size = C.sizeof(_lib.AgdConfig)
    u, v = cfg.unet, cfg.vae
    a.in_channels, a.out_channels, a.n_levels = u.in_channels, u.out_channels, len(u.block_out_channels)
    for i, c in enumerate(u.block_out_channels):
        a.block_out_channels[i] = c
        a.down_cross[i] = int(u.down_cross[i])
        a.num_heads[i] = u.num_heads[i]
    a.layers_per_block, a.cross_attention_dim = u.layers_per_block, u.cross_attention_dim
    a.use_linear_projection, a.norm_num_groups = int(u.use_linear_projection), u.norm_num_groups
    a.vae_latent_channels, a.vae_out_channels, a.vae_n_levels = v.latent_channels, v.out_channels, len(v.block_out_channels)
    for i, c in enumerate(v.block_out_channels):
        a.vae_block_out_channels[i] = c
    a.vae_layers_per_block, a.vae_norm_num_groups = v.layers_per_block, v.norm_num_groups
    a.vae_scaling_factor = v.scaling_factor
    a.max_tokens = cfg.max_tokens
    a.prediction_type = 1 if cfg.sched.prediction_type == "v_prediction" else 0
    a.workspace_bytes = workspace_bytes
    t = getattr(cfg, "text", None)
    if t is not None:
        a.text_hidden, a.text_layers, a.text_heads = t.hidden_size, t.num_hidden_layers, t.num_attention_heads
        a.text_intermediate, a.text_vocab, a.text_max_pos = t.intermediate_size, t.vocab_size, t.max_position_embeddings
        a.text_act = 0 if t.hidden_act == "quick_gelu" else 1
        a.text_eps = t.layer_norm_eps
    return a


class Engine:
    """Owns one `agd_ctx` (one per GPU per process)."""

    def __init__(self, cfg: SDConfig, device: int = 0, workspace_bytes: int = 0):
        if not torch.cuda.is_available():
            raise _lib.AgendaHipError("agenda_amd needs an MI355X (no CPU fallback)")
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = device
        self._acfg = _make_cfg(cfg, workspace_bytes)
        self.ctx = self.lib.agd_create(device, C.byref(self._acfg))
        if not self.ctx:
            raise _lib.AgendaHipError("agd_create failed: " + self.lib.agd_last_error(None).decode())
        self.finalized = False
        # IP-Adapter: (embed_dim, n_tokens) of the loaded adapter, the rows of the last ip_adapter_set and its embeddings, the image encoder's config
        self._ipa_dims: Optional[Tuple[int, int]] = None
        self._ipa_rows = 0
        self._ipa_keepalive = None
        self._ienc_cfg = None

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.agd_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        _lib.check(rc, self.ctx, what)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str):
        for k, t in sd.items():
            t = t.detach().to(torch.float32).contiguous()
            shape = (C.c_longlong * t.ndim)(*t.shape)
            self._ck(self.lib.agd_load_tensor(self.ctx, (prefix + k).encode(), C.c_void_p(t.data_ptr()), 0, t.ndim, shape),
                     f"agd_load_tensor({prefix + k})")

    def finalize(self):
        self._ck(self.lib.agd_finalize(self.ctx), "agd_finalize")
        self.finalized = True

    @staticmethod
    def _stream():
        return _lib.current_stream_ptr()

    def _h2d(self, t: torch.Tensor) -> torch.Tensor:
        """fp32 copy of `t` on the engine's device.  A host tensor goes through one of two persistent pinned staging buffers per shape with a
        NON-blocking transfer: a pageable `.to(device)` blocks the launching thread until the copy ran -- behind everything already queued on
        the stream -- so every batch ended with the GPU idle while the host prepared the next one (1 - 1.5 ms per batch in the kernel trace);
        a fresh `pin_memory()` per call is worse (the pinned allocation stalls for tens of ms).  A staging buffer is rewritten only after the
        event behind its previous copy has completed."""
        t = t.detach().to(torch.float32)
        if t.device.type != "cpu":
            return t.to(device=f"cuda:{self.device}").contiguous()
        pool = self.__dict__.setdefault("_stage", {})
        slot = pool.get(tuple(t.shape))
        if slot is None:                                   # both buffers at the first use of a shape (a warm-up batch): pinning stalls for tens of ms
            slot = pool[tuple(t.shape)] = {"bufs": [torch.empty(t.shape, dtype=torch.float32).pin_memory() for _ in range(2)],
                                           "evs": [torch.cuda.Event() for _ in range(2)], "next": 0}
            for e in slot["evs"]:
                e.record()
        k = slot["next"]; slot["next"] = (k + 1) % 2
        slot["evs"][k].synchronize()
        slot["bufs"][k].copy_(t)
        out = slot["bufs"][k].to(device=f"cuda:{self.device}", non_blocking=True)
        slot["evs"][k].record()
        return out

    def set_context(self, ctx_emb: torch.Tensor):
        ctx_emb = self._h2d(ctx_emb)
        b2, t, _ = ctx_emb.shape
        self._ck(self.lib.agd_set_context(self.ctx, _lib.ptr(ctx_emb), b2, t, self._stream()), "agd_set_context")
        self._ctx_keepalive = ctx_emb

    def text_encode(self, input_ids: torch.Tensor) -> torch.Tensor:
        """`text_encoder(input_ids)[0]`: int [B,T] -> fp32 [B,T,H] (cuda)."""
        ids = input_ids.to(torch.int32).contiguous()
        b, t = ids.shape
        out = torch.empty(b, t, self.cfg.text.hidden_size, device=f"cuda:{self.device}", dtype=torch.float32)
        self._ck(self.lib.agd_text_encode(self.ctx, C.c_void_p(ids.data_ptr()), b, t, _lib.ptr(out), self._stream()), "agd_text_encode")
        torch.cuda.synchronize()          # `ids` may be a host tensor: keep it alive until the copy ran
        return out

    def safety_configure(self, scfg):
        from .safety import vision_config
        self._vcfg = vision_config(scfg)
        self._ck(self.lib.agd_safety_configure(self.ctx, C.byref(self._vcfg)), "agd_safety_configure")

    def safety_scores(self, images_u8: torch.Tensor, want_pixels: bool = False):
        """`agd_safety_scores`: uint8 [B,H,W,3] -> cosines fp32 [B, n_special + n_concepts] (cuda), and the processor's
        pixel_values [B,3,R,R] when asked."""
        s = self.cfg.safety
        img = images_u8.to(device=f"cuda:{self.device}", dtype=torch.uint8).contiguous()
        if img.ndim != 4 or img.shape[3] != 3:
            raise ValueError(f"safety checker takes uint8 [B,H,W,3] images, got {tuple(img.shape)}")
        b, h, w = img.shape[0], img.shape[1], img.shape[2]
        cos = torch.empty(b, s.n_special + s.n_concepts, device=img.device, dtype=torch.float32)
        pix = torch.empty(b, 3, s.image_size, s.image_size, device=img.device, dtype=torch.float32) if want_pixels else None
        self._ck(self.lib.agd_safety_scores_hw(self.ctx, _lib.ptr(img), b, h, w, _lib.ptr(cos), _lib.ptr(pix), self._stream()),
                 "agd_safety_scores_hw")
        return (cos, pix) if want_pixels else cos

    def controlnet_configure(self, cncfg):
        self._cncfg = _lib.AgdControlNetConfig()
        self._cncfg.struct_size = C.sizeof(_lib.AgdControlNetConfig)
        emb = cncfg.conditioning_embedding_out_channels
        self._cncfg.n_emb = len(emb)
        for i, c in enumerate(emb):
            self._cncfg.emb_channels[i] = int(c)
        self._cncfg.bgr = int(cncfg.conditioning_channel_order == "bgr")
        self._ck(self.lib.agd_controlnet_configure(self.ctx, C.byref(self._cncfg)), "agd_controlnet_configure")

    def controlnet_set_cond(self, cond: torch.Tensor, repeat: int = 2):
        """`agd_controlnet_set_cond`: the control image fp32 [B,3,H,W] in [0,1] -> the conditioning embedding of B * repeat UNet rows
        ([cond; cond] for the CFG batch), computed once."""
        cond = self._h2d(cond)
        b, c, h, w = cond.shape
        if c != 3:
            raise ValueError(f"control image must be [B,3,H,W], got {tuple(cond.shape)}")
        self._ck(self.lib.agd_controlnet_set_cond_hw(self.ctx, _lib.ptr(cond), b, h, w, int(repeat), self._stream()), "agd_controlnet_set_cond_hw")
        self._cond_keepalive = cond

    def controlnet_set_schedule(self, scales):
        """Per-model-evaluation conditioning scales of the next fused loop (or one-element: the next unet_forward); empty clears."""
        self._ck(self.lib.agd_controlnet_set_schedule(self.ctx, _floats(scales), len(scales)), "agd_controlnet_set_schedule")

    def controlnet_residuals(self, sample: torch.Tensor, timestep: float, scale: float = 1.0, nhwc: bool = False) -> torch.Tensor:
        """`agd_controlnet_residuals`: the scaled ControlNet residuals of one forward, back to back in one fp32 vector (down residuals in
        res-sample order, then the mid residual; each [B2,C,h,w], or [B2,h,w,C] with nhwc)."""
        sample = sample.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        b2, _, Lh, Lw = sample.shape
        n = C.c_longlong(0)
        self._ck(self.lib.agd_controlnet_residuals_hw(self.ctx, None, b2, Lh, Lw, 0.0, 0.0, int(nhwc), None, C.byref(n), None), "agd_controlnet_residuals")
        out = torch.empty(n.value, device=sample.device, dtype=torch.float32)
        self._ck(self.lib.agd_controlnet_residuals_hw(self.ctx, _lib.ptr(sample), b2, Lh, Lw, float(timestep), float(scale), int(nhwc),
                                                      _lib.ptr(out), C.byref(n), self._stream()), "agd_controlnet_residuals_hw")
        return out

    def adapter_configure(self, acfg):
        self._adcfg = _lib.AgdAdapterConfig()
        self._adcfg.struct_size = C.sizeof(_lib.AgdAdapterConfig)
        if len(acfg.channels) > _lib.AGD_MAX_LEVELS:
            raise ValueError(f"T2IAdapter channels has {len(acfg.channels)} entries (at most {_lib.AGD_MAX_LEVELS})")
        self._adcfg.in_channels, self._adcfg.n_channels = int(acfg.in_channels), len(acfg.channels)
        for i, c in enumerate(acfg.channels):
            self._adcfg.channels[i] = int(c)
        self._adcfg.num_res_blocks, self._adcfg.downscale_factor = int(acfg.num_res_blocks), int(acfg.downscale_factor)
        self._ck(self.lib.agd_adapter_configure(self.ctx, C.byref(self._adcfg)), "agd_adapter_configure")

    def adapter_set_cond(self, image: torch.Tensor):
        """`agd_adapter_set_cond_hw`: the conditioning image uint8 [B,H,W,C] or float [B,C,H,W] in [0,1] -> the adapter's features, computed
        once and kept for B images (UNet row image b reads feature image b % B)."""
        f32 = image.dtype != torch.uint8
        image = image.to(device=f"cuda:{self.device}", dtype=torch.float32 if f32 else torch.uint8).contiguous()
        if image.ndim != 4:
            raise ValueError(f"adapter image must be uint8 [B,H,W,C] or float [B,C,H,W], got {tuple(image.shape)}")
        b = image.shape[0]
        (c, h, w) = tuple(image.shape[1:]) if f32 else (image.shape[3], image.shape[1], image.shape[2])
        if c != self._adcfg.in_channels:
            raise ValueError(f"adapter image has {c} channels, the adapter takes {self._adcfg.in_channels}")
        self._ck(self.lib.agd_adapter_set_cond_hw(self.ctx, C.c_void_p(image.data_ptr()), int(f32), b, h, w, self._stream()), "agd_adapter_set_cond_hw")
        self._adapter_keepalive = image
        r = self._adcfg.downscale_factor
        self._adapter_shape = (b, h // r, w // r)

    def adapter_features(self) -> List[torch.Tensor]:
        """`agd_adapter_features`: the unscaled features of the last adapter_set_cond, fp32 [B, channels[i], Lh >> i, Lw >> i] (cuda)."""
        if getattr(self, "_adapter_shape", None) is None:      # nothing set through this object: the engine says so
            self._ck(self.lib.agd_adapter_features(self.ctx, None), "agd_adapter_features")
        b, Lh, Lw = self._adapter_shape
        shapes = [(b, self._adcfg.channels[i], Lh >> i, Lw >> i) for i in range(self._adcfg.n_channels)]
        flat = torch.empty(sum(s[0] * s[1] * s[2] * s[3] for s in shapes), device=f"cuda:{self.device}", dtype=torch.float32)
        self._ck(self.lib.agd_adapter_features(self.ctx, _lib.ptr(flat)), "agd_adapter_features")
        out, off = [], 0
        for s in shapes:
            n = s[0] * s[1] * s[2] * s[3]
            out.append(flat[off:off + n].view(s))
            off += n
        return out

    def adapter_set_schedule(self, scales):
        """Per-model-evaluation adapter scales of the next fused loop (or one-element: the next unet_forward); empty clears."""
        self._ck(self.lib.agd_adapter_set_schedule(self.ctx, _floats(scales), len(scales)), "agd_adapter_set_schedule")

    def adapter_clear(self):
        self._ck(self.lib.agd_adapter_clear(self.ctx), "agd_adapter_clear")
        self._adapter_shape = None

    def adapter_add_counts(self):
        """(adds that left GroupNorm partial sums, adds that did not) since the engine was created."""
        n = (C.c_longlong * 2)()
        self._ck(self.lib.agd_adapter_add_counts(self.ctx, n), "agd_adapter_add_counts")
        return int(n[0]), int(n[1])

    def ip_adapter_load(self, tensors: Dict[str, torch.Tensor], embed_dim: int, n_tokens: int):
        """`agd_ip_adapter_begin` .. `agd_ip_adapter_commit`: `tensors` under the engine's names (ip_adapter.to_engine_names)."""
        self._ck(self.lib.agd_ip_adapter_begin(self.ctx, int(embed_dim), int(n_tokens)), "agd_ip_adapter_begin")
        try:
            for k, t in tensors.items():
                t = t.detach().to(torch.float32).contiguous()
                shape = (C.c_longlong * max(t.ndim, 1))(*t.shape)
                self._ck(self.lib.agd_ip_adapter_tensor(self.ctx, k.encode(), C.c_void_p(t.data_ptr()), 0, t.ndim, shape), f"agd_ip_adapter_tensor({k})")
            self._ck(self.lib.agd_ip_adapter_commit(self.ctx), "agd_ip_adapter_commit")
        except Exception:
            self.lib.agd_ip_adapter_unload(self.ctx)
            raise
        self._ipa_dims = (int(embed_dim), int(n_tokens))

    def ip_adapter_unload(self):
        self._ck(self.lib.agd_ip_adapter_unload(self.ctx), "agd_ip_adapter_unload")
        self._ipa_dims = None
        self._ipa_rows = 0

    def ip_adapter_set(self, image_embeds: torch.Tensor, scale: float = 1.0):
        """`agd_ip_adapter_set`: image embeddings fp32 [B2, embed_dim] ([negative; positive]) -> the projected tokens and every attn2
        layer's pre-multiplied image matrices, for the next forwards on B2 rows."""
        emb = self._h2d(image_embeds.to(torch.float32)).clone().contiguous()
        dims = self._ipa_dims                                  # (None: nothing loaded -- the engine says so by name)
        if emb.ndim != 2 or (dims is not None and emb.shape[1] != dims[0]):
            raise ValueError(f"ip_adapter_set: image_embeds {tuple(emb.shape)}, the adapter takes [rows, {dims[0] if dims else 'embed_dim'}]")
        self._ck(self.lib.agd_ip_adapter_set(self.ctx, _lib.ptr(emb), int(emb.shape[0]), float(scale), self._stream()), "agd_ip_adapter_set")
        self._ipa_keepalive = emb
        self._ipa_rows = int(emb.shape[0])

    def ip_adapter_clear(self):
        self._ck(self.lib.agd_ip_adapter_clear(self.ctx), "agd_ip_adapter_clear")
        self._ipa_rows = 0

    def ip_adapter_tokens(self) -> torch.Tensor:
        """`agd_ip_adapter_tokens`: the projected tokens of the last ip_adapter_set, fp32 [B2, n_tokens, cross_attention_dim] (cuda)."""
        if not self._ipa_rows or self._ipa_dims is None:
            raise _lib.AgendaHipError("ip_adapter_tokens: no image tokens set (ip_adapter_set first)")
        out = torch.empty(self._ipa_rows, self._ipa_dims[1], self.cfg.unet.cross_attention_dim, device=f"cuda:{self.device}", dtype=torch.float32)
        self._ck(self.lib.agd_ip_adapter_tokens(self.ctx, _lib.ptr(out)), "agd_ip_adapter_tokens")
        return out

    def ip_adapter_block(self, block: str, x: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """`agd_ip_adapter_block`: x + scale * to_out_weight . attn_ip(norm2(x)) of `block` on x fp32 [B2, h*w, C]."""
        x = x.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        self._ck(self.lib.agd_ip_adapter_block(self.ctx, block.encode(), _lib.ptr(x), x.shape[0], h, w, _lib.ptr(out), self._stream()),
                 "agd_ip_adapter_block")
        return out

    def image_encoder_load(self, scfg, tensors: Dict[str, torch.Tensor]):
        """`agd_image_encoder_begin` .. `agd_image_encoder_commit`: the IP-Adapter's CLIP image encoder (scfg: ip_adapter.image_encoder_config;
        tensors under the transformers CLIPVisionModelWithProjection keys).  One per engine, until image_encoder_unload; a load that fails
        part way unloads itself, so it can be tried again."""
        from .safety import vision_config
        vcfg = vision_config(scfg)
        self._ck(self.lib.agd_image_encoder_begin(self.ctx, C.byref(vcfg)), "agd_image_encoder_begin")
        try:
            for k, t in tensors.items():
                t = t.detach().to(torch.float32).contiguous()
                shape = (C.c_longlong * max(t.ndim, 1))(*t.shape)
                self._ck(self.lib.agd_image_encoder_tensor(self.ctx, ("image_encoder." + k).encode(), C.c_void_p(t.data_ptr()), 0, t.ndim, shape),
                         f"agd_image_encoder_tensor({k})")
            self._ck(self.lib.agd_image_encoder_commit(self.ctx), "agd_image_encoder_commit")
        except Exception:
            self.lib.agd_image_encoder_unload(self.ctx)
            raise
        self._ienc_cfg = scfg

    def image_encoder_unload(self):
        self._ck(self.lib.agd_image_encoder_unload(self.ctx), "agd_image_encoder_unload")
        self._ienc_cfg = None

    def image_embeds(self, images_u8: torch.Tensor) -> torch.Tensor:
        """`agd_image_embeds`: uint8 [B,H,W,3] -> CLIP image embeddings fp32 [B, projection_dim] (cuda)."""
        img = images_u8.to(device=f"cuda:{self.device}", dtype=torch.uint8).contiguous()
        if img.ndim != 4 or img.shape[3] != 3:
            raise ValueError(f"the image encoder takes uint8 [B,H,W,3] images, got {tuple(img.shape)}")
        if self._ienc_cfg is None:
            raise _lib.AgendaHipError("image_embeds: no image encoder loaded (image_encoder_load first)")
        out = torch.empty(img.shape[0], self._ienc_cfg.projection_dim, device=img.device, dtype=torch.float32)
        self._ck(self.lib.agd_image_embeds(self.ctx, _lib.ptr(img), img.shape[0], img.shape[1], img.shape[2], _lib.ptr(out), self._stream()),
                 "agd_image_embeds")
        return out

    def ip_adapter_counts(self):
        """`agd_ip_adapter_counts`: (score launches, add launches) of the block walk since the last ip_adapter_clear."""
        n = (C.c_longlong * 2)()
        self._ck(self.lib.agd_ip_adapter_counts(self.ctx, n), "agd_ip_adapter_counts")
        return int(n[0]), int(n[1])

    def freeu_set(self, s1: float, s2: float, b1: float, b2: float):
        """`agd_freeu_set`: FreeU on every later UNet evaluation of this engine, until freeu_clear (all four 1: the plain UNet)."""
        self._ck(self.lib.agd_freeu_set(self.ctx, float(s1), float(s2), float(b1), float(b2)), "agd_freeu_set")

    def freeu_clear(self):
        self._ck(self.lib.agd_freeu_clear(self.ctx), "agd_freeu_clear")

    def freeu_counts(self):
        """`agd_freeu_counts`: (FreeU launches that left GroupNorm partial sums, launches that left none) since the engine was created."""
        n = (C.c_longlong * 2)()
        self._ck(self.lib.agd_freeu_counts(self.ctx, n), "agd_freeu_counts")
        return int(n[0]), int(n[1])

    def guidance_rescale_set(self, phi: float):
        """`agd_guidance_rescale_set`: every later evaluation of the DDIM / PLMS / DPM loops rescales its CFG-combined prediction to the text
        branch's per-image standard deviation, blended by phi in [0, 1], until guidance_rescale_clear (0: clear)."""
        self._ck(self.lib.agd_guidance_rescale_set(self.ctx, float(phi)), "agd_guidance_rescale_set")

    def guidance_rescale_clear(self):
        self._ck(self.lib.agd_guidance_rescale_clear(self.ctx), "agd_guidance_rescale_clear")

    def guidance_rescale_counts(self) -> int:
        """`agd_guidance_rescale_counts`: factor launches (one per rescaled evaluation) since the engine was created."""
        n = C.c_longlong(0)
        self._ck(self.lib.agd_guidance_rescale_counts(self.ctx, C.byref(n)), "agd_guidance_rescale_counts")
        return int(n.value)

    def pag_set(self, scales, layers):
        """`agd_pag_set`: Perturbed-Attention Guidance for the calls to come, until pag_clear -- one scale >= 0 per model evaluation, and
        the applied self-attention layers as attn1 module names (`config.self_attn_layer_names`; [] perturbs nothing)."""
        sc = _floats(scales)
        names = [str(n).encode() for n in layers]
        arr = (C.c_char_p * max(len(names), 1))(*names)
        self._ck(self.lib.agd_pag_set(self.ctx, sc, len(scales), arr, len(names)), "agd_pag_set")

    def pag_clear(self):
        self._ck(self.lib.agd_pag_clear(self.ctx), "agd_pag_clear")

    def pag_counts(self) -> Tuple[int, int]:
        """`agd_pag_counts`: (perturbed walks run, perturbed self-attention layers launched) since the engine was created."""
        w, l = C.c_longlong(0), C.c_longlong(0)
        self._ck(self.lib.agd_pag_counts(self.ctx, C.byref(w), C.byref(l)), "agd_pag_counts")
        return int(w.value), int(l.value)

    def sega_set(self, sched: dict, mom_scale: float, mom_beta: float):
        """`agd_sega_set`: Semantic Guidance for the calls to come, until sega_clear -- `sched` is `config.sega_schedule`'s result (the
        per-evaluation coef / w_mom / w_add / add_mom and the concepts' quantiles); the context must then hold (2 + K) B rows."""
        K, n = int(sched["concepts"]), int(sched["n_evals"])
        flat = lambda rows: (C.c_float * (n * K))(*[float(x) for r in rows for x in r])  # noqa: E731
        d = _lib.AgdSegaDesc(struct_size=C.sizeof(_lib.AgdSegaDesc), concepts=K, n_evals=n, mom_scale=float(mom_scale), mom_beta=float(mom_beta),
                             coef=flat(sched["coef"]), q=(C.c_double * K)(*[float(x) for x in sched["q"]]), w_mom=flat(sched["w_mom"]),
                             w_add=flat(sched["w_add"]), add_mom=(C.c_float * n)(*[float(x) for x in sched["add_mom"]]))
        self._ck(self.lib.agd_sega_set(self.ctx, C.byref(d)), "agd_sega_set")

    def sega_clear(self):
        self._ck(self.lib.agd_sega_clear(self.ctx), "agd_sega_clear")

    def sega_counts(self) -> Tuple[int, int]:
        """`agd_sega_counts`: (concept walks run, folds run) since the engine was created."""
        w, f = C.c_longlong(0), C.c_longlong(0)
        self._ck(self.lib.agd_sega_counts(self.ctx, C.byref(w), C.byref(f)), "agd_sega_counts")
        return int(w.value), int(f.value)

    def deepcache_set(self, full_flags, branch: int = 0):
        """`agd_deepcache_set`: DeepCache for the calls to come, until deepcache_clear -- one flag per model evaluation (1 = the full walk,
        0 = the shallow walk at `branch` on the features the last full one cached; `config.deepcache_schedule`)."""
        flags = [int(f) for f in full_flags]
        arr = (C.c_int * max(len(flags), 1))(*flags)
        self._ck(self.lib.agd_deepcache_set(self.ctx, arr, len(flags), int(branch)), "agd_deepcache_set")

    def deepcache_clear(self):
        self._ck(self.lib.agd_deepcache_clear(self.ctx), "agd_deepcache_clear")

    def deepcache_counts(self) -> Tuple[int, int]:
        """`agd_deepcache_counts`: (full evaluations that captured, shallow evaluations) since the engine was created."""
        n = (C.c_longlong * 2)()
        self._ck(self.lib.agd_deepcache_counts(self.ctx, n), "agd_deepcache_counts")
        return int(n[0]), int(n[1])

    def deepcache_forward(self, sample: torch.Tensor, timestep: float, branch: int = 0, shallow: bool = False) -> torch.Tensor:
        """`agd_deepcache_forward_hw`: one evaluation of a DeepCache pair -- shallow=False is unet_forward plus the capture for `branch`,
        shallow=True the shallow walk on that capture (refused on the host when there is no valid one)."""
        sample = sample.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        b2, _, Lh, Lw = sample.shape
        out = torch.empty(b2, self.cfg.unet.out_channels, Lh, Lw, device=sample.device, dtype=torch.float32)
        self._ck(self.lib.agd_deepcache_forward_hw(self.ctx, _lib.ptr(sample), b2, Lh, Lw, float(timestep), int(branch), int(bool(shallow)),
                                                   _lib.ptr(out), self._stream()), "agd_deepcache_forward_hw")
        return out

    def gligen_configure(self, positive_len: int, max_objs: int = 30, fourier_freqs: int = 8):
        self._glcfg = _lib.AgdGligenConfig()
        self._glcfg.struct_size = C.sizeof(_lib.AgdGligenConfig)
        self._glcfg.max_objs, self._glcfg.positive_len, self._glcfg.fourier_freqs = int(max_objs), int(positive_len), int(fourier_freqs)
        self._ck(self.lib.agd_gligen_configure(self.ctx, C.byref(self._glcfg)), "agd_gligen_configure")

    def gligen_set(self, boxes: torch.Tensor, pos_emb: torch.Tensor, masks: torch.Tensor):
        """`agd_gligen_set`: boxes [B2,n,4], phrase embeddings [B2,n,D] and masks [B2,n] (fp32) -> the PositionNet output and every fuser's
        grounding K/V, computed once for the next forwards on B2 rows."""
        boxes, pos_emb, masks = (self._h2d(t).clone().contiguous() for t in (boxes, pos_emb, masks))
        self._ck(self.lib.agd_gligen_set(self.ctx, _lib.ptr(boxes), _lib.ptr(pos_emb), _lib.ptr(masks), int(boxes.shape[0]), self._stream()),
                 "agd_gligen_set")
        self._gl_keepalive = (boxes, pos_emb, masks)

    def gligen_set_schedule(self, flags):
        """One flag per model evaluation of the next fused loop (or one: the next unet_forward); empty clears."""
        n = len(flags)
        arr = (C.c_int * max(n, 1))(*[int(bool(x)) for x in flags])
        self._ck(self.lib.agd_gligen_set_schedule(self.ctx, arr, n), "agd_gligen_set_schedule")

    def gligen_clear(self):
        self._ck(self.lib.agd_gligen_clear(self.ctx), "agd_gligen_clear")

    def gligen_objs(self, batch2: int) -> torch.Tensor:
        """`agd_gligen_objs`: the PositionNet output of the current call, fp32 [B2, max_objs, cross_attention_dim] (cuda)."""
        out = torch.empty(batch2, self._glcfg.max_objs, self.cfg.unet.cross_attention_dim, device=f"cuda:{self.device}", dtype=torch.float32)
        self._ck(self.lib.agd_gligen_objs(self.ctx, _lib.ptr(out)), "agd_gligen_objs")
        return out

    def gligen_fuser(self, block: str, x: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """`agd_gligen_fuser`: one GatedSelfAttentionDense forward of `block` on x fp32 [B2, h*w, C]."""
        x = x.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        self._ck(self.lib.agd_gligen_fuser(self.ctx, block.encode(), _lib.ptr(x), x.shape[0], h, w, _lib.ptr(out), self._stream()),
                 "agd_gligen_fuser")
        return out

    def inpaint_prepare(self, image: torch.Tensor, mask: torch.Tensor, want_image: bool, want_masked: bool):
        """`agd_inpaint_prepare`: image uint8 [B,H,W,3] or float [B,3,H,W] in [-1,1], mask uint8 or float [B,H,W] -> (x, mask_lat): x fp32
        [n B,3,H,W] holds the [-1,1] image rows (want_image), then the masked-image rows (want_masked), ready for one vae_encode; mask_lat
        fp32 [B,1,H/8,W/8] binary."""
        dev = f"cuda:{self.device}"
        img_f32 = image.dtype != torch.uint8
        image = image.to(device=dev, dtype=torch.float32 if img_f32 else torch.uint8).contiguous()
        mask_f32 = mask.dtype != torch.uint8
        mask = mask.to(device=dev, dtype=torch.float32 if mask_f32 else torch.uint8).contiguous()
        b = image.shape[0]
        H, W = tuple(image.shape[2:4]) if img_f32 else tuple(image.shape[1:3])
        f = self.cfg.vae_scale_factor
        x = torch.empty((int(want_image) + int(want_masked)) * b, 3, H, W, device=dev, dtype=torch.float32)
        m = torch.empty(b, 1, H // f, W // f, device=dev, dtype=torch.float32)
        xi = _lib.ptr(x) if want_image else None
        xm = C.c_void_p(x.data_ptr() + (b * 3 * H * W * 4 if want_image else 0)) if want_masked else None
        img_p, mask_p = C.c_void_p(image.data_ptr()), C.c_void_p(mask.data_ptr())
        self._ck(self.lib.agd_inpaint_prepare_hw(self.ctx, img_p, int(img_f32), mask_p, int(mask_f32), b, H, W, xi, xm, _lib.ptr(m),
                                                 self._stream()), "agd_inpaint_prepare_hw")
        self._inpaint_keep = (image, mask)
        return x, m

    def inpaint_set(self, mask: torch.Tensor, cond: torch.Tensor, noise: Optional[torch.Tensor] = None):
        """`agd_inpaint_set`: mask [B,Cm,Lh,Lw] and cond [B,Cc,Lh,Lw] (masked-image latents, or image latents with the noise for the blend)."""
        dev = f"cuda:{self.device}"
        f = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()
        mask, cond, noise = f(mask), f(cond), f(noise)
        b, cm, Lh, Lw = mask.shape
        if cond.shape[0] != b or tuple(cond.shape[2:]) != (Lh, Lw) or (noise is not None and noise.shape != cond.shape):
            raise ValueError(f"inpaint state shapes disagree: mask {tuple(mask.shape)}, cond {tuple(cond.shape)}, "
                             f"noise {None if noise is None else tuple(noise.shape)}")
        self._ck(self.lib.agd_inpaint_set_hw(self.ctx, _lib.ptr(mask), cm, _lib.ptr(cond), cond.shape[1], _lib.ptr(noise), b, Lh, Lw,
                                             self._stream()), "agd_inpaint_set_hw")
        self._inpaint_state = (mask, cond, noise)

    def inpaint_set_schedule(self, sa_sb):
        """The blend's (sa, sb) per model evaluation of the next fused loop."""
        self._ck(self.lib.agd_inpaint_set_schedule(self.ctx, _floats(v for pair in sa_sb for v in pair), len(sa_sb)), "agd_inpaint_set_schedule")

    def inpaint_clear(self):
        self._ck(self.lib.agd_inpaint_clear(self.ctx), "agd_inpaint_clear")
        self._inpaint_state = None

    def ip2p_prepare(self, image: torch.Tensor) -> torch.Tensor:
        """`agd_ip2p_prepare_hw`: image uint8 [B,H,W,3] or float [B,3,H,W] in [-1,1] -> the image latents fp32 [B,c,H/8,W/8]: the VAE
        posterior's mean, not multiplied by the scaling factor."""
        dev = f"cuda:{self.device}"
        img_f32 = image.dtype != torch.uint8
        image = image.to(device=dev, dtype=torch.float32 if img_f32 else torch.uint8).contiguous()
        b = image.shape[0]
        H, W = tuple(image.shape[2:4]) if img_f32 else tuple(image.shape[1:3])
        f = self.cfg.vae_scale_factor
        out = torch.empty(b, self.cfg.vae.latent_channels, H // f, W // f, device=dev, dtype=torch.float32)
        self._ck(self.lib.agd_ip2p_prepare_hw(self.ctx, C.c_void_p(image.data_ptr()), int(img_f32), b, H, W, _lib.ptr(out), self._stream()),
                 "agd_ip2p_prepare_hw")
        return out

    def ip2p_set(self, image_latents: torch.Tensor, image_guidance: float):
        """`agd_ip2p_set_hw`: image latents [B,c,Lh,Lw] (unscaled) and the image guidance scale of the next fused loop."""
        lat = image_latents.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        b, _, Lh, Lw = lat.shape
        if lat.shape[1] != self.cfg.vae.latent_channels:
            raise ValueError(f"image latents have {lat.shape[1]} channels, the VAE's latents {self.cfg.vae.latent_channels}")
        self._ck(self.lib.agd_ip2p_set_hw(self.ctx, _lib.ptr(lat), b, Lh, Lw, float(image_guidance), self._stream()), "agd_ip2p_set_hw")

    def ip2p_clear(self):
        self._ck(self.lib.agd_ip2p_clear(self.ctx), "agd_ip2p_clear")

    def lora_add(self, key: str, down: torch.Tensor, up: torch.Tensor, alpha: float):
        """Stages one target's fp32 factors (down [r, in], up [out, r]) and a copy of its base matrix; the weights stay at the base."""
        d, u = down.detach().to("cpu", torch.float32).contiguous(), up.detach().to("cpu", torch.float32).contiguous()
        self._ck(self.lib.agd_lora_add(self.ctx, key.encode(), C.c_void_p(d.data_ptr()), C.c_void_p(u.data_ptr()), int(d.shape[0]), float(alpha)),
                 f"agd_lora_add({key})")

    def lora_set_scale(self, s: float):
        """Merges the staged LoRA at scale s and rewrites every derived form (no work when s is the current scale)."""
        self._ck(self.lib.agd_lora_set_scale(self.ctx, float(s), self._stream()), "agd_lora_set_scale")

    def lora_clear(self):
        self._ck(self.lib.agd_lora_clear(self.ctx), "agd_lora_clear")

    def text_set_embedding_row(self, token_id: int, row: torch.Tensor):
        row = row.detach().to(torch.float32).contiguous()
        self._ck(self.lib.agd_text_set_embedding_row(self.ctx, int(token_id), C.c_void_p(row.data_ptr())), "agd_text_set_embedding_row")

    def unet_forward(self, sample: torch.Tensor, timestep) -> torch.Tensor:
        """`timestep`: a number (one timestep for the batch) or a [B] tensor / sequence (one per image, the training call)."""
        sample = sample.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        b2, _, Lh, Lw = sample.shape
        out = torch.empty(b2, self.cfg.unet.out_channels, Lh, Lw, device=sample.device, dtype=torch.float32)   # an inpainting or ip2p sample is wider
        ts = timestep.detach().flatten().tolist() if torch.is_tensor(timestep) else (list(timestep) if isinstance(timestep, (list, tuple)) else [timestep])
        if len(ts) == 1:
            self._ck(self.lib.agd_unet_forward_hw(self.ctx, _lib.ptr(sample), b2, Lh, Lw, float(ts[0]), _lib.ptr(out), self._stream()),
                     "agd_unet_forward_hw")
        else:
            if len(ts) != b2:
                raise ValueError(f"timestep has {len(ts)} entries for a batch of {b2}")
            self._ck(self.lib.agd_unet_forward_ts_hw(self.ctx, _lib.ptr(sample), b2, Lh, Lw, _floats(ts), _lib.ptr(out), self._stream()),
                     "agd_unet_forward_ts_hw")
        return out

    def denoise(self, latents: torch.Tensor, timesteps, a_t, a_p, guidance: float):
        assert latents.is_cuda and latents.dtype == torch.float32 and latents.is_contiguous()
        b, _, Lh, Lw = latents.shape
        self._ck(self.lib.agd_denoise_hw(self.ctx, _lib.ptr(latents), b, Lh, Lw, len(timesteps), _floats(timesteps), _floats(a_t), _floats(a_p),
                                         float(guidance), self._stream()), "agd_denoise_hw")
        return latents

    def denoise_panorama(self, canvas: torch.Tensor, window: int, stride: int, view_batch: Optional[int], timesteps, a_t, a_p, guidance: float):
        """The fused MultiDiffusion DDIM loop (`agd_denoise_panorama`) on a canvas [B,4,Lh,Lw] in place: per step every window x window
        view is run and stepped on its own, `view_batch` views of every panorama per UNet call (None: all), then overlap-averaged."""
        assert canvas.is_cuda and canvas.dtype == torch.float32 and canvas.is_contiguous()
        b, _, Lh, Lw = canvas.shape
        self._ck(self.lib.agd_denoise_panorama(self.ctx, _lib.ptr(canvas), b, Lh, Lw, int(window), int(stride), int(view_batch or 0), len(timesteps),
                                               _floats(timesteps), _floats(a_t), _floats(a_p), float(guidance), self._stream()), "agd_denoise_panorama")
        return canvas

    def daam_global_panorama(self, img: int, rows: int, S) -> torch.Tensor:
        """[rows, Lh, Lw] over the canvas of the last denoise_panorama: the overlap mean of the views' global maps (`S`: its (Lh, Lw))."""
        Sh, Sw = _hw(S)
        out = torch.empty(rows, Sh, Sw, device=f"cuda:{self.device}", dtype=torch.float32)
        rc = self.lib.agd_daam_global_panorama(self.ctx, img, rows, _lib.ptr(out), self._stream())
        if rc == -2:
            raise RuntimeError(self.lib.agd_last_error(self.ctx).decode())
        self._ck(rc, "agd_daam_global_panorama")
        return out

    def denoise_regions(self, canvas: torch.Tensor, masks: torch.Tensor, noise: Optional[torch.Tensor], backgrounds: Optional[torch.Tensor],
                        idx, sqrt_ac, bootstrapping: int, timesteps, a_t, a_p, guidance: float):
        """The fused region-based MultiDiffusion DDIM loop (`agd_denoise_regions`) on a canvas [B,4,Lh,Lw] in place.  masks [R,B,Lh,Lw] on
        the device; for the first `bootstrapping` steps: noise [B,4,Lh,Lw], backgrounds [N,4,Lh,Lw], idx[bootstrapping][R-1] (host
        integers) and sqrt_ac[bootstrapping] = (sqrt(ac_t), sqrt(1 - ac_t)) pairs.  The context must hold 2 R B rows."""
        for t in (canvas, masks, noise, backgrounds):
            assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
        b, _, Lh, Lw = canvas.shape
        R = masks.shape[0]
        if tuple(masks.shape) != (R, b, Lh, Lw):
            raise ValueError(f"denoise_regions: masks {tuple(masks.shape)} for a canvas {tuple(canvas.shape)}")
        if noise is not None and tuple(noise.shape) != tuple(canvas.shape):
            raise ValueError(f"denoise_regions: noise {tuple(noise.shape)} for a canvas {tuple(canvas.shape)}")
        if backgrounds is not None and (backgrounds.ndim != 4 or tuple(backgrounds.shape[1:]) != tuple(canvas.shape[1:])):
            raise ValueError(f"denoise_regions: backgrounds {tuple(backgrounds.shape)} for a canvas {tuple(canvas.shape)}")
        flat_idx = [int(v) for row in (idx if idx is not None else []) for v in row]
        flat_ac = [float(v) for pair in (sqrt_ac if sqrt_ac is not None else []) for v in pair]
        if len(flat_idx) != max(int(bootstrapping), 0) * (R - 1) or len(flat_ac) != 2 * max(int(bootstrapping), 0):
            raise ValueError(f"denoise_regions: {len(flat_idx)} indices and {len(flat_ac) // 2} sqrt_ac pairs for {bootstrapping} bootstrapped "
                             f"steps of {R - 1} foreground regions")
        ci = (C.c_int * max(len(flat_idx), 1))(*flat_idx)
        cf = (C.c_float * max(len(flat_ac), 1))(*flat_ac)
        d = _lib.AgdRegionsDesc(struct_size=C.sizeof(_lib.AgdRegionsDesc), regions=R, bootstrapping=int(bootstrapping),
                                n_backgrounds=0 if backgrounds is None else int(backgrounds.shape[0]),
                                masks=masks.data_ptr(), noise=None if noise is None else noise.data_ptr(),
                                backgrounds=None if backgrounds is None else backgrounds.data_ptr(),
                                idx=C.cast(ci, C.POINTER(C.c_int)), sqrt_ac=C.cast(cf, C.POINTER(C.c_float)))
        self._ck(self.lib.agd_denoise_regions(self.ctx, _lib.ptr(canvas), b, Lh, Lw, C.byref(d), len(timesteps), _floats(timesteps), _floats(a_t),
                                              _floats(a_p), float(guidance), self._stream()), "agd_denoise_regions")
        return canvas

    def cfg_ddim_step(self, eps: torch.Tensor, latents: torch.Tensor, guidance: float, alpha_t: float, alpha_prev: float):
        """`scheduler.step` of the call-by-call loop: CFG combine of eps [2B,4,L,L] (rows [0,B) unconditional) + one DDIM
        (eta 0) update of `latents` [B,4,L,L] in place (`agd_cfg_ddim_step`; the fused loop is `denoise`)."""
        assert latents.is_cuda and latents.dtype == torch.float32 and latents.is_contiguous()
        eps = eps.to(device=latents.device, dtype=torch.float32).contiguous()
        b, _, Lh, Lw = latents.shape
        if eps.shape[0] != 2 * b:
            raise ValueError(f"eps batch {eps.shape[0]} != 2 x latents batch {b}")
        self._ck(self.lib.agd_cfg_ddim_step_hw(self.ctx, _lib.ptr(eps), _lib.ptr(latents), b, Lh, Lw, float(guidance), float(alpha_t),
                                               float(alpha_prev), self._stream()), "agd_cfg_ddim_step_hw")
        return latents

    def denoise_plms(self, latents: torch.Tensor, timesteps, sample_coeff, eps_coeff, guidance: float):
        """The fused loop under PNDM/PLMS (`agd_denoise_plms`): len(timesteps) = num_inference_steps + 1 model evaluations."""
        assert latents.is_cuda and latents.dtype == torch.float32 and latents.is_contiguous()
        b, _, Lh, Lw = latents.shape
        self._ck(self.lib.agd_denoise_plms_hw(self.ctx, _lib.ptr(latents), b, Lh, Lw, len(timesteps), _floats(timesteps), _floats(sample_coeff),
                                              _floats(eps_coeff), float(guidance), self._stream()), "agd_denoise_plms_hw")
        return latents

    def denoise_dpm(self, latents: torch.Tensor, timesteps, cx, ce, a, b0, b1, guidance: float):
        """The fused loop under DPM-Solver++ 2M (`agd_denoise_dpm`): one model evaluation per timestep; the per-evaluation
        coefficients are `DPMSolverMultistepScheduler.dpm_program()`'s."""
        assert latents.is_cuda and latents.dtype == torch.float32 and latents.is_contiguous()
        n = len(timesteps)
        if not all(len(x) == n for x in (cx, ce, a, b0, b1)):
            raise ValueError("denoise_dpm: one (cx, ce, a, b0, b1) per timestep")
        co = _floats(v for row in zip(cx, ce, a, b0, b1) for v in row)
        b, _, Lh, Lw = latents.shape
        self._ck(self.lib.agd_denoise_dpm_hw(self.ctx, _lib.ptr(latents), b, Lh, Lw, n, _floats(timesteps), co, float(guidance), self._stream()),
                 "agd_denoise_dpm_hw")
        return latents

    def vae_decode(self, latents: torch.Tensor, want_f32: bool = False):
        latents = latents.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        b, _, Lh, Lw = latents.shape
        f = 2 ** (len(self.cfg.vae.block_out_channels) - 1)
        u8 = torch.empty(b, Lh * f, Lw * f, 3, device=latents.device, dtype=torch.uint8)
        f32 = torch.empty(b, Lh * f, Lw * f, 3, device=latents.device, dtype=torch.float32) if want_f32 else None
        self._ck(self.lib.agd_vae_decode_hw(self.ctx, _lib.ptr(latents), b, Lh, Lw, _lib.ptr(u8), _lib.ptr(f32), self._stream()), "agd_vae_decode_hw")
        return (u8, f32) if want_f32 else u8

    def vae_encode(self, image: torch.Tensor):
        """`vae.encode(image).latent_dist` moments: image [B,3,H,W] in [-1,1] -> (mean, logvar) fp32 [B,4,H/8,W/8]."""
        image = image.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        b, _, H, W = image.shape
        f = 2 ** (len(self.cfg.vae.block_out_channels) - 1)
        mean = torch.empty(b, self.cfg.vae.latent_channels, H // f, W // f, device=image.device, dtype=torch.float32)
        logvar = torch.empty_like(mean)
        self._ck(self.lib.agd_vae_encode_hw(self.ctx, _lib.ptr(image), b, H, W, _lib.ptr(mean), _lib.ptr(logvar), self._stream()), "agd_vae_encode_hw")
        return mean, logvar.clamp_(-30.0, 20.0)

    def set_option(self, name: str, value: int):
        self._ck(self.lib.agd_set_option(self.ctx, name.encode(), int(value)), f"agd_set_option({name})")

    # recorder
    def record_config(self, mode: int, is_train: bool = False, rec_tokens: int = 0):
        self._ck(self.lib.agd_record_config(self.ctx, mode, int(is_train), rec_tokens), "agd_record_config")

    def record_reset(self, batch: int, L):
        """`L`: the latent side, or an (Lh, Lw) pair."""
        Lh, Lw = _hw(L)
        self._ck(self.lib.agd_record_reset_hw(self.ctx, batch, Lh, Lw, self._stream()), "agd_record_reset_hw")

    def daam_global(self, img: int, rows: int, S) -> torch.Tensor:
        """[rows, Lh, Lw] at the size the last record_reset stored; `S`: the latent side, or an (Lh, Lw) pair."""
        Sh, Sw = _hw(S)
        out = torch.empty(rows, Sh, Sw, device=f"cuda:{self.device}", dtype=torch.float32)
        rc = self.lib.agd_daam_global(self.ctx, img, rows, _lib.ptr(out), self._stream())
        if rc == -2:
            raise RuntimeError(self.lib.agd_last_error(self.ctx).decode())
        self._ck(rc, "agd_daam_global")
        return out

    def hook_global(self, bp: int, T: int, S: int) -> torch.Tensor:
        out = torch.empty(bp, T, S, S, device=f"cuda:{self.device}", dtype=torch.float32)
        rc = self.lib.agd_hook_global(self.ctx, _lib.ptr(out), self._stream())
        if rc == -2:
            raise RuntimeError("No heat maps found.")          # hook.py:74-77
        self._ck(rc, "agd_hook_global")
        return out

    def hook_last_map(self, bp: int, T: int, n_query: int) -> torch.Tensor:
        side = int(round(n_query ** 0.5))
        out = torch.empty(bp, T, side, side, device=f"cuda:{self.device}", dtype=torch.float32)
        self._ck(self.lib.agd_hook_last_map(self.ctx, _lib.ptr(out), n_query, self._stream()), "agd_hook_last_map")
        return out

    def hook_count(self) -> int:
        return int(self.lib.agd_hook_count(self.ctx))

    def cross_attn(self, layer: str, hidden: torch.Tensor, ctx_emb: Optional[torch.Tensor], record: bool) -> torch.Tensor:
        hidden = hidden.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        b2, n, _ = hidden.shape
        t = self.cfg.max_tokens
        if ctx_emb is not None:
            ctx_emb = ctx_emb.to(device=hidden.device, dtype=torch.float32).contiguous()
            t = ctx_emb.shape[1]
        out = torch.empty_like(hidden)
        self._ck(self.lib.agd_cross_attn(self.ctx, layer.encode(), _lib.ptr(hidden), _lib.ptr(ctx_emb), b2, n, t,
                                         _lib.ptr(out), int(record), self._stream()), "agd_cross_attn")
        return out

    def attn_processor(self, layer: str, hidden: torch.Tensor, ctx_emb: Optional[torch.Tensor], mask: Optional[torch.Tensor],
                       record: bool) -> torch.Tensor:
        """One `Attention` module call (hook.py:83-122): attn2 with `ctx_emb`, attn1 with `ctx_emb=None`; additive mask [B2, keys]."""
        dev = f"cuda:{self.device}"
        hidden = hidden.to(device=dev, dtype=torch.float32).contiguous()
        b2, n, _ = hidden.shape
        t = 0
        if ctx_emb is not None:
            ctx_emb = ctx_emb.to(device=dev, dtype=torch.float32).contiguous()
            t = ctx_emb.shape[1]
        if mask is not None:
            mask = mask.to(device=dev, dtype=torch.float32).contiguous()
        out = torch.empty_like(hidden)
        self._ck(self.lib.agd_attn_processor(self.ctx, layer.encode(), _lib.ptr(hidden), _lib.ptr(ctx_emb), _lib.ptr(mask), b2, n, t,
                                             _lib.ptr(out), int(record), self._stream()), "agd_attn_processor")
        self._keep = (hidden, ctx_emb, mask)
        return out

    # training-mode seam
    def hook_reset(self, rows: int, L: int):
        self._ck(self.lib.agd_hook_reset(self.ctx, rows, L, self._stream()), "agd_hook_reset")

    def hook_num_maps(self) -> int:
        return int(self.lib.agd_hook_num_maps(self.ctx))

    def hook_map(self, k: int) -> torch.Tensor:
        """The k-th per-call map kept since the last reset (train mode): [B', T, h, w] fp32 (hook.py:110-112)."""
        d = (C.c_int * 3)()
        self._ck(self.lib.agd_hook_map_dims(self.ctx, k, d), "agd_hook_map_dims")
        side = int(round(d[2] ** 0.5))
        out = torch.empty(d[0], d[1], side, side, device=f"cuda:{self.device}", dtype=torch.float32)
        self._ck(self.lib.agd_hook_map(self.ctx, k, _lib.ptr(out), self._stream()), "agd_hook_map")
        return out

    def attn_processor_backward(self, layer: str, hidden: torch.Tensor, ctx_emb: Optional[torch.Tensor], d_out: Optional[torch.Tensor],
                                d_map: Optional[torch.Tensor], is_train: bool, want_hidden: bool = True, want_ctx: bool = True):
        """Backward of one cross-attention seam call: (d_hidden [B2,N,C], d_ctx [B2,T,ctx_dim]) from d_out and/or d_map."""
        dev = f"cuda:{self.device}"
        f = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float32).contiguous()
        hidden, ctx_emb, d_out, d_map = f(hidden), f(ctx_emb), f(d_out), f(d_map)
        b2, n, _ = hidden.shape
        t = ctx_emb.shape[1] if ctx_emb is not None else self.cfg.max_tokens
        if d_map is not None:
            d_map = d_map.reshape(d_map.shape[0], d_map.shape[1], -1).contiguous()
            if d_map.shape[0] != (b2 if is_train else b2 // 2) or d_map.shape[2] != n:
                raise ValueError(f"d_map shape {tuple(d_map.shape)} does not match the recorded map of this call")
        dh = torch.empty_like(hidden) if want_hidden else None
        dc = torch.empty(b2, t, self.cfg.unet.cross_attention_dim, device=dev, dtype=torch.float32) if want_ctx else None
        self._ck(self.lib.agd_attn_processor_backward(self.ctx, layer.encode(), _lib.ptr(hidden), _lib.ptr(ctx_emb), _lib.ptr(d_out), _lib.ptr(d_map),
                                                      int(is_train), b2, n, t, _lib.ptr(dh), _lib.ptr(dc), self._stream()), "agd_attn_processor_backward")
        self._keep = (hidden, ctx_emb, d_out, d_map)
        return dh, dc

    def profile_begin(self):
        self._ck(self.lib.agd_profile_begin(self.ctx), "agd_profile_begin")

    def profile_end(self, mfma_peak_flops: float = 2.5e15, hbm_peak_bytes: float = 8.0e12):
        """Per kernel class: HIP-event ms, algorithmic flop / HBM bytes, launches, and `roof_ms` = the time the binding roof
        (max of flop / MFMA peak and bytes / HBM peak, per launch) allows."""
        n = _lib.AGD_N_CLASSES
        ms, fl, by, rf, rh = ((C.c_double * n)() for _ in range(5))
        ln = (C.c_longlong * n)()
        self._ck(self.lib.agd_profile_end_ex(self.ctx, mfma_peak_flops, hbm_peak_bytes, ms, fl, by, rf, rh, ln), "agd_profile_end_ex")
        return {self.lib.agd_profile_class_name(i).decode(): {"ms": ms[i], "flops": fl[i], "bytes": by[i], "roof_ms": rf[i],
                                                              "roof_ms_hbm_bound": rh[i], "launches": ln[i]} for i in range(n)}


class AttnHandle:
    """Stand-in for a diffusers `Attention` module of the UNet: identifies the layer for the seam."""

    def __init__(self, unet, name: str, heads: int, is_cross: bool):
        self.unet, self.name, self.heads, self.is_cross = unet, name, heads, is_cross
        self.norm_cross = None


class UNetHandle:
    """`pipeline.unet`: config + the attention-processor registry (`set_attn_processor`,
    `attn_processors`; reference finetune_sd_token.py:755-757 installs hook.py's hooker this way)."""

    def __init__(self, pipe):
        self._pipe = pipe
        self.config = pipe.cfg.unet
        self._default = "AttnProcessor(fused-hip)"
        names = cross_attn_layer_names(pipe.cfg.unet, include_mid=True)
        self._attn2 = {n: AttnHandle(self, n, 0, True) for n in names}
        self._attn1 = {n.replace("attn2", "attn1"): AttnHandle(self, n.replace("attn2", "attn1"), 0, False) for n in names}
        self.freeu = None                 # enable_freeu: (s1, s2, b1, b2)
        self._procs = {}
        for n in names:
            self._procs[n + ".processor"] = self._default
            self._procs[n.replace("attn2", "attn1") + ".processor"] = self._default

    @property
    def attn_processors(self):
        return dict(self._procs)

    def set_attn_processor(self, proc):
        from .hook import UNetCrossAttentionHooker
        if isinstance(proc, dict):
            procs = proc
        else:
            procs = {k: proc for k in self._procs}
        hookers = {id(p): p for p in procs.values() if isinstance(p, UNetCrossAttentionHooker)}
        if len(hookers) > 1:
            raise ValueError("only one UNetCrossAttentionHooker instance may be installed (it is shared by all layers)")
        self._procs.update(procs)
        hooker = next(iter(hookers.values()), None)
        self._pipe._install_hooker(hooker)

    def attn2(self, name: str) -> AttnHandle:
        return self._attn2[name]

    def attn1(self, name: str) -> AttnHandle:
        return self._attn1[name]

    def attn(self, name: str) -> AttnHandle:
        """The `Attention` module handle (attn1 = self-, attn2 = cross-attention) the processor is called with."""
        return self._attn2[name] if name in self._attn2 else self._attn1[name]

    def __call__(self, sample, timestep, encoder_hidden_states=None, class_labels=None, return_dict: bool = True, **unused):
        """`unet(sample, t, encoder_hidden_states)`: one fused forward; an installed hooker records its attn2 calls (train mode keeps
        the 16 per-call maps, hook.py:110-112).  finetune_sd_token.py:1027 calls it as
        `unet(noisy_latents, timesteps, encoder_hidden_states, class_labels=None, return_dict=False)[0]` with a per-sample
        [bsz] timestep tensor and without CFG: `timestep` may be a number or a [B] tensor, the result is `UNetOutput(sample=...)`
        (diffusers' UNet2DConditionOutput) or, with return_dict=False, the tuple `(sample,)`.  The maps recorded by this fused
        call are detached (no UNet backward here -- INTEGRATION.md); gradients flow only through direct seam calls."""
        if class_labels is not None:
            raise NotImplementedError("class-conditional UNets (class_labels) are not part of this path")
        if unused:
            raise TypeError(f"unsupported unet() arguments: {sorted(unused)}")
        out = self._forward(sample, timestep, encoder_hidden_states)
        return UNetOutput(sample=out) if return_dict else (out,)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """diffusers' `unet.enable_freeu`: FreeU on every later evaluation of this UNet (the engine holds the state) until disable_freeu."""
        self._pipe.engine.freeu_set(s1, s2, b1, b2)
        self.freeu = (float(s1), float(s2), float(b1), float(b2))

    def disable_freeu(self):
        self._pipe.engine.freeu_clear()
        self.freeu = None

    def _forward(self, sample, timestep, encoder_hidden_states=None):
        if encoder_hidden_states is not None:
            self._pipe.engine.set_context(encoder_hidden_states)
        hk = self._pipe._hooker
        if hk is not None and self._pipe._trace is None:
            hk._ensure(sample.shape[0] if hk.is_train else sample.shape[0] // 2, sample.shape[-1],
                       encoder_hidden_states.shape[1] if encoder_hidden_states is not None else self._pipe.cfg.max_tokens)
        out = self._pipe.engine.unet_forward(sample, timestep)
        if hk is not None:
            hk._cache = (-1, [])
        return out


class VAEHandle:
    def __init__(self, pipe):
        self._pipe = pipe
        self.config = pipe.cfg.vae

    def decode(self, z):
        """`vae.decode(z)`: z already divided by scaling_factor by the caller (diffusers convention)."""
        u8, f32 = self._pipe.engine.vae_decode(z * self.config.scaling_factor, want_f32=True)
        return f32.permute(0, 3, 1, 2)


class StableDiffusionPipeline:
    _gligen = False                       # StableDiffusionGLIGENPipeline loads and runs the position net and the fusers
    def __init__(self, cfg: SDConfig, unet_sd: Dict[str, torch.Tensor], vae_sd: Dict[str, torch.Tensor],
                 tokenizer=None, text_encoder=None, device: Union[int, str] = 0, workspace_bytes: int = 0,
                 text_sd: Optional[Dict[str, torch.Tensor]] = None, scheduler: str = "DDIMScheduler",
                 safety_sd: Optional[Dict[str, torch.Tensor]] = None, pag_applied_layers: Union[str, Sequence[str]] = ("mid",)):
        self.cfg = cfg
        self._deepcache = None                              # enable_deepcache: (cache_interval, cache_branch_id)
        self.set_pag_applied_layers(pag_applied_layers)     # (refuses a string that matches no layer before anything is loaded)
        dev = int(str(device).split(":")[-1]) if not isinstance(device, int) and ":" in str(device) else (device if isinstance(device, int) else 0)
        self.engine = Engine(cfg, dev, workspace_bytes)
        if not self._gligen:      # a GLIGEN (gated) UNet under the plain pipeline: diffusers never runs its fusers, so they are not loaded
            from .gligen import is_gligen_key
            unet_sd = {k: v for k, v in unet_sd.items() if not is_gligen_key(k)}
        self.engine.load_state_dict(unet_sd, "unet.")
        self.engine.load_state_dict(vae_sd, "vae.")
        if text_sd is not None:
            if cfg.text is None:
                raise ValueError("text_sd given but cfg.text is None")
            self.engine.load_state_dict({k[len("text_model."):] if k.startswith("text_model.") else k: v
                                         for k, v in text_sd.items() if "position_ids" not in k}, "text.")
        if (safety_sd is None) != (getattr(cfg, "safety", None) is None):
            raise ValueError("the safety checker needs both cfg.safety and safety_sd")
        if safety_sd is not None:
            self.engine.safety_configure(cfg.safety)
            self.engine.load_state_dict({k: v for k, v in safety_sd.items() if "position_ids" not in k}, "safety.")
        self._load_extra()
        self.engine.finalize()
        self.device = torch.device(f"cuda:{dev}")
        self.tokenizer = tokenizer or SimpleTokenizer(cfg.max_tokens)
        if text_encoder is None and text_sd is not None:
            from .text import HipCLIPTextEncoder
            text_encoder = HipCLIPTextEncoder(self.engine, self.tokenizer, text_sd)
        self.text_encoder = text_encoder or SyntheticTextEncoder(self.tokenizer, cfg.unet.cross_attention_dim)
        if scheduler not in SCHEDULERS:
            raise ValueError(f"scheduler '{scheduler}' is not implemented (have: {sorted(SCHEDULERS)})")
        self.scheduler = SCHEDULERS[scheduler].from_config(cfg.sched)
        self.unet = UNetHandle(self)
        self.vae = VAEHandle(self)
        self.vae_scale_factor = cfg.vae_scale_factor
        self._trace = None
        self._hooker = None
        self._last_prompt = None
        self._last_tokens = None          # the weight-stripped token stream of the last weighted prompt (max_embeddings_multiples), else None
        self._progress = {}
        self._lora = None                 # load_lora_weights: {"targets": n, "fused": scale or None}
        self._ip_adapter = None           # load_ip_adapter: {"embed_dim": E, "n_tokens": n, "scale": s}
        self._image_encoder = None        # the IP-Adapter's image encoder config once loaded (load_ip_adapter / load_image_encoder)
        self._source_path = None          # from_pretrained: the checkpoint directory (save_pretrained re-exports from it)
        # diffusers' `pipeline.safety_checker` slot: None (no checker weights ship with this repo) or a callable
        # images uint8 [B,H,W,3] (cuda tensor) -> sequence of B bools; flagged images are returned black, which the generation
        # driver then skips exactly as data_generation.py:61-62 does
        self.safety_checker = None
        if safety_sd is not None:
            from .safety import HipSafetyChecker
            self.safety_checker = HipSafetyChecker(self.engine, cfg.safety, safety_sd["special_care_embeds_weights"],
                                                   safety_sd["concept_embeds_weights"])

    def _load_extra(self):
        """Models a subclass adds to the engine before it is finalized (StableDiffusionControlNetPipeline: the ControlNet)."""

    # ---- construction -------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, cfg: Union[str, SDConfig] = "sd15", seed: int = 1234, device=0, workspace_bytes: int = 0,
                       weights_device: str = "cpu", keep_weights: bool = False, scheduler: str = "DDIMScheduler",
                       pag_applied_layers: Union[str, Sequence[str]] = ("mid",), **kw):
        from . import synthetic
        cfg = CONFIGS[cfg]() if isinstance(cfg, str) else cfg
        usd = synthetic.make_unet_weights(cfg, seed, device=weights_device, **kw)
        vsd = synthetic.make_vae_weights(cfg, seed + 1, device=weights_device, **kw)
        pipe = cls(cfg, usd, vsd, device=device, workspace_bytes=workspace_bytes, scheduler=scheduler, pag_applied_layers=pag_applied_layers)
        if keep_weights:
            pipe.synthetic_weights = (usd, vsd)
        return pipe

    @classmethod
    def from_pretrained(cls, path: str, device=0, workspace_bytes: int = 0, scheduler: Optional[str] = None, safety_checker=_KEEP, **init_kw):
        """Reads the diffusers on-disk layout (`unet/config.json`, `unet/diffusion_pytorch_model.safetensors`,
        `vae/...`) that `save_pretrained` writes (reference finetune_sd_token.py:164-187).  The safety checker is loaded when
        `model_index.json` names one (`safety_checker/` + `feature_extractor/` must then exist); `safety_checker=None` turns it off
        and any other object is installed in the slot as given, as with diffusers."""
        from safetensors.torch import load_file

        def jload(p):
            with open(p) as f:
                return json.load(f)

        uc = jload(os.path.join(path, "unet", "config.json"))
        vc = jload(os.path.join(path, "vae", "config.json"))
        boc = tuple(uc["block_out_channels"])
        ahd = uc.get("attention_head_dim", 8)
        heads = tuple(ahd) if isinstance(ahd, (list, tuple)) else (ahd,) * len(boc)
        ucfg = UNetConfig(in_channels=uc.get("in_channels", 4), out_channels=uc.get("out_channels", 4), block_out_channels=boc,
                          down_cross=tuple("CrossAttn" in t for t in uc["down_block_types"]),
                          layers_per_block=uc.get("layers_per_block", 2), num_heads=heads,
                          cross_attention_dim=uc.get("cross_attention_dim", 768),
                          use_linear_projection=uc.get("use_linear_projection", False),
                          norm_num_groups=uc.get("norm_num_groups", 32))
        vcfg = VAEConfig(latent_channels=vc.get("latent_channels", 4), out_channels=vc.get("out_channels", 3),
                         block_out_channels=tuple(vc["block_out_channels"]), layers_per_block=vc.get("layers_per_block", 2),
                         norm_num_groups=vc.get("norm_num_groups", 32), scaling_factor=vc.get("scaling_factor", 0.18215))
        sc = SchedulerConfig()
        sched_name = scheduler or "DDIMScheduler"
        sp = os.path.join(path, "scheduler", "scheduler_config.json")
        if os.path.exists(sp):
            sj = jload(sp)
            if scheduler is None:           # the checkpoint's own scheduler, as `from_pretrained` of the reference gives it
                sched_name = sj.get("_class_name", "DDIMScheduler")
                if sched_name not in SCHEDULERS:
                    raise _lib.AgendaHipError(f"{sp}: scheduler '{sched_name}' is not implemented (have: {sorted(SCHEDULERS)}); "
                                              "pass from_pretrained(..., scheduler='DDIMScheduler') to override")
            sc = scheduler_config_from_json(sj, sched_name)
        cfg = SDConfig(name=os.path.basename(path.rstrip("/")), unet=ucfg, vae=vcfg, sched=sc,
                       default_sample_size=uc.get("sample_size", 64))
        src_path = path

        def wload(sub):
            for fn in ("diffusion_pytorch_model.safetensors", "model.safetensors"):
                p = os.path.join(path, sub, fn)
                if os.path.exists(p):
                    return load_file(p)
            raise FileNotFoundError(f"no safetensors weights under {path}/{sub}")

        usd = wload("unet")
        # decoder side for txt2img, encoder side (`vae.encode`, img2img front end) as well
        vsd = {k: v for k, v in wload("vae").items()
               if k.startswith(("decoder.", "post_quant_conv.", "encoder.", "quant_conv."))}
        # pre-0.18 VAE attention naming
        ren = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}
        vsd = {(".".join(ren.get(p, p) for p in k.split(".")) if ".attentions." in k else k): v for k, v in vsd.items()}
        # prompt side: text_encoder/ runs on the device (agd_text_encode); tokenizer/ via transformers when present
        tok = None
        tsd = None
        tcj = os.path.join(path, "text_encoder", "config.json")
        if os.path.exists(tcj):
            from .config import TextConfig
            tj = jload(tcj)
            cfg.text = TextConfig(hidden_size=tj.get("hidden_size", 768), num_hidden_layers=tj.get("num_hidden_layers", 12),
                                  num_attention_heads=tj.get("num_attention_heads", 12), intermediate_size=tj.get("intermediate_size", 3072),
                                  vocab_size=tj.get("vocab_size", 49408), max_position_embeddings=tj.get("max_position_embeddings", 77),
                                  hidden_act=tj.get("hidden_act", "quick_gelu"), layer_norm_eps=tj.get("layer_norm_eps", 1e-5))
            tsd = wload("text_encoder")
        if os.path.isdir(os.path.join(path, "tokenizer")):
            try:
                from transformers import CLIPTokenizer
                tok = CLIPTokenizer.from_pretrained(os.path.join(path, "tokenizer"))
            except Exception as e:
                if tsd is not None:        # real CLIP weights + a word-level stand-in tokenizer = garbage embeddings: refuse
                    raise _lib.AgendaHipError(f"text_encoder/ weights found but tokenizer/ could not be loaded ({e}); "
                                              "no silent fallback to the synthetic tokenizer") from e
                tok = None
        elif tsd is not None:
            raise _lib.AgendaHipError(f"{path}: text_encoder/ weights found but no tokenizer/ directory; "
                                      "no silent fallback to the synthetic tokenizer")
        # the safety checker, when model_index.json names one (diffusers: a non-null entry is loaded or the load fails)
        ssd = None
        mi = os.path.join(path, "model_index.json")
        entry = jload(mi).get("safety_checker") if os.path.exists(mi) else None
        named = isinstance(entry, (list, tuple)) and len(entry) == 2 and entry[0] is not None and entry[1] is not None
        if named and safety_checker is _KEEP:
            from .config import safety_config_from_json
            scj = os.path.join(path, "safety_checker", "config.json")
            fej = os.path.join(path, "feature_extractor", "preprocessor_config.json")
            missing = [p for p in (scj, fej) if not os.path.exists(p)]
            if missing:
                raise _lib.AgendaHipError(f"{mi} names a safety checker but {', '.join(missing)} is missing; "
                                          "pass from_pretrained(..., safety_checker=None) to load without it")
            ssd = wload("safety_checker")
            cfg.safety = safety_config_from_json(jload(scj), jload(fej), n_special=int(ssd["special_care_embeds"].shape[0]),
                                                 n_concepts=int(ssd["concept_embeds"].shape[0]))
        pipe = cls(cfg, usd, vsd, tokenizer=tok, device=device, workspace_bytes=workspace_bytes, text_sd=tsd, scheduler=sched_name,
                   safety_sd=ssd, **init_kw)
        if safety_checker is not _KEEP and safety_checker is not None:
            pipe.safety_checker = safety_checker
        pipe._source_path = src_path
        return pipe

    # ---- LoRA (diffusers 0.21 LoraLoaderMixin surface; merged on the device, lora.py / agd_lora_*) -----------------------------
    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, weight_name: Optional[str] = None, **kwargs):
        """One LoRA adapter for the UNet transformer blocks and the text encoder: a state dict, a file, or a directory holding
        `weight_name` (default pytorch_lora_weights.safetensors, then .bin).  A second load replaces the first.  Its strength is
        `cross_attention_kwargs={"scale": s}` per call (default 1.0), or fixed by fuse_lora()."""
        from . import lora
        entries = lora.lora_to_engine(lora.load_lora_state_dict(pretrained_model_name_or_path_or_dict, weight_name), self.cfg)
        self.unload_lora_weights()
        try:
            for e in entries:
                self.engine.lora_add(e.key, e.down, e.up, e.alpha)
        except Exception:
            self.engine.lora_clear()
            raise
        self._lora = {"targets": len(entries), "fused": None}

    def unload_lora_weights(self):
        """The base weights back (bit for bit) and the LoRA state freed."""
        if getattr(self, "_lora", None) is not None:
            self.engine.lora_clear()
        self._lora = None

    def fuse_lora(self, lora_scale: float = 1.0):
        """Keeps the LoRA merged at `lora_scale`: per-call scales are ignored until unfuse_lora()."""
        if getattr(self, "_lora", None) is None:
            raise ValueError("fuse_lora: no LoRA loaded (load_lora_weights first)")
        self.engine.lora_set_scale(float(lora_scale))
        self._lora["fused"] = float(lora_scale)

    def unfuse_lora(self):
        if getattr(self, "_lora", None) is not None:
            self._lora["fused"] = None

    def _apply_lora_scale(self, cross_attention_kwargs: Optional[dict]):
        """Before the prompt is encoded and the context projected: the call's LoRA scale (a fused scale wins)."""
        st = getattr(self, "_lora", None)
        if st is None:
            return
        s = st["fused"] if st["fused"] is not None else float((cross_attention_kwargs or {}).get("scale", 1.0))
        self.engine.lora_set_scale(s)

    # ---- IP-Adapter (diffusers >= 0.24 IPAdapterMixin surface; ip_adapter.py / agd_ip_adapter_*) -------------------------------------
    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder: Optional[str] = None, weight_name: Optional[str] = None,
                        image_encoder_folder: Optional[str] = "image_encoder"):
        """Loads one plain IP-Adapter (4 image tokens; `.safetensors` or `.bin`) from a state dict, a local file, or `weight_name` under
        `subfolder` of a local directory.  The image branch then runs in every call that passes `ip_adapter_image` or
        `ip_adapter_image_embeds`, at set_ip_adapter_scale's strength.  `image_encoder_folder`: a transformers
        CLIPVisionModelWithProjection directory (config.json + model.safetensors), itself a path or a folder beside the weights; the
        default name is optional (without it only embeddings are taken), any other name that is not found raises.  The call's image
        state stays set in the engine until the next call of this pipeline (a direct engine forward on the same rows runs it too)."""
        from . import ip_adapter as ipa
        for k in type(self).__mro__:
            if k.__name__ in ipa.REFUSED_PIPELINES:
                raise ValueError(f"load_ip_adapter: the IP-Adapter with {k.__name__} is not implemented (StableDiffusionPipeline only)")
        if getattr(self, "_ip_adapter", None) is not None:
            raise ValueError("load_ip_adapter: an IP-Adapter is already loaded; more than one adapter is not supported (unload_ip_adapter first)")
        sd = ipa.load_ip_adapter_state_dict(pretrained_model_name_or_path_or_dict, subfolder, weight_name)
        tensors, embed_dim, n_tokens = ipa.to_engine_tensors(sd, self.cfg)
        enc = ipa.find_image_encoder(pretrained_model_name_or_path_or_dict, subfolder, image_encoder_folder)
        if enc is None and image_encoder_folder not in (None, "image_encoder"):
            raise FileNotFoundError(f"load_ip_adapter: image_encoder_folder '{image_encoder_folder}' holds no config.json (a local transformers "
                                    "CLIPVisionModelWithProjection directory)")
        scfg = esd = None
        if enc is not None and not getattr(self, "_image_encoder", None):
            scfg, esd = ipa.load_image_encoder(enc)
            if scfg.projection_dim != embed_dim:
                raise ValueError(f"load_ip_adapter: the image encoder in {enc} projects to {scfg.projection_dim}, the adapter takes {embed_dim}")
        # everything is read and checked on the host before the engine changes; the adapter goes first, and an encoder the engine
        # refuses takes it out again: a failed call leaves the pipeline as it found it
        self.engine.ip_adapter_load(tensors, embed_dim, n_tokens)
        if scfg is not None:
            try:
                self.engine.image_encoder_load(scfg, esd)
            except Exception:
                self.engine.ip_adapter_unload()
                raise
            self._image_encoder = scfg
        self._ip_adapter = {"embed_dim": embed_dim, "n_tokens": n_tokens, "scale": 1.0}

    def load_image_encoder(self, scfg, sd: Dict[str, torch.Tensor]):
        """The IP-Adapter's image encoder from a config (ip_adapter.image_encoder_config) and a state dict under the transformers keys."""
        if getattr(self, "_image_encoder", None):
            raise ValueError("load_image_encoder: an image encoder is already loaded (one per pipeline; unload_image_encoder first)")
        self.engine.image_encoder_load(scfg, sd)
        self._image_encoder = scfg

    def unload_image_encoder(self):
        if getattr(self, "_image_encoder", None):
            self.engine.image_encoder_unload()
        self._image_encoder = None

    def set_ip_adapter_scale(self, scale: float = 1.0):
        if getattr(self, "_ip_adapter", None) is None:
            raise ValueError("set_ip_adapter_scale: no IP-Adapter loaded (load_ip_adapter first)")
        if isinstance(scale, (list, tuple, dict)):
            raise ValueError("set_ip_adapter_scale: a list-valued scale (per adapter or per layer) is not supported; pass one number")
        if not math.isfinite(float(scale)):
            raise ValueError(f"set_ip_adapter_scale: scale {scale}")
        self._ip_adapter["scale"] = float(scale)

    def unload_ip_adapter(self):
        if getattr(self, "_ip_adapter", None) is not None:
            self.engine.ip_adapter_unload()
        self._ip_adapter = None

    def _apply_ip_adapter(self, B: int, prompt_batch: int, images_per_prompt: int, ip_adapter_image, ip_adapter_image_embeds):
        """The call's image prompt into the engine (after the LoRA scale: the image products are built from the merged to_q / to_out);
        with neither argument a loaded adapter is left idle and the call runs the plain UNet."""
        st = getattr(self, "_ip_adapter", None)
        if ip_adapter_image is not None and ip_adapter_image_embeds is not None:
            raise ValueError("ip_adapter_image and ip_adapter_image_embeds were both given; pass one of them")
        if ip_adapter_image is None and ip_adapter_image_embeds is None:
            if st is not None:
                self.engine.ip_adapter_clear()
            return
        which = "ip_adapter_image" if ip_adapter_image is not None else "ip_adapter_image_embeds"
        if st is None:
            raise ValueError(f"{which} was given but no IP-Adapter is loaded (load_ip_adapter first)")
        from . import ip_adapter as ipa
        if ip_adapter_image is not None:
            enc = getattr(self, "_image_encoder", None)
            if not enc:
                raise ValueError("ip_adapter_image was given but no image encoder is loaded (load_ip_adapter with an image_encoder_folder, or "
                                 "load_image_encoder; or pass ip_adapter_image_embeds)")
            if enc.projection_dim != st["embed_dim"]:
                raise ValueError(f"ip_adapter_image: the image encoder projects to {enc.projection_dim}, the adapter takes {st['embed_dim']}")
            if st["scale"] == 0.0:
                self.engine.ip_adapter_clear()
                return
            ip_adapter_image_embeds = self.engine.image_embeds(ipa.prepare_ip_adapter_image(ip_adapter_image))
        emb = ipa.cfg_image_embeds(ip_adapter_image_embeds, B, prompt_batch, images_per_prompt, st["embed_dim"])
        if st["scale"] == 0.0:
            self.engine.ip_adapter_clear()                     # scale 0: exactly the plain UNet, nothing projected
            return
        self.engine.ip_adapter_set(emb, st["scale"])

    def save_pretrained(self, save_directory: str):
        """`pipeline.save_pretrained(dir)` (finetune_sd_token.py:164-187 writes its result this way): the diffusers layout
        `from_pretrained` reads.  This pipeline is an inference engine -- UNet / VAE / scheduler are exactly what was loaded, so
        their directories are re-exported from the source checkpoint; what CAN have changed is the prompt side
        (`tokenizer.add_tokens` + rows written into `text_encoder.get_input_embeddings().weight`, data_generation.py:45-52): the
        tokenizer is saved with its added tokens and the text encoder with its current (resized) embedding table."""
        import shutil
        from safetensors.torch import load_file, save_file
        if getattr(self, "_lora", None) is not None:
            raise ValueError("save_pretrained: a LoRA is loaded; call unload_lora_weights() to save the base weights")
        if self._source_path is None:
            raise ValueError("save_pretrained: this pipeline was built from in-memory weights (no checkpoint directory to re-export)")
        src, dst = self._source_path, save_directory
        os.makedirs(dst, exist_ok=True)
        same = os.path.realpath(src) == os.path.realpath(dst)          # saving over the source: nothing to copy, only the rewritten files
        from .safety import HipSafetyChecker
        keep_checker = isinstance(self.safety_checker, HipSafetyChecker) and os.path.isdir(os.path.join(src, "safety_checker"))
        for sub in ("unet", "vae", "scheduler") + (("safety_checker", "feature_extractor") if keep_checker else ()):
            if not same and os.path.isdir(os.path.join(src, sub)):
                shutil.copytree(os.path.join(src, sub), os.path.join(dst, sub), dirs_exist_ok=True)
        sched_cls = type(self.scheduler).__name__
        sp = os.path.join(src, "scheduler", "scheduler_config.json")
        sj = {}
        if os.path.exists(sp):
            with open(sp) as f:
                sj = json.load(f)
        if sj.get("_class_name") != sched_cls:
            # the pipeline runs a different scheduler than the source directory names (from_pretrained(..., scheduler=...)): a reload
            # must give the scheduler this pipeline ran, so its config is written from the live objects
            sj = scheduler_config_to_json(sched_cls, self.cfg.sched)
            os.makedirs(os.path.join(dst, "scheduler"), exist_ok=True)
            with open(os.path.join(dst, "scheduler", "scheduler_config.json"), "w") as f:
                json.dump(sj, f, indent=2)
        mi = os.path.join(src, "model_index.json")
        mj = None
        if os.path.exists(mi):
            with open(mi) as f:
                mj = json.load(f)
        if mj is None:
            mj = {"_class_name": "StableDiffusionPipeline", "unet": ["diffusers", "UNet2DConditionModel"], "vae": ["diffusers", "AutoencoderKL"],
                  "text_encoder": ["transformers", "CLIPTextModel"], "tokenizer": ["transformers", "CLIPTokenizer"], "safety_checker": [None, None]}
        mj["scheduler"] = ["diffusers", sched_cls]
        if not keep_checker and isinstance(mj.get("safety_checker"), (list, tuple)) and None not in mj["safety_checker"]:
            mj["safety_checker"] = [None, None]          # loaded with safety_checker=None: the copy has no checker either (diffusers)
        with open(os.path.join(dst, "model_index.json"), "w") as f:
            json.dump(mj, f, indent=2)
        te = os.path.join(src, "text_encoder")
        if os.path.isdir(te):
            os.makedirs(os.path.join(dst, "text_encoder"), exist_ok=True)
            cands = ("model.safetensors", "diffusion_pytorch_model.safetensors")
            fn = next((f for f in cands if os.path.exists(os.path.join(te, f))), None)
            if fn is None:
                raise _lib.AgendaHipError(f"save_pretrained: no single-file safetensors text encoder under {te} (looked for {', '.join(cands)}; "
                                          "pytorch_model.bin and sharded checkpoints are not re-exported)")
            tsd = load_file(os.path.join(te, fn))
            key = next(k for k in tsd if k.endswith("embeddings.token_embedding.weight"))
            w = self.text_encoder.get_input_embeddings().weight
            tsd[key] = w.detach().to(tsd[key].dtype).contiguous().clone()
            save_file(tsd, os.path.join(dst, "text_encoder", fn))
            with open(os.path.join(te, "config.json")) as f:
                tj = json.load(f)
            tj["vocab_size"] = int(w.shape[0])
            with open(os.path.join(dst, "text_encoder", "config.json"), "w") as f:
                json.dump(tj, f, indent=2)
        if hasattr(self.tokenizer, "save_pretrained"):
            self.tokenizer.save_pretrained(os.path.join(dst, "tokenizer"))
        elif os.path.isdir(os.path.join(src, "tokenizer")):
            shutil.copytree(os.path.join(src, "tokenizer"), os.path.join(dst, "tokenizer"), dirs_exist_ok=True)


    def to(self, device):
        if "cuda" not in str(device):
            raise _lib.AgendaHipError("agenda_amd runs on the GPU only")
        return self

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU (Si et al. 2023; diffusers >= 0.22 `pipe.enable_freeu`): in up blocks 0 / 1 the first half of the backbone's channels times
        b1 / b2 and the skip's lowest frequencies times s1 / s2, at every UNet evaluation of every later call, until disable_freeu.
        Suggested: SD-1.4 (0.9, 0.2, 1.2, 1.4), SD-1.5 (0.9, 0.2, 1.5, 1.6), SD-2.1 (0.9, 0.2, 1.4, 1.6).  Not saved by save_pretrained."""
        self.unet.enable_freeu(s1, s2, b1, b2)

    def disable_freeu(self):
        """The plain UNet again, launch for launch: results are bit-identical to a pipeline that never enabled FreeU."""
        self.unet.disable_freeu()

    def enable_deepcache(self, cache_interval: int = 3, cache_branch_id: int = 0, skip_mode: str = "uniform"):
        """DeepCache (Ma, Fang, Wang, CVPR 2024; the upstream DeepCacheSDHelper [upstream-knowledge], parity-unpinned): of every later
        call's model evaluations only each `cache_interval`-th runs the whole UNet; the ones between run conv_in, layers 0 .. cache_branch_id
        of the first down block, the up layers that consume their skips and conv_out, on the deep features the last full evaluation
        cached on the device.  Evaluations count from 0 per call.  The state persists like FreeU's until disable_deepcache; `to()` and LoRA
        scale changes leave it alone and save_pretrained does not write it.  cache_interval=1 sets nothing: the plain call, bit for bit.
        The recorders see the attn2 layers that run, so the deep layers' maps accumulate on full evaluations only."""
        check_deepcache(cache_interval, cache_branch_id, self.cfg.unet.layers_per_block, skip_mode)
        self._deepcache = (cache_interval, cache_branch_id)

    def disable_deepcache(self):
        """The plain loops again, launch for launch: results are bit-identical to a pipeline that never enabled DeepCache."""
        self._deepcache = None

    def set_pag_applied_layers(self, layers: Union[str, Sequence[str]]):
        """diffusers' `pag_applied_layers` (the constructor / from_pretrained keyword of StableDiffusionPAGPipeline, default ["mid"]): every
        string is `re.search`ed against the UNet's self-attention module names (`config.self_attn_layer_names`); the layers they match are
        the ones the perturbed branch of a call with pag_scale > 0 runs with an identity attention map.  A string that matches none is a
        ValueError naming it."""
        from .config import resolve_pag_layers
        pats = [layers] if isinstance(layers, str) else list(layers)
        self._pag_layers = resolve_pag_layers(self.cfg, pats)
        self.pag_applied_layers = pats

    def set_progress_bar_config(self, **kw):
        self._progress = kw

    # ---- recorder plumbing --------------------------------------------------------------
    def _install_hooker(self, hooker):
        self._hooker = hooker
        if hooker is not None:
            hooker._bind(self)
        self._apply_record_mode()

    def _apply_record_mode(self):
        if self._trace is not None:
            self.engine.record_config(1, False, self._trace.rec_tokens)
        elif self._hooker is not None:
            self.engine.record_config(2, self._hooker.is_train, 0)
        else:
            self.engine.record_config(0)

    # ---- prompt -------------------------------------------------------------------------
    def encode_prompt(self, prompts: List[str], negative: Optional[List[str]] = None) -> torch.Tensor:
        """[uncond x B, cond x B] context, the CFG batch order (hook.py:48-49)."""
        neg = negative if negative is not None else [""] * len(prompts)
        self._last_prompt, self._last_tokens = prompts[0], None
        return torch.cat([self.text_encoder(neg), self.text_encoder(prompts)], 0)

    def encode_prompt_weighted(self, prompts: List[str], negative: Optional[List[str]], max_embeddings_multiples: int) -> torch.Tensor:
        """`encode_prompt` through the weighted / long-prompt encoder (lpw.py): [uncond x B, cond x B] of T = 75 m_eff + 2 rows."""
        from . import lpw
        neg = negative if negative is not None else [""] * len(prompts)
        emb, toks = lpw.encode_weighted(self.tokenizer, self.text_encoder, prompts, neg, max_embeddings_multiples)
        self._last_prompt, self._last_tokens = prompts[0], toks
        return emb

    def _expand_prompts(self, prompt, negative_prompt, num_images_per_prompt: int, prompt_embeds: Optional[torch.Tensor],
                        max_embeddings_multiples: Optional[int] = None):
        """The call's context and how it was batched: (prompt_embeds, prompt batch, images per prompt).  `prompt` is a string or a list,
        every entry repeated num_images_per_prompt times; `negative_prompt` a string (for every row) or one entry per row.  Given
        `prompt_embeds` are taken as they are, one image per row.  max_embeddings_multiples: None = the plain encoder (parentheses stay
        literal, 75 tokens), 1 .. 4 = the weighted one for prompt and negative_prompt."""
        if prompt_embeds is not None:
            return prompt_embeds, prompt_embeds.shape[0] // 2, 1
        prompts = [prompt] if isinstance(prompt, str) else list(prompt)
        pb = len(prompts)
        prompts = [p for p in prompts for _ in range(num_images_per_prompt)]
        negs = None if negative_prompt is None else ([negative_prompt] * len(prompts) if isinstance(negative_prompt, str) else list(negative_prompt))
        if max_embeddings_multiples is not None:
            return self.encode_prompt_weighted(prompts, negs, max_embeddings_multiples), pb, num_images_per_prompt
        return self.encode_prompt(prompts, negs), pb, num_images_per_prompt

    def _refuse_long_beside(self, prompt_embeds: torch.Tensor, max_embeddings_multiples, ip_adapter_image=None, ip_adapter_image_embeds=None):
        """Weighted / long prompts run the plain UNet recorded by trace() alone: an installed hooker and an active IP-Adapter refuse the
        argument, and a context over 96 tokens."""
        T = prompt_embeds.shape[1]
        if T <= LONG_CONTEXT and max_embeddings_multiples is None:
            return
        what = f"max_embeddings_multiples={max_embeddings_multiples!r}" if max_embeddings_multiples is not None else f"a context of {T} tokens (over {LONG_CONTEXT})"
        if self._hooker is not None:
            raise ValueError(f"a UNetCrossAttentionHooker is installed: {what} is not implemented with it (weighted / long prompts record "
                             "through trace()); remove it with unet.set_attn_processor('default')")
        st = getattr(self, "_ip_adapter", None)
        if (ip_adapter_image is not None or ip_adapter_image_embeds is not None) and st is not None and st["scale"] != 0.0:
            raise ValueError(f"an active IP-Adapter (scale {st['scale']!r}): {what} is not implemented with it; "
                             "leave the image prompt out or set_ip_adapter_scale(0)")

    def _draw_latents(self, B: int, Lh: int, Lw: int, generator, latents: Optional[torch.Tensor]) -> torch.Tensor:
        """The initial latents [B, C, Lh, Lw] on the device, scaled by the scheduler's init_noise_sigma: `latents` when given, else drawn."""
        Cl = self.cfg.unet.out_channels
        if latents is None:
            # data_generation.py:58 seeds `torch.Generator(device="cuda")`: accepted (torch's device Philox stream; whether it is
            # bit-identical to an NVIDIA run of the reference is not verifiable here).  CPU generators give host-reproducible latents.
            if isinstance(generator, (list, tuple)):           # diffusers randn_tensor: one (1, C, Lh, Lw) draw per generator
                if len(generator) != B:
                    raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch size of {B}.")
                parts = [torch.randn(1, Cl, Lh, Lw, generator=g, device=g.device if g is not None else "cpu") for g in generator]
                if len({p_.device for p_ in parts}) > 1:
                    parts = [p_.cpu() for p_ in parts]
                latents = torch.cat(parts, 0)
            else:                                              # ONE (B, C, Lh, Lw) draw, kept on the generator's device (no host round trip)
                latents = torch.randn(B, Cl, Lh, Lw, generator=generator, device=generator.device if generator is not None else "cpu")
        expect = (B, Cl, Lh, Lw)
        if tuple(latents.shape) != expect:                 # diffusers prepare_latents raises the same way
            raise ValueError(f"Unexpected latents shape, got {tuple(latents.shape)}, expected {expect}")
        return self.engine._h2d(latents.to(torch.float32) * self.scheduler.init_noise_sigma).clone()

    def _begin_recording(self, prompt_embeds: torch.Tensor, B: int, L, context: Optional[torch.Tensor] = None):
        """Sets the call's context and, with a tracer or a hooker installed, starts their recording of B images at latent size L.
        `context`: what the engine gets when it is more than the prompts' rows (Semantic Guidance's concept rows behind them)."""
        self.engine.set_context(prompt_embeds if context is None else context)
        self._apply_record_mode()
        T = prompt_embeds.shape[1]
        if self._trace is not None and T > LONG_CONTEXT:       # a long context records its T rows, unless the tracer was given rec_tokens
            self.engine.record_config(1, False, self._trace._rows_for(T))
        if self._trace is not None or self._hooker is not None:
            self.engine.record_reset(B, L)
            if self._trace is not None:
                self._trace._on_generate(B, L, self._last_prompt, tokens=self._last_tokens, context_tokens=T)
            if self._hooker is not None:
                self._hooker._on_generate(B, L, prompt_embeds.shape[1])

    # ---- txt2img ------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None,
                 generator: Union[torch.Generator, Sequence[torch.Generator], None] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil", num_images_per_prompt: int = 1,
                 cross_attention_kwargs: Optional[dict] = None, ip_adapter_image=None, ip_adapter_image_embeds=None,
                 guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 max_embeddings_multiples: Optional[int] = None,
                 editing_prompt: Union[str, List[str], None] = None, editing_prompt_embeddings: Optional[torch.Tensor] = None,
                 reverse_editing_direction=False, edit_guidance_scale=5, edit_warmup_steps=10, edit_cooldown_steps=None, edit_threshold=0.9,
                 edit_momentum_scale: float = 0.1, edit_mom_beta: float = 0.4, edit_weights=None, sem_guidance=None):
        from .lpw import check_multiples
        check_multiples(max_embeddings_multiples)
        self._refuse_inpainting_unet()
        check_guidance_rescale(guidance_rescale)
        check_pag(pag_scale, pag_adaptive_scale, guidance_rescale)
        sega = check_sega(editing_prompt, editing_prompt_embeddings, reverse_editing_direction, edit_guidance_scale, edit_warmup_steps,
                          edit_cooldown_steps, edit_threshold, edit_momentum_scale, edit_mom_beta, edit_weights, sem_guidance, pag_scale,
                          guidance_rescale, getattr(self, "_deepcache", None), getattr(self, "_ip_adapter", None), ip_adapter_image,
                          ip_adapter_image_embeds, max_embeddings_multiples)
        refuse_deepcache_beside(getattr(self, "_deepcache", None), pag_scale, getattr(self, "_ip_adapter", None), ip_adapter_image, ip_adapter_image_embeds)
        self._apply_lora_scale(cross_attention_kwargs)
        side = self.cfg.default_sample_size * self.vae_scale_factor
        height, width = height or side, width or side
        check_image_size(height, width)
        Lh, Lw = height // self.vae_scale_factor, width // self.vae_scale_factor
        self._refuse_rectangular_hook(Lh, Lw)
        L = Lh if Lh == Lw else (Lh, Lw)                       # the square path passes one side, exactly as before
        prompt_embeds, pb, ipp = self._expand_prompts(prompt, negative_prompt, num_images_per_prompt, prompt_embeds, max_embeddings_multiples)
        B = prompt_embeds.shape[0] // 2
        self._refuse_long_beside(prompt_embeds, max_embeddings_multiples, ip_adapter_image, ip_adapter_image_embeds)
        context = self._sega_context(sega, prompt_embeds, B)   # (its refusals come as soon as the prompts' context is known: nothing is on the device yet)
        self._apply_ip_adapter(B, pb, ipp, ip_adapter_image, ip_adapter_image_embeds)
        lat = self._draw_latents(B, Lh, Lw, generator, latents)
        self._begin_recording(prompt_embeds, B, L, context)
        with self._guidance_rescaled(guidance_rescale), self._pag(pag_scale, pag_adaptive_scale, self.scheduler, num_inference_steps), \
                self._deepcached(self.scheduler, num_inference_steps), self._sega(sega, self.scheduler, num_inference_steps):
            self._denoise(lat, num_inference_steps, guidance_scale)
        if output_type == "latent":
            return PipelineOutput(images=[], latents=lat)
        return self._finish(lat, B, output_type)

    def _refuse_rectangular_hook(self, Lh: int, Lw: int):
        """hook.py's `_unravel_attn` unravels every map as h = w = sqrt(N): a rectangular generate has no meaning there."""
        if self._hooker is not None and Lh != Lw:
            raise ValueError(f"UNetCrossAttentionHooker records square latents only (h = w = sqrt(N), as hook.py's _unravel_attn); "
                             f"got a {Lh * self.vae_scale_factor} x {Lw * self.vae_scale_factor} generate")

    def _refuse_inpainting_unet(self):
        u = self.cfg.unet
        if u.in_channels == u.out_channels + self.cfg.vae.latent_channels:
            raise ValueError(f"this UNet takes {u.in_channels} input channels (an InstructPix2Pix checkpoint): txt2img and img2img need "
                             f"{u.out_channels}; use StableDiffusionInstructPix2PixPipeline")
        if u.in_channels != u.out_channels:
            raise ValueError(f"this UNet takes {u.in_channels} input channels (an inpainting checkpoint): txt2img and img2img need "
                             f"{u.out_channels}; use StableDiffusionInpaintPipeline")

    @contextlib.contextmanager
    def _guidance_rescaled(self, guidance_rescale: float):
        """diffusers' `guidance_rescale` (Lin et al. 2023, section 3.4) around one call's denoise loop: the engine state is set for the loop
        and cleared when it ends, on an error too, so the next call without the argument is the plain one.  0 sets nothing."""
        if not guidance_rescale:
            yield
            return
        self.engine.guidance_rescale_set(guidance_rescale)
        try:
            yield
        finally:
            self.engine.guidance_rescale_clear()

    @contextlib.contextmanager
    def _pag(self, pag_scale: float, pag_adaptive_scale: float, scheduler, num_inference_steps: int, strength: float = 1.0):
        """Perturbed-Attention Guidance (Ahn et al. 2024; diffusers >= 0.30 StableDiffusionPAGPipeline) around one call's denoise loop: the
        scale of every model evaluation (`config.pag_schedule` over `inpaint.evaluation_timesteps`) and the applied layers are set for the
        loop and cleared when it ends, on an error too, so the next call without the argument is the plain one.  0 sets nothing."""
        if not pag_scale:
            yield
            return
        from .config import pag_schedule
        from .inpaint import evaluation_timesteps
        sched = pag_schedule(evaluation_timesteps(scheduler, num_inference_steps, strength), pag_scale, pag_adaptive_scale)
        self.engine.pag_set(sched, self._pag_layers)
        try:
            yield
        finally:
            self.engine.pag_clear()

    def _sega_context(self, sega: Optional[dict], prompt_embeds: torch.Tensor, B: int) -> Optional[torch.Tensor]:
        """The context of a Semantic Guidance call: [uncond x B | cond x B | concept_0 x B | ... | concept_{K-1} x B], the concepts shared by
        the call's images (an editing prompt is encoded as a prompt is).  None without concepts.  A context over 96 tokens and given
        embeddings of another shape are refused before anything is encoded."""
        if sega is None:
            return None
        T, D = prompt_embeds.shape[1], prompt_embeds.shape[2]
        if T > LONG_CONTEXT:
            raise ValueError(f"a context of {T} tokens (over {LONG_CONTEXT}) with an editing prompt: Semantic Guidance with long prompts is not implemented")
        if sega["embeds"] is not None and tuple(sega["embeds"].shape[1:]) != (T, D):
            raise ValueError(f"editing_prompt_embeddings of shape {tuple(sega['embeds'].shape)}: the prompts' context has {T} tokens of {D} (expected [K, {T}, {D}])")
        emb = sega["embeds"] if sega["embeds"] is not None else self.text_encoder(sega["prompts"])
        if tuple(emb.shape[1:]) != (T, D):
            raise ValueError(f"editing_prompt encodes to {tuple(emb.shape)}: the prompts' context has {T} tokens of {D} (expected [K, {T}, {D}])")
        emb = emb.to(device=prompt_embeds.device, dtype=prompt_embeds.dtype)
        return torch.cat([prompt_embeds, emb.repeat_interleave(B, dim=0)], 0)

    @contextlib.contextmanager
    def _sega(self, sega: Optional[dict], scheduler, num_inference_steps: int, strength: float = 1.0):
        """Semantic Guidance (Brack et al. 2023; diffusers 0.21.2 SemanticStableDiffusionPipeline) around one call's denoise loop: the
        schedule of every model evaluation (`config.sega_schedule` over the length of `inpaint.evaluation_timesteps`) is set for the loop and
        cleared when it ends, on an error too, so the next call without an editing prompt is the plain one.  None sets nothing."""
        if sega is None:
            yield
            return
        from .config import sega_schedule
        from .inpaint import evaluation_timesteps
        sched = sega_schedule(len(evaluation_timesteps(scheduler, num_inference_steps, strength)), sega["K"], **sega["args"])
        self.engine.sega_set(sched, sega["mu"], sega["beta"])
        try:
            yield
        finally:
            self.engine.sega_clear()

    @contextlib.contextmanager
    def _deepcached(self, scheduler, num_inference_steps: int, strength: float = 1.0):
        """DeepCache around one call's denoise loop: the full / shallow flag of every model evaluation (`config.deepcache_schedule` over the
        length of `inpaint.evaluation_timesteps`) is set for the loop and cleared when it ends, on an error too.  Disabled, or interval 1,
        sets nothing."""
        if self._deepcache is None or self._deepcache[0] == 1:
            yield
            return
        from .config import deepcache_schedule
        from .inpaint import evaluation_timesteps
        interval, branch = self._deepcache
        self.engine.deepcache_set(deepcache_schedule(len(evaluation_timesteps(scheduler, num_inference_steps, strength)), interval), branch)
        try:
            yield
        finally:
            self.engine.deepcache_clear()

    def _denoise(self, lat, num_inference_steps, guidance_scale):
        """`for t in scheduler.timesteps: unet -> CFG -> scheduler.step`, fused on the device, under the pipeline's scheduler."""
        ts = self.scheduler.set_timesteps(num_inference_steps)
        if isinstance(self.scheduler, PNDMScheduler):
            tsf, ca, cb = self.scheduler.plms_program()
            self.engine.denoise_plms(lat, tsf, ca, cb, guidance_scale)
        elif isinstance(self.scheduler, DPMSolverMultistepScheduler):
            self.engine.denoise_dpm(lat, *self.scheduler.dpm_program(), guidance_scale)
        else:
            a_t, a_p = self.scheduler.step_coeffs()
            self.engine.denoise(lat, ts, a_t, a_p, guidance_scale)

    def _finish(self, lat, B, output_type):
        u8 = self.engine.vae_decode(lat)
        flags = [False] * B
        if self.safety_checker is not None:        # diffusers run_safety_checker: flagged images come back black
            flags = [bool(f) for f in self.safety_checker(u8)]
            if len(flags) != B:
                raise ValueError(f"safety_checker returned {len(flags)} flags for {B} images")
            if any(flags):
                u8 = u8.clone()
                u8[torch.tensor(flags, device=u8.device)] = 0
        if output_type == "pt":
            return PipelineOutput(images=u8, latents=lat, nsfw_content_detected=flags)
        arr = u8.cpu().numpy()
        if output_type == "np":
            return PipelineOutput(images=arr, latents=lat, nsfw_content_detected=flags)
        from PIL import Image
        return PipelineOutput(images=[Image.fromarray(a) for a in arr], latents=lat, nsfw_content_detected=flags)

    # ---- img2img (diffusers StableDiffusionImg2ImgPipeline semantics, parity-unpinned) ------
    @torch.no_grad()
    def img2img(self, prompt=None, image: torch.Tensor = None, strength: float = 0.8, num_inference_steps: int = 50,
                guidance_scale: float = 7.5, generator: Optional[torch.Generator] = None, prompt_embeds: Optional[torch.Tensor] = None,
                noise_enc: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, output_type: str = "pil",
                cross_attention_kwargs: Optional[dict] = None, ip_adapter_image=None, ip_adapter_image_embeds=None,
                guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                max_embeddings_multiples: Optional[int] = None,
                editing_prompt: Union[str, List[str], None] = None, editing_prompt_embeddings: Optional[torch.Tensor] = None,
                reverse_editing_direction=False, edit_guidance_scale=5, edit_warmup_steps=10, edit_cooldown_steps=None, edit_threshold=0.9,
                edit_momentum_scale: float = 0.1, edit_mom_beta: float = 0.4, edit_weights=None, sem_guidance=None):
        """image: float [B,3,H,W] in [-1,1] (or uint8 [B,H,W,3]).  Noise draws come from a CPU generator (or are passed
        explicitly) for the same host-reproducibility reason as the txt2img latents."""
        from .lpw import check_multiples
        check_multiples(max_embeddings_multiples)
        # img2img runs the strength-truncated DDIM schedule.  A checkpoint whose own scheduler is PNDM (SD-1.x) or DPM-Solver++ gets a
        # DDIM scheduler built from the same scheduler config for this call (the reference has no img2img call site; strength-truncated
        # PLMS and DPM-Solver++ img2img are not implemented)
        self._refuse_inpainting_unet()
        check_guidance_rescale(guidance_rescale)
        check_pag(pag_scale, pag_adaptive_scale, guidance_rescale)
        sega = check_sega(editing_prompt, editing_prompt_embeddings, reverse_editing_direction, edit_guidance_scale, edit_warmup_steps,
                          edit_cooldown_steps, edit_threshold, edit_momentum_scale, edit_mom_beta, edit_weights, sem_guidance, pag_scale,
                          guidance_rescale, getattr(self, "_deepcache", None), getattr(self, "_ip_adapter", None), ip_adapter_image,
                          ip_adapter_image_embeds, max_embeddings_multiples)
        refuse_deepcache_beside(getattr(self, "_deepcache", None), pag_scale, getattr(self, "_ip_adapter", None), ip_adapter_image, ip_adapter_image_embeds)
        self._apply_lora_scale(cross_attention_kwargs)
        sched = self.scheduler if isinstance(self.scheduler, DDIMScheduler) else DDIMScheduler.from_config(self.cfg.sched)
        if image.dtype == torch.uint8:
            image = image.permute(0, 3, 1, 2).float() / 127.5 - 1.0
        B, _, H, W = image.shape
        if H != W:                                             # (square images keep the acceptance they always had)
            check_image_size(H, W)
        Lh, Lw = H // self.vae_scale_factor, W // self.vae_scale_factor
        self._refuse_rectangular_hook(Lh, Lw)
        L = Lh if Lh == Lw else (Lh, Lw)
        if prompt_embeds is None:
            prompts = [prompt] * B if isinstance(prompt, str) else list(prompt)
            prompt_embeds = self.encode_prompt(prompts) if max_embeddings_multiples is None else \
                self.encode_prompt_weighted(prompts, None, max_embeddings_multiples)
        self._refuse_long_beside(prompt_embeds, max_embeddings_multiples, ip_adapter_image, ip_adapter_image_embeds)
        context = self._sega_context(sega, prompt_embeds, B)   # (refused here, before the image prompt, the noise draws and the VAE encode)
        self._apply_ip_adapter(B, B, 1, ip_adapter_image, ip_adapter_image_embeds)
        shape = (B, self.cfg.unet.out_channels, Lh, Lw)
        if generator is not None and generator.device.type != "cpu":
            raise ValueError("use a CPU torch.Generator")
        noise_enc = noise_enc if noise_enc is not None else torch.randn(shape, generator=generator)
        noise = noise if noise is not None else torch.randn(shape, generator=generator)
        ts = sched.set_timesteps(num_inference_steps)
        a_t, a_p = sched.step_coeffs()
        init = min(int(num_inference_steps * strength), num_inference_steps)
        t0 = max(num_inference_steps - init, 0)
        ts, a_t, a_p = ts[t0:], a_t[t0:], a_p[t0:]
        mean, logvar = self.engine.vae_encode(image)
        x0 = (mean + torch.exp(0.5 * logvar) * noise_enc.to(mean.device)) * self.cfg.vae.scaling_factor
        a = float(sched.alphas_cumprod[int(ts[0])])
        lat = (a ** 0.5 * x0 + (1 - a) ** 0.5 * noise.to(mean.device)).contiguous()
        self._begin_recording(prompt_embeds, B, L, context)
        with self._guidance_rescaled(guidance_rescale), self._pag(pag_scale, pag_adaptive_scale, sched, num_inference_steps, strength), \
                self._deepcached(sched, num_inference_steps, strength), self._sega(sega, sched, num_inference_steps, strength):
            self.engine.denoise(lat, ts, a_t, a_p, guidance_scale)
        if output_type == "latent":
            return PipelineOutput(images=[], latents=lat)
        return self._finish(lat, B, output_type)
