"""`StableDiffusionRegionPipeline`: region-based MultiDiffusion (Bar-Tal et al. 2023) txt2img -- every region of the image has its own prompt
and mask, and one latent is denoised under all of them at once.

Restated from the MultiDiffusion repository's `region_based.py` from memory [upstream-knowledge].  Parity-unpinned: diffusers 0.21.2 has no
such pipeline, so nothing here is checked against an installed upstream.  Region 0 is the background (its prompt is `prompt`, its mask
`max(0, 1 - sum of the foreground masks)`); regions 1 .. R - 1 are `region_prompts` with `region_masks` / `region_boxes`.  Every step the one
latent canvas is handed to every region, the CFG UNet runs all R x B rows in ONE forward (each against its own context), the DDIM step
updates them, and every latent pixel becomes `sum_r m_r x_r / sum_r m_r`.  For the first `bootstrapping` steps a foreground region sees,
outside its mask, a randomly chosen constant-colour background noised to the step's level, so the object stays inside the mask.  The whole
loop is `agd_denoise_regions` on the device: spread -> UNet -> CFG + DDIM -> masked mean (csrc/regions.hip).

Row (region r, image p) is `r * B + p` everywhere: the UNet batch within a CFG half, the latent masks and the DAAM states.

Deliberate differences from upstream:
 * every image of a batch is independent (its own background prompt, optionally its own masks);
 * there are no views: the UNet runs the whole latent, at any size the plain pipeline accepts;
 * DDIM only;
 * `trace(pipe)` keeps one DAAM state per (region, image); `compute_region_word_heat_map` composes them over the canvas with the masks
   that generated each pixel (this project's definition, trace.py).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from .pipeline import (LONG_CONTEXT, PipelineOutput, StableDiffusionPipeline, check_image_size, refuse_deepcache, refuse_long_prompt, refuse_pag, refuse_sega)
from .scheduler import DDIMScheduler

MAX_REGIONS = 8        # R, the background included (AGD_MAX_REGIONS)
NAME = "StableDiffusionRegionPipeline"


def _is_pil_list(x) -> bool:
    return isinstance(x, (list, tuple)) and len(x) > 0 and all(hasattr(m, "convert") for m in x)


def rasterize_boxes(boxes, height: int, width: int) -> torch.Tensor:
    """Normalised `x0, y0, x1, y1` boxes [..., 4] -> uint8 masks [..., H, W], box b set on `[int(y0 H):int(y1 H), int(x0 W):int(x1 W)]`."""
    b = torch.as_tensor(boxes, dtype=torch.float64)
    if b.ndim not in (2, 3) or b.shape[-1] != 4:
        raise ValueError(f"region_boxes must be [R - 1][4] or [B][R - 1][4] (x0, y0, x1, y1 in [0, 1]), got shape {tuple(b.shape)}")
    flat = b.reshape(-1, 4).tolist()
    out = torch.zeros(len(flat), height, width, dtype=torch.uint8)
    for k, (x0, y0, x1, y1) in enumerate(flat):
        if not (0.0 <= x0 < x1 <= 1.0 and 0.0 <= y0 < y1 <= 1.0):
            raise ValueError(f"region box {k} = {[x0, y0, x1, y1]}: needs 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1")
        out[k, int(y0 * height):int(y1 * height), int(x0 * width):int(x1 * width)] = 255
    return out.reshape(*b.shape[:-1], height, width)


def pixel_masks(region_masks, height: int, width: int) -> torch.Tensor:
    """`region_masks` as given (bool, uint8 or float tensor / array, or a list of PIL "L" images) -> a uint8 or fp32 tensor
    [R - 1, H, W] or [B, R - 1, H, W]; thresholding is the kernel's (uint8 > 127, float > 0.5)."""
    import numpy as np
    if _is_pil_list(region_masks):
        region_masks = np.stack([np.asarray(m.convert("L")) for m in region_masks])
    m = torch.as_tensor(np.asarray(region_masks) if isinstance(region_masks, (list, tuple)) else region_masks)
    if m.dtype == torch.bool:
        m = m.to(torch.uint8) * 255
    elif m.dtype != torch.uint8:
        m = m.to(torch.float32)
    if m.ndim not in (3, 4):
        raise ValueError(f"region_masks must be [R - 1, H, W] or [B, R - 1, H, W], got shape {tuple(m.shape)}")
    if tuple(m.shape[-2:]) != (height, width):
        raise ValueError(f"region_masks are {m.shape[-2]} x {m.shape[-1]}, the image is {height} x {width}")
    return m


def check_region_count(scheduler_name: str, n_region_prompts: int) -> None:
    """The scheduler and the number of regions: DDIM only, at most MAX_REGIONS regions with the background."""
    if scheduler_name != "DDIMScheduler":
        raise ValueError(f"{NAME} runs DDIM only, this pipeline's scheduler is {scheduler_name} (per-region multistep state is not "
                         f"implemented); load it with from_pretrained(..., scheduler=\"DDIMScheduler\")")
    if n_region_prompts + 1 > MAX_REGIONS:
        raise ValueError(f"{n_region_prompts} region prompts: at most {MAX_REGIONS} regions in all, the background included (R <= {MAX_REGIONS})")


def check_region_args(scheduler_name: str, n_region_prompts: int, region_masks, region_boxes, height: int, width: int,
                      batch: Optional[int] = None) -> Optional[torch.Tensor]:
    """Everything the pipeline refuses about its region arguments, known before a device is touched (generation.py checks its flags with it
    too).  Returns the pixel masks, uint8 or fp32 [R - 1, H, W] or [B, R - 1, H, W] on the host (None without foreground regions)."""
    check_region_count(scheduler_name, n_region_prompts)
    if n_region_prompts == 0:
        if region_masks is not None or region_boxes is not None:
            n = len(region_masks if region_masks is not None else region_boxes)
            if n:
                raise ValueError(f"{n} region masks / boxes for 0 region prompts (one per region prompt)")
        return None
    if (region_masks is None) == (region_boxes is None):
        raise ValueError("give exactly one of region_masks and region_boxes (got " + ("both" if region_masks is not None else "neither") + ")")
    m = pixel_masks(region_masks, height, width) if region_masks is not None else rasterize_boxes(region_boxes, height, width)
    what = "masks" if region_masks is not None else "boxes"
    if m.shape[-3] != n_region_prompts:
        raise ValueError(f"{m.shape[-3]} region {what} for {n_region_prompts} region prompts (one per region prompt)")
    if m.ndim == 4 and batch is not None and m.shape[0] != batch:
        raise ValueError(f"per-image region {what} for {m.shape[0]} images, the call makes {batch}")
    return m


class StableDiffusionRegionPipeline(StableDiffusionPipeline):
    last_region_state: Optional[dict] = None     # the last call's bootstrap draws: colors, noise, backgrounds, idx (tests read it)

    @classmethod
    def from_synthetic(cls, cfg="sd15", seed: int = 1234, device=0, workspace_bytes: int = 0, weights_device: str = "cpu",
                       keep_weights: bool = False, scheduler: str = "DDIMScheduler", **kw):
        """Random weights as StableDiffusionPipeline.from_synthetic, plus the VAE encoder (the bootstrap backgrounds are encoded once per
        call; the decoder's weights do not depend on it)."""
        from . import synthetic
        from .config import CONFIGS
        cfg = CONFIGS[cfg]() if isinstance(cfg, str) else cfg
        usd = synthetic.make_unet_weights(cfg, seed, device=weights_device, **kw)
        vsd = synthetic.make_vae_weights(cfg, seed + 1, device=weights_device, with_encoder=True, **kw)
        pipe = cls(cfg, usd, vsd, device=device, workspace_bytes=workspace_bytes, scheduler=scheduler)
        if keep_weights:
            pipe.synthetic_weights = (usd, vsd)
        return pipe

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, region_prompts: Optional[Sequence[str]] = None, region_masks=None,
                 region_boxes=None, region_negative_prompts: Optional[Sequence[str]] = None, bootstrapping: int = 20,
                 bootstrap_backgrounds: Optional[torch.Tensor] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None, num_images_per_prompt: int = 1,
                 generator: Union[torch.Generator, Sequence[torch.Generator], None] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, region_prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil",
                 cross_attention_kwargs: Optional[dict] = None, guidance_rescale: float = 0.0, pag_scale: float = 0.0,
                 pag_adaptive_scale: float = 0.0, max_embeddings_multiples: Optional[int] = None, ip_adapter_image=None,
                 ip_adapter_image_embeds=None, editing_prompt=None, editing_prompt_embeddings=None, sem_guidance=None):
        # ---- refusals: all by name, before any device work ------------------------------------------------------------------------
        refuse_pag(NAME, pag_scale, pag_adaptive_scale)
        refuse_sega(NAME, editing_prompt, editing_prompt_embeddings, sem_guidance)
        refuse_deepcache(NAME, getattr(self, "_deepcache", None))
        refuse_long_prompt(NAME, max_embeddings_multiples, prompt_embeds)
        if region_prompt_embeds is not None and region_prompt_embeds.shape[-2] > LONG_CONTEXT:
            refuse_long_prompt(NAME, None, region_prompt_embeds.reshape(-1, *region_prompt_embeds.shape[-2:]))
        if guidance_rescale:
            raise ValueError(f"guidance_rescale={guidance_rescale!r}: guidance rescale is not implemented for {NAME} (its regions are "
                             "stepped one by one); leave it 0")
        st = getattr(self, "_ip_adapter", None)
        if ip_adapter_image is not None or ip_adapter_image_embeds is not None or (st is not None and st.get("scale", 0.0) != 0.0):
            raise ValueError(f"an active IP-Adapter: image prompts are not implemented for {NAME}; leave the image prompt out and "
                             "unload_ip_adapter() or set_ip_adapter_scale(0)")
        self._refuse_inpainting_unet()
        if self._hooker is not None:
            raise ValueError("a UNetCrossAttentionHooker is installed: region prompts record through trace() only (hook.py's maps are one "
                             "generate of one prompt); remove it with unet.set_attn_processor('default')")
        f = self.vae_scale_factor
        side = self.cfg.default_sample_size * f
        height, width = height or side, width or side
        check_image_size(height, width)
        if region_prompt_embeds is not None:
            if region_prompts:
                raise ValueError("give region_prompts or region_prompt_embeds, not both")
            if region_prompt_embeds.ndim != 4:
                raise ValueError(f"region_prompt_embeds must be [R - 1, 2, T, D] or [R - 1, 2B, T, D], got {tuple(region_prompt_embeds.shape)}")
            n = int(region_prompt_embeds.shape[0])
        else:
            if isinstance(region_prompts, str):
                raise ValueError("region_prompts is a list of strings, one per foreground region")
            region_prompts = list(region_prompts or [])
            n = len(region_prompts)
        if prompt_embeds is not None:
            B = prompt_embeds.shape[0] // 2
        else:
            if prompt is None:
                raise ValueError("give prompt (the background's) or prompt_embeds")
            B = (1 if isinstance(prompt, str) else len(list(prompt))) * num_images_per_prompt
        px = check_region_args(type(self.scheduler).__name__, n, region_masks, region_boxes, height, width, B)
        R = n + 1
        if region_negative_prompts is not None and (isinstance(region_negative_prompts, str) or len(region_negative_prompts) != n):
            raise ValueError(f"region_negative_prompts: one string per region prompt ({n}), got {region_negative_prompts!r}")
        if isinstance(bootstrapping, bool) or not isinstance(bootstrapping, int) or bootstrapping < 0:
            raise ValueError(f"bootstrapping={bootstrapping!r}: a number of steps >= 0")
        Lh, Lw = height // f, width // f
        Cl = self.cfg.unet.out_channels
        boot = min(bootstrapping, num_inference_steps) if R > 1 else 0
        if bootstrap_backgrounds is not None and boot > 0:
            if bootstrap_backgrounds.ndim != 4 or tuple(bootstrap_backgrounds.shape[1:]) != (Cl, Lh, Lw) or bootstrap_backgrounds.shape[0] < 1:
                raise ValueError(f"bootstrap_backgrounds must be [N, {Cl}, {Lh}, {Lw}] with N >= 1, got {tuple(bootstrap_backgrounds.shape)}")
        assert isinstance(self.scheduler, DDIMScheduler)
        # ---- contexts: [uncond x R B | cond x R B], row r * B + p ------------------------------------------------------------------
        self._apply_lora_scale(cross_attention_kwargs)
        reg = None                                               # [n, 2 or 2B, T, D]
        if region_prompt_embeds is not None:
            reg = region_prompt_embeds
        elif n:
            negs = list(region_negative_prompts) if region_negative_prompts is not None else \
                [negative_prompt if isinstance(negative_prompt, str) else ""] * n
            keep = (getattr(self, "_last_prompt", None), getattr(self, "_last_tokens", None))
            e = self.encode_prompt(region_prompts, negs)         # [uncond x n | cond x n]
            self._last_prompt, self._last_tokens = keep          # (the tracer's prompt stays the background's)
            reg = torch.stack([e[:n], e[n:]], 1)
        prompt_embeds = self._expand_prompts(prompt, negative_prompt, num_images_per_prompt, prompt_embeds)[0]
        if prompt_embeds.shape[0] != 2 * B:
            raise ValueError(f"prompt_embeds of {prompt_embeds.shape[0]} rows for {B} images")
        un, co = [prompt_embeds[:B]], [prompt_embeds[B:]]
        for r in range(n):
            e = reg[r].to(prompt_embeds.device, prompt_embeds.dtype)
            if e.shape[0] == 2:
                un.append(e[0:1].expand(B, -1, -1)); co.append(e[1:2].expand(B, -1, -1))
            elif e.shape[0] == 2 * B:
                un.append(e[:B]); co.append(e[B:])
            else:
                raise ValueError(f"region_prompt_embeds hold {e.shape[0]} rows per region, need 2 (shared) or 2B = {2 * B}")
            if tuple(e.shape[1:]) != tuple(prompt_embeds.shape[1:]):
                raise ValueError(f"region_prompt_embeds are {tuple(e.shape[1:])} per row, prompt_embeds {tuple(prompt_embeds.shape[1:])}")
        ctx = torch.cat(un + co, 0).contiguous()                 # [2 R B, T, D]
        # ---- draws: the initial latents first (the plain pipeline's for the same seed), then colours, sampling noise, choices --------
        lat = self._draw_latents(B, Lh, Lw, generator, latents)
        g = generator[0] if isinstance(generator, (list, tuple)) else generator
        gdev = g.device if g is not None else "cpu"
        state = {"colors": None, "noise": None, "backgrounds": None, "idx": None}
        bgs = idx = None
        if boot > 0:
            if bootstrap_backgrounds is not None:
                bgs = self.engine._h2d(bootstrap_backgrounds.to(torch.float32)).contiguous()
            else:
                colors = torch.rand(boot, 3, generator=g, device=gdev)
                e = torch.randn(boot, self.cfg.vae.latent_channels, Lh, Lw, generator=g, device=gdev)
                state["colors"], state["noise"] = colors, e
                bgs = self._encode_backgrounds(colors, e, height, width)
            idx = torch.randint(0, bgs.shape[0], (boot, n), generator=g, device=gdev).cpu()
            state["backgrounds"], state["idx"] = bgs, idx
        self.last_region_state = state
        from . import ops
        masks = ops.region_masks(None if px is None else px.to(f"cuda:{self.engine.device}"), B, Lh, Lw, regions=R)   # [R, B, Lh, Lw], one launch per call
        # ---- the loop ---------------------------------------------------------------------------------------------------------------
        self.engine.set_context(ctx)
        self._apply_record_mode()
        if self._trace is not None:
            self.engine.record_reset(R * B, Lh if Lh == Lw else (Lh, Lw))       # one DAAM state per (region, image): image r * B + p
            prompts = None if region_prompt_embeds is not None else [self._last_prompt if prompt is not None else None] + list(region_prompts)
            self._trace._on_generate(B, Lh if Lh == Lw else (Lh, Lw), self._last_prompt, regions={"prompts": prompts, "masks": masks, "count": R})
        ts = self.scheduler.set_timesteps(num_inference_steps)
        a_t, a_p = self.scheduler.step_coeffs()
        sq = [(float(a_t[s]) ** 0.5, (1.0 - float(a_t[s])) ** 0.5) for s in range(boot)]
        self.engine.denoise_regions(lat, masks, lat.clone() if boot > 0 else None, bgs, idx.tolist() if idx is not None else None, sq, boot,
                                    ts, a_t, a_p, guidance_scale)
        if output_type == "latent":
            return PipelineOutput(images=[], latents=lat)
        return self._finish(lat, B, output_type)

    def _encode_backgrounds(self, colors: torch.Tensor, e: torch.Tensor, height: int, width: int, chunk: int = 4) -> torch.Tensor:
        """N constant-colour images (`2 c - 1` in [-1, 1]) -> [N, 4, Lh, Lw]: the VAE posterior sampled as img2img does
        (`mean + exp(0.5 logvar) * e`), times the scaling factor."""
        out = []
        for k in range(0, colors.shape[0], chunk):
            img = (2.0 * colors[k:k + chunk].to(torch.float32) - 1.0)[:, :, None, None].expand(-1, -1, height, width)
            mean, logvar = self.engine.vae_encode(img)
            out.append((mean + torch.exp(0.5 * logvar) * e[k:k + chunk].to(mean.device)) * self.cfg.vae.scaling_factor)
        return torch.cat(out, 0).contiguous()

    def img2img(self, *a, **kw):
        raise NotImplementedError("img2img with region prompts is not implemented; use StableDiffusionPipeline")
