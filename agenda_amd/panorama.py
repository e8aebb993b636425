"""`StableDiffusionPanoramaPipeline`: MultiDiffusion (Bar-Tal et al. 2023) txt2img on a latent canvas larger than the UNet's field of view.

Restated from diffusers 0.21.2 `StableDiffusionPanoramaPipeline` [upstream-knowledge]: every denoising step runs the CFG UNet and the
scheduler step on overlapping window-sized views of ONE latent (`get_views`, window = the UNet's sample size, stride 8 latent pixels) and
sets every latent pixel to the mean of the stepped views that cover it (`value[view] += stepped; count[view] += 1;
latents = where(count > 0, value / count, value)`, the sum in view order).  Here the whole loop is `agd_denoise_panorama` on the device:
window gather -> UNet -> CFG + DDIM on the views, one overlap mean per step (csrc/panorama.hip).

Deliberate differences:
 * `view_batch_size=None` (default) runs all views of a step in one UNet call; diffusers' default of 1 is a memory setting and changes no
   result.  An integer is honoured.
 * every panorama of a batch is independent and equals its own batch-1 result (diffusers pairs `repeat_interleave(2)` latents with
   `[uncond; cond]` embeddings, which is only right for one prompt);
 * DDIM only: diffusers keeps one scheduler state per view for multistep solvers, which is not built here;
 * `circular_padding` is not implemented and is refused;
 * `trace(pipe)` heat maps cover the canvas: the overlap mean of the views' global maps (this project's definition, trace.py).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch

from .pipeline import PipelineOutput, StableDiffusionPipeline, refuse_deepcache, refuse_long_prompt, refuse_pag, refuse_sega
from .scheduler import DDIMScheduler

STRIDE = 8            # latent pixels between views (diffusers get_views default)


def get_views(panorama_height: int, panorama_width: int, window_size: int = 64, stride: int = 8) -> List[Tuple[int, int, int, int]]:
    """diffusers `StableDiffusionPanoramaPipeline.get_views` [upstream-knowledge]: pixel sizes in, latent windows
    (h_start, h_end, w_start, w_end) out, row-major."""
    lh, lw = panorama_height // 8, panorama_width // 8
    nbh = (lh - window_size) // stride + 1 if lh > window_size else 1
    nbw = (lw - window_size) // stride + 1 if lw > window_size else 1
    views = []
    for i in range(nbh * nbw):
        hs, ws = (i // nbw) * stride, (i % nbw) * stride
        views.append((hs, hs + window_size, ws, ws + window_size))
    return views


def check_panorama_size(height: int, width: int, window: int, stride: int = STRIDE, scale: int = 8) -> None:
    """Each side a multiple of the view stride (stride * scale pixels) and at least the window (window * scale pixels)."""
    step, least = stride * scale, window * scale
    if not all(isinstance(v, int) and v >= least and v % step == 0 for v in (height, width)):
        raise ValueError(f"a panorama's height and width must each be a multiple of {step} and at least the UNet window of {least} pixels, "
                         f"got height={height}, width={width}")


def check_panorama_args(scheduler_name: str, height: int, width: int, window: int, view_batch_size: Optional[int] = None,
                        circular_padding: bool = False, scale: int = 8) -> None:
    """Everything the pipeline refuses that is known before a device is touched (generation.py checks its flags with it too)."""
    if scheduler_name != "DDIMScheduler":
        raise ValueError(f"StableDiffusionPanoramaPipeline runs DDIM only, this pipeline's scheduler is {scheduler_name} (per-view multistep "
                         f"state is not implemented); load it with from_pretrained(..., scheduler=\"DDIMScheduler\")")
    if circular_padding:
        raise ValueError("circular_padding=True is not implemented (the views never wrap around the canvas)")
    check_panorama_size(height, width, window, STRIDE, scale)
    if view_batch_size is not None and (not isinstance(view_batch_size, int) or view_batch_size < 1):
        raise ValueError(f"view_batch_size must be None (all views per UNet call) or a positive integer, got {view_batch_size!r}")


class StableDiffusionPanoramaPipeline(StableDiffusionPipeline):
    get_views = staticmethod(get_views)

    @property
    def window(self) -> int:
        """The view side in latent pixels: the UNet's `sample_size` (64 SD-1.x, 96 SD-2.1 768)."""
        return int(self.cfg.default_sample_size)

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, view_batch_size: Optional[int] = None,
                 circular_padding: bool = False, negative_prompt=None, num_images_per_prompt: int = 1,
                 generator: Union[torch.Generator, Sequence[torch.Generator], None] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil", cross_attention_kwargs: Optional[dict] = None,
                 guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 max_embeddings_multiples: Optional[int] = None, editing_prompt=None, editing_prompt_embeddings=None, sem_guidance=None):
        refuse_pag("StableDiffusionPanoramaPipeline", pag_scale, pag_adaptive_scale)
        refuse_sega("StableDiffusionPanoramaPipeline", editing_prompt, editing_prompt_embeddings, sem_guidance)
        refuse_deepcache("StableDiffusionPanoramaPipeline", getattr(self, "_deepcache", None))
        refuse_long_prompt("StableDiffusionPanoramaPipeline", max_embeddings_multiples, prompt_embeds)
        if guidance_rescale:
            raise ValueError(f"guidance_rescale={guidance_rescale!r}: guidance rescale is not implemented for the panorama pipeline "
                             "(its views are stepped one by one); leave it 0")
        f, win = self.vae_scale_factor, self.window
        height = height or f * win
        width = width or 4 * height
        self._refuse_inpainting_unet()
        check_panorama_args(type(self.scheduler).__name__, height, width, win, view_batch_size, circular_padding, f)
        if self._hooker is not None:
            raise ValueError("a UNetCrossAttentionHooker is installed: a panorama records through trace() only (hook.py's maps are one "
                             "square generate); remove it with unet.set_attn_processor('default')")
        assert isinstance(self.scheduler, DDIMScheduler)
        self._apply_lora_scale(cross_attention_kwargs)
        Lh, Lw = height // f, width // f
        n_views = len(get_views(height, width, win, STRIDE))
        prompt_embeds = self._expand_prompts(prompt, negative_prompt, num_images_per_prompt, prompt_embeds)[0]
        B = prompt_embeds.shape[0] // 2
        lat = self._draw_latents(B, Lh, Lw, generator, latents)       # ONE latent of the canvas size, drawn exactly as for txt2img
        self.engine.set_context(prompt_embeds)                 # the [2B, T, D] of the prompts; the loop tiles its projections per view
        self._apply_record_mode()
        if self._trace is not None:
            self.engine.record_reset(B * n_views, win)         # one DAAM state per (panorama, view): image v * B + p
            self._trace._on_generate(B, (Lh, Lw), self._last_prompt, panorama=True)
        ts = self.scheduler.set_timesteps(num_inference_steps)
        a_t, a_p = self.scheduler.step_coeffs()
        self.engine.denoise_panorama(lat, win, STRIDE, view_batch_size, ts, a_t, a_p, guidance_scale)
        if output_type == "latent":
            return PipelineOutput(images=[], latents=lat)
        return self._finish(lat, B, output_type)

    def img2img(self, *a, **kw):
        raise NotImplementedError("img2img on a panorama is not implemented; use StableDiffusionPipeline")
