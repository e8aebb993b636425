"""Inpainting: diffusers' `StableDiffusionInpaintPipeline` (0.21.2 semantics) over the device engine.

Two flavours, chosen by the UNet's input width (`config.inpaint_flavour`):
 * a 9-channel inpainting UNet ("concat") reads latents | mask | masked-image latents at every evaluation: the fused loops build that
   64-channel bf16 input in place of txt2img's 4-channel one (`agd_inpaint_set`, inpaint.hip prep_inpaint_kernel);
 * a 4-channel UNet ("blend", e.g. the project's own fine-tuned SD-1.4) runs as txt2img, and after every scheduler step the latents are
   blended with the image latents noised to the next timestep: x = (1 - m) (sa image_latents + sb noise) + m x (inpaint.hip
   inpaint_blend_kernel), with (sa, sb) per evaluation from `blend_schedule`.
The mask front end (image to [-1,1], masked image, latent-resolution binary mask) is one kernel per call, and the image and the masked
image go through the VAE encoder as one batch.  DAAM and the hook.py hooker see the UNet, as in txt2img.
Rules restated from the published pipeline are marked [upstream-knowledge].  Deliberate differences:
 * the blend uses each image's own latents and mask; 0.21.2 blends every row with the first image's (the two agree whenever all rows
   share one image and mask);
 * the 4-channel flavour does not encode the masked image: 0.21.2 encodes it there only to discard it (it consumes generator draws,
   which are skipped here too);
 * `latents=` is taken as the noise draw and the start follows the strength rule (0.21.2 starts from `latents` whatever the strength);
 * an image batch of 1 serves every row, else it pairs with the prompts (repeat_interleave over num_images_per_prompt), as the
   ControlNet pipeline does.
Refused: strength < 1 under PNDM / DPM-Solver++, the blend with Karras sigmas, UNet widths other than 4 and 9, ControlNet inpainting.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .config import SDConfig, inpaint_flavour, inpaint_variant
from .pipeline import PipelineOutput, StableDiffusionPipeline, check_guidance_rescale, check_image_size, refuse_deepcache, refuse_long_prompt, refuse_pag, refuse_sega
from .scheduler import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler


def prepare_mask_and_image(image, mask_image, height: int, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """[upstream-knowledge] `VaeImageProcessor.preprocess` for image and mask, up to the point the device front end takes over.
    image: PIL image(s) (RGB) or a uint8 [B,H,W,3] tensor -> uint8 [B,H,W,3] (x / 255 then 2 x - 1 on the device), or a float [B,3,H,W]
    tensor already in [-1,1].  mask_image: PIL image(s) (converted to "L") or a uint8 [B,H,W] / [B,1,H,W] tensor -> uint8 [B,H,W] (/ 255 on
    the device), or a float tensor in [0,1].  Sizes other than height x width are refused (nothing is resized)."""
    from PIL import Image

    def pil_list(x):
        if isinstance(x, Image.Image):
            return [x]
        if isinstance(x, (list, tuple)) and x and all(isinstance(i, Image.Image) for i in x):
            return list(x)
        return None

    ims = pil_list(image)
    if ims is not None:
        img = torch.from_numpy(np.stack([np.asarray(i.convert("RGB")) for i in ims]))
    elif torch.is_tensor(image) and image.ndim == 4:
        if image.dtype == torch.uint8:
            if image.shape[3] != 3:
                raise ValueError(f"uint8 images are [B,H,W,3], got {tuple(image.shape)}")
            img = image
        else:
            if image.shape[1] != 3:
                raise ValueError(f"float images are [B,3,H,W] in [-1,1], got {tuple(image.shape)}")
            img = image.to(torch.float32)
    else:
        raise ValueError("image: a PIL image, a list of PIL images, a uint8 [B,H,W,3] or a float [B,3,H,W] tensor")
    ms = pil_list(mask_image)
    if ms is not None:
        mask = torch.from_numpy(np.stack([np.asarray(m.convert("L")) for m in ms]))
    elif torch.is_tensor(mask_image) and mask_image.ndim in (3, 4):
        mask = mask_image
        if mask.ndim == 4:
            if mask.shape[1] != 1:
                raise ValueError(f"mask tensors are [B,H,W] or [B,1,H,W], got {tuple(mask.shape)}")
            mask = mask[:, 0]
        if mask.dtype != torch.uint8:
            mask = mask.to(torch.float32)
    else:
        raise ValueError("mask_image: a PIL image, a list of PIL images, or a [B,H,W] / [B,1,H,W] tensor")
    hw = tuple(img.shape[2:]) if img.dtype != torch.uint8 else tuple(img.shape[1:3])
    if hw != (height, width) or tuple(mask.shape[1:]) != (height, width):
        raise ValueError(f"image {hw[0]}x{hw[1]} and mask {mask.shape[1]}x{mask.shape[2]} must both be {height}x{width} "
                         "(inputs are not resized)")
    if mask.shape[0] not in (1, img.shape[0]) and img.shape[0] != 1:
        raise ValueError(f"image batch {img.shape[0]} and mask batch {mask.shape[0]} disagree")
    n = max(img.shape[0], mask.shape[0])
    img = img.expand(n, *img.shape[1:]) if img.shape[0] == 1 else img
    mask = mask.expand(n, *mask.shape[1:]) if mask.shape[0] == 1 else mask
    return img.contiguous(), mask.contiguous()


def evaluation_timesteps(scheduler, num_inference_steps: int, strength: float = 1.0) -> List[int]:
    """The UNet timesteps of the loop, one per model evaluation (PNDM's repeated second entry included; DDIM truncated by strength)."""
    scheduler.set_timesteps(num_inference_steps)
    if isinstance(scheduler, PNDMScheduler):
        ts = scheduler.plms_program()[0]
    elif isinstance(scheduler, DPMSolverMultistepScheduler):
        ts = scheduler.dpm_program()[0]
    else:
        ts = scheduler.timesteps
    ts = [int(round(float(t))) for t in ts]
    if strength < 1.0:
        return ts[strength_start(num_inference_steps, strength):]
    return ts


def strength_start(num_inference_steps: int, strength: float) -> int:
    """[upstream-knowledge] `get_timesteps`: the first of the num_inference_steps timesteps the loop runs."""
    init = min(int(num_inference_steps * strength), num_inference_steps)
    return max(num_inference_steps - init, 0)


def blend_schedule(scheduler, timesteps: Sequence[int]) -> List[Tuple[float, float]]:
    """[upstream-knowledge] The 4-channel blend after the step of evaluation i: `scheduler.add_noise(image_latents, noise, t_{i+1})`,
    i.e. (sa, sb) = (sqrt(abar(t_{i+1})), sqrt(1 - abar(t_{i+1}))), computed in float64; the image latents themselves, (1, 0), after the
    last step."""
    ac = np.asarray(scheduler.alphas_cumprod, dtype=np.float64)
    out = []
    for i in range(len(timesteps)):
        if i + 1 < len(timesteps):
            a = float(ac[int(timesteps[i + 1])])
            out.append((float(np.sqrt(a)), float(np.sqrt(1.0 - a))))
        else:
            out.append((1.0, 0.0))
    return out


def check_request(cfg: SDConfig, scheduler, strength: float, num_inference_steps: int) -> str:
    """The refusals of one inpainting call, before anything runs; returns the flavour ("concat" or "blend")."""
    flavour = inpaint_flavour(cfg)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must be in (0, 1], got {strength}")
    if num_inference_steps * strength < 1:
        raise ValueError(f"num_inference_steps * strength = {num_inference_steps * strength} < 1: the loop would run no step")
    if strength < 1.0 and not isinstance(scheduler, DDIMScheduler):
        raise ValueError(f"strength < 1 runs the strength-truncated DDIM schedule only (the pipeline's scheduler is {type(scheduler).__name__})")
    if flavour == "blend" and getattr(scheduler, "use_karras_sigmas", False):
        raise ValueError("the 4-channel blend with use_karras_sigmas is not implemented (add_noise would need integer timesteps)")
    return flavour


def draw_noises(generator, n_images: int, batch: int, c: int, L, need_image: bool, need_masked: bool, noise_enc_image=None,
                noise=None, noise_enc_masked=None):
    """The call's N(0, 1) draws in diffusers' order [upstream-knowledge]: the image's posterior sample (when its latents are needed),
    the start noise, the masked image's posterior sample (9-channel UNets).  Explicit tensors replace draws; a draw is taken only where
    no tensor is given.  CPU generators only (host-reproducible).  `L`: the latent side, or an (Lh, Lw) pair."""
    Lh, Lw = (L, L) if isinstance(L, int) else tuple(L)
    if generator is not None and (not isinstance(generator, torch.Generator) or generator.device.type != "cpu"):
        raise ValueError("use one CPU torch.Generator")
    ne = me = None
    if need_image:
        ne = noise_enc_image if noise_enc_image is not None else torch.randn(n_images, c, Lh, Lw, generator=generator)
    nz = noise if noise is not None else torch.randn(batch, c, Lh, Lw, generator=generator)
    if need_masked:
        me = noise_enc_masked if noise_enc_masked is not None else torch.randn(n_images, c, Lh, Lw, generator=generator)
    return ne, nz, me


class StableDiffusionInpaintPipeline(StableDiffusionPipeline):
    """`StableDiffusionInpaintPipeline`: `pipe(prompt, image, mask_image, ...)`; everything else is StableDiffusionPipeline's."""

    def __init__(self, cfg: SDConfig, unet_sd, vae_sd, **kw):
        if "controlnet" in kw:
            raise NotImplementedError("ControlNet inpainting is not implemented")
        inpaint_flavour(cfg)
        super().__init__(cfg, unet_sd, vae_sd, **kw)

    @classmethod
    def from_synthetic(cls, cfg: Union[str, SDConfig] = "sd15", seed: int = 1234, device=0, workspace_bytes: int = 0,
                       weights_device: str = "cpu", keep_weights: bool = False, scheduler: str = "DDIMScheduler", inpaint: bool = True, **kw):
        """Random weights; inpaint=True gives the preset's 9-channel UNet, inpaint=False its 4-channel one (the blend)."""
        from . import config as _config
        cfg = _config.CONFIGS[cfg]() if isinstance(cfg, str) else cfg
        from . import synthetic
        if inpaint and cfg.unet.in_channels == cfg.unet.out_channels:
            cfg = inpaint_variant(cfg)
        usd = synthetic.make_unet_weights(cfg, seed, device=weights_device, **kw)
        vsd = synthetic.make_vae_weights(cfg, seed + 1, device=weights_device, with_encoder=True, **kw)    # vae.encode runs every call
        pipe = cls(cfg, usd, vsd, device=device, workspace_bytes=workspace_bytes, scheduler=scheduler)
        if keep_weights:
            pipe.synthetic_weights = (usd, vsd)
        return pipe

    def save_pretrained(self, save_directory: str):
        super().save_pretrained(save_directory)
        mi = os.path.join(save_directory, "model_index.json")
        with open(mi) as f:
            mj = json.load(f)
        mj["_class_name"] = "StableDiffusionInpaintPipeline"
        with open(mi, "w") as f:
            json.dump(mj, f, indent=2)

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, image=None, mask_image=None, height: Optional[int] = None,
                 width: Optional[int] = None, strength: float = 1.0, num_inference_steps: int = 50, guidance_scale: float = 7.5,
                 negative_prompt=None, num_images_per_prompt: int = 1, generator: Optional[torch.Generator] = None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil",
                 noise_enc_image: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                 noise_enc_masked: Optional[torch.Tensor] = None, cross_attention_kwargs: Optional[dict] = None,
                 guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 max_embeddings_multiples: Optional[int] = None, editing_prompt=None, editing_prompt_embeddings=None, sem_guidance=None):
        """image / mask_image as `prepare_mask_and_image` takes them.  Noise draws come from a CPU generator in diffusers' order, or are
        passed explicitly (noise_enc_image [N,4,L,L], noise (or latents) [B,4,L,L], noise_enc_masked [N,4,L,L]; N distinct images)."""
        refuse_pag("StableDiffusionInpaintPipeline", pag_scale, pag_adaptive_scale)
        refuse_sega("StableDiffusionInpaintPipeline", editing_prompt, editing_prompt_embeddings, sem_guidance)
        refuse_deepcache("StableDiffusionInpaintPipeline", getattr(self, "_deepcache", None))
        refuse_long_prompt("StableDiffusionInpaintPipeline", max_embeddings_multiples, prompt_embeds)
        if image is None or mask_image is None:
            raise ValueError("StableDiffusionInpaintPipeline needs image= and mask_image=")
        check_guidance_rescale(guidance_rescale)
        side = self.cfg.default_sample_size * self.vae_scale_factor
        height, width = height or side, width or side
        check_image_size(height, width)
        flavour = check_request(self.cfg, self.scheduler, strength, num_inference_steps)
        Lh, Lw = height // self.vae_scale_factor, width // self.vae_scale_factor
        self._refuse_rectangular_hook(Lh, Lw)
        self._apply_lora_scale(cross_attention_kwargs)
        L = Lh if Lh == Lw else (Lh, Lw)                       # the square path passes one side, exactly as before
        img, mask = prepare_mask_and_image(image, mask_image, height, width)
        prompt_embeds, pb, per = self._expand_prompts(prompt, negative_prompt, num_images_per_prompt, prompt_embeds)
        B = prompt_embeds.shape[0] // 2
        n = img.shape[0]
        if n != 1 and n != pb:
            raise ValueError(f"image batch size {n} must be 1 or equal the prompt batch size {pb}")
        rep = B if n == 1 else per
        need_image = flavour == "blend" or strength < 1.0
        need_masked = flavour == "concat"
        Cl = self.cfg.unet.out_channels
        if noise is None and latents is not None:
            noise = latents                                       # diffusers: `noise = latents`
        ne, nz, me = draw_noises(generator, n, B, Cl, L, need_image, need_masked, noise_enc_image, noise, noise_enc_masked)
        if tuple(nz.shape) != (B, Cl, Lh, Lw):
            raise ValueError(f"Unexpected noise shape, got {tuple(nz.shape)}, expected {(B, Cl, Lh, Lw)}")
        for t_, nm in ((ne, "noise_enc_image"), (me, "noise_enc_masked")):
            if t_ is not None and tuple(t_.shape) != (n, Cl, Lh, Lw):
                raise ValueError(f"Unexpected {nm} shape, got {tuple(t_.shape)}, expected {(n, Cl, Lh, Lw)}")
        eng = self.engine
        x, mask_lat = eng.inpaint_prepare(img, mask, need_image, need_masked)
        mean, logvar = eng.vae_encode(x)                          # image rows, then masked-image rows: one encoder pass
        sf = self.cfg.vae.scaling_factor
        dev = mean.device
        post = lambda k, e: (mean[k * n:(k + 1) * n] + torch.exp(0.5 * logvar[k * n:(k + 1) * n]) * e.to(dev, torch.float32)) * sf
        image_lat = post(0, ne).repeat_interleave(rep, 0).contiguous() if need_image else None
        masked_lat = post(int(need_image), me).repeat_interleave(rep, 0).contiguous() if need_masked else None
        mask_lat = mask_lat.repeat_interleave(rep, 0).contiguous()
        nz = eng._h2d(nz).clone()
        if strength < 1.0:
            sched = self.scheduler
            ts = sched.set_timesteps(num_inference_steps)
            a_t, a_p = sched.step_coeffs()
            t0 = strength_start(num_inference_steps, strength)
            a = float(sched.alphas_cumprod[int(ts[t0])])
            lat = (a ** 0.5 * image_lat + (1 - a) ** 0.5 * nz).contiguous()      # [upstream-knowledge] scheduler.add_noise
        else:
            lat = (nz * self.scheduler.init_noise_sigma).contiguous()
        try:
            if flavour == "concat":
                eng.inpaint_set(mask_lat, masked_lat)
            else:
                eng.inpaint_set(mask_lat, image_lat, nz)
                eng.inpaint_set_schedule(blend_schedule(self.scheduler, evaluation_timesteps(self.scheduler, num_inference_steps, strength)))
            self._begin_recording(prompt_embeds, B, L)
            with self._guidance_rescaled(guidance_rescale):
                if strength < 1.0:
                    eng.denoise(lat, ts[t0:], a_t[t0:], a_p[t0:], guidance_scale)
                else:
                    self._denoise(lat, num_inference_steps, guidance_scale)
        finally:
            eng.inpaint_clear()
        self._inpaint_inputs = {"mask": mask_lat, "image_latents": image_lat, "masked_image_latents": masked_lat, "noise": nz}
        if output_type == "latent":
            return PipelineOutput(images=[], latents=lat)
        return self._finish(lat, B, output_type)

    def img2img(self, *a, **kw):
        raise NotImplementedError("StableDiffusionInpaintPipeline runs inpainting only (call the pipeline with image= and mask_image=)")
