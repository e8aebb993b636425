"""InstructPix2Pix: diffusers' `StableDiffusionInstructPix2PixPipeline` (0.21.2 semantics) over the device engine.

An 8-channel UNet reads latents | image latents.  The image goes through the front end and the VAE encoder once per call
(`agd_ip2p_prepare_hw`: the posterior's mean, not multiplied by the scaling factor), the latents start as pure noise at the image's size
and the whole schedule runs.  Every evaluation of the fused loops then runs three guidance branches -- text (prompt, image latents),
image (negative prompt, image latents), uncond (negative prompt, zero image latents) -- and combines them on the device as
    e = e_uncond + guidance_scale (e_text - e_image) + image_guidance_scale (e_image - e_uncond)
before the scheduler's own step kernel (ip2p.hip, model.hip run_ip2p_loop).  DAAM and the hook.py hooker see the text branch only.
Rules restated from the published pipeline are marked [upstream-knowledge].  Deliberate differences:
 * guidance_scale <= 1 or image_guidance_scale < 1 is refused: 0.21.2 then silently drops guidance altogether, and that mode is not built;
 * images are not resized: height and width are the image's and each must be a multiple of 64;
 * an image batch of 1 serves every row, else it pairs with the prompts (repeat_interleave over num_images_per_prompt), as the
   ControlNet and inpainting pipelines do.
Refused: UNets of other widths (4-channel txt2img, 9-channel inpainting), img2img, ControlNet.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from .config import SDConfig, ip2p_variant
from .pipeline import PipelineOutput, StableDiffusionPipeline, check_image_size, refuse_deepcache, refuse_long_prompt, refuse_pag, refuse_sega


def check_unet(cfg: SDConfig) -> None:
    """[upstream-knowledge] latent channels + image-latent channels must equal the UNet's in_channels."""
    u = cfg.unet
    want = u.out_channels + cfg.vae.latent_channels
    if u.in_channels != want:
        raise ValueError(f"InstructPix2Pix needs a UNet of {want} input channels ({u.out_channels} latent + {cfg.vae.latent_channels} "
                         f"image-latent channels), this one takes {u.in_channels}")


def check_guidance(guidance_scale: float, image_guidance_scale: float) -> None:
    if not guidance_scale > 1.0 or not image_guidance_scale >= 1.0:
        raise ValueError(f"guidance_scale must be > 1 and image_guidance_scale >= 1 (got guidance_scale={guidance_scale}, "
                         f"image_guidance_scale={image_guidance_scale}): the no-guidance mode is not implemented")


def prepare_image(image) -> torch.Tensor:
    """[upstream-knowledge] `VaeImageProcessor.preprocess` up to the point the device front end takes over.  image: PIL image(s) (RGB)
    or a uint8 [B,H,W,3] tensor -> uint8 [B,H,W,3] (x / 255 then 2 x - 1 on the device), or a float [B,3,H,W] tensor already in [-1,1].
    Returns the tensor; its height and width must each be a multiple of 64 (nothing is resized)."""
    from PIL import Image
    if isinstance(image, Image.Image):
        image = [image]
    if isinstance(image, (list, tuple)) and image and all(isinstance(i, Image.Image) for i in image):
        sizes = {i.size for i in image}
        if len(sizes) != 1:
            raise ValueError(f"the images must share one size, got {sorted(sizes)}")
        img = torch.from_numpy(np.stack([np.asarray(i.convert("RGB")) for i in image]))
    elif isinstance(image, np.ndarray) and image.ndim == 4:
        img = torch.from_numpy(image)
    elif torch.is_tensor(image) and image.ndim == 4:
        img = image
    else:
        raise ValueError("image: a PIL image, a list of PIL images, a uint8 [B,H,W,3] or a float [B,3,H,W] tensor")
    if img.dtype == torch.uint8:
        if img.shape[3] != 3:
            raise ValueError(f"uint8 images are [B,H,W,3], got {tuple(img.shape)}")
        h, w = int(img.shape[1]), int(img.shape[2])
    else:
        if img.shape[1] != 3:
            raise ValueError(f"float images are [B,3,H,W] in [-1,1], got {tuple(img.shape)}")
        img = img.to(torch.float32)
        h, w = int(img.shape[2]), int(img.shape[3])
    check_image_size(h, w)
    return img.contiguous()


class StableDiffusionInstructPix2PixPipeline(StableDiffusionPipeline):
    """`StableDiffusionInstructPix2PixPipeline`: `pipe(prompt, image, ...)`; everything else is StableDiffusionPipeline's."""

    def __init__(self, cfg: SDConfig, unet_sd, vae_sd, **kw):
        if "controlnet" in kw:
            raise NotImplementedError("ControlNet with InstructPix2Pix is not implemented")
        check_unet(cfg)
        super().__init__(cfg, unet_sd, vae_sd, **kw)

    @classmethod
    def from_synthetic(cls, cfg: Union[str, SDConfig] = "sd15", seed: int = 1234, device=0, workspace_bytes: int = 0,
                       weights_device: str = "cpu", keep_weights: bool = False, scheduler: str = "DDIMScheduler", ip2p: bool = True, **kw):
        """Random weights; ip2p=True gives the preset's 8-channel UNet (ip2p=False keeps the preset's own width, which is then refused
        unless it already has 8 channels)."""
        from . import config as _config
        cfg = _config.CONFIGS[cfg]() if isinstance(cfg, str) else cfg
        from . import synthetic
        if ip2p and cfg.unet.in_channels == cfg.unet.out_channels:
            cfg = ip2p_variant(cfg)
        check_unet(cfg)
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
        mj["_class_name"] = "StableDiffusionInstructPix2PixPipeline"
        with open(mi, "w") as f:
            json.dump(mj, f, indent=2)

    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, image=None, num_inference_steps: int = 100, guidance_scale: float = 7.5,
                 image_guidance_scale: float = 1.5, negative_prompt=None, num_images_per_prompt: int = 1,
                 generator: Union[torch.Generator, Sequence[torch.Generator], None] = None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil", cross_attention_kwargs: Optional[dict] = None,
                 height: Optional[int] = None, width: Optional[int] = None, guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 max_embeddings_multiples: Optional[int] = None, editing_prompt=None, editing_prompt_embeddings=None, sem_guidance=None):
        """image as `prepare_image` takes it; height and width are the image's (given ones must equal them: nothing is resized).
        prompt_embeds is [2B,T,D] = [uncond | cond]."""
        refuse_pag("StableDiffusionInstructPix2PixPipeline", pag_scale, pag_adaptive_scale)
        refuse_sega("StableDiffusionInstructPix2PixPipeline", editing_prompt, editing_prompt_embeddings, sem_guidance)
        refuse_deepcache("StableDiffusionInstructPix2PixPipeline", getattr(self, "_deepcache", None))
        refuse_long_prompt("StableDiffusionInstructPix2PixPipeline", max_embeddings_multiples, prompt_embeds)
        if image is None:
            raise ValueError("StableDiffusionInstructPix2PixPipeline needs image=")
        if guidance_rescale:
            raise ValueError(f"guidance_rescale={guidance_rescale!r}: guidance rescale is not implemented for the InstructPix2Pix pipeline "
                             "(its three-branch loop has no text-branch spread to rescale to); leave it 0")
        check_unet(self.cfg)
        check_guidance(guidance_scale, image_guidance_scale)
        img = prepare_image(image)
        h0, w0 = height, width
        height, width = (int(img.shape[1]), int(img.shape[2])) if img.dtype == torch.uint8 else (int(img.shape[2]), int(img.shape[3]))
        if (h0 is not None and h0 != height) or (w0 is not None and w0 != width):
            raise ValueError(f"height={h0}, width={w0} given for a {height} x {width} image (inputs are not resized)")
        Lh, Lw = height // self.vae_scale_factor, width // self.vae_scale_factor
        self._refuse_rectangular_hook(Lh, Lw)
        self._apply_lora_scale(cross_attention_kwargs)
        L = Lh if Lh == Lw else (Lh, Lw)
        prompt_embeds, pb, per = self._expand_prompts(prompt, negative_prompt, num_images_per_prompt, prompt_embeds)
        B = prompt_embeds.shape[0] // 2
        n = img.shape[0]
        if n != 1 and n != pb:
            raise ValueError(f"image batch size {n} must be 1 or equal the prompt batch size {pb}")
        rep = B if n == 1 else per
        lat = self._draw_latents(B, Lh, Lw, generator, latents)
        eng = self.engine
        image_lat = eng.ip2p_prepare(img).repeat_interleave(rep, 0).contiguous()
        try:
            eng.ip2p_set(image_lat, image_guidance_scale)
            self._begin_recording(prompt_embeds, B, L)
            self._denoise(lat, num_inference_steps, guidance_scale)
        finally:
            eng.ip2p_clear()
        self._ip2p_inputs = {"image_latents": image_lat}
        if output_type == "latent":
            return PipelineOutput(images=[], latents=lat)
        return self._finish(lat, B, output_type)

    def img2img(self, *a, **kw):
        raise NotImplementedError("StableDiffusionInstructPix2PixPipeline runs instruction edits only (call the pipeline with image=)")
