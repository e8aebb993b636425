"""T2I-Adapter conditioned txt2img: diffusers' `T2IAdapter` ("full_adapter") + `StableDiffusionAdapterPipeline` (0.21.2 semantics) over the
device engine.

The adapter is a small convolutional network that runs ONCE per call on the conditioning image; its four feature maps do not depend on the
timestep.  Inside every fused denoise loop (`agd_denoise`, `agd_denoise_plms`, `agd_denoise_dpm`) feature i, times
`adapter_conditioning_scale`, is added to the output of UNet down block i: structural control at txt2img price.  DAAM and the hook.py
hooker record as in the plain pipeline (the adapter has no attention).  Rules restated from the published pipeline are marked
[upstream-knowledge].  One extension, named after the later diffusers argument: `adapter_conditioning_factor` adds the features on the
first int(factor * n) model evaluations only.  Not implemented, and refused: "light_adapter" / SDXL adapters, several adapters
(MultiAdapter), a list-valued scale, img2img.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from .config import AdapterConfig, SDConfig, adapter_config_for, adapter_config_from_json, adapter_schedule
from .controlnet import evaluation_count
from .pipeline import StableDiffusionPipeline, check_image_size, refuse_deepcache, refuse_long_prompt, refuse_pag, refuse_sega

_WEIGHTS = "diffusion_pytorch_model.safetensors"
_IMAGE_HELP = "image: a PIL image, a list of PIL images, a uint8 [B,H,W,C] or a float [B,C,H,W] tensor in [0,1]"


class T2IAdapter:
    """Holder of a T2I-Adapter's diffusers `config.json` and state dict (`T2IAdapter.from_pretrained(dir)`); the pipeline loads it onto
    the device."""

    def __init__(self, config: dict, state_dict: Dict[str, torch.Tensor]):
        self.config = dict(config)
        self.state_dict = state_dict

    @classmethod
    def from_pretrained(cls, path: str) -> "T2IAdapter":
        from safetensors.torch import load_file
        with open(os.path.join(path, "config.json")) as f:
            cj = json.load(f)
        for fn in (_WEIGHTS, "model.safetensors"):
            p = os.path.join(path, fn)
            if os.path.exists(p):
                return cls(cj, load_file(p))
        raise FileNotFoundError(f"no safetensors weights under {path}")

    @classmethod
    def from_config(cls, acfg: AdapterConfig, state_dict: Dict[str, torch.Tensor]) -> "T2IAdapter":
        return cls(acfg.to_json(), state_dict)

    def save_pretrained(self, path: str):
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.config, f, indent=2)
        save_file({k: v.detach().contiguous() for k, v in self.state_dict.items()}, os.path.join(path, _WEIGHTS))


def prepare_adapter_image(image, height: Optional[int], width: Optional[int], in_channels: int) -> torch.Tensor:
    """The conditioning image for the device front end [upstream-knowledge: `_preprocess_adapter_image`]: a PIL image or a list of them is
    resized to (width, height) with LANCZOS and becomes uint8 [B,H,W,C] -- "L"-mode images give C = 1, every other mode is taken as it
    is (RGB: 3); the device scales by 1 / 255 and there is no 2x - 1.  A uint8 [B,H,W,C] or a float [B,C,H,W] tensor in [0,1] is taken as
    given.  height / width None: the image's own size.  The channel count must be the adapter's, each side a multiple of 64."""
    from PIL import Image
    if isinstance(image, Image.Image):
        image = [image]
    if isinstance(image, (list, tuple)):
        if not image or not all(isinstance(im, Image.Image) for im in image):
            raise ValueError(_IMAGE_HELP)
        height, width = height or image[0].height, width or image[0].width
        check_image_size(height, width)
        arr = [np.asarray(im.resize((width, height), resample=Image.LANCZOS)) for im in image]
        arr = [a[:, :, None] if a.ndim == 2 else a for a in arr]
        if any(a.shape != arr[0].shape for a in arr):
            raise ValueError("image: the PIL images of one call must share a mode")
        out = torch.from_numpy(np.stack(arr).astype(np.uint8))
        c = out.shape[3]
    else:
        if not torch.is_tensor(image) or image.ndim != 4:
            raise ValueError(_IMAGE_HELP)
        if image.dtype == torch.uint8:
            h, w, c = image.shape[1], image.shape[2], image.shape[3]
            out = image.detach().contiguous()
        else:
            c, h, w = image.shape[1], image.shape[2], image.shape[3]
            out = image.detach().to(torch.float32).contiguous()
        height, width = height or h, width or w
        check_image_size(height, width)
        if (h, w) != (height, width):
            raise ValueError(f"adapter image is {h}x{w}, the output {height}x{width}: tensors must already have the output size "
                             "(PIL images are resized)")
    if c != in_channels:
        raise ValueError(f"adapter image has {c} channels, the adapter takes in_channels={in_channels}")
    return out


def expand_adapter_image(image: torch.Tensor, prompt_batch: int, num_images_per_prompt: int) -> torch.Tensor:
    """One image serves every image of the call (the engine reads feature image b % 1); else there is one per prompt, repeated
    `num_images_per_prompt` times like the prompts (repeat_interleave)."""
    n = image.shape[0]
    if n != 1 and n != prompt_batch:
        raise ValueError(f"image batch size {n} must be 1 or equal the prompt batch size {prompt_batch}")
    return image if n == 1 or num_images_per_prompt == 1 else image.repeat_interleave(num_images_per_prompt, dim=0)


class StableDiffusionAdapterPipeline(StableDiffusionPipeline):
    """`StableDiffusionAdapterPipeline(..., adapter=T2IAdapter)`: `pipe(prompt, image, ...)` with `adapter_conditioning_scale` and
    `adapter_conditioning_factor`; everything else is StableDiffusionPipeline's."""

    def __init__(self, cfg: SDConfig, unet_sd, vae_sd, adapter: T2IAdapter = None, **kw):
        if isinstance(adapter, (list, tuple)):
            raise NotImplementedError("several adapters (MultiAdapter) are not implemented")
        if not isinstance(adapter, T2IAdapter):
            raise ValueError("StableDiffusionAdapterPipeline needs adapter=T2IAdapter(...)")
        self.adapter = adapter
        self.adapter_cfg = adapter_config_from_json(adapter.config)
        self._ad_pending = None
        super().__init__(cfg, unet_sd, vae_sd, **kw)

    def _load_extra(self):
        self.engine.adapter_configure(self.adapter_cfg)
        self.engine.load_state_dict(self.adapter.state_dict, "adapter.")

    # ---- construction -------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, cfg: Union[str, SDConfig] = "sd15", seed: int = 1234, device=0, workspace_bytes: int = 0,
                       weights_device: str = "cpu", keep_weights: bool = False, scheduler: str = "DDIMScheduler", adapter=True, **kw):
        """Random UNet / VAE / adapter weights (adapter=True; or a T2IAdapter to use as given)."""
        from . import config as _config, synthetic
        cfg = _config.CONFIGS[cfg]() if isinstance(cfg, str) else cfg
        usd = synthetic.make_unet_weights(cfg, seed, device=weights_device, **kw)
        vsd = synthetic.make_vae_weights(cfg, seed + 1, device=weights_device, **kw)
        if adapter is True:
            acfg = adapter_config_for(cfg.unet)
            adapter = T2IAdapter.from_config(acfg, synthetic.make_adapter_weights(cfg, acfg, seed + 2, device=weights_device))
        pipe = cls(cfg, usd, vsd, adapter=adapter, device=device, workspace_bytes=workspace_bytes, scheduler=scheduler)
        if keep_weights:
            pipe.synthetic_weights = (usd, vsd)
        return pipe

    @classmethod
    def from_pretrained(cls, path: str, adapter: Optional[T2IAdapter] = None, **kw):
        """`from_pretrained(path, adapter=T2IAdapter.from_pretrained(dir))`, or a checkpoint whose model_index.json names
        `"adapter": ["diffusers", "T2IAdapter"]` (its `adapter/` directory is loaded)."""
        if isinstance(adapter, (list, tuple)):
            raise NotImplementedError("several adapters (MultiAdapter) are not implemented")
        if adapter is None:
            mi = os.path.join(path, "model_index.json")
            entry = None
            if os.path.exists(mi):
                with open(mi) as f:
                    entry = json.load(f).get("adapter")
            if isinstance(entry, (list, tuple)) and len(entry) == 2 and (isinstance(entry[0], (list, tuple)) or entry[1] == "MultiAdapter"):
                raise NotImplementedError("several adapters (MultiAdapter) are not implemented")
            if not (isinstance(entry, (list, tuple)) and len(entry) == 2 and entry[1] == "T2IAdapter"):
                raise ValueError(f"{path}: model_index.json names no T2IAdapter; pass adapter=T2IAdapter.from_pretrained(dir)")
            adapter = T2IAdapter.from_pretrained(os.path.join(path, "adapter"))
        return super().from_pretrained(path, adapter=adapter, **kw)

    def save_pretrained(self, save_directory: str):
        """StableDiffusionPipeline.save_pretrained plus `adapter/` and its model_index.json entry."""
        super().save_pretrained(save_directory)
        self.adapter.save_pretrained(os.path.join(save_directory, "adapter"))
        mi = os.path.join(save_directory, "model_index.json")
        with open(mi) as f:
            mj = json.load(f)
        mj["_class_name"] = "StableDiffusionAdapterPipeline"
        mj["adapter"] = ["diffusers", "T2IAdapter"]
        with open(mi, "w") as f:
            json.dump(mj, f, indent=2)

    # ---- txt2img ------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, image=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None, generator=None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil",
                 num_images_per_prompt: int = 1, adapter_conditioning_scale: float = 1.0, adapter_conditioning_factor: float = 1.0,
                 cross_attention_kwargs: Optional[dict] = None, guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 max_embeddings_multiples: Optional[int] = None, editing_prompt=None, editing_prompt_embeddings=None, sem_guidance=None):
        refuse_pag("StableDiffusionAdapterPipeline", pag_scale, pag_adaptive_scale)
        refuse_sega("StableDiffusionAdapterPipeline", editing_prompt, editing_prompt_embeddings, sem_guidance)
        refuse_deepcache("StableDiffusionAdapterPipeline", getattr(self, "_deepcache", None))
        refuse_long_prompt("StableDiffusionAdapterPipeline", max_embeddings_multiples, prompt_embeds)
        if isinstance(adapter_conditioning_scale, (list, tuple)):
            raise NotImplementedError("a list-valued adapter_conditioning_scale (MultiAdapter) is not implemented")
        if image is None:
            raise ValueError("StableDiffusionAdapterPipeline needs a conditioning image (image=...)")
        adapter_schedule(1, float(adapter_conditioning_scale), float(adapter_conditioning_factor))   # (validates the factor)
        cond = prepare_adapter_image(image, height, width, self.adapter_cfg.in_channels)
        if cond.dtype == torch.uint8:
            height, width = int(cond.shape[1]), int(cond.shape[2])
        else:
            height, width = int(cond.shape[2]), int(cond.shape[3])
        if prompt_embeds is not None:
            prompt_batch, per = prompt_embeds.shape[0] // 2, 1
        else:
            prompt_batch, per = (1 if isinstance(prompt, str) else len(prompt)), num_images_per_prompt
        cond = expand_adapter_image(cond, prompt_batch, per)
        self._ad_pending = (cond, float(adapter_conditioning_scale), float(adapter_conditioning_factor))
        try:
            return super().__call__(prompt, height=height, width=width, num_inference_steps=num_inference_steps,
                                    guidance_scale=guidance_scale, negative_prompt=negative_prompt, generator=generator, latents=latents,
                                    prompt_embeds=prompt_embeds, output_type=output_type, num_images_per_prompt=num_images_per_prompt,
                                    cross_attention_kwargs=cross_attention_kwargs, guidance_rescale=guidance_rescale)
        finally:
            self._ad_pending = None
            self.engine.adapter_set_schedule([])

    def adapter_scales(self, num_inference_steps: int, scale: float, factor: float) -> List[float]:
        """Per model evaluation: the scale on the first int(factor * n) evaluations, 0 after (config.adapter_schedule)."""
        return adapter_schedule(evaluation_count(self.scheduler, num_inference_steps), scale, factor)

    def _denoise(self, lat, num_inference_steps, guidance_scale):
        if self._ad_pending is None:
            raise RuntimeError("the adapter pipeline's loop runs from __call__ (it needs the conditioning image)")
        cond, scale, factor = self._ad_pending
        if cond.shape[0] not in (1, lat.shape[0]):
            raise ValueError(f"adapter image batch {cond.shape[0]} != latents batch {lat.shape[0]}")
        scales = self.adapter_scales(num_inference_steps, scale, factor)
        if any(s != 0.0 for s in scales):                        # (an all-zero schedule runs the plain UNet: the adapter is not run at all)
            self.engine.adapter_set_cond(cond)
        self.engine.adapter_set_schedule(scales)
        super()._denoise(lat, num_inference_steps, guidance_scale)

    def img2img(self, *a, **kw):
        raise NotImplementedError("T2I-Adapter img2img is not implemented")
