"""ControlNet-conditioned txt2img: diffusers' `ControlNetModel` + `StableDiffusionControlNetPipeline` (0.21.2 semantics) over the
device engine.

The ControlNet runs inside every fused denoise loop (`agd_denoise`, `agd_denoise_plms`, `agd_denoise_dpm`): after the UNet's mid block
its down and mid blocks run on the same latents, timestep and prompt embeddings, and its scaled residuals are added to the UNet's skip
connections and mid output.  Its conditioning embedding depends on the control image alone and is computed once per call.  DAAM and the
hook.py hooker see the UNet's cross-attention only.  Rules restated from the published pipeline are marked [upstream-knowledge].
Not implemented, and refused: guess mode, several ControlNets (MultiControlNet), ControlNet img2img / inpainting (StableDiffusionInpaintPipeline
runs inpainting without a ControlNet).
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from .config import ControlNetConfig, SDConfig, controlnet_config_from_json, controlnet_keep_schedule
from .pipeline import PipelineOutput, StableDiffusionPipeline, refuse_deepcache, refuse_long_prompt, refuse_pag, refuse_sega
from .scheduler import DPMSolverMultistepScheduler, PNDMScheduler

_WEIGHTS = "diffusion_pytorch_model.safetensors"


class ControlNetModel:
    """Holder of a ControlNet's diffusers `config.json` and state dict (`ControlNetModel.from_pretrained(dir)`); the pipeline loads it
    onto the device."""

    def __init__(self, config: dict, state_dict: Dict[str, torch.Tensor]):
        self.config = dict(config)
        self.state_dict = state_dict

    @classmethod
    def from_pretrained(cls, path: str) -> "ControlNetModel":
        from safetensors.torch import load_file
        with open(os.path.join(path, "config.json")) as f:
            cj = json.load(f)
        for fn in (_WEIGHTS, "model.safetensors"):
            p = os.path.join(path, fn)
            if os.path.exists(p):
                return cls(cj, load_file(p))
        raise FileNotFoundError(f"no safetensors weights under {path}")

    @classmethod
    def from_config(cls, unet_cfg, cncfg: ControlNetConfig, state_dict: Dict[str, torch.Tensor]) -> "ControlNetModel":
        return cls(cncfg.to_json(unet_cfg), state_dict)

    def save_pretrained(self, path: str):
        from safetensors.torch import save_file
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(self.config, f, indent=2)
        save_file({k: v.detach().contiguous() for k, v in self.state_dict.items()}, os.path.join(path, _WEIGHTS))


def prepare_control_image(image, height: int, width: int) -> torch.Tensor:
    """The control image as fp32 [B,3,H,W] in [0,1]: diffusers `VaeImageProcessor(do_convert_rgb=True, do_normalize=False).preprocess`
    [upstream-knowledge] for a PIL image or a list of them (RGB, LANCZOS resize to width x height, / 255); a uint8 [B,H,W,3] tensor
    (/ 255) or a float [B,3,H,W] tensor is taken as it is and must already have the output size."""
    from PIL import Image
    if isinstance(image, Image.Image):
        image = [image]
    if isinstance(image, (list, tuple)):
        if not image or not all(isinstance(im, Image.Image) for im in image):
            raise ValueError("image: a PIL image, a list of PIL images, a uint8 [B,H,W,3] or a float [B,3,H,W] tensor")
        arr = [np.asarray(im.convert("RGB").resize((width, height), resample=Image.LANCZOS)).astype(np.float32) / 255.0 for im in image]
        return torch.from_numpy(np.stack(arr)).permute(0, 3, 1, 2).contiguous()
    if not torch.is_tensor(image) or image.ndim != 4:
        raise ValueError("image: a PIL image, a list of PIL images, a uint8 [B,H,W,3] or a float [B,3,H,W] tensor")
    if image.dtype == torch.uint8:
        if image.shape[3] != 3:
            raise ValueError(f"uint8 control images are [B,H,W,3], got {tuple(image.shape)}")
        image = image.permute(0, 3, 1, 2).float() / 255.0
    elif image.shape[1] != 3:
        raise ValueError(f"float control images are [B,3,H,W], got {tuple(image.shape)}")
    if tuple(image.shape[2:]) != (height, width):
        raise ValueError(f"control image is {image.shape[2]}x{image.shape[3]}, the output {height}x{width}: tensors must already have "
                         "the output size (PIL images are resized)")
    return image.detach().to(torch.float32).contiguous()


def expand_control_image(image: torch.Tensor, prompt_batch: int, num_images_per_prompt: int) -> torch.Tensor:
    """[upstream-knowledge] `prepare_image`: an image batch of 1 is repeated for every image of the call, else it must match the prompt
    batch and is repeated `num_images_per_prompt` times (repeat_interleave)."""
    n = image.shape[0]
    if n != 1 and n != prompt_batch:
        raise ValueError(f"image batch size {n} must be 1 or equal the prompt batch size {prompt_batch}")
    return image.repeat_interleave(prompt_batch * num_images_per_prompt if n == 1 else num_images_per_prompt, dim=0)


def evaluation_count(scheduler, num_inference_steps: int) -> int:
    """Model evaluations of one loop: PNDM (PLMS) evaluates its second timestep twice (steps + 1), DDIM and DPM-Solver++ once per step."""
    scheduler.set_timesteps(num_inference_steps)
    if isinstance(scheduler, PNDMScheduler):
        return len(scheduler.plms_program()[0])
    if isinstance(scheduler, DPMSolverMultistepScheduler):
        return len(scheduler.dpm_program()[0])
    return len(scheduler.timesteps)


class StableDiffusionControlNetPipeline(StableDiffusionPipeline):
    """`StableDiffusionControlNetPipeline(..., controlnet=ControlNetModel)`: `pipe(prompt, image, ...)` with
    `controlnet_conditioning_scale`, `control_guidance_start` / `control_guidance_end`; everything else is StableDiffusionPipeline's."""

    def __init__(self, cfg: SDConfig, unet_sd, vae_sd, controlnet: ControlNetModel = None, **kw):
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("several ControlNets (MultiControlNetModel) are not implemented")
        if not isinstance(controlnet, ControlNetModel):
            raise ValueError("StableDiffusionControlNetPipeline needs controlnet=ControlNetModel(...)")
        self.controlnet = controlnet
        self.cn_cfg = controlnet_config_from_json(controlnet.config, cfg.unet)
        self._cn_pending = None
        super().__init__(cfg, unet_sd, vae_sd, **kw)

    def _load_extra(self):
        self.engine.controlnet_configure(self.cn_cfg)
        self.engine.load_state_dict(self.controlnet.state_dict, "controlnet.")

    # ---- construction -------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, cfg: Union[str, SDConfig] = "sd15", seed: int = 1234, device=0, workspace_bytes: int = 0,
                       weights_device: str = "cpu", keep_weights: bool = False, scheduler: str = "DDIMScheduler", controlnet=True, **kw):
        """Random UNet / VAE / ControlNet weights (controlnet=True; or a ControlNetModel to use as given)."""
        from . import config as _config, synthetic
        cfg = _config.CONFIGS[cfg]() if isinstance(cfg, str) else cfg
        usd = synthetic.make_unet_weights(cfg, seed, device=weights_device, **kw)
        vsd = synthetic.make_vae_weights(cfg, seed + 1, device=weights_device, **kw)
        if controlnet is True:
            cncfg = ControlNetConfig()
            controlnet = ControlNetModel.from_config(cfg.unet, cncfg, synthetic.make_controlnet_weights(cfg, cncfg, seed + 2, device=weights_device, **kw))
        pipe = cls(cfg, usd, vsd, controlnet=controlnet, device=device, workspace_bytes=workspace_bytes, scheduler=scheduler)
        if keep_weights:
            pipe.synthetic_weights = (usd, vsd)
        return pipe

    @classmethod
    def from_pretrained(cls, path: str, controlnet: Optional[ControlNetModel] = None, **kw):
        """`from_pretrained(path, controlnet=ControlNetModel.from_pretrained(dir))`, or a checkpoint whose model_index.json names
        `"controlnet": ["diffusers", "ControlNetModel"]` (its `controlnet/` directory is loaded)."""
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("several ControlNets (MultiControlNetModel) are not implemented")
        if controlnet is None:
            mi = os.path.join(path, "model_index.json")
            entry = None
            if os.path.exists(mi):
                with open(mi) as f:
                    entry = json.load(f).get("controlnet")
            if isinstance(entry, (list, tuple)) and len(entry) == 2 and isinstance(entry[0], (list, tuple)):
                raise NotImplementedError("several ControlNets (MultiControlNetModel) are not implemented")
            if not (isinstance(entry, (list, tuple)) and len(entry) == 2 and entry[1] == "ControlNetModel"):
                raise ValueError(f"{path}: model_index.json names no ControlNetModel; pass controlnet=ControlNetModel.from_pretrained(dir)")
            controlnet = ControlNetModel.from_pretrained(os.path.join(path, "controlnet"))
        return super().from_pretrained(path, controlnet=controlnet, **kw)

    def save_pretrained(self, save_directory: str):
        """StableDiffusionPipeline.save_pretrained plus `controlnet/` and its model_index.json entry."""
        super().save_pretrained(save_directory)
        self.controlnet.save_pretrained(os.path.join(save_directory, "controlnet"))
        mi = os.path.join(save_directory, "model_index.json")
        with open(mi) as f:
            mj = json.load(f)
        mj["_class_name"] = "StableDiffusionControlNetPipeline"
        mj["controlnet"] = ["diffusers", "ControlNetModel"]
        with open(mi, "w") as f:
            json.dump(mj, f, indent=2)

    # ---- txt2img ------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt: Union[str, List[str], None] = None, image=None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 50, guidance_scale: float = 7.5, negative_prompt=None, generator=None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil",
                 num_images_per_prompt: int = 1, controlnet_conditioning_scale: float = 1.0, guess_mode: bool = False,
                 control_guidance_start: float = 0.0, control_guidance_end: float = 1.0, cross_attention_kwargs: Optional[dict] = None,
                 guidance_rescale: float = 0.0, pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0,
                 max_embeddings_multiples: Optional[int] = None, editing_prompt=None, editing_prompt_embeddings=None, sem_guidance=None):
        refuse_pag("StableDiffusionControlNetPipeline", pag_scale, pag_adaptive_scale)
        refuse_sega("StableDiffusionControlNetPipeline", editing_prompt, editing_prompt_embeddings, sem_guidance)
        refuse_deepcache("StableDiffusionControlNetPipeline", getattr(self, "_deepcache", None))
        refuse_long_prompt("StableDiffusionControlNetPipeline", max_embeddings_multiples, prompt_embeds)
        if guess_mode:
            raise NotImplementedError("ControlNet guess_mode is not implemented")
        if isinstance(controlnet_conditioning_scale, (list, tuple)) or isinstance(control_guidance_start, (list, tuple)) \
                or isinstance(control_guidance_end, (list, tuple)):
            raise NotImplementedError("per-ControlNet lists (MultiControlNetModel) are not implemented")
        if image is None:
            raise ValueError("StableDiffusionControlNetPipeline needs a control image (image=...)")
        keep = controlnet_keep_schedule(1, control_guidance_start, control_guidance_end)   # (validates the window)
        del keep
        side = self.cfg.default_sample_size * self.vae_scale_factor
        height, width = height or side, width or side
        cond = prepare_control_image(image, height, width)
        if prompt_embeds is not None:
            prompt_batch, per = prompt_embeds.shape[0] // 2, 1
        else:
            prompt_batch, per = (1 if isinstance(prompt, str) else len(prompt)), num_images_per_prompt
        cond = expand_control_image(cond, prompt_batch, per)
        self._cn_pending = (cond, float(controlnet_conditioning_scale), float(control_guidance_start), float(control_guidance_end))
        try:
            return super().__call__(prompt, height=height, width=width, num_inference_steps=num_inference_steps,
                                    guidance_scale=guidance_scale, negative_prompt=negative_prompt, generator=generator, latents=latents,
                                    prompt_embeds=prompt_embeds, output_type=output_type, num_images_per_prompt=num_images_per_prompt,
                                    cross_attention_kwargs=cross_attention_kwargs, guidance_rescale=guidance_rescale)
        finally:
            self._cn_pending = None
            self.engine.controlnet_set_schedule([])

    def controlnet_scales(self, num_inference_steps: int, scale: float, start: float, end: float) -> List[float]:
        """Per model evaluation: `controlnet_conditioning_scale * controlnet_keep[i]` [upstream-knowledge]."""
        n = evaluation_count(self.scheduler, num_inference_steps)
        return [scale * k for k in controlnet_keep_schedule(n, start, end)]

    def _denoise(self, lat, num_inference_steps, guidance_scale):
        if self._cn_pending is None:
            raise RuntimeError("the ControlNet pipeline's loop runs from __call__ (it needs the control image)")
        cond, scale, start, end = self._cn_pending
        if cond.shape[0] != lat.shape[0]:
            raise ValueError(f"control image batch {cond.shape[0]} != latents batch {lat.shape[0]}")
        self.engine.controlnet_set_cond(cond, repeat=2)          # the CFG doubling: [cond; cond]
        self.engine.controlnet_set_schedule(self.controlnet_scales(num_inference_steps, scale, start, end))
        super()._denoise(lat, num_inference_steps, guidance_scale)

    def img2img(self, *a, **kw):
        raise NotImplementedError("ControlNet img2img is not implemented (StableDiffusionControlNetImg2ImgPipeline)")
