"""`pipeline.safety_checker` on the device: diffusers' StableDiffusionSafetyChecker behind the checkpoints the reference generates
with (reference finetune_sd_token.py:164-187 saves it; data_generation.py:59-62 skips the seeds it blacks out).

The CLIPImageProcessor front end, the CLIP ViT vision tower, `visual_projection` and the cosines against the concept embeddings
run in `agd_safety_scores`; the per-image decision runs here on the host in float64 on one copy of at most B x 20 cosines, in the
order diffusers 0.21 `StableDiffusionSafetyChecker.forward` applies it.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np
import torch

from . import _lib
from .config import SafetyConfig


def vision_config(s: SafetyConfig) -> _lib.AgdVisionConfig:
    if s.hidden_act not in ("quick_gelu", "gelu"):
        raise ValueError(f"safety checker hidden_act '{s.hidden_act}' is not supported (quick_gelu, gelu)")
    if s.num_channels != 3:
        raise ValueError(f"safety checker num_channels {s.num_channels} is not supported (3)")
    if s.size != s.crop_size or s.crop_size != s.image_size or s.resample != 3 or abs(s.rescale_factor - 1 / 255) > 1e-12:
        raise ValueError("safety checker preprocessing must be BICUBIC resize to image_size, identity crop, rescale 1/255")
    v = _lib.AgdVisionConfig()
    v.struct_size = C.sizeof(_lib.AgdVisionConfig)
    v.hidden, v.layers, v.heads, v.intermediate = s.hidden_size, s.num_hidden_layers, s.num_attention_heads, s.intermediate_size
    v.image_size, v.patch_size, v.projection_dim = s.image_size, s.patch_size, s.projection_dim
    v.n_special, v.n_concepts = s.n_special, s.n_concepts
    v.act = 0 if s.hidden_act == "quick_gelu" else 1
    v.eps = s.layer_norm_eps
    for i in range(3):
        v.mean[i], v.std[i] = s.image_mean[i], s.image_std[i]
    return v


def nsfw_flags(special_cos: np.ndarray, cos: np.ndarray, special_w: Sequence[float], concept_w: Sequence[float]) -> List[bool]:
    """StableDiffusionSafetyChecker.forward's decision per image: the special-care scores round(cos - w + adjustment, 3) come first,
    and each one above 0 sets adjustment = 0.01 for every score after it; the image is flagged when a concept score
    round(cos - w + adjustment, 3) is above 0.  The reference computes the scores as a float32 cosine minus a Python float, which
    NumPy 1.x evaluates in float64, then applies np.round; the same is done here explicitly in float64."""
    special_cos = np.asarray(special_cos, dtype=np.float32)
    cos = np.asarray(cos, dtype=np.float32)
    sw = [float(np.float32(w)) for w in special_w]
    cw = [float(np.float32(w)) for w in concept_w]
    flags = []
    for i in range(cos.shape[0]):
        adjustment = 0.0
        for j in range(special_cos.shape[1]):
            if np.round(np.float64(special_cos[i, j]) - sw[j] + adjustment, 3) > 0:
                adjustment = 0.01
        flags.append(any(np.round(np.float64(cos[i, k]) - cw[k] + adjustment, 3) > 0 for k in range(cos.shape[1])))
    return flags


class HipSafetyChecker:
    """Callable `u8 images [B,S,S,3] -> B flags`, the contract of the pipeline's `safety_checker` slot."""

    def __init__(self, engine, cfg: SafetyConfig, special_weights, concept_weights):
        self.engine = engine
        self.cfg = cfg
        self.special_weights = np.asarray(torch.as_tensor(special_weights).detach().float().cpu(), dtype=np.float32)
        self.concept_weights = np.asarray(torch.as_tensor(concept_weights).detach().float().cpu(), dtype=np.float32)
        if self.special_weights.shape != (cfg.n_special,) or self.concept_weights.shape != (cfg.n_concepts,):
            raise ValueError(f"safety checker thresholds {self.special_weights.shape} / {self.concept_weights.shape} do not match "
                             f"{cfg.n_special} special / {cfg.n_concepts} concepts")

    def scores(self, images_u8: torch.Tensor, pixels: bool = False):
        """Cosines fp32 [B, n_special + n_concepts] (device; special-care first); with `pixels` also the processor's pixel_values
        [B, 3, image_size, image_size]."""
        return self.engine.safety_scores(images_u8, want_pixels=pixels)

    def __call__(self, images_u8: torch.Tensor) -> List[bool]:
        cos = self.scores(images_u8).cpu().numpy()
        ns = self.cfg.n_special
        return nsfw_flags(cos[:, :ns], cos[:, ns:], self.special_weights, self.concept_weights)
