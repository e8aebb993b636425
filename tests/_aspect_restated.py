"""Rectangular (height != width) restatements for the aspect-ratio tests.

`AspectDaamRecorder` is the fp32 oracle's `DaamRecorder` with the latent size given per axis: a call of N query tokens has daam's
factor f = sqrt(Lh * Lw / N), its conditional-half maps are viewed as (Lh / f) x (Lw / f), and the global map resizes every
(layer, head) accumulator with torch bicubic to (Lh, Lw) (separate y and x scales), clamps at 0 and takes the mean.  daam itself
unravels h = w = sqrt(N); on square latents this class is exactly `oracle.sd_oracle.DaamRecorder` (tests/test_aspect_cpu.py pins
that), on rectangular ones it is the direct generalisation of daam's own factor formula (parity-unpinned).

`inpaint_mask_latents` restates the mask step of the inpainting front end for an H x W mask: binarise at 0.5, then the nearest
resize to (H / 8, W / 8) (latent pixel (i, j) = mask pixel (8 i, 8 j)).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F


class AspectDaamRecorder:
    def __init__(self, latent_hw: Tuple[int, int], context_size: int = 77):
        self.lh, self.lw = int(latent_hw[0]), int(latent_hw[1])
        self.context_size = context_size
        self.acc: Dict[Tuple[int, str, int], torch.Tensor] = {}   # (factor, layer, head) -> [B', T, h, w]

    def __call__(self, p: torch.Tensor, heads: int, layer: str = ""):
        bh, n, t = p.shape
        if "mid_block" in layer:
            return
        factor = int(math.sqrt((self.lh * self.lw) // n))
        if t != self.context_size or factor == 8:
            return
        h, w = self.lh // factor, self.lw // factor
        assert h * w == n, (self.lh, self.lw, n, factor)
        cond = p[bh // 2:]
        b = cond.shape[0] // heads
        m = cond.reshape(b, heads, n, t).permute(1, 0, 3, 2).reshape(heads, b, t, h, w)
        for hd in range(heads):
            key = (factor, layer, hd)
            self.acc[key] = self.acc.get(key, 0) + m[hd]

    def compute_global_heat_map(self, n_rows: Optional[int] = None) -> torch.Tensor:
        """[B', T', Lh, Lw]"""
        if not self.acc:
            raise RuntimeError("No heat maps found.")
        ups = [F.interpolate(m, size=(self.lh, self.lw), mode="bicubic", align_corners=False).clamp_(min=0) for m in self.acc.values()]
        g = torch.stack(ups, 0).mean(0)
        return g if n_rows is None else g[:, :n_rows]


def latent_mask_hw(mask: torch.Tensor, f: int = 8) -> torch.Tensor:
    """binary mask [B, 1, H, W] -> [B, 1, H / f, W / f] (nearest: latent pixel (i, j) = mask pixel (f i, f j))."""
    return F.interpolate(mask, size=(mask.shape[2] // f, mask.shape[3] // f), mode="nearest")


def inpaint_mask_latents(mask: torch.Tensor, f: int = 8) -> torch.Tensor:
    """mask float [B, H, W] in [0, 1] -> binary [B, 1, H / f, W / f]."""
    return latent_mask_hw((mask >= 0.5).to(torch.float32)[:, None], f)


def clip_resize_crop_geometry(h: int, w: int, size: int) -> Tuple[int, int, int, int]:
    """transformers CLIPImageProcessor: shortest edge -> size, long edge -> int(size * long / short); then the size x size
    center crop at ((rh - size) // 2, (rw - size) // 2).  Returns (rh, rw, top, left)."""
    if h <= w:
        rh, rw = size, int(size * w / h)
    else:
        rh, rw = int(size * h / w), size
    return rh, rw, (rh - size) // 2, (rw - size) // 2
