"""fp32 CPU restatement of region-based MultiDiffusion (Bar-Tal et al. 2023; the MultiDiffusion repository's `region_based.py`
[upstream-knowledge: written from its published source as the issue restates it; neither it nor diffusers is installed where the tests
run, and diffusers 0.21.2 has no such pipeline, so this is parity-unpinned]).

Row (region r, image p) is `r * B + p` everywhere.  `latent_masks` = threshold, `F.interpolate(mode="nearest")`, background
`max(0, 1 - sum)`; `spread` = step 1 of the loop; `masked_mean` = `sum_r m_r x_r / sum_r m_r` in ascending r
(`where(count > 0, value / count, value)`); `generate_regions` = the loop on the oracle's `unet_forward` / `DDIM` / `vae_decode` with one
recorder per region; `region_word_map` = this project's composed canvas map.  Unlike upstream every image of a batch is independent, the UNet
runs the whole latent (no views) and the scheduler is DDIM."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.nn.functional as F


def latent_masks(pixel_masks: Optional[torch.Tensor], batch: int, lh: int, lw: int) -> torch.Tensor:
    """pixel masks [R - 1, H, W] or [B, R - 1, H, W], uint8 (> 127), bool or float (> 0.5) -> fp32 [R, B, lh, lw]; None: R = 1."""
    if pixel_masks is None:
        return torch.ones(1, batch, lh, lw)
    m = pixel_masks
    if m.ndim == 3:
        m = m[None].expand(batch, *m.shape)
    assert m.shape[0] == batch
    fg = (m > 127) if m.dtype == torch.uint8 else (m.bool() if m.dtype == torch.bool else (m.float() > 0.5))
    fg = F.interpolate(fg.float(), size=(lh, lw), mode="nearest")        # [B, R - 1, lh, lw]: latent (y, x) reads pixel (8 y, 8 x)
    bg = (1.0 - fg.sum(1, keepdim=True)).clamp(min=0)
    return torch.cat([bg, fg], 1).transpose(0, 1).contiguous()


def boxes_to_masks(boxes, height: int, width: int) -> torch.Tensor:
    """normalised x0, y0, x1, y1 boxes [n][4] -> uint8 [n, H, W], set on [int(y0 H):int(y1 H), int(x0 W):int(x1 W)]"""
    out = torch.zeros(len(boxes), height, width, dtype=torch.uint8)
    for k, (x0, y0, x1, y1) in enumerate(boxes):
        out[k, int(y0 * height):int(y1 * height), int(x0 * width):int(x1 * width)] = 255
    return out


def spread(canvas: torch.Tensor, masks: torch.Tensor, noise: Optional[torch.Tensor] = None, backgrounds: Optional[torch.Tensor] = None,
           idx: Optional[Sequence[int]] = None, sa: float = 0.0, sb: float = 0.0) -> torch.Tensor:
    """canvas [B, C, h, w], masks [R, B, h, w] -> x [R * B, C, h, w].  idx None: every region is the canvas (a step at or past
    `bootstrapping`); else R - 1 indices into backgrounds [N, C, h, w] and, for r >= 1,
    x[r] = canvas m + (sa bg[idx[r - 1]] + sb noise) (1 - m)."""
    R, B = masks.shape[:2]
    out = []
    for r in range(R):
        if r == 0 or idx is None:
            out.append(canvas.clone())
            continue
        m = masks[r][:, None].to(canvas.dtype)
        bg = sa * backgrounds[int(idx[r - 1])][None].to(canvas.dtype) + sb * noise.to(canvas.dtype)
        out.append(canvas * m + bg * (1 - m))
    return torch.cat(out, 0)


def masked_mean(x: torch.Tensor, masks: torch.Tensor) -> torch.Tensor:
    """x [R * B, C, h, w], masks [R, B, h, w] -> [B, C, h, w]: value += m_r x_r, count += m_r in ascending r; where(count > 0, value / count, value)"""
    R, B = masks.shape[:2]
    xs = x.reshape(R, B, *x.shape[1:])
    value = torch.zeros_like(xs[0])
    count = torch.zeros_like(xs[0])
    for r in range(R):
        m = masks[r][:, None].to(x.dtype)
        value = value + m * xs[r]
        count = count + m.expand_as(value)
    return torch.where(count > 0, value / count, value)


def generate_regions(unet_sd, vae_sd, cfg, ctx: torch.Tensor, latents: torch.Tensor, masks: torch.Tensor, backgrounds: Optional[torch.Tensor],
                     idx, steps: int, guidance: float, bootstrapping: int, recorders: Optional[list] = None, decode: bool = True):
    """ctx [2 R B, T, D] = [uncond x R B | cond x R B], row r * B + p; latents [B, 4, h, w]; masks [R, B, h, w]; backgrounds [N, 4, h, w];
    idx [bootstrapping][R - 1]; recorders: one per region (each sees the B images of its region).  Returns (uint8 images or None, latents)."""
    from oracle import sd_oracle as O
    sch = O.DDIM(cfg.sched.num_train_timesteps, cfg.sched.beta_start, cfg.sched.beta_end, cfg.sched.steps_offset, cfg.sched.set_alpha_to_one,
                 cfg.sched.prediction_type)
    ts = sch.set_timesteps(steps)
    R, B = masks.shape[:2]
    assert ctx.shape[0] == 2 * R * B
    x = latents.clone().float() * sch.init_noise_sigma
    noise = x.clone()
    un, co = ctx[:R * B], ctx[R * B:]
    with torch.no_grad():
        for s, t in enumerate(ts):
            if s < bootstrapping and R > 1:
                ac = float(sch.alphas_cumprod[int(t)])
                xr = spread(x, masks, noise, backgrounds, idx[s], ac ** 0.5, (1 - ac) ** 0.5)
            else:
                xr = spread(x, masks)
            stepped = []
            for r in range(R):                                     # one forward per region: its recorder sees exactly its rows
                xv = xr[r * B:(r + 1) * B]
                c = torch.cat([un[r * B:(r + 1) * B], co[r * B:(r + 1) * B]], 0)
                eps = O.unet_forward(unet_sd, cfg.unet, torch.cat([xv, xv], 0), torch.tensor(int(t)), c, recorders[r] if recorders else None)
                eu, ec = eps.chunk(2)
                stepped.append(sch.step(eu + guidance * (ec - eu), int(t), xv))
            x = masked_mean(torch.cat(stepped, 0), masks)
        img = O.postprocess_image(O.vae_decode(vae_sd, cfg.vae, x / cfg.vae.scaling_factor)) if decode else None
    return img, x


def region_word_map(word_maps: List[Optional[torch.Tensor]], masks: torch.Tensor) -> torch.Tensor:
    """word_maps: per region [B, h, w] or None (the word is not in that region's prompt: zeros); masks [R, B, h, w] -> [B, h, w]:
    sum_r m_r w_r / sum_r m_r (the sum itself where no mask covers the pixel)."""
    num = torch.zeros_like(masks[0])
    for r, w in enumerate(word_maps):
        if w is not None:
            num = num + masks[r] * w
    den = masks.sum(0)
    return torch.where(den > 0, num / den, num)
