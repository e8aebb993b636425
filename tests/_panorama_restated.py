"""fp32 CPU restatement of diffusers 0.21.2 `StableDiffusionPanoramaPipeline` (MultiDiffusion) for the panorama tests [upstream-knowledge:
diffusers is not installed where the tests run; the loop below is written from its published source as the issue restates it].

`get_views` in latent units, `overlap_mean` = `value[view] += x; count[view] += 1; where(count > 0, value / count, value)` in view order,
`generate_panorama` = the denoising loop on top of the oracle's `unet_forward` / `DDIM` / `vae_decode`, with one `DaamRecorder` per view,
and `canvas_heat_map` = this project's panorama heat map: every view's daam global map, overlap-averaged like the latents (daam itself has
no panorama support).  Unlike diffusers, every panorama of a batch is independent ([uncond x B | cond x B] contexts, as `O.generate`)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch


def get_views(lh: int, lw: int, window: int, stride: int = 8) -> List[Tuple[int, int, int, int]]:
    nbh = (lh - window) // stride + 1 if lh > window else 1
    nbw = (lw - window) // stride + 1 if lw > window else 1
    out = []
    for i in range(nbh * nbw):
        hs, ws = (i // nbw) * stride, (i % nbw) * stride
        out.append((hs, hs + window, ws, ws + window))
    return out


def slice_views(canvas: torch.Tensor, window: int, stride: int = 8) -> torch.Tensor:
    """[B, C, Lh, Lw] -> [B * V, C, window, window], view-major within a panorama."""
    B = canvas.shape[0]
    vs = get_views(canvas.shape[2], canvas.shape[3], window, stride)
    return torch.stack([canvas[b, :, hs:he, ws:we] for b in range(B) for (hs, he, ws, we) in vs])


def overlap_mean(views: torch.Tensor, batch: int, lh: int, lw: int, stride: int = 8, return_count: bool = False):
    """views [B * V, C, window, window] (view-major within a panorama) -> [B, C, Lh, Lw], diffusers' value / count in view order."""
    window = views.shape[-1]
    vs = get_views(lh, lw, window, stride)
    V = len(vs)
    assert views.shape[0] == batch * V, (views.shape, batch, V)
    value = torch.zeros(batch, views.shape[1], lh, lw, dtype=views.dtype, device=views.device)
    count = torch.zeros_like(value)
    x = views.reshape(batch, V, *views.shape[1:])
    for i, (hs, he, ws, we) in enumerate(vs):
        value[:, :, hs:he, ws:we] += x[:, i]
        count[:, :, hs:he, ws:we] += 1
    out = torch.where(count > 0, value / count, value)
    return (out, count) if return_count else out


def generate_panorama(unet_sd, vae_sd, cfg, ctx: torch.Tensor, latents: torch.Tensor, steps: int, guidance: float, window: int,
                      stride: int = 8, recorders: Optional[list] = None, decode: bool = True):
    """ctx [2B, T, D] = [uncond x B, cond x B]; latents [B, 4, Lh, Lw]; recorders: one per view (each sees the B panoramas as images).
    Returns (uint8 images or None, final latents)."""
    from oracle import sd_oracle as O
    sch = O.DDIM(cfg.sched.num_train_timesteps, cfg.sched.beta_start, cfg.sched.beta_end, cfg.sched.steps_offset, cfg.sched.set_alpha_to_one,
                 cfg.sched.prediction_type)
    ts = sch.set_timesteps(steps)
    x = latents.clone().float() * sch.init_noise_sigma
    vs = get_views(x.shape[2], x.shape[3], window, stride)
    with torch.no_grad():
        for t in ts:
            value, count = torch.zeros_like(x), torch.zeros_like(x)
            for i, (hs, he, ws, we) in enumerate(vs):
                xv = x[:, :, hs:he, ws:we]
                eps = O.unet_forward(unet_sd, cfg.unet, torch.cat([xv, xv], 0), torch.tensor(int(t)), ctx, recorders[i] if recorders else None)
                eu, ec = eps.chunk(2)
                value[:, :, hs:he, ws:we] += sch.step(eu + guidance * (ec - eu), int(t), xv)
                count[:, :, hs:he, ws:we] += 1
            x = torch.where(count > 0, value / count, value)
        img = O.postprocess_image(O.vae_decode(vae_sd, cfg.vae, x / cfg.vae.scaling_factor)) if decode else None
    return img, x


def view_recorders(lh: int, lw: int, window: int, tokens: int, stride: int = 8) -> list:
    from oracle import sd_oracle as O
    return [O.DaamRecorder(window * window, context_size=tokens) for _ in get_views(lh, lw, window, stride)]


def view_heat_maps(recorders: list) -> torch.Tensor:
    """[V, B, T, window, window]: every view's daam global map."""
    return torch.stack([r.compute_global_heat_map() for r in recorders])


def canvas_heat_map(recorders: list, lh: int, lw: int, stride: int = 8) -> torch.Tensor:
    """[B, T, Lh, Lw]: the overlap mean of the views' global maps."""
    hm = view_heat_maps(recorders)                        # [V, B, T, w, w]
    V, B = hm.shape[:2]
    return overlap_mean(hm.transpose(0, 1).reshape(B * V, *hm.shape[2:]), B, lh, lw, stride)
