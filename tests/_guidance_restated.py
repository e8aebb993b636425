"""guidance_rescale, the DDIM timestep spacings and the zero-terminal-SNR beta table of Lin et al. 2023 ("Common Diffusion Noise Schedules
and Sample Steps are Flawed"), restated from diffusers 0.21.2 [upstream-knowledge] and independent of agenda_amd: `rescale_noise_cfg` with
torch.std, the three grids of `DDIMScheduler.set_timesteps`, `rescale_zero_terminal_snr`, and a re-walk of the oracle's loop -- DDIM and
PNDM of oracle.sd_oracle, DPM-Solver++ 2M of tests/_dpm_restated.py -- with the rescale between the CFG combine and the scheduler step."""
import numpy as np
import torch

import _dpm_restated as D
from oracle import sd_oracle as O


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """diffusers' function, line for line: std over every dimension but the batch's, unbiased (torch.std's default)."""
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg


def factor(eps_u, eps_c, guidance, phi, dtype=torch.float64):
    """f_b of every image [B] in `dtype`: rescale_noise_cfg(m, eps_c, phi) == f_b m with m = eps_u + g (eps_c - eps_u)."""
    eu, ec = eps_u.to(dtype), eps_c.to(dtype)
    m = eu + guidance * (ec - eu)
    dims = list(range(1, m.ndim))
    return phi * ec.std(dim=dims) / m.std(dim=dims) + (1 - phi)


def ddim_grid(spacing, n, T=1000, steps_offset=1):
    if spacing == "leading":
        return (np.arange(0, n) * (T // n)).round()[::-1].copy().astype(np.int64) + steps_offset
    if spacing == "trailing":
        return np.round(np.arange(T, 0, -T / n)).astype(np.int64) - 1
    if spacing == "linspace":
        return np.linspace(0, T - 1, n).round()[::-1].copy().astype(np.int64)
    raise ValueError(spacing)


def zero_snr_betas(betas):
    """diffusers' rescale_zero_terminal_snr (the paper's algorithm 1) in torch float32."""
    alphas_bar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    first, last = alphas_bar_sqrt[0].clone(), alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt -= last
    alphas_bar_sqrt *= first / (first - last)
    alphas_bar = alphas_bar_sqrt ** 2
    alphas = torch.cat([alphas_bar[0:1], alphas_bar[1:] / alphas_bar[:-1]])
    return 1 - alphas


def alphas_cumprod(zero_snr=False, T=1000, beta_start=0.00085, beta_end=0.012):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
    if zero_snr:
        betas = zero_snr_betas(betas)
    return torch.cumprod(1.0 - betas, dim=0)


class DDIM(O.DDIM):
    """The oracle's DDIM step on another grid and, with zero_snr, the rescaled table (prev_t = t - T // n for every spacing, as upstream)."""

    def __init__(self, s, spacing="leading", zero_snr=False):
        super().__init__(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type)
        self.spacing = spacing
        if zero_snr:
            self.alphas_cumprod = alphas_cumprod(True, s.num_train_timesteps, s.beta_start, s.beta_end)
            self.final_alpha_cumprod = torch.tensor(1.0) if s.set_alpha_to_one else self.alphas_cumprod[0]

    def set_timesteps(self, n):
        self.num_inference_steps = n
        self.timesteps = ddim_grid(self.spacing, n, self.T, self.steps_offset)
        return self.timesteps


def generate(usd, vsd, cfg, ctx, latents, steps, scheduler, phi=0.0, guidance=7.5, recorder=None, eps_fn=None, spacing="leading",
             zero_snr=False, factors=None):
    """The oracle's UNet and VAE, stepped by the oracle's DDIM / PNDM or the restated DPM-Solver++ 2M, with rescale_noise_cfg between
    combine and step when phi > 0.  eps_fn(x2, t, ctx, recorder) -> eps replaces the plain forward.  factors: a list that receives
    every evaluation's f_b.  Returns (uint8 images, latents)."""
    s = cfg.sched

    def model(x, t):
        x2, tt = torch.cat([x, x], 0), torch.as_tensor(t, dtype=torch.float32)
        eps = eps_fn(x2, tt, ctx, recorder) if eps_fn else O.unet_forward(usd, cfg.unet, x2, tt, ctx, recorder)
        eu, ec = eps.chunk(2)
        m = eu + guidance * (ec - eu)
        if phi > 0:
            if factors is not None:
                factors.append(factor(eu, ec, guidance, phi))
            m = rescale_noise_cfg(m, ec, phi)
        return m

    with torch.no_grad():
        x = latents.clone().float()
        if scheduler == "dpm":
            _, x = D.sample(steps, False, s.prediction_type, lambda x_, i, t: model(x_, t), x)
        else:
            sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
                   DDIM(s, spacing, zero_snr))
            for t in sch.set_timesteps(steps):
                x = sch.step(model(x, float(int(t))), int(t), x)
        img = O.postprocess_image(O.vae_decode(vsd, cfg.vae, x / cfg.vae.scaling_factor))
    return img, x
