"""Stable Diffusion inpainting restated in fp32 from diffusers 0.21.2 StableDiffusionInpaintPipeline [upstream-knowledge], built from the
oracle's blocks (unet_forward takes any conv_in width from the weights, vae_encode_moments, DDIM, PNDM) and the DPM-Solver++ restatement.
Independent of agenda_amd.  The rules, numbered as the tests cite them:
  1 image: x / 255 in fp32, then 2 x - 1
  2 mask: grayscale / 255, then m < 0.5 -> 0, else 1
  4 masked image = image * (mask < 0.5)
  5 latent mask = nearest interpolation: latent pixel (i, j) takes mask pixel (8 i, 8 j)
  6 latents of an image = (mean + exp(logvar / 2) draw) * scaling_factor
  7 start: noise * init_noise_sigma (strength 1) or add_noise(image_latents, noise, t_0)
  8 a 9-channel UNet reads cat(latents, mask, masked-image latents) in both CFG halves
  9 a 4-channel UNet: after step i, latents = (1 - mask) add_noise(image_latents, noise, t_{i+1}) + mask latents (image_latents after the
    last step), each image with its own latents and mask."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sd_oracle as O


def preprocess_image(u8):
    """Rule 1: uint8 [B,S,S,3] -> fp32 [B,3,S,S]."""
    x = torch.as_tensor(np.asarray(u8)).permute(0, 3, 1, 2).to(torch.float32) / 255.0
    return 2.0 * x - 1.0


def preprocess_mask(m):
    """Rule 2: uint8 [B,S,S] (/ 255) or float [B,S,S] in [0,1] -> binary fp32 [B,1,S,S]."""
    m = torch.as_tensor(np.asarray(m) if not torch.is_tensor(m) else m)
    m = m.to(torch.float32) / 255.0 if m.dtype == torch.uint8 else m.to(torch.float32)
    m = m[:, None].clone()
    m[m < 0.5] = 0.0
    m[m >= 0.5] = 1.0
    return m


def masked_image(image, mask):
    """Rule 4."""
    return image * (mask < 0.5)


def latent_mask(mask, L):
    """Rule 5."""
    return F.interpolate(mask, size=(L, L))


def latents_of(vsd, vcfg, x, draw):
    """Rule 6."""
    mean, logvar = O.vae_encode_moments(vsd, vcfg, x)
    return (mean + torch.exp(0.5 * logvar) * draw) * vcfg.scaling_factor


def add_noise(abar, x0, noise, t):
    a = abar[int(t)]
    return a ** 0.5 * x0 + (1 - a) ** 0.5 * noise


def _abar(s):
    betas = torch.linspace(s.beta_start ** 0.5, s.beta_end ** 0.5, s.num_train_timesteps, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def _dpm_loop(n, pred, model, x, after_step):
    """DPM-Solver++ (2M), linspace spacing, as tests/_dpm_restated.sample, with after_step(i, x) -> x run after every step."""
    import _dpm_restated as R
    t, al, sg = R.grid(n, False)
    lam = [math.log(float(a) / float(s)) for a, s in zip(al, sg)]
    x0_prev = None
    for i in range(n):
        a_s, s_s, a_t, s_t = float(al[i]), float(sg[i]), float(al[i + 1]), float(sg[i + 1])
        m = model(x, float(t[i]))
        x0 = (x - s_s * m) / a_s if pred == "epsilon" else a_s * x - s_s * m
        h = lam[i + 1] - lam[i]
        if i == 0 or (i == n - 1 and n < 15) or h == 0:
            D = x0
        else:
            r = (lam[i] - lam[i - 1]) / h
            D = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * x0_prev
        x = (s_t / s_s) * x - a_t * math.expm1(-h) * D
        x0_prev = x0
        x = after_step(i, x)
    return [int(round(v)) for v in t], x


def generate(usd, vsd, cfg, ctx, image_u8, mask, steps, scheduler, strength=1.0, noise_enc_image=None, noise=None,
             noise_enc_masked=None, guidance=7.5, recorder=None):
    """image_u8 uint8 [B,S,S,3], mask uint8 / float [B,S,S], one row per image (no batch expansion); ctx [2B,T,D]; scheduler "ddim",
    "pndm" or "dpm".  The draws are explicit: noise_enc_image (image latents; 4-channel UNets or strength < 1), noise (start),
    noise_enc_masked (9-channel UNets).  Returns (uint8 images, final latents, dict of the intermediate inputs)."""
    s = cfg.sched
    nine = cfg.unet.in_channels != cfg.unet.out_channels
    abar = _abar(s)
    with torch.no_grad():
        img = preprocess_image(image_u8)
        m = preprocess_mask(mask)
        L = img.shape[-1] // cfg.vae_scale_factor
        mlat = latent_mask(m, L)
        img_lat = latents_of(vsd, cfg.vae, img, noise_enc_image) if (not nine or strength < 1.0) else None
        msk_lat = latents_of(vsd, cfg.vae, masked_image(img, m), noise_enc_masked) if nine else None

        def model(x, t):
            xin = torch.cat([x, mlat, msk_lat], 1) if nine else x
            eps = O.unet_forward(usd, cfg.unet, torch.cat([xin, xin], 0), torch.tensor(t, dtype=torch.float32), ctx, recorder)
            eu, ec = eps.chunk(2)
            return eu + guidance * (ec - eu)

        def blend(ts):
            def after(i, x):
                if nine:
                    return x
                proper = add_noise(abar, img_lat, noise, ts[i + 1]) if i + 1 < len(ts) else img_lat
                return (1 - mlat) * proper + mlat * x
            return after

        if scheduler == "dpm":
            import _dpm_restated as R
            ts = [int(round(v)) for v in R.grid(steps, False)[0]]
            x = noise.clone().float()
            _, x = _dpm_loop(steps, s.prediction_type, lambda x_, t: model(x_, t), x, blend(ts))
        else:
            sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
                   O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type))
            ts = [int(t) for t in sch.set_timesteps(steps)]
            if strength < 1.0:
                init = min(int(steps * strength), steps)
                ts = ts[max(steps - init, 0):]
                x = add_noise(abar, img_lat, noise, ts[0])
            else:
                x = noise.clone().float() * sch.init_noise_sigma
            after = blend(ts)
            for i, t in enumerate(ts):
                x = sch.step(model(x, float(t)), t, x)
                x = after(i, x)
        out = O.postprocess_image(O.vae_decode(vsd, cfg.vae, x / cfg.vae.scaling_factor))
    return out, x, {"mask": mlat, "image_latents": img_lat, "masked_image_latents": msk_lat, "image": img}
