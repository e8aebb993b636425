"""InstructPix2Pix restated in fp32 from diffusers 0.21.2 StableDiffusionInstructPix2PixPipeline [upstream-knowledge], built from the
oracle's blocks (unet_forward takes any conv_in width from the weights, vae_encode_moments, DDIM, PNDM) and the DPM-Solver++ restatement.
Independent of agenda_amd.  The rules, numbered as the tests cite them:
  1 image: x / 255 in fp32, then 2 x - 1 (a float image is taken as it is)
  2 image latents = the VAE posterior's mean (`latent_dist.mode()`), NOT multiplied by the scaling factor
  3 the latents start as noise * init_noise_sigma at the image's size; the whole schedule runs (no strength)
  4 the UNet reads cat(latents, image latents) on the channel axis, in three branches: text (prompt, image latents), image (negative
    prompt, image latents), uncond (negative prompt, zero image latents)
  5 e = e_uncond + s_t (e_text - e_image) + s_i (e_image - e_uncond), for eps and v output alike, then the scheduler's step
The [image | text] pair runs as one unet_forward with the recorder (which keeps the conditional half: the text branch); the uncond rows run
on their own without it."""
import numpy as np
import torch

from oracle import sd_oracle as O


def preprocess_image(image):
    """Rule 1: uint8 [B,H,W,3] -> fp32 [B,3,H,W]; float [B,3,H,W] unchanged."""
    x = torch.as_tensor(np.asarray(image) if not torch.is_tensor(image) else image)
    if x.dtype != torch.uint8:
        return x.to(torch.float32)
    x = x.permute(0, 3, 1, 2).to(torch.float32) / 255.0
    return 2.0 * x - 1.0


def image_latents(vsd, vcfg, x):
    """Rule 2."""
    return O.vae_encode_moments(vsd, vcfg, x)[0]


def combine(e_uncond, e_image, e_text, s_t, s_i):
    """Rule 5."""
    return e_uncond + s_t * (e_text - e_image) + s_i * (e_image - e_uncond)


def fold(e_uncond, e_image, e_text, s_i):
    """The two-way form of rule 5: (lo, hi) with lo + s_t (hi - lo) = combine(..., s_t, s_i) for every s_t."""
    lo = s_i * e_image - (s_i - 1.0) * e_uncond
    return lo, lo + e_text - e_image


def model_fn(usd, cfg, ctx, img_lat, s_t, s_i, recorder=None):
    """x, t -> the combined model output of rules 4 and 5.  ctx [2B,T,D] = [uncond | cond]; img_lat [B,c,Lh,Lw]."""
    B = img_lat.shape[0]

    def model(x, t):
        tt = torch.tensor(t, dtype=torch.float32)
        xi = torch.cat([x, img_lat], 1)
        e_image, e_text = O.unet_forward(usd, cfg.unet, torch.cat([xi, xi], 0), tt, ctx, recorder).chunk(2)
        e_uncond = O.unet_forward(usd, cfg.unet, torch.cat([x, torch.zeros_like(img_lat)], 1), tt, ctx[:B], None)
        return combine(e_uncond, e_image, e_text, s_t, s_i)
    return model


def denoise(usd, cfg, ctx, img_lat, noise, steps, scheduler, guidance=7.5, image_guidance=1.5, recorder=None):
    """The three-branch loop from `noise` [B,c,Lh,Lw] under "ddim", "pndm" or "dpm"; returns the final latents."""
    s = cfg.sched
    model = model_fn(usd, cfg, ctx, img_lat, guidance, image_guidance, recorder)
    with torch.no_grad():
        if scheduler == "dpm":
            from _inpaint_restated import _dpm_loop
            return _dpm_loop(steps, s.prediction_type, model, noise.clone().float(), lambda i, x: x)[1]
        sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
               O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type))
        ts = [int(t) for t in sch.set_timesteps(steps)]
        x = noise.clone().float() * sch.init_noise_sigma
        for t in ts:
            x = sch.step(model(x, float(t)), t, x)
    return x


def generate(usd, vsd, cfg, ctx, image, noise, steps, scheduler, guidance=7.5, image_guidance=1.5, recorder=None, img_lat=None):
    """image uint8 [B,H,W,3] or float [B,3,H,W], one row per image; ctx [2B,T,D]; noise [B,c,H/8,W/8].  `img_lat` replaces the encoded
    image latents when given.  Returns (uint8 images, final latents, image latents)."""
    with torch.no_grad():
        if img_lat is None:
            img_lat = image_latents(vsd, cfg.vae, preprocess_image(image))
        x = denoise(usd, cfg, ctx, img_lat, noise, steps, scheduler, guidance, image_guidance, recorder)
        out = O.postprocess_image(O.vae_decode(vsd, cfg.vae, x / cfg.vae.scaling_factor))
    return out, x, img_lat
