"""An fp32 restatement of FreeU [upstream-knowledge: Si et al. 2023; diffusers >= 0.22 `enable_freeu(s1, s2, b1, b2)`, `fourier_filter`
and `apply_freeu` of diffusers.utils.torch_utils, and the up blocks' use of them], written for this suite from the published code's
behaviour and composed from oracle.sd_oracle's blocks.  Independent of agenda_amd's implementation.

`fourier_filter` with torch.fft is the truth.  `fourier_filter_moments` is the rank-4 form the device kernel computes, kept here so the CPU
suite can pin the identity between the two."""
import math

import torch
import torch.nn.functional as F

from oracle import sd_oracle as O


def fourier_filter(x, threshold, scale):
    """x [B,C,H,W]: the centred (2 threshold) x (2 threshold) block of the shifted spectrum times `scale`, everything else kept."""
    dtype = x.dtype
    x = x.float() if dtype not in (torch.float32, torch.float64) else x
    X = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    B, C, H, W = X.shape
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    cr, cc = H // 2, W // 2
    mask[..., cr - threshold:cr + threshold, cc - threshold:cc + threshold] = scale      # (a side of 1: -1:1 is its one element)
    X = X * mask
    y = torch.fft.ifftn(torch.fft.ifftshift(X, dim=(-2, -1)), dim=(-2, -1)).real
    return y.to(dtype)


def fourier_filter_moments(x, scale):
    """The same map for threshold = 1 without a transform: the mask scales the frequencies {-1 mod H, 0} x {-1 mod W, 0} (as sets), so
    y = x + (scale - 1) / (H W) * sum_k [C_k cos a_k + S_k sin a_k] with C_k = sum x cos a_k, S_k = sum x sin a_k and
    a_k(y, x) = 2 pi (ky y / H + kx x / W)."""
    B, C, H, W = x.shape
    ys = torch.arange(H, dtype=x.dtype)[:, None]
    xs = torch.arange(W, dtype=x.dtype)[None, :]
    out = x.clone()
    for ky in sorted({(-1) % H, 0}):
        for kx in sorted({(-1) % W, 0}):
            a = 2.0 * math.pi * (ky * ys / H + kx * xs / W)
            ca, sa = torch.cos(a), torch.sin(a)
            Ck = (x * ca).sum((-2, -1), keepdim=True)
            Sk = (x * sa).sum((-2, -1), keepdim=True)
            out = out + (scale - 1.0) / (H * W) * (Ck * ca + Sk * sa)
    return out


def apply_freeu(resolution_idx, hidden, skip, s1, s2, b1, b2):
    """Up block `resolution_idx` in {0, 1}: the first half of the backbone's channels times b, the skip's low frequencies times s."""
    if resolution_idx == 0:
        b, s = b1, s1
    elif resolution_idx == 1:
        b, s = b2, s2
    else:
        return hidden, skip
    n = hidden.shape[1] // 2
    hidden = torch.cat([hidden[:, :n] * b, hidden[:, n:]], 1)
    skip = fourier_filter(skip, 1, s)
    return hidden, skip


def unet_forward_with_freeu(sd, ucfg, x, t, ctx, s1, s2, b1, b2, recorder=None, down_residuals=None, mid_residual=None):
    """UNet2DConditionModel.forward with FreeU on: in up blocks 0 and 1, every resnet's (hidden, skip) pair goes through apply_freeu
    immediately before the concat.  down_residuals / mid_residual: a ControlNet's, added to the skips / the mid output first, so the
    filtered skip is the injected one.  The oracle's blocks, walked here so the injection point is explicit."""
    boc, g = ucfg.block_out_channels, ucfg.norm_num_groups
    if t.ndim == 0:
        t = t[None].expand(x.shape[0])
    temb = O.timestep_embedding(t, boc[0])
    temb = F.linear(temb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    temb = F.linear(F.silu(temb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    h = F.conv2d(x, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    skips = [h]
    nlev = len(boc)
    for i in range(nlev):
        for j in range(ucfg.layers_per_block):
            h = O.resnet_block(h, temb, sd, f"down_blocks.{i}.resnets.{j}.", g, 1e-5)
            if ucfg.down_cross[i]:
                nm = f"down_blocks.{i}.attentions.{j}."
                h = O.transformer_2d(h, ctx, sd, nm, ucfg.num_heads[i], g, ucfg.use_linear_projection, recorder, nm + "transformer_blocks.0.attn2")
            skips.append(h)
        if i != nlev - 1:
            h = F.conv2d(h, sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], sd[f"down_blocks.{i}.downsamplers.0.conv.bias"], stride=2, padding=1)
            skips.append(h)
    if down_residuals is not None:
        skips = [s + r for s, r in zip(skips, down_residuals)]
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.0.", g, 1e-5)
    h = O.transformer_2d(h, ctx, sd, "mid_block.attentions.0.", ucfg.num_heads[-1], g, ucfg.use_linear_projection,
                         recorder, "mid_block.attentions.0.transformer_blocks.0.attn2")
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.1.", g, 1e-5)
    if mid_residual is not None:
        h = h + mid_residual
    on = not (s1 == 1 and s2 == 1 and b1 == 1 and b2 == 1)
    up_cross, rev_heads = tuple(reversed(ucfg.down_cross)), tuple(reversed(ucfg.num_heads))
    for i in range(nlev):
        for j in range(ucfg.layers_per_block + 1):
            sk = skips.pop()
            if on:
                h, sk = apply_freeu(i, h, sk, s1, s2, b1, b2)
            h = torch.cat([h, sk], dim=1)
            h = O.resnet_block(h, temb, sd, f"up_blocks.{i}.resnets.{j}.", g, 1e-5)
            if up_cross[i]:
                nm = f"up_blocks.{i}.attentions.{j}."
                h = O.transformer_2d(h, ctx, sd, nm, rev_heads[i], g, ucfg.use_linear_projection, recorder, nm + "transformer_blocks.0.attn2")
        if i != nlev - 1:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, sd[f"up_blocks.{i}.upsamplers.0.conv.weight"], sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], padding=1)
    h = F.silu(O._gn(h, sd, "conv_norm_out", g, 1e-5))
    return F.conv2d(h, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


def generate(usd, vsd, cfg, ctx, latents, steps, scheduler, s1, s2, b1, b2, guidance=7.5, recorder=None, eps_fn=None):
    """The oracle's UNet (with FreeU) and VAE, stepped by the oracle's DDIM / PNDM or the restated DPM-Solver++ 2M.  eps_fn(x2, t, ctx,
    recorder) -> eps replaces the FreeU forward (a ControlNet-conditioned one, say).  Returns (uint8 images, latents)."""
    import _dpm_restated as R
    s = cfg.sched

    def model(x, t):
        x2, tt = torch.cat([x, x], 0), torch.as_tensor(t, dtype=torch.float32)
        eps = eps_fn(x2, tt, ctx, recorder) if eps_fn else unet_forward_with_freeu(usd, cfg.unet, x2, tt, ctx, s1, s2, b1, b2, recorder)
        eu, ec = eps.chunk(2)
        return eu + guidance * (ec - eu)

    with torch.no_grad():
        x = latents.clone().float()
        if scheduler == "dpm":
            _, x = R.sample(steps, False, s.prediction_type, lambda x_, i, t: model(x_, t), x)
        else:
            sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
                   O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type))
            ts = sch.set_timesteps(steps)
            for t in ts:
                x = sch.step(model(x, float(int(t))), int(t), x)
        img = O.postprocess_image(O.vae_decode(vsd, cfg.vae, x / cfg.vae.scaling_factor))
    return img, x
