"""An fp32 restatement of diffusers 0.21.2's ControlNet [upstream-knowledge: ControlNetConditioningEmbedding, ControlNetModel.forward,
UNet2DConditionModel.forward with down_block_additional_residuals / mid_block_additional_residual, and
StableDiffusionControlNetPipeline's controlnet_keep rule], written for this suite from the published code's behaviour and composed from
oracle.sd_oracle's blocks.  Independent of agenda_amd's implementation."""
import torch
import torch.nn.functional as F

from oracle import sd_oracle as O


def keep_rule(n, start, end):
    """[upstream-knowledge] controlnet_keep: 1 - float(i / n < start or (i + 1) / n > end) for evaluation i of n."""
    return [1.0 - float(i / n < start or (i + 1) / n > end) for i in range(n)]


def cond_embedding(sd, cond, n_emb, bgr=False):
    """ControlNetConditioningEmbedding: silu(conv_in), per step silu(conv c->c), silu(conv c->c' stride 2), conv_out (no activation)."""
    if bgr:
        cond = cond.flip(1)
    e = "controlnet_cond_embedding."
    h = F.silu(F.conv2d(cond, sd[e + "conv_in.weight"], sd[e + "conv_in.bias"], padding=1))
    for i in range(n_emb - 1):
        h = F.silu(F.conv2d(h, sd[e + f"blocks.{2 * i}.weight"], sd[e + f"blocks.{2 * i}.bias"], padding=1))
        h = F.silu(F.conv2d(h, sd[e + f"blocks.{2 * i + 1}.weight"], sd[e + f"blocks.{2 * i + 1}.bias"], padding=1, stride=2))
    return F.conv2d(h, sd[e + "conv_out.weight"], sd[e + "conv_out.bias"], padding=1)


def controlnet_forward(sd, ucfg, x, t, ctx, cond, scale=1.0, n_emb=4, bgr=False):
    """ControlNetModel.forward -> (12 down residuals, mid residual), each times `scale`."""
    boc, g = ucfg.block_out_channels, ucfg.norm_num_groups
    if t.ndim == 0:
        t = t[None].expand(x.shape[0])
    temb = O.timestep_embedding(t, boc[0])
    temb = F.linear(temb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    temb = F.linear(F.silu(temb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    h = F.conv2d(x, sd["conv_in.weight"], sd["conv_in.bias"], padding=1) + cond_embedding(sd, cond, n_emb, bgr)
    res = [h]
    for i in range(len(boc)):
        for j in range(ucfg.layers_per_block):
            h = O.resnet_block(h, temb, sd, f"down_blocks.{i}.resnets.{j}.", g, 1e-5)
            if ucfg.down_cross[i]:
                h = O.transformer_2d(h, ctx, sd, f"down_blocks.{i}.attentions.{j}.", ucfg.num_heads[i], g, ucfg.use_linear_projection)
            res.append(h)
        if i != len(boc) - 1:
            h = F.conv2d(h, sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], sd[f"down_blocks.{i}.downsamplers.0.conv.bias"],
                         stride=2, padding=1)
            res.append(h)
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.0.", g, 1e-5)
    h = O.transformer_2d(h, ctx, sd, "mid_block.attentions.0.", ucfg.num_heads[-1], g, ucfg.use_linear_projection)
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.1.", g, 1e-5)
    down = [F.conv2d(r, sd[f"controlnet_down_blocks.{k}.weight"], sd[f"controlnet_down_blocks.{k}.bias"]) * scale for k, r in enumerate(res)]
    mid = F.conv2d(h, sd["controlnet_mid_block.weight"], sd["controlnet_mid_block.bias"]) * scale
    return down, mid


def unet_forward_with_residuals(sd, ucfg, x, t, ctx, down, mid, recorder=None):
    """UNet2DConditionModel.forward with additional residuals: skip k += down[k] after the down pass, mid output += mid.  The oracle's
    blocks, walked here so the injection point is explicit."""
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
    skips = [s + r for s, r in zip(skips, down)]
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.0.", g, 1e-5)
    h = O.transformer_2d(h, ctx, sd, "mid_block.attentions.0.", ucfg.num_heads[-1], g, ucfg.use_linear_projection,
                         recorder, "mid_block.attentions.0.transformer_blocks.0.attn2")
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.1.", g, 1e-5)
    h = h + mid
    up_cross, rev_heads = tuple(reversed(ucfg.down_cross)), tuple(reversed(ucfg.num_heads))
    for i in range(nlev):
        for j in range(ucfg.layers_per_block + 1):
            h = torch.cat([h, skips.pop()], dim=1)
            h = O.resnet_block(h, temb, sd, f"up_blocks.{i}.resnets.{j}.", g, 1e-5)
            if up_cross[i]:
                nm = f"up_blocks.{i}.attentions.{j}."
                h = O.transformer_2d(h, ctx, sd, nm, rev_heads[i], g, ucfg.use_linear_projection, recorder, nm + "transformer_blocks.0.attn2")
        if i != nlev - 1:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, sd[f"up_blocks.{i}.upsamplers.0.conv.weight"], sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], padding=1)
    h = F.silu(O._gn(h, sd, "conv_norm_out", g, 1e-5))
    return F.conv2d(h, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


def generate(usd, vsd, csd, cfg, ctx, latents, cond, steps, scheduler, scale=1.0, start=0.0, end=1.0, guidance=7.5, recorder=None):
    """The oracle's UNet and VAE with the restated ControlNet, stepped by the oracle's DDIM / PNDM or the restated DPM-Solver++ 2M;
    cond [B,3,S,S] is doubled for CFG.  Returns (uint8 images, latents)."""
    import _dpm_restated as R
    cond2 = torch.cat([cond, cond], 0)
    s = cfg.sched

    def model(x, i, t, n):
        k = scale * keep_rule(n, start, end)[i]
        eps = controlled_eps(usd, csd, cfg.unet, torch.cat([x, x], 0), t, ctx, cond2, k, recorder)
        eu, ec = eps.chunk(2)
        return eu + guidance * (ec - eu)

    with torch.no_grad():
        x = latents.clone().float()
        if scheduler == "dpm":
            _, x = R.sample(steps, False, s.prediction_type, lambda x_, i, t: model(x_, i, t, steps), x)
        else:
            sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
                   O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type))
            ts = sch.set_timesteps(steps)
            for i, t in enumerate(ts):
                x = sch.step(model(x, i, float(int(t)), len(ts)), int(t), x)
        img = O.postprocess_image(O.vae_decode(vsd, cfg.vae, x / cfg.vae.scaling_factor))
    return img, x


def controlled_eps(usd, csd, ucfg, x, t, ctx, cond, scale, recorder=None, n_emb=4):
    """One ControlNet-conditioned UNet evaluation (scale 0: the UNet alone, as the device skips it)."""
    t = torch.as_tensor(t, dtype=torch.float32)
    if scale == 0.0:
        return O.unet_forward(usd, ucfg, x, t, ctx, recorder)
    down, mid = controlnet_forward(csd, ucfg, x, t, ctx, cond, scale, n_emb)
    return unet_forward_with_residuals(usd, ucfg, x, t, ctx, down, mid, recorder)
