"""An fp32 restatement of diffusers 0.21.2's T2I-Adapter [upstream-knowledge: T2IAdapter / FullAdapter / AdapterBlock /
AdapterResnetBlock, UNet2DConditionModel.forward with down_block_additional_residuals and no mid residual, and
StableDiffusionAdapterPipeline], written for this suite from the published code's behaviour and composed from oracle.sd_oracle's blocks.
Independent of agenda_amd's implementation."""
import torch
import torch.nn.functional as F

from oracle import sd_oracle as O


def pixel_unshuffle(x, r):
    """PixelUnshuffle(r): out[c r^2 + i r + j][h][w] = in[c][h r + i][w r + j]."""
    b, c, H, W = x.shape
    x = x.reshape(b, c, H // r, r, W // r, r)            # [b, c, h, i, w, j]
    return x.permute(0, 1, 3, 5, 2, 4).reshape(b, c * r * r, H // r, W // r)


def factor_rule(n, scale, factor):
    """The features times `scale` on evaluations i < int(factor * n), the plain UNet on the rest."""
    return [float(scale) if i < int(factor * n) else 0.0 for i in range(n)]


def adapter_forward(sd, acfg, image):
    """FullAdapter.forward: image [B,C,H,W] in [0,1] -> one feature per entry of `channels`.  conv_in on the unshuffled image; block 0
    keeps the resolution, block i > 0 starts with AvgPool2d(2, 2); `in_conv` (1x1) exists only where the width changes; each
    AdapterResnetBlock is x + block2(relu(block1(x))) with block1 3x3 and block2 1x1, no normalisation."""
    ch = acfg.channels
    x = pixel_unshuffle(image, acfg.downscale_factor)
    x = F.conv2d(x, sd["adapter.conv_in.weight"], sd["adapter.conv_in.bias"], padding=1)
    feats = []
    for i in range(len(ch)):
        b = f"adapter.body.{i}."
        if i > 0:
            x = F.avg_pool2d(x, kernel_size=2, stride=2)
        if (ch[i - 1] if i else ch[0]) != ch[i]:
            x = F.conv2d(x, sd[b + "in_conv.weight"], sd[b + "in_conv.bias"])
        for j in range(acfg.num_res_blocks):
            r = b + f"resnets.{j}."
            h = F.relu(F.conv2d(x, sd[r + "block1.weight"], sd[r + "block1.bias"], padding=1))
            x = x + F.conv2d(h, sd[r + "block2.weight"], sd[r + "block2.bias"])
        feats.append(x)
    return feats


def unet_forward_with_adapter(sd, ucfg, x, t, ctx, feats, recorder=None):
    """UNet2DConditionModel.forward with the adapter's features as down_block_additional_residuals and no mid residual.  Feature i
    belongs to down block i.

    - In a block with cross-attention, the feature is added to the hidden state after the block's **last** resnet + transformer pair.
      That is before the state is appended as a res sample and before the downsampler.  So the sum is both a skip and the
      downsampler's input.
    - In the last, attention-free block, `sample += feature` runs in place after the block.  That is the same tensor as the block's
      last res sample, so there too the sum is both the skip and the mid block's input.

    The oracle's blocks, walked here so the injection point is explicit."""
    boc, g = ucfg.block_out_channels, ucfg.norm_num_groups
    if t.ndim == 0:
        t = t[None].expand(x.shape[0])
    temb = O.timestep_embedding(t, boc[0])
    temb = F.linear(temb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    temb = F.linear(F.silu(temb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    h = F.conv2d(x, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    skips = [h]
    nlev = len(boc)
    assert len(feats) == nlev
    for i in range(nlev):
        for j in range(ucfg.layers_per_block):
            h = O.resnet_block(h, temb, sd, f"down_blocks.{i}.resnets.{j}.", g, 1e-5)
            if ucfg.down_cross[i]:
                nm = f"down_blocks.{i}.attentions.{j}."
                h = O.transformer_2d(h, ctx, sd, nm, ucfg.num_heads[i], g, ucfg.use_linear_projection, recorder, nm + "transformer_blocks.0.attn2")
            if j == ucfg.layers_per_block - 1:
                h = h + feats[i]                         # both rules above: the sum is this layer's res sample and what runs on
            skips.append(h)
        if i != nlev - 1:
            h = F.conv2d(h, sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], sd[f"down_blocks.{i}.downsamplers.0.conv.bias"], stride=2, padding=1)
            skips.append(h)
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.0.", g, 1e-5)
    h = O.transformer_2d(h, ctx, sd, "mid_block.attentions.0.", ucfg.num_heads[-1], g, ucfg.use_linear_projection,
                         recorder, "mid_block.attentions.0.transformer_blocks.0.attn2")
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.1.", g, 1e-5)
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


def adapted_eps(usd, ucfg, x, t, ctx, feats, scale, recorder=None):
    """One adapter-conditioned UNet evaluation on rows x; feats hold one image per row (scale 0: the UNet alone, as the device skips it)."""
    t = torch.as_tensor(t, dtype=torch.float32)
    if scale == 0.0:
        return O.unet_forward(usd, ucfg, x, t, ctx, recorder)
    return unet_forward_with_adapter(usd, ucfg, x, t, ctx, [f * scale for f in feats], recorder)


def generate(usd, vsd, asd, cfg, acfg, ctx, latents, image, steps, scheduler, scale=1.0, factor=1.0, guidance=7.5, recorder=None):
    """The oracle's UNet and VAE with the restated adapter, stepped by the oracle's DDIM / PNDM or the restated DPM-Solver++ 2M; image
    [B,C,H,W] in [0,1]; the features are computed once and both CFG halves get the same ones.  Returns (uint8 images, latents)."""
    import _dpm_restated as R
    s = cfg.sched
    with torch.no_grad():
        feats = [torch.cat([f, f], 0) for f in adapter_forward(asd, acfg, image.float())]

    def model(x, i, t, n):
        k = factor_rule(n, scale, factor)[i]
        eps = adapted_eps(usd, cfg.unet, torch.cat([x, x], 0), t, ctx, feats, k, recorder)
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
