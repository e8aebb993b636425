"""An fp32 restatement of diffusers 0.21.2's GLIGEN [upstream-knowledge: get_fourier_embeds_from_boundingbox, PositionNet,
GatedSelfAttentionDense, BasicTransformerBlock's fuser call after attn1, and StableDiffusionGLIGENPipeline's object preparation and
scheduled sampling], written for this suite from the published code's behaviour and composed from oracle.sd_oracle's blocks.  Independent of
agenda_amd's implementation."""
import torch
import torch.nn.functional as F

from oracle import sd_oracle as O

MAX_OBJS = 30


def fourier_embed(boxes, freqs=8):
    """[upstream-knowledge] emb_f = 100 ** (f / freqs); stack(sin, cos) of emb_f * box[k], permuted to flat index f * 8 + s * 4 + k."""
    b, n = boxes.shape[:2]
    emb = 100 ** (torch.arange(freqs, dtype=torch.float32) / freqs)
    emb = emb[None, None, None] * boxes.unsqueeze(-1)             # b, n, 4, freqs
    emb = torch.stack((emb.sin(), emb.cos()), dim=-1)             # b, n, 4, freqs, 2
    return emb.permute(0, 1, 3, 4, 2).reshape(b, n, freqs * 2 * 4)


def position_net(sd, boxes, masks, pos, freqs=8):
    """PositionNet.forward: null replacement of the phrase and box features by the mask, then Linear -> SiLU -> Linear -> SiLU -> Linear."""
    p = "position_net."
    m = masks.unsqueeze(-1)
    xyxy = fourier_embed(boxes, freqs)
    pos = pos * m + (1 - m) * sd[p + "null_positive_feature"].view(1, 1, -1)
    xyxy = xyxy * m + (1 - m) * sd[p + "null_position_feature"].view(1, 1, -1)
    h = torch.cat([pos, xyxy], -1)
    h = F.silu(F.linear(h, sd[p + "linears.0.weight"], sd[p + "linears.0.bias"]))
    h = F.silu(F.linear(h, sd[p + "linears.2.weight"], sd[p + "linears.2.bias"]))
    return F.linear(h, sd[p + "linears.4.weight"], sd[p + "linears.4.bias"])


def fuser(sd, pre, x, objs, heads, keep_objs=True):
    """GatedSelfAttentionDense.forward on x [B, N, C] (pre = the transformer block prefix).  keep_objs=False drops the grounding tokens
    from the attention (for the test that they matter)."""
    f = pre + "transformer_blocks.0.fuser."
    c, n = x.shape[-1], x.shape[1]
    o = F.linear(objs, sd[f + "linear.weight"], sd[f + "linear.bias"])
    xo = torch.cat([x, o], 1) if keep_objs else x
    a = F.layer_norm(xo, (c,), sd[f + "norm1.weight"], sd[f + "norm1.bias"], 1e-5)
    a = O.explicit_attention_processor(a, None, sd[f + "attn.to_q.weight"], sd[f + "attn.to_k.weight"], sd[f + "attn.to_v.weight"],
                                       sd[f + "attn.to_out.0.weight"], sd[f + "attn.to_out.0.bias"], heads)[:, :n]
    x = x + torch.tanh(sd[f + "alpha_attn"]) * a
    h = F.linear(F.layer_norm(x, (c,), sd[f + "norm2.weight"], sd[f + "norm2.bias"], 1e-5), sd[f + "ff.net.0.proj.weight"], sd[f + "ff.net.0.proj.bias"])
    val, gate = h.chunk(2, dim=-1)
    return x + torch.tanh(sd[f + "alpha_dense"]) * F.linear(val * F.gelu(gate), sd[f + "ff.net.2.weight"], sd[f + "ff.net.2.bias"])


def transformer_2d(x, ctx, sd, pre, heads, groups, linear_proj, objs, recorder=None, layer_name=""):
    """oracle.sd_oracle.transformer_2d with the fuser between attn1's residual add and norm2 (objs None: no fuser)."""
    b, c, hh, ww = x.shape
    res = x
    h = O._gn(x, sd, pre + "norm", groups, 1e-6)
    if not linear_proj:
        h = F.conv2d(h, sd[pre + "proj_in.weight"], sd[pre + "proj_in.bias"]).permute(0, 2, 3, 1).reshape(b, hh * ww, c)
    else:
        h = F.linear(h.permute(0, 2, 3, 1).reshape(b, hh * ww, c), sd[pre + "proj_in.weight"], sd[pre + "proj_in.bias"])
    t = pre + "transformer_blocks.0."
    n1 = F.layer_norm(h, (c,), sd[t + "norm1.weight"], sd[t + "norm1.bias"], 1e-5)
    h = h + O.explicit_attention_processor(n1, None, sd[t + "attn1.to_q.weight"], sd[t + "attn1.to_k.weight"], sd[t + "attn1.to_v.weight"],
                                           sd[t + "attn1.to_out.0.weight"], sd[t + "attn1.to_out.0.bias"], heads)
    if objs is not None:
        h = fuser(sd, pre, h, objs, heads)
    n2 = F.layer_norm(h, (c,), sd[t + "norm2.weight"], sd[t + "norm2.bias"], 1e-5)
    rec = (lambda p, nh: recorder(p, nh, layer_name)) if recorder is not None else None
    h = h + O.explicit_attention_processor(n2, ctx, sd[t + "attn2.to_q.weight"], sd[t + "attn2.to_k.weight"], sd[t + "attn2.to_v.weight"],
                                           sd[t + "attn2.to_out.0.weight"], sd[t + "attn2.to_out.0.bias"], heads, recorder=rec)
    n3 = F.layer_norm(h, (c,), sd[t + "norm3.weight"], sd[t + "norm3.bias"], 1e-5)
    val, gate = F.linear(n3, sd[t + "ff.net.0.proj.weight"], sd[t + "ff.net.0.proj.bias"]).chunk(2, dim=-1)
    h = h + F.linear(val * F.gelu(gate), sd[t + "ff.net.2.weight"], sd[t + "ff.net.2.bias"])
    if not linear_proj:
        h = F.conv2d(h.reshape(b, hh, ww, c).permute(0, 3, 1, 2), sd[pre + "proj_out.weight"], sd[pre + "proj_out.bias"])
    else:
        h = F.linear(h, sd[pre + "proj_out.weight"], sd[pre + "proj_out.bias"]).reshape(b, hh, ww, c).permute(0, 3, 1, 2)
    return h + res


def unet_forward(sd, ucfg, x, t, ctx, objs=None, recorder=None):
    """UNet2DConditionModel.forward with cross_attention_kwargs={"gligen": ...}: the oracle's walk with every transformer block's fuser on
    `objs` (the PositionNet output); objs None is the oracle's UNet exactly."""
    t = torch.as_tensor(t, dtype=torch.float32)
    if objs is None:
        return O.unet_forward(sd, ucfg, x, t, ctx, recorder)
    boc, g = ucfg.block_out_channels, ucfg.norm_num_groups
    if t.ndim == 0:
        t = t[None].expand(x.shape[0])
    temb = O.timestep_embedding(t, boc[0])
    temb = F.linear(temb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    temb = F.linear(F.silu(temb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    h = F.conv2d(x, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    skips = [h]
    nlev = len(boc)
    tf = lambda h_, nm, heads: transformer_2d(h_, ctx, sd, nm, heads, g, ucfg.use_linear_projection, objs, recorder, nm + "transformer_blocks.0.attn2")
    for i in range(nlev):
        for j in range(ucfg.layers_per_block):
            h = O.resnet_block(h, temb, sd, f"down_blocks.{i}.resnets.{j}.", g, 1e-5)
            if ucfg.down_cross[i]:
                h = tf(h, f"down_blocks.{i}.attentions.{j}.", ucfg.num_heads[i])
            skips.append(h)
        if i != nlev - 1:
            h = F.conv2d(h, sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], sd[f"down_blocks.{i}.downsamplers.0.conv.bias"], stride=2, padding=1)
            skips.append(h)
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.0.", g, 1e-5)
    h = tf(h, "mid_block.attentions.0.", ucfg.num_heads[-1])
    h = O.resnet_block(h, temb, sd, "mid_block.resnets.1.", g, 1e-5)
    up_cross, rev_heads = tuple(reversed(ucfg.down_cross)), tuple(reversed(ucfg.num_heads))
    for i in range(nlev):
        for j in range(ucfg.layers_per_block + 1):
            h = torch.cat([h, skips.pop()], dim=1)
            h = O.resnet_block(h, temb, sd, f"up_blocks.{i}.resnets.{j}.", g, 1e-5)
            if up_cross[i]:
                h = tf(h, f"up_blocks.{i}.attentions.{j}.", rev_heads[i])
        if i != nlev - 1:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, sd[f"up_blocks.{i}.upsamplers.0.conv.weight"], sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], padding=1)
    h = F.silu(O._gn(h, sd, "conv_norm_out", g, 1e-5))
    return F.conv2d(h, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


def prepare_objects(boxes_list, emb_list, cross_dim, batch):
    """[upstream-knowledge] the pipeline's tensors for one layout (n boxes, their pooled embeddings [n, D]): zero beyond n, masks[:n] = 1,
    repeated over the batch, doubled for CFG with masks[:batch] = 0."""
    n = len(boxes_list)
    boxes = torch.zeros(MAX_OBJS, 4)
    emb = torch.zeros(MAX_OBJS, cross_dim)
    masks = torch.zeros(MAX_OBJS)
    if n:
        boxes[:n] = torch.tensor(boxes_list, dtype=torch.float32)
        emb[:n] = emb_list
        masks[:n] = 1
    boxes = boxes.unsqueeze(0).expand(batch, -1, -1).clone()
    emb = emb.unsqueeze(0).expand(batch, -1, -1).clone()
    masks = masks.unsqueeze(0).expand(batch, -1).clone()
    boxes, emb, masks = torch.cat([boxes] * 2), torch.cat([emb] * 2), torch.cat([masks] * 2)
    masks[: 2 * batch // 2] = 0
    return boxes, emb, masks


def num_grounding_steps(beta, n_evals):
    """[upstream-knowledge] int(gligen_scheduled_sampling_beta * len(timesteps)); len(timesteps) counts model evaluations."""
    return int(beta * n_evals)


def generate(usd, vsd, cfg, ctx, latents, objs2, steps, scheduler, beta=0.3, guidance=7.5, recorder=None):
    """The restated GLIGEN UNet (objs2: the PositionNet output for the 2B CFG rows) stepped by the oracle's DDIM / PNDM or the restated
    DPM-Solver++ 2M on the host; the fusers run on evaluations i < num_grounding_steps.  Returns (uint8 images, latents)."""
    import _dpm_restated as D
    s = cfg.sched

    def model(x, i, t, n):
        k = num_grounding_steps(beta, n)
        eps = unet_forward(usd, cfg.unet, torch.cat([x, x], 0), t, ctx, objs2 if i < k else None, recorder)
        eu, ec = eps.chunk(2)
        return eu + guidance * (ec - eu)

    with torch.no_grad():
        x = latents.clone().float()
        if scheduler == "dpm":
            _, x = D.sample(steps, False, s.prediction_type, lambda x_, i, t: model(x_, i, t, steps), x)
        else:
            sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
                   O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type))
            ts = sch.set_timesteps(steps)
            for i, t in enumerate(ts):
                x = sch.step(model(x, i, float(int(t)), len(ts)), int(t), x)
        img = O.postprocess_image(O.vae_decode(vsd, cfg.vae, x / cfg.vae.scaling_factor))
    return img, x
