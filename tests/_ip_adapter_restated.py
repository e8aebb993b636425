"""An fp32 restatement of the IP-Adapter [upstream-knowledge: the IP-Adapter paper and diffusers >= 0.24's ImageProjection and
IPAdapterAttnProcessor: out = to_out(attn(q, K_text, V_text) + scale * attn(q, to_k_ip(tokens), to_v_ip(tokens)))], written for this suite
from the published behaviour with explicit q / k / v (no pre-multiplication) and composed from oracle.sd_oracle's blocks.  Independent of
agenda_amd's implementation; the weights `ip` carry the file's own flat keys."""
import torch
import torch.nn.functional as F

from oracle import sd_oracle as O


def attn2_order(ucfg):
    """Transformer-block prefixes in diffusers' `unet.attn_processors` order: down blocks, up blocks, the mid block last."""
    n = len(ucfg.block_out_channels)
    up_cross = tuple(reversed(ucfg.down_cross))
    out = [f"down_blocks.{i}.attentions.{j}." for i in range(n) if ucfg.down_cross[i] for j in range(ucfg.layers_per_block)]
    out += [f"up_blocks.{i}.attentions.{j}." for i in range(n) if up_cross[i] for j in range(ucfg.layers_per_block + 1)]
    return out + ["mid_block.attentions.0."]


def file_index(ucfg, pre):
    """k = 2 i + 1 of the block's attn2 processor."""
    return 2 * attn2_order(ucfg).index(pre) + 1


def image_tokens(ip, image_embeds, cross_dim):
    """ImageProjection: LayerNorm(Linear(image_embeds).reshape(B, n_tok, cross_dim)), eps 1e-5."""
    w = ip["image_proj.proj.weight"]
    h = F.linear(image_embeds.to(w.dtype), w, ip["image_proj.proj.bias"])
    return F.layer_norm(h.reshape(image_embeds.shape[0], -1, cross_dim), (cross_dim,), ip["image_proj.norm.weight"], ip["image_proj.norm.bias"], 1e-5)


def cfg_embeds(pos):
    """[negative; positive] rows: the negative rows are zeros_like (their TOKENS are the projection of zeros, not zeros)."""
    return torch.cat([torch.zeros_like(pos), pos], 0)


def ip_branch(sd, ip, ucfg, pre, n2, tokens, heads):
    """to_out.weight . attn(to_q(n2), to_k_ip(tokens), to_v_ip(tokens)) -- no bias (to_out's bias belongs to the sum, added once)."""
    t, k = pre + "transformer_blocks.0.", file_index(ucfg, pre)
    return O.explicit_attention_processor(n2, tokens, sd[t + "attn2.to_q.weight"], ip[f"ip_adapter.{k}.to_k_ip.weight"],
                                          ip[f"ip_adapter.{k}.to_v_ip.weight"], sd[t + "attn2.to_out.0.weight"], None, heads)


def block(sd, ip, ucfg, pre, x, tokens, heads, scale):
    """x + scale * to_out.weight . attn_ip(norm2(x)) on x [B, N, C]: the image branch's whole contribution to the residual stream."""
    t, c = pre + "transformer_blocks.0.", x.shape[-1]
    n2 = F.layer_norm(x, (c,), sd[t + "norm2.weight"], sd[t + "norm2.bias"], 1e-5)
    return x + scale * ip_branch(sd, ip, ucfg, pre, n2, tokens, heads)


def transformer_2d(x, ctx, sd, ucfg, pre, heads, ip, tokens, scale, recorder=None, layer_name=""):
    """oracle.sd_oracle.transformer_2d with the decoupled image attention inside attn2."""
    groups, linear_proj = ucfg.norm_num_groups, ucfg.use_linear_projection
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
    n2 = F.layer_norm(h, (c,), sd[t + "norm2.weight"], sd[t + "norm2.bias"], 1e-5)
    rec = (lambda p, nh: recorder(p, nh, layer_name)) if recorder is not None else None
    a = O.explicit_attention_processor(n2, ctx, sd[t + "attn2.to_q.weight"], sd[t + "attn2.to_k.weight"], sd[t + "attn2.to_v.weight"],
                                       sd[t + "attn2.to_out.0.weight"], sd[t + "attn2.to_out.0.bias"], heads, recorder=rec)
    h = h + a + scale * ip_branch(sd, ip, ucfg, pre, n2, tokens, heads)
    n3 = F.layer_norm(h, (c,), sd[t + "norm3.weight"], sd[t + "norm3.bias"], 1e-5)
    val, gate = F.linear(n3, sd[t + "ff.net.0.proj.weight"], sd[t + "ff.net.0.proj.bias"]).chunk(2, dim=-1)
    h = h + F.linear(val * F.gelu(gate), sd[t + "ff.net.2.weight"], sd[t + "ff.net.2.bias"])
    if not linear_proj:
        h = F.conv2d(h.reshape(b, hh, ww, c).permute(0, 3, 1, 2), sd[pre + "proj_out.weight"], sd[pre + "proj_out.bias"])
    else:
        h = F.linear(h, sd[pre + "proj_out.weight"], sd[pre + "proj_out.bias"]).reshape(b, hh, ww, c).permute(0, 3, 1, 2)
    return h + res


def unet_forward(sd, ucfg, x, t, ctx, ip=None, tokens=None, scale=1.0, recorder=None):
    """UNet2DConditionModel.forward with the IP-Adapter processors installed (ip None: the oracle's UNet exactly)."""
    t = torch.as_tensor(t, dtype=torch.float32)
    if ip is None:
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
    tf = lambda h_, nm, heads: transformer_2d(h_, ctx, sd, ucfg, nm, heads, ip, tokens, scale, recorder, nm + "transformer_blocks.0.attn2")
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


def generate(usd, vsd, cfg, ctx, latents, ip, tokens2, scale, steps, scheduler, guidance=7.5, recorder=None, timesteps_from=0):
    """The restated UNet with the image branch (tokens2: the projected tokens of the 2B CFG rows) stepped by the oracle's DDIM / PNDM on the
    host.  timesteps_from: the first index of the DDIM schedule that runs (img2img's strength truncation).  Returns (uint8 images, latents)."""
    s = cfg.sched

    def model(x, t):
        eps = unet_forward(usd, cfg.unet, torch.cat([x, x], 0), t, ctx, ip, tokens2, scale, recorder)
        eu, ec = eps.chunk(2)
        return eu + guidance * (ec - eu)

    with torch.no_grad():
        x = latents.clone().float()
        sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
               O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type))
        ts = sch.set_timesteps(steps)
        for t in ts[timesteps_from:]:
            x = sch.step(model(x, float(int(t))), int(t), x)
        img = O.postprocess_image(O.vae_decode(vsd, cfg.vae, x / cfg.vae.scaling_factor))
    return img, x


def premultiplied(sd, ip, ucfg, pre, tokens, heads, dtype=torch.float64):
    """The pre-multiplied form of one block's image branch, exact in `dtype`: K'' [B][heads n_tok][C], cs, bs [B][heads n_tok], V'' [B][C][heads n_tok]
    with column (h, t) = h n_tok + t, such that  S = rstd (x K''^T - mu cs) + bs,  P = softmax over each head's n_tok columns,
    delta = P V''^T  equals  to_out.weight . attn_ip(norm2(x))."""
    t, k = pre + "transformer_blocks.0.", file_index(ucfg, pre)
    wq, wo = sd[t + "attn2.to_q.weight"].to(dtype), sd[t + "attn2.to_out.0.weight"].to(dtype)
    gamma, beta = sd[t + "norm2.weight"].to(dtype), sd[t + "norm2.bias"].to(dtype)
    tok = tokens.to(dtype)
    kk = F.linear(tok, ip[f"ip_adapter.{k}.to_k_ip.weight"].to(dtype))          # [B, n_tok, C]
    vv = F.linear(tok, ip[f"ip_adapter.{k}.to_v_ip.weight"].to(dtype))
    B, nt, C = kk.shape
    D = C // heads
    scale = D ** -0.5
    kh = kk.reshape(B, nt, heads, D).permute(0, 2, 1, 3)                        # [B, H, nt, D]
    vh = vv.reshape(B, nt, heads, D).permute(0, 2, 1, 3)
    wqh = wq.reshape(heads, D, C)                                               # rows (h, d)
    kpp = scale * torch.einsum("bhtd,hdc->bhtc", kh, wqh) * gamma               # [B, H, nt, C]
    cs = kpp.sum(-1)
    bs = scale * torch.einsum("bhtd,hd->bht", kh, (wq @ beta).reshape(heads, D))
    woh = wo.reshape(C, heads, D)
    vpp = torch.einsum("nhd,bhtd->bnht", woh, vh)                               # [B, C, H, nt]
    return kpp.reshape(B, heads * nt, C), cs.reshape(B, -1), bs.reshape(B, -1), vpp.reshape(B, C, heads * nt)


def premultiplied_delta(x, kpp, cs, bs, vpp, heads, eps=1e-5):
    """to_out.weight . attn_ip(norm2(x)) from the pre-multiplied matrices (x [B, N, C] raw rows, norm2 folded)."""
    mu = x.mean(-1, keepdim=True)
    rstd = (x.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    s = rstd * (torch.einsum("bnc,bkc->bnk", x, kpp) - mu * cs[:, None]) + bs[:, None]
    B, N, K = s.shape
    p = s.reshape(B, N, heads, K // heads).softmax(-1).reshape(B, N, K)
    return torch.einsum("bnk,bck->bnc", p, vpp)
