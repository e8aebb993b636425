"""An fp32 restatement of DeepCache [upstream-knowledge: Ma, Fang, Wang, "DeepCache: Accelerating Diffusion Models for Free", CVPR 2024; the
upstream DeepCacheSDHelper with skip_mode "uniform"; parity-unpinned -- the upstream package is not available to this suite], written for
this suite from the paper's description in this project's terms and composed from oracle.sd_oracle's blocks.  Independent of agenda_amd.

Skips are numbered in the order the down path makes them: s_0 = conv_in's output, s_1 .. s_lpb the layers of down block 0, then the
downsampler's, ...; U_k is the up layer that consumes s_k, so U_lpb .. U_0 are layers 0 .. lpb of the last up block.  A full evaluation is
the oracle's forward and leaves in `cache` the hidden state that entered U_{b+1}; a shallow evaluation at branch b runs conv_in, layers
0 .. b of down block 0, U_{b+1} .. U_0 on the cached hidden state, conv_norm_out and conv_out.  Evaluation i of a call is full iff
i % cache_interval == 0."""
import torch
import torch.nn.functional as F

from oracle import sd_oracle as O


def unet_forward(sd, ucfg, x, t, ctx, mode="full", branch=0, cache=None, recorder=None, freeu=None):
    """UNet2DConditionModel.forward with mode in {"full", "shallow"}.  full: the oracle's forward, operation for operation; with a `cache`
    dict given, cache["h"] becomes the hidden state entering layer lpb - branch - 1 of the last up block.  shallow: only the layers named
    above run, on cache["h"].  `recorder` sees exactly the attn2 calls that run.  freeu = (s1, s2, b1, b2) as tests/_freeu_restated.py."""
    assert mode in ("full", "shallow")
    boc, g, lpb = ucfg.block_out_channels, ucfg.norm_num_groups, ucfg.layers_per_block
    assert 0 <= branch <= lpb - 1, branch
    nlev = len(boc)
    j_enter = lpb - branch - 1

    def tr(h, nm, heads):
        return O.transformer_2d(h, ctx, sd, nm, heads, g, ucfg.use_linear_projection, recorder, nm + "transformer_blocks.0.attn2")

    if t.ndim == 0:
        t = t[None].expand(x.shape[0])
    temb = O.timestep_embedding(t, boc[0])
    temb = F.linear(temb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
    temb = F.linear(F.silu(temb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    h = F.conv2d(x, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    skips = [h]
    shallow = mode == "shallow"
    for i in range(nlev):
        for j in range(lpb):
            h = O.resnet_block(h, temb, sd, f"down_blocks.{i}.resnets.{j}.", g, 1e-5)
            if ucfg.down_cross[i]:
                h = tr(h, f"down_blocks.{i}.attentions.{j}.", ucfg.num_heads[i])
            skips.append(h)
            if shallow and i == 0 and j == branch:
                break
        if shallow:
            break
        if i != nlev - 1:
            h = F.conv2d(h, sd[f"down_blocks.{i}.downsamplers.0.conv.weight"], sd[f"down_blocks.{i}.downsamplers.0.conv.bias"], stride=2, padding=1)
            skips.append(h)
    if shallow:
        assert len(skips) == branch + 2
        h = cache["h"]
    else:
        h = O.resnet_block(h, temb, sd, "mid_block.resnets.0.", g, 1e-5)
        h = tr(h, "mid_block.attentions.0.", ucfg.num_heads[-1])
        h = O.resnet_block(h, temb, sd, "mid_block.resnets.1.", g, 1e-5)
    up_cross, rev_heads = tuple(reversed(ucfg.down_cross)), tuple(reversed(ucfg.num_heads))
    for i in range(nlev - 1 if shallow else 0, nlev):
        for j in range(j_enter if shallow else 0, lpb + 1):
            if not shallow and cache is not None and i == nlev - 1 and j == j_enter:
                cache["h"] = h
            sk = skips.pop()
            if freeu is not None:
                import _freeu_restated as FR
                h, sk = FR.apply_freeu(i, h, sk, *freeu)
            h = torch.cat([h, sk], dim=1)
            h = O.resnet_block(h, temb, sd, f"up_blocks.{i}.resnets.{j}.", g, 1e-5)
            if up_cross[i]:
                h = tr(h, f"up_blocks.{i}.attentions.{j}.", rev_heads[i])
        if i != nlev - 1:
            h = F.interpolate(h, scale_factor=2.0, mode="nearest")
            h = F.conv2d(h, sd[f"up_blocks.{i}.upsamplers.0.conv.weight"], sd[f"up_blocks.{i}.upsamplers.0.conv.bias"], padding=1)
    assert not skips
    h = F.silu(O._gn(h, sd, "conv_norm_out", g, 1e-5))
    return F.conv2d(h, sd["conv_out.weight"], sd["conv_out.bias"], padding=1)


def schedule(n_evaluations, cache_interval):
    """The uniform schedule: evaluation i is full iff i % cache_interval == 0."""
    return [i % cache_interval == 0 for i in range(n_evaluations)]


def shallow_attn2_layers(ucfg, branch):
    """attn2 layers a shallow evaluation runs: one per layer 0 .. b of down block 0 and one per up layer U_{b+1} .. U_0."""
    return (branch + 1 + branch + 2) if ucfg.down_cross[0] else 0


def generate(usd, vsd, cfg, ctx, latents, steps, scheduler, guidance=7.5, cache_interval=1, branch=0, recorder=None, freeu=None,
             ddim_start=0):
    """The oracle's UNet and VAE under DeepCache, stepped by the oracle's DDIM / PNDM or the restated DPM-Solver++ 2M.  ctx [2B,T,D] ordered
    [uncond x B | cond x B].  Evaluations count from 0 per call (PNDM's extra one included); ddim_start > 0 runs the tail of the DDIM grid
    from that index (img2img).  Returns (uint8 images, latents, (full evaluations followed by a shallow one, shallow evaluations))."""
    import _dpm_restated as R
    s = cfg.sched
    cache, n = {}, [0]
    kinds = []

    def model(x, t):
        full = n[0] % cache_interval == 0
        n[0] += 1
        kinds.append(full)
        tt = torch.as_tensor(t, dtype=torch.float32)
        eps = unet_forward(usd, cfg.unet, torch.cat([x, x], 0), tt, ctx, "full" if full else "shallow", branch, cache, recorder, freeu)
        e_u, e_c = eps.chunk(2)
        return e_u + guidance * (e_c - e_u)

    with torch.no_grad():
        x = latents.clone().float()
        if scheduler == "dpm":
            _, x = R.sample(steps, False, s.prediction_type, lambda x_, i, t: model(x_, t), x)
        else:
            sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
                   O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type))
            for t in list(sch.set_timesteps(steps))[ddim_start:]:
                x = sch.step(model(x, float(int(t))), int(t), x)
        img = O.postprocess_image(O.vae_decode(vsd, cfg.vae, x / cfg.vae.scaling_factor))
    captures = sum(1 for i in range(len(kinds) - 1) if kinds[i] and not kinds[i + 1])
    return img, x, (captures, sum(1 for k in kinds if not k))
