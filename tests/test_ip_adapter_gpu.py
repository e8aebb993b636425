"""The IP-Adapter on the device against the fp32 restatement (tests/_ip_adapter_restated.py): the projected tokens, one block's image branch
at every SD-1.5 width on square, rectangular and ragged maps (and the one-head 3 x 3 block of tiny21), one UNet forward, scale 0 / no image /
unloaded against the plain pipeline bit for bit, full tiny txt2img under DDIM and PNDM against a host-stepped loop, img2img, a rectangular
generate under trace, hook.py counts, the scale's monotone effect, the rebuild after a LoRA scale change, the CLI and the error statuses of
the new ABI; the image encoder's two synthetic towers against a restated tower, ip_adapter_image through it, and the safety checker's scores
against a recording of the build before its vision path was shared."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ip_adapter_restated as R
from _report import report
from agenda_amd import ip_adapter as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_TINY, E_SD15 = 96, 1024


def _rms(t):
    return float((t.detach().float().cpu() ** 2).mean().sqrt())


def _rms_rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _rel(got, want):
    got = got.detach().float().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _weights(cfg, small=True):
    from agenda_amd import synthetic
    kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
    return synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw), synthetic.make_vae_weights(cfg, 12 if small else 1235, **kw)


_CACHE = {}


def _model(name):
    """(cfg, unet weights, vae weights, adapter weights, embed_dim), built once per config and left unchanged."""
    if name not in _CACHE:
        from agenda_amd import config
        cfg = config.CONFIGS[name]()
        E = E_SD15 if name == "sd15" else E_TINY
        u, v = _weights(cfg, small=name != "sd15")
        _CACHE[name] = (cfg, u, v, A.make_ip_adapter_weights(cfg, 21, E), E)
    return _CACHE[name]


def _pipe(cfg, u, v, scheduler="DDIMScheduler", ws=2 << 30):
    from agenda_amd import StableDiffusionPipeline
    return StableDiffusionPipeline(cfg, u, v, workspace_bytes=ws, scheduler=scheduler)


def _embeds(n, E, seed):
    return torch.randn(n, E, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).float()


@pytest.mark.parametrize("name", ["tiny", "sd15"])
def test_tokens_match_image_projection(name):
    cfg, u, v, ip, E = _model(name)
    pipe = _pipe(cfg, u, v, ws=1 << 30)
    pipe.load_ip_adapter(ip)
    emb = R.cfg_embeds(_embeds(2, E, 5))
    pipe.engine.ip_adapter_set(emb, 1.0)
    got = pipe.engine.ip_adapter_tokens().cpu()
    want = R.image_tokens(ip, emb, cfg.unet.cross_attention_dim)
    e = _rms_rel(got, want)
    print(f"ip-adapter tokens {name}: rms rel {e:.5f}; negative-row token rms {_rms(got[:2]):.3f}")
    report(f"ip_adapter_tokens[{name}]", rms_rel=e)
    assert got.shape == (4, 4, cfg.unet.cross_attention_dim)
    assert e < 0.01, e
    assert _rms(got[:2]) > 0.1                                   # the projection of zeros is not zero tokens
    pipe.engine.close()


BLOCK_CASES = [("sd15", "down_blocks.0.attentions.0.", 320, 8, 8), ("sd15", "down_blocks.1.attentions.1.", 640, 16, 8),
               ("sd15", "up_blocks.1.attentions.2.", 1280, 8, 8), ("sd15", "up_blocks.3.attentions.0.", 320, 12, 20),
               ("sd15", "mid_block.attentions.0.", 1280, 4, 6),    # HW = 24: no multiple of 16, images meet inside a 64-row tile
               ("tiny21", "down_blocks.0.attentions.0.", 64, 3, 3)]  # one head, HW = 9


@pytest.mark.parametrize("name", ["sd15", "tiny21"])
def test_block_matches_restatement_and_images_do_not_share_weights(name):
    cfg, u, v, ip, E = _model(name)
    pipe = _pipe(cfg, u, v, ws=1 << 30)
    pipe.load_ip_adapter(ip)
    B2 = 4
    pos = _embeds(2, E, 9)
    emb, emb_sw = R.cfg_embeds(pos), R.cfg_embeds(pos.flip(0))      # rows 0, 1 the negative half; rows 2, 3 swapped in emb_sw
    tok, tok_sw = (R.image_tokens(ip, e_, cfg.unet.cross_attention_dim) for e_ in (emb, emb_sw))
    for nm, pre, C, h, w in BLOCK_CASES:
        if nm != name:
            continue
        heads = cfg.unet.num_heads[0] if name == "tiny21" else 8
        x = torch.randn(B2, h * w, C, generator=torch.Generator().manual_seed(C + h)).to(torch.bfloat16).float()
        pipe.engine.ip_adapter_set(emb, 1.0)
        got = pipe.engine.ip_adapter_block(pre, x, h, w).cpu()
        pipe.engine.ip_adapter_set(emb_sw, 1.0)
        got_sw = pipe.engine.ip_adapter_block(pre, x, h, w).cpu()
        want, want_sw = R.block(u, ip, cfg.unet, pre, x, tok, heads, 1.0), R.block(u, ip, cfg.unet, pre, x, tok_sw, heads, 1.0)
        e, e_neg, e_sw = _rms_rel(got - x, want - x), _rms_rel(got[:2] - x[:2], want[:2] - x[:2]), _rms_rel(got_sw - x, want_sw - x)
        err, delta, swap = _rms(got - want), _rms(got - x), _rms(got_sw - got)
        print(f"ip-adapter block {pre} C={C} {h}x{w}: delta rms rel {e:.4f} (negative rows {e_neg:.4f}, swapped {e_sw:.4f}); "
              f"|delta| {delta:.4f}, |error| {err:.5f}, |swap effect| {swap:.4f}")
        report(f"ip_adapter_block[{pre}{h}x{w}]", delta_rms_rel=e, negative_rows=e_neg, swapped=e_sw, delta=delta, error=err, swap_effect=swap)
        assert e < 0.02 and e_neg < 0.02 and e_sw < 0.02, (pre, e, e_neg, e_sw)
        assert delta > 10 * err, (pre, delta, err)                  # a stage that does nothing fails
        assert swap > 10 * err, (pre, swap, err)                    # per-image weights shared between the images fail
    pipe.engine.close()


@pytest.mark.parametrize("name,L,B2", [("tiny", 16, 2), ("tiny21", 24, 2)])
def test_unet_forward_matches_restatement(name, L, B2):
    from agenda_amd import synthetic
    cfg, u, v, ip, E = _model(name)
    pipe = _pipe(cfg, u, v)
    pipe.load_ip_adapter(ip)
    ctx = synthetic.make_context(cfg, B2 // 2, seed=3)
    x = torch.randn(B2, 4, L, L, generator=torch.Generator().manual_seed(4))
    emb = R.cfg_embeds(_embeds(B2 // 2, E, 6))
    e = pipe.engine
    e.set_context(ctx)
    e.ip_adapter_set(emb, 1.0)
    got = e.unet_forward(x.cuda(), 401.0).cpu()
    counts = e.ip_adapter_counts()
    e.ip_adapter_clear()
    plain = e.unet_forward(x.cuda(), 401.0).cpu()
    tok = R.image_tokens(ip, emb, cfg.unet.cross_attention_dim)
    with torch.no_grad():
        want = R.unet_forward(u, cfg.unet, x, 401.0, ctx, ip, tok, 1.0)
        want_plain = R.unet_forward(u, cfg.unet, x, 401.0, ctx)
    err, err_plain, effect = _rms_rel(got, want), _rms_rel(plain, want_plain), _rms_rel(want_plain, want)
    print(f"ip-adapter unet {name} L={L}: rms rel {err:.4f}, plain {err_plain:.4f}, adapter effect {effect:.4f}; launches {counts}")
    report(f"ip_adapter_unet[{name}]", rms_rel=err, plain_rms_rel=err_plain, effect=effect)
    n_blocks = len(A.attn2_blocks(cfg.unet))
    assert counts == (n_blocks, n_blocks), counts
    assert err < 0.03 and err_plain < 0.03, (err, err_plain)
    assert effect > 3 * err, (effect, err)
    pipe.engine.close()


def _gen(pipe, ctx, lat, steps, **kw):
    from agenda_amd import trace
    B = lat.shape[0]
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="np", **kw)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    return out, hm


@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "DPMSolverMultistepScheduler"])
def test_idle_adapter_is_bit_identical_to_the_plain_pipeline(scheduler):
    from agenda_amd import synthetic
    cfg, u, v, ip, E = _model("tiny")
    B, L, steps = 2, 16, 5
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    pp = _pipe(cfg, u, v, scheduler=scheduler)
    ref, rhm = _gen(pp, ctx, lat, steps)
    pp.engine.close()
    pipe = _pipe(cfg, u, v, scheduler=scheduler)
    pipe.load_ip_adapter(ip)
    emb = _embeds(B, E, 8)
    pipe.set_ip_adapter_scale(0.0)
    runs = {"scale 0": _gen(pipe, ctx, lat, steps, ip_adapter_image_embeds=emb)}
    assert pipe.engine.ip_adapter_counts() == (0, 0)
    pipe.set_ip_adapter_scale(1.0)
    runs["no image"] = _gen(pipe, ctx, lat, steps)
    assert pipe.engine.ip_adapter_counts() == (0, 0)
    live = _gen(pipe, ctx, lat, steps, ip_adapter_image_embeds=emb)[0]
    assert pipe.engine.ip_adapter_counts()[0] > 0
    assert not torch.equal(live.latents.cpu(), ref.latents.cpu())
    pipe.unload_ip_adapter()
    runs["unloaded"] = _gen(pipe, ctx, lat, steps)
    pipe.engine.close()
    for what, (out, hm) in runs.items():
        assert torch.equal(out.latents.cpu(), ref.latents.cpu()), what
        assert np.array_equal(out.images, ref.images), what
        assert torch.equal(hm, rhm), what


@pytest.mark.parametrize("scheduler,key,steps", [("DDIMScheduler", "ddim", 4), ("PNDMScheduler", "pndm", 3)])
def test_pipeline_matches_host_stepped_restatement(scheduler, key, steps):
    """16 x 16 latent, 4 model evaluations (PLMS at 3 steps evaluates 4 times)."""
    from agenda_amd import synthetic
    from agenda_amd.controlnet import evaluation_count
    from oracle import sd_oracle as O
    cfg, u, v, ip, E = _model("tiny")
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    emb = _embeds(B, E, 10)
    pipe = _pipe(cfg, u, v, scheduler=scheduler)
    pipe.load_ip_adapter(ip)
    out, hm = _gen(pipe, ctx, lat, steps, ip_adapter_image_embeds=emb)
    evals = evaluation_count(pipe.scheduler, steps)
    pipe.engine.close()
    tok2 = R.image_tokens(ip, R.cfg_embeds(emb), cfg.unet.cross_attention_dim)
    rec = O.DaamRecorder(L * L, context_size=cfg.max_tokens)
    want_img, want_lat = R.generate(u, v, cfg, ctx, lat, ip, tok2, 1.0, steps, key, recorder=rec)
    whm = rec.compute_global_heat_map()
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(hm, whm)
    print(f"ip-adapter pipe {key}: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map rel {e_hm:.4f}")
    report(f"ip_adapter_pipeline[{key}]", latents_rms_rel=e_lat, psnr_db=psnr, heat_map_rel=e_hm)
    assert evals == 4
    assert e_lat < 0.06, e_lat
    assert psnr > 30.0, psnr
    assert e_hm < 0.06, e_hm
    assert float(hm.sum(1).mean()) == pytest.approx(evals, rel=0.02)      # the image branch records nothing: one map per evaluation


def test_img2img_matches_host_stepped_restatement():
    from agenda_amd import synthetic
    cfg, u, v, ip, E = _model("tiny")
    B, L, steps, strength = 1, 16, 6, 0.5
    ctx = synthetic.make_context(cfg, B, seed=45)
    g = torch.Generator().manual_seed(3)
    image = torch.rand(B, 3, L * 8, L * 8, generator=g) * 2 - 1
    noise_enc, noise = torch.randn(B, 4, L, L, generator=g), torch.randn(B, 4, L, L, generator=g)
    emb = _embeds(B, E, 11)
    v = synthetic.make_vae_weights(cfg, 12, bias_std=0.05, perturb_norm=0.1, with_encoder=True)      # (the decoder's weights are _model's)
    pipe = _pipe(cfg, u, v)
    pipe.load_ip_adapter(ip)
    kw = dict(prompt_embeds=ctx, image=image, strength=strength, num_inference_steps=steps, noise_enc=noise_enc, noise=noise, output_type="latent")
    got = pipe.img2img(ip_adapter_image_embeds=emb, **kw).latents.cpu()
    plain = pipe.img2img(**kw).latents.cpu()
    # the call's initial latents, as img2img draws them (the VAE encode is the engine's: the loop is what this test compares)
    ts = pipe.scheduler.set_timesteps(steps)
    t0 = steps - int(steps * strength)
    mean, logvar = pipe.engine.vae_encode(image)
    x0 = ((mean + torch.exp(0.5 * logvar) * noise_enc.to(mean.device)) * cfg.vae.scaling_factor).cpu()
    a = float(pipe.scheduler.alphas_cumprod[int(ts[t0])])
    lat0 = a ** 0.5 * x0 + (1 - a) ** 0.5 * noise
    pipe.engine.close()
    tok2 = R.image_tokens(ip, R.cfg_embeds(emb), cfg.unet.cross_attention_dim)
    _, want = R.generate(u, v, cfg, ctx, lat0, ip, tok2, 1.0, steps, "ddim", timesteps_from=t0)
    e, effect = _rms_rel(got, want), _rms_rel(plain, got)
    print(f"ip-adapter img2img: latents rms rel {e:.4f}; adapter effect {effect:.4f}")
    report("ip_adapter_img2img", latents_rms_rel=e, effect=effect)
    assert e < 0.06, e
    assert effect > 3 * e, (effect, e)


def test_rectangular_generate_under_trace():
    from agenda_amd import synthetic
    cfg, u, v, ip, E = _model("tiny")
    B, Lh, Lw, steps = 1, 16, 24, 3
    ctx = synthetic.make_context(cfg, B, seed=46)
    lat = torch.randn(B, 4, Lh, Lw, generator=torch.Generator().manual_seed(12))
    emb = _embeds(B, E, 13)
    pipe = _pipe(cfg, u, v)
    pipe.load_ip_adapter(ip)
    out, hm = _gen(pipe, ctx, lat, steps, height=Lh * 8, width=Lw * 8, ip_adapter_image_embeds=emb)
    pipe.engine.close()
    tok2 = R.image_tokens(ip, R.cfg_embeds(emb), cfg.unet.cross_attention_dim)
    _, want = R.generate(u, v, cfg, ctx, lat, ip, tok2, 1.0, steps, "ddim")
    e = _rms_rel(out.latents, want)
    print(f"ip-adapter rectangular {Lh}x{Lw}: latents rms rel {e:.4f}")
    report("ip_adapter_rectangular", latents_rms_rel=e)
    assert tuple(hm.shape[-2:]) == (Lh, Lw) and out.images.shape[1:3] == (Lh * 8, Lw * 8)          # rectangular maps at the latent size
    assert float(hm.sum(1).mean()) == pytest.approx(steps, rel=0.02)
    assert e < 0.06, e


def test_hook_counts_stay_and_scale_is_monotone():
    from agenda_amd import UNetCrossAttentionHooker, synthetic
    cfg, u, v, ip, E = _model("tiny")
    B, L, steps = 2, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=43)
    lat = synthetic.make_latents(cfg, [6, 7], L)
    emb = _embeds(B, E, 14)
    pipe = _pipe(cfg, u, v)
    pipe.load_ip_adapter(ip)
    res = {}
    for on in (False, True):
        hk = UNetCrossAttentionHooker(is_train=False, latent_hw=L)
        pipe.unet.set_attn_processor(hk)
        try:
            out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", ip_adapter_image_embeds=emb if on else None)
            res[on] = (out.latents.cpu(), pipe.engine.hook_count(), hk.compute_global_heat_map().cpu())
        finally:
            pipe.unet.set_attn_processor("default")
    assert res[False][1] == res[True][1] and res[True][1] > 0          # the image branch records nothing
    assert res[False][2].shape == res[True][2].shape
    assert _rms_rel(res[True][0], res[False][0]) > 0.01
    plain = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent").latents.cpu()
    dist = []
    for s in (0.25, 0.5, 1.0):
        pipe.set_ip_adapter_scale(s)
        dist.append(_rms_rel(pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", ip_adapter_image_embeds=emb).latents.cpu(), plain))
    pipe.engine.close()
    print(f"ip-adapter scale 0.25 / 0.5 / 1.0: distance from the plain latents {dist[0]:.4f} / {dist[1]:.4f} / {dist[2]:.4f}")
    assert 0 < dist[0] < dist[1] < dist[2], dist


def test_lora_scale_change_rebuilds_the_image_products():
    from agenda_amd import _lib, synthetic
    from test_lora_gpu import _kohya
    cfg, u, v, ip, E = _model("tiny")
    B, L, steps = 1, 16, 3
    ctx = synthetic.make_context(cfg, B, seed=47)
    lat = synthetic.make_latents(cfg, [8], L)
    emb = _embeds(B, E, 15)
    lora = _kohya(cfg, 4, 5, text=False)
    kw = dict(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", ip_adapter_image_embeds=emb)

    def fresh():
        p = _pipe(cfg, u, v)
        p.load_lora_weights(lora)
        p.load_ip_adapter(ip)
        return p

    a = fresh()
    first = a(cross_attention_kwargs={"scale": 0.5}, **kw).latents.cpu()
    second = a(cross_attention_kwargs={"scale": 1.0}, **kw).latents.cpu()
    # the engine's own forward after a scale change, without a new agd_ip_adapter_set: refused as stale
    a.engine.lora_set_scale(0.25)
    a.engine.set_context(ctx)
    with pytest.raises(_lib.AgendaHipError, match="agd_ip_adapter_set"):
        a.engine.unet_forward(torch.randn(2, 4, L, L).cuda(), 11.0)
    a.engine.close()
    b = fresh()
    want = b(cross_attention_kwargs={"scale": 1.0}, **kw).latents.cpu()
    b.engine.close()
    assert not torch.equal(first, second)
    assert torch.equal(second, want)


def test_error_statuses():
    from agenda_amd import _lib, synthetic
    cfg, u, v, ip, E = _model("tiny")
    pipe = _pipe(cfg, u, v, ws=1 << 30)
    e, lib, c = pipe.engine, pipe.engine.lib, pipe.engine.ctx
    err = lambda: lib.agd_last_error(c)
    emb = R.cfg_embeds(_embeds(1, E, 1))
    with pytest.raises(_lib.AgendaHipError, match="no IP-Adapter loaded"):
        e.ip_adapter_set(emb, 1.0)
    assert lib.agd_ip_adapter_tokens(c, None) != 0 and b"no image tokens" in err()
    assert lib.agd_ip_adapter_commit(c) != 0 and b"agd_ip_adapter_begin" in err()
    assert lib.agd_ip_adapter_tensor(c, b"image_proj.proj.bias", None, 0, 1, None) != 0 and b"agd_ip_adapter_begin" in err()
    assert lib.agd_ip_adapter_begin(c, 0, 4) != 0 and b"embed_dim" in err()
    assert lib.agd_ip_adapter_begin(c, E, 64) != 0 and b"n_tokens" in err()
    assert lib.agd_ip_adapter_counts(c, None) != 0
    tensors, _, _ = A.to_engine_tensors(ip, cfg)
    missing = {k: t for k, t in tensors.items() if "mid_block" not in k}
    with pytest.raises(_lib.AgendaHipError, match=r"mid_block\.attentions\.0\.transformer_blocks\.0\.attn2\.to_k_ip\.weight \(missing\)"):
        e.ip_adapter_load(missing, E, 4)
    bad = dict(tensors)
    bad["image_proj.norm.weight"] = torch.ones(cfg.unet.cross_attention_dim + 1)
    with pytest.raises(_lib.AgendaHipError, match=r"image_proj\.norm\.weight \(\[65\], expected \[64\]\)"):
        e.ip_adapter_load(bad, E, 4)
    with pytest.raises(_lib.AgendaHipError, match="not an IP-Adapter tensor"):
        e.ip_adapter_load({"image_proj.other": torch.ones(3)}, E, 4)
    e.ip_adapter_load(tensors, E, 4)                               # (every failed load above unloaded itself)
    with pytest.raises(_lib.AgendaHipError, match="already loaded"):
        e.ip_adapter_load(tensors, E, 4)
    assert lib.agd_ip_adapter_set(c, None, 2, 1.0, None) != 0 and b"bad arguments" in err()
    with pytest.raises(_lib.AgendaHipError, match="scale"):
        e.ip_adapter_set(emb, float("nan"))
    x = torch.randn(2, 4 * 4, 64)
    with pytest.raises(_lib.AgendaHipError, match="no image tokens"):
        e.ip_adapter_block("down_blocks.0.attentions.0.", x, 4, 4)
    e.ip_adapter_set(emb, 1.0)
    with pytest.raises(_lib.AgendaHipError, match="no attn2 layer in block"):
        e.ip_adapter_block("down_blocks.3.attentions.0.", x, 4, 4)
    with pytest.raises(_lib.AgendaHipError, match="set for 2 rows"):
        e.ip_adapter_block("down_blocks.0.attentions.0.", torch.randn(4, 16, 64), 4, 4)
    assert lib.agd_ip_adapter_block(c, None, None, 2, 4, 4, None, None) != 0 and b"bad arguments" in err()
    # forwards the image branch does not serve, each refused by name before anything runs
    e.set_context(synthetic.make_context(cfg, 2, seed=2))
    with pytest.raises(_lib.AgendaHipError, match="set for 2 rows, this call runs 4"):
        e.unet_forward(torch.randn(4, 4, 16, 16).cuda(), 11.0)
    e.set_context(synthetic.make_context(cfg, 1, seed=2))
    ts = (torch.tensor([11.0, 12.0]).numpy()).astype(np.float32)
    import ctypes
    xs, out = torch.randn(2, 4, 16, 16).cuda(), torch.empty(2, 4, 16, 16).cuda()
    rc = lib.agd_unet_forward_ts(c, _lib.ptr(xs), 2, 16, ts.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _lib.ptr(out), None)
    assert rc != 0 and b"unet_forward_ts: an IP-Adapter image is set" in err()
    pipe.scheduler.set_timesteps(2)
    a_t, a_p = pipe.scheduler.step_coeffs()
    with pytest.raises(_lib.AgendaHipError, match="denoise_panorama: an IP-Adapter image is set"):
        e.denoise_panorama(torch.randn(1, 4, 16, 32).cuda(), 16, 8, None, pipe.scheduler.timesteps, a_t, a_p, 7.5)
    e.ip_adapter_clear()
    assert e.ip_adapter_counts() == (0, 0)
    e.ip_adapter_unload()
    with pytest.raises(_lib.AgendaHipError, match="no IP-Adapter loaded"):
        e.ip_adapter_set(emb, 1.0)
    e.close()


TOWER = dict(num_hidden_layers=2, image_size=28, size=28, crop_size=28, patch_size=14, projection_dim=64)
TOWERS = {"d64": dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, **TOWER),
          "d80": dict(hidden_size=320, num_attention_heads=4, intermediate_size=640, **TOWER)}


def _images(n, h, w, seed):
    """Random uint8 images over a per-image colour ramp (the generator the stored safety recording was made with)."""
    rng = np.random.default_rng(seed)
    ry, rx = np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32)
    out = []
    for _ in range(n):
        base = rng.uniform(0, 255, 3) * ry[:, None, None] + rng.uniform(0, 255, 3) * rx[None, :, None] * (1 - ry[:, None, None])
        out.append(np.clip(base + rng.normal(0, 40, (h, w, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


@pytest.mark.parametrize("name", ["d64", "d80"])
def test_image_embeds_match_a_restated_tower(name):
    """Two layers, image 28, patch 14 (T = 5), projection 64, head dim 64 and 80, against transformers' CLIPVisionModel + projection;
    the bound is the one test_safety_gpu holds the small tower's embeddings to (2^-6 rel-rms)."""
    from _safety_restated import hf_tower, preprocess
    cfg, u, v, ip, E = _model("tiny")
    scfg = A.image_encoder_config(**TOWERS[name])
    esd = A.make_image_encoder_weights(scfg, 17)
    pipe = _pipe(cfg, u, v, ws=1 << 30)
    pipe.load_image_encoder(scfg, esd)
    im = _images(3, 64, 64, 7)
    got = pipe.engine.image_embeds(torch.from_numpy(im)).cpu()
    pipe.engine.close()
    checker_keys = {("vision_model." + k if k.startswith("vision_model.") else k): t for k, t in esd.items()}
    want = hf_tower(scfg, checker_keys)(torch.from_numpy(preprocess(im, size=28)))
    e, e_n = _rms_rel(got, want), _rms_rel(torch.nn.functional.normalize(got), torch.nn.functional.normalize(want))
    print(f"image encoder {name}: embeds rel-rms {e:.5f}, normalised {e_n:.5f}")
    report(f"image_embeds[{name}]", rms_rel=e, normalised_rms_rel=e_n)
    assert got.shape == (3, 64)
    assert e <= 2.0 ** -6 and e_n <= 2.0 ** -6, (e, e_n)


def test_safety_scores_are_bit_identical_to_the_recording_of_the_parent_build():
    """tests/golden/safety_scores_parent.npz holds agd_safety_scores_hw of the build BEFORE the vision path was factored into the helper the
    image encoder shares, on these inputs: written by tools/record_safety_scores.py in a checkout of commit 6d8f2a9, built for gfx950 and
    run on one MI355X (safety weights seed 21; images seed 31, 2 of 160 x 208, and seed 32, 3 of 224 x 224).  It is a committed file because
    a test session has no history to build that commit from; the script remakes it there."""
    from agenda_amd import StableDiffusionPipeline, config, synthetic
    rec = np.load(os.path.join(ROOT, "tests", "golden", "safety_scores_parent.npz"))
    cfg = config.tiny()
    cfg.safety = config.SafetyConfig(n_special=3, n_concepts=17, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                                     projection_dim=64)
    pipe = StableDiffusionPipeline(cfg, synthetic.make_unet_weights(cfg), synthetic.make_vae_weights(cfg), safety_sd=synthetic.make_safety_weights(cfg, 21),
                                   workspace_bytes=1 << 30)
    for name, (n, h, w, seed) in {"rect": (2, 160, 208, 31), "square": (3, 224, 224, 32)}.items():
        cos, pix = pipe.safety_checker.scores(torch.from_numpy(_images(n, h, w, seed)).cuda(), pixels=True)
        assert np.array_equal(cos.cpu().numpy(), rec[name + "_cos"]), name
        assert np.array_equal(pix.double().sum(dim=(1, 2, 3)).cpu().numpy(), rec[name + "_pix_sum"]), name
    pipe.engine.close()


def test_ip_adapter_image_runs_the_encoder_and_equals_its_embeddings():
    from agenda_amd import _lib, synthetic
    cfg, u, v, ip, E = _model("tiny")
    scfg = A.image_encoder_config(**{**TOWERS["d64"], "projection_dim": E})
    B, L, steps = 2, 16, 2
    ctx = synthetic.make_context(cfg, B, seed=48)
    lat = synthetic.make_latents(cfg, [2, 3], L)
    pipe = _pipe(cfg, u, v)
    pipe.load_ip_adapter(ip)
    im = torch.from_numpy(_images(1, 48, 80, 9))
    kw = dict(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent")
    with pytest.raises(ValueError, match="no image encoder is loaded"):
        pipe(ip_adapter_image=im, **kw)
    pipe.load_image_encoder(scfg, A.make_image_encoder_weights(scfg, 18))
    a = pipe(ip_adapter_image=im, **kw).latents.cpu()                       # one image serves both prompts
    emb = pipe.engine.image_embeds(im).cpu()
    b = pipe(ip_adapter_image_embeds=emb, **kw).latents.cpu()
    plain = pipe(**kw).latents.cpu()
    assert torch.equal(a, b) and not torch.equal(a, plain)
    e, lib, c = pipe.engine, pipe.engine.lib, pipe.engine.ctx
    assert lib.agd_image_embeds(c, None, 1, 8, 8, None, None) != 0 and b"null buffer" in lib.agd_last_error(c)
    assert lib.agd_image_encoder_commit(c) != 0 and b"agd_image_encoder_begin" in lib.agd_last_error(c)
    with pytest.raises(_lib.AgendaHipError, match="already loaded"):
        e.image_encoder_load(scfg, {})
    e.close()
    p2 = _pipe(cfg, u, v, ws=1 << 30)
    with pytest.raises(_lib.AgendaHipError, match="no image encoder loaded"):
        p2.engine._ienc_cfg = scfg
        p2.engine.image_embeds(im)
    p2.engine._ienc_cfg = None
    bad = A.image_encoder_config(**{**TOWERS["d64"], "num_attention_heads": 4})          # head dim 32
    with pytest.raises(_lib.AgendaHipError, match="head dim 32 unsupported"):
        p2.engine.image_encoder_load(bad, {})
    short = dict(A.make_image_encoder_weights(scfg, 18))
    short["visual_projection.weight"] = torch.zeros(E + 1, 128)
    with pytest.raises(_lib.AgendaHipError, match="visual_projection.weight' has"):
        p2.engine.image_encoder_load(scfg, short)
    # the refused load unloaded itself: the same context takes the right weights next, and computes what the first pipeline did
    p2.load_image_encoder(scfg, A.make_image_encoder_weights(scfg, 18))
    assert torch.equal(p2.engine.image_embeds(im).cpu(), emb)
    p2.unload_image_encoder()
    with pytest.raises(_lib.AgendaHipError, match="no image encoder loaded"):
        p2.engine.image_embeds(im)
    assert p2.engine.lib.agd_image_encoder_unload(None) != 0
    p2.engine.close()


def test_an_encoder_the_engine_refuses_leaves_no_adapter_behind(tmp_path):
    from agenda_amd import _lib
    cfg, u, v, ip, E = _model("tiny")
    bad = A.image_encoder_config(**{**TOWERS["d64"], "num_attention_heads": 4, "projection_dim": E})     # head dim 32: the engine's refusal
    folder = A.write_image_encoder(str(tmp_path / "image_encoder"), bad, A.make_image_encoder_weights(bad, 19))
    pipe = _pipe(cfg, u, v, ws=1 << 30)
    with pytest.raises(_lib.AgendaHipError, match="head dim 32 unsupported"):
        pipe.load_ip_adapter(ip, image_encoder_folder=folder)
    assert pipe._ip_adapter is None and pipe._image_encoder is None
    with pytest.raises(_lib.AgendaHipError, match="no IP-Adapter loaded"):
        pipe.engine.ip_adapter_set(R.cfg_embeds(_embeds(1, E, 1)), 1.0)
    pipe.load_ip_adapter(ip)                                       # (and the engine takes the adapter again)
    pipe.engine.close()


def test_engine_scale_zero_launches_nothing_and_equals_plain():
    """agd_ip_adapter_set at scale 0 (the engine's own idle path, which the pipeline never takes: it clears instead)."""
    from agenda_amd import _lib, synthetic
    cfg, u, v, ip, E = _model("tiny")
    pipe = _pipe(cfg, u, v)
    pipe.load_ip_adapter(ip)
    e = pipe.engine
    e.set_context(synthetic.make_context(cfg, 1, seed=3))
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(4)).cuda()
    plain = e.unet_forward(x, 401.0).cpu()
    e.ip_adapter_set(R.cfg_embeds(_embeds(1, E, 6)), 0.0)
    got = e.unet_forward(x, 401.0).cpu()
    assert e.ip_adapter_counts() == (0, 0) and torch.equal(got, plain)
    import ctypes
    ts = np.asarray([11.0, 12.0], np.float32)
    out = torch.empty_like(x)
    assert e.lib.agd_unet_forward_ts(e.ctx, _lib.ptr(x), 2, 16, ts.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _lib.ptr(out), None) == 0     # not refused
    e.close()


def test_sd15_forward_matches_restatement_through_the_fused_plan():
    """One forward at SD-1.5 widths, 256 px: the attn2 chain at C 320 / 640 with attn1.to_out outside it, the pre-multiplied form at
    C 1280 (8 x 8) and the kernels form at 4 x 4, each with norm3's statistics retaken after the add."""
    from agenda_amd import synthetic
    cfg, u, v, ip, E = _model("sd15")
    pipe = _pipe(cfg, u, v, ws=4 << 30)
    pipe.load_ip_adapter(ip)
    ctx = synthetic.make_context(cfg, 1, seed=3)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(4))
    emb = R.cfg_embeds(_embeds(1, E, 6))
    e = pipe.engine
    e.set_context(ctx)
    e.ip_adapter_set(emb, 1.0)
    got = e.unet_forward(x.cuda(), 401.0).cpu()
    e.close()
    tok = R.image_tokens(ip, emb, cfg.unet.cross_attention_dim)
    with torch.no_grad():
        want = R.unet_forward(u, cfg.unet, x, 401.0, ctx, ip, tok, 1.0)
        want_plain = R.unet_forward(u, cfg.unet, x, 401.0, ctx)
    err, effect = _rms_rel(got, want), _rms_rel(want_plain, want)
    print(f"ip-adapter unet sd15 L=32: rms rel {err:.4f}, adapter effect {effect:.4f}")
    report("ip_adapter_unet[sd15]", rms_rel=err, effect=effect)
    assert err < 0.03, err
    assert effect > 3 * err, (effect, err)


def test_cli_round_trip(tmp_path):
    from PIL import Image
    from _util import write_tiny_checkpoint
    cfg, u, v, ip, E = _model("tiny")
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, u, v, scheduler="DDIMScheduler")
    ipf = A.write_ip_adapter(str(tmp_path / "ip" / "ip_adapter.safetensors"), ip)
    scfg = A.image_encoder_config(**{**TOWERS["d64"], "projection_dim": E})
    A.write_image_encoder(str(tmp_path / "ip" / "image_encoder"), scfg, A.make_image_encoder_weights(scfg, 18))   # found beside the weights
    os.makedirs(tmp_path / "prompts")
    for i, im in enumerate(_images(2, 40, 56, 3)):
        Image.fromarray(im).save(tmp_path / "prompts" / f"{i}.png")
    save = tmp_path / "out"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--pretrained-model-path", ck, "--save-dir", str(save), "--num-images", "3",
           "--batch-size", "3", "--num-inference-steps", "2", "--image-size", "128", "--word_token_heatmaps", "cars",
           "--prompt", "an aerial view with cars", "--ip-adapter-path", ipf, "--ip-adapter-image", str(tmp_path / "prompts"), "--ip-adapter-scale", "0.7"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(os.listdir(save / "images")) == 3
