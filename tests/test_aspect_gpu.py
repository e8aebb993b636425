"""Non-square outputs (height != width) on the device: the `_hw` entry points, the rectangular DAAM recorder, the three fused
denoise loops, the VAE both ways, img2img, ControlNet, inpainting and the safety checker front end, each against the fp32 oracle
(or its restatements) in both orientations, plus bit-identity of the `_hw` forms at h == w with the one-side entry points."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _aspect_restated import AspectDaamRecorder, clip_resize_crop_geometry, inpaint_mask_latents, latent_mask_hw
from _report import report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIENT = [(16, 24), (24, 16)]                 # tiny configs: 128 x 192 and 192 x 128 px


def _rms_rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _latents(cfg, seeds, lh, lw):
    out = []
    for s in seeds:
        g = torch.Generator("cpu").manual_seed(int(s))
        out.append(torch.randn(1, cfg.unet.out_channels, lh, lw, generator=g))
    return torch.cat(out, 0)


def _tiny(name="tiny", scheduler=None, encoder=False):
    from agenda_amd import StableDiffusionPipeline, config, synthetic
    cfg = config.CONFIGS[name]()
    seeds = (11, 12) if name == "tiny" else (31, 32)
    u = synthetic.make_unet_weights(cfg, seeds[0], bias_std=0.05, perturb_norm=0.1)
    v = synthetic.make_vae_weights(cfg, seeds[1], bias_std=0.05, perturb_norm=0.1, with_encoder=encoder)
    kw = {} if scheduler is None else {"scheduler": scheduler}
    return StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30, **kw), cfg, u, v


# ---- the pipeline surface -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sched,key", [("tiny", None, "ddim"), ("tiny", "PNDMScheduler", "pndm"), ("tiny21", None, "ddim")])
@pytest.mark.parametrize("lh,lw", ORIENT)
def test_txt2img_rectangular_matches_oracle(name, sched, key, lh, lw):
    """End to end with decode and DAAM on, against O.generate and the rectangular restated recorder; the bounds of the square tests
    of the same configs (test_model_gpu.py: PNDM 0.06 / 30 dB / 0.06, tiny21 0.06 / 30 dB / 0.05)."""
    from agenda_amd import synthetic, trace
    from oracle import sd_oracle as O
    pipe, cfg, u, v = _tiny(name, sched)
    B, steps = 2, (6 if key == "pndm" else 2)
    ctx = synthetic.make_context(cfg, B, seed=5)
    lat = _latents(cfg, [3, 4], lh, lw)
    rec = AspectDaamRecorder((lh, lw), cfg.max_tokens)
    want_img, want_lat = O.generate(u, v, cfg, ctx, lat, steps, 7.5, recorder=rec, scheduler=key)
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, height=8 * lh, width=8 * lw, output_type="np")
        hms = [trc.compute_global_heat_map(image_index=i).heat_maps.cpu() for i in range(B)]
    whm = rec.compute_global_heat_map()
    assert out.images.shape == want_img.shape == (B, 8 * lh, 8 * lw, 3)
    assert hms[0].shape == (cfg.max_tokens, lh, lw)
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(torch.stack(hms), whm)
    print(f"{name}/{key} {8 * lh}x{8 * lw}: latents {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map {e_hm:.4f}")
    report(f"aspect_txt2img[{name},{key},{8 * lh}x{8 * lw}]", latents_rms_rel=e_lat, psnr=psnr, heat_map_rel=e_hm)
    assert e_lat < 0.06 and psnr > 30.0 and e_hm < 0.05, (e_lat, psnr, e_hm)
    pipe.engine.close()


@pytest.mark.parametrize("lh,lw", ORIENT)
def test_dpm_rectangular_matches_restated_host_loop(lh, lw):
    """The fused DPM-Solver++ loop at a rectangular size against the same UNet stepped on the host by the scheduler's program
    (float64 update), and the program's timesteps / coefficients against tests/_dpm_restated.py's grid."""
    import _dpm_restated as R
    from agenda_amd import synthetic
    pipe, cfg, u, v = _tiny("tiny", "DPMSolverMultistepScheduler")
    B, steps, g = 2, 6, 7.5
    ctx = synthetic.make_context(cfg, B, seed=31)
    lat0 = _latents(cfg, [7, 8], lh, lw)
    fused = pipe(prompt_embeds=ctx, latents=lat0, num_inference_steps=steps, height=8 * lh, width=8 * lw, output_type="latent").latents.cpu()
    pipe.scheduler.set_timesteps(steps)
    ts, cx, ce, a, b0, b1 = (np.asarray(p, dtype=np.float64) for p in pipe.scheduler.dpm_program())
    assert np.allclose(ts, np.asarray(R.grid(steps, False)[0], dtype=np.float64)[:steps], atol=1e-3)
    pipe.engine.set_context(ctx)
    x, prev = lat0.clone().double(), torch.zeros(B, cfg.unet.out_channels, lh, lw, dtype=torch.float64)
    for i in range(steps):
        eps = pipe.engine.unet_forward(torch.cat([x, x]).float().cuda().contiguous(), float(np.float32(ts[i]))).cpu().double()
        eu, ec = eps.chunk(2)
        x0 = cx[i] * x + ce[i] * (eu + g * (ec - eu))
        x = (a[i] * x + b0[i] * x0 + b1[i] * prev).float().double()
        prev = x0
    e = _rms_rel(fused, x)
    report(f"aspect_dpm_fused_vs_host[{8 * lh}x{8 * lw}]", latents_rms_rel=e)
    assert e < 1e-4, e
    pipe.engine.close()


@pytest.mark.parametrize("lh,lw", ORIENT)
def test_vae_both_ways_and_img2img_rectangular(lh, lw):
    from agenda_amd import synthetic
    from oracle import sd_oracle as O
    pipe, cfg, u, v = _tiny("tiny", encoder=True)
    B = 2
    z = _latents(cfg, [21, 22], lh, lw)
    got = pipe.engine.vae_decode(z).cpu().numpy()
    want = O.postprocess_image(O.vae_decode(v, cfg.vae, z / cfg.vae.scaling_factor))
    assert got.shape == want.shape == (B, 8 * lh, 8 * lw, 3)
    assert _psnr(got, want) > 30.0, _psnr(got, want)
    g = torch.Generator().manual_seed(9)
    img = torch.rand(B, 3, 8 * lh, 8 * lw, generator=g) * 2 - 1
    mean, logvar = pipe.engine.vae_encode(img)
    wm, wl = O.vae_encode_moments(v, cfg.vae, img)
    assert mean.shape == wm.shape == (B, cfg.vae.latent_channels, lh, lw)
    assert _rms_rel(mean, wm) < 2.0 ** -6 and _rms_rel(logvar, wl) < 2.0 ** -6, (_rms_rel(mean, wm), _rms_rel(logvar, wl))
    ctx = synthetic.make_context(cfg, B, seed=13)
    ne, nz = torch.randn(B, 4, lh, lw, generator=g), torch.randn(B, 4, lh, lw, generator=g)
    out = pipe.img2img(prompt_embeds=ctx, image=img, num_inference_steps=4, strength=0.75, noise_enc=ne, noise=nz, output_type="np")
    want_img, want_lat, _ = O.img2img(u, v, cfg, ctx, img, ne, nz, 4, strength=0.75)
    e = _rms_rel(out.latents, want_lat)
    report(f"aspect_vae_img2img[{8 * lh}x{8 * lw}]", img2img_latents_rms_rel=e, img2img_psnr=_psnr(out.images, want_img))
    assert out.images.shape == (B, 8 * lh, 8 * lw, 3)
    assert e < 0.06 and _psnr(out.images, want_img) > 30.0, (e, _psnr(out.images, want_img))
    pipe.engine.close()


def test_trace_and_word_maps_are_rectangular():
    from agenda_amd import synthetic, trace
    pipe, cfg, u, v = _tiny("tiny")
    lh, lw = 16, 24
    ctx = synthetic.make_context(cfg, 1, seed=3)
    with trace(pipe) as trc:
        pipe(prompt_embeds=ctx, latents=_latents(cfg, [5], lh, lw), num_inference_steps=2, height=128, width=192, output_type="latent")
        gm = trc.compute_global_heat_map(image_index=0)
    assert gm.heat_maps.shape == (cfg.max_tokens, lh, lw)
    wm = gm.compute_word_heat_map("x", word_idx=2)
    assert wm.heatmap.shape == (lh, lw)
    pipe.engine.close()


def test_hooker_refuses_rectangular_then_square_runs_as_before():
    from agenda_amd import UNetCrossAttentionHooker, synthetic
    pipe, cfg, u, v = _tiny("tiny")
    ctx = synthetic.make_context(cfg, 2, seed=19)
    lat = synthetic.make_latents(cfg, [7, 8], 16)

    def hooked():
        hk = UNetCrossAttentionHooker(is_train=False, latent_hw=16)
        pipe.unet.set_attn_processor(hk)
        try:
            out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, output_type="latent").latents.cpu()
            return out, hk.compute_global_heat_map().cpu()
        finally:
            pipe.unet.set_attn_processor("default")

    before = hooked()
    hk = UNetCrossAttentionHooker(is_train=False, latent_hw=16)
    pipe.unet.set_attn_processor(hk)
    try:
        with pytest.raises(ValueError, match="square latents only"):
            pipe(prompt_embeds=ctx, latents=_latents(cfg, [7, 8], 16, 24), num_inference_steps=2, height=128, width=192, output_type="latent")
    finally:
        pipe.unet.set_attn_processor("default")
    after = hooked()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    pipe.engine.close()


# ---- square identity ----------------------------------------------------------------------------------------------------------
def test_hw_entry_points_at_square_are_bit_identical():
    """Each `_hw` form at h == w against its one-side entry point, called through the C ABI: latents, eps, decoded image, DAAM maps."""
    from agenda_amd import _lib, synthetic
    pipe, cfg, u, v = _tiny("tiny", encoder=True)
    eng, lib = pipe.engine, pipe.engine.lib
    L, B = 16, 2
    ctx = synthetic.make_context(cfg, B, seed=3)
    x = synthetic.make_latents(cfg, [0, 1, 2, 3], L).cuda().contiguous()
    eng.set_context(ctx)
    st = eng._stream()
    outs = {}
    for hw in (False, True):
        eng.record_config(1, False, 77)
        rc = lib.agd_record_reset_hw(eng.ctx, B, L, L, st) if hw else lib.agd_record_reset(eng.ctx, B, L, st)
        _lib.check(rc, eng.ctx, "record_reset")
        eps = torch.empty_like(x)
        rc = (lib.agd_unet_forward_hw(eng.ctx, _lib.ptr(x), 2 * B, L, L, 501.0, _lib.ptr(eps), st) if hw else
              lib.agd_unet_forward(eng.ctx, _lib.ptr(x), 2 * B, L, 501.0, _lib.ptr(eps), st))
        _lib.check(rc, eng.ctx, "unet_forward")
        hm = eng.daam_global(1, 77, L).clone()
        lat = x[:B].clone().contiguous()
        n = 3
        ts, at, ap = (C.c_float * n)(901., 601., 301.), (C.c_float * n)(0.1, 0.3, 0.6), (C.c_float * n)(0.3, 0.6, 0.9)
        rc = (lib.agd_denoise_hw(eng.ctx, _lib.ptr(lat), B, L, L, n, ts, at, ap, 7.5, st) if hw else
              lib.agd_denoise(eng.ctx, _lib.ptr(lat), B, L, n, ts, at, ap, 7.5, st))
        _lib.check(rc, eng.ctx, "denoise")
        u8 = torch.empty(B, 8 * L, 8 * L, 3, device=lat.device, dtype=torch.uint8)
        rc = (lib.agd_vae_decode_hw(eng.ctx, _lib.ptr(lat), B, L, L, _lib.ptr(u8), None, st) if hw else
              lib.agd_vae_decode(eng.ctx, _lib.ptr(lat), B, L, _lib.ptr(u8), None, st))
        _lib.check(rc, eng.ctx, "vae_decode")
        img = (u8.permute(0, 3, 1, 2).float() / 127.5 - 1).contiguous()
        mean, logv = torch.empty(B, 4, L, L, device=lat.device), torch.empty(B, 4, L, L, device=lat.device)
        rc = (lib.agd_vae_encode_hw(eng.ctx, _lib.ptr(img), B, 8 * L, 8 * L, _lib.ptr(mean), _lib.ptr(logv), st) if hw else
              lib.agd_vae_encode(eng.ctx, _lib.ptr(img), B, 8 * L, _lib.ptr(mean), _lib.ptr(logv), st))
        _lib.check(rc, eng.ctx, "vae_encode")
        torch.cuda.synchronize()
        outs[hw] = [t_.cpu() for t_ in (eps, hm, lat, u8, mean, logv)]
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a, b)
    eng.record_config(0)
    pipe.engine.close()


def test_square_pipeline_call_is_unchanged():
    """`pipe(height=S, width=S)` passes one side through the same entry points as the default call: identical latents and maps."""
    from agenda_amd import synthetic, trace
    pipe, cfg, u, v = _tiny("tiny")
    ctx = synthetic.make_context(cfg, 2, seed=3)
    lat = synthetic.make_latents(cfg, [1, 2], 16)
    res = []
    for kw in ({}, {"height": 128, "width": 128}):
        with trace(pipe) as trc:
            out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, output_type="np", **kw)
            res.append((out.latents.cpu(), out.images, trc.compute_global_heat_map(image_index=1).heat_maps.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    pipe.engine.close()


# ---- ControlNet, inpainting, safety checker -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lh,lw", ORIENT)
def test_controlnet_residuals_and_pipeline_rectangular(lh, lw):
    import _controlnet_restated as R
    from agenda_amd import StableDiffusionControlNetPipeline, config, synthetic
    from agenda_amd.config import ControlNetConfig, controlnet_res_channels
    from agenda_amd.controlnet import ControlNetModel
    cfg = config.tiny()
    kw = dict(bias_std=0.05, perturb_norm=0.1)
    u, v = synthetic.make_unet_weights(cfg, 11, **kw), synthetic.make_vae_weights(cfg, 12, **kw)
    c = synthetic.make_controlnet_weights(cfg, seed=13, **kw)
    pipe = StableDiffusionControlNetPipeline(cfg, u, v, controlnet=ControlNetModel.from_config(cfg.unet, ControlNetConfig(), c), workspace_bytes=2 << 30)
    B2 = 2
    ctx = synthetic.make_context(cfg, B2 // 2, seed=5)
    x = _latents(cfg, [0, 1], lh, lw)
    cond = torch.rand(B2, 3, 8 * lh, 8 * lw, generator=torch.Generator().manual_seed(21))
    pipe.engine.set_context(ctx)
    pipe.engine.controlnet_set_cond(cond, repeat=1)
    flat = pipe.engine.controlnet_residuals(x, 501.0, 0.8).cpu()
    with torch.no_grad():
        parts = [R.controlnet_forward(c, cfg.unet, x[i:i + 1], torch.tensor(501.0), ctx[i:i + 1], cond[i:i + 1], 0.8) for i in range(B2)]
    want = [torch.cat([p_[0][k] for p_ in parts]) for k in range(len(parts[0][0]))] + [torch.cat([p_[1] for p_ in parts])]
    off, errs = 0, []
    for w_ in want:
        n = w_.numel()
        errs.append(_rms_rel(flat[off:off + n].view(w_.shape), w_))
        off += n
    assert off == flat.numel()
    assert max(errs) < 0.03, errs
    # the pipeline: the conditioning embedding at (height, width), two DDIM steps against the restated controlled generate
    ctx1 = synthetic.make_context(cfg, 1, seed=9)
    lat = _latents(cfg, [4], lh, lw)
    cimg = torch.rand(1, 3, 8 * lh, 8 * lw, generator=torch.Generator().manual_seed(22))
    out = pipe(prompt_embeds=ctx1, image=cimg, latents=lat, num_inference_steps=2, height=8 * lh, width=8 * lw, output_type="latent")
    _, want_lat = R.generate(u, v, c, cfg, ctx1, lat, cimg, 2, "ddim")
    e = _rms_rel(out.latents, want_lat)
    report(f"aspect_controlnet[{8 * lh}x{8 * lw}]", residuals_rms_rel_max=max(errs), latents_rms_rel=e)
    assert e < 0.06, e
    pipe.engine.close()


@pytest.mark.parametrize("nine", [True, False], ids=["9ch", "blend"])
@pytest.mark.parametrize("lh,lw", ORIENT)
def test_inpainting_rectangular_matches_restatement(nine, lh, lw, monkeypatch):
    import _inpaint_restated as R
    from agenda_amd import StableDiffusionInpaintPipeline, config, synthetic
    monkeypatch.setattr(R, "latent_mask", lambda m, L: latent_mask_hw(m, 8))       # the mask step at (H / 8, W / 8)
    cfg = config.tiny()
    cfg = config.inpaint_variant(cfg) if nine else cfg
    kw = dict(bias_std=0.05, perturb_norm=0.1)
    u, v = synthetic.make_unet_weights(cfg, 11, **kw), synthetic.make_vae_weights(cfg, 12, with_encoder=True, **kw)
    pipe = StableDiffusionInpaintPipeline(cfg, u, v, workspace_bytes=2 << 30)
    B, H, W = 2, 8 * lh, 8 * lw
    rng = np.random.default_rng(5)
    img = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8))
    m = np.zeros((B, H, W), dtype=np.uint8)
    m[0, H // 4:H // 2, W // 3:] = 255
    m[1, H // 2:, :W // 2] = 255
    mask = torch.from_numpy(m)
    g = torch.Generator().manual_seed(7)
    ne, nz, me = (torch.randn(B, 4, lh, lw, generator=g) for _ in range(3))
    ctx = synthetic.make_context(cfg, B, seed=41)
    x, mlat = pipe.engine.inpaint_prepare(img, mask, True, False)
    assert mlat.shape == (B, 1, lh, lw)
    assert torch.equal(mlat.cpu(), inpaint_mask_latents(mask.float() / 255.0))
    want_img, want_lat, _ = R.generate(u, v, cfg, ctx, img, mask, 3, "ddim", noise_enc_image=ne, noise=nz, noise_enc_masked=me)
    out = pipe(prompt_embeds=ctx, image=img, mask_image=mask, noise_enc_image=ne, noise=nz, noise_enc_masked=me, num_inference_steps=3,
               height=H, width=W, output_type="np")
    e, psnr = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img)
    report(f"aspect_inpaint[{'9ch' if nine else 'blend'},{H}x{W}]", latents_rms_rel=e, psnr=psnr)
    assert out.images.shape == (B, H, W, 3)
    assert e < 0.06 and psnr > 30.0, (e, psnr)
    pipe.engine.close()


@pytest.mark.parametrize("h,w", [(512, 768), (768, 512)])
def test_safety_front_end_rectangular_matches_clip_image_processor(h, w):
    from PIL import Image
    from agenda_amd import StableDiffusionPipeline, config, synthetic
    from _safety_restated import CLIP_MEAN, CLIP_STD, cosine_distance, hf_tower
    try:
        from transformers import CLIPImageProcessorPil as Proc
    except ImportError:
        from transformers import CLIPImageProcessor as Proc
    cfg = config.tiny()
    cfg.safety = config.SafetyConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, projection_dim=64,
                                     n_special=3, n_concepts=17)
    ssd = synthetic.make_safety_weights(cfg, 3)
    pipe = StableDiffusionPipeline(cfg, synthetic.make_unet_weights(cfg), synthetic.make_vae_weights(cfg), safety_sd=ssd, workspace_bytes=1 << 30)
    rng = np.random.default_rng(h + w)
    im = np.clip(rng.uniform(0, 255, (2, 1, 1, 3)) + rng.normal(0, 40, (2, h, w, 3)), 0, 255).astype(np.uint8)
    cos, pix = pipe.safety_checker.scores(torch.from_numpy(im).cuda(), pixels=True)
    hf = Proc(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, resample=3, image_mean=list(CLIP_MEAN),
              image_std=list(CLIP_STD))(images=[Image.fromarray(x) for x in im], return_tensors="np").pixel_values
    assert clip_resize_crop_geometry(h, w, 224)[:2] == ((224, 336) if h < w else (336, 224))
    pix = pix.cpu().numpy()
    assert pix.shape == hf.shape == (2, 3, 224, 224)
    assert np.abs(pix - hf).max() <= 1e-6
    emb = hf_tower(cfg.safety, ssd)(torch.from_numpy(hf))
    want = np.concatenate([cosine_distance(emb, ssd["special_care_embeds"]), cosine_distance(emb, ssd["concept_embeds"])], 1)
    e = float(np.abs(cos.cpu().numpy() - want).max())
    report(f"aspect_safety[{h}x{w}]", cos_max_abs=e)
    assert e < 0.003, e
    want_flags = pipe.safety_checker(torch.from_numpy(im).cuda())
    assert len(want_flags) == 2
    pipe.engine.close()


# ---- SD-1.5 shapes ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd15():
    from agenda_amd import StableDiffusionPipeline, config, synthetic
    cfg = config.sd15()
    u, v = synthetic.make_unet_weights(cfg, 1234), synthetic.make_vae_weights(cfg, 1235)
    pipe = StableDiffusionPipeline(cfg, u, v, workspace_bytes=12 << 30)
    yield pipe, cfg, u, v
    pipe.engine.close()


@pytest.mark.parametrize("h,w", [(512, 768), (768, 512)])
def test_sd15_cfg_pair_forward_with_daam_rectangular(sd15, h, w):
    """The bounds of test_sd15_unet_forward_512px_matches_oracle: rms rel < 2^-6, heat map rel < 0.02, 15 x 8 accumulators."""
    from agenda_amd import synthetic
    from oracle import sd_oracle as O
    pipe, cfg, u, v = sd15
    lh, lw = h // 8, w // 8
    ctx = synthetic.make_context(cfg, 1, seed=7)
    lat = _latents(cfg, [0], lh, lw)
    x = torch.cat([lat, lat]).to(torch.bfloat16).float()
    rec = AspectDaamRecorder((lh, lw), 77)
    with torch.no_grad():
        want = O.unet_forward(u, cfg.unet, x, torch.tensor(981), ctx, rec)
    pipe.engine.set_context(ctx)
    pipe.engine.record_config(1, False, 77)
    pipe.engine.record_reset(1, (lh, lw))
    got = pipe.engine.unet_forward(x, 981.0)
    hm = pipe.engine.daam_global(0, 77, (lh, lw)).cpu()
    pipe.engine.record_config(0)
    whm = rec.compute_global_heat_map()[0]
    e, e_hm = _rms_rel(got, want), _rel(hm, whm)
    print(f"SD-1.5 {h}x{w} CFG-pair forward: rms rel {e:.5f}, heat map rel {e_hm:.4f}")
    report(f"aspect_sd15_forward[{h}x{w}]", rms_rel=e, heat_map_rel=e_hm)
    assert len(rec.acc) == 15 * 8
    assert hm.shape == (77, lh, lw)
    assert e < 2.0 ** -6, e
    assert e_hm < 0.02, e_hm


@pytest.mark.parametrize("h,w", [(512, 768), (768, 512)])
def test_sd15_two_ddim_steps_merged_vs_unmerged_vs_oracle(sd15, h, w):
    """The option sets and bounds of test_merged_launches_at_odd_sizes_match_the_unmerged_walk: every merge decides from the launch's
    shape whether it applies; portrait sizes put the row-halo kernels on maps with Hout != Wout."""
    from agenda_amd import synthetic
    from oracle import sd_oracle as O
    pipe, cfg, u, v = sd15
    lh, lw = h // 8, w // 8
    ctx = synthetic.make_context(cfg, 1, seed=h)
    lat = _latents(cfg, [w], lh, lw)
    off = {"tblock_fuse": 0, "reduce_gn": 0, "shortcut_fuse": 0, "ff_proj_fuse": 0, "upsample_phases": 0, "igemm_kgroups": 0, "wreg_mask": 0, "conv_smap": 0,
           "attn2_premul": 0, "igemm_pc": 0, "xcd_block": 0}
    on = {"tblock_fuse": 7935, "reduce_gn": 1, "shortcut_fuse": 3, "ff_proj_fuse": 1, "upsample_phases": 7, "igemm_kgroups": 1, "wreg_mask": 3, "conv_smap": 1,
          "attn2_premul": 1, "igemm_pc": 49, "xcd_block": 1}

    def run():
        return pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, height=h, width=w, output_type="latent").latents.clone()

    try:
        a = run()
        for k, val in off.items():
            pipe.engine.set_option(k, val)
        b = run()
    finally:
        for k, val in on.items():
            pipe.engine.set_option(k, val)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    _, want = O.generate(u, v, cfg, ctx, lat, 2, 7.5, decode=False)
    e, e_a, e_b = _rms_rel(a, b.cpu()), _rms_rel(a, want), _rms_rel(b, want)
    print(f"SD-1.5 {h}x{w}: merged vs unmerged {e:.5f}, vs oracle merged {e_a:.5f} unmerged {e_b:.5f}")
    report(f"aspect_sd15_two_steps[{h}x{w}]", merged_vs_unmerged=e, merged_vs_oracle=e_a, unmerged_vs_oracle=e_b)
    assert e < 0.08, e
    assert e_a < 0.05 and e_b < 0.05, (e_a, e_b)


@pytest.mark.parametrize("h,w", [(128, 192), (192, 128)])
def test_generation_cli_writes_rectangular_images_and_heat_maps(tmp_path, h, w):
    from PIL import Image
    save = tmp_path / "out"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--synthetic-config", "tiny", "--height", str(h), "--width", str(w),
           "--save-dir", str(save), "--num-images", "2", "--batch-size", "2", "--num-inference-steps", "2", "--image-size", str(h // 2),
           str(w // 2), "--word_token_heatmaps", "cars", "--prompt", "an aerial view with cars", "--no-safety-checker"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for sub in ("images", "daam_cars_heatmaps"):
        files = sorted(os.listdir(save / sub))
        assert files == ["0.png", "1.png"], files
        assert Image.open(save / sub / "0.png").size == (w // 2, h // 2)
