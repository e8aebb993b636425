"""InstructPix2Pix on the device: the image front end and VAE mean against the restatement, the three-branch fused loops under DDIM, PNDM
and DPM-Solver++ against the fp32 restatement (tests/_ip2p_restated.py) with DAAM on, the fused loop against a host-stepped one, the
exact branch-wiring identities, batch independence, the recorders, state clearing, the error statuses and the CLI."""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ip2p_restated as R
from _report import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DDIM2 = ([500, 1], [0.5, 0.9], [0.9, 0.99])                # a two-evaluation DDIM program for the engine-level calls


def _rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def _rms_rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _cfg(name="tiny"):
    from agenda_amd import config
    return config.ip2p_variant(config.CONFIGS[name]())


@functools.lru_cache(maxsize=None)
def _weights(name="tiny", small=True):
    """The small synthetic weights test_inpaint_gpu.py uses, with the 8-channel conv_in."""
    from agenda_amd import synthetic
    cfg = _cfg(name)
    kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
    return synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw), synthetic.make_vae_weights(cfg, 12 if small else 1235, with_encoder=True, **kw)


def _pipe(name="tiny", scheduler="DDIMScheduler", small=True):
    from agenda_amd import StableDiffusionInstructPix2PixPipeline
    u, v = _weights(name, small)
    return StableDiffusionInstructPix2PixPipeline(_cfg(name), u, v, workspace_bytes=2 << 30, scheduler=scheduler)


def _image(B, H, W, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8))


def _noise(cfg, B, Lh, Lw, seed):
    return torch.randn(B, cfg.unet.out_channels, Lh, Lw, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _image_latents(B, H, W, seed):
    """The restatement's image latents of `_image(B, H, W, seed)` under the small tiny weights: computed once, shared, never modified."""
    cfg = _cfg()
    return R.image_latents(_weights()[1], cfg.vae, R.preprocess_image(_image(B, H, W, seed)))


# ---- front end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("H,W", [(64, 64), (64, 128)])
def test_front_end_and_vae_mean_match_restatement(as_float, H, W):
    """uint8 NHWC and float NCHW inputs, B = 3: the image latents (VAE mean, unscaled) against the restatement; the rms bound is the one
    test_inpaint_gpu.py asserts for its masked-image latents (0.03)."""
    pipe = _pipe()
    B = 3
    img = _image(B, H, W, 3)
    want = _image_latents(B, H, W, 3)
    got = pipe.engine.ip2p_prepare(R.preprocess_image(img) if as_float else img).cpu()
    assert got.shape == want.shape == (B, 4, H // 8, W // 8)
    e = _rms_rel(got, want)
    report(f"ip2p_front_end[{'f32' if as_float else 'u8'},{H}x{W}]", image_latents_rms_rel=e)
    pipe.engine.close()
    assert e < 0.03, e


# ---- loops against the restatement -----------------------------------------------------------------------------------------------
CASES = [("tiny", "DDIMScheduler", "ddim", 6, 16, 16, True), ("tiny", "PNDMScheduler", "pndm", 6, 16, 16, True),
         ("tiny", "DPMSolverMultistepScheduler", "dpm", 6, 16, 16, True), ("tiny", "DDIMScheduler", "ddim", 6, 16, 24, True),
         ("sd15", "DDIMScheduler", "ddim", 3, 32, 32, False)]


@pytest.mark.parametrize("name,scheduler,key,steps,Lh,Lw,small", CASES)
def test_loop_matches_restatement(name, scheduler, key, steps, Lh, Lw, small):
    """B = 2, guidance_scale 7.5, image_guidance_scale 1.5: latents, decoded image and the DAAM heat map of each image against the
    restatement, which records the text branch only.  The bounds are the ones test_inpaint_gpu.py asserts for its 9-channel loop at the
    same configs and step counts: latents rms-rel < 0.06, PSNR > 30 dB, heat map max-rel < 0.06."""
    from _aspect_restated import AspectDaamRecorder
    from agenda_amd import synthetic, trace
    cfg = _cfg(name)
    u, v = _weights(name, small)
    B = 2
    ctx = synthetic.make_context(cfg, B, seed=41)
    img = _image(B, 8 * Lh, 8 * Lw, 5)
    nz = _noise(cfg, B, Lh, Lw, 7)
    rec = AspectDaamRecorder((Lh, Lw), context_size=cfg.max_tokens)
    want_img, want_lat, want_il = R.generate(u, v, cfg, ctx, img, nz, steps, key, 7.5, 1.5, recorder=rec)
    whm = rec.compute_global_heat_map()
    pipe = _pipe(name, scheduler, small)
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, image=img, latents=nz, num_inference_steps=steps, guidance_scale=7.5, image_guidance_scale=1.5,
                   output_type="np")
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    e_il = _rms_rel(pipe._ip2p_inputs["image_latents"], want_il)
    pipe.engine.close()
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(hm, whm)
    e_hm_each = [_rel(hm[i], whm[i]) for i in range(B)]
    print(f"ip2p {name} {key} {Lh}x{Lw}: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map rel {e_hm:.4f} {e_hm_each}, image latents {e_il:.4f}")
    report(f"ip2p[{name},{key},{Lh}x{Lw}]", latents_rms_rel=e_lat, psnr_db=psnr, heat_map_rel=e_hm, image_latents_rms_rel=e_il)
    assert out.images.shape == (B, 8 * Lh, 8 * Lw, 3) and hm.shape == whm.shape
    assert e_il < 0.03, e_il
    assert e_lat < 0.06, e_lat
    assert psnr > 30.0, psnr
    assert max(e_hm_each) < 0.06, e_hm_each


# ---- fused against host-stepped ---------------------------------------------------------------------------------------------------
def test_fused_loop_matches_host_stepped_loop():
    """The same call two ways: the fused DDIM loop, and per step three unet forwards (text, image, uncond) with the guidance formula and
    the DDIM update in torch.  The bound is the one of test_inpaint_gpu.py's fused-versus-host-stepped case (1e-3)."""
    from agenda_amd import synthetic
    cfg = _cfg()
    pipe = _pipe()
    B, L, steps, s_t, s_i = 2, 16, 5, 7.5, 1.5
    ctx = synthetic.make_context(cfg, B, seed=8)
    img = _image(B, 8 * L, 8 * L, 6)
    nz = _noise(cfg, B, L, L, 12)
    out = pipe(prompt_embeds=ctx, image=img, latents=nz, num_inference_steps=steps, guidance_scale=s_t, image_guidance_scale=s_i,
               output_type="latent")
    il = pipe._ip2p_inputs["image_latents"]
    x = (nz * pipe.scheduler.init_noise_sigma).cuda()
    ts = pipe.scheduler.set_timesteps(steps)
    a_t, a_p = pipe.scheduler.step_coeffs()
    for i, t in enumerate(ts):
        xi = torch.cat([x, il], 1)
        e_text = pipe.unet(xi, float(t), encoder_hidden_states=ctx[B:]).sample
        e_image = pipe.unet(xi, float(t), encoder_hidden_states=ctx[:B]).sample
        e_uncond = pipe.unet(torch.cat([x, torch.zeros_like(il)], 1), float(t), encoder_hidden_states=ctx[:B]).sample
        e = R.combine(e_uncond, e_image, e_text, s_t, s_i)
        x0 = (x - (1 - a_t[i]) ** 0.5 * e) / a_t[i] ** 0.5
        x = a_p[i] ** 0.5 * x0 + (1 - a_p[i]) ** 0.5 * e
    e = _rms_rel(out.latents, x)
    report("ip2p_fused_vs_host_stepped[tiny]", latents_rms_rel=e)
    pipe.engine.close()
    assert e < 1e-3, e


# ---- branch wiring ------------------------------------------------------------------------------------------------------------
def test_text_scale_cancels_exactly_when_prompt_equals_negative_prompt():
    """prompt_embeds whose cond rows equal the uncond rows: e_text == e_image row for row, so guidance_scale 2 and 20 give bit-identical
    latents (the fold writes hi = lo + (e_text - e_image) = lo)."""
    from agenda_amd import synthetic
    cfg = _cfg()
    pipe = _pipe()
    B, L = 2, 16
    half = synthetic.make_context(cfg, B, seed=4)[:B]
    ctx = torch.cat([half, half])
    img, nz = _image(B, 8 * L, 8 * L, 2), _noise(cfg, B, L, L, 3)
    run = lambda g: pipe(prompt_embeds=ctx, image=img, latents=nz, num_inference_steps=4, guidance_scale=g, image_guidance_scale=1.5,
                         output_type="latent").latents.cpu()
    a, b = run(2.0), run(20.0)
    pipe.engine.close()
    assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())


def test_image_scale_cancels_exactly_with_zero_image_latents():
    """Zero image latents installed through agd_ip2p_set_hw: the image branch's input and context equal the uncond branch's, so
    e_image == e_uncond, the fold writes lo = e_uncond + s_i * 0 and image_guidance_scale 1 and 5 give bit-identical latents.  This
    needs the uncond walk (B rows, no shared prefix) to reproduce the [uncond | cond] walk's uncond rows (2 B rows, shared prefix) bit for
    bit, which holds for the kernels these shapes take."""
    from agenda_amd import synthetic
    cfg = _cfg()
    pipe = _pipe()
    eng = pipe.engine
    B, L = 2, 16
    eng.set_context(synthetic.make_context(cfg, B, seed=6))
    nz = _noise(cfg, B, L, L, 9).cuda().contiguous()
    zero = torch.zeros(B, 4, L, L)

    def run(s_i):
        eng.ip2p_set(zero, s_i)
        try:
            return eng.denoise(nz.clone(), *DDIM2, 7.5).cpu()
        finally:
            eng.ip2p_clear()
    a, b = run(1.0), run(5.0)
    eng.close()
    assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())


# ---- batch shapes -----------------------------------------------------------------------------------------------------------------
def test_rows_of_a_batch_match_their_batch_1_runs():
    """B = 3 (the uncond walk runs an odd row count) against B = 1 runs of each row.  The issue allows the panorama test's bounds for batch
    independence (latents rms-rel < 0.06, heat map max-rel < 0.05); at these shapes every kernel of the walk computes a row from that row's
    data alone in a fixed order and both differences were measured as 0, so bit equality is asserted: a row-mixing bug of any size
    fails.  A B = 1 run repeated is bit-identical too."""
    from agenda_amd import synthetic, trace
    cfg = _cfg()
    pipe = _pipe()
    B, L, steps = 3, 16, 3
    ctx = synthetic.make_context(cfg, B, seed=13)
    img, nz = _image(B, 8 * L, 8 * L, 14), _noise(cfg, B, L, L, 15)

    def run(rows):
        c = torch.cat([ctx[rows], ctx[[B + r for r in rows]]])
        with trace(pipe) as trc:
            lat = pipe(prompt_embeds=c, image=img[rows], latents=nz[rows], num_inference_steps=steps, output_type="latent").latents.cpu()
            hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(len(rows))]).cpu()
        return lat, hm
    lat3, hm3 = run([0, 1, 2])
    for r in range(B):
        lat1, hm1 = run([r])
        e, h = _rms_rel(lat3[r:r + 1], lat1), _rel(hm3[r:r + 1], hm1)
        report(f"ip2p_batch1[tiny,row={r}]", latents_rms_rel=e, heat_map_rel=h)
        assert torch.equal(lat3[r:r + 1], lat1) and torch.equal(hm3[r:r + 1], hm1), (r, e, h)
    again = run([2])
    pipe.engine.close()
    assert torch.equal(again[0], lat1) and torch.equal(again[1], hm1)


# ---- recorders ------------------------------------------------------------------------------------------------------------------
def test_hooker_records_the_text_branch_only():
    """A hooker-recorded square call keeps one map per cross-attention layer and evaluation (16 for this UNet), not 32 or 48: the uncond walk
    records nothing and the [image | text] walk records its conditional half.  (The DAAM heat map against the restatement, which records
    the text branch only, is asserted by test_loop_matches_restatement.)"""
    from agenda_amd import UNetCrossAttentionHooker, synthetic
    cfg = _cfg()
    pipe = _pipe()
    B, L, steps = 2, 16, 2
    n_layers = sum(cfg.unet.down_cross) * (2 * cfg.unet.layers_per_block + 1) + 1
    assert n_layers == 16
    hk = UNetCrossAttentionHooker(is_train=False, latent_hw=L)
    pipe.unet.set_attn_processor(hk)
    try:
        pipe(prompt_embeds=synthetic.make_context(cfg, B, seed=19), image=_image(B, 8 * L, 8 * L, 20), latents=_noise(cfg, B, L, L, 21),
             num_inference_steps=steps, output_type="latent")
        n, g = hk.num_recorded, hk.compute_global_heat_map().cpu()
    finally:
        pipe.unet.set_attn_processor("default")
    pipe.engine.close()
    assert n == steps * n_layers, n
    assert g.shape == (B, cfg.max_tokens, L, L) and torch.isfinite(g).all() and float(g.abs().max()) > 0


# ---- state ------------------------------------------------------------------------------------------------------------------------
def test_state_is_cleared_and_plain_txt2img_is_unchanged():
    from agenda_amd import StableDiffusionPipeline, config, synthetic
    cfg4 = config.tiny()
    u4 = synthetic.make_unet_weights(cfg4, 11, bias_std=0.05, perturb_norm=0.1)
    v4 = synthetic.make_vae_weights(cfg4, 12, bias_std=0.05, perturb_norm=0.1)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg4, B, seed=2)
    lat = synthetic.make_latents(cfg4, [5, 6], L)

    def plain():
        p = StableDiffusionPipeline(cfg4, u4, v4, workspace_bytes=2 << 30)
        try:
            return p(prompt_embeds=ctx, latents=lat, num_inference_steps=4, output_type="latent").latents.cpu()
        finally:
            p.engine.close()
    want = plain()
    pipe = _pipe()
    pipe(prompt_embeds=ctx, image=_image(B, 8 * L, 8 * L, 1), latents=lat, num_inference_steps=3, output_type="latent")
    assert torch.equal(plain(), want)                          # a fresh plain pipeline in the same process: bit for bit
    # the call left no state behind: the 8-channel UNet's fused loop is refused, with the message that names both pipelines' states
    x = lat.cuda().contiguous()
    with pytest.raises(Exception, match="agd_ip2p_set_hw"):
        pipe.engine.denoise(x, *DDIM2, 7.5)
    pipe.engine.ip2p_set(torch.zeros(B, 4, L, L), 1.5)
    pipe.engine.ip2p_clear()
    with pytest.raises(Exception, match="agd_ip2p_set_hw"):
        pipe.engine.denoise(x, *DDIM2, 7.5)
    with pytest.raises(ValueError, match="StableDiffusionInstructPix2PixPipeline"):
        StableDiffusionPipeline.__call__(pipe, prompt_embeds=ctx, latents=lat, num_inference_steps=2)
    # an error inside the call clears the state too
    def boom(*a):
        raise RuntimeError("boom")
    pipe._denoise = boom
    with pytest.raises(RuntimeError, match="boom"):
        pipe(prompt_embeds=ctx, image=_image(B, 8 * L, 8 * L, 1), latents=lat, num_inference_steps=2, output_type="latent")
    with pytest.raises(Exception, match="agd_ip2p_set_hw"):
        pipe.engine.denoise(x, *DDIM2, 7.5)
    pipe.engine.close()


# ---- error statuses -----------------------------------------------------------------------------------------------------------------
def test_error_statuses():
    """Every refusal of the engine, through the C ABI, and of the pipeline.  The ControlNet refusal runs on a ControlNet pipeline built on
    the 8-channel config; the GLIGEN one on test_gligen_schedule_is_refused's subclass."""
    from agenda_amd import StableDiffusionControlNetPipeline, StableDiffusionPipeline, config, synthetic
    from agenda_amd._lib import AgendaHipError
    P = lambda t: C.c_void_p(t.data_ptr())
    B, L = 2, 16
    z = torch.zeros(B, 4, L, L, device="cuda")
    # a 4-channel UNet takes no ip2p state
    p4 = StableDiffusionPipeline.from_synthetic("tiny", seed=5, workspace_bytes=2 << 30)
    assert p4.engine.lib.agd_ip2p_set_hw(p4.engine.ctx, P(z), B, L, L, C.c_float(1.5), None) != 0
    assert b"input channels" in p4.engine.lib.agd_last_error(p4.engine.ctx)
    with pytest.raises(AgendaHipError, match="input channels"):
        p4.engine.ip2p_set(z, 1.5)
    p4.engine.close()
    # the 8-channel UNet with a ControlNet loaded
    cfg = _cfg()
    pipe = StableDiffusionControlNetPipeline.from_synthetic(cfg, seed=5, workspace_bytes=2 << 30)
    eng, lib = pipe.engine, pipe.engine.lib
    eng.set_context(synthetic.make_context(cfg, B, seed=1))
    x = torch.zeros(B, 4, L, L, device="cuda")
    with pytest.raises(AgendaHipError, match="agd_ip2p_set_hw"):                              # no state
        eng.denoise(x, *DDIM2, 7.5)
    assert lib.agd_ip2p_set_hw(eng.ctx, P(z), 0, L, L, C.c_float(1.5), None) != 0             # batch 0
    assert lib.agd_ip2p_set_hw(eng.ctx, None, B, L, L, C.c_float(1.5), None) != 0             # no latents given and none prepared
    assert lib.agd_ip2p_set_hw(eng.ctx, P(z), B, L, L, C.c_float(float("nan")), None) != 0
    assert lib.agd_ip2p_prepare_hw(eng.ctx, None, 0, B, 64, 64, None, None) != 0
    img60 = torch.zeros(B, 60, 60, 3, dtype=torch.uint8, device="cuda")
    assert lib.agd_ip2p_prepare_hw(eng.ctx, P(img60), 0, B, 60, 60, None, None) != 0          # side not a multiple of 8
    eng.ip2p_set(z, 1.5)
    with pytest.raises(AgendaHipError, match="holds 2 images"):                               # size mismatch
        eng.denoise(torch.zeros(B, 4, 8, 8, device="cuda"), *DDIM2, 7.5)
    eng.set_context(synthetic.make_context(cfg, 1, seed=1))
    with pytest.raises(AgendaHipError, match="holds 2 images"):                               # batch mismatch
        eng.denoise(torch.zeros(1, 4, L, L, device="cuda"), *DDIM2, 7.5)
    eng.set_context(synthetic.make_context(cfg, B, seed=1))
    eng.controlnet_set_schedule([0.0, 0.0])
    for loop in (lambda: eng.denoise(x, *DDIM2, 7.5), lambda: eng.denoise_plms(x, [500, 1], [1.0, 1.0], [0.1, 0.1], 7.5),
                 lambda: eng.denoise_dpm(x, [500, 1], [1.0, 1.0], [0.1, 0.1], [1.0, 1.0], [0.1, 0.1], [0.0, 0.0], 7.5)):
        with pytest.raises(AgendaHipError, match="ControlNet"):
            loop()
    eng.controlnet_set_schedule([])
    eng.inpaint_set(torch.zeros(B, 1, L, L), torch.zeros(B, 3, L, L))                        # 4 + 1 + 3 channels: an inpainting state fits
    with pytest.raises(AgendaHipError, match="inpainting"):
        eng.denoise(x, *DDIM2, 7.5)
    eng.inpaint_clear()
    with pytest.raises(AgendaHipError, match="InstructPix2Pix"):                              # a panorama with the state set
        eng.denoise_panorama(torch.zeros(B, 4, L, 2 * L, device="cuda"), L, 8, None, *DDIM2, 7.5)
    eng.denoise(x, *DDIM2, 7.5)                                                               # and with nothing else set it runs
    torch.cuda.synchronize()
    assert torch.isfinite(x).all()
    eng.ip2p_clear()
    eng.close()
    # the pipeline's own refusals
    pipe = _pipe()
    ctx = synthetic.make_context(cfg, B, seed=1)
    img = _image(B, 8 * L, 8 * L, 1)
    with pytest.raises(ValueError, match="guidance_scale"):
        pipe(prompt_embeds=ctx, image=img, guidance_scale=1.0)
    with pytest.raises(ValueError, match="image_guidance_scale"):
        pipe(prompt_embeds=ctx, image=img, image_guidance_scale=0.5)
    with pytest.raises(ValueError, match="height=72, width=128"):
        pipe(prompt_embeds=ctx, image=_image(B, 72, 128, 1))
    with pytest.raises(ValueError, match="must be 1 or equal"):
        pipe(prompt_embeds=synthetic.make_context(cfg, 3, seed=1), image=img)
    with pytest.raises(NotImplementedError, match="instruction edits only"):
        pipe.img2img(prompt="x", image=img)
    pipe.engine.close()


def test_gligen_schedule_is_refused():
    """The GLIGEN pipeline builds 4-channel UNets only, but the C ABI can configure GLIGEN on an 8-channel one: a subclass loads a
    PositionNet and fusers as StableDiffusionGLIGENPipeline._load_extra does.  A GLIGEN schedule together with the ip2p state is then refused
    by name, before anything runs, under all three schedulers."""
    from agenda_amd import StableDiffusionInstructPix2PixPipeline, synthetic
    from agenda_amd._lib import AgendaHipError
    from agenda_amd.gligen import FOURIER_FREQS, MAX_OBJS, make_gligen_weights
    cfg = _cfg()
    u, v = _weights()

    class Gated(StableDiffusionInstructPix2PixPipeline):
        def _load_extra(self):
            self.engine.gligen_configure(self.cfg.unet.cross_attention_dim, MAX_OBJS, FOURIER_FREQS)
            self.engine.load_state_dict(make_gligen_weights(self.cfg, 14), "unet.")
    pipe = Gated(cfg, u, v, workspace_bytes=2 << 30)
    eng = pipe.engine
    B, L = 2, 16
    eng.set_context(synthetic.make_context(cfg, B, seed=1))
    x = torch.ones(B, 4, L, L, device="cuda")
    eng.ip2p_set(torch.zeros(B, 4, L, L), 1.5)
    eng.gligen_set_schedule([0, 0])
    rc = eng.lib.agd_denoise_hw(eng.ctx, C.c_void_p(x.data_ptr()), B, L, L, 2, (C.c_float * 2)(500, 1), (C.c_float * 2)(0.5, 0.9),
                                (C.c_float * 2)(0.9, 0.99), 7.5, None)
    assert rc != 0 and b"GLIGEN" in eng.lib.agd_last_error(eng.ctx)
    for loop in (lambda: eng.denoise(x, *DDIM2, 7.5), lambda: eng.denoise_plms(x, [500, 1], [1.0, 1.0], [0.1, 0.1], 7.5),
                 lambda: eng.denoise_dpm(x, [500, 1], [1.0, 1.0], [0.1, 0.1], [1.0, 1.0], [0.1, 0.1], [0.0, 0.0], 7.5)):
        with pytest.raises(AgendaHipError, match="GLIGEN"):
            loop()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.ones(B, 4, L, L))        # refused before the first launch
    eng.gligen_set_schedule([])
    eng.denoise(x, *DDIM2, 7.5)                                # with the schedule cleared the same call runs
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and not torch.equal(x.cpu(), torch.ones(B, 4, L, L))
    eng.ip2p_clear()
    eng.close()


def test_prepared_latents_can_be_installed_without_a_copy_back():
    """agd_ip2p_set_hw with a null pointer installs the latents agd_ip2p_prepare_hw left on the device: the loop equals the one on the
    same latents passed explicitly, bit for bit; a prepare of another shape in between is refused."""
    from agenda_amd import synthetic
    cfg = _cfg()
    pipe = _pipe()
    eng, lib = pipe.engine, pipe.engine.lib
    B, L = 2, 16
    eng.set_context(synthetic.make_context(cfg, B, seed=6))
    nz = _noise(cfg, B, L, L, 9).cuda().contiguous()
    img = _image(B, 8 * L, 8 * L, 3)
    il = eng.ip2p_prepare(img)
    assert lib.agd_ip2p_set_hw(eng.ctx, None, B, L, L, C.c_float(1.5), None) == 0
    a = eng.denoise(nz.clone(), *DDIM2, 7.5).cpu()
    eng.ip2p_set(il, 1.5)
    b = eng.denoise(nz.clone(), *DDIM2, 7.5).cpu()
    eng.ip2p_clear()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert lib.agd_ip2p_set_hw(eng.ctx, None, B, L, L, C.c_float(1.5), None) != 0             # clear forgot the prepared latents
    eng.ip2p_prepare(img[:1])
    assert lib.agd_ip2p_set_hw(eng.ctx, None, B, L, L, C.c_float(1.5), None) != 0             # one image prepared, two asked for
    assert b"agd_ip2p_prepare_hw left 1 images" in lib.agd_last_error(eng.ctx)
    eng.close()


def test_unet_forward_returns_the_latent_channels_for_a_wider_sample():
    """`unet(sample)` of an 8-channel ip2p sample and of a 9-channel inpainting sample comes back [B, 4, L, L]."""
    from agenda_amd import StableDiffusionInpaintPipeline, config, synthetic
    B, L = 2, 16
    pipe = _pipe()
    ctx = synthetic.make_context(pipe.cfg, 1, seed=2)
    out = pipe.unet(torch.randn(B, 8, L, L), 500.0, encoder_hidden_states=ctx).sample
    pipe.engine.close()
    assert tuple(out.shape) == (B, 4, L, L) and torch.isfinite(out).all()
    p9 = StableDiffusionInpaintPipeline.from_synthetic("tiny", seed=11, workspace_bytes=2 << 30)
    assert p9.cfg.unet.in_channels == 9
    out9 = p9.unet(torch.randn(B, 9, L, L), 500.0, encoder_hidden_states=ctx).sample
    p9.engine.close()
    assert tuple(out9.shape) == (B, 4, L, L) and torch.isfinite(out9).all()


# ---- checkpoint round trip, LoRA, CLI ---------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_lora(tmp_path):
    from _util import write_tiny_checkpoint
    from agenda_amd import StableDiffusionInstructPix2PixPipeline, StableDiffusionPipeline, synthetic
    cfg = _cfg()
    u, v = _weights()
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, u, v, scheduler="DDIMScheduler")
    uc = os.path.join(ck, "unet", "config.json")
    with open(uc) as f:
        j = json.load(f)
    j["in_channels"] = cfg.unet.in_channels
    with open(uc, "w") as f:
        json.dump(j, f)
    pipe = StableDiffusionInstructPix2PixPipeline.from_pretrained(ck)
    assert pipe.cfg.unet.in_channels == 8
    out2 = str(tmp_path / "saved")
    pipe.save_pretrained(out2)
    with open(os.path.join(out2, "model_index.json")) as f:
        assert json.load(f)["_class_name"] == "StableDiffusionInstructPix2PixPipeline"
    pipe2 = StableDiffusionInstructPix2PixPipeline.from_pretrained(out2)
    B, L = 2, 16
    ctx, img, nz = synthetic.make_context(cfg, B, seed=3), _image(1, 8 * L, 8 * L, 4), _noise(cfg, B, L, L, 5)
    run = lambda p, **kw: p(prompt_embeds=ctx, image=img, latents=nz, num_inference_steps=2, output_type="latent", **kw).latents.cpu()
    base = run(pipe)
    assert torch.equal(base, run(pipe2))                       # one image shared by both rows; the reloaded checkpoint edits alike
    plain = StableDiffusionPipeline.from_pretrained(out2)      # the txt2img pipeline keeps refusing the 8-channel checkpoint
    with pytest.raises(ValueError, match="StableDiffusionInstructPix2PixPipeline"):
        plain(prompt_embeds=ctx, latents=nz, num_inference_steps=2)
    plain.engine.close()
    # LoRA: scale 0 is the base, scale 1 moves the result, unloading restores it bit for bit
    g = torch.Generator().manual_seed(0)
    key = "unet.down_blocks.0.attentions.0.transformer_blocks.0.attn2.processor.to_q_lora"
    wq = u["down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_q.weight"]
    sd = {key + ".down.weight": 0.3 * torch.randn(4, wq.shape[1], generator=g), key + ".up.weight": 0.3 * torch.randn(wq.shape[0], 4, generator=g)}
    pipe.load_lora_weights(sd)
    assert torch.equal(run(pipe, cross_attention_kwargs={"scale": 0.0}), base)
    assert not torch.equal(run(pipe, cross_attention_kwargs={"scale": 1.0}), base)
    pipe.unload_lora_weights()
    assert torch.equal(run(pipe), base)
    pipe.engine.close(); pipe2.engine.close()


def test_cli_writes_images_and_heat_maps(tmp_path):
    from PIL import Image
    d = tmp_path / "src"
    d.mkdir()
    g = np.random.default_rng(0)
    for n in ("a.png", "b.png"):
        Image.fromarray(g.integers(0, 256, (128, 128, 3), dtype=np.uint8)).save(d / n)
    save = tmp_path / "out"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--synthetic-config", "tiny", "--instruct-image", str(d), "--image-guidance-scale", "1.2",
           "--save-dir", str(save), "--num-images", "3", "--batch-size", "3", "--num-inference-steps", "3", "--image-size", "128",
           "--word_token_heatmaps", "cars", "--prompt", "add cars to the road"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for sub in ("images", "daam_cars_heatmaps"):
        assert sorted(os.listdir(save / sub)) == ["0.png", "1.png", "2.png"], (sub, os.listdir(save))
    assert Image.open(save / "images" / "0.png").size == (128, 128)
