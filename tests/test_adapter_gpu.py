"""T2I-Adapter on the device: the four features and one injected UNet forward against the fp32 restatement (tests/_adapter_restated.py),
`pipe(prompt, image=...)` end to end under DDIM, PNDM and DPM-Solver++ with DAAM on, the factor rule, scale 0 / factor 0 against the plain
pipeline bit for bit, the CFG-shared loop at SD-1.5 widths, the error contract, and the checkpoint + CLI round trip."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _adapter_restated as R
from _report import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, want):
    got = got.detach().float().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def _rms_rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


_W = {}


def _weights(name, in_channels=3):
    """(cfg, acfg, unet, vae, adapter) of a config, drawn once per session: the tiny configs with biases and norm perturbations as the tiny
    parity tests draw them; the adapter at gain 1 (tests/test_adapter_cpu.py checks on the CPU that it moves the restated forward by
    more than 0.15 rms-rel at the tiny cases; 0.46 at sd15, L = 32)."""
    key = (name, in_channels)
    if key not in _W:
        from agenda_amd import config, synthetic
        cfg = config.CONFIGS[name]()
        small = name != "sd15"
        kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
        acfg = config.adapter_config_for(cfg.unet, in_channels)
        u = synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw)
        v = synthetic.make_vae_weights(cfg, 12 if small else 1235, **kw)
        a = synthetic.make_adapter_weights(cfg, acfg, seed=15 if small else 1237, gain=1.0, bias_std=0.05 if small else 0.0)
        _W[key] = (cfg, acfg, u, v, a)
    return _W[key]


def _pipe(cfg, acfg, u, v, a, scheduler="DDIMScheduler", ws=2 << 30, cls=None):
    from agenda_amd import StableDiffusionAdapterPipeline, T2IAdapter
    return (cls or StableDiffusionAdapterPipeline)(cfg, u, v, adapter=T2IAdapter.from_config(acfg, a), workspace_bytes=ws, scheduler=scheduler)


def _image(b, c, h, w, seed, u8=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(b, c, h, w, generator=g)
    if u8:
        return (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return x


def _as_float(img):
    return img.permute(0, 3, 1, 2).float() / 255.0 if img.dtype == torch.uint8 else img


# config, latent height, latent width, images, uint8 image, adapter in_channels.  Rows per map: tiny 16 x 16 -> 256 / 64 / 16 / 4 (no in_conv
# between the equal-width levels); tiny21 24 x 24 -> 576 / 144 / 36 / 9 (ragged); 16 x 24 -> 384 / 96 / 24 / 6; sd15 32 x 32 -> 1024 / 256 /
# 64 / 16 at 320 / 640 / 1280 / 1280 channels (both in_convs, the 192-channel first conv)
CASES = [("tiny", 16, 16, 2, False, 3), ("tiny21", 24, 24, 2, False, 3), ("tiny", 16, 24, 2, True, 3), ("tiny", 16, 16, 2, False, 1),
         ("sd15", 32, 32, 1, False, 3)]
_ID = lambda c: f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}" + ("-u8" if c[4] else "") + (f"-C{c[5]}" if c[5] != 3 else "")


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_features_match_restatement(case):
    name, Lh, Lw, B, u8, cin = case
    cfg, acfg, u, v, a = _weights(name, cin)
    pipe = _pipe(cfg, acfg, u, v, a, ws=(6 if name == "sd15" else 2) << 30)
    img = _image(B, cin, 8 * Lh, 8 * Lw, 21, u8)
    pipe.engine.adapter_set_cond(img)
    got = [f.cpu() for f in pipe.engine.adapter_features()]
    with torch.no_grad():
        want = R.adapter_forward(a, acfg, _as_float(img))
    assert [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    errs = [_rms_rel(g, w) for g, w in zip(got, want)]
    print(f"adapter features {_ID(case)}: rms rel {', '.join(f'{e:.4f}' for e in errs)}")
    report(f"adapter_features[{_ID(case)}]", rms_rel_max=max(errs))
    assert max(errs) < 0.03, errs
    pipe.engine.close()


# (adds with GroupNorm partial sums, adds without) of one forward: a 64-row statistics tile needs HW % 64 == 0
_COUNTS = {("tiny", 16, 16): (2, 2), ("tiny21", 24, 24): (1, 3), ("tiny", 16, 24): (1, 3), ("sd15", 32, 32): (3, 1)}


@pytest.mark.parametrize("case", [c for c in CASES if c[5] == 3], ids=_ID)
def test_injected_unet_forward_matches_restatement(case):
    """One UNet forward of two rows with a one-element schedule at scale 1.  Stale GroupNorm statistics of an injected skip (the up path's
    concat norm, the mid block's first norm) would show here.  Both forms of the add run: with the partial sums and, with
    gn_fused_stats off, without them."""
    name, Lh, Lw, B, u8, cin = case
    from agenda_amd import synthetic
    cfg, acfg, u, v, a = _weights(name, cin)
    pipe = _pipe(cfg, acfg, u, v, a, ws=(6 if name == "sd15" else 2) << 30)
    e = pipe.engine
    rows = 2
    ctx = synthetic.make_context(cfg, rows // 2, seed=6)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, 4, Lh, Lw, generator=g)
    img = _image(B, cin, 8 * Lh, 8 * Lw, 22, u8)
    t = 301.0
    e.set_context(ctx)
    e.adapter_set_cond(img)
    plain = e.unet_forward(x, t).cpu()
    c0 = e.adapter_add_counts()
    e.adapter_set_schedule([1.0])
    got = e.unet_forward(x, t).cpu()
    c1 = e.adapter_add_counts()
    e.set_option("gn_fused_stats", 0)                    # no partial sums anywhere: every add takes the cpart_bm = 0 form
    got_fb = e.unet_forward(x, t).cpu()
    c2 = e.adapter_add_counts()
    e.set_option("gn_fused_stats", 1)
    e.adapter_set_schedule([])
    assert torch.equal(e.unet_forward(x, t).cpu(), plain)                 # the schedule cleared: the plain UNet again, bit for bit
    with torch.no_grad():                                # one image at a time (the oracle's attention holds every score)
        feats = R.adapter_forward(a, acfg, _as_float(img))
        want = torch.cat([R.adapted_eps(u, cfg.unet, x[i:i + 1], t, ctx[i:i + 1], [f[i % B:i % B + 1] for f in feats], 1.0) for i in range(rows)])
    err, err_fb, moved, both = _rms_rel(got, want), _rms_rel(got_fb, want), _rms_rel(plain, want), _rms_rel(got_fb, got)
    print(f"injected unet {_ID(case)}: rms rel {err:.4f} (statistics pass: {err_fb:.4f}, the two {both:.4f} apart; the un-injected forward is {moved:.3f} away); "
          f"adds with / without partial sums {tuple(b_ - a_ for a_, b_ in zip(c0, c1))}")
    report(f"adapter_injected_unet[{_ID(case)}]", rms_rel=err, rms_rel_stats_pass=err_fb)
    assert c0 == (0, 0)
    assert tuple(b_ - a_ for a_, b_ in zip(c0, c1)) == _COUNTS[(name, Lh, Lw)]
    assert tuple(b_ - a_ for a_, b_ in zip(c1, c2)) == (0, 4)
    assert moved > 5 * err, (moved, err)                 # the features matter at this scale
    assert err < 0.03, err
    assert err_fb < 0.03 and both < 0.03, (err_fb, both)
    pipe.engine.close()


def test_cfg_shared_prefix_at_sd15_widths_matches_unshared_forwards():
    """SD-1.5 shapes at 256 px: the fused DDIM loop (the CFG halves share everything ahead of the first attn2; the rows are back to B2
    before the first add) against the same steps through unshared `unet_forward` calls of the CFG pair + `cfg_ddim_step`."""
    from agenda_amd import synthetic
    cfg, acfg, u, v, a = _weights("sd15")
    pipe = _pipe(cfg, acfg, u, v, a, ws=6 << 30)
    B, L, steps, g, scale = 1, 32, 3, 7.5, 0.9
    ctx = synthetic.make_context(cfg, B, seed=8)
    lat0 = synthetic.make_latents(cfg, [9], L)
    img = _image(B, 3, 8 * L, 8 * L, 25)
    fused = pipe(prompt_embeds=ctx, image=img, latents=lat0, num_inference_steps=steps, guidance_scale=g, output_type="latent",
                 adapter_conditioning_scale=scale).latents.cpu()
    pipe.scheduler.set_timesteps(steps)
    a_t, a_p = pipe.scheduler.step_coeffs()
    pipe.engine.set_context(ctx)
    pipe.engine.adapter_set_cond(img)
    x = lat0.clone().cuda().contiguous()
    for i, t in enumerate(pipe.scheduler.timesteps):
        pipe.engine.adapter_set_schedule([scale])
        eps = pipe.engine.unet_forward(torch.cat([x, x]).contiguous(), float(t))
        pipe.engine.cfg_ddim_step(eps, x, g, float(a_t[i]), float(a_p[i]))
    pipe.engine.adapter_set_schedule([])
    err = _rms_rel(fused, x)
    print(f"adapter fused (CFG-shared) vs unshared DDIM loop, SD-1.5 256 px: rms rel {err:.2e}")
    report("adapter_cfg_shared_vs_unshared[sd15,256px]", latents_rms_rel=err)
    assert err < 1e-3, err
    pipe.engine.close()


def _run(scheduler, sched_key, scale=1.0, factor=1.0, steps=6):
    from agenda_amd import synthetic, trace
    from oracle import sd_oracle as O
    cfg, acfg, u, v, a = _weights("tiny")
    pipe = _pipe(cfg, acfg, u, v, a, scheduler=scheduler)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    u8 = _image(B, 3, 8 * L, 8 * L, 23, u8=True)
    rec = O.DaamRecorder(L * L, context_size=cfg.max_tokens)
    want_img, want_lat = R.generate(u, v, a, cfg, acfg, ctx, lat, _as_float(u8), steps, sched_key, scale=scale, factor=factor, recorder=rec)
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, image=u8, latents=lat, num_inference_steps=steps, output_type="np",
                   adapter_conditioning_scale=scale, adapter_conditioning_factor=factor)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    whm = rec.compute_global_heat_map()
    pipe.engine.close()
    return out, hm, want_img, want_lat, whm


@pytest.mark.parametrize("scheduler,key,n_evals,scale,factor", [("DDIMScheduler", "ddim", 6, 1.0, 1.0), ("PNDMScheduler", "pndm", 7, 1.0, 1.0),
                                                                  ("DPMSolverMultistepScheduler", "dpm", 6, 1.0, 1.0),
                                                                  ("DDIMScheduler", "ddim", 6, 0.7, 0.5)])
def test_pipeline_matches_restatement(scheduler, key, n_evals, scale, factor):
    out, hm, want_img, want_lat, whm = _run(scheduler, key, scale, factor)
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(hm, whm)
    tag = key if (scale, factor) == (1.0, 1.0) else f"{key},scale={scale},factor={factor}"
    print(f"adapter pipe {tag}: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map rel {e_hm:.4f}")
    report(f"adapter_pipeline[{tag}]", latents_rms_rel=e_lat, psnr_db=psnr, heat_map_rel=e_hm)
    assert e_lat < 0.06, e_lat
    assert psnr > 30.0, psnr
    assert e_hm < 0.06, e_hm
    # the plain pipeline's recorded evaluation count: the adapter has no attention
    assert float(hm.sum(1).mean()) == pytest.approx(n_evals, rel=0.02)


@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_scale_zero_and_factor_zero_are_bit_identical_to_the_plain_pipeline(scheduler):
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    cfg, acfg, u, v, a = _weights("tiny")
    B, L, steps = 2, 16, 5
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    res = []
    for kw in (None, dict(adapter_conditioning_scale=0.0), dict(adapter_conditioning_factor=0.0)):
        pipe = StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30, scheduler=scheduler) if kw is None else _pipe(cfg, acfg, u, v, a, scheduler=scheduler)
        kw = {} if kw is None else dict(kw, image=_image(1, 3, 8 * L, 8 * L, 3))
        with trace(pipe) as trc:
            out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="np", **kw)
            hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
        res.append((out.latents.cpu(), out.images, hm))
        pipe.engine.close()
    for r in res[1:]:
        assert torch.equal(res[0][0], r[0])
        assert np.array_equal(res[0][1], r[1])
        assert torch.equal(res[0][2], r[2])


def test_two_identical_adapter_calls_are_bit_identical():
    from agenda_amd import synthetic, trace
    cfg, acfg, u, v, a = _weights("tiny")
    pipe = _pipe(cfg, acfg, u, v, a)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=43)
    lat = synthetic.make_latents(cfg, [6, 7], L)
    img = _image(B, 3, 8 * L, 8 * L, 4)
    res = []
    for _ in range(2):
        with trace(pipe) as trc:
            out = pipe(prompt_embeds=ctx, image=img, latents=lat, num_inference_steps=4, output_type="np")
            hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
        res.append((out.latents.cpu(), out.images, hm))
    plain = pipe(prompt_embeds=ctx, image=img, latents=lat, num_inference_steps=4, output_type="latent", adapter_conditioning_scale=0.0).latents.cpu()
    pipe.engine.close()
    assert torch.equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert not torch.equal(res[0][0], plain)             # (and the features did something)


def test_engine_error_contract():
    """Every engine refusal, matched by message; the schedule is left clear afterwards and the engine still runs the plain UNet."""
    from agenda_amd import StableDiffusionAdapterPipeline, _lib, config, synthetic
    from agenda_amd import gligen as G
    cfg, acfg, u, v, a = _weights("tiny")
    pipe = _pipe(cfg, acfg, u, v, a)
    e = pipe.engine
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=1)
    lat = synthetic.make_latents(cfg, [0, 1], L)
    x = torch.cat([lat, lat]).cuda()
    e.set_context(ctx)
    plain = e.unet_forward(x, 11.0).cpu()
    pipe.scheduler.set_timesteps(4)
    a_t, a_p = pipe.scheduler.step_coeffs()
    denoise = lambda eng=e: eng.denoise(lat.clone().cuda(), pipe.scheduler.timesteps, a_t, a_p, 7.5)
    # a schedule before any features
    e.adapter_set_schedule([1.0])
    with pytest.raises(_lib.AgendaHipError, match="features are set for 0 images"):
        e.unet_forward(x, 11.0)
    with pytest.raises(_lib.AgendaHipError, match="no features set"):
        e.adapter_features()
    # a schedule length that does not match
    e.adapter_set_cond(_image(2, 3, 128, 128, 1))
    e.adapter_set_schedule([1.0, 1.0])
    with pytest.raises(_lib.AgendaHipError, match="schedule has 2 scales, this call runs 1"):
        e.unet_forward(x, 11.0)
    e.adapter_set_schedule([1.0] * 3)
    with pytest.raises(_lib.AgendaHipError, match="schedule has 3 scales, this call runs 4"):
        denoise()
    # features set for other sizes or rows
    e.adapter_set_schedule([1.0] * 4)
    e.adapter_set_cond(_image(2, 3, 128, 192, 1))
    with pytest.raises(_lib.AgendaHipError, match="features are set for 2 images at latent sides 16 x 24"):
        denoise()
    e.adapter_set_cond(_image(3, 3, 128, 128, 1))
    with pytest.raises(_lib.AgendaHipError, match="features are set for 3 images"):
        denoise()
    with pytest.raises(_lib.AgendaHipError, match="multiple of 64"):
        e.adapter_set_cond(_image(1, 3, 128, 96, 1))
    with pytest.raises(ValueError, match="channels"):
        e.adapter_set_cond(_image(1, 1, 128, 128, 1))
    e.adapter_set_cond(_image(2, 3, 128, 128, 1))
    # per-image timesteps, a panorama, an inpainting state
    e.adapter_set_schedule([1.0])
    with pytest.raises(_lib.AgendaHipError, match="unet_forward_ts: a T2I-Adapter schedule"):
        e.unet_forward(x, [11.0, 12.0, 13.0, 14.0])
    e.adapter_set_schedule([1.0] * 4)
    with pytest.raises(_lib.AgendaHipError, match="denoise_panorama: a T2I-Adapter schedule"):
        e.denoise_panorama(torch.zeros(2, 4, 16, 32, device="cuda"), 16, 8, None, pipe.scheduler.timesteps, a_t, a_p, 7.5)
    e.inpaint_set(torch.ones(2, 1, L, L), torch.zeros(2, 4, L, L), torch.zeros(2, 4, L, L))
    e.inpaint_set_schedule([(1.0, 0.0)] * 4)
    with pytest.raises(_lib.AgendaHipError, match="adapter: an inpainting state"):
        denoise()
    e.inpaint_clear()
    # nothing above left a mark: the same schedule runs, and cleared, the plain UNet comes back bit for bit
    denoise()
    e.adapter_clear()
    assert torch.equal(e.unet_forward(x, 11.0).cpu(), plain)
    e.close()

    # the adapter beside a ControlNet and beside GLIGEN: engines that load both
    cn = synthetic.make_controlnet_weights(cfg, seed=13, bias_std=0.05, perturb_norm=0.1)

    class WithControlNet(StableDiffusionAdapterPipeline):
        def _load_extra(self):
            super()._load_extra()
            self.engine.controlnet_configure(config.ControlNetConfig())
            self.engine.load_state_dict(cn, "controlnet.")

    e = _pipe(cfg, acfg, u, v, a, cls=WithControlNet).engine
    e.set_context(ctx)
    e.adapter_set_cond(_image(2, 3, 128, 128, 1))
    e.adapter_set_schedule([1.0])
    e.controlnet_set_schedule([0.0])
    with pytest.raises(_lib.AgendaHipError, match="adapter: a ControlNet schedule"):
        e.unet_forward(x, 11.0)
    e.controlnet_set_schedule([])
    e.unet_forward(x, 11.0)
    e.close()

    gl = G.make_gligen_weights(cfg, 13)

    class WithGligen(StableDiffusionAdapterPipeline):
        def _load_extra(self):
            super()._load_extra()
            self.engine.gligen_configure(cfg.unet.cross_attention_dim, G.MAX_OBJS, G.FOURIER_FREQS)
            self.engine.load_state_dict(gl, "unet.")

    e = _pipe(cfg, acfg, u, v, a, cls=WithGligen).engine
    e.set_context(ctx)
    e.adapter_set_cond(_image(2, 3, 128, 128, 1))
    e.adapter_set_schedule([1.0])
    e.gligen_set_schedule([0])
    with pytest.raises(_lib.AgendaHipError, match="adapter: a GLIGEN schedule"):
        e.unet_forward(x, 11.0)
    e.gligen_set_schedule([])
    e.unet_forward(x, 11.0)
    e.close()

    # an InstructPix2Pix state: an 8-channel UNet
    icfg = config.ip2p_variant(cfg)
    ui = synthetic.make_unet_weights(icfg, 11, bias_std=0.05, perturb_norm=0.1)
    e = _pipe(icfg, acfg, ui, v, a).engine
    e.set_context(ctx)
    e.adapter_set_cond(_image(2, 3, 128, 128, 1))
    e.adapter_set_schedule([1.0] * 4)
    e.ip2p_set(torch.zeros(2, 4, L, L), 1.5)
    with pytest.raises(_lib.AgendaHipError, match="ip2p: a T2I-Adapter schedule"):
        denoise(e)
    e.close()

    # finalize names what does not fit the UNet
    bad = config.AdapterConfig(channels=(64, 128, 128))
    with pytest.raises(_lib.AgendaHipError, match="channels has 3 entries, the UNet has 4 levels"):
        _pipe(cfg, bad, u, v, synthetic.make_adapter_weights(cfg, bad, seed=1))
    bad = config.AdapterConfig(channels=(64, 128, 128, 256))
    with pytest.raises(_lib.AgendaHipError, match=r"channels\[3\] = 256"):
        _pipe(cfg, bad, u, v, synthetic.make_adapter_weights(cfg, bad, seed=1))
    bad = config.AdapterConfig(channels=tuple(cfg.unet.block_out_channels), downscale_factor=4)
    with pytest.raises(_lib.AgendaHipError, match="downscale_factor = 4"):
        _pipe(cfg, bad, u, v, synthetic.make_adapter_weights(cfg, bad, seed=1))
    short = {k: t for k, t in a.items() if "body.1.in_conv" not in k}
    with pytest.raises(_lib.AgendaHipError, match="body.1.in_conv"):
        _pipe(cfg, acfg, u, v, short)
    wrong = dict(a)
    wrong["adapter.body.2.resnets.1.block2.weight"] = torch.zeros(128, 128, 3, 3)
    with pytest.raises(_lib.AgendaHipError, match="body.2.resnets.1.block2"):
        _pipe(cfg, acfg, u, v, wrong)


def test_python_error_contract():
    from agenda_amd import StableDiffusionAdapterPipeline, T2IAdapter, synthetic
    cfg, acfg, u, v, a = _weights("tiny")
    pipe = _pipe(cfg, acfg, u, v, a)
    ctx = synthetic.make_context(cfg, 2, seed=1)
    lat = synthetic.make_latents(cfg, [0, 1], 16)
    kw = dict(prompt_embeds=ctx, latents=lat, num_inference_steps=2, output_type="latent")
    with pytest.raises(ValueError, match="channels"):
        pipe(image=_image(1, 1, 128, 128, 1), **kw)
    with pytest.raises(ValueError, match="multiple of 64"):
        pipe(image=_image(1, 3, 96, 128, 1), **kw)
    with pytest.raises(ValueError, match="output"):
        pipe(image=_image(1, 3, 128, 128, 1), height=64, width=64, **kw)
    with pytest.raises(ValueError, match="batch"):
        pipe(image=_image(3, 3, 128, 128, 1), **kw)
    with pytest.raises(NotImplementedError):
        pipe(image=_image(1, 3, 128, 128, 1), adapter_conditioning_scale=[1.0, 0.5], **kw)
    with pytest.raises(NotImplementedError):
        pipe.img2img(prompt_embeds=ctx, image=torch.rand(2, 3, 128, 128))
    m = T2IAdapter.from_config(acfg, a)
    with pytest.raises(NotImplementedError):
        StableDiffusionAdapterPipeline(cfg, u, v, adapter=[m, m])
    with pytest.raises(NotImplementedError):
        StableDiffusionAdapterPipeline(cfg, u, v, adapter=T2IAdapter(dict(m.config, adapter_type="light_adapter"), a))
    # a refused call leaves no schedule behind: one image serves both prompts, rectangular sizes follow the image
    out = pipe(image=_image(1, 3, 128, 192, 1), prompt_embeds=ctx, latents=torch.randn(2, 4, 16, 24), num_inference_steps=2, output_type="np")
    assert out.images.shape == (2, 128, 192, 3)
    pipe.engine.close()


def test_from_synthetic_builds_an_adapter_that_fits_the_unet():
    from agenda_amd import StableDiffusionAdapterPipeline, config
    pipe = StableDiffusionAdapterPipeline.from_synthetic("tiny", seed=5, workspace_bytes=2 << 30)
    assert pipe.adapter_cfg == config.adapter_config_for(pipe.cfg.unet)
    assert set(pipe.adapter.state_dict) == set(config.adapter_param_shapes(pipe.cfg.unet, pipe.adapter_cfg))
    img = _image(1, 3, 128, 128, 2)
    kw = dict(prompt=["a", "b"], image=img, num_inference_steps=2, output_type="latent", generator=torch.Generator().manual_seed(0))
    on = pipe(**kw).latents.cpu()
    kw["generator"] = torch.Generator().manual_seed(0)
    off = pipe(adapter_conditioning_scale=0.0, **kw).latents.cpu()
    pipe.engine.close()
    assert on.shape == (2, 4, 16, 16) and torch.isfinite(on).all() and not torch.equal(on, off)


def test_checkpoint_round_trip_and_cli(tmp_path):
    from PIL import Image
    from _util import write_tiny_checkpoint
    from agenda_amd import StableDiffusionAdapterPipeline, StableDiffusionPipeline, T2IAdapter
    from agenda_amd.generation import adapter_images_for, generate_batch, save_outputs
    cfg, acfg, u, v, a = _weights("tiny")
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, u, v, scheduler="DDIMScheduler")
    T2IAdapter.from_config(acfg, a).save_pretrained(os.path.join(ck, "adapter"))
    img_dir = tmp_path / "cond"
    img_dir.mkdir()
    g = np.random.default_rng(0)
    for n in ("a.png", "b.png"):
        Image.fromarray(g.integers(0, 256, (96, 80, 3), dtype=np.uint8)).save(img_dir / n)      # a size that needs resizing
    pipe = StableDiffusionAdapterPipeline.from_pretrained(ck, adapter=T2IAdapter.from_pretrained(os.path.join(ck, "adapter")))
    out2 = str(tmp_path / "saved")
    pipe.save_pretrained(out2)
    with open(os.path.join(out2, "model_index.json")) as f:
        assert json.load(f)["adapter"] == ["diffusers", "T2IAdapter"]
    pipe2 = StableDiffusionAdapterPipeline.from_pretrained(out2)          # found through model_index.json
    seeds = [0, 1, 2]
    files = sorted(str(img_dir / n) for n in os.listdir(img_dir))
    ctl = {"image": adapter_images_for(files, seeds), "adapter_conditioning_scale": 0.7}
    imgs, hms = generate_batch(pipe2, seeds, ["cars"], prompt="an aerial view with cars", num_inference_steps=3, control=ctl, height=128, width=128)
    imgs, hms = imgs.cpu().numpy(), hms.cpu()
    # seeds 0 and 2 share a conditioning image, seed 1 takes the other
    picked = [np.asarray(im) for im in ctl["image"]]
    assert np.array_equal(picked[0], picked[2]) and not np.array_equal(picked[0], picked[1])
    assert np.array_equal(picked[1], np.asarray(Image.open(files[1]).convert("RGB")))
    same = {"image": [ctl["image"][0]] * 3, "adapter_conditioning_scale": 0.7}     # every seed under the first image: only seed 1 changes
    alt, _ = generate_batch(pipe2, seeds, ["cars"], prompt="an aerial view with cars", num_inference_steps=3, control=same, height=128, width=128)
    alt = alt.cpu().numpy()
    assert _psnr(alt[0], imgs[0]) > 40.0 and _psnr(alt[2], imgs[2]) > 40.0
    assert _psnr(alt[1], imgs[1]) < 40.0
    pipe.engine.close(); pipe2.engine.close()
    plain = StableDiffusionPipeline.from_pretrained(out2)
    pimgs, _ = generate_batch(plain, seeds, ["cars"], prompt="an aerial view with cars", num_inference_steps=3, height=128, width=128)
    plain.engine.close()
    assert not np.array_equal(pimgs.cpu().numpy(), imgs)                 # the outputs differ from the plain pipeline's
    save = tmp_path / "cli"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--pretrained-model-path", out2, "--adapter-model-path", os.path.join(out2, "adapter"),
           "--adapter-image", str(img_dir), "--adapter-conditioning-scale", "0.7", "--save-dir", str(save), "--num-images", "3",
           "--batch-size", "3", "--num-inference-steps", "3", "--image-size", "128", "--word_token_heatmaps", "cars",
           "--prompt", "an aerial view with cars"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the CLI writes the API's images and heat maps: the same files, byte for byte
    ref = tmp_path / "api"
    save_outputs(str(ref), seeds, torch.from_numpy(imgs), hms, ["cars"], 128)
    want = sorted(os.path.relpath(os.path.join(d, f), ref) for d, _, fs in os.walk(ref) for f in fs)
    got = sorted(os.path.relpath(os.path.join(d, f), save) for d, _, fs in os.walk(save) for f in fs)
    assert want and want == got, (want, got)
    for p in want:
        with open(ref / p, "rb") as fa, open(save / p, "rb") as fb:
            assert fa.read() == fb.read(), p
