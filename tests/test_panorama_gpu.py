"""MultiDiffusion panorama on the device: the window gather and the overlap mean as ops, the one-view identity with the plain pipeline,
the fused loop against its host-composed form, and the pipeline end to end (latents, decoded image, canvas heat map, per-view DAAM
states) against the fp32 restatement in tests/_panorama_restated.py."""
import math

import numpy as np
import pytest
import torch

import _panorama_restated as R
from _report import report

pytestmark = pytest.mark.gpu

CANVASES = {"tiny": [(16, 40), (40, 16), (32, 32)], "tiny21": [(24, 48), (48, 24), (40, 40)]}     # latent units; 4, 4 and 9 views


def _rms_rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def _psnr(a, b):
    mse = np.mean((np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _latents(cfg, seeds, lh, lw):
    return torch.cat([torch.randn(1, cfg.unet.out_channels, lh, lw, generator=torch.Generator("cpu").manual_seed(int(s))) for s in seeds], 0)


def _tiny(name="tiny", cls=None):
    from agenda_amd import StableDiffusionPanoramaPipeline, config, synthetic
    cfg = config.CONFIGS[name]()
    seeds = (11, 12) if name == "tiny" else (31, 32)
    u = synthetic.make_unet_weights(cfg, seeds[0], bias_std=0.05, perturb_norm=0.1)
    v = synthetic.make_vae_weights(cfg, seeds[1], bias_std=0.05, perturb_norm=0.1)
    return (cls or StableDiffusionPanoramaPipeline)(cfg, u, v, workspace_bytes=2 << 30), cfg, u, v


# ---- ops ------------------------------------------------------------------------------------------------------------------------
OP_SHAPES = [(1, 4, 16, 40, 16), (2, 4, 40, 16, 16), (2, 4, 32, 32, 16), (1, 77, 32, 40, 16), (1, 4, 64, 256, 64), (2, 4, 128, 128, 64),
             (1, 77, 64, 128, 64), (1, 4, 96, 192, 96), (2, 4, 192, 96, 96), (1, 77, 112, 112, 96)]


@pytest.mark.parametrize("B,C,lh,lw,win", OP_SHAPES)
def test_window_gather_is_bit_exact(B, C, lh, lw, win):
    from agenda_amd import ops
    x = torch.randn(B, C, lh, lw, generator=torch.Generator().manual_seed(lh * lw + C)).cuda()
    want = R.slice_views(x, win)
    got = ops.window_gather(x, win, 8)
    assert got.shape == want.shape and torch.equal(got, want)
    V = want.shape[0] // B
    if V > 2:                                             # a chunk of views: [1, V - 1)
        part = ops.window_gather(x, win, 8, v0=1, n=V - 2)
        assert torch.equal(part, want.reshape(B, V, C, win, win)[:, 1:V - 1].reshape(-1, C, win, win))


@pytest.mark.parametrize("B,C,lh,lw,win", OP_SHAPES)
def test_window_mean_matches_restated_value_over_count(B, C, lh, lw, win):
    """rtol 1e-5 covers any reordering of the at most (96 / 8)^2 = 144 terms of a pixel (144 x 2^-24 ~ 8.6e-6); the kernel adds in
    diffusers' view order, so bit-identity with the fp32 restatement is expected and reported."""
    from agenda_amd import ops
    V = len(R.get_views(lh, lw, win))
    views = torch.randn(B * V, C, win, win, generator=torch.Generator().manual_seed(V + C))
    want = R.overlap_mean(views, B, lh, lw)
    got = ops.window_mean(views.cuda(), B, lh, lw, 8).cpu()
    exact = bool(torch.equal(got, want))
    worst = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
    print(f"window_mean B={B} C={C} {lh}x{lw} win={win}: {V} views, bit-identical={exact}, worst rel {worst:.3e}")
    report(f"panorama_window_mean[{B},{C},{lh}x{lw},{win}]", bit_identical=int(exact), worst_rel=worst)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=0)


def test_window_ops_refuse_bad_geometry():
    from agenda_amd import _lib, ops
    x = torch.zeros(1, 4, 16, 16).cuda()
    with pytest.raises(_lib.AgendaHipError, match="window 24"):
        ops.window_gather(x, 24, 8)
    with pytest.raises(_lib.AgendaHipError, match=r"views \[3, 5\) of 4"):
        ops.window_gather(torch.zeros(1, 4, 16, 40).cuda(), 16, 8, v0=3, n=2)


# ---- one view = the plain pipeline ----------------------------------------------------------------------------------------------
def test_one_view_is_bit_identical_to_the_plain_pipeline():
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    pano, cfg, u, v = _tiny("tiny")
    plain = StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=5)
    lat = synthetic.make_latents(cfg, [3, 4], L)
    outs = []
    for pipe in (plain, pano):
        with trace(pipe) as trc:
            out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=3, height=8 * L, width=8 * L, output_type="pt")
            hms = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
        outs.append((out.latents.cpu(), out.images.cpu(), hms))
    assert outs[1][2].shape == (B, cfg.max_tokens, L, L)
    for a, b, what in zip(outs[0], outs[1], ("latents", "images", "heat maps")):
        assert torch.equal(a, b), what
    plain.engine.close(); pano.engine.close()


# ---- the fused loop against the existing entry points ---------------------------------------------------------------------------------
def _host_loop(pipe, ctx, lat, win, steps, g):
    """torch slicing -> engine.denoise for one step on the B * V views -> torch value / count, per step."""
    eng = pipe.engine
    B, _, lh, lw = lat.shape
    V = len(R.get_views(lh, lw, win))
    ts = pipe.scheduler.set_timesteps(steps)
    a_t, a_p = pipe.scheduler.step_coeffs()
    eng.set_context(torch.cat([ctx[:B].repeat_interleave(V, 0), ctx[B:].repeat_interleave(V, 0)], 0))
    x = lat.clone().cuda()
    for s in range(steps):
        views = R.slice_views(x, win).contiguous()
        eng.denoise(views, ts[s:s + 1], a_t[s:s + 1], a_p[s:s + 1], g)
        x = R.overlap_mean(views, B, lh, lw)
    return x.cpu()


@pytest.mark.parametrize("lh,lw", [(16, 40), (32, 32)])
def test_fused_loop_matches_host_composed_loop_tiny(lh, lw, vb=None):
    from agenda_amd import synthetic
    pipe, cfg, u, v = _tiny("tiny")
    B, steps, g, win = 2, 3, 7.5, 16
    ctx = synthetic.make_context(cfg, B, seed=21)
    lat = _latents(cfg, [7, 8], lh, lw)
    want = _host_loop(pipe, ctx, lat, win, steps, g)
    got = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, guidance_scale=g, height=8 * lh, width=8 * lw, view_batch_size=vb,
               output_type="latent").latents.cpu()
    e = _rms_rel(got, want)
    print(f"fused vs host loop {lh}x{lw} view_batch={vb}: latents rms-rel {e:.3e}")
    report(f"panorama_fused_vs_host[tiny,{lh}x{lw},vb={vb}]", latents_rms_rel=e)
    assert e < 1e-4, e
    pipe.engine.close()


def test_fused_loop_matches_host_composed_loop_sd15():
    """SD-1.5 shapes: 512 x 1024 px = 9 views of 64 x 64 latents, B = 1, 2 steps; also finite output and the canvas heat-map shape."""
    from agenda_amd import StableDiffusionPanoramaPipeline, synthetic, trace
    pipe = StableDiffusionPanoramaPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg = pipe.cfg
    B, steps, g, win, lh, lw = 1, 2, 7.5, 64, 64, 128
    ctx = synthetic.make_context(cfg, B, seed=3)
    lat = _latents(cfg, [5], lh, lw)
    want = _host_loop(pipe, ctx, lat, win, steps, g)
    with trace(pipe) as trc:
        got = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, guidance_scale=g, height=512, width=1024, output_type="latent").latents
        hm = trc.compute_global_heat_map(image_index=0).heat_maps
    assert tuple(hm.shape) == (77, 64, 128) and bool(torch.isfinite(hm).all()) and bool(torch.isfinite(got).all())
    assert float(hm.min()) >= 0.0 and float(hm.max()) > 0.0
    e = _rms_rel(got, want)
    print(f"fused vs host loop sd15 512x1024: latents rms-rel {e:.3e}")
    report("panorama_fused_vs_host[sd15,64x128]", latents_rms_rel=e)
    assert e < 1e-4, e
    pipe.engine.close()


# ---- end to end against the restatement -----------------------------------------------------------------------------------------
def _restated(cfg, u, v, ctx, lat, steps, win):
    lh, lw = lat.shape[2:]
    recs = R.view_recorders(lh, lw, win, cfg.max_tokens)
    img, x = R.generate_panorama(u, v, cfg, ctx, lat, steps, 7.5, win, recorders=recs)
    return img, x, R.canvas_heat_map(recs, lh, lw), R.view_heat_maps(recs)


def _run(pipe, ctx, lat, steps, vb=None):
    from agenda_amd import trace
    B, _, lh, lw = lat.shape
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, height=8 * lh, width=8 * lw, view_batch_size=vb, output_type="np")
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
        V = len(R.get_views(lh, lw, pipe.window))
        views = torch.stack([torch.stack([pipe.engine.daam_global(k * B + p, pipe.cfg.max_tokens, pipe.window) for p in range(B)])
                             for k in range(V)]).cpu()                 # [V, B, T, win, win]: state of (panorama p, view k) = k * B + p
    return out.latents.cpu(), out.images, hm, views


@pytest.mark.parametrize("name,lh,lw", [(n, h, w) for n, cs in CANVASES.items() for (h, w) in cs])
def test_panorama_matches_restatement(name, lh, lw):
    """B = 2 distinct contexts, DDIM x 2, decode and DAAM on; the bounds of the square and rectangular tests of the same configs
    (test_model_gpu.py, test_aspect_gpu.py): latents rms-rel < 0.06, PSNR > 30 dB, canvas heat map max-rel < 0.05.  Each panorama of the
    batch also matches its own batch-1 run to the same bounds."""
    from agenda_amd import synthetic
    pipe, cfg, u, v = _tiny(name)
    B, steps, win = 2, 2, pipe.window
    ctx = synthetic.make_context(cfg, B, seed=5)
    lat = _latents(cfg, [3, 4], lh, lw)
    want_img, want_lat, want_hm, _ = _restated(cfg, u, v, ctx, lat, steps, win)
    got_lat, got_img, got_hm, _ = _run(pipe, ctx, lat, steps)
    assert got_img.shape == want_img.shape == (B, 8 * lh, 8 * lw, 3) and got_hm.shape == (B, cfg.max_tokens, lh, lw)
    e_lat, psnr, e_hm = _rms_rel(got_lat, want_lat), _psnr(got_img, want_img), _rel(got_hm, want_hm)
    print(f"{name} {lh}x{lw}: latents {e_lat:.4f}, PSNR {psnr:.1f} dB, canvas heat map {e_hm:.4f}")
    report(f"panorama_txt2img[{name},{lh}x{lw}]", latents_rms_rel=e_lat, psnr=psnr, heat_map_rel=e_hm)
    assert e_lat < 0.06 and psnr > 30.0 and e_hm < 0.05, (e_lat, psnr, e_hm)
    for p in range(B):
        one_lat, one_img, one_hm, _ = _run(pipe, torch.stack([ctx[p], ctx[B + p]]), lat[p:p + 1], steps)
        e1, p1, h1 = _rms_rel(got_lat[p:p + 1], one_lat), _psnr(got_img[p:p + 1], one_img), _rel(got_hm[p:p + 1], one_hm)
        print(f"{name} {lh}x{lw}: panorama {p} of the batch against its batch-1 run: latents {e1:.2e}, PSNR {p1:.1f} dB, heat map {h1:.2e}")
        report(f"panorama_batch1[{name},{lh}x{lw},{p}]", latents_rms_rel=e1, psnr=p1, heat_map_rel=h1)
        assert e1 < 0.06 and p1 > 30.0 and h1 < 0.05, (p, e1, p1, h1)
    pipe.engine.close()


def test_view_batch_sizes_and_per_view_records():
    """view_batch_size 1, 2 and None (9 views: chunks of 1; of 2 with a remainder of 1; of 9) each meet the end-to-end bounds; their
    mutual latents rms-rel is reported, not gated.  The per-view DAAM states are checked against the restated per-view recorders for each
    setting: with view_batch_size = 1 every chunk's image 0 is another view, so a dead record offset would pile every view into state 0."""
    from agenda_amd import synthetic
    pipe, cfg, u, v = _tiny("tiny")
    B, steps, win, lh, lw = 2, 2, pipe.window, 32, 32
    ctx = synthetic.make_context(cfg, B, seed=9)
    lat = _latents(cfg, [13, 14], lh, lw)
    want_img, want_lat, want_hm, want_views = _restated(cfg, u, v, ctx, lat, steps, win)
    assert _rel(want_views[4], want_views[0]) > 0.05            # the views' maps are different maps (else the check below shows nothing)
    lats = {}
    for vb in (1, 2, None):
        got_lat, got_img, got_hm, got_views = _run(pipe, ctx, lat, steps, vb)
        lats[vb] = got_lat
        e_lat, psnr, e_hm = _rms_rel(got_lat, want_lat), _psnr(got_img, want_img), _rel(got_hm, want_hm)
        e_views = max(_rel(got_views[k], want_views[k]) for k in range(got_views.shape[0]))
        print(f"view_batch_size={vb}: latents {e_lat:.4f}, PSNR {psnr:.1f} dB, canvas heat map {e_hm:.4f}, worst per-view map {e_views:.4f}")
        report(f"panorama_view_batch[tiny,32x32,vb={vb}]", latents_rms_rel=e_lat, psnr=psnr, heat_map_rel=e_hm, view_map_rel=e_views)
        assert e_lat < 0.06 and psnr > 30.0 and e_hm < 0.05, (vb, e_lat, psnr, e_hm)
        assert e_views < 0.05, (vb, e_views)
        assert _rel(got_views[4], got_views[0]) > 0.05, vb        # view k's accumulators differ from view 0's
    m1, m2 = _rms_rel(lats[1], lats[None]), _rms_rel(lats[2], lats[None])
    print(f"mutual latents rms-rel: view_batch_size 1 vs None {m1:.3e}, 2 vs None {m2:.3e}")
    report("panorama_view_batch_mutual[tiny,32x32]", vb1_vs_all=m1, vb2_vs_all=m2)
    pipe.engine.close()


def test_engine_refuses_foreign_state_and_bad_sizes():
    from agenda_amd import _lib, synthetic
    pipe, cfg, u, v = _tiny("tiny")
    eng = pipe.engine
    ctx = synthetic.make_context(cfg, 1, seed=1)
    eng.set_context(ctx)
    ts = pipe.scheduler.set_timesteps(2)
    a_t, a_p = pipe.scheduler.step_coeffs()
    with pytest.raises(_lib.AgendaHipError, match=r"latent size 16 x 36 with window 16 and stride 8"):
        eng.denoise_panorama(torch.zeros(1, 4, 16, 36).cuda(), 16, 8, None, ts, a_t, a_p, 7.5)
    with pytest.raises(_lib.AgendaHipError, match=r"latent size 8 x 40 with window 16"):
        eng.denoise_panorama(torch.zeros(1, 4, 8, 40).cuda(), 16, 8, None, ts, a_t, a_p, 7.5)
    z = torch.zeros(1, 4, 16, 40).cuda()
    eng.inpaint_set(torch.ones(1, 1, 16, 40), z, z)                  # a foreign state: the 4-channel inpainting blend
    with pytest.raises(_lib.AgendaHipError, match="an inpainting state is set"):
        eng.denoise_panorama(torch.zeros(1, 4, 16, 40).cuda(), 16, 8, None, ts, a_t, a_p, 7.5)
    eng.inpaint_clear()
    eng.record_config(1, False, 77)
    eng.record_reset(1, 16)                                          # a recorder sized for one image, not for 1 x 4 views
    with pytest.raises(_lib.AgendaHipError, match=r"the recorder holds 1 images at 16 x 16, this call records 1 panoramas x 4 views"):
        eng.denoise_panorama(torch.zeros(1, 4, 16, 40).cuda(), 16, 8, None, ts, a_t, a_p, 7.5)
    eng.record_config(0)
    x = _latents(cfg, [2], 16, 40).cuda()
    eng.denoise_panorama(x, 16, 8, None, ts, a_t, a_p, 7.5)          # and the plain call runs afterwards
    assert bool(torch.isfinite(x).all())
    pipe.engine.close()
