"""Region-based MultiDiffusion on the device: the mask front end, the spread and the masked mean as ops against fp64, the R = 1 identity with
the plain pipeline, the fused loop against its host-composed form, the pipeline end to end (latents, decoded image, every region's DAAM
maps, the composed word map) against the fp32 restatement in tests/_regions_restated.py, the pipeline's own bootstrap backgrounds against
the oracle's VAE encoder, and the engine's refusals."""
import math

import numpy as np
import pytest
import torch

import _regions_restated as R
from _aspect_restated import AspectDaamRecorder
from _report import report

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


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


def _tiny(name="tiny", cls=None, encoder=False):
    from agenda_amd import StableDiffusionRegionPipeline, config, synthetic
    cfg = config.CONFIGS[name]()
    seeds = (11, 12) if name == "tiny" else (31, 32)
    u = synthetic.make_unet_weights(cfg, seeds[0], bias_std=0.05, perturb_norm=0.1)
    v = synthetic.make_vae_weights(cfg, seeds[1], bias_std=0.05, perturb_norm=0.1, with_encoder=encoder)
    return (cls or StableDiffusionRegionPipeline)(cfg, u, v, workspace_bytes=2 << 30), cfg, u, v


def _split_context(ctx, Rn, B):
    """[2 R B, T, D] = [uncond x R B | cond x R B] (row r * B + p) -> the call's prompt_embeds [2B, T, D] and region_prompt_embeds [R - 1, 2B, T, D]"""
    RB = Rn * B
    pe = torch.cat([ctx[:B], ctx[RB:RB + B]], 0)
    rpe = torch.stack([torch.cat([ctx[r * B:(r + 1) * B], ctx[RB + r * B:RB + (r + 1) * B]], 0) for r in range(1, Rn)]) if Rn > 1 else None
    return pe, rpe


# ---- ops ------------------------------------------------------------------------------------------------------------------------
OP_SHAPES = [(1, 1, 4, 16, 16), (2, 2, 4, 16, 16), (3, 2, 4, 16, 24), (5, 1, 4, 24, 16), (3, 2, 4, 5, 7), (4, 2, 77, 16, 16)]
MASK_SETS = ["binary", "soft", "per_image"]


def _masks(kind, Rn, B, lh, lw, seed=0):
    """[R, B, lh, lw] fp32 latent masks, stated directly (not through the front end) so that a pixel can be left uncovered."""
    g = torch.Generator().manual_seed(1000 * Rn + 100 * B + lh * lw + seed)
    if kind == "soft":                                        # fractional, uniform in [0, 1], shared by the images
        return torch.rand(Rn, 1, lh, lw, generator=g).expand(Rn, B, lh, lw).contiguous()
    if kind == "per_image":                                   # every image its own binary masks
        m = (torch.rand(Rn, B, lh, lw, generator=g) > 0.5).float()
        if B > 1:
            assert not torch.equal(m[:, 0], m[:, 1])
        return m
    m = (torch.rand(Rn, 1, lh, lw, generator=g) > 0.5).float().expand(Rn, B, lh, lw).contiguous()
    m[:, :, :, 0] = 0                                         # a column no mask covers
    if Rn > 2:
        m[1:3, :, 1, 1] = 1                                   # two foreground regions overlap there
    elif Rn > 1:
        m[0:2, :, 1, 1] = 1
    return m


@pytest.mark.parametrize("Rn,B,C,lh,lw", OP_SHAPES[:-1])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("per_image", [False, True])
def test_region_masks_are_bit_exact(Rn, B, C, lh, lw, f32, per_image):
    from agenda_amd import ops
    if Rn == 1:
        got = ops.region_masks(None, B, lh, lw, regions=1).cpu()
        assert torch.equal(got, R.latent_masks(None, B, lh, lw)) and torch.equal(got, torch.ones(1, B, lh, lw))
        return
    g = torch.Generator().manual_seed(Rn * lh + lw + int(f32))
    shape = ((B,) if per_image else ()) + (Rn - 1, 8 * lh, 8 * lw)
    # coarse blobs (so that latent pixels are set in runs) plus pixel noise around both thresholds
    blobs = torch.rand(*shape[:-2], lh, lw, generator=g).repeat_interleave(8, -2).repeat_interleave(8, -1)
    px = (blobs + 0.2 * (torch.rand(shape, generator=g) - 0.5)).clamp(0, 1)
    px = px if f32 else (px * 255).round().to(torch.uint8)
    want = R.latent_masks(px, B, lh, lw)
    got = ops.region_masks(px.cuda(), B, lh, lw).cpu()
    assert got.shape == want.shape == (Rn, B, lh, lw)
    assert 0 < float(want[1:].mean()) < 1 and (Rn < 3 or float((want[1:].sum(0) > 1).sum()) > 0)      # set and unset pixels, and overlaps
    assert torch.equal(got, want)
    if not per_image:
        assert torch.equal(got[:, 0], got[:, -1])


@pytest.mark.parametrize("Rn,B,C,lh,lw", OP_SHAPES[:-1])
@pytest.mark.parametrize("kind", MASK_SETS)
def test_region_spread_matches_fp64(Rn, B, C, lh, lw, kind):
    """|got - want64| <= 8 * 2^-24 * (|x| m + (|sa bg| + |sb n|) (1 - m)) per element: the formula has at most five fp32 roundings, each
    relative to a partial result no larger than that sum, and 8 leaves room for any contraction.  Region 0, and every region of a step that
    is not bootstrapped, is the canvas bit for bit; so is every covered element under binary masks."""
    from agenda_amd import ops
    g = torch.Generator().manual_seed(Rn + 7 * B + lh * lw)
    N = 3
    x, n, bg = torch.randn(B, C, lh, lw, generator=g), torch.randn(B, C, lh, lw, generator=g), torch.randn(N, C, lh, lw, generator=g)
    m = _masks(kind, Rn, B, lh, lw)
    idx = torch.randint(0, N, (max(Rn - 1, 1),), generator=g).tolist()[:Rn - 1]
    sa, sb = float(np.float32(0.6)), float(np.float32(0.8))
    plain = ops.region_spread(x.cuda(), m.cuda()).cpu().reshape(Rn, B, C, lh, lw)
    assert all(torch.equal(plain[r], x) for r in range(Rn))                       # a step at or beyond `bootstrapping`
    got = ops.region_spread(x.cuda(), m.cuda(), n.cuda(), bg.cuda(), idx, sa, sb).cpu().reshape(Rn, B, C, lh, lw)
    assert torch.equal(got[0], x)                                                 # region 0 at any step
    want = R.spread(x.double(), m.double(), n.double(), bg.double(), idx, sa, sb).reshape(Rn, B, C, lh, lw)
    worst, tol_max = 0.0, 0.0
    for r in range(1, Rn):
        mm = m[r][:, None].double()
        tol = 8 * EPS * (x.double().abs() * mm + ((sa * bg[idx[r - 1]].double()).abs()[None] + (sb * n.double()).abs()) * (1 - mm))
        err = (got[r].double() - want[r]).abs()
        worst, tol_max = max(worst, float((err / tol.clamp_min(1e-300)).max())), max(tol_max, float(tol.max()))
        assert bool((err <= tol).all()), (r, float((err - tol).max()))
        if kind != "soft":
            cov = (m[r] == 1)[:, None].expand(-1, C, -1, -1)
            assert torch.equal(got[r][cov], x[cov])                               # covered elements are the canvas bit for bit
    if kind == "per_image" and B > 1 and Rn > 1:                                  # a r * B + p / p * R + r mix-up would swap these
        assert float((want[1:, 0] - want[1:, 1]).abs().max()) > tol_max
    report(f"region_spread[{Rn},{B},{C},{lh}x{lw},{kind}]", worst_err_over_tol=worst)


@pytest.mark.parametrize("Rn,B,C,lh,lw", OP_SHAPES)
@pytest.mark.parametrize("kind", MASK_SETS)
def test_region_mean_matches_fp64(Rn, B, C, lh, lw, kind):
    """|got - want64| <= (R + 2) * 2^-24 * sum_r m_r |x_r| / sum_r m_r: R products and R - 1 sums of the numerator, the denominator's sums
    and one division, each within half an ulp of a partial result no larger than sum m |x|.  An uncovered pixel is exactly 0; the kernel
    adds in the restatement's order, so bit-identity with it is expected and reported, not gated."""
    from agenda_amd import ops
    g = torch.Generator().manual_seed(3 * Rn + B + C + lh * lw)
    x = torch.randn(Rn * B, C, lh, lw, generator=g)
    m = _masks(kind, Rn, B, lh, lw, seed=1)
    got = ops.region_mean(x.cuda(), m.cuda()).cpu()
    again = ops.region_mean(x.cuda(), m.cuda()).cpu()
    assert torch.equal(got, again)                                                # two runs give equal bits
    want = R.masked_mean(x.double(), m.double())
    den = m.double().sum(0)[:, None].expand(-1, C, -1, -1)
    num_abs = (m.double()[:, :, None] * x.double().reshape(Rn, B, C, lh, lw).abs()).sum(0)
    tol = torch.where(den > 0, (Rn + 2) * EPS * num_abs / den.clamp_min(1e-300), torch.zeros_like(den))
    err = (got.double() - want).abs()
    assert bool((err <= tol).all()), float((err - tol).max())
    if kind == "binary":
        assert float(den[:, :, :, 0].max()) == 0.0 and bool((got[:, :, :, 0] == 0).all())     # the uncovered column is exactly 0
    assert bool((got[den == 0] == 0).all())
    if kind == "per_image" and B > 1:
        assert float((want[0] - want[1]).abs().max()) > float(tol.max())
    w32 = R.masked_mean(x, m)
    exact = bool(torch.equal(got, w32))
    worst = float((err / tol.clamp_min(1e-300))[den > 0].max())
    print(f"region_mean R={Rn} B={B} C={C} {lh}x{lw} {kind}: bit-identical to the fp32 restatement={exact}, worst err / tol {worst:.3f}")
    report(f"region_mean[{Rn},{B},{C},{lh}x{lw},{kind}]", bit_identical=int(exact), worst_err_over_tol=worst)


def test_region_ops_refuse_bad_arguments():
    from agenda_amd import _lib, ops
    x, m = torch.zeros(1, 4, 8, 8).cuda(), torch.ones(2, 1, 8, 8).cuda()
    with pytest.raises(_lib.AgendaHipError, match=r"background index 3 of region 1 outside 0 \.\. 2"):
        ops.region_spread(x, m, x, torch.zeros(3, 4, 8, 8).cuda(), [3], 0.5, 0.5)
    with pytest.raises(_lib.AgendaHipError, match="no whole multiple of the latent size"):
        ops.region_masks(torch.zeros(1, 60, 64, dtype=torch.uint8).cuda(), 1, 8, 8)
    with pytest.raises(_lib.AgendaHipError, match=r"9 regions \(1 \.\. 8\)"):
        ops.region_mean(torch.zeros(9, 4, 8, 8).cuda(), torch.ones(9, 1, 8, 8).cuda())


# ---- R = 1 is the plain pipeline ------------------------------------------------------------------------------------------------
def test_no_regions_is_bit_identical_to_the_plain_pipeline():
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    reg, cfg, u, v = _tiny("tiny")
    plain = StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=5)
    lat = synthetic.make_latents(cfg, [3, 4], L)
    outs = []
    for pipe, kw in ((plain, {}), (reg, {"region_prompts": []})):
        with trace(pipe) as trc:
            out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=3, height=8 * L, width=8 * L, output_type="pt", **kw)
            hms = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
        outs.append((out.latents.cpu(), out.images.cpu(), hms))
    assert outs[1][2].shape == (B, cfg.max_tokens, L, L)
    for a, b, what in zip(outs[0], outs[1], ("latents", "images", "heat maps")):
        assert torch.equal(a, b), what
    plain.engine.close(); reg.engine.close()


# ---- the fused loop against the existing entry points ---------------------------------------------------------------------------------
def _pixel_boxes(B, lh, lw):
    """per-image pixel masks [B, 2, 8 lh, 8 lw]: two overlapping boxes, different for every image"""
    lay = [[[0.0, 0.0, 0.5, 1.0], [0.25, 0.0, 1.0, 0.5]], [[0.5, 0.0, 1.0, 1.0], [0.0, 0.5, 0.75, 1.0]]]
    return torch.stack([R.boxes_to_masks(lay[p % 2], 8 * lh, 8 * lw) for p in range(B)])


def _host_loop(pipe, ctx, lat, masks, bgs, idx, steps, boot, g):
    """torch spread -> engine.denoise for one step on the R B rows under the 2 R B context -> torch masked mean, per step."""
    eng = pipe.engine
    ts = pipe.scheduler.set_timesteps(steps)
    a_t, a_p = pipe.scheduler.step_coeffs()
    eng.set_context(ctx)
    x = lat.clone().cuda()
    noise, masks, bgs = x.clone(), masks.cuda(), bgs.cuda()
    for s in range(steps):
        if s < boot:
            xr = R.spread(x, masks, noise, bgs, idx[s], float(a_t[s]) ** 0.5, (1.0 - float(a_t[s])) ** 0.5).contiguous()
        else:
            xr = R.spread(x, masks).contiguous()
        eng.denoise(xr, ts[s:s + 1], a_t[s:s + 1], a_p[s:s + 1], g)
        x = R.masked_mean(xr, masks)
    return x.cpu()


def _fused_vs_host(pipe, cfg, Rn, B, lh, lw, steps, boot, g, seed):
    from agenda_amd import synthetic
    ctx = synthetic.make_context(cfg, Rn * B, seed=seed)
    pe, rpe = _split_context(ctx, Rn, B)
    lat = _latents(cfg, [7 + p for p in range(B)], lh, lw)
    px = _pixel_boxes(B, lh, lw)
    bgs = torch.randn(3, cfg.unet.out_channels, lh, lw, generator=torch.Generator().manual_seed(seed + 1))
    out = pipe(prompt_embeds=pe, region_prompt_embeds=rpe, region_masks=px, bootstrapping=boot, bootstrap_backgrounds=bgs, latents=lat,
               num_inference_steps=steps, guidance_scale=g, height=8 * lh, width=8 * lw, output_type="latent",
               generator=torch.Generator().manual_seed(seed))
    got = out.latents.cpu()
    idx = pipe.last_region_state["idx"].tolist()
    assert len(idx) == boot and all(len(r) == Rn - 1 and all(0 <= k < 3 for k in r) for r in idx)
    want = _host_loop(pipe, ctx, lat, R.latent_masks(px, B, lh, lw), bgs, idx, steps, boot, g)
    return got, want


@pytest.mark.parametrize("lh,lw", [(16, 16), (16, 24)])
def test_fused_loop_matches_host_composed_loop_tiny(lh, lw):
    pipe, cfg, u, v = _tiny("tiny")
    got, want = _fused_vs_host(pipe, cfg, 3, 2, lh, lw, steps=3, boot=2, g=7.5, seed=21)
    e = _rms_rel(got, want)
    print(f"regions fused vs host loop {lh}x{lw}: latents rms-rel {e:.3e}")
    report(f"regions_fused_vs_host[tiny,{lh}x{lw}]", latents_rms_rel=e)
    assert e < 1e-4, e
    pipe.engine.close()


# ---- end to end against the restatement -----------------------------------------------------------------------------------------
WORD_IDX = 2


def _run(pipe, pe, rpe, px, bgs, lat, steps, boot, seed):
    from agenda_amd import trace
    B, _, lh, lw = lat.shape
    Rn = 1 + (0 if rpe is None else rpe.shape[0])
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=pe, region_prompt_embeds=rpe, region_masks=px, bootstrapping=boot, bootstrap_backgrounds=bgs, latents=lat,
                   num_inference_steps=steps, height=8 * lh, width=8 * lw, output_type="np", generator=torch.Generator().manual_seed(seed))
        hm = torch.stack([torch.stack([trc.compute_global_heat_map(image_index=p, region=r).heat_maps for p in range(B)]) for r in range(Rn)]).cpu()
        wm = torch.stack([trc.compute_region_word_heat_map("", image_index=p, word_idx=WORD_IDX).heatmap for p in range(B)]).cpu()
    return out.latents.cpu(), out.images, hm, wm, pipe.last_region_state["idx"].tolist()


@pytest.mark.parametrize("name,lh,lw", [("tiny", 16, 16), ("tiny", 24, 16), ("tiny21", 24, 24)])
def test_regions_match_restatement(name, lh, lw):
    """B = 2 distinct contexts, R = 3, per-image masks, DDIM x 2 with bootstrapping = 1, decode and DAAM on; the bounds of the same configs
    in test_panorama_gpu.py / test_model_gpu.py: latents rms-rel < 0.06, PSNR > 30 dB, every region's global heat map and the composed word
    map max-rel < 0.05.  Each image of the batch also matches its own batch-1 run to the same bounds."""
    from agenda_amd import synthetic
    pipe, cfg, u, v = _tiny(name)
    Rn, B, steps, boot, seed = 3, 2, 2, 1, 5
    ctx = synthetic.make_context(cfg, Rn * B, seed=seed)
    pe, rpe = _split_context(ctx, Rn, B)
    lat = _latents(cfg, [3, 4], lh, lw)
    px = _pixel_boxes(B, lh, lw)
    bgs = torch.randn(2, cfg.unet.out_channels, lh, lw, generator=torch.Generator().manual_seed(77))
    got_lat, got_img, got_hm, got_wm, idx = _run(pipe, pe, rpe, px, bgs, lat, steps, boot, seed)
    masks = R.latent_masks(px, B, lh, lw)
    recs = [AspectDaamRecorder((lh, lw), cfg.max_tokens) for _ in range(Rn)]
    want_img, want_lat = R.generate_regions(u, v, cfg, ctx, lat, masks, bgs, idx, steps, 7.5, boot, recorders=recs)
    want_hm = torch.stack([r.compute_global_heat_map() for r in recs])                                   # [R, B, T, lh, lw]
    want_wm = R.region_word_map([want_hm[r][:, WORD_IDX + 1] for r in range(Rn)], masks)
    assert got_img.shape == want_img.shape == (B, 8 * lh, 8 * lw, 3) and got_hm.shape == want_hm.shape == (Rn, B, cfg.max_tokens, lh, lw)
    assert _rel(want_hm[1], want_hm[2]) > 0.05                 # the regions' maps are different maps (else the check below shows nothing)
    e_lat, psnr = _rms_rel(got_lat, want_lat), _psnr(got_img, want_img)
    e_hm, e_wm = max(_rel(got_hm[r], want_hm[r]) for r in range(Rn)), _rel(got_wm, want_wm)
    print(f"{name} {lh}x{lw}: latents {e_lat:.4f}, PSNR {psnr:.1f} dB, worst region heat map {e_hm:.4f}, composed word map {e_wm:.4f}")
    report(f"regions_txt2img[{name},{lh}x{lw}]", latents_rms_rel=e_lat, psnr=psnr, heat_map_rel=e_hm, word_map_rel=e_wm)
    assert e_lat < 0.06 and psnr > 30.0 and e_hm < 0.05 and e_wm < 0.05, (e_lat, psnr, e_hm, e_wm)
    assert _rel(got_hm[1], got_hm[2]) > 0.05                   # region 2's accumulators differ from region 1's: the record offset is alive
    for p in range(B):
        pe1, rpe1 = torch.stack([pe[p], pe[B + p]]), torch.stack([rpe[:, p], rpe[:, B + p]], 1)
        one_lat, one_img, one_hm, one_wm, idx1 = _run(pipe, pe1, rpe1, px[p:p + 1], bgs, lat[p:p + 1], steps, boot, seed)
        assert idx1 == idx
        e1, p1 = _rms_rel(got_lat[p:p + 1], one_lat), _psnr(got_img[p:p + 1], one_img)
        h1, w1 = max(_rel(got_hm[r][p:p + 1], one_hm[r]) for r in range(Rn)), _rel(got_wm[p:p + 1], one_wm)
        print(f"{name} {lh}x{lw}: image {p} of the batch against its batch-1 run: latents {e1:.2e}, PSNR {p1:.1f} dB, heat map {h1:.2e}, word map {w1:.2e}")
        report(f"regions_batch1[{name},{lh}x{lw},{p}]", latents_rms_rel=e1, psnr=p1, heat_map_rel=h1, word_map_rel=w1)
        assert e1 < 0.06 and p1 > 30.0 and h1 < 0.05 and w1 < 0.05, (p, e1, p1, h1, w1)
    pipe.engine.close()


# ---- the pipeline's own backgrounds ---------------------------------------------------------------------------------------------
def test_pipeline_builds_its_backgrounds_like_the_oracle_encoder():
    """bootstrap_backgrounds left None: the N = bootstrapping colours, the sampling noise and the choices come from the call's generator,
    after the initial latents; the encoded backgrounds match the oracle's `vae_encode_moments` of the same colours and noise to the encode
    bound of tests/test_aspect_gpu.py's img2img test (rms-rel < 2^-6), and two calls with the same seed give equal bits."""
    from agenda_amd import synthetic
    from oracle import sd_oracle as O
    pipe, cfg, u, v = _tiny("tiny", encoder=True)
    B, L, N, steps = 1, 16, 2, 2
    ctx = synthetic.make_context(cfg, 2 * B, seed=9)
    pe, rpe = _split_context(ctx, 2, B)
    kw = dict(prompt_embeds=pe, region_prompt_embeds=rpe, region_boxes=[[0.25, 0.25, 0.75, 0.75]], bootstrapping=N, num_inference_steps=steps,
              height=8 * L, width=8 * L, output_type="latent")
    a = pipe(generator=torch.Generator().manual_seed(123), **kw).latents.cpu()
    st = {k: (t.cpu().clone() if t is not None else None) for k, t in pipe.last_region_state.items()}
    g = torch.Generator().manual_seed(123)
    lat0 = torch.randn(B, cfg.unet.out_channels, L, L, generator=g)                      # the plain pipeline's draw comes first
    colors, e = torch.rand(N, 3, generator=g), torch.randn(N, cfg.vae.latent_channels, L, L, generator=g)
    idx = torch.randint(0, N, (N, 1), generator=g)
    assert torch.equal(st["colors"], colors) and torch.equal(st["noise"], e) and torch.equal(st["idx"], idx)
    img = (2 * colors - 1)[:, :, None, None].expand(-1, -1, 8 * L, 8 * L).contiguous()
    assert float(img.min()) >= -1 and float(img.max()) <= 1
    wm, wl = O.vae_encode_moments(v, cfg.vae, img)
    want = (wm + torch.exp(0.5 * wl) * e) * cfg.vae.scaling_factor
    assert st["backgrounds"].shape == want.shape == (N, cfg.vae.latent_channels, L, L)
    err = _rms_rel(st["backgrounds"], want)
    report("regions_backgrounds[tiny,16x16]", backgrounds_rms_rel=err)
    assert err < 2.0 ** -6, err
    b = pipe(generator=torch.Generator().manual_seed(123), **kw).latents.cpu()
    assert torch.equal(a, b) and torch.equal(pipe.last_region_state["backgrounds"].cpu(), st["backgrounds"])
    c = pipe(generator=torch.Generator().manual_seed(123), latents=lat0, bootstrap_backgrounds=st["backgrounds"], **kw).latents.cpu()
    assert pipe.last_region_state["colors"] is None
    pipe.engine.close()


# ---- engine refusals ------------------------------------------------------------------------------------------------------------
def test_engine_refuses_foreign_state_and_bad_descriptors():
    from agenda_amd import _lib, synthetic
    pipe, cfg, u, v = _tiny("tiny")
    eng = pipe.engine
    Rn, B, L, N = 2, 1, 16, 2
    eng.set_context(synthetic.make_context(cfg, Rn * B, seed=1))
    ts = pipe.scheduler.set_timesteps(2)
    a_t, a_p = pipe.scheduler.step_coeffs()
    masks = R.latent_masks(R.boxes_to_masks([[0.0, 0.0, 0.5, 1.0]], 8 * L, 8 * L), B, L, L).cuda()
    bgs = torch.zeros(N, 4, L, L).cuda()
    sq = [(float(a) ** 0.5, (1 - float(a)) ** 0.5) for a in a_t]

    def run(x, idx=((0,),), boot=1):
        return eng.denoise_regions(x, masks, x.clone(), bgs, [list(r) for r in idx], sq[:boot], boot, ts, a_t, a_p, 7.5)

    z = torch.zeros(B, 4, L, L).cuda()
    eng.inpaint_set(torch.ones(B, 1, L, L), z, z)                    # a foreign state: the 4-channel inpainting blend
    with pytest.raises(_lib.AgendaHipError, match="denoise_regions: an inpainting state is set"):
        run(z.clone())
    eng.inpaint_clear()
    eng.record_config(1, False, 77)
    eng.record_reset(B, L)                                           # a recorder sized for B images, not for R B
    with pytest.raises(_lib.AgendaHipError, match=r"the recorder holds 1 images at 16 x 16, this call records 2 regions x 1 images"):
        run(z.clone())
    eng.record_config(0)
    eng.set_context(synthetic.make_context(cfg, B, seed=1))          # a context of 2 B rows
    with pytest.raises(_lib.AgendaHipError, match=r"context batch 2 != 2 \* regions \* batch = 2 \* 2 \* 1"):
        run(z.clone())
    eng.set_context(synthetic.make_context(cfg, Rn * B, seed=1))
    with pytest.raises(_lib.AgendaHipError, match=r"background index 2 \(step 0, region 1\) outside 0 \.\. 1"):
        run(z.clone(), idx=((N,),))
    with pytest.raises(_lib.AgendaHipError, match=r"bootstrapping 3 outside 0 \.\. 2"):
        eng.denoise_regions(z.clone(), masks, z.clone(), bgs, [[0], [0], [0]], sq + [(0.5, 0.5)], 3, ts, a_t, a_p, 7.5)
    x = _latents(cfg, [2], L, L).cuda()
    run(x)                                                           # and the plain region call runs afterwards
    assert bool(torch.isfinite(x).all())
    pipe.engine.close()


# ---- SD-1.5 shapes ----------------------------------------------------------------------------------------------------------------
def test_sd15_smoke_and_fused_loop_matches_host_composed_loop():
    """SD-1.5 synthetic, 512 x 512, R = 2, B = 1, 2 steps under trace: finite output, maps (77, 64, 64) non-negative and not all zero, and
    the latents against the host-composed loop to the tiny test's bound."""
    from agenda_amd import StableDiffusionRegionPipeline, synthetic, trace
    pipe = StableDiffusionRegionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg = pipe.cfg
    Rn, B, L, steps, boot, g, seed = 2, 1, 64, 2, 1, 7.5, 3
    ctx = synthetic.make_context(cfg, Rn * B, seed=seed)
    pe, rpe = _split_context(ctx, Rn, B)
    lat = _latents(cfg, [5], L, L)
    px = R.boxes_to_masks([[0.25, 0.25, 0.75, 0.75]], 8 * L, 8 * L)
    bgs = torch.randn(2, 4, L, L, generator=torch.Generator().manual_seed(8))
    with trace(pipe) as trc:
        got = pipe(prompt_embeds=pe, region_prompt_embeds=rpe, region_masks=px, bootstrapping=boot, bootstrap_backgrounds=bgs, latents=lat,
                   num_inference_steps=steps, guidance_scale=g, output_type="latent", generator=torch.Generator().manual_seed(seed)).latents
        hms = [trc.compute_global_heat_map(image_index=0, region=r).heat_maps for r in range(Rn)]
        wm = trc.compute_region_word_heat_map("", image_index=0, word_idx=1).heatmap
    assert bool(torch.isfinite(got).all()) and tuple(wm.shape) == (64, 64)
    for hm in hms:
        assert tuple(hm.shape) == (77, 64, 64) and bool(torch.isfinite(hm).all()) and float(hm.min()) >= 0.0 and float(hm.max()) > 0.0
    idx = pipe.last_region_state["idx"].tolist()
    want = _host_loop(pipe, ctx, lat, R.latent_masks(px, B, L, L), bgs, idx, steps, boot, g)
    e = _rms_rel(got, want)
    print(f"regions fused vs host loop sd15 512x512: latents rms-rel {e:.3e}")
    report("regions_fused_vs_host[sd15,64x64]", latents_rms_rel=e)
    assert e < 1e-4, e
    pipe.engine.close()
