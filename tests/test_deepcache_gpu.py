"""DeepCache on the device: the capture kernel through its op seam, the full / shallow pair of one evaluation (exact, and against the fp32
restatement tests/_deepcache_restated.py), whole loops against the restatement with the plain call's own error as the yardstick, the fused
loop against a host-stepped one, the off switches and counters, the recorders, batch rows, DeepCache beside a LoRA and FreeU, every refusal
and the CLI.  No test here provokes a fault: every refusal tested is a host-side status returned before any launch."""
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _deepcache_restated as R
from _report import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 7.5                               # guidance_scale
# The combine is the plain CFG one, so a DeepCache evaluation amplifies its inputs' errors exactly as a plain one does; the factor 2 (6 dB on
# PSNR) covers the different trajectory and the cached tensor's own bf16 error entering a second evaluation.
LOOP_FACTOR, LOOP_DB = 2.0, 6.0
FWD_FACTOR = 2.0                      # one forward made of the same arithmetic


def _rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def _rms_rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


_W = {}


def _weights(name):
    """(cfg, unet, vae) of a config, drawn once per session: the tiny configs as tests/test_deepcache_cpu.py draws them."""
    if name not in _W:
        from agenda_amd import config, synthetic
        cfg = config.CONFIGS[name]()
        small = name != "sd15"
        kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
        _W[name] = (cfg, synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw), synthetic.make_vae_weights(cfg, 12 if small else 1235, **kw))
    return _W[name]


def _pipe(name="tiny", scheduler="DDIMScheduler", **kw):
    from agenda_amd import StableDiffusionPipeline
    cfg, u, v = _weights(name)
    return StableDiffusionPipeline(cfg, u, v, workspace_bytes=(6 if name == "sd15" else 2) << 30, scheduler=scheduler, **kw)


def _ddim(pipe, steps):
    ts = pipe.scheduler.set_timesteps(steps)
    a_t, a_p = pipe.scheduler.step_coeffs()
    return ts, a_t, a_p


def _n_attn2(u):
    return sum(u.down_cross) * (2 * u.layers_per_block + 1) + 1


# ---- 1. the capture kernel alone ------------------------------------------------------------------------------------------------
# (activation shape, partial-sum floats): a few bytes (tails only, one workgroup); tails of 2 and 4 bytes behind whole words; 576 ragged
# tokens x 320 channels x 2 rows = 46080 words, 180 workgroups, with the 64-row-tile table [2 * 576 / 64][320][2]; more words than the
# 8192 x 256 grid covers in one trip (2.6 M words: grid-stride); and no table at all (cpart_bm == 0)
CAPTURE_CASES = [((5,), 3), ((3, 7, 5), 33), ((2, 576, 320), 2 * 9 * 320 * 2), ((16, 4096, 320), 16 * 64 * 320 * 2), ((2, 100, 64), 0)]


@pytest.mark.parametrize("shape,n_part", CAPTURE_CASES, ids=[f"{'x'.join(map(str, c[0]))}+{c[1]}" for c in CAPTURE_CASES])
def test_capture_copies_both_regions_bit_for_bit(shape, n_part):
    from agenda_amd import ops
    g = torch.Generator().manual_seed(sum(shape) + n_part)
    act = torch.randn(*shape, generator=g).to(torch.bfloat16)
    part = torch.randn(n_part, generator=g) if n_part else None
    (a, a_guard), p = ops.deepcache_capture(act.cuda(), part.cuda() if n_part else None)
    assert a.dtype == torch.bfloat16 and torch.equal(a.cpu().view(torch.int16), act.view(torch.int16))
    assert bool((a_guard.cpu() == 0xA5).all())                     # nothing written behind the region's last byte
    if n_part:
        assert torch.equal(p[0].cpu().view(torch.int32), part.view(torch.int32)) and bool((p[1].cpu() == 0xA5).all())
    else:
        assert p is None


def test_capture_refuses_unaligned_regions_and_nothing_to_copy():
    from agenda_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.uint8).cuda()
    dst = torch.zeros(256, dtype=torch.uint8).cuda()
    with pytest.raises(_lib.AgendaHipError, match="16-byte boundary"):
        _lib.check(lib.agd_op_deepcache_capture(None, buf.data_ptr() + 2, dst.data_ptr(), 32, None, None, 0, _lib.current_stream_ptr()), None, "capture")
    with pytest.raises(_lib.AgendaHipError, match="deepcache_capture: 0 \\+ 0 bytes"):
        _lib.check(lib.agd_op_deepcache_capture(None, None, None, 0, None, None, 0, _lib.current_stream_ptr()), None, "capture")
    assert bool((dst.cpu() == 0).all())


# ---- 2. one full / shallow pair -------------------------------------------------------------------------------------------------
# tiny: lpb = 2, both branches (at b = 1 the cache comes from the upsampler), two and three rows (three: odd, the unshared prefix); tiny40:
# C = 320 / 640 plans, lpb = 1; tiny21 at 24 x 24: linear projections, 576 ragged tokens (no 64-row partial sums: the cpart_bm == 0 cache),
# v-prediction; sd15: the real channel counts, two rows at 16 x 16
FWD_CASES = [("tiny", 16, 0, 2), ("tiny", 16, 1, 2), ("tiny", 16, 0, 3), ("tiny", 16, 1, 3), ("tiny40", 16, 0, 2), ("tiny21", 24, 0, 2), ("sd15", 16, 0, 2)]


@pytest.mark.parametrize("name,L,branch,rows", FWD_CASES, ids=[f"{c[0]}-b{c[2]}-r{c[3]}" for c in FWD_CASES])
def test_full_is_the_plain_forward_and_shallow_matches_restatement(name, L, branch, rows):
    """Exact: deepcache_forward(shallow=0) is unet_forward bit for bit, and shallow=1 straight after it on the same input and t repeats it bit
    for bit (the same launches on the same inputs).  Then the shallow forward at another (x', t') after the capture at (x, t) against the
    restatement; the bound is the plain forward's own rms-rel error against the plain oracle forward, measured here, times 2."""
    from agenda_amd import synthetic
    from oracle import sd_oracle as O
    cfg, u, v = _weights(name)
    ctx = synthetic.make_context(cfg, 2, seed=6)[:rows]
    x = torch.randn(rows, 4, L, L, generator=torch.Generator().manual_seed(3))
    x2 = x + 0.3 * torch.randn(rows, 4, L, L, generator=torch.Generator().manual_seed(4))
    t, t2 = 301.0, 281.0
    pipe = _pipe(name)
    e = pipe.engine
    e.set_context(ctx)
    plain = e.unet_forward(x, t).cpu()
    c0 = e.deepcache_counts()
    full = e.deepcache_forward(x, t, branch, shallow=False).cpu()
    same = e.deepcache_forward(x, t, branch, shallow=True).cpu()
    moved = e.deepcache_forward(x2, t2, branch, shallow=True).cpu()
    again = e.deepcache_forward(x, t, branch, shallow=True).cpu()      # the cache is read, never written, by a shallow evaluation
    c1 = e.deepcache_counts()
    plain_after = e.unet_forward(x, t).cpu()
    e.close()
    assert c0 == (0, 0) and c1 == (1, 3)
    assert torch.equal(full, plain) and torch.equal(plain_after, plain)
    assert torch.equal(same, plain), _rms_rel(same, plain)
    assert torch.equal(again, plain)
    with torch.no_grad():
        def one(i, xx, tt, mode, cache):
            return R.unet_forward(u, cfg.unet, xx[i:i + 1], torch.tensor(tt), ctx[i:i + 1], mode, branch, cache)
        caches = [{} for _ in range(rows)]
        want_full = torch.cat([one(i, x, t, "full", caches[i]) for i in range(rows)])            # one image at a time
        want = torch.cat([one(i, x2, t2, "shallow", caches[i]) for i in range(rows)])
        full2 = torch.cat([O.unet_forward(u, cfg.unet, x2[i:i + 1], torch.tensor(t2), ctx[i:i + 1]) for i in range(rows)])
    err_plain, err, stale = _rms_rel(plain, want_full), _rms_rel(moved, want), _rms_rel(want, full2)
    print(f"deepcache forward {name} b{branch} r{rows}: rms rel {err:.5f} (plain {err_plain:.5f}; the full forward at (x', t') is {stale:.3f} away)")
    report(f"deepcache_forward[{name},b{branch},rows{rows}]", rms_rel=err, plain_rms_rel=err_plain, shallow_vs_full_rms_rel=stale)
    assert not torch.equal(moved, plain)
    assert err <= FWD_FACTOR * err_plain, (err, err_plain)


# ---- 3. loops -------------------------------------------------------------------------------------------------------------------
# (config, scheduler, restatement key, steps, Lh, Lw, interval, branch)
LOOP_CASES = [("tiny", "DDIMScheduler", "ddim", 6, 16, 16, 2, 0), ("tiny", "PNDMScheduler", "pndm", 5, 16, 16, 3, 1),
              ("tiny", "DPMSolverMultistepScheduler", "dpm", 6, 16, 16, 3, 0), ("tiny", "DDIMScheduler", "ddim", 5, 16, 24, 2, 1),
              ("tiny", "DPMSolverMultistepScheduler", "dpm", 4, 16, 16, 2, 1), ("tiny", "PNDMScheduler", "pndm", 4, 16, 16, 2, 0),
              ("tiny40", "DDIMScheduler", "ddim", 4, 16, 16, 2, 0), ("tiny21", "DDIMScheduler", "ddim", 4, 24, 24, 3, 0)]


def _call(pipe, ctx, lat, steps, **kw):
    from agenda_amd import trace
    B, Lh, Lw = lat.shape[0], lat.shape[2], lat.shape[3]
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, height=8 * Lh, width=8 * Lw, guidance_scale=S, output_type="np", **kw)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    return out.latents.cpu(), out.images, hm


def _restated(u, v, cfg, ctx, lat, steps, key, interval, branch, freeu=None, ddim_start=0):
    from _aspect_restated import AspectDaamRecorder
    rec = AspectDaamRecorder((lat.shape[2], lat.shape[3]), context_size=cfg.max_tokens)
    img, x, counts = R.generate(u, v, cfg, ctx, lat, steps, key, S, interval, branch, rec, freeu, ddim_start)
    return x, img, rec.compute_global_heat_map(), counts


def _figures(got, want):
    (lat, img, hm), (wlat, wimg, whm) = got, want[:3]
    assert hm.shape == whm.shape and img.shape == wimg.shape
    return _rms_rel(lat, wlat), _psnr(img, wimg), max(_rel(hm[i], whm[i]) for i in range(hm.shape[0]))


def _assert_relative(tag, plain, dc, drift):
    (pl, pp, ph), (gl, gp, gh) = plain, dc
    print(f"deepcache {tag}: latents rms rel {gl:.4f} (plain {pl:.4f}), PSNR {gp:.1f} dB (plain {pp:.1f}), heat map max rel {gh:.4f} "
          f"(plain {ph:.4f}); the plain result is {drift:.4f} away")
    report(f"deepcache_loop[{tag}]", latents_rms_rel=gl, psnr_db=gp, heat_map_rel=gh, plain_latents_rms_rel=pl, plain_psnr_db=pp,
           plain_heat_map_rel=ph, drift_from_plain_rms_rel=drift)
    assert gl <= LOOP_FACTOR * pl, ("latents", gl, pl)
    assert gh <= LOOP_FACTOR * ph, ("heat map", gh, ph)
    assert gp >= pp - LOOP_DB, ("psnr", gp, pp)


@pytest.mark.parametrize("name,scheduler,key,steps,Lh,Lw,interval,branch", LOOP_CASES,
                         ids=[f"{c[0]}-{c[2]}-{c[4]}x{c[5]}-k{c[6]}-b{c[7]}" for c in LOOP_CASES])
def test_loop_matches_restatement(name, scheduler, key, steps, Lh, Lw, interval, branch):
    """B = 2, guidance_scale 7.5, DAAM on: latents, decoded image and each image's heat map (the restatement's recorder is fed the same
    calls) against the restatement, and in the same test the plain call against the plain oracle loop; DeepCache's errors may be 2 x the
    plain ones (6 dB).  The counters are (full evaluations followed by a shallow one, shallow evaluations)."""
    from agenda_amd import synthetic
    cfg, u, v = _weights(name)
    B = 2
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = torch.randn(B, 4, Lh, Lw, generator=torch.Generator().manual_seed(8))
    pipe = _pipe(name, scheduler)
    plain = _call(pipe, ctx, lat, steps)
    c0 = pipe.engine.deepcache_counts()
    pipe.enable_deepcache(cache_interval=interval, cache_branch_id=branch)
    got = _call(pipe, ctx, lat, steps)
    c1 = pipe.engine.deepcache_counts()
    pipe.engine.close()
    want_plain = _restated(u, v, cfg, ctx, lat, steps, key, 1, 0)
    want = _restated(u, v, cfg, ctx, lat, steps, key, interval, branch)
    n_evals = steps + (key == "pndm")
    flags = R.schedule(n_evals, interval)
    assert want_plain[3] == (0, 0) and want[3] == (sum(1 for i in range(n_evals - 1) if flags[i] and not flags[i + 1]), flags.count(False))
    assert c0 == (0, 0) and c1 == want[3]
    assert not torch.equal(want_plain[0], want[0]) and not torch.equal(got[0], plain[0])      # (the cache did something)
    _assert_relative(f"{name},{key},{Lh}x{Lw},k{interval},b{branch}", _figures(plain, want_plain), _figures(got, want), _rms_rel(got[0], plain[0]))


def test_img2img_matches_restatement():
    """img2img runs the tail of the DDIM grid; the flags count its own evaluations from 0.  Strength 0.5 of 8 steps, interval 2: F S F S."""
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    from _aspect_restated import AspectDaamRecorder
    cfg, u, _ = _weights("tiny")
    v = synthetic.make_vae_weights(cfg, 12, with_encoder=True, bias_std=0.05, perturb_norm=0.1)
    pipe = StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30)
    B, L, steps, branch = 2, 16, 8, 1
    ctx = synthetic.make_context(cfg, B, seed=3)
    img = torch.rand(B, 3, 8 * L, 8 * L, generator=torch.Generator().manual_seed(4)) * 2 - 1
    nz = torch.randn(2, B, 4, L, L, generator=torch.Generator().manual_seed(5))

    def run():
        with trace(pipe) as trc:
            out = pipe.img2img(image=img, strength=0.5, num_inference_steps=steps, prompt_embeds=ctx, noise_enc=nz[0], noise=nz[1],
                               guidance_scale=S, output_type="np")
            hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
        return out.latents.cpu(), out.images, hm
    plain = run()
    pipe.enable_deepcache(cache_interval=2, cache_branch_id=branch)
    got = run()
    counts = pipe.engine.deepcache_counts()
    pipe.enable_deepcache(cache_interval=1)
    off = run()
    # the start of the loop, as the pipeline makes it (the encoder's own error is not under test here)
    mean, logvar = pipe.engine.vae_encode(img)
    x0 = (mean + torch.exp(0.5 * logvar) * nz[0].to(mean.device)) * cfg.vae.scaling_factor
    ts = pipe.scheduler.set_timesteps(steps)
    a = float(pipe.scheduler.alphas_cumprod[int(ts[4])])
    start = (a ** 0.5 * x0 + (1 - a) ** 0.5 * nz[1].to(mean.device)).cpu()
    pipe.engine.close()
    assert counts == (2, 2)
    assert torch.equal(off[0], plain[0]) and np.array_equal(off[1], plain[1]) and torch.equal(off[2], plain[2])
    assert not torch.equal(got[0], plain[0])
    v_dec = {k: w for k, w in v.items()}
    wants = []
    for interval in (1, 2):
        rec = AspectDaamRecorder((L, L), context_size=cfg.max_tokens)
        im, x, c = R.generate(u, v_dec, cfg, ctx, start, steps, "ddim", S, interval, branch, rec, None, 4)
        wants.append((x, im, rec.compute_global_heat_map(), c))
    assert wants[0][3] == (0, 0) and wants[1][3] == (2, 2)
    _assert_relative("tiny,img2img,16x16,k2,b1", _figures(plain, wants[0]), _figures(got, wants[1]), _rms_rel(got[0], plain[0]))


# ---- 4. the fused loop against a host-stepped one -------------------------------------------------------------------------------
@pytest.mark.parametrize("interval,branch", [(2, 0), (3, 1)])
def test_fused_loop_matches_host_stepped_loop(interval, branch):
    """The same call two ways: the fused DDIM loop, and per step one deepcache_forward on [uncond | cond] (full with a capture, or shallow),
    the CFG combine and the DDIM update in torch.  Bound: tests/test_ip2p_gpu.py's fused-versus-host-stepped 1e-3."""
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 5
    pipe = _pipe("tiny")
    eng = pipe.engine
    ctx = synthetic.make_context(cfg, B, seed=8)
    lat = synthetic.make_latents(cfg, [7, 8], L)
    pipe.enable_deepcache(cache_interval=interval, cache_branch_id=branch)
    out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, guidance_scale=S, output_type="latent").latents
    pipe.disable_deepcache()
    x = (lat * pipe.scheduler.init_noise_sigma).cuda()
    ts, a_t, a_p = _ddim(pipe, steps)
    eng.set_context(ctx)
    for i, t in enumerate(ts):
        e_u, e_c = eng.deepcache_forward(torch.cat([x, x]), float(t), branch, shallow=i % interval != 0).chunk(2)
        e = e_u + S * (e_c - e_u)
        x0 = (x - (1 - a_t[i]) ** 0.5 * e) / a_t[i] ** 0.5
        x = a_p[i] ** 0.5 * x0 + (1 - a_p[i]) ** 0.5 * e
    err = _rms_rel(out, x)
    report(f"deepcache_fused_vs_host_stepped[tiny,k{interval},b{branch}]", latents_rms_rel=err)
    eng.close()
    assert err < 1e-3, err


# ---- 5. off switches and counters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_interval_1_and_disable_are_bit_identical_to_the_plain_call(scheduler):
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 4
    n_evals = steps + (scheduler == "PNDMScheduler")
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    pipe = _pipe("tiny", scheduler)
    plain = _call(pipe, ctx, lat, steps)                        # never heard of DeepCache
    pipe.enable_deepcache(cache_interval=1)
    one = _call(pipe, ctx, lat, steps)
    assert torch.equal(one[0], plain[0]) and np.array_equal(one[1], plain[1]) and torch.equal(one[2], plain[2])
    assert pipe.engine.deepcache_counts() == (0, 0)
    pipe.enable_deepcache(cache_interval=3, cache_branch_id=1)
    on = _call(pipe, ctx, lat, steps)
    flags = R.schedule(n_evals, 3)
    assert not torch.equal(on[0], plain[0])
    assert pipe.engine.deepcache_counts() == (sum(1 for i in range(n_evals - 1) if flags[i] and not flags[i + 1]), flags.count(False))
    pipe.disable_deepcache()
    again = _call(pipe, ctx, lat, steps)                        # and the call after disable_deepcache is the plain one again
    assert torch.equal(again[0], plain[0]) and np.array_equal(again[1], plain[1]) and torch.equal(again[2], plain[2])
    # an explicit all-full flag list at the engine level: the state is set, every evaluation is the plain one, nothing is captured
    c0 = pipe.engine.deepcache_counts()
    pipe.engine.deepcache_set([1] * n_evals, 1)
    try:
        full = _call(pipe, ctx, lat, steps)
    finally:
        pipe.engine.deepcache_clear()
    assert torch.equal(full[0], plain[0]) and np.array_equal(full[1], plain[1]) and torch.equal(full[2], plain[2])
    assert pipe.engine.deepcache_counts() == c0
    pipe.engine.close()


# ---- 6. the recorders -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval,branch", [(2, 0), (3, 1)])
def test_hooker_sees_exactly_the_attn2_calls_that_run(interval, branch):
    """full x (all 16 attn2 layers) + shallow x (the b + 1 down and b + 2 up layers of the shallow walk)."""
    from agenda_amd import UNetCrossAttentionHooker, synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 5
    n_all, n_sh = _n_attn2(cfg.unet), R.shallow_attn2_layers(cfg.unet, branch)
    assert n_all == 16 and n_sh == 2 * branch + 3
    pipe = _pipe("tiny")
    ctx = synthetic.make_context(cfg, B, seed=19)
    lat = synthetic.make_latents(cfg, [20, 21], L)
    seen = {}
    for tag in ("plain", "dc"):
        if tag == "dc":
            pipe.enable_deepcache(cache_interval=interval, cache_branch_id=branch)
        hk = UNetCrossAttentionHooker(is_train=False, latent_hw=L)
        pipe.unet.set_attn_processor(hk)
        try:
            pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent")
            seen[tag] = (hk.num_recorded, hk.compute_global_heat_map().cpu())
        finally:
            pipe.unet.set_attn_processor("default")
    pipe.engine.close()
    flags = R.schedule(steps, interval)
    assert seen["plain"][0] == steps * n_all
    assert seen["dc"][0] == flags.count(True) * n_all + flags.count(False) * n_sh
    assert seen["dc"][1].shape == seen["plain"][1].shape == (B, cfg.max_tokens, L, L)
    assert torch.isfinite(seen["dc"][1]).all() and float(seen["dc"][1].abs().max()) > 0


# ---- 7. batch rows, a LoRA, FreeU -----------------------------------------------------------------------------------------------
def test_image_0_of_a_batch_matches_its_batch_1_run():
    """Image 0 of B = 2 against the B = 1 call on that seed and context, bit for bit (tests/test_ip2p_gpu.py asserts the same at these
    shapes: every kernel of the walk computes a row from that row's data alone, in a fixed order -- the capture copies rows).  A batch of
    three (six UNet rows) runs too; its image 0 is held to the fused-versus-host-stepped 1e-3, other row counts pick other kernel forms."""
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    L, steps = 16, 4
    pipe = _pipe("tiny")
    pipe.enable_deepcache(cache_interval=2, cache_branch_id=1)
    ctx3 = synthetic.make_context(cfg, 3, seed=13)
    lat3 = synthetic.make_latents(cfg, [14, 15, 16], L)
    ctx2, lat = torch.cat([ctx3[0:2], ctx3[3:5]]), lat3[0:2]
    lat2, _, hm2 = _call(pipe, ctx2, lat, steps)
    lat1, _, hm1 = _call(pipe, torch.cat([ctx3[0:1], ctx3[3:4]]), lat[0:1], steps)
    c0 = pipe.engine.deepcache_counts()
    lat3o, _, hm3 = _call(pipe, ctx3, lat3, steps)
    c1 = pipe.engine.deepcache_counts()
    pipe.engine.close()
    e, h = _rms_rel(lat2[0:1], lat1), _rel(hm2[0:1], hm1)
    e3 = _rms_rel(lat3o[0:1], lat1)
    report("deepcache_batch1[tiny,row=0]", latents_rms_rel=e, heat_map_rel=h, batch3_latents_rms_rel=e3)
    assert torch.equal(lat2[0:1], lat1) and torch.equal(hm2[0:1], hm1), (e, h)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (2, 2)
    assert torch.isfinite(lat3o).all() and e3 < 1e-3, e3


def _lora(cfg, u, scale):
    """tests/test_freeu_gpu.py's adapter: rank 4 on every target, and the host-merged fp32 weights at `scale`."""
    from agenda_amd import lora
    g = torch.Generator().manual_seed(31)
    rank, sd = 4, {}
    for m, (_, (n_out, n_in)) in lora.target_modules(cfg).items():
        k = "lora_unet_" + m.replace(".", "_")
        d, up = torch.randn(rank, n_in, generator=g) / n_in ** 0.5, torch.randn(n_out, rank, generator=g) * 0.05
        if m.endswith(("proj_in", "proj_out")) and not cfg.unet.use_linear_projection:
            d, up = d.reshape(rank, n_in, 1, 1), up.reshape(n_out, rank, 1, 1)
        sd[k + ".lora_down.weight"], sd[k + ".lora_up.weight"] = d, up
    um = dict(u)
    for e in lora.lora_to_engine(sd, cfg):
        k = e.key[len("unet."):]
        dw = (scale * e.alpha / e.down.shape[0]) * (e.up.double() @ e.down.double()).float()
        um[k] = (um[k].float().reshape(dw.shape) + dw).reshape(um[k].shape)
    return sd, um


@pytest.mark.parametrize("beside", ["lora", "freeu"])
def test_deepcache_beside_a_lora_and_freeu(beside):
    """The shallow walk reads the LoRA-merged matrices, and on tiny40 (two levels: the last up block is up block 1) FreeU acts inside it:
    against the restatement composed with theirs, with section 3's bound (the yardstick is the LoRA / FreeU call without DeepCache).  The
    state survives a LoRA scale change."""
    from agenda_amd import synthetic
    name = "tiny" if beside == "lora" else "tiny40"
    cfg, u, v = _weights(name)
    B, L, steps = 2, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    pipe = _pipe(name)
    kw, freeu, uw = {}, None, u
    if beside == "lora":
        sd, uw = _lora(cfg, u, 0.8)
        pipe.load_lora_weights(sd)
        kw = {"cross_attention_kwargs": {"scale": 0.8}}
    else:
        freeu = (0.9, 0.2, 1.5, 1.6)
        pipe.enable_freeu(*freeu)
    plain = _call(pipe, ctx, lat, steps, **kw)
    pipe.enable_deepcache(cache_interval=2, cache_branch_id=0)
    fu0 = pipe.engine.freeu_counts()
    got = _call(pipe, ctx, lat, steps, **kw)
    fu1 = pipe.engine.freeu_counts()
    assert pipe.engine.deepcache_counts() == (2, 2) and pipe._deepcache == (2, 0)
    pipe.engine.close()
    if beside == "freeu":                                       # two full walks x (2 + 2 layers of up blocks 0 and 1) + two shallow x 2 layers of up block 1
        assert sum(fu1) - sum(fu0) == 2 * 2 * (cfg.unet.layers_per_block + 1) + 2 * 2
    want_plain = _restated(uw, v, cfg, ctx, lat, steps, "ddim", 1, 0, freeu)
    want = _restated(uw, v, cfg, ctx, lat, steps, "ddim", 2, 0, freeu)
    _assert_relative(f"{name},ddim,{beside}", _figures(plain, want_plain), _figures(got, want), _rms_rel(got[0], plain[0]))


def test_deepcache_takes_guidance_rescale():
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    ctx = synthetic.make_context(cfg, 2, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], 16)
    pipe = _pipe("tiny")
    pipe.enable_deepcache(cache_interval=2)
    a = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=4, output_type="latent").latents.cpu()
    b = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=4, guidance_rescale=0.7, output_type="latent").latents.cpu()
    n = pipe.engine.guidance_rescale_counts()
    pipe.engine.close()
    assert n == 4 and torch.isfinite(b).all() and not torch.equal(a, b)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rigs():
    """tools/record_conditioning.py's engines: the 4-channel UNet with a ControlNet, GLIGEN fusers, a T2I-Adapter and an IP-Adapter loaded,
    the 8-channel InstructPix2Pix variant and the 9-channel inpainting variant."""
    from agenda_amd import config
    spec = importlib.util.spec_from_file_location("record_conditioning", os.path.join(ROOT, "tools", "record_conditioning.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = {"e4": mod.Rig(config.tiny(), True), "e8": mod.Rig(config.ip2p_variant(config.tiny()), False),
         "e9": mod.Rig(config.inpaint_variant(config.tiny()), False)}
    yield r
    for rig in r.values():
        rig.e.close()


ROW = {"cn": "deepcache: a ControlNet schedule is set; DeepCache with a ControlNet is not implemented",
       "gl": "deepcache: a GLIGEN schedule is set; DeepCache with GLIGEN is not implemented",
       "inp": "deepcache: an inpainting state is set; DeepCache with inpainting is not implemented",
       "i2p": "deepcache: an InstructPix2Pix state is set; DeepCache with InstructPix2Pix is not implemented",
       "ad": "deepcache: a T2I-Adapter schedule is set; DeepCache with a T2I-Adapter is not implemented",
       "ipa": "deepcache: an IP-Adapter image is set; DeepCache with an IP-Adapter is not implemented"}
FWD_ROW = {"cn": "deepcache_forward: a ControlNet schedule is set", "gl": "deepcache_forward: a GLIGEN schedule is set",
           "ad": "deepcache_forward: a T2I-Adapter schedule is set", "ipa": "deepcache_forward: an IP-Adapter image is set"}


def _x4(rows=4, L=16):
    return torch.randn(rows, 4, L, L, generator=torch.Generator().manual_seed(41)).cuda()


@pytest.mark.parametrize("state", ["cn", "gl", "inp", "ad", "ipa"])
def test_conflict_row_on_the_4_channel_engine(rigs, state):
    """Each state beside a DeepCache schedule is refused by name before the first launch, by the fused loops and by deepcache_forward."""
    from agenda_amd._lib import AgendaHipError
    rig = rigs["e4"]
    rig.clear(); rig.e.deepcache_clear()
    rig.context(2)
    try:
        # what a refused loop leaves behind: it fails before it invalidates anything, so a capture made through the seam before it is still
        # valid afterwards and the schedule is still set
        x = _x4()
        rig.e.deepcache_set([1, 0], 0)
        rig.e.deepcache_forward(x, 11.0, 0, shallow=False)
        kept = rig.e.deepcache_forward(x, 11.0, 0, shallow=True).cpu()
        c0 = rig.e.deepcache_counts()
        rig.set(state, 2)
        with pytest.raises(AgendaHipError) as ei:
            rig.denoise()
        assert ROW[state] in str(ei.value), str(ei.value)
        rig.clear()
        assert torch.equal(rig.e.deepcache_forward(x, 11.0, 0, shallow=True).cpu(), kept)
        with pytest.raises(AgendaHipError, match="deepcache: the schedule has 2 flags, this call runs 3"):      # (the flags are still there)
            rig.plms()
        c0 = (c0[0], c0[1] + 1)
        rig.set(state, 2)
        for loop, n in ((rig.denoise, 2), (rig.plms, 3), (rig.dpm, 2)) if state != "inp" else ((rig.denoise, 2),):
            rig.e.deepcache_set([1] + [0] * (n - 1), 0)
            with pytest.raises(AgendaHipError) as ei:
                loop()
            assert ROW[state] in str(ei.value), str(ei.value)
        rig.e.deepcache_clear()
        if state in FWD_ROW:
            rig.set(state, 1)
            with pytest.raises(AgendaHipError) as ei:
                rig.e.deepcache_forward(_x4(), 11.0, 0, shallow=False)
            assert FWD_ROW[state] in str(ei.value), str(ei.value)
        # with the DeepCache state cleared the same call runs (the state fits it)
        rig.set(state, 2)
        assert torch.isfinite(rig.denoise()).all()
    finally:
        rig.clear(); rig.e.deepcache_clear()
    assert rig.e.deepcache_counts() == c0


def test_conflict_rows_on_the_other_engines_and_entry_points(rigs):
    from agenda_amd._lib import AgendaHipError
    e8, e9, e4 = rigs["e8"], rigs["e9"], rigs["e4"]
    c0 = e4.e.deepcache_counts()
    try:
        e8.clear(); e8.context(2); e8.set("i2p", 2); e8.e.deepcache_set([1, 0], 0)
        with pytest.raises(AgendaHipError) as ei:
            e8.denoise()
        assert ROW["i2p"] in str(ei.value), str(ei.value)
        e9.clear(); e9.context(2); e9.set("inp", 2); e9.e.deepcache_set([1, 0], 0)      # the 9-channel mode
        with pytest.raises(AgendaHipError) as ei:
            e9.denoise()
        assert ROW["inp"] in str(ei.value), str(ei.value)
        e4.clear(); e4.context(2); e4.e.deepcache_set([1, 0], 0)
        with pytest.raises(AgendaHipError, match="denoise_panorama: a DeepCache schedule is set"):
            e4.panorama()
        e4.e.deepcache_set([1], 0)
        with pytest.raises(AgendaHipError, match="unet_forward_ts: a DeepCache schedule is set"):
            e4.forward(per_image=True)
        assert torch.isfinite(e4.forward()).all()                # agd_unet_forward_hw does not read the state
        # Perturbed-Attention Guidance beside DeepCache: refused by all three loops and by deepcache_forward
        mid = ["mid_block.attentions.0.transformer_blocks.0.attn1"]
        for loop, n in ((e4.denoise, 2), (e4.plms, 3), (e4.dpm, 2)):      # (PLMS x 2 steps is three evaluations)
            e4.e.deepcache_set([1] + [0] * (n - 1), 0); e4.e.pag_set([3.0] * n, mid)
            with pytest.raises(AgendaHipError, match="deepcache: a Perturbed-Attention Guidance schedule is set"):
                loop()
        e4.e.deepcache_clear(); e4.e.pag_set([3.0], mid)
        with pytest.raises(AgendaHipError, match="deepcache_forward: a Perturbed-Attention Guidance schedule is set"):
            e4.e.deepcache_forward(_x4(), 11.0, 0, shallow=False)
        e4.e.pag_clear()
        # the schedule's length is the call's evaluations
        e4.e.deepcache_set([1, 0, 0, 1, 0], 0)
        for loop in (e4.denoise, e4.plms, e4.dpm):
            with pytest.raises(AgendaHipError, match="deepcache: the schedule has 5 flags, this call runs"):
                loop()
        e4.e.deepcache_clear()
        assert torch.isfinite(e4.denoise()).all()
    finally:
        for r in (e4, e8, e9):
            r.clear(); r.e.deepcache_clear(); r.e.pag_clear()
    assert e4.e.deepcache_counts() == c0


def test_deepcache_set_refusals(rigs):
    from agenda_amd._lib import AgendaHipError
    rig = rigs["e4"]
    e = rig.e
    e.deepcache_clear()
    with pytest.raises(AgendaHipError, match="deepcache_set: flag 0 is shallow"):
        e.deepcache_set([0, 1], 0)
    with pytest.raises(AgendaHipError, match="deepcache_set: 0 flags"):
        e.deepcache_set([], 0)
    with pytest.raises(AgendaHipError, match="deepcache_set: flag 1 is 2"):
        e.deepcache_set([1, 2], 0)
    for bad in (2, -1, 7):
        with pytest.raises(AgendaHipError, match=f"deepcache_set: branch {bad} \\(this UNet has branches 0 .. 1"):
            e.deepcache_set([1, 0], bad)
        with pytest.raises(AgendaHipError, match=f"deepcache_forward: branch {bad} \\(this UNet has branches 0 .. 1"):
            e.deepcache_forward(_x4(), 11.0, bad, shallow=False)
    # a refused set leaves the state clear: a two-evaluation loop runs as the plain one
    c0 = e.deepcache_counts()
    rig.clear(); rig.context(2)
    assert torch.isfinite(rig.denoise()).all() and e.deepcache_counts() == c0


def test_shallow_without_a_valid_cache_is_refused_after_each_invalidating_call():
    """A capture is valid for one (rows, Lh, Lw, branch), until a fused loop, agd_set_context, a LoRA scale change, agd_freeu_set /
    agd_freeu_clear, agd_deepcache_set or agd_deepcache_clear.  Each refusal is a host-side status: the counters do not move."""
    from agenda_amd import synthetic
    from agenda_amd._lib import AgendaHipError
    cfg, u, v = _weights("tiny")
    pipe = _pipe("tiny")
    e = pipe.engine
    sd, _ = _lora(cfg, u, 0.8)
    pipe.load_lora_weights(sd)
    ctx = synthetic.make_context(cfg, 2, seed=6)
    x = _x4()
    e.set_context(ctx)
    no = "without a valid cache"

    def refused(xx=x, branch=0):
        c = e.deepcache_counts()
        with pytest.raises(AgendaHipError, match=no):
            e.deepcache_forward(xx, 11.0, branch, shallow=True)
        assert e.deepcache_counts() == c

    def capture():
        e.deepcache_forward(x, 11.0, 0, shallow=False)
        assert torch.isfinite(e.deepcache_forward(x, 11.0, 0, shallow=True)).all()
    refused()                                                   # nothing captured yet
    capture()
    refused(branch=1)                                           # another branch
    refused(xx=_x4(rows=2))                                     # other rows
    refused(xx=_x4(L=24))                                       # another size
    assert torch.isfinite(e.deepcache_forward(x, 11.0, 0, shallow=True)).all()      # (the refusals left the capture whole)
    e.set_context(ctx); refused()
    capture(); e.lora_set_scale(0.5); refused(); e.set_context(ctx)
    capture(); e.freeu_set(0.9, 0.2, 1.2, 1.4); refused()
    capture(); e.freeu_clear(); refused()
    capture(); e.deepcache_clear(); refused()
    capture(); e.deepcache_set([1, 0], 0); refused(); e.deepcache_clear()
    capture()
    e.denoise(synthetic.make_latents(cfg, [1, 2], 16).cuda().contiguous(), *_ddim(pipe, 2), S)      # a loop invalidates at its start and its end
    refused()
    e.close()


def test_pipeline_value_errors_and_state_after_an_error():
    from agenda_amd import StableDiffusionInpaintPipeline, StableDiffusionPanoramaPipeline, _lib, config, synthetic
    cfg, u, v = _weights("tiny")
    pipe = _pipe("tiny")
    ctx = synthetic.make_context(cfg, 2, seed=1)
    lat = synthetic.make_latents(cfg, [1, 2], 16)
    for kw, msg in (({"cache_interval": 0}, "cache_interval=0"), ({"cache_interval": 2.0}, "cache_interval=2.0"),
                    ({"cache_branch_id": 2}, "cache_branch_id=2"), ({"skip_mode": "pow"}, "skip_mode='pow'")):
        with pytest.raises(ValueError, match=msg):
            pipe.enable_deepcache(**kw)
    pipe.enable_deepcache(cache_interval=2)
    with pytest.raises(ValueError, match="DeepCache .* with pag_scale=3.0"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, pag_scale=3.0)
    assert pipe.to("cuda") is pipe and pipe._deepcache == (2, 0)         # to() leaves the state alone
    # an error inside the call clears the engine's flags: a direct two-evaluation loop is not refused for a schedule of four
    def boom(*a):
        raise RuntimeError("boom")
    real, pipe._denoise = pipe._denoise, boom
    with pytest.raises(RuntimeError, match="boom"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=4, output_type="latent")
    pipe._denoise = real
    c0 = pipe.engine.deepcache_counts()
    x = pipe.engine.denoise(lat.cuda().contiguous().clone(), *_ddim(pipe, 2), S)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and pipe.engine.deepcache_counts() == c0
    pipe.engine.close()
    pano = StableDiffusionPanoramaPipeline(cfg, u, v, workspace_bytes=1 << 30)
    pano.enable_deepcache()
    with pytest.raises(ValueError, match="not implemented for StableDiffusionPanoramaPipeline"):
        pano(prompt_embeds=ctx[[0, 2]], num_inference_steps=2)
    pano.engine.close()
    icfg = config.inpaint_variant(config.tiny())
    inp = StableDiffusionInpaintPipeline.from_synthetic(icfg, workspace_bytes=1 << 30)
    inp.enable_deepcache(cache_interval=2)
    with pytest.raises(ValueError, match="not implemented for StableDiffusionInpaintPipeline"):
        inp(prompt_embeds=ctx, image=torch.zeros(2, 3, 128, 128), mask_image=torch.zeros(2, 1, 128, 128))
    inp.engine.close()


def test_pipeline_refuses_an_active_ip_adapter_before_any_device_work():
    """A loaded IP-Adapter with an image prompt and a non-zero scale beside an enabled DeepCache is a ValueError raised from the call's
    arguments: nothing is projected, no context is set, no counter moves.  At scale 0, and without an image prompt, the adapter is idle and
    the call is the DeepCache call of a pipeline without one, bit for bit."""
    from agenda_amd import ip_adapter as A
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    E = 96
    pipe = _pipe("tiny")
    ctx = synthetic.make_context(cfg, 2, seed=1)
    lat = synthetic.make_latents(cfg, [1, 2], 16)
    emb = torch.randn(2, E, generator=torch.Generator().manual_seed(5))
    run = lambda **kw: pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=4, output_type="latent", **kw).latents.cpu()
    pipe.enable_deepcache(cache_interval=2)
    want = run()
    pipe.load_ip_adapter(A.make_ip_adapter_weights(cfg, 21, E))
    c0, i0 = pipe.engine.deepcache_counts(), pipe.engine.ip_adapter_counts()
    for call in (lambda: run(ip_adapter_image_embeds=emb),
                 lambda: pipe.img2img(image=torch.zeros(2, 3, 128, 128), prompt_embeds=ctx, num_inference_steps=4, ip_adapter_image_embeds=emb)):
        with pytest.raises(ValueError, match=r"DeepCache \(cache_interval=2, cache_branch_id=0\) .* with an active IP-Adapter \(scale 1.0\)"):
            call()
    assert pipe.engine.deepcache_counts() == c0 and pipe.engine.ip_adapter_counts() == i0 and not pipe.engine._ipa_rows
    assert torch.equal(run(), want)                             # no image prompt: the adapter is idle
    pipe.set_ip_adapter_scale(0.0)
    assert torch.equal(run(ip_adapter_image_embeds=emb), want)  # scale 0: idle too
    pipe.set_ip_adapter_scale(1.0)
    pipe.disable_deepcache()
    assert torch.isfinite(run(ip_adapter_image_embeds=emb)).all()      # and without DeepCache the image prompt runs
    pipe.engine.close()


# ---- 9. the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_writes_images_and_heat_maps(tmp_path):
    from PIL import Image
    save = tmp_path / "out"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--synthetic-config", "tiny", "--deepcache-interval", "2", "--deepcache-branch", "1",
           "--save-dir", str(save), "--num-images", "3", "--batch-size", "3", "--num-inference-steps", "3", "--image-size", "128",
           "--word_token_heatmaps", "cars", "--prompt", "an aerial view with cars"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for sub in ("images", "daam_cars_heatmaps"):
        assert sorted(os.listdir(save / sub)) == ["0.png", "1.png", "2.png"], (sub, os.listdir(save))
    assert Image.open(save / "images" / "0.png").size == (128, 128)
