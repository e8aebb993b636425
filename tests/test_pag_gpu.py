"""Perturbed-Attention Guidance on the device: the two kernels through their op seams, one perturbed UNet forward and whole loops against
the fp32 restatement (tests/_pag_restated.py) with the plain call's own error as the yardstick, the exact properties of the off switch,
the schedule, the counters, batch rows, the recorders and the engine state a call leaves behind, every refusal, the CLI, and PAG beside a
LoRA and FreeU.  No test here provokes a fault: every refusal tested is a host-side status returned before any launch."""
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _pag_restated as R
from _report import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, P = 7.5, 3.0                       # guidance_scale, pag_scale
# Linear error propagation: the combined prediction e_u + s (e_c - e_u) + p (e_c - e_p) carries (2 s - 1 + 2 p) / (2 s - 1) = 1.43 times
# the plain combine's error at these scales; a margin of 2 over that for step-to-step amplification gives 3 x, or 20 log10(3) = 9.5 dB
LOOP_FACTOR, LOOP_DB = 3.0, 9.5
FWD_FACTOR = 2.0                      # one forward: the same arithmetic with one attention per applied layer removed


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
    """(cfg, unet, vae) of a config, drawn once per session: the tiny configs as tests/test_pag_cpu.py draws them."""
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


def _layers(name, pats):
    from agenda_amd import config
    return config.resolve_pag_layers(_weights(name)[0], pats)


def _ddim(pipe, steps):
    ts = pipe.scheduler.set_timesteps(steps)
    a_t, a_p = pipe.scheduler.step_coeffs()
    return ts, a_t, a_p


# ---- 1. the op seams ------------------------------------------------------------------------------------------------------------
# one row of one vector-of-8 block per thread trip; 63 x 320 and 257 x 640: odd row counts, more than one workgroup; 64 x 1280: 160 vectors a row
@pytest.mark.parametrize("M,C", [(1, 64), (63, 320), (257, 640), (64, 1280)])
def test_v_rows_is_the_value_third_bit_for_bit(M, C):
    from agenda_amd import ops
    qkv = torch.randn(M, 3 * C, generator=torch.Generator().manual_seed(M + C)).to(torch.bfloat16)
    got = ops.pag_v_rows(qkv.cuda()).cpu()
    assert got.shape == (M, C) and got.dtype == torch.bfloat16
    assert torch.equal(got, qkv[:, 2 * C:])


def test_v_rows_refuses_rows_that_are_no_multiple_of_8():
    from agenda_amd import _lib, ops
    with pytest.raises(_lib.AgendaHipError, match="multiple of 8"):
        ops.pag_v_rows(torch.zeros(4, 36, dtype=torch.bfloat16).cuda())          # C = 12


@pytest.mark.parametrize("n", [1, 255, 4099])
def test_fold_is_the_fp32_expression_bit_for_bit(n):
    from agenda_amd import ops
    eps = torch.randn(3, n, generator=torch.Generator().manual_seed(n))
    got = ops.pag_fold(eps.cuda(), P).cpu()
    d = P * (eps[1] - eps[2])
    assert torch.equal(got[0], eps[0] + d) and torch.equal(got[1], eps[1] + d)
    assert torch.equal(got[0], eps[0] + P * (eps[1] - eps[2]))                    # the torch expression as written
    assert torch.equal(got[2], eps[2])
    same = eps.clone()
    same[2] = same[1]                                                             # e_p == e_c: both rows untouched
    got = ops.pag_fold(same.cuda(), P).cpu()
    assert torch.equal(got, same)
    assert torch.equal(ops.pag_fold(eps.cuda(), 0.0).cpu(), eps)


def test_fold_refuses_a_bad_scale():
    from agenda_amd import _lib, ops
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.AgendaHipError, match="pag_fold"):
            ops.pag_fold(torch.zeros(3, 8).cuda(), bad)


# ---- 2. one perturbed forward ---------------------------------------------------------------------------------------------------
# tiny / tiny40 with every layer: tiny40 is the C = 320 / 640 plans (the qkv chain; attn1.to_out inside the attn2 chain).  sd15: the mid block
# alone, then the 64-wide C = 320 layers of both ends.
FWD_CASES = [("tiny", [None]), ("tiny40", [None]), ("tiny21", [["mid"]]), ("sd15", [["mid"], ["down_blocks.0", "up_blocks.3"]])]


@pytest.mark.parametrize("name,layer_sets", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_perturbed_forward_matches_restatement(name, layer_sets):
    """agd_unet_forward_hw under a length-1 schedule, two rows at 16 x 16, t = 301.  The bound is the plain forward's own rms-rel error
    against the plain oracle forward, measured here, times 2."""
    from agenda_amd import config, synthetic
    from oracle import sd_oracle as O
    cfg, u, v = _weights(name)
    ctx = synthetic.make_context(cfg, 1, seed=6)
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    t = 301.0
    pipe = _pipe(name)
    e = pipe.engine
    e.set_context(ctx)
    plain = e.unet_forward(x, t).cpu()
    assert e.pag_counts() == (0, 0)
    e.pag_set([0.0], _layers(name, ["mid"]))                    # a zero scale: the plain forward, launch for launch
    assert torch.equal(e.unet_forward(x, t).cpu(), plain) and e.pag_counts() == (0, 0)
    got = []
    for pats in layer_sets:
        names = config.self_attn_layer_names(cfg) if pats is None else _layers(name, pats)
        c0 = e.pag_counts()
        e.pag_set([P], names)
        got.append((names, e.unet_forward(x, t).cpu()))
        assert e.pag_counts() == (c0[0] + 1, c0[1] + len(names))
    e.pag_clear()
    assert torch.equal(e.unet_forward(x, t).cpu(), plain)       # cleared: the plain UNet again, bit for bit
    e.close()
    with torch.no_grad():
        rows = lambda f: torch.cat([f(x[i:i + 1], ctx[i:i + 1]) for i in range(2)])       # one image at a time
        err_plain = _rms_rel(plain, rows(lambda xi, ci: O.unet_forward(u, cfg.unet, xi, torch.tensor(t), ci)))
        for (names, out), pats in zip(got, layer_sets):
            want = rows(lambda xi, ci: R.unet_forward_perturbed(u, cfg.unet, xi, torch.tensor(t), ci, names))
            err, moved = _rms_rel(out, want), _rms_rel(plain, want)
            print(f"pag forward {name} {pats or 'all'}: rms rel {err:.5f} (plain {err_plain:.5f}; the plain forward is {moved:.3f} away)")
            report(f"pag_forward[{name},{'+'.join(pats) if pats else 'all'}]", rms_rel=err, plain_rms_rel=err_plain)
            assert not torch.equal(out, plain)
            assert err <= FWD_FACTOR * err_plain, (err, err_plain)


# ---- 3. loops -------------------------------------------------------------------------------------------------------------------
LOOP_CASES = [("tiny", "DDIMScheduler", "ddim", 6, 16, 16), ("tiny", "PNDMScheduler", "pndm", 6, 16, 16),
              ("tiny", "DPMSolverMultistepScheduler", "dpm", 6, 16, 16), ("tiny", "DDIMScheduler", "ddim", 6, 16, 24),
              ("tiny40", "DDIMScheduler", "ddim", 4, 16, 16), ("sd15", "DDIMScheduler", "ddim", 3, 32, 32)]
LOOP_LAYERS = {"tiny": ["mid", "up_blocks.1"], "tiny40": ["mid", "up_blocks.1"], "sd15": ["mid"]}


def _call(pipe, ctx, lat, steps, **kw):
    from agenda_amd import trace
    B, Lh, Lw = lat.shape[0], lat.shape[2], lat.shape[3]
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, height=8 * Lh, width=8 * Lw, guidance_scale=S, output_type="np", **kw)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    return out.latents.cpu(), out.images, hm


def _restated(u, v, cfg, ctx, lat, steps, key, p, a, names, freeu=None):
    from _aspect_restated import AspectDaamRecorder
    rec = AspectDaamRecorder((lat.shape[2], lat.shape[3]), context_size=cfg.max_tokens)
    img, x, walks = R.generate(u, v, cfg, ctx, lat, steps, key, S, p, a, names, rec, freeu=freeu)
    return x, img, rec.compute_global_heat_map(), walks


def _figures(got, want):
    (lat, img, hm), (wlat, wimg, whm) = got, want[:3]
    assert hm.shape == whm.shape and img.shape == wimg.shape
    return _rms_rel(lat, wlat), _psnr(img, wimg), max(_rel(hm[i], whm[i]) for i in range(hm.shape[0]))


def _assert_relative(tag, plain, pag):
    (pl, pp, ph), (gl, gp, gh) = plain, pag
    print(f"pag {tag}: latents rms rel {gl:.4f} (plain {pl:.4f}), PSNR {gp:.1f} dB (plain {pp:.1f}), heat map max rel {gh:.4f} (plain {ph:.4f})")
    report(f"pag_loop[{tag}]", latents_rms_rel=gl, psnr_db=gp, heat_map_rel=gh, plain_latents_rms_rel=pl, plain_psnr_db=pp, plain_heat_map_rel=ph)
    assert gl <= LOOP_FACTOR * pl, ("latents", gl, pl)
    assert gh <= LOOP_FACTOR * ph, ("heat map", gh, ph)
    assert gp >= pp - LOOP_DB, ("psnr", gp, pp)


@pytest.mark.parametrize("name,scheduler,key,steps,Lh,Lw", LOOP_CASES, ids=[f"{c[0]}-{c[2]}-{c[4]}x{c[5]}" for c in LOOP_CASES])
def test_loop_matches_restatement(name, scheduler, key, steps, Lh, Lw):
    """B = 2, guidance_scale 7.5, pag_scale 3, DAAM on: latents, decoded image and each image's heat map against the restatement, and in
    the same test the plain call against the plain oracle loop; PAG's errors may be 3 x the plain ones (9.5 dB)."""
    from agenda_amd import synthetic
    cfg, u, v = _weights(name)
    B = 2
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = torch.randn(B, 4, Lh, Lw, generator=torch.Generator().manual_seed(8))
    names = _layers(name, LOOP_LAYERS[name])
    pipe = _pipe(name, scheduler, pag_applied_layers=LOOP_LAYERS[name])
    plain = _call(pipe, ctx, lat, steps)
    c0 = pipe.engine.pag_counts()
    got = _call(pipe, ctx, lat, steps, pag_scale=P)
    c1 = pipe.engine.pag_counts()
    pipe.engine.close()
    want_plain = _restated(u, v, cfg, ctx, lat, steps, key, 0.0, 0.0, names)
    want = _restated(u, v, cfg, ctx, lat, steps, key, P, 0.0, names)
    n_evals = want[3]
    assert want_plain[3] == 0 and n_evals == steps + (key == "pndm")
    assert c0 == (0, 0) and c1 == (n_evals, n_evals * len(names))
    assert not torch.equal(want_plain[0], want[0]) and not torch.equal(got[0], plain[0])      # (the guidance moved the sample)
    assert float(got[2].sum(1).mean()) == pytest.approx(float(plain[2].sum(1).mean()), rel=0.02)   # the perturbed walk recorded nothing
    _assert_relative(f"{name},{key},{Lh}x{Lw}", _figures(plain, want_plain), _figures(got, want))


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
def test_pag_beside_a_lora_and_freeu(beside):
    """The perturbed branch reads the LoRA-merged attn1 matrices / runs FreeU like the other two branches: against the restatement composed
    with theirs, with the same relative bound (the yardstick is the LoRA / FreeU call without PAG)."""
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    names = _layers("tiny", ["mid", "down"])
    pipe = _pipe("tiny", pag_applied_layers=["mid", "down"])
    kw, freeu, uw = {}, None, u
    if beside == "lora":
        sd, uw = _lora(cfg, u, 0.8)
        pipe.load_lora_weights(sd)
        kw = {"cross_attention_kwargs": {"scale": 0.8}}
    else:
        freeu = (0.9, 0.2, 1.5, 1.6)
        pipe.enable_freeu(*freeu)
    plain = _call(pipe, ctx, lat, steps, **kw)
    got = _call(pipe, ctx, lat, steps, pag_scale=P, **kw)
    assert pipe.engine.pag_counts() == (steps, steps * len(names))
    pipe.engine.close()
    want_plain = _restated(uw, v, cfg, ctx, lat, steps, "ddim", 0.0, 0.0, names, freeu)
    want = _restated(uw, v, cfg, ctx, lat, steps, "ddim", P, 0.0, names, freeu)
    _assert_relative(f"tiny,ddim,{beside}", _figures(plain, want_plain), _figures(got, want))


# ---- 4. exact properties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_zero_scale_is_bit_identical_to_the_plain_call(scheduler):
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    pipe = _pipe("tiny", scheduler)
    plain = _call(pipe, ctx, lat, steps)                        # never saw the argument
    off = _call(pipe, ctx, lat, steps, pag_scale=0.0, pag_adaptive_scale=0.0)
    assert torch.equal(off[0], plain[0]) and np.array_equal(off[1], plain[1]) and torch.equal(off[2], plain[2])
    assert pipe.engine.pag_counts() == (0, 0)
    # an adaptive scale that zeroes every evaluation: the state is set, every evaluation is the plain one
    zero = _call(pipe, ctx, lat, steps, pag_scale=0.001, pag_adaptive_scale=1.0)
    assert torch.equal(zero[0], plain[0]) and np.array_equal(zero[1], plain[1]) and torch.equal(zero[2], plain[2])
    assert pipe.engine.pag_counts() == (0, 0)
    on = _call(pipe, ctx, lat, steps, pag_scale=P)
    assert not torch.equal(on[0], plain[0]) and pipe.engine.pag_counts()[0] == steps + (scheduler == "PNDMScheduler")
    again = _call(pipe, ctx, lat, steps)                        # and the call after a PAG call is the plain one again
    pipe.engine.close()
    assert torch.equal(again[0], plain[0]) and torch.equal(again[2], plain[2])


def test_adaptive_scale_runs_the_third_walk_only_where_the_scale_is_positive():
    from agenda_amd import config, synthetic
    from agenda_amd.inpaint import evaluation_timesteps
    cfg, u, v = _weights("tiny")
    B, L, steps, a = 2, 16, 6, 0.006
    pipe = _pipe("tiny", pag_applied_layers=["mid", "down"])
    sched = config.pag_schedule(evaluation_timesteps(pipe.scheduler, steps), P, a)
    nz = sum(1 for p in sched if p > 0)
    assert 0 < nz < steps and all(p == 0 for p in sched[nz:])
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    got = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, pag_scale=P, pag_adaptive_scale=a, output_type="latent").latents.cpu()
    counts = pipe.engine.pag_counts()
    pipe.engine.close()
    n_layers = len(_layers("tiny", ["mid", "down"]))
    assert counts == (nz, nz * n_layers)
    with torch.no_grad():
        _, want, walks = R.generate(u, v, cfg, ctx, lat, steps, "ddim", S, P, a, _layers("tiny", ["mid", "down"]), None)
    assert walks == nz
    assert _rms_rel(got, want) < 0.06                           # (tests/test_ip2p_gpu.py's loop bound; the relative bound is section 3's)


def test_no_applied_layers_is_the_plain_loop_up_to_kernel_forms():
    """layers = [] at the engine level, p = 3: e_p is e_c from a B-row walk without the CFG-shared prefix (other attn2 forms), so the result
    is the plain loop's to tests/test_ip2p_gpu.py's fused-versus-host-stepped bound (1e-3), not bit for bit."""
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 5
    pipe = _pipe("tiny")
    eng = pipe.engine
    eng.set_context(synthetic.make_context(cfg, B, seed=8))
    x = synthetic.make_latents(cfg, [7, 8], L).cuda().contiguous()
    prog = _ddim(pipe, steps)
    plain = eng.denoise(x.clone(), *prog, S).cpu()
    eng.pag_set([P] * steps, [])
    got = eng.denoise(x.clone(), *prog, S).cpu()
    counts = eng.pag_counts()
    eng.close()
    e = _rms_rel(got, plain)
    report("pag_no_layers_vs_plain[tiny]", latents_rms_rel=e)
    assert counts == (steps, 0)
    assert e < 1e-3, e


def test_fused_loop_matches_host_stepped_loop():
    """The same call two ways: the fused DDIM loop, and per step one plain unet_forward on [uncond | cond], one perturbed unet_forward on the
    cond rows, the three-term formula and the DDIM update in torch.  Bound: tests/test_ip2p_gpu.py's fused-versus-host-stepped 1e-3."""
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 5
    pats = ["mid", "up_blocks.1"]
    pipe = _pipe("tiny", pag_applied_layers=pats)
    eng = pipe.engine
    ctx = synthetic.make_context(cfg, B, seed=8)
    lat = synthetic.make_latents(cfg, [7, 8], L)
    out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, guidance_scale=S, pag_scale=P, output_type="latent").latents
    x = (lat * pipe.scheduler.init_noise_sigma).cuda()
    ts, a_t, a_p = _ddim(pipe, steps)
    for i, t in enumerate(ts):
        e_u, e_c = pipe.unet(torch.cat([x, x]), float(t), encoder_hidden_states=ctx).sample.chunk(2)
        eng.pag_set([P], _layers("tiny", pats))
        try:
            e_p = pipe.unet(x, float(t), encoder_hidden_states=ctx[B:]).sample
        finally:
            eng.pag_clear()
        e = R.combine(e_u, e_c, e_p, S, P)
        x0 = (x - (1 - a_t[i]) ** 0.5 * e) / a_t[i] ** 0.5
        x = a_p[i] ** 0.5 * x0 + (1 - a_p[i]) ** 0.5 * e
    err = _rms_rel(out, x)
    report("pag_fused_vs_host_stepped[tiny]", latents_rms_rel=err)
    eng.close()
    assert err < 1e-3, err


def test_image_0_of_a_batch_matches_its_batch_1_run():
    """Image 0 of B = 2 against the B = 1 call on that seed and context.  tests/test_ip2p_gpu.py asserts bit equality for this property at
    these shapes (every kernel of the walk computes a row from that row's data alone, in a fixed order); so does this."""
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 3
    pipe = _pipe("tiny", pag_applied_layers=["mid", "up_blocks.1"])
    ctx = synthetic.make_context(cfg, B, seed=13)
    lat = synthetic.make_latents(cfg, [14, 15], L)
    lat2, _, hm2 = _call(pipe, ctx, lat, steps, pag_scale=P)
    lat1, _, hm1 = _call(pipe, torch.cat([ctx[0:1], ctx[B:B + 1]]), lat[0:1], steps, pag_scale=P)
    pipe.engine.close()
    e, h = _rms_rel(lat2[0:1], lat1), _rel(hm2[0:1], hm1)
    report("pag_batch1[tiny,row=0]", latents_rms_rel=e, heat_map_rel=h)
    assert torch.equal(lat2[0:1], lat1) and torch.equal(hm2[0:1], hm1), (e, h)


def test_hooker_sees_the_main_walk_only():
    """16 attn2 maps per evaluation, the conditional half of the main walk, with and without PAG: none from the perturbed walk."""
    from agenda_amd import UNetCrossAttentionHooker, synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 2
    n_layers = sum(cfg.unet.down_cross) * (2 * cfg.unet.layers_per_block + 1) + 1
    assert n_layers == 16
    pipe = _pipe("tiny", pag_applied_layers=["mid", "down"])
    ctx = synthetic.make_context(cfg, B, seed=19)
    lat = synthetic.make_latents(cfg, [20, 21], L)
    seen = {}
    for tag, kw in (("plain", {}), ("pag", {"pag_scale": P})):
        hk = UNetCrossAttentionHooker(is_train=False, latent_hw=L)
        pipe.unet.set_attn_processor(hk)
        try:
            pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", **kw)
            seen[tag] = (hk.num_recorded, hk.compute_global_heat_map().cpu())
        finally:
            pipe.unet.set_attn_processor("default")
    assert pipe.engine.pag_counts()[0] == steps
    pipe.engine.close()
    assert seen["plain"][0] == seen["pag"][0] == steps * n_layers
    assert seen["pag"][1].shape == seen["plain"][1].shape == (B, cfg.max_tokens, L, L)
    assert torch.isfinite(seen["pag"][1]).all() and float(seen["pag"][1].abs().max()) > 0


def test_engine_state_after_a_call_and_after_a_refused_one():
    """After a PAG call, and after one refused for a wrong schedule length, the context batch, the recorder mode and every layer's K/V are
    as set_context left them: a following plain call is bit-identical to one on a fresh pipeline, and a direct agd_denoise on the context
    already set runs and gives the same latents."""
    from agenda_amd import _lib, synthetic, trace
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=2)
    lat = synthetic.make_latents(cfg, [5, 6], L)
    fresh = _pipe("tiny")
    want = _call(fresh, ctx, lat, steps)
    prog = _ddim(fresh, steps)
    # the same loop again on the context the call left (the tracer is gone, so nothing is recorded: other attn2 launches than `want`'s)
    want_direct = fresh.engine.denoise(lat.cuda().contiguous().clone(), *prog, S).cpu()
    fresh.engine.close()
    pipe = _pipe("tiny", pag_applied_layers=["mid", "up_blocks.1"])
    eng = pipe.engine
    _call(pipe, ctx, lat, steps, pag_scale=P)
    direct = eng.denoise(lat.cuda().contiguous().clone(), *prog, S).cpu()        # no set_context in between: the call's own is still whole
    assert torch.equal(direct, want_direct)
    after = _call(pipe, ctx, lat, steps)
    assert torch.equal(after[0], want[0]) and np.array_equal(after[1], want[1]) and torch.equal(after[2], want[2])
    # refused before the first launch: a schedule of the wrong length
    eng.pag_set([P] * (steps - 1), _layers("tiny", ["mid"]))
    c0 = eng.pag_counts()
    with trace(pipe):
        with pytest.raises(_lib.AgendaHipError, match=f"pag: the schedule has {steps - 1} scales, this call runs {steps} model evaluations"):
            pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent")
    eng.pag_clear()
    assert eng.pag_counts() == c0
    direct = eng.denoise(lat.cuda().contiguous().clone(), *prog, S).cpu()
    assert torch.equal(direct, want_direct)
    after = _call(pipe, ctx, lat, steps)
    assert torch.equal(after[0], want[0]) and np.array_equal(after[1], want[1]) and torch.equal(after[2], want[2])
    # an error inside the call clears the state: a two-evaluation loop is not refused for a schedule of four
    def boom(*a):
        raise RuntimeError("boom")
    real, pipe._denoise = pipe._denoise, boom
    with pytest.raises(RuntimeError, match="boom"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, pag_scale=P, output_type="latent")
    pipe._denoise = real
    x = eng.denoise(lat.cuda().contiguous().clone(), *_ddim(pipe, 2), S)
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and eng.pag_counts() == c0
    eng.close()


def test_img2img_takes_pag():
    from agenda_amd import StableDiffusionPipeline, synthetic
    cfg, u, _ = _weights("tiny")
    v = synthetic.make_vae_weights(cfg, 12, with_encoder=True, bias_std=0.05, perturb_norm=0.1)
    pipe = StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30)
    B, L, steps = 2, 16, 6
    ctx = synthetic.make_context(cfg, B, seed=3)
    img = torch.rand(B, 3, 8 * L, 8 * L, generator=torch.Generator().manual_seed(4)) * 2 - 1
    nz = torch.randn(2, B, 4, L, L, generator=torch.Generator().manual_seed(5))
    run = lambda **kw: pipe.img2img(image=img, strength=0.5, num_inference_steps=steps, prompt_embeds=ctx, noise_enc=nz[0], noise=nz[1],
                                    output_type="latent", **kw).latents.cpu()
    plain, on = run(), run(pag_scale=P)
    counts = pipe.engine.pag_counts()
    off = run(pag_scale=0.0)
    pipe.engine.close()
    assert counts == (3, 3)                                      # strength 0.5 of 6 steps: three evaluations, the mid block each
    assert torch.isfinite(on).all() and not torch.equal(on, plain) and torch.equal(off, plain)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
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


MID = ["mid_block.attentions.0.transformer_blocks.0.attn1"]
ROW = {"cn": "pag: a ControlNet schedule is set; Perturbed-Attention Guidance with a ControlNet is not implemented",
       "gl": "pag: a GLIGEN schedule is set; Perturbed-Attention Guidance with GLIGEN is not implemented",
       "inp": "pag: an inpainting state is set; Perturbed-Attention Guidance with inpainting is not implemented",
       "i2p": "pag: an InstructPix2Pix state is set; Perturbed-Attention Guidance with InstructPix2Pix is not implemented",
       "ad": "pag: a T2I-Adapter schedule is set; Perturbed-Attention Guidance with a T2I-Adapter is not implemented",
       "ipa": "pag: an IP-Adapter image is set; Perturbed-Attention Guidance with an IP-Adapter is not implemented"}


@pytest.mark.parametrize("state", ["cn", "gl", "inp", "ad", "ipa"])
def test_conflict_row_on_the_4_channel_engine(rigs, state):
    """Each state beside a PAG schedule is refused by name before the first launch, by the fused loops and by unet_forward."""
    from agenda_amd._lib import AgendaHipError
    rig = rigs["e4"]
    rig.clear(); rig.e.pag_clear()
    rig.context(2)
    c0 = rig.e.pag_counts()
    try:
        rig.set(state, 2)
        rig.e.pag_set([P, P], MID)
        for loop in (rig.denoise, rig.plms, rig.dpm) if state != "inp" else (rig.denoise,):
            with pytest.raises(AgendaHipError) as ei:
                loop()
            assert ROW[state] in str(ei.value), str(ei.value)
        rig.set(state, 1)
        rig.e.pag_set([P], MID)
        with pytest.raises(AgendaHipError) as ei:
            rig.forward()
        assert ROW[state] in str(ei.value), str(ei.value)
        # with the PAG state cleared the same call runs (the state fits it)
        rig.e.pag_clear()
        rig.set(state, 2)
        assert torch.isfinite(rig.denoise()).all()
    finally:
        rig.clear(); rig.e.pag_clear()
    assert rig.e.pag_counts() == c0


def test_conflict_row_on_the_other_engines_and_entry_points(rigs):
    from agenda_amd._lib import AgendaHipError
    e8, e9, e4 = rigs["e8"], rigs["e9"], rigs["e4"]
    try:
        e8.clear(); e8.context(2); e8.set("i2p", 2); e8.e.pag_set([P, P], MID)
        with pytest.raises(AgendaHipError) as ei:
            e8.denoise()
        assert ROW["i2p"] in str(ei.value), str(ei.value)
        e9.clear(); e9.context(2); e9.set("inp", 2); e9.e.pag_set([P, P], MID)      # the 9-channel mode
        with pytest.raises(AgendaHipError) as ei:
            e9.denoise()
        assert ROW["inp"] in str(ei.value), str(ei.value)
        e4.clear(); e4.context(2); e4.e.pag_set([P, P], MID)
        with pytest.raises(AgendaHipError, match="denoise_panorama: a Perturbed-Attention Guidance schedule is set"):
            e4.panorama()
        e4.e.pag_set([P], MID)
        with pytest.raises(AgendaHipError, match="unet_forward_ts: a Perturbed-Attention Guidance schedule is set"):
            e4.forward(per_image=True)
        # guidance rescale beside PAG: refused by all three loops, as the InstructPix2Pix loop refuses it
        e4.e.guidance_rescale_set(0.7)
        for loop, n in ((e4.denoise, 2), (e4.plms, 3), (e4.dpm, 2)):      # (PLMS x 2 steps is three evaluations)
            e4.e.pag_set([P] * n, MID)
            with pytest.raises(AgendaHipError, match=r"Perturbed-Attention Guidance denoise loop: guidance rescale \(phi = 0.7\) is set"):
                loop()
        e4.e.guidance_rescale_clear()
        # the schedule's length is the call's evaluations
        e4.e.pag_set([P] * 5, MID)
        for loop in (e4.denoise, e4.plms, e4.dpm, e4.forward):
            with pytest.raises(AgendaHipError, match="pag: the schedule has 5 scales, this call runs"):
                loop()
    finally:
        e4.e.guidance_rescale_clear()
        for r in (e4, e8, e9):
            r.clear(); r.e.pag_clear()


def test_pag_set_refusals(rigs):
    from agenda_amd._lib import AgendaHipError
    e = rigs["e4"].e
    e.pag_clear()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(AgendaHipError, match="pag_set: scale 1 is"):
            e.pag_set([P, bad], MID)
    with pytest.raises(AgendaHipError, match="pag_set: 0 scales"):
        e.pag_set([], MID)
    for bad in ("mid", "mid_block.attentions.0.transformer_blocks.0.attn2", "down_blocks.3.attentions.0.transformer_blocks.0.attn1",
                "controlnet.mid_block.attentions.0.transformer_blocks.0.attn1"):
        with pytest.raises(AgendaHipError) as ei:
            e.pag_set([P], MID + [bad])
        assert f"'{bad}' is not a self-attention layer" in str(ei.value)
    # a refused set leaves the state clear: a two-evaluation loop runs as the plain one
    c0 = e.pag_counts()
    rigs["e4"].clear(); rigs["e4"].context(2)
    assert torch.isfinite(rigs["e4"].denoise()).all() and e.pag_counts() == c0
    e.pag_set([P, P], [])                                        # no layers is accepted
    e.pag_clear()


def test_pipeline_value_errors():
    from agenda_amd import StableDiffusionInpaintPipeline, StableDiffusionPanoramaPipeline, StableDiffusionPipeline, config, synthetic
    cfg, u, v = _weights("tiny")
    with pytest.raises(ValueError, match="nowhere"):
        StableDiffusionPipeline(cfg, u, v, workspace_bytes=1 << 30, pag_applied_layers=["mid", "nowhere"])
    with pytest.raises(ValueError, match="nowhere"):
        StableDiffusionPipeline.from_synthetic("tiny", pag_applied_layers="nowhere")
    pipe = _pipe("tiny")
    assert pipe.pag_applied_layers == ["mid"]
    ctx = synthetic.make_context(cfg, 2, seed=1)
    lat = synthetic.make_latents(cfg, [1, 2], 16)
    for kw, msg in (({"pag_scale": -1.0}, "pag_scale"), ({"pag_scale": float("inf")}, "pag_scale"), ({"pag_adaptive_scale": 0.01}, "needs pag_scale > 0"),
                    ({"pag_scale": P, "pag_adaptive_scale": float("nan")}, "pag_adaptive_scale"), ({"pag_scale": P, "guidance_rescale": 0.7}, "guidance_rescale")):
        with pytest.raises(ValueError, match=msg):
            pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, **kw)
    with pytest.raises(ValueError, match="nowhere"):
        pipe.set_pag_applied_layers(["nowhere"])
    assert pipe.engine.pag_counts() == (0, 0)
    pipe.engine.close()
    pano = StableDiffusionPanoramaPipeline(cfg, u, v, workspace_bytes=1 << 30)
    with pytest.raises(ValueError, match="not implemented for StableDiffusionPanoramaPipeline"):
        pano(prompt_embeds=ctx[[0, 2]], num_inference_steps=2, pag_scale=P)
    pano.engine.close()
    icfg = config.inpaint_variant(config.tiny())
    inp = StableDiffusionInpaintPipeline.from_synthetic(icfg, workspace_bytes=1 << 30)
    with pytest.raises(ValueError, match="not implemented for StableDiffusionInpaintPipeline"):
        inp(prompt_embeds=ctx, image=torch.zeros(2, 3, 128, 128), mask_image=torch.zeros(2, 1, 128, 128), pag_scale=P)
    inp.engine.close()


# ---- 6. the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_writes_images_and_heat_maps(tmp_path):
    from PIL import Image
    save = tmp_path / "out"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--synthetic-config", "tiny", "--pag-scale", "3", "--pag-adaptive-scale", "0.001",
           "--pag-applied-layers", "mid", "up_blocks.1", "--save-dir", str(save), "--num-images", "3", "--batch-size", "3",
           "--num-inference-steps", "3", "--image-size", "128", "--word_token_heatmaps", "cars", "--prompt", "an aerial view with cars"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for sub in ("images", "daam_cars_heatmaps"):
        assert sorted(os.listdir(save / sub)) == ["0.png", "1.png", "2.png"], (sub, os.listdir(save))
    assert Image.open(save / "images" / "0.png").size == (128, 128)
