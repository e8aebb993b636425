"""guidance_rescale, DDIM's trailing spacing and the zero-terminal-SNR table on the device: the factor kernel through its op seam against
the float64 restatement (tests/_guidance_restated.py), the three step kernels through the loop entry points against a host-stepped loop on
the same device UNet, the off switch bit for bit, `pipe(..., guidance_rescale=0.7)` end to end under DDIM, PNDM and DPM-Solver++ with DAAM
on, the zero-SNR schedule end to end, the rescale beside a ControlNet, a LoRA, a rectangular call and FreeU, and the error contract."""
import copy
import math

import numpy as np
import pytest
import torch

import _guidance_restated as R
from _report import report

pytestmark = pytest.mark.gpu
G, PHI = 7.5, 0.7


def _rms_rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


_W = {}


def _weights():
    """(cfg, unet, vae with encoder) of the tiny config, drawn once per session as tests/test_freeu_gpu.py draws them."""
    if not _W:
        from agenda_amd import config, synthetic
        cfg = config.tiny()
        _W["tiny"] = (cfg, synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1),
                      synthetic.make_vae_weights(cfg, 12, with_encoder=True, bias_std=0.05, perturb_norm=0.1))
    return _W["tiny"]


def _pipe(scheduler="DDIMScheduler", cfg=None, ws=2 << 30):
    from agenda_amd import StableDiffusionPipeline
    c, u, v = _weights()
    return StableDiffusionPipeline(cfg or c, u, v, workspace_bytes=ws, scheduler=scheduler)


def _call(pipe, ctx, lat, steps, **kw):
    from agenda_amd import trace
    B = lat.shape[0]
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="np", **kw)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    return out.latents.cpu(), out.images, hm


# ---- 1. the op seam -------------------------------------------------------------------------------------------------------------
# (B, C, HW, ldc): 64 pixels = fewer than the workgroup's 1024 threads; 192 = no power of two; 4096 = 512 px, four pixels a thread, three
# images; 9216 = 768 px, nine a thread; ldc 8 = rows wider than the latent, the padding filled with 1e6 so that a read of it shows.
OP_SHAPES = [(1, 4, 64, 4), (2, 4, 192, 4), (3, 4, 4096, 4), (1, 4, 9216, 4), (2, 4, 384, 8)]
OP_DRAWS = [(0.0, 1.0), (3.0, 0.5), (10.0, 0.1)]
# torch's own fp32 std is within 1.3e-7 of float64 on these inputs (fp32 rounding through a pairwise sum of at most 36 864 terms); a naive
# sum / sum-of-squares kernel errs by 1.2e-4 to 8e-4 on the (10, 0.1) draws.  The bound sits between, about 80 times the reference's error.
OP_BOUND = 1e-5


def _eps(B, C, HW, ldc, mean, std, seed):
    g = torch.Generator().manual_seed(seed)
    eu = mean + std * torch.randn(B, HW, C, generator=g)
    ec = eu + 0.3 * std * torch.randn(B, HW, C, generator=g)
    eps = torch.full((2 * B, HW, ldc), 1e6)
    eps[:B, :, :C], eps[B:, :, :C] = eu, ec
    return eu, ec, eps.contiguous()


@pytest.mark.parametrize("B,C,HW,ldc", OP_SHAPES, ids=lambda v: str(v))
def test_op_seam_matches_float64_restatement(B, C, HW, ldc):
    from agenda_amd import ops
    worst = 0.0
    for k, (mean, std) in enumerate(OP_DRAWS):
        eu, ec, eps = _eps(B, C, HW, ldc, mean, std, 100 * HW + k)
        want = R.factor(eu, ec, G, PHI)
        dev = eps.cuda()
        got = ops.guidance_rescale(dev, C, G, PHI).cpu()
        again = ops.guidance_rescale(dev, C, G, PHI).cpu()
        err = float(((got.double() - want) / want).abs().max())
        ref32 = float(((R.factor(eu, ec, G, PHI, torch.float32).double() - want) / want).abs().max())
        print(f"guidance factor {(B, C, HW, ldc)} draw {(mean, std)}: rel err {err:.2e} (torch fp32 std: {ref32:.2e}), f = {got.tolist()}")
        worst = max(worst, err)
        assert torch.equal(got, again), "two runs differ"
        assert err <= OP_BOUND, (mean, std, err)
        assert ((got > 1 - PHI) & (got <= 1)).all()
        assert torch.equal(ops.guidance_rescale(dev, C, G, 0.0).cpu(), torch.ones(B)), "phi = 0 is exactly 1"
        for b in range(B):                               # an image alone is the same bits as the image in its batch
            alone = torch.cat([eps[b:b + 1], eps[B + b:B + b + 1]]).contiguous().cuda()
            assert torch.equal(ops.guidance_rescale(alone, C, G, PHI).cpu(), got[b:b + 1]), b
    report(f"guidance_factor[{B},{C},{HW},{ldc}]", max_rel=worst)


@pytest.mark.parametrize("value", [0.0, 0.1, -3.25, 10.0])
def test_op_seam_constant_input_gives_exactly_one(value):
    """std(m) == 0 where diffusers divides by zero: f = 1 (and sums of a constant that do not round to it exactly change nothing,
    m and eps_c being the same bits)."""
    from agenda_amd import ops
    for HW, ldc in ((64, 4), (4096, 4), (384, 8)):
        eps = torch.full((6, HW, ldc), value).cuda()
        assert torch.equal(ops.guidance_rescale(eps, 4, G, PHI).cpu(), torch.ones(3)), (value, HW)


# ---- 2. the step kernels --------------------------------------------------------------------------------------------------------
def _device_eps(e, x, t):
    """The device UNet on the CFG pair of host latents x (float64) at timestep t: (eps_u, eps_c) in float64."""
    eps = e.unet_forward(torch.cat([x, x]).float().cuda().contiguous(), float(np.float32(t))).cpu().double()
    return eps.chunk(2)


def _rescaled(eu, ec, fs=None):
    m = eu + G * (ec - eu)
    f = R.factor(eu, ec, G, PHI)
    if fs is not None:
        fs.append(f)
    return f.view(-1, 1, 1, 1) * m


def _step_inputs():
    from agenda_amd import synthetic
    cfg = _weights()[0]
    return synthetic.make_context(cfg, 2, seed=31), synthetic.make_latents(cfg, [7, 8], 16)


def test_ddim_step_kernel_applies_the_factor():
    """One evaluation through agd_denoise_hw against a float64 step on the same device UNet's eps; tolerance of
    tests/test_model_gpu.py::test_cfg_ddim_step_matches_oracle (2e-5 of the largest value)."""
    ctx, lat0 = _step_inputs()
    pipe = _pipe()
    e = pipe.engine
    e.set_context(ctx)
    ts = pipe.scheduler.set_timesteps(4)[:1]
    a_t, a_p = (v[:1] for v in pipe.scheduler.step_coeffs())
    outs = {}
    for phi in (0.0, PHI):
        e.guidance_rescale_set(phi)
        outs[phi] = e.denoise(lat0.clone().cuda(), ts, a_t, a_p, G).cpu()
        e.guidance_rescale_clear()
    assert e.guidance_rescale_counts() == 1
    x = lat0.double()
    eu, ec = _device_eps(e, x, ts[0])
    e.close()
    at, ap = float(a_t[0]), float(a_p[0])
    for phi, m in ((0.0, eu + G * (ec - eu)), (PHI, _rescaled(eu, ec))):
        x0 = (x - (1 - at) ** 0.5 * m) / at ** 0.5
        want = ap ** 0.5 * x0 + (1 - ap) ** 0.5 * m
        err = float((outs[phi].double() - want).abs().max() / want.abs().max())
        print(f"ddim step phi = {phi}: max rel {err:.2e}")
        report(f"guidance_step[ddim,phi={phi}]", max_rel=err)
        assert err < 2e-5, (phi, err)
    assert not torch.equal(outs[0.0], outs[PHI])


def test_plms_step_kernel_stores_the_rescaled_history():
    """Three evaluations (num_inference_steps 2) through agd_denoise_plms_hw: evaluation 1 averages with the stored e0 and evaluation 2
    extrapolates from it, so a history that kept the unscaled e0 would show.  Tolerance of the host-stepped loop in tests/test_dpm_gpu.py."""
    ctx, lat0 = _step_inputs()
    pipe = _pipe("PNDMScheduler")
    e = pipe.engine
    e.set_context(ctx)
    pipe.scheduler.set_timesteps(2)
    ts, ca, cb = (np.asarray(p, dtype=np.float64) for p in pipe.scheduler.plms_program())
    assert len(ts) == 3
    e.guidance_rescale_set(PHI)
    fused = e.denoise_plms(lat0.clone().cuda(), ts, ca, cb, G).cpu()
    e.guidance_rescale_clear()
    assert e.guidance_rescale_counts() == 3
    x = lat0.double()
    fs = []
    e0 = _rescaled(*_device_eps(e, x, ts[0]), fs)
    kept, x = x, (ca[0] * x + cb[0] * e0).float().double()
    e1 = _rescaled(*_device_eps(e, x, ts[1]), fs)
    wrong = (ca[1] * kept + cb[1] * 0.5 * (e1 + e0 / fs[0].view(-1, 1, 1, 1))).float().double()      # (an unscaled history)
    x = (ca[1] * kept + cb[1] * 0.5 * (e1 + e0)).float().double()
    e2 = _rescaled(*_device_eps(e, x, ts[2]), fs)
    x = (ca[2] * x + cb[2] * (1.5 * e2 - 0.5 * e0)).float().double()
    e.close()
    err, apart = _rms_rel(fused, x), _rms_rel(wrong, x)
    print(f"plms 3 evaluations, rescaled history: rms rel {err:.2e}; f = {[f.tolist() for f in fs]}")
    report("guidance_step[plms]", latents_rms_rel=err)
    assert err < 1e-4, err
    assert all(float(f.max()) < 0.99 for f in fs) and apart > 100 * err, (fs, apart)


def test_dpm_step_kernel_applies_the_factor():
    """Two evaluations through agd_denoise_dpm_hw (the second reads the stored x0 of the first); tolerance of
    tests/test_dpm_gpu.py::test_fused_dpm_loop_matches_host_stepped_loop."""
    ctx, lat0 = _step_inputs()
    pipe = _pipe("DPMSolverMultistepScheduler")
    e = pipe.engine
    e.set_context(ctx)
    pipe.scheduler.set_timesteps(2)
    prog = pipe.scheduler.dpm_program()
    ts, cx, ce, a, b0, b1 = (np.asarray(p, dtype=np.float64) for p in prog)
    e.guidance_rescale_set(PHI)
    fused = e.denoise_dpm(lat0.clone().cuda(), *prog, G).cpu()
    e.guidance_rescale_clear()
    assert e.guidance_rescale_counts() == 2
    x = lat0.double()
    prev = torch.zeros_like(x)
    for i in range(2):
        x0 = cx[i] * x + ce[i] * _rescaled(*_device_eps(e, x, ts[i]))
        x = (a[i] * x + b0[i] * x0 + b1[i] * prev).float().double()
        prev = x0
    e.close()
    err = _rms_rel(fused, x)
    print(f"dpm 2 evaluations: rms rel {err:.2e}")
    report("guidance_step[dpm]", latents_rms_rel=err)
    assert err < 1e-4, err


# ---- 3. off is off --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheduler,extra", [("DDIMScheduler", 0), ("PNDMScheduler", 1), ("DPMSolverMultistepScheduler", 0)])
def test_off_is_bit_identical_to_a_pipeline_that_never_rescaled(scheduler, extra):
    from agenda_amd import synthetic
    cfg = _weights()[0]
    B, L, steps = 2, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    plain_pipe = _pipe(scheduler)                        # never saw the argument
    plain = _call(plain_pipe, ctx, lat, steps)
    assert plain_pipe.engine.guidance_rescale_counts() == 0
    plain_pipe.engine.close()
    pipe = _pipe(scheduler)
    on = _call(pipe, ctx, lat, steps, guidance_rescale=PHI)
    assert pipe.engine.guidance_rescale_counts() == steps + extra          # one factor launch per evaluation
    assert not torch.equal(on[0], plain[0])
    for kw in ({}, {"guidance_rescale": 0.0}):
        res = _call(pipe, ctx, lat, steps, **kw)
        assert torch.equal(res[0], plain[0]) and np.array_equal(res[1], plain[1]) and torch.equal(res[2], plain[2]), kw
        assert pipe.engine.guidance_rescale_counts() == steps + extra, kw
    # a call that raises inside the loop's host part (after the state was set) leaves the engine clear
    with pytest.raises(ValueError, match="num_inference_steps|num_train_timesteps"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2000, output_type="latent", guidance_rescale=PHI)
    res = _call(pipe, ctx, lat, steps)
    assert torch.equal(res[0], plain[0]) and torch.equal(res[2], plain[2])
    assert pipe.engine.guidance_rescale_counts() == steps + extra
    pipe.engine.close()


# ---- 4 / 5. the pipeline against the restated loop, and that it is on -------------------------------------------------------------
@pytest.mark.parametrize("scheduler,key,n_evals", [("DDIMScheduler", "ddim", 6), ("PNDMScheduler", "pndm", 7), ("DPMSolverMultistepScheduler", "dpm", 6)])
def test_pipeline_matches_restatement(scheduler, key, n_evals):
    """guidance_rescale = 0.7 against the restated loop, and in the same run the plain pipeline against the plain restated loop for the
    same seeds.  The rescaled errors may be at most twice the plain ones: f_b lies in (1 - phi, 1] for g > 1 and is an average over at
    least 1024 values, so it adds no error of its own; the factor 2 (6.02 dB) covers the two trajectories diverging.  And they stay inside
    tests/test_adapter_gpu.py's pipeline bounds: 0.06, 30 dB, 0.06."""
    from agenda_amd import synthetic
    from oracle import sd_oracle as O
    cfg, u, v = _weights()
    B, L, steps = 2, 16, 6
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    fig, lats, fs = {}, {}, []
    for tag, phi in (("plain", 0.0), ("rescaled", PHI)):
        rec = O.DaamRecorder(L * L, context_size=cfg.max_tokens)
        want_img, want_lat = R.generate(u, v, cfg, ctx, lat, steps, key, phi, G, recorder=rec, factors=fs)
        whm = rec.compute_global_heat_map()
        pipe = _pipe(scheduler)
        got_lat, got_img, hm = _call(pipe, ctx, lat, steps, **({"guidance_rescale": phi} if phi else {}))
        assert pipe.engine.guidance_rescale_counts() == (n_evals if phi else 0)
        pipe.engine.close()
        fig[tag] = (_rms_rel(got_lat, want_lat), _psnr(got_img, want_img), _rms_rel(hm, whm))
        lats[tag] = got_lat
        assert float(hm.sum(1).mean()) == pytest.approx(n_evals, rel=0.02)      # the rescale adds no model evaluation
    (pl, pp, ph), (fl, fp, fh) = fig["plain"], fig["rescaled"]
    moved = _rms_rel(lats["rescaled"], lats["plain"])
    print(f"guidance_rescale pipe {key}: latents rms rel {fl:.4f} (plain {pl:.4f}), PSNR {fp:.1f} dB (plain {pp:.1f}), heat map rms rel {fh:.4f} "
          f"(plain {ph:.4f}); rescaled and plain latents are {moved:.3f} apart; f in [{min(float(f.min()) for f in fs):.3f}, {max(float(f.max()) for f in fs):.3f}]")
    report(f"guidance_pipeline[{key}]", latents_rms_rel=fl, psnr_db=fp, heat_map_rms_rel=fh, plain_latents_rms_rel=pl, plain_psnr_db=pp,
           plain_heat_map_rms_rel=ph, moved=moved)
    assert fl <= 2 * pl, (fl, pl)
    assert fp >= pp - 20 * math.log10(2), (fp, pp)
    assert fh <= 2 * ph, (fh, ph)
    assert fl < 0.06 and fp > 30.0 and fh < 0.06, (fl, fp, fh)
    assert moved > 2 * fl, (moved, fl)                   # it is on


# ---- 6. the zero-SNR schedule end to end ----------------------------------------------------------------------------------------
def _vcfg(spacing="leading", zero_snr=False):
    from agenda_amd.config import SchedulerConfig
    cfg = copy.deepcopy(_weights()[0])
    cfg.sched = SchedulerConfig(prediction_type="v_prediction", ddim_timestep_spacing=spacing, rescale_betas_zero_snr=zero_snr)
    return cfg


def test_zero_snr_trailing_ddim_end_to_end():
    """The tiny UNet read as a v-prediction model.  trailing + rescale_betas_zero_snr: the first evaluation is at t = 999 where alpha = 0
    (x0 = -v, the direction term is the sample itself).  Its error against the restated loop may be at most twice that of the same
    config under leading spacing and the plain table; the same again with guidance_rescale = 0.7."""
    from agenda_amd import synthetic
    _, u, v = _weights()
    B, L, steps = 2, 16, 4
    base_cfg, z_cfg = _vcfg(), _vcfg("trailing", True)
    ctx = synthetic.make_context(base_cfg, B, seed=41)
    lat = synthetic.make_latents(base_cfg, [1, 2], L)
    err = {}
    for tag, cfg, spacing, zs, phi in (("leading", base_cfg, "leading", False, 0.0), ("zero_snr", z_cfg, "trailing", True, 0.0),
                                       ("zero_snr+rescale", z_cfg, "trailing", True, PHI)):
        _, want = R.generate(u, v, cfg, ctx, lat, steps, "ddim", phi, G, spacing=spacing, zero_snr=zs)
        pipe = _pipe(cfg=cfg)
        ts = pipe.scheduler.set_timesteps(steps)
        if zs:
            assert ts[0] == 999 and pipe.scheduler.step_coeffs()[0][0] == 0.0
        got_lat, got_img, hm = _call(pipe, ctx, lat, steps, **({"guidance_rescale": phi} if phi else {}))
        assert pipe.engine.guidance_rescale_counts() == (steps if phi else 0)
        pipe.engine.close()
        assert torch.isfinite(got_lat).all() and torch.isfinite(hm).all() and np.isfinite(got_img.astype(np.float64)).all(), tag
        assert torch.isfinite(want).all()
        err[tag] = _rms_rel(got_lat, want)
    print(f"zero-SNR trailing ddim x {steps}: latents rms rel {err['zero_snr']:.4f}, with guidance_rescale {err['zero_snr+rescale']:.4f} "
          f"(leading, plain table: {err['leading']:.4f})")
    report("guidance_zero_snr[ddim]", latents_rms_rel=err["zero_snr"], rescaled_latents_rms_rel=err["zero_snr+rescale"],
           leading_latents_rms_rel=err["leading"])
    assert err["zero_snr"] <= 2 * err["leading"], err
    assert err["zero_snr+rescale"] <= 2 * err["leading"], err


def test_epsilon_pipeline_refuses_a_zero_alpha_timestep():
    from agenda_amd import synthetic
    from agenda_amd.config import SchedulerConfig
    cfg = copy.deepcopy(_weights()[0])
    cfg.sched = SchedulerConfig(ddim_timestep_spacing="trailing", rescale_betas_zero_snr=True)
    pipe = _pipe(cfg=cfg)
    ctx = synthetic.make_context(cfg, 1, seed=41)
    lat = synthetic.make_latents(cfg, [1], 16)
    with pytest.raises(ValueError, match="alphas_cumprod == 0"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=4, output_type="latent")
    pipe.engine.close()


def test_img2img_follows_the_trailing_grid():
    """strength 0.5 of 4 steps: the last 2 timesteps of the trailing grid [999 749 499 249] -- two evaluations, counted by the factor
    launches, starting from the noise level of t = 499."""
    from agenda_amd import synthetic
    cfg = _vcfg("trailing", True)
    pipe = _pipe(cfg=cfg)
    assert list(pipe.scheduler.set_timesteps(4)) == [999, 749, 499, 249]
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=41)
    g = torch.Generator().manual_seed(9)
    img = torch.rand(B, 3, 8 * L, 8 * L, generator=g) * 2 - 1
    kw = dict(prompt_embeds=ctx, image=img, strength=0.5, num_inference_steps=4, output_type="latent",
              noise_enc=torch.randn(B, 4, L, L, generator=g), noise=torch.randn(B, 4, L, L, generator=g))
    plain = pipe.img2img(**kw).latents.cpu()
    assert pipe.engine.guidance_rescale_counts() == 0
    on = pipe.img2img(guidance_rescale=PHI, **kw).latents.cpu()
    assert pipe.engine.guidance_rescale_counts() == 2
    again = pipe.img2img(**kw).latents.cpu()
    pipe.engine.close()
    lead = _pipe(cfg=_vcfg())
    other = lead.img2img(**kw).latents.cpu()
    lead.engine.close()
    assert torch.isfinite(on).all() and torch.equal(again, plain) and not torch.equal(on, plain)
    assert not torch.equal(other, plain)                 # the leading grid [751 501 251 1] starts elsewhere


# ---- 7. beside other code -------------------------------------------------------------------------------------------------------
def _beside(tag, want, want_off, got):
    err, moved = _rms_rel(got, want), _rms_rel(want_off, want)
    print(f"guidance_rescale + {tag}: latents rms rel {err:.4f} (without the rescale the restatement is {moved:.3f} away)")
    report(f"guidance_beside[{tag}]", latents_rms_rel=err, moved=moved)
    assert err < 0.06, err
    assert moved > 2 * err, (moved, err)


def test_rescale_beside_a_controlnet():
    import _controlnet_restated as CR
    from agenda_amd import StableDiffusionControlNetPipeline, synthetic
    from agenda_amd.config import ControlNetConfig
    from agenda_amd.controlnet import ControlNetModel
    cfg, u, v = _weights()
    c = synthetic.make_controlnet_weights(cfg, seed=13, bias_std=0.05, perturb_norm=0.1)
    B, L, steps = 2, 16, 3
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    u8 = (torch.rand(B, 3, 8 * L, 8 * L, generator=torch.Generator().manual_seed(23)) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    cond = u8.permute(0, 3, 1, 2).float() / 255.0
    cond2 = torch.cat([cond, cond])

    def eps_fn(x2, t, ctx_, rec):
        down, mid = CR.controlnet_forward(c, cfg.unet, x2, t, ctx_, cond2, 1.0)
        return CR.unet_forward_with_residuals(u, cfg.unet, x2, t, ctx_, down, mid, recorder=rec)

    _, want = R.generate(u, v, cfg, ctx, lat, steps, "ddim", PHI, G, eps_fn=eps_fn)
    _, want_off = R.generate(u, v, cfg, ctx, lat, steps, "ddim", 0.0, G, eps_fn=eps_fn)
    pipe = StableDiffusionControlNetPipeline(cfg, u, v, controlnet=ControlNetModel.from_config(cfg.unet, ControlNetConfig(), c), workspace_bytes=2 << 30)
    got = pipe(prompt_embeds=ctx, image=u8, latents=lat, num_inference_steps=steps, height=8 * L, width=8 * L, output_type="latent",
               guidance_rescale=PHI).latents.cpu()
    assert pipe.engine.guidance_rescale_counts() == steps
    pipe.engine.close()
    _beside("controlnet", want, want_off, got)


def test_rescale_beside_a_lora():
    from agenda_amd import lora, synthetic
    cfg, u, v = _weights()
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
        dw = (0.8 * e.alpha / e.down.shape[0]) * (e.up.double() @ e.down.double()).float()
        um[k] = (um[k].float().reshape(dw.shape) + dw).reshape(um[k].shape)
    B, L, steps = 2, 16, 3
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    _, want = R.generate(um, v, cfg, ctx, lat, steps, "ddim", PHI, G)
    _, want_off = R.generate(um, v, cfg, ctx, lat, steps, "ddim", 0.0, G)
    pipe = _pipe()
    pipe.load_lora_weights(sd)
    got = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", cross_attention_kwargs={"scale": 0.8},
               guidance_rescale=PHI).latents.cpu()
    pipe.engine.close()
    _beside("lora", want, want_off, got)


def test_rescale_on_a_rectangular_call():
    from agenda_amd import synthetic
    cfg, u, v = _weights()
    B, Lh, Lw, steps = 2, 16, 24, 3
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = torch.randn(B, 4, Lh, Lw, generator=torch.Generator().manual_seed(8))
    _, want = R.generate(u, v, cfg, ctx, lat, steps, "ddim", PHI, G)
    _, want_off = R.generate(u, v, cfg, ctx, lat, steps, "ddim", 0.0, G)
    pipe = _pipe()
    got = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, height=8 * Lh, width=8 * Lw, output_type="latent",
               guidance_rescale=PHI).latents.cpu()
    pipe.engine.close()
    _beside("rect[128x192]", want, want_off, got)


def test_rescale_beside_freeu():
    import _freeu_restated as FR
    from agenda_amd import synthetic
    cfg, u, v = _weights()
    sd15 = (0.9, 0.2, 1.5, 1.6)
    B, L, steps = 2, 16, 3
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    eps_fn = lambda x2, t, ctx_, rec: FR.unet_forward_with_freeu(u, cfg.unet, x2, t, ctx_, *sd15, recorder=rec)
    _, want = R.generate(u, v, cfg, ctx, lat, steps, "ddim", PHI, G, eps_fn=eps_fn)
    _, want_off = R.generate(u, v, cfg, ctx, lat, steps, "ddim", 0.0, G, eps_fn=eps_fn)
    pipe = _pipe()
    pipe.enable_freeu(*sd15)
    got = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", guidance_rescale=PHI).latents.cpu()
    assert pipe.unet.freeu == sd15
    pipe.engine.close()
    _beside("freeu", want, want_off, got)


# ---- 8. the error contract ------------------------------------------------------------------------------------------------------
def _no_launch(e, fn, match):
    """fn is refused with `match` in the message and nothing was launched: every kernel class counts 0, and so does the factor counter."""
    from agenda_amd import _lib
    n0 = e.guidance_rescale_counts()
    e.profile_begin()
    with pytest.raises((_lib.AgendaHipError, ValueError), match=match):
        fn()
    torch.cuda.synchronize()
    prof = e.profile_end()
    assert sum(p["launches"] for p in prof.values()) == 0, {k: p["launches"] for k, p in prof.items() if p["launches"]}
    assert e.guidance_rescale_counts() == n0


def test_error_contract():
    from agenda_amd import (StableDiffusionInstructPix2PixPipeline, StableDiffusionPanoramaPipeline, _lib, config, ops, synthetic)
    cfg, u, v = _weights()
    pipe = _pipe()
    e = pipe.engine
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    for bad in (-0.1, 1.5, float("nan")):
        _no_launch(e, lambda: e.guidance_rescale_set(bad), "guidance rescale phi = ")
        _no_launch(e, lambda: pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, output_type="latent", guidance_rescale=bad),
                   "guidance rescale takes a number in")
        _no_launch(e, lambda: pipe.img2img(prompt_embeds=ctx, image=torch.zeros(B, 3, 8 * L, 8 * L), num_inference_steps=2, output_type="latent",
                                           guidance_rescale=bad), "guidance rescale takes a number in")
        with pytest.raises(_lib.AgendaHipError, match="guidance rescale"):
            ops.guidance_rescale(torch.zeros(2, 64, 4).cuda(), 4, G, bad)
    # a refused set leaves the engine clear: the next call is the plain one
    out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, output_type="latent").latents
    assert torch.isfinite(out).all() and e.guidance_rescale_counts() == 0
    # one value per image has no standard deviation
    with pytest.raises(_lib.AgendaHipError, match="C \\* HW >= 2"):
        ops.guidance_rescale(torch.zeros(2, 1, 4).cuda(), 1, G, PHI)
    with pytest.raises(ValueError, match="2B, HW, ldc"):
        ops.guidance_rescale(torch.zeros(3, 64, 4).cuda(), 4, G, PHI)
    e.close()

    # the panorama pipeline: by name on the host, and the loop itself refuses a set state before its first launch
    pano = StableDiffusionPanoramaPipeline(cfg, u, v, workspace_bytes=2 << 30)
    pctx = synthetic.make_context(cfg, 1, seed=21)
    plat = torch.randn(1, 4, 16, 32, generator=torch.Generator().manual_seed(7))
    call = lambda **kw: pano(prompt_embeds=pctx, latents=plat, num_inference_steps=2, height=128, width=256, output_type="latent", **kw)
    _no_launch(pano.engine, lambda: call(guidance_rescale=PHI), "guidance rescale is not implemented for the panorama pipeline")
    pano.engine.set_context(pctx)
    pano.engine.guidance_rescale_set(PHI)
    ts = pano.scheduler.set_timesteps(2)
    a_t, a_p = pano.scheduler.step_coeffs()
    _no_launch(pano.engine, lambda: pano.engine.denoise_panorama(plat.clone().cuda(), 16, 8, None, ts, a_t, a_p, G),
               "denoise_panorama: guidance rescale")
    pano.engine.guidance_rescale_clear()
    assert torch.isfinite(call().latents).all()
    pano.engine.close()

    # InstructPix2Pix: by name on the host, and the three-branch loop refuses a set state
    icfg = config.ip2p_variant(config.tiny())
    iu = synthetic.make_unet_weights(icfg, 11, bias_std=0.05, perturb_norm=0.1)
    ip = StableDiffusionInstructPix2PixPipeline(icfg, iu, v, workspace_bytes=2 << 30)
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (B, 8 * L, 8 * L, 3), dtype=np.uint8))
    nz = torch.randn(B, icfg.unet.out_channels, L, L, generator=torch.Generator().manual_seed(7))
    icall = lambda **kw: ip(prompt_embeds=ctx, image=img, latents=nz, num_inference_steps=2, output_type="latent", **kw)
    _no_launch(ip.engine, lambda: icall(guidance_rescale=PHI), "guidance rescale is not implemented for the InstructPix2Pix pipeline")
    ip.engine.guidance_rescale_set(PHI)
    with pytest.raises(_lib.AgendaHipError, match="the InstructPix2Pix denoise loop: guidance rescale"):
        icall()
    assert ip.engine.guidance_rescale_counts() == 0
    ip.engine.guidance_rescale_clear()
    assert torch.isfinite(icall().latents).all()
    ip.engine.close()
