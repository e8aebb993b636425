"""DPM-Solver++ (2M) on the device (`agd_denoise_dpm`, `cfg_dpm_kernel`): the fused loop through `pipe(...)` against the fp32 CPU
oracle's UNet stepped by this suite's own restatement of the solver (tests/_dpm_restated.py), DAAM recording on; the fused loop
against a host-stepped loop; the checkpoint round trip and the error contract."""
import json
import math

import numpy as np
import pytest
import torch

import _dpm_restated as R
from _report import report

pytestmark = pytest.mark.gpu


def _rel(got, want):
    got = got.detach().float().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def _rms_rel(got, want):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _oracle_dpm(u, v, cfg, ctx, lat, steps, karras, guidance=7.5, recorder=None):
    """The oracle's UNet / VAE (oracle/sd_oracle.py), stepped by the restated DPM-Solver++ 2M; returns (uint8 images, latents)."""
    from oracle import sd_oracle as O

    def model(x, i, t):
        eps = O.unet_forward(u, cfg.unet, torch.cat([x, x], 0), torch.tensor(t, dtype=torch.float32), ctx, recorder)
        eu, ec = eps.chunk(2)
        return eu + guidance * (ec - eu)

    with torch.no_grad():
        _, x = R.sample(steps, karras, cfg.sched.prediction_type, model, lat.clone().float())
        img = O.postprocess_image(O.vae_decode(v, cfg.vae, x / cfg.vae.scaling_factor))
    return img, x


def _pipe(cfg, u, v, karras=False, ws=1 << 30):
    from agenda_amd import StableDiffusionPipeline
    cfg.sched.use_karras_sigmas = karras
    return StableDiffusionPipeline(cfg, u, v, workspace_bytes=ws, scheduler="DPMSolverMultistepScheduler")


@pytest.mark.parametrize("cfgname,karras,L", [("tiny", False, 16), ("tiny", True, 16), ("tiny21", False, 24)])
def test_dpm_generation_matches_oracle(cfgname, karras, L):
    """B = 2, 8 steps, DAAM on: latents, image and heat maps within the PNDM test's bounds; one recorded evaluation per step."""
    from agenda_amd import config, synthetic, trace
    from agenda_amd.scheduler import DPMSolverMultistepScheduler
    from oracle import sd_oracle as O
    cfg = config.CONFIGS[cfgname]()
    u = synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)
    v = synthetic.make_vae_weights(cfg, 12, bias_std=0.05, perturb_norm=0.1)
    pipe = _pipe(cfg, u, v, karras, ws=2 << 30)
    assert isinstance(pipe.scheduler, DPMSolverMultistepScheduler) and pipe.scheduler.use_karras_sigmas == karras
    B, steps = 2, 8
    ctx = synthetic.make_context(cfg, B, seed=51)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    rec = O.DaamRecorder(L * L, context_size=cfg.max_tokens)
    want_img, want_lat = _oracle_dpm(u, v, cfg, ctx, lat, steps, karras, recorder=rec)
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, height=8 * L, width=8 * L, output_type="np")
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    whm = rec.compute_global_heat_map()
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(hm, whm)
    print(f"dpm {cfgname} karras={karras}: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map rel {e_hm:.4f}")
    report(f"dpm_generation[{cfgname},karras={karras}]", latents_rms_rel=e_lat, psnr_db=psnr, heat_map_rel=e_hm)
    assert e_lat < 0.06, e_lat
    assert psnr > 30.0, psnr
    assert float(hm.sum(1).mean()) == pytest.approx(steps, rel=0.02)          # one recorded UNet evaluation per step
    assert e_hm < 0.06, e_hm
    pipe.engine.close()


@pytest.mark.parametrize("karras", [False, True])
def test_fused_dpm_loop_matches_host_stepped_loop(karras):
    """`agd_denoise_dpm` vs `engine.unet_forward` of the CFG pair + a float64 host update with the same coefficient program:
    pins the kernel and the device loop's history handling apart from UNet error (the same UNet runs on both sides)."""
    from agenda_amd import config, synthetic
    cfg = config.tiny()
    u = synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)
    v = synthetic.make_vae_weights(cfg, 12, bias_std=0.05, perturb_norm=0.1)
    pipe = _pipe(cfg, u, v, karras)
    B, L, steps, g = 2, 16, 6, 7.5
    ctx = synthetic.make_context(cfg, B, seed=31)
    lat0 = synthetic.make_latents(cfg, [7, 8], L)
    fused = pipe(prompt_embeds=ctx, latents=lat0, num_inference_steps=steps, output_type="latent").latents.cpu()
    pipe.scheduler.set_timesteps(steps)
    ts, cx, ce, a, b0, b1 = (np.asarray(p, dtype=np.float64) for p in pipe.scheduler.dpm_program())
    pipe.engine.set_context(ctx)
    x = lat0.clone().double()
    prev = torch.zeros_like(x)
    for i in range(steps):
        eps = pipe.engine.unet_forward(torch.cat([x, x]).float().cuda().contiguous(), float(np.float32(ts[i]))).cpu().double()
        eu, ec = eps.chunk(2)
        x0 = cx[i] * x + ce[i] * (eu + g * (ec - eu))
        x = (a[i] * x + b0[i] * x0 + b1[i] * prev).float().double()       # the latents are stored in fp32 between steps
        prev = x0
    e = _rms_rel(fused, x)
    print(f"fused vs host-stepped DPM loop (karras={karras}): rms rel {e:.2e}")
    report(f"dpm_fused_vs_host_stepped[karras={karras}]", latents_rms_rel=e)
    assert e < 1e-4, e
    pipe.engine.close()


def test_config1_sd15_256px_10_dpm_steps_end_to_end_vs_oracle():
    """SD-1.5 shapes, 1 x 256 x 256, 10 DPM-Solver++ 2M steps, CFG 7.5, DAAM on, against the fp32 CPU oracle stepped by the
    restatement; config 1's bounds (tests/test_fullsize_gpu.py)."""
    from agenda_amd import config, synthetic, trace
    from oracle import sd_oracle as O
    cfg = config.sd15()
    u = synthetic.make_unet_weights(cfg, 1234)
    v = synthetic.make_vae_weights(cfg, 1235)
    pipe = _pipe(cfg, u, v, ws=4 << 30)
    L, steps = 32, 10
    ctx = synthetic.make_context(cfg, 1, seed=7)
    lat = synthetic.make_latents(cfg, [0], L)
    rec = O.DaamRecorder(L * L, context_size=77)
    want_img, want_lat = _oracle_dpm(u, v, cfg, ctx, lat, steps, False, recorder=rec)
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, height=256, width=256, num_inference_steps=steps, output_type="np")
        got = trc.compute_global_heat_map(prompt=None, image_index=0).heat_maps.cpu()
    want = rec.compute_global_heat_map()[0]
    lat_err, psnr = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img)
    hm_err = float((got - want).abs().max() / want.abs().max())
    print(f"config1 DPM++ 2M: latents rms rel {lat_err:.4f}, image PSNR {psnr:.1f} dB, heat map rel {hm_err:.4f}")
    report("config1_256px_10_dpm_steps_end_to_end", latents_rms_rel=lat_err, psnr_db=psnr, heat_map_rel=hm_err)
    assert lat_err < 0.05, lat_err
    assert psnr > 36.0, psnr
    assert hm_err < 0.02, hm_err
    pipe.engine.close()


def _write_checkpoint(path, cfg, u, v, sched_json):
    from safetensors.torch import save_file
    for sub in ("unet", "vae", "scheduler"):
        (path / sub).mkdir(parents=True)
    uc = {"in_channels": 4, "out_channels": 4, "block_out_channels": list(cfg.unet.block_out_channels),
          "down_block_types": ["CrossAttnDownBlock2D" if c else "DownBlock2D" for c in cfg.unet.down_cross],
          "layers_per_block": cfg.unet.layers_per_block, "attention_head_dim": list(cfg.unet.num_heads),
          "cross_attention_dim": cfg.unet.cross_attention_dim, "use_linear_projection": False, "norm_num_groups": 32,
          "sample_size": cfg.default_sample_size}
    vc = {"latent_channels": 4, "out_channels": 3, "block_out_channels": list(cfg.vae.block_out_channels),
          "layers_per_block": cfg.vae.layers_per_block, "norm_num_groups": 32, "scaling_factor": cfg.vae.scaling_factor}
    json.dump(uc, open(path / "unet" / "config.json", "w"))
    json.dump(vc, open(path / "vae" / "config.json", "w"))
    json.dump(sched_json, open(path / "scheduler" / "scheduler_config.json", "w"))
    save_file({k: t.contiguous() for k, t in u.items()}, str(path / "unet" / "diffusion_pytorch_model.safetensors"))
    save_file({k: t.contiguous() for k, t in v.items()}, str(path / "vae" / "diffusion_pytorch_model.safetensors"))


def test_from_pretrained_round_trip_and_errors(tmp_path):
    """A checkpoint whose scheduler_config.json names DPMSolverMultistepScheduler (Karras on) loads as that scheduler and runs the
    same loop as the in-memory pipeline; save_pretrained -> from_pretrained keeps scheduler and options; a PNDM checkpoint
    overridden with scheduler="DPMSolverMultistepScheduler" gets DPM's defaults.  Error contract of agd_denoise_dpm."""
    from agenda_amd import StableDiffusionPipeline, config, synthetic
    from agenda_amd._lib import AgendaHipError
    from agenda_amd.pipeline import Engine
    from agenda_amd.scheduler import DPMSolverMultistepScheduler
    cfg = config.tiny()
    u = synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)
    v = synthetic.make_vae_weights(cfg, 12, bias_std=0.05, perturb_norm=0.1)
    sj = {"_class_name": "DPMSolverMultistepScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012,
          "beta_schedule": "scaled_linear", "steps_offset": 1, "prediction_type": "epsilon", "algorithm_type": "dpmsolver++",
          "solver_order": 2, "solver_type": "midpoint", "lower_order_final": True, "use_karras_sigmas": True,
          "timestep_spacing": "linspace", "lambda_min_clipped": -float("inf"), "thresholding": False, "variance_type": None}
    _write_checkpoint(tmp_path / "dpm", cfg, u, v, sj)
    B, L, steps = 1, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=3)
    lat = synthetic.make_latents(cfg, [5], L)
    p1 = StableDiffusionPipeline.from_pretrained(str(tmp_path / "dpm"), workspace_bytes=1 << 30)
    assert isinstance(p1.scheduler, DPMSolverMultistepScheduler) and p1.scheduler.use_karras_sigmas
    a = p1(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent").latents.cpu()
    ref = _pipe(config.tiny(), u, v, karras=True)
    b = ref(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent").latents.cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    p1.save_pretrained(str(tmp_path / "saved"))
    p2 = StableDiffusionPipeline.from_pretrained(str(tmp_path / "saved"), workspace_bytes=1 << 30)
    assert isinstance(p2.scheduler, DPMSolverMultistepScheduler) and p2.scheduler.use_karras_sigmas
    p2.engine.close()
    # a PNDM checkpoint, DPM by override; save_pretrained then writes a DPM config that reloads as DPM
    pj = {"_class_name": "PNDMScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012, "steps_offset": 1,
          "set_alpha_to_one": False, "prediction_type": "epsilon", "skip_prk_steps": True}
    _write_checkpoint(tmp_path / "pndm", cfg, u, v, pj)
    p3 = StableDiffusionPipeline.from_pretrained(str(tmp_path / "pndm"), workspace_bytes=1 << 30, scheduler="DPMSolverMultistepScheduler")
    assert isinstance(p3.scheduler, DPMSolverMultistepScheduler) and not p3.scheduler.use_karras_sigmas
    p3.save_pretrained(str(tmp_path / "saved3"))
    sj3 = json.load(open(tmp_path / "saved3" / "scheduler" / "scheduler_config.json"))
    assert sj3["_class_name"] == "DPMSolverMultistepScheduler" and sj3["use_karras_sigmas"] is False
    p3.engine.close()
    # unsupported DPM options in a checkpoint, and a PNDM-only option given to DPM, are refused
    _write_checkpoint(tmp_path / "dpm3", cfg, u, v, dict(sj, solver_order=3))
    with pytest.raises(ValueError):
        StableDiffusionPipeline.from_pretrained(str(tmp_path / "dpm3"), workspace_bytes=1 << 28)
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(skip_prk_steps=True)
    # error contract: context batch mismatch, no evaluations, unfinalised context -- reported through agd_last_error
    p1.engine.set_context(ctx)
    x3 = synthetic.make_latents(cfg, [1, 2, 3], L).cuda()
    p1.scheduler.set_timesteps(2)
    prog = p1.scheduler.dpm_program()
    with pytest.raises(AgendaHipError, match="context batch"):
        p1.engine.denoise_dpm(x3, *prog, 7.5)
    with pytest.raises(AgendaHipError, match="evaluation"):
        p1.engine.denoise_dpm(x3[:1].contiguous(), [], [], [], [], [], [], 7.5)
    eng = Engine(cfg, 0, 1 << 28)
    with pytest.raises(AgendaHipError, match="finalize"):
        eng.denoise_dpm(x3[:1].contiguous(), *prog, 7.5)
    eng.close()
    p1.engine.close(); ref.engine.close()
