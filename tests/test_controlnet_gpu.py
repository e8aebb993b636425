"""ControlNet on the device: the 13 scaled residuals and one injected UNet forward against the fp32 restatement (tests/_controlnet_restated.py),
`pipe(prompt, image=...)` end to end under DDIM, PNDM and DPM-Solver++ with DAAM on, the guidance window, scale 0 against the plain
pipeline bit for bit, the error contract, and the checkpoint + CLI round trip."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _controlnet_restated as R
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


def _weights(cfg, small=True):
    from agenda_amd import synthetic
    kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
    u = synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw)
    v = synthetic.make_vae_weights(cfg, 12 if small else 1235, **kw)
    c = synthetic.make_controlnet_weights(cfg, seed=13 if small else 1236, **kw)
    return u, v, c


def _pipe(cfg, u, v, c, scheduler="DDIMScheduler", ws=2 << 30, cncfg=None):
    from agenda_amd import StableDiffusionControlNetPipeline
    from agenda_amd.config import ControlNetConfig
    from agenda_amd.controlnet import ControlNetModel
    return StableDiffusionControlNetPipeline(cfg, u, v, controlnet=ControlNetModel.from_config(cfg.unet, cncfg or ControlNetConfig(), c),
                                             workspace_bytes=ws, scheduler=scheduler)


def _cond(b, side, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(b, 3, side, side, generator=g)


# config, latent side, UNet rows, small weights (biases and norm perturbations, as the tiny parity tests draw them)
CASES = [("tiny", 16, 2, True), ("tiny21", 24, 2, True), ("sd15", 32, 2, False), ("sd15", 64, 8, False)]


def _split(flat, cfg, B2, L):
    from agenda_amd.config import controlnet_res_channels
    sizes, side = [], L
    ch = controlnet_res_channels(cfg.unet)
    k = 0
    sizes.append((ch[k], side)); k += 1
    for i in range(len(cfg.unet.block_out_channels)):
        for _ in range(cfg.unet.layers_per_block):
            sizes.append((ch[k], side)); k += 1
        if i != len(cfg.unet.block_out_channels) - 1:
            side //= 2
            sizes.append((ch[k], side)); k += 1
    sizes.append((cfg.unet.block_out_channels[-1], side))
    out, off = [], 0
    for c, s in sizes:
        n = B2 * c * s * s
        out.append(flat[off:off + n].view(B2, c, s, s))
        off += n
    assert off == flat.numel()
    return out


@pytest.mark.parametrize("name,L,B2,small", CASES)
def test_residuals_match_restatement(name, L, B2, small):
    from agenda_amd import config, synthetic
    cfg = config.CONFIGS[name]()
    u, v, c = _weights(cfg, small)
    pipe = _pipe(cfg, u, v, c, ws=6 << 30)
    ctx = synthetic.make_context(cfg, B2 // 2, seed=5)
    x = synthetic.make_latents(cfg, list(range(B2)), L)
    cond = _cond(B2, 8 * L, 21)
    t, scale = 501.0, 0.8
    pipe.engine.set_context(ctx)
    pipe.engine.controlnet_set_cond(cond, repeat=1)
    got = _split(pipe.engine.controlnet_residuals(x, t, scale).cpu(), cfg, B2, L)
    nhwc = pipe.engine.controlnet_residuals(x, t, scale, nhwc=True).cpu()
    with torch.no_grad():                                # one image at a time (the oracle's attention holds every score)
        parts = [R.controlnet_forward(c, cfg.unet, x[i:i + 1], torch.tensor(t), ctx[i:i + 1], cond[i:i + 1], scale) for i in range(B2)]
    want = [torch.cat([p_[0][k] for p_ in parts]) for k in range(12)] + [torch.cat([p_[1] for p_ in parts])]
    assert len(got) == 13 == len(want)
    errs = [_rms_rel(g_, w_) for g_, w_ in zip(got, want)]
    # NHWC is the same numbers in the other layout
    off = 0
    for g_ in got:
        n = g_.numel()
        assert torch.equal(nhwc[off:off + n].view(g_.shape[0], g_.shape[2], g_.shape[3], g_.shape[1]), g_.permute(0, 2, 3, 1)), "nhwc layout"
        off += n
    print(f"controlnet residuals {name} L={L} B2={B2}: rms rel max {max(errs):.4f} ({', '.join(f'{e:.3f}' for e in errs)})")
    report(f"controlnet_residuals[{name},L={L},B2={B2}]", rms_rel_max=max(errs))
    assert max(errs) < 0.03, errs
    pipe.engine.close()


def test_residuals_with_wide_embedding_and_bgr_match_restatement():
    """Embedding widths other than (16, 32, 96, 256) -- a first map wider than 64 channels -- and the BGR channel order, with the
    embedding set for [cond; cond]: the copies of the second half and the scratch sized by the widest stage."""
    from agenda_amd import config, synthetic
    cfg = config.tiny()
    cn = config.ControlNetConfig(conditioning_embedding_out_channels=(128, 192, 96, 320), conditioning_channel_order="bgr")
    u, v, _ = _weights(cfg)
    c = synthetic.make_controlnet_weights(cfg, cn, seed=14, bias_std=0.05, perturb_norm=0.1)
    pipe = _pipe(cfg, u, v, c, cncfg=cn)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=5)
    x = synthetic.make_latents(cfg, [0, 1, 0, 1], L)
    cond = _cond(B, 8 * L, 24)
    pipe.engine.set_context(ctx)
    pipe.engine.controlnet_set_cond(cond, repeat=2)
    got = _split(pipe.engine.controlnet_residuals(x, 401.0, 0.9).cpu(), cfg, 2 * B, L)
    with torch.no_grad():
        down, mid = R.controlnet_forward(c, cfg.unet, x, torch.tensor(401.0), ctx, torch.cat([cond, cond]), 0.9, n_emb=4, bgr=True)
    errs = [_rms_rel(g_, w_) for g_, w_ in zip(got, down + [mid])]
    print(f"controlnet residuals, embedding (128, 192, 96, 320) bgr: rms rel max {max(errs):.4f}")
    report("controlnet_residuals[tiny,wide_bgr]", rms_rel_max=max(errs))
    assert max(errs) < 0.03, errs
    pipe.engine.close()


@pytest.mark.parametrize("name,L,B2,small", CASES)
def test_injected_unet_forward_matches_restatement(name, L, B2, small):
    """One UNet forward with a one-element schedule: the ControlNet's residuals in every skip and the mid output.  Stale GroupNorm
    statistics of an injected skip (the up path's concat norm) would show here."""
    from agenda_amd import config, synthetic
    cfg = config.CONFIGS[name]()
    u, v, c = _weights(cfg, small)
    pipe = _pipe(cfg, u, v, c, ws=(12 if L >= 64 else 6) << 30)
    ctx = synthetic.make_context(cfg, B2 // 2, seed=6)
    x = synthetic.make_latents(cfg, list(range(3, 3 + B2)), L)
    cond = _cond(B2, 8 * L, 22)
    t, scale = 301.0, 1.0
    pipe.engine.set_context(ctx)
    pipe.engine.controlnet_set_cond(cond, repeat=1)
    plain = pipe.engine.unet_forward(x, t).cpu()
    pipe.engine.controlnet_set_schedule([scale])
    got = pipe.engine.unet_forward(x, t).cpu()
    pipe.engine.controlnet_set_schedule([])
    with torch.no_grad():                                # one image at a time (the oracle's attention holds every score)
        want = torch.cat([R.controlled_eps(u, c, cfg.unet, x[i:i + 1], t, ctx[i:i + 1], cond[i:i + 1], scale) for i in range(B2)])
    e, moved = _rms_rel(got, want), _rms_rel(plain, want)
    print(f"injected unet {name} L={L}: rms rel {e:.4f} (the un-injected forward is {moved:.3f} away)")
    report(f"controlnet_injected_unet[{name},L={L}]", rms_rel=e)
    assert moved > 5 * e, (moved, e)                 # the residuals matter at this scale
    assert e < 0.03, e
    pipe.engine.close()


def test_cfg_shared_prefix_at_sd15_widths_matches_unshared_forwards():
    """SD-1.5 shapes at 256 px: the fused DDIM loop (the CFG halves share everything ahead of the first attn2, in the UNet and in the
    ControlNet, whose conv_in adds the embedding there; the C = 320 fused row-panel kernels duplicate the rows) against the same steps
    through unshared `unet_forward` calls of the CFG pair + `cfg_ddim_step`."""
    from agenda_amd import config, synthetic
    cfg = config.sd15()
    u, v, c = _weights(cfg, small=False)
    pipe = _pipe(cfg, u, v, c, ws=6 << 30)
    B, L, steps, g, scale = 1, 32, 3, 7.5, 0.9
    ctx = synthetic.make_context(cfg, B, seed=8)
    lat0 = synthetic.make_latents(cfg, [9], L)
    cond = _cond(B, 8 * L, 25)
    fused = pipe(prompt_embeds=ctx, image=cond, latents=lat0, num_inference_steps=steps, guidance_scale=g, height=8 * L, width=8 * L, output_type="latent",
                 controlnet_conditioning_scale=scale).latents.cpu()
    pipe.scheduler.set_timesteps(steps)
    a_t, a_p = pipe.scheduler.step_coeffs()
    pipe.engine.set_context(ctx)
    pipe.engine.controlnet_set_cond(cond, repeat=2)
    x = lat0.clone().cuda().contiguous()
    for i, t in enumerate(pipe.scheduler.timesteps):
        pipe.engine.controlnet_set_schedule([scale])
        eps = pipe.engine.unet_forward(torch.cat([x, x]).contiguous(), float(t))
        pipe.engine.cfg_ddim_step(eps, x, g, float(a_t[i]), float(a_p[i]))
    pipe.engine.controlnet_set_schedule([])
    e = _rms_rel(fused, x)
    print(f"controlnet fused (CFG-shared) vs unshared DDIM loop, SD-1.5 256 px: rms rel {e:.2e}")
    report("controlnet_cfg_shared_vs_unshared[sd15,256px]", latents_rms_rel=e)
    assert e < 1e-3, e
    pipe.engine.close()


def _run(name, scheduler, sched_key, start=0.0, scale=1.0, steps=6):
    from agenda_amd import config, synthetic, trace
    from oracle import sd_oracle as O
    cfg = config.CONFIGS[name]()
    u, v, c = _weights(cfg)
    pipe = _pipe(cfg, u, v, c, scheduler=scheduler)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    u8 = (_cond(B, 8 * L, 23) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    cond = u8.permute(0, 3, 1, 2).float() / 255.0
    rec = O.DaamRecorder(L * L, context_size=cfg.max_tokens)
    want_img, want_lat = R.generate(u, v, c, cfg, ctx, lat, cond, steps, sched_key, scale=scale, start=start, recorder=rec)
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, image=u8, latents=lat, num_inference_steps=steps, height=8 * L, width=8 * L, output_type="np",
                   control_guidance_start=start, controlnet_conditioning_scale=scale)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    whm = rec.compute_global_heat_map()
    pipe.engine.close()
    return out, hm, want_img, want_lat, whm


@pytest.mark.parametrize("scheduler,key,n_evals", [("DDIMScheduler", "ddim", 6), ("PNDMScheduler", "pndm", 7),
                                                   ("DPMSolverMultistepScheduler", "dpm", 6)])
def test_pipeline_matches_oracle(scheduler, key, n_evals):
    out, hm, want_img, want_lat, whm = _run("tiny", scheduler, key)
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(hm, whm)
    print(f"controlnet pipe {key}: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map rel {e_hm:.4f}")
    report(f"controlnet_pipeline[{key}]", latents_rms_rel=e_lat, psnr_db=psnr, heat_map_rel=e_hm)
    assert e_lat < 0.06, e_lat
    assert psnr > 30.0, psnr
    assert e_hm < 0.06, e_hm
    # the plain pipeline's recorded evaluation count: the ControlNet's cross-attention is not recorded
    assert float(hm.sum(1).mean()) == pytest.approx(n_evals, rel=0.02)


def test_guidance_start_matches_restatement():
    out, hm, want_img, want_lat, whm = _run("tiny", "DDIMScheduler", "ddim", start=0.4)
    e_lat, psnr = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img)
    print(f"controlnet start=0.4: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB")
    assert e_lat < 0.06 and psnr > 30.0, (e_lat, psnr)


@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_scale_zero_is_bit_identical_to_the_plain_pipeline(scheduler):
    from agenda_amd import StableDiffusionPipeline, config, synthetic, trace
    cfg = config.tiny()
    u, v, c = _weights(cfg)
    B, L, steps = 2, 16, 5
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    res = []
    for cn in (False, True):
        pipe = _pipe(cfg, u, v, c, scheduler=scheduler) if cn else StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30, scheduler=scheduler)
        kw = dict(image=_cond(1, 8 * L, 3), controlnet_conditioning_scale=0.0) if cn else {}
        with trace(pipe) as trc:
            out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="np", **kw)
            hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
        res.append((out.latents.cpu(), out.images, hm))
        pipe.engine.close()
    assert torch.equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])


def test_error_contract():
    from agenda_amd import _lib, config, synthetic
    from agenda_amd.controlnet import ControlNetModel, StableDiffusionControlNetPipeline
    cfg = config.tiny()
    u, v, c = _weights(cfg)
    pipe = _pipe(cfg, u, v, c)
    ctx = synthetic.make_context(cfg, 2, seed=1)
    lat = synthetic.make_latents(cfg, [0, 1], 16)
    kw = dict(prompt_embeds=ctx, latents=lat, num_inference_steps=2, output_type="latent")
    with pytest.raises(ValueError):
        pipe(image=_cond(2, 64, 1), **kw)                    # wrong size
    with pytest.raises(ValueError):
        pipe(image=_cond(3, 128, 1), **kw)                   # batch neither 1 nor the prompt batch
    with pytest.raises(NotImplementedError):
        pipe(image=_cond(1, 128, 1), guess_mode=True, **kw)
    with pytest.raises(NotImplementedError):
        pipe(image=_cond(1, 128, 1), controlnet_conditioning_scale=[1.0, 0.5], **kw)
    with pytest.raises(NotImplementedError):
        pipe.img2img(prompt_embeds=ctx, image=torch.rand(2, 3, 128, 128))
    m = ControlNetModel.from_config(cfg.unet, config.ControlNetConfig(), c)
    with pytest.raises(NotImplementedError):
        StableDiffusionControlNetPipeline(cfg, u, v, controlnet=[m, m])
    bad = ControlNetModel(dict(m.config, cross_attention_dim=128), c)
    with pytest.raises(ValueError):
        StableDiffusionControlNetPipeline(cfg, u, v, controlnet=bad)
    e = pipe.engine
    e.set_context(ctx)
    x = torch.cat([lat, lat]).cuda()
    fresh = _pipe(cfg, u, v, c)                              # no conditioning image ever set
    fresh.engine.set_context(ctx)
    fresh.engine.controlnet_set_schedule([1.0])
    with pytest.raises(_lib.AgendaHipError, match="conditioning image"):
        fresh.engine.unet_forward(x, 11.0)
    fresh.engine.close()
    e.controlnet_set_cond(_cond(2, 128, 1), repeat=1)
    e.controlnet_set_schedule([1.0, 1.0])
    with pytest.raises(_lib.AgendaHipError, match="schedule"):
        e.unet_forward(x, 11.0)                              # one evaluation, two scales
    e.controlnet_set_cond(_cond(2, 128, 1), repeat=2)
    e.controlnet_set_schedule([1.0] * 3)
    pipe.scheduler.set_timesteps(4)
    a_t, a_p = pipe.scheduler.step_coeffs()
    with pytest.raises(_lib.AgendaHipError, match="schedule"):
        e.denoise(lat.clone().cuda(), pipe.scheduler.timesteps, a_t, a_p, 7.5)
    e.controlnet_set_schedule([])
    e.close()


def test_checkpoint_round_trip_and_cli(tmp_path):
    from PIL import Image
    from _util import write_tiny_checkpoint
    from agenda_amd import StableDiffusionControlNetPipeline, config, synthetic
    from agenda_amd.controlnet import ControlNetModel
    from agenda_amd.generation import generate_batch
    cfg = config.tiny()
    u, v, c = _weights(cfg)
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, u, v, scheduler="DDIMScheduler")
    ControlNetModel.from_config(cfg.unet, config.ControlNetConfig(), c).save_pretrained(os.path.join(ck, "controlnet"))
    img_dir = tmp_path / "ctl"
    img_dir.mkdir()
    g = np.random.default_rng(0)
    for n in ("a.png", "b.png"):
        Image.fromarray(g.integers(0, 256, (96, 80, 3), dtype=np.uint8)).save(img_dir / n)
    pipe = StableDiffusionControlNetPipeline.from_pretrained(ck, controlnet=ControlNetModel.from_pretrained(os.path.join(ck, "controlnet")))
    out2 = str(tmp_path / "saved")
    pipe.save_pretrained(out2)
    with open(os.path.join(out2, "model_index.json")) as f:
        assert json.load(f)["controlnet"] == ["diffusers", "ControlNetModel"]
    pipe2 = StableDiffusionControlNetPipeline.from_pretrained(out2)      # found through model_index.json
    seeds = [0, 1, 2]
    files = sorted(str(img_dir / n) for n in os.listdir(img_dir))
    from agenda_amd.generation import control_images_for
    ctl = {"image": control_images_for(files, seeds), "controlnet_conditioning_scale": 0.7}
    imgs, hms = generate_batch(pipe2, seeds, ["cars"], prompt="an aerial view with cars", num_inference_steps=3, control=ctl)
    imgs, hms = imgs.cpu().numpy(), hms.cpu()
    pipe.engine.close(); pipe2.engine.close()
    save = tmp_path / "cli"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--pretrained-model-path", out2, "--controlnet-model-path", os.path.join(out2, "controlnet"),
           "--control-image", str(img_dir), "--controlnet-conditioning-scale", "0.7", "--save-dir", str(save), "--num-images", "3",
           "--batch-size", "3", "--num-inference-steps", "3", "--image-size", "128", "--word_token_heatmaps", "cars",
           "--prompt", "an aerial view with cars"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # the CLI writes the API's images and heat maps: the same files, byte for byte
    from agenda_amd.generation import save_outputs
    ref = tmp_path / "api"
    save_outputs(str(ref), seeds, torch.from_numpy(imgs), hms, ["cars"], 128)
    want = sorted(os.path.relpath(os.path.join(d, f), ref) for d, _, fs in os.walk(ref) for f in fs)
    got = sorted(os.path.relpath(os.path.join(d, f), save) for d, _, fs in os.walk(save) for f in fs)
    assert want and want == got, (want, got)
    for p in want:
        with open(ref / p, "rb") as fa, open(save / p, "rb") as fb:
            assert fa.read() == fb.read(), p
