"""Inpainting on the device: the mask front end against the host rule, the 9-channel and 4-channel (blend) loops under DDIM, PNDM and
DPM-Solver++ against the fp32 restatement (tests/_inpaint_restated.py) with DAAM on, the fused 9-channel loop against a host-stepped one,
exact preservation of the unmasked latents, state clearing, the checkpoint + CLI round trip and the error statuses."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _inpaint_restated as R
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


def _cfg(name, nine):
    from agenda_amd import config
    cfg = config.CONFIGS[name]()
    return config.inpaint_variant(cfg) if nine else cfg


def _weights(cfg, small=True):
    from agenda_amd import synthetic
    kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
    return synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw), synthetic.make_vae_weights(cfg, 12 if small else 1235, with_encoder=True, **kw)


def _pipe(cfg, u, v, scheduler="DDIMScheduler"):
    from agenda_amd import StableDiffusionInpaintPipeline
    return StableDiffusionInpaintPipeline(cfg, u, v, workspace_bytes=2 << 30, scheduler=scheduler)


def _inputs(B, S, seed):
    """A random image and a mask with a filled rectangle per image (values on both sides of 0.5 and 0.5 itself inside)."""
    g = np.random.default_rng(seed)
    img = torch.from_numpy(g.integers(0, 256, (B, S, S, 3), dtype=np.uint8))
    m = np.zeros((B, S, S), dtype=np.uint8)
    for b in range(B):
        y0, x0 = g.integers(0, S // 2, 2)
        m[b, y0:y0 + S // 2, x0:x0 + S // 3] = 255
    m[:, ::7, ::5] = g.integers(0, 256, m[:, ::7, ::5].shape, dtype=np.uint8)
    return img, torch.from_numpy(m)


def _draws(cfg, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    c = cfg.unet.out_channels
    return torch.randn(B, c, L, L, generator=g), torch.randn(B, c, L, L, generator=g), torch.randn(B, c, L, L, generator=g)


def _run(name, nine, scheduler, key, steps, L=16, strength=1.0, small=True):
    from agenda_amd import synthetic, trace
    from oracle import sd_oracle as O
    cfg = _cfg(name, nine)
    u, v = _weights(cfg, small)
    pipe = _pipe(cfg, u, v, scheduler)
    B, S = 2, 8 * L
    ctx = synthetic.make_context(cfg, B, seed=41)
    img, mask = _inputs(B, S, 5)
    ne, nz, me = _draws(cfg, B, L, 7)
    rec = O.DaamRecorder(L * L, context_size=cfg.max_tokens)
    want_img, want_lat, aux = R.generate(u, v, cfg, ctx, img, mask, steps, key, strength=strength, noise_enc_image=ne, noise=nz,
                                         noise_enc_masked=me, recorder=rec)
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, image=img, mask_image=mask, noise_enc_image=ne, noise=nz, noise_enc_masked=me, strength=strength,
                   num_inference_steps=steps, height=S, width=S, output_type="np")
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    whm = rec.compute_global_heat_map()
    got_aux = dict(pipe._inpaint_inputs)
    pipe.engine.close()
    return out, hm, want_img, want_lat, whm, aux, got_aux


def test_front_end_matches_host_rule():
    from agenda_amd import config
    cfg = config.tiny()
    u, v = _weights(cfg)
    pipe = _pipe(cfg, u, v)
    B, S = 3, 64
    img, mask = _inputs(B, S, 3)
    mask[0, :8, :8] = 127
    mask[0, 8:16, :8] = 128
    want_img, want_m = R.preprocess_image(img), R.preprocess_mask(mask)
    want_masked, want_lat = R.masked_image(want_img, want_m), R.latent_mask(want_m, S // 8)
    x, m = pipe.engine.inpaint_prepare(img, mask, True, True)
    x, m = x.cpu(), m.cpu()
    e_img = float((x[:B] - want_img).abs().max())
    report("inpaint_front_end[u8]", image_max_abs=e_img)
    assert e_img <= 1e-6, e_img
    assert torch.equal(m, want_lat)
    assert torch.equal(x[B:], R.masked_image(x[:B], want_m))
    assert torch.equal(x[B:] == 0, want_masked == 0)
    # float mask in [0,1], 0.5 itself goes to 1; a float [-1,1] image is taken as it is
    fm = mask.float() / 255.0
    fm[1, 0:8, 0:8] = 0.5
    fimg = want_img.clone()
    x2, m2 = pipe.engine.inpaint_prepare(fimg, fm, False, True)
    wm2 = R.preprocess_mask(fm)
    assert torch.equal(m2.cpu(), R.latent_mask(wm2, S // 8))
    assert torch.equal(x2.cpu(), R.masked_image(fimg, wm2))
    assert float(m2.cpu()[1, 0, 0, 0]) == 1.0
    pipe.engine.close()


CASES_9 = [("tiny", "DDIMScheduler", "ddim", 6, 16, True), ("tiny", "PNDMScheduler", "pndm", 6, 16, True),
           ("tiny", "DPMSolverMultistepScheduler", "dpm", 6, 16, True), ("sd15", "DDIMScheduler", "ddim", 3, 32, False)]


@pytest.mark.parametrize("name,scheduler,key,steps,L,small", CASES_9)
def test_nine_channel_loop_matches_restatement(name, scheduler, key, steps, L, small):
    out, hm, want_img, want_lat, whm, aux, got = _run(name, True, scheduler, key, steps, L=L, small=small)
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(hm, whm)
    e_ml = _rms_rel(got["masked_image_latents"], aux["masked_image_latents"])
    print(f"inpaint 9ch {name} {key}: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map rel {e_hm:.4f}, masked latents {e_ml:.4f}")
    report(f"inpaint9[{name},{key},L={L}]", latents_rms_rel=e_lat, psnr_db=psnr, heat_map_rel=e_hm, masked_latents_rms_rel=e_ml)
    assert torch.equal(got["mask"].cpu(), aux["mask"])
    assert e_ml < 0.03, e_ml
    assert e_lat < 0.06, e_lat
    assert psnr > 30.0, psnr
    assert e_hm < 0.06, e_hm


@pytest.mark.parametrize("scheduler,key,strength", [("DDIMScheduler", "ddim", 1.0), ("PNDMScheduler", "pndm", 1.0),
                                                    ("DPMSolverMultistepScheduler", "dpm", 1.0), ("DDIMScheduler", "ddim", 0.6)])
def test_blend_loop_matches_restatement(scheduler, key, strength):
    out, hm, want_img, want_lat, whm, aux, got = _run("tiny", False, scheduler, key, 6, strength=strength)
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(hm, whm)
    print(f"inpaint blend {key} strength {strength}: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map rel {e_hm:.4f}")
    report(f"inpaint_blend[{key},strength={strength}]", latents_rms_rel=e_lat, psnr_db=psnr, heat_map_rel=e_hm)
    assert e_lat < 0.06, e_lat
    assert psnr > 30.0, psnr
    assert e_hm < 0.06, e_hm


@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_blend_preserves_unmasked_latents_exactly(scheduler):
    from agenda_amd import synthetic
    cfg = _cfg("tiny", False)
    u, v = _weights(cfg)
    pipe = _pipe(cfg, u, v, scheduler)
    B, L = 2, 16
    img, mask = _inputs(B, 8 * L, 9)
    out = pipe(prompt_embeds=synthetic.make_context(cfg, B, seed=3), image=img, mask_image=mask, generator=torch.Generator().manual_seed(4),
               num_inference_steps=5, height=8 * L, width=8 * L, output_type="latent")
    got = pipe._inpaint_inputs
    keep = (got["mask"] == 0).expand_as(out.latents)
    assert 0 < int(keep.sum()) < keep.numel()
    assert torch.equal(out.latents[keep], got["image_latents"][keep])
    assert not torch.equal(out.latents[~keep], got["image_latents"][~keep])
    pipe.engine.close()


def test_nine_channel_fused_loop_matches_host_stepped_loop():
    from agenda_amd import synthetic
    cfg = _cfg("tiny", True)
    u, v = _weights(cfg)
    pipe = _pipe(cfg, u, v)
    B, L, steps = 2, 16, 5
    ctx = synthetic.make_context(cfg, B, seed=8)
    img, mask = _inputs(B, 8 * L, 6)
    gen = lambda: torch.Generator().manual_seed(12)
    out = pipe(prompt_embeds=ctx, image=img, mask_image=mask, generator=gen(), num_inference_steps=steps, height=8 * L, width=8 * L,
               output_type="latent")
    got = pipe._inpaint_inputs
    x = got["noise"].clone()
    m2, ml2 = torch.cat([got["mask"]] * 2), torch.cat([got["masked_image_latents"]] * 2)
    ts = pipe.scheduler.set_timesteps(steps)
    a_t, a_p = pipe.scheduler.step_coeffs()
    for i, t in enumerate(ts):
        eps = pipe.unet(torch.cat([torch.cat([x, x]), m2, ml2], 1), float(t), encoder_hidden_states=ctx).sample
        pipe.engine.cfg_ddim_step(eps, x, 7.5, a_t[i], a_p[i])
    e = _rms_rel(out.latents, x)
    report("inpaint9_fused_vs_host_stepped[tiny]", latents_rms_rel=e)
    assert e < 1e-3, e
    pipe.engine.close()


@pytest.mark.parametrize("nine", [False, True])
def test_state_is_cleared_after_an_inpaint_call(nine):
    from agenda_amd import StableDiffusionPipeline, synthetic
    cfg = _cfg("tiny", False)
    u, v = _weights(cfg)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=2)
    lat = synthetic.make_latents(cfg, [5, 6], L)
    fresh = StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30)
    want = fresh(prompt_embeds=ctx, latents=lat, num_inference_steps=4, output_type="latent").latents.cpu()
    fresh.engine.close()
    pipe = _pipe(cfg, u, v)
    img, mask = _inputs(B, 8 * L, 1)
    pipe(prompt_embeds=ctx, image=img, mask_image=mask, generator=torch.Generator().manual_seed(0), num_inference_steps=4, output_type="latent",
         height=8 * L, width=8 * L)
    got = StableDiffusionPipeline.__call__(pipe, prompt_embeds=ctx, latents=lat, num_inference_steps=4, output_type="latent").latents.cpu()
    assert torch.equal(got, want)
    pipe.engine.close()
    if nine:                       # a 9-channel UNet refuses txt2img and, without the state, the device loop refuses it too
        cfg9 = _cfg("tiny", True)
        u9, v9 = _weights(cfg9)
        p9 = _pipe(cfg9, u9, v9)
        with pytest.raises(ValueError, match="StableDiffusionInpaintPipeline"):
            StableDiffusionPipeline.__call__(p9, prompt_embeds=ctx, latents=lat, num_inference_steps=2)
        p9.engine.set_context(ctx)
        x = lat.cuda().contiguous()
        with pytest.raises(Exception, match="agd_inpaint_set"):
            p9.engine.denoise(x, [1], [0.5], [0.6], 7.5)
        p9.engine.close()


def test_error_statuses():
    from agenda_amd import StableDiffusionControlNetPipeline, synthetic
    from agenda_amd._lib import AgendaHipError
    cfg = _cfg("tiny", False)
    u, v = _weights(cfg)
    pipe = StableDiffusionControlNetPipeline.from_synthetic("tiny", seed=5, workspace_bytes=2 << 30)
    eng, lib = pipe.engine, pipe.engine.lib
    B, L = 2, 16
    eng.set_context(synthetic.make_context(cfg, B, seed=1))
    m = torch.zeros(B, 1, L, L, device="cuda")
    z = torch.zeros(B, 4, L, L, device="cuda")
    x = torch.zeros(B, 4, L, L, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    assert lib.agd_inpaint_set(eng.ctx, P(m), 1, P(z), 4, None, B, L, None) != 0             # the blend needs the noise
    assert lib.agd_inpaint_set(eng.ctx, P(m), 2, P(z), 4, P(z), B, L, None) != 0             # 2 mask channels
    assert lib.agd_inpaint_set_schedule(eng.ctx, (C.c_float * 2)(1, 0), 1) != 0              # no blend state yet
    eng.inpaint_set(m, z, z)
    eng.inpaint_set_schedule([(1.0, 0.0)] * 3)
    with pytest.raises(AgendaHipError, match="blend schedule"):                               # 3 entries, 2 evaluations
        eng.denoise(x, [500, 1], [0.5, 0.9], [0.9, 0.99], 7.5)
    eng.inpaint_set_schedule([(1.0, 0.0)] * 2)
    with pytest.raises(AgendaHipError, match="latent side"):                                  # side mismatch
        eng.denoise(torch.zeros(B, 4, 8, 8, device="cuda"), [500, 1], [0.5, 0.9], [0.9, 0.99], 7.5)
    eng.set_context(synthetic.make_context(cfg, 1, seed=1))
    with pytest.raises(AgendaHipError, match="holds 2 images"):                               # batch mismatch
        eng.denoise(torch.zeros(1, 4, L, L, device="cuda"), [500, 1], [0.5, 0.9], [0.9, 0.99], 7.5)
    eng.set_context(synthetic.make_context(cfg, B, seed=1))
    eng.controlnet_set_schedule([0.0, 0.0])
    with pytest.raises(AgendaHipError, match="ControlNet"):
        eng.denoise(x, [500, 1], [0.5, 0.9], [0.9, 0.99], 7.5)
    eng.controlnet_set_schedule([])
    eng.denoise(x, [500, 1], [0.5, 0.9], [0.9, 0.99], 7.5)
    torch.cuda.synchronize()
    eng.inpaint_clear()
    assert lib.agd_inpaint_prepare(eng.ctx, None, 0, P(m), 0, B, 64, None, None, None, None) != 0
    img8 = torch.zeros(B, 60, 60, 3, dtype=torch.uint8, device="cuda")
    m8 = torch.zeros(B, 60, 60, dtype=torch.uint8, device="cuda")
    assert lib.agd_inpaint_prepare(eng.ctx, P(img8), 0, P(m8), 0, B, 60, None, None, None, None) != 0   # side not a multiple of 8
    pipe.engine.close()
    # a 9-channel UNet: the channel counts must add up
    cfg9 = _cfg("tiny", True)
    u9, v9 = _weights(cfg9)
    p9 = _pipe(cfg9, u9, v9)
    z3 = torch.zeros(B, 3, L, L, device="cuda")
    assert p9.engine.lib.agd_inpaint_set(p9.engine.ctx, P(m), 1, P(z3), 3, None, B, L, None) != 0
    assert p9.engine.lib.agd_inpaint_set(p9.engine.ctx, P(m), 1, P(z), 4, P(z), B, L, None) != 0   # no noise for a concatenating UNet
    p9.engine.inpaint_set(m, z)
    p9.engine.close()


@pytest.mark.parametrize("nine", [True, False])
def test_checkpoint_round_trip_and_cli(tmp_path, nine):
    from PIL import Image
    from _util import write_tiny_checkpoint
    from agenda_amd import StableDiffusionInpaintPipeline
    from agenda_amd.generation import generate_batch, inpaint_inputs_for, save_outputs
    cfg = _cfg("tiny", nine)
    u, v = _weights(cfg)
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, u, v, scheduler="DDIMScheduler")
    uc = os.path.join(ck, "unet", "config.json")
    with open(uc) as f:
        j = json.load(f)
    j["in_channels"] = cfg.unet.in_channels
    with open(uc, "w") as f:
        json.dump(j, f)
    d_img, d_msk = tmp_path / "img", tmp_path / "msk"
    d_img.mkdir(); d_msk.mkdir()
    g = np.random.default_rng(0)
    for n in ("a.png", "b.png"):
        Image.fromarray(g.integers(0, 256, (128, 128, 3), dtype=np.uint8)).save(d_img / n)
        mk = np.zeros((128, 128), dtype=np.uint8); mk[20:90, 30:100] = 255
        Image.fromarray(mk).save(d_msk / n)
    pipe = StableDiffusionInpaintPipeline.from_pretrained(ck)
    assert pipe.cfg.unet.in_channels == cfg.unet.in_channels
    out2 = str(tmp_path / "saved")
    pipe.save_pretrained(out2)
    with open(os.path.join(out2, "model_index.json")) as f:
        assert json.load(f)["_class_name"] == "StableDiffusionInpaintPipeline"
    pipe2 = StableDiffusionInpaintPipeline.from_pretrained(out2)
    seeds = [0, 1, 2]
    pairs = list(zip(sorted(str(d_img / n) for n in os.listdir(d_img)), sorted(str(d_msk / n) for n in os.listdir(d_msk))))
    a = generate_batch(pipe, seeds, ["cars"], prompt="an aerial view with cars", num_inference_steps=3, control=inpaint_inputs_for(pairs, seeds, 1.0))
    imgs, hms = generate_batch(pipe2, seeds, ["cars"], prompt="an aerial view with cars", num_inference_steps=3,
                               control=inpaint_inputs_for(pairs, seeds, 1.0))
    assert torch.equal(a[0], imgs)                             # the reloaded checkpoint paints the same images
    imgs, hms = imgs.cpu().numpy(), hms.cpu()
    pipe.engine.close(); pipe2.engine.close()
    save = tmp_path / "cli"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--pretrained-model-path", out2, "--init-image", str(d_img), "--mask-image", str(d_msk),
           "--save-dir", str(save), "--num-images", "3", "--batch-size", "3", "--num-inference-steps", "3", "--image-size", "128",
           "--word_token_heatmaps", "cars", "--prompt", "an aerial view with cars"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    ref = tmp_path / "api"
    save_outputs(str(ref), seeds, torch.from_numpy(imgs), hms, ["cars"], 128)
    want = sorted(os.path.relpath(os.path.join(d, f), ref) for d, _, fs in os.walk(ref) for f in fs)
    got = sorted(os.path.relpath(os.path.join(d, f), save) for d, _, fs in os.walk(save) for f in fs)
    assert want and want == got, (want, got)
    for p in want:
        with open(ref / p, "rb") as fa, open(save / p, "rb") as fb:
            assert fa.read() == fb.read(), p
