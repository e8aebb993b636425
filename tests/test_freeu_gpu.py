"""FreeU on the device: the one-launch kernel through its op seam and one re-weighted UNet forward against the fp32 restatement
(tests/_freeu_restated.py, whose filter is torch.fft), both forms of the GroupNorm hand-over, the off switch bit for bit, `enable_freeu`
end to end under DDIM, PNDM and DPM-Solver++ with DAAM on, FreeU beside a ControlNet, a LoRA, a rectangular call, InstructPix2Pix and the
panorama loop, and the error contract."""
import math

import numpy as np
import pytest
import torch

import _freeu_restated as R
from _report import report

pytestmark = pytest.mark.gpu
REL = 2.0 ** -7                      # tests/test_ops_gpu.py: a bf16-output seam against fp32, relative to the largest value
SD15 = (0.9, 0.2, 1.5, 1.6)          # diffusers' suggestion for SD-1.5


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
    """(cfg, unet, vae) of a config, drawn once per session: the tiny configs as tests/test_freeu_cpu.py draws them."""
    if name not in _W:
        from agenda_amd import config, synthetic
        cfg = config.CONFIGS[name]()
        small = name != "sd15"
        kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
        _W[name] = (cfg, synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw), synthetic.make_vae_weights(cfg, 12 if small else 1235, **kw))
    return _W[name]


def _pipe(name="tiny", scheduler="DDIMScheduler", ws=2 << 30):
    from agenda_amd import StableDiffusionPipeline
    cfg, u, v = _weights(name)
    return StableDiffusionPipeline(cfg, u, v, workspace_bytes=ws, scheduler=scheduler)


# ---- 1. the op seam -------------------------------------------------------------------------------------------------------------
# 1 x 1 and 1 x 2: a side of 1 has frequency 0 only; 2 x 2, 2 x 3: -1 = +1 mod 2; 3 x 3, 9 x 8: odd sides; 8 x 8, 16 x 16: one and four
# 64-pixel statistics tiles (the partial sums are written); 24 x 24: nine tiles.  128 / 320 / 640 / 1280 channels: 16, 40, 80 and 160
# vectors of 8 -- every vectors-per-workgroup choice but 1 and 2 -- with 1280 / 640 more than one workgroup per image.
OP_SIZES = [(1, 1), (1, 2), (2, 2), (3, 3), (2, 3), (8, 8), (9, 8), (16, 16), (24, 24)]
OP_CHANNELS = [(128, 128), (1280, 640), (320, 320)]
OP_PARAMS = [(1.5, 0.9), (1.6, 0.2), (1.0, 0.2), (1.6, 1.0)]


@pytest.mark.parametrize("Ch,Cs", OP_CHANNELS, ids=lambda v: str(v))
@pytest.mark.parametrize("H,W", OP_SIZES, ids=lambda v: str(v))
def test_op_seam_matches_restatement(H, W, Ch, Cs):
    from agenda_amd import ops
    B = 2
    g = torch.Generator().manual_seed(1000 * H + 10 * W + Ch)
    hid = torch.randn(B, Ch, H, W, generator=g).to(torch.bfloat16).float()
    # a skip with a mean and a slope, so the four low frequencies carry weight
    skip = (torch.randn(B, Cs, H, W, generator=g) + torch.randn(B, Cs, 1, 1, generator=g) +
            torch.linspace(-1, 1, H * W).view(1, 1, H, W) * torch.randn(B, Cs, 1, 1, generator=g)).to(torch.bfloat16).float()
    worst = 0.0
    for b, s in OP_PARAMS:
        ho, so = (t.cpu() for t in ops.freeu(hid.cuda(), skip.cuda(), b, s))
        ho2, so2 = (t.cpu() for t in ops.freeu(hid.cuda(), skip.cuda(), b, s))
        assert torch.equal(ho, ho2) and torch.equal(so, so2), "two runs differ"
        n = Ch // 2
        want_h = torch.cat([hid[:, :n] * b, hid[:, n:]], 1)
        want_s = R.fourier_filter(skip, 1, s)
        assert torch.equal(ho[:, n:], hid[:, n:]), "unscaled backbone channels changed"
        if b == 1.0:
            assert torch.equal(ho, hid)
        if s == 1.0:
            assert torch.equal(so, skip)
        e_h, e_s = _rel(ho, want_h), _rel(so, want_s)
        worst = max(worst, e_h, e_s)
        assert e_h < REL and e_s < REL, (b, s, e_h, e_s)
    print(f"freeu op {H}x{W} Ch={Ch} Cs={Cs}: max rel {worst:.2e}")
    report(f"freeu_op[{H}x{W},Ch={Ch},Cs={Cs}]", max_rel=worst)


# ---- 2. one UNet forward --------------------------------------------------------------------------------------------------------
# config, latent height, latent width.  FreeU launches once per resnet of up blocks 0 and 1 (both tensors in one launch): 6 at
# layers_per_block 2, 4 at tiny40's 1.  A launch leaves GroupNorm partial sums where its map holds whole 64-pixel tiles:
#   tiny 16 x 16: up blocks 0 / 1 run at 2 x 2 / 4 x 4 (4 / 16 pixels) -> (0, 6);  tiny21 24 x 24: 3 x 3 / 6 x 6 -> (0, 6);
#   tiny 16 x 24: 2 x 3 / 4 x 6 -> (0, 6);  tiny40 16 x 16 (two levels): 8 x 8 / 16 x 16 (64 / 256) -> (4, 0);
#   sd15 32 x 32: 4 x 4 / 8 x 8 (16 / 64) -> (3, 3)
FWD_CASES = [("tiny", 16, 16), ("tiny21", 24, 24), ("tiny", 16, 24), ("tiny40", 16, 16), ("sd15", 32, 32)]
_COUNTS = {("tiny", 16, 16): (0, 6), ("tiny21", 24, 24): (0, 6), ("tiny", 16, 24): (0, 6), ("tiny40", 16, 16): (4, 0), ("sd15", 32, 32): (3, 3)}


def _forward_inputs(cfg, Lh, Lw):
    from agenda_amd import synthetic
    ctx = synthetic.make_context(cfg, 1, seed=6)
    x = torch.randn(2, 4, Lh, Lw, generator=torch.Generator().manual_seed(3))
    return ctx, x, 301.0


def _restated_forward(u, cfg, x, t, ctx, params):
    with torch.no_grad():                                # one image at a time (the oracle's attention holds every score)
        return torch.cat([R.unet_forward_with_freeu(u, cfg.unet, x[i:i + 1], torch.tensor(t), ctx[i:i + 1], *params) for i in range(x.shape[0])])


def _delta(a, b):
    return tuple(y - x for x, y in zip(a, b))


@pytest.mark.parametrize("name,Lh,Lw", FWD_CASES, ids=lambda v: str(v))
def test_unet_forward_matches_restatement(name, Lh, Lw):
    """Two rows, t = 301, the suggested SD-1.5 values.  Stale GroupNorm statistics of a re-weighted tensor (the concat norm reads both
    operands' partial sums) would show here.  Both hand-overs run: with the partial sums where the maps allow them and, with
    gn_fused_stats off, without any."""
    cfg, u, v = _weights(name)
    pipe = _pipe(name, ws=(6 if name == "sd15" else 2) << 30)
    e = pipe.engine
    ctx, x, t = _forward_inputs(cfg, Lh, Lw)
    e.set_context(ctx)
    plain = e.unet_forward(x, t).cpu()
    c0 = e.freeu_counts()
    e.freeu_set(*SD15)
    got = e.unet_forward(x, t).cpu()
    c1 = e.freeu_counts()
    again = e.unet_forward(x, t).cpu()
    c2 = e.freeu_counts()
    e.set_option("gn_fused_stats", 0)                    # no partial sums anywhere: every launch takes the cpart_bm = 0 form
    got_fb = e.unet_forward(x, t).cpu()
    c3 = e.freeu_counts()
    e.set_option("gn_fused_stats", 1)
    e.freeu_clear()
    off = e.unet_forward(x, t).cpu()
    c4 = e.freeu_counts()
    e.close()
    want = _restated_forward(u, cfg, x, t, ctx, SD15)
    err, err_fb, both, moved = _rms_rel(got, want), _rms_rel(got_fb, want), _rms_rel(got_fb, got), _rms_rel(plain, want)
    print(f"freeu unet {name} {Lh}x{Lw}: rms rel {err:.4f} (statistics pass: {err_fb:.4f}, the two {both:.4f} apart; the plain forward is {moved:.3f} away); "
          f"launches with / without partial sums {_delta(c0, c1)}")
    report(f"freeu_unet[{name},{Lh}x{Lw}]", rms_rel=err, rms_rel_stats_pass=err_fb)
    assert c0 == (0, 0)
    assert _delta(c0, c1) == _COUNTS[(name, Lh, Lw)] == _delta(c1, c2)
    assert _delta(c2, c3) == (0, sum(_COUNTS[(name, Lh, Lw)]))
    assert c4 == c3 and torch.equal(off, plain)           # cleared: the plain UNet again, bit for bit, and nothing launched
    assert torch.equal(again, got)
    assert err < 0.03, err
    assert err_fb < 0.03 and both < 0.03, (err_fb, both)


@pytest.mark.parametrize("params", [(0.9, 0.2, 1.0, 1.0), (1.0, 1.0, 1.5, 1.6)], ids=["filter-only", "backbone-only"])
def test_unet_forward_with_one_half_of_freeu(params):
    """s = 1 / b = 1 skip that tensor (its Act and partial sums stay the producer's); the launch count stays one per resnet."""
    cfg, u, v = _weights("tiny")
    pipe = _pipe("tiny")
    e = pipe.engine
    ctx, x, t = _forward_inputs(cfg, 16, 16)
    e.set_context(ctx)
    e.freeu_set(*params)
    got = e.unet_forward(x, t).cpu()
    counts = e.freeu_counts()
    e.close()
    err = _rms_rel(got, _restated_forward(u, cfg, x, t, ctx, params))
    print(f"freeu unet tiny 16x16 {params}: rms rel {err:.4f}")
    report(f"freeu_unet_half[{params}]", rms_rel=err)
    assert counts == (0, 6)
    assert err < 0.03, err


# ---- 3. the off switch ----------------------------------------------------------------------------------------------------------
def _call(pipe, ctx, lat, steps, **kw):
    from agenda_amd import trace
    B = lat.shape[0]
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="np", **kw)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    return out.latents.cpu(), out.images, hm


@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_disabled_freeu_is_bit_identical_to_the_plain_engine(scheduler):
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    cx, x, t = _forward_inputs(cfg, L, L)
    plain_pipe = _pipe("tiny", scheduler)                # never saw FreeU
    plain = _call(plain_pipe, ctx, lat, steps)
    plain_pipe.engine.set_context(cx)
    plain_fwd = plain_pipe.engine.unet_forward(x, t).cpu()
    plain_pipe.engine.close()
    pipe = _pipe("tiny", scheduler)
    pipe.enable_freeu(*SD15)
    on = _call(pipe, ctx, lat, steps)
    assert not torch.equal(on[0], plain[0])              # (it was on)
    c_on = pipe.engine.freeu_counts()
    assert sum(c_on) > 0
    for how in ("disable", "ones"):
        if how == "disable":
            pipe.disable_freeu()
        else:
            pipe.enable_freeu(1, 1, 1, 1)
        res = _call(pipe, ctx, lat, steps)
        assert torch.equal(res[0], plain[0]) and np.array_equal(res[1], plain[1]) and torch.equal(res[2], plain[2]), how
        pipe.engine.set_context(cx)
        assert torch.equal(pipe.engine.unet_forward(x, t).cpu(), plain_fwd), how
        assert pipe.engine.freeu_counts() == c_on, how
    pipe.engine.close()


# ---- 4. the pipeline ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheduler,key,n_evals", [("DDIMScheduler", "ddim", 6), ("PNDMScheduler", "pndm", 7), ("DPMSolverMultistepScheduler", "dpm", 6)])
def test_pipeline_matches_restatement(scheduler, key, n_evals):
    """enable_freeu against the restated loop, and in the same run the plain pipeline against the plain restated loop (all four
    parameters 1: the oracle's forward bit for bit, tests/test_freeu_cpu.py) for the same seeds.  FreeU's errors may be at most twice the
    plain ones: the largest b, 1.6, scales the bf16 rounding error of half the backbone by at most that.  For the PSNR a factor 2 in
    the error is 20 log10(2) = 6.02 dB.  And they stay inside tests/test_adapter_gpu.py's pipeline bounds: 0.06, 30 dB, 0.06."""
    from agenda_amd import synthetic
    from oracle import sd_oracle as O
    cfg, u, v = _weights("tiny")
    B, L, steps = 2, 16, 6
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    fig = {}
    for tag, params in (("plain", (1.0, 1.0, 1.0, 1.0)), ("freeu", SD15)):
        rec = O.DaamRecorder(L * L, context_size=cfg.max_tokens)
        want_img, want_lat = R.generate(u, v, cfg, ctx, lat, steps, key, *params, recorder=rec)
        whm = rec.compute_global_heat_map()
        pipe = _pipe("tiny", scheduler)
        if tag == "freeu":
            pipe.enable_freeu(*params)
        got_lat, got_img, hm = _call(pipe, ctx, lat, steps)
        pipe.engine.close()
        fig[tag] = (_rms_rel(got_lat, want_lat), _psnr(got_img, want_img), _rms_rel(hm, whm))
        assert float(hm.sum(1).mean()) == pytest.approx(n_evals, rel=0.02)      # FreeU adds no model evaluation
    (pl, pp, ph), (fl, fp, fh) = fig["plain"], fig["freeu"]
    print(f"freeu pipe {key}: latents rms rel {fl:.4f} (plain {pl:.4f}), PSNR {fp:.1f} dB (plain {pp:.1f}), heat map rms rel {fh:.4f} (plain {ph:.4f})")
    report(f"freeu_pipeline[{key}]", latents_rms_rel=fl, psnr_db=fp, heat_map_rms_rel=fh, plain_latents_rms_rel=pl, plain_psnr_db=pp,
           plain_heat_map_rms_rel=ph)
    assert fl <= 2 * pl, (fl, pl)
    assert fp >= pp - 20 * math.log10(2), (fp, pp)
    assert fh <= 2 * ph, (fh, ph)
    assert fl < 0.06 and fp > 30.0 and fh < 0.06, (fl, fp, fh)


# ---- 5. beside other code -------------------------------------------------------------------------------------------------------
def test_freeu_beside_a_controlnet():
    """The filtered skip is the injected one: the restated ControlNet's residuals go into the restated FreeU walk."""
    import _controlnet_restated as CR
    from agenda_amd import StableDiffusionControlNetPipeline, synthetic
    from agenda_amd.config import ControlNetConfig
    from agenda_amd.controlnet import ControlNetModel
    cfg, u, v = _weights("tiny")
    c = synthetic.make_controlnet_weights(cfg, seed=13, bias_std=0.05, perturb_norm=0.1)
    B, L, steps = 2, 16, 3
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    u8 = (torch.rand(B, 3, 8 * L, 8 * L, generator=torch.Generator().manual_seed(23)) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    cond = u8.permute(0, 3, 1, 2).float() / 255.0
    cond2 = torch.cat([cond, cond])

    def eps_fn(x2, t, ctx_, rec, params=SD15):
        down, mid = CR.controlnet_forward(c, cfg.unet, x2, t, ctx_, cond2, 1.0)
        return R.unet_forward_with_freeu(u, cfg.unet, x2, t, ctx_, *params, recorder=rec, down_residuals=down, mid_residual=mid)

    _, want = R.generate(u, v, cfg, ctx, lat, steps, "ddim", *SD15, eps_fn=eps_fn)
    _, want_off = R.generate(u, v, cfg, ctx, lat, steps, "ddim", *SD15, eps_fn=lambda *a: eps_fn(*a, params=(1.0, 1.0, 1.0, 1.0)))
    pipe = StableDiffusionControlNetPipeline(cfg, u, v, controlnet=ControlNetModel.from_config(cfg.unet, ControlNetConfig(), c), workspace_bytes=2 << 30)
    pipe.enable_freeu(*SD15)
    got = pipe(prompt_embeds=ctx, image=u8, latents=lat, num_inference_steps=steps, height=8 * L, width=8 * L, output_type="latent").latents.cpu()
    pipe.engine.close()
    err, moved = _rms_rel(got, want), _rms_rel(want_off, want)
    print(f"freeu + controlnet ddim x {steps}: latents rms rel {err:.4f} (without FreeU the restatement is {moved:.3f} away)")
    report("freeu_controlnet[ddim]", latents_rms_rel=err)
    assert err < 0.06, err
    assert moved > 2 * err, (moved, err)             # (a FreeU that missed the injected skips would sit near `moved`)


def test_freeu_beside_a_lora():
    """A LoRA on the UNet's attention projections, merged on the device, against the restated loop on host-merged fp32 weights; the FreeU
    state survives the load and the scale change."""
    from agenda_amd import lora, synthetic
    cfg, u, v = _weights("tiny")
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
    _, want = R.generate(um, v, cfg, ctx, lat, steps, "ddim", *SD15)
    _, want_base = R.generate(u, v, cfg, ctx, lat, steps, "ddim", *SD15)
    pipe = _pipe("tiny")
    pipe.enable_freeu(*SD15)
    pipe.load_lora_weights(sd)
    got = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", cross_attention_kwargs={"scale": 0.8}).latents.cpu()
    assert pipe.unet.freeu == SD15
    pipe.engine.close()
    err, moved = _rms_rel(got, want), _rms_rel(want_base, want)
    print(f"freeu + lora ddim x {steps}: latents rms rel {err:.4f} (without the LoRA the restatement is {moved:.3f} away)")
    report("freeu_lora[ddim]", latents_rms_rel=err)
    assert err < 0.06, err


def test_freeu_on_a_rectangular_call():
    from agenda_amd import synthetic
    cfg, u, v = _weights("tiny")
    B, Lh, Lw, steps = 2, 16, 24, 3
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = torch.randn(B, 4, Lh, Lw, generator=torch.Generator().manual_seed(8))
    _, want = R.generate(u, v, cfg, ctx, lat, steps, "ddim", *SD15)
    pipe = _pipe("tiny")
    pipe.enable_freeu(*SD15)
    got = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, height=8 * Lh, width=8 * Lw, output_type="latent").latents.cpu()
    pipe.engine.close()
    err = _rms_rel(got, want)
    print(f"freeu 128 x 192 ddim x {steps}: latents rms rel {err:.4f}")
    report("freeu_rect[128x192,ddim]", latents_rms_rel=err)
    assert err < 0.06, err


def _smoke(run, pipe):
    off = run()
    pipe.enable_freeu(*SD15)
    on1, on2 = run(), run()
    pipe.disable_freeu()
    off2 = run()
    pipe.engine.close()
    assert torch.isfinite(on1).all()
    assert torch.equal(on1, on2), "two runs differ"
    assert not torch.equal(on1, off)
    assert torch.equal(off, off2)


def test_freeu_in_the_instructpix2pix_loop():
    from agenda_amd import StableDiffusionInstructPix2PixPipeline, config, synthetic
    cfg = config.ip2p_variant(config.tiny())
    u = synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)
    v = synthetic.make_vae_weights(cfg, 12, with_encoder=True, bias_std=0.05, perturb_norm=0.1)
    pipe = StableDiffusionInstructPix2PixPipeline(cfg, u, v, workspace_bytes=2 << 30)
    B, L = 2, 16
    ctx = synthetic.make_context(cfg, B, seed=41)
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (B, 8 * L, 8 * L, 3), dtype=np.uint8))
    nz = torch.randn(B, cfg.unet.out_channels, L, L, generator=torch.Generator().manual_seed(7))
    _smoke(lambda: pipe(prompt_embeds=ctx, image=img, latents=nz, num_inference_steps=3, guidance_scale=7.5, image_guidance_scale=1.5,
                        output_type="latent").latents.cpu(), pipe)


def test_freeu_in_the_panorama_loop():
    from agenda_amd import StableDiffusionPanoramaPipeline, synthetic
    cfg, u, v = _weights("tiny")
    pipe = StableDiffusionPanoramaPipeline(cfg, u, v, workspace_bytes=2 << 30)
    B, lh, lw = 1, 16, 32
    ctx = synthetic.make_context(cfg, B, seed=21)
    lat = torch.randn(B, 4, lh, lw, generator=torch.Generator().manual_seed(7))
    _smoke(lambda: pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=3, height=8 * lh, width=8 * lw, output_type="latent").latents.cpu(), pipe)


# ---- 6. the error contract ------------------------------------------------------------------------------------------------------
def test_error_contract():
    from agenda_amd import StableDiffusionPipeline, _lib, config, generation, ops, synthetic
    pipe = _pipe("tiny")
    e = pipe.engine
    for i, name in enumerate(("s1", "s2", "b1", "b2")):
        for bad in (float("nan"), float("inf"), -float("inf")):
            p = [0.9, 0.2, 1.5, 1.6]
            p[i] = bad
            with pytest.raises(_lib.AgendaHipError, match=f"freeu_set: {name} = "):
                e.freeu_set(*p)
    with pytest.raises(_lib.AgendaHipError, match="freeu_set"):
        pipe.enable_freeu(0.9, 0.2, float("nan"), 1.6)
    assert pipe.unet.freeu is None and e.freeu_counts() == (0, 0)       # a refused set leaves FreeU off
    with pytest.raises(_lib.AgendaHipError, match="multiples of 8"):
        ops.freeu(torch.zeros(1, 12, 4, 4).cuda(), torch.zeros(1, 16, 4, 4).cuda(), 1.5, 0.9)
    with pytest.raises(_lib.AgendaHipError, match="finite"):
        ops.freeu(torch.zeros(1, 16, 4, 4).cuda(), torch.zeros(1, 16, 4, 4).cuda(), float("nan"), 0.9)
    with pytest.raises(ValueError, match="share batch and map size"):
        ops.freeu(torch.zeros(1, 16, 4, 4).cuda(), torch.zeros(1, 16, 4, 5).cuda(), 1.5, 0.9)
    e.close()
    with pytest.raises(SystemExit):
        generation.parse_args(["--freeu", "0.9", "0.2", "1.5"])
    # a one-level UNet has no up block 1
    one = config.SDConfig(name="one", unet=config.UNetConfig(block_out_channels=(64,), down_cross=(True,), num_heads=(2,), cross_attention_dim=64),
                          vae=config.VAEConfig(block_out_channels=(64, 64, 128, 128)), default_sample_size=16)
    p1 = StableDiffusionPipeline(one, synthetic.make_unet_weights(one, 11), synthetic.make_vae_weights(one, 12), workspace_bytes=1 << 30)
    with pytest.raises(_lib.AgendaHipError, match="1 level"):
        p1.enable_freeu(*SD15)
    assert p1.unet.freeu is None
    p1.engine.close()
