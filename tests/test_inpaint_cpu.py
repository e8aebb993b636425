"""Inpainting host rules without a GPU: the mask rules, the blend-coefficient program of every scheduler, the generator draw order, the
9-channel config round trip and the refusals."""
import json
import types

import numpy as np
import pytest
import torch

import _inpaint_restated as R


def test_mask_rules_on_hand_built_arrays():
    m = torch.tensor([[[0, 127, 128, 255]]], dtype=torch.uint8).expand(1, 4, 4).contiguous()
    b = R.preprocess_mask(m)
    assert b[0, 0, 0].tolist() == [0.0, 0.0, 1.0, 1.0]
    f = torch.tensor([[[0.0, 0.49999, 0.5, 1.0]]]).expand(1, 4, 4)
    assert R.preprocess_mask(f)[0, 0, 0].tolist() == [0.0, 0.0, 1.0, 1.0]          # 0.5 itself goes to 1
    img = torch.tensor([0, 255, 51], dtype=torch.uint8).view(1, 1, 1, 3)
    assert R.preprocess_image(img).flatten().tolist() == [-1.0, 1.0, 2.0 * (np.float32(51) / np.float32(255)) - 1.0]
    xm = R.masked_image(torch.ones(1, 3, 1, 4), b[:, :, :1])
    assert xm[0, 0, 0].tolist() == [1.0, 1.0, 0.0, 0.0]
    big = torch.zeros(1, 1, 16, 16)
    big[0, 0, 8, 0] = 1.0                       # the pixel (8 i, 8 j) of latent (1, 0)
    big[0, 0, 9, 9] = 1.0                       # never sampled
    lat = R.latent_mask(big, 2)
    assert lat[0, 0].tolist() == [[0.0, 0.0], [1.0, 0.0]]


def _sched(name, n, **kw):
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import SCHEDULERS
    s = SCHEDULERS[name].from_config(SchedulerConfig(**kw))
    return s


def _closed(ts):
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    ac = torch.cumprod(1.0 - betas, 0).numpy().astype(np.float64)
    return [(np.sqrt(ac[t]), np.sqrt(1 - ac[t])) for t in ts[1:]] + [(1.0, 0.0)]


@pytest.mark.parametrize("name,steps,strength,n_evals", [("DDIMScheduler", 10, 1.0, 10), ("DDIMScheduler", 10, 0.6, 6),
                                                         ("PNDMScheduler", 10, 1.0, 11), ("DPMSolverMultistepScheduler", 10, 1.0, 10)])
def test_blend_schedule_matches_closed_form(name, steps, strength, n_evals):
    from agenda_amd.inpaint import blend_schedule, evaluation_timesteps
    s = _sched(name, steps)
    ts = evaluation_timesteps(s, steps, strength)
    assert len(ts) == n_evals
    if name == "DDIMScheduler":
        full = [int(t) for t in (np.arange(0, steps) * (1000 // steps))[::-1] + 1]
        assert ts == full[steps - int(steps * strength):]
    if name == "PNDMScheduler":
        assert ts[1] == ts[2]                                  # the repeated second entry
    if name == "DPMSolverMultistepScheduler":
        assert ts == [int(t) for t in np.linspace(0, 999, steps + 1).round()[::-1][:-1]]
    got = blend_schedule(s, ts)
    want = _closed(ts)
    assert len(got) == len(ts)
    assert got[-1] == (1.0, 0.0)
    for (a, b), (c, d) in zip(got, want):
        assert a == pytest.approx(c, abs=1e-15) and b == pytest.approx(d, abs=1e-15)


def test_generator_draw_order():
    from agenda_amd.inpaint import draw_noises
    N, B, c, L = 1, 2, 4, 8
    g = torch.Generator().manual_seed(3)
    want = [torch.randn(N, c, L, L, generator=g), torch.randn(B, c, L, L, generator=g), torch.randn(N, c, L, L, generator=g)]
    ne, nz, me = draw_noises(torch.Generator().manual_seed(3), N, B, c, L, True, True)
    assert torch.equal(ne, want[0]) and torch.equal(nz, want[1]) and torch.equal(me, want[2])
    # 9-channel at strength 1: no image draw, the noise comes first
    ne, nz, me = draw_noises(torch.Generator().manual_seed(3), N, B, c, L, False, True)
    g = torch.Generator().manual_seed(3)
    assert ne is None and torch.equal(nz, torch.randn(B, c, L, L, generator=g)) and torch.equal(me, torch.randn(N, c, L, L, generator=g))
    # the blend: no masked-image draw
    ne, nz, me = draw_noises(torch.Generator().manual_seed(3), N, B, c, L, True, False)
    assert me is None and torch.equal(ne, want[0]) and torch.equal(nz, want[1])
    # explicit tensors replace their draws only
    x = torch.zeros(B, c, L, L)
    ne, nz, me = draw_noises(torch.Generator().manual_seed(3), N, B, c, L, True, True, noise=x)
    g = torch.Generator().manual_seed(3)
    assert torch.equal(ne, torch.randn(N, c, L, L, generator=g)) and nz is x and torch.equal(me, torch.randn(N, c, L, L, generator=g))


def test_config_json_round_trip_with_nine_input_channels(tmp_path):
    from _util import write_tiny_checkpoint
    from agenda_amd import config, synthetic
    cfg = config.inpaint_variant(config.tiny())
    assert (cfg.unet.in_channels, cfg.unet.out_channels) == (9, 4)
    assert config.inpaint_flavour(cfg) == "concat" and config.inpaint_flavour(config.tiny()) == "blend"
    u = synthetic.make_unet_weights(cfg, 1)
    assert tuple(u["conv_in.weight"].shape) == (64, 9, 3, 3)
    assert tuple(synthetic.make_latents(cfg, [0], 8).shape) == (1, 4, 8, 8)
    write_tiny_checkpoint(str(tmp_path), cfg, {}, {}, scheduler="DDIMScheduler")
    p = tmp_path / "unet" / "config.json"
    j = json.loads(p.read_text())
    j["in_channels"] = 9
    p.write_text(json.dumps(j))
    j2 = json.loads(p.read_text())
    ucfg = config.UNetConfig(in_channels=j2["in_channels"], out_channels=j2["out_channels"])
    assert (ucfg.in_channels, ucfg.out_channels) == (9, 4)


def test_refusals():
    from agenda_amd import StableDiffusionInpaintPipeline, StableDiffusionPipeline, config
    from agenda_amd.inpaint import check_request, prepare_mask_and_image
    cfg4, cfg9 = config.tiny(), config.inpaint_variant(config.tiny())
    ddim, pndm = _sched("DDIMScheduler", 10), _sched("PNDMScheduler", 10)
    dpm_k = _sched("DPMSolverMultistepScheduler", 10, use_karras_sigmas=True)
    assert check_request(cfg9, ddim, 0.5, 10) == "concat"
    assert check_request(cfg4, pndm, 1.0, 10) == "blend"
    assert check_request(cfg9, dpm_k, 1.0, 10) == "concat"                  # Karras is fine without the blend
    with pytest.raises(ValueError, match="use_karras_sigmas"):
        check_request(cfg4, dpm_k, 1.0, 10)
    with pytest.raises(ValueError, match="DDIM"):
        check_request(cfg9, pndm, 0.5, 10)
    with pytest.raises(ValueError, match="< 1"):
        check_request(cfg9, ddim, 0.05, 10)
    odd = config.tiny()
    odd.unet.in_channels = 8
    with pytest.raises(ValueError, match="input channels"):
        check_request(odd, ddim, 1.0, 10)
    with pytest.raises(ValueError, match="input channels"):
        StableDiffusionInpaintPipeline(odd, {}, {})
    with pytest.raises(NotImplementedError, match="ControlNet"):
        StableDiffusionInpaintPipeline(cfg4, {}, {}, controlnet=object())
    fake = types.SimpleNamespace(cfg=cfg9, vae_scale_factor=8, _refuse_inpainting_unet=lambda: StableDiffusionPipeline._refuse_inpainting_unet(fake))
    with pytest.raises(ValueError, match="StableDiffusionInpaintPipeline"):
        StableDiffusionPipeline.__call__(fake, prompt="x")
    with pytest.raises(ValueError, match="StableDiffusionInpaintPipeline"):
        StableDiffusionPipeline.img2img(fake, prompt="x", image=torch.zeros(1, 3, 64, 64))
    img = torch.zeros(1, 64, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="not resized"):
        prepare_mask_and_image(img, torch.zeros(1, 32, 32, dtype=torch.uint8), 64, 64)
    with pytest.raises(ValueError, match="not resized"):
        prepare_mask_and_image(img, torch.zeros(1, 64, 64, dtype=torch.uint8), 128, 128)


def test_cli_flags():
    from agenda_amd.generation import parse_args
    a = parse_args(["--init-image", "a.png", "--mask-image", "m.png", "--strength", "0.7"])
    assert (a.init_image, a.mask_image, a.strength) == ("a.png", "m.png", 0.7)
    with pytest.raises(SystemExit):
        parse_args(["--init-image", "a.png"])
    with pytest.raises(SystemExit):
        parse_args(["--strength", "0.5"])
    with pytest.raises(SystemExit):
        parse_args(["--init-image", "a", "--mask-image", "m", "--controlnet-model-path", "c", "--control-image", "i"])
