"""InstructPix2Pix host rules without a GPU: the 8-channel config round trip, the checkpoint's class name, the argument refusals of the
pipeline (on stubs) and of generation.py's flags, the C ABI's new symbols, and two properties of the fp32 restatement the GPU tests lean
on: its three-way combine equals the two-way fold, and with zero image latents it does not depend on image_guidance_scale."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import _ip2p_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["agd_ip2p_prepare_hw", "agd_ip2p_set_hw", "agd_ip2p_clear"]


def test_ip2p_variant():
    from agenda_amd import config, synthetic
    cfg = config.ip2p_variant(config.tiny())
    assert (cfg.unet.in_channels, cfg.unet.out_channels, cfg.vae.latent_channels) == (8, 4, 4) and cfg.name == "tiny-ip2p"
    assert config.tiny().unet.in_channels == 4                                         # the preset itself is untouched
    with pytest.raises(ValueError, match="input channels"):                            # inpainting keeps refusing 8 channels
        config.inpaint_flavour(cfg)
    u = synthetic.make_unet_weights(cfg, 1)
    assert tuple(u["conv_in.weight"].shape) == (64, 8, 3, 3)
    assert tuple(synthetic.make_latents(cfg, [0], 8).shape) == (1, 4, 8, 8)


def test_checkpoint_config_round_trip_and_class_name(tmp_path, monkeypatch):
    """from_pretrained -> save_pretrained -> from_pretrained through the project's own checkpoint reader and writer, with the engine
    construction (the only part that needs a device) replaced: an 8-channel unet/config.json comes back as an 8-channel config, the saved
    model_index.json names the class, and a 4-channel checkpoint is refused by this class."""
    from _util import write_tiny_checkpoint
    from agenda_amd import StableDiffusionInstructPix2PixPipeline, StableDiffusionPipeline, config
    from agenda_amd.scheduler import SCHEDULERS
    seen = []

    def no_engine(self, cfg, unet_sd, vae_sd, scheduler="DDIMScheduler", **kw):
        seen.append((cfg, scheduler))
        self.cfg, self.scheduler = cfg, SCHEDULERS[scheduler].from_config(cfg.sched)
        self.safety_checker, self._lora, self._source_path, self.tokenizer = None, None, None, object()
    monkeypatch.setattr(StableDiffusionPipeline, "__init__", no_engine)
    cfg = config.ip2p_variant(config.tiny())
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, {}, {}, scheduler="PNDMScheduler")
    uc = os.path.join(ck, "unet", "config.json")
    with open(uc) as f:
        j = json.load(f)
    assert j["in_channels"] == 4                                                       # the helper writes txt2img checkpoints
    with pytest.raises(ValueError, match="8 input channels"):
        StableDiffusionInstructPix2PixPipeline.from_pretrained(ck)
    j["in_channels"] = cfg.unet.in_channels
    with open(uc, "w") as f:
        json.dump(j, f)
    pipe = StableDiffusionInstructPix2PixPipeline.from_pretrained(ck)
    got = pipe.cfg.unet
    assert (got.in_channels, got.out_channels, got.block_out_channels) == (8, 4, cfg.unet.block_out_channels)
    assert pipe.cfg.vae.latent_channels == 4 and seen[-1][1] == "PNDMScheduler"
    out = str(tmp_path / "saved")
    pipe.save_pretrained(out)
    with open(os.path.join(out, "model_index.json")) as f:
        assert json.load(f)["_class_name"] == "StableDiffusionInstructPix2PixPipeline"
    with open(os.path.join(out, "unet", "config.json")) as f:
        assert json.load(f)["in_channels"] == 8
    again = StableDiffusionInstructPix2PixPipeline.from_pretrained(out)
    assert again.cfg.unet == got and type(again.scheduler).__name__ == "PNDMScheduler"


def _stub(in_channels=8, hooker=None):
    from agenda_amd import StableDiffusionInstructPix2PixPipeline, config
    pipe = object.__new__(StableDiffusionInstructPix2PixPipeline)
    cfg = config.tiny()
    cfg.unet.in_channels = in_channels
    pipe.cfg = cfg
    pipe.vae_scale_factor = 8
    pipe._hooker, pipe._trace, pipe._lora = hooker, None, None
    return pipe


def test_pipeline_refusals():
    from agenda_amd import StableDiffusionGLIGENPipeline, StableDiffusionInstructPix2PixPipeline, StableDiffusionPipeline, config
    img = torch.zeros(1, 64, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="needs image="):
        _stub()("make it snowy")
    for g, s in ((1.0, 1.5), (0.5, 1.5), (7.5, 0.99), (7.5, 0.0)):
        with pytest.raises(ValueError) as e:
            _stub()("make it snowy", image=img, guidance_scale=g, image_guidance_scale=s)
        assert f"guidance_scale={g}" in str(e.value) and f"image_guidance_scale={s}" in str(e.value) and "not implemented" in str(e.value)
    for c in (4, 9):                                                                   # txt2img and inpainting UNets, by their width
        with pytest.raises(ValueError) as e:
            _stub(in_channels=c)("make it snowy", image=img)
        assert f"takes {c}" in str(e.value) and "8 input channels" in str(e.value)
        bad = config.tiny()
        bad.unet.in_channels = c
        with pytest.raises(ValueError, match="8 input channels"):
            StableDiffusionInstructPix2PixPipeline(bad, {}, {})
        with pytest.raises(ValueError, match="8 input channels"):
            StableDiffusionInstructPix2PixPipeline.from_synthetic(bad, ip2p=False)
    with pytest.raises(NotImplementedError, match="ControlNet"):
        StableDiffusionInstructPix2PixPipeline(config.ip2p_variant(config.tiny()), {}, {}, controlnet=object())
    with pytest.raises(ValueError, match="GLIGEN"):                                    # GLIGEN UNets are built with 4 input channels only
        StableDiffusionGLIGENPipeline(config.ip2p_variant(config.tiny()), {}, {})
    for shape in ((1, 72, 128, 3), (1, 64, 100, 3)):                                   # each side a multiple of 64, both named
        with pytest.raises(ValueError) as e:
            _stub()("make it snowy", image=torch.zeros(shape, dtype=torch.uint8))
        assert f"height={shape[1]}" in str(e.value) and f"width={shape[2]}" in str(e.value) and "64" in str(e.value)
    with pytest.raises(ValueError, match="height=128"):                                # a given size must be the image's
        _stub()("make it snowy", image=img, height=128)
    with pytest.raises(ValueError, match=r"\[B,H,W,3\]"):
        _stub()("make it snowy", image=torch.zeros(1, 3, 64, 64, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        _stub()("make it snowy", image=torch.zeros(1, 64, 64, 3))
    with pytest.raises(ValueError, match="square latents only"):
        _stub(hooker=object())("make it snowy", image=torch.zeros(1, 64, 128, 3, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="instruction edits only"):
        _stub().img2img(prompt="x", image=img)
    # the txt2img pipeline on an 8-channel UNet keeps refusing, and names the pipeline to use
    fake = types.SimpleNamespace(cfg=config.ip2p_variant(config.tiny()), vae_scale_factor=8,
                                 _refuse_inpainting_unet=lambda: StableDiffusionPipeline._refuse_inpainting_unet(fake))
    with pytest.raises(ValueError, match="StableDiffusionInstructPix2PixPipeline"):
        StableDiffusionPipeline.__call__(fake, prompt="x")
    with pytest.raises(ValueError, match="StableDiffusionInstructPix2PixPipeline"):
        StableDiffusionPipeline.img2img(fake, prompt="x", image=torch.zeros(1, 3, 64, 64))
    # a legal call passes every check and fails only where the prompt encoder / engine is first needed
    with pytest.raises(AttributeError):
        _stub()("make it snowy", image=img)


def test_prepare_image_forms():
    from PIL import Image
    from agenda_amd.ip2p import prepare_image
    a = np.random.default_rng(0).integers(0, 256, (64, 128, 3), dtype=np.uint8)
    one = prepare_image(Image.fromarray(a))
    assert one.dtype == torch.uint8 and tuple(one.shape) == (1, 64, 128, 3) and np.array_equal(one[0].numpy(), a)
    two = prepare_image([Image.fromarray(a), Image.fromarray(a[::-1].copy())])
    assert tuple(two.shape) == (2, 64, 128, 3)
    with pytest.raises(ValueError, match="share one size"):
        prepare_image([Image.fromarray(a), Image.fromarray(a[:, :64].copy())])
    f = prepare_image(torch.zeros(2, 3, 64, 64, dtype=torch.float64))
    assert f.dtype == torch.float32 and tuple(f.shape) == (2, 3, 64, 64)
    assert torch.equal(R.preprocess_image(one), 2.0 * (one.permute(0, 3, 1, 2).float() / 255.0) - 1.0)


def test_generation_flags():
    from agenda_amd.generation import parse_args
    a = parse_args(["--instruct-image", "a.png"])
    assert (a.instruct_image, a.image_guidance_scale) == ("a.png", 1.5)
    a = parse_args(["--instruct-image", "dir", "--image-guidance-scale", "2.5", "--scheduler", "DPMSolverMultistepScheduler"])
    assert (a.instruct_image, a.image_guidance_scale) == ("dir", 2.5)
    for bad in (["--image-guidance-scale", "2"], ["--instruct-image", "a", "--image-guidance-scale", "0.5"],
                ["--instruct-image", "a", "--init-image", "i", "--mask-image", "m"],
                ["--instruct-image", "a", "--controlnet-model-path", "c", "--control-image", "i"],
                ["--instruct-image", "a", "--gligen-phrases", "p", "--gligen-boxes", "0", "0", "1", "1"],
                ["--instruct-image", "a", "--gligen-layouts", "l.json"], ["--instruct-image", "a", "--panorama"],
                ["--instruct-image", "a", "--height", "128"], ["--instruct-image", "a", "--width", "128"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
    plain = parse_args([])
    assert plain.instruct_image is None and plain.image_guidance_scale is None


def test_ip2p_inputs_take_image_s_mod_n(tmp_path):
    from PIL import Image
    from agenda_amd.generation import control_image_files, ip2p_inputs_for
    for i, n in enumerate(("a.png", "b.png")):
        Image.fromarray(np.full((64, 128, 3), 10 * (i + 1), dtype=np.uint8)).save(tmp_path / n)
    files = control_image_files(str(tmp_path))
    kw = ip2p_inputs_for(files, [0, 1, 2, 5], 1.5)
    assert [int(np.asarray(im)[0, 0, 0]) for im in kw["image"]] == [10, 20, 10, 20]
    assert (kw["height"], kw["width"], kw["image_guidance_scale"]) == (64, 128, 1.5)
    Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8)).save(tmp_path / "c.png")
    with pytest.raises(ValueError, match="share one size"):
        ip2p_inputs_for(control_image_files(str(tmp_path)), [0, 2], 1.5)


def test_new_symbols_declared_exported_and_bound():
    from agenda_amd import _lib
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/agenda_hip.h"
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.EXPORTS


def test_restated_combine_equals_the_two_way_fold():
    """lo = s_i e_image - (s_i - 1) e_uncond, hi = lo + e_text - e_image: lo + s_t (hi - lo) is the three-way formula for every s_t."""
    g = torch.Generator().manual_seed(0)
    eu, ei, et = (torch.randn(2, 4, 8, 12, generator=g, dtype=torch.float64) for _ in range(3))
    for s_t, s_i in ((7.5, 1.5), (2.0, 1.0), (20.0, 5.0), (1.0, 3.0)):
        lo, hi = R.fold(eu, ei, et, s_i)
        want = R.combine(eu, ei, et, s_t, s_i)
        assert torch.allclose(lo + s_t * (hi - lo), want, rtol=0, atol=1e-12 * float(want.abs().max()))
    eu32, ei32, et32 = eu.float(), ei.float(), et.float()                              # and in fp32 to rounding
    lo, hi = R.fold(eu32, ei32, et32, 1.5)
    want = R.combine(eu, ei, et, 7.5, 1.5)
    assert float((lo + 7.5 * (hi - lo) - want).abs().max()) < 1e-5 * float(want.abs().max())


def test_restatement_ignores_image_scale_with_zero_image_latents():
    """With zero image latents the image branch is the uncond branch, so the loop cannot depend on image_guidance_scale."""
    from agenda_amd import config, synthetic
    cfg = config.ip2p_variant(config.tiny())
    u = synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)
    B, L = 1, 8
    ctx = synthetic.make_context(cfg, B, seed=3)
    nz = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(1))
    zero = torch.zeros(B, 4, L, L)
    a = R.denoise(u, cfg, ctx, zero, nz, 2, "ddim", 7.5, 1.0)
    b = R.denoise(u, cfg, ctx, zero, nz, 2, "ddim", 7.5, 5.0)
    c = R.denoise(u, cfg, ctx, 0.5 * torch.ones(B, 4, L, L), nz, 2, "ddim", 7.5, 5.0)
    assert torch.isfinite(a).all()
    assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max())       # fp32 rounding (~1e-6) times the scales
    assert float((a - c).abs().max()) > 1e-3 * float(a.abs().max())                    # while non-zero image latents do matter
