"""T2I-Adapter, the parts that need no GPU: the restatement's pixel unshuffle, the parameter inventory against the published SD-1.5 full
adapter, the factor-to-schedule rule, the image front door, the Python-side refusals, the T2IAdapter round trip, the library's symbols,
and the restated injection against the oracle's UNet."""
import os
import re

import numpy as np
import pytest
import torch

import _adapter_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rms_rel(got, want):
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def adapter_weights(cfg, acfg, small=True):
    """The synthetic adapter the GPU tests load: gain 1 (features about as large as the UNet's hidden states), small biases on the tiny
    configs as the tiny parity tests draw them."""
    from agenda_amd import synthetic
    return synthetic.make_adapter_weights(cfg, acfg, seed=15 if small else 1237, gain=1.0, bias_std=0.05 if small else 0.0)


def test_restated_unshuffle_is_torch_pixel_unshuffle():
    g = torch.Generator().manual_seed(0)
    for shape, r in (((2, 3, 16, 24), 8), ((1, 1, 8, 8), 2), ((2, 5, 12, 6), 3)):
        x = torch.randn(shape, generator=g)
        assert torch.equal(R.pixel_unshuffle(x, r), torch.nn.functional.pixel_unshuffle(x, r))
    # the index rule itself: out[c r^2 + i r + j][h][w] = in[c][h r + i][w r + j]
    x = torch.arange(2 * 4 * 6, dtype=torch.float32).view(1, 2, 4, 6)
    y = R.pixel_unshuffle(x, 2)
    for c in range(2):
        for i in range(2):
            for j in range(2):
                assert torch.equal(y[0, c * 4 + i * 2 + j], x[0, c, i::2, j::2])


@pytest.mark.parametrize("in_channels", [3, 1])
def test_param_shapes_are_the_published_sd15_full_adapter(in_channels):
    """[upstream-knowledge] TencentARC/t2iadapter_*_sd15v2: conv_in on in_channels * 64 unshuffled channels, four blocks of two resnets at
    320 / 640 / 1280 / 1280, in_conv only where the width changes (blocks 1 and 2)."""
    from agenda_amd import config
    acfg = config.AdapterConfig(in_channels=in_channels)
    got = config.adapter_param_shapes(config.sd15().unet, acfg)
    want = {"adapter.conv_in.weight": (320, in_channels * 64, 3, 3), "adapter.conv_in.bias": (320,),
            "adapter.body.1.in_conv.weight": (640, 320, 1, 1), "adapter.body.1.in_conv.bias": (640,),
            "adapter.body.2.in_conv.weight": (1280, 640, 1, 1), "adapter.body.2.in_conv.bias": (1280,)}
    for i, c in enumerate((320, 640, 1280, 1280)):
        for j in range(2):
            want[f"adapter.body.{i}.resnets.{j}.block1.weight"] = (c, c, 3, 3)
            want[f"adapter.body.{i}.resnets.{j}.block1.bias"] = (c,)
            want[f"adapter.body.{i}.resnets.{j}.block2.weight"] = (c, c, 1, 1)
            want[f"adapter.body.{i}.resnets.{j}.block2.bias"] = (c,)
    assert len(want) == 38
    assert got == want
    # the tiny configs' equal-width levels have no in_conv either
    tiny = config.tiny()
    keys = config.adapter_param_shapes(tiny.unet, config.adapter_config_for(tiny.unet))
    assert [k for k in keys if "in_conv" in k] == ["adapter.body.1.in_conv.weight", "adapter.body.1.in_conv.bias"]


def test_factor_to_schedule_rule():
    from agenda_amd import config
    from agenda_amd.controlnet import evaluation_count
    from agenda_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler
    assert config.adapter_schedule(6, 0.7, 1.0) == [0.7] * 6
    assert config.adapter_schedule(6, 0.7, 0.5) == [0.7] * 3 + [0.0] * 3
    assert config.adapter_schedule(7, 1.0, 0.5) == [1.0] * 3 + [0.0] * 4           # int(3.5) = 3
    assert config.adapter_schedule(5, 1.0, 0.0) == [0.0] * 5
    assert config.adapter_schedule(5, 0.0, 1.0) == [0.0] * 5
    for n, s, f in ((6, 0.7, 0.5), (7, 1.0, 0.99), (50, 0.3, 0.25)):
        assert config.adapter_schedule(n, s, f) == R.factor_rule(n, s, f)
    with pytest.raises(ValueError):
        config.adapter_schedule(5, 1.0, 1.5)
    with pytest.raises(ValueError):
        config.adapter_schedule(5, 1.0, -0.1)
    sc = config.SchedulerConfig()
    # the rule counts model evaluations: PNDM's repeated one counts
    assert evaluation_count(DDIMScheduler.from_config(sc), 6) == 6
    assert evaluation_count(PNDMScheduler.from_config(sc), 6) == 7
    assert evaluation_count(DPMSolverMultistepScheduler.from_config(sc), 6) == 6
    n = evaluation_count(PNDMScheduler.from_config(sc), 6)
    assert config.adapter_schedule(n, 1.0, 0.5) == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]


def test_prepare_adapter_image():
    from PIL import Image
    from agenda_amd.adapter import expand_adapter_image, prepare_adapter_image
    g = np.random.default_rng(0)
    rgb = Image.fromarray(g.integers(0, 256, (96, 80, 3), dtype=np.uint8))
    out = prepare_adapter_image(rgb, 128, 64, 3)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 128, 64, 3)
    assert np.array_equal(out[0].numpy(), np.asarray(rgb.resize((64, 128), resample=Image.LANCZOS)))
    gray = Image.fromarray(g.integers(0, 256, (64, 128), dtype=np.uint8), mode="L")
    out = prepare_adapter_image([gray, gray], None, None, 1)                          # height / width default to the image's
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 64, 128, 1)
    assert np.array_equal(out[1, :, :, 0].numpy(), np.asarray(gray))
    u8 = torch.from_numpy(g.integers(0, 256, (2, 64, 128, 3), dtype=np.uint8))
    assert prepare_adapter_image(u8, None, None, 3) is not None and torch.equal(prepare_adapter_image(u8, 64, 128, 3), u8)
    f = torch.rand(1, 3, 128, 64)
    out = prepare_adapter_image(f.double(), 128, 64, 3)
    assert out.dtype == torch.float32 and torch.equal(out, f)                         # [0,1] stays [0,1]: no 2x - 1
    with pytest.raises(ValueError, match="channels"):
        prepare_adapter_image(rgb, 128, 64, 1)                                        # an RGB image for a 1-channel adapter
    with pytest.raises(ValueError, match="channels"):
        prepare_adapter_image(f, 128, 64, 1)
    with pytest.raises(ValueError, match="multiple of 64"):
        prepare_adapter_image(torch.rand(1, 3, 96, 80), None, None, 3)
    with pytest.raises(ValueError, match="multiple of 64"):
        prepare_adapter_image(rgb, None, None, 3)                                     # 96 x 80 as it is
    with pytest.raises(ValueError, match="output"):
        prepare_adapter_image(f, 128, 128, 3)                                         # a tensor is not resized
    with pytest.raises(ValueError):
        prepare_adapter_image(torch.rand(3, 128, 64), 128, 64, 3)
    with pytest.raises(ValueError):
        prepare_adapter_image([], 128, 64, 3)
    assert expand_adapter_image(u8, 2, 1) is u8
    assert expand_adapter_image(u8[:1], 3, 2).shape[0] == 1                           # one image serves every image of the call
    assert torch.equal(expand_adapter_image(u8, 2, 2), u8.repeat_interleave(2, dim=0))
    with pytest.raises(ValueError, match="batch"):
        expand_adapter_image(u8, 3, 1)


def test_python_refusals_that_need_no_engine():
    from agenda_amd import StableDiffusionAdapterPipeline, T2IAdapter, config
    cfg = config.tiny()
    acfg = config.adapter_config_for(cfg.unet)
    a = T2IAdapter.from_config(acfg, {})
    for kind in ("light_adapter", "full_adapter_xl"):
        with pytest.raises(NotImplementedError, match="adapter_type"):
            StableDiffusionAdapterPipeline(cfg, {}, {}, adapter=T2IAdapter(dict(a.config, adapter_type=kind), {}))
    with pytest.raises(NotImplementedError, match="MultiAdapter"):
        StableDiffusionAdapterPipeline(cfg, {}, {}, adapter=[a, a])
    with pytest.raises(NotImplementedError, match="MultiAdapter"):
        StableDiffusionAdapterPipeline.from_pretrained("nowhere", adapter=[a, a])
    with pytest.raises(ValueError, match="adapter=T2IAdapter"):
        StableDiffusionAdapterPipeline(cfg, {}, {}, adapter=None)
    pipe = object.__new__(StableDiffusionAdapterPipeline)                             # the checks below run before anything touches the engine
    pipe.adapter_cfg = acfg
    with pytest.raises(NotImplementedError, match="list-valued"):
        pipe(prompt="x", image=torch.rand(1, 3, 128, 128), adapter_conditioning_scale=[1.0, 0.5])
    with pytest.raises(NotImplementedError, match="img2img"):
        pipe.img2img(prompt="x", image=torch.rand(1, 3, 128, 128))
    with pytest.raises(ValueError, match="conditioning image"):
        pipe(prompt="x")
    with pytest.raises(ValueError, match="factor"):
        pipe(prompt="x", image=torch.rand(1, 3, 128, 128), adapter_conditioning_factor=2.0)
    with pytest.raises(ValueError, match="channels"):
        pipe(prompt="x", image=torch.rand(1, 1, 128, 128))
    with pytest.raises(ValueError, match="multiple of 64"):
        pipe(prompt="x", image=torch.rand(1, 3, 96, 128))
    with pytest.raises(ValueError, match="output"):
        pipe(prompt="x", image=torch.rand(1, 3, 128, 128), height=64, width=128)
    with pytest.raises(ValueError, match="batch"):
        pipe(prompt=["x", "y"], image=torch.rand(3, 3, 128, 128))


def test_model_index_lookup_refusals(tmp_path):
    import json
    from agenda_amd import StableDiffusionAdapterPipeline
    d = tmp_path / "ck"
    d.mkdir()
    (d / "model_index.json").write_text(json.dumps({"_class_name": "StableDiffusionPipeline"}))
    with pytest.raises(ValueError, match="names no T2IAdapter"):
        StableDiffusionAdapterPipeline.from_pretrained(str(d))
    (d / "model_index.json").write_text(json.dumps({"adapter": ["diffusers", "MultiAdapter"]}))
    with pytest.raises(NotImplementedError, match="MultiAdapter"):
        StableDiffusionAdapterPipeline.from_pretrained(str(d))


@pytest.mark.parametrize("in_channels", [3, 1])
def test_t2iadapter_save_load_round_trip(tmp_path, in_channels):
    import json
    from agenda_amd import T2IAdapter, config
    cfg = config.tiny()
    acfg = config.adapter_config_for(cfg.unet, in_channels)
    sd = adapter_weights(cfg, acfg)
    T2IAdapter.from_config(acfg, sd).save_pretrained(str(tmp_path / "a"))
    with open(tmp_path / "a" / "config.json") as f:
        cj = json.load(f)
    assert cj["adapter_type"] == "full_adapter" and cj["channels"] == list(cfg.unet.block_out_channels)
    assert cj["in_channels"] == in_channels and cj["num_res_blocks"] == 2 and cj["downscale_factor"] == 8
    back = T2IAdapter.from_pretrained(str(tmp_path / "a"))
    assert config.adapter_config_from_json(back.config) == acfg
    assert set(back.state_dict) == set(sd) == set(config.adapter_param_shapes(cfg.unet, acfg))
    for k in sd:
        assert torch.equal(back.state_dict[k], sd[k]), k


ADAPTER_SYMBOLS = ("agd_adapter_configure", "agd_adapter_set_cond_hw", "agd_adapter_features", "agd_adapter_set_schedule",
                   "agd_adapter_clear", "agd_adapter_add_counts")


def test_library_exports_every_adapter_symbol():
    import ctypes
    from agenda_amd import _lib
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    for s in ADAPTER_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/agenda_hip.h"
        assert s in _lib.EXPORTS
    a = _lib.AgdAdapterConfig()
    assert ctypes.sizeof(a) == 4 * (5 + _lib.AGD_MAX_LEVELS)                          # the header's struct: 5 ints + channels[AGD_MAX_LEVELS]


# config, latent height, latent width: the GPU cases' shapes (sd15 runs on the GPU machine only: its fp32 restatement takes minutes here)
CPU_CASES = [("tiny", 16, 16), ("tiny21", 24, 24), ("tiny", 16, 24)]


@pytest.mark.parametrize("name,Lh,Lw", CPU_CASES)
def test_restated_injection_against_the_oracle(name, Lh, Lw):
    """All-zero features give the oracle's UNet exactly; the synthetic adapter the GPU tests load moves the restated forward by at least
    0.15 rms-rel (so "the un-injected forward is five times further away" can hold for an engine within the 0.03 bound)."""
    from agenda_amd import config, synthetic
    from oracle import sd_oracle as O
    cfg = config.CONFIGS[name]()
    acfg = config.adapter_config_for(cfg.unet)
    u = synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)
    a = adapter_weights(cfg, acfg)
    ctx = synthetic.make_context(cfg, 1, seed=6)[1:]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, Lh, Lw, generator=g)
    img = torch.rand(1, 3, 8 * Lh, 8 * Lw, generator=g)
    t = torch.tensor(301.0)
    with torch.no_grad():
        feats = R.adapter_forward(a, acfg, img)
        assert [tuple(f.shape) for f in feats] == [(1, c, Lh >> i, Lw >> i) for i, c in enumerate(cfg.unet.block_out_channels)]
        plain = O.unet_forward(u, cfg.unet, x, t, ctx)
        zero = R.unet_forward_with_adapter(u, cfg.unet, x, t, ctx, [torch.zeros_like(f) for f in feats])
        assert torch.equal(zero, plain)
        assert torch.equal(R.adapted_eps(u, cfg.unet, x, t, ctx, feats, 0.0), plain)
        inj = R.unet_forward_with_adapter(u, cfg.unet, x, t, ctx, feats)
    moved = _rms_rel(plain, inj)
    print(f"restated adapter {name} {Lh}x{Lw}: the plain forward is {moved:.3f} rms-rel away from the injected one")
    assert moved >= 0.15, moved
