"""ControlNet host side: config parsing and refusals, the parameter-shape table, the keep schedule against the restated rule for every
scheduler's evaluation count, the model_index.json round trip of ControlNetModel, the control-image rules and the CLI flags."""
import json

import pytest
import torch

import _controlnet_restated as R


def _cn_json(cfg, **over):
    from agenda_amd.config import ControlNetConfig
    cj = ControlNetConfig().to_json(cfg.unet)
    cj.update(over)
    return cj


def test_config_parses_the_defaults_and_bgr():
    from agenda_amd import config
    cfg = config.sd15()
    c = config.controlnet_config_from_json(_cn_json(cfg), cfg.unet)
    assert c.conditioning_embedding_out_channels == (16, 32, 96, 256) and c.conditioning_channel_order == "rgb"
    assert config.controlnet_config_from_json(_cn_json(cfg, transformer_layers_per_block=[1, 1, 1, 1], num_class_embeds=None), cfg.unet) == c
    c = config.controlnet_config_from_json(_cn_json(cfg, controlnet_conditioning_channel_order="bgr",
                                                    conditioning_embedding_out_channels=[8, 16]), cfg.unet)
    assert c.conditioning_channel_order == "bgr" and c.conditioning_embedding_out_channels == (8, 16)


@pytest.mark.parametrize("over", [
    {"global_pool_conditions": True}, {"class_embed_type": "timestep"}, {"addition_embed_type": "text"}, {"conditioning_channels": 1},
    {"block_out_channels": [320, 640, 1280, 640]}, {"attention_head_dim": 5}, {"cross_attention_dim": 1024},
    {"layers_per_block": 1}, {"use_linear_projection": True}, {"down_block_types": ["DownBlock2D"] * 4},
    {"controlnet_conditioning_channel_order": "rbg"}, {"upcast_attention": True}, {"only_cross_attention": True},
    {"conditioning_embedding_out_channels": [16]}, {"num_class_embeds": 10}, {"transformer_layers_per_block": 2},
    {"transformer_layers_per_block": [1, 2, 1, 1]},
])
def test_config_refuses_what_is_not_implemented(over):
    from agenda_amd import config
    cfg = config.sd15()
    with pytest.raises(ValueError):
        config.controlnet_config_from_json(_cn_json(cfg, **over), cfg.unet)


def test_shape_table_sd15():
    from agenda_amd import config
    cfg = config.sd15()
    p = config.controlnet_param_shapes(cfg.unet, config.ControlNetConfig())
    zc = sorted(k for k in p if k.startswith("controlnet_down_blocks.") and k.endswith(".weight"))
    assert len(zc) == 12
    assert p["controlnet_mid_block.weight"] == (1280, 1280, 1, 1)
    emb = [k for k in p if k.startswith("controlnet_cond_embedding.") and k.endswith(".weight")]
    assert len(emb) == 8
    assert p["controlnet_cond_embedding.conv_in.weight"] == (16, 3, 3, 3)
    assert p["controlnet_cond_embedding.blocks.5.weight"] == (256, 96, 3, 3)
    assert p["controlnet_cond_embedding.conv_out.weight"] == (320, 256, 3, 3)
    assert [p[f"controlnet_down_blocks.{k}.weight"][0] for k in range(12)] == [320] * 4 + [640] * 3 + [1280] * 5
    unet = config.unet_param_shapes(cfg.unet)
    for k, v in p.items():                       # the UNet's encoder half under the same keys and shapes
        if k.startswith(("conv_in.", "time_embedding.", "down_blocks.", "mid_block.")):
            assert unet[k] == v, k
    assert not any(k.startswith(("up_blocks.", "conv_out.", "conv_norm_out.")) for k in p)


def test_synthetic_zero_convs_are_not_zero():
    from agenda_amd import config, synthetic
    cfg = config.tiny()
    sd = synthetic.make_controlnet_weights(cfg)
    for k in range(12):
        assert float(sd[f"controlnet_down_blocks.{k}.weight"].abs().max()) > 0
    assert float(sd["controlnet_mid_block.weight"].abs().max()) > 0


@pytest.mark.parametrize("name,steps,n_evals", [("DDIMScheduler", 50, 50), ("PNDMScheduler", 20, 21), ("DPMSolverMultistepScheduler", 20, 20)])
@pytest.mark.parametrize("start,end", [(0.0, 1.0), (0.4, 1.0), (0.0, 0.5), (0.25, 0.75), (0.1, 0.9)])
def test_keep_schedule_matches_the_restated_rule(name, steps, n_evals, start, end):
    from agenda_amd.config import SchedulerConfig, controlnet_keep_schedule
    from agenda_amd.controlnet import evaluation_count
    from agenda_amd.scheduler import SCHEDULERS
    sch = SCHEDULERS[name].from_config(SchedulerConfig())
    n = evaluation_count(sch, steps)
    assert n == n_evals
    got = controlnet_keep_schedule(n, start, end)
    assert got == R.keep_rule(n, start, end)
    if start == 0.4:
        assert got[:int(0.4 * n)] == [0.0] * int(0.4 * n) and got[-1] == 1.0


def test_keep_schedule_refuses_an_empty_window():
    from agenda_amd.config import controlnet_keep_schedule
    for s, e in [(0.5, 0.5), (0.6, 0.4), (-0.1, 1.0), (0.0, 1.1)]:
        with pytest.raises(ValueError):
            controlnet_keep_schedule(10, s, e)


def test_controlnet_model_round_trip(tmp_path):
    from agenda_amd import config, synthetic
    from agenda_amd.controlnet import ControlNetModel
    cfg = config.tiny()
    cn = config.ControlNetConfig(conditioning_channel_order="bgr")
    sd = synthetic.make_controlnet_weights(cfg, cn, seed=3)
    m = ControlNetModel.from_config(cfg.unet, cn, sd)
    m.save_pretrained(str(tmp_path / "controlnet"))
    back = ControlNetModel.from_pretrained(str(tmp_path / "controlnet"))
    assert back.config["_class_name"] == "ControlNetModel"
    assert config.controlnet_config_from_json(back.config, cfg.unet) == cn
    assert set(back.state_dict) == set(sd)
    assert all(torch.equal(back.state_dict[k], sd[k]) for k in sd)
    json.dumps(back.config)


def test_control_image_rules():
    from PIL import Image
    import numpy as np
    from agenda_amd.controlnet import expand_control_image, prepare_control_image
    im = Image.fromarray((np.arange(40 * 30 * 3) % 251).astype(np.uint8).reshape(40, 30, 3))
    t = prepare_control_image(im, 64, 64)
    want = np.asarray(im.resize((64, 64), resample=Image.LANCZOS)).astype(np.float32) / 255.0
    assert t.shape == (1, 3, 64, 64) and torch.allclose(t[0].permute(1, 2, 0), torch.from_numpy(want))
    u8 = torch.randint(0, 256, (2, 64, 64, 3), dtype=torch.uint8)
    assert torch.equal(prepare_control_image(u8, 64, 64), u8.permute(0, 3, 1, 2).float() / 255.0)
    with pytest.raises(ValueError):
        prepare_control_image(torch.rand(1, 3, 32, 32), 64, 64)
    with pytest.raises(ValueError):
        prepare_control_image(torch.rand(1, 4, 64, 64), 64, 64)
    one = torch.rand(1, 3, 8, 8)
    assert expand_control_image(one, 3, 2).shape[0] == 6
    two = torch.rand(2, 3, 8, 8)
    e = expand_control_image(two, 2, 3)
    assert e.shape[0] == 6 and torch.equal(e[2], two[0]) and torch.equal(e[3], two[1])
    with pytest.raises(ValueError):
        expand_control_image(torch.rand(3, 3, 8, 8), 2, 1)


def test_cli_flags(tmp_path):
    from PIL import Image
    from agenda_amd import generation
    a = generation.parse_args(["--controlnet-model-path", "cn", "--control-image", "x.png", "--controlnet-conditioning-scale", "0.5",
                               "--control-guidance-start", "0.2", "--control-guidance-end", "0.9"])
    assert a.controlnet_model_path == "cn" and a.control_image == "x.png"
    assert (a.controlnet_conditioning_scale, a.control_guidance_start, a.control_guidance_end) == (0.5, 0.2, 0.9)
    d = generation.parse_args([])
    assert d.controlnet_model_path is None and d.controlnet_conditioning_scale == 1.0
    for bad in (["--controlnet-model-path", "cn"], ["--control-image", "x.png"],
                ["--controlnet-model-path", "cn", "--control-image", "x", "--control-guidance-start", "0.9", "--control-guidance-end", "0.1"]):
        with pytest.raises(SystemExit):
            generation.parse_args(bad)
    for n in ("b.png", "a.png", "c.png"):
        Image.new("RGB", (8, 8), (ord(n[0]), 0, 0)).save(tmp_path / n)
    files = generation.control_image_files(str(tmp_path))
    assert [f.split("/")[-1] for f in files] == ["a.png", "b.png", "c.png"]
    imgs = generation.control_images_for(files, [0, 4, 5])
    assert [im.getpixel((0, 0))[0] for im in imgs] == [ord("a"), ord("b"), ord("c")]
    assert generation.control_image_files(str(tmp_path / "a.png")) == [str(tmp_path / "a.png")]
