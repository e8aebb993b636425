"""LoRA state dicts -> engine merge inputs (agenda_amd/lora.py), no GPU: key mapping of every accepted format, alpha / rank, 1x1-conv
factors, refusals naming the offending key, file loading by weight_name, and generation.py's --lora-* flags."""
import os

import pytest
import torch

from agenda_amd import config, lora
from agenda_amd.generation import parse_args

B0 = "down_blocks.0.attentions.0"
T0 = B0 + ".transformer_blocks.0"


def _cfg():
    c = config.tiny()
    c.text = config.TextConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, vocab_size=600)
    return c


def _f(r, n, seed=0):
    return torch.randn(r, n, generator=torch.Generator().manual_seed(seed))


def _shape(cfg, key):
    return lora.target_modules(cfg)[key][1]


def test_targets_cover_every_block_and_text_layer():
    cfg = _cfg()
    t = lora.target_modules(cfg)
    blocks = {k[:k.index(".transformer_blocks.")] for k in config.unet_param_shapes(cfg.unet) if ".transformer_blocks.0.attn1.to_q.weight" in k}
    assert len([k for k in t if not k.startswith("text_model.")]) == 12 * len(blocks)
    assert len([k for k in t if k.startswith("text_model.")]) == 6 * cfg.text.num_hidden_layers
    assert t[T0 + ".ff.net.0.proj"][0] == "unet." + T0 + ".ff.net.0.proj.weight"
    assert t["text_model.encoder.layers.1.mlp.fc2"][0] == "text.encoder.layers.1.mlp.fc2.weight"


def test_kohya_mapping_and_alpha():
    cfg = _cfg()
    n_out, n_in = _shape(cfg, T0 + ".attn2.to_k")
    sd = {"lora_unet_" + (T0 + ".attn2.to_k").replace(".", "_") + ".lora_down.weight": _f(4, n_in),
          "lora_unet_" + (T0 + ".attn2.to_k").replace(".", "_") + ".lora_up.weight": _f(n_out, 4, 1),
          "lora_unet_" + (T0 + ".attn2.to_k").replace(".", "_") + ".alpha": torch.tensor(2.0),
          "lora_te_text_model_encoder_layers_1_self_attn_out_proj.lora_down.weight": _f(8, 128, 2),
          "lora_te_text_model_encoder_layers_1_self_attn_out_proj.lora_up.weight": _f(128, 8, 3)}
    es = {e.key: e for e in lora.lora_to_engine(sd, cfg)}
    e = es["unet." + T0 + ".attn2.to_k.weight"]
    assert e.alpha == 2.0 and e.alpha / e.down.shape[0] == 0.5 and e.down.dtype == torch.float32
    assert tuple(e.down.shape) == (4, n_in) and tuple(e.up.shape) == (n_out, 4)
    t = es["text.encoder.layers.1.self_attn.out_proj.weight"]
    assert t.alpha == 8.0                      # no .alpha key: scale 1
    assert torch.equal(t.down, sd["lora_te_text_model_encoder_layers_1_self_attn_out_proj.lora_down.weight"])


def test_diffusers_and_attn_procs_mapping():
    cfg = _cfg()
    C = _shape(cfg, T0 + ".attn1.to_q")[0]
    H4 = _shape(cfg, T0 + ".ff.net.0.proj")[0]
    sd = {f"unet.{T0}.attn1.to_q.lora.down.weight": _f(2, C), f"unet.{T0}.attn1.to_q.lora.up.weight": _f(C, 2),
          f"unet.{T0}.ff.net.0.proj.lora.down.weight": _f(2, C), f"unet.{T0}.ff.net.0.proj.lora.up.weight": _f(H4, 2),
          f"{T0}.attn1.processor.to_out_lora.down.weight": _f(2, C), f"{T0}.attn1.processor.to_out_lora.up.weight": _f(C, 2),
          f"unet.{T0}.attn2.processor.to_v_lora.down.weight": _f(2, cfg.unet.cross_attention_dim),
          f"unet.{T0}.attn2.processor.to_v_lora.up.weight": _f(C, 2),
          "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_linear_layer.down.weight": _f(2, 128),
          "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_linear_layer.up.weight": _f(128, 2),
          "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_linear_layer.down.weight": _f(2, 128),
          "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_linear_layer.up.weight": _f(256, 2),
          "text_encoder.text_model.encoder.layers.1.self_attn.to_out_lora.down.weight": _f(2, 128),
          "text_encoder.text_model.encoder.layers.1.self_attn.to_out_lora.up.weight": _f(128, 2)}
    keys = sorted(e.key for e in lora.lora_to_engine(sd, cfg))
    assert keys == sorted(["unet." + T0 + ".attn1.to_q.weight", "unet." + T0 + ".ff.net.0.proj.weight", "unet." + T0 + ".attn1.to_out.0.weight",
                           "unet." + T0 + ".attn2.to_v.weight", "text.encoder.layers.0.self_attn.q_proj.weight",
                           "text.encoder.layers.0.mlp.fc1.weight", "text.encoder.layers.1.self_attn.out_proj.weight"])


def test_conv1x1_factors_reshape():
    cfg = _cfg()
    C = _shape(cfg, B0 + ".proj_in")[0]
    d, u = _f(3, C).reshape(3, C, 1, 1), _f(C, 3, 1).reshape(C, 3, 1, 1)
    (e,) = lora.lora_to_engine({f"lora_unet_{B0.replace('.', '_')}_proj_in.lora_down.weight": d,
                                f"lora_unet_{B0.replace('.', '_')}_proj_in.lora_up.weight": u}, cfg)
    assert e.key == f"unet.{B0}.proj_in.weight" and tuple(e.down.shape) == (3, C) and tuple(e.up.shape) == (C, 3)
    assert torch.equal(e.down, d.reshape(3, C)) and torch.equal(e.up, u.reshape(C, 3))


@pytest.mark.parametrize("bad", [
    "lora_unet_down_blocks_0_resnets_0_conv1.lora_down.weight",            # LoCon on a resnet
    "lora_unet_down_blocks_0_resnets_0_time_emb_proj.lora_down.weight",
    "lora_unet_input_blocks_1_1_proj_in.lora_down.weight",                # LDM naming
    "lora_unet_down_blocks_0_downsamplers_0_conv.lora_down.weight",
    "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q.hada_w1_a",   # LoHa
    "lora_unet_down_blocks_0_attentions_0_transformer_blocks_0_attn1_to_q.lokr_w1",     # LoKr
    "unet.down_blocks.0.resnets.0.conv1.lora.down.weight",
])
def test_refusals_name_the_key(bad):
    cfg = _cfg()
    good = f"lora_unet_{T0.replace('.', '_')}_attn1_to_q"
    C = _shape(cfg, T0 + ".attn1.to_q")[0]
    sd = {good + ".lora_down.weight": _f(2, C), good + ".lora_up.weight": _f(C, 2), bad: _f(2, C)}
    with pytest.raises(ValueError, match=bad.replace(".", r"\.")):
        lora.lora_to_engine(sd, cfg)


def test_shape_rank_and_conv_refusals():
    cfg = _cfg()
    k = f"lora_unet_{T0.replace('.', '_')}_attn1_to_q"
    C = _shape(cfg, T0 + ".attn1.to_q")[0]
    with pytest.raises(ValueError, match=k + r"\.lora_up\.weight"):
        lora.lora_to_engine({k + ".lora_down.weight": _f(4, C), k + ".lora_up.weight": _f(C, 2)}, cfg)          # rank mismatch
    with pytest.raises(ValueError, match=k + r"\.lora_down\.weight"):
        lora.lora_to_engine({k + ".lora_down.weight": _f(4, C + 1), k + ".lora_up.weight": _f(C, 4)}, cfg)      # shape mismatch
    with pytest.raises(ValueError, match=k + r"\.lora_down\.weight.*conv"):
        lora.lora_to_engine({k + ".lora_down.weight": torch.zeros(4, C, 3, 3), k + ".lora_up.weight": _f(C, 4)}, cfg)
    with pytest.raises(ValueError, match=k + r"\.lora_down\.weight"):
        lora.lora_to_engine({k + ".lora_down.weight": _f(4, C)}, cfg)                                            # no up factor
    no_text = config.tiny()
    with pytest.raises(ValueError, match="lora_te_text_model_encoder_layers_0_mlp_fc1"):
        lora.lora_to_engine({"lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": _f(2, 128),
                             "lora_te_text_model_encoder_layers_0_mlp_fc1.lora_up.weight": _f(256, 2)}, no_text)


def test_load_by_weight_name(tmp_path):
    from safetensors.torch import save_file
    cfg = _cfg()
    k = f"lora_unet_{T0.replace('.', '_')}_attn1_to_v"
    C = _shape(cfg, T0 + ".attn1.to_v")[0]
    sd = {k + ".lora_down.weight": _f(2, C), k + ".lora_up.weight": _f(C, 2), k + ".alpha": torch.tensor(1.0)}
    save_file(sd, str(tmp_path / "pytorch_lora_weights.safetensors"))
    torch.save({k_: v * 2 for k_, v in sd.items()}, str(tmp_path / "pytorch_lora_weights.bin"))
    save_file({k_: v * 3 for k_, v in sd.items()}, str(tmp_path / "mine.safetensors"))
    got = lora.load_lora_state_dict(str(tmp_path))                                   # .safetensors first
    assert torch.equal(got[k + ".lora_down.weight"], sd[k + ".lora_down.weight"])
    got = lora.load_lora_state_dict(str(tmp_path), weight_name="pytorch_lora_weights.bin")
    assert torch.equal(got[k + ".lora_down.weight"], 2 * sd[k + ".lora_down.weight"])
    got = lora.load_lora_state_dict(str(tmp_path), weight_name="mine.safetensors")
    assert torch.equal(got[k + ".lora_down.weight"], 3 * sd[k + ".lora_down.weight"])
    os.remove(tmp_path / "pytorch_lora_weights.safetensors")
    got = lora.load_lora_state_dict(str(tmp_path))                                   # then .bin
    assert torch.equal(got[k + ".lora_down.weight"], 2 * sd[k + ".lora_down.weight"])
    with pytest.raises(FileNotFoundError):
        lora.load_lora_state_dict(str(tmp_path), weight_name="absent.safetensors")
    (e,) = lora.lora_to_engine(lora.load_lora_state_dict(str(tmp_path / "mine.safetensors")), cfg)
    assert e.alpha == 3.0


def test_generation_lora_flags():
    a = parse_args(["--lora-path", "/x/lora", "--lora-weight-name", "w.safetensors", "--lora-scale", "0.6"])
    assert a.lora_path == "/x/lora" and a.lora_weight_name == "w.safetensors" and a.lora_scale == 0.6
    a = parse_args([])
    assert a.lora_path is None and a.lora_weight_name is None and a.lora_scale == 1.0
    with pytest.raises(SystemExit):
        parse_args(["--lora-scale", "0.5"])
