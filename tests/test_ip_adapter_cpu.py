"""IP-Adapter host side: the file's k numbering, both file formats through the writer and the loader, the pre-multiplied form of the
decoupled attention against the explicit restatement in fp64 (the formula DESIGN.md states), scale 0 and the negative rows of the
restatement, every refusal of the Python surface (none needs the library) and the exported symbols."""
import os
import re

import pytest
import torch

import _ip_adapter_restated as R
from agenda_amd import config, ip_adapter as A, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IPA_SYMBOLS = ["agd_ip_adapter_begin", "agd_ip_adapter_tensor", "agd_ip_adapter_commit", "agd_ip_adapter_unload", "agd_ip_adapter_set",
               "agd_ip_adapter_clear", "agd_ip_adapter_tokens", "agd_ip_adapter_block", "agd_ip_adapter_counts", "agd_image_encoder_begin",
               "agd_image_encoder_tensor", "agd_image_encoder_commit", "agd_image_encoder_unload", "agd_image_embeds"]


def test_key_numbering_is_down_up_mid():
    u = config.sd15().unet
    idx = A.key_indices(u)
    assert sorted(idx) == list(range(1, 32, 2))
    assert idx[1] == "down_blocks.0.attentions.0." and idx[11] == "down_blocks.2.attentions.1."
    assert idx[13] == "up_blocks.1.attentions.0." and idx[29] == "up_blocks.3.attentions.2."
    assert idx[31] == "mid_block.attentions.0."
    assert A.attn2_blocks(u) == R.attn2_order(u)                      # the restatement states the order on its own
    assert R.file_index(u, "mid_block.attentions.0.") == 31
    shapes = A.ip_adapter_param_shapes(u, 1024)
    assert shapes["image_proj.proj.weight"] == (4 * 768, 1024) and shapes["ip_adapter.31.to_k_ip.weight"] == (1280, 768)
    assert shapes["ip_adapter.1.to_v_ip.weight"] == (320, 768) and len(shapes) == 4 + 32


@pytest.mark.parametrize("ext", ["safetensors", "bin"])
def test_both_file_formats_round_trip(tmp_path, ext):
    cfg = config.tiny()
    sd = A.make_ip_adapter_weights(cfg, 3, 96)
    f = A.write_ip_adapter(str(tmp_path / "sub" / f"ip_adapter.{ext}"), sd)
    for got in (A.load_ip_adapter_state_dict(f), A.load_ip_adapter_state_dict(str(tmp_path), subfolder="sub"),
                A.load_ip_adapter_state_dict(str(tmp_path), subfolder="sub", weight_name=f"ip_adapter.{ext}")):
        assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    if ext == "bin":
        nested = torch.load(f, weights_only=True)
        assert sorted(nested) == ["image_proj", "ip_adapter"] and "proj.weight" in nested["image_proj"] and "1.to_k_ip.weight" in nested["ip_adapter"]
    tensors, E, nt = A.to_engine_tensors(A.load_ip_adapter_state_dict(f), cfg)
    assert (E, nt) == (96, 4) and len(tensors) == len(sd)
    assert torch.equal(tensors["mid_block.attentions.0.transformer_blocks.0.attn2.to_k_ip.weight"], sd[f"ip_adapter.{max(A.key_indices(cfg.unet))}.to_k_ip.weight"])
    with pytest.raises(FileNotFoundError, match="local directories and files only"):
        A.load_ip_adapter_state_dict(str(tmp_path / "nowhere"))


CASES = [("sd15", "mid_block.attentions.0.", 8), ("tiny", "down_blocks.1.attentions.0.", 2), ("tiny21", "up_blocks.3.attentions.1.", 1)]


@pytest.mark.parametrize("name,pre,heads", CASES)
def test_premultiplied_form_equals_the_explicit_attention_in_fp64(name, pre, heads):
    cfg = config.CONFIGS[name]()
    assert heads == (cfg.unet.num_heads[-1] if pre.startswith("mid") else tuple(reversed(cfg.unet.num_heads))[3] if pre.startswith("up_blocks.3") else cfg.unet.num_heads[1])
    C, D = A.block_channels(cfg.unet, pre), cfg.unet.cross_attention_dim
    g = torch.Generator().manual_seed(7)
    t = pre + "transformer_blocks.0."
    u = {t + "attn2.to_q.weight": torch.randn(C, C, generator=g, dtype=torch.float64) / C ** 0.5,
         t + "attn2.to_out.0.weight": torch.randn(C, C, generator=g, dtype=torch.float64) / C ** 0.5,
         t + "norm2.weight": 1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64), t + "norm2.bias": 0.1 * torch.randn(C, generator=g, dtype=torch.float64)}
    ip = {k: v.double() for k, v in A.make_ip_adapter_weights(cfg, 5, 32).items()}
    tok = R.image_tokens(ip, R.cfg_embeds(torch.randn(2, 32, generator=g, dtype=torch.float64)), D)
    x = torch.randn(4, 9, C, generator=g, dtype=torch.float64)
    want = R.block(u, ip, cfg.unet, pre, x, tok, heads, 1.0) - x
    kpp, cs, bs, vpp = R.premultiplied(u, ip, cfg.unet, pre, tok, heads)
    assert kpp.shape == (4, heads * 4, C) and vpp.shape == (4, C, heads * 4)
    got = R.premultiplied_delta(x, kpp, cs, bs, vpp, heads)
    assert float((got - want).abs().max()) < 1e-9 and float(want.abs().max()) > 0.1


def test_scale_zero_is_the_text_only_block_and_negative_rows_are_not_zero():
    cfg = config.tiny()
    u = synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)
    ip = A.make_ip_adapter_weights(cfg, 21, 96)
    g = torch.Generator().manual_seed(1)
    emb = R.cfg_embeds(torch.randn(1, 96, generator=g))
    tok = R.image_tokens(ip, emb, 64)
    assert tok.shape == (2, 4, 64) and float(tok[0].abs().mean()) > 0.1            # the projection of zeros: LayerNorm(bias), not zeros
    assert torch.equal(tok, A.project_tokens(ip, emb, 64))
    ctx = synthetic.make_context(cfg, 1, seed=3)
    x = torch.randn(2, 64, 8, 8, generator=g)
    pre = "down_blocks.0.attentions.0."
    with torch.no_grad():
        from _gligen_restated import transformer_2d as text_only
        a = R.transformer_2d(x, ctx, u, cfg.unet, pre, 2, ip, tok, 0.0)
        b = text_only(x, ctx, u, pre, 2, 32, False, None)
        c = R.transformer_2d(x, ctx, u, cfg.unet, pre, 2, ip, tok, 1.0)
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_cfg_image_embeds_builds_the_negative_rows():
    e = torch.randn(2, 8)
    out = A.cfg_image_embeds(e, 2, 2, 1, 8)
    assert out.shape == (4, 8) and torch.equal(out[2:], e) and float(out[:2].abs().max()) == 0.0
    assert torch.equal(A.cfg_image_embeds(e[:1], 3, 3, 1, 8)[3:], e[:1].expand(3, -1))                 # one image for every prompt
    assert torch.equal(A.cfg_image_embeds(e, 4, 2, 2, 8)[4:], e.repeat_interleave(2, 0))               # one per prompt
    both = torch.randn(4, 8)
    assert torch.equal(A.cfg_image_embeds(both, 2, 2, 1, 8), both)                                     # [2B, E] is [neg; pos]
    with pytest.raises(ValueError, match="3 rows for 2 images"):
        A.cfg_image_embeds(torch.randn(3, 8), 2, 2, 1, 8)
    with pytest.raises(ValueError, match="expected \\[rows, 8\\]"):
        A.cfg_image_embeds(torch.randn(2, 9), 2, 2, 1, 8)
    with pytest.raises(ValueError, match="more than one adapter"):
        A.cfg_image_embeds([e, e], 2, 2, 1, 8)


def test_unsupported_files_are_refused_by_name():
    cfg = config.tiny()
    sd = A.make_ip_adapter_weights(cfg, 3, 96)
    with pytest.raises(ValueError, match="'plus'"):
        A.to_engine_tensors({**sd, "image_proj.latents": torch.zeros(1, 16, 64)}, cfg)
    with pytest.raises(ValueError, match="Resampler"):
        A.to_engine_tensors({**sd, "image_proj.layers.0.0.to_q.weight": torch.zeros(4, 4)}, cfg)
    with pytest.raises(ValueError, match="'full-face'"):
        A.to_engine_tensors({**sd, "image_proj.ff.net.0.proj.weight": torch.zeros(4, 4)}, cfg)
    with pytest.raises(ValueError, match="FaceID"):
        A.to_engine_tensors({**sd, "ip_adapter.1.to_k_lora.down.weight": torch.zeros(4, 4)}, cfg)
    sdxl = {k: (torch.zeros(v.shape[0], 2048) if k.endswith("_ip.weight") else v) for k, v in sd.items()}
    with pytest.raises(ValueError, match="SDXL"):
        A.to_engine_tensors(sdxl, cfg)
    with pytest.raises(ValueError, match="SDXL"):
        A.to_engine_tensors({**sd, "image_proj.proj.weight": torch.zeros(4 * 64 + 1, 96)}, cfg)
    more = {**sd, "ip_adapter.33.to_k_ip.weight": torch.zeros(64, 64), "ip_adapter.33.to_v_ip.weight": torch.zeros(64, 64)}
    with pytest.raises(ValueError, match="this UNet has 16"):
        A.to_engine_tensors(more, cfg)
    with pytest.raises(ValueError, match="'ip_adapter.1.to_v_ip.weight' is missing"):
        A.to_engine_tensors({k: v for k, v in sd.items() if k != "ip_adapter.1.to_v_ip.weight"}, cfg)
    with pytest.raises(ValueError, match=r"'ip_adapter.3.to_k_ip.weight' is \(65, 64\)"):
        A.to_engine_tensors({**sd, "ip_adapter.3.to_k_ip.weight": torch.zeros(65, 64)}, cfg)
    with pytest.raises(ValueError, match="'image_proj.norm.bias' is missing"):
        A.to_engine_tensors({k: v for k, v in sd.items() if k != "image_proj.norm.bias"}, cfg)
    with pytest.raises(ValueError, match="cannot place key 'something.else'"):
        A.to_engine_tensors({**sd, "something.else": torch.zeros(1)}, cfg)
    with pytest.raises(ValueError, match="more than one adapter"):
        A.load_ip_adapter_state_dict([sd, sd])
    with pytest.raises(ValueError, match="more than one adapter"):
        A.load_ip_adapter_state_dict("/tmp", weight_name=["a.bin", "b.bin"])


class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was reached ({name}) before the refusal")


def _bare(cls, loaded):
    p = cls.__new__(cls)
    p.cfg = config.tiny()
    p.engine = _NoEngine()
    p._ip_adapter = {"embed_dim": 96, "n_tokens": 4, "scale": 1.0} if loaded else None
    return p


def test_pipeline_refusals_need_no_library():
    import agenda_amd as M
    sd = A.make_ip_adapter_weights(config.tiny(), 3, 96)
    for cls in (M.StableDiffusionControlNetPipeline, M.StableDiffusionAdapterPipeline, M.StableDiffusionGLIGENPipeline,
                M.StableDiffusionInpaintPipeline, M.StableDiffusionInstructPix2PixPipeline, M.StableDiffusionPanoramaPipeline):
        with pytest.raises(ValueError, match=f"load_ip_adapter: the IP-Adapter with {cls.__name__} is not implemented"):
            _bare(cls, False).load_ip_adapter(sd)
    P = M.StableDiffusionPipeline
    with pytest.raises(ValueError, match="more than one adapter is not supported"):
        _bare(P, True).load_ip_adapter(sd)
    with pytest.raises(ValueError, match="list-valued scale"):
        _bare(P, True).set_ip_adapter_scale([0.5, 0.7])
    with pytest.raises(ValueError, match="no IP-Adapter loaded"):
        _bare(P, False).set_ip_adapter_scale(0.5)
    emb = torch.randn(1, 96)
    with pytest.raises(ValueError, match="ip_adapter_image and ip_adapter_image_embeds were both given"):
        _bare(P, True)._apply_ip_adapter(1, 1, 1, object(), emb)
    with pytest.raises(ValueError, match="ip_adapter_image_embeds was given but no IP-Adapter is loaded"):
        _bare(P, False)._apply_ip_adapter(1, 1, 1, None, emb)
    with pytest.raises(ValueError, match="ip_adapter_image was given but no IP-Adapter is loaded"):
        _bare(P, False)._apply_ip_adapter(1, 1, 1, object(), None)
    with pytest.raises(ValueError, match="ip_adapter_image was given but no image encoder is loaded"):
        _bare(P, True)._apply_ip_adapter(1, 1, 1, object(), None)
    _bare(P, False)._apply_ip_adapter(1, 1, 1, None, None)                # nothing loaded, nothing given: the engine is not touched
    p = _bare(P, True)
    p.set_ip_adapter_scale(0.25)
    assert p._ip_adapter["scale"] == 0.25


def test_cli_flags_go_together():
    from agenda_amd import generation
    base = ["--synthetic-config", "tiny", "--save-dir", "/tmp/x", "--num-images", "1", "--prompt", "p"]
    for extra in (["--ip-adapter-path", "a.bin"], ["--ip-adapter-image", "e.png"], ["--ip-adapter-scale", "0.5"], ["--image-encoder-path", "d"],
                  ["--ip-adapter-path", "a.bin", "--ip-adapter-image", "e.png", "--panorama"]):
        with pytest.raises(SystemExit):
            generation.parse_args(base + extra)
    a = generation.parse_args(base + ["--ip-adapter-path", "a.bin", "--ip-adapter-image", "e.png", "--image-encoder-path", "d"])
    assert (a.ip_adapter_path, a.ip_adapter_image, a.image_encoder_path, a.ip_adapter_scale) == ("a.bin", "e.png", "d", 1.0)


def test_image_encoder_directory_round_trips(tmp_path):
    scfg = A.image_encoder_config(hidden_size=320, num_attention_heads=4, intermediate_size=640, num_hidden_layers=2, image_size=28, size=28,
                                  crop_size=28, projection_dim=64)
    sd = A.make_image_encoder_weights(scfg, 4)
    assert "vision_model.embeddings.class_embedding" in sd and sd["visual_projection.weight"].shape == (64, 320)
    assert not any(k.startswith("vision_model.vision_model.") or "concept" in k for k in sd)
    d = A.write_image_encoder(str(tmp_path / "ad" / "image_encoder"), scfg, sd)
    got_cfg, got = A.load_image_encoder(d)
    assert (got_cfg.hidden_size, got_cfg.num_attention_heads, got_cfg.image_size, got_cfg.projection_dim, got_cfg.hidden_act, got_cfg.n_concepts) == (320, 4, 28, 64, "gelu", 0)
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    f = str(tmp_path / "ad" / "ip_adapter.bin")
    assert A.find_image_encoder(f, None, "image_encoder") == d and A.find_image_encoder(str(tmp_path / "ad"), None, "image_encoder") == d
    assert A.find_image_encoder({}, None, d) == d and A.find_image_encoder({}, None, "image_encoder") is None
    full = A.image_encoder_config()
    assert (full.hidden_size // full.num_attention_heads, full.num_hidden_layers, full.projection_dim) == (80, 32, 1024)
    with pytest.raises(ValueError, match="is missing"):
        from safetensors.torch import save_file
        save_file({k: t for k, t in sd.items() if k != "visual_projection.weight"}, os.path.join(d, "model.safetensors"))
        A.load_image_encoder(d)
    imgs = A.prepare_ip_adapter_image([torch.zeros(8, 6, 3, dtype=torch.uint8), torch.zeros(2, 8, 6, 3, dtype=torch.uint8)])
    assert imgs.shape == (3, 8, 6, 3)
    with pytest.raises(ValueError, match="share one size"):
        A.prepare_ip_adapter_image([torch.zeros(8, 6, 3, dtype=torch.uint8), torch.zeros(8, 7, 3, dtype=torch.uint8)])


def test_library_exports_every_ip_adapter_symbol():
    import ctypes
    from agenda_amd import _lib
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    for s in IPA_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/agenda_hip.h"
        assert s in _lib.EXPORTS
