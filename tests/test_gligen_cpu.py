"""GLIGEN host side, no GPU: the restated PositionNet pieces, the pipeline's object preparation and scheduled-sampling flags, the refusals,
the config and checkpoint JSON, the per-image layout extension and the pooled-embedding gather."""
import json
import os
import warnings

import pytest
import torch

import _gligen_restated as R
from agenda_amd import gligen as G
from agenda_amd import config


def test_fourier_embedding_matches_the_closed_form_and_index_order():
    g = torch.Generator().manual_seed(0)
    boxes = torch.rand(2, 5, 4, generator=g)
    e = R.fourier_embed(boxes)
    assert e.shape == (2, 5, 64)
    for f in range(8):
        for s in range(2):
            for k in range(4):
                want = (torch.cos if s else torch.sin)(100 ** (f / 8) * boxes[..., k])
                assert torch.allclose(e[..., f * 8 + s * 4 + k], want, atol=1e-5), (f, s, k)


def test_position_net_null_row_is_the_mlp_of_the_null_features():
    cfg = config.tiny()
    sd = G.make_gligen_weights(cfg, seed=3)
    D = cfg.unet.cross_attention_dim
    g = torch.Generator().manual_seed(1)
    boxes, pos = torch.rand(1, 30, 4, generator=g), torch.randn(1, 30, D, generator=g)
    masks = torch.zeros(1, 30)
    masks[0, :4] = 1
    out = R.position_net(sd, boxes, masks, pos)
    p = "position_net."
    h = torch.cat([sd[p + "null_positive_feature"], sd[p + "null_position_feature"]])[None]
    h = torch.nn.functional.silu(torch.nn.functional.linear(h, sd[p + "linears.0.weight"], sd[p + "linears.0.bias"]))
    h = torch.nn.functional.silu(torch.nn.functional.linear(h, sd[p + "linears.2.weight"], sd[p + "linears.2.bias"]))
    null = torch.nn.functional.linear(h, sd[p + "linears.4.weight"], sd[p + "linears.4.bias"])[0]
    for r in range(4, 30):
        assert torch.allclose(out[0, r], null, atol=1e-5)
    assert not torch.allclose(out[0, 0], null, atol=1e-3)


def test_object_tensors_follow_the_pipeline_rules_and_the_uncond_half_is_null():
    D, B = 16, 3
    lay = (["a car", "a truck"], [[0.1, 0.1, 0.4, 0.5], [0.5, 0.2, 0.9, 0.7]])
    pooled = {"a car": torch.ones(D), "a truck": 2 * torch.ones(D)}
    boxes, emb, masks = G.object_tensors([lay] * B, pooled, D)
    wb, we, wm = R.prepare_objects(lay[1], torch.stack([pooled[p] for p in lay[0]]), D, B)
    assert torch.equal(boxes, wb) and torch.equal(emb, we) and torch.equal(masks, wm)
    assert boxes.shape == (2 * B, 30, 4) and masks.shape == (2 * B, 30)
    assert float(masks[:B].abs().sum()) == 0.0                     # the unconditional half sees only null objects
    assert masks[B:, :2].eq(1).all() and masks[B:, 2:].eq(0).all()
    assert float(boxes[:, 2:].abs().sum()) == 0.0 and float(emb[:, 2:].abs().sum()) == 0.0


@pytest.mark.parametrize("sched,steps,n_evals", [("DDIMScheduler", 50, 50), ("PNDMScheduler", 20, 21), ("DPMSolverMultistepScheduler", 20, 20)])
def test_grounding_steps_and_the_flag_schedule(sched, steps, n_evals):
    from agenda_amd.controlnet import evaluation_count
    from agenda_amd.pipeline import SCHEDULERS
    s = SCHEDULERS[sched].from_config(config.SchedulerConfig())
    n = evaluation_count(s, steps)
    assert n == n_evals
    for beta in (0.0, 0.3, 0.5, 1.0):
        flags = G.grounding_flags(beta, n)
        k = R.num_grounding_steps(beta, n)
        assert len(flags) == n and flags == [1] * k + [0] * (n - k)
    assert sum(G.grounding_flags(0.3, 21)) == 6                    # PNDM x 20: int(0.3 * 21)


def test_truncation_warning_and_refusals():
    boxes = [[0.0, 0.0, 0.5, 0.5]] * 31
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ph, bx = G.check_layout(["car"] * 31, boxes)
    assert len(ph) == 30 and len(bx) == 30 and any("30" in str(x.message) for x in w)
    with pytest.raises(ValueError, match="same"):
        G.check_layout(["car", "car"], [[0, 0, 1, 1]])
    with pytest.raises(ValueError, match="outside"):
        G.check_layout(["car"], [[0, 0, 1.2, 1]])
    with pytest.raises(ValueError, match="x0 > x1"):
        G.check_layout(["car"], [[0.6, 0, 0.5, 1]])
    with pytest.raises(ValueError, match="x0 > x1"):
        G.check_layout(["car"], [[0.1, 0.8, 0.5, 0.2]])
    with pytest.raises(ValueError, match="gated-text-image"):
        G.attention_type_of({"attention_type": "gated-text-image"})
    with pytest.raises(ValueError):
        G.attention_type_of({"attention_type": "other"})
    assert G.attention_type_of({}) == "default" and G.attention_type_of({"attention_type": "gated"}) == "gated"


def test_pipeline_level_refusals_before_any_device_work():
    # the class-level refusals need no engine: they fire in __call__ / __init__ before anything touches the device
    p = G.StableDiffusionGLIGENPipeline.__new__(G.StableDiffusionGLIGENPipeline)
    with pytest.raises(ValueError, match="gligen_inpaint_image"):
        p(prompt="x", gligen_phrases=["a"], gligen_boxes=[[0, 0, 1, 1]], gligen_inpaint_image=object())
    with pytest.raises(ValueError, match="img2img"):
        p.img2img(prompt="x")
    cfg = config.tiny()
    with pytest.raises(ValueError, match="ControlNet"):
        G.StableDiffusionGLIGENPipeline(cfg, {}, {}, controlnet=object())
    with pytest.raises(ValueError, match="inpainting"):
        G.StableDiffusionGLIGENPipeline(config.inpaint_variant(cfg), {}, {})
    with pytest.raises(ValueError, match="not a GLIGEN UNet"):
        G.StableDiffusionGLIGENPipeline(cfg, {}, {})
    lora = {"unet.down_blocks.0.attentions.0.transformer_blocks.0.fuser.attn.to_q.lora.down.weight": torch.zeros(4, 64),
            "unet.down_blocks.0.attentions.0.transformer_blocks.0.fuser.attn.to_q.lora.up.weight": torch.zeros(64, 4)}
    with pytest.raises(ValueError, match="fuser"):
        p.load_lora_weights(lora)


def test_param_shapes_cover_every_transformer_block():
    for name in ("tiny", "sd15"):
        cfg = config.CONFIGS[name]()
        shapes = G.gligen_param_shapes(cfg.unet)
        blocks = G.transformer_blocks(cfg.unet)
        assert len(blocks) == 16
        for b in blocks:
            assert shapes[b + "transformer_blocks.0.fuser.alpha_attn"] == ()
        D = cfg.unet.cross_attention_dim
        assert shapes["position_net.linears.0.weight"] == (512, D + 64)
        assert shapes["position_net.linears.4.weight"] == (D, 512)
    sd = G.make_gligen_weights(config.tiny())
    assert all(float(v) != 0.0 for k, v in sd.items() if k.endswith(("alpha_attn", "alpha_dense")))
    assert all(G.is_gligen_key(k) for k in sd)
    assert not G.is_gligen_key("down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q.weight")


def test_checkpoint_config_round_trip(tmp_path):
    from _util import write_tiny_checkpoint
    cfg = config.tiny()
    from agenda_amd import synthetic
    u = synthetic.make_unet_weights(cfg, 1)
    u.update(G.make_gligen_weights(cfg, 2))
    v = synthetic.make_vae_weights(cfg, 3)
    write_tiny_checkpoint(str(tmp_path), cfg, u, v, scheduler="DDIMScheduler")
    uc = tmp_path / "unet" / "config.json"
    j = json.loads(uc.read_text())
    j["attention_type"] = "gated"
    uc.write_text(json.dumps(j))
    assert G.attention_type_of(json.loads(uc.read_text())) == "gated"
    from safetensors.torch import load_file
    back = load_file(str(tmp_path / "unet" / "diffusion_pytorch_model.safetensors"))
    for k in G.gligen_param_shapes(cfg.unet):
        assert k in back and tuple(back[k].shape) == G.gligen_param_shapes(cfg.unet)[k]


def test_per_image_layouts_extension():
    l1 = (["car"], [[0.1, 0.1, 0.3, 0.3]])
    l2 = (["car", "bus"], [[0.5, 0.5, 0.7, 0.9], [0, 0, 0.2, 0.2]])
    lays = G.layouts_for([l1[0], l2[0]], [l1[1], l2[1]], 2)
    assert lays[0] == l1 and lays[1] == l2
    with pytest.raises(ValueError, match="per-image"):
        G.layouts_for([l1[0], l2[0]], [l1[1], l2[1]], 3)
    same = G.layouts_for(l2[0], l2[1], 3)
    assert same == [l2] * 3
    D = 8
    pooled = {"car": torch.ones(D), "bus": -torch.ones(D)}
    boxes, emb, masks = G.object_tensors(lays, pooled, D)
    assert masks[2].tolist()[:2] == [1.0, 0.0] and masks[3].tolist()[:2] == [1.0, 1.0]
    assert torch.equal(emb[3, 1], -torch.ones(D)) and torch.equal(boxes[2, 0], torch.tensor(l1[1][0]))


def test_pooled_gather_is_the_first_eos_row():
    ids = torch.tensor([[0, 5, 9, 1, 1, 1], [0, 7, 1, 1, 1, 1]])
    assert G.first_eos(ids, 1).tolist() == [3, 2]
    # CLIP: EOS is the largest id, so the first EOS is argmax(input_ids) (pooler_output's rule)
    clip = torch.tensor([[49406, 320, 1615, 49407, 49407], [49406, 1615, 49407, 49407, 49407]])
    assert G.first_eos(clip, 49407).tolist() == clip.argmax(-1).tolist()
    from agenda_amd.text import SimpleTokenizer, SyntheticTextEncoder
    tok = SimpleTokenizer(77)
    te = SyntheticTextEncoder(tok, 16)
    p = G.StableDiffusionGLIGENPipeline.__new__(G.StableDiffusionGLIGENPipeline)
    p.tokenizer, p.text_encoder = tok, te
    pooled = p.pooled_phrase_embeddings(["a red car", "a bus"])
    hid = te(["a red car", "a bus"])
    assert torch.equal(pooled["a red car"], hid[0, 4]) and torch.equal(pooled["a bus"], hid[1, 3])
