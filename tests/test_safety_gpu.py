"""The safety checker on the device (`agd_safety_scores`) against transformers' CLIPImageProcessor / CLIPVisionModel and the
restated StableDiffusionSafetyChecker decision (tests/_safety_restated.py), and its place in the pipeline: flagged images come
back black, everything else is untouched, and the generation driver skips the flagged seeds (reference
data_generation/data_generation.py:59-62)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from _safety_restated import CLIP_MEAN, CLIP_STD, cosine_distance, decide, hf_tower, preprocess

pytestmark = pytest.mark.gpu

SMALL = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, projection_dim=64)


def _cfg(n_special=3, n_concepts=17, **tower):
    from agenda_amd import config
    cfg = config.tiny()
    cfg.safety = config.SafetyConfig(n_special=n_special, n_concepts=n_concepts, **tower)
    return cfg


def _pipe(cfg, ssd):
    from agenda_amd import StableDiffusionPipeline, synthetic
    return StableDiffusionPipeline(cfg, synthetic.make_unet_weights(cfg), synthetic.make_vae_weights(cfg), safety_sd=ssd,
                                   workspace_bytes=1 << 30)


def _images(n, side, seed):
    """Random uint8 images with some large-scale structure (a per-image colour ramp under the noise)."""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(0, 1, side, dtype=np.float32)
    out = []
    for _ in range(n):
        base = rng.uniform(0, 255, 3) * ramp[:, None, None] + rng.uniform(0, 255, 3) * ramp[None, :, None] * (1 - ramp[:, None, None])
        out.append(np.clip(base + rng.normal(0, 40, (side, side, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def _rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


# ---- 1. front end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [256, 512, 768])
def test_front_end_matches_clip_image_processor(side):
    from agenda_amd import synthetic
    from PIL import Image
    try:
        from transformers import CLIPImageProcessorPil as Proc
    except ImportError:
        from transformers import CLIPImageProcessor as Proc
    cfg = _cfg(**SMALL)
    pipe = _pipe(cfg, synthetic.make_safety_weights(cfg, 3))
    im = _images(2, side, side)
    _, pix = pipe.safety_checker.scores(torch.from_numpy(im).cuda(), pixels=True)
    pix = pix.cpu().numpy()
    want = preprocess(im)
    hf = Proc(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, resample=3, image_mean=list(CLIP_MEAN),
              image_std=list(CLIP_STD))(images=[Image.fromarray(x) for x in im], return_tensors="np").pixel_values
    assert pix.shape == want.shape == hf.shape == (2, 3, 224, 224)
    assert np.abs(pix - want).max() <= 1e-6
    assert np.abs(pix - hf).max() <= 1e-6
    pipe.engine.close()


# ---- 2. tower -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tower,bound", [(SMALL, 2.0 ** -6), ({}, 2.0 ** -5)], ids=["2x128", "vit_l14"])
def test_tower_matches_transformers_clip_vision(tower, bound):
    """Normalised image embeddings through identity concept rows (cos = e / |e| component by component), plus the cosines
    against 3 special + 17 random concept rows in the same launch."""
    from agenda_amd import _lib, config, synthetic
    P = tower.get("projection_dim", config.SafetyConfig.projection_dim)
    cfg = _cfg(n_special=3, n_concepts=P + 17, **tower)
    ssd = synthetic.make_safety_weights(cfg, 21)
    rnd = ssd["concept_embeds"][P:].clone()
    ssd["concept_embeds"][:P] = torch.eye(P)
    pipe = _pipe(cfg, ssd)
    im = _images(2, 512, 5)
    pipe.engine.profile_begin()
    got = pipe.safety_checker.scores(torch.from_numpy(im).cuda()).cpu().numpy()
    prof = pipe.engine.profile_end()
    other = _lib.load().agd_profile_class_name(9).decode()
    assert [k for k, v in prof.items() if v["launches"]] == [other]        # every launch of the checker is timed under PC_OTHER
    emb = hf_tower(cfg.safety, ssd)(torch.from_numpy(preprocess(im)))
    want_e = torch.nn.functional.normalize(emb).numpy()
    err_e = _rel_rms(got[:, 3:3 + P], want_e)
    want_c = np.concatenate([cosine_distance(emb, ssd["special_care_embeds"]), cosine_distance(emb, rnd)], 1)
    got_c = np.concatenate([got[:, :3], got[:, 3 + P:]], 1)
    err_c = float(np.abs(got_c - want_c).max())
    print(f"safety tower {tower or 'ViT-L/14'}: embeds rel-rms {err_e:.5f}, cosine max abs err {err_c:.5f}")
    assert err_e <= bound, err_e
    assert err_c <= 2.0 ** -7, err_c
    pipe.engine.close()


# ---- 3. flags -------------------------------------------------------------------------------------------------------------
def _threshold(values, margin=0.006):
    """A threshold at least `margin` away from every value, with values on both sides when the gaps allow it."""
    v = np.sort(np.asarray(values, np.float64))
    gaps = [(v[i + 1] - v[i], 0.5 * (v[i] + v[i + 1])) for i in range(len(v) - 1)]
    ok = [m for g, m in gaps if g >= 2 * margin]
    return ok[len(ok) // 2] if ok else float(v[-1] + 0.05)


def test_flags_match_the_restated_rule():
    from agenda_amd import synthetic
    cfg = _cfg(**SMALL)
    ssd = synthetic.make_safety_weights(cfg, 31)
    im = _images(8, 256, 13)
    emb = hf_tower(cfg.safety, ssd)(torch.from_numpy(preprocess(im)))
    sc = cosine_distance(emb, ssd["special_care_embeds"]).astype(np.float64)
    cc = cosine_distance(emb, ssd["concept_embeds"]).astype(np.float64)
    # special care: concept 0's threshold in a gap between the images (clear of each by >= 0.006), the others never reached
    sw = [_threshold(sc[:, 0])] + [float(sc[:, k].max() + 0.05) for k in range(1, sc.shape[1])]
    adj = np.where(sc[:, 0] - sw[0] > 0, 0.01, 0.0)
    assert 0 < adj.sum() < 0.01 * len(im), adj
    # one concept sits 0.005 above an adjusted image (flagged only through the adjustment), clear of every image by >= 0.004 and
    # below at least one; the others are never reached
    cw = [float(x) for x in cc.max(0) + 0.05]
    k0, j = next((k, j) for k in range(cc.shape[1]) for j in np.flatnonzero(adj)
                 if np.all(np.abs(cc[:, k] + adj - cc[j, k] - 0.005) >= 0.004) and np.any(cc[:, k] + adj - cc[j, k] - 0.005 < 0))
    cw[k0] = float(cc[j, k0] + 0.005)
    ssd["special_care_embeds_weights"] = torch.tensor(sw, dtype=torch.float32)
    ssd["concept_embeds_weights"] = torch.tensor(cw, dtype=torch.float32)
    want, detail = decide(sc.astype(np.float32), cc.astype(np.float32), ssd["special_care_embeds_weights"].numpy(),
                          ssd["concept_embeds_weights"].numpy())
    assert detail[j]["concept_scores"][k0] == pytest.approx(0.005) and want[j]
    assert any(want) and not all(want), want
    pipe = _pipe(cfg, ssd)
    dev = torch.from_numpy(im).cuda()
    got = pipe.safety_checker(dev)
    assert got == want
    cos = pipe.safety_checker.scores(dev).cpu().numpy()
    assert np.abs(cos - np.concatenate([sc, cc], 1)).max() < 0.003
    assert decide(cos[:, :3], cos[:, 3:], ssd["special_care_embeds_weights"].numpy(), ssd["concept_embeds_weights"].numpy())[0] == want
    pipe.engine.close()


# ---- 4. end to end --------------------------------------------------------------------------------------------------------
def _write_checker(ck, cfg, ssd):
    from safetensors.torch import save_file
    s = cfg.safety
    os.makedirs(os.path.join(ck, "safety_checker"), exist_ok=True)
    os.makedirs(os.path.join(ck, "feature_extractor"), exist_ok=True)
    vision = {"hidden_size": s.hidden_size, "intermediate_size": s.intermediate_size, "num_hidden_layers": s.num_hidden_layers,
              "num_attention_heads": s.num_attention_heads, "patch_size": s.patch_size, "image_size": s.image_size}
    with open(os.path.join(ck, "safety_checker", "config.json"), "w") as f:
        json.dump({"architectures": ["StableDiffusionSafetyChecker"], "model_type": "clip", "projection_dim": s.projection_dim,
                   "vision_config_dict": vision, "vision_config": vision}, f)
    with open(os.path.join(ck, "feature_extractor", "preprocessor_config.json"), "w") as f:
        json.dump({"crop_size": 224, "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True, "do_resize": True,
                   "feature_extractor_type": "CLIPFeatureExtractor", "image_mean": list(CLIP_MEAN), "image_std": list(CLIP_STD),
                   "resample": 3, "size": 224}, f)
    save_file({k: t.contiguous() for k, t in ssd.items()}, os.path.join(ck, "safety_checker", "model.safetensors"))
    with open(os.path.join(ck, "model_index.json"), "w") as f:
        json.dump({"_class_name": "StableDiffusionPipeline", "unet": ["diffusers", "UNet2DConditionModel"],
                   "vae": ["diffusers", "AutoencoderKL"], "scheduler": ["diffusers", "PNDMScheduler"],
                   "safety_checker": ["stable_diffusion", "StableDiffusionSafetyChecker"],
                   "feature_extractor": ["transformers", "CLIPImageProcessor"]}, f)


PROMPT = "an aerial view image with cars"


def _run(pipe, seeds):
    """The generation pass (images, flags, DAAM maps) and a hook.py-recorder pass of the same batch."""
    from agenda_amd import synthetic, UNetCrossAttentionHooker
    from agenda_amd.trace import trace
    L = pipe.cfg.default_sample_size
    lat = synthetic.make_latents(pipe.cfg, seeds, L)
    with trace(pipe) as trc:
        out = pipe([PROMPT] * len(seeds), num_inference_steps=2, latents=lat, output_type="pt")
        daam = torch.stack([trc.compute_global_heat_map(prompt=PROMPT, image_index=i).heat_maps for i in range(len(seeds))]).cpu()
    hk = UNetCrossAttentionHooker(is_train=False, latent_hw=L)
    pipe.unet.set_attn_processor(hk)
    try:
        out2 = pipe([PROMPT] * len(seeds), num_inference_steps=2, latents=lat, output_type="pt")
        hook = hk.compute_global_heat_map().cpu()
    finally:
        pipe.unet.set_attn_processor("default")
    assert out2.nsfw_content_detected == out.nsfw_content_detected       # (the hook.py pass runs the attn2 kernel chain: images may differ in the last bit)
    return out.images.cpu(), out.nsfw_content_detected, daam, hook


def test_checkpoint_with_safety_checker_end_to_end(tmp_path):
    from _util import write_tiny_checkpoint
    from agenda_amd import StableDiffusionPipeline, config, generation, synthetic
    from agenda_amd.safety import HipSafetyChecker
    from safetensors.torch import save_file
    cfg = config.tiny()
    u, v = synthetic.make_unet_weights(cfg, 3, bias_std=0.05, perturb_norm=0.1), synthetic.make_vae_weights(cfg, 4, bias_std=0.05, perturb_norm=0.1)
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, u, v)
    seeds = [0, 1, 2, 3]
    # phase 1: the checkpoint's checker with identity concept rows gives every image's normalised embedding
    P = SMALL["projection_dim"]
    scfg = _cfg(n_special=3, n_concepts=P, **SMALL)
    ssd = synthetic.make_safety_weights(scfg, 41)
    ssd["concept_embeds"] = torch.eye(P)
    ssd["concept_embeds_weights"] = torch.full((P,), 2.0)
    ssd["special_care_embeds_weights"] = torch.full((3,), 2.0)
    _write_checker(ck, scfg, ssd)
    off = StableDiffusionPipeline.from_pretrained(ck, workspace_bytes=1 << 30, safety_checker=None)
    assert off.safety_checker is None
    img_off, nsfw_off, daam_off, hook_off = _run(off, seeds)
    assert nsfw_off == [False] * 4
    on = StableDiffusionPipeline.from_pretrained(ck, workspace_bytes=1 << 30)
    assert isinstance(on.safety_checker, HipSafetyChecker)
    e = on.safety_checker.scores(img_off.cuda()).cpu().numpy().astype(np.float64)[:, 3:]
    on.engine.close()
    # phase 2: 17 concepts, concept 0 pointing at image 0 with its threshold in the widest gap; nothing else can flag
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(17, P, generator=g)
    d = e[0] - e.mean(0)
    rows[0] = torch.from_numpy(d / np.linalg.norm(d)).float()
    c0 = e @ (d / np.linalg.norm(d))
    w0 = _threshold(c0, margin=0.001)          # both sides are this checker's own fp32 cosines (same tower, same images)
    expect = [bool(np.round(c - w0, 3) > 0) for c in c0]
    assert any(expect) and not all(expect), (c0, w0)
    ssd2 = dict(ssd)
    ssd2["concept_embeds"] = rows
    ssd2["concept_embeds_weights"] = torch.tensor([w0] + [2.0] * 16, dtype=torch.float32)
    save_file({k: t.contiguous() for k, t in ssd2.items()}, os.path.join(ck, "safety_checker", "model.safetensors"))
    on = StableDiffusionPipeline.from_pretrained(ck, workspace_bytes=1 << 30)
    assert on.cfg.safety.n_concepts == 17
    img_on, nsfw_on, daam_on, hook_on = _run(on, seeds)
    assert nsfw_on == expect
    for i, f in enumerate(expect):
        if f:
            assert int(img_on[i].max()) == 0
        else:
            assert torch.equal(img_on[i], img_off[i])
    assert torch.equal(daam_on, daam_off)
    assert torch.equal(hook_on, hook_off)
    # save_pretrained -> from_pretrained keeps the checker; a pipeline loaded without it saves none
    on.save_pretrained(str(tmp_path / "saved"))
    with open(tmp_path / "saved" / "model_index.json") as f:
        assert json.load(f)["safety_checker"] == ["stable_diffusion", "StableDiffusionSafetyChecker"]
    on.engine.close()
    re = StableDiffusionPipeline.from_pretrained(str(tmp_path / "saved"), workspace_bytes=1 << 30)
    assert isinstance(re.safety_checker, HipSafetyChecker) and re.safety_checker(img_off.cuda()) == expect
    re.engine.close()
    off.save_pretrained(str(tmp_path / "saved_off"))
    off.engine.close()
    with open(tmp_path / "saved_off" / "model_index.json") as f:
        assert json.load(f)["safety_checker"] == [None, None]
    p = StableDiffusionPipeline.from_pretrained(str(tmp_path / "saved_off"), workspace_bytes=1 << 30)
    assert p.safety_checker is None
    p.engine.close()
    # the generation driver skips the flagged seeds (black images, data_generation.py:61-62); --no-safety-checker keeps them all
    args = ["--pretrained-model-path", ck, "--num-images", "4", "--batch-size", "4", "--num-inference-steps", "2", "--prompt", PROMPT,
            "--word_token_heatmaps", "cars", "--image-size", "56"]
    generation.main(["--save-dir", str(tmp_path / "gen")] + args)
    assert sorted(os.listdir(tmp_path / "gen" / "images")) == [f"{s}.png" for s, f in zip(seeds, expect) if not f]
    assert sorted(os.listdir(tmp_path / "gen" / "daam_cars_heatmaps")) == [f"{s}.png" for s, f in zip(seeds, expect) if not f]
    generation.main(["--save-dir", str(tmp_path / "gen_all"), "--no-safety-checker"] + args)
    assert sorted(os.listdir(tmp_path / "gen_all" / "images")) == [f"{s}.png" for s in seeds]


def test_checkpoint_without_safety_checker(tmp_path):
    from _util import write_tiny_checkpoint
    from agenda_amd import StableDiffusionPipeline, _lib, config, synthetic
    cfg = config.tiny()
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, synthetic.make_unet_weights(cfg, 3), synthetic.make_vae_weights(cfg, 4))
    p = StableDiffusionPipeline.from_pretrained(ck, workspace_bytes=1 << 30)      # no model_index.json (SD-2.x-style: no checker)
    assert p.safety_checker is None and p.cfg.safety is None
    p.engine.close()
    with open(os.path.join(ck, "model_index.json"), "w") as f:
        json.dump({"_class_name": "StableDiffusionPipeline", "safety_checker": [None, None], "feature_extractor": [None, None]}, f)
    p = StableDiffusionPipeline.from_pretrained(ck, workspace_bytes=1 << 30)
    assert p.safety_checker is None
    p.engine.close()
    with open(os.path.join(ck, "model_index.json"), "w") as f:
        json.dump({"_class_name": "StableDiffusionPipeline", "safety_checker": ["stable_diffusion", "StableDiffusionSafetyChecker"]}, f)
    with pytest.raises(_lib.AgendaHipError, match="safety"):
        StableDiffusionPipeline.from_pretrained(ck, workspace_bytes=1 << 30)
    p = StableDiffusionPipeline.from_pretrained(ck, workspace_bytes=1 << 30, safety_checker=None)
    assert p.safety_checker is None
    p.engine.close()


# ---- 5. errors ------------------------------------------------------------------------------------------------------------
def test_errors_are_statuses_not_faults():
    from agenda_amd import config, synthetic
    from agenda_amd.pipeline import Engine
    from agenda_amd.safety import vision_config
    cfg = _cfg(**SMALL)
    u, v = synthetic.make_unet_weights(cfg), synthetic.make_vae_weights(cfg)
    ssd = synthetic.make_safety_weights(cfg, 51)
    img = torch.zeros(1, 64, 64, 3, dtype=torch.uint8, device="cuda")
    cos = torch.zeros(1, 20, device="cuda")

    def engine():
        e = Engine(cfg, 0, 1 << 30)
        e.load_state_dict(u, "unet.")
        e.load_state_dict(v, "vae.")
        return e

    def err(e):
        return e.lib.agd_last_error(e.ctx).decode()

    # scores without agd_safety_configure
    e = engine()
    e.finalize()
    rc = e.lib.agd_safety_scores(e.ctx, C.c_void_p(img.data_ptr()), 1, 64, C.c_void_p(cos.data_ptr()), None, None)
    assert rc != 0 and "not configured" in err(e)
    e.close()
    # a missing tensor: agd_finalize names it
    e = engine()
    e.safety_configure(cfg.safety)
    e.load_state_dict({k: t for k, t in ssd.items() if k != "vision_model.vision_model.post_layernorm.bias"}, "safety.")
    rc = e.lib.agd_finalize(e.ctx)
    assert rc != 0 and "post_layernorm.bias" in err(e)
    e.close()
    # a wrong struct_size
    e = engine()
    vc = vision_config(cfg.safety)
    vc.struct_size -= 4
    rc = e.lib.agd_safety_configure(e.ctx, C.byref(vc))
    assert rc != 0 and "struct_size" in err(e)
    e.close()
