"""GLIGEN on the device against the fp32 restatement (tests/_gligen_restated.py): the PositionNet output, one fuser forward at C = 320 / 640 /
1280 on square and rectangular maps with real and null objects, a grounded UNet forward, beta = 0 against the plain pipeline bit for bit,
full tiny txt2img under DDIM and DPM-Solver++ against a host-stepped loop, DAAM and hook.py counts, the checkpoint + CLI round trip and the
error statuses of the new ABI."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _gligen_restated as R
from _report import report
from agenda_amd import gligen as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rms_rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _rel(got, want):
    got = got.detach().float().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _weights(cfg, small=True):
    from agenda_amd import synthetic
    kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
    u = synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw)
    v = synthetic.make_vae_weights(cfg, 12 if small else 1235, **kw)
    u.update(G.make_gligen_weights(cfg, 13 if small else 1236))
    return u, v


_SD15 = {}


def _sd15():
    if not _SD15:
        from agenda_amd import config
        cfg = config.sd15()
        _SD15["w"] = (cfg,) + _weights(cfg, small=False)
    return _SD15["w"]


def _pipe(cfg, u, v, scheduler="DDIMScheduler", ws=2 << 30):
    return G.StableDiffusionGLIGENPipeline(cfg, u, v, workspace_bytes=ws, scheduler=scheduler)


def _objects(B2, D, seed, n_real=(3, 0)):
    """boxes / embeddings / masks of B2 rows: the first half with n_real[0] ... objects as the rows' counts cycle through n_real."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B2, 30, 2, generator=g) * 0.5
    boxes = torch.cat([x0, x0 + torch.rand(B2, 30, 2, generator=g) * 0.5], -1)
    emb = torch.randn(B2, 30, D, generator=g).to(torch.bfloat16).float()
    masks = torch.zeros(B2, 30)
    for r in range(B2):
        n = n_real[r % len(n_real)]
        masks[r, :n] = 1
        boxes[r, n:] = 0
        emb[r, n:] = 0
    return boxes, emb, masks


@pytest.mark.parametrize("name", ["tiny", "sd15"])
def test_objs_match_position_net(name):
    from agenda_amd import config
    cfg, u, v = _sd15() if name == "sd15" else ((config.tiny(),) + _weights(config.tiny()))
    pipe = _pipe(cfg, u, v, ws=1 << 30)
    boxes, emb, masks = _objects(4, cfg.unet.cross_attention_dim, 5, (0, 2, 30, 7))
    pipe.engine.gligen_set(boxes, emb, masks)
    got = pipe.engine.gligen_objs(4)
    want = R.position_net(u, boxes, masks, emb)
    e = _rms_rel(got, want)
    print(f"gligen objs {name}: rms rel {e:.4f}")
    report(f"gligen_objs[{name}]", rms_rel=e)
    assert e < 0.01, e
    pipe.engine.close()


FUSER_CASES = [("down_blocks.0.attentions.0.", 320, 8, 8), ("down_blocks.1.attentions.1.", 640, 16, 8), ("up_blocks.1.attentions.2.", 1280, 8, 8),
               ("up_blocks.3.attentions.0.", 320, 12, 20), ("mid_block.attentions.0.", 1280, 4, 6)]


def test_fuser_matches_restatement_and_the_tail_matters():
    cfg, u, v = _sd15()
    pipe = _pipe(cfg, u, v, ws=1 << 30)
    B2 = 4
    boxes, emb, masks = _objects(B2, cfg.unet.cross_attention_dim, 9, (0, 0, 4, 30))     # rows 0, 1 null objects only (the CFG half)
    pipe.engine.gligen_set(boxes, emb, masks)
    objs = R.position_net(u, boxes, masks, emb)
    for pre, C, h, w in FUSER_CASES:
        g = torch.Generator().manual_seed(C + h)
        x = torch.randn(B2, h * w, C, generator=g).to(torch.bfloat16).float()
        got = pipe.engine.gligen_fuser(pre, x, h, w).cpu()
        want = R.fuser(u, pre, x, objs, 8)
        drop = R.fuser(u, pre, x, objs, 8, keep_objs=False)
        e, e_null = _rms_rel(got - x, want - x), _rms_rel(got[:2] - x[:2], want[:2] - x[:2])
        tail = _rms_rel(drop - x, want - x)
        print(f"gligen fuser {pre} C={C} {h}x{w}: delta rms rel {e:.4f} (null rows {e_null:.4f}); without the grounding keys {tail:.4f}")
        report(f"gligen_fuser[{pre}{h}x{w}]", delta_rms_rel=e, null_rows=e_null, tail_effect=tail)
        assert e < 0.02 and e_null < 0.02, (pre, e, e_null)
        assert tail > 10 * e, (pre, tail, e)                       # the 30 grounding keys change the result well beyond the error
    pipe.engine.close()


@pytest.mark.parametrize("name,L,B2", [("tiny", 16, 2), ("sd15", 32, 2)])
def test_grounded_unet_forward_matches_restatement(name, L, B2):
    from agenda_amd import config, synthetic
    cfg, u, v = _sd15() if name == "sd15" else ((config.tiny(),) + _weights(config.tiny()))
    pipe = _pipe(cfg, u, v)
    ctx = synthetic.make_context(cfg, B2 // 2, seed=3)
    x = torch.randn(B2, 4, L, L, generator=torch.Generator().manual_seed(4))
    boxes, emb, masks = _objects(B2, cfg.unet.cross_attention_dim, 6, (0, 5))
    e = pipe.engine
    e.set_context(ctx)
    e.gligen_set(boxes, emb, masks)
    e.gligen_set_schedule([1])
    got = e.unet_forward(x.cuda(), 401.0).cpu()
    e.gligen_set_schedule([0])
    plain = e.unet_forward(x.cuda(), 401.0).cpu()
    e.gligen_set_schedule([])
    objs = R.position_net(u, boxes, masks, emb)
    with torch.no_grad():
        want = R.unet_forward(u, cfg.unet, x, 401.0, ctx, objs)
        want_plain = R.unet_forward(u, cfg.unet, x, 401.0, ctx, None)
    err, err_plain, effect = _rms_rel(got, want), _rms_rel(plain, want_plain), _rms_rel(want_plain, want)
    print(f"gligen unet {name} L={L}: grounded rms rel {err:.4f}, ungrounded {err_plain:.4f}, grounding effect {effect:.4f}")
    report(f"gligen_unet[{name}]", rms_rel=err, plain_rms_rel=err_plain, effect=effect)
    assert err < 0.03 and err_plain < 0.03, (err, err_plain)
    assert effect > 3 * err, (effect, err)
    pipe.engine.close()


def _gen(pipe, ctx, lat, steps, beta, trace_on=True, **kw):
    from agenda_amd import trace
    B = lat.shape[0]
    lay = dict(gligen_phrases=["a car", "a red truck"], gligen_boxes=[[0.1, 0.2, 0.4, 0.5], [0.5, 0.5, 0.9, 0.8]])
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="np", gligen_scheduled_sampling_beta=beta,
                   **lay, **kw)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    return out, hm


@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_beta_zero_is_bit_identical_to_the_plain_pipeline(scheduler):
    from agenda_amd import StableDiffusionPipeline, config, synthetic, trace
    cfg = config.tiny()
    u, v = _weights(cfg)
    B, L, steps = 2, 16, 5
    ctx = synthetic.make_context(cfg, B, seed=42)
    lat = synthetic.make_latents(cfg, [4, 5], L)
    gp = _pipe(cfg, u, v, scheduler=scheduler)
    out, hm = _gen(gp, ctx, lat, steps, 0.0)
    gp.engine.close()
    pp = StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30, scheduler=scheduler)     # the gated UNet, fusers never run
    with trace(pp) as trc:
        ref = pp(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="np")
        rhm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    pp.engine.close()
    assert torch.equal(out.latents.cpu(), ref.latents.cpu())
    assert np.array_equal(out.images, ref.images)
    assert torch.equal(hm, rhm)


def test_beta_zero_is_bit_identical_at_sd15_512_batch4():
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    cfg, u, v = _sd15()
    ctx = synthetic.make_context(cfg, 4, seed=8)
    lat = synthetic.make_latents(cfg, [0, 1, 2, 3], 64)
    gp = _pipe(cfg, u, v, ws=8 << 30)
    out, hm = _gen(gp, ctx, lat, 2, 0.0)
    gp.engine.close()
    pp = StableDiffusionPipeline(cfg, u, v, workspace_bytes=8 << 30)
    with trace(pp) as trc:
        ref = pp(prompt_embeds=ctx, latents=lat, num_inference_steps=2, output_type="np")
        rhm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(4)]).cpu()
    pp.engine.close()
    assert torch.equal(out.latents.cpu(), ref.latents.cpu())
    assert np.array_equal(out.images, ref.images)
    assert torch.equal(hm, rhm)


@pytest.mark.parametrize("scheduler,key", [("DDIMScheduler", "ddim"), ("DPMSolverMultistepScheduler", "dpm")])
def test_pipeline_matches_host_stepped_restatement(scheduler, key):
    from agenda_amd import config, synthetic
    from oracle import sd_oracle as O
    cfg = config.tiny()
    u, v = _weights(cfg)
    B, L, steps, beta = 2, 16, 10, 0.3
    ctx = synthetic.make_context(cfg, B, seed=41)
    lat = synthetic.make_latents(cfg, [1, 2], L)
    pipe = _pipe(cfg, u, v, scheduler=scheduler)
    out, hm = _gen(pipe, ctx, lat, steps, beta)
    lays = pipe.last_layouts
    boxes, emb, masks = G.object_tensors(lays, pipe.pooled_phrase_embeddings([p for ph, _ in lays for p in ph]), cfg.unet.cross_attention_dim)
    pipe.engine.close()
    objs2 = R.position_net(u, boxes, masks, emb)
    rec = O.DaamRecorder(L * L, context_size=cfg.max_tokens)
    want_img, want_lat = R.generate(u, v, cfg, ctx, lat, objs2, steps, key, beta=beta, recorder=rec)
    whm = rec.compute_global_heat_map()
    e_lat, psnr, e_hm = _rms_rel(out.latents, want_lat), _psnr(out.images, want_img), _rel(hm, whm)
    print(f"gligen pipe {key}: latents rms rel {e_lat:.4f}, PSNR {psnr:.1f} dB, heat map rel {e_hm:.4f}")
    report(f"gligen_pipeline[{key}]", latents_rms_rel=e_lat, psnr_db=psnr, heat_map_rel=e_hm)
    assert e_lat < 0.06, e_lat
    assert psnr > 30.0, psnr
    assert e_hm < 0.06, e_hm
    assert float(hm.sum(1).mean()) == pytest.approx(steps, rel=0.02)      # the fusers record nothing: one map per evaluation


def test_grounding_changes_the_output_and_hook_counts_stay():
    from agenda_amd import UNetCrossAttentionHooker, config, synthetic
    cfg = config.tiny()
    u, v = _weights(cfg)
    B, L, steps = 2, 16, 4
    ctx = synthetic.make_context(cfg, B, seed=43)
    lat = synthetic.make_latents(cfg, [6, 7], L)
    pipe = _pipe(cfg, u, v)
    res = {}
    for beta in (0.0, 1.0):
        hk = UNetCrossAttentionHooker(is_train=False, latent_hw=L)
        pipe.unet.set_attn_processor(hk)
        try:
            out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="np", gligen_scheduled_sampling_beta=beta,
                       gligen_phrases=["a car"], gligen_boxes=[[0.2, 0.2, 0.6, 0.6]])
            res[beta] = (out.latents.cpu(), pipe.engine.hook_count(), hk.compute_global_heat_map().cpu())
        finally:
            pipe.unet.set_attn_processor("default")
    pipe.engine.close()
    d = _rms_rel(res[1.0][0], res[0.0][0])
    print(f"gligen beta 1 vs 0: latents rms rel {d:.4f}; hook counts {res[0.0][1]} / {res[1.0][1]}")
    assert d > 0.01, d
    assert res[0.0][1] == res[1.0][1] and res[0.0][1] > 0
    assert res[0.0][2].shape == res[1.0][2].shape


def test_per_image_layouts_match_single_layout_runs():
    from agenda_amd import config, synthetic
    cfg = config.tiny()
    u, v = _weights(cfg)
    L, steps = 16, 3
    pipe = _pipe(cfg, u, v)
    l1 = (["a car"], [[0.1, 0.1, 0.5, 0.5]])
    l2 = (["a bus", "a car"], [[0.5, 0.1, 0.9, 0.6], [0.0, 0.6, 0.3, 1.0]])
    ctx = synthetic.make_context(cfg, 1, seed=44)
    both = pipe(prompt_embeds=torch.cat([ctx[:1], ctx[:1], ctx[1:], ctx[1:]]), latents=synthetic.make_latents(cfg, [3, 4], L),
                num_inference_steps=steps, output_type="latent", gligen_scheduled_sampling_beta=1.0,
                gligen_phrases=[l1[0], l2[0]], gligen_boxes=[l1[1], l2[1]]).latents.cpu()
    singles = [pipe(prompt_embeds=ctx, latents=synthetic.make_latents(cfg, [s], L), num_inference_steps=steps, output_type="latent",
                    gligen_scheduled_sampling_beta=1.0, gligen_phrases=l[0], gligen_boxes=l[1]).latents.cpu() for s, l in ((3, l1), (4, l2))]
    pipe.engine.close()
    e = _rms_rel(both, torch.cat(singles))
    print(f"gligen per-image layouts vs single runs: rms rel {e:.2e}")
    assert e < 2e-2, e


def test_error_statuses():
    from agenda_amd import StableDiffusionPipeline, _lib, config, synthetic
    cfg = config.tiny()
    u, v = _weights(cfg)
    plain = StableDiffusionPipeline(cfg, u, v, workspace_bytes=1 << 30)      # a gated checkpoint under the plain pipeline: no GLIGEN state
    b, e_, m = _objects(2, cfg.unet.cross_attention_dim, 1)
    rc = plain.engine.lib.agd_gligen_set(plain.engine.ctx, None, None, None, 2, None)      # set before configure
    assert rc != 0 and b"no GLIGEN" in plain.engine.lib.agd_last_error(plain.engine.ctx)
    with pytest.raises(_lib.AgendaHipError, match="no GLIGEN"):
        plain.engine.gligen_set(b, e_, m)
    with pytest.raises(_lib.AgendaHipError, match="no GLIGEN"):
        plain.engine.gligen_set_schedule([1])
    plain.engine.close()
    pipe = _pipe(cfg, u, v)
    e = pipe.engine
    ctx = synthetic.make_context(cfg, 1, seed=2)
    e.set_context(ctx)
    b4, e4, m4 = _objects(4, cfg.unet.cross_attention_dim, 1)
    with pytest.raises(_lib.AgendaHipError, match="context holds"):
        e.gligen_set(b4, e4, m4)                                    # 4 rows, the context has 2
    x = torch.randn(2, 4, 16, 16).cuda()
    e.gligen_set_schedule([1])
    with pytest.raises(_lib.AgendaHipError, match="objects are set for 0"):
        e.unet_forward(x, 11.0)                                     # no objects set for these rows
    e.gligen_set(b, e_, m)
    e.gligen_set_schedule([1, 1])
    with pytest.raises(_lib.AgendaHipError, match="schedule"):
        e.unet_forward(x, 11.0)                                     # one evaluation, two flags
    e.gligen_set_schedule([1] * 3)
    pipe.scheduler.set_timesteps(4)
    a_t, a_p = pipe.scheduler.step_coeffs()
    with pytest.raises(_lib.AgendaHipError, match="schedule"):
        e.denoise(torch.randn(1, 4, 16, 16).cuda(), pipe.scheduler.timesteps, a_t, a_p, 7.5)
    e.gligen_clear()
    e.close()


def test_checkpoint_round_trip_and_cli(tmp_path):
    from _util import write_tiny_checkpoint
    from agenda_amd import StableDiffusionPipeline, config, synthetic
    cfg = config.tiny()
    u, v = _weights(cfg)
    ck = str(tmp_path / "ck")
    write_tiny_checkpoint(ck, cfg, u, v, scheduler="DDIMScheduler")
    with pytest.raises(ValueError, match="not a GLIGEN UNet"):
        G.StableDiffusionGLIGENPipeline.from_pretrained(ck)          # attention_type absent: "default"
    uc = os.path.join(ck, "unet", "config.json")
    with open(uc) as f:
        j = json.load(f)
    j["attention_type"] = "gated"
    with open(uc, "w") as f:
        json.dump(j, f)
    pipe = G.StableDiffusionGLIGENPipeline.from_pretrained(ck)
    out2 = str(tmp_path / "saved")
    pipe.save_pretrained(out2)
    with open(os.path.join(out2, "unet", "config.json")) as f:
        assert json.load(f)["attention_type"] == "gated"
    with open(os.path.join(out2, "model_index.json")) as f:
        assert json.load(f)["_class_name"] == "StableDiffusionGLIGENPipeline"
    pipe2 = G.StableDiffusionGLIGENPipeline.from_pretrained(out2)
    ctx = synthetic.make_context(cfg, 1, seed=5)
    lat = synthetic.make_latents(cfg, [9], 16)
    kw = dict(prompt_embeds=ctx, latents=lat, num_inference_steps=3, output_type="latent", gligen_phrases=["a car"],
              gligen_boxes=[[0.1, 0.1, 0.5, 0.5]], gligen_scheduled_sampling_beta=1.0)
    a, b = pipe(**kw).latents.cpu(), pipe2(**kw).latents.cpu()
    pipe.engine.close(); pipe2.engine.close()
    assert torch.equal(a, b)
    plain = StableDiffusionPipeline.from_pretrained(out2)             # the gated UNet under the plain pipeline: no fuser runs
    c = plain(prompt_embeds=ctx, latents=lat, num_inference_steps=3, output_type="latent").latents.cpu()
    plain.engine.close()
    assert not torch.equal(a, c)
    save = tmp_path / "cli"
    cmd = [sys.executable, "-m", "agenda_amd.generation", "--pretrained-model-path", out2, "--save-dir", str(save), "--num-images", "3",
           "--batch-size", "3", "--num-inference-steps", "3", "--image-size", "96", "--word_token_heatmaps", "cars",
           "--prompt", "an aerial view with cars", "--gligen-phrases", "a car", "a bus", "--gligen-boxes", "0.1", "0.1", "0.4", "0.4",
           "0.5", "0.5", "0.9", "0.8", "--gligen-beta", "0.5"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(save / "gligen_layouts.json") as f:
        lj = json.load(f)
    names = sorted(os.listdir(save / "images"))
    assert sorted(lj) == names and len(names) == 3
    e0 = lj[names[0]]
    assert e0["phrases"] == ["a car", "a bus"] and e0["boxes"][1] == [0.5, 0.5, 0.9, 0.8]
    assert e0["boxes_px"][1] == pytest.approx([48.0, 48.0, 86.4, 76.8])
