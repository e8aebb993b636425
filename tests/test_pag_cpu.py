"""Perturbed-Attention Guidance without a GPU: layer-name resolution, the per-evaluation scale schedule under the three schedulers, the
restatement's identities (tests/_pag_restated.py), argument validation and the refusals that are raised before any device work, the CLI
flags, and the C ABI's new symbols."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import _pag_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- layer names ----------------------------------------------------------------------------------------------------------------
def _n_transformers(u):
    return sum(u.down_cross) * (2 * u.layers_per_block + 1) + 1


@pytest.mark.parametrize("name", ["tiny", "tiny40", "sd15"])
def test_layer_name_resolution(name):
    from agenda_amd import config
    cfg = config.CONFIGS[name]()
    names = config.self_attn_layer_names(cfg)
    assert names == config.self_attn_layer_names(cfg.unet)
    assert len(names) == len(set(names)) == _n_transformers(cfg.unet)
    assert names == [n.replace("attn2", "attn1") for n in config.cross_attn_layer_names(cfg.unet)]
    assert config.resolve_pag_layers(cfg, ["mid"]) == ["mid_block.attentions.0.transformer_blocks.0.attn1"]
    assert config.resolve_pag_layers(cfg, "mid") == config.resolve_pag_layers(cfg, ["mid"])
    down = config.resolve_pag_layers(cfg, ["down"])
    assert down == [n for n in names if n.startswith("down_blocks.")] and len(down) == sum(cfg.unet.down_cross) * cfg.unet.layers_per_block
    up1 = config.resolve_pag_layers(cfg, ["up_blocks.1"])
    want_up1 = [f"up_blocks.1.attentions.{j}.transformer_blocks.0.attn1" for j in range(cfg.unet.layers_per_block + 1)] if cfg.unet.up_cross[1] else None
    assert want_up1 is not None and up1 == want_up1
    full = names[-2]
    assert config.resolve_pag_layers(cfg, [full]) == [full]
    # several strings: the union, each layer once, in self_attn_layer_names' order
    assert config.resolve_pag_layers(cfg, ["mid", "down", "mid"]) == [n for n in names if n.startswith(("down_blocks.", "mid_block."))]
    assert config.resolve_pag_layers(cfg, [r"attentions\.0"]) == [n for n in names if ".attentions.0." in n]
    assert config.resolve_pag_layers(cfg, []) == []
    for bad in ("middle", "up_blocks.9", "attn2"):
        with pytest.raises(ValueError, match=re.escape(bad)):
            config.resolve_pag_layers(cfg, ["mid", bad])


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
def test_pag_schedule_values():
    from agenda_amd.config import pag_schedule
    ts = [981, 741, 501, 261, 21]
    assert pag_schedule(ts, 3.0, 0.0) == [3.0] * 5
    assert pag_schedule(ts, 3.0) == [3.0] * 5
    got = pag_schedule(ts, 3.0, 0.005)
    assert got == [max(0.0, 3.0 - 0.005 * (1000 - t)) for t in ts]
    assert got[0] == pytest.approx(2.905) and got[2] == pytest.approx(0.505) and got[3] == 0.0 and got[4] == 0.0      # clipped at 0
    assert all(a >= b for a, b in zip(got, got[1:]))
    assert pag_schedule([], 3.0, 0.1) == []
    for t in ts:
        assert R.pag_scale_at(t, 3.0, 0.005) == got[ts.index(t)] and R.pag_scale_at(t, 3.0, 0.0) == 3.0


@pytest.mark.parametrize("name,steps,n_evals", [("DDIMScheduler", 6, 6), ("PNDMScheduler", 6, 7), ("DPMSolverMultistepScheduler", 6, 6)])
def test_pag_schedule_has_one_entry_per_model_evaluation(name, steps, n_evals):
    from agenda_amd.config import SchedulerConfig, pag_schedule
    from agenda_amd.inpaint import evaluation_timesteps
    from agenda_amd.scheduler import SCHEDULERS
    sch = SCHEDULERS[name].from_config(SchedulerConfig())
    ts = evaluation_timesteps(sch, steps)
    assert len(ts) == n_evals
    s = pag_schedule(ts, 3.0, 0.004)
    assert len(s) == n_evals and s == [max(0.0, 3.0 - 0.004 * (1000 - t)) for t in ts]
    if name == "PNDMScheduler":
        assert ts[1] == ts[2] and s[1] == s[2]                 # the repeated second timestep is two evaluations
    if name == "DDIMScheduler":                                # img2img: the strength-truncated tail
        assert pag_schedule(evaluation_timesteps(sch, steps, 0.5), 3.0, 0.004) == s[3:]


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _tiny_weights(name="tiny"):
    from agenda_amd import config, synthetic
    cfg = config.CONFIGS[name]()
    return cfg, synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)


@pytest.mark.parametrize("name", ["tiny", "tiny21"])
def test_restated_forward_without_layers_is_the_oracle_forward(name):
    from agenda_amd import config, synthetic
    from oracle import sd_oracle as O
    cfg, u = _tiny_weights(name)
    ctx = synthetic.make_context(cfg, 1, seed=6)
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3))     # (the mid block runs 2 x 2 tokens: one token alone is its own identity)
    t = torch.tensor(301.0)
    with torch.no_grad():
        want = O.unet_forward(u, cfg.unet, x, t, ctx)
        assert torch.equal(R.unet_forward_perturbed(u, cfg.unet, x, t, ctx, []), want)
        mid = R.unet_forward_perturbed(u, cfg.unet, x, t, ctx, config.resolve_pag_layers(cfg, ["mid"]))
        every = R.unet_forward_perturbed(u, cfg.unet, x, t, ctx, config.self_attn_layer_names(cfg))
    assert not torch.equal(mid, want) and not torch.equal(every, mid)
    assert torch.isfinite(every).all()


def test_restated_perturbed_block_is_value_then_out_projection():
    """One transformer, by hand: with the identity map the attention output of token n is its own value row, so attn1 is
    to_out(to_v(norm1(h))), and a softmax forced onto the diagonal gives the same."""
    import torch.nn.functional as F
    from oracle import sd_oracle as O
    cfg, u = _tiny_weights()
    pre, C = "mid_block.attentions.0.", cfg.unet.block_out_channels[-1]
    t = pre + "transformer_blocks.0."
    n1 = torch.randn(2, 9, C, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    w = {k: v.double() for k, v in u.items() if k.startswith(t + "attn1.")}
    heads = cfg.unet.num_heads[-1]
    v = O.head_to_batch_dim(F.linear(n1, w[t + "attn1.to_v.weight"]), heads)
    eye = torch.eye(9, dtype=torch.float64).expand(v.shape[0], 9, 9)
    via_map = F.linear(O.batch_to_head_dim(torch.bmm(eye, v), heads), w[t + "attn1.to_out.0.weight"], w[t + "attn1.to_out.0.bias"])
    direct = F.linear(F.linear(n1, w[t + "attn1.to_v.weight"]), w[t + "attn1.to_out.0.weight"], w[t + "attn1.to_out.0.bias"])
    assert torch.equal(via_map, direct)


def test_fold_identity_in_fp64():
    g = torch.Generator().manual_seed(9)
    e_u, e_c, e_p = (torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) for _ in range(3))
    s, p = 7.5, 3.0
    lo, hi = R.fold(e_u, e_c, e_p, p)
    two_way = lo + s * (hi - lo)
    assert torch.allclose(two_way, R.combine(e_u, e_c, e_p, s, p), rtol=1e-12, atol=1e-12)
    # e_p == e_c: d = 0 and both rows are untouched, bit for bit; p = 0 likewise
    lo, hi = R.fold(e_u, e_c, e_c, p)
    assert torch.equal(lo, e_u) and torch.equal(hi, e_c)
    lo, hi = R.fold(e_u, e_c, e_p, 0.0)
    assert torch.equal(lo, e_u) and torch.equal(hi, e_c)


def test_restated_loop_counts_perturbed_evaluations():
    from agenda_amd import config, synthetic
    cfg, u = _tiny_weights()
    v = synthetic.make_vae_weights(cfg, 12, bias_std=0.05, perturb_norm=0.1)
    ctx = synthetic.make_context(cfg, 1, seed=41)
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(2))
    mid = config.resolve_pag_layers(cfg, ["mid"])
    _, plain, n0 = R.generate(u, v, cfg, ctx, lat, 3, "ddim", 7.5, 0.0, 0.0, mid, None)
    from oracle import sd_oracle as O
    _, want = O.generate(u, v, cfg, ctx, lat, 3, 7.5)
    assert n0 == 0 and torch.equal(plain, want)
    _, on, n1 = R.generate(u, v, cfg, ctx, lat, 3, "ddim", 7.5, 3.0, 0.0, mid, None)
    assert n1 == 3 and not torch.equal(on, plain)
    # ddim x 3 evaluates t = 667, 334, 1: an adaptive scale of 0.006 leaves 3 - 0.006 * 333 > 0 at the first evaluation only
    _, _, n2 = R.generate(u, v, cfg, ctx, lat, 3, "ddim", 7.5, 3.0, 0.006, mid, None)
    assert n2 == 1


# ---- validation and refusals raised before any device work ----------------------------------------------------------------------
def test_check_pag():
    from agenda_amd.pipeline import check_pag
    check_pag(0.0, 0.0)
    check_pag(3.0, 0.0)
    check_pag(3.0, 0.01)
    check_pag(0.0, 0.0, 0.7)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pag_scale"):
            check_pag(bad, 0.0)
        with pytest.raises(ValueError, match="pag_adaptive_scale"):
            check_pag(3.0, bad)
    with pytest.raises(ValueError, match="needs pag_scale > 0"):
        check_pag(0.0, 0.01)
    with pytest.raises(ValueError, match="guidance_rescale"):
        check_pag(3.0, 0.0, 0.7)


def test_base_pipeline_validates_before_any_device_work():
    from agenda_amd import StableDiffusionPipeline
    stand_in = SimpleNamespace(_refuse_inpainting_unet=lambda: None)      # (anything past the checks would need an engine)
    for kw, msg in (({"pag_scale": -1.0}, "pag_scale"), ({"pag_scale": float("nan")}, "pag_scale"),
                    ({"pag_adaptive_scale": 0.01}, "needs pag_scale > 0"), ({"pag_scale": 3.0, "pag_adaptive_scale": -0.1}, "pag_adaptive_scale"),
                    ({"pag_scale": 3.0, "guidance_rescale": 0.7}, "guidance_rescale")):
        with pytest.raises(ValueError, match=msg):
            StableDiffusionPipeline.__call__(stand_in, prompt="x", **kw)
        with pytest.raises(ValueError, match=msg):
            StableDiffusionPipeline.img2img(stand_in, prompt="x", image=torch.zeros(1, 3, 64, 64), **kw)


@pytest.mark.parametrize("sub", ["StableDiffusionControlNetPipeline", "StableDiffusionAdapterPipeline", "StableDiffusionGLIGENPipeline",
                                 "StableDiffusionInpaintPipeline", "StableDiffusionInstructPix2PixPipeline", "StableDiffusionPanoramaPipeline"])
def test_other_pipelines_refuse_pag_by_name(sub):
    import inspect
    import agenda_amd
    cls = getattr(agenda_amd, sub)
    sig = inspect.signature(cls.__call__).parameters
    assert sig["pag_scale"].default == 0.0 and sig["pag_adaptive_scale"].default == 0.0
    for kw in ({"pag_scale": 3.0}, {"pag_scale": 3.0, "pag_adaptive_scale": 0.01}, {"pag_adaptive_scale": 0.01}):
        with pytest.raises(ValueError, match=f"not implemented for {sub}"):
            cls.__call__(SimpleNamespace(), prompt="x", **kw)


def test_set_pag_applied_layers_on_a_stand_in():
    from agenda_amd import StableDiffusionPipeline, config
    p = SimpleNamespace(cfg=config.tiny())
    StableDiffusionPipeline.set_pag_applied_layers(p, "mid")
    assert p.pag_applied_layers == ["mid"] and p._pag_layers == ["mid_block.attentions.0.transformer_blocks.0.attn1"]
    StableDiffusionPipeline.set_pag_applied_layers(p, ["mid", "up_blocks.1"])
    assert len(p._pag_layers) == 1 + config.tiny().unet.layers_per_block + 1
    with pytest.raises(ValueError, match="nowhere"):
        StableDiffusionPipeline.set_pag_applied_layers(p, ["nowhere"])
    assert p.pag_applied_layers == ["mid", "up_blocks.1"]                # a refused set leaves the previous layers


def test_generation_cli_flags():
    from agenda_amd import generation
    a = generation.parse_args([])
    assert a.pag_scale == 0.0 and a.pag_adaptive_scale == 0.0 and a.pag_applied_layers is None
    a = generation.parse_args(["--pag-scale", "3", "--pag-adaptive-scale", "0.005", "--pag-applied-layers", "mid", "up_blocks.1",
                               "--freeu", "0.9", "0.2", "1.5", "1.6", "--scheduler", "PNDMScheduler", "--height", "128", "--width", "192"])
    assert a.pag_scale == 3.0 and a.pag_adaptive_scale == 0.005 and a.pag_applied_layers == ["mid", "up_blocks.1"]
    assert generation.parse_args(["--pag-scale", "3", "--lora-path", "x"]).pag_scale == 3.0
    for bad in (["--pag-scale", "-1"], ["--pag-scale", "nan"], ["--pag-scale"], ["--pag-adaptive-scale", "0.01"],
                ["--pag-applied-layers", "mid"], ["--pag-scale", "3", "--pag-adaptive-scale", "-1"],
                ["--pag-scale", "3", "--panorama", "--synthetic-config", "tiny"],
                ["--pag-scale", "3", "--guidance-rescale", "0.7"],
                ["--pag-scale", "3", "--instruct-image", "a.png"],
                ["--pag-scale", "3", "--init-image", "a.png", "--mask-image", "m.png"],
                ["--pag-scale", "3", "--controlnet-model-path", "cn", "--control-image", "a.png"],
                ["--pag-scale", "3", "--adapter-model-path", "ad", "--adapter-image", "a.png"],
                ["--pag-scale", "3", "--ip-adapter-path", "ip", "--ip-adapter-image", "a.png"],
                ["--pag-scale", "3", "--gligen-phrases", "a car", "--gligen-boxes", "0.1", "0.1", "0.5", "0.5"]):
        with pytest.raises(SystemExit):
            generation.parse_args(bad)


# ---- surface --------------------------------------------------------------------------------------------------------------------
PAG_SYMBOLS = ("agd_pag_set", "agd_pag_clear", "agd_pag_counts", "agd_op_pag_v_rows", "agd_op_pag_fold")


def test_library_exports_every_pag_symbol():
    import ctypes
    from agenda_amd import _lib
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    for s in PAG_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/agenda_hip.h"
        assert s in _lib.EXPORTS
    # the header's parameter counts are the ctypes signatures'
    for s in PAG_SYMBOLS:
        m = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, s
        assert len(m.group(1).split(",")) == len(_lib._SIGS[s][1]), s


def test_python_surface():
    import inspect
    import agenda_amd
    from agenda_amd import config, ops, pipeline
    for name in ("pag_set", "pag_clear", "pag_counts"):
        assert callable(getattr(pipeline.Engine, name))
    assert callable(ops.pag_v_rows) and callable(ops.pag_fold)
    assert callable(config.self_attn_layer_names) and callable(config.pag_schedule)
    P = pipeline.StableDiffusionPipeline
    for f in (P.__call__, P.img2img):
        sig = inspect.signature(f).parameters
        assert sig["pag_scale"].default == 0.0 and sig["pag_adaptive_scale"].default == 0.0
    assert agenda_amd.StableDiffusionPAGPipeline is P                    # diffusers' name, the same class
    assert "pag_applied_layers" in inspect.signature(P.__init__).parameters
    assert tuple(inspect.signature(P.__init__).parameters["pag_applied_layers"].default) == ("mid",)
    assert callable(P.set_pag_applied_layers) and callable(P._pag)
