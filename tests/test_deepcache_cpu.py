"""DeepCache without a GPU: the uniform schedule under the three schedulers, argument validation and every refusal raised before any device
work, the upstream-shaped helper, the restatement's own invariants (tests/_deepcache_restated.py), the CLI flags and the C ABI's new symbols."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import _deepcache_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
def test_deepcache_schedule_values():
    from agenda_amd.config import deepcache_schedule
    assert deepcache_schedule(7, 3) == [1, 0, 0, 1, 0, 0, 1]
    assert deepcache_schedule(5, 2) == [1, 0, 1, 0, 1]
    assert deepcache_schedule(4, 1) == [1, 1, 1, 1]
    assert deepcache_schedule(3, 10) == [1, 0, 0]
    assert deepcache_schedule(1, 3) == [1]
    for n, k in ((7, 3), (50, 5), (20, 2)):
        assert deepcache_schedule(n, k) == [int(f) for f in R.schedule(n, k)]
        assert deepcache_schedule(n, k)[0] == 1
    for bad in (0, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="cache_interval"):
            deepcache_schedule(5, bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="n_evaluations"):
            deepcache_schedule(bad, 3)


@pytest.mark.parametrize("name,steps,n_evals", [("DDIMScheduler", 6, 6), ("PNDMScheduler", 6, 7), ("DPMSolverMultistepScheduler", 6, 6)])
def test_schedule_has_one_flag_per_model_evaluation(name, steps, n_evals):
    """Flags count model evaluations from 0, not timesteps: PNDM's repeated timestep is two evaluations, img2img counts its own tail."""
    from agenda_amd.config import SchedulerConfig, deepcache_schedule
    from agenda_amd.inpaint import evaluation_timesteps
    from agenda_amd.scheduler import SCHEDULERS
    sch = SCHEDULERS[name].from_config(SchedulerConfig())
    n = len(evaluation_timesteps(sch, steps))
    assert n == n_evals
    assert deepcache_schedule(n, 3) == [1, 0, 0, 1, 0, 0, 1][:n]
    if name == "DDIMScheduler":
        tail = evaluation_timesteps(sch, steps, 0.5)
        assert len(tail) == 3 and deepcache_schedule(len(tail), 2) == [1, 0, 1]           # (not a slice of the full call's flags)


# ---- validation and refusals raised before any device work ----------------------------------------------------------------------
def test_check_deepcache():
    from agenda_amd.pipeline import check_deepcache
    check_deepcache(1, 0, 2)
    check_deepcache(3, 1, 2)
    check_deepcache(5, 0, 1)
    for bad in (0, -2):
        with pytest.raises(ValueError, match=f"cache_interval={bad}"):
            check_deepcache(bad, 0, 2)
    for bad in (2.0, "3", None, True):
        with pytest.raises(ValueError, match=re.escape(f"cache_interval={bad!r}")):
            check_deepcache(bad, 0, 2)
    with pytest.raises(ValueError, match=re.escape("cache_branch_id=1.0")):
        check_deepcache(3, 1.0, 2)
    for bad, lpb in ((2, 2), (-1, 2), (1, 1), (3, 2)):
        with pytest.raises(ValueError, match=f"cache_branch_id={bad}: this UNet has branches 0 .. {lpb - 1}"):
            check_deepcache(3, bad, lpb)
    with pytest.raises(ValueError, match="skip_mode='pow'"):
        check_deepcache(3, 0, 2, "pow")


def test_enable_and_disable_on_a_stand_in():
    from agenda_amd import StableDiffusionPipeline, config
    p = SimpleNamespace(cfg=config.tiny(), _deepcache=None)
    StableDiffusionPipeline.enable_deepcache(p)
    assert p._deepcache == (3, 0)                                        # the documented defaults
    StableDiffusionPipeline.enable_deepcache(p, cache_interval=2, cache_branch_id=1)
    assert p._deepcache == (2, 1)
    for kw, msg in (({"cache_interval": 0}, "cache_interval=0"), ({"cache_interval": 2.5}, "cache_interval=2.5"),
                    ({"cache_branch_id": 2}, "cache_branch_id=2"), ({"skip_mode": "center"}, "skip_mode='center'")):
        with pytest.raises(ValueError, match=msg):
            StableDiffusionPipeline.enable_deepcache(p, **kw)
    assert p._deepcache == (2, 1)                                        # a refused enable leaves the previous state
    p40 = SimpleNamespace(cfg=config.tiny40(), _deepcache=None)
    with pytest.raises(ValueError, match="cache_branch_id=1: this UNet has branches 0 .. 0"):
        StableDiffusionPipeline.enable_deepcache(p40, cache_branch_id=1)
    StableDiffusionPipeline.disable_deepcache(p)
    assert p._deepcache is None


def test_helper_forwards_to_the_pipeline():
    import agenda_amd
    from agenda_amd import DeepCacheSDHelper, StableDiffusionPipeline, config
    assert agenda_amd.DeepCacheSDHelper is agenda_amd.pipeline.DeepCacheSDHelper
    calls = []
    p = SimpleNamespace(cfg=config.tiny(), _deepcache=None)
    p.enable_deepcache = lambda **kw: (calls.append(kw), StableDiffusionPipeline.enable_deepcache(p, **kw))
    p.disable_deepcache = lambda: StableDiffusionPipeline.disable_deepcache(p)
    h = DeepCacheSDHelper(pipe=p)
    h.set_params(cache_interval=3, cache_branch_id=0)
    assert p._deepcache is None                                          # set_params alone enables nothing
    h.enable()
    assert p._deepcache == (3, 0) and calls == [dict(cache_interval=3, cache_branch_id=0, skip_mode="uniform")]
    h.disable()
    assert p._deepcache is None
    for kw, msg in (({"cache_interval": 0}, "cache_interval=0"), ({"cache_interval": 3, "cache_branch_id": 5}, "cache_branch_id=5"),
                    ({"cache_interval": 3, "skip_mode": "pow"}, "skip_mode='pow'")):
        with pytest.raises(ValueError, match=msg):
            h.set_params(**kw)


def test_refuse_deepcache():
    from agenda_amd.pipeline import refuse_deepcache
    refuse_deepcache("X", None)
    refuse_deepcache("X", (1, 0))                                        # interval 1 sets nothing
    with pytest.raises(ValueError, match=r"DeepCache \(cache_interval=3, cache_branch_id=1\) is enabled: it is not implemented for X;? "):
        refuse_deepcache("X", (3, 1))
    with pytest.raises(ValueError, match="not implemented for X with pag_scale=3.0"):
        refuse_deepcache("X", (2, 0), "pag_scale=3.0")


@pytest.mark.parametrize("sub", ["StableDiffusionControlNetPipeline", "StableDiffusionAdapterPipeline", "StableDiffusionGLIGENPipeline",
                                 "StableDiffusionInpaintPipeline", "StableDiffusionInstructPix2PixPipeline", "StableDiffusionPanoramaPipeline"])
def test_other_pipelines_refuse_deepcache_by_name(sub):
    import agenda_amd
    cls = getattr(agenda_amd, sub)
    with pytest.raises(ValueError, match=f"DeepCache .* not implemented for {sub}"):
        cls.__call__(SimpleNamespace(_deepcache=(3, 0)), prompt="x")


def test_base_pipeline_refuses_pag_beside_deepcache_before_any_device_work():
    from agenda_amd import StableDiffusionPipeline
    stand_in = SimpleNamespace(_refuse_inpainting_unet=lambda: None, _deepcache=(3, 0))
    with pytest.raises(ValueError, match="DeepCache .* not implemented for StableDiffusionPipeline with pag_scale=3.0"):
        StableDiffusionPipeline.__call__(stand_in, prompt="x", pag_scale=3.0)
    with pytest.raises(ValueError, match="DeepCache .* not implemented for StableDiffusionPipeline with pag_scale=3.0"):
        StableDiffusionPipeline.img2img(stand_in, prompt="x", image=torch.zeros(1, 3, 64, 64), pag_scale=3.0)


def test_base_pipeline_refuses_an_active_ip_adapter_beside_deepcache_before_any_device_work():
    """Decided from the arguments and the loaded adapter's scale, right after the argument checks: an image prompt (an image or embeddings)
    for an adapter whose scale is not 0 is refused by name; scale 0, no image prompt, interval 1 and a disabled DeepCache are not -- those
    calls go on to the first thing a stand-in lacks."""
    from agenda_amd import StableDiffusionPipeline
    from agenda_amd.pipeline import refuse_deepcache_beside
    past = "reached the LoRA step"                                       # the first call after the checks

    def stand_in(deepcache, scale):
        def lora(kw):
            raise RuntimeError(past)
        return SimpleNamespace(_refuse_inpainting_unet=lambda: None, _deepcache=deepcache, _apply_lora_scale=lora,
                               _ip_adapter=None if scale is None else {"scale": scale, "embed_dim": 8})
    emb, img = torch.zeros(2, 8), torch.zeros(1, 3, 64, 64)
    calls = (lambda s, **kw: StableDiffusionPipeline.__call__(s, prompt="x", **kw),
             lambda s, **kw: StableDiffusionPipeline.img2img(s, prompt="x", image=img, **kw))
    for call in calls:
        for kw in ({"ip_adapter_image_embeds": emb}, {"ip_adapter_image": img}):
            with pytest.raises(ValueError, match=r"DeepCache \(cache_interval=3, cache_branch_id=0\) .* with an active IP-Adapter \(scale 0.6\)"):
                call(stand_in((3, 0), 0.6), **kw)
            for dc, scale in (((3, 0), 0.0), ((1, 0), 0.6), (None, 0.6), ((3, 0), None)):      # idle adapter, interval 1, disabled, none loaded
                with pytest.raises(RuntimeError, match=past):
                    call(stand_in(dc, scale), **kw)
        with pytest.raises(RuntimeError, match=past):                    # a loaded adapter without an image prompt is left idle
            call(stand_in((3, 0), 0.6))
    refuse_deepcache_beside(None, 3.0, {"scale": 1.0}, img, None)
    refuse_deepcache_beside((2, 1), 0.0, {"scale": 1.0}, None, None)
    with pytest.raises(ValueError, match="with pag_scale=3.0"):          # the pag_scale refusal comes first
        refuse_deepcache_beside((2, 1), 3.0, {"scale": 1.0}, img, None)


def test_loop_context_manager_sets_and_clears_on_an_error_too():
    from agenda_amd import StableDiffusionPipeline
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import SCHEDULERS
    log = []
    eng = SimpleNamespace(deepcache_set=lambda flags, branch: log.append(("set", list(flags), branch)), deepcache_clear=lambda: log.append(("clear",)))
    p = SimpleNamespace(engine=eng, _deepcache=None)
    pndm = SCHEDULERS["PNDMScheduler"].from_config(SchedulerConfig())
    ddim = SCHEDULERS["DDIMScheduler"].from_config(SchedulerConfig())
    with StableDiffusionPipeline._deepcached(p, pndm, 4):
        pass
    p._deepcache = (1, 0)
    with StableDiffusionPipeline._deepcached(p, pndm, 4):
        pass
    assert log == []                                                     # disabled, and interval 1: nothing is set in the engine
    p._deepcache = (2, 1)
    with StableDiffusionPipeline._deepcached(p, pndm, 4):                # PNDM x 4 steps: five evaluations
        assert log == [("set", [1, 0, 1, 0, 1], 1)]
    assert log[-1] == ("clear",)
    del log[:]
    with pytest.raises(RuntimeError, match="boom"):
        with StableDiffusionPipeline._deepcached(p, ddim, 6, 0.5):       # img2img, strength 0.5 of 6 steps: three evaluations
            raise RuntimeError("boom")
    assert log == [("set", [1, 0, 1], 1), ("clear",)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _tiny_weights(name="tiny"):
    from agenda_amd import config, synthetic
    cfg = config.CONFIGS[name]()
    return cfg, synthetic.make_unet_weights(cfg, 11, bias_std=0.05, perturb_norm=0.1)


@pytest.mark.parametrize("name,branches", [("tiny", (0, 1)), ("tiny21", (0,))])
def test_restated_full_is_the_oracle_and_shallow_after_full_repeats_it(name, branches):
    from agenda_amd import synthetic
    from oracle import sd_oracle as O
    cfg, u = _tiny_weights(name)
    ctx = synthetic.make_context(cfg, 1, seed=6)
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    t = torch.tensor(301.0)
    with torch.no_grad():
        want = O.unet_forward(u, cfg.unet, x, t, ctx)
        assert torch.equal(R.unet_forward(u, cfg.unet, x, t, ctx), want)
        for b in branches:
            cache, calls_full, calls_sh = {}, [], []
            full = R.unet_forward(u, cfg.unet, x, t, ctx, "full", b, cache, lambda p, nh, nm: calls_full.append(nm))
            assert torch.equal(full, want) and "h" in cache
            sh = R.unet_forward(u, cfg.unet, x, t, ctx, "shallow", b, cache, lambda p, nh, nm: calls_sh.append(nm))
            assert torch.equal(sh, want)                                 # the same operations on the same inputs
            nl, lpb = len(cfg.unet.block_out_channels), cfg.unet.layers_per_block
            assert calls_sh == ([f"down_blocks.0.attentions.{j}.transformer_blocks.0.attn2" for j in range(b + 1)] +
                                [f"up_blocks.{nl - 1}.attentions.{j}.transformer_blocks.0.attn2" for j in range(lpb - b - 1, lpb + 1)])
            assert len(calls_sh) == R.shallow_attn2_layers(cfg.unet, b) and set(calls_sh) < set(calls_full)
            # at another input the cached features are stale: the shallow result moves away from the full one, and is finite
            x2 = x + 0.3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(4))
            sh2 = R.unet_forward(u, cfg.unet, x2, torch.tensor(281.0), ctx, "shallow", b, cache)
            full2 = R.unet_forward(u, cfg.unet, x2, torch.tensor(281.0), ctx)
            assert torch.isfinite(sh2).all() and not torch.equal(sh2, full2)


def test_restated_generate_counts_and_interval_1():
    from agenda_amd import config, synthetic
    from oracle import sd_oracle as O
    cfg, u = _tiny_weights()
    v = synthetic.make_vae_weights(cfg, 12, bias_std=0.05, perturb_norm=0.1)
    ctx = synthetic.make_context(cfg, 1, seed=6)
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3))
    img1, x1, c1 = R.generate(u, v, cfg, ctx, lat, 3, "ddim")
    assert c1 == (0, 0)
    _, x3, c3 = R.generate(u, v, cfg, ctx, lat, 3, "pndm", cache_interval=3)      # four evaluations: F S S F
    assert c3 == (1, 2)
    _, x2, c2 = R.generate(u, v, cfg, ctx, lat, 3, "ddim", cache_interval=2, branch=1)   # F S F
    assert c2 == (1, 1) and not torch.equal(x2, x1) and torch.isfinite(x2).all()
    # interval 1 is the oracle's own loop
    s = cfg.sched
    sch = O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type)
    with torch.no_grad():
        x = lat.clone()
        for t in sch.set_timesteps(3):
            e_u, e_c = O.unet_forward(u, cfg.unet, torch.cat([x, x]), torch.tensor(float(int(t))), ctx).chunk(2)
            x = sch.step(e_u + 7.5 * (e_c - e_u), int(t), x)
    assert torch.equal(x, x1)


# ---- the CLI --------------------------------------------------------------------------------------------------------------------
def test_generation_cli_flags():
    from agenda_amd import generation
    a = generation.parse_args([])
    assert a.deepcache_interval is None and a.deepcache_branch is None
    a = generation.parse_args(["--deepcache-interval", "3", "--deepcache-branch", "1", "--freeu", "0.9", "0.2", "1.5", "1.6",
                               "--scheduler", "PNDMScheduler", "--height", "128", "--width", "192", "--guidance-rescale", "0.7"])
    assert a.deepcache_interval == 3 and a.deepcache_branch == 1
    assert generation.parse_args(["--deepcache-interval", "2", "--lora-path", "x"]).deepcache_interval == 2
    assert generation.parse_args(["--deepcache-interval", "1", "--pag-scale", "3"]).deepcache_interval == 1      # interval 1 is off
    for bad in (["--deepcache-interval", "0"], ["--deepcache-interval", "-2"], ["--deepcache-interval", "2.5"], ["--deepcache-interval"],
                ["--deepcache-branch", "1"], ["--deepcache-interval", "3", "--deepcache-branch", "-1"],
                ["--deepcache-interval", "3", "--pag-scale", "3"],
                ["--deepcache-interval", "3", "--panorama", "--synthetic-config", "tiny"],
                ["--deepcache-interval", "3", "--instruct-image", "a.png"],
                ["--deepcache-interval", "3", "--init-image", "a.png", "--mask-image", "m.png"],
                ["--deepcache-interval", "3", "--controlnet-model-path", "cn", "--control-image", "a.png"],
                ["--deepcache-interval", "3", "--adapter-model-path", "ad", "--adapter-image", "a.png"],
                ["--deepcache-interval", "3", "--ip-adapter-path", "ip", "--ip-adapter-image", "a.png"],
                ["--deepcache-interval", "3", "--gligen-phrases", "a car", "--gligen-boxes", "0.1", "0.1", "0.5", "0.5"]):
        with pytest.raises(SystemExit):
            generation.parse_args(bad)


# ---- surface --------------------------------------------------------------------------------------------------------------------
DC_SYMBOLS = ("agd_deepcache_set", "agd_deepcache_clear", "agd_deepcache_counts", "agd_deepcache_forward_hw", "agd_op_deepcache_capture")


def test_library_exports_every_deepcache_symbol():
    import ctypes
    from agenda_amd import _lib
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    for s in DC_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        m = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{s} not declared in include/agenda_hip.h"
        assert s in _lib.EXPORTS
        assert len(m.group(1).split(",")) == len(_lib._SIGS[s][1]), s      # the header's parameter count is the ctypes signature's


def test_python_surface():
    import inspect
    from agenda_amd import config, ops, pipeline
    for name in ("deepcache_set", "deepcache_clear", "deepcache_counts", "deepcache_forward"):
        assert callable(getattr(pipeline.Engine, name))
    assert callable(ops.deepcache_capture) and callable(config.deepcache_schedule)
    P = pipeline.StableDiffusionPipeline
    sig = inspect.signature(P.enable_deepcache).parameters
    assert sig["cache_interval"].default == 3 and sig["cache_branch_id"].default == 0
    assert callable(P.disable_deepcache) and callable(P._deepcached)
    assert "deepcache" not in inspect.getsource(P.save_pretrained).lower()          # the state is not written
