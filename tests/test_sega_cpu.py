"""Semantic Guidance off the device: config.sega_schedule against the scalars the tensor restatement (tests/_sega_restated.py) amounts
to, the restated quantile, the argument refusals of every pipeline, the CLI flags, and the C ABI's new symbols."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _sega_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(x):
    return float(np.float32(x))


# (n, K, keywords): no concept warmed / some / all, cooled down (one and every concept), scalars against lists, reversed directions, weights
SCHEDULES = [
    (6, 2, dict(edit_warmup_steps=[1, 3], edit_cooldown_steps=[None, 5])),
    (5, 1, dict()),                                                                   # warm-up 10 > n: never warmed, momentum only
    (12, 1, dict(edit_warmup_steps=10)),
    (8, 3, dict(edit_warmup_steps=[0, 2, 4], edit_cooldown_steps=[3, 6, None], edit_weights=[1.0, 2.0, 0.5], edit_guidance_scale=[5, 7.5, 3],
                reverse_editing_direction=[False, True, False], edit_threshold=[0.9, 0.95, 0.5])),
    (7, 2, dict(edit_warmup_steps=2, edit_cooldown_steps=4, reverse_editing_direction=True, edit_guidance_scale=6.5)),   # all cooled from 4 on
    (4, 8, dict(edit_warmup_steps=0, edit_weights=[0.1 * k for k in range(8)])),
]


@pytest.mark.parametrize("n,K,kw", SCHEDULES, ids=[f"n{c[0]}-K{c[1]}" for c in SCHEDULES])
def test_schedule_is_what_the_restated_tensors_amount_to(n, K, kw):
    from agenda_amd.config import sega_schedule
    s = sega_schedule(n, K, **kw)
    assert s["concepts"] == K and s["n_evals"] == n and s["folds"] == n
    assert s["q"] == [float(x) for x in R.per_concept(kw.get("edit_threshold"), K, 0.9)]
    sg = R.Sega(K, **kw)
    g = torch.Generator().manual_seed(n * 10 + K)
    for i in range(n):
        e_u = torch.randn(1, 4, 4, 4, generator=g, dtype=torch.float64)
        sg.step(i, e_u, [torch.randn(1, 4, 4, 4, generator=g, dtype=torch.float64) for _ in range(K)])
        L = sg.last
        assert s["coef"][i] == L["coef"], (i, s["coef"][i], L["coef"])
        assert s["add_mom"][i] == L["add_mom"]
        for key in ("w_mom", "w_add"):
            assert all(v == _f32(v) for v in s[key][i])                                  # rounded to fp32
            assert s[key][i] == pytest.approx(L[key], rel=0, abs=2 ** -23), (i, key)
    assert s["walks"] == sg.walks
    # the three cases by their definition
    warm = R.per_concept(kw.get("edit_warmup_steps"), K, 10)
    for i in range(n):
        W = [k for k in range(K) if i >= warm[k]]
        assert abs(sum(s["w_mom"][i]) - 1.0) < 1e-6
        if len(W) == K:
            assert s["w_add"][i] == s["w_mom"][i] and s["add_mom"][i] == 1.0
        elif not W:
            assert s["w_add"][i] == [0.0] * K and s["add_mom"][i] == 0.0
        else:
            assert s["add_mom"][i] == 0.0 and abs(sum(s["w_add"][i]) - 1.0) < 1e-6 and all(s["w_add"][i][k] == 0.0 for k in range(K) if k not in W)


def test_scalars_are_lists_of_equal_entries():
    from agenda_amd.config import sega_schedule
    a = sega_schedule(9, 3, edit_guidance_scale=4, edit_warmup_steps=2, edit_cooldown_steps=7, edit_threshold=0.8, edit_weights=1.5,
                      reverse_editing_direction=True)
    b = sega_schedule(9, 3, edit_guidance_scale=[4] * 3, edit_warmup_steps=[2] * 3, edit_cooldown_steps=[7] * 3, edit_threshold=[0.8] * 3,
                      edit_weights=[1.5] * 3, reverse_editing_direction=[True] * 3)
    assert a == b and a["coef"][0] == [-4.0] * 3 and a["coef"][7] == [0.0] * 3 and a["walks"] == 7


@pytest.mark.parametrize("name,steps,n_evals", [("DDIMScheduler", 6, 6), ("PNDMScheduler", 6, 7), ("DPMSolverMultistepScheduler", 6, 6)])
def test_schedule_has_one_row_per_model_evaluation(name, steps, n_evals):
    """PNDM's extra evaluation has its own index; img2img counts along its shortened grid."""
    from agenda_amd import scheduler as S
    from agenda_amd.config import SchedulerConfig, sega_schedule
    from agenda_amd.inpaint import evaluation_timesteps
    sch = getattr(S, name).from_config(SchedulerConfig())
    n = len(evaluation_timesteps(sch, steps))
    assert n == n_evals
    s = sega_schedule(n, 2, edit_warmup_steps=[1, n - 1])
    assert len(s["coef"]) == len(s["w_mom"]) == len(s["w_add"]) == len(s["add_mom"]) == n
    assert s["add_mom"] == [0.0] * (n - 1) + [1.0]
    if name == "DDIMScheduler":
        assert len(evaluation_timesteps(sch, 10, 0.5)) == 5


def test_schedule_refusals_name_the_argument():
    from agenda_amd.config import sega_schedule
    for kw, msg in ((dict(edit_threshold=1.5), "edit_threshold"), (dict(edit_threshold=[0.9, -0.1]), "edit_threshold"),
                    (dict(edit_guidance_scale=[5, 5, 5]), "edit_guidance_scale has 3 entries"), (dict(edit_warmup_steps=[1]), "edit_warmup_steps"),
                    (dict(edit_cooldown_steps=[1, 2, 3]), "edit_cooldown_steps"), (dict(edit_weights=[1.0]), "edit_weights"),
                    (dict(reverse_editing_direction=[True]), "reverse_editing_direction"), (dict(edit_guidance_scale=float("nan")), "edit_guidance_scale"),
                    (dict(edit_warmup_steps=-1), "edit_warmup_steps"), (dict(edit_threshold=float("nan")), "edit_threshold")):
        with pytest.raises(ValueError, match=msg):
            sega_schedule(4, 2, **kw)
    with pytest.raises(ValueError, match="editing concepts"):
        sega_schedule(4, 9)
    with pytest.raises(ValueError, match="n_evaluations"):
        sega_schedule(0, 1)


def test_restated_quantile_is_the_order_statistic_lerp():
    g = torch.Generator().manual_seed(4)
    x = torch.rand(3, 4, 81, generator=g, dtype=torch.float64)
    for q in (0.0, 0.5, 0.9, 0.95, 1.0):
        thr, a, b, f = R.quantile(x, q)
        assert torch.allclose(thr, torch.quantile(x, q, dim=-1), rtol=0, atol=1e-7)       # (f is rounded to fp32)
        assert (a <= thr).all() and (thr <= b).all()
    assert R.rank(0.0, 1) == (0, 0.0) and R.rank(1.0, 64) == (63, 0.0) and R.rank(0.5, 64) == (31, 0.5)
    t = torch.tensor([[1.0, 1.0, 1.0, 2.0]], dtype=torch.float64)
    assert float(R.quantile(t, 0.5)[0]) == 1.0                                         # a == b: thr is a exactly


def test_restated_step_momentum_and_warmup():
    """K = 1 by hand: before warm-up nothing is added but the momentum builds; from warm-up on added = G + mu m."""
    g = torch.Generator().manual_seed(1)
    sg = R.Sega(1, edit_guidance_scale=2.0, edit_warmup_steps=1, edit_threshold=0.0, edit_momentum_scale=0.3, edit_mom_beta=0.4)
    e_u, e_k = (torch.randn(1, 4, 3, 3, generator=g, dtype=torch.float64) for _ in range(2))
    v = (e_k - e_u) * 2.0
    assert torch.equal(sg.step(0, e_u, [e_k]), torch.zeros_like(e_u))
    assert torch.allclose(sg.m, 0.6 * v)
    added = sg.step(1, e_u, [e_k])
    assert torch.allclose(added, v + 0.3 * 0.6 * v)


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def test_check_sega():
    from agenda_amd.pipeline import check_sega
    assert check_sega() is None and check_sega(edit_guidance_scale=7) is None
    s = check_sega("cars")
    assert s["K"] == 1 and s["prompts"] == ["cars"] and s["mu"] == 0.1 and s["beta"] == 0.4
    s = check_sega(["cars", "trees"], reverse_editing_direction=[False, True], edit_threshold=[0.9, 0.95])
    assert s["K"] == 2 and s["args"]["reverse_editing_direction"] == [False, True]
    assert check_sega(editing_prompt_embeddings=torch.zeros(3, 77, 32))["K"] == 3
    for kw, msg in ((dict(editing_prompt="a", editing_prompt_embeddings=torch.zeros(1, 77, 32)), "editing_prompt and editing_prompt_embeddings"),
                    (dict(editing_prompt=["a"] * 9), "editing_prompt: 9 editing concepts"),
                    (dict(editing_prompt_embeddings=torch.zeros(9, 77, 32)), "editing_prompt_embeddings: 9 editing concepts"),
                    (dict(editing_prompt_embeddings=torch.zeros(77, 32)), "editing_prompt_embeddings"),
                    (dict(editing_prompt=["a", "b"], edit_guidance_scale=[5, 5, 5]), "edit_guidance_scale"),
                    (dict(editing_prompt=["a", "b"], edit_warmup_steps=[1]), "edit_warmup_steps"),
                    (dict(editing_prompt=["a", "b"], edit_cooldown_steps=[1]), "edit_cooldown_steps"),
                    (dict(editing_prompt=["a", "b"], edit_threshold=[0.5]), "edit_threshold"),
                    (dict(editing_prompt=["a", "b"], edit_weights=[1.0]), "edit_weights"),
                    (dict(editing_prompt=["a", "b"], reverse_editing_direction=[True]), "reverse_editing_direction"),
                    (dict(editing_prompt="a", edit_threshold=1.01), "edit_threshold"), (dict(editing_prompt="a", edit_threshold=-0.01), "edit_threshold"),
                    (dict(editing_prompt="a", sem_guidance=[torch.zeros(1)]), "sem_guidance"), (dict(sem_guidance=[torch.zeros(1)]), "sem_guidance"),
                    (dict(editing_prompt="a", edit_momentum_scale=float("inf")), "edit_momentum_scale"),
                    (dict(editing_prompt="a", edit_mom_beta=float("nan")), "edit_mom_beta"),
                    (dict(editing_prompt="a", pag_scale=3.0), "pag_scale"), (dict(editing_prompt="a", guidance_rescale=0.7), "guidance_rescale"),
                    (dict(editing_prompt="a", deepcache=(3, 0)), "DeepCache"),
                    (dict(editing_prompt="a", ip_adapter={"scale": 0.5}, ip_adapter_image=object()), "IP-Adapter"),
                    (dict(editing_prompt="a", max_embeddings_multiples=2), "max_embeddings_multiples")):
        with pytest.raises(ValueError, match=msg):
            check_sega(**kw)
    # what leaves the other feature idle is allowed
    assert check_sega("a", deepcache=(1, 0), ip_adapter={"scale": 0.0}, ip_adapter_image=object())["K"] == 1


def test_base_pipeline_validates_before_any_device_work():
    from agenda_amd import StableDiffusionPipeline
    stand_in = SimpleNamespace(_refuse_inpainting_unet=lambda: None)      # (anything past the checks would need an engine)
    for kw, msg in (({"editing_prompt": "a", "editing_prompt_embeddings": torch.zeros(1, 77, 32)}, "both given"),
                    ({"editing_prompt": ["a"] * 9}, "9 editing concepts"), ({"editing_prompt": "a", "edit_threshold": 2.0}, "edit_threshold"),
                    ({"editing_prompt": ["a", "b"], "edit_weights": [1.0, 2.0, 3.0]}, "edit_weights"),
                    ({"editing_prompt": "a", "sem_guidance": [0]}, "sem_guidance"), ({"editing_prompt": "a", "pag_scale": 3.0}, "pag_scale"),
                    ({"editing_prompt": "a", "guidance_rescale": 0.5}, "guidance_rescale"),
                    ({"editing_prompt": "a", "max_embeddings_multiples": 2}, "max_embeddings_multiples")):
        with pytest.raises(ValueError, match=msg):
            StableDiffusionPipeline.__call__(stand_in, prompt="x", **kw)
        with pytest.raises(ValueError, match=msg):
            StableDiffusionPipeline.img2img(stand_in, prompt="x", image=torch.zeros(1, 3, 64, 64), **kw)


def test_context_refuses_long_prompts_and_mismatched_embeddings():
    from agenda_amd import StableDiffusionPipeline as P
    from agenda_amd.pipeline import check_sega
    me = SimpleNamespace()
    sega = check_sega(editing_prompt_embeddings=torch.ones(2, 77, 32))
    assert P._sega_context(me, None, torch.zeros(4, 77, 32), 2) is None
    ctx = P._sega_context(me, sega, torch.zeros(4, 77, 32), 2)
    assert ctx.shape == (8, 77, 32) and float(ctx[:4].abs().max()) == 0 and float(ctx[4:].min()) == 1
    with pytest.raises(ValueError, match="over 96"):
        P._sega_context(me, sega, torch.zeros(4, 152, 32), 2)
    with pytest.raises(ValueError, match="editing_prompt_embeddings of shape"):
        P._sega_context(me, sega, torch.zeros(4, 77, 64), 2)


def test_context_refusals_come_before_any_device_work():
    """On a stand-in with no engine, no IP-Adapter hook-up, no latent draw and no VAE: the refusals are reached in __call__ and img2img, so
    they run before all of those (anything past them would fail on the missing attribute instead)."""
    import types
    from agenda_amd import StableDiffusionPipeline as P
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import DDIMScheduler
    me = SimpleNamespace(_refuse_inpainting_unet=lambda: None, _apply_lora_scale=lambda kw: None, cfg=SimpleNamespace(default_sample_size=16),
                         vae_scale_factor=8, _hooker=None, _trace=None, scheduler=DDIMScheduler.from_config(SchedulerConfig()))
    for n in ("_refuse_rectangular_hook", "_expand_prompts", "_refuse_long_beside", "_sega_context"):
        setattr(me, n, types.MethodType(getattr(P, n), me))
    for kw, msg in ((dict(prompt_embeds=torch.zeros(2, 152, 32), editing_prompt_embeddings=torch.zeros(1, 152, 32)), "over 96"),
                    (dict(prompt_embeds=torch.zeros(2, 77, 32), editing_prompt_embeddings=torch.zeros(1, 50, 32)), "editing_prompt_embeddings of shape")):
        with pytest.raises(ValueError, match=msg):
            P.__call__(me, **kw)
        with pytest.raises(ValueError, match=msg):
            P.img2img(me, image=torch.zeros(1, 3, 128, 128), **kw)
    with pytest.raises(AttributeError, match="_apply_ip_adapter"):       # (and a call that passes them goes on to the device work)
        P.__call__(me, prompt_embeds=torch.zeros(2, 77, 32), editing_prompt_embeddings=torch.zeros(1, 77, 32))


def test_rank_where_the_fraction_rounds_up_to_one():
    """q (HW - 1) in double a few ulp below an integer: lo is the integer below and f = float(p - lo) is exactly 1 (thr = b); valid inputs."""
    for HW, q in ((361, 0.7), (2401, 0.82), (2601, 0.7), (5376, 0.688), (9801, 0.57)):
        lo, f = R.rank(q, HW)
        assert f == 1.0 and lo + 1 == round(q * (HW - 1)), (HW, q, lo, f)
        x = torch.arange(HW, dtype=torch.float64)[None]
        thr, a, b, _ = R.quantile(x, q)
        assert float(thr) == float(b) == lo + 1


@pytest.mark.parametrize("sub", ["StableDiffusionControlNetPipeline", "StableDiffusionAdapterPipeline", "StableDiffusionGLIGENPipeline",
                                 "StableDiffusionInpaintPipeline", "StableDiffusionInstructPix2PixPipeline", "StableDiffusionPanoramaPipeline",
                                 "StableDiffusionRegionPipeline"])
def test_other_pipelines_refuse_the_arguments_by_name(sub):
    import inspect
    import agenda_amd
    cls = getattr(agenda_amd, sub)
    sig = inspect.signature(cls.__call__).parameters
    for name in ("editing_prompt", "editing_prompt_embeddings", "sem_guidance"):
        assert sig[name].default is None
        with pytest.raises(ValueError, match=f"{name}: Semantic Guidance is not implemented for {sub}"):
            cls.__call__(SimpleNamespace(), prompt="x", **{name: ["cars"]})


def test_generation_cli_flags():
    from agenda_amd import generation
    a = generation.parse_args([])
    assert a.editing_prompt is None and a.sega is None
    a = generation.parse_args(["--editing-prompt", "more cars", "no trees", "--reverse-editing-direction", "0", "1", "--edit-guidance-scale", "6",
                               "--edit-warmup-steps", "5", "8", "--edit-cooldown-steps", "40", "--edit-threshold", "0.9", "0.95",
                               "--edit-weights", "1", "2", "--edit-momentum-scale", "0.3", "--edit-mom-beta", "0.6", "--scheduler", "PNDMScheduler"])
    assert a.sega == {"editing_prompt": ["more cars", "no trees"], "reverse_editing_direction": [False, True], "edit_guidance_scale": 6.0,
                      "edit_warmup_steps": [5, 8], "edit_cooldown_steps": 40, "edit_threshold": [0.9, 0.95], "edit_weights": [1.0, 2.0],
                      "edit_momentum_scale": 0.3, "edit_mom_beta": 0.6}
    from agenda_amd.pipeline import check_sega
    assert check_sega(**a.sega)["K"] == 2                                   # the flags are the pipeline's keywords
    assert generation.parse_args(["--editing-prompt", "cars", "--lora-path", "x", "--freeu", "0.9", "0.2", "1.5", "1.6"]).sega == {"editing_prompt": ["cars"]}
    for bad in (["--edit-threshold", "0.5"], ["--edit-momentum-scale", "0.3"], ["--editing-prompt"], ["--editing-prompt"] + ["c"] * 9,
                ["--editing-prompt", "a", "b", "--edit-threshold", "0.5", "0.6", "0.7"], ["--editing-prompt", "a", "--edit-threshold", "1.5"],
                ["--editing-prompt", "a", "--reverse-editing-direction", "2"], ["--editing-prompt", "a", "--edit-mom-beta", "nan"],
                ["--editing-prompt", "a", "--pag-scale", "3"], ["--editing-prompt", "a", "--guidance-rescale", "0.7"],
                ["--editing-prompt", "a", "--deepcache-interval", "3"], ["--editing-prompt", "a", "--max-embeddings-multiples", "2"],
                ["--editing-prompt", "a", "--panorama", "--synthetic-config", "tiny"], ["--editing-prompt", "a", "--instruct-image", "a.png"],
                ["--editing-prompt", "a", "--init-image", "a.png", "--mask-image", "m.png"],
                ["--editing-prompt", "a", "--controlnet-model-path", "cn", "--control-image", "a.png"],
                ["--editing-prompt", "a", "--adapter-model-path", "ad", "--adapter-image", "a.png"],
                ["--editing-prompt", "a", "--ip-adapter-path", "ip", "--ip-adapter-image", "a.png"],
                ["--editing-prompt", "a", "--gligen-phrases", "a car", "--gligen-boxes", "0.1", "0.1", "0.5", "0.5"]):
        with pytest.raises(SystemExit):
            generation.parse_args(bad)


# ---- surface --------------------------------------------------------------------------------------------------------------------
SEGA_SYMBOLS = ("agd_sega_set", "agd_sega_clear", "agd_sega_counts", "agd_op_sega_threshold", "agd_op_sega_fold")


def test_library_exports_every_sega_symbol():
    import ctypes
    from agenda_amd import _lib
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    for s in SEGA_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert s in _lib.EXPORTS
        m = re.search(r"\bint\s+" + s + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{s} not declared in include/agenda_hip.h"
        assert len(m.group(1).split(",")) == len(_lib._SIGS[s][1]), s        # the header's parameter counts are the ctypes signatures'
    assert re.search(r"#define\s+AGD_MAX_EDIT_CONCEPTS\s+8\b", txt) and _lib.AGD_MAX_EDIT_CONCEPTS == 8
    fields = re.search(r"typedef struct agd_sega_desc \{(.*?)\} agd_sega_desc;", txt, re.S).group(1)
    for name, _ in _lib.AgdSegaDesc._fields_:
        assert re.search(r"\b" + name + r"\b", fields), name


def test_python_surface():
    import inspect
    import agenda_amd
    from agenda_amd import config, ops, pipeline
    for name in ("sega_set", "sega_clear", "sega_counts"):
        assert callable(getattr(pipeline.Engine, name))
    assert callable(ops.sega_threshold) and callable(ops.sega_fold) and callable(config.sega_schedule)
    P = pipeline.StableDiffusionPipeline
    want = {"editing_prompt": None, "editing_prompt_embeddings": None, "reverse_editing_direction": False, "edit_guidance_scale": 5,
            "edit_warmup_steps": 10, "edit_cooldown_steps": None, "edit_threshold": 0.9, "edit_momentum_scale": 0.1, "edit_mom_beta": 0.4,
            "edit_weights": None}
    for f in (P.__call__, P.img2img):
        sig = inspect.signature(f).parameters
        for k, d in want.items():
            assert sig[k].default == d or (d is None and sig[k].default is None), k
    assert agenda_amd.SemanticStableDiffusionPipeline is P                   # diffusers' name, the same class
    assert callable(P._sega)
