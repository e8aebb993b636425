"""guidance_rescale, DDIM's timestep spacings and the zero-terminal-SNR table without a GPU: the grids and the table against
tests/_guidance_restated.py and the values the issue pins, the refusals, the scheduler JSON round trip, the CLI flags and the ABI."""
import json
import os
import re

import numpy as np
import pytest
import torch

import _guidance_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- grids ----------------------------------------------------------------------------------------------------------------------
def test_trailing_grid():
    from agenda_amd.scheduler import DDIMScheduler
    s = DDIMScheduler(timestep_spacing="trailing")
    assert list(s.set_timesteps(50)) == list(range(999, 0, -20)) and s.timesteps[-1] == 19
    assert list(s.set_timesteps(7)) == [999, 856, 713, 570, 428, 285, 142]
    for n in (1, 3, 7, 20, 50, 333, 1000):
        assert np.array_equal(s.set_timesteps(n), R.ddim_grid("trailing", n)), n
        assert s.timesteps[0] == 999 and s.timesteps.dtype == np.int64


def test_linspace_grid():
    from agenda_amd.scheduler import DDIMScheduler
    s = DDIMScheduler(timestep_spacing="linspace")
    for n in (2, 3, 7, 20, 50, 333, 1000):
        ts = s.set_timesteps(n)
        assert ts[0] == 999 and ts[-1] == 0 and len(ts) == n
        assert np.array_equal(ts, R.ddim_grid("linspace", n)), n


def test_leading_grid_is_unchanged():
    from agenda_amd.scheduler import DDIMScheduler
    from oracle import sd_oracle as O
    assert list(DDIMScheduler().set_timesteps(50)[:3]) == [981, 961, 941] and DDIMScheduler().set_timesteps(50)[-1] == 1
    for n in (1, 4, 7, 20, 50, 1000):
        for s in (DDIMScheduler(), DDIMScheduler(timestep_spacing="leading")):
            assert np.array_equal(s.set_timesteps(n), O.DDIM().set_timesteps(n)), n
            assert np.array_equal(s.timesteps, R.ddim_grid("leading", n))


@pytest.mark.parametrize("spacing", ["leading", "trailing", "linspace"])
@pytest.mark.parametrize("n", [4, 7, 50])
def test_prev_t_rule(spacing, n):
    """prev_t = t - T // n whatever the spacing; prev_t < 0 takes final_alpha_cumprod (= alphas_cumprod[0]: set_alpha_to_one False)."""
    from agenda_amd.scheduler import DDIMScheduler
    s = DDIMScheduler(timestep_spacing=spacing)
    ts = s.set_timesteps(n)
    a_t, a_p = s.step_coeffs()
    ac = R.alphas_cumprod().numpy()
    negative = 0
    for i, t in enumerate(ts):
        p = int(t) - 1000 // n
        assert a_t[i] == ac[t]
        assert a_p[i] == (ac[p] if p >= 0 else ac[0]), (spacing, n, i)
        negative += p < 0
    # 1000 // n = 250, 142, 20: linspace ends at t = 0, trailing n = 7 at 142 (prev 0, not negative), leading at 1
    assert negative == {"leading": 1, "linspace": 1, "trailing": 0 if n == 7 else 1}[spacing]
    one = DDIMScheduler(timestep_spacing=spacing, set_alpha_to_one=True)
    one.set_timesteps(n)
    assert (one.step_coeffs()[1] == 1.0).sum() == negative


# ---- zero terminal SNR ----------------------------------------------------------------------------------------------------------
def test_zero_snr_table():
    from agenda_amd.scheduler import DDIMScheduler
    z = DDIMScheduler(rescale_betas_zero_snr=True, prediction_type="v_prediction").alphas_cumprod
    p = DDIMScheduler().alphas_cumprod
    assert z.dtype == np.float32 and z[-1] == 0.0
    assert z[0] == p[0] == np.float32(0.9991499781608582)
    assert (np.diff(z) < 0).all()
    assert np.array_equal(z, R.alphas_cumprod(True).numpy())              # the same float32 operations: bit for bit
    assert np.array_equal(p, R.alphas_cumprod(False).numpy())
    assert p[-1] > 0.004                                                  # (the plain table keeps signal at t = 999)


def test_zero_snr_first_step_is_finite_under_v_prediction():
    from agenda_amd.scheduler import DDIMScheduler
    s = DDIMScheduler(rescale_betas_zero_snr=True, prediction_type="v_prediction", timestep_spacing="trailing")
    s.set_timesteps(4)
    a_t, a_p = s.step_coeffs()
    assert a_t[0] == 0.0 and (a_t[1:] > 0).all() and (a_p > 0).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_epsilon_with_a_zero_alpha_timestep_is_refused():
    from agenda_amd.scheduler import DDIMScheduler
    s = DDIMScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")
    s.set_timesteps(4)
    with pytest.raises(ValueError, match="timestep 999 has alphas_cumprod == 0.*epsilon"):
        s.step_coeffs()
    lead = DDIMScheduler(rescale_betas_zero_snr=True)                     # a leading grid never visits 999: it runs
    lead.set_timesteps(4)
    assert (lead.step_coeffs()[0] > 0).all()


def test_unknown_spacing_is_refused():
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import DDIMScheduler, scheduler_config_from_json
    with pytest.raises(ValueError, match="DDIMScheduler: timestep_spacing 'karras'"):
        DDIMScheduler(timestep_spacing="karras")
    with pytest.raises(ValueError, match="timestep_spacing 'even'"):
        DDIMScheduler.from_config(SchedulerConfig(ddim_timestep_spacing="even"))
    with pytest.raises(ValueError, match="timestep_spacing 'even'"):
        scheduler_config_from_json({"_class_name": "DDIMScheduler", "timestep_spacing": "even"}, "DDIMScheduler")


@pytest.mark.parametrize("spacing", ["trailing", "linspace"])
def test_pndm_runs_leading_only(spacing):
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import PNDMScheduler
    with pytest.raises(ValueError, match=f"PNDMScheduler: only timestep_spacing='leading'.*{spacing}"):
        PNDMScheduler(timestep_spacing=spacing)
    with pytest.raises(ValueError, match="PNDMScheduler: only timestep_spacing='leading'"):
        PNDMScheduler.from_config(SchedulerConfig(ddim_timestep_spacing=spacing))
    assert PNDMScheduler(timestep_spacing="leading").set_timesteps(4) is not None


def test_dpm_refuses_zero_snr():
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import DPMSolverMultistepScheduler, PNDMScheduler
    with pytest.raises(ValueError, match="DPMSolverMultistepScheduler: rescale_betas_zero_snr"):
        DPMSolverMultistepScheduler(rescale_betas_zero_snr=True)
    with pytest.raises(ValueError, match="DPMSolverMultistepScheduler: rescale_betas_zero_snr"):
        DPMSolverMultistepScheduler.from_config(SchedulerConfig(rescale_betas_zero_snr=True))
    with pytest.raises(ValueError, match="PNDMScheduler: rescale_betas_zero_snr"):
        PNDMScheduler(rescale_betas_zero_snr=True)
    # DPM keeps its own spacings, untouched by DDIM's field
    d = DPMSolverMultistepScheduler.from_config(SchedulerConfig(ddim_timestep_spacing="trailing"))
    assert d.timestep_spacing == "linspace"


def test_pipelines_refuse_a_bad_guidance_rescale_on_the_host():
    from agenda_amd.pipeline import check_guidance_rescale
    for ok in (0, 0.0, 0.7, 1, 1.0):
        check_guidance_rescale(ok)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="guidance rescale takes a number in \\[0, 1\\]"):
            check_guidance_rescale(bad)


# ---- JSON -----------------------------------------------------------------------------------------------------------------------
def test_json_round_trip():
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import DDIMScheduler, scheduler_config_from_json, scheduler_config_to_json
    sc = SchedulerConfig(prediction_type="v_prediction", ddim_timestep_spacing="trailing", rescale_betas_zero_snr=True)
    sj = scheduler_config_to_json("DDIMScheduler", sc)
    assert sj["timestep_spacing"] == "trailing" and sj["rescale_betas_zero_snr"] is True
    back = scheduler_config_from_json(json.loads(json.dumps(sj)), "DDIMScheduler")
    assert back == sc
    s = DDIMScheduler.from_config(back)
    assert s.timestep_spacing == "trailing" and s.rescale_betas_zero_snr and s.alphas_cumprod[-1] == 0.0
    # one key alone
    sj = scheduler_config_to_json("DDIMScheduler", SchedulerConfig(ddim_timestep_spacing="linspace"))
    assert sj["timestep_spacing"] == "linspace" and "rescale_betas_zero_snr" not in sj
    assert scheduler_config_from_json(sj, "DDIMScheduler").ddim_timestep_spacing == "linspace"
    # a DDIM checkpoint that says trailing is honoured; the same JSON run under another scheduler keeps that scheduler's defaults
    up = {"_class_name": "DDIMScheduler", "timestep_spacing": "trailing", "rescale_betas_zero_snr": True, "prediction_type": "v_prediction"}
    assert scheduler_config_from_json(up, "DDIMScheduler").ddim_timestep_spacing == "trailing"
    other = scheduler_config_from_json(up, "PNDMScheduler")
    assert other.ddim_timestep_spacing == "leading" and other.rescale_betas_zero_snr is False
    # a PNDM / DPM JSON overridden to DDIM: its spacing key is that scheduler's, not DDIM's
    assert scheduler_config_from_json({"_class_name": "DPMSolverMultistepScheduler", "timestep_spacing": "trailing"},
                                      "DDIMScheduler").ddim_timestep_spacing == "leading"


def test_default_json_is_byte_for_byte_what_it_was():
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import scheduler_config_to_json
    was = ('{"_class_name": "DDIMScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012, '
           '"beta_schedule": "scaled_linear", "steps_offset": 1, "set_alpha_to_one": false, "prediction_type": "epsilon"}')
    assert json.dumps(scheduler_config_to_json("DDIMScheduler", SchedulerConfig())) == was
    # the other two never write DDIM's keys
    for name in ("PNDMScheduler", "DPMSolverMultistepScheduler"):
        sj = scheduler_config_to_json(name, SchedulerConfig())
        assert "rescale_betas_zero_snr" not in sj and sj.get("timestep_spacing", "linspace") == "linspace"
    assert SchedulerConfig().timestep_spacing == "linspace" and SchedulerConfig().ddim_timestep_spacing == "leading"


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
def test_restated_factor_is_rescale_noise_cfg():
    g = torch.Generator().manual_seed(3)
    eu = torch.randn(3, 4, 8, 8, generator=g, dtype=torch.float64)
    ec = eu + 0.3 * torch.randn(3, 4, 8, 8, generator=g, dtype=torch.float64)
    m = eu + 7.5 * (ec - eu)
    f = R.factor(eu, ec, 7.5, 0.7)
    assert torch.allclose(R.rescale_noise_cfg(m, ec, 0.7), f.view(3, 1, 1, 1) * m, rtol=1e-12, atol=0)
    assert ((f > 0.3) & (f <= 1.0)).all()
    assert torch.equal(R.rescale_noise_cfg(m, ec, 0.0), m)


# ---- surface --------------------------------------------------------------------------------------------------------------------
def test_generation_cli_flags():
    from agenda_amd import generation
    a = generation.parse_args([])
    assert a.guidance_rescale == 0.0 and a.timestep_spacing is None and a.rescale_betas_zero_snr is False
    a = generation.parse_args(["--guidance-rescale", "0.7", "--timestep-spacing", "trailing", "--rescale-betas-zero-snr",
                               "--scheduler", "DDIMScheduler", "--freeu", "0.9", "0.2", "1.5", "1.6", "--height", "128", "--width", "192"])
    assert a.guidance_rescale == 0.7 and a.timestep_spacing == "trailing" and a.rescale_betas_zero_snr and a.freeu and a.height == 128
    assert generation.parse_args(["--scheduler", "DPMSolverMultistepScheduler", "--timestep-spacing", "trailing"]).timestep_spacing == "trailing"
    assert generation.parse_args(["--scheduler", "PNDMScheduler", "--timestep-spacing", "leading", "--guidance-rescale", "1"]).guidance_rescale == 1.0
    for bad in (["--guidance-rescale", "-0.1"], ["--guidance-rescale", "1.5"], ["--guidance-rescale", "nan"], ["--guidance-rescale"],
                ["--timestep-spacing", "karras"], ["--scheduler", "PNDMScheduler", "--timestep-spacing", "trailing"],
                ["--scheduler", "DPMSolverMultistepScheduler", "--rescale-betas-zero-snr"],
                ["--scheduler", "PNDMScheduler", "--rescale-betas-zero-snr"],
                ["--guidance-rescale", "0.7", "--panorama", "--synthetic-config", "tiny"]):
        with pytest.raises(SystemExit):
            generation.parse_args(bad)


def test_schedule_flags_rebuild_the_scheduler():
    """generation.apply_schedule_flags on a stand-in pipeline (cfg.sched + scheduler are all it touches)."""
    from types import SimpleNamespace
    from agenda_amd import generation
    from agenda_amd.config import SchedulerConfig
    from agenda_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler
    sc = SchedulerConfig(prediction_type="v_prediction")
    pipe = SimpleNamespace(cfg=SimpleNamespace(sched=sc), scheduler=DDIMScheduler.from_config(sc))
    generation.apply_schedule_flags(pipe, "trailing", True)
    assert isinstance(pipe.scheduler, DDIMScheduler) and pipe.scheduler.set_timesteps(4)[0] == 999 and pipe.scheduler.alphas_cumprod[-1] == 0
    sc = SchedulerConfig()
    pipe = SimpleNamespace(cfg=SimpleNamespace(sched=sc), scheduler=DPMSolverMultistepScheduler.from_config(sc))
    generation.apply_schedule_flags(pipe, "trailing", False)
    assert pipe.scheduler.timestep_spacing == "trailing" and sc.ddim_timestep_spacing == "leading"
    sc = SchedulerConfig()
    pipe = SimpleNamespace(cfg=SimpleNamespace(sched=sc), scheduler=PNDMScheduler.from_config(sc))
    with pytest.raises(ValueError, match="PNDMScheduler: only timestep_spacing='leading'"):
        generation.apply_schedule_flags(pipe, "linspace", False)


GUIDANCE_SYMBOLS = ("agd_guidance_rescale_set", "agd_guidance_rescale_clear", "agd_guidance_rescale_counts", "agd_op_guidance_rescale")


def test_library_exports_every_guidance_symbol():
    import ctypes
    from agenda_amd import _lib
    so = os.path.join(ROOT, "agenda_amd", "libagenda_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    txt = open(os.path.join(ROOT, "include", "agenda_hip.h")).read()
    for s in GUIDANCE_SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported"
        assert re.search(r"\b" + s + r"\s*\(", txt), f"{s} not declared in include/agenda_hip.h"
        assert s in _lib.EXPORTS


def test_python_surface():
    import inspect
    import agenda_amd
    from agenda_amd import ops, pipeline
    for name in ("guidance_rescale_set", "guidance_rescale_clear", "guidance_rescale_counts"):
        assert callable(getattr(pipeline.Engine, name))
    assert callable(ops.guidance_rescale)
    P = pipeline.StableDiffusionPipeline
    assert inspect.signature(P.__call__).parameters["guidance_rescale"].default == 0.0
    assert inspect.signature(P.img2img).parameters["guidance_rescale"].default == 0.0
    for sub in ("StableDiffusionControlNetPipeline", "StableDiffusionInpaintPipeline", "StableDiffusionInstructPix2PixPipeline",
                "StableDiffusionPanoramaPipeline", "StableDiffusionAdapterPipeline", "StableDiffusionGLIGENPipeline"):
        assert inspect.signature(getattr(agenda_amd, sub).__call__).parameters["guidance_rescale"].default == 0.0, sub
