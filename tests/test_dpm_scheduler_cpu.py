"""DPM-Solver++ (2M) host scheduler (agenda_amd/scheduler.py DPMSolverMultistepScheduler), CPU only: the coefficient program
`dpm_program()` the device loop applies, checked against closed forms and against an independent restatement of the update."""
import json

import _dpm_restated as R
import numpy as np
import pytest

from agenda_amd.config import SchedulerConfig
from agenda_amd.scheduler import (SCHEDULERS, DPMSolverMultistepScheduler, scheduler_config_from_json,
                                  scheduler_config_to_json)


def _sched(pred="epsilon", karras=False, spacing="linspace"):
    return DPMSolverMultistepScheduler.from_config(SchedulerConfig(prediction_type=pred, use_karras_sigmas=karras, timestep_spacing=spacing))


def _run_program(s, model, x):
    """Chain dpm_program() in float64: x0 = cx x + ce m, x = a x + b0 x0 + b1 x0_prev."""
    ts, cx, ce, a, b0, b1 = (np.asarray(v, dtype=np.float64) for v in s.dpm_program())
    prev = np.zeros_like(x)
    for i in range(len(ts)):
        x0 = cx[i] * x + ce[i] * model(x, i)
        x = a[i] * x + b0[i] * x0 + b1[i] * prev
        prev = x0
    return x


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("n", [1, 2, 5, 20, 50])
def test_constant_data_prediction_is_integrated_exactly(pred, karras, n):
    """A model whose data prediction is a fixed c: DPM-Solver++ is exact at first and second order, so the chained program lands on
    x_f = (sigma_f / sigma_0) x_0 + (alpha_f - sigma_f alpha_0 / sigma_0) c (alpha / sigma: the scheduler's own grid values)."""
    s = _sched(pred, karras)
    s.set_timesteps(n)
    al, sg = s.alpha, s.sigma
    rng = np.random.default_rng(n)
    x_init = rng.standard_normal(4096)
    c = 0.7 + 0.3 * rng.standard_normal(4096)

    def model(x, i):
        eps = (x - al[i] * c) / sg[i]
        return eps if pred == "epsilon" else al[i] * eps - sg[i] * c

    got = _run_program(s, model, x_init)
    want = (sg[-1] / sg[0]) * x_init + (al[-1] - sg[-1] * al[0] / sg[0]) * c
    rel = np.abs(got - want).max() / np.abs(want).max()
    assert rel < 1e-5, rel


# ---- independent restatement (tests/_dpm_restated.py) ---------------------------------------------------------------------
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("n", [3, 8, 20, 25])
def test_program_matches_an_independent_restatement(pred, karras, n):
    """A smooth nonlinear toy model, stepped by the formulas written out in this file and by the scheduler's coefficient program."""
    rng = np.random.default_rng(7)
    x_init = rng.standard_normal(2048)
    w = rng.standard_normal(2048)

    def toy(x, t):
        return 0.6 * np.tanh(x) + 0.3 * np.sin(0.004 * t + w) * x + 0.1 * w

    t_ref, want = R.sample(n, karras, pred, lambda x, i, t: toy(x, t), x_init)
    s = _sched(pred, karras)
    ts = s.set_timesteps(n)
    np.testing.assert_allclose(ts, t_ref, rtol=1e-12, atol=1e-9)
    tsf = s.dpm_program()[0]
    got = _run_program(s, lambda x, i: toy(x, float(tsf[i])), x_init)
    rel = np.abs(got - want).max() / np.abs(want).max()
    assert rel < 1e-5, rel


# ---- program structure ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("n", [1, 2, 10, 14, 15, 20, 50])
def test_program_structure(karras, n):
    s = _sched("epsilon", karras)
    s.set_timesteps(n)
    ts, cx, ce, a, b0, b1 = s.dpm_program()
    assert all(len(v) == n for v in (ts, cx, ce, a, b0, b1)) and all(v.dtype == np.float32 for v in (ts, cx, ce, a, b0, b1))
    assert len(s.alpha) == len(s.sigma) == n + 1
    assert np.all(np.diff(ts) < 0) and ts[0] <= 999 and ts[-1] >= 0
    np.testing.assert_allclose(s.alpha ** 2 + s.sigma ** 2, 1.0, rtol=1e-12)
    ab0 = float(s.alphas_cumprod[0])
    assert s.alpha[-1] == pytest.approx(ab0 ** 0.5, rel=1e-9)             # the last step targets timestep 0 of the table
    if not karras:
        assert np.array_equal(ts, np.round(ts))
    else:
        abar = s.alphas_cumprod.astype(np.float64)
        table = np.sqrt((1 - abar) / abar)
        ks = s.karras_sigmas
        assert np.all(np.diff(ks) < 0) if n > 1 else True
        assert ks[0] == pytest.approx(table[-1], rel=1e-12)
        if n > 1:
            assert ks[-1] == pytest.approx(table[0], rel=1e-12)
        if n > 2:
            assert not np.array_equal(ts[1:-1], np.round(ts[1:-1]))         # fractional in between
    assert b1[0] == 0.0                                                    # step 0: first order
    if n >= 2:
        assert np.all(b1[1:-1] != 0.0)                                     # second order in between
        if karras:                                                         # the last evaluation sits on sigma_min: identity update
            assert (a[-1], b0[-1], b1[-1]) == (1.0, 0.0, 0.0)
        elif n < 15:                                                       # lower_order_final: first order below 15 steps
            assert b1[-1] == 0.0 and b0[-1] != 0.0
        else:
            assert b1[-1] != 0.0


@pytest.mark.parametrize("spacing,first,last", [("linspace", 999, 50), ("leading", 941, 48), ("trailing", 999, 49)])
def test_timestep_spacings(spacing, first, last):
    """20 steps over 1000 training steps, each upstream spacing rule."""
    ts = _sched(spacing=spacing).set_timesteps(20)
    assert len(ts) == 20 and ts[0] == first and ts[-1] == last


def test_prediction_type_sets_the_data_prediction():
    for pred in ("epsilon", "v_prediction"):
        s = _sched(pred)
        s.set_timesteps(5)
        _, cx, ce, *_ = s.dpm_program()
        al, sg = s.alpha[:-1], s.sigma[:-1]
        want = (1 / al, -sg / al) if pred == "epsilon" else (al, -sg)
        np.testing.assert_allclose(cx, want[0], rtol=1e-6)
        np.testing.assert_allclose(ce, want[1], rtol=1e-6)


# ---- configuration -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver++"), dict(solver_order=3),
                                 dict(solver_order=1), dict(solver_type="heun"), dict(lower_order_final=False),
                                 dict(final_sigmas_type="zero"), dict(thresholding=True), dict(euler_at_final=True),
                                 dict(use_lu_lambdas=True), dict(variance_type="learned_range"), dict(lambda_min_clipped=-5.1),
                                 dict(beta_schedule="linear"), dict(skip_prk_steps=True), dict(prediction_type="sample"),
                                 dict(timestep_spacing="karras")])
def test_unsupported_options_raise(opt):
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler(**opt)


def test_supported_options_construct():
    DPMSolverMultistepScheduler(algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint", lower_order_final=True,
                                lambda_min_clipped=-float("inf"), thresholding=False, variance_type=None, final_sigmas_type="sigma_min")
    with pytest.raises(ValueError):
        DPMSolverMultistepScheduler().set_timesteps(0)


@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_json_round_trip(karras, pred):
    """save_pretrained's writer -> JSON text -> from_pretrained's parser: the same scheduler and options come back."""
    sc = SchedulerConfig(prediction_type=pred, use_karras_sigmas=karras, timestep_spacing="trailing")
    sj = json.loads(json.dumps(scheduler_config_to_json("DPMSolverMultistepScheduler", sc)))
    assert sj["_class_name"] == "DPMSolverMultistepScheduler"
    back = scheduler_config_from_json(sj, sj["_class_name"])
    assert back == sc
    s = SCHEDULERS[sj["_class_name"]].from_config(back)
    assert isinstance(s, DPMSolverMultistepScheduler) and s.use_karras_sigmas == karras and s.prediction_type == pred


def test_json_parsing_of_diffusers_configs():
    """A DPM config as diffusers writes it (-Infinity, thresholding keys) loads; an unsupported value in it raises; a PNDM config
    overridden to DPM gets DPM's defaults (linspace spacing, no Karras), not the PNDM-only keys."""
    sj = json.loads('{"_class_name": "DPMSolverMultistepScheduler", "algorithm_type": "dpmsolver++", "beta_end": 0.012, '
                    '"beta_schedule": "scaled_linear", "beta_start": 0.00085, "dynamic_thresholding_ratio": 0.995, '
                    '"lambda_min_clipped": -Infinity, "lower_order_final": true, "num_train_timesteps": 1000, '
                    '"prediction_type": "v_prediction", "sample_max_value": 1.0, "solver_order": 2, "solver_type": "midpoint", '
                    '"steps_offset": 1, "thresholding": false, "timestep_spacing": "leading", "trained_betas": null, '
                    '"use_karras_sigmas": true, "variance_type": null}')
    sc = scheduler_config_from_json(sj, "DPMSolverMultistepScheduler")
    assert sc.use_karras_sigmas and sc.timestep_spacing == "leading" and sc.prediction_type == "v_prediction"
    for k, v in (("solver_order", 3), ("algorithm_type", "sde-dpmsolver++"), ("lambda_min_clipped", -5.1), ("thresholding", True)):
        with pytest.raises(ValueError):
            scheduler_config_from_json(dict(sj, **{k: v}), "DPMSolverMultistepScheduler")
    pndm = {"_class_name": "PNDMScheduler", "skip_prk_steps": True, "steps_offset": 1, "set_alpha_to_one": False}
    sc = scheduler_config_from_json(pndm, "DPMSolverMultistepScheduler")
    assert not sc.use_karras_sigmas and sc.timestep_spacing == "linspace"
    assert isinstance(DPMSolverMultistepScheduler.from_config(sc), DPMSolverMultistepScheduler)


def test_registry_and_cli():
    from agenda_amd import generation
    assert SCHEDULERS["DPMSolverMultistepScheduler"] is DPMSolverMultistepScheduler
    a = generation.parse_args(["--scheduler", "DPMSolverMultistepScheduler", "--use-karras-sigmas"])
    assert a.scheduler == "DPMSolverMultistepScheduler" and a.use_karras_sigmas
    with pytest.raises(SystemExit):
        generation.parse_args(["--use-karras-sigmas"])
    with pytest.raises(SystemExit):
        generation.parse_args(["--scheduler", "PNDMScheduler", "--use-karras-sigmas"])


def test_generation_help_lists_the_scheduler(capsys):
    from agenda_amd import generation
    with pytest.raises(SystemExit):
        generation.parse_args(["--help"])
    out = capsys.readouterr().out
    assert "DPMSolverMultistepScheduler" in out and "--use-karras-sigmas" in out
