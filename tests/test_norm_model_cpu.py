"""tests/_norm_model.py on its own, without a GPU: the fp64 references agree with torch's own GroupNorm / LayerNorm, the host-made
partial-sum tables add up to the statistics, and every case of tests/test_norm_ops_gpu.py stays under the ceiling with the model alone
(a case above it would prove too little on the GPU and has to change its inputs)."""
import pytest
import torch
import torch.nn.functional as F
import test_norm_ops_gpu as T
from _norm_model import (MODEL_CEILING, MODEL_FACTOR, fold_fp64, fold_model, fold_slabs, gn_slabs, groupnorm_fp64, groupnorm_model, layernorm_fp64,
                         layernorm_model, ln_slabs, model_bounds, nhwc, partials, slab_errors)


def test_references_agree_with_torch():
    x0, x1, ga, be = T._gn_inputs(2, 64, 32, (6, 4), 12, 1)
    x = torch.cat([x0, x1], 1).double()
    want = F.silu(F.group_norm(x, 12, ga.double(), be.double(), 1e-5))
    assert float((groupnorm_fp64(x0, x1, 12, ga, be, 1e-5, True) - want).abs().max()) < 1e-9
    xl, ga, be = T._ln_inputs(9, 72, 1)
    want = F.layer_norm(xl.double(), (72,), ga.double(), be.double(), 1e-6)
    assert float((layernorm_fp64(xl, ga, be, 1e-6) - want).abs().max()) < 1e-9


def test_partials_add_up_to_the_statistics():
    x0, _, _, _ = T._gn_inputs(2, 64, 0, (8, 16), 32, 2)
    p = partials(nhwc(x0), 64).double()                                               # [B, 2, C, 2]
    n = 2 * 128
    s = p.sum(1).reshape(2, 32, 2, 2).sum(2)                                          # per (image, group): sum, sum of squares
    xs = x0.double().reshape(2, 32, -1)
    assert float((s[..., 0] / n - xs.mean(-1)).abs().max()) < 1e-6
    assert float((s[..., 1] / n - xs.pow(2).mean(-1)).abs().max()) < 1e-5
    assert partials(nhwc(x0), 48).shape == (2, 2, 64, 2)                              # a ragged last tile is left out


def test_slab_measure_sees_one_wrong_slab_and_refuses_an_unjudgeable_zero_slab():
    want = torch.randn(2, 4, 50, dtype=torch.float64)
    want[1, 2] *= 2.0 ** -10                                                          # a small slab
    got = want.clone()
    got[1, 2] *= 1.5
    mx, rms = slab_errors(got, want)
    assert float(mx[1, 2]) == pytest.approx(0.5) and float(rms[1, 2]) == pytest.approx(0.5) and float(mx.sum()) == pytest.approx(0.5)
    assert float((got - want).abs().max() / want.abs().max()) < 2.0 ** -7             # ... which the global measure does not see
    want[0, 0] = 0
    with pytest.raises(AssertionError):
        slab_errors(got, want)
    got[0, 0] = 0
    with pytest.raises(AssertionError):
        slab_errors(got, want, got + 1)
    assert float(slab_errors(got, want, got)[0][0, 0]) == 0.0


@pytest.mark.parametrize("inst,rows,C", T.LN_CASES)
def test_layernorm_cases_stay_under_the_ceiling(inst, rows, C):
    x, ga, be = T._ln_inputs(rows, C)
    e = model_bounds(ln_slabs(layernorm_model(x, ga, be, 1e-5)), ln_slabs(layernorm_fp64(x, ga, be, 1e-5)))
    assert 0 < MODEL_FACTOR * max(e) <= MODEL_CEILING


@pytest.mark.parametrize("case", T.GN_TWO + [(c[0], c[1], c[2], c[5], c[6], c[7], c[8]) for c in T.GN_PART])
def test_groupnorm_cases_stay_under_the_ceiling(case):
    C0, C1, shape, groups, B, silu, eps = case
    x0, x1, ga, be = T._gn_inputs(B, C0, C1, shape, groups)
    e = model_bounds(gn_slabs(groupnorm_model(x0, x1, groups, ga, be, eps, silu), groups), gn_slabs(groupnorm_fp64(x0, x1, groups, ga, be, eps, silu), groups))
    assert 0 < MODEL_FACTOR * max(e) <= MODEL_CEILING


@pytest.mark.parametrize("C,N,HW,bm,B", T.FOLD)
def test_fold_cases_stay_under_the_ceiling(C, N, HW, bm, B):
    x, ga, be, w, bias = T._fold_inputs(C, N, HW, bm, B)
    m = fold_model(x, 32, ga, be, 1e-6, w, bias)
    e = model_bounds(fold_slabs(m["y"]), fold_slabs(fold_fp64(x, 32, ga, be, 1e-6, w, bias)))
    assert 0 < MODEL_FACTOR * max(e) <= MODEL_CEILING
    assert float((m["wb_lo"] != m["wb_hi"]).float().mean()) < 1e-3                    # the share of Wb whose rounding the declared arithmetic leaves open


@pytest.mark.parametrize("ratio", [0, 4, 32, 128])
def test_large_mean_cases_stay_under_the_ceiling(ratio):
    x0, x1, ga, be = T._gn_inputs(2, 320, 320, (32, 32), 32, 9, ratio=ratio)
    model_bounds(gn_slabs(groupnorm_model(x0, x1, 32, ga, be, 1e-5, True), 32), gn_slabs(groupnorm_fp64(x0, x1, 32, ga, be, 1e-5, True), 32))
    xs = torch.cat([x0, x1], 1).double().reshape(2, 32, -1)
    got = xs.mean(-1).abs() / xs.std(-1)
    assert float((got - ratio).abs().max()) <= 0.1 * ratio + 0.05                     # the inputs have the mean / sigma they claim (bf16 rounding widens sigma a little)
    x, ga, be = T._ln_inputs(33, 320, 9, ratio=ratio)
    model_bounds(ln_slabs(layernorm_model(x, ga, be, 1e-5)), ln_slabs(layernorm_fp64(x, ga, be, 1e-5)))
    x, ga, be, w, bias = T._fold_inputs(320, 320, 256, 64, 2, 9, ratio=ratio)
    model_bounds(fold_slabs(fold_model(x, 32, ga, be, 1e-6, w, bias)["y"]), fold_slabs(fold_fp64(x, 32, ga, be, 1e-6, w, bias)))
