"""tests/_tblock_model.py on its own, without a GPU: the fp64 references agree with torch and with each other where the kernels claim two
forms compute the same thing, every case of tests/test_tblock_ops_gpu.py stays under the ceiling with the model alone and meets the
residual condition (a case that does not would prove too little on the GPU and has to change its inputs), and the measure sees the
faults it is there for: one wrong 16 x 80 slab, an image with another's statistics, a dropped tile of the partial sums, a misplaced
recorder slice."""
import math

import pytest
import torch
import torch.nn.functional as F
import _tblock_model as TM
from _norm_model import _gn_stats
from _tblock_model import MODEL_CEILING, MODEL_FACTOR


def _worst(got, want):
    mx, rms = TM.slab_errors(TM.slabs(got), TM.slabs(want))
    return float(mx.max()), float(rms.max())


# ------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------
def test_references_agree_with_torch():
    i = TM.qkv_inputs(320, 2, 128, 32, 1)
    x = i["x"].double()
    y = F.group_norm(x.transpose(1, 2), 32, i["gn_gamma"].double(), i["gn_beta"].double(), TM.GN_EPS).transpose(1, 2).reshape(-1, 320)
    h = F.linear(y, i["w_in"].double(), i["b_in"].double())
    q = F.linear(F.layer_norm(h, (320,), i["gamma"].double(), i["beta"].double(), TM.LN_EPS), i["wqkv"].double())
    h64, q64 = TM.qkv_fp64(i)
    assert float((h64 - h).abs().max()) < 1e-9 and float((q64 - q).abs().max()) < 1e-9

    i = TM.ff_inputs(128, 1)
    x = i["x"].double()
    v, g = F.linear(F.layer_norm(x, (320,), i["gamma"].double(), i["beta"].double(), TM.LN_EPS), i["w1"].double(), i["b1"].double()).chunk(2, -1)
    y = x + F.linear(v * F.gelu(g), i["w2"].double(), i["b2"].double())
    p = F.linear(y, i["wp"].double(), i["bp"].double()) + i["xres"].double()
    y64, p64 = TM.ff_fp64(i, True)
    assert float((y64 - y).abs().max()) < 1e-9 and float((p64 - p).abs().max()) < 1e-9

    i = TM.attn_inputs(320, 2, 128, 17, 1, pre=True)
    x = i["x"].double()
    h1 = x + F.linear(i["o1"].double(), i["wo1"].double(), i["bo1"].double())
    qh = F.linear(F.layer_norm(h1, (320,), i["gamma"].double(), i["beta"].double(), TM.LN_EPS), i["wq"].double()).reshape(2, 128, 8, 40).transpose(1, 2)
    kv = i["kv"].double()
    kh, vh = (t.reshape(2, 17, 8, 40).transpose(1, 2) for t in (kv[..., :320], kv[..., 320:]))
    o = F.scaled_dot_product_attention(qh, kh, vh, scale=float(torch.tensor(40 ** -0.5, dtype=torch.float32))).transpose(1, 2).reshape(256, 320)
    y = h1 + F.linear(o, i["wo"].double(), i["bo"].double())
    y64, h64, P = TM.attn_fp64(i)
    assert float((y64 - y).abs().max()) < 1e-9 * float(y.abs().max()) and float((h64 - h1).abs().max()) < 1e-9
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12


def test_the_folded_groupnorm_is_the_inside_one_in_fp64():
    i = TM.qkv_inputs(320, 3, 128, 32, 2)
    x = i["x"].double()
    mean, var = _gn_stats(x.transpose(1, 2), 32)
    rstd = (var + TM._eps64(TM.GN_EPS)).rsqrt()
    sa = rstd.repeat_interleave(10, 1) * i["gn_gamma"].double()[None]                 # [B, C]
    W = i["w_in"].double()
    wb = W[None] * sa[:, None, :]
    rowadd = i["b_in"].double()[None] + (W @ i["gn_beta"].double())[None] - (wb * mean.repeat_interleave(10, 1)[:, None, :]).sum(-1)
    h = (x @ wb.transpose(1, 2) + rowadd[:, None, :]).reshape(-1, 320)
    assert float((h - TM.qkv_fp64(i)[0]).abs().max()) < 1e-9


def test_the_premultiplied_projection_is_the_two_stage_one_in_fp64():
    i = TM.ff_inputs(128, 2)
    y, p = TM.ff_fp64(i, True)
    x = i["x"].double()
    inc = y - x - i["b2"].double()                                                     # hidden . W2^T
    hid = torch.linalg.lstsq(i["w2"].double(), inc.T).solution.T                       # any hidden activation with that image serves the algebra
    w2p, bcp = TM.premul_fp64(i)
    p2 = hid @ w2p.T + x @ i["wp"].double().T + bcp + i["xres"].double()
    assert float((p2 - p).abs().max()) < 1e-8 * float(p.abs().max())


def test_shared_rows_are_duplicated_rows():
    for pre in (False, True):
        i = TM.attn_inputs(320, 2, 128, 17, 3, pre=pre, src_rows=128)
        j = dict(i, src_rows=0, x=i["x"].repeat(2, 1), **({"o1": i["o1"].repeat(2, 1)} if pre else {}))
        for a, b in zip(TM.attn_fp64(i) + TM.attn_model(i), TM.attn_fp64(j) + TM.attn_model(j)):
            assert torch.equal(a, b)
        assert not torch.equal(TM.attn_fp64(i)[0][:128], TM.attn_fp64(i)[0][128:])       # each half has its own context
    i = TM.ff_inputs(512, 3, xres_rows=256)
    j = dict(i, xres_rows=0, xres=i["xres"].repeat(2, 1))
    assert torch.equal(TM.ff_fp64(i, True)[1], TM.ff_fp64(j, True)[1])
    for post in (1, 2):
        assert torch.equal(TM.ff_model(i, post), TM.ff_model(j, post))


def test_head_group_sums_are_sums_of_heads():
    i = TM.attn_inputs(320, 2, 128, 17, 4)
    P = TM.attn_fp64(i)[2]
    one = TM.recorder_rows(P, 1)
    assert one.shape == (2, 8, 17, 128)
    for hpb in (2, 4, 8):
        assert float((TM.recorder_rows(P, hpb) - one.reshape(2, 8 // hpb, hpb, 17, 128).sum(2)).abs().max()) < 1e-14
    assert float((TM.recorder_rows(P, 8).sum(2) - 8).abs().max()) < 1e-12
    assert torch.equal(TM.recorder_rows(P, 2, 1, 9), TM.recorder_rows(P, 2)[1:, :, :9])


def test_partials_add_up_to_the_groupnorm_statistics():
    i = TM.qkv_inputs(320, 2, 384, 32, 5)
    x = i["x"].double()
    mean, var = _gn_stats(x.transpose(1, 2), 32)
    for bm in (64, 128):
        p = TM.qkv_part(i, bm).double()
        assert p.shape == (2, 384 // bm, 320, 2)
        s = p.sum(1).reshape(2, 32, 10, 2).sum(2) / (384 * 10)
        assert float((s[..., 0] - mean).abs().max()) < 1e-5 and float((s[..., 1] - mean * mean - var).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------------------------------------
# every GPU case: the ceiling, the residual condition
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,B,HW,bm,groups", TM.QKV_SHAPES_320 + TM.QKV_SHAPES_640)
def test_qkv_cases_stay_under_the_ceiling(C, B, HW, bm, groups):
    i = TM.qkv_inputs(C, B, HW, groups)
    h64, q64 = TM.qkv_fp64(i)
    for inside in (False, True):
        h, q = TM.qkv_model(i, inside)
        for e in TM.model_bounds(h, h64) + TM.model_bounds(q, q64):
            assert 0 < MODEL_FACTOR * e <= MODEL_CEILING


@pytest.mark.parametrize("name,M,posts,kw", TM.FF_CASES)
def test_ff_cases_stay_under_the_ceiling(name, M, posts, kw):
    i = TM.ff_inputs(M, **kw)
    y64, p64 = TM.ff_fp64(i, True)
    assert TM.residual_condition(y64, i["x"]) >= 1 and TM.residual_condition(p64, i["xres"]) >= 1
    for post in posts:
        for e in TM.model_bounds(TM.ff_model(i, post), y64 if post == 0 else p64):
            assert 0 < MODEL_FACTOR * e <= MODEL_CEILING
    if kw.get("tails"):
        x = i["x"].double()
        u = TM._ln64(x, i["gamma"], i["beta"], TM.LN_EPS) @ i["w1"].double().T + i["b1"].double()
        assert float(u[:, 1280:].min()) < -12 and float(u[:, 1280:].max()) > 12      # the gate pre-activations do reach both tails


@pytest.mark.parametrize("C,rows32", TM.ATTN_FORMS)
@pytest.mark.parametrize("pre", [False, True])
def test_attn_cases_stay_under_the_ceiling(C, rows32, pre):
    B, HW = 2, 2 * TM.attn_bm(C, rows32)
    cases = [dict(T=T, pre=pre) for T in TM.ATTN_T] + [dict(T=77, pre=pre, src_rows=HW)] + ([] if pre else [dict(T=77, peaked=True)])
    for kw in cases:
        i = TM.attn_inputs(C, B, HW, kw.pop("T"), **kw)
        y64, h64, P64 = TM.attn_fp64(i)
        ym, hm, Pm = TM.attn_model(i)
        assert TM.residual_condition(y64, h64) >= 1, kw
        for e in TM.model_bounds(ym, y64) + (TM.model_bounds(hm, h64) if pre else ()):
            assert 0 < MODEL_FACTOR * e <= MODEL_CEILING
        for hpb in (1, 2, 4, 8):
            assert TM.abs_bound(TM.recorder_rows(Pm, hpb), TM.recorder_rows(P64, hpb), hpb) < hpb * MODEL_CEILING


@pytest.mark.parametrize("ratio", TM.RATIOS_ASSERTED)
def test_large_mean_cases_stay_under_the_ceiling(ratio):
    for C in (320, 640):
        _, B, HW, bm, groups = TM.QKV_RATIO_SHAPE[C]
        i = TM.qkv_inputs(C, B, HW, groups, 9, ratio=ratio)
        xs = i["x"].double().reshape(B, HW, groups, -1).permute(0, 2, 1, 3).reshape(B, groups, -1)
        assert float((xs.mean(-1).abs() / xs.std(-1) - ratio).abs().max()) <= 0.1 * ratio + 0.15       # (the sample mean of HW x 10 or 20 values wanders by 0.03 sigma)
        h64, q64 = TM.qkv_fp64(i)
        for inside in (False, True):
            h, q = TM.qkv_model(i, inside)
            TM.model_bounds(h, h64), TM.model_bounds(q, q64)
    i = TM.ff_inputs(TM.FF_RATIO_M, 9, ratio=ratio)
    x = i["x"].double()
    assert float((x.mean(1).abs() / x.std(1) - ratio).abs().max()) <= 0.15 * ratio + 0.25
    y64, p64 = TM.ff_fp64(i, True)
    assert TM.residual_condition(y64, i["x"]) >= 1 and TM.residual_condition(p64, i["xres"]) >= 1
    for post in (0, 1, 2):
        TM.model_bounds(TM.ff_model(i, post), y64 if post == 0 else p64)
    for C, rows32 in TM.ATTN_FORMS:
        i = TM.attn_inputs(C, 1, 2 * TM.attn_bm(C, rows32), 77, 9, ratio=ratio)
        y64, h64, _ = TM.attn_fp64(i)
        assert TM.residual_condition(y64, h64) >= 1
        TM.model_bounds(TM.attn_model(i)[0], y64)


# ------------------------------------------------------------------------------------------------------------------------------
# the measure sees what it is there for
# ------------------------------------------------------------------------------------------------------------------------------
def _exceeds(bad, want, model):
    e_model, e_rms = TM.model_bounds(model, want)
    k_max, k_rms = TM.kernel_errors(bad, want, model)
    return k_max > MODEL_FACTOR * e_model and k_rms > MODEL_FACTOR * e_rms


def _one_slab_wrong(t, tile, wave, by=1.03):
    t = t.clone()
    t[16 * tile:16 * tile + 16, 80 * wave:80 * wave + 80] *= by
    return t


def test_qkv_measure_sees_a_wrong_slab_borrowed_statistics_and_a_dropped_tile():
    C, B, HW, bm, groups = 320, 3, 128, 64, 32
    i = TM.qkv_inputs(C, B, HW, groups)
    h64, q64 = TM.qkv_fp64(i)
    h, q = TM.qkv_model(i, True)
    assert _exceeds(_one_slab_wrong(h, 23, 3), h64, h) and _exceeds(_one_slab_wrong(q, 17, 11), q64, q)
    glob = float((_one_slab_wrong(q, 17, 11) - q64).abs().max() / q64.abs().max())
    assert glob < 2.0 ** -5                                                              # ... where a whole-tensor maximum hardly moves

    def chain(y):                                        # the rest of the model behind a given GroupNorm output [B, HW, C]
        hh = TM._r(TM._r(y.reshape(-1, C)) @ i["w_in"].double().T + i["b_in"].double())
        return hh, TM._r(TM._ln_model(hh, i["gamma"], i["beta"], TM.LN_EPS) @ i["wqkv"].double().T)

    x = i["x"].double()
    cpg = C // groups

    def normed(mean, var):                               # [B, G] statistics -> GroupNorm output
        m, r = mean.repeat_interleave(cpg, 1)[:, None, :], (var + TM._eps64(TM.GN_EPS)).rsqrt().repeat_interleave(cpg, 1)[:, None, :]
        return (x - m) * r * i["gn_gamma"].double() + i["gn_beta"].double()

    mean, var = _gn_stats(x.transpose(1, 2), groups)
    hh, qq = chain(normed(mean, var))
    assert not _exceeds(hh, h64, h) and not _exceeds(qq, q64, q)                         # the harness itself is the model
    m2, v2 = mean.clone(), var.clone()
    m2[1], v2[1] = mean[0], var[0]                       # image 1 takes image 0's statistics
    hh, qq = chain(normed(m2, v2))
    assert _exceeds(hh, h64, h) and _exceeds(qq, q64, q)
    assert _worst(hh[:HW], h64[:HW])[0] <= MODEL_FACTOR * TM.model_bounds(h, h64)[0]     # ... and only image 1 shows it

    C, B, HW, bm = 320, 1, 2112, 64                      # 33 tiles; the sums lose the last one
    i = TM.qkv_inputs(C, B, HW, groups)
    x = i["x"].double()
    h64, q64 = TM.qkv_fp64(i)
    h, q = TM.qkv_model(i, True)
    p = TM.qkv_part(i, bm).double()[:, :32].sum(1).reshape(B, groups, cpg, 2).sum(2) / (HW * cpg)
    hh, qq = chain(normed(p[..., 0], (p[..., 1] - p[..., 0] ** 2).clamp(min=0)))
    assert _exceeds(hh, h64, h)


def test_ff_measure_sees_a_wrong_slab_in_every_output():
    i = TM.ff_inputs(512, xres_rows=256)
    y64, p64 = TM.ff_fp64(i, True)
    for post in (0, 1, 2):
        m, want = TM.ff_model(i, post), (y64 if post == 0 else p64)
        assert _exceeds(_one_slab_wrong(m, 31, 2), want, m) and _exceeds(_one_slab_wrong(m, 0, 0), want, m)
        assert not _exceeds(m, want, m)
    # a residual row taken from the wrong half of the shared prefix
    m = TM.ff_model(dict(i, xres=i["xres"].roll(128, 0)), 1)
    assert _exceeds(m, p64, TM.ff_model(i, 1))


def test_attn_measure_sees_a_wrong_slab_and_a_misplaced_recorder_slice():
    i = TM.attn_inputs(640, 2, 128, 77)
    y64, _, P64 = TM.attn_fp64(i)
    ym, _, Pm = TM.attn_model(i)
    assert _exceeds(_one_slab_wrong(ym, 15, 7), y64, ym) and not _exceeds(ym, y64, ym)
    for hpb in (1, 2, 4):
        want, mod = TM.recorder_rows(P64, hpb), TM.recorder_rows(Pm, hpb)
        bound = TM.abs_bound(mod, want, hpb)
        assert float((mod - want).abs().max()) <= bound
        assert float((mod.roll(1, 1) - want).abs().max()) > bound                       # slices in each other's place
        assert float((mod.roll(1, 0) - want).abs().max()) > bound                       # images in each other's place
        assert float((mod.roll(1, 2) - want).abs().max()) > bound                       # token rows shifted by one
    # image 1 attending to image 0's context
    j = dict(i, kv=i["kv"].flip(0))
    assert _exceeds(TM.attn_model(j)[0], y64, ym)
    assert math.isclose(TM.MODEL_FACTOR, 2.0) and math.isclose(TM.MODEL_CEILING, 2.0 ** -6)
