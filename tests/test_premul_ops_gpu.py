"""The pre-multiplied cross-attention kernels of csrc/xattn_pre.hip (`premul_gemm_kernel`, `premul_rowsum_kernel`, `matvec_bf16_kernel`,
`xattn_s_kernel`) and csrc/ipadapter.hip (`ipa_linear_kernel`, `ipa_layernorm_kernel`, `ipa_kpp_kernel` / `ipa_csbs_kernel` / `ipa_vpp_kernel`,
`ipa_scores_kernel<1..5>`, `ipa_add_kernel`) stage by stage, through the single-op entries `ops.xattn_context`, `ops.xattn_scores`, `ops.ipa_*`,
and end to end through the unchanged `ops.xattn_premul`.

Reference: tests/_premul_model.py, fp64 on the bf16-rounded inputs.  Measure: every slab of 16 rows x 80 columns on its own (for P exactly one
wave's tile of one head; operands narrower than 80 columns or no multiple of it: 16 rows x the whole width), max |error| / max |slab| and RMS
error / RMS slab.  Bound, per case and from the reference alone: the model restates the roundings the kernels declare; its worst slab against
fp64 is E_model / E_rms, the kernel must stay within MODEL_FACTOR = 2 x each, and no case may have 2 x E above 2^-6.  Where the model IS the
reference (one token: P = 1) the kernel must equal it bit for bit.  y and h' are judged on inputs whose increment is at least as large (RMS) as
the residual, asserted from the reference.  Recorder rows: `abs_bound`.  fp32 sums (cs, bs, ipa_linear): MODEL_FACTOR x `fp32_sum_error` of the
model's terms, relative to sum |terms|; bs adds what its inputs carry -- the mat-vec Wq . beta behind it is an fp32 sum of its own (its error,
taken the same way, weighs on term d with |k_d|), and the final product with the scale rounds once more (2^-24 of sum |terms|).  A run with the
statistics in several slots against the one-slot run (the library's own row sums): both sets of sums are within the fp32-sum error of the exact
ones (`fp32_sum_error` of the row's terms; `slots` x 2^-24 for the sum over the slots), so the fp32 probabilities may differ by what the model's
probabilities move when its sums are shifted by that much in either direction, plus the floor of `abs_bound`.  Where two launches must do the
same arithmetic (a batch against its images, a second run, two launches onto one recorder, tied keys) the outputs are compared bit for bit.

Sensitivity (verified on the CPU in tests/test_premul_model_cpu.py by applying each perturbation to the model's output): the measure rejects the
attention branch scaled by 0.97 -- which max |err| / max |y| < 2^-7 on the residual-dominated inputs of test_xattn_premul_matches_torch accepts
(0.005 to 0.0077 against 0.0078) --, two (head, token) columns of V'' swapped, token T - 1 dropped from one head, the recorder's rows shifted by
one, and only the first statistics slot summed.

Which instantiation a case runs: `ipa_scores_kernel<NT>` with NT = colsP / 16 (`_premul_model.ipa_nt_inst`), recorded in every case's name.

MEASURED_RATIOS below records kernel error / model error as measured on an MI355X."""
import functools

import pytest
import torch
import _premul_model as PM
from _premul_model import MODEL_FACTOR
from _report import report

pytestmark = pytest.mark.gpu

# kernel error / model error (max-measure, rms-measure): the worst case of each kernel over this file, measured on an MI355X.  The worst slab of
# every bf16 output is the model's own worst slab, element for element; the RMS shows the fp32 accumulation and the hardware exp2 the model leaves
# out.  The only case off 1.00 on the max-measure is |mean| / sigma = 128 at C = 320 (1.0221).  One number: kernel error / bound, for the fp32
# sums, the recorder rows (bound: `abs_bound`) and the several-slots run against the one-slot run.
MEASURED_RATIOS = {
    "premul_gemm_kernel K''": (1.0000, 1.0000), "premul_gemm_kernel V''": (1.0000, 1.0000),
    "premul_rowsum_kernel cs": 0.9651, "premul_rowsum_kernel bs (with matvec_bf16_kernel behind it)": 0.0954,
    "xattn_s_kernel P": (1.0221, 1.0005), "xattn_s_kernel recorder": 0.5001, "xattn_s_kernel slots vs one": 0.0857,
    "xattn_premul y": (1.0000, 1.0015), "xattn_premul recorder": 0.5092,
    "ipa_linear_kernel": 0.6193, "ipa_layernorm_kernel": (1.0189, 1.0585),
    "ipa_kpp_kernel": (1.0000, 1.0000), "ipa_vpp_kernel": (1.0000, 1.0000), "ipa_csbs_kernel cs": 0.7762, "ipa_csbs_kernel bs": 0.1809,
    "ipa_scores_kernel<1>": (1.0000, 1.0000), "ipa_scores_kernel<2>": (1.0000, 1.0000), "ipa_scores_kernel<3>": (1.0000, 1.0000),
    "ipa_scores_kernel<4>": (1.0000, 1.0000), "ipa_scores_kernel<5>": (1.0000, 1.0000),
    "ipa_add_kernel": (1.0000, 1.0000), "ipa branch h' (context -> scores -> add on the kernels' own intermediates)": (1.0000, 1.0006),
}


@pytest.fixture(scope="module")
def ops():
    from agenda_amd import ops as o
    return o


@pytest.fixture(scope="module")
def err_type():
    from agenda_amd._lib import AgendaHipError
    return AgendaHipError


def cu(t):
    return None if t is None else t.float().cuda()


def _judge(kernel, name, got, want, model, cols=80, ratio_only=False):
    """[M, N] operands -> (kernel max / model max, kernel rms / model rms)"""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), (kernel, name)
    if ratio_only:
        e_model, e_rms = PM.errors(model, want, model, cols)
    else:
        e_model, e_rms = PM.bounds(model, want, cols)
    if e_model == 0.0:                                     # the model is the reference: so must the kernel be
        assert torch.equal(got, model.double()), (kernel, name, "not bit-identical to a model that is exact")
        print(f"RATIO|{kernel}|1.0|1.0|{name}: bit-identical to the exact model")
        report(f"premul_ops[{kernel} {name}]", bit_identical=1)
        return 1.0, 1.0
    k_max, k_rms = PM.errors(got, want, model, cols)
    print(f"RATIO|{kernel}|{k_max / e_model:.4f}|{k_rms / e_rms:.4f}|{name}: worst slab max {k_max:.6f} (E_model {e_model:.6f}), rms {k_rms:.6f} (E_rms {e_rms:.6f})")
    report(f"premul_ops[{kernel} {name}]", kernel_max=k_max, model_max=e_model, kernel_rms=k_rms, model_rms=e_rms, ratio_max=k_max / e_model, ratio_rms=k_rms / e_rms)
    if not ratio_only:
        assert k_max <= MODEL_FACTOR * e_model, (kernel, name, "max", k_max, e_model)
        assert k_rms <= MODEL_FACTOR * e_rms, (kernel, name, "rms", k_rms, e_rms)
    return k_max / e_model, k_rms / e_rms


def _sum_check(kernel, name, got, exact, terms, extra=None):
    """fp32 sums along the last axis of `terms` (fp64): |got - exact| <= MODEL_FACTOR x fp32_sum_error(terms) x sum |terms| (+ extra, absolute)"""
    e_ref, scale = PM.fp32_sum_error(terms, -1)
    bound = MODEL_FACTOR * e_ref * scale + (0.0 if extra is None else extra)
    err = (got.double().cpu() - exact).abs()
    worst = float((err / bound.clamp(min=1e-300)).max()) if float(bound.max()) > 0 else 0.0
    rel = float((err / scale).max())
    print(f"RATIO|{kernel}|{worst:.4f}|{worst:.4f}|{name}: {rel:.3e} of sum |terms| (fp32 in other orders {e_ref:.3e}); error / bound {worst:.3f}")
    report(f"premul_ops[{kernel} {name}]", err_over_bound=worst, fp32_other_orders=e_ref * 1e6, err_rel=rel * 1e6)
    assert bool((err <= bound).all()), (kernel, name, rel, e_ref)


def _rec_check(kernel, name, rec, P64, Pm, b0=0, T=None, base=0.0):
    want, mod = PM.recorder_rows(P64, b0, T), PM.recorder_rows(Pm, b0, T)
    bound = PM.abs_bound(mod, want)
    err = float((rec.double().cpu() - base - want).abs().max())
    print(f"RATIO|{kernel} recorder|{err / bound:.4f}|{err / bound:.4f}|{name}: max abs error {err:.3e} (bound {bound:.3e})")
    report(f"premul_ops[{kernel} recorder {name}]", max_abs=err * 1e3, bound=bound * 1e3)
    assert err <= bound, (name, err, bound)


# ------------------------------------------------------------------------------------------------------------------------------
# the context products
# ------------------------------------------------------------------------------------------------------------------------------
def _ctx_run(ops, i):
    return tuple(t.cpu() for t in ops.xattn_context(cu(i["kv"]), cu(i["wq"]), cu(i["wo"]), cu(i["gamma"]), cu(i["beta"]), i["heads"]))


def _bs_check(kernel, name, got, exact, k, wq, beta, D):
    """bs = scale sum_d k_d fp32(Wq beta)_d: see the file's docstring for the bound"""
    terms, e_mv, a_mv = PM.bs_terms(k, wq, beta)
    sc = PM.scale32(D)
    extra = sc * (2.0 ** -24 * terms.abs().sum(-1) + MODEL_FACTOR * e_mv * (k.permute(0, 2, 1, 3).abs() * a_mv[None, :, None, :]).sum(-1))
    _sum_check(kernel, name, got, exact, terms * sc, extra)


@pytest.mark.parametrize("B,T,C,heads", PM.CONTEXT_CASES)
def test_xattn_context_products(ops, B, T, C, heads):
    """K'' and V'' slab by slab; the padding exactly zero; cs against the sum of the K'' that came back; bs; every image alone and a second run
    bit for bit"""
    i = PM.xattn_inputs(C, B, 64, T, heads=heads, gain=False)
    want, model = PM.xattn_context_fp64(i), PM.xattn_context_model(i)
    kpp, cs, bs, vpp = got = _ctx_run(ops, i)
    name = f"B={B} T={T} C={C} heads={heads}"
    assert kpp.shape == (B, heads, 80, C) and cs.shape == (B, heads, 80) and bs.shape == cs.shape and vpp.shape == (B, C, heads, 80)
    _judge("premul_gemm_kernel K''", name, kpp.reshape(-1, C), want[0].reshape(-1, C), model[0].reshape(-1, C))
    _judge("premul_gemm_kernel V''", name, vpp.reshape(B * C, -1), want[3].reshape(B * C, -1), model[3].reshape(B * C, -1))
    for nm, t in (("K''", kpp[:, :, T:]), ("V''", vpp[..., T:]), ("cs", cs[..., T:]), ("bs", bs[..., T:])):
        assert bool((t == 0).all()), (name, nm, "padding of token rows >= T")
    _sum_check("premul_rowsum_kernel cs", name, cs[..., :T], kpp[:, :, :T].double().sum(-1), model[0][:, :, :T])
    _bs_check("premul_rowsum_kernel bs", name, bs[..., :T], want[2][..., :T], PM._kv_heads(i)[0], i["wq"], i["beta"], C // heads)
    for a, b in zip(got, _ctx_run(ops, i)):
        assert torch.equal(a, b), (name, "second run")
    for b in range(B if B > 1 else 0):
        for a, t in zip(_ctx_run(ops, dict(i, kv=i["kv"][b:b + 1], B=1)), got):
            assert torch.equal(a[0], t[b]), (name, "image alone", b)


# ------------------------------------------------------------------------------------------------------------------------------
# xattn_s_kernel
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _xs_ref(C, B, HW, T, ratio=None, special=False):
    i = PM.xattn_inputs(C, B, HW, T, *((9,) if ratio is not None else ()), ratio=ratio)
    if special:
        i = PM.special_rows(i)
    return i, PM.xattn_fp64(i), PM.xattn_context_model(i)


def _xs_run(ops, i, ctx, T=None, **kw):
    return ops.xattn_scores(cu(i["x"]), cu(ctx[0]), cu(ctx[1]), cu(ctx[2]), i["T"] if T is None else T, i["heads"], PM.LN_EPS, **kw).cpu()


def _stats(i, slots):
    return PM.slot_stats(i["x"].reshape(-1, i["C"]), slots)


def _row_sums(name, P, Pbm, T):
    """every head's bf16 row sums to 1 as closely as the model's does (x MODEL_FACTOR)"""
    dev, devm = float((P.double().sum(-1) - 1).abs().max()), float((Pbm.sum(-1) - 1).abs().max())
    print(f"xattn_s_kernel {name}: row sums within {dev:.3e} of 1 (the model's: {devm:.3e})")
    assert dev <= MODEL_FACTOR * devm, (name, dev, devm)


@pytest.mark.parametrize("C,T,B,HW,slots", PM.XS_CASES)
def test_xattn_scores_every_shape(ops, C, T, B, HW, slots):
    """P slab by slab with the statistics in `slots` uneven partial sums; columns t >= T zero; rows sum to 1; the recorder; the one-slot run (the
    library's own row sums) agrees; every image alone and a second run bit for bit"""
    i, (_, P64), ctx = _xs_ref(C, B, HW, T)
    H, M = i["heads"], B * HW
    st = _stats(i, slots)
    Pm, Pbm = PM.xattn_scores(i, ctx, st)
    name = f"C={C} T={T} B={B} HW={HW} slots={slots}"
    rec = torch.zeros(B, H, T, HW, device="cuda")
    P = _xs_run(ops, i, ctx, stats=cu(st), rec=rec)
    assert P.shape == (B, HW, H, 80)
    _judge("xattn_s_kernel P", name, P.reshape(M, -1), P64.reshape(M, -1), Pbm.reshape(M, -1))
    assert bool((P[..., T:] == 0).all()), (name, "columns t >= T")
    _row_sums(name, P[..., :T], Pbm[..., :T], T)
    _rec_check("xattn_s_kernel", name, rec, P64, Pm, 0, T)
    # p (1 / sum p) with the sum of T <= 80 terms taken in fp32, one rounding each for the reciprocal and the product
    assert float((rec.double().sum(2) - 1).abs().max()) <= (T + 8) * 2.0 ** -24, name
    rec2 = torch.zeros_like(rec)
    assert torch.equal(_xs_run(ops, i, ctx, stats=cu(st), rec=rec2), P) and torch.equal(rec2, rec), (name, "second run")
    if slots > 1:
        rec1 = torch.zeros_like(rec)
        P1 = _xs_run(ops, i, ctx, rec=rec1)
        _judge("xattn_s_kernel P", name + " (one slot, the library's sums)", P1.reshape(M, -1), P64.reshape(M, -1), PM.xattn_scores(i, ctx)[1].reshape(M, -1))
        x2 = i["x"].double().reshape(M, C)
        e = MODEL_FACTOR * max(PM.fp32_sum_error(x2, 1)[0], PM.fp32_sum_error(x2 * x2, 1)[0]) + slots * 2.0 ** -24
        move = max(float((PM.xattn_scores(i, ctx, st, shift=(a * e, b * e))[0] - Pm).abs().max()) for a in (-1, 1) for b in (-1, 1))
        bound = 2 * move + MODEL_FACTOR * 2.0 ** -22       # (each run within `move` of the exact sums' probabilities)
        err = float((rec.double() - rec1.double()).abs().max())
        print(f"RATIO|xattn_s_kernel slots vs one|{err / bound:.4f}|{err / bound:.4f}|{name}: fp32 probabilities differ by {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (name, err, bound)
    for b in range(B if B > 1 else 0):
        ib = dict(i, x=i["x"][b:b + 1], B=1)
        recb = torch.zeros(1, H, T, HW, device="cuda")
        Pb = _xs_run(ops, ib, tuple(t[b:b + 1] for t in ctx), stats=cu(st.reshape(B, HW, slots, 2)[b]), rec=recb)
        assert torch.equal(Pb[0], P[b]) and torch.equal(recb[0], rec[b]), (name, "image alone", b)


@pytest.mark.parametrize("C", [320, 1280])
def test_xattn_scores_recorder_forms(ops, C):
    """rec_b0 = B / 2 at B = 4 and rec_T in T, T - 1, 20, 1 inside a larger buffer full of a sentinel: only the recording images' first rec_T
    rows change, by old + P in fp32 bit for bit; two launches onto a zeroed recorder give exactly twice the first"""
    B, HW, T = 4, 64, 77
    i, (_, P64), ctx = _xs_ref(C, B, HW, T)
    H, st = i["heads"], _stats(i, 1)
    Pm, _ = PM.xattn_scores(i, ctx, st)
    zero = torch.zeros(B, H, T, HW, device="cuda")
    P = _xs_run(ops, i, ctx, stats=cu(st), rec=zero)
    once = zero.clone()
    assert torch.equal(_xs_run(ops, i, ctx, stats=cu(st), rec=zero), P) and torch.equal(zero, 2 * once), (C, "two launches onto one recorder")
    for rec_T in (T, T - 1, 20, 1):
        for rows in (rec_T, T + 2):                        # the walk's layout (rows == rec_T) and one with rows behind rec_T
            big = torch.full((B // 2 + 2, H, rows, HW), 0.5, device="cuda")
            old = big.clone()
            got = _xs_run(ops, i, ctx, stats=cu(st), rec=big[1:B // 2 + 1], rec_b0=B // 2, rec_T=rec_T)
            name = f"C={C} b0={B // 2} rec_T={rec_T} of {rows} rows"
            assert torch.equal(got, P), (name, "the recorder changes P")
            assert torch.equal(big[0], old[0]) and torch.equal(big[-1], old[-1]) and torch.equal(big[:, :, rec_T:], old[:, :, rec_T:]), (name, "outside the recorded rows")
            assert torch.equal(big[1:B // 2 + 1, :, :rec_T], 0.5 + once[B // 2:, :, :rec_T]), (name, "old + P in fp32")
            _rec_check("xattn_s_kernel", name, big[1:B // 2 + 1, :, :rec_T], P64, Pm, B // 2, rec_T, base=0.5)


@pytest.mark.parametrize("C", PM.XS_C)
def test_xattn_scores_hand_made_rows_and_products(ops, C):
    """rows of zero variance, an all-zero row and tied keys against the attention; a saturated softmax against the products' own fp64"""
    B, HW, T = 2, 64, 77
    i, (_, P64), ctx = _xs_ref(C, B, HW, T, None, True)
    M, st = B * HW, _stats(i, 1)
    P = _xs_run(ops, i, ctx, stats=cu(st))
    _judge("xattn_s_kernel P", f"C={C} constant and zero rows", P.reshape(M, -1), P64.reshape(M, -1), PM.xattn_scores(i, ctx, st)[1].reshape(M, -1))
    # one dominant token per head: bs made by hand, against the same sums in fp64
    hand = PM.saturated(ctx, T)
    want = PM.xattn_scores(i, hand, rounding=False)[0]
    Pm, Pbm = PM.xattn_scores(i, hand, st)
    rec = torch.zeros(B, i["heads"], T, HW, device="cuda")
    P = _xs_run(ops, i, hand, stats=cu(st), rec=rec)
    _judge("xattn_s_kernel P", f"C={C} saturated", P.reshape(M, -1), want.reshape(M, -1), Pbm.reshape(M, -1))
    _rec_check("xattn_s_kernel", f"C={C} saturated", rec, want, Pm, 0, T)
    # tied keys: identical rows of K'', cs and bs (the special rows included: their logits are bs alone) give bit-equal probabilities
    j = PM.tied_inputs(i)
    _, P64 = PM.xattn_fp64(j)
    ctx = PM.xattn_context_model(j)
    Pm, Pbm = PM.xattn_scores(j, ctx, st)
    rec = torch.zeros(B, i["heads"], T, HW, device="cuda")
    P = _xs_run(ops, j, ctx, stats=cu(st), rec=rec)
    _judge("xattn_s_kernel P", f"C={C} tied keys", P.reshape(M, -1), P64.reshape(M, -1), Pbm.reshape(M, -1))
    _rec_check("xattn_s_kernel", f"C={C} tied keys", rec, P64, Pm, 0, T)
    for a, b in PM.TIED_PAIRS:
        assert torch.equal(P[..., a], P[..., b]) and torch.equal(rec[:, :, a], rec[:, :, b]), (C, "tied keys", a, b)


@pytest.mark.parametrize("ratio", PM.XS_RATIOS)
@pytest.mark.parametrize("C", PM.XS_C)
def test_xattn_scores_with_a_large_mean(ops, C, ratio):
    """|mean| / sigma of the rows = ratio, the sign alternating: 0 and 4 asserted; 32 and 128 asserted where the reference alone keeps the model
    inside the ceiling (tests/test_premul_model_cpu.py prints which), reported otherwise"""
    B, HW, T = PM.XS_RATIO_SHAPE
    i, (_, P64), ctx = _xs_ref(C, B, HW, T, ratio)
    M, st = B * HW, _stats(i, 1)
    Pbm = PM.xattn_scores(i, ctx, st)[1]
    only = ratio > 4 and not PM.inside_ceiling(Pbm.reshape(M, -1), P64.reshape(M, -1))
    P = _xs_run(ops, i, ctx, stats=cu(st))
    _judge("xattn_s_kernel P", f"C={C} ratio={ratio}{' (reported)' if only else ''}", P.reshape(M, -1), P64.reshape(M, -1), Pbm.reshape(M, -1), ratio_only=only)


def test_xattn_scores_refuses(ops, err_type):
    i, _, ctx = _xs_ref(320, 1, 64, 19)
    with pytest.raises(err_type, match="xattn_s"):
        _xs_run(ops, i, ctx, T=81)
    with pytest.raises(err_type, match="xattn_s"):
        _xs_run(ops, dict(i, x=i["x"][:, :32]), ctx)
    with pytest.raises(err_type, match="recorder"):
        _xs_run(ops, i, ctx, rec=torch.zeros(1, 8, 19, 64, device="cuda"), rec_T=20)


# ------------------------------------------------------------------------------------------------------------------------------
# end to end: ops.xattn_premul
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,T,C", PM.E2E_CASES)
def test_xattn_premul_end_to_end(ops, B, HW, T, C):
    i = PM.xattn_inputs(C, B, HW, T)
    y64, P64 = PM.xattn_fp64(i)
    assert PM.residual_condition(y64, i["x"].reshape(-1, C)) >= 1
    m = PM.xattn_model(i)
    y, pr = ops.xattn_premul(cu(i["x"]), cu(i["gamma"]), cu(i["beta"]), cu(i["wq"]), cu(i["kv"]), cu(i["wo"]), cu(i["bo"]), heads=8, return_probs=True)
    name = f"B={B} HW={HW} T={T} C={C}"
    _judge("xattn_premul y", name, y.reshape(B * HW, C).cpu(), y64, m["y"])
    _rec_check("xattn_premul", name, pr, P64, m["P"], 0, T)


# ------------------------------------------------------------------------------------------------------------------------------
# IP-Adapter
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("R,N,K", PM.IPA_LINEAR_CASES)
def test_ipa_linear(ops, R, N, K, bias):
    g = PM.TM.gen(R, N, K, int(bias))
    x, w = torch.randn(R, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    y = ops.ipa_linear(cu(x), cu(w), cu(b)).cpu()
    terms = PM.linear_terms(x, w, b)
    _sum_check("ipa_linear_kernel", f"R={R} N={N} K={K} bias={int(bias)}", y, terms.sum(-1), terms)
    assert torch.equal(y, ops.ipa_linear(cu(x), cu(w), cu(b)).cpu())


@pytest.mark.parametrize("ratio", PM.IPA_LN_RATIOS)
@pytest.mark.parametrize("rows,C", PM.IPA_LN_CASES)
def test_ipa_layernorm(ops, rows, C, ratio):
    x, g, b = PM.layernorm_inputs(rows, C, ratio)
    y = ops.ipa_layernorm(cu(x), cu(g), cu(b), PM.LN_EPS).cpu()
    _judge("ipa_layernorm_kernel", f"rows={rows} C={C} ratio={ratio}", y, PM.layernorm_fp64(x, g, b), PM.layernorm_model(x, g, b), C)
    if rows > 1:
        assert torch.equal(y[1], b), "a constant row is beta"


def _ipa_ctx_run(ops, i, **kw):
    return tuple(t.cpu() for t in ops.ipa_context(cu(i["kip"]), cu(i["vip"]), cu(i["wq"]), cu(i["wo"]), cu(i["gamma"]), cu(i["beta"]), i["heads"], **kw))


@pytest.mark.parametrize("nt", PM.IPA_NT)
@pytest.mark.parametrize("C,heads", PM.IPA_C)
def test_ipa_context_products(ops, C, heads, nt):
    B, cols, live = 2, PM.ipa_cols(heads, nt), heads * nt
    i = PM.ipa_inputs(C, heads, nt, B, 1)
    want, model = PM.ipa_context(i, False), PM.ipa_context(i, True)
    kpp, cs, bs, vpp = got = _ipa_ctx_run(ops, i)
    name = f"C={C} heads={heads} nt={nt} colsP={cols}"
    assert kpp.shape == (B, cols, C) and cs.shape == (B, cols) and vpp.shape == (B, C, cols)
    _judge("ipa_kpp_kernel", name, kpp.reshape(-1, C), want[0].reshape(-1, C), model[0].reshape(-1, C), PM.slab_cols(C))
    _judge("ipa_vpp_kernel", name, vpp.reshape(B * C, cols), want[3].reshape(B * C, cols), model[3].reshape(B * C, cols), cols)
    for nm, t in (("K''", kpp[:, live:]), ("V''", vpp[..., live:]), ("cs", cs[:, live:]), ("bs", bs[:, live:])):
        assert bool((t == 0).all()), (name, nm, "padded columns")
    _sum_check("ipa_csbs_kernel cs", name, cs[:, :live], kpp[:, :live].double().sum(-1), model[0][:, :live])
    k = PM._ip_heads(i)[0]
    _bs_check("ipa_csbs_kernel bs", name, bs[:, :live].reshape(B, heads, nt), want[2][:, :live].reshape(B, heads, nt), k, i["wq"], i["beta"], C // heads)
    for a, b in zip(got, _ipa_ctx_run(ops, i)):
        assert torch.equal(a, b), (name, "second run")


@pytest.mark.parametrize("nt", PM.IPA_NT)
@pytest.mark.parametrize("C,heads", PM.IPA_C)
def test_ipa_scores(ops, C, heads, nt):
    """every HW (1, 16, 64, 100: one ragged tile, a whole one, a second ragged one) at B = 2: P slab by slab, the padded columns zero, a guard
    region behind the buffer untouched, every image alone bit for bit (image 0's ragged tile leaves image 1's rows alone)"""
    B, cols, live, guard = 2, PM.ipa_cols(heads, nt), heads * nt, 64
    for HW in PM.IPA_HW:
        i = PM.ipa_inputs(C, heads, nt, B, HW)
        ctx = PM.ipa_context(i, True)
        _, P64 = PM.ipa_fp64(i, 1.0)
        _, Pbm = PM.ipa_scores(i, ctx)
        name = f"ipa_scores_kernel<{PM.ipa_nt_inst(heads, nt)}> C={C} heads={heads} nt={nt} HW={HW}"
        buf = ops.ipa_scores(cu(i["h"]), cu(ctx[0]), cu(ctx[1]), cu(ctx[2]), heads, nt, PM.LN_EPS, guard_rows=guard).cpu()
        P = buf[:B * HW]
        assert bool((buf[B * HW:] == ops.IPA_SENTINEL).all()), (name, "the guard rows behind P")
        _judge(f"ipa_scores_kernel<{PM.ipa_nt_inst(heads, nt)}>", name, P, P64.reshape(B * HW, cols), Pbm.reshape(B * HW, cols), cols)
        assert bool((P[:, live:] == 0).all()), (name, "padded columns")
        for b in range(B):
            Pb = ops.ipa_scores(cu(i["h"][b:b + 1]), cu(ctx[0][b:b + 1]), cu(ctx[1][b:b + 1]), cu(ctx[2][b:b + 1]), heads, nt, PM.LN_EPS).cpu()
            assert torch.equal(Pb.reshape(HW, cols), P[b * HW:(b + 1) * HW]), (name, "image alone", b)


@pytest.mark.parametrize("C", [72, 320, 1280])
def test_ipa_add(ops, C):
    """h' slab by slab for s = 1 and -0.5 (half the product at least as large as h); s = 0 returns h bit for bit; the guard rows behind h
    untouched; a second identical call on a fresh copy bit for bit"""
    guard = 64
    for HW in PM.IPA_ADD_HW:
        i = PM.ipa_add_inputs(C, HW)
        B = i["B"]
        h2 = i["h"].reshape(B * HW, C)
        for s in PM.IPA_S:
            name = f"C={C} HW={HW} s={s}"
            buf = ops.ipa_add(cu(i["h"]), cu(i["P"]), cu(i["vpp"]), s, guard_rows=guard).cpu()
            assert bool((buf[B * HW:] == ops.IPA_SENTINEL).all()), (name, "the guard rows behind h")
            got = buf[:B * HW]
            assert torch.equal(got, ops.ipa_add(cu(i["h"]), cu(i["P"]), cu(i["vpp"]), s).reshape(B * HW, C).cpu()), (name, "second call")
            if s == 0:
                assert torch.equal(got, h2), (name, "s = 0 returns h")
                continue
            want = PM.ipa_add(i["h"], i["P"], i["vpp"], s, False)
            assert PM.residual_condition(want, h2) >= 1
            _judge("ipa_add_kernel", name, got, want, PM.ipa_add(i["h"], i["P"], i["vpp"], s), PM.slab_cols(C))


def test_ipa_branch_end_to_end_through_the_three_stages(ops):
    """context -> scores -> add on the kernels' own intermediates against the attention itself"""
    for (C, heads), nt in zip(PM.IPA_C, (5, 4, 10)):
        i = PM.ipa_inputs(C, heads, nt, 2, 100)
        kpp, cs, bs, vpp = ops.ipa_context(cu(i["kip"]), cu(i["vip"]), cu(i["wq"]), cu(i["wo"]), cu(i["gamma"]), cu(i["beta"]), heads)
        P = ops.ipa_scores(cu(i["h"]), kpp, cs, bs, heads, nt, PM.LN_EPS)
        for s in (1.0, -0.5):
            y64, _ = PM.ipa_fp64(i, s)
            assert PM.residual_condition(y64, i["h"].reshape(-1, C)) >= 1
            got = ops.ipa_add(cu(i["h"]), P, vpp, s).reshape(-1, C).cpu()
            _judge("ipa branch h'", f"C={C} heads={heads} nt={nt} s={s}", got, y64, PM.ipa_model(i, s)["y"], PM.slab_cols(C))


def test_ipa_launchers_refuse(ops, err_type):
    """colsP - H nt >= 16, colsP > 80 and C % 8 != 0 come back with the launcher's message, and nothing is written"""
    z = lambda *s: torch.zeros(*s, device="cuda")
    out = torch.full((16, 32), ops.IPA_SENTINEL, device="cuda")
    with pytest.raises(err_type, match="ipa scores"):                      # 8 heads x 1 token in 32 columns: a whole tile of padding
        ops.ipa_scores(z(1, 16, 320), z(1, 32, 320), z(1, 32), z(1, 32), 8, 1, out=out)
    assert bool((out == ops.IPA_SENTINEL).all())
    with pytest.raises(err_type, match="ipa scores"):                      # 96 columns
        ops.ipa_scores(z(1, 16, 320), z(1, 96, 320), z(1, 96), z(1, 96), 8, 12)
    with pytest.raises(err_type, match="ipa scores"):                      # C % 8
        ops.ipa_scores(z(1, 16, 68), z(1, 16, 68), z(1, 16), z(1, 16), 4, 4)
    with pytest.raises(err_type, match="ipa premul"):
        ops.ipa_context(z(1, 12, 320), z(1, 12, 320), z(320, 320), z(320, 320), z(320), z(320), 8)
    with pytest.raises(err_type, match="ipa premul"):
        ops.ipa_context(z(1, 1, 320), z(1, 1, 320), z(320, 320), z(320, 320), z(320), z(320), 8, cols=8)
    with pytest.raises(err_type, match="ipa premul"):
        ops.ipa_context(z(1, 4, 68), z(1, 4, 68), z(68, 68), z(68, 68), z(68), z(68), 4)
    with pytest.raises(err_type, match="ipa add"):
        ops.ipa_add(z(1, 16, 320), z(1, 16, 96), z(1, 320, 96), 1.0)
    with pytest.raises(err_type, match="ipa add"):
        ops.ipa_add(z(1, 16, 68), z(1, 16, 16), z(1, 68, 16), 1.0)
