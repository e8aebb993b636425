"""The row-panel transformer-block kernels of csrc/tblock.hip, each on its own: `qkv_chain_kernel` / `qkv_chain2_kernel` (six
instantiations), `ff_fused_kernel<320, 0, POST>` (three) and `attn_chain_kernel<C, PRE, MI>` (six), through `agd_op_qkv_chain`,
`agd_op_ff_fused_ex` and `agd_op_attn_chain_ex`, which reach every form the launchers have.

Reference: tests/_tblock_model.py, fp64 on the bf16-rounded inputs.  Measure: every slab of 16 rows x 80 columns on its own (one MFMA row
tile of one wave's column range): max |error| / max |slab| and RMS error / RMS slab, so that no row tile, wave, column quarter, panel or image
hides behind another.  Bound, per case and from the reference alone: the model restates the roundings the kernels declare; its worst slab
against fp64 is E_model (max) / E_rms, the kernel must stay within MODEL_FACTOR = 2 x each, and no case may have 2 x E_model above 2^-6.
Outputs that carry a residual (y, pout) are judged on inputs whose increment is at least as large as the residual (asserted from the
reference).  Recorder rows, `colstat` and `rowstat_out` have absolute bounds taken from the model in the same way.  Where two launches must do
the same arithmetic (`sched2`, `rows64`, a batch against its images, in place, shared input rows against duplicated ones, a second run) the
outputs are compared bit for bit.

Which instantiation a case runs is not returned by the launchers; every case records the one it expects, by the launchers' rules:
  qkv chain   `qkv_chain_kernel` (`sched2`: `qkv_chain2_kernel`) `<320, 2>` on 128-row panels, `<320, 1>` with `rows64`, `<640, 1>` at C = 640.
  ff_fused    `ff_fused_kernel<320, 0, POST>`: POST = 0 without a proj_out matrix, 1 with it, 2 with it and `premul`.
  attn_chain  `attn_chain_kernel<C, PRE, MI>`: PRE = 1 with o1; MI = 2 (32-row panels) at C = 640 with `rows32`, fewer than 200 64-row panels
              and HW % 32 == 0, else MI = 4 (C = 320: 128-row panels, C = 640: 64-row panels).

What the proj_out forms of ff_fused require of M: nothing beyond M >= 1.  The launcher rounds the grid up to whole 128-row panels; the
kernel loads rows >= M as zeros, reads residual row 0 for them, stores none of them and leaves them out of `colstat`, which has
ceil(M / 128) tiles -- so the ragged M = 1000 runs through POST = 1 and 2 as well, and is asserted here.

Large row mean (|mean| / sigma = 0, 4, 32 asserted; 128 and 512 measured and reported with the ratio the rounded inputs really have).  The
chains take LayerNorm statistics in one fp32 pass (Q / C - mu^2), whose relative error in the variance grows like a few times
2^-24 (1 + ratio^2): 6e-5 at 32, 1e-3 at 128, 1.6e-2 and more at 512.  Measured on an MI355X (kernel / model, max-measure, MEASURED_LARGE_MEAN):
at most 1.15 up to 32 (inside the bound of 2), 1.19 at 128, and 4 to 9 at 512, where the kernels' error is 2 to 4 per cent of a slab's
largest value.  Rows of the UNet's residual stream stay far below that (|mean| / sigma of a few units); nothing changes in the kernels.  For the qkv chain the rows' mean is the GroupNorm's (per image and group, fp64 in the kernel); norm1 inside it
reads h, which the kernel itself has rounded to bf16, so a mean of ratio x sigma there costs ratio x 2^-8 / sqrt(12) of sigma in the model
already and cannot be driven past ~4 under the ceiling: its one-pass form is the same expression as the other two chains'.

MEASURED_RATIOS below records kernel error / model error as measured on an MI355X."""
import functools

import pytest
import torch
import _tblock_model as TM
from _report import report
from _tblock_model import MODEL_FACTOR

pytestmark = pytest.mark.gpu

# kernel error / model error (max-measure, rms-measure): the worst case of each kernel over this file (the large-mean cases apart), measured
# on an MI355X.  The worst slab of every kernel is the model's own worst slab, element for element; the RMS shows the fp32 accumulation and
# the polynomial erf / hardware exp2 that the model leaves out.  The `sched2` and `rows64` kernels are bit-identical to their plain forms.
MEASURED_RATIOS = {
    "qkv_chain_kernel<320, 2> h": (1.0000, 1.0000), "qkv_chain_kernel<320, 2> qkv": (1.0000, 1.0000),
    "qkv_chain_kernel<320, 1> h": (1.0000, 1.0000), "qkv_chain_kernel<320, 1> qkv": (1.0000, 1.0000),
    "qkv_chain_kernel<640, 1> h": (1.0000, 1.0000), "qkv_chain_kernel<640, 1> qkv": (1.0000, 1.0000),
    "qkv_chain2_kernel<320, 2> / <320, 1> / <640, 1>": "bit-identical to qkv_chain_kernel",
    "ff_fused_kernel<320, 0, 0>": (1.0000, 1.0009), "ff_fused_kernel<320, 0, 1>": (1.0000, 1.0077), "ff_fused_kernel<320, 0, 2>": (1.0000, 1.0009),
    "attn_chain_kernel<320, 0, 4> y": (1.0000, 1.0018), "attn_chain_kernel<320, 1, 4> y": (1.0000, 1.0045), "attn_chain_kernel<320, 1, 4> h1": (1.0000, 1.0000),
    "attn_chain_kernel<640, 0, 4> y": (1.0000, 1.0005), "attn_chain_kernel<640, 1, 4> y": (1.0000, 1.0016), "attn_chain_kernel<640, 1, 4> h1": (1.0000, 1.0000),
    "attn_chain_kernel<640, 0, 2> y": (1.0000, 1.0100), "attn_chain_kernel<640, 1, 2> y": (1.0000, 1.0000), "attn_chain_kernel<640, 1, 2> h1": (1.0000, 1.0000),
}
# |mean| / sigma -> kernel / model (max-measure), the worst form of each chain, measured on an MI355X (the rounded inputs of the two reported
# ratios really have 125 and 521: bf16 rounding of a row whose mean is hundreds of sigma widens sigma)
MEASURED_LARGE_MEAN = {
    "qkv_chain (the GroupNorm's mean, fp64 sums)": {0: 1.000, 4: 1.000, 32: 1.000, 128: 1.000, 512: 1.041},
    "ff_fused (norm3, one fp32 pass)": {0: 1.000, 4: 1.000, 32: 1.000, 128: 1.193, 512: 9.219},
    "attn_chain (norm2, one fp32 pass)": {0: 1.000, 4: 1.000, 32: 1.152, 128: 1.193, 512: 5.498},
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
    return None if t is None else t.cuda()


def _judge(kind, name, got, want, model, ratio_only=False):
    """[M, N] operands -> (kernel max / model max, kernel rms / model rms)"""
    e_model, e_rms = TM.model_bounds(model, want) if not ratio_only else tuple(float(v.max()) for v in TM.slab_errors(TM.slabs(model), TM.slabs(want)))
    got = got.detach().double().cpu()
    k_max, k_rms = TM.kernel_errors(got, want, model)
    print(f"{kind}[{name}]: worst slab max {k_max:.6f} (E_model {e_model:.6f}), rms {k_rms:.6f} (E_rms {e_rms:.6f})")
    report(f"tblock_ops[{kind} {name}]", kernel_max=k_max, model_max=e_model, kernel_rms=k_rms, model_rms=e_rms)
    assert bool(torch.isfinite(got).all()), name
    if not ratio_only:
        assert k_max <= MODEL_FACTOR * e_model, (kind, name, "max", k_max, e_model)
        assert k_rms <= MODEL_FACTOR * e_rms, (kind, name, "rms", k_rms, e_rms)
    return k_max / e_model, k_rms / e_rms


def _sums_check(name, table, values, dim, model_values, depth=None):
    """table [..., 2] = (sum, sum of squares) of `values` (the kernel's own bf16 output) along dim: exact up to fp32 summation, measured relative
    to sum |terms|.  colstat (depth None): bounded by what the model's values lose in two other fp32 summation orders (a running sum and torch's
    blocked one).  rowstat: bounded by the standard bound of an fp32 sum whose longest chain of additions is `depth`, depth x 2^-24 (the squares
    one more, for the product) -- the kernel adds a lane's 20 values four at a time ((a + b) + (c + d), then onto the running sum: 7 deep), two
    shuffle levels, and the C / 80 column ranges in sequence (<= 8): 17."""
    v = values.double().cpu()
    t = table.double().cpu()
    for k, (vv, mm) in enumerate(((v, model_values), (v * v, model_values * model_values))):
        e_other, _ = TM.fp32_sum_error(mm.double(), dim)
        bound = MODEL_FACTOR * e_other if depth is None else (depth + k) * 2.0 ** -24
        err = float(((t[..., k] - vv.sum(dim)).abs() / vv.abs().sum(dim)).max())
        print(f"{name} {'sum' if k == 0 else 'sum of squares'}: {err:.3e} of sum |terms| (bound {bound:.3e}; fp32 in other orders {e_other:.3e})")
        assert err <= bound, (name, k, err, bound)


# ------------------------------------------------------------------------------------------------------------------------------
# qkv chain
# ------------------------------------------------------------------------------------------------------------------------------
def qkv_inst(C, rows64, sched2):
    return f"qkv_chain{'2' if sched2 else ''}_kernel<{C}, {1 if C == 640 or rows64 else 2}>"


@functools.lru_cache(maxsize=4)
def _qkv_ref(C, B, HW, groups, ratio=None):
    i = TM.qkv_inputs(C, B, HW, groups) if ratio is None else TM.qkv_inputs(C, B, HW, groups, 9, ratio=ratio)
    return i, TM.qkv_fp64(i), {True: TM.qkv_model(i, True), False: TM.qkv_model(i, False)}


def _qkv_run(ops, i, bm, inside, rows64=False, sched2=False, images=None, hw=None, part=None, groups=None, x=None):
    xx = i["x"] if images is None else i["x"][images]
    B, HW, C = xx.shape
    part = TM.partials(xx.double(), bm) if part is None else part
    x2 = xx.reshape(B * HW, C) if x is None else x
    h, qkv = ops.qkv_chain(cu(x2), HW if hw is None else hw, cu(i["gn_gamma"]), cu(i["gn_beta"]), i["groups"] if groups is None else groups, cu(part), bm,
                           cu(i["w_in"]), cu(i["b_in"]), cu(i["gamma"]), cu(i["beta"]), cu(i["wqkv"]), gn_eps=TM.GN_EPS, ln_eps=TM.LN_EPS,
                           inside=inside, rows64=rows64, sched2=sched2)
    return h.cpu(), qkv.cpu()


def _qkv_forms(C, HW):
    """(rows64, sched2) of every launch form the shape admits"""
    if C == 640:
        return [(False, False), (False, True)]
    return [(r, s) for r in (False, True) for s in (False, True) if r or HW % 128 == 0]


@pytest.mark.parametrize("C,B,HW,bm,groups", TM.QKV_SHAPES_320 + TM.QKV_SHAPES_640)
def test_qkv_chain_every_form(ops, C, B, HW, bm, groups):
    """{folded, inside} x {128-row, rows64} x {sched2 off, on} at C = 320, {folded, inside} x {sched2} at C = 640: each GroupNorm form against
    its model, and within a form every panel height and schedule bit for bit"""
    i, (h64, q64), model = _qkv_ref(C, B, HW, groups)
    for inside in (False, True):
        first = None
        for rows64, sched2 in _qkv_forms(C, HW):
            h, q = _qkv_run(ops, i, bm, inside, rows64, sched2)
            name = f"{qkv_inst(C, rows64, sched2)} {'inside' if inside else 'folded'} B={B} HW={HW} bm={bm} groups={groups}"
            if first is None:
                first = (h, q)
                _judge("qkv_chain h", name, h, h64, model[inside][0])
                _judge("qkv_chain qkv", name, q, q64, model[inside][1])
            else:
                assert torch.equal(h, first[0]) and torch.equal(q, first[1]), name      # rows64 / sched2: the same arithmetic
                report(f"tblock_ops[qkv_chain {name}]", bit_identical=1)


@pytest.mark.parametrize("C", [320, 640])
def test_qkv_chain_batch_against_its_images_and_a_second_run(ops, C):
    B, HW, bm, groups = 3, 128, 64, 32
    i, _, _ = _qkv_ref(C, B, HW, groups)
    for inside in (False, True):
        for rows64, sched2 in _qkv_forms(C, HW):
            h, q = _qkv_run(ops, i, bm, inside, rows64, sched2)
            h2, q2 = _qkv_run(ops, i, bm, inside, rows64, sched2)
            assert torch.equal(h, h2) and torch.equal(q, q2)
            for b in range(B):
                hb, qb = _qkv_run(ops, i, bm, inside, rows64, sched2, images=slice(b, b + 1))
                assert torch.equal(hb, h[b * HW:(b + 1) * HW]) and torch.equal(qb, q[b * HW:(b + 1) * HW]), (qkv_inst(C, rows64, sched2), inside, b)


QKV_REFUSALS = [(w, f) for w in ("HW % BM", "M % HW", "C % groups", "HW % bm", "C = 1280") for f in (False, True)] + [("groups > 32", True)]


@pytest.mark.parametrize("what,inside", QKV_REFUSALS)
def test_qkv_chain_refuses(ops, err_type, what, inside):
    """(more than 32 groups is the limit of the kernel's own GroupNorm; the folded form's launch_gn_fold_weight takes up to 64)"""
    i, _, _ = _qkv_ref(320, 3, 128, 32)
    rows = i["x"].reshape(-1, 320)
    if what == "HW % BM":               # 384 rows as two images of 192 on 128-row panels: M % 128 == 0 and M % HW == 0, HW % 128 != 0
        kw = {"x": rows, "hw": 192, "part": TM.partials(i["x"].double().reshape(2, 192, 320), 64)}
    elif what == "M % HW":              # 192 rows of images of 128 on 64-row panels: M % 64 == 0 and HW % 64 == 0
        kw = {"x": rows[:192].contiguous(), "hw": 128, "rows64": True}
    elif what == "groups > 32":
        kw = {"groups": 64}
    elif what == "C % groups":
        kw = {"groups": 7}
    elif what == "HW % bm":
        kw = {"bm": 48, "part": TM.partials(i["x"].double(), 64)}
    else:
        z = torch.zeros
        with pytest.raises(err_type):
            ops.qkv_chain(cu(z(128, 1280)), 128, cu(z(1280)), cu(z(1280)), 32, cu(z(1, 2, 1280, 2)), 64, cu(z(1280, 1280)), cu(z(1280)), cu(z(1280)), cu(z(1280)),
                          cu(z(3840, 1280)), inside=inside)
        return
    with pytest.raises(err_type):
        _qkv_run(ops, i, kw.pop("bm", 64), inside, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# feed-forward
# ------------------------------------------------------------------------------------------------------------------------------
def ff_inst(post):
    return f"ff_fused_kernel<320, 0, {post}>"


@functools.lru_cache(maxsize=2)
def _ff_ref(name, ratio=None):
    if ratio is not None:
        i = TM.ff_inputs(TM.FF_RATIO_M, 9, ratio=ratio)
    else:
        _, M, _, kw = [c for c in TM.FF_CASES if c[0] == name][0]
        i = TM.ff_inputs(M, **kw)
    y, pout = TM.ff_fp64(i, True)
    return i, y, pout, {p: TM.ff_model(i, p) for p in (0, 1, 2)}


def _ff_run(ops, i, post, colstat=False, inplace=False):
    kw = {}
    if post:
        kw = {"wp": cu(i["wp"]), "bp": cu(i["bp"]), "xres": cu(i["xres"]), "xres_rows": i["xres_rows"], "premul": post == 2}
    return ops.ff_fused_ex(cu(i["x"]), cu(i["gamma"]), cu(i["beta"]), cu(i["w1"]), cu(i["b1"]), cu(i["w2"]), cu(i["b2"]), TM.LN_EPS, colstat=colstat,
                           inplace=inplace, **kw)


@pytest.mark.parametrize("name,M,posts", [c[:3] for c in TM.FF_CASES])
def test_ff_fused_every_form(ops, name, M, posts):
    """POST 0 / 1 / 2, with and without colstat, in place against out of place and a second run bit for bit"""
    i, y64, p64, model = _ff_ref(name)
    assert TM.residual_condition(y64, i["x"]) >= 1 and TM.residual_condition(p64, i["xres"]) >= 1
    for post in posts:
        got = _ff_run(ops, i, post).cpu()
        _judge("ff_fused", f"{ff_inst(post)} {name} M={M}", got, y64 if post == 0 else p64, model[post])
        assert torch.equal(got, _ff_run(ops, i, post, inplace=True).cpu()), (name, post, "in place")
        assert torch.equal(got, _ff_run(ops, i, post).cpu()), (name, post, "second run")
        if post:
            got2, cst = _ff_run(ops, i, post, colstat=True)
            assert torch.equal(got, got2.cpu()), (name, post, "colstat changes pout")
            tiles = (M + 127) // 128
            pad = torch.zeros(tiles * 128, 320, dtype=torch.float64)
            padm = pad.clone()
            pad[:M] = got.double()
            padm[:M] = model[post]
            _sums_check(f"ff_fused colstat {ff_inst(post)} {name}", cst, pad.reshape(tiles, 128, 320), 1, padm.reshape(tiles, 128, 320))


def test_ff_premul_product_is_one_rounding_from_fp64(ops):
    """the pre-multiplied matrix the wrapper builds as the loader does (the library's GEMM, rounded to bf16 once) against the fp64 product: within
    one bf16 rounding (2^-8 relative: eight bits of significand) plus the GEMM's fp32 accumulation, which is far below it; the bias within fp32 rounding"""
    i, _, _, _ = _ff_ref("one panel")
    w2p, bcp = ops.ff_premul_weights(cu(i["w2"]), cu(i["b2"]), cu(i["wp"]), cu(i["bp"]))
    want_w, want_b = TM.premul_fp64(i)
    err = (w2p.double().cpu() - want_w).abs()
    assert bool((err <= want_w.abs() * 2.0 ** -8 + 320 * 2.0 ** -24 * want_w.abs().max()).all()), float((err / want_w.abs().max()).max())
    assert bool(((bcp.double().cpu() - want_b).abs() <= want_b.abs() * 2.0 ** -24 + 1e-30).all())


def test_ff_fused_refuses(ops, err_type):
    i, _, _, _ = _ff_ref("one panel")
    a = [cu(i[k]) for k in ("x", "gamma", "beta", "w1", "b1", "w2", "b2")]
    with pytest.raises(err_type):                                       # the proj_out stage without its residual
        ops.ff_fused_ex(*a, wp=cu(i["wp"]), bp=cu(i["bp"]))
    with pytest.raises(err_type):                                       # ... without its bias
        ops.ff_fused_ex(*a, wp=cu(i["wp"]), xres=cu(i["xres"]))
    with pytest.raises(err_type):                                       # colstat belongs to the proj_out stage
        ops.ff_fused_ex(*a, colstat=True)
    with pytest.raises(err_type):                                       # C = 640 is not built
        ops.ff_fused_ex(cu(torch.zeros(128, 640)), *[cu(torch.zeros(s)) for s in ((640,), (640,), (5120, 640), (5120,), (640, 2560), (640,))])


# ------------------------------------------------------------------------------------------------------------------------------
# attention chain
# ------------------------------------------------------------------------------------------------------------------------------
def attn_inst(C, pre, rows32, M, HW):
    mi = 2 if (C == 640 and rows32 and M // 64 < 200 and HW % 32 == 0) else 4
    return f"attn_chain_kernel<{C}, {int(pre)}, {mi}>"


@functools.lru_cache(maxsize=2)
def _attn_ref(C, B, HW, T, pre=False, src_rows=0, peaked=False, ratio=None):
    i = TM.attn_inputs(C, B, HW, T, *((9,) if ratio is not None else ()), ratio=ratio, pre=pre, src_rows=src_rows, peaked=peaked)
    return i, TM.attn_fp64(i), TM.attn_model(i)


def _attn_run(ops, i, rows32=False, dup=False, heads=8, **kw):
    """dup: the shared input rows physically duplicated (src_rows = 0)"""
    B, HW, C = i["B"], i["HW"], i["x"].shape[-1]
    src = i["src_rows"] if not dup else 0
    shape = (lambda t: t) if src else (lambda t: TM._expand(i, t).float().reshape(B, HW, C))
    if "o1" in i:
        kw.update(o1=cu(shape(i["o1"])), wo1=cu(i["wo1"]), bo1=cu(i["bo1"]))
    return ops.attn_chain_ex(cu(shape(i["x"])), cu(i["gamma"]), cu(i["beta"]), cu(i["wq"]), cu(i["kv"]), cu(i["wo"]), cu(i["bo"]), heads, TM.LN_EPS,
                             hw=HW, src_rows=src, rows32=rows32, **kw)


def _rec_check(name, rec, P64, Pm, hpb, b0=0, T=None, base=0.0):
    want, mod = TM.recorder_rows(P64, hpb, b0, T), TM.recorder_rows(Pm, hpb, b0, T)
    bound = TM.abs_bound(mod, want, hpb)
    err = float((rec.double().cpu() - base - want).abs().max())
    print(f"attn_chain recorder {name} hpb={hpb}: max abs error {err:.3e} (bound {bound:.3e})")
    report(f"tblock_ops[attn_chain recorder {name} hpb={hpb}]", max_abs=err, bound=bound)
    assert err <= bound, (name, hpb, err, bound)


@pytest.mark.parametrize("T", TM.ATTN_T)
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("C,rows32", TM.ATTN_FORMS)
def test_attn_chain_every_form(ops, C, rows32, pre, T):
    """two images with their own contexts, two panels each: y (and h1 with the prologue), the row statistics of the kernel's own output, the
    probabilities summed over all heads; in place (PRE = 0) and a second run bit for bit"""
    B, HW = 2, 2 * TM.attn_bm(C, rows32)
    i, (y64, h64, P64), (ym, hm, Pm) = _attn_ref(C, B, HW, T, pre)
    assert TM.residual_condition(y64, h64) >= 1
    name = f"{attn_inst(C, pre, rows32, B * HW, HW)} T={T}"
    rec = torch.zeros(B, 1, T, HW, device="cuda")
    out = _attn_run(ops, i, rows32, rowstat=True, rec=rec, rec_hpb=8)
    y = out["y"].reshape(B * HW, C).cpu()
    _judge("attn_chain y", name, y, y64, ym)
    if pre:
        _judge("attn_chain h1", name, out["h1"].reshape(B * HW, C).cpu(), h64, hm)
    _sums_check(f"attn_chain rowstat {name}", out["rowstat"].reshape(B * HW, 2), y, 1, ym, depth=17)
    _rec_check(name, rec, P64, Pm, 8)
    again = _attn_run(ops, i, rows32)
    assert torch.equal(again["y"].reshape(B * HW, C).cpu(), y), (name, "second run, and neither recorder nor row statistics change y")
    if not pre:
        assert torch.equal(_attn_run(ops, i, rows32, inplace=True)["y"].reshape(B * HW, C).cpu(), y), (name, "in place")


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("C,rows32", TM.ATTN_FORMS)
def test_attn_chain_shared_input_rows(ops, C, rows32, pre):
    """src_rows = M / 2 (both images read the same rows, each with its own context) against physically duplicated inputs: bit for bit, and
    against the model"""
    B, HW, T = 2, 2 * TM.attn_bm(C, rows32), 77
    i, (y64, h64, _), (ym, hm, _) = _attn_ref(C, B, HW, T, pre, HW)
    name = f"{attn_inst(C, pre, rows32, B * HW, HW)} src_rows={HW}"
    a, b = _attn_run(ops, i, rows32, rowstat=True), _attn_run(ops, i, rows32, dup=True, rowstat=True)
    for k in a:
        assert torch.equal(a[k], b[k]), (name, k)
    _judge("attn_chain y", name, a["y"].reshape(B * HW, C).cpu(), y64, ym)
    if pre:
        _judge("attn_chain h1", name, a["h1"].reshape(B * HW, C).cpu(), h64, hm)


@pytest.mark.parametrize("C,rows32", TM.ATTN_FORMS)
def test_attn_chain_recorder_forms(ops, C, rows32):
    """head groups of 1 / 2 / 4 / 8 against the fp64 probabilities; every group's rows sum to hpb; rec_b0 = 1 and rec_T < T leave everything
    else of a sentinel-filled buffer alone; the recorder adds onto what the buffer holds"""
    B, HW, T = 2, 2 * TM.attn_bm(C, rows32), 77
    i, (_, _, P64), (_, _, Pm) = _attn_ref(C, B, HW, T)
    name = attn_inst(C, False, rows32, B * HW, HW)
    for hpb in (1, 2, 4, 8):
        rec = torch.zeros(B, 8 // hpb, T, HW, device="cuda")
        _attn_run(ops, i, rows32, rec=rec, rec_hpb=hpb)
        _rec_check(name, rec, P64, Pm, hpb)
        # a head's probabilities are p_t / sum p with the sum taken in fp32 over 96 slots: each sums to 1 within (96 + 8) x 2^-24, hpb of them to hpb
        assert float((rec.double().sum(2) - hpb).abs().max()) <= hpb * 104 * 2.0 ** -24, hpb
        once = rec.clone()
        _attn_run(ops, i, rows32, rec=rec, rec_hpb=hpb)
        assert torch.equal(rec, 2 * once), (name, hpb, "two calls onto one buffer")              # p + p is exact
    for hpb in (2, 8):
        # rec_b0 = 1, rec_T = 40 of 43 rows, inside a larger sentinel-filled allocation: only image 1's first 40 token rows change
        big = torch.full((3, 8 // hpb, 43, HW), 0.5, device="cuda")
        _attn_run(ops, i, rows32, rec=big[1:2], rec_hpb=hpb, rec_b0=1, rec_T=40)
        assert bool((big[0] == 0.5).all()) and bool((big[2] == 0.5).all()) and bool((big[1, :, 40:] == 0.5).all()), (name, hpb, "outside the recorded rows")
        _rec_check(name + " b0=1 T=40 prefilled", big[1:2, :, :40], P64, Pm, hpb, 1, 40, base=0.5)


@pytest.mark.parametrize("C,rows32", TM.ATTN_FORMS)
def test_attn_chain_where_the_row_maximum_matters(ops, C, rows32):
    """image 0: key 0's logits about 40 above the rest; image 1: every logit of a row equal"""
    B, HW, T = 2, 2 * TM.attn_bm(C, rows32), 77
    i, (y64, h64, P64), (ym, _, Pm) = _attn_ref(C, B, HW, T, peaked=True)
    assert float(P64[0, :, :, 0].min()) > 0.999 and float((P64[1] - 1.0 / T).abs().max()) < 1e-12
    name = f"{attn_inst(C, False, rows32, B * HW, HW)} peaked"
    rec = torch.zeros(B, 8, T, HW, device="cuda")
    out = _attn_run(ops, i, rows32, rec=rec, rec_hpb=1)
    _judge("attn_chain y", name, out["y"].reshape(B * HW, C).cpu(), y64, ym)
    _rec_check(name, rec, P64, Pm, 1)


def test_attn_chain_refuses(ops, err_type):
    i, _, _ = _attn_ref(320, 2, 256, 77)
    ip, _, _ = _attn_ref(320, 2, 256, 77, True)
    isrc, _, _ = _attn_ref(320, 2, 256, 77, False, 256)
    for T in (0, 97):
        j = dict(i, kv=torch.zeros(2, T, 640), T=T)
        with pytest.raises(err_type):
            _attn_run(ops, j)
    with pytest.raises(err_type):
        _attn_run(ops, i, heads=4)
    with pytest.raises(err_type):
        _attn_run(ops, ip, inplace=True)
    with pytest.raises(err_type):
        _attn_run(ops, isrc, inplace=True)
    with pytest.raises(err_type):
        _attn_run(ops, i, rec=torch.zeros(2, 2, 77, 256, device="cuda"), rec_hpb=3)


# ------------------------------------------------------------------------------------------------------------------------------
# a large row mean
# ------------------------------------------------------------------------------------------------------------------------------
def _row_ratio(x):
    x = x.double().reshape(-1, x.shape[-1])
    return float((x.mean(1).abs() / x.std(1)).median())


@pytest.mark.parametrize("ratio", TM.RATIOS_ASSERTED + TM.RATIOS_REPORTED)
def test_statistics_with_a_large_mean(ops, ratio):
    """|mean| / sigma of the rows (qkv chain: of every (image, group)) = ratio, the sign alternating; asserted to 32, reported beyond"""
    only = ratio in TM.RATIOS_REPORTED
    seen = {}
    for C in (320, 640):
        _, B, HW, bm, groups = TM.QKV_RATIO_SHAPE[C]
        i, (h64, q64), model = _qkv_ref(C, B, HW, groups, ratio)
        xs = i["x"].double().reshape(B, HW, groups, -1).permute(0, 2, 1, 3).reshape(B, groups, -1)
        real = float((xs.mean(-1).abs() / xs.std(-1)).median())
        for inside in (False, True):
            h, q = _qkv_run(ops, i, bm, inside, sched2=inside)
            name = f"{qkv_inst(C, False, inside)} {'inside' if inside else 'folded'} ratio={ratio} (rounded inputs: {real:.1f})"
            seen[("qkv", C, inside)] = max(_judge("qkv_chain h", name, h, h64, model[inside][0], only)[0], _judge("qkv_chain qkv", name, q, q64, model[inside][1], only)[0])
    i, y64, p64, model = _ff_ref(None, ratio)
    for post in (0, 1, 2):
        name = f"{ff_inst(post)} ratio={ratio} (rounded inputs: {_row_ratio(i['x']):.1f})"
        seen[("ff", post)] = _judge("ff_fused", name, _ff_run(ops, i, post).cpu(), y64 if post == 0 else p64, model[post], only)[0]
    for C, rows32 in TM.ATTN_FORMS:
        B, HW = 1, 2 * TM.attn_bm(C, rows32)
        i, (y64, _, _), (ym, _, _) = _attn_ref(C, B, HW, 77, ratio=ratio)
        name = f"{attn_inst(C, False, rows32, B * HW, HW)} ratio={ratio} (rounded inputs: {_row_ratio(i['x']):.1f})"
        seen[("attn", C, rows32)] = _judge("attn_chain y", name, _attn_run(ops, i, rows32)["y"].reshape(B * HW, C).cpu(), y64, ym, only)[0]
    print(f"large mean {ratio}: kernel / model (max-measure) " + ", ".join(f"{k}: {v:.3f}" for k, v in seen.items()))
    report(f"tblock_ops[large mean {ratio}]", **{"_".join(str(p) for p in k): v for k, v in seen.items()})
