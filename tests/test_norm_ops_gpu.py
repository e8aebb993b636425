"""Every kernel of csrc/norm.hip on its own: the three `layernorm_kernel<LPR, MAXV>` instantiations, the two-kernel GroupNorm
(`gn_stats_kernel` + `gn_apply_kernel`) on one source and on the channel concat x0 | x1, `gn_apply_part_kernel` on partial-sum tables made
by the test (so that it is separated from the conv that makes them in production, and the two sources may bring different tile heights),
and `gn_fold_weight_kernel` piece by piece (Wb, rowadd, the fragment order, the folded projection).  Every case asserts which kernel ran.

Reference: tests/_norm_model.py, fp64 on the bf16-rounded inputs.  Measure: every slab on its own -- GroupNorm (image, group), LayerNorm
row, folded projection (image, block of 16 output columns) -- max |error| / max |slab| and RMS error / RMS slab, so that one wrong group,
image or row cannot hide behind a larger one.  Bound, per case and from the reference alone: the model of the same file restates the
roundings the kernels declare; its worst slab against fp64 is E_model (max) / E_rms, the kernel must stay within MODEL_FACTOR = 2 x each,
and no case may have 2 x E_model above 2^-6.  Inputs give every (image, group) or row its own mean (up to one sigma) and its own scale
(2^-2 .. 2^2); gamma and beta are random around 1 and 0.1.  Where two launches must do the same arithmetic (rows permuted, a batch against
its images, a second run) the outputs are compared bit for bit.

MEASURED_RATIOS below records kernel error / model error as measured on an MI355X."""
import pytest
import torch
from _norm_model import (MODEL_FACTOR, ROWADD_TOL, bfr, fold_fp64, fold_model, fold_slabs, gn_slabs, groupnorm_fp64, groupnorm_model,
                         layernorm_fp64, layernorm_model, ln_slabs, model_bounds, nhwc, partials, slab_errors)
from _report import report

pytestmark = pytest.mark.gpu

PART, TWO = 1, 2            # ops.group_norm(..., return_path=True)
BF16_ULP = 2.0 ** -7        # of the largest value, as tests/test_ops_gpu.py compares the two GroupNorm paths

# kernel error / model error (max-measure, rms-measure): the worst case of each kernel over this file, measured on an MI355X.  The kernels
# finalize their statistics in fp64 and then do exactly the model's arithmetic, so nearly every element is the model's bit for bit.
MEASURED_RATIOS = {
    "layernorm_kernel<64,4>": (1.0000, 1.0000), "layernorm_kernel<16,5>": (1.0000, 1.0000), "layernorm_kernel<16,10>": (1.0000, 1.0000),
    "gn_stats_kernel + gn_apply_kernel": (1.0000, 1.0000), "gn_apply_part_kernel": (1.0000, 1.0000),
    "gn_fold_weight_kernel + per-image GEMM": (1.0007, 1.0001),
}


@pytest.fixture(scope="module")
def ops():
    from agenda_amd import ops as o
    return o


@pytest.fixture(scope="module")
def err_type():
    from agenda_amd._lib import AgendaHipError
    return AgendaHipError


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _affine(C, g):
    return torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.2 + 0.1


def _judge(kind, name, got, want, model, ratio_only=False):
    """got / want / model slab-major.  -> (kernel max / model max, kernel rms / model rms)"""
    e_model, e_rms = model_bounds(model, want)
    mx, rms = slab_errors(got, want, model)
    k_max, k_rms = float(mx.max()), float(rms.max())
    print(f"{kind}[{name}]: worst slab max {k_max:.6f} (E_model {e_model:.6f}), rms {k_rms:.6f} (E_rms {e_rms:.6f})")
    report(f"norm_ops[{kind} {name}]", kernel_max=k_max, model_max=e_model, kernel_rms=k_rms, model_rms=e_rms)
    assert bool(torch.isfinite(got).all()), name
    if not ratio_only:
        assert k_max <= MODEL_FACTOR * e_model, (name, "max", k_max, e_model)
        assert k_rms <= MODEL_FACTOR * e_rms, (name, "rms", k_rms, e_rms)
    return k_max / e_model, k_rms / e_rms


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------
def _ln_inputs(rows, C, *seed, ratio=None):
    g = _gen(rows, C, *seed)
    z = torch.randn(rows, C, generator=g)
    sig = 2.0 ** torch.randint(-2, 3, (rows, 1), generator=g).float()
    mu = torch.randn(rows, 1, generator=g).clamp(-2, 2) * 0.5 if ratio is None else torch.full((rows, 1), float(ratio)) * (1 - 2 * (torch.arange(rows)[:, None] % 2))
    ga, be = _affine(C, g)
    return bfr((z + mu) * sig), ga, be


def _ln_check(ops, name, x, ga, be, eps, inst, ratio_only=False):
    got, ran = ops.layer_norm(x.cuda(), ga.cuda(), be.cuda(), eps, return_path=True)
    assert ran == inst, (name, ran)
    return got, _judge("layernorm", name, ln_slabs(got), layernorm_fp64(x, ga, be, eps), layernorm_model(x, ga, be, eps), ratio_only)


LN_CASES = [((64, 4), r, c) for r, c in ((7, 8), (33, 320), (10, 1280), (5, 2048), (8200, 1344))] + \
           [((16, 5), r, c) for r, c in ((8192, 64), (8200, 320), (8195, 640), (8193, 8))] + \
           [((16, 10), r, c) for r, c in ((8200, 648), (8197, 960), (8192, 1280))]


@pytest.mark.parametrize("inst,rows,C", LN_CASES)
def test_layernorm_instantiations(ops, inst, rows, C):
    """`<64,4>` below 8192 rows or above 1280 channels, `<16,5>` to 640 channels, `<16,10>` to 1280: ragged last blocks (rows % 4, rows % 16),
    the `vi < nvec` tail (C = 8, 320, 648, 960, 1344), the full width of each (2048, 640, 1280)."""
    x, ga, be = _ln_inputs(rows, C)
    eps = 1e-5 if (rows + C) % 2 else 1e-6
    _ln_check(ops, f"<{inst[0]},{inst[1]}> rows={rows} C={C} eps={eps}", x, ga, be, eps, inst)


@pytest.mark.parametrize("inst,rows,C", [((64, 4), 33, 320), ((16, 5), 8200, 320), ((16, 10), 8197, 960)])
def test_layernorm_rows_are_independent_and_runs_repeat(ops, inst, rows, C):
    x, ga, be = _ln_inputs(rows, C, 3)
    perm = torch.randperm(rows, generator=_gen(rows, C, 4))
    y, ran = ops.layer_norm(x.cuda(), ga.cuda(), be.cuda(), 1e-5, return_path=True)
    yp, ranp = ops.layer_norm(x[perm].contiguous().cuda(), ga.cuda(), be.cuda(), 1e-5, return_path=True)
    assert ran == inst and ranp == inst
    assert torch.equal(yp.cpu(), y.cpu()[perm])                                       # a row's result does not depend on its place or its neighbours
    assert torch.equal(ops.layer_norm(x.cuda(), ga.cuda(), be.cuda(), 1e-5), y)       # run to run


@pytest.mark.parametrize("rows,C", [(4, 12), (4, 2056), (0, 64), (4, 4)])
def test_layernorm_refuses(ops, err_type, rows, C):
    with pytest.raises(err_type):
        ops.layer_norm(torch.zeros(rows, C).cuda(), torch.ones(C).cuda(), torch.zeros(C).cuda())


# ------------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ------------------------------------------------------------------------------------------------------------------------------
def _gn_inputs(B, C0, C1, shape, groups, *seed, ratio=None):
    """-> x0, x1 (or None), gamma, beta: every (image, group) with its own scale 2^-2 .. 2^2 and its own mean (|mean| <= sigma, or ratio x sigma
    with alternating sign)"""
    g = _gen(B, C0, C1, groups, *shape, *seed)
    C = C0 + C1
    z = torch.randn(B, C, *shape, generator=g)
    sig = 2.0 ** torch.randint(-2, 3, (B, groups), generator=g).float()
    if ratio is None:
        mu = (torch.randn(B, groups, generator=g) * 0.5).clamp(-1, 1)
    else:
        mu = float(ratio) * (1 - 2 * ((torch.arange(groups)[None, :] + torch.arange(B)[:, None]) % 2)).float()
    ex = (slice(None), slice(None)) + (None,) * len(shape)
    x = bfr((z + mu.repeat_interleave(C // groups, 1)[ex]) * sig.repeat_interleave(C // groups, 1)[ex])
    ga, be = _affine(C, g)
    return x[:, :C0].contiguous(), (x[:, C0:].contiguous() if C1 else None), ga, be


def _tables(x0, x1, bm0, bm1):
    return partials(nhwc(x0), bm0).cuda(), (partials(nhwc(x1), bm1).cuda() if x1 is not None else None)


def _gn_run(ops, x0, x1, groups, ga, be, eps, silu, part=None, bm=None, part1=None, bm1=None):
    y, path = ops.group_norm(x0.cuda(), groups, ga.cuda(), be.cuda(), eps, silu, x1=None if x1 is None else x1.cuda(),
                             part=part, bm=bm, part1=part1, bm1=bm1, return_path=True)
    return y.cpu(), path


def _gn_ref(x0, x1, groups, ga, be, eps, silu):
    return (gn_slabs(groupnorm_fp64(x0, x1, groups, ga, be, eps, silu), groups), gn_slabs(groupnorm_model(x0, x1, groups, ga, be, eps, silu), groups))


def _two_kernel_rounds(B, C, HW):
    """pixel rounds per block of the two-kernel path (norm.hip gn_geom): the summation order of its statistics depends on nothing else"""
    pr = 512 // (C // 8)
    target = -(-HW * B // 256)
    return min(max(-(-target // pr), 1), 16)


GN_TWO = [  # C0, C1, map, groups, B, silu, eps
    (8, 0, (8, 8), 1, 3, True, 1e-5), (8, 0, (8, 8), 8, 1, False, 1e-6),               # one vector per pixel, 512 pixel rows per block
    (320, 0, (64, 64), 32, 3, True, 1e-5),                                             # four loads in flight + a ragged last chunk
    (640, 320, (32, 32), 32, 3, True, 1e-5),                                           # 30 .. 120 vectors: 480 active threads, ragged chunk
    (1280, 1280, (8, 8), 64, 3, True, 1e-6),                                           # one pixel per block, cpg = 40
    (1280, 640, (16, 16), 32, 1, True, 1e-5),                                          # cpg = 60
    (320, 320, (24, 24), 64, 3, False, 1e-5),                                          # cpg = 10: vectors straddle groups
    (320, 320, (24, 24), 1, 1, True, 1e-6),
    (192, 64, (16, 24), 32, 1, True, 1e-5), (192, 64, (16, 24), 1, 3, False, 1e-6),    # the non-square map
    (4096, 0, (4, 4), 64, 1, True, 1e-5), (4096, 0, (4, 4), 1, 3, False, 1e-5),        # the widest: 512 vectors
]


@pytest.mark.parametrize("C0,C1,shape,groups,B,silu,eps", GN_TWO)
def test_groupnorm_two_kernel(ops, C0, C1, shape, groups, B, silu, eps):
    x0, x1, ga, be = _gn_inputs(B, C0, C1, shape, groups)
    got, path = _gn_run(ops, x0, x1, groups, ga, be, eps, silu)
    assert path == TWO
    want, model = _gn_ref(x0, x1, groups, ga, be, eps, silu)
    _judge("gn_two_kernel", f"{C0}+{C1} {shape} G={groups} B={B} silu={silu} eps={eps}", gn_slabs(got, groups), want, model)
    assert torch.equal(_gn_run(ops, x0, x1, groups, ga, be, eps, silu)[0], got)        # run to run


@pytest.mark.parametrize("C0,C1,shape,groups", [(8, 0, (8, 8), 1), (192, 64, (16, 24), 32), (1280, 1280, (8, 8), 64), (640, 320, (32, 32), 32)])
def test_groupnorm_images_are_independent(ops, C0, C1, shape, groups):
    """A batch of 3 against three batches of 1: bit for bit where both run the same pixel rounds per block (the statistics are then the same
    sums in the same order); otherwise each within the bound."""
    x0, x1, ga, be = _gn_inputs(3, C0, C1, shape, groups, 5)
    got, _ = _gn_run(ops, x0, x1, groups, ga, be, 1e-5, True)
    HW = shape[0] * shape[1]
    same = _two_kernel_rounds(3, C0 + C1, HW) == _two_kernel_rounds(1, C0 + C1, HW)
    assert same == (C0 != 640)                                                         # three cases of the one kind, one of the other
    for i in range(3):
        xi0, xi1 = x0[i:i + 1].contiguous(), (None if x1 is None else x1[i:i + 1].contiguous())
        one, path = _gn_run(ops, xi0, xi1, groups, ga, be, 1e-5, True)
        assert path == TWO
        if same:
            assert torch.equal(one, got[i:i + 1]), i
        else:
            want, model = _gn_ref(xi0, xi1, groups, ga, be, 1e-5, True)
            _judge("gn_two_kernel", f"image {i} of {C0}+{C1} {shape}", gn_slabs(one, groups), want, model)


GN_PART = [  # C0, C1, map, bm0, bm1, groups, B, silu, eps
    (640, 320, (32, 32), 128, 64, 32, 2, True, 1e-5),              # cpg = 30, 30 vectors per slice: 510 active threads; nt0 != nt1
    (1280, 640, (16, 16), 64, 128, 32, 1, True, 1e-5),             # cpg = 60
    (1280, 1280, (8, 8), 64, 64, 32, 3, True, 1e-6),               # cpg = 80, one tile per image
    (320, 320, (24, 24), 64, 64, 32, 1, False, 1e-5),              # cpg = 20, 25 pixel rows per block against 576 pixels: clamped loads
    (640, 320, (16, 16), 256, 64, 32, 3, True, 1e-6),              # one tile against four
    (64, 0, (16, 16), 256, 0, 32, 2, True, 1e-5),                  # cpg = 2
    (64, 0, (16, 16), 128, 0, 8, 1, False, 1e-6),                  # two groups per slice
    (960, 0, (32, 32), 128, 0, 32, 1, True, 1e-5),                 # 30 vectors per slice on one source
    (320, 0, (64, 64), 64, 0, 32, 2, True, 1e-5),                  # 640 partial sums per group: two rounds of the batched loads
]


@pytest.mark.parametrize("C0,C1,shape,bm0,bm1,groups,B,silu,eps", GN_PART)
def test_groupnorm_partial_sum_kernel(ops, C0, C1, shape, bm0, bm1, groups, B, silu, eps):
    x0, x1, ga, be = _gn_inputs(B, C0, C1, shape, groups, 1)
    p0, p1 = _tables(x0, x1, bm0, bm1)
    got, path = _gn_run(ops, x0, x1, groups, ga, be, eps, silu, p0, bm0, p1, bm1)
    assert path == PART
    want, model = _gn_ref(x0, x1, groups, ga, be, eps, silu)
    name = f"{C0}+{C1} {shape} bm={bm0}/{bm1} G={groups} B={B} silu={silu} eps={eps}"
    _judge("gn_partial", name, gn_slabs(got, groups), want, model)
    sep, path = _gn_run(ops, x0, x1, groups, ga, be, eps, silu)
    assert path == TWO
    _judge("gn_two_kernel", name, gn_slabs(sep, groups), want, model)
    d = (got - sep).abs()
    assert float(d.max()) <= float(want.abs().max()) * BF16_ULP                        # at most a bf16 ulp of the largest value
    assert float((d > 0).float().mean()) < 0.02                                        # ... and only on isolated elements
    assert torch.equal(_gn_run(ops, x0, x1, groups, ga, be, eps, silu, p0, bm0, p1, bm1)[0], got)


@pytest.mark.parametrize("why,C0,C1,shape,bm0,bm1,groups", [
    ("C % 32", 40, 0, (8, 16), 64, 0, 4),
    ("HW % bm", 64, 0, (8, 24), 128, 0, 32),
    ("cpg * tiles >= 65536", 512, 0, (64, 64), 8, 0, 4),
    ("no part1", 64, 64, (8, 16), 64, None, 32),
])
def test_groupnorm_partial_sum_fallbacks(ops, why, C0, C1, shape, bm0, bm1, groups):
    """tables that the one-kernel form cannot use: the two-kernel path runs, and is right"""
    x0, x1, ga, be = _gn_inputs(2, C0, C1, shape, groups, 2)
    p0 = partials(nhwc(x0), bm0).cuda()
    p1 = partials(nhwc(x1), bm1).cuda() if bm1 else None
    got, path = _gn_run(ops, x0, x1, groups, ga, be, 1e-5, True, p0, bm0, p1, bm1)
    assert path == TWO, why
    want, model = _gn_ref(x0, x1, groups, ga, be, 1e-5, True)
    _judge("gn_fallback", why, gn_slabs(got, groups), want, model)


@pytest.mark.parametrize("form", ["two_kernel", "partial"])
@pytest.mark.parametrize("value", [0.0, 2.0, 1.5])
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_constant_groups(ops, form, value, silu):
    """Zero variance: group 3 of image 0 and all of image 1 hold one bf16 value, image 2 is ordinary.  The output there is
    bf16(silu?(beta)) as the model gives it: exactly for 0 and for 2 (a power of two: mean * scale is exact, so fused or not the shift is
    rounded once); with SiLU except where the kernel's approximate exponential rounds the other way; 1.5 within the bound."""
    C0, C1, shape, groups, eps = 64, 64, (16, 16), 32, 1e-5
    x0, x1, ga, be = _gn_inputs(3, C0, C1, shape, groups, 6)
    x0[0, 12:16] = value
    x0[1], x1[1] = value, value
    p0, p1 = _tables(x0, x1, 128, 64) if form == "partial" else (None, None)
    got, path = _gn_run(ops, x0, x1, groups, ga, be, eps, silu, p0, 128, p1, 64)
    assert path == (PART if form == "partial" else TWO)
    want, model = _gn_ref(x0, x1, groups, ga, be, eps, silu)
    g = gn_slabs(got, groups)
    _judge(f"gn_{form}", f"constant {value} silu={silu}", g, want, model)
    const = torch.zeros(3, groups, dtype=torch.bool)
    const[0, 3], const[1] = True, True
    b32 = be.float()[None, :, None].expand(3, C0 + C1, shape[0] * shape[1])
    expect = gn_slabs((b32 / (1 + torch.exp(-b32)) if silu else b32).to(torch.bfloat16).double(), groups)
    ulp = expect[const].abs() * 2.0 ** -7
    # the model itself: beta, to a bf16 ulp and the fp32 rounding of the shift (2^-24 |mean rstd gamma| < 2^-24 * 2 * 317 * 2 < 2^-13)
    assert bool(((model[const] - expect[const]).abs() <= ulp + 2.0 ** -13).all())
    if value != 1.5:
        d = (g[const] - model[const]).abs()
        if silu:
            assert bool((d <= ulp).all()) and float((d > 0).float().mean()) < 0.02
        else:
            assert torch.equal(g[const], model[const])


# ------------------------------------------------------------------------------------------------------------------------------
# the fold
# ------------------------------------------------------------------------------------------------------------------------------
def _fold_inputs(C, N, HW, bm, B, *seed, ratio=None):
    x, _, ga, be = _gn_inputs(B, C, 0, (HW,), 32, N, bm, *seed, ratio=ratio)
    g = _gen(C, N, HW, bm, B, 11, *seed)
    w = bfr(torch.randn(N, C, generator=g) / C ** 0.5)
    bias = torch.randn(N, generator=g) * 0.1
    return x, ga, be, w, bias


def _fold_projection(ops, name, out, x, ga, be, eps, w, bias, m, ratio_only=False):
    want = fold_slabs(fold_fp64(x, 32, ga, be, eps, w, bias))
    return want, _judge("gn_fold", name, fold_slabs(out["y"]), want, fold_slabs(m["y"]), ratio_only)


FOLD = [(320, 320, 128, 64, 2), (320, 960, 1024, 128, 1), (640, 640, 256, 128, 3), (64, 32, 128, 128, 1), (1024, 64, 128, 64, 1),
        (64, 40, 128, 64, 2),                  # N is no multiple of 16: a ragged last row block of the fold and a ragged GEMM tile
        (320, 80, 4096, 64, 1)]                # 640 partial sums per group: two rounds of the fold kernel's batched loads


@pytest.mark.parametrize("C,N,HW,bm,B", FOLD)
def test_gn_fold(ops, C, N, HW, bm, B):
    """Wb: equal to the model wherever the rounding is decided by the declared arithmetic -- an element whose fp32 product lies within
    WB_SCALE_SLACK (relative) of a bf16 rounding boundary may take either neighbour, and that share, derived on the CPU, stays below 1e-3.
    rowadd against fp64 relative to sum |terms|.  The fragment order (frag_ni = C / 64, where N allows it) bit-equal to the library's
    re-layout of the row-major matrices.  The projection per (image, 16-column block) against fp64 GroupNorm -> linear, and against the
    unfolded chain of ops within the two forms' model errors."""
    eps = 1e-6 if C != 640 else 1e-5
    x, ga, be, w, bias = _fold_inputs(C, N, HW, bm, B)
    bias = None if N == 32 else bias
    ni = C // 64 if N % (16 * (C // 64)) == 0 else 0
    assert (ni > 0) == ((C, N) not in ((1024, 64), (64, 40)))
    cu = lambda t: None if t is None else t.cuda()      # noqa: E731
    out = {k: v.cpu() for k, v in ops.gn_fold(partials(nhwc(x), bm).cuda(), bm, 32, cu(ga), cu(be), cu(w), cu(bias), eps, x=cu(x), frag_ni=ni).items()}
    m = fold_model(x, 32, ga, be, eps, w, bias)
    name = f"C={C} N={N} HW={HW} bm={bm} B={B}"
    wb = out["wb"].double()
    undecided = m["wb_lo"] != m["wb_hi"]
    share = float(undecided.float().mean())
    off = wb != m["wb"]
    report(f"norm_ops[gn_fold {name}]", wb_undecided_share=share, wb_off_model_share=float(off.float().mean()))
    assert share < 1e-3, share
    assert not bool((off & ~undecided).any())
    assert bool(((wb == m["wb_lo"]) | (wb == m["wb_hi"]))[undecided].all())
    e_row = float(((out["rowadd"].double() - m["rowadd"]).abs() / m["rowadd_scale"]).max())
    print(f"gn_fold[{name}]: rowadd {e_row:.3e} of sum |terms| (bound {ROWADD_TOL:.3e}); Wb undecided share {share:.2e}, off the model {float(off.float().mean()):.2e}")
    report(f"norm_ops[gn_fold {name}]", rowadd_rel_e9=e_row * 1e9)
    assert e_row <= ROWADD_TOL, e_row
    if ni:
        assert torch.equal(out["wb_frag"], out["wb_frag_ref"])
        assert torch.equal(out["wb_frag"].sort(-1).values, out["wb"].reshape(B, -1).sort(-1).values)        # (a re-ordering of the same values)
    want, _ = _fold_projection(ops, name, out, x, ga, be, eps, w, bias, m)
    yn = ops.group_norm(cu(x), 32, cu(ga), cu(be), eps, False)
    chain = fold_slabs(ops.linear(yn.transpose(1, 2).contiguous(), cu(w), cu(bias)).cpu())
    cm = bfr(groupnorm_model(x, None, 32, ga, be, eps, False).float()).double().transpose(1, 2) @ w.double().T
    cm = fold_slabs(cm if bias is None else cm + bias.double())
    e_fold, r_fold = model_bounds(fold_slabs(m["y"]), want)
    e_chain, r_chain = model_bounds(cm, want)
    mx, rms = slab_errors(fold_slabs(out["y"]) - chain + want, want)
    report(f"norm_ops[gn_fold {name}]", chain_max=float(mx.max()), chain_rms=float(rms.max()), chain_model_max=e_fold + e_chain)
    assert float(mx.max()) <= MODEL_FACTOR * (e_fold + e_chain) and float(rms.max()) <= MODEL_FACTOR * (r_fold + r_chain)


def test_gn_fold_refuses(ops, err_type):
    def run(C, N, HW, bm, ni=0, hw=None):
        z = lambda *s: torch.zeros(*s).cuda()      # noqa: E731
        return ops.gn_fold(z(1, HW // bm, C, 2), bm, 32, z(C), z(C), z(N, C), None, frag_ni=ni, hw=hw)
    with pytest.raises(err_type):
        run(1088, 64, 128, 64)                     # C > 1024
    with pytest.raises(err_type):
        run(320, 64, 96, 96, hw=128)               # HW % bm
    with pytest.raises(err_type):
        run(320, 64, 128, 64, ni=5)                # N % (16 frag_ni)
    run(320, 80, 128, 64, ni=5)                    # (the same call on a shape it takes)


# ------------------------------------------------------------------------------------------------------------------------------
# statistics with a large mean
# ------------------------------------------------------------------------------------------------------------------------------
# |mean| / sigma at which every form must hold the bound.  128 was first measured only: every form held it (see the docstring below), so it is
# asserted as well.  512 is measured and reported (bf16 inputs that far out take three or four distinct values per group: the ratio of the
# rounded inputs, which is what the kernels see, is reported with the figures)
ASSERTED_RATIOS = (0, 4, 32, 128)


@pytest.mark.parametrize("ratio", [0, 4, 32, 128, 512])
@pytest.mark.parametrize("form", ["two_kernel", "partial", "fold", "layernorm<64,4>", "layernorm<16,5>", "layernorm<16,10>"])
def test_statistics_with_a_large_mean(ops, form, ratio):
    """Every GroupNorm form takes the variance as E[x^2] - mean^2 from fp32 partial sums; LayerNorm takes two passes.  The inputs are
    bf16(sigma (z + ratio)) with the sign of the mean alternating between neighbouring groups / rows.

    Measured on an MI355X, kernel error / model error against the fp64 reference (max-measure, rms-measure), at |mean| / sigma = 0, 4, 32
    and 128 alike: two-kernel 1.0000 / 1.0000, partial-sum 1.0000 / 1.0000, fold 1.0005 / 1.0000, LayerNorm <64,4>, <16,5> and <16,10>
    1.0000 / 1.0000 -- the fp32 partial sums are short (at most 16 values per thread before the tree) and the finalize is fp64, so the
    cancellation in E[x^2] - mean^2 stays three orders of magnitude below the bf16 rounding of the output up to 128.  At 512 (the rounded
    inputs measure 516 .. 524): 1.0000 / 1.0000 for every form but the fold, 0.9966 / 1.0011 there -- no form has left the bound yet."""
    only = ratio not in ASSERTED_RATIOS
    if form.startswith("layernorm"):
        inst, rows, C = {"layernorm<64,4>": ((64, 4), 33, 320), "layernorm<16,5>": ((16, 5), 8200, 320), "layernorm<16,10>": ((16, 10), 8197, 960)}[form]
        x, ga, be = _ln_inputs(rows, C, 9, ratio=ratio)
        seen = x.double()
        _, r = _ln_check(ops, f"{form} mean/sigma={ratio}", x, ga, be, 1e-5, inst, only)
    elif form == "fold":
        C, N, HW, bm, B = 320, 320, 256, 64, 2
        x, ga, be, w, bias = _fold_inputs(C, N, HW, bm, B, 9, ratio=ratio)
        seen = x.double().reshape(B, 32, -1)
        out = {k: v.cpu() for k, v in ops.gn_fold(partials(nhwc(x), bm).cuda(), bm, 32, ga.cuda(), be.cuda(), w.cuda(), bias.cuda(), 1e-6, x=x.cuda()).items()}
        _, r = _fold_projection(ops, f"mean/sigma={ratio}", out, x, ga, be, 1e-6, w, bias, fold_model(x, 32, ga, be, 1e-6, w, bias), only)
    else:
        x0, x1, ga, be = _gn_inputs(2, 320, 320, (32, 32), 32, 9, ratio=ratio)
        seen = torch.cat([x0, x1], 1).double().reshape(2, 32, -1)
        p0, p1 = _tables(x0, x1, 128, 64) if form == "partial" else (None, None)
        got, path = _gn_run(ops, x0, x1, 32, ga, be, 1e-5, True, p0, 128, p1, 64)
        assert path == (PART if form == "partial" else TWO)
        want, model = _gn_ref(x0, x1, 32, ga, be, 1e-5, True)
        r = _judge(f"gn_{form}", f"mean/sigma={ratio}", gn_slabs(got, 32), want, model, only)
    eff = float((seen.mean(-1).abs() / seen.std(-1)).median())
    print(f"large mean[{form} {ratio}]: kernel / model max {r[0]:.4f} rms {r[1]:.4f}; |mean| / sigma of the rounded inputs {eff:.1f}")
    report(f"norm_ops[large mean {form} {ratio}]", ratio_max=r[0], ratio_rms=r[1], holds=float(max(r) <= MODEL_FACTOR), input_ratio=eff)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: before anything is computed from the arguments
# ------------------------------------------------------------------------------------------------------------------------------
BAD_GN = [("C < 8", 4, 0, 1), ("C % 8", 12, 0, 4), ("C0 % 8", 12, 20, 4), ("groups < 1", 64, 0, 0), ("groups > 64", 1024, 0, 128),
          ("C % groups", 64, 0, 24), ("C > 4096", 4104, 0, 8)]


@pytest.mark.parametrize("why,C0,C1,groups", BAD_GN)
def test_groupnorm_refuses(ops, err_type, why, C0, C1, groups):
    C = C0 + C1
    z = lambda *s: torch.zeros(*s).cuda()      # noqa: E731
    with pytest.raises(err_type):
        ops.group_norm(z(1, C0, 8, 8), groups, z(C), z(C), x1=z(1, C1, 8, 8) if C1 else None, return_path=True)
    if C1:
        return                                 # the other entries take one source
    with pytest.raises(err_type):
        ops.group_norm(z(1, C, 8, 8), groups, z(C), z(C))
    with pytest.raises(err_type):
        ops.conv_groupnorm(z(1, 64, 8, 8), z(C, 64, 3, 3), z(C), z(C), z(C), groups=groups, fused=False)
    with pytest.raises(err_type):
        ops.gn_fold(z(1, 1, C, 2), 64, groups, z(C), z(C), z(16, C))
