"""Every forward instantiation of csrc/attention.hip's `attn_kernel<D, KB, QB, RECORD, AMASK, EXTRA>` on its own, through the
context-free entry `agd_op_attention_ex` (`ops.attention` with keyword arguments): the plain kernel on two- and three-block key tiles,
causal order, the additive mask, the second K/V source, the two recording forms with and without a mask, the fused operand layouts of
the production callers, and the deferred rescale of the online softmax -- at all six head dims.

Reference: `_attn_model.attention_fp64`, fp64 on the bf16-rounded operands.  Measure: every (batch row, head) slab of the output on its
own, max |error| / max |slab| and RMS error / RMS slab; V of head h is multiplied by 4^-h (exact in bf16), so a leak from a neighbouring
head is a multiple of the slab's scale.  Bound, per case and from the reference alone: `_attn_model.attention_model` restates the
roundings the kernel declares (q folded with scale * log2 e and rounded to bf16 -- not in the recording kernels --, P rounded to bf16
before P V, the output rounded to bf16); its worst slab against fp64 is E_model (max) / E_rms; the kernel must stay within 2 x each,
and no case may have 2 x E_model above 2^-6.  Recorded probabilities: 2e-3 absolute, rows summing to 1 within 1e-3 (the project's bounds).
Where two launches must do the same arithmetic (layouts, a `-inf` mask against fewer keys, the second source against concatenated
keys, an all-zero mask, a second run) the outputs are compared bit for bit."""
import functools
import math

import pytest
import torch
from _attn_model import LOG2E, MODEL_FACTOR, attention_fp64, attention_model, bfr, heads_of, model_bounds, slab_errors
from _report import report

pytestmark = pytest.mark.gpu

DIMS = (32, 40, 64, 80, 128, 160)
INF = math.inf


@pytest.fixture(scope="module")
def ops():
    from agenda_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (CPU, deterministic per case)
# ------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _scale_v_by_head(v, H):
    """V of head h times 4^-h: exact in bf16"""
    B, N, C = v.shape
    return (v.view(B, N, H, C // H) * (4.0 ** -torch.arange(H, dtype=torch.float32))[None, None, :, None]).reshape(B, N, C)


def _qkv(B, H, D, Nq, Nk, *seed, q_gain=1.0):
    g = _gen(B, H, D, Nq, Nk, *seed)
    q = bfr(q_gain * torch.randn(B, Nq, H * D, generator=g))
    k = bfr(torch.randn(B, Nk, H * D, generator=g))
    v = _scale_v_by_head(bfr(torch.randn(B, Nk, H * D, generator=g)), H)
    return q, k, v


def _mask(kind, B, Nk, seed=0):
    """fp32 [B, Nk]; never a row with every key removed"""
    m = torch.zeros(B, Nk)
    if kind == "zero":
        return m
    if kind == "finite":                      # -10000 on a different key set per batch row (about 40 % of the keys, key b kept)
        g = _gen(B, Nk, seed, 17)
        m[torch.rand(B, Nk, generator=g) < 0.4] = -10000.0
        for b in range(B):
            m[b, b % Nk] = 0.0
        assert len({tuple(r.tolist()) for r in m}) == B or Nk == 1
        return m
    if kind == "tail":                        # -inf on keys >= j_b, a different j per batch row
        js = [max(1, Nk - 5), max(1, Nk // 2), min(3, Nk)]
        for b in range(B):
            m[b, js[b % 3]:] = -INF
        return m
    if kind == "tile0":                       # the whole first 64-key tile gone
        assert Nk > 64
        m[:, :64] = -INF
        return m
    if kind == "mixed":                       # the recording kernel: row 0 finite, row 1 a -inf tail, row 2 finite on another set
        m = _mask("finite", B, Nk, seed)
        if B > 1 and Nk > 1:
            m[1] = 0.0
            m[1, max(1, Nk // 2):] = -INF
        return m
    raise ValueError(kind)


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _run(ops, q, k, v, H, **kw):
    mask, k2, v2 = _cuda(kw.pop("mask", None), kw.pop("k2", None), kw.pop("v2", None))
    out = ops.attention(q.cuda(), k.cuda(), v.cuda(), H, mask=mask, k2=k2, v2=v2, **kw)
    return tuple(t.cpu() for t in out) if isinstance(out, tuple) else out.cpu()


# ------------------------------------------------------------------------------------------------------------------------------
# the check against the reference
# ------------------------------------------------------------------------------------------------------------------------------
def _bounds_of(q, k, v, H, fold=True, **kw):
    """(reference output, reference probabilities, E_model, E_rms) of a case; refuses a case whose model error is too large to judge by"""
    want, p = attention_fp64(q, k, v, H, **kw)
    e_model, e_rms = model_bounds(attention_model(q, k, v, H, fold=fold, **kw), want, H)
    return want, p, e_model, e_rms


def _judge(name, got, want, H, e_model, e_rms):
    mx, rms = slab_errors(got, want, H)
    k_max, k_rms = float(mx.max()), float(rms.max())
    print(f"attention[{name}]: worst slab max {k_max:.5f} (E_model {e_model:.5f}), rms {k_rms:.5f} (E_rms {e_rms:.5f})")
    report(f"attention_ops[{name}]", kernel_max=k_max, model_max=e_model, kernel_rms=k_rms, model_rms=e_rms)
    assert bool(torch.isfinite(got).all()), name
    assert k_max <= MODEL_FACTOR * e_model, (name, "max", k_max, e_model, mx.tolist())
    assert k_rms <= MODEL_FACTOR * e_rms, (name, "rms", k_rms, e_rms, rms.tolist())


def _check(ops, name, q, k, v, H, layout=0, **kw):
    want, _, e_model, e_rms = _bounds_of(q, k, v, H, **kw)
    got = _run(ops, q, k, v, H, layout=layout, **kw)
    _judge(name, got, want, H, e_model, e_rms)
    return got


B0, H0 = 2, 3


# ------------------------------------------------------------------------------------------------------------------------------
# the plain kernel: key edges, query edges, scale
# ------------------------------------------------------------------------------------------------------------------------------
KEY_EDGES = (1, 63, 64, 65, 96, 97, 128, 129, 257)      # 65 .. 96: three 32-key blocks in one tile; 97: two 64-key tiles; 257: a tile of ONE key
QUERY_EDGES = (1, 31, 32, 33, 127, 128, 129)


@pytest.mark.parametrize("Nk", KEY_EDGES)
@pytest.mark.parametrize("D", DIMS)
def test_key_edges(ops, D, Nk):
    """Nq = 130: one whole query tile, then a ragged one whose second, third and fourth wave hold no valid query."""
    q, k, v = _qkv(B0, H0, D, 130, Nk)
    got = _check(ops, f"keys D{D} Nk{Nk}", q, k, v, H0)
    if Nk == 1:                               # softmax over one key is 1: the output IS that key's V row
        assert torch.equal(got, v.expand(B0, 130, H0 * D))


@pytest.mark.parametrize("Nq", QUERY_EDGES)
@pytest.mark.parametrize("D", DIMS)
def test_query_edges(ops, D, Nq):
    q, k, v = _qkv(B0, H0, D, Nq, 97)
    _check(ops, f"queries D{D} Nq{Nq}", q, k, v, H0)


@pytest.mark.parametrize("scale", (0.3, 1.0, None))
@pytest.mark.parametrize("D", DIMS)
def test_scale_is_honoured(ops, D, scale):
    """q is sized so that the logits have a standard deviation of 1.5 at the scale under test: a kernel that ignored the argument and
    used D^-0.5 would be off by the ratio of the two."""
    s = D ** -0.5 if scale is None else scale
    q, k, v = _qkv(B0, H0, D, 130, 97, 5, q_gain=1.5 / (s * math.sqrt(D)))
    _check(ops, f"scale D{D} s{scale}", q, k, v, H0, scale=scale, layout=2)      # (layout = 2 takes the new entry at scale = None too)
    if scale is not None:                                                        # and the old entry
        want, _, e_model, e_rms = _bounds_of(q, k, v, H0, scale=scale)
        _judge(f"scale(op_attention) D{D} s{scale}", _run(ops, q, k, v, H0, scale=scale), want, H0, e_model, e_rms)


# ------------------------------------------------------------------------------------------------------------------------------
# causal order
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 64, 65, 77, 96, 97, 200))
@pytest.mark.parametrize("D", DIMS)
def test_causal(ops, D, N):
    q, k, v = _qkv(B0, H0, D, N, N, 1)
    got = _check(ops, f"causal D{D} N{N}", q, k, v, H0, causal=True)
    assert torch.equal(got[:, 0], v[:, 0])                       # query 0 sees key 0 alone


@pytest.mark.parametrize("N,j", [(77, 32), (200, 96), (200, 128), (200, 100), (77, 40)])
@pytest.mark.parametrize("D", DIMS)
def test_causal_ignores_future_keys(ops, D, N, j):
    """K and V rows >= j replaced by other (larger) finite values: output rows < j keep every bit -- a mask off by one key would move
    row j - 1.  Bit-identity holds for the rows of the WAVES below j: the deferred rescale is voted per wave of 32 queries
    (`__all(mx <= DEFER_THR)`), so a row >= j that meets a large new logit makes its whole wave rescale, and the rows < j that share
    the wave come out by another, equally valid, rounding path (measured on the first run of this test: j = 100 of N = 200 moved rows
    96 .. 99 at every head dim).  With j in mid-wave those rows are therefore held to the reference bound instead, the rows of the
    waves below still to every bit."""
    q, k, v = _qkv(B0, H0, D, N, N, 2)
    _, k_other, v_other = _qkv(B0, H0, D, N, N, 3)
    k2, v2 = k.clone(), v.clone()
    k2[:, j:], v2[:, j:] = 3.0 * k_other[:, j:], 5.0 * v_other[:, j:]
    a = _run(ops, q, k, v, H0, causal=True)
    b = _run(ops, q, k2, v2, H0, causal=True)
    whole = j if N <= 96 else j - j % 32          # one key tile: the only rescale is the first tile's, per lane -- no vote to share
    assert torch.equal(a[:, :whole], b[:, :whole])
    assert not torch.equal(a[:, j:], b[:, j:])
    if whole < j:                     # rows whole .. j - 1: the same exact values (no key >= j is theirs), judged against them
        want, _, e_model, e_rms = _bounds_of(q[:, :j], k[:, :j], v[:, :j], H0, causal=True)
        _judge(f"causal future D{D} N{N} j{j}", b[:, :j], want, H0, e_model, e_rms)


# ------------------------------------------------------------------------------------------------------------------------------
# additive mask
# ------------------------------------------------------------------------------------------------------------------------------
BM = 3       # three batch rows: three different masks


@pytest.mark.parametrize("kind", ("finite", "tail", "tile0"))
@pytest.mark.parametrize("Nk", (77, 128, 200))
@pytest.mark.parametrize("D", DIMS)
def test_additive_mask(ops, D, Nk, kind):
    """finite: -10000 on another key set in every batch row (the index is mask[b * Nk + key]); tail: -inf from another key on in every
    batch row; tile0: -inf on keys 0 .. 63, so the first tile leaves no reference maximum and the maximum jumps in the second."""
    q, k, v = _qkv(BM, H0, D, 70, Nk, 4)
    _check(ops, f"mask {kind} D{D} Nk{Nk}", q, k, v, H0, mask=_mask(kind, BM, Nk, D))


@pytest.mark.parametrize("D", DIMS)
def test_inf_mask_equals_fewer_keys(ops, D):
    """-inf on keys >= 100 of 128 against the plain kernel on the first 100 keys: both run two 64-key tiles, the same bits."""
    q, k, v = _qkv(BM, H0, D, 70, 128, 6)
    m = torch.zeros(BM, 128)
    m[:, 100:] = -INF
    assert torch.equal(_run(ops, q, k, v, H0, mask=m), _run(ops, q, k[:, :100], v[:, :100], H0))


@pytest.mark.parametrize("Nk", (77, 200))
@pytest.mark.parametrize("D", DIMS)
def test_zero_mask_equals_no_mask(ops, D, Nk):
    """The masked path adds 0 to every logit: the same bits as the plain kernel."""
    q, k, v = _qkv(BM, H0, D, 70, Nk, 7)
    assert torch.equal(_run(ops, q, k, v, H0, mask=_mask("zero", BM, Nk)), _run(ops, q, k, v, H0))


# ------------------------------------------------------------------------------------------------------------------------------
# second K/V source
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nk2", (1, 30, 64))
@pytest.mark.parametrize("Nk", (128, 144, 256))
@pytest.mark.parametrize("D", DIMS)
def test_second_source(ops, D, Nk, Nk2):
    q, k, v = _qkv(B0, H0, D, 70, Nk, 8)
    _, k2, v2 = _qkv(B0, H0, D, 70, Nk2, 9)
    got = _check(ops, f"second D{D} Nk{Nk}+{Nk2}", q, k, v, H0, k2=k2, v2=v2)
    if Nk % 64 == 0:             # the second source starts a tile of its own either way: the plain kernel on [k; k2] does the same arithmetic
        assert torch.equal(got, _run(ops, q, torch.cat([k, k2], 1), torch.cat([v, v2], 1), H0))


# ------------------------------------------------------------------------------------------------------------------------------
# recording
# ------------------------------------------------------------------------------------------------------------------------------
REC_T = (1, 33, 64, 65, 77, 96)


def _check_probs(name, probs, want_p, B, rec_b0, rec_T, head_sum, H):
    """probs [B, H, T, Nq] (or [B, T, Nq] head-summed) against the reference probabilities [B, H, Nq, T]; untouched rows exactly zero"""
    want = want_p.permute(0, 1, 3, 2)                       # token-major
    tol, one = 2e-3, 1.0
    if head_sum:
        want, tol, one = want.sum(1), 2e-3 * H, float(H)
    T = want.shape[-2]
    assert probs.shape == want.shape
    assert bool((probs[:rec_b0] == 0).all()), (name, "batch rows below rec_b0 were written")
    assert bool((probs[rec_b0:, ..., rec_T:, :] == 0).all()), (name, "token rows from rec_T on were written")
    if rec_b0 < B:
        got = probs[rec_b0:, ..., :rec_T, :].double()
        err = float((got - want[rec_b0:, ..., :rec_T, :]).abs().max())
        assert err < tol, (name, err)
        if rec_T == T:
            assert float((got.sum(-2) - one).abs().max()) < 1e-3 * one, name
        if T == 1:
            assert bool((got == one).all()), (name, "one key: every probability is exactly 1")
        return err
    return 0.0


@pytest.mark.parametrize("T", REC_T)
@pytest.mark.parametrize("D", DIMS)
def test_per_head_probabilities_with_mask(ops, D, T):
    """The RECORD + AMASK instantiation (the hook seam with an attention_mask): rec_b0 = 0, 1, B and rec_T = T, T - 5."""
    B = 3
    q, k, v = _qkv(B, H0, D, 70, T, 10)
    m = _mask("mixed", B, T, D)
    want, want_p, e_model, e_rms = _bounds_of(q, k, v, H0, fold=False, mask=m)
    first = None
    for rec_b0 in (0, 1, B):
        for rec_T in sorted({T, max(1, T - 5)}):
            name = f"record+mask D{D} T{T} b0={rec_b0} recT={rec_T}"
            got, probs = _run(ops, q, k, v, H0, mask=m, return_probs=True, rec_b0=rec_b0, rec_T=rec_T)
            err = _check_probs(name, probs, want_p, B, rec_b0, rec_T, False, H0)
            if first is None:
                first = got
                _judge(f"record+mask D{D} T{T}", got, want, H0, e_model, e_rms)
                report(f"attention_ops[record+mask D{D} T{T}]", probs_abs=err)
            assert torch.equal(got, first), name                 # what is recorded does not touch the output
    if T == 1:
        assert torch.equal(first, v.expand(B, 70, H0 * D))


@pytest.mark.parametrize("T", REC_T)
@pytest.mark.parametrize("D", DIMS)
def test_recorded_probabilities_without_mask(ops, D, T):
    """RECORD 1 (per head) and RECORD 2 (one workgroup walks the heads and adds their sum once), with partial recording."""
    B = 3
    q, k, v = _qkv(B, H0, D, 70, T, 11)
    want, want_p, e_model, e_rms = _bounds_of(q, k, v, H0, fold=False)
    outs = []
    for head_sum in (False, True):
        for rec_b0, rec_T in ((0, T), (1, max(1, T - 5)), (B, T)):
            name = f"record{'-sum' if head_sum else ''} D{D} T{T} b0={rec_b0} recT={rec_T}"
            got, probs = _run(ops, q, k, v, H0, return_probs=True, head_sum=head_sum, rec_b0=rec_b0, rec_T=rec_T)
            err = _check_probs(name, probs, want_p, B, rec_b0, rec_T, head_sum, H0)
            if rec_b0 == 0:
                _judge(f"record{'-sum' if head_sum else ''} D{D} T{T}", got, want, H0, e_model, e_rms)
                report(f"attention_ops[record{'-sum' if head_sum else ''} D{D} T{T}]", probs_abs=err)
            outs.append(got)
    assert all(torch.equal(o, outs[0]) for o in outs)            # both forms do the same arithmetic per head


# ------------------------------------------------------------------------------------------------------------------------------
# the fused operand layouts of the production callers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_layouts_keep_every_bit(ops, D):
    """q|k|v rows of pitch 3C (UNet / CLIP self-attention, GLIGEN's fuser) and k|v rows of pitch 2C (cross-attention): other pitches,
    batch strides and buffer-descriptor bounds, the same values -- the same bits, on every variant those callers run."""
    _, k2, v2 = _qkv(B0, H0, D, 8, 30, 13)
    for N in (77, 200, 257):                 # self-attention shapes: three-block tile, mid-tile end, a last tile of one key
        q, k, v = _qkv(B0, H0, D, N, N, 12)
        for kw in ({}, {"causal": True}, {"k2": k2, "v2": v2}):
            base = _run(ops, q, k, v, H0, **kw)
            for layout in (1, 2):
                assert torch.equal(_run(ops, q, k, v, H0, layout=layout, **kw), base), (N, sorted(kw), layout)
    for Nq, Nk in ((130, 77), (70, 257), (33, 1)):      # cross-attention shapes
        q, k, v = _qkv(B0, H0, D, Nq, Nk, 14)
        m = _mask("finite", B0, Nk, D)
        variants = [{}, {"mask": m}]
        if Nk <= 96:
            variants += [{"return_probs": True}, {"return_probs": True, "mask": m}, {"return_probs": True, "head_sum": True}]
        for kw in variants:
            base, packed = _run(ops, q, k, v, H0, **kw), _run(ops, q, k, v, H0, layout=2, **kw)
            if isinstance(base, tuple):
                assert torch.equal(base[0], packed[0]) and torch.equal(base[1], packed[1]), (Nq, Nk, sorted(kw))
            else:
                assert torch.equal(base, packed), (Nq, Nk, sorted(kw))


@pytest.mark.parametrize("D", DIMS)
def test_every_variant_is_reproducible(ops, D):
    q, k, v = _qkv(B0, H0, D, 130, 200, 15)
    _, k2, v2 = _qkv(B0, H0, D, 8, 30, 16)
    m = _mask("finite", B0, 200, D)
    for kw in ({}, {"layout": 1, "causal": True}, {"causal": True}, {"mask": m}, {"k2": k2, "v2": v2}):
        qq = q if "layout" not in kw else bfr(torch.randn(B0, 200, H0 * D, generator=_gen(D, 99)))
        assert torch.equal(_run(ops, qq, k, v, H0, **kw), _run(ops, qq, k, v, H0, **kw)), sorted(kw)
    ks, vs, ms = k[:, :77], v[:, :77], m[:, :77].contiguous()
    for kw in ({}, {"return_probs": True}, {"return_probs": True, "mask": ms}, {"return_probs": True, "head_sum": True}, {"mask": ms}):
        a, b = _run(ops, q, ks, vs, H0, **kw), _run(ops, q, ks, vs, H0, **kw)
        if isinstance(a, tuple):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), sorted(kw)
        else:
            assert torch.equal(a, b), sorted(kw)


# ------------------------------------------------------------------------------------------------------------------------------
# the deferred rescale (DEFER_THR = 8 log2 units): D = 40 (Q pad column + ones column), 64 (C operand), 80 (C operand + ones column)
# ------------------------------------------------------------------------------------------------------------------------------
def _log2_logits(q, k, H):
    D = q.shape[-1] // H
    return (heads_of(q, H) @ heads_of(k, H).transpose(-1, -2)) * (D ** -0.5) * LOG2E          # [B, H, Nq, Nk]


# (batch row, query, spike key, growth of the row maximum over tile 0's, log2 units)
SPIKES = ((0, 5, 130, 7.5), (0, 40, 140, 9.5),      # batch row 0: wave 0 must NOT rescale, wave 1 must
          (1, 3, 130, 7.5), (1, 9, 140, 9.5))       # batch row 1: both in wave 0 -- the wave rescales, lanes without growth take delta = 0


@functools.lru_cache(maxsize=None)
def _spiked(D):
    """Nq = 64 (waves 0 and 1), Nk = 256; spike keys alpha q_r / (|q_r|^2 scale) in the third tile, alpha chosen per head from the
    realised maximum of tile 0.  Everything the construction promises is measured in fp64 on the rounded operands and asserted."""
    B, H, Nq, Nk = 2, 2, 64, 256
    q, k, v = _qkv(B, H, D, Nq, Nk, 20)
    scale = D ** -0.5
    m0 = _log2_logits(q, k, H)[..., :64].amax(-1)                       # [B, H, Nq]
    for b, r, key, grow in SPIKES:
        for h in range(H):
            qr = q[b, r, h * D:(h + 1) * D].double()
            alpha = (grow + float(m0[b, h, r])) / LOG2E
            k[b, key, h * D:(h + 1) * D] = bfr((alpha * qr / (qr.pow(2).sum() * scale)).float())
    L = _log2_logits(q, k, H)
    m0 = L[..., :64].amax(-1, keepdim=True)
    growth = torch.stack([L[..., 64 * t:64 * t + 64].amax(-1) for t in range(1, 4)], -1) - m0        # [B, H, Nq, tiles 1..3]
    for h in range(H):
        # batch row 0, wave 0 (queries 0 .. 31): no lane of the wave reaches the threshold at any tile, yet query 5 carries P near 2^7.5
        assert float(growth[0, h, :32].max()) <= 7.75 and float(growth[0, h, 5, 1]) >= 7.25, (D, h, growth[0, h, :32].max(), growth[0, h, 5])
        # batch row 0, wave 1: query 40 crosses it in the third tile
        assert float(growth[0, h, 40, 1]) >= 8.25, (D, h, growth[0, h, 40])
        # batch row 1, wave 0: query 9 crosses it, query 3 stays below, and some lanes have no growth at all (delta = 0)
        assert float(growth[1, h, 9, 1]) >= 8.25 and 7.25 <= float(growth[1, h, 3, 1]) <= 7.75, (D, h, growth[1, h, 3], growth[1, h, 9])
        assert int((growth[1, h, :32, 1] < -0.25).sum()) >= 1, (D, h)
    return q, k, v


@pytest.mark.parametrize("D", (40, 64, 80))
def test_deferred_rescale_on_both_sides_of_the_threshold(ops, D):
    q, k, v = _spiked(D)
    _check(ops, f"defer spikes D{D}", q, k, v, 2)


def _shifted(D, which):
    """Every query carries 4.0 in the first column of each head; the keys of one side carry -s there: their logits drop by 4 s scale."""
    B, H, Nq, Nk = 2, 2, 64, 256
    q, k, v = _qkv(B, H, D, Nq, Nk, 21)
    scale = D ** -0.5
    q[:, :, 0::D], k[:, :, 0::D] = 4.0, 0.0
    if which == "tile0_low":                  # tile 0 lies 60 below the later tiles: the first rescale multiplies by about 2^-86
        k[:, :64, 0::D] = bfr(torch.tensor(-60.0 / (4.0 * scale)))
    elif which == "tile0_very_low":           # ... 100 below, 2^144: past the fp32 exponent range -- a probability kept on tile 0's reference overflows
        k[:, :64, 0::D] = bfr(torch.tensor(-100.0 / (4.0 * scale)))
    else:                                     # the later tiles lie 100 below tile 0: their probabilities underflow to 0 in fp32
        k[:, 64:, 0::D] = bfr(torch.tensor(-110.0 / (4.0 * scale)))
    L = _log2_logits(q, k, H) / LOG2E         # natural units
    lo, hi = L[..., :64].amax(-1), L[..., 64:].amax(-1)
    if which == "tile0_low":
        assert float((hi - lo).min()) >= 50.0
    elif which == "tile0_very_low":
        assert float((hi - lo).min()) * LOG2E >= 130.0
    else:
        assert float((lo - L[..., 64:].amax(-1)).min()) >= 100.0 and float((lo - hi).min()) >= 100.0
    return q, k, v


@pytest.mark.parametrize("which", ("tile0_low", "tile0_very_low", "later_low"))
@pytest.mark.parametrize("D", (40, 64, 80))
def test_tiles_far_apart(ops, D, which):
    q, k, v = _shifted(D, which)
    _check(ops, f"defer {which} D{D}", q, k, v, 2)


@pytest.mark.parametrize("D", (40, 64, 80))
def test_masked_first_tile_then_low_logits(ops, D):
    """-inf on keys 0 .. 63 leaves the first tile without a reference maximum; every surviving logit lies near -100 (2^-144): a
    reference that stayed at its initial 0 would let all of them underflow and divide 0 by 0."""
    B, H, Nq, Nk = 2, 2, 64, 200
    q, k, v = _qkv(B, H, D, Nq, Nk, 22)
    q[:, :, 0::D], k[:, :, 0::D] = 4.0, bfr(torch.tensor(-100.0 / (4.0 * D ** -0.5)))
    assert float(_log2_logits(q, k, H).amax(-1).max()) <= -130.0
    _check(ops, f"mask tile0 low logits D{D}", q, k, v, H, mask=_mask("tile0", B, Nk))


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ops):
    """Every refusal is an error with a message naming what it refuses -- the entry's own before any allocation, the launcher's before
    its launch -- and the entry serves a good call afterwards."""
    from agenda_amd import _lib
    from agenda_amd._lib import AgendaHipError
    B, H, D = 2, 2, 64

    def t(*shape):
        return torch.zeros(*shape, device="cuda")

    def call(D=D, Nq=16, Nk=77, Nk2=None, B=B, **kw):
        C = H * D
        if kw.pop("with_mask", False):
            kw["mask"] = t(B, Nk)
        if Nk2 is not None:
            kw["k2"], kw["v2"] = t(B, Nk2, C), t(B, Nk2, C)
        return ops.attention(t(B, Nq, C), t(B, Nk, C), t(B, Nk, C), H, **kw)

    with pytest.raises(AgendaHipError, match=r"D=48\b"):
        call(D=48, causal=True)
    with pytest.raises(AgendaHipError, match=r"Nk=0\b"):
        call(Nk=0, causal=True)
    with pytest.raises(AgendaHipError, match=r"Nq=0\b"):
        call(Nq=0, layout=2)
    with pytest.raises(AgendaHipError, match=r"B=0\b"):
        call(B=0, layout=2)
    with pytest.raises(AgendaHipError, match=r"H=0\b"):      # (ops.attention divides by the head count: straight to the library)
        x = t(B, 16, 128)
        _lib.check(_lib.load().agd_op_attention_ex(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), B, 0, 64, 16, 16, 0.125, 1, None, None, None, 0, 0,
                                                   None, 0, 0, 16, _lib.current_stream_ptr()), None, "agd_op_attention_ex")
    with pytest.raises(AgendaHipError, match=r"Nk <= 96 \(got Nk=97\)"):
        call(Nk=97, return_probs=True, rec_b0=1)
    with pytest.raises(AgendaHipError, match=r"layout=1 .* Nq == Nk"):
        call(Nq=16, Nk=77, layout=1)
    with pytest.raises(AgendaHipError, match=r"layout=3\b"):
        call(layout=3)
    with pytest.raises(AgendaHipError, match=r"rec_b0=3\b"):
        call(return_probs=True, rec_b0=3)
    with pytest.raises(AgendaHipError, match=r"rec_T=78\b"):
        call(return_probs=True, rec_T=78)
    # the launcher's
    with pytest.raises(AgendaHipError, match="mask \\+ causal"):
        call(with_mask=True, causal=True)
    with pytest.raises(AgendaHipError, match="second K/V source takes no"):
        call(Nk2=8, with_mask=True)
    with pytest.raises(AgendaHipError, match="second K/V source takes no"):
        call(Nk2=8, causal=True)
    with pytest.raises(AgendaHipError, match="second K/V source takes no"):
        call(Nk2=8, return_probs=True)
    with pytest.raises(AgendaHipError, match="second K/V source of 0 keys"):
        call(Nk2=0)
    with pytest.raises(AgendaHipError, match="second K/V source of 65 keys"):
        call(Nk2=65)
    with pytest.raises(AgendaHipError, match="head-summed recording does not take"):
        call(with_mask=True, return_probs=True, head_sum=True)
    out, probs = call(with_mask=True, return_probs=True)
    assert float(out.abs().max()) == 0.0 and float((probs - 1.0 / 77).abs().max()) < 1e-6
