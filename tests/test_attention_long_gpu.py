"""csrc/attention_long.hip on its own, through the context-free entry `agd_op_attention_long` (`ops.attention_long`): the recording
cross-attention kernel for 97 .. 320 keys, which walks 64-key tiles twice so that every recorded probability is divided by the row sum
over ALL keys.

Reference: `_attn_model.attention_fp64`, fp64 on the bf16-rounded operands.  Output measure and bound as in test_attention_ops_gpu.py:
every (batch row, head) slab on its own (V of head h times 4^-h, so a leak from the neighbouring head is a multiple of the slab's scale),
within 2 x the distance of `_attn_model.attention_model(fold=False)` -- the roundings the kernel's header declares: raw logits scaled in
fp32, unnormalised probabilities rounded to bf16 before P V, the output rounded to bf16 -- from fp64.  Recorded probabilities: 2e-3
absolute, columns summing to 1 within 1e-3 when every token row is recorded (the bounds of the existing recording tests).  Rows that
must not be written are exactly zero, and where two launches do the same arithmetic (layouts, what is recorded, a second run) the bits
are equal.

Key counts: 97 (one key in the second tile), 128 / 129 and 193 (a tile edge and one past it), 152 / 227 / 302 (the contexts of 2 / 3 / 4
prompt chunks), 320 (the largest; five full tiles).  Queries: 1, 70 (one ragged wave pair), 130 (two workgroups, the second with 2 rows)."""
import pytest
import torch
from _attn_model import MODEL_FACTOR, attention_fp64, attention_model, bfr, model_bounds, slab_errors
from _report import report

pytestmark = pytest.mark.gpu

DIMS = (32, 40, 64, 80, 128, 160)
KEYS = (97, 128, 129, 152, 193, 227, 302, 320)
QUERIES = (1, 70, 130)
B, H = 3, 2


@pytest.fixture(scope="module")
def ops():
    from agenda_amd import ops as o
    return o


def _qkv(D, Nq, Nk):
    g = torch.Generator().manual_seed(1000003 * D + 1009 * Nq + Nk)
    q = bfr(torch.randn(B, Nq, H * D, generator=g))
    k = bfr(torch.randn(B, Nk, H * D, generator=g))
    v = bfr(torch.randn(B, Nk, H * D, generator=g))
    v = (v.view(B, Nk, H, D) * (4.0 ** -torch.arange(H, dtype=torch.float32))[None, None, :, None]).reshape(B, Nk, H * D)   # exact in bf16
    return q, k, v


def _run(ops, q, k, v, **kw):
    o, p = ops.attention_long(q.cuda(), k.cuda(), v.cuda(), H, **kw)
    return o.cpu(), p.cpu()


def _check_probs(name, probs, want_p, rec_b0, rec_T):
    """probs [B, H, Nk, Nq] against the reference [B, H, Nq, Nk]; what must not be written is exactly zero"""
    want = want_p.permute(0, 1, 3, 2)
    Nk = want.shape[-2]
    assert probs.shape == want.shape, name
    assert bool((probs[:rec_b0] == 0).all()), (name, "batch rows below rec_b0 were written")
    assert bool((probs[rec_b0:, :, rec_T:, :] == 0).all()), (name, "token rows from rec_T on were written")
    if rec_b0 == B:
        return 0.0, 0.0
    got = probs[rec_b0:, :, :rec_T, :].double()
    err = float((got - want[rec_b0:, :, :rec_T, :]).abs().max())
    col = float((got.sum(-2) - 1.0).abs().max()) if rec_T == Nk else 0.0
    print(f"attention_long[{name}]: probabilities max abs error {err:.2e}, column sums off 1 by {col:.2e}")
    assert bool(torch.isfinite(got).all()), name
    assert err < 2e-3, (name, err)
    assert col < 1e-3, (name, col)
    return err, col


@pytest.mark.parametrize("Nk", KEYS)
@pytest.mark.parametrize("D", DIMS)
def test_output_and_probabilities(ops, D, Nk):
    """Every head dim x key count, at 1 / 70 / 130 queries, packed and k|v-fused operands, against fp64."""
    for Nq in QUERIES:
        q, k, v = _qkv(D, Nq, Nk)
        want, want_p = attention_fp64(q, k, v, H)
        e_model, e_rms = model_bounds(attention_model(q, k, v, H, fold=False), want, H)
        outs = []
        for layout in (0, 2):
            name = f"D{D} Nk{Nk} Nq{Nq} layout{layout}"
            got, probs = _run(ops, q, k, v, layout=layout)
            mx, rms = slab_errors(got, want, H)
            k_max, k_rms = float(mx.max()), float(rms.max())
            print(f"attention_long[{name}]: worst slab max {k_max:.5f} (E_model {e_model:.5f}), rms {k_rms:.5f} (E_rms {e_rms:.5f})")
            err, col = _check_probs(name, probs, want_p, 0, Nk)
            report(f"attention_long[{name}]", kernel_max=k_max, model_max=e_model, kernel_rms=k_rms, model_rms=e_rms, probs_abs=err, colsum=col)
            assert bool(torch.isfinite(got).all()), name
            assert k_max <= MODEL_FACTOR * e_model, (name, "max", k_max, e_model, mx.tolist())
            assert k_rms <= MODEL_FACTOR * e_rms, (name, "rms", k_rms, e_rms, rms.tolist())
            outs.append((got, probs))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (D, Nk, Nq, "the layout changed the arithmetic")


@pytest.mark.parametrize("Nk", KEYS)
@pytest.mark.parametrize("D", DIMS)
def test_partial_recording_determinism_accumulation(ops, D, Nk):
    """rec_b0 in (0, 1, B) x rec_T in (Nk, Nk - 5, 77, 100 -- inside the first tile, across a tile edge): untouched rows are exactly zero and
    the output's bits do not depend on what is recorded; a second run gives the same bits; a second launch into the same rows adds."""
    Nq = 70
    q, k, v = _qkv(D, Nq, Nk)
    _, want_p = attention_fp64(q, k, v, H)
    full_o, full_p = _run(ops, q, k, v, layout=2)
    for rec_b0 in (0, 1, B):
        for rec_T in sorted(t for t in {Nk, Nk - 5, 77, 100} if t <= Nk):       # (97 keys have no row 100: rec_T <= Nk)
            name = f"D{D} Nk{Nk} b0={rec_b0} recT={rec_T}"
            got, probs = _run(ops, q, k, v, layout=2, rec_b0=rec_b0, rec_T=rec_T)
            _check_probs(name, probs, want_p, rec_b0, rec_T)
            assert torch.equal(got, full_o), (name, "what is recorded changed the output")
            assert torch.equal(probs[rec_b0:, :, :rec_T], full_p[rec_b0:, :, :rec_T]), (name, "a recorded row depends on which rows are recorded")
    # two runs: equal bits (no float atomics; one lane owns each (image, head, token, pixel))
    again_o, again_p = _run(ops, q, k, v, layout=2)
    assert torch.equal(again_o, full_o) and torch.equal(again_p, full_p)
    # the kernel adds into the rows it is given: p + p = 2 p exactly
    acc = full_p.cuda().clone()
    o2, acc2 = ops.attention_long(q.cuda(), k.cuda(), v.cuda(), H, layout=2, probs=acc)
    assert acc2.data_ptr() == acc.data_ptr()
    assert torch.equal(acc.cpu(), 2 * full_p) and torch.equal(o2.cpu(), full_o)


def test_refusals(ops):
    """96 and 321 keys, and the other arguments the entry refuses, by name and before anything runs."""
    from agenda_amd._lib import AgendaHipError

    def call(Nk=152, D=64, Nq=16, **kw):
        return ops.attention_long(torch.zeros(B, Nq, H * D).cuda(), torch.zeros(B, Nk, H * D).cuda(), torch.zeros(B, Nk, H * D).cuda(), H, **kw)

    with pytest.raises(AgendaHipError, match=r"Nk=96 keys outside \[97, 320\]"):
        call(Nk=96)
    with pytest.raises(AgendaHipError, match=r"Nk=321 keys outside \[97, 320\]"):
        call(Nk=321)
    with pytest.raises(AgendaHipError, match=r"D=48\b"):
        call(D=48)
    with pytest.raises(AgendaHipError, match=r"layout=1\b"):
        call(layout=1)
    with pytest.raises(AgendaHipError, match=r"rec_b0=4\b"):
        call(rec_b0=4)
    with pytest.raises(AgendaHipError, match=r"rec_T=153\b"):
        call(rec_T=153)
    with pytest.raises(AgendaHipError, match=r"rec_T=0\b"):
        call(rec_T=0)
    out, probs = call()                                        # all-zero operands: a uniform softmax, and the engine still runs
    assert float(out.abs().max()) == 0.0 and float((probs - 1.0 / 152).abs().max()) < 1e-6
