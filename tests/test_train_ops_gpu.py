"""The training-side kernels of csrc/train.hip one at a time, through their context-free entries (`ops.attention_backward`,
`ops.hook_headmean`): attn_bwd_kernel<D> + kv_grad_reduce_kernel against fp64 torch autograd at every instantiated head dim, at
ragged query tiles, short key counts and with either gradient absent; hook_headmean_kernel against the same ordered fp32 sum.

Metric of the attention backward: per (batch row, head) slab -- dq [N][D], dK [T][D], dV [T][D] separately --
max|got - want| / max|want|, so that no head hides behind another's scale.  Bound 2^-7: fp32 arithmetic on bf16 operands with
one bf16 rounding of the result; an fp32 torch restatement with that one rounding measures 0.0026-0.0037
(about 2^-8.1) against the same fp64 reference, so the bound leaves a factor of two."""
import functools

import pytest
import torch
from _report import report

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -7


def bfr(t):
    """round to bf16 and back: the values the kernels see"""
    return t.to(torch.bfloat16).float()


@pytest.fixture(scope="module")
def ops():
    from agenda_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def _inputs(B, H, D, N, T, b0, spike=False):
    """q [B,N,C], kv [B,T,2C], d_o [B,N,C] (all bf16-representable: what the kernel sees), d_map [B-b0,T,N] fp32."""
    g = torch.Generator().manual_seed(1000 * D + 10 * N + T + b0)
    C = H * D
    q = bfr(torch.randn(B, N, C, generator=g))
    kv = bfr(torch.randn(B, T, 2 * C, generator=g))
    d_o = bfr(0.01 * torch.randn(B, N, C, generator=g))
    d_map = torch.randn(B - b0, T, N, generator=g)
    if spike:                                   # key 5 dominates query 7 in every head: scores of 4 sqrt(D) |q|^2 / D ~ 4 sqrt(D)
        kv[:, 5, :C] = 4.0 * q[:, 7]
    return q, kv, d_o, d_map


def _reference(q, kv, H, d_o, d_map, b0, scale=None):
    """fp64 autograd of  sum(O . d_o) + sum(mean_heads(P)[b0:] . d_map)  w.r.t. q and kv."""
    B, N, C = q.shape
    T, D = kv.shape[1], C // H
    scale = D ** -0.5 if scale is None else scale
    q64, kv64 = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    Q = q64.view(B, N, H, D).permute(0, 2, 1, 3)                    # [B, H, N, D]
    K = kv64[..., :C].reshape(B, T, H, D).permute(0, 2, 1, 3)       # [B, H, T, D]
    V = kv64[..., C:].reshape(B, T, H, D).permute(0, 2, 1, 3)
    P = torch.softmax(scale * (Q @ K.transpose(-1, -2)), dim=-1)    # [B, H, N, T]
    O = (P @ V).permute(0, 2, 1, 3).reshape(B, N, C)
    m = P.mean(dim=1).permute(0, 2, 1)                              # [B, T, N]
    loss = q64.new_zeros(())
    if d_o is not None:
        loss = loss + (O * d_o.double()).sum()
    if d_map is not None:
        loss = loss + (m[b0:] * d_map.double()).sum()
    gq, gkv = torch.autograd.grad(loss, (q64, kv64))
    return gq, gkv


@functools.lru_cache(maxsize=None)
def _reference_of_case(B, H, D, N, T, b0, spike=False):
    q, kv, d_o, d_map = _inputs(B, H, D, N, T, b0, spike)
    return _reference(q, kv, H, d_o, d_map, b0)


def _slabs(dq, dkv, H):
    """dq [B,N,C], dkv [B,T,2C] -> {"dq": [B,H,N,D], "dk": [B,H,T,D], "dv": [B,H,T,D]} (fp64, cpu)"""
    dq, dkv = dq.detach().double().cpu(), dkv.detach().double().cpu()
    B, N, C = dq.shape
    T, D = dkv.shape[1], C // H
    return {"dq": dq.view(B, N, H, D).permute(0, 2, 1, 3),
            "dk": dkv[..., :C].reshape(B, T, H, D).permute(0, 2, 1, 3),
            "dv": dkv[..., C:].reshape(B, T, H, D).permute(0, 2, 1, 3)}


def _check(name, got, want, H, zero=lambda kind, b: False):
    """Every (batch row, head) slab of dq / dK / dV: below BOUND relative to the slab's own reference maximum, or -- where `zero(kind, b)`
    says the reference is identically zero -- exactly zero.  Which slabs are zero is asserted on the reference, so none is skipped."""
    g, w = _slabs(*got, H), _slabs(*want, H)
    worst = {}
    for kind in ("dq", "dk", "dv"):
        err = (g[kind] - w[kind]).abs().amax(dim=(2, 3))
        top = w[kind].abs().amax(dim=(2, 3))
        worst[kind] = 0.0
        for b in range(top.shape[0]):
            for h in range(top.shape[1]):
                if zero(kind, b):
                    assert float(top[b, h]) == 0.0, (name, kind, b, h, "the reference slab was expected to be identically zero")
                    assert bool((g[kind][b, h] == 0).all()), (name, kind, b, h, "must be exactly zero")
                else:
                    assert float(top[b, h]) > 0.0, (name, kind, b, h, "reference slab is zero: the metric is undefined")
                    worst[kind] = max(worst[kind], float(err[b, h] / top[b, h]))
    print(f"attention_backward {name}: worst slab dq {worst['dq']:.5f} dK {worst['dk']:.5f} dV {worst['dv']:.5f} (bound {BOUND:.5f})")
    report(f"attention_backward[{name}]", worst_dq=worst["dq"], worst_dk=worst["dk"], worst_dv=worst["dv"])
    assert max(worst.values()) < BOUND, (name, worst)


def _run(ops, q, kv, H, d_o, d_map, b0, scale=None):
    dq, dkv = ops.attention_backward(q.cuda(), kv.cuda(), H, d_o=None if d_o is None else d_o.cuda(),
                                     d_map=None if d_map is None else d_map.cuda(), b0=b0, scale=scale)
    return dq.cpu(), dkv.cpu()


# (B, H, D, N, T, b0): every instantiation of attn_bwd_kernel<D> with both gradients; ragged last tiles (200, 144, 100), T at the 96
# limit, four tiles through the ordered reduce (200)
EVERY_D = [(2, 2, 32, 64, 77, 0), (2, 8, 40, 200, 77, 1), (2, 2, 64, 144, 77, 0), (2, 8, 80, 100, 77, 1), (2, 2, 128, 64, 96, 1),
           (2, 2, 160, 100, 77, 1)]
# one partial tile; a second tile holding one row; exactly one tile
TILE_EDGES = [(2, 2, 40, 9, 77, 1), (2, 2, 40, 65, 77, 1), (2, 2, 40, 64, 77, 1)]
RAGGED = (2, 8, 40, 200, 77, 1)


@pytest.mark.parametrize("case", EVERY_D + TILE_EDGES + [(2, 2, 64, 100, 20, 1)], ids=lambda c: "x".join(map(str, c)))
def test_attention_backward_matches_fp64_autograd(ops, case):
    B, H, D, N, T, b0 = case
    q, kv, d_o, d_map = _inputs(*case)
    got = _run(ops, q, kv, H, d_o, d_map, b0)
    _check("x".join(map(str, case)), got, _reference_of_case(*case), H)


def test_attention_backward_single_key(ops):
    """T = 1: P is 1 everywhere, so the softmax passes no gradient back -- dq and dK are exactly zero (in the reference too); dV = sum_n dO."""
    case = (2, 2, 64, 100, 1, 1)
    q, kv, d_o, d_map = _inputs(*case)
    got = _run(ops, q, kv, 2, d_o, d_map, 1)
    _check("single_key", got, _reference_of_case(*case), 2, zero=lambda kind, b: kind != "dv")


def test_attention_backward_output_gradient_only(ops):
    """d_map = None (the dO-only path), and b0 = B with a map gradient given: no batch row takes it, the same bits."""
    B, H, D, N, T, b0 = case = (2, 2, 64, 144, 77, 0)
    q, kv, d_o, d_map = _inputs(*case)
    got = _run(ops, q, kv, H, d_o, None, 0)
    _check("d_o_only", got, _reference(q, kv, H, d_o, None, 0), H)
    same = _run(ops, q, kv, H, d_o, d_map[:0], B)
    assert torch.equal(same[0], got[0]) and torch.equal(same[1], got[1])


def test_attention_backward_map_gradient_only(ops):
    """d_o = None with b0 = 1: batch row 0 is outside the recorded map and receives exactly zero; dV is zero everywhere (V only reaches O)."""
    B, H, D, N, T, b0 = case = (2, 8, 40, 200, 77, 1)
    q, kv, d_o, d_map = _inputs(*case)
    got = _run(ops, q, kv, H, None, d_map, b0)
    _check("d_map_only", got, _reference(q, kv, H, None, d_map, b0), H, zero=lambda kind, b: kind == "dv" or b < b0)
    assert bool((got[0][0] == 0).all()) and bool((got[1][0] == 0).all())


def test_attention_backward_softmax_stability(ops):
    """A key that dominates one query (scores near 4 sqrt(D)): the row maximum has to be subtracted before the exponential."""
    case = (2, 2, 64, 144, 77, 0)
    q, kv, d_o, d_map = _inputs(*case, spike=True)
    C = q.shape[2]
    assert float((64 ** -0.5 * (q[:, 7].view(2, 2, 64) * kv[:, 5, :C].view(2, 2, 64)).sum(-1)).min()) > 10.0      # the spike is there
    got = _run(ops, q, kv, 2, d_o, d_map, 0)
    _check("spike", got, _reference_of_case(*case, spike=True), 2)


def test_attention_backward_padded_rows_do_not_leak_and_rows_are_independent(ops):
    """The first 64 queries of the ragged four-tile case against a run on those 64 queries alone: dq bit-identical (a query row's
    gradient depends on no other row, whichever tile holds it; the padding of the last tile reaches nothing)."""
    B, H, D, N, T, b0 = RAGGED
    q, kv, d_o, d_map = _inputs(*RAGGED)
    full, _ = _run(ops, q, kv, H, d_o, d_map, b0)
    part, _ = _run(ops, q[:, :64], kv, H, d_o[:, :64], d_map[..., :64], b0)
    assert part.shape == (B, 64, H * D) and torch.equal(full[:, :64], part)


def test_attention_backward_is_reproducible(ops):
    q, kv, d_o, d_map = _inputs(*RAGGED)
    a = _run(ops, q, kv, RAGGED[1], d_o, d_map, RAGGED[5])
    b = _run(ops, q, kv, RAGGED[1], d_o, d_map, RAGGED[5])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_attention_backward_refusals(ops):
    """Host-side checks of agd_op_attention_backward, each before any allocation or launch, each naming what it refuses."""
    from agenda_amd._lib import AgendaHipError
    B, H, D, N = 2, 2, 64, 16

    def call(D=D, T=77, d_o=True, d_map=True, b0=0):
        C = H * D
        q, kv = torch.zeros(B, N, C, device="cuda"), torch.zeros(B, T, 2 * C, device="cuda")
        return ops.attention_backward(q, kv, H, d_o=torch.zeros_like(q) if d_o else None,
                                      d_map=torch.zeros(max(B - b0, 1), T, N, device="cuda") if d_map else None, b0=b0)

    with pytest.raises(AgendaHipError, match=r"T=97\b"):
        call(T=97)
    with pytest.raises(AgendaHipError, match=r"T=0\b"):
        call(T=0)
    with pytest.raises(AgendaHipError, match=r"D=48\b"):
        call(D=48)
    with pytest.raises(AgendaHipError, match="d_o and d_map"):
        call(d_o=False, d_map=False)
    with pytest.raises(AgendaHipError, match=r"b0=3\b"):
        call(b0=B + 1)
    dq, dkv = call()                                # and the entry still serves a good call afterwards
    assert float(dq.abs().max()) == 0.0 and float(dkv.abs().max()) == 0.0


# (7, 2, 77, 4096): 2,207,744 outputs, just above the 8192 x 256 threads of the capped grid -- the grid-stride loop runs a second pass
@pytest.mark.parametrize("Bp,H,T,N", [(2, 2, 20, 9), (3, 5, 77, 144), (7, 2, 77, 4096)])
def test_hook_headmean_is_the_ordered_fp32_sum(ops, Bp, H, T, N):
    """hook_headmean_kernel: s = 0; s += heads[:, h] for h = 0, 1, ...; s * (1 / H) in fp32 -- the same arithmetic in torch, so the same bits."""
    g = torch.Generator().manual_seed(Bp * 100 + H)
    heads = torch.rand(Bp, H, T, N, generator=g)
    if N == 4096:
        assert 8192 * 256 < Bp * T * N < 2 * 8192 * 256          # the capped grid's second pass is a partial one
    s = torch.zeros(Bp, T, N, dtype=torch.float32)
    for h in range(H):
        s += heads[:, h]
    want = s * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32))
    got = ops.hook_headmean(heads.cuda()).cpu()
    assert got.shape == want.shape and torch.equal(got, want)
