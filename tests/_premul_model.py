"""What the pre-multiplied cross-attention tests compare csrc/xattn_pre.hip and csrc/ipadapter.hip with, on the CPU in fp64 (no test in here), and
the case lists that tests/test_premul_ops_gpu.py and tests/test_premul_model_cpu.py share.

Per stage two functions on the bf16-rounded inputs (`rounding=False` / `rounding=True` of one body, so that the model is the algebra by
construction and the CPU tests can show it):

`*_fp64`   the operation with nothing else rounded.  The attention: LayerNorm (two-pass statistics), to_q, the head split, softmax(scale q k^T),
           P v, to_out + bias + x.  The context products: the sums as the kernels' comments define them.
`*_model`  the same with the roundings the kernels' comments declare and nothing else (every GEMM stays exact):
  context   K'' = bf16(fp32(k Wq) scale gamma), one rounding of the fp32 product; cs = the row sums of that bf16 K''; bs = scale k . (Wq beta) with
            Wq beta in fp32; V'' = bf16(Wo v).  cs and bs are stored in fp32.
  scores    S = rstd (x . K'' - mu cs) + bs with mu = S_sum / C, var = Q_sum / C - mu^2 (one pass), rstd = rsqrt(var + eps) in fp32 from the fp32 sum
            of the statistics slots in slot order; P = p (1 / sum p) in fp32, rounded to bf16 once.  The recorder adds the fp32 P, not the bf16 one.
  output    y = bf16(P_bf16 V''^T + bo + x).
  IP-Adapter  the same chain with fp32 k_ip / v_ip, the statistics from the row itself (one slot), a softmax per head over n_tok columns, and
            h' = bf16(h + s P_bf16 V''^T).  ipa_linear: fp32 sums (judged by `fp32_sum_error`).  ipa_layernorm: two passes, every operation and both
            sums in fp32, in the order one wave takes them (`wave_sum32`): at |mean| / sigma = 512 a row's error IS the error of that sum.
Their distance from the fp64 functions is the error a correct kernel is entitled to; the tests bound the kernel by `MODEL_FACTOR` x that distance,
slab by slab (`slabs` / `slab_errors` of tests/_tblock_model.py: 16 rows x 80 columns -- for P exactly one wave's tile of one head).

The score scale.  A bf16 K'' costs every logit about 2^-9 / sqrt(3) of the root sum of squares of its C terms, about 0.0011 sigma_S, and a slab's
worst probability about four times that: with the keys of tests/_tblock_model.py (sigma_S = 1.5) the model alone sits at 0.007 of the ceiling's
half 0.0078 at C = 1280, T = 77.  The keys here have unit scale (`K_SCALE`), which keeps the reference inside the ceiling for every case."""
import math

import torch
import _tblock_model as TM
from _tblock_model import (MODEL_CEILING, MODEL_FACTOR, abs_bound, bfr, fp32_sum_error, kernel_errors, model_bounds, residual_condition,  # noqa: F401
                           slab_errors, slabs)

HEADS = 8
TP = 80                      # token rows per head of the pre-multiplied matrices
LN_EPS = 1e-5
K_SCALE = 1.0
_f32, _r, _b, _eps64 = TM._f32, TM._r, TM._b, TM._eps64


def scale32(D):
    return float(torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32))


def ipa_cols(heads, nt):
    return (heads * nt + 15) // 16 * 16


def slab_cols(N):
    """the slab width for an [M, N] operand: 80 where N is a multiple of it, else the whole row"""
    return 80 if N % 80 == 0 else N


def bounds(model_o, want_o, cols=80):
    """`model_bounds` for slabs of 16 x cols: (E_model, E_rms) of [M, N] operands, refusing a case whose 2 x E is above the ceiling.  A model that
    IS the reference, element for element (one token: P = 1), has no error to scale by: (0, 0), and the kernel must then equal it bit for bit."""
    m, w = slabs(model_o, 16, cols), slabs(want_o, 16, cols)
    mx, rms = slab_errors(m, w, m)
    e_model, e_rms = float(mx.max()), float(rms.max())
    if e_model == 0.0:
        assert torch.equal(model_o.double(), want_o.double())
        return 0.0, 0.0
    assert 0 < MODEL_FACTOR * e_model <= MODEL_CEILING and 0 < MODEL_FACTOR * e_rms <= MODEL_CEILING, (e_model, e_rms)
    return e_model, e_rms


def inside_ceiling(model_o, want_o, cols=80):
    """whether the reference alone keeps the model inside the ceiling: such a case is asserted, any other only reported"""
    try:
        bounds(model_o, want_o, cols)
    except AssertionError:
        return False
    return True


def errors(got, want, model, cols=80):
    mx, rms = slab_errors(slabs(got, 16, cols), slabs(want, 16, cols), slabs(model, 16, cols))
    return float(mx.max()), float(rms.max())


# --------------------------------------------------------------------------------------------------------------------------------
# the context products
# --------------------------------------------------------------------------------------------------------------------------------
def _products(k, v, wq, wo, gamma, beta, rounding):
    """k / v [B, T, H, D] (fp64), wq / wo [C, C] bf16 values -> K'' [B, H, T, C], cs [B, H, T], bs [B, H, T], V'' [B, C, H, T]"""
    B, T, H, D = k.shape
    C = H * D
    sc = scale32(D)
    wqd, wod = _b(wq), _b(wo)
    kw = torch.einsum("bthd,hdc->bhtc", k, wqd.reshape(H, D, C))
    wqb = wqd @ beta.double()
    if rounding:
        kpp = ((_f32(kw) * torch.tensor(sc, dtype=torch.float32)) * _f32(gamma)).to(torch.bfloat16).double()
        wqb = _f32(wqb).double()
    else:
        kpp = kw * sc * gamma.double()
    cs = kpp.sum(-1)
    bs = torch.einsum("bthd,hd->bht", k, wqb.reshape(H, D)) * sc
    vpp = torch.einsum("nhd,bthd->bnht", wod.reshape(C, H, D), v)
    if rounding:
        cs, bs, vpp = _f32(cs).double(), _f32(bs).double(), _r(vpp)
    return kpp, cs, bs, vpp


def bs_terms(k, wq, beta):
    """the terms of bs [B, H, T, D] as the kernel adds them (k_d x fp32(Wq beta)_d), the scale left out, and what the mat-vec behind them may
    have lost: (relative fp32-sum error of (Wq beta), sum_c |Wq[j][c] beta[c]| per j)"""
    B, T, H, D = k.shape
    wqd = _b(wq)
    mv = wqd * beta.double()[None, :]
    e_mv, a_mv = fp32_sum_error(mv, 1)
    wqb = _f32(mv.sum(1)).double()
    return k.permute(0, 2, 1, 3) * wqb.reshape(1, H, 1, D), e_mv, a_mv.reshape(H, D)


def xattn_inputs(C, B, HW, T, *seed, heads=HEADS, ratio=None, gain=True):
    """-> dict.  x [B, HW, C] (bf16 values, every row its own scale and mean); kv [B, T, 2C], every image its own context; wo / bo scaled by a
    power of two until the attention's increment is at least as large as the residual (gain)"""
    g = TM.gen(C, B, HW, T, heads, *seed)
    x = TM._rows(B * HW, C, g, ratio).reshape(B, HW, C)
    ga, be = TM.affine(C, g)
    wq = bfr(torch.randn(C, C, generator=g) / math.sqrt(C))
    wo = torch.randn(C, C, generator=g) / math.sqrt(C)
    bo = torch.randn(C, generator=g) * 0.1
    kv = torch.randn(B, T, 2 * C, generator=g)
    kv[..., :C] *= K_SCALE
    i = {"x": x, "gamma": ga, "beta": be, "wq": wq, "wo": bfr(wo), "bo": bo, "kv": bfr(kv), "B": B, "HW": HW, "T": T, "C": C, "heads": heads}
    if gain:
        y, _ = xattn_fp64(i)
        x2 = x.double().reshape(-1, C)
        k = TM._gain(float((y - x2).pow(2).mean().sqrt()), float(x2.pow(2).mean().sqrt()))
        i["wo"], i["bo"] = bfr(wo * k), bo * k
    return i


def _kv_heads(i):
    B, T, C, H = i["B"], i["T"], i["C"], i["heads"]
    kv = _b(i["kv"])
    return kv[..., :C].reshape(B, T, H, C // H), kv[..., C:].reshape(B, T, H, C // H)


def xattn_fp64(i):
    """-> (y [M, C], P [B, HW, H, 80] with zero columns t >= T)"""
    B, HW, T, C, H = i["B"], i["HW"], i["T"], i["C"], i["heads"]
    D = C // H
    x = i["x"].double().reshape(B * HW, C)
    k, v = _kv_heads(i)
    q = (TM._ln64(x, i["gamma"], i["beta"], LN_EPS) @ _b(i["wq"]).T).reshape(B, HW, H, D)
    L = torch.einsum("bmhd,bthd->bmht", q, k) * scale32(D)
    P = torch.softmax(L, -1)
    o = torch.einsum("bmht,bthd->bmhd", P, v).reshape(B * HW, C)
    y = o @ _b(i["wo"]).T + i["bo"].double() + x
    return y, torch.nn.functional.pad(P, (0, TP - T))


def xattn_context(i, rounding=True):
    """-> (kpp [B, H, 80, C], cs [B, H, 80], bs [B, H, 80], vpp [B, C, H, 80]), rows / columns t >= T zero"""
    k, v = _kv_heads(i)
    kpp, cs, bs, vpp = _products(k, v, i["wq"], i["wo"], i["gamma"], i["beta"], rounding)
    pad = TP - i["T"]
    return (torch.nn.functional.pad(kpp, (0, 0, 0, pad)), torch.nn.functional.pad(cs, (0, pad)), torch.nn.functional.pad(bs, (0, pad)),
            torch.nn.functional.pad(vpp, (0, pad)))


def xattn_context_fp64(i):
    return xattn_context(i, False)


def xattn_context_model(i):
    return xattn_context(i, True)


# --------------------------------------------------------------------------------------------------------------------------------
# the scores
# --------------------------------------------------------------------------------------------------------------------------------
def slot_stats(x, slots):
    """x [M, C] (bf16 values) -> [M, slots, 2] fp32: the rows' (sum, sum of squares) over `slots` uneven column ranges (widths 1 : 2 : ... : slots)"""
    x = x.double()
    C = x.shape[1]
    edges = [C * j * (j + 1) // (slots * (slots + 1)) for j in range(slots + 1)]
    out = torch.stack([torch.stack([x[:, a:b].sum(1), x[:, a:b].pow(2).sum(1)], -1) for a, b in zip(edges[:-1], edges[1:])], 1)
    return _f32(out)


def _mu_rstd(x, stats, eps, rounding, shift=(0.0, 0.0)):
    """-> (mu, rstd) [M, 1] (fp64 values).  rounding: the kernel's one fp32 pass over the slots' sums; else the exact two-pass statistics.
    shift = (a, b): the summed statistics moved by a x sum |x| and b x sum x^2 (what another fp32 summation order may do to them)"""
    x = x.double()
    C = x.shape[1]
    if not rounding:
        mean, var = TM._ln_stats(x)
        return mean, (var + _eps64(eps)).rsqrt()
    st = slot_stats(x, 1) if stats is None else _f32(stats)
    S, Q = torch.zeros_like(st[:, 0, 0]), torch.zeros_like(st[:, 0, 1])
    for k in range(st.shape[1]):
        S, Q = S + st[:, k, 0], Q + st[:, k, 1]
    S = _f32(S.double() + shift[0] * x.abs().sum(1))
    Q = _f32(Q.double() * (1.0 + shift[1]))
    inv = torch.tensor(1.0 / C, dtype=torch.float32)
    mu = S * inv
    var = (Q * inv - mu * mu).clamp(min=0)
    rstd = (var + torch.tensor(eps, dtype=torch.float32)).rsqrt()
    return mu.double()[:, None], rstd.double()[:, None]


def _softmax_groups(L, H, n, valid, rounding):
    """L [M, >= H n] logits, head h owns columns h n .. h n + n - 1, the first `valid` of them live -> (P fp32 values, P bf16 values), both
    [M, L's width] with every other column zero"""
    M, N = L.shape
    Lh = L[:, :H * n].reshape(M, H, n)[..., :valid]
    p = torch.exp(Lh - Lh.amax(-1, keepdim=True))
    den = p.sum(-1, keepdim=True)
    P = (_f32(p) * (1.0 / _f32(den))).double() if rounding else p / den
    P = torch.nn.functional.pad(torch.nn.functional.pad(P, (0, n - valid)).reshape(M, H * n), (0, N - H * n))
    return P, (_r(P) if rounding else P)


def scores(x, kpp, cs, bs, H, n, valid, eps=LN_EPS, stats=None, rounding=True, shift=(0.0, 0.0)):
    """x [B, HW, C]; kpp [B, N, C], cs / bs [B, N] (N = H n columns and padding) -> (P fp32 [B, HW, N], P bf16 [B, HW, N]) as fp64 values"""
    B, HW, C = x.shape
    x2 = x.double().reshape(B * HW, C)
    mu, rstd = _mu_rstd(x2, stats, eps, rounding, shift)
    N = kpp.shape[1]
    Sx = torch.einsum("bmc,bnc->bmn", x2.reshape(B, HW, C), kpp.double()).reshape(B * HW, N)
    cs2 = cs.double().reshape(B, 1, N).expand(B, HW, N).reshape(B * HW, N)
    bs2 = bs.double().reshape(B, 1, N).expand(B, HW, N).reshape(B * HW, N)
    P, Pb = _softmax_groups(rstd * (Sx - mu * cs2) + bs2, H, n, valid, rounding)
    return P.reshape(B, HW, N), Pb.reshape(B, HW, N)


def xattn_scores(i, ctx, stats=None, rounding=True, shift=(0.0, 0.0), T=None):
    """ctx = (kpp [B, H, 80, C], cs, bs, ...) -> (P fp32, P bf16) [B, HW, H, 80]"""
    B, HW, C, H = i["B"], i["HW"], i["C"], i["heads"]
    P, Pb = scores(i["x"], ctx[0].reshape(B, H * TP, C), ctx[1].reshape(B, H * TP), ctx[2].reshape(B, H * TP), H, TP, i["T"] if T is None else T, LN_EPS,
                   stats, rounding, shift)
    return P.reshape(B, HW, H, TP), Pb.reshape(B, HW, H, TP)


def xattn_output(i, Pb, vpp, rounding=True):
    """y [M, C] = P V''^T + bo + x, per image"""
    B, HW, C = i["B"], i["HW"], i["C"]
    y = torch.einsum("bmk,bnk->bmn", Pb.reshape(B, HW, -1), vpp.reshape(B, C, -1)) + i["bo"].double() + i["x"].double()
    y = y.reshape(B * HW, C)
    return _r(y) if rounding else y


def xattn_model(i, stats=None):
    """-> dict: ctx (the four products), P (fp32 values), Pb (bf16 values) [B, HW, H, 80], y [M, C]"""
    ctx = xattn_context_model(i)
    P, Pb = xattn_scores(i, ctx, stats)
    return {"ctx": ctx, "P": P, "Pb": Pb, "y": xattn_output(i, Pb, ctx[3])}


def xattn_algebra(i):
    """the model with the rounding switched off: must be `xattn_fp64`"""
    ctx = xattn_context_fp64(i)
    P, _ = xattn_scores(i, ctx, rounding=False)
    return xattn_output(i, P, ctx[3], False), P


def recorder_rows(P, b0=0, T=None):
    """P [B, HW, H, 80] -> the recorder's rows [B - b0, H, T, HW]"""
    r = P[b0:].permute(0, 2, 3, 1)
    return r[:, :, :TP if T is None else T].contiguous()


def special_rows(i):
    """rows of zero variance and an all-zero row among the others (first image): row 0 constant 1.5, row 5 zero, row 17 constant -3, row 63 constant 2^-6"""
    x = i["x"].clone()
    x[0, 0], x[0, 5], x[0, 17], x[0, 63] = 1.5, 0.0, -3.0, 2.0 ** -6
    return dict(i, x=x)


def saturated(ctx, T, by=40.0):
    """hand-made bs: token (3 h + 1) % T of head h stands `by` above what it was -- one dominant token per head, in every lane quarter"""
    kpp, cs, bs = ctx[0], ctx[1], ctx[2].clone()
    for h in range(bs.shape[1]):
        bs[:, h, (3 * h + 1) % T] += by
    return kpp, cs, _f32(bs).double()


TIED_PAIRS = [(3, 45), (19, 20), (0, 76)]                 # (a, b): other lane quarters, neighbours across a quarter's edge, first and last token


def tied_inputs(i, pairs=TIED_PAIRS):
    """key b is a copy of key a (the values stay their own): the rows a and b of K'', cs and bs come out identical, and so must the probabilities"""
    kv = i["kv"].clone()
    C = i["C"]
    for a, b in pairs:
        kv[:, b, :C] = kv[:, a, :C]
    return dict(i, kv=kv)


# --------------------------------------------------------------------------------------------------------------------------------
# IP-Adapter
# --------------------------------------------------------------------------------------------------------------------------------
def ipa_inputs(C, heads, nt, B, HW, *seed):
    """-> dict.  h [B, HW, C] bf16 values; kip / vip [B, nt, C] fp32 (to_k_ip / to_v_ip of the tokens); wo scaled by a power of two until half the
    branch (|s| = 0.5) is at least as large as the residual"""
    g = TM.gen(C, heads, nt, B, HW, *seed)
    h = TM._rows(B * HW, C, g, None).reshape(B, HW, C)
    ga, be = TM.affine(C, g)
    wq = bfr(torch.randn(C, C, generator=g) / math.sqrt(C))
    wo = torch.randn(C, C, generator=g) / math.sqrt(C)
    kip = torch.randn(B, nt, C, generator=g) * K_SCALE
    vip = torch.randn(B, nt, C, generator=g)
    i = {"h": h, "gamma": ga, "beta": be, "wq": wq, "wo": bfr(wo), "kip": kip, "vip": vip, "B": B, "HW": HW, "C": C, "heads": heads, "nt": nt}
    h2 = h.double().reshape(-1, C)
    y, _ = ipa_fp64(i, 0.5)
    k = TM._gain(float((y - h2).pow(2).mean().sqrt()), float(h2.pow(2).mean().sqrt()))
    i["wo"] = bfr(wo * k)
    return i


def _ip_heads(i):
    B, nt, C, H = i["B"], i["nt"], i["C"], i["heads"]
    return i["kip"].double().reshape(B, nt, H, C // H), i["vip"].double().reshape(B, nt, H, C // H)


def ipa_fp64(i, s):
    """-> (h' [M, C], P [B, HW, colsP] with zero padding)"""
    B, HW, C, H, nt = i["B"], i["HW"], i["C"], i["heads"], i["nt"]
    D = C // H
    h = i["h"].double().reshape(B * HW, C)
    k, v = _ip_heads(i)
    q = (TM._ln64(h, i["gamma"], i["beta"], LN_EPS) @ _b(i["wq"]).T).reshape(B, HW, H, D)
    P = torch.softmax(torch.einsum("bmhd,bthd->bmht", q, k) * scale32(D), -1)
    o = torch.einsum("bmht,bthd->bmhd", P, v).reshape(B * HW, C)
    return h + s * (o @ _b(i["wo"]).T), torch.nn.functional.pad(P.reshape(B, HW, H * nt), (0, ipa_cols(H, nt) - H * nt))


def ipa_context(i, rounding=True):
    """-> (kpp [B, colsP, C], cs [B, colsP], bs [B, colsP], vpp [B, C, colsP]); col = head * nt + token, padded with zeros"""
    B, C, H, nt = i["B"], i["C"], i["heads"], i["nt"]
    k, v = _ip_heads(i)
    kpp, cs, bs, vpp = _products(k, v, i["wq"], i["wo"], i["gamma"], i["beta"], rounding)
    pad = ipa_cols(H, nt) - H * nt
    return (torch.nn.functional.pad(kpp.reshape(B, H * nt, C), (0, 0, 0, pad)), torch.nn.functional.pad(cs.reshape(B, H * nt), (0, pad)),
            torch.nn.functional.pad(bs.reshape(B, H * nt), (0, pad)), torch.nn.functional.pad(vpp.reshape(B, C, H * nt), (0, pad)))


def ipa_scores(i, ctx, rounding=True):
    """-> (P fp32, P bf16) [B, HW, colsP]"""
    return scores(i["h"], ctx[0], ctx[1], ctx[2], i["heads"], i["nt"], i["nt"], LN_EPS, None, rounding)


def ipa_add(h, P, vpp, s, rounding=True):
    """h [B, HW, C], P [B, HW, colsP], vpp [B, C, colsP] -> h' [M, C]; s is taken as the fp32 value the kernel gets"""
    B, HW, C = h.shape
    s = float(torch.tensor(s, dtype=torch.float32))
    y = (h.double() + s * torch.einsum("bmk,bnk->bmn", P.double(), vpp.double())).reshape(B * HW, C)
    return _r(y) if rounding else y


def ipa_model(i, s):
    ctx = ipa_context(i, True)
    P, Pb = ipa_scores(i, ctx)
    return {"ctx": ctx, "P": P, "Pb": Pb, "y": ipa_add(i["h"], Pb, ctx[3], s)}


def ipa_algebra(i, s):
    ctx = ipa_context(i, False)
    P, _ = ipa_scores(i, ctx, False)
    return ipa_add(i["h"], P, ctx[3], s, False), P


def ipa_add_inputs(C, HW, *seed, B=2, heads=8, nt=4):
    """hand-made operands of ipa_add alone: h [B, HW, C] bf16 values, P [B, HW, colsP] bf16 probabilities (a softmax per head, zero padding),
    vpp [B, C, colsP] bf16 values scaled (by a power of two) so that half the product is at least as large as h"""
    g = TM.gen(C, HW, B, heads, nt, *seed)
    colsP = ipa_cols(heads, nt)
    h = TM._rows(B * HW, C, g, None).reshape(B, HW, C)
    P = torch.softmax(torch.randn(B, HW, heads, nt, generator=g) * 1.5, -1).reshape(B, HW, heads * nt)
    P = bfr(torch.nn.functional.pad(P, (0, colsP - heads * nt)))
    v = torch.nn.functional.pad(torch.randn(B, C, heads * nt, generator=g), (0, colsP - heads * nt))
    inc = 0.5 * torch.einsum("bmk,bnk->bmn", P.double(), v.double())
    k = TM._gain(float(inc.pow(2).mean().sqrt()), float(h.double().pow(2).mean().sqrt()))
    return {"h": h, "P": P, "vpp": bfr(v * k), "B": B, "HW": HW, "C": C, "colsP": colsP}


def linear_terms(x, w, bias):
    """the terms of ipa_linear's sums [R, N, K (+ 1)]: x[r][k] bf16(w)[n][k], and the bias as one more term"""
    t = x.double()[:, None, :] * _b(w)[None, :, :]
    if bias is not None:
        t = torch.cat([t, bias.double()[None, :, None].expand(t.shape[0], -1, 1)], -1)
    return t


def layernorm_inputs(rows, C, ratio, *seed):
    """fp32 rows, every row its own scale and mean (ratio x sigma, the sign alternating); row 1 (where there is one) constant 1.5"""
    g = TM.gen(rows, C, int(ratio), *seed)
    z = torch.randn(rows, C, generator=g)
    sig = 2.0 ** torch.randint(-1, 2, (rows, 1), generator=g).float()
    x = (z + float(ratio) * (1 - 2 * (torch.arange(rows)[:, None] % 2))) * sig
    if rows > 1:
        x[1] = 1.5
    ga, be = TM.affine(C, g)
    return x, ga, be


def layernorm_fp64(x, g, b, eps=LN_EPS):
    return TM._ln64(x.double(), g, b, eps)


def wave_sum32(v):
    """[rows, C] fp32 -> [rows, 1]: the sum as one wave takes it, every addition in fp32 -- lane l adds columns l, l + 64, ... in turn, then the 64
    lanes halve five times and once more (the xor shuffles 32, 16, .. 1).  (torch's own cumsum / sum are no stand-in: on the CPU they accumulate
    an fp32 row in fp64 or in blocks)"""
    rows, C = v.shape
    v = torch.nn.functional.pad(v, (0, (-C) % 64)).reshape(rows, -1, 64)
    s = torch.zeros(rows, 64, dtype=torch.float32)
    for k in range(v.shape[1]):
        s = s + v[:, k]
    w = 32
    while w >= 1:
        s = s[:, :w] + s[:, w:2 * w]
        w //= 2
    return s


def layernorm_model(x, g, b, eps=LN_EPS):
    """two passes, every operation in fp32, both sums in the kernel's order (`wave_sum32`)"""
    x = _f32(x)
    C = x.shape[1]
    mu = wave_sum32(x) / float(C)
    d = x - mu
    rstd = (wave_sum32(d * d) / float(C) + torch.tensor(eps, dtype=torch.float32)).rsqrt()
    return (d * rstd * _f32(g) + _f32(b)).double()


# --------------------------------------------------------------------------------------------------------------------------------
# the cases both test files walk
# --------------------------------------------------------------------------------------------------------------------------------
# (B, T, C, heads): the production shape, a batch with fewer tokens, the full 80 rows, one token; D = 80 (a ragged last 32-deep k step); D = 40;
# D = 80 with four heads; the fragment edge (16 | 17) and the 64-row block edge (64 | 65) of the 80-row K'' tile
CONTEXT_CASES = [(1, 77, 1280, 8), (2, 50, 1280, 8), (1, 80, 1280, 8), (3, 1, 1280, 8), (1, 77, 640, 8), (2, 33, 640, 8), (1, 21, 320, 8), (1, 21, 320, 4),
                 (1, 16, 320, 8), (1, 17, 320, 8), (1, 64, 320, 8), (1, 65, 320, 8)]

XS_SHAPES = [(1, 64), (3, 64), (2, 128)]
XS_C = (320, 640, 1280)
XS_T = (1, 19, 20, 21, 40, 41, 77, 80)                    # lane q owns tokens 20 q .. 20 q + 19
XS_SLOTS = (1, 5, 8)
# (C, T, B, HW, slots): every C with every T; within a C every (B, HW) and every slot count, and over the list every (B, HW) x slots pair
XS_CASES = [(C, T, *XS_SHAPES[(ti + ci) % 3], XS_SLOTS[(ti // 3 + ti + ci) % 3]) for ci, C in enumerate(XS_C) for ti, T in enumerate(XS_T)]
XS_RATIOS = (0, 4, 32, 128)                               # 0 and 4 asserted; 32 and 128 where the model alone is inside the ceiling
XS_RATIO_SHAPE = (1, 64, 77)                              # (B, HW, T), at every C
XS_REC_T = ("T", "T-1", 20, 1)

# the shapes of test_xattn_premul_matches_torch cut to HW = 64 or 128: (B, HW, T, C)
E2E_CASES = [(2, 128, 77, 1280), (1, 64, 77, 1280), (2, 128, 50, 1280), (1, 128, 80, 1280), (3, 64, 1, 1280), (2, 128, 77, 640), (1, 128, 33, 640)]

# (R, N, K): R N = 15, 126, 7 leave the last workgroup of four outputs ragged; 128 fills it
IPA_LINEAR_CASES = [(3, 5, 1), (2, 64, 1), (3, 5, 63), (2, 63, 63), (3, 5, 64), (2, 64, 64), (3, 5, 65), (2, 63, 65), (3, 5, 1024), (1, 7, 1024)]
# (rows, C): 37 and 21 rows leave the last workgroup of four rows ragged and make three and two row tiles
IPA_LN_CASES = [(37, C) for C in (1, 63, 64, 65, 768)] + [(21, 768)]
IPA_LN_RATIOS = (0, 4, 32, 128, 512)
IPA_C = ((72, 3), (320, 8), (1280, 8))                    # (C, heads): D = 24 (C % 32 = 8: a ragged last k step), 40, 160
IPA_NT = (1, 4, 5, 7, 10)
IPA_HW = (1, 16, 64, 100)
IPA_ADD_HW = (1, 64, 100)
IPA_S = (0.0, 1.0, -0.5)


def ipa_nt_inst(heads, nt):
    """the instantiation of ipa_scores_kernel a case expects: NT = colsP / 16"""
    return ipa_cols(heads, nt) // 16
