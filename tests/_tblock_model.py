"""What the row-panel transformer-block tests compare csrc/tblock.hip with, on the CPU in fp64 (no test in here), and the case lists that
tests/test_tblock_ops_gpu.py and tests/test_tblock_model_cpu.py share.

For each chain two functions on the bf16-rounded inputs:

`qkv_fp64` / `ff_fp64` / `attn_fp64`     the operation itself, nothing else rounded: two-pass statistics, exact erf, explicit softmax.
`qkv_model` / `ff_model` / `attn_model`  the same with the roundings the kernels' comments declare and nothing else (the GEMMs stay exact):
  qkv chain   GroupNorm inside: rows := bf16(x sc + sh) with sc = rstd gamma, sh = beta - mean sc in fp32 (`_norm_model.groupnorm_model`);
              folded: Wb = bf16(W gamma rstd), rowadd = bias + W beta - Wb mu (`_norm_model.fold_model`); h to bf16; norm1's statistics from
              the rounded h; normalised rows to bf16; q / k / v to bf16.
  feed-forward  the folded LayerNorm: W1' = bf16(W1 gamma), cs = the column sums of W1', b1' = b1 + W1 beta, u = rstd (x W1'^T - mu cs) + b1';
              hidden activation value * gelu(gate) to bf16; POST = 0: y = bf16(hidden W2^T + b2 + x).  POST = 1 rounds that y to bf16 (it is
              written back into the LDS panel as h3) and then pout = bf16(h3 Wp^T + bp + xres): two roundings.  POST = 2 forms no h3: pout =
              bf16(hidden (Wp W2)^T + x Wp^T + (Wp b2 + bp) + xres) with Wp W2 rounded to bf16 once at load time: one rounding of the
              activations, one of the product matrix.
  attention chain  h1 = bf16(o1 Wo1^T + bo1 + x) (prologue), norm2's statistics from the rounded h1; normalised rows to bf16; Q to bf16; the
              un-normalised probabilities exp(l - max) to bf16 before P V; O = (P V) / sum to bf16; y = bf16(O Wo^T + bo + h1).  The recorder
              adds the fp32 probabilities (not the bf16 ones).
Their distance from the fp64 functions is the error a correct kernel is entitled to; the tests bound the kernel by `MODEL_FACTOR` x that distance.

`slabs` / `slab_errors`  the measure: every slab of 16 rows x 80 columns on its own -- one MFMA row tile of one wave's column range -- max |error|
              over the slab's max |value| and RMS error over the slab's RMS, so that no row tile, wave, column quarter, panel or image hides
              behind another.  Outputs that carry a residual are judged on inputs whose increment is at least as large (RMS) as the residual
              (`residual_condition`), so that the residual cannot hide the function either."""
import math

import torch
from _attn_model import MODEL_CEILING, MODEL_FACTOR, bfr  # noqa: F401  (re-exported)
from _norm_model import fold_model, groupnorm_fp64, groupnorm_model, partials, slab_errors  # noqa: F401

HEADS = 8
GN_EPS = 1e-6
LN_EPS = 1e-5


def _b(t):
    """bf16-rounded values in fp64"""
    return t.detach().float().cpu().to(torch.bfloat16).double()


def _f32(t):
    return t.to(torch.float32)


def _eps64(eps):
    return float(torch.tensor(eps, dtype=torch.float32))


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def affine(C, g):
    return torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.2 + 0.1


def _ln_stats(x):
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return mean, var


def _ln64(x, g, b, eps):
    mean, var = _ln_stats(x)
    return (x - mean) * (var + _eps64(eps)).rsqrt() * g.double() + b.double()


def _ln_model(x, g, b, eps):
    """x: bf16 values (fp64).  Exact statistics cast to fp32, (v - mean) * rstd * g + b in fp32 left to right, one rounding to bf16"""
    mean, var = _ln_stats(x)
    r = (_f32(x) - _f32(mean)) * _f32((var + _eps64(eps)).rsqrt()) * _f32(g) + _f32(b)
    return r.to(torch.bfloat16).double()


def _r(t):
    """fp64 -> fp32 (the accumulator) -> bf16"""
    return _f32(t).to(torch.bfloat16).double()


# --------------------------------------------------------------------------------------------------------------------------------
# the measure
# --------------------------------------------------------------------------------------------------------------------------------
def slabs(t, rows=16, cols=80):
    """[M, N] -> [ceil(M / 16), N / 80, 16 * 80]; a ragged last row tile is padded with zeros in every operand alike, which changes neither measure"""
    t = t.detach().double().cpu()
    t = t.reshape(-1, t.shape[-1])
    M, N = t.shape
    assert N % cols == 0
    t = torch.nn.functional.pad(t, (0, 0, 0, (-M) % rows))
    return t.reshape(-1, rows, N // cols, cols).permute(0, 2, 1, 3).reshape(-1, N // cols, rows * cols)


def model_bounds(model_o, want_o):
    """(E_model, E_rms) over the 16 x 80 slabs of [M, N] operands; refuses a case that proves too little"""
    mx, rms = slab_errors(slabs(model_o), slabs(want_o), slabs(model_o))
    e_model, e_rms = float(mx.max()), float(rms.max())
    assert 0 < MODEL_FACTOR * e_model <= MODEL_CEILING and 0 < MODEL_FACTOR * e_rms <= MODEL_CEILING, (e_model, e_rms)
    return e_model, e_rms


def kernel_errors(got, want, model):
    mx, rms = slab_errors(slabs(got), slabs(want), slabs(model))
    return float(mx.max()), float(rms.max())


def residual_condition(out, residual):
    """RMS of the increment out - residual over the RMS of the residual (row m of the output carries residual row m % rows): must be >= 1"""
    out, residual = out.double().reshape(-1, out.shape[-1]), residual.double().reshape(-1, residual.shape[-1])
    res = residual.repeat(out.shape[0] // residual.shape[0], 1)
    return float((out - res).pow(2).mean().sqrt() / res.pow(2).mean().sqrt())


def abs_bound(model_t, want_t, hpb=1):
    """for recorder rows: MODEL_FACTOR x (the model's largest absolute error + what fp32 itself costs).  A recorded value is the fp32 sum of
    hpb probabilities <= 1, each made by an exp2, a reciprocal and a product of about one ulp each: hpb x 4 x 2^-24 -- the floor that keeps a
    case judgeable whose probabilities the model happens to hit exactly (one key, equal logits, a saturated softmax)"""
    return MODEL_FACTOR * (float((model_t.double() - want_t.double()).abs().max()) + hpb * 2.0 ** -22)


def fp32_sum_error(v, dim):
    """what an fp32 sum of `v` (fp64 holding fp32-exact values) along `dim` may lose, from two fp32 sums in other orders than the kernel's (a
    running sum and torch's blocked one), relative to sum |v|: the worst entry.  -> (relative error, sum |v|)"""
    exact, scale = v.sum(dim), v.abs().sum(dim)
    v32 = _f32(v)
    run = v32.cumsum(dim).select(dim, -1).double()
    blk = v32.sum(dim).double()
    e = torch.maximum((run - exact).abs(), (blk - exact).abs()) / scale
    return float(e.max()), scale


# --------------------------------------------------------------------------------------------------------------------------------
# qkv chain: GroupNorm -> proj_in -> h -> norm1 -> q | k | v
# --------------------------------------------------------------------------------------------------------------------------------
def qkv_inputs(C, B, HW, groups, *seed, ratio=None):
    """-> dict.  x [B, HW, C] (bf16 values): every (image, group) with its own scale 2^-2 .. 2^2 and its own mean (|mean| <= sigma, or ratio x
    sigma with the sign alternating between groups and images)"""
    g = gen(C, B, HW, groups, *seed)
    z = torch.randn(B, HW, C, generator=g)
    sig = 2.0 ** torch.randint(-2, 3, (B, groups), generator=g).float()
    if ratio is None:
        mu = (torch.randn(B, groups, generator=g) * 0.5).clamp(-1, 1)
    else:
        mu = float(ratio) * (1 - 2 * ((torch.arange(groups)[None, :] + torch.arange(B)[:, None]) % 2)).float()
    cpg = C // groups
    x = bfr((z + mu.repeat_interleave(cpg, 1)[:, None, :]) * sig.repeat_interleave(cpg, 1)[:, None, :])
    gg, gb = affine(C, g)
    g1, b1 = affine(C, g)
    return {"x": x, "groups": groups, "gn_gamma": gg, "gn_beta": gb, "w_in": bfr(torch.randn(C, C, generator=g) / math.sqrt(C)),
            "b_in": torch.randn(C, generator=g) * 0.1, "gamma": g1, "beta": b1, "wqkv": bfr(torch.randn(3 * C, C, generator=g) / math.sqrt(C))}


def _nchw(x):
    return x.transpose(1, 2).contiguous()                  # [B, HW, C] -> [B, C, HW]


def qkv_fp64(i):
    x = i["x"]
    B, HW, C = x.shape
    y = groupnorm_fp64(_nchw(x), None, i["groups"], i["gn_gamma"], i["gn_beta"], GN_EPS, False).transpose(1, 2).reshape(B * HW, C)
    h = y @ _b(i["w_in"]).T + i["b_in"].double()
    return h, _ln64(h, i["gamma"], i["beta"], LN_EPS) @ _b(i["wqkv"]).T


def qkv_model(i, inside):
    x = i["x"]
    B, HW, C = x.shape
    if inside:
        y = groupnorm_model(_nchw(x), None, i["groups"], i["gn_gamma"], i["gn_beta"], GN_EPS, False).transpose(1, 2).reshape(B * HW, C)
        h = _r(y @ _b(i["w_in"]).T + _f32(i["b_in"]).double())
    else:
        h = _r(fold_model(_nchw(x), i["groups"], i["gn_gamma"], i["gn_beta"], GN_EPS, i["w_in"], i["b_in"])["y"].reshape(B * HW, C))
    return h, _r(_ln_model(h, i["gamma"], i["beta"], LN_EPS) @ _b(i["wqkv"]).T)


def qkv_part(i, bm):
    return partials(_b(i["x"]), bm)


# --------------------------------------------------------------------------------------------------------------------------------
# feed-forward: norm3 -> GEGLU -> ff.net.2 + residual (-> proj_out + bias + residual)
# --------------------------------------------------------------------------------------------------------------------------------
def _rows(M, C, g, ratio):
    """[M, C] bf16 values: every row with its own scale 2^-1 .. 2^1 and its own mean (|mean| <= sigma, or ratio x sigma, the sign alternating
    between rows)"""
    z = torch.randn(M, C, generator=g)
    sig = 2.0 ** torch.randint(-1, 2, (M, 1), generator=g).float()
    mu = torch.randn(M, 1, generator=g).clamp(-2, 2) * 0.5 if ratio is None else torch.full((M, 1), float(ratio)) * (1 - 2 * (torch.arange(M)[:, None] % 2))
    return bfr((z + mu) * sig)


def _gain(inc_rms, res_rms):
    """the power of two that lifts an increment of RMS inc_rms to at least 1.25 x res_rms"""
    return 2.0 ** math.ceil(math.log2(1.25 * res_rms / inc_rms))


def ff_inputs(M, *seed, ratio=None, tails=False, xres_rows=0, C=320):
    """-> dict.  tails: the gate bias spreads the gate pre-activations over -12 .. 12.  w2 / b2 are scaled (by a power of two) until the
    feed-forward's increment is at least as large as the residual rows"""
    g = gen(M, C, *seed)
    x = _rows(M, C, g, ratio)
    ga, be = affine(C, g)
    w1 = bfr(torch.randn(8 * C, C, generator=g) / math.sqrt(C))
    b1 = torch.randn(8 * C, generator=g) * 0.1
    if tails:
        b1[4 * C:] = torch.linspace(-12, 12, 4 * C)[torch.randperm(4 * C, generator=g)]
    w2 = torch.randn(C, 4 * C, generator=g) / math.sqrt(4 * C)
    b2 = torch.randn(C, generator=g) * 0.1
    wp = bfr(torch.randn(C, C, generator=g) / math.sqrt(C))
    bp = torch.randn(C, generator=g) * 0.1
    i = {"x": x, "gamma": ga, "beta": be, "w1": w1, "b1": b1, "w2": bfr(w2), "b2": b2, "wp": wp, "bp": bp, "xres_rows": xres_rows}
    inc = ff_fp64(i)[0] - x.double()
    k = _gain(float(inc.pow(2).mean().sqrt()), float(x.double().pow(2).mean().sqrt()))
    i["w2"], i["b2"] = bfr(w2 * k), b2 * k
    xr = torch.randn(xres_rows if xres_rows else M, C, generator=g)
    i["xres"] = bfr(xr * float(x.double().pow(2).mean().sqrt()))
    return i


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def _xres(i, M):
    xr = _b(i["xres"])
    return xr.repeat(M // xr.shape[0], 1)


def ff_fp64(i, post=False):
    """-> (y, pout or None)"""
    x = i["x"].double()
    C = x.shape[1]
    u = _ln64(x, i["gamma"], i["beta"], LN_EPS) @ _b(i["w1"]).T + i["b1"].double()
    y = x + (u[:, :4 * C] * _gelu64(u[:, 4 * C:])) @ _b(i["w2"]).T + i["b2"].double()
    return y, (y @ _b(i["wp"]).T + i["bp"].double() + _xres(i, x.shape[0])) if post else None


def premul_fp64(i):
    """(Wp W2, Wp b2 + bp) in fp64 from the bf16 matrices"""
    wp = _b(i["wp"])
    return wp @ _b(i["w2"]), wp @ i["b2"].double() + i["bp"].double()


def ff_hidden_model(i):
    x = i["x"].double()
    C = x.shape[1]
    w1 = _f32(_b(i["w1"]))
    w1f = (w1 * _f32(i["gamma"])[None, :]).to(torch.bfloat16).double()                 # fp32 product, one rounding
    cs = w1f.sum(1)
    b1f = i["b1"].double() + w1.double() @ i["beta"].double()
    mean, var = _ln_stats(x)
    mu32, rs32 = _f32(mean).double(), _f32((var + _eps64(LN_EPS)).rsqrt()).double()
    u = rs32 * (x @ w1f.T - mu32 * cs[None, :]) + b1f[None, :]
    return _r(u[:, :4 * C] * _gelu64(u[:, 4 * C:]))


def ff_model(i, post=0):
    """post 0 -> y; 1 -> pout through the rounded h3; 2 -> pout through the pre-multiplied matrix (no h3)"""
    x = i["x"].double()
    hid = ff_hidden_model(i)
    if post == 2:
        w2p, bcp = premul_fp64(i)
        return _r(hid @ _r(w2p).T + x @ _b(i["wp"]).T + _f32(bcp).double() + _xres(i, x.shape[0]))
    y = _r(hid @ _b(i["w2"]).T + i["b2"].double() + x)
    return y if post == 0 else _r(y @ _b(i["wp"]).T + i["bp"].double() + _xres(i, x.shape[0]))


# --------------------------------------------------------------------------------------------------------------------------------
# attention chain: (attn1.to_out + residual ->) norm2 -> to_q -> cross-attention -> to_out + bias + residual
# --------------------------------------------------------------------------------------------------------------------------------
def attn_inputs(C, B, HW, T, *seed, ratio=None, pre=False, src_rows=0, peaked=False):
    """-> dict.  x (and o1) [B, HW, C], or with src_rows [src_rows, C]; kv [B, T, 2C], every image its own context.  peaked (B >= 2): norm2's
    beta is about 1, so every Q row shares the component Wq beta, and key 0 of image 0 is laid along it head by head, long enough that its
    logits stand about 40 above the rest (the row maximum decides everything); the keys of image 1 are all the same vector, so every one
    of its rows has all logits equal (bit for bit in any arithmetic) and attends to the mean of V"""
    g = gen(C, B, HW, T, *seed, int(pre), src_rows)
    rows = src_rows if src_rows else B * HW
    x = _rows(rows, C, g, ratio)
    ga, be = affine(C, g)
    D = C // HEADS
    wq = bfr(torch.randn(C, C, generator=g) / math.sqrt(C))
    kv = torch.randn(B, T, 2 * C, generator=g)
    kv[..., :C] *= 1.5
    i = {"gamma": ga, "beta": be, "wq": wq, "bo": torch.randn(C, generator=g) * 0.1, "B": B, "HW": HW, "T": T, "src_rows": src_rows}
    if pre:
        i["o1"] = bfr(torch.randn(rows, C, generator=g))
        i["wo1"] = bfr(torch.randn(C, C, generator=g) / math.sqrt(C))
        i["bo1"] = torch.randn(C, generator=g) * 0.1
    if peaked:
        i["beta"] = be = 1.0 + torch.randn(C, generator=g) * 0.1
        qd = (wq.double() @ be.double()).view(HEADS, D)
        kv[0, 0, :C] = (qd * (40.0 * math.sqrt(D) / qd.pow(2).sum(1, keepdim=True))).reshape(C).float()
        kv[1, :, :C] = kv[1, :1, :C]
    i["x"] = x
    i["kv"] = bfr(kv)
    wo = torch.randn(C, C, generator=g) / math.sqrt(C)
    i["wo"] = bfr(wo)
    y, h1, _ = attn_fp64(i)
    k = _gain(float((y - h1).pow(2).mean().sqrt()), float(h1.pow(2).mean().sqrt()))
    i["wo"], i["bo"] = bfr(wo * k), i["bo"] * k
    return i


def _expand(i, t):
    """input rows [src_rows or M, C] -> [M, C]"""
    M = i["B"] * i["HW"]
    t = t.double().reshape(-1, t.shape[-1])
    return t.repeat(M // t.shape[0], 1)


def _attend(i, h1, xn, model):
    B, HW, T = i["B"], i["HW"], i["T"]
    C = h1.shape[1]
    D = C // HEADS
    rq = _r if model else (lambda t: t)
    Q = rq(xn @ _b(i["wq"]).T).reshape(B, HW, HEADS, D).permute(0, 2, 1, 3)
    kv = _b(i["kv"])
    K = kv[..., :C].reshape(B, T, HEADS, D).permute(0, 2, 1, 3)
    V = kv[..., C:].reshape(B, T, HEADS, D).permute(0, 2, 1, 3)
    L = (Q @ K.transpose(-1, -2)) * float(torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32))
    p = torch.exp(L - L.amax(-1, keepdim=True))
    den = p.sum(-1, keepdim=True)
    O = rq(((_r(p) if model else p) @ V) / den).permute(0, 2, 1, 3).reshape(B * HW, C)
    y = rq(O @ _b(i["wo"]).T + i["bo"].double() + h1)
    if model:                                              # the recorded probabilities are fp32: p * (1 / sum)
        return y, (_f32(p) * (1.0 / _f32(den))).double()
    return y, p / den                                      # probabilities [B, H, HW, T]


def attn_fp64(i):
    """-> (y [M, C], h1 [M, C] (= x without the prologue), probabilities [B, H, HW, T])"""
    h1 = _expand(i, i["x"])
    if "o1" in i:
        h1 = h1 + _expand(i, i["o1"]) @ _b(i["wo1"]).T + i["bo1"].double()
    y, P = _attend(i, h1, _ln64(h1, i["gamma"], i["beta"], LN_EPS), False)
    return y, h1, P


def attn_model(i):
    h1 = _expand(i, i["x"])
    if "o1" in i:
        h1 = _r(h1 + _expand(i, i["o1"]) @ _b(i["wo1"]).T + i["bo1"].double())
    y, P = _attend(i, h1, _ln_model(h1, i["gamma"], i["beta"], LN_EPS), True)
    return y, h1, P


def recorder_rows(P, hpb, b0=0, T=None):
    """probabilities [B, H, HW, T] -> the recorder's rows [B - b0, H / hpb, T, HW]: head groups of hpb summed, token-major"""
    B, H, HW, Tk = P.shape
    r = P[b0:].reshape(B - b0, H // hpb, hpb, HW, Tk).sum(2).transpose(-1, -2)
    return r[:, :, :Tk if T is None else T].contiguous()


# --------------------------------------------------------------------------------------------------------------------------------
# the cases both test files walk
# --------------------------------------------------------------------------------------------------------------------------------
# (C, B, HW, bm, groups): one panel of one image; three images with their own statistics; more than one tile per image, both tile heights;
# 33 and 40 tiles (across the 16-load round of qkv_chain_kernel and the 32-load round of qkv_chain2_kernel); groups 8 and 1
QKV_SHAPES_320 = [(320, 1, 64, 64, 32), (320, 1, 128, 64, 32), (320, 3, 128, 64, 32), (320, 1, 384, 64, 32), (320, 1, 384, 128, 32), (320, 1, 2112, 64, 32),
                  (320, 1, 2560, 64, 32), (320, 2, 128, 128, 8), (320, 2, 128, 32, 1)]
QKV_SHAPES_640 = [(640, 1, 64, 64, 32), (640, 3, 128, 64, 32), (640, 1, 384, 128, 32), (640, 1, 2112, 64, 32), (640, 2, 128, 64, 8), (640, 2, 64, 32, 1)]
RATIOS_ASSERTED = (0, 4, 32)
RATIOS_REPORTED = (128, 512)
QKV_RATIO_SHAPE = {320: (320, 2, 256, 64, 32), 640: (640, 2, 128, 64, 32)}

# (name, M, post forms, keyword arguments of ff_inputs)
FF_CASES = [("one panel", 128, (0, 1, 2), {}), ("four panels", 512, (0, 1, 2), {}), ("ragged tail", 1000, (0, 1, 2), {}),
            ("shared residual", 512, (1, 2), {"xres_rows": 256}), ("gate tails", 128, (0, 1, 2), {"tails": True})]
FF_RATIO_M = 256

# (C, rows32) -> rows per workgroup
ATTN_FORMS = [(320, False), (640, False), (640, True)]
ATTN_T = (1, 16, 17, 64, 77, 96)


def attn_bm(C, rows32):
    return 128 if C == 320 else 32 if rows32 else 64
