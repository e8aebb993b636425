"""What the normalisation tests compare csrc/norm.hip with, on the CPU in fp64 (no test in here):

`groupnorm_fp64` / `layernorm_fp64`    the operation itself on the bf16-rounded inputs (two-pass statistics in fp64, nothing else rounded).
`groupnorm_model` / `layernorm_model`  the same with the roundings the kernels declare and nothing else: the statistics exact, then cast to
                   fp32; GroupNorm: sc = rstd * gamma and sh = beta - mean * sc in fp32, one fma per element, SiLU in fp32, one rounding to
                   bf16; LayerNorm: (v - mean) * rstd * g + b in fp32, one rounding to bf16.  Their distance from the fp64 functions is the
                   error a correct kernel is entitled to; the tests bound the kernel by `MODEL_FACTOR` x that distance, case by case.
`fold_fp64` / `fold_model`             the GroupNorm folded into the projection behind it: Wb = bf16(W rstd gamma) per image,
                   rowadd = bias + W beta - Wb mu, y = x Wb^T + rowadd (model) against linear(GroupNorm(x)) in fp64 (reference).
`partials`         the partial-sum tables the producing GEMM leaves in production, made on the host: per (image, tile of bm pixels, channel)
                   the sum and the sum of squares, summed in fp64 and rounded to fp32 once.
`slab_errors`      the measure: every slab on its own -- max |error| over the slab's max |value|, and RMS error over the slab's RMS -- so
                   that no group, image or row hides behind a larger one.  GroupNorm: (image, group) slabs; LayerNorm: rows; the folded
                   projection: (image, block of 16 output columns)."""
import torch
import torch.nn.functional as F

from _attn_model import MODEL_CEILING, MODEL_FACTOR, bfr  # noqa: F401  (re-exported: the tests take them from here)


def _bf64(t):
    return t.detach().float().cpu().to(torch.bfloat16).double()


def _f32(t):
    return t.to(torch.float32)


def _eps64(eps):
    return float(torch.tensor(eps, dtype=torch.float32))          # the kernels widen the fp32 eps they are handed


def _cat(x0, x1):
    x = _bf64(x0)
    return x if x1 is None else torch.cat([x, _bf64(x1)], 1)


def _gn_stats(x, groups):
    """exact (fp64, two-pass) mean and 1 / sqrt(var + eps) inputs per (image, group): -> mean [B, G], var [B, G]"""
    B = x.shape[0]
    xs = x.reshape(B, groups, -1)
    mean = xs.mean(-1)
    var = (xs - mean[..., None]).pow(2).mean(-1)
    return mean, var


def _per_channel(t, C):
    """[B, G] -> [B, C, 1]"""
    return t.repeat_interleave(C // t.shape[1], 1)[..., None]


def groupnorm_fp64(x0, x1, groups, gamma, beta, eps, silu):
    x = _cat(x0, x1)
    B, C = x.shape[:2]
    mean, var = _gn_stats(x, groups)
    rstd = (var + _eps64(eps)).rsqrt()
    y = (x.reshape(B, C, -1) - _per_channel(mean, C)) * _per_channel(rstd, C) * gamma.double()[None, :, None] + beta.double()[None, :, None]
    if silu:
        y = y * torch.sigmoid(y)
    return y.reshape(x.shape)


def groupnorm_model(x0, x1, groups, gamma, beta, eps, silu):
    x = _cat(x0, x1)
    B, C = x.shape[:2]
    mean, var = _gn_stats(x, groups)
    mean32, rstd32 = _f32(mean), _f32((var + _eps64(eps)).rsqrt())
    sc = _per_channel(rstd32, C) * _f32(gamma)[None, :, None]                         # fp32 product
    sh = _f32(beta)[None, :, None] - _per_channel(mean32, C) * sc                     # fp32 product, fp32 difference
    r = _f32(x.reshape(B, C, -1) * sc.double() + sh.double())                         # one fma: the fp64 expression is exact up to its one rounding
    if silu:
        r = r / (1.0 + torch.exp(-r))                                                 # fp32
    return r.to(torch.bfloat16).double().reshape(x.shape)


def layernorm_fp64(x, gamma, beta, eps):
    x = _bf64(x)
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return (x - mean) * (var + _eps64(eps)).rsqrt() * gamma.double() + beta.double()


def layernorm_model(x, gamma, beta, eps):
    x = _bf64(x)
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    mean32, rstd32 = _f32(mean), _f32((var + _eps64(eps)).rsqrt())
    r = (_f32(x) - mean32) * rstd32 * _f32(gamma) + _f32(beta)                        # fp32, left to right
    return r.to(torch.bfloat16).double()


# --------------------------------------------------------------------------------------------------------------------------------
# the fold
# --------------------------------------------------------------------------------------------------------------------------------
def fold_fp64(x, groups, gamma, beta, eps, w, bias):
    """linear(GroupNorm(x)) in fp64 on the bf16-rounded x and W: -> y [B, HW, N]"""
    y = groupnorm_fp64(x, None, groups, gamma, beta, eps, False)
    B, C = y.shape[:2]
    out = y.reshape(B, C, -1).transpose(1, 2) @ _bf64(w).T
    return out if bias is None else out + bias.double()


# relative perturbation of the per-channel scale rstd * gamma under which an element of Wb may legitimately round the other way: the kernel's
# statistics come from fp32-rounded partial sums (2^-24 relative each), var = E[x^2] - mean^2 amplifies that by 1 + 2 (mean / sigma)^2 <= 3
# for the fold cases (|mean| <= sigma), rstd takes half of var's error, and rstd and rstd * gamma are rounded to fp32 once each:
# 1.5 * 2^-24 + 2 * 2^-24 < 2^-22; one more binade of margin
WB_SCALE_SLACK = 2.0 ** -21


def fold_model(x, groups, gamma, beta, eps, w, bias):
    """-> dict: wb [B, N, C] (bf16 values), wb_lo / wb_hi (the same with the scale moved by -+ WB_SCALE_SLACK: where they differ from each other
    the rounding of that element is not decided by the declared arithmetic), rowadd [B, N] and its scale sum|terms| [B, N] (fp64 from the
    rounded wb, as the kernel forms it), y [B, HW, N] = x wb^T + rowadd (fp64 arithmetic on the rounded matrices)"""
    xx = _bf64(x)
    B, C = xx.shape[:2]
    mean, var = _gn_stats(xx, groups)
    rstd32 = _f32((var + _eps64(eps)).rsqrt())
    sa = (_per_channel(rstd32, C)[..., 0] * _f32(gamma)[None, :])                     # [B, C] fp32
    mu = _per_channel(mean, C)[..., 0]                                                # [B, C], exact: rowadd is judged against fp64
    w32 = _f32(_bf64(w))

    def rounded(scale):
        return (w32[None] * scale[:, None, :]).to(torch.bfloat16).double()            # fp32 product, one rounding to bf16

    wb = rounded(sa)
    wb_lo, wb_hi = rounded(sa * (1.0 - WB_SCALE_SLACK)), rounded(sa * (1.0 + WB_SCALE_SLACK))
    wbeta = w32.double() * beta.double()[None, :]                                     # [N, C]
    wmu = wb * mu[:, None, :]                                                         # [B, N, C]
    b64 = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()
    rowadd = b64[None] + wbeta.sum(-1)[None] - wmu.sum(-1)
    scale = b64.abs()[None] + wbeta.abs().sum(-1)[None] + wmu.abs().sum(-1)
    y = xx.reshape(B, C, -1).transpose(1, 2) @ wb.transpose(1, 2) + rowadd[:, None, :]
    return {"wb": wb, "wb_lo": wb_lo, "wb_hi": wb_hi, "rowadd": rowadd, "rowadd_scale": scale, "y": y}


# 16 products summed in a lane (two 8-channel vectors), 6 shuffle levels, the three-term final sum, and the fp32 roundings of the scale and
# the mean inside every product: under 27 roundings of 2^-24 relative to sum|terms| in the worst case = 1.6e-6; an element of Wb that rounds
# the other way (a share below 1e-3 of them, each off by 2^-8 of itself) adds under 4e-6 * share: together below 2^-18
ROWADD_TOL = 2.0 ** -18


def partials(x_nhwc, bm):
    """[B, HW, Cs] (bf16 values) -> [B, HW // bm, Cs, 2] fp32: (sum, sum of squares) per tile of bm pixels; a ragged last tile is left out"""
    x = x_nhwc.double()
    B, HW, Cs = x.shape
    nt = HW // bm
    t = x[:, :nt * bm].reshape(B, nt, bm, Cs)
    return torch.stack([t.sum(2), t.pow(2).sum(2)], -1).to(torch.float32).contiguous()


def nhwc(x):
    """[B, C, ...] -> [B, HW, C] of the bf16-rounded values (fp64)"""
    x = _bf64(x)
    return x.reshape(x.shape[0], x.shape[1], -1).transpose(1, 2).contiguous()


# --------------------------------------------------------------------------------------------------------------------------------
# the measure
# --------------------------------------------------------------------------------------------------------------------------------
def gn_slabs(t, groups):
    """[B, C, ...] -> [B, G, cpg * HW]"""
    return t.detach().double().cpu().reshape(t.shape[0], groups, -1)


def ln_slabs(t):
    """[..., C] -> [rows, C]"""
    return t.detach().double().cpu().reshape(-1, t.shape[-1])


def fold_slabs(t):
    """[B, HW, N] -> [B, ceil(N / 16), HW * 16]; a ragged last block is padded with zeros in every operand alike, which changes neither measure"""
    t = t.detach().double().cpu()
    B, HW, N = t.shape
    t = F.pad(t, (0, (-N) % 16))
    return t.reshape(B, HW, -1, 16).permute(0, 2, 1, 3).reshape(B, -1, HW * 16)


def slab_errors(got, want, model=None):
    """slab-major operands [..., L] -> (max-measure [...], rms-measure [...]).  A slab that is identically zero in the reference has no scale:
    there `got` must equal `model` exactly, and both measures are 0."""
    g, w = got.double(), want.double()
    e = g - w
    top, rms = w.abs().amax(-1), w.pow(2).mean(-1).sqrt()
    zero = top == 0
    if bool(zero.any()):
        assert model is not None, "a reference slab is identically zero and no model was given to compare it with"
        assert torch.equal(g[zero], model.double()[zero]), "a slab that is identically zero in the reference differs from the model"
    one = torch.ones_like(top)
    mx = e.abs().amax(-1) / torch.where(zero, one, top)
    rm = e.pow(2).mean(-1).sqrt() / torch.where(zero, one, rms)
    return torch.where(zero, torch.zeros_like(mx), mx), torch.where(zero, torch.zeros_like(rm), rm)


def model_bounds(model_o, want_o):
    """(E_model, E_rms): the worst slab of the rounding model against the exact reference; refuses a case that proves too little"""
    mx, rms = slab_errors(model_o, want_o, model_o)
    e_model, e_rms = float(mx.max()), float(rms.max())
    assert MODEL_FACTOR * e_model <= MODEL_CEILING and MODEL_FACTOR * e_rms <= MODEL_CEILING, (e_model, e_rms)
    return e_model, e_rms
