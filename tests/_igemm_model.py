"""What the implicit-GEMM tests compare csrc/igemm.hip with, on the CPU in fp64 (no test in here), and the case lists that
tests/test_igemm_ops_gpu.py and tests/test_igemm_model_cpu.py share.

`igemm_fp64(c)`   the operation itself on the bf16-rounded inputs, written without the kernel's index arithmetic: `torch.cat` of the sources,
                  `F.interpolate` (nearest 2x), `F.pad(x, (0, 1, 0, 1))` + a pad-0 stride-2 conv for the asymmetric form, `F.conv2d`, the
                  shortcut as `conv3x3(cat(src0, src1)) + conv1x1(cat(sc0, sc1))`, the LayerNorm consumer as `layer_norm(x) @ W^T`.
                  Epilogue order: alpha * acc, the LayerNorm fold, bias, (GEGLU: value * gelu(gate)), rowadd, residual, activation.
                  Exact erf and exp; act 2 is x * sigmoid(1.702 x).
`igemm_model(c)`  the same with the roundings the kernels declare and nothing else: one rounding of the output to bf16 (none for fp32 output;
                  the GEGLU product is that one rounding); the LayerNorm consumer from the folded operands (W' = bf16(W gamma), cs = column
                  sums of W', b' = b + W beta) with mean and rstd in fp32 from the fp32 partial sums as `ln_row_stats` forms them
                  (mu = S invC, var = max(Q invC - mu^2, 0)); the fused slab-sum + GroupNorm pass: the activation rounded to bf16, then
                  `_norm_model.groupnorm_model` of it.

Bounds.
  fp32 output   |got - fp64| <= (K + 8) 2^-24 (|alpha| sum_k |a_k w_k| + sum |epilogue terms|) per element (behind an activation: ACT_LIPSCHITZ x
                that + ACT_APPROX |pre-activation|, see there).  Derivation: the products of two
                bf16 values are exact in fp32; an fp32 sum of n terms in ANY order (MFMA blocks, K slices, slab sums) is off by at most
                (n - 1) u sum |terms| (1 + O(n u)) with u = 2^-24; the alpha product, the up to three epilogue additions and the final
                rounding add one u each against a partial sum that sum |terms| bounds: K - 1 + 5 < K + 8.  It needs no measurement.
  bf16 output   every slab of 16 rows (one MFMA row tile) x one lane group's column run on its own, `SLAB_COLS` by tile width: max |error| over
                the slab's max |value| and RMS error over the slab's RMS, each at most MODEL_FACTOR x the model's own distance from fp64
                on the worst slab; a case whose bound exceeds MODEL_CEILING is refused (tests/test_igemm_model_cpu.py).
  statistics    `rowstat` / `colstat` tables against fp64 sums of the bf16 values the same launch returned: |table - sum| <= depth 2^-24
                sum |terms| (one more for the squares), depth = the longest chain of additions in igemm_epilogue.h's reduction,
                `rowstat_depth` / `colstat_depth`, per family and tile.
Inputs: every image, source and 64-channel block has its own scale and offset; bias, rowadd and residual are non-constant and of the GEMM term's
magnitude, so a term taken from the wrong image or row, or dropped, moves the output by far more than a bound; residual cases satisfy
`residual_condition` (the increment at least as large, RMS, as the residual)."""
import math
import zlib

import torch
import torch.nn.functional as F
from _norm_model import groupnorm_model, slab_errors  # (reused, not copied)
from _tblock_model import MODEL_CEILING, MODEL_FACTOR, bfr, residual_condition  # noqa: F401

U = 2.0 ** -24
LN_EPS = 1e-5
GN_EPS = 1e-5
# columns of one lane's channel run (4 NI accumulator columns, igemm_epilogue.h `CA`) by tile width BN: 64-wide tiles on 2 column waves hold
# 32 columns per wave = 8 per lane group; 128-wide 16; 160-wide 20; the 8-phase 256-wide tile 16; the whole-images 8 x 8 kernel's 64-wide tile 16
SLAB_COLS = {64: 8, 128: 16, 160: 20, 256: 16, "smap": 16}


def _waves(c):
    """(row waves WM, column waves WN) of the tile a case runs on: the general, row-halo and pc kernels 2 x 2 (igemm.hip launch_cfg, igemm_pc.h
    PcGeom); the weight-streaming kernel one row wave and one column wave per 32 columns (igemm_wreg.h); the 8-phase kernel 2 x 4 on its
    256-wide tile and 4 x 2 on its 160-wide one (igemm.hip launch_8p)"""
    bn = c["cfg"][1]
    if c["family"] == "wreg":
        return 1, bn // 32
    if c["family"] == "8p":
        return (2, 4) if bn == 256 else (4, 2)
    return 2, 2


def rowstat_depth(c):
    """the longest chain of additions behind one `rowstat_out` entry (igemm_epilogue.h): a lane adds the BN / WN / 4 bf16-rounded values of its
    channel run one by one, two shuffle levels join the four lanes of a pixel row, the tile's WN column waves are added in sequence.
    64 x 64 tiles: 8 + 2 + 2 = 12; 128-wide 20; 160-wide 24; the weight-streaming kernel's 128-wide tile 8 + 2 + 4 = 14"""
    wm, wn = _waves(c)
    return c["cfg"][1] // wn // 4 + 2 + wn


def colstat_depth(c):
    """the longest chain behind one `colstat_out` entry: lane = column adds the BM / WM rows of its wave tile one by one, then the tile's WM row
    waves in sequence.  64-row tiles on 2 row waves: 32 + 2 = 34; 128-row tiles 66; the weight-streaming kernel 64 + 1 = 65; the 8-phase
    kernel's 256-wide tile 128 + 2 = 130"""
    wm, wn = _waves(c)
    return c["cfg"][0] // wm + wm


# fp32 output behind an activation.  The largest slope of x sigmoid(x) is 1.0998, of x sigmoid(1.702 x) 1.0998, of gelu 1.1290: 1.13.  The kernels'
# own activations (common.h): silu / quick gelu = x / (1 + __expf(-a x)) -- an exp of 2 ulp and a division of 1 ulp move the result by at most
# |x| (2 ulp / 4 + 1 ulp) < 2^-22 |x|; gelu through Abramowitz-Stegun 7.1.26 (|erf error| <= 1.5e-7, so 0.75e-7 |x| = 2^-23.7 |x|) with a
# hardware reciprocal and exp2 of about 1 ulp each on the tail term (< 2^-23 |x|).  All under 2^-21 |x|.  The ulp figures of __expf, the
# division and the hardware reciprocal / exp2 are ASSUMED from their documented accuracy classes; nobody measured them for this bound.  It
# judges the extra "... fp32" activation cases only -- every other fp32 case stands under the plain sum bound.
ACT_LIPSCHITZ = 1.13
ACT_APPROX = 2.0 ** -21


def _f32(t):
    return t.to(torch.float32)


def _r(t):
    """fp64 -> fp32 (the accumulator) -> bf16"""
    return _f32(t).to(torch.bfloat16).double()


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % (2 ** 31))


# --------------------------------------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(images=1, H=1, W=64, C0=64, C1=0, ksize=1, stride=1, up=1, asym=False, sc=None, N=64, geglu=False, bias_mode=1, rowadd=False,
                residual=False, ldr_extra=0, ldo_extra=0, alpha=1.0, act=0, out_f32=True, ln=None, rowstat=0, colstat=False, gn=None, wpi=False,
                batched=None, flags=None, seed=None)


def case(name, family, slab="none", cfg=None, **kw):
    """family / slab: what the launcher must report for this case (ops.IGEMM_FAMILY / IGEMM_SLAB names); cfg: (BM, BN, K splits)"""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    c = dict(DEFAULTS)
    c.update(kw)
    c.update(name=name, family=family, slab=slab, cfg=cfg, flags=dict(kw.get("flags") or {}))
    return c


def out_hw(c):
    if c["asym"]:
        return c["H"] // 2, c["W"] // 2
    pad = 1 if c["ksize"] == 3 else 0
    return ((c["H"] * c["up"] + 2 * pad - c["ksize"]) // c["stride"] + 1, (c["W"] * c["up"] + 2 * pad - c["ksize"]) // c["stride"] + 1)


def dims(c):
    """-> (M, N, Nout, K, HWo)"""
    ho, wo = out_hw(c)
    sc = sum(c["sc"]) if c["sc"] else 0
    K = c["ksize"] ** 2 * (c["C0"] + c["C1"]) + sc
    return c["images"] * ho * wo, c["N"], (c["N"] // 2 if c["geglu"] else c["N"]), K, ho * wo


_INPUTS = {}


def _source(g, images, h, w, C, which):
    """[images, h, w, C] bf16 values: image i of source `which` has its own scale 2^-1 .. 2^1 and offset, every 64-channel block its own offset"""
    z = torch.randn(images, h, w, C, generator=g)
    i = torch.arange(images)
    scale = 2.0 ** (((i + which) % 3) - 1.0)
    off = 0.25 * (1 + i % 4) * (1.0 - 2.0 * ((i + which) % 2))
    blk = 0.125 * ((torch.arange(C) // 64) % 5).float() * (1.0 - 2.0 * which)
    return bfr((z * scale[:, None, None, None] + off[:, None, None, None] + blk) * (1.5 if which else 1.0))


def inputs(c):
    """-> dict of CPU fp32 tensors (bf16-rounded where the launch rounds them); cached per case name"""
    if c["name"] in _INPUTS:
        return _INPUTS[c["name"]]
    g = gen(c["seed"] or c["name"])          # cases that state one problem two ways share a seed
    M, N, Nout, K, HWo = dims(c)
    ho, wo = out_hw(c)
    C = c["C0"] + c["C1"]
    if c["batched"]:
        _INPUTS[c["name"]] = i = _batched_inputs(c, g)
        return i
    i = {"x0": _source(g, c["images"], c["H"], c["W"], c["C0"], 0)}
    if c["C1"]:
        i["x1"] = _source(g, c["images"], c["H"], c["W"], c["C1"], 1)
    if c["sc"]:
        i["s0"] = _source(g, c["images"], ho, wo, c["sc"][0], 0) * 0.5
        if c["sc"][1]:
            i["s1"] = _source(g, c["images"], ho, wo, c["sc"][1], 1) * 0.5
        i["wsc"] = bfr(torch.randn(N, sum(c["sc"]), generator=g) / math.sqrt(sum(c["sc"])))
    nmat = c["images"] if c["wpi"] else 1
    i["w4"] = bfr(torch.randn(nmat, N, C, c["ksize"], c["ksize"], generator=g) * (1.0 + torch.arange(nmat).float())[:, None, None, None, None] / math.sqrt(K))
    if c["bias_mode"]:
        i["bias"] = torch.randn(N if c["bias_mode"] == 1 else M, generator=g)
    if c["rowadd"]:
        i["rowadd"] = torch.randn(c["images"], N, generator=g) * 1.5
    if c["residual"]:
        ldr = Nout + c["ldr_extra"]
        res = torch.full((M, ldr), 1000.0)          # the pad columns: a read outside [0, Nout) of a row is visible
        res[:, :Nout] = torch.randn(M, Nout, generator=g) * 0.5
        i["res"] = bfr(res)
    if c["ln"]:
        # rows with their own scale and mean: |mean| <= 2 sigma, or the deliberate offset (mean = ratio x sigma, sign alternating)
        ln = c["ln"]
        z = torch.randn(M, C, generator=g)
        sig = 2.0 ** torch.randint(-1, 2, (M, 1), generator=g).float()
        if ln.get("mean") is not None:
            mu, sig = torch.full((M, 1), float(ln["mean"])) * (1 - 2 * (torch.arange(M)[:, None] % 2)), torch.full((M, 1), float(ln["std"]))
            i["x0"] = bfr(z * sig + mu).reshape(c["images"], c["H"], c["W"], C)
        else:
            i["x0"] = bfr((z + torch.randn(M, 1, generator=g).clamp(-2, 2) * 0.5) * sig).reshape(c["images"], c["H"], c["W"], C)
        i["gamma"], i["beta"] = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.2 + 0.1
    if c["gn"]:
        i["gn_gamma"], i["gn_beta"] = torch.randn(N, generator=g) * 0.2 + 1.0, torch.randn(N, generator=g) * 0.2 + 0.1
    _INPUTS[c["name"]] = i
    return i


def _batched_inputs(c, g):
    """the VAE attention's launches: batch row b multiplies A[b] (or the one shared A) [M, K] with its own matrix [N, K]"""
    M, N, Nout, K, HWo = dims(c)
    B = c["batched"]["B"]
    nA = 1 if c["batched"].get("shared_a") else B
    b = torch.arange(B).float()
    i = {"x0": bfr(torch.randn(nA, 1, 1, M, K, generator=g) * (1.0 + torch.arange(nA).float())[:, None, None, None, None] + 0.25),
         "w4": bfr((torch.randn(B, N, K, 1, 1, generator=g) * (1.0 + b)[:, None, None, None, None] + 0.1 * (b - 1)[:, None, None, None, None]) / math.sqrt(K))}
    if c["bias_mode"]:
        i["bias"] = torch.randn(N if c["bias_mode"] == 1 else M, generator=g)
    return i


def kernel_matrix(c, i):
    """[matrices, N, K] in the kernel's K order: k = tap * (C0 + C1) + channel, then the shortcut's columns"""
    w = i["w4"].permute(0, 1, 3, 4, 2).reshape(i["w4"].shape[0], c["N"], -1)
    if c["sc"]:
        w = torch.cat([w, i["wsc"][None]], 2)
    return w.contiguous()


# --------------------------------------------------------------------------------------------------------------------------------
# the operation
# --------------------------------------------------------------------------------------------------------------------------------
def _gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))


def _act64(t, act):
    if act == 1:
        return t * torch.sigmoid(t)
    if act == 2:
        return t * torch.sigmoid(1.702 * t)
    if act == 3:
        return _gelu64(t)
    return t


def _conv(c, x, w4, sc_x, wsc):
    """x [images, H, W, C] and w4 [N, C, k, k] (any dtype) -> [M, N]: the gather forms through torch's own ops"""
    t = x.permute(0, 3, 1, 2)
    if c["up"] == 2:
        t = F.interpolate(t, scale_factor=2, mode="nearest")
    if c["asym"]:
        y = F.conv2d(F.pad(t, (0, 1, 0, 1)), w4, stride=2)
    else:
        y = F.conv2d(t, w4, stride=c["stride"], padding=1 if c["ksize"] == 3 else 0)
    y = y.permute(0, 2, 3, 1).reshape(-1, w4.shape[0])
    if sc_x is not None:
        y = y + sc_x.reshape(-1, sc_x.shape[-1]) @ wsc.T
    return y


def _sources(c, i, mutate=None):
    xs = [i["x0"]] + ([i["x1"]] if c["C1"] else [])
    if mutate == "swap_sources" and c["C1"]:
        assert c["C0"] == c["C1"], "the swap mutation needs sources of one width"
        xs = xs[::-1]
    x = torch.cat(xs, -1)
    if mutate == "drop_chunk":
        x = x.clone()
        x[..., -64:] = 0
    sc = None
    if c["sc"]:
        sc = torch.cat([i["s0"]] + ([i["s1"]] if c["sc"][1] else []), -1)
    return x, sc


def _acc(c, i, dtype, absolute=False, mutate=None):
    """the GEMM term alone, [M, N]; absolute: sum_k |a_k w_k|"""
    f = (lambda t: t.abs().to(dtype)) if absolute else (lambda t: t.to(dtype))
    if c["batched"]:
        B, x, w = c["batched"]["B"], i["x0"], i["w4"]
        return torch.cat([f(x[b % x.shape[0]].reshape(-1, x.shape[-1])) @ f(w[b].reshape(w.shape[1], -1)).T for b in range(B)], 0)
    x, sc = _sources(c, i, mutate)
    wsc = f(i["wsc"]) if c["sc"] else None
    if c["wpi"]:
        ys = [_conv(c, f(x[k:k + 1]), f(i["w4"][k]), None, None) for k in range(c["images"])]
        return torch.cat(ys, 0)
    w4 = f(i["w4"][0])
    if mutate == "skip_slab" and c["cfg"] and c["cfg"][2] > 1:
        # K slices are whole 64-channel steps of the tap-major walk: the last slice = the last taps' trailing channels; drop the last tap's last chunk range
        w4 = w4.clone()
        per = (dims(c)[3] // 64 + c["cfg"][2] - 1) // c["cfg"][2] * 64
        flat = w4.permute(0, 2, 3, 1).reshape(w4.shape[0], -1)
        flat[:, -min(per, flat.shape[1]):] = 0
        w4 = flat.reshape(w4.shape[0], c["ksize"], c["ksize"], -1).permute(0, 3, 1, 2)
    return _conv(c, f(x), w4, None if sc is None else f(sc), wsc)


def ln_fold(c, i):
    """the folded operands as launch_ln_fold_weight states them: W' = bf16(W gamma) (fp32 product, one rounding), cs = column sums of W',
    b' = b + W beta -> (W' [N, C] fp64, cs fp32 [N], b' fp32 [N])"""
    w = _f32(i["w4"][0].reshape(c["N"], -1))
    wf = (w * _f32(i["gamma"])[None, :]).to(torch.bfloat16).double()
    bf = (i["bias"].double() if c["bias_mode"] else torch.zeros(c["N"], dtype=torch.float64)) + w.double() @ i["beta"].double()
    return wf, _f32(wf.sum(1)), _f32(bf)


def ln_table(c, i):
    """the producer's table made on the host: [M, slots, 2] fp32 = (sum, sum of squares) of each of `slots` column ranges of a row"""
    x = i["x0"].double().reshape(dims(c)[0], -1)
    parts = torch.tensor_split(x, c["ln"]["slots"], dim=1)
    return torch.stack([torch.stack([p.sum(1), p.pow(2).sum(1)], -1) for p in parts], 1).to(torch.float32).contiguous()


def _pre(c, i, model, mutate=None):
    """alpha * acc, LayerNorm fold, bias: -> [M, N] fp64"""
    M, N, Nout, K, HWo = dims(c)
    if c["ln"]:
        x = i["x0"].double().reshape(M, -1)
        if model:
            wf, cs, bf = ln_fold(c, i)
            t = ln_table(c, i)
            S, Q = t[:, 0, 0].clone(), t[:, 0, 1].clone()
            for k in range(1, t.shape[1]):                      # fp32, slot order
                S, Q = S + t[:, k, 0], Q + t[:, k, 1]
            invC = torch.tensor(1.0 / x.shape[1], dtype=torch.float32)
            mu = S * invC
            var = (Q * invC - mu * mu).clamp_min(0)
            rstd = 1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=torch.float32))
            v = rstd.double()[:, None] * (x @ wf.T - mu.double()[:, None] * cs.double()[None, :]) + bf.double()[None, :]
        else:
            y = F.layer_norm(x, (x.shape[1],), i["gamma"].double(), i["beta"].double(), float(torch.tensor(LN_EPS, dtype=torch.float32)))
            v = y @ i["w4"][0].reshape(N, -1).double().T
            if c["bias_mode"]:
                v = v + i["bias"].double()[None, :]
        return v
    alpha = float(torch.tensor(c["alpha"], dtype=torch.float32))
    v = alpha * _acc(c, i, torch.float64, mutate=mutate)
    if c["bias_mode"] == 1:
        v = v + i["bias"].double()[None, :]
    elif c["bias_mode"] == 2 and mutate == "bias_n_for_mode2":
        v = v + i["bias"].double()[torch.arange(N) % M][None, :]
    elif c["bias_mode"] == 2:
        v = v + i["bias"].double().repeat(v.shape[0] // M)[:, None]
    return v


def _epilogue(c, i, v, mutate=None):
    M, N, Nout, K, HWo = dims(c)
    if c["geglu"]:
        v = v[:, :Nout] * _gelu64(v[:, Nout:])
    if mutate == "act_before_residual":
        v = _act64(v, c["act"])
    if c["rowadd"]:
        img = torch.arange(M) // HWo
        if mutate == "rowadd_next_image":
            img = (img + 1) % c["images"]
        v = v + i["rowadd"].double()[img][:, :Nout]
    if c["residual"]:
        v = v + i["res"].double()[:, :Nout]
    return v if mutate == "act_before_residual" else _act64(v, c["act"])


def igemm_fp64(c, mutate=None):
    i = inputs(c)
    return _epilogue(c, i, _pre(c, i, False, mutate), mutate)


def igemm_model(c, mutate=None):
    i = inputs(c)
    v = _epilogue(c, i, _pre(c, i, True, mutate), mutate)
    return v if c["out_f32"] else _r(v)


def f32_bound(c):
    """(K + 8) 2^-24 (|alpha| sum |a w| + sum |epilogue terms|), [M, N].  The sum of |products| is formed in fp32 to keep the CPU cost down; the
    factor 1 + 2^-10 covers what that fp32 sum itself may lose (K 2^-24 <= 2^-11 for K <= 8192), so the bound is never below the stated one"""
    i = inputs(c)
    M, N, Nout, K, HWo = dims(c)
    assert not c["geglu"] and not c["ln"], "the fp32 bound is stated for the plain epilogue forms"
    s = abs(c["alpha"]) * _acc(c, i, torch.float32, absolute=True).double() * (1.0 + 2.0 ** -10)
    if c["bias_mode"] == 1:
        s = s + i["bias"].double().abs()[None, :]
    elif c["bias_mode"] == 2:
        s = s + i["bias"].double().abs().repeat(s.shape[0] // M)[:, None]
    if c["rowadd"]:
        s = s + i["rowadd"].double().abs()[torch.arange(M) // HWo]
    if c["residual"]:
        s = s + i["res"].double().abs()[:, :Nout]
    bound = (K + 8) * U * s
    if c["act"]:
        # behind an activation: f(pre + e) - f(pre) <= ACT_LIPSCHITZ |e|, plus what the kernel's own f costs (ACT_APPROX |pre|)
        pre = _epilogue(dict(c, act=0), i, _pre(c, i, False))
        bound = ACT_LIPSCHITZ * bound + ACT_APPROX * pre.abs()
    return bound


def gn_model(c, act_bf16):
    """the fused slab pass's second output: GroupNorm(+SiLU) of the ROUNDED activation [M, N] (bf16 values) -> [M, N]"""
    i = inputs(c)
    M, N, Nout, K, HWo = dims(c)
    gn = c["gn"]
    x = act_bf16.double().reshape(c["images"], HWo, N).transpose(1, 2)
    return groupnorm_model(x, None, gn["groups"], i["gn_gamma"], i["gn_beta"], GN_EPS, bool(gn.get("silu"))).transpose(1, 2).reshape(M, N)


# --------------------------------------------------------------------------------------------------------------------------------
# the measure
# --------------------------------------------------------------------------------------------------------------------------------
def slab_cols(c):
    if c["family"] == "smap":
        return SLAB_COLS["smap"]
    return SLAB_COLS[c["cfg"][1]]


def slabs(t, cols, rows=16):
    """[M, N] -> [ceil(M / 16), ceil(N / cols), 16 * cols]; ragged edges are padded with zeros in every operand alike, which changes neither measure"""
    t = t.detach().double().cpu()
    M, N = t.shape
    t = F.pad(t, (0, (-N) % cols, 0, (-M) % rows))
    return t.reshape(-1, rows, t.shape[1] // cols, cols).permute(0, 2, 1, 3).reshape(-1, t.shape[1] // cols, rows * cols)


_REFS = {}


def reference(c):
    """-> dict: want (fp64), model, and for fp32 output `bound` [M, N], for bf16 output (e_model, e_rms) of the worst slab; cached per case"""
    if c["name"] in _REFS:
        return _REFS[c["name"]]
    want, model = igemm_fp64(c), igemm_model(c)
    r = {"want": want, "model": model}
    if c["out_f32"]:
        r["bound"] = f32_bound(c)
    else:
        w = slab_cols(c)
        mx, rms = slab_errors(slabs(model, w), slabs(want, w), slabs(model, w))
        r["e_model"], r["e_rms"] = float(mx.max()), float(rms.max())
    _REFS[c["name"]] = r
    return r


def check_case_conditions(c):
    """what every case must satisfy before a kernel is judged on it (tests/test_igemm_model_cpu.py)"""
    r = reference(c)
    i = inputs(c)
    if not c["out_f32"]:
        assert 0 < MODEL_FACTOR * r["e_model"] <= MODEL_CEILING and 0 < MODEL_FACTOR * r["e_rms"] <= MODEL_CEILING, (c["name"], r["e_model"], r["e_rms"])
    else:
        assert float((r["bound"] / r["want"].abs().clamp_min(1e-30)).median()) < MODEL_CEILING, c["name"]      # the bound is small against the values
    if c["residual"]:
        assert residual_condition(r["want"], i["res"][:, :r["want"].shape[1]]) >= 1.0, c["name"]
    if c["ln"]:
        x = i["x0"].double().reshape(dims(c)[0], -1)
        ratio = float((x.mean(1).abs() / x.std(1)).max())
        assert (ratio > 2.0) == bool(c["ln"].get("offset")), (c["name"], ratio)


def errors(c, got, want=None, model=None, bound=None):
    """the measured figures of one output [M, Nout] -> dict; `violations` lists which bound it breaks (empty: inside)"""
    r = reference(c) if want is None else {"want": want, "model": model, "bound": bound}
    got = got.detach().double().cpu()
    out = {"violations": []}
    if not bool(torch.isfinite(got).all()):
        out["violations"].append("not finite")
    if c["out_f32"]:
        ratio = ((got - r["want"]).abs() / r["bound"].clamp_min(1e-300))
        out["worst_over_bound"] = float(ratio.max())
        if out["worst_over_bound"] > 1.0:
            out["violations"].append("fp32 bound")
    else:
        w = slab_cols(c)
        e_model, e_rms = (r["e_model"], r["e_rms"]) if want is None else tuple(float(v.max()) for v in slab_errors(slabs(model, w), slabs(want, w), slabs(model, w)))
        mx, rms = slab_errors(slabs(got, w), slabs(r["want"], w), slabs(r["model"], w))
        out.update(kernel_max=float(mx.max()), model_max=e_model, kernel_rms=float(rms.max()), model_rms=e_rms)
        if out["kernel_max"] > MODEL_FACTOR * e_model:
            out["violations"].append("slab max")
        if out["kernel_rms"] > MODEL_FACTOR * e_rms:
            out["violations"].append("slab rms")
    return out


def sums_errors(table, values, dim, depth):
    """table [..., 2] against fp64 sums of `values` (bf16 values the launch itself returned) along dim -> (worst sum error, worst
    sum-of-squares error) relative to their bounds depth 2^-24 sum |terms| (the squares: depth + 1); <= 1 is inside"""
    v, t = values.double().cpu(), table.double().cpu()
    out = []
    for k, vv in enumerate((v, v * v)):
        scale = vv.abs().sum(dim)
        err = (t[..., k] - vv.sum(dim)).abs()
        ok = scale > 0
        assert bool((err[~ok] == 0).all()), "a table entry over all-zero values is not zero"
        out.append(float((err[ok] / ((depth + k) * U * scale[ok])).max()) if bool(ok.any()) else 0.0)
    return tuple(out)


# --------------------------------------------------------------------------------------------------------------------------------
# the launch as tests/test_igemm_ops_gpu.py states it (CPU tensors; the test moves them to the GPU)
# --------------------------------------------------------------------------------------------------------------------------------
def launch_args(c):
    """-> (tensors, keywords) of agenda_amd.ops.igemm"""
    i = inputs(c)
    M, N, Nout, K, HWo = dims(c)
    w = kernel_matrix(c, i)
    assert w.shape[-1] == K
    t = {"src0": i["x0"], "w": w if c["wpi"] else w[0], "src1": i.get("x1"), "sc0": i.get("s0"), "sc1": i.get("s1"), "bias": i.get("bias"),
         "rowadd": i.get("rowadd"), "residual": i.get("res")}
    ho, wo = out_hw(c)
    kw = dict(ksize=c["ksize"], stride=c["stride"], up=c["up"], alpha=c["alpha"], geglu=c["geglu"], act=c["act"], out_f32=c["out_f32"],
              ldo=Nout + c["ldo_extra"], w_per_image=c["wpi"], bias_mode=c["bias_mode"])
    if c["asym"]:
        kw.update(stride=2, pad=0, hout=ho, wout=wo)        # as the VAE encoder's downsampling convs state it
    if c["ln"]:
        wf, cs, bf = ln_fold(c, i)
        t.update(w=wf.float(), bias=bf, ln_stats=ln_table(c, i), ln_cs=cs)
        kw.update(ln_invC=1.0 / (c["C0"] + c["C1"]), ln_eps=LN_EPS, bias_mode=1)
    if c["gn"]:
        t.update(gn_gamma=i["gn_gamma"], gn_beta=i["gn_beta"])
    if c["batched"]:
        B = c["batched"]["B"]
        t["w"] = w
        kw.update(batch=B, strides=(0 if c["batched"].get("shared_a") else M * K, 0, N * K, M * (Nout + c["ldo_extra"]), 0))
    kw.update(c["flags"])
    return t, kw


# --------------------------------------------------------------------------------------------------------------------------------
# the cases both test files walk.  family / slab / cfg = (BM, BN, K splits) are what launch_igemm's shape rules give (restated by hand in
# tests/test_igemm_model_cpu.py); shapes are the smallest that reach the route.
# --------------------------------------------------------------------------------------------------------------------------------
HALO = {"halo": 1}
# 12288 output rows x 160 columns = 96 x 2 tiles of 128 x 128: the fewest tiles (192) at which a 3x3 launch of K = 576 takes 128-row tiles
BIG = dict(N=160, ksize=3)

GATHER = [
    # general kernel, 64 x 64 tiles: every gather form, concat with C0 != C1 both ways, non-square maps, ragged M, 1 / 2 / 3 / 8 images
    case("g64 1x1 cat 64|128", "general", cfg=(64, 64, 1), images=2, H=8, W=12, C0=64, C1=128, N=96),
    case("g64 1x1 cat 192|64", "general", cfg=(64, 64, 1), images=2, H=8, W=12, C0=192, C1=64, N=96),
    case("g64 3x3 cat 64|128", "general", cfg=(64, 64, 1), images=3, H=6, W=10, C0=64, C1=128, N=72, ksize=3),
    case("g64 3x3 stride 2 cat 192|64", "general", cfg=(64, 64, 1), images=3, H=9, W=12, C0=192, C1=64, N=64, ksize=3, stride=2),
    case("g64 3x3 up 2 cat 64|128", "general", cfg=(64, 64, 1), H=5, W=7, C0=64, C1=128, N=72, ksize=3, up=2),
    case("g64 asymmetric even", "general", cfg=(64, 64, 1), images=2, H=8, W=12, C0=128, N=64, ksize=3, asym=True),
    case("g64 asymmetric odd", "general", cfg=(64, 64, 1), images=2, H=9, W=11, C0=64, C1=64, N=64, ksize=3, asym=True),
    case("g64 3x3 eight images", "general", cfg=(64, 64, 1), images=8, H=4, W=4, C0=64, N=64, ksize=3),
    # general kernel, the wider tiles (1x1: the cheapest K)
    case("g128x128 two stages cat", "general", cfg=(128, 128, 1), images=3, H=32, W=32, C0=64, C1=64, N=1024),
    case("g128x128 four stages cat", "general", cfg=(128, 128, 1), images=3, H=32, W=32, C0=192, C1=320, N=1024),
    case("g128x160 two stages", "general", cfg=(128, 160, 1), images=3, H=64, W=64, C0=64, N=160),
    case("g64x160 deep ring cat", "general", cfg=(64, 160, 1), images=3, H=64, W=64, C0=256, C1=256, N=160),
    case("g64x160 3x3 without halo", "general", cfg=(64, 160, 1), images=3, H=128, W=32, C0=64, **BIG),
    # row-halo kernel: every tile-row geometry (Wout 16 .. 256), H != W, concat, up = 2
    case("halo Wout 16", "halo", cfg=(128, 160, 1), images=3, H=256, W=16, C0=64, flags=HALO, **BIG),
    case("halo Wout 32 cat 64|128", "halo", cfg=(128, 160, 1), images=3, H=128, W=32, C0=64, C1=128, flags=HALO, **BIG),
    case("halo Wout 64", "halo", cfg=(128, 160, 1), H=192, W=64, C0=64, flags=HALO, **BIG),
    case("halo Wout 128", "halo", cfg=(128, 160, 1), H=96, W=128, C0=64, flags=HALO, **BIG),
    case("halo Wout 256", "halo", cfg=(128, 160, 1), H=48, W=256, C0=64, flags=HALO, **BIG),
    case("halo up 2", "halo", cfg=(128, 160, 1), H=48, W=64, C0=64, up=2, flags=HALO, **BIG),
    case("pch Wout 64", "pch", cfg=(128, 160, 1), H=192, W=64, C0=64, flags={"halo": 1, "pc": 16}, **BIG),
    case("pc 3x3 cat 64|64", "pc", cfg=(64, 160, 1), images=2, H=32, W=32, C0=64, C1=64, N=1280, ksize=3, flags={"pc": 2}),
    case("8p 256 wide cat", "8p", cfg=(256, 256, 1), images=2, H=16, W=16, C0=64, C1=64, N=256, ksize=3, flags={"p8": 2}),
    case("8p 160 wide stride 2 cat", "8p", cfg=(256, 160, 1), images=2, H=32, W=32, C0=64, C1=128, N=160, ksize=3, stride=2, flags={"p8": 3}),
    case("smap unsplit", "smap", cfg=(512, 64, 1), images=8, H=8, W=8, C0=64, N=64, ksize=3, flags={"smap": 1}),
    case("smap cat 64|64 split", "smap", "plain", cfg=(512, 64, 2), images=8, H=8, W=8, C0=64, C1=64, N=64, ksize=3, flags={"smap": 1}),
]
# the same total of channels as one source: (concat case, single-source case); the pair shares inputs through `single_of`
CONCAT_PAIRS = ["g64 1x1 cat 192|64", "g64 3x3 cat 64|128", "8p 256 wide cat"]

SHORTCUT = [
    case("sc halo one source", "halo", cfg=(128, 160, 1), images=3, H=128, W=32, C0=64, sc=(64, 0), flags=HALO, **BIG),
    case("sc halo two sources residual rowadd", "halo", cfg=(128, 160, 1), images=3, H=128, W=32, C0=64, sc=(128, 64), residual=True, rowadd=True, flags=HALO, **BIG),
    case("sc halo split", "halo", "plain", cfg=(128, 128, 8), H=8, W=16, C0=512, N=128, ksize=3, sc=(64, 0), flags=HALO),
    case("sc halo split two sources residual rowadd", "halo", "plain", cfg=(128, 128, 8), H=8, W=16, C0=512, N=128, ksize=3, sc=(128, 64), residual=True,
         rowadd=True, out_f32=False, flags=HALO),
    case("sc smap", "smap", cfg=(512, 64, 1), images=8, H=8, W=8, C0=64, N=64, ksize=3, sc=(128, 0), flags={"smap": 1}),
    case("sc smap split two sources residual", "smap", "plain", cfg=(512, 64, 2), images=8, H=8, W=8, C0=128, N=64, ksize=3, sc=(64, 64), residual=True,
         flags={"smap": 1}),
]
# launches the launcher refuses (-1, nothing launched): (case, a word of the message)
SHORTCUT_REFUSED = [
    (case("sc refused: no halo shape", "none", images=2, H=12, W=12, C0=64, N=160, ksize=3, sc=(64, 0), flags=HALO), "shortcut"),
    (case("sc refused: small tile", "none", images=2, H=16, W=16, C0=64, N=64, ksize=3, sc=(64, 0), flags=HALO), "shortcut"),
    (case("sc refused: 32 channels", "none", images=3, H=128, W=32, C0=64, sc=(32, 0), flags=HALO, **BIG), "multiples of 64"),
    (case("sc refused: geglu", "none", images=3, H=128, W=32, C0=64, N=256, ksize=3, sc=(64, 0), geglu=True, flags=HALO), "shortcut"),
]

# one epilogue form at a time, then all compatible ones together
FORMS = {
    "alpha 0.5": dict(alpha=0.5), "alpha rsqrt": dict(alpha=128 ** -0.5), "row bias": dict(bias_mode=2), "no bias": dict(bias_mode=0),
    "rowadd": dict(rowadd=True), "residual": dict(residual=True, ldr_extra=8), "ldo": dict(ldo_extra=8), "bf16": dict(out_f32=False),
    "silu": dict(act=1, out_f32=False), "quick gelu": dict(act=2, out_f32=False), "gelu": dict(act=3, out_f32=False),
    "silu fp32": dict(act=1, rowadd=True), "quick gelu fp32": dict(act=2, residual=True, ldr_extra=8), "gelu fp32": dict(act=3, alpha=0.5),
    "linear forms together": dict(alpha=0.5, rowadd=True, residual=True, ldr_extra=8, ldo_extra=8),
    "all together": dict(alpha=0.5, rowadd=True, residual=True, ldr_extra=8, ldo_extra=8, act=1, out_f32=False),
}


def _element(f):
    """the same form on the element-by-element path: odd pitches"""
    f = dict(f)
    f["ldo_extra"] = 1
    if f.get("residual"):
        f["ldr_extra"] = 1
    return f


# general kernel: images of 48 rows, so that a 64-row tile straddles two images (rowadd); N = 200 on the vector path, N = 72 with odd pitches on
# the element path; the pair of a form shares its inputs where the shapes agree (N = 200 both)
EPILOGUE = []
for _n, _f in FORMS.items():
    EPILOGUE.append(case(f"general vector {_n}", "general", cfg=(64, 64, 1), images=4, W=48, C0=128, N=200, seed=f"ep {_n}", **_f))
    EPILOGUE.append(case(f"general element {_n}", "general", cfg=(64, 64, 1), images=4, W=48, C0=128, N=200, seed=f"ep {_n}", **_element(_f)))
    EPILOGUE.append(case(f"general element N 72 {_n}", "general", cfg=(64, 64, 1), images=4, W=48, C0=128, N=72, **_element(_f)))
EPILOGUE_PAIRS = [(f"general vector {_n}", f"general element {_n}") for _n in FORMS]
_LIN, _ALL = FORMS["linear forms together"], FORMS["all together"]
# the other families: every form one at a time and together on one row-halo launch (160-wide tile: 8-byte vectors), one pc launch, one
# 8-phase launch (vector path only, 128-row wave tiles) and one weight-streaming launch (one row wave; bf16 output is that kernel's only
# one, so its fp32 forms run rounded and the forms named after fp32 are left out); images of 64 rows or more
FAMILY_SHAPES = {
    "halo": dict(family="halo", cfg=(128, 160, 1), images=3, H=128, W=32, C0=64, flags=HALO, **BIG),
    "pc": dict(family="pc", cfg=(64, 160, 1), images=24, H=8, W=8, C0=1024, N=1280, flags={"pc": 1}),
    "8p": dict(family="8p", cfg=(256, 256, 1), images=8, H=8, W=8, C0=128, N=256, flags={"p8": 2}),
    "wreg": dict(family="wreg", cfg=(64, 128, 1), images=16, H=8, W=8, C0=128, N=1024, flags={"wreg": 1}),
}
for _fam, _shape in FAMILY_SHAPES.items():
    for _n, _f in FORMS.items():
        if _fam == "wreg":
            if _n.endswith("fp32"):
                continue
            _f = dict(_f, out_f32=False)
        EPILOGUE.append(case(f"{_fam} {_n}", _shape["family"], cfg=_shape["cfg"], **{k: v for k, v in _shape.items() if k not in ("family", "cfg")}, **_f))
# the plain slab pass behind every kernel that splits K; pitch % 4 != 0 takes its element stores
SLAB = [
    case("slab general linear forms", "general", "plain", cfg=(64, 160, 4), images=8, H=8, W=8, C0=5120, N=1280, **_LIN),
    case("slab general all forms", "general", "plain", cfg=(64, 160, 4), images=8, H=8, W=8, C0=5120, N=1280, **_ALL),
    case("slab general N 320 linear forms", "general", "plain", cfg=(64, 160, 5), images=8, H=8, W=8, C0=5120, N=320, seed="slab 320", **_LIN),
    case("slab general N 320 odd pitch", "general", "plain", cfg=(64, 160, 5), images=8, H=8, W=8, C0=5120, N=320, seed="slab 320", **dict(_LIN, ldo_extra=2, ldr_extra=2)),
    case("slab general N 320 all forms odd pitch", "general", "plain", cfg=(64, 160, 5), images=8, H=8, W=8, C0=5120, N=320, **dict(_ALL, ldo_extra=2, ldr_extra=2)),
    case("slab general N 320 row bias quick gelu", "general", "plain", cfg=(64, 160, 5), images=8, H=8, W=8, C0=5120, N=320, bias_mode=2, act=2, out_f32=False),
    case("slab general N 320 gelu", "general", "plain", cfg=(64, 160, 5), images=8, H=8, W=8, C0=5120, N=320, act=3, out_f32=False),
    case("slab halo all forms", "halo", "plain", cfg=(128, 128, 8), images=2, H=4, W=16, C0=512, N=128, ksize=3, flags=HALO, **_ALL),
    case("slab halo linear forms", "halo", "plain", cfg=(128, 128, 8), images=2, H=4, W=16, C0=512, N=128, ksize=3, flags=HALO, **_LIN),
    case("slab pc all forms", "pc", "plain", cfg=(64, 160, 4), images=2, H=8, W=8, C0=512, N=160, ksize=3, flags={"pc": 8}, **_ALL),
    case("slab pc linear forms", "pc", "plain", cfg=(64, 160, 4), images=2, H=8, W=8, C0=512, N=160, ksize=3, flags={"pc": 8}, **_LIN),
    case("slab smap all forms", "smap", "plain", cfg=(512, 64, 2), images=8, H=8, W=8, C0=128, N=64, ksize=3, flags={"smap": 1}, **_ALL),
    case("slab smap linear forms", "smap", "plain", cfg=(512, 64, 2), images=8, H=8, W=8, C0=128, N=64, ksize=3, flags={"smap": 1}, **_LIN),
]
SLAB_PAIRS = [("slab general N 320 linear forms", "slab general N 320 odd pitch")]

# the VAE attention's three launches at B = 3, 80 tokens (ragged against the 64-row tile), C = 128.  The P V^T launch contracts over the tokens;
# the launcher takes K in multiples of 64 only, so its key axis is 128 tokens against 80 query rows
BATCHED = [
    case("batched shared A row bias", "general", cfg=(64, 64, 1), W=128, C0=128, N=80, bias_mode=2, out_f32=False, batched={"B": 3, "shared_a": True}),
    case("batched scores alpha fp32", "general", cfg=(64, 64, 1), W=80, C0=128, N=80, bias_mode=0, alpha=128 ** -0.5, batched={"B": 3}),
    case("batched P V^T", "general", cfg=(64, 64, 1), W=80, C0=128, N=128, bias_mode=0, out_f32=False, batched={"B": 3}),
]

# LayerNorm fold.  Producers: plain bf16 launches that also leave per-row (sum, sum of squares) per N tile; `rowstat` = the N tiles expected
LN_PRODUCERS = [
    case("rowstat one slot", "general", cfg=(128, 128, 1), W=200, C0=4096, N=128, out_f32=False, rowstat=1),
    case("rowstat two slots 160 wide", "general", cfg=(128, 160, 1), W=8164, C0=512, N=320, out_f32=False, rowstat=2),
    case("rowstat three slots ragged tile", "general", cfg=(128, 128, 1), W=200, C0=4096, N=320, out_f32=False, rowstat=3),
    case("rowstat 64 wide tiles", "general", cfg=(64, 64, 1), W=200, C0=128, N=200, out_f32=False, rowstat=4),
    case("rowstat pc", "pc", cfg=(64, 160, 1), W=1536, C0=1024, N=1280, out_f32=False, rowstat=8, flags={"pc": 1}),
    case("rowstat wreg", "wreg", cfg=(64, 128, 1), W=1024, C0=128, N=1024, out_f32=False, rowstat=8, flags={"wreg": 1}),
    case("rowstat 8p declines", "general", cfg=(64, 64, 1), W=512, C0=128, N=256, out_f32=False, rowstat=4, flags={"p8": 2}),
]
_LNC = dict(out_f32=False)
LN_CONSUMERS = [
    case("ln general one slot", "general", cfg=(64, 64, 1), W=200, C0=128, N=200, ln={"slots": 1}, **_LNC),
    case("ln general two slots element", "general", cfg=(64, 64, 1), W=200, C0=128, N=200, ln={"slots": 2}, ldo_extra=1, **_LNC),
    case("ln general three slots mean 1 std 3", "general", cfg=(64, 64, 1), W=200, C0=192, N=200, ln={"slots": 3, "mean": 1.0, "std": 3.0}, **_LNC),
    case("ln general offset rows", "general", cfg=(64, 64, 1), W=200, C0=128, N=200, ln={"slots": 2, "mean": 8.0, "std": 1.0, "offset": True}, **_LNC),
    case("ln general geglu", "general", cfg=(128, 128, 1), W=200, C0=128, N=256, geglu=True, ln={"slots": 2}, **_LNC),
    case("ln general geglu element", "general", cfg=(128, 128, 1), W=200, C0=128, N=256, geglu=True, ln={"slots": 3}, ldo_extra=1, **_LNC),
    case("ln pc", "pc", cfg=(64, 160, 1), W=1536, C0=1024, N=1280, ln={"slots": 2}, flags={"pc": 1}, **_LNC),
    case("ln wreg", "wreg", cfg=(64, 128, 1), W=1024, C0=128, N=1024, ln={"slots": 2}, flags={"wreg": 1}, **_LNC),
    case("ln wreg geglu", "wreg", cfg=(64, 256, 1), W=2048, C0=128, N=1024, geglu=True, ln={"slots": 1}, flags={"wreg": 2}, **_LNC),
    case("ln 8p", "8p", cfg=(256, 256, 1), W=512, C0=128, N=256, ln={"slots": 3}, flags={"p8": 2}, **_LNC),
]

# GroupNorm statistics producer: per-(M tile, channel) sums of the launch's own bf16 output; several images, tiles inside one image
COLSTAT = [
    case("colstat 1x1", "general", cfg=(64, 64, 1), images=3, H=8, W=8, C0=128, N=96, out_f32=False, colstat=True),
    case("colstat halo", "halo", cfg=(128, 128, 1), images=2, H=8, W=16, C0=512, N=128, ksize=3, out_f32=False, colstat=True, flags=HALO),
    case("colstat pc", "pc", cfg=(64, 160, 1), images=24, H=8, W=8, C0=1024, N=1280, out_f32=False, colstat=True, flags={"pc": 1}),
    case("colstat wreg", "wreg", cfg=(64, 128, 1), images=16, H=8, W=8, C0=128, N=1024, out_f32=False, colstat=True, flags={"wreg": 1}),
    case("colstat 8p", "8p", cfg=(256, 256, 1), images=2, H=16, W=16, C0=128, N=256, out_f32=False, colstat=True, flags={"p8": 2}),
]
COLSTAT_REFUSED = [(case("colstat refused: 48-row images", "none", images=4, W=48, C0=128, N=96, out_f32=False, colstat=True), "column statistics")]

# slab sum + GroupNorm: the three instantiations by quads = Hout Wout (channels per group) / 4, and the shapes the pass declines
_GN = dict(out_f32=False, ksize=1, C0=4096)
SLAB_GN = [
    case("gn 640 quads", "general", "gn", cfg=(64, 160, 4), images=2, H=8, W=8, N=160, gn={"groups": 4, "silu": 1}, **_GN),
    case("gn 640 quads all forms", "general", "gn", cfg=(64, 160, 4), images=2, H=8, W=8, N=160, gn={"groups": 4, "silu": 1}, rowadd=True, residual=True, act=1, **_GN),
    case("gn 704 quads no bias", "general", "gn", cfg=(128, 128, 8), images=2, H=8, W=8, N=176, gn={"groups": 4}, bias_mode=0, **_GN),
    case("gn 1280 quads rowadd", "general", "gn", cfg=(64, 160, 4), images=2, H=16, W=16, N=160, gn={"groups": 8, "silu": 1}, rowadd=True, **_GN),
    case("gn 2560 quads residual", "general", "gn", cfg=(64, 160, 4), images=2, H=16, W=16, N=160, gn={"groups": 4}, residual=True, **_GN),
]
SLAB_GN_DECLINED = [
    case("gn declined: 42 channels per group", "general", "plain", cfg=(128, 128, 8), images=2, H=8, W=8, N=168, gn={"groups": 4}, **_GN),
    case("gn declined: 3328 quads", "general", "plain", cfg=(128, 128, 8), images=2, H=16, W=16, N=208, gn={"groups": 4}, **_GN),
    case("gn declined: quick gelu", "general", "plain", cfg=(64, 160, 4), images=2, H=8, W=8, N=160, gn={"groups": 4}, act=2, **_GN),
    case("gn declined: fp32 output", "general", "plain", cfg=(64, 160, 4), images=2, H=8, W=8, N=160, gn={"groups": 4}, **dict(_GN, out_f32=True)),
]

# per-image weights: image i multiplies with its own matrix
WPI = [
    case("wpi 64x160", "general", cfg=(64, 160, 1), images=4, H=16, W=32, C0=64, N=1280, wpi=True, rowadd=True),
    case("wpi 64x160 pc", "pc", cfg=(64, 160, 1), images=4, H=16, W=32, C0=64, N=1280, wpi=True, rowadd=True, flags={"pc": 1}),
    case("wpi 64-row images", "general", cfg=(64, 64, 1), images=3, H=8, W=8, C0=128, N=128, wpi=True, rowadd=True, out_f32=False),
    case("wpi 128-row tiles", "general", cfg=(128, 128, 1), images=3, H=64, W=128, C0=64, N=128, wpi=True, rowadd=True),
]
WPI_REFUSED = [
    (case("wpi refused: 48-row images", "none", images=4, W=48, C0=128, N=128, wpi=True), "per-image"),
    (case("wpi refused: geglu", "none", images=3, H=8, W=8, C0=128, N=256, wpi=True, geglu=True), "per-image"),
    (case("wpi refused: 3x3", "none", images=3, H=8, W=8, C0=128, N=128, wpi=True, ksize=3), "per-image"),
]

LAUNCHED = GATHER + SHORTCUT + EPILOGUE + SLAB + BATCHED + LN_PRODUCERS + LN_CONSUMERS + COLSTAT + SLAB_GN + SLAB_GN_DECLINED + WPI
BY_NAME = {c["name"]: c for c in LAUNCHED}
assert len(BY_NAME) == len(LAUNCHED), "case names are unique"
