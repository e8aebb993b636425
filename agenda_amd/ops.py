"""Single-op bindings (fp32 torch tensors on the GPU -> HIP kernels -> fp32).  These mirror the
torch.nn.functional calls that diffusers makes on the reference path so each HIP kernel can be
parity-tested in isolation through the C ABI (`agd_op_*` in include/agenda_hip.h)."""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def _f32c(t):
    assert t.is_cuda, "ops run on the GPU only (no CPU fallback)"
    return t.detach().to(torch.float32).contiguous()


_P8 = {0: 0, 1: 2, 2: 4, 3: 8}      # igemm8p.h: 1 = where the launcher would pick it, 2 / 3 = force the 256- / 160-wide tile


def conv2d(x, w, bias=None, stride=1, padding=None, upsample=False, halo=False, p8=0, smap=False, phases=False, pc=0, xcd_block=False):
    lib = _lib.load()
    x, w = _f32c(x), _f32c(w)
    b = _f32c(bias) if bias is not None else None
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    pad = (1 if k == 3 else 0) if padding is None else padding
    up = 2 if upsample else 1
    Ho = (H * up + 2 * pad - k) // stride + 1
    Wo = (W * up + 2 * pad - k) // stride + 1
    y = torch.empty(B, Cout, Ho, Wo, device=x.device, dtype=torch.float32)
    _lib.check(lib.agd_op_conv2d_ex(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), B, Cin, H, W, Cout, k, stride,
                                    pad, int(upsample), (1 if halo else 0) | _P8[p8] | (16 if smap else 0) | (64 if phases else 0) | ((int(pc) & 15) << 7) | ((int(pc) & 48) << 8) | (2048 if xcd_block else 0), _lib.current_stream_ptr()), None, "agd_op_conv2d")
    return y


def linear(x, w, bias=None, residual=None, geglu=False, p8=0, wreg=False, kgroups=False, pc=0, xcd_block=False):
    lib = _lib.load()
    x2 = _f32c(x).reshape(-1, x.shape[-1])
    w = _f32c(w)
    M, K = x2.shape
    N = w.shape[0]
    Nout = N // 2 if geglu else N
    b = _f32c(bias) if bias is not None else None
    r = _f32c(residual).reshape(M, Nout) if residual is not None else None
    y = torch.empty(M, Nout, device=x.device, dtype=torch.float32)
    _lib.check(lib.agd_op_linear(_lib.ptr(x2), _lib.ptr(w), _lib.ptr(b), _lib.ptr(r), _lib.ptr(y), M, K, N, int(geglu) | _P8[p8] | (16 if wreg else 0) | (32 if kgroups else 0) | (64 if (wreg and kgroups) else 0) | ((int(pc) & 15) << 7) | ((int(pc) & 48) << 8) | (2048 if xcd_block else 0),
                                 _lib.current_stream_ptr()), None, "agd_op_linear")
    return y.reshape(*x.shape[:-1], Nout)


IGEMM_FAMILY = {0: "none", 1: "general", 2: "halo", 3: "pch", 4: "pc", 5: "8p", 6: "smap", 7: "wreg"}     # agd_igemm_desc.ran[0]
IGEMM_SLAB = {0: "none", 1: "plain", 2: "gn"}                                                           # agd_igemm_desc.ran[1]
IGEMM_SENTINEL = -24576.0        # exact in bf16: what `igemm` pre-fills every output buffer with
IGEMM_GUARD_ROWS = 16            # rows allocated (and pre-filled) behind the M rows of every output


def igemm(src0, w, *, src1=None, sc0=None, sc1=None, ksize=1, stride=1, pad=None, up=1, hout=0, wout=0, bias=None, bias_mode=None, rowadd=None,
          rowadd_ld=None, residual=None, ldr=None, alpha=1.0, geglu=False, act=0, out_f32=True, ldo=None, batch=1, strides=None, w_per_image=False,
          rowstat_slots=0, ln_stats=None, ln_cs=None, ln_invC=0.0, ln_eps=0.0, colstat_rows=0, gn=None, halo=0, p8=0, smap=0, pc=0, kg2=0, wreg=0,
          xcd_block=0, check=True):
    """One implicit-GEMM launch stated field by field (`agd_op_igemm`, the launcher's `IgemmP`).  src0 / src1 / sc0 / sc1: NHWC
    [images, H, W, C] (batch > 1: [batch, 1, H, W, C] with `strides` = (sA0, sA1, sW, sO, sR) in elements); w [N, K] or [images or batch, N, K]
    in the kernel's K order (tap-major, then the shortcut columns; geglu: value rows then gate rows); residual [M, ldr] (batch: [batch, M, ldr]).
    bias / rowadd / ln_stats / ln_cs and gn["gamma"] / gn["beta"] reach the launch as the tensors they are (storage offset included).
    gn: {"gamma", "beta", "groups", "eps", "silu", "keep_out"} -- the GroupNorm a split-K launch's slab pass may apply.
    -> dict: out [M + IGEMM_GUARD_ROWS, ldo] (batch > 1: the flat buffer), pre-filled with IGEMM_SENTINEL; rc / err (check=False: a refusal is
    returned, not raised); cfg (BM, BN, splits); family / slab (names of IGEMM_FAMILY / IGEMM_SLAB); gn_fused; can_fuse_sc; gn_y [M, N];
    rowstat [M + guard, slots, 2]; colstat [ceil(M / 64), N, 2] (the launch fills M / BM tiles of it)."""
    lib = _lib.load()
    d = _lib.AgdIgemmDesc()
    d.struct_size = ctypes.sizeof(d)
    keep = []

    def dev(t):
        if t is None:
            return None, 0
        t = _f32c(t)
        keep.append(t)
        return t.data_ptr(), t.numel()

    def given(t):
        if t is None:
            return None
        assert t.is_cuda and t.dtype == torch.float32
        keep.append(t)
        return t.data_ptr()

    images, H, W, C0 = src0.shape[-4:]
    d.images, d.H, d.W, d.C0 = images, H, W, C0
    d.C1 = 0 if src1 is None else src1.shape[-1]
    d.ksize, d.stride, d.up, d.hout, d.wout = ksize, stride, up, hout, wout
    d.pad = (1 if ksize == 3 else 0) if pad is None else pad
    Ho = hout if hout > 0 else (H * up + 2 * d.pad - ksize) // stride + 1
    Wo = wout if wout > 0 else (W * up + 2 * d.pad - ksize) // stride + 1
    M = images * Ho * Wo
    N, K = w.shape[-2:]
    Nout = N // 2 if geglu else N
    d.N, d.K, d.w_per_image = N, K, int(bool(w_per_image))
    d.sc_C0 = 0 if sc0 is None else sc0.shape[-1]
    d.sc_C1 = 0 if sc1 is None else sc1.shape[-1]
    d.src0, d.n_src0 = dev(src0)
    d.src1, d.n_src1 = dev(src1)
    d.sc0, d.n_sc0 = dev(sc0)
    d.sc1, d.n_sc1 = dev(sc1)
    d.w, d.n_w = dev(w)
    d.residual, d.n_res = dev(residual)
    d.bias = given(bias)
    d.bias_mode = (0 if bias is None else 1) if bias_mode is None else bias_mode
    d.rowadd = given(rowadd)
    d.rowadd_ld = (0 if rowadd is None else N) if rowadd_ld is None else rowadd_ld
    d.ldr = (residual.shape[-1] if residual is not None else Nout) if ldr is None else ldr
    d.ldo = Nout if ldo is None else ldo
    d.alpha, d.geglu, d.act, d.out_f32, d.batch = float(alpha), int(bool(geglu)), int(act), int(bool(out_f32)), int(batch)
    if strides is not None:
        d.sA0, d.sA1, d.sW, d.sO, d.sR = (int(s) for s in strides)
    d.ln_stats, d.ln_cs = given(ln_stats), given(ln_cs)
    d.ln_slots = 0 if ln_stats is None else ln_stats.shape[-2]
    d.ln_invC, d.ln_eps = float(ln_invC), float(ln_eps)
    d.halo, d.p8, d.smap, d.pc, d.kg2, d.wreg, d.xcd_block = int(halo), int(p8), int(smap), int(pc), int(kg2), int(wreg), int(xcd_block)
    device = src0.device
    rows = M + IGEMM_GUARD_ROWS
    n_out = (batch - 1) * d.sO + rows * d.ldo if batch > 1 else rows * d.ldo
    out = torch.full((n_out,), IGEMM_SENTINEL, device=device, dtype=torch.float32)
    d.out, d.n_out = out.data_ptr(), n_out
    res = {}
    if rowstat_slots > 0:
        res["rowstat"] = torch.full((rows, rowstat_slots, 2), IGEMM_SENTINEL, device=device, dtype=torch.float32)
        d.rowstat, d.rowstat_slots = res["rowstat"].data_ptr(), rowstat_slots
    if colstat_rows > 0:
        res["colstat"] = torch.full(((M + 63) // 64, N, 2), IGEMM_SENTINEL, device=device, dtype=torch.float32)
        d.colstat, d.colstat_rows = res["colstat"].data_ptr(), colstat_rows
    if gn is not None:
        res["gn_y"] = torch.full((M, N), IGEMM_SENTINEL, device=device, dtype=torch.float32)
        d.gn_y, d.gn_gamma, d.gn_beta = res["gn_y"].data_ptr(), given(gn["gamma"]), given(gn["beta"])
        d.gn_groups, d.gn_eps, d.gn_silu, d.gn_keep_out = int(gn["groups"]), float(gn.get("eps", 1e-5)), int(gn.get("silu", 0)), int(gn.get("keep_out", 0))
    rc = lib.agd_op_igemm(ctypes.byref(d), _lib.current_stream_ptr())
    err = ""
    if rc != 0:
        msg = lib.agd_last_error(None)
        err = msg.decode() if msg else "?"
        if check:
            raise _lib.AgendaHipError(f"agd_op_igemm failed (rc={rc}): {err}")
    res.update(out=out if batch > 1 else out.view(rows, d.ldo), rc=rc, err=err, cfg=tuple(d.cfg), family=IGEMM_FAMILY.get(d.ran[0], d.ran[0]),
               slab=IGEMM_SLAB.get(d.ran[1], d.ran[1]), gn_fused=d.gn_fused, can_fuse_sc=d.can_fuse_sc, M=M, Nout=Nout)
    return res


GN_PATH_PARTIAL, GN_PATH_TWO_KERNEL = 1, 2      # what return_path reports: the partial-sum kernel, or statistics kernel + apply kernel


def group_norm(x, groups, gamma, beta, eps=1e-5, silu=False, *, x1=None, part=None, bm=None, part1=None, bm1=None, return_path=False):
    """GroupNorm(+SiLU) of x [B, C0, ...], or of the channel concat x | x1.  part / bm (and part1 / bm1 for x1): partial-sum tables made by
    the caller, [B, HW / bm, Cs, 2] fp32 = (sum, sum of squares) of the source's bf16 values per tile of bm pixels -- what the producing GEMM
    leaves in production; given for every source and on a supported shape, the one-kernel form runs.  return_path: also which form ran."""
    lib = _lib.load()
    x = _f32c(x)
    B, C0 = x.shape[:2]
    HW = x[0, 0].numel()
    C1 = 0
    if x1 is not None:
        x1 = _f32c(x1)
        assert x1.shape[0] == B and x1.shape[2:] == x.shape[2:], "x1 must share x's batch and map"
        C1 = x1.shape[1]
    if part is None and part1 is None and x1 is None and not return_path:
        y = torch.empty_like(x)
        _lib.check(lib.agd_op_groupnorm(_lib.ptr(x), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(y), B, C0, HW,
                                        groups, float(eps), int(silu), _lib.current_stream_ptr()), None, "agd_op_groupnorm")
        return y
    for t, b_, cs in ((part, bm, C0), (part1, bm1, C1)):
        if t is not None:
            assert b_ and b_ > 0 and t.dtype == torch.float32 and t.numel() == B * (HW // b_) * cs * 2, "partial-sum table [B, HW // bm, Cs, 2] fp32"
    part = _f32c(part) if part is not None else None
    part1 = _f32c(part1) if part1 is not None else None
    y = torch.empty(B, C0 + C1, *x.shape[2:], device=x.device, dtype=torch.float32)
    path = ctypes.c_int(0)
    _lib.check(lib.agd_op_groupnorm_ex(_lib.ptr(x), _lib.ptr(x1), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(y), B, C0, C1, HW,
                                       groups, float(eps), int(silu), _lib.ptr(part), int(bm or 0), _lib.ptr(part1), int(bm1 or 0),
                                       ctypes.byref(path), _lib.current_stream_ptr()), None, "agd_op_groupnorm_ex")
    return (y, path.value) if return_path else y


def gn_fold(part, bm, groups, gamma, beta, w, bias=None, eps=1e-6, x=None, frag_ni=0, hw=None):
    """The GroupNorm folded into the projection behind it, piece by piece (agd_op_gn_fold): part [B, HW / bm, C, 2] fp32 partial sums, w [N, C].
    -> dict: wb [B, N, C], rowadd [B, N]; with frag_ni > 0 wb_frag and wb_frag_ref [B, N * C] (the kernel's fragment order, and the library's
    re-layout of the row-major wb); with x [B, C, ...]: y [B, HW, N] = the raw x through the per-image matrices plus rowadd.
    hw: the pixel count where it is not (tiles x bm) -- a shape the entry refuses."""
    lib = _lib.load()
    part, w = _f32c(part), _f32c(w)
    B, nt, Cc = part.shape[:3]
    HW = nt * bm if hw is None else hw
    N = w.shape[0]
    assert w.shape[1] == Cc and part.shape[3] == 2
    b = _f32c(bias) if bias is not None else None
    dev = part.device
    out = {"wb": torch.empty(B, N, Cc, device=dev), "rowadd": torch.empty(B, N, device=dev)}
    if frag_ni > 0:
        out["wb_frag"] = torch.empty(B, N * Cc, device=dev)
        out["wb_frag_ref"] = torch.empty(B, N * Cc, device=dev)
    if x is not None:
        x = _f32c(x)
        assert x.shape[0] == B and x.shape[1] == Cc and x[0, 0].numel() == HW
        out["y"] = torch.empty(B, HW, N, device=dev)
    _lib.check(lib.agd_op_gn_fold(_lib.ptr(x), _lib.ptr(part), int(bm), B, Cc, HW, groups, float(eps), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)),
                                  _lib.ptr(w), _lib.ptr(b), N, int(frag_ni), _lib.ptr(out["wb"]), _lib.ptr(out["rowadd"]), _lib.ptr(out.get("wb_frag")),
                                  _lib.ptr(out.get("wb_frag_ref")), _lib.ptr(out.get("y")), _lib.current_stream_ptr()), None, "agd_op_gn_fold")
    return out


def layer_norm(x, gamma, beta, eps=1e-5, return_path=False):
    """return_path: also which layernorm_kernel<LPR, MAXV> ran, as (LPR, MAXV)"""
    lib = _lib.load()
    x = _f32c(x)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty_like(x)
    if return_path:
        inst = ctypes.c_int(0)
        _lib.check(lib.agd_op_layernorm_ex(_lib.ptr(x), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(y), rows, Cc,
                                           float(eps), ctypes.byref(inst), _lib.current_stream_ptr()), None, "agd_op_layernorm_ex")
        return y, divmod(inst.value, 100)
    _lib.check(lib.agd_op_layernorm(_lib.ptr(x), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(y), rows, Cc,
                                    float(eps), _lib.current_stream_ptr()), None, "agd_op_layernorm")
    return y


def ff_fused(x, gamma, beta, w1, b1, w2, b2, eps=1e-5):
    """x + ff.net.2(GEGLU(ff.net.0(LayerNorm(x)))) as ONE launch (tblock.hip); x [..., C], w1 [8C, C] (value rows then gate rows), w2 [C, 4C]."""
    lib = _lib.load()
    Cc = x.shape[-1]
    x2 = _f32c(x).reshape(-1, Cc)
    y = torch.empty_like(x2)
    _lib.check(lib.agd_op_ff_fused(_lib.ptr(x2), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(_f32c(w1)), _lib.ptr(_f32c(b1)),
                                   _lib.ptr(_f32c(w2)), _lib.ptr(_f32c(b2)), _lib.ptr(y), x2.shape[0], Cc, float(eps),
                                   _lib.current_stream_ptr()), None, "agd_op_ff_fused")
    return y.reshape(x.shape)


def attn_chain(x, gamma, beta, wq, kv, wo, bo, heads=8, eps=1e-5, return_probs=False, rows32=False):
    """x + to_out(attention(to_q(LayerNorm(x)), k, v)) as ONE launch (tblock.hip); x [B, HW, C], kv [B, T, 2C] (K columns then V columns).
    With return_probs: also the probabilities summed over the heads, [B, T, HW]."""
    lib = _lib.load()
    x, kv = _f32c(x), _f32c(kv)
    B, HW, Cc = x.shape
    T = kv.shape[1]
    y = torch.empty_like(x)
    pr = torch.empty(B, T, HW, device=x.device, dtype=torch.float32) if return_probs else None
    _lib.check(lib.agd_op_attn_chain(_lib.ptr(x), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(_f32c(wq)), _lib.ptr(kv), _lib.ptr(_f32c(wo)),
                                     _lib.ptr(_f32c(bo)), _lib.ptr(y), _lib.ptr(pr), B, HW, T, Cc, heads | (256 if rows32 else 0), float(eps), _lib.current_stream_ptr()),
               None, "agd_op_attn_chain")
    return (y, pr) if return_probs else y


def ff_premul_weights(w2, b2, wp, bp):
    """The pre-multiplied form's operands as the loader builds them: Wp W2 through the library's own GEMM, rounded to bf16 once, and
    Wp b2 + bp in fp64 from the bf16 Wp (rounded to fp32 once).  -> (w2p [C, 4C], bcp [C]), fp32 on the GPU"""
    wpb = _f32c(wp).to(torch.bfloat16).float()
    w2p = linear(wpb, _f32c(w2).t().contiguous()).to(torch.bfloat16).float()
    bcp = (wpb.double() @ _f32c(b2).double() + _f32c(bp).double()).float()
    return w2p, bcp


def ff_fused_ex(x, gamma, beta, w1, b1, w2, b2, eps=1e-5, *, wp=None, bp=None, xres=None, xres_rows=0, premul=False, colstat=False, inplace=False):
    """`ff_fused` reaching every form of the kernel (agd_op_ff_fused_ex); x [M, C].  wp / bp / xres: the proj_out stage behind it, -> pout
    [M, C] = (x + FF(x)) wp^T + bp + xres, xres [xres_rows or M, C] (output row m adds row m % xres_rows).  premul: the launch gets
    `ff_premul_weights(w2, b2, wp, bp)` in place of w2 and bp.  colstat: also the [ceil(M / 128), C, 2] channel sums of pout's tiles.
    inplace: the launch writes over its own input."""
    lib = _lib.load()
    x2 = _f32c(x)
    M, Cc = x2.shape
    y = pout = cst = xr = None
    w2_, bp_ = _f32c(w2), (None if bp is None else _f32c(bp))
    if wp is not None:
        pout = torch.empty_like(x2)
        if xres is not None:
            xr = _f32c(xres)
            assert tuple(xr.shape) == ((xres_rows if xres_rows > 0 else M), Cc), "xres [xres_rows or M, C]"
        if premul:
            w2_, bp_ = ff_premul_weights(w2, b2, wp, bp)
        if colstat:
            cst = torch.full(((M + 127) // 128, Cc, 2), float("nan"), device=x2.device, dtype=torch.float32)
    else:
        y = torch.empty_like(x2)
        if colstat:
            cst = torch.zeros(1, device=x2.device)
    _lib.check(lib.agd_op_ff_fused_ex(_lib.ptr(x2), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(_f32c(w1)), _lib.ptr(_f32c(b1)),
                                      _lib.ptr(w2_), _lib.ptr(_f32c(b2)), _lib.ptr(y), M, Cc, float(eps), _lib.ptr(None if wp is None else _f32c(wp)),
                                      _lib.ptr(bp_), _lib.ptr(xr), int(xres_rows), _lib.ptr(pout), int(bool(premul)), _lib.ptr(cst), int(bool(inplace)),
                                      _lib.current_stream_ptr()), None, "agd_op_ff_fused_ex")
    out = y if wp is None else pout
    return (out, cst) if colstat else out


def attn_chain_ex(x, gamma, beta, wq, kv, wo, bo, heads=8, eps=1e-5, *, hw=None, o1=None, wo1=None, bo1=None, src_rows=0, rowstat=False, rec=None,
                  rec_hpb=8, rec_b0=0, rec_T=None, rows32=False, inplace=False):
    """`attn_chain` reaching every form of the kernel (agd_op_attn_chain_ex); kv [B, T, 2C]; x [B, HW, C], or with src_rows > 0 x [src_rows, C]
    and hw given: output row m reads input row m % src_rows.  o1 (x's shape) / wo1 / bo1: the attn1.to_out prologue, h1 = o1 wo1^T + bo1 + x is
    the chain's input.  rec: the recorder rows [B - rec_b0, 8 / rec_hpb, rows, HW], fp32 on the GPU, ADDED to in place (token rows < rec_T,
    default all the buffer's).  -> dict: y [B, HW, C]; h1 (with the prologue); rowstat [B, HW, 2] (if asked)."""
    lib = _lib.load()
    x, kv = _f32c(x), _f32c(kv)
    Cc = x.shape[-1]
    B, T = kv.shape[:2]
    if src_rows > 0:
        assert x.dim() == 2 and x.shape[0] == src_rows and hw, "src_rows: x [src_rows, C] and hw"
        HW = int(hw)
    else:
        assert x.dim() == 3 and x.shape[0] == B, "x [B, HW, C]"
        HW = x.shape[1]
    dev = x.device
    out = {"y": torch.empty(B, HW, Cc, device=dev, dtype=torch.float32)}
    pre = o1 is not None
    if pre:
        o1 = _f32c(o1)
        assert o1.shape == x.shape, "o1 has x's shape"
        out["h1"] = torch.empty(B, HW, Cc, device=dev, dtype=torch.float32)
    if rowstat:
        out["rowstat"] = torch.full((B, HW, 2), float("nan"), device=dev, dtype=torch.float32)
    rec_rows = 0
    if rec is not None:
        assert rec.is_cuda and rec.dtype == torch.float32 and rec.is_contiguous() and rec.dim() == 4 and rec.shape[3] == HW, "rec [B - rec_b0, groups, rows, HW]"
        assert 0 <= rec_b0 <= B and rec.shape[0] == max(B - rec_b0, 0) and rec.shape[0] > 0, "one recorder image per recording batch row"
        assert rec_hpb not in (1, 2, 4, 8) or rec.shape[1] == 8 // rec_hpb, "one slice per head group"
        rec_rows = rec.shape[2]
        rec_T = rec_rows if rec_T is None else int(rec_T)
    _lib.check(lib.agd_op_attn_chain_ex(_lib.ptr(x), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(_f32c(wq)), _lib.ptr(_given(kv)), _lib.ptr(_f32c(wo)),
                                        _lib.ptr(_f32c(bo)), _lib.ptr(out["y"]), B, HW, T, Cc, int(heads), float(eps), _lib.ptr(o1),
                                        _lib.ptr(_f32c(wo1) if pre else None), _lib.ptr(_f32c(bo1) if pre else None), _lib.ptr(out.get("h1")), int(src_rows),
                                        _lib.ptr(out.get("rowstat")), _lib.ptr(rec), int(rec_hpb), int(rec_b0), int(rec_T or 0), int(rec_rows), int(bool(rows32)),
                                        int(bool(inplace)), _lib.current_stream_ptr()), None, "agd_op_attn_chain_ex")
    return out


def qkv_chain(x, hw, gn_gamma, gn_beta, groups, part, bm, w_in, b_in, gamma, beta, wqkv, *, gn_eps=1e-6, ln_eps=1e-5, inside=False, rows64=False, sched2=False):
    """GroupNorm -> proj_in -> h -> norm1 -> q | k | v as ONE launch (agd_op_qkv_chain): x [M, C] = the raw rows of M / hw images, part
    [M // hw, hw // bm, C, 2] fp32 = the partial sums of those rows per tile of bm pixels (the table the producing GEMM leaves).  inside: the
    GroupNorm is applied by the kernel; else it is folded into per-image proj_in matrices first.  -> (h [M, C], qkv [M, 3C])"""
    lib = _lib.load()
    x, part = _f32c(x), _f32c(part)
    M, Cc = x.shape
    h = torch.empty(M, Cc, device=x.device, dtype=torch.float32)
    qkv = torch.empty(M, 3 * Cc, device=x.device, dtype=torch.float32)
    if hw > 0 and bm > 0:
        assert part.numel() >= max(M // hw, 1) * (hw // bm) * Cc * 2, "partial-sum table [M // hw, hw // bm, C, 2] fp32"
    _lib.check(lib.agd_op_qkv_chain(_lib.ptr(x), _lib.ptr(_f32c(gn_gamma)), _lib.ptr(_f32c(gn_beta)), int(groups), float(gn_eps), _lib.ptr(_given(part)), int(bm),
                                    _lib.ptr(_f32c(w_in)), _lib.ptr(_f32c(b_in)), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), float(ln_eps),
                                    _lib.ptr(_f32c(wqkv)), _lib.ptr(h), _lib.ptr(qkv), M, int(hw), Cc, (1 if inside else 0) | (2 if rows64 else 0) | (4 if sched2 else 0),
                                    _lib.current_stream_ptr()), None, "agd_op_qkv_chain")
    return h, qkv


def xattn_premul(x, gamma, beta, wq, kv, wo, bo, heads=8, eps=1e-5, return_probs=False):
    """x + to_out(attention(to_q(LayerNorm(x)), k, v)) through the pre-multiplied context matrices of the C = 1280 blocks (xattn_pre.hip): x [B, HW, C],
    kv [B, T, 2C] (K columns then V columns).  With return_probs: also every head's probabilities, [B, heads, T, HW]."""
    lib = _lib.load()
    x, kv = _f32c(x), _f32c(kv)
    B, HW, Cc = x.shape
    T = kv.shape[1]
    y = torch.empty_like(x)
    pr = torch.empty(B, heads, T, HW, device=x.device, dtype=torch.float32) if return_probs else None
    _lib.check(lib.agd_op_xattn_premul(_lib.ptr(x), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(_f32c(wq)), _lib.ptr(kv), _lib.ptr(_f32c(wo)),
                                       _lib.ptr(_f32c(bo)), _lib.ptr(y), _lib.ptr(pr), B, HW, T, Cc, heads, float(eps), _lib.current_stream_ptr()),
               None, "agd_op_xattn_premul")
    return (y, pr) if return_probs else y


XATTN_TP = 80                    # token rows per head of the pre-multiplied matrices (kernels.h)


def xattn_context(kv, wq, wo, gamma, beta, heads=8):
    """The context products of `xattn_premul` as its launches write them (agd_op_xattn_context): kv [B, T, 2C] ->
    (kpp [B, H, 80, C], cs [B, H, 80], bs [B, H, 80], vpp [B, C, H, 80]), the bf16 ones widened, the padding included."""
    lib = _lib.load()
    kv = _f32c(kv)
    B, T, C2 = kv.shape
    Cc, H = C2 // 2, int(heads)
    dev = kv.device
    kpp = torch.empty(B, H, XATTN_TP, Cc, device=dev, dtype=torch.float32)
    cs = torch.empty(B, H, XATTN_TP, device=dev, dtype=torch.float32)
    bs = torch.empty_like(cs)
    vpp = torch.empty(B, Cc, H, XATTN_TP, device=dev, dtype=torch.float32)
    _lib.check(lib.agd_op_xattn_context(_lib.ptr(_given(kv)), _lib.ptr(_f32c(wq)), _lib.ptr(_f32c(wo)), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(kpp),
                                        _lib.ptr(cs), _lib.ptr(bs), _lib.ptr(vpp), B, T, Cc, H, _lib.current_stream_ptr()), None, "agd_op_xattn_context")
    return kpp, cs, bs, vpp


def xattn_scores(x, kpp, cs, bs, T, heads=8, eps=1e-5, *, stats=None, rec=None, rec_b0=0, rec_T=None):
    """`xattn_s_kernel` alone (agd_op_xattn_scores): x [B, HW, C], kpp [B, H, 80, C], cs / bs [B, H, 80] (the caller's, hand-made ones included)
    -> P [B, HW, H, 80].  stats [B * HW, slots, 2]: the rows' (sum, sum of squares) as slots partial sums (None: one slot, computed by the
    library).  rec: [B - rec_b0, H, rows, HW] fp32 on the GPU, ADDED to in place and never zeroed (token rows < rec_T, default all rows)."""
    lib = _lib.load()
    x, kpp, cs, bs = _f32c(x), _f32c(kpp), _f32c(cs), _f32c(bs)
    B, HW, Cc = x.shape
    H = int(heads)
    assert kpp.shape == (B, H, XATTN_TP, Cc) and cs.shape == (B, H, XATTN_TP) and bs.shape == cs.shape, "kpp [B, H, 80, C], cs / bs [B, H, 80]"
    slots = 0
    if stats is not None:
        stats = _f32c(stats)
        assert stats.dim() == 3 and stats.shape[0] == B * HW and stats.shape[2] == 2, "stats [B * HW, slots, 2]"
        slots = stats.shape[1]
    rec_rows = 0
    if rec is not None:
        assert rec.is_cuda and rec.dtype == torch.float32 and rec.is_contiguous() and rec.dim() == 4, "rec: contiguous fp32 on the GPU"
        assert 0 <= rec_b0 < B and rec.shape[0] == B - rec_b0 and rec.shape[1] == H and rec.shape[3] == HW, "rec [B - rec_b0, H, rows, HW]"
        rec_rows = rec.shape[2]
        rec_T = rec_rows if rec_T is None else int(rec_T)
    P = torch.empty(B, HW, H, XATTN_TP, device=x.device, dtype=torch.float32)
    _lib.check(lib.agd_op_xattn_scores(_lib.ptr(x), _lib.ptr(stats), slots, _lib.ptr(kpp), _lib.ptr(cs), _lib.ptr(bs), _lib.ptr(P), _lib.ptr(rec), int(rec_b0),
                                       int(rec_T or 0), int(rec_rows), B, HW, int(T), Cc, H, float(eps), _lib.current_stream_ptr()), None, "agd_op_xattn_scores")
    return P


def ipa_cols(heads, nt):
    """heads * nt padded to a multiple of 16: the column count of the IP-Adapter's pre-multiplied matrices"""
    return (int(heads) * int(nt) + 15) // 16 * 16


def ipa_linear(x, w, bias=None):
    """`ipa_linear_kernel` (agd_op_ipa_linear): fp32 rows x [R, K] against bf16(w [N, K]) (+ bias) -> [R, N] fp32"""
    lib = _lib.load()
    x, w = _f32c(x), _f32c(w)
    R, K = x.shape
    N = w.shape[0]
    y = torch.empty(R, N, device=x.device, dtype=torch.float32)
    _lib.check(lib.agd_op_ipa_linear(_lib.ptr(x), _lib.ptr(w), _lib.ptr(None if bias is None else _f32c(bias)), _lib.ptr(y), R, N, K, _lib.current_stream_ptr()),
               None, "agd_op_ipa_linear")
    return y


def ipa_layernorm(x, gamma, beta, eps=1e-5):
    """`ipa_layernorm_kernel` (agd_op_ipa_layernorm): fp32 LayerNorm of the rows of x [rows, C]"""
    lib = _lib.load()
    x = _f32c(x)
    rows, Cc = x.shape
    y = torch.empty_like(x)
    _lib.check(lib.agd_op_ipa_layernorm(_lib.ptr(x), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)), _lib.ptr(y), rows, Cc, float(eps), _lib.current_stream_ptr()),
               None, "agd_op_ipa_layernorm")
    return y


def ipa_context(kip, vip, wq, wo, gamma, beta, heads, *, cols=None):
    """The IP-Adapter's context products (agd_op_ipa_context: the Wq . beta mat-vec and launch_ipa_premul): kip / vip [B, nt, C] fp32 ->
    (kpp [B, colsP, C], cs [B, colsP], bs [B, colsP], vpp [B, C, colsP]) with colsP = heads * nt padded to 16 (cols: another count, to be refused)."""
    lib = _lib.load()
    kip, vip = _f32c(kip), _f32c(vip)
    B, nt, Cc = kip.shape
    colsP = ipa_cols(heads, nt) if cols is None else int(cols)
    dev = kip.device
    kpp = torch.empty(B, colsP, Cc, device=dev, dtype=torch.float32)
    cs = torch.empty(B, colsP, device=dev, dtype=torch.float32)
    bs = torch.empty_like(cs)
    vpp = torch.empty(B, Cc, colsP, device=dev, dtype=torch.float32)
    _lib.check(lib.agd_op_ipa_context(_lib.ptr(kip), _lib.ptr(vip), _lib.ptr(_f32c(wq)), _lib.ptr(_f32c(wo)), _lib.ptr(_f32c(gamma)), _lib.ptr(_f32c(beta)),
                                      _lib.ptr(kpp), _lib.ptr(cs), _lib.ptr(bs), _lib.ptr(vpp), B, Cc, int(heads), nt, colsP, _lib.current_stream_ptr()),
               None, "agd_op_ipa_context")
    return kpp, cs, bs, vpp


IPA_SENTINEL = -24576.0          # exact in bf16: what `ipa_scores` / `ipa_add` fill the guard rows with


def ipa_scores(h, kpp, cs, bs, heads, nt, eps=1e-5, *, out=None, guard_rows=0):
    """`ipa_scores_kernel` (agd_op_ipa_scores): h [B, HW, C], kpp [B, colsP, C], cs / bs [B, colsP] -> P [B, HW, colsP].  out: the caller's
    [B * HW + guard_rows, colsP] fp32 buffer (bf16 values) the kernel writes into; without it one is made, filled with IPA_SENTINEL, and returned
    whole when guard_rows > 0."""
    lib = _lib.load()
    h, kpp, cs, bs = _f32c(h), _f32c(kpp), _f32c(cs), _f32c(bs)
    B, HW, Cc = h.shape
    colsP = kpp.shape[1]
    assert kpp.shape == (B, colsP, Cc) and cs.shape == (B, colsP) and bs.shape == cs.shape, "kpp [B, colsP, C], cs / bs [B, colsP]"
    if out is None:
        out = torch.full((B * HW + guard_rows, colsP), IPA_SENTINEL, device=h.device, dtype=torch.float32)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == (B * HW + guard_rows, colsP), "out [B * HW + guard_rows, colsP]"
    _lib.check(lib.agd_op_ipa_scores(_lib.ptr(h), _lib.ptr(kpp), _lib.ptr(cs), _lib.ptr(bs), _lib.ptr(out), B, HW, Cc, int(heads), int(nt), colsP, float(eps),
                                     int(guard_rows), _lib.current_stream_ptr()), None, "agd_op_ipa_scores")
    return out if guard_rows else out.reshape(B, HW, colsP)


def ipa_add(h, P, vpp, s, *, guard_rows=0):
    """`ipa_add_kernel` (agd_op_ipa_add): h' = bf16(h + s P V''^T) on a copy of h [B, HW, C]; P [B, HW, colsP], vpp [B, C, colsP].  With guard_rows
    the copy has that many rows of IPA_SENTINEL behind it and comes back whole, [B * HW + guard_rows, C]."""
    lib = _lib.load()
    h, P, vpp = _f32c(h), _f32c(P), _f32c(vpp)
    B, HW, Cc = h.shape
    colsP = P.shape[-1]
    assert P.shape == (B, HW, colsP) and vpp.shape == (B, Cc, colsP), "P [B, HW, colsP], vpp [B, C, colsP]"
    buf = torch.full((B * HW + guard_rows, Cc), IPA_SENTINEL, device=h.device, dtype=torch.float32)
    buf[:B * HW] = h.reshape(B * HW, Cc)
    _lib.check(lib.agd_op_ipa_add(_lib.ptr(buf), _lib.ptr(P), _lib.ptr(vpp), B, HW, Cc, colsP, float(s), int(guard_rows), _lib.current_stream_ptr()),
               None, "agd_op_ipa_add")
    return buf if guard_rows else buf.reshape(B, HW, Cc)


def _given(t):
    """a tensor to hand over even when it is empty (an empty tensor has a null data pointer): the library refuses the shape, by name"""
    t = _f32c(t)
    return t if t.numel() else torch.zeros(1, device=t.device, dtype=torch.float32)


def attention(q, k, v, heads, scale=None, return_probs=False, *, causal=False, mask=None, k2=None, v2=None, layout=0, head_sum=False,
              rec_b0=0, rec_T=None):
    """q [B,Nq,H*D], k/v [B,Nk,H*D] -> o [B,Nq,H*D] (+ probs [B,H,Nk,Nq] token-major if asked, Nk<=96).

    The keyword arguments reach the other forms of the kernel (`agd_op_attention_ex`); without them the call is what it always was.
    causal: key j is seen by queries i >= j.  mask: additive [B,Nk], broadcast over heads and queries.  k2 / v2 [B,Nk2,H*D]: a second
    K/V source of 1..64 keys attended after the Nk keys.  layout: 0 packed operands, 1 q|k|v as column blocks of one [B,N,3C] buffer
    (Nq == Nk), 2 k|v as column blocks of one [B,Nk,2C] buffer -- built by the library from the same packed tensors.  With return_probs:
    head_sum gives the probabilities summed over the heads, [B,Nk,Nq]; only batch rows >= rec_b0 and token rows < rec_T (default Nk)
    are recorded, the rest of probs stays zero."""
    lib = _lib.load()
    q, k, v = _f32c(q), _f32c(k), _f32c(v)
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    D = Cc // heads
    scale = D ** -0.5 if scale is None else scale
    o = torch.empty_like(q)
    if causal or mask is not None or k2 is not None or v2 is not None or layout != 0 or head_sum or rec_b0 != 0 or rec_T is not None:
        if k.shape != (B, Nk, Cc) or v.shape != k.shape:
            raise ValueError(f"attention: k {tuple(k.shape)} / v {tuple(v.shape)} must both be [B, Nk, H*D] = [{B}, Nk, {Cc}]")
        if mask is not None and tuple(mask.shape) != (B, Nk):
            raise ValueError(f"attention: mask {tuple(mask.shape)} must be {(B, Nk)}")
        if (k2 is None) != (v2 is None) or (k2 is not None and (k2.shape != v2.shape or k2.ndim != 3 or k2.shape[0] != B or k2.shape[2] != Cc)):
            raise ValueError("attention: k2 and v2 come together, both [B, Nk2, H*D]")
        if head_sum and not return_probs:
            raise ValueError("attention: head_sum is a form of return_probs")
        Nk2 = 0 if k2 is None else k2.shape[1]
        probs = None
        if return_probs:       # an empty key axis would make this a null pointer: keep one element, the library refuses Nk < 1 by name
            probs = torch.empty((B, max(Nk, 1), max(Nq, 1)) if head_sum else (B, heads, max(Nk, 1), max(Nq, 1)), device=q.device, dtype=torch.float32)
        _lib.check(lib.agd_op_attention_ex(_lib.ptr(_given(q)), _lib.ptr(_given(k)), _lib.ptr(_given(v)), _lib.ptr(_given(o)), B, heads, D, Nq, Nk, float(scale),
                                           int(bool(causal)), _lib.ptr(None if mask is None else _given(mask)),
                                           _lib.ptr(None if k2 is None else _given(k2)), _lib.ptr(None if v2 is None else _given(v2)), Nk2, int(layout),
                                           _lib.ptr(probs), (2 if head_sum else 1) if return_probs else 0, int(rec_b0),
                                           Nk if rec_T is None else int(rec_T), _lib.current_stream_ptr()), None, "agd_op_attention_ex")
        return (o, probs) if return_probs else o
    probs = torch.empty(B, heads, Nk, Nq, device=q.device, dtype=torch.float32) if return_probs else None
    _lib.check(lib.agd_op_attention(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), B, heads, D, Nq, Nk, float(scale),
                                    _lib.ptr(probs), _lib.current_stream_ptr()), None, "agd_op_attention")
    return (o, probs) if return_probs else o


def attention_long(q, k, v, heads, scale=None, *, layout=0, rec_b0=0, rec_T=None, probs=None):
    """The recording kernel for 97..320 keys alone (`agd_op_attention_long`, csrc/attention_long.hip): q [B,Nq,H*D], k/v [B,Nk,H*D] ->
    (o [B,Nq,H*D], probs [B,H,Nk,Nq]).  layout 0 packed, 2 k|v as column blocks of one [B,Nk,2C] buffer.  Only batch rows >= rec_b0 and
    token rows < rec_T (default Nk) are recorded.  The kernel ADDS, as it does into the DAAM accumulators: `probs` given = added to in
    place, else a zeroed tensor."""
    lib = _lib.load()
    q, k, v = _f32c(q), _f32c(k), _f32c(v)
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    if k.shape != (B, Nk, Cc) or v.shape != k.shape:
        raise ValueError(f"attention_long: k {tuple(k.shape)} / v {tuple(v.shape)} must both be [B, Nk, H*D] = [{B}, Nk, {Cc}]")
    D = Cc // heads
    scale = D ** -0.5 if scale is None else scale
    o = torch.empty_like(q)
    if probs is None:
        probs = torch.zeros(B, heads, max(Nk, 1), max(Nq, 1), device=q.device, dtype=torch.float32)
    elif tuple(probs.shape) != (B, heads, Nk, Nq) or probs.dtype != torch.float32 or not probs.is_contiguous() or not probs.is_cuda:
        raise ValueError(f"attention_long: probs must be a contiguous fp32 GPU tensor {(B, heads, Nk, Nq)}")
    _lib.check(lib.agd_op_attention_long(_lib.ptr(_given(q)), _lib.ptr(_given(k)), _lib.ptr(_given(v)), _lib.ptr(_given(o)), B, heads, D, Nq, Nk,
                                         float(scale), int(layout), _lib.ptr(probs), int(rec_b0), Nk if rec_T is None else int(rec_T),
                                         _lib.current_stream_ptr()), None, "agd_op_attention_long")
    return o, probs


def attention_headsum(q, k, v, heads, scale=None):
    """As `attention(..., return_probs=True)` with the probabilities summed over the heads: probs [B,Nk,Nq] (Nk<=96) -- the form
    the daam recorder keeps for the layers at latent resolution."""
    lib = _lib.load()
    q, k, v = _f32c(q), _f32c(k), _f32c(v)
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    D = Cc // heads
    scale = D ** -0.5 if scale is None else scale
    o = torch.empty_like(q)
    probs = torch.empty(B, Nk, Nq, device=q.device, dtype=torch.float32)
    _lib.check(lib.agd_op_attention_headsum(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(o), B, heads, D, Nq, Nk, float(scale),
                                            _lib.ptr(probs), _lib.current_stream_ptr()), None, "agd_op_attention_headsum")
    return o, probs


def attention_backward(q, kv, heads, d_o=None, d_map=None, b0=0, scale=None):
    """The attention backward of the training seam (train.hip) in isolation: q [B,N,H*D], kv [B,T,2*H*D] (K columns then V columns),
    d_o [B,N,H*D] = gradient of the per-head attention output (before to_out), d_map [B-b0,T,N] = gradient of the head-mean map of
    batch rows >= b0 -> (dq [B,N,H*D], dkv [B,T,2*H*D]), the gradient of sum(O * d_o) + sum(map[b0:] * d_map).  Operands are rounded
    to bf16; the outputs are the bf16 results as fp32.  The library refuses unsupported head dims / key counts / b0 and two absent gradients."""
    lib = _lib.load()
    q, kv = _f32c(q), _f32c(kv)
    if q.ndim != 3 or kv.ndim != 3 or kv.shape[0] != q.shape[0] or q.shape[2] % heads or kv.shape[2] != 2 * q.shape[2]:
        raise ValueError(f"attention_backward: q {tuple(q.shape)} / kv {tuple(kv.shape)} must be [B, N, H*D] / [B, T, 2*H*D] with H = {heads}")
    B, N, Cc = q.shape
    T = kv.shape[1]
    D = Cc // heads
    scale = D ** -0.5 if scale is None else scale
    do = _f32c(d_o) if d_o is not None else None
    dm = _f32c(d_map) if d_map is not None else None
    if do is not None and do.shape != q.shape:
        raise ValueError(f"attention_backward: d_o {tuple(do.shape)} must match q {tuple(q.shape)}")
    if dm is not None and 0 <= b0 <= B:
        if tuple(dm.shape) != (B - b0, T, N):
            raise ValueError(f"attention_backward: d_map {tuple(dm.shape)} must be {(B - b0, T, N)}")
        if dm.numel() == 0:                  # b0 == B: given but empty -- still a valid pointer, the kernel's `b >= b0` keeps every row out
            dm = torch.zeros(1, device=q.device, dtype=torch.float32)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    _lib.check(lib.agd_op_attention_backward(_lib.ptr(q), _lib.ptr(kv), _lib.ptr(do), _lib.ptr(dm), int(b0), B, heads, D, N, T, float(scale),
                                             _lib.ptr(dq), _lib.ptr(dkv), _lib.current_stream_ptr()), None, "agd_op_attention_backward")
    return dq, dkv


def hook_headmean(heads):
    """hook.py:55 `maps.mean(dim=1)`, the production kernel: heads [Bp, H, T, N] -> [Bp, T, N], the heads summed in order times 1/H."""
    lib = _lib.load()
    heads = _f32c(heads)
    if heads.ndim != 4:
        raise ValueError(f"hook_headmean: heads {tuple(heads.shape)} must be [Bp, H, T, N]")
    Bp, H, T, N = heads.shape
    out = torch.empty(Bp, T, N, device=heads.device, dtype=torch.float32)
    _lib.check(lib.agd_op_hook_headmean(_lib.ptr(heads), Bp, H, T, N, _lib.ptr(out), _lib.current_stream_ptr()), None, "agd_op_hook_headmean")
    return out


def bicubic_clamp_mean(maps, out_side):
    """maps [n_maps, T, side, side] -> mean_n clamp(bicubic(maps[n]), 0) : [T, S, S]"""
    lib = _lib.load()
    maps = _f32c(maps)
    n, T, side, _ = maps.shape
    out = torch.empty(T, out_side, out_side, device=maps.device, dtype=torch.float32)
    _lib.check(lib.agd_op_bicubic_clamp_mean(_lib.ptr(maps), n, T, side, out_side, _lib.ptr(out),
                                             _lib.current_stream_ptr()), None, "agd_op_bicubic_clamp_mean")
    return out


def attn_reg_loss(attn_map: torch.Tensor, obj_idx, fg_idx, bg_idx, coef: float, want_grad: bool = True):
    """finetune_sd_token.py:1046-1066 on one recorded map [B, T, h, w] (cuda fp32): returns (loss [B, 2] = {bg, fg} per sample,
    d_map [B, T, h, w] or None).  `*_idx`: int sequences / tensors of length B; obj < 0 skips the sample."""
    lib = _lib.load()
    m = attn_map.detach().to(torch.float32).contiguous()
    assert m.is_cuda and m.ndim == 4
    B, T = m.shape[:2]
    P = m.shape[2] * m.shape[3]
    host = [torch.as_tensor(list(map(int, i)) if not torch.is_tensor(i) else i.detach().cpu(), dtype=torch.int32) for i in (obj_idx, fg_idx, bg_idx)]
    has = host[0] >= 0
    # the reference indexes the map's token rows directly (finetune_sd_token.py:1049-1060): a row the map does not have is an
    # IndexError there, never a silently skipped sample (only obj < 0 means "no object in this sample")
    if bool(has.any()):
        worst = max(int(h[has].max()) for h in host)
        if worst >= T:
            raise IndexError(f"index {worst} is out of bounds for dimension 0 with size {T}")
    idx = [h.to(m.device).contiguous() for h in host]
    loss = torch.empty(B, 2, device=m.device, dtype=torch.float32)
    dmap = torch.empty_like(m) if want_grad else None
    _lib.check(lib.agd_op_attn_reg_loss(_lib.ptr(m), B, T, P, _lib.ptr(idx[0]), _lib.ptr(idx[1]), _lib.ptr(idx[2]), float(coef), _lib.ptr(loss),
                                        _lib.ptr(dmap), _lib.current_stream_ptr()), None, "agd_op_attn_reg_loss")
    return loss, dmap


def conv_groupnorm(x, w, bias, gamma, beta, groups=32, eps=1e-5, silu=True, fused=True, p8=0):
    """conv3x3 -> GroupNorm(+SiLU) chained like the graph walk; `fused`: GroupNorm statistics from the conv launch's epilogue."""
    lib = _lib.load()
    x, w = _f32c(x), _f32c(w)
    b = _f32c(bias) if bias is not None else None
    ga, be = _f32c(gamma), _f32c(beta)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    y = torch.empty(B, Cout, H, W, device=x.device, dtype=torch.float32)
    _lib.check(lib.agd_op_conv_groupnorm(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(ga), _lib.ptr(be), _lib.ptr(y), B, Cin, H, W, Cout,
                                         groups, float(eps), int(silu), int(fused) | _P8[p8], _lib.current_stream_ptr()), None, "agd_op_conv_groupnorm")
    return y


def window_gather(canvas, window, stride=8, v0=0, n=None):
    """MultiDiffusion views of a canvas [B, C, Lh, Lw]: views [v0, v0 + n) of every panorama as [B * n, C, window, window]
    (view-major within a panorama; diffusers get_views order)."""
    lib = _lib.load()
    canvas = _f32c(canvas)
    B, Cc, Lh, Lw = canvas.shape
    V = max((Lh - window) // stride + 1, 0) * max((Lw - window) // stride + 1, 0)
    n = max(V - v0, 0) if n is None else n
    out = torch.empty(B * n, Cc, window, window, device=canvas.device, dtype=torch.float32)
    _lib.check(lib.agd_op_window_gather(_lib.ptr(canvas), _lib.ptr(out), B, Cc, Lh, Lw, window, stride, v0, n, _lib.current_stream_ptr()), None,
               "agd_op_window_gather")
    return out


def window_mean(views, batch, Lh, Lw, stride=8):
    """The overlap mean: views [B * V, C, window, window] -> canvas [B, C, Lh, Lw], each element the sum of its covering views in view
    order divided by their number."""
    lib = _lib.load()
    views = _f32c(views)
    _, Cc, window, _ = views.shape
    out = torch.empty(batch, Cc, Lh, Lw, device=views.device, dtype=torch.float32)
    V = ((Lh - window) // stride + 1) * ((Lw - window) // stride + 1)
    if views.shape[0] != batch * V:
        raise ValueError(f"window_mean: {views.shape[0]} views for {batch} canvases of {V} views")
    _lib.check(lib.agd_op_window_mean(_lib.ptr(views), _lib.ptr(out), batch, Cc, Lh, Lw, window, stride, _lib.current_stream_ptr()), None,
               "agd_op_window_mean")
    return out


def region_masks(pixel_masks, batch, Lh, Lw, regions=None):
    """Region-based MultiDiffusion's mask front end: pixel masks [R - 1, H, W] (shared by the images) or [B, R - 1, H, W], uint8 (set: > 127)
    or float (set: > 0.5; bool counts as uint8 0 / 255) -> latent masks fp32 [R, B, Lh, Lw], nearest-sampled, row 0 the background
    max(0, 1 - sum of the others).  `pixel_masks` None (with regions=1): the background alone."""
    lib = _lib.load()
    if pixel_masks is None:
        R, H, W, px, f32, per = int(regions or 1), 0, 0, None, 0, 0
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        px = pixel_masks.detach()
        assert px.is_cuda, "ops run on the GPU only (no CPU fallback)"
        if px.dtype == torch.bool:
            px = px.to(torch.uint8) * 255
        elif px.dtype != torch.uint8:
            px = px.to(torch.float32)
        px = px.contiguous()
        if px.ndim not in (3, 4) or (px.ndim == 4 and px.shape[0] != batch):
            raise ValueError(f"region_masks: masks {tuple(px.shape)} must be [R - 1, H, W] or [{batch}, R - 1, H, W]")
        per, (n, H, W) = int(px.ndim == 4), px.shape[-3:]
        R, f32, dev = n + 1, int(px.dtype == torch.float32), px.device
        if regions is not None and regions != R:
            raise ValueError(f"region_masks: {n} masks for {regions} regions")
    out = torch.empty(R, batch, Lh, Lw, device=dev, dtype=torch.float32)
    _lib.check(lib.agd_op_region_masks(_lib.ptr(px), f32, per, _lib.ptr(out), R, batch, H, W, Lh, Lw, _lib.current_stream_ptr()), None,
               "agd_op_region_masks")
    return out


def region_spread(canvas, masks, noise=None, backgrounds=None, idx=None, sa=0.0, sb=0.0):
    """Region-based MultiDiffusion's spread: canvas [B, C, Lh, Lw], masks [R, B, Lh, Lw] -> x [R * B, C, Lh, Lw] (row r * B + p).  idx None: a
    step past the bootstrapping phase, every region is the canvas.  Else idx holds R - 1 indices into backgrounds [N, C, Lh, Lw] and
    x[r] = canvas m + (sa backgrounds[idx[r - 1]] + sb noise) (1 - m) for r >= 1; region 0 is the canvas."""
    lib = _lib.load()
    canvas, masks = _f32c(canvas), _f32c(masks)
    B, Cc, Lh, Lw = canvas.shape
    R = masks.shape[0]
    if tuple(masks.shape) != (R, B, Lh, Lw):
        raise ValueError(f"region_spread: masks {tuple(masks.shape)} for a canvas {tuple(canvas.shape)}")
    ci, nbg = None, 0
    if idx is not None:
        noise, backgrounds = _f32c(noise), _f32c(backgrounds)
        idx = [int(i) for i in idx]
        if len(idx) != R - 1 or tuple(noise.shape) != tuple(canvas.shape) or tuple(backgrounds.shape[1:]) != (Cc, Lh, Lw):
            raise ValueError(f"region_spread: {len(idx)} indices, noise {tuple(noise.shape)}, backgrounds {tuple(backgrounds.shape)} for {R} regions "
                             f"of a canvas {tuple(canvas.shape)}")
        import ctypes
        ci, nbg = (ctypes.c_int * max(len(idx), 1))(*idx), backgrounds.shape[0]
    out = torch.empty(R * B, Cc, Lh, Lw, device=canvas.device, dtype=torch.float32)
    _lib.check(lib.agd_op_region_spread(_lib.ptr(canvas), _lib.ptr(out), _lib.ptr(masks), _lib.ptr(noise) if idx is not None else None,
                                        _lib.ptr(backgrounds) if idx is not None else None, R, B, Cc, Lh, Lw, nbg, ci, float(sa), float(sb),
                                        _lib.current_stream_ptr()), None, "agd_op_region_spread")
    return out


def region_mean(x, masks):
    """Region-based MultiDiffusion's masked mean: x [R * B, C, Lh, Lw] (row r * B + p), masks [R, B, Lh, Lw] -> canvas [B, C, Lh, Lw],
    sum_r m_r x_r / sum_r m_r in ascending r (0 where no mask covers the element)."""
    lib = _lib.load()
    x, masks = _f32c(x), _f32c(masks)
    R, B, Lh, Lw = masks.shape
    if x.ndim != 4 or x.shape[0] != R * B or tuple(x.shape[2:]) != (Lh, Lw):
        raise ValueError(f"region_mean: x {tuple(x.shape)} for masks {tuple(masks.shape)}")
    out = torch.empty(B, x.shape[1], Lh, Lw, device=x.device, dtype=torch.float32)
    _lib.check(lib.agd_op_region_mean(_lib.ptr(x), _lib.ptr(masks), _lib.ptr(out), R, B, x.shape[1], Lh, Lw, _lib.current_stream_ptr()), None,
               "agd_op_region_mean")
    return out


def freeu(hidden, skip, b, s):
    """FreeU on one resnet's inputs, the production kernel: hidden [B, Ch, H, W] with its first Ch // 2 channels times b, skip [B, Cs, H, W]
    with the four lowest frequencies of every map times s (diffusers fourier_filter, threshold 1).  Inputs are rounded to bf16; the outputs
    are the bf16 results as fp32 (b == 1 / s == 1: the rounded input itself)."""
    lib = _lib.load()
    hidden, skip = _f32c(hidden), _f32c(skip)
    B, Ch, H, W = hidden.shape
    if skip.ndim != 4 or skip.shape[0] != B or tuple(skip.shape[2:]) != (H, W):
        raise ValueError(f"freeu: hidden {tuple(hidden.shape)} and skip {tuple(skip.shape)} must share batch and map size")
    ho, so = torch.empty_like(hidden), torch.empty_like(skip)
    _lib.check(lib.agd_op_freeu(_lib.ptr(hidden), _lib.ptr(skip), _lib.ptr(ho), _lib.ptr(so), B, Ch, skip.shape[1], H, W, float(b), float(s),
                                _lib.current_stream_ptr()), None, "agd_op_freeu")
    return ho, so


def guidance_rescale(eps, channels, guidance, phi):
    """The guidance_rescale factor of every image, the production kernel: eps [2B, HW, ldc] fp32 as the step kernels read it (rows [0, B)
    unconditional, [B, 2B) conditional; only channels < `channels` of each ldc-wide row count) -> [B] fp32,
    f_b = 1 + phi (std(eps_c[b]) / std(m[b]) - 1) with m = eps_u + guidance (eps_c - eps_u) and the unbiased std over all of an image."""
    lib = _lib.load()
    eps = _f32c(eps)
    if eps.ndim != 3 or eps.shape[0] % 2 or eps.shape[0] < 2:
        raise ValueError(f"guidance_rescale: eps {tuple(eps.shape)} must be [2B, HW, ldc]")
    B2, HW, ldc = eps.shape
    out = torch.empty(B2 // 2, dtype=torch.float32, device=eps.device)
    _lib.check(lib.agd_op_guidance_rescale(None, _lib.ptr(eps), ldc, B2 // 2, int(channels), HW, float(guidance), float(phi), _lib.ptr(out),
                                           _lib.current_stream_ptr()), None, "agd_op_guidance_rescale")
    return out


def pag_v_rows(qkv):
    """The "attention" of a perturbed self-attention layer, the production kernel: qkv bf16 [M, 3C] (the fused q | k | v rows) -> bf16 [M, C],
    the value third of every row, bit for bit.  C % 8 != 0 is refused."""
    lib = _lib.load()
    assert qkv.is_cuda and qkv.dtype == torch.bfloat16, "ops run on the GPU only (no CPU fallback); pag_v_rows takes bf16 rows"
    qkv = qkv.detach().contiguous()
    if qkv.ndim != 2 or qkv.shape[1] % 3:
        raise ValueError(f"pag_v_rows: qkv {tuple(qkv.shape)} must be [M, 3C]")
    M, C = qkv.shape[0], qkv.shape[1] // 3
    out = torch.empty(M, C, dtype=torch.bfloat16, device=qkv.device)
    _lib.check(lib.agd_op_pag_v_rows(None, _lib.ptr(qkv), _lib.ptr(out), M, C, _lib.current_stream_ptr()), None, "agd_op_pag_v_rows")
    return out


def pag_fold(eps, p):
    """The Perturbed-Attention Guidance fold, the production kernel: eps fp32 [3, n] (uncond | cond | perturbed) -> a folded copy whose rows
    0 and 1 are e_u + d and e_c + d with d = p (e_c - e_p); row 2 is unchanged."""
    lib = _lib.load()
    eps = _f32c(eps).clone()
    if eps.ndim != 2 or eps.shape[0] != 3:
        raise ValueError(f"pag_fold: eps {tuple(eps.shape)} must be [3, n]")
    _lib.check(lib.agd_op_pag_fold(None, _lib.ptr(eps), eps.shape[1], float(p), _lib.current_stream_ptr()), None, "agd_op_pag_fold")
    return eps


def _sega_rows(eps, B, K):
    eps = _f32c(eps)
    if eps.ndim != 3 or eps.shape[0] != (2 + K) * B or eps.shape[2] != 4:
        raise ValueError(f"sega: eps {tuple(eps.shape)} must be [(2 + K) B, HW, 4] = [{(2 + K) * B}, HW, 4] (NHWC rows: uncond | cond | concepts)")
    return eps


def sega_threshold(eps, B, coef, q):
    """The Semantic Guidance threshold, the production kernel: eps fp32 [(2 + K) B, HW, 4] (uncond x B | cond x B | concept_k x B), coef [K]
    (this evaluation's sign * scale, 0 = inactive: the concept's rows are not read, thr = 0) and q [K] in [0, 1] -> thr fp32 [B, K, 4], the
    exact q-quantile of |(e_k - e_u) coef_k| over the HW pixels per image, concept and channel."""
    import ctypes as C
    lib = _lib.load()
    K = len(coef)
    eps = _sega_rows(eps, B, K)
    thr = torch.empty(B, K, 4, dtype=torch.float32, device=eps.device)
    _lib.check(lib.agd_op_sega_threshold(None, _lib.ptr(eps), B, K, eps.shape[1], (C.c_float * K)(*[float(c) for c in coef]),
                                         (C.c_double * K)(*[float(x) for x in q]), _lib.ptr(thr), _lib.current_stream_ptr()),
               None, "agd_op_sega_threshold")
    return thr


def sega_fold(eps, m, thr, B, coef, w_mom, w_add, add_mom, mom_scale, mom_beta):
    """The Semantic Guidance fold, the production kernel: eps fp32 [(2 + K) B, HW, 4], momentum m fp32 [B, HW, 4], thr [B, K, 4] and this
    evaluation's scalars -> (a folded copy of eps -- rows [0, 2 B) plus `added`, the concept rows as they were -- and the updated momentum)."""
    import ctypes as C
    lib = _lib.load()
    K = len(coef)
    eps = _sega_rows(eps, B, K).clone()
    m, thr = _f32c(m).clone(), _f32c(thr)
    if tuple(m.shape) != (B, eps.shape[1], 4) or tuple(thr.shape) != (B, K, 4) or len(w_mom) != K or len(w_add) != K:
        raise ValueError(f"sega_fold: m {tuple(m.shape)} must be [{B}, {eps.shape[1]}, 4], thr {tuple(thr.shape)} [{B}, {K}, 4], the weights lists of {K}")
    fl = lambda v: (C.c_float * K)(*[float(x) for x in v])  # noqa: E731
    _lib.check(lib.agd_op_sega_fold(None, _lib.ptr(eps), _lib.ptr(m), _lib.ptr(thr), B, K, eps.shape[1], fl(coef), fl(w_mom), fl(w_add),
                                    float(add_mom), float(mom_scale), float(mom_beta), _lib.current_stream_ptr()), None, "agd_op_sega_fold")
    return eps, m


def deepcache_capture(act, part=None):
    """DeepCache's capture launch, the production kernel: two device byte regions (the cached activation and its GroupNorm partial sums, any
    dtype, any byte count; `part` None or empty = the cpart_bm == 0 case, one region) -> bit-for-bit copies (act_copy, part_copy) made by ONE
    launch.  The copies are allocated with 64 guard bytes behind each, returned as well so a test can see they were left alone."""
    lib = _lib.load()
    assert act.is_cuda and (part is None or part.is_cuda), "ops run on the GPU only (no CPU fallback)"
    regions, outs = [], []
    for t in (act, part):
        if t is None or t.numel() == 0:
            regions.append((None, None, 0))
            outs.append(None)
            continue
        src = t.detach().contiguous().view(torch.uint8).reshape(-1)
        nb = src.numel()
        dst = torch.full(((nb + 15) // 16 * 16 + 64,), 0xA5, dtype=torch.uint8, device=src.device)
        regions.append((src, dst, nb))
        outs.append((dst[:nb].view(t.dtype).reshape(t.shape), dst[nb:]))
    (s0, d0, n0), (s1, d1, n1) = regions
    _lib.check(lib.agd_op_deepcache_capture(None, _lib.ptr(s0), _lib.ptr(d0), n0, _lib.ptr(s1), _lib.ptr(d1), n1, _lib.current_stream_ptr()),
               None, "agd_op_deepcache_capture")
    return outs[0], outs[1]
