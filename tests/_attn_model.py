"""What the attention tests compare the kernel with, on the CPU in fp64 (no test in here):

`attention_fp64`   the operation itself on the bf16-rounded operands: explicit softmax(scale q k^T + mask) v per head, `-inf` where causal
                   order or the mask removes a key, the keys of a second source appended.
`attention_model`  the same with the three roundings that csrc/attention.hip's comments declare and nothing else: q * (scale * log2 e)
                   in fp32 rounded to bf16 (`fold=True`: the non-recording kernels; the recording kernels keep raw logits), the
                   unnormalised probabilities rounded to bf16 before P V, the output rounded to bf16.  Its distance from `attention_fp64`
                   is the error a correct kernel is entitled to; the tests bound the kernel by twice that distance, case by case.
`slab_errors`      the measure: every (batch row, head) slab [N, D] of the output on its own -- max |error| over the slab's max |value|,
                   and RMS error over the slab's RMS -- so that no head or batch row hides behind a larger one."""
import math

import torch

LOG2E = 1.4426950408889634


def bfr(t):
    """round to bf16 and back: the values the kernels see"""
    return t.to(torch.bfloat16).float()


def _bf64(t):
    return t.float().to(torch.bfloat16).double()


def heads_of(t, H):
    """[B, N, H*D] -> [B, H, N, D] (fp64, cpu)"""
    t = t.detach().double().cpu()
    B, N, C = t.shape
    return t.view(B, N, H, C // H).permute(0, 2, 1, 3)


def _attention(q, k, v, H, scale, causal, mask, k2, v2, model, fold):
    D = q.shape[-1] // H
    scale = D ** -0.5 if scale is None else scale
    if k2 is not None:
        k, v = torch.cat([k, k2], 1), torch.cat([v, v2], 1)
        assert mask is None and not causal
    Q, K, V = heads_of(q, H), heads_of(k, H), heads_of(v, H)
    if model and fold:           # log2-domain logits from the folded q, as the kernel forms them
        qs = (torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32))
        Q = heads_of((q.float() * qs).to(torch.bfloat16).float(), H)
        L = Q @ K.transpose(-1, -2)
        unit = LOG2E
    else:
        L = (Q @ K.transpose(-1, -2)) * scale
        unit = 1.0
    if mask is not None:
        L = L + mask.double()[:, None, None, :] * unit
    if causal:
        Nq, Nk = L.shape[-2:]
        L = L.masked_fill(torch.arange(Nk)[None, :] > torch.arange(Nq)[:, None], -math.inf)
    m = L.amax(-1, keepdim=True)
    assert bool(torch.isfinite(m).all()), "a row with every key removed is unspecified"
    p = torch.exp2(L - m) if unit != 1.0 else torch.exp(L - m)
    den = p.sum(-1, keepdim=True)
    o = ((_bf64(p) if model else p) @ V) / den
    if model:
        o = _bf64(o)
    B, _, N, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, N, -1), p / den          # [B, N, C], [B, H, Nq, Nk (+ Nk2)]


def attention_fp64(q, k, v, H, scale=None, causal=False, mask=None, k2=None, v2=None):
    return _attention(q, k, v, H, scale, causal, mask, k2, v2, False, False)


def attention_model(q, k, v, H, scale=None, causal=False, mask=None, k2=None, v2=None, fold=True):
    return _attention(q, k, v, H, scale, causal, mask, k2, v2, True, fold)[0]


def slab_errors(got, want, H):
    """-> (max-measure [B, H], rms-measure [B, H]); a slab that is identically zero in the reference has no scale: refused"""
    g, w = heads_of(got, H), heads_of(want, H)
    e = g - w
    top, rms = w.abs().amax(dim=(2, 3)), w.pow(2).mean(dim=(2, 3)).sqrt()
    assert bool((top > 0).all()), "a reference slab is identically zero: the measure is undefined"
    return e.abs().amax(dim=(2, 3)) / top, e.pow(2).mean(dim=(2, 3)).sqrt() / rms


MODEL_FACTOR = 2.0          # the kernel's rounding points and summation order differ from the model's by about one more model error
MODEL_CEILING = 2.0 ** -6   # a case whose 2 x model error is above this proves too little: its inputs have to change


def model_bounds(model_o, want_o, H):
    """(E_model, E_rms): the worst slab of the rounding model against the exact reference"""
    mx, rms = slab_errors(model_o, want_o, H)
    e_model, e_rms = float(mx.max()), float(rms.max())
    assert MODEL_FACTOR * e_model <= MODEL_CEILING and MODEL_FACTOR * e_rms <= MODEL_CEILING, (e_model, e_rms)
    return e_model, e_rms
