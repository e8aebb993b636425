"""Semantic Guidance restated in torch (Brack et al. 2023; the per-step loop of diffusers 0.21.2 SemanticStableDiffusionPipeline
[upstream-knowledge], parity-unpinned, with the project's stated rules where they differ: the editing direction's sign multiplies the
direction, not the concept's weight, and the quantile is the order-statistic lerp min(b, a + f (b - a))).  Written with tensors --
concept_weights, warmup_inds, index_select, softmax, einsum -- as upstream is, not with the schedule arrays of config.sega_schedule, so the
two can be held against each other.  Any floating dtype: fp32 as the device computes, fp64 as the reference."""
import math

import numpy as np
import torch

from oracle import sd_oracle as O


def per_concept(v, K, default=None):
    v = default if v is None else v
    return list(v) if isinstance(v, (list, tuple)) else [v] * K


def rank(q, HW):
    """p = q (HW - 1) in double, lo = floor(p), f = float(p - lo) (fp32)."""
    p = float(q) * (HW - 1)
    lo = min(max(int(math.floor(p)), 0), HW - 1)
    return lo, float(np.float32(p - lo))


def quantile(absv, q):
    """absv [..., HW] -> the q-quantile over the last axis in absv's dtype, and (a, b, f): thr = min(b, a + f (b - a)) with a, b the lo-th
    and min(lo + 1, HW - 1)-th smallest values."""
    HW = absv.shape[-1]
    lo, f = rank(q, HW)
    s = absv.sort(-1).values
    a, b = s[..., lo], s[..., min(lo + 1, HW - 1)]
    return torch.minimum(b, a + f * (b - a)), a, b, f


class Sega:
    """One call's guidance: step(i, e_u, [e_k]) -> `added` (what lands on both e_u and e_c), NCHW [B, C, H, W]; the momentum is the state."""

    def __init__(self, K, reverse_editing_direction=False, edit_guidance_scale=5, edit_warmup_steps=10, edit_cooldown_steps=None,
                 edit_threshold=0.9, edit_momentum_scale=0.1, edit_mom_beta=0.4, edit_weights=None):
        self.K = K
        self.rev = per_concept(reverse_editing_direction, K, False)
        self.scale = per_concept(edit_guidance_scale, K, 5)
        self.warm = per_concept(edit_warmup_steps, K, 10)
        self.cool = per_concept(edit_cooldown_steps, K, None)
        self.q = per_concept(edit_threshold, K, 0.9)
        self.w = per_concept(edit_weights, K, 1.0)
        self.mu, self.beta = float(edit_momentum_scale), float(edit_mom_beta)
        self.m = None
        self.walks = 0
        self.last = None          # the scalars the tensors of the last step amount to (for config.sega_schedule's test)

    def step(self, i, e_u, e_ks):
        K, B, dt = self.K, e_u.shape[0], e_u.dtype
        if self.m is None:
            self.m = torch.zeros_like(e_u)
        concept_weights = torch.zeros(K, B, dtype=dt)
        edits = torch.zeros(K, *e_u.shape, dtype=dt)
        coef = torch.zeros(K, dtype=torch.float64)
        warmup_inds = []
        for c in range(K):
            if i >= self.warm[c]:
                warmup_inds.append(c)
            if self.cool[c] is not None and i >= self.cool[c]:
                continue                                       # (zeros, and a weight of 0 that keeps its share of the softmax)
            concept_weights[c] = torch.full((B,), float(self.w[c]), dtype=dt)
            cf = float(np.float32((-1.0 if self.rev[c] else 1.0) * float(self.scale[c])))
            coef[c] = cf
            if cf == 0.0:
                continue
            v = (e_ks[c] - e_u) * cf
            thr = quantile(v.abs().flatten(2), self.q[c])[0]
            edits[c] = torch.where(v.abs() >= thr[:, :, None, None], v, torch.zeros_like(v))
        if (coef != 0).any():
            self.walks += 1
        w_all = torch.softmax(concept_weights, 0)
        added = torch.zeros_like(e_u)
        w_add = torch.zeros(K, B, dtype=dt)
        if K > len(warmup_inds) > 0:
            idx = torch.tensor(warmup_inds)
            w_tmp = torch.softmax(concept_weights.index_select(0, idx), 0)
            w_tmp = w_tmp / w_tmp.sum(0)
            added = added + torch.einsum("cb,cbijk->bijk", w_tmp, edits.index_select(0, idx))
            w_add[idx] = w_tmp
        g = torch.einsum("cb,cbijk->bijk", w_all, edits) + self.mu * self.m
        self.m = self.beta * self.m + (1 - self.beta) * g
        add_mom = 0.0
        if len(warmup_inds) == K:
            added = added + g
            w_add, add_mom = w_all, 1.0
        self.last = {"coef": coef.tolist(), "w_mom": w_all[:, 0].double().tolist(), "w_add": w_add[:, 0].double().tolist(), "add_mom": add_mom}
        return added


def fold_reference(eps, m, thr, B, coef, w_mom, w_add, add_mom, mu, beta):
    """The fold in fp64 from the SAME fp32 v and the given thr: eps fp32 [(2 + K) B, HW, 4], m [B, HW, 4], thr [B, K, 4].  Returns (added,
    new m, sum_k |w_add_k G_k| -- what the pair's sum holds --, sum_k |w_mom_k G_k| -- what the momentum's holds) in fp64, and the masks
    [K, B, HW, 4]."""
    K = len(coef)
    e_u = eps[:B]
    gm = torch.zeros_like(e_u, dtype=torch.float64)
    ga, mag_add, mag_mom = gm.clone(), gm.clone(), gm.clone()
    masks = torch.zeros(K, *e_u.shape, dtype=torch.bool)
    for k in range(K):
        if coef[k] == 0.0:
            continue
        v = (eps[(2 + k) * B:(3 + k) * B] - e_u) * torch.tensor(coef[k], dtype=torch.float32)      # fp32, as the device forms it
        masks[k] = v.abs() >= thr[:, k][:, None, :]
        G = torch.where(masks[k], v, torch.zeros_like(v)).double()
        gm, ga = gm + float(w_mom[k]) * G, ga + float(w_add[k]) * G
        mag_add, mag_mom = mag_add + abs(float(w_add[k])) * G.abs(), mag_mom + abs(float(w_mom[k])) * G.abs()
    md = m.double()
    g = gm + float(mu) * md
    added = ga + float(add_mom) * float(mu) * md
    return added, float(beta) * md + (1.0 - float(beta)) * g, mag_add, mag_mom, masks


def generate(usd, vsd, cfg, ctx, latents, steps, scheduler, guidance, sega, dtype=torch.float32):
    """The oracle's UNet under Semantic Guidance, stepped by the oracle's DDIM / PNDM or the restated DPM-Solver++ 2M.  ctx [(2 + K) B, T, D]
    ordered [uncond x B | cond x B | concept_k x B]; sega: a Sega, or None for the plain loop.  Evaluation i counts the model's calls.
    Returns (latents, evaluations)."""
    import _dpm_restated as R
    s = cfg.sched
    B = latents.shape[0]
    n = [0]

    def model(x, t):
        tt = torch.as_tensor(t, dtype=torch.float32)
        e_u, e_c = O.unet_forward(usd, cfg.unet, torch.cat([x, x], 0), tt, ctx[:2 * B]).chunk(2)
        i = n[0]
        n[0] += 1
        if sega is None:
            return e_u + guidance * (e_c - e_u)
        e_ks = [O.unet_forward(usd, cfg.unet, x, tt, ctx[(2 + k) * B:(3 + k) * B]) for k in range(sega.K)]
        added = sega.step(i, e_u.to(dtype), [e.to(dtype) for e in e_ks]).to(e_u.dtype)
        return e_u + guidance * (e_c - e_u) + added

    with torch.no_grad():
        x = latents.clone().float()
        if scheduler == "dpm":
            _, x = R.sample(steps, False, s.prediction_type, lambda x_, i, t: model(x_, t), x)
        else:
            sch = (O.PNDM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one) if scheduler == "pndm" else
                   O.DDIM(s.num_train_timesteps, s.beta_start, s.beta_end, s.steps_offset, s.set_alpha_to_one, s.prediction_type))
            for t in sch.set_timesteps(steps):
                x = sch.step(model(x, float(int(t))), int(t), x)
    return x, n[0]
