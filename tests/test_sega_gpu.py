"""Semantic Guidance on the device: the threshold and fold kernels through their op seams against fp64, one evaluation through
agd_unet_forward_hw, whole loops against the tensor restatement (tests/_sega_restated.py) with the plain call's own error as the yardstick,
the off switch, the counters, the recorders, every refusal, and SEGA beside a LoRA, FreeU, img2img and a rectangular size.  No test here
provokes a fault: every refusal tested is a host-side status returned before any launch."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import _sega_restated as R
from _report import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 7.5                                # guidance_scale
SCALE, MU, BETA = 5.0, 0.3, 0.4        # edit_guidance_scale, edit_momentum_scale, edit_mom_beta of the loops
# Linear error propagation: with eps the error of one UNet output, the plain combine e_u + s (e_c - e_u) carries (2 s - 1) eps = 14 eps.  The
# guidance adds sum_k w_k c (e_k - e_u) with weights that sum to 1 -- 2 c eps = 10 eps -- and mu m, where m is a running mean of g and so
# carries no more than g: (1 + mu) 2 c eps = 13 eps in all.  (14 + 13) / 14 = 1.93; a margin of 2 for step-to-step amplification: 3.86 x.
LOOP_FACTOR = 2.0 * (1.0 + (1.0 + MU) * 2.0 * SCALE / (2.0 * S - 1.0))
FWD_FACTOR = 2.0                       # one forward of the concept rows: the plain forward's arithmetic under another context


def _rms_rel(got, want):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    return float(((got - want) ** 2).mean().sqrt() / ((want ** 2).mean().sqrt() + 1e-12))


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)


def _f32(x):
    return float(np.float32(x))


def _ulp(t):
    """fp32 spacing at |t| (a float64 tensor of fp32 values)."""
    return torch.from_numpy(np.spacing(np.abs(t.numpy()).astype(np.float32)).astype(np.float64))


_W = {}


def _weights(name):
    if name not in _W:
        from agenda_amd import config, synthetic
        cfg = config.CONFIGS[name]()
        small = name != "sd15"
        kw = dict(bias_std=0.05, perturb_norm=0.1) if small else {}
        _W[name] = (cfg, synthetic.make_unet_weights(cfg, 11 if small else 1234, **kw), synthetic.make_vae_weights(cfg, 12 if small else 1235, **kw))
    return _W[name]


def _pipe(name="tiny", scheduler="DDIMScheduler", **kw):
    from agenda_amd import StableDiffusionPipeline
    cfg, u, v = _weights(name)
    return StableDiffusionPipeline(cfg, u, v, workspace_bytes=(6 if name == "sd15" else 2) << 30, scheduler=scheduler, **kw)


def _contexts(cfg, B, K, seed):
    """(prompt context [2 B, T, D], concept embeddings [K, T, D], the engine's context [(2 + K) B, T, D])."""
    from agenda_amd import synthetic
    ctx = synthetic.make_context(cfg, B, seed=seed)
    emb = torch.cat([synthetic.make_context(cfg, 1, seed=seed + 100 + k)[1:2] for k in range(K)])
    return ctx, emb, torch.cat([ctx, emb.repeat_interleave(B, dim=0)])


# ---- 1. the threshold op ----------------------------------------------------------------------------------------------------------
# 1: one pixel; 64 / 81: less than one trip of the workgroup, odd; 1000: one trip, ragged; 4096: 64 x 64 latents, four trips; 9216: the
# largest slab staged in LDS; 20000: past it, re-read through L2
THR_CASES = [(1, 1, 1), (2, 3, 64), (1, 2, 81), (3, 1, 1000), (1, 2, 4096), (1, 1, 9216), (1, 1, 20000)]
QS = (0.0, 0.5, 0.9, 0.95, 1.0)
COEFS = [5.0, -7.5, 3.0]


def _slab(B, K, HW, seed, grid=None):
    eps = torch.randn((2 + K) * B, HW, 4, generator=torch.Generator().manual_seed(seed))
    return eps if grid is None else torch.round(eps / grid) * grid


def _v32(eps, B, K, coef):
    """v of every (concept, image) in fp32 as the device forms it: [K, B, HW, 4]."""
    return torch.stack([(eps[(2 + k) * B:(3 + k) * B] - eps[:B]) * torch.tensor(coef[k], dtype=torch.float32) for k in range(K)])


def _thr_reference(eps, B, K, coef, q):
    """fp64 order-statistic lerp of the fp32 |v|: thr, a, b [B, K, 4] and f."""
    av = _v32(eps, B, K, coef).abs().double().permute(1, 0, 3, 2)          # [B, K, 4, HW]
    return R.quantile(av, q)


def _condition_holds(eps, B, K, coef):
    for q in QS:
        _, a, b, f = _thr_reference(eps, B, K, coef, q)
        if f > 0 and not bool(((a == b) | (b - a >= 16 * _ulp(b))).all()):
            return False
    return True


def _seeded_slab(B, K, HW):
    """Seed 1000 B + 100 K + HW: the 16-ulp condition holds at every q for every case (asserted by the test, on the reference)."""
    eps = _slab(B, K, HW, 1000 * B + 100 * K + HW)
    assert _condition_holds(eps, B, K, COEFS[:K])
    return eps


@pytest.mark.parametrize("B,K,HW", THR_CASES, ids=[f"B{c[0]}-K{c[1]}-HW{c[2]}" for c in THR_CASES])
def test_threshold_is_the_exact_quantile(B, K, HW):
    from agenda_amd import ops
    coef = COEFS[:K]
    eps = _seeded_slab(B, K, HW)
    v = _v32(eps, B, K, coef).permute(1, 0, 2, 3)                          # [B, K, HW, 4]
    dev = eps.cuda()
    for q in QS:
        want, a, b, f = _thr_reference(eps, B, K, coef, q)
        if f > 0:                                                          # the condition, on the reference, no element left out
            assert bool(((a == b) | (b - a >= 16 * _ulp(b))).all()), (q, "seed")
        got = ops.sega_threshold(dev, B, coef, [q] * K).cpu()
        assert got.shape == (B, K, 4)
        err = ((got.double() - want).abs() / _ulp(want)).max()
        print(f"sega threshold B{B} K{K} HW{HW} q{q}: max {float(err):.2f} ulp (f = {f:.4f})")
        assert float(err) <= 4.0, (q, float(err))
        assert torch.equal(v.abs() >= got[:, :, None, :], v.abs().double() >= want[:, :, None, :]), q
        if f == 0:
            assert torch.equal(got.double(), a), q                         # an order statistic itself, exactly
        assert torch.equal(ops.sega_threshold(dev, B, coef, [q] * K).cpu(), got)          # two runs, equal bits


@pytest.mark.parametrize("B,K,HW", [(2, 3, 64), (1, 2, 4096), (1, 1, 20000)])
def test_threshold_with_ties(B, K, HW):
    """Inputs on a grid of 1/2: a few dozen distinct |v|, so every rank sits inside a run of equal values.  thr is an input value exactly
    wherever a == b, and the mask is the reference's."""
    from agenda_amd import ops
    coef = [2.0, -4.0, 1.0][:K]                                            # powers of two: v stays on the grid
    eps = _slab(B, K, HW, 7 + HW, grid=0.5)
    v = _v32(eps, B, K, coef).permute(1, 0, 2, 3)
    interior_ties = 0
    for q in QS:
        want, a, b, f = _thr_reference(eps, B, K, coef, q)
        got = ops.sega_threshold(eps.cuda(), B, coef, [q] * K).cpu()
        tie = a == b
        if 0.0 < q < 1.0:                                                  # (at q = 1 a == b by construction: lo is the last rank)
            interior_ties += int(tie.sum())
        assert torch.equal(got.double()[tie], a[tie])
        assert float(((got.double() - want).abs() / _ulp(want).clamp_min(1e-45)).max()) <= 4.0
        assert torch.equal(v.abs() >= got[:, :, None, :], v.abs().double() >= want[:, :, None, :]), q
    assert interior_ties > 0


# q (HW - 1) in double lands a few ulp below an integer, so f = float(p - lo) rounds up to exactly 1 and thr is b: 19 x 19 latents, 56 x 96
# (two concepts), 99 x 99 (past the staged size)
F1_CASES = [(1, 1, 361, 0.7), (1, 2, 5376, 0.688), (1, 1, 9801, 0.57)]


@pytest.mark.parametrize("B,K,HW,q", F1_CASES, ids=[f"HW{c[2]}-q{c[3]}" for c in F1_CASES])
def test_threshold_where_the_fraction_rounds_up_to_one(B, K, HW, q):
    from agenda_amd import ops
    lo, f = R.rank(q, HW)
    assert f == 1.0 and lo == int(q * (HW - 1)) and lo + 1 == round(q * (HW - 1))
    coef = COEFS[:K]
    eps = _slab(B, K, HW, 1000 * B + 100 * K + HW)
    v = _v32(eps, B, K, coef).permute(1, 0, 2, 3)
    want, a, b, _ = _thr_reference(eps, B, K, coef, q)
    assert bool(((a == b) | (b - a >= 16 * _ulp(b))).all()) and torch.equal(want, b)
    got = ops.sega_threshold(eps.cuda(), B, coef, [q] * K).cpu()
    err = float(((got.double() - want).abs() / _ulp(want)).max())
    print(f"sega threshold B{B} K{K} HW{HW} q{q}: max {err:.2f} ulp (f = 1)")
    assert err <= 4.0
    assert torch.equal(v.abs() >= got[:, :, None, :], v.abs().double() >= want[:, :, None, :])


def test_threshold_edge_slabs():
    from agenda_amd import _lib, ops
    B, K, HW = 2, 2, 100
    zero = torch.zeros((2 + K) * B, HW, 4)
    for q in QS:
        assert torch.equal(ops.sega_threshold(zero.cuda(), B, [5.0, 5.0], [q, q]).cpu(), torch.zeros(B, K, 4))
    # an inactive concept's rows are not read: NaN there, coef 0 -> a finite threshold, and the other concept's is what it is alone
    eps = _slab(B, K, HW, 3)
    eps[3 * B:] = float("nan")
    got = ops.sega_threshold(eps.cuda(), B, [5.0, 0.0], [0.9, 0.9]).cpu()
    assert torch.isfinite(got).all() and torch.equal(got[:, 1], torch.zeros(B, 4))
    alone = ops.sega_threshold(eps[:3 * B].cuda(), B, [5.0], [0.9]).cpu()
    assert torch.equal(got[:, 0], alone[:, 0])
    m = torch.randn(B, HW, 4, generator=torch.Generator().manual_seed(5))
    out, m2 = ops.sega_fold(eps.cuda(), m.cuda(), got.cuda(), B, [5.0, 0.0], [0.5, 0.5], [0.5, 0.5], 1.0, MU, BETA)
    assert torch.isfinite(out[:2 * B]).all() and torch.isfinite(m2).all()
    clean = eps.clone()
    clean[3 * B:] = 0.0
    out2, m3 = ops.sega_fold(clean.cuda(), m.cuda(), got.cuda(), B, [5.0, 0.0], [0.5, 0.5], [0.5, 0.5], 1.0, MU, BETA)
    assert torch.equal(out[:2 * B], out2[:2 * B]) and torch.equal(m2, m3)            # G of the inactive concept is 0, whatever its rows hold
    for bad, msg in ((dict(q=[1.5, 0.5]), "quantile"), (dict(coef=[float("nan"), 1.0]), "coef")):
        with pytest.raises(_lib.AgendaHipError, match=msg):
            ops.sega_threshold(zero.cuda(), B, bad.get("coef", [5.0, 5.0]), bad.get("q", [0.9, 0.9]))
    with pytest.raises(ValueError, match="NHWC"):
        ops.sega_threshold(torch.zeros(8, HW, 8).cuda(), B, [5.0, 5.0], [0.9, 0.9])


# ---- 2. the fold op ---------------------------------------------------------------------------------------------------------------
def _fold_bound(K, mag, mu, m, e):
    return (K + 4) * 2.0 ** -24 * (mag + (abs(mu) * m.double().abs()) + e.double().abs())


def _check_fold(eps, m, thr, B, coef, w_mom, w_add, add_mom, mu, beta, got_eps, got_m):
    K = len(coef)
    added, m_want, mag_add, mag_mom, masks = R.fold_reference(eps, m, thr, B, coef, w_mom, w_add, add_mom, mu, beta)
    worst = 0.0
    for half in range(2):                                                  # the pair: w_k = w_add[k], what its sum holds
        e = eps[half * B:(half + 1) * B]
        err = (got_eps[half * B:(half + 1) * B].double() - (e.double() + added)).abs()
        bound = _fold_bound(K, mag_add, mu, m, e)
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), ("pair", half, float((err / bound.clamp_min(1e-300)).max()))
    if got_m is not None:                                                  # the momentum: w_k = w_mom[k]
        err = (got_m.double() - m_want).abs()
        bound = _fold_bound(K, mag_mom, mu, m, eps[:B])
        assert bool((err <= bound).all()), ("momentum", float((err / bound.clamp_min(1e-300)).max()))
    assert torch.equal(got_eps[2 * B:], eps[2 * B:])                        # the concept rows, bit for bit
    # exact masks: where no concept's mask is on and no momentum is added, the pair is untouched
    off = ~masks.any(0)
    if add_mom == 0.0 or mu == 0.0 or not bool(m.any()):
        assert torch.equal(got_eps[:B][off], eps[:B][off]) and torch.equal(got_eps[B:2 * B][off], eps[B:2 * B][off])
    return worst


FOLD_CASES = [(1, 1, 1), (2, 3, 64), (1, 2, 81), (3, 1, 1000), (1, 8, 4096)]


@pytest.mark.parametrize("B,K,HW", FOLD_CASES, ids=[f"B{c[0]}-K{c[1]}-HW{c[2]}" for c in FOLD_CASES])
def test_fold_matches_fp64(B, K, HW):
    """Against fp64 from the same fp32 v and the given thr; per element (K + 4) 2^-24 (sum_k |w_k G_k| + |mu m| + |e|), the momentum to the
    same bound, the concept rows untouched."""
    from agenda_amd import ops
    g = torch.Generator().manual_seed(B * 100 + K * 10 + HW)
    eps = torch.randn((2 + K) * B, HW, 4, generator=g)
    m = torch.randn(B, HW, 4, generator=g)
    coef = [_f32(c) for c in ([5.0, -7.5, 3.0, 0.0, 2.5, -1.0, 6.0, 4.0][:K])]
    thr = R.quantile(_v32(eps, B, K, coef).abs().permute(1, 0, 3, 2), 0.7)[0].float().contiguous()       # [B, K, 4]
    w = torch.softmax(torch.randn(K, generator=g).double(), 0)
    w_mom = [_f32(x) for x in w]
    mu, beta = _f32(MU), _f32(BETA)
    for tag, w_add, add_mom in (("all", w_mom, 1.0), ("some", [w_mom[k] * (k % 2 == 0) for k in range(K)], 0.0), ("none", [0.0] * K, 0.0)):
        got_eps, got_m = ops.sega_fold(eps.cuda(), m.cuda(), thr.cuda(), B, coef, w_mom, w_add, add_mom, mu, beta)
        worst = _check_fold(eps, m, thr, B, coef, w_mom, w_add, add_mom, mu, beta, got_eps.cpu(), got_m.cpu())
        print(f"sega fold B{B} K{K} HW{HW} {tag}: worst error / bound {worst:.3f}")
        again = ops.sega_fold(eps.cuda(), m.cuda(), thr.cuda(), B, coef, w_mom, w_add, add_mom, mu, beta)
        assert torch.equal(again[0], got_eps) and torch.equal(again[1], got_m)
    # the all-zero schedule: the pair bit for bit (a zero is not added: -0 stays -0), the momentum decays
    eps[0, 0, 0] = -0.0
    got_eps, got_m = ops.sega_fold(eps.cuda(), m.cuda(), thr.cuda(), B, [0.0] * K, w_mom, [0.0] * K, 0.0, 0.0, beta)
    assert torch.equal(got_eps.cpu().view(torch.int32), eps.view(torch.int32))
    assert torch.equal(got_m.cpu(), torch.tensor(beta) * m + (1 - torch.tensor(beta)) * (0.0 * m))


# ---- 3. one evaluation ------------------------------------------------------------------------------------------------------------
def _nhwc(x):
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).contiguous()


@pytest.mark.parametrize("name", ["tiny", "tiny40", "sd15"])
def test_one_evaluation(name):
    """agd_unet_forward_hw under a length-1 schedule, B = 1, K = 2, 16 x 16 latents, t = 301."""
    from agenda_amd import config, ops
    from oracle import sd_oracle as O
    cfg, u, v = _weights(name)
    B, K, L, t = 1, 2, 16, 301.0
    ctx, emb, full = _contexts(cfg, B, K, 6)
    x1 = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(3))
    x = x1.repeat(2 + K, 1, 1, 1)
    pipe = _pipe(name)
    e = pipe.engine
    e.set_context(ctx)
    plain = e.unet_forward(x[:2 * B], t).cpu()
    e.set_context(full)
    zero = config.sega_schedule(1, K, edit_guidance_scale=0.0, edit_warmup_steps=0, edit_threshold=0.9)
    real = config.sega_schedule(1, K, edit_guidance_scale=SCALE, reverse_editing_direction=[False, True], edit_warmup_steps=0, edit_threshold=0.9)
    assert e.sega_counts() == (0, 0)
    e.sega_set(zero, 0.0, BETA)
    A = e.unet_forward(x, t).cpu()
    assert e.sega_counts() == (1, 1)
    e.sega_set(real, MU, BETA)
    Bo = e.unet_forward(x, t).cpu()
    again = e.unet_forward(x, t).cpu()
    assert e.sega_counts() == (3, 3)
    thr = ops.sega_threshold(_nhwc(A).cuda(), B, real["coef"][0], real["q"]).cpu()
    e.sega_clear()
    e.set_context(ctx)
    assert torch.equal(e.unet_forward(x[:2 * B], t).cpu(), plain)            # cleared: the plain UNet again
    e.close()
    assert torch.equal(A[:2 * B], plain)                                    # coef = 0, mu = 0: the unfolded rows; the pair is the plain forward's
    assert torch.equal(Bo[2 * B:], A[2 * B:]) and torch.equal(again, Bo)    # the concept rows are left as the walk made them
    assert not torch.equal(Bo[:2 * B], A[:2 * B])
    # the pair of B is the fold of A's rows: the CPU fold from the fp64 thresholds, within the fold op's bound, with exact masks
    rows = _nhwc(A)
    c, q = real["coef"][0], real["q"]
    want_thr = torch.stack([R.quantile(_v32(rows, B, K, c)[k].abs().double().permute(0, 2, 1), q[k])[0] for k in range(K)], 1)     # [B, K, 4]
    vv = _v32(rows, B, K, c).permute(1, 0, 2, 3)
    assert torch.equal(vv.abs() >= thr[:, :, None, :], vv.abs().double() >= want_thr[:, :, None, :])
    m0 = torch.zeros(B, L * L, 4)
    worst = _check_fold(rows, m0, thr, B, c, real["w_mom"][0], real["w_add"][0], real["add_mom"][0], _f32(MU), _f32(BETA),
                        torch.cat([_nhwc(Bo[:2 * B]), rows[2 * B:]]), None)           # (the momentum of a forward is not returned)
    # the concept rows against the oracle forward under the concept's context, with the plain forward's own error as the yardstick
    with torch.no_grad():
        fwd = lambda ci: O.unet_forward(u, cfg.unet, x1, torch.tensor(t), ci)
        err_plain = _rms_rel(plain, torch.cat([fwd(ctx[i:i + 1]) for i in range(2)]))
        err_k = [_rms_rel(A[2 + k:3 + k], fwd(emb[k:k + 1])) for k in range(K)]
    print(f"sega one evaluation {name}: concept rows rms rel {err_k} (plain {err_plain:.5f}); fold worst error / bound {worst:.3f}")
    report(f"sega_forward[{name}]", concept_rms_rel=max(err_k), plain_rms_rel=err_plain, fold_error_over_bound=worst)
    assert max(err_k) <= FWD_FACTOR * err_plain, (err_k, err_plain)


# ---- 4. loops ---------------------------------------------------------------------------------------------------------------------
LOOP_KW = dict(edit_guidance_scale=SCALE, edit_warmup_steps=[1, 3], edit_cooldown_steps=[None, 5], edit_momentum_scale=MU, edit_mom_beta=BETA,
               reverse_editing_direction=[False, True])
LOOP_CASES = [("DDIMScheduler", "ddim", 6, 16, 16), ("PNDMScheduler", "pndm", 5, 16, 16), ("DPMSolverMultistepScheduler", "dpm", 6, 16, 16),
              ("DDIMScheduler", "ddim", 6, 16, 24)]


def _call(pipe, ctx, lat, steps, **kw):
    from agenda_amd import trace
    B, Lh, Lw = lat.shape[0], lat.shape[2], lat.shape[3]
    with trace(pipe) as trc:
        out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, height=8 * Lh, width=8 * Lw, guidance_scale=S, output_type="np", **kw)
        hm = torch.stack([trc.compute_global_heat_map(image_index=i).heat_maps for i in range(B)]).cpu()
    return out.latents.cpu(), out.images, hm


def _decode(v, cfg, x):
    from oracle import sd_oracle as O
    with torch.no_grad():
        return O.postprocess_image(O.vae_decode(v, cfg.vae, x / cfg.vae.scaling_factor))


@pytest.mark.parametrize("scheduler,key,steps,Lh,Lw", LOOP_CASES, ids=[f"{c[1]}-{c[3]}x{c[4]}" for c in LOOP_CASES])
def test_loop_matches_restatement(scheduler, key, steps, Lh, Lw):
    """tiny, B = 2, K = 2, six evaluations, warm-up (1, 3), cool-down (never, 5), mu = 0.3.  At q = 0 nothing is masked and the fold is
    linear: the latents against the restatement within LOOP_FACTOR x the plain call's own error against the plain oracle loop.  At
    q = 0.9: finite, moved, two runs equal bits, the counters the schedule's; its PSNR against the restatement is reported, not asserted
    (an element next to the threshold may fall on the other side of it: no bound can be derived)."""
    from agenda_amd import config
    cfg, u, v = _weights("tiny")
    B, K = 2, 2
    ctx, emb, full = _contexts(cfg, B, K, 41)
    lat = torch.randn(B, 4, Lh, Lw, generator=torch.Generator().manual_seed(8))
    pipe = _pipe("tiny", scheduler)
    plain = _call(pipe, ctx, lat, steps)
    c0 = pipe.engine.sega_counts()
    got0 = _call(pipe, ctx, lat, steps, editing_prompt_embeddings=emb, edit_threshold=0.0, **LOOP_KW)
    c1 = pipe.engine.sega_counts()
    got9 = _call(pipe, ctx, lat, steps, editing_prompt_embeddings=emb, edit_threshold=0.9, **LOOP_KW)
    c2 = pipe.engine.sega_counts()
    again9 = _call(pipe, ctx, lat, steps, editing_prompt_embeddings=emb, edit_threshold=0.9, **LOOP_KW)
    after = _call(pipe, ctx, lat, steps)
    pipe.engine.close()
    n = 6
    sched = config.sega_schedule(n, K, **{k: w for k, w in LOOP_KW.items() if k not in ("edit_momentum_scale", "edit_mom_beta")})
    assert (sched["walks"], sched["folds"]) == (6, 6)
    assert c0 == (0, 0) and c1 == (sched["walks"], sched["folds"]) and c2 == (2 * sched["walks"], 2 * sched["folds"])
    want_plain, n_plain = R.generate(u, v, cfg, ctx, lat, steps, key, S, None)
    want0, n0 = R.generate(u, v, cfg, full, lat, steps, key, S, R.Sega(K, edit_threshold=0.0, **LOOP_KW))
    sg9 = R.Sega(K, edit_threshold=0.9, **LOOP_KW)
    want9, _ = R.generate(u, v, cfg, full, lat, steps, key, S, sg9)
    assert n_plain == n0 == n and sg9.walks == sched["walks"]
    e_plain, e0 = _rms_rel(plain[0], want_plain), _rms_rel(got0[0], want0)
    print(f"sega loop {key} {Lh}x{Lw}: q = 0 latents rms rel {e0:.5f} (plain {e_plain:.5f}, factor {LOOP_FACTOR:.2f})")
    assert not torch.equal(want0, want_plain) and not torch.equal(got0[0], plain[0])
    # the same call at q = 0.9
    assert torch.isfinite(got9[0]).all() and not torch.equal(got9[0], plain[0]) and not torch.equal(got9[0], got0[0])
    assert torch.equal(again9[0], got9[0]) and np.array_equal(again9[1], got9[1]) and torch.equal(again9[2], got9[2])
    assert torch.equal(after[0], plain[0]) and torch.equal(after[2], plain[2])            # and the call after is the plain one again
    psnr9, e9 = _psnr(got9[1], _decode(v, cfg, want9)), _rms_rel(got9[0], want9)
    report(f"sega_loop[tiny,{key},{Lh}x{Lw}]", q0_latents_rms_rel=e0, plain_latents_rms_rel=e_plain, q09_psnr_db=psnr9, q09_latents_rms_rel=e9,
           plain_psnr_db=_psnr(plain[1], _decode(v, cfg, want_plain)))
    assert e0 <= LOOP_FACTOR * e_plain, (e0, e_plain)


# ---- 5. the off switch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheduler", ["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"])
def test_off_switch_is_bit_identical_to_the_plain_call(scheduler):
    """No editing prompt sets nothing.  edit_guidance_scale = 0 with mu = 0 sets the state -- the context holds the concept rows, every
    evaluation folds -- and gives the plain call's latents, images and trace maps bit for bit: no concept walk, nothing recorded, nothing added."""
    cfg, u, v = _weights("tiny")
    B, K, L, steps = 2, 2, 16, 4
    ctx, emb, _ = _contexts(cfg, B, K, 42)
    lat = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(4))
    pipe = _pipe("tiny", scheduler)
    plain = _call(pipe, ctx, lat, steps)
    none = _call(pipe, ctx, lat, steps, editing_prompt=None, edit_guidance_scale=9.0, edit_threshold=0.5)
    assert pipe.engine.sega_counts() == (0, 0)
    zero = _call(pipe, ctx, lat, steps, editing_prompt_embeddings=emb, edit_guidance_scale=0.0, edit_momentum_scale=0.0, edit_warmup_steps=0)
    n = steps + (scheduler == "PNDMScheduler")
    assert pipe.engine.sega_counts() == (0, n)
    on = _call(pipe, ctx, lat, steps, editing_prompt_embeddings=emb, edit_warmup_steps=1)
    assert pipe.engine.sega_counts() == (n, 2 * n)
    pipe.engine.close()
    for got in (none, zero):
        assert torch.equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and torch.equal(got[2], plain[2])
    assert not torch.equal(on[0], plain[0])
    assert float(on[2].sum(1).mean()) == pytest.approx(float(plain[2].sum(1).mean()), rel=0.02)      # the concept walk recorded nothing


def test_engine_is_clear_after_a_call_that_raises():
    from agenda_amd import _lib
    cfg, u, v = _weights("tiny")
    B, K, L, steps = 2, 1, 16, 3
    ctx, emb, _ = _contexts(cfg, B, K, 2)
    lat = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(5))
    pipe = _pipe("tiny")
    eng = pipe.engine
    want = _call(pipe, ctx, lat, steps)

    def boom(*a):
        raise RuntimeError("boom")
    real, pipe._denoise = pipe._denoise, boom
    with pytest.raises(RuntimeError, match="boom"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, editing_prompt_embeddings=emb, output_type="latent")
    pipe._denoise = real
    # a state left set would refuse this call (a schedule of 3 evaluations, a context of 3 B rows against a plain 2 B one)
    after = _call(pipe, ctx, lat, steps)
    assert torch.equal(after[0], want[0]) and torch.equal(after[2], want[2])
    # refused by the engine inside the loop (a Perturbed-Attention Guidance schedule set behind the pipeline's back): cleared all the same
    eng.pag_set([3.0] * steps, [])
    with pytest.raises(_lib.AgendaHipError, match="sega: a Perturbed-Attention Guidance schedule is set"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, editing_prompt_embeddings=emb, output_type="latent")
    eng.pag_clear()
    assert eng.sega_counts() == (0, 0)
    after = _call(pipe, ctx, lat, steps)
    eng.close()
    assert torch.equal(after[0], want[0]) and torch.equal(after[2], want[2])


# ---- 6. beside other features -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rigs():
    """tools/record_conditioning.py's engines: the 4-channel UNet with a ControlNet, GLIGEN fusers, a T2I-Adapter and an IP-Adapter loaded,
    the 8-channel InstructPix2Pix variant and the 9-channel inpainting variant."""
    from agenda_amd import config
    spec = importlib.util.spec_from_file_location("record_conditioning", os.path.join(ROOT, "tools", "record_conditioning.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = {"e4": mod.Rig(config.tiny(), True), "e8": mod.Rig(config.ip2p_variant(config.tiny()), False),
         "e9": mod.Rig(config.inpaint_variant(config.tiny()), False)}
    yield r
    for rig in r.values():
        rig.e.close()


def _sched(n, K=1):
    from agenda_amd import config
    return config.sega_schedule(n, K, edit_warmup_steps=0)


ROW = {"cn": "sega: a ControlNet schedule is set; Semantic Guidance with a ControlNet is not implemented",
       "gl": "sega: a GLIGEN schedule is set; Semantic Guidance with GLIGEN is not implemented",
       "inp": "sega: an inpainting state is set; Semantic Guidance with inpainting is not implemented",
       "i2p": "sega: an InstructPix2Pix state is set; Semantic Guidance with InstructPix2Pix is not implemented",
       "ad": "sega: a T2I-Adapter schedule is set; Semantic Guidance with a T2I-Adapter is not implemented",
       "ipa": "sega: an IP-Adapter image is set; Semantic Guidance with an IP-Adapter is not implemented"}


@pytest.mark.parametrize("state", ["cn", "gl", "inp", "ad", "ipa"])
def test_conflict_row_on_the_4_channel_engine(rigs, state):
    """Each state beside a Semantic Guidance state is refused by name before the first launch, by the fused loops and by unet_forward."""
    from agenda_amd._lib import AgendaHipError
    rig = rigs["e4"]
    rig.clear(); rig.e.sega_clear()
    rig.context(2)
    c0 = rig.e.sega_counts()
    try:
        rig.set(state, 2)
        rig.e.sega_set(_sched(2), MU, BETA)
        for loop in (rig.denoise, rig.plms, rig.dpm) if state != "inp" else (rig.denoise,):
            with pytest.raises(AgendaHipError) as ei:
                loop()
            assert ROW[state] in str(ei.value), str(ei.value)
        rig.set(state, 1)
        rig.e.sega_set(_sched(1), MU, BETA)
        with pytest.raises(AgendaHipError) as ei:
            rig.forward()
        assert ROW[state] in str(ei.value), str(ei.value)
        rig.e.sega_clear()                                       # with the state cleared the same call runs
        rig.set(state, 2)
        assert torch.isfinite(rig.denoise()).all()
    finally:
        rig.clear(); rig.e.sega_clear()
    assert rig.e.sega_counts() == c0


def test_conflict_row_on_the_other_engines_and_entry_points(rigs):
    from agenda_amd import synthetic
    from agenda_amd._lib import AgendaHipError
    e8, e9, e4 = rigs["e8"], rigs["e9"], rigs["e4"]
    try:
        e8.clear(); e8.context(2); e8.set("i2p", 2); e8.e.sega_set(_sched(2), MU, BETA)
        with pytest.raises(AgendaHipError) as ei:
            e8.denoise()
        assert ROW["i2p"] in str(ei.value), str(ei.value)
        e9.clear(); e9.context(2); e9.set("inp", 2); e9.e.sega_set(_sched(2), MU, BETA)         # the 9-channel mode
        with pytest.raises(AgendaHipError) as ei:
            e9.denoise()
        assert ROW["inp"] in str(ei.value), str(ei.value)
        e = e4.e
        e4.clear(); e4.context(2); e.sega_set(_sched(2), MU, BETA)
        with pytest.raises(AgendaHipError, match="denoise_panorama: a Semantic Guidance state is set"):
            e4.panorama()
        ddim2 = type(e4).denoise.__globals__["DDIM2"]             # the rig's two-step DDIM program
        canvas, masks = torch.zeros(2, 4, 16, 16).cuda(), torch.ones(2, 2, 16, 16).cuda()
        with pytest.raises(AgendaHipError, match="denoise_regions: a Semantic Guidance state is set"):
            e.denoise_regions(canvas, masks, None, None, [], [], 0, *ddim2, 7.5)
        e.pag_set([3.0, 3.0], [])
        with pytest.raises(AgendaHipError, match="sega: a Perturbed-Attention Guidance schedule is set"):
            e4.denoise()
        e.pag_clear()
        e.deepcache_set([1, 0], 0)
        with pytest.raises(AgendaHipError, match="sega: a DeepCache schedule is set"):
            e4.denoise()
        e.deepcache_clear()
        e.guidance_rescale_set(0.7)
        for loop, n in ((e4.denoise, 2), (e4.plms, 3), (e4.dpm, 2)):       # (PLMS x 2 steps is three evaluations)
            e.sega_set(_sched(n), MU, BETA)
            with pytest.raises(AgendaHipError, match=r"Semantic Guidance denoise loop: guidance rescale \(phi = 0.7\) is set"):
                loop()
        e.guidance_rescale_clear()
        e.sega_set(_sched(1), MU, BETA)
        with pytest.raises(AgendaHipError, match="unet_forward_ts: a Semantic Guidance state is set"):
            e4.forward(per_image=True)
        with pytest.raises(AgendaHipError, match="deepcache_forward: a Semantic Guidance state is set"):
            e.deepcache_forward(torch.zeros(4, 4, 16, 16).cuda(), 11.0, 0, False)
        # the schedule's length is the call's evaluations; the context's rows are (2 + K) B
        e.sega_set(_sched(5), MU, BETA)
        for loop in (e4.denoise, e4.plms, e4.dpm, e4.forward):
            with pytest.raises(AgendaHipError, match="sega: the schedule covers 5 model evaluations, this call runs"):
                loop()
        e.sega_set(_sched(2), MU, BETA)
        with pytest.raises(AgendaHipError, match=r"sega: the context holds 4 rows; 1 concepts on 2 images take \(2 \+ K\) B = 6"):
            e4.denoise()
        e.sega_set(_sched(1, 3), MU, BETA)
        with pytest.raises(AgendaHipError, match="sega: unet_forward on 4 rows; 3 concepts take"):
            e4.forward()
        # a context over 96 tokens
        e.sega_set(_sched(2), MU, BETA)
        long_ctx = synthetic.make_context(e4.cfg, 3, seed=1)
        e.set_context(torch.cat([long_ctx, long_ctx], 1)[:, :152].contiguous())
        with pytest.raises(AgendaHipError, match="long context: a Semantic Guidance state is set"):
            e4.denoise()
        # with the state cleared the loop runs again
        e.sega_clear(); e4.context(2)
        assert torch.isfinite(e4.denoise()).all()
    finally:
        e4.e.guidance_rescale_clear(); e4.e.pag_clear(); e4.e.deepcache_clear()
        for r in (e4, e8, e9):
            r.clear(); r.e.sega_clear()
        e4.context(2)


def test_sega_set_refusals(rigs):
    import ctypes as C
    from agenda_amd import _lib
    from agenda_amd._lib import AgendaHipError
    e = rigs["e4"].e
    e.sega_clear()
    good = _sched(2, 2)
    for key, bad, msg in (("q", [0.5, 1.5], r"q\[1\]"), ("coef", [[5.0, float("nan")], [5.0, 5.0]], "coef"), ("add_mom", [1.0, float("inf")], "add_mom")):
        with pytest.raises(AgendaHipError, match="sega_set: .*" + msg):
            e.sega_set(dict(good, **{key: bad}), MU, BETA)
    with pytest.raises(AgendaHipError, match="sega_set: momentum"):
        e.sega_set(good, float("nan"), BETA)
    with pytest.raises(AgendaHipError, match=r"sega_set: 9 concepts"):
        e.sega_set({"concepts": 9, "n_evals": 1, "coef": [[1.0] * 9], "w_mom": [[0.0] * 9], "w_add": [[0.0] * 9], "add_mom": [0.0], "q": [0.5] * 9}, MU, BETA)
    d = _lib.AgdSegaDesc(struct_size=4)
    with pytest.raises(AgendaHipError, match="struct_size"):
        _lib.check(e.lib.agd_sega_set(e.ctx, C.byref(d)), e.ctx, "agd_sega_set")
    c0 = e.sega_counts()
    rigs["e4"].clear(); rigs["e4"].context(2)                   # a refused set leaves the state clear: the plain loop runs
    assert torch.isfinite(rigs["e4"].denoise()).all() and e.sega_counts() == c0


def test_pipeline_refusals_on_the_device():
    """What the argument checks need a pipeline for: a long context, embeddings of another shape, an enabled DeepCache; the other pipelines'
    refusals run before any device work (tests/test_sega_cpu.py)."""
    cfg, u, v = _weights("tiny")
    pipe = _pipe("tiny")
    B, L = 2, 16
    ctx, emb, _ = _contexts(cfg, B, 1, 1)
    lat = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(1))
    long_ctx = torch.cat([ctx, ctx], 1)[:, :152].contiguous()
    with pytest.raises(ValueError, match="over 96"):
        pipe(prompt_embeds=long_ctx, latents=lat, num_inference_steps=2, editing_prompt_embeddings=torch.cat([emb, emb], 1)[:, :152].contiguous())
    with pytest.raises(ValueError, match="editing_prompt_embeddings of shape"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, editing_prompt_embeddings=emb[:, :50].contiguous())
    pipe.enable_deepcache(cache_interval=3)
    with pytest.raises(ValueError, match="DeepCache"):
        pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, editing_prompt_embeddings=emb)
    pipe.disable_deepcache()
    out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=2, editing_prompt_embeddings=emb, edit_warmup_steps=0, output_type="latent").latents
    assert torch.isfinite(out).all() and pipe.engine.sega_counts() == (2, 2)
    pipe.engine.close()


def test_editing_prompt_strings_are_encoded_as_a_prompt_is():
    """The string form on a pipeline with a text encoder (what the CLI passes): the same bits as the call given the encoder's rows for the
    same strings as editing_prompt_embeddings, one string as a one-entry list, and the context refusals ahead of any encoding."""
    from agenda_amd import StableDiffusionPipeline
    pipe = StableDiffusionPipeline.from_synthetic("tiny", workspace_bytes=1 << 30)
    B, L, steps = 2, 16, 3
    lat = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(6))
    prompt = ["an aerial view image with cars"] * B
    run = lambda **kw: pipe(prompt=prompt, latents=lat, num_inference_steps=steps, edit_warmup_steps=1, output_type="latent", **kw).latents.cpu()
    plain = pipe(prompt=prompt, latents=lat, num_inference_steps=steps, output_type="latent").latents.cpu()
    words = ["more cars", "trees"]
    got = run(editing_prompt=words, reverse_editing_direction=[False, True])
    assert pipe.engine.sega_counts() == (steps, steps)
    emb = pipe.text_encoder(words)
    assert tuple(emb.shape) == (2, pipe.cfg.max_tokens, pipe.cfg.unet.cross_attention_dim)
    same = run(editing_prompt_embeddings=emb, reverse_editing_direction=[False, True])
    one, one_list = run(editing_prompt="trees"), run(editing_prompt=["trees"])
    with pytest.raises(ValueError, match="editing_prompt_embeddings of shape"):
        run(editing_prompt_embeddings=emb[:, :40].contiguous())
    pipe.engine.close()
    assert torch.isfinite(got).all() and not torch.equal(got, plain)
    assert torch.equal(got, same) and torch.equal(one, one_list) and not torch.equal(one, got)


@pytest.mark.parametrize("beside", ["lora", "freeu"])
def test_sega_beside_a_lora_and_freeu(beside):
    """The concept walk reads the LoRA-merged matrices / runs FreeU like the main walk: the call runs, moves the sample, and with every
    coefficient 0 is the LoRA / FreeU call bit for bit."""
    from agenda_amd import lora
    cfg, u, v = _weights("tiny")
    B, K, L, steps = 2, 2, 16, 4
    ctx, emb, _ = _contexts(cfg, B, K, 41)
    lat = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(9))
    pipe = _pipe("tiny")
    kw = {}
    if beside == "lora":
        g = torch.Generator().manual_seed(31)
        rank, sd = 4, {}
        for m, (_, (n_out, n_in)) in lora.target_modules(cfg).items():
            k = "lora_unet_" + m.replace(".", "_")
            d, up = torch.randn(rank, n_in, generator=g) / n_in ** 0.5, torch.randn(n_out, rank, generator=g) * 0.05
            if m.endswith(("proj_in", "proj_out")) and not cfg.unet.use_linear_projection:
                d, up = d.reshape(rank, n_in, 1, 1), up.reshape(n_out, rank, 1, 1)
            sd[k + ".lora_down.weight"], sd[k + ".lora_up.weight"] = d, up
        pipe.load_lora_weights(sd)
        kw = {"cross_attention_kwargs": {"scale": 0.8}}
    else:
        pipe.enable_freeu(0.9, 0.2, 1.5, 1.6)
    base = _call(pipe, ctx, lat, steps, **kw)
    zero = _call(pipe, ctx, lat, steps, editing_prompt_embeddings=emb, edit_guidance_scale=0.0, edit_momentum_scale=0.0, **kw)
    on = _call(pipe, ctx, lat, steps, editing_prompt_embeddings=emb, edit_warmup_steps=1, **kw)
    counts = pipe.engine.sega_counts()
    pipe.engine.close()
    assert torch.equal(zero[0], base[0]) and torch.equal(zero[2], base[2])
    assert torch.isfinite(on[0]).all() and not torch.equal(on[0], base[0]) and counts == (steps, 2 * steps)


def test_img2img_counts_its_shortened_grid():
    from agenda_amd import StableDiffusionPipeline, synthetic
    cfg, u, _ = _weights("tiny")
    v = synthetic.make_vae_weights(cfg, 12, with_encoder=True, bias_std=0.05, perturb_norm=0.1)
    pipe = StableDiffusionPipeline(cfg, u, v, workspace_bytes=2 << 30)
    B, K, L, steps = 2, 2, 16, 6
    ctx, emb, _ = _contexts(cfg, B, K, 3)
    img = torch.rand(B, 3, 8 * L, 8 * L, generator=torch.Generator().manual_seed(4)) * 2 - 1
    nz = torch.randn(2, B, 4, L, L, generator=torch.Generator().manual_seed(5))
    run = lambda **kw: pipe.img2img(image=img, strength=0.5, num_inference_steps=steps, prompt_embeds=ctx, noise_enc=nz[0], noise=nz[1],
                                    output_type="latent", **kw).latents.cpu()
    plain = run()
    on = run(editing_prompt_embeddings=emb, edit_warmup_steps=1, edit_cooldown_steps=[None, 2])
    counts = pipe.engine.sega_counts()
    off = run(editing_prompt_embeddings=emb, edit_guidance_scale=0.0, edit_momentum_scale=0.0)
    pipe.engine.close()
    assert counts == (3, 3)                                      # strength 0.5 of 6 steps: three evaluations, counted from 0
    assert torch.isfinite(on).all() and not torch.equal(on, plain) and torch.equal(off, plain)
