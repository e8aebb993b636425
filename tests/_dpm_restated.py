"""DPM-Solver++ (2M) written out from its formulas, independent of agenda_amd/scheduler.py (shared by the DPM tests).

alpha_s = sqrt(abar_s), sigma_s = sqrt(1 - abar_s), lambda_s = log alpha_s - log sigma_s; one step s -> t with model output m:
    x0 = (x - sigma_s m) / alpha_s  (eps)  or  alpha_s x - sigma_s m  (v)
    h = lambda_t - lambda_s, r = (lambda_s - lambda_prev) / h
    D = x0 (first order: step 0, and the last step below 15 steps)  or  (1 + 1/(2r)) x0 - 1/(2r) x0_prev
    x_t = (sigma_t / sigma_s) x - alpha_t (exp(-h) - 1) D"""
import math

import numpy as np
import torch


def grid(n, karras, num_train=1000, beta_start=0.00085, beta_end=0.012):
    """linspace spacing or Karras (rho = 7) noise levels: (UNet timesteps, alpha, sigma); alpha / sigma carry the final target
    (timestep 0 of the table) as their last entry."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train, dtype=torch.float32) ** 2
    abar = torch.cumprod(1.0 - betas, dim=0).numpy().astype(np.float64)
    if not karras:
        t = np.linspace(0, num_train - 1, n + 1).round()[::-1][:-1].astype(np.int64)
        ab = np.append(abar[t], abar[0])
        return t.astype(np.float64), np.sqrt(ab), np.sqrt(1 - ab)
    table = np.sqrt((1 - abar) / abar)
    lo, hi = table[0] ** (1 / 7), table[-1] ** (1 / 7)
    ks = np.array([(hi + k / max(n - 1, 1) * (lo - hi)) ** 7 for k in range(n)])
    t = np.interp(np.log(ks), np.log(table), np.arange(float(num_train)))
    sig = np.append(ks, table[0])
    al = 1 / np.sqrt(1 + sig ** 2)
    return t, al, sig * al


def sample(n, karras, pred, model, x):
    """Run n steps from x; model(x, i, t) -> model output (numpy array or torch tensor, same kind as x)."""
    t, al, sg = grid(n, karras)
    lam = [math.log(float(a) / float(s)) for a, s in zip(al, sg)]
    x0_prev = None
    for i in range(n):
        a_s, s_s, a_t, s_t = float(al[i]), float(sg[i]), float(al[i + 1]), float(sg[i + 1])
        m = model(x, i, float(t[i]))
        x0 = (x - s_s * m) / a_s if pred == "epsilon" else a_s * x - s_s * m
        h = lam[i + 1] - lam[i]
        if i == 0 or (i == n - 1 and n < 15) or h == 0:
            D = x0
        else:
            r = (lam[i] - lam[i - 1]) / h
            D = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * x0_prev
        x = (s_t / s_s) * x - a_t * math.expm1(-h) * D
        x0_prev = x0
    return t, x
