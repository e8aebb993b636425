"""Host-side schedulers (timesteps + alpha products); the per-step arithmetic runs on the GPU
(`agd_denoise` / `agd_cfg_ddim_step` for DDIM, `agd_denoise_plms` for PNDM, `agd_denoise_dpm` for DPM-Solver++ 2M).

DDIM is BASELINE.json's metric (50 DDIM steps).  PNDM (skip_prk_steps = PLMS) is what the reference itself runs:
`pipeline(prompt, num_inference_steps=20)` at data_generation.py:59 never constructs a scheduler, so the fine-tuned
CompVis SD-1.4 checkpoint's `scheduler/scheduler_config.json` (`PNDMScheduler`) decides [upstream-knowledge].
Both mirror the config SD ships with [upstream-knowledge, SURVEY.md §8a row S1]: scaled-linear betas, "leading" spacing,
steps_offset=1, clip_sample=False, set_alpha_to_one=False; DDIM eta=0."""
from __future__ import annotations

import numpy as np

from .config import SchedulerConfig


def rescale_zero_terminal_snr(betas):
    """diffusers' `rescale_zero_terminal_snr` (Lin et al. 2023, algorithm 1) in the same torch float32 operations [upstream-knowledge:
    diffusers 0.21.2 scheduling_ddim.py], so the table is bit-identical: sqrt(alphas_cumprod) is shifted so that its last entry is 0 and
    scaled so that its first is unchanged, then turned back into betas."""
    import torch
    alphas = 1.0 - betas
    alphas_cumprod = torch.cumprod(alphas, dim=0)
    alphas_bar_sqrt = alphas_cumprod.sqrt()
    alphas_bar_sqrt_0 = alphas_bar_sqrt[0].clone()
    alphas_bar_sqrt_T = alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt -= alphas_bar_sqrt_T
    alphas_bar_sqrt *= alphas_bar_sqrt_0 / (alphas_bar_sqrt_0 - alphas_bar_sqrt_T)
    alphas_bar = alphas_bar_sqrt ** 2
    alphas = alphas_bar[1:] / alphas_bar[:-1]
    alphas = torch.cat([alphas_bar[0:1], alphas])
    return 1 - alphas


class DDIMScheduler:
    """diffusers `DDIMScheduler` (eta 0) [upstream-knowledge: diffusers 0.21.2 set_timesteps / step].  Timestep grids (T training
    timesteps, n steps):
        "leading"  (SD's own): arange(0, n) * (T // n), reversed, + steps_offset;
        "trailing": round(arange(T, 0, -T / n)) - 1          (the first evaluation is at T - 1);
        "linspace": linspace(0, T - 1, n).round(), reversed  (end points T - 1 and 0).
    For every spacing prev_t = t - T // n, and prev_t < 0 takes final_alpha_cumprod.  `rescale_betas_zero_snr`: the zero-terminal-SNR
    beta table (alphas_cumprod[-1] == 0); a grid that visits such a timestep needs v-prediction -- epsilon prediction divides by
    sqrt(alpha) -- and step_coeffs refuses it otherwise."""

    _SPACINGS = ("leading", "trailing", "linspace")

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 set_alpha_to_one=False, prediction_type="epsilon", timestep_spacing="leading", rescale_betas_zero_snr=False):
        if timestep_spacing not in self._SPACINGS:
            raise ValueError(f"DDIMScheduler: timestep_spacing {timestep_spacing!r} is not one of {self._SPACINGS}")
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self.prediction_type = prediction_type
        self.timestep_spacing = timestep_spacing
        self.rescale_betas_zero_snr = bool(rescale_betas_zero_snr)
        # the same torch float32 ops diffusers uses (scaled_linear betas -> cumprod), so the table is bit-identical
        import torch
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        if self.rescale_betas_zero_snr:
            betas = rescale_zero_terminal_snr(betas)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).numpy()
        self.final_alpha_cumprod = np.float32(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.timesteps = None
        self.num_inference_steps = None

    @classmethod
    def from_config(cls, sc):
        return cls(sc.num_train_timesteps, sc.beta_start, sc.beta_end, sc.steps_offset, sc.set_alpha_to_one,
                   sc.prediction_type, timestep_spacing=getattr(sc, "ddim_timestep_spacing", "leading"),
                   rescale_betas_zero_snr=getattr(sc, "rescale_betas_zero_snr", False))

    def set_timesteps(self, num_inference_steps: int):
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError("num_inference_steps exceeds num_train_timesteps")
        T = self.num_train_timesteps
        if self.timestep_spacing == "trailing":
            ts = np.round(np.arange(T, 0, -T / num_inference_steps)).astype(np.int64) - 1
        elif self.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        else:
            ratio = T // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.steps_offset
        self.num_inference_steps = num_inference_steps
        self.timesteps = ts
        return ts

    def step_coeffs(self):
        """Per-step (alpha_cumprod[t], alpha_cumprod[prev_t]) arrays for the current timesteps."""
        ratio = self.num_train_timesteps // self.num_inference_steps
        a_t = np.array([self.alphas_cumprod[t] for t in self.timesteps], dtype=np.float32)
        a_p = np.array([self.alphas_cumprod[t - ratio] if t - ratio >= 0 else self.final_alpha_cumprod
                        for t in self.timesteps], dtype=np.float32)
        if self.prediction_type == "epsilon" and (a_t == 0).any():
            t0 = int(self.timesteps[int(np.argmax(a_t == 0))])
            raise ValueError(f"DDIMScheduler: timestep {t0} has alphas_cumprod == 0 (rescale_betas_zero_snr) and epsilon prediction divides "
                             "by its square root there; a zero-terminal-SNR schedule needs prediction_type='v_prediction'")
        return a_t, a_p


class PNDMScheduler:
    """diffusers `PNDMScheduler` as SD-1.x checkpoints configure it [upstream-knowledge: diffusers 0.21.2]: scaled-linear betas,
    `skip_prk_steps=True` (pure PLMS), "leading" spacing, `steps_offset=1`, `set_alpha_to_one=False`, epsilon prediction.
    `num_inference_steps` = n means n + 1 model evaluations: the second timestep is evaluated twice."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1, set_alpha_to_one=False,
                 prediction_type="epsilon", skip_prk_steps=True, timestep_spacing="leading", rescale_betas_zero_snr=False):
        if timestep_spacing != "leading":
            raise ValueError(f"PNDMScheduler: only timestep_spacing='leading' is implemented (got {timestep_spacing!r}); "
                             "'trailing' and 'linspace' are DDIMScheduler's")
        if rescale_betas_zero_snr:
            raise ValueError("PNDMScheduler: rescale_betas_zero_snr is not implemented (diffusers 0.21.2 has it on DDIMScheduler only)")
        if prediction_type != "epsilon":
            raise ValueError("PNDMScheduler: only epsilon prediction is implemented (what SD-1.x checkpoints use)")
        if not skip_prk_steps:
            raise ValueError("PNDMScheduler: only skip_prk_steps=True (the SD configuration) is implemented")
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self.prediction_type = prediction_type
        import torch
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).numpy()
        self.final_alpha_cumprod = np.float32(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.timesteps = None
        self.num_inference_steps = None

    @classmethod
    def from_config(cls, sc):
        return cls(sc.num_train_timesteps, sc.beta_start, sc.beta_end, sc.steps_offset, sc.set_alpha_to_one, sc.prediction_type,
                   getattr(sc, "skip_prk_steps", True), timestep_spacing=getattr(sc, "ddim_timestep_spacing", "leading"),
                   rescale_betas_zero_snr=getattr(sc, "rescale_betas_zero_snr", False))

    def set_timesteps(self, num_inference_steps: int):
        if num_inference_steps < 2 or num_inference_steps > self.num_train_timesteps:
            raise ValueError("PNDM needs 2 <= num_inference_steps <= num_train_timesteps")
        ratio = self.num_train_timesteps // num_inference_steps
        t = (np.arange(0, num_inference_steps) * ratio).round().astype(np.int64) + self.steps_offset
        # plms_timesteps = concat(t[:-1], t[-2:-1], t[-1:])[::-1]: the second (in run order) timestep appears twice
        self.timesteps = np.concatenate([t[:-1], t[-2:-1], t[-1:]])[::-1].copy()
        self.num_inference_steps = num_inference_steps
        return self.timesteps

    def plms_program(self):
        """Per model evaluation i: (UNet timestep, sample_coeff, eps_coeff) of `_get_prev_sample`:
        prev = sample_coeff * sample + eps_coeff * model_output (model_output = the PLMS combination, applied on the device)."""
        ratio = self.num_train_timesteps // self.num_inference_steps
        a, b = [], []
        for i, t in enumerate(self.timesteps):
            t, prev = int(t), int(t) - ratio
            if i == 1:                                   # step_plms with counter == 1: redo the first step from the kept sample
                prev, t = t, t + ratio
            al_t = float(self.alphas_cumprod[t])
            al_p = float(self.alphas_cumprod[prev]) if prev >= 0 else float(self.final_alpha_cumprod)
            denom = al_t * (1 - al_p) ** 0.5 + (al_t * (1 - al_t) * al_p) ** 0.5
            a.append((al_p / al_t) ** 0.5)
            b.append(-(al_p - al_t) / denom)
        return np.asarray(self.timesteps, dtype=np.float32), np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)


class DPMSolverMultistepScheduler:
    """diffusers `DPMSolverMultistepScheduler` in its DPM-Solver++ 2M form [upstream-knowledge: diffusers 0.21.2]:
    `algorithm_type="dpmsolver++"`, `solver_order=2`, `solver_type="midpoint"`, `lower_order_final=True`, epsilon or
    v-prediction, with or without Karras sigmas.  One model evaluation per step.  Any other option raises ValueError.

    Notation: alpha_s = sqrt(abar_s), sigma_s = sqrt(1 - abar_s), lambda_s = log alpha_s - log sigma_s.  One step s -> t with the
    CFG-combined model output m:
        x0  = cx x + ce m                    (eps: cx = 1/alpha_s, ce = -sigma_s/alpha_s;  v: cx = alpha_s, ce = -sigma_s)
        h   = lambda_t - lambda_s,  r = (lambda_s - lambda_prev) / h
        D   = x0                                          first order
        D   = (1 + 1/(2r)) x0 - 1/(2r) x0_prev            second order (midpoint)
        x_t = (sigma_t/sigma_s) x - alpha_t (exp(-h) - 1) D

    Edge rules restated from upstream [upstream-knowledge: diffusers 0.21.2 DPMSolverMultistepScheduler.set_timesteps / step]:
     * timestep grid (lambda_min_clipped = -inf, so the last usable training timestep is num_train_timesteps = T):
         "linspace" (the default): linspace(0, T - 1, n + 1).round(), reversed, the trailing 0 dropped;
         "leading":  arange(0, n + 1) * (T // (n + 1)), reversed, the trailing 0 dropped, + steps_offset;
         "trailing": arange(T, 0, -T / n).round() - 1;
       duplicates (n close to T) are dropped keeping the first occurrence, so the step count can fall below n.
     * Karras sigmas: sigma = sqrt((1 - abar) / abar) of the table; n sigmas on the rho = 7 ramp from the table's largest sigma
       (timestep T - 1) to its smallest (timestep 0); each timestep is the log-sigma interpolation of its sigma into the table
       (timestep_spacing then plays no part).
       Upstream rounds that timestep to an integer; here it stays fractional so the UNet's time embedding and the solver's
       alpha / sigma describe the same point (alpha = 1 / sqrt(1 + sigma^2), sigma_t = sigma alpha).  The UNet time embedding
       takes float timesteps.
     * last target: every step's target is the next grid point, and the last step targets timestep 0 of the table
       (abar_0, not sigma = 0: upstream's later `final_sigmas_type="sigma_min"`).  With Karras sigmas the last evaluation already
       sits on that point, so upstream's last update is the identity (h = 0: a = 1, b0 = b1 = 0); it is kept as such.
     * order: step 0 is first order (no history); with lower_order_final the last step drops to first order when the run has
       fewer than 15 steps; every other step is second order."""

    _ONLY = {"algorithm_type": "dpmsolver++", "solver_order": 2, "solver_type": "midpoint", "lower_order_final": True,
             "thresholding": False, "euler_at_final": False, "use_lu_lambdas": False, "final_sigmas_type": "sigma_min",
             "variance_type": None, "beta_schedule": "scaled_linear", "trained_betas": None}
    _SPACINGS = ("linspace", "leading", "trailing")

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1, prediction_type="epsilon",
                 use_karras_sigmas=False, timestep_spacing="linspace", rescale_betas_zero_snr=False, **options):
        self.check_options(options)
        if rescale_betas_zero_snr:
            raise ValueError("DPMSolverMultistepScheduler: rescale_betas_zero_snr is not implemented (diffusers 0.21.2 has no such "
                             "option there; it is DDIMScheduler's)")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"DPMSolverMultistepScheduler: prediction_type {prediction_type!r} is not implemented")
        if timestep_spacing not in self._SPACINGS:
            raise ValueError(f"DPMSolverMultistepScheduler: timestep_spacing {timestep_spacing!r} is not one of {self._SPACINGS}")
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self.prediction_type = prediction_type
        self.use_karras_sigmas = bool(use_karras_sigmas)
        self.timestep_spacing = timestep_spacing
        import torch
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).numpy()
        self.init_noise_sigma = 1.0
        self.timesteps = None
        self.num_inference_steps = None
        self.alpha = self.sigma = self.karras_sigmas = None

    @classmethod
    def check_options(cls, options):
        """Raise ValueError for any option (diffusers config key) this restatement does not implement."""
        for k, v in options.items():
            if k == "lambda_min_clipped":
                if v != -float("inf"):
                    raise ValueError(f"DPMSolverMultistepScheduler: only lambda_min_clipped=-inf is implemented (got {v!r})")
            elif k not in cls._ONLY:
                raise ValueError(f"DPMSolverMultistepScheduler: unknown option {k}={v!r}")
            elif v != cls._ONLY[k]:
                raise ValueError(f"DPMSolverMultistepScheduler: only {k}={cls._ONLY[k]!r} is implemented (got {v!r})")

    @classmethod
    def from_config(cls, sc):
        return cls(sc.num_train_timesteps, sc.beta_start, sc.beta_end, sc.steps_offset, sc.prediction_type,
                   use_karras_sigmas=sc.use_karras_sigmas, timestep_spacing=sc.timestep_spacing,
                   rescale_betas_zero_snr=getattr(sc, "rescale_betas_zero_snr", False), algorithm_type=sc.algorithm_type,
                   solver_order=sc.solver_order, solver_type=sc.solver_type, lower_order_final=sc.lower_order_final)

    def _grid(self, n):
        T = self.num_train_timesteps
        if self.timestep_spacing == "linspace":
            return np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        if self.timestep_spacing == "leading":
            return (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + self.steps_offset
        return np.arange(T, 0, -T / n).round().copy().astype(np.int64) - 1

    def set_timesteps(self, num_inference_steps: int):
        """UNet timesteps (float64; integer-valued without Karras) and the alpha / sigma of every grid point: `alpha[i]`,
        `sigma[i]` for evaluation i, `alpha[-1]`, `sigma[-1]` for the final target (timestep 0)."""
        n = int(num_inference_steps)
        if n < 1 or n > self.num_train_timesteps:
            raise ValueError("DPMSolverMultistepScheduler needs 1 <= num_inference_steps <= num_train_timesteps")
        ac = self.alphas_cumprod.astype(np.float64)
        if self.use_karras_sigmas:
            table = np.sqrt((1.0 - ac) / ac)                          # increasing in t
            rho, s_min, s_max = 7.0, table[0], table[-1]
            ramp = np.linspace(0, 1, n)
            ks = (s_max ** (1 / rho) + ramp * (s_min ** (1 / rho) - s_max ** (1 / rho))) ** rho
            ts = np.interp(np.log(ks), np.log(table), np.arange(self.num_train_timesteps, dtype=np.float64))
            sig = np.concatenate([ks, [s_min]])
            self.karras_sigmas = ks
            self.alpha = 1.0 / np.sqrt(1.0 + sig ** 2)
            self.sigma = sig * self.alpha
        else:
            ts = self._grid(n)
            _, first = np.unique(ts, return_index=True)
            ts = ts[np.sort(first)]
            at = np.concatenate([ac[ts], ac[:1]])
            self.karras_sigmas = None
            self.alpha, self.sigma = np.sqrt(at), np.sqrt(1.0 - at)
            ts = ts.astype(np.float64)
        self.timesteps = ts
        self.num_inference_steps = len(ts)
        return ts

    def dpm_program(self):
        """Per model evaluation i (float32 arrays, computed in float64): (UNet timestep, cx, ce, a, b0, b1) with
        x0 = cx * x + ce * m and x_next = a * x + b0 * x0 + b1 * x0_prev (m: the CFG-combined model output)."""
        n = self.num_inference_steps
        al, sg = self.alpha, self.sigma
        lam = np.log(al) - np.log(sg)
        cx, ce, a, b0, b1 = (np.zeros(n) for _ in range(5))
        for i in range(n):
            if self.prediction_type == "epsilon":
                cx[i], ce[i] = 1.0 / al[i], -sg[i] / al[i]
            else:
                cx[i], ce[i] = al[i], -sg[i]
            h = lam[i + 1] - lam[i]
            a[i] = sg[i + 1] / sg[i]
            w = -al[i + 1] * np.expm1(-h)                             # -alpha_t (e^-h - 1)
            first = i == 0 or (i == n - 1 and n < 15) or h == 0.0     # h == 0 (Karras' last step): D is multiplied by 0 anyway
            if first:
                b0[i] = w
            else:
                r = (lam[i] - lam[i - 1]) / h
                b0[i], b1[i] = w * (1.0 + 0.5 / r), -w * 0.5 / r
        f = lambda v: np.asarray(v, dtype=np.float32)
        return f(self.timesteps), f(cx), f(ce), f(a), f(b0), f(b1)


SCHEDULERS = {"DDIMScheduler": DDIMScheduler, "PNDMScheduler": PNDMScheduler,
              "DPMSolverMultistepScheduler": DPMSolverMultistepScheduler}


def scheduler_config_from_json(sj: dict, sched_name: str) -> SchedulerConfig:
    """`scheduler/scheduler_config.json` -> SchedulerConfig for the scheduler `sched_name` the pipeline will run (the JSON's own
    `_class_name`, or an override).  DPM solver keys are taken only from a DPM config (a PNDM / DDIM config converted by an override
    gets diffusers' DPM defaults, as `from_config` gives them); values DPMSolverMultistepScheduler does not implement raise ValueError."""
    sc = SchedulerConfig(sj.get("num_train_timesteps", 1000), sj.get("beta_start", 0.00085), sj.get("beta_end", 0.012),
                         sj.get("steps_offset", 1), sj.get("set_alpha_to_one", False), sj.get("prediction_type", "epsilon"),
                         # diffusers' PNDMScheduler defaults skip_prk_steps to False; SD checkpoints store True
                         # (that default applies only when the JSON itself is a PNDMScheduler config: an explicit scheduler="PNDMScheduler"
                         # override on a DDIM checkpoint has no such key and means the SD form, skip_prk_steps=True)
                         bool(sj.get("skip_prk_steps", False)) if sj.get("_class_name") == "PNDMScheduler" else True)
    if sched_name == "DPMSolverMultistepScheduler":
        own = sj.get("_class_name") == sched_name
        opts = {k: sj[k] for k in list(DPMSolverMultistepScheduler._ONLY) + ["lambda_min_clipped"] if own and k in sj}
        DPMSolverMultistepScheduler.check_options(opts)
        sc.use_karras_sigmas = bool(sj.get("use_karras_sigmas", False)) if own else False
        sc.timestep_spacing = sj.get("timestep_spacing", "linspace")
    if sched_name == "DDIMScheduler" and sj.get("_class_name") == sched_name:
        # a DDIM checkpoint's own spacing and beta rescale are honoured (they used to be run as "leading" / unrescaled, silently)
        sc.ddim_timestep_spacing = sj.get("timestep_spacing", "leading")
        sc.rescale_betas_zero_snr = bool(sj.get("rescale_betas_zero_snr", False))
        if sc.ddim_timestep_spacing not in DDIMScheduler._SPACINGS:
            raise ValueError(f"DDIMScheduler: timestep_spacing {sc.ddim_timestep_spacing!r} is not one of {DDIMScheduler._SPACINGS}")
    return sc


def scheduler_config_to_json(sched_name: str, sc: SchedulerConfig) -> dict:
    """The `scheduler_config.json` that reloads (scheduler_config_from_json) to scheduler `sched_name` with the options of `sc`."""
    sj = {"_class_name": sched_name, "num_train_timesteps": sc.num_train_timesteps, "beta_start": sc.beta_start, "beta_end": sc.beta_end,
          "beta_schedule": "scaled_linear", "steps_offset": sc.steps_offset, "set_alpha_to_one": sc.set_alpha_to_one,
          "prediction_type": sc.prediction_type}
    if sched_name == "DDIMScheduler":                  # written only off their defaults: every JSON written before them is unchanged
        if sc.ddim_timestep_spacing != "leading":
            sj["timestep_spacing"] = sc.ddim_timestep_spacing
        if sc.rescale_betas_zero_snr:
            sj["rescale_betas_zero_snr"] = True
    if sched_name == "PNDMScheduler":
        sj["skip_prk_steps"] = bool(sc.skip_prk_steps)
    if sched_name == "DPMSolverMultistepScheduler":
        sj.update(algorithm_type=sc.algorithm_type, solver_order=sc.solver_order, solver_type=sc.solver_type,
                  lower_order_final=sc.lower_order_final, use_karras_sigmas=sc.use_karras_sigmas, timestep_spacing=sc.timestep_spacing)
    return sj
