"""Records what the engine's entry points refuse and compute under every conditioning state, in the form of
tests/golden/conditioning_parent.npz: ControlNet, GLIGEN, T2I-Adapter, IP-Adapter, inpainting and InstructPix2Pix set alone, in pairs and
misfitted, through unet_forward (one timestep and one per image), the three fused loops and the panorama -- the full message of every
refusal ("" where the call runs), the latents / eps of the calls that run, and their launches per kernel class.

    python tools/record_conditioning.py OUT.npz [--compare tests/golden/conditioning_parent.npz]

Everything runs on config.tiny(), 2 images (4 CFG rows) at latent 16 x 16 unless a case says otherwise, on three engines: `e4` (the 4-channel
UNet with a ControlNet, GLIGEN fusers, a T2I-Adapter and an IP-Adapter loaded), `e8` (config.ip2p_variant, the same four loaded) and `e9`
(config.inpaint_variant).  On e8 the schedules are all zero -- set, but nothing beside the UNet runs.

The committed file was written by this script in a checkout of commit 00fefd3 ("Add IP-Adapter image prompts with decoupled attention on
the device"), the last one whose entry points resolved their conditioning with one helper per feature, built for gfx950 and run on one
MI355X; two runs there gave identical files.  It uses only the Engine API and weight makers of that commit, so the recording can be made
again there; tests/test_conditioning_gpu.py replays record() on the current build and compares bit for bit."""
import argparse
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, L, E = 2, 16, 96                                       # images, latent side, the IP-Adapter's embed_dim
DDIM2 = ([500, 1], [0.5, 0.9], [0.9, 0.99])               # a two-evaluation DDIM program
STATES = ("cn", "gl", "inp", "i2p", "ad", "ipa")


def _randn(seed, *shape):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rand(seed, *shape):
    import torch
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


class Rig:
    """One engine with its models loaded, and the cases' way of setting one state so that it fits a call of n evaluations."""

    def __init__(self, cfg, extras):
        from agenda_amd import config, synthetic
        from agenda_amd import gligen as G
        from agenda_amd import ip_adapter as A
        from agenda_amd.pipeline import Engine
        kw = dict(bias_std=0.05, perturb_norm=0.1)
        self.cfg, self.extras = cfg, extras
        self.cin = cfg.unet.in_channels
        self.states = [s for s in STATES if (s in ("cn", "gl", "ad", "ipa") and extras) or s == "inp" or (s == "i2p" and self.cin == 8)]
        e = self.e = Engine(cfg, 0, 1 << 30)
        e.load_state_dict(synthetic.make_unet_weights(cfg, 11, **kw), "unet.")
        e.load_state_dict(synthetic.make_vae_weights(cfg, 12, **kw), "vae.")
        if extras:
            e.controlnet_configure(config.ControlNetConfig())
            e.load_state_dict(synthetic.make_controlnet_weights(cfg, seed=13, **kw), "controlnet.")
            e.gligen_configure(cfg.unet.cross_attention_dim, G.MAX_OBJS, G.FOURIER_FREQS)
            e.load_state_dict(G.make_gligen_weights(cfg, 14), "unet.")
            acfg = config.adapter_config_for(cfg.unet)
            e.adapter_configure(acfg)
            e.load_state_dict(synthetic.make_adapter_weights(cfg, acfg, 15, bias_std=0.05), "adapter.")
        e.finalize()
        if extras:
            tensors, _, nt = A.to_engine_tensors(A.make_ip_adapter_weights(cfg, 21, E), cfg)
            e.ip_adapter_load(tensors, E, nt)
        self.context(B)

    def context(self, images):
        from agenda_amd import synthetic
        self.e.set_context(synthetic.make_context(self.cfg, images, seed=1))

    def clear(self):
        e = self.e
        e.inpaint_clear(); e.ip2p_clear()
        if self.extras:
            e.controlnet_set_schedule([]); e.gligen_clear(); e.adapter_clear(); e.ip_adapter_clear()

    def set(self, s, n, images=B, Lh=L, Lw=L, length=None):
        """State s for `images` images at Lh x Lw with a schedule of `length` (default n) entries; e4's schedules mix a zero and a non-zero."""
        import torch
        e, live, D = self.e, self.cin == 4, self.cfg.unet.cross_attention_dim
        m = n if length is None else length
        if s == "cn":
            e.controlnet_set_cond(_rand(31, images, 3, 8 * Lh, 8 * Lw), repeat=2)
            e.controlnet_set_schedule([1.0 if live and i % 2 == 0 else 0.0 for i in range(m)])
        elif s == "gl":
            boxes = torch.zeros(2 * images, 30, 4); boxes[:, 0] = torch.tensor([0.1, 0.2, 0.6, 0.7]); boxes[:, 1] = torch.tensor([0.5, 0.4, 0.9, 0.95])
            masks = torch.zeros(2 * images, 30); masks[images:, :2] = 1
            e.gligen_set(boxes, _randn(32, 2 * images, 30, D), masks)
            e.gligen_set_schedule([1 if live and i % 2 == 0 else 0 for i in range(m)])
        elif s == "ad":
            e.adapter_set_cond(_rand(33, images, 3, 8 * Lh, 8 * Lw))
            e.adapter_set_schedule([0.5 if live and i % 2 == 0 else 0.0 for i in range(m)])
        elif s == "ipa":
            e.ip_adapter_set(_randn(34, 2 * images, E).to(torch.bfloat16).float(), 0.6)
        elif s == "inp":
            mask = (_rand(35, images, 1, Lh, Lw) > 0.5).float()
            if live:
                e.inpaint_set(mask, _randn(36, images, 4, Lh, Lw), _randn(37, images, 4, Lh, Lw))
                e.inpaint_set_schedule([(0.9, 0.1), (0.7, 0.3), (0.5, 0.5)][:m])
            else:
                e.inpaint_set(mask, _randn(36, images, self.cin - 5, Lh, Lw))
        elif s == "i2p":
            e.ip2p_set(_randn(38, images, 4, Lh, Lw), 1.5)

    # ---- the callers ----
    def forward(self, per_image=False, Lh=L, Lw=L):
        return self.e.unet_forward(_randn(41, 2 * B, self.cin, Lh, Lw).cuda(), [11.0, 12.0, 13.0, 14.0] if per_image else 11.0)

    def denoise(self, images=B, Lh=L, Lw=L):
        return self.e.denoise(_randn(42, images, 4, Lh, Lw).cuda(), *DDIM2, 7.5)

    def plms(self):
        from agenda_amd.scheduler import PNDMScheduler
        sch = PNDMScheduler.from_config(self.cfg.sched); sch.set_timesteps(2)
        return self.e.denoise_plms(_randn(42, B, 4, L, L).cuda(), *sch.plms_program(), 7.5)

    def dpm(self):
        from agenda_amd.scheduler import DPMSolverMultistepScheduler
        sch = DPMSolverMultistepScheduler.from_config(self.cfg.sched); sch.set_timesteps(2)
        return self.e.denoise_dpm(_randn(42, B, 4, L, L).cuda(), *sch.dpm_program(), 7.5)

    def panorama(self):
        return self.e.denoise_panorama(_randn(43, B, 4, L, 2 * L).cuda(), 16, 8, None, *DDIM2, 7.5)

    CALLERS = {"unet_forward": (forward, 1), "unet_forward_ts": (lambda self: self.forward(per_image=True), 1), "denoise": (denoise, 2),
               "denoise_panorama": (panorama, 2)}


def record():
    """{name: array}: "refusal/<case>" (a string), "out/<case>" (fp32), "launches/<case>" (int64, in `classes` order)."""
    import torch
    from agenda_amd import config
    from agenda_amd._lib import AgendaHipError
    rec = {}

    def refusal(name, rig, call):
        """Runs `call` on the states the case has set and records its refusal; the states are cleared afterwards."""
        try:
            call()
            torch.cuda.synchronize()
            rec["refusal/" + name] = np.array("")
        except AgendaHipError as err:
            if "illegal memory access" in str(err):                 # a device fault is no refusal: nothing more runs
                raise
            rec["refusal/" + name] = np.array(str(err))
        except Exception as err:                                    # not the engine's: recorded by type, so that a comparison shows it
            rec["refusal/" + name] = np.array(f"{type(err).__name__}: {err}")
        rig.clear()

    def output(name, rig, call):
        rig.e.profile_begin()
        out = call()
        torch.cuda.synchronize()
        prof = rig.e.profile_end()
        rec.setdefault("classes", np.array(sorted(prof)))
        rec["out/" + name] = out.cpu().numpy()
        rec["launches/" + name] = np.array([prof[k]["launches"] for k in sorted(prof)], dtype=np.int64)
        rig.clear()

    def cells(tag, rig):
        """Every caller with nothing set, each state alone, and for unet_forward / denoise each pair of states (every state is set so that
        it fits the call; the 8-channel UNet's loops fit no call without the ip2p state, so there the pairs are the ip2p state's)."""
        for caller, (fn, n) in Rig.CALLERS.items():
            combos = [()] + [(s,) for s in rig.states]
            if caller in ("unet_forward", "denoise"):
                combos += [p for p in itertools.combinations(rig.states, 2) if caller == "unet_forward" or rig.cin != 8 or "i2p" in p]
            for combo in combos:
                for s in combo:
                    rig.set(s, n)
                refusal(f"{tag}/{caller}/{'+'.join(combo) or 'none'}", rig, lambda: fn(rig))

    e4 = Rig(config.tiny(), True)
    cells("e4", e4)
    # the fused loops share one path: PLMS runs 3 evaluations, DPM 2
    for name, fn, n in (("plms", e4.plms, 3), ("dpm", e4.dpm, 2)):
        e4.set("cn", n); e4.set("ad", n)
        refusal(f"e4/{name}/cn+ad", e4, fn)
    # states that do not fit the call: schedule lengths, rows, latent sizes
    for s in ("cn", "gl", "ad", "inp"):
        e4.set(s, 2, length=3)
        refusal(f"e4/denoise/{s}-length", e4, e4.denoise)
        e4.set(s, 1, length=2)
        refusal(f"e4/unet_forward/{s}-length", e4, e4.forward)
    for s in ("cn", "gl", "ipa", "inp"):
        if s == "gl":                                               # (the grounding objects are set for the context's rows)
            e4.context(1)
        e4.set(s, 2, images=1)
        e4.context(B)
        refusal(f"e4/denoise/{s}-rows", e4, e4.denoise)
    e4.set("ad", 2, images=3)
    refusal("e4/denoise/ad-rows", e4, e4.denoise)
    for s in ("cn", "ad", "inp"):
        e4.set(s, 2, Lh=16, Lw=24)
        refusal(f"e4/denoise/{s}-size", e4, e4.denoise)
    e4.set("ad", 1, images=3)
    refusal("e4/unet_forward/ad-rows", e4, e4.forward)
    e4.set("ipa", 1, images=1)
    refusal("e4/unet_forward/ipa-rows", e4, e4.forward)
    # a context for another batch beside a set state
    e4.context(1)
    for s in ("cn", "ad", "ipa"):
        e4.set(s, 2)
        refusal(f"e4/denoise/{s}-context", e4, e4.denoise)
    e4.context(B)

    # ---- what the calls that run compute, and what they launch ----
    output("e4/denoise/plain", e4, e4.denoise)
    for combo in (("cn",), ("gl",), ("cn", "gl"), ("ad",), ("ipa",), ("inp",), ("inp", "gl")):
        for s in combo:
            e4.set(s, 2)
        output("e4/denoise/" + "+".join(combo), e4, e4.denoise)
    for name, fn, n in (("plms", e4.plms, 3), ("dpm", e4.dpm, 2)):
        output(f"e4/{name}/plain", e4, fn)
        e4.set("cn", n)
        output(f"e4/{name}/cn", e4, fn)
    e4.set("ad", 2, Lh=16, Lw=24)
    output("e4/denoise/ad-16x24", e4, lambda: e4.denoise(Lh=16, Lw=24))
    output("e4/unet_forward/plain", e4, e4.forward)
    for s in ("cn", "gl", "ad", "ipa"):
        e4.set(s, 1)
        output("e4/unet_forward/" + s, e4, e4.forward)
    output("e4/unet_forward_ts/plain", e4, lambda: e4.forward(per_image=True))
    output("e4/denoise_panorama/plain", e4, e4.panorama)
    # a LoRA scale change after the image products were built leaves them stale (last: it rewrites e4's weights)
    from agenda_amd.lora import target_modules
    key, (n_out, n_in) = next(v for k, v in sorted(target_modules(e4.cfg).items()) if k.endswith("attn2.to_q"))
    e4.e.lora_add(key, _randn(51, 4, n_in), _randn(52, n_out, 4), 4.0)
    e4.e.lora_set_scale(1.0)
    e4.set("ipa", 1)
    e4.e.lora_set_scale(0.5)
    e4.context(B)
    refusal("e4/unet_forward/ipa-stale", e4, e4.forward)
    e4.e.close()

    e8 = Rig(config.ip2p_variant(config.tiny()), True)
    cells("e8", e8)
    for name, fn, n in (("plms", e8.plms, 3), ("dpm", e8.dpm, 2)):
        e8.set("i2p", n); e8.set("gl", n)
        refusal(f"e8/{name}/i2p+gl", e8, fn)
    e8.set("i2p", 2, Lh=16, Lw=24)
    refusal("e8/denoise/i2p-size", e8, e8.denoise)
    e8.set("i2p", 2, images=1)
    refusal("e8/denoise/i2p-rows", e8, e8.denoise)
    e8.context(1)
    e8.set("i2p", 2)
    refusal("e8/denoise/i2p-context", e8, e8.denoise)
    e8.set("i2p", 2); e8.set("cn", 2)
    refusal("e8/denoise/i2p+cn-context", e8, e8.denoise)
    e8.context(B)
    e8.set("i2p", 2)
    output("e8/denoise/i2p", e8, e8.denoise)
    e8.e.close()

    e9 = Rig(config.inpaint_variant(config.tiny()), False)
    cells("e9", e9)
    e9.set("inp", 2)
    output("e9/denoise/inp", e9, e9.denoise)
    e9.e.close()
    return rec


def differences(rec, old):
    """The names whose arrays are not identical (or are missing on one side)."""
    names = sorted(set(rec) | set(old.files))
    return [k for k in names if k not in rec or k not in old.files or rec[k].dtype.kind != old[k].dtype.kind or not np.array_equal(rec[k], old[k])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--compare", help="an earlier recording; exit status 1 unless every array is bit-identical")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("record_conditioning: no GPU visible")
    rec = record()
    np.savez_compressed(args.out, **rec)
    n = sum(k.startswith("refusal/") for k in rec)
    print(f"{n} refusal cases ({sum(bool(str(rec[k])) for k in rec if k.startswith('refusal/'))} refused), {sum(k.startswith('out/') for k in rec)} outputs")
    if args.compare:
        diff = differences(rec, np.load(args.compare))
        print("differences:", diff or "none")
        for k in diff:
            if k.startswith("refusal/"):
                print(f"  {k}: {str(rec.get(k))!r}")
        if diff:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
