"""LoRA timings at SD-1.5 (synthetic weights), 512 px, batch 4, a rank-32 LoRA on every UNet target: load_lora_weights, one scale change
(merge + in-place re-derivation), and DDIM x 50 / DPM-Solver++ 2M x 20 with and without the LoRA.  Prints one JSON line of
median [min, max] in ms, and the bytes the base copies and factors take.

    python tools/lora_timing.py [--reps 5] [--rank 32]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(xs[len(xs) // 2], 2), "min_ms": round(xs[0], 2), "max_ms": round(xs[-1], 2), "n": len(xs)}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    from agenda_amd import StableDiffusionPipeline, config, lora, synthetic
    from agenda_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    cfg = config.sd15()
    pipe = StableDiffusionPipeline.from_synthetic(cfg)
    g = torch.Generator().manual_seed(0)
    sd, n_params = {}, 0
    for m, (_, (n_out, n_in)) in lora.target_modules(cfg).items():
        k = "lora_unet_" + m.replace(".", "_")
        sd[k + ".lora_down.weight"] = torch.randn(a.rank, n_in, generator=g) / n_in ** 0.5
        sd[k + ".lora_up.weight"] = torch.randn(n_out, a.rank, generator=g) * 0.02
        sd[k + ".alpha"] = torch.tensor(a.rank / 2.0)
        n_params += n_out * n_in
    ctx = synthetic.make_context(cfg, a.batch, seed=7)
    lat = synthetic.make_latents(cfg, list(range(a.batch)), 64)

    def run(sched, steps, scale):
        pipe.scheduler = sched
        kw = {"cross_attention_kwargs": {"scale": scale}} if scale is not None else {}
        return _timed(lambda: pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", **kw))

    ddim, dpm = DDIMScheduler.from_config(cfg.sched), DPMSolverMultistepScheduler.from_config(cfg.sched)
    res = {"config": "sd15 512px", "batch": a.batch, "rank": a.rank, "targets": len(sd) // 3, "target_params": n_params,
           "base_copy_bytes": 2 * n_params}
    for name, sched, steps in (("ddim50", ddim, 50), ("dpm20", dpm, 20)):
        run(sched, steps, None)
        res[name + "_base"] = _stats([run(sched, steps, None) for _ in range(a.reps)])
    free0 = torch.cuda.mem_get_info()[0]
    loads = []
    for _ in range(a.reps):
        loads.append(_timed(lambda: pipe.load_lora_weights(sd)))
    res["load_lora_weights"] = _stats(loads)
    res["lora_state_bytes"] = free0 - torch.cuda.mem_get_info()[0]
    changes = []
    for i in range(2 * a.reps + 1):
        s = 1.0 if i % 2 == 0 else 0.5
        changes.append(_timed(lambda: pipe.engine.lora_set_scale(s)))
    res["scale_change"] = _stats(changes[1:])
    for name, sched, steps in (("ddim50", ddim, 50), ("dpm20", dpm, 20)):
        run(sched, steps, 1.0)
        res[name + "_lora"] = _stats([run(sched, steps, 1.0) for _ in range(a.reps)])
    pipe.unload_lora_weights()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
