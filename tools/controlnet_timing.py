"""Wall time of one txt2img denoise loop with and without a ControlNet (SD-1.5 synthetic weights, 512 px, batch 4, CFG 7.5, DAAM
recording on): DDIM x --ddim-steps and DPM-Solver++ 2M x --dpm-steps, each plain and ControlNet-conditioned, the four variants
interleaved in one process; one JSON line per variant on stdout (median and spread over --repeats), plus the once-per-call
conditioning embedding on its own.

    python tools/controlnet_timing.py [--ddim-steps 50] [--dpm-steps 20] [--repeats 5]

Only the loop is timed (set_context + recorder reset + the embedding when conditioned + the fused denoise, ended by a device
synchronise); no VAE decode.  The plain variants run on a StableDiffusionPipeline with the same UNet weights."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionControlNetPipeline, StableDiffusionPipeline, synthetic, trace
    from agenda_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    if not torch.cuda.is_available():
        raise SystemExit("controlnet_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    cn = StableDiffusionControlNetPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    plain = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B = cn.cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    image = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(3))
    scheds = {"DDIMScheduler": (DDIMScheduler, args.ddim_steps), "DPMSolverMultistepScheduler": (DPMSolverMultistepScheduler, args.dpm_steps)}
    variants = [(s, c) for s in scheds for c in (False, True)]
    times = {v: [] for v in variants}
    emb = []
    with trace(plain), trace(cn):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for name, controlled in variants:
                pipe = cn if controlled else plain
                cls, steps = scheds[name]
                pipe.scheduler = cls.from_config(cfg.sched)
                kw = {"image": image} if controlled else {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", **kw)
                torch.cuda.synchronize()
                if rep:
                    times[(name, controlled)].append(time.perf_counter() - t0)
                assert torch.isfinite(out.latents).all(), name
            cond = image.repeat_interleave(B, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cn.engine.controlnet_set_cond(cond, repeat=2)
            torch.cuda.synchronize()
            if rep:
                emb.append(time.perf_counter() - t0)
    for (name, controlled), t in times.items():
        t = sorted(t)
        steps = scheds[name][1]
        print(json.dumps({"scheduler": name, "controlnet": controlled, "steps": steps, "batch": B, "px": 512,
                          "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2),
                          "ms_per_step": round(1e3 * t[len(t) // 2] / steps, 3)}))
    e = sorted(emb)
    print(json.dumps({"conditioning_embedding_ms_median": round(1e3 * e[len(e) // 2], 3), "min": round(1e3 * e[0], 3), "max": round(1e3 * e[-1], 3),
                      "rows": 2 * B, "px": 512}))
    cn.engine.close()
    plain.engine.close()


if __name__ == "__main__":
    main()
