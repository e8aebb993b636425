"""Wall time of one txt2img denoise loop (SD-1.5 synthetic weights, 512 px, batch 4, CFG 7.5, DAAM recording on): DPM-Solver++ 2M
at --dpm-steps against DDIM at --ddim-steps, same pipeline, alternating runs; one JSON line per scheduler on stdout.

    python tools/dpm_timing.py [--dpm-steps 20] [--ddim-steps 50] [--repeats 3]

Only the loop is timed (set_context + recorder reset + the fused denoise, ended by a device synchronise); no VAE decode.
Under `rocprofv3 --kernel-trace --stats` the same run gives cfg_dpm_kernel's and cfg_ddim_kernel's per-launch times."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    from agenda_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    if not torch.cuda.is_available():
        raise SystemExit("dpm_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipe = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B = pipe.cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    runs = {"DDIMScheduler": (DDIMScheduler.from_config(cfg.sched), args.ddim_steps),
            "DPMSolverMultistepScheduler": (DPMSolverMultistepScheduler.from_config(cfg.sched), args.dpm_steps)}
    times = {k: [] for k in runs}
    with trace(pipe):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for name, (sched, steps) in runs.items():
                pipe.scheduler = sched
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent")
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                assert torch.isfinite(out.latents).all(), name
    for name, (_, steps) in runs.items():
        t = sorted(times[name])
        print(json.dumps({"scheduler": name, "steps": steps, "batch": B, "px": 512, "loop_ms_median": round(1e3 * t[len(t) // 2], 2),
                          "loop_ms_all": [round(1e3 * x, 2) for x in times[name]],
                          "ms_per_step": round(1e3 * t[len(t) // 2] / steps, 3)}))
    pipe.engine.close()


if __name__ == "__main__":
    main()
