"""Wall time of one txt2img denoise loop with guidance_rescale off and on (SD-1.5 synthetic weights, 512 px, batch 4, CFG 7.5, DDIM x
--steps, DAAM recording on): the same pipeline, plain and rescaled calls interleaved in one process; one JSON line per variant on stdout
(median, min and max over --repeats), then the rescale's cost per evaluation derived from the medians.

    python tools/guidance_rescale_timing.py [--steps 50] [--repeats 5] [--phi 0.7]

Only the loop is timed (set_context + recorder reset + the fused denoise, ended by a device synchronise); no VAE decode.  The expectation
to compare with comes from the code: one extra launch per evaluation -- one 1024-thread workgroup per image, two passes over that image's
2 x 16 384 eps floats (128 KB, the second pass out of L2) -- and one multiply in the step kernel: a few microseconds against an evaluation
of several milliseconds, so the rescaled loop should sit within the plain loop's own spread.  The kernel's own time per launch comes from
a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/guidance_rescale_timing.py --repeats 1

(its row is guidance_factor_kernel)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--phi", type=float, default=0.7)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    if not torch.cuda.is_available():
        raise SystemExit("guidance_rescale_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipe = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B = pipe.cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    times = {"plain": [], "rescaled": []}
    c0 = pipe.engine.guidance_rescale_counts()
    with trace(pipe):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for name in times:
                kw = {"guidance_rescale": args.phi} if name == "rescaled" else {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=args.steps, output_type="latent", **kw)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                assert torch.isfinite(out.latents).all()
    c1 = pipe.engine.guidance_rescale_counts()
    med = {}
    for name, t in times.items():
        t = sorted(t)
        med[name] = t[len(t) // 2]
        print(json.dumps({"scheduler": "DDIMScheduler", "variant": name, "steps": args.steps, "batch": B, "px": 512,
                          "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2)}))
    print(json.dumps({"plain_ms_per_evaluation": round(1e3 * med["plain"] / args.steps, 3),
                      "rescale_us_per_evaluation_over_plain": round(1e6 * (med["rescaled"] - med["plain"]) / args.steps, 2),
                      "rescale_over_plain_percent": round(100.0 * (med["rescaled"] - med["plain"]) / med["plain"], 3),
                      "factor_launches_per_evaluation": (c1 - c0) / ((args.repeats + 1) * args.steps), "phi": args.phi, "images": B}))
    pipe.engine.close()


if __name__ == "__main__":
    main()
