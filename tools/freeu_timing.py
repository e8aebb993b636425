"""Wall time of one txt2img denoise loop with FreeU off and on (SD-1.5 synthetic weights, 512 px, batch 4, CFG 7.5, DDIM x --steps, DAAM
recording on): the same pipeline, plain and FreeU calls interleaved in one process; one JSON line per variant on stdout (median and spread
over --repeats), then FreeU's cost per evaluation derived from the medians.

    python tools/freeu_timing.py [--steps 50] [--repeats 5]

Only the loop is timed (set_context + recorder reset + the fused denoise, ended by a device synchronise); no VAE decode.  The expectation
to compare with comes from the code: six launches per evaluation (one per resnet of up blocks 0 and 1), each over a few hundred workgroups
that read and write 8 x 8 or 16 x 16 maps -- ten to twenty microseconds apiece against an evaluation of several milliseconds -- so the FreeU
loop should sit within one percent of the plain one.  The kernel's own time per launch comes from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/freeu_timing.py --repeats 1

(its row is freeu_kernel)."""
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
    ap.add_argument("--freeu", type=float, nargs=4, default=[0.9, 0.2, 1.5, 1.6], metavar=("S1", "S2", "B1", "B2"))
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    if not torch.cuda.is_available():
        raise SystemExit("freeu_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipe = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B = pipe.cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    times = {"plain": [], "freeu": []}
    c0 = pipe.engine.freeu_counts()
    with trace(pipe):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for name in times:
                if name == "freeu":
                    pipe.enable_freeu(*args.freeu)
                else:
                    pipe.disable_freeu()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=args.steps, output_type="latent")
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                assert torch.isfinite(out.latents).all()
    c1 = pipe.engine.freeu_counts()
    med = {}
    for name, t in times.items():
        t = sorted(t)
        med[name] = t[len(t) // 2]
        print(json.dumps({"scheduler": "DDIMScheduler", "variant": name, "steps": args.steps, "batch": B, "px": 512,
                          "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2)}))
    launches = (c1[0] - c0[0] + c1[1] - c0[1]) / ((args.repeats + 1) * args.steps)
    print(json.dumps({"plain_ms_per_evaluation": round(1e3 * med["plain"] / args.steps, 3),
                      "freeu_ms_per_evaluation_over_plain": round(1e3 * (med["freeu"] - med["plain"]) / args.steps, 4),
                      "freeu_over_plain_percent": round(100.0 * (med["freeu"] - med["plain"]) / med["plain"], 3),
                      "freeu_launches_per_evaluation": launches, "freeu": args.freeu, "rows": 2 * B}))
    pipe.engine.close()


if __name__ == "__main__":
    main()
