"""Wall time of one txt2img denoise loop without and with Semantic Guidance (SD-1.5 synthetic weights, 512 px, batch 4, CFG 7.5,
DDIM x --steps, DAAM recording on): the same pipeline, the variants interleaved in one process; one JSON line per variant on stdout (median,
min and max over --repeats), then each SEGA variant's cost over the plain loop derived from the medians.

    python tools/sega_timing.py [--steps 50] [--repeats 5] [--warmup-steps 10]

Variants: plain; one edit concept (K = 1); two edit concepts (K = 2), one of them reversed.  Only the loop is timed (set_context + recorder
reset + the fused denoise, ended by a device synchronise); no VAE decode.  Per evaluation a SEGA call runs, beside the usual 2 B-row walk,
one K B-row walk (at every evaluation: warm-up delays the addition, not the concept branch, and no cool-down is set), one copy launch, the
threshold launch and the fold launch.  Per-kernel times come from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/sega_timing.py --repeats 1

(the new rows are sega_threshold_kernel and sega_fold_kernel)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("plain", 0), ("sega_k1", 1), ("sega_k2", 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup-steps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    if not torch.cuda.is_available():
        raise SystemExit("sega_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipe = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B = pipe.cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    emb = torch.cat([synthetic.make_context(cfg, 1, seed=70 + k)[1:2] for k in range(2)])
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    times = {name: [] for name, _ in VARIANTS}
    counts = {name: [0, 0] for name, _ in VARIANTS}
    with trace(pipe):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for name, K in VARIANTS:
                kw = {}
                if K:
                    kw = {"editing_prompt_embeddings": emb[:K], "edit_warmup_steps": args.warmup_steps,
                          "reverse_editing_direction": [False, True][:K]}
                c0 = pipe.engine.sega_counts()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=args.steps, output_type="latent", **kw)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                c1 = pipe.engine.sega_counts()
                counts[name][0] += c1[0] - c0[0]
                counts[name][1] += c1[1] - c0[1]
                assert torch.isfinite(out.latents).all()
    med = {}
    evals = (args.repeats + 1) * args.steps
    for (name, K) in VARIANTS:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        print(json.dumps({"scheduler": "DDIMScheduler", "variant": name, "concepts": K, "steps": args.steps, "batch": B, "px": 512,
                          "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2),
                          "concept_walks_per_evaluation": counts[name][0] / evals, "folds_per_evaluation": counts[name][1] / evals}))
    print(json.dumps({"plain_ms_per_evaluation": round(1e3 * med["plain"] / args.steps, 3), "images": B,
                      **{f"{name}_over_plain_percent": round(100.0 * (med[name] - med["plain"]) / med["plain"], 2) for name in med if name != "plain"},
                      **{f"{name}_ms_per_evaluation_over_plain": round(1e3 * (med[name] - med["plain"]) / args.steps, 3) for name in med if name != "plain"}}))
    pipe.engine.close()


if __name__ == "__main__":
    main()
