"""Wall time of one txt2img denoise loop with and without GLIGEN grounding (SD-1.5 synthetic weights with a PositionNet and 16 fusers,
512 px, batch 4, CFG 7.5, DAAM recording on): DDIM x --steps at gligen_scheduled_sampling_beta = --beta against the plain pipeline on the
same UNet, interleaved in one process; one JSON line per variant on stdout (median and spread over --repeats), the cost per grounded
evaluation derived from the two, and the once-per-call agd_gligen_set (PositionNet + every fuser's grounding K/V) on its own.

    python tools/gligen_timing.py [--steps 50] [--beta 0.3] [--repeats 5]

Only the loop is timed (set_context + recorder reset + agd_gligen_set when grounded + the fused denoise, ended by a device synchronise);
no VAE decode.  The new attention instantiation's time per launch comes from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/gligen_timing.py --repeats 1

(its rows are the attn_kernel instantiations whose last template argument is 1)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--beta", type=float, default=0.3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionGLIGENPipeline, StableDiffusionPipeline, synthetic, trace
    from agenda_amd.gligen import grounding_flags
    if not torch.cuda.is_available():
        raise SystemExit("gligen_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    gl = StableDiffusionGLIGENPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    plain = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B = gl.cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    phrases = ["a car", "a car", "a truck", "a bus", "a car"]
    boxes = [[0.05, 0.1, 0.25, 0.3], [0.3, 0.1, 0.5, 0.3], [0.55, 0.4, 0.9, 0.7], [0.1, 0.6, 0.45, 0.95], [0.7, 0.05, 0.95, 0.3]]
    times = {False: [], True: []}
    sets = []
    with trace(plain), trace(gl):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for grounded in (False, True):
                pipe = gl if grounded else plain
                kw = dict(gligen_phrases=phrases, gligen_boxes=boxes, gligen_scheduled_sampling_beta=args.beta) if grounded else {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=args.steps, output_type="latent", **kw)
                torch.cuda.synchronize()
                if rep:
                    times[grounded].append(time.perf_counter() - t0)
                assert torch.isfinite(out.latents).all()
            from agenda_amd.gligen import object_tensors
            lays = [(phrases, boxes)] * B
            objs = object_tensors(lays, gl.pooled_phrase_embeddings(phrases), cfg.unet.cross_attention_dim)
            objs = tuple(t.cuda() for t in objs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gl.engine.gligen_set(*objs)
            torch.cuda.synchronize()
            if rep:
                sets.append(time.perf_counter() - t0)
    med = {}
    for grounded, t in times.items():
        t = sorted(t)
        med[grounded] = t[len(t) // 2]
        print(json.dumps({"scheduler": "DDIMScheduler", "gligen": grounded, "beta": args.beta if grounded else None, "steps": args.steps,
                          "batch": B, "px": 512, "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2),
                          "loop_ms_max": round(1e3 * t[-1], 2)}))
    n_g = sum(grounding_flags(args.beta, args.steps))
    s = sorted(sets)
    print(json.dumps({"grounded_evaluations": n_g, "ms_per_grounded_evaluation": round(1e3 * (med[True] - med[False]) / max(n_g, 1), 3),
                      "plain_ms_per_evaluation": round(1e3 * med[False] / args.steps, 3),
                      "gligen_set_ms_median": round(1e3 * s[len(s) // 2], 3), "gligen_set_ms_min": round(1e3 * s[0], 3), "rows": 2 * B}))
    gl.engine.close()
    plain.engine.close()


if __name__ == "__main__":
    main()
