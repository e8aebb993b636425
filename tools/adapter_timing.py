"""Wall time of one txt2img denoise loop under the plain pipeline, the T2I-Adapter pipeline and the ControlNet pipeline (SD-1.5 synthetic
weights on the same UNet, 512 px, batch 4, CFG 7.5, DDIM x --steps, DAAM recording on), interleaved in one process; one JSON line per
variant on stdout (median and spread over --repeats), then the once-per-call agd_adapter_set_cond_hw on its own and the adapter's cost
per evaluation derived from the medians.

    python tools/adapter_timing.py [--steps 50] [--repeats 5]

Only the loop is timed (set_context + recorder reset + the conditioning front end of the variant + the fused denoise, ended by a device
synchronise); no VAE decode.  The expectation to compare with comes from bytes: at UNet batch 8 the four adds read a bf16 activation and an
fp32 feature and write a bf16 activation, about 0.1 GB per evaluation -- tens of microseconds against an evaluation of several
milliseconds -- so the adapter loop should sit within the run-to-run spread of the plain one.  The add kernel's own time per launch comes
from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/adapter_timing.py --repeats 1

(its rows are the adapter_add_kernel instantiations)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def add_bytes(cfg, rows, L):
    """Algorithmic bytes of the four adds of one evaluation: per element 2 (h) + 4 (feature) + 2 (out)."""
    return sum(rows * (L >> i) * (L >> i) * c * 8 for i, c in enumerate(cfg.unet.block_out_channels))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionAdapterPipeline, StableDiffusionControlNetPipeline, StableDiffusionPipeline, synthetic, trace
    if not torch.cuda.is_available():
        raise SystemExit("adapter_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    kw = dict(seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    pipes = {"plain": StableDiffusionPipeline.from_synthetic("sd15", **kw), "adapter": StableDiffusionAdapterPipeline.from_synthetic("sd15", **kw),
             "controlnet": StableDiffusionControlNetPipeline.from_synthetic("sd15", **kw)}
    cfg, B = pipes["plain"].cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    img = torch.rand(B, 3, 512, 512, generator=torch.Generator().manual_seed(3)).cuda()
    times = {k: [] for k in pipes}
    sets = []
    with trace(pipes["plain"]), trace(pipes["adapter"]), trace(pipes["controlnet"]):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for name, pipe in pipes.items():
                extra = {} if name == "plain" else {"image": img}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=args.steps, output_type="latent", **extra)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                assert torch.isfinite(out.latents).all()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipes["adapter"].engine.adapter_set_cond(img)
            torch.cuda.synchronize()
            if rep:
                sets.append(time.perf_counter() - t0)
    med = {}
    for name, t in times.items():
        t = sorted(t)
        med[name] = t[len(t) // 2]
        print(json.dumps({"scheduler": "DDIMScheduler", "pipeline": name, "steps": args.steps, "batch": B, "px": 512,
                          "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2)}))
    s = sorted(sets)
    print(json.dumps({"plain_ms_per_evaluation": round(1e3 * med["plain"] / args.steps, 3),
                      "adapter_ms_per_evaluation_over_plain": round(1e3 * (med["adapter"] - med["plain"]) / args.steps, 4),
                      "controlnet_ms_per_evaluation_over_plain": round(1e3 * (med["controlnet"] - med["plain"]) / args.steps, 4),
                      "adapter_set_cond_ms_median": round(1e3 * s[len(s) // 2], 3), "adapter_set_cond_ms_min": round(1e3 * s[0], 3),
                      "add_bytes_per_evaluation": add_bytes(cfg, 2 * B, 64), "rows": 2 * B}))
    for p in pipes.values():
        p.engine.close()


if __name__ == "__main__":
    main()
