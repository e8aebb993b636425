"""Wall time of one region-based MultiDiffusion call against the same UNet rows as a plain batch.

SD-1.5 (synthetic weights), 512 x 512, DDIM x --steps, DAAM on: StableDiffusionRegionPipeline with R = 3 regions at B = 2 (6 UNet rows per
CFG half) and the plain pipeline at B = 6, interleaved in one process, --reps repeats each; the line per variant is the median
[min - max].  What the feature adds to the plain pipeline at equal rows is its three small launches per step (spread, masked mean, and the
DDIM step on R B rows instead of B), the mask front end and -- in the default call, the `backgrounds_encoded` line -- the once-per-call VAE encode of the
`bootstrapping` constant-colour backgrounds.  Per-kernel time: `rocprofv3 --kernel-trace --stats -- python tools/regions_timing.py --steps 10
--only regions` and read region_spread_kernel / region_mean_kernel; bytes per launch are printed here for the GB/s figure.

    python tools/regions_timing.py [--steps 50] [--reps 5] [--bootstrapping 20] [--only regions|plain]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bootstrapping", type=int, default=20)
    ap.add_argument("--only", choices=["regions", "plain"], default=None)
    a = ap.parse_args()
    from agenda_amd import StableDiffusionPipeline, StableDiffusionRegionPipeline, synthetic, trace
    pipe = StableDiffusionRegionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=24 << 30)
    cfg = pipe.cfg
    R, B, L = 3, 2, 64
    ctx = synthetic.make_context(cfg, R * B, seed=3)                      # [uncond x R B | cond x R B]
    RB = R * B
    pe = torch.cat([ctx[:B], ctx[RB:RB + B]], 0)
    rpe = torch.stack([torch.cat([ctx[r * B:(r + 1) * B], ctx[RB + r * B:RB + (r + 1) * B]], 0) for r in range(1, R)])
    lat = torch.randn(B, 4, L, L, generator=torch.Generator().manual_seed(1))
    lat6 = torch.randn(RB, 4, L, L, generator=torch.Generator().manual_seed(2))
    boxes = [[0.05, 0.1, 0.55, 0.6], [0.45, 0.4, 0.95, 0.9]]            # two overlapping boxes
    bgs = torch.randn(max(a.bootstrapping, 1), 4, L, L, generator=torch.Generator().manual_seed(4))

    def regions(encode):
        with trace(pipe) as trc:
            pipe(prompt_embeds=pe, region_prompt_embeds=rpe, region_boxes=boxes, bootstrapping=a.bootstrapping,
                 bootstrap_backgrounds=None if encode else bgs, latents=lat, num_inference_steps=a.steps, output_type="pt",
                 generator=torch.Generator().manual_seed(7))
            for p in range(B):
                trc.compute_region_word_heat_map("", image_index=p, word_idx=1)

    def plain():
        with trace(pipe) as trc:
            StableDiffusionPipeline.__call__(pipe, prompt_embeds=ctx, latents=lat6, num_inference_steps=a.steps, output_type="pt")
            for i in range(RB):
                trc.compute_global_heat_map(image_index=i)

    variants = {}
    if a.only != "plain":
        variants["regions_R3_B2_backgrounds_given_ms"] = lambda: regions(False)
        variants["regions_R3_B2_backgrounds_encoded_ms"] = lambda: regions(True)
    if a.only != "regions":
        variants["plain_B6_ms"] = plain
    for fn in variants.values():                                          # warm-up: buffers, staging, first touch
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):                                               # interleaved: every variant once per round
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"steps": a.steps, "reps": a.reps, "bootstrapping": a.bootstrapping, "rows_per_cfg_half": RB}
    for k, v in times.items():
        res[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(f"{k}: {statistics.median(v):.1f} [{min(v):.1f} - {max(v):.1f}]")
    img = 4 * L * L * 4
    res["spread_bytes_per_step"] = {"bootstrapped": (4 * RB - 2 * B) * img + (RB - B) * L * L * 4, "plain": 2 * RB * img}
    res["mean_bytes_per_step"] = RB * img + RB * L * L * 4 + B * img      # every region row and mask read once, the canvas written
    print(json.dumps(res))


if __name__ == "__main__":
    main()
