"""Wall time of one MultiDiffusion panorama against the same UNet work as a plain batch.

SD-1.5 (synthetic weights), 512 x 2048, B = 1, DDIM x --steps, DAAM on: StableDiffusionPanoramaPipeline with view_batch_size=None and 1,
and the plain pipeline at batch 25, 512 x 512 in the same process (25 views = the same UNet work per step).  The difference between the
first and the last is the cost of the feature's own kernels (window gather, overlap mean, context tiling) and of projecting the tiled
context.  Per-kernel time: `rocprofv3 --kernel-trace --stats -- python tools/panorama_timing.py --steps 10 --only panorama` and read
window_gather_kernel / window_mean_kernel; bytes per launch are printed here for the GB/s figure.

    python tools/panorama_timing.py [--steps 50] [--reps 2] [--only panorama|plain]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    fn()                                                  # warm-up: buffers, staging, first-touch
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", choices=["panorama", "plain"], default=None)
    a = ap.parse_args()
    from agenda_amd import StableDiffusionPanoramaPipeline, get_views, synthetic, trace
    pipe = StableDiffusionPanoramaPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=24 << 30)
    cfg = pipe.cfg
    H, W = 512, 2048
    V = len(get_views(H, W))
    res = {"steps": a.steps, "views": V}
    ctx1 = synthetic.make_context(cfg, 1, seed=3)
    lat = torch.randn(1, 4, H // 8, W // 8, generator=torch.Generator().manual_seed(1))

    def pano(vb):
        with trace(pipe) as trc:
            pipe(prompt_embeds=ctx1, latents=lat, num_inference_steps=a.steps, height=H, width=W, view_batch_size=vb, output_type="pt")
            trc.compute_global_heat_map(image_index=0)

    if a.only != "plain":
        res["panorama_ms_all_views"] = timed(lambda: pano(None), a.reps)
        if a.only is None:
            res["panorama_ms_view_batch_1"] = timed(lambda: pano(1), 1)
    if a.only != "panorama":
        from agenda_amd import StableDiffusionPipeline
        ctxv = torch.cat([ctx1[:1].repeat(V, 1, 1), ctx1[1:].repeat(V, 1, 1)])
        latv = torch.randn(V, 4, 64, 64, generator=torch.Generator().manual_seed(2))

        def plain():
            with trace(pipe) as trc:
                StableDiffusionPipeline.__call__(pipe, prompt_embeds=ctxv, latents=latv, num_inference_steps=a.steps, output_type="pt")
                for i in range(V):
                    trc.compute_global_heat_map(image_index=i)

        res[f"plain_batch{V}_512_ms"] = timed(plain, a.reps)
    img = 4 * 64 * 64 * 4
    res["gather_bytes_per_step"] = 2 * V * img                                    # read + write of every view
    res["mean_bytes_per_step"] = V * img + 4 * (H // 8) * (W // 8) * 4            # every view read once, the canvas written
    print(json.dumps(res))


if __name__ == "__main__":
    main()
