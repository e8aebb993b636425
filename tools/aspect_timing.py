"""Wall time of one txt2img call per output size (SD-1.5 synthetic weights, batch 4, DDIM x --steps, CFG 7.5, DAAM recording on,
VAE decode included): 512x512, 512x768, 768x512 and 768x768 interleaved in one process; one JSON line per size on stdout with the
median wall ms per batch over --repeats and ms per megapixel of output.

    python tools/aspect_timing.py [--steps 50] [--batch 4] [--repeats 3]

Landscape latents (width 96 / 48 / 24 / 12) fall back from the row-halo conv kernels to the general ones; portrait latents (width 64)
keep them with Hout != Wout.  The sizes are measured as they are, nothing is tuned for them."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(512, 512), (512, 768), (768, 512), (768, 768)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    if not torch.cuda.is_available():
        raise SystemExit("aspect_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipe = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=24 << 30)
    cfg, B = pipe.cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lats = {}
    for h, w in SIZES:
        g = torch.Generator().manual_seed(h * 10 + w)
        lats[(h, w)] = torch.randn(B, cfg.unet.out_channels, h // 8, w // 8, generator=g)

    def once(h, w):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with trace(pipe):
            pipe(prompt_embeds=ctx, latents=lats[(h, w)], num_inference_steps=args.steps, height=h, width=w, output_type="pt")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for hw in SIZES:                                   # warm every size once (buffers, coefficient tables)
        once(*hw)
    times = {hw: [] for hw in SIZES}
    for _ in range(args.repeats):
        for hw in SIZES:
            times[hw].append(once(*hw))
    for (h, w) in SIZES:
        ms = statistics.median(times[(h, w)])
        mp = B * h * w / 1e6
        print(json.dumps({"size": f"{h}x{w}", "batch": B, "ddim_steps": args.steps, "daam": True, "wall_ms_per_batch": round(ms, 1),
                          "ms_per_megapixel": round(ms / mp, 1), "spread_ms": round(max(times[(h, w)]) - min(times[(h, w)]), 1)}))
    pipe.engine.close()


if __name__ == "__main__":
    main()
