"""Wall time of one txt2img denoise loop without and with DeepCache (SD-1.5 synthetic weights, 512 px, batch 4, CFG 7.5, DAAM recording
on, DDIM x --ddim-steps and DPM-Solver++ x --dpm-steps): the same pipeline, the variants interleaved in one process; one JSON line per
(scheduler, variant) on stdout (median, min and max over --repeats), then each variant's loop time over the plain loop's from the medians.

    python tools/deepcache_timing.py [--ddim-steps 50] [--dpm-steps 20] [--repeats 5]

Variants: plain; cache_interval 2, 3 and 5 at branch 0; cache_interval 3 at branch 1.  Only the loop is timed (set_context + recorder reset
+ the fused denoise, ended by a device synchronise); no VAE decode.  Then, on the loop's 8 UNet rows through the engine's op seam: the
time of one plain forward, of one full forward that captures, and of one shallow forward at each branch (HIP events around --evals
back-to-back calls), and of the capture launch alone on its two regions at the loop's sizes (the activation 8 x 64 x 64 x 320 bf16 at
branch 0, x 640 at branch 1, and the 64-row-tile partial sums) -- that seam synchronises the stream after every launch, so its figure is
launch + host synchronise + kernel, an upper bound; the kernel's own time is its row of the kernel trace below.  The expectation to compare with comes from layer counts: a shallow
evaluation at branch 0 runs conv_in, one down layer, two up layers and conv_out, where the full walk runs conv_in, 8 down layers with 3
downsamplers, the mid block, 12 up layers with 3 upsamplers and conv_out -- but its layers are the ones on the 64 x 64 maps.  Per-kernel
times come from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/deepcache_timing.py --repeats 1

(the new row is deepcache_capture_kernel)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = (("plain", None), ("k2_b0", (2, 0)), ("k3_b0", (3, 0)), ("k5_b0", (5, 0)), ("k3_b1", (3, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--evals", type=int, default=10)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, _lib, synthetic, trace
    from agenda_amd.scheduler import SCHEDULERS
    if not torch.cuda.is_available():
        raise SystemExit("deepcache_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipe = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B = pipe.cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    for sched, steps in (("DDIMScheduler", args.ddim_steps), ("DPMSolverMultistepScheduler", args.dpm_steps)):
        pipe.scheduler = SCHEDULERS[sched].from_config(cfg.sched)
        times = {name: [] for name, _ in VARIANTS}
        counts = {}
        with trace(pipe):
            for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
                for name, kb in VARIANTS:
                    if kb is None:
                        pipe.disable_deepcache()
                    else:
                        pipe.enable_deepcache(cache_interval=kb[0], cache_branch_id=kb[1])
                    c0 = pipe.engine.deepcache_counts()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent")
                    torch.cuda.synchronize()
                    if rep:
                        times[name].append(time.perf_counter() - t0)
                    c1 = pipe.engine.deepcache_counts()
                    counts[name] = (c1[0] - c0[0], c1[1] - c0[1])
                    assert torch.isfinite(out.latents).all()
        pipe.disable_deepcache()
        med = {}
        for name, t in times.items():
            t = sorted(t)
            med[name] = t[len(t) // 2]
            print(json.dumps({"scheduler": sched, "variant": name, "steps": steps, "batch": B, "px": 512, "loop_ms_median": round(1e3 * med[name], 2),
                              "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2), "captures": counts[name][0],
                              "shallow_evaluations": counts[name][1]}))
        print(json.dumps({"scheduler": sched, "plain_ms_per_evaluation": round(1e3 * med["plain"] / steps, 3),
                          **{f"plain_over_{name}": round(med["plain"] / med[name], 3) for name in med if name != "plain"}}))

    # one evaluation of each kind on the loop's rows (the seam runs without the CFG-shared prefix; the loop shares it)
    eng = pipe.engine
    eng.set_context(ctx)
    eng.record_config(0)
    x = torch.cat([lat, lat]).cuda().contiguous()

    def timed(fn):
        fn(); fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.evals):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.evals
    one = {"forward_ms_plain": timed(lambda: eng.unet_forward(x, 501.0))}
    for b in (0, 1):
        one[f"forward_ms_full_with_capture_b{b}"] = timed(lambda: eng.deepcache_forward(x, 501.0, b, shallow=False))
        one[f"forward_ms_shallow_b{b}"] = timed(lambda: eng.deepcache_forward(x, 501.0, b, shallow=True))
    lib = _lib.load()
    for b, C in ((0, cfg.unet.block_out_channels[0]), (1, cfg.unet.block_out_channels[1])):
        act = torch.zeros(2 * B * 64 * 64 * C, dtype=torch.bfloat16, device="cuda")
        part = torch.zeros(2 * B * 64 * C * 2, dtype=torch.float32, device="cuda")
        d0, d1 = torch.empty_like(act), torch.empty_like(part)
        st = _lib.current_stream_ptr()
        one[f"capture_ms_b{b}"] = timed(lambda: _lib.check(lib.agd_op_deepcache_capture(None, _lib.ptr(act), _lib.ptr(d0), act.numel() * 2, _lib.ptr(part),
                                                                                         _lib.ptr(d1), part.numel() * 4, st), None, "capture"))
        one[f"capture_mbytes_b{b}"] = round((act.numel() * 2 + part.numel() * 4) / 1e6, 2)
    print(json.dumps({"rows": 2 * B, "px": 512, **{k: round(v, 4) for k, v in one.items()},
                      **{f"shallow_over_plain_b{b}": round(one[f"forward_ms_shallow_b{b}"] / one["forward_ms_plain"], 3) for b in (0, 1)}}))
    eng.close()


if __name__ == "__main__":
    main()
