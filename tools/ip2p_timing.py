"""Wall time of one fused denoise loop for txt2img and InstructPix2Pix (SD-1.5 synthetic weights, 512 px, batch 4, guidance 7.5, image
guidance 1.5, DAAM recording on): DDIM x --steps, the two variants interleaved in one process; one JSON line per variant on stdout
(median and spread over --repeats), plus the once-per-call front end (image kernel + one VAE encode of the batch) on its own.

    python tools/ip2p_timing.py [--steps 50] [--repeats 5]

Only the fused loop is timed (the engine's denoise call, between two device synchronises); the InstructPix2Pix variant runs through the
pipeline, so its state is set exactly as a user's call sets it.  It has its own UNet (same seed, conv_in 8 channels wide).  The UNet runs
3 B rows per evaluation instead of 2 B, so about 1.5 x the txt2img loop is the figure to compare with."""
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
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionInstructPix2PixPipeline, StableDiffusionPipeline, synthetic, trace
    if not torch.cuda.is_available():
        raise SystemExit("ip2p_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipes = {"txt2img": StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30),
             "ip2p": StableDiffusionInstructPix2PixPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)}
    loop_s = []

    def timed(fn):
        def run(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **kw)
            torch.cuda.synchronize()
            loop_s.append(time.perf_counter() - t0)
            return r
        return run
    for p in pipes.values():
        p.engine.denoise = timed(p.engine.denoise)
    cfg, B = pipes["txt2img"].cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    g = torch.Generator().manual_seed(3)
    image = (torch.rand(B, 512, 512, 3, generator=g) * 255).to(torch.uint8)
    times = {k: [] for k in pipes}
    front = []
    with trace(pipes["txt2img"]), trace(pipes["ip2p"]):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for kind, pipe in pipes.items():
                kw = {} if kind == "txt2img" else {"image": image}
                loop_s.clear()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=args.steps, output_type="latent", **kw)
                assert len(loop_s) == 1 and torch.isfinite(out.latents).all(), kind
                if rep:
                    times[kind].append(loop_s[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipes["ip2p"].engine.ip2p_prepare(image)
            torch.cuda.synchronize()
            if rep:
                front.append(time.perf_counter() - t0)
    med = {}
    for kind, t in times.items():
        t = sorted(t)
        med[kind] = t[len(t) // 2]
        print(json.dumps({"scheduler": "DDIMScheduler", "variant": kind, "steps": args.steps, "batch": B, "px": 512,
                          "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2),
                          "ms_per_step": round(1e3 * t[len(t) // 2] / args.steps, 3)}))
    f = sorted(front)
    print(json.dumps({"ip2p_over_txt2img": round(med["ip2p"] / med["txt2img"], 3),
                      "front_end_plus_vae_encode_ms_median": round(1e3 * f[len(f) // 2], 3), "min": round(1e3 * f[0], 3), "max": round(1e3 * f[-1], 3),
                      "encoded_rows": B, "px": 512}))
    for p in pipes.values():
        p.engine.close()


if __name__ == "__main__":
    main()
