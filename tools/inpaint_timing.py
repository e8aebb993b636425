"""Wall time of one fused denoise loop for txt2img, 9-channel inpainting and the 4-channel inpainting blend (SD-1.5 synthetic weights,
512 px, batch 4, CFG 7.5, DAAM recording on): DDIM x --ddim-steps and DPM-Solver++ 2M x --dpm-steps, the six variants interleaved in
one process; one JSON line per variant on stdout (median and spread over --repeats), plus the once-per-call front end (mask kernel +
one VAE encode of the image and the masked image, 2 x batch rows) on its own.

    python tools/inpaint_timing.py [--ddim-steps 50] [--dpm-steps 20] [--repeats 5]

Only the fused loop is timed (the engine's denoise / denoise_dpm call, between two device synchronises); the inpainting variants run
through the pipeline, so their state is set exactly as a user's call sets it.  The 9-channel pipeline has its own UNet (same seed, conv_in
9 channels wide); the blend runs on the txt2img pipeline's weights."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--dpm-steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionInpaintPipeline, StableDiffusionPipeline, synthetic, trace
    from agenda_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    if not torch.cuda.is_available():
        raise SystemExit("inpaint_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipes = {"txt2img": StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30),
             "inpaint9": StableDiffusionInpaintPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30),
             "blend": StableDiffusionInpaintPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30,
                                                                    inpaint=False)}
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
        p.engine.denoise, p.engine.denoise_dpm = timed(p.engine.denoise), timed(p.engine.denoise_dpm)
    cfg, B = pipes["txt2img"].cfg, args.batch
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    g = torch.Generator().manual_seed(3)
    image = (torch.rand(1, 512, 512, 3, generator=g) * 255).to(torch.uint8)
    mask = torch.zeros(1, 512, 512, dtype=torch.uint8)
    mask[:, 128:384, 96:320] = 255
    scheds = {"DDIMScheduler": (DDIMScheduler, args.ddim_steps), "DPMSolverMultistepScheduler": (DPMSolverMultistepScheduler, args.dpm_steps)}
    variants = [(s, k) for s in scheds for k in pipes]
    times = {v: [] for v in variants}
    front = []
    eng9 = pipes["inpaint9"].engine
    imgB, maskB = image.expand(B, -1, -1, -1).contiguous(), mask.expand(B, -1, -1).contiguous()
    with trace(pipes["txt2img"]), trace(pipes["inpaint9"]), trace(pipes["blend"]):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for name, kind in variants:
                pipe = pipes[kind]
                cls, steps = scheds[name]
                pipe.scheduler = cls.from_config(cfg.sched)
                kw = {} if kind == "txt2img" else {"image": image, "mask_image": mask}
                loop_s.clear()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=steps, output_type="latent", **kw)
                assert len(loop_s) == 1 and torch.isfinite(out.latents).all(), (name, kind)
                if rep:
                    times[(name, kind)].append(loop_s[0])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, m = eng9.inpaint_prepare(imgB, maskB, True, True)
            eng9.vae_encode(x)
            torch.cuda.synchronize()
            if rep:
                front.append(time.perf_counter() - t0)
    for (name, kind), t in times.items():
        t = sorted(t)
        steps = scheds[name][1]
        print(json.dumps({"scheduler": name, "variant": kind, "steps": steps, "batch": B, "px": 512,
                          "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2),
                          "ms_per_step": round(1e3 * t[len(t) // 2] / steps, 3)}))
    f = sorted(front)
    print(json.dumps({"front_end_plus_vae_encode_ms_median": round(1e3 * f[len(f) // 2], 3), "min": round(1e3 * f[0], 3), "max": round(1e3 * f[-1], 3),
                      "encoded_rows": 2 * B, "px": 512}))
    for p in pipes.values():
        p.engine.close()


if __name__ == "__main__":
    main()
