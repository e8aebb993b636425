"""Wall time of one txt2img denoise loop under the plain pipeline and with an IP-Adapter at scale 1 (SD-1.5 synthetic weights, one pipeline,
512 px, batch 4, CFG 7.5, DDIM x --steps, DAAM recording on), interleaved in one process; one JSON line per variant on stdout (median and
spread over --repeats), then the once-per-call agd_ip_adapter_set on its own and the adapter's cost per evaluation from the medians.

    python tools/ip_adapter_timing.py [--steps 50] [--repeats 5]

Only the loop is timed (set_context + recorder reset + agd_ip_adapter_set for the adapter variant + the fused denoise, ended by a device
synchronise); no VAE decode.  The expectation to compare with comes from bytes: per transformer block the score stage reads h, the add
stage reads and writes h, three passes over [rows][C] bf16 -- about 0.4 GB per evaluation at UNet batch 8, well under 0.1 ms at copy
bandwidth.  What the plan gives up while the adapter is active (attn1.to_out inside the attn2 chain, the lazy duplication of the CFG-shared
prefix on the 64 x 64 blocks) is expected to cost more than the two stages themselves.  The stages' own time per launch comes from a kernel
trace of the same run:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/ip_adapter_timing.py --repeats 1

(its rows are ipa_scores_kernel and ipa_add_kernel).  The loops take drawn embeddings; agd_image_embeds is timed on its own with a synthetic
OpenCLIP ViT-H/14 (the published SD-1.5 adapters' encoder: 32 layers, 16 heads of 80) on `batch` 512 px images (--no-encoder skips it)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stage_bytes(cfg, rows, L):
    """Algorithmic bytes of the two stages over one evaluation: three bf16 passes over every transformer block's [rows][HW][C]."""
    from agenda_amd import ip_adapter
    total = 0
    n = len(cfg.unet.block_out_channels)
    for pre in ip_adapter.attn2_blocks(cfg.unet):
        lvl = n - 1 if pre.startswith("mid") else int(pre.split(".")[1]) if pre.startswith("down") else n - 1 - int(pre.split(".")[1])
        total += 3 * 2 * rows * (L >> lvl) * (L >> lvl) * ip_adapter.block_channels(cfg.unet, pre)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-encoder", action="store_true")
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, ip_adapter, synthetic, trace
    if not torch.cuda.is_available():
        raise SystemExit("ip_adapter_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipe = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B, E = pipe.cfg, args.batch, 1024
    pipe.load_ip_adapter(ip_adapter.make_ip_adapter_weights(cfg, 888, E))
    ctx = synthetic.make_context(cfg, B, seed=7)
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    emb = torch.randn(B, E, generator=torch.Generator().manual_seed(3))
    emb2 = torch.cat([torch.zeros_like(emb), emb]).cuda()
    times = {"plain": [], "ip_adapter": []}
    sets, encs = [], []
    if not args.no_encoder:
        scfg = ip_adapter.image_encoder_config()
        pipe.load_image_encoder(scfg, ip_adapter.make_image_encoder_weights(scfg, 5))
        imgs = torch.randint(0, 256, (B, 512, 512, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).cuda()
    with trace(pipe):
        for rep in range(args.repeats + 1):                  # repeat 0 warms every shape up and is not counted
            for name in times:
                extra = {} if name == "plain" else {"ip_adapter_image_embeds": emb}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx, latents=lat, num_inference_steps=args.steps, output_type="latent", **extra)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                assert torch.isfinite(out.latents).all()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.engine.ip_adapter_set(emb2, 1.0)
            torch.cuda.synchronize()
            if rep:
                sets.append(time.perf_counter() - t0)
            if not args.no_encoder:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.engine.image_embeds(imgs)
                torch.cuda.synchronize()
                if rep:
                    encs.append(time.perf_counter() - t0)
    med = {}
    for name, t in times.items():
        t = sorted(t)
        med[name] = t[len(t) // 2]
        print(json.dumps({"scheduler": "DDIMScheduler", "pipeline": name, "steps": args.steps, "batch": B, "px": 512,
                          "loop_ms_median": round(1e3 * t[len(t) // 2], 2), "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2)}))
    s = sorted(sets)
    print(json.dumps({"plain_ms_per_evaluation": round(1e3 * med["plain"] / args.steps, 3),
                      "ip_adapter_ms_per_evaluation_over_plain": round(1e3 * (med["ip_adapter"] - med["plain"]) / args.steps, 4),
                      "ip_adapter_set_ms_median": round(1e3 * s[len(s) // 2], 3), "ip_adapter_set_ms_min": round(1e3 * s[0], 3),
                      "stage_bytes_per_evaluation": stage_bytes(cfg, 2 * B, 64), "rows": 2 * B,
                      **({"image_embeds_ms_median": round(1e3 * sorted(encs)[len(encs) // 2], 3), "image_embeds_ms_min": round(1e3 * min(encs), 3),
                          "image_embeds_images": B} if encs else {})}))
    pipe.engine.close()


if __name__ == "__main__":
    main()
