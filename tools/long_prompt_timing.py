"""Wall time of one txt2img denoise loop under contexts of 77, 152, 227 and 302 tokens (SD-1.5 synthetic weights, 512 px, batch 4, CFG 7.5,
DAAM recording on, DDIM x --steps): the same pipeline, the contexts interleaved in one process; one JSON line per context on stdout
(median, min and max over --repeats), then the added time per model evaluation of each long context over the 77-token loop, from the medians.

    python tools/long_prompt_timing.py [--steps 50] [--repeats 5]

Only the loop is timed (set_context + recorder reset + the fused denoise, ended by a device synchronise); no VAE decode.  What a context
beyond 96 tokens pays: attn2 leaves the fused chain / pre-multiplied forms for to_q, attention, to_out as separate launches; the
recording half runs csrc/attention_long.hip (K streamed twice); the DAAM accumulators hold T rows per head at every level (no head-group
sums at latent resolution), and K/V of T rows are projected per call.  Per-kernel times come from a kernel trace of the same run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/long_prompt_timing.py --repeats 1

(the new row is attn_long_kernel)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONTEXTS = (77, 152, 227, 302)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from agenda_amd import StableDiffusionPipeline, synthetic, trace
    if not torch.cuda.is_available():
        raise SystemExit("long_prompt_timing: no GPU visible (a CPU time says nothing about the MI355X)")
    pipe = StableDiffusionPipeline.from_synthetic("sd15", seed=1234, weights_device="cuda", workspace_bytes=12 << 30)
    cfg, B, steps = pipe.cfg, args.batch, args.steps
    g = torch.Generator().manual_seed(7)
    ctx = {T: torch.randn(2 * B, T, cfg.unet.cross_attention_dim, generator=g).to(torch.bfloat16).float() for T in CONTEXTS}
    lat = synthetic.make_latents(cfg, list(range(B)), 64)
    times = {T: [] for T in CONTEXTS}
    with trace(pipe):
        for rep in range(args.repeats + 1):                      # repeat 0 warms every shape up and is not counted
            for T in CONTEXTS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe(prompt_embeds=ctx[T], latents=lat, num_inference_steps=steps, output_type="latent")
                torch.cuda.synchronize()
                if rep:
                    times[T].append(time.perf_counter() - t0)
                assert torch.isfinite(out.latents).all()
    med = {}
    for T, t in times.items():
        t = sorted(t)
        med[T] = t[len(t) // 2]
        print(json.dumps({"context_tokens": T, "steps": steps, "batch": B, "px": 512, "loop_ms_median": round(1e3 * med[T], 2),
                          "loop_ms_min": round(1e3 * t[0], 2), "loop_ms_max": round(1e3 * t[-1], 2)}))
    print(json.dumps({"ms_per_evaluation_77": round(1e3 * med[77] / steps, 3),
                      **{f"added_ms_per_evaluation_{T}": round(1e3 * (med[T] - med[77]) / steps, 3) for T in CONTEXTS if T != 77},
                      **{f"loop_{T}_over_77": round(med[T] / med[77], 3) for T in CONTEXTS if T != 77}}))
    pipe.engine.close()


if __name__ == "__main__":
    main()
