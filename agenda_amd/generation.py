"""Driver for the generation hot loop, mirroring reference data_generation/data_generation.py:26-86
(token selection, per-seed image + per-word DAAM heat-map export), batched and seed-sharded
across ranks: images are independent per seed, so rank r takes seeds
s = r (mod world); the only exchange is one all_gather of uint8 images + fp32 word heat maps per
batch (RCCL over xGMI on GPUs; gloo in the CPU tests)."""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import List, Optional, Sequence

import numpy as np
import torch


def select_learned_tokens(prompt_template: str, initialize_token: Sequence[str], learned: Sequence[str],
                          word_token_heatmaps: Optional[List[str]], store_learnable: bool):
    """data_generation.py:36-43,54 -- a learned token is used iff its init word is a substring of the
    UNFORMATTED template; the heat-map word list aliases the CLI list and is appended in place."""
    words = word_token_heatmaps if word_token_heatmaps is not None else []
    new_tokens = []
    for t, n in zip(initialize_token, learned):
        if t in prompt_template:
            if store_learnable:
                words.append(n)
            new_tokens.append(n)
    return new_tokens, words, prompt_template.format(*new_tokens)


def inject_learned_tokens(pipe, embeds_dict, new_tokens):
    """data_generation.py:45-52."""
    if not new_tokens:
        return []
    emb = torch.stack([embeds_dict[t] for t in new_tokens])
    pipe.tokenizer.add_tokens(list(new_tokens))
    ids = pipe.tokenizer.convert_tokens_to_ids(list(new_tokens))
    pipe.text_encoder.resize_token_embeddings(len(pipe.tokenizer))
    with torch.no_grad():
        w = pipe.text_encoder.get_input_embeddings().weight
        w.data[ids] = emb.to(w.dtype)
    return ids


def shard_seeds(num_images: int, rank: int, world: int) -> List[int]:
    return list(range(rank, num_images, world))


def export_heatmap_u8(hm: np.ndarray) -> np.ndarray:
    """data_generation.py:82-84: min-max (+1e-8), x255, truncating uint8 cast."""
    hm = np.asarray(hm, dtype=np.float32)
    hm = (hm - hm.min()) / (hm.max() - hm.min() + 1e-8) * 255
    return hm.astype(np.uint8)


def stack_heatmaps(obj: np.ndarray, fg: np.ndarray, bg: np.ndarray):
    """postprocess_heatmap.py:44-48."""
    inv = 255 - bg
    return np.stack([obj, fg, inv], axis=-1), inv


def generate_batch(pipe, seeds: Sequence[int], words: Sequence[str], prompt: Optional[str] = None,
                   prompt_embeds: Optional[torch.Tensor] = None, num_inference_steps: int = 50,
                   guidance_scale: float = 7.5, height: Optional[int] = None, rec_tokens: Optional[int] = None,
                   word_rows: Optional[Sequence[Sequence[int]]] = None, control: Optional[dict] = None, width: Optional[int] = None):
    """One hot-path pass: len(seeds) images + per-word DAAM maps.  control: extra keyword arguments of a ControlNet pipeline's call
    (`image`, `controlnet_conditioning_scale`, `control_guidance_start`, `control_guidance_end`), of a T2I-Adapter one (`image`,
    `adapter_conditioning_scale`, `adapter_conditioning_factor`), of an inpainting one
    (`inpaint_inputs_for`) or of an InstructPix2Pix one (`ip2p_inputs_for`, with height and width the image's).
    Returns (uint8 images [B,H,W,3] on GPU, fp32 heat maps [B, n_words, H/8, W/8] on GPU)."""
    from .trace import trace
    from . import synthetic
    B = len(seeds)
    side = pipe.cfg.default_sample_size * pipe.vae_scale_factor
    height, width = height or side, width or side
    f = pipe.vae_scale_factor
    if height == width:
        lat = synthetic.make_latents(pipe.cfg, seeds, height // f)      # CPU generator per image seed (data_generation.py:58)
    else:                                                               # the same per-seed draw at the rectangular shape
        lat = torch.cat([torch.randn(1, pipe.cfg.unet.out_channels, height // f, width // f, generator=torch.Generator("cpu").manual_seed(int(s)))
                         for s in seeds], 0)
    with trace(pipe, rec_tokens=rec_tokens) as trc:
        if prompt_embeds is None:
            out = pipe([prompt] * B, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                       latents=lat, height=height, width=width, output_type="pt", **(control or {}))
        else:
            out = pipe(prompt_embeds=prompt_embeds, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                       latents=lat, height=height, width=width, output_type="pt", **(control or {}))
        hms = []
        for i in range(B):
            g = trc.compute_global_heat_map(prompt=prompt, image_index=i)
            if word_rows is not None:
                # integer (view) indexing: a python list index makes torch upload an index tensor with a BLOCKING pageable copy, i.e. a host
                # sync at the end of every batch
                hms.append(torch.stack([torch.stack([g.heat_maps[int(i)] for i in r]).mean(0) for r in word_rows]))
            elif words and getattr(trc, "regions", None) is not None:      # a region call: the canvas map composed from the regions' states
                hms.append(torch.stack([trc.compute_region_word_heat_map(w, image_index=i).heatmap for w in words]))
            elif words:
                hms.append(torch.stack([g.compute_word_heat_map(w).heatmap for w in words]))
            else:
                hms.append(g.heat_maps[:0])
    return out.images, torch.stack(hms)


class PendingGather:
    """Handle of an all_gather posted with `gather_outputs(..., async_op=True)`: the collectives run on the backend's own stream
    while the caller enqueues the next batch; `wait()` returns what the blocking call returns."""

    def __init__(self, works, finish):
        self._works, self._finish, self._out = works, finish, None

    def wait(self):
        if self._out is None:
            for w in self._works:
                w.wait()
            self._out = self._finish()
        return self._out


def gather_outputs(images: torch.Tensor, heatmaps: torch.Tensor, seeds: Optional[Sequence[int]] = None, max_batch: Optional[int] = None,
                   async_op: bool = False, global_seeds: Optional[Sequence[int]] = None):
    """The final exchange step: literally ONE all_gather per batch.  Every rank packs its seed ids, images and
    heat maps into one byte buffer ([ids int64 | images | heat maps], sections 16-byte aligned); one collective moves it; the
    result is unpacked as views of the gathered buffer.

    Ranks may hold different batch sizes (the last, ragged round of `shard_seeds`; even zero images): every rank pads its
    sections to `max_batch` rows (id -1), the padding is dropped after the collective, and rows come back ordered by seed.
    `max_batch` must be the same on every rank (defaults to the local batch: the equal-batch case of bench.py).
    Returns (images, heatmaps) when `seeds` is None (equal full batches: rank-interleaved = the global seed order of
    `shard_seeds`, a pure view permutation), else (seeds, images, heatmaps).  With `global_seeds` (the sorted seeds of ALL ranks in
    this round, which callers of `shard_seeds` know on the host) nothing here synchronises with the host: rows are ordered by a
    masked argsort on the device and sliced by len(global_seeds); without it the seed list is read back from the gathered ids
    (one device -> host copy).  No-op for world size 1.

    Contract of `global_seeds`: it must be EXACTLY the sorted union of the seeds the ranks packed this round (what `shard_seeds`
    hands each rank, derived from one place -- `round_seeds` in `generation.main`).  The sync-free path cannot check that: a list
    that disagrees with the packed ids (a rank that dropped an image, a different `max_batch`) would pair seeds with the wrong rows
    silently.  Set AGD_GATHER_CHECK=1 to verify it (one device -> host copy per round: gathered ids == global_seeds, the next id the
    padding sentinel); the ragged tests run with it on."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        res = (images, heatmaps) if seeds is None else (list(seeds), images, heatmaps)
        return PendingGather([], lambda: res) if async_op else res
    w = dist.get_world_size()
    b = images.shape[0]
    mb = int(max_batch) if max_batch is not None else b
    if b > mb:
        raise ValueError(f"local batch {b} > max_batch {mb}")
    if seeds is None and b != mb:
        raise ValueError("gather_outputs without seeds is the equal-batch form: pass seeds (and max_batch) for ragged rounds")
    dev = images.device
    ishape, hshape = tuple(images.shape[1:]), tuple(heatmaps.shape[1:])
    ib = images[:0].new_empty((1,) + ishape).numel() * images.element_size()        # bytes per image row
    hb = heatmaps[:0].new_empty((1,) + hshape).numel() * heatmaps.element_size()
    a16 = lambda n: (n + 15) & ~15
    o_img = a16(mb * 8)
    o_hm = o_img + a16(mb * ib)
    total = o_hm + a16(mb * hb)
    buf = torch.zeros(total, dtype=torch.uint8, device=dev)
    ids = buf[:mb * 8].view(torch.int64)
    ids.fill_(-1)
    if b:
        if seeds is not None:
            ids[:b] = torch.as_tensor(list(seeds), dtype=torch.int64).to(dev, non_blocking=True)
        else:
            ids[:b] = torch.arange(b, device=dev) * w + dist.get_rank()             # seed = rank + world * local_index
        buf[o_img:o_img + b * ib] = images.contiguous().view(torch.uint8).reshape(-1)
        buf[o_hm:o_hm + b * hb] = heatmaps.contiguous().view(torch.uint8).reshape(-1)
    # the collective form is chosen up front, identically on every rank (never retry a collective after one failed: the other
    # ranks would not join the second one): RCCL takes the flat form, other backends (gloo rehearsals) the list form
    if dist.get_backend() == "nccl":
        out = torch.empty(w * total, dtype=torch.uint8, device=dev)
        works = [dist.all_gather_into_tensor(out, buf, async_op=True)]
        gathered = lambda: out.view(w, total)
    else:
        parts = [torch.empty_like(buf) for _ in range(w)]
        works = [dist.all_gather(parts, buf, async_op=True)]
        gathered = lambda: torch.stack(parts)

    def finish():
        g = gathered()                                                              # [world][total] bytes
        gs = g[:, :mb * 8].contiguous().view(torch.int64).reshape(w * mb)
        gi = g[:, o_img:o_img + mb * ib].contiguous().view(images.dtype).reshape((w, mb) + ishape)
        gh = g[:, o_hm:o_hm + mb * hb].contiguous().view(heatmaps.dtype).reshape((w, mb) + hshape)
        if seeds is None:                       # equal full batches: seed = rank + world * local index -> transpose, no sort, no sync
            return gi.transpose(0, 1).reshape((w * mb,) + ishape), gh.transpose(0, 1).reshape((w * mb,) + hshape)
        gi, gh = gi.reshape((w * mb,) + ishape), gh.reshape((w * mb,) + hshape)
        key = torch.where(gs >= 0, gs, torch.full_like(gs, torch.iinfo(torch.int64).max))
        order = torch.argsort(key)
        if global_seeds is not None:            # the caller knows every rank's seeds of this round: no host sync at all
            n = len(global_seeds)
            if os.environ.get("AGD_GATHER_CHECK"):      # debug: the caller's list against what the ranks really packed (host sync)
                got = key[order].tolist()
                sentinel = torch.iinfo(torch.int64).max
                if got[:n] != [int(s_) for s_ in global_seeds] or (n < len(got) and got[n] != sentinel):
                    raise RuntimeError(f"gather_outputs: global_seeds {list(global_seeds)} disagree with the gathered ids "
                                       f"{[g_ for g_ in got if g_ != sentinel]}")
            return list(global_seeds), gi[order[:n]], gh[order[:n]]
        srt = key[order].tolist()               # (device -> host: the seed list is part of the result)
        n = sum(1 for s_ in srt if s_ != torch.iinfo(torch.int64).max)
        return srt[:n], gi[order[:n]], gh[order[:n]]

    pend = PendingGather(works, finish)
    return pend if async_op else pend.wait()


def save_outputs(save_dir: str, seeds, images_u8, heatmaps, words, image_size, stack_words=None, exported: bool = False):
    """data_generation.py:60-62,66-86: resize, skip all-black, images/ + daam_<word>_heatmaps/ PNGs.
    CUDA tensors take the device export path (agenda_amd/export.py: min-max -> uint8 -> PIL-exact bicubic resize on
    the GPU, one D2H copy of the finished buffers); numpy inputs take the reference's literal host code.  Both
    produce identical bytes (tests/test_export.py).  `stack_words=(obj, fg, bg)` additionally writes
    daam_stack_heatmaps/ + daam_inv_heatmaps/ as postprocess_heatmap.py:44-50 would.  `image_size`: one side (square PNGs, the
    reference's `resize((S, S))`) or an (h, w) pair."""
    from PIL import Image
    sh, sw = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
    os.makedirs(os.path.join(save_dir, "images"), exist_ok=True)
    if exported:                                # already the final payloads (export_batch ran before the gather)
        small, hm = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (images_u8, heatmaps))
    elif torch.is_tensor(images_u8) and images_u8.is_cuda:
        from . import export
        small, hm = export.export_batch(images_u8, heatmaps, image_size)
        small, hm = small.cpu().numpy(), hm.cpu().numpy()
    else:
        images_u8, heatmaps = np.asarray(images_u8), np.asarray(heatmaps)
        small = np.stack([np.asarray(Image.fromarray(im).resize((sw, sh))) for im in images_u8])
        hm = np.stack([np.stack([np.asarray(Image.fromarray(export_heatmap_u8(h)).resize((sw, sh)))
                                 for h in hs]) if len(hs) else np.zeros((0, sh, sw), np.uint8) for hs in heatmaps])
    for i, seed in enumerate(seeds):
        if np.max(small[i]) < 1e-5:             # NSFW content filter (black image), data_generation.py:61-62
            continue
        Image.fromarray(small[i]).save(os.path.join(save_dir, "images", f"{seed}.png"))
        for wi, word in enumerate(words):
            d = os.path.join(save_dir, "daam_" + word + "_heatmaps")
            os.makedirs(d, exist_ok=True)
            Image.fromarray(hm[i, wi]).save(os.path.join(d, f"{seed}.png"))
        if stack_words is not None:
            o, f, b = (hm[i, list(words).index(w)] for w in stack_words)
            rgb, inv = stack_heatmaps(o, f, b)
            for sub, arr in (("daam_stack_heatmaps", rgb), ("daam_inv_heatmaps", inv)):
                os.makedirs(os.path.join(save_dir, sub), exist_ok=True)
                Image.fromarray(arr).save(os.path.join(save_dir, sub, f"{seed}.png"))


def sega_arguments(p, args) -> Optional[dict]:
    """The Semantic Guidance flags as the pipeline's keywords (None without --editing-prompt), refused where they cannot run."""
    flags = {"reverse_editing_direction": args.reverse_editing_direction, "edit_guidance_scale": args.edit_guidance_scale,
             "edit_warmup_steps": args.edit_warmup_steps, "edit_cooldown_steps": args.edit_cooldown_steps,
             "edit_threshold": args.edit_threshold, "edit_weights": args.edit_weights}
    scalars = {"edit_momentum_scale": args.edit_momentum_scale, "edit_mom_beta": args.edit_mom_beta}
    if args.editing_prompt is None:
        given = [k for k, v in {**flags, **scalars}.items() if v is not None]
        if given:
            p.error(f"--{given[0].replace('_', '-')} needs --editing-prompt")
        return None
    K = len(args.editing_prompt)
    if K > 8:
        p.error(f"--editing-prompt: {K} concepts (at most 8)")
    if (args.controlnet_model_path or args.adapter_model_path or args.ip_adapter_path or args.init_image or args.instruct_image
            or args.gligen_phrases is not None or args.gligen_layouts is not None or args.panorama or args.guidance_rescale or args.pag_scale
            or args.region_prompts is not None or args.region_layouts is not None or (args.deepcache_interval or 1) > 1
            or args.max_embeddings_multiples is not None):
        p.error("--editing-prompt with --controlnet-model-path, --adapter-model-path, --ip-adapter-path, --init-image, --instruct-image, "
                "--gligen-phrases / --gligen-layouts, --panorama, --region-prompts / --region-layouts, --guidance-rescale, --pag-scale, "
                "--deepcache-interval or --max-embeddings-multiples is not implemented")
    out = {"editing_prompt": list(args.editing_prompt)}
    for name, v in flags.items():
        if v is None:
            continue
        if len(v) not in (1, K):
            p.error(f"--{name.replace('_', '-')}: {len(v)} values for {K} concepts (one, or one per concept)")
        v = [bool(x) for x in v] if name == "reverse_editing_direction" else list(v)
        out[name] = v[0] if len(v) == 1 else v
    if args.edit_threshold is not None and not all(0.0 <= q <= 1.0 for q in args.edit_threshold):
        p.error(f"--edit-threshold {' '.join(str(q) for q in args.edit_threshold)}: quantiles in [0, 1]")
    for name, v in scalars.items():
        if v is not None:
            if not math.isfinite(v):
                p.error(f"--{name.replace('_', '-')} {v}: a finite number")
            out[name] = v
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Image and attention map generation (MI355X).")
    p.add_argument("--save-dir", type=str, default="Data/Synthetic")
    p.add_argument("--pretrained-model-path", type=str, default=None, help="diffusers-layout checkpoint; omit for synthetic weights")
    p.add_argument("--learnable-tokens-embedding-path", type=str, default=None)
    p.add_argument("--prompt", type=str, default="An aerial view image with {} cars in {} Utah")
    p.add_argument("--initialize_token", type=str, default=["cars", "Utah", "New Zealand"], nargs="+")
    p.add_argument("--word_token_heatmaps", type=str, default=None, nargs="+")
    p.add_argument("--store_learnable_token_heatmaps", action="store_true")
    p.add_argument("--num-images", type=int, default=10000)
    p.add_argument("--image-size", type=int, default=[112], nargs="+", metavar="S",
                   help="saved PNG size: one value S (square, S x S) or two values H W")
    p.add_argument("--height", type=int, default=None, help="generated image height, a multiple of 64 (default: the checkpoint's size)")
    p.add_argument("--width", type=int, default=None, help="generated image width, a multiple of 64 (default: the checkpoint's size)")
    p.add_argument("--batch-size", type=int, default=4)
    p.add_argument("--num-inference-steps", type=int, default=20)
    p.add_argument("--synthetic-config", type=str, default="sd15", help="architecture for synthetic weights when no checkpoint is given")
    p.add_argument("--stack", type=str, default=None, nargs=3, metavar=("OBJ", "FG", "BG"),
                   help="also write daam_stack_heatmaps/ + daam_inv_heatmaps/ for these three words (postprocess_heatmap.py)")
    p.add_argument("--scheduler", type=str, default=None, choices=["DDIMScheduler", "PNDMScheduler", "DPMSolverMultistepScheduler"],
                   help="default: the checkpoint's scheduler/scheduler_config.json (PNDM for SD-1.4, as the reference runs it); "
                        "DDIMScheduler for synthetic weights.  DPMSolverMultistepScheduler: DPM-Solver++ 2M, one UNet evaluation per step")
    p.add_argument("--use-karras-sigmas", action="store_true",
                   help="DPMSolverMultistepScheduler only: Karras (rho = 7) noise levels instead of the checkpoint's timestep spacing")
    p.add_argument("--no-safety-checker", action="store_true",
                   help="load the checkpoint without its safety checker (by default flagged images come back black and are skipped)")
    p.add_argument("--no-gather", action="store_true",
                   help="multi-GPU: every rank writes its own files instead of the final all_gather to rank 0")
    p.add_argument("--controlnet-model-path", type=str, default=None, help="a diffusers ControlNetModel directory: ControlNet-conditioned txt2img")
    p.add_argument("--control-image", type=str, default=None,
                   help="control image file (every seed), or a directory: seed s uses its sorted file s mod n")
    p.add_argument("--controlnet-conditioning-scale", type=float, default=1.0)
    p.add_argument("--control-guidance-start", type=float, default=0.0)
    p.add_argument("--control-guidance-end", type=float, default=1.0)
    p.add_argument("--adapter-model-path", type=str, default=None, help="a diffusers T2IAdapter directory: T2I-Adapter conditioned txt2img")
    p.add_argument("--adapter-image", type=str, default=None,
                   help="adapter conditioning image file (every seed), or a directory: seed s uses its sorted file s mod n")
    p.add_argument("--adapter-conditioning-scale", type=float, default=1.0)
    p.add_argument("--adapter-conditioning-factor", type=float, default=1.0,
                   help="the share of the model evaluations, from the first on, that get the adapter's features")
    p.add_argument("--ip-adapter-path", type=str, default=None,
                   help="an IP-Adapter weight file (.safetensors / .bin) or a local directory holding one: image-prompted txt2img")
    p.add_argument("--ip-adapter-image", type=str, default=None,
                   help="the image prompt (every seed), or a directory: seed s uses its sorted file s mod n")
    p.add_argument("--ip-adapter-scale", type=float, default=1.0)
    p.add_argument("--image-encoder-path", type=str, default=None,
                   help="the adapter's CLIPVisionModelWithProjection directory (default: image_encoder/ beside the adapter weights)")
    p.add_argument("--init-image", type=str, default=None,
                   help="inpainting: the image to paint into (a file for every seed, or a directory: seed s uses its sorted file s mod n)")
    p.add_argument("--mask-image", type=str, default=None,
                   help="inpainting: the mask, white = repaint (file or directory, paired with --init-image by sorted name)")
    p.add_argument("--strength", type=float, default=1.0, help="inpainting: 1 starts from noise; < 1 (DDIM only) from the noised image")
    p.add_argument("--instruct-image", type=str, default=None,
                   help="InstructPix2Pix checkpoint: the image the prompt edits (a file for every seed, or a directory: seed s uses its sorted "
                        "file s mod n); the output has the image's size")
    p.add_argument("--image-guidance-scale", type=float, default=None, help="InstructPix2Pix: image_guidance_scale (default 1.5, at least 1)")
    p.add_argument("--lora-path", type=str, default=None,
                   help="a LoRA file or directory (kohya or diffusers format) merged into the UNet / text encoder on every rank")
    p.add_argument("--lora-weight-name", type=str, default=None, help="the LoRA file inside --lora-path (default pytorch_lora_weights.safetensors, then .bin)")
    p.add_argument("--lora-scale", type=float, default=1.0, help="the LoRA's strength (cross_attention_kwargs scale)")
    p.add_argument("--gligen-phrases", type=str, default=None, nargs="+", metavar="P",
                   help="GLIGEN checkpoint: one phrase per box, the same layout for every seed")
    p.add_argument("--gligen-boxes", type=float, default=None, nargs="+", metavar="V",
                   help="GLIGEN: x0 y0 x1 y1 per phrase, normalised to [0, 1]")
    p.add_argument("--gligen-layouts", type=str, default=None,
                   help="GLIGEN: a JSON file holding a list of {\"phrases\": [...], \"boxes\": [[x0, y0, x1, y1], ...]}; seed s uses layout s mod n")
    p.add_argument("--panorama", action="store_true",
                   help="MultiDiffusion panorama txt2img (StableDiffusionPanoramaPipeline): --height / --width give the canvas, each a multiple of 64 "
                        "and at least the checkpoint's size (default: that size x 4 times it); DDIM only")
    p.add_argument("--view-batch-size", type=int, default=None, help="panorama: views per UNet call (default: all views of a step at once)")
    p.add_argument("--region-prompts", type=str, default=None, nargs="+", metavar="P",
                   help="region-based MultiDiffusion (StableDiffusionRegionPipeline): one prompt per foreground region, the same layout for "
                        "every seed; --prompt is the background's; DDIM only, any checkpoint")
    p.add_argument("--region-boxes", type=float, default=None, nargs="+", metavar="V",
                   help="regions: x0 y0 x1 y1 per region prompt, normalised to [0, 1]")
    p.add_argument("--region-masks", type=str, default=None, nargs="+", metavar="FILE",
                   help="regions: one mask image per region prompt (white = the region), of the generated size")
    p.add_argument("--region-layouts", type=str, default=None,
                   help="regions: a JSON file holding a list of {\"prompts\": [...], \"boxes\": [[x0, y0, x1, y1], ...]}; seed s uses layout s mod n")
    p.add_argument("--bootstrapping", type=int, default=None, metavar="N",
                   help="regions: the first N steps show every foreground region a random constant-colour background outside its mask "
                        "(default 20, clipped to the steps)")
    p.add_argument("--gligen-beta", type=float, default=0.3, help="GLIGEN: gligen_scheduled_sampling_beta (the grounded share of the evaluations)")
    p.add_argument("--freeu", type=float, default=None, nargs=4, metavar=("S1", "S2", "B1", "B2"),
                   help="FreeU (enable_freeu) on every UNet evaluation, with any pipeline: the skip filters' scales and the backbone scales of "
                        "up blocks 0 and 1; suggested 0.9 0.2 1.2 1.4 (SD-1.4), 0.9 0.2 1.5 1.6 (SD-1.5), 0.9 0.2 1.4 1.6 (SD-2.1)")
    p.add_argument("--guidance-rescale", type=float, default=0.0, metavar="PHI",
                   help="guidance_rescale (Lin et al. 2023): after the CFG combine, rescale the prediction to the text branch's per-image "
                        "standard deviation, blended by PHI in [0, 1] (0: off; 0.7 is the paper's value); not with --panorama / --instruct-image")
    p.add_argument("--pag-scale", type=float, default=0.0, metavar="P",
                   help="Perturbed-Attention Guidance (Ahn et al. 2024): every evaluation runs a third UNet branch whose applied self-attention "
                        "maps are the identity, and sampling is pushed away from it by P (0: off; 3 is the paper's value); plain txt2img only")
    p.add_argument("--pag-adaptive-scale", type=float, default=0.0, metavar="A",
                   help="PAG: the scale of the evaluation at timestep t is max(0, P - A (1000 - t)) (0: constant P); needs --pag-scale")
    p.add_argument("--pag-applied-layers", type=str, default=None, nargs="+", metavar="L",
                   help="PAG: regular expressions searched in the UNet's self-attention module names (default: mid); needs --pag-scale")
    p.add_argument("--deepcache-interval", type=int, default=None, metavar="N",
                   help="DeepCache (Ma et al. 2024; enable_deepcache): only every N-th model evaluation runs the whole UNet, the others its "
                        "shallowest layers on the cached deep features (1: off; 2 - 3 suggested at 50 steps); plain txt2img only")
    p.add_argument("--deepcache-branch", type=int, default=None, metavar="B",
                   help="DeepCache: the layers 0 .. B of the first down block run on a shallow evaluation (default 0); needs --deepcache-interval")
    p.add_argument("--max-embeddings-multiples", type=int, default=None, metavar="M", choices=[1, 2, 3, 4],
                   help="weighted and long prompts (lpw_stable_diffusion's rules): in the prompt, after its placeholders are filled, (x) weighs "
                        "x by 1.1, [x] by 1 / 1.1, (x:w) by w, and up to 75 M tokens are kept (contexts of 77, 152, 227, 302 rows); heat maps "
                        "follow the weight-stripped tokens; plain txt2img only (default: off, parentheses are literal, 75 tokens)")
    p.add_argument("--editing-prompt", type=str, default=None, nargs="+", metavar="P",
                   help="Semantic Guidance (Brack et al. 2023; SemanticStableDiffusionPipeline): up to 8 edit concepts, each steering only "
                        "the image regions where its direction is strongest; the prompt, the seed and the heat maps stay as they are; plain "
                        "txt2img only.  The --edit-* / --reverse-editing-direction flags take one value for all concepts or one per concept")
    p.add_argument("--reverse-editing-direction", type=int, default=None, nargs="+", metavar="R", choices=[0, 1],
                   help="SEGA: 1 steers away from the concept, 0 towards it (default 0)")
    p.add_argument("--edit-guidance-scale", type=float, default=None, nargs="+", metavar="S", help="SEGA: the concept's guidance scale (default 5)")
    p.add_argument("--edit-warmup-steps", type=int, default=None, nargs="+", metavar="N",
                   help="SEGA: model evaluations before the concept is applied (default 10)")
    p.add_argument("--edit-cooldown-steps", type=int, default=None, nargs="+", metavar="N",
                   help="SEGA: the evaluation from which the concept is no longer applied (default: never)")
    p.add_argument("--edit-threshold", type=float, default=None, nargs="+", metavar="Q",
                   help="SEGA: the quantile in [0, 1] of the direction's magnitude below which the image is left untouched (default 0.9)")
    p.add_argument("--edit-weights", type=float, default=None, nargs="+", metavar="W", help="SEGA: the concepts' relative weights (default 1)")
    p.add_argument("--edit-momentum-scale", type=float, default=None, metavar="MU", help="SEGA: the momentum added to the guidance (default 0.1)")
    p.add_argument("--edit-mom-beta", type=float, default=None, metavar="BETA", help="SEGA: how much of the momentum is kept per evaluation (default 0.4)")
    p.add_argument("--timestep-spacing", type=str, default=None, choices=["leading", "trailing", "linspace"],
                   help="the scheduler's timestep grid (default: the checkpoint's; DDIM and img2img take all three, DPM-Solver++ its own "
                        "three, PNDM runs 'leading' only)")
    p.add_argument("--rescale-betas-zero-snr", action="store_true",
                   help="DDIM: the zero-terminal-SNR beta table (the last timestep is pure noise); needs a v-prediction checkpoint and a grid "
                        "that starts there (--timestep-spacing trailing)")
    args = p.parse_args(argv)
    if not (math.isfinite(args.guidance_rescale) and 0.0 <= args.guidance_rescale <= 1.0):
        p.error(f"--guidance-rescale {args.guidance_rescale}: a number in [0, 1]")
    if args.guidance_rescale and (args.panorama or args.instruct_image):
        p.error("--guidance-rescale with --panorama or --instruct-image is not implemented")
    if not (math.isfinite(args.pag_scale) and args.pag_scale >= 0.0 and math.isfinite(args.pag_adaptive_scale) and args.pag_adaptive_scale >= 0.0):
        p.error(f"--pag-scale {args.pag_scale} / --pag-adaptive-scale {args.pag_adaptive_scale}: finite numbers >= 0")
    if not args.pag_scale and (args.pag_adaptive_scale or args.pag_applied_layers is not None):
        p.error("--pag-adaptive-scale and --pag-applied-layers need --pag-scale P with P > 0")
    if args.pag_scale and (args.controlnet_model_path or args.adapter_model_path or args.ip_adapter_path or args.init_image or args.instruct_image
                           or args.gligen_phrases is not None or args.gligen_layouts is not None or args.panorama or args.guidance_rescale):
        p.error("--pag-scale with --controlnet-model-path, --adapter-model-path, --ip-adapter-path, --init-image, --instruct-image, "
                "--gligen-phrases / --gligen-layouts, --panorama or --guidance-rescale is not implemented")
    if args.max_embeddings_multiples is not None and (
            args.controlnet_model_path or args.adapter_model_path or args.ip_adapter_path or args.init_image or args.instruct_image
            or args.gligen_phrases is not None or args.gligen_layouts is not None or args.panorama):
        p.error("--max-embeddings-multiples with --controlnet-model-path, --adapter-model-path, --ip-adapter-path, --init-image, --instruct-image, "
                "--gligen-phrases / --gligen-layouts or --panorama is not implemented")
    args.sega = sega_arguments(p, args)
    if args.deepcache_branch is not None and args.deepcache_interval is None:
        p.error("--deepcache-branch needs --deepcache-interval N")
    if args.deepcache_interval is not None and args.deepcache_interval < 1:
        p.error(f"--deepcache-interval {args.deepcache_interval}: an integer >= 1")
    if args.deepcache_branch is not None and args.deepcache_branch < 0:
        p.error(f"--deepcache-branch {args.deepcache_branch}: an integer >= 0")
    if (args.deepcache_interval or 1) > 1 and (
            args.controlnet_model_path or args.adapter_model_path or args.ip_adapter_path or args.init_image or args.instruct_image
            or args.gligen_phrases is not None or args.gligen_layouts is not None or args.panorama or args.pag_scale):
        p.error("--deepcache-interval with --controlnet-model-path, --adapter-model-path, --ip-adapter-path, --init-image, --instruct-image, "
                "--gligen-phrases / --gligen-layouts, --panorama or --pag-scale is not implemented")
    if args.scheduler == "PNDMScheduler" and args.timestep_spacing not in (None, "leading"):
        p.error(f"--timestep-spacing {args.timestep_spacing}: PNDMScheduler runs 'leading' only")
    if args.rescale_betas_zero_snr and args.scheduler in ("PNDMScheduler", "DPMSolverMultistepScheduler"):
        p.error(f"--rescale-betas-zero-snr is DDIMScheduler's ({args.scheduler} has no such option)")
    if args.freeu is not None and not all(math.isfinite(v) for v in args.freeu):
        p.error(f"--freeu {' '.join(str(v) for v in args.freeu)}: four finite numbers")
    if args.lora_path is None and (args.lora_weight_name is not None or args.lora_scale != 1.0):
        p.error("--lora-weight-name / --lora-scale need --lora-path")
    if (args.init_image is None) != (args.mask_image is None):
        p.error("--init-image and --mask-image go together")
    if args.init_image is not None and args.controlnet_model_path:
        p.error("ControlNet inpainting is not implemented (--init-image with --controlnet-model-path)")
    if args.init_image is None and args.strength != 1.0:
        p.error("--strength needs --init-image / --mask-image")
    if args.instruct_image is None and args.image_guidance_scale is not None:
        p.error("--image-guidance-scale needs --instruct-image")
    if args.instruct_image is not None:
        # everything StableDiffusionInstructPix2PixPipeline refuses is refused here, before a device is touched
        if args.controlnet_model_path or args.control_image or args.init_image or args.gligen_phrases is not None or args.gligen_layouts is not None or args.panorama:
            p.error("--instruct-image with ControlNet, inpainting, GLIGEN or --panorama is not implemented")
        if args.height is not None or args.width is not None:
            p.error("--instruct-image takes its size from the image: --height / --width cannot be given (nothing is resized)")
        if args.image_guidance_scale is None:
            args.image_guidance_scale = 1.5
        if not args.image_guidance_scale >= 1.0:
            p.error(f"--image-guidance-scale {args.image_guidance_scale}: at least 1 (the no-guidance mode is not implemented)")
    if (args.controlnet_model_path is None) != (args.control_image is None):
        p.error("--controlnet-model-path and --control-image go together")
    if (args.adapter_model_path is None) != (args.adapter_image is None):
        p.error("--adapter-model-path and --adapter-image go together")
    if args.adapter_model_path is None and (args.adapter_conditioning_scale != 1.0 or args.adapter_conditioning_factor != 1.0):
        p.error("--adapter-conditioning-scale / --adapter-conditioning-factor need --adapter-model-path")
    if not 0.0 <= args.adapter_conditioning_factor <= 1.0:
        p.error("--adapter-conditioning-factor: 0 <= factor <= 1")
    if args.adapter_model_path and (args.controlnet_model_path or args.init_image or args.instruct_image or args.gligen_phrases is not None
                                    or args.gligen_layouts is not None or args.panorama):
        p.error("--adapter-model-path with ControlNet, inpainting, InstructPix2Pix, GLIGEN or --panorama is not implemented")
    if (args.ip_adapter_path is None) != (args.ip_adapter_image is None):
        p.error("--ip-adapter-path and --ip-adapter-image go together")
    if args.ip_adapter_path is None and (args.ip_adapter_scale != 1.0 or args.image_encoder_path is not None):
        p.error("--ip-adapter-scale / --image-encoder-path need --ip-adapter-path")
    if args.ip_adapter_path and (args.controlnet_model_path or args.adapter_model_path or args.init_image or args.instruct_image
                                 or args.gligen_phrases is not None or args.gligen_layouts is not None or args.panorama):
        p.error("--ip-adapter-path with ControlNet, a T2I-Adapter, inpainting, InstructPix2Pix, GLIGEN or --panorama is not implemented")
    if not 0.0 <= args.control_guidance_start < args.control_guidance_end <= 1.0:
        p.error("--control-guidance-start / --control-guidance-end: 0 <= start < end <= 1")
    if args.use_karras_sigmas and args.scheduler != "DPMSolverMultistepScheduler":
        p.error("--use-karras-sigmas needs --scheduler DPMSolverMultistepScheduler")
    if len(args.image_size) not in (1, 2) or min(args.image_size) < 1:
        p.error("--image-size takes one positive value S (square) or two, H W")
    args.image_size = args.image_size[0] if len(args.image_size) == 1 else tuple(args.image_size)
    if (args.gligen_phrases is None) != (args.gligen_boxes is None):
        p.error("--gligen-phrases and --gligen-boxes go together")
    if args.gligen_phrases is not None and args.gligen_layouts is not None:
        p.error("--gligen-layouts replaces --gligen-phrases / --gligen-boxes")
    if args.gligen_boxes is not None and len(args.gligen_boxes) != 4 * len(args.gligen_phrases):
        p.error(f"--gligen-boxes takes four values per phrase ({len(args.gligen_phrases)} phrases, {len(args.gligen_boxes)} values)")
    if (args.gligen_phrases is not None or args.gligen_layouts is not None) and (args.controlnet_model_path or args.init_image):
        p.error("GLIGEN with ControlNet or inpainting is not implemented")
    for name in ("height", "width"):
        v = getattr(args, name)
        if v is not None and (v < 1 or v % 64):
            p.error(f"--{name} {v}: a positive multiple of 64")
    if args.view_batch_size is not None and not args.panorama:
        p.error("--view-batch-size needs --panorama")
    region = args.region_prompts is not None or args.region_layouts is not None
    if not region and (args.region_boxes is not None or args.region_masks is not None or args.bootstrapping is not None):
        p.error("--region-boxes / --region-masks / --bootstrapping need --region-prompts or --region-layouts")
    if region:
        # everything StableDiffusionRegionPipeline refuses is refused here, before a device is touched
        if (args.panorama or args.gligen_phrases is not None or args.gligen_layouts is not None or args.controlnet_model_path or args.control_image
                or args.adapter_model_path or args.ip_adapter_path or args.init_image or args.instruct_image):
            p.error("region prompts with --panorama, GLIGEN, ControlNet, a T2I-Adapter, an IP-Adapter, inpainting or InstructPix2Pix are not implemented")
        if args.guidance_rescale or args.pag_scale or (args.deepcache_interval or 1) > 1 or args.max_embeddings_multiples is not None:
            p.error("region prompts with --guidance-rescale, --pag-scale, --deepcache-interval or --max-embeddings-multiples are not implemented")
        if args.region_layouts is not None and (args.region_prompts is not None or args.region_boxes is not None or args.region_masks is not None):
            p.error("--region-layouts replaces --region-prompts / --region-boxes / --region-masks")
        if args.region_prompts is not None and (args.region_boxes is None) == (args.region_masks is None):
            p.error("--region-prompts takes exactly one of --region-boxes and --region-masks")
        if args.region_boxes is not None and len(args.region_boxes) != 4 * len(args.region_prompts):
            p.error(f"--region-boxes takes four values per region prompt ({len(args.region_prompts)} prompts, {len(args.region_boxes)} values)")
        if args.region_masks is not None and len(args.region_masks) != len(args.region_prompts):
            p.error(f"--region-masks takes one file per region prompt ({len(args.region_prompts)} prompts, {len(args.region_masks)} files)")
        if args.bootstrapping is not None and args.bootstrapping < 0:
            p.error(f"--bootstrapping {args.bootstrapping}: a number of steps >= 0")
        if args.scheduler is None:
            args.scheduler = "DDIMScheduler"
        from .regions import check_region_args, check_region_count
        try:
            for lay in region_layouts_from_args(args):                        # (mask files are opened, and their size checked, per batch)
                if lay["boxes"] is not None:
                    check_region_args(args.scheduler, len(lay["prompts"]), None, lay["boxes"], 64, 64)
                else:
                    check_region_count(args.scheduler, len(lay["prompts"]))
        except (ValueError, OSError) as e:
            p.error(f"region prompts: {e}")
    if args.panorama:
        # everything StableDiffusionPanoramaPipeline refuses is refused here, before a device is touched
        if args.controlnet_model_path or args.init_image or args.gligen_phrases is not None or args.gligen_layouts is not None:
            p.error("--panorama with ControlNet, inpainting or GLIGEN is not implemented")
        if args.scheduler is None:
            args.scheduler = "DDIMScheduler"
        from .panorama import check_panorama_args
        window = panorama_window(args)
        args.height = args.height or 8 * window
        args.width = args.width or 4 * args.height
        try:
            check_panorama_args(args.scheduler, args.height, args.width, window, args.view_batch_size)
        except ValueError as e:
            p.error(f"--panorama: {e}")
    return args


def apply_schedule_flags(pipe, timestep_spacing: Optional[str], rescale_betas_zero_snr: bool) -> None:
    """--timestep-spacing / --rescale-betas-zero-snr on a built pipeline: the scheduler config takes them and the pipeline's scheduler is
    built again from it (every rank does the same).  DPM-Solver++ takes the spacing as its own; PNDM and DPM-Solver++ refuse what they
    do not implement, by name (ValueError)."""
    from .scheduler import DPMSolverMultistepScheduler
    sc = pipe.cfg.sched
    if timestep_spacing is not None:
        if isinstance(pipe.scheduler, DPMSolverMultistepScheduler):
            sc.timestep_spacing = timestep_spacing
        else:
            sc.ddim_timestep_spacing = timestep_spacing
    if rescale_betas_zero_snr:
        sc.rescale_betas_zero_snr = True
    pipe.scheduler = type(pipe.scheduler).from_config(sc)


def panorama_window(args) -> int:
    """The view side in latent pixels of the model the arguments name: the checkpoint's UNet `sample_size`, or the synthetic config's."""
    if args.pretrained_model_path:
        with open(os.path.join(args.pretrained_model_path, "unet", "config.json")) as f:
            return int(json.load(f).get("sample_size", 64))
    from .config import CONFIGS
    return int(CONFIGS[args.synthetic_config]().default_sample_size)


def gligen_layouts_from_args(args) -> Optional[List[dict]]:
    """The GLIGEN layouts of the run: one from --gligen-phrases / --gligen-boxes, or the list of --gligen-layouts; None without either."""
    if args.gligen_layouts is not None:
        with open(args.gligen_layouts) as f:
            lays = json.load(f)
        if not isinstance(lays, list) or not lays or not all(isinstance(x, dict) and {"phrases", "boxes"} <= set(x) for x in lays):
            raise ValueError(f"{args.gligen_layouts}: a non-empty list of {{'phrases': [...], 'boxes': [...]}} objects")
        return [{"phrases": list(x["phrases"]), "boxes": [list(map(float, b)) for b in x["boxes"]]} for x in lays]
    if args.gligen_phrases is None:
        return None
    v = args.gligen_boxes
    return [{"phrases": list(args.gligen_phrases), "boxes": [v[4 * i: 4 * i + 4] for i in range(len(args.gligen_phrases))]}]


def region_layouts_from_args(args) -> Optional[List[dict]]:
    """The region layouts of the run: one from --region-prompts with --region-boxes or --region-masks, or the list of --region-layouts;
    None without either.  A layout is {"prompts": [...], "boxes": [[x0, y0, x1, y1], ...] or None, "masks": [files] or None}."""
    if args.region_layouts is not None:
        with open(args.region_layouts) as f:
            lays = json.load(f)
        if not isinstance(lays, list) or not lays or not all(isinstance(x, dict) and {"prompts", "boxes"} <= set(x) for x in lays):
            raise ValueError(f"{args.region_layouts}: a non-empty list of {{'prompts': [...], 'boxes': [...]}} objects")
        return [{"prompts": list(x["prompts"]), "boxes": [list(map(float, b)) for b in x["boxes"]], "masks": None} for x in lays]
    if args.region_prompts is None:
        return None
    v = args.region_boxes
    return [{"prompts": list(args.region_prompts), "masks": list(args.region_masks) if args.region_masks is not None else None,
             "boxes": None if v is None else [v[4 * i: 4 * i + 4] for i in range(len(args.region_prompts))]}]


def region_inputs_for(layout: dict, bootstrapping: Optional[int]) -> dict:
    """The region pipeline's keyword arguments for a batch whose images share `layout`."""
    from PIL import Image
    kw = {"region_prompts": layout["prompts"]}
    if layout["boxes"] is not None:
        kw["region_boxes"] = layout["boxes"]
    else:
        kw["region_masks"] = [Image.open(f).convert("L") for f in layout["masks"]]
    if bootstrapping is not None:
        kw["bootstrapping"] = bootstrapping
    return kw


def generate_region_batch(pipe, layouts: Sequence[dict], bootstrapping: Optional[int], seeds: Sequence[int], words, **kw):
    """`generate_batch` for region prompts: seed s takes layout s mod n; the seeds of one layout run as one call (a call's images share its
    region prompts), and the results come back in the order of `seeds`.  The bootstrap draws come from a CPU generator seeded with the
    first seed of each call, so a batch paints the same images in every run."""
    groups = {}
    for k, s_ in enumerate(seeds):
        groups.setdefault(int(s_) % len(layouts), []).append(k)
    imgs, hms = [None] * len(seeds), [None] * len(seeds)
    for li, ks in groups.items():
        sub = [seeds[k] for k in ks]
        control = dict(region_inputs_for(layouts[li], bootstrapping), generator=torch.Generator().manual_seed(int(sub[0])))
        im, hm = generate_batch(pipe, sub, words, control=control, **kw)
        for j, k in enumerate(ks):
            imgs[k], hms[k] = im[j], hm[j]
    return torch.stack(imgs), torch.stack(hms)


def write_region_layouts(save_dir: str, records: dict):
    """region_layouts.json: each saved image's file name -> its region prompts and boxes (normalised and in saved-image pixels) or mask files."""
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "region_layouts.json"), "w") as f:
        json.dump(records, f, indent=2, sort_keys=True)


def region_records(seeds, layouts, image_size, images_dir: Optional[str] = None) -> dict:
    """The region_layouts.json entries of the seeds whose image was written (`images_dir` given: skipped black images have no file)."""
    sh, sw = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
    out = {}
    for s in seeds:
        name = f"{s}.png"
        if images_dir is not None and not os.path.exists(os.path.join(images_dir, name)):
            continue
        lay = layouts[int(s) % len(layouts)]
        out[name] = {"prompts": lay["prompts"]}
        if lay["boxes"] is not None:
            out[name].update(boxes=lay["boxes"], boxes_px=[[b[0] * sw, b[1] * sh, b[2] * sw, b[3] * sh] for b in lay["boxes"]])
        else:
            out[name].update(masks=lay["masks"])
    return out


def gligen_inputs_for(layouts: Sequence[dict], seeds: Sequence[int], beta: float) -> dict:
    """The GLIGEN pipeline's keyword arguments for a batch: seed s takes layout s mod n, one layout per image (the per-image extension)."""
    lay = [layouts[int(s) % len(layouts)] for s in seeds]
    return {"gligen_phrases": [x["phrases"] for x in lay], "gligen_boxes": [x["boxes"] for x in lay], "gligen_scheduled_sampling_beta": beta}


def write_gligen_layouts(save_dir: str, records: dict):
    """gligen_layouts.json: each saved image's file name -> its phrases and boxes, normalised and in saved-image pixels."""
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "gligen_layouts.json"), "w") as f:
        json.dump(records, f, indent=2, sort_keys=True)


def gligen_records(seeds, layouts, image_size, images_dir: Optional[str] = None) -> dict:
    """The gligen_layouts.json entries of the seeds whose image was written (`images_dir` given: skipped black images have no file)."""
    sh, sw = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
    out = {}
    for s in seeds:
        name = f"{s}.png"
        if images_dir is not None and not os.path.exists(os.path.join(images_dir, name)):
            continue
        lay = layouts[int(s) % len(layouts)]
        out[name] = {"phrases": lay["phrases"], "boxes": lay["boxes"],
                     "boxes_px": [[b[0] * sw, b[1] * sh, b[2] * sw, b[3] * sh] for b in lay["boxes"]]}
    return out


def control_image_files(path: str) -> List[str]:
    """The control image of every seed: one file, or a directory's image files in sorted order (seed s takes file s mod n)."""
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith((".png", ".jpg", ".jpeg", ".bmp", ".webp")))
        if not files:
            raise FileNotFoundError(f"no control images in {path}")
        return files
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    return [path]


def control_images_for(files: Sequence[str], seeds: Sequence[int]):
    from PIL import Image
    return [Image.open(files[s % len(files)]).convert("RGB") for s in seeds]


def ip_adapter_images_for(files: Sequence[str], seeds: Sequence[int]):
    """The image prompt of every seed (seed s takes file s mod n), as RGB PIL images resized to the first one's size (the encoder's own
    front end then resizes and crops to its input)."""
    from PIL import Image
    ims = [Image.open(files[int(s) % len(files)]).convert("RGB") for s in seeds]
    return [im if im.size == ims[0].size else im.resize(ims[0].size, Image.BICUBIC) for im in ims]


def adapter_images_for(files: Sequence[str], seeds: Sequence[int], in_channels: int = 3):
    """The adapter's conditioning image of every seed (seed s takes file s mod n): "L" for a 1-channel adapter, else RGB."""
    from PIL import Image
    return [Image.open(files[s % len(files)]).convert("L" if in_channels == 1 else "RGB") for s in seeds]


def inpaint_inputs_for(pairs: Sequence, seeds: Sequence[int], strength: float) -> dict:
    """The inpainting call's image / mask_image of every seed (seed s takes pair s mod n) and strength.  The start noise is the seeds'
    latents (generate_batch passes them); the VAE posterior draws come from a CPU generator seeded with the batch's first seed, so a
    batch paints the same images in every run."""
    from PIL import Image
    picked = [pairs[s % len(pairs)] for s in seeds]
    return {"image": [Image.open(i).convert("RGB") for i, _ in picked], "mask_image": [Image.open(m).convert("L") for _, m in picked],
            "strength": strength, "generator": torch.Generator().manual_seed(int(seeds[0]))}


def ip2p_inputs_for(files: Sequence[str], seeds: Sequence[int], image_guidance_scale: float) -> dict:
    """The InstructPix2Pix call's image of every seed (seed s takes file s mod n), the image guidance scale and the images' size (the
    call's height and width; the images of one batch must share it)."""
    from PIL import Image
    ims = [Image.open(files[s % len(files)]).convert("RGB") for s in seeds]
    sizes = {i.size for i in ims}
    if len(sizes) != 1:
        raise ValueError(f"the --instruct-image files of one batch must share one size, got {sorted(sizes)}")
    w, h = ims[0].size
    return {"image": ims, "image_guidance_scale": image_guidance_scale, "height": h, "width": w}


def main(argv=None):
    import torch.distributed as dist
    from . import StableDiffusionPipeline
    args = parse_args(argv)
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if "AGD_FORCE_DEVICE" in os.environ:          # rehearsal of the multi-rank path on a 1-GPU box (ranks share one card)
        local = int(os.environ["AGD_FORCE_DEVICE"])
    torch.cuda.set_device(local)
    own_group = False
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("AGD_DIST_BACKEND", "nccl"))          # "nccl" = RCCL on ROCm
        own_group = True
    kw = {"safety_checker": None} if args.no_safety_checker else {}
    cls, cn_files = StableDiffusionPipeline, None
    gl_layouts = gligen_layouts_from_args(args)
    if gl_layouts is not None:
        from .gligen import StableDiffusionGLIGENPipeline
        cls = StableDiffusionGLIGENPipeline
    if args.controlnet_model_path:
        from .controlnet import ControlNetModel, StableDiffusionControlNetPipeline
        cls = StableDiffusionControlNetPipeline
        kw["controlnet"] = ControlNetModel.from_pretrained(args.controlnet_model_path)
        cn_files = control_image_files(args.control_image)
    ad_files = None
    if args.adapter_model_path:
        from .adapter import StableDiffusionAdapterPipeline, T2IAdapter
        cls = StableDiffusionAdapterPipeline
        kw["adapter"] = T2IAdapter.from_pretrained(args.adapter_model_path)
        ad_files = control_image_files(args.adapter_image)
    ip_files = None
    if args.init_image:
        from .inpaint import StableDiffusionInpaintPipeline
        cls = StableDiffusionInpaintPipeline
        ip_files = list(zip(control_image_files(args.init_image), control_image_files(args.mask_image)))
        if len(ip_files) != len(control_image_files(args.init_image)) or len(ip_files) != len(control_image_files(args.mask_image)):
            raise ValueError(f"{args.init_image} and {args.mask_image} hold different numbers of images")
    if args.panorama:
        from .panorama import StableDiffusionPanoramaPipeline
        cls = StableDiffusionPanoramaPipeline
    rg_layouts = region_layouts_from_args(args)
    if rg_layouts is not None:
        from .regions import StableDiffusionRegionPipeline
        cls = StableDiffusionRegionPipeline
    i2_files = None
    if args.instruct_image:
        from .ip2p import StableDiffusionInstructPix2PixPipeline
        cls = StableDiffusionInstructPix2PixPipeline
        i2_files = control_image_files(args.instruct_image)
    pipe = (cls.from_pretrained(args.pretrained_model_path, device=local, scheduler=args.scheduler, **kw)
            if args.pretrained_model_path else
            cls.from_synthetic(args.synthetic_config, device=local, scheduler=args.scheduler or "DDIMScheduler",
                               **({"controlnet": kw["controlnet"]} if cn_files else {}), **({"adapter": kw["adapter"]} if ad_files else {})))
    if args.lora_path:
        pipe.load_lora_weights(args.lora_path, weight_name=args.lora_weight_name)
        pipe.fuse_lora(lora_scale=args.lora_scale)
    if args.freeu is not None:
        pipe.enable_freeu(*args.freeu)
    if args.pag_applied_layers is not None:
        pipe.set_pag_applied_layers(args.pag_applied_layers)
    if args.deepcache_interval is not None:
        pipe.enable_deepcache(cache_interval=args.deepcache_interval, cache_branch_id=args.deepcache_branch or 0)
    ipa_files = None
    if args.ip_adapter_path:
        pipe.load_ip_adapter(args.ip_adapter_path, image_encoder_folder=args.image_encoder_path or "image_encoder")
        pipe.set_ip_adapter_scale(args.ip_adapter_scale)
        ipa_files = control_image_files(args.ip_adapter_image)
    if args.use_karras_sigmas:
        from .scheduler import DPMSolverMultistepScheduler
        pipe.cfg.sched.use_karras_sigmas = True
        pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.cfg.sched)
    if args.timestep_spacing is not None or args.rescale_betas_zero_snr:
        apply_schedule_flags(pipe, args.timestep_spacing, args.rescale_betas_zero_snr)
    embeds = torch.load(args.learnable_tokens_embedding_path) if args.learnable_tokens_embedding_path else {}
    if embeds:
        new_tokens, words, prompt = select_learned_tokens(args.prompt, args.initialize_token, list(embeds.keys()),
                                                         args.word_token_heatmaps, args.store_learnable_token_heatmaps)
        inject_learned_tokens(pipe, embeds, new_tokens)
    else:       # no learned-token file (the reference requires one): plain prompt, placeholders dropped
        words = args.word_token_heatmaps if args.word_token_heatmaps is not None else []
        prompt = " ".join(args.prompt.replace("{}", " ").split())
    seeds = shard_seeds(args.num_images, rank, world)
    gather = world > 1 and not args.no_gather
    # every rank joins every round (the collective count must match): ranks whose shard ran out contribute zero rows
    per_rank = (args.num_images + world - 1) // world
    rounds = (per_rank + args.batch_size - 1) // args.batch_size if gather else (len(seeds) + args.batch_size - 1) // args.batch_size
    S = args.image_size
    gl_done, rg_done = {}, {}
    for r in range(rounds):
        chunk = seeds[r * args.batch_size:(r + 1) * args.batch_size]
        if chunk:
            control = None
            if cn_files:
                control = {"image": control_images_for(cn_files, chunk), "controlnet_conditioning_scale": args.controlnet_conditioning_scale,
                           "control_guidance_start": args.control_guidance_start, "control_guidance_end": args.control_guidance_end}
            if ad_files:
                control = {"image": adapter_images_for(ad_files, chunk, pipe.adapter_cfg.in_channels),
                           "adapter_conditioning_scale": args.adapter_conditioning_scale, "adapter_conditioning_factor": args.adapter_conditioning_factor}
            if ip_files:
                control = inpaint_inputs_for(ip_files, chunk, args.strength)
            if gl_layouts is not None:
                control = gligen_inputs_for(gl_layouts, chunk, args.gligen_beta)
            if args.panorama:
                control = {"view_batch_size": args.view_batch_size}
            if ipa_files is not None:
                control = {"ip_adapter_image": ip_adapter_images_for(ipa_files, chunk)}
            height, width = args.height, args.width
            if i2_files:                                                             # (parse_args refused --height / --width: both are None)
                control = ip2p_inputs_for(i2_files, chunk, args.image_guidance_scale)
                height, width = control.pop("height"), control.pop("width")          # the image's size is the call's
            if args.guidance_rescale:
                control = dict(control or {}, guidance_rescale=args.guidance_rescale)
            if args.pag_scale:
                control = dict(control or {}, pag_scale=args.pag_scale, pag_adaptive_scale=args.pag_adaptive_scale)
            if args.max_embeddings_multiples is not None:
                control = dict(control or {}, max_embeddings_multiples=args.max_embeddings_multiples)
            if args.sega is not None:
                control = dict(control or {}, **args.sega)
            if rg_layouts is not None:                                               # (parse_args refused every other control)
                imgs, hms = generate_region_batch(pipe, rg_layouts, args.bootstrapping, chunk, words, prompt=prompt,
                                                  num_inference_steps=args.num_inference_steps, height=height, width=width)
            else:
                imgs, hms = generate_batch(pipe, chunk, words, prompt=prompt, num_inference_steps=args.num_inference_steps, control=control,
                                           height=height, width=width)
        if not gather:
            save_outputs(args.save_dir, chunk, imgs, hms, words, S, stack_words=args.stack)
            if gl_layouts is not None:
                gl_done.update(gligen_records(chunk, gl_layouts, S, os.path.join(args.save_dir, "images")))
                write_gligen_layouts(args.save_dir, gl_done)
            if rg_layouts is not None:
                rg_done.update(region_records(chunk, rg_layouts, S, os.path.join(args.save_dir, "images")))
                write_region_layouts(args.save_dir, rg_done)
            continue
        # export on the producing GPU (resize 512 -> S, min-max -> uint8 -> resize), then ONE gather of the finished
        # payloads (S*S*3 + S*S per word bytes per image instead of the full-size tensors); rank 0 writes the files
        from . import export
        dev = torch.device("cuda", local)
        if chunk:
            small, hm8 = export.export_batch(imgs, hms, S)
        else:
            sh, sw = (S, S) if isinstance(S, int) else S
            small = torch.zeros(0, sh, sw, 3, dtype=torch.uint8, device=dev)
            hm8 = torch.zeros(0, len(words), sh, sw, dtype=torch.uint8, device=dev)
        if dist.get_backend() == "gloo":
            small, hm8 = small.cpu(), hm8.cpu()
        round_seeds = sorted(s_ for rk in range(world) for s_ in shard_seeds(args.num_images, rk, world)[r * args.batch_size:(r + 1) * args.batch_size])
        all_seeds, small, hm8 = gather_outputs(small, hm8, seeds=chunk, max_batch=args.batch_size, global_seeds=round_seeds)
        if rank == 0:
            save_outputs(args.save_dir, all_seeds, small, hm8, words, S, stack_words=args.stack, exported=True)
            if gl_layouts is not None:
                gl_done.update(gligen_records(all_seeds, gl_layouts, S, os.path.join(args.save_dir, "images")))
                write_gligen_layouts(args.save_dir, gl_done)
            if rg_layouts is not None:
                rg_done.update(region_records(all_seeds, rg_layouts, S, os.path.join(args.save_dir, "images")))
                write_region_layouts(args.save_dir, rg_done)
    if world > 1:
        dist.barrier()
        if own_group:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
