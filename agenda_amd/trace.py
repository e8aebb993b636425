"""`daam.trace` surface (reference data_generation/data_generation.py:57,64,74-77) over the fused
HIP recorder.  Semantics restated from the public `daam` package [upstream-knowledge, SURVEY.md
§8a rows D1-D4]: per-(layer, head) time-summed conditional-half maps, mid block excluded,
bicubic -> clamp -> mean, rows truncated to len(tokenize(prompt)) + 2.

Rectangular generates (height != width) give maps of [rows, Lh, Lw].  daam itself is square-only (its `_unravel_attn` takes
h = w = sqrt(N)); here a layer's maps are (Lh / f) x (Lw / f) with daam's own factor f = sqrt(Lh * Lw / N), resized by bicubic with
separate y and x scales (torch `F.interpolate(size=(Lh, Lw), mode="bicubic", align_corners=False)`).  That is the direct
generalisation of daam's formula, not a behaviour daam has: parity-unpinned.  Square generates are exactly daam's.

A panorama (StableDiffusionPanoramaPipeline) gives maps [rows, Lh, Lw] over the whole canvas: every view's global map, computed exactly as
for a square generate of the window size, then the mean over the views that cover each latent pixel (the rule that fuses the latents).
daam has no panorama support; this definition is this project's (parity-unpinned).

A region call (StableDiffusionRegionPipeline) keeps one DAAM state per (region r, image p), image r * B + p of the recorder:
`compute_global_heat_map(image_index=p, region=r)` gives region r's maps, rows and word lookup following region r's prompt (region None =
region 0, the background).  `compute_region_word_heat_map(word, image_index=p)` is the canvas map [Lh, Lw] = sum_r m_r w_r / sum_r m_r with
m_r the region's latent mask and w_r its word heat map of `word`; a region whose prompt does not contain the word contributes zeros.  The map
of "car" over the canvas is thus composed from the regions that generated each pixel.  daam has no such notion; this definition is this
project's (parity-unpinned).

A context of more than 77 rows (`max_embeddings_multiples`, or long `prompt_embeds`): daam records 77-wide maps only, so this too is the
project's definition (parity-unpinned).  The recorder keeps all T context rows (unless the tracer was given `rec_tokens`); the global map
is truncated to tokens + 2 rows, counted on the weight-stripped token stream of the prompt (every weighted piece tokenised on its own, cut
to T - 2); token i of that stream is row i + 1 -- the rows are contiguous, the middle chunks' bos / eos rows are not part of the context --
and `compute_word_heat_map(word)` finds the word in that stream."""
from __future__ import annotations

from typing import List, Optional

import torch


def compute_token_merge_indices(tokenizer, prompt: str, word: str, word_idx: Optional[int] = None, offset_idx: int = 0):
    """`daam.utils.compute_token_merge_indices` (also used by reference dataset.py:93)."""
    merge_idxs: List[int] = []
    tokens = [x.replace("</w>", "") for x in tokenizer.tokenize(prompt.lower())]
    if word_idx is None:
        word = word.lower()
        search = [x.replace("</w>", "") for x in tokenizer.tokenize(word)]
        starts = [x + offset_idx for x in range(len(tokens)) if tokens[x:x + len(search)] == search]
        for s in starts:
            merge_idxs += [i + s for i in range(len(search))]
        if not merge_idxs:
            raise ValueError(f"Search word {word} not found in prompt!")
    else:
        merge_idxs.append(word_idx)
    return [x + 1 for x in merge_idxs], word_idx


def token_stream_merge_indices(tokenizer, tokens: List[str], word: str, word_idx: Optional[int] = None, offset_idx: int = 0):
    """`compute_token_merge_indices` on a token stream that is already there (a weighted prompt's, lpw.tokenize_weighted): token i is row i + 1"""
    if word_idx is not None:
        return [word_idx + 1], word_idx
    strip = lambda xs: [x.replace("</w>", "").lower() for x in xs]          # noqa: E731
    stream, search = strip(tokens), strip(tokenizer.tokenize(word.lower()))
    starts = [x for x in range(len(stream)) if search and stream[x:x + len(search)] == search]
    if not starts:
        raise ValueError(f"Search word {word} not found in prompt!")
    return [i + s + offset_idx + 1 for s in starts for i in range(len(search))], None


class WordHeatMap:
    def __init__(self, heatmap: torch.Tensor, word: str):
        self.heatmap = heatmap
        self.word = word

    @property
    def value(self):
        return self.heatmap


class GlobalHeatMap:
    def __init__(self, tokenizer, prompt: str, heat_maps: torch.Tensor, tokens: Optional[List[str]] = None):
        self.tokenizer, self.prompt, self.heat_maps = tokenizer, prompt, heat_maps
        self.tokens = tokens                 # a weighted prompt's weight-stripped token stream (the words are looked up there), else None

    def compute_word_heat_map(self, word: str, word_idx: Optional[int] = None, offset_idx: int = 0) -> WordHeatMap:
        if self.tokens is not None:
            merge_idxs, _ = token_stream_merge_indices(self.tokenizer, self.tokens, word, word_idx, offset_idx)
        else:
            merge_idxs, _ = compute_token_merge_indices(self.tokenizer, self.prompt, word, word_idx, offset_idx)
        if max(merge_idxs) >= self.heat_maps.shape[0]:
            raise ValueError(f"token index {max(merge_idxs)} beyond the {self.heat_maps.shape[0]} recorded rows")
        # (integer indexing: views, no index tensor uploaded through a blocking copy)
        return WordHeatMap(torch.stack([self.heat_maps[int(i)] for i in merge_idxs]).mean(0), word)


class trace:
    """`with trace(pipe) as trc: pipe(...); trc.compute_global_heat_map()`."""

    def __init__(self, pipe, rec_tokens: Optional[int] = None):
        self.pipe = pipe
        # recording fewer rows than 77 is safe: daam only ever reads the first len(tokens)+2 rows
        self.rec_tokens = rec_tokens or pipe.cfg.max_tokens
        self._rec_given = bool(rec_tokens)
        self._rows = self.rec_tokens         # rows the recorder of the last generate kept
        self.last_tokens = None
        self.batch = 0
        self.latent_side = 0                 # the latent side, or (Lh, Lw) after a rectangular generate
        self.last_prompt = None
        self._ran = False

    def __enter__(self):
        if self.pipe._trace is not None:
            raise RuntimeError("a trace is already active on this pipeline")
        self.pipe._trace = self
        self.pipe._apply_record_mode()
        return self

    def __exit__(self, *exc):
        self.pipe._trace = None
        self.pipe._apply_record_mode()
        return False

    def _rows_for(self, context_tokens: Optional[int]) -> int:
        """rows recorded under a context of that many tokens: all of a long one (over 96) unless rec_tokens was given"""
        if context_tokens is not None and context_tokens > 96 and not self._rec_given:
            return context_tokens
        return self.rec_tokens

    def _on_generate(self, batch: int, latent_side, prompt: Optional[str], panorama: bool = False, tokens: Optional[List[str]] = None,
                     context_tokens: Optional[int] = None, regions: Optional[dict] = None):
        self.batch, self.latent_side, self.last_prompt, self._ran = batch, latent_side, prompt, True
        self.last_tokens, self._rows = tokens, self._rows_for(context_tokens)
        self.panorama = panorama             # a StableDiffusionPanoramaPipeline call: latent_side is the canvas (Lh, Lw)
        # a StableDiffusionRegionPipeline call: {"prompts": [background, region 1, ...] or None, "masks": [R, B, Lh, Lw], "count": R}
        self.regions = regions

    def compute_global_heat_map(self, prompt: Optional[str] = None, image_index: int = 0, normalize: bool = False,
                                region: Optional[int] = None) -> GlobalHeatMap:
        """Heat maps [rows, Lh, Lw] of image `image_index` (word maps from it are [Lh, Lw]).  `region`: after a region call, the region
        whose DAAM state and prompt are read (None: region 0, the background)."""
        if not self._ran:
            raise RuntimeError("No heat maps found. Did you forget to call `with trace(...)`?")
        regions = getattr(self, "regions", None)
        if regions is None:
            if region is not None:
                raise ValueError(f"region={region!r}: the last generate was not a StableDiffusionRegionPipeline call")
        else:
            r = 0 if region is None else int(region)
            if not 0 <= r < regions["count"] or not 0 <= image_index < self.batch:
                raise ValueError(f"region {r} of {regions['count']}, image {image_index} of {self.batch}")
            if prompt is None and regions["prompts"] is not None:
                prompt = regions["prompts"][r]
            image_index = r * self.batch + image_index
        # the weighted prompt of the last generate is counted on its own token stream; any other prompt given here as daam counts it
        tokens = self.last_tokens if prompt is None or prompt == self.last_prompt else None
        prompt = prompt if prompt is not None else self.last_prompt
        rows = self._rows
        if tokens is not None:
            rows = min(rows, len(tokens) + 2)
        elif prompt is not None:
            rows = min(rows, len(self.pipe.tokenizer.tokenize(prompt)) + 2)   # 1 for SOS and 1 for padding
        if getattr(self, "panorama", False):
            maps = self.pipe.engine.daam_global_panorama(image_index, rows, self.latent_side)
        else:
            maps = self.pipe.engine.daam_global(image_index, rows, self.latent_side)
        if normalize:
            maps = maps / (maps[1:-1].sum(0, keepdim=True) + 1e-6)
        return GlobalHeatMap(self.pipe.tokenizer, prompt or "", maps, tokens)

    def compute_region_word_heat_map(self, word: str, image_index: int = 0, word_idx: Optional[int] = None) -> WordHeatMap:
        """The canvas map [Lh, Lw] of `word` after a region call: sum_r m_r w_r / sum_r m_r, with w_r region r's word heat map and m_r its
        latent mask; a region whose prompt does not contain the word contributes zeros (a word no region contains raises).  `word_idx`:
        the token position instead of the word, read in every region.  Plain torch on the device tensors."""
        regions = getattr(self, "regions", None)
        if not self._ran or regions is None:
            raise RuntimeError("compute_region_word_heat_map needs a StableDiffusionRegionPipeline call under this trace")
        masks = regions["masks"][:, image_index]                 # [R, Lh, Lw]
        num, found = torch.zeros_like(masks[0]), False
        for r in range(regions["count"]):
            g = self.compute_global_heat_map(image_index=image_index, region=r)
            if word_idx is not None:
                if word_idx + 1 >= g.heat_maps.shape[0]:
                    raise ValueError(f"token index {word_idx + 1} beyond the {g.heat_maps.shape[0]} recorded rows")
                w = g.heat_maps[int(word_idx) + 1]
            else:
                try:
                    w = g.compute_word_heat_map(word).heatmap
                except ValueError:
                    continue                                     # not in this region's prompt: zeros
            found = True
            num = num + masks[r] * w
        if not found:
            raise ValueError(f"Search word {word} not found in any region's prompt!")
        den = masks.sum(0)
        return WordHeatMap(torch.where(den > 0, num / den, num), word)
