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
                     context_tokens: Optional[int] = None):
        self.batch, self.latent_side, self.last_prompt, self._ran = batch, latent_side, prompt, True
        self.last_tokens, self._rows = tokens, self._rows_for(context_tokens)
        self.panorama = panorama             # a StableDiffusionPanoramaPipeline call: latent_side is the canvas (Lh, Lw)

    def compute_global_heat_map(self, prompt: Optional[str] = None, image_index: int = 0, normalize: bool = False) -> GlobalHeatMap:
        """Heat maps [rows, Lh, Lw] of image `image_index` (word maps from it are [Lh, Lw])."""
        if not self._ran:
            raise RuntimeError("No heat maps found. Did you forget to call `with trace(...)`?")
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
