"""Weighted and long prompts: `pipe(prompt, max_embeddings_multiples=m)`.

The rules of the diffusers community pipeline `lpw_stable_diffusion` [upstream-knowledge, parity-unpinned], restated:

grammar   `(x)` multiplies the weight of x by 1.1, `[x]` divides it by 1.1, `(x:w)` multiplies it by w; brackets nest; `\\(` `\\)` `\\[`
          `\\]` `\\\\` are literals; an opener that is never closed applies to the end of the text; neighbouring pieces of equal weight merge.
tokens    every piece is tokenised on its own, without BOS / EOS, and its weight repeated per token.
chunks    n = the longest token list over the batch's prompts AND negative prompts; m_eff = min(m, (n - 1) // 75 + 1), at least 1;
          T = 75 m_eff + 2; longer lists are truncated to T - 2 with a warning; row = [bos] + tokens + [pad] * k + [eos], weights of bos /
          pad / eos are 1.  Chunk i is ids [75 i : 75 i + 77] with its first and last id overwritten by bos / eos; all chunks of the batch
          go through the text encoder in one call; chunk 0 loses its last row, the last chunk its first, middle chunks both (one chunk:
          nothing), and the rest is concatenated to T rows.
weights   per prompt: mean0 = emb.mean(); emb *= w[:, None]; emb *= mean0 / emb.mean().  All weights 1 multiply by exactly 1.0.

Token i of the weight-stripped stream is context row i + 1 (rows are contiguous because the middle bos / eos rows are dropped): that is
where `trace` finds a word's heat map."""
from __future__ import annotations

import re
import warnings
from typing import List, Optional, Sequence, Tuple

import torch

CHUNK = 75                    # tokens per chunk (the text encoder's 77 positions less bos / eos)
MAX_MULTIPLES = 4             # 75 * 4 + 2 = 302 rows <= the engine's 320

_RE_ATTENTION = re.compile(r"\\\(|\\\)|\\\[|\\]|\\\\|\\|\(|\[|:([+-]?[.\d]+)\)|\)|]|[^\\()\[\]:]+|:", re.X)


def check_multiples(m) -> Optional[int]:
    """None (the plain path) or an integer 1 .. 4"""
    if m is None:
        return None
    if isinstance(m, bool) or not isinstance(m, int):
        raise TypeError(f"max_embeddings_multiples must be None or an integer 1 .. {MAX_MULTIPLES}, got {m!r}")
    if not 1 <= m <= MAX_MULTIPLES:
        raise ValueError(f"max_embeddings_multiples must be 1 .. {MAX_MULTIPLES}, got {m}")
    return m


def parse_prompt_attention(text: str) -> List[List]:
    """-> [[piece, weight], ...]"""
    res: List[List] = []
    rounds: List[int] = []
    squares: List[int] = []

    def scale_from(start: int, factor: float):
        for p in range(start, len(res)):
            res[p][1] *= factor

    for m in _RE_ATTENTION.finditer(text):
        tok, w = m.group(0), m.group(1)
        if tok.startswith("\\") and len(tok) > 1:
            res.append([tok[1:], 1.0])
        elif tok == "(":
            rounds.append(len(res))
        elif tok == "[":
            squares.append(len(res))
        elif w is not None and rounds:
            scale_from(rounds.pop(), float(w))
        elif tok == ")" and rounds:
            scale_from(rounds.pop(), 1.1)
        elif tok == "]" and squares:
            scale_from(squares.pop(), 1 / 1.1)
        else:
            res.append([tok, 1.0])
    for pos in rounds:
        scale_from(pos, 1.1)
    for pos in squares:
        scale_from(pos, 1 / 1.1)
    if not res:
        res = [["", 1.0]]
    i = 0
    while i + 1 < len(res):                      # neighbours of equal weight merge
        if res[i][1] == res[i + 1][1]:
            res[i][0] += res[i + 1][0]
            res.pop(i + 1)
        else:
            i += 1
    return res


def special_ids(tokenizer) -> Tuple[int, int, int]:
    """(bos, eos, pad) of a CLIPTokenizer, or of the SimpleTokenizer stand-in (which pads with its eos id, as SD-1.x's CLIP does)"""
    bos = getattr(tokenizer, "bos_token_id", None)
    eos = getattr(tokenizer, "eos_token_id", None)
    if bos is None or eos is None:
        bos, eos = tokenizer.convert_tokens_to_ids([tokenizer.bos_token, tokenizer.eos_token])
    pad = getattr(tokenizer, "pad_token_id", None)
    return int(bos), int(eos), int(eos if pad is None else pad)


def _piece_tokens(tokenizer, text: str) -> Tuple[List[int], List[str]]:
    """ids and token strings of one piece, no bos / eos"""
    toks = tokenizer.tokenize(text)
    return [int(i) for i in tokenizer.convert_tokens_to_ids(toks)], list(toks)


def tokenize_weighted(tokenizer, prompt: str) -> Tuple[List[int], List[float], List[str]]:
    """-> (ids, weights, token strings) of the weight-stripped token stream"""
    ids: List[int] = []
    ws: List[float] = []
    toks: List[str] = []
    for piece, w in parse_prompt_attention(prompt):
        pi, pt = _piece_tokens(tokenizer, piece)
        ids += pi
        toks += pt
        ws += [float(w)] * len(pi)
    return ids, ws, toks


def context_tokens(n_longest: int, m: int) -> int:
    """T of a batch whose longest token list has n_longest tokens"""
    m_eff = max(1, min(m, (n_longest - 1) // CHUNK + 1))
    return CHUNK * m_eff + 2


def build_rows(id_lists: Sequence[Sequence[int]], weight_lists: Sequence[Sequence[float]], m: int, bos: int, eos: int, pad: int):
    """-> (ids [N, T] int64, weights [N, T] fp32, T); every list of the batch (prompts and negative prompts) lands in the same T"""
    T = context_tokens(max(len(x) for x in id_lists), m)
    ids = torch.full((len(id_lists), T), pad, dtype=torch.int64)
    ws = torch.ones(len(id_lists), T, dtype=torch.float32)
    cut = [len(x) for x in id_lists if len(x) > T - 2]
    if cut:
        warnings.warn(f"prompt of {max(cut)} tokens truncated to {T - 2} (max_embeddings_multiples={m}: {T} context rows)", stacklevel=3)
    for r, (pi, pw) in enumerate(zip(id_lists, weight_lists)):
        n = min(len(pi), T - 2)
        ids[r, 0] = bos
        ids[r, 1:1 + n] = torch.tensor(list(pi[:n]), dtype=torch.int64)
        ws[r, 1:1 + n] = torch.tensor(list(pw[:n]), dtype=torch.float32)
        ids[r, T - 1] = eos
    return ids, ws, T


def chunk_rows(ids: torch.Tensor, bos: int, eos: int) -> torch.Tensor:
    """ids [N, T] -> [N * n_chunks, 77], the chunks of a row next to each other"""
    N, T = ids.shape
    n = (T - 2) // CHUNK
    out = torch.stack([ids[:, CHUNK * i: CHUNK * i + CHUNK + 2] for i in range(n)], 1).clone()     # [N, n, 77]
    out[:, :, 0] = bos
    out[:, :, -1] = eos
    return out.reshape(N * n, CHUNK + 2)


def join_chunks(emb: torch.Tensor, N: int) -> torch.Tensor:
    """encoder output [N * n, 77, D] -> [N, 75 n + 2, D]"""
    n = emb.shape[0] // N
    emb = emb.reshape(N, n, CHUNK + 2, emb.shape[-1])
    if n == 1:
        return emb[:, 0]
    parts = [emb[:, 0, :-1]] + [emb[:, i, 1:-1] for i in range(1, n - 1)] + [emb[:, n - 1, 1:]]
    return torch.cat(parts, 1)


def apply_weights(emb: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """emb [N, T, D] fp32, ws [N, T]: scale the rows, then restore every prompt's mean"""
    emb = emb.to(torch.float32)
    mean0 = emb.mean(dim=(1, 2))
    emb = emb * ws.to(emb.device)[:, :, None]
    return emb * (mean0 / emb.mean(dim=(1, 2)))[:, None, None]


def encode_ids(text_encoder, ids: torch.Tensor) -> torch.Tensor:
    """`text_encoder(input_ids)[0]` for ids [n, 77]: the project's encoders take ids through `encode_ids`"""
    if not hasattr(text_encoder, "encode_ids"):
        raise TypeError(f"max_embeddings_multiples needs a text encoder with encode_ids(ids); {type(text_encoder).__name__} has none")
    return text_encoder.encode_ids(ids)


def encode_weighted(tokenizer, text_encoder, prompts: Sequence[str], negatives: Sequence[str], m: int):
    """-> (context [2B, T, D] fp32 in CFG order [uncond x B | cond x B], token strings of prompts[0]'s weight-stripped stream, cut to T - 2)"""
    B = len(prompts)
    parsed = [tokenize_weighted(tokenizer, p) for p in list(negatives) + list(prompts)]
    bos, eos, pad = special_ids(tokenizer)
    ids, ws, T = build_rows([p[0] for p in parsed], [p[1] for p in parsed], m, bos, eos, pad)
    emb = join_chunks(encode_ids(text_encoder, chunk_rows(ids, bos, eos)), 2 * B)
    return apply_weights(emb, ws), parsed[B][2][: T - 2]
