"""An independent restatement of the weighted / long prompt rules (no test in here), written from the rules alone -- a character walk
for the grammar, numpy for the rows -- to compare agenda_amd/lpw.py with:

grammar   `(x)` weight x 1.1, `[x]` weight / 1.1, `(x:w)` weight x w, nested; `\\(` `\\)` `\\[` `\\]` `\\\\` literal; an unclosed opener runs
          to the end of the text; neighbours of equal weight merge.
rows      n = longest token list of the batch, m_eff = max(1, min(m, (n - 1) // 75 + 1)), T = 75 m_eff + 2,
          row = [bos] + tokens[:T - 2] + [pad] * k + [eos], weights 1 outside the tokens.
chunks    chunk i = row[75 i : 75 i + 77] with bos / eos written over its ends; of the encoder's output chunk 0 keeps rows 0 .. 75, a middle
          chunk rows 1 .. 75, the last chunk rows 1 .. 76, a single chunk all 77.
weights   emb * w, then times mean(before) / mean(after), per prompt.
rows of words   token i of the weight-stripped stream is context row i + 1."""
import numpy as np

NUM = "+-.0123456789"


def parse(text):
    out = []            # [piece, weight]
    opened = []         # (kind, index into out)

    def close(kind, factor):
        for j in range(len(opened) - 1, -1, -1):
            if opened[j][0] == kind:
                start = opened.pop(j)[1]
                for piece in out[start:]:
                    piece[1] *= factor
                return True
        return False

    i, n, buf = 0, len(text), ""

    def flush():
        nonlocal buf
        if buf:
            out.append([buf, 1.0])
            buf = ""

    while i < n:
        ch = text[i]
        if ch == "\\" and i + 1 < n and text[i + 1] in "()[]\\":
            flush()
            out.append([text[i + 1], 1.0])
            i += 2
        elif ch == "\\":
            flush()
            out.append(["\\", 1.0])
            i += 1
        elif ch in "([":
            flush()
            opened.append((ch, len(out)))
            i += 1
        elif ch == ":":
            j = i + 1
            while j < n and text[j] in NUM:
                j += 1
            has_round = any(k == "(" for k, _ in opened)
            if j > i + 1 and j < n and text[j] == ")" and any(c.isdigit() or c == "." for c in text[i + 1:j]):
                flush()
                if has_round:
                    close("(", float(text[i + 1:j]))
                else:
                    out.append([text[i:j + 1], 1.0])
                i = j + 1
            else:
                flush()
                out.append([":", 1.0])
                i += 1
        elif ch == ")":
            flush()
            if not close("(", 1.1):
                out.append([")", 1.0])
            i += 1
        elif ch == "]":
            flush()
            if not close("[", 1 / 1.1):
                out.append(["]", 1.0])
            i += 1
        else:
            buf += ch
            i += 1
    flush()
    for kind, start in opened:
        for piece in out[start:]:
            piece[1] *= 1.1 if kind == "(" else 1 / 1.1
    if not out:
        out = [["", 1.0]]
    merged = [out[0]]
    for piece in out[1:]:
        if piece[1] == merged[-1][1]:
            merged[-1][0] += piece[0]
        else:
            merged.append(piece)
    return merged


def context_tokens(n, m):
    return 75 * max(1, min(m, (n - 1) // 75 + 1)) + 2


def rows(id_lists, weight_lists, m, bos, eos, pad):
    T = context_tokens(max(len(x) for x in id_lists), m)
    ids = np.full((len(id_lists), T), pad, dtype=np.int64)
    ws = np.ones((len(id_lists), T), dtype=np.float32)
    for r, (a, w) in enumerate(zip(id_lists, weight_lists)):
        a, w = list(a)[:T - 2], list(w)[:T - 2]
        ids[r, 0], ids[r, -1] = bos, eos
        ids[r, 1:1 + len(a)] = a
        ws[r, 1:1 + len(w)] = w
    return ids, ws, T


def chunks(ids, bos, eos):
    out = []
    for row in ids:
        for i in range((len(row) - 2) // 75):
            c = np.array(row[75 * i:75 * i + 77])
            c[0], c[-1] = bos, eos
            out.append(c)
    return np.stack(out)


def join(emb, N):
    """emb [N * n, 77, D] -> [N, 75 n + 2, D]"""
    n = emb.shape[0] // N
    res = []
    for r in range(N):
        parts = []
        for i in range(n):
            c = emb[r * n + i]
            lo = 0 if i == 0 else 1
            hi = 77 if i == n - 1 else 76
            parts.append(c[lo:hi])
        res.append(np.concatenate(parts, 0))
    return np.stack(res)


def weigh(emb, ws):
    out = []
    for e, w in zip(emb.astype(np.float32), ws.astype(np.float32)):
        m0 = e.mean(dtype=np.float32)
        e2 = e * w[:, None]
        out.append(e2 * (m0 / e2.mean(dtype=np.float32)))
    return np.stack(out)


def word_rows(stream, word_tokens):
    """context rows of every occurrence of the word's tokens in the stream"""
    k = len(word_tokens)
    return [s + j + 1 for s in range(len(stream) - k + 1) if stream[s:s + k] == word_tokens for j in range(k)]
