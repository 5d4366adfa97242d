"""Not a test: the torch-CPU restatement of vdx/prompt.py and csrc/prompt.hip that the prompt tests compare against, written
independently of both: the parser as a character scanner (no regular expression), the chunker as a flat token stream cut by a
recursive rule, the weighting in float64 sums and torch fp16 / fp32 casts."""
import torch

ROUND, SQUARE, CHUNK, SEQ, BACKTRACK = 1.1, 1 / 1.1, 75, 77, 20
BREAK = ("BREAK", -1.0)


def _number_close(text, i):
    """`:  1.5 )` at text[i] -> (the number, the index behind `)`), or None."""
    j = i + 1
    while j < len(text) and text[j].isspace():
        j += 1
    k = j
    if k < len(text) and text[k] in "+-":
        k += 1
    d0 = k
    while k < len(text) and (text[k].isdigit() or text[k] == "."):
        k += 1
    if k == d0:
        return None
    e = k
    while e < len(text) and text[e].isspace():
        e += 1
    if e < len(text) and text[e] == ")":
        try:
            return float(text[j:k]), e + 1
        except ValueError:
            return None, e + 1                           # `:1.2.3)`: no number, the whole of it is text
    return None


def _split_break(run):
    """A run of plain text -> its parts around every `BREAK` that stands as a word; the whitespace around it goes with it."""
    parts, cur, i = [], "", 0
    while i < len(run):
        if run.startswith("BREAK", i):
            before = run[i - 1] if i else " "
            after = run[i + 5] if i + 5 < len(run) else " "
            if not (before.isalnum() or before == "_") and not (after.isalnum() or after == "_"):
                parts.append(cur.rstrip())
                i += 5
                while i < len(run) and run[i].isspace():
                    i += 1
                cur = ""
                continue
        cur += run[i]
        i += 1
    parts.append(cur)
    return parts


def parse(text):
    segs, rounds, squares = [], [], []          # segs: [text, weight] in order; the stacks hold where a bracket's range starts

    def scale(start, f):
        for s in segs[start:]:
            if tuple(s) != BREAK:
                s[1] *= f

    def plain(run):
        for n, part in enumerate(_split_break(run)):
            if n:
                segs.append(list(BREAK))
            segs.append([part, 1.0])

    i, run = 0, ""

    def flush():
        nonlocal run
        if run:
            plain(run)
            run = ""

    while i < len(text):
        ch = text[i]
        if ch == "\\":
            flush()
            if i + 1 < len(text) and text[i + 1] in "()[]\\":
                segs.append([text[i + 1], 1.0])
                i += 2
            else:
                segs.append(["", 1.0])
                i += 1
        elif ch == "(":
            flush()
            rounds.append(len(segs))
            i += 1
        elif ch == "[":
            flush()
            squares.append(len(segs))
            i += 1
        elif ch == ":":
            flush()
            hit = _number_close(text, i)
            if hit is not None and hit[0] is not None and rounds:
                scale(rounds.pop(), hit[0])
                i = hit[1]
            elif hit is not None:
                plain(text[i:hit[1]])
                i = hit[1]
            else:
                plain(":")
                i += 1
        elif ch == ")":
            flush()
            if rounds:
                scale(rounds.pop(), ROUND)
            else:
                plain(")")
            i += 1
        elif ch == "]":
            flush()
            if squares:
                scale(squares.pop(), SQUARE)
            else:
                plain("]")
            i += 1
        else:
            run += ch
            i += 1
    flush()
    for start in rounds:
        scale(start, ROUND)
    for start in squares:
        scale(start, SQUARE)
    if not segs:
        segs = [["", 1.0]]
    out = []
    for s, w in segs:
        if out and out[-1][1] == w and (s, w) != BREAK and tuple(out[-1]) != BREAK:
            out[-1][0] += s
        else:
            out.append([s, w])
    return [(s, w) for s, w in out]


def chunks(segments, words_to_ids, bos, eos, pad, comma):
    """-> (ids (n, 77) int64, weights (n, 77) fp32, token count).  The stream between two BREAKs is cut recursively: 75 or fewer
    tokens are one chunk; else, where one of tokens 55..74 is a comma and token 75 is none, the cut is behind the last such
    comma, else behind token 74."""
    spans, cur = [], []
    for s, w in segments:
        if (s, w) == BREAK:
            spans.append(cur)
            cur = []
        else:
            cur += [(t, w) for t in words_to_ids(s)]
    spans.append(cur)
    if len(spans) > 1 and not spans[-1]:
        spans.pop()                                     # a BREAK at the very end opens no chunk

    def cut(stream):
        if len(stream) <= CHUNK:
            return [stream]
        at = CHUNK
        if stream[CHUNK][0] != comma:
            back = [p for p in range(CHUNK - BACKTRACK, CHUNK) if stream[p][0] == comma]
            if back:
                at = back[-1] + 1
        return [stream[:at]] + cut(stream[at:])

    rows = [c for span in spans for c in cut(span)]
    ids = torch.full((len(rows), SEQ), pad, dtype=torch.int64)
    wts = torch.ones((len(rows), SEQ), dtype=torch.float32)
    for r, row in enumerate(rows):
        ids[r, 0], ids[r, 1 + len(row)] = bos, eos
        for p, (t, w) in enumerate(row):
            ids[r, 1 + p], wts[r, 1 + p] = t, w
    return ids, wts, sum(len(r) for r in rows)


def weight(z, w):
    """csrc/prompt.hip on the CPU.  z fp16 (n_seq, n_tok, D), w fp32 (n_seq, n_tok) -> fp16 like z."""
    y = (z.float() * w.float()[:, :, None]).half()
    m0 = z.double().sum(dim=(1, 2))
    m1 = y.double().sum(dim=(1, 2))
    r = (m0 / m1).float()                                # the quotient in fp64, rounded to fp32 once
    return (y.float() * r[:, None, None]).half()


def sums_are_exact(z, w):
    """The bound the bit-for-bit claim rests on: |z| <= 64 and |y| <= 64 x |w| <= 128 keep every partial sum of at most 77 x 1024
    fp16 values (multiples of 2^-24, below 2^7 x 2^17 = 2^24 in magnitude) inside 48 bits: exact in fp64 in any order."""
    y = (z.float() * w.float()[:, :, None]).half()
    fin = torch.isfinite(z.float()).all(dim=(1, 2)) & torch.isfinite(y.float()).all(dim=(1, 2))
    ok = (z.float().abs().amax(dim=(1, 2)) <= 64) & (y.float().abs().amax(dim=(1, 2)) <= 128) & (z[0].numel() <= 77 * 1024)
    return fin & ok
