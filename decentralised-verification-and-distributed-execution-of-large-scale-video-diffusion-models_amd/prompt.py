"""Weighted and long prompts: the AUTOMATIC1111 web UI's emphasis syntax and 75-token chunks (`prompt_parser.parse_prompt_attention`
and `sd_hijack_clip`'s chunking, restated here and not pinned against an external implementation: the web UI is not installed;
diffusers has the same behaviour as `lpw_stable_diffusion`, and `compel`).  `DiffuserConfig(prompt_syntax="a1111")` /
`--prompt_syntax a1111`; "plain", the default, is the job as it always was.

  * `parse_attention(text)`: `(x)` multiplies x's weight by 1.1, `[x]` divides it by 1.1, `(x:1.5)` multiplies it by 1.5; `\\(`,
    `\\)`, `\\[`, `\\]` and `\\\\` are literals; openers left open are closed at the end of the text; neighbours of equal weight
    are merged; `BREAK` between whitespace ends the current chunk.
  * `chunk_tokens(segments, tokenizer)`: every segment is tokenised on its own, without special tokens and without truncation, and
    the stream is laid into chunks of 75 tokens between BOS and EOS, each token with its segment's weight.  A chunk that fills is
    split behind the last comma among its final 20 tokens where there is one (the tokens behind it open the next chunk), else at
    75.  Nothing is ever dropped: more than `max_chunks` chunks is a `ValueError` that names the token count.
  * `encode_texts(pipe, texts, "a1111", device)`: all texts padded to the job's largest chunk count k with empty chunks, the
    n_texts k sequences through the CLIP text encoder as ONE batch, `ops.prompt_weight` (csrc/prompt.hip: the weights, mean
    restored per sequence) on the sequences that carry a weight, and each text's chunks side by side: fp16 (n_texts, 77 k, D).
    The UNet takes the longer text as it is (vdx/unet3d.py `text_pad_of`).

A text of at most 75 tokens without emphasis is one chunk of weights 1.0 with exactly the ids of the plain tokeniser call, no
kernel runs, and the job equals "plain" bit for bit.
"""
from __future__ import annotations

import re
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

SYNTAXES = ("plain", "a1111")
CHUNK = 75                      # tokens of a chunk between BOS and EOS
SEQ = CHUNK + 2                 # positions of a chunk: the text encoder's sequence length
MAX_CHUNKS = 4                  # 308 positions: what the UNet takes (unet3d.MAX_TEXT_LEN)
COMMA_BACKTRACK = 20            # A1111's comma_padding_backtrack
ROUND, SQUARE = 1.1, 1 / 1.1
BREAK = ("BREAK", -1.0)         # the marker `parse_attention` puts where a chunk ends

_TOKEN = re.compile(r"\\[()\[\]\\]|\\|[()\[\]]|:\s*([+-]?[.\d]+)\s*\)|[^\\()\[\]:]+|:")
_BREAK = re.compile(r"\s*\bBREAK\b\s*")


def parse_attention(text: str) -> List[Tuple[str, float]]:
    """`text` -> [(segment, weight), ...]; a `BREAK` is the pair `BREAK` = ("BREAK", -1.0).  The empty text is [("", 1.0)]."""
    if not isinstance(text, str):
        raise ValueError(f"parse_attention: the text must be a string, got {text!r}")
    out: List[list] = []
    open_round: List[int] = []          # index into `out` where each open bracket's range starts
    open_square: List[int] = []

    def scale(start: int, factor: float) -> None:
        for seg in out[start:]:
            if tuple(seg) != BREAK:
                seg[1] *= factor

    for m in _TOKEN.finditer(text):
        tok, number = m.group(0), m.group(1)
        if tok[0] == "\\":                              # an escaped bracket or backslash is itself; a lone backslash is dropped
            out.append([tok[1:], 1.0])
        elif tok == "(":
            open_round.append(len(out))
        elif tok == "[":
            open_square.append(len(out))
        elif number is not None and open_round and _is_number(number):
            scale(open_round.pop(), float(number))
        elif tok == ")" and open_round:
            scale(open_round.pop(), ROUND)
        elif tok == "]" and open_square:
            scale(open_square.pop(), SQUARE)
        else:                                           # text (also a closer or a ':1.2)' that closes nothing)
            for i, part in enumerate(_BREAK.split(tok)):
                if i:
                    out.append(list(BREAK))
                out.append([part, 1.0])
    for start in open_round:
        scale(start, ROUND)
    for start in open_square:
        scale(start, SQUARE)
    if not out:
        out = [["", 1.0]]
    merged: List[list] = []
    for seg, wt in out:
        if merged and merged[-1][1] == wt and (seg, wt) != BREAK and tuple(merged[-1]) != BREAK:
            merged[-1][0] += seg
        else:
            merged.append([seg, wt])
    return [(seg, wt) for seg, wt in merged]


def _is_number(s: str) -> bool:
    try:
        float(s)
    except ValueError:
        return False
    return True


def strip_syntax(text: str) -> str:
    """`text` without its emphasis syntax: the segments in order, a `BREAK` as one blank.  What the scores (`--clip_json`,
    `--mdvqs_json`) are taken against: CLIP ViT-B/32 knows no weights and truncates at its own 77 tokens."""
    return "".join(" " if (seg, wt) == BREAK else seg for seg, wt in parse_attention(text)).strip()


def _special_ids(tokenizer) -> Tuple[int, int, int]:
    """(BOS, EOS, pad) of `tokenizer`; pad is its pad id where it has one (SD-2.x pads with `!`, id 0), else EOS."""
    bos, eos = int(tokenizer.bos_token_id), int(tokenizer.eos_token_id)
    pad = getattr(tokenizer, "pad_token_id", None)
    return bos, eos, eos if pad is None else int(pad)


def _ids(tokenizer, text: str) -> List[int]:
    ids = tokenizer(text, add_special_tokens=False, truncation=False, padding=False, return_tensors=None).input_ids
    return [int(i) for i in ids]


def chunk_tokens(segments: Sequence[Tuple[str, float]], tokenizer, max_chunks: int = MAX_CHUNKS):
    """`parse_attention`'s segments -> (ids int64 (n_chunks, 77), weights fp32 (n_chunks, 77)), n_chunks >= 1.  BOS, EOS and pad
    positions have weight 1.0.  `ValueError` for more than `max_chunks` chunks; the message names the token count."""
    return _chunk(segments, tokenizer, max_chunks)[:2]


def _chunk(segments, tokenizer, max_chunks):
    """`chunk_tokens` and the number of tokens laid out."""
    bos, eos, pad = _special_ids(tokenizer)
    comma = _ids(tokenizer, ",")
    comma = comma[0] if len(comma) == 1 else None
    chunks: List[Tuple[List[int], List[float]]] = []
    ids: List[int] = []
    wts: List[float] = []
    last_comma = -1                                      # position in `ids` of the current chunk's last comma
    n_tokens = 0

    def close():
        nonlocal ids, wts, last_comma
        chunks.append((ids, wts))
        ids, wts, last_comma = [], [], -1

    for seg, wt in segments:
        if (seg, wt) == BREAK:
            close()                                      # pads out the current chunk, an empty one included (as the web UI does)
            continue
        for tok in _ids(tokenizer, seg):
            n_tokens += 1
            if len(ids) == CHUNK:
                if tok != comma and last_comma >= 0 and CHUNK - last_comma <= COMMA_BACKTRACK:
                    cut = last_comma + 1                 # behind the comma: what follows it opens the next chunk
                    tail_ids, tail_wts = ids[cut:], wts[cut:]
                    ids, wts = ids[:cut], wts[:cut]
                    close()
                    ids, wts = tail_ids, tail_wts
                else:
                    close()
            if tok == comma:
                last_comma = len(ids)
            ids.append(tok)
            wts.append(float(wt))
    if ids or not chunks:
        close()
    if len(chunks) > max_chunks:
        raise ValueError(f"prompt: {n_tokens} tokens make {len(chunks)} chunks of {CHUNK}, at most {max_chunks} ({max_chunks * SEQ} positions) "
                         "are taken; nothing is dropped silently: shorten the text")
    out_ids = torch.full((len(chunks), SEQ), pad, dtype=torch.int64)
    out_w = torch.ones((len(chunks), SEQ), dtype=torch.float32)
    for c, (ci, cw) in enumerate(chunks):
        out_ids[c, 0] = bos
        out_ids[c, 1 + len(ci)] = eos
        if ci:
            out_ids[c, 1:1 + len(ci)] = torch.tensor(ci, dtype=torch.int64)
            out_w[c, 1:1 + len(cw)] = torch.tensor(cw, dtype=torch.float32)
    return out_ids, out_w, n_tokens


class PromptPlan(NamedTuple):
    """The job's texts, chunked: ids int64 (n_texts, k, 77), weights fp32 (n_texts, k, 77), the tokens of each text (without
    specials and padding), all on the host."""
    ids: torch.Tensor
    weights: torch.Tensor
    tokens: Tuple[int, ...]

    @property
    def chunks(self) -> int:
        return int(self.ids.shape[1])

    @property
    def weighted(self) -> bool:
        return bool((self.weights != 1.0).any())

    def record(self, syntax: str = "a1111") -> dict:
        return {"syntax": syntax, "chunks": self.chunks, "tokens": list(self.tokens), "weighted": self.weighted}


def plan_texts(texts: Sequence[str], tokenizer, max_chunks: int = MAX_CHUNKS) -> PromptPlan:
    """Every text parsed and chunked, all padded to the largest chunk count k with empty chunks (BOS, EOS, padding)."""
    if not texts:
        raise ValueError("prompt: no texts")
    per = [_chunk(parse_attention(t), tokenizer, max_chunks) for t in texts]
    k = max(i.shape[0] for i, _, _ in per)
    empty_ids, empty_w = chunk_tokens([("", 1.0)], tokenizer)
    ids = torch.stack([torch.cat([i] + [empty_ids] * (k - i.shape[0])) for i, _, _ in per])
    wts = torch.stack([torch.cat([w] + [empty_w] * (k - w.shape[0])) for _, w, _ in per])
    return PromptPlan(ids, wts, tuple(n for _, _, n in per))


def check_texts(texts: Sequence[str], tokenizer, max_chunks: int = MAX_CHUNKS) -> None:
    """`ValueError` for a text that is no string or that makes more than `max_chunks` chunks; nothing is encoded."""
    for t in texts:
        chunk_tokens(parse_attention(t), tokenizer, max_chunks)


def encode_texts(pipe, texts: Sequence[str], syntax: str, device, return_plan: bool = False):
    """The texts' UNet conditioning under `syntax` = "a1111" -> fp16 (n_texts, 77 k, D) on `device`, k the job's largest chunk
    count (with `return_plan`: and the `PromptPlan`).  One text-encoder call over the n_texts k sequences; the sequences that
    carry a weight other than 1.0 go through `ops.prompt_weight`, the others keep the encoder's bits."""
    from . import ops
    if syntax != "a1111":
        raise ValueError(f"encode_texts: syntax {syntax!r}: \"a1111\" is what it encodes (\"plain\" is the tokeniser call itself)")
    plan = plan_texts(list(texts), pipe.tokenizer)
    n, k = plan.ids.shape[:2]
    device = torch.device(device)
    with torch.no_grad():
        z = pipe.text_encoder(plan.ids.reshape(n * k, SEQ).to(device))[0]
    z = z.to(torch.float16).contiguous()
    if plan.weighted:
        z = ops.prompt_weight(z, plan.weights.reshape(n * k, SEQ))
    emb = z.reshape(n, k * SEQ, z.shape[-1])
    return (emb, plan) if return_plan else emb
