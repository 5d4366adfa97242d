"""Prompt travel: the text changes along the clip's time axis (the host side: the schedule; the arithmetic is csrc/travel.hip).

`DiffuserConfig(prompt_travel=((frame, text), ...))` / `--prompt_at FRAME TEXT` (repeatable) names KEY frames and their prompts.
`cfg.prompt` is the key at frame 0 unless a key names frame 0.  A frame between two keys gets the linear blend of the two keys'
CLIP embeddings, a frame after the last key the last key's; with `loop` the frames after the last key blend towards the first
key instead, which then also sits one clip length later, so the seam pair (T - 1, 0) is as continuous as any other pair.  The
unconditional branch keeps `negative_prompt` on every frame.  What AnimateDiff-Evolved's batch prompt schedule ("prompt travel")
does; no external implementation is installed or pinned, the schedule is restated here and in tests/travel_ref.py.  The
reference has no counterpart: the option is off by default, and without it nothing here runs.

`travel_plan` turns the keys into three arrays of length T: `lo`, `hi` (indices into the keys sorted by frame) and `w`, the
weight of `hi`, `(t - f_lo) / (f_hi - f_lo)` in float64 rounded once to fp32: exactly 0 on a key frame and wherever `lo == hi`.
Every window of every mode builds its UNet text from the plan with `ops.text_travel` (one launch, once per window and job) and
passes the (2, L, 77, 1024) tensor where the job passes (2, 77, 1024) without the option; the UNet takes it per frame through
every cross-attention (vdx/unet3d.py).  Every rank builds its own windows' text from the same keys: no collective.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np
import torch

MAX_KEYS = 64


@dataclass(frozen=True)
class TravelPlan:
    """`frames`: the keys' frames, ascending; `lo`, `hi`: int32 (T,), indices into them; `w`: fp32 (T,), the weight of `hi`."""
    frames: Tuple[int, ...]
    lo: np.ndarray
    hi: np.ndarray
    w: np.ndarray

    @property
    def T(self) -> int:
        return int(self.lo.shape[0])

    def to(self, device):
        """(lo, hi, w) as device tensors, what `ops.text_travel` takes."""
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (self.lo, self.hi, self.w))


def check_keys(keys, T: int) -> Tuple[Tuple[int, str], ...]:
    """`keys` as a tuple of (frame, text) sorted by frame; `ValueError` for an entry that is no (frame, text) pair, a frame that is
    no integer in [0, T), a frame named twice, a text that is no string, no key at all, and more than `MAX_KEYS` keys."""
    if isinstance(keys, (str, bytes)) or not isinstance(keys, Sequence):
        raise ValueError(f"prompt_travel must be a sequence of (frame, text) pairs, got {keys!r}")
    if len(keys) < 1:
        raise ValueError("prompt_travel: no keys")
    if len(keys) > MAX_KEYS:
        raise ValueError(f"prompt_travel: {len(keys)} keys, at most {MAX_KEYS} are taken")
    seen, out = set(), []
    for k in keys:
        if isinstance(k, (str, bytes)) or not isinstance(k, Sequence) or len(k) != 2:
            raise ValueError(f"prompt_travel: an entry must be a (frame, text) pair, got {k!r}")
        f, text = k
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)):
            raise ValueError(f"prompt_travel: a key's frame must be an integer, got {f!r}")
        if not isinstance(text, str):
            raise ValueError(f"prompt_travel: the text of frame {int(f)} must be a string, got {text!r}")
        f = int(f)
        if not 0 <= f < T:
            raise ValueError(f"prompt_travel: frame {f} lies outside the clip's {T} frames")
        if f in seen:
            raise ValueError(f"prompt_travel: frame {f} is named twice")
        seen.add(f)
        out.append((f, text))
    return tuple(sorted(out, key=lambda k: k[0]))


def travel_plan(keys, T: int, loop: bool = False) -> TravelPlan:
    """The plan of `keys` ((frame, text) pairs; only the frames are read) for a clip of T frames.  A frame before the first key
    holds the first key, a frame after the last the last; with `loop` both ranges blend from the last key to the first one a clip
    length later instead.  One key is a constant prompt: `lo == hi`, `w == 0` everywhere."""
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
        raise ValueError(f"travel_plan: T must be an integer >= 1, got {T!r}")
    frames = [f for f, _ in check_keys(keys, int(T))]
    n = len(frames)
    lo, hi, w = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.float32)
    for t in range(T):
        j = int(np.searchsorted(frames, t, side="right")) - 1          # the last key at or before t; -1: none
        if 0 <= j < n - 1:
            a, b, fa, fb = j, j + 1, frames[j], frames[j + 1]
        elif loop and n > 1:                                             # the wrap: from the last key to the first, one clip later
            a, b = n - 1, 0
            fa, fb = (frames[-1], frames[0] + T) if j == n - 1 else (frames[-1] - T, frames[0])
        else:
            a = b = max(j, 0)
            fa = fb = t
        lo[t], hi[t] = a, b
        if a != b and t != fa:
            w[t] = np.float32(np.float64(t - fa) / np.float64(fb - fa))
        if w[t] == 0:                                                    # a key frame: the key itself, a select on the device
            hi[t] = a
    return TravelPlan(tuple(frames), lo, hi, w)


def keys_of(cfg) -> Tuple[Tuple[int, str], ...]:
    """The job's keys: `cfg.prompt_travel`, checked and sorted, with `cfg.prompt` at frame 0 unless a key names frame 0."""
    keys = check_keys(cfg.prompt_travel, cfg.num_frames)
    if keys[0][0] != 0:
        if len(keys) + 1 > MAX_KEYS:
            raise ValueError(f"prompt_travel: {len(keys)} keys and the prompt at frame 0, at most {MAX_KEYS} are taken")
        keys = ((0, cfg.prompt),) + keys
    return keys


def record(keys) -> dict:
    """The option's entry in the result dict and the JSON records."""
    return {"keys": [[f, text] for f, text in keys]}
