"""FreeNoise (Qiu et al., "FreeNoise: Tuning-Free Longer Video Diffusion via Noise Rescheduling", ICLR 2024; diffusers'
`enable_free_noise(context_length, context_stride, weighting_scheme, noise_type)`, restated and unpinned): the host side.  No
reference counterpart.  The UNet runs once over the whole long clip; only its temporal self-attentions are restricted to sliding
windows of the trained length, the windows' outputs averaged per frame (`ops.temporal_attn_windows`, csrc/freenoise.hip), and
the start noise of the frames past the first window is a shuffled repeat of the first window's (`ops.frame_gather` of
`reschedule_index`).  The windows, their weight table and the rescheduling index are built here;
`UNet3DConditionModel.enable_free_noise` (vdx/unet3d.py) is the switch, `--free_noise L S` the job's.
tests/freenoise_ref.py states the definitions.

Deviation from diffusers, stated: its AnimateDiff form runs whole transformer blocks per window and averages their outputs;
here each temporal attention is fused on its own, as the paper states it.  Its `shuffle_context` draws from torch's generator;
here the permutations come from a SplitMix64 stream written out below, so they depend on no library and are the same on every
rank."""
from __future__ import annotations

from typing import List

import torch

WEIGHTINGS = ("pyramid", "flat")
MAX_LENGTH, MAX_FRAMES = 32, 128          # the kernel's domain: one 32 x 32 score tile per window, F <= 128 (csrc/freenoise.hip)


def check_params(L, S, weighting="pyramid") -> dict:
    """The parameters as the record {"context_length", "context_stride", "weighting"}; `ValueError` for what the kernel does not
    take: integers 2 <= L <= 32 and 1 <= S <= L, a weighting out of `WEIGHTINGS`."""
    for what, v in (("context_length", L), ("context_stride", S)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"free_noise: {what} must be an integer, got {v!r}")
    if not 2 <= L <= MAX_LENGTH:
        raise ValueError(f"free_noise: context_length {L} outside [2, {MAX_LENGTH}]")
    if not 1 <= S <= L:
        raise ValueError(f"free_noise: context_stride {S} outside [1, context_length = {L}]")
    if weighting not in WEIGHTINGS:
        raise ValueError(f"free_noise: weighting must be one of {WEIGHTINGS}, got {weighting!r}")
    return {"context_length": L, "context_stride": S, "weighting": weighting}


def window_starts(F: int, L: int, S: int) -> List[int]:
    """The first frames of the n = ceil((F - L) / S) + 1 windows of L frames over F > L frames: stride S, the last window moved
    back to end with the clip (diffusers' `_get_frame_indices`)."""
    if not 1 <= S <= L < F:
        raise ValueError(f"free_noise: windows need 1 <= S <= L < F, got F={F} L={L} S={S}")
    n = -(-(F - L) // S) + 1
    return [min(i * S, F - L) for i in range(n)]


def window_weights(F: int, L: int, S: int, weighting: str = "pyramid") -> torch.Tensor:
    """fp32 [n][L]: entry [i][j] is the share of window i in frame s_i + j.  The raw weight is min(j + 1, L - j) ("pyramid") or 1
    ("flat"); a frame's shares are normalised over the windows that cover it in float64 and rounded to fp32 once, so a frame
    one window covers gets exactly 1.0f (the convention of `codenoise.window_table`)."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"free_noise: weighting must be one of {WEIGHTINGS}, got {weighting!r}")
    starts = window_starts(F, L, S)
    j = torch.arange(L, dtype=torch.float64)
    raw = torch.minimum(j + 1, L - j) if weighting == "pyramid" else torch.ones(L, dtype=torch.float64)
    total = torch.zeros(F, dtype=torch.float64)
    for s in starts:
        total[s:s + L] += raw
    return torch.stack([raw / total[s:s + L] for s in starts]).to(torch.float32)


_M64 = (1 << 64) - 1


def _splitmix64(state: int):
    """Steele, Lea & Flood's SplitMix64: (the next state, its output)."""
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def block_permutation(m: int, seed: int, block: int) -> List[int]:
    """A permutation of range(m): Fisher-Yates from the top (j = m - 1 .. 1, swap j with `draw mod (j + 1)`), the draws from the
    SplitMix64 stream whose state starts at (seed + (block + 1) 0xD1B54A32D192ED03) mod 2^64."""
    state = (seed + (block + 1) * 0xD1B54A32D192ED03) & _M64
    perm = list(range(m))
    for j in range(m - 1, 0, -1):
        state, z = _splitmix64(state)
        k = z % (j + 1)
        perm[j], perm[k] = perm[k], perm[j]
    return perm


def reschedule_index(T: int, L: int, S: int, seed: int = 0) -> List[int]:
    """diffusers' `shuffle_context`, restated: idx[t] = t for t < L; for block b = 0, 1, ... at i = L + b S < T, with
    m = min(S, T - i), the frames [i, i + m) take the first m of `block_permutation(S, seed, b)` applied to the frames
    [i - L, i - L + S).  Blocks are applied in order and later blocks copy earlier copies: the result is the composed map, one
    index into the original noise per frame, every one below L."""
    if not 1 <= S <= L:
        raise ValueError(f"free_noise: rescheduling needs 1 <= S <= L, got L={L} S={S}")
    idx = list(range(min(T, L))) + [0] * max(T - L, 0)
    for b, i in enumerate(range(L, T, S)):
        perm = block_permutation(S, seed, b)
        for k in range(min(S, T - i)):
            idx[i + k] = idx[i - L + perm[k]]
    return idx
