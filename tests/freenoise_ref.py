"""FreeNoise restated in float64 torch (no test of its own): the window-fused temporal attention of include/vdx.h
`vdx_temporal_attn_windows_f16` as a loop over windows, and literal restatements of `freenoise.window_starts` and
`freenoise.reschedule_index`."""
import math

import torch


def window_starts(F, L, S):
    return [min(i * S, F - L) for i in range(math.ceil((F - L) / S) + 1)]


def window_weights(F, L, S, weighting):
    raw = [float(min(j + 1, L - j)) if weighting == "pyramid" else 1.0 for j in range(L)]
    total = [0.0] * F
    for s in window_starts(F, L, S):
        for j in range(L):
            total[s + j] += raw[j]
    return torch.tensor([[raw[j] / total[s + j] for j in range(L)] for s in window_starts(F, L, S)], dtype=torch.float64).float()


def windowed_attention(q, k, v, scale, L, S, wn):
    """q, k, v (..., F, d) -> (..., F, d) float64: softmax attention inside each window, summed with the fp32 table `wn`."""
    q, k, v = q.double(), k.double(), v.double()
    out = torch.zeros_like(q)
    for i, s in enumerate(window_starts(q.shape[-2], L, S)):
        p = torch.softmax(scale * q[..., s:s + L, :] @ k[..., s:s + L, :].transpose(-1, -2), dim=-1)
        out[..., s:s + L, :] += wn[i].double()[:, None] * (p @ v[..., s:s + L, :])
    return out


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) % 2 ** 64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    return state, z ^ (z >> 31)


def reschedule_index(T, L, S, seed):
    """The frames as lists of original indices, shuffled block by block in place, as diffusers' `shuffle_context` moves latents."""
    frames = list(range(T))
    for b, i in enumerate(range(L, T, S)):
        state, perm = (seed + (b + 1) * 0xD1B54A32D192ED03) % 2 ** 64, list(range(S))
        for j in range(S - 1, 0, -1):
            state, z = splitmix64(state)
            perm[j], perm[z % (j + 1)] = perm[z % (j + 1)], perm[j]
        source = frames[i - L:i - L + S]
        for k in range(min(S, T - i)):
            frames[i + k] = source[perm[k]]
    return frames
