"""FreeLong (Lu et al., "FreeLong: Training-Free Long Video Generation with SpectralBlend Temporal Attention", NeurIPS 2024,
restated and unpinned): the host side.  No reference counterpart.  The UNet runs once over a clip longer than it was trained
on; every temporal attention is taken twice from one set of scores, globally over all F frames (consistent, but its high
temporal frequencies are damaged at an unseen length) and locally inside a band of `window` frames around each frame (the
trained statistics, no long-range view), and the result keeps the low temporal frequencies of the global one and the high
ones of the local one (`ops.temporal_attn_blend`, csrc/freelong.hip).  The low-pass filter along the frame axis is a fixed
real circulant F x F matrix, built here; `UNet3DConditionModel.enable_free_long` (vdx/unet3d.py) is the switch,
`--free_long WINDOW D_T` the job's.  tests/freelong_ref.py states the definition.

Deliberate restriction, stated: the paper's filter is three-dimensional; only its temporal factor is built (spatial distance
0 in vdx/freeinit.py's filters).  That factor carries the method's point, global attention fails along time, and it keeps the
blend inside one (pixel, head)."""
from __future__ import annotations

import numpy as np
import torch

from .freeinit import METHODS, check_filter_args

MAX_FRAMES = 128                          # the kernel's domain: at most four 32-key score tiles per wave (csrc/freelong.hip)


def radius_of(window: int) -> int:
    """The band |t - j| <= radius that stands for a local window of `window` frames centred on frame t."""
    return window // 2


def check_params(window=24, d_t=0.25, method="gaussian", order=4) -> dict:
    """The parameters as the record {"window", "d_t", "method", "order"}; `ValueError` for what the kernel or the filter does
    not take: an integer 2 <= window <= 128 (so the radius is at least 1), a finite d_t >= 0, a method out of
    `freeinit.METHODS`, a positive integer order."""
    if isinstance(window, bool) or not isinstance(window, int):
        raise ValueError(f"free_long: window must be an integer, got {window!r}")
    if not 2 <= window <= MAX_FRAMES:
        raise ValueError(f"free_long: window {window} outside [2, {MAX_FRAMES}]")
    try:
        check_filter_args(method, 1.0, d_t, order)
    except ValueError as err:
        raise ValueError(str(err).replace("free_init:", "free_long:")) from None
    return {"window": window, "d_t": float(d_t), "method": method, "order": order}


def temporal_gain(F: int, method: str = "gaussian", d_t: float = 0.25, order: int = 4) -> np.ndarray:
    """g[k], float64 [F], k the un-shifted DFT index: the temporal factor of `freeinit.lowpass_filter` at spatial distance 0.
    That filter's coordinate for the fftshift-ed index i is 2 i / F - 1, normalised by d_t; the un-shifted index k sits at
    i = (k + F // 2) mod F.  All zeros when d_t == 0."""
    check_filter_args(method, 1.0, d_t, order)
    if d_t == 0:
        return np.zeros(F, dtype=np.float64)
    i = (np.arange(F) + F // 2) % F
    x2 = ((2.0 * i.astype(np.float64) / F - 1.0) / float(d_t)) ** 2
    if method == "butterworth":
        return 1.0 / (1.0 + x2 ** order)
    if method == "gaussian":
        return np.exp(-x2 / 2.0)
    return (x2 <= 1.0).astype(np.float64)


def blend_matrix(F: int, method: str = "gaussian", d_t: float = 0.25, order: int = 4) -> torch.Tensor:
    """Lp = Re(IDFT_F diag(g) DFT_F), float64 (F, F) on the host: Lp[t][s] = (1 / F) sum_k g[k] cos(2 pi k (t - s) / F).  Real,
    symmetric and circulant, its rows sum to g[0]; 0 when d_t == 0, the identity for a filter that passes everything."""
    if isinstance(F, bool) or not isinstance(F, int) or not 2 <= F <= MAX_FRAMES:
        raise ValueError(f"free_long: F={F!r} frames outside [2, {MAX_FRAMES}]")
    g = temporal_gain(F, method, d_t, order)
    k = np.arange(F, dtype=np.float64)
    first = (g[None, :] * np.cos(2.0 * np.pi * k[None, :] * k[:, None] / F)).sum(axis=1) / F       # column s = 0: Lp[t][0]
    first = 0.5 * (first + first[(-np.arange(F)) % F])             # cos is even: Lp[t][0] = Lp[F - t][0], here to the last bit
    idx = (np.arange(F)[:, None] - np.arange(F)[None, :]) % F
    return torch.from_numpy(first[idx])
