"""The intake of a clip of uint8 RGB frames, for everything that scores, compares, interpolates or writes one ("Frame intake").

A clip arrives as a tensor (F, H, W, 3), on the GPU or not, as a numpy array of that shape, or as a sequence of (H, W, 3)
arrays and / or tensors of one size (what the VAE decode leaves).  `check` says whether it is one, `device_for` where it is to
be worked on, `on_device` gets it there; `is_packed` is the pixel layout the u8 kernels read (`ops.check_u8_frames`).  What a
clip of no frames means is the caller's business.  Nothing else of the package is imported here, so `ops` may.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import VdxError


def _is_u8(x) -> bool:
    return x.dtype == (torch.uint8 if isinstance(x, torch.Tensor) else np.uint8)


def check(frames, who: str) -> Tuple[int, int, int]:
    """-> (F, H, W) of a clip in one of the three forms (F may be 0: (0, 0, 0) for an empty sequence); `VdxError` under the
    caller's name `who` otherwise.  Nothing is copied."""
    if isinstance(frames, (torch.Tensor, np.ndarray)):
        if not _is_u8(frames) or frames.ndim != 4 or frames.shape[3] != 3:
            raise VdxError(f"{who}: expected uint8 RGB frames (F, H, W, 3), got {frames.dtype} {tuple(frames.shape)}")
        return tuple(int(v) for v in frames.shape[:3])
    fr = [f if isinstance(f, torch.Tensor) else np.asarray(f) for f in frames]
    for f in fr:
        if not _is_u8(f) or f.ndim != 3 or f.shape[2] != 3 or f.shape != fr[0].shape:
            raise VdxError(f"{who}: expected uint8 RGB frames (H, W, 3) of one size, got {f.dtype} {tuple(f.shape)}")
    return (len(fr),) + (tuple(int(v) for v in fr[0].shape[:2]) if fr else (0, 0))


def is_packed(t: torch.Tensor) -> bool:
    """Pixels are 3 adjacent bytes and pixels adjacent in a row; rows and frames may be pitched but do not overlap."""
    if t.dim() != 4:
        return False
    H, W = t.shape[1:3]
    return t.stride(3) == 1 and t.stride(2) == 3 and t.stride(1) >= 3 * W and t.stride(0) >= t.stride(1) * H


def device_for(frames, device=None) -> torch.device:
    """The given device; without one the GPU the clip is on, else "cuda"."""
    if device is not None:
        return torch.device(device)
    return frames.device if isinstance(frames, torch.Tensor) and frames.is_cuda else torch.device("cuda")


def _host(a) -> torch.Tensor:
    """Contiguous, and a copy when the array is read-only (torch tensors cannot wrap those)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy())


def on_device(frames, device, index: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Frames `index` (all of them without one) of a clip as one tensor (n, H, W, 3) on `device`.  A whole tensor that is
    there with packed pixels is returned as it is, pitched or not; anything else becomes one packed copy of exactly the frames
    asked for, and no other frame is looked at."""
    index = None if index is None else list(index)
    if index is not None and index == list(range(len(frames))):
        index = None
    if isinstance(frames, torch.Tensor):
        t = (frames if index is None else frames[torch.as_tensor(index, device=frames.device)]).to(device)
        return t if is_packed(t) else t.contiguous()
    if isinstance(frames, np.ndarray):
        return _host(frames if index is None else frames[index]).to(device)
    picked = frames if index is None else [frames[i] for i in index]
    return torch.stack([f if isinstance(f, torch.Tensor) else _host(f) for f in picked]).to(device)
