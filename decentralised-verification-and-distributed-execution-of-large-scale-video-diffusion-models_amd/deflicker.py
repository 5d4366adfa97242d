"""Motion-compensated temporal filtering on libvdx_hip.so: the job's `--deflicker STRENGTH`.

The reference has no such step (fsdp_chunked_coherent.py:250-253 writes the decoded frames as they are); clips of this kind
shimmer from frame to frame where motion is smooth, and a temporal filter along the motion is what is usually run over them,
beside a frame interpolator.  This one is built from what the project already has on the GPU: the Farneback flows of every
consecutive pair in both directions, taken exactly as vdx/interp.py takes them, and one kernel (csrc/deflicker.hip) per pass.
A frame is blended with its two neighbours warped onto it; a neighbour's weight at a pixel is 1 / (1 + d / sigma^2), d the mean
squared difference to the warped neighbour over the pixel's 3x3 patch, so that a neighbour counts where the motion explains it
and not where it does not (occlusions, wrong flows).  tests/deflicker_ref.py states the definition in float64 numpy and the
tests pin the kernel to it.  What is pinned: the kernel against that restatement on the same flows, and that it lowers the
error on a moving texture whose brightness flickers.  What is not, and is not claimed: agreement with any external deflicker
tool, or any gain on real model output.

Further passes filter the pass before with the same flows, which are computed once, from the input clip.  Frames on the GPU
stay there.  With `loop` (the job's `--loop`) frames F-1 and 0 are neighbours, through the flows of the pair (F-1, 0).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import flow as _flow, frames as _frames
from ._lib import VdxError

MAX_PASSES = 4


def check_params(strength, sigma, passes) -> dict:
    """-> {"strength", "sigma", "passes"}; `VdxError` unless strength is a number in (0, 1], sigma a finite number > 0 (grey
    levels) and passes an integer in 1..4."""
    for name, v in (("strength", strength), ("sigma", sigma)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise VdxError(f"deflicker: {name} must be a number, got {v!r}")
    if not 0 < strength <= 1:
        raise VdxError(f"deflicker: strength must lie in (0, 1], got {strength!r}")
    if not (math.isfinite(sigma) and sigma > 0):
        raise VdxError(f"deflicker: sigma must be finite and > 0, got {sigma!r}")
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= int(passes) <= MAX_PASSES:
        raise VdxError(f"deflicker: passes must be an integer in 1..{MAX_PASSES}, got {passes!r}")
    return {"strength": float(strength), "sigma": float(sigma), "passes": int(passes)}


def check_size(H: int, W: int) -> None:
    """`VdxError` for a frame size the flow refuses (`flow.level_plan`)."""
    _flow.level_plan(H, W, _flow.LEVELS)


def clip_flows(u8: torch.Tensor, loop: bool = False):
    """(fab, fba) of a clip on the GPU as `interp.interpolate_frames` takes them: the backward flows are the forward flows of the
    frame-reversed clip; with `loop` frame 0 is appended first, so entry F-1 of each is the pair (F-1, 0)."""
    if loop:
        u8 = torch.cat([u8, u8[:1]])
    fab = _flow.farneback_flows(u8)
    fba = _flow.farneback_flows(u8.flip(0)).flip(0).contiguous()        # pair i of the reversed clip's flows is frame F-1-i -> F-2-i
    return fab, fba


def run_passes(u8: torch.Tensor, fab, fba, strength: float, sigma: float, passes: int, loop: bool = False) -> torch.Tensor:
    """`passes` launches on given flows; the kernel never writes what it reads, so two buffers take turns."""
    from . import ops
    src, bufs = u8, [None, None]
    for i in range(passes):
        bufs[i % 2] = src = ops.deflicker_frames(src, fab, fba, strength, sigma, loop=loop, out=bufs[i % 2])
    return src


def filter_frames(frames, strength=0.5, sigma=10.0, passes=1, device=None, loop: bool = False) -> torch.Tensor:
    """uint8 RGB `frames` (F, H, W, 3) (a tensor, an array or a sequence of (H, W, 3) frames) -> the filtered clip, uint8
    (F, H, W, 3) on the GPU.  Host frames are uploaded once; frames on the GPU are used where they are.  A single frame: the
    input bytes.  Everything is checked before anything is uploaded or launched."""
    p = check_params(strength, sigma, passes)
    F, H, W = _frames.check(frames, "deflicker")
    if F < 1:
        raise VdxError("deflicker: no frames")
    check_size(H, W)
    u8 = _frames.on_device(frames, _frames.device_for(frames, device))
    if F == 1:
        return u8
    fab, fba = clip_flows(u8, loop)
    return run_passes(u8, fab, fba, p["strength"], p["sigma"], p["passes"], loop)
