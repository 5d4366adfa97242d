"""Motion-compensated frame interpolation on libvdx_hip.so: the job's `--interpolate N`.

The reference has no such step (fsdp_chunked_coherent.py:250-253 writes the generated frames as they are, 24 frames at
8 fps); everyone who shows such a clip runs a frame interpolator over it first.  This one is built from what the project
already has on the GPU: the Farneback flows of every consecutive pair in both directions (vdx/flow.py, default parameters;
the backward flows are the forward flows of the frame-reversed clip), and one kernel (csrc/interp.hip) that writes the whole
output clip.  Between frames A and B at t = k / N it samples A and B along Super SloMo's linear combination of the two flows
(Jiang et al. 2018; exact for a uniform translation) and blends the samples with a rational forward-backward consistency
weight; tests/interp_ref.py states the expression in float64 numpy and the tests pin the kernel to it.  What is pinned: the
kernel against that restatement on the same flows, and that the result beats the plain blend on a moving texture.  What is
not, and is not claimed: agreement with any external interpolator.

The output has (F - 1) N + 1 frames; frame i N is input frame i byte for byte.  Frames on the GPU stay there.  With `loop`
(the job's `--loop`) frame 0 is appended first and the last output frame, its copy, is dropped: F N frames, the last of which
leads back into the first.
"""
from __future__ import annotations

import numpy as np
import torch

from . import flow as _flow, frames as _frames
from ._lib import VdxError

MAX_FACTOR = 64


def check_factor(factor) -> int:
    """-> the factor as an int; `VdxError` unless it is an integer (not a bool, not a float) in 1..64."""
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)):
        raise VdxError(f"interpolate: the factor must be an integer, got {factor!r}")
    if not 1 <= int(factor) <= MAX_FACTOR:
        raise VdxError(f"interpolate: the factor must lie in 1..{MAX_FACTOR}, got {factor}")
    return int(factor)


def check_frames(frames):
    """A uint8 RGB clip (vdx/frames.py), F >= 1, min(H, W) >= 16 (the flow's own limit) -> (F, H, W); `VdxError` otherwise."""
    F, H, W = _frames.check(frames, "interpolate")
    if F < 1:
        raise VdxError("interpolate: no frames")
    if min(H, W) < _flow.MIN_SIDE:
        raise VdxError(f"interpolate: frames of {H}x{W} are too small (min(H, W) >= {_flow.MIN_SIDE})")
    return F, H, W


def n_output_frames(n_frames: int, factor: int, loop: bool = False) -> int:
    return int(n_frames) * int(factor) if loop else (int(n_frames) - 1) * int(factor) + 1


def interpolate_frames(frames, factor, device=None, loop: bool = False) -> torch.Tensor:
    """uint8 RGB `frames` (F, H, W, 3) (a tensor, an array or a sequence of (H, W, 3) frames) -> uint8 ((F-1)*factor + 1, H, W, 3)
    on the GPU.  Host frames are uploaded once; frames on the GPU are used where they are.  factor 1 or a single frame: the
    input bytes.  Everything is checked before anything is uploaded or launched.  `loop`: the clip is a loop, so the pair
    (F-1, 0) is interpolated too: frame 0 is appended, the F + 1 frames go through the same kernels, and the last output frame
    (frame 0 again) is dropped -> (F*factor, H, W, 3), whose last frame leads back into its first."""
    factor = check_factor(factor)
    F, H, W = check_frames(frames)
    u8 = _frames.on_device(frames, _frames.device_for(frames, device))
    if factor == 1 or F == 1:
        return u8
    if loop:
        return interpolate_frames(torch.cat([u8, u8[:1]]), factor)[:-1].contiguous()
    from . import ops
    fab = _flow.farneback_flows(u8)
    fba = _flow.farneback_flows(u8.flip(0)).flip(0).contiguous()        # pair i of the reversed clip's flows is frame F-1-i -> F-2-i
    return ops.interp_frames(u8, fab, fba, factor)
