"""Farneback dense optical flow on libvdx_hip.so, batched over the frame pairs of a clip, and the two public numbers built
on it:

    InferNet/template/validator/scoring.py:311-339             MD-VQS temporal consistency: mean over pairs of mean |flow|
    Distribution/strategies/fsdp_chunked_coherent.py:236-246   flow_err: mean |remap(prev, flow) - next| at chunk boundaries

The algorithm is `vdx.compat.cv2_shim.calcOpticalFlowFarneback` (cv2_shim.py:99-182) stage by stage on the device (csrc/flow.hip;
planes in memory are fp32, the arithmetic inside the polynomial expansion and the displacement update is fp64, because the
2 x 2 systems of straight edges on flat backgrounds are nearly singular; the rest is fp32): grey image, Gaussian pyramid, polynomial expansion, `iterations` displacement updates per level with a
15 x 15 box window, bilinear upsampling between levels.  What is pinned: this path against the project's own shim
(tests/test_flow_gpu.py, profiles/flow_parity.txt).  What is not: the shim against OpenCV (no `cv2` was available where it
was written), so the numbers' agreement with the reference's own remains unpinned as before.

Only the parameters both callers use are provided: pyr_scale 0.5, winsize 15, poly_n 5, poly_sigma 1.2, flags 0
(scoring.py:325-327, fsdp_chunked_coherent.py:240); `levels` and `iterations` are free.  Anything else, frames that are not
a uint8 RGB clip (vdx/frames.py), or min(H, W) < 16 raise `VdxError` before any launch.

Every frame's pyramid and polynomial expansion are computed once and serve both pairs the frame belongs to; each update
iteration is one launch over all pairs.  All sums run in a fixed order without floating-point atomics, so a pair's flow has
the same bits on every run and whatever else the batch holds.  Frames already on the device stay there: the metric
functions bring a few scalars per pair to the host, nothing else.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import frames as _frames
from ._lib import VdxError

PYR_SCALE, LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA, FLAGS = 0.5, 3, 15, 3, 5, 1.2, 0     # the callers' arguments
MIN_SIDE = 16


# ---- host side: plans and tables ---------------------------------------------------------------------------------------
def level_plan(H: int, W: int, levels: int) -> List[Tuple[int, int, float, int]]:
    """The pyramid of an H x W image, finest level first: [(h, w, sigma, radius)] (cv2_shim.py:161-170).  The level count
    drops while the coarsest level's shorter side would fall below 16; level k has scale 0.5^k, sides
    max(round(side * scale), 1) with Python's round (half to even: 97 -> 48, 131 -> 66) and, for k > 0, the full-size image
    blurred with sigma = (1 / scale - 1) / 2 over radius int(4 sigma + 0.5) before it is resized."""
    H, W, levels = int(H), int(W), max(int(levels), 1)
    if min(H, W) < MIN_SIDE:
        raise VdxError(f"flow: frames of {H}x{W} are too small (min(H, W) >= {MIN_SIDE})")
    while levels > 1 and min(H, W) * PYR_SCALE ** (levels - 1) < 16:
        levels -= 1
    plan = []
    for k in range(levels):
        scale = PYR_SCALE ** k
        sigma = (1.0 / scale - 1.0) * 0.5
        plan.append((max(int(round(H * scale)), 1), max(int(round(W * scale)), 1), sigma, int(4.0 * sigma + 0.5) if k else 0))
    return plan


def gaussian_taps(sigma: float, radius: int) -> np.ndarray:
    """scipy.ndimage.gaussian_filter1d's normalised taps (truncate 4.0: radius = int(4 sigma + 0.5)), float64 [2 radius + 1]."""
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-0.5 / (sigma * sigma) * x * x)
    return g / g.sum()


def poly_tables(n: int = POLY_N, sigma: float = POLY_SIGMA) -> Tuple[np.ndarray, np.ndarray]:
    """`_poly_exp`'s constants in float64 (cv2_shim.py:102-117): taps (3, 2n+1) = g, g x, g x^2 with g the normalised Gaussian
    applicability, and rows 1..5 of inv(G) (5, 6) — G the Gram matrix of (1, x, y, x^2, y^2, xy) under g(x) g(y) — that turn the
    six moments into bx, by, axx, ayy, axy."""
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2 * sigma * sigma))
    g /= g.sum()
    X, Y = np.meshgrid(x, x)
    basis = np.stack([np.ones_like(X), X, Y, X * X, Y * Y, X * Y], 0).reshape(6, -1)
    G = (basis * np.outer(g, g).reshape(1, -1)) @ basis.T
    return np.stack([g, g * x, g * x * x]), np.linalg.inv(G)[1:]


def check_params(pyr_scale=PYR_SCALE, levels=LEVELS, winsize=WINSIZE, iterations=ITERATIONS, poly_n=POLY_N,
                 poly_sigma=POLY_SIGMA, flags=FLAGS) -> Tuple[int, int]:
    """-> (levels, iterations) as the shim clamps them (at least 1 each); `VdxError` for any parameter the kernels do not provide."""
    if (pyr_scale, winsize, poly_n, poly_sigma, flags) != (PYR_SCALE, WINSIZE, POLY_N, POLY_SIGMA, FLAGS):
        raise VdxError(f"flow: only pyr_scale {PYR_SCALE}, winsize {WINSIZE}, poly_n {POLY_N}, poly_sigma {POLY_SIGMA}, flags {FLAGS} "
                       f"are provided on the GPU, got {(pyr_scale, winsize, poly_n, poly_sigma, flags)}")
    for name, v in (("levels", levels), ("iterations", iterations)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise VdxError(f"flow: {name} must be an integer, got {v!r}")
    return max(int(levels), 1), max(int(iterations), 1)


# ---- the flow ------------------------------------------------------------------------------------------------------------
_TAPS: dict = {}        # (device, radius) -> fp32 taps on the device


def _taps_on(device, sigma: float, radius: int) -> torch.Tensor:
    t = _TAPS.get((str(device), radius))
    if t is None:
        t = _TAPS[(str(device), radius)] = torch.from_numpy(gaussian_taps(sigma, radius).astype(np.float32)).to(device)
    return t


def _flows(u8: torch.Tensor, levels: int, iterations: int, step: int, bgr: bool) -> torch.Tensor:
    """Flows of the pairs (p*step, p*step + 1) of uint8 frames on the GPU (`ops.check_u8_frames`) -> fp32 (P, H, W, 2)."""
    from . import ops
    F, H, W = (int(v) for v in u8.shape[:3])
    P = (F - 2) // step + 1
    plan = level_plan(H, W, levels)
    taps, inv_g = poly_tables()
    grey = ops.flow_grey(u8, bgr=bgr)
    flow = None
    for k in range(len(plan) - 1, -1, -1):
        h, w, sigma, radius = plan[k]
        if k > 0:       # gaussian_filter runs axis 0 first, then axis 1
            t = _taps_on(u8.device, sigma, radius)
            img = ops.flow_resize(ops.flow_corr1d(ops.flow_corr1d(grey, t, 0), t, 1), h, w)
        else:
            img = grey
        R = ops.flow_polyexp(img, taps, inv_g)                          # once per frame: both of its pairs read it
        del img
        if flow is None:
            flow = torch.zeros((P, h, w, 2), dtype=torch.float32, device=u8.device)
        else:
            flow = ops.flow_resize(flow, h, w, mul=1.0 / PYR_SCALE)
        other = torch.empty_like(flow)
        for _ in range(iterations):
            flow, other = ops.flow_update(R, flow, step=step, out=other), flow
        del R, other
    return flow


def farneback_flows(frames, levels: int = LEVELS, iterations: int = ITERATIONS, *, pyr_scale: float = PYR_SCALE,
                    winsize: int = WINSIZE, poly_n: int = POLY_N, poly_sigma: float = POLY_SIGMA, flags: int = FLAGS,
                    device=None, bgr: bool = False) -> torch.Tensor:
    """`calcOpticalFlowFarneback(grey(frame i), grey(frame i+1), None, 0.5, levels, 15, iterations, 5, 1.2, 0)` for every
    consecutive pair of uint8 RGB `frames` (F, H, W, 3) -> fp32 (F-1, H, W, 2) on the GPU.  Grey is COLOR_RGB2GRAY, or with
    `bgr` COLOR_BGR2GRAY of the same bytes (what vdx/metrics.py does).  Frames on the GPU are used where they are."""
    levels, iterations = check_params(pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)
    F, H, W = _frames.check(frames, "flow")
    if F < 2:
        raise VdxError(f"flow: at least two frames are needed, got {F}")
    level_plan(H, W, levels)                                            # the size check, before anything is uploaded
    u8 = _frames.on_device(frames, _frames.device_for(frames, device))
    return _flows(u8, levels, iterations, 1, bgr)


def temporal_consistency(frames, device=None) -> float:
    """MD-VQS TC (scoring.py:311-339; vdx/mdvqs.py `compute_temporal_consistency`) on the GPU: the mean over consecutive pairs
    of mean |Farneback flow| of the COLOR_RGB2GRAY frames; fewer than two frames -> 0.0 (:336-337)."""
    from . import ops
    levels, iterations = check_params()
    F, H, W = _frames.check(frames, "flow")
    if F < 2:
        return 0.0
    level_plan(H, W, levels)
    flows = _flows(_frames.on_device(frames, _frames.device_for(frames, device)), levels, iterations, 1, False)
    sums = ops.flow_abs_sum(flows).cpu().numpy()                        # fp32 [F-1]
    scores = sums / np.float32(H * W * 2)                               # np.mean(np.abs(flow)) of a float32 array
    return float(np.mean(scores))


def boundary_pairs(n_frames: int, ranges: Sequence[Tuple[int, int]]) -> List[int]:
    """The chunk ends e whose frames (e-1, e) `flow_warp_error` compares (vdx/metrics.py:53-57): every chunk end but the last
    chunk's in start order, with 0 < e < n_frames."""
    ends = [e for (_s, e) in sorted(ranges, key=lambda r: r[0])[:-1]]
    return [e for e in ends if 0 < e < n_frames]


def warp_pairs(frames, ends: Sequence[int], device=None, want_warped: bool = False):
    """For every e in `ends`: the flow frame e-1 -> frame e (grey as vdx/metrics.py:59), frame e-1 warped by it and the sum of
    |warp - frame e| over all bytes -> (flows fp32 (P, H, W, 2), sums int64 [P], warped uint8 (P, H, W, 3) or None), on the GPU."""
    from . import ops
    levels, iterations = check_params()
    F, H, W = _frames.check(frames, "flow")
    level_plan(H, W, levels)
    index = [i for e in ends for i in (e - 1, e)]
    if not index or min(index) < 0 or max(index) >= F:
        raise VdxError(f"flow: boundaries {list(ends)} do not lie inside {F} frames")
    u8 = _frames.on_device(frames, _frames.device_for(frames, device), index)
    flows = _flows(u8, levels, iterations, 2, True)
    sums, warped = ops.flow_remap_absdiff(u8, flows, step=2, want_warped=want_warped)
    return flows, sums, warped


def flow_warp_error(frames, ranges: Sequence[Tuple[int, int]], device=None) -> Optional[float]:
    """The result row's `flow_err` (fsdp_chunked_coherent.py:229-246; vdx/metrics.py `flow_warp_error`, same boundaries, same
    channel handling) on the GPU; None for a single frame or when there is no boundary."""
    F, H, W = _frames.check(frames, "flow")
    if F <= 1:
        return None
    ends = boundary_pairs(F, ranges)
    if not ends:
        return None
    _flows_, sums, _ = warp_pairs(frames, ends, device=device)
    diffs = sums.cpu().numpy().astype(np.float64) / float(H * W * 3)   # the exact byte sums over their number
    return float(np.mean(diffs))
