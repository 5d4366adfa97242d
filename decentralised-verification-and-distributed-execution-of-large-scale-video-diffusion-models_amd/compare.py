"""Full-reference comparison of two clips on libvdx_hip.so: how far is one clip from another, frame by frame.

The reference has nothing of the kind: it never holds two clips.  The questions this answers are the project's own: how far
is `--mode hybrid_ctx` from `--mode fsdp` on one seed and is the difference at the chunk seams, what did `--scheduler dpmpp_2m`
cost, what did the Motion-JPEG round trip change, how close is a miner's file to the clip a validator re-generated.

Definition (tests/compare_ref.py states it in float64 numpy; Wang et al. 2004 for SSIM, Wang et al. 2003 for MS-SSIM).  Two
uint8 RGB clips of one shape (F, H, W, 3), everything per frame, every R, G, B plane on its own and the three plane results
averaged (no grey conversion):
  psnr     10 log10(255^2 / (sse / (3 H W))) in float64 on the host from the exact integer sse; inf for sse == 0;
  ssim     11 x 11 Gaussian window, sigma 1.5, as a valid correlation (the map is (H-10) x (W-10)), C1 = (0.01 255)^2,
           C2 = (0.03 255)^2; the mean of the map; min(H, W) >= 11;
  ms_ssim  5 scales, weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), a 2 x 2 mean between scales (an odd last row or column
           is dropped), per plane the mean cs of scales 0..3 and the mean ssim of scale 4, each clamped at 0 before its power;
           min(H, W) >= 176.
What is pinned: the kernels (csrc/compare.hip) against that restatement (tests/test_compare_gpu.py, profiles/compare_parity.txt),
sse exactly.  What is not: the restatement against any external SSIM implementation (none was installed where it was written):
restated from the published definition, not pinned against an external implementation.

On the GPU: one launch per scale computes every plane's windowed moments in fp64 and leaves one partial sum per block, a
second sums them in a fixed order; between the scales one launch halves both clips.  The host turns 30 means and one integer
per frame into the numbers.  No atomics: the same bits on every run, for any number of frames per call, and for (b, a).

    python -m vdx.compare A B [--json OUT] [--lpips_model FILE] [--no_ms_ssim]
"""
from __future__ import annotations

import json
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import flow as _flow, frames as _frames
from ._lib import VdxError

WIN, SIGMA = 11, 1.5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIDE = WIN
MS_MIN_SIDE = WIN << (len(MS_WEIGHTS) - 1)            # 176: the fifth scale still holds one window
METRICS = ("psnr", "ssim", "ms_ssim", "lpips")


def window() -> np.ndarray:
    """The 11 float64 taps: exp(-d^2 / (2 sigma^2)), normalised to sum 1."""
    d = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def check_pair(a, b, ms_ssim: bool = True) -> Tuple[int, int, int]:
    """Two uint8 RGB clips of one shape, F >= 1, min(H, W) >= 11 (176 with `ms_ssim`) -> (F, H, W); `VdxError` otherwise."""
    sa, sb = _frames.check(a, "compare"), _frames.check(b, "compare")
    if sa != sb:
        raise VdxError(f"compare: the clips differ in shape: {sa} and {sb} (frames, height, width)")
    F, H, W = sa
    if F < 1:
        raise VdxError("compare: no frames")
    if min(H, W) < MIN_SIDE:
        raise VdxError(f"compare: frames of {H}x{W} are too small for SSIM (min(H, W) >= {MIN_SIDE})")
    if ms_ssim and min(H, W) < MS_MIN_SIDE:
        raise VdxError(f"compare: frames of {H}x{W} are too small for MS-SSIM (min(H, W) >= {MS_MIN_SIDE}); SSIM and PSNR "
                       "are available with ms_ssim=False")
    return F, H, W


def seam_frames(n_frames: int, ranges: Sequence[Tuple[int, int]]) -> List[int]:
    """The frames either side of every chunk boundary `metrics.boundary_l1` compares: e-1 and e for every chunk end e but the
    last chunk's (in start order) with 0 < e < n_frames; sorted, each once."""
    out = set()
    for e in _flow.boundary_pairs(n_frames, ranges):
        out.update((e - 1, e))
    return sorted(out)


def plane_means(a: torch.Tensor, b: torch.Tensor, scales: int = 1):
    """Two packed uint8 RGB clips (F, H, W, 3) on one GPU -> (means fp64 (F, 3, 5, 2) on the device: mean ssim and mean cs of
    every plane at scales 0 .. scales-1, zeros beyond; sse int64 [F])."""
    from . import ops
    F, H, W = (int(v) for v in a.shape[:3])
    taps = window()
    means = torch.zeros((F, 3, ops.COMPARE_SCALES, 2), dtype=torch.float64, device=a.device)
    sse = torch.empty((F,), dtype=torch.int64, device=a.device)
    part, sse_part = ops.compare_ssim_scale(a, b, taps)
    ops.compare_finalize(part, sse_part, (H - WIN + 1) * (W - WIN + 1), 0, means, sse)
    x, y = a, b
    for s in range(1, scales):
        x, y = ops.compare_down2(x, y)
        h, w = int(x.shape[1]), int(x.shape[2])
        part, _ = ops.compare_ssim_scale(x, y, taps)
        ops.compare_finalize(part, None, (h - WIN + 1) * (w - WIN + 1), s, means)
    return means, sse


def psnr_from_sse(sse: int, n: int) -> float:
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 / (sse / n))


def _ssim_of(m: np.ndarray) -> float:
    return float((m[0, 0, 0] + m[1, 0, 0] + m[2, 0, 0]) / 3.0)


def _ms_ssim_of(m: np.ndarray) -> float:
    vals = []
    for c in range(3):
        v = 1.0
        for s, w in enumerate(MS_WEIGHTS):
            mean = m[c, s, 1] if s < len(MS_WEIGHTS) - 1 else m[c, s, 0]
            v *= max(float(mean), 0.0) ** w
        vals.append(v)
    return (vals[0] + vals[1] + vals[2]) / 3.0


def _mean(values: Sequence[float], index=None) -> float:
    v = [values[i] for i in index] if index is not None else list(values)
    return float(sum(v) / len(v))                     # inf when a PSNR in it is


def compare_frames(a, b, *, ms_ssim: bool = True, lpips=None, ranges=None, device=None) -> dict:
    """Two uint8 RGB clips of one shape (tensors, on the GPU used in place; arrays; sequences of (H, W, 3) frames) -> a record:
    per-frame lists `psnr` (floats, `math.inf` where the frames are equal), `sse` (ints), `ssim`, `ms_ssim` (unless
    `ms_ssim=False`; `VdxError` below 176) and, with an `LPIPSAlex` as `lpips`, `lpips` (the distance between a[i] and b[i]);
    `mean` of each; `identical` (every sse is 0); `n_frames`, `height`, `width`.  With `ranges` (the planner's chunk ranges, as
    `metrics.boundary_l1` takes them) that hold a seam: `seam_frames` and the means over them and over the others under `seam`
    and `interior` (absent when every frame is a seam frame).  Everything is checked before anything is uploaded or launched."""
    F, H, W = check_pair(a, b, ms_ssim)
    if lpips is not None and not hasattr(lpips, "distances_device"):
        raise VdxError(f"compare: lpips must be a vdx.lpips.LPIPSAlex, got {type(lpips).__name__}")
    seams = seam_frames(F, ranges) if ranges is not None else []
    dev = _frames.device_for(a if isinstance(a, torch.Tensor) and a.is_cuda else b, device)
    ua, ub = _frames.on_device(a, dev), _frames.on_device(b, dev)
    means, sse = plane_means(ua, ub, len(MS_WEIGHTS) if ms_ssim else 1)
    means, sse = means.cpu().numpy(), [int(v) for v in sse.cpu().tolist()]
    n = 3 * H * W
    rec = {"n_frames": F, "height": H, "width": W, "sse": sse, "psnr": [psnr_from_sse(s, n) for s in sse],
           "ssim": [_ssim_of(means[f]) for f in range(F)]}
    if ms_ssim:
        rec["ms_ssim"] = [_ms_ssim_of(means[f]) for f in range(F)]
    if lpips is not None:
        # pair by pair through the consecutive-frame distance of vdx.lpips: exactly the call a user would make on (a[i], b[i])
        d = torch.cat([lpips.distances_device(torch.stack([ua[i], ub[i]])) for i in range(F)])
        rec["lpips"] = [float(v) for v in d.cpu().tolist()]
    keys = [k for k in METRICS if k in rec]
    rec["mean"] = {k: _mean(rec[k]) for k in keys}
    rec["identical"] = all(s == 0 for s in sse)
    if seams:
        rec["seam_frames"] = seams
        rec["seam"] = {k: _mean(rec[k], seams) for k in keys}
        inner = [i for i in range(F) if i not in set(seams)]
        if inner:
            rec["interior"] = {k: _mean(rec[k], inner) for k in keys}
    return rec


def npy_header_shape(path: str):
    """(shape, dtype) from a .npy file's header, without reading the data; `VdxError` when it is not one."""
    try:
        with open(path, "rb") as f:
            major, minor = np.lib.format.read_magic(f)
            read = {1: np.lib.format.read_array_header_1_0, 2: np.lib.format.read_array_header_2_0}.get(major)
            if read is None:
                raise ValueError(f"format version {major}.{minor}")
            shape, _fortran, dtype = read(f)
    except (OSError, ValueError) as e:
        raise VdxError(f"compare: cannot read {path!r} as .npy: {e}") from None
    return tuple(int(v) for v in shape), dtype


def check_target(path: str, shape: Optional[Tuple[int, int, int, int]] = None) -> None:
    """What can be said about a clip file before anything is loaded: it exists; a .npy is uint8 (F, H, W, 3), and when `shape`
    is given, of that shape.  `VdxError` otherwise."""
    if not os.path.isfile(path):
        raise VdxError(f"compare: {path!r} is not a file")
    if str(path).lower().endswith(".npy"):
        got, dtype = npy_header_shape(path)
        if dtype != np.uint8 or len(got) != 4 or got[3] != 3:
            raise VdxError(f"compare: {path!r} holds {dtype} {got}, expected uint8 (frames, height, width, 3)")
        if shape is not None and got != tuple(shape):
            raise VdxError(f"compare: {path!r} holds frames of shape {got}, the job makes {tuple(shape)}")


def load_clip(path, device=None):
    """A clip file -> uint8 RGB frames: a `.npy` of (F, H, W, 3) (a host array) or a Motion-JPEG `.mp4`, decoded on the GPU by
    `vdx.video.read_frames`, whose refusals are raised as they are."""
    path = os.fspath(path)
    check_target(path)
    if path.lower().endswith(".npy"):
        return np.load(path, allow_pickle=False)
    from .video import read_frames
    frames, _info = read_frames(path, device=device if device is not None else "cuda")
    if frames.dim() != 4:
        raise VdxError(f"compare: {path!r} is a grey stream; RGB frames are needed")
    return frames


def compare_files(path_a, path_b, **kw) -> dict:
    """`compare_frames` of two clip files (`.npy` of uint8 frames, or Motion-JPEG `.mp4` through `vdx.video.read_frames`)."""
    dev = kw.get("device")
    return compare_frames(load_clip(path_a, dev), load_clip(path_b, dev), **kw)


def to_json(rec):
    """The record with every non-finite float as None: JSON has no infinity (an infinite PSNR is `null`; `identical` and the
    per-frame `sse` say why)."""
    if isinstance(rec, dict):
        return {k: to_json(v) for k, v in rec.items()}
    if isinstance(rec, (list, tuple)):
        return [to_json(v) for v in rec]
    if isinstance(rec, float) and not math.isfinite(rec):
        return None
    return rec


def dumps(rec) -> str:
    return json.dumps(to_json(rec), indent=1, allow_nan=False)


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m vdx.compare", description="PSNR / SSIM / MS-SSIM between two clips on the GPU")
    p.add_argument("a", help=".npy of uint8 frames (F, H, W, 3) or a Motion-JPEG .mp4")
    p.add_argument("b")
    p.add_argument("--json", default=None, help="also write the record here")
    p.add_argument("--lpips_model", default=None, help="local LPIPS-AlexNet state dict (lpips layout): adds the lpips distance")
    p.add_argument("--no_ms_ssim", action="store_true", help="PSNR and SSIM only (frames below 176 pixels)")
    p.add_argument("--device", default="cuda")
    args = p.parse_args(argv)
    for path in (args.a, args.b):
        check_target(path)
    lp = None
    if args.lpips_model:
        from .lpips import LPIPSAlex
        lp = LPIPSAlex.from_local(args.lpips_model, device=args.device)
    rec = compare_files(args.a, args.b, ms_ssim=not args.no_ms_ssim, lpips=lp, device=args.device)
    rec = {"a": args.a, "b": args.b, **rec}
    text = dumps(rec)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
