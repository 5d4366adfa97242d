"""The validator's MD-VQS score and authenticity gate of a generated video on libvdx_hip.so:

    InferNet/neurons/validator.py:120, 1295        self.quality_scorer = MDVQS(); .compute_quality_score(video, prompt)
    InferNet/neurons/validator.py:259, 872         verify_video_authenticity(video)
    InferNet/template/validator/scoring.py:154-343 MDVQS: total = alpha PF + beta VQ + gamma TC, (0.4, 0.3, 0.3)
    InferNet/template/validator/scoring.py:13-67   verify_video_authenticity_common

What it computes, term by term (the same as the reference unless stated):
  * frames: a decoded uint8 RGB clip in any form vdx/frames.py takes.  DEVIATION: every term of the reference re-reads
    the mp4 with OpenCV; here the frames the pipeline decoded are scored directly (vdx/clip_score.py's deviation).  The
    `*_file` entry points start from the file instead: it is decoded once on the GPU (vdx/video.py) and scored from there;
  * PF, prompt fidelity (:213-267): the CLIP score, `CLIPScorer.score` (vdx/clip_score.py), unchanged;
  * VQ, video quality (:269-309): max(0, 1 - mean over consecutive pairs of LPIPS-AlexNet(frame_i, frame_i-1))
    (vdx/lpips.py: restated from the published definition, parity with the `lpips` package unpinned); fewer than two
    frames score 0.0 (:295-297).  The mean is numpy's, over the fp32 per-pair distances as float64 (`.item()` values, :288-301);
  * TC, temporal consistency (:311-339): the mean over consecutive pairs of mean(|Farneback flow|) with the reference's
    parameters (0.5, 3, 15, 3, 5, 1.2, 0); no pairs score 0.0 (:336-337).  By default (`flow="cpu"`) on the CPU through
    `metrics._cv2()` — OpenCV when installed, else the project's own Farneback (vdx/compat/cv2_shim.py: parity with OpenCV
    unpinned).  `MDVQS(..., flow="gpu")` computes the same flow in HIP kernels, batched over all pairs (vdx/flow.py,
    csrc/flow.hip): pinned against the shim (tests/test_flow_gpu.py), the shim against OpenCV still is not.  Measured on one
    MI355X box (profiles/flow_bench.json, 24 frames at 576x1024): the 23 flows take 3.4 ms, TC as a whole 3.5 ms, i.e. 0.15 ms
    per pair where the shim takes 0.70 s for one pair on the same box — 4 700 times the GPU's per-pair time.
    DEVIATION: the reference hands Farneback the 3-channel BGR frames as read (:319-327).  OpenCV's Farneback takes
    single-channel 8-bit images and is believed to reject those, in which case the reference's own TC is its exception
    value 0.0 (:341-343); nobody could run `cv2` where this was written to confirm.  Here the flow is computed on the
    COLOR_RGB2GRAY frames, the evident intent.  Note that TC as defined grows with motion: it is the reference's formula;
  * total = alpha PF + beta VQ + gamma TC (:201-205), in Python floats in this order.
  DEVIATION: the reference turns every exception into 0.0 scores (:186-188, :209-211, ...); here errors raise `VdxError`.

The authenticity gate (:13-67), `verify_video_authenticity(frames)`: per frame the grey image (OpenCV's 8-bit fixed-point
weights, (4899 R + 9617 G + 1868 B + 8192) >> 14 — the reference converts the BGR frame it read with COLOR_BGR2GRAY, the same
weights per colour), its 256-bin histogram normalised in float32 and the entropy -sum p log2(p + 1e-10) in float32 on the
(256, 1) array `calcHist` returns; per consecutive pair mean |a - b| over all bytes; False when the mean or the standard
deviation of either list is below 0.01, or when there are no pairs.  The GPU produces the exact integers
(`ops.frame_stats`: uint32 counts, uint64 absolute-difference sums); `authenticity_from_counts` finishes in numpy with the
reference's dtypes, so the statistics are bit-equal to a numpy restatement of the reference (tests/lpips_ref.py).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import frames as _frames, ops
from ._lib import VdxError
from .clip_score import CLIPScorer
from .lpips import LPIPSAlex

FARNEBACK = (0.5, 3, 15, 3, 5, 1.2, 0)          # scoring.py:325-327
THRESHOLD = 0.01                                # :51, :60


def authenticity_from_counts(hist, diff_sums, bytes_per_frame: int) -> Tuple[bool, Dict[str, Optional[float]]]:
    """The gate's finishing math (:28-63) from exact integers: `hist` [F][256] grey-level counts, `diff_sums` [F-1] sums of
    |a - b| over the `bytes_per_frame` bytes of each consecutive pair -> (verdict, statistics)."""
    hist, diff_sums = np.asarray(hist), np.asarray(diff_sums)
    entropies = []
    for counts in hist:
        h = counts.astype(np.float32).reshape(256, 1)                 # cv2.calcHist: float32 (256, 1)
        h = h / h.sum()
        entropies.append(-np.sum(h * np.log2(h + 1e-10)))
    # np.mean of a uint8 image: the float64 sum of its bytes (exact) over their number
    frame_diffs = [np.float64(int(s)) / np.float64(bytes_per_frame) for s in diff_sums]
    stats = {"entropy_mean": None, "entropy_std": None, "diff_mean": None, "diff_std": None}
    if entropies:
        stats["entropy_mean"], stats["entropy_std"] = float(np.mean(entropies)), float(np.std(entropies))
    if frame_diffs:
        stats["diff_mean"], stats["diff_std"] = float(np.mean(frame_diffs)), float(np.std(frame_diffs))
    if not frame_diffs or not entropies:
        return False, stats
    ok = not (stats["entropy_std"] < THRESHOLD or stats["entropy_mean"] < THRESHOLD
              or stats["diff_std"] < THRESHOLD or stats["diff_mean"] < THRESHOLD)
    return ok, stats


def verify_video_authenticity(frames, device="cuda") -> Tuple[bool, Dict[str, Optional[float]]]:
    """`verify_video_authenticity_common` (scoring.py:13-67) of uint8 RGB frames (F, H, W, 3) -> (verdict, statistics)."""
    F, H, W = _frames.check(frames, "verify_video_authenticity")
    if F == 0:
        return authenticity_from_counts(np.zeros((0, 256), np.uint32), np.zeros((0,), np.uint64), 1)
    hist, diff = ops.frame_stats(_frames.on_device(frames, device))
    return authenticity_from_counts(hist.cpu().numpy().view(np.uint32), diff.cpu().numpy().view(np.uint64), H * W * 3)


def verify_video_authenticity_file(src, device="cuda") -> Tuple[bool, Dict[str, Optional[float]]]:
    """`verify_video_authenticity_common(video_path)` (scoring.py:13-67) of the FILE: `src` (a path, the file's bytes, or a list
    of JPEG byte strings) is decoded on the GPU (vdx/video.py `read_frames`, bit for bit Pillow's decode) and the frames go,
    still on the device, through `verify_video_authenticity`."""
    from .video import read_frames
    return verify_video_authenticity(read_frames(src, device=device)[0], device=device)


class MDVQS:
    """`MDVQS` (scoring.py:154-343) on the HIP path; see the module docstring.  `clip` / `lpips`: a `CLIPScorer` and an
    `LPIPSAlex` (each term raises `VdxError` without its model)."""

    def __init__(self, clip: Optional[CLIPScorer] = None, lpips: Optional[LPIPSAlex] = None, alpha: float = 0.4,
                 beta: float = 0.3, gamma: float = 0.3, flow: str = "cpu"):
        if flow not in ("cpu", "gpu"):
            raise VdxError(f"MDVQS: flow must be 'cpu' or 'gpu', got {flow!r}")
        self.clip, self.lpips, self.flow = clip, lpips, flow
        self.alpha, self.beta, self.gamma = alpha, beta, gamma

    @classmethod
    def synthetic(cls, seed: int = 0, device="cuda", **weights) -> "MDVQS":
        return cls(CLIPScorer.synthetic(seed=seed, device=device), LPIPSAlex.synthetic(seed=seed, device=device), **weights)

    @property
    def synthetic_weights(self) -> bool:
        return any(m is not None and m.synthetic_weights for m in (self.clip, self.lpips))

    def compute_prompt_fidelity(self, frames, prompt, tokenizer=None) -> float:
        """:213-267 — `CLIPScorer.score`."""
        if self.clip is None:
            raise VdxError("MDVQS: prompt fidelity needs a CLIPScorer")
        return self.clip.score(frames, prompt, tokenizer=tokenizer)[0]

    def compute_video_quality(self, frames) -> Tuple[float, torch.Tensor]:
        """:269-309 -> (max(0, 1 - mean LPIPS), per-pair distances fp32 [F-1] on the host); no pairs -> (0.0, empty)."""
        if self.lpips is None:
            raise VdxError("MDVQS: video quality needs an LPIPSAlex")
        per = self.lpips(frames)
        if per.numel() == 0:
            return 0.0, per
        avg = float(np.mean([float(d) for d in per]))
        return max(0.0, 1.0 - avg), per

    def compute_temporal_consistency(self, frames) -> float:
        """:311-339 on grey frames (the module docstring's deviation), on the CPU or with `flow="gpu"` on the device of the
        frames (host frames: of the models, else "cuda"); no pairs -> 0.0."""
        if self.flow == "gpu":
            from . import flow as _flow
            if len(frames) == 0:
                return 0.0
            model = self.lpips if self.lpips is not None else self.clip
            on_gpu = isinstance(frames, torch.Tensor) and frames.is_cuda
            return _flow.temporal_consistency(frames, device=None if on_gpu or model is None else model.device)
        from .metrics import _cv2
        cv2 = _cv2()
        fr = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else [np.asarray(f) for f in frames]
        scores, prev = [], None
        for f in fr:
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
                raise VdxError(f"MDVQS: expected uint8 RGB frames (H, W, 3), got {f.dtype} {f.shape}")
            g = cv2.cvtColor(np.ascontiguousarray(f), cv2.COLOR_RGB2GRAY)
            if prev is not None:
                flow = cv2.calcOpticalFlowFarneback(prev, g, None, *FARNEBACK)
                scores.append(np.mean(np.abs(flow)))
            prev = g
        return float(np.mean(scores)) if scores else 0.0

    def compute_md_vqs(self, frames, prompt, tokenizer=None) -> Tuple[float, float, float, float]:
        """:190-207 -> (pf, vq, tc, alpha pf + beta vq + gamma tc)."""
        pf = self.compute_prompt_fidelity(frames, prompt, tokenizer=tokenizer)
        vq = self.compute_video_quality(frames)[0]
        tc = self.compute_temporal_consistency(frames)
        return pf, vq, tc, self.alpha * pf + self.beta * vq + self.gamma * tc

    def compute_md_vqs_file(self, src, prompt, tokenizer=None, device=None) -> Tuple[float, float, float, float]:
        """:190-207 starting from the file as the reference does (`cv2.VideoCapture(video_path)`, :230, :272, :314): `src` is
        decoded once on the GPU (vdx/video.py `read_frames`) and `compute_md_vqs` scores those frames on the device."""
        from .video import read_frames
        model = self.clip if self.clip is not None else self.lpips
        dev = device if device is not None else (model.device if model is not None else "cuda")
        return self.compute_md_vqs(read_frames(src, device=dev)[0], prompt, tokenizer=tokenizer)

    def compute_quality_score(self, frames, prompt, tokenizer=None) -> float:
        """:177-188 — the total alone."""
        return self.compute_md_vqs(frames, prompt, tokenizer=tokenizer)[3]
