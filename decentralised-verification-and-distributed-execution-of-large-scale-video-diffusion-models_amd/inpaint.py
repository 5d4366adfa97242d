"""Masked video-to-video: the host side (mask intake, refusals, the per-step coefficients; the selects are csrc/inpaint.hip).

`--init_video` refines a whole clip.  With `DiffuserConfig(mask=...)` / `--mask PATH` or `keep_frames=` / `--keep_frames SPEC`
part of that clip is HELD FIXED and the rest is generated: continuing a clip from its last frames (the replacement method of Ho
et al. 2022, "Video Diffusion Models"), repainting a region through time (RePaint, Lugmayr et al. 2022; Blended Latent
Diffusion, Avrahami et al. 2023; diffusers' `StableDiffusionInpaintPipeline` branch for 4-channel UNets), or filling a hole of a
few frames.  The reference has no counterpart: the option is off by default, and without it nothing here runs.

The definition (restated in tests/inpaint_ref.py).  x0: the scaled clean latent of `--init_video`; base: the job's seeded noise;
m: the latent mask (T,h,w) uint8, 1 = regenerate, 0 = keep; ts: the job's schedule (`vid2vid_timesteps`).  The start is
video-to-video's, unchanged: add_noise(x0, base, ts[0]).  After the scheduler step of ts[i] has produced z: where m == 1 z keeps
its bits; where m == 0 z takes the bits of known_i = add_noise(x0, base, ts[i+1]) (the rounding chain of `vdx_add_noise_f16`,
the coefficients as `scheduler.add_noise` computes them), and known = x0 itself after the last step.  A multistep sampler's x0
history is left as the model produced it.  The mask is binary, so this is a select and not a blend.  After the windows' ramp
blend (which zeroes the clip's first and last frame and re-weights overlaps) the kept cells are pasted once more from x0, and
with `mask_paste` the kept PIXELS of the decoded frames are the input clip's bytes.  Every rank holds identical x0, base and m:
no collective is added.

Pinned (tests/test_inpaint_gpu.py, bit for bit): the four kernels against the torch restatement, an all-zeros mask against
`ops.add_noise` (one shared chain), the windowed and the co-denoised job against a Python loop over the planner's windows, an
all-ones mask against plain video-to-video, two ranks against one.  NOT pinned and not claimed: agreement with diffusers or any
other external implementation, and any quality effect on real Zeroscope weights.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from . import ops

MASK_RULES = ops.MASK_RULES


def keep_frames_mask(spec: str, T: int) -> np.ndarray:
    """`--keep_frames`: comma-separated Python-style slices ("0:8", ":4", "20:", "::2") or single indices ("3", "-1") of the
    frames to KEEP -> uint8 (T,), 1 = regenerate, 0 = keep.  An index outside [-T, T), a slice bound outside [-T, T], a step of
    zero and an empty item are refused."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError(f"keep_frames: expected a spec such as \"0:8,20:24\", got {spec!r}")
    m = np.ones((T,), dtype=np.uint8)
    for item in spec.split(","):
        item = item.strip()
        if not item:
            raise ValueError(f"keep_frames: empty item in {spec!r}")
        try:
            parts = [int(p) if p.strip() else None for p in item.split(":")]
        except ValueError:
            raise ValueError(f"keep_frames: {item!r} is neither an index nor a slice of integers") from None
        if len(parts) > 3:
            raise ValueError(f"keep_frames: {item!r} is neither an index nor a slice")
        if len(parts) == 1:
            i = parts[0]
            if not -T <= i < T:
                raise ValueError(f"keep_frames: frame {i} is outside the clip's {T} frames")
            m[i] = 0
            continue
        for b in parts[:2]:
            if b is not None and not -T <= b <= T:
                raise ValueError(f"keep_frames: {item!r} leaves the clip's {T} frames")
        if len(parts) == 3 and parts[2] == 0:
            raise ValueError(f"keep_frames: {item!r} has a step of zero")
        m[slice(*parts)] = 0
    return m


def load_mask(spec: str, T: int, H: int, W: int) -> np.ndarray:
    """`--mask`: a `.npy` of uint8 / bool shaped (T,H,W), (H,W) (the same region in every frame) or (T,) (whole frames), nonzero
    = regenerate -> the pixel mask uint8 (T,H,W) in {0,1}.  H, W must be the job's height and width: anything else is refused."""
    arr = np.load(spec)
    if arr.dtype != np.uint8 and arr.dtype != np.bool_:
        raise ValueError(f"--mask {spec}: expected uint8 or bool, got {arr.dtype}")
    return expand_mask(arr, T, H, W, f"--mask {spec}")


def expand_mask(arr: np.ndarray, T: int, H: int, W: int, what: str = "mask") -> np.ndarray:
    """(T,H,W), (H,W) or (T,) -> contiguous uint8 (T,H,W) in {0,1} (nonzero = regenerate)."""
    arr = (np.asarray(arr) != 0).astype(np.uint8)
    if arr.shape == (T, H, W):
        full = arr
    elif arr.shape == (H, W):
        full = np.broadcast_to(arr[None], (T, H, W))
    elif arr.shape == (T,):
        full = np.broadcast_to(arr[:, None, None], (T, H, W))
    else:
        raise ValueError(f"{what}: shape {arr.shape} is none of ({T},{H},{W}), ({H},{W}), ({T},) (the job's frames, height, width)")
    return np.ascontiguousarray(full)


def masked(cfg) -> bool:
    return cfg.mask is not None or cfg.keep_frames is not None


def pixel_mask(cfg) -> Optional[np.ndarray]:
    """The job's pixel mask uint8 (T,H,W) from `cfg.mask` (a path, or an array in one of `load_mask`'s shapes) or
    `cfg.keep_frames`; None without either."""
    T, H, W = cfg.num_frames, cfg.height, cfg.width
    if cfg.mask is not None:
        return load_mask(cfg.mask, T, H, W) if isinstance(cfg.mask, str) else expand_mask(cfg.mask, T, H, W)
    if cfg.keep_frames is not None:
        return expand_mask(keep_frames_mask(cfg.keep_frames, T), T, H, W, "keep_frames")
    return None


def latent_mask_host(px: np.ndarray, rule: str = "nearest") -> np.ndarray:
    """What `ops.mask_to_latent` computes, on the host (numpy): the refusals need it before any model or device is touched."""
    if rule not in MASK_RULES:
        raise ValueError(f"mask_rule must be one of {MASK_RULES}, got {rule!r}")
    T, H, W = px.shape
    if H % 8 or W % 8:
        raise ValueError(f"mask: height {H} and width {W} must be multiples of 8")
    if rule == "nearest":
        return np.ascontiguousarray(px[:, ::8, ::8] != 0).astype(np.uint8)
    return (px.reshape(T, H // 8, 8, W // 8, 8) != 0).any(axis=(2, 4)).astype(np.uint8)


def check_mask(cfg, exchange: str = "allgather") -> Optional[np.ndarray]:
    """The job's pixel mask (None when the option is off); `ValueError` before any model is loaded when the job cannot run it: a
    mask without `init_video`, `mask` together with `keep_frames`, the halo exchange (the paste needs the whole blend on every
    rank), a rule that is not one, a mask of another shape, or a mask that regenerates nothing."""
    if not masked(cfg):
        if cfg.mask_rule not in MASK_RULES:
            raise ValueError(f"mask_rule must be one of {MASK_RULES}, got {cfg.mask_rule!r}")
        return None
    if cfg.mask is not None and cfg.keep_frames is not None:
        raise ValueError("mask and keep_frames exclude each other: give the frames to keep as part of the mask, or only one of them")
    if cfg.init_video is None:
        raise ValueError("mask / keep_frames need init_video: the kept content is that clip's")
    if exchange == "halo":
        raise ValueError("mask / keep_frames need exchange=\"allgather\": the paste after the blend needs the whole latent on every rank")
    px = pixel_mask(cfg)
    lat = latent_mask_host(px, cfg.mask_rule)
    if not lat.any():
        raise ValueError("the mask keeps everything: no latent cell is left to regenerate (nonzero = regenerate; "
                         f"mask_rule {cfg.mask_rule!r})")
    return px


def mask_record(latent_mask, rule: str, paste: bool) -> dict:
    """The `"mask"` entry of the result dict and the JSON records: `kept_fraction` of latent cells, `kept_frames` = frames kept
    entirely."""
    m = latent_mask.cpu().numpy() if torch.is_tensor(latent_mask) else np.asarray(latent_mask)
    return {"rule": rule, "paste": bool(paste), "kept_fraction": float((m == 0).mean()),
            "kept_frames": int((m.reshape(m.shape[0], -1) == 0).all(axis=1).sum())}


def known_coefficients(scheduler, schedule: List[int], like: torch.Tensor) -> List[Optional[Tuple[float, float]]]:
    """Per step i of `schedule`, `add_noise`'s (sqrt(a), sqrt(1 - a)) of the NEXT timestep, as `scheduler.add_noise` computes
    them for a sample like `like`; None for the last step (known = x0)."""
    return [scheduler.add_noise_coefficients(t, like) for t in schedule[1:]] + [None]
