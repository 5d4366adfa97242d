"""Regional prompts: the text changes along the frame's space (the host side: the weights; the blend is csrc/region.hip).

`DiffuserConfig(regions=((mask, text), ...))` / `--region MASK.npy TEXT` (repeatable) names up to `MAX_REGIONS` regions: a mask,
uint8 or bool of shape (H, W) or (T, H, W) in pixels, values 0..255 (255: the region's text has full weight; soft edges are
allowed), and the text that conditions the pixels under it.  `cfg.prompt` is text 0, the base: it fills what the regions leave.
In every spatial transformer the cross-attention sub-block `t + attn2(norm2(t), text_j)` of the CONDITIONAL item is evaluated
once per text and the results are blended per pixel with the weights below (vdx/unet3d.py, `ops.region_blend`); the unconditional
item keeps `negative_prompt`, the temporal transformers see no text.  What ComfyUI and AnimateDiff-Evolved call "attention
couple" or regional conditioning: MultiDiffusion's region control moved into the cross-attention, so it costs no extra UNet
call.  No external implementation is installed or pinned; the definition is restated here and in tests/region_ref.py.  The
reference has no counterpart: the option is off by default, and without it nothing here runs.

Weights, once per job, in float64: `a_r` of a latent cell is the mean of `mask / 255` over its 8x8 pixels; a UNet level with
downsample factor `down` has the grid (ceil(h / down), ceil(w / down)) (the UNet's own halving rule) and its cell (y, x) covers
the latent cells [y down, min((y + 1) down, h)) x [x down, min((x + 1) down, w)): its `a_r` is the mean over those.  The base
has `a_0 = max(0, 1 - sum_r a_r)`, and `w_j = a_j / sum_j a_j`, rounded once to fp32: exactly 1.0f / 0.0f where one text owns
a cell.  `region_plan` holds one table (T, hh ww, R + 1) per level and, per (level, clip frame, j), whether text j has any
weight there: a text without weight on any frame of a window is not launched at that level.

One case to know: the weights are the stated float64 arithmetic and nothing else.  Two soft masks meant to be complementary
(`m` and `255 - m`) sum to 1 only up to float64 rounding, so `a_0` can come out as some 1e-16 instead of 0 on a cell; the base text
then has a non-zero fp32 weight there, keeps its flag and is launched, with no visible effect on the row.  Masks that are 0 / 255,
or any set that leaves the base real room, do not meet it.  The definition is kept as stated (tests/region_ref.py is its
yardstick) rather than snapped.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

MAX_REGIONS = 7
VAE_SCALE = 8            # pixels per latent cell and axis
UNET_LEVELS = 4          # the levels a job's plan is built for: the UNet3D's four (downsample factors 1, 2, 4, 8)


@dataclass(frozen=True)
class RegionPlan:
    """`tables[l]`: fp32 (T, hh_l ww_l, R + 1), level l's weights (numpy on the host; device tensors after `to`); `grids[l]`: its
    (hh_l, ww_l); `flags`: bool (levels, T, R + 1), always on the host: text j has a non-zero weight on some cell of that frame."""
    T: int
    h: int
    w: int
    tables: Tuple
    grids: Tuple[Tuple[int, int], ...]
    flags: np.ndarray
    texts: Tuple[str, ...] = ()            # the regions' texts (the base prompt is not among them)

    @property
    def n_texts(self) -> int:
        return int(self.flags.shape[2])

    @property
    def levels(self) -> int:
        return len(self.tables)

    @property
    def on_device(self) -> bool:
        return all(torch.is_tensor(t) and t.is_cuda for t in self.tables)

    def to(self, device) -> "RegionPlan":
        """The plan with its tables as contiguous fp32 tensors on `device`, what `ops.region_blend` takes."""
        tabs = tuple((t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))).to(device).contiguous() for t in self.tables)
        return RegionPlan(self.T, self.h, self.w, tabs, self.grids, self.flags, self.texts)

    def active(self, level: int, s: int, L: int, d: int = 1, ring: bool = False):
        """The texts j with any weight at `level` on the window's clip frames `s + f d` (`ring`: mod T), ascending."""
        if L < 1 or d < 1 or not 0 <= s < self.T or s + (L - 1) * d >= (2 * self.T if ring else self.T):
            raise ValueError(f"regions: bad window start {s}, length {L}, stride {d}{' on the ring' if ring else ''} of {self.T} frames")
        frames = [(s + f * d) % self.T if ring else s + f * d for f in range(L)]
        return [j for j in range(self.n_texts) if self.flags[level, frames, j].any()]


def _mask_array(mask, i: int) -> np.ndarray:
    if isinstance(mask, (str, bytes)) or hasattr(mask, "__fspath__"):
        try:
            mask = np.load(mask, allow_pickle=False)
        except Exception as e:
            raise ValueError(f"regions: the mask of region {i} cannot be read from {mask!r}: {e}")
    if torch.is_tensor(mask):
        mask = mask.cpu().numpy()
    if not isinstance(mask, np.ndarray):
        raise ValueError(f"regions: the mask of region {i} must be an array or the path of a .npy file, got {type(mask).__name__}")
    return mask


def check_region_list(regions, T: int, H: int, W: int):
    """`regions` as a tuple of (mask uint8 (H, W) or (T, H, W), text); `ValueError` for an entry that is no (mask, text) pair, a text that
    is no string, a mask that is not uint8 / bool of shape (H, W) or (T, H, W) for this job's `H`, `W`, `T`, no region at all, and
    more than `MAX_REGIONS` regions."""
    if isinstance(regions, (str, bytes)) or not isinstance(regions, Sequence):
        raise ValueError(f"regions must be a sequence of (mask, text) pairs, got {regions!r}")
    if len(regions) < 1:
        raise ValueError("regions: no region")
    if len(regions) > MAX_REGIONS:
        raise ValueError(f"regions: {len(regions)} regions, at most {MAX_REGIONS} are taken")
    out = []
    for i, r in enumerate(regions):
        if isinstance(r, (str, bytes, np.ndarray)) or torch.is_tensor(r) or not isinstance(r, Sequence) or len(r) != 2:
            raise ValueError(f"regions: an entry must be a (mask, text) pair, got {type(r).__name__} at region {i}")
        mask, text = r
        if not isinstance(text, str):
            raise ValueError(f"regions: the text of region {i} must be a string, got {text!r}")
        mask = _mask_array(mask, i)
        if mask.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"regions: the mask of region {i} must be uint8 or bool, got {mask.dtype}")
        if mask.ndim not in (2, 3):
            raise ValueError(f"regions: the mask of region {i} must have shape (H, W) or (T, H, W), got {tuple(mask.shape)}")
        if tuple(mask.shape[-2:]) != (H, W):
            raise ValueError(f"regions: the mask of region {i} is {mask.shape[-2]}x{mask.shape[-1]}, the job's frames are {H}x{W}")
        if mask.ndim == 3 and mask.shape[0] != T:
            raise ValueError(f"regions: the mask of region {i} has {mask.shape[0]} frames, the clip has {T}")
        mask = mask.astype(np.uint8) * 255 if mask.dtype == np.bool_ else mask
        out.append((np.ascontiguousarray(mask), text))
    return tuple(out)


def check_regions(cfg) -> Optional[tuple]:
    """`cfg.regions` as the job's regions, ((mask uint8 (H, W) or (T, H, W), text), ...) (None when off); `ValueError` before anything
    loads for what `check_region_list` refuses and for the two combinations this version does not take: `tile` (a tile's origin is
    not a whole cell at the deeper levels, and the table has no cropped form) and `prompt_travel` (one text per region for the
    whole clip)."""
    if getattr(cfg, "regions", None) is None:
        return None
    if getattr(cfg, "tile", None) is not None:
        raise ValueError("regions cannot be combined with tile: a tile's origin is not a whole cell at the deeper levels")
    if getattr(cfg, "prompt_travel", None) is not None:
        raise ValueError("regions cannot be combined with prompt_travel: a region has one text for the whole clip")
    if cfg.height % VAE_SCALE or cfg.width % VAE_SCALE:
        raise ValueError(f"regions: the frame {cfg.height}x{cfg.width} is no multiple of {VAE_SCALE} pixels")
    return check_region_list(cfg.regions, cfg.num_frames, cfg.height, cfg.width)


def _segment_mean(a: np.ndarray, down: int) -> np.ndarray:
    """float64 (T, h, w) -> (T, ceil(h / down), ceil(w / down)): the mean over each cell's existing members (clipped at the edges)."""
    h, w = a.shape[1:]
    ys, xs = np.arange(0, h, down), np.arange(0, w, down)
    sums = np.add.reduceat(np.add.reduceat(a, ys, axis=1), xs, axis=2)
    ny = np.minimum(ys + down, h) - ys
    nx = np.minimum(xs + down, w) - xs
    return sums / (ny[:, None] * nx[None, :]).astype(np.float64)


def region_plan(regions, T: int, h: int, w: int, levels: int) -> RegionPlan:
    """The plan of `regions` ((mask, text) pairs; only the masks are read: uint8 / bool (H, W) or (T, H, W) with H = 8 h, W = 8 w)
    for a clip of T frames with the latent grid (h, w) and a UNet of `levels` levels (downsample factors 1, 2, ..., 2^(levels-1)).
    A static mask is broadcast over T."""
    for v, name in ((T, "T"), (h, "h"), (w, "w"), (levels, "levels")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"region_plan: {name} must be an integer >= 1, got {v!r}")
    T, h, w, levels = int(T), int(h), int(w), int(levels)
    checked = check_region_list(regions, T, h * VAE_SCALE, w * VAE_SCALE)
    lat = []
    for mask, _ in checked:
        mask = mask if mask.ndim == 3 else mask[None]
        a = (mask.astype(np.float64) / 255.0).reshape(mask.shape[0], h, VAE_SCALE, w, VAE_SCALE).mean(axis=(2, 4))
        lat.append(np.broadcast_to(a, (T, h, w)))
    tables, grids = [], []
    for lev in range(levels):
        down = 1 << lev
        a = np.stack([_segment_mean(np.ascontiguousarray(x), down) for x in lat], axis=-1)        # (T, hh, ww, R)
        base = np.maximum(0.0, 1.0 - a.sum(axis=-1, keepdims=True))
        a = np.concatenate([base, a], axis=-1)
        wgt = (a / a.sum(axis=-1, keepdims=True)).astype(np.float32)
        hh, ww = wgt.shape[1:3]
        grids.append((hh, ww))
        tables.append(np.ascontiguousarray(wgt.reshape(T, hh * ww, len(checked) + 1)))
    flags = np.stack([(t != 0).any(axis=1) for t in tables])
    return RegionPlan(T, h, w, tuple(tables), tuple(grids), flags, tuple(text for _, text in checked))


def record(plan: RegionPlan) -> dict:
    """The option's entry in the result dict and the JSON records: the regions' count and texts, and `coverage`, the mean weight
    of each text j (the base first) over level 0's cells and frames."""
    t0 = plan.tables[0]
    t0 = t0.cpu().numpy() if torch.is_tensor(t0) else t0
    return {"regions": {"count": len(plan.texts), "texts": list(plan.texts),
                        "coverage": [float(v) for v in t0.astype(np.float64).mean(axis=(0, 1))]}}
