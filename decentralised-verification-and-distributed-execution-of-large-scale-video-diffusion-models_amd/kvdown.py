"""ToDo, token downsampling (Smith et al., "ToDo: Token Downsampling for Efficient Generation of High-Resolution Images",
2024; unpinned): the spatial self-attention of a frame keeps every query, and its keys and values are the hidden state
downsampled by nearest neighbour with factor s, so the attention work falls by s^2 and every query still sees the whole frame.
The projections act per token, so "downsample, then project" names the rows "project, then take every s-th row and column"
names: the kernel, `ops.flash_attn_kvdown` (csrc/flash_kvdown.hip), reads them in the one q|k|v projection.
The host side lives here: the parameters' check, the per-level factor rule, the row map and the record; the switch is
`UNet3DConditionModel.enable_kv_downsample` (vdx/unet3d.py).

The method is restated, not ported: the row choice is pinned against torch's `F.interpolate(scale_factor=1/s,
mode="nearest")` (tests/test_kvdown_host.py), nothing else is."""
from typing import List, Tuple

import torch

MIN_KEY_GRID = 4    # key-grid cells a side below which a job's level-0 frame is refused (`check_frame`)


def check_params(factor=2, max_downsample=1) -> dict:
    """The parameters as the record {"factor", "max_downsample"}; `ValueError` for a factor that is no integer 2..8 or a
    max_downsample outside {1, 2, 4, 8}."""
    for what, v in (("factor", factor), ("max_downsample", max_downsample)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"kv_downsample: {what} must be an integer, got {v!r}")
    if not 2 <= factor <= 8:
        raise ValueError(f"kv_downsample: factor must be 2..8, got {factor} (1 is the plain attention)")
    if max_downsample not in (1, 2, 4, 8):
        raise ValueError(f"kv_downsample: max_downsample must be 1, 2, 4 or 8, got {max_downsample!r}")
    return {"factor": factor, "max_downsample": max_downsample}


def level_factor(params: dict, down: int) -> int:
    """The factor at a level with downsample factor `down`: max(1, factor // down) — the key pitch stays fixed in pixels — and
    1, the plain attention, above max_downsample."""
    return 1 if down > params["max_downsample"] else max(1, params["factor"] // down)


def key_grid(hh: int, ww: int, s: int) -> Tuple[int, int]:
    """(kh, kw) = (hh // s, ww // s): the key grid of an (hh, ww) token grid."""
    return hh // s, ww // s


def key_rows(n_img: int, hh: int, ww: int, s: int) -> torch.Tensor:
    """int64 [n_img][kh kw]: key j of image n is row n hh ww + (j // kw) s ww + (j % kw) s of the row matrices (the tests' map;
    the kernel carries it in registers)."""
    kh, kw = key_grid(hh, ww, s)
    j = torch.arange(kh * kw, dtype=torch.int64)
    one = torch.div(j, kw, rounding_mode="floor") * (s * ww) + (j % kw) * s
    return torch.arange(n_img, dtype=torch.int64)[:, None] * (hh * ww) + one[None, :]


def check_frame(hh: int, ww: int, params: dict) -> None:
    """`ValueError` if the level-0 token grid (hh, ww) of a job leaves a key grid of fewer than `MIN_KEY_GRID` cells a side:
    what the job driver asks before anything is loaded."""
    kh, kw = key_grid(hh, ww, params["factor"])
    if kh < MIN_KEY_GRID or kw < MIN_KEY_GRID:
        raise ValueError(f"kv_downsample: factor {params['factor']} leaves {kh} x {kw} keys of the UNet's frame of {hh} x {ww} "
                         f"latent cells; at least {MIN_KEY_GRID} a side")


def levels(params: dict, hh: int, ww: int, n_levels: int = 4) -> List[dict]:
    """The levels of a UNet on an (hh, ww) level-0 frame whose self-attention runs on downsampled keys:
    [{"down", "factor", "keys"}]."""
    out = []
    for lvl in range(n_levels):
        s = level_factor(params, 1 << lvl)
        if s > 1 and min(key_grid(hh, ww, s)) >= 1:
            out.append({"down": 1 << lvl, "factor": s, "keys": list(key_grid(hh, ww, s))})
        hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    return out
