"""HyperTile (tfernd, "HyperTile: Tiled-optimizations for Stable-Diffusion", 2023; unpinned): the spatial self-attention of a
frame computed inside the windows of an ny x nx grid instead of over the whole frame.  The attention work falls by ny nx and
nothing is matched, selected or merged.  The host side lives here: the parameters' check, the per-level grid rule and the
record; the kernel is `ops.flash_attn_win` (csrc/flash_win.hip), the switch
`UNet3DConditionModel.enable_hypertile` (vdx/unet3d.py).

Deviation from the published method, stated: it redraws the tile count per call among the nearest divisors (`swap_size`);
here the grid is fixed, as token merging's seeded offsets are held."""
from typing import List, Optional, Tuple

MIN_WINDOW = 8      # latent cells a side below which a job's level-0 window is refused (`check_frame`)


def check_params(ny, nx, max_downsample=1) -> dict:
    """The parameters as the record {"grid": (ny, nx), "max_downsample"}; `ValueError` for a grid count that is no integer >= 1
    or a max_downsample outside {1, 2, 4, 8}."""
    for what, v in (("ny", ny), ("nx", nx), ("max_downsample", max_downsample)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"hypertile: {what} must be an integer, got {v!r}")
    if ny < 1 or nx < 1:
        raise ValueError(f"hypertile: a grid of ny x nx = {ny} x {nx} windows (each at least 1)")
    if max_downsample not in (1, 2, 4, 8):
        raise ValueError(f"hypertile: max_downsample must be 1, 2, 4 or 8, got {max_downsample!r}")
    return {"grid": (ny, nx), "max_downsample": max_downsample}


def level_grid(params: dict, down: int) -> Optional[Tuple[int, int]]:
    """The grid at a level with downsample factor `down`: (max(1, ny // down), max(1, nx // down)) — a tile keeps its size in
    pixels — or None above max_downsample."""
    if down > params["max_downsample"]:
        return None
    ny, nx = params["grid"]
    return max(1, ny // down), max(1, nx // down)


def window_grid(params: dict, hh: int, ww: int, down: int) -> Optional[Tuple[int, int]]:
    """The grid the windowed kernel runs with on an (hh, ww) token grid at that level, or None where the plain attention runs:
    above max_downsample, a 1 x 1 grid, a grid that does not divide the tokens.  At level 0 the last is a `ValueError`."""
    g = level_grid(params, down)
    if g is None or g == (1, 1):
        return None
    if hh % g[0] or ww % g[1]:
        if down == 1:
            raise ValueError(f"hypertile: the {g[0]} x {g[1]} grid does not divide the {hh} x {ww} tokens of level 0")
        return None
    return g


def check_frame(hh: int, ww: int, params: dict) -> None:
    """`ValueError` if the level-0 token grid (hh, ww) of a job is one the grid does not divide, or its windows have fewer than
    `MIN_WINDOW` latent cells a side: what the job driver asks before anything is loaded."""
    ny, nx = params["grid"]
    if hh % ny or ww % nx:
        raise ValueError(f"hypertile: the {ny} x {nx} grid does not divide the UNet's frame of {hh} x {ww} latent cells")
    if hh // ny < MIN_WINDOW or ww // nx < MIN_WINDOW:
        raise ValueError(f"hypertile: windows of {hh // ny} x {ww // nx} latent cells; at least {MIN_WINDOW} a side")


def levels(params: dict, hh: int, ww: int, n_levels: int = 4) -> List[dict]:
    """The levels of a UNet on an (hh, ww) level-0 frame whose self-attention runs windowed: [{"down", "grid", "window"}]."""
    out = []
    for lvl in range(n_levels):
        g = window_grid(params, hh, ww, 1 << lvl)
        if g is not None:
            out.append({"down": 1 << lvl, "grid": list(g), "window": [hh // g[0], ww // g[1]]})
        hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    return out
