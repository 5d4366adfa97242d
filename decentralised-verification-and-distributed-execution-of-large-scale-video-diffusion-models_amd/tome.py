"""Token merging (Bolya & Hoffman, "Token Merging for Stable Diffusion", CVPRW 2023; the `tomesd` package, unpinned) around the
spatial self-attention: the host side.  No reference counterpart.  The partition of an (hh, ww) token grid into destinations
and sources is built here, once per grid; matching, selection, merge and unmerge are `ops.tome_*` (csrc/tome.hip);
`UNet3DConditionModel.enable_tome` (vdx/unet3d.py) is the switch.  tests/tome_ref.py states the whole definition.

Deviation from `tomesd`, stated: with a seed it redraws the cell offsets on every call; here they are drawn once per (hh, ww)
from a seeded CPU generator and held fixed over steps and calls, so a run is reproducible launch for launch.  Without a seed
every cell's destination is its (0, 0) token (`tomesd`'s `use_rand=False`)."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch


class Partition(NamedTuple):
    src_idx: torch.Tensor       # int32 [n_src] token indices of the sources, ascending (CPU)
    dst_idx: torch.Tensor       # int32 [n_dst] token indices of the destinations, ascending (CPU)
    r: int                      # sources merged per image: min(int(S ratio), n_src)
    offsets: torch.Tensor       # int64 [cells_h][cells_w] the destination's index oy * sx + ox inside each cell

    @property
    def n_src(self) -> int:
        return int(self.src_idx.numel())

    @property
    def n_dst(self) -> int:
        return int(self.dst_idx.numel())


def check_params(ratio, sx=2, sy=2, seed=None, max_downsample=1) -> dict:
    """The parameters as the record {"ratio", "sx", "sy", "seed", "max_downsample"}; `ValueError` for a ratio that is not finite
    or outside (0, 1 - 1 / (sx sy)], a stride below 1 or cells of one token, a max_downsample outside {1, 2, 4, 8}."""
    def _int(what, v):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"tome: {what} must be an integer, got {v!r}")
        return v
    sx, sy = _int("sx", sx), _int("sy", sy)
    if sx < 1 or sy < 1 or sx * sy < 2:
        raise ValueError(f"tome: cells of sy x sx = {sy} x {sx} tokens (each stride at least 1, at least 2 tokens per cell)")
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not math.isfinite(ratio):
        raise ValueError(f"tome: ratio must be a finite number, got {ratio!r}")
    if not 0 < ratio <= 1 - 1 / (sx * sy):
        raise ValueError(f"tome: ratio {ratio!r} outside (0, {1 - 1 / (sx * sy)}]")
    if _int("max_downsample", max_downsample) not in (1, 2, 4, 8):
        raise ValueError(f"tome: max_downsample must be 1, 2, 4 or 8, got {max_downsample!r}")
    if seed is not None:
        _int("seed", seed)
    return {"ratio": float(ratio), "sx": sx, "sy": sy, "seed": seed, "max_downsample": max_downsample}


SELECT_LDS_MAX = 160 * 1024 - 256     # bytes of LDS `vdx_tome_select` takes (csrc/tome.hip): it holds one image's keys there


def select_lds(n_src: int, n_dst: int) -> int:
    """`vdx_tome_select_lds` restated for the host: 64-bit keys for n_src rounded up to a power of two, a counter per
    destination, a flag per source."""
    if n_src < 1 or n_dst < 1:
        return 0
    return (1 << (n_src - 1).bit_length()) * 8 + n_dst * 4 + (n_src + 15) // 16 * 16


def check_grid(hh: int, ww: int, params: dict) -> None:
    """`ValueError` if the level-0 token grid (hh, ww) of a job is one the select kernel cannot take (about 16 000 tokens):
    what the job driver asks before anything is loaded.  Deeper levels have a quarter of the tokens each and always fit then."""
    ch, cw = hh // params["sy"], ww // params["sx"]
    n_dst = ch * cw
    n_src = hh * ww - n_dst
    if n_dst and min(int(hh * ww * params["ratio"]), n_src) and select_lds(n_src, n_dst) > SELECT_LDS_MAX:
        raise ValueError(f"tome: a {hh} x {ww} token grid ({n_src} sources, {n_dst} destinations) is more than the select kernel "
                         f"holds in LDS ({select_lds(n_src, n_dst)} > {SELECT_LDS_MAX} bytes): use a smaller frame or --tile")


def partition(hh: int, ww: int, ratio: float, sx: int = 2, sy: int = 2, seed: Optional[int] = None) -> Partition:
    """The grid cut into (hh // sy) (ww // sx) cells of sy x sx tokens: the token at each cell's offset is a destination, every
    other token, the leftover rows and columns included, a source.  Offsets are (0, 0), or with `seed` one draw of
    `torch.randint(sy sx, (cells_h, cells_w))` from `torch.Generator().manual_seed(seed)` (index v = oy sx + ox)."""
    ch, cw = hh // sy, ww // sx
    if seed is None:
        offsets = torch.zeros((ch, cw), dtype=torch.int64)
    else:
        offsets = torch.randint(sy * sx, (ch, cw), generator=torch.Generator().manual_seed(seed))
    is_dst = torch.zeros((hh, ww), dtype=torch.bool)
    if ch and cw:
        ys = torch.arange(ch).view(-1, 1) * sy + offsets // sx
        xs = torch.arange(cw).view(1, -1) * sx + offsets % sx
        is_dst[ys, xs] = True
    flat = is_dst.reshape(-1)
    tok = torch.arange(hh * ww, dtype=torch.int32)
    src, dst = tok[~flat].contiguous(), tok[flat].contiguous()
    return Partition(src, dst, min(int(hh * ww * ratio), int(src.numel())), offsets)
