"""Cross-frame attention: the spatial self-attention (`attn1`) of a frame takes its keys and values from REFERENCE FRAMES of
the same clip instead of from the frame's own tokens (all unpinned, restated from the papers):
  first          every frame attends to frame 0 (Khachatryan et al., "Text2Video-Zero", ICCV 2023);
  sparse_causal  frame 0 || the previous frame (Wu et al., "Tune-A-Video", ICCV 2023);
  self_first     the frame itself || frame 0 ("extended attention", ControlVideo);
  self_prev      the frame itself || the previous frame;
  a table        a list of F rows of R frame indices each.
The host side lives here: the table, the parameters' check and the record; the kernel is `ops.flash_attn_frames`
(csrc/flash_frames.hip), the switch `UNet3DConditionModel.enable_cross_frame` (vdx/unet3d.py).

Frame indices are those of the UNet call: in a windowed or co-denoised job every window is a call of its own, and the anchor
("frame 0") is each window's first frame, not the clip's."""
from typing import Sequence, Union

import torch

MODES = ("first", "sparse_causal", "self_first", "self_prev")
MAX_REFS = 4        # the kernel's limit on reference frames per frame

Mode = Union[str, Sequence[Sequence[int]]]


def _rows_of(mode) -> tuple:
    """An explicit table as a tuple of rows of ints; `ValueError` for anything but rows of 1..MAX_REFS integers >= 0, all
    of one length."""
    if isinstance(mode, (str, bytes)) or not isinstance(mode, (list, tuple)) or len(mode) == 0:
        raise ValueError(f"cross_frame: mode must be one of {MODES} or a list of rows of frame indices, got {mode!r}")
    rows = []
    for row in mode:
        if not isinstance(row, (list, tuple)) or not 1 <= len(row) <= MAX_REFS:
            raise ValueError(f"cross_frame: every row of the table names 1 .. {MAX_REFS} frames, got {row!r}")
        if len(row) != len(mode[0]):
            raise ValueError(f"cross_frame: ragged table: rows of {len(mode[0])} and of {len(row)} frames")
        for v in row:
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"cross_frame: a frame index must be an integer >= 0, got {v!r}")
        rows.append(tuple(row))
    return tuple(rows)


def check_params(mode: Mode = "sparse_causal", max_downsample: int = 8) -> dict:
    """The parameters as the record {"mode", "refs_per_frame", "max_downsample"} (`mode`: the name, or the table as a tuple of
    rows); `ValueError` for an unknown name, a table that is ragged, empty, has rows outside 1..4 entries or a negative or
    non-integer index, and a max_downsample outside {1, 2, 4, 8}."""
    if isinstance(max_downsample, bool) or max_downsample not in (1, 2, 4, 8):
        raise ValueError(f"cross_frame: max_downsample must be 1, 2, 4 or 8, got {max_downsample!r}")
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"cross_frame: unknown mode {mode!r}; one of {MODES} or a table")
        return {"mode": mode, "refs_per_frame": 1 if mode == "first" else 2, "max_downsample": max_downsample}
    rows = _rows_of(mode)
    return {"mode": rows, "refs_per_frame": len(rows[0]), "max_downsample": max_downsample}


def ref_table(mode: Mode, F: int) -> torch.Tensor:
    """int32 [F][R] on the host: row f names the frames whose keys and values frame f of a UNet call of F frames attends to, in
    the order of the key stream.  `ValueError` for what `check_params` refuses, F < 1, a table that has not F rows or names a
    frame outside 0 .. F-1."""
    if isinstance(F, bool) or not isinstance(F, int) or F < 1:
        raise ValueError(f"cross_frame: F must be an integer >= 1, got {F!r}")
    mode = check_params(mode)["mode"]
    if mode == "first":
        rows = [(0,) for f in range(F)]
    elif mode == "sparse_causal":
        rows = [(0, max(f - 1, 0)) for f in range(F)]
    elif mode == "self_first":
        rows = [(f, 0) for f in range(F)]
    elif mode == "self_prev":
        rows = [(f, max(f - 1, 0)) for f in range(F)]
    else:
        rows = mode
        if len(rows) != F:
            raise ValueError(f"cross_frame: a table of {len(rows)} rows for a call of {F} frames")
        bad = [v for row in rows for v in row if v >= F]
        if bad:
            raise ValueError(f"cross_frame: the table names frame {bad[0]} of a call of {F} frames")
    return torch.tensor(rows, dtype=torch.int32)
