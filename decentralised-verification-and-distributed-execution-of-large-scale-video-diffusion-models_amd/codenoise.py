"""Temporal co-denoising: the host side (integers, weights and the per-step loop; the arithmetic is csrc/codenoise.hip).

The job's default keeps one trajectory per window and lets the windows meet once, after the loop, in the ramp blend.  With
`DiffuserConfig(co_denoise=True)` / `--co_denoise` there is ONE latent for the whole clip instead (MultiDiffusion, Bar-Tal et al.
2023, applied along time; Gen-L-Video's "temporal co-denoising", Wang et al. 2023; what AnimateDiff's context windows do): at
every step each window predicts noise for its slice of that latent, the predictions are averaged where windows overlap, and one
scheduler step advances the whole clip.  Frames that two windows share cannot diverge: there is one copy of them.  DDIM (eta 0)
and DPM-Solver++ 2M are linear in the noise and the weights sum to 1, so averaging the predictions is averaging the stepped
latents.  The reference has no counterpart: the option is off by default, and without it nothing here runs.

Pinned (tests/test_codenoise_gpu.py, bit for bit): the kernels against the torch restatement of tests/codenoise_ref.py, a
one-window job against `DistributedVideoDiffuser.denoise`, a several-window job against a Python loop over the same windows, and
a two-rank job against the one-rank job.  NOT pinned and not claimed: agreement with any external implementation, and any
seam-quality effect on real Zeroscope weights.

With `DiffuserConfig(tile=(TH, TW))` / `--tile TH TW` the windows are additionally tiled in space (MultiDiffusion's original form;
csrc/cotile.hip): a window is the product of a time window, a row band and a column band, every UNet call is a crop of one tile's
size, and the fused step averages with the product of three per-axis normalised weights (`tile_plan` below; `check_tile` in vdx/options.py).  Pinned
in tests/test_cotile_gpu.py against tests/cotile_ref.py; again no external implementation and no quality claim.

With `DiffuserConfig(loop=True)` / `--loop` the windows lie on a RING (AnimateDiff's `closed_loop` context option; MultiDiffusion
along time with periodic windows; csrc/codenoise.hip, its RING flag): `loop_plan` spreads windows of one length evenly over the clip and lets the
last ones wrap over its end into the first frames, so frames T-1 and 0 are denoised together in one UNet call at every step like
any other neighbouring pair, and the clip played as a loop has no jump there (`loop_table` below; `check_loop` in vdx/options.py).  Pinned in
tests/test_coloop_gpu.py against tests/coloop_ref.py, the wrap itself by rotation equivariance; NOT pinned and not claimed: no
external implementation is pinned, and there is no quality claim on real Zeroscope weights.

With `DiffuserConfig(context_stride=N)` / `--context_stride N`, N > 1, the job also denoises STRIDED windows (AnimateDiff-Evolved's
`context_stride`, the "uniform" context schedule; csrc/codenoise.hip, its `costride_tab`): level l < N adds windows that take
every 2^l-th frame, so frames further apart than a window share a UNet call at every step, and every level has the share 1/N of a
frame's fused noise (`stride_plan`, `stride_table` below; `check_stride` in vdx/options.py).  Each level costs its windows' UNet calls.  Pinned in
tests/test_costride_gpu.py against tests/costride_ref.py, the stride itself by permuting the clip; NOT pinned and not claimed:
no external implementation is pinned (the schedule is restated), and there is no quality claim on real Zeroscope weights, whose
temporal layers were trained on consecutive frames and see faster motion in a strided window.

Whatever the plan, a window is ONE row here, `Window(s, L, d, ring)`: the frames `s + f * d`, f in [0, L), mod T on a ring
(`plan_windows`, `rank_windows`).  `_fuse_table` is the one builder of the normalised weights, behind `window_table`, `loop_table`
and `stride_table`, and `co_denoise_round` the one per-step loop: it reads its input op and its scheduler step from `_KINDS` once.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .options import MIN_TILE_CELLS, check_co_denoise, check_loop, check_stride, check_tile  # noqa: F401  (their home is vdx/options.py)
from .planner import ChunkPlan, PlannerError, auto_chunk


def fuse_weights(length: int, overlap: int) -> List[float]:
    """Raw weight of frame j of a window: `min(j + 1, length - j, overlap + 1) / (overlap + 1)`: a ramp of `overlap` frames at
    either end and 1 between, STRICTLY positive.  (The reference's blend ramp has exact zeros at a window's ends, which survive
    its division only through `clamp(min=1e-6)`; a frame that only such an end covers would have no noise to step with.)"""
    if length < 1 or overlap < 0:
        raise ValueError(f"fuse_weights: length {length} must be >= 1 and overlap {overlap} >= 0")
    return [min(j + 1, length - j, overlap + 1) / (overlap + 1) for j in range(length)]


class Window(NamedTuple):
    """One window, whatever plan it came from: the `L` frames `s + f * d`, f in [0, L), taken mod T when `ring`.  It is what
    `DistributedVideoDiffuser.window_text` and `region_kw` take, in their order."""
    s: int
    L: int
    d: int = 1
    ring: bool = False


def plan_windows(plan, ring: bool = False) -> List[Window]:
    """Every window of a plan in plan order: a `ChunkPlan`'s ranges (`ring`: a `loop_plan`'s) or a `StridePlan`'s windows."""
    if isinstance(plan, StridePlan):
        return [Window(s, L, d) for s, L, d in plan.windows]
    return [Window(s, e - s, 1, ring) for s, e in plan.ranges]


def rank_windows(plan, rank: int, ring: bool = False) -> Tuple[List[Window], int, int]:
    """(this rank's windows, `chunk`, `per_rank`) of any plan: window i belongs to rank `i % world`; `chunk`, the longest window,
    sizes a slot of the packed buffer, and every rank has `per_rank` of them."""
    return plan_windows(plan, ring)[rank::plan.world], plan.chunk, plan.per_rank


@dataclass(frozen=True)
class StrideTable:
    """`fused`: (index in the plan, s, L, d) of the windows that enter the fuse, in plan order; `wn`: fp32 (K, T), the normalised
    weights, zero outside a window."""
    fused: Tuple[Tuple[int, int, int, int], ...]
    wn: torch.Tensor

    def rows(self, world: int, per_rank: int, slot_elems: int) -> List[Tuple[int, int, int, int]]:
        """(element offset, first frame, length, stride) per fused window in the packed buffer `[world][per_rank][slot]`: window i
        of the plan sits at rank i % world, slot i // world."""
        return [(((i % world) * per_rank + i // world) * slot_elems, s, L, d) for i, s, L, d in self.fused]


@dataclass(frozen=True)
class WindowTable:
    """A `StrideTable` of stride 1 as flat and ring plans are read: `fused` rows (index in the plan, s, e), e = s + L (past T where
    a ring window wraps), and `rows()` without the stride column."""
    fused: Tuple[Tuple[int, int, int], ...]
    wn: torch.Tensor

    def rows(self, world: int, per_rank: int, slot_elems: int) -> List[Tuple[int, int, int]]:
        return [(((i % world) * per_rank + i // world) * slot_elems, s, e - s) for i, s, e in self.fused]


def _fuse_table(windows: List[Window], T: int, overlap: int, name: str) -> StrideTable:
    """The one builder of fuse tables: `windows` in plan order, window i at index i.  A window that repeats an earlier one (the
    planner's repeated tail, a strided plan's padding) is still DENOISED by its rank, so that all ranks make the same number of
    UNet calls and the sharded parameters' gathers stay in lockstep, but it is left out of the fuse; a ring plan has no such
    window, and every ring window given enters the fuse.  Raw weights `fuse_weights(L, overlap)[f]` at frame `s + f * d` (mod T on
    a ring), normalised in float64 PER STRIDE over the fused windows of that stride that hold the frame (every frame must be in
    one), times `1 / strides` in float64 where there is more than one stride, rounded to fp32 once: exactly 1.0 where one window
    covers a frame, and every stride has the same share of every frame's noise.  `ValueError`, under `name`: a window that
    leaves the T frames, more than `ops.COFUSE_MAX_WINDOWS` fused windows, a frame in no window."""
    fused = []                                                    # (index in the plan, s, L, d)
    for i, w in enumerate(windows):
        s, L, d, ring = w
        if not (d >= 1 and L >= 1 and 0 <= s < T and (L - 1) * d + (0 if ring else s) < T):   # a ring window may pass T, not lap itself
            raise ValueError(f"{name}: window {i} = " + (f"[{s}, {s + L})" if d == 1 else f"({s}, {L}, {d})")
                             + (f" is no ring window of {T} frames" if ring else f" leaves the {T} frames"))
        if ring or w not in windows[:i]:                          # a ring plan repeats none: what `loop_table` is given, it fuses
            fused.append((i, s, L, d))
    if len(fused) > ops.COFUSE_MAX_WINDOWS:
        raise ValueError(f"{name}: {len(fused)} windows, the fused step takes {ops.COFUSE_MAX_WINDOWS}")
    raw = np.zeros((len(fused), T), dtype=np.float64)
    for k, (_, s, L, d) in enumerate(fused):
        raw[k, (s + d * np.arange(L)) % T] = fuse_weights(L, overlap)     # only a ring window reaches T
    strides = sorted({w[3] for w in fused}) or [1]
    wn = np.zeros_like(raw)
    for d in strides:
        level = np.array([w[3] == d for w in fused], dtype=bool)
        total = raw[level].sum(axis=0)
        if (total <= 0).any():
            raise ValueError(f"{name}: frame {int(np.argmin(total > 0))} is in no window" + (f" of stride {d}" if strides != [1] else ""))
        wn[level] = raw[level] / total
    if len(strides) > 1:
        wn = wn * (1.0 / len(strides))
    return StrideTable(tuple(fused), torch.from_numpy(wn.astype(np.float32)))


def _flat_table(tab: StrideTable) -> WindowTable:
    return WindowTable(tuple((i, s, s + L) for i, s, L, _ in tab.fused), tab.wn)


def window_table(chunk_plan: ChunkPlan, T: int) -> WindowTable:
    """`_fuse_table` of the plan's windows `[s, e)`; `rows()`: (offset, first frame, length)."""
    return _flat_table(_fuse_table(plan_windows(chunk_plan), T, chunk_plan.overlap, "window_table"))


# ---- ring windows (seamless looping; csrc/codenoise.hip, its RING flag) -----------------------------------------------------------------------------
def loop_plan(total: int, world: int, chunk_size: int = 0, overlap: int = 4, overlap_rule: str = "coherent") -> ChunkPlan:
    """The windows of a looping clip: `size` and `ov` by the planner's own rules (`auto_chunk`, the overlap rule), `ov >= 1`;
    with `step = size - ov`, `n = world * ceil(ceil(total / step) / world)` windows `(s_i, s_i + size)`, `s_i = (i * total) // n`:
    evenly spread, ascending, ALL of one length (no short tail window, no repeated window).  A range's end may exceed `total`: it
    means the frames `(s + f) mod total`.  Consecutive starts (cyclically) are at most `step` apart, so every cyclically
    adjacent pair of windows shares at least `ov` frames and every pair of frames `(t, (t + 1) mod total)` lies together in some
    window.  `PlannerError` when `size >= total` (one window is a line, not a ring, and the UNet's temporal layers are not
    circular) and when `n > total` (the starts could not be distinct)."""
    if total <= 0 or world <= 0:
        raise PlannerError("num_frames and world size must be positive")
    size = chunk_size if chunk_size > 0 else auto_chunk(total, world)
    if overlap_rule == "coherent":
        ov = overlap if overlap > 0 else max(4, size // 3)
    elif overlap_rule == "third":
        ov = min(overlap, size // 3)
    else:
        raise PlannerError(f"unknown overlap rule {overlap_rule!r}")
    if size >= total:
        raise PlannerError(f"a window of {size} frames holds the whole clip of {total}: one window is a line, not a ring "
                           "(the UNet's temporal layers are not circular); use a chunk shorter than the clip")
    if ov < 1:
        raise PlannerError(f"overlap {ov}: neighbouring ring windows must share at least one frame")
    step = size - ov
    if step <= 0:
        raise PlannerError(f"overlap {ov} >= chunk {size}: windows would never advance")
    n = world * -(-(-(-total // step)) // world)
    if n > total:
        raise PlannerError(f"{n} ring windows for {total} frames: their starts could not be distinct")
    return ChunkPlan(size, ov, tuple(((i * total) // n, (i * total) // n + size) for i in range(n)), world)


def loop_plan_of(cfg, world: int) -> ChunkPlan:
    """`loop_plan` of a job's config; mode "fsdp" (`no_chunking`) asks for one window of the whole clip, which it refuses."""
    return loop_plan(cfg.num_frames, world, cfg.num_frames if cfg.no_chunking else cfg.chunk_size, cfg.overlap, cfg.overlap_rule)


def loop_table(chunk_plan: ChunkPlan, T: int) -> WindowTable:
    """`window_table` for a ring plan: a range `(s, e)` means the frames `(s + f) mod T`, `0 <= s < T`, `1 <= e - s <= T` (a ring
    plan repeats no window, so every one enters the fuse); `rows()` is unchanged: (offset, first frame, length)."""
    return _flat_table(_fuse_table(plan_windows(chunk_plan, True), T, chunk_plan.overlap, "loop_table"))


# ---- strided context windows (AnimateDiff-Evolved's `context_stride`; csrc/codenoise.hip, its `costride_tab`) -----------------------
@dataclass(frozen=True)
class StridePlan:
    """The windows of a strided job in plan order, `(s, L, d)` = the frames `s + f * d`, f in [0, L): window i belongs to rank
    `i % world`.  `chunk` is the longest window (it sizes a slot of the packed buffer), `overlap` the planner's, `levels` the
    number of strides 1, 2, 4, ...; `base` is the level-0 `ChunkPlan`, the job's plan without the option."""
    chunk: int
    overlap: int
    windows: Tuple[Tuple[int, int, int], ...]
    world: int
    levels: int
    base: ChunkPlan

    def for_rank(self, rank: int) -> List[Tuple[int, int, int]]:
        return [w for i, w in enumerate(self.windows) if i % self.world == rank]

    @property
    def per_rank(self) -> int:
        return len(self.windows) // self.world

    @property
    def strides(self) -> List[int]:
        return [1 << l for l in range(self.levels)]


def stride_plan(total: int, world: int, chunk_size: int = 0, overlap: int = 4, overlap_rule: str = "coherent", levels: int = 1,
                no_chunking: bool = False) -> StridePlan:
    """The "uniform" context schedule: level l in [0, levels) has stride d = 2^l.  Level 0 is the planner's own plan (`plan`, its
    repeated tail window included), as `(s, e - s, 1)`.  For d > 1 every residue r in [0, d) has the subsequence r, r + d, ... of
    `n_r = ceil((total - r) / d)` frames, covered by windows of ONE length `min(size, n_r)` by `tile_starts`' rule (starts 0,
    size - ov, ..., the last moved back to end at the edge; `size`, `ov` the level-0 plan's) and mapped back to
    `(r + d * s', L, d)`.  Levels ascending, residues ascending, starts ascending; the count is then padded to a multiple of
    `world` by repeating the last window (denoised, so the ranks stay in lockstep, but not fused: `stride_table`).  With
    `ov >= 1` (every "coherent" plan) any two frames t, t + d with t + d < total lie together in some window of the level of d.
    `PlannerError` for `levels < 1` and for `2^levels > total` (a level whose subsequences hold fewer than two frames adds
    nothing); `no_chunking` (mode "fsdp") makes level 0 one window of the whole clip and every residue one window."""
    if isinstance(levels, bool) or not isinstance(levels, int) or levels < 1:
        raise PlannerError(f"context_stride {levels!r}: the number of stride levels must be an integer >= 1")
    if total <= 0 or world <= 0:
        raise PlannerError("num_frames and world size must be positive")
    if levels > 1 and (1 << levels) > total:
        raise PlannerError(f"context_stride {levels}: stride {1 << (levels - 1)} leaves fewer than two frames per window "
                           f"in a clip of {total}")
    from .planner import plan
    base = plan(total, world, chunk_size, overlap, no_chunking, overlap_rule)
    size, ov = base.chunk, base.overlap
    wins = [(s, e - s, 1) for s, e in base.ranges]
    for l in range(1, levels):
        d = 1 << l
        for r in range(d):
            n_r = -(-(total - r) // d)
            L = min(size, n_r)
            wins += [(r + d * s, L, d) for s in tile_starts(n_r, L, min(ov, L - 1))]
    if len(wins) % world:
        wins += [wins[-1]] * (world - len(wins) % world)
    return StridePlan(max(L for _, L, _ in wins), ov, tuple(wins), world, levels, base)


def stride_plan_of(cfg, world: int) -> StridePlan:
    """`stride_plan` of a job's config."""
    return stride_plan(cfg.num_frames, world, cfg.chunk_size, cfg.overlap, cfg.overlap_rule, cfg.context_stride, cfg.no_chunking)


def stride_table(sp: StridePlan, T: int) -> StrideTable:
    """`_fuse_table` of a strided plan's windows `(s, L, d)`: every level has the share `1 / levels` of every frame's noise.  With
    one level that is `window_table`'s table, bit for bit."""
    return _fuse_table(plan_windows(sp), T, sp.overlap, "stride_table")


# ---- spatial tiles (MultiDiffusion's original form; csrc/cotile.hip) ------------------------------------------------------------
def tile_starts(n: int, tile: int, overlap: int) -> List[int]:
    """First cells of the tiles of `tile` cells that cover `n` cells: 0, tile - overlap, 2 (tile - overlap), ..., the last one
    moved back so that its tile ends at `n` (all tiles have ONE size, so every UNet call and every slot of the packed buffer has
    one shape); a start the move repeats is dropped.  `n == tile` gives [0]."""
    if not 1 <= tile <= n or not 0 <= overlap < tile:
        raise ValueError(f"tile_starts: a tile of {tile} cells (overlap {overlap}) for {n} cells: need 1 <= tile <= n, 0 <= overlap < tile")
    starts, step = [], tile - overlap
    for s in range(0, n, step):
        s = min(s, n - tile)
        if not starts or s != starts[-1]:
            starts.append(s)
        if s == n - tile:
            break
    return starts


def axis_weights(n: int, tile: int, overlap: int, starts: List[int]) -> torch.Tensor:
    """fp32 (len(starts), n): `fuse_weights(tile, overlap)` of every tile along one axis, normalised over the tiles that cover a
    cell in float64 and rounded to fp32 once, exactly as `window_table` does along time: zero outside a tile, exactly 1.0 where
    one tile covers a cell.  A cell in no tile is a `ValueError`."""
    raw = np.zeros((len(starts), n), dtype=np.float64)
    for k, s in enumerate(starts):
        if not 0 <= s <= n - tile:
            raise ValueError(f"axis_weights: tile {k} = [{s}, {s + tile}) leaves the {n} cells")
        raw[k, s:s + tile] = fuse_weights(tile, overlap)
    total = raw.sum(axis=0)
    if (total <= 0).any():
        raise ValueError(f"axis_weights: cell {int(np.argmin(total > 0))} is in no tile")
    return torch.from_numpy((raw / total).astype(np.float32))


@dataclass(frozen=True)
class TilePlan:
    """The spatial windows of a tiled job, in latent cells: tiles of `th` x `tw` at rows `ys` and columns `xs` (the windows are the
    Cartesian product time x `ys` x `xs`, fused in ascending (kt, ky, kx)), and the per-axis normalised weights `wyn` (ny, h),
    `wxn` (nx, w): the product of three weights that are each normalised is normalised."""
    th: int
    tw: int
    oy: int
    ox: int
    ys: Tuple[int, ...]
    xs: Tuple[int, ...]
    wyn: torch.Tensor
    wxn: torch.Tensor

    @property
    def count(self) -> int:
        return len(self.ys) * len(self.xs)

    @property
    def boxes(self) -> List[Tuple[int, int, int, int]]:
        """(y0, th, x0, tw) per tile, in the order of the packed buffer's slots: ky-major."""
        return [(y, self.th, x, self.tw) for y in self.ys for x in self.xs]

    def grid(self, stride: int, device) -> "ops.TileGrid":
        return ops.TileGrid(stride, self.ys, self.xs, self.th, self.tw, self.wyn.to(device), self.wxn.to(device))

    def record(self, time_windows: int) -> dict:
        return {"tile": [self.th, self.tw], "overlap": [self.oy, self.ox], "grid": [len(self.ys), len(self.xs)],
                "windows": time_windows * self.count}


def tile_plan(h: int, w: int, th: int, tw: int, oy: int, ox: int) -> TilePlan:
    """The tiles of a `h` x `w` latent frame (everything in latent cells); more than `ops.COTILE_MAX_TILES` is a `ValueError`."""
    ys, xs = tile_starts(h, th, oy), tile_starts(w, tw, ox)
    if len(ys) * len(xs) > ops.COTILE_MAX_TILES:
        raise ValueError(f"tile_plan: {len(ys)} x {len(xs)} tiles, the fused step takes {ops.COTILE_MAX_TILES}")
    return TilePlan(th, tw, oy, ox, tuple(ys), tuple(xs), axis_weights(h, th, oy, ys), axis_weights(w, tw, ox, xs))


# kind of round -> (`ops`' input op, the range it takes of a `Window`, the scheduler's step method, the name in a table's errors)
_KINDS = {"flat": ("cfg_input_window", lambda w: (w.s, w.s + w.L), "step_cfg_windows", "window_table"),
          "tiles": ("cfg_input_tile", lambda w: (w.s, w.s + w.L), "step_cfg_tiles", "window_table"),
          "ring": ("cfg_input_loop", lambda w: (w.s, w.L), "step_cfg_loop", "loop_table"),
          "strided": ("cfg_input_stride", lambda w: (w.s, w.L, w.d), "step_cfg_strided", "stride_table")}


def co_denoise_round(d, start: torch.Tensor, cp: ChunkPlan, tiles: Optional[TilePlan] = None, strided: Optional[StridePlan] = None):
    """One co-denoised sampling round of `d` (a `DistributedVideoDiffuser`) from the whole clip's start latent -> (z.float(),
    the round's seconds and bytes under `info`'s names, the `info["co_denoise"]` record).  The plan is `strided` (a `StridePlan`
    of more than one level) where given, else `cp`, a `loop_plan` with `cfg.loop`; a window is its `Window` (s, L, d, ring)
    throughout, and `_KINDS` names the input op, the scheduler's method and the `_fuse_table` name of the four kinds.  Per step:
    this rank's windows go through the input op -> UNet into one packed buffer `[per_rank][2][C][chunk][h][w]` (a window shorter
    than the chunk, the plan's longest, fills the front of its slot; the rest is never read); with more than one rank, one
    `all_gather_into_tensor` of that buffer; then every rank runs the fused step on its own copy of z (identical bits on every
    rank: no broadcast; with `guidance_rescale` the step's statistic is taken over that same gathered buffer, so every rank gets
    the same r), and the mask step on the whole clip.  There is no final blend, so the zeroed first and last frame of the
    reference's ramp blend does not occur.
    `tiles` (a `TilePlan`): every window is run once per tile, on the tile's crop of z (and of the whole frame's ctx), into
    `tiles.count` consecutive slots of the packed buffer `[per_rank][ny nx][2][C][chunk][th][tw]`.
    The record gains `"tile"`, `"loop"` (the fused windows as [s, L]) and `"context_stride"` (the levels, their strides and the
    fused windows as [s, L, d]) with their options.
    `d.travel` (prompt travel, vdx/travel.py): every window is called with its own text, `d.window_text` of it, built once; every
    tile of a window shares it.  `d.regions` (regional prompts, vdx/region.py): a window's UNet call gains `d.region_kw` of it."""
    from .pipeline import emu_gather_delay_s
    cfg, sched = d.cfg, d.scheduler
    _, C, T, H, W = start.shape
    loop, plan, world = bool(cfg.loop), cp if strided is None else strided, d.world
    kind = "strided" if strided is not None else "ring" if loop else "flat" if tiles is None else "tiles"
    input_name, takes, step_name, table_name = _KINDS[kind]      # the window's UNet input and the step, decided once per round
    table = _fuse_table(plan_windows(plan, loop), T, plan.overlap, table_name)
    spans, chunk, per = rank_windows(plan, d.rank, loop)
    boxes = [()] if tiles is None else tiles.boxes                # (): the whole frame, as always
    nt = len(boxes)
    area = H * W if tiles is None else tiles.th * tiles.tw
    slot = 2 * C * chunk * area
    rows = table.rows(world, per, nt * slot)
    wn = table.wn.to(start.device)
    local = torch.zeros((per, nt * slot), dtype=torch.float16, device=start.device)
    packed = torch.zeros((world, per, nt * slot), dtype=torch.float16, device=start.device) if world > 1 else local
    payload_step = sum(w.L * C * 2 for w in spans)                # the reference's formula (:194), per exchange
    actual_step = sum(2 * C * w.L * area * nt * 2 for w in spans)
    bytes_step = (world - 1) * per * nt * slot * 2
    z = start.clone()
    reset = getattr(sched, "reset", None)
    if reset is not None:                                         # ONE x0 history for the whole clip, fresh per round
        reset()
    spent = {"denoise_s": 0.0, "emu_gather_delay_s": 0.0, "net_gather_s": 0.0, "network_bytes": 0, "payload_bytes": 0,
             "payload_bytes_actual": 0}
    input_op, ranges = getattr(ops, input_name), [takes(w) for w in spans]     # the op with the range it takes of a window
    step, head = getattr(sched, step_name), (packed, rows, wn) if tiles is None else (packed, rows, wn, tiles.grid(slot, start.device))
    step_kw = d._rescale_kw if kind == "flat" else {}             # the other kinds have no rescaled or thresholded form
    # prompt travel: every window has its own text (every tile of a window shares it), built once; else the one text of the job
    texts = [torch.cat([d.uncond_emb, d.cond_emb], dim=0)] * len(spans) if d.travel is None else [d.window_text(*w) for w in spans]
    # regional prompts: every window's UNet call gains the plan and the window's place in the clip ({} when off; never with tiles)
    region_kws = [{}] * len(spans) if getattr(d, "regions", None) is None else [d.region_kw(*w) for w in spans]
    t_round = time.time()
    for i, t in enumerate(d.schedule):
        for j, span in enumerate(ranges):
            for k, box in enumerate(boxes):
                noise = d.unet(input_op(z, d.ctx, cfg.context_weight, *span, *box), t, encoder_hidden_states=texts[j], **region_kws[j]).sample
                local[j, k * slot:k * slot + noise.numel()].copy_(noise.reshape(-1))
        delay = emu_gather_delay_s(payload_step, cfg)             # per step: one exchange per step is what the method costs
        if delay > 0:
            d._sync()
            time.sleep(delay)
            spent["emu_gather_delay_s"] += delay
        if world > 1:
            d._sync()
            t0 = time.time()
            dist.all_gather_into_tensor(packed.view(-1), local.view(-1))
            d._sync()
            spent["net_gather_s"] += time.time() - t0
        z = step(*head, t, z, cfg.guidance_scale, **step_kw)
        if d.latent_mask is not None:                             # masked video-to-video (vdx/inpaint.py): the whole clip, s = 0
            d._mask_step(z, i, 0)
        spent["network_bytes"] += bytes_step
        spent["payload_bytes"] += payload_step
        spent["payload_bytes_actual"] += actual_step
    if world > 1:
        dist.barrier()
    d._sync()
    spent["denoise_s"] = time.time() - t_round - spent["net_gather_s"] - spent["emu_gather_delay_s"]
    rec = {"windows": len(table.fused), "steps": len(d.schedule), "exchange_s": spent["net_gather_s"], "bytes_per_step": bytes_step}
    if tiles is not None:
        rec["tile"] = tiles.record(len(table.fused))
    if loop:
        rec["loop"] = {"windows": [[s, L] for _, s, L, _ in table.fused]}
    if strided is not None:
        rec["context_stride"] = {"levels": strided.levels, "strides": strided.strides, "windows": [list(w[1:]) for w in table.fused]}
    return z.float(), spent, rec
