"""CPU: the host side of seamless looping (vdx/codenoise.py `loop_plan`, `loop_table`, `check_loop`; the flag; the small helpers
of vdx/interp.py and vdx/metrics.py) and the restatement of tests/coloop_ref.py against tests/codenoise_ref.py, which it must
reduce to when no window wraps."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import vdx  # noqa: E402,F401
import codenoise_ref as R  # noqa: E402
import coloop_ref as L  # noqa: E402
from vdx.codenoise import check_loop, fuse_weights, loop_plan, loop_table, window_table  # noqa: E402
from vdx.planner import ChunkPlan, PlannerError, auto_chunk  # noqa: E402


def _size_ov(total, world, chunk, overlap, rule):
    """The planner's own rules (vdx/planner.py `plan`), restated."""
    size = chunk if chunk > 0 else auto_chunk(total, world)
    return size, (overlap if overlap > 0 else max(4, size // 3)) if rule == "coherent" else min(overlap, size // 3)


def _frames(s, e, T):
    return {(s + f) % T for f in range(e - s)}


def test_the_ring_plan_over_a_sweep():
    """total 2..64 x chunk x overlap x world 1..8 (x both overlap rules): either one of the two stated refusals (or no overlap),
    or a plan with every stated property."""
    planned = refused = 0
    for total in range(2, 65):
        for world in range(1, 9):
            for chunk in (0, 2, 3, 4, 6, 8, 16, 24):
                for overlap, rule in ((0, "coherent"), (1, "coherent"), (2, "coherent"), (4, "coherent"), (8, "coherent"),
                                      (1, "third"), (4, "third")):
                    size, ov = _size_ov(total, world, chunk, overlap, rule)
                    step = size - ov
                    n = world * -(-(-(-total // step)) // world) if step > 0 else None
                    if size >= total or ov < 1 or step <= 0 or n > total:
                        with pytest.raises(PlannerError):
                            loop_plan(total, world, chunk, overlap, rule)
                        refused += 1
                        continue
                    cp = loop_plan(total, world, chunk, overlap, rule)
                    planned += 1
                    starts = [s for s, _ in cp.ranges]
                    assert (cp.chunk, cp.overlap, cp.world, len(cp.ranges)) == (size, ov, world, n)
                    assert all(e - s == size for s, e in cp.ranges)                    # ONE length: no short tail, no repeat
                    assert starts == sorted(set(starts)) and starts[0] == 0 and starts[-1] < total
                    assert starts == [(i * total) // n for i in range(n)]
                    assert len(cp.ranges) % world == 0 and len(cp.for_rank(world - 1)) == cp.per_rank
                    held = [_frames(s, e, total) for s, e in cp.ranges]
                    assert set().union(*held) == set(range(total))                     # every frame is covered
                    for i in range(n):                                                 # cyclic neighbours share >= ov frames
                        gap = (starts[(i + 1) % n] - starts[i]) % total
                        assert 1 <= gap <= step
                        assert len(held[i] & held[(i + 1) % n]) >= ov
                    for t in range(total):                                             # every (t, t+1 mod T) in a common window
                        assert any(t in h and (t + 1) % total in h for h in held)
    assert planned > 1000 and refused > 1000


def test_the_two_refusals_and_the_default_job():
    assert loop_plan(24, 1, 16, 4).ranges == ((0, 16), (12, 28))                       # Zeroscope's default: 24 frames, chunk 16
    assert loop_plan(24, 2, 16, 4).ranges == ((0, 16), (12, 28))
    assert loop_plan(8, 1, 6, 2).ranges == loop_plan(8, 2, 6, 2).ranges == ((0, 6), (4, 10))
    assert loop_plan(10, 3, 4, 1).ranges == ((0, 4), (1, 5), (3, 7), (5, 9), (6, 10), (8, 12))
    with pytest.raises(PlannerError, match="line, not a ring"):
        loop_plan(16, 1, 16, 4)                                                        # size == total
    with pytest.raises(PlannerError, match="line, not a ring"):
        loop_plan(8, 1, 16, 4)                                                         # size > total
    with pytest.raises(PlannerError, match="distinct"):
        loop_plan(5, 4, 3, 2)                                                          # step 1: ceil(5/1) = 5 -> n = 8 > 5
    with pytest.raises(PlannerError, match="share at least one frame"):
        loop_plan(24, 1, 2, 4, "third")                                                # min(4, 2 // 3) = 0
    with pytest.raises(PlannerError):
        loop_plan(24, 1, 4, 4)                                                         # overlap >= chunk
    with pytest.raises(PlannerError):
        loop_plan(24, 1, 16, 4, "nonsense")


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("T,world,chunk,ov", [(24, 1, 16, 4), (8, 1, 6, 2), (8, 2, 6, 2), (10, 3, 4, 1), (7, 1, 4, 3), (32, 4, 0, 4),
                                              (17, 3, 6, 2), (9, 1, 5, 4), (64, 8, 3, 2)])
def test_table_of_a_ring_plan(T, world, chunk, ov):
    cp = loop_plan(T, world, chunk, ov)
    tab = loop_table(cp, T)
    wn = tab.wn
    assert wn.dtype == torch.float32 and tuple(wn.shape) == (len(cp.ranges), T)
    assert tab.fused == tuple((i, s, e) for i, (s, e) in enumerate(cp.ranges))         # every window, plan order
    num = [min(j + 1, cp.chunk - j, cp.overlap + 1) for j in range(cp.chunk)]          # fuse_weights' numerators: integers
    assert fuse_weights(cp.chunk, cp.overlap) == [v / (cp.overlap + 1) for v in num]
    cover = torch.zeros(T, dtype=torch.int64)
    for k, (s, e) in enumerate(cp.ranges):
        inside = torch.zeros(T, dtype=torch.bool)
        inside[list(_frames(s, e, T))] = True
        assert bool((wn[k][inside] > 0).all()) and float(wn[k][~inside].abs().sum()) == 0
        cover += inside
    for t in range(T):
        col = wn[:, t]
        total = sum(num[(t - s) % T] for s, e in cp.ranges if (t - s) % T < e - s)
        for k, (s, e) in enumerate(cp.ranges):                                         # the exact quotient, rounded (once) to fp32
            f = (t - s) % T
            exact = num[f] / total if f < e - s else 0.0
            assert abs(float(col[k]) - exact) <= _ulp32(exact) / 2 * (1 + 2.0 ** -20) and (float(col[k]) > 0) == (f < e - s)
        if cover[t] == 1:
            assert float(col.max()) == 1.0 and int((col != 0).sum()) == 1              # exactly 1.0f, not nearly
        # each entry is a float64 quotient rounded once to fp32: within one fp32 ulp (of a value <= 1) per term
        assert abs(float(col.double().sum()) - 1.0) <= int(cover[t]) * _ulp32(1.0)
    assert bool((cover >= 1).all()) and int(cover.max()) >= 2
    # rows(): (offset, first frame, length), window i at rank i % world, slot i // world
    rows = tab.rows(world, cp.per_rank, 100)
    assert rows == [(((i % world) * cp.per_rank + i // world) * 100, s, cp.chunk) for i, (s, _) in enumerate(cp.ranges)]


def test_table_refusals_and_a_plan_that_does_not_wrap():
    with pytest.raises(ValueError, match="no ring window"):
        loop_table(ChunkPlan(4, 1, ((0, 4), (8, 12)), 1), 8)                           # s = T
    with pytest.raises(ValueError, match="no ring window"):
        loop_table(ChunkPlan(9, 1, ((0, 9),), 1), 8)                                   # L > T
    with pytest.raises(ValueError, match="frame 4 is in no window"):
        loop_table(ChunkPlan(4, 1, ((0, 4), (5, 9)), 1), 8)                            # frames 0..3 and 5, 6, 7, 0
    with pytest.raises(ValueError, match="64"):
        loop_table(ChunkPlan(2, 1, tuple((i, i + 2) for i in range(65)), 1), 66)
    flat = ChunkPlan(4, 3, ((0, 4), (1, 5), (2, 6), (3, 7)), 1)                         # nothing wraps: window_table's weights
    assert torch.equal(loop_table(flat, 7).wn, window_table(flat, 7).wn)


def _cfg(**kw):
    from vdx.pipeline import DiffuserConfig
    return DiffuserConfig(**{**dict(num_frames=8, steps=2, chunk_size=6, overlap=2, height=64, width=64, mode="chunk", device="cpu",
                                    co_denoise=True, loop=True), **kw})


REFUSALS = [(dict(co_denoise=False), "allgather", "needs co_denoise"), (dict(), "halo", "allgather"),
            (dict(tile=(64, 64)), "allgather", "tile"), (dict(guidance_rescale=0.5), "allgather", "guidance_rescale"),
            (dict(mode="fsdp"), "allgather", "line, not a ring"), (dict(chunk_size=8), "allgather", "line, not a ring"),
            (dict(num_frames=5, chunk_size=3, overlap=2, world=4), "allgather", "distinct"),
            (dict(num_frames=200, chunk_size=3, overlap=1), "allgather", "64"),
            (dict(overlap=1, overlap_rule="third", chunk_size=2), "allgather", "share at least one frame")]


def test_refused_before_anything_loads():
    from vdx.pipeline import DistributedVideoDiffuser, run_job
    from vdx.scheduler import DDIMScheduler
    assert check_loop(_cfg()) is True and check_loop(_cfg(loop=False, co_denoise=False), "halo") is False
    for kw, exchange, match in REFUSALS:
        kw = dict(kw)
        world = kw.pop("world", 1)
        with pytest.raises(ValueError, match=match):
            check_loop(_cfg(**kw), exchange, world)
        if world == 1:
            with pytest.raises(ValueError, match=match):
                run_job(_cfg(**kw), exchange=exchange, out_video=None)                   # before any model is loaded: needs no GPU
    unet = SimpleNamespace(config=SimpleNamespace(in_channels=4))                         # never called
    for kw, exchange, match in ((dict(chunk_size=8), "allgather", "line, not a ring"), (dict(), "halo", "allgather"),
                                (dict(co_denoise=False), "allgather", "needs co_denoise")):
        d = DistributedVideoDiffuser(_cfg(**kw), unet, DDIMScheduler(), None, None)
        with pytest.raises(ValueError, match=match):
            d(exchange=exchange)
    d = DistributedVideoDiffuser(_cfg(), unet, DDIMScheduler(), None, None)
    assert d.plan().ranges == ((0, 6), (4, 10))
    assert DistributedVideoDiffuser(_cfg(loop=False), unet, DDIMScheduler(), None, None).plan().ranges == ((0, 6), (4, 8))


def test_the_flag_round_trips_and_is_off_by_default():
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args
    p = build_arg_parser()
    assert DiffuserConfig().loop is False and config_from_args(p.parse_args(["--co_denoise"])).loop is False
    on = config_from_args(p.parse_args(["--co_denoise", "--loop", "--num_frames", "24", "--chunk_size", "16"]))
    assert on.loop is True and on.co_denoise is True and check_loop(on) is True
    off = config_from_args(p.parse_args(["--co_denoise", "--num_frames", "24", "--chunk_size", "16"]))
    on.loop = False
    assert on == off


def test_output_frame_counts():
    from vdx.interp import n_output_frames
    for F in (1, 2, 8, 24):
        for N in (1, 2, 3, 8):
            assert n_output_frames(F, N, loop=True) == F * N
            assert n_output_frames(F, N) == n_output_frames(F, N, loop=False) == (F - 1) * N + 1


def test_loop_l1_on_a_hand_made_clip():
    from vdx.metrics import loop_l1
    levels = (0, 10, 30, 4)                                                            # |10-0|, |30-10|, |4-30| -> mean 56/3; wrap |4-0|
    clip = [np.full((4, 6, 3), v, dtype=np.uint8) for v in levels]
    wrap, mean = loop_l1(clip)
    assert wrap == 4.0 and mean == float(np.mean(np.array([10, 20, 26], dtype=np.float32)))
    clip[3][0, 0, 0] = 255                                                             # one byte of 72: uint8 must not wrap around
    wrap, _ = loop_l1(clip)
    assert wrap == float(np.float32((71 * 4 + 255) / 72))
    assert loop_l1(clip[:1]) == (None, None) and loop_l1([]) == (None, None)
    assert loop_l1(np.stack(clip))[0] == wrap                                          # an array of frames too


# ---- the restatement without a wrap is tests/codenoise_ref.py's -----------------------------------------------------------------
def test_restatement_without_a_wrap_is_the_plain_one_and_a_rotation_commutes():
    C, T, h, w = 2, 7, 2, 3
    ranges = [(0, 4), (1, 5), (2, 6), (3, 7)]
    table = [(s, e - s) for s, e in ranges]
    wn = window_table(ChunkPlan(4, 3, tuple(ranges), 1), T).wn
    g = torch.Generator().manual_seed(1)
    wins = [torch.randn(2, C, 4, h, w, generator=g).half() for _ in ranges]
    want = R.fuse(wins, table, wn, (1, C, T, h, w))
    assert torch.equal(L.fuse(wins, table, wn, (1, C, T, h, w)).view(torch.int16), want.view(torch.int16))
    for r in range(1, T):                                                              # the same windows, r frames on: the same clip, rolled
        rolled = L.fuse(wins, [((s + r) % T, n) for s, n in table], wn.roll(r, 1), (1, C, T, h, w))
        assert torch.equal(rolled.view(torch.int16), want.roll(r, 2).view(torch.int16))
    z = torch.randn(1, C, T, h, w, generator=g).half()
    assert torch.equal(L.take(z, 5, 4), torch.cat([z[:, :, 5:], z[:, :, :2]], dim=2))
    assert torch.equal(L.cfg_input_loop(z, None, 0.0, 2, 3), R.cfg_input_window(z, None, 0.0, 2, 5))
    with pytest.raises(ValueError, match="no window"):
        L.fuse(wins[:1], [(5, 4)], torch.ones(1, T), (1, C, T, h, w))
