"""CPU: the host side of strided context windows (vdx/codenoise.py `stride_plan`, `stride_table`, `check_stride`; the flag) and
the restatement of tests/costride_ref.py against tests/codenoise_ref.py, which it must reduce to when every stride is 1."""
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
import costride_ref as S  # noqa: E402
import dpm_ref  # noqa: E402
from vdx.codenoise import StridePlan, check_stride, fuse_weights, stride_plan, stride_table, window_table  # noqa: E402
from vdx.planner import ChunkPlan, PlannerError, plan  # noqa: E402

TOTALS, LEVELS, WORLDS = (4, 5, 8, 24, 33, 64), (1, 2, 3), (1, 2, 3)
SETTINGS = ((0, 4), (4, 2), (16, 8), (3, 1), (6, 2))                 # (chunk_size, overlap), the "coherent" rule: overlap >= 1


def _frames(s, L, d):
    return [s + f * d for f in range(L)]


def _plans():
    for T in TOTALS:
        for levels in LEVELS:
            for world in WORLDS:
                for chunk, ov in SETTINGS:
                    yield T, levels, world, chunk, ov


def test_the_plan_over_a_sweep():
    """Either level 0 is refused by the planner itself, or the deepest level would hold fewer than two frames per window, or
    the plan has every stated property."""
    planned = refused = 0
    for T, levels, world, chunk, ov in _plans():
        try:
            base = plan(T, world, chunk, ov)
        except PlannerError:
            with pytest.raises(PlannerError):
                stride_plan(T, world, chunk, ov, "coherent", levels)
            refused += 1
            continue
        if levels > 1 and 2 ** levels > T:
            with pytest.raises(PlannerError, match="fewer than two frames"):
                stride_plan(T, world, chunk, ov, "coherent", levels)
            refused += 1
            continue
        sp = stride_plan(T, world, chunk, ov, "coherent", levels)
        planned += 1
        what = (T, levels, world, chunk, ov)
        assert isinstance(sp, StridePlan) and sp.levels == levels and sp.strides == [2 ** l for l in range(levels)], what
        assert len(sp.windows) % world == 0 and sp.per_rank * world == len(sp.windows), what
        assert sp.base == base and sp.overlap == base.overlap and sp.chunk == max(L for _, L, _ in sp.windows), what
        for s, L, d in sp.windows:                                   # every window inside the clip
            assert d in sp.strides and L >= 1 and 0 <= s and s + (L - 1) * d < T, what
        # level 0 is the planner's plan, in its order, in front
        assert list(sp.windows[:len(base.ranges)]) == [(s, e - s, 1) for s, e in base.ranges], what
        fused = list(dict.fromkeys(sp.windows))                      # first occurrences, in order
        assert [w for w in fused if w[2] == 1] == list(dict.fromkeys((s, e - s, 1) for s, e in base.ranges)), what
        # ascending levels, residues, starts; one length per (level, residue)
        deeper = [w for w in fused if w[2] > 1]
        assert deeper == sorted(deeper, key=lambda w: (w[2], w[0] % w[2], w[0])), what
        lengths = {}
        for s, L, d in deeper:
            lengths.setdefault((d, s % d), set()).add(L)
        assert all(len(v) == 1 for v in lengths.values()), what
        assert set(lengths) == {(d, r) for d in sp.strides[1:] for r in range(d)}, what
        for (d, r), (L,) in ((k, tuple(v)) for k, v in lengths.items()):
            assert L == min(base.chunk, -(-(T - r) // d)), what
        # the padding repeats the last window
        pad = len(sp.windows) - len(base.ranges) - len(deeper)
        assert 0 <= pad < world and all(w == sp.windows[-1] for w in sp.windows[len(sp.windows) - pad:]), what
        # the pair property: t and t + d lie together in some window of stride d
        for d in sp.strides:
            held = [set(_frames(*w)) for w in fused if w[2] == d]
            for t in range(T - d):
                assert any(t in h and t + d in h for h in held), (what, d, t)
            assert set().union(*held) == set(range(T)), what       # and every frame is in some window of every level
        # rank shares
        assert sorted(w for r in range(world) for w in sp.for_rank(r)) == sorted(sp.windows), what
    assert planned > 150 and refused > 20


def test_one_level_is_the_planners_plan_and_window_table_bit_for_bit():
    for T in TOTALS:
        for world in WORLDS:
            for chunk, ov in SETTINGS:
                try:
                    base = plan(T, world, chunk, ov)
                except PlannerError:
                    continue
                sp = stride_plan(T, world, chunk, ov, "coherent", 1)
                assert list(sp.windows) == [(s, e - s, 1) for s, e in base.ranges] and sp.chunk <= base.chunk
                st, wt = stride_table(sp, T), window_table(base, T)
                assert st.wn.dtype == torch.float32 and torch.equal(st.wn.view(torch.int32), wt.wn.view(torch.int32))
                assert [(i, s, s + L) for i, s, L, _ in st.fused] == list(wt.fused)
                assert [r[:3] for r in st.rows(world, sp.per_rank, 1000)] == wt.rows(world, base.per_rank, 1000)
                assert all(r[3] == 1 for r in st.rows(world, sp.per_rank, 1000))
    sp = stride_plan(8, 1, 8, 0, "coherent", 1, no_chunking=True)     # mode "fsdp": one window of the whole clip
    assert sp.windows == ((0, 8, 1),)
    sp = stride_plan(8, 1, 8, 0, "coherent", 2, no_chunking=True)     # and every residue one window
    assert sp.windows == ((0, 8, 1), (0, 4, 2), (1, 4, 2))


def test_the_default_job_and_hand_checked_plans():
    # 24 frames, chunk 16, overlap 8 on two ranks (the planner grows the chunk to 20 for an even count): 32 + 24 = 56 window-frames
    sp = stride_plan(24, 2, 16, 8, "coherent", 2)
    assert sp.windows == ((0, 20, 1), (12, 12, 1), (0, 12, 2), (1, 12, 2)) and sum(L for _, L, _ in sp.windows) == 56
    sp = stride_plan(24, 1, 16, 8, "coherent", 2)                     # on one rank the planner's three windows stay
    assert sp.windows == ((0, 16, 1), (8, 16, 1), (16, 8, 1), (0, 12, 2), (1, 12, 2))
    sp = stride_plan(33, 3, 8, 2, "coherent", 2)
    # level 0 by the planner; d = 2: residue 0 has 17 frames -> starts 0, 6, 9 (moved back); residue 1 has 16 -> 0, 6, 8
    assert [w for w in sp.windows if w[2] == 2][:6] == [(0, 8, 2), (12, 8, 2), (18, 8, 2), (1, 8, 2), (13, 8, 2), (17, 8, 2)]
    assert len(sp.windows) % 3 == 0
    sp = stride_plan(5, 2, 4, 2, "coherent", 2)
    assert sp.windows == ((0, 5, 1), (3, 2, 1), (0, 3, 2), (1, 2, 2))   # the planner grew the chunk to 5 for two ranks


def test_the_table_columns_and_level_shares():
    """Every column sums to 1 and every level's part of it to 1/levels, within one fp32 rounding per term: a term w rounded to
    fp32 is off by at most 2^-24 w, so a sum of terms is off by at most 2^-24 times itself (the sums are taken in float64)."""
    checked = 0
    for T, levels, world, chunk, ov in _plans():
        try:
            sp = stride_plan(T, world, chunk, ov, "coherent", levels)
        except PlannerError:
            continue
        if len(set(sp.windows)) > 64:                                # more than the fused step takes: refused, not truncated
            with pytest.raises(ValueError, match="64"):
                stride_table(sp, T)
            continue
        st = stride_table(sp, T)
        assert len(st.fused) == len(set(sp.windows)) and tuple(st.wn.shape) == (len(st.fused), T)
        wn = st.wn.double().numpy()
        inside = np.zeros_like(wn, dtype=bool)
        for k, (_, s, L, d) in enumerate(st.fused):
            inside[k, _frames(s, L, d)] = True
        assert (wn[inside] > 0).all() and (wn[~inside] == 0).all()
        col = wn.sum(axis=0)
        assert (np.abs(col - 1.0) <= 2.0 ** -24 * col + 1e-15).all(), (T, levels, world, chunk, ov)
        for d in sp.strides:
            part = wn[[w[3] == d for w in st.fused]].sum(axis=0)
            assert (np.abs(part - 1.0 / levels) <= 2.0 ** -24 * part + 1e-15).all(), (T, levels, world, chunk, ov, d)
        checked += 1
    assert checked > 150
    # by hand: T = 3, d = 2 windows {0, 2} and {1} and one d = 1 window of the clip; overlap 1
    sp = StridePlan(3, 1, ((0, 3, 1), (0, 2, 2), (1, 1, 2)), 1, 2, ChunkPlan(3, 1, ((0, 3),), 1))
    st = stride_table(sp, 3)
    assert torch.equal(st.wn, torch.tensor([[0.5, 0.5, 0.5], [0.5, 0.0, 0.5], [0.0, 0.5, 0.0]]))
    assert st.rows(1, 3, 100) == [(0, 0, 3, 1), (100, 0, 2, 2), (200, 1, 1, 2)]
    # raw weights are fuse_weights at the window's frames, normalised per level
    sp = stride_plan(8, 1, 4, 2, "coherent", 2)
    st = stride_table(sp, 8)
    k = [w[1:] for w in st.fused].index((0, 4, 2))
    raw = np.zeros((2, 4))
    raw[0] = fuse_weights(4, 2)
    assert [w[1:] for w in st.fused if w[3] == 2] == [(0, 4, 2), (1, 4, 2)]        # one window per residue: normalised to 1, halved
    assert torch.equal(st.wn[k, 0::2], torch.full((4,), 0.5)) and not bool(st.wn[k, 1::2].any())


def test_tables_the_fused_step_cannot_take():
    base = ChunkPlan(1, 0, tuple((t, t + 1) for t in range(70)), 1)
    with pytest.raises(ValueError, match="64"):
        stride_table(StridePlan(1, 0, tuple((t, 1, 1) for t in range(70)), 1, 1, base), 70)
    with pytest.raises(ValueError, match="leaves"):
        stride_table(StridePlan(4, 1, ((0, 4, 2),), 1, 1, base), 6)    # 0 + 3 * 2 = 6 is past the last of 6 frames
    with pytest.raises(ValueError, match="no window of stride 2"):
        stride_table(StridePlan(4, 1, ((0, 4, 1), (0, 2, 2)), 1, 2, base), 4)


def _cfg(**kw):
    from vdx.pipeline import DiffuserConfig
    return DiffuserConfig(**{**dict(num_frames=8, steps=2, chunk_size=6, overlap=2, height=64, width=64, mode="chunk", device="cpu",
                                    co_denoise=True, context_stride=2), **kw})


REFUSALS = [(dict(co_denoise=False), "allgather", "needs co_denoise"), (dict(), "halo", "allgather"),
            (dict(tile=(64, 64)), "allgather", "tile"), (dict(loop=True), "allgather", "loop"),
            (dict(guidance_rescale=0.5), "allgather", "guidance_rescale"),
            (dict(context_stride=0), "allgather", ">= 1"), (dict(context_stride=-2), "allgather", ">= 1"),
            (dict(context_stride=4), "allgather", "fewer than two frames"),
            (dict(num_frames=3, chunk_size=2, overlap=1), "allgather", "fewer than two frames"),
            (dict(overlap=6), "allgather", "never advance"),
            (dict(num_frames=200, chunk_size=3, overlap=1), "allgather", "64")]


def test_refused_before_anything_loads():
    from vdx.pipeline import DistributedVideoDiffuser, run_job
    from vdx.scheduler import DDIMScheduler
    assert check_stride(_cfg()) == 2 and check_stride(_cfg(context_stride=1, co_denoise=False), "halo") == 1
    assert check_stride(_cfg(mode="fsdp")) == 2                       # level 0 is then one window
    for kw, exchange, match in REFUSALS:
        with pytest.raises(ValueError, match=match):
            check_stride(_cfg(**kw), exchange, 1)
        with pytest.raises(ValueError, match=match):
            run_job(_cfg(**kw), exchange=exchange, out_video=None)   # before any model is loaded: needs no GPU
    unet = SimpleNamespace(config=SimpleNamespace(in_channels=4))     # never called
    for kw, exchange, match in ((dict(context_stride=4), "allgather", "fewer than two frames"), (dict(), "halo", "allgather"),
                                (dict(co_denoise=False), "allgather", "needs co_denoise"), (dict(loop=True), "allgather", "loop")):
        d = DistributedVideoDiffuser(_cfg(**kw), unet, DDIMScheduler(), None, None)
        with pytest.raises(ValueError, match=match):
            d(exchange=exchange)
    for levels in (1, 2):                                             # the job's plan, `info["ranges"]`, stays level 0
        d = DistributedVideoDiffuser(_cfg(context_stride=levels), unet, DDIMScheduler(), None, None)
        assert d.plan().ranges == ((0, 6), (4, 8))
    with pytest.raises(PlannerError, match=">= 1"):
        stride_plan(8, 1, 6, 2, "coherent", 0)
    with pytest.raises(PlannerError, match="fewer than two frames"):
        stride_plan(3, 1, 2, 1, "coherent", 2)
    assert stride_plan(4, 1, 4, 0, "coherent", 2, no_chunking=True).windows == ((0, 4, 1), (0, 2, 2), (1, 2, 2))


def test_the_flag_round_trips_and_is_off_by_default():
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args
    p = build_arg_parser()
    assert DiffuserConfig().context_stride == 1 and config_from_args(p.parse_args(["--co_denoise"])).context_stride == 1
    on = config_from_args(p.parse_args(["--co_denoise", "--context_stride", "2", "--num_frames", "24", "--chunk_size", "16"]))
    assert on.context_stride == 2 and on.co_denoise is True and check_stride(on) == 2
    off = config_from_args(p.parse_args(["--co_denoise", "--num_frames", "24", "--chunk_size", "16"]))
    on.context_stride = 1
    assert on == off


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
def _case(T, table, seed=1, C=4, h=3, w=5):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(1, C, T, h, w, generator=g).half()
    prev = torch.randn(1, C, T, h, w, generator=g).half()
    wins = [torch.randn(2, C, L, h, w, generator=g).half() for _, L, _ in table]
    return z, prev, wins


def _wn(table, T, ov):
    base = ChunkPlan(max(L for _, L, _ in table), ov, ((0, T),), 1)
    return stride_table(StridePlan(base.chunk, ov, tuple(table), 1, len({d for _, _, d in table}), base), T).wn


def test_with_every_stride_one_the_restatement_is_codenoise_refs():
    T, table = 8, [(0, 4, 1), (2, 4, 1), (4, 4, 1)]
    z, prev, wins = _case(T, table)
    wn = _wn(table, T, 2)
    flat = [(s, L) for s, L, _ in table]
    assert torch.equal(S.fuse(wins, table, wn, z.shape).view(torch.int16), R.fuse(wins, flat, wn, z.shape).view(torch.int16))
    coeffs = (0.6, 0.8, 0.9, 0.43)
    assert torch.equal(S.costride_ddim(z, wins, table, wn, 7.5, coeffs), R.cofuse_ddim(z, wins, flat, wn, 7.5, coeffs))
    for i, second in ((0, False), (2, True)):
        k = dpm_ref.scalars(dpm_ref.sigmas(6), i, second)
        got, want = S.costride_dpm(z, wins, table, wn, 7.5, k, prev if second else None), R.cofuse_dpm(z, wins, flat, wn, 7.5, k, prev if second else None)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ctx = torch.randn(1, 4, 1, 3, 5, generator=torch.Generator().manual_seed(2)).half()
    assert torch.equal(S.cfg_input_stride(z, ctx, 0.35, 2, 4, 1), R.cfg_input_window(z, ctx, 0.35, 2, 6))
    assert torch.equal(S.cfg_input_stride(z, None, 0.0, 1, 3, 3)[0], z[0, :, [1, 4, 7]])


def test_the_restatement_by_permutation():
    """A table of d = 2 windows only on an even clip is a flat table on the clip permuted to evens-then-odds."""
    T, ov = 8, 1
    table = [(0, 3, 2), (2, 3, 2), (1, 4, 2)]                         # evens 0 2 4 | 2 4 6, odds 1 3 5 7
    z, prev, wins = _case(T, table, seed=3)
    wn = _wn(table, T, ov)
    perm = torch.tensor([0, 2, 4, 6, 1, 3, 5, 7])
    flat = [(0, 3), (1, 3), (4, 4)]                                   # the same windows in permuted positions
    got = S.fuse(wins, table, wn, z.shape)
    want = R.fuse(wins, flat, wn[:, perm], z.shape)
    assert torch.equal(got[:, :, perm].view(torch.int16), want.view(torch.int16))
    with pytest.raises(ValueError, match="no window"):
        S.fuse(wins[:2], table[:2], wn[:2], z.shape)
