"""CPU: the one fuse-table builder of vdx/codenoise.py behind `window_table`, `loop_table` and `stride_table`, and the one
whole-clip step launcher `ops._co_step` behind the fused steps' public wrappers, against tests/golden/cowin_tables.json, which
tests/golden/make_cowin_tables.py recorded from the three builders and the two launchers they replace: every table's `fused`,
`rows()` and weight bits, and every launch's argument tuple, exactly."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")) if p not in sys.path]

import vdx  # noqa: E402,F401
import make_cowin_tables as M  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "cowin_tables.json")) as f:
    GOLDEN = json.load(f)


def test_the_fixture_covers_the_sweep():
    kinds = [t["args"][4] for t in GOLDEN["tables"]]
    assert len(kinds) >= 100 and all(kinds.count(k) > 0 for k in M.KINDS)
    assert {tuple(t["args"]) for t in GOLDEN["tables"]} <= set(M.SWEEP) and len(set(map(str, GOLDEN["tables"]))) == len(kinds)
    assert sorted(GOLDEN["launches"]) == sorted(f"{stem}_cfg_{form}_step" for stem in ("cofuse", "coloop", "costride", "cotile")
                                                for form in ("ddim", "dpm"))


def test_every_recorded_table_is_rebuilt_exactly():
    for want in GOLDEN["tables"]:
        got = M.table_case(*want["args"])
        for field in ("fused", "rows", "sha256"):
            assert got[field] == want[field], (want["args"], field)


def test_what_the_sweep_left_out_is_still_refused():
    recorded = {tuple(t["args"]) for t in GOLDEN["tables"]}
    for case in M.SWEEP:
        if case not in recorded:
            with pytest.raises(ValueError):
                M.table_case(*case)


def test_co_step_hands_the_launch_the_recorded_arguments():
    from vdx import ops
    assert not hasattr(ops, "_co_ddim_step") and not hasattr(ops, "_co_dpm_step") and callable(ops._co_step)
    got = M.launches()
    assert sorted(got) == sorted(GOLDEN["launches"])
    for name, want in GOLDEN["launches"].items():
        assert got[name] == want, name


def test_only_a_flat_or_strided_plan_drops_a_repeated_window():
    """The planner's repeated tail and a strided plan's padding are denoised, not fused; a ring table takes what it is given (the
    hand-written 64-row tables of tests/test_coloop_gpu.py repeat windows and count on every one)."""
    import torch
    from vdx import codenoise as cn
    from vdx.planner import ChunkPlan
    twice = ChunkPlan(4, 1, ((0, 4), (3, 7), (3, 7)), 1)
    assert cn.window_table(twice, 7).fused == ((0, 0, 4), (1, 3, 7))
    assert cn.stride_table(cn.StridePlan(4, 1, ((0, 4, 1), (3, 4, 1), (3, 4, 1)), 1, 1, twice), 7).fused == ((0, 0, 4, 1), (1, 3, 4, 1))
    ring = cn.loop_table(twice, 7)
    assert ring.fused == ((0, 0, 4), (1, 3, 7), (2, 3, 7)) and torch.equal(ring.wn[1], ring.wn[2])
    assert torch.allclose(ring.wn.sum(dim=0), torch.ones(7), rtol=0, atol=1e-6) and ring.wn[1, 4].item() == 0.5


def test_a_window_is_one_row_whatever_the_plan():
    from vdx import codenoise as cn
    from vdx.planner import plan
    flat, ring, strided = plan(13, 2, 6, 2), cn.loop_plan(13, 2, 6, 2), cn.stride_plan(13, 2, 6, 2, levels=2)
    for p, is_ring in ((flat, False), (ring, True)):
        for rank in range(2):
            wins, chunk, per = cn.rank_windows(p, rank, is_ring)
            assert [(w.s, w.s + w.L) for w in wins] == p.for_rank(rank) and (chunk, per) == (p.chunk, p.per_rank)
            assert all(w.d == 1 and w.ring is is_ring for w in wins)
    for rank in range(2):
        wins, chunk, per = cn.rank_windows(strided, rank)
        assert [tuple(w[:3]) for w in wins] == strided.for_rank(rank) and (chunk, per) == (strided.chunk, strided.per_rank)
        assert not any(w.ring for w in wins)
