"""CPU: the host side of temporal co-denoising (vdx/codenoise.py: weights, the window table, the refusals, the flag) and the
restatement of tests/codenoise_ref.py against the plain CFG-step restatements it must reduce to with one window."""
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
import dpm_ref  # noqa: E402
from vdx.codenoise import check_co_denoise, fuse_weights, window_table  # noqa: E402
from vdx.planner import ChunkPlan, plan  # noqa: E402


def test_weights_are_strictly_positive_and_follow_the_formula():
    for length in range(1, 20):
        for ov in range(0, 9):
            w = fuse_weights(length, ov)
            assert len(w) == length and all(x > 0 for x in w)
            assert w == [min(j + 1, length - j, ov + 1) / (ov + 1) for j in range(length)]
            assert w == w[::-1] and max(w) <= 1.0
    assert fuse_weights(6, 2) == [1 / 3, 2 / 3, 1.0, 1.0, 2 / 3, 1 / 3]
    for bad in ((0, 2), (4, -1)):
        with pytest.raises(ValueError):
            fuse_weights(*bad)


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("T,world,chunk,ov", [(8, 1, 6, 2), (8, 2, 6, 2), (10, 1, 6, 2), (7, 1, 4, 3), (24, 1, 16, 8), (32, 4, 0, 4),
                                              (17, 3, 6, 2), (9, 1, 5, 4)])
def test_table_of_a_planned_job(T, world, chunk, ov):
    cp = plan(T, world, chunk, ov)
    tab = window_table(cp, T)
    wn = tab.wn
    assert wn.dtype == torch.float32 and tuple(wn.shape) == (len(tab.fused), T)
    assert [(s, e) for _, s, e in tab.fused] == list(dict.fromkeys(cp.ranges))         # plan order, repeats left out
    cover = torch.zeros(T, dtype=torch.int64)
    for k, (i, s, e) in enumerate(tab.fused):
        assert cp.ranges[i] == (s, e)
        assert bool((wn[k, s:e] > 0).all()) and float(wn[k, :s].abs().sum()) == 0 and float(wn[k, e:].abs().sum()) == 0
        cover[s:e] += 1
    assert bool((cover >= 1).all())
    for t in range(T):
        col = wn[:, t]
        if cover[t] == 1:
            assert float(col.max()) == 1.0 and int((col != 0).sum()) == 1              # exactly 1.0f, not nearly
        # each entry is a float64 quotient rounded once to fp32: the column sums to 1 within 1 fp32 ulp of 1
        assert abs(float(col.double().sum()) - 1.0) <= _ulp32(1.0)


def test_repeated_tail_window_is_denoised_but_not_fused_and_the_table_ignores_the_world():
    ranges = ((0, 6), (4, 8), (4, 8))                                                  # the planner's repeated tail window
    tabs = [window_table(ChunkPlan(6, 2, ranges + extra, world), 8) for world, extra in ((1, ()), (2, (((4, 8),))))]
    for tab in tabs:
        assert tab.fused == ((0, 0, 6), (1, 4, 8))                                     # one fused window per distinct range
        assert torch.equal(tab.wn, tabs[0].wn)
    assert len(ChunkPlan(6, 2, ranges + ((4, 8),), 2).for_rank(1)) == 2                # still two UNet calls on every rank
    # where each fused window sits in the packed buffer [world][per_rank][slot]: rank i % world, slot i // world
    assert tabs[0].rows(1, 3, 100) == [(0, 0, 6), (100, 4, 4)]
    assert tabs[1].rows(2, 2, 100) == [(0, 0, 6), (200, 4, 4)]
    # a plan that is the same for one and two ranks gives the same table
    a, b = plan(8, 1, 6, 2), plan(8, 2, 6, 2)
    assert a.ranges == b.ranges == ((0, 6), (4, 8)) and a.chunk == b.chunk and a.overlap == b.overlap
    assert window_table(a, 8).fused == window_table(b, 8).fused and torch.equal(window_table(a, 8).wn, window_table(b, 8).wn)


def test_an_uncovered_frame_and_a_bad_range_raise():
    with pytest.raises(ValueError, match="frame 6 is in no window"):
        window_table(ChunkPlan(4, 1, ((0, 4), (3, 6), (7, 9)), 1), 9)
    with pytest.raises(ValueError, match="leaves"):
        window_table(ChunkPlan(4, 1, ((0, 4), (3, 9)), 1), 8)
    with pytest.raises(ValueError, match="64"):
        window_table(ChunkPlan(2, 1, tuple((i, i + 2) for i in range(65)), 1), 66)


def test_halo_is_refused_before_any_work():
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, run_job
    from vdx.scheduler import DDIMScheduler
    on = DiffuserConfig(co_denoise=True)
    assert check_co_denoise(on) is True and check_co_denoise(DiffuserConfig(), "halo") is False
    with pytest.raises(ValueError, match="allgather"):
        check_co_denoise(on, "halo")
    with pytest.raises(ValueError, match="allgather"):
        run_job(on, exchange="halo", out_video=None)                                   # before any model is loaded: needs no GPU
    unet = SimpleNamespace(config=SimpleNamespace(in_channels=4))                     # never called
    cfg = DiffuserConfig(num_frames=8, steps=2, chunk_size=6, overlap=2, height=64, width=64, mode="chunk", device="cpu",
                         co_denoise=True)
    d = DistributedVideoDiffuser(cfg, unet, DDIMScheduler(), None, None)
    with pytest.raises(ValueError, match="allgather"):
        d(exchange="halo")


def test_the_flag_round_trips_and_is_off_by_default():
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args
    p = build_arg_parser()
    assert DiffuserConfig().co_denoise is False
    assert config_from_args(p.parse_args([])).co_denoise is False
    on = config_from_args(p.parse_args(["--co_denoise", "--scheduler", "dpmpp_2m", "--free_init", "2"]))
    assert on.co_denoise is True and on.scheduler == "dpmpp_2m" and on.free_init_iters == 2
    off = config_from_args(p.parse_args(["--scheduler", "dpmpp_2m", "--free_init", "2"]))
    on.co_denoise = False
    assert on == off


# ---- the restatement with one window is the plain CFG step's restatement ------------------------------------------------------
def _one_window(seed=0, shape=(1, 4, 3, 5, 7)):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g).half()
    eps2 = torch.randn((2,) + shape[1:], generator=g).half()
    eps2[0, 0, 0, 0, 0], eps2[1, 0, 0, 0, 0] = -0.0, 0.0                               # signed zeros go through 1.0f * x untouched
    eps2[0, 1, 1, 2, 3] = 65504.0
    prev = torch.randn(shape, generator=g).half()
    return z, eps2, prev, torch.ones(1, shape[2])


def test_one_window_ddim_restatement_is_the_plain_one():
    from oracle.ddim_ref import DDIMSchedulerRef
    z, eps2, _, wn = _one_window()
    ref = DDIMSchedulerRef()
    ref.set_timesteps(10)
    for t in (901, 401, 1):
        coeffs = tuple(float(c) for c in ref.coefficients(t))
        got = R.cofuse_ddim(z, [eps2], [(0, z.shape[2])], wn, 7.5, coeffs)
        want = ref.step_gpu_rules(dpm_ref.cfg_combine(eps2, 7.5), t, z).prev_sample
        assert got.dtype == torch.float16 and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_one_window_dpm_restatement_is_the_plain_one():
    z, eps2, prev, wn = _one_window(seed=1)
    sig = dpm_ref.sigmas(6)
    for i, second in ((0, False), (2, True), (5, False)):                              # first order, second order, the last step
        k = dpm_ref.scalars(sig, i, second)
        got, got_x0 = R.cofuse_dpm(z, [eps2], [(0, z.shape[2])], wn, 7.5, k, prev if second else None)
        want, want_x0 = dpm_ref.step(dpm_ref.cfg_combine(eps2, 7.5), z, prev if second else None, k)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert torch.equal(got_x0.view(torch.int16), want_x0.view(torch.int16))


def test_restatement_averages_in_fp32_in_window_order():
    """Three windows over one frame, values chosen so that the order of the fp32 adds shows in the result."""
    shape = (1, 1, 1, 1, 1)
    wins = [torch.full((2, 1, 1, 1, 1), v, dtype=torch.float16) for v in (1024.0, 2.0 ** -16, -1024.0)]
    wn = torch.tensor([[1 / 3], [1 / 3], [1 / 3]], dtype=torch.float32)
    fused = R.fuse(wins, [(0, 1)] * 3, wn, shape)
    w = np.float32(1 / 3)
    want = np.float32(np.float32(np.float32(w * np.float32(1024.0)) + np.float32(w * np.float32(2.0 ** -16))) + np.float32(w * np.float32(-1024.0)))
    assert float(fused[0, 0, 0, 0, 0]) == float(np.float16(want)) == 0.0               # the small term is lost in the first add
    assert float(R.fuse(wins[1:] + wins[:1], [(0, 1)] * 3, wn, shape)[0, 0, 0, 0, 0]) == 0.0
    assert float(R.fuse([wins[0], wins[2], wins[1]], [(0, 1)] * 3, wn, shape)[0, 0, 0, 0, 0]) > 0   # another order, another sum
    with pytest.raises(ValueError, match="no window"):
        R.fuse(wins[:1], [(1, 1)], torch.ones(1, 2), (1, 1, 2, 1, 1))
