"""CPU: the host side of spatially tiled co-denoising (vdx/codenoise.py: tile starts, per-axis weights, the refusals, the flags)
and the restatement of tests/cotile_ref.py against tests/codenoise_ref.py, which it must reduce to with one spatial tile."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import vdx  # noqa: E402,F401
import codenoise_ref as R  # noqa: E402
import cotile_ref as RT  # noqa: E402
import dpm_ref  # noqa: E402
from vdx.codenoise import axis_weights, check_tile, fuse_weights, tile_plan, tile_starts  # noqa: E402


def test_tile_starts_on_hand_checked_cases():
    assert tile_starts(8, 8, 3) == [0]                              # n == tile
    assert tile_starts(13, 8, 3) == [0, 5]                          # an exact fit: 8 + 5
    assert tile_starts(18, 8, 3) == [0, 5, 10]
    assert tile_starts(20, 8, 3) == [0, 5, 10, 12]                  # the last tile moved back from 15 to end at 20
    assert tile_starts(12, 8, 3) == [0, 4]                          # moved back from 5
    assert tile_starts(12, 4, 0) == [0, 4, 8]                       # overlap 0, an exact fit
    assert tile_starts(10, 4, 0) == [0, 4, 6]                       # overlap 0, moved
    assert tile_starts(9, 8, 7) == [0, 1]
    assert tile_starts(144, 72, 18) == [0, 54, 72] and tile_starts(256, 128, 32) == [0, 96, 128]
    assert tile_starts(1, 1, 0) == [0]
    for bad in ((8, 9, 0), (8, 0, 0), (8, 4, 4), (8, 4, -1), (0, 1, 0)):
        with pytest.raises(ValueError):
            tile_starts(*bad)


@pytest.mark.parametrize("n,tile,ov", [(8, 8, 3), (13, 8, 3), (20, 8, 3), (12, 8, 3), (14, 6, 2), (9, 6, 2), (12, 4, 0), (10, 4, 0),
                                       (144, 72, 18), (256, 128, 32), (37, 9, 8), (64, 8, 1)])
def test_every_cell_is_covered_and_the_weights_sum_to_one(n, tile, ov):
    starts = tile_starts(n, tile, ov)
    assert starts[0] == 0 and starts[-1] == n - tile and starts == sorted(set(starts))
    cover = np.zeros(n, dtype=np.int64)
    for s in starts:
        cover[s:s + tile] += 1
    assert (cover >= 1).all()
    w = axis_weights(n, tile, ov, starts)
    assert w.dtype == torch.float32 and tuple(w.shape) == (len(starts), n)
    raw = np.zeros((len(starts), n))
    for k, s in enumerate(starts):
        raw[k, s:s + tile] = fuse_weights(tile, ov)
        assert bool((w[k, s:s + tile] > 0).all()) and float(w[k, :s].abs().sum()) == 0 and float(w[k, s + tile:].abs().sum()) == 0
    norm = raw / raw.sum(axis=0)                                    # float64
    assert np.abs(norm.sum(axis=0) - 1.0).max() <= cover.max() * 2.0 ** -53     # sums to 1 per cell: float64 quotients, each rounded once
    assert np.array_equal(w.numpy(), norm.astype(np.float32))       # rounded to fp32 once
    for p in range(n):
        if cover[p] == 1:
            assert float(w[:, p].max()) == 1.0 and int((w[:, p] != 0).sum()) == 1      # exactly 1.0f, not nearly
        assert abs(float(w[:, p].double().sum()) - 1.0) <= float(np.spacing(np.float32(1.0))) * cover[p] / 2


def test_tile_plan_is_the_product_of_the_axes():
    tp = tile_plan(12, 20, 8, 8, 3, 3)
    assert (tp.ys, tp.xs, tp.count) == ((0, 4), (0, 5, 10, 12), 8)
    assert tp.boxes[:5] == [(0, 8, 0, 8), (0, 8, 5, 8), (0, 8, 10, 8), (0, 8, 12, 8), (4, 8, 0, 8)]      # ky-major: the slots' order
    assert torch.equal(tp.wyn, axis_weights(12, 8, 3, [0, 4])) and torch.equal(tp.wxn, axis_weights(20, 8, 3, [0, 5, 10, 12]))
    assert tp.record(3) == {"tile": [8, 8], "overlap": [3, 3], "grid": [2, 4], "windows": 24}
    one = tile_plan(9, 16, 9, 16, 2, 4)                                # a tile equal to the frame
    assert (one.ys, one.xs) == ((0,), (0,)) and bool((one.wyn == 1).all()) and bool((one.wxn == 1).all())
    with pytest.raises(ValueError, match="64"):
        tile_plan(64, 64, 8, 8, 1, 1)                                  # 9 x 9 tiles
    with pytest.raises(ValueError, match="no tile"):
        axis_weights(10, 4, 0, [0, 6])


def _cfg(**kw):
    from vdx.pipeline import DiffuserConfig
    return DiffuserConfig(**{**dict(height=128, width=192, co_denoise=True, tile=(64, 128)), **kw})


def test_check_tile_converts_pixels_and_defaults_the_overlap():
    from vdx.pipeline import DiffuserConfig
    assert check_tile(DiffuserConfig()) is None and check_tile(DiffuserConfig(), "halo") is None
    assert check_tile(_cfg()) == (8, 16, 2, 4)                      # a quarter of the tile, in latent cells
    assert check_tile(_cfg(tile_overlap=(0, 0))) == (8, 16, 0, 0)
    assert check_tile(_cfg(tile_overlap=(48, 112))) == (8, 16, 6, 14)
    assert check_tile(_cfg(tile=(128, 192))) == (16, 24, 4, 6)      # a tile equal to the frame is allowed
    assert check_tile(_cfg(tile=[64, 128])) == (8, 16, 2, 4)
    assert check_tile(_cfg(height=1152, width=2048, tile=(576, 1024))) == (72, 128, 18, 32)


@pytest.mark.parametrize("kw,exchange,match", [
    (dict(co_denoise=False), "allgather", "co_denoise"),
    (dict(), "halo", "allgather"),
    (dict(guidance_rescale=0.5), "allgather", "guidance_rescale"),
    (dict(tile=(136, 128)), "allgather", "larger"),
    (dict(tile=(64, 200)), "allgather", "larger"),
    (dict(tile=(60, 128)), "allgather", "multiples of 8"),
    (dict(tile=(64, 100)), "allgather", "multiples of 8"),
    (dict(tile=(56, 128)), "allgather", "UNet"),                    # 7 latent cells a side
    (dict(tile=(64, 8)), "allgather", "UNet"),
    (dict(tile=(64,)), "allgather", "two integers"),
    (dict(tile=(64.0, 128)), "allgather", "two integers"),
    (dict(tile_overlap=(64, 0)), "allgather", r"\[0, tile\)"),
    (dict(tile_overlap=(0, 128)), "allgather", r"\[0, tile\)"),
    (dict(tile_overlap=(-8, 0)), "allgather", r"\[0, tile\)"),
    (dict(tile_overlap=(4, 0)), "allgather", "multiples of 8"),
    (dict(tile=None, tile_overlap=(8, 8)), "allgather", "needs tile"),
    (dict(height=1024, width=1024, tile=(64, 64), tile_overlap=(8, 8)), "allgather", "64"),        # 19 x 19 tiles
])
def test_check_tile_refusals(kw, exchange, match):
    with pytest.raises(ValueError, match=match):
        check_tile(_cfg(**kw), exchange)


def test_refused_before_anything_loads():
    from types import SimpleNamespace

    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, run_job
    from vdx.scheduler import DDIMScheduler
    for kw, exchange, match in ((dict(co_denoise=False), "allgather", "co_denoise"), (dict(), "halo", "allgather"),
                                (dict(guidance_rescale=0.5), "allgather", "guidance_rescale")):
        with pytest.raises(ValueError, match=match):
            run_job(_cfg(**kw), exchange=exchange, out_video=None)                       # before any model is loaded: needs no GPU
    unet = SimpleNamespace(config=SimpleNamespace(in_channels=4))                         # never called
    cfg = DiffuserConfig(num_frames=8, steps=2, chunk_size=6, overlap=2, height=64, width=64, mode="chunk", device="cpu",
                         co_denoise=True, tile=(72, 64))
    d = DistributedVideoDiffuser(cfg, unet, DDIMScheduler(), None, None)
    with pytest.raises(ValueError, match="larger"):
        d()


def test_the_flags_round_trip_and_are_off_by_default():
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args
    p = build_arg_parser()
    assert DiffuserConfig().tile is None and DiffuserConfig().tile_overlap is None
    off = config_from_args(p.parse_args(["--co_denoise"]))
    assert off.tile is None and off.tile_overlap is None
    on = config_from_args(p.parse_args(["--co_denoise", "--tile", "576", "1024", "--height", "1152", "--width", "2048"]))
    assert on.tile == (576, 1024) and on.tile_overlap is None and check_tile(on) == (72, 128, 18, 32)
    both = config_from_args(p.parse_args(["--co_denoise", "--tile", "64", "128", "--tile_overlap", "8", "16"]))
    assert both.tile == (64, 128) and both.tile_overlap == (8, 16)
    both.tile = both.tile_overlap = None
    assert both == off
    with pytest.raises(SystemExit):
        p.parse_args(["--tile", "64"])


# ---- the restatement with one spatial tile is tests/codenoise_ref.py's ---------------------------------------------------------
def test_one_tile_restatement_is_the_temporal_one():
    from vdx.codenoise import window_table
    from vdx.planner import ChunkPlan
    C, T, H, W = 3, 7, 5, 6
    ranges = [(0, 4), (1, 5), (2, 6), (3, 7)]
    wn = window_table(ChunkPlan(4, 3, tuple(ranges), 1), T).wn
    g = torch.Generator().manual_seed(2)
    z, prev = (torch.randn(1, C, T, H, W, generator=g).half() for _ in range(2))
    wins = [torch.randn(2, C, e - s, H, W, generator=g).half() for s, e in ranges]
    wins[0][0, 0, 0, 0, 0], wins[1][1, 0, 0, 0, 0] = -0.0, 65504.0
    table = [(s, e - s) for s, e in ranges]
    one = dict(ys=[0], xs=[0], th=H, tw=W, wyn=torch.ones(1, H), wxn=torch.ones(1, W))
    nested = [[[w]] for w in wins]
    coeffs = (0.6, 0.8, 0.9, 0.435889894)
    a = RT.cotile_ddim(z, nested, table, wn, gs=7.5, coeffs=coeffs, **one)
    b = R.cofuse_ddim(z, wins, table, wn, 7.5, coeffs)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    sig = dpm_ref.sigmas(6)
    for i, second in ((0, False), (2, True), (5, False)):
        k = dpm_ref.scalars(sig, i, second)
        a, ax0 = RT.cotile_dpm(z, nested, table, wn, gs=7.5, k=k, x0_prev=prev if second else None, **one)
        b, bx0 = R.cofuse_dpm(z, wins, table, wn, 7.5, k, prev if second else None)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(ax0.view(torch.int16), bx0.view(torch.int16))
    ctx = torch.randn(1, C, 1, H, W, generator=g).half()
    for c, cw in ((None, 0.0), (ctx, 0.35)):
        assert torch.equal(RT.cfg_input_tile(z, c, cw, 2, 6, 0, H, 0, W), R.cfg_input_window(z, c, cw, 2, 6))


def test_restatement_multiplies_time_row_column_and_adds_in_window_order():
    """One cell under 2 x 2 spatial tiles and one time window, weights that are no powers of two: the three-factor product and
    the order of the adds show in the fp32 sum."""
    wins = [[[torch.full((2, 1, 1, 1, 1), v, dtype=torch.float16) for v in row] for row in ((1024.0, 2.0 ** -14), (-1024.0, 3.0))]]
    wn = torch.tensor([[1.0]])
    wy = torch.tensor([[1 / 3], [2 / 3]], dtype=torch.float32)
    wx = torch.tensor([[0.3], [0.7]], dtype=torch.float32)
    got = RT.fuse(wins, [(0, 1)], wn, [0, 0], [0, 0], 1, 1, wy, wx, (1, 1, 1, 1, 1))
    f = np.float32
    w = [[f(f(f(1.0) * wy[a, 0].numpy()) * wx[b, 0].numpy()) for b in range(2)] for a in range(2)]
    vals = [[f(1024.0), f(2.0 ** -14)], [f(-1024.0), f(3.0)]]
    acc = f(w[0][0] * vals[0][0])
    for a, b in ((0, 1), (1, 0), (1, 1)):
        acc = f(acc + f(w[a][b] * vals[a][b]))
    assert float(got[0, 0, 0, 0, 0]) == float(np.float16(acc))
    with pytest.raises(ValueError, match="no window"):
        RT.fuse(wins, [(0, 1)], wn, [0, 0], [0, 0], 1, 1, torch.ones(2, 2), torch.ones(2, 1), (1, 1, 1, 2, 1))
