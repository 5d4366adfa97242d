"""Token downsampling's host side: the row map against torch's nearest-neighbour `interpolate`, the refusals of
`kvdown.check_params` / `check_frame` / `options.check_kv_downsample`, the per-level factor rule and the record (no GPU)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT,) if p not in sys.path]

import vdx  # noqa: E402,F401
from vdx import kvdown  # noqa: E402
from vdx.options import RECORD_KEYS, check_kv_downsample, info_options, kv_downsample_record, resolve  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args  # noqa: E402


@pytest.mark.parametrize("hh,ww", [(6, 10), (9, 16), (7, 9), (18, 32), (4, 144), (72, 128), (5, 5)])
@pytest.mark.parametrize("s", [2, 3, 4, 5, 8])
def test_key_rows_are_nearest_interpolation(hh, ww, s):
    if min(hh, ww) < s:
        with pytest.raises(RuntimeError):                      # torch refuses an empty output too
            F.interpolate(torch.zeros(1, 1, hh, ww), scale_factor=1 / s, mode="nearest")
        assert min(kvdown.key_grid(hh, ww, s)) == 0
        return
    grid = torch.arange(2 * hh * ww, dtype=torch.float64).view(2, 1, hh, ww)       # a token's value is its row
    want = F.interpolate(grid, scale_factor=1 / s, mode="nearest")
    assert tuple(want.shape[2:]) == kvdown.key_grid(hh, ww, s)
    assert torch.equal(kvdown.key_rows(2, hh, ww, s), want.view(2, -1).long())


@pytest.mark.parametrize("kw", [
    dict(kv_downsample=1), dict(kv_downsample=9), dict(kv_downsample=2.0), dict(kv_downsample=True), dict(kv_downsample=(2, 2)),
    dict(kv_downsample=2, kv_downsample_max_downsample=3),
    dict(kv_downsample_max_downsample=2),                         # needs kv_downsample
    dict(kv_downsample=8, height=192, width=1024),                # 24 x 128 latent cells: a key grid of 3 x 16, under 4 a side
    dict(kv_downsample=8, co_denoise=True, tile=(192, 320)),      # the UNet's frame is the tile: 24 cells, 3 keys
    dict(kv_downsample=2, tome=0.5), dict(kv_downsample=2, hypertile=(2, 2)), dict(kv_downsample=2, cross_frame="first"),
], ids=str)
def test_check_kv_downsample_refuses(kw):
    cfg = DiffuserConfig(**{**dict(height=576, width=1024), **kw})
    with pytest.raises(ValueError):
        check_kv_downsample(cfg)
    with pytest.raises(ValueError):
        resolve(cfg, "allgather", 1)
    assert check_kv_downsample(DiffuserConfig(height=256, width=1024, kv_downsample=8))["factor"] == 8       # 4 x 16 keys


@pytest.mark.parametrize("factor,md,want", [
    (2, 1, [{"down": 1, "factor": 2, "keys": [36, 64]}]),
    (4, 2, [{"down": 1, "factor": 4, "keys": [18, 32]}, {"down": 2, "factor": 2, "keys": [18, 32]}]),
    (2, 8, [{"down": 1, "factor": 2, "keys": [36, 64]}]),         # 2 // 2 = 1 from level 1 on: the plain attention
])
def test_level_rule_at_the_headline_frame(factor, md, want):
    params = kvdown.check_params(factor, md)
    assert kvdown.levels(params, 72, 128) == want
    assert [kvdown.level_factor(params, 1 << lvl) for lvl in range(4)] == \
        [next((r["factor"] for r in want if r["down"] == 1 << lvl), 1) for lvl in range(4)]
    with pytest.raises(ValueError):
        kvdown.check_frame(6, 128, params)                        # 3 or 1 key rows


def test_record_only_when_set():
    assert "kv_downsample" not in RECORD_KEYS
    off = resolve(DiffuserConfig(height=576, width=1024), "allgather", 1)
    assert off.kv_downsample is None and kv_downsample_record(off) == {} and "kv_downsample" not in info_options(off, [])
    on = resolve(DiffuserConfig(height=576, width=1024, kv_downsample=4, kv_downsample_max_downsample=2), job=True)
    want = {"factor": 4, "max_downsample": 2, "levels": kvdown.levels(kvdown.check_params(4, 2), 72, 128)}
    assert on.kv_downsample == want and kv_downsample_record(on) == {"kv_downsample": want} == kv_downsample_record({"kv_downsample": want, "x": 1})
    assert info_options(on, [])["kv_downsample"] == want

    p = build_arg_parser()                                        # the flags reach the fields
    base = ["--prompt", "x"] if any(a.dest == "prompt" and a.required for a in p._actions) else []
    cfg = config_from_args(p.parse_args(base + ["--kv_downsample", "4", "--kv_downsample_max_downsample", "2"]))
    assert cfg.kv_downsample == 4 and cfg.kv_downsample_max_downsample == 2
