"""HyperTile's host side: `options.check_hypertile`'s refusals, the per-level grid rule and the record (no GPU)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT,) if p not in sys.path]

import vdx  # noqa: E402,F401
from vdx import hypertile  # noqa: E402
from vdx.options import RECORD_KEYS, check_hypertile, hypertile_record, info_options, resolve  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args  # noqa: E402


@pytest.mark.parametrize("kw", [
    dict(hypertile=(5, 2)),                                   # 72 x 128 latent cells: 5 does not divide 72
    dict(hypertile=(2, 3)),                                   # 3 does not divide 128
    dict(hypertile=(12, 2)),                                  # windows of 6 cells: under 8 a side
    dict(hypertile=(2, 2), tome=0.5),                         # merged rows have no grid
    dict(hypertile=(2, 2), hypertile_max_downsample=3),
    dict(hypertile=(0, 2)), dict(hypertile=(2.0, 2)), dict(hypertile=(2, 2, 2)), dict(hypertile=4),
    dict(hypertile_max_downsample=2),                         # needs hypertile
    dict(hypertile=(2, 3), co_denoise=True, tile=(256, 320)), # the UNet's frame is the tile: 40 cells, 3 does not divide
], ids=str)
def test_check_hypertile_refuses(kw):
    cfg = DiffuserConfig(**{**dict(height=576, width=1024), **kw})
    with pytest.raises(ValueError):
        check_hypertile(cfg)
    with pytest.raises(ValueError):
        resolve(cfg, "allgather", 1)
    assert check_hypertile(DiffuserConfig(height=576, width=1024, hypertile=(3, 2)))["grid"] == [3, 2]      # 24 x 64 windows


@pytest.mark.parametrize("grid,md,down,hh,ww,want", [
    ((2, 2), 1, 1, 72, 128, (2, 2)), ((2, 2), 1, 2, 36, 64, None),        # above max_downsample
    ((4, 4), 2, 2, 36, 64, (2, 2)), ((4, 4), 8, 4, 18, 32, None),          # ny // d: 4 // 4 = 1 x 1 is the plain attention
    ((8, 2), 8, 4, 18, 32, (2, 1)), ((4, 4), 2, 2, 9, 64, None),           # max(1, 2 // 4); a deeper grid that does not divide
    ((1, 1), 1, 1, 72, 128, None),
])
def test_level_grid_rule(grid, md, down, hh, ww, want):
    assert hypertile.window_grid(hypertile.check_params(*grid, md), hh, ww, down) == want


def test_level_zero_must_divide():
    with pytest.raises(ValueError):
        hypertile.window_grid(hypertile.check_params(2, 2), 9, 14, 1)


def test_record_only_when_set():
    keys = RECORD_KEYS
    assert "hypertile" not in keys and keys == ("freeu", "tome", "co_denoise", "tile", "loop", "context_stride", "mask", "negative_prompt",
                                                "guidance_rescale")
    off = resolve(DiffuserConfig(height=576, width=1024), "allgather", 1)
    assert off.hypertile is None and hypertile_record(off) == {} and "hypertile" not in info_options(off, [])
    on = resolve(DiffuserConfig(height=576, width=1024, hypertile=(4, 4), hypertile_max_downsample=2), job=True)
    want = {"grid": [4, 4], "max_downsample": 2, "levels": [{"down": 1, "grid": [4, 4], "window": [18, 32]},
                                                            {"down": 2, "grid": [2, 2], "window": [18, 32]}]}
    assert on.hypertile == want and hypertile_record(on) == {"hypertile": want} == hypertile_record({"hypertile": want, "x": 1})
    assert info_options(on, [])["hypertile"] == want


def test_flags():
    p = build_arg_parser()
    base = ["--prompt", "x"] if any(a.dest == "prompt" and a.required for a in p._actions) else []
    cfg = config_from_args(p.parse_args(base + ["--hypertile", "2", "4", "--hypertile_max_downsample", "2"]))
    assert cfg.hypertile == (2, 4) and cfg.hypertile_max_downsample == 2
    cfg = config_from_args(p.parse_args(base))
    assert cfg.hypertile is None and cfg.hypertile_max_downsample == 1
