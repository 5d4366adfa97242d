"""Cross-frame attention's host side: `crossframe.ref_table`, the refusals, `options.check_cross_frame` and the record (no GPU)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT,) if p not in sys.path]

import vdx  # noqa: E402,F401
from vdx import crossframe  # noqa: E402
from vdx.options import RECORD_KEYS, check_cross_frame, cross_frame_record, info_options, resolve  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args  # noqa: E402


@pytest.mark.parametrize("F", [1, 2, 5])
@pytest.mark.parametrize("mode,row", [
    ("first", lambda f: [0]), ("sparse_causal", lambda f: [0, max(f - 1, 0)]),
    ("self_first", lambda f: [f, 0]), ("self_prev", lambda f: [f, max(f - 1, 0)])])
def test_ref_table(mode, row, F):
    t = crossframe.ref_table(mode, F)
    assert str(t.dtype) == "torch.int32" and t.tolist() == [row(f) for f in range(F)]


def test_explicit_table():
    rows = [[f, f, 0, 4] for f in range(5)]
    assert crossframe.ref_table(rows, 5).tolist() == rows
    assert crossframe.check_params(rows, 2) == {"mode": tuple(map(tuple, rows)), "refs_per_frame": 4, "max_downsample": 2}


@pytest.mark.parametrize("mode,F", [
    ("causal", 3), (None, 3), ([], 3), ([[0], [0, 1], [0]], 3),          # unknown names, no rows, ragged rows
    ([[]] * 3, 3), ([[0] * 5] * 3, 3),                                     # R = 0, R = 5
    ([[0], [3], [0]], 3), ([[0], [-1], [0]], 3), ([[0], [1.0], [0]], 3),   # out of range, negative, no integer
    ([[0], [1]], 3), ("first", 0)], ids=str)                               # two rows for three frames; no frames
def test_ref_table_refuses(mode, F):
    with pytest.raises(ValueError):
        crossframe.ref_table(mode, F)


@pytest.mark.parametrize("kw", [
    dict(cross_frame="causal"), dict(cross_frame="first", cross_frame_max_downsample=3),
    dict(cross_frame=[[0], [0, 1]]), dict(cross_frame_max_downsample=2),                     # ragged; needs cross_frame
    dict(cross_frame="first", tome=0.5), dict(cross_frame="first", hypertile=(2, 2))], ids=str)
def test_check_cross_frame_refuses(kw):
    cfg = DiffuserConfig(**{**dict(height=576, width=1024), **kw})
    with pytest.raises(ValueError):
        check_cross_frame(cfg)
    with pytest.raises(ValueError):
        resolve(cfg, "allgather", 1)


def test_record_only_when_set():
    assert "cross_frame" not in RECORD_KEYS
    off = resolve(DiffuserConfig(height=576, width=1024), "allgather", 1)
    assert off.cross_frame is None and cross_frame_record(off) == {} and "cross_frame" not in info_options(off, [])
    on = resolve(DiffuserConfig(height=576, width=1024, cross_frame="sparse_causal", cross_frame_max_downsample=2), job=True)
    want = {"mode": "sparse_causal", "refs_per_frame": 2, "max_downsample": 2}
    assert on.cross_frame == want and cross_frame_record(on) == {"cross_frame": want} == cross_frame_record({"cross_frame": want, "x": 1})
    assert info_options(on, [])["cross_frame"] == want
    table = resolve(DiffuserConfig(height=576, width=1024, cross_frame=[[0], [0]]), "allgather", 1).cross_frame
    assert table == {"mode": [[0], [0]], "refs_per_frame": 1, "max_downsample": 8}


def test_flags():
    p = build_arg_parser()
    base = ["--prompt", "x"] if any(a.dest == "prompt" and a.required for a in p._actions) else []
    cfg = config_from_args(p.parse_args(base + ["--cross_frame", "self_prev", "--cross_frame_max_downsample", "2"]))
    assert cfg.cross_frame == "self_prev" and cfg.cross_frame_max_downsample == 2
    cfg = config_from_args(p.parse_args(base))
    assert cfg.cross_frame is None and cfg.cross_frame_max_downsample == 8
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--cross_frame", "causal"])
