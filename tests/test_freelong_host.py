"""CPU: FreeLong's host side (vdx/freelong.py) against the numpy.fft restatement of tests/freelong_ref.py, and the job option."""
import dataclasses
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import vdx  # noqa: E402,F401
import freelong_ref as R  # noqa: E402
from vdx import freelong  # noqa: E402
from vdx.options import RECORD_KEYS, check_free_long, free_long_record, resolve  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args  # noqa: E402


@pytest.mark.parametrize("method", ["gaussian", "butterworth", "ideal"])
@pytest.mark.parametrize("F,d_t", [(7, 0.25), (33, 0.25), (40, 0.5), (128, 0.25), (48, 0.1)])
def test_blend_matrix_is_the_filter_as_a_real_symmetric_circulant(F, d_t, method):
    lp, ref, g = freelong.blend_matrix(F, method, d_t), R.blend_matrix(F, method, d_t), R.temporal_gain(F, method, d_t)
    assert lp.dtype == torch.float64 and float((lp - ref).abs().max()) <= 1e-13
    assert torch.equal(lp, lp.T) and all(torch.equal(lp[t], lp[0].roll(t)) for t in range(F))
    assert float((lp.sum(dim=1) - g[0]).abs().max()) <= 1e-13


def test_blend_matrix_anchors():
    assert torch.equal(freelong.blend_matrix(17, "gaussian", 0.0), torch.zeros(17, 17, dtype=torch.float64))
    for F in (8, 17):                                              # |coordinate| <= 1 everywhere: a cutoff of 1 passes all
        assert float((freelong.blend_matrix(F, "ideal", 1.0) - torch.eye(F, dtype=torch.float64)).abs().max()) <= 1e-14
    assert freelong.radius_of(24) == 12 and freelong.radius_of(2) == 1 and freelong.MAX_FRAMES == 128


@pytest.mark.parametrize("args,text", [((1,), "window 1 outside"), ((129,), "window 129 outside"), ((24.0,), "must be an integer"),
                                       ((24, -0.1), "d_t"), ((24, float("nan")), "d_t"), ((24, 0.25, "box"), "unknown filter"),
                                       ((24, 0.25, "butterworth", 0), "order")])
def test_check_params_refuses(args, text):
    with pytest.raises(ValueError, match=text):
        freelong.check_params(*args)


ON = dict(free_long=(24, 0.25))
REFUSALS = [
    (dict(free_long=(1, 0.25)), "window 1 outside"), (dict(free_long=(24.5, 0.25)), "must be an integer"), (dict(free_long=(24,)), "two numbers"),
    (dict(free_long=(24, -1.0)), "d_t"), (dict(free_long_method="ideal"), "needs free_long"), (dict(ON, free_long_method="box"), "unknown filter"),
    (dict(ON, free_noise=(16, 4)), "free_noise"), (dict(ON, co_denoise=True), "co_denoise"),
    (dict(ON, mode="chunk", chunk_size=24), "nothing to blend"), (dict(ON, num_frames=24), "nothing to blend"), (dict(ON, num_frames=200), "exceeds the 128"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[t for _, t in REFUSALS])
def test_check_free_long_refuses_before_any_model_loads(kw, text):
    cfg = DiffuserConfig(**{"num_frames": 64, "mode": "fsdp", **kw})
    with pytest.raises(ValueError, match=text):
        check_free_long(cfg, "allgather", 1)


def test_accepted_record_and_the_default_job():
    cfg = DiffuserConfig(num_frames=64, mode="fsdp", free_long=(24, 0.25), free_long_method="ideal")
    want = {"window": 24, "d_t": 0.25, "method": "ideal"}
    on, off = resolve(cfg, "allgather", 1), resolve(DiffuserConfig(num_frames=64, mode="fsdp"), "allgather", 1)
    assert check_free_long(cfg, "halo", 2) == want and on.free_long == want and off.free_long is None
    assert {**dataclasses.asdict(on), "free_long": None} == dataclasses.asdict(off)                       # nothing else moves
    assert free_long_record(on) == {"free_long": want} == free_long_record({"free_long": want, "x": 1})
    assert free_long_record(off) == {} == free_long_record({"x": 1})
    assert "free_long" not in RECORD_KEYS and [f.name for f in dataclasses.fields(on)][-1] == "free_long"


def test_flags_round_trip():
    p = build_arg_parser()
    cfg = config_from_args(p.parse_args(["--free_long", "24", "0.25", "--free_long_method", "butterworth"]))
    assert cfg.free_long == (24, 0.25) and isinstance(cfg.free_long[0], int) and cfg.free_long_method == "butterworth"
    off = config_from_args(p.parse_args([]))
    assert off.free_long is None and off.free_long_method == "gaussian"
