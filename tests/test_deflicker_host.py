"""CPU: the temporal filter's refusals, before any device work, and its option through vdx/options.py and the front end."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import vdx  # noqa: E402,F401
from vdx import deflicker  # noqa: E402
from vdx._lib import VdxError  # noqa: E402
from vdx.options import check_deflicker, deflicker_record, info_options, resolve  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args, run_job  # noqa: E402

REFUSALS = [
    (dict(deflicker=(0.0, 10.0)), "strength must lie in"), (dict(deflicker=(1.5, 10.0)), "strength must lie in"),
    (dict(deflicker=(float("nan"), 10.0)), "strength must lie in"), (dict(deflicker=("0.5", 10.0)), "strength must be a number"),
    (dict(deflicker=(0.5, 0.0)), "sigma must be finite"), (dict(deflicker=(0.5, float("inf"))), "sigma must be finite"),
    (dict(deflicker=(0.5, float("nan"))), "sigma must be finite"), (dict(deflicker=(0.5, -1.0)), "sigma must be finite"),
    (dict(deflicker=(0.5, 10.0), deflicker_passes=0), "passes must be an integer in 1..4"),
    (dict(deflicker=(0.5, 10.0), deflicker_passes=5), "passes must be an integer in 1..4"),
    (dict(deflicker=(0.5, 10.0), deflicker_passes=2.0), "passes must be an integer in 1..4"),
    (dict(deflicker=0.5), "two numbers"), (dict(deflicker_passes=2), "needs deflicker"),
    (dict(deflicker=(0.5, 10.0), height=8, width=64), "too small"),
]


class Boom:
    def __getattr__(self, name):
        raise AssertionError(f"the pipeline was touched ({name}) before the refusal")


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[f"{i}-{t}" for i, (_, t) in enumerate(REFUSALS)])
def test_refused_before_anything_loads(kw, text):
    with pytest.raises(ValueError, match=text):
        check_deflicker(DiffuserConfig(**kw))
    with pytest.raises(ValueError, match=text):
        run_job(DiffuserConfig(**kw), out_video=None, pipe=Boom())


def test_filter_frames_checks_before_any_device_work():
    clip = np.zeros((3, 32, 32, 3), np.uint8)
    for bad in (lambda: deflicker.filter_frames(clip, 0.0), lambda: deflicker.filter_frames(clip, 0.5, float("inf")),
                lambda: deflicker.filter_frames(clip, passes=5), lambda: deflicker.filter_frames(clip[:, :8]),
                lambda: deflicker.filter_frames(clip.astype(np.float32)), lambda: deflicker.filter_frames(clip[:0])):
        with pytest.raises(VdxError):
            bad()


def test_the_option_resolves_and_records_only_when_set():
    want = {"strength": 0.25, "sigma": 4.0, "passes": 3}
    on = resolve(DiffuserConfig(deflicker=(0.25, 4), deflicker_passes=3), "allgather", 1)
    off = resolve(DiffuserConfig(), "allgather", 1)
    assert on.deflicker == want and off.deflicker is None and resolve(DiffuserConfig(deflicker=(0.25, 4), deflicker_passes=3), job=True).deflicker == want
    assert {**dataclasses.asdict(on), "deflicker": None} == dataclasses.asdict(off)                      # nothing else moves
    assert deflicker_record(on) == {"deflicker": want} == deflicker_record({"deflicker": want, "x": 1}) and deflicker_record(off) == {}
    assert info_options(on, [])["deflicker"] == want and "deflicker" not in info_options(off, [])
    parse = lambda argv: config_from_args(build_arg_parser().parse_args(argv))
    assert (parse([]).deflicker, parse([]).deflicker_passes) == (None, 1)
    cfg = parse(["--deflicker", "0.25", "--deflicker_sigma", "4", "--deflicker_passes", "3"])
    assert cfg.deflicker == (0.25, 4.0) and check_deflicker(cfg) == want and parse(["--deflicker", "1"]).deflicker == (1.0, 10.0)


def test_help_lists_the_flags():
    out = subprocess.run([sys.executable, "-m", "vdx.pipeline", "--help"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert all(flag in out for flag in ("--deflicker STRENGTH", "--deflicker_sigma S", "--deflicker_passes N"))

