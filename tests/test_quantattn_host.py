"""The INT8 attention's host side: `quantattn.check_params` / `levels`, the refusals of `options.check_quant_attn`, the record
and the flags (no GPU)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT,) if p not in sys.path]

import vdx  # noqa: E402,F401
from vdx import quantattn  # noqa: E402
from vdx.options import RECORD_KEYS, check_quant_attn, info_options, quant_attn_record, resolve  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args  # noqa: E402


@pytest.mark.parametrize("md", [0, 3, 16, 2.0, True, None, "2"], ids=repr)
def test_check_params_refuses(md):
    with pytest.raises(ValueError):
        quantattn.check_params(md)


def test_levels_at_the_headline_frame():
    assert quantattn.check_params() == {"mode": "qk_int8", "max_downsample": 1}
    assert quantattn.levels(quantattn.check_params(1), 72, 128) == [{"down": 1, "tokens": 9216, "blocks": 144}]
    assert quantattn.levels(quantattn.check_params(8), 72, 128)[1:] == [
        {"down": 2, "tokens": 2304, "blocks": 36}, {"down": 4, "tokens": 576, "blocks": 9}, {"down": 8, "tokens": 144, "blocks": 3}]
    assert quantattn.levels(quantattn.check_params(2), 9, 9) == [{"down": 1, "tokens": 81, "blocks": 2}, {"down": 2, "tokens": 25, "blocks": 1}]


@pytest.mark.parametrize("kw", [
    dict(quant_attn=1), dict(quant_attn="on"), dict(quant_attn=True, quant_attn_max_downsample=3),
    dict(quant_attn_max_downsample=2),                            # needs quant_attn
    dict(quant_attn=True, tome=0.5), dict(quant_attn=True, hypertile=(2, 2)), dict(quant_attn=True, cross_frame="first"),
    dict(quant_attn=True, kv_downsample=2),
], ids=str)
def test_check_quant_attn_refuses(kw):
    cfg = DiffuserConfig(**{**dict(height=576, width=1024), **kw})
    with pytest.raises(ValueError):
        check_quant_attn(cfg)
    with pytest.raises(ValueError):
        resolve(cfg, "allgather", 1)


def test_record_only_when_set():
    assert "quant_attn" not in RECORD_KEYS
    off = resolve(DiffuserConfig(height=576, width=1024), "allgather", 1)
    assert off.quant_attn is None and quant_attn_record(off) == {} and "quant_attn" not in info_options(off, [])
    on = resolve(DiffuserConfig(height=576, width=1024, quant_attn=True, quant_attn_max_downsample=2), job=True)
    want = {"mode": "qk_int8", "max_downsample": 2, "levels": quantattn.levels(quantattn.check_params(2), 72, 128)}
    assert on.quant_attn == want and quant_attn_record(on) == {"quant_attn": want} == quant_attn_record({"quant_attn": want, "x": 1})
    assert info_options(on, [])["quant_attn"] == want
    tiled = check_quant_attn(DiffuserConfig(height=576, width=1024, quant_attn=True, co_denoise=True, tile=(192, 320)))
    assert tiled["levels"] == [{"down": 1, "tokens": 24 * 40, "blocks": 15}]          # the UNet's frame is the tile

    p = build_arg_parser()                                        # the flags reach the fields
    base = ["--prompt", "x"] if any(a.dest == "prompt" and a.required for a in p._actions) else []
    cfg = config_from_args(p.parse_args(base + ["--quant_attn", "--quant_attn_max_downsample", "4"]))
    assert cfg.quant_attn is True and cfg.quant_attn_max_downsample == 4
    assert config_from_args(p.parse_args(base)).quant_attn is False
