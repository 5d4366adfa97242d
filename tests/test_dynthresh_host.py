"""Dynamic thresholding with a mimic scale without a GPU: `mimic_factors`, every refusal and its message, the flags through the
config to `resolve`, the records only when set, the rule table untouched, and the restatement's own properties
(tests/dynthresh_ref.py)."""
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dynthresh_ref as D  # noqa: E402
import vdx  # noqa: E402,F401
from vdx import ops, options  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args, run_job  # noqa: E402

f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]     # noqa: E731


@pytest.mark.parametrize("ms,q,M", [(7.0, 1.0, 9216), (7.0, 0.995, 9216), (3.3, 0.5, 7), (1.1, 1 / 7, 7), (0.1, 1e-9, 2056),
                                    (7.0, 1.0, 1), (7.0, 0.3, 1), (7.0, 0.5, 2), (2.5, 0.999, (1 << 32) - 1)])
def test_mimic_factors_form_the_rank_in_double(ms, q, M):
    got = ops.mimic_factors(ms, q, M)
    pos = q * (M - 1)
    k = math.floor(pos)
    assert got == D.factors(ms, q, M)
    assert got[0] == f32(ms) and 0 <= got[1] <= M - 1 and 0.0 <= got[2] < 1.0
    assert (got[1], got[2]) == (k, f32(pos - k)) or (f32(pos - k) == 1.0 and (got[1], got[2]) == (min(k + 1, M - 1), 0.0))
    if q == 1.0:
        assert got[1:] == (M - 1, 0.0)


def test_a_fraction_that_rounds_to_one_is_the_next_rank():
    M = 3
    q = (1.0 - 2.0 ** -40) / 2                                    # pos = 1 - 2^-40: floor 0, and fp32 rounds the rest to 1.0
    assert f32(q * (M - 1)) == 1.0
    assert ops.mimic_factors(7.0, q, M)[1:] == (1, 0.0)


@pytest.mark.parametrize("ms", [0, -1.0, float("nan"), float("inf"), "7", None, True])
def test_a_scale_that_is_no_positive_finite_number_is_refused(ms):
    with pytest.raises(ValueError, match="cfg_mimic must be a finite number > 0"):
        ops.mimic_factors(ms, 1.0, 8)


@pytest.mark.parametrize("q", [0, 0.0, -0.5, 1.0000001, float("nan"), float("inf"), "0.5", None, True])
def test_a_percentile_outside_the_half_open_interval_is_refused(q):
    with pytest.raises(ValueError, match=r"cfg_mimic_percentile must be a number in \(0, 1\]"):
        ops.mimic_factors(7.0, q, 8)
    with pytest.raises(ValueError, match="cfg_mimic_percentile"):
        options.check_cfg_mimic(DiffuserConfig(cfg_mimic=7.0, cfg_mimic_percentile=q))


@pytest.mark.parametrize("M", [0, -3, 1 << 32, 2.0])
def test_a_channel_size_the_counts_cannot_hold_is_refused(M):
    with pytest.raises(ValueError, match="2\\^32"):
        ops.mimic_factors(7.0, 1.0, M)


def test_defaults_and_the_flags_round_trip():
    cfg = DiffuserConfig()
    assert cfg.cfg_mimic is None and cfg.cfg_mimic_percentile == 1.0 and options.check_cfg_mimic(cfg) is None
    a = build_arg_parser().parse_args([])
    assert a.cfg_mimic is None and a.cfg_mimic_percentile == 1.0 and config_from_args(a) == cfg
    cfg = config_from_args(build_arg_parser().parse_args(["--cfg_mimic", "7", "--cfg_mimic_percentile", "0.995", "--guidance_scale", "15"]))
    assert cfg.cfg_mimic == 7.0 and cfg.cfg_mimic_percentile == 0.995 and cfg.guidance_scale == 15
    want = {"scale": 7.0, "percentile": 0.995}
    assert options.check_cfg_mimic(cfg) == want
    for job in (False, True):
        opts = options.resolve(cfg, world=1, job=job)
        assert opts.cfg_mimic == want and options.mimic_record(opts) == {"cfg_mimic": want}
        assert options.info_options(opts, [])["cfg_mimic"] == want
        off = options.resolve(DiffuserConfig(), world=1, job=job)
        assert off.cfg_mimic is None and options.mimic_record(off) == {} and "cfg_mimic" not in options.info_options(off, [])
    assert options.JobOptions.__dataclass_fields__["cfg_mimic"].default is None
    assert options.mimic_record({"cfg_mimic": want, "x": 1}) == {"cfg_mimic": want} and options.mimic_record({"x": 1}) == {}
    # ms > gs is a valid request: the range is then widened, not squeezed
    assert options.check_cfg_mimic(DiffuserConfig(cfg_mimic=12.0, guidance_scale=3.0)) == {"scale": 12.0, "percentile": 1.0}


REFUSALS = [
    (dict(cfg_mimic=7.0, guidance_scale=1.0), "cfg_mimic 7.0 needs guidance_scale > 1, got 1.0"),
    (dict(cfg_mimic=7.0, guidance_scale=0.5), "needs guidance_scale > 1"),
    (dict(cfg_mimic=7.0, guidance_rescale=0.7), "cfg_mimic and guidance_rescale exclude each other: both rewrite the guided noise"),
    (dict(cfg_mimic=7.0, co_denoise=True, tile=(128, 128), height=256, width=256),
     "cfg_mimic and tile exclude each other: the thresholding's statistics pass has no tiled form yet"),
    (dict(cfg_mimic=7.0, co_denoise=True, loop=True),
     "cfg_mimic and loop exclude each other: the thresholding's statistics pass has no ring form yet"),
    (dict(cfg_mimic=7.0, co_denoise=True, context_stride=2),
     "cfg_mimic and context_stride exclude each other: the thresholding's statistics pass has no strided form yet"),
    (dict(cfg_mimic_percentile=0.99), "cfg_mimic_percentile 0.99 needs cfg_mimic"),
    (dict(cfg_mimic=-2.0), "cfg_mimic must be a finite number > 0, got -2.0"),
    (dict(cfg_mimic=7.0, cfg_mimic_percentile=0.0), "cfg_mimic_percentile must be a number in (0, 1], got 0.0"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[m[:40] for _, m in REFUSALS])
def test_every_refusal_and_its_message(kw, message):
    cfg = DiffuserConfig(**kw)
    with pytest.raises(ValueError) as err:
        options.check_cfg_mimic(cfg)
    assert message in str(err.value)


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[m[:40] for _, m in REFUSALS])
def test_refused_before_anything_loads(kw, message):
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the pipeline was touched ({name}) before the refusal")
    with pytest.raises(ValueError) as err:
        run_job(DiffuserConfig(**kw), pipe=Boom())
    assert message in str(err.value)


def test_the_rule_table_and_the_record_keys_are_untouched():
    assert set(options.RULES) == {"co_denoise", "tile", "loop", "context_stride"}
    assert not any("mimic" in str(row) for rows in options.RULES.values() for row in rows)
    assert set(options._IS_ON) == {"tile", "loop", "guidance_rescale"}
    assert options.RECORD_KEYS == ("freeu", "tome", "co_denoise", "tile", "loop", "context_stride", "mask", "negative_prompt",
                                   "guidance_rescale")
    assert options.record_options({"cfg_mimic": {"scale": 7.0, "percentile": 1.0}, "freeu": 1}) == {"freeu": 1}


def test_it_goes_with_everything_else():
    cfg = DiffuserConfig(cfg_mimic=7.0, guidance_scale=15.0, co_denoise=True, negative_prompt="blurry", freeu=(1.1, 1.2, 0.9, 0.2),
                         tome=0.5, free_init_iters=2, scheduler="dpmpp_2m", prompt_syntax="a1111", prompt_travel=((8, "a cat"),))
    assert options.resolve(cfg, world=1, job=True).cfg_mimic == {"scale": 7.0, "percentile": 1.0}


# ---- the restatement's own properties -------------------------------------------------------------------------------------------
def _eps2(seed, shape=(3, 2, 5, 7)):
    return torch.randn((2,) + shape, generator=torch.Generator().manual_seed(seed)).half()


@pytest.mark.parametrize("gs,ms", [(15.0, 7.0), (7.5, 3.0), (2.0, 1.5)])
def test_full_percentile_squeezes_every_channel_into_the_mimic_range(gs, ms):
    """q = 1: s is at least the channel's largest |d|, nothing is clamped, and the result's deviation from mg is d * ref_lo / s up to
    three fp16 roundings: its largest magnitude is ref_lo's, the mimic scale's range, and the channel means are the high scale's."""
    eps2 = _eps2(5)
    scal = D.stats(eps2, gs, ms, 1.0)
    sc = scal.view(np.float16).astype(np.float64)
    out = D.threshold_with_scal(eps2, gs, scal).double().reshape(3, -1)
    g = D.combines(eps2, gs, ms)[0].double()
    for ch in range(3):
        mg, ref_lo, ref_hi, s = sc[ch]
        assert s == max(ref_lo, ref_hi) and ref_lo < ref_hi                 # gs > ms: the high scale's range is the wider one
        want = (g[ch] - mg) * ref_lo / s + mg
        assert float((out[ch] - want).abs().max()) <= 4 * 2.0 ** -11 * (ref_lo + abs(mg))
        assert abs(float((out[ch] - mg).abs().max()) - ref_lo) <= 4 * 2.0 ** -11 * (ref_lo + abs(mg))


def test_a_lower_percentile_clamps_and_a_higher_mimic_scale_widens():
    eps2 = _eps2(6)
    hi = D.stats(eps2, 15.0, 7.0, 1.0).view(np.float16).astype(np.float64)
    lo = D.stats(eps2, 15.0, 7.0, 0.5).view(np.float16).astype(np.float64)
    assert (lo[:, 2] < hi[:, 2]).all() and (lo[:, 1] == hi[:, 1]).all() and (lo[:, 0] == hi[:, 0]).all()
    wide = D.stats(eps2, 2.0, 7.0, 1.0).view(np.float16).astype(np.float64)      # ms > gs: ref_lo is the larger, and s is ref_lo
    assert (wide[:, 1] > wide[:, 2]).all() and (wide[:, 3] == wide[:, 1]).all()


def test_the_interpolated_rank_lies_between_its_neighbours_and_matches_a_sort():
    eps2 = _eps2(7, (1, 1, 3, 4))
    means = D.means_of(D.sums64(eps2, 7.5, 3.0)[0], 12)
    d, _ = D.deviations(eps2, 7.5, 3.0, means)
    a = np.sort(np.abs(d[0].numpy().astype(np.float64)))
    for q in (1.0, 0.995, 0.5, 1 / 12, 1e-9):
        _, k, f = D.factors(3.0, q, 12)
        got = float(D.select(eps2, 7.5, 3.0, q, means)[0].view(np.float16)[2])
        assert a[k] <= got <= a[min(k + 1, 11)]
        assert abs(got - (a[k] + f * (a[min(k + 1, 11)] - a[k]))) <= 2.0 ** -11 * a[-1]


def test_degenerate_channels_do_what_the_expression_says():
    eps2 = _eps2(8)
    eps2[:, 1] = 0.25                                             # channel 1 constant: d = 0, s = 0, 0 / 0
    out = D.threshold_with_scal(eps2, 7.5, D.stats(eps2, 7.5, 3.0, 1.0))
    nan = torch.isnan(out[0])
    assert bool(nan[1].all()) and not bool(nan[0].any()) and not bool(nan[2].any())
    bad = _eps2(8)
    bad[1, 2, 0, 1, 1] = float("inf")
    bad[0, 0, 1, 2, 3] = float("nan")
    out = D.threshold_with_scal(bad, 7.5, D.stats(bad, 7.5, 3.0, 0.9))
    fin = torch.isfinite(out[0])
    assert not bool(fin[0].any()) and bool(fin[1].all()) and not bool(fin[2].any())
