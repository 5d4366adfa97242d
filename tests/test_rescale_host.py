"""Negative prompts and CFG rescale without a GPU: the refusals, the flags, the defaults, what the tokenizer is handed, and the
restatement's own property (tests/rescale_ref.py)."""
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import rescale_ref as R  # noqa: E402
import vdx  # noqa: E402,F401
from vdx import ops  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, check_guidance_rescale, config_from_args, run_job  # noqa: E402


def test_defaults_and_the_flags_round_trip():
    cfg = DiffuserConfig()
    assert cfg.negative_prompt == "" and cfg.guidance_rescale == 0.0 and check_guidance_rescale(cfg) == 0.0
    a = build_arg_parser().parse_args([])
    assert a.negative_prompt == "" and a.guidance_rescale == 0.0
    assert config_from_args(a) == cfg
    cfg = config_from_args(build_arg_parser().parse_args(["--negative_prompt", "watermark, text", "--guidance_rescale", "0.7"]))
    assert cfg.negative_prompt == "watermark, text" and cfg.guidance_rescale == 0.7 and check_guidance_rescale(cfg) == 0.7


@pytest.mark.parametrize("phi", [-0.1, 1.0000001, float("nan"), float("inf"), -float("inf"), "0.5", None, True])
def test_values_outside_the_unit_interval_are_refused(phi):
    with pytest.raises(ValueError, match="guidance_rescale"):
        check_guidance_rescale(DiffuserConfig(guidance_rescale=phi))


@pytest.mark.parametrize("gs", [1.0, 0.5, 0.0, float("nan")])
def test_rescale_needs_a_guidance_scale_above_one(gs):
    with pytest.raises(ValueError, match="guidance_scale"):
        check_guidance_rescale(DiffuserConfig(guidance_rescale=0.7, guidance_scale=gs))
    assert check_guidance_rescale(DiffuserConfig(guidance_rescale=0.0, guidance_scale=gs)) == 0.0     # off: nothing to refuse
    assert check_guidance_rescale(DiffuserConfig(guidance_rescale=1, guidance_scale=1.0001)) == 1.0


def test_refused_before_anything_loads():
    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"the pipeline was touched ({name}) before the refusal")
    with pytest.raises(ValueError, match="guidance_scale"):
        run_job(DiffuserConfig(guidance_rescale=0.7, guidance_scale=1.0), pipe=Boom())
    with pytest.raises(ValueError, match="guidance_rescale"):
        run_job(DiffuserConfig(guidance_rescale=1.5), pipe=Boom())


@pytest.mark.parametrize("phi", [0.0, 0.3, 0.7, 1.0, 0.9, 1e-9, 1 - 2.0 ** -30])
def test_the_two_scalars_are_formed_in_double_and_rounded_once(phi):
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]     # noqa: E731
    got = ops.rescale_factors(phi)
    assert got == (f32(phi), f32(1.0 - phi)) == R.factors(phi)
    assert all(0.0 <= v <= 1.0 and math.isfinite(v) for v in got)
    # NOT 1 - fp32(phi) in fp32: at phi = 0.9 the two differ in the last bit of fp32 ...
    if phi == 0.9:
        assert float(np.float32(1.0) - np.float32(phi)) != got[1]
    # ... and a phi that fp32 rounds to 1.0 keeps a non-negative partner
    if phi == 1 - 2.0 ** -30:
        assert got == (1.0, f32(2.0 ** -30))


def test_the_tokenizer_is_handed_the_negative_prompt():
    seen = []

    class Stop(Exception):
        pass

    class Tok:
        model_max_length = 77

        def __call__(self, texts, **kw):
            seen.append((list(texts), kw))
            raise Stop

    class Pipe:
        tokenizer = Tok()

        class _M:
            def to(self, dev):
                return self
        unet = text_encoder = vae = _M()

    for neg in ("", "watermark, text"):
        with pytest.raises(Stop):
            run_job(DiffuserConfig(prompt="a rocket", negative_prompt=neg, device="cpu"), pipe=Pipe())
    assert [s[0] for s in seen] == [["a rocket", ""], ["a rocket", "watermark, text"]]
    assert seen[0][1] == seen[1][1] == dict(padding="max_length", max_length=77, truncation=True, return_tensors="pt")
    with pytest.raises(ValueError, match="negative_prompt"):
        run_job(DiffuserConfig(negative_prompt=None, device="cpu"), pipe=Pipe())


@pytest.mark.parametrize("gs", [2.0, 7.5, 12.0])
def test_full_rescale_gives_the_conditional_noise_its_standard_deviation(gs):
    """The restatement's own property, in float64 before its roundings: with phi = 1 the rescaled noise has std(c); with phi = 0 it
    is g; in between its deviation lies between the two."""
    eps2 = torch.randn(2, 4, 3, 5, 7, generator=torch.Generator().manual_seed(3)).half()
    c, g = eps2[1:].double(), R.dpm_ref.cfg_combine(eps2, gs).double()
    full = R.rescale_f64(eps2, gs, 1.0)
    assert abs(float(full.std() / c.std()) - 1.0) < 1e-12
    assert torch.equal(R.rescale_f64(eps2, gs, 0.0), g)
    mid = float(R.rescale_f64(eps2, gs, 0.5).std())
    assert float(c.std()) < mid < float(g.std())
    # and the rounded chain stays within fp16's reach of it: three roundings of values of g's size
    got = R.rescaled(eps2, gs, 1.0).double()
    assert float((got - full).abs().max()) <= 4 * 2.0 ** -11 * float(g.abs().max())


def test_degenerate_samples_do_what_the_expression_says():
    one = torch.tensor([[1.0], [2.0]]).half()                     # N = 1: no variance
    assert all(np.isnan(v) for v in R.stats(one, 7.5))
    eps2 = torch.randn(2, 64, generator=torch.Generator().manual_seed(1)).half()
    const_c = eps2.clone()
    const_c[1] = 0.5                                              # sd_c = 0: r = 0, and g' = (1 - phi) g
    sd_c, sd_g, r = R.stats(const_c, 7.5)
    assert sd_c == 0 and sd_g > 0 and r == 0
    same = torch.full((2, 64), 0.25).half()                       # g constant too: 0 / 0
    assert np.isnan(R.stats(same, 7.5)[2])
    assert bool(torch.isnan(R.rescaled(same, 7.5, 0.7)).all())
