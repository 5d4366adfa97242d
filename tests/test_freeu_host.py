"""FreeU on the host: the projection form the kernels run against the literal FFT form (tests/freeu_ref.py), what FreeU does to the
oracle, argument validation, the driver's flag and field, and the diffusers shim's switches.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import freeu_ref as R  # noqa: E402

TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
SETTING = dict(b1=1.2, b2=1.4, s1=0.9, s2=0.2)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (5, 9), (9, 16), (18, 32)])
def test_projection_form_is_the_literal_form(H, W):
    """Pins K_N = {0, -1 mod N}: one frequency for N = 1, the whole axis for N = 2."""
    g = torch.Generator().manual_seed(H * 37 + W)
    x = torch.randn(3, 5, H, W, generator=g, dtype=torch.float64) + 3.0
    for s in (0.9, 0.2, 0.0, -1.5):
        d = float((R.fourier_filter_projection(x, s) - R.fourier_filter_ref(x, s)).abs().max())
        print(f"{H}x{W} s={s}: largest difference {d:.2e}")
        assert d <= 1e-13
    assert float((R.fourier_filter_ref(x, 1.0) - x).abs().max()) <= 1e-15 * float(x.abs().max())
    assert torch.equal(R.fourier_filter_projection(x, 1.0), x)
    assert R.masked_frequencies(1) == [0] and R.masked_frequencies(2) == [0, 1] and R.masked_frequencies(9) == [0, 8]


def test_the_real_part_is_not_redundant():
    """Frequency -1 is scaled without +1: the filtered spectrum is not Hermitian."""
    x = torch.randn(5, 9, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    f = torch.fft.fftshift(torch.fft.fft2(x))
    mask = torch.ones(5, 9, dtype=torch.float64)
    mask[1:3, 3:5] = 0.2
    assert float(torch.fft.ifft2(torch.fft.ifftshift(f * mask)).imag.abs().max()) > 1e-3


def test_twiddle_tables():
    import vdx  # noqa: F401
    from vdx import ops
    for n in (1, 2, 3, 4, 9, 16, 18, 32):
        tw = ops.freeu_twiddles(n)
        j = torch.arange(n, dtype=torch.float64)
        want = torch.stack([torch.cos(2 * torch.pi * j / n), -torch.sin(2 * torch.pi * j / n)], 1)
        assert tw.dtype == torch.float64 and tw.shape == (n, 2) and float((tw - want).abs().max()) < 2e-16
    assert ops.freeu_twiddles(2).tolist() == [[1.0, 0.0], [-1.0, 0.0]]
    assert ops.freeu_twiddles(4).tolist() == [[1.0, 0.0], [0.0, -1.0], [-1.0, 0.0], [0.0, 1.0]]


def test_make_case_leaves_no_undecided_tie():
    """The GPU test's inputs: no restated value within TIE_DISTANCE of a rounding boundary unless the tie is exact (s = 0)."""
    for H, W in R.PLANES[:8]:
        for s in (0.9, 0.2, 0.0):
            x, want16, want64 = R.make_case(H, W, 40, 3, s)
            near = R.tie_distance(want64) < R.TIE_DISTANCE
            assert s == 0.0 or not near.any()
            proj = R.fourier_filter_projection(x, s)
            assert float((proj - want64).abs().max()) < 2e-14
            assert R.differing(R.to_fp16(proj), want16) == 0


def test_scale_ref_is_the_fp32_product_rounded_once():
    import numpy as np
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16).reshape(-1, 2)
    for b in (1.2, 1.4, 1.0):
        got = R.scale_ref(x, b)
        with np.errstate(all="ignore"):
            want = torch.from_numpy((x[:, 0].numpy().astype(np.float32) * np.float32(b)).astype(np.float16))
        same = (got[:, 0].view(torch.int16) == want.view(torch.int16)) | (got[:, 0].isnan() & want.isnan())
        assert bool(same.all()) and torch.equal(got[:, 1].view(torch.int16), x[:, 1].view(torch.int16))


@pytest.fixture(scope="module")
def oracle_runs():
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg, synthetic_state_dict
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    g = torch.Generator().manual_seed(21)
    sample = torch.randn(2, 4, 5, 16, 32, generator=g).half().float()
    ehs = torch.randn(2, 77, TINY["cross"], generator=g).half().float()

    def run(setting):
        m = UNet3DConditionModelRef(RefCfg.tiny(**TINY)).eval()
        m.load_state_dict({k: v.half().float() for k, v in sd.items()})
        if setting is not None:
            R.with_freeu(m, **setting)
        with torch.no_grad():
            return m(sample, torch.tensor(7), ehs).sample
    return run, run(None)


def test_freeu_moves_the_oracle(oracle_runs):
    """What makes the GPU parity test mean something: at this shape the full setting moves the output by 0.18 rel-L2, the s factors
    alone by 0.09, the b factors alone by 0.16, and (1, 1, 1, 1) by nothing."""
    run, plain = oracle_runs
    for setting, least in ((SETTING, 0.05), (dict(SETTING, b1=1.0, b2=1.0), 0.05), (dict(SETTING, s1=1.0, s2=1.0), 0.05)):
        d = rel_l2(run(setting), plain)
        print(f"{setting}: rel-L2 {d:.3f} from the plain oracle")
        assert d > least
    assert rel_l2(run(dict(b1=1.0, b2=1.0, s1=1.0, s2=1.0)), plain) < 1e-6


def test_enable_freeu_validates_and_keeps_state():
    import vdx  # noqa: F401
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    m = UNet3DConditionModel(UNet3DConfig(block_out_channels=TINY["ch"], cross_attention_dim=TINY["cross"],
                                          transformer_in_heads=TINY["in_heads"]))
    assert m.freeu is None
    m.enable_freeu(0.9, 0.2, 1.2, 1.4)                                     # diffusers' order: s1, s2, b1, b2
    assert m.freeu == dict(b1=1.2, b2=1.4, s1=0.9, s2=0.2)
    m.enable_freeu(b2=1.1, s1=0.0, b1=1.0, s2=-0.5)                        # keywords; s = 0 and a negative s are allowed
    assert m.freeu == dict(b1=1.0, b2=1.1, s1=0.0, s2=-0.5)
    for bad in (dict(b1=0.0), dict(b2=-1.0), dict(b1=float("nan")), dict(s1=float("inf")), dict(s2=float("nan")),
                dict(b2=float("inf")), dict(s1="0.9"), dict(b1=None), dict(b1=True)):
        with pytest.raises(ValueError):
            m.enable_freeu(**{**SETTING, **bad})
        assert m.freeu == dict(b1=1.0, b2=1.1, s1=0.0, s2=-0.5)           # a refused call changes nothing
    m.disable_freeu()
    assert m.freeu is None


def test_flag_and_field():
    import vdx  # noqa: F401
    from dataclasses import fields
    from vdx.pipeline import FLAG_OF_FIELD, DiffuserConfig, build_arg_parser, check_freeu, config_from_args
    assert DiffuserConfig().freeu is None and "freeu" in {f.name for f in fields(DiffuserConfig)}
    assert FLAG_OF_FIELD.get("freeu", "freeu") == "freeu"
    p = build_arg_parser()
    assert config_from_args(p.parse_args([])).freeu is None and p.parse_args([]).freeu is None
    cfg = config_from_args(p.parse_args(["--freeu", "1.2", "1.4", "0.9", "0.2", "--free_init", "2", "--scheduler", "dpmpp_2m"]))
    assert cfg.freeu == (1.2, 1.4, 0.9, 0.2) and cfg.free_init_iters == 2 and cfg.scheduler == "dpmpp_2m"
    assert check_freeu(cfg) == dict(b1=1.2, b2=1.4, s1=0.9, s2=0.2) and check_freeu(DiffuserConfig()) is None
    assert check_freeu(DiffuserConfig(freeu=(1.0, 1.0, 0.0, 0.0))) == dict(b1=1.0, b2=1.0, s1=0.0, s2=0.0)
    for bad in ((1.2, 1.4, 0.9), (0.0, 1.4, 0.9, 0.2), (1.2, -1.0, 0.9, 0.2), (1.2, 1.4, float("nan"), 0.2),
                (1.2, 1.4, 0.9, float("inf")), 1.2, "1.2 1.4 0.9 0.2"):
        with pytest.raises(ValueError):
            check_freeu(DiffuserConfig(freeu=bad))
    with pytest.raises(SystemExit):
        p.parse_args(["--freeu", "1.2", "1.4", "0.9"])


def test_bad_setting_is_refused_before_any_work():
    import vdx  # noqa: F401
    from vdx.pipeline import DiffuserConfig, run_job

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError(f"run_job touched pipe.{name} before refusing the setting")
    with pytest.raises(ValueError, match="freeu"):
        run_job(DiffuserConfig(freeu=(0.0, 1.4, 0.9, 0.2)), pipe=Untouched())


def test_shim_switches_reach_the_unet():
    import vdx  # noqa: F401
    from vdx.compat.diffusers_shim import DiffusionPipeline
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    assert pipe.unet.freeu is None
    pipe.enable_freeu(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
    assert pipe.unet.freeu == SETTING
    pipe.disable_freeu()
    assert pipe.unet.freeu is None
    pipe.unet.enable_freeu(0.9, 0.2, 1.2, 1.4)
    assert pipe.unet.freeu == SETTING
    pipe.enable_freeu(0.5, 0.6, 1.1, 1.3)                                  # positional, diffusers' order
    assert pipe.unet.freeu == dict(b1=1.1, b2=1.3, s1=0.5, s2=0.6)
    with pytest.raises(ValueError):
        pipe.enable_freeu(0.9, 0.2, -1.0, 1.4)
    pipe.unet.disable_freeu()
    assert pipe.unet.freeu is None
