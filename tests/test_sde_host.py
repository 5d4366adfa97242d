"""Host tests of the stochastic samplers (vdx/scheduler.py, vdx/noise.py `stream_of_step`, vdx/options.py `check_eta`): the
restatement tests/sde_ref.py at eta 0 against the deterministic ones, a box's noise against the clip's, the streams, every refusal
of the option, its record, and the scheduler the front end builds."""
import math

import numpy as np
import pytest
import torch

import codenoise_ref
import dpm_ref as D
import noise_ref as N
import sde_ref as R

import vdx  # noqa: F401
from vdx import noise, options
from vdx.pipeline import SCHEDULERS, DiffuserConfig, build_arg_parser, config_from_args, make_scheduler
from vdx.scheduler import _STEPS, DDIMScheduler, DPMSolverMultistepScheduler, SDEDPMSolverMultistepScheduler


def _tensors(seed=0, shape=(1, 4, 3, 5, 4)):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*shape, generator=g).half() for _ in range(3))


def test_eta_zero_has_the_bits_of_the_deterministic_restatements():
    e, x, _ = _tensors()
    s = DDIMScheduler()
    s.set_timesteps(5)
    assert s._host_timesteps == [int(t) for t in R.ddim_timesteps(5)]
    for t in s._host_timesteps:                                         # tests/codenoise_ref.py holds the DDIM (eta 0) restatement
        k = R.ddim_scalars(t, 5, 0.0)
        assert k["std"] == 0.0 and (k["s1"], k["sa"], k["sp"], k["dir"]) == s.coefficients(t)
        want = codenoise_ref.ddim_chain(e, x, s.coefficients(t))
        assert torch.equal(R.ddim_step(e, x, k).view(torch.int16), want.view(torch.int16)), t
    # the scheduler's coefficients at eta 0 are the deterministic ones; at eta > 0 the restatement's
    for t in s._host_timesteps:
        assert s.eta_coefficients(t, 0.0) == (s.coefficients(t), 0.0)
        for eta in (0.3, 1.0):
            k = R.ddim_scalars(t, 5, eta)
            assert s.eta_coefficients(t, eta) == ((k["s1"], k["sa"], k["sp"], k["dir"]), k["std"]) and 0 < k["std"] < 1
    # SDE-DPM-Solver++ with its noise and the SDE's factors taken out is dpm_ref's step: same x0, and the chain adds where dpm_ref subtracts
    sig = D.sigmas(5)
    e, x, p = _tensors(1)
    for i, second in ((0, False), (2, True), (3, False)):
        kd, ks = D.scalars(sig, i, second), R.sde_scalars(sig, i, second)
        as_sde = dict(kd, k=-kd["k"], cn=0.0, **({"half_k": -kd["half_k"]} if second else {}))
        got, got_x0 = R.sde_step(e, x, p if second else None, as_sde, None)
        want, want_x0 = D.step(e, x, p if second else None, kd)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and torch.equal(got_x0.view(torch.int16), want_x0.view(torch.int16))
        assert (ks["s0"], ks["inv_a0"]) == (kd["s0"], kd["inv_a0"]) and ks["cn"] > 0 and ks["cx"] < kd["cx"]


def test_sde_coefficients_equal_the_restatement_and_the_last_step_is_x0():
    s = SDEDPMSolverMultistepScheduler()
    assert s.stochastic and s.config.algorithm_type == "sde-dpmsolver++" and not DPMSolverMultistepScheduler().stochastic
    for n in (2, 5, 25):
        s.set_timesteps(n)
        sig = D.sigmas(n)
        for i in range(n):
            for second in ([False, True] if 0 < i < n - 1 else [False]):
                assert s.sde_coefficients(i, second) == R.sde_coeffs(R.sde_scalars(sig, i, second)), (n, i, second)
        c, c_n = s.sde_coefficients(n - 1, False)
        assert (c[2], c[3], c_n) == (0.0, 1.0, 0.0)
        assert s._step_coefficients(n - 1, False) == (s.coefficients(n - 1, False), None)       # the deterministic kernel, no draw
    via = DPMSolverMultistepScheduler.from_config(DDIMScheduler().config, algorithm_type="sde-dpmsolver++")
    again = DPMSolverMultistepScheduler.from_config(via.config)
    assert via.stochastic and again.stochastic and again.config.algorithm_type == "sde-dpmsolver++"
    assert type(via) is type(again) is SDEDPMSolverMultistepScheduler and vars(again.config) == vars(via.config)
    assert type(SDEDPMSolverMultistepScheduler.from_config(vars(via.config))) is SDEDPMSolverMultistepScheduler
    back = DPMSolverMultistepScheduler.from_config(via.config, algorithm_type="dpmsolver++")
    assert type(back) is DPMSolverMultistepScheduler and not back.stochastic
    assert type(SDEDPMSolverMultistepScheduler.from_config(DDIMScheduler().config)) is SDEDPMSolverMultistepScheduler
    # the plain class runs its own algorithm only, as it always did, and says where the stochastic one lives; each refuses the other's
    with pytest.raises(NotImplementedError, match="SDEDPMSolverMultistepScheduler"):
        DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    for cls, kw in ((DPMSolverMultistepScheduler, dict(algorithm_type="sde-dpmsolver")), (SDEDPMSolverMultistepScheduler, dict(algorithm_type="dpmsolver++")),
                    (SDEDPMSolverMultistepScheduler, dict(solver_order=3))):
        with pytest.raises(NotImplementedError):
            cls(**kw)
    assert SDEDPMSolverMultistepScheduler(solver_order=1).config.solver_order == 1


def test_a_box_draws_the_slice_of_the_clip():
    shape, seed, stream = (1, 4, 5, 3, 3), 0x89ABCDEF01234567, R.stream_of_step(0, 7)
    whole = R.clip_noise(shape, seed, stream)
    assert torch.equal(whole.view(torch.int16), torch.from_numpy(N.normal(shape, seed, stream)).view(torch.int16))
    for s, L in ((0, 5), (1, 2), (4, 1)):
        assert torch.equal(R.clip_noise(shape, seed, stream, (s, L)).view(torch.int16), whole[:, :, s:s + L].contiguous().view(torch.int16))
    # the kernel's map: logical = i + c (T - L) HW + s HW
    C_, T, HW, s, L = 4, 5, 9, 1, 2
    i = np.arange(C_ * L * HW)
    logical = i + (i // (L * HW)) * (T - L) * HW + s * HW
    box = ((0, 0, s, 0, 0), (1, C_, L, 3, 3))
    assert np.array_equal(logical.astype(np.uint64), N.box_indices(shape, box).reshape(-1))


def test_stream_of_step():
    assert noise.STREAM_SAMPLER == 2 ** 33 == R.STREAM_SAMPLER
    assert noise.stream_of_step(0, 0) == 2 ** 33 and noise.stream_of_step(0, 49) == 2 ** 33 + 49
    assert noise.stream_of_step(2, 3) == 2 ** 33 + 2 * 2 ** 16 + 3 == R.stream_of_step(2, 3)
    assert noise.stream_of_step(noise.STREAM_ROUND_MAX, noise.STREAM_STEP_MAX) < 2 ** 64
    assert noise.stream_of_step(1, 0) > noise.stream_of_step(0, noise.STREAM_STEP_MAX) > noise.STREAM_POSTERIOR
    for bad in ((-1, 0), (0, -1), (0, 2 ** 16), (2 ** 30, 0), (True, 0), (0, 1.0), ("0", 0), (None, 0)):
        with pytest.raises(ValueError):
            noise.stream_of_step(*bad)


def test_scheduler_surface():
    assert _STEPS["one", "noise"] == (None, ("cfg_ddim_eta_step", "cfg_sde_dpm_step"))
    assert _STEPS["windows", "noise"] == (None, ("cofuse_cfg_ddim_eta_step", "cofuse_cfg_sde_dpm_step"))
    s = DDIMScheduler()
    assert s.eta == 0.0 and DDIMScheduler(eta=0.25).eta == 0.25
    for bad in (-0.1, 1.5, float("nan"), "1", True):
        with pytest.raises(ValueError):
            DDIMScheduler(eta=bad)
    s.seed_noise(5, 2)
    assert s._noise_seed == (5, 2) and s._draw(0.5, 3) == (0.5, 5, noise.stream_of_step(2, 3))
    s.seed_noise(None)
    with pytest.raises(ValueError, match="seed_noise"):
        s._draw(0.5, 3)
    for bad in ((-1, 0), (2 ** 64, 0), (1, -1), (1.0, 0)):
        with pytest.raises(ValueError):
            s.seed_noise(*bad)


def _cfg(**kw):
    return DiffuserConfig(**{"noise": "philox", **kw})


def test_check_eta_refusals_and_record():
    assert options.check_eta(DiffuserConfig()) is None and options.check_eta(_cfg(scheduler="dpmpp_2m")) is None
    assert options.check_eta(_cfg(eta=0.5)) == {"eta": 0.5, "algorithm": "ddim"}
    assert options.check_eta(_cfg(eta=1, seed=3)) == {"eta": 1.0, "algorithm": "ddim"}
    for eta in (0.0, 1.0):
        assert options.check_eta(_cfg(eta=eta, scheduler="dpmpp_2m_sde")) == {"eta": 1.0, "algorithm": "sde-dpmsolver++"}
    for bad in (-0.5, 1.01, float("nan"), float("inf"), "0.5", True, None):
        with pytest.raises(ValueError, match="eta"):
            options.check_eta(_cfg(eta=bad))
    with pytest.raises(ValueError, match="0 or 1"):
        options.check_eta(_cfg(eta=0.5, scheduler="dpmpp_2m_sde"))
    with pytest.raises(ValueError, match="deterministic"):
        options.check_eta(_cfg(eta=0.5, scheduler="dpmpp_2m"))
    for kw in (dict(eta=0.5), dict(scheduler="dpmpp_2m_sde")):
        with pytest.raises(ValueError, match="no per-step form"):
            options.check_eta(DiffuserConfig(**kw))
    for kw, name in ((dict(guidance_rescale=0.5), "guidance_rescale"), (dict(cfg_mimic=4.0), "cfg_mimic"),
                     (dict(co_denoise=True, tile=(128, 128)), "tile"), (dict(co_denoise=True, loop=True), "loop"),
                     (dict(co_denoise=True, context_stride=2), "context_stride")):
        with pytest.raises(ValueError, match=f"eta and {name} exclude each other.*no .* noise form yet"):
            options.check_eta(_cfg(eta=1.0, **kw))
        with pytest.raises(ValueError, match=f"eta and {name} exclude"):
            options.check_eta(_cfg(scheduler="dpmpp_2m_sde", **kw))
    # `resolve` runs it, after `check_noise`
    with pytest.raises(ValueError, match="no per-step form"):
        options.resolve(DiffuserConfig(eta=0.5, num_frames=8, chunk_size=6, overlap=2), world=1)
    with pytest.raises(ValueError, match="needs noise"):                # check_noise speaks first
        options.resolve(DiffuserConfig(eta=0.5, seed=1, num_frames=8, chunk_size=6, overlap=2), world=1)
    on = options.resolve(_cfg(eta=0.5, num_frames=8, chunk_size=6, overlap=2), world=1)
    off = options.resolve(_cfg(num_frames=8, chunk_size=6, overlap=2), world=1)
    assert on.sampler_noise == {"eta": 0.5, "algorithm": "ddim"} and off.sampler_noise is None
    assert options.sampler_noise_record(on) == {"sampler_noise": {"eta": 0.5, "algorithm": "ddim"}} and options.sampler_noise_record(off) == {}
    assert options.sampler_noise_record({"sampler_noise": 1, "x": 2}) == {"sampler_noise": 1} and options.sampler_noise_record({}) == {}
    assert options.info_options(on, None)["sampler_noise"] == on.sampler_noise and "sampler_noise" not in options.info_options(off, None)
    assert "sampler_noise" not in options.RECORD_KEYS and "eta" not in options.RECORD_KEYS


def test_front_end():
    assert SCHEDULERS == ("ddim", "dpmpp_2m", "dpmpp_2m_sde") and DiffuserConfig().eta == 0.0
    parse = lambda argv: config_from_args(build_arg_parser().parse_args(argv))      # noqa: E731
    assert parse([]).eta == 0.0 and parse(["--eta", "0.5", "--seed", "3"]).eta == 0.5
    cfg = parse(["--scheduler", "dpmpp_2m_sde", "--seed", "3"])
    assert cfg.scheduler == "dpmpp_2m_sde" and cfg.noise == "philox" and options.check_eta(cfg)["eta"] == 1.0
    base = DDIMScheduler()
    sde = make_scheduler("dpmpp_2m_sde", base)
    assert type(sde) is SDEDPMSolverMultistepScheduler and sde.stochastic and sde.config.solver_order == 2
    assert make_scheduler("dpmpp_2m_sde", sde) is sde and make_scheduler("ddim", base) is base
    det = make_scheduler("dpmpp_2m", base)
    assert not det.stochastic and make_scheduler("dpmpp_2m", det) is det and not make_scheduler("dpmpp_2m", sde).stochastic
    assert torch.equal(sde.alphas_cumprod, base.alphas_cumprod)
    with pytest.raises(ValueError):
        make_scheduler("dpmpp_sde", base)
    assert math.isfinite(DiffuserConfig().eta)
