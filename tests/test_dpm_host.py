"""Host tests of the DPM-Solver++ (2M) scheduler (vdx/scheduler.py `DPMSolverMultistepScheduler`): the schedule against its
stated formula, the refused configurations, `from_config`, the shim export, and — through the torch restatement
tests/dpm_ref.py on a problem with a closed-form answer — that the stated update really is a second-order solver."""
import numpy as np
import pytest
import torch

import dpm_ref as R

STEPS = [1, 2, 10, 25, 50, 999]


def _sched(**kw):
    import vdx  # noqa: F401
    from vdx.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**kw)


@pytest.mark.parametrize("n", STEPS)
def test_schedule_matches_the_formula(n):
    s = _sched()
    s.set_timesteps(n)
    want = (np.arange(0, n + 1) * (1000 // (n + 1))).round()[::-1][:-1].astype(np.int64) + 1
    assert s._host_timesteps == [int(t) for t in want] and s.timesteps.dtype == torch.int64
    assert torch.equal(s.timesteps, torch.from_numpy(want.copy())) and len(s._host_timesteps) == n
    assert all(a > b for a, b in zip(s._host_timesteps, s._host_timesteps[1:]))
    if n == 25:
        assert s._host_timesteps[:2] == [951, 913] and s._host_timesteps[-1] == 39
        assert s._host_timesteps == list(range(951, 38, -38))
    assert s.sigmas.dtype == torch.float32 and len(s.sigmas) == n + 1 and float(s.sigmas[-1]) == 0.0
    ac = s.alphas_cumprod
    sigma_all = ((1 - ac) / ac) ** 0.5
    # (n = 999 only: timestep 1000 takes the sigma of 999, interp's clamp — tested on its own below)
    assert torch.equal(s.sigmas[:-1], sigma_all[torch.from_numpy(np.minimum(want, 999))])
    assert torch.equal(s.sigmas, R.sigmas(n)) and list(R.timesteps(n)) == s._host_timesteps
    # the last step: sigma 0 -> st/s0 = 0, at*(exp(-h)-1) = -1: the update reduces to x0
    c = s.coefficients(n - 1, False)
    assert (c[2], c[3]) == (0.0, -1.0 * (-1.0)) and c[4] == 0.0
    assert s.init_noise_sigma == 1.0 and s.order == 1 and s.scale_model_input("x", 3) == "x"


def test_coefficients_equal_the_restatement():
    s = _sched()
    for n in (2, 10, 25):
        s.set_timesteps(n)
        sig = R.sigmas(n)
        for i in range(n):
            for second in ([False, True] if i > 0 else [False]):
                k = R.scalars(sig, i, second)
                want = (k["s0"], k["inv_a0"], k["cx"], -k["k"], -k.get("half_k", 0.0), k.get("inv_r0", 0.0))
                assert s.coefficients(i, second) == want, (n, i, second)


@pytest.mark.parametrize("kw", [dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver++"), dict(solver_order=3),
                                dict(solver_type="heun"), dict(prediction_type="v_prediction"), dict(thresholding=True),
                                dict(lower_order_final=False), dict(final_sigmas_type="sigma_min"),
                                dict(timestep_spacing="trailing"), dict(steps_offset=0), dict(beta_schedule="linear")])
def test_unsupported_configuration_is_refused(kw):
    with pytest.raises(NotImplementedError):
        _sched(**kw)


def test_solver_order_one_is_accepted():
    assert _sched(solver_order=1).config.solver_order == 1


def test_from_config_round_trips_the_beta_schedule():
    import vdx  # noqa: F401
    from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    d = DDIMScheduler()
    s = DPMSolverMultistepScheduler.from_config(d.config)
    assert torch.equal(s.alphas_cumprod, d.alphas_cumprod) and torch.equal(s.alphas_cumprod, R.alphas_cumprod())
    for k in ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "steps_offset", "prediction_type",
              "timestep_spacing"):
        assert getattr(s.config, k) == getattr(d.config, k)
    assert (s.config.algorithm_type, s.config.solver_order, s.config.solver_type) == ("dpmsolver++", 2, "midpoint")
    d2 = DDIMScheduler(beta_start=0.001, beta_end=0.02)
    s2 = DPMSolverMultistepScheduler.from_config(d2.config)
    assert torch.equal(s2.alphas_cumprod, d2.alphas_cumprod) and not torch.equal(s2.alphas_cumprod, d.alphas_cumprod)
    s3 = DPMSolverMultistepScheduler.from_config(vars(s.config))          # its own config, as a dict
    assert vars(s3.config) == vars(s.config)


def test_ddim_surface_is_unchanged_by_the_shared_base():
    import vdx  # noqa: F401
    from vdx.scheduler import DDIMScheduler
    d = DDIMScheduler()
    d.set_timesteps(10)
    assert d._host_timesteps == [901, 801, 701, 601, 501, 401, 301, 201, 101, 1]
    assert d._host_timestep(torch.tensor(301)) == 301 and d._host_timestep(7) == 7
    assert d.reset() is None and d.init_noise_sigma == 1.0 and d.order == 1 and d.scale_model_input("x") == "x"


def _adv(s, t, x):
    """What `step` does around its kernel: plan the step, then (the launch having succeeded) commit it."""
    i, prev, out = s._plan(t, x)
    s._commit(i)
    return i, prev, out


def test_a_failed_launch_leaves_the_scheduler_where_it_was():
    """`step` on host tensors is refused by ops before any kernel: the index, the history flag and the buffer in turn are those
    of before the call, so a retry does not read a history that was never written."""
    import vdx  # noqa: F401
    from vdx._lib import VdxError
    s = _sched()
    s.set_timesteps(10)
    x = torch.zeros(1, 4, 2, 2, 2, dtype=torch.float16)
    for call in (lambda: s.step(x, s._host_timesteps[0], x), lambda: s.step_cfg(torch.cat([x, x]), s._host_timesteps[0], x, 7.5)):
        with pytest.raises(VdxError):
            call()
        assert (s._step_index, s._have_prev, s._cur) == (None, False, 0)
    _adv(s, s._host_timesteps[0], x)
    with pytest.raises(VdxError):
        s.step(x, s._host_timesteps[1], x)
    assert (s._step_index, s._have_prev, s._cur) == (1, True, 1)


def test_the_999_step_schedule_clamps_its_first_sigma_and_refuses_alpha_lookups():
    """n = 999: the stated formula puts the first timestep at 1000, past the training range.  Its sigma is that of timestep 999
    (`interp` clamps); what reads alphas_cumprod[t] says so instead of raising IndexError."""
    import vdx  # noqa: F401
    from vdx.miner import denoise_with_trace
    s = _sched()
    s.set_timesteps(999)
    assert s._host_timesteps[0] == 1000 and float(s.sigmas[0]) == float(s.sigmas[1])
    x = torch.zeros(1, 4, 1, 2, 2, dtype=torch.float16)
    with pytest.raises(ValueError, match="training steps"):
        s.add_noise(x, x, 1000)
    with pytest.raises(ValueError, match="training steps"):
        denoise_with_trace(None, s, x, None, 999)


def test_step_index_is_found_by_value_and_must_continue():
    """The bookkeeping around the kernel, without one: index by value on the first step, first order without history and on
    the last step, ping-pong buffers, an error for a timestep that does not continue the schedule."""
    s = _sched()
    s.set_timesteps(10)
    x = torch.zeros(1, 4, 2, 2, 2, dtype=torch.float16)
    ts = s._host_timesteps
    i, prev, out = _adv(s, ts[4], x)                 # a truncated (video-to-video) schedule starts mid-way
    assert (i, prev) == (4, None)
    i2, prev2, out2 = _adv(s, ts[5], x)
    assert i2 == 5 and prev2 is out and out2 is not out
    with pytest.raises(ValueError):
        _adv(s, ts[9], x)                            # skips ahead
    s.reset()
    for j, t in enumerate(ts):
        i, prev, out = _adv(s, torch.tensor(t), x)
        assert i == j and (prev is None) == (j in (0, 9)) and out is not prev
    with pytest.raises(ValueError):
        _adv(s, ts[0], x)                            # exhausted: reset() first
    s.reset()
    assert _adv(s, ts[0], x)[:2] == (0, None)
    with pytest.raises(ValueError):
        s.set_timesteps(10), _adv(s, 123, x)         # not a timestep of the schedule
    o1 = _sched(solver_order=1)
    o1.set_timesteps(4)
    assert all(_adv(o1, t, x)[1] is None for t in o1._host_timesteps)


def test_vid2vid_timesteps_accepts_the_scheduler():
    import vdx  # noqa: F401
    from vdx.pipeline import vid2vid_timesteps
    s = _sched()
    s.set_timesteps(10)
    assert vid2vid_timesteps(s, 10, 0.6) == s._host_timesteps[4:]


def _ddim_sample(x, n):
    from oracle.ddim_ref import DDIMSchedulerRef
    d = DDIMSchedulerRef()
    d.set_timesteps(n)
    t_first = int(d.timesteps[0])
    for t in d.timesteps:
        x = d.step(R.toy_eps(x, int(t)), t, x).prev_sample
    return x, t_first


def test_convergence_on_the_gaussian_toy_problem():
    """Data ~ N(0, 2^2): eps*(x, t) is linear in x and the probability-flow ODE has a closed-form solution, so the error of a
    sampler is measurable without any model.  fp16 tensors, the schedule of the product.  Measured on the CPU when this was
    written: 2M 10 steps 1.34e-2 < DDIM 50 steps 2.14e-2; 2M 20 steps 4.98e-3 vs 2M 10 steps 1.34e-2; 2M 25 steps 4.39e-3 vs
    DDIM 25 steps 4.13e-2; order 1 at 20 steps 4.87e-2 vs 2M 4.98e-3: every inequality has 1.3x headroom or more."""
    x_T = R.toy_start()
    err = {}
    for n in (10, 20, 25):
        x, _ = R.sample(R.toy_eps, x_T, n)
        err["2m", n] = R.rel_err(x, R.toy_exact(x_T, int(R.timesteps(n)[0])))
    x, _ = R.sample(R.toy_eps, x_T, 20, order=1)
    err["o1", 20] = R.rel_err(x, R.toy_exact(x_T, int(R.timesteps(20)[0])))
    for n in (25, 50):
        x, t_first = _ddim_sample(x_T, n)
        err["ddim", n] = R.rel_err(x, R.toy_exact(x_T, t_first))
    print({k: f"{v:.3e}" for k, v in err.items()})
    assert err["2m", 10] < err["ddim", 50]
    assert err["2m", 20] < 0.5 * err["2m", 10]
    assert err["2m", 25] < 0.25 * err["ddim", 25]
    assert err["o1", 20] > 3 * err["2m", 20]                      # the history is really used


def test_last_step_of_the_restatement_returns_x0():
    x_T = R.toy_start()
    for n in (1, 2, 10):
        x, trace = R.sample(R.toy_eps, x_T, n)
        assert torch.equal(trace[-1][0], trace[-1][1]) and torch.equal(x, trace[-1][1])


def test_diffusers_shim_exports_the_class():
    import vdx  # noqa: F401
    from vdx.compat import diffusers_shim
    from vdx.scheduler import DPMSolverMultistepScheduler
    assert diffusers_shim.DPMSolverMultistepScheduler is DPMSolverMultistepScheduler
    s = diffusers_shim.DPMSolverMultistepScheduler.from_config(diffusers_shim.DDIMScheduler().config)
    assert isinstance(s, DPMSolverMultistepScheduler)


def test_front_end_flag_and_config():
    import vdx  # noqa: F401
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args, make_scheduler
    from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    assert DiffuserConfig().scheduler == "ddim"
    p = build_arg_parser()
    assert config_from_args(p.parse_args([])).scheduler == "ddim"
    assert config_from_args(p.parse_args(["--scheduler", "dpmpp_2m"])).scheduler == "dpmpp_2m"
    with pytest.raises(SystemExit):
        p.parse_args(["--scheduler", "euler"])
    d = DDIMScheduler()
    assert make_scheduler("ddim", d) is d and isinstance(make_scheduler("dpmpp_2m", d), DPMSolverMultistepScheduler)
    with pytest.raises(ValueError):
        make_scheduler("euler", d)


STEP_CFG = ("step_cfg", "step_cfg_windows", "step_cfg_tiles", "step_cfg_loop")


def _fused_calls(s, x):
    """One call of each `step_cfg*` method on the sample `x` at the scheduler's next timestep -> nothing; the arguments beside the
    sample are tokens that only the recording stubs see."""
    return {"step_cfg": lambda t: s.step_cfg("noise2", t, x, 7.5),
            "step_cfg_windows": lambda t: s.step_cfg_windows("windows", "table", "wn", t, x, 7.5),
            "step_cfg_tiles": lambda t: s.step_cfg_tiles("windows", "table", "wn", "tiles", t, x, 7.5),
            "step_cfg_loop": lambda t: s.step_cfg_loop("windows", "table", "wn", t, x, 7.5)}


def test_step_cfg_methods_are_defined_once_and_a_failed_launch_changes_nothing(monkeypatch):
    """The four `step_cfg*` names are ONE function object each on both schedulers (`_SchedulerBase`'s); with `ops` replaced by
    recording stubs nothing launches: each scheduler reaches its own sampler's op with its coefficients, the DPM-Solver++ history
    ping-pongs, and a launch that raises leaves `_step_index`, `_cur` and `_have_prev` where they were."""
    import vdx  # noqa: F401
    from vdx import scheduler as S
    for name in STEP_CFG:
        assert getattr(S.DDIMScheduler, name) is getattr(S.DPMSolverMultistepScheduler, name) is getattr(S._SchedulerBase, name)
        assert name not in vars(S.DDIMScheduler) and name not in vars(S.DPMSolverMultistepScheduler)
    calls, fail = [], []

    class Stubs:
        def __getattr__(self, op):
            def stub(*args, **kw):
                calls.append((op, args, kw))
                if fail:
                    raise RuntimeError("launch failed")
                return ("new", kw["x0_out"]) if op.endswith("_dpm_step") else "new"
            return stub
    monkeypatch.setattr(S, "ops", Stubs())
    x = torch.zeros(1, 2, 3, 1, 4)
    heads = {"step_cfg": ("cfg", ("noise2", x)), "step_cfg_windows": ("cofuse_cfg", (x, "windows", "table", "wn")),
             "step_cfg_tiles": ("cotile_cfg", (x, "windows", "table", "wn", "tiles")),
             "step_cfg_loop": ("coloop_cfg", (x, "windows", "table", "wn"))}
    d = S.DDIMScheduler()
    d.set_timesteps(4)
    for name, call in _fused_calls(d, x).items():
        calls.clear()
        t = d._host_timesteps[1]
        assert call(t) == "new"
        stem, head = heads[name]
        (op, args, kw), = calls
        assert op == f"{stem}_ddim_step" and kw == {} and len(args) == len(head) + 2
        assert all(a is b for a, b in zip(args, head)) and args[-2:] == (7.5, d.coefficients(t))
    for name in STEP_CFG:
        p = S.DPMSolverMultistepScheduler()
        p.set_timesteps(4)
        call = _fused_calls(p, x)[name]
        stem, head = heads[name]
        calls.clear()
        assert call(p._host_timesteps[0]) == "new" and call(p._host_timesteps[1]) == "new"
        (op0, a0, k0), (op1, a1, k1) = calls
        assert op0 == op1 == f"{stem}_dpm_step" and all(a is b for a, b in zip(a1, head))
        assert a0[-2:] == (7.5, p.coefficients(0, False)) and a1[-2:] == (7.5, p.coefficients(1, True))
        assert k0["x0_prev"] is None and k1["x0_prev"] is k0["x0_out"] and k1["x0_out"] is not k0["x0_out"]
        before = (p._step_index, p._cur, p._have_prev)
        assert before == (2, 0, True)
        fail.append(True)
        with pytest.raises(RuntimeError, match="launch failed"):
            call(p._host_timesteps[2])
        fail.clear()
        assert (p._step_index, p._cur, p._have_prev) == before
        assert call(p._host_timesteps[2]) == "new" and p._step_index == 3      # the same step goes through afterwards
