"""-m gpu: the fused DPM-Solver++ (2M) step (csrc/dpm.hip: `vdx_cfg_dpm_step_f16`, `vdx_dpm_step_f16`) bit for bit against
the torch restatement tests/dpm_ref.py evaluated on the GPU, and the scheduler built on it through every entry point: the
CFG loop, per-chunk reset in `DistributedVideoDiffuser`, the truncated video-to-video schedule, the miner trace and the
`python -m vdx.pipeline --scheduler` front end."""
import csv
import os

import numpy as np
import pytest
import torch

import dpm_ref as R

pytestmark = pytest.mark.gpu

TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
GS = 7.5
BLOCK_CAP = 4096                                   # csrc/dpm.hip: the grid-stride loop's block cap (its neighbours' too)
SIZES = [1, 7, 8, 9, 2047, 2048 * 8 + 3]           # below / at / above one 8-half group, a tail, more than one block
# ±max, ±0, subnormals (smallest, largest), values whose difference / CFG combine overflows fp16, small and ordinary values
SPECIAL_U = [65504., -65504., 0., -0., 2.0 ** -24, -2.0 ** -24, 1023 * 2.0 ** -24, -60000., 60000., 30000., 1e-3, 1., -3., 9000.]
SPECIAL_C = [-65504., 65504., -0., 0., -2.0 ** -24, 2.0 ** -24, 2.0 ** -14, 60000., -60000., 40000., -1e-3, 1., 2.5, -9000.]
SPECIAL_X = [65504., -65504., -0., 0., 2.0 ** -24, 1023 * 2.0 ** -24, -2.0 ** -24, 1., -1., 65504., 2.0 ** -14, -5., 0.5, 100.]
SPECIAL_P = [0., 65504., -65504., -0., 2.0 ** -24, -2.0 ** -24, 1., 60000., -60000., 3., -2.0 ** -14, 7., -0.25, -100.]


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    return ops, VdxError


def _coeffs(k):
    """tests/dpm_ref.py's scalars -> the kernel's six coefficients (include/vdx.h)."""
    return (k["s0"], k["inv_a0"], k["cx"], -k["k"], -k.get("half_k", 0.0), k.get("inv_r0", 0.0))


def _with_specials(t, special):
    """Put the special values at the front (the 16-byte path) and, rotated, at the back (the tail) of a flat fp16 tensor."""
    flat = t.view(-1)
    sp = torch.tensor(special, dtype=torch.float16)
    k = min(flat.numel(), sp.numel())
    flat[:k] = sp[:k]
    if flat.numel() >= 2 * sp.numel():
        flat[-sp.numel():] = sp.roll(3)
    return t


def _inputs(n, seed, gpu, specials=True):
    g = torch.Generator().manual_seed(seed)
    eps2 = torch.randn(2, n, generator=g).half()
    lat = torch.randn(1, n, generator=g).half()
    prev = torch.randn(1, n, generator=g).half()
    if specials:
        _with_specials(eps2[0], SPECIAL_U), _with_specials(eps2[1], SPECIAL_C)
        _with_specials(lat, SPECIAL_X), _with_specials(prev, SPECIAL_P)
    return eps2.to(gpu), lat.to(gpu), prev.to(gpu)


def _same(got, want, what):
    """torch.equal, with NaNs required in the same places (the inf pattern is part of the values)."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype == torch.float16 and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
    assert torch.equal(got[~nan], want[~nan]), f"{what}: {int((got[~nan] != want[~nan]).sum())} of {got.numel()} values differ"


def _check_one(ops, eps2, lat, prev, k, second, what):
    """Both entry points against the restatement for one set of scalars: (lat', x0) each."""
    guided = R.cfg_combine(eps2, GS)
    want, want_x0 = R.step(guided, lat, prev if second else None, k)
    got, got_x0 = ops.cfg_dpm_step(eps2, lat, GS, _coeffs(k), x0_prev=prev if second else None)
    _same(got_x0, want_x0, what + " cfg x0")
    _same(got, want, what + " cfg lat'")
    got, got_x0 = ops.dpm_step(guided, lat, _coeffs(k), x0_prev=prev if second else None)
    _same(got_x0, want_x0, what + " x0")
    _same(got, want, what + " lat'")
    return want, want_x0


@pytest.mark.parametrize("steps", [2, 10, 25])
def test_step_bit_exact_at_every_step_of_the_schedule(gpu, steps):
    """First-order (no history), second-order and last-step forms with the scalars of every step of the schedule."""
    ops, _ = _ops()
    sig = R.sigmas(steps)
    eps2, lat, prev = _inputs(2047, steps, gpu)
    for i in range(steps):
        forms = [False] if i == 0 or i == steps - 1 else [False, True]      # a truncated run starts first-order anywhere
        for second in forms:
            want, x0 = _check_one(ops, eps2, lat, prev, R.scalars(sig, i, second), second, f"steps {steps} i {i} second {second}")
            if i == steps - 1:
                _same(want, x0, "the restatement's last step is x0")


@pytest.mark.parametrize("n", SIZES + [BLOCK_CAP * 256 * 8 + 8 * 5 + 3])
def test_step_bit_exact_sizes(gpu, n):
    """Sizes around the 8-half vector group, a scalar tail, several blocks, and one n just above block cap x 256 x 8 where
    the grid-stride loop takes a second trip (and the tail sits behind it)."""
    ops, _ = _ops()
    sig = R.sigmas(10)
    eps2, lat, prev = _inputs(n, n % 1000, gpu)
    for i, second in ((0, False), (5, True), (9, False)):
        _check_one(ops, eps2, lat, prev, R.scalars(sig, i, second), second, f"n {n} i {i}")


@pytest.mark.parametrize("n", [2048, 2052, 2051])
def test_step_bit_exact_at_every_access_width(gpu, n):
    """n a multiple of 8, of 4 only, and odd (16-, 8- and 2-byte accesses), both orders, both entries; at 2048 also in place."""
    ops, _ = _ops()
    sig = R.sigmas(10)
    eps2, lat, prev = _inputs(n, n, gpu)
    for i, second in ((0, False), (5, True)):
        k = R.scalars(sig, i, second)
        want, want_x0 = _check_one(ops, eps2, lat, prev, k, second, f"n {n} i {i}")
        if n == 2048:
            p = prev if second else None
            x = lat.clone()
            got, got_x0 = ops.cfg_dpm_step(eps2, x, GS, _coeffs(k), x0_prev=p, out=x)
            assert got is x
            _same(got, want, "in place cfg"), _same(got_x0, want_x0, "in place cfg x0")
            x = lat.clone()
            got, got_x0 = ops.dpm_step(R.cfg_combine(eps2, GS), x, _coeffs(k), x0_prev=p, out=x)
            _same(got, want, "in place"), _same(got_x0, want_x0, "in place x0")


def test_last_step_returns_the_bits_of_x0(gpu):
    ops, _ = _ops()
    for steps in (1, 2, 10, 25):
        k = R.scalars(R.sigmas(steps), steps - 1, False)
        assert (k["cx"], k["k"]) == (0.0, -1.0)
        eps2, lat, _ = _inputs(2048 * 8 + 3, steps, gpu, specials=False)
        got, x0 = ops.cfg_dpm_step(eps2, lat, GS, _coeffs(k))
        assert torch.equal(got, x0) and bool(torch.isfinite(got.float()).all())
        got, x0 = ops.dpm_step(eps2[:1].contiguous(), lat, _coeffs(k))
        assert torch.equal(got, x0)


def test_in_place_equals_out_of_place_and_aliasing_is_refused(gpu):
    ops, VdxError = _ops()
    sig = R.sigmas(10)
    eps2, lat, prev = _inputs(2048 * 8 + 3, 77, gpu)
    for i, second in ((0, False), (5, True)):
        c = _coeffs(R.scalars(sig, i, second))
        p = prev if second else None
        want, want_x0 = ops.cfg_dpm_step(eps2, lat, GS, c, x0_prev=p)
        x = lat.clone()
        got, got_x0 = ops.cfg_dpm_step(eps2, x, GS, c, x0_prev=p, out=x)
        assert got is x
        _same(got, want, "in place cfg"), _same(got_x0, want_x0, "in place cfg x0")
        e = eps2[1:].clone()                            # (a view of row 1 would start off a 16-byte boundary: n is odd)
        want, want_x0 = ops.dpm_step(e, lat, c, x0_prev=p)
        x = lat.clone()
        got, got_x0 = ops.dpm_step(e, x, c, x0_prev=p, out=x)
        _same(got, want, "in place"), _same(got_x0, want_x0, "in place x0")
    c = _coeffs(R.scalars(sig, 5, True))
    with pytest.raises(VdxError):
        ops.cfg_dpm_step(eps2, lat, GS, c, x0_prev=prev, x0_out=prev)
    with pytest.raises(VdxError):
        ops.dpm_step(eps2[:1].contiguous(), lat, c, x0_prev=prev, x0_out=prev)
    with pytest.raises(VdxError):                       # the library's own check: the history written over the sample
        ops.dpm_step(eps2[:1].contiguous(), lat, c, x0_prev=prev, x0_out=lat)
    with pytest.raises(VdxError):                       # ... or both results in one buffer
        buf = torch.empty_like(lat)
        ops.cfg_dpm_step(eps2, lat, GS, c, x0_prev=prev, x0_out=buf, out=buf)
    torch.cuda.synchronize()


def test_views_two_bytes_off_a_16_byte_boundary_are_refused(gpu):
    """`ops._p` enforces 16-byte pointers for every kernel: a view that starts 2 bytes off is refused on the host, before any
    launch, and the aligned call right after it still works."""
    ops, VdxError = _ops()
    n = 2048 + 5
    c = _coeffs(R.scalars(R.sigmas(10), 5, True))
    eps2, lat, prev = _inputs(n, 5, gpu)
    off_lat = torch.zeros(n + 8, dtype=torch.float16, device=gpu)[1:1 + n].view(1, n)
    off_eps = torch.zeros(2 * n + 8, dtype=torch.float16, device=gpu)[1:1 + 2 * n].view(2, n)
    assert off_lat.data_ptr() % 16 == 2 and off_eps.data_ptr() % 16 == 2 and off_lat.is_contiguous()
    off_lat.copy_(lat), off_eps.copy_(eps2)
    for kw in (dict(eps2=eps2, lat=off_lat), dict(eps2=off_eps, lat=lat), dict(eps2=off_eps, lat=off_lat)):
        with pytest.raises(VdxError, match="16-byte"):
            ops.cfg_dpm_step(kw["eps2"], kw["lat"], GS, c, x0_prev=prev)
    with pytest.raises(VdxError, match="16-byte"):
        ops.dpm_step(off_eps[:1], off_lat, c, x0_prev=prev)
    # the library's own check, below `ops`: each pointer in turn 2 bytes off is an error return, not a launch
    from vdx import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [torch.zeros(2 * n + 8, dtype=torch.float16, device=gpu) for _ in range(5)]      # eps2, lat, x0_prev, x0_out, lat_out
    for bad in range(5):
        ptrs = [b.data_ptr() + (2 if k == bad else 0) for k, b in enumerate(bufs)]
        assert lib.vdx_cfg_dpm_step_f16(*ptrs, GS, *c, n, stream) != 0, bad
        assert lib.vdx_dpm_step_f16(*ptrs, *c, n, stream) != 0, bad
        with pytest.raises(VdxError, match="16-byte"):
            _lib.check(lib.vdx_dpm_step_f16(*ptrs, *c, n, stream), "vdx_dpm_step_f16")
    assert lib.vdx_dpm_step_f16(*[b.data_ptr() for b in bufs], *c, n, stream) == 0
    got, _ = ops.cfg_dpm_step(eps2, lat, GS, c, x0_prev=prev)
    _same(got, R.step(R.cfg_combine(eps2, GS), lat, prev, R.scalars(R.sigmas(10), 5, True))[0], "aligned call afterwards")


# ---- the scheduler on the kernel -------------------------------------------------------------------------------------------
def _sched(**kw):
    import vdx  # noqa: F401
    from vdx.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**kw)


def _toy_cfg_loop(s, x, timesteps, ac):
    """The CFG loop with the Gaussian toy model as the UNet (both halves the same prediction)."""
    for t in timesteps:
        eps = R.toy_eps(x, int(t), ac)
        x = s.step_cfg(torch.cat([eps, eps]), t, x, GS)
    return x


def test_trajectory_equals_the_restatement_and_converges(gpu):
    ac = R.alphas_cumprod()
    x_T = R.toy_start(gpu)
    model = lambda x, t: R.cfg_combine(torch.cat([R.toy_eps(x, t, ac)] * 2), GS)      # noqa: E731
    err = {}
    s = _sched()
    for n in (10, 20, 25):
        s.set_timesteps(n, device=gpu)
        got = _toy_cfg_loop(s, x_T, s._host_timesteps, ac)
        want, _ = R.sample(model, x_T, n)
        assert torch.equal(got, want), n
        err["2m", n] = R.rel_err(got, R.toy_exact(x_T.cpu(), s._host_timesteps[0]))
        if n == 10:
            s.reset()                                   # the same loop again (device-tensor timesteps): the same bits
            assert torch.equal(_toy_cfg_loop(s, x_T, s.timesteps, ac), got)
            s.reset()                                   # `scheduler.step` on the caller's own combine: the same bits
            x = x_T
            for t in s.timesteps:
                x = s.step(model(x, s._host_timestep(t)), t, x).prev_sample
            assert torch.equal(x, got)
    s1 = _sched(solver_order=1)
    s1.set_timesteps(20, device=gpu)
    got = _toy_cfg_loop(s1, x_T, s1._host_timesteps, ac)
    assert torch.equal(got, R.sample(model, x_T, 20, order=1)[0])
    err["o1", 20] = R.rel_err(got, R.toy_exact(x_T.cpu(), s1._host_timesteps[0]))
    from vdx.scheduler import DDIMScheduler
    d = DDIMScheduler()
    for n in (25, 50):
        d.set_timesteps(n, device=gpu)
        err["ddim", n] = R.rel_err(_toy_cfg_loop(d, x_T, d._host_timesteps, ac), R.toy_exact(x_T.cpu(), d._host_timesteps[0]))
    print({k: f"{v:.3e}" for k, v in err.items()})
    assert err["2m", 10] < err["ddim", 50]
    assert err["2m", 20] < 0.5 * err["2m", 10]
    assert err["2m", 25] < 0.25 * err["ddim", 25]
    assert err["o1", 20] > 3 * err["2m", 20]


def test_vid2vid_truncated_schedule_starts_first_order_mid_way(gpu):
    from vdx.pipeline import vid2vid_timesteps
    ac = R.alphas_cumprod()
    x = R.toy_start(gpu)
    s = _sched()
    s.set_timesteps(10, device=gpu)
    ts = vid2vid_timesteps(s, 10, 0.6)
    assert ts == s._host_timesteps[4:] and len(ts) == 6
    got = _toy_cfg_loop(s, x, ts, ac)
    model = lambda x, t: R.toy_eps(x, t, ac)            # noqa: E731
    want, trace = R.sample(model, x, 10, t_start=4)
    assert torch.equal(got, want)
    # the first step run is the first-order update with sigmas[index_of(t_first)] = sigmas[4]
    first, _ = R.step(model(x, ts[0]), x, None, R.scalars(R.sigmas(10), 4, False))
    assert torch.equal(trace[0][0], first)
    s.reset()
    assert torch.equal(s.step_cfg(torch.cat([model(x, ts[0])] * 2), ts[0], x, GS), first)


@pytest.fixture(scope="module")
def tiny_unet(gpu):
    import vdx  # noqa: F401
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from oracle.unet3d_ref import UNet3DConfig as RefCfg, synthetic_state_dict
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    cfg = UNet3DConfig(block_out_channels=TINY["ch"], cross_attention_dim=TINY["cross"], transformer_in_heads=TINY["in_heads"])
    unet = UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(2, 77, TINY["cross"], generator=g).half().to(gpu)
    return unet, emb


def test_history_is_reset_per_chunk(gpu, tiny_unet):
    """Two chunks on one rank: chunk 2's latent is the one a fresh scheduler gives for chunk 2 alone — chunk 1's x0 history and
    step index do not reach it."""
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, seeded_noise
    unet, emb = tiny_unet
    cfg = DiffuserConfig(num_frames=10, steps=3, chunk_size=6, overlap=2, height=128, width=128, mode="hybrid", device="cuda",
                         noise_device="cpu", scheduler="dpmpp_2m")
    d = DistributedVideoDiffuser(cfg, unet, _sched(), emb[:1], emb[1:])
    ranges = d.plan().for_rank(0)
    assert len(ranges) >= 2
    start = seeded_noise((1, 4, 10, 16, 16), 1.0, "cuda", "cpu")
    mine = [d.denoise(start[:, :, s:e].clone()) for s, e in ranges]
    for k in range(1, len(ranges)):                     # (the later windows may be shorter: the history buffers follow the shape)
        s, e = ranges[k]
        alone = DistributedVideoDiffuser(cfg, unet, _sched(), emb[:1], emb[1:]).denoise(start[:, :, s:e].clone())
        assert torch.equal(mine[k], alone) and bool(torch.isfinite(alone.float()).all()), k
    lat, info = d()                                     # and the whole call runs on it
    assert info["steps_run"] == 3 and tuple(lat.shape) == (1, 4, 10, 16, 16) and bool(torch.isfinite(lat).all())


def test_miner_trace_is_bit_stable(gpu, tiny_unet):
    from vdx.miner import denoise_with_trace, leaf_hash
    unet, emb = tiny_unet
    g = torch.Generator().manual_seed(4)
    z0 = torch.randn(1, 4, 3, 16, 16, generator=g).half().to(gpu)
    s = _sched()
    runs = [denoise_with_trace(unet, s, z0, emb[1:], 3) for _ in range(2)]      # the SAME scheduler twice: the trace resets it
    a, b = runs
    assert len(a["latents"]) == len(a["noise_preds"]) == 3 and a["timesteps"] == [751, 501, 251]
    leaves = [[leaf_hash(t, z, e) for t, z, e in zip(r["timesteps"], r["latents"], r["noise_preds"])] for r in runs]
    assert leaves[0] == leaves[1] and torch.equal(a["z"], b["z"]) and torch.equal(a["latents"][0], z0)
    # the leaves hold the model output, and the chain is the scheduler's: z_{i+1} = step(eps_i, t_i, z_i) with the history
    f = _sched()
    f.set_timesteps(3, device=gpu)
    z = z0
    for i, t in enumerate(a["timesteps"]):
        assert torch.equal(z, a["latents"][i])
        z = f.step(a["noise_preds"][i], t, z).prev_sample
    assert torch.equal(z, a["z"])


def test_front_end_scheduler_flag(gpu, tmp_path):
    """`python -m vdx.pipeline --scheduler dpmpp_2m --steps 4` on the tiny stand-in job finishes and writes its row;
    `--scheduler ddim` gives the frames of a run without the flag."""
    import vdx  # noqa: F401
    from vdx import metrics
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import build_arg_parser, config_from_args, main, run_job
    from vdx.scheduler import DDIMScheduler
    out_csv, mp4 = str(tmp_path / "r.csv"), str(tmp_path / "o.mp4")
    base = ["--model_id", "synthetic:tiny", "--num_frames", "10", "--height", "128", "--width", "256", "--chunk_size", "6",
            "--overlap", "2", "--mode", "hybrid_ctx", "--out_csv", out_csv, "--out_video", mp4, "--noise_device", "cpu"]
    assert main(base + ["--steps", "4", "--scheduler", "dpmpp_2m"]) == 0
    rows = list(csv.DictReader(open(out_csv)))
    assert len(rows) == 1 and list(rows[0].keys()) == metrics.CSV_HEADER and rows[0]["mode"] == "hybrid_ctx"
    assert rows[0]["temp_instab"] != "" and os.path.getsize(mp4) > 1000
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    frames = {}
    for name, extra in (("none", []), ("ddim", ["--scheduler", "ddim"]), ("dpm", ["--scheduler", "dpmpp_2m"])):
        got = {}
        res = run_job(config_from_args(build_arg_parser().parse_args(base + ["--steps", "2"] + extra)), out_video=None, pipe=pipe,
                      clip_inputs=got)
        assert res["scheduler"] == ("dpmpp_2m" if name == "dpm" else "ddim") and res["steps_run"] == 2
        frames[name] = np.stack(got["frames"])
    assert isinstance(pipe.scheduler, DDIMScheduler)                    # the pipeline's own scheduler is left alone
    assert np.array_equal(frames["none"], frames["ddim"])
    assert not np.array_equal(frames["none"], frames["dpm"])


def test_stock_scheduler_swap_runs_on_the_shims(gpu):
    """Zeroscope's recipe line, `pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`, in a script
    written against diffusers, under `python -m vdx.compat.run`."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "vdx.compat.run", os.path.join(root, "tests", "compat_dpm_style.py")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("COMPAT-DPM-OK")]
    assert line and "[801, 601, 401, 201]" in line[0], r.stdout[-2000:]
