"""-m gpu: the stochastic sampler steps (csrc/dpm.hip `vdx_*_eta_step_f16`, `vdx_*sde_dpm_step_f16`; csrc/codenoise.hip
`vdx_cofuse_cfg_ddim_eta_step_f16`, `vdx_cofuse_cfg_sde_dpm_step_f16`; csrc/step_noise.h) bit for bit against the CPU restatement
tests/sde_ref.py, whose noise is tests/noise_ref.py's; then the schedulers and the job built on them."""
import os
import sys

import numpy as np
import pytest
import torch

import dpm_ref as D
import sde_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS = 7.5
C = 4
# (T, h, w): 16-byte accesses, two Philox blocks a lane; 8-byte; element-wise with logical indices off the 4-grid
SHAPES = [(5, 6, 8), (3, 5, 4), (3, 3, 3)]
SEEDS = [0, 0x89ABCDEF01234567]
STREAM = R.stream_of_step(1, 3)
# ±max, ±0, subnormals, values whose combine overflows fp16, NaN and ±inf, small and ordinary values (tests/test_dpm_gpu.py's, plus)
SPECIAL_U = [65504., -65504., 0., -0., 2.0 ** -24, -2.0 ** -24, 1023 * 2.0 ** -24, -60000., 60000., float("nan"), float("inf"), 1., -3.]
SPECIAL_C = [-65504., 65504., -0., 0., -2.0 ** -24, 2.0 ** -24, 2.0 ** -14, 60000., -60000., 1., -float("inf"), float("nan"), 2.5]
SPECIAL_X = [65504., -65504., -0., 0., 2.0 ** -24, 1023 * 2.0 ** -24, -2.0 ** -24, 1., float("inf"), float("nan"), 2.0 ** -14, -5., 0.5]
SPECIAL_P = [0., 65504., -65504., -0., 2.0 ** -24, -2.0 ** -24, float("nan"), 60000., -60000., -float("inf"), -2.0 ** -14, 7., -0.25]


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    return ops, VdxError


def _boxes(T):
    return [(0, T), (1, 2), (T - 1, 1)]


def _specials(t, special):
    sp = torch.tensor(special, dtype=torch.float16)
    flat = t.reshape(-1)
    flat[:sp.numel()] = sp
    flat[-sp.numel():] = sp.roll(3)
    return flat.reshape(t.shape)


def _clip(shape, seed):
    """CPU inputs of the whole clip: eps2 (2,C,T,h,w), lat, prev (1,C,T,h,w), with the specials at both ends."""
    T, h, w = shape
    g = torch.Generator().manual_seed(seed)
    eps2 = torch.randn(2, C, T, h, w, generator=g).half()
    lat, prev = torch.randn(1, C, T, h, w, generator=g).half(), torch.randn(1, C, T, h, w, generator=g).half()
    eps2 = torch.stack([_specials(eps2[0], SPECIAL_U), _specials(eps2[1], SPECIAL_C)])
    return eps2, _specials(lat, SPECIAL_X), _specials(prev, SPECIAL_P)


def _cut(t, s, L):
    return t[:, :, s:s + L].contiguous()


def _same(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype == torch.float16 and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)), \
        f"{what}: {int((got[~nan].view(torch.int16) != want[~nan].view(torch.int16)).sum())} of {got.numel()} values differ"


# ---- the references, computed once per (shape, seed) and shared -------------------------------------------------------------
_REF = {}


def _ddim_cases():
    """(name, t, n, eta): eta 0.3 and 1 at the first, a middle and the last step of a 5-step schedule."""
    ts = R.ddim_timesteps(5)
    return [(f"eta {eta} step {i}", int(ts[i]), 5, eta) for eta in (0.3, 1.0) for i in (0, 2, 4)]


def _reference(shape, seed):
    key = (shape, seed)
    if key not in _REF:
        T, h, w = shape
        eps2, lat, prev = _clip(shape, 7)
        guided = D.cfg_combine(eps2, GS)
        wn = R.clip_noise((1, C, T, h, w), seed, STREAM)
        ref = {"inputs": (eps2, lat, prev), "guided": guided, "w": wn, "ddim": {}, "sde": {}}
        for name, t, n, eta in _ddim_cases():
            k = R.ddim_scalars(t, n, eta)
            ref["ddim"][name] = (k, R.ddim_step(guided, lat, k, wn))
        sig = D.sigmas(5)
        for second in (False, True):
            k = R.sde_scalars(sig, 2, second)
            ref["sde"][second] = (k, R.sde_step(guided, lat, prev if second else None, k, wn))
        _REF[key] = ref
    return _REF[key]


def _ddim_coeffs(k):
    return (k["s1"], k["sa"], k["sp"], k["dir"])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_one_buffer_steps_equal_the_reference_on_every_box(gpu, shape, seed):
    """Every one-buffer op, with and without the CFG combine, on the whole clip and on frame boxes: each equals the reference, and
    so the same frames of the whole-clip step."""
    ops, _ = _ops()
    ref = _reference(shape, seed)
    T = shape[0]
    eps2, lat, prev = ref["inputs"]
    for s, L in _boxes(T):
        e2, g, x, p = (_cut(t, s, L).to(gpu) for t in (eps2, ref["guided"], lat, prev))
        what = f"{shape} seed {seed:#x} box ({s}, {L})"
        for name, (k, want) in ref["ddim"].items():
            noise = (k["std"], seed, STREAM)
            _same(ops.cfg_ddim_eta_step(e2, x, GS, _ddim_coeffs(k), noise, frames=(s, T)), _cut(want, s, L), f"{what} cfg ddim {name}")
            _same(ops.ddim_eta_step(g, x, _ddim_coeffs(k), noise, frames=(s, T)), _cut(want, s, L), f"{what} ddim {name}")
        for second, (k, (want, want_x0)) in ref["sde"].items():
            coeffs, cn = R.sde_coeffs(k)
            kw = dict(frames=(s, T), x0_prev=p if second else None)
            for got, got_x0 in (ops.cfg_sde_dpm_step(e2, x, GS, coeffs, (cn, seed, STREAM), **kw),
                                ops.sde_dpm_step(g, x, coeffs, (cn, seed, STREAM), **kw)):
                _same(got, _cut(want, s, L), f"{what} sde second {second}")
                _same(got_x0, _cut(want_x0, s, L), f"{what} sde x0 second {second}")


def test_the_whole_sample_without_frames_is_the_clip(gpu):
    ops, _ = _ops()
    shape, seed = SHAPES[0], SEEDS[1]
    ref = _reference(shape, seed)
    eps2, lat, _ = ref["inputs"]
    k, want = ref["ddim"]["eta 1.0 step 2"]
    _same(ops.cfg_ddim_eta_step(eps2.to(gpu), lat.to(gpu), GS, _ddim_coeffs(k), (k["std"], seed, STREAM)), want, "frames None")


def test_in_place_equals_out_of_place(gpu):
    ops, _ = _ops()
    for shape in SHAPES:
        ref = _reference(shape, 0)
        eps2, lat, prev = (t.to(gpu) for t in ref["inputs"])
        k, want = ref["ddim"]["eta 0.3 step 2"]
        x = lat.clone()
        assert ops.cfg_ddim_eta_step(eps2, x, GS, _ddim_coeffs(k), (k["std"], 0, STREAM), out=x) is x
        _same(x, want, f"{shape} ddim in place")
        k, (want, want_x0) = ref["sde"][True]
        coeffs, cn = R.sde_coeffs(k)
        x = lat.clone()
        _, x0 = ops.cfg_sde_dpm_step(eps2, x, GS, coeffs, (cn, 0, STREAM), x0_prev=prev, out=x)
        _same(x, want, f"{shape} sde in place")
        _same(x0, want_x0, f"{shape} sde in place x0")


def test_refusals(gpu):
    """The alias rules are the deterministic steps'; a box that leaves the clip and a c_n that is not finite are refused, by the
    wrapper and by the library."""
    import vdx  # noqa: F401
    from vdx import _lib
    ops, VdxError = _ops()
    ref = _reference(SHAPES[0], 0)
    T = SHAPES[0][0]
    eps2, lat, prev = (t.to(gpu) for t in ref["inputs"])
    k, _ = ref["sde"][True]
    coeffs, cn = R.sde_coeffs(k)
    kd = _ddim_coeffs(ref["ddim"]["eta 1.0 step 2"][0])
    with pytest.raises(VdxError):                                       # x0_out is x0_prev
        ops.cfg_sde_dpm_step(eps2, lat, GS, coeffs, (cn, 0, STREAM), x0_prev=prev, x0_out=prev)
    with pytest.raises(VdxError):                                       # lat_out overlaps an input
        ops.cfg_ddim_eta_step(eps2, lat, GS, kd, (0.5, 0, STREAM), out=eps2[:1])
    with pytest.raises(VdxError):                                       # x0_out overlaps the latent
        ops.cfg_sde_dpm_step(eps2, lat, GS, coeffs, (cn, 0, STREAM), x0_out=lat)
    box = _cut(lat, 0, 2)
    with pytest.raises(VdxError):                                       # frames [4, 6) of 5
        ops.cfg_ddim_eta_step(_cut(eps2, 0, 2), box, GS, kd, (0.5, 0, STREAM), frames=(T - 1, T))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(VdxError):
            ops.cfg_ddim_eta_step(eps2, lat, GS, kd, (bad, 0, STREAM))
    with pytest.raises(ValueError):
        ops.cfg_ddim_eta_step(eps2, lat, GS, kd, (0.5, 2 ** 64, STREAM))
    # the library's own checks, behind the wrapper's
    lib, out = _lib.load(), torch.empty_like(box)
    _, _, L, h, w = box.shape
    e2 = _cut(eps2, 0, 2)
    args = lambda c_n, s: (e2.data_ptr(), box.data_ptr(), out.data_ptr(), GS, *kd, c_n, 0, STREAM, C, T, h * w, s, L, None)   # noqa: E731
    assert lib.vdx_cfg_ddim_eta_step_f16(*args(0.5, T - 1)) != 0 and b"leave the clip" in lib.vdx_last_error()
    assert lib.vdx_cfg_ddim_eta_step_f16(*args(float("inf"), 0)) != 0 and b"finite" in lib.vdx_last_error()
    assert lib.vdx_cfg_ddim_eta_step_f16(*args(0.5, 0)) == 0
    torch.cuda.synchronize()


def test_cofuse_steps_equal_the_one_buffer_steps_on_the_fused_noise(gpu):
    """Two windows (0, 4), (2, 6) of T = 6: the co-fused stochastic steps have the bits of the one-buffer steps on the noise the
    deterministic fuse gives, and of the reference."""
    ops, _ = _ops()
    T, h, w, seed = 6, 5, 4, SEEDS[1]
    g = torch.Generator().manual_seed(11)
    z, prev = torch.randn(1, C, T, h, w, generator=g).half(), torch.randn(1, C, T, h, w, generator=g).half()
    wins = [torch.randn(2, C, 4, h, w, generator=g).half() for _ in range(2)]
    packed = torch.cat([x.reshape(-1) for x in wins]).to(gpu)
    rows = [(0, 0, 4), (wins[0].numel(), 2, 4)]
    wn = torch.zeros(2, T)
    wn[0, :2], wn[1, 4:] = 1.0, 1.0
    wn[0, 2:4], wn[1, 2:4] = torch.tensor([0.75, 0.25]), torch.tensor([0.25, 0.75])
    U = torch.zeros(2, C, T, h, w)
    for t in range(T):                                                  # the stated fuse: products and sums in fp32, k ascending
        terms = [(wn[k, t] * wins[k][:, :, t - s].float()) for k, (_, s, L) in enumerate(rows) if s <= t < s + L]
        acc = terms[0]
        for x in terms[1:]:
            acc = acc + x
        U[:, :, t] = acc
    fused = U.half()
    zg, pg, wng, fg = z.to(gpu), prev.to(gpu), wn.to(gpu), fused.to(gpu)
    noise_w = R.clip_noise((1, C, T, h, w), seed, STREAM)
    guided = D.cfg_combine(fused, GS)
    k = R.ddim_scalars(int(R.ddim_timesteps(5)[2]), 5, 1.0)
    got = ops.cofuse_cfg_ddim_eta_step(zg, packed, rows, wng, GS, _ddim_coeffs(k), (k["std"], seed, STREAM))
    _same(got, ops.cfg_ddim_eta_step(fg, zg, GS, _ddim_coeffs(k), (k["std"], seed, STREAM)), "cofuse ddim vs one buffer")
    _same(got, R.ddim_step(guided, z, k, noise_w), "cofuse ddim vs reference")
    for second in (False, True):
        ks = R.sde_scalars(D.sigmas(5), 2, second)
        coeffs, cn = R.sde_coeffs(ks)
        kw = dict(x0_prev=pg if second else None)
        got, got_x0 = ops.cofuse_cfg_sde_dpm_step(zg, packed, rows, wng, GS, coeffs, (cn, seed, STREAM), **kw)
        one, one_x0 = ops.cfg_sde_dpm_step(fg, zg, GS, coeffs, (cn, seed, STREAM), **kw)
        want, want_x0 = R.sde_step(guided, z, prev if second else None, ks, noise_w)
        _same(got, one, f"cofuse sde {second} vs one buffer"), _same(got_x0, one_x0, f"cofuse sde x0 {second} vs one buffer")
        _same(got, want, f"cofuse sde {second} vs reference"), _same(got_x0, want_x0, f"cofuse sde x0 {second} vs reference")
    zi = zg.clone()
    ops.cofuse_cfg_ddim_eta_step(zi, packed, rows, wng, GS, _ddim_coeffs(k), (k["std"], seed, STREAM), out=zi)
    _same(zi, R.ddim_step(guided, z, k, noise_w), "cofuse ddim in place")


# ---- the schedulers ---------------------------------------------------------------------------------------------------------
def _toy_model(ac):
    return lambda x, t: torch.cat([D.toy_eps(x, t, ac)] * 2)


def _toy_cfg_loop(s, x, timesteps, ac, **kw):
    for t in timesteps:
        eps = D.toy_eps(x, int(t), ac)
        x = s.step_cfg(torch.cat([eps, eps]), t, x, GS, **kw)
    return x


def test_ddim_eta_trajectory_equals_the_restatement(gpu):
    import vdx  # noqa: F401
    from vdx.scheduler import DDIMScheduler
    ac, x_T, seed = D.alphas_cumprod(), D.toy_start(), 5
    s = DDIMScheduler(eta=1.0)
    s.set_timesteps(5, device=gpu)
    with pytest.raises(ValueError):                                     # no seed set
        s.step_cfg(torch.cat([x_T, x_T]).to(gpu), s._host_timesteps[0], x_T.to(gpu), GS)
    s.seed_noise(seed)
    got = _toy_cfg_loop(s, x_T.to(gpu), s._host_timesteps, ac).cpu()
    want = R.ddim_sample(_toy_model(ac), x_T, 5, 1.0, GS, seed)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(_toy_cfg_loop(s, x_T.to(gpu), s.timesteps, ac).cpu().view(torch.int16), got.view(torch.int16))   # the same seed repeats
    s.seed_noise(seed + 1)
    other = _toy_cfg_loop(s, x_T.to(gpu), s._host_timesteps, ac).cpu()
    assert not torch.equal(other, got)                                  # two seeds differ
    s.seed_noise(seed, 1)
    rnd = _toy_cfg_loop(s, x_T.to(gpu), s._host_timesteps, ac).cpu()
    assert not torch.equal(rnd, got)                                    # two rounds differ
    assert torch.equal(rnd.view(torch.int16), R.ddim_sample(_toy_model(ac), x_T, 5, 1.0, GS, seed, rnd=1).view(torch.int16))
    # a video-to-video start mid-schedule draws the stream of its timestep's index in the full schedule, not 0
    s.seed_noise(seed)
    mid = _toy_cfg_loop(s, x_T.to(gpu), s._host_timesteps[2:], ac).cpu()
    assert torch.equal(mid.view(torch.int16), R.ddim_sample(_toy_model(ac), x_T, 5, 1.0, GS, seed, t_start=2).view(torch.int16))
    # `step` on the caller's own combine, eta as its keyword; eta 0 launches the deterministic op
    s0 = DDIMScheduler()
    s0.set_timesteps(5, device=gpu)
    s0.seed_noise(seed)
    x, t = x_T.to(gpu), s0._host_timesteps[0]
    e = D.cfg_combine(_toy_model(ac)(x_T, t), GS).to(gpu)
    k = R.ddim_scalars(t, 5, 0.5)
    want = R.ddim_step(e.cpu(), x_T, k, R.clip_noise(tuple(x_T.shape), seed, R.stream_of_step(0, 0)))
    assert torch.equal(s0.step(e, t, x, eta=0.5).prev_sample.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(s0.step(e, t, x).prev_sample.cpu(), R.ddim_step(e.cpu(), x_T, R.ddim_scalars(t, 5, 0.0)))
    for kw in (dict(generator=torch.Generator()), dict(variance_noise=x)):
        with pytest.raises(NotImplementedError, match="seeded generator"):
            s0.step(e, t, x, eta=0.5, **kw)


def test_sde_dpm_trajectory_equals_the_restatement(gpu):
    import vdx  # noqa: F401
    from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, SDEDPMSolverMultistepScheduler
    ac, x_T, seed = D.alphas_cumprod(), D.toy_start(), 9
    s = DPMSolverMultistepScheduler.from_config(DDIMScheduler().config, algorithm_type="sde-dpmsolver++")
    assert type(s) is SDEDPMSolverMultistepScheduler and s.stochastic and s.config.algorithm_type == "sde-dpmsolver++"
    s.set_timesteps(5, device=gpu)
    with pytest.raises(ValueError):
        s.step_cfg(torch.cat([x_T, x_T]).to(gpu), s._host_timesteps[0], x_T.to(gpu), GS)
    s.seed_noise(seed)
    got = _toy_cfg_loop(s, x_T.to(gpu), s._host_timesteps, ac).cpu()
    want, want_x0 = R.sde_sample(_toy_model(ac), x_T, 5, GS, seed)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    last_x0 = s._x0[1][1 - s._cur].cpu()                               # the last step's x0: x' has its bits
    assert torch.equal(got.view(torch.int16), last_x0.view(torch.int16)) and torch.equal(last_x0.view(torch.int16), want_x0.view(torch.int16))
    s.reset()
    assert torch.equal(_toy_cfg_loop(s, x_T.to(gpu), s.timesteps, ac).cpu().view(torch.int16), got.view(torch.int16))
    s.reset(), s.seed_noise(seed + 1)
    assert not torch.equal(_toy_cfg_loop(s, x_T.to(gpu), s._host_timesteps, ac).cpu(), got)
    s.reset(), s.seed_noise(seed, 2)
    rnd = _toy_cfg_loop(s, x_T.to(gpu), s._host_timesteps, ac).cpu()
    assert not torch.equal(rnd, got)
    assert torch.equal(rnd.view(torch.int16), R.sde_sample(_toy_model(ac), x_T, 5, GS, seed, rnd=2)[0].view(torch.int16))
    s.reset(), s.seed_noise(seed)
    mid = _toy_cfg_loop(s, x_T.to(gpu), s._host_timesteps[1:], ac).cpu()
    assert torch.equal(mid.view(torch.int16), R.sde_sample(_toy_model(ac), x_T, 5, GS, seed, t_start=1)[0].view(torch.int16))
    # a frame box through `step_cfg(frames=)`: the clip's step at those frames (one first-order step)
    s.reset()
    t = s._host_timesteps[0]
    eps = D.toy_eps(x_T, t, ac)
    whole = s.step_cfg(torch.cat([eps, eps]).to(gpu), t, x_T.to(gpu), GS).cpu()
    s.reset()
    part = s.step_cfg(torch.cat([eps, eps])[:, :, 1:3].contiguous().to(gpu), t, x_T[:, :, 1:3].contiguous().to(gpu), GS, frames=(1, 3)).cpu()
    assert torch.equal(part.view(torch.int16), whole[:, :, 1:3].contiguous().view(torch.int16))
    s.reset()
    with pytest.raises(ValueError, match="no noise form"):
        s.step_cfg(torch.cat([eps, eps]).to(gpu), t, x_T.to(gpu), GS, guidance_rescale=0.5)


# ---- the job ----------------------------------------------------------------------------------------------------------------
def _job(gpu, m, emb, **kw):
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    cfg = DiffuserConfig(num_frames=8, steps=2, chunk_size=6, overlap=2, height=256, width=256, mode="hybrid_ctx", device="cuda",
                         noise="philox", **kw)
    lat, info = DistributedVideoDiffuser(cfg, m, make_scheduler(cfg.scheduler, DDIMScheduler()), emb[1:], emb[:1])()
    return lat.cpu(), info


def test_job_repeats_under_a_seed_and_differs_from_eta_zero(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    m, emb = build(gpu, 0, 1)
    a, info = _job(gpu, m, emb, seed=3, eta=1.0)
    b, _ = _job(gpu, m, emb, seed=3, eta=1.0)
    off, info0 = _job(gpu, m, emb, seed=3)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, off) and bool(torch.isfinite(a).all())
    assert info["sampler_noise"] == {"eta": 1.0, "algorithm": "ddim"} and "sampler_noise" not in info0
    co, cinfo = _job(gpu, m, emb, seed=3, eta=1.0, co_denoise=True)
    co0, _ = _job(gpu, m, emb, seed=3, co_denoise=True)
    assert bool(torch.isfinite(co).all()) and not torch.equal(co, co0) and cinfo["sampler_noise"]["eta"] == 1.0
    sde, sinfo = _job(gpu, m, emb, seed=3, scheduler="dpmpp_2m_sde")
    det, _ = _job(gpu, m, emb, seed=3, scheduler="dpmpp_2m")
    assert bool(torch.isfinite(sde).all()) and not torch.equal(sde, det)
    assert sinfo["sampler_noise"] == {"eta": 1.0, "algorithm": "sde-dpmsolver++"}


def test_front_end_flags_write_the_record(gpu, tmp_path):
    """`--eta` and `--scheduler dpmpp_2m_sde` through the front end: the job's result and the JSON records' source hold the entry."""
    import json
    import vdx  # noqa: F401
    from vdx.pipeline import main
    base = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--height", "128", "--width", "256", "--chunk_size", "6", "--overlap", "2",
            "--mode", "hybrid_ctx", "--steps", "2", "--out_csv", str(tmp_path / "r.csv"), "--out_video", str(tmp_path / "o.mp4"), "--seed", "4"]
    for name, extra, want in (("eta", ["--eta", "0.5"], {"eta": 0.5, "algorithm": "ddim"}),
                              ("sde", ["--scheduler", "dpmpp_2m_sde"], {"eta": 1.0, "algorithm": "sde-dpmsolver++"})):
        rec = tmp_path / f"{name}.json"
        assert main(base + extra + ["--clip_json", str(rec)]) == 0
        got = json.loads(rec.read_text())
        assert got["sampler_noise"] == want and got["noise"]["seed"] == 4
