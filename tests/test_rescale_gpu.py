"""Negative prompts and CFG rescale on the GPU (csrc/rescale.hip, vdx/scheduler.py, vdx/pipeline.py) against the torch-CPU
restatement of tests/rescale_ref.py: the statistics pass within the bound of a fixed-order fp64 sum and bit-equal from run to
run; the step kernels bit for bit given their own r, and end to end; the co-fused variants; NaN, infinity and constant samples;
the refusals; the job against a Python loop over its windows, the defaults untouched, `run_job` with a negative prompt, and two
ranks against one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import codenoise_ref as CR
import dpm_ref
import rescale_ref as R
import stats_order_ref as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (C, L, h, w): N = 2; the scalar path with a ragged tail; the 8-byte path; the 16-byte path; several blocks with a partial last
# one; the headline, where the block cap is reached
SHAPES = [(1, 1, 1, 2), (4, 3, 5, 7), (4, 2, 2, 6), (4, 2, 4, 6), (4, 16, 18, 32)]
HEADLINE = (4, 24, 72, 128)
GS, PHI = (2.0, 7.5, 12.0), (0.3, 0.7, 1.0)
DDIM = (0.9493, 0.3143, 0.4206, 0.9073)                            # any four fp32 coefficients: the chain is pinned, not the schedule


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    return ops, VdxError


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = _bits(got) != _bits(want)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ"


_CASES = {}


def _case(shape):
    """Seeded Gaussian u, c, x and an x0 history at `shape`, made once and never written."""
    if shape not in _CASES:
        g = torch.Generator().manual_seed(1000 + sum(shape))
        _CASES[shape] = tuple(torch.randn((k,) + shape, generator=g).half() for k in (2, 1, 1))
    return _CASES[shape]


def _stats16(t):
    return tuple(np.float16(v) for v in t.cpu()[:3].numpy())


def _same_scalars(got, want, what):
    for name, a, b in zip(("sd_c", "sd_g", "r"), got, want):
        assert np.float16(a).view(np.uint16) == np.float16(b).view(np.uint16) or (np.isnan(a) and np.isnan(b)), \
            f"{what}: {name} = {a!r}, the restatement's is {b!r}"


@pytest.mark.parametrize("shape", SHAPES + [HEADLINE], ids=str)
def test_partial_sums(gpu, shape):
    ops, _ = _ops()
    eps2 = _case(shape)[0]
    n = eps2.numel() // 2
    part = ops.cfg_rescale_stats(eps2.to(gpu), 7.5).cpu().clone()
    rows = ops.cfg_rescale_rows(n)
    width = 8 if n % 8 == 0 else 4 if n % 4 == 0 else 1
    assert tuple(part.shape) == (rows, 4) and part.dtype == torch.float64
    assert rows == min(256, -(-(n // width) // 256)) and (rows == 256) == (shape == HEADLINE)
    want, scale = R.sums64(eps2, 7.5)
    for q, name in enumerate(("sum c", "sum c*c", "sum g", "sum g*g")):
        got = float(part[:, q].sum())                              # rows ascending, as the step kernels add them
        err, bound = abs(got - want[q]), n * 2.0 ** -53 * scale[q]
        print(f"{shape} {name}: {got!r} vs {want[q]!r}, |diff| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, name
    again = ops.cfg_rescale_stats(eps2.to(gpu), 7.5).cpu()
    assert torch.equal(again.view(torch.int64), part.view(torch.int64))


WIDTHS = [(2048,), (2052,), (2051,)]                               # n a multiple of 8, of 4 only, and odd: every access width


@pytest.mark.parametrize("shape", SHAPES + [HEADLINE] + WIDTHS, ids=str)
def test_steps_given_the_kernels_own_r(gpu, shape):
    ops, VdxError = _ops()
    eps2, x, prev = _case(shape)
    e, xg, pg = eps2.to(gpu), x.to(gpu), prev.to(gpu)
    gs, phi = 7.5, 0.7
    fac = ops.rescale_factors(phi)
    st = torch.zeros(8, dtype=torch.float16, device=gpu)
    part = ops.cfg_rescale_stats(e, gs)
    got = ops.cfg_rescale_ddim_step(e, xg, gs, fac, DDIM, part, stats_out=st)
    r = _stats16(st)[2]
    _same_bits(got, R.ddim_step(eps2, x, gs, phi, DDIM, r=r), "ddim")
    sig = dpm_ref.sigmas(10)
    for second in (False, True):
        k = dpm_ref.scalars(sig, 4, second)
        coeffs = (k["s0"], k["inv_a0"], k["cx"], -k["k"], -k.get("half_k", 0.0), k.get("inv_r0", 0.0))
        st.zero_()
        new, x0 = ops.cfg_rescale_dpm_step(e, xg, gs, fac, coeffs, part, x0_prev=pg if second else None, stats_out=st)
        assert _stats16(st)[2].view(np.uint16) == r.view(np.uint16)
        want, want0 = R.dpm_step(eps2, x, prev if second else None, gs, phi, k, r=r)
        _same_bits(new, want, f"dpm order {1 + second}")
        _same_bits(x0, want0, f"dpm order {1 + second}: history")
    # in place on the latent, as the plain steps allow
    y = xg.clone()
    assert ops.cfg_rescale_ddim_step(e, y, gs, fac, DDIM, part, out=y) is y and torch.equal(y, got)
    y = xg.clone()
    assert ops.cfg_rescale_dpm_step(e, y, gs, fac, coeffs, part, x0_prev=pg, out=y)[0] is y and torch.equal(y, new)
    # the history may be neither its predecessor nor the latent
    with pytest.raises(VdxError):
        ops.cfg_rescale_dpm_step(e, xg, gs, fac, coeffs, part, x0_prev=pg, x0_out=pg)
    with pytest.raises(VdxError):
        ops.cfg_rescale_dpm_step(e, xg, gs, fac, coeffs, part, x0_prev=pg, x0_out=xg)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_stats_and_step_end_to_end(gpu, shape):
    ops, _ = _ops()
    eps2, x, _ = _case(shape)
    e, xg = eps2.to(gpu), x.to(gpu)
    st = torch.zeros(8, dtype=torch.float16, device=gpu)
    for gs in GS:
        want_s = R.stats(eps2, gs)
        for phi in PHI:
            got = ops.cfg_rescale_ddim_step(e, xg, gs, ops.rescale_factors(phi), DDIM, ops.cfg_rescale_stats(e, gs), stats_out=st)
            _same_scalars(_stats16(st), want_s, f"{shape} gs {gs}")
            _same_bits(got, R.ddim_step(eps2, x, gs, phi, DDIM), f"{shape} gs {gs} phi {phi}")


def test_headline_end_to_end_through_the_schedulers(gpu):
    """(4, 24, 72, 128) once, through `step_cfg` of both schedulers: two steps each, so DPM-Solver++ runs both orders."""
    _ops()
    from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    eps2, x, _ = _case(HEADLINE)
    e, gs, phi = eps2.to(gpu), 7.5, 0.7
    want_s = R.stats(eps2, gs)
    s = DDIMScheduler()
    s.set_timesteps(10, device=gpu)
    t = s._host_timesteps[2]
    _same_bits(s.step_cfg(e, t, x.to(gpu), gs, guidance_rescale=phi), R.ddim_step(eps2, x, gs, phi, s.coefficients(t)), "ddim")
    _same_scalars(_stats16(s.rescale_stats), want_s, "ddim")
    p = DPMSolverMultistepScheduler()
    p.set_timesteps(10, device=gpu)
    sig, lat, ref, prev = dpm_ref.sigmas(10), x.to(gpu), x, None
    for i in (3, 4):
        lat = p.step_cfg(e, p._host_timesteps[i], lat, gs, guidance_rescale=phi)
        ref, prev = R.dpm_step(eps2, ref, prev, gs, phi, dpm_ref.scalars(sig, i, prev is not None))
        _same_bits(lat, ref, f"dpm step {i}")
    _same_scalars(_stats16(p.rescale_stats), want_s, "dpm")


# ---- the co-fused variants ----------------------------------------------------------------------------------------------------
def _windows(C, T, h, w, table, seed):
    """Packed windows [u; c] per row of `table` = [(s, L)], fuse weights normalised as vdx/codenoise.py does."""
    g = torch.Generator().manual_seed(seed)
    wins = [torch.randn(2, C, L, h, w, generator=g).half() for _, L in table]
    raw = np.zeros((len(table), T))
    for k, (s, L) in enumerate(table):
        raw[k, s:s + L] = [min(j + 1, L - j, 3) / 3 for j in range(L)]
    wn = torch.from_numpy((raw / raw.sum(axis=0)).astype(np.float32))
    offs, off = [], 0
    for wv in wins:
        offs.append(off)
        off += wv.numel()
    packed = torch.cat([wv.reshape(-1) for wv in wins])
    return wins, packed, [(o, s, L) for o, (s, L) in zip(offs, table)], wn


@pytest.mark.parametrize("C,T,h,w,table", [(4, 6, 4, 6, [(0, 4), (2, 4)]), (4, 7, 3, 5, [(0, 4), (2, 4), (3, 4)]),
                                           (3, 9, 2, 6, [(0, 5), (3, 4), (5, 4)]), (4, 8, 32, 32, [(0, 6), (4, 4)])], ids=str)
def test_cofused_steps_match_the_restatement_on_the_fused_noise(gpu, C, T, h, w, table):
    ops, _ = _ops()
    wins, packed, rows, wn = _windows(C, T, h, w, table, 7 + T)
    g = torch.Generator().manual_seed(T)
    z, prev = (torch.randn(1, C, T, h, w, generator=g).half() for _ in range(2))
    eps2 = CR.fuse(wins, table, wn, z.shape)
    zg, bg, wg, gs, phi = z.to(gpu), packed.to(gpu), wn.to(gpu), 7.5, 0.7
    fac = ops.rescale_factors(phi)
    part = ops.cofuse_cfg_rescale_stats(zg, bg, rows, wg, gs)
    assert tuple(part.shape) == (min(256, C * T), 4)
    want, scale = R.sums64(eps2, gs)
    for q in range(4):
        assert abs(float(part[:, q].cpu().sum()) - want[q]) <= z.numel() * 2.0 ** -53 * scale[q]
    keep = part.cpu().clone()
    assert torch.equal(ops.cofuse_cfg_rescale_stats(zg, bg, rows, wg, gs).cpu().view(torch.int64), keep.view(torch.int64))
    st = torch.zeros(8, dtype=torch.float16, device=gpu)
    got = ops.cofuse_cfg_rescale_ddim_step(zg, bg, rows, wg, gs, fac, DDIM, part, stats_out=st)
    _same_scalars(_stats16(st), R.stats(eps2, gs), "cofuse ddim")
    _same_bits(got, R.ddim_step(eps2, z, gs, phi, DDIM), "cofuse ddim")
    sig = dpm_ref.sigmas(10)
    for second in (False, True):
        k = dpm_ref.scalars(sig, 4, second)
        coeffs = (k["s0"], k["inv_a0"], k["cx"], -k["k"], -k.get("half_k", 0.0), k.get("inv_r0", 0.0))
        new, x0 = ops.cofuse_cfg_rescale_dpm_step(zg, bg, rows, wg, gs, fac, coeffs, part, x0_prev=prev.to(gpu) if second else None)
        want, want0 = R.dpm_step(eps2, z, prev if second else None, gs, phi, k)
        _same_bits(new, want, f"cofuse dpm order {1 + second}")
        _same_bits(x0, want0, f"cofuse dpm order {1 + second}: history")


def _rescale_terms(eps2, gs):
    """float64 (n, 4): c, c*c, g, g*g per element, in memory order (the products are exact in fp32, so in float64 too)."""
    c = eps2[1].reshape(-1).double().numpy()
    g = dpm_ref.cfg_combine(eps2, gs).reshape(-1).double().numpy()
    return np.stack([c, c * c, g, g * g], axis=1)


@pytest.mark.parametrize("shape", [(2052,), (2, 3, 4, 5)], ids=str)
def test_partial_rows_bit_for_bit_in_the_stated_order(gpu, shape):
    """Every row of `cfg_rescale_stats` against tests/stats_order_ref.py: per lane in stride order, shuffle tree, waves ascending."""
    ops, _ = _ops()
    eps2 = _case(shape)[0]
    n = eps2.numel() // 2
    E, nx = O.width(n), ops.cfg_rescale_rows(n)
    want = O.rows(_rescale_terms(eps2, 7.5), lambda x, k: O.direct_order(n, E, x, k), nx)
    assert O.same_bits(ops.cfg_rescale_stats(eps2.to(gpu), 7.5).cpu().numpy(), want)


def test_cofused_partial_rows_bit_for_bit_in_the_stated_order(gpu):
    """(C, T, HW) = (2, 3, 20), two windows that overlap in frame 1: the clip as C T lines, block b the lines b, b + rows, ..."""
    ops, _ = _ops()
    C, T, h, w, table = 2, 3, 4, 5, [(0, 2), (1, 2)]
    wins, packed, rows, wn = _windows(C, T, h, w, table, 5)
    eps2 = CR.fuse(wins, table, wn, (1, C, T, h, w))
    z = torch.zeros(1, C, T, h, w, dtype=torch.float16, device=gpu)
    got = ops.cofuse_cfg_rescale_stats(z, packed.to(gpu), rows, wn.to(gpu), 7.5).cpu().numpy()
    want = O.rows(_rescale_terms(eps2, 7.5), lambda x, k: O.line_order(C * T, h * w, O.width(h * w), x, k), min(C * T, 256))
    assert O.same_bits(got, want)


def test_rescaled_step_past_the_block_cap_equals_its_halves(gpu):
    """n = 4096 * 256 * 8 + 8 * 300: a lane of the capped grid takes a second trip behind a prologue that uses LDS.  The same entry
    on the two halves of the buffers, given the same statistics buffer, gives the same bits: the buffer holds S1 = 0 and
    S2c = 4 S2g, so sd_c = 2 sd_g in fp16 and r = 2 whatever N is."""
    ops, _ = _ops()
    n = 4096 * 256 * 8 + 8 * 300
    h = n // 2
    assert h % 8 == 0 and ops.cfg_rescale_rows(n) == ops.cfg_rescale_rows(h) == 256
    g = torch.Generator(device=gpu).manual_seed(12)
    noise = torch.randn(2, n, generator=g, device=gpu).half()
    lat = torch.randn(1, n, generator=g, device=gpu).half()
    part = torch.zeros(256, 4, dtype=torch.float64, device=gpu)
    part[0, 1], part[0, 3] = 4.0 * n, 1.0 * n
    st = torch.zeros(8, dtype=torch.float16, device=gpu)
    fac = ops.rescale_factors(0.7)
    got = ops.cfg_rescale_ddim_step(noise, lat, 7.5, fac, DDIM, part, stats_out=st)
    assert float(st[2]) == 2.0
    for sl in (slice(0, h), slice(h, n)):
        st.zero_()
        half = ops.cfg_rescale_ddim_step(noise[:, sl].contiguous(), lat[:, sl].contiguous(), 7.5, fac, DDIM, part, stats_out=st)
        assert float(st[2]) == 2.0 and torch.equal(got[:, sl], half)


@pytest.mark.parametrize("shape", [(4, 3, 5, 7), (4, 2, 4, 6), (4, 16, 18, 32)], ids=str)
def test_one_window_is_the_plain_rescaled_step(gpu, shape):
    ops, _ = _ops()
    eps2, x, _ = _case(shape)
    e, xg, gs = eps2.to(gpu), x.to(gpu), 7.5
    fac = ops.rescale_factors(0.7)
    rows, wn = [(0, 0, shape[1])], torch.ones(1, shape[1], device=gpu)
    plain = ops.cfg_rescale_ddim_step(e, xg, gs, fac, DDIM, ops.cfg_rescale_stats(e, gs))
    fused = ops.cofuse_cfg_rescale_ddim_step(xg, e, rows, wn, gs, fac, DDIM, ops.cofuse_cfg_rescale_stats(xg, e, rows, wn, gs))
    _same_bits(fused, plain, "one window")


# ---- special values and refusals ----------------------------------------------------------------------------------------------
def test_nan_infinity_and_constant_samples(gpu):
    ops, _ = _ops()
    shape = (4, 3, 5, 7)
    eps2, x, _ = _case(shape)
    gs, phi = 7.5, 0.7
    fac = ops.rescale_factors(phi)
    st = torch.zeros(8, dtype=torch.float16, device=gpu)
    guard = torch.full((2, 64), 3.0, dtype=torch.float16, device=gpu)   # a neighbouring sample: nothing outside the sample changes

    def run(e2):
        e = e2.to(gpu)
        out = ops.cfg_rescale_ddim_step(e, x.to(gpu), gs, fac, DDIM, ops.cfg_rescale_stats(e, gs), stats_out=st)
        torch.cuda.synchronize()
        return out, _stats16(st)
    for half, value in ((0, float("nan")), (1, float("nan")), (0, float("inf")), (1, -float("inf"))):
        bad = eps2.clone()
        bad[half, 1, 2, 3, 4] = value
        out, s = run(bad)
        assert np.isnan(s[2]) and np.isnan(R.stats(bad, gs)[2])
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(R.ddim_step(bad, x, gs, phi, DDIM)).all())
    const_c = eps2.clone()
    const_c[1] = 0.5
    out, s = run(const_c)
    _same_scalars(s, R.stats(const_c, gs), "constant c")
    assert s[0] == 0 and s[2] == 0
    _same_bits(out, R.ddim_step(const_c, x, gs, phi, DDIM), "constant c")
    const_g = torch.full((2,) + shape, 0.25).half()
    out, s = run(const_g)
    _same_scalars(s, R.stats(const_g, gs), "constant g")
    assert np.isnan(s[2]) and bool(torch.isnan(out).all())
    assert bool((guard == 3.0).all())


def test_bad_arguments_are_refused_before_a_launch(gpu):
    ops, VdxError = _ops()
    from vdx import _lib
    lib = _lib.load()
    eps2, x, _ = _case((4, 2, 4, 6))
    e, xg = eps2.to(gpu), x.to(gpu)
    n, stream = x.numel(), torch.cuda.current_stream().cuda_stream
    part = ops.cfg_rescale_stats(e, 7.5).clone()
    pe, px, pp = e.data_ptr(), xg.data_ptr(), part.data_ptr()
    out = torch.empty_like(xg)
    assert lib.vdx_cfg_rescale_stats_f16(None, n, 7.5, pp, stream) != 0
    assert lib.vdx_cfg_rescale_stats_f16(pe, n, 7.5, None, stream) != 0
    assert lib.vdx_cfg_rescale_stats_f16(pe, 0, 7.5, pp, stream) != 0
    assert lib.vdx_cfg_rescale_rows(0) == 0 and lib.vdx_cofuse_cfg_rescale_rows(0, 4) == 0
    tail = (0.9, 0.3, 0.4, 0.9, n, stream)
    assert lib.vdx_cfg_rescale_ddim_step_f16(pe, px, out.data_ptr(), pp, None, 7.5, 0.5, 0.5, *tail) == 0
    for phi, phi1 in ((-0.1, 1.0), (1.5, 0.0), (0.5, 1.5), (float("nan"), 0.5), (0.5, float("nan"))):
        assert lib.vdx_cfg_rescale_ddim_step_f16(pe, px, out.data_ptr(), pp, None, 7.5, phi, phi1, *tail) != 0
        assert b"[0, 1]" in lib.vdx_last_error()
    for args in ((None, px, out.data_ptr(), pp), (pe, None, out.data_ptr(), pp), (pe, px, None, pp), (pe, px, out.data_ptr(), None)):
        assert lib.vdx_cfg_rescale_ddim_step_f16(*args, None, 7.5, 0.5, 0.5, *tail) != 0
    assert lib.vdx_cfg_rescale_ddim_step_f16(pe, px, out.data_ptr(), pp, None, 7.5, 0.5, 0.5, 0.9, 0.3, 0.4, 0.9, 0, stream) != 0
    assert lib.vdx_cfg_rescale_dpm_step_f16(pe, px, None, None, out.data_ptr(), pp, None, 7.5, 0.5, 0.5, 1, 1, 1, 1, 0, 0, n, stream) != 0
    for bad in (-0.5, 1.5, float("nan"), float("inf"), "0.5"):
        with pytest.raises(ValueError):
            ops.rescale_factors(bad)
    with pytest.raises(VdxError):
        ops.cfg_rescale_ddim_step(e, xg, 7.5, (0.5, 0.5), DDIM, part[:1, :2].contiguous())   # fewer rows than the sample has
    with pytest.raises(VdxError):
        ops.cfg_rescale_ddim_step(e[:1], xg, 7.5, (0.5, 0.5), DDIM, part)
    with pytest.raises(VdxError):
        ops.cfg_rescale_ddim_step(e, xg, 7.5, (1.5, 0.0), DDIM, part)
    T = x.shape[2]
    many = [(0, 0, T)] * 65
    with pytest.raises(VdxError, match="64"):
        ops.cofuse_cfg_rescale_stats(xg, e, many, torch.ones(65, T, device=gpu), 7.5)
    with pytest.raises(VdxError, match="64"):
        ops.cofuse_cfg_rescale_ddim_step(xg, e, many, torch.ones(65, T, device=gpu), 7.5, (0.5, 0.5), DDIM, part)
    with pytest.raises(VdxError):
        ops.cofuse_cfg_rescale_ddim_step(xg, e, [(0, 0, T)], torch.ones(1, T, device=gpu), 7.5, (2.0, 0.5), DDIM, part)
    torch.cuda.synchronize()


# ---- the job on the tiny golden UNet ------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 8, 32, 32, 3                                     # 8 frames, chunk 6, overlap 2: windows (0, 6), (4, 8)
RANGES = [(0, 6), (4, 8)]
PHI_JOB = 0.7


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    return build(gpu, 0, 1)


def _diffuser(model, sampler="ddim", init=None, mask=None, **kw):
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    kw = {**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx", device="cuda",
                 noise_device="cpu", scheduler=sampler, strength=0.75), **kw}
    return DistributedVideoDiffuser(DiffuserConfig(**kw), m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1],
                                    init_latents=init, latent_mask=mask)


def _loop(d, model, co, mask=None):
    """The job of the diffuser `d` (one rank) written out: the product's UNet on the GPU, and for every scheduler step the
    restatement on the CPU -> the final fp32 latent on the CPU."""
    import inpaint_ref as IR
    from vdx import ops
    from vdx.pipeline import seeded_noise
    unet, emb = model
    emb2 = torch.cat([emb[1:], emb[:1]], dim=0)
    cfg, sched, ts, dev = d.cfg, d.scheduler, list(d.schedule), torch.device("cuda")
    gs, phi, dpm = cfg.guidance_scale, cfg.guidance_rescale, cfg.scheduler == "dpmpp_2m"
    start = d._start if d._start is not None else seeded_noise(d.latent_shape, 1.0, cfg.device, cfg.noise_device)
    cp, sig = d.plan(), dpm_ref.sigmas(cfg.steps)
    first = list(dpm_ref.timesteps(cfg.steps)).index(ts[0]) if dpm else 0
    if mask is not None:
        coef = [IR.add_noise_coefficients(sched, t, d._x0) for t in ts[1:]] + [None]
        x0c, basec, mc = d._x0.cpu(), d._base.cpu(), mask.cpu()

    def step(eps2, x, prev, i, s):
        eps2, x = eps2.cpu(), x.cpu()
        if dpm:
            second = prev is not None and first + i != cfg.steps - 1
            new, x0 = R.dpm_step(eps2, x, prev if second else None, gs, phi, dpm_ref.scalars(sig, first + i, second))
        else:
            new, x0 = R.ddim_step(eps2, x, gs, phi, sched.coefficients(ts[i])), None
        if mask is not None:
            sa, s1 = coef[i] if coef[i] is not None else (0.0, 0.0)
            new = IR.renoise_ref(new, x0c, basec, mc, sa, s1, coef[i] is None, s)
        return new.to(dev), x0

    if co:
        table = [(s, e - s) for s, e in cp.ranges]
        from vdx.codenoise import window_table
        wn = window_table(cp, T).wn
        z, prev = start.clone(), None
        for i, t in enumerate(ts):
            wins = [unet(ops.cfg_input(z[:, :, s:e].contiguous(), d.ctx, cfg.context_weight), t, encoder_hidden_states=emb2).sample.cpu()
                    for s, e in cp.ranges]
            z, prev = step(CR.fuse(wins, table, wn, z.shape), z, prev, i, 0)
        return z.float().cpu()
    chunks = []
    for s, e in cp.for_rank(0):
        lat, prev = start[:, :, s:e].clone(), None
        for i, t in enumerate(ts):
            noise = unet(ops.cfg_input(lat, d.ctx, cfg.context_weight), t, encoder_hidden_states=emb2).sample
            lat, prev = step(noise, lat, prev, i, s)
        chunks.append((s, e, lat))
    out = d.blend(chunks, start, cp.overlap).cpu()
    return IR.paste_ref(out, x0c, mc) if mask is not None else out


@pytest.mark.parametrize("co", [False, True], ids=["windowed", "co_denoise"])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_rescaled_job_is_the_loop(gpu, model, sampler, co):
    d = _diffuser(model, sampler, co_denoise=co, guidance_rescale=PHI_JOB)
    lat, info = d()
    assert info["ranges"] == RANGES and info["steps_run"] == STEPS and info["guidance_rescale"] == PHI_JOB
    _same_bits(lat, _loop(d, model, co), f"{sampler} co={co}")
    plain, info0 = _diffuser(model, sampler, co_denoise=co)()
    assert "guidance_rescale" not in info0 and not torch.equal(plain, lat)
    again, _ = d()
    _same_bits(again, lat, "run to run")


def test_rescaled_masked_job_is_the_loop(gpu, model):
    from dist_inpaint_worker import clean_latent
    from vdx import inpaint, ops
    clean = clean_latent(T, HL, WL, gpu)
    lm = ops.mask_to_latent(torch.from_numpy(inpaint.expand_mask(inpaint.keep_frames_mask("0:3", T), T, HL * 8, WL * 8)).to(gpu))
    d = _diffuser(model, "ddim", init=clean, mask=lm, steps=4, guidance_rescale=PHI_JOB)
    lat, _ = d()
    _same_bits(lat, _loop(d, model, False, mask=lm), "masked")
    keep = ~lm.bool().cpu()[None, None].expand(lat.shape)
    assert torch.equal(_bits(lat)[keep], _bits(clean.float())[keep])


def test_defaults_are_untouched(gpu, model, monkeypatch):
    """guidance_rescale 0.0 and negative_prompt "" are the config that names neither: the same latent and `info` keys, and the
    scheduler's `step_cfg` is called with the four arguments it always was (no keyword, so never the new branch)."""
    from vdx.scheduler import DDIMScheduler
    calls = []
    real = DDIMScheduler.step_cfg

    def counting(self, *a, **kw):
        calls.append((len(a), dict(kw)))
        return real(self, *a, **kw)
    monkeypatch.setattr(DDIMScheduler, "step_cfg", counting)
    named, info1 = _diffuser(model, guidance_rescale=0.0, negative_prompt="")()
    n_named, calls[:] = len(calls), []
    bare, info0 = _diffuser(model)()
    assert len(calls) == n_named == STEPS * len(RANGES) and all(c == (4, {}) for c in calls)
    _same_bits(named, bare, "defaults")
    assert set(info1) == set(info0) and "guidance_rescale" not in info0
    calls[:] = []
    _diffuser(model, guidance_rescale=PHI_JOB)()
    assert all(c == (4, {"guidance_rescale": PHI_JOB}) for c in calls) and len(calls) == STEPS * len(RANGES)


def test_run_job_with_a_negative_prompt(gpu, tmp_path):
    """`run_job` on synthetic weights, 128 x 128, 4 frames: the negative prompt changes the latent's frames, equals a diffuser built
    by hand from the tokenizer and text encoder, and the result and the records carry the new keys; the defaults' do not."""
    import json
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import (DistributedVideoDiffuser, build_arg_parser, config_from_args, main, make_scheduler, run_job)
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    base = ["--model_id", "synthetic:tiny", "--num_frames", "4", "--steps", "2", "--height", "128", "--width", "128", "--chunk_size", "4",
            "--overlap", "2", "--noise_device", "cpu"]
    neg = "watermark, text"

    def job(extra):
        got = {}
        cfg = config_from_args(build_arg_parser().parse_args(base + extra))
        return cfg, run_job(cfg, out_video=None, pipe=pipe, clip_inputs=got), np.stack(got["frames"])
    cfg0, res0, plain = job([])
    _, res0b, named = job(["--negative_prompt", "", "--guidance_rescale", "0"])
    cfg1, res1, negged = job(["--negative_prompt", neg, "--guidance_rescale", "0.7"])
    assert np.array_equal(plain, named) and set(res0) == set(res0b)
    assert "negative_prompt" not in res0 and "guidance_rescale" not in res0
    assert set(res1) == set(res0) | {"negative_prompt", "guidance_rescale"}
    assert res1["negative_prompt"] == neg and res1["guidance_rescale"] == 0.7
    assert not np.array_equal(plain, negged)
    # by hand: uncond = text_encoder(tokenizer(negative prompt))
    tok = pipe.tokenizer
    ids = tok([cfg1.prompt, neg], padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
    with torch.no_grad():
        emb = pipe.text_encoder(ids.to(gpu))[0]
    d = DistributedVideoDiffuser(cfg1, pipe.unet, make_scheduler("ddim", pipe.scheduler), emb[1:].contiguous(), emb[:1].contiguous())
    lat, _ = d()
    assert np.array_equal(np.stack(d.decode_frames(lat, pipe.vae)), negged)
    with pytest.raises(ValueError, match="guidance_scale"):
        job(["--guidance_rescale", "0.7", "--guidance_scale", "1.0"])
    # the records of `main`
    out = tmp_path / "clip.json"
    assert main(base + ["--negative_prompt", neg, "--guidance_rescale", "0.7", "--out_csv", str(tmp_path / "r.csv"), "--out_video", "",
                        "--clip_json", str(out)]) == 0
    rec = json.load(open(out))
    assert rec["negative_prompt"] == neg and rec["guidance_rescale"] == 0.7


def test_two_ranks_end_with_the_bits_of_one(gpu, model, tmp_path):
    """Two processes, one rank each, both on this box's one GPU and talking over gloo, co-denoised with rescale: every rank forms
    the same r from the same gathered buffer.  The child has its own time limit."""
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29761", os.path.join(ROOT, "tests", "dist_rescale_worker.py"), str(out), str(T), "6", "2",
                        str(STEPS), "dpmpp_2m", str(PHI_JOB)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
    got = torch.load(out, weights_only=True)
    lat, _ = _diffuser(model, "dpmpp_2m", co_denoise=True, guidance_rescale=PHI_JOB)()
    assert got["ranges"] == RANGES and got["world_size"] == 2 and got["guidance_rescale"] == PHI_JOB
    _same_bits(got["lat"], lat, "two ranks")
