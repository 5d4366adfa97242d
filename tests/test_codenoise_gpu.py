"""-m gpu: temporal co-denoising (csrc/codenoise.hip, vdx/codenoise.py).  The kernels bit for bit against the torch-CPU
restatement of tests/codenoise_ref.py (every operation is a correctly rounded fp32 operation in a stated order, so equality is
derived, not measured), the one-window identities against the plain fused steps, and the co-denoised job on the tiny golden
UNet against a Python loop written here, from run to run, and from one rank to two."""
import os
import subprocess
import sys

import pytest
import torch

import codenoise_ref as R
import dpm_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS = 7.5
NAN = float("nan")


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    return ops, VdxError


def _coeffs(k):
    """tests/dpm_ref.py's scalars -> the kernel's six coefficients (include/vdx.h)."""
    return (k["s0"], k["inv_a0"], k["cx"], -k["k"], -k.get("half_k", 0.0), k.get("inv_r0", 0.0))


def _same_bits(got, want, what):
    """Every fp16 bit equal (signed zeros too); NaNs in the same places (a NaN's payload is not part of the statement)."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype == torch.float16 and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
    g, w = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {got.numel()} values differ"


def _ddim_coeffs(steps=10):
    from oracle.ddim_ref import DDIMSchedulerRef
    ref = DDIMSchedulerRef()
    ref.set_timesteps(steps)
    return [tuple(float(c) for c in ref.coefficients(int(t))) for t in ref.timesteps]


def _table(ranges, T, ov):
    """The product's normalised weights for hand-written ranges (host logic, tests/test_codenoise_host.py)."""
    from vdx.codenoise import window_table
    from vdx.planner import ChunkPlan
    tab = window_table(ChunkPlan(max(e - s for s, e in ranges), ov, tuple(ranges), 1), T)
    assert len(tab.fused) == len(ranges)
    return tab.wn


def _case(C, T, h, w, ranges, ov, seed, pads=None, plant=False):
    """-> z, prev (1,C,T,h,w); the windows' outputs [(2,C,L,h,w)]; the packed buffer (every element outside a window's block is
    NaN: slot tails and the pads in front); rows [(offset, s, L)]; wn.  `pads[k]`: NaN elements in front of window k's block."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(1, C, T, h, w, generator=g).half()
    prev = torch.randn(1, C, T, h, w, generator=g).half()
    wins = [torch.randn(2, C, e - s, h, w, generator=g).half() for s, e in ranges]
    if plant:
        z[0, 0, 0, 0, 0], z[0, C - 1, T - 1, h - 1, w - 1] = 65504.0, -65504.0
        wins[0][0, 0, 0, 0, 0] = NAN                               # NaN in u of the first frame
        wins[-1][1, C - 1, -1, h - 1, w - 1] = float("inf")        # inf in c of the last frame
        wins[0][1, 0, -1, 0, 0] = float("-inf")                    # where windows overlap: -inf from one of them
        wins[0][0, C - 1, 0, h - 1, 0] = 65504.0
        wins[-1][0, 0, -1, 0, w - 1] = -65504.0
        prev[0, 0, T - 1, 0, 0] = NAN
    chunk = max(e - s for s, e in ranges)
    slot = 2 * C * chunk * h * w
    pads = pads or [0] * len(ranges)
    rows, chunks, off = [], [], 0
    for (s, e), win, pad in zip(ranges, wins, pads):
        chunks.append(torch.full((pad,), NAN, dtype=torch.float16))
        off += pad
        rows.append((off, s, e - s))
        chunks.append(win.reshape(-1))
        chunks.append(torch.full((slot - win.numel(),), NAN, dtype=torch.float16))     # pad frames of a short window
        off += slot
    return z, prev, wins, torch.cat(chunks), rows, _table(ranges, T, ov)


def _check_case(gpu, z, prev, wins, packed, rows, wn, what):
    ops, _ = _ops()
    table = [(s, L) for _, s, L in rows]
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    for i, coeffs in enumerate(_ddim_coeffs()[::4]):
        got = ops.cofuse_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs)
        _same_bits(got, R.cofuse_ddim(z, wins, table, wn, GS, coeffs), f"{what} ddim {i}")
    sig = dpm_ref.sigmas(6)
    for i, second in ((0, False), (2, True), (5, False)):          # first order, second order, the last step (sigma 0)
        k = dpm_ref.scalars(sig, i, second)
        got, got_x0 = ops.cofuse_cfg_dpm_step(zg, bg, rows, wg, GS, _coeffs(k), x0_prev=pg if second else None)
        want, want_x0 = R.cofuse_dpm(z, wins, table, wn, GS, k, prev if second else None)
        _same_bits(got_x0, want_x0, f"{what} dpm step {i} x0")
        _same_bits(got, want, f"{what} dpm step {i} lat'")


W4 = [(0, 4), (1, 5), (2, 6), (3, 7)]                              # windows of 4, overlap 3: frame 3 lies in all four
CASES = {
    "4x7x3x5 windows of 4 overlap 3": dict(C=4, T=7, h=3, w=5, ranges=W4, ov=3),                         # h*w = 15: scalar path
    "a window of length 1": dict(C=2, T=5, h=2, w=4, ranges=[(0, 3), (2, 3), (2, 5)], ov=1),             # h*w = 8: 16-byte path
    "K = 1": dict(C=3, T=4, h=2, w=3, ranges=[(0, 4)], ov=2),
    "h*w = 1": dict(C=4, T=7, h=1, w=1, ranges=W4, ov=3),
    "1x4x24x9x16 three windows": dict(C=4, T=24, h=9, w=16, ranges=[(0, 12), (6, 18), (12, 24)], ov=6),
    "h*w = 12: 8-byte path": dict(C=2, T=7, h=3, w=4, ranges=W4, ov=3),
    "offsets a multiple of 4 only": dict(C=2, T=7, h=2, w=4, ranges=W4, ov=3, pads=[0, 4, 8, 4]),        # falls back to 8-byte
    "offsets odd": dict(C=2, T=7, h=2, w=4, ranges=W4, ov=3, pads=[0, 1, 2, 4]),                         # falls back to scalar
    "two tiles per line": dict(C=1, T=3, h=48, w=48, ranges=[(0, 2), (1, 3)], ov=1),                     # 2304 > 256 lanes x 8
    "two tiles per line, scalar": dict(C=1, T=3, h=17, w=17, ranges=[(0, 2), (1, 3)], ov=1),             # 289 > 256 lanes x 1
    "uneven windows, short last": dict(C=4, T=10, h=4, w=4, ranges=[(0, 6), (4, 10), (8, 10)], ov=2),    # the job's plan below
}


@pytest.mark.parametrize("name", list(CASES))
def test_fused_steps_match_the_restatement(gpu, name):
    _check_case(gpu, *_case(seed=3, **CASES[name]), name)


@pytest.mark.parametrize("name", ["4x7x3x5 windows of 4 overlap 3", "a window of length 1", "h*w = 12: 8-byte path"])
def test_nan_inf_and_the_largest_values_stay_in_their_element(gpu, name):
    ops, _ = _ops()
    case = _case(seed=5, plant=True, **CASES[name])
    _check_case(gpu, *case, name + " planted")
    # and only there: every element whose inputs were left alone has the bits of the run without the planted values
    clean = _case(seed=5, **CASES[name])
    touched = torch.zeros(clean[0].shape, dtype=torch.bool)
    for (z0, z1) in ((clean[0], case[0]), (clean[1], case[1])):
        touched |= ~(z0.view(torch.int16) == z1.view(torch.int16))
    for (_, s, L), w0, w1 in zip(case[4], clean[2], case[2]):
        diff = ~(w0.view(torch.int16) == w1.view(torch.int16))
        touched[0, :, s:s + L] |= diff[0] | diff[1]
    k = dpm_ref.scalars(dpm_ref.sigmas(6), 2, True)
    outs = []
    for z, prev, _, packed, rows, wn in (clean, case):
        got, x0 = ops.cofuse_cfg_dpm_step(z.to(gpu), packed.to(gpu), rows, wn.to(gpu), GS, _coeffs(k), x0_prev=prev.to(gpu))
        outs.append((got.cpu().view(torch.int16), x0.cpu().view(torch.int16)))
    assert 0 < int(touched.sum()) <= 8
    for a, b in zip(*outs):
        assert torch.equal(a[~touched], b[~touched])


def test_pad_frames_full_of_nan_do_not_leak(gpu):
    """`_case` fills everything outside the windows' blocks with NaN (the tail of a short window's slot, the gaps); a result
    without a NaN shows that none of it was read.  `wn` is zero there, and 0 * NaN would be NaN."""
    ops, _ = _ops()
    z, prev, wins, packed, rows, wn = _case(seed=7, pads=[8, 0, 16], **CASES["uneven windows, short last"])
    assert int(torch.isnan(packed).sum()) > 0
    got = ops.cofuse_cfg_ddim_step(z.to(gpu), packed.to(gpu), rows, wn.to(gpu), GS, _ddim_coeffs()[3])
    new, x0 = ops.cofuse_cfg_dpm_step(z.to(gpu), packed.to(gpu), rows, wn.to(gpu), GS,
                                      _coeffs(dpm_ref.scalars(dpm_ref.sigmas(6), 2, True)), x0_prev=prev.to(gpu))
    for t in (got, new, x0):
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("shape", [(1, 4, 5, 3, 5), (1, 4, 6, 8, 16), (1, 1, 2, 48, 48)], ids=lambda s: "x".join(map(str, s)))
def test_one_window_has_the_bits_of_the_plain_fused_steps(gpu, shape):
    """wn = 1.0f: the fused noise is the window's noise, and the chain is the plain kernels' own."""
    ops, _ = _ops()
    g = torch.Generator().manual_seed(11)
    z, prev = (torch.randn(shape, generator=g).half().to(gpu) for _ in range(2))
    eps2 = torch.randn((2,) + shape[1:], generator=g).half()
    eps2.view(-1)[:6] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, NAN], dtype=torch.float16)
    eps2 = eps2.to(gpu)
    rows, wn = [(0, 0, shape[2])], torch.ones(1, shape[2], device=gpu)
    for coeffs in _ddim_coeffs()[::3]:
        _same_bits(ops.cofuse_cfg_ddim_step(z, eps2, rows, wn, GS, coeffs), ops.cfg_ddim_step(eps2, z, GS, coeffs), "ddim")
    sig = dpm_ref.sigmas(6)
    for i, second in ((0, False), (2, True), (5, False)):
        c = _coeffs(dpm_ref.scalars(sig, i, second))
        got, got_x0 = ops.cofuse_cfg_dpm_step(z, eps2, rows, wn, GS, c, x0_prev=prev if second else None)
        want, want_x0 = ops.cfg_dpm_step(eps2, z, GS, c, x0_prev=prev if second else None)
        _same_bits(got, want, f"dpm {i} lat'")
        _same_bits(got_x0, want_x0, f"dpm {i} x0")


def test_in_place_and_run_to_run(gpu):
    ops, _ = _ops()
    z, prev, wins, packed, rows, wn = _case(seed=13, **CASES["1x4x24x9x16 three windows"])
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    coeffs = _ddim_coeffs()[2]
    want = ops.cofuse_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs)
    assert torch.equal(want, ops.cofuse_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs))
    x = zg.clone()
    assert ops.cofuse_cfg_ddim_step(x, bg, rows, wg, GS, coeffs, out=x) is x and torch.equal(x, want)
    c = _coeffs(dpm_ref.scalars(dpm_ref.sigmas(6), 2, True))
    want, want_x0 = ops.cofuse_cfg_dpm_step(zg, bg, rows, wg, GS, c, x0_prev=pg)
    x = zg.clone()
    got, got_x0 = ops.cofuse_cfg_dpm_step(x, bg, rows, wg, GS, c, x0_prev=pg, out=x)
    assert got is x and torch.equal(x, want) and torch.equal(got_x0, want_x0)


def test_bad_tables_are_refused_before_a_launch(gpu):
    ops, VdxError = _ops()
    z, prev, wins, packed, rows, wn = _case(seed=17, **CASES["a window of length 1"])
    zg, bg, wg = z.to(gpu), packed.to(gpu), wn.to(gpu)
    coeffs, T = _ddim_coeffs()[0], z.shape[2]
    ops.cofuse_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs)
    bad = {"past T": [rows[0], rows[1], (rows[2][0], 3, 3)], "negative start": [(rows[0][0], -1, 3)] + rows[1:],
           "length 0": [rows[0], (rows[1][0], 2, 0), rows[2]], "leaves the buffer": rows[:2] + [(packed.numel() - 8, 2, 3)],
           "negative offset": [(-8, 0, 3)] + rows[1:], "frame 4 uncovered": [rows[0], rows[1], (rows[2][0], 2, 2)]}
    for what, table in bad.items():
        with pytest.raises(VdxError):
            ops.cofuse_cfg_ddim_step(zg, bg, table, wg, GS, coeffs)
        with pytest.raises(VdxError):
            ops.cofuse_cfg_dpm_step(zg, bg, table, wg, GS, _coeffs(dpm_ref.scalars(dpm_ref.sigmas(6), 0, False)))
    many = [(0, 0, T)] * 65
    with pytest.raises(VdxError, match="64"):
        ops.cofuse_cfg_ddim_step(zg, bg, many, torch.ones(65, T, device=gpu), GS, coeffs)
    lib = ops._lib.load()                                           # and by the library itself, not only by the wrapper
    import ctypes
    off, st, ln = (ctypes.c_int64 * 65)(), (ctypes.c_int32 * 65)(), (ctypes.c_int32 * 65)(*([T] * 65))
    w65 = torch.ones(65, T, device=gpu)
    args = (zg.data_ptr(), bg.data_ptr(), bg.numel(), off, st, ln)
    tail = (w65.data_ptr(), torch.empty_like(zg).data_ptr(), GS, *coeffs, z.shape[1], T, z.shape[3] * z.shape[4], None)
    assert lib.vdx_cofuse_cfg_ddim_step_f16(*args, 65, *tail) != 0 and b"64" in lib.vdx_last_error()
    assert lib.vdx_cofuse_cfg_ddim_step_f16(*args, 0, *tail) != 0
    with pytest.raises(VdxError):
        ops.cofuse_cfg_ddim_step(zg, bg, rows, wg[:, :-1].contiguous(), GS, coeffs)
    with pytest.raises(VdxError):
        ops.cfg_input_window(zg, None, 0.0, 2, 2)
    with pytest.raises(VdxError):
        ops.cfg_input_window(zg, None, 0.0, 3, T + 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape,s,e", [((1, 4, 7, 3, 5), 2, 6), ((1, 4, 7, 3, 5), 0, 7), ((1, 4, 9, 8, 16), 8, 9), ((1, 2, 5, 1, 1), 1, 4),
                                       ((1, 1, 3, 40, 64), 1, 3)])
def test_cfg_input_window_is_slice_plus_cfg_input(gpu, shape, s, e):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(19)
    z = torch.randn(shape, generator=g).half()
    z.view(-1)[:4] = torch.tensor([65504.0, -0.0, 2.0 ** -24, float("inf")], dtype=torch.float16)
    ctx = torch.randn((1, shape[1], 1) + shape[3:], generator=g).half()
    zg, cg = z.to(gpu), ctx.to(gpu)
    for c, cw in ((None, 0.0), (cg, 0.35)):
        got = ops.cfg_input_window(zg, c, cw, s, e)
        want = ops.cfg_input(zg[:, :, s:e].contiguous(), c, cw)
        assert got.is_contiguous() and tuple(got.shape) == (2, shape[1], e - s) + shape[3:]
        assert ops.is_cfg_duplicate(got) and ops.is_cfg_duplicate(want)            # the shared prefix still applies
        _same_bits(got, want, "against slice + cfg_input")
        _same_bits(got, R.cfg_input_window(z, None if c is None else ctx, cw, s, e), "against the restatement")
        got.add_(1)
        assert not ops.is_cfg_duplicate(got)                                        # a write drops the tag, as for cfg_input


# ---- the job on the tiny golden UNet ------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 10, 32, 32, 3                                                     # tests/test_e2e_gpu.py's shapes
RANGES = [(0, 6), (4, 10), (8, 10)]                                                  # plan(10, 1, 6, 2)
INFO_KEYS = {"chunk_size", "overlap", "ranges", "world_size", "num_frames", "denoise_s", "exchange", "steps_run",
             "emu_gather_delay_s", "net_gather_s", "network_bytes", "payload_bytes", "payload_bytes_actual"}


def _config(**kw):
    from vdx.pipeline import DiffuserConfig
    kw = {**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                 device="cuda", noise_device="cpu", co_denoise=True), **kw}
    return DiffuserConfig(**kw)


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    return build(gpu, 0, 1)


def _diffuser(model, sampler="ddim", init_latents=None, **kw):
    from vdx.pipeline import DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    return DistributedVideoDiffuser(_config(scheduler=sampler, **kw), m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1],
                                    init_latents=init_latents)


def _loop(d, model, start, ctx, sampler, ranges=RANGES, ov=2):
    """The co-denoised round, written out: per step every window's UNet output from `ops.cfg_input` on a COPIED slice, the
    restatement's fuse and chain on the CPU.  -> fp16 latent on the CPU."""
    from vdx import ops
    m, emb = model
    emb2 = torch.cat([emb[1:], emb[:1]], dim=0)
    n_frames = start.shape[2]
    wn, table = _table(ranges, n_frames, ov), [(s, e - s) for s, e in ranges]
    z, x0_prev = start.cpu(), None
    sched = d.schedule
    n = d.cfg.steps
    first = n - len(sched)                                                           # video-to-video starts mid-schedule
    if sampler == "dpmpp_2m":
        assert [int(t) for t in dpm_ref.timesteps(n)[first:]] == list(sched)
    for j, t in enumerate(sched):
        zg = z.to(start.device)
        outs = []
        for s, e in ranges:
            x = ops.cfg_input(zg[:, :, s:e].contiguous().clone(), ctx, d.cfg.context_weight)
            outs.append(m(x, t, encoder_hidden_states=emb2).sample.cpu())
        if sampler == "ddim":
            z = R.cofuse_ddim(z, outs, table, wn, d.cfg.guidance_scale, d.scheduler.coefficients(t))
        else:
            i = first + j
            second = x0_prev is not None and i != n - 1
            z, x0_prev = R.cofuse_dpm(z, outs, table, wn, d.cfg.guidance_scale, dpm_ref.scalars(dpm_ref.sigmas(n), i, second),
                                      x0_prev if second else None)
    return z


def _base(d):
    from vdx.pipeline import seeded_noise
    return seeded_noise(d.latent_shape, d.scheduler.init_noise_sigma, "cuda", "cpu")


def test_one_window_job_is_denoise(model):
    d = _diffuser(model, mode="fsdp", num_frames=6)                                  # no chunking: one window, no ctx
    lat, info = d()
    assert info["ranges"] == [(0, 6)] and info["co_denoise"]["windows"] == 1
    want = d.denoise(_base(d))
    assert lat.dtype == torch.float32 and torch.equal(lat, want.float())


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_three_window_job_is_the_loop_and_the_same_on_every_run(model, sampler):
    d = _diffuser(model, sampler)
    lat, info = d()
    assert info["ranges"] == RANGES and lat.dtype == torch.float32 and tuple(lat.shape) == d.latent_shape
    want = _loop(d, model, _base(d), d.ctx, sampler)
    assert torch.equal(lat.cpu(), want.float())
    again, info2 = d()
    assert torch.equal(again, lat)
    # accounting: one rank receives nothing; the payload formulas count every step's exchange
    assert set(info) == INFO_KEYS | {"co_denoise"}
    rec = info["co_denoise"]
    assert (rec["windows"], rec["steps"], rec["bytes_per_step"]) == (3, STEPS, 0) and rec["exchange_s"] == info["net_gather_s"] == 0.0
    assert info["network_bytes"] == 0 and info["steps_run"] == STEPS and info["denoise_s"] > 0
    assert info["payload_bytes"] == STEPS * sum((e - s) * 4 * 2 for s, e in RANGES)
    assert info["payload_bytes_actual"] == STEPS * sum(2 * 4 * (e - s) * HL * WL * 2 for s, e in RANGES)
    # the frames two windows share are one copy: the default job's blend zeroes the clip's first and last frame, this does not
    assert bool((lat[:, :, 0].abs().sum() > 0) & (lat[:, :, -1].abs().sum() > 0))


def test_job_without_the_flag_is_untouched(model):
    d = _diffuser(model, co_denoise=False)
    lat, info = d()
    assert set(info) == INFO_KEYS
    chunks = [(s, e, d.denoise(_base(d)[:, :, s:e].clone())) for s, e in RANGES]
    assert torch.equal(lat, d.blend(chunks, _base(d), 2))


def test_free_init_rounds_are_co_denoised(model):
    d = _diffuser(model, steps=2, free_init_iters=2)
    lat, info = d()
    assert len(d.free_init_starts) == 1 and info["free_init"]["iters"] == 2 and info["co_denoise"]["steps"] == 4
    start = d.free_init_starts[0]
    want = _loop(d, model, start, start.mean(dim=2, keepdim=True).contiguous(), "ddim")
    assert torch.equal(lat.cpu(), want.float())


def test_freeu_and_co_denoise(model):
    m, _ = model
    d = _diffuser(model, steps=2, freeu=(1.2, 1.4, 0.9, 0.2))
    lat, info = d()
    assert info["freeu"] == {"b1": 1.2, "b2": 1.4, "s1": 0.9, "s2": 0.2} and m.freeu is None
    m.enable_freeu(**info["freeu"])
    try:
        want = _loop(d, model, _base(d), d.ctx, "ddim")
    finally:
        m.disable_freeu()
    assert torch.equal(lat.cpu(), want.float())
    plain, _ = _diffuser(model, steps=2)()
    assert not torch.equal(plain, lat)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_init_latents_start_mid_schedule(gpu, model, sampler):
    g = torch.Generator().manual_seed(23)
    init = (torch.randn(1, 4, T, HL, WL, generator=g) * 0.5).half().to(gpu)
    d = _diffuser(model, sampler, init_latents=init, steps=4, strength=0.5)
    assert len(d.schedule) == 2
    lat, info = d()
    assert info["steps_run"] == 2 and info["co_denoise"]["steps"] == 2
    want = _loop(d, model, d._start, d.ctx, sampler)
    assert torch.equal(lat.cpu(), want.float())


def test_two_ranks_end_with_the_bits_of_one(gpu, model, tmp_path):
    """Two processes, one rank each, both on this box's one GPU and talking over gloo (tests/test_dist_gpu.py's arrangement), on a
    plan that is the same for one rank and for two: 8 frames, chunk 6, overlap 2."""
    from vdx.planner import plan
    assert plan(8, 1, 6, 2).ranges == plan(8, 2, 6, 2).ranges == ((0, 6), (4, 8))
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29747",
                        os.path.join(ROOT, "tests", "dist_codenoise_worker.py"), str(out), "8", "6", "2", "2", "dpmpp_2m"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
    got = torch.load(out, weights_only=True)
    d = _diffuser(model, "dpmpp_2m", num_frames=8, steps=2)
    lat, info = d()
    assert torch.equal(got["lat"], lat.cpu())
    gi = got["info"]
    assert [tuple(x) for x in gi["ranges"]] == [(0, 6), (4, 8)] and gi["world_size"] == 2
    per_step = 1 * 1 * (2 * 4 * 6 * HL * WL) * 2                                     # (world-1) x per_rank x slot halves x 2 bytes
    assert gi["co_denoise"]["bytes_per_step"] == per_step and gi["network_bytes"] == 2 * per_step
    assert gi["co_denoise"]["windows"] == 2 and gi["co_denoise"]["steps"] == 2 and gi["co_denoise"]["exchange_s"] > 0
    assert gi["payload_bytes"] == 2 * 6 * 4 * 2                                      # rank 0's window (0, 6), twice
    if got["gathers"] is not None:
        assert got["gathers"] > 0                                                    # the parameters were sharded and gathered
