"""-m gpu: seamless looping, ring windows for co-denoising (csrc/codenoise.hip, its RING flag, vdx/codenoise.py `loop_plan`).  Everything bit for
bit: the kernels against the torch-CPU restatement of tests/coloop_ref.py (every operation a correctly rounded fp32 operation in
a stated order, so equality is derived, not measured), a table without a wrap against the `cofuse` steps, one window against the
plain fused steps on the rolled noise, the wrap itself by rotation equivariance, and the looping job on the tiny golden UNet
against a Python loop written here, from run to run, masked, and end to end through `run_job`."""
import os
import sys

import numpy as np
import pytest
import torch

import codenoise_ref as R
import coloop_ref as L
import dpm_ref
import inpaint_ref

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


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


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


def _dpm(i, second):
    return dpm_ref.scalars(dpm_ref.sigmas(6), i, second)


def _wn(table, T, ov):
    """The product's normalised ring weights for hand-written windows (host logic, tests/test_coloop_host.py)."""
    from vdx.codenoise import loop_table
    from vdx.planner import ChunkPlan
    return loop_table(ChunkPlan(max(n for _, n in table), ov, tuple((s, s + n) for s, n in table), 1), T).wn


def _case(C, T, h, w, table, ov, seed, pads=None):
    """-> z, prev (1,C,T,h,w); the windows' outputs [(2,C,L,h,w)]; the packed buffer (every element outside a window's block is
    NaN: slot tails and the pads in front); rows [(offset, s, L)]; wn.  `table`: [(s, L)], ring windows; `pads[k]`: NaN elements
    in front of window k's block."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(1, C, T, h, w, generator=g).half()
    prev = torch.randn(1, C, T, h, w, generator=g).half()
    wins = [torch.randn(2, C, n, h, w, generator=g).half() for _, n in table]
    slot = 2 * C * max(n for _, n in table) * h * w
    pads = pads or [0] * len(table)
    rows, chunks, off = [], [], 0
    for (s, n), win, pad in zip(table, wins, pads):
        chunks.append(torch.full((pad,), NAN, dtype=torch.float16))
        off += pad
        rows.append((off, s, n))
        chunks.append(win.reshape(-1))
        chunks.append(torch.full((slot - win.numel(),), NAN, dtype=torch.float16))     # pad frames of a short window
        off += slot
    return z, prev, wins, torch.cat(chunks), rows, _wn(table, T, ov)


VARIANTS = [("ddim", 3), ("dpm first order", 0), ("dpm second order", 2), ("dpm last step", 5)]


def _run(ops, variant, i, zg, bg, rows, wg, pg, **kw):
    """One of the step variants on the GPU -> (z', x0 or None)."""
    if variant == "ddim":
        return ops.coloop_cfg_ddim_step(zg, bg, rows, wg, GS, _ddim_coeffs()[i], **kw), None
    second = variant == "dpm second order"
    return ops.coloop_cfg_dpm_step(zg, bg, rows, wg, GS, _coeffs(_dpm(i, second)), x0_prev=pg if second else None, **kw)


def _want(variant, i, z, wins, table, wn, prev):
    if variant == "ddim":
        return L.coloop_ddim(z, wins, table, wn, GS, _ddim_coeffs()[i]), None
    second = variant == "dpm second order"
    return L.coloop_dpm(z, wins, table, wn, GS, _dpm(i, second), prev if second else None)


def _check_case(gpu, z, prev, wins, packed, rows, wn, what):
    ops, _ = _ops()
    table = [(s, n) for _, s, n in rows]
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    for variant, i in VARIANTS:
        got, got_x0 = _run(ops, variant, i, zg, bg, rows, wg, pg)
        want, want_x0 = _want(variant, i, z, wins, table, wn, prev)
        _same_bits(got, want, f"{what} {variant} lat'")
        if want_x0 is not None:
            _same_bits(got_x0, want_x0, f"{what} {variant} x0")
    assert bool(torch.isfinite(got).all())                          # the NaN pads and slot tails were never read


K64 = [(i % 8, 1 + i % 3) for i in range(64)]
CASES = {
    # C = 4; T in {3, 5, 8}; h*w in {1, 15, 12, 64}: E = 1, 1, 4 and 8
    "K = 2, both windows wrap, h*w = 64": dict(C=4, T=8, h=8, w=8, table=[(3, 6), (7, 6)], ov=2),
    "K = 3, frames 0 and 1 in all three, h*w = 15": dict(C=4, T=5, h=3, w=5, table=[(3, 4), (0, 3), (4, 3)], ov=1),
    "T = 3, h*w = 1": dict(C=4, T=3, h=1, w=1, table=[(2, 2), (1, 2)], ov=1),
    "h*w = 12: 8-byte path": dict(C=4, T=5, h=3, w=4, table=[(4, 3), (1, 4)], ov=1),
    "an odd offset forces E = 1": dict(C=4, T=8, h=8, w=8, table=[(3, 6), (7, 6)], ov=2, pads=[0, 1]),
    "an offset a multiple of 4 only": dict(C=4, T=8, h=8, w=8, table=[(3, 6), (7, 6)], ov=2, pads=[0, 4]),
    "K = 64": dict(C=4, T=8, h=3, w=4, table=K64, ov=1),
    "windows of length 1 and T": dict(C=4, T=5, h=3, w=5, table=[(4, 1), (2, 5)], ov=1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_ring_steps_match_the_restatement(gpu, name):
    _check_case(gpu, *_case(seed=3, **CASES[name]), name)


@pytest.mark.parametrize("T,h,w,s", [(3, 1, 1, 2), (5, 3, 5, 3), (8, 8, 8, 5), (5, 3, 4, 1)])
def test_one_window_of_the_whole_ring_is_the_plain_step_on_the_rolled_noise(gpu, T, h, w, s):
    """K = 1, s > 0, L = T: every wn is 1.0f, the fused noise is the window's noise with frame f at clip frame (s + f) mod T."""
    ops, _ = _ops()
    g = torch.Generator().manual_seed(11)
    z, prev = (torch.randn(1, 4, T, h, w, generator=g).half().to(gpu) for _ in range(2))
    eps2 = torch.randn(2, 4, T, h, w, generator=g).half()
    eps2.view(-1)[:3] = torch.tensor([-0.0, 65504.0, 2.0 ** -24], dtype=torch.float16)
    eps2 = eps2.to(gpu)
    rolled = eps2.roll(s, 2).contiguous()
    rows, wn = [(0, s, T)], _wn([(s, T)], T, 2).to(gpu)
    assert bool((wn == 1.0).all())
    for coeffs in _ddim_coeffs()[::4]:
        _same_bits(ops.coloop_cfg_ddim_step(z, eps2, rows, wn, GS, coeffs), ops.cfg_ddim_step(rolled, z, GS, coeffs), "ddim")
    for i, second in ((0, False), (2, True), (5, False)):
        c = _coeffs(_dpm(i, second))
        got, got_x0 = ops.coloop_cfg_dpm_step(z, eps2, rows, wn, GS, c, x0_prev=prev if second else None)
        want, want_x0 = ops.cfg_dpm_step(rolled, z, GS, c, x0_prev=prev if second else None)
        _same_bits(got, want, f"dpm {i} lat'")
        _same_bits(got_x0, want_x0, f"dpm {i} x0")


@pytest.mark.parametrize("h,w,pads", [(8, 8, None), (3, 5, None), (3, 4, None), (8, 8, [0, 1, 2])], ids=["E8", "E1", "E4", "odd offsets"])
def test_a_table_without_a_wrap_is_the_cofuse_step(gpu, h, w, pads):
    from vdx.codenoise import window_table
    from vdx.planner import ChunkPlan
    ops, _ = _ops()
    table = [(0, 4), (2, 4), (4, 4)]
    z, prev, wins, packed, rows, wn = _case(4, 8, h, w, table, 2, seed=7, pads=pads)
    assert torch.equal(wn, window_table(ChunkPlan(4, 2, tuple((s, s + n) for s, n in table), 1), 8).wn)
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    for coeffs in _ddim_coeffs()[::4]:
        _same_bits(ops.coloop_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs), ops.cofuse_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs), "ddim")
    for i, second in ((0, False), (2, True), (5, False)):
        c = _coeffs(_dpm(i, second))
        got, got_x0 = ops.coloop_cfg_dpm_step(zg, bg, rows, wg, GS, c, x0_prev=pg if second else None)
        want, want_x0 = ops.cofuse_cfg_dpm_step(zg, bg, rows, wg, GS, c, x0_prev=pg if second else None)
        _same_bits(got, want, f"dpm {i} lat'")
        _same_bits(got_x0, want_x0, f"dpm {i} x0")


@pytest.mark.parametrize("name", ["K = 2, both windows wrap, h*w = 64", "K = 3, frames 0 and 1 in all three, h*w = 15", "T = 3, h*w = 1",
                                  "h*w = 12: 8-byte path"])
def test_rotation_equivariance(gpu, name):
    """The test of the wrap itself: roll the clip (z, x0_prev, the columns of wn) by r frames and move every window's start r
    frames on, for every r: the outputs are the rolled outputs of the unrotated call.  No frame of a ring is special."""
    ops, _ = _ops()
    z, prev, wins, packed, rows, wn = _case(seed=9, **CASES[name])
    T = z.shape[2]
    bg = packed.to(gpu)
    for variant, i in VARIANTS[:3]:
        base, base_x0 = _run(ops, variant, i, z.to(gpu), bg, rows, wn.to(gpu), prev.to(gpu))
        for r in range(1, T):
            rows_r = [(off, (s + r) % T, n) for off, s, n in rows]
            got, got_x0 = _run(ops, variant, i, z.roll(r, 2).contiguous().to(gpu), bg, rows_r, wn.roll(r, 1).contiguous().to(gpu),
                               prev.roll(r, 2).contiguous().to(gpu))
            _same_bits(got, base.roll(r, 2), f"{name} {variant} r = {r} lat'")
            if base_x0 is not None:
                _same_bits(got_x0, base_x0.roll(r, 2), f"{name} {variant} r = {r} x0")


@pytest.mark.parametrize("name", ["K = 2, both windows wrap, h*w = 64", "K = 3, frames 0 and 1 in all three, h*w = 15"])
def test_nan_and_inf_stay_in_their_element(gpu, name):
    """A NaN in u and an inf in c, each in one element of the LAST window's block at a frame past the wrap: each shows in that
    element (c, (s + f) mod T, p) of the outputs and nowhere else."""
    ops, _ = _ops()
    clean = _case(seed=5, **CASES[name])
    case = _case(seed=5, **CASES[name])
    z, prev, wins, packed, rows, wn = case
    C, T, h, w = z.shape[1:]
    off, s, n = rows[-1]
    f = n - 1
    assert s + f >= T                                               # past the wrap
    t = (s + f) % T
    spots = [(0, 1, f, h - 1, w - 1, NAN), (1, C - 1, f, 0, 0, float("inf"))]
    touched = torch.zeros(z.shape, dtype=torch.bool)
    for half, c, ff, y, x, v in spots:
        wins[-1][half, c, ff, y, x] = v
        packed[off + (((half * C + c) * n + ff) * h + y) * w + x] = v
        touched[0, c, t, y, x] = True
    table = [(ss, nn) for _, ss, nn in rows]
    for variant, i in VARIANTS[:3]:
        outs = []
        for zz, pp, _, bb, rr, ww in (clean, case):
            outs.append(_run(ops, variant, i, zz.to(gpu), bb.to(gpu), rr, ww.to(gpu), pp.to(gpu)))
        want, want_x0 = _want(variant, i, z, wins, table, wn, prev)
        _same_bits(outs[1][0], want, f"{name} {variant} planted")
        for a, b in zip(outs[0], outs[1]):
            if a is None:
                continue
            a, b = a.cpu(), b.cpu()
            assert torch.equal(_bits(a)[~touched], _bits(b)[~touched]) and bool(torch.isfinite(a).all())
            assert not bool(torch.isfinite(b[touched]).any()) and int(touched.sum()) == 2


def test_in_place_and_run_to_run(gpu):
    ops, _ = _ops()
    z, prev, wins, packed, rows, wn = _case(seed=13, **CASES["K = 2, both windows wrap, h*w = 64"])
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    coeffs = _ddim_coeffs()[2]
    want = ops.coloop_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs)
    assert torch.equal(want, ops.coloop_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs))
    x = zg.clone()
    assert ops.coloop_cfg_ddim_step(x, bg, rows, wg, GS, coeffs, out=x) is x and torch.equal(x, want)
    for i, second in ((0, False), (2, True)):
        c = _coeffs(_dpm(i, second))
        want, want_x0 = ops.coloop_cfg_dpm_step(zg, bg, rows, wg, GS, c, x0_prev=pg if second else None)
        x = zg.clone()
        got, got_x0 = ops.coloop_cfg_dpm_step(x, bg, rows, wg, GS, c, x0_prev=pg if second else None, out=x)
        assert got is x and torch.equal(x, want) and torch.equal(got_x0, want_x0)


def test_bad_tables_are_refused_before_a_launch(gpu):
    ops, VdxError = _ops()
    z, prev, wins, packed, rows, wn = _case(seed=17, **CASES["K = 2, both windows wrap, h*w = 64"])
    zg, bg, wg = z.to(gpu), packed.to(gpu), wn.to(gpu)
    coeffs, T = _ddim_coeffs()[0], z.shape[2]
    ops.coloop_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs)
    short = packed.numel() - 2 * 4 * 6 * 64 + 8                       # the last window's block would end 8 elements past the buffer
    bad = {"L > T": [rows[0], (rows[1][0], 7, T + 1)], "s = T": [rows[0], (rows[1][0], T, 6)], "s < 0": [(rows[0][0], -1, 6), rows[1]],
           "L = 0": [rows[0], (rows[1][0], 7, 0)], "frames 5 and 6 in no window": [(rows[0][0], 3, 2), rows[1]],
           "leaves the buffer": [rows[0], (short, 7, 6)], "negative offset": [(-8, 3, 6), rows[1]]}
    for what, table in bad.items():
        with pytest.raises(VdxError):
            ops.coloop_cfg_ddim_step(zg, bg, table, wg, GS, coeffs)
        with pytest.raises(VdxError):
            ops.coloop_cfg_dpm_step(zg, bg, table, wg, GS, _coeffs(_dpm(0, False)))
    with pytest.raises(VdxError, match="no window"):
        ops.coloop_cfg_ddim_step(zg, bg, bad["frames 5 and 6 in no window"], wg, GS, coeffs)
    many = [(0, 0, T)] * 65
    with pytest.raises(VdxError, match="64"):
        ops.coloop_cfg_ddim_step(zg, bg, many, torch.ones(65, T, device=gpu), GS, coeffs)
    lib = ops._lib.load()                                           # and by the library itself, not only by the wrapper
    import ctypes
    off, st, ln = (ctypes.c_int64 * 65)(), (ctypes.c_int32 * 65)(), (ctypes.c_int32 * 65)(*([T] * 65))
    w65 = torch.ones(65, T, device=gpu)
    args = (zg.data_ptr(), bg.data_ptr(), bg.numel(), off, st, ln)
    tail = (w65.data_ptr(), torch.empty_like(zg).data_ptr(), GS, *coeffs, z.shape[1], T, z.shape[3] * z.shape[4], None)
    assert lib.vdx_coloop_cfg_ddim_step_f16(*args, 65, *tail) != 0 and b"64" in lib.vdx_last_error()
    assert lib.vdx_coloop_cfg_ddim_step_f16(*args, 0, *tail) != 0
    assert lib.vdx_coloop_cfg_ddim_step_f16(*args, 64, *tail) == 0
    for s, n in ((0, T + 1), (T, 2), (-1, 2), (0, 0)):
        with pytest.raises(VdxError):
            ops.cfg_input_loop(zg, None, 0.0, s, n)
    torch.cuda.synchronize()


@pytest.mark.parametrize("T,h,w", [(3, 1, 1), (5, 3, 5), (8, 8, 8), (5, 3, 4)])
def test_cfg_input_loop(gpu, T, h, w):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(19)
    z = torch.randn(1, 4, T, h, w, generator=g).half()
    z.view(-1)[:4] = torch.tensor([65504.0, -0.0, 2.0 ** -24, float("inf")], dtype=torch.float16)
    ctx = torch.randn(1, 4, 1, h, w, generator=g).half()
    zg, cg = z.to(gpu), ctx.to(gpu)
    for s in (0, T - 1, T // 2):
        for n in (1, T, 2, T - 1):                                  # 2 and T - 1 wrap for s = T - 1, and T - 1 for s = T // 2
            for c, cw in ((None, 0.0), (cg, 0.35)):
                got = ops.cfg_input_loop(zg, c, cw, s, n)
                assert got.is_contiguous() and tuple(got.shape) == (2, 4, n, h, w) and ops.is_cfg_duplicate(got)
                _same_bits(got, L.cfg_input_loop(z, None if c is None else ctx, cw, s, n), f"s = {s}, L = {n}")
                if s + n <= T:                                      # no wrap: cfg_input_window's bits
                    _same_bits(got, ops.cfg_input_window(zg, c, cw, s, s + n), "against cfg_input_window")
                got.add_(1)
                assert not ops.is_cfg_duplicate(got)                # a write drops the tag, as for cfg_input


# ---- the job on the tiny golden UNet ------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 8, 32, 32, 2
RING = [(0, 6), (4, 10)]                                            # loop_plan(8, 1, 6, 2): the second window holds frames 4..7, 0, 1
CLIPPED = [(0, 6), (4, 8)]
INFO_KEYS = {"chunk_size", "overlap", "ranges", "world_size", "num_frames", "denoise_s", "exchange", "steps_run",
             "emu_gather_delay_s", "net_gather_s", "network_bytes", "payload_bytes", "payload_bytes_actual"}


def _config(**kw):
    from vdx.pipeline import DiffuserConfig
    kw = {**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                 device="cuda", noise_device="cpu", co_denoise=True, loop=True), **kw}
    return DiffuserConfig(**kw)


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    return build(gpu, 0, 1)


def _diffuser(model, sampler="ddim", **kw):
    from vdx.pipeline import DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    extra = {k: kw.pop(k) for k in ("init_latents", "latent_mask") if k in kw}
    return DistributedVideoDiffuser(_config(scheduler=sampler, **kw), m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1], **extra)


def _loop(d, model, start, ctx, sampler, masked=None):
    """The looping round, written out: per step every ring window's UNet output from `ops.cfg_input` on an index_select of the
    clip, the restatement's fuse and chain on the CPU, then (masked: (x0, base, latent mask)) tests/inpaint_ref.py's restatement
    of the mask step on the whole clip.  -> fp16 latent on the CPU."""
    from vdx import ops
    from vdx.codenoise import loop_plan, loop_table
    m, emb = model
    emb2 = torch.cat([emb[1:], emb[:1]], dim=0)
    n_frames = start.shape[2]
    cp = loop_plan(n_frames, 1, d.cfg.chunk_size, d.cfg.overlap)
    assert list(cp.ranges) == RING
    wn, table = loop_table(cp, n_frames).wn, [(s, e - s) for s, e in cp.ranges]
    z, x0_prev = start.cpu(), None
    sched, n = list(d.schedule), d.cfg.steps
    first = n - len(sched)                                          # video-to-video starts mid-schedule
    if masked is not None:
        x0, base, lm = masked
        coef = [inpaint_ref.add_noise_coefficients(d.scheduler, t, x0) for t in sched[1:]] + [None]
        x0c, basec, lmc = x0.cpu(), base.cpu(), lm.cpu()
    for j, t in enumerate(sched):
        zg = z.to(start.device)
        outs = []
        for s, length in table:
            idx = ((s + torch.arange(length)) % n_frames).to(start.device)
            x = ops.cfg_input(zg.index_select(2, idx).contiguous(), ctx, d.cfg.context_weight)
            outs.append(m(x, t, encoder_hidden_states=emb2).sample.cpu())
        if sampler == "ddim":
            z = L.coloop_ddim(z, outs, table, wn, d.cfg.guidance_scale, d.scheduler.coefficients(t))
        else:
            i = first + j
            second = x0_prev is not None and i != n - 1
            z, x0_prev = L.coloop_dpm(z, outs, table, wn, d.cfg.guidance_scale, dpm_ref.scalars(dpm_ref.sigmas(n), i, second),
                                      x0_prev if second else None)
        if masked is not None:
            sa, s1 = coef[j] if coef[j] is not None else (0.0, 0.0)
            z = inpaint_ref.renoise_ref(z, x0c, basec, lmc, sa, s1, coef[j] is None, 0)
    return z


def _base(d):
    from vdx.pipeline import seeded_noise
    return seeded_noise(d.latent_shape, d.scheduler.init_noise_sigma, "cuda", "cpu")


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_looping_job_is_the_loop_and_the_same_on_every_run(model, sampler):
    d = _diffuser(model, sampler)
    lat, info = d()
    assert info["ranges"] == CLIPPED and lat.dtype == torch.float32 and tuple(lat.shape) == d.latent_shape
    want = _loop(d, model, _base(d), d.ctx, sampler)
    assert bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat), _bits(want.float()))
    again, _ = d()
    assert torch.equal(_bits(again), _bits(lat))                    # run to run
    assert set(info) == INFO_KEYS | {"co_denoise", "loop"} and info["loop"] == {"windows": [[0, 6], [4, 6]]}
    rec = info["co_denoise"]
    assert (rec["windows"], rec["steps"], rec["bytes_per_step"]) == (2, STEPS, 0)
    assert info["chunk_size"] == 6 and info["overlap"] == 2
    assert info["payload_bytes"] == STEPS * 2 * 6 * 4 * 2           # both windows have the chunk's length
    assert info["payload_bytes_actual"] == STEPS * 2 * (2 * 4 * 6 * HL * WL * 2)
    plain, info0 = _diffuser(model, sampler, loop=False)()          # the same job without the flag: other windows, no record
    assert "loop" not in info0 and set(info0) == INFO_KEYS | {"co_denoise"} and info0["ranges"] == CLIPPED
    assert not torch.equal(plain, lat)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_masked_looping_job_is_the_loop_with_the_mask_step(gpu, model, sampler):
    from dist_inpaint_worker import clean_latent
    from vdx import inpaint, ops
    clean = clean_latent(T, HL, WL, gpu)
    px = torch.from_numpy(inpaint.expand_mask(inpaint.keep_frames_mask("0:2,7", T), T, HL * 8, WL * 8))   # keep both sides of the seam
    lm = ops.mask_to_latent(px.to(gpu))
    d = _diffuser(model, sampler, init_latents=clean, latent_mask=lm, steps=4, strength=0.75)
    assert len(d.schedule) == 3
    lat, info = d()
    assert info["steps_run"] == 3 and info["ranges"] == CLIPPED
    want = _loop(d, model, d._start, d.ctx, sampler, masked=(clean, d._base, lm))
    assert torch.equal(_bits(lat), _bits(want.float()))
    keep = ~lm.bool().cpu()[None, None].expand(lat.shape)
    assert torch.equal(_bits(lat)[keep], _bits(clean.float())[keep]) and int(keep[0, 0, :, 0, 0].sum()) == 3
    again, _ = d()
    assert torch.equal(_bits(again), _bits(lat))


def test_free_init_rounds_loop_too(model):
    d = _diffuser(model, free_init_iters=2)
    lat, info = d()
    assert len(d.free_init_starts) == 1 and info["co_denoise"]["steps"] == 2 * STEPS and info["loop"] == {"windows": [[0, 6], [4, 6]]}
    start = d.free_init_starts[0]
    want = _loop(d, model, start, start.mean(dim=2, keepdim=True).contiguous(), "ddim")
    assert torch.equal(_bits(lat), _bits(want.float()))


# ---- run_job end to end on synthetic weights ---------------------------------------------------------------------------------
def test_run_job_end_to_end(gpu, tmp_path):
    """128 x 128, 8 frames, chunk 6, overlap 2: the result carries "loop" with the windows and two finite numbers that are the
    host's `metrics.loop_l1` of the decoded frames, the ranges handed to the metrics are clipped to the clip, and with
    `--interpolate 2` the file holds 2 F frames, the last of which is new (between frame F-1 and frame 0)."""
    from vdx import metrics
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import build_arg_parser, config_from_args, run_job
    from vdx.video import read_frames
    F = 8
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    base = ["--model_id", "synthetic:tiny", "--num_frames", str(F), "--steps", "2", "--height", "128", "--width", "128", "--chunk_size", "6",
            "--overlap", "2", "--noise_device", "cpu", "--co_denoise"]

    def job(extra, out_video=None):
        got = {}
        res = run_job(config_from_args(build_arg_parser().parse_args(base + extra)), out_video=out_video, pipe=pipe, clip_inputs=got)
        return res, got
    res0, got0 = job([])
    mp4 = str(tmp_path / "loop.mp4")
    res1, got1 = job(["--loop", "--interpolate", "2"], out_video=mp4)
    assert "loop" not in res0 and set(res1) == set(res0) | {"loop"}
    rec = res1["loop"]
    assert set(rec) == {"windows", "wrap_l1", "mean_l1"} and rec["windows"] == [[0, 6], [4, 6]]
    assert np.isfinite(rec["wrap_l1"]) and np.isfinite(rec["mean_l1"]) and rec["wrap_l1"] >= 0 and rec["mean_l1"] >= 0
    assert (rec["wrap_l1"], rec["mean_l1"]) == metrics.loop_l1(got1["frames"])
    assert [tuple(r) for r in got1["ranges"]] == CLIPPED == [tuple(r) for r in got0["ranges"]]
    assert res1["temp_instab"] is not None and res1["co_denoise"]["windows"] == 2
    frames = np.stack(got1["frames"])
    assert frames.shape == (F, 128, 128, 3) and not np.array_equal(frames, np.stack(got0["frames"]))
    assert res1["frames_written"] == 2 * F and res1["interpolate"] == 2
    written = read_frames(mp4, device=gpu)[0]
    assert written.shape[0] == 2 * F
    res2, _ = job(["--interpolate", "2"], out_video=str(tmp_path / "line.mp4"))
    assert res2["frames_written"] == 2 * F - 1                      # without the flag: as always


def test_interpolate_frames_closes_the_loop(gpu):
    from vdx.interp import interpolate_frames
    g = torch.Generator().manual_seed(41)
    clip = torch.randint(0, 256, (3, 32, 48, 3), generator=g, dtype=torch.uint8).to(gpu)
    line = interpolate_frames(torch.cat([clip, clip[:1]]), 3)
    ring = interpolate_frames(clip, 3, loop=True)
    assert tuple(line.shape) == (10, 32, 48, 3) and tuple(ring.shape) == (9, 32, 48, 3) and ring.is_contiguous()
    assert torch.equal(ring, line[:-1]) and torch.equal(ring[::3], clip) and torch.equal(line[-1], clip[0])
    assert torch.equal(interpolate_frames(clip, 3), line[:7])       # without the flag: the open clip's pairs, untouched
    assert torch.equal(interpolate_frames(clip, 1, loop=True), clip)
