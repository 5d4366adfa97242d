"""-m gpu: strided context windows for co-denoising (csrc/codenoise.hip, its `costride_tab`; vdx/codenoise.py `stride_plan`).
Everything bit for bit: the kernels against the torch-CPU restatement of tests/costride_ref.py (every operation a correctly
rounded fp32 operation in a stated order, so equality is derived, not measured), a table of strides 1 against the `cofuse` steps,
the stride itself by permuting the clip to evens-then-odds, and the strided job on the tiny golden UNet against a Python loop
written here, from run to run, masked, with a FreeInit round, and end to end through `run_job`."""
import os
import sys

import numpy as np
import pytest
import torch

import codenoise_ref as R
import costride_ref as S
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
    """The product's normalised weights for hand-written strided windows (host logic, tests/test_costride_host.py)."""
    from vdx.codenoise import StridePlan, stride_table
    from vdx.planner import ChunkPlan
    chunk = max(n for _, n, _ in table)
    sp = StridePlan(chunk, ov, tuple(table), 1, len({d for _, _, d in table}), ChunkPlan(chunk, ov, ((0, T),), 1))
    return stride_table(sp, T).wn


def _case(C, T, h, w, table, ov, seed, pads=None):
    """-> z, prev (1,C,T,h,w); the windows' outputs [(2,C,L,h,w)]; the packed buffer (every element outside a window's block is
    NaN: slot tails and the pads in front); rows [(offset, s, L, d)]; wn.  `table`: [(s, L, d)]; `pads[k]`: NaN elements in front
    of window k's block."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(1, C, T, h, w, generator=g).half()
    prev = torch.randn(1, C, T, h, w, generator=g).half()
    wins = [torch.randn(2, C, n, h, w, generator=g).half() for _, n, _ in table]
    slot = 2 * C * max(n for _, n, _ in table) * h * w
    pads = pads or [0] * len(table)
    rows, chunks, off = [], [], 0
    for (s, n, d), win, pad in zip(table, wins, pads):
        chunks.append(torch.full((pad,), NAN, dtype=torch.float16))
        off += pad
        rows.append((off, s, n, d))
        chunks.append(win.reshape(-1))
        chunks.append(torch.full((slot - win.numel(),), NAN, dtype=torch.float16))     # pad frames of a short window
        off += slot
    return z, prev, wins, torch.cat(chunks), rows, _wn(table, T, ov)


VARIANTS = [("ddim", 3), ("dpm first order", 0), ("dpm second order", 2), ("dpm last step", 5)]


def _run(ops, variant, i, zg, bg, rows, wg, pg, strided=True, **kw):
    """One of the step variants on the GPU -> (z', x0 or None); `strided` False: the flat `cofuse` step on rows (off, s, L)."""
    ddim, dpm = (ops.costride_cfg_ddim_step, ops.costride_cfg_dpm_step) if strided else (ops.cofuse_cfg_ddim_step, ops.cofuse_cfg_dpm_step)
    if variant == "ddim":
        return ddim(zg, bg, rows, wg, GS, _ddim_coeffs()[i], **kw), None
    second = variant == "dpm second order"
    return dpm(zg, bg, rows, wg, GS, _coeffs(_dpm(i, second)), x0_prev=pg if second else None, **kw)


def _want(variant, i, z, wins, table, wn, prev):
    if variant == "ddim":
        return S.costride_ddim(z, wins, table, wn, GS, _ddim_coeffs()[i]), None
    second = variant == "dpm second order"
    return S.costride_dpm(z, wins, table, wn, GS, _dpm(i, second), prev if second else None)


def _check_case(gpu, z, prev, wins, packed, rows, wn, what):
    ops, _ = _ops()
    table = [r[1:] for r in rows]
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    for variant, i in VARIANTS:
        got, got_x0 = _run(ops, variant, i, zg, bg, rows, wg, pg)
        want, want_x0 = _want(variant, i, z, wins, table, wn, prev)
        _same_bits(got, want, f"{what} {variant} lat'")
        if want_x0 is not None:
            _same_bits(got_x0, want_x0, f"{what} {variant} x0")
    assert bool(torch.isfinite(got).all())                          # the NaN pads and slot tails were never read


TWO_LEVELS = [(0, 6, 1), (4, 4, 1), (0, 4, 2), (1, 4, 2)]           # stride_plan(8, 1, 6, 2, levels=2)
# every window of 8 frames at d = 1 (36) and at d = 2 (20), and the 8 single frames as d = 4 windows: 64 distinct rows
K64 = [(s, n, 1) for s in range(8) for n in range(1, 9 - s)] + [(s, n, 2) for s in range(8) for n in range(1, (7 - s) // 2 + 2)] \
    + [(s, 1, 4) for s in range(8)]
assert len(K64) == len(set(K64)) == 64
CASES = {
    # C = 4; h*w in {1, 15, 12, 64}: E = 1, 1, 4 and 8
    "T = 3, h*w = 1, {0, 2} and {1} at d = 2": dict(C=4, T=3, h=1, w=1, table=[(0, 3, 1), (0, 2, 2), (1, 1, 2)], ov=1),
    "T = 5, h*w = 15: scalar path": dict(C=4, T=5, h=3, w=5, table=[(0, 4, 1), (2, 3, 1), (0, 3, 2), (1, 2, 2)], ov=2),
    "T = 8, h*w = 12: 8-byte path": dict(C=4, T=8, h=3, w=4, table=TWO_LEVELS, ov=2),
    "T = 8, h*w = 64: 16-byte path": dict(C=4, T=8, h=8, w=8, table=TWO_LEVELS, ov=2),
    "T = 9, d = 1, 2 and 4": dict(C=4, T=9, h=3, w=4, ov=1,
                                  table=[(0, 5, 1), (4, 5, 1), (0, 5, 2), (1, 4, 2), (0, 3, 4), (1, 2, 4), (2, 2, 4), (3, 2, 4)]),
    "an odd offset forces E = 1": dict(C=4, T=8, h=8, w=8, table=TWO_LEVELS, ov=2, pads=[0, 1, 0, 2]),
    "an offset a multiple of 4 only": dict(C=4, T=8, h=8, w=8, table=TWO_LEVELS, ov=2, pads=[0, 0, 4, 0]),
    "K = 64": dict(C=4, T=8, h=3, w=4, table=K64, ov=1),
    "more than one tile per line": dict(C=2, T=4, h=48, w=48, table=[(0, 4, 1), (0, 2, 2), (1, 2, 2)], ov=1),
}


@pytest.mark.parametrize("name", list(CASES))
def test_strided_steps_match_the_restatement(gpu, name):
    _check_case(gpu, *_case(seed=3, **CASES[name]), name)


@pytest.mark.parametrize("h,w,pads", [(8, 8, None), (3, 5, None), (3, 4, None), (8, 8, [0, 1, 2])], ids=["E8", "E1", "E4", "odd offsets"])
def test_a_table_of_strides_one_is_the_cofuse_step(gpu, h, w, pads):
    from vdx.codenoise import window_table
    from vdx.planner import ChunkPlan
    ops, _ = _ops()
    table = [(0, 4, 1), (2, 4, 1), (4, 4, 1)]
    z, prev, wins, packed, rows, wn = _case(4, 8, h, w, table, 2, seed=7, pads=pads)
    assert torch.equal(wn, window_table(ChunkPlan(4, 2, tuple((s, s + n) for s, n, _ in table), 1), 8).wn)
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    flat = [r[:3] for r in rows]
    for variant, i in VARIANTS:
        got, got_x0 = _run(ops, variant, i, zg, bg, rows, wg, pg)
        want, want_x0 = _run(ops, variant, i, zg, bg, flat, wg, pg, strided=False)
        _same_bits(got, want, f"{variant} lat'")
        if want_x0 is not None:
            _same_bits(got_x0, want_x0, f"{variant} x0")


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (3, 4), (8, 8)])
def test_the_stride_by_permutation(gpu, h, w):
    """The test of the stride itself: a table of d = 2 windows only, on an even clip.  Permuting the clip's frames to
    evens-then-odds makes it a flat d = 1 table: the strided step equals the flat step on the permuted clip, permuted back."""
    ops, _ = _ops()
    T = 8
    table = [(0, 3, 2), (2, 3, 2), (1, 4, 2)]                        # frames 0 2 4 | 2 4 6 | 1 3 5 7
    flat = [(0, 3), (1, 3), (4, 4)]                                  # the same windows at their permuted positions
    z, prev, wins, packed, rows, wn = _case(4, T, h, w, table, 1, seed=9)
    perm = torch.tensor([0, 2, 4, 6, 1, 3, 5, 7])
    rows_flat = [(off, s, n) for (off, _, _, _), (s, n) in zip(rows, flat)]
    bg = packed.to(gpu)
    zp, pp, wp = (t.contiguous().to(gpu) for t in (z[:, :, perm], prev[:, :, perm], wn[:, perm]))
    for variant, i in VARIANTS[:3]:
        got, got_x0 = _run(ops, variant, i, z.to(gpu), bg, rows, wn.to(gpu), prev.to(gpu))
        want, want_x0 = _run(ops, variant, i, zp, bg, rows_flat, wp, pp, strided=False)
        _same_bits(got[:, :, perm.to(gpu)].contiguous(), want, f"{variant} lat'")
        if want_x0 is not None:
            _same_bits(got_x0[:, :, perm.to(gpu)].contiguous(), want_x0, f"{variant} x0")


@pytest.mark.parametrize("name", ["T = 8, h*w = 64: 16-byte path", "T = 5, h*w = 15: scalar path"])
def test_nan_and_inf_stay_in_their_element(gpu, name):
    """A NaN in u and an inf in c, each in one element of the LAST window's block (a strided one) at its last frame: each shows
    in that element (c, s + f * d, p) of the outputs and nowhere else."""
    ops, _ = _ops()
    clean = _case(seed=5, **CASES[name])
    case = _case(seed=5, **CASES[name])
    z, prev, wins, packed, rows, wn = case
    C, T, h, w = z.shape[1:]
    off, s, n, d = rows[-1]
    f = n - 1
    assert d == 2
    t = s + f * d
    spots = [(0, 1, f, h - 1, w - 1, NAN), (1, C - 1, f, 0, 0, float("inf"))]
    touched = torch.zeros(z.shape, dtype=torch.bool)
    for half, c, ff, y, x, v in spots:
        wins[-1][half, c, ff, y, x] = v
        packed[off + (((half * C + c) * n + ff) * h + y) * w + x] = v
        touched[0, c, t, y, x] = True
    table = [r[1:] for r in rows]
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
    z, prev, wins, packed, rows, wn = _case(seed=13, **CASES["T = 8, h*w = 64: 16-byte path"])
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    coeffs = _ddim_coeffs()[2]
    want = ops.costride_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs)
    assert torch.equal(want, ops.costride_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs))
    x = zg.clone()
    assert ops.costride_cfg_ddim_step(x, bg, rows, wg, GS, coeffs, out=x) is x and torch.equal(x, want)
    for i, second in ((0, False), (2, True)):
        c = _coeffs(_dpm(i, second))
        want, want_x0 = ops.costride_cfg_dpm_step(zg, bg, rows, wg, GS, c, x0_prev=pg if second else None)
        x = zg.clone()
        got, got_x0 = ops.costride_cfg_dpm_step(x, bg, rows, wg, GS, c, x0_prev=pg if second else None, out=x)
        assert got is x and torch.equal(x, want) and torch.equal(got_x0, want_x0)


def test_bad_tables_are_refused_before_a_launch(gpu):
    """Only the errors are asserted: every call below is refused by the host checks, nothing is launched."""
    ops, VdxError = _ops()
    z, prev, wins, packed, rows, wn = _case(seed=17, **CASES["T = 8, h*w = 64: 16-byte path"])
    zg, bg, wg = z.to(gpu), packed.to(gpu), wn.to(gpu)
    coeffs, T = _ddim_coeffs()[0], z.shape[2]
    r = rows
    short = packed.numel() - 2 * 4 * 4 * 64 + 8                      # the last window's block would end 8 elements past the buffer
    bad = {"d = 0": [r[0], r[1], (r[2][0], 0, 4, 0), r[3]], "d < 0": [r[0], r[1], (r[2][0], 0, 4, -2), r[3]],
           "s + (L - 1) d = T": [r[0], r[1], (r[2][0], 2, 4, 2), r[3]], "s + (L - 1) d > T": [r[0], r[1], r[2], (r[3][0], 1, 4, 3)],
           "a product past 2^31": [r[0], r[1], r[2], (r[3][0], 1, 4, 2 ** 30)], "s < 0": [(r[0][0], -1, 6, 1), r[1], r[2], r[3]],
           "L = 0": [r[0], r[1], r[2], (r[3][0], 1, 0, 2)], "odd frames in no window": [(r[2][0], 0, 4, 2)],
           "frame 7 in no window": [(r[0][0], 0, 6, 1), (r[2][0], 0, 4, 2)],
           "leaves the buffer": [r[0], r[1], r[2], (short, 1, 4, 2)], "negative offset": [(-8, 0, 6, 1), r[1], r[2], r[3]]}
    for what, table in bad.items():
        w = wg[:len(table)].contiguous()
        with pytest.raises(VdxError):
            ops.costride_cfg_ddim_step(zg, bg, table, w, GS, coeffs)
        with pytest.raises(VdxError):
            ops.costride_cfg_dpm_step(zg, bg, table, w, GS, _coeffs(_dpm(0, False)))
    with pytest.raises(VdxError, match="no window"):
        ops.costride_cfg_ddim_step(zg, bg, bad["frame 7 in no window"], wg[:2].contiguous(), GS, coeffs)
    many = [(0, 0, T, 1)] * 65
    with pytest.raises(VdxError, match="64"):
        ops.costride_cfg_ddim_step(zg, bg, many, torch.ones(65, T, device=gpu), GS, coeffs)
    lib = ops._lib.load()                                           # and by the library itself, not only by the wrapper
    import ctypes
    off, st, ln = (ctypes.c_int64 * 65)(), (ctypes.c_int32 * 65)(), (ctypes.c_int32 * 65)(*([T] * 65))
    sd = (ctypes.c_int32 * 65)(*([1] * 65))
    w65 = torch.ones(65, T, device=gpu)
    out = torch.empty_like(zg)
    args = (zg.data_ptr(), bg.data_ptr(), bg.numel(), off, st, ln)
    tail = (w65.data_ptr(), out.data_ptr(), GS, *coeffs, z.shape[1], T, z.shape[3] * z.shape[4], None)
    assert lib.vdx_costride_cfg_ddim_step_f16(*args, sd, 65, *tail) != 0 and b"64" in lib.vdx_last_error()
    assert lib.vdx_costride_cfg_ddim_step_f16(*args, sd, 0, *tail) != 0
    assert lib.vdx_costride_cfg_ddim_step_f16(*args, None, 4, *tail) != 0 and b"null" in lib.vdx_last_error()
    # misaligned pointers: the windows buffer, z and the output one element off a 16-byte boundary
    with pytest.raises(VdxError, match="aligned"):
        ops.costride_cfg_ddim_step(zg, bg[1:], rows, wg, GS, coeffs)
    one = (ctypes.c_int32 * 65)(*([1] * 65))
    for shifted in ((zg.data_ptr() + 2, bg.data_ptr()), (zg.data_ptr(), bg.data_ptr() + 2)):   # the library's own check
        assert lib.vdx_costride_cfg_ddim_step_f16(*shifted, bg.numel() - 1, off, st, ln, one, 1, *tail) != 0
        assert b"aligned" in lib.vdx_last_error()
    odd =torch.empty(zg.numel() + 1, dtype=torch.float16, device=gpu)[1:].view(zg.shape)
    with pytest.raises(VdxError, match="aligned"):
        ops.costride_cfg_ddim_step(odd, bg, rows, wg, GS, coeffs)
    with pytest.raises(VdxError, match="aligned"):
        ops.costride_cfg_ddim_step(zg, bg, rows, wg, GS, coeffs, out=odd)
    for s, n, d in ((0, 4, 0), (0, 4, -1), (2, 4, 2), (-1, 2, 1), (0, 0, 1), (1, 2, 2 ** 30), (T, 1, 1)):
        with pytest.raises(VdxError):
            ops.cfg_input_stride(zg, None, 0.0, s, n, d)
    torch.cuda.synchronize()


@pytest.mark.parametrize("T,h,w", [(3, 1, 1), (5, 3, 5), (8, 8, 8), (5, 3, 4)])
def test_cfg_input_stride(gpu, T, h, w):
    """Against `index_select` + `ops.cfg_input` and the restatement; d = 1 against `cfg_input_window`."""
    ops, _ = _ops()
    g = torch.Generator().manual_seed(19)
    z = torch.randn(1, 4, T, h, w, generator=g).half()
    z.view(-1)[:4] = torch.tensor([65504.0, -0.0, 2.0 ** -24, float("inf")], dtype=torch.float16)
    ctx = torch.randn(1, 4, 1, h, w, generator=g).half()
    zg, cg = z.to(gpu), ctx.to(gpu)
    for d in (1, 2, 3, T - 1):
        for s in range(min(d, T - 1) + 1):
            longest = (T - 1 - s) // d + 1
            for n in sorted({1, longest, max(1, longest - 1)}):
                for c, cw in ((None, 0.0), (cg, 0.35)):
                    got = ops.cfg_input_stride(zg, c, cw, s, n, d)
                    assert got.is_contiguous() and tuple(got.shape) == (2, 4, n, h, w) and ops.is_cfg_duplicate(got)
                    _same_bits(got, S.cfg_input_stride(z, None if c is None else ctx, cw, s, n, d), f"s = {s}, L = {n}, d = {d}")
                    idx = (s + d * torch.arange(n)).to(gpu)
                    _same_bits(got, ops.cfg_input(zg.index_select(2, idx).contiguous(), c, cw), "against index_select + cfg_input")
                    if d == 1:
                        _same_bits(got, ops.cfg_input_window(zg, c, cw, s, s + n), "against cfg_input_window")
    got.add_(1)
    assert not ops.is_cfg_duplicate(got)                            # a write drops the tag, as for cfg_input


# ---- the job on the tiny golden UNet ------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 8, 32, 32, 2
WINDOWS = [[0, 6, 1], [4, 4, 1], [0, 4, 2], [1, 4, 2]]              # stride_plan(8, 1, 6, 2, levels=2)
RANGES = [(0, 6), (4, 8)]                                           # level 0: what `info["ranges"]` carries
RECORD = {"levels": 2, "strides": [1, 2], "windows": WINDOWS}
INFO_KEYS = {"chunk_size", "overlap", "ranges", "world_size", "num_frames", "denoise_s", "exchange", "steps_run",
             "emu_gather_delay_s", "net_gather_s", "network_bytes", "payload_bytes", "payload_bytes_actual"}


def _config(**kw):
    from vdx.pipeline import DiffuserConfig
    kw = {**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                 device="cuda", noise_device="cpu", co_denoise=True, context_stride=2), **kw}
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
    """The strided round, written out: per step every window's UNet output from `ops.cfg_input` on an index_select of the clip,
    the restatement's fuse and chain on the CPU, then (masked: (x0, base, latent mask)) tests/inpaint_ref.py's restatement of the
    mask step on the whole clip.  -> fp16 latent on the CPU."""
    from vdx import ops
    from vdx.codenoise import stride_plan, stride_table
    m, emb = model
    emb2 = torch.cat([emb[1:], emb[:1]], dim=0)
    n_frames = start.shape[2]
    sp = stride_plan(n_frames, 1, d.cfg.chunk_size, d.cfg.overlap, "coherent", d.cfg.context_stride)
    assert [list(w) for w in sp.windows] == WINDOWS
    wn, table = stride_table(sp, n_frames).wn, list(sp.windows)
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
        for s, length, stride in table:
            idx = (s + stride * torch.arange(length)).to(start.device)
            x = ops.cfg_input(zg.index_select(2, idx).contiguous(), ctx, d.cfg.context_weight)
            outs.append(m(x, t, encoder_hidden_states=emb2).sample.cpu())
        if sampler == "ddim":
            z = S.costride_ddim(z, outs, table, wn, d.cfg.guidance_scale, d.scheduler.coefficients(t))
        else:
            i = first + j
            second = x0_prev is not None and i != n - 1
            z, x0_prev = S.costride_dpm(z, outs, table, wn, d.cfg.guidance_scale, dpm_ref.scalars(dpm_ref.sigmas(n), i, second),
                                        x0_prev if second else None)
        if masked is not None:
            sa, s1 = coef[j] if coef[j] is not None else (0.0, 0.0)
            z = inpaint_ref.renoise_ref(z, x0c, basec, lmc, sa, s1, coef[j] is None, 0)
    return z


def _base(d):
    from vdx.pipeline import seeded_noise
    return seeded_noise(d.latent_shape, d.scheduler.init_noise_sigma, "cuda", "cpu")


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_strided_job_is_the_loop_and_the_same_on_every_run(model, sampler):
    d = _diffuser(model, sampler)
    lat, info = d()
    assert info["ranges"] == RANGES and lat.dtype == torch.float32 and tuple(lat.shape) == d.latent_shape
    want = _loop(d, model, _base(d), d.ctx, sampler)
    assert bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat), _bits(want.float()))
    again, _ = d()
    assert torch.equal(_bits(again), _bits(lat))                    # run to run
    assert set(info) == INFO_KEYS | {"co_denoise", "context_stride"} and info["context_stride"] == RECORD
    rec = info["co_denoise"]
    assert (rec["windows"], rec["steps"], rec["bytes_per_step"], rec["context_stride"]) == (4, STEPS, 0, RECORD)
    assert info["chunk_size"] == 6 and info["overlap"] == 2
    assert info["payload_bytes"] == STEPS * (6 + 4 + 4 + 4) * 4 * 2
    assert info["payload_bytes_actual"] == STEPS * (6 + 4 + 4 + 4) * (2 * 4 * HL * WL * 2)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_one_level_is_the_plain_co_denoised_job(model, sampler):
    """`context_stride = 1`, the default: the plain co-denoised job's bits and records, and no `context_stride` key anywhere."""
    from vdx import ops
    from vdx.pipeline import DiffuserConfig

    def never(*a, **kw):
        raise AssertionError("a strided op ran in a job with one level")
    strided_ops = ("cfg_input_stride", "costride_cfg_ddim_step", "costride_cfg_dpm_step")
    kept = {name: getattr(ops, name) for name in strided_ops}
    try:
        for name in strided_ops:                                    # one level takes the plain path: windows, launches and all
            setattr(ops, name, never)
        one, info1 = _diffuser(model, sampler, context_stride=1)()
        d0 = _diffuser(model, sampler)
        d0.cfg = DiffuserConfig(**{k: v for k, v in vars(d0.cfg).items() if k != "context_stride"})    # the field's default
        plain, info0 = d0()
    finally:
        for name, fn in kept.items():
            setattr(ops, name, fn)
    assert torch.equal(_bits(one), _bits(plain)) and info0["ranges"] == info1["ranges"] == RANGES
    for info in (info0, info1):
        assert set(info) == INFO_KEYS | {"co_denoise"} and set(info["co_denoise"]) == {"windows", "steps", "exchange_s", "bytes_per_step"}
    timed = ("denoise_s", "net_gather_s")
    assert {k: v for k, v in info0.items() if k not in timed and k != "co_denoise"} == \
           {k: v for k, v in info1.items() if k not in timed and k != "co_denoise"}
    strided, _ = _diffuser(model, sampler)()
    assert not torch.equal(strided, plain)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_masked_strided_job_is_the_loop_with_the_mask_step(gpu, model, sampler):
    from dist_inpaint_worker import clean_latent
    from vdx import inpaint, ops
    clean = clean_latent(T, HL, WL, gpu)
    px = torch.from_numpy(inpaint.expand_mask(inpaint.keep_frames_mask("0:2,7", T), T, HL * 8, WL * 8))
    lm = ops.mask_to_latent(px.to(gpu))
    d = _diffuser(model, sampler, init_latents=clean, latent_mask=lm, steps=4, strength=0.75)
    assert len(d.schedule) == 3
    lat, info = d()
    assert info["steps_run"] == 3 and info["ranges"] == RANGES and info["context_stride"] == RECORD
    want = _loop(d, model, d._start, d.ctx, sampler, masked=(clean, d._base, lm))
    assert torch.equal(_bits(lat), _bits(want.float()))
    keep = ~lm.bool().cpu()[None, None].expand(lat.shape)
    assert torch.equal(_bits(lat)[keep], _bits(clean.float())[keep]) and int(keep[0, 0, :, 0, 0].sum()) == 3


def test_free_init_rounds_are_strided_too(model):
    d = _diffuser(model, free_init_iters=2)
    lat, info = d()
    assert len(d.free_init_starts) == 1 and info["co_denoise"]["steps"] == 2 * STEPS and info["context_stride"] == RECORD
    start = d.free_init_starts[0]
    want = _loop(d, model, start, start.mean(dim=2, keepdim=True).contiguous(), "ddim")
    assert torch.equal(_bits(lat), _bits(want.float()))


# ---- run_job end to end on synthetic weights ---------------------------------------------------------------------------------
def test_run_job_end_to_end(gpu, tmp_path):
    """128 x 128, 8 frames, chunk 6, overlap 2: with `--context_stride 2` the result carries the record, inside "co_denoise" too,
    the ranges handed to the metrics are the level-0 windows, and the frames differ from the plain co-denoised job's; with
    `--context_stride 1` the result has the plain job's keys and frames."""
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import build_arg_parser, config_from_args, run_job
    F = 8
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    base = ["--model_id", "synthetic:tiny", "--num_frames", str(F), "--steps", "2", "--height", "128", "--width", "128", "--chunk_size", "6",
            "--overlap", "2", "--noise_device", "cpu", "--co_denoise"]

    def job(extra, out_video=None):
        got = {}
        res = run_job(config_from_args(build_arg_parser().parse_args(base + extra)), out_video=out_video, pipe=pipe, clip_inputs=got)
        return res, got
    res0, got0 = job([])
    res1, got1 = job(["--context_stride", "2"], out_video=str(tmp_path / "strided.mp4"))
    res2, got2 = job(["--context_stride", "1"])
    assert "context_stride" not in res0 and set(res1) == set(res0) | {"context_stride"} and set(res2) == set(res0)
    assert res1["context_stride"] == RECORD == res1["co_denoise"]["context_stride"] and "context_stride" not in res0["co_denoise"]
    assert [tuple(r) for r in got1["ranges"]] == RANGES == [tuple(r) for r in got0["ranges"]]
    assert res1["temp_instab"] is not None and res1["co_denoise"]["windows"] == 4 and res0["co_denoise"]["windows"] == 2
    frames = np.stack(got1["frames"])
    assert frames.shape == (F, 128, 128, 3) and not np.array_equal(frames, np.stack(got0["frames"]))
    assert np.array_equal(np.stack(got2["frames"]), np.stack(got0["frames"]))
    assert res1["frames_written"] == F and os.path.getsize(tmp_path / "strided.mp4") > 0
