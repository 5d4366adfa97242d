"""Dynamic thresholding with a mimic scale on the GPU (csrc/dynthresh.hip, vdx/scheduler.py, vdx/pipeline.py) against the torch-CPU
restatement of tests/dynthresh_ref.py, stage by stage: each stage is compared with the restatement fed the kernel's own output of
the stage before, so no sum order leaks into a comparison of bits; then end to end on seeds whose channel means lie further from
an fp16 rounding boundary than the sum bound (asserted here); the co-fused variants; ties, a constant channel, signed zeros,
infinity and NaN; the schedulers; the job against a Python loop over its windows, and the defaults untouched.

A NaN's sign and payload are the platform's (0/0 is +NaN on the GPU and -NaN in torch on x86), so `_same` asks that NaNs sit at the
same elements and that every other element has the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

import codenoise_ref as CR
import dpm_ref
import dynthresh_ref as D
import stats_order_ref as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (T, h, w) with M = 1, 2, 7 (one half per access), 12 (four), 8, 257 * 8 (eight, two rows per channel, a ragged last block) and
# 9216 (eight, five rows per channel), each with C = 1, 3 and 4
DIMS = [(1, 1, 1), (1, 1, 2), (7, 1, 1), (2, 2, 2), (3, 2, 2), (2, 4, 257), (4, 48, 48)]
SHAPES = [(C,) + d for d in DIMS for C in (1, 3, 4)]
QS = (1.0, 0.995, 0.5, None, 1e-9)                                 # None: 1 / M
GS, MS = 7.5, 3.0
DDIM = (0.9493, 0.3143, 0.4206, 0.9073)                            # any four fp32 coefficients: the chain is pinned, not the schedule
CANARY = 256


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    return ops, VdxError


def _u16(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.float16 else t.view(torch.int32).numpy().view(np.uint32)


def _same(got, want, what):
    """Bits equal, a NaN at the same elements counting as equal."""
    assert tuple(got.shape) == tuple(want.shape), what
    a, b = _u16(got), _u16(want)
    if a.dtype == np.uint16:
        na, nb = (a & 0x7fff) > 0x7c00, (b & 0x7fff) > 0x7c00
    else:
        na, nb = (a & 0x7fffffff) > 0x7f800000, (b & 0x7fffffff) > 0x7f800000
    assert np.array_equal(na, nb), f"{what}: NaNs at different elements ({int(na.sum())} vs {int(nb.sum())})"
    bad = (a != b) & ~na
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ"


def _same_scal(got, want, what):
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    nan = ((got & 0x7fff) > 0x7c00) & ((want & 0x7fff) > 0x7c00)
    assert np.array_equal(got[~nan], want[~nan]), f"{what}: scal {got.tolist()} vs the restatement's {want.tolist()}"


_CASES = {}
# Seeds picked beforehand, on the CPU and with the restatement alone: the first of base, base + 1000, ... at which every channel
# mean, at both pairs of scales the end-to-end test uses, lies further from an fp16 rounding boundary than the bound of a
# fixed-order float64 sum (`dynthresh_ref.mean_margin`; with M = 2 or 8 a mean of halves lands exactly on a tie now and then).
# The end-to-end tests assert the condition themselves.
SEED_OFFSET = {(3, 1, 1, 2): 2000, (4, 1, 1, 2): 15000, (4, 7, 1, 1): 2000, (3, 2, 2, 2): 3000, (1, 3, 2, 2): 1000}


def _case(shape):
    """Seeded Gaussian u, c, x and an x0 history at `shape` = (C, T, h, w), made once and never written."""
    if shape not in _CASES:
        g = torch.Generator().manual_seed(2000 + 7 * shape[0] + sum(shape) + SEED_OFFSET.get(shape, 0))
        _CASES[shape] = tuple(torch.randn((k,) + shape, generator=g).half() for k in (2, 1, 1))
    return _CASES[shape]


def _workspace(ops, shape, gpu):
    """A workspace filled with 0xFF with canaries behind it -> (the whole buffer, the workspace's view)."""
    need = ops.mimic_ws_bytes(shape[0], shape[1], shape[2] * shape[3])
    buf = torch.full((need + CANARY,), 0xFF, dtype=torch.uint8, device=gpu)
    return buf, buf[:need]


def _kernel_sums(views, C, rows):
    """The kernel's rows added in ascending order, as its blocks add them -> float64 (C, 2)."""
    part = views["partials"].cpu().numpy()
    S = np.zeros((C, 2))
    for ch in range(C):
        for q in range(2):
            acc = part[ch, 0, q]
            for r in range(1, rows):
                acc = acc + part[ch, r, q]
            S[ch, q] = acc
    return S


def _rows(M):
    width = 8 if M % 8 == 0 else 4 if M % 4 == 0 else 1
    return min(64, -(-(M // width) // 256))


def _stages(ops, gpu, eps2, x, prev, gs, ms, qs, rows, stats, steps, what, finite=True):
    """Every stage of one sample against the restatement fed the stage before: `stats(ws, factors, stages)` runs the statistics
    launches, `steps` = (ddim(ws, out), dpm(ws, x0_prev, out)) the step ops."""
    C, M = eps2.shape[1], eps2[0, 0].numel()
    buf, ws = _workspace(ops, tuple(eps2.shape[1:]), gpu)
    stats(ws, ops.mimic_factors(ms, 1.0, M), 7)
    v = ops.mimic_ws_views(ws, C)
    # sums
    S = _kernel_sums(v, C, rows)
    if finite:
        want, scale = D.sums64(eps2, gs, ms)
        err, bound = np.abs(S - want), M * 2.0 ** -53 * scale
        print(f"PARITY {what}: sums |diff| max {err.max():.3e} <= bound min {bound.min():.3e}; C {C} M {M}; compared bit for bit: "
              f"{C * 32768} bins, {len(qs)} x {C * 4} scalars, 6 x {C * M} step outputs")
        assert (err <= bound).all(), f"{what}: sums"
    means = D.means_of(S, M)
    # histogram and maximum, from the kernel's own means
    hist, maxbits = D.histogram(eps2, gs, ms, means)
    assert torch.equal(v["hist"].cpu().long(), hist), f"{what}: hist"
    assert int(v["hist"].sum()) == C * M
    assert torch.equal(v["maxbits"].cpu().long(), maxbits), f"{what}: maxbits"
    keep = v["partials"][:, :rows].cpu().clone()
    # select, every percentile on the same counts
    scal = None
    for q in qs:
        q = 1.0 / M if q is None else q
        stats(ws, ops.mimic_factors(ms, q, M), 4)
        scal = _u16(v["scal"])
        _same_scal(scal, D.select(eps2, gs, ms, q, means), f"{what} q {q}")
    assert bool((buf[-CANARY:] == 0xFF).all()), f"{what}: the canaries behind the workspace changed"
    # the steps, from the kernel's own scalars (the last percentile's)
    ddim, dpm = steps
    xg = x.to(gpu)
    got = ddim(ws, None)
    _same(got, D.ddim_step(eps2, x, gs, ms, 1.0, DDIM, scal=scal), f"{what}: ddim")
    y = xg.clone()
    assert ddim(ws, y, lat=y) is y
    _same(y, got, f"{what}: ddim in place")
    sig = dpm_ref.sigmas(10)
    for second in (False, True):
        k = dpm_ref.scalars(sig, 4, second)
        new, x0 = dpm(ws, prev.to(gpu) if second else None, None, k)
        want, want0 = D.dpm_step(eps2, x, prev if second else None, gs, ms, 1.0, k, scal=scal)
        _same(new, want, f"{what}: dpm order {1 + second}")
        _same(x0, want0, f"{what}: dpm order {1 + second}: history")
    # run to run: the whole workspace, bit for bit
    first = ws.cpu().clone()
    stats(ws, ops.mimic_factors(ms, 1.0 / M if qs[-1] is None else qs[-1], M), 7)
    assert torch.equal(ws.cpu(), first), f"{what}: run to run"
    assert torch.equal(v["partials"][:, :rows].cpu().view(torch.int64), keep.view(torch.int64))
    return scal


def _dpm_coeffs(k):
    return (k["s0"], k["inv_a0"], k["cx"], -k["k"], -k.get("half_k", 0.0), k.get("inv_r0", 0.0))


def _flat(ops, gpu, eps2, x, gs):
    """`_stages`' callables for the flat form."""
    e, xg = eps2.to(gpu), x.to(gpu)

    def stats(ws, fac, stages):
        assert ops.cfg_mimic_stats(e, gs, fac, ws=ws, stages=stages) is ws

    def ddim(ws, out, lat=None):
        return ops.cfg_mimic_ddim_step(e, xg if lat is None else lat, gs, DDIM, ws, out=out)

    def dpm(ws, prev, out, k):
        return ops.cfg_mimic_dpm_step(e, xg, gs, _dpm_coeffs(k), ws, x0_prev=prev, out=out)
    return stats, (ddim, dpm)


# (C, T, HW) = (3, 2, 24), (3, 2, 20), (3, 1, 7): M a multiple of 8, of 4 only, and odd, so a channel boundary falls inside what a
# wider access would span
WIDTHS = [(3, 2, 4, 6), (3, 2, 4, 5), (3, 1, 1, 7)]


@pytest.mark.parametrize("shape", SHAPES + WIDTHS, ids=str)
def test_every_stage_from_the_stage_before(gpu, shape):
    ops, _ = _ops()
    eps2, x, prev = _case(shape)
    M = shape[1] * shape[2] * shape[3]
    rows = _rows(M)
    assert (rows > 1) == (M >= 2056)
    stats, steps = _flat(ops, gpu, eps2, x, GS)
    _stages(ops, gpu, eps2, x, prev, GS, MS, QS, rows, stats, steps, str(shape))


def _levels(shape, seed):
    g = torch.Generator().manual_seed(seed)
    lv = torch.tensor([-1.5, -0.25, 0.0, 0.5, 2.0])
    return lv[torch.randint(0, 5, (2,) + shape, generator=g)].half()


def _data_cases():
    shape = (3, 2, 4, 9)                                           # M = 72: eight halves per access
    base = _case(shape)[0]
    cases = {"ties": (_levels(shape, 11), GS, MS), "ms above gs": (base, 2.0, 7.0)}
    for gs in (2.0, 7.5, 15.0):
        cases[f"gs {gs}"] = (base, gs, 1.5)
    const = base.clone()
    const[:, 1] = 0.25
    cases["constant channel"] = (const, GS, MS)
    zeros = base.clone()
    zeros[0, 0, 0] = 0.0
    zeros[1, 0, 0] = -0.0
    zeros[0, 2, 1, :2] = -0.0
    zeros[1, 2, 1, :2] = 0.0
    cases["signed zeros"] = (zeros, GS, MS)
    bad = base.clone()
    bad[1, 2, 0, 1, 1] = float("inf")
    bad[0, 0, 1, 2, 3] = float("nan")
    cases["inf and nan"] = (bad, GS, MS)
    return shape, cases


@pytest.mark.parametrize("name", ["ties", "ms above gs", "gs 2.0", "gs 7.5", "gs 15.0", "constant channel", "signed zeros", "inf and nan"])
def test_data_cases(gpu, name):
    ops, _ = _ops()
    shape, cases = _data_cases()
    eps2, gs, ms = cases[name]
    _, x, prev = _case(shape)
    stats, steps = _flat(ops, gpu, eps2, x, gs)
    scal = _stages(ops, gpu, eps2, x, prev, gs, ms, (0.5, 0.995, 1.0), 1, stats, steps, name, finite=name != "inf and nan")
    out = steps[0](_ws_after(ops, gpu, eps2, gs, ms), None).cpu()
    nan = torch.isnan(out[0]).reshape(shape[0], -1)
    if name == "constant channel":                                 # s = 0: the NaN the lines give, and only in that channel
        assert scal[1, 3] == 0 and bool(nan[1].all()) and not bool(nan[0].any()) and not bool(nan[2].any())
    elif name == "inf and nan":                                    # they stay in their channels
        assert bool(nan[0].all()) and bool(nan[2].all()) and not bool(nan[1].any())
    else:
        assert not bool(nan.any())
    if name == "ms above gs":                                      # ref_lo is the larger: s is ref_lo
        assert (scal[:, 3] == scal[:, 1]).all() and (scal[:, 1] > scal[:, 2]).all()


def _ws_after(ops, gpu, eps2, gs, ms, q=1.0):
    return ops.cfg_mimic_stats(eps2.to(gpu), gs, ops.mimic_factors(ms, q, eps2[0, 0].numel())).clone()


# ---- end to end: the restatement's own statistics -------------------------------------------------------------------------------
def _assert_margin(eps2, gs, ms, what):
    dist, bound = D.mean_margin(eps2, gs, ms)
    assert (dist > bound).all(), f"{what}: a channel mean lies within the sum bound of an fp16 rounding boundary: pick another seed"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("gs,ms,q", [(7.5, 3.0, 0.995), (15.0, 7.0, 1.0)])
def test_stats_and_step_end_to_end(gpu, shape, gs, ms, q):
    ops, _ = _ops()
    eps2, x, prev = _case(shape)
    _assert_margin(eps2, gs, ms, str(shape))
    e, xg, M = eps2.to(gpu), x.to(gpu), shape[1] * shape[2] * shape[3]
    ws = ops.cfg_mimic_stats(e, gs, ops.mimic_factors(ms, q, M))
    _same_scal(_u16(ops.mimic_ws_views(ws, shape[0])["scal"]), D.stats(eps2, gs, ms, q), str(shape))
    _same(ops.cfg_mimic_ddim_step(e, xg, gs, DDIM, ws), D.ddim_step(eps2, x, gs, ms, q, DDIM), f"{shape} ddim")
    k = dpm_ref.scalars(dpm_ref.sigmas(10), 4, True)
    new, x0 = ops.cfg_mimic_dpm_step(e, xg, gs, _dpm_coeffs(k), ws, x0_prev=prev.to(gpu))
    want, want0 = D.dpm_step(eps2, x, prev, gs, ms, q, k)
    _same(new, want, f"{shape} dpm")
    _same(x0, want0, f"{shape} dpm history")


def test_through_the_schedulers(gpu):
    """`step_cfg(..., cfg_mimic=...)` is `ops` called by hand: DDIM once, DPM-Solver++ twice so both orders run."""
    ops, _ = _ops()
    from vdx.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    shape = (4, 4, 48, 48)
    eps2, x, _ = _case(shape)
    e, gs, ms, q, M = eps2.to(gpu), 15.0, 7.0, 0.995, 9216
    fac = ops.mimic_factors(ms, q, M)
    s = DDIMScheduler()
    s.set_timesteps(10, device=gpu)
    t = s._host_timesteps[2]
    got = s.step_cfg(e, t, x.to(gpu), gs, cfg_mimic=ms, cfg_mimic_percentile=q)
    _same(got, ops.cfg_mimic_ddim_step(e, x.to(gpu), gs, s.coefficients(t), ops.cfg_mimic_stats(e, gs, fac)), "ddim")
    assert not torch.equal(got, s.step_cfg(e, t, x.to(gpu), gs))
    with pytest.raises(ValueError, match="exclude each other"):
        s.step_cfg(e, t, x.to(gpu), gs, guidance_rescale=0.5, cfg_mimic=ms)
    p = DPMSolverMultistepScheduler()
    p.set_timesteps(10, device=gpu)
    lat, ref, prev = x.to(gpu), x.to(gpu), None
    for i in (3, 4):
        lat = p.step_cfg(e, p._host_timesteps[i], lat, gs, cfg_mimic=ms, cfg_mimic_percentile=q)
        ref, x0 = ops.cfg_mimic_dpm_step(e, ref, gs, p.coefficients(i, prev is not None), ops.cfg_mimic_stats(e, gs, fac), x0_prev=prev)
        prev = x0.clone()
        _same(lat, ref, f"dpm step {i}")


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


@pytest.mark.parametrize("C,T,h,w,table", [(4, 6, 4, 6, [(0, 4), (2, 4)]), (3, 7, 3, 5, [(0, 4), (2, 4), (3, 4)]),
                                           (4, 8, 32, 32, [(0, 6), (4, 4)])], ids=str)
def test_cofused_stages_and_end_to_end_on_the_fused_noise(gpu, C, T, h, w, table):
    ops, _ = _ops()
    wins, packed, rows, wn = _windows(C, T, h, w, table, 7 + T)
    g = torch.Generator().manual_seed(T)
    z, prev = (torch.randn(1, C, T, h, w, generator=g).half() for _ in range(2))
    eps2 = CR.fuse(wins, table, wn, z.shape)
    zg, bg, wg = z.to(gpu), packed.to(gpu), wn.to(gpu)

    def stats(ws, fac, stages):
        assert ops.cofuse_cfg_mimic_stats(zg, bg, rows, wg, GS, fac, ws=ws, stages=stages) is ws

    def ddim(ws, out, lat=None):
        return ops.cofuse_cfg_mimic_ddim_step(zg if lat is None else lat, bg, rows, wg, GS, DDIM, ws, out=out)

    def dpm(ws, p, out, k):
        return ops.cofuse_cfg_mimic_dpm_step(zg, bg, rows, wg, GS, _dpm_coeffs(k), ws, x0_prev=p, out=out)
    _stages(ops, gpu, eps2, z, prev, GS, MS, (0.5, 0.995), min(T, 64), stats, (ddim, dpm), f"cofuse {(C, T, h, w)}")
    # end to end against the restatement fused through tests/codenoise_ref.py
    _assert_margin(eps2, GS, MS, "cofuse")
    ws = ops.cofuse_cfg_mimic_stats(zg, bg, rows, wg, GS, ops.mimic_factors(MS, 0.995, T * h * w))
    _same(ops.cofuse_cfg_mimic_ddim_step(zg, bg, rows, wg, GS, DDIM, ws), D.ddim_step(eps2, z, GS, MS, 0.995, DDIM), "cofuse end to end")


def _workspace_in_the_stated_order(ops, ws, eps2, order, rows, q, what):
    """`scal`, `partials`, `hist` and `maxbits` of a finished statistics pass against the host: the partial rows bit for bit
    (tests/stats_order_ref.py: `order(x, nx)` is the source's block map), and everything after them from those rows."""
    C, M = eps2.shape[1], eps2[0, 0].numel()
    v = ops.mimic_ws_views(ws, C)
    g, l = D.combines(eps2, GS, MS)
    want = np.stack([O.rows(np.stack([g[ch].double().numpy(), l[ch].double().numpy()], axis=1), order, rows) for ch in range(C)])
    assert O.same_bits(v["partials"][:, :rows].cpu().numpy(), want), f"{what}: partials"
    means = D.means_of(_kernel_sums({"partials": torch.from_numpy(want)}, C, rows), M)
    hist, maxbits = D.histogram(eps2, GS, MS, means)
    assert torch.equal(v["hist"].cpu().long(), hist), f"{what}: hist"
    assert torch.equal(v["maxbits"].cpu().long(), maxbits), f"{what}: maxbits"
    _same_scal(_u16(v["scal"]), D.select(eps2, GS, MS, q, means), f"{what}: scal")


@pytest.mark.parametrize("shape", [(1, 1, 1, 2052), (2, 3, 4, 5)], ids=str)
def test_workspace_bit_for_bit_in_the_stated_order(gpu, shape):
    ops, _ = _ops()
    eps2 = _case(shape)[0]
    M = shape[1] * shape[2] * shape[3]
    ws = ops.cfg_mimic_stats(eps2.to(gpu), GS, ops.mimic_factors(MS, 0.995, M))
    _workspace_in_the_stated_order(ops, ws, eps2, lambda x, k: O.direct_order(M, O.width(M), x, k), _rows(M), 0.995, str(shape))


def test_cofused_workspace_bit_for_bit_in_the_stated_order(gpu):
    """(C, T, HW) = (2, 3, 20), two windows that overlap in frame 1: a channel's T lines, block x the lines x, x + rows, ..."""
    ops, _ = _ops()
    C, T, h, w, table = 2, 3, 4, 5, [(0, 2), (1, 2)]
    wins, packed, rows, wn = _windows(C, T, h, w, table, 5)
    eps2 = CR.fuse(wins, table, wn, (1, C, T, h, w))
    z = torch.zeros(1, C, T, h, w, dtype=torch.float16, device=gpu)
    ws = ops.cofuse_cfg_mimic_stats(z, packed.to(gpu), rows, wn.to(gpu), GS, ops.mimic_factors(MS, 0.995, T * h * w))
    _workspace_in_the_stated_order(ops, ws, eps2, lambda x, k: O.line_order(T, h * w, O.width(h * w), x, k), min(T, 64), 0.995, "cofuse")


def test_thresholded_step_past_the_block_cap_equals_its_halves_and_runs_in_place(gpu):
    """C = 1, M = 1024 * 256 * 8 + 8 * 300 as two frames: a lane of the 1024-block grid takes a second trip.  The same entry on
    each frame alone, given the same workspace (the step reads the channel's scalars only), gives the same bits; then the
    DPM-Solver++ entry, second order, with `out` being `lat`."""
    ops, _ = _ops()
    M = 1024 * 256 * 8 + 8 * 300
    h = M // 2
    assert h % 8 == 0
    g = torch.Generator(device=gpu).manual_seed(13)
    noise = torch.randn(2, 1, 2, 1, h, generator=g, device=gpu).half()
    lat, prev = (torch.randn(1, 1, 2, 1, h, generator=g, device=gpu).half() for _ in range(2))
    ws = ops.cfg_mimic_stats(noise, GS, ops.mimic_factors(MS, 0.995, M)).clone()
    got = ops.cfg_mimic_ddim_step(noise, lat, GS, DDIM, ws)
    assert bool(torch.isfinite(got.float()).all())
    for t in (0, 1):
        half = ops.cfg_mimic_ddim_step(noise[:, :, t:t + 1].contiguous(), lat[:, :, t:t + 1].contiguous(), GS, DDIM, ws)
        assert torch.equal(got[:, :, t:t + 1], half)
    c = _dpm_coeffs(dpm_ref.scalars(dpm_ref.sigmas(10), 4, True))
    new, x0 = ops.cfg_mimic_dpm_step(noise, lat, GS, c, ws, x0_prev=prev)
    y = lat.clone()
    same, x0_again = ops.cfg_mimic_dpm_step(noise, y, GS, c, ws, x0_prev=prev, out=y)
    assert same is y and torch.equal(y, new) and torch.equal(x0_again, x0)


@pytest.mark.parametrize("shape", [(4, 3, 5, 7), (3, 2, 2, 6), (4, 4, 48, 48)], ids=str)
def test_one_window_is_the_flat_step(gpu, shape):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(31 + sum(shape))
    eps2, x = (torch.randn((k,) + shape, generator=g).half() for k in (2, 1))
    _assert_margin(eps2, GS, MS, str(shape))                        # the two forms add their rows in different orders
    e, xg, M = eps2.to(gpu), x.to(gpu), shape[1] * shape[2] * shape[3]
    fac = ops.mimic_factors(MS, 0.995, M)
    rows, wn = [(0, 0, shape[1])], torch.ones(1, shape[1], device=gpu)
    plain = ops.cfg_mimic_ddim_step(e, xg, GS, DDIM, ops.cfg_mimic_stats(e, GS, fac))
    keep = _u16(ops.mimic_ws_views(ops.cfg_mimic_stats(e, GS, fac), shape[0])["scal"]).copy()
    ws = ops.cofuse_cfg_mimic_stats(xg, e, rows, wn, GS, fac)
    assert np.array_equal(_u16(ops.mimic_ws_views(ws, shape[0])["scal"]), keep)
    _same(ops.cofuse_cfg_mimic_ddim_step(xg, e, rows, wn, GS, DDIM, ws), plain, "one window")


def test_bad_arguments_are_refused_before_a_launch(gpu):
    ops, VdxError = _ops()
    from vdx import _lib
    lib = _lib.load()
    shape = (4, 2, 2, 6)
    eps2, x = (torch.randn((k,) + shape, generator=torch.Generator().manual_seed(1)).half() for k in (2, 1))
    e, xg, M = eps2.to(gpu), x.to(gpu), 24
    ws = _ws_after(ops, gpu, eps2, GS, MS)
    out, stream = torch.empty_like(xg), torch.cuda.current_stream().cuda_stream
    pe, px, po, pw = e.data_ptr(), xg.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert lib.vdx_cfg_mimic_ws_bytes(0, 2, 12) == 0 and lib.vdx_cfg_mimic_ws_bytes(4, 1 << 16, 1 << 16) == 0
    assert lib.vdx_cfg_mimic_ws_bytes(4, 2, 12) == ws.numel() == lib.vdx_cofuse_cfg_mimic_ws_bytes(4, 2, 12)

    def stats(**kw):
        a = dict(eps2=pe, C=4, T=2, HW=12, gs=GS, ms=MS, k=M - 1, f=0.0, ws=pw, stages=7)
        a.update(kw)
        return lib.vdx_cfg_mimic_stats_f16(*a.values(), stream)
    assert stats() == 0
    for kw, word in ((dict(eps2=None), b"null"), (dict(ws=None), b"null"), (dict(ws=pw + 8), b"aligned"), (dict(ws=pe), b"overlaps"),
                     (dict(T=1 << 16, HW=1 << 16), b"2^32"), (dict(k=M), b"[0, M - 1]"), (dict(f=1.0), b"[0, 1)"),
                     (dict(f=-0.25), b"[0, 1)"), (dict(f=float("nan")), b"[0, 1)"), (dict(ms=0.0), b"finite and > 0"),
                     (dict(ms=-1.0), b"finite and > 0"), (dict(ms=float("inf")), b"finite and > 0"),
                     (dict(ms=float("nan")), b"finite and > 0"), (dict(stages=0), b"stages"), (dict(stages=8), b"stages")):
        assert stats(**kw) != 0, kw
        assert word in lib.vdx_last_error(), (kw, lib.vdx_last_error())
    tail = (GS, 0.9, 0.3, 0.4, 0.9, 4, 2, 12, stream)
    assert lib.vdx_cfg_mimic_ddim_step_f16(pe, px, po, pw, *tail) == 0
    for args in ((None, px, po, pw), (pe, None, po, pw), (pe, px, None, pw), (pe, px, po, None), (pe, px, po, pw + 8), (pe, px, pe, pw),
                 (pe, px, pw, pw), (pe, px, po, px), (pe, px, px + 16, pw)):
        assert lib.vdx_cfg_mimic_ddim_step_f16(*args, *tail) != 0, args
    assert lib.vdx_cfg_mimic_dpm_step_f16(pe, px, None, None, po, pw, GS, 1, 1, 1, 1, 0, 0, 4, 2, 12, stream) != 0
    assert lib.vdx_cfg_mimic_dpm_step_f16(pe, px, None, po, po, pw, GS, 1, 1, 1, 1, 0, 0, 4, 2, 12, stream) != 0
    prev = torch.zeros_like(xg)                           # the history may be neither its predecessor nor the latent
    assert lib.vdx_cfg_mimic_dpm_step_f16(pe, px, prev.data_ptr(), prev.data_ptr(), po, pw, GS, 1, 1, 1, 1, 0, 0, 4, 2, 12, stream) != 0
    assert lib.vdx_cfg_mimic_dpm_step_f16(pe, px, prev.data_ptr(), px, po, pw, GS, 1, 1, 1, 1, 0, 0, 4, 2, 12, stream) != 0
    with pytest.raises(VdxError, match="bytes"):
        ops.cfg_mimic_ddim_step(e, xg, GS, DDIM, ws[:64])
    with pytest.raises(VdxError):
        ops.cfg_mimic_stats(e.reshape(2, -1), GS, (MS, 0, 0.0))
    with pytest.raises(VdxError):
        ops.cfg_mimic_stats(e, GS, (MS, M, 0.0))
    T = shape[1]
    with pytest.raises(VdxError, match="64"):
        ops.cofuse_cfg_mimic_stats(xg, e, [(0, 0, T)] * 65, torch.ones(65, T, device=gpu), GS, (MS, 0, 0.0))
    with pytest.raises(VdxError):
        ops.cofuse_cfg_mimic_stats(xg, e, [(0, 0, T)], torch.ones(1, T, device=gpu), GS, (-1.0, 0, 0.0))
    torch.cuda.synchronize()


# ---- the job on the tiny golden UNet ------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 8, 32, 32, 3                                     # 8 frames, chunk 6, overlap 2: windows (0, 6), (4, 8)
RANGES = [(0, 6), (4, 8)]
JOB = dict(guidance_scale=15.0, cfg_mimic=7.0, cfg_mimic_percentile=0.995)


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    return build(gpu, 0, 1)


def _diffuser(model, sampler="ddim", **kw):
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    kw = {**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx", device="cuda",
                 noise_device="cpu", scheduler=sampler), **kw}
    return DistributedVideoDiffuser(DiffuserConfig(**kw), m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1])


def _loop(d, model, co):
    """The job of the diffuser `d` (one rank) written out: the product's UNet on the GPU, and for every scheduler step the
    product's statistics and step ops called by hand on that sample -> the final fp32 latent on the CPU.  The kernels themselves
    are pinned against the restatement above; this pins the job's plumbing: which sample the statistics are taken over."""
    from vdx import ops
    from vdx.codenoise import window_table
    from vdx.pipeline import seeded_noise
    unet, emb = model
    emb2 = torch.cat([emb[1:], emb[:1]], dim=0)
    cfg, sched, ts = d.cfg, d.scheduler, list(d.schedule)
    gs, ms, q, dpm = cfg.guidance_scale, cfg.cfg_mimic, cfg.cfg_mimic_percentile, cfg.scheduler == "dpmpp_2m"
    start = seeded_noise(d.latent_shape, 1.0, cfg.device, cfg.noise_device)
    cp, sig = d.plan(), dpm_ref.sigmas(cfg.steps)

    def step(eps2, x, prev, i):
        eps2, x = eps2.contiguous(), x.contiguous()
        ws = ops.cfg_mimic_stats(eps2, gs, ops.mimic_factors(ms, q, x[0, 0].numel()))
        if not dpm:
            return ops.cfg_mimic_ddim_step(eps2, x, gs, sched.coefficients(ts[i]), ws), None
        second = prev is not None and i != cfg.steps - 1
        return ops.cfg_mimic_dpm_step(eps2, x, gs, _dpm_coeffs(dpm_ref.scalars(sig, i, second)), ws, x0_prev=prev if second else None)

    if co:
        table = [(s, e - s) for s, e in cp.ranges]
        wn = window_table(cp, T).wn
        z, prev = start.clone(), None
        for i, t in enumerate(ts):
            wins = [unet(ops.cfg_input(z[:, :, s:e].contiguous(), d.ctx, cfg.context_weight), t, encoder_hidden_states=emb2).sample.cpu()
                    for s, e in cp.ranges]
            z, prev = step(CR.fuse(wins, table, wn.cpu(), z.shape).to(z.device), z, prev, i)
        return z.float().cpu()
    chunks = []
    for s, e in cp.for_rank(0):
        lat, prev = start[:, :, s:e].clone(), None
        for i, t in enumerate(ts):
            noise = unet(ops.cfg_input(lat, d.ctx, cfg.context_weight), t, encoder_hidden_states=emb2).sample
            lat, prev = step(noise, lat, prev, i)
        chunks.append((s, e, lat))
    return d.blend(chunks, start, cp.overlap).cpu()


@pytest.mark.parametrize("co", [False, True], ids=["windowed", "co_denoise"])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_thresholded_job_is_the_loop(gpu, model, sampler, co):
    d = _diffuser(model, sampler, co_denoise=co, **JOB)
    lat, info = d()
    assert info["ranges"] == RANGES and info["steps_run"] == STEPS and info["cfg_mimic"] == {"scale": 7.0, "percentile": 0.995}
    _same(lat, _loop(d, model, co), f"{sampler} co={co}")
    plain, info0 = _diffuser(model, sampler, co_denoise=co, guidance_scale=15.0)()
    assert "cfg_mimic" not in info0 and not torch.equal(plain, lat)


def test_defaults_are_untouched(gpu, model, monkeypatch):
    """cfg_mimic None is the config that does not name it: the same latent and `info` keys, and the scheduler's `step_cfg` is
    called with the four arguments it always was (no keyword, so never the new branch)."""
    from vdx.scheduler import DDIMScheduler
    calls = []
    real = DDIMScheduler.step_cfg

    def counting(self, *a, **kw):
        calls.append((len(a), dict(kw)))
        return real(self, *a, **kw)
    monkeypatch.setattr(DDIMScheduler, "step_cfg", counting)
    named, info1 = _diffuser(model, cfg_mimic=None, cfg_mimic_percentile=1.0)()
    n_named, calls[:] = len(calls), []
    bare, info0 = _diffuser(model)()
    assert len(calls) == n_named == STEPS * len(RANGES) and all(c == (4, {}) for c in calls)
    _same(named, bare, "defaults")
    assert set(info1) == set(info0) and "cfg_mimic" not in info0
    calls[:] = []
    _diffuser(model, **JOB)()
    assert all(c == (4, {"cfg_mimic": 7.0, "cfg_mimic_percentile": 0.995}) for c in calls) and len(calls) == STEPS * len(RANGES)
