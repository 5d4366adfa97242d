"""-m gpu: spatially tiled co-denoising (csrc/cotile.hip, vdx/codenoise.py `tile_plan`).  The kernels bit for bit against the
torch-CPU restatement of tests/cotile_ref.py (every operation is a correctly rounded fp32 operation in a stated order, so equality
is derived, not measured), the one-tile identities against the temporal kernels, an exactness property of the whole job with dyadic
weights, and the tiled job on the tiny golden UNet against a Python loop written here, from run to run, from one rank to two, and
through `run_job`.

The shapes of the kernel test are the issue's.  By the kernel's own alignment rule (W, tw and every x0 multiples of 8) `12x20`
with tile `8x8`, overlap 3 has x0 = (0, 5, 10, 12) and takes the element-wise path, and `8x12` with tile `8x4` takes the 8-byte one;
`8x32` with tile `8x16`, overlap 8 is added here for the 16-byte path, and `2x264` with tile `2x133` for a row of two segments."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cotile_ref as RT
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


def _wn(ranges, T, ov):
    from vdx.codenoise import window_table
    from vdx.planner import ChunkPlan
    return window_table(ChunkPlan(max(e - s for s, e in ranges), ov, tuple(ranges), 1), T).wn


RANGES, T_OV = [(0, 4), (2, 5)], 2                                 # two windows of 4 and 3 frames: the second leaves a slot's tail


def _case(C, T, H, W, tile, ov, seed, ranges=RANGES, plant=False):
    """-> z, prev (1,C,T,H,W); the windows' outputs [kt][ky][kx] (2,C,L,th,tw); the packed buffer [Kt][ny nx][slot] (every element
    outside a window's block is NaN: the tail of a short window's slot); rows [(offset, s, L)]; wn; the TilePlan."""
    from vdx.codenoise import tile_plan
    (th, tw), (oy, ox) = tile, ov
    tp = tile_plan(H, W, th, tw, oy, ox)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(1, C, T, H, W, generator=g).half()
    prev = torch.randn(1, C, T, H, W, generator=g).half()
    wins = [[[torch.randn(2, C, e - s, th, tw, generator=g).half() for _ in tp.xs] for _ in tp.ys] for s, e in ranges]
    if plant:                                                      # in ONE window, the first: a NaN in u, an infinity in c
        wins[0][0][0][0, 0, 0, 0, 0] = NAN
        wins[0][0][0][1, C - 1, -1, th - 1, tw - 1] = float("inf")
    slot = 2 * C * max(e - s for s, e in ranges) * th * tw
    packed = torch.full((len(ranges), tp.count, slot), NAN, dtype=torch.float16)
    rows = []
    for kt, (s, e) in enumerate(ranges):
        rows.append((kt * tp.count * slot, s, e - s))
        for ky in range(len(tp.ys)):
            for kx in range(len(tp.xs)):
                w = wins[kt][ky][kx]
                packed[kt, ky * len(tp.xs) + kx, :w.numel()] = w.reshape(-1)
    return z, prev, wins, packed.reshape(-1), rows, _wn(ranges, T, T_OV), tp, slot


def _ref_args(rows, wn, tp):
    return dict(table=[(s, L) for _, s, L in rows], wn=wn, ys=tp.ys, xs=tp.xs, th=tp.th, tw=tp.tw, wyn=tp.wyn, wxn=tp.wxn)


def _check_case(gpu, case, what):
    ops, _ = _ops()
    z, prev, wins, packed, rows, wn, tp, slot = case
    grid = tp.grid(slot, gpu)
    zg, pg, bg, wg = z.to(gpu), prev.to(gpu), packed.to(gpu), wn.to(gpu)
    ref = _ref_args(rows, wn, tp)
    for i, coeffs in enumerate(_ddim_coeffs()[::4]):
        want = RT.cotile_ddim(z, wins, gs=GS, coeffs=coeffs, **ref)
        _same_bits(ops.cotile_cfg_ddim_step(zg, bg, rows, wg, grid, GS, coeffs), want, f"{what} ddim {i}")
        x = zg.clone()
        assert ops.cotile_cfg_ddim_step(x, bg, rows, wg, grid, GS, coeffs, out=x) is x
        _same_bits(x, want, f"{what} ddim {i} out=z")
    sig = dpm_ref.sigmas(6)
    for i, second in ((0, False), (2, True), (5, False)):          # first order, second order, the last step (sigma 0)
        k = dpm_ref.scalars(sig, i, second)
        want, want_x0 = RT.cotile_dpm(z, wins, gs=GS, k=k, x0_prev=prev if second else None, **ref)
        got, got_x0 = ops.cotile_cfg_dpm_step(zg, bg, rows, wg, grid, GS, _coeffs(k), x0_prev=pg if second else None)
        _same_bits(got_x0, want_x0, f"{what} dpm step {i} x0")
        _same_bits(got, want, f"{what} dpm step {i} lat'")
        x = zg.clone()
        got, got_x0 = ops.cotile_cfg_dpm_step(x, bg, rows, wg, grid, GS, _coeffs(k), x0_prev=pg if second else None, out=x)
        assert got is x
        _same_bits(x, want, f"{what} dpm step {i} out=z")
        _same_bits(got_x0, want_x0, f"{what} dpm step {i} x0, out=z")


CASES = {
    "12x20 tile 8x8 overlap 3": dict(C=4, T=5, H=12, W=20, tile=(8, 8), ov=(3, 3)),           # moved last tiles; x0 = 5: element-wise
    "9x14 tile 6x6 overlap 2": dict(C=4, T=5, H=9, W=14, tile=(6, 6), ov=(2, 2)),             # element-wise
    "8x12 tile 8x4 overlap 0": dict(C=4, T=5, H=8, W=12, tile=(8, 4), ov=(0, 0)),             # one row band; 8-byte
    "8x32 tile 8x16 overlap 8": dict(C=4, T=5, H=8, W=32, tile=(8, 16), ov=(0, 8)),           # x0 = 0, 8, 16: 16-byte
    "2x264 tile 2x133 overlap 2": dict(C=1, T=5, H=2, W=264, tile=(2, 133), ov=(0, 2)),       # 264 > 256 lanes: two segments per row
}


@pytest.mark.parametrize("name", list(CASES))
def test_fused_steps_match_the_restatement(gpu, name):
    _check_case(gpu, _case(seed=3, **CASES[name]), name)


@pytest.mark.parametrize("name", list(CASES)[:4])
def test_nan_and_inf_stay_in_their_element(gpu, name):
    ops, _ = _ops()
    case = _case(seed=5, plant=True, **CASES[name])
    _check_case(gpu, case, name + " planted")
    clean = _case(seed=5, **CASES[name])
    k = _coeffs(dpm_ref.scalars(dpm_ref.sigmas(6), 2, True))
    outs = []
    for z, prev, _, packed, rows, wn, tp, slot in (clean, case):
        got, x0 = ops.cotile_cfg_dpm_step(z.to(gpu), packed.to(gpu), rows, wn.to(gpu), tp.grid(slot, gpu), GS, k, x0_prev=prev.to(gpu))
        outs.append((got.cpu().view(torch.int16), x0.cpu().view(torch.int16)))
    for a, b in zip(*outs):
        assert 1 <= int((a != b).sum()) <= 2                       # the two planted cells, and no other


def test_slot_tails_full_of_nan_are_never_read(gpu):
    ops, _ = _ops()
    z, prev, wins, packed, rows, wn, tp, slot = _case(seed=7, **CASES["12x20 tile 8x8 overlap 3"])
    assert int(torch.isnan(packed).sum()) > 0
    got = ops.cotile_cfg_ddim_step(z.to(gpu), packed.to(gpu), rows, wn.to(gpu), tp.grid(slot, gpu), GS, _ddim_coeffs()[3])
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("shape", [(1, 4, 5, 3, 5), (1, 4, 5, 8, 16), (1, 2, 5, 6, 12)], ids=lambda s: "x".join(map(str, s)))
def test_one_spatial_tile_has_the_bits_of_the_temporal_kernels(gpu, shape):
    ops, _ = _ops()
    _, C, T, H, W = shape
    g = torch.Generator().manual_seed(11)
    z, prev = (torch.randn(shape, generator=g).half().to(gpu) for _ in range(2))
    wins = [torch.randn(2, C, e - s, H, W, generator=g).half() for s, e in RANGES]
    wins[0].view(-1)[:6] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, NAN], dtype=torch.float16)
    slot = wins[0].numel()
    packed = torch.zeros(2, slot, dtype=torch.float16)
    for k, w in enumerate(wins):
        packed[k, :w.numel()] = w.reshape(-1)
    packed, wn = packed.reshape(-1).to(gpu), _wn(RANGES, T, T_OV).to(gpu)
    rows = [(k * slot, s, e - s) for k, (s, e) in enumerate(RANGES)]
    grid = ops.TileGrid(slot, (0,), (0,), H, W, torch.ones(1, H, device=gpu), torch.ones(1, W, device=gpu))
    for coeffs in _ddim_coeffs()[::3]:
        assert torch.equal(ops.cotile_cfg_ddim_step(z, packed, rows, wn, grid, GS, coeffs).view(torch.int16),
                           ops.cofuse_cfg_ddim_step(z, packed, rows, wn, GS, coeffs).view(torch.int16))
    sig = dpm_ref.sigmas(6)
    for i, second in ((0, False), (2, True), (5, False)):
        c = _coeffs(dpm_ref.scalars(sig, i, second))
        got, got_x0 = ops.cotile_cfg_dpm_step(z, packed, rows, wn, grid, GS, c, x0_prev=prev if second else None)
        want, want_x0 = ops.cofuse_cfg_dpm_step(z, packed, rows, wn, GS, c, x0_prev=prev if second else None)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and torch.equal(got_x0.view(torch.int16), want_x0.view(torch.int16))


@pytest.mark.parametrize("shape,s,e,box", [((1, 4, 7, 12, 20), 2, 6, (4, 8, 5, 8)), ((1, 4, 7, 12, 20), 0, 7, (0, 12, 0, 20)),
                                           ((1, 4, 5, 8, 32), 4, 5, (0, 8, 16, 16)), ((1, 2, 5, 9, 12), 1, 4, (3, 6, 8, 4)),
                                           ((1, 1, 3, 40, 64), 1, 3, (39, 1, 63, 1))])
def test_cfg_input_tile_is_slice_plus_cfg_input(gpu, shape, s, e, box):
    ops, _ = _ops()
    y0, th, x0, tw = box
    g = torch.Generator().manual_seed(19)
    z = torch.randn(shape, generator=g).half()
    z.view(-1)[:4] = torch.tensor([65504.0, -0.0, 2.0 ** -24, float("inf")], dtype=torch.float16)
    ctx = torch.randn((1, shape[1], 1) + shape[3:], generator=g).half()
    zg, cg = z.to(gpu), ctx.to(gpu)
    for c, cw in ((None, 0.0), (cg, 0.35)):
        got = ops.cfg_input_tile(zg, c, cw, s, e, *box)
        crop = None if c is None else c[:, :, :, y0:y0 + th, x0:x0 + tw].clone(memory_format=torch.contiguous_format)   # a copy: aligned
        want = ops.cfg_input(zg[:, :, s:e, y0:y0 + th, x0:x0 + tw].clone(memory_format=torch.contiguous_format), crop, cw)
        assert got.is_contiguous() and tuple(got.shape) == (2, shape[1], e - s, th, tw)
        assert ops.is_cfg_duplicate(got)                                            # the shared prefix still applies
        _same_bits(got, want, "against slice + cfg_input")
        _same_bits(got, RT.cfg_input_tile(z, None if c is None else ctx, cw, s, e, *box), "against the restatement")
        got.add_(1)
        assert not ops.is_cfg_duplicate(got)                                        # a write drops the tag, as for cfg_input


def test_bad_grids_are_refused_before_a_launch(gpu):
    ops, VdxError = _ops()
    z, prev, wins, packed, rows, wn, tp, slot = _case(seed=17, **CASES["8x12 tile 8x4 overlap 0"])
    zg, bg, wg = z.to(gpu), packed.to(gpu), wn.to(gpu)
    coeffs, grid = _ddim_coeffs()[0], tp.grid(slot, gpu)
    ops.cotile_cfg_ddim_step(zg, bg, rows, wg, grid, GS, coeffs)
    bad = {"a column band past W": grid._replace(xs=(0, 4, 9)), "a negative row": grid._replace(ys=(-1,)),
           "column 4..7 uncovered": grid._replace(xs=(0, 0, 8)), "tiles overlap in the buffer": grid._replace(stride=slot - 8),
           "the last tile leaves the buffer": grid._replace(stride=slot * 2), "a tile wider than the frame": grid._replace(tw=16),
           "weights of another shape": grid._replace(wxn=grid.wxn[:, :-1].contiguous())}
    for what, gr in bad.items():
        with pytest.raises(VdxError):
            ops.cotile_cfg_ddim_step(zg, bg, rows, wg, gr, GS, coeffs)
        with pytest.raises(VdxError):
            ops.cotile_cfg_dpm_step(zg, bg, rows, wg, gr, GS, _coeffs(dpm_ref.scalars(dpm_ref.sigmas(6), 0, False)))
    many = grid._replace(ys=(0,) * 13, xs=(0, 1, 2, 3, 8), wyn=torch.ones(13, 8, device=gpu), wxn=torch.ones(5, 12, device=gpu))
    with pytest.raises(VdxError, match="64"):
        ops.cotile_cfg_ddim_step(zg, bg, rows, wg, many, GS, coeffs)                # 65 tiles: by the wrapper
    import ctypes
    lib = ops._lib.load()                                           # and by the library itself
    T, H, W = z.shape[2:]
    off = (ctypes.c_int64 * 2)(*(r[0] for r in rows))
    st, ln = (ctypes.c_int32 * 2)(*(r[1] for r in rows)), (ctypes.c_int32 * 2)(*(r[2] for r in rows))
    ys, xs = (ctypes.c_int32 * 13)(), (ctypes.c_int32 * 5)(0, 1, 2, 3, 8)
    out = torch.empty_like(zg)
    rc = lib.vdx_cotile_cfg_ddim_step_f16(zg.data_ptr(), bg.data_ptr(), bg.numel(), off, st, ln, 2, wg.data_ptr(), 0, ys, 13,
                                          many.wyn.data_ptr(), xs, 5, many.wxn.data_ptr(), 8, 4, out.data_ptr(), GS, *coeffs,
                                          z.shape[1], T, H, W, None)
    assert rc != 0 and b"64" in lib.vdx_last_error()
    ops.cfg_input_tile(zg, None, 0.0, 0, 5, 0, 8, 8, 4)
    for args in ((3, 3, 0, 8, 0, 4), (0, 6, 0, 8, 0, 4), (0, 5, 1, 8, 0, 4), (0, 5, 0, 8, 9, 4), (0, 5, 0, 9, 0, 4), (0, 5, 0, 8, -1, 4),
                 (0, 5, 0, 0, 0, 4)):                               # (s, e, y0, th, x0, tw) of an 8 x 12 frame of 5
        with pytest.raises(VdxError):
            ops.cfg_input_tile(zg, None, 0.0, *args)
    torch.cuda.synchronize()


# ---- an exactness property of the whole job: dyadic weights, a "UNet" that crops one fixed field -----------------------------
class _CropField:
    """Stands in for the UNet: whatever it is given, it returns the crop of ONE fixed fp16 field (2,C,T,H,W) that the input was
    cropped from; the box comes from the `ops.cfg_input_*` call that built the input (patched below)."""

    def __init__(self, field):
        self.field, self.box = field, None
        self.config = SimpleNamespace(in_channels=field.shape[1])

    def __call__(self, x, t, encoder_hidden_states=None):
        s, e, y0, th, x0, tw = self.box
        out = self.field[:, :, s:e, y0:y0 + th, x0:x0 + tw].contiguous()
        assert out.shape == x.shape
        return SimpleNamespace(sample=out)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_tiled_job_equals_the_untiled_one_when_the_weights_are_dyadic(gpu, monkeypatch, sampler):
    """Latent 13 x 18, tiles 8 x 8 with overlap 3 on both axes: 13 = 8 + 5 and 18 = 8 + 2 * 5, so no tile is moved, overlap + 1 = 4
    is a power of two and the normalised spatial weights are k/4; 7 frames in windows of 4 with overlap 1 give time weights 1/2 and
    1.  Every window returns the same value for a cell, every product w * u and every partial sum is then exact in fp32 and the
    sum is u itself, tiled or not: the two jobs' latents are equal, with no tolerance.  (The issue suggests 14 x 20, at which the
    last tile of either axis IS moved; 13 x 18 is the nearest size that meets its own premise.)"""
    ops, _ = _ops()
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    C, T, H, W = 4, 7, 13, 18
    field = torch.randn(2, C, T, H, W, generator=torch.Generator().manual_seed(29)).half().to(gpu)
    stub = _CropField(field)
    real_tile, real_window = ops.cfg_input_tile, ops.cfg_input_window

    def tile(z, ctx, weight, s, e, y0, th, x0, tw, out=None):
        stub.box = (s, e, y0, th, x0, tw)
        return real_tile(z, ctx, weight, s, e, y0, th, x0, tw, out=out)

    def window(z, ctx, weight, s, e, out=None):
        stub.box = (s, e, 0, H, 0, W)
        return real_window(z, ctx, weight, s, e, out=out)
    monkeypatch.setattr(ops, "cfg_input_tile", tile)
    monkeypatch.setattr(ops, "cfg_input_window", window)
    emb = torch.zeros(1, 77, 64, dtype=torch.float16, device=gpu)
    lats = []
    for kw in (dict(), dict(tile=(64, 64), tile_overlap=(24, 24))):
        cfg = DiffuserConfig(num_frames=T, steps=3, chunk_size=4, overlap=1, height=H * 8, width=W * 8, mode="chunk", device="cuda",
                             noise_device="cpu", co_denoise=True, scheduler=sampler, **kw)
        d = DistributedVideoDiffuser(cfg, stub, make_scheduler(sampler, DDIMScheduler()), emb, emb)
        lat, info = d()
        assert info["ranges"] == [(0, 4), (3, 7), (6, 7)]
        lats.append(lat)
    assert info["tile"] == {"tile": [8, 8], "overlap": [3, 3], "grid": [2, 3], "windows": 18}
    assert bool(torch.isfinite(lats[0]).all()) and torch.equal(lats[0].view(torch.int32), lats[1].view(torch.int32))


# ---- the job on the tiny golden UNet ------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 6, 16, 24, 2
TILE = (64, 128)                                                    # 8 x 16 latent cells, default overlap (2, 4): rows 0, 6, 8 x columns 0, 8
J_RANGES = [(0, 4), (2, 6), (4, 6)]                                 # plan(6, 1, 4, 2)
INFO_KEYS = {"chunk_size", "overlap", "ranges", "world_size", "num_frames", "denoise_s", "exchange", "steps_run",
             "emu_gather_delay_s", "net_gather_s", "network_bytes", "payload_bytes", "payload_bytes_actual"}


def _config(**kw):
    from vdx.pipeline import DiffuserConfig
    kw = {**dict(num_frames=T, steps=STEPS, chunk_size=4, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                 device="cuda", noise_device="cpu", co_denoise=True, tile=TILE), **kw}
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
    return DistributedVideoDiffuser(_config(scheduler=sampler, **kw), m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1])


def _loop(d, model, start, sampler, ranges, ov):
    """The tiled round, written out with the ops pinned above: per step every (window, tile)'s UNet output from
    `ops.cfg_input_tile` into a packed buffer, then ONE `ops.cotile_cfg_*_step`.  -> fp16 latent."""
    from vdx import ops
    from vdx.codenoise import tile_plan
    m, emb = model
    emb2 = torch.cat([emb[1:], emb[:1]], dim=0)
    _, C, n_frames, H, W = start.shape
    tp = tile_plan(H, W, 8, 16, 2, 4)
    assert (tp.ys, tp.xs) == ((0, 6, 8), (0, 8))
    slot = 2 * C * max(e - s for s, e in ranges) * tp.th * tp.tw
    rows = [(k * tp.count * slot, s, e - s) for k, (s, e) in enumerate(ranges)]
    wn, grid = _wn(ranges, n_frames, ov).to(start.device), tp.grid(slot, start.device)
    packed = torch.zeros(len(ranges), tp.count, slot, dtype=torch.float16, device=start.device)
    z, x0_prev, n = start.clone(), None, d.cfg.steps
    for i, t in enumerate(d.schedule):
        for k, (s, e) in enumerate(ranges):
            for j, box in enumerate(tp.boxes):
                noise = m(ops.cfg_input_tile(z, d.ctx, d.cfg.context_weight, s, e, *box), t, encoder_hidden_states=emb2).sample
                packed[k, j, :noise.numel()] = noise.reshape(-1)
        if sampler == "ddim":
            z = ops.cotile_cfg_ddim_step(z, packed.view(-1), rows, wn, grid, d.cfg.guidance_scale, d.scheduler.coefficients(t))
        else:
            second = x0_prev is not None and i != n - 1
            k = dpm_ref.scalars(dpm_ref.sigmas(n), i, second)
            z, x0_prev = ops.cotile_cfg_dpm_step(z, packed.view(-1), rows, wn, grid, d.cfg.guidance_scale, _coeffs(k),
                                                 x0_prev=x0_prev if second else None)
    return z


def _base(d):
    from vdx.pipeline import seeded_noise
    return seeded_noise(d.latent_shape, d.scheduler.init_noise_sigma, "cuda", "cpu")


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_tiled_job_is_the_loop_and_the_same_on_every_run(model, sampler):
    d = _diffuser(model, sampler)
    lat, info = d()
    assert info["ranges"] == J_RANGES and lat.dtype == torch.float32 and tuple(lat.shape) == (1, 4, T, HL, WL)
    want = _loop(d, model, _base(d), sampler, J_RANGES, 2)
    assert bool(torch.isfinite(lat).all()) and torch.equal(lat, want.float())
    again, _ = d()
    assert torch.equal(again, lat)                                  # run to run
    assert set(info) == INFO_KEYS | {"co_denoise", "tile"}
    assert info["tile"] == {"tile": [8, 16], "overlap": [2, 4], "grid": [3, 2], "windows": 18}
    rec = info["co_denoise"]
    assert (rec["windows"], rec["steps"], rec["bytes_per_step"]) == (3, STEPS, 0)
    assert info["payload_bytes"] == STEPS * sum((e - s) * 4 * 2 for s, e in J_RANGES)
    assert info["payload_bytes_actual"] == STEPS * sum(6 * 2 * 4 * (e - s) * 8 * 16 * 2 for s, e in J_RANGES)


def test_a_tile_equal_to_the_frame_is_plain_co_denoising(model):
    tiled, info = _diffuser(model, tile=(HL * 8, WL * 8))()
    plain, info0 = _diffuser(model, tile=None)()
    assert torch.equal(tiled, plain)
    assert info["tile"]["grid"] == [1, 1] and "tile" not in info0 and set(info0) == INFO_KEYS | {"co_denoise"}
    assert set(info0["co_denoise"]) == {"windows", "steps", "exchange_s", "bytes_per_step"}


def test_two_ranks_end_with_the_bits_of_one(gpu, model, tmp_path):
    """Two fresh processes, one rank each, both on this box's one GPU and talking over gloo (tests/test_codenoise_gpu.py's
    arrangement), on a plan that is the same for one rank and for two: 8 frames, chunk 6, overlap 2."""
    from vdx.planner import plan
    assert plan(8, 1, 6, 2).ranges == plan(8, 2, 6, 2).ranges == ((0, 6), (4, 8))
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29748",
                        os.path.join(ROOT, "tests", "dist_cotile_worker.py"), str(out), "8", "6", "2", "2", "dpmpp_2m"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
    got = torch.load(out, weights_only=True)
    d = _diffuser(model, "dpmpp_2m", num_frames=8, steps=2, chunk_size=6)
    lat, info = d()
    assert torch.equal(got["lat"], lat.cpu())
    gi = got["info"]
    assert [tuple(x) for x in gi["ranges"]] == [(0, 6), (4, 8)] and gi["world_size"] == 2
    per_step = 1 * 1 * 6 * (2 * 4 * 6 * 8 * 16) * 2                 # (world-1) x per_rank x tiles x slot halves x 2 bytes
    assert gi["co_denoise"]["bytes_per_step"] == per_step and gi["network_bytes"] == 2 * per_step
    assert gi["tile"] == info["tile"] == {"tile": [8, 16], "overlap": [2, 4], "grid": [3, 2], "windows": 12}


# ---- run_job end to end on synthetic weights ---------------------------------------------------------------------------------
def test_run_job_end_to_end(gpu, tmp_path):
    """128 x 128, 4 frames, 64 x 64 tiles (8 x 8 latent cells, rows and columns 0, 6, 8): text-to-video, then masked
    video-to-video keeping frames 0 and 1: the record carries "tile", the frames have the full size, and the kept frames are the
    input's bytes."""
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import build_arg_parser, config_from_args, run_job
    F, H, W = 4, 128, 128
    clip = torch.randint(0, 256, (F, H, W, 3), generator=torch.Generator().manual_seed(37), dtype=torch.uint8).numpy()
    np.save(tmp_path / "clip.npy", clip)
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    base = ["--model_id", "synthetic:tiny", "--num_frames", "4", "--steps", "2", "--height", "128", "--width", "128", "--chunk_size", "4",
            "--overlap", "2", "--noise_device", "cpu", "--co_denoise"]

    def job(extra):
        got = {}
        res = run_job(config_from_args(build_arg_parser().parse_args(base + extra)), out_video=None, pipe=pipe, clip_inputs=got)
        return res, np.stack(got["frames"])
    res0, plain = job([])
    res1, tiled = job(["--tile", "64", "64"])
    res2, kept = job(["--tile", "64", "64", "--init_video", str(tmp_path / "clip.npy"), "--strength", "0.5", "--keep_frames", "0:2"])
    want = {"tile": [8, 8], "overlap": [2, 2], "grid": [3, 3], "windows": 9 * res0["co_denoise"]["windows"]}
    assert "tile" not in res0 and res1["tile"] == res2["tile"] == want and set(res1) == set(res0) | {"tile"}
    assert res1["co_denoise"]["windows"] == res0["co_denoise"]["windows"]
    for fr in (plain, tiled, kept):
        assert fr.shape == (F, H, W, 3) and fr.dtype == np.uint8
    assert not np.array_equal(tiled, plain)
    assert np.array_equal(kept[:2], clip[:2]) and not np.array_equal(kept[2:], clip[2:])
    assert res2["mask"]["kept_frames"] == 2
