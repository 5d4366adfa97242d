"""-m gpu: masked video-to-video (csrc/inpaint.hip, vdx/inpaint.py).  Every comparison is bit for bit: the definition is a select
around chains that are already pinned (tests/inpaint_ref.py restates it), so no tolerance is needed.  The four kernels against
the restatement; the masked job on the tiny golden UNet against a Python loop over the planner's windows, from run to run and
from one rank to two; `run_job` end to end on synthetic weights.

Where `known` is COMPUTED from a planted NaN the NaN's payload is not part of the statement (`_same_bits`, as in
tests/test_codenoise_gpu.py); wherever bits are only moved (regenerated cells, `last`, the paste) every bit is compared."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inpaint_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
SA, S1 = 0.83984375, 0.54296875                                     # fp16 values, as `add_noise` hands them over


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    return ops, VdxError


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(got, want, what):
    """Every bit equal (signed zeros too); NaNs in the same places."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
    g, w = _bits(got)[~nan], _bits(want)[~nan]
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {got.numel()} values differ"


def _masks(T, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx, tt = torch.arange(h)[None, :, None], torch.arange(w)[None, None, :], torch.arange(T)[:, None, None]
    return {"random": (torch.rand(T, h, w, generator=g) < 0.5).to(torch.uint8),
            "checkerboard": ((yy + xx + tt) % 2).to(torch.uint8).contiguous(),
            "per-frame": (tt % 2).expand(T, h, w).to(torch.uint8).contiguous()}


def _clip(C, T, h, w, L, seed, plant=False):
    g = torch.Generator().manual_seed(seed)
    x0, base = (torch.randn(1, C, T, h, w, generator=g).half() for _ in range(2))
    z = torch.randn(1, C, L, h, w, generator=g).half()
    if plant:
        vals = torch.tensor([NAN, INF, -INF, 0.0, -0.0, 65504.0, -65504.0], dtype=torch.float16)
        for t in (z, x0, base):
            idx = torch.randperm(t.numel(), generator=g)[:4 * len(vals)]
            t.view(-1)[idx] = vals.repeat(4)[:idx.numel()]
    return z, x0, base


# (C, T_clip, h, w; s, L)
SHAPES = [(4, 1, 1, 1, 0, 1), (4, 7, 3, 5, 2, 3), (3, 5, 2, 6, 4, 1), (4, 9, 8, 16, 0, 9), (4, 9, 8, 16, 8, 1), (1, 2, 48, 48, 1, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_renoise_matches_the_restatement(gpu, shape):
    ops, _ = _ops()
    C, T, h, w, s, L = shape
    z, x0, base = _clip(C, T, h, w, L, seed=3)
    xg, bg = x0.to(gpu), base.to(gpu)
    for kind, m in _masks(T, h, w, 5).items():
        mg = m.to(gpu)
        for last in (False, True):
            want = R.renoise_ref(z, x0, base, m, SA, S1, last, s)
            zg = z.to(gpu)
            got = ops.mask_renoise(zg, xg, bg, mg, SA, S1, last, s)
            assert got is zg                                                           # in place
            assert torch.equal(_bits(got), _bits(want)), f"{kind} last={last}"
            again = ops.mask_renoise(z.to(gpu), xg, bg, mg, SA, S1, last, s)           # run to run
            assert torch.equal(_bits(again), _bits(got))
            twice = ops.mask_renoise(got.clone(), xg, bg, mg, SA, S1, last, s)         # the select applied twice is itself
            assert torch.equal(_bits(twice), _bits(got))


@pytest.mark.parametrize("shape", [(4, 7, 3, 5, 2, 3), (3, 5, 2, 6, 1, 3), (4, 9, 8, 16, 0, 9)], ids=lambda s: "x".join(map(str, s)))
def test_nan_inf_zeros_and_the_largest_values_stay_in_their_element(gpu, shape):
    ops, _ = _ops()
    C, T, h, w, s, L = shape
    z, x0, base = _clip(C, T, h, w, L, seed=7, plant=True)
    assert int(torch.isnan(z).sum()) and int(torch.isinf(x0).sum()) and int((_bits(base) == -32768).sum())    # -0.0 is there
    xg, bg = x0.to(gpu), base.to(gpu)
    for kind, m in _masks(T, h, w, 9).items():
        mm = m[s:s + L].bool()[None, None].expand(1, C, L, h, w)
        for last in (False, True):
            got = ops.mask_renoise(z.to(gpu), xg, bg, m.to(gpu), SA, S1, last, s)
            # regenerated cells: z's bits exactly, a NaN's payload included
            assert torch.equal(_bits(got)[mm], _bits(z)[mm]), f"{kind} last={last}"
            if last:                                                                   # kept cells: x0's bits exactly
                assert torch.equal(_bits(got)[~mm], _bits(x0[:, :, s:s + L])[~mm])
            else:                                                                      # kept cells: add_noise's bits
                known = ops.add_noise(xg, bg, SA, S1)[:, :, s:s + L]
                assert torch.equal(_bits(got)[~mm], _bits(known)[~mm])                 # the kernel's own chain: every bit
                _same_bits(got, R.renoise_ref(z, x0, base, m, SA, S1, False, s), f"{kind} against the restatement")


@pytest.mark.parametrize("shape", [(4, 7, 3, 5), (3, 5, 2, 6), (4, 9, 8, 16), (1, 2, 48, 48)], ids=lambda s: "x".join(map(str, s)))
def test_all_ones_all_zeros_and_the_shared_chain(gpu, shape):
    ops, _ = _ops()
    C, T, h, w = shape
    z, x0, base = _clip(C, T, h, w, T, seed=11, plant=True)
    xg, bg = x0.to(gpu), base.to(gpu)
    ones, zeros = torch.ones(T, h, w, dtype=torch.uint8, device=gpu), torch.zeros(T, h, w, dtype=torch.uint8, device=gpu)
    for last in (False, True):
        assert torch.equal(_bits(ops.mask_renoise(z.to(gpu), xg, bg, ones, SA, S1, last, 0)), _bits(z))
    # an all-zeros mask (the job refuses one; the kernel does not): add_noise's bits, all of them, from one shared function
    for sa, s1 in ((SA, S1), (1.0, 0.0), (0.0999755859375, 0.99462890625)):
        got = ops.mask_renoise(z.to(gpu), xg, bg, zeros, sa, s1, False, 0)
        assert torch.equal(_bits(got), _bits(ops.add_noise(xg, bg, sa, s1)))
    assert torch.equal(_bits(ops.mask_renoise(z.to(gpu), xg, bg, zeros, SA, S1, True, 0)), _bits(x0))
    assert torch.equal(_bits(ops.mask_renoise(z.to(gpu), xg, None, zeros, 0.0, 0.0, True, 0)), _bits(x0))    # base unused with last


def test_bad_arguments_are_refused_before_a_launch(gpu):
    ops, VdxError = _ops()
    z, x0, base = _clip(4, 7, 3, 5, 3, seed=13)
    zg, xg, bg = z.to(gpu), x0.to(gpu), base.to(gpu)
    m = torch.ones(7, 3, 5, dtype=torch.uint8, device=gpu)
    keep = _bits(zg).clone()
    for s in (-1, 5, 7):
        with pytest.raises(VdxError, match="frames"):
            ops.mask_renoise(zg, xg, bg, m, SA, S1, False, s)
    two = m.clone()
    two[3, 1, 1] = 2
    with pytest.raises(ValueError, match="0 .keep. or 1"):
        ops.mask_renoise(zg, xg, bg, two, SA, S1, False, 0)
    m[0, 0, 0] = 0                                                  # a write drops the tag: the values are read again
    ops.mask_renoise(zg.clone(), xg, bg, m, SA, S1, False, 0)
    m[0, 0, 1] = 3
    with pytest.raises(ValueError):
        ops.mask_renoise(zg, xg, bg, m, SA, S1, False, 0)
    m[0, 0, 1] = 1
    for bad in (m[:, :, :4].contiguous(), m[:6].contiguous(), m.to(torch.int32), m.cpu()):
        with pytest.raises((VdxError, ValueError)):
            ops.mask_renoise(zg, xg, bg, bad, SA, S1, False, 0)
    with pytest.raises((VdxError, ValueError)):
        ops.mask_renoise(zg, xg[:, :3].contiguous(), bg, m, SA, S1, False, 0)
    with pytest.raises((VdxError, ValueError)):
        ops.mask_renoise(zg, xg, bg[:, :, :6].contiguous(), m, SA, S1, False, 0)
    with pytest.raises((VdxError, ValueError)):
        ops.mask_renoise(zg.float(), xg, bg, m, SA, S1, False, 0)
    with pytest.raises((VdxError, ValueError)):
        ops.mask_paste_f32(zg.float(), xg, m)                       # 3 frames against the clip's 7
    lib = ops._lib.load()                                           # and by the library itself, not only by the wrapper
    args = (zg.data_ptr(), xg.data_ptr(), bg.data_ptr(), m.data_ptr(), SA, S1, 0, 4, 7, 15)
    for s, L in ((-1, 3), (5, 3), (0, 0), (7, 1), (0, 8)):
        assert lib.vdx_mask_renoise_f16(*args, s, L, None) != 0 and b"frames" in lib.vdx_last_error()
    assert lib.vdx_mask_renoise_f16(*args[:2], None, *args[3:], 0, 3, None) != 0
    assert lib.vdx_mask_renoise_f16(xg.data_ptr(), *args[1:], 0, 7, None) != 0            # z overlaps an input
    with pytest.raises((VdxError, ValueError)):
        ops.mask_to_latent(torch.ones(2, 12, 16, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError):
        ops.mask_to_latent(torch.ones(2, 16, 16, dtype=torch.uint8, device=gpu), "bilinear")
    torch.cuda.synchronize()
    assert torch.equal(_bits(zg), keep)                             # nothing was launched on z


@pytest.mark.parametrize("shape", [(4, 7, 3, 5), (3, 5, 2, 6), (4, 9, 8, 16), (1, 2, 48, 48), (2, 1, 1, 1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_mask_paste_f32(gpu, shape):
    ops, _ = _ops()
    C, T, h, w = shape
    _, x0, _ = _clip(C, T, h, w, T, seed=17, plant=True)
    g = torch.Generator().manual_seed(19)
    z = torch.randn(1, C, T, h, w, generator=g)
    z.view(-1)[:4] = torch.tensor([NAN, -0.0, INF, 1e-42])[:min(4, z.numel())]          # an fp32 denormal among them
    for kind, m in _masks(T, h, w, 21).items():
        zg = z.to(gpu)
        got = ops.mask_paste_f32(zg, x0.to(gpu), m.to(gpu))
        assert got is zg
        _same_bits(got, R.paste_ref(z, x0, m), kind)                # float(x0) of a NaN is computed: its payload is not stated
        mm = m.bool()[None, None].expand(z.shape)
        assert torch.equal(_bits(got)[mm], _bits(z)[mm]), kind      # regenerated cells: every bit, a NaN's payload included


@pytest.mark.parametrize("shape", [(1, 8, 8), (3, 16, 24), (2, 72, 128)], ids=lambda s: "x".join(map(str, s)))
def test_mask_to_latent(gpu, shape):
    ops, _ = _ops()
    T, H, W = shape
    g = torch.Generator().manual_seed(23)
    px = (torch.rand(T, H, W, generator=g) < 0.02).to(torch.uint8) * 255
    px[0, 7, 7] = 1                                                 # dropped by nearest, kept by any
    px[0, 0, 0] = 0
    for rule in ("nearest", "any"):
        got = ops.mask_to_latent(px.to(gpu), rule)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (T, H // 8, W // 8)
        assert torch.equal(got.cpu(), R.latent_mask_ref(px, rule)), rule
        assert torch.equal(ops.mask_to_latent(px.bool().to(gpu), rule), got)
    assert int(ops.mask_to_latent(px.to(gpu), "nearest")[0, 0, 0]) == 0 and int(ops.mask_to_latent(px.to(gpu), "any")[0, 0, 0]) == 1
    assert ops.mask_to_latent(px.to(gpu)).equal(ops.mask_to_latent(px.to(gpu), "nearest"))          # the default


@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 8, 16, 3), (3, 24, 40, 3), (2, 6, 12, 3)], ids=lambda s: "x".join(map(str, s)))
def test_mask_composite_u8(gpu, shape):
    """Rows of 21 bytes (scalar), 48 (16 pixels per lane), 120 and 36 (4 pixels per lane: not a multiple of 16 bytes)."""
    ops, VdxError = _ops()
    g = torch.Generator().manual_seed(29)
    gen, orig = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) for _ in range(2))
    for kind, m in _masks(*shape[:3], 31).items():
        m = m * (255 if kind == "random" else 1)                    # nonzero = generated, whatever the value
        want = R.composite_ref(gen, orig, m)
        got = ops.mask_composite_u8(gen.to(gpu), orig.to(gpu), m.to(gpu))
        assert torch.equal(got.cpu(), want), kind
        x = gen.to(gpu)
        assert ops.mask_composite_u8(x, orig.to(gpu), m.to(gpu), out=x) is x and torch.equal(x.cpu(), want)     # in place
    # a batch that starts in mid-clip (decode_frames hands such views over): any pointer, the library picks the width
    T = shape[0]
    if T > 1:
        big_g, big_o, big_m = gen.to(gpu), orig.to(gpu), _masks(*shape[:3], 33)["random"].to(gpu)
        got = ops.mask_composite_u8(big_g[1:], big_o[1:], big_m[1:])
        assert torch.equal(got.cpu(), R.composite_ref(gen[1:], orig[1:], big_m[1:].cpu()))
    with pytest.raises(VdxError):
        ops.mask_composite_u8(gen.to(gpu), orig.to(gpu)[:, :, :-1], m.to(gpu))
    with pytest.raises(VdxError):
        ops.mask_composite_u8(gen.to(gpu), orig.to(gpu), m.to(gpu)[:, :-1])


# ---- the job on the tiny golden UNet ------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 8, 32, 32, 4                                     # 8 frames, chunk 6, overlap 2: windows (0, 6), (4, 8)
RANGES = [(0, 6), (4, 8)]
INFO_KEYS = {"chunk_size", "overlap", "ranges", "world_size", "num_frames", "denoise_s", "exchange", "steps_run",
             "emu_gather_delay_s", "net_gather_s", "network_bytes", "payload_bytes", "payload_bytes_actual"}


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    return build(gpu, 0, 1)


@pytest.fixture(scope="module")
def clean(gpu):
    from dist_inpaint_worker import clean_latent
    return clean_latent(T, HL, WL, gpu)


def _latent_masks(gpu):
    from vdx import inpaint, ops
    frames = torch.from_numpy(inpaint.expand_mask(inpaint.keep_frames_mask("0:3", T), T, HL * 8, WL * 8))
    block = torch.ones(T, HL * 8, WL * 8, dtype=torch.uint8)
    block[:, 40:168, 64:200] = 0                                    # keep a block through time; its edges cut latent cells
    return {"keep_frames 0:3": ops.mask_to_latent(frames.to(gpu)), "block": ops.mask_to_latent(block.to(gpu), "any")}


def _diffuser(model, clean, latent_mask, sampler="ddim", **kw):
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    kw = {**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx", device="cuda",
                 noise_device="cpu", strength=0.75, scheduler=sampler), **kw}
    return DistributedVideoDiffuser(DiffuserConfig(**kw), m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1],
                                    init_latents=clean, latent_mask=latent_mask)


@pytest.mark.parametrize("mode", ["hybrid_ctx", "hybrid"])
@pytest.mark.parametrize("co", [False, True], ids=["windowed", "co_denoise"])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_masked_job_is_the_loop(gpu, model, clean, sampler, co, mode):
    for kind, lm in _latent_masks(gpu).items():
        d = _diffuser(model, clean, lm, sampler, co_denoise=co, mode=mode)
        assert len(d.schedule) == 3 and (d.ctx is not None) == (mode == "hybrid_ctx")
        lat, info = d()
        assert info["ranges"] == RANGES and info["steps_run"] == 3 and lat.dtype == torch.float32
        assert set(info) == INFO_KEYS | ({"co_denoise"} if co else set())
        want, blended = R.masked_job_ref(d, model, clean, d._base, lm, co=co)
        assert torch.equal(_bits(lat), _bits(want)), kind
        # kept cells are the clip's latent exactly, frame 0 and the last frame included; regenerated ones are not
        keep = ~lm.bool().cpu()[None, None].expand(lat.shape)
        assert torch.equal(_bits(lat)[keep], _bits(clean.float())[keep]), kind
        assert not torch.equal(lat.cpu()[~keep], clean.float().cpu()[~keep])
        if not co:                                                  # the ramp blend zeroes frame 0: without the paste it is lost
            assert bool((blended[:, :, 0] == 0).all()) and bool(keep[:, :, 0].any())
            assert not torch.equal(blended[keep], clean.float().cpu()[keep])
        again, _ = d()                                              # run to run
        assert torch.equal(_bits(again), _bits(lat))


@pytest.mark.parametrize("co", [False, True], ids=["windowed", "co_denoise"])
def test_all_ones_mask_is_plain_video_to_video(gpu, model, clean, co):
    ones = torch.ones(T, HL, WL, dtype=torch.uint8, device=gpu)
    for sampler in ("ddim", "dpmpp_2m"):
        lat, _ = _diffuser(model, clean, ones, sampler, co_denoise=co)()
        plain, _ = _diffuser(model, clean, None, sampler, co_denoise=co)()
        assert torch.equal(_bits(lat), _bits(plain)), sampler


def test_job_without_the_flag_is_untouched(gpu, model, clean):
    d = _diffuser(model, clean, None)
    assert d.latent_mask is None and d._known is None
    lat, info = d()
    assert set(info) == INFO_KEYS
    chunks = [(s, e, d.denoise(d._start[:, :, s:e].clone())) for s, e in RANGES]
    assert torch.equal(lat, d.blend(chunks, d._start, 2))
    with pytest.raises(ValueError, match="init_latents"):
        from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser
        from vdx.scheduler import DDIMScheduler
        DistributedVideoDiffuser(DiffuserConfig(num_frames=T, steps=2, height=256, width=256, mode="chunk"), model[0], DDIMScheduler(),
                                 model[1][1:], model[1][:1], latent_mask=torch.ones(T, HL, WL, dtype=torch.uint8, device=gpu))
    masked = _diffuser(model, clean, torch.ones(T, HL, WL, dtype=torch.uint8, device=gpu))
    with pytest.raises(ValueError, match="allgather"):
        masked(exchange="halo")


def test_two_ranks_end_with_the_bits_of_one(gpu, model, clean, tmp_path):
    """Two processes, one rank each, both on this box's one GPU and talking over gloo, windowed and co-denoised.  Each child has
    its own time limit; a failure ends the test before the next one starts."""
    from vdx.planner import plan
    assert plan(8, 1, 6, 2).ranges == plan(8, 2, 6, 2).ranges == ((0, 6), (4, 8))
    lm = _latent_masks(gpu)["keep_frames 0:3"]
    for co, port in ((False, "29751"), (True, "29753")):
        out = tmp_path / f"rank0_{int(co)}.pt"
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                            "--master-addr", "127.0.0.1", "--master-port", port,
                            os.path.join(ROOT, "tests", "dist_inpaint_worker.py"), str(out), "8", "6", "2", str(STEPS), "dpmpp_2m",
                            "0:3", str(int(co))], capture_output=True, text=True, timeout=300, env=dict(os.environ))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert r.stdout.count("ok") == 2
        got = torch.load(out, weights_only=True)
        lat, _ = _diffuser(model, clean, lm, "dpmpp_2m", co_denoise=co)()
        assert got["ranges"] == RANGES and got["world_size"] == 2 and got["steps_run"] == 3
        assert torch.equal(_bits(got["lat"]), _bits(lat)), "co_denoise" if co else "windowed"


# ---- run_job end to end on synthetic weights ---------------------------------------------------------------------------------
def test_run_job_end_to_end(gpu, tmp_path):
    """128 x 128 (the smallest the synthetic VAE's tests use), 4 frames: the written frames' kept pixels are the input's bytes
    with the paste, the decoder's without; the record; the CSV row's header and columns as without the flag."""
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.metrics import CSV_HEADER, append_csv, result_row
    from vdx.pipeline import build_arg_parser, config_from_args, run_job
    F, H, W = 4, 128, 128
    g = torch.Generator().manual_seed(37)
    clip = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8).numpy()
    mask = np.ones((F, H, W), np.uint8)
    mask[:2] = 0                                                    # keep frames 0 and 1 ...
    mask[2:, 16:72, 24:100] = 0                                     # ... and a block of the others
    np.save(tmp_path / "clip.npy", clip)
    np.save(tmp_path / "mask.npy", mask)
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    base = ["--model_id", "synthetic:tiny", "--init_video", str(tmp_path / "clip.npy"), "--strength", "0.5", "--num_frames", "4",
            "--steps", "4", "--height", "128", "--width", "128", "--chunk_size", "4", "--overlap", "2", "--noise_device", "cpu"]

    def job(extra):
        got = {}
        res = run_job(config_from_args(build_arg_parser().parse_args(base + extra)), out_video=None, pipe=pipe, clip_inputs=got)
        return res, np.stack(got["frames"])
    res0, plain = job([])
    res1, pasted = job(["--mask", str(tmp_path / "mask.npy")])
    res2, raw = job(["--mask", str(tmp_path / "mask.npy"), "--mask_paste", "off"])
    res3, _ = job(["--keep_frames", "0:2", "--mask_rule", "any"])
    keep = mask == 0
    assert np.array_equal(pasted[keep], clip[keep])                 # the input's bytes
    assert not np.array_equal(raw[keep], clip[keep])                # the decoder's rendering of the kept latent
    assert np.array_equal(pasted[~keep], raw[~keep])                # the generated pixels are the same with and without the paste
    assert not np.array_equal(raw, plain)
    assert "mask" not in res0
    lat_kept = float((R.latent_mask_ref(torch.from_numpy(mask)).numpy() == 0).mean())
    assert res1["mask"] == {"rule": "nearest", "paste": True, "kept_fraction": lat_kept, "kept_frames": 2}
    assert res2["mask"] == {**res1["mask"], "paste": False}
    assert res3["mask"] == {"rule": "any", "paste": True, "kept_fraction": 0.5, "kept_frames": 2}
    assert set(res1) == set(res0) | {"mask"} and res1["steps_run"] == res0["steps_run"] == 2
    rows = []
    for res in (res0, res1):
        path = tmp_path / f"r{len(rows)}.csv"
        append_csv(str(path), result_row(res, mode="hybrid_ctx", num_frames=F, elapsed_s=1.0))
        rows.append(list(csv.reader(open(path))))
    assert rows[0][0] == rows[1][0] == CSV_HEADER and len(rows[1][1]) == len(CSV_HEADER)
    timed = {"timestamp", "latency_s", "denoise_s", "net_gather_s", "net_reduce_s", "peak_vram_mb", "end_vram_mb", "temp_instab", "flow_err",
             "throughput_fps"}
    for name, a, b in zip(CSV_HEADER, rows[0][1], rows[1][1]):
        if name not in timed:
            assert a == b, name
