"""-m gpu: prompt travel through the job (vdx/pipeline.py, vdx/codenoise.py) on the tiny UNet: 8 frames, chunk 6, overlap 2, 2
steps.  Bit for bit: the windowed job and the co-denoised job (flat, ring windows, strided windows, tiles) against a Python loop
written here over the same windows, which builds each window's text with the restatement of tests/travel_ref.py and calls the
UNet, the window inputs and the scheduler steps that the job without the option calls; a single key equal to the prompt against
the job without the option; and `run_job` end to end."""
import os
import sys

import numpy as np
import pytest
import torch

import travel_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HL, WL, STEPS = 8, 32, 32, 2
KEY_FRAMES = [0, 3, 7]


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    m, emb = build(gpu, 0, 1)
    keys = torch.randn(len(KEY_FRAMES), 77, emb.shape[2], generator=torch.Generator().manual_seed(9)).half().to(gpu)
    return m, emb, keys


def _config(**kw):
    from vdx.pipeline import DiffuserConfig
    return DiffuserConfig(**{**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                                    device="cuda", noise_device="cpu"), **kw})


def _diffuser(model, travel=True, sampler="ddim", frames=KEY_FRAMES, key_embs=None, **kw):
    from vdx.pipeline import DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    from vdx.travel import travel_plan
    m, emb, keys = model
    cfg = _config(scheduler=sampler, **kw)
    extra = {}
    if travel:
        extra["travel"] = (keys if key_embs is None else key_embs, travel_plan([(f, "") for f in frames], T, loop=cfg.loop))
    return DistributedVideoDiffuser(cfg, m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1], **extra)


def _base(d):
    from vdx.pipeline import seeded_noise
    return seeded_noise(d.latent_shape, d.scheduler.init_noise_sigma, "cuda", "cpu")


def _window_text(model, gpu, loop, s, L, dd=1, ring=False):
    """A window's text by the restatement, from the keys on the CPU."""
    _, emb, keys = model
    lo, hi, w = R.plan(KEY_FRAMES, T, loop)
    return R.text_travel(keys.cpu(), emb[1].cpu(), lo, hi, w, s, L, dd, ring).to(gpu)


def _windowed_loop(d, model, gpu):
    """The windowed job written out: every window's own trajectory with its restated text, then the job's ramp blend."""
    from vdx import ops
    m = model[0]
    start, chunks = _base(d), []
    for s, e in d.plan().ranges:
        text = _window_text(model, gpu, False, s, e - s)
        lat = start[:, :, s:e].clone().contiguous()
        reset = getattr(d.scheduler, "reset", None)
        if reset is not None:
            reset()
        for t in d.schedule:
            noise = m(ops.cfg_input(lat, d.ctx, d.cfg.context_weight), t, encoder_hidden_states=text).sample
            lat = d.scheduler.step_cfg(noise, t, lat, d.cfg.guidance_scale)
        chunks.append((s, e, lat))
    return d.blend(chunks, start, d.plan().overlap)


def _co_loop(d, model, gpu, tiles=None, strided=None):
    """The co-denoised round written out: per step every window (and every tile of it) through the window input the job uses and
    the UNet with the window's restated text into the packed buffer, then the job's fused step."""
    from vdx import ops
    from vdx.codenoise import loop_table, stride_table, window_table
    m, cfg, sched = model[0], d.cfg, d.scheduler
    cp = strided if strided is not None else d.plan()
    table = stride_table(strided, T) if strided is not None else (loop_table(cp, T) if cfg.loop else window_table(cp, T))
    boxes = [()] if tiles is None else tiles.boxes
    area = HL * WL if tiles is None else tiles.th * tiles.tw
    slot = 2 * 4 * cp.chunk * area
    nt = len(boxes)
    rows = table.rows(1, cp.per_rank, nt * slot)
    wn = table.wn.to(gpu)
    wins = list(cp.windows) if strided is not None else [(s, e - s, 1) for s, e in cp.ranges]
    packed = torch.zeros((cp.per_rank, nt * slot), dtype=torch.float16, device=gpu)
    z = _base(d).clone()
    reset = getattr(sched, "reset", None)
    if reset is not None:
        reset()
    for t in d.schedule:
        for j, (s, L, dd) in enumerate(wins):
            text = _window_text(model, gpu, cfg.loop, s, L, dd, cfg.loop)
            for k, box in enumerate(boxes):
                if strided is not None:
                    x = ops.cfg_input_stride(z, d.ctx, cfg.context_weight, s, L, dd)
                elif cfg.loop:
                    x = ops.cfg_input_loop(z, d.ctx, cfg.context_weight, s, L)
                elif tiles is not None:
                    x = ops.cfg_input_tile(z, d.ctx, cfg.context_weight, s, s + L, *box)
                else:
                    x = ops.cfg_input_window(z, d.ctx, cfg.context_weight, s, s + L)
                noise = m(x, t, encoder_hidden_states=text).sample
                packed[j, k * slot:k * slot + noise.numel()].copy_(noise.reshape(-1))
        if strided is not None:
            z = sched.step_cfg_strided(packed, rows, wn, t, z, cfg.guidance_scale)
        elif cfg.loop:
            z = sched.step_cfg_loop(packed, rows, wn, t, z, cfg.guidance_scale)
        elif tiles is not None:
            z = sched.step_cfg_tiles(packed, rows, wn, tiles.grid(slot, gpu), t, z, cfg.guidance_scale)
        else:
            z = sched.step_cfg_windows(packed, rows, wn, t, z, cfg.guidance_scale)
    return z.float()


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_the_windowed_job_is_the_loop(gpu, model, sampler):
    d = _diffuser(model, sampler=sampler)
    lat, info = d()
    assert info["ranges"] == [(0, 6), (4, 8)] and "prompt_travel" not in info      # the record is the front end's: it knows the texts
    want = _windowed_loop(d, model, gpu)
    assert bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat), _bits(want))
    assert model[0].text_cache_slots == 1                            # handed back as it came
    again, _ = d()
    assert torch.equal(_bits(again), _bits(lat))
    plain, _ = _diffuser(model, travel=False, sampler=sampler)()
    assert not torch.equal(plain, lat)


CO = {"flat": dict(), "loop": dict(loop=True), "context_stride 2": dict(context_stride=2),
      "tile": dict(tile=(128, 256), tile_overlap=(64, 64))}


@pytest.mark.parametrize("mode", list(CO))
def test_the_co_denoised_job_is_the_loop(gpu, model, mode):
    from vdx.codenoise import stride_plan_of, tile_plan
    from vdx.options import check_tile
    d = _diffuser(model, co_denoise=True, **CO[mode])
    lat, info = d()
    tiles = tile_plan(HL, WL, *check_tile(d.cfg)) if d.cfg.tile is not None else None
    strided = stride_plan_of(d.cfg, 1) if d.cfg.context_stride > 1 else None
    assert tiles is None or tiles.count > 1
    want = _co_loop(d, model, gpu, tiles, strided)
    assert bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat), _bits(want))
    assert info["co_denoise"]["windows"] == {"flat": 2, "loop": 2, "context_stride 2": 4, "tile": 2}[mode] and model[0].text_cache_slots == 1
    assert tiles is None or info["tile"]["windows"] == 2 * tiles.count      # every tile of a window shared the window's text
    plain, _ = _diffuser(model, travel=False, co_denoise=True, **CO[mode])()
    assert not torch.equal(plain, lat)


@pytest.mark.parametrize("kw", [dict(), dict(co_denoise=True), dict(mode="fsdp")], ids=["windowed", "co_denoise", "no_chunking"])
def test_a_single_key_equal_to_the_prompt_is_the_job_without_the_option(gpu, model, kw):
    _, emb, _ = model
    one = _diffuser(model, frames=[0], key_embs=emb[:1].clone(), **kw)
    lat, info = one()
    plain, info0 = _diffuser(model, travel=False, **kw)()
    assert torch.equal(_bits(lat), _bits(plain)) and set(info) == set(info0)


def test_travel_is_checked_against_the_clip(gpu, model):
    from vdx.travel import travel_plan
    m, emb, keys = model
    from vdx.pipeline import DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    for travel in ((keys[:2], travel_plan([(f, "") for f in KEY_FRAMES], T)), (keys, travel_plan([(f, "") for f in KEY_FRAMES], T + 1))):
        with pytest.raises(ValueError, match="travel"):
            DistributedVideoDiffuser(_config(), m, DDIMScheduler(), emb[1:], emb[:1], travel=travel)


# ---- run_job end to end on synthetic weights ---------------------------------------------------------------------------------
def test_run_job_end_to_end_writes_the_record(gpu, tmp_path):
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import build_arg_parser, config_from_args, run_job
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    base = ["--model_id", "synthetic:tiny", "--num_frames", str(T), "--steps", "2", "--height", "128", "--width", "128", "--chunk_size", "6",
            "--overlap", "2", "--noise_device", "cpu", "--prompt", "a forest"]

    def job(extra, out_video=None):
        got = {}
        res = run_job(config_from_args(build_arg_parser().parse_args(base + extra)), out_video=out_video, pipe=pipe, clip_inputs=got)
        return res, got
    res0, got0 = job([])
    res1, got1 = job(["--prompt_at", "7", "a desert: dusk; wide", "--prompt_at", "4", "a shore"], out_video=str(tmp_path / "travel.mp4"))
    assert "prompt_travel" not in res0 and set(res1) == set(res0) | {"prompt_travel"} and list(res1)[-1] == "prompt_travel"
    assert res1["prompt_travel"] == {"keys": [[0, "a forest"], [4, "a shore"], [7, "a desert: dusk; wide"]]}
    f0, f1 = np.stack(got0["frames"]), np.stack(got1["frames"])
    assert f1.shape == (T, 128, 128, 3) and not np.array_equal(f0, f1)
    assert res1["frames_written"] == T and os.path.getsize(tmp_path / "travel.mp4") > 0
    res2, got2 = job(["--co_denoise", "--loop", "--prompt_at", "5", "a desert"])
    assert res2["prompt_travel"] == {"keys": [[0, "a forest"], [5, "a desert"]]} and "loop" in res2 and "co_denoise" in res2
    assert pipe.unet.text_cache_slots == 1
