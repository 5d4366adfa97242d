"""-m gpu: regional prompts through the job (vdx/pipeline.py, vdx/codenoise.py) on the tiny UNet: 8 frames, chunk 6, overlap 2, 2
steps.  Bit for bit: the windowed job (both schedulers) and the co-denoised job (flat, ring windows, strided windows) against a
Python loop written here over the same windows, which calls the UNet with the tables restated by tests/region_ref.py and each
window's own (s, L, d, ring), also with a kept-frames mask and with FreeInit; all-zero masks against the job without the option;
two ranks against one (two fresh processes on this box's one GPU, tests/dist_region_worker.py), with both exchanges; `run_job` end
to end with two `--region` flags; and `main`'s CSV row and JSON records with and without the flag."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import region_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HL, WL, STEPS = 8, 32, 32, 2


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _masks():
    """0 / 255 only, edges off the cell grid: every weight is a ratio of small integers, the same float64 in any order of
    summation, so the restated tables equal the plan's exactly.  Region 1: static, the left 100 pixels; region 2: per frame, a
    band from the top that grows with the frames and is absent on frames 0 and 1; they overlap."""
    H, W = 8 * HL, 8 * WL
    m1 = np.zeros((H, W), np.uint8)
    m1[:, :100] = 255
    m2 = np.zeros((T, H, W), np.uint8)
    for t in range(2, T):
        m2[t, :20 * t, 60:] = 255
    return m1, m2


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    from vdx.region import RegionPlan, region_plan
    m, emb = build(gpu, 0, 1)
    rtext = torch.randn(2, 77, emb.shape[2], generator=torch.Generator().manual_seed(9)).half().to(gpu)
    masks = _masks()
    plan = region_plan([(mk, f"text {i}") for i, mk in enumerate(masks)], T, HL, WL, 4)
    tabs = R.weights(masks, T, HL, WL, 4)
    assert all(np.array_equal(a, b) for a, b in zip(plan.tables, tabs)) and any(((t > 0) & (t < 1)).any() for t in tabs)
    restated = RegionPlan(T, HL, WL, tuple(torch.from_numpy(t).to(gpu) for t in tabs), tuple(R.level_grid(HL, WL, 1 << l) for l in range(4)),
                          np.stack([(t != 0).any(axis=1) for t in tabs]))
    return m, emb, rtext, plan, restated


def _config(**kw):
    from vdx.pipeline import DiffuserConfig
    return DiffuserConfig(**{**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                                    device="cuda", noise_device="cpu"), **kw})


def _diffuser(model, regions=True, sampler="ddim", plan=None, extra=None, **kw):
    from vdx.pipeline import DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    m, emb, rtext, rplan, _ = model
    cfg = _config(scheduler=sampler, **kw)
    extra = dict(extra or {})
    if regions:
        extra["regions"] = (rtext, plan or rplan)
    return DistributedVideoDiffuser(cfg, m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1], **extra)


def _base(d):
    from vdx.pipeline import seeded_noise
    return seeded_noise(d.latent_shape, d.scheduler.init_noise_sigma, "cuda", "cpu")


def _windowed_loop(d, model, start=None, ctx=None, masked=False):
    """The windowed job written out: every window's own trajectory with the restated tables and its place in the clip, then the
    job's ramp blend.  `start`, `ctx`: the round's start latent and context (default: the seeded noise and the job's context);
    `masked`: after every step the job's mask step on the window's frames, and after the blend its paste."""
    from vdx import ops
    m, emb, rtext, _, restated = model
    text = torch.cat([emb[1:], emb[:1]])
    start = _base(d) if start is None else start
    ctx = d.ctx if ctx is None else ctx
    chunks = []
    for s, e in d.plan().ranges:
        lat = start[:, :, s:e].clone().contiguous()
        reset = getattr(d.scheduler, "reset", None)
        if reset is not None:
            reset()
        for i, t in enumerate(d.schedule):
            noise = m(ops.cfg_input(lat, ctx, d.cfg.context_weight), t, encoder_hidden_states=text, regions=(rtext, restated, (s, e - s, 1, False))).sample
            lat = d.scheduler.step_cfg(noise, t, lat, d.cfg.guidance_scale)
            if masked:
                d._mask_step(lat, i, s)
        chunks.append((s, e, lat))
    out = d.blend(chunks, start, d.plan().overlap)
    if masked:
        ops.mask_paste_f32(out, d._x0, d.latent_mask)
    return out


def _co_loop(d, model, gpu, strided=None):
    """The co-denoised round written out: per step every window through the window input the job uses and the UNet with the restated
    tables and the window's (s, L, d, ring) into the packed buffer, then the job's fused step."""
    from vdx import ops
    from vdx.codenoise import loop_table, stride_table, window_table
    m, emb, rtext, _, restated = model
    text = torch.cat([emb[1:], emb[:1]])
    cfg, sched = d.cfg, d.scheduler
    cp = strided if strided is not None else d.plan()
    table = stride_table(strided, T) if strided is not None else (loop_table(cp, T) if cfg.loop else window_table(cp, T))
    slot = 2 * 4 * cp.chunk * HL * WL
    rows = table.rows(1, cp.per_rank, slot)
    wn = table.wn.to(gpu)
    wins = list(cp.windows) if strided is not None else [(s, e - s, 1) for s, e in cp.ranges]
    packed = torch.zeros((cp.per_rank, slot), dtype=torch.float16, device=gpu)
    z = _base(d).clone()
    reset = getattr(sched, "reset", None)
    if reset is not None:
        reset()
    for t in d.schedule:
        for j, (s, L, dd) in enumerate(wins):
            if strided is not None:
                x = ops.cfg_input_stride(z, d.ctx, cfg.context_weight, s, L, dd)
            elif cfg.loop:
                x = ops.cfg_input_loop(z, d.ctx, cfg.context_weight, s, L)
            else:
                x = ops.cfg_input_window(z, d.ctx, cfg.context_weight, s, s + L)
            noise = m(x, t, encoder_hidden_states=text, regions=(rtext, restated, (s, L, dd, bool(cfg.loop)))).sample
            packed[j, :noise.numel()].copy_(noise.reshape(-1))
        if strided is not None:
            z = sched.step_cfg_strided(packed, rows, wn, t, z, cfg.guidance_scale)
        elif cfg.loop:
            z = sched.step_cfg_loop(packed, rows, wn, t, z, cfg.guidance_scale)
        else:
            z = sched.step_cfg_windows(packed, rows, wn, t, z, cfg.guidance_scale)
    return z.float()


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_the_windowed_job_is_the_loop(gpu, model, sampler):
    d = _diffuser(model, sampler=sampler)
    lat, info = d()
    assert info["ranges"] == [(0, 6), (4, 8)] and "regions" not in info             # the record is the front end's: it knows the texts
    want = _windowed_loop(d, model)
    assert bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat), _bits(want))
    again, _ = d()
    assert torch.equal(_bits(again), _bits(lat))
    plain, _ = _diffuser(model, regions=False, sampler=sampler)()
    assert not torch.equal(plain, lat)


CO = {"flat": dict(), "loop": dict(loop=True), "context_stride 2": dict(context_stride=2)}


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("mode", list(CO))
def test_the_co_denoised_job_is_the_loop(gpu, model, mode, sampler):
    from vdx.codenoise import stride_plan_of
    d = _diffuser(model, sampler=sampler, co_denoise=True, **CO[mode])
    lat, info = d()
    strided = stride_plan_of(d.cfg, 1) if d.cfg.context_stride > 1 else None
    want = _co_loop(d, model, gpu, strided)
    assert bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat), _bits(want))
    assert info["co_denoise"]["windows"] == {"flat": 2, "loop": 2, "context_stride 2": 4}[mode]
    plain, _ = _diffuser(model, regions=False, sampler=sampler, co_denoise=True, **CO[mode])()
    assert not torch.equal(plain, lat)


def _masked_extra(gpu):
    g = torch.Generator().manual_seed(4)
    keep = torch.ones(T, HL, WL, dtype=torch.uint8)
    keep[:3] = 0                                                    # keep the first three frames
    return dict(init_latents=torch.randn(1, 4, T, HL, WL, generator=g).half().to(gpu), latent_mask=keep.to(gpu))


def test_the_masked_job_is_the_loop_with_the_mask_step(gpu, model):
    """Frames 0 to 2 kept (`--keep_frames 0:2`), the regions' non-zero masks: the loop with the job's mask step after every step and
    its paste after the blend; the kept frames end as the clean latent's."""
    extra = _masked_extra(gpu)
    d = _diffuser(model, extra=extra, strength=0.75, steps=4)
    lat, _ = d()
    want = _windowed_loop(d, model, start=d._start, masked=True)
    assert len(d.schedule) == 3 and bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat), _bits(want))
    assert torch.equal(lat[:, :, :3], extra["init_latents"][:, :, :3].float())
    plain, _ = _diffuser(model, regions=False, extra=extra, strength=0.75, steps=4)()
    assert not torch.equal(plain[:, :, 3:], lat[:, :, 3:])


def test_the_free_init_job_is_the_loop_round_after_round(gpu, model):
    """`--free_init 2`: the windowed loop, the job's re-initialisation of its result, the context of the new start, the loop again."""
    from vdx import freeinit
    d = _diffuser(model, free_init_iters=2)
    lat, info = d()
    cfg, base = d.cfg, _base(d)
    first = _windowed_loop(d, model, start=base)
    filt = freeinit.lowpass_filter(base.shape[2:], cfg.free_init_method, cfg.free_init_spatial, cfg.free_init_temporal, cfg.free_init_order).to(gpu)
    start = freeinit.reinit(first, base, d.scheduler, 1, filt, cfg.noise_device)
    want = _windowed_loop(d, model, start=start, ctx=start.mean(dim=2, keepdim=True).contiguous())
    assert info["free_init"]["iters"] == 2 and bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat), _bits(want))
    assert not torch.equal(_bits(first), _bits(want))
    plain, _ = _diffuser(model, regions=False, free_init_iters=2)()
    assert not torch.equal(plain, lat)


@pytest.mark.parametrize("case", ["windowed", "co_denoise", "no_chunking", "masked", "free_init"])
def test_all_zero_masks_are_the_job_without_the_option(gpu, model, case):
    """Every window of every mode passes its place in the clip, and nothing beyond the base text is launched: the job's bits."""
    from vdx.region import region_plan
    zero = region_plan([(np.zeros((8 * HL, 8 * WL), np.uint8), "a"), (np.zeros((T, 8 * HL, 8 * WL), np.uint8), "b")], T, HL, WL, 4)
    kw = {"windowed": dict(), "co_denoise": dict(co_denoise=True), "no_chunking": dict(mode="fsdp"), "masked": dict(strength=0.75, steps=4),
          "free_init": dict(free_init_iters=2)}[case]
    extra = _masked_extra(gpu) if case == "masked" else None
    calls, m = [], model[0]
    forward = m.forward

    def spy(*a, **k):
        calls.append(k.get("regions"))
        return forward(*a, **k)

    try:
        m.forward = spy
        lat, info = _diffuser(model, plan=zero, extra=extra, **kw)()
        with_regions, calls[:] = list(calls), []
        plain, info0 = _diffuser(model, regions=False, extra=extra, **kw)()
    finally:
        del m.forward
    assert torch.equal(_bits(lat), _bits(plain)) and set(info) == set(info0)
    assert with_regions and all(r is not None and r[2][1] <= T for r in with_regions) and all(r is None for r in calls)
    assert len(with_regions) == len(calls)
    if case in ("windowed", "masked", "free_init"):
        assert {r[2] for r in with_regions} == {(0, 6, 1, False), (4, 4, 1, False)}


def test_regions_are_checked_against_the_clip(gpu, model):
    from vdx.pipeline import DistributedVideoDiffuser
    from vdx.region import region_plan
    from vdx.scheduler import DDIMScheduler
    m, emb, rtext, plan, _ = model
    short = region_plan([(mk[:4] if mk.ndim == 3 else mk, "t") for mk in _masks()], 4, HL, WL, 4)
    for regions in ((rtext[:1], plan), (rtext, short)):
        with pytest.raises(ValueError, match="regions"):
            DistributedVideoDiffuser(_config(), m, DDIMScheduler(), emb[1:], emb[:1], regions=regions)


def test_denoise_needs_the_window_with_regions(gpu, model):
    d = _diffuser(model)
    with pytest.raises(ValueError, match="window"):
        d.denoise(_base(d)[:, :, 4:8].clone())


# ---- two ranks against one ----------------------------------------------------------------------------------------------------------
LIMIT_S = 300


@pytest.mark.parametrize("co,exchange,port", [(True, "allgather", "29771"), (False, "allgather", "29773"), (False, "halo", "29775")],
                         ids=["co_denoise", "windowed", "windowed halo"])
def test_two_ranks_end_with_the_bits_of_one(gpu, tmp_path, co, exchange, port):
    """8 frames, chunk 6, overlap 2: windows (0, 6) and (4, 8), one per rank, so rank 1's window starts at clip frame 4 and takes
    the masks of frames 4 to 7; every rank holds the same plan.  With the all-gather the worker itself checks that both ranks hold
    identical bits; with the halo exchange it assembles the ranks' owned segments.  The test starts the two ranks itself, each under
    its own time limit, and nothing else."""
    from dist_pipeline_worker import build
    from dist_region_worker import masks_of, regions_of
    from vdx.pipeline import DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    out = tmp_path / "rank0.pt"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "dist_region_worker.py"), str(out), str(T), "6", "2", str(STEPS), "dpmpp_2m", "1" if co else "0",
           exchange]
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, VDX_SHARE_GPU="1")
    logs = [open(tmp_path / f"rank{r}.log", "w+") for r in range(2)]    # files, not pipes: a rank never blocks on its output
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=logs[r], stderr=subprocess.STDOUT)
             for r in range(2)]
    try:
        for p in procs:
            p.wait(timeout=LIMIT_S)                                  # each rank under its own limit
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r, (p, log) in enumerate(zip(procs, logs)):
        log.seek(0)
        text = log.read()
        log.close()
        assert p.returncode == 0, text[-4000:]
        assert f"rank {r} ok" in text
    got = torch.load(out, weights_only=True)
    assert all(np.array_equal(a, b) for a, b in zip(masks_of(T), _masks()))
    m, emb = build(gpu, 0, 1)
    d = DistributedVideoDiffuser(_config(scheduler="dpmpp_2m", co_denoise=co), m, make_scheduler("dpmpp_2m", DDIMScheduler()), emb[1:], emb[:1],
                                 regions=regions_of(emb, T, gpu))
    lat, info = d()
    assert torch.equal(got["lat"].view(torch.int32), lat.cpu().view(torch.int32))
    gi = got["info"]
    assert [tuple(x) for x in gi["ranges"]] == [(0, 6), (4, 8)] == [tuple(x) for x in info["ranges"]] and gi["world_size"] == 2
    assert [tuple(w) for w in got["windows"]] == [(0, 6, 1, False)]   # rank 0 ran its own window only; rank 1 the one from frame 4
    plain, _ = DistributedVideoDiffuser(_config(scheduler="dpmpp_2m", co_denoise=co), m, make_scheduler("dpmpp_2m", DDIMScheduler()), emb[1:], emb[:1])()
    assert not torch.equal(plain[:, :, 6:], lat[:, :, 6:])           # frames only rank 1 computed carry the regions


# ---- run_job end to end on synthetic weights ---------------------------------------------------------------------------------
def test_run_job_end_to_end_writes_the_record(gpu, tmp_path):
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import build_arg_parser, config_from_args, run_job
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    base = ["--model_id", "synthetic:tiny", "--num_frames", str(T), "--steps", "2", "--height", "128", "--width", "128", "--chunk_size", "6",
            "--overlap", "2", "--noise_device", "cpu", "--prompt", "a forest"]
    left = np.zeros((128, 128), np.uint8)
    left[:, :64] = 255
    late = np.zeros((T, 128, 128), np.uint8)
    late[4:, 64:, 32:] = 255
    np.save(tmp_path / "left.npy", left)
    np.save(tmp_path / "late.npy", late)
    np.save(tmp_path / "zero.npy", np.zeros((128, 128), np.uint8))

    def job(extra, out_video=None):
        got = {}
        res = run_job(config_from_args(build_arg_parser().parse_args(base + extra)), out_video=out_video, pipe=pipe, clip_inputs=got)
        return res, got
    res0, got0 = job([])
    res1, got1 = job(["--region", str(tmp_path / "left.npy"), "a fox: red; close", "--region", str(tmp_path / "late.npy"), "a pine forest"],
                     out_video=str(tmp_path / "regions.mp4"))
    assert "regions" not in res0 and set(res1) == set(res0) | {"regions"} and list(res1)[-1] == "regions"
    rec = res1["regions"]
    assert rec["count"] == 2 and rec["texts"] == ["a fox: red; close", "a pine forest"]
    # the left half; 4 of 8 frames x the lower half x 3/4 of the width; a quarter of the width is shared, half and half
    assert rec["coverage"] == [0.375, 0.5 - 0.03125, 0.1875 - 0.03125]
    f0, f1 = np.stack(got0["frames"]), np.stack(got1["frames"])
    assert f1.shape == (T, 128, 128, 3) and not np.array_equal(f0, f1)
    assert res1["frames_written"] == T and os.path.getsize(tmp_path / "regions.mp4") > 0
    res2, got2 = job(["--region", str(tmp_path / "zero.npy"), "nothing"])            # all-zero: the job without the flag, byte for byte
    assert np.array_equal(np.stack(got2["frames"]), f0) and res2["regions"]["coverage"] == [1.0, 0.0]
    res3, _ = job(["--co_denoise", "--loop", "--region", str(tmp_path / "late.npy"), "a pine forest"])
    assert res3["regions"]["count"] == 1 and "loop" in res3 and "co_denoise" in res3
    with pytest.raises(ValueError, match="cannot be combined with prompt_travel"):
        job(["--region", str(tmp_path / "left.npy"), "a fox", "--prompt_at", "3", "a desert"])


def test_main_writes_the_csv_row_and_the_records(gpu, tmp_path):
    """`python -m vdx.pipeline`: without the flag the CSV row and the JSON records have the columns and keys they always had and no
    "regions"; with `--region` (an all-zero mask: the same frames) the CSV row is the same outside the timed columns, and the
    --compare_json and --clip_json records gain "regions" beside their own entries."""
    from vdx import pipeline
    base = ["--model_id", "synthetic:tiny", "--num_frames", str(T), "--steps", "2", "--height", "128", "--width", "256", "--chunk_size", "6",
            "--overlap", "2", "--mode", "chunk", "--out_video", "", "--noise_device", "cpu"]
    got = {}
    res = pipeline.run_job(pipeline.config_from_args(pipeline.build_arg_parser().parse_args(base)), out_video=None, clip_inputs=got)
    first = tmp_path / "first.npy"
    np.save(first, np.stack(got["frames"]))
    np.save(tmp_path / "zero.npy", np.zeros((128, 256), np.uint8))
    out_csv = str(tmp_path / "r.csv")
    records = {}
    for name, flags in (("off", []), ("on", ["--region", str(tmp_path / "zero.npy"), "a fox: red"])):
        cmp_js, clip_js = tmp_path / f"cmp_{name}.json", tmp_path / f"clip_{name}.json"
        assert pipeline.main(base + flags + ["--out_csv", out_csv, "--compare_to", str(first), "--compare_json", str(cmp_js),
                                             "--clip_json", str(clip_js)]) == 0
        records[name] = (json.loads(cmp_js.read_text()), json.loads(clip_js.read_text()))
    rows = list(csv.DictReader(open(out_csv)))
    timed = {"timestamp", "latency_s", "throughput_fps", "net_gather_s", "net_reduce_s", "peak_vram_mb", "end_vram_mb"}
    assert len(rows) == 2 and rows[0].keys() == rows[1].keys() and not any("region" in k for k in rows[0])
    assert {k: v for k, v in rows[0].items() if k not in timed} == {k: v for k, v in rows[1].items() if k not in timed}
    rec = {"count": 1, "texts": ["a fox: red"], "coverage": [1.0, 0.0]}
    for off, on in zip(records["off"], records["on"]):
        assert "regions" not in off and on["regions"] == rec and set(on) == set(off) | {"regions"}
    assert records["off"][0]["identical"] is True and records["on"][0]["identical"] is True      # today's bytes, with and without
    assert set(records["off"][1]) == {"clip_score", "per_frame", "synthetic_weights", "tokenizer", "n_frames"}
    assert "regions" not in res
