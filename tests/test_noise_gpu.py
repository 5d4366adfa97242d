"""The seeded noise generator "philox4x32-10/v1" on the GPU (csrc/noise.hip, ops.philox_normal, vdx/noise.py, vdx/pipeline.py,
vdx/miner.py) against the numpy restatement of tests/noise_ref.py, bit for bit: whole tensors in both dtypes over the seeds and
streams, sigma against torch-CPU's half multiply, boxes against slices of the whole, the counter's high word, refusals that launch
nothing, and the job: its start latent, context, FreeInit and posterior streams, the masked job's base, and the records.

Every output is a view into a byte buffer with 256 canary bytes on both sides."""
import os
import sys

import numpy as np
import pytest
import torch

import noise_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, FILL = 256, 0xA5
RAGGED, EVEN, HEADLINE = (1, 3, 3, 5, 7), (1, 4, 2, 8, 8), (1, 4, 24, 72, 128)     # 315 elements: a ragged last block
NP = {torch.float16: np.float16, torch.float32: np.float32}


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    return ops, VdxError


def _bits(t):
    if torch.is_tensor(t):
        t = t.detach().cpu().contiguous().numpy()
    return t.view(np.uint16) if t.dtype == np.float16 else t.view(np.uint32)


def _same(got, want, what):
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


def _draw(gpu, shape, seed, stream=0, box=None, sigma=1.0, dtype=torch.float16, call=None):
    """`ops.philox_normal` into a buffer with canaries on both sides -> the output (the canaries checked)."""
    ops, _ = _ops()
    extent = tuple(shape) if box is None else tuple(box[1])
    nbytes = int(np.prod(extent)) * (2 if dtype == torch.float16 else 4)
    buf = torch.full((CANARY + nbytes + CANARY,), FILL, dtype=torch.uint8, device=gpu)
    out = buf[CANARY:CANARY + nbytes].view(dtype).view(extent)
    try:
        got = (call or ops.philox_normal)(shape, seed, stream, box=box, sigma=sigma, dtype=dtype, device=gpu, out=out)
        assert got is out
    finally:
        torch.cuda.synchronize()
        host = buf.cpu()
        assert bool((host[:CANARY] == FILL).all()) and bool((host[-CANARY:] == FILL).all()), f"{shape} {box}: a canary changed"
    return out


def _want(shape, seed, stream=0, box=None, sigma=1.0, dtype=torch.float16):
    return R.normal(shape, seed, stream, box=box, sigma=sigma, dtype=NP[dtype])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("shape", [RAGGED, EVEN], ids=str)
def test_whole_tensors(gpu, shape, dtype):
    for seed in R.SEEDS:
        for stream in R.STREAMS:
            _same(_draw(gpu, shape, seed, stream, dtype=dtype), _want(shape, seed, stream, dtype=dtype), f"seed {seed:#x} stream {stream:#x}")


def test_headline_tensor_once(gpu):
    _same(_draw(gpu, HEADLINE, 5), _want(HEADLINE, 5), "headline fp16")
    _same(_draw(gpu, HEADLINE, 5, 1, dtype=torch.float32), _want(HEADLINE, 5, 1, dtype=torch.float32), "headline fp32")


@pytest.mark.parametrize("sigma", [1.0, 0.5, 14.6146])
def test_sigma_is_the_half_multiply(gpu, sigma):
    got = _draw(gpu, RAGGED, 3, sigma=sigma)
    _same(got, _want(RAGGED, 3, sigma=sigma), f"sigma {sigma}")
    base = torch.from_numpy(_want(RAGGED, 3))
    base *= sigma                                                       # what `seeded_noise` does to torch's draw
    _same(got, base, f"sigma {sigma} against torch")
    _same(_draw(gpu, RAGGED, 3, sigma=1.0), _draw(gpu, RAGGED, 3, sigma=1), "sigma 1 is the identity")


def _slice(whole, box):
    return whole[tuple(slice(s, s + e) for s, e in zip(*box))]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_boxes_are_slices_of_the_whole(gpu, dtype):
    ops, _ = _ops()
    whole = _want(RAGGED, 7, 3, dtype=dtype)
    boxes = [((0, 0, 0, 0, s), (1, 3, 3, 5, w)) for s in range(6) for w in (1, 3, 5) if s + w <= 7]          # every start at odd widths
    boxes += [((0, 1, 1, 2, s), (1, 2, 2, 3, w)) for s in range(6) for w in (1, 3) if s + w <= 7]            # every axis cut
    boxes += [((0, 0, 1, 0, 0), (1, 3, 2, 5, 7)), ((0, 2, 2, 4, 6), (1, 1, 1, 1, 1)), ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1))]
    for box in boxes:
        _same(_draw(gpu, RAGGED, 7, 3, box=box, dtype=dtype), _slice(whole, box), f"box {box}")
    whole = _want(EVEN, 7, 3, dtype=dtype)
    fast = [((0, 0, 1, 0, 0), (1, 4, 1, 8, 8)), ((0, 1, 0, 4, 4), (1, 3, 2, 4, 4)), ((0, 0, 0, 0, 0), (1, 4, 2, 8, 4))]   # a frame, aligned rows
    slow = [((0, 0, 0, 0, 2), (1, 4, 2, 8, 4)), ((0, 3, 1, 7, 7), (1, 1, 1, 1, 1))]
    for box in fast + slow:
        assert ops.philox_form(EVEN, box) == (box in fast)
        _same(_draw(gpu, EVEN, 7, 3, box=box, dtype=dtype), _slice(whole, box), f"box {box}")
    # two boxes that tile the tensor are one call; a call for B frames is B calls
    lo, hi = _draw(gpu, EVEN, 7, 3, box=((0, 0, 0, 0, 0), (1, 4, 2, 8, 3)), dtype=dtype), _draw(gpu, EVEN, 7, 3, box=((0, 0, 0, 0, 3), (1, 4, 2, 8, 5)), dtype=dtype)
    _same(torch.cat([lo, hi], dim=4), whole, "two boxes")
    frames = [_draw(gpu, EVEN, 7, 3, box=((0, 0, t, 0, 0), (1, 4, 1, 8, 8)), dtype=dtype) for t in range(2)]
    _same(torch.cat(frames, dim=2), _draw(gpu, EVEN, 7, 3, dtype=dtype), "B frames")
    # fewer axes: the same logical indices, the same bits
    _same(_draw(gpu, (315,), 7, 3, dtype=dtype).view(RAGGED), _want(RAGGED, 7, 3, dtype=dtype), "one axis")
    _same(_draw(gpu, (9, 35), 7, 3, box=((2, 1), (3, 33)), dtype=dtype), _slice(_want((9, 35), 7, 3, dtype=dtype), ((2, 1), (3, 33))), "two axes")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_the_counter_s_high_word(gpu, dtype):
    """Logical (1, 1, 1, 3, 2^33 + 9): boxes of 16 elements across i = 2^32, 2^33 and 2^34, where q's bit 30, 31 and 32 first
    turn: the smallest case in which 64-bit index arithmetic and the counter's second word can go wrong."""
    W = 2 ** 33 + 9
    shape = (1, 1, 1, 3, W)
    for at in (2 ** 32, 2 ** 33, 2 ** 34):
        for shift in (8, 11):                                           # block-aligned (the fast form) and not
            row, col = divmod(at - shift, W)
            box = ((0, 0, 0, row, col), (1, 1, 1, 1, 16))
            idx = R.box_indices(shape, box)
            assert int(idx.min()) < at <= int(idx.max())
            _same(_draw(gpu, shape, 9, 2 ** 32, box=box, dtype=dtype), _want(shape, 9, 2 ** 32, box=box, dtype=dtype), f"across {at} - {shift}")
    lo_q, hi_q = _draw(gpu, shape, 9, box=((0, 0, 0, 0, 0), (1, 1, 1, 1, 16)), dtype=dtype), _draw(gpu, shape, 9, box=((0, 0, 0, 1, 2 ** 33 - 9), (1, 1, 1, 1, 16)), dtype=dtype)
    assert not np.array_equal(_bits(lo_q), _bits(hi_q))                 # i and i + 2^34 differ in q's high word alone
    # a seed or a stream that differs in its high word alone
    base = _draw(gpu, EVEN, 1, 1, dtype=dtype)
    for seed, stream in ((1 + 2 ** 32, 1), (1, 1 + 2 ** 32), (1 + 2 ** 63, 1), (1, 1 + 2 ** 63)):
        other = _draw(gpu, EVEN, seed, stream, dtype=dtype)
        _same(other, _want(EVEN, seed, stream, dtype=dtype), f"seed {seed:#x} stream {stream:#x}")
        assert not np.array_equal(_bits(other), _bits(base))


def test_run_to_run(gpu):
    for shape, box in ((HEADLINE, None), (RAGGED, ((0, 1, 1, 2, 3), (1, 2, 2, 3, 3)))):
        a, b = _draw(gpu, shape, 11, 4, box=box), _draw(gpu, shape, 11, 4, box=box)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_refusals_launch_nothing(gpu):
    ops, VdxError = _ops()
    for kw in (dict(box=((0, 0, 0, 0, 0), (1, 4, 2, 8, 9))), dict(box=((0, 0, 0, 0, 1), (1, 4, 2, 8, 8))), dict(seed=2 ** 64), dict(stream=-1),
               dict(sigma=float("inf")), dict(sigma=float("nan"))):
        def refused(shape, seed, stream, **rest):
            with pytest.raises((VdxError, ValueError)):
                ops.philox_normal(**{**dict(shape=shape, seed=seed, stream=stream), **rest, **kw})
            return rest["out"]
        out = _draw(gpu, EVEN, 1, call=refused)
        assert bool((out.view(torch.uint8) == FILL).all()), f"{kw}: the output was written"
    for bad in (torch.empty(EVEN, dtype=torch.float16), torch.empty(EVEN, dtype=torch.float32, device=gpu),
                torch.empty((1, 4, 2, 8, 16), dtype=torch.float16, device=gpu)[..., ::2], torch.empty((4, 2, 8, 8), dtype=torch.float16, device=gpu)):
        with pytest.raises(VdxError):
            ops.philox_normal(EVEN, 1, device=gpu, out=bad)
    odd = torch.empty(8 + EVEN[1] * 128, dtype=torch.float16, device=gpu)[4:4 + EVEN[1] * 128].view(EVEN)     # 8 bytes off
    with pytest.raises(VdxError, match="aligned"):
        ops.philox_normal(EVEN, 1, device=gpu, out=odd)


def test_miner_start_latent(gpu):
    from vdx.miner import seeded_latent
    seed, shape = 0x0123456789ABCDEF, (1, 4, 6, 8, 8)
    whole = seeded_latent(seed, shape, gpu)
    assert whole.dtype == torch.float16 and tuple(whole.shape) == shape and whole.is_contiguous()
    _same(whole, _want(shape, seed), "the miner's latent")
    _same(seeded_latent(seed, shape, gpu, frames=(0, 1)), whole[:, :, 0:1], "frame 0 alone")
    _same(seeded_latent(seed, shape, gpu, frames=(2, 5)), whole[:, :, 2:5], "frames 2..4")


# ---- the job ----------------------------------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 8, 32, 32, 2
SEED = 5
LATENT = (1, 4, T, HL, WL)


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    return build(gpu, 0, 1)


def _diffuser(model, **kw):
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    extra = {k: kw.pop(k) for k in ("init_latents", "latent_mask") if k in kw}
    kw = {**dict(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx", device="cuda"), **kw}
    return DistributedVideoDiffuser(DiffuserConfig(**kw), m, DDIMScheduler(), emb[1:], emb[:1], **extra)


@pytest.fixture(scope="module")
def base(gpu):
    """The restatement's base noise of the job's latent, on the GPU."""
    return torch.from_numpy(_want(LATENT, SEED)).to(gpu)


def _by_hand(monkeypatch, base):
    """The torch job handed `base` as its seeded noise."""
    import vdx.pipeline as P
    monkeypatch.setattr(P, "seeded_noise", lambda shape, sigma, device, noise_device=None, dtype=torch.float16: (base * sigma).to(device))


def test_start_latent_and_context(gpu, model, base):
    from vdx.pipeline import seeded_noise
    _same(seeded_noise(LATENT, 1.0, "cuda", seed=SEED), base, "the start latent")
    sigma = 14.6146
    _same(seeded_noise(LATENT, sigma, "cuda", None, torch.float16, seed=SEED), _want(LATENT, SEED, sigma=sigma), "the start latent times sigma")
    d = _diffuser(model, noise="philox", seed=SEED)
    _same(d.ctx, base.mean(dim=2, keepdim=True), "ctx")
    assert not torch.equal(_diffuser(model, noise="philox").ctx, d.ctx)           # seed 0 is another latent
    state = torch.random.get_rng_state()
    _diffuser(model, noise="philox", seed=SEED)
    assert torch.equal(torch.random.get_rng_state(), state)                        # torch's global generator is left alone


@pytest.mark.parametrize("windows", ["one", "two"])
def test_job_is_the_job_handed_that_latent(gpu, model, base, monkeypatch, windows):
    kw = dict(mode="fsdp") if windows == "one" else {}                  # "fsdp": the whole clip is one window
    lat, info = _diffuser(model, noise="philox", seed=SEED, **kw)()
    assert info["noise"] == {"generator": "philox4x32-10/v1", "seed": SEED} and len(info["ranges"]) == (1 if windows == "one" else 2)
    _by_hand(monkeypatch, base)
    want, info0 = _diffuser(model, **kw)()
    assert "noise" not in info0 and set(info) == set(info0) | {"noise"}
    assert torch.equal(lat.view(torch.int32), want.view(torch.int32))


def test_free_init_and_posterior_streams(gpu, model, base, monkeypatch, tmp_path):
    import vdx.pipeline as P
    from vdx import freeinit
    _same(P.iteration_noise(LATENT, 2, "cuda", seed=SEED), _want(LATENT, SEED, 2, dtype=torch.float32), "iteration 2")
    d = _diffuser(model, noise="philox", seed=SEED, free_init_iters=2)
    d()
    filt = freeinit.lowpass_filter(LATENT[2:], d.cfg.free_init_method, d.cfg.free_init_spatial, d.cfg.free_init_temporal, d.cfg.free_init_order)
    # the second pass's start: the first pass's blend re-noised with the base stream and mixed with stream 1
    d1 = _diffuser(model, noise="philox", seed=SEED)
    out, _ = d1()
    z_T = d1.scheduler.add_noise(out.to(gpu, torch.float16).contiguous(), base, 999)
    eta = torch.from_numpy(_want(LATENT, SEED, 1, dtype=torch.float32)).to(gpu)
    _same(d.free_init_starts[0], freeinit.freq_mix(z_T, eta, filt.to(gpu)), "FreeInit's start of iteration 1")

    # the posterior sample: stream 2^32 over (T, 4, h, w), handed to the encoder
    class Vae:
        cfg, seen = None, None

        def load_diffusers_encoder_state_dict(self, sd, device):
            pass

        def encode_frames_u8(self, frames, posterior, noise):
            Vae.seen = noise
            return torch.zeros(LATENT, dtype=torch.float16, device=frames.device)
    import vdx.weights as W
    monkeypatch.setattr(W, "synthetic_vae_encoder_state_dict", lambda *a, **k: {})
    clip = tmp_path / "clip.npy"
    np.save(clip, np.zeros((T, HL * 8, WL * 8, 3), dtype=np.uint8))
    cfg = P.DiffuserConfig(num_frames=T, height=HL * 8, width=WL * 8, init_video=str(clip), model_id="none", noise="philox", seed=SEED)
    P.encode_init_video(cfg, Vae(), gpu)
    _same(Vae.seen, _want((T, 4, HL, WL), SEED, 2 ** 32), "the posterior sample")
    cfg.noise, cfg.seed = "torch", None
    P.encode_init_video(cfg, Vae(), gpu)
    assert not np.array_equal(_bits(Vae.seen), _want((T, 4, HL, WL), SEED, 2 ** 32).view(np.uint16))


def test_masked_job_keeps_its_base(gpu, model, base, monkeypatch):
    g = torch.Generator().manual_seed(3)
    clean = torch.randn(LATENT, generator=g).half().to(gpu)
    keep = torch.ones(T, HL, WL, dtype=torch.uint8)
    keep[:3] = 0
    keep[:, :8, :8] = 0
    extra = dict(init_latents=clean, latent_mask=keep.to(gpu), steps=4, strength=0.75)
    d = _diffuser(model, noise="philox", seed=SEED, **extra)
    _same(d._base, base, "the masked job's base")
    lat, info = d()
    _same(d._base, base, "the base after the job")
    _by_hand(monkeypatch, base)
    want, _ = _diffuser(model, **extra)()
    assert torch.equal(lat.view(torch.int32), want.view(torch.int32)) and info["noise"]["seed"] == SEED


def test_records_only_when_set(gpu, model):
    from vdx.options import noise_record, resolve
    from vdx.pipeline import DiffuserConfig
    _, info = _diffuser(model, noise="philox")()
    assert info["noise"] == {"generator": "philox4x32-10/v1", "seed": 0}
    _, info0 = _diffuser(model)()
    assert "noise" not in info0 and noise_record(info0) == {} and noise_record(info) == {"noise": info["noise"]}
    assert resolve(DiffuserConfig(), job=True).noise is None
    with pytest.raises(ValueError, match="needs noise"):
        _diffuser(model, seed=SEED)()
