"""-m gpu: weighted and long prompts through the job (vdx/pipeline.py, vdx/prompt.py) on the tiny synthetic pipeline: 8 frames, chunk 6,
overlap 2, 2 steps, 128x128.  A 100-token weighted prompt under "a1111" reaches the UNet as 154 rows, differs from "plain", and
equals a `DistributedVideoDiffuser` driven by hand with `encode_texts`' output; a short prompt without emphasis gives "plain"'s
frames and file byte for byte; a weighted prompt with a weighted negative prompt, windowed and co-denoised under DPM-Solver++,
equals a Python loop over the planner's windows with embeddings made by hand (tests/prompt_ref.py on the CPU), bit for bit; two
ranks equal one (two fresh processes on this box's one GPU, tests/dist_prompt_worker.py); a long `--prompt_at` key and a long
`--region` text each run and carry the job's chunk count in the record."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prompt_ref as R  # noqa: E402
from dist_prompt_worker import JOB, LONG, NEGATIVE, run  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = JOB["num_frames"]


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.fixture(scope="module")
def pipe(gpu):
    import vdx  # noqa: F401
    from vdx.compat.diffusers_shim import DiffusionPipeline
    return DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)


def _cfg(**kw):
    from vdx.pipeline import DiffuserConfig
    return DiffuserConfig(**{**JOB, **kw})


def _hand_embeddings(pipe, texts, gpu):
    """The texts' embeddings made without vdx/prompt.py and without the kernel: tests/prompt_ref.py parses, chunks and weights (on the
    CPU), the pipeline's text encoder encodes.  -> fp16 (n_texts, 77 k, D) on the GPU."""
    tok = pipe.tokenizer
    ids_of = lambda s: tok(s, add_special_tokens=False, truncation=False, padding=False, return_tensors=None).input_ids     # noqa: E731
    per = [R.chunks(R.parse(t), ids_of, tok.bos_token_id, tok.eos_token_id, tok.eos_token_id, ids_of(",")[0]) for t in texts]
    k = max(i.shape[0] for i, _, _ in per)
    eid, ew, _ = R.chunks(R.parse(""), ids_of, tok.bos_token_id, tok.eos_token_id, tok.eos_token_id, ids_of(",")[0])
    ids = torch.cat([torch.cat([i] + [eid] * (k - i.shape[0])) for i, _, _ in per])
    wts = torch.cat([torch.cat([w] + [ew] * (k - w.shape[0])) for _, w, _ in per])
    with torch.no_grad():
        z = pipe.text_encoder(ids.to(gpu))[0].half().cpu()
    assert bool(R.sums_are_exact(z, wts).all())                      # the restatement's sums do not depend on their order here
    out = z.clone()
    on = (wts != 1.0).any(dim=1)
    out[on] = R.weight(z[on], wts[on])
    return out.reshape(len(texts), k * 77, -1).to(gpu), k


def _diffuser(pipe, cfg, emb):
    from vdx.pipeline import DistributedVideoDiffuser, make_scheduler
    return DistributedVideoDiffuser(cfg, pipe.unet, make_scheduler(cfg.scheduler, pipe.scheduler), emb[1:2].contiguous(), emb[:1].contiguous())


def test_a_100_token_prompt_reaches_the_unet_as_154_rows(gpu, pipe):
    """Fails on the parent: the option does not exist there and its UNet refuses 154 rows."""
    from vdx.prompt import encode_texts
    lat, res, texts = run(_cfg(), pipe)
    assert texts == {(2, 154, 128)}
    assert res["prompt_syntax"] == {"syntax": "a1111", "chunks": 2, "tokens": [100, 4], "weighted": True} and list(res)[-1] == "prompt_syntax"
    plain, res0, texts0 = run(_cfg(prompt_syntax="plain"), pipe)
    assert texts0 == {(2, 77, 128)} and "prompt_syntax" not in res0 and set(res) == set(res0) | {"prompt_syntax"}
    assert bool(torch.isfinite(lat).all()) and not torch.equal(_bits(lat), _bits(plain))
    emb = encode_texts(pipe, [LONG, NEGATIVE], "a1111", gpu)
    assert tuple(emb.shape) == (2, 154, 128) and emb.dtype == torch.float16
    by_hand, _ = _diffuser(pipe, _cfg(), emb)()
    assert torch.equal(_bits(lat), _bits(by_hand))
    hand_emb, k = _hand_embeddings(pipe, [LONG, NEGATIVE], gpu)
    assert k == 2 and torch.equal(_bits(emb), _bits(hand_emb))       # the kernel and the chunker against the restatement, end to end


def test_a_short_plain_prompt_is_plain_byte_for_byte(gpu, pipe, tmp_path):
    from vdx.pipeline import run_job
    files = {}
    for syntax in ("plain", "a1111"):
        got = {}
        path = str(tmp_path / f"{syntax}.mp4")
        res = run_job(_cfg(prompt="a rocket in space, 4k", negative_prompt="", prompt_syntax=syntax), out_video=path, pipe=pipe, clip_inputs=got)
        files[syntax] = (np.stack(got["frames"]), open(path, "rb").read(), res)
    assert np.array_equal(files["plain"][0], files["a1111"][0]) and files["plain"][1] == files["a1111"][1] and len(files["plain"][1]) > 0
    assert files["a1111"][2]["prompt_syntax"] == {"syntax": "a1111", "chunks": 1, "tokens": [5, 0], "weighted": False}
    # 75 tokens, still one chunk, still the plain job; one more and "plain" truncates while "a1111" does not
    edge = " ".join(f"w{j}" for j in range(75))
    a, _, ta = run(_cfg(prompt=edge, negative_prompt=""), pipe)
    b, _, tb = run(_cfg(prompt=edge, negative_prompt="", prompt_syntax="plain"), pipe)
    assert ta == tb == {(2, 77, 128)} and torch.equal(_bits(a), _bits(b))


def _windowed_loop(d, text):
    from vdx import ops
    from vdx.pipeline import seeded_noise
    start = seeded_noise(d.latent_shape, d.scheduler.init_noise_sigma, "cuda", "cpu")
    chunks = []
    for s, e in d.plan().ranges:
        lat = start[:, :, s:e].clone().contiguous()
        d.scheduler.reset()
        for t in d.schedule:
            noise = d.unet(ops.cfg_input(lat, d.ctx, d.cfg.context_weight), t, encoder_hidden_states=text).sample
            lat = d.scheduler.step_cfg(noise, t, lat, d.cfg.guidance_scale)
        chunks.append((s, e, lat))
    return d.blend(chunks, start, d.plan().overlap)


def _co_loop(d, text, gpu):
    from vdx import ops
    from vdx.codenoise import window_table
    from vdx.pipeline import seeded_noise
    cfg, sched, cp = d.cfg, d.scheduler, d.plan()
    table = window_table(cp, T)
    slot = 2 * 4 * cp.chunk * (cfg.height // 8) * (cfg.width // 8)
    rows, wn = table.rows(1, cp.per_rank, slot), table.wn.to(gpu)
    packed = torch.zeros((cp.per_rank, slot), dtype=torch.float16, device=gpu)
    z = seeded_noise(d.latent_shape, sched.init_noise_sigma, "cuda", "cpu").clone()
    sched.reset()
    for t in d.schedule:
        for j, (s, e) in enumerate(cp.ranges):
            noise = d.unet(ops.cfg_input_window(z, d.ctx, cfg.context_weight, s, e), t, encoder_hidden_states=text).sample
            packed[j, :noise.numel()].copy_(noise.reshape(-1))
        z = sched.step_cfg_windows(packed, rows, wn, t, z, cfg.guidance_scale)
    return z.float()


@pytest.mark.parametrize("co", [False, True], ids=["windowed", "co_denoise"])
def test_weighted_prompts_under_dpm_are_the_loop_with_hand_made_embeddings(gpu, pipe, co):
    kw = dict(scheduler="dpmpp_2m", co_denoise=co)
    lat, res, texts = run(_cfg(**kw), pipe)
    assert texts == {(2, 154, 128)} and res["scheduler"] == "dpmpp_2m" and ("co_denoise" in res) == co
    emb, _ = _hand_embeddings(pipe, [LONG, NEGATIVE], gpu)
    d = _diffuser(pipe, _cfg(**kw), emb)
    text = torch.cat([emb[1:2], emb[:1]]).contiguous()              # (negative, prompt): the job's CFG order
    want = _co_loop(d, text, gpu) if co else _windowed_loop(d, text)
    assert bool(torch.isfinite(lat).all()) and torch.equal(_bits(lat.float()), _bits(want.float()))
    unweighted, _, _ = run(_cfg(prompt=LONG.replace(":1.3", ":1.0"), **kw), pipe)
    assert not torch.equal(_bits(unweighted), _bits(lat))            # the weight shows in the latent


LIMIT_S = 300


def test_two_ranks_end_with_the_bits_of_one(gpu, pipe, tmp_path):
    """Windows (0, 6) and (4, 8), one per rank; every rank encodes the texts for itself.  The worker checks that both ranks hold
    identical bits and that its UNet received 154 rows.  The test starts the two ranks itself, each under its own time limit."""
    out = tmp_path / "rank0.pt"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "dist_prompt_worker.py"), str(out)]
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29791", VDX_SHARE_GPU="1", VDX_DIST_BACKEND="gloo")
    logs = [open(tmp_path / f"rank{r}.log", "w+") for r in range(2)]    # files, not pipes: a rank never blocks on its output
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=logs[r], stderr=subprocess.STDOUT) for r in range(2)]
    try:
        for p in procs:
            p.wait(timeout=LIMIT_S)
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
    lat, res, _ = run(_cfg(), pipe)
    assert got["world_size"] == 2 and got["prompt_syntax"] == res["prompt_syntax"]
    assert torch.equal(got["lat"].view(torch.int32), lat.float().cpu().view(torch.int32))


def test_long_travel_keys_and_region_texts_share_the_chunk_count(gpu, pipe, tmp_path):
    long_key = "a (desert:1.4) at dusk , " + " ".join(f"sand{j}" for j in range(180))       # 185 tokens: three chunks
    lat, res, texts = run(_cfg(prompt="a forest", negative_prompt="", prompt_travel=((5, long_key),)), pipe)
    assert texts == {(2, 6, 231, 128), (2, 4, 231, 128)}             # per-frame text, every text of the job at 3 x 77 rows
    assert res["prompt_syntax"] == {"syntax": "a1111", "chunks": 3, "tokens": [2, 0, 2, 185], "weighted": True}
    assert res["prompt_travel"]["keys"][1][0] == 5 and bool(torch.isfinite(lat).all())
    short, _, _ = run(_cfg(prompt="a forest", negative_prompt="", prompt_travel=((5, "a (desert:1.4) at dusk"),)), pipe)
    assert not torch.equal(_bits(short), _bits(lat))                 # the tokens past 75 are not dropped
    mask = np.zeros((128, 128), np.uint8)
    mask[:, :64] = 255
    np.save(tmp_path / "left.npy", mask)
    long_region = "a [grey] wall , " + " ".join(f"brick{j}" for j in range(96))             # 100 tokens: two chunks
    lat2, res2, texts2 = run(_cfg(prompt="a forest", negative_prompt="", regions=((str(tmp_path / "left.npy"), long_region),)), pipe)
    assert texts2 == {(2, 154, 128)} and res2["regions"]["count"] == 1
    assert res2["prompt_syntax"] == {"syntax": "a1111", "chunks": 2, "tokens": [2, 0, 100], "weighted": True}
    assert bool(torch.isfinite(lat2).all())
    with pytest.raises(ValueError, match="tokens make"):
        run(_cfg(prompt=" ".join(f"w{j}" for j in range(301))), pipe)
