"""-m gpu: LoRA adapters through the job (vdx/pipeline.py `run_job`, `--lora`) on `synthetic:tiny`: 8 frames, chunk 6, overlap 2, 2
steps, 128x128.  Bit for bit: the job with `lora=((path, 0.8),)` against the job without the option on a passed pipe whose UNet and
text-encoder state dicts were merged by hand on the CPU (tests/lora_ref.py), plain, co-denoised and with DPM-Solver++; the record;
two `--lora` flags; two ranks against one (two fresh processes on one GPU, tests/dist_lora_worker.py); the sharded UNet against the
resident one, and the refusal of a change of adapters after `shard_`."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lora_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu
SCALE = 0.8
B = "transformer_blocks.0"
UNET_MODS = [f"down_blocks.0.attentions.0.{B}.attn1.to_q", f"down_blocks.0.attentions.0.{B}.attn2.to_v", f"down_blocks.0.temp_attentions.0.{B}.attn1.to_k",
             f"mid_block.attentions.0.{B}.ff.net.0.proj", f"up_blocks.1.attentions.0.{B}.ff.net.2", "up_blocks.3.attentions.2.proj_out",
             "transformer_in.proj_in", "down_blocks.0.resnets.0.conv1", "mid_block.temp_convs.0.conv2.3"]
TEXT_MODS = ["encoder.layers.0.self_attn.q_proj", "encoder.layers.1.mlp.fc2"]


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def files(gpu, tmp_path_factory):
    """Two seeded adapter files, one per key convention, and the tiny models' configs."""
    import vdx  # noqa: F401
    from safetensors.torch import save_file
    from vdx import lora
    from vdx.compat.diffusers_shim import DiffusionPipeline
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    ucfg, tcfg = pipe.unet.cfg, pipe.text_encoder.cfg
    us, ts = lora.targets("unet", ucfg), lora.targets("text_encoder", tcfg)
    d = tmp_path_factory.mktemp("lora")
    paths = {}
    for name, seed, conv, rank in (("style", 51, "kohya", 4), ("motion", 52, "peft", 2)):
        parts = {("unet", m): v for m, v in L.seeded_adapter(us, UNET_MODS, rank, seed, magnitude=0.3, alpha=2.0).items()}
        parts.update({("text_encoder", m): v for m, v in L.seeded_adapter(ts, TEXT_MODS, rank, seed + 100, magnitude=0.3).items()})
        sd = L.adapter_file_dict(parts, conv)
        if conv == "kohya":
            paths[name] = str(d / f"{name}.safetensors")
            save_file({k: v.contiguous() for k, v in sd.items()}, paths[name])
        else:
            paths[name] = str(d / f"{name}.pt")
            torch.save(sd, paths[name])
    return dict(paths=paths, ucfg=ucfg, tcfg=tcfg)


def _hand_pipe(files, pairs):
    """A pipe whose UNet and text encoder were loaded from state dicts merged by hand on the CPU."""
    from vdx import lora, weights
    from vdx.compat.diffusers_shim import DiffusionPipeline
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    ads = [(lora.read_lora(files["paths"][n], unet_cfg=files["ucfg"], text_cfg=files["tcfg"]), s) for n, s in pairs]
    pipe.unet.load_diffusers_state_dict(L.hand_merge(weights.synthetic_state_dict(files["ucfg"], 1234, "cpu"), "unet", ads), device="cpu")
    pipe.text_encoder.load_transformers_state_dict(L.hand_merge(weights.synthetic_clip_state_dict(files["tcfg"], 11, "cpu"), "text_encoder", ads),
                                                   device="cpu")
    return pipe


def _cfg(**kw):
    from dist_lora_worker import JOB
    from vdx.pipeline import DiffuserConfig
    return DiffuserConfig(**{**JOB, **kw})


@pytest.mark.parametrize("extra", [{}, {"co_denoise": True}, {"scheduler": "dpmpp_2m"}], ids=["windowed", "co_denoise", "dpmpp_2m"])
def test_job_equals_the_job_on_hand_merged_weights(gpu, files, extra):
    from dist_lora_worker import run
    lat, res = run(_cfg(lora=((files["paths"]["style"], SCALE),), **extra))
    want, res0 = run(_cfg(**extra), pipe=_hand_pipe(files, [("style", SCALE)]))
    assert torch.equal(_bits(lat), _bits(want))
    assert "lora" not in res0 and set(res) == set(res0) | {"lora"}
    assert res["lora"] == [{"name": "style", "scale": SCALE, "rank": 4, "unet_modules": len(UNET_MODS), "text_modules": len(TEXT_MODS)}]
    if not extra:
        plain, _ = run(_cfg())
        assert not torch.equal(_bits(plain), _bits(lat))                 # the adapter moved the job


def test_cli_takes_two_lora_flags(gpu, files):
    from dist_lora_worker import run
    from vdx.pipeline import build_arg_parser, config_from_args
    base = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "128", "--chunk_size", "6",
            "--overlap", "2", "--noise_device", "cpu", "--prompt", "a forest"]
    p = files["paths"]
    cfg = config_from_args(build_arg_parser().parse_args(base + ["--lora", p["style"], "0.8", "--lora", p["motion"], "-0.5"]))
    assert cfg.lora == ((p["style"], 0.8), (p["motion"], -0.5))
    lat, res = run(cfg)
    want, _ = run(config_from_args(build_arg_parser().parse_args(base)), pipe=_hand_pipe(files, [("style", 0.8), ("motion", -0.5)]))
    assert torch.equal(_bits(lat), _bits(want))
    assert [(r["name"], r["scale"], r["rank"]) for r in res["lora"]] == [("style", 0.8, 4), ("motion", -0.5, 2)]
    zero, resz = run(config_from_args(build_arg_parser().parse_args(base + ["--lora", p["style"], "0.8", "--lora", p["motion"], "0"])))
    one, _ = run(config_from_args(build_arg_parser().parse_args(base + ["--lora", p["style"], "0.8"])))
    assert torch.equal(_bits(zero), _bits(one)) and len(resz["lora"]) == 2        # weight 0: recorded, and the base for that adapter
    with pytest.raises(ValueError, match="not a local file"):
        run(config_from_args(build_arg_parser().parse_args(base + ["--lora", p["style"] + ".missing", "1"])))


LIMIT_S = 300


def test_two_ranks_end_with_the_bits_of_one(gpu, files, tmp_path):
    """Windows (0, 6) and (4, 8), one per rank; each rank merges the adapter for itself and then shards its UNet.  The worker checks
    that both ranks hold identical bits; the test starts the two ranks itself, each under its own time limit, and nothing else."""
    from dist_lora_worker import run
    out = tmp_path / "rank0.pt"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "dist_lora_worker.py"), str(out), files["paths"]["style"], str(SCALE)]
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29791", VDX_SHARE_GPU="1", VDX_DIST_BACKEND="gloo")
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
    lat, res = run(_cfg(lora=((files["paths"]["style"], SCALE),)))
    assert got["world_size"] == 2 and res["world_size"] == 1 and got["lora"] == res["lora"]
    assert torch.equal(got["lat"].view(torch.int32), _bits(lat))


def test_sharded_unet_equals_the_resident_one_and_refuses_a_change(gpu, files):
    from vdx._lib import VdxError
    from vdx.compat.diffusers_shim import DiffusionPipeline
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16).to(gpu)
    pipe.load_lora_weights(files["paths"]["style"], adapter_name="style")
    g = torch.Generator().manual_seed(4)
    x, e = torch.randn(2, 4, 4, 16, 16, generator=g).half().to(gpu), torch.randn(2, 77, 128, generator=g).half().to(gpu)
    resident = pipe.unet(x, 7, encoder_hidden_states=e).sample.clone()
    pipe.unet.shard_(0, 1)
    sharded = pipe.unet(x, 7, encoder_hidden_states=e).sample
    assert torch.equal(sharded.view(torch.int16), resident.view(torch.int16))
    for change in (lambda: pipe.load_lora_weights(files["paths"]["motion"], adapter_name="motion"), lambda: pipe.set_adapters("style", 0.5),
                   lambda: pipe.unload_lora_weights(), lambda: pipe.unfuse_lora()):
        with pytest.raises(VdxError, match="shard"):
            change()
    assert pipe.get_active_adapters() == ["style"]
    assert torch.equal(pipe.unet(x, 7, encoder_hidden_states=e).sample.view(torch.int16), resident.view(torch.int16))
