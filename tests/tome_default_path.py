"""The default path's workloads for tests/test_tome_default_gpu.py and tools/tome_record_default.py: the tiny golden forwards
(tests/golden/unet_tiny_{a,b}.npz) and the tiny chunked denoising job (tests/golden/denoise_tiny.npz), as tests/test_unet_gpu.py
runs them, each with the sequence of library entry points it launches and the sha256 of its output bytes.

tests/golden/tome_default_launches.json holds what these gave on the commit BEFORE token merging existed (written by
tools/tome_record_default.py on an MI355X): with token merging never enabled, or enabled and disabled again, they must give
the same sequence and the same bytes."""
import hashlib
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "tome_default_launches.json")
TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
WORKLOADS = ("unet_tiny_a", "unet_tiny_b", "denoise_tiny")


def tiny_model(gpu):
    import vdx  # noqa: F401
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from oracle.unet3d_ref import UNet3DConfig as RefCfg, synthetic_state_dict
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    cfg = UNet3DConfig(block_out_channels=TINY["ch"], cross_attention_dim=TINY["cross"], transformer_in_heads=TINY["in_heads"])
    return UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)


def record(fn):
    """fn() with `ops._launch` wrapped -> (fn's result, the symbols launched, in order)."""
    from vdx import ops
    seen, real = [], ops._launch

    def spy(symbol, *args):
        seen.append(symbol)
        return real(symbol, *args)
    ops._launch = spy
    try:
        out = fn()
    finally:
        ops._launch = real
    return out, seen


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(name, m, gpu):
    """One workload on model m -> (output on the host, launched symbols)."""
    if name.startswith("unet_tiny_"):
        gold = np.load(os.path.join(GOLD, name + ".npz"))
        F, H, W, t = (int(v) for v in gold["shape"])
        g = torch.Generator().manual_seed(7)
        sample = torch.randn(2, 4, F, H, W, generator=g).half().to(gpu)
        ehs = torch.randn(2, 77, TINY["cross"], generator=g).half().to(gpu)
        out, seen = record(lambda: m(sample, torch.tensor(t, device=gpu), encoder_hidden_states=ehs).sample)
        return out.cpu(), seen
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    gold = np.load(os.path.join(GOLD, "denoise_tiny.npz"))
    T, H, W, steps = int(gold["T"]), int(gold["H"]), int(gold["W"]), int(gold["steps"])
    emb = torch.randn(2, 77, TINY["cross"], generator=torch.Generator().manual_seed(1)).half().to(gpu)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=6, overlap=2, height=H * 8, width=W * 8, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu")
    d = DistributedVideoDiffuser(cfg, m, DDIMScheduler(), emb[1:], emb[:1])
    (lat, _), seen = record(lambda: d())
    return lat.cpu(), seen


def pack(seen):
    """The sequence run-length encoded: [[symbol, count], ...]."""
    runs = []
    for s in seen:
        if runs and runs[-1][0] == s:
            runs[-1][1] += 1
        else:
            runs.append([s, 1])
    return runs
