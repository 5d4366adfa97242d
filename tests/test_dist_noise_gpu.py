"""The seeded noise across ranks (tests/dist_noise_worker.py): two processes, one rank each, both on this box's one GPU and talking
over gloo, against the job of one rank, bit for bit: every rank draws the start latent from the seed alone, with no broadcast of its
own, and the latent it draws is the restatement's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import noise_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, STEPS, SEED = 8, 2, 0x0123456789ABCDEF
RANGES = [(0, 6), (4, 8)]


def test_two_ranks_end_with_the_bits_of_one(gpu, tmp_path, co=0):
    """The windowed job (`co` 1: co-denoised, for a run by hand).  The child has its own time limit."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, seeded_noise
    from vdx.scheduler import DDIMScheduler
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29771", os.path.join(ROOT, "tests", "dist_noise_worker.py"), str(out), str(T), "6", "2",
                        str(STEPS), str(SEED), str(co)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
    got = torch.load(out, weights_only=True)
    m, emb = build(gpu, 0, 1)
    cfg = DiffuserConfig(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=256, width=256, mode="hybrid_ctx", device="cuda",
                         noise="philox", seed=SEED, co_denoise=bool(co))
    d = DistributedVideoDiffuser(cfg, m, DDIMScheduler(), emb[1:], emb[:1])
    start = seeded_noise(d.latent_shape, 1.0, "cuda", seed=SEED).cpu().numpy()
    assert np.array_equal(start.view(np.uint16), R.normal(d.latent_shape, SEED).view(np.uint16))
    lat, _ = d()
    assert got["ranges"] == RANGES and got["world_size"] == 2 and got["noise"] == {"generator": "philox4x32-10/v1", "seed": SEED}
    assert torch.equal(got["lat"].view(torch.int32), lat.cpu().view(torch.int32))
