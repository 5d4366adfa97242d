"""The stochastic sampler across ranks (tests/dist_sde_worker.py): two processes, one rank each, both on this box's one GPU and
talking over gloo, against the job of one rank, bit for bit: a chunk draws the clip's noise at its own frames, so it does not matter
which rank denoises it."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, STEPS, SEED = 8, 2, 0x0123456789ABCDEF
RANGES = [(0, 6), (4, 8)]


def test_two_ranks_end_with_the_bits_of_one(gpu, tmp_path):
    """The windowed job with eta = 1.  The child has its own port and time limit."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29783", os.path.join(ROOT, "tests", "dist_sde_worker.py"), str(out), str(T), "6", "2",
                        str(STEPS), str(SEED)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
    got = torch.load(out, weights_only=True)
    m, emb = build(gpu, 0, 1)
    cfg = DiffuserConfig(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=256, width=256, mode="hybrid_ctx", device="cuda",
                         noise="philox", seed=SEED, eta=1.0)
    lat, _ = DistributedVideoDiffuser(cfg, m, DDIMScheduler(), emb[1:], emb[:1])()
    assert got["ranges"] == RANGES and got["world_size"] == 2 and got["sampler_noise"] == {"eta": 1.0, "algorithm": "ddim"}
    assert torch.equal(got["lat"].view(torch.int32), lat.cpu().view(torch.int32))
