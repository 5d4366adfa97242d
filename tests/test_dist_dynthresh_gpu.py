"""Dynamic thresholding across ranks (tests/dist_dynthresh_worker.py): two processes, one rank each, both on this box's one GPU and
talking over gloo, co-denoised, against the job of one rank, bit for bit: every rank forms the same channel statistics from the
same gathered buffer, with no collective added."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, STEPS, GS, MS, Q = 8, 3, 15.0, 7.0, 0.995
RANGES = [(0, 6), (4, 8)]


def test_two_ranks_end_with_the_bits_of_one(gpu, tmp_path):
    """The child has its own time limit."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29767", os.path.join(ROOT, "tests", "dist_dynthresh_worker.py"), str(out), str(T), "6", "2",
                        str(STEPS), "dpmpp_2m", str(GS), str(MS), str(Q)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
    got = torch.load(out, weights_only=True)
    m, emb = build(gpu, 0, 1)
    cfg = DiffuserConfig(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=256, width=256, mode="hybrid_ctx", device="cuda",
                         noise_device="cpu", scheduler="dpmpp_2m", co_denoise=True, guidance_scale=GS, cfg_mimic=MS,
                         cfg_mimic_percentile=Q)
    lat, _ = DistributedVideoDiffuser(cfg, m, make_scheduler("dpmpp_2m", DDIMScheduler()), emb[1:], emb[:1])()
    assert got["ranges"] == RANGES and got["world_size"] == 2 and got["cfg_mimic"] == {"scale": MS, "percentile": Q}
    assert torch.equal(got["lat"].view(torch.int32), lat.cpu().view(torch.int32))
