"""-m gpu: the looping co-denoised job (vdx/codenoise.py `loop_plan`) on two ranks against one: two fresh processes, one rank
each, both on this box's one GPU and talking over gloo (tests/test_dist_gpu.py's arrangement; tests/dist_coloop_worker.py)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HL, WL, STEPS = 8, 32, 32, 2                                     # the worker's 256 x 256 frame


def test_two_ranks_end_with_the_bits_of_one(gpu, tmp_path):
    """A ring plan that is the same for one rank and for two: 8 frames, chunk 6, overlap 2 -> windows (0, 6) and (4, 10); rank 1
    runs the window that wraps.  The worker itself checks that both ranks hold identical bits."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    from vdx.codenoise import loop_plan
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    assert loop_plan(T, 1, 6, 2).ranges == loop_plan(T, 2, 6, 2).ranges == ((0, 6), (4, 10))
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29749",
                        os.path.join(ROOT, "tests", "dist_coloop_worker.py"), str(out), str(T), "6", "2", str(STEPS), "dpmpp_2m"],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
    got = torch.load(out, weights_only=True)
    m, emb = build(gpu, 0, 1)
    cfg = DiffuserConfig(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", scheduler="dpmpp_2m", co_denoise=True, loop=True)
    lat, info = DistributedVideoDiffuser(cfg, m, make_scheduler("dpmpp_2m", DDIMScheduler()), emb[1:], emb[:1])()
    assert torch.equal(got["lat"].view(torch.int32), lat.cpu().view(torch.int32))
    gi = got["info"]
    assert [tuple(x) for x in gi["ranges"]] == [(0, 6), (4, 8)] == [tuple(x) for x in info["ranges"]] and gi["world_size"] == 2
    assert gi["loop"] == info["loop"] == {"windows": [[0, 6], [4, 6]]}
    per_step = 1 * 1 * (2 * 4 * 6 * HL * WL) * 2                     # (world-1) x per_rank x slot halves x 2 bytes
    assert gi["co_denoise"]["bytes_per_step"] == per_step and gi["network_bytes"] == STEPS * per_step
    assert gi["co_denoise"]["windows"] == 2 and gi["co_denoise"]["steps"] == STEPS and gi["co_denoise"]["exchange_s"] > 0
    assert gi["payload_bytes"] == STEPS * 6 * 4 * 2                  # rank 0's window (0, 6), every step
    if got["gathers"] is not None:
        assert got["gathers"] > 0                                    # the parameters were sharded and gathered
