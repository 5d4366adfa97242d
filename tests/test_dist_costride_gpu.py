"""-m gpu: the co-denoised job with strided context windows (vdx/codenoise.py `stride_plan`) on two ranks against one: two fresh
processes, one rank each, both on this box's one GPU and talking over gloo (tests/dist_costride_worker.py).  The test starts the
two ranks itself, each under its own time limit, and nothing else."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HL, WL, STEPS = 8, 32, 32, 2                                     # the worker's 256 x 256 frame
LIMIT_S = 300


def test_two_ranks_end_with_the_bits_of_one(gpu, tmp_path):
    """A strided plan that is the same for one rank and for two: 8 frames, chunk 6, overlap 2, two levels -> windows (0, 6, 1),
    (4, 4, 1), (0, 4, 2), (1, 4, 2); rank 0 runs (0, 6, 1) and (0, 4, 2), rank 1 the other two.  The worker itself checks that
    both ranks hold identical bits."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    from vdx.codenoise import stride_plan
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    windows = ((0, 6, 1), (4, 4, 1), (0, 4, 2), (1, 4, 2))
    assert stride_plan(T, 1, 6, 2, "coherent", 2).windows == stride_plan(T, 2, 6, 2, "coherent", 2).windows == windows
    out = tmp_path / "rank0.pt"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "dist_costride_worker.py"), str(out), str(T), "6", "2", str(STEPS), "dpmpp_2m", "2"]
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29751", VDX_SHARE_GPU="1")
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
    m, emb = build(gpu, 0, 1)
    cfg = DiffuserConfig(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", scheduler="dpmpp_2m", co_denoise=True, context_stride=2)
    lat, info = DistributedVideoDiffuser(cfg, m, make_scheduler("dpmpp_2m", DDIMScheduler()), emb[1:], emb[:1])()
    assert torch.equal(got["lat"].view(torch.int32), lat.cpu().view(torch.int32))
    gi = got["info"]
    assert [tuple(x) for x in gi["ranges"]] == [(0, 6), (4, 8)] == [tuple(x) for x in info["ranges"]] and gi["world_size"] == 2
    record = {"levels": 2, "strides": [1, 2], "windows": [list(w) for w in windows]}
    assert gi["context_stride"] == info["context_stride"] == record == gi["co_denoise"]["context_stride"]
    per_step = 1 * 2 * (2 * 4 * 6 * HL * WL) * 2                     # (world-1) x per_rank x slot halves (the longest window) x 2 bytes
    assert gi["co_denoise"]["bytes_per_step"] == per_step and gi["network_bytes"] == STEPS * per_step
    assert gi["co_denoise"]["windows"] == 4 and gi["co_denoise"]["steps"] == STEPS and gi["co_denoise"]["exchange_s"] > 0
    assert gi["payload_bytes"] == STEPS * (6 + 4) * 4 * 2            # rank 0's windows (0, 6, 1) and (0, 4, 2), every step
    if got["gathers"] is not None:
        assert got["gathers"] > 0                                    # the parameters were sharded and gathered
