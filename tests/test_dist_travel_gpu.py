"""-m gpu: a job with prompt travel (vdx/travel.py) on two ranks against one: two fresh processes, one rank each, both on this box's
one GPU and talking over gloo (tests/dist_travel_worker.py).  The test starts the two ranks itself, each under its own time limit,
and nothing else."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HL, WL, STEPS = 8, 32, 32, 2                                     # the worker's 256 x 256 frame
LIMIT_S = 300


@pytest.mark.parametrize("co,port", [(True, "29761"), (False, "29763")], ids=["co_denoise", "windowed"])
def test_two_ranks_end_with_the_bits_of_one(gpu, tmp_path, co, port):
    """8 frames, chunk 6, overlap 2: windows (0, 6) and (4, 8), one per rank; each rank builds its own window's text (rank 0 holds
    the text of (0, 6, 1) only).  The worker itself checks that both ranks hold identical bits."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    from dist_travel_worker import travel_of
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    out = tmp_path / "rank0.pt"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "dist_travel_worker.py"), str(out), str(T), "6", "2", str(STEPS), "dpmpp_2m", "1" if co else "0"]
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
    m, emb = build(gpu, 0, 1)
    cfg = DiffuserConfig(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", scheduler="dpmpp_2m", co_denoise=co)
    d = DistributedVideoDiffuser(cfg, m, make_scheduler("dpmpp_2m", DDIMScheduler()), emb[1:], emb[:1], travel=travel_of(emb, T, gpu))
    lat, info = d()
    assert torch.equal(got["lat"].view(torch.int32), lat.cpu().view(torch.int32))
    gi = got["info"]
    assert [tuple(x) for x in gi["ranges"]] == [(0, 6), (4, 8)] == [tuple(x) for x in info["ranges"]] and gi["world_size"] == 2
    assert [tuple(k) for k in got["texts"]] == [(0, 6, 1, False)] and sorted(d._travel_text) == [(0, 6, 1, False), (4, 4, 1, False)]
    if got["gathers"] is not None:
        assert got["gathers"] > 0                                    # the parameters were sharded and gathered
