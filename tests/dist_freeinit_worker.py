"""Worker of tests/test_freeinit_gpu.py (not a test): one rank of a real multi-process job with `free_init_iters=2`.  All
ranks compute on cuda:0 and talk over gloo (the share-GPU rehearsal of tests/dist_pipeline_worker.py).  With the all-gather
exchange every rank holds the whole blend, so every rank computes the next start latent itself (no collective); the ranks then
check over gloo that their start latents and results carry the same bits; rank 0 saves them.

    torchrun --nproc-per-node W tests/dist_freeinit_worker.py OUT.pt T CHUNK OVERLAP STEPS"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from dist_pipeline_worker import build  # noqa: E402
from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser  # noqa: E402
from vdx.scheduler import DDIMScheduler  # noqa: E402


def main():
    out = sys.argv[1]
    T, chunk, ov, steps = (int(a) for a in sys.argv[2:6])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m, emb = build(dev, rank, world)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=256, width=256, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", free_init_iters=2)
    d = DistributedVideoDiffuser(cfg, m, DDIMScheduler(), emb[1:], emb[:1])
    lat, info = d(exchange="allgather")
    mine = {"lat": lat.cpu(), "start": d.free_init_starts[0].cpu()}
    for k, v in mine.items():
        every = [torch.empty_like(v) for _ in range(world)]
        dist.all_gather(every, v)
        for r, t in enumerate(every):
            assert torch.equal(t, v), (k, rank, r)
    if rank == 0:
        torch.save({"lat": mine["lat"], "starts": [mine["start"]], "free_init": info["free_init"]}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
