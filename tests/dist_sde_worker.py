"""Worker of tests/test_dist_sde_gpu.py (not a test): one rank of a real multi-process windowed job whose sampler is stochastic
(`eta` 1).  All ranks compute on cuda:0 and talk over gloo (the share-GPU rehearsal of tests/dist_pipeline_worker.py).  Every step
of every chunk draws the whole clip's noise at its frames from the seed alone; the ranks check over gloo that their blends carry
the same bits; rank 0 saves its blend.

    torchrun --nproc-per-node W tests/dist_sde_worker.py OUT.pt T CHUNK OVERLAP STEPS SEED"""
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
    T, chunk, ov, steps, seed = (int(a) for a in sys.argv[2:7])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m, emb = build(dev, rank, world)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=256, width=256, mode="hybrid_ctx", device="cuda",
                         noise="philox", seed=seed, eta=1.0)
    d = DistributedVideoDiffuser(cfg, m, DDIMScheduler(), emb[1:], emb[:1])
    lat, info = d(exchange="allgather")
    mine = lat.cpu()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    for r, t in enumerate(every):
        assert torch.equal(t.view(torch.uint8), mine.view(torch.uint8)), ("blend", rank, r)
    if rank == 0:
        torch.save({"lat": mine, "ranges": [tuple(r) for r in info["ranges"]], "world_size": info["world_size"],
                    "sampler_noise": info["sampler_noise"]}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
