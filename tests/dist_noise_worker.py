"""Worker of tests/test_dist_noise_gpu.py (not a test): one rank of a real multi-process job whose noise comes from the portable
generator.  All ranks compute on cuda:0 and talk over gloo (the share-GPU rehearsal of tests/dist_pipeline_worker.py).  Every rank
draws the whole clip's start latent itself, from the seed alone; the ranks check over gloo that their start latents and their
blends carry the same bits; rank 0 saves its blend.

    torchrun --nproc-per-node W tests/dist_noise_worker.py OUT.pt T CHUNK OVERLAP STEPS SEED CO_DENOISE"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from dist_pipeline_worker import build  # noqa: E402
from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, seeded_noise  # noqa: E402
from vdx.scheduler import DDIMScheduler  # noqa: E402


def _all_equal(mine, rank, world, what):
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    for r, t in enumerate(every):
        assert torch.equal(t.view(torch.uint8), mine.view(torch.uint8)), (what, rank, r)


def main():
    out = sys.argv[1]
    T, chunk, ov, steps, seed, co = (int(a) for a in sys.argv[2:8])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m, emb = build(dev, rank, world)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=256, width=256, mode="hybrid_ctx", device="cuda",
                         noise="philox", seed=seed, co_denoise=bool(co))
    d = DistributedVideoDiffuser(cfg, m, DDIMScheduler(), emb[1:], emb[:1])
    _all_equal(seeded_noise(d.latent_shape, 1.0, "cuda", seed=seed).cpu(), rank, world, "start latent")
    lat, info = d(exchange="allgather")
    mine = lat.cpu()
    _all_equal(mine, rank, world, "blend")
    if rank == 0:
        torch.save({"lat": mine, "ranges": [tuple(r) for r in info["ranges"]], "world_size": info["world_size"], "noise": info["noise"]}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
