"""Worker of tests/test_dist_travel_gpu.py (not a test): one rank of a real multi-process job with prompt travel (vdx/travel.py).
All ranks compute on cuda:0 and talk over gloo (the share-GPU rehearsal of tests/dist_pipeline_worker.py).  Every rank builds the
text of its own windows from the same keys (no collective for the text); the co-denoised job then gathers the packed noise buffers
once per step and every rank steps its own copy of the clip's latent, the windowed job gathers the denoised chunks and blends; the
ranks then check over gloo that their latents carry the same bits; rank 0 saves its latent and `info`.  The rank, the world size
and the rendezvous come from the environment (RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT): the test starts each rank as a process of
its own.

    RANK=r WORLD_SIZE=W MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/dist_travel_worker.py OUT.pt T CHUNK OVERLAP STEPS SCHEDULER CO"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from dist_pipeline_worker import build  # noqa: E402
from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler  # noqa: E402
from vdx.scheduler import DDIMScheduler  # noqa: E402
from vdx.travel import travel_plan  # noqa: E402

KEY_FRAMES = (0, 3, 7)


def travel_of(emb, T, dev):
    """The job's keys: seeded embeddings at KEY_FRAMES, the same on every rank and in the test."""
    keys = torch.randn(len(KEY_FRAMES), 77, emb.shape[2], generator=torch.Generator().manual_seed(9)).half().to(dev)
    return keys, travel_plan([(f, "") for f in KEY_FRAMES], T)


def main():
    out = sys.argv[1]
    T, chunk, ov, steps = (int(a) for a in sys.argv[2:6])
    sampler, co = sys.argv[6], sys.argv[7] == "1"
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m, emb = build(dev, rank, world)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=256, width=256, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", scheduler=sampler, co_denoise=co)
    d = DistributedVideoDiffuser(cfg, m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1], travel=travel_of(emb, T, dev))
    lat, info = d(exchange="allgather")
    mine = lat.cpu()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    for r, t in enumerate(every):
        assert torch.equal(t.view(torch.int32), mine.view(torch.int32)), (rank, r)
    if rank == 0:
        keep = ("ranges", "chunk_size", "overlap", "world_size", "steps_run")
        torch.save({"lat": mine, "info": {k: info[k] for k in keep}, "gathers": getattr(m.W, "gathers", None),
                    "texts": sorted(d._travel_text)}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
