"""Worker of tests/test_region_job_gpu.py (not a test): one rank of a real multi-process job with regional prompts (vdx/region.py).
All ranks compute on cuda:0 and talk over gloo (the share-GPU rehearsal of tests/dist_pipeline_worker.py).  Every rank builds the
same plan from the same masks (no collective for the regions) and passes each of its own windows' place in the clip to the UNet.
With the all-gather exchange every rank ends with the whole latent, and the ranks check over gloo that their latents carry the
same bits; with the halo exchange a rank ends with the frames it owns, and rank 0 collects the owned segments into the clip.  Rank 0
saves the latent and `info`.  The rank, the world size and the rendezvous come from the environment (RANK, WORLD_SIZE, MASTER_ADDR,
MASTER_PORT): the test starts each rank as a process of its own.

    RANK=r WORLD_SIZE=W MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/dist_region_worker.py OUT.pt T CHUNK OVERLAP STEPS SCHEDULER CO EXCHANGE"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from dist_pipeline_worker import build  # noqa: E402
from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler  # noqa: E402
from vdx.region import region_plan  # noqa: E402
from vdx.scheduler import DDIMScheduler  # noqa: E402

HL = WL = 32


def masks_of(T):
    """0 / 255 only, edges off the cell grid.  Region 1: static, the left 100 pixels; region 2: per frame, a band from the top that
    grows with the frames and is absent on frames 0 and 1; they overlap."""
    H, W = 8 * HL, 8 * WL
    m1 = np.zeros((H, W), np.uint8)
    m1[:, :100] = 255
    m2 = np.zeros((T, H, W), np.uint8)
    for t in range(2, T):
        m2[t, :20 * t, 60:] = 255
    return m1, m2


def regions_of(emb, T, dev):
    """The job's regions: seeded text embeddings and the plan of `masks_of`, the same on every rank and in the test."""
    rtext = torch.randn(2, 77, emb.shape[2], generator=torch.Generator().manual_seed(9)).half().to(dev)
    return rtext, region_plan([(m, f"text {i}") for i, m in enumerate(masks_of(T))], T, HL, WL, 4)


def main():
    out = sys.argv[1]
    T, chunk, ov, steps = (int(a) for a in sys.argv[2:6])
    sampler, co, exchange = sys.argv[6], sys.argv[7] == "1", sys.argv[8]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m, emb = build(dev, rank, world)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=8 * HL, width=8 * WL, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", scheduler=sampler, co_denoise=co)
    d = DistributedVideoDiffuser(cfg, m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1], regions=regions_of(emb, T, dev))
    windows = []
    forward = m.forward

    def spy(*a, **k):
        windows.append(k["regions"][2])
        return forward(*a, **k)
    m.forward = spy
    lat, info = d(exchange=exchange)
    del m.forward
    if exchange == "allgather":
        mine = lat.cpu()
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        for r, t in enumerate(every):
            assert torch.equal(t.view(torch.int32), mine.view(torch.int32)), (rank, r)
    else:                                       # the owned segments of every rank -> the clip, on every rank
        owned = [None] * world
        dist.all_gather_object(owned, [(s, e, t.cpu()) for s, e, t in lat])
        mine = torch.zeros(d.latent_shape, dtype=torch.float32)
        seen = torch.zeros(T, dtype=torch.int32)
        for segs in owned:
            for s, e, t in segs:
                mine[:, :, s:e] = t
                seen[s:e] += 1
        assert bool((seen == 1).all()), seen.tolist()
    if rank == 0:
        keep = ("ranges", "chunk_size", "overlap", "world_size", "steps_run")
        torch.save({"lat": mine, "info": {k: info[k] for k in keep}, "gathers": getattr(m.W, "gathers", None),
                    "windows": sorted(set(windows))}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
