"""Worker of tests/test_lora_job_gpu.py (not a test): one rank of a real multi-process `run_job` with a LoRA adapter (vdx/lora.py).
All ranks compute on cuda:0 and talk over gloo (VDX_DIST_BACKEND=gloo, VDX_SHARE_GPU=1: the share-GPU rehearsal of
tests/dist_pipeline_worker.py).  Every rank reads the same adapter file and merges it for itself, before the UNet is sharded: no
collective for the adapter.  The ranks check over gloo that their latents carry the same bits; rank 0 saves the latent and the
result's "lora" entry.  The rank, the world size and the rendezvous come from the environment.

    RANK=r WORLD_SIZE=W MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/dist_lora_worker.py OUT.pt ADAPTER SCALE"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from vdx import pipeline  # noqa: E402

JOB = dict(model_id="synthetic:tiny", num_frames=8, steps=2, chunk_size=6, overlap=2, height=128, width=128, mode="hybrid_ctx",
           device="cuda", noise_device="cpu", prompt="a forest")


def run(cfg, pipe=None):
    """`run_job` -> (the latent it decoded, its result): the latent is taken where the job hands it to the decoder."""
    seen = {}
    orig = pipeline.DistributedVideoDiffuser.decode_frames

    def spy(self, lat, vae, **kw):
        seen["lat"] = lat.detach().clone()
        return orig(self, lat, vae, **kw)
    pipeline.DistributedVideoDiffuser.decode_frames = spy
    try:
        res = pipeline.run_job(cfg, out_video=None, pipe=pipe)
    finally:
        pipeline.DistributedVideoDiffuser.decode_frames = orig
    return seen["lat"], res


def main():
    out, adapter, scale = sys.argv[1], sys.argv[2], float(sys.argv[3])
    lat, res = run(pipeline.DiffuserConfig(**JOB, lora=((adapter, scale),)))
    rank, world = dist.get_rank(), dist.get_world_size()
    mine = lat.float().cpu()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    for r, t in enumerate(every):
        assert torch.equal(t.view(torch.int32), mine.view(torch.int32)), (rank, r)
    if rank == 0:
        torch.save({"lat": mine, "lora": res["lora"], "world_size": res["world_size"]}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
