"""Worker of tests/test_prompt_job_gpu.py (not a test): one rank of a real multi-process `run_job` with `prompt_syntax="a1111"` and a
weighted prompt of more than 75 tokens (vdx/prompt.py).  All ranks compute on cuda:0 and talk over gloo (VDX_DIST_BACKEND=gloo,
VDX_SHARE_GPU=1: the share-GPU rehearsal of tests/dist_pipeline_worker.py).  Every rank chunks, encodes and weights the same texts for
itself: no collective for the text.  The ranks check over gloo that their latents carry the same bits; rank 0 saves the latent and
the result's "prompt_syntax" entry.  The rank, the world size and the rendezvous come from the environment.

    RANK=r WORLD_SIZE=W MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/dist_prompt_worker.py OUT.pt"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from vdx import pipeline  # noqa: E402

LONG = "a (red fox:1.3) in a [dull] forest , " + " ".join(f"word{j}" for j in range(92))          # 100 tokens of the hash tokenizer
NEGATIVE = "(blurry:1.2) , low quality"
JOB = dict(model_id="synthetic:tiny", num_frames=8, steps=2, chunk_size=6, overlap=2, height=128, width=128, mode="hybrid_ctx",
           device="cuda", noise_device="cpu", prompt=LONG, negative_prompt=NEGATIVE, prompt_syntax="a1111")


def run(cfg, pipe=None, exchange="allgather", **kw):
    """`run_job` -> (the latent it decoded, its result, the text shapes the UNet received): the latent is taken where the job hands
    it to the decoder."""
    seen = {"text": set()}
    orig = pipeline.DistributedVideoDiffuser.decode_frames
    denoise = pipeline.DistributedVideoDiffuser.__call__

    def spy(self, lat, vae, **k):
        seen["lat"] = lat.detach().clone()
        return orig(self, lat, vae, **k)

    def call(self, *a, **k):
        forward = self.unet.forward

        def fwd(sample, t, encoder_hidden_states, **fk):
            seen["text"].add(tuple(encoder_hidden_states.shape))
            return forward(sample, t, encoder_hidden_states, **fk)
        self.unet.forward = fwd
        try:
            return denoise(self, *a, **k)
        finally:
            del self.unet.forward
    pipeline.DistributedVideoDiffuser.decode_frames = spy
    pipeline.DistributedVideoDiffuser.__call__ = call
    try:
        res = pipeline.run_job(cfg, exchange=exchange, out_video=None, pipe=pipe, **kw)
    finally:
        pipeline.DistributedVideoDiffuser.decode_frames = orig
        pipeline.DistributedVideoDiffuser.__call__ = denoise
    return seen["lat"], res, seen["text"]


def main():
    out = sys.argv[1]
    lat, res, texts = run(pipeline.DiffuserConfig(**JOB))
    rank, world = dist.get_rank(), dist.get_world_size()
    mine = lat.float().cpu()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    for r, t in enumerate(every):
        assert torch.equal(t.view(torch.int32), mine.view(torch.int32)), (rank, r)
    assert texts == {(2, 154, 128)}, texts
    if rank == 0:
        torch.save({"lat": mine, "prompt_syntax": res["prompt_syntax"], "world_size": res["world_size"]}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
