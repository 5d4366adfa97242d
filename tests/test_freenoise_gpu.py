"""-m gpu: FreeNoise's kernels (csrc/freenoise.hip) against tests/freenoise_ref.py, their exact properties, the UNet, the job."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import freenoise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
SCALE = 0.125
# key padding + a moved-back last window; two windows one frame apart; the 32-frame block edge; L = 32; three blocks; 29 windows
SHAPES = [(7, 3, 2), (17, 16, 4), (33, 16, 4), (40, 32, 8), (65, 5, 5), (128, 16, 4)]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def make_qkv(F, B=2, HW=3, heads=2, seed=0):           # fp16 N(0, 1) q, k, v (3, B, HW, heads, F, 64) on the host
    return torch.randn(3, B, HW, heads, F, 64, generator=torch.Generator().manual_seed(seed)).half()


def run_core(gpu, qkv, L, S, weighting="pyramid", pad=(16, 8)):
    """-> the kernel's (B, HW, heads, F, 64) on the host; rows padded past their minimum, the canary columns checked."""
    from vdx import freenoise, ops
    _, B, HW, heads, F, _ = qkv.shape
    inner = heads * 64
    rows = qkv.permute(1, 4, 2, 0, 3, 5).reshape(B * F * HW, 3 * inner)           # row (b F + f) HW + p, columns [q | k | v]
    wide = torch.full((rows.shape[0], 3 * inner + pad[0]), 7.0, dtype=torch.float16, device=gpu)
    wide[:, :3 * inner] = rows.to(gpu)
    out = torch.full((rows.shape[0], inner + pad[1]), 9.0, dtype=torch.float16, device=gpu)
    wn = freenoise.window_weights(F, L, S, weighting).to(gpu)
    ops.temporal_attn_windows(wide[:, :3 * inner], wn, B=B, F=F, HW=HW, heads=heads, scale=SCALE, L=L, S=S, out=out[:, :inner])
    assert bool((out[:, inner:] == 9.0).all()) and bool((wide[:, 3 * inner:] == 7.0).all())
    return out[:, :inner].cpu().reshape(B, F, HW, heads, 64).permute(0, 2, 3, 1, 4)


@pytest.mark.parametrize("weighting", ["pyramid", "flat"])
@pytest.mark.parametrize("F,L,S", SHAPES)
def test_core_matches_the_restatement(gpu, F, L, S, weighting):
    """The bound of tests/test_ops_gpu.py::test_temporal_attention: |err| <= 4e-3 max|ref| + 4e-3 |ref|."""
    qkv = make_qkv(F, seed=F)
    got = run_core(gpu, qkv, L, S, weighting).double()
    ref = R.windowed_attention(*qkv, SCALE, L, S, R.window_weights(F, L, S, weighting))
    err = (got - ref).abs()
    print(f"F={F} L={L} S={S} {weighting}: max err {float(err.max()):.3e}, max|ref| {float(ref.abs().max()):.3f}")
    assert bool((err <= 4e-3 * ref.abs().max() + 4e-3 * ref.abs()).all())


@pytest.mark.parametrize("F,L,S", [(17, 16, 4), (40, 32, 8), (65, 5, 5)])
def test_core_same_bits_whatever_runs_beside_it(gpu, F, L, S):
    qkv = make_qkv(F, HW=5, seed=1)
    a = run_core(gpu, qkv, L, S)
    assert torch.equal(run_core(gpu, qkv, L, S), a)                                        # run to run
    for b in range(2):                                                                     # each half of the batch alone
        assert torch.equal(run_core(gpu, qkv[:, b:b + 1], L, S)[0], a[b])
    for p in range(5):                                                                     # each pixel alone
        assert torch.equal(run_core(gpu, qkv[:, :, p:p + 1], L, S)[:, 0], a[:, p])
    bad = qkv.clone()
    bad[:, 1, 2, 1, F // 2] = float("nan")                                                 # q, k and v of one frame of one (pixel, head)
    got = run_core(gpu, bad, L, S)
    clean = torch.ones(2, 5, 2, dtype=torch.bool)
    clean[1, 2, 1] = False
    assert torch.equal(got[clean].view(torch.int16), a[clean].view(torch.int16)) and bool(got[1, 2, 1].isnan().any())


@pytest.mark.parametrize("h,w", [(2, 4), (1, 5)])
def test_frame_gather(gpu, h, w):
    from vdx import ops
    src = torch.randn(1, 4, 9, h, w, generator=torch.Generator().manual_seed(2)).half().to(gpu)
    idx = [0, 1, 2, 3, 1, 0, 3, 2, 8]
    assert torch.equal(ops.frame_gather(src, idx), src.index_select(2, torch.tensor(idx, device=gpu)))
    for bad in ([0] * 8 + [9], [-1] + [0] * 8, [0] * 8):
        with pytest.raises(ops.VdxError):
            ops.frame_gather(src, bad)
    with pytest.raises(ops.VdxError):
        ops.frame_gather(src, idx, out=src)


@pytest.mark.parametrize("F,L,S", [(40, 33, 4), (40, 1, 1), (40, 16, 0), (40, 16, 17), (16, 16, 4), (129, 16, 4)])
def test_core_refuses_what_lies_outside_its_domain(gpu, F, L, S):
    from vdx import ops
    qkv = torch.zeros((F, 192), dtype=torch.float16, device=gpu)
    with pytest.raises(ops.VdxError):
        ops.temporal_attn_windows(qkv, torch.ones((64, 32), device=gpu), B=1, F=F, HW=1, heads=1, scale=SCALE, L=L, S=S)


def windowed_oracle(ref_m, L, S, weighting="pyramid"):
    """Replace the forward of attn1 / attn2 of every temporal transformer of the fp32 oracle by the windowed restatement."""
    def windowed(att):
        def forward(x, ctx=None):
            n, F, _ = x.shape
            q, k, v = (p(x).view(n, F, att.heads, att.dim_head).transpose(1, 2) for p in (att.to_q, att.to_k, att.to_v))
            o = R.windowed_attention(q, k, v, att.dim_head ** -0.5, L, S, R.window_weights(F, L, S, weighting)).float()
            return att.to_out[0](o.transpose(1, 2).reshape(n, F, att.heads * att.dim_head))
        return forward
    for m in ref_m.modules():
        if type(m).__name__ == "TransformerTemporalModel":
            for att in (m.transformer_blocks[0].attn1, m.transformer_blocks[0].attn2):
                att.forward = windowed(att)


def test_unet_with_free_noise_matches_the_oracle_with_windows(gpu):
    """(2, 4, 9, 16, 32), t = 7, windows of 4 at stride 2: the bound this model has without the option, 4e-3."""
    from test_freeu_gpu import tiny_model
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg
    m, sd = tiny_model(gpu)
    ref_m = UNet3DConditionModelRef(RefCfg.tiny(**TINY)).eval()
    ref_m.load_state_dict({k: v.half().float() for k, v in sd.items()})
    windowed_oracle(ref_m, 4, 2)
    g = torch.Generator().manual_seed(21)
    sample = torch.randn(2, 4, 9, 16, 32, generator=g).half()
    ehs = torch.randn(2, 77, TINY["cross"], generator=g).half()
    with torch.no_grad():
        ref = ref_m(sample.float(), torch.tensor(7), ehs.float()).sample
    x, e = sample.to(gpu), ehs.to(gpu)
    off = m(x, 7, encoder_hidden_states=e).sample
    short = m(x[:, :, :4].contiguous(), 7, encoder_hidden_states=e).sample
    m.enable_free_noise(4, 2)
    on = m(x, 7, encoder_hidden_states=e).sample
    err, moved = rel_l2(on.float().cpu(), ref), rel_l2(on.float().cpu(), off.float().cpu())
    print(f"FreeNoise on: rel-L2 {err:.3e} from the oracle with windows; {moved:.3f} from the forward without")
    assert err <= 4e-3 and moved > 0.01
    assert torch.equal(m(x[:, :, :4].contiguous(), 7, encoder_hidden_states=e).sample, short)       # F = 4 <= L: one window, as without
    m.disable_free_noise()
    assert torch.equal(m(x, 7, encoder_hidden_states=e).sample, off)


def test_run_job_with_free_noise(gpu, monkeypatch):
    """The tiny job of tests/test_freeu_gpu.py, 12 frames in one chunk."""
    from vdx import freenoise, ops
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import DiffuserConfig, run_job, seeded_noise
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    starts, real_gather = [], ops.frame_gather

    def job(**kw):
        got = {}
        cfg = DiffuserConfig(model_id="synthetic:tiny", num_frames=12, steps=2, height=128, width=256, mode="fsdp", noise_device="cpu", **kw)
        res = run_job(cfg, out_video=None, pipe=pipe, clip_inputs=got)
        assert pipe.unet.free_noise is None
        return res, np.stack(got["frames"])
    res0, frames0 = job()
    assert "free_noise" not in res0
    monkeypatch.setattr(ops, "frame_gather", lambda src, idx: starts.append((src, idx, real_gather(src, idx))) or starts[-1][2])
    res1, frames1 = job(free_noise=(4, 2))
    assert res1["free_noise"] == {"context_length": 4, "context_stride": 2, "weighting": "pyramid", "windows": 5}
    assert set(res1) == set(res0) | {"free_noise"} and not np.array_equal(frames1, frames0)
    (plain, idx, start), = starts
    assert list(idx) == freenoise.reschedule_index(12, 4, 2, 0)
    assert torch.equal(plain, seeded_noise(plain.shape, pipe.scheduler.init_noise_sigma, "cuda", "cpu"))
    assert torch.equal(start, plain.index_select(2, torch.tensor(idx, device=plain.device)))
    assert np.array_equal(job(free_noise=(4, 2))[1], frames1)                              # two runs, equal frames
    assert np.array_equal(job()[1], frames0)                                               # and the default job is still the default job
