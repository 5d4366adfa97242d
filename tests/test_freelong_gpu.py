"""-m gpu: FreeLong's kernel (csrc/freelong.hip) against tests/freelong_ref.py, its anchors and exact properties, the UNet, the job."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import freelong_ref as R  # noqa: E402
from test_freenoise_gpu import SCALE, TINY, make_qkv, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

# key padding in one block, r = 1; the 32-frame block edge; the band crosses it; three blocks and a key block outside the band;
# the full domain; Lp = 0
SHAPES = [(7, 2, 0.25), (33, 16, 0.25), (40, 24, 0.5), (65, 8, 0.25), (128, 24, 0.25), (17, 16, 0.0)]


def run_core(gpu, qkv, lp, r, pad=(16, 8)):
    """-> the kernel's (B, HW, heads, F, 64) on the host; rows padded past their minimum, the canary columns checked."""
    from vdx import ops
    _, B, HW, heads, F, _ = qkv.shape
    inner = heads * 64
    rows = qkv.permute(1, 4, 2, 0, 3, 5).reshape(B * F * HW, 3 * inner)           # row (b F + f) HW + p, columns [q | k | v]
    wide = torch.full((rows.shape[0], 3 * inner + pad[0]), 7.0, dtype=torch.float16, device=gpu)
    wide[:, :3 * inner] = rows.to(gpu)
    out = torch.full((rows.shape[0], inner + pad[1]), 9.0, dtype=torch.float16, device=gpu)
    ops.temporal_attn_blend(wide[:, :3 * inner], lp.to(torch.float16).to(gpu).contiguous(), B=B, F=F, HW=HW, heads=heads, scale=SCALE,
                            radius=r, out=out[:, :inner])
    assert bool((out[:, inner:] == 9.0).all()) and bool((wide[:, 3 * inner:] == 7.0).all())
    return out[:, :inner].cpu().reshape(B, F, HW, heads, 64).permute(0, 2, 3, 1, 4)


def within_bound(got, ref, what):
    """The bound of tests/test_ops_gpu.py::test_temporal_attention: |err| <= 4e-3 max|ref| + 4e-3 |ref|."""
    err = (got.double() - ref).abs()
    print(f"{what}: max err {float(err.max()):.3e}, max|ref| {float(ref.abs().max()):.3f}")
    return bool((err <= 4e-3 * ref.abs().max() + 4e-3 * ref.abs()).all())


@pytest.mark.parametrize("F,window,d_t", SHAPES)
def test_core_matches_the_restatement(gpu, F, window, d_t):
    from vdx import freelong
    qkv, r = make_qkv(F, seed=F), freelong.radius_of(window)
    got = run_core(gpu, qkv, freelong.blend_matrix(F, "gaussian", d_t), r)
    assert within_bound(got, R.blended_attention(*qkv, SCALE, r, R.blend_matrix(F, "gaussian", d_t)), f"F={F} window={window} d_t={d_t}")


@pytest.mark.parametrize("F", [17, 40, 128])
def test_anchors_and_a_matrix_that_is_not_symmetric(gpu, F):
    from vdx import ops
    qkv = make_qkv(F, seed=100 + F)
    _, B, HW, heads, _, _ = qkv.shape
    rows = qkv.permute(1, 4, 2, 0, 3, 5).reshape(B * F * HW, 3 * heads * 64).to(gpu)
    plain = ops.temporal_attn(rows, B=B, F=F, HW=HW, heads=heads, scale=SCALE).cpu().reshape(B, F, HW, heads, 64).permute(0, 2, 3, 1, 4).double()
    shift = torch.eye(F, dtype=torch.float64).roll(1, dims=1)                      # out[t] takes D[t + 1 mod F]: not its transpose
    assert within_bound(run_core(gpu, qkv, torch.eye(F), 2), plain, f"F={F} Lp=I against temporal_attn")
    assert within_bound(run_core(gpu, qkv, shift, F - 1), plain, f"F={F} r=F-1 against temporal_attn")
    assert within_bound(run_core(gpu, qkv, shift, 3), R.blended_attention(*qkv, SCALE, 3, shift), f"F={F} cyclic shift, r=3")


@pytest.mark.parametrize("F,window", [(40, 24), (65, 8)])
def test_core_same_bits_whatever_runs_beside_it(gpu, F, window):
    from vdx import freelong
    qkv, lp, r = make_qkv(F, HW=5, seed=1), freelong.blend_matrix(F, "gaussian", 0.25), window // 2
    a = run_core(gpu, qkv, lp, r)
    assert torch.equal(run_core(gpu, qkv, lp, r), a)                                       # run to run
    for b in range(2):                                                                     # each half of the batch alone
        assert torch.equal(run_core(gpu, qkv[:, b:b + 1], lp, r)[0], a[b])
    assert torch.equal(run_core(gpu, qkv[:, :, 3:4, 1:2], lp, r)[:, 0, 0], a[:, 3, 1])      # one (pixel, head) alone
    bad = qkv.clone()
    bad[:, 1, 2, 1, F // 2] = float("nan")                                                 # q, k and v of one frame of one (pixel, head)
    got = run_core(gpu, bad, lp, r)
    clean = torch.ones(2, 5, 2, dtype=torch.bool)
    clean[1, 2, 1] = False
    assert torch.equal(got[clean].view(torch.int16), a[clean].view(torch.int16)) and bool(got[1, 2, 1].isnan().any())


def test_core_refuses_what_lies_outside_its_domain(gpu):
    from vdx import ops

    def call(F=40, r=4, lp=None, out=None):
        qkv = torch.zeros((F, 192), dtype=torch.float16, device=gpu)
        lp = torch.zeros((F, F), dtype=torch.float16, device=gpu) if lp is None else lp
        return ops.temporal_attn_blend(qkv, lp, B=1, F=F, HW=1, heads=1, scale=SCALE, radius=r, out=qkv[:, :64] if out == "alias" else None)
    call()
    for kw in (dict(F=129), dict(F=1), dict(r=0), dict(out="alias"), dict(lp=torch.zeros((40, 41), dtype=torch.float16, device=gpu)),
               dict(lp=torch.zeros((40, 40), dtype=torch.float16)), dict(lp=torch.zeros((40, 40), device=gpu))):
        with pytest.raises(ops.VdxError):
            call(**kw)


def blended_oracle(ref_m, window, d_t):
    """Replace the forward of attn1 / attn2 of every temporal transformer of the fp32 oracle by the blended restatement."""
    def blended(att):
        def forward(x, ctx=None):
            n, F, _ = x.shape
            q, k, v = (p(x).view(n, F, att.heads, att.dim_head).transpose(1, 2) for p in (att.to_q, att.to_k, att.to_v))
            o = R.blended_attention(q, k, v, att.dim_head ** -0.5, window // 2, R.blend_matrix(F, "gaussian", d_t)).float()
            return att.to_out[0](o.transpose(1, 2).reshape(n, F, att.heads * att.dim_head))
        return forward
    for m in ref_m.modules():
        if type(m).__name__ == "TransformerTemporalModel":
            for att in (m.transformer_blocks[0].attn1, m.transformer_blocks[0].attn2):
                att.forward = blended(att)


def test_unet_with_free_long_matches_the_oracle_with_the_blend(gpu):
    """(2, 4, 9, 16, 32), t = 7, window 4, d_t 0.25: the bound this model has without the option, 4e-3."""
    from test_freeu_gpu import tiny_model
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg
    m, sd = tiny_model(gpu)
    ref_m = UNet3DConditionModelRef(RefCfg.tiny(**TINY)).eval()
    ref_m.load_state_dict({k: v.half().float() for k, v in sd.items()})
    blended_oracle(ref_m, 4, 0.25)
    g = torch.Generator().manual_seed(21)
    sample = torch.randn(2, 4, 9, 16, 32, generator=g).half()
    ehs = torch.randn(2, 77, TINY["cross"], generator=g).half()
    with torch.no_grad():
        ref = ref_m(sample.float(), torch.tensor(7), ehs.float()).sample
    x, e = sample.to(gpu), ehs.to(gpu)
    off = m(x, 7, encoder_hidden_states=e).sample
    short = m(x[:, :, :4].contiguous(), 7, encoder_hidden_states=e).sample
    m.enable_free_long(4, 0.25)
    assert m.free_long == {"window": 4, "d_t": 0.25, "method": "gaussian", "order": 4}
    with pytest.raises(ValueError):
        m.enable_free_noise(4, 2)
    on = m(x, 7, encoder_hidden_states=e).sample
    err, moved = rel_l2(on.float().cpu(), ref), rel_l2(on.float().cpu(), off.float().cpu())
    print(f"FreeLong on: rel-L2 {err:.3e} from the oracle with the blend; {moved:.3f} from the forward without")
    assert err <= 4e-3 and moved > 0.01
    assert torch.equal(m(x[:, :, :4].contiguous(), 7, encoder_hidden_states=e).sample, short)       # F = 4 <= window: as without
    m.disable_free_long()
    assert m.free_long is None and torch.equal(m(x, 7, encoder_hidden_states=e).sample, off)
    m.enable_free_noise(4, 2)
    with pytest.raises(ValueError):
        m.enable_free_long(4, 0.25)
    m.disable_free_noise()


def test_run_job_with_free_long(gpu):
    """The tiny job of tests/test_freeu_gpu.py, 12 frames in one chunk."""
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import DiffuserConfig, run_job
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)

    def job(**kw):
        got = {}
        cfg = DiffuserConfig(model_id="synthetic:tiny", num_frames=12, steps=2, height=128, width=256, mode="fsdp", noise_device="cpu", **kw)
        res = run_job(cfg, out_video=None, pipe=pipe, clip_inputs=got)
        assert pipe.unet.free_long is None
        return res, np.stack(got["frames"])
    res0, frames0 = job()
    res1, frames1 = job(free_long=(4, 0.25))
    assert "free_long" not in res0 and res1["free_long"] == {"window": 4, "d_t": 0.25, "method": "gaussian"}
    assert set(res1) == set(res0) | {"free_long"} and not np.array_equal(frames1, frames0)
    assert np.array_equal(job(free_long=(4, 0.25))[1], frames1) and np.array_equal(job()[1], frames0)
