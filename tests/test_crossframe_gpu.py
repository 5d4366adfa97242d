"""Cross-frame attention on the GPU: `ops.flash_attn_frames` (csrc/flash_frames.hip) against the float64 definition
(tests/crossframe_ref.py), reference isolation, determinism, the `_self_attention` stage and the UNet switch.

Measured on an MI355X (profiles/crossframe_parity.txt): max |out - float64| per shape is recorded there; bound 4e-3."""
import pytest
import torch

from crossframe_ref import attention
from test_hypertile_gpu import TINY, close, tiny_model

pytestmark = pytest.mark.gpu

#        (n_samples, F, S, heads, refs)
SHAPES = [(1, 2, 4, 1, "first"),             # fewer keys than one tile
          (2, 3, 45, 1, "sparse_causal"),    # a seam inside a tile, 90 keys, a masked tail
          (1, 3, 64, 2, "self_first"),       # seams exactly on tile edges
          (1, 3, 65, 1, "sparse_causal"),    # a one-key spill
          (2, 4, 144, 5, "sparse_causal"),   # a query-block tail, five heads with ld = 960, more than 8 pairs
          (1, 5, 24, 1, "table"),            # several seams in one tile, duplicates, a forward reference
          (1, 2, 576, 2, "self_prev")]       # 64 queries per wave
_CACHE = {}


def table(mode, F):
    from vdx.crossframe import ref_table
    return ref_table([[f, f, 0, F - 1] for f in range(F)] if mode == "table" else mode, F)


def case(shape):
    """(qkv fp16 [M][3C] on the host, float64 reference [M][C]), built once per shape and shared."""
    if shape not in _CACHE:
        n, F, S, heads, mode = shape
        qkv = torch.randn(n * F * S, 3 * heads * 64, generator=torch.Generator().manual_seed(S * 100 + F)).half()
        _CACHE[shape] = (qkv, attention(qkv, n, F, S, heads, table(mode, F)))
    return _CACHE[shape]


def run(gpu, qkv, shape, refs=None, n=None, out=None):
    from vdx import ops
    _, F, S, heads, mode = shape
    C = heads * 64
    x = qkv.to(gpu)
    refs = table(mode, F) if refs is None else torch.tensor(refs, dtype=torch.int32)
    return ops.flash_attn_frames(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], n_samples=n or shape[0], F=F, S=S, heads=heads, refs=refs.to(gpu),
                                 scale=0.125, out=out)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(gpu, shape):
    qkv, ref = case(shape)
    out = run(gpu, qkv, shape)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"flash_attn_frames {shape}: max |out - float64| = {err:.3e}, max |ref| = {ref.abs().max().item():.3e}")
    close(out, ref.float(), tol=4e-3)


@pytest.mark.parametrize("dup", [1, 2])
def test_own_frame_is_the_plain_attention(gpu, dup):
    """refs = [[f]] and [[f, f]]: a frame attending to itself (twice) is `flash_attn` on the same rows; duplicates leave a softmax alone."""
    from vdx import ops
    shape = (2, 3, 45, 1, "sparse_causal")
    qkv, _ = case(shape)
    x = qkv.to(gpu)
    plain = ops.flash_attn(x[:, :64], x[:, 64:128], x[:, 128:], n_seq=6, sq=45, skv=45, skv_pad=45, heads=1, seq_per_kv=1, scale=0.125, v_rows=True)
    close(run(gpu, qkv, shape, refs=[[f] * dup for f in range(3)]), plain.float().cpu(), tol=4e-3)


@pytest.mark.parametrize("poison", ["frames", "sample"])
def test_references_are_isolated(gpu, poison):
    """Frames 2 and 3 (or the whole second sample) are NaN in q, k and v: frames 0 and 1 of the first sample reference frames
    0 and 1 only, so their outputs are finite and the bits of the clean run."""
    n = 1 if poison == "frames" else 2
    shape = (n, 4, 45, 1, "sparse_causal")
    qkv = torch.randn(n * 4 * 45, 192, generator=torch.Generator().manual_seed(5)).half()
    clean = run(gpu, qkv, shape)
    bad = qkv.clone()
    bad[2 * 45:4 * 45 if poison == "frames" else None] = float("nan")
    out = run(gpu, bad, shape)
    assert bool(torch.isfinite(out[:2 * 45]).all()) and torch.equal(out[:2 * 45], clean[:2 * 45])


def test_deterministic_and_batch_independent(gpu):
    shape = (2, 4, 144, 5, "sparse_causal")
    qkv, _ = case(shape)
    out = run(gpu, qkv, shape)
    assert torch.equal(run(gpu, qkv, shape), out)
    M = 4 * 144
    for b in range(2):
        assert torch.equal(run(gpu, qkv[b * M:(b + 1) * M], shape, n=1), out[b * M:(b + 1) * M])


def test_library_refusals(gpu):
    from vdx._lib import VdxError
    shape = (1, 2, 4, 1, "first")
    qkv = torch.zeros(8, 192, dtype=torch.float16)
    for refs in ([[], []], [[0] * 5] * 2):                       # R = 0, R = 5
        with pytest.raises(VdxError):
            run(gpu, qkv, shape, refs=refs)
    with pytest.raises(VdxError):                                 # ld = 196 is no multiple of 8
        run(gpu, torch.zeros(8, 196, dtype=torch.float16), shape)
    x = qkv.to(gpu)
    with pytest.raises(VdxError):                                 # out is k
        run(gpu, x, shape, out=x[:, 64:128])


def test_self_attention_stage(gpu):
    """The stage against its composition from existing ops: gather + concat of the reference frames' K and V rows, `flash_attn`
    over 2 S keys.  Two kernels with different tile seams: fp16 rounding apart, inside the flash family's bound."""
    from vdx import ops
    m = tiny_model(gpu).enable_cross_frame("sparse_causal")
    p, b = "down_blocks.0.attentions.0", "down_blocks.0.attentions.0.transformer_blocks.0"
    n_img, F, hh, ww, C = 6, 3, 10, 14, 64
    S = hh * ww
    M = n_img * S
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(23)).half().to(gpu)
    t = m._norm_proj_in(p, x, n_img, S, M)
    got = m._self_attention(b, t, n_img, hh, ww, 1, F=F)
    W = m.W
    ln = ops.layernorm(t, W[b + ".norm1.weight"], W[b + ".norm1.bias"], M=M)
    qkv = ops.gemm(ln, W[b + ".attn1.to_qkv.weight"], M=M)
    img = torch.tensor([[s * F + r for r in row] for s in range(n_img // F) for row in table("sparse_causal", F).tolist()], device=gpu)
    kv = qkv.view(n_img, S, 3 * C)[img].reshape(n_img * 2 * S, 3 * C)          # image i: its two reference frames' rows
    o = ops.flash_attn(qkv[:, :C], kv[:, C:2 * C], kv[:, 2 * C:], n_seq=n_img, sq=S, skv=2 * S, skv_pad=2 * S, heads=1, seq_per_kv=1,
                       scale=64 ** -0.5, v_rows=True)
    want = ops.gemm(o, W[b + ".attn1.to_out.0.weight"], M=M, bias=W[b + ".attn1.to_out.0.bias"], residual=t)
    print(f"cross-frame stage: max |stage - composed| = {(got.float() - want.float()).abs().max().item():.3e}")
    close(got, want.float().cpu(), tol=4e-3)
    plain = tiny_model(gpu)._self_attention(b, t, n_img, hh, ww, 1)
    assert not torch.equal(got, plain)
    assert torch.equal(m._self_attention(b, t, n_img, hh, ww, 1), plain)               # F unknown: the plain attention
    m.enable_cross_frame("sparse_causal", max_downsample=1)
    assert torch.equal(m._self_attention(b, t, n_img, hh, ww, 2, F=F), plain)          # above max_downsample
    assert torch.equal(m.disable_cross_frame()._self_attention(b, t, n_img, hh, ww, 1, F=F), plain)


def test_unet_with_cross_frame(gpu, monkeypatch):
    from vdx import ops
    launched, launch = [], ops._launch
    monkeypatch.setattr(ops, "_launch", lambda symbol, *a: (launched.append(symbol), launch(symbol, *a))[1])
    m = tiny_model(gpu)
    g = torch.Generator().manual_seed(21)
    lat = torch.randn(1, 4, 4, 16, 32, generator=g).half().to(gpu)
    e = torch.randn(2, 77, TINY["cross"], generator=g).half().to(gpu)
    x = ops.cfg_input(lat, None, 0.0)
    m(x, 7, encoder_hidden_states=e)                                                   # the text's keys / values are cached from here on
    del launched[:]
    off = m(x, 7, encoder_hidden_states=e).sample
    off_launches = list(launched)
    m.enable_cross_frame("sparse_causal")
    assert m.cross_frame == {"mode": "sparse_causal", "refs_per_frame": 2, "max_downsample": 8}
    del launched[:]
    on = m(x, 7, encoder_hidden_states=e).sample
    assert m.last_forward_shared_prefix
    assert bool(torch.isfinite(on.float()).all()) and not torch.equal(on, off)
    assert "vdx_flash_attn_frames_f16" in launched and "vdx_flash_attn_frames_f16" not in off_launches
    assert [s.replace("attn_frames", "attn_rows") for s in launched] == off_launches    # the attention swapped, nothing added
    dup = m(x.clone(), 7, encoder_hidden_states=e).sample                              # the shared prefix off
    assert not m.last_forward_shared_prefix and torch.equal(dup, on)
    with pytest.raises(ValueError):
        m.enable_tome(0.5)
    with pytest.raises(ValueError):
        m.enable_hypertile(2, 2)
    with pytest.raises(ValueError):
        m.enable_cross_frame("causal")
    assert m.tome is None and m.hypertile is None and m.cross_frame["mode"] == "sparse_causal"   # a refusal leaves the state
    m.disable_cross_frame()
    assert m.cross_frame is None and torch.equal(m(x, 7, encoder_hidden_states=e).sample, off)
    m.enable_hypertile(2, 2)
    with pytest.raises(ValueError):
        m.enable_cross_frame("first")
    assert m.cross_frame is None
