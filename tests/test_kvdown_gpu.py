"""Token downsampling on the GPU: `ops.flash_attn_kvdown` (csrc/flash_kvdown.hip) against the float64 definition on the rows
`kvdown.key_rows` names, the rows it may not read, image isolation, determinism, the composition gather + `ops.flash_attn`,
the `_self_attention` stage and the UNet switch."""
import pytest
import torch

from test_hypertile_gpu import TINY, close, tiny_model

pytestmark = pytest.mark.gpu

#        (n_img, hh, ww, s, heads)
SHAPES = [(2, 6, 10, 2, 1),       # Tk = 15: one partial tile, odd kw, a partial query block
          (3, 18, 32, 2, 2),      # Tk = 144: 2 1/4 tiles; S = 576
          (1, 9, 16, 2, 5),       # odd hh: the last row is never a key; five heads, ldq = 3 * 320
          (2, 7, 9, 3, 1),        # neither side divisible; Tk = 6
          (1, 4, 144, 2, 1),      # kw = 72 > 64: a tile inside one key run
          (1, 36, 64, 2, 2),      # Tk = 576: nine whole tiles, 64 queries per wave
          (1, 16, 32, 4, 1)]      # s = 4
_CACHE = {}


def case(shape):
    """(qkv fp16 [M][3C] on the host, float64 reference [M][C]), built once per shape and shared."""
    if shape not in _CACHE:
        from vdx.kvdown import key_rows
        n_img, hh, ww, s, heads = shape
        S, C = hh * ww, heads * 64
        qkv = torch.randn(n_img * S, 3 * C, generator=torch.Generator().manual_seed(hh * 100 + ww)).half()
        ref = torch.zeros(n_img * S, C, dtype=torch.float64)
        for n, rows in enumerate(key_rows(n_img, hh, ww, s)):
            q = qkv[n * S:(n + 1) * S, :C].double().view(-1, heads, 64).transpose(0, 1)
            k, v = (qkv[rows][:, j * C:(j + 1) * C].double().view(-1, heads, 64).transpose(0, 1) for j in (1, 2))
            ref[n * S:(n + 1) * S] = (torch.softmax(q @ k.transpose(1, 2) / 8, -1) @ v).transpose(0, 1).reshape(-1, C)
        _CACHE[shape] = (qkv, ref)
    return _CACHE[shape]


def run(gpu, qkv, shape, n_img=None):
    from vdx import ops
    _, hh, ww, s, heads = shape
    C = heads * 64
    x = qkv.to(gpu)
    return ops.flash_attn_kvdown(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], n_img=n_img or shape[0], hh=hh, ww=ww, s=s, heads=heads, scale=0.125)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(gpu, shape):
    qkv, ref = case(shape)
    out = run(gpu, qkv, shape)
    print(f"flash_attn_kvdown {shape}: max |out - float64| = {(out.cpu().double() - ref).abs().max().item():.3e}, max |ref| = {ref.abs().max().item():.3e}")
    close(out, ref.float(), tol=4e-3)


@pytest.mark.parametrize("shape", [(3, 18, 32, 2, 2), (2, 7, 9, 3, 1)], ids=str)
def test_non_key_rows_are_never_read(gpu, shape):
    """K and V of every row that is not a key are NaN, q is clean: the output is finite and has the clean run's bits."""
    from vdx.kvdown import key_rows
    qkv, _ = case(shape)
    n_img, hh, ww, s, heads = shape
    not_key = torch.ones(n_img * hh * ww, dtype=torch.bool)
    not_key[key_rows(n_img, hh, ww, s).flatten()] = False
    bad = qkv.clone()
    bad[not_key, heads * 64:] = float("nan")
    out = run(gpu, bad, shape)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, run(gpu, qkv, shape))


def test_images_are_isolated_and_bits_repeat(gpu):
    """Every image but one is NaN in q, k and v: that image's output is finite and the bits it has on the clean input; the
    same bits run to run, and from one call per image."""
    shape = (3, 18, 32, 2, 2)
    qkv, _ = case(shape)
    clean, S = run(gpu, qkv, shape), 18 * 32
    assert torch.equal(run(gpu, qkv, shape), clean)
    for n in range(3):
        mine = slice(n * S, (n + 1) * S)
        bad = torch.full_like(qkv, float("nan"))
        bad[mine] = qkv[mine]
        out = run(gpu, bad, shape)[mine]
        assert bool(torch.isfinite(out).all()) and torch.equal(out, clean[mine])
        assert torch.equal(run(gpu, qkv[mine], shape, n_img=1), clean[mine])


@pytest.mark.parametrize("shape", [(3, 18, 32, 2, 2), (1, 36, 64, 2, 2)], ids=str)
def test_equals_flash_attn_on_gathered_keys(gpu, shape):
    """Bit for bit: the kernel runs `flash_attn`'s tile, in its order, with its queries per wave, on the keys where they lie."""
    from vdx import ops
    from vdx.kvdown import key_rows
    n_img, hh, ww, s, heads = shape
    C, S = heads * 64, hh * ww
    x = case(shape)[0].to(gpu)
    rows = key_rows(n_img, hh, ww, s)
    kv = x[rows.flatten().to(gpu)][:, C:].contiguous()
    want = ops.flash_attn(x[:, :C], kv[:, :C], kv[:, C:], n_seq=n_img, sq=S, skv=rows.shape[1], skv_pad=rows.shape[1], heads=heads,
                          seq_per_kv=1, scale=0.125, v_rows=True)
    assert torch.equal(run(gpu, case(shape)[0], shape), want)


def test_library_refusals(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    x = torch.zeros(2 * 6 * 10, 192, dtype=torch.float16, device=gpu)
    for n_img, s in ((2, 1), (2, 7), (3, 2)):         # the plain attention's factor; s > hh; rows for two images only
        with pytest.raises(VdxError):
            ops.flash_attn_kvdown(x[:, :64], x[:, 64:128], x[:, 128:], n_img=n_img, hh=6, ww=10, s=s, heads=1, scale=0.125)


def test_self_attention_stage_bit_for_bit(gpu):
    """`_self_attention` with the option is LayerNorm + q|k|v GEMM + gather + `flash_attn` + `to_out`, composed by hand."""
    from vdx import ops
    from vdx.kvdown import key_rows
    m = tiny_model(gpu).enable_kv_downsample(2)
    p, b = "down_blocks.0.attentions.0", "down_blocks.0.attentions.0.transformer_blocks.0"
    n_img, hh, ww, C = 3, 9, 14, 64
    S = hh * ww
    M = n_img * S
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(23)).half().to(gpu)
    t = m._norm_proj_in(p, x, n_img, S, M)
    got = m._self_attention(b, t, n_img, hh, ww, 1)
    W = m.W
    ln = ops.layernorm(t, W[b + ".norm1.weight"], W[b + ".norm1.bias"], M=M)
    qkv = ops.gemm(ln, W[b + ".attn1.to_qkv.weight"], M=M)
    rows = key_rows(n_img, hh, ww, 2)
    kv = qkv[rows.flatten().to(gpu)][:, C:].contiguous()
    o = ops.flash_attn(qkv[:, :C], kv[:, :C], kv[:, C:], n_seq=n_img, sq=S, skv=rows.shape[1], skv_pad=rows.shape[1], heads=1,
                       seq_per_kv=1, scale=64 ** -0.5, v_rows=True)
    want = ops.gemm(o, W[b + ".attn1.to_out.0.weight"], M=M, bias=W[b + ".attn1.to_out.0.bias"], residual=t)
    assert torch.equal(got, want)
    plain = tiny_model(gpu)._self_attention(b, t, n_img, hh, ww, 1)
    assert not torch.equal(got, plain)
    assert torch.equal(m._self_attention(b, t, n_img, hh, ww, 2), plain)              # above max_downsample
    m.enable_kv_downsample(2, max_downsample=2)                                         # level 1: factor 2 // 2 = 1, the plain attention
    assert torch.equal(m._self_attention(b, t, n_img, hh, ww, 2), plain)


def test_unet_with_kv_downsample(gpu):
    from vdx import ops
    m, never = tiny_model(gpu), tiny_model(gpu)
    g = torch.Generator().manual_seed(21)
    lat = torch.randn(1, 4, 4, 16, 32, generator=g).half().to(gpu)
    e = torch.randn(2, 77, TINY["cross"], generator=g).half().to(gpu)
    x = ops.cfg_input(lat, None, 0.0)
    off = never(x, 7, encoder_hidden_states=e).sample
    m.enable_kv_downsample()
    assert m.kv_downsample == {"factor": 2, "max_downsample": 1}
    on = m(x, 7, encoder_hidden_states=e).sample
    assert bool(torch.isfinite(on.float()).all()) and not torch.equal(on, off)
    assert torch.equal(m(x, 7, encoder_hidden_states=e).sample, on)                    # run to run
    rel = float((on.double() - off.double()).norm() / off.double().norm())
    print(f"kv_downsample 2: rel-L2 {rel:.3e} from the forward without (synthetic weights)")
    deep = m.enable_kv_downsample(4, max_downsample=2)(x, 7, encoder_hidden_states=e).sample     # level 0: 4, level 1: 2
    assert bool(torch.isfinite(deep.float()).all()) and not torch.equal(deep, on)
    for other in (lambda: m.enable_tome(0.5), lambda: m.enable_hypertile(2, 2), lambda: m.enable_cross_frame("first"), lambda: m.enable_kv_downsample(1)):
        with pytest.raises(ValueError):
            other()
    assert m.kv_downsample == {"factor": 4, "max_downsample": 2} and m.tome is None    # a refusal leaves the state
    m.disable_kv_downsample()
    assert m.kv_downsample is None and torch.equal(m(x, 7, encoder_hidden_states=e).sample, off)
    for enable in (lambda: m.enable_tome(0.5), lambda: m.enable_hypertile(2, 2), lambda: m.enable_cross_frame("first")):
        enable()
        with pytest.raises(ValueError):
            m.enable_kv_downsample()
        m.disable_tome().disable_hypertile().disable_cross_frame()
