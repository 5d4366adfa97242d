"""HyperTile on the GPU: `ops.flash_attn_win` (csrc/flash_win.hip) against the float64 definition on the row map, window
isolation, determinism, the `_self_attention` stage and the UNet switch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
#        (n_img, hh, ww, ny, nx, heads)
SHAPES = [(2, 6, 10, 2, 2, 1),      # T = 15: one partial tile, odd tw
          (3, 18, 32, 2, 2, 2),     # T = 144: 2 1/4 tiles, a query-block tail
          (2, 36, 64, 2, 2, 2),     # T = 576: 64 queries per wave; pairs % 8 == 0
          (1, 12, 16, 1, 4, 5),     # row-only split; 20 pairs; five heads with ldq = 3 * 320
          (2, 12, 16, 3, 1, 1),     # column-only split
          (1, 16, 144, 1, 2, 1)]    # tw = 72 > 64: a tile inside one run
_CACHE = {}


def rows_of(n_img, hh, ww, ny, nx):
    """int64 [n_img ny nx][T]: the rows of every window's tokens, by the row map of include/vdx.h."""
    th, tw = hh // ny, ww // nx
    i = torch.arange(th * tw)
    win = [n * hh * ww + (wy * th + i // tw) * ww + wx * tw + i % tw for n in range(n_img) for wy in range(ny) for wx in range(nx)]
    return torch.stack(win)


def case(shape):
    """(qkv fp16 [M][3C] on the host, float64 reference [M][C]), built once per shape and shared."""
    if shape not in _CACHE:
        n_img, hh, ww, ny, nx, heads = shape
        M, C = n_img * hh * ww, heads * 64
        qkv = torch.randn(M, 3 * C, generator=torch.Generator().manual_seed(hh * 100 + ww)).half()
        ref = torch.zeros(M, C, dtype=torch.float64)
        for rows in rows_of(n_img, hh, ww, ny, nx):
            q, k, v = (qkv[rows][:, j * C:(j + 1) * C].double().view(-1, heads, 64).transpose(0, 1) for j in range(3))
            ref[rows] = (torch.softmax(q @ k.transpose(1, 2) / 8, -1) @ v).transpose(0, 1).reshape(-1, C)
        _CACHE[shape] = (qkv, ref)
    return _CACHE[shape]


def close(out, ref, tol):
    """tests/test_ops_gpu.py `close`: |out - ref| <= tol (max |ref| + |ref|) everywhere, and finite."""
    out = out.float().cpu()
    assert out.shape == ref.shape and torch.isfinite(out).all()
    err, bound = (out - ref).abs(), tol * (ref.abs().max().item() + 1e-6) + tol * ref.abs()
    assert not (err > bound).any(), f"max err {err.max().item():.4g}, {int((err > bound).sum())} / {err.numel()} bad"


def run(gpu, qkv, shape, n_img=None):
    from vdx import ops
    _, hh, ww, ny, nx, heads = shape
    C = heads * 64
    x = qkv.to(gpu)
    return ops.flash_attn_win(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], n_img=n_img or shape[0], hh=hh, ww=ww, ny=ny, nx=nx, heads=heads,
                              scale=0.125)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(gpu, shape):
    qkv, ref = case(shape)
    out = run(gpu, qkv, shape)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"flash_attn_win {shape}: max |out - float64| = {err:.3e}, max |ref| = {ref.abs().max().item():.3e}")
    close(out, ref.float(), tol=4e-3)


def test_windows_are_isolated(gpu):
    """Every window but one is NaN in q, k and v: that window's output is finite and the bits it has on the clean input (its
    tail tile stages nothing of a neighbour's)."""
    shape = (2, 18, 32, 2, 2, 2)
    qkv, _ = case((3, 18, 32, 2, 2, 2))
    qkv = qkv[:2 * 18 * 32]
    clean = run(gpu, qkv, shape)
    rows = rows_of(*shape[:5])
    for keep in (0, 3, 6):
        bad = torch.full_like(qkv, float("nan"))
        bad[rows[keep]] = qkv[rows[keep]]
        out = run(gpu, bad, shape)[rows[keep].to(gpu)]
        assert bool(torch.isfinite(out).all()) and torch.equal(out, clean[rows[keep].to(gpu)])


def test_deterministic_and_batch_independent(gpu):
    shape = (3, 18, 32, 2, 2, 2)
    qkv, _ = case(shape)
    out = run(gpu, qkv, shape)
    assert torch.equal(run(gpu, qkv, shape), out)
    S = 18 * 32
    for n in range(3):
        assert torch.equal(run(gpu, qkv[n * S:(n + 1) * S], shape, n_img=1), out[n * S:(n + 1) * S])


def test_library_refusals(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    x = torch.zeros(2 * 6 * 10, 192, dtype=torch.float16, device=gpu)
    for ny, nx in ((1, 1), (4, 2), (2, 3)):           # the plain attention's grid; grids that do not divide 6 x 10
        with pytest.raises(VdxError):
            ops.flash_attn_win(x[:, :64], x[:, 64:128], x[:, 128:], n_img=2, hh=6, ww=10, ny=ny, nx=nx, heads=1, scale=0.125)
    with pytest.raises(VdxError):                     # rows for two images only
        ops.flash_attn_win(x[:, :64], x[:, 64:128], x[:, 128:], n_img=3, hh=6, ww=10, ny=2, nx=2, heads=1, scale=0.125)


def tiny_model(gpu):
    import vdx  # noqa: F401
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from oracle.unet3d_ref import UNet3DConfig as RefCfg, synthetic_state_dict
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    cfg = UNet3DConfig(block_out_channels=TINY["ch"], cross_attention_dim=TINY["cross"], transformer_in_heads=TINY["in_heads"])
    return UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)


def test_self_attention_stage_bit_for_bit(gpu):
    from vdx import ops
    m = tiny_model(gpu).enable_hypertile(2, 2)
    p, b = "down_blocks.0.attentions.0", "down_blocks.0.attentions.0.transformer_blocks.0"
    n_img, hh, ww, C = 3, 10, 14, 64
    S = hh * ww
    M = n_img * S
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(23)).half().to(gpu)
    t = m._norm_proj_in(p, x, n_img, S, M)
    got = m._self_attention(b, t, n_img, hh, ww, 1)
    W = m.W
    ln = ops.layernorm(t, W[b + ".norm1.weight"], W[b + ".norm1.bias"], M=M)
    qkv = ops.gemm(ln, W[b + ".attn1.to_qkv.weight"], M=M)
    o = ops.flash_attn_win(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_img=n_img, hh=hh, ww=ww, ny=2, nx=2, heads=1, scale=64 ** -0.5)
    want = ops.gemm(o, W[b + ".attn1.to_out.0.weight"], M=M, bias=W[b + ".attn1.to_out.0.bias"], residual=t)
    assert torch.equal(got, want)
    plain = tiny_model(gpu)._self_attention(b, t, n_img, hh, ww, 1)
    assert not torch.equal(got, plain)
    assert torch.equal(m._self_attention(b, t, n_img, hh, ww, 2), plain)              # above max_downsample
    with pytest.raises(ValueError):                                                     # a level-0 grid that does not divide
        m._self_attention(b, t[:3 * 9 * 14], 3, 9, 14, 1)
    m.enable_hypertile(2, 2, max_downsample=2)                                          # level 1: grid 1 x 1, the plain attention
    assert torch.equal(m._self_attention(b, t, n_img, hh, ww, 2), plain)


def test_unet_with_hypertile(gpu):
    from vdx import ops
    m, never = tiny_model(gpu), tiny_model(gpu)
    g = torch.Generator().manual_seed(21)
    lat = torch.randn(1, 4, 4, 16, 32, generator=g).half().to(gpu)
    e = torch.randn(2, 77, TINY["cross"], generator=g).half().to(gpu)
    x = ops.cfg_input(lat, None, 0.0)
    off = never(x, 7, encoder_hidden_states=e).sample
    m.enable_hypertile(2, 2)
    assert m.hypertile == {"grid": (2, 2), "max_downsample": 1}
    on = m(x, 7, encoder_hidden_states=e).sample
    assert m.last_forward_shared_prefix
    assert bool(torch.isfinite(on.float()).all()) and not torch.equal(on, off)
    assert torch.equal(m(x, 7, encoder_hidden_states=e).sample, on)                    # run to run
    dup = m(x.clone(), 7, encoder_hidden_states=e).sample                              # the shared prefix off
    assert not m.last_forward_shared_prefix and torch.equal(dup, on)
    rel = float((on.double() - off.double()).norm() / off.double().norm())
    print(f"hypertile 2 x 2: rel-L2 {rel:.3e} from the forward without (synthetic weights)")
    deep = m.enable_hypertile(4, 4, max_downsample=2)(x, 7, encoder_hidden_states=e).sample      # level 0: 4 x 4, level 1: 2 x 2
    assert bool(torch.isfinite(deep.float()).all()) and not torch.equal(deep, on)
    assert torch.equal(m.enable_hypertile(1, 1)(x, 7, encoder_hidden_states=e).sample, off)
    m.enable_hypertile(2, 2)
    with pytest.raises(ValueError):
        m.enable_tome(0.5)
    with pytest.raises(ValueError):
        m.enable_hypertile(0, 2)
    assert m.tome is None and m.hypertile == {"grid": (2, 2), "max_downsample": 1}   # a refusal leaves the state
    m.disable_hypertile()
    assert m.hypertile is None and torch.equal(m(x, 7, encoder_hidden_states=e).sample, off)
    m.enable_tome(0.5)
    with pytest.raises(ValueError):
        m.enable_hypertile(2, 2)
    assert m.hypertile is None and m.tome is not None
