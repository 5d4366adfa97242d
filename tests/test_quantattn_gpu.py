"""The INT8 score product on the GPU: `ops.attn_quant_i8` against the torch-CPU restatement of the quantiser,
`ops.flash_attn_i8` against float64 attention on the kernel's own quantised operands (tests/quantattn_ref.py), the corner cases
of the definition, and the UNet switch."""
import os

import numpy as np
import pytest
import torch

import quantattn_ref as R
from test_hypertile_gpu import TINY, close, tiny_model

pytestmark = pytest.mark.gpu

#        (n_img, S, heads)
SHAPES = [(1, 64, 1),        # one block, one tile
          (4, 65, 2),        # a last block of one token; 8 pairs: the XCD block order
          (2, 72, 1),        # 9 x 8: a short last block, tail rows
          (1, 144, 2),       # the level-3 frame: 2 1/4 tiles, a query-block tail
          (3, 576, 2)]       # 18 x 32: 64 queries per wave, nine whole tiles, three query blocks of which the last is partial
SCALE = 0.125
_CACHE = {}


def case(shape):
    """qkv fp16 [n_img*S][3C] on the host, seeded, built once per shape."""
    if shape not in _CACHE:
        n_img, S, heads = shape
        _CACHE[shape] = torch.randn(n_img * S, 3 * heads * 64, generator=torch.Generator().manual_seed(S * 10 + n_img)).half()
    return _CACHE[shape]


def run(gpu, qkv, shape, n_img=None, readback=False):
    """`flash_attn_i8` on the column blocks of qkv; with `readback` also the pre-pass's (q8, k8, dq, dk) on the host."""
    from vdx import ops
    _, S, heads = shape
    n_img, C = n_img or shape[0], heads * 64
    x = qkv.to(gpu)
    ws = ops.attn_quant_i8_workspace(n_img, S, heads, gpu)
    out = ops.flash_attn_i8(x[:, :C], x[:, C:2 * C], x[:, 2 * C:], n_img=n_img, S=S, heads=heads, scale=SCALE, workspace=ws)
    return (out, [t.cpu() for t in ops._quant_i8_views(ws, n_img, S, heads)]) if readback else out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prepass_against_the_restatement(gpu, shape):
    """delta bit for bit, every int8 value within one level, at most 1e-3 of them different at all (on the CPU the
    restatement's quotients on these inputs lie within 1e-4 of a half-way point for under 3e-4 of the values)."""
    from vdx import ops
    n_img, S, heads = shape
    C, x = heads * 64, case(shape).to(gpu)
    got = [t.cpu() for t in ops.attn_quant_i8(x[:, :C], x[:, C:2 * C], n_img=n_img, S=S, heads=heads, scale=SCALE)]
    want = R.quantiser(case(shape)[:, :C], case(shape)[:, C:2 * C], n_img, S, heads, SCALE)
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    for name, g, w in (("q8", got[0], want[0]), ("k8", got[1], want[1])):
        diff = (g.int() - w.int()).abs()
        share = float((diff != 0).float().mean())
        print(f"attn_quant_i8 {shape} {name}: {int((diff != 0).sum())} of {diff.numel()} values differ from the restatement ({share:.2e})")
        assert int(diff.max()) <= 1 and share <= 1e-3
        assert not bool(g[:, :, S:].any())                                      # tail rows


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64_on_its_own_operands(gpu, shape):
    n_img, S, heads = shape
    qkv = case(shape)
    out, (q8, k8, dq, dk) = run(gpu, qkv, shape, readback=True)
    ref = R.attention64(q8, k8, dq, dk, qkv[:, 2 * heads * 64:], S)
    print(f"flash_attn_i8 {shape}: max |out - float64| = {(out.cpu().double() - ref).abs().max().item():.3e}, max |ref| = {ref.abs().max().item():.3e}")
    close(out, ref.float(), tol=4e-3)


@pytest.mark.parametrize("mean", [1.0, 50.0], ids=lambda m: f"mean{m:g}")
def test_a_constant_added_to_every_key_changes_nothing(gpu, mean):
    """k + c against k: the key mean takes c out before the quantiser sees it.  k lies on a grid of 2^-5 inside +-4 and c on the
    same grid, so k + c is exact in fp16; at 50 the mean is 50 times the keys' spread, and without the smoothing the block
    scale would be 50 / 127 = 0.4 against a spread of 1."""
    shape = (2, 72, 1)
    qkv = case(shape).clone()
    qkv[:, 64:128] = (qkv[:, 64:128].float().clamp(-4, 4) * 32).round() / 32
    c = (torch.randn(64, generator=torch.Generator().manual_seed(5)).sign() * mean * 32).round() / 32
    moved = qkv.clone()
    moved[:, 64:128] = (qkv[:, 64:128].float() + c).half()
    assert torch.equal(moved[:, 64:128].float(), qkv[:, 64:128].float() + c)
    base = run(gpu, qkv, shape)
    out, (_, _, _, dk) = run(gpu, moved, shape, readback=True)
    assert float(dk.max()) * 127 <= 8.5                                         # the scale is the spread's, not the mean's
    close(out, base.float().cpu(), tol=4e-3)


def test_an_all_zero_block_runs_clean(gpu):
    shape = (1, 144, 2)
    qkv = case(shape).clone()
    qkv[64:128, :128] = 0                  # q: block 1 of both heads
    qkv[:, 192:256] = 0                    # k: all of head 1 (its mean is 0, every block of K' is zero: uniform attention)
    out, (q8, k8, dq, dk) = run(gpu, qkv, shape, readback=True)
    assert bool((dq[0, :, 1] == 1).all()) and bool((dk[0, 1] == 1).all()) and not bool(q8[0, :, 64:128].any()) and not bool(k8[0, 1].any())
    close(out, R.attention64(q8, k8, dq, dk, qkv[:, 256:], 144).float(), tol=4e-3)
    close(out[:, 64:], qkv[:, 320:].float().mean(0).expand(144, 64), tol=4e-3)


def test_bits_repeat_and_images_are_isolated(gpu):
    """The same bits run to run and from one call per image; a NaN row of q, k and v in image 1, head 0 leaves every other
    (image, head) its bits."""
    shape = (3, 144, 2)
    qkv, S = case(shape), 144
    clean = run(gpu, qkv, shape)
    assert torch.equal(run(gpu, qkv, shape), clean) and bool(torch.isfinite(clean).all())
    for n in range(3):
        assert torch.equal(run(gpu, qkv[n * S:(n + 1) * S], shape, n_img=1), clean[n * S:(n + 1) * S])
    bad = qkv.clone()
    for j in range(3):
        bad[S + 70, j * 128:j * 128 + 64] = float("nan")
    out = run(gpu, bad, shape)
    keep = torch.ones(3 * S, 128, dtype=torch.bool)
    keep[S:2 * S, :64] = False
    assert torch.equal(out.cpu()[keep], clean.cpu()[keep]) and not bool(torch.isfinite(out[S:2 * S, :64]).any())


def test_library_refusals(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    x = torch.zeros(2 * 72, 3 * 64, dtype=torch.float16, device=gpu)
    q, k, v = x[:, :64], x[:, 64:128], x[:, 128:]
    small = torch.empty(64, dtype=torch.uint8, device=gpu)
    with pytest.raises(VdxError):
        ops.flash_attn_i8(q, k, v, n_img=3, S=72, heads=1, scale=SCALE)                      # rows for two images only
    with pytest.raises(VdxError):
        ops.flash_attn_i8(q, k, v, n_img=2, S=72, heads=1, scale=SCALE, workspace=small)     # an undersized workspace
    with pytest.raises(VdxError):
        ops.flash_attn_i8(q[:, :32], k[:, :32], v[:, :32], n_img=2, S=72, heads=1, scale=SCALE)   # a head dimension of 32
    with pytest.raises(VdxError):
        ops.flash_attn_i8(q, k, v, n_img=2, S=72, heads=1, scale=SCALE, out=v)              # out overlaps v
    with pytest.raises(VdxError):
        ops.flash_attn_i8(x[:, 4:68], k, v, n_img=2, S=72, heads=1, scale=SCALE)             # q 8 bytes off a 16-byte boundary


# rel-L2 of the tiny golden forward with enable_quant_attn(8) against the fp32 oracle's stored result, measured on an MI355X
# (profiles/quantattn_parity.txt); the test allows twice that: the margin covers the seed-to-seed spread of a quantisation error
UNET_PARITY = {"a": 1.771e-3, "b": 1.729e-3}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_unet_with_quant_attn(gpu, tag):
    from test_unet_gpu import GOLD, rel_l2, tiny_inputs
    gold = np.load(os.path.join(GOLD, f"unet_tiny_{tag}.npz"))
    F, H, W, t = (int(v) for v in gold["shape"])
    m = tiny_model(gpu)
    sample, ehs = tiny_inputs(F, H, W)
    args = (sample.to(gpu), torch.tensor(t, device=gpu))
    off = m(*args, encoder_hidden_states=ehs.to(gpu)).sample
    assert m.enable_quant_attn(8).quant_attn == {"mode": "qk_int8", "max_downsample": 8}
    on = m(*args, encoder_hidden_states=ehs.to(gpu)).sample
    assert not torch.equal(on, off) and torch.equal(m(*args, encoder_hidden_states=ehs.to(gpu)).sample, on)
    ref = torch.from_numpy(gold["out"])
    err = rel_l2(on.float().cpu(), ref)
    print(f"unet_tiny_{tag} with quant_attn(8): rel-L2 {err:.3e} from the fp32 oracle ({rel_l2(off.float().cpu(), ref):.3e} without, "
          f"{rel_l2(on.float().cpu(), off.float().cpu()):.3e} between the two)")
    assert err <= 2.0 * UNET_PARITY[tag]
    for other in (lambda: m.enable_tome(0.5), lambda: m.enable_hypertile(2, 2), lambda: m.enable_cross_frame("first"),
                  lambda: m.enable_kv_downsample(2), lambda: m.enable_quant_attn(3)):
        with pytest.raises(ValueError):
            other()
    assert m.quant_attn == {"mode": "qk_int8", "max_downsample": 8} and m.tome is None    # a refusal leaves the state
    m.disable_quant_attn()
    assert m.quant_attn is None and torch.equal(m(*args, encoder_hidden_states=ehs.to(gpu)).sample, off)
    for enable in (lambda: m.enable_tome(0.5), lambda: m.enable_hypertile(2, 2), lambda: m.enable_cross_frame("first"),
                   lambda: m.enable_kv_downsample(2)):
        enable()
        with pytest.raises(ValueError):
            m.enable_quant_attn()
        m.disable_tome().disable_hypertile().disable_cross_frame().disable_kv_downsample()
