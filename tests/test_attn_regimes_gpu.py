"""-m gpu: the attention sub-block kernels — the temporal core (csrc/attn.hip), K7 (csrc/tattn_fused.hip), K7b
(csrc/tattn2.hip) and K5 (csrc/xattn.hip) — outside the one regime tests/test_ops_gpu.py holds them in: a peaked softmax
(one_hot), exact two-way ties, rows with a large mean and outlier channels, an exactly flat softmax; every F the fused kernels
accept; and what the key masks promise — a pixel's output depends on its own frames only, a K5 row on its own item's real keys
only, bit for bit.  The reference is the float64 statement of the sub-block (tests/attn_regimes_ref.py), the bound is the
close() bound of the kernel's sibling test; tests/test_attn_regimes_host.py shows on the CPU that the kernels' own fp16 roundings
use at most half of it in every case run here."""
import pytest
import torch

import attn_regimes_ref as R

pytestmark = pytest.mark.gpu

TEMPORAL_KERNELS = [("core", 320), ("k7", 320), ("k7", 512), ("k7b", 320)]


def _ops():
    import vdx  # noqa: F401
    from vdx import ops, packing
    return ops, packing


def _temporal_input(kernel, c):
    """The rows the kernel reads: t [M][inner], or for the core the fp16 q|k|v rows [M][3 * inner] of the un-fused chain."""
    return R.core_qkv(c) if kernel == "core" else c.t


def _temporal_exact(kernel, c):
    if kernel == "core":
        return R.exact_core(R.core_qkv(c), c.B, c.F, c.HW, c.heads)[0]
    return R.exact_temporal(c)[0]


def _temporal_launcher(kernel, c, gpu):
    """-> f(rows on the CPU) -> the kernel's output; the weights are packed once."""
    ops, packing = _ops()
    d = lambda x: x.half().to(gpu)   # noqa: E731
    dims = dict(B=c.B, F=c.F, HW=c.HW)
    if kernel == "core":
        return lambda x: ops.temporal_attn(d(x), heads=c.heads, scale=R.SCALE, **dims)
    if kernel == "k7":
        assert ops.temporal_attn_block_supported(c.inner, c.F)
        w = [d(c.gamma), d(c.beta), d(packing.pack_k7_qkv(c.wq, c.wk, c.wv)), d(packing.pack_k7_out(c.wo)), d(c.bo)]
        return lambda x: ops.temporal_attn_block(d(x), *w, scale=R.SCALE, **dims)
    assert ops.temporal_attn_block2_supported(c.inner, c.F)
    blob = packing.pack_k7b(c.wq, c.wk, c.wv, c.wo, c.gamma, c.beta, c.bo, R.SCALE).to(gpu)
    return lambda x: ops.temporal_attn_block2(d(x), blob, **dims)


def _cross_launcher(c, gpu, junk_seed=None):
    """-> f(rows on the CPU) -> K5's output.  The text keys / values as the un-fused path keeps them (k rows of the zero-padded
    text, V^T); `junk_seed`: every slot at or past kv_len then holds finite values of magnitude 50 .. 100 instead of zeros."""
    ops, packing = _ops()
    d = lambda x: x.half().to(gpu)   # noqa: E731
    assert ops.cross_attn_block_supported(c.inner, c.kv_len)
    ehs_pad = d(R.padded_text(c))
    k_rows = ops.gemm(ehs_pad, d(c.wk), M=c.n_items * R.PAD)
    vt = ops.gemm(d(c.wv), ehs_pad, M=c.inner)
    if junk_seed is not None:
        k_rows, vt = R.fill_padding(k_rows, vt, c.n_items, c.kv_len, junk_seed)
    blob = packing.pack_k5(c.wq, c.wo, c.gamma, c.beta, c.bo, R.SCALE).to(gpu)
    kvb = packing.pack_k5_kv(k_rows, vt, c.n_items, R.PAD)
    return lambda x: ops.cross_attn_block(d(x), blob, kvb, kv_len=c.kv_len, n_items=c.n_items, rows_per_item=c.rows)


def _within_bound(out, exact, tol, what):
    assert bool(torch.isfinite(out.float()).all()), what
    ratio = R.err_over_bound(out, exact, tol)
    print(f"\nkernel/exact {what}: {ratio:.3f} of the bound")
    assert ratio <= 1.0, f"{what}: error is {ratio:.3f} of the bound"


# ---- 1. the regimes against the float64 statement
@pytest.mark.parametrize("B,Fr,HW", R.TEMPORAL_SHAPES)
@pytest.mark.parametrize("kernel,inner", TEMPORAL_KERNELS)
@pytest.mark.parametrize("regime", R.REGIMES)
def test_temporal_regimes(gpu, regime, kernel, inner, B, Fr, HW):
    c = R.temporal_case(regime, inner, B, Fr, HW)
    run, x = _temporal_launcher(kernel, c, gpu), _temporal_input(kernel, c)
    out = run(x)
    _within_bound(out, _temporal_exact(kernel, c), R.TOL[kernel], f"{kernel}-{inner} {regime} (B,F,HW)=({B},{Fr},{HW})")
    assert torch.equal(out, run(x))


@pytest.mark.parametrize("n_items,rows,kv_len", R.CROSS_SHAPES)
@pytest.mark.parametrize("regime", R.REGIMES)
def test_cross_regimes(gpu, regime, n_items, rows, kv_len):
    c = R.cross_case(regime, n_items, rows, kv_len)
    run = _cross_launcher(c, gpu)
    out = run(c.t)
    _within_bound(out, R.exact_cross(c)[0], R.TOL["k5"], f"k5 {regime} (items,rows,kv)=({n_items},{rows},{kv_len})")
    assert torch.equal(out, run(c.t))


# ---- 2. every F the fused temporal kernels accept (F < 16: several pixels share a 16-row MFMA tile)
@pytest.mark.parametrize("Fr", [1, 2, 3, 4, 6, 8, 12, 16, 24, 48])
@pytest.mark.parametrize("kernel,inner", TEMPORAL_KERNELS[1:])
def test_every_supported_f(gpu, kernel, inner, Fr):
    c = R.temporal_case("ordinary", inner, 2, Fr, 11)
    out = _temporal_launcher(kernel, c, gpu)(c.t)
    _within_bound(out, R.exact_temporal(c)[0], R.TOL[kernel], f"{kernel}-{inner} ordinary F={Fr}")


def test_supported_f_is_the_divisors_of_48(gpu):
    ops, _ = _ops()
    for Fr in (1, 2, 3, 4, 6, 8, 12, 16, 24, 48):
        assert ops.temporal_attn_block_supported(320, Fr) and ops.temporal_attn_block_supported(512, Fr)
        assert ops.temporal_attn_block2_supported(320, Fr)
    for Fr in (5, 7, 32, 96):
        assert not ops.temporal_attn_block_supported(320, Fr) and not ops.temporal_attn_block_supported(512, Fr)
        assert not ops.temporal_attn_block2_supported(320, Fr)


# ---- 3. a pixel's output depends on its own frames only
@pytest.mark.parametrize("Fr", [2, 4, 8, 12, 24])
@pytest.mark.parametrize("kernel,inner", TEMPORAL_KERNELS)
def test_pixel_depends_on_its_own_rows_only(gpu, kernel, inner, Fr):
    """HW = 13: the last tile is ragged and, for F < 16, several pixels share a tile.  Every row but those of pixels 0, 5 and
    12 of item 0 is replaced by another draw four times as large (finite values only: a masked weight of exactly 0 times a
    non-finite v is NaN in any MFMA); the kept pixels' output rows must not move by a bit."""
    B, HW = 2, 13
    c = R.temporal_case("ordinary", inner, B, Fr, HW)
    run, x = _temporal_launcher(kernel, c, gpu), _temporal_input(kernel, c)
    keep = R.pixel_rows(B, Fr, HW, 0, (0, 5, 12))
    x2 = R.redraw_except(x, keep, seed=1000 + Fr)
    out, out2 = run(x), run(x2)
    assert bool(torch.isfinite(out2.float()).all())
    assert torch.equal(out[keep.to(gpu)], out2[keep.to(gpu)])
    assert not torch.equal(out, out2)


# ---- 4. K5 never uses a padded key
@pytest.mark.parametrize("kv_len", [1, 15, 16, 17, 31, 32, 33, 64, 65, 79, 80])
def test_cross_never_uses_a_padded_key(gpu, kv_len):
    """Texts of one token, of a whole number of 16-key tiles and of one key more or less: the slots past kv_len (up to the pad
    of 128) hold zeros in one run and values of magnitude 50 .. 100 in the other; the outputs must be the same bits."""
    ops, _ = _ops()
    assert not ops.cross_attn_block_supported(320, 0) and not ops.cross_attn_block_supported(320, 81)
    c = R.cross_case("ordinary", 2, 70, kv_len)
    out = _cross_launcher(c, gpu)(c.t)
    _within_bound(out, R.exact_cross(c)[0], R.TOL["k5"], f"k5 ordinary kv_len={kv_len}")
    assert torch.equal(out, _cross_launcher(c, gpu, junk_seed=kv_len)(c.t))


# ---- 5. K5 rows are independent
def test_cross_rows_are_independent(gpu):
    """All rows of item 1 and rows 10 .. of item 0 are replaced by another draw: rows 0 .. 9 of item 0 keep their bits."""
    c = R.cross_case("ordinary", 2, 70, 77)
    run = _cross_launcher(c, gpu)
    keep = torch.arange(10)
    out, out2 = run(c.t), run(R.redraw_except(c.t, keep, seed=77))
    assert bool(torch.isfinite(out2.float()).all())
    assert torch.equal(out[:10], out2[:10]) and not torch.equal(out[10:], out2[10:])
