"""No GPU: the inputs and references of tests/attn_regimes_ref.py.  For every case the GPU file runs, `rounded` (fp32 with the
kernel's fp16 roundings) must lie within HALF the kernel's bound of `exact` (float64) — so that holding the kernel to the full
bound is fair in the peaked regimes — and the regimes must be what they claim on `exact` alone: one_hot at least 90 % one-hot
with a 10-nat margin, every two_way_tie top pair exactly equal, every flat weight exactly 1 / keys.  Run with -s to see the
measured ratio of every case (the table in attn_regimes_ref.py's docstring is taken from that output)."""
import pytest
import torch

import attn_regimes_ref as R

ALL = ("ordinary",) + R.REGIMES
TEMPORAL_KERNELS = [("core", 320), ("k7", 320), ("k7", 512), ("k7b", 320)]


def _temporal_pair(kernel, c):
    """-> (rounded, exact, P, scores) of `kernel` on temporal case c."""
    if kernel == "core":
        qkv = R.core_qkv(c)
        exact, p, s = R.exact_core(qkv, c.B, c.F, c.HW, c.heads)
        return R.rounded_core(qkv, c.B, c.F, c.HW, c.heads), exact, p, s
    exact, p, s = R.exact_temporal(c)
    return (R.rounded_k7 if kernel == "k7" else R.rounded_k7b)(c), exact, p, s


@pytest.mark.parametrize("B,Fr,HW", R.TEMPORAL_SHAPES)
@pytest.mark.parametrize("kernel,inner", TEMPORAL_KERNELS)
@pytest.mark.parametrize("regime", ALL)
def test_temporal_rounded_within_half_the_bound(regime, kernel, inner, B, Fr, HW):
    c = R.temporal_case(regime, inner, B, Fr, HW)
    rounded, exact, _, _ = _temporal_pair(kernel, c)
    ratio = R.err_over_bound(rounded, exact, R.TOL[kernel])
    print(f"\nrounded/exact {kernel}-{inner} {regime} (B,F,HW)=({B},{Fr},{HW}): {ratio:.3f} of the bound")
    assert torch.isfinite(rounded).all() and ratio <= 0.5


@pytest.mark.parametrize("n_items,rows,kv_len", R.CROSS_SHAPES)
@pytest.mark.parametrize("regime", ALL)
def test_cross_rounded_within_half_the_bound(regime, n_items, rows, kv_len):
    c = R.cross_case(regime, n_items, rows, kv_len)
    exact, _, _ = R.exact_cross(c)
    rounded = R.rounded_k5(c)
    ratio = R.err_over_bound(rounded, exact, R.TOL["k5"])
    print(f"\nrounded/exact k5 {regime} (items,rows,kv)=({n_items},{rows},{kv_len}): {ratio:.3f} of the bound")
    assert torch.isfinite(rounded).all() and ratio <= 0.5


@pytest.mark.parametrize("kv_len", [1, 15, 16, 17, 31, 32, 33, 64, 65, 79, 80])
def test_cross_kv_len_edges_rounded_within_half_the_bound(kv_len):
    c = R.cross_case("ordinary", 2, 70, kv_len)
    ratio = R.err_over_bound(R.rounded_k5(c), R.exact_cross(c)[0], R.TOL["k5"])
    print(f"\nrounded/exact k5 ordinary kv_len={kv_len}: {ratio:.3f} of the bound")
    assert ratio <= 0.5


@pytest.mark.parametrize("Fr", [1, 2, 3, 4, 6, 8, 12, 16, 24, 48])
@pytest.mark.parametrize("kernel,inner", TEMPORAL_KERNELS[1:])
def test_every_supported_f_rounded_within_half_the_bound(kernel, inner, Fr):
    c = R.temporal_case("ordinary", inner, 2, Fr, 11)
    rounded, exact, _, _ = _temporal_pair(kernel, c)
    ratio = R.err_over_bound(rounded, exact, R.TOL[kernel])
    print(f"\nrounded/exact {kernel}-{inner} ordinary F={Fr}: {ratio:.3f} of the bound")
    assert ratio <= 0.5


def _pairs(kind):
    if kind == "temporal":
        for inner in (320, 512):
            for shape in R.TEMPORAL_SHAPES:
                yield lambda regime, inner=inner, shape=shape: R.temporal_case(regime, inner, *shape), R.exact_temporal, f"{inner} {shape}"
        for shape in R.TEMPORAL_SHAPES:       # the core sees the fp16 q|k|v rows of the 320-wide case
            yield (lambda regime, shape=shape: R.temporal_case(regime, 320, *shape),
                   lambda c: R.exact_core(R.core_qkv(c), c.B, c.F, c.HW, c.heads), f"core {shape}")
    else:
        for shape in R.CROSS_SHAPES:
            yield lambda regime, shape=shape: R.cross_case(regime, *shape), R.exact_cross, f"k5 {shape}"


@pytest.mark.parametrize("kind", ["temporal", "cross"])
def test_one_hot_share(kind):
    for case, exact, name in _pairs(kind):
        _, p, s = exact(case("one_hot"))
        share = R.one_hot_share(p, s)
        if not name.startswith("core"):      # the builders keep only rows whose every (query, head) pair has the margin
            sv = s.topk(2, dim=-1).values
            assert float((sv[..., 0] - sv[..., 1]).min()) >= R.MARGIN, name
        print(f"\none_hot {name}: {100 * share:.1f} % of (query, head) pairs one-hot with a 10-nat margin")
        assert share >= 0.90, name


@pytest.mark.parametrize("kind", ["temporal", "cross"])
def test_two_way_ties_are_exact(kind):
    for case, exact, name in _pairs(kind):
        c = case("two_way_tie")
        _, p, _ = exact(c)
        keys = p.shape[-1]
        half = keys // 2
        w1, w2, i1 = R.top_two(p)
        assert torch.equal(w1, w2), name                                     # the split is exact ...
        assert torch.equal(p[..., :half], p[..., half:2 * half]), name       # ... between a key and its copy
        assert bool((i1 < 2 * half).all()), name                             # (never the zero token an odd text ends in)
        share = float((w1 >= 0.4995).double().mean())
        print(f"\ntwo_way_tie {name}: {100 * share:.1f} % of pairs split 0.5 / 0.5 to within 1e-3")
        assert share >= 0.90, name


@pytest.mark.parametrize("kind", ["temporal", "cross"])
def test_flat_weights_are_one_over_the_keys(kind):
    for case, exact, name in _pairs(kind):
        c = case("flat")
        out, p, _ = exact(c)
        keys = p.shape[-1]
        assert torch.equal(p, torch.full_like(p, 1.0 / keys)), name
        if kind == "cross":                  # the output is the mean of v over the item's real keys
            v = (c.ehs.double() @ c.wv.double().t()).mean(1)                 # [item][inner]
            want = c.t.double() + (v @ c.wo.double().t()).repeat_interleave(c.rows, 0) + c.bo.double()
            assert (out - want).abs().max().item() < 1e-12, name


def test_builders_are_seeded_fp16_and_follow_their_recipes():
    for regime in ALL:
        a, b = R.temporal_case(regime, 320, 2, 4, 9), R.temporal_case.__wrapped__(regime, 320, 2, 4, 9)
        for k in ("t", "gamma", "beta", "wq", "wk", "wv", "wo", "bo"):
            x = getattr(a, k)
            assert torch.equal(x, getattr(b, k)) and torch.equal(x, R.h(x)) and torch.isfinite(x).all(), (regime, k)
        a, b = R.cross_case(regime, 2, 70, 17), R.cross_case.__wrapped__(regime, 2, 70, 17)
        for k in ("t", "gamma", "beta", "wq", "wk", "wv", "wo", "bo", "ehs"):
            x = getattr(a, k)
            assert torch.equal(x, getattr(b, k)) and torch.equal(x, R.h(x)) and torch.isfinite(x).all(), (regime, k)
    base, hot = R.temporal_case("ordinary", 320, 2, 4, 9), R.temporal_case("one_hot", 320, 2, 4, 9)
    assert torch.equal(hot.wq, base.wq * 32) and torch.equal(hot.wk, base.wk * 32) and torch.equal(hot.wv, base.wv)
    tie = R.temporal_case("two_way_tie", 320, 2, 4, 9).t.view(2, 4, 9, 320)
    assert torch.equal(tie[:, 2:], tie[:, :2]) and not torch.equal(tie[:, 0], tie[:, 1])
    ctie = R.cross_case("two_way_tie", 2, 70, 17).ehs
    assert torch.equal(ctie[:, 8:16], ctie[:, :8]) and bool((ctie[:, 16] == 0).all())
    out = R.temporal_case("outlier_rows", 320, 2, 4, 9).t
    big = out.abs() == 300.0
    assert bool((big.sum(1) == 4).all()) and abs(out[~big].mean().item() - 20.0) < 0.05 and bool((out[~big].abs() < 25).all())
    assert not R.temporal_case("flat", 512, 1, 2, 13).wq.any() and not R.cross_case("flat", 1, 200, 16).wq.any()


def test_padding_and_redraw_helpers():
    n_items, kv_len, inner = 2, 17, 320
    g = torch.Generator().manual_seed(3)
    k_rows, vt = torch.randn(n_items * R.PAD, inner, generator=g).half(), torch.randn(inner, n_items * R.PAD, generator=g).half()
    k2, v2 = R.fill_padding(k_rows, vt, n_items, kv_len, seed=1)
    kk, kk2 = k_rows.view(n_items, R.PAD, inner), k2.view(n_items, R.PAD, inner)
    vv, vv2 = vt.view(inner, n_items, R.PAD), v2.view(inner, n_items, R.PAD)
    assert torch.equal(kk2[:, :kv_len], kk[:, :kv_len]) and torch.equal(vv2[:, :, :kv_len], vv[:, :, :kv_len])
    for junk in (kk2[:, kv_len:], vv2[:, :, kv_len:]):
        assert bool(((junk.abs() >= 50) & (junk.abs() <= 100)).all()) and bool((junk > 0).any()) and bool((junk < 0).any())
    B, Fr, HW = 2, 4, 13
    keep = R.pixel_rows(B, Fr, HW, 0, (0, 5, 12))
    assert keep.tolist()[:4] == [0, 5, 12, 13] and len(keep) == 3 * Fr
    t = R.temporal_case("ordinary", 320, B, Fr, HW).t
    t2 = R.redraw_except(t, keep, seed=7)
    other = torch.ones(t.shape[0], dtype=torch.bool)
    other[keep] = False
    assert torch.equal(t2[keep], t[keep]) and bool((t2[other] != t[other]).any(1).all()) and torch.equal(t2, R.h(t2))
    assert t2[other].std().item() > 3.5
