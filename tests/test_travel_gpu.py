"""-m gpu: prompt travel's kernels and the UNet's per-frame text path (csrc/travel.hip, vdx/unet3d.py).  Bit for bit: `text_travel`
against the torch-CPU restatement of tests/travel_ref.py (two fp32 products and their fp32 sum, each a correctly rounded operation,
so equality is derived, not measured), the pack kernel against `packing.pack_k5_kv`, K5 and flash attention over six K/V items
against six calls over one, and a (B, F, N, D) text that repeats one text against the (B, N, D) forward.  Within the tiny UNet's
standing bound against the fp32 oracle: the forward with three different texts."""
import os
import sys

import pytest
import torch

import travel_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
T = 8
ROWS = 192                                                          # K5's row tile (csrc/rowtile_common.h)


def _ops():
    import vdx  # noqa: F401
    from vdx import ops, packing
    from vdx._lib import VdxError
    return ops, packing, VdxError


def _same_bits(got, want, what):
    """Every fp16 bit equal (signed zeros too); NaNs in the same places (a NaN's payload is not part of the statement)."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype == torch.float16 and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
    g, w = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {got.numel()} values differ"


# ---- text_travel --------------------------------------------------------------------------------------------------------------
FRAMES = {1: [0], 2: [0, 7], 3: [0, 3, 7], 4: [1, 3, 4, 6]}          # the keys' frames in a clip of T = 8, by n_keys
SHAPES = [(1, 77, 1024), (3, 77, 1024), (2, 5, 3), (4, 1, 8)]        # (n_keys, N, D): 16-byte lanes, and D = 3: one element per lane
WINDOWS = [(0, 1, 1, False), (2, 6, 1, False), (1, 4, 2, False), (T - 2, 5, 1, True)]


def _texts(n_keys, N, D, seed=3):
    g = torch.Generator().manual_seed(seed + n_keys * N + D)
    keys = torch.randn(n_keys, N, D, generator=g).half()
    uncond = torch.randn(N, D, generator=g).half()
    edge = torch.tensor([65504.0, -65504.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 6e-5, 0.0, 1.0], dtype=torch.float16)
    for k in range(n_keys):                                         # every key starts with the edge values, rotated: all pairs meet
        n = min(edge.numel(), N * D)
        keys[k].view(-1)[:n] = edge.roll(k)[:n]
    return keys, uncond


def _plan_on(gpu, n_keys, loop):
    lo, hi, w = R.plan(FRAMES[n_keys], T, loop)
    return (lo, hi, w), tuple(torch.from_numpy(a).to(gpu) for a in (lo, hi, w))


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_text_travel_is_the_restatement(gpu, shape):
    """Every window of the list, on the flat plan and (for the ring window) on the looping plan; a key frame has the key's bits,
    item 0 is `uncond` on every frame, and a second run has the first one's bits."""
    ops, _, _ = _ops()
    n_keys, N, D = shape
    keys, uncond = _texts(n_keys, N, D)
    kg, ug = keys.to(gpu), uncond.to(gpu)
    for s, L, d, ring in WINDOWS:
        (lo, hi, w), dev = _plan_on(gpu, n_keys, ring)
        got = ops.text_travel(kg, ug, *dev, s, L, d, ring)
        assert tuple(got.shape) == (2, L, N, D) and got.is_contiguous() and got.dtype == torch.float16
        _same_bits(got, R.text_travel(keys, uncond, lo, hi, w, s, L, d, ring), f"{shape} window {(s, L, d, ring)}")
        _same_bits(got[0], uncond.expand(L, N, D), "item 0")
        for f in range(L):
            t = (s + f * d) % T
            if t in FRAMES[n_keys]:
                _same_bits(got[1, f], keys[FRAMES[n_keys].index(t)], f"key frame {t}")
        assert torch.equal(got, ops.text_travel(kg, ug[None], *dev, s, L, d, ring))        # run to run; uncond as (1, N, D)
    if n_keys > 1:                                                  # the blend did blend: some frame lies strictly between two keys
        (lo, hi, w), dev = _plan_on(gpu, n_keys, False)
        mid = next(t for t in range(T) if w[t] != 0)
        got = ops.text_travel(kg, ug, *dev, mid, 1, 1)
        assert not torch.equal(got[1, 0].cpu(), keys[lo[mid]]) and not torch.equal(got[1, 0].cpu(), keys[hi[mid]])


@pytest.mark.parametrize("shape", [(3, 77, 1024), (2, 5, 3)], ids=["vector", "scalar"])
def test_a_nan_in_a_key_stays_in_the_frames_that_read_it(gpu, shape):
    ops, _, _ = _ops()
    n_keys, N, D = shape
    keys, uncond = _texts(n_keys, N, D)
    keys[1, N - 1, D - 1] = NAN
    keys[1, 0, 0] = float("inf")
    (lo, hi, w), dev = _plan_on(gpu, n_keys, False)
    got = ops.text_travel(keys.to(gpu), uncond.to(gpu), *dev, 0, T, 1).cpu()
    _same_bits(got, R.text_travel(keys, uncond, lo, hi, w, 0, T, 1), "planted")
    reads = [t for t in range(T) if (lo[t] == 1) or (hi[t] == 1 and w[t] != 0)]
    assert reads and len(reads) < T
    for t in range(T):
        bad = ~torch.isfinite(got[1, t].float())
        assert int(bad.sum()) == (2 if t in reads else 0), t
        assert not t in reads or (bool(bad[N - 1, D - 1]) and bool(bad[0, 0]))
    assert bool(torch.isfinite(got[0].float()).all())


def test_text_travel_refuses_bad_arguments_before_a_launch(gpu):
    ops, _, VdxError = _ops()
    keys, uncond = _texts(2, 5, 8)
    kg, ug = keys.to(gpu), uncond.to(gpu)
    _, (lo, hi, w) = _plan_on(gpu, 2, False)
    for s, L, d, ring in ((0, 0, 1, False), (0, 1, 0, False), (-1, 1, 1, False), (T, 1, 1, False), (3, 6, 1, False), (1, 5, 2, False),
                          (0, 2, 2 ** 30, False), (T, 1, 1, True), (T - 1, T + 2, 1, True)):
        with pytest.raises(VdxError):
            ops.text_travel(kg, ug, lo, hi, w, s, L, d, ring)
    with pytest.raises(VdxError, match="outside"):
        ops.text_travel(kg, ug, lo, hi + 1, w, 0, 1, 1)
    with pytest.raises(VdxError, match="outside"):
        ops.text_travel(kg, ug, lo - 1, hi, w, 0, 1, 1)
    with pytest.raises(VdxError):
        ops.text_travel(kg, ug, lo.long(), hi, w, 0, 1, 1)
    with pytest.raises(VdxError):
        ops.text_travel(kg, ug[:, :4], lo, hi, w, 0, 1, 1)
    with pytest.raises(VdxError):
        ops.text_travel(kg, ug, lo, hi, w[:4], 0, 1, 1)
    torch.cuda.synchronize()


# ---- the pack kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [1, 2, 6])
def test_pack_kv_is_pack_k5_kv(gpu, n_items):
    ops, packing, VdxError = _ops()
    inner, pad = 320, 128
    g = torch.Generator().manual_seed(n_items)
    k_rows = torch.randn(n_items * pad, inner, generator=g).half().to(gpu)
    vt = torch.randn(inner, n_items * pad, generator=g).half().to(gpu)
    want = packing.pack_k5_kv(k_rows, vt, n_items, pad)
    got = ops.cross_attn_block_pack_kv(k_rows, vt, n_items, pad)
    assert tuple(got.shape) == tuple(want.shape) == (n_items, 5, 3 * 4096)
    _same_bits(got, want, "contiguous")
    assert not bool(got[:, :, 10240:].any()) and torch.equal(got, ops.cross_attn_block_pack_kv(k_rows, vt, n_items, pad))
    out = torch.full_like(want, 7.0)                                # a given out is overwritten whole, its zeroed unit included
    assert ops.cross_attn_block_pack_kv(k_rows, vt, n_items, pad, out=out) is out and torch.equal(out, want)
    wide_k = torch.randn(n_items * pad + 3, inner + 64, generator=g).half().to(gpu)     # views: a column block, a column range
    wide_v = torch.randn(inner, (n_items + 1) * pad, generator=g).half().to(gpu)
    _same_bits(ops.cross_attn_block_pack_kv(wide_k[:, 64:], wide_v[:, pad:], n_items, pad),
               packing.pack_k5_kv(wide_k[:n_items * pad, 64:].contiguous(), wide_v[:, pad:].contiguous(), n_items, pad), "views")
    with pytest.raises(VdxError):
        ops.cross_attn_block_pack_kv(k_rows[:, :256], vt[:256], n_items, pad)           # inner 256: K5 does not take it
    with pytest.raises(VdxError):
        ops.cross_attn_block_pack_kv(k_rows, vt, n_items + 1, pad)                      # more items than rows
    with pytest.raises(VdxError):
        ops.cross_attn_block_pack_kv(k_rows, vt, n_items * 2, 64)                       # fewer than the blob's 80 key slots


# ---- the parent's kernels at the arguments per-frame text calls them with ----------------------------------------------------------
@pytest.mark.parametrize("rows", [40, ROWS + 8])
def test_k5_over_six_items_is_six_calls_over_one(gpu, rows):
    """Six different K/V items, `rows` rows each: a part tile at every item boundary."""
    ops, packing, _ = _ops()
    inner, pad, kv_len, n_items = 320, 128, 77, 6
    g = torch.Generator().manual_seed(rows)
    r = lambda *shape, k=1.0: (torch.randn(*shape, generator=g) * k).half().to(gpu)     # noqa: E731
    t = r(n_items * rows, inner, k=1.5)
    blob = packing.pack_k5(r(inner, inner, k=0.09), r(inner, inner, k=0.05), r(inner, k=0.2) + 1, r(inner, k=0.1), r(inner, k=0.1), 0.125)
    kvb = ops.cross_attn_block_pack_kv(r(n_items * pad, inner), r(inner, n_items * pad), n_items, pad)
    whole = ops.cross_attn_block(t, blob, kvb, kv_len=kv_len, n_items=n_items, rows_per_item=rows)
    for i in range(n_items):
        one = ops.cross_attn_block(t[i * rows:(i + 1) * rows], blob, kvb[i:i + 1], kv_len=kv_len, n_items=1, rows_per_item=rows)
        _same_bits(whole[i * rows:(i + 1) * rows], one, f"item {i}")
    assert not torch.equal(whole[:rows], ops.cross_attn_block(t[:rows], blob, kvb[1:2], kv_len=kv_len, n_items=1, rows_per_item=rows))


@pytest.mark.parametrize("sq", [40, ROWS + 8])
def test_flash_attention_with_one_sequence_per_kv_is_per_sequence_calls(gpu, sq):
    ops, _, _ = _ops()
    heads, pad, skv, n = 2, 128, 77, 6
    inner = heads * 64
    g = torch.Generator().manual_seed(sq)
    r = lambda *shape: torch.randn(*shape, generator=g).half().to(gpu)                  # noqa: E731
    q, k, vt = r(n * sq, inner), r(n * pad, inner), r(inner, n * pad)
    whole = ops.flash_attn(q, k, vt, n_seq=n, sq=sq, skv=skv, skv_pad=pad, heads=heads, seq_per_kv=1, scale=0.125)
    for i in range(n):
        one = ops.flash_attn(q[i * sq:(i + 1) * sq], k[i * pad:(i + 1) * pad], vt[:, i * pad:(i + 1) * pad], n_seq=1, sq=sq, skv=skv,
                             skv_pad=pad, heads=heads, seq_per_kv=1, scale=0.125)
        _same_bits(whole[i * sq:(i + 1) * sq], one, f"sequence {i}")


# ---- the UNet ------------------------------------------------------------------------------------------------------------------
F_, H_, W_ = R.PARITY_F, R.PARITY_H, R.PARITY_W
MODELS = {"tiny": R.TINY, "level 0 at 320": dict(ch=(320, 128, 128, 128), cross=128, in_heads=8)}      # the second runs K5 and K8
# The latent of the rank-3 comparison.  K5 walks the heads of its output projection in an order rotated by the tile's index inside
# its K/V item (csrc/xattn.hip `set_tile`: a row's sum order is a function of (row in item // 192) % 5).  One text per sample makes
# an item of F h w rows, a text per frame items of h w rows, so a frame's rows keep their tile index, and with it their bits, only
# while F h w <= 192: 3 x 8 x 8 for the model that runs K5.  Beyond one tile the two forms agree to fp16 rounding, not bit for bit:
# the parent's kernel, which this test file does not change.  Without K5 (the tiny UNet, and `fuse_cross_attn = False`) any size.
LATENT = {"tiny": (H_, W_), "level 0 at 320": (8, 8)}


@pytest.fixture(scope="module")
def models(gpu):
    import vdx  # noqa: F401
    from oracle.unet3d_ref import UNet3DConfig as RefCfg, synthetic_state_dict
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    out = {}
    for name, kw in MODELS.items():
        sd = synthetic_state_dict(RefCfg.tiny(**kw), seed=1234)
        cfg = UNet3DConfig(block_out_channels=kw["ch"], cross_attention_dim=kw["cross"], transformer_in_heads=kw["in_heads"])
        out[name] = UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)
    assert any(k.endswith(".attn2.k5") for k in out["level 0 at 320"].W) and not any(k.endswith(".attn2.k5") for k in out["tiny"].W)
    return out


def _set(m, k5, prefix):
    m.fuse_cross_attn, m.share_cfg_prefix, m.text_cache_slots = k5, prefix, 1


@pytest.mark.parametrize("prefix", [True, False], ids=["shared prefix", "no prefix"])
@pytest.mark.parametrize("k5", [True, False], ids=["K5", "unfused"])
@pytest.mark.parametrize("name", list(MODELS))
def test_one_text_on_every_frame_is_the_rank_3_forward(gpu, models, name, k5, prefix):
    ops, _, VdxError = _ops()
    m = models[name]
    _set(m, k5, prefix)
    try:
        g = torch.Generator().manual_seed(11)
        lat = torch.randn(1, 4, F_, *LATENT[name], generator=g).half().to(gpu)
        assert name == "tiny" or F_ * LATENT[name][0] * LATENT[name][1] == ROWS
        text = torch.randn(2, 77, 128, generator=g).half().to(gpu)
        x = ops.cfg_input(lat, None, 0.0)
        want = m(x, 501, encoder_hidden_states=text).sample
        assert m.last_forward_shared_prefix == prefix
        per_frame = text[:, None].expand(2, F_, 77, 128).contiguous()
        got = m(x, 501, encoder_hidden_states=per_frame).sample
        assert m.last_forward_shared_prefix == prefix and m._text_per_frame
        _same_bits(got, want, "the same text on every frame")
        # three different texts: the shared prefix (one launch per item over its F K/V items) has the bits of the plain batch
        other = torch.randn(2, F_, 77, 128, generator=g).half().to(gpu)
        a = m(x, 501, encoder_hidden_states=other).sample
        assert not torch.equal(a, got)
        m.share_cfg_prefix = not prefix
        _same_bits(m(x, 501, encoder_hidden_states=other.clone()).sample, a, "shared prefix on against off")
        with pytest.raises(VdxError, match="frames"):
            m(x, 501, encoder_hidden_states=other[:, :2].contiguous())
    finally:
        _set(m, True, True)


def test_three_different_texts_lie_within_the_bound_of_the_per_frame_oracle(gpu, models):
    """The bound is the one the tiny UNet has against the oracle today (tests/test_unet_gpu.py: 4e-3).  That it shows anything:
    swapping the texts of frames 0 and 2 moves the oracle's own output by at least ten times the bound (19x, CPU, recorded in
    profiles/travel_parity.txt), so a forward that mixed up its frames' texts could not pass."""
    ref, _ = R.parity_oracle()
    moved, want = R.swap_sensitivity(ref)
    print(f"oracle alone: swapping two frames' texts moves the output by rel-L2 {moved:.3e} = {moved / R.PARITY_BOUND:.1f} x the bound")
    assert moved >= 10 * R.PARITY_BOUND
    sample, text = R.parity_inputs()
    m = models["tiny"]
    _set(m, True, True)
    got = m(sample.to(gpu), R.PARITY_T, encoder_hidden_states=text.to(gpu)).sample
    err = float((got.float().cpu().double() - want.double()).norm() / want.double().norm())
    print(f"per-frame text against the per-frame oracle: rel-L2 {err:.3e} (bound {R.PARITY_BOUND:.0e})")
    assert err <= R.PARITY_BOUND
    swapped = m(sample.to(gpu), R.PARITY_T, encoder_hidden_states=text[:, [2, 1, 0]].contiguous().to(gpu)).sample
    assert float((swapped.float().cpu().double() - want.double()).norm() / want.double().norm()) > 5 * R.PARITY_BOUND


@pytest.mark.parametrize("name", list(MODELS))
def test_the_text_cache_keeps_as_many_texts_as_it_has_slots(gpu, models, name):
    """Two alternating text tensors: with two slots each misses once and then hits; with the default one slot every call is a
    miss, as always.  The outputs are the same either way."""
    m = models[name]
    _set(m, True, True)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, F_, H_, W_, generator=g).half().to(gpu)
    a, b = (torch.randn(2, F_, 77, 128, generator=g).half().to(gpu) for _ in range(2))
    c = torch.randn(2, 77, 128, generator=g).half().to(gpu)          # a rank-3 text shares the store
    try:
        assert m.text_cache_slots == 1
        n0 = m.text_cache_misses
        one = [m(x, 501, encoder_hidden_states=e).sample for e in (a, b, a, b)]
        assert m.text_cache_misses - n0 == 4 and m._text_store == []
        m.text_cache_slots = 2
        n0 = m.text_cache_misses
        two = [m(x, 501, encoder_hidden_states=e).sample for e in (a, b, a, b, a)]
        assert m.text_cache_misses - n0 == 1 and len(m._text_store) == 1      # `b` was the text in use: only `a` had to come back
        for got, want in zip(two, one + one[:1]):
            _same_bits(got, want, "two slots against one")
        n0 = m.text_cache_misses
        m(x, 501, encoder_hidden_states=c)                           # a third text drops the least recently used: b
        m(x, 501, encoder_hidden_states=a)
        assert m.text_cache_misses - n0 == 1
        _same_bits(m(x, 501, encoder_hidden_states=b).sample, one[1], "after the drop")
        assert m.text_cache_misses - n0 == 2
        a.mul_(0.5)                                                  # written in place: its entry no longer stands for it
        n0 = m.text_cache_misses
        m(x, 501, encoder_hidden_states=a)
        assert m.text_cache_misses - n0 == 1
    finally:
        m.text_cache_slots = 1
        m._text_store.clear()
