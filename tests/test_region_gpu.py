"""-m gpu: the regional-prompt blend kernel and the UNet's `regions=` path (csrc/region.hip, vdx/unet3d.py).  Bit for bit:
`ops.region_blend` against the torch-CPU restatement of tests/region_ref.py (fp32 products and fp32 sums in ascending j, each a
correctly rounded operation, so equality is derived, not measured); all-zero masks against the plain forward, one all-255 region
against the plain forward with that text, hard masks against a forward assembled from plain sub-block calls and `torch.where`.
Within the tiny UNet's standing bound: the same text in every region against the plain forward, and three different texts
against the fp32 oracle with its `attn2` in the attention-couple form."""
import os
import sys

import numpy as np
import pytest
import torch

import region_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
T = 5


def _ops():
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    return ops, VdxError


def _same_bits(got, want, what):
    """Every fp16 bit equal (signed zeros too); NaNs in the same places (a NaN's payload is not part of the statement)."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype == torch.float16 and got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
    g, w = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {got.numel()} values differ"


# ---- region_blend ---------------------------------------------------------------------------------------------------------------
WINDOWS = {1: [(0, 1, 1, False), (3, 1, 1, False)], 3: [(1, 3, 1, False), (0, 3, 2, False), (T - 2, 3, 1, True), (T - 1, 3, 2, True)]}


def _table(S, n, seed):
    """fp32 (T, S, n): rows cycle through an exact one (1.0f on one text), a two-way and a three-way soft mix (zeros elsewhere) and
    a mix of all n; text n - 1 (n >= 3) has no weight anywhere on frame 0 and text 1 (n >= 2) none on the last frame."""
    g = np.random.default_rng(seed)
    tab = np.zeros((T, S, n), np.float32)
    for t in range(T):
        for p in range(S):
            kind = (t * S + p) % 4
            k = 1 if kind == 0 or n == 1 else min(n, {1: 2, 2: 3, 3: n}[kind])
            js = g.choice(n, size=k, replace=False)
            a = g.random(k) + 0.05
            tab[t, p, js] = (a / a.sum()).astype(np.float32) if k > 1 else 1.0
    if n == 1:
        tab[:, 1::2, 0] = g.random((T, len(range(1, S, 2)))).astype(np.float32) + 0.25     # one input, soft: fp16(w x)
    if n >= 3:
        tab[0, :, n - 1] = 0.0
    if n >= 2:
        tab[T - 1, :, 1] = 0.0
    return tab


def _inputs(n, M, C, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [(torch.randn(M, C, generator=g) * 2).half() for _ in range(n)]
    edge = torch.tensor([65504.0, -65504.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 6e-5, 0.0, 1.0], dtype=torch.float16)
    for j, x in enumerate(xs):
        k = min(edge.numel(), x.numel())
        x.view(-1)[:k] = edge.roll(j)[:k]
    return xs


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("C", [1, 4, 6, 8, 320])
def test_region_blend_is_the_restatement(gpu, C, n):
    """S in {1, 45, 144}, L in {1, 3}, every window of the list (d = 2, s > 0, a ring that wraps): the restatement's bits, `out`
    aliasing input 0, canaries behind `out`, the same bits from run to run and for the rows of one call or of two."""
    ops, _ = _ops()
    for S in (1, 45, 144):
        tab = _table(S, n, seed=S * 10 + n)
        tg = torch.from_numpy(tab).to(gpu)
        for L, windows in WINDOWS.items():
            M = L * S
            xs = _inputs(n, M, C, seed=C + S + L)
            xg = [x.to(gpu) for x in xs]
            for s, _, d, ring in windows:
                what = f"C={C} n={n} S={S} window {(s, L, d, ring)}"
                want = R.blend(xs, tab, s, L, d, ring)
                buf = torch.full((M * C + 64,), 7.0, dtype=torch.float16, device=gpu)      # canaries behind out
                out = buf[:M * C].view(M, C)
                assert ops.region_blend(xg, tg, s, L, d, ring, out=out) is out
                _same_bits(out, want, what)
                assert bool((buf[M * C:] == 7.0).all()), what + ": wrote behind out"
                _same_bits(ops.region_blend(xg, tg, s, L, d, ring), want, what + " again")
                alias = [xg[0].clone()] + xg[1:]
                assert ops.region_blend(alias, tg, s, L, d, ring, out=alias[0]) is alias[0]
                _same_bits(alias[0], want, what + " in place")
                if L == 3:                                          # frames 0..1 and frame 2 in two calls
                    tau2 = (s + 2 * d) % T if ring else s + 2 * d
                    a = ops.region_blend([x[:2 * S] for x in xg], tg, s, 2, d, ring)
                    b = ops.region_blend([x[2 * S:] for x in xg], tg, tau2, 1, 1, False)
                    _same_bits(torch.cat([a, b]), want, what + " in two calls")


def test_a_text_that_was_not_launched_is_skipped(gpu):
    """None for the inputs without weight on the window (the table's last text on frame 0, text 1 on the last frame)."""
    ops, _ = _ops()
    S, C, n = 45, 8, 4
    tab = _table(S, n, seed=9)
    tg = torch.from_numpy(tab).to(gpu)
    xs = _inputs(n, S, C, seed=2)
    for tau, absent in ((0, n - 1), (T - 1, 1)):
        assert not tab[tau, :, absent].any()
        some = [None if j == absent else x for j, x in enumerate(xs)]
        got = ops.region_blend([None if x is None else x.to(gpu) for x in some], tg, tau, 1)
        _same_bits(got, R.blend(some, tab, tau, 1), f"frame {tau}")
        _same_bits(got, R.blend(xs, tab, tau, 1), f"frame {tau}, against all inputs given")


@pytest.mark.parametrize("C", [320, 6], ids=["vector", "scalar"])
def test_a_nan_stays_where_its_weight_is(gpu, C):
    """A NaN-filled input with zero weight on the window's frame does not appear; a NaN in one row of a weighted input appears
    in that row's element only (and only if the row has weight for that input)."""
    ops, _ = _ops()
    S, n = 45, 3
    tab = _table(S, n, seed=4)
    tg = torch.from_numpy(tab).to(gpu)
    xs = _inputs(n, S, C, seed=8)
    poisoned = [x.clone() for x in xs]
    poisoned[n - 1][:] = NAN                                        # no weight on frame 0
    got = ops.region_blend([x.to(gpu) for x in poisoned], tg, 0, 1).cpu()
    assert bool(torch.isfinite(got.float()).all())
    _same_bits(got, R.blend(xs, tab, 0, 1), "zero-weight NaN")
    rows = [p for p in range(S) if tab[2, p, 1] != 0]               # frame 2: text 1 has weight on some rows, none on others
    assert rows and len(rows) < S
    planted = [x.clone() for x in xs]
    planted[1][:, C - 1] = NAN
    planted[1][:, 0] = float("inf")
    got = ops.region_blend([x.to(gpu) for x in planted], tg, 2, 1).cpu()
    _same_bits(got, R.blend(planted, tab, 2, 1), "planted")
    bad = ~torch.isfinite(got.float())
    for p in range(S):
        assert int(bad[p].sum()) == (2 if p in rows else 0), p
        assert p not in rows or (bool(bad[p, C - 1]) and bool(bad[p, 0]))


def test_region_blend_refuses_bad_arguments_before_a_launch(gpu):
    ops, VdxError = _ops()
    S, C, n = 4, 8, 2
    tg = torch.from_numpy(_table(S, n, seed=1)).to(gpu)
    xg = [x.to(gpu) for x in _inputs(n, 3 * S, C, seed=1)]
    for s, L, d, ring in ((0, 0, 1, False), (0, 3, 0, False), (-1, 3, 1, False), (T, 3, 1, False), (3, 3, 1, False), (1, 3, 2, False),
                          (T, 3, 1, True), (T - 1, 3, T, True)):
        with pytest.raises(VdxError):
            ops.region_blend(xg if L == 3 else [x[:max(L, 1) * S] for x in xg], tg, s, L, d, ring)
    with pytest.raises(VdxError):
        ops.region_blend(xg * 5, tg, 0, 3)                          # 10 inputs
    with pytest.raises(VdxError):
        ops.region_blend(xg + xg[:1], tg, 0, 3)                     # 3 inputs, a table of 2
    with pytest.raises(VdxError):
        ops.region_blend([None, None], tg, 0, 3)
    with pytest.raises(VdxError):
        ops.region_blend([xg[0], xg[1][:, :4]], tg, 0, 3)
    with pytest.raises(VdxError):
        ops.region_blend(xg, tg.double(), 0, 3)
    with pytest.raises(VdxError):
        ops.region_blend([xg[0], xg[1].view(-1)[4:4 + 2 * S * C].view(2 * S, C)], tg, 0, 2)    # 8-byte aligned at C = 8
    torch.cuda.synchronize()


# ---- the UNet --------------------------------------------------------------------------------------------------------------------
F_ = R.PARITY_F
MODELS = {"tiny": R.TINY, "level 0 at 320": dict(ch=(320, 128, 128, 128), cross=128, in_heads=8)}      # the second runs K5 and K8
LATENTS = [(16, 16), (5, 9)]
CLIP = 4                                                            # the clip of the UNet tests: windows of F_ = 3 frames of it


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


def _plan(masks, h, w, gpu, T_=CLIP):
    from vdx.region import region_plan
    return region_plan([(m, f"text {i}") for i, m in enumerate(masks)], T_, h, w, 4).to(gpu)


def _case(gpu, h, w, B=2, seed=11):
    ops, _ = _ops()
    g = torch.Generator().manual_seed(seed + h)
    lat = torch.randn(1, 4, F_, h, w, generator=g).half().to(gpu)
    text = torch.randn(2, 77, 128, generator=g).half().to(gpu)
    rtext = torch.randn(2, 77, 128, generator=g).half().to(gpu)
    x = ops.cfg_input(lat, None, 0.0) if B == 2 else lat
    return x, (text if B == 2 else text[1:].contiguous()), rtext


def _set(m, k5, prefix):
    m.fuse_cross_attn, m.share_cfg_prefix, m.text_cache_slots = k5, prefix, 1


BATCHES = [(True, 2), (False, 2), (False, 1)]                       # (shared prefix, batch)
BATCH_IDS = ["shared prefix", "no prefix", "batch 1"]


@pytest.mark.parametrize("prefix,B", BATCHES, ids=BATCH_IDS)
@pytest.mark.parametrize("name", list(MODELS))
def test_mask_identities(gpu, models, name, prefix, B):
    """All-zero masks: the plain forward, bit for bit (nothing beyond the base is launched).  One all-255 region: the plain forward
    with that region's text as the prompt, bit for bit (the base is not launched).  On 16x16 and the odd 5x9 grid."""
    m = models[name]
    _set(m, True, prefix)
    try:
        for h, w in LATENTS:
            x, text, rtext = _case(gpu, h, w, B)
            want = m(x, 501, encoder_hidden_states=text).sample
            assert m.last_forward_shared_prefix == (prefix and B == 2)
            zero = np.zeros((8 * h, 8 * w), np.uint8)
            got = m(x, 501, encoder_hidden_states=text, regions=(rtext, _plan([zero, zero], h, w, gpu), (1, F_, 1, False))).sample
            assert m.last_forward_shared_prefix == (prefix and B == 2)
            _same_bits(got, want, f"{h}x{w}: all-zero masks")
            full = np.full((CLIP, 8 * h, 8 * w), 255, np.uint8)
            swapped = torch.cat([text[:B - 1], rtext[:1]]).contiguous()
            want1 = m(x, 501, encoder_hidden_states=swapped).sample
            assert not torch.equal(want1, want)
            got1 = m(x, 501, encoder_hidden_states=text, regions=(rtext[:1].contiguous(), _plan([full], h, w, gpu), (0, F_, 1, False))).sample
            _same_bits(got1, want1, f"{h}x{w}: one all-255 region")
            _same_bits(m(x, 501, encoder_hidden_states=text).sample, want, "the plain forward after a regional one")
    finally:
        _set(m, True, True)


def _soft_masks(h, w):
    """Two soft-edged masks in pixels: a static ramp over the left half and a per-frame ramp from the top that grows with the
    frames; they overlap, and the base keeps the bottom right."""
    H, W = 8 * h, 8 * w
    x = np.arange(W, dtype=np.float64)[None, :].repeat(H, 0)
    y = np.arange(H, dtype=np.float64)[:, None].repeat(W, 1)
    m1 = np.round(255 * np.clip((W / 2 - x) / (W / 4), 0, 1)).astype(np.uint8)
    m2 = np.stack([np.round(255 * np.clip((H * (f + 1) / (CLIP + 1) - y) / (H / 4), 0, 1)).astype(np.uint8) for f in range(CLIP)])
    return m1, m2


@pytest.mark.parametrize("prefix,B", BATCHES, ids=BATCH_IDS)
@pytest.mark.parametrize("name", list(MODELS))
def test_the_same_text_in_every_region_is_the_plain_forward_to_fp16_rounding(gpu, models, name, prefix, B):
    """Base and two soft regions, all with the base's text: every sub-block result is the same, the weights sum to 1 within an
    fp32 ulp, so the blend differs from it by fp16 rounding only.  Bound: the 4e-3 of this UNet's forward."""
    m = models[name]
    _set(m, True, prefix)
    try:
        for h, w in LATENTS:
            x, text, _ = _case(gpu, h, w, B)
            want = m(x, 501, encoder_hidden_states=text).sample.float()
            same = text[B - 1:].expand(2, -1, -1).contiguous()
            got = m(x, 501, encoder_hidden_states=text, regions=(same, _plan(_soft_masks(h, w), h, w, gpu), (1, F_, 1, False))).sample.float()
            err = float((got - want).norm() / want.norm())
            print(f"{name} {h}x{w} B={B}: repeated text against the plain forward rel-L2 {err:.3e}")
            assert err <= R.PARITY_BOUND
    finally:
        _set(m, True, True)


def _hard_masks(h, w):
    """0 / 255 masks aligned to 64-pixel blocks (every cell of every level has one owner): region 1 the left 64-pixel column block
    on every frame, region 2 the bottom row block right of it from clip frame 2 on."""
    H, W = 8 * h, 8 * w
    m1 = np.zeros((H, W), np.uint8)
    m1[:, :64] = 255
    m2 = np.zeros((CLIP, H, W), np.uint8)
    m2[2:, H - 64:, 64:] = 255
    return m1, m2


@pytest.mark.parametrize("prefix,B", BATCHES, ids=BATCH_IDS)
@pytest.mark.parametrize("name", list(MODELS))
def test_hard_masks_are_a_select_of_plain_sub_blocks(gpu, models, name, prefix, B):
    """Hard masks on 64-pixel blocks, latent 16x16: the forward equals, bit for bit, the forward whose blend is replaced by
    `torch.where` over all R + 1 plain sub-block results with the owner map of the restated tables (tests/region_ref.py).  The
    window (1, 3, 1) holds clip frames where region 2 is absent (1) and present (2, 3)."""
    ops, _ = _ops()
    m = models[name]
    _set(m, True, prefix)
    h = w = 16
    x, text, rtext = _case(gpu, h, w, B)
    masks = _hard_masks(h, w)
    plan = _plan(masks, h, w, gpu)
    tabs = R.weights(masks, CLIP, h, w, 4)
    assert all(np.isin(t, (0.0, 1.0)).all() for t in tabs)
    window = (1, F_, 1, False)
    got = m(x, 501, encoder_hidden_states=text, regions=(rtext, plan, window)).sample
    blend, calls = ops.region_blend, []

    def select(subs, table, s, L, d=1, ring=False, out=None):
        tab = next(t for t in tabs if t.shape[1] == table.shape[1])
        owner = torch.from_numpy(np.concatenate([tab[tau].argmax(axis=1) for tau in R.window_frames(CLIP, s, L, d, ring)])).to(gpu)
        res = torch.zeros_like(out)
        for j, sub in enumerate(subs):
            if sub is not None:
                res = torch.where((owner == j)[:, None], sub, res)
            else:
                assert not bool((owner == j).any())
        calls.append(sum(sub is not None for sub in subs))
        out.copy_(res)
        return out

    try:
        ops.region_blend = select
        want = m(x, 501, encoder_hidden_states=text, regions=(rtext, plan, window)).sample
    finally:
        ops.region_blend = blend
        _set(m, True, True)
    assert len(calls) == 16 and set(calls) == {3}
    _same_bits(got, want, "hard masks")
    assert not torch.equal(got, m(x, 501, encoder_hidden_states=text).sample)


def test_a_region_without_weight_on_the_window_adds_no_launch(gpu, models):
    """Region 2 of the hard masks is zero on clip frames 0 and 1: on a window of those frames the forward launches what it
    launches with region 1 alone, at every level, and gives its bits; on a window that reaches frame 2 it launches more."""
    ops, _ = _ops()
    h = w = 16
    masks = _hard_masks(h, w)
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(1, 4, 2, h, w, generator=g).half().to(gpu)
    x = ops.cfg_input(lat, None, 0.0)
    _, text, rtext = _case(gpu, h, w)
    counted = ("cross_attn_block", "flash_attn", "region_blend")
    plain = {k: getattr(ops, k) for k in counted}
    for name, m in models.items():
        _set(m, True, True)
        n = dict.fromkeys(counted, 0)

        def counting(k):
            def call(*a, **kw):
                n[k] += 1
                return plain[k](*a, **kw)
            return call

        def run(regions):
            for k in counted:
                n[k] = 0
            m._text_ref = None
            out = m(x, 501, encoder_hidden_states=text, regions=regions).sample
            return out, dict(n)

        try:
            for k in counted:
                setattr(ops, k, counting(k))
            one, n_one = run((rtext[:1].contiguous(), _plan(masks[:1], h, w, gpu), (0, 2, 1, False)))
            two, n_two = run((rtext, _plan(masks, h, w, gpu), (0, 2, 1, False)))
            _, n_later = run((rtext, _plan(masks, h, w, gpu), (1, 2, 1, False)))
            _, n_off = run(None)
        finally:
            for k in counted:
                setattr(ops, k, plain[k])
            _set(m, True, True)
        print(f"{name}: launches plain {n_off}, one region {n_one}, two regions (one absent) {n_two}, both present {n_later}")
        assert n_two == n_one and n_one["region_blend"] == 16 and n_off["region_blend"] == 0
        assert sum(n_later.values()) == sum(n_one.values()) + 16          # one more sub-block per spatial transformer
        _same_bits(two, one, name)


def test_three_different_texts_lie_within_the_bound_of_the_attention_couple_oracle(gpu, models):
    """Base and two soft-edged regions (one per-frame), three different texts, against the fp32 oracle whose spatial `attn2` is
    wrapped in the attention-couple form (tests/region_ref.py).  The bound is the one the tiny UNet has against the oracle without
    regions (tests/test_unet_gpu.py: 4e-3).  That it shows anything: swapping the two regions' texts moves the oracle's own output by
    at least five times the bound (10.8x, CPU, recorded in profiles/region_parity.txt), so a forward that mixed up its regions
    could not pass."""
    ref, _ = R.parity_oracle()
    moved, want, tables, _ = R.parity_case(ref)
    print(f"oracle alone: swapping the regions' texts moves the output by rel-L2 {moved:.3e} = {moved / R.PARITY_BOUND:.1f} x the bound")
    assert moved >= 5 * R.PARITY_BOUND
    sample, text, rtext = R.parity_inputs()
    plan = _plan(R.parity_masks(), R.PARITY_H, R.PARITY_W, gpu, T_=R.PARITY_F)
    for lev, tab in enumerate(tables):
        assert np.abs(plan.tables[lev].cpu().numpy().astype(np.float64) - tab).max() <= 2.0 ** -23
    m = models["tiny"]
    for prefix in (True, False):
        _set(m, True, prefix)
        got = m(sample.to(gpu), R.PARITY_T, encoder_hidden_states=text.to(gpu), regions=(rtext.to(gpu), plan, (0, R.PARITY_F, 1, False))).sample
        err = float((got.float().cpu().double() - want.double()).norm() / want.double().norm())
        print(f"regional prompts against the attention-couple oracle (shared prefix {prefix}): rel-L2 {err:.3e} (bound {R.PARITY_BOUND:.0e})")
        assert err <= R.PARITY_BOUND
    _set(m, True, True)
    swapped = m(sample.to(gpu), R.PARITY_T, encoder_hidden_states=text.to(gpu), regions=(rtext.flip(0).contiguous().to(gpu), plan, (0, R.PARITY_F, 1, False))).sample
    assert float((swapped.float().cpu().double() - want.double()).norm() / want.double().norm()) > 5 * R.PARITY_BOUND
