"""-m gpu: token merging (csrc/tome.hip) against the restatement of tests/tome_ref.py: the match within the stated fp32 bound of
the float64 scores, select / merge / unmerge bit for bit, the self-attention stage against the same stage composed from the
existing ops around the reference merge, and the UNet, the sharded and shared-prefix forwards and the job with the switch.

Measured on an MI355X: profiles/tome_parity.txt."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tome_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
SHAPES = [(1, 2, 2, 64), (3, 5, 7, 64), (2, 8, 16, 320), (2, 9, 9, 128), (4, 18, 32, 320), (1, 24, 40, 1280)]
_CACHE = {}


def tol(C):
    """fp16 products are exact in fp32; C accumulations and two inverse norms each carry relative error of order C 2^-24 on terms
    whose normalised magnitudes sum to at most 1; the factor 4 is head-room."""
    return 4 * (C + 8) * 2.0 ** -24


def case(shape, ratio=0.5):
    """(t fp16 rows on the host, partition, float64 reference match), built once per shape and shared."""
    from vdx.tome import partition
    key = (shape, ratio)
    if key not in _CACHE:
        n_img, hh, ww, C = shape
        g = torch.Generator().manual_seed(hh * 1000 + ww * 10 + C)
        t = torch.randn(n_img * hh * ww, C, generator=g).half()
        part = partition(hh, ww, ratio)
        _CACHE[key] = (t, part, R.match(t, part.src_idx, part.dst_idx, n_img, hh * ww))
    return _CACHE[key]


def gpu_match(gpu, t, part, n_img, S):
    from vdx import ops
    return ops.tome_match(t.to(gpu), part.src_idx.to(gpu), part.dst_idx.to(gpu), n_img=n_img, S=S)


def check_match(sc, ref_max, node_max, node_idx, C, label=""):
    n_dst = sc.shape[-1]
    got_max, got_idx = node_max.cpu().double(), node_idx.cpu().long()
    assert int(got_idx.min()) >= 0 and int(got_idx.max()) < n_dst
    err = float((got_max - ref_max).abs().max())
    print(f"tome_match {label}: max |node_max - float64| = {err:.3e} (bound {tol(C):.3e})")
    assert err <= tol(C)
    picked = sc.gather(-1, got_idx[..., None])[..., 0]
    assert bool((picked >= ref_max - 2 * tol(C)).all())
    return err


# ---- match --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_match_within_the_fp32_bound(gpu, shape):
    n_img, hh, ww, C = shape
    t, part, (sc, ref_max, _) = case(shape)
    node_max, node_idx = gpu_match(gpu, t, part, n_img, hh * ww)
    check_match(sc, ref_max, node_max, node_idx, C, str(shape))
    again = gpu_match(gpu, t, part, n_img, hh * ww)
    assert torch.equal(again[0], node_max) and torch.equal(again[1], node_idx)          # run to run
    one = gpu_match(gpu, t[-hh * ww:], part, 1, hh * ww)                                  # any n_img
    assert torch.equal(one[0][0], node_max[-1]) and torch.equal(one[1][0], node_idx[-1])


def test_match_rows_with_a_stride(gpu):
    from vdx import ops
    n_img, hh, ww, C = 2, 8, 16, 320
    t, part, (sc, ref_max, _) = case((n_img, hh, ww, C))
    wide = torch.full((t.shape[0], C + 64), float("nan"), dtype=torch.float16)
    wide[:, :C] = t
    got = ops.tome_match(wide.to(gpu)[:, :C], part.src_idx.to(gpu), part.dst_idx.to(gpu), n_img=n_img, S=hh * ww)
    want = gpu_match(gpu, t, part, n_img, hh * ww)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("shape", [(2, 9, 9, 128), (2, 18, 32, 320)], ids=lambda s: "x".join(map(str, s)))
def test_match_planted_destinations_exact(gpu, shape):
    """Each source is a copy of a known destination plus noise; the margin to the runner-up is asserted on the reference first."""
    from vdx.tome import partition
    n_img, hh, ww, C = shape
    S = hh * ww
    part = partition(hh, ww, 0.5)
    g = torch.Generator().manual_seed(7)
    t = torch.randn(n_img, S, C, generator=g)
    planted = torch.randint(part.n_dst, (n_img, part.n_src), generator=g)
    for n in range(n_img):
        t[n, part.src_idx.long()] = t[n, part.dst_idx.long()][planted[n]] + 0.3 * torch.randn(part.n_src, C, generator=g)
    t = t.half().view(n_img * S, C)
    sc, ref_max, ref_idx = R.match(t, part.src_idx, part.dst_idx, n_img, S)
    top2 = sc.topk(2, dim=-1).values
    assert bool((top2[..., 0] - top2[..., 1] >= 0.1).all()) and torch.equal(ref_idx, planted)
    node_max, node_idx = gpu_match(gpu, t, part, n_img, S)
    assert torch.equal(node_idx.cpu().long(), planted)
    check_match(sc, ref_max, node_max, node_idx, C, f"planted {shape}")


def test_match_duplicate_destinations_take_the_lowest(gpu):
    from vdx.tome import partition
    n_img, hh, ww, C = 2, 18, 32, 320
    S = hh * ww
    part = partition(hh, ww, 0.5)
    g = torch.Generator().manual_seed(11)
    t = torch.randn(n_img, S, C, generator=g).half()
    d = part.dst_idx.long()
    t[:, d] = t[:, d[:5]].repeat(1, (part.n_dst + 4) // 5, 1)[:, :part.n_dst]            # every destination is one of five rows
    t = t.view(n_img * S, C)
    _, node_idx = gpu_match(gpu, t, part, n_img, S)
    assert int(node_idx.max()) < 5                                                       # the first copy, never a later tile's
    _, _, ref_idx = R.match(t, part.src_idx, part.dst_idx, n_img, S)
    sc = R.scores(t, part.src_idx, part.dst_idx, n_img, S)[..., :5]
    margin = sc.topk(2, dim=-1).values
    clear = (margin[..., 0] - margin[..., 1]) > 2 * tol(C)
    assert bool((node_idx.cpu().long() == ref_idx)[clear].all())


def test_match_non_finite_rows_stay_in_their_image(gpu):
    n_img, hh, ww, C = 3, 8, 16, 320
    S = hh * ww
    t, part, _ = case((2, 8, 16, 320))
    t = torch.cat([t, t[:S]]).clone()
    clean = gpu_match(gpu, t, part, n_img, S)
    bad = t.clone().view(n_img, S, C)
    bad[1, int(part.src_idx[3])] = 0                   # a zero source
    bad[1, int(part.dst_idx[2])] = 0                   # a zero destination
    bad[1, int(part.src_idx[9])] = float("nan")
    bad[1, int(part.dst_idx[7])] = float("nan")
    bad[1, int(part.src_idx[20]), 5] = float("inf")
    bad[1, int(part.dst_idx[11]), 0] = float("-inf")
    node_max, node_idx = gpu_match(gpu, bad.view(-1, C), part, n_img, S)
    assert int(node_idx.min()) >= 0 and int(node_idx.max()) < part.n_dst
    for n in (0, 2):
        assert torch.equal(node_max[n], clean[0][n]) and torch.equal(node_idx[n], clean[1][n])
    assert not bool(torch.isnan(node_max).any())        # a NaN score never wins: (-inf, 0) where nothing does
    assert float(node_max[1, 3]) == float("-inf") and int(node_idx[1, 3]) == 0
    assert float(node_max[1, 9]) == float("-inf") and int(node_idx[1, 9]) == 0


# ---- select, merge, unmerge ---------------------------------------------------------------------------------------------------
def run_select_merge(gpu, node_max, node_idx, y, t, part, n_img, S, r):
    """The three kernels on given (node_max, node_idx), checked bit for bit against the restatement."""
    from vdx import ops
    src, dst = part.src_idx.to(gpu), part.dst_idx.to(gpu)
    slot, off, items = ops.tome_select(node_max.to(gpu), node_idx.to(gpu), src, dst, S=S, r=r)
    rows = ops.tome_merge(y.to(gpu), src, dst, slot, off, items, n_img=n_img, S=S, r=r)
    w_slot, w_off, w_items, w_rows = R.select_merge_all(node_max, node_idx, y, part.src_idx, part.dst_idx, n_img, S, r)
    assert torch.equal(slot.cpu(), w_slot) and torch.equal(off.cpu(), w_off) and torch.equal(items.cpu(), w_items)
    assert torch.equal(rows.cpu().view(torch.int16), w_rows.view(torch.int16))
    a = torch.randn(rows.shape, generator=torch.Generator().manual_seed(5)).half()
    out = ops.tome_unmerge_add(a.to(gpu), slot, t.to(gpu), src, dst, n_img=n_img, S=S, r=r)
    Sm = S - r
    want = torch.cat([R.unmerge_add(a[n * Sm:(n + 1) * Sm], w_slot[n], t[n * S:(n + 1) * S]) for n in range(n_img)])
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    return slot, off, items


@pytest.mark.parametrize("ratio", [0.25, 0.5, 0.75])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_select_merge_unmerge_on_the_kernels_matching(gpu, shape, ratio):
    """ratio 0.75 merges every source (r = n_src) where the grid has no leftover rows or columns."""
    from vdx.tome import partition
    n_img, hh, ww, C = shape
    S = hh * ww
    t, part, _ = case(shape)
    part = partition(hh, ww, ratio)
    node_max, node_idx = gpu_match(gpu, t, part, n_img, S)
    y = torch.randn(t.shape, generator=torch.Generator().manual_seed(3)).half()
    run_select_merge(gpu, node_max.cpu(), node_idx.cpu(), y, t, part, n_img, S, part.r)


@pytest.mark.parametrize("craft", ["equal maxima", "nan entries", "one destination", "r = 1", "r = n_src", "index out of range"])
def test_select_merge_unmerge_on_crafted_matchings(gpu, craft):
    from vdx.tome import partition
    n_img, hh, ww, C = 2, 9, 9, 128
    S = hh * ww
    part = partition(hh, ww, 0.5)
    g = torch.Generator().manual_seed(13)
    t = torch.randn(n_img * S, C, generator=g).half()
    y = torch.randn(n_img * S, C, generator=g).half()
    node_max = torch.rand(n_img, part.n_src, generator=g)
    node_idx = torch.randint(part.n_dst, (n_img, part.n_src), generator=g).int()
    r = part.r
    if craft == "equal maxima":
        node_max = (node_max * 3).floor() / 4                         # three values, -0 among them: the index decides
        node_max[0, ::7] = -0.0
        node_max[0, 1::7] = 0.0
    elif craft == "nan entries":
        node_max[:, ::3] = float("nan")
        node_max[1, 1::3] = float("-inf")
        node_max[1, 2] = float("inf")
    elif craft == "one destination":
        node_idx[:] = 3
        r = part.n_src
    elif craft == "r = 1":
        r = 1
    elif craft == "r = n_src":
        r = part.n_src
    else:
        node_idx[0, ::2] = 2 ** 31 - 1
        node_idx[0, 1::4] = -5
        node_idx[1, :] = part.n_dst
    slot, off, items = run_select_merge(gpu, node_max, node_idx, y, t, part, n_img, S, r)
    assert int(slot.min()) >= 0 and int(slot.max()) < S - r and int(items.min()) >= 0 and int(items.max()) < part.n_src


def test_crafted_tables_and_lists_run_clean(gpu):
    """Caller-made buffers with entries outside every range: clamped, nothing faults, every output row is finite."""
    from vdx import ops
    from vdx.tome import partition
    n_img, hh, ww, C = 2, 8, 16, 64
    S = hh * ww
    part = partition(hh, ww, 0.5)
    g = torch.Generator().manual_seed(17)
    t = torch.randn(n_img * S, C, generator=g).half().to(gpu)
    wild = lambda n: torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).int().to(gpu)  # noqa: E731
    src, dst = wild(part.n_src), wild(part.n_dst)
    node_max, node_idx = ops.tome_match(t, src, dst, n_img=n_img, S=S)
    assert int(node_idx.min()) >= 0 and int(node_idx.max()) < part.n_dst
    slot, off, items = ops.tome_select(node_max, wild(n_img * part.n_src).view(n_img, -1), src, dst, S=S, r=part.r)
    rows = ops.tome_merge(t, src, dst, wild(n_img * S).view(n_img, S), wild(n_img * (part.n_dst + 1)).view(n_img, -1),
                          wild(n_img * part.r).view(n_img, -1), n_img=n_img, S=S, r=part.r,
                          out=torch.zeros((n_img * (S - part.r), C), dtype=torch.float16, device=gpu))
    out = ops.tome_unmerge_add(rows, wild(n_img * S).view(n_img, S), t, src, dst, n_img=n_img, S=S, r=part.r)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rows.float()).all()) and bool(torch.isfinite(out.float()).all())


def test_wrappers_refuse_what_they_cannot_take(gpu):
    from vdx import ops
    from vdx.ops import VdxError
    from vdx.tome import partition
    part = partition(8, 16, 0.5)
    S, src, dst = 128, part.src_idx.to(gpu), part.dst_idx.to(gpu)
    t = torch.zeros((2 * S, 64), dtype=torch.float16, device=gpu)
    with pytest.raises(VdxError):
        ops.tome_match(t[:, :32], src, dst, n_img=2, S=S)                       # C % 64
    with pytest.raises(VdxError):
        ops.tome_match(t, src, dst, n_img=3, S=S)                               # rows
    with pytest.raises(VdxError):
        ops.tome_match(t, src[:-1], dst, n_img=2, S=S)                          # tables do not add up to S
    with pytest.raises(VdxError):
        ops.tome_match(t, src.long(), dst, n_img=2, S=S)
    node_max, node_idx = ops.tome_match(t + 1, src, dst, n_img=2, S=S)
    for r in (0, part.n_src + 1):
        with pytest.raises(VdxError):
            ops.tome_select(node_max, node_idx, src, dst, S=S, r=r)
    slot, off, items = ops.tome_select(node_max, node_idx, src, dst, S=S, r=part.r)
    with pytest.raises(VdxError):
        ops.tome_merge(t, src, dst, slot, off, items[:, :-1], n_img=2, S=S, r=part.r)
    with pytest.raises(VdxError):
        ops.tome_unmerge_add(t[:2 * (S - part.r)], slot[:1], t, src, dst, n_img=2, S=S, r=part.r)


# ---- the stage ----------------------------------------------------------------------------------------------------------------
def tiny_model(gpu):
    import vdx  # noqa: F401
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from oracle.unet3d_ref import UNet3DConfig as RefCfg, synthetic_state_dict
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    cfg = UNet3DConfig(block_out_channels=TINY["ch"], cross_attention_dim=TINY["cross"], transformer_in_heads=TINY["in_heads"])
    return UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)


def test_self_attention_stage_bit_for_bit(gpu):
    """`_self_attention` with token merging (the stage `_spatial_transformer` runs, LayerNorm through residual) equals the stage
    composed here from ops.layernorm / ops.gemm / ops.flash_attn around the REFERENCE select, merge and unmerge on the kernel's
    own matching; above `max_downsample` it is the unmerged stage."""
    from vdx import ops
    from vdx.tome import partition
    m = tiny_model(gpu).enable_tome(0.5)
    p, b = "down_blocks.0.attentions.0", "down_blocks.0.attentions.0.transformer_blocks.0"
    n_img, hh, ww, C = 3, 9, 14, 64
    S = hh * ww
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n_img * S, C, generator=g).half().to(gpu)
    t = m._norm_proj_in(p, x, n_img, S, n_img * S)
    got = m._self_attention(b, t, n_img, hh, ww, m._level_down_of(p))
    assert [m._level_down_of(q) for q in ("down_blocks.0.attentions.1", "down_blocks.2.attentions.0", "mid_block.attentions.0",
                                          "up_blocks.1.attentions.2", "up_blocks.3.attentions.0")] == [1, 4, 8, 4, 1]
    plain = m._self_attention(b, t, n_img, hh, ww, 2)
    assert torch.equal(plain, tiny_model(gpu)._self_attention(b, t, n_img, hh, ww, 1)) and not torch.equal(plain, got)
    W = m.W
    part = partition(hh, ww, 0.5)
    ln = ops.layernorm(t, W[b + ".norm1.weight"], W[b + ".norm1.bias"], M=n_img * S)
    node_max, node_idx = ops.tome_match(t, part.src_idx.to(gpu), part.dst_idx.to(gpu), n_img=n_img, S=S)
    slot, _, _, rows = R.select_merge_all(node_max.cpu(), node_idx.cpu(), ln.cpu(), part.src_idx, part.dst_idx, n_img, S, part.r)
    Sm = S - part.r
    qkv = ops.gemm(rows.to(gpu), W[b + ".attn1.to_qkv.weight"], M=n_img * Sm)
    o = ops.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_seq=n_img, sq=Sm, skv=Sm, skv_pad=Sm, heads=C // 64, seq_per_kv=1,
                       scale=64 ** -0.5, v_rows=True)
    a = ops.gemm(o, W[b + ".attn1.to_out.0.weight"], M=n_img * Sm, bias=W[b + ".attn1.to_out.0.bias"]).cpu()
    want = torch.cat([R.unmerge_add(a[n * Sm:(n + 1) * Sm], slot[n], t.cpu()[n * S:(n + 1) * S]) for n in range(n_img)])
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


# ---- the UNet -----------------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_unet_with_tome(gpu):
    from vdx import ops
    m, never = tiny_model(gpu), tiny_model(gpu)
    g = torch.Generator().manual_seed(21)
    lat = torch.randn(1, 4, 4, 16, 32, generator=g).half().to(gpu)
    e = torch.randn(2, 77, TINY["cross"], generator=g).half().to(gpu)
    x = ops.cfg_input(lat, None, 0.0)
    off = never(x, 7, encoder_hidden_states=e).sample
    outs = {}
    for ratio in (0.25, 0.5):
        m.enable_tome(ratio)
        assert m.tome == {"ratio": ratio, "sx": 2, "sy": 2, "seed": None, "max_downsample": 1}
        on = m(x, 7, encoder_hidden_states=e).sample
        assert m.last_forward_shared_prefix
        assert bool(torch.isfinite(on.float()).all()) and not torch.equal(on, off)
        assert torch.equal(m(x, 7, encoder_hidden_states=e).sample, on)                    # run to run
        dup = m(x.clone(), 7, encoder_hidden_states=e).sample                              # the shared prefix off
        assert not m.last_forward_shared_prefix and torch.equal(dup, on)
        print(f"tome ratio {ratio}: rel-L2 {rel_l2(on.float().cpu(), off.float().cpu()):.3e} from the forward without (synthetic weights)")
        outs[ratio] = on
    # one image alone is that image inside a batch: a one-frame clip against the same frame as item 0 of a batch of two
    one = torch.randn(1, 4, 1, 16, 32, generator=g).half().to(gpu)
    two = torch.cat([one, torch.randn(1, 4, 1, 16, 32, generator=g).half().to(gpu)])
    alone = m(one, 7, encoder_hidden_states=e[:1]).sample
    both = m(two, 7, encoder_hidden_states=torch.cat([e[:1], e[:1]])).sample
    assert torch.equal(both[:1], alone)
    m.enable_tome(0.5, seed=4)
    seeded = m(x, 7, encoder_hidden_states=e).sample
    assert not torch.equal(seeded, outs[0.5]) and torch.equal(m(x, 7, encoder_hidden_states=e).sample, seeded)
    m.enable_tome(0.5, max_downsample=8)                                                  # every level that has cells
    deep = m(x, 7, encoder_hidden_states=e).sample
    assert bool(torch.isfinite(deep.float()).all()) and not torch.equal(deep, outs[0.5])
    assert {k[:2] for k in m._tome_tables} == {(16, 32), (8, 16), (4, 8), (2, 4)}
    with pytest.raises(ValueError):
        m.enable_tome(0.9)
    assert m.tome["max_downsample"] == 8                                                  # a refusal leaves the state
    m.disable_tome()
    assert m.tome is None and torch.equal(m(x, 7, encoder_hidden_states=e).sample, off)


def test_sharded_forward_has_the_resident_bits_with_tome(gpu):
    import vdx  # noqa: F401
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from vdx.weights import synthetic_state_dict
    cfg = UNet3DConfig(block_out_channels=(64, 128, 128, 128), cross_attention_dim=128, transformer_in_heads=2)
    sd = synthetic_state_dict(cfg, seed=9, device=gpu)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 4, 16, 32, generator=g).half().to(gpu)
    e = torch.randn(2, 77, 128, generator=g).half().to(gpu)
    a = UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)
    plain = a(x, 501, encoder_hidden_states=e).sample
    want = a.enable_tome(0.5)(x, 501, encoder_hidden_states=e).sample
    assert not torch.equal(want, plain)
    b = UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu).shard_(0, 1).enable_tome(0.5)
    assert torch.equal(b(x, 501, encoder_hidden_states=e).sample, want)
    assert torch.equal(b.disable_tome()(x, 501, encoder_hidden_states=e).sample, plain)


# ---- the job ------------------------------------------------------------------------------------------------------------------
def test_run_job_with_tome(gpu):
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import DiffuserConfig, run_job
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)

    def job(**kw):
        got = {}
        cfg = DiffuserConfig(**{**dict(model_id="synthetic:tiny", num_frames=8, steps=2, height=128, width=256, chunk_size=6, overlap=2,
                                       mode="chunk", noise_device="cpu"), **kw})
        res = run_job(cfg, out_video=None, pipe=pipe, clip_inputs=got)
        assert pipe.unet.tome is None
        return res, np.stack(got["frames"])
    res0, frames0 = job()
    assert "tome" not in res0
    res1, frames1 = job(tome=0.5)
    assert res1["tome"] == {"ratio": 0.5, "sx": 2, "sy": 2, "seed": None, "max_downsample": 1}
    assert set(res1) == set(res0) | {"tome"}
    assert frames1.shape == frames0.shape and not np.array_equal(frames1, frames0)
    res2, frames2 = job(tome=0.5, tome_seed=3, co_denoise=True, chunk_size=8, overlap=0)      # one window, co-denoised
    assert res2["tome"]["seed"] == 3 and "co_denoise" in res2 and frames2.std() > 0
    res3, frames3 = job()                                                                     # the default job is still the default job
    assert "tome" not in res3 and np.array_equal(frames3, frames0)
    pipe.enable_tome(0.25)
    assert pipe.unet.tome["ratio"] == 0.25
    pipe.disable_tome()
    assert pipe.unet.tome is None
