"""-m gpu: text of more than 128 rows through the UNet (vdx/unet3d.py `text_pad_of`), on the tiny UNet of tests/ckpt_dir.py at 2 frames
and a 16x16 latent, t = 501.  Text of 154, 231 and 308 rows lies within the forward's bound of the fp32 oracle on the same text
(rel-L2 <= 4e-3), and truncating that text to 77 rows moves the oracle itself by at least five times the bound (checked on the CPU
when the seed was chosen: 0.0557, 0.0620, 0.0653 = 13.9, 15.5, 16.3 x the bound), so a forward that dropped the rows past 77 or 128
could not pass.  Bit for bit: 77 and 128 rows with the padding forced to the old constant against the padding the call works out;
per-frame text with one text on every frame against the rank-3 forward; a region at 154 rows against the forward whose blend is
replaced by a select over plain sub-block results, and an all-255 region against the forward with that region's text as the prompt;
the CFG-shared prefix on against off; the sharded store against the resident weights."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ckpt_dir  # noqa: E402
import region_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = 4e-3                                                        # test_unet_tiny_live_oracle_other_shape's
F_, H, W, T = 2, 16, 16, 501
LONG = (154, 231, 308)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def world(gpu):
    import vdx  # noqa: F401
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg
    from vdx import ops
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    sd = ckpt_dir.unet_state_dict()
    cfg = UNet3DConfig(block_out_channels=ckpt_dir.UNET_CH, cross_attention_dim=ckpt_dir.CROSS, transformer_in_heads=8)
    m = UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)
    ref = UNet3DConditionModelRef(RefCfg.tiny(ch=ckpt_dir.UNET_CH, cross=ckpt_dir.CROSS, in_heads=8)).eval()
    ref.load_state_dict({k: v.half().float() for k, v in sd.items()})
    g = torch.Generator().manual_seed(77)
    sample = torch.randn(2, 4, F_, H, W, generator=g).half()
    text = torch.randn(2, 308, ckpt_dir.CROSS, generator=g).half()
    with torch.no_grad():                                           # computed once, shared, left unchanged
        oracle = {n: ref(sample.float(), torch.tensor(T), text[:, :n].float()).sample for n in (77,) + LONG}
    lat = torch.randn(1, 4, F_, H, W, generator=g).half().to(gpu)
    return dict(m=m, cfg=cfg, sd=sd, sample=sample, text=text, oracle=oracle, x=ops.cfg_input(lat, None, 0.0), gpu=gpu)


def run(world, text, m=None, x=None, **kw):
    m = m or world["m"]
    return m(world["x"] if x is None else x, T, encoder_hidden_states=text, **kw).sample.clone()


@pytest.mark.parametrize("n", LONG)
def test_long_text_lies_within_the_bound_of_the_oracle(world, n):
    gpu, text = world["gpu"], world["text"][:, :n].contiguous()
    moved = rel_l2(world["oracle"][77], world["oracle"][n])
    got = world["m"](world["sample"].to(gpu), T, encoder_hidden_states=text.to(gpu)).sample.float().cpu()
    err = rel_l2(got, world["oracle"][n])
    print(f"text of {n} rows: HIP vs oracle rel-L2 {err:.3e} (bound {BOUND:.0e}); truncating to 77 rows moves the oracle {moved:.3e} = {moved / BOUND:.1f} x")
    assert world["m"]._text_pad == {154: 192, 231: 256, 308: 320}[n] and world["m"]._text_len == n
    assert moved >= 5 * BOUND
    assert err <= BOUND
    assert rel_l2(got, world["oracle"][77]) > 5 * BOUND / 2         # and the HIP forward did see the rows past 77


def test_more_than_308_rows_is_refused(world):
    from vdx._lib import VdxError
    gpu = world["gpu"]
    with pytest.raises(VdxError, match="does not fit"):
        run(world, torch.zeros(2, 309, ckpt_dir.CROSS, dtype=torch.float16, device=gpu))
    with pytest.raises(VdxError, match="does not fit"):
        run(world, torch.zeros(2, F_, 309, ckpt_dir.CROSS, dtype=torch.float16, device=gpu))


@pytest.mark.parametrize("n", [77, 128])
def test_short_text_keeps_the_bits_of_the_old_constant(world, n):
    from vdx.unet3d import TEXT_PAD
    m, text = world["m"], world["text"][:, :n].contiguous().to(world["gpu"])
    got = run(world, text)
    assert m._text_pad == TEXT_PAD == 128
    try:
        m.force_text_pad = TEXT_PAD
        forced = run(world, text.clone())
    finally:
        m.force_text_pad = None
    assert torch.equal(_bits(got), _bits(forced))
    try:                                                            # the padding is part of the cache key: another layout, same text object
        m.force_text_pad = 192
        misses = m.text_cache_misses
        wider = run(world, text)
        assert m._text_pad == 192 and m.text_cache_misses == misses + 1
    finally:
        m.force_text_pad = None
    assert rel_l2(wider.float().cpu(), got.float().cpu()) <= BOUND  # zero rows past the text: masked keys, not other arithmetic


def test_per_frame_text_of_154_rows_is_the_rank_3_forward(world):
    """One text on every frame through the per-frame path (B F key / value items) against the rank-3 call, with the CFG prefix
    shared and not: two rank-3 calls, bit for bit."""
    m, text = world["m"], world["text"][:, :154].contiguous().to(world["gpu"])
    per_frame = text[:, None].expand(2, F_, 154, ckpt_dir.CROSS).contiguous()
    try:
        for prefix in (True, False):
            m.share_cfg_prefix = prefix
            want = run(world, text)
            assert not m._text_per_frame and m.last_forward_shared_prefix == prefix
            got = run(world, per_frame)
            assert m._text_per_frame and m._text_pad == 192
            assert torch.equal(_bits(got), _bits(want)), prefix
        # two different texts on the two frames differ from either rank-3 forward
        mixed = torch.stack([text, world["text"][:, 154:308].contiguous().to(world["gpu"])], dim=1).contiguous()
        assert not torch.equal(_bits(run(world, mixed)), _bits(want))
    finally:
        m.share_cfg_prefix = True


def test_a_region_at_154_rows_is_a_select_of_plain_sub_blocks(world):
    """One hard-edged region on a 64-pixel block (every cell of every level has one owner), texts of 154 rows: the forward equals,
    bit for bit, the forward whose blend is replaced by `torch.where` over the two plain sub-block results with the owner map of
    the restated tables (tests/region_ref.py); an all-255 region is the plain forward with the region's text as the prompt."""
    from vdx import ops
    from vdx.region import region_plan
    gpu, m = world["gpu"], world["m"]
    text = world["text"][:, :154].contiguous().to(gpu)
    rtext = world["text"][:1, 154:308].contiguous().to(gpu)
    mask = np.zeros((8 * H, 8 * W), np.uint8)
    mask[:, :64] = 255
    plan = region_plan([(mask, "left")], F_, H, W, 4).to(gpu)
    tabs = RR.weights((mask,), F_, H, W, 4)
    assert all(np.isin(t, (0.0, 1.0)).all() for t in tabs)
    window = (0, F_, 1, False)
    got = run(world, text, regions=(rtext, plan, window))
    blend, calls = ops.region_blend, []

    def select(subs, table, s, L, d=1, ring=False, out=None):
        tab = next(t for t in tabs if t.shape[1] == table.shape[1])
        owner = torch.from_numpy(np.concatenate([tab[tau].argmax(axis=1) for tau in RR.window_frames(F_, s, L, d, ring)])).to(gpu)
        res = torch.zeros_like(out)
        for j, sub in enumerate(subs):
            assert sub is not None
            res = torch.where((owner == j)[:, None], sub, res)
        calls.append(len(subs))
        out.copy_(res)
        return out

    try:
        ops.region_blend = select
        want = run(world, text, regions=(rtext, plan, window))
    finally:
        ops.region_blend = blend
    assert len(calls) == 16 and set(calls) == {2}
    assert torch.equal(_bits(got), _bits(want)) and not torch.equal(_bits(got), _bits(run(world, text)))
    full = region_plan([(np.full((8 * H, 8 * W), 255, np.uint8), "all")], F_, H, W, 4).to(gpu)
    swapped = torch.cat([text[:1], rtext]).contiguous()
    assert torch.equal(_bits(run(world, text, regions=(rtext, full, window))), _bits(run(world, swapped)))


@pytest.mark.parametrize("n", LONG)
def test_the_cfg_shared_prefix_on_is_off(world, n):
    m, text = world["m"], world["text"][:, :n].contiguous().to(world["gpu"])
    try:
        on = run(world, text)
        assert m.last_forward_shared_prefix
        m.share_cfg_prefix = False
        off = run(world, text)
        assert not m.last_forward_shared_prefix
    finally:
        m.share_cfg_prefix = True
    assert torch.equal(_bits(on), _bits(off))


def test_the_sharded_store_is_the_resident_forward(world):
    from vdx.unet3d import UNet3DConditionModel
    gpu, text = world["gpu"], world["text"][:, :231].contiguous().to(world["gpu"])
    want = run(world, text)
    b = UNet3DConditionModel(world["cfg"]).load_diffusers_state_dict(world["sd"], device=gpu).shard_(0, 1)
    for _ in range(2):
        assert torch.equal(_bits(run(world, text, m=b)), _bits(want))
