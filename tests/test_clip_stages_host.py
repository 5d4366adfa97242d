"""CPU suite for the device stages of the CLIP score (csrc/clip.hip), the host half of tests/test_clip_stages_gpu.py: which band
and LDS span `ops.clip_preprocess` gives each height (from the tables alone, and from the wrapper with its launches captured),
Pillow's pass order and the resize tables against Pillow at the edge sizes, and the float64 references of tests/clip_stage_ref.py against independent
statements and against the caps the GPU tests apply."""
import numpy as np
import pytest
import torch

import clip_stage_ref as R
import vdx  # noqa: F401
from test_clip_score_host import emulate_resize
from vdx import ops
from vdx._lib import VdxError

LDS_ROW = 672


def test_constants_the_table_was_computed_for():
    assert (ops.CLIP_BAND, ops.CLIP_IMAGE * 3, ops.CLIP_LDS_MAX) == (8, LDS_ROW, 65536)
    assert {b for _, b, _ in R.BAND_TABLE.values()} == {8, 4, 2, 1}               # every branch of the halving loop
    assert all(R.BAND_TABLE[H][2] * LDS_ROW == 65184 for H in R.FULL_LDS_H)
    assert [H for H, _ in R.HEIGHT_SIZES] == list(R.BAND_TABLE) and {W for _, W in R.HEIGHT_SIZES} == {8, 12}


@pytest.mark.parametrize("H", list(R.BAND_TABLE) + [R.REFUSED_H])
def test_band_and_span_from_the_tables(H):
    yb, yk = ops.clip_resize_coeffs(H)
    band, span = R.choose_band(yb, ops.CLIP_BAND, ops.CLIP_LDS_MAX, ops.clip_band_span)
    if H == R.REFUSED_H:
        assert (yk.shape[1], band, span) == (101, 1, 99) and span * LDS_ROW == 66528 > ops.CLIP_LDS_MAX
        return
    assert (yk.shape[1], band, span) == R.BAND_TABLE[H]
    assert span * LDS_ROW <= ops.CLIP_LDS_MAX
    if band < ops.CLIP_BAND:                                                      # the next larger band did not fit
        assert ops.clip_band_span(yb, 2 * band) * LDS_ROW > ops.CLIP_LDS_MAX
    # what the kernel's guards (`nr = min(..., span)`, `r >= 0 && r < nr`) take for granted: they never cut anything
    assert R.band_windows_fit(yb, band, span)
    assert not R.band_windows_fit(yb, band, span - 1)
    assert (yb[:, 1] >= 1).all() and (yb[:, 1] <= yk.shape[1]).all() and (yb[:, 0] >= 0).all() and (yb.sum(1) <= H).all()


def _emulate(fr):
    """The tables in Pillow's pass order: vertical first for a frame more than 100 times taller than wide."""
    H, W = fr.shape[:2]
    return emulate_resize(fr, "vh" if ops.pillow_resizes_vertically_first(H, W, 224) else "hv")


def _launch_of(monkeypatch, H, W):
    """`ops.clip_preprocess` on a host tensor with its checks of the device and its launches replaced: -> [(symbol, args)]."""
    calls = []
    monkeypatch.setattr(ops, "check_u8_frames", lambda fr, what: tuple(fr.shape[:3]))
    monkeypatch.setattr(ops, "_p", lambda t, name, dtype=torch.float16: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "_launch", lambda symbol, *args: calls.append((symbol, args)))
    ops.clip_preprocess(torch.zeros((2, H, W, 3), dtype=torch.uint8))
    return calls


def _clip_args(call):
    symbol, (ref,) = call
    assert symbol == "vdx_clip_preprocess_u8"
    return {k: getattr(ref._obj, k) for k in ("band", "span", "kx", "ky", "F", "H", "W", "ldo")}


@pytest.mark.parametrize("H,W", R.BAND_SIZES)
def test_wrapper_launches_with_the_tabled_band(monkeypatch, H, W):
    assert not ops.pillow_resizes_vertically_first(H, W, 224) and (W == 8 or W == 12 or ops.pillow_resizes_vertically_first(H, W - 1, 224))
    call, = _launch_of(monkeypatch, H, W)
    a = _clip_args(call)
    ksize, band, span = R.BAND_TABLE[H]
    assert (a["ky"], a["band"], a["span"]) == (ksize, band, span) and (a["F"], a["H"], a["W"], a["ldo"]) == (2, H, W, 3072)
    assert a["kx"] == 3                                                           # W < 224: upscaled


@pytest.mark.parametrize("H,W", [s for s in R.HEIGHT_SIZES if s not in R.BAND_SIZES] + [(R.REFUSED_H, 8)])
def test_wrapper_resizes_a_tall_narrow_frame_vertically_first(monkeypatch, H, W):
    """Pillow's order for H > 100 W: vdx_resample_v_u8 to (2, 224, W, 3), then the kernel on 224 rows (its vertical pass is the
    identity there), whatever LDS the frame's own height would have asked for."""
    first, second = _launch_of(monkeypatch, H, W)
    assert first[0] == "vdx_resample_v_u8" and first[1][3:6] == (2, H, W) and first[1][9] == 224
    assert first[1][8] == ops.clip_resize_coeffs(H)[1].shape[1]
    a = _clip_args(second)
    assert (a["H"], a["W"], a["ky"], a["band"], a["span"]) == (224, W, 3, 8, 9)
    yb, yk = ops.clip_resize_coeffs(224)
    assert np.array_equal(yb[:, 0], np.arange(224)) and (yk[:, 0] == 1 << 22).all() and (yk[:, 1:] == 0).all()


def test_wrapper_refuses_what_lds_cannot_hold(monkeypatch):
    with pytest.raises(VdxError, match="H=11000"):
        _launch_of(monkeypatch, *R.REFUSED_SIZE)


@pytest.mark.parametrize("H,W", [(800, 8), (801, 8), (1200, 12), (1201, 12), (226, 2), (4000, 3), (300, 2), (224, 1), (200, 1)])
def test_pillow_switches_its_pass_order_past_100_to_1(H, W):
    """The rule of `ops.pillow_resizes_vertically_first` against Pillow itself, on both sides of it: the other order is off by
    one grey level somewhere (the intermediate image is uint8)."""
    pytest.importorskip("PIL.Image")
    fr = R.content("random", H, W, seed=H)[0]
    want = R.pil_resize(fr[None])[0]
    vertical_first = ops.pillow_resizes_vertically_first(H, W, 224)
    assert vertical_first == (H > 100 * W and H > 224)
    assert np.array_equal(emulate_resize(fr, "vh" if vertical_first else "hv"), want)
    if W > 1 and H != 224:
        assert not np.array_equal(emulate_resize(fr, "hv" if vertical_first else "vh"), want)


@pytest.mark.parametrize("H,W", sorted(set(R.HEIGHT_SIZES + R.BAND_SIZES + R.WIDTH_SIZES + R.MIXED_SIZES)), ids=lambda v: str(v))
def test_tables_reproduce_pillow_at_the_edge_sizes(H, W):
    pytest.importorskip("PIL.Image")
    for fr in R.content("random", H, W, seed=H + W):
        assert np.array_equal(_emulate(fr), R.pil_resize(fr[None])[0])


@pytest.mark.parametrize("kind", R.CONTENT_KINDS)
def test_tables_reproduce_pillow_on_every_content_kind(kind):
    pytest.importorskip("PIL.Image")
    for H, W in ((4320, 8), (4320, 44), (8, 225)):
        fr = R.content(kind, H, W, seed=1)
        assert fr.dtype == np.uint8 and fr.shape[1:] == (H, W, 3)
        want = R.pil_resize(fr)
        for f in range(len(fr)):
            assert np.array_equal(_emulate(fr[f]), want[f])
        if kind in ("zeros", "white"):
            assert (want == fr[0, 0, 0, 0]).all()                                  # the 2^21 rounding constant and clip8
    if kind == "impulses":
        assert [int((f > 0).any(-1).sum()) for f in R.content(kind, 9, 7)] == [1] * 5


def test_one_pixel_gives_a_constant_image():
    pytest.importorskip("PIL.Image")
    fr = np.array([[[[7, 130, 255]]], [[[0, 1, 254]]]], np.uint8)
    assert np.array_equal(R.pil_resize(fr), np.broadcast_to(fr, (2, 224, 224, 3)))
    assert np.array_equal(emulate_resize(fr[0]), np.broadcast_to(fr[0], (224, 224, 3)))


# ---- embedding + pre-LayerNorm -----------------------------------------------------------------------------------------------
def test_embed_reference_is_torch_layer_norm_in_float64():
    case = R.embed_case("gauss", 100, 49)
    c = {k: torch.from_numpy(v.astype(np.float64)) for k, v in case.items()}
    x = torch.cat([(c["cls"] + c["pos"][0]).expand(3, 1, 100), c["patch"][:3 * 49].view(3, 49, 100) + c["pos"][1:]], 1)
    want = torch.nn.functional.layer_norm(x, (100,), c["gamma"], c["beta"], float(np.float32(R.EMBED_EPS)))
    assert np.abs(R.embed_ref(case, 3) - want.numpy()).max() <= 1e-13


@pytest.mark.parametrize("regime", R.EMBED_REGIMES)
def test_embed_reference_alone_satisfies_the_bound_and_the_cap(regime):
    """fp64 -> fp16 rounding of the reference: finite, inside the rounding terms (excess <= 0), hence inside any bound the GPU
    test can apply, the cap 2^-10 max|ref| included."""
    for D in R.EMBED_D:
        for P in R.EMBED_P:
            case = R.embed_case(regime, D, P)
            assert all(v.dtype == np.float16 and np.isfinite(v).all() for v in case.values())
            ref = R.embed_ref(case, max(R.EMBED_F))
            assert ref.shape == (5, P + 1, D) and np.isfinite(ref).all() and np.abs(ref).max() <= 65504.0
            r16 = ref.astype(np.float16).astype(np.float64)
            assert np.isfinite(r16).all()
            cap = 2.0 ** -10 * np.abs(ref).max()
            assert R.embed_excess(r16, ref) <= 0.0 <= R.embed_bound(regime, ref) <= cap
            assert np.abs(r16 - ref).max() <= cap
            if regime == "constant" or D == 1:
                assert np.abs(ref - case["beta"].astype(np.float64)).max() <= 1e-9  # variance 0: beta
            if regime == "gamma0":
                assert np.array_equal(ref, np.broadcast_to(case["beta"].astype(np.float64), ref.shape))


def test_embed_excess_rejects_a_lost_term_and_a_wrong_lane():
    """The comparator on the CPU: the reference without beta, or with one element of a lane tail replaced by its neighbour, is
    outside the cap in every regime where that term is not zero."""
    for regime in ("gauss", "large_mean", "outlier", "extreme"):
        case = R.embed_case(regime, 65, 49)
        ref = R.embed_ref(case, 1)
        cap = 2.0 ** -10 * np.abs(ref).max()
        lost = ref - case["beta"].astype(np.float64)
        assert R.embed_excess(lost.astype(np.float16).astype(np.float64), ref) > cap
        wrong = ref.copy()
        wrong[..., 64] = ref[..., 63]
        assert R.embed_excess(wrong.astype(np.float16).astype(np.float64), ref) > cap


# ---- the score -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", R.COSINE_REGIMES)
def test_cosine_reference_is_torch_normalize_in_float64_and_inside_the_cap(regime):
    for D in R.COSINE_D:
        img, txt = R.cosine_case(regime, D)
        assert img.shape == (257, D) and img.dtype == txt.dtype == np.float16 and np.isfinite(img).all()
        per, mean = R.cosine_ref(img, txt)
        x, t = torch.from_numpy(img.astype(np.float64)), torch.from_numpy(txt.astype(np.float64))
        want = torch.nn.functional.normalize(x, dim=-1) @ torch.nn.functional.normalize(t, dim=-1)
        assert np.abs(per - want.numpy()).max() <= 1e-14 and abs(mean - float(want.mean())) <= 1e-14
        assert np.abs(per).max() <= 1 + 1e-15
        if regime in ("max", "subnormal") or D == 1:
            assert np.abs(np.abs(per) - 1).max() <= 1e-15
        # fp32 holds the reference within 2^-24: inside the cap D * 2^-23, which 0 <= bound <= cap never exceeds
        assert np.abs(per.astype(np.float32).astype(np.float64) - per).max() <= 2.0 ** -24
        assert 0.0 <= R.cosine_bound(regime, D) <= D * 2.0 ** -23


def test_mean_of_per_frame_is_a_sequential_fp32_sum():
    per = np.array([1.0, 2.0 ** -24, 2.0 ** -24, -1.0], np.float32)
    assert R.mean_of_per_frame_f32(per) == np.float32(0.0)                        # (1 + 2^-24) + 2^-24 = 1 in fp32, in this order
    assert R.mean_of_per_frame_f32(per[::-1]) != np.float32(0.0)
    assert R.mean_of_per_frame_f32(np.float32([0.1, 0.2, 0.4])) == np.float32(np.float32(np.float32(np.float32(0.1) + np.float32(0.2))
                                                                                         + np.float32(0.4)) / np.float32(3))
