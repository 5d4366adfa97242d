"""-m gpu: each device stage of the CLIP score (csrc/clip.hip) on its own, at its edges: the resize front end against Pillow and
torch-CPU bit for bit at every band of the LDS halving and at frames smaller than the filter, the embedding + pre-LayerNorm and
the cosine score against the float64 statements of tests/clip_stage_ref.py, and quick_gelu's grid-stride tail.  The bounds are
4x what profiles/clip_stage_parity.txt measured on the MI355X, under caps that the references alone satisfy
(tests/test_clip_stages_host.py); every figure is printed before it is asserted (`pytest -s`)."""
import numpy as np
import pytest
import torch

import clip_stage_ref as R
import test_activations_host as H16

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")

SENTINEL = 0x5A5A                       # int16 pattern of untouched fp16 output (203.25: no stage here writes a buffer full of it)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _dev16(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to(gpu).view(torch.float16)


# ---- 1. the front end ------------------------------------------------------------------------------------------------------------
def _check_front_end(gpu, fr):
    """u8 == Pillow, rows == unfold_patches(reference_pixels(fr)).half() in every bit, with and without `return_u8`; the frames
    are left as they were."""
    from vdx import ops
    t = torch.from_numpy(fr.copy()).to(gpu)
    rows, u8 = ops.clip_preprocess(t, return_u8=True)
    alone = ops.clip_preprocess(t)
    want_u8 = R.pil_resize(fr)
    bad = np.argwhere(u8.cpu().numpy() != want_u8)
    assert bad.size == 0, f"{len(bad)} bytes differ from Pillow; the first (frame, y, x, c): {bad[0]}"
    want = R.unfold_patches(R.pixels_of_u8(want_u8)).half()
    assert rows.shape == (len(fr) * 49, 3072) and torch.equal(_bits(rows), _bits(want))
    assert torch.equal(_bits(alone), _bits(rows))
    assert torch.equal(t.cpu(), torch.from_numpy(fr))
    return u8


@pytest.mark.parametrize("H,W", sorted(set(R.HEIGHT_SIZES + R.BAND_SIZES + R.WIDTH_SIZES + R.MIXED_SIZES)), ids=lambda v: str(v))
def test_front_end_is_pillow_bit_for_bit_at_the_edge_sizes(gpu, H, W):
    """Every height of the band table twice: 8 or 12 pixels wide (H > 100 W: Pillow's vertical pass first, and ours) and at the
    narrowest width that reaches the kernel at that height, so that bands 8, 4, 2 and 1 each run, three of them with LDS full;
    widths with kx from 3 to 71; one axis up and the other down; frames smaller than the filter support."""
    u8 = _check_front_end(gpu, R.frames_like_video(2, H, W, seed=H + W))
    if (H, W) == (1, 1):
        assert bool((u8 == u8[:, :1, :1]).all())


@pytest.mark.parametrize("kind", R.CONTENT_KINDS)
@pytest.mark.parametrize("H,W", R.FULL_LDS_SIZES + [(8, 225), (3, 3)], ids=lambda v: str(v))
def test_front_end_content_that_exposes_a_wrong_tap_or_weight(gpu, H, W, kind):
    u8 = _check_front_end(gpu, R.content(kind, H, W, seed=2))
    if kind in ("zeros", "white"):
        assert bool((u8 == (0 if kind == "zeros" else 255)).all())


def test_front_end_refuses_a_height_lds_cannot_hold_and_launches_nothing(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    H, W = R.REFUSED_SIZE
    out = torch.full((2 * 49, 3072), 7.0, dtype=torch.float16, device=gpu)
    fr = torch.zeros((2, H, W, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(VdxError, match="H=11000"):
        ops.clip_preprocess(fr, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # eight pixels wide the same height is Pillow's vertical-first case: nothing to hold in LDS, and computed
    _check_front_end(gpu, R.frames_like_video(2, H, 8, seed=4))


def test_front_end_layout_pitched_input_and_sliced_output(gpu):
    from vdx import ops
    H, W = 2464, 25                                                     # band 4
    fr = R.content("random", H, W, seed=5)
    wide = torch.zeros((2, H + 5, W + 6, 3), dtype=torch.uint8, device=gpu)
    wide[:, 2:2 + H, 1:1 + W] = torch.from_numpy(fr).to(gpu)
    view = wide[:, 2:2 + H, 1:1 + W]
    assert not view.is_contiguous() and view.stride(1) % 2 == 1 and (view.data_ptr() - wide.data_ptr()) % 2 == 1
    before = wide.clone()
    buf = torch.full((2 * 49 + 1, 3072 + 24), 0, dtype=torch.int16, device=gpu).fill_(SENTINEL).view(torch.float16)
    rows, u8 = ops.clip_preprocess(view, out=buf[:, 8:8 + 3072], return_u8=True)
    assert rows.data_ptr() == buf.data_ptr() + 16 and rows.stride(0) == 3096
    assert torch.equal(wide, before)
    want_u8 = R.pil_resize(fr)
    assert np.array_equal(u8.cpu().numpy(), want_u8)
    b = _bits(buf)
    assert torch.equal(b[:98, 8:8 + 3072], _bits(R.unfold_patches(R.pixels_of_u8(want_u8)).half()))
    assert bool((b[:, :8] == SENTINEL).all()) and bool((b[:, 8 + 3072:] == SENTINEL).all()) and bool((b[98] == SENTINEL).all())
    assert torch.equal(_bits(ops.clip_preprocess(view)), b[:98, 8:8 + 3072])
    # the pitched view of a frame that Pillow resizes vertically first
    assert torch.equal(ops.clip_preprocess(view[:, :, :8]), ops.clip_preprocess(view[:, :, :8].contiguous()))
    assert np.array_equal(ops.clip_preprocess(view[:, :, :8], return_u8=True)[1].cpu().numpy(), R.pil_resize(fr[:, :, :8]))


@pytest.mark.parametrize("filter", ["bilinear", "bicubic"])
def test_resize_u8_takes_pillows_order_for_a_tall_narrow_frame(gpu, filter):
    from vdx import ops
    for (H, W), (h, w) in (((2464, 8), (224, 224)), ((801, 8), (100, 40)), ((800, 8), (100, 40)), ((801, 8), (900, 40))):
        fr = R.content("random", H, W, seed=6)
        got = ops.resize_u8(torch.from_numpy(fr).to(gpu), h, w, filter).cpu().numpy()
        want = np.stack([np.asarray(Image.fromarray(f).resize((w, h), getattr(Image, filter.upper()))) for f in fr])
        assert np.array_equal(got, want), ((H, W), (h, w))


def test_front_end_entry_point_refusals(gpu):
    """vdx_clip_preprocess_u8's own refusals, through `vdx_last_error`: nothing is launched (the output keeps its sentinel)."""
    import ctypes as C
    from vdx import ops
    from vdx._lib import ClipPreprocessArgs, load
    lib = load()
    F, Hh, W = 2, 16, 12
    fr = torch.zeros((F, Hh, W, 3), dtype=torch.uint8, device=gpu)
    out = torch.zeros((F * 49, 3080), dtype=torch.int16, device=gpu).fill_(SENTINEL)
    tabs = [torch.from_numpy(a).to(gpu) for a in ops.clip_resize_coeffs(W) + ops.clip_resize_coeffs(Hh)]
    span = ops.clip_band_span(ops.clip_resize_coeffs(Hh)[0], 8)

    def args(**kw):
        a = ClipPreprocessArgs()
        a.frames, a.frame_pitch, a.row_pitch = fr.data_ptr(), fr.stride(0), fr.stride(1)
        a.x_bounds, a.x_coeffs, a.y_bounds, a.y_coeffs = (t.data_ptr() for t in tabs)
        a.out, a.out_u8 = out.data_ptr(), None
        a.F, a.H, a.W, a.kx, a.ky, a.band, a.span, a.ldo = F, Hh, W, 3, 3, 8, span, 3080
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.vdx_clip_preprocess_u8(C.byref(args()), None) == 0          # the arguments the refusals below vary are good
    torch.cuda.synchronize()
    assert bool((out[:, :3072] != SENTINEL).any()) and bool((out[:, 3072:] == SENTINEL).all())
    out.fill_(SENTINEL)
    cases = [(dict(band=0), "band=0"), (dict(band=225), "band=225"), (dict(span=0), "span=0"), (dict(span=98), "LDS"),
             (dict(ldo=3071), "ldo=3071"), (dict(ldo=3076), "ldo=3076"), (dict(F=0), "F=0"), (dict(F=65536), "F=65536"),
             (dict(row_pitch=3 * W - 1), "pitches"), (dict(frame_pitch=3 * W * Hh - 1), "pitches"), (dict(H=0), "H=0"),
             (dict(W=0), "W=0"), (dict(kx=0), "kx=0"), (dict(ky=0), "ky=0")]
    cases += [({k: None}, "null") for k in ("frames", "x_bounds", "x_coeffs", "y_bounds", "y_coeffs", "out")]
    for kw, word in cases:
        assert lib.vdx_clip_preprocess_u8(C.byref(args(**kw)), None) != 0, kw
        assert word in lib.vdx_last_error().decode(), (kw, lib.vdx_last_error())
    assert lib.vdx_clip_preprocess_u8(None, None) != 0 and "null" in lib.vdx_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- 2. embedding + pre-LayerNorm ----------------------------------------------------------------------------------------------
def _embed(ops, gpu, dev, F, P, D, seq_pad, first_row=0):
    """One launch into a column slice of a sentinel buffer (ldo = D + 13, one row to spare) -> the buffer's int16 bits."""
    buf = torch.zeros((F * seq_pad + 1, D + 13), dtype=torch.int16, device=gpu).fill_(SENTINEL).view(torch.float16)
    out = ops.clip_vision_embed(dev["patch"][first_row:first_row + F * P], dev["cls"], dev["pos"], dev["gamma"], dev["beta"], F=F,
                                seq_pad=seq_pad, eps=R.EMBED_EPS, out=buf[:, 8:8 + D])
    assert out.data_ptr() == buf.data_ptr() + 16
    return _bits(buf)


@pytest.mark.parametrize("D", R.EMBED_D)
@pytest.mark.parametrize("regime", R.EMBED_REGIMES)
def test_embed_against_float64(gpu, regime, D):
    """Every P, seq_pad in (P + 1, 64) and F in (1, 3, 5), with ldp > D and ldo > D: the bound on the P + 1 rows, +0.0 in every
    bit of the padding rows, sentinels outside the slice, the same bits in any batch and from run to run."""
    from vdx import ops
    worst, outside = -np.inf, []
    for P in R.EMBED_P:
        case = R.embed_case(regime, D, P)
        Fm = max(R.EMBED_F)
        ref = R.embed_ref(case, Fm)
        dev = {k: _dev16(v, gpu) for k, v in case.items()}
        wide = torch.zeros((Fm * P, D + 11), dtype=torch.float16, device=gpu)     # ldp = D + 11, the slice 16 bytes in
        wide[:, 8:8 + D] = dev["patch"]
        packed, dev["patch"] = dev["patch"], wide[:, 8:8 + D]
        before = {k: v.clone() for k, v in dev.items()}
        bound = R.embed_bound(regime, ref)
        for seq_pad in (P + 1, 64):
            full = None
            for F in sorted(R.EMBED_F, reverse=True):
                b = _embed(ops, gpu, dev, F, P, D, seq_pad)
                rows = b[:F * seq_pad, 8:8 + D].reshape(F, seq_pad, D)
                assert bool((b[:, :8] == SENTINEL).all()) and bool((b[:, 8 + D:] == SENTINEL).all()) and bool((b[-1] == SENTINEL).all())
                assert bool((rows[:, P + 1:] == 0).all()), "a padding row is not +0.0"
                got = rows[:, :P + 1].numpy().view(np.float16).astype(np.float64)
                excess = R.embed_excess(got, ref[:F])
                worst = max(worst, excess)
                if excess > bound:
                    outside.append((P, seq_pad, F, excess, bound))
                if regime == "gamma0":
                    assert np.array_equal(got, np.broadcast_to(case["beta"].astype(np.float64), got.shape))
                if full is None:
                    full = rows
                    assert torch.equal(_embed(ops, gpu, dev, F, P, D, seq_pad), b)               # run to run
                else:
                    assert torch.equal(rows, full[:F]), "a frame's rows depend on the batch"
            # frame 2 alone, from packed rows (ldp = D) and into a tensor of its own (ldo = D)
            alone = ops.clip_vision_embed(packed[2 * P:3 * P].clone(), dev["cls"], dev["pos"], dev["gamma"], dev["beta"], F=1,
                                          seq_pad=seq_pad, eps=R.EMBED_EPS)
            assert torch.equal(_bits(alone).reshape(seq_pad, D), full[2])
        for k, v in dev.items():
            assert torch.equal(_bits(v), _bits(before[k]))
    print(f"PARITY embed {regime} D={D}: worst excess {worst:.3e} (bound at P=50: {bound:.3e}, cap {2.0 ** -10 * np.abs(ref).max():.3e})")
    assert not outside, f"(P, seq_pad, F, excess, bound) outside the bound: {outside}"


def test_embed_refusals(gpu):
    from vdx import ops
    from vdx._lib import VdxError, load
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device=gpu)       # noqa: E731
    with pytest.raises(VdxError):
        ops.clip_vision_embed(z(49, 1025), z(1025), z(50, 1025), z(1025), z(1025), F=1, seq_pad=64)
    with pytest.raises(VdxError):
        ops.clip_vision_embed(z(49, 64), z(64), z(50, 64), z(64), z(64), F=1, seq_pad=49)
    lib, out = load(), torch.zeros((64, 1032), dtype=torch.int16, device=gpu).fill_(SENTINEL)
    p, v, pos = z(49, 1032), z(1032), z(50, 1032)
    call = lambda P, seq_pad, D, ldp=1032, ldo=1032: lib.vdx_clip_vision_embed_f16(                  # noqa: E731
        p.data_ptr(), ldp, v.data_ptr(), pos.data_ptr(), v.data_ptr(), v.data_ptr(), 1e-5, 1, P, seq_pad, D, out.data_ptr(), ldo, None)
    for a, word in (((49, 64, 1025), "D=1025"), ((49, 49, 64), "seq_pad=49"), ((49, 64, 0), "D=0"), ((49, 64, 64, 63), "leading"),
                    ((49, 64, 64, 64, 63), "leading")):
        assert call(*a) != 0 and word in lib.vdx_last_error().decode(), (a, lib.vdx_last_error())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- 3. the score ----------------------------------------------------------------------------------------------------------------
def _score(ops, img, txt):
    mean, per = ops.clip_cosine_score(img, txt)
    assert mean.shape == (1,) and per.shape == (img.shape[0],) and mean.dtype == per.dtype == torch.float32
    return mean.cpu().numpy()[0], per.cpu().numpy()


@pytest.mark.parametrize("D", R.COSINE_D)
@pytest.mark.parametrize("regime", R.COSINE_REGIMES)
def test_score_against_float64(gpu, regime, D):
    """Every F with ldi > D.  Bit for bit: `mean` is the fp32 sum of the returned per_frame in frame order over float32(F);
    per_frame[f] is the same in every batch, alone, and in a shuffled batch; the same bits from run to run."""
    from vdx import ops
    img, txt = R.cosine_case(regime, D)
    ref, _ = R.cosine_ref(img, txt)
    ldi = (D + 7) // 8 * 8 + 8
    wide = torch.zeros((len(img), ldi), dtype=torch.float16, device=gpu)
    wide[:, :D] = _dev16(img, gpu)
    t = _dev16(txt, gpu)
    before = (wide.clone(), t.clone())
    bound = R.cosine_bound(regime, D)
    worst, full, outside = 0.0, None, []
    for F in sorted(R.COSINE_F, reverse=True):
        mean, per = _score(ops, wide[:F, :D], t)
        assert mean.tobytes() == R.mean_of_per_frame_f32(per).tobytes(), (F, mean, R.mean_of_per_frame_f32(per))
        if full is None:
            full = per
            again = _score(ops, wide[:F, :D], t)
            assert again[0].tobytes() == mean.tobytes() and again[1].tobytes() == per.tobytes()
        assert per.tobytes() == full[:F].tobytes(), "per_frame depends on the batch"
        err = max(float(np.abs(per - ref[:F]).max()), abs(float(mean) - float(ref[:F].mean())))
        worst = max(worst, err)
        if err > bound:
            outside.append((F, err, bound))
    for f in (0, 5, 256):
        assert _score(ops, wide[f:f + 1, :D], t)[1].tobytes() == full[f:f + 1].tobytes()
    perm = np.random.default_rng(D).permutation(len(img))
    assert _score(ops, wide[torch.from_numpy(perm).to(gpu)][:, :D], t)[1].tobytes() == full[perm].tobytes()
    assert torch.equal(wide, before[0]) and torch.equal(t, before[1])
    print(f"PARITY cosine {regime} D={D}: worst |got - ref64| {worst:.3e} (bound {bound:.3e}, cap {D * 2.0 ** -23:.3e})")
    assert not outside, f"(F, error, bound) outside the bound: {outside}"


@pytest.mark.parametrize("D", R.COSINE_D)
def test_score_properties(gpu, D):
    """A zero row scores exactly 0, the text itself 1 and its negation -1 within the bound, and a zero text gives all zeros."""
    from vdx import ops
    img, txt = R.cosine_case("gauss", D)
    img = img[:9].copy()
    img[1], img[4], img[6], img[8] = 0.0, txt, -txt, 0.0
    x, t = _dev16(img, gpu), _dev16(txt, gpu)
    mean, per = _score(ops, x, t)
    bound = R.cosine_bound("gauss", D)
    print(f"PARITY cosine properties D={D}: |1 - cos(t, t)| {abs(per[4] - 1):.3e}, |1 + cos(-t, t)| {abs(per[6] + 1):.3e} (bound {bound:.3e})")
    assert per[1] == 0.0 and per[8] == 0.0
    assert abs(float(per[4]) - 1) <= bound and abs(float(per[6]) + 1) <= bound and per[4] == -per[6]
    assert mean.tobytes() == R.mean_of_per_frame_f32(per).tobytes()
    mean0, per0 = _score(ops, x, torch.zeros_like(t))
    assert mean0 == 0.0 and bool((per0 == 0.0).all())
    ref, _ = R.cosine_ref(img, txt)
    assert float(np.abs(per - ref).max()) <= bound


# ---- 4. quick_gelu's grid-stride tail ------------------------------------------------------------------------------------------
def test_quick_gelu_tail_sizes(gpu):
    """n = 1, 255, 257 and 4096 * 256 + 3 (three elements past one full trip of the largest grid) over all 65 536 bit patterns:
    the bits of the contiguous sweep (tests/test_activations_gpu.py::test_direct_ops[quick_gelu] bounds its values), and nothing
    written past n."""
    from vdx import ops
    bits = H16.all_fp16_bits()
    table = _bits(ops.quick_gelu(_dev16(bits.view(np.float16), gpu))).numpy().view(np.uint16)
    fin = np.isfinite(bits.view(np.float16))
    x64 = bits.view(np.float16).astype(np.float64)
    env = H16.compare("QuickGELU: vdx_quick_gelu_f16", x64[fin], table.view(np.float16).astype(np.float64)[fin], H16.quick_gelu64(x64[fin]))
    print(env.row())
    for n in (1, 255, 257, 4096 * 256 + 3):
        src = np.resize(np.roll(bits, -0x3C00 if n == 1 else 0), n)             # n = 1: one finite value that is not zero
        x = _dev16(src.view(np.float16), gpu)
        out = torch.zeros(n + 8, dtype=torch.int16, device=gpu).fill_(SENTINEL)
        y = ops.quick_gelu(x, out=out.view(torch.float16)[:n])
        got = _bits(out).numpy().view(np.uint16)
        assert y.data_ptr() == out.data_ptr()
        assert np.array_equal(got[:n], table[src.view(np.uint16)]), n
        assert (got[n:] == SENTINEL).all(), n
        assert np.array_equal(_bits(x).numpy().view(np.uint16), src.view(np.uint16))
