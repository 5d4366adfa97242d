"""The animated-GIF writer's definition without a GPU: tests/gif_ref.py (the numpy restatement of csrc/gif.hip and vdx/gif.py)
against Pillow's decoder and its own, `vdx.gif.median_cut` against the second median cut, the delay rule, the header writer and
every refusal that needs no device.  The palette's sanity condition is asserted on the figures tests/gif_ref.py `parity_figures` computes
(tools/gif_parity.py records them in profiles/gif_parity.txt)."""
import io

import numpy as np
import pytest
import torch

import gif_ref as R
from vdx import gif
from vdx._lib import VdxError

Image = pytest.importorskip("PIL.Image")


def _rng(seed):
    return np.random.default_rng(seed)


def _pillow_frames(blob):
    im = Image.open(io.BytesIO(blob))
    out = []
    for t in range(im.n_frames):
        im.seek(t)
        out.append(np.asarray(im.convert("RGB")))
    return np.stack(out), im.info


def index_cases():
    rng = _rng(0)
    flat = np.full((3, 40, 64), 7, np.uint8)
    flat[1:] = 9
    y, x = np.mgrid[0:96, 0:128]
    return {
        "random-47x33-rows4": (rng.integers(0, 256, (3, 33, 47), dtype=np.uint8), 4),
        "random-one-strip-table-fills": (rng.integers(0, 256, (2, 64, 96), dtype=np.uint8), 64),
        "flat-rows1": (flat, 1),
        "flat-one-strip": (flat, 200),
        "smooth-rows8": (np.stack([(x // 8 + y // 16 + t) % 256 for t in range(2)]).astype(np.uint8), 8),
        "three-colours-rows7": (rng.integers(0, 3, (2, 130, 70), dtype=np.uint8), 7),
        "1x1": (rng.integers(0, 256, (1, 1, 1), dtype=np.uint8), 1),
    }


CASES = index_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatements_files_decode_in_pillow_and_in_its_own_decoder(name):
    idx, strip_rows = CASES[name]
    T = idx.shape[0]
    pal = _rng(1).integers(0, 256, (256, 3), dtype=np.uint8)
    blob = R.gif_file(idx, pal, strip_rows, 13, loop=0)
    got, info = _pillow_frames(blob)
    assert got.shape[0] == T and np.array_equal(got, pal[idx])
    assert info["duration"] == 130 and info["loop"] == 0
    own = R.decode_file(blob)
    assert np.array_equal(own["frames"], idx) and own["delays"] == [13] * T and own["loop"] == 0
    if "table-fills" in name:
        assert sum(1 for c, _w in R.strip_codes(idx[0].reshape(-1), True, True) if c == R.CLEAR) >= 2
    for t in range(T):                                                      # a strip's bits do not depend on any other strip
        _data, bits, alone = R.frame_stream(idx[t], strip_rows)
        spans = R.strips_of(idx.shape[1], strip_rows)
        for (a, b), (_bytes, nb), nbits in zip(spans, alone, bits):
            assert nb == nbits <= 32 * R.slot_words(strip_rows, idx.shape[1], idx.shape[2])


def test_loop_count_and_a_short_palette_reach_pillow():
    idx = _rng(2).integers(0, 5, (2, 9, 11), dtype=np.uint8)
    pal = _rng(3).integers(0, 256, (5, 3), dtype=np.uint8)
    blob = R.gif_file(idx, pal, 4, 8, loop=7)
    got, info = _pillow_frames(blob)
    assert np.array_equal(got, pal[idx]) and info["loop"] == 7 and info["duration"] == 80
    assert R.decode_file(blob)["palette"].shape == (8, 3)                   # padded with zeros to a power of two
    blocks = [R.sub_blocks(R.frame_stream(idx[t], 4)[0]) for t in range(2)]
    assert gif.file_bytes(11, 9, pal, blocks, 8, 7) == blob
    one = np.zeros((1, 3, 3), np.uint8)
    assert _pillow_frames(R.gif_file(one, pal[:1], 3, 10))[0].shape == (1, 3, 3, 3)
    assert gif.file_bytes(3, 3, pal[:1], [R.sub_blocks(R.frame_stream(one[0], 3)[0])], 10, 0) == R.gif_file(one, pal[:1], 3, 10)


def test_sub_blocks_at_the_edges_of_255():
    for n in (1, 254, 255, 256, 510, 511):
        data = bytes(_rng(n).integers(0, 256, n, dtype=np.uint8))
        sb = R.sub_blocks(data)
        assert len(sb) == n + -(-n // 255) + 1 and sb[-1] == 0 and sb[0] == min(n, 255)


# ---- the palette -----------------------------------------------------------------------------------------------------------------
def histograms():
    rng = _rng(4)
    out = {}
    h = np.zeros(R.BINS, np.int64)
    h[12345] = 99
    out["one-bin"] = h
    for n in (256, 257):
        h = np.zeros(R.BINS, np.int64)
        h[rng.choice(R.BINS, n, replace=False)] = rng.integers(1, 1000, n)
        out[f"{n}-bins"] = h
    out["every-bin"] = rng.integers(1, 50, R.BINS).astype(np.int64)
    out["equal-counts"] = np.full(R.BINS, 3, np.int64)                      # ties on count and on axis everywhere
    h = np.zeros(R.BINS, np.int64)
    for r in range(0, 32, 4):
        for g in range(0, 32, 4):
            for b in range(0, 32, 4):
                h[(r << 10) | (g << 5) | b] = 10                            # a cube: equal extents, equal box counts
    out["cube-ties"] = h
    h = np.zeros(R.BINS, np.int64)
    h[:400] = rng.integers(1, 2 ** 31, 400)                                 # counts a uint32 holds, sums beyond it
    h[0] = 2 ** 32 - 1
    out["large-counts"] = h
    f = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    out["noise-clip"] = R.hist(f)
    return out


HISTS = histograms()


@pytest.mark.parametrize("name", list(HISTS))
def test_median_cut_is_the_second_restatement(name):
    h = HISTS[name]
    pal = gif.median_cut(h)
    assert pal.dtype == np.uint8 and pal.ndim == 2 and pal.shape[1] == 3
    assert np.array_equal(pal, R.median_cut(h))
    occ = np.flatnonzero(h)
    assert len(pal) == min(len(occ), 256)
    if len(occ) <= 256:                                                     # exactly the bins' centres
        centres = np.stack([((occ >> 10) << 3) | 4, (((occ >> 5) & 31) << 3) | 4, ((occ & 31) << 3) | 4], axis=1)
        assert sorted(map(tuple, pal.tolist())) == sorted(map(tuple, centres.tolist()))


def test_median_cut_takes_the_devices_int32_view_of_uint32_counts():
    h = HISTS["large-counts"]
    as_i32 = h.astype(np.uint32).view(np.int32)
    assert (as_i32 < 0).any() and np.array_equal(gif.median_cut(as_i32), gif.median_cut(h))
    with pytest.raises(VdxError):
        gif.median_cut(np.zeros(R.BINS, np.int64))
    with pytest.raises(VdxError):
        gif.median_cut(np.ones(100, np.int64))


def test_palette_is_no_worse_than_a_uniform_one_on_a_gradient():
    """A sanity condition, not parity: Pillow cuts per image in 24 bits, this cuts once per clip in 15."""
    ours, uniform, lines = R.parity_figures(gif.median_cut)
    print("\n".join(lines))
    assert ours >= uniform


def test_strip_cost_is_a_modest_ratio_on_a_small_frame():
    """The same measurement at a size a test can afford; the 576 x 1024 figures are in profiles/gif_parity.txt."""
    f = R.gradient_clip(1, 64, 256)
    pal = gif.median_cut(R.hist(f))
    idx = R.index_map(f, R.lut(pal), "bayer")
    a, b = len(R.gif_file(idx, pal, 32, 13)), len(R.gif_file(idx, pal, 64, 13))
    print(f"64x256 dithered gradient: {a} bytes in two strips, {b} in one")
    assert np.array_equal(R.decode_file(R.gif_file(idx, pal, 32, 13))["frames"], idx)


# ---- the delay rule and the refusals ---------------------------------------------------------------------------------------------
def test_delay_rule():
    assert [gif.delay_cs(f) for f in (8, 10, 12.5, 16, 24, 25, 30, 50, 1, 0.5)] == [13, 10, 8, 6, 4, 4, 3, 2, 100, 200]
    assert all(gif.delay_cs(f) == R.delay_cs(f) for f in (7, 8, 9, 11, 15, 23.976, 29.97, 40))
    for bad in (0, -1, float("nan"), float("inf"), 67, 100, 1000, "fast", None, 0.001):
        with pytest.raises(VdxError, match="fps"):
            gif.delay_cs(bad)
    assert gif.default_strip_rows(1024) == 8 and gif.default_strip_rows(47) == 175 and gif.default_strip_rows(9000) == 1


def test_refusals_without_a_device():
    ok = np.zeros((2, 8, 8, 3), np.uint8)
    pal = np.zeros((4, 3), np.uint8)
    bad = [
        (dict(fps=0), "fps"), (dict(fps=float("nan")), "fps"), (dict(fps=100), "delay"), (dict(fps=-3), "fps"),
        (dict(loop=-1), "loop=-1"), (dict(loop=65536), "loop=65536"), (dict(loop=1.5), "loop"),
        (dict(dither="floyd"), "floyd"), (dict(strip_rows=0), "strip_rows=0"), (dict(strip_rows=-2), "strip_rows=-2"),
        (dict(palette=np.zeros((257, 3), np.uint8)), "257"), (dict(palette=pal.astype(np.int32)), "int32"),
        (dict(palette=torch.zeros((4, 3))), "float32"), (dict(palette=np.zeros((4, 4), np.uint8)), r"\(4, 4\)"),
        (dict(palette=np.zeros((0, 3), np.uint8)), r"\(0, 3\)"),
    ]
    for kw, pattern in bad:
        args = {"fps": 8, **kw}
        with pytest.raises(VdxError, match=pattern):
            gif.encode_gif(ok, **args)
    for frames, pattern in ((ok[:0], "T=0"), (np.zeros((1, 0, 8, 3), np.uint8), "H=0"), (np.zeros((1, 8, 0, 3), np.uint8), "W=0"),
                            (ok.astype(np.float32), "uint8"), (ok[..., :2], "uint8 RGB"), ([], "T=0")):
        with pytest.raises(VdxError, match=pattern):
            gif.encode_gif(frames, 8)
    wide = np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), (1, 1, 65536, 3), (0, 0, 0, 1))
    with pytest.raises(VdxError, match="W=65536"):
        gif.encode_gif(wide, 8)
    tall = np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), (1, 65536, 1, 3), (0, 0, 0, 1))
    with pytest.raises(VdxError, match="H=65536"):
        gif.encode_gif(tall, 8)
    huge = np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), (2, 65535, 65535, 3), (0, 0, 0, 1))
    with pytest.raises(VdxError, match="2\\^32"):
        gif.encode_gif(huge, 8)
    with pytest.raises(VdxError, match="GPU"):
        gif.encode_gif(ok, 8, device="cpu")
    for kw, pattern in ((dict(fps=100, dither="bayer", loop=0), "delay"), (dict(fps=8, dither="x", loop=0), "'x'"),
                        (dict(fps=8, dither="none", loop=70000), "70000")):
        with pytest.raises(VdxError, match=pattern):
            gif.check_job_args(**kw)


def test_the_job_takes_the_flags_and_the_config_does_not():
    from vdx.pipeline import GIF_RECORD_KEYS, build_arg_parser, config_from_args, gif_record
    a = build_arg_parser().parse_args(["--out_gif", "x.gif", "--gif_dither", "none", "--gif_loop", "3"])
    assert (a.out_gif, a.gif_dither, a.gif_loop) == ("x.gif", "none", 3)
    d = build_arg_parser().parse_args([])
    assert (d.out_gif, d.gif_dither, d.gif_loop) == (None, "bayer", 0)
    cfg = config_from_args(a)
    assert not any("gif" in k for k in vars(cfg))
    assert gif_record({"rank": 0, "gif": {"frames": 8}}) == {"gif": {"frames": 8}} and gif_record({"rank": 0}) == {}
    assert GIF_RECORD_KEYS == ("frames", "colors", "bytes", "delay_cs", "dither", "strip_rows")
