"""The Motion-JPEG writer's definition without a GPU: tests/mjpeg_enc_ref.py (the numpy restatement of csrc/mjpeg_enc.hip) and
`vdx.video.jpeg_header` against the bytes Pillow (libjpeg) writes, with no tolerance; and the container builder factored out
of `cv2_shim.VideoWriter.release` against a copy of the builder as it stood."""
import io
import struct

import numpy as np
import pytest

import mjpeg_enc_ref as E
import mjpeg_ref
from vdx import video
from vdx.compat import cv2_shim

Image = pytest.importorskip("PIL.Image")

CASES = E.cases()


@pytest.fixture(scope="module")
def encoded():
    """Every case through the restatement, once: {(id, restart_rows): jpeg}, and the counters of what the entropy stage met."""
    counters, out = E.Counters(), {}
    for name, img in CASES:
        for rr in E.RESTART_ROWS:
            out[name, rr] = E.encode(img[None], 92, rr, counters)[0]
    return out, counters


@pytest.mark.parametrize("name,img", CASES, ids=[c[0] for c in CASES])
def test_restatement_bytes_are_pillows(encoded, name, img):
    for rr in E.RESTART_ROWS:
        assert encoded[0][name, rr] == E.pillow_encode(img, rr), f"restart_rows={rr}"


def test_the_inputs_reach_what_a_smooth_image_never_does(encoded):
    c = encoded[1]
    assert c.stuffed >= 1, "no FF byte was stuffed"
    assert c.zrl >= 1, "no ZRL symbol"
    assert c.max_dc_size >= 10, f"largest DC difference has size {c.max_dc_size}"
    assert c.segments_whole_bytes >= 1 and c.segments_padded >= 1, (c.segments_whole_bytes, c.segments_padded)


@pytest.mark.parametrize("H", list(range(1, 34)) + [38, 72])
def test_every_height_and_its_bottom_edge(H):
    """The bottom edge: a cut row pair, replicas of the last downsampled chroma row, a dummy luma block row (H % 16 in 1..8),
    at a width with and without a dummy block column."""
    for W in (16, 24):
        img = E.content("noise", W, H, "RGB", seed=H)
        assert E.encode(img[None])[0] == E.pillow_encode(img), f"{W}x{H}"


@pytest.mark.parametrize("W", [1, 4, 8, 9, 15, 17, 20, 24, 27, 33])
def test_every_kind_of_right_edge(W):
    for H in (16, 24):
        for mode in E.MODES:
            img = E.content("noise", W, H, mode, seed=W)
            assert E.encode(img[None], 92, 1)[0] == E.pillow_encode(img, 1), f"{W}x{H} {mode}"


@pytest.mark.parametrize("quality", [30, 75, 92, 100])
def test_jpeg_header_is_pillows(quality):
    for sampling, shape in (("4:2:0", (38, 50, 3)), ("L", (38, 50))):
        for rr in (0, 1, 2):
            jpeg = E.pillow_encode(np.zeros(shape, np.uint8), rr, quality)
            head = video.jpeg_header(50, 38, sampling, quality, rr)
            assert jpeg[:len(head)] == head, (sampling, rr)
            info = video.parse_jpeg(jpeg)
            assert info.scan[0] == len(head) and info.sampling == sampling
            assert info.restart_interval == rr * (4 if sampling == "4:2:0" else 7)
            assert info.huffman == video.STANDARD_HUFFMAN if sampling == "4:2:0" else info.huffman[(1, 0)] == video.STANDARD_HUFFMAN[(1, 0)]
            assert info.quant[0] == video.quant_tables(quality)[0].tolist()


def test_encoder_tables_are_the_canonical_codes():
    import mjpeg_enc
    t = video.encoder_tables()
    for (tc, th), payload in video.STANDARD_HUFFMAN.items():
        codes = mjpeg_enc.codes_of(payload)
        base = 16 if tc else 0
        for sym in range(256 if tc else 16):
            want = (codes[sym][1] << 16) | codes[sym][0] if sym in codes else 0
            assert int(t[th, base + sym]) == want


def test_refusals_on_the_host():
    with pytest.raises(video.VdxError):
        video.jpeg_header(16, 16, "4:4:4")
    with pytest.raises(video.VdxError):
        video.jpeg_header(0, 16, "L")
    with pytest.raises(video.VdxError):
        video.jpeg_header(70000, 16, "L")
    with pytest.raises(video.VdxError):
        video.encode_frames(np.zeros((1, 16, 16, 3), np.uint8))


# ---------------------------------------------------------------------------------------------
# The container: VideoWriter's file must not change by a byte
# ---------------------------------------------------------------------------------------------
def _old_release_bytes(jpegs, fps, w, h):
    """The file `VideoWriter` wrote before its box builder was factored out: a copy of open() + write() + release() as they
    stood, on bytes instead of a file."""
    _box, _full = cv2_shim._box, cv2_shim._full
    out = _box(b"ftyp", b"isom" + struct.pack(">I", 0x200) + b"isomiso2mp41")
    mdat_pos = len(out)
    body = b"".join(jpegs)
    out += struct.pack(">I", 8 + len(body)) + b"mdat" + body
    sizes, n = [len(j) for j in jpegs], len(jpegs)
    ts = max(int(round(fps * 1000)), 1)
    dur = n * 1000
    mvhd = _full(b"mvhd", 0, 0, struct.pack(">IIII", 0, 0, ts, dur) + struct.pack(">IH", 0x00010000, 0x0100) + b"\0" * 10 +
                 struct.pack(">9I", 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000) + b"\0" * 24 + struct.pack(">I", 2))
    tkhd = _full(b"tkhd", 0, 3, struct.pack(">IIIII", 0, 0, 1, 0, dur) + b"\0" * 8 + struct.pack(">HHHH", 0, 0, 0, 0) +
                 struct.pack(">9I", 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000) +
                 struct.pack(">II", w << 16, h << 16))
    mdhd = _full(b"mdhd", 0, 0, struct.pack(">IIIIHH", 0, 0, ts, dur, 0x55C4, 0))
    hdlr = _full(b"hdlr", 0, 0, struct.pack(">I", 0) + b"vide" + b"\0" * 12 + b"VideoHandler\0")
    dcd = bytes([0x04, 13, 0x6C, 0x11, 0, 0, 0]) + struct.pack(">II", 0, 0)
    esd = bytes([0x03, 3 + len(dcd) + 3, 0, 1, 0]) + dcd + bytes([0x06, 1, 2])
    entry = (b"\0" * 6 + struct.pack(">H", 1) + b"\0" * 16 + struct.pack(">HH", w, h) +
             struct.pack(">II", 0x00480000, 0x00480000) + struct.pack(">I", 0) + struct.pack(">H", 1) + b"\0" * 32 +
             struct.pack(">Hh", 24, -1) + _full(b"esds", 0, 0, esd))
    stsd = _full(b"stsd", 0, 0, struct.pack(">I", 1) + _box(b"mp4v", entry))
    stts = _full(b"stts", 0, 0, struct.pack(">III", 1, n, 1000))
    stsc = _full(b"stsc", 0, 0, struct.pack(">IIII", 1, 1, max(n, 1), 1))
    stsz = _full(b"stsz", 0, 0, struct.pack(">II", 0, n) + b"".join(struct.pack(">I", s) for s in sizes))
    stco = _full(b"stco", 0, 0, struct.pack(">II", 1, mdat_pos + 8))
    stbl = _box(b"stbl", stsd + stts + stsc + stsz + stco)
    dinf = _box(b"dinf", _full(b"dref", 0, 0, struct.pack(">I", 1) + _full(b"url ", 0, 1, b"")))
    minf = _box(b"minf", _full(b"vmhd", 0, 1, b"\0" * 8) + dinf + stbl)
    trak = _box(b"trak", tkhd + _box(b"mdia", mdhd + hdlr + minf))
    return out + _box(b"moov", mvhd + trak)


@pytest.mark.parametrize("n,fps,rr", [(3, 8, 0), (1, 23.976, 1), (0, 8, 0)])
def test_videowriter_file_is_unchanged_and_mp4_bytes_is_that_file(tmp_path, n, fps, rr):
    frames = [E.content("noise", 50, 38, "RGB", seed=i) for i in range(n)]
    path = tmp_path / "w.mp4"
    vw = cv2_shim.VideoWriter(str(path), cv2_shim.VideoWriter_fourcc(*"mp4v"), fps, (50, 38), restart_rows=rr)
    for f in frames:
        vw.write(cv2_shim.cvtColor(f, cv2_shim.COLOR_RGB2BGR))
    vw.release()
    jpegs = [E.pillow_encode(f, rr) for f in frames]
    want = _old_release_bytes(jpegs, float(fps), 50, 38)
    assert path.read_bytes() == want
    assert cv2_shim.mp4_bytes(jpegs, fps, 50, 38) == want
    if n:
        assert video.demux(want)[0] == jpegs


def test_restatement_coefficients_are_the_ones_pillow_coded():
    """Stage by stage: the restatement's coefficients equal those the reader's restatement finds in Pillow's bytes."""
    img = E.content("saturated", 47, 33, "RGB")
    stages = {}
    E.encode(img[None], stages=stages)
    blob, off, info, _ = video.plan([E.pillow_encode(img)])
    coef, err = mjpeg_ref.entropy(blob, off, info)
    assert not err.any() and np.array_equal(coef, stages["coef"])


# ---------------------------------------------------------------------------------------------
# The edges of every stage: the inputs tests/test_video_enc_stages_gpu.py puts before the kernels, pinned here without a GPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", E.QUALITIES)
def test_restatement_bytes_are_pillows_at_every_quality(quality):
    """Quality 1 (every divisor clamped to 255) to 100 (every divisor 1: the longest codes, the largest DC differences)."""
    for kind in E.KINDS:
        for W, H in E.SWEEP_SIZES:
            for mode in E.MODES:
                img = E.content(kind, W, H, mode)
                for rr in (0, 1):
                    assert E.encode(img[None], quality, rr)[0] == E.pillow_encode(img, rr, quality), (kind, W, H, mode, rr)


def test_quality_reaches_both_ends_of_the_divisors():
    assert (video.quant_tables(100) == 1).all() and (video.quant_tables(1) == 255).all()
    assert len(np.unique(video.quant_tables(50))) > 20


def test_basis_blocks_reach_the_extremes_of_stage_2():
    """The 0 / 255 sign pattern of each basis function at quality 100: bytes are Pillow's for grey and RGB, the coefficients
    are those Pillow coded, and they reach |AC| = 1020, DC -1024 ... 1016 and a DC difference of size 11."""
    blocks = E.basis_blocks()
    assert blocks.shape == (130, 8, 8) and set(np.unique(blocks)) == {0, 255}
    assert (blocks[0] == 255).all() and (blocks[1] == 0).all() and (blocks[128] == 0).all() and (blocks[129] == 255).all()
    assert all(np.array_equal(blocks[2 * k + 1], 255 - blocks[2 * k]) for k in range(64))
    assert len({b.tobytes() for b in blocks}) == 128
    for mode in E.MODES:
        img = E.basis_image(mode)
        stages, counters = {}, E.Counters()
        jpeg = E.encode(img[None], 100, 0, counters, stages)[0]
        assert jpeg == E.pillow_encode(img, 0, 100), mode
        assert E.encode(img[None], 100, 1)[0] == E.pillow_encode(img, 1, 100), mode
        blob, off, info, _ = video.plan([E.pillow_encode(img, 0, 100)])
        coef, err = mjpeg_ref.entropy(blob, off, info)
        assert not err.any() and np.array_equal(coef, stages["coef"]), mode
        if mode == "L":
            E.check_basis(stages["coef"], counters)
            zz = np.abs(stages["coef"][0].astype(np.int64))
            assert (zz.max(0)[1:] >= 127 * 8 * 0.4).all(), "every basis function's coefficient is driven far from zero"
    # the planes of the stage-2 test hold nothing but these blocks, in every component, dummy blocks included
    pl = E.basis_planes(24, 40, 2, 22)
    assert [p.shape for p in pl] == [(22, 48, 32), (22, 24, 16), (22, 24, 16)]
    for p in pl:
        seen = {p[f, y:y + 8, x:x + 8].tobytes() for f in range(22) for y in range(0, p.shape[1], 8) for x in range(0, p.shape[2], 8)}
        assert seen == {b.tobytes() for b in blocks}


SETS = E.coef_sets()


def test_the_coefficient_sets_are_the_ones_the_issue_names():
    assert sorted(SETS) == sorted(["max-bits-L-dri0", "max-bits-L-dri1", "max-bits-420-dri0", "max-bits-420-dri1", "all-ones", "zrl-L",
                                   "zrl-420", "zeros-300", "rst-wrap", "one-segment-dri2", "one-segment-dri7"] +
                                  [f"mod8-{m}" for m in range(8)])
    in_domain = {n for n, e in SETS.items() if E.in_reader_domain(e)}
    assert in_domain == {n for n in SETS if not n.startswith(("max-bits", "all-ones"))}


@pytest.mark.parametrize("name", sorted(SETS))
def test_coefficient_set_has_one_stream_by_two_hands_and_reads_back(name):
    """The restatement's scan equals the hand writer's (tests/mjpeg_enc.py: another definition of the stream), the reader's
    restatement finds the coefficients that were put in, and the set reaches what it exists for."""
    entry = SETS[name]
    header, scan, jpeg, hand = E.coef_stream(entry)
    assert hand[:len(header)] == header and hand[-2:] == b"\xff\xd9"
    assert scan == hand[len(header):-2]
    blob, off, info, _ = video.plan([jpeg])
    assert info["restart_interval"] == entry[4]
    coef, err = mjpeg_ref.entropy(blob, off, info)
    assert not err.any() and np.array_equal(coef[0], entry[3])
    E.check_coef_set(name, entry)


def test_slots_of_adds_up_to_the_scan():
    for name, (layout, W, H, coef, dri) in SETS.items():
        raws, lengths, step = E.segments(coef, W, H, layout, dri)
        slots = E.slots_of(raws, step, len(lengths))
        assert len(slots) == len(lengths) and sum(slots) == len(E.entropy(coef, W, H, layout, dri)[0]), name
        assert max(slots) <= 2 * E.SLOT_BYTES + 2
