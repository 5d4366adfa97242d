"""A minimal baseline JPEG writer for the tests of the Motion-JPEG reader: from coefficient blocks to the bytes of one
frame.  It exists so that a test can put any coefficient, any Huffman table and any bit pattern in front of vdx/video.py and
csrc/mjpeg.hip, which no encoder that starts from 8-bit samples will produce: ZRL runs, a block that ends at k = 63 without
EOB, DC differences of size 11, codes of 16 bits, FF 00 as the last entropy byte, and the invalid streams the decoder must
refuse (a run past k = 63, a bit pattern no code matches, a DC symbol above 15, a stream that stops inside a symbol).

    write(sampling, W, H, blocks, quant, dri=0, huffman=None, cut=None) -> Written(jpeg, seg_bits)

`blocks` holds the frame's blocks in the decoder's order (component after component, each row-major over its padded MCU
extent: mjpeg_ref._geometry).  A block is either 64 integers in natural (row-major) order, or a list of operations written
as they stand:
    ("dc", diff)           a DC difference (the writer's prediction moves with it)
    ("ac", run, value)     run zeros, then a non-zero coefficient
    ("zrl",)  ("eob",)     the symbols 0xF0 and 0x00
    ("sym", "dc" | "ac", s)  the Huffman code of symbol s from the component's DC / AC table, nothing else
    ("bits", value, n)     n raw bits
`quant`: [components][64] in natural order, 1..255; component c uses table c.  `huffman`: {(class, id): 16 counts + symbols}
as `video.parse_jpeg(...).huffman` returns them; the first component uses id 0, the others id 1 where there is one.
`cut`: {segment: bits}; that restart interval is cut after so many bits.  Every segment is padded to a byte with 1-bits."""
import io
import struct
from typing import NamedTuple

import numpy as np

from vdx import video

import mjpeg_ref

ZIGZAG = np.asarray(video._ZIGZAG)
SAMPLINGS = {"L": 0, "4:4:4": 1, "4:2:0": 2}


class Written(NamedTuple):
    jpeg: bytes
    seg_bits: list          # bits of every segment before the padding


def standard_tables():
    """The four tables of Annex K, as Pillow writes them without `optimize`: {(class, id): 16 counts + symbols}."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, format="JPEG", quality=90)
    return dict(video.parse_jpeg(buf.getvalue()).huffman)


def table_of(lengths):
    """{symbol: code length} -> 16 counts + symbols (symbols of one length keep the dictionary's order)."""
    counts = [0] * 16
    syms = []
    for ln in range(1, 17):
        here = [s for s, n in lengths.items() if n == ln]
        counts[ln - 1] = len(here)
        syms += here
    assert len(syms) == len(lengths), "code lengths are 1..16"
    return bytes(counts) + bytes(syms)


def codes_of(payload):
    """16 counts + symbols -> {symbol: (code, length)}: the canonical assignment of the standard's Annex C."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(payload[ln - 1]):
            out[payload[16 + k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def block_ops(blk, pred):
    """64 coefficients in natural order -> the operations of a regular encoder."""
    zz = np.asarray(blk, np.int64)[ZIGZAG]
    ops = [("dc", int(zz[0]) - pred)]
    at = 1
    for k in np.flatnonzero(zz[1:]) + 1:
        run = int(k) - at
        while run > 15:
            ops.append(("zrl",))
            run -= 16
        ops.append(("ac", run, int(zz[k])))
        at = int(k) + 1
    if at < 64:
        ops.append(("eob",))
    return ops


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc = (self.acc << n) | value
        self.n += n

    def bytes(self, cut=None):
        acc, n = self.acc, self.n
        if cut is not None and cut < n:
            acc, n = acc >> (n - cut), cut
        fill = -n % 8
        acc = (acc << fill) | ((1 << fill) - 1)
        return acc.to_bytes((n + fill) // 8, "big").replace(b"\xff", b"\xff\x00")


def _emit(b, ops, dc, ac, pred):
    for op in ops:
        if op[0] == "dc":
            size = abs(op[1]).bit_length()
            b.put(*dc[size])
            if size:
                b.put(op[1] if op[1] >= 0 else op[1] + (1 << size) - 1, size)
            pred += op[1]
        elif op[0] == "ac":
            size = abs(op[2]).bit_length()
            assert 0 <= op[1] <= 15 and 1 <= size <= 15
            b.put(*ac[(op[1] << 4) | size])
            b.put(op[2] if op[2] >= 0 else op[2] + (1 << size) - 1, size)
        elif op[0] == "zrl":
            b.put(*ac[0xF0])
        elif op[0] == "eob":
            b.put(*ac[0x00])
        elif op[0] == "sym":
            b.put(*(dc if op[1] == "dc" else ac)[op[2]])
        elif op[0] == "bits":
            b.put(op[1], op[2])
        else:
            raise ValueError(op)
    return pred


def _segment(marker, body):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(body) + 2) + body


def write(sampling, W, H, blocks, quant, dri=0, huffman=None, cut=None):
    layout = SAMPLINGS[sampling]
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    assert len(blocks) == boff[-1], f"{len(blocks)} blocks, the frame has {boff[-1]}"
    huffman = huffman or standard_tables()
    quant = np.asarray(quant).reshape(ncomp, 64)
    assert quant.min() >= 1 and quant.max() <= 255
    ids = [0] + [1 if (0, 1) in huffman and (1, 1) in huffman else 0] * (ncomp - 1)
    lut = {key: {s: (c, n) for s, (c, n) in codes_of(p).items()} for key, p in huffman.items()}
    head = b"\xff\xd8"
    for c in range(ncomp):
        head += _segment(0xDB, bytes([c]) + bytes(int(v) for v in quant[c][ZIGZAG]))
    head += _segment(0xC0, struct.pack(">BHHB", 8, H, W, ncomp) +
                     b"".join(bytes([c + 1, (hs[c] << 4) | hs[c], c]) for c in range(ncomp)))
    for (tc, th), payload in sorted(huffman.items()):
        head += _segment(0xC4, bytes([(tc << 4) | th]) + payload)
    if dri:
        head += _segment(0xDD, struct.pack(">H", dri))
    head += _segment(0xDA, bytes([ncomp]) + b"".join(bytes([c + 1, (ids[c] << 4) | ids[c]]) for c in range(ncomp)) + bytes([0, 63, 0]))
    nmcu = mcux * mcuy
    step = dri or nmcu
    scan, seg_bits = b"", []
    for si, m0 in enumerate(range(0, nmcu, step)):
        b = _Bits()
        pred = [0] * ncomp
        for m in range(m0, min(m0 + step, nmcu)):
            my, mx = divmod(m, mcux)
            for c in range(ncomp):
                dc, ac = lut[(0, ids[c])], lut[(1, ids[c])]
                for by in range(hs[c]):
                    for bx in range(hs[c]):
                        blk = blocks[boff[c] + (my * hs[c] + by) * bw[c] + mx * hs[c] + bx]
                        ops = blk if isinstance(blk, list) else block_ops(blk, pred[c])
                        pred[c] = _emit(b, ops, dc, ac, pred[c])
        if si:
            scan += bytes([0xFF, 0xD0 + (si - 1) % 8])
        scan += b.bytes(None if cut is None else cut.get(si))
        seg_bits.append(b.n)
    return Written(head + scan + b"\xff\xd9", seg_bits)


# ---------------------------------------------------------------------------------------------
# Streams shared by tests/test_video_host.py (against Pillow and the restatement) and tests/test_video_gpu.py (the kernels)
# ---------------------------------------------------------------------------------------------
def patch_dqt(jpeg, fn):
    """Rewrite only the 64 values of every quantisation table: fn(uint8 [64]) -> values 1..255."""
    out, pos = bytearray(jpeg), 2
    while jpeg[pos + 1] != 0xDA:
        ln = struct.unpack_from(">H", jpeg, pos + 2)[0]
        if jpeg[pos + 1] == 0xDB:
            for p in range(pos + 4, pos + 2 + ln, 65):
                q = np.asarray(fn(np.frombuffer(jpeg[p + 1:p + 65], np.uint8).astype(np.int64)))
                assert q.min() >= 1 and q.max() <= 255
                out[p + 1:p + 65] = q.astype(np.uint8).tobytes()
        pos += 2 + ln
    return bytes(out)


DQT_PATCHES = {"x4": lambda q: np.minimum(q * 4, 255), "+40": lambda q: np.minimum(q + 40, 255), "255": lambda q: np.full(64, 255)}


def dqt_family():
    """48 files: a Pillow-encoded 38x50 noise image (two seeds, quality 30 / 75 / 92 / 100, 4:2:0 and 4:4:4) whose quantisation
    tables alone were rewritten to larger legal values -> [(name, original jpeg, patched jpeg)]."""
    from PIL import Image
    out = []
    for seed in (1, 2):
        img = np.random.default_rng(seed).integers(0, 256, (38, 50, 3), dtype=np.uint8)
        for quality in (30, 75, 92, 100):
            for sub in (2, 0):
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=sub)
                for name, fn in DQT_PATCHES.items():
                    out.append((f"s{seed}-q{quality}-sub{sub}-{name}", buf.getvalue(), patch_dqt(buf.getvalue(), fn)))
    return out


def custom_tables(symbols_dc, symbols_ac):
    """Tables whose codes are all 10..16 bits long (none fits the decoder's 9-bit lookahead), one id for every component."""
    lengths = lambda syms: {s: 10 + i % 7 for i, s in enumerate(syms)}      # noqa: E731
    return {(0, 0): table_of(lengths(symbols_dc)), (1, 0): table_of(lengths(symbols_ac))}


def _block(dc=0, **ac):
    """dc and z<k>=value for zigzag position k -> 64 coefficients in natural order."""
    b = np.zeros(64, np.int64)
    b[0] = dc
    for k, v in ac.items():
        b[ZIGZAG[int(k[1:])]] = v
    return b


def valid_streams():
    """Hand-encoded VALID frames an encoder from pixels never writes -> {name: (sampling, W, H, blocks [bpf][64] int64, quant,
    Written, in_domain)}.  `blocks` are the coefficients as written; the decoder keeps their low 16 bits."""
    out = {}

    def add(name, sampling, W, H, blocks, quant=1, in_domain=True, **kw):
        ncomp = 1 if sampling == "L" else 3
        q = np.full((ncomp, 64), quant)
        out[name] = (sampling, W, H, np.stack(blocks), q, write(sampling, W, H, list(blocks), q, **kw), in_domain)

    # ZRL: one and two of them before a coefficient, a run of exactly 16 + 0, and three ZRL + run 14 reaching k = 63
    add("zrl", "L", 24, 8, [_block(40, z1=3, z20=-5, z56=7), _block(-30, z17=9, z49=-2), _block(12, z63=6)])
    # k = 63 without EOB in every block; the last value is ten 1-bits, so the segment's last entropy byte is FF (stuffed: FF 00)
    add("k63-ff00", "L", 16, 16, [_block(5, z62=1, z63=-1), _block(-7, z63=255), _block(9, z1=1, z63=1023),
                                  _block(0, z63=1023)], dri=2)
    # DC differences of size 11 (the largest the standard tables code), both signs, in domain: |DC| / 8 stays below 512
    add("dc11", "4:2:0", 16, 16, [_block(900), _block(-900), _block(1000), _block(-1047), _block(-1024), _block(1023)])
    # the prediction runs past int16 in both directions: the decoder's (short) cast wraps; no image to compare, coefficients only
    add("dc-wrap", "L", 8 * 60, 8, [_block(2047 * (i + 1)) for i in range(20)] + [_block(2047 * (19 - i)) for i in range(40)],
        in_domain=False)
    # every code 10..16 bits long, DC and AC, three components on one table each
    blocks = [_block(3 * i - 9, z1=i + 1, z2=-(2 * i + 1), **{f"z{20 + i}": 1, "z63": (-1) ** i * 2}) for i in range(6)]
    ac_syms = sorted({0x00, 0xF0} | {(r << 4) | s for r in range(16) for s in range(1, 5)})
    add("huff16", "4:2:0", 16, 16, blocks, huffman=custom_tables(list(range(12)), ac_syms))
    return out


def sized(mod8):
    """A grey frame of two blocks whose single segment is n bits long with n % 8 == mod8, and whose last symbol's last bit is
    the segment's last bit (k = 63, no EOB) -> (blocks, Written)."""
    for v in range(1, 1024):
        for w in (1, 2, 5, 11, 23, 47, 95, 191):
            blocks = [_block(17, z1=w), _block(-4, z5=3, z63=v)]
            wr = write("L", 16, 8, blocks, np.ones((1, 64)))
            if wr.seg_bits[0] % 8 == mod8:
                return np.stack(blocks), wr
    raise AssertionError("no such length")


def error_streams():
    """Frames the entropy stage must refuse -> {name: (jpeg, error code, MCU within the segment)}; all grey 32x8 (four MCUs in
    one segment) but "short", which is 16x8."""
    q = np.ones((1, 64))
    good = [_block(10 * i, z1=i + 1, z9=-3) for i in range(4)]
    out = {}
    b = list(good)
    b[2] = [("dc", 3), ("zrl",), ("zrl",), ("zrl",), ("ac", 15, 1), ("eob",)]         # k = 49, then a run of 15: k = 64
    out["code2"] = (write("L", 32, 8, b, q).jpeg, 2, 2)
    b = list(good)
    b[1] = [("bits", 0xFFFF, 16), ("dc", 1), ("eob",)]                                 # sixteen 1-bits: no code of the table
    out["code3"] = (write("L", 32, 8, b, q).jpeg, 3, 1)
    std = standard_tables()
    dc17 = {(0, 0): std[(0, 0)][:16][:8] + bytes([std[(0, 0)][8] + 1]) + std[(0, 0)][9:16] + std[(0, 0)][16:] + bytes([16]),
            (1, 0): std[(1, 0)]}
    b = list(good)
    b[3] = [("sym", "dc", 16), ("eob",)]
    out["code4"] = (write("L", 32, 8, b, q, huffman=dc17).jpeg, 4, 3)
    blocks, wr = sized(1)
    cut = write("L", 16, 8, list(blocks), q, cut={0: wr.seg_bits[0] - 1})
    assert (wr.seg_bits[0] - 1) % 8 == 0 and len(cut.jpeg) < len(wr.jpeg)       # no padding bit follows the cut
    out["short"] = (cut.jpeg, 1, 1)
    return out


# ---------------------------------------------------------------------------------------------
# The domain search: where does the integer definition (mjpeg_ref, csrc/mjpeg.hip) equal Pillow's decode?
# ---------------------------------------------------------------------------------------------
_FRAME = {"L": (8, 8, 1, 1), "4:4:4": (8, 8, 3, 3), "4:2:0": (16, 16, 6, 3)}     # W, H, blocks, components of one MCU
_SWEEP = [0.5, 0.9, 0.97, 0.99, 1.0, 1.01, 1.03, 1.1, 1.5, 3.0, 8.0]           # largest |sample| before the limit, in units of 512


def basis_gain():
    """Per natural position k: the largest |sample before the range limit| of the unit basis function, per unit product."""
    g = np.zeros(64)
    for k in range(64):
        c = np.zeros((1, 1, 64), np.int16)
        c[0, 0, k] = 1024
        g[k] = np.abs(mjpeg_ref.extents(c, np.ones((1, 3, 64), np.uint16), 8, 8, 0)[0, 2]).max() / 1024
    return g


def domain_streams(seed):
    """One-MCU frames whose amplitude sweeps across the domain's boundary -> (sampling, coefficients [blocks][64], quant
    [components][64]): every basis function alone, DC plus one AC, dense random blocks; all three layouts."""
    g = np.random.default_rng(seed)
    gain = basis_gain()
    for samp, (W, H, nb, nc) in _FRAME.items():
        for k in range(64):
            for sign in (1, -1):
                for f in _SWEEP:
                    a = f * 512 / gain[k]
                    q = int(min(255, max(1, np.ceil(a / (2047 if k == 0 else 1023)))))
                    q = int(g.integers(q, 256)) if g.random() < 0.5 else q
                    coef = np.zeros((nb, 64), np.int64)
                    coef[int(g.integers(0, nb)), k] = sign * int(round(a / q))
                    yield samp, coef, np.full((nc, 64), q)
        for k in range(1, 64):
            for f in _SWEEP:
                for dcf in (-0.9, 0.4):
                    q, qd = int(g.integers(8, 256)), int(g.integers(4, 256))
                    coef = np.zeros((nb, 64), np.int64)
                    b = int(g.integers(0, nb))
                    dc = dcf * 512 * 8
                    coef[b, 0] = int(np.clip(round(dc / qd), -2047, 2047))
                    coef[b, k] = int(np.clip(round((f * 512 - abs(dc) / 8) / gain[k] / q), -1023, 1023)) * (1 if g.random() < .5 else -1)
                    quant = np.full((nc, 64), q)
                    quant[:, 0] = qd
                    yield samp, coef, quant
        for i in range(700 if samp == "L" else 350):
            quant = g.integers(1, 256, (nc, 64))
            if i % 3 == 0:
                quant[:] = g.integers(1, 256)
            raw = g.normal(0, 1, (nb, 64)) * (g.random((nb, 64)) < g.choice([0.1, 0.3, 1.0])) * np.exp(-g.random() * np.arange(64) / 8)
            per_block = quant[[0] * (nb - nc + 1) + list(range(1, nc))]
            scale = g.choice(_SWEEP) * 512 / max(np.abs(raw).sum() / 8, 1e-6) * g.uniform(1, 6)
            yield samp, np.clip(np.round(raw * scale / per_block), -1023, 1023).astype(np.int64), quant


def domain_search(seed, product=None, pass1=None):
    """Decode every stream of domain_streams with Pillow and with the restatement; a stream is flagged as the kernel flags it.
    -> counts, the extents seen among unflagged streams, and the differing stream nearest to the domain."""
    from PIL import Image
    res = {"seed": seed, "streams": 0, "blocks": 0, "flagged": 0, "unflagged": 0, "unflagged_differ": 0, "flagged_equal": 0,
           "flagged_differ": 0, "unflagged_extents": np.zeros((3, 2), np.int64), "nearest": None, "counterexamples": []}
    groups = {s: ([], [], []) for s in _FRAME}
    for samp, coef, quant in domain_streams(seed):
        W, H, nb, nc = _FRAME[samp]
        jpeg = write(samp, W, H, list(coef), quant).jpeg
        q3 = np.ones((3, 64), np.uint16)
        q3[:nc] = quant
        groups[samp][0].append(coef.astype(np.int16))
        groups[samp][1].append(q3)
        groups[samp][2].append(np.asarray(Image.open(io.BytesIO(jpeg)).convert("L" if samp == "L" else "RGB")))
    for samp, (coefs, quants, images) in groups.items():
        W, H, nb, nc = _FRAME[samp]
        coef, quant, want = np.stack(coefs), np.stack(quants), np.stack(images)
        ext = mjpeg_ref.extents(coef, quant, W, H, SAMPLINGS[samp])
        flag = mjpeg_ref.flagged(ext, product, pass1)
        got = mjpeg_ref.color(mjpeg_ref.idct(coef, quant, W, H, SAMPLINGS[samp]), W, H, SAMPLINGS[samp])
        differ = (got != want).reshape(len(got), -1).any(1)
        res["streams"] += len(got)
        res["blocks"] += len(got) * nb
        res["flagged"] += int(flag.sum())
        res["unflagged"] += int((~flag).sum())
        res["unflagged_differ"] += int((differ & ~flag).sum())
        res["flagged_equal"] += int((~differ & flag).sum())
        res["flagged_differ"] += int((differ & flag).sum())
        res["counterexamples"] += [(samp, coef[i], quant[i], ext[i]) for i in np.flatnonzero(differ & ~flag)]
        e = ext[~flag]
        res["unflagged_extents"][:, 0] = np.minimum(res["unflagged_extents"][:, 0], e[..., 0].min(0))
        res["unflagged_extents"][:, 1] = np.maximum(res["unflagged_extents"][:, 1], e[..., 1].max(0))
        for i in np.flatnonzero(differ & flag):                    # how far outside [-512, 511] is the nearest differing stream
            over = int(max(ext[i, 2, 1] - 511, -512 - ext[i, 2, 0]))
            if res["nearest"] is None or over < res["nearest"][0]:
                res["nearest"] = (over, samp, ext[i].tolist())
    return res
