"""Float64 reference of vdx_gemm_f16 and the table of exact cases (no GPU; used by test_gemm_exact_host.py / _gpu.py).

out[M][N] = epilogue(gather(A)[M][K] . W[N][K]^T).  The gathers are written out as explicit zero padding and slicing:
plain rows (one or two sources), conv3x3 (pad 1 at stride 1 | 2, pad (0,1,0,1) at stride 2, nearest x2, nearest-to-size)
and tconv3 (zero frames at both clip ends); then bias, bias2 row m // rows_per_bias2, residual.  Weights go through
packing.pack_conv3x3 / pack_tconv3 / pack_geglu as the callers' do.

Exact cases use small integers (activations and weights in [-2, 2], bias / bias2 / residual in [-8, 8]): products of fp16
integers are exact, their fp32 sums are exact in any order below 2^24, and the epilogue adds in fp32 and rounds once.  With
max|ref| < 2048 every output is an fp16-exact integer, so a kernel must return the reference BIT FOR BIT in every tile
family, K-slice order and ring depth.  GEGLU cases go through the erf table and keep the project's bound.

A case is a dict: id, kind (plain | geglu | conv | tconv), variant (the pinned kernel family, vdx_gemm_args.epilogue bits
8..11), M, N, c1, c2, epi (none | bias | all | bias_res), rpb2, rows (row_begin, row_end) | None, pad (extra elements of
every leading dimension), conv = (n, h_in, w_in, h_out, w_out, stride, upsample) + pad_mode, tconv = (B, frames, hw),
ksplit, wset_rows, reserve (CUs held back while the case runs: the weights-stationary grids shrink and their blocks walk
several chunks), refused (the library rejects the call by design: the tests assert the VdxError)."""
import functools
import zlib

import numpy as np
import torch

PLAIN, CONV3X3, TCONV3 = 0, 1, 2
MODE = {"plain": PLAIN, "geglu": PLAIN, "conv": CONV3X3, "tconv": TCONV3}
TAPS = {"plain": 1, "geglu": 1, "conv": 9, "tconv": 3}

# pinned variant -> (BM, BN) of its tile; 1 9 5 2 6 are gemm_kernel (gemm.hip), 3 4 8 gemm_ring_kernel (gemm_ring.hip)
VARIANTS = {1: (128, 128), 9: (128, 128), 5: (256, 64), 2: (256, 320), 6: (256, 320), 3: (256, 320), 4: (128, 320), 8: (128, 320)}
UPS2_VARIANTS = (1, 2)          # the two kernels that carry the nearest-to-size gather
# weights-stationary families (variant 7): family -> (K, waves, chunk rows, pipelined)
WS_FAMILIES = {1: (320, 10, 64, False), 2: (320, 8, 64, True), 3: (512, 8, 32, True), 4: (640, 8, 32, True)}
WS_RESERVE = 248                # CUs held back in the `walk` cases: a grid of 8 blocks


def ws_family(M, N, K, geglu):
    """The family vdx_gemm_ws_family gives plain single-source rows without bias2 (0: not covered).  The host test checks
    this restatement against the names the library reports."""
    if N % 32 or N > 256 * 256:
        return 0
    if K == 320 and M % 64 == 0:
        return 1 if N % 320 == 0 and not (geglu and N % 256 == 0) else 2
    if K == 512 and M % 32 == 0 and N % 256 == 0:
        return 3
    if K == 640 and M % 32 == 0:
        return 4
    return 0


# ---- the case table ---------------------------------------------------------------------------------------------------
def _case(kind, variant, M, N, c1, c2=0, epi="none", rpb2=0, rows=None, pad=0, conv=None, pad_mode=0, tconv=None, ksplit=0,
          wset_rows=0, reserve=0, refused=False, tag=""):
    c = dict(kind=kind, variant=variant, M=M, N=N, c1=c1, c2=c2, epi=epi, rpb2=rpb2 if epi == "all" else 0, rows=rows, pad=pad,
             conv=conv, pad_mode=pad_mode, tconv=tconv, ksplit=ksplit, wset_rows=wset_rows, reserve=reserve, refused=refused)
    c["K"] = TAPS[kind] * (c1 + c2)
    c["exact"] = kind != "geglu"
    geo = "x".join(map(str, conv)) + f"p{pad_mode}" if conv else "x".join(map(str, tconv)) if tconv else ""
    c["id"] = "-".join(s for s in (f"v{variant}", kind, f"M{M}N{N}K{c['K']}", f"c2_{c2}" if c2 else "", geo, epi,
                                   f"rpb{c['rpb2']}" if c["rpb2"] else "", f"rows{rows[0]}_{rows[1]}" if rows else "",
                                   f"ks{ksplit}" if ksplit else "", f"wset{wset_rows}" if wset_rows else "",
                                   f"res{reserve}" if reserve else "", tag) if s)
    return c


def _conv_out(h, w, stride, pad_mode, ups, size=None):
    if ups == 1:
        h, w = 2 * h, 2 * w
    elif ups == 2:
        h, w = size
    if pad_mode == 1:
        return h // 2, w // 2
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def _conv_geometries(with_ups2):
    """(h, w, stride, pad_mode, upsample, size): 1-pixel-wide and 1-pixel images, odd sizes, three images per call."""
    g = [(1, 1, 1, 0, 0), (1, 9, 1, 0, 0), (9, 1, 1, 0, 0), (2, 2, 1, 0, 0), (5, 7, 1, 0, 0),
         (9, 10, 1, 0, 0),                   # 270 rows: an M tail behind a whole 256-row (two 128-row) tile(s)
         (5, 7, 2, 0, 0), (6, 8, 2, 0, 0), (2, 2, 2, 0, 0), (1, 1, 2, 0, 0),
         (6, 8, 2, 1, 0), (7, 9, 2, 1, 0), (2, 3, 2, 1, 0),
         (1, 1, 1, 0, 1), (3, 5, 1, 0, 1)]
    g = [x + (None,) for x in g]
    if with_ups2:
        g += [(3, 3, 1, 0, 2, (5, 6)), (7, 2, 1, 0, 2, (7, 3)), (9, 6, 1, 0, 2, (11, 9))]     # the last: 297 rows, an M tail
    return g


def _tiled_cases(v):
    BM, BN = VARIANTS[v]
    out = []
    # plain: every M edge, N edge and K value; the three epilogues; rows_per_bias2 in {1, 37, M}
    Ms = [1, 15, BM - 1, BM, BM + 1, 2 * BM + 17]
    Ns = sorted({64, BN, BN + 64} | ({BN - 64} if BN > 64 else set()))
    Ks = [64, 128, 192, 320]
    for i, M in enumerate(Ms):
        out.append(_case("plain", v, M, Ns[i % len(Ns)], Ks[i % 4], epi=("none", "bias", "all")[i % 3], rpb2=(37, 1)[i // 3 % 2],
                         pad=8 * (i % 2)))
    out.append(_case("plain", v, 2 * BM + 17, BN + 64, 320, epi="all", rpb2=1, pad=8))
    out.append(_case("plain", v, BM + 1, BN, 64, epi="all", rpb2=BM + 1))
    out.append(_case("plain", v, BM - 1, Ns[-2], 320, epi="bias", pad=16))
    out.append(_case("plain", v, BM + 1, BN + 64, 64, 128, epi="all", rpb2=37, pad=24))              # two sources, wide rows
    out.append(_case("plain", v, 2 * BM + 17, BN, 128, epi="all", rpb2=37, rows=(21, BM + 45), pad=8))   # a range inside tiles
    out.append(_case("plain", v, 15, 64, 64, 64, epi="none", rows=(3, 14)))
    # GEGLU (bounded, not exact): the layer's shapes N = 8C, and one N tail
    for M in (1, BM + 1):
        for C in (64, 320):
            out.append(_case("geglu", v, M, 8 * C, C, epi="bias"))
    out.append(_case("geglu", v, 15, BN + 64, 64, epi="bias", pad=8))
    # conv3x3: three images, so that 16-row pieces and tiles straddle image boundaries
    for i, (h, w, stride, pm, ups, size) in enumerate(_conv_geometries(v in UPS2_VARIANTS)):
        ho, wo = _conv_out(h, w, stride, pm, ups, size)
        out.append(_case("conv", v, 3 * ho * wo, (64, 320, 384)[i % 3], (64, 128)[i % 2], epi=("all", "none", "bias")[i % 3 if i != 5 else 0],
                         rpb2=ho * wo, conv=(3, h, w, ho, wo, stride, ups), pad_mode=pm, pad=8 * (i % 2)))
    # tconv3: B = 2 clips; bias + residual, and the full epilogue once
    for i, (fr, hw, C, Co) in enumerate([(1, 1, 64, 64), (2, 7, 128, 320), (3, 16, 64, 320), (5, 33, 64, 64), (1, 33, 128, 64),
                                         (5, 1, 64, 320), (2, 33, 128, 320), (3, 7, 64, 64), (5, 16, 128, 64), (2, 1, 64, 320)]):
        out.append(_case("tconv", v, 2 * fr * hw, Co, C, epi="all" if i == 3 else "bias_res", rpb2=hw, tconv=(2, fr, hw), pad=8 * (i % 2)))
    return out


def _ksplit_cases():
    """Pinned split-K on the 256x320 tile.  ksplit 3 at K = 320 leaves a slice of one K tile and N = 384 does not fill
    320-wide tiles: gemm_route refuses both (vdx_gemm_plan_ksplit, the only caller that picks a ksplit, asks for four K
    tiles per slice and fits320, so no caller reaches either).  N = 256 is the N tail the split-K kernels do take, and
    ksplit 4 at K = 576 the conv slice of the minimum two K tiles."""
    out = []
    for ks in (2, 3):
        for M in (1, 257):
            for N in (320, 384, 256):
                out.append(_case("plain", 0, M, N, 320, epi="all", rpb2=37, ksplit=ks, pad=8, refused=ks == 3 or N == 384))
        out.append(_case("plain", 0, 297, 320, 320, epi="all", rpb2=1, rows=(40, 297), ksplit=ks, refused=ks == 3))
    for ks in (2, 3, 4):
        for n, h, w in ((1, 1, 1), (1, 257, 1), (3, 9, 10)):
            for N in (320, 384, 256):
                out.append(_case("conv", 0, n * h * w, N, 64, epi="all", rpb2=h * w, conv=(n, h, w, h, w, 1, 0), ksplit=ks,
                                 refused=N == 384))
        out.append(_case("conv", 0, 270, 320, 64, epi="all", rpb2=90, rows=(37, 270), conv=(3, 9, 10, 9, 10, 1, 0), ksplit=ks))
    for ks in (2, 3):
        for B, fr, hw in ((1, 1, 1), (1, 257, 1), (2, 3, 43)):
            for N in (320, 384, 256):
                out.append(_case("tconv", 0, B * fr * hw, N, 128, epi="all", rpb2=hw, tconv=(B, fr, hw), ksplit=ks, refused=N == 384))
        out.append(_case("tconv", 0, 258, 320, 128, epi="all", rpb2=43, rows=(50, 258), tconv=(2, 3, 43), ksplit=ks))
    return out


def _ws_cases():
    """Variant 7.  K = 512 takes N in multiples of 256 only, so the listed N in {64, 320, 384} are refused there (the automatic
    route then runs the tiled kernels) and 256 / 512 stand in; the 32-row-chunk families also get M = 32 and 96.  `walk`
    cases hold back all but 8 CUs so that a block walks more chunks than its ring has stages."""
    out = []
    for fam, (K, nw, rows, _) in WS_FAMILIES.items():
        Ns = {1: [320, 640], 2: [64, 384], 3: [256, 512], 4: [64, 320, 384]}[fam]
        Ms = [64, 192, 320] if rows == 64 else [32, 96, 64, 192, 320]
        for flav in ("none", "bias", "bias_res", "geglu", "wset"):
            if flav == "wset" and fam == 3:
                continue
            ms = [64, 192, 320] if flav == "wset" else Ms
            shapes = [(M, Ns[i % len(Ns)], 0) for i, M in enumerate(ms)] + [(2368, Ns[-1], WS_RESERVE)]
            for i, (M, N, reserve) in enumerate(shapes):
                kind = "geglu" if flav == "geglu" else "plain"
                epi = {"geglu": "bias", "wset": "none"}.get(flav, flav)
                out.append(_case(kind, 7, M, N, K, epi=epi, pad=8 * (i % 2) if flav != "bias_res" else 8,
                                 wset_rows=64 if flav == "wset" else 0, reserve=reserve, tag="walk" if reserve else ""))
    for N in (64, 320, 384):                                  # K = 512 at the listed N: refused by design
        out.append(_case("plain", 7, 64, N, 512, epi="bias", refused=True))
    out.append(_case("plain", 7, 100, 320, 320, epi="bias", refused=True))                    # M no multiple of the chunk
    out.append(_case("plain", 7, 128, 320, 320, epi="bias", rows=(0, 64), refused=True))      # whole products only
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = [c for v in VARIANTS for c in _tiled_cases(v)] + _ksplit_cases() + _ws_cases()
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return tuple(out)


def group_of(c):
    """(variant label, mode) of the GPU test that runs the case."""
    label = "ksplit" if c["ksplit"] else "ws" if c["variant"] == 7 else "ups2" if c["conv"] and c["conv"][6] == 2 else f"v{c['variant']}"
    return label, c["kind"]


# ---- which instantiation a case names, and the edges it hits ----------------------------------------------------------------
def family_of(c):
    """Tile geometry of the instantiation the case pins: BM x BN (weights-stationary: chunk rows x panel columns), whether
    an N tail can exist there, the shortest K it takes."""
    if c["variant"] == 7:
        fam = ws_family(c["M"], c["N"], c["K"], c["kind"] == "geglu")
        K, nw, rows, pipe = WS_FAMILIES[fam]
        # ring stages: four where they fill the LDS exactly (K = 640 without a GELU table or a bias page behind the ring), else three
        ns = 4 if K == 640 and c["kind"] != "geglu" and not c["wset_rows"] else 3
        return dict(ws=fam, BM=rows, BN=32 * nw, n_tail_possible=fam in (2, 4), kmin=K, stages=ns)
    BM, BN = (256, 320) if c["ksplit"] else VARIANTS[c["variant"]]
    return dict(ws=0, BM=BM, BN=BN, n_tail_possible=BN != 64, kmin=64 * TAPS[c["kind"]])


def edges_of(c):
    """The edges a case hits, derived from its shape alone:
    m_below   fewer rows than one tile (weights-stationary: the smallest product the family takes)
    m_tail    whole tiles and a partial one (weights-stationary: blocks walk unequal numbers of chunks, one of them more
              than the ring has stages)
    n_tail    a partial column tile — where N % 64 == 0 (gemm_prepare) or the family's own rule admits none (the 64-wide
              tile; the weights-stationary families that take whole panels only), more than one column tile
    k_short   the shortest K walk: one 64-wide K tile per tap (K-32 rings: two stages against a three-stage prologue);
              split-K: a slice of the minimum two K tiles"""
    f = family_of(c)
    e = set()
    rows = ((c["rows"][1] or c["M"]) - c["rows"][0]) if c["rows"] else c["M"]
    if f["ws"]:
        nch = c["M"] // f["BM"]
        groups = max(1, (256 - c["reserve"]) // -(-c["N"] // f["BN"]))
        if c["M"] == max(f["BM"], c["wset_rows"]):
            e.add("m_below")
        if nch % groups and -(-nch // groups) > f["stages"]:
            e.add("m_tail")
    else:
        if rows < f["BM"]:
            e.add("m_below")
        if rows > f["BM"] and rows % f["BM"]:
            e.add("m_tail")
    if (c["N"] % f["BN"] != 0) if f["n_tail_possible"] else c["N"] > f["BN"]:
        e.add("n_tail")
    if c["ksplit"]:
        nk = c["K"] // 64
        if min((s + 1) * nk // c["ksplit"] - s * nk // c["ksplit"] for s in range(c["ksplit"])) == 2:
            e.add("k_short")
    elif c["K"] == f["kmin"]:
        e.add("k_short")
    return e


def name_kwargs(c):
    """Arguments of ops.gemm_kernel_name for the case."""
    kw = dict(M=c["M"], N=c["N"], K=c["K"], mode=MODE[c["kind"]], geglu=c["kind"] == "geglu", variant=c["variant"],
              single_source=c["c2"] == 0, residual=c["epi"] in ("all", "bias_res"), pad_mode=c["pad_mode"], ksplit=c["ksplit"],
              rows=c["rows"], wset_rows=c["wset_rows"])
    if c["conv"]:
        kw["conv"] = c["conv"]
    if c["tconv"]:
        kw["tconv"] = c["tconv"][1:]
    return kw


# ---- the operator in float64 ------------------------------------------------------------------------------------------------
def nearest_index(dst, n_in, n_out):
    """Source index of torch's "nearest" rule: floor(dst * (in / out)) with the scale and the product in fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    return [min(int(np.floor(np.float32(d) * scale)), n_in - 1) for d in range(dst)]


def conv3x3_ref(x, w, stride, pad_mode, ups, size=None):
    """x [n][C][h][w], w [Co][C][3][3] (float64) -> [n][Co][ho][wo]: upsample, explicit zero border, nine shifted slices."""
    if ups == 1:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    elif ups == 2:
        x = x[:, :, nearest_index(size[0], x.shape[2], size[0])][:, :, :, nearest_index(size[1], x.shape[3], size[1])]
    n, C, h, wd = x.shape
    lo = 0 if pad_mode == 1 else 1                      # pad (0,1,0,1): nothing above / left, one row below / right
    xp = torch.zeros(n, C, h + lo + 1, wd + lo + 1, dtype=torch.float64)
    xp[:, :, lo:lo + h, lo:lo + wd] = x
    ho, wo = (h // 2, wd // 2) if pad_mode == 1 else ((h - 1) // stride + 1, (wd - 1) // stride + 1)
    out = torch.zeros(n, w.shape[0], ho, wo, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            out += torch.einsum("nchw,oc->nohw", win, w[:, :, ky, kx])
    return out


def tconv3_ref(x, w):
    """x [B][F][hw][C], w [Co][C][3] (float64) -> [B][F][hw][Co]: one zero frame before and after every clip."""
    B, Fr, hw, C = x.shape
    xp = torch.zeros(B, Fr + 2, hw, C, dtype=torch.float64)
    xp[:, 1:Fr + 1] = x
    return sum(xp[:, t:t + Fr] @ w[:, :, t].t() for t in range(3))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))


def _wide(t, pad, col0=0):
    """`t` [r][c] as a column slice of a zero-filled fp16 buffer `pad` elements wider: (buffer, first column, columns)."""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype)
    buf[:, col0:col0 + t.shape[1]] = t
    return buf, col0, t.shape[1]


def build(c):
    """-> (operands, ref, kwargs): operands name -> (buffer, first column, columns) of fp16 CPU buffers whose column slice is
    the operand (`w`, `bias`, `wset_bias`: plain tensors), the float64 reference [M][N out], and ops.gemm's keyword arguments
    apart from the tensors."""
    from vdx import packing
    g = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    exact = c["exact"]
    kind, M, N, c1, c2, K = c["kind"], c["M"], c["N"], c["c1"], c["c2"], c["K"]

    def acts(*shape):
        if exact:
            return torch.randint(-2, 3, shape, generator=g).double()
        return torch.randn(*shape, generator=g).half().double()

    def wts(*shape):
        if exact:
            return torch.randint(-2, 3, shape, generator=g).double()
        return (torch.randn(*shape, generator=g) / np.sqrt(K)).half().double()

    def side(*shape):
        if exact:
            return torch.randint(-8, 9, shape, generator=g).double()
        return (torch.randn(*shape, generator=g) * 0.1).half().double()

    ops_, kw = {}, dict(M=M, mode=MODE[kind], variant=c["variant"], ksplit=c["ksplit"], pad_mode=c["pad_mode"])
    if c["rows"]:
        kw["row_begin"], kw["row_end"] = c["rows"]
    sets = M // c["wset_rows"] if c["wset_rows"] else 1
    if kind in ("plain", "geglu"):
        a1, a2 = acts(M, c1), acts(M, c2) if c2 else None
        w = wts(sets * N, K)
        A = torch.cat([a1, a2], 1) if c2 else a1
        ref = torch.cat([A[s * (M // sets):(s + 1) * (M // sets)] @ w[s * N:(s + 1) * N].t() for s in range(sets)])
        ops_["a"] = _wide(a1.half(), c["pad"])
        if c2:
            ops_["a2"] = _wide(a2.half(), c["pad"] + 8, 8)
        wp = w.half()
    elif kind == "conv":
        n, h, wd, ho, wo, stride, ups = c["conv"]
        x, w4 = acts(n, c1, h, wd), wts(N, c1, 3, 3)
        y = conv3x3_ref(x, w4, stride, c["pad_mode"], ups, (ho, wo))
        assert y.shape == (n, N, ho, wo), (y.shape, c["id"])
        ref = y.permute(0, 2, 3, 1).reshape(M, N)
        ops_["a"] = _wide(x.permute(0, 2, 3, 1).reshape(n * h * wd, c1).half(), c["pad"])
        wp = packing.pack_conv3x3(w4.half())
        kw["conv"] = c["conv"]
    else:
        B, Fr, hw = c["tconv"]
        x, w3 = acts(B, Fr, hw, c1), wts(N, c1, 3)
        ref = tconv3_ref(x, w3).reshape(M, N)
        ops_["a"] = _wide(x.reshape(M, c1).half(), c["pad"])
        wp = packing.pack_tconv3(w3.half().reshape(N, c1, 3, 1, 1))
        kw["tconv"] = (Fr, hw)
    if c["wset_rows"]:
        wb = side(sets, N)
        ref = ref + wb.repeat_interleave(c["wset_rows"], 0)
        ops_["wset_bias"] = wb.float()
        kw["wset_rows"] = c["wset_rows"]
    bias = side(N) if c["epi"] != "none" else None
    if bias is not None:
        ref = ref + bias
    if kind == "geglu":
        val, gate = ref.chunk(2, dim=-1)
        ref = val * gelu64(gate)
        wp, bias16 = packing.pack_geglu(wp, bias.half())
        kw["geglu"] = True
    elif bias is not None:
        bias16 = bias.half()
    if bias is not None:
        ops_["bias"] = bias16
    if c["epi"] == "all":
        b2 = side(-(-M // c["rpb2"]), N)
        ref = ref + b2.repeat_interleave(c["rpb2"], 0)[:M]
        ops_["bias2"] = _wide(b2.half(), 8)
        kw["rows_per_bias2"] = c["rpb2"]
    if c["epi"] in ("all", "bias_res"):
        res = side(M, N)
        ref = ref + res
        ops_["residual"] = _wide(res.half(), 16, 8)
    ops_["w"] = wp.contiguous()
    return ops_, ref, kw
