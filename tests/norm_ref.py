"""Host-only reference for csrc/norm.hip (numpy; no GPU, no library): the launch geometry restated, GroupNorm / fold /
LayerNorm in float64 from the fp16-rounded inputs, a float32 emulator of the statistics pass in the kernel's order, the
data regimes and the shape tables that tests/test_norm_host.py and tests/test_norm_gpu.py share.

Geometry (csrc/norm.hip): `gn_rows_for` halves the slab from 128 rows down to 8 until n_samples * slabs reaches min_blocks
(256 for the statistics pass, 1024 for the apply pass); `gn_threads` gives krows = rows a block reads in parallel
(ceil(256 / (C / 8)), 1 from C = 2048 up) and the block size krows * C / 8; thread (rsub, cv) of a slab reads rows
slab * slab_rows + rsub, + krows, ...: the first row alone (it sets the shift), then trips of four, then the tail."""
import math

import numpy as np

F32, F64 = np.float32, np.float64


# ---- geometry -----------------------------------------------------------------------------------------------------------
def rows_for(n_samples, rps, min_blocks):
    rows = 128
    while rows > 8 and n_samples * ((rps + rows - 1) // rows) < min_blocks:
        rows >>= 1
    return rows


def stat_rows(n_samples, rps, partition_samples=0):
    return rows_for(partition_samples if partition_samples > 0 else n_samples, rps, 256)


def apply_rows(n_samples, rps):
    return rows_for(n_samples, rps, 1024)


def krows_threads(C):
    """-> (krows, threads per block)."""
    nvec = C // 8
    k = 1 if nvec >= 256 else (256 + nvec - 1) // nvec
    return k, k * nvec


def nslabs(n_samples, rps, partition_samples=0):
    rows = stat_rows(n_samples, rps, partition_samples)
    return (rps + rows - 1) // rows


def round_up4(n):
    return (n + 3) & ~3


def workspace_bytes(n_samples, rps, C, G, partition_samples=0):
    return (round_up4(n_samples * nslabs(n_samples, rps, partition_samples) * G * 3) + n_samples * C * 2) * 4


def rows_of_thread(slab, rsub, slab_rows, krows, rps):
    """-> (first, trips, tail): the rows of a sample that row subset `rsub` of `slab` reads, in the kernel's order:
    `first` = [] or [row], `trips` = list of 4-tuples (the unrolled loop), `tail` = list of rows."""
    r_end = min(rps, (slab + 1) * slab_rows)
    r = slab * slab_rows + rsub
    first, trips, tail = [], [], []
    if r < r_end:
        first.append(r)
        r += krows
    while r + 3 * krows < r_end:
        trips.append((r, r + krows, r + 2 * krows, r + 3 * krows))
        r += 4 * krows
    while r < r_end:
        tail.append(r)
        r += krows
    return first, trips, tail


def features(ns, rps, C, G, part=0):
    """What the statistics pass of one shape reaches -> dict."""
    sr, (kr, nt) = stat_rows(ns, rps, part), krows_threads(C)
    nsl = (rps + sr - 1) // sr
    walks = [rows_of_thread(s, r, sr, kr, rps) for s in sorted({0, nsl - 1}) for r in range(kr)]
    per_thread = max(len(f) + 4 * len(t) + len(tl) for f, t, tl in walks)
    return dict(slab_rows=sr, krows=kr, threads=nt, nslabs=nsl, cpg=C // G, rows_per_thread=per_thread,
                apply_rows=apply_rows(ns, rps),
                unrolled_then_tail=any(t and tl for _, t, tl in walks),
                unrolled=any(t for _, t, _ in walks),
                idle_threads=any(not f for f, _, _ in walks),
                last_slab_rows=rps - (nsl - 1) * sr,
                last_slab_one_row=nsl > 1 and rps - (nsl - 1) * sr == 1,
                cpg_over_64=C // G > 64,
                block_not_wave_multiple=nt % 64 != 0)


# ---- shape tables (shared by the host and the GPU module) ----------------------------------------------------------------
# (ns, rps, c1, c2, G, partition_samples)
GN_SHAPES = [
    (1, 1, 64, 0, 32, 0), (1, 5, 320, 0, 32, 0),             # one slab, most threads idle, 280-thread blocks at C = 320
    (6, 35, 64, 0, 32, 0),                                   # krows 32 > slab_rows 8, last slab 3 rows
    (3, 300, 320, 0, 32, 0), (1, 300, 320, 0, 32, 48),       # the same rows under slab 8 and slab 32
    (2, 130, 64, 128, 32, 0),                                # cpg 6, two sources, strided ldx / ldx2 / ldy
    (2, 513, 1280, 640, 32, 0),                              # krows 2, 65 slabs, last slab 1 row
    (2, 257, 2560, 0, 32, 0), (2, 40, 320, 0, 1, 0),         # cpg 80 and cpg 320
    (3, 1000, 2048, 0, 32, 0),                               # krows 1, 8 rows per thread: first + one trip + 3 tail rows
    (2, 16389, 320, 0, 32, 0),                               # slab 128, krows 7, 18-19 rows per thread, 5-row last slab
    (1, 2049, 128, 0, 32, 0), (1, 8065, 64, 0, 32, 0), (1, 24705, 64, 0, 32, 0), (1, 32897, 64, 0, 32, 0),
    (1, 497, 64, 0, 32, 0), (1, 505, 64, 0, 32, 0), (1, 1529, 64, 0, 32, 0), (1, 1537, 64, 0, 32, 0),   # 63, 64, 192, 193 slabs
    (2, 129, 512, 0, 32, 8),                                 # the VAE's form
]
# regimes per shape: every shape gets "a"; the others go where the regime has something to say
GN_REGIMES = {
    (1, 1, 64, 0, 32, 0): "ae", (1, 5, 320, 0, 32, 0): "adg", (6, 35, 64, 0, 32, 0): "acf",
    (3, 300, 320, 0, 32, 0): "abcdefg", (1, 300, 320, 0, 32, 48): "ac", (2, 130, 64, 128, 32, 0): "adg",
    (2, 513, 1280, 640, 32, 0): "acf", (2, 257, 2560, 0, 32, 0): "adeg", (2, 40, 320, 0, 1, 0): "adg",
    (3, 1000, 2048, 0, 32, 0): "abcf", (2, 16389, 320, 0, 32, 0): "abcf", (1, 2049, 128, 0, 32, 0): "ac",
    (1, 8065, 64, 0, 32, 0): "abc", (1, 24705, 64, 0, 32, 0): "ac", (1, 32897, 64, 0, 32, 0): "abce",
    (1, 497, 64, 0, 32, 0): "ac", (1, 505, 64, 0, 32, 0): "ac", (1, 1529, 64, 0, 32, 0): "ac", (1, 1537, 64, 0, 32, 0): "ac",
    (2, 129, 512, 0, 32, 8): "abf",
}
# regime "b" stands for its two variants
REGIME_VARIANTS = {"a": ["a"], "b": ["b1", "b2"], "c": ["c"], "d": ["d"], "e": ["e"], "f": ["f"], "g": ["g"]}
GN_CASES = [(s, v) for s in GN_SHAPES for r in GN_REGIMES[s] for v in REGIME_VARIANTS[r]]
GN_EPS = 1e-5

FOLD_SHAPES = [(320, 320, 3, 128), (640, 640, 2, 192), (320, 32, 5, 64)]          # (C, N, ns, rps)
FOLD_REGIMES = ["a", "b1", "b2", "g"]          # (b) is both of its variants
FOLD_EPS = 1e-6


def case_id(shape, regime):
    return "-".join(str(v) for v in shape) + "-" + regime


def _seed(shape, regime):
    return [int(v) for v in shape] + [ord(c) for c in regime]


def wide_affine(C, rng):
    """Regime (g): gamma spanning 1e-3 .. 30 (log-uniform, both signs) with exact zeros, fp16 subnormals and +-30 planted,
    beta in +-5 (tests/test_ops_gpu.py `_wide_affine` plus the zeros)."""
    mag = np.exp(rng.uniform(math.log(1e-3), math.log(30.0), C))
    gamma = (mag * np.where(rng.random(C) < 0.25, -1.0, 1.0)).astype(np.float16)
    special = np.array([0.0, -0.0, 2.0 ** -24, -3 * 2.0 ** -24, 2.0 ** -15, 30.0, -30.0, 0.0], dtype=np.float16)
    pos = rng.permutation(C)[:special.size]
    gamma[pos] = special
    beta = rng.uniform(-5.0, 5.0, C).astype(np.float16)
    beta[pos[:2]] = np.array([5.0, -5.0], dtype=np.float16)
    return gamma, beta


def gn_inputs(shape, regime):
    """-> (x fp16 [ns][rps][C], gamma fp16 [C], beta fp16 [C]) of one (shape, regime); deterministic."""
    ns, rps, c1, c2, G, part = shape
    C = c1 + c2
    cpg = C // G
    rng = np.random.default_rng(_seed(shape, regime))
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float16)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float16)
    noise = rng.standard_normal((ns, rps, C), dtype=np.float32)
    off = rng.standard_normal((1, 1, C), dtype=np.float32)
    if regime in ("a", "g"):
        x = 2 * noise + off
        if regime == "g":
            gamma, beta = wide_affine(C, rng)
    elif regime == "b1":
        x = 4 * noise + 1500 + 0.4 * off
    elif regime == "b2":
        x = 2 * noise - 700 + 0.2 * off
    elif regime == "c":                                     # every slab has another mean: the between-slab terms dominate
        x = np.arange(rps, dtype=np.float32)[None, :, None] / 8 + noise
    elif regime == "d":                                     # M2 comes from the in-group deviation term alone
        x = np.broadcast_to(((np.arange(C) % cpg) * 0.25 + (np.arange(C) // cpg) % 7 - 3).astype(np.float32), (ns, rps, C))
    elif regime == "e":                                     # var = 0
        x = np.broadcast_to((3.5 * ((np.arange(C) // cpg + np.arange(ns)[:, None, None]) % 5 - 2)).astype(np.float32), (ns, rps, C))
    elif regime == "f":                                     # the shift of row subset 0 is an outlier 60 sigma out
        x = noise + off
        x[:, ::stat_rows(ns, rps, part), :] += 60
    else:
        raise ValueError(regime)
    return np.ascontiguousarray(x.astype(np.float16)), gamma, beta


def fold_inputs(fshape, regime):
    """-> (x, gamma, beta, w fp16 [N][C], bias fp16 [N]) for a fold case."""
    C, N, ns, rps = fshape
    x, gamma, beta = gn_inputs((ns, rps, C, 0, 32, 0), regime)
    rng = np.random.default_rng(_seed(fshape, regime) + [7])
    w = (0.05 * rng.standard_normal((N, C))).astype(np.float16)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float16)
    return x, gamma, beta, w, bias


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def eps64(eps):
    """The kernels take eps as a float."""
    return F64(F32(eps))


def ref_partial(x, G, slab_rows):
    """x [ns][rps][C] -> (n, mean, M2), each float64 [ns][nslabs][G], of every row slab."""
    x = np.asarray(x, dtype=F64)
    ns, rps, C = x.shape
    cpg, nsl = C // G, (rps + slab_rows - 1) // slab_rows
    n, mean, m2 = (np.zeros((ns, nsl, G)) for _ in range(3))
    for s in range(nsl):
        blk = x[:, s * slab_rows:min(rps, (s + 1) * slab_rows), :].reshape(ns, -1, G, cpg)
        n[:, s] = blk.shape[1] * cpg
        mean[:, s] = blk.mean(axis=(1, 3))
        m2[:, s] = ((blk - mean[:, s][:, None, :, None]) ** 2).sum(axis=(1, 3))
    return n, mean, m2


def ref_group(x, G):
    """-> (mean, var) float64 [ns][G]; var is the biased variance, two-pass."""
    x = np.asarray(x, dtype=F64)
    ns, rps, C = x.shape
    g = x.reshape(ns, rps, G, C // G)
    mean = g.mean(axis=(1, 3))
    return mean, ((g - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))


def ref_table(x, gamma, beta, G, eps):
    """-> (scale, shift, mean_c, var_c) float64 [ns][C]: scale = gamma / sqrt(var + eps), shift = beta - mean * scale."""
    mean, var = ref_group(x, G)
    cpg = np.asarray(x).shape[2] // G
    mean_c, var_c = np.repeat(mean, cpg, axis=1), np.repeat(var, cpg, axis=1)
    scale = np.asarray(gamma, dtype=F64)[None, :] / np.sqrt(var_c + eps64(eps))
    return scale, np.asarray(beta, dtype=F64)[None, :] - mean_c * scale, mean_c, var_c


def silu64(v):
    v = np.asarray(v, dtype=F64)
    return v / (1.0 + np.exp(-v))


def ref_fold(w, bias, beta, w16, mean_c):
    """bias_s [ns][N] = bias + sum_c w beta - sum_c w16 mean (w16 [ns][N][C]: the ROUNDED per-sample weights), and the
    magnitude sum (|w beta| + |w16 mean|) its bound scales with."""
    w, beta, w16 = np.asarray(w, dtype=F64), np.asarray(beta, dtype=F64), np.asarray(w16, dtype=F64)
    wb = w * beta[None, :]
    wm = w16 * mean_c[:, None, :]
    b = (0.0 if bias is None else np.asarray(bias, dtype=F64))[None, :] + wb.sum(axis=1)[None, :] - wm.sum(axis=2)
    return b, np.abs(wb).sum(axis=1)[None, :] + np.abs(wm).sum(axis=2)


def ref_layernorm(x, gamma, beta, eps):
    """-> (y, mean [M][1], rstd [M][1]) float64."""
    x = np.asarray(x, dtype=F64)
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + eps64(eps))
    return (x - mean) * rstd * np.asarray(gamma, dtype=F64) + np.asarray(beta, dtype=F64), mean, rstd


def ulp16(v):
    """fp16 spacing at v, floored at the subnormal spacing 2^-24."""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, dtype=F64)), 2.0 ** -14)))
    return np.exp2(np.minimum(e, 15.0) - 10.0)


# ---- float32 emulator of the statistics pass -------------------------------------------------------------------------------
def _merge(a, b):
    """Chan's merge of `Moments` a and b (float32 arrays), with the kernel's early outs."""
    an, am, aq = a
    bn, bm, bq = b
    with np.errstate(divide="ignore", invalid="ignore"):
        n = an + bn
        d = bm - am
        mean = am + d * (bn / n)
        q = aq + bq + d * d * (an * bn / n)
    ta, tb = bn == 0, an == 0
    return (np.where(ta, an, np.where(tb, bn, n)), np.where(ta, am, np.where(tb, bm, mean)), np.where(ta, aq, np.where(tb, bq, q)))


def emulate_stats(x, gamma, beta, G, eps, slab_rows, krows):
    """gn_partial_kernel + gn_finalize_kernel with every float operation rounded to float32 on its own (no contraction):
    shifted per-thread sums over `rows_of_thread`, the (group, row subset) stage, Chan merges over krows in ascending order,
    the finalize in float64 relative to K = the mean of slab 0.
    -> dict(n, mean, m2 [ns][nslabs][G] float32; scale, shift [ns][C] float32; thread_m2_max = largest per-thread M2)."""
    x = np.asarray(x, dtype=F32)
    ns, rps, C = x.shape
    cpg, nsl = C // G, (rps + slab_rows - 1) // slab_rows
    xp = np.zeros((ns, nsl * slab_rows, C), dtype=F32)
    xp[:, :rps] = x
    xp = xp.reshape(ns, nsl, slab_rows, C)
    valid = (np.arange(nsl * slab_rows) < rps).reshape(nsl, slab_rows)
    tmean = np.zeros((ns, nsl, krows, C), dtype=F32)
    tm2 = np.zeros_like(tmean)
    tcnt = np.zeros((nsl, krows), dtype=F32)
    for rsub in range(min(krows, slab_rows)):
        rows = xp[:, :, rsub::krows, :]                     # the first row, the trips and the tail: row after row
        ok = valid[:, rsub::krows]
        k = np.where(ok[None, :, 0, None], rows[:, :, 0, :], F32(0))
        s = np.zeros_like(k)
        ss = np.zeros_like(k)
        for i in range(rows.shape[2]):
            f = rows[:, :, i, :] - k
            m = ok[None, :, i, None]
            s = np.where(m, s + f, s)
            ss = np.where(m, ss + f * f, ss)
        cnt = ok.sum(axis=1).astype(F32)
        with np.errstate(divide="ignore"):
            inv = np.where(cnt > 0, F32(1) / cnt, F32(0)).astype(F32)[None, :, None]
        tmean[:, :, rsub] = k + s * inv
        tm2[:, :, rsub] = ss - s * s * inv
        tcnt[:, rsub] = cnt
    # (group, row subset) pairs: equal counts, so mean = average of the means, M2 = sum M2 + n * sum (mean_c - mean)^2
    mp = tmean.reshape(ns, nsl, krows, G, cpg)
    qp = tm2.reshape(ns, nsl, krows, G, cpg)
    ms = np.zeros(mp.shape[:4], dtype=F32)
    qs = np.zeros_like(ms)
    for c in range(cpg):
        ms = ms + mp[..., c]
        qs = qs + qp[..., c]
    gmean = ms / F32(cpg)
    dev = np.zeros_like(ms)
    for c in range(cpg):
        d = mp[..., c] - gmean
        dev = dev + d * d
    gq = qs + tcnt[None, :, :, None] * dev
    m = tuple(np.zeros((ns, nsl, G), dtype=F32) for _ in range(3))
    for r in range(krows):
        nr = np.broadcast_to((tcnt[:, r] * F32(cpg))[None, :, None], (ns, nsl, G))
        m = _merge(m, (nr, gmean[:, :, r], gq[:, :, r]))
    pn, pmean, pm2 = (np.ascontiguousarray(v, dtype=F32) for v in m)
    # finalize
    K = pmean[:, :1, :].astype(F64)
    nn, d = pn.astype(F64), pmean.astype(F64) - K
    N, S1, S2, Q = nn.sum(axis=1), (nn * d).sum(axis=1), (nn * d * d).sum(axis=1), pm2.astype(F64).sum(axis=1)
    mean = K[:, 0] + S1 / N
    var = np.maximum((Q + S2 - S1 * S1 / N) / N, 0.0)
    rstd = (1.0 / np.sqrt(var + eps64(eps))).astype(F32)
    a = np.repeat(rstd, cpg, axis=1) * np.asarray(gamma, dtype=F32)[None, :]
    shift = np.asarray(beta, dtype=F32)[None, :] - np.repeat(mean.astype(F32), cpg, axis=1) * a
    return dict(n=pn, mean=pmean, m2=pm2, scale=a.astype(F32), shift=shift.astype(F32), thread_m2_max=float(np.abs(tm2).max()))


# ---- the error metrics of the statistics (the figures recorded at the top of tests/test_norm_gpu.py) ------------------------
FIGURES = ("pmean", "pm2", "scale", "shift")


def stat_errors(got, x, gamma, beta, G, eps, slab_rows):
    """Largest errors of a statistics result (dict with n, mean, m2, scale, shift) against float64:
      pmean  |mean_slab - ref| / sqrt(var_slab + eps)          (in standard deviations: a large mean does not flatter it;
             the per-slab terms are returned too, as "pmean_slabs", for `pmean_ratio`)
      pm2    |M2_slab - ref| / ref                             (a reference of exactly 0 must be met exactly: then inf)
      scale  |scale - ref| / |ref|                             (gamma = 0: exactly 0, else inf)
      shift  (|shift - ref| - 2^-24 (|beta| + |mean scale|))+ / (sqrt(var + eps) |scale|)
             (net of the rounding of the final fp32 subtraction, which no order of the sums can avoid and which would
             otherwise swamp the figure wherever |gamma| is tiny; gamma = 0: exactly beta, else inf)
    -> dict of floats.  The slab counts must be exact: asserted here."""
    rn, rmean, rm2 = ref_partial(x, G, slab_rows)
    assert np.array_equal(np.asarray(got["n"], dtype=F64), rn), "slab counts differ from rows * cpg"
    e = eps64(eps)
    out = {}
    emean, sd = np.abs(got["mean"].astype(F64) - rmean), np.sqrt(rm2 / rn + e)
    out["pmean"] = float((emean / sd).max())
    out["pmean_slabs"] = (emean, sd, np.abs(rmean))
    em2 = np.abs(got["m2"].astype(F64) - rm2)
    out["pm2"] = float(np.where(rm2 > 0, em2 / np.where(rm2 > 0, rm2, 1.0), np.where(em2 == 0, 0.0, np.inf)).max())
    scale, shift, mean_c, var_c = ref_table(x, gamma, beta, G, eps)
    nz = scale != 0
    es = np.abs(got["scale"].astype(F64) - scale)
    out["scale"] = float(np.where(nz, es / np.where(nz, np.abs(scale), 1.0), np.where(es == 0, 0.0, np.inf)).max())
    esh = np.abs(got["shift"].astype(F64) - shift)
    net = np.maximum(esh - 2.0 ** -24 * (np.abs(np.asarray(beta, dtype=F64))[None, :] + np.abs(mean_c * scale)), 0.0)
    out["shift"] = float(np.where(nz, net / np.where(nz, np.sqrt(var_c + e) * np.abs(scale), 1.0), np.where(esh == 0, 0.0, np.inf)).max())
    return out


def pmean_ratio(err, figure, factor):
    """Largest |slab mean - ref| over its bound, slab by slab: factor * max(figure * sd_i, 2^-24 |mean_i|).  The second term
    is what storing THAT slab's mean in fp32 costs; it is there for the slabs whose mean the emulator happens to get
    exactly (figure 0: constant groups) and it never lends one slab the allowance of another."""
    emean, sd, absmean = err["pmean_slabs"]
    return float((emean / (factor * np.maximum(figure * sd, 2.0 ** -24 * absmean) + 1e-300)).max())


# ---- marker rows ------------------------------------------------------------------------------------------------------------
def marker_rows(rps, C, partition_samples):
    """Rows at the seams of the statistics pass's row walk under the partition of `partition_samples` samples: the first
    and last row of slab 0, slab 1 and the last slab, the first row of the unrolled loop (krows rows into the slab: the
    second row its thread reads), the last row before and the first row after the seam between the unrolled trips and
    the tail, and row rps - 1.  -> sorted list without duplicates."""
    sr, (kr, _) = stat_rows(partition_samples, rps), krows_threads(C)
    nsl = (rps + sr - 1) // sr
    rows = {rps - 1}
    for s in {0, min(1, nsl - 1), nsl - 1}:
        rows |= {s * sr, min(rps, (s + 1) * sr) - 1}
    if kr < min(sr, rps):
        rows.add(kr)
    for rsub in range(kr):
        _, trips, tail = rows_of_thread(0, rsub, sr, kr, rps)
        if trips and tail:
            rows |= {trips[-1][-1], tail[0]}
            break
    return sorted(rows)


# ---- LayerNorm dispatch (vdx_layernorm_f16) ---------------------------------------------------------------------------------
def ln_dispatch(C):
    """-> ("rows", LPR, NL): layernorm_rows_kernel<LPR, NL>, 64 / LPR rows per wave; or ("wave", NV): layernorm_kernel<NV>."""
    nvec = C // 8
    for lpr in (8, 16, 32, 64):
        if nvec % lpr == 0 and nvec // lpr <= 5:
            return ("rows", lpr, nvec // lpr)
    return ("wave", (nvec + 63) // 64)


LN_WIDTHS = {64: ("rows", 8, 1), 320: ("rows", 8, 5), 640: ("rows", 16, 5), 1280: ("rows", 32, 5), 512: ("rows", 16, 4),
             1024: ("rows", 32, 4), 2048: ("rows", 64, 4), 768: ("rows", 32, 3), 1536: ("rows", 64, 3),
             96: ("wave", 1), 32: ("wave", 1), 576: ("wave", 2), 1088: ("wave", 3), 1600: ("wave", 4)}
LN_REGIMES = ["a", "mean", "mid", "const", "g"]
LN_BIG = [(70001, 320), (140001, 64)]          # a wave walks 1-2 and 2-3 row groups on the 2048-block grid
LN_EPS = 1e-5


def ln_rows(C):
    """The row counts at which padded rows share a wave (or a block) with real ones."""
    d = LN_WIDTHS[C]
    rw = 64 // d[1] if d[0] == "rows" else 4           # rows per wave / waves per block
    return sorted({m for m in (1, rw - 1, rw, rw + 1, 4 * rw + 1) if m > 0})


def ln_inputs(M, C, regime):
    rng = np.random.default_rng([M, C] + [ord(c) for c in regime])
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float16)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float16)
    if regime in ("a", "g"):                                # regime a as for GroupNorm: N(0, 2^2) plus a per-channel offset
        x = 2 * rng.standard_normal((M, C), dtype=np.float32) + rng.standard_normal((1, C), dtype=np.float32)
        if regime == "g":
            gamma, beta = wide_affine(C, rng)
    elif regime == "mean":
        x = rng.standard_normal((M, C), dtype=np.float32) + 2000
    elif regime == "mid":                                   # a moderate row mean: 1, at 3 standard deviations
        x = 3 * rng.standard_normal((M, C), dtype=np.float32) + 1
    elif regime == "const":
        x = np.full((M, C), 3.0, dtype=np.float32)
        x[1::2] = -0.5
    else:
        raise ValueError(regime)
    return x.astype(np.float16), gamma, beta


# ---- the table of recorded figures --------------------------------------------------------------------------------------------
FIGURE_FLOORS = {"pmean": 0.0, "pm2": 2.0 ** -24, "scale": 2.0 ** -24, "shift": 2.0 ** -24}     # pmean: per slab, see pmean_ratio
RECORD_SLACK = 1.12                                      # rounding a figure up to two digits adds at most 10 %


def round_up2(v):
    """v rounded UP to two significant digits."""
    if v <= 0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(v)) - 1)
    return float(f"{math.ceil(v / q - 1e-9) * q:.1e}")


def emulator_figures(shape, regime):
    """The emulator's own errors against float64 for one case -> dict over FIGURES."""
    ns, rps, c1, c2, G, part = shape
    x, gamma, beta = gn_inputs(shape, regime)
    emu = emulate_stats(x, gamma, beta, G, GN_EPS, stat_rows(ns, rps, part), krows_threads(c1 + c2)[0])
    return stat_errors(emu, x, gamma, beta, G, GN_EPS, stat_rows(ns, rps, part))


def record():
    """Prints the RECORDED table of tests/test_norm_gpu.py: per case the emulator's figures rounded up to two digits, pm2 /
    scale / shift floored at 2^-24 (one fp32 rounding in the figure's own, relative, unit)."""
    print("RECORDED = {")
    for shape, regime in GN_CASES:
        err = emulator_figures(shape, regime)
        figs = [round_up2(max(err[f], FIGURE_FLOORS[f])) for f in FIGURES]
        print(f'    "{case_id(shape, regime)}": (' + ", ".join(f"{v:.1e}" for v in figs) + "),")
    print("}")


if __name__ == "__main__":                                 # python tests/norm_ref.py --record
    import sys
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/norm_ref.py --record   (prints the RECORDED table for tests/test_norm_gpu.py)")
    record()
