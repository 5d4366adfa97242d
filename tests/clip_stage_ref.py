"""References and input builders for the device stages of the CLIP score (csrc/clip.hip), shared by tests/test_clip_score_gpu.py,
tests/test_clip_stages_host.py and tests/test_clip_stages_gpu.py: Pillow and torch-CPU for the front end (bit for bit), float64
numpy statements of the embedding + pre-LayerNorm and of the cosine score, and the bounds measured against them on the MI355X
(profiles/clip_stage_parity.txt).  Everything here is deterministic and runs on the CPU; the embedding and score cases are built once, shared and read-only."""
import functools

import numpy as np
import torch

MEAN = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)


# ---- the front end ---------------------------------------------------------------------------------------------------------
def frames_like_video(F, H, W, seed):
    """Smooth colour fields + noise: natural-image-like statistics, every frame different."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = []
    for f in range(F):
        a, b, c = g.uniform(0, 6.3, 3)
        base = np.stack([np.sin(3 * xx + a + 0.2 * f), np.cos(4 * yy + b), np.sin(2 * (xx + yy) + c)], -1)
        img = 127.5 + 90 * base + g.normal(0, 20, (H, W, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return np.stack(out)


def pil_resize(frames):
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(f).resize((224, 224), Image.BILINEAR)) for f in frames])


def pixels_of_u8(u8):
    """ToTensor + Normalize(ImageNet) of resized uint8 (F, 224, 224, 3) on torch-CPU: fp32 (F, 3, 224, 224)."""
    return (torch.from_numpy(u8).permute(0, 3, 1, 2).float() / 255 - MEAN) / STD


def reference_pixels(frames):
    """The reference's transform (scoring.py:81-85) on torch-CPU: fp32 (F, 3, 224, 224)."""
    return pixels_of_u8(pil_resize(frames))


def unfold_patches(px):
    """(F, 3, 224, 224) -> the patch-GEMM rows [F*49][3072]: row f*49 + py*7 + px, column c*1024 + ky*32 + kx."""
    F = px.shape[0]
    return px.view(F, 3, 7, 32, 7, 32).permute(0, 2, 4, 1, 3, 5).reshape(F * 49, 3072)


# H -> (ksize, band, span) that `ops.clip_preprocess` must choose: the 8 -> 4 -> 2 -> 1 halving against 64 KiB of LDS at 672
# bytes per row.  2400, 4320 and 10753 fill 65 184 bytes, the most that fits; 11000 needs 66 528 with one output row: refused.
BAND_TABLE = {1: (3, 8, 1), 2: (3, 8, 2), 3: (3, 8, 2), 7: (3, 8, 2), 223: (3, 8, 9), 224: (3, 8, 9), 225: (5, 8, 9),
              576: (7, 8, 24), 2160: (21, 8, 87), 2400: (23, 8, 97), 2464: (23, 4, 55), 4320: (41, 4, 97), 5000: (47, 2, 67),
              8000: (73, 1, 72), 10753: (99, 1, 97)}
REFUSED_H = 11000                       # (ksize 101, band 1, span 99)
FULL_LDS_H = (2400, 4320, 10753)        # span = 97: the kernel's `nr` equals `a.span` in the widest band
HEIGHT_SIZES = [(H, 8 if i % 2 == 0 else 12) for i, H in enumerate(BAND_TABLE)]
# Pillow resizes a frame with H > 100 W vertically first (PIL/Image.py `resize`), and so does `ops.clip_preprocess`, through
# vdx_resample_v_u8: the kernel then sees 224 rows.  The narrowest frames that reach the kernel at their own height:
BAND_SIZES = [(H, max(W, -(-H // 100))) for H, W in HEIGHT_SIZES]
REFUSED_SIZE = (REFUSED_H, 110)
FULL_LDS_SIZES = [(4320, 8), (10753, 8), (4320, 44), (10753, 108)]
WIDTH_SIZES = [(8, W) for W in (1, 2, 3, 223, 225, 2400, 7680)]          # kx from 3 to 71
MIXED_SIZES = [(3, 4000), (4000, 3), (1, 1)]
CONTENT_KINDS = ("video", "zeros", "white", "impulses", "checker", "row_ramp", "col_ramp", "random")


def content(kind, H, W, seed=0):
    """uint8 (F, H, W, 3) of one content kind; F = 2 except "impulses": one white pixel per frame, at each corner and the centre."""
    if kind == "video":
        return frames_like_video(2, H, W, seed)
    if kind == "zeros":
        return np.zeros((2, H, W, 3), np.uint8)
    if kind == "white":
        return np.full((2, H, W, 3), 255, np.uint8)
    if kind == "impulses":
        out = np.zeros((5, H, W, 3), np.uint8)
        for f, (y, x) in enumerate([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]):
            out[f, y, x] = 255
        return out
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "checker":
        one = ((yy + xx) % 2 * 255).astype(np.uint8)
        return np.stack([one, 255 - one])[..., None].repeat(3, -1)
    if kind == "row_ramp":                       # a shifted or dropped window row changes the bytes
        return np.stack([yy % 256, (yy * 7 + 3) % 256]).astype(np.uint8)[..., None].repeat(3, -1)
    if kind == "col_ramp":
        return np.stack([xx % 256, (xx * 7 + 3) % 256]).astype(np.uint8)[..., None].repeat(3, -1)
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    raise KeyError(kind)


def choose_band(y_bounds, band0, lds_max, span_of):
    """The band `ops.clip_preprocess` must arrive at: halve from `band0` while the widest band's rows overflow `lds_max`."""
    band = band0
    while band > 1 and span_of(y_bounds, band) * 672 > lds_max:
        band //= 2
    return band, span_of(y_bounds, band)


def band_windows_fit(y_bounds, band, span):
    """What the kernel's silent guards assume, for every band: the band's input rows [first window's start, last window's end)
    number at most `span`, and every output row's window lies inside them (so `nr` is never cut and no tap is dropped)."""
    yb = np.asarray(y_bounds, np.int64)
    for oy0 in range(0, len(yb), band):
        rows = yb[oy0:oy0 + band]
        iy0, end = rows[0, 0], rows[-1].sum()
        if end - iy0 > span or (rows[:, 0] < iy0).any() or (rows.sum(1) > end).any():
            return False
    return True


# ---- embedding + pre-LayerNorm ---------------------------------------------------------------------------------------------
EMBED_D = (1, 63, 64, 65, 100, 768, 1024)
EMBED_P = (1, 49, 50)
EMBED_F = (1, 3, 5)
EMBED_REGIMES = ("gauss", "large_mean", "constant", "outlier", "gamma0", "extreme")
EMBED_EPS = 1e-5
# worst |got - ref| - (2^-11 |ref| + 2^-25) per regime over every shape above, MI355X against the float64 statement
# (profiles/clip_stage_parity.txt); never below 0.  The test allows 4x this, capped at 2^-10 max|ref|.
EMBED_MEASURED_EXCESS = {"gauss": 2.691e-8, "large_mean": 2.262e-4, "constant": 0.0, "outlier": 0.0, "gamma0": 0.0, "extreme": 1.468e-6}


def _h(a):
    return np.asarray(a, np.float64).astype(np.float16)


@functools.lru_cache(maxsize=None)
def _embed_case(regime, D, P):
    F = max(EMBED_F)
    g = np.random.default_rng([EMBED_REGIMES.index(regime), D, P])
    patch, cls, pos = g.normal(0, 1, (F * P, D)), g.normal(0, 1, D), g.normal(0, 0.5, (P + 1, D))
    gamma, beta = g.normal(1, 0.2, D), g.normal(0, 0.5, D)
    if regime == "large_mean":                   # mean 100, std 0.1: v - mean cancels seven of fp32's bits
        patch, cls, pos = patch * 0.1, cls * 0.1, np.full((P + 1, D), 100.0)
    elif regime == "constant":                   # variance 0: the output is beta, eps alone decides rstd
        patch, cls, pos = np.repeat(patch[:, :1], D, 1), np.repeat(cls[:1], D), np.repeat(pos[:, :1], D, 1)
    elif regime == "outlier":                    # one 60000 among zeros, in another column in each row
        patch, cls, pos = np.zeros((F * P, D)), np.zeros(D), np.zeros((P + 1, D))
        patch[np.arange(F * P), (np.arange(F * P) * 7 + 3) % D] = 60000.0
        cls[D // 2] = 60000.0
    elif regime == "gamma0":
        gamma = np.zeros(D)
    elif regime == "extreme":                    # |normalised| <= 17 keeps 2048 |n| + 30000 inside fp16 (checked on the CPU)
        gamma = np.array([2048.0, -2048.0, 2.0 ** -24, 2.0 ** -14])[np.arange(D) % 4]
        beta = np.array([30000.0, -30000.0, 0.0, 2.0 ** -24, -(2.0 ** -14)])[np.arange(D) % 5]
    case = {"patch": _h(patch), "cls": _h(cls), "pos": _h(pos), "gamma": _h(gamma), "beta": _h(beta)}
    for v in case.values():
        v.setflags(write=False)
    return case


def embed_case(regime, D, P):
    """fp16 inputs of max(EMBED_F) frames (read-only, shared): patch [F*P][D], cls [D], pos [P+1][D], gamma [D], beta [D]."""
    return _embed_case(regime, D, P)


def embed_ref(case, F, eps=EMBED_EPS):
    """float64 [F][P+1][D] of the same fp16 values: row 0 = class + pos[0], row t = patch t-1 + pos[t]; LayerNorm; gamma, beta.
    eps is the fp32 value the entry point receives.  (Rows past P of the device output are zero.)"""
    c = {k: v.astype(np.float64) for k, v in case.items()}
    P, D = c["pos"].shape[0] - 1, c["pos"].shape[1]
    x = np.empty((F, P + 1, D))
    x[:, 0] = c["cls"] + c["pos"][0]
    x[:, 1:] = c["patch"][:F * P].reshape(F, P, D) + c["pos"][1:]
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + float(np.float32(eps))) * c["gamma"] + c["beta"]


def embed_excess(got, ref):
    """Worst |got - ref| beyond one fp16 rounding of ref (2^-11 |ref| + 2^-25): what the fp32 evaluation has to answer for."""
    return float((np.abs(got - ref) - (2.0 ** -11 * np.abs(ref) + 2.0 ** -25)).max())


def embed_bound(regime, ref):
    return min(4 * EMBED_MEASURED_EXCESS[regime], 2.0 ** -10 * float(np.abs(ref).max()))


# ---- the score ---------------------------------------------------------------------------------------------------------------
COSINE_F = (1, 3, 4, 5, 8, 257)
COSINE_D = (1, 63, 64, 65, 512, 768, 1000)
COSINE_REGIMES = ("gauss", "max", "subnormal", "alternating")
# worst |got - ref64| of per_frame and of mean, per (regime, D) over every F above, MI355X (profiles/clip_stage_parity.txt).
# The test allows 4x this, capped at D * 2^-23: a sequential fp32 sum's worst case for a cosine of magnitude at most 1.
_COSINE_ROWS = {"gauss": (9.934e-9, 3.574e-8, 3.629e-8, 4.208e-8, 1.611e-8, 1.182e-8, 1.097e-8),
                "max": (2.384e-8, 2.384e-8, 2.384e-8, 2.384e-8, 2.384e-8, 5.960e-8, 1.192e-7),
                "subnormal": (2.384e-8, 2.384e-8, 2.384e-8, 2.384e-8, 1.192e-7, 2.384e-8, 1.192e-7),
                "alternating": (0.0, 7.871e-8, 7.442e-8, 9.629e-8, 7.402e-8, 7.507e-8, 6.865e-8)}
COSINE_MEASURED = {(r, D): v for r in COSINE_REGIMES for D, v in zip(COSINE_D, _COSINE_ROWS[r])}


@functools.lru_cache(maxsize=None)
def _cosine_case(regime, D):
    F = max(COSINE_F)
    g = np.random.default_rng([100 + COSINE_REGIMES.index(regime), D])
    img, txt = g.normal(0, 1, (F, D)), g.normal(0, 1, D)
    sign = np.where(np.arange(F) % 3 == 2, -1.0, 1.0)[:, None]
    if regime == "max":                          # xx = D * 65504^2 reaches 4e12: finite in fp32
        img, txt = sign * np.full((F, D), 65504.0), np.full(D, 65504.0)
    elif regime == "subnormal":                  # the smallest fp16 subnormal: the norms (2^-24 sqrt(D)) stay above 1e-12
        img, txt = sign * np.full((F, D), 2.0 ** -24), np.full(D, 2.0 ** -24)
    elif regime == "alternating":                # the dot product is a near-cancelled sum of terms of magnitude 1
        img = np.where(np.arange(D) % 2 == 0, 1.0, -1.0) * (1 + 0.01 * img)
        txt = 1 + 0.01 * txt
    case = (_h(img), _h(txt))
    for v in case:
        v.setflags(write=False)
    return case


def cosine_case(regime, D):
    """fp16 (img [max(COSINE_F)][D], txt [D]), read-only and shared."""
    return _cosine_case(regime, D)


def cosine_ref(img, txt):
    """float64 F.normalize(img[f]) . F.normalize(txt) of the same fp16 values -> (per_frame [F], mean)."""
    x, t = img.astype(np.float64), txt.astype(np.float64)
    per = (x @ t) / (np.maximum(np.sqrt((x * x).sum(1)), 1e-12) * max(np.sqrt((t * t).sum()), 1e-12))
    return per, float(per.mean())


def cosine_bound(regime, D):
    return min(4 * COSINE_MEASURED[(regime, D)], D * 2.0 ** -23)


def mean_of_per_frame_f32(per):
    """The device's `mean` restated: the fp32 sum of the returned per_frame in frame order, divided by float32(F)."""
    s = np.float32(0)
    for v in np.asarray(per, np.float32):
        s = np.float32(s + v)
    return np.float32(s / np.float32(len(per)))
