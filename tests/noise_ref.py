"""Numpy restatement, op for op, of the seeded noise generator "philox4x32-10/v1" as csrc/noise.hip computes it: the yardstick of
tests/test_noise_host.py and tests/test_noise_gpu.py.  These lines ARE the definition; it does not import the product's kernels.
Element i (the C-order linear index in the LOGICAL tensor, whatever box of it is asked for) of stream s under seed k:

    bits     Philox4x32-10 (Salmon et al., SC'11): key = (k lo, k hi), counter = (q lo, q hi, s lo, s hi), q = i >> 2; the block's
             four words x0..x3 serve the elements 4q..4q + 3
    normals  Box-Muller in float64 on (x0, x1) -> elements 4q, 4q + 1 and on (x2, x3) -> elements 4q + 2, 4q + 3:
             u = (xa + 0.5) 2^-32,  r = sqrt(-2 ln u),  the angle (xb + 0.5) 2^-32 of a turn,  (r cos, r sin)
    ln       u = m 2^e by the float64's own exponent bits, m in [1/2, 1); m < sqrt(1/2): m = 2m, e = e - 1;
             t = (m - 1) / (m + 1),  z = t t,  p = Horner over 1/3, 1/5, ..., 1/23 in z,  ln m = 2t + 2t (z p),
             ln u = e LN2 + ln m
    sin/cos  octant o = xb >> 29, j = xb & (2^29 - 1); odd octants reflect IN INTEGERS, j = 2^29 - 1 - j;
             theta = ((j + 0.5) 2^-29) (pi/4), in (0, pi/4);  z = theta theta;
             s = theta + (theta z) Horner(-1/3!, 1/5!, ..., 1/17!),  c = 1 + z Horner(-1/2!, 1/4!, ..., -1/18!);
             octants 1, 2, 5, 6 swap s and c; the cosine is negative in octants 2..5, the sine in 4..7
    output   fp32: fp32(n).  fp16: fp16(fp32(fp16(n)) fp32(sigma)), what `base *= sigma` gives a torch fp16 tensor

Every + - * / sqrt is one IEEE float64 operation rounded on its own (numpy never fuses a product into a sum); the kernel is built
without contraction to do the same.
"""
import math

import numpy as np

GENERATOR = "philox4x32-10/v1"
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SEEDS = (0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF)
STREAMS = (0, 1, 2 ** 32)

LN2 = math.log(2.0)
SQRT_HALF = math.sqrt(0.5)
PI_4 = math.pi / 4
LN_COEF = tuple(1.0 / (2 * k + 1) for k in range(1, 12))                                        # 1/3 .. 1/23
SIN_COEF = tuple((-1.0) ** k / math.factorial(2 * k + 1) for k in range(1, 9))                  # -1/3! .. 1/17!
COS_COEF = tuple((-1.0) ** k / math.factorial(2 * k) for k in range(1, 10))                     # -1/2! .. -1/18!


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> the block's four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) for x in ctr]
    k0, k1 = int(key[0]), int(key[1])
    for rnd in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def _horner(z, coef):
    p = np.full_like(z, coef[-1])
    for a in coef[-2::-1]:
        p = p * z + a
    return p


def ln_unit(u):
    """ln u of float64 u in (0, 1], normal numbers: the stated sequence."""
    u = np.asarray(u, dtype=np.float64)
    bits = u.view(np.uint64)
    e = (bits >> np.uint64(52)).astype(np.int64) - 1022
    m = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FE0000000000000)).view(np.float64)
    low = m < SQRT_HALF
    m = np.where(low, m * 2.0, m)
    e = np.where(low, e - 1, e)
    t = (m - 1.0) / (m + 1.0)
    z = t * t
    t2 = t * 2.0
    lnm = t2 + t2 * (z * _horner(z, LN_COEF))
    return e.astype(np.float64) * LN2 + lnm


def sincos_octant(theta):
    """(sin, cos) of float64 theta in [0, pi/4]: the stated polynomials."""
    theta = np.asarray(theta, dtype=np.float64)
    z = theta * theta
    s = theta + (theta * z) * _horner(z, SIN_COEF)
    c = 1.0 + z * _horner(z, COS_COEF)
    return s, c


def cos_sin_turn(x):
    """(cos, sin) of the angle (x + 0.5) 2^-32 of a turn, x uint32: octant in integers, then `sincos_octant`."""
    x = np.asarray(x, dtype=np.uint32)
    o = (x >> np.uint32(29)).astype(np.int64)
    j = (x & np.uint32(0x1FFFFFFF)).astype(np.int64)
    j = np.where(o & 1, 0x1FFFFFFF - j, j)
    theta = ((j.astype(np.float64) + 0.5) * 2.0 ** -29) * PI_4
    s, c = sincos_octant(theta)
    swap = ((o + 1) >> 1) & 1
    cc, ss = np.where(swap, s, c), np.where(swap, c, s)
    cc = np.where(((o + 2) >> 2) & 1, -cc, cc)
    ss = np.where(o >= 4, -ss, ss)
    return cc, ss


def box_muller(xa, xb):
    """The pair (r cos, r sin) of two uint32 words, float64."""
    u = (np.asarray(xa, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32
    r = np.sqrt(-2.0 * ln_unit(u))
    c, s = cos_sin_turn(xb)
    return r * c, r * s


def normal_at(idx, seed: int, stream: int = 0):
    """float64 normals of the logical linear indices `idx` (any integer array, values < 2^63)."""
    idx = np.asarray(idx, dtype=np.uint64)
    q = idx >> np.uint64(2)
    lane = (idx & np.uint64(3)).astype(np.int64)
    x = philox4x32_10((q & MASK32, q >> np.uint64(32), np.uint64(stream & 0xFFFFFFFF), np.uint64(stream >> 32)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    hi = lane >= 2
    n0, n1 = box_muller(np.where(hi, x[2], x[0]), np.where(hi, x[3], x[1]))
    return np.where(lane & 1, n1, n0)


def box_indices(shape, box=None):
    """The logical linear indices of `box` = (start, extent) in the C-order tensor `shape` (None: the whole), as a uint64 array of
    the box's shape."""
    shape = tuple(int(v) for v in shape)
    start, extent = ((0,) * len(shape), shape) if box is None else box
    idx = np.zeros((1,) * len(shape), dtype=np.uint64)
    stride = 1
    for d in range(len(shape) - 1, -1, -1):
        view = [1] * len(shape)
        view[d] = extent[d]
        idx = idx + ((np.arange(extent[d], dtype=np.uint64) + np.uint64(start[d])) * np.uint64(stride)).reshape(view)
        stride *= shape[d]
    return idx


def normal64(shape, seed: int, stream: int = 0, box=None):
    return normal_at(box_indices(shape, box), seed, stream)


def to_f32(n64):
    return np.asarray(n64).astype(np.float32)


def to_f16(n64, sigma: float = 1.0):
    """fp16(fp32(fp16(n)) fp32(sigma))."""
    with np.errstate(all="ignore"):
        return (np.asarray(n64).astype(np.float16).astype(np.float32) * np.float32(sigma)).astype(np.float16)


def normal(shape, seed: int, stream: int = 0, box=None, sigma: float = 1.0, dtype=np.float16):
    n = normal64(shape, seed, stream, box)
    return to_f16(n, sigma) if dtype == np.float16 else to_f32(n)
