"""The seeded noise generator "philox4x32-10/v1" without a GPU: the numpy restatement itself (tests/noise_ref.py: the published
Philox known-answer vectors, its ln / sin / cos against numpy's, the distribution and the independence of streams and seeds at the
headline latent's size), and the host side of the option: `check_seed`, `options.check_noise`'s refusals, the flags, the records
and the op's refusals, which raise before any device is touched.

The distribution bounds are conditions, not measurements: 4 standard errors for the mean, the variance and a correlation, and the
Kolmogorov-Smirnov statistic D sqrt(N) <= 1.95 (P(K > 1.95) = 1e-3 for one case of a true normal sample)."""
import math

import numpy as np
import pytest
import torch

import noise_ref as R

import vdx  # noqa: F401
from vdx import noise, options
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args

N = 1 * 4 * 24 * 72 * 128                                              # 884 736: the headline latent
SHAPE = (1, 4, 24, 72, 128)
# measured over 2 000 000 arguments against numpy's 80-bit ln / sin / cos (profiles/noise_parity.txt): 1.56, 0.72 and 1.12 ulp; the
# bounds are the next half ulp above.  Where numpy has no wider type the yardstick is its own fp64 function, itself within an ulp
ULP_BOUND = {"ln": 2.0, "sin": 1.0, "cos": 1.5}
WIDE = np.finfo(np.longdouble).nmant >= 63


def test_known_answer_vectors():
    def words(ctr, key):
        return " ".join(f"{int(v):08x}" for v in R.philox4x32_10(ctr, key))
    assert words((0, 0, 0, 0), (0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays and scalars agree, and a counter's high word and a stream's high word are live
    q = np.array([0, 1, 2 ** 32], dtype=np.uint64)
    a = R.philox4x32_10((q & R.MASK32, q >> np.uint64(32), np.uint64(0), np.uint64(0)), (0, 0))
    assert [int(v[0]) for v in a] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert len({tuple(int(v[k]) for v in a) for k in range(3)}) == 3


def _ulp(got, want):
    """max |got - want| in ulps of fp64 at `want` (`want` in the widest type numpy has)."""
    wide = np.longdouble if WIDE else np.float64
    return float((np.abs(got.astype(wide) - want) / np.spacing(np.abs(want).astype(np.float64)).astype(wide)).max())


@pytest.fixture(scope="module")
def words():
    rng = np.random.default_rng(20261021)
    x = rng.integers(0, 2 ** 32, size=1_200_000, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0, 1, 2, 2 ** 32 - 1, 2 ** 32 - 2, 2 ** 31, 2 ** 31 - 1, 2 ** 29, 2 ** 29 - 1, 0xB504F333, 0xB504F334], dtype=np.uint32)
    return np.concatenate([x, edge])


def test_ln_sin_cos_against_numpy(words):
    wide = np.longdouble if WIDE else np.float64
    slack = 0.0 if WIDE else 1.0
    u = (words.astype(np.float64) + 0.5) * 2.0 ** -32
    e_ln = _ulp(R.ln_unit(u), np.log(u.astype(wide)))
    j = (words & np.uint32(0x1FFFFFFF)).astype(np.float64)
    theta = ((j + 0.5) * 2.0 ** -29) * R.PI_4
    s, c = R.sincos_octant(theta)
    e_sin, e_cos = _ulp(s, np.sin(theta.astype(wide))), _ulp(c, np.cos(theta.astype(wide)))
    print(f"ln {e_ln:.3f} ulp, sin {e_sin:.3f} ulp, cos {e_cos:.3f} ulp over {words.size} arguments (wide={WIDE})")
    assert e_ln <= ULP_BOUND["ln"] + slack and e_sin <= ULP_BOUND["sin"] + slack and e_cos <= ULP_BOUND["cos"] + slack
    # the whole turn: every octant's swap and signs, against numpy at the same angle (an absolute error: the angle itself is rounded)
    co, si = R.cos_sin_turn(words)
    ang = (words.astype(np.float64) + 0.5) * 2.0 ** -32 * (2 * math.pi)
    assert np.abs(co - np.cos(ang)).max() < 2e-15 and np.abs(si - np.sin(ang)).max() < 2e-15
    assert np.abs(co * co + si * si - 1.0).max() < 1e-15 and (co != 0).all() and (si != 0).all()


def test_extremes_fit_fp16():
    """|n| <= 6.77: the smallest u is 2^-33; the largest u still gives a radius above zero."""
    r_max = math.sqrt(-2.0 * float(R.ln_unit(np.array([0.5 * 2.0 ** -32]))[0]))
    r_min = math.sqrt(-2.0 * float(R.ln_unit(np.array([(2.0 ** 32 - 0.5) * 2.0 ** -32]))[0]))
    assert 6.76 < r_max <= 6.77 and 0 < r_min < 2e-5
    n0, n1 = R.box_muller(np.array([0, 0, 2 ** 32 - 1], dtype=np.uint32), np.array([0, 2 ** 31, 5], dtype=np.uint32))
    assert np.isfinite(R.to_f16(n0).astype(np.float64)).all() and abs(float(n0[0])) <= 6.77 and abs(float(n0[1])) <= 6.77


def _phi(x):
    return 0.5 * (1.0 + torch.erf(torch.from_numpy(x) / math.sqrt(2.0))).numpy()


def _moments(x):
    n = x.size
    x = np.sort(x.astype(np.float64))
    cdf = _phi(x)
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    return abs(float(x.mean())) * math.sqrt(n), abs(float(x.var()) - 1.0) * math.sqrt(n / 2), d * math.sqrt(n)


@pytest.fixture(scope="module")
def samples():
    return {(seed, stream): R.normal_at(np.arange(N, dtype=np.uint64), seed, stream) for seed in R.SEEDS for stream in R.STREAMS}


@pytest.mark.parametrize("rounded", [False, True], ids=["fp64", "fp16"])
@pytest.mark.parametrize("stream", R.STREAMS)
@pytest.mark.parametrize("seed", R.SEEDS, ids=hex)
def test_distribution(samples, seed, stream, rounded):
    x = samples[(seed, stream)]
    if rounded:
        x = R.to_f16(x).astype(np.float64)
    mean, var, ks = _moments(x)
    print(f"seed {seed:#x} stream {stream:#x} {'fp16' if rounded else 'fp64'}: |mean| sqrt N {mean:.2f}, |var - 1| sqrt(N/2) {var:.2f}, D sqrt N {ks:.2f}")
    assert mean <= 4 and var <= 4 and ks <= 1.95


def _corr(a, b):
    return abs(float(np.corrcoef(a, b)[0, 1])) * math.sqrt(a.size)


def test_correlations(samples):
    lag = max(_corr(x[:-1], x[1:]) for x in samples.values())
    streams = max(_corr(samples[(k, a)], samples[(k, b)]) for k in R.SEEDS for a in R.STREAMS for b in R.STREAMS if a < b)
    seeds = max(_corr(samples[(a, s)], samples[(b, s)]) for s in R.STREAMS for a in R.SEEDS for b in R.SEEDS if a < b)
    print(f"|corr| sqrt N: lag-1 {lag:.2f}, across streams {streams:.2f}, across seeds {seeds:.2f}")
    assert lag <= 4 and streams <= 4 and seeds <= 4


def test_a_box_is_the_slice_of_the_whole():
    whole = R.normal((2, 3, 5, 7), 7, 3, dtype=np.float32)
    box = ((1, 0, 2, 3), (1, 2, 3, 4))
    assert np.array_equal(R.normal((2, 3, 5, 7), 7, 3, box=box, dtype=np.float32).view(np.uint32), whole[1:2, 0:2, 2:5, 3:7].view(np.uint32))
    half = torch.from_numpy(R.normal((3, 5), 1, dtype=np.float16))
    for sigma in (1.0, 0.5, 14.6146):
        want = half.clone()
        want *= sigma
        assert torch.equal(torch.from_numpy(R.normal((3, 5), 1, sigma=sigma)).view(torch.int16), want.view(torch.int16))


# ---- the option's host side -------------------------------------------------------------------------------------------------------
def test_streams_and_check_seed():
    assert (noise.STREAM_BASE, noise.STREAM_POSTERIOR, noise.STREAM_SAMPLER, noise.STREAM_ITERATION_MAX) == (0, 2 ** 32, 2 ** 33, 2 ** 32 - 1)
    assert noise.GENERATOR == R.GENERATOR == "philox4x32-10/v1" and noise.GENERATORS == ("torch", "philox")
    assert [noise.stream_of_iteration(k) for k in (1, 2, 2 ** 32 - 1)] == [1, 2, 2 ** 32 - 1]
    for bad in (0, 2 ** 32, -1, 1.0, True):
        with pytest.raises(ValueError):
            noise.stream_of_iteration(bad)
    assert [noise.check_seed(s) for s in R.SEEDS] == list(R.SEEDS)
    for bad in (-1, 2 ** 64, 1.5, "7", None, True):
        with pytest.raises(ValueError, match="seed"):
            noise.check_seed(bad)
    assert noise.generator_of(DiffuserConfig()) is None and noise.generator_of(DiffuserConfig(noise="philox")) == 0
    assert noise.generator_of(DiffuserConfig(noise="philox", seed=2 ** 64 - 1)) == 2 ** 64 - 1
    assert noise.normal((2,), "cpu", torch_draw=lambda: "torch's") == "torch's"


def test_check_noise():
    assert options.check_noise(DiffuserConfig()) is None
    assert options.check_noise(DiffuserConfig(noise="philox")) == {"generator": "philox4x32-10/v1", "seed": 0}
    assert options.check_noise(DiffuserConfig(noise="philox", seed=5, noise_device="cuda")) == {"generator": "philox4x32-10/v1", "seed": 5}
    assert options.check_noise(DiffuserConfig(noise="philox", seed=5, device="cuda:0", noise_device="cuda"))["seed"] == 5
    for kw, msg in ((dict(seed=5), "needs noise"), (dict(noise="torch", seed=0), "needs noise"), (dict(noise="mt"), "one of"),
                    (dict(noise="philox", seed=-1), "2\\^64"), (dict(noise="philox", seed=2 ** 64), "2\\^64"),
                    (dict(noise="philox", seed=1.0), "integer"), (dict(noise="philox", seed=True), "integer"),
                    (dict(noise="philox", noise_device="cpu"), "no host form"),
                    (dict(noise="philox", device="cuda:0", noise_device="cuda:1"), "no host form"),
                    (dict(noise="philox", noise_device="no such device"), "no device")):
        with pytest.raises(ValueError, match=msg):
            options.check_noise(DiffuserConfig(**kw))
    # both entries of `resolve` run it, before anything loads
    for job in (False, True):
        with pytest.raises(ValueError, match="needs noise"):
            options.resolve(DiffuserConfig(seed=5), job=job)
        on = options.resolve(DiffuserConfig(noise="philox", seed=5), job=job)
        off = options.resolve(DiffuserConfig(), job=job)
        assert on.noise == {"generator": "philox4x32-10/v1", "seed": 5} and off.noise is None
        assert options.noise_record(on) == {"noise": on.noise} and options.noise_record(off) == {}
        assert options.info_options(on, [])["noise"] == on.noise and "noise" not in options.info_options(off, [])
    assert options.noise_record({"noise": {"seed": 1}, "x": 2}) == {"noise": {"seed": 1}} and options.noise_record({"x": 2}) == {}
    assert "noise" not in options.RECORD_KEYS and "seed" not in options.RECORD_KEYS


def test_flags():
    p = build_arg_parser()
    off = config_from_args(p.parse_args([]))
    assert (off.seed, off.noise) == (None, "torch") and off == DiffuserConfig()
    assert (lambda c: (c.seed, c.noise))(config_from_args(p.parse_args(["--seed", "18446744073709551615"]))) == (2 ** 64 - 1, "philox")
    assert (lambda c: (c.seed, c.noise))(config_from_args(p.parse_args(["--noise", "philox"]))) == (None, "philox")
    assert (lambda c: (c.seed, c.noise))(config_from_args(p.parse_args(["--noise", "torch"]))) == (None, "torch")
    with pytest.raises(ValueError, match="needs noise"):
        options.check_noise(config_from_args(p.parse_args(["--noise", "torch", "--seed", "3"])))
    with pytest.raises(ValueError, match="2\\^64"):
        options.check_noise(config_from_args(p.parse_args(["--seed", "-3"])))
    with pytest.raises(SystemExit):
        p.parse_args(["--seed", "1.5"])


def test_the_op_refuses_on_the_host():
    """Every refusal is raised before a device is touched: none of these needs a GPU."""
    from vdx import ops
    from vdx._lib import VdxError
    ok = dict(shape=(1, 4, 2, 8, 8), seed=1, device="cuda")
    for kw in (dict(shape=()), dict(shape=(1,) * 6), dict(shape=(1, 0, 2)), dict(shape=(2 ** 32, 2 ** 31)), dict(shape=(2.0, 3)),
               dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.0), dict(stream=-1), dict(stream=2 ** 64),
               dict(box=((0, 0, 0, 0, 0), (1, 4, 2, 8, 9))), dict(box=((0, 0, 0, 0, 1), (1, 4, 2, 8, 8))), dict(box=((0, 0, 0, 0, 0), (1, 4, 2, 8, 0))),
               dict(box=((0, 0, 0, 0, -1), (1, 4, 2, 8, 1))), dict(box=((0, 0, 0, 0), (1, 4, 2, 8))), dict(box=(0, 1)),
               dict(sigma=float("inf")), dict(sigma=float("nan")), dict(sigma=1e39), dict(sigma="1"), dict(dtype=torch.float64),
               dict(dtype=torch.float32, sigma=2.0)):
        with pytest.raises(ValueError):
            ops.philox_normal(**{**ok, **kw})
    with pytest.raises(VdxError, match="no host form"):
        ops.philox_normal(**{**ok, "device": "cpu"})
    from vdx.miner import seeded_latent
    for kw in (dict(shape=(4, 2, 8, 8)), dict(shape=(2, 4, 2, 8, 8))):
        with pytest.raises(VdxError):
            seeded_latent(1, device="cuda", **kw)
    for frames in ((0, 3), (1, 1), (-1, 1), (0,), (0.0, 1)):
        with pytest.raises(ValueError):
            seeded_latent(1, (1, 4, 2, 8, 8), "cuda", frames=frames)


def test_the_library_checks_again_and_names_the_form():
    """`vdx_noise_form` runs the library's own checks and plan on the host: which boxes take the fast form, and a refusal (-1) for
    what the Python checks would have stopped."""
    import ctypes as C

    from vdx import _lib, ops
    assert ops.philox_form((1, 3, 3, 5, 7)) and ops.philox_form((1, 4, 24, 72, 128)) and ops.philox_form((315,))
    assert ops.philox_form((1, 4, 24, 72, 128), ((0, 0, 3, 0, 0), (1, 4, 16, 72, 128)))          # a frame range: rows of 16 * 72 * 128
    assert ops.philox_form((1, 4, 6, 8, 8), ((0, 1, 2, 4, 4), (1, 3, 3, 4, 4)))                  # 4-aligned rows
    assert not ops.philox_form((1, 3, 3, 5, 7), ((0, 0, 0, 0, 0), (1, 3, 3, 5, 4)))              # a row pitch of 7
    assert not ops.philox_form((1, 4, 6, 8, 8), ((0, 0, 0, 0, 1), (1, 4, 6, 8, 4)))              # starts inside a block
    assert ops.philox_form((1, 1, 1, 3, 2 ** 33 + 9), ((0, 0, 0, 0, 2 ** 32 - 8), (1, 1, 1, 1, 16)))
    lib = _lib.load()
    arr = C.c_size_t * 2
    for shape, start, extent in (((4, 8), (0, 1), (4, 8)), ((4, 8), (0, 0), (4, 0)), ((0, 8), (0, 0), (1, 1)), ((2 ** 32, 2 ** 31), (0, 0), (1, 1))):
        assert lib.vdx_noise_form(2, arr(*shape), arr(*start), arr(*extent)) == -1
    assert lib.vdx_noise_form(0, arr(1, 1), arr(0, 0), arr(1, 1)) == -1 and lib.vdx_noise_form(6, arr(1, 1), arr(0, 0), arr(1, 1)) == -1
    for sym in ("vdx_noise_f16", "vdx_noise_f32"):                          # sigma and the output pointer, before any launch
        args = [1, 0, 2, arr(4, 8), arr(0, 0), arr(4, 8)] + ([C.c_float(float("inf"))] if sym.endswith("f16") else [])
        if sym.endswith("f16"):
            assert getattr(lib, sym)(*args, None, None) == -1 and b"finite" in lib.vdx_last_error()
        bad = [1, 0, 2, arr(4, 8), arr(0, 0), arr(4, 9)] + ([C.c_float(1.0)] if sym.endswith("f16") else [])
        assert getattr(lib, sym)(*bad, None, None) == -1 and b"leaves the shape" in lib.vdx_last_error()
        null = [1, 0, 2, arr(4, 8), arr(0, 0), arr(4, 8)] + ([C.c_float(1.0)] if sym.endswith("f16") else [])
        assert getattr(lib, sym)(*null, None, None) == -1 and b"aligned" in lib.vdx_last_error()
