"""CPU: prompt travel's host side (vdx/travel.py, `check_prompt_travel` in vdx/options.py, the job's `--prompt_at`): the plan against
the restatement of tests/travel_ref.py and against hand-written rows, every refusal, and the records."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import vdx  # noqa: E402,F401
import travel_ref as R  # noqa: E402
from vdx.options import RECORD_KEYS, JobOptions, check_prompt_travel, info_options, record_options, resolve, travel_record  # noqa: E402
from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args  # noqa: E402
from vdx.travel import MAX_KEYS, TravelPlan, keys_of, travel_plan  # noqa: E402


def _keysets(T):
    sets = [[0], [0, T - 1], [5], [3, 4, 20]]
    kept = [sorted(set(k)) for k in sets if all(0 <= f < T for f in k)]
    return [k for i, k in enumerate(kept) if k not in kept[:i]]          # T = 1: {0, T - 1} is {0}


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("T", [1, 2, 24])
def test_the_plan_is_the_restatement(T, loop):
    seen = 0
    for frames in _keysets(T):
        p = travel_plan([(f, f"text {f}") for f in reversed(frames)], T, loop=loop)      # any order: the plan sorts
        lo, hi, w = R.plan(frames, T, loop)
        assert isinstance(p, TravelPlan) and p.frames == tuple(frames) and p.T == T
        assert p.lo.dtype == p.hi.dtype == np.int32 and p.w.dtype == np.float32
        assert np.array_equal(p.lo, lo) and np.array_equal(p.hi, hi) and np.array_equal(p.w.view(np.int32), w.view(np.int32))
        assert all(p.w[f] == 0 and p.lo[f] == p.hi[f] == i for i, f in enumerate(frames))   # a key frame is the key: exactly 0
        assert np.all((p.w >= 0) & (p.w < 1)) and np.all(p.w[p.lo == p.hi] == 0)
        assert np.all((0 <= p.lo) & (p.lo < len(frames)) & (0 <= p.hi) & (p.hi < len(frames)))
        seen += 1
    assert seen == {1: 1, 2: 2, 24: 4}[T]


def test_hand_written_rows():
    p = travel_plan([(3, "a"), (4, "b"), (20, "c")], 24)
    assert list(p.lo[:5]) == [0, 0, 0, 0, 1] and list(p.hi[:5]) == [0, 0, 0, 0, 1] and not p.w[:5].any()    # before the first key: it holds
    assert list(p.lo[5:20]) == [1] * 15 and list(p.hi[5:20]) == [2] * 15
    assert p.w[12] == np.float32(8 / 16) and p.w[5] == np.float32(np.float64(1) / np.float64(16))
    assert list(p.lo[20:]) == [2] * 4 and list(p.hi[20:]) == [2] * 4 and not p.w[20:].any()                    # the hold after the last key
    ring = travel_plan([(0, "a"), (20, "c")], 24, loop=True)
    assert list(ring.lo[21:]) == [1, 1, 1] and list(ring.hi[21:]) == [0, 0, 0]                                # back towards key 0 at frame T
    assert [float(x) for x in ring.w[21:]] == [float(np.float32(k / 4)) for k in (1, 2, 3)] and ring.w[0] == 0 and ring.w[20] == 0
    flat = travel_plan([(0, "a"), (20, "c")], 24)
    assert not flat.w[20:].any() and list(flat.hi[20:]) == [1] * 4
    off = travel_plan([(3, "a"), (4, "b"), (20, "c")], 24, loop=True)      # no key at 0: the wrap runs from 20 over the seam to 3 + 24
    assert off.w[0] == np.float32(np.float64(4) / np.float64(7)) and (off.lo[0], off.hi[0]) == (2, 0) and off.w[3] == 0
    one = travel_plan([(5, "only")], 24, loop=True)
    assert not one.w.any() and not one.lo.any() and not one.hi.any()        # one key: a constant prompt
    assert travel_plan([(0, "x")], 1).w.tolist() == [0.0]


BASE = dict(num_frames=8, steps=2, chunk_size=6, overlap=2, height=64, width=64, mode="chunk", device="cpu", prompt="a forest")


@pytest.mark.parametrize("bad,match", [
    ("0:a", "sequence"), ([], "no keys"), ([(1,)], "pair"), ([(1, "a", "b")], "pair"), (["ab"], "pair"), ([5], "pair"),
    ([(8, "a")], "outside"), ([(-1, "a")], "outside"), ([(1.0, "a")], "integer"), ([(True, "a")], "integer"), ([("1", "a")], "integer"),
    ([(1, "a"), (1, "b")], "twice"), ([(1, None)], "string"), ([(1, 7)], "string"), ([(1, b"x")], "string"),
    ([(i % 8, "t") for i in range(65)], "64"),
])
def test_every_refusal_comes_before_any_work(bad, match):
    cfg = DiffuserConfig(**BASE, prompt_travel=bad)
    for call in (lambda: check_prompt_travel(cfg), lambda: resolve(cfg, job=True), lambda: resolve(cfg)):
        with pytest.raises(ValueError, match=match):
            call()
    assert MAX_KEYS == 64


def test_the_prompt_is_the_key_at_frame_zero_unless_a_key_names_it():
    assert check_prompt_travel(DiffuserConfig(**BASE)) is None
    cfg = DiffuserConfig(**BASE, prompt_travel=((7, "a desert"), (3, "a shore")))
    assert check_prompt_travel(cfg) == ((0, "a forest"), (3, "a shore"), (7, "a desert")) == keys_of(cfg)
    cfg = DiffuserConfig(**BASE, prompt_travel=[[7, "a desert"], [0, "a swamp"]])
    assert check_prompt_travel(cfg) == ((0, "a swamp"), (7, "a desert"))
    assert check_prompt_travel(DiffuserConfig(**BASE, prompt_travel=((0, "a forest"),))) == ((0, "a forest"),)     # one key is valid
    with pytest.raises(ValueError, match="64"):                          # 64 keys away from frame 0 and the prompt make 65
        check_prompt_travel(DiffuserConfig(**{**BASE, "num_frames": 80}, prompt_travel=[(i + 1, "t") for i in range(64)]))


def test_record_keys_are_unchanged_and_the_record_appears_only_when_set():
    assert RECORD_KEYS == ("freeu", "tome", "co_denoise", "tile", "loop", "context_stride", "mask", "negative_prompt", "guidance_rescale")
    off = resolve(DiffuserConfig(**BASE), job=True)
    assert off == JobOptions("allgather", 1, 1, None, None, False, None, False, 1, None) and off.prompt_travel is None
    assert info_options(off, None) == {} and travel_record(off) == {} and travel_record({"rank": 0}) == {}
    on = resolve(DiffuserConfig(**BASE, prompt_travel=((7, "a desert: dusk; wide"),)), job=True)
    rec = {"prompt_travel": {"keys": [[0, "a forest"], [7, "a desert: dusk; wide"]]}}
    assert on.prompt_travel == ((0, "a forest"), (7, "a desert: dusk; wide"))
    assert info_options(on, None) == rec == travel_record(on) and travel_record({"rank": 0, **rec}) == rec
    assert record_options({"rank": 0, **rec, "freeu": {"b1": 1.2}}) == {"freeu": {"b1": 1.2}}      # beside record_options, not inside
    assert resolve(DiffuserConfig(**BASE, prompt_travel=((7, "x"),))).prompt_travel == ((0, "a forest"), (7, "x"))


def test_prompt_at_parses_texts_with_colons_and_semicolons():
    parse = lambda argv: config_from_args(build_arg_parser().parse_args(argv))      # noqa: E731
    assert parse([]).prompt_travel is None
    cfg = parse(["--num_frames", "24", "--prompt_at", "23", "a desert: dusk; 4k, wide", "--prompt", "a forest", "--prompt_at", "12", "--x: y;"])
    assert cfg.prompt_travel == ((23, "a desert: dusk; 4k, wide"), (12, "--x: y;"))
    assert check_prompt_travel(cfg) == ((0, "a forest"), (12, "--x: y;"), (23, "a desert: dusk; 4k, wide"))
    with pytest.raises(ValueError, match="integer"):
        check_prompt_travel(parse(["--prompt_at", "soon", "a desert"]))
    with pytest.raises(ValueError, match="outside"):
        check_prompt_travel(parse(["--num_frames", "8", "--prompt_at", "8", "a desert"]))
    with pytest.raises(SystemExit):
        build_arg_parser().parse_args(["--prompt_at", "3"])


def test_the_restated_blend_on_the_host():
    """The restatement itself: a key frame is the key's bits, the midpoint of two keys is their fp32 mean rounded once."""
    import torch
    g = torch.Generator().manual_seed(1)
    keys, uncond = torch.randn(2, 5, 3, generator=g).half(), torch.randn(5, 3, generator=g).half()
    lo, hi, w = R.plan([0, 2], 3)
    out = R.text_travel(keys, uncond, lo, hi, w, 0, 3)
    assert torch.equal(out[0], uncond.expand(3, 5, 3)) and torch.equal(out[1, 0], keys[0]) and torch.equal(out[1, 2], keys[1])
    assert torch.equal(out[1, 1], (0.5 * keys[0].float() + 0.5 * keys[1].float()).half())
