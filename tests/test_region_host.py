"""CPU: regional prompts' host side (vdx/region.py, `check_regions` in vdx/options.py, the job's `--region`): the plan against the
float64 restatement of tests/region_ref.py, the launch flags against the tables, every refusal, and the records."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import vdx  # noqa: E402,F401
import region_ref as R  # noqa: E402
from vdx.options import RECORD_KEYS, JobOptions, info_options, record_options, region_record, resolve  # noqa: E402
from vdx.options import check_regions as resolve_regions  # noqa: E402
from vdx.pipeline import FLAG_OF_FIELD, DiffuserConfig, build_arg_parser, config_from_args  # noqa: E402
from vdx.region import MAX_REGIONS, RegionPlan, check_regions, record, region_plan  # noqa: E402

ULP = 2.0 ** -23                                                    # of 1.0f: the weights lie in [0, 1]


def _masks(T, h, w, seed):
    """A static soft mask, a per-frame hard one, a per-frame soft one that overlaps both, and an all-zero one."""
    g = np.random.default_rng(seed)
    H, W = 8 * h, 8 * w
    x = np.arange(W)[None, :].repeat(H, 0)
    soft = np.clip(255 - 6 * x, 0, 255).astype(np.uint8)
    hard = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        hard[t, H // 2:, (8 * t) % W:] = 255
    noise = g.integers(0, 256, size=(T, H, W)).astype(np.uint8)
    noise[:, :8, :8] = 0
    return [soft, hard, noise, np.zeros((H, W), np.uint8)]


@pytest.mark.parametrize("h,w", [(5, 9), (16, 16), (1, 1), (8, 3)])
def test_the_plan_is_the_restatement(h, w):
    """Odd grids: latent 5x9 gives 3x5, 2x3 and 1x2, the clipped edge cells the mean over the cells that exist."""
    T = 3
    masks = _masks(T, h, w, seed=h * w)
    plan = region_plan([(m, f"text {i}") for i, m in enumerate(masks)], T, h, w, 4)
    want = R.weights(masks, T, h, w, 4)
    assert isinstance(plan, RegionPlan) and plan.levels == 4 and plan.n_texts == 5 and plan.texts == tuple(f"text {i}" for i in range(4))
    assert list(plan.grids) == [R.level_grid(h, w, 1 << l) for l in range(4)]
    if (h, w) == (5, 9):
        assert list(plan.grids) == [(5, 9), (3, 5), (2, 3), (1, 2)]
    for lev, (got, ref) in enumerate(zip(plan.tables, want)):
        assert got.dtype == np.float32 and got.shape == ref.shape == (T, plan.grids[lev][0] * plan.grids[lev][1], 5)
        # float64 sums taken in another order differ by ~1e-16 relative: at most one fp32 rounding step of a weight in [0, 1]
        assert np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() <= ULP
        assert np.array_equal(got == 0, ref == 0) and np.array_equal(got == 1, ref == 1)
        assert np.abs(got.astype(np.float64).sum(axis=2) - 1.0).max() <= ULP
        assert not got[:, :, 4].any()                               # the all-zero mask has no weight anywhere
        assert np.array_equal(plan.flags[lev], (got != 0).any(axis=1))
    assert plan.flags.shape == (4, T, 5) and plan.flags.dtype == np.bool_ and not plan.flags[:, :, 4].any()


def test_one_owner_gets_exactly_one():
    """Hard masks on 64-pixel blocks: every cell of every level has one owner, weight exactly 1.0f, the others exactly 0.0f; the
    base fills what the regions leave; an overlap of two full regions halves."""
    h = w = 16
    a, b = np.zeros((128, 128), np.uint8), np.zeros((2, 128, 128), bool)
    a[:, :64] = 255
    b[1, 64:, 64:] = True                                           # bool: True is 255
    plan = region_plan([(a, "left"), (b, "corner")], 2, h, w, 4)
    for tab, (hh, ww) in zip(plan.tables, plan.grids):
        assert np.isin(tab, (0.0, 1.0)).all()
        t = tab.reshape(2, hh, ww, 3)
        assert (t[:, :, :ww // 2, 1] == 1).all() and (t[0, :, ww // 2:, 0] == 1).all()
        assert (t[1, hh // 2:, ww // 2:, 2] == 1).all() and (t[1, :hh // 2, ww // 2:, 0] == 1).all()
    assert plan.flags[:, 0].tolist() == [[True, True, False]] * 4 and plan.flags[:, 1].tolist() == [[True, True, True]] * 4
    assert plan.active(0, 0, 1) == [0, 1] and plan.active(3, 0, 2) == [0, 1, 2] and plan.active(2, 1, 2, 1, True) == [0, 1, 2]
    both = region_plan([(np.full((128, 128), 255, np.uint8), "x"), (np.full((128, 128), 255, np.uint8), "y")], 1, h, w, 2)
    assert (both.tables[1][..., 0] == 0).all() and (both.tables[1][..., 1:] == 0.5).all() and both.active(1, 0, 1) == [1, 2]
    with pytest.raises(ValueError, match="window"):
        plan.active(0, 1, 2)


def test_a_static_mask_is_the_same_mask_on_every_frame():
    T, h, w = 4, 5, 9
    m = _masks(1, h, w, seed=2)[2][0]
    a = region_plan([(m, "t")], T, h, w, 4)
    b = region_plan([(np.repeat(m[None], T, 0), "t")], T, h, w, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a.tables, b.tables)) and np.array_equal(a.flags, b.flags)
    assert all((x == x[:1]).all() for x in a.tables)


BASE = dict(num_frames=4, steps=2, chunk_size=4, overlap=0, height=64, width=64, mode="chunk", device="cpu", prompt="a forest")
OK = np.zeros((64, 64), np.uint8)


@pytest.mark.parametrize("bad,match", [
    ("mask:a", "sequence"), ([], "no region"), ([(OK,)], "pair"), ([(OK, "a", "b")], "pair"), (["ab"], "pair"), ([OK], "pair"), ([5], "pair"),
    ([(OK, None)], "string"), ([(OK, 7)], "string"), ([(OK, b"x")], "string"),
    ([(OK.astype(np.float32), "a")], "uint8 or bool"), ([(OK.astype(np.int64), "a")], "uint8 or bool"), ([(7, "a")], "array"),
    ([(OK[0], "a")], "shape"), ([(OK[None, None], "a")], "shape"),
    ([(np.zeros((64, 72), np.uint8), "a")], "64x72"), ([(np.zeros((8, 8), np.uint8), "a")], "8x8"),
    ([(np.zeros((3, 64, 64), np.uint8), "a")], "3 frames"), ([(np.zeros((1, 64, 64), np.uint8), "a")], "1 frames"),
    ([(OK, "t")] * 8, "at most 7"), ([("/nonexistent/mask.npy", "a")], "cannot be read"),
])
def test_every_refusal_comes_before_any_work(bad, match):
    cfg = DiffuserConfig(**BASE, regions=bad)
    for call in (lambda: check_regions(cfg), lambda: resolve_regions(cfg), lambda: resolve(cfg, job=True), lambda: resolve(cfg)):
        with pytest.raises(ValueError, match=match):
            call()
    assert MAX_REGIONS == 7


def test_tile_and_prompt_travel_are_refused():
    co = dict(BASE, co_denoise=True, height=128, width=128)
    mask = np.zeros((128, 128), np.uint8)
    with pytest.raises(ValueError, match="cannot be combined with tile"):
        resolve(DiffuserConfig(**co, tile=(64, 64), regions=((mask, "a"),)), job=True)
    with pytest.raises(ValueError, match="cannot be combined with tile"):
        check_regions(DiffuserConfig(**co, tile=(64, 64), regions=((mask, "a"),)))
    for call in (check_regions, lambda c: resolve(c, job=True), resolve):
        with pytest.raises(ValueError, match="cannot be combined with prompt_travel"):
            call(DiffuserConfig(**BASE, prompt_travel=((2, "b"),), regions=((OK, "a"),)))
    assert resolve(DiffuserConfig(**co, tile=(64, 64)), job=True).regions is None       # each alone stands
    assert resolve(DiffuserConfig(**BASE, prompt_travel=((2, "b"),)), job=True).regions is None


def test_record_keys_are_unchanged_and_the_record_appears_only_when_set():
    assert RECORD_KEYS == ("freeu", "tome", "co_denoise", "tile", "loop", "context_stride", "mask", "negative_prompt", "guidance_rescale")
    off = resolve(DiffuserConfig(**BASE), job=True)
    assert off == JobOptions("allgather", 1, 1, None, None, False, None, False, 1, None) and off.regions is None
    assert check_regions(DiffuserConfig(**BASE)) is None and resolve_regions(DiffuserConfig(**BASE)) is None
    assert info_options(off, None) == {} and region_record(off) == {} and region_record({"rank": 0}) == {}
    left = OK.copy()
    left[:, :16] = 255
    on = resolve(DiffuserConfig(**BASE, regions=((left, "a fox: red; close"), (OK, "a pine forest"))), job=True)
    assert isinstance(on.regions, RegionPlan) and on.regions.T == 4 and (on.regions.h, on.regions.w) == (8, 8) and on.regions.levels == 4
    rec = {"regions": {"count": 2, "texts": ["a fox: red; close", "a pine forest"], "coverage": [0.75, 0.25, 0.0]}}
    assert info_options(on, None) == rec == region_record(on) == record(on.regions) and region_record({"rank": 0, **rec}) == rec
    assert record_options({"rank": 0, **rec, "freeu": {"b1": 1.2}}) == {"freeu": {"b1": 1.2}}      # beside record_options, not inside
    assert isinstance(resolve(DiffuserConfig(**BASE, regions=((left, "x"),))).regions, RegionPlan)


def test_region_flag_parses_masks_from_files(tmp_path):
    parse = lambda argv: config_from_args(build_arg_parser().parse_args(argv))      # noqa: E731
    assert parse([]).regions is None and FLAG_OF_FIELD["regions"] == "region"
    left = OK.copy()
    left[:, :32] = 255
    moving = np.zeros((4, 64, 64), np.uint8)
    moving[2:] = 255
    np.save(tmp_path / "left.npy", left)
    np.save(tmp_path / "moving.npy", moving)
    argv = ["--num_frames", "4", "--height", "64", "--width", "64", "--prompt", "a forest"]
    cfg = parse(argv + ["--region", str(tmp_path / "left.npy"), "a fox: red; 4k, close", "--region", str(tmp_path / "moving.npy"), "--x: y;"])
    assert cfg.regions == ((str(tmp_path / "left.npy"), "a fox: red; 4k, close"), (str(tmp_path / "moving.npy"), "--x: y;"))
    plan = resolve(cfg, job=True).regions
    assert plan.texts == ("a fox: red; 4k, close", "--x: y;")
    want = R.weights([left, moving], 4, 8, 8, 4)
    assert all(np.array_equal(a, b) for a, b in zip(plan.tables, want))              # 0, 1/2 and 1: exact in any order
    with pytest.raises(ValueError, match="cannot be read"):
        resolve(parse(argv + ["--region", str(tmp_path / "none.npy"), "a"]), job=True)
    with pytest.raises(SystemExit):
        build_arg_parser().parse_args(["--region", "mask.npy"])


def test_the_restated_blend_on_the_host():
    """The restatement itself: an exact one is a select, a zero weight skips (a NaN there stays out), two halves are the fp32 mean."""
    import torch
    g = torch.Generator().manual_seed(1)
    a, b, c = (torch.randn(2, 6, generator=g).half() for _ in range(3))
    c[:] = float("nan")
    tab = np.array([[[1.0, 0.0, 0.0], [0.5, 0.5, 0.0]], [[0.0, 0.0, 1.0], [0.0, 0.25, 0.0]]], np.float32)     # (T = 2, S = 2, 3)
    out = R.blend([a, b, c], tab, 0, 1)
    assert torch.equal(out[0], a[0]) and torch.equal(out[1], (0.5 * a[1].float() + 0.5 * b[1].float()).half())
    out = R.blend([a, b, c], tab, 1, 1)
    assert bool(torch.isnan(out[0]).all()) and torch.equal(out[1], (0.25 * b[1].float()).half())
    assert torch.equal(R.blend([a, b, None], tab, 1, 1)[0], torch.zeros(6).half())
    assert R.window_frames(5, 3, 3, 1, True) == [3, 4, 0] and R.window_frames(5, 0, 3, 2) == [0, 2, 4]
