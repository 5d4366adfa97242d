"""CPU: a job's options (vdx/options.py).  The refusals, their texts and their order are those recorded from the commit before
the checks moved (tests/golden/job_options_parent.json, made by tests/golden/make_job_options.py); the records' option keys keep
their order; a job validates once and builds each plan once."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")) if p not in sys.path]

import vdx  # noqa: E402,F401
import make_job_options as G  # noqa: E402
from vdx.options import RECORD_KEYS, RULES, JobOptions, record_options, resolve, world_size  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "job_options_parent.json")) as f:
    RECORDED = json.load(f)


def test_the_fixture_holds_the_cases_it_was_asked_for():
    entries = RECORDED["entries"]
    assert len(entries) == len(G.configs()) and [[e["cfg"], e["exchange"]] for e in entries] == G.configs()
    assert len(G.TWO_RULES) >= 20
    kinds = {(type(e["run_job"]).__name__, type(e["call"]).__name__) for e in entries}
    assert kinds == {("str", "dict"), ("list", "list"), ("list", "dict"), ("str", "list")}     # accepted and refused, by either


def test_every_recorded_config_is_refused_or_accepted_as_on_the_parent_commit():
    """Strings are compared as strings: the same exception type and the same message, byte for byte, from both entry points;
    an accepted call returns an `info` with the same keys."""
    wrong = []
    with G.no_device():
        for e in RECORDED["entries"]:
            job, call = G.outcomes(e["cfg"], e["exchange"])
            for name, got in (("run_job", job), ("call", call)):
                if got != e[name]:
                    wrong.append((e["cfg"], e["exchange"], name, got, e[name]))
    assert not wrong, f"{len(wrong)} of {len(RECORDED['entries'])} differ, the first: {wrong[0]}"


def test_the_rule_table_names_every_shared_refusal_once():
    assert list(RULES) == ["co_denoise", "tile", "loop", "context_stride"]
    assert [[w for w, _ in RULES[o]] for o in RULES] == [
        ["needs allgather"], ["needs co_denoise", "needs allgather", "guidance_rescale"],
        ["needs co_denoise", "needs allgather", "tile", "guidance_rescale"],
        ["needs co_denoise", "needs allgather", "tile", "loop", "guidance_rescale"]]
    texts = [m for rows in RULES.values() for _, m in rows]
    assert len(set(texts)) == len(texts) == 13
    assert RULES["loop"][2][1] == "loop and tile exclude each other: the tiled kernels have no ring form yet"


def test_the_checks_are_importable_from_their_old_modules_and_are_the_same_functions():
    from vdx import codenoise, options, pipeline
    for mod, names in ((pipeline, ("check_free_init", "check_freeu", "check_guidance_rescale", "check_tome")),
                       (codenoise, ("check_co_denoise", "check_tile", "check_loop", "check_stride", "MIN_TILE_CELLS"))):
        for name in names:
            assert getattr(mod, name) is getattr(options, name)


def test_world_size_reads_the_environment_only_when_asked(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "4")
    assert world_size() == 1 and world_size(env=True) == 4                              # no group is initialised here
    monkeypatch.delenv("WORLD_SIZE")
    assert world_size() == 1 and world_size(env=True) == 1


def test_resolve_returns_plain_values():
    from vdx.codenoise import StridePlan
    from vdx.pipeline import DiffuserConfig
    base = dict(num_frames=8, steps=2, chunk_size=6, overlap=2, height=64, width=64, mode="chunk", device="cpu")
    off = resolve(DiffuserConfig(**base), job=True)
    assert isinstance(off, JobOptions) and off == JobOptions("allgather", 1, 1, None, None, False, None, False, 1, None)
    on = resolve(DiffuserConfig(**base, co_denoise=True, context_stride=2, freeu=(1.2, 1.4, 0.9, 0.2), tome=0.5, interpolate=2,
                                negative_prompt="blurry"), "allgather", 2, job=True)
    assert (on.world, on.co_denoise, on.context_stride, on.interpolate) == (2, True, 2, 2)
    assert isinstance(on.stride_plan, StridePlan) and on.stride_plan.world == 2 and on.stride_plan.levels == 2
    assert on.freeu == dict(b1=1.2, b2=1.4, s1=0.9, s2=0.2) and on.tome["ratio"] == 0.5
    assert on.guidance == {"negative_prompt": "blurry"} and on.guidance_rescale == 0.0
    tiled = resolve(DiffuserConfig(**base, co_denoise=True, tile=(64, 64), guidance_scale=7.5))
    assert tiled.tile == (8, 8, 2, 2) and tiled.stride_plan is None and tiled.pixel_mask is None
    phi = resolve(DiffuserConfig(**base, guidance_rescale=0.5, negative_prompt="x"), job=True)
    assert list(phi.guidance.items()) == [("negative_prompt", "x"), ("guidance_rescale", 0.5)]
    with pytest.raises(Exception):                                                      # frozen
        off.loop = True


# ---- the records' option keys -------------------------------------------------------------------------------------------------
ALL = {"freeu": {"b1": 1.2}, "tome": {"ratio": 0.5}, "co_denoise": {"windows": 2}, "tile": {"grid": [1, 2]}, "loop": {"windows": [[0, 6]]},
       "context_stride": {"levels": 2}, "mask": {"rule": "nearest"}, "negative_prompt": "blurry", "guidance_rescale": 0.7}
# (res, its option keys in order, what the parent commit's `if "x" in res:` ladder wrote for {"clip_score": 0.5} + those keys)
RECORDS = [
    ({"rank": 0, "world_size": 1}, [], '{"clip_score": 0.5}'),
    ({"guidance_rescale": 0.7, "rank": 0, "loop": {"windows": [[0, 6]]}, "freeu": {"b1": 1.2}, "free_init": {"iters": 2}},
     ["freeu", "loop", "guidance_rescale"], '{"clip_score": 0.5, "freeu": {"b1": 1.2}, "loop": {"windows": [[0, 6]]}, "guidance_rescale": 0.7}'),
    ({"negative_prompt": "blurry", "mask": {"rule": "nearest"}, "co_denoise": {"windows": 2}, "tome": {"ratio": 0.5}, "interpolate": 1},
     ["tome", "co_denoise", "mask", "negative_prompt"],
     '{"clip_score": 0.5, "tome": {"ratio": 0.5}, "co_denoise": {"windows": 2}, "mask": {"rule": "nearest"}, "negative_prompt": "blurry"}'),
    (dict(reversed(list({"rank": 0, **ALL}.items()))), list(RECORD_KEYS),
     '{"clip_score": 0.5, "freeu": {"b1": 1.2}, "tome": {"ratio": 0.5}, "co_denoise": {"windows": 2}, "tile": {"grid": [1, 2]}, '
     '"loop": {"windows": [[0, 6]]}, "context_stride": {"levels": 2}, "mask": {"rule": "nearest"}, "negative_prompt": "blurry", '
     '"guidance_rescale": 0.7}'),
]


@pytest.mark.parametrize("res,keys,parent_json", RECORDS)
def test_record_options_picks_the_keys_in_the_records_order(res, keys, parent_json):
    assert RECORD_KEYS == ("freeu", "tome", "co_denoise", "tile", "loop", "context_stride", "mask", "negative_prompt", "guidance_rescale")
    before = dict(res)
    picked = record_options(res)
    assert list(picked) == keys and all(picked[k] is res[k] for k in keys) and res == before     # pure: `res` is left alone
    assert json.dumps({**{"clip_score": 0.5}, **picked}) == parent_json


# ---- a job validates once -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,plan,parent", [("loop", "loop_plan", 3), ("context_stride", "stride_plan", 3)])
def test_a_job_builds_its_plan_once_to_validate_and_once_to_run(option, plan, parent):
    """On the parent commit a job built its ring plan 3 times (`run_job`'s `check_loop`, the call's `check_loop`, the call's
    `plan()`) and its strided plan 3 times (`run_job`'s `check_stride`, the call's `check_stride`, the call's `stride_plan_of`):
    counted there with this same counter (`plan_builds` of tests/golden/make_job_options.py, recorded in the fixture).  Now: once
    in `resolve`; the ring plan once more through `d.plan()`, the strided plan never again (the call takes `opts.stride_plan`)."""
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    kw, exchange = G.PLAN_JOBS[option]
    assert RECORDED["plan_builds"][option][plan] == parent
    seen = {}

    def job():
        cfg = DiffuserConfig(**kw)
        opts = resolve(cfg, exchange, 1, job=True)
        d = DistributedVideoDiffuser(cfg, G._Unet(), DDIMScheduler(), None, None)
        _, seen["info"] = d(exchange, options=opts)

    with G.no_device():
        n = G.plan_builds(kw, exchange, job)
    assert n[plan] == (2 if option == "loop" else 1) and n[plan] < parent and sum(n.values()) == n[plan]
    assert option in seen["info"] and "co_denoise" in seen["info"]
    with G.no_device():                                                                 # without `options=` the call resolves itself
        cfg = DiffuserConfig(**kw)
        d = DistributedVideoDiffuser(cfg, G._Unet(), DDIMScheduler(), None, None)
        n = G.plan_builds(kw, exchange, lambda: d(exchange))
        assert n[plan] == (2 if option == "loop" else 1)
        assert not any(hasattr(d, name) for name in ("_tiles", "_stride", "_co_rec"))    # per-call state is the call's
