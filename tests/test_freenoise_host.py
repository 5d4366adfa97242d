"""CPU: FreeNoise's host side (vdx/freenoise.py) against the restatement of tests/freenoise_ref.py, and the job option's check."""
import dataclasses
import os
import sys
from collections import Counter

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

import vdx  # noqa: E402,F401
import freenoise_ref as R  # noqa: E402
from vdx import freenoise  # noqa: E402
from vdx.options import check_free_noise, resolve  # noqa: E402
from vdx.pipeline import DiffuserConfig  # noqa: E402

SHAPES = [(7, 3, 2), (17, 16, 4), (33, 16, 4), (40, 32, 8), (65, 5, 5), (128, 16, 4), (9, 4, 2), (128, 2, 1)]


@pytest.mark.parametrize("F,L,S", SHAPES)
@pytest.mark.parametrize("weighting", ["pyramid", "flat"])
def test_windows_and_weights_match_the_restatement(F, L, S, weighting):
    starts = freenoise.window_starts(F, L, S)
    assert starts == R.window_starts(F, L, S) and starts[0] == 0 and starts[-1] == F - L and len(set(starts)) == len(starts)
    wn = freenoise.window_weights(F, L, S, weighting)
    assert wn.dtype == torch.float32 and torch.equal(wn, R.window_weights(F, L, S, weighting))
    total, cover = torch.zeros(F, dtype=torch.float64), torch.zeros(F, dtype=torch.int64)
    for i, s in enumerate(starts):
        total[s:s + L] += wn[i].double()
        cover[s:s + L] += 1
    assert float((total - 1).abs().max()) <= cover.max() * 2.0 ** -24          # each share is within half an fp32 ulp of its value
    single = [wn[i, t - s] for i, s in enumerate(starts) for t in range(s, s + L) if cover[t] == 1]
    assert all(float(w) == 1.0 for w in single)


@pytest.mark.parametrize("T,L,S", [(12, 4, 2), (64, 16, 4), (33, 16, 4), (23, 5, 5), (7, 3, 2), (3, 4, 2)])
def test_reschedule_index_is_the_restatement_and_repeats_the_first_window(T, L, S):
    idx = freenoise.reschedule_index(T, L, S, 7)
    assert idx == R.reschedule_index(T, L, S, 7) == freenoise.reschedule_index(T, L, S, 7)
    assert idx[:L] == list(range(min(T, L))) and all(0 <= v < L for v in idx)
    other, found = R.reschedule_index(T, L, S, 8), R.reschedule_index(T, L, S, 7)
    for i in range(L, T, S):               # a whole block is a permutation of its source block, a cut one a part of it
        took, source = Counter(found[i:i + S]), Counter(found[i - L:i - L + S])
        assert took == source if i + S <= T else not took - source
    assert T < L + 8 or S == 1 or other != found                              # the seed moves it


ON = dict(free_noise=(16, 4))
REFUSALS = [
    (dict(free_noise=(1, 1)), "context_length 1 outside"), (dict(free_noise=(33, 4)), "context_length 33 outside"),
    (dict(free_noise=(16, 0)), "context_stride 0 outside"), (dict(free_noise=(16, 17)), "context_stride 17 outside"),
    (dict(free_noise=(16.0, 4)), "must be an integer"), (dict(free_noise=(16,)), "two integers"), (dict(free_noise_weighting="flat"), "needs free_noise"),
    (dict(ON, free_noise_weighting="cone"), "weighting must be one of"), (dict(ON, mode="chunk", chunk_size=16), "nothing to window"),
    (dict(ON, num_frames=200), "exceeds the 128"), (dict(ON, init_video="clip.npy"), "init_video"), (dict(ON, keep_frames="0:4"), "keep_frames"),
    (dict(ON, mask="m.npy"), "mask"), (dict(ON, free_init_iters=2), "free_init_iters"), (dict(ON, co_denoise=True), "co_denoise"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[t for _, t in REFUSALS])
def test_check_free_noise_refuses_before_any_model_loads(kw, text):
    cfg = DiffuserConfig(**{"num_frames": 64, "mode": "fsdp", **kw})
    with pytest.raises(ValueError, match=text):
        check_free_noise(cfg, "allgather", 1)


def test_accepted_record_and_the_default_job():
    cfg = DiffuserConfig(num_frames=64, mode="fsdp", free_noise=(16, 4), free_noise_weighting="flat")
    want = {"context_length": 16, "context_stride": 4, "weighting": "flat", "windows": 13}
    assert check_free_noise(cfg, "halo", 2) == want and resolve(cfg, "allgather", 1).free_noise == want
    assert resolve(DiffuserConfig(), "allgather", 1).free_noise is None
    on = dataclasses.asdict(resolve(cfg, "allgather", 1))
    off = dataclasses.asdict(resolve(DiffuserConfig(num_frames=64, mode="fsdp"), "allgather", 1))
    assert off["free_noise"] is None and {**on, "free_noise": None} == off                                # nothing else moves
