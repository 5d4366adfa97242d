"""-m gpu: with token merging off, the default path is the one it was before token merging existed.  The tiny golden forwards
and the tiny denoising job of tests/test_unet_gpu.py run on a model that never had `enable_tome` called and on one that had it
enabled, used and disabled again; both must (1) launch exactly the entry-point sequence recorded on the commit before token
merging (tests/golden/tome_default_launches.json, tools/tome_record_default.py), with no vdx_tome_* symbol in it, (2) give the
output bytes recorded there, and (3) stay within the existing bounds of the oracle's stored results."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tome_default_path as D  # noqa: E402

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def used_and_disabled(gpu):
    """A model that ran a forward with token merging at every level, then had it disabled."""
    m = D.tiny_model(gpu).enable_tome(0.5, seed=1, max_downsample=8)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 4, 2, 16, 32, generator=g).half().to(gpu)
    e = torch.randn(2, 77, D.TINY["cross"], generator=g).half().to(gpu)
    _, seen = D.record(lambda: m(x, 5, encoder_hidden_states=e).sample)
    assert any(s.startswith("vdx_tome_") for s in seen) and m._tome_tables
    m.disable_tome()
    assert m.tome is None and not m._tome_tables
    return m


@pytest.mark.parametrize("state", ["never enabled", "enabled then disabled"])
@pytest.mark.parametrize("name", D.WORKLOADS)
def test_default_path_is_the_parents(gpu, name, state):
    want = json.load(open(D.FIXTURE))["workloads"][name]
    m = D.tiny_model(gpu) if state == "never enabled" else used_and_disabled(gpu)
    out, seen = D.run(name, m, gpu)
    assert not [s for s in seen if s.startswith("vdx_tome_")]
    assert len(seen) == want["launches"] and D.pack(seen) == want["sequence"]
    assert D.sha(out) == want["sha256"]
    gold = np.load(os.path.join(D.GOLD, name + ".npz"))
    if name == "denoise_tiny":                      # tests/test_unet_gpu.py::test_denoise_blend_matches_golden's bound
        err, bound = rel_l2(out, torch.from_numpy(gold["lat"])), 2e-2
    else:                                           # tests/test_unet_gpu.py::test_unet_tiny_matches_golden's bound
        err, bound = rel_l2(out.float(), torch.from_numpy(gold["out"])), 2.0 * float(gold["floor"])
    print(f"{name}, {state}: {len(seen)} launches, rel-L2 {err:.3e} from the stored oracle result (bound {bound:.3e})")
    assert err <= bound
