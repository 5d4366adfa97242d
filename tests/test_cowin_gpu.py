"""-m gpu: a flat or ring fused step has no place for a frame stride (vdx/ops.py `_cofuse_args`): a window row whose fourth entry
is not 1 is refused before any launch, and a fourth entry of 1 changes nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_a_flat_step_refuses_a_row_with_a_frame_stride(monkeypatch):
    import vdx  # noqa: F401
    from vdx import ops
    from vdx._lib import VdxError
    T, C, h, w = 4, 4, 8, 8
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    z = torch.randn(1, C, T, h, w, generator=g).half().to(dev)
    windows = torch.randn(2 * C * T * h * w, generator=g).half().to(dev)
    wn = torch.ones(1, T, dtype=torch.float32, device=dev)
    coeffs = (0.6, 0.8, 0.9, 0.4)
    want = ops.cofuse_cfg_ddim_step(z, windows, [(0, 0, T)], wn, 7.5, coeffs)
    assert torch.equal(ops.cofuse_cfg_ddim_step(z, windows, [(0, 0, T, 1)], wn, 7.5, coeffs), want)
    launched, launch = [], ops._launch
    monkeypatch.setattr(ops, "_launch", lambda symbol, *a: (launched.append(symbol), launch(symbol, *a))[1])
    for step in (ops.cofuse_cfg_ddim_step, ops.coloop_cfg_ddim_step):
        with pytest.raises(VdxError, match="frame stride"):
            step(z, windows, [(0, 0, 2, 2)], wn, 7.5, coeffs)
    assert launched == []
    assert torch.equal(ops.costride_cfg_ddim_step(z, windows, [(0, 0, T, 1)], wn, 7.5, coeffs), want) and len(launched) == 1
