"""LPIPS-AlexNet between consecutive frames on libvdx_hip.so: the distance behind the validator's video-quality term

    InferNet/template/validator/scoring.py:163      self.lpips_model = lpips.LPIPS(net='alex')
    InferNet/template/validator/scoring.py:171-175  Resize((224, 224)) + ToTensor + Normalize(ImageNet)
    InferNet/template/validator/scoring.py:269-309  compute_video_quality: lpips_model(frame_i, frame_i-1) per pair

The `lpips` package (and torchvision) is not installed where this was written and nothing can be fetched, so LPIPS is
restated from its published definition (R. Zhang et al., "The Unreasonable Effectiveness of Deep Features as a Perceptual
Metric", CVPR 2018; version 0.1 with the `lin` layers): parity with the package is NOT pinned by any fixture ("parity
unpinned").  The yardstick of the tests is an fp32 torch-CPU restatement of the same definition (tests/lpips_ref.py).

What it computes, step by step (the same as the reference unless stated):
  * frames: a decoded uint8 RGB clip in any form vdx/frames.py takes.  DEVIATION: the reference re-reads the mp4 with
    OpenCV (:272-281); here the frames the pipeline decoded are scored directly, as in vdx/clip_score.py;
  * Resize((224, 224)): Pillow's antialiased bilinear resize, bit for bit (`ops.resize_u8(..., "bilinear")`), then
    ((u / 255) - mean) / std in fp32 with the ImageNet statistics (:171-175);
  * that already-normalised tensor goes straight into LPIPS with normalize=False (:288), whose ScalingLayer applies
    (x - shift) / scale with shift (-.030, -.088, -.188), scale (.458, .448, .450) on top of it — the reference's choice
    (LPIPS expects [-1, 1] inputs), kept.  Both affine maps are evaluated in fp32 in this order and rounded to fp16 once
    (`stem_lut`: 3 x 256 values); the pixels then enter the network in fp16;
  * AlexNet features: conv 3->64 k11 s4 p2 (55x55), ReLU (tap 1), maxpool 3/2 (27x27), conv 64->192 k5 p2, ReLU (tap 2),
    maxpool 3/2 (13x13), conv 192->384 k3 p1 + ReLU (tap 3), conv 384->256 k3 p1 + ReLU (tap 4), conv 256->256 k3 p1 + ReLU
    (tap 5).  conv1 = `ops.lpips_stem` + GEMM, conv2 = `ops.im2col` + GEMM, conv3..5 = the GEMM's implicit 3x3 mode; fp16
    activations, fp32 accumulation;
  * per tap and pixel n = x / (sqrt(sum_c x^2) + 1e-10); per pair (f, f+1) sum_c lin_c (n_f - n_f+1)^2, the mean over
    pixels, the sum over the five taps (`ops.lpips_distance`: fp32, a fixed reduction order).  Dropout in the `lin` layers
    is the identity in eval mode; the `lin` weights are non-negative 1x1 convolutions without bias;
  DEVIATION: features are computed once per frame; the reference runs the network on both frames of every pair, i.e. on
  every inner frame twice (:283-291).  The numbers are the same.
  DEVIATION: the reference turns every exception into a score of 0.0 (:307-309); here errors raise `VdxError`.

Weights come from a local file in the `lpips` state-dict layout (`from_local`) or from a seeded generator (`synthetic`);
nothing is downloaded.  The key map is RECALLED from the package's source, not checked against it ("recalled, unpinned"):
    net.slice{1..5}.{0,3,6,8,10}.{weight,bias}    the five AlexNet convolutions (torchvision `features` indices)
    lin{0..4}.model.1.weight  [1, C, 1, 1]        the 1x1 `lin` layers (index 0 of `model` is the Dropout)
    scaling_layer.{shift,scale}  [1, 3, 1, 1]
`lins.{0..4}.model.1.weight` (the same tensors under the ModuleList a full `state_dict()` also lists) are accepted and
ignored; any other key, and any missing one, raises `VdxError`.
"""
from __future__ import annotations

import os
from typing import Dict, List

import torch

from . import frames as _frames, ops, packing
from ._lib import VdxError

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)            # scoring.py:174
LPIPS_SHIFT, LPIPS_SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)             # lpips.ScalingLayer
# (slice, torchvision features index, Cin, Cout, kernel, stride, padding)
ALEX_CONVS = ((1, 0, 3, 64, 11, 4, 2), (2, 3, 64, 192, 5, 1, 2), (3, 6, 192, 384, 3, 1, 1), (4, 8, 384, 256, 3, 1, 1),
              (5, 10, 256, 256, 3, 1, 1))
TAP_SIZES = (55, 27, 13, 13, 13)                                                        # tap images are square


def conv_key(i: int) -> str:
    s, idx = ALEX_CONVS[i][:2]
    return f"net.slice{s}.{idx}"


def expected_shapes() -> Dict[str, tuple]:
    """Every key of the recalled `lpips` layout -> its shape."""
    want = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for i, (_s, _idx, ci, co, k, _st, _p) in enumerate(ALEX_CONVS):
        want[conv_key(i) + ".weight"] = (co, ci, k, k)
        want[conv_key(i) + ".bias"] = (co,)
        want[f"lin{i}.model.1.weight"] = (1, co, 1, 1)
    return want


def synthetic_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded fp32 weights in the recalled layout: He-scaled convolutions (std sqrt(2 / fan_in)), small biases
    (0.05 N(0, 1)), lin ~ U(0, 0.2), the package's scaling constants.  Shared with tests/lpips_ref.py."""
    g = torch.Generator().manual_seed(seed)
    sd = {"scaling_layer.shift": torch.tensor(LPIPS_SHIFT).view(1, 3, 1, 1),
          "scaling_layer.scale": torch.tensor(LPIPS_SCALE).view(1, 3, 1, 1)}
    for i, (_s, _idx, ci, co, k, _st, _p) in enumerate(ALEX_CONVS):
        sd[conv_key(i) + ".weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[conv_key(i) + ".bias"] = 0.05 * torch.randn(co, generator=g)
        sd[f"lin{i}.model.1.weight"] = 0.2 * torch.rand(1, co, 1, 1, generator=g)
    return sd


def check_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The recalled layout, exactly: -> {key: fp32 tensor} for the expected keys; extras, gaps and wrong shapes raise."""
    want = expected_shapes()
    alias = {f"lins.{i}.model.1.weight" for i in range(5)}
    for k in sd:
        if k not in want and k not in alias:
            raise VdxError(f"LPIPSAlex: unexpected key in the lpips state dict: {k}")
    out = {}
    for k, shape in want.items():
        if k not in sd:
            raise VdxError(f"LPIPSAlex: missing key in the lpips state dict: {k}")
        if tuple(sd[k].shape) != shape:
            raise VdxError(f"LPIPSAlex: {k} has shape {tuple(sd[k].shape)}, expected {shape}")
        out[k] = sd[k].detach().float()
    for i in range(5):
        if bool((out[f"lin{i}.model.1.weight"] < 0).any()):
            raise VdxError(f"LPIPSAlex: lin{i} has negative weights (LPIPS' lin layers are non-negative)")
    return out


def stem_lut(shift: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp16 [3][256]: channel c of uint8 value u as conv1 sees it, ((u / 255 - mean_c) / std_c - shift_c) / scale_c with every
    step an fp32 torch-CPU op (ToTensor + Normalize, then LPIPS' ScalingLayer), rounded to fp16 once."""
    u = torch.arange(256, dtype=torch.float32).view(1, 256)
    x = (u / 255 - torch.tensor(IMAGENET_MEAN).view(3, 1)) / torch.tensor(IMAGENET_STD).view(3, 1)
    x = (x - shift.float().view(3, 1)) / scale.float().view(3, 1)
    return x.half().contiguous()


class LPIPSAlex:
    """`lpips.LPIPS(net='alex')` over consecutive frames (scoring.py:269-309) on the HIP path; see the module docstring."""

    def __init__(self):
        self.w: List[torch.Tensor] = []          # GEMM weights of the five convolutions, fp16
        self.b: List[torch.Tensor] = []          # their biases, fp16
        self.lin: List[torch.Tensor] = []        # fp32 [C] per tap
        self.lut = None                          # fp16 [3][256]
        self.synthetic_weights = False
        self.device = torch.device("cpu")

    # ---- construction ------------------------------------------------------------------------
    @torch.no_grad()
    def load_lpips_state_dict(self, sd: Dict[str, torch.Tensor], device="cuda") -> "LPIPSAlex":
        dev = torch.device(device)
        sd = check_state_dict(sd)
        self.w, self.b, self.lin = [], [], []
        for i, (_s, _idx, _ci, co, k, _st, _p) in enumerate(ALEX_CONVS):
            w = sd[conv_key(i) + ".weight"].half()
            if k == 3:
                w = packing.pack_conv3x3(w)                                       # the GEMM's implicit 3x3 mode
            else:
                w = w.permute(0, 2, 3, 1).reshape(co, -1)                         # K = (ky*k + kx)*Cin + c: stem / im2col rows
                w = torch.nn.functional.pad(w, (0, packing.round_up(w.shape[1], 64) - w.shape[1]))
            self.w.append(w.contiguous().to(dev))
            self.b.append(sd[conv_key(i) + ".bias"].half().contiguous().to(dev))
            self.lin.append(sd[f"lin{i}.model.1.weight"].reshape(co).contiguous().to(dev))
        self.lut = stem_lut(sd["scaling_layer.shift"], sd["scaling_layer.scale"]).to(dev)
        self.device = dev
        return self

    @classmethod
    def from_local(cls, path: str, device="cuda") -> "LPIPSAlex":
        """A local file (torch.save of the state dict, or .safetensors) in the recalled `lpips` layout.  Only a file that
        exists is read; nothing is fetched."""
        if not os.path.isfile(path):
            raise VdxError(f"LPIPSAlex.from_local: {path!r} is not a file (weights are read from disk only)")
        from .compat.diffusers_shim import _load_file
        sd = _load_file([path])
        if sd is None:
            raise VdxError(f"LPIPSAlex.from_local: could not read a state dict from {path}")
        return cls().load_lpips_state_dict(sd, device=device)

    @classmethod
    def synthetic(cls, seed: int = 0, device="cuda") -> "LPIPSAlex":
        """`synthetic_state_dict(seed)`: the distance of a run without a checkpoint.  `synthetic_weights` is then True."""
        s = cls().load_lpips_state_dict(synthetic_state_dict(seed), device=device)
        s.synthetic_weights = True
        return s

    # ---- features and distance ---------------------------------------------------------------
    @torch.no_grad()
    def features(self, frames) -> List[torch.Tensor]:
        """uint8 RGB frames (F, H, W, 3) -> the five ReLU taps as fp16 rows [F*S*S][C], S = 55, 27, 13, 13, 13."""
        if not self.w:
            raise VdxError("LPIPSAlex: no weights loaded")
        F = _frames.check(frames, "LPIPSAlex")[0]
        if F == 0:
            raise VdxError("LPIPSAlex.features: no frames")
        t = _frames.on_device(frames, self.device)
        u8 = ops.resize_u8(t, ops.CLIP_IMAGE, ops.CLIP_IMAGE, "bilinear")
        c1 = ops.gemm(ops.lpips_stem(u8, self.lut), self.w[0], M=F * 55 * 55, bias=self.b[0])
        p1 = ops.relu_maxpool(c1, n_img=F, H=55, W=55)                            # c1 is tap 1 from here on
        c2 = ops.gemm(ops.im2col(p1, n_img=F, H=27, W=27, k=5, pad=2), self.w[1], M=F * 27 * 27, bias=self.b[1])
        x = ops.relu_maxpool(c2, n_img=F, H=27, W=27)
        taps = [c1, c2]
        for i in (2, 3, 4):
            x = ops.gemm(x, self.w[i], M=F * 169, mode=ops.CONV3X3, conv=(F, 13, 13, 13, 13, 1, 0), bias=self.b[i])
            taps.append(ops.relu(x, out=x))
        return taps

    @torch.no_grad()
    def distances_device(self, frames) -> torch.Tensor:
        """-> fp32 [F-1] on the device: LPIPS(frame f, frame f+1)."""
        taps = self.features(frames)
        F = taps[0].shape[0] // (55 * 55)
        if F < 2:
            raise VdxError("LPIPSAlex: a distance needs two frames")
        out = None
        for x, lin, s in zip(taps, self.lin, TAP_SIZES):
            out = ops.lpips_distance(x, lin, F=F, HW=s * s, out=out)
        return out

    def __call__(self, frames) -> torch.Tensor:
        """uint8 RGB frames (F, H, W, 3) -> per-pair distances fp32 [F-1] on the host (empty for F < 2: no pairs, :295-297)."""
        if len(frames) < 2:
            return torch.empty(0, dtype=torch.float32)
        return self.distances_device(frames).cpu()
