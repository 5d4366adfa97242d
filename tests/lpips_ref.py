"""fp32 CPU restatement of what vdx/lpips.py and vdx/mdvqs.py compute: the yardstick of the MD-VQS tests.

  * the validator's transform (InferNet/template/validator/scoring.py:171-175) with Pillow's own resize, then LPIPS'
    ScalingLayer on the already-normalised tensor (normalize=False, :288);
  * AlexNet's features with torch.nn.functional.conv2d / max_pool2d and the LPIPS formula (R. Zhang et al., CVPR 2018, v0.1
    with `lin` layers), restated from the published definition: the `lpips` package is not installed, so parity with it is
    unpinned — as for the other restated dependencies (tests/vae_encoder_ref.py);
  * a numpy restatement of verify_video_authenticity_common (scoring.py:13-67) on RGB frames in memory, with
    `cv2_shim.cvtColor` for the grey image;
  * the seeded weights are `vdx.lpips.synthetic_state_dict`, shared with `LPIPSAlex.synthetic`.
"""
import numpy as np
import torch
import torch.nn.functional as F

from vdx.compat import cv2_shim
from vdx.lpips import ALEX_CONVS, conv_key, synthetic_state_dict  # noqa: F401  (re-exported for the tests)

MEAN = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)


def frames_like_video(F_, H, W, seed):
    """tests/test_clip_score_gpu.py's recipe: smooth colour fields + noise, every frame different."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    out = []
    for f in range(F_):
        a, b, c = g.uniform(0, 6.3, 3)
        base = np.stack([np.sin(3 * xx + a + 0.2 * f), np.cos(4 * yy + b), np.sin(2 * (xx + yy) + c)], -1)
        img = 127.5 + 90 * base + g.normal(0, 20, (H, W, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return np.stack(out)


def pil_resize(frames):
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(f).resize((224, 224), Image.BILINEAR)) for f in frames])


def scaled_pixels_u8(u8_224, sd):
    """Resized uint8 (F, 224, 224, 3) -> what conv1 sees, fp32 (F, 3, 224, 224): ToTensor + Normalize (:171-175), then
    (x - shift) / scale (LPIPS' ScalingLayer; normalize=False, :288)."""
    x = (torch.from_numpy(np.ascontiguousarray(u8_224)).permute(0, 3, 1, 2).float() / 255 - MEAN) / STD
    return (x - sd["scaling_layer.shift"].float()) / sd["scaling_layer.scale"].float()


def scaled_pixels(frames, sd):
    return scaled_pixels_u8(pil_resize(frames), sd)


def alex_taps(x, sd):
    """fp32 (F, 3, 224, 224) -> the five ReLU taps, NCHW."""
    taps = []
    for i, (_s, _idx, _ci, _co, _k, stride, pad) in enumerate(ALEX_CONVS):
        if i in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[conv_key(i) + ".weight"].float(), sd[conv_key(i) + ".bias"].float(), stride=stride, padding=pad))
        taps.append(x)
    return taps


def tap_distance(a, b, lin, dtype=torch.float32):
    """One tap of LPIPS between feature maps a, b (n, C, H, W) with lin (C,) -> (n,)."""
    a, b, lin = a.to(dtype), b.to(dtype), lin.to(dtype)
    na = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    nb = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((na - nb).pow(2) * lin.view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_pairs_from_taps(taps, sd):
    """-> (per-pair distances (F-1,), per-tap contributions (5, F-1))."""
    per_tap = torch.stack([tap_distance(t[:-1], t[1:], sd[f"lin{i}.model.1.weight"].reshape(-1)) for i, t in enumerate(taps)])
    return per_tap.sum(0), per_tap


def lpips_pairs(frames, sd):
    with torch.no_grad():
        return lpips_pairs_from_taps(alex_taps(scaled_pixels(frames, sd), sd), sd)


def lpips_state_dict_file_layout(sd):
    """The synthetic weights as a full `lpips.LPIPS(net='alex').state_dict()` is recalled to list them: the `lin` layers also
    under the `lins` ModuleList."""
    out = dict(sd)
    for i in range(5):
        out[f"lins.{i}.model.1.weight"] = sd[f"lin{i}.model.1.weight"]
    return out


def rows_to_nchw(rows, n, s):
    """Channels-last rows [n*s*s][C] -> (n, C, s, s) float32."""
    return rows.float().view(n, s, s, -1).permute(0, 3, 1, 2).contiguous()


# ---- the authenticity gate (scoring.py:13-67) ---------------------------------------------------------------------------
def grey_hist(frame):
    """cv2.calcHist([gray], [0], None, [256], [0, 256]) of the frame's grey image: float32 (256, 1)."""
    gray = cv2_shim.cvtColor(frame, cv2_shim.COLOR_RGB2GRAY)
    return np.bincount(gray.reshape(-1), minlength=256).astype(np.float32).reshape(256, 1)


def authenticity(frames):
    """scoring.py:17-63 on frames in memory -> (verdict, entropies, frame_diffs)."""
    prev, frame_diffs, entropies = None, [], []
    for frame in frames:
        hist = grey_hist(frame)
        hist = hist / hist.sum()
        entropies.append(-np.sum(hist * np.log2(hist + 1e-10)))
        if prev is not None:
            diff = np.abs(frame.astype(np.int16) - prev.astype(np.int16)).astype(np.uint8)       # cv2.absdiff
            frame_diffs.append(np.mean(diff))
        prev = frame.copy()
    if not frame_diffs or not entropies:
        return False, entropies, frame_diffs
    if np.std(entropies) < 0.01 or np.mean(entropies) < 0.01:
        return False, entropies, frame_diffs
    if np.std(frame_diffs) < 0.01 or np.mean(frame_diffs) < 0.01:
        return False, entropies, frame_diffs
    return True, entropies, frame_diffs
