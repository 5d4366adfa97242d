"""`AutoencoderKL` (decode half) on libvdx_hip.so — the call the reference makes per frame after the blend:

    fsdp_chunked_coherent.py:219-225
        img_lat = self.vae.decode(z/0.18215).sample
        img = (img_lat[0].permute(1,2,0)*0.5+0.5).clamp(0,1);  frames.append((img*255).byte().cpu().numpy())

Same call surface as diffusers (`vae.decode(z).sample`, `vae.config.scaling_factor`, `named_children()` through
nn.Module), same state-dict keys (oracle/vae_ref.py restates the arithmetic).  Everything is
the UNet's kernels on channels-last fp16 rows [n*h*w][C]:

  * post_quant_conv (1x1, 4->4) is folded EXACTLY into conv_in: the latent gets a fifth channel of ones, whose
    folded weights carry conv_in(bias of post_quant_conv) — zero padding then still pads the *output* of
    post_quant_conv, as in the reference (a plain bias fold would be wrong on the border pixels);
  * ResNet blocks = GroupNorm+SiLU kernels + implicit-GEMM 3x3 convolutions (residual / 1x1 shortcut fused);
  * mid-block attention (ONE head of 512 channels over h*w tokens): q and k GEMMs, V^T by the swapped GEMM (per
    image), scores = one GEMM per image (fp16 [tokens][tokens], as diffusers' baddbmm materialises them; a power of two
    of its 1/sqrt(C) rides in the packed to_q so that they are finite wherever diffusers' are: `qk_fold`), row softmax
    kernel (fp32, the rest of the scale applied in fp32), P.V^T GEMM, output projection with fused residual; the value
    bias is folded into the output projection's bias (softmax rows sum to 1);
  * upsamplers = the conv kernel's fused nearest-x2 gather;
  * the video path maps the last rows straight to uint8 HWC frames (`decode_frames_u8`), bit-exact with the
    reference's fp16 mapping given the same decoder output.
`load_diffusers_state_dict` accepts and drops the encoder / quant_conv keys (they are not on the reference's path).

The encoder half (video-to-video refinement, Zeroscope v2 XL's second stage: diffusers `VideoToVideoSDPipeline` +
`AutoencoderKL.encode`; UNPINNED — diffusers is not part of the parity set, like the decoder and DDIM) is
ingested on its own by `load_diffusers_encoder_state_dict` into `self.E`, so `W` / `num_parameters()` keep their meaning:
  * conv_in (3->128) as im2col rows + GEMM; `encode_frames_u8` writes those rows straight from uint8 frames
    (vdx_frames_to_conv_in_u8, the [-1, 1] map as a 256-entry fp16 table);
  * down blocks of ResNets (the decoder's `_resnet`), each but the last followed by Downsample2D(padding=0) =
    conv3x3 stride 2 on F.pad(x, (0,1,0,1)): the GEMM's pad_mode 1 gather;
  * the mid block (ResNet, single-head attention, ResNet: `_attention`), GroupNorm + SiLU, conv_out (512->8) with
    quant_conv (1x1, 8->8) folded in exactly: W' = Wq.Wout, b' = Wq.bout + bq;
  * the diagonal-Gaussian posterior, sampled (or its mode) and scaled in one kernel (vdx_vae_posterior_f16).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import ops, packing
from ._lib import VdxError


GN_PARTITION = 8      # GroupNorm statistics are reduced with the row-slab partition of an 8-frame batch whatever the
                      # batch: a frame decoded alone (as the reference does, :219-225) has the bits of its batched self


def qk_fold(C: int) -> Tuple[float, float]:
    """(pre, scale) of the mid-block attention at width C.  The score GEMM stores q.k^T as fp16 BEFORE the softmax kernel
    applies 1/sqrt(C), where diffusers' baddbmm(alpha = 1/sqrt(C)) scales first: unscaled, a raw dot product above 65504
    is +inf and its row NaN, while diffusers' form is finite up to 65504 sqrt(C).  So both loaders pack to_q (weight and
    bias) times `pre`, the power of two 2^-ceil(log2(C)/2) <= 1/sqrt(C) (2^-5 at C = 512; exact in fp16 above the
    subnormal range), and `_attention` hands `scale` = 1/(pre sqrt(C)) in [1, 2) to the softmax: pre * scale = 1/sqrt(C),
    and the stored scores are never larger than diffusers' scaled ones."""
    pre = 2.0 ** -(((C - 1).bit_length() + 1) // 2)
    return pre, 1.0 / (pre * math.sqrt(C))


@dataclass
class VaeConfig:
    latent_channels: int = 4
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.18215

    @staticmethod
    def sd() -> "VaeConfig":
        return VaeConfig()


class AutoencoderKL(nn.Module):
    def __init__(self, cfg: Optional[VaeConfig] = None):
        super().__init__()
        self.cfg = cfg or VaeConfig()
        self.config = SimpleNamespace(**vars(self.cfg))
        self.W: Dict[str, torch.Tensor] = {}
        self.E: Dict[str, torch.Tensor] = {}      # packed encoder (load_diffusers_encoder_state_dict)
        self._device = torch.device("cpu")
        for c in self.cfg.block_out_channels:
            if c % 64 != 0:
                raise VdxError(f"AutoencoderKL: channel width {c} is not a multiple of 64")

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def load_diffusers_state_dict(self, sd: Dict[str, torch.Tensor], device=None):
        """Ingest a diffusers-format AutoencoderKL state dict (decoder.* and post_quant_conv.*) and pack it."""
        dev = torch.device(device) if device is not None else self._device
        cfg = self.cfg
        W: Dict[str, torch.Tensor] = {}
        used = set()

        def put(name, t):
            W[name] = t.to(device=dev, dtype=torch.float16).contiguous()

        def get(k):
            used.add(k)
            if k not in sd:
                raise VdxError(f"missing key in state dict: {k}")
            return sd[k].to(dev)

        def norm(p):
            put(p + ".weight", get(p + ".weight"))
            put(p + ".bias", get(p + ".bias"))

        def conv3(p, pad_out=False):
            w, b = packing.pack_conv3x3(get(p + ".weight")), get(p + ".bias")
            put(p + ".weight", packing.pad_rows(w, 64) if pad_out else w)
            put(p + ".bias", packing.pad_rows(b, 64) if pad_out else b)

        def resnet(p, cin, cout):
            norm(p + ".norm1"); conv3(p + ".conv1"); norm(p + ".norm2"); conv3(p + ".conv2")
            if cin != cout:
                put(p + ".conv_shortcut.weight", packing.pack_conv1x1(get(p + ".conv_shortcut.weight")))
                put(p + ".conv_shortcut.bias", get(p + ".conv_shortcut.bias"))

        rev = tuple(reversed(cfg.block_out_channels))
        # conv_in o post_quant_conv, exactly: input channels [z0..z3, 1]
        wq, bq = get("post_quant_conv.weight").float().reshape(cfg.latent_channels, -1), get("post_quant_conv.bias").float()
        wi = get("decoder.conv_in.weight").float()                               # [512][4][3][3]
        folded = torch.cat([torch.einsum("ocyx,ci->oiyx", wi, wq),               # sum_c' W_in[o,c',ky,kx] W_pq[c',c]
                            torch.einsum("ocyx,c->oyx", wi, bq)[:, None]], 1)    # ones channel: W_in . b_pq
        put("decoder.conv_in.weight", packing.pack_conv_in(folded))
        put("decoder.conv_in.bias", get("decoder.conv_in.bias"))
        # mid block
        mb = "decoder.mid_block"
        resnet(mb + ".resnets.0", rev[0], rev[0])
        a = mb + ".attentions.0"
        norm(a + ".group_norm")
        pre = qk_fold(rev[0])[0]                                                  # keeps the fp16 scores finite: qk_fold
        put(a + ".to_q.weight", packing.pack_conv1x1(get(a + ".to_q.weight")).float() * pre)
        put(a + ".to_q.bias", get(a + ".to_q.bias").float() * pre)
        put(a + ".to_k.weight", packing.pack_conv1x1(get(a + ".to_k.weight")))
        put(a + ".to_k.bias", get(a + ".to_k.bias"))
        put(a + ".to_v.weight", packing.pack_conv1x1(get(a + ".to_v.weight")))    # issued as the swapped GEMM (V^T)
        wo = packing.pack_conv1x1(get(a + ".to_out.0.weight"))
        put(a + ".to_out.0.weight", wo)
        # P.(V + 1 b_v^T) = P.V + b_v  (rows of P sum to 1): the value bias moves behind the output projection
        put(a + ".to_out.0.bias", get(a + ".to_out.0.bias").float() + wo.float() @ get(a + ".to_v.bias").float())
        resnet(mb + ".resnets.1", rev[0], rev[0])
        # up blocks
        prev = rev[0]
        for i, ch in enumerate(rev):
            for j in range(cfg.layers_per_block + 1):
                resnet(f"decoder.up_blocks.{i}.resnets.{j}", prev if j == 0 else ch, ch)
            if i != len(rev) - 1:
                conv3(f"decoder.up_blocks.{i}.upsamplers.0.conv")
            prev = ch
        norm("decoder.conv_norm_out")
        conv3("decoder.conv_out", pad_out=True)
        extra = {k for k in sd if k not in used and not k.startswith(("encoder.", "quant_conv."))}
        if extra:
            raise VdxError(f"unexpected keys in state dict: {sorted(extra)[:5]} ... ({len(extra)})")
        self.W, self._device = W, dev
        return self

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        if self.W or self.E:
            probe = fn(torch.empty(0, dtype=torch.float16, device=self._device))
            self.W = {k: v.to(probe.device) for k, v in self.W.items()}
            self.E = {k: v.to(probe.device) for k, v in self.E.items()}
            self._device = probe.device
        return out

    def num_parameters(self) -> int:
        return sum(v.numel() for v in self.W.values())

    # ------------------------------------------------------------------------------------------
    def _resnet(self, p, x, n, hh, ww, W=None):
        W, g = (self.W if W is None else W), self.cfg.norm_num_groups
        M, S = n * hh * ww, hh * ww
        geo = (n, hh, ww, hh, ww, 1, False)
        h = ops.groupnorm(x, W[p + ".norm1.weight"], W[p + ".norm1.bias"], groups=g, n_samples=n, rows_per_sample=S,
                          eps=1e-6, silu_act=True, partition_samples=GN_PARTITION)
        h = ops.gemm(h, W[p + ".conv1.weight"], M=M, mode=ops.CONV3X3, bias=W[p + ".conv1.bias"], conv=geo)
        h = ops.groupnorm(h, W[p + ".norm2.weight"], W[p + ".norm2.bias"], groups=g, n_samples=n, rows_per_sample=S,
                          eps=1e-6, silu_act=True, partition_samples=GN_PARTITION)
        sc = x
        if p + ".conv_shortcut.weight" in W:
            sc = ops.gemm(x, W[p + ".conv_shortcut.weight"], M=M, bias=W[p + ".conv_shortcut.bias"])
        return ops.gemm(h, W[p + ".conv2.weight"], M=M, mode=ops.CONV3X3, bias=W[p + ".conv2.bias"], residual=sc, conv=geo)

    def _attention(self, p, x, n, hh, ww, W=None):
        W, g = (self.W if W is None else W), self.cfg.norm_num_groups
        S, M, C = hh * ww, n * hh * ww, x.shape[1]
        if S % 64 != 0:
            raise VdxError(f"AutoencoderKL attention needs h*w % 64 == 0 (got {hh}x{ww})")
        t = ops.groupnorm(x, W[p + ".group_norm.weight"], W[p + ".group_norm.bias"], groups=g, n_samples=n,
                          rows_per_sample=S, eps=1e-6, silu_act=False, partition_samples=GN_PARTITION)
        q = ops.gemm(t, W[p + ".to_q.weight"], M=M, bias=W[p + ".to_q.bias"])
        k = ops.gemm(t, W[p + ".to_k.weight"], M=M, bias=W[p + ".to_k.bias"])
        o = torch.empty((M, C), dtype=torch.float16, device=x.device)
        scores = torch.empty((S, S), dtype=torch.float16, device=x.device)
        vt = torch.empty((C, S), dtype=torch.float16, device=x.device)
        scale = qk_fold(C)[1]                                                     # q carries the other factor of 1/sqrt(C)
        for i in range(n):                                                        # one image at a time: [S][S] scores
            rows = slice(i * S, (i + 1) * S)
            ops.gemm(W[p + ".to_v.weight"], t[rows], M=C, out=vt)                 # V^T [C][S] (its bias: see load)
            ops.gemm(q[rows], k[rows], M=S, out=scores)                           # q . k^T  (k rows = the GEMM's W)
            ops.softmax_rows(scores, rows=S, cols=S, scale=scale)
            ops.gemm(scores, vt, M=S, out=o[rows])
        return ops.gemm(o, W[p + ".to_out.0.weight"], M=M, bias=W[p + ".to_out.0.bias"], residual=x)

    def _decode_rows(self, z):
        """z (n,4,h,w) fp16 on the GPU -> channels-last rows [n*H*W][64] (RGB in the first 3 columns), H, W."""
        cfg, W = self.cfg, self.W
        if not W:
            raise VdxError("AutoencoderKL: no weights loaded")
        if z.dim() != 4 or z.shape[1] != cfg.latent_channels:
            raise VdxError(f"AutoencoderKL.decode: expected (n,{cfg.latent_channels},h,w), got {tuple(z.shape)}")
        if not z.is_cuda:
            raise VdxError("AutoencoderKL.decode: expected a GPU tensor (the decode path has no CPU fallback)")
        n, _, hh, ww = z.shape
        z5 = torch.cat([z.to(torch.float16), torch.ones_like(z[:, :1], dtype=torch.float16)], 1)
        x = ops.conv_in(z5.unsqueeze(2).contiguous(), W["decoder.conv_in.weight"], W["decoder.conv_in.bias"])
        mb = "decoder.mid_block"
        x = self._resnet(mb + ".resnets.0", x, n, hh, ww)
        x = self._attention(mb + ".attentions.0", x, n, hh, ww)
        x = self._resnet(mb + ".resnets.1", x, n, hh, ww)
        nb = len(cfg.block_out_channels)
        for i in range(nb):
            for j in range(cfg.layers_per_block + 1):
                x = self._resnet(f"decoder.up_blocks.{i}.resnets.{j}", x, n, hh, ww)
            if i != nb - 1:
                p = f"decoder.up_blocks.{i}.upsamplers.0.conv"
                x = ops.gemm(x, W[p + ".weight"], M=n * 4 * hh * ww, mode=ops.CONV3X3, bias=W[p + ".bias"],
                             conv=(n, hh, ww, 2 * hh, 2 * ww, 1, True))
                hh, ww = 2 * hh, 2 * ww
        t = ops.groupnorm(x, W["decoder.conv_norm_out.weight"], W["decoder.conv_norm_out.bias"], groups=cfg.norm_num_groups,
                          n_samples=n, rows_per_sample=hh * ww, eps=1e-6, silu_act=True, partition_samples=GN_PARTITION)
        y = ops.gemm(t, W["decoder.conv_out.weight"], M=n * hh * ww, mode=ops.CONV3X3, bias=W["decoder.conv_out.bias"],
                     conv=(n, hh, ww, hh, ww, 1, False))
        return y, hh, ww

    @torch.no_grad()
    def decode(self, z, return_dict=True):
        """diffusers surface: `.decode(z).sample` -> (n,3,H,W) fp16."""
        y, H, Wd = self._decode_rows(z)
        n = z.shape[0]
        out = ops.rows_to_ncfhw(y, n, self.cfg.out_channels, 1, H, Wd).reshape(n, self.cfg.out_channels, H, Wd)
        return SimpleNamespace(sample=out) if return_dict else (out,)

    @torch.no_grad()
    def decode_frames_u8(self, z):
        """z (n,4,h,w) -> uint8 (n,H,W,3) on the GPU: decode + the reference's frame mapping (:224-225) in one pass."""
        y, H, Wd = self._decode_rows(z)
        return ops.rows_to_u8_frames(y, z.shape[0], H, Wd)

    # ------------------------------------------------------------------------------------------
    # encoder (video-to-video refinement; the module docstring)
    @torch.no_grad()
    def load_diffusers_encoder_state_dict(self, sd: Dict[str, torch.Tensor], device=None):
        """Ingest the `encoder.*` and `quant_conv.*` keys of a diffusers AutoencoderKL state dict and pack them into `self.E`.
        Keys of the decoder half are ignored (a whole VAE table may be passed); unknown encoder keys are refused."""
        dev = torch.device(device) if device is not None else self._device
        cfg = self.cfg
        E: Dict[str, torch.Tensor] = {}
        used = set()

        def put(name, t):
            E[name] = t.to(device=dev, dtype=torch.float16).contiguous()

        def get(k):
            used.add(k)
            if k not in sd:
                raise VdxError(f"missing key in state dict: {k}")
            return sd[k].to(dev)

        def norm(p):
            put(p + ".weight", get(p + ".weight"))
            put(p + ".bias", get(p + ".bias"))

        def conv3(p):
            put(p + ".weight", packing.pack_conv3x3(get(p + ".weight")))
            put(p + ".bias", get(p + ".bias"))

        def resnet(p, cin, cout):
            norm(p + ".norm1"); conv3(p + ".conv1"); norm(p + ".norm2"); conv3(p + ".conv2")
            if cin != cout:
                put(p + ".conv_shortcut.weight", packing.pack_conv1x1(get(p + ".conv_shortcut.weight")))
                put(p + ".conv_shortcut.bias", get(p + ".conv_shortcut.bias"))

        ch = tuple(cfg.block_out_channels)
        put("encoder.conv_in.weight", packing.pack_conv_in(get("encoder.conv_in.weight")))    # [128][64]: K = tap*3 + c
        put("encoder.conv_in.bias", get("encoder.conv_in.bias"))
        prev = ch[0]
        for i, c in enumerate(ch):
            for j in range(cfg.layers_per_block):
                resnet(f"encoder.down_blocks.{i}.resnets.{j}", prev if j == 0 else c, c)
            if i != len(ch) - 1:
                conv3(f"encoder.down_blocks.{i}.downsamplers.0.conv")
            prev = c
        mb = "encoder.mid_block"
        resnet(mb + ".resnets.0", ch[-1], ch[-1])
        a = mb + ".attentions.0"
        norm(a + ".group_norm")
        pre = qk_fold(ch[-1])[0]                                                  # keeps the fp16 scores finite: qk_fold
        put(a + ".to_q.weight", packing.pack_conv1x1(get(a + ".to_q.weight")).float() * pre)
        put(a + ".to_q.bias", get(a + ".to_q.bias").float() * pre)
        put(a + ".to_k.weight", packing.pack_conv1x1(get(a + ".to_k.weight")))
        put(a + ".to_k.bias", get(a + ".to_k.bias"))
        put(a + ".to_v.weight", packing.pack_conv1x1(get(a + ".to_v.weight")))
        wo = packing.pack_conv1x1(get(a + ".to_out.0.weight"))
        put(a + ".to_out.0.weight", wo)
        put(a + ".to_out.0.bias", get(a + ".to_out.0.bias").float() + wo.float() @ get(a + ".to_v.bias").float())
        resnet(mb + ".resnets.1", ch[-1], ch[-1])
        norm("encoder.conv_norm_out")
        # quant_conv o conv_out, exactly (a 1x1 conv after a 3x3 conv is one 3x3 conv): W' = Wq.Wout, b' = Wq.bout + bq
        nz = 2 * cfg.latent_channels
        wq = get("quant_conv.weight").float().reshape(nz, nz)
        bq = get("quant_conv.bias").float()
        wout, bout = get("encoder.conv_out.weight").float(), get("encoder.conv_out.bias").float()
        wf = torch.einsum("qo,ocyx->qcyx", wq, wout)
        bf = wq @ bout + bq
        put("encoder.conv_out.weight", packing.pad_rows(packing.pack_conv3x3(wf), 64))
        put("encoder.conv_out.bias", packing.pad_rows(bf, 64))
        extra = {k for k in sd if k.startswith(("encoder.", "quant_conv.")) and k not in used}
        if extra:
            raise VdxError(f"unexpected encoder keys in state dict: {sorted(extra)[:5]} ... ({len(extra)})")
        self.E = E
        if not self.W:
            self._device = dev
        return self

    def _check_encode_size(self, H, Wd):
        if not self.E:
            raise VdxError("AutoencoderKL: no encoder weights loaded (load_diffusers_encoder_state_dict)")
        if H % 8 or Wd % 8 or ((H // 8) * (Wd // 8)) % 64:
            raise VdxError(f"AutoencoderKL.encode: H and W must be multiples of 8 with (H/8)*(W/8) % 64 == 0 "
                           f"(the mid-block attention's token tiles), got {H}x{Wd}")

    def _encode_rows(self, cols, n, H, Wd):
        """conv_in's im2col rows [n*H*W][64] -> the posterior's moment rows [n*h*w][64] (mean 0..3, logvar 4..7), h, w."""
        cfg, E = self.cfg, self.E
        x = ops.gemm(cols, E["encoder.conv_in.weight"], M=n * H * Wd, bias=E["encoder.conv_in.bias"])
        hh, ww = H, Wd
        nb = len(cfg.block_out_channels)
        for i in range(nb):
            for j in range(cfg.layers_per_block):
                x = self._resnet(f"encoder.down_blocks.{i}.resnets.{j}", x, n, hh, ww, E)
            if i != nb - 1:
                p = f"encoder.down_blocks.{i}.downsamplers.0.conv"
                x = ops.gemm(x, E[p + ".weight"], M=n * (hh // 2) * (ww // 2), mode=ops.CONV3X3, bias=E[p + ".bias"],
                             conv=(n, hh, ww, hh // 2, ww // 2, 2, False), pad_mode=1)
                hh, ww = hh // 2, ww // 2
        mb = "encoder.mid_block"
        x = self._resnet(mb + ".resnets.0", x, n, hh, ww, E)
        x = self._attention(mb + ".attentions.0", x, n, hh, ww, E)
        x = self._resnet(mb + ".resnets.1", x, n, hh, ww, E)
        t = ops.groupnorm(x, E["encoder.conv_norm_out.weight"], E["encoder.conv_norm_out.bias"], groups=cfg.norm_num_groups,
                          n_samples=n, rows_per_sample=hh * ww, eps=1e-6, silu_act=True, partition_samples=GN_PARTITION)
        m = ops.gemm(t, E["encoder.conv_out.weight"], M=n * hh * ww, mode=ops.CONV3X3, bias=E["encoder.conv_out.bias"],
                     conv=(n, hh, ww, hh, ww, 1, False))
        return m, hh, ww

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        """diffusers surface: `.encode(x).latent_dist` for x (n,3,H,W) fp16 in [-1, 1] on the GPU -> a
        `DiagonalGaussianDistribution` (.mean, .logvar, .mode(), .sample(noise=))."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise VdxError(f"AutoencoderKL.encode: expected (n,3,H,W), got {tuple(x.shape)}")
        if not x.is_cuda:
            raise VdxError("AutoencoderKL.encode: expected a GPU tensor (the encode path has no CPU fallback)")
        n, _, H, Wd = x.shape
        self._check_encode_size(H, Wd)
        cols = torch.empty((n * H * Wd, 64), dtype=torch.float16, device=x.device)
        x5 = x.to(torch.float16).unsqueeze(2).contiguous()
        ops._launch("vdx_im2col_in_f16", x5.data_ptr(), cols.data_ptr(), n, 3, 1, H, Wd, 64)
        m, hh, ww = self._encode_rows(cols, n, H, Wd)
        dist_ = DiagonalGaussianDistribution(m, n, hh, ww)
        return SimpleNamespace(latent_dist=dist_) if return_dict else (dist_,)

    @torch.no_grad()
    def encode_frames_u8(self, frames, posterior: str = "sample", noise=None, batch: int = 8):
        """uint8 RGB frames (T,H,W,3) on the GPU -> the scaled latent (1,4,T,H/8,W/8) fp16:
        `scaling_factor * encode(map(frames)).latent_dist.sample(noise)` (or `.mode()`), bit for bit, `batch` frames per pass
        (frames are independent samples: the bits do not depend on `batch`).  map = diffusers' video preprocessing cast to
        fp16; noise (T,4,h,w) fp16 is required for "sample"."""
        if posterior not in ("sample", "mode"):
            raise VdxError(f"encode_frames_u8: posterior must be 'sample' or 'mode', got {posterior!r}")
        T, H, Wd = ops.check_u8_frames(frames, "encode_frames_u8")
        self._check_encode_size(H, Wd)
        h, w = H // 8, Wd // 8
        hw = h * w
        if posterior == "sample":
            if noise is None or tuple(noise.shape) != (T, 4, h, w) or noise.dtype != torch.float16 or not noise.is_cuda:
                raise VdxError(f"encode_frames_u8: posterior 'sample' needs fp16 noise ({T},4,{h},{w}) on the GPU")
            noise = noise.contiguous()
        lat = torch.empty((1, 4, T, h, w), dtype=torch.float16, device=frames.device)
        for i0 in range(0, T, batch):
            nb = min(batch, T - i0)
            cols = ops.frames_to_conv_in(frames[i0:i0 + nb])
            m, _, _ = self._encode_rows(cols, nb, H, Wd)
            ops.vae_posterior(m, nb, hw, eps=noise[i0:i0 + nb] if posterior == "sample" else None,
                              scale=self.cfg.scaling_factor, out=lat, out_offset=i0 * hw, out_strides=(T * hw, hw))
        return lat


class DiagonalGaussianDistribution:
    """diffusers' `DiagonalGaussianDistribution` over the encoder's moment rows [n*h*w][64] (mean = columns 0..3,
    logvar = 4..7): `.mean` / `.logvar` (clamped to [-30, 20]) as (n,4,h,w) fp16, `.mode()`, `.sample(noise=)`; the last
    two run vdx_vae_posterior_f16 (std = exp(0.5*logvar), mean + std*noise, fp16 after every op)."""

    def __init__(self, moments, n, h, w):
        self.moments, self.n, self.h, self.w = moments, n, h, w

    def _cols(self, c0):
        n, h, w = self.n, self.h, self.w
        return self.moments[:n * h * w, c0:c0 + 4].reshape(n, h, w, 4).permute(0, 3, 1, 2).contiguous()

    @property
    def mean(self):
        return self._cols(0)

    @property
    def logvar(self):
        return torch.clamp(self._cols(4), -30.0, 20.0)

    def mode(self):
        return ops.vae_posterior(self.moments, self.n, self.h * self.w).view(self.n, 4, self.h, self.w)

    def sample(self, noise=None, generator=None):
        if noise is None:
            noise = torch.randn((self.n, 4, self.h, self.w), generator=generator, device=self.moments.device,
                                dtype=torch.float16)
        return ops.vae_posterior(self.moments, self.n, self.h * self.w, eps=noise.to(torch.float16).contiguous()
                                 ).view(self.n, 4, self.h, self.w)
