/* vdx.h — C-ABI of libvdx_hip.so: the MI355X (gfx950) kernels behind the
 * diffusers `UNet3DConditionModel` / `DDIMScheduler` call surface that the
 * reference's `Distribution/strategies/fsdp_chunked_coherent.py` uses.
 *
 * The reference has no native code; every entry point below
 * replaces a group of torch/diffusers operator calls reached from
 *   fsdp_chunked_coherent.py:140   noise = self.unet(x, t, encoder_hidden_states=emb).sample
 *   fsdp_chunked_coherent.py:133-137,141-142   ctx injection, CFG combine, scheduler.step
 *   fsdp_chunked_coherent.py:204-217   linear-ramp overlap blend
 * Each declaration cites the operator(s) it stands in for.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (the host side allocates through PyTorch-ROCm); no allocation, no sync inside;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, not waited for;
 *   - return 0 on success, negative on error; `vdx_last_error()` gives the message
 *     (thread-local);
 *   - activations are fp16, channels-last: a (B,C,F,H,W) tensor of diffusers is held as the
 *     row-major matrix [B*F*H*W rows][C] ("rows" = latent pixels of one frame);
 *   - all contractions accumulate in fp32 on the matrix cores (v_mfma_f32_16x16x32_f16).
 */
#ifndef VDX_H
#define VDX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vdx_stream_t;

const char* vdx_last_error(void);
int vdx_version(void);
/* 0 for the product build.  Non-zero: some translation unit was compiled with a lab macro (phase stamps, ablations — timing
 * only, some variants compute wrong results); bit = unit (1 gemm, 2 gemm_ws, 4 tattn_fused, 8 tattn2, 16 flash, 32 ff_fused,
 * 64 conv_fused, 128 xattn; csrc/lab.h lists every unit's switches).  The Python binding refuses such a library unless VDX_ALLOW_LAB_BUILD=1 (the lab tools set it). */
int vdx_build_flags(void);

/* ------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM family:  out[M][N] = epilogue( A_gathered[M][K] * W[N][K]^T )
 * Replaces torch.nn.Linear / Conv2d(3x3,1x1) / Conv3d((3,1,1)) as composed by diffusers
 * ResnetBlock2D, TemporalConvLayer, Transformer2DModel, TransformerTemporalModel,
 * Downsample2D, Upsample2D, all reached from
 * fsdp_chunked_coherent.py:140.
 * ---------------------------------------------------------------------------------------- */
enum { VDX_GEMM_PLAIN = 0, VDX_GEMM_CONV3X3 = 1, VDX_GEMM_TCONV3 = 2 };
enum { VDX_EPI_GEGLU = 1 };

typedef struct vdx_gemm_args {
    const void* a;        /* fp16 source 0, row stride lda (elements)                           */
    const void* a2;       /* fp16 source 1 (channel concat after source 0) or NULL              */
    const void* w;        /* fp16 [N][K], K contiguous; gathers: K = (c/64)*T*64 + tap*64 + c%64,
                             T = 9 (tap = ky*3+kx) or 3 (tap = kt)                                 */
    const void* bias;     /* fp16 [N] or NULL                                                    */
    const void* bias2;    /* fp16 [M / rows_per_bias2][N] or NULL (time-embedding projection)    */
    const void* residual; /* fp16 [M][ldr] or NULL, added after bias                             */
    void* out;            /* fp16 [M][ldo]   (GEGLU: [M][N/2])                                   */
    int32_t M, N, K;      /* N % 64 == 0, K % 64 == 0                                            */
    int32_t mode;         /* VDX_GEMM_*                                                          */
    int32_t c1, c2;       /* channels of source 0 / 1; per-tap K = c1 + c2; both % 64 == 0       */
    int32_t lda, lda2, ldo, ldr;
    int32_t h_in, w_in;   /* conv3x3: source image size (rows of `a` = n*h_in*w_in)              */
    int32_t h_out, w_out; /* conv3x3: output image size (M = n*h_out*w_out)                      */
    int32_t stride;       /* conv3x3: 1 or 2 (pad 1, or pad_mode below)                          */
    int32_t upsample;     /* conv3x3: 1 = source is nearest-x2 upsampled on the fly; 2 = nearest-upsampled to
                           * (h_out, w_out) — diffusers' `upsample_size` path for latents not divisible by 8;
                           * 3 = nearest x2 in PHASE form: the same result as 1 computed as four 2x2 convolutions on the
                           * source image, one per output parity.  `w` is the phase table [4][N][4*c1] (phase p = 2a + b for
                           * output (2i+a, 2j+b); tap 2*ty + tx reads source (i+a-1+ty, j+b-1+tx); weights = the sums of the
                           * 3x3 taps that fall on that source pixel; K order as for 9 taps), K = 4*c1, M = n*h_out*w_out
                           * as ever, N a multiple of 8, stride 1, h_out = 2*h_in, w_out = 2*w_in.  The kernels walk
                           * 4 * round_up(M / 4, 256) VIRTUAL rows, phase-major: row_begin (a multiple of 256) / row_end
                           * and vdx_gemm_plan's split_row count those.  Tiled kernels only (variants 1 2 5 6 9); refused
                           * with bias2, residual, a2, GEGLU, pad_mode, stride 2, ksplit and weight sets          */
    int32_t frames, hw;   /* tconv3: M = b*frames*hw, taps step `hw` rows, zero pad in time      */
    int32_t rows_per_bias2, ldb2; /* bias2 row = m / rows_per_bias2, row stride ldb2 elements        */
    int32_t epilogue;     /* VDX_EPI_* flags                                                     */
    int32_t row_begin, row_end; /* only output rows [row_begin, row_end) are computed (row_end 0 = M); every pointer
                             still addresses row 0 and M stays the whole product's row count.  Lets a caller cover one
                             product with two calls that use different tile shapes (vdx_gemm_plan); the results are
                             bit-identical however the rows are split                                 */
    int32_t ksplit;       /* > 1: the rows of this call are computed on 256x320 tiles as `ksplit` slices of K per tile
                             (fp32 partial slabs in `workspace`) + a fixed-order reduction that runs the epilogue.  Fills
                             the chip when the call has far fewer than 256 tiles (the tail of a product).  Changes the
                             summation order of these rows (NOT bit-identical to ksplit = 0; deterministic)          */
    int32_t wset_rows;    /* > 0: ONE WEIGHT SET PER `wset_rows` ROWS — rows [s*wset_rows, (s+1)*wset_rows) use w + s*N*K and
                             wset_bias + s*N (a GroupNorm folded into this Linear: vdx_groupnorm_fold_linear_f16).  Plain
                             mode on the weights-stationary kernels only (K = 320 / 640, M and wset_rows multiples of 64),
                             no bias / bias2 / residual / GEGLU                                                    */
    void* workspace;      /* ksplit > 1: >= tiles * ksplit * 327 680 bytes (vdx_gemm_plan_ksplit), 16-byte aligned    */
    const float* wset_bias; /* wset_rows > 0: fp32 [M / wset_rows][N], the initial accumulators                          */
    size_t workspace_bytes; /* ksplit > 1: the size of `workspace`; the call is refused when the slabs would not fit        */
    int32_t pad_mode;     /* conv3x3 zero padding: 0 = 1 on every side (Conv2d(padding=1)); 1 = (0, 1, 0, 1), stride 2 only:
                             diffusers Downsample2D(padding=0) = conv3x3_s2(F.pad(x, (0,1,0,1))) — output pixel yo reads
                             rows 2yo .. 2yo+2, row h_in is zero, h_out = h_in / 2.  Refused with upsample and split-K;
                             the fused GroupNorm conv (vdx_conv3x3_gn_f16) has no such mode                           */
} vdx_gemm_args;

int vdx_gemm_f16(const vdx_gemm_args* a, vdx_stream_t stream);

/* What vdx_gemm_f16 would do with `a` (host-only, launches nothing): *variant = the kernel family it picks for rows
 * [row_begin, row_end) (1 = 128x128, 2 = 256x320, 8 = 128x320 ring, 5 = 256x64, 7 = weights-stationary), *split_row = a row at
 * which splitting the product into two calls ([row_begin, split_row) and [split_row, row_end)) is expected to be faster
 * (whole rounds of 256 big tiles + a tail of small ones instead of a mostly idle last round), or 0.                  */
int vdx_gemm_plan(const vdx_gemm_args* a, int32_t* variant, int32_t* split_row);
/* The name of the kernel instantiation vdx_gemm_f16(a) would launch for rows [row_begin, row_end) with a->ksplit, as
 * rocprofv3 prints it without `void `, namespaces and the argument list ("gemm_kernel<256, 320, 4, 2, 1, false, true, 0>";
 * a split-K call: its slice kernel + " split-K + reduce").  Host-only: launches nothing, needs no GPU, and formats the
 * name where the template is instantiated, so it cannot differ from the launch.  It runs vdx_gemm_f16's whole validation
 * of shapes, flags and geometry (a refused call has no name) but not that of the split-K workspace; pointers are tested
 * for null (the weights-stationary route depends on `residual` and `bias2`), never dereferenced.  `n`: the size of `buf`;
 * a name that does not fit (with its terminator) is an error, never truncated.                                      */
int vdx_gemm_kernel_name(const vdx_gemm_args* a, char* buf, size_t n);
/* The same question with a split-K tail allowed (whole products only): rows [0, *split_row) as one ordinary call, rows
 * [*split_row, M) as one call with ksplit = *ksplit and a workspace of *workspace_bytes; *ksplit = 0 when vdx_gemm_plan's
 * answer is at least as good.  Pays on the 16-frame windows of BASELINE cfg4 / cfg5, whose row counts leave 1/8 - 1/2 of a
 * round of big tiles (level 2: 288 tiles on 256 CUs).                                                              */
int vdx_gemm_plan_ksplit(const vdx_gemm_args* a, int32_t* split_row, int32_t* ksplit, size_t* workspace_bytes);

/* conv_in gather: (B,Cin,F,H,W) fp16 latent -> im2col rows [B*F*H*W][Kpad], K = (ky*3+kx)*Cin + ci,
 * zero padded to Kpad (multiple of 64); conv_in = this + vdx_gemm_f16 with w [Cout][Kpad]
 * (UNet3DConditionModel.conv_in after the permute/reshape).                         */
int vdx_im2col_in_f16(const void* x_ncfhw, void* out_rows, int B, int Cin, int F, int H, int W,
                      int Kpad, vdx_stream_t stream);

/* channels-last rows [B*F*H*W][ld] (first C columns) -> (B,C,F,H,W) fp16 (UNet output permute) */
int vdx_rows_to_ncfhw_f16(const void* rows, int ld, void* out, int B, int C, int F, int H, int W,
                          vdx_stream_t stream);

/* y = x * sigmoid(x), n elements (TimestepEmbedding act / ResnetBlock2D.nonlinearity(temb)).  The correctly rounded
 * function to 0.51 fp16 ulp for every finite fp16 x; +inf -> +inf, -inf and NaN -> NaN, as torch. */
int vdx_silu_f16(const void* x, void* y, size_t n, vdx_stream_t stream);

/* Sinusoidal timestep embedding of UNet3DConditionModel (`Timesteps(320, flip_sin_to_cos=True, shift 0)`):
 * out[b][0:dim/2] = cos(t*f_j), out[b][dim/2:] = sin(t*f_j), f_j = exp(-ln(1e4) j / (dim/2)); fp32 math, fp16 store.
 * `t_device` points at ONE fp32 timestep in device memory (all B batch items share it, fsdp_chunked_coherent.py:140). */
int vdx_timestep_embedding_f16(const float* t_device, void* out, int B, int dim, vdx_stream_t stream);

/* y = gelu(x) (exact, erf), n elements: CLIPMLP's activation between fc1 and fc2 (hidden_act "gelu").  Within 0.75e-7 |x|
 * (+ rounding) of x Phi(x) for every finite fp16 x; +inf -> +inf, -inf and NaN -> NaN (torch's CPU fp32 gelu gives NaN for
 * +inf too). */
int vdx_gelu_f16(const void* x, void* y, size_t n, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Normalisation (torch.nn.GroupNorm on 4-D and 5-D inputs, torch.nn.LayerNorm).
 * GroupNorm over `rows_per_sample` rows x (C/G) channels per (sample, group):
 *   4-D GN: rows_per_sample = H*W (sample = one frame); 5-D GN: rows_per_sample = F*H*W.
 * Two sources (x | x2) cover the skip concatenation in up blocks.
 * ---------------------------------------------------------------------------------------- */
size_t vdx_groupnorm_workspace(int n_samples, int rows_per_sample, int C, int G);
/* y[M][C] = act( (x - mean) * rstd * gamma + beta ), act = SiLU if silu != 0                   */
int vdx_groupnorm_f16(const void* x, int c1, int ldx, const void* x2, int c2, int ldx2,
                      const void* gamma, const void* beta, float eps, int G,
                      int n_samples, int rows_per_sample, int silu,
                      void* y, int ldy, void* workspace, vdx_stream_t stream);
/* The same with the row-slab partition of the statistics fixed as for `partition_samples` samples (0 = n_samples): a
 * sample's result then has the same bits alone, in part of a batch or in the whole batch (callers that split a batch
 * to save memory, or decode frames one by one like fsdp_chunked_coherent.py:219-225, pass the full batch size). */
size_t vdx_groupnorm_workspace_part(int n_samples, int rows_per_sample, int C, int G, int partition_samples);
/* GroupNorm folded into the Linear that follows it without an activation (Transformer2DModel / TransformerTemporalModel:
 * `norm` -> `proj_in`): the statistics pass of vdx_groupnorm_part_f16, then per sample s
 *   w_out[s] = fp16(w diag(scale_s))  [N][C],   bias_out[s] = bias + w.beta - w_out[s].mean_s  (fp32 [N])
 * so that  vdx_gemm_f16(x, w_out, wset_rows = rows_per_sample, wset_bias = bias_out)  ==  Linear(GroupNorm(x)) without
 * the normalised tensor ever being written.  w_out: n_samples*N*C fp16, bias_out: n_samples*N fp32.              */
int vdx_groupnorm_fold_linear_f16(const void* x, int C, int ldx, const void* gamma, const void* beta, float eps, int G,
                                  int n_samples, int rows_per_sample, void* workspace, int partition_samples,
                                  const void* w, const void* bias, int N, void* w_out, void* bias_out, vdx_stream_t stream);
int vdx_groupnorm_part_f16(const void* x, int c1, int ldx, const void* x2, int c2, int ldx2,
                           const void* gamma, const void* beta, float eps, int G,
                           int n_samples, int rows_per_sample, int silu,
                           void* y, int ldy, void* workspace, int partition_samples, vdx_stream_t stream);
/* The statistics pass alone: leaves scale[s][c] = rstd_s,g * gamma_c and shift[s][c] = beta_c - mean_s,g * scale as
 * [n_samples][C][2] fp32 at byte *scale_shift_offset of `workspace` (vdx_groupnorm_workspace_part bytes), for a consumer that
 * applies the normalisation itself (vdx_tconv_gn_f16).                                                               */
int vdx_groupnorm_stats_f16(const void* x, int c1, int ldx, const void* x2, int c2, int ldx2, const void* gamma,
                            const void* beta, float eps, int G, int n_samples, int rows_per_sample, void* workspace,
                            int partition_samples, size_t* scale_shift_offset, vdx_stream_t stream);
/* K3 — TemporalConvLayer's Sequential(GroupNorm, SiLU, Conv3d (3,1,1)) with the normalisation applied INSIDE the convolution
 * (SURVEY.md §2.3 row TemporalConvLayer, App. A.4; reached four times per layer from fsdp_chunked_coherent.py:140):
 *   out[(b*F + f)*S + p][n] = bias[n] + residual + sum_kt sum_c w[n][(c/64)*192 + kt*64 + c%64] * silu(x[(b*F + f+kt-1)*S + p][c] * scale[b][c] + shift[b][c])
 * with zero rows for frames outside [0, F) (the padding applies to the normalised tensor).  x: raw rows [B*F*S][ldx];
 * scale_shift: [B][C][2] fp32 from vdx_groupnorm_stats_f16 (n_samples = B, rows_per_sample = F*S); w: the packed temporal
 * weights of vdx_gemm_f16's VDX_GEMM_TCONV3 mode ([N][3*C]).  Supported: C % 64 == 0, N % 320 == 0, F % 8 == 0
 * (vdx_tconv_gn_supported); other shapes take vdx_groupnorm_f16 + vdx_gemm_f16.                                        */
/* K1 — ResnetBlock2D's conv(SiLU(GroupNorm(x))) with the normalisation applied INSIDE the 3x3 convolution (SURVEY.md §2.3 row
 * ResnetBlock2D, App. A.3; conv1 and conv2 of every ResNet block, reached from fsdp_chunked_coherent.py:140):
 *   out[n*h*w + y*w + x][o] = bias[o] + bias2[(n*h*w) / rows_per_bias2][o] + residual + sum_{ky,kx,c} w[o][(c/64)*576 + (ky*3+kx)*64 + c%64]
 *                             * silu(cat(a, a2)[n*h*w + (y+ky-1)*w + (x+kx-1)][c] * scale[n][c] + shift[n][c])
 * with zero for pixels outside the image (the padding applies to the normalised tensor).  a / a2: raw rows (a2 / c2 = the skip
 * tensor of the up blocks, or NULL / 0); scale_shift: [n_img][c1 + c2][2] fp32 from vdx_groupnorm_stats_f16 (n_samples = n_img,
 * rows_per_sample = h*w); w: the packed weights of vdx_gemm_f16's VDX_GEMM_CONV3X3 mode.  Stride 1, no upsampling.
 * Supported: c1 % 64 == 0, c2 % 64 == 0, N % 320 == 0; vdx_conv3x3_gn_preferred: expected to beat vdx_groupnorm_f16 + vdx_gemm_f16
 * (one column tile, image width a multiple of 32, the chip filled twice over: level 0 of the XL UNet).                */
int vdx_conv3x3_gn_supported(int c1, int c2, int N);
int vdx_conv3x3_gn_preferred(int c1, int c2, int N, int n_img, int h, int w);
int vdx_conv3x3_gn_f16(const void* a, int lda, const void* a2, int lda2, int c1, int c2, const float* scale_shift,
                       const void* w, const void* bias, const void* bias2, int rows_per_bias2, int ldb2,
                       const void* residual, int ldr, void* out, int ldo, int n_img, int h, int w_px, int N,
                       vdx_stream_t stream);
int vdx_tconv_gn_supported(int C, int N, int F);
/* 1 when K3 is expected to beat vdx_groupnorm_f16 + vdx_gemm_f16 on this shape (one column tile, the chip filled twice over) */
int vdx_tconv_gn_preferred(int C, int N, int B, int F, int S);
int vdx_tconv_gn_f16(const void* x, int ldx, const float* scale_shift, const void* w, const void* bias,
                     const void* residual, int ldr, void* out, int ldo, int B, int F, int S, int C, int N,
                     vdx_stream_t stream);
/* In-place softmax over the first `cols` columns of each of `rows` rows of x (row stride ld), logits scaled by
 * `scale` in fp32: the probabilities of AutoencoderKL's mid-block attention (one 512-channel head over h*w
 * tokens; diffusers Attention with upcast softmax), reached from fsdp_chunked_coherent.py:223.            */
int vdx_softmax_rows_f16(void* x, int ld, int rows, int cols, float scale, vdx_stream_t stream);

int vdx_layernorm_f16(const void* x, int ldx, const void* gamma, const void* beta, float eps,
                      int M, int C, void* y, int ldy, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Attention cores (diffusers `Attention` with plain softmax, scale = d^-0.5, head dim 64).
 * ---------------------------------------------------------------------------------------- */
/* Flash-style attention over contiguous sequences (spatial self-attention and text
 * cross-attention of Transformer2DModel).
 *   q  : fp16 rows [n_seq*sq][ldq], head h at columns h*64..h*64+63
 *   k  : fp16 rows [n_kv*skv_pad][ldk]
 *   vt : fp16 [heads*64][ldvt]  V transposed: vt[h*64+d][kvb*skv_pad + key]
 *   kv batch of sequence s is s / seq_per_kv (cross-attn: all frames of a sample share text).
 *   causal != 0: query i sees keys <= i only (CLIPTextModel's self-attention, fsdp_chunked_coherent.py:102).
 *   out: fp16 rows [n_seq*sq][ldo].
 *   Supported score range: |q.k * scale| <= 5000 nat.  The kernel's lazy softmax offset is carried as an fp16 MFMA
 *   operand; up to that magnitude its spacing (<= 4 exp2-units) keeps a re-centred row inside the window in which
 *   no further move is needed; it is clamped at +-60000 exp2-units, beyond ~11000 nat rows can stay mis-centred.  */
int vdx_flash_attn_f16(const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt,
                       void* out, int ldo, int n_seq, int sq, int skv, int skv_pad, int heads,
                       int seq_per_kv, float scale, int causal, vdx_stream_t stream);
/* The same with V as ROWS: v fp16 [n_kv*skv_pad][ldv], head h at columns h*64.. like k — q, k and v can then be the
 * three column blocks of ONE projection's output (spatial self-attention of Transformer2DModel: no transposed V
 * product).  The V tile is staged like K and transposed by the LDS read (ds_read_b64_tr_b16).  skv_pad >= skv, any
 * value (a V^T row of 8-key chunks is what asks for a multiple of 8 above); rows skv..skv_pad-1 must hold finite values. */
int vdx_flash_attn_rows_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                            void* out, int ldo, int n_seq, int sq, int skv, int skv_pad, int heads,
                            int seq_per_kv, float scale, int causal, vdx_stream_t stream);

/* K8 — the feed-forward sub-block of BasicTransformerBlock (`t = t + ff(norm3(t))`, GEGLU with the
 * erf GELU, both in Transformer2DModel and TransformerTemporalModel) as ONE kernel: LayerNorm -> [val | gate] projection ->
 * val * gelu(gate) -> output projection (+bias) + residual; the [rows][4*inner] intermediate never leaves the CU
 * (csrc/ff_fused.hip).  Built for inner 320 (level 0).  Its GELU is a polynomial in clamp(gate, -4.5, 4.5): within
 * 2.1e-5 |gate| of gate Phi(gate) for gate >= -4.5; for gate < -4.5 the result is up to 2.44e-5 |gate| below the exact -0
 * (a linear left tail: -4e-4 at gate = -16).  The GEGLU epilogue of vdx_gemm_f16 (a table of Phi on [-5, 5)) is within
 * 3.1e-6 |gate| everywhere and gives exactly -0 for gate < -5.
 *   t, out : fp16 rows [M][ld], `inner` columns used; out may not alias t
 *   packed : vdx/packing.py pack_k8 (LayerNorm's affine folded into the first projection), vdx_ff_block_pack_bytes bytes */
int vdx_ff_block_supported(int inner);
size_t vdx_ff_block_pack_bytes(int inner);
int vdx_ff_block_f16(const void* t, int ldt, const void* packed, float eps, void* out, int ldo, int M, int inner,
                     vdx_stream_t stream);
/* The same kernel with the transformer's `proj_out` and its residual behind the feed-forward (the sub-block's output never
 * reaches HBM): out[r] = x[r % xrows] + W_p . (t[r] + ff(LayerNorm(t[r]))) + b_p.  x: the transformer's input rows, xrows = M, or
 * M / 2 when both halves of the batch pair with the same rows of x (the CFG-shared prefix); proj_packed: vdx/packing.py
 * pack_k8_proj (25 weight units, fp32 b_p; vdx_ff_block_proj_pack_bytes bytes).  out may alias neither t nor x. */
size_t vdx_ff_block_proj_pack_bytes(int inner);
int vdx_ff_block_proj_f16(const void* t, int ldt, const void* packed, float eps, const void* x, int ldx, int xrows,
                          const void* proj_packed, void* out, int ldo, int M, int inner, vdx_stream_t stream);

/* Temporal self-attention of TransformerTemporalModel: sequences run over the
 * F frames of one latent pixel.  qkv: fp16 rows [B*F*HW][ldqkv] = [q | k | v] each heads*64
 * wide, row = (b*F + f)*HW + p.  out rows likewise, [ldo] wide.  F <= 128.                     */
int vdx_temporal_attn_f16(const void* qkv, int ldqkv, void* out, int ldo, int B, int F, int HW,
                          int heads, float scale, vdx_stream_t stream);

/* K7 — one attention sub-block of TransformerTemporalModel (`s = s + attn(LN(s))`, both attn1 and the
 * "double self-attention" attn2) as ONE kernel: LayerNorm -> q|k|v -> softmax over the F frames of each latent pixel
 * -> P.V -> to_out.0 (+bias) + residual.  Rows are read once and written once (csrc/tattn_fused.hip).
 *   t, out : fp16 rows [B*F*HW][ld], row = (b*F + f)*HW + p, `inner` columns used; out may not alias t
 *   gamma, beta : LayerNorm affine [inner];  bo : to_out.0 bias [inner]
 *   wqkv_packed / wo_packed : weight stage images (vdx/packing.py pack_k7_qkv / pack_k7_out), sizes given by
 *   vdx_temporal_attn_block_wqkv_bytes / _wo_bytes.
 * Supported: inner 320 or 512, F a divisor of 48 (vdx_temporal_attn_block_supported); callers use the separate
 * LayerNorm / GEMM / vdx_temporal_attn_f16 kernels otherwise.                                              */
int vdx_temporal_attn_block_supported(int inner, int F);
size_t vdx_temporal_attn_block_wqkv_bytes(int inner);
size_t vdx_temporal_attn_block_wo_bytes(int inner);
int vdx_temporal_attn_block_f16(const void* t, int ldt, const void* gamma, const void* beta, float eps,
                                const void* wqkv_packed, const void* wo_packed, const void* bo,
                                void* out, int ldo, int B, int F, int HW, int inner, float scale,
                                vdx_stream_t stream);

/* K5 (csrc/xattn.hip) — the cross-attention sub-block of diffusers' BasicTransformerBlock in a spatial transformer
 * (`t = t + attn2(norm2(t), encoder_hidden_states)`; call site fsdp_chunked_coherent.py:140) as one kernel:
 *   out[r] = t[r] + W_o . softmax_k( c . (W_q LN(t[r]))_h . K[item(r)]_h[k] ) V[item(r)]_h + b_o      per head h, k < kv_len
 * t / out: [n_items * rows_per_item][inner] fp16 rows, item(r) = r / rows_per_item; `packed`: vdx/packing.py pack_k5 (q units
 * with LayerNorm's affine and the scale folded in, output-projection units, fp32 q bias, fp32 b_o;
 * vdx_cross_attn_block_pack_bytes bytes); `kv_packed`: the text keys / values of every item in MFMA-fragment order
 * (pack_k5_kv: n_items * vdx_cross_attn_block_kv_bytes bytes), 80 key slots of which the first kv_len are used.
 * out may not alias t.  Supported: inner 320, 1 <= kv_len <= 80.                                                          */
int vdx_cross_attn_block_supported(int inner, int kv_len);
size_t vdx_cross_attn_block_pack_bytes(int inner);
size_t vdx_cross_attn_block_kv_bytes(int inner);
int vdx_cross_attn_block_f16(const void* t, int ldt, const void* packed, const void* kv_packed, int kv_len, float eps,
                             void* out, int ldo, int n_items, int rows_per_item, int inner, vdx_stream_t stream);

/* K7, second design (csrc/tattn2.hip) — the same sub-block (`s = s + attn(LN(s))`; call site
 * fsdp_chunked_coherent.py:140) with LayerNorm's affine, the softmax scale and all biases folded into ONE packed blob
 * (vdx/packing.py pack_k7b: q|k|v units, output-projection units with the permuted k index, fp32 q bias, fp32 output
 * bias; vdx_temporal_attn_block2_pack_bytes bytes).  t / out as above.  Supported: inner 320, F a divisor of 48.   */
int vdx_temporal_attn_block2_supported(int inner, int F);
size_t vdx_temporal_attn_block2_pack_bytes(int inner);
int vdx_temporal_attn_block2_f16(const void* t, int ldt, const void* packed, float eps, void* out, int ldo,
                                 int B, int F, int HW, int inner, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Orchestration ops the reference owns (fsdp_chunked_coherent.py).
 * ---------------------------------------------------------------------------------------- */
/* :133-137  x = cat[lat,lat] (+ w * ctx.repeat(F));  lat (1,C,F,H,W), ctx (1,C,1,H,W) or NULL  */
int vdx_cfg_input_f16(const void* lat, const void* ctx, float weight, void* x2, int C, int F,
                      int HW, vdx_stream_t stream);
/* :141-142  lat' = DDIM.step(u + gs*(c-u), t, lat)  with the four scheduler coefficients;
 * eps2 (2,C,F,H,W) = [u; c].  Rounds to fp16 after every tensor op, like torch.              */
int vdx_cfg_ddim_step_f16(const void* eps2, const void* lat, void* lat_out, float guidance,
                          float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                          float sqrt_one_minus_aprev, size_t n, vdx_stream_t stream);
/* :142 alone: lat' = DDIM.step(eps, t, lat) (no CFG combine) — what `scheduler.step` of the
 * unchanged reference script binds to.                                                        */
int vdx_ddim_step_f16(const void* eps, const void* lat, void* lat_out, float sqrt_one_minus_at,
                      float sqrt_at, float sqrt_aprev, float sqrt_one_minus_aprev, size_t n,
                      vdx_stream_t stream);
/* DPM-Solver++ (2M, midpoint; diffusers `DPMSolverMultistepScheduler.step`, the scheduler Zeroscope's published recipe
 * swaps in for DDIM) fused with the CFG combine of :141 — replaces `u + gs*(c-u)` + `convert_model_output` +
 * `dpm_solver_first_order_update` / `multistep_dpm_solver_second_order_update`, about a dozen elementwise launches per step.
 * fp32 host coefficients, fp16 rounding after every tensor op, in this order (vdx/scheduler.py states the schedule):
 *   e  = u + guidance*(c - u);        x0 = (lat - c_s0*e) * c_inv_a0        -> x0_out (the next step's history)
 *   lat' = c_x*lat + c_d0*x0  [ + c_d1 * (c_inv_r0 * (x0 - x0_prev)) ]        -> lat_out
 * x0_prev == NULL selects the first-order form (c_d1, c_inv_r0 unused).  c_d0 = -at*(exp(-h)-1), c_d1 = 0.5*c_d0,
 * c_inv_r0 = 1/r0: D1 = (1/r0)*(x0 - x0_prev) is a tensor of its own and rounds before the 0.5*... product, so the two
 * scalars cannot be folded into one.  lat_out may be lat; x0_out may not be x0_prev, and no other two may overlap.
 * Every pointer 16-byte aligned (16-byte accesses; eps2's second half element-wise when n % 8 != 0); any n.             */
int vdx_cfg_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                         float guidance, float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1,
                         float c_inv_r0, size_t n, vdx_stream_t stream);
/* the same step on a model output the caller already combined (or never guided: the miner loop, an unchanged
 * reference-style script calling `scheduler.step`) — replaces diffusers' `DPMSolverMultistepScheduler.step` alone.     */
int vdx_dpm_step_f16(const void* eps, const void* lat, const void* x0_prev, void* x0_out, void* lat_out, float c_s0,
                     float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, size_t n,
                     vdx_stream_t stream);
/* Temporal co-denoising (MultiDiffusion along time; no reference counterpart, opt-in: vdx/codenoise.py, csrc/codenoise.hip).
 * `vdx_cfg_input_f16` above, reading frames [s, e) out of the whole clip's latent z (1,C,T,H,W): x2 (2,C,e-s,H,W) contiguous,
 * one launch, the ctx term with the same two fp16 roundings.  Pointers 16-byte aligned; x2 must not overlap z.           */
int vdx_cfg_input_window_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int HW, int s, int e,
                             vdx_stream_t stream);
/* One denoising step of the whole clip from K windows' raw UNet outputs.  `windows` + win_off[k] (elements) is window k's
 * contiguous (2,C,L_k,H,W) block [u; c] for frames [win_start[k], win_start[k] + win_len[k]); the three tables are HOST
 * arrays of K rows (they travel to the kernel as arguments, so every row is checked here first: 1 <= K <= 64, every range
 * inside [0, T), every block inside the `windows_elems` halves behind `windows`, every frame in some window).  wn: DEVICE
 * fp32 [K][T], the normalised weights (only entries inside a window's range are read).  Per element (c, t, p), over the
 * windows that hold t, k ascending:  U = sum wn[k][t]*u_k,  Cc = sum wn[k][t]*c_k  (fp32; every product and every add its
 * own rounding, the sum starts with the first product), u = fp16(U), c = fp16(Cc), and from there EXACTLY the chain of
 * vdx_cfg_ddim_step_f16 with the same four coefficients: lat_out (1,C,T,H,W); lat_out may be z.                            */
int vdx_cofuse_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                 const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                 float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                 float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream);
/* The same fused noise into EXACTLY the chain of vdx_cfg_dpm_step_f16, with its seven scalars and its rules for x0_prev
 * (NULL: first order), x0_out and lat_out, all of the whole clip's shape (1,C,T,H,W).                                      */
int vdx_cofuse_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev,
                                void* x0_out, void* lat_out, float guidance, float c_s0, float c_inv_a0, float c_x,
                                float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW, vdx_stream_t stream);
/* Spatially tiled co-denoising (MultiDiffusion along space on top of the above; no reference counterpart, opt-in: vdx/codenoise.py
 * `DiffuserConfig.tile`, csrc/cotile.hip, restated in tests/cotile_ref.py).  `vdx_cfg_input_window_f16` additionally cropped to rows
 * [y0, y0 + th) and columns [x0, x0 + tw) of z (1,C,T,H,W) and of ctx (1,C,1,H,W): x2 (2,C,e-s,th,tw) contiguous, one launch, the ctx
 * term with the same two fp16 roundings.  Every range is checked; pointers 16-byte aligned; x2 must not overlap z or ctx.          */
int vdx_cfg_input_tile_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int H, int W, int s, int e, int y0,
                           int th, int x0, int tw, vdx_stream_t stream);
/* One denoising step of the whole clip from Kt x ny x nx windows' raw UNet outputs: the Cartesian product of the Kt time windows of
 * vdx_cofuse_cfg_ddim_step_f16 (same three HOST tables, same wn), ny row bands [tile_y0[ky], + th) and nx column bands
 * [tile_x0[kx], + tw) (HOST arrays; 1 <= Kt <= 64, ny*nx <= 64, every band inside the frame, every frame, row and column in some
 * band).  `windows` + win_off[kt] + (ky*nx + kx)*tile_stride (elements) is the contiguous (2,C,L_kt,th,tw) block [u; c] of that
 * window; blocks may not overlap and must lie inside the `windows_elems` halves.  wyn: DEVICE fp32 [ny][H], wxn: DEVICE fp32 [nx][W],
 * the per-axis normalised weights (only entries inside a band are read).  Per element (c, t, y, x), over the windows that hold it,
 * in ascending (kt, ky, kx):  w = fp32(fp32(wn[kt][t]*wyn[ky][y])*wxn[kx][x]),  U = sum w*u_k,  Cc = sum w*c_k  (fp32; every product
 * and every add its own rounding, the sum starts with the first product), u = fp16(U), c = fp16(Cc), and from there EXACTLY the
 * chain of vdx_cfg_ddim_step_f16 / vdx_cfg_dpm_step_f16 with their scalars and their rules for x0_prev, x0_out and lat_out (which
 * may be z).  With ny = nx = 1 and th = H, tw = W the result has the bits of the vdx_cofuse_* step.  16-byte accesses where W, tw,
 * every tile_x0, every win_off and tile_stride are multiples of 8, 8-byte for multiples of 4, else element-wise.               */
int vdx_cotile_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                 const int* win_start, const int* win_len, int Kt, const float* wn, size_t tile_stride,
                                 const int* tile_y0, int ny, const float* wyn, const int* tile_x0, int nx, const float* wxn, int th,
                                 int tw, void* lat_out, float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                 float sqrt_one_minus_aprev, int C, int T, int H, int W, vdx_stream_t stream);
int vdx_cotile_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                const int* win_start, const int* win_len, int Kt, const float* wn, size_t tile_stride,
                                const int* tile_y0, int ny, const float* wyn, const int* tile_x0, int nx, const float* wxn, int th,
                                int tw, const void* x0_prev, void* x0_out, void* lat_out, float guidance, float c_s0, float c_inv_a0,
                                float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int H, int W, vdx_stream_t stream);
/* Seamless looping for co-denoising: ring windows (AnimateDiff's `closed_loop` context option; MultiDiffusion along time with
 * periodic windows; no reference counterpart, opt-in: vdx/codenoise.py `loop_plan`, `DiffuserConfig.loop`, csrc/codenoise.hip, its RING flag, restated
 * in tests/coloop_ref.py).  A window (s, L) holds the frames (s + f) mod T, f in [0, L), with 0 <= s < T and 1 <= L <= T.
 * vdx_cfg_input_loop_f16: `vdx_cfg_input_window_f16` under that rule (note: a LENGTH, not an end): x2 (2,C,L,h,w) contiguous, one
 * launch, the ctx term with the same two fp16 roundings; 16-byte accesses where HW % 8 == 0, else element-wise; x2 must not overlap
 * z; pointers 16-byte aligned.  A call with s + L <= T has the bits of vdx_cfg_input_window_f16(…, s, s + L).                     */
int vdx_cfg_input_loop_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int HW, int s, int L,
                           vdx_stream_t stream);
/* `vdx_cofuse_cfg_ddim_step_f16` / `vdx_cofuse_cfg_dpm_step_f16` (same arguments, same three HOST tables, same wn, same fuse term
 * for term, same chains, same rules for x0_prev, x0_out and lat_out, same alignment and overlap rules and access widths) with every
 * window row meaning the frames (win_start[k] + f) mod T: per (c, t), for k ascending, f = t - s_k, f += T if f < 0, window k enters
 * if f < L_k.  Checked: 0 <= s_k < T, 1 <= L_k <= T, every block inside the buffer, every frame in some window under the modular
 * rule, 1 <= K <= 64.  A table in which no window wraps gives the bits of the vdx_cofuse_* step.                                 */
int vdx_coloop_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                 const int* win_start, const int* win_len, int K, const float* wn, void* lat_out, float guidance,
                                 float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float sqrt_one_minus_aprev, int C, int T,
                                 int HW, vdx_stream_t stream);
int vdx_coloop_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev,
                                void* x0_out, void* lat_out, float guidance, float c_s0, float c_inv_a0, float c_x,
                                float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW, vdx_stream_t stream);
/* Strided context windows for co-denoising (AnimateDiff-Evolved's `context_stride`, the "uniform" context schedule, restated, not
 * pinned against it; no reference counterpart, opt-in: vdx/codenoise.py `stride_plan`, `DiffuserConfig.context_stride`,
 * csrc/codenoise.hip, restated in tests/costride_ref.py).  A window (s, L, d) holds the frames s + f * d, f in [0, L), with d >= 1,
 * 0 <= s, L >= 1 and s + (L - 1) * d < T (checked in 64 bits).
 * vdx_cfg_input_stride_f16: `vdx_cfg_input_window_f16` under that rule (a LENGTH, not an end): x2 (2,C,L,h,w) contiguous, one
 * launch, no slice copy, the ctx term with the same two fp16 roundings; 16-byte accesses where HW % 8 == 0, else element-wise; x2
 * must not overlap z; pointers 16-byte aligned.  A call with d = 1 has the bits of vdx_cfg_input_window_f16(…, s, s + L).        */
int vdx_cfg_input_stride_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int HW, int s, int L, int d,
                             vdx_stream_t stream);
/* `vdx_cofuse_cfg_ddim_step_f16` / `vdx_cofuse_cfg_dpm_step_f16` (same arguments, same wn, same fuse term for term, same chains,
 * same rules for x0_prev, x0_out and lat_out, same alignment and overlap rules and access widths) with a fourth HOST table,
 * win_stride[K]: per (c, t), for k ascending, q = t - s_k; window k enters with its frame q / d_k if q >= 0, q % d_k == 0 and
 * q / d_k < L_k.  Checked: every row as above, every block (2,C,L_k,h,w) inside the buffer, every frame in some window under the
 * strided rule, 1 <= K <= 64.  The table travels by value in the kernel arguments: 64 rows of (8 + 4 + 4 + 4) bytes, 1.25 KiB.  A
 * table whose strides are all 1 gives the bits of the vdx_cofuse_* step.                                                       */
int vdx_costride_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                   const int* win_start, const int* win_len, const int* win_stride, int K, const float* wn,
                                   void* lat_out, float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                   float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream);
int vdx_costride_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                  const int* win_start, const int* win_len, const int* win_stride, int K, const float* wn,
                                  const void* x0_prev, void* x0_out, void* lat_out, float guidance, float c_s0, float c_inv_a0,
                                  float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW, vdx_stream_t stream);
/* Classifier-free guidance with CFG rescale (Lin et al. 2023, section 3.4; diffusers `rescale_noise_cfg`; no reference counterpart,
 * opt-in: `guidance_rescale` of vdx/scheduler.py, csrc/rescale.hip, restated in tests/rescale_ref.py).  With g the combine above,
 * over the N = n elements of the sample (fp64 sums S1 = sum x, S2 = sum x*x of the fp16 values):
 *   var(x) = (N*S2 - S1*S1) / (N*(N-1))    (fp64, each operation rounded; 0 for a constant x),   sd_x = fp16(sqrt(var(x)))
 *   r = fp16(fp32(sd_c) / fp32(sd_g)),     g' = fp16(fp16(phi * fp16(g * r)) + fp16(phi1 * g)),  phi1 = fp32(1 - rescale)
 * and g' takes g's place in the step.  No clamp: N = 1, sd_g = 0, NaN and infinity give what the lines give.  Two launches:
 * the statistics pass writes `rows` rows [S1c, S2c, S1g, S2g] of doubles (rows: the query next to it, a function of the shapes
 * alone, <= 256; fixed summation order, no atomics), the step adds them in ascending order in every block and forms r itself.
 * stats_out: NULL, or 3 halves that receive [sd_c, sd_g, r].  phi and phi1 outside [0, 1] are refused.  Everything else as
 * for the step of the same name without "rescale"; partials 16-byte aligned and apart from every other buffer.              */
int vdx_cfg_rescale_rows(size_t n);
int vdx_cfg_rescale_stats_f16(const void* eps2, size_t n, float guidance, double* partials, vdx_stream_t stream);
int vdx_cfg_rescale_ddim_step_f16(const void* eps2, const void* lat, void* lat_out, const double* partials, void* stats_out,
                                  float guidance, float phi, float phi1, float sqrt_one_minus_at, float sqrt_at,
                                  float sqrt_aprev, float sqrt_one_minus_aprev, size_t n, vdx_stream_t stream);
int vdx_cfg_rescale_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                                 const double* partials, void* stats_out, float guidance, float phi, float phi1, float c_s0,
                                 float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, size_t n,
                                 vdx_stream_t stream);
/* The same for co-denoising: U and Cc fused from the windows exactly as in vdx_cofuse_cfg_ddim_step_f16 (in both launches), the
 * statistics those of the fused Cc and of g(U, Cc) over the whole clip, N = C*T*HW.                                          */
int vdx_cofuse_cfg_rescale_rows(int C, int T);
int vdx_cofuse_cfg_rescale_stats_f16(const void* windows, size_t windows_elems, const int64_t* win_off, const int* win_start,
                                     const int* win_len, int K, const float* wn, float guidance, double* partials, int C, int T,
                                     int HW, vdx_stream_t stream);
int vdx_cofuse_cfg_rescale_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                         const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                         const double* partials, void* stats_out, float guidance, float phi, float phi1,
                                         float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float sqrt_one_minus_aprev,
                                         int C, int T, int HW, vdx_stream_t stream);
int vdx_cofuse_cfg_rescale_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                        const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev,
                                        void* x0_out, void* lat_out, const double* partials, void* stats_out, float guidance,
                                        float phi, float phi1, float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1,
                                        float c_inv_r0, int C, int T, int HW, vdx_stream_t stream);
/* Classifier-free guidance with dynamic thresholding towards a mimic scale (the "Dynamic Thresholding (CFG Scale Fix)" of the A1111 /
 * ComfyUI world; no reference counterpart and no external pin, opt-in: `cfg_mimic` of vdx/scheduler.py, csrc/dynthresh.hip, restated
 * in tests/dynthresh_ref.py).  The sample is (C, T, HW), M = T*HW elements per channel, M below 2^32.  With g the combine above at
 * `guidance` and l the same combine at `mimic`, per channel: mg = fp16(sum g / M), ml = fp16(sum l / M) (fp64 sums in a fixed order,
 * one division, one rounding); d = fp16(g - mg), e = fp16(l - ml); ref_lo = max |e| as the integer bits & 0x7fff; ref_hi = the
 * linear interpolation fp16(lo + f*(hi - lo)) (fp32, each operation rounded; lo's bits when f == 0) between the order statistics
 * lo = a[k], hi = a[min(k+1, M-1)] of the channel's bits(d) & 0x7fff in ascending integer order; s = whichever of ref_lo, ref_hi
 * has the larger bit pattern; g' = fp16(fp16(fp16(clamp(d, -s, s) / s) * ref_lo) + mg) takes g's place in the step.  No other clamp:
 * a constant channel (s = 0), NaN and infinity give what the lines give, in their channel only.  k in [0, M-1] and f in [0, 1) are
 * the host's floor and fraction of q*(M-1) in float64; `mimic` is finite and > 0; all refused otherwise.
 * ws: `vdx_cfg_mimic_ws_bytes(C, T, HW)` bytes (0 for a shape the entries refuse), 16-byte aligned, apart from every other buffer;
 * it may hold anything on entry.  Its layout, every part at a multiple of 16 bytes:
 *   scal fp16 [C][4] = (mg, ref_lo, ref_hi, s) | maxbits uint32 [C] | partials double [C][64][2] | hist uint32 [C][32768]
 * The statistics entry is three launches: 1 the sums (rows [sum g, sum l] per channel, their number a function of the shapes
 * alone and <= 64; it also zeroes hist and maxbits), 2 the histogram and the maximum (integer atomics only), 4 the select, which
 * writes scal.  `stages` is the set of launches to run: 7 for a step; tests and the benchmark run them one at a time.  The step
 * entries read scal.  Everything else as for the step of the same name without "mimic".                                          */
size_t vdx_cfg_mimic_ws_bytes(int C, int T, int HW);
int vdx_cfg_mimic_stats_f16(const void* eps2, int C, int T, int HW, float guidance, float mimic, size_t k, float f, void* ws,
                            int stages, vdx_stream_t stream);
int vdx_cfg_mimic_ddim_step_f16(const void* eps2, const void* lat, void* lat_out, const void* ws, float guidance,
                                float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float sqrt_one_minus_aprev, int C, int T,
                                int HW, vdx_stream_t stream);
int vdx_cfg_mimic_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out, const void* ws,
                               float guidance, float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, int C,
                               int T, int HW, vdx_stream_t stream);
/* The same for co-denoising: U and Cc fused from the windows exactly as in vdx_cofuse_cfg_ddim_step_f16 (in launches 1 and 2 and
 * in the step), the statistics over the whole clip; the rows per channel are min(T, 64).                                         */
size_t vdx_cofuse_cfg_mimic_ws_bytes(int C, int T, int HW);
int vdx_cofuse_cfg_mimic_stats_f16(const void* windows, size_t windows_elems, const int64_t* win_off, const int* win_start,
                                   const int* win_len, int K, const float* wn, float guidance, float mimic, size_t k, float f,
                                   void* ws, int stages, int C, int T, int HW, vdx_stream_t stream);
int vdx_cofuse_cfg_mimic_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                       const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                       const void* ws, float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                       float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream);
int vdx_cofuse_cfg_mimic_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                      const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev,
                                      void* x0_out, void* lat_out, const void* ws, float guidance, float c_s0, float c_inv_a0,
                                      float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW, vdx_stream_t stream);
/* Masked video-to-video (keep frames or regions of --init_video, generate the rest; no reference counterpart, opt-in:
 * vdx/inpaint.py, csrc/inpaint.hip).  Masks are uint8, 1 = regenerate, 0 = keep; every entry point is a SELECT of bits (no
 * arithmetic on the mask: no 0*inf, -0 keeps its sign, NaN / inf stay in their element).  tests/inpaint_ref.py states it.
 * In place on a window's latent z (1,C,L,H,W) after a scheduler step: where mask == 1 z keeps its bits; where mask == 0 z takes
 * the bits of `known` = fp16(fp16(sqrt_ab*x0) + fp16(sqrt_1mab*base)), EXACTLY the chain of vdx_add_noise_f16 (one function,
 * csrc/step_chains.h), or with last != 0 the bits of x0 itself.  x0, base (1,C,T_clip,H,W) fp16 and mask (T_clip,H,W) are the
 * whole CLIP's tensors, read at frame s + f for the window's frame f: 0 <= s, L >= 1, s + L <= T_clip, refused otherwise.
 * Pointers 16-byte aligned; z must not overlap an input; base may be NULL with last != 0.  Any C, T_clip, L, HW >= 1.        */
int vdx_mask_renoise_f16(void* z, const void* x0, const void* base, const void* mask, float sqrt_ab, float sqrt_1mab, int last,
                         int C, int T_clip, int HW, int s, int L, vdx_stream_t stream);
/* The same select on the fp32 blended latent z (1,C,T,H,W), in place: mask ? z : float(x0).                                */
int vdx_mask_paste_f32(float* z, const void* x0, const void* mask, int C, int T, int HW, vdx_stream_t stream);
/* Pixel mask (T,H,W) uint8, nonzero = regenerate, H and W multiples of 8 -> latent mask (T,H/8,W/8) in {0,1}.
 * any == 0 ("nearest"): pixel (8y, 8x), what F.interpolate(mode="nearest") takes at the exact factor 8; any == 1: a cell
 * regenerates if any of its 64 pixels does.  pixel_mask 8-byte aligned.                                                     */
int vdx_mask_to_latent_u8(const void* pixel_mask, void* latent_mask, int T, int H, int W, int any, vdx_stream_t stream);
/* out = mask ? generated : original on packed uint8 (T,H,W,3) frames with a (T,H,W) mask (nonzero = generated); out may be
 * `generated`.  16 pixels per lane where W % 16 == 0, 4 where W % 4 == 0 (and the pointers allow), else one.                */
int vdx_mask_composite_u8(const void* generated, const void* original, const void* mask, void* out, int T, int H, int W,
                          vdx_stream_t stream);
/* :204-217 one chunk's contribution: full[s:e] += lat*w (fp16 accumulator), weight[s:e] += w;
 * w = fp32 device vector of length e-s (the linear ramps, built by the host exactly as :207-213) */
int vdx_blend_accumulate_f16(void* full, float* weight, const void* chunk, const float* w, int C,
                             int T, int HW, int s, int e, vdx_stream_t stream);
/* :217 lat = full / clamp(weight, 1e-6) -> fp32                                                */
int vdx_blend_finalize_f32(const void* full, const float* weight, float* out, int C, int T,
                           int HW, vdx_stream_t stream);

/* Decoded frames -> uint8 HWC exactly as fsdp_chunked_coherent.py:224-225 maps them
 * ((sample*0.5+0.5).clamp(0,1), *255, .byte(); fp16 rounding after every op, truncation at the end).
 * rows: the decoder's channels-last output rows [n_pixels][ld], RGB in the first 3 columns.            */
int vdx_rows_to_u8_frames(const void* rows, int ld, size_t n_pixels, void* out_u8, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Exchange steps on RCCL (resolved at run time: no link-time dependency).  One communicator per process / GPU.
 *   vdx_comm_unique_id : rank 0 fills a 128-byte id and shares it with the other ranks out of band
 *   vdx_comm_init      : collective; every rank passes the same id
 *   vdx_allgather_shard: full[r*shard_bytes ..] = rank r's shard — the per-unit parameter gather that stands in for
 *                        FSDP's flat-parameter all-gather (fsdp_chunked_coherent.py:63-88), once per shard unit per step
 *   vdx_halo_exchange  : send `send_bytes` to rank `send_to` and receive `recv_bytes` from rank `recv_from` as one group
 *                        (either side may be 0 bytes) — the overlap frames of the post-loop exchange (:190-202)
 * Both enqueue on `side_stream` and return; the caller orders them against its compute stream with events. */
typedef struct vdx_comm vdx_comm;
/* Peer-mapped shards — the same parameter gather WITHOUT a collective and without compute units: weights
 * are read-only after load, so every rank exports the allocation holding its shards once, maps the others', and pulls.
 *   vdx_ipc_export : 64-byte HIP IPC handle of the allocation `dev_ptr` lies in + its byte offset inside it
 *   vdx_ipc_open   : map a peer's export (another process; same or another GPU of the node) -> device pointer here
 *   vdx_ipc_close  : unmap (pointer and offset as returned / passed above)
 *   vdx_peer_gather: full[r*shard_bytes ..] = srcs[r][0 .. shard_bytes) for r < world, as device-to-device copies on
 *                    `side_stream` (copy engines; srcs[own rank] = the local shard)                              */
int vdx_ipc_export(const void* dev_ptr, void* handle64, size_t* offset_bytes);
int vdx_ipc_open(const void* handle64, size_t offset_bytes, void** dev_ptr);
int vdx_ipc_close(void* dev_ptr, size_t offset_bytes);
int vdx_peer_gather(void* full, const void* const* srcs, int world, size_t shard_bytes, vdx_stream_t side_stream);
int vdx_comm_unique_id(void* id128);
int vdx_comm_init(const void* id128, int rank, int world, vdx_comm** out);
int vdx_comm_destroy(vdx_comm* comm);
int vdx_allgather_shard(vdx_comm* comm, const void* shard, void* full, size_t shard_bytes, vdx_stream_t side_stream);
int vdx_halo_exchange(vdx_comm* comm, const void* send_buf, size_t send_bytes, int send_to, void* recv_buf,
                      size_t recv_bytes, int recv_from, vdx_stream_t side_stream);

/* ------------------------------------------------------------------------------------------
 * Exact-fit grids and the CUs a collective holds.  The weights-stationary GEMMs and the fused sub-block kernels (K5, K7,
 * K8) launch one workgroup per compute unit, and vdx_gemm_plan covers a product with whole rounds of one 256x320 tile per
 * CU + a tail.  While a parameter gather (fsdp_chunked_coherent.py:63-88's FSDP all-gather; here RCCL on a side stream)
 * runs beside the step, each of its channel kernels holds a CU, and an exact-fit launch then runs a whole round more.
 * `vdx_set_reserved_cus(r)` makes every persistent grid and every such main launch leave r CUs free per round (rounded so
 * the grid stays a multiple of 8 = the XCD count; the tail launch takes the rows left over); results do not depend on r,
 * bit for bit.  Process-wide, not thread-safe against concurrent launches; a caller that caches vdx_gemm_plan's answers
 * must drop them when r changes (vdx/ops.py does).  Default 0; vdx/shard.py sets VDX_RESERVED_CUS for a world > 1.       */
int vdx_set_reserved_cus(int n);
int vdx_reserved_cus(void);
int vdx_persistent_grid_cus(void);

/* Box probes — not on the denoising path; bench.py's `box` object and the one-GPU rehearsal of the distributed path.
 *   vdx_probe_mfma_f16      : a fixed dense v_mfma_f32_32x32x16_f16 stream (2 waves / SIMD, per-lane operands) on every CU;
 *                             *flops = its FLOP count; time it with events around the call -> the part's sustained MFMA rate
 *   vdx_probe_occupancy_hog : `blocks` workgroups x 256 threads holding `lds_bytes` of LDS each for `micros` us, touching
 *                             no memory: stands in for the CUs a collective's channel kernels hold                        */
int vdx_probe_mfma_f16(float* out, size_t out_floats, int iters, double* flops, vdx_stream_t stream);
int vdx_probe_occupancy_hog(int blocks, int lds_bytes, int micros, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CLIP prompt-fidelity score of a generated video: the validator's quality score
 *   InferNet/neurons/validator.py:277,898   compute_quality_score_clip(video, prompt)
 *   InferNet/template/validator/scoring.py:87-147   CLIPScorer.compute_quality_score
 *   Q = 1/F * sum_i cos(E_text, E_frame_i) under CLIP ViT-B/32 (csrc/clip.hip; the towers: vdx/clip_vision.py,
 *   vdx/clip_text.py, vdx/clip_score.py).  Frames come as decoded uint8 RGB, not re-read from the mp4 (:110-121).
 * ---------------------------------------------------------------------------------------- */
/* transforms.Resize((224, 224)) + ToTensor + Normalize(ImageNet mean/std) (scoring.py:81-85, :121-122) of F uint8 RGB frames.
 * The resize is Pillow's bilinear filter with antialiasing, bit for bit: a horizontal pass, then a vertical pass, each
 * out = clip8((2^21 + sum px * k) >> 22) with 22-bit weights (uint8 intermediate).  Normalization is
 * ((u / 255) - mean) / std in fp32 with correctly rounded division, then fp16.  The rows are the patch GEMM's operand:
 * row f*49 + py*7 + px, column c*1024 + ky*32 + kx (patch_embedding.weight.reshape(768, 3072)).                        */
typedef struct vdx_clip_preprocess_args {
    const void* frames;         /* uint8: frame f, row y, pixel x, channel c at f*frame_pitch + y*row_pitch + x*3 + c     */
    const int32_t* x_bounds;    /* [224][2] (first input column, count) of each output column's window                 */
    const int32_t* x_coeffs;    /* [224][kx] 22-bit fixed-point weights of those windows                               */
    const int32_t* y_bounds;    /* [224][2] the same for output rows                                                    */
    const int32_t* y_coeffs;    /* [224][ky]                                                                            */
    void* out;                  /* fp16 [F*49][ldo], 3072 columns written                                               */
    void* out_u8;               /* optional uint8 (F, 224, 224, 3): the resized image (tests); NULL in production         */
    size_t frame_pitch;         /* bytes                                                                                 */
    int32_t row_pitch;          /* bytes, >= 3*W                                                                         */
    int32_t F, H, W;
    int32_t kx, ky;             /* row lengths of x_coeffs / y_coeffs                                                    */
    int32_t band;               /* output rows per block                                                                 */
    int32_t span;               /* input rows the widest band's vertical windows cover (LDS: span*224*3 bytes <= 64 KiB)  */
    int32_t ldo;                /* >= 3072, a multiple of 8                                                              */
} vdx_clip_preprocess_args;
int vdx_clip_preprocess_u8(const vdx_clip_preprocess_args* a, vdx_stream_t stream);

/* CLIPVisionEmbeddings + pre_layrnorm (transformers CLIPVisionTransformer; scoring.py:123 get_image_features): patch GEMM
 * rows [F*patches][ldp] -> out rows [F*seq_pad][ldo]: row f*seq_pad + 0 = class_emb + pos[0], row f*seq_pad + t =
 * patch[f*patches + t-1] + pos[t] (t = 1..patches), each LayerNorm'd with fp32 statistics; rows patches+1..seq_pad-1 zero
 * (the attention kernel's key padding).  D <= 1024.                                                                   */
int vdx_clip_vision_embed_f16(const void* patch, int ldp, const void* class_emb, const void* pos_emb, const void* gamma,
                              const void* beta, float eps, int F, int patches, int seq_pad, int D, void* out, int ldo,
                              vdx_stream_t stream);
/* y = x * sigmoid(1.702 x): the `quick_gelu` activation of CLIP ViT-B/32's MLPs (both towers).  y may alias x.  The
 * correctly rounded function to 0.51 fp16 ulp for every finite fp16 x; +inf -> +inf, -inf and NaN -> NaN, as torch.    */
int vdx_quick_gelu_f16(const void* x, void* y, size_t n, vdx_stream_t stream);
/* scoring.py:106-107, :123-124, :137-140: per_frame[f] = F.normalize(img[f]) . F.normalize(txt) (eps 1e-12), *mean = their
 * mean over the F frames.  img fp16 [F][ldi], txt fp16 [D]; per_frame / mean fp32 device memory.  A fixed reduction
 * order: the same bits on every run.                                                                                    */
int vdx_clip_cosine_score_f16(const void* img, int ldi, const void* txt, int F, int D, float* per_frame, float* mean,
                              vdx_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Video-to-video refinement (Zeroscope v2 XL's second stage): diffusers VideoToVideoSDPipeline + AutoencoderKL.encode
 * (unpinned: diffusers is not part of the parity set).  The first-stage clip is resized to the target size
 * (Image.resize, BICUBIC), mapped to [-1, 1], encoded (vdx/vae.py: encoder on the GEMM / GroupNorm / attention kernels),
 * sampled from the diagonal Gaussian posterior, scaled, and noised to the first timestep of the truncated schedule.
 * ---------------------------------------------------------------------------------------- */
/* One pass of Pillow's ImagingResample on 8-bit RGB (any filter; windows + 22-bit weights from the host,
 * vdx/ops.py `clip_resize_coeffs(.., filter=)`): out = clip8((2^21 + sum px * k) >> 22).  Horizontal: (F, H, Wi, 3) -> (F, H, Wo, 3);
 * vertical: (F, Hi, W, 3) -> (F, Ho, W, 3).  bounds [out][2] = (first input index, count), coeffs [out][ksize].
 * Pitches in bytes; pixels packed RGB.  Window indices are clamped to the input.                                */
int vdx_resample_h_u8(const void* in, size_t in_frame_pitch, int in_row_pitch, int F, int H, int Wi, const int32_t* bounds,
                      const int32_t* coeffs, int ksize, int Wo, void* out, size_t out_frame_pitch, int out_row_pitch,
                      vdx_stream_t stream);
int vdx_resample_v_u8(const void* in, size_t in_frame_pitch, int in_row_pitch, int F, int Hi, int W, const int32_t* bounds,
                      const int32_t* coeffs, int ksize, int Ho, void* out, size_t out_frame_pitch, int out_row_pitch,
                      vdx_stream_t stream);
/* uint8 RGB frames (F, H, W, 3) -> the im2col rows of the encoder's conv_in: row f*H*W + y*W + x, column
 * K = (ky*3+kx)*3 + ci holds map(u[f, y+ky-1, x+kx-1, ci]) (0.0 outside the image: the conv pads the NORMALISED image),
 * columns 27..63 zero.  map = lut (256 fp16 on the device, fp16(float32(u)/255*2-1) built on the host).  ldo >= 64, % 8;
 * out_rows 16-byte aligned (16-byte stores).                                                                       */
int vdx_frames_to_conv_in_u8(const void* frames, size_t frame_pitch, int row_pitch, int F, int H, int W, const void* lut_f16,
                             void* out_rows, int ldo, vdx_stream_t stream);
/* DiagonalGaussianDistribution(moments) -> scaled latent.  moments: the encoder's rows [n*h*w][ld] (mean = columns 0..3,
 * logvar = 4..7).  Per element, fp16 after every op like torch: lv = clamp(lv, -30, 20); std = exp(0.5*lv) (expf);
 * x = mean + std*eps (mode_only: x = mean); out = scale*x.  eps fp16 (n,4,h,w) (unused with mode_only).
 * out[c*out_c_stride + i*out_f_stride + p] for image i, channel c, pixel p: (1,4,T,h,w) at frame f0 is
 * out + f0*h*w with strides (T*h*w, h*w); (n,4,h,w) is strides (h*w, 4*h*w).                                   */
int vdx_vae_posterior_f16(const void* moments, int ld, int n, int hw, const void* eps, int mode_only, float scale, void* out,
                          size_t out_c_stride, size_t out_f_stride, vdx_stream_t stream);
/* DDIMScheduler.add_noise: out = sqrt_ab*x0 + sqrt_1mab*noise with fp16 rounding after each op; the two coefficients are
 * fp16 values (alphas_cumprod cast to the sample dtype first, then ** 0.5 — the host evaluates them like diffusers).  */
int vdx_add_noise_f16(const void* x0, const void* noise, void* out, float sqrt_ab, float sqrt_1mab, size_t n,
                      vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MD-VQS: the validator's video-quality term and its authenticity gate
 *   InferNet/neurons/validator.py:120,1295   self.quality_scorer = MDVQS(); compute_quality_score = 0.4 PF + 0.3 VQ + 0.3 TC
 *   InferNet/neurons/validator.py:259,872    verify_video_authenticity
 *   InferNet/template/validator/scoring.py:269-309   VQ = max(0, 1 - mean LPIPS-AlexNet(frame_i, frame_i-1))
 *   InferNet/template/validator/scoring.py:13-67     grey-level entropy and frame differences
 * (csrc/mdvqs.hip; vdx/lpips.py, vdx/mdvqs.py).  The `lpips` package is not part of the parity set: LPIPS is restated from
 * its published definition (unpinned).  The five AlexNet convolutions run on vdx_gemm_f16.
 * ---------------------------------------------------------------------------------------- */
/* conv1's operand from the RESIZED uint8 frames (F, 224, 224, 3) (scoring.py:171-175 Resize((224, 224)): vdx_resample_*_u8 /
 * vdx_clip_preprocess_u8's out_u8): row f*3025 + oy*55 + ox, column (ky*11 + kx)*3 + c = lut[c][u8[f][4oy-2+ky][4ox-2+kx][c]],
 * 0.0 outside the image (Conv2d(3, 64, 11, stride 4, padding 2) pads its input, i.e. after the scaling layer), columns
 * 363..383 zero.  lut_f16: fp16 [3][256] on the device = fp16(((u/255 - mean_c)/std_c - shift_c)/scale_c), both affine maps
 * (ToTensor + Normalize, :171-175; LPIPS' ScalingLayer, reached with normalize=False, :288) in fp32 on the host.
 * ldo >= 384, % 8; out_rows 16-byte aligned.                                                                          */
int vdx_lpips_stem_u8(const void* u8_frames, int F, const void* lut_f16, void* out_rows, int ldo, vdx_stream_t stream);
/* y = max(x, 0) as torch.relu (NaN -> NaN), n elements: AlexNet's ReLU behind conv3..conv5 (:288).  y may alias x.        */
int vdx_relu_f16(const void* x, void* y, size_t n, vdx_stream_t stream);
/* AlexNet's ReLU + MaxPool2d(3, stride 2) behind conv1 and conv2 (:288): rows x [n_img*H*W][ldx] (C columns) are ReLU'd IN
 * PLACE (the LPIPS tap) and out rows [n_img*Ho*Wo][ldo] get the window maxima of the ReLU'd rows, Ho = (H-3)/2 + 1 (no
 * padding; 55 -> 27, 27 -> 13).  C % 8 == 0; out may not alias x.                                                       */
int vdx_relu_maxpool_f16(void* x, int ldx, int n_img, int H, int W, int C, void* out, int ldo, vdx_stream_t stream);
/* Stride-1 im2col of channels-last rows x [n_img*H*W][ldx] (C % 64 == 0): out row n*Ho*Wo + oy*Wo + ox, column
 * (ky*k + kx)*C + c = x[n][oy-pad+ky][ox-pad+kx][c], 0 outside the image, Ho = H + 2 pad - k + 1.  With vdx_gemm_f16 (plain)
 * and w.permute(0, 2, 3, 1).reshape(N, k*k*C): Conv2d(C, N, k, padding=pad) — AlexNet's conv2 (k 5, pad 2; :288).          */
int vdx_im2col_f16(const void* x, int ldx, int n_img, int H, int W, int C, int k, int pad, void* out, int ldo,
                   vdx_stream_t stream);
/* One tap of LPIPS (:288, lpips.LPIPS.forward with lpips=True, spatial=False) for the F-1 consecutive frame pairs: with
 * n(v) = v / (sqrt(sum_c v^2) + 1e-10) per pixel, out[p] (+)= mean_pix sum_c lin[c] (n(x_p) - n(x_p+1))^2.  x: tap rows fp16
 * [F*HW][ldx], C <= 512 columns; lin: fp32 [C] (the non-negative 1x1 `lin` layer; Dropout is the identity in eval mode);
 * out: fp32 [F-1], overwritten (accumulate = 0) or added to (the sum over taps).  fp32 norms, a fixed reduction order without
 * atomics: the same bits on every run; identical frames give exactly 0.                                                */
int vdx_lpips_distance_f16(const void* x, int ldx, int F, int HW, int C, const float* lin, float* out, int accumulate,
                           vdx_stream_t stream);
/* The integer half of verify_video_authenticity_common (:27-36) over F uint8 RGB frames (pitches in bytes as in
 * vdx_clip_preprocess_args): hist[f][g] = pixels of frame f with grey level g = (4899 R + 9617 G + 1868 B + 8192) >> 14
 * (cv2.cvtColor's 8-bit weights; cv2.calcHist's counts), absdiff[f] = sum over all bytes of |frame f+1 - frame f|
 * (cv2.absdiff; F-1 sums, may be NULL for F = 1).  Both are zeroed on the stream, then filled with integer atomics: exact.
 * The host finishes (normalise, entropy, means) in numpy with the reference's dtypes (vdx/mdvqs.py).                      */
int vdx_frame_stats_u8(const void* frames, size_t frame_pitch, int row_pitch, int F, int H, int W, uint32_t* hist,
                       uint64_t* absdiff, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Farneback dense optical flow, batched over the frame pairs of a clip, and the two numbers built on it
 *   InferNet/template/validator/scoring.py:311-339            TC = mean over consecutive pairs of mean |Farneback flow|
 *   Distribution/strategies/fsdp_chunked_coherent.py:236-246  flow_err = mean |remap(prev, flow) - next| at chunk boundaries
 * (csrc/flow.hip; vdx/flow.py).  The algorithm is vdx/compat/cv2_shim.py's calcOpticalFlowFarneback stage by stage
 * (cv2_shim.py:99-182; parameters 0.5, levels, 15, iterations, 5, 1.2, 0), which stands in for cv2's where OpenCV is not
 * installed: the GPU path is pinned against that shim, the shim against OpenCV is not.  fp32 planes in memory; fp64 arithmetic
 * inside polyexp and update (nearly singular 2 x 2 systems along straight edges), fp32 elsewhere; fixed summation
 * orders, no floating-point atomics: the same bits on every run and for every batch size.  Images are fp32 [n][H][W],
 * flows fp32 [P][H][W][2] (x, y), both packed.
 * ---------------------------------------------------------------------------------------- */
/* cv2.cvtColor(frame, COLOR_RGB2GRAY) (scoring.py:319-327 as vdx/mdvqs.py states it; bgr = 0) or COLOR_BGR2GRAY applied to
 * the same bytes (fsdp_chunked_coherent.py:238-239 / vdx/metrics.py:59; bgr = 1: channel 0 takes the blue weight) of F uint8
 * frames (pitches in bytes), as fp32: (4899 R + 9617 G + 1868 B + 8192) >> 14.                                        */
int vdx_flow_grey_u8(const void* frames, size_t frame_pitch, int row_pitch, int F, int H, int W, int bgr, float* out,
                     vdx_stream_t stream);
/* scipy.ndimage.correlate1d(.., mode="mirror") along axis 0 (rows) or 1 (columns) of n_img images: one pass of the pyramid's
 * gaussian_filter (cv2_shim.py:170-172).  taps: fp32 [2 radius + 1] on the device (vdx/flow.py gaussian_taps).           */
int vdx_flow_corr1d_f32(const float* in, float* out, int n_img, int H, int W, const float* taps, int radius, int axis,
                        vdx_stream_t stream);
/* _resize_linear (cv2_shim.py:55-67): bilinear, src = (dst + 0.5) Hi / Ho - 0.5 clipped to the image, evaluated in exact
 * integer arithmetic; in [n][Hi][Wi][C] -> out [n][Ho][Wo][C], C = 1 (pyramid level, :171-172) or 2 (the flow carried to the
 * next level, :178), times mul (1, or 1 / pyr_scale = 2 for the flow).                                                 */
int vdx_flow_resize_f32(const float* in, int n_img, int Hi, int Wi, int C, float* out, int Ho, int Wo, float mul,
                        vdx_stream_t stream);
/* _poly_exp (cv2_shim.py:99-118) with poly_n = 5 of n_img images -> out [n][5][H][W] = bx, by, axx, ayy, axy.  taps_host:
 * fp64 [3][11] HOST memory, g, g x, g x^2; inv_g_host: fp64 [5][6] HOST memory, rows 1..5 of inv(G) (both from
 * vdx/flow.py poly_tables); they travel as kernel arguments.  Sums and products are fp64, each result rounded once to fp32. */
int vdx_flow_polyexp_f32(const float* img, int n_img, int H, int W, const double* taps_host, const double* inv_g_host, float* out,
                         vdx_stream_t stream);
/* _update_flow (cv2_shim.py:132-153), box window of 15, for P pairs in one launch: pair p reads the expansions of images
 * p*step and p*step + 1 of R ([..][5][H][W]; step 1: consecutive frames, each expansion serving two pairs; step 2: disjoint
 * pairs) and flow_in[p], and writes flow_out[p] (may not alias flow_in).  The five window products stay in LDS.
 * Samples, products, box sums, determinant and solve are fp64; the flow is rounded once to fp32.                          */
int vdx_flow_update_f32(const float* R, const float* flow_in, float* flow_out, int P, int step, int H, int W,
                        vdx_stream_t stream);
/* scoring.py:329-331: out[p] = sum of |flow[p]| over its n = H*W*2 values (the host divides).  workspace: fp32 [P][64].
 * Two stages of fixed order.                                                                                          */
int vdx_flow_abs_sum_f32(const float* flow, int P, size_t n, float* workspace, float* out, vdx_stream_t stream);
/* fsdp_chunked_coherent.py:241-246 / vdx/metrics.py:61-65 for P pairs: prev = frame p*step, next = frame p*step + 1 of
 * `frames` (uint8 RGB, pitches in bytes); warp = cv2.remap(prev, x + flow_x, y + flow_y, INTER_LINEAR) (cv2_shim.py:70-93:
 * constant-0 border, round half to even, clip), absdiff[p] = sum over all bytes of |warp - next| (zeroed on the stream,
 * integer atomics: exact).  warped: NULL, or uint8 [P][H][W][3] that receives the warped frames.                         */
int vdx_flow_remap_absdiff_u8(const void* frames, size_t frame_pitch, int row_pitch, const float* flow, int P, int step, int H,
                              int W, uint64_t* absdiff, void* warped, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Motion-compensated frame interpolation (no reference counterpart: fsdp_chunked_coherent.py:250-253 writes the generated
 * frames as they are; the job's --interpolate N, vdx/interp.py, csrc/interp.hip).  tests/interp_ref.py states the expression.
 * ------------------------------------------------------------------------------------------ */
/* frames: uint8 RGB [F] (pitches in bytes); fab / fba: fp32 [F-1][H][W][2], the Farneback flows frame i -> i+1 and
 * i+1 -> i (8-byte aligned, never NULL); out: uint8 [(F-1)*N + 1] frames of packed rows, out_frame_pitch >= 3*W*H bytes apart.
 * Output frame i*N is frame i byte for byte; frame i*N + k, k = 1 .. N-1, with t = k/N and a = (N-k)/N, per pixel x:
 *   gA = (t*t)*Fba(x) - (a*t)*Fab(x), gB = (a*a)*Fab(x) - (a*t)*Fba(x)  (a non-finite g: 0, and the side's weight * 1e-6);
 *   S = bilinear sample of the frame at x + g clamped to the frame; v = 1 / (1 + |r|^2), r = the frame's own flow there plus
 *   the other flow where that points (0 for a non-finite |r|^2; * 1e-6 when x + g is outside [-0.5, W-0.5] x [-0.5, H-0.5]);
 *   out = (a*vA*SA + t*vB*SB) / (a*vA + t*vB), the plain a*SA + t*SB when that denominator is not positive, then
 *   floor(out + 0.5) clamped to 0..255.  fp32 without contraction; every gather index is clamped as an integer after the float
 *   was clamped, so no flow value reads outside the frames.  One launch, no atomics: the same bits on every run and for any F.
 * 1 <= N <= 64, 1 <= F <= 65536.                                                                                          */
int vdx_interp_frames_u8(const void* frames, size_t frame_pitch, int row_pitch, const float* fab, const float* fba, int F, int H,
                         int W, int N, void* out, size_t out_frame_pitch, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Full-reference comparison of two uint8 RGB clips of one shape: SSE (PSNR), SSIM, MS-SSIM (nothing in the reference: it never
 * holds two clips; vdx/compare.py, csrc/compare.hip).  tests/compare_ref.py states the definition: every R, G, B plane on its
 * own, the 11-tap Gaussian window (sigma 1.5) as a valid correlation, C1 = (0.01*255)^2, C2 = (0.03*255)^2, a 2x2 mean between
 * the five scales.  fp64 between the fp32 samples and the fp64 results, no mul-add contraction, fixed-order sums, no atomics:
 * the same bits on every run, for any number of frames per call, and with the two clips exchanged.
 * ------------------------------------------------------------------------------------------ */
/* Blocks (16 x 32 tiles of the (H-10) x (W-10) map of window positions) per plane; 0 unless H, W >= 11 and H*W < 2^28.      */
int vdx_compare_tiles(int H, int W);
/* One scale of all 3 F plane pairs of uint8 RGB frames a, b (pitches in bytes).  taps: float64 [11] in HOST memory, read
 * before the call returns.  partials: fp64 [3F][tiles][2], every block's sum of ssim and of cs over its valid positions;
 * sse_partials: uint64 [3F][tiles], every block's sum of (a - b)^2 over the bytes it owns (each byte of a plane has one
 * owner).  F <= 21845.  Replaces nothing in the reference.                                                               */
int vdx_compare_ssim_scale_u8(const void* a, size_t a_frame_pitch, int a_row_pitch, const void* b, size_t b_frame_pitch,
                              int b_row_pitch, int F, int H, int W, const double* taps, double* partials, uint64_t* sse_partials,
                              vdx_stream_t stream);
/* The same for packed fp32 planes [n_planes][H][W] (scales 1..4); no byte sums.  Replaces nothing in the reference.        */
int vdx_compare_ssim_scale_f32(const float* a, const float* b, int n_planes, int H, int W, const double* taps, double* partials,
                               vdx_stream_t stream);
/* 2x2 mean, ((p00 + p01) + (p10 + p11)) * 0.25 in fp32, of every plane of uint8 RGB frames a and (unless NULL, with out_b) b ->
 * packed fp32 planes [3F][H/2][W/2]; an odd last row or column is dropped.  Replaces nothing in the reference.            */
int vdx_compare_down2_u8(const void* a, size_t a_frame_pitch, int a_row_pitch, const void* b, size_t b_frame_pitch, int b_row_pitch,
                         int F, int H, int W, float* out_a, float* out_b, vdx_stream_t stream);
/* The same for packed fp32 planes [n_planes][H][W].  Replaces nothing in the reference.                                   */
int vdx_compare_down2_f32(const float* a, const float* b, int n_planes, int H, int W, float* out_a, float* out_b, vdx_stream_t stream);
/* Per frame f and plane c: the n_tiles partials summed in a fixed order over `count` (the positions of a plane) ->
 * means[f][c][scale][0..1] = mean ssim, mean cs (means: fp64 [F][3][5][2]; the other scales are left alone); with
 * sse_partials, sse[f] = the exact sum of (a - b)^2 over the frame's 3 H W bytes (uint64 [F]).  Replaces nothing in the
 * reference.                                                                                                             */
int vdx_compare_finalize(const double* partials, const uint64_t* sse_partials, int F, int n_tiles, double count, int scale,
                         double* means, uint64_t* sse, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * FreeInit's frequency mix (Wu et al. 2023; diffusers' free_init_utils, unpinned) for n_vol = B*C independent volumes of
 * extent (T, h, w) (nothing in the reference: fsdp_chunked_coherent.py:180-182 samples once from white noise; the job's
 * --free_init N, vdx/freeinit.py, csrc/freeinit.hip).  tests/freeinit_ref.py states the definition:
 *   out = fp16( Re ifftn( ifftshift( fftshift(fftn(z_t)) H + fftshift(fftn(eta)) (1 - H) ) ) )   over (T, h, w), in fp32,
 * computed as eta + Re IDFT3( ifftshift(H) . DFT3(z_t - eta) ) / (T h w) with separable direct DFTs in fp64 (fp32 sums miss
 * the fp16 rounding of results near zero, where fp16's spacing is 6e-8), one sum per output in a fixed order, no atomics: the same bits on every run, for any n_vol and wherever in the batch a volume lies.
 * No index or branch depends on the data.  Each of T, h, w in 1..512 (any factorisation), n_vol*T*h*w <= 2^30.
 * ------------------------------------------------------------------------------------------ */
/* Bytes of workspace (one complex fp64 per element); 0 for sizes the kernels do not take.                              */
size_t vdx_freeinit_workspace(int n_vol, int T, int h, int w);
/* z_t: fp16 [n_vol][T][h][w]; eta: fp32 of that shape; filt: fp32 [T][h][w], H in fftshift-ed coordinates (the ifftshift is
 * an index computation in the kernel); tw_t, tw_h, tw_w: fp64 [N][2] on the device for N = T, h, w, entry j =
 * (cos(2 pi j / N), -sin(2 pi j / N)) evaluated in float64 on the host (indexed by (k n) mod N kept in integers); workspace:
 * vdx_freeinit_workspace bytes, 16-byte aligned like the tables; out: fp16 [n_vol][T][h][w], may not alias z_t's memory
 * only in part (out == z_t is allowed: z_t is consumed by the first launch).  Five launches (three when h == 1).          */
int vdx_freeinit_mix_f16(const void* z_t, const float* eta, const float* filt, const double* tw_t, const double* tw_h,
                         const double* tw_w, int n_vol, int T, int h, int w, void* workspace, size_t workspace_bytes, void* out,
                         vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * FreeU (Si et al. 2023; diffusers' enable_freeu(s1, s2, b1, b2), unpinned) on the UNet's rows [n_img][H W][C] fp16 (nothing
 * in the reference: it never touches the up path; UNet3DConditionModel.enable_freeu, the job's --freeu, csrc/freeu.hip).
 * tests/freeu_ref.py states the definition.  No atomics, one fixed summation order per plane: the same bits on every run and
 * for any n_img.  No index or branch depends on the data: NaN and inf stay inside their plane.
 * ------------------------------------------------------------------------------------------ */
/* The skip filter, diffusers' fourier_filter(threshold = 1, scale = s), per image and channel plane (H, W):
 *   out = fp16( Re ifft2( ifftshift( fftshift(fft2(x)) M ) ) ),   M = 1 except M[H/2-1 : H/2+1, W/2-1 : W/2+1] = s
 * computed as x + (s - 1) / (H W) Re sum X(ky, kx) e^{+2 pi i (ky y / H + kx x / W)} over ky in {0, H - 1}, kx in {0, W - 1}
 * (one frequency on an axis of length 1) with the at most four coefficients X summed in fp64, the correction added in fp64
 * and one rounding to fp16; an element whose fp64 result equals its input keeps its bits (s = 1: the identity).
 * x, out: fp16 rows of stride ldx, ldo >= C elements, image i owns rows [i H W, (i + 1) H W); out == x is allowed, any other
 * overlap is not.  tw_h, tw_w: fp64 [N][2] on the device for N = H, W, entry j = (cos(2 pi j / N), -sin(2 pi j / N))
 * evaluated in float64 on the host, 16-byte aligned.  Any n_img, H, W, C >= 1; s finite.  One launch.                      */
int vdx_freeu_filter_f16(const void* x, int ldx, const double* tw_h, const double* tw_w, int n_img, int H, int W, int C, double s,
                         void* out, int ldo, vdx_stream_t stream);
/* The backbone scale, in place: x[r][c] = fp16(fp32(x[r][c]) fp32(b)) for c < C / 2 of every row (torch's half-by-scalar
 * multiply); channels >= C / 2 are not touched.  x: fp16 rows of stride ld >= C; b finite and positive.  One launch, none
 * for C = 1.                                                                                                              */
int vdx_freeu_scale_f16(void* x, int ld, size_t rows, int C, float b, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Token merging (Bolya & Hoffman, "Token Merging for Stable Diffusion", CVPRW 2023; the tomesd package's
 * bipartite_soft_matching_random2d, unpinned) around a spatial self-attention, on rows [n_img][S][C] fp16 (nothing in the
 * reference; UNet3DConditionModel.enable_tome, the job's --tome, vdx/tome.py, csrc/tome.hip).  tests/tome_ref.py states the
 * definition.  The S tokens of an image are partitioned on the host into n_dst destinations and n_src = S - n_dst sources
 * (tables of token indices, ascending, shared by all images).  Per image: every source finds its most similar destination
 * (match); the r sources with the largest similarity are merged into it (select); a tensor's merged layout has
 * S' = S - r rows, first the unmerged sources in ascending token index, then the destinations (merge); after the attention
 * every token reads its row back (unmerge).  No float atomics; a result depends on its own image alone and is the same on
 * every run and for any n_img.  Every index read from a device buffer is clamped to its range before it addresses anything.
 * "The same on every run" holds for tables that are a partition (every token once, as vdx/tome.py builds them): with
 * caller-made tables that name a token twice, several writers meet in slot[] and which one stays is not defined; every
 * value is still in range and nothing faults.
 * ------------------------------------------------------------------------------------------ */
typedef struct vdx_tome_args {
    const int32_t* src_idx;  /* [n_src] token index of source i, in [0, S)                                          */
    const int32_t* dst_idx;  /* [n_dst] token index of destination j                                                */
    float* inv;              /* [n_img][S] match: workspace, 1 / sqrt(sum_c fp32(t)^2) of every token               */
    float* node_max;         /* [n_img][n_src] match out, select in: the largest score of source i (-inf: none)     */
    int32_t* node_idx;       /* [n_img][n_src] match out, select in: its j, the lowest of equal ones, in [0, n_dst) */
    int32_t* slot;           /* [n_img][S] select out: the merged row token p reads back from, in [0, S - r)        */
    int32_t* off;            /* [n_img][n_dst + 1] select out: CSR offsets into items, off[n_dst] = r               */
    int32_t* items;          /* [n_img][r] select out: the merged sources of each destination, ascending i          */
    int32_t n_img, S, n_src, n_dst;  /* n_src + n_dst = S, each at least 1                                          */
    int32_t r;               /* sources merged per image, 1 <= r <= n_src                                           */
    int32_t C;               /* channels of the rows handed to match / merge / unmerge                              */
} vdx_tome_args;
/* score[i][j] = (sum_c t[src i][c] t[dst j][c]) inv[src i] inv[dst j], fp32 accumulation on MFMA; node_max / node_idx are its
 * maximum over j and the lowest such j.  A NaN score never wins; a source with no winning score keeps (-inf, 0).  The score
 * matrix is never stored.  t: rows of stride ld >= C (a multiple of 8), 16-byte aligned; C a multiple of 64, at most 1280.
 * Two launches (the inverse norms, the match).                                                                          */
int vdx_tome_match_f16(const vdx_tome_args* a, const void* t, int ld, vdx_stream_t stream);
/* Bytes of LDS the select needs for (n_src, n_dst); it refuses plans above 160 KiB - 256.                               */
size_t vdx_tome_select_lds(int n_src, int n_dst);
/* Order the sources by node_max descending (ties: lower i; NaN below every number; -0 = +0); the first r are merged into
 * destination clamp(node_idx[i]).  Writes slot, off and items.  One workgroup per image, one launch.                    */
int vdx_tome_select(const vdx_tome_args* a, vdx_stream_t stream);
/* out rows [n_img][S - r][C]: an unmerged source's row is y's, bit for bit; destination j's row is
 * fp16((fp32(y[dst j]) + sum fp32(y[src i])) / fp32(1 + count)) over its items in ascending i, each add rounded to fp32.
 * C a multiple of 8; out must not overlap y.  One launch.                                                               */
int vdx_tome_merge_f16(const vdx_tome_args* a, const void* y, int ldy, void* out, int ldo, vdx_stream_t stream);
/* out[p] = fp16(fp32(x[slot[p]]) + fp32(t[p])) for every token p of every image; x: the merged rows [n_img][S - r][C],
 * t, out: [n_img][S][C]; out may be t, it must not overlap x.  One launch.                                              */
int vdx_tome_unmerge_add_f16(const vdx_tome_args* a, const void* x, int ldx, const void* t, int ldt, void* out, int ldo,
                             vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Prompt travel: per-frame text through every cross-attention (nothing in the reference: it encodes one prompt per job;
 * AnimateDiff-Evolved's batch prompt schedule, unpinned; vdx/travel.py, the job's --prompt_at, csrc/travel.hip).
 * tests/travel_ref.py states the schedule and the blend.  No atomics: the same bits on every run.
 * ------------------------------------------------------------------------------------------ */
/* One window's UNet text in one launch.  keys: fp16 (n_keys, N, D); uncond: fp16 (N, D); lo, hi: int32 [T], w: fp32 [T] on the
 * device, the plan of vdx/travel.py `travel_plan`; out: fp16 (2, L, N, D).  out[0][f] = uncond; out[1][f], for the clip frame
 * t = s + f d (with `ring`, t - T where that is >= T), is keys[lo[t]]'s bits where w[t] == 0 or lo[t] == hi[t], else
 *   fp16( fp32( fp32(1 - w[t]) fp32(keys[lo[t]]) ) + fp32( w[t] fp32(keys[hi[t]]) ) )
 * with every product and the sum rounded on its own.  lo and hi are clamped to [0, n_keys) on the device before use.
 * 0 <= s < T, L >= 1, d >= 1, s + (L - 1) d < T (with `ring`: < 2 T).  16 bytes per lane where D % 8 == 0 (keys, uncond and
 * out then 16-byte aligned), else one element.                                                                            */
int vdx_text_travel_f16(const void* keys, int n_keys, const void* uncond, const int32_t* lo, const int32_t* hi, const float* w,
                        int T, int s, int L, int d, int ring, int N, int D, void* out, vdx_stream_t stream);
/* vdx/packing.py pack_k5_kv as one launch: k_rows fp16 [n_items text_pad][inner] (stride ldk), vt fp16 [inner][n_items
 * text_pad] (stride ldvt) -> out [n_items][heads][3 * 4096] fp16, K5's key / value blobs (vdx_cross_attn_block_kv_bytes each),
 * the zeroed rest of the third unit included; the first 80 keys of every item are read.  Supported where
 * vdx_cross_attn_block_supported(inner, .) is; text_pad >= 80 and a multiple of 4, ldk and ldvt multiples of 4, k_rows and
 * vt 8-byte, out 16-byte aligned.  Every index is a function of the thread's position only.                               */
int vdx_cross_attn_block_pack_kv_f16(const void* k_rows, int ldk, const void* vt, int ldvt, int n_items, int text_pad, int inner,
                                     void* out, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Regional prompts: per-region text through every spatial cross-attention (nothing in the reference: it conditions every
 * pixel of a frame on one prompt; "attention couple" / regional conditioning of ComfyUI and AnimateDiff-Evolved, unpinned;
 * vdx/region.py, the job's --region, csrc/region.hip).  tests/region_ref.py states the weights and the blend.  No atomics:
 * the same bits on every run.
 * ------------------------------------------------------------------------------------------ */
/* The per-pixel blend of one window's cross-attention sub-block results.  in: a HOST array of n_in device pointers
 * (1 <= n_in <= 8: the base text and at most 7 regions), in[j] fp16 [L S][C] contiguous, the sub-block evaluated with text j,
 * or NULL for a text that was not launched (no weight on any cell of the window); table: fp32 [T][S][n_in] on the device, the
 * level's weights of vdx/region.py `region_plan`; out: fp16 [L S][C], which may be in[0] (or any one input).  Row (f, p) is the clip frame
 * tau = s + f d (with `ring`, tau - T where that is >= T), clamped to [0, T).  out[row] is in[j][row]'s bits for the first j
 * with table[tau][p][j] == 1.0f, else
 *   fp16( ... fp32( fp32( w_a fp32(in[a][row]) ) + fp32( w_b fp32(in[b][row]) ) ) ... )
 * over the j with a non-zero weight (and a non-NULL input) in ascending order, every product and every sum rounded on its own;
 * a zero-weight input is not read for that row.  0 <= s < T, L >= 1, d >= 1, s + (L - 1) d < T (with `ring`: < 2 T).
 * A block owns whole rows (groups of consecutive rows, never a part of one).  16 bytes per lane where C % 8 == 0 (inputs and
 * out then 16-byte aligned), 8 where C % 4 == 0 (8-byte aligned), else one element.                                                                                                                  */
int vdx_region_blend_f16(const void* const* in, int n_in, const float* table, int T, int s, int L, int d, int ring, int S, int C,
                         void* out, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LoRA adapters, merged into the weights in the diffusers layout before the loader packs them (nothing in the reference: it
 * loads one checkpoint; diffusers' load_lora_weights / set_adapters / fuse_lora and peft's merge, unpinned; vdx/lora.py, the
 * job's --lora, csrc/lora.hip).  tests/lora_ref.py states the expression.  No atomics: the same bits on every run and rank.
 * ------------------------------------------------------------------------------------------ */
/* out = W + sum_a s_a up_a down_a on one weight.  W, out: fp16 [n_out][n_in] contiguous (a conv weight flattened over its input
 * axes), out may be W.  up, down, rank, scale: HOST arrays of A entries (1 <= A <= 8): up[a] fp32 [n_out][rank[a]] and down[a]
 * fp32 [rank[a]][n_in] on the device, contiguous, 1 <= rank[a] <= 512, scale[a] finite.  Per element, every product and every
 * sum rounded to fp32 on its own:
 *   acc_a = 0;  for r ascending: acc_a = acc_a + up_a[o][r] down_a[r][i];     d = 0;  for a ascending: d = d + scale[a] acc_a;
 *   out[o][i] = fp16_rn( fp32(W[o][i]) + d )
 * VALU fp32, not MFMA: the order of summation is part of the contract.  A block owns a 32 x 256 tile of W and stages up and
 * down through LDS 32 ranks at a time.  Accesses along n_in are 16 bytes where n_in % 8 == 0 and W, out and every down are
 * 16-byte aligned, 8 bytes where n_in % 4 == 0 and they are 8-byte aligned, else one element (fp16 2-byte, fp32 4-byte
 * aligned).  Any n_out, n_in >= 1.                                                                                          */
int vdx_lora_merge_f16(const void* W, int n_out, int n_in, int A, const float* const* up, const float* const* down,
                       const int32_t* rank, const float* scale, void* out, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Prompt emphasis: `(text:1.3)` weights on the text encoder's output, with mean restoration (nothing in the reference: it
 * encodes one plain prompt; the AUTOMATIC1111 web UI's prompt emphasis, diffusers' lpw_stable_diffusion and compel, unpinned;
 * vdx/prompt.py, the job's --prompt_syntax, csrc/prompt.hip).  tests/prompt_ref.py states the expression.  No atomics: the
 * same bits on every run and rank.
 * ------------------------------------------------------------------------------------------ */
/* z: fp16 [n_seq][n_tok][D] contiguous, the CLIP last hidden state, one sequence per (text, 75-token chunk); w: fp32
 * [n_seq][n_tok] on the device; out: fp16 like z, which may be z.  1 <= n_tok <= 77, 1 <= D <= 2^20.  Per sequence, every
 * product rounded on its own:
 *   y = fp16( fp32(z) w[tok] );   m0 = sum z, m1 = sum y (fp64, over the sequence's n_tok D elements);   r = fp32( m0 / m1 ),
 *   the quotient in fp64;   out = fp16( fp32(y) r )
 * One block of 1024 lanes owns one sequence and passes over it twice.  The sums' order: lane l adds the elements of its
 * accesses l, l + 1024, ... (V elements each, ascending) to its partials, and the partials meet in a binary tree, p[l] += p[l + h]
 * for h = 512, ..., 1.  V = 8 where D % 8 == 0 and z and out are 16-byte aligned, 4 where D % 4 == 0 and they are 8-byte aligned,
 * else 1.  No branch on data: m1 = 0, a NaN or an infinity give what the lines give, in that sequence only.  The caller (vdx/ops.py
 * `prompt_weight`) refuses a non-finite w and does not pass a sequence whose weights are all 1.0.                              */
int vdx_prompt_weight_f16(const void* z, const float* w, void* out, int n_seq, int n_tok, int D, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Motion-JPEG decode of a whole clip: the read side of the validator's cv2.VideoCapture(video_path)
 *   InferNet/template/validator/scoring.py:16, :110, :230, :272, :314   every score opens the FILE the miner sent
 *   vdx/compat/cv2_shim.py:199-289                                      the writer whose .mp4 this reads back
 * (csrc/mjpeg.hip; vdx/video.py parses the container and the JPEG headers on the host).  Baseline sequential JPEG, 8 bit;
 * `layout` 0: one component, 1: three components 1x1 (4:4:4), 2: 2x2, 1x1, 1x1 (4:2:0).  All frames of a call share W, H and
 * layout.  Integers only and no atomics: the same bits on every run and for any number of frames per call, and bit for bit
 * libjpeg's decode (slow-integer IDCT, h2v2 fancy upsampling, 16-bit fixed-point YCbCr -> RGB), i.e. Pillow's, for every
 * frame whose coefficients lie in the range 8-bit samples produce; stage 2 flags the others (decoders disagree on them).
 * The three stages share `workspace` (vdx_mjpeg_workspace bytes, 16-byte aligned) and are enqueued in this order.
 * ---------------------------------------------------------------------------------------- */
/* Bytes of workspace for F frames of W x H (int16 coefficients [F][block][64], then uint8 component planes at the padded MCU
 * extent); 0 for arguments the decoder does not take.                                                                  */
size_t vdx_mjpeg_workspace(int F, int W, int H, int layout);
/* Stage 1, Huffman decode, one lane per segment.  data: the entropy-coded bytes of all frames, nbytes (% 4 == 0) of them.
 * segs: int32 [nseg][4] = byte begin, byte end, first MCU, MCU count of every restart interval (a frame without DRI is one
 * segment); seg_off: int32 [F + 1], frame f owns rows seg_off[f] .. seg_off[f + 1], at most max_segs_per_frame of them.
 * huff: per frame four tables (DC 0, DC 1, AC 0, AC 1) of 384 words each: 512 uint16 entries (length << 8 | symbol) for a
 * 9-bit lookahead, then int32 maxcode[17], int32 valoff[17] (indexed by code length), the 256 symbols, padding.
 * sel: int32 [F][3], component c decodes with DC table sel & 1 and AC table (sel >> 4) & 1.  FF 00 is unstuffed here, the
 * DC prediction restarts with each segment.  err: uint32 [nseg], 0 or (code | MCU within the segment << 8) with code
 * 1: the data ended inside a symbol, 2: a coefficient index past 63, 3: no Huffman code matches, 4: a DC size above 15,
 * 5: a segment row outside the clip; a lane stops at its first error.  No access depends on unchecked stream bytes.     */
int vdx_mjpeg_entropy(const void* data, size_t nbytes, const int32_t* seg_off, const int32_t* segs, int nseg,
                      int max_segs_per_frame, const void* huff, const int32_t* sel, int F, int W, int H, int layout,
                      void* workspace, uint32_t* err, vdx_stream_t stream);
/* Stage 2: coefficient * quant (uint16 [F][3][64] in natural order, per component), the 8x8 slow-integer IDCT in int32
 * (13-bit constants, 2 pass-1 bits), + 128, clamp -> the component planes.  flags: uint32 [F], zeroed here on the stream;
 * word f becomes 1 when frame f holds coefficients outside the range 8-bit samples produce (a dequantised product or a
 * pass-1 value beyond the bounds in csrc/mjpeg.hip, or a sample before the range limit outside [-512, 511]): there libjpeg,
 * libjpeg-turbo and this arithmetic return different pixels, and the caller refuses the frame.                          */
int vdx_mjpeg_idct(const void* quant_u16, int F, int W, int H, int layout, void* workspace, uint32_t* flags,
                   vdx_stream_t stream);
/* Stage 3: 4:2:0 chroma through the h2v2 fancy upsampling (edges replicate at ceil(W/2) x ceil(H/2)), YCbCr -> RGB, crop:
 * out uint8 (F, H, W, 3) RGB packed, or (F, H, W) for layout 0.  4-byte aligned.  4:2:0 needs W >= 5.                   */
int vdx_mjpeg_color(const void* workspace, int F, int W, int H, int layout, void* out, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Motion-JPEG encode of a whole clip: the write side of the job's cv2.VideoWriter
 *   fsdp_chunked_coherent.py:250-253            the reference writes the decoded frames to an .mp4
 *   vdx/compat/cv2_shim.py VideoWriter.write    the host path (Pillow, quality 92) whose bytes this reproduces
 * (csrc/mjpeg_enc.hip; vdx/video.py builds the header and the container on the host).  Baseline JPEG with the standard
 * Huffman tables; `layout` 0: grey, 2: 4:2:0 (as above; 4:4:4 is not written).  Integers only; the only atomics are ORs into
 * zeroed words: the same bytes on every run and for any number of frames per call, and byte for byte libjpeg's (Pillow's)
 * for the same frames, every width and height included.  The four stages share `workspace` (vdx_mjpeg_enc_workspace bytes,
 * 16-byte aligned) and are enqueued in this order; the coefficients and planes lie where vdx_mjpeg_workspace puts them.
 * ---------------------------------------------------------------------------------------- */
/* Bytes of workspace for F frames of W x H; 0 for arguments the encoder does not take.                                  */
size_t vdx_mjpeg_enc_workspace(int F, int W, int H, int layout);
/* offsets[6] (host memory): byte offsets in the workspace of the int16 coefficients [F][block][64], the uint8 component planes,
 * the uint32 bit offsets [F][block] (scan order), the uint32 bits per restart interval [F][MCUs], the uint32 byte offsets of
 * the slots [F][block] and the unstuffed bit stream (208 bytes per block, 32-bit words, first bit in the MSB).           */
int vdx_mjpeg_enc_offsets(int F, int W, int H, int layout, size_t* offsets);
/* Stage 1.  frames: uint8 (F, H, W, 3) RGB packed (layout 2) or (F, H, W) (layout 0).  libjpeg's 16-bit fixed-point RGB ->
 * YCbCr, the h2v2 downsample (2x2 sum + 1, 2, 1, 2, ... along the columns, >> 2), edges replicated as libjpeg does: columns
 * and a cut row pair at full resolution, the chroma rows below ceil(H / 2) from the last downsampled row.               */
int vdx_mjpeg_enc_color(const void* frames, int F, int W, int H, int layout, void* workspace, vdx_stream_t stream);
/* Stage 2.  quant: uint16 [2][64] (luma, chroma; natural order, 1..255).  - 128, the 8x8 slow-integer forward DCT (13-bit
 * constants, 2 pass-1 bits, rows then columns), sign(v) (|v| + (8q >> 1)) / 8q with an exact quotient; luma blocks wholly
 * outside ceil(extent / 8) blocks are libjpeg's dummy blocks (AC zero, DC of the block before them in the MCU).          */
int vdx_mjpeg_enc_fdct(const void* quant_u16, int F, int W, int H, int layout, void* workspace, vdx_stream_t stream);
/* Stage 3.  tables: uint32 [2][272], per table id 16 DC words (by size) and 256 AC words (by run << 4 | size) of
 * length << 16 | code.  restart_interval: MCUs per restart interval, 0 for none.  Counts the bits of every block, scans them
 * per interval, emits them (intervals padded to a byte with 1-bits), counts the bytes after FF -> FF 00 stuffing and scans
 * those.  lengths: int32 [F] (device), the bytes of every frame's file: header_bytes + entropy data + RSTn markers + EOI. */
int vdx_mjpeg_enc_entropy(const void* tables, int F, int W, int H, int layout, int restart_interval, int header_bytes,
                          void* workspace, int32_t* lengths, vdx_stream_t stream);
/* Stage 4.  header: the header_bytes bytes every frame starts with (device).  out: the frames' files back to back, frame f
 * at the sum of lengths[0 .. f); out_bytes: the size of `out`, past which nothing is stored.                             */
int vdx_mjpeg_enc_pack(const void* header, int header_bytes, int F, int W, int H, int layout, int restart_interval,
                       const void* workspace, const int32_t* lengths, void* out, size_t out_bytes, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Animated GIF89a of a whole clip (no reference counterpart: the reference leaves through an .mp4 alone)
 * (csrc/gif.hip; vdx/gif.py cuts the palette and writes the headers on the host; tests/gif_ref.py is the definition).
 * One global colour table of at most 256 entries for the clip, an ordered dither, and LZW with a minimum code size of 8 over
 * independent strips of rows.  Integers only; the only atomics are integer adds (the histogram) and ORs into zeroed words (the
 * strips' bits): the same bytes on every run and for any number of frames per call.  u8 frames are (T, H, W, 3) RGB with
 * packed pixels, frame_pitch and row_pitch in bytes; T * H * W < 2^32, H and W in 1..65535.
 * ---------------------------------------------------------------------------------------- */
/* Stage 1.  hist: uint32 [32768] (device), zeroed here on the stream, then the pixels of the whole clip per 5-5-5 bin
 * (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3).  Plain global integer atomics (a thread adds a run of equal bins at once): the
 * counts are exact.                                                                                                     */
int vdx_gif_hist_u8(const void* frames, size_t frame_pitch, int row_pitch, int T, int H, int W, uint32_t* hist,
                    vdx_stream_t stream);
/* Stage 3.  palette: uint8 [n][3] (device), n in 1..256.  lut: uint8 [32768], for every bin the entry nearest to the bin's
 * centre (v << 3 | 4 per channel) by integer squared distance, a tie to the lowest index.  One launch, the palette in LDS. */
int vdx_gif_lut(const void* palette, int n, void* lut, vdx_stream_t stream);
/* Stage 4.  dither 1 (bayer): v' = clamp(v + D[y & 7][x & 7], 0, 255) per channel with D = ((B8 * 8 + 4) >> 6) - 4 in -4..3, B8
 * the standard 8x8 Bayer matrix; dither 0: v' = v.  out: uint8 (T, H, W) contiguous = lut[bin(v')].  A pixel's index depends
 * on that pixel, its position in its frame and the lut alone.                                                           */
int vdx_gif_index_u8(const void* frames, size_t frame_pitch, int row_pitch, int T, int H, int W, const void* lut, int dither,
                     void* out, vdx_stream_t stream);
/* Bytes of workspace of stages 5 and 6 for T frames of W x H cut into strips of strip_rows rows (>= H: one strip); 0 for
 * arguments the encoder does not take (a frame whose strips' slots reach 2^32 bits among them).                        */
size_t vdx_gif_lzw_workspace(int T, int H, int W, int strip_rows);
/* offsets[8] (host memory): byte offsets in the workspace of the uint32 bits of every strip [T][strips], their uint32 bit
 * offsets in the frame [T][strips], the uint32 bits of every frame [T], the strips' slots uint32 [T][strips][slot_words] and
 * the frames' streams uint32 [T][strips * slot_words] (bit i of a stream is bit i & 31 of word i >> 5) and the uint64 byte
 * offsets of the frames' sub-blocks in the packed output [T]; then the strips of a frame and slot_words.  The slot bound: a strip of n pixels emits at most n data codes (each consumes a pixel), one CLEAR
 * per 3838 of them (what the table takes between resets), its opening CLEAR and its closing CLEAR / EOI, at most 12 bits
 * each: slot_words = ceil(12 (n + n / 3838 + 3) / 32), n = min(strip_rows, H) * W.                                      */
int vdx_gif_lzw_offsets(int T, int H, int W, int strip_rows, size_t* offsets);
/* Stage 5.  idx: uint8 (T, H, W) contiguous.  Strip s of a frame is rows [s * strip_rows, ...); its codes are [CLEAR, for
 * the frame's first strip] data codes, then CLEAR, or EOI for the frame's last strip, from an empty table at width 9: no
 * strip's bits depend on another strip.  CLEAR = 256, EOI = 257; the table holds 4096 codes and a full table is answered by
 * CLEAR; the width grows when the next free code exceeds 1 << width, up to 12, and the closing code is written at the width
 * after the entry the decoder adds for the last data code.  One strip per wave, the dictionary an open-addressed table of
 * 8192 words in LDS (33 024 bytes per workgroup with the staged pixels: four strips per compute unit); every probe sequence is bounded by the table's slots, the pixel loop by the strip's pixels.  The strips'
 * bits are concatenated per frame, LSB first.  lengths: int32 [T] (device): the bytes of every frame's data sub-blocks,
 * L + ceil(L / 255) + 1 for L stream bytes; their exclusive sums go to the workspace for stage 6.                        */
int vdx_gif_lzw(const void* idx, int T, int H, int W, int strip_rows, void* workspace, int32_t* lengths, vdx_stream_t stream);
/* Stage 6, on the workspace stage 5 left.  out: every frame's stream as data sub-blocks (a length byte, up to 255 bytes, ..., a
 * 00 terminator), frame f at the sum of stage 5's lengths[0 .. f); out_bytes: the size of `out`, past which nothing is stored. */
int vdx_gif_pack(const void* workspace, int T, int H, int W, int strip_rows, void* out, size_t out_bytes, vdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Portable seeded noise "philox4x32-10/v1" (no reference counterpart: fsdp_chunked_coherent.py:180-182 is torch's stream, which
 * depends on the device and the torch build) (csrc/noise.hip; vdx/noise.py; tests/noise_ref.py is the definition).
 * Element i of stream `stream` under `seed` is a pure function of (seed, stream, i), i the C-order linear index in the LOGICAL
 * tensor `shape` (ndim 1..5 axes, fewer than 2^63 elements): Philox4x32-10 with key (seed lo, seed hi) and counter (q lo, q hi,
 * stream lo, stream hi), q = i >> 2; Box-Muller in fp64 on the block's word pairs with the file's own ln, sin and cos (stated
 * sequences of fp64 + - * / sqrt: the same bits on every device).  out: the box [start, start + extent) of the logical tensor,
 * contiguous, of the box's shape, 16-byte aligned: fp32(n), or fp16(fp32(fp16(n)) * sigma).  The same bits for the whole tensor or
 * any box of it; no atomics, no state.  Refused: a box that leaves the shape, an extent < 1, 2^63 elements or more, a sigma
 * that is not finite.  seed and stream are 64-bit values passed as size_t.
 * ---------------------------------------------------------------------------------------- */
int vdx_noise_f16(size_t seed, size_t stream, int ndim, const size_t* shape, const size_t* start, const size_t* extent, float sigma,
                  void* out, vdx_stream_t stream_handle);
int vdx_noise_f32(size_t seed, size_t stream, int ndim, const size_t* shape, const size_t* start, const size_t* extent, void* out,
                  vdx_stream_t stream_handle);
/* Stochastic sampling: DDIM with eta > 0 (diffusers `DDIMScheduler.step(eta=)`) and SDE-DPM-Solver++ 2M (diffusers
 * `algorithm_type="sde-dpmsolver++"`, A1111's "DPM++ 2M SDE"); restated and unpinned; no reference counterpart, opt-in:
 * vdx/scheduler.py, `DiffuserConfig.eta`; csrc/dpm.hip, csrc/codenoise.hip, csrc/step_noise.h; restated in tests/sde_ref.py.
 * Each entry is its deterministic sibling (the same kernel, chain, alignment and overlap rules: lat_out may be lat / z) run with
 * other host coefficients, followed inside the same kernel by one more link:
 *     lat' = fp16(lat' + fp16(c_n * w))
 * w: what vdx_noise_f16 holds, with sigma 1, under `seed` and `noise_stream` for the LOGICAL tensor (1,C,T,h,w) of the whole clip
 * at the element's place in the clip.  The one-buffer entries take a sample (1,C,L,h,w) that is the frames [s, s + L) of the clip
 * (eps / eps2 shaped alike): two samples that share frames add the same noise to them.  The co-fused entries' sample is the clip.
 *   DDIM, eta in (0, 1]:  std = eta * sqrt(((1-a_prev)/(1-a_t)) * (1 - a_t/a_prev));  dir_coef = sqrt(1 - a_prev - std^2) stands
 *                         where the deterministic entry takes sqrt(1 - a_prev);  c_n = std
 *   SDE-DPM-Solver++:     c_x = (st/s0)*exp(-h),  c_d0 = at*(1 - exp(-2h)),  c_d1 = 0.5*c_d0,  c_n = st*sqrt(1 - exp(-2h));
 *                         x0_prev == NULL: first order.  (The last step, sigma 0, has c_n = 0: callers run the deterministic entry.)
 * 16-byte accesses where L*HW, (T-L)*HW and s*HW are multiples of 8 (a lane then computes two Philox blocks), 8-byte for
 * multiples of 4, else element-wise; the bits do not depend on the width.  One launch; no atomics, no state, no noise buffer.
 * Refused: a c_n that is not finite, frames [s, s + L) that leave [0, T), a clip of 2^63 elements or more, and whatever the
 * deterministic sibling refuses.  seed and noise_stream are 64-bit values passed as size_t.                                      */
int vdx_cfg_ddim_eta_step_f16(const void* eps2, const void* lat, void* lat_out, float guidance, float sqrt_one_minus_at,
                              float sqrt_at, float sqrt_aprev, float dir_coef, float c_n, size_t seed, size_t noise_stream, int C,
                              int T, int HW, int s, int L, vdx_stream_t stream);
int vdx_ddim_eta_step_f16(const void* eps, const void* lat, void* lat_out, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                          float dir_coef, float c_n, size_t seed, size_t noise_stream, int C, int T, int HW, int s, int L,
                          vdx_stream_t stream);
int vdx_cfg_sde_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out, float guidance,
                             float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, float c_n, size_t seed,
                             size_t noise_stream, int C, int T, int HW, int s, int L, vdx_stream_t stream);
int vdx_sde_dpm_step_f16(const void* eps, const void* lat, const void* x0_prev, void* x0_out, void* lat_out, float c_s0,
                         float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, float c_n, size_t seed,
                         size_t noise_stream, int C, int T, int HW, int s, int L, vdx_stream_t stream);
int vdx_cofuse_cfg_ddim_eta_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                     const int* win_start, const int* win_len, int K, const float* wn, void* lat_out, float guidance,
                                     float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float dir_coef, float c_n, size_t seed,
                                     size_t noise_stream, int C, int T, int HW, vdx_stream_t stream);
int vdx_cofuse_cfg_sde_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                    const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev,
                                    void* x0_out, void* lat_out, float guidance, float c_s0, float c_inv_a0, float c_x, float c_d0,
                                    float c_d1, float c_inv_r0, float c_n, size_t seed, size_t noise_stream, int C, int T, int HW,
                                    vdx_stream_t stream);
/* 1 when that box takes the fast form (a lane per Philox block, 8- or 16-byte stores), 0 for the general one (a lane per
 * output), -1 for a box the entries refuse.  The bits do not depend on the form.                                            */
int vdx_noise_form(int ndim, const size_t* shape, const size_t* start, const size_t* extent);

#ifdef __cplusplus
}
#endif
#endif /* VDX_H */
