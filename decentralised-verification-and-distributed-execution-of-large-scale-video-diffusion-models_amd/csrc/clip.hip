// clip.hip — the validator's CLIP prompt-fidelity score (InferNet/template/validator/scoring.py:87-147) on the device:
// the image front end (PIL bilinear resize to 224x224 + ToTensor + ImageNet Normalize, :81-85, :121-122) written straight
// into the patch-GEMM operand, the ViT's embedding + pre-LayerNorm, quick_gelu, and the pooled cosine score (:137-140).
// The contractions of the two towers run on the GEMM / flash-attention kernels (vdx/clip_vision.py, vdx/clip_score.py).
#include "vdx_common.h"

// ---- image front end --------------------------------------------------------------------------------------------
// Pillow's ImagingResample for 8-bit RGB: a horizontal pass, then a vertical pass, each with 22-bit fixed-point
// weights; out = clip8((2^21 + sum px * k) >> 22) and the intermediate image is uint8.  The windows and weights come from
// the host (vdx/ops.py `clip_resize_coeffs`).  One block per (band of output rows, frame): the horizontal pass fills
// LDS with the input rows the band's vertical windows read, resized to 224 columns; the vertical pass reads them back.
#define CLIP_PX 224
#define CLIP_ROW (CLIP_PX * 3)

__device__ __forceinline__ int clip8_22(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void clip_preprocess_kernel(vdx_clip_preprocess_args a) {
    extern __shared__ unsigned char tmp[];                      // [span][224*3] horizontally resized input rows
    const int f = blockIdx.y;
    const int oy0 = blockIdx.x * a.band;
    const int nb = min(a.band, CLIP_PX - oy0);
    const int2* yb = (const int2*)a.y_bounds;
    const int2* xb = (const int2*)a.x_bounds;
    const int iy0 = yb[oy0].x;
    const int nr = min(yb[oy0 + nb - 1].x + yb[oy0 + nb - 1].y - iy0, a.span);   // the host sized span for every band
    const unsigned char* src = (const unsigned char*)a.frames + (size_t)f * a.frame_pitch;
    for (int i = threadIdx.x; i < nr * CLIP_ROW; i += blockDim.x) {
        const int r = i / CLIP_ROW, col = i - r * CLIP_ROW;
        const int ox = col / 3, c = col - ox * 3;
        const unsigned char* row = src + (size_t)min(iy0 + r, a.H - 1) * a.row_pitch + c;
        const int2 w = xb[ox];
        const int n = min(w.y, a.kx);
        const int32_t* k = a.x_coeffs + ox * a.kx;
        int acc = 1 << 21;
        for (int j = 0; j < n; ++j) acc += (int)row[min(w.x + j, a.W - 1) * 3] * k[j];
        tmp[i] = (unsigned char)clip8_22(acc);
    }
    __syncthreads();
    // ToTensor + Normalize (scoring.py:81-85): ((u / 255) - mean) / std in fp32, every step rounded like torch-CPU.  These
    // are ImageNet's statistics, not CLIP's — the reference's choice, kept.
    f16* out = (f16*)a.out;
    const int per_c = nb * CLIP_PX;
    for (int i = threadIdx.x; i < 3 * per_c; i += blockDim.x) {
        const int c = i / per_c, rem = i - c * per_c;
        const int oyl = rem / CLIP_PX, ox = rem - oyl * CLIP_PX, oy = oy0 + oyl;
        const int2 w = yb[oy];
        const int n = min(w.y, a.ky), r0 = w.x - iy0;
        const int32_t* k = a.y_coeffs + oy * a.ky;
        int acc = 1 << 21;
        for (int j = 0; j < n; ++j) {
            const int r = r0 + j;
            if (r >= 0 && r < nr) acc += (int)tmp[r * CLIP_ROW + ox * 3 + c] * k[j];
        }
        const int u = clip8_22(acc);
        const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
        const float stdv = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
        const float v = __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.0f), mean), stdv);
        // patch-GEMM operand: row f*49 + py*7 + px, column c*1024 + ky*32 + kx (= patch_embedding.weight.reshape(768, 3072))
        const size_t orow = (size_t)f * 49 + (oy >> 5) * 7 + (ox >> 5);
        out[orow * a.ldo + c * 1024 + (oy & 31) * 32 + (ox & 31)] = (f16)v;
        if (a.out_u8) ((unsigned char*)a.out_u8)[(((size_t)f * CLIP_PX + oy) * CLIP_PX + ox) * 3 + c] = (unsigned char)u;
    }
}

extern "C" int vdx_clip_preprocess_u8(const vdx_clip_preprocess_args* a, vdx_stream_t stream) {
    VDX_CHECK(a && a->frames && a->x_bounds && a->x_coeffs && a->y_bounds && a->y_coeffs && a->out,
              "clip_preprocess: null pointer");
    VDX_CHECK(a->F > 0 && a->H > 0 && a->W > 0 && a->F <= 65535, "clip_preprocess: F=%d H=%d W=%d", a->F, a->H, a->W);
    VDX_CHECK(a->row_pitch >= 3 * a->W && a->frame_pitch >= (size_t)a->row_pitch * a->H, "clip_preprocess: pitches too small");
    VDX_CHECK(a->kx > 0 && a->ky > 0 && a->band > 0 && a->band <= CLIP_PX && a->span > 0, "clip_preprocess: kx=%d ky=%d band=%d span=%d",
              a->kx, a->ky, a->band, a->span);
    VDX_CHECK(a->ldo >= 3072 && a->ldo % 8 == 0, "clip_preprocess: ldo=%d (needs >= 3072, a multiple of 8)", a->ldo);
    const size_t lds = (size_t)a->span * CLIP_ROW;
    VDX_CHECK(lds <= 65536, "clip_preprocess: a band needs %zu bytes of LDS (> 64 KiB): pick a smaller band", lds);
    dim3 grid((CLIP_PX + a->band - 1) / a->band, a->F);
    hipLaunchKernelGGL(clip_preprocess_kernel, grid, dim3(256), lds, (hipStream_t)stream, *a);
    return vdx_launch_status("vdx_clip_preprocess_u8");
}

// ---- CLIPVisionEmbeddings + pre_layrnorm ------------------------------------------------------------------------
// row f*seq_pad + t of the output: t = 0 the class token, t = 1..P patch t-1 (the patch GEMM's row f*P + t-1), each plus
// position t, then LayerNorm with fp32 statistics; rows P+1..seq_pad-1 are zero (the attention kernel's key padding).
#define EMB_MAXV 16   // D <= 64 * 16
__global__ __launch_bounds__(256) void clip_vision_embed_kernel(const f16* patch, int ldp, const f16* cls, const f16* pos,
                                                                const f16* gamma, const f16* beta, float eps, int F, int P,
                                                                int seq_pad, int D, f16* out, int ldo) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= F * seq_pad) return;
    const int f = row / seq_pad, t = row - f * seq_pad;
    f16* dst = out + (size_t)row * ldo;
    if (t > P) {
        for (int j = lane; j < D; j += 64) dst[j] = (f16)0.f;
        return;
    }
    const f16* srcr = t == 0 ? cls : patch + ((size_t)f * P + t - 1) * ldp;
    const f16* posr = pos + (size_t)t * D;
    float v[EMB_MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < EMB_MAXV; ++i) {
        const int j = lane + 64 * i;
        v[i] = j < D ? (float)srcr[j] + (float)posr[j] : 0.f;
        s += v[i];
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < EMB_MAXV; ++i) {
        const float d = lane + 64 * i < D ? v[i] - mean : 0.f;
        q += d * d;
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < EMB_MAXV; ++i) {
        const int j = lane + 64 * i;
        if (j < D) dst[j] = (f16)((v[i] - mean) * rstd * (float)gamma[j] + (float)beta[j]);
    }
}

extern "C" int vdx_clip_vision_embed_f16(const void* patch, int ldp, const void* class_emb, const void* pos_emb,
                                         const void* gamma, const void* beta, float eps, int F, int patches, int seq_pad,
                                         int D, void* out, int ldo, vdx_stream_t stream) {
    VDX_CHECK(patch && class_emb && pos_emb && gamma && beta && out, "clip_vision_embed: null pointer");
    VDX_CHECK(F > 0 && patches > 0 && seq_pad > patches && D > 0 && D <= 64 * EMB_MAXV,
              "clip_vision_embed: F=%d patches=%d seq_pad=%d D=%d", F, patches, seq_pad, D);
    VDX_CHECK(ldp >= D && ldo >= D, "clip_vision_embed: leading dims smaller than D");
    const int rows = F * seq_pad;
    hipLaunchKernelGGL(clip_vision_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const f16*)patch, ldp,
                       (const f16*)class_emb, (const f16*)pos_emb, (const f16*)gamma, (const f16*)beta, eps, F, patches,
                       seq_pad, D, (f16*)out, ldo);
    return vdx_launch_status("vdx_clip_vision_embed_f16");
}

// ---- quick_gelu (CLIP ViT-B/32's MLP activation: x * sigmoid(1.702 x)) ------------------------------------------
__global__ void quick_gelu_kernel(const f16* x, f16* y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = (float)x[i];
        y[i] = (f16)(v / (1.0f + __expf(-1.702f * v)));
    }
}
extern "C" int vdx_quick_gelu_f16(const void* x, void* y, size_t n, vdx_stream_t stream) {
    VDX_CHECK(x && y && n > 0, "quick_gelu: bad arguments");
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(quick_gelu_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const f16*)x, (f16*)y, n);
    return vdx_launch_status("vdx_quick_gelu_f16");
}

// ---- the score (scoring.py:106-107, :123-124, :137-140) ---------------------------------------------------------
// per_frame[f] = <img_f, txt> / (max(|img_f|, 1e-12) * max(|txt|, 1e-12)) (F.normalize on both sides), mean = their sum in
// frame order / F.  One block; wave w takes frames w, w+4, ...; lane j sums columns j, j+64, ... and the butterfly adds the
// lanes: the order is fixed, so the result is the same bits on every run.
__global__ __launch_bounds__(256) void clip_cosine_kernel(const f16* img, int ldi, const f16* txt, int F, int D,
                                                          float* per_frame, float* mean) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float tt = 0.f;
    for (int j = lane; j < D; j += 64) tt += (float)txt[j] * (float)txt[j];
    const float nt = fmaxf(sqrtf(wave_sum(tt)), 1e-12f);
    for (int f = wave; f < F; f += 4) {
        const f16* r = img + (size_t)f * ldi;
        float xx = 0.f, xt = 0.f;
        for (int j = lane; j < D; j += 64) {
            const float x = (float)r[j];
            xx += x * x;
            xt += x * (float)txt[j];
        }
        xx = wave_sum(xx);
        xt = wave_sum(xt);
        if (lane == 0) per_frame[f] = xt / (fmaxf(sqrtf(xx), 1e-12f) * nt);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int f = 0; f < F; ++f) s += per_frame[f];
        *mean = s / (float)F;
    }
}

extern "C" int vdx_clip_cosine_score_f16(const void* img, int ldi, const void* txt, int F, int D, float* per_frame,
                                         float* mean, vdx_stream_t stream) {
    VDX_CHECK(img && txt && per_frame && mean, "clip_cosine_score: null pointer");
    VDX_CHECK(F > 0 && D > 0 && ldi >= D, "clip_cosine_score: F=%d D=%d ldi=%d", F, D, ldi);
    hipLaunchKernelGGL(clip_cosine_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const f16*)img, ldi, (const f16*)txt, F, D,
                       per_frame, mean);
    return vdx_launch_status("vdx_clip_cosine_score_f16");
}
