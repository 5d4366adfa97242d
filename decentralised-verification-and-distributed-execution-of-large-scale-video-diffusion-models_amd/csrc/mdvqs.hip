// mdvqs.hip — the validator's MD-VQS video-quality term and authenticity gate on the device
// (InferNet/template/validator/scoring.py:13-67 verify_video_authenticity_common, :269-309 MDVQS.compute_video_quality):
// LPIPS-AlexNet between consecutive frames and the integer frame statistics of the gate.  The five convolutions run on the
// GEMM kernels (vdx/lpips.py); here are the gathers that feed them (conv1's stem from the resized uint8 frames, a generic
// stride-1 im2col), ReLU and ReLU + max-pool, the LPIPS distance of one tap, and the grey histograms / absolute differences.
#include "vdx_common.h"

static inline int mdvqs_grid(long long n) {                   // memory-bound, grid-stride: at most 8 blocks per CU
    const long long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// ---- conv1 stem: resized uint8 frames -> im2col rows of AlexNet's Conv2d(3, 64, 11, stride 4, padding 2) ------------------
// Row f*3025 + oy*55 + ox, column (ky*11 + kx)*3 + c = lut[c][u8[f][4oy-2+ky][4ox-2+kx][c]], 0 outside the image (the padding
// is applied to the conv's input, after both affine maps), columns 363..383 zero.  lut: fp16 [3][256] of
// ((u/255 - mean_c)/std_c - shift_c)/scale_c evaluated in fp32 on the host (vdx/lpips.py `stem_lut`).
#define STEM_PX 224
#define STEM_OUT 55
#define STEM_K 363
#define STEM_KPAD 384
__global__ __launch_bounds__(256) void lpips_stem_kernel(const unsigned char* u8, int F, const f16* lut, f16* out, int ldo) {
    __shared__ f16 tab[768];
    for (int i = threadIdx.x; i < 768; i += blockDim.x) tab[i] = lut[i];
    __syncthreads();
    const long long total = (long long)F * STEM_OUT * STEM_OUT * (STEM_KPAD / 8);
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(idx % (STEM_KPAD / 8));
        const long long row = idx / (STEM_KPAD / 8);
        const int ox = (int)(row % STEM_OUT);
        const long long fy = row / STEM_OUT;
        const int oy = (int)(fy % STEM_OUT), f = (int)(fy / STEM_OUT);
        const unsigned char* img = u8 + (size_t)f * STEM_PX * STEM_PX * 3;
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = q * 8 + j;
            const int tap = k / 3, c = k - tap * 3;
            const int ky = tap / 11, kx = tap - ky * 11;
            const int iy = oy * 4 - 2 + ky, ix = ox * 4 - 2 + kx;
            const bool ok = k < STEM_K && (unsigned)iy < (unsigned)STEM_PX && (unsigned)ix < (unsigned)STEM_PX;
            const f16 t = tab[c * 256 + img[((size_t)(ok ? iy : 0) * STEM_PX + (ok ? ix : 0)) * 3 + c]];   // the load stays in bounds
            v[j] = ok ? t : (f16)0.f;
        }
        *(f16x8*)(out + (size_t)row * ldo + q * 8) = v;
    }
}

extern "C" int vdx_lpips_stem_u8(const void* u8, int F, const void* lut_f16, void* out_rows, int ldo, vdx_stream_t stream) {
    VDX_CHECK(u8 && lut_f16 && out_rows, "lpips_stem: null pointer");
    VDX_CHECK(F > 0 && F <= 65536, "lpips_stem: F=%d", F);
    VDX_CHECK(ldo >= STEM_KPAD && ldo % 8 == 0, "lpips_stem: ldo=%d (needs >= 384, a multiple of 8)", ldo);
    VDX_CHECK(((uintptr_t)out_rows & 15) == 0, "lpips_stem: out_rows must be 16-byte aligned (16-byte stores)");
    const long long total = (long long)F * STEM_OUT * STEM_OUT * (STEM_KPAD / 8);
    hipLaunchKernelGGL(lpips_stem_kernel, dim3(mdvqs_grid(total)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)u8, F,
                       (const f16*)lut_f16, (f16*)out_rows, ldo);
    return vdx_launch_status("vdx_lpips_stem_u8");
}

// ---- ReLU -------------------------------------------------------------------------------------------------------------
// x < 0 ? 0 : x per element: NaN stays NaN, +-inf as torch.relu.  8 values per lane where both pointers are 16-byte
// aligned, the tail (and unaligned calls) one by one.  y may alias x.
__device__ __forceinline__ f16 relu1(f16 v) { return v < (f16)0.f ? (f16)0.f : v; }
__device__ __forceinline__ f16x8 relu8(f16x8 v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = relu1(v[j]);
    return v;
}
__global__ __launch_bounds__(256) void relu_kernel(const f16* x, f16* y, size_t n, int vec) {
    const size_t n8 = vec ? n / 8 : 0;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = t0; i < n8; i += stride) ((f16x8*)y)[i] = relu8(((const f16x8*)x)[i]);
    for (size_t i = n8 * 8 + t0; i < n; i += stride) y[i] = relu1(x[i]);
}
extern "C" int vdx_relu_f16(const void* x, void* y, size_t n, vdx_stream_t stream) {
    VDX_CHECK(x && y && n > 0, "relu: bad arguments");
    const int vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    hipLaunchKernelGGL(relu_kernel, dim3(mdvqs_grid((long long)((n + 7) / 8))), dim3(256), 0, (hipStream_t)stream, (const f16*)x,
                       (f16*)y, n, vec);
    return vdx_launch_status("vdx_relu_f16");
}

// ---- ReLU in place + MaxPool2d(3, stride 2) ------------------------------------------------------------------------------
// Two launches on the stream: the pool reads the RAW rows (max over the window of relu(x) = max(0, max x); NaN propagates as
// in torch), then the rows are ReLU'd in place (the LPIPS tap) — no launch reads what another thread of it writes.
__global__ __launch_bounds__(256) void relu_maxpool_kernel(const f16* x, int ldx, int n_img, int H, int W, int C, int Ho, int Wo,
                                                           f16* out, int ldo) {
    const int cq = C / 8;
    const long long total = (long long)n_img * Ho * Wo * cq;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(idx % cq);
        const long long row = idx / cq;
        const int ox = (int)(row % Wo);
        const long long ny = row / Wo;
        const int oy = (int)(ny % Ho), n = (int)(ny / Ho);
        f16x8 m = {};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int iy = oy * 2 + t / 3, ix = ox * 2 + t % 3;         // < H, W: Ho = (H - 3) / 2 + 1
            const f16x8 v = *(const f16x8*)(x + ((size_t)n * H * W + (size_t)iy * W + ix) * ldx + q * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = (v[j] > m[j] || v[j] != v[j]) ? v[j] : m[j];
        }
        *(f16x8*)(out + (size_t)row * ldo + q * 8) = m;
    }
}
__global__ __launch_bounds__(256) void relu_rows_kernel(f16* x, int ldx, long long rows, int C) {
    const int cq = C / 8;
    const long long total = rows * cq;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        f16x8* p = (f16x8*)(x + (size_t)(idx / cq) * ldx + (idx % cq) * 8);
        *p = relu8(*p);
    }
}
extern "C" int vdx_relu_maxpool_f16(void* x, int ldx, int n_img, int H, int W, int C, void* out, int ldo, vdx_stream_t stream) {
    VDX_CHECK(x && out && x != out, "relu_maxpool: null or aliased pointers");
    VDX_CHECK(n_img > 0 && H >= 3 && W >= 3 && C > 0 && C % 8 == 0, "relu_maxpool: n=%d H=%d W=%d C=%d (C %% 8 == 0, H, W >= 3)", n_img, H, W, C);
    VDX_CHECK((long long)n_img * H * W < (1ll << 31), "relu_maxpool: too many rows");
    VDX_CHECK(ldx >= C && ldo >= C && ldx % 8 == 0 && ldo % 8 == 0, "relu_maxpool: ldx=%d ldo=%d (>= C, multiples of 8)", ldx, ldo);
    VDX_CHECK((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "relu_maxpool: pointers must be 16-byte aligned");
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    hipLaunchKernelGGL(relu_maxpool_kernel, dim3(mdvqs_grid((long long)n_img * Ho * Wo * (C / 8))), dim3(256), 0, (hipStream_t)stream,
                       (const f16*)x, ldx, n_img, H, W, C, Ho, Wo, (f16*)out, ldo);
    hipLaunchKernelGGL(relu_rows_kernel, dim3(mdvqs_grid((long long)n_img * H * W * (C / 8))), dim3(256), 0, (hipStream_t)stream,
                       (f16*)x, ldx, (long long)n_img * H * W, C);
    return vdx_launch_status("vdx_relu_maxpool_f16");
}

// ---- stride-1 im2col of channels-last rows -------------------------------------------------------------------------------
// out row n*Ho*Wo + oy*Wo + ox, column (ky*k + kx)*C + c = x[n][oy - pad + ky][ox - pad + kx][c], 0 outside the image;
// Ho = H + 2 pad - k + 1.  One 16-byte chunk per lane.
__global__ __launch_bounds__(256) void im2col_kernel(const f16* x, int ldx, int n_img, int H, int W, int C, int k, int pad, int Ho,
                                                     int Wo, f16* out, int ldo) {
    const int cq = C / 8, kq = k * k * cq;
    const long long total = (long long)n_img * Ho * Wo * kq;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int kk = (int)(idx % kq);
        const long long row = idx / kq;
        const int tap = kk / cq, q = kk - tap * cq;
        const int ky = tap / k, kx = tap - ky * k;
        const int ox = (int)(row % Wo);
        const long long ny = row / Wo;
        const int oy = (int)(ny % Ho), n = (int)(ny / Ho);
        const int iy = oy - pad + ky, ix = ox - pad + kx;
        f16x8 v = {};
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
            v = *(const f16x8*)(x + ((size_t)n * H * W + (size_t)iy * W + ix) * ldx + q * 8);
        *(f16x8*)(out + (size_t)row * ldo + (size_t)tap * C + q * 8) = v;
    }
}
extern "C" int vdx_im2col_f16(const void* x, int ldx, int n_img, int H, int W, int C, int k, int pad, void* out, int ldo,
                              vdx_stream_t stream) {
    VDX_CHECK(x && out && x != out, "im2col: null or aliased pointers");
    VDX_CHECK(n_img > 0 && H > 0 && W > 0 && C > 0 && C % 64 == 0, "im2col: n=%d H=%d W=%d C=%d (C %% 64 == 0)", n_img, H, W, C);
    VDX_CHECK(k >= 1 && k <= 11 && pad >= 0 && pad < k && H + 2 * pad >= k && W + 2 * pad >= k, "im2col: k=%d pad=%d on %dx%d", k, pad, H, W);
    VDX_CHECK((long long)n_img * H * W < (1ll << 31), "im2col: too many rows");
    VDX_CHECK(ldx >= C && ldx % 8 == 0 && ldo >= k * k * C && ldo % 8 == 0, "im2col: ldx=%d ldo=%d", ldx, ldo);
    VDX_CHECK((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "im2col: pointers must be 16-byte aligned");
    const int Ho = H + 2 * pad - k + 1, Wo = W + 2 * pad - k + 1;
    hipLaunchKernelGGL(im2col_kernel, dim3(mdvqs_grid((long long)n_img * Ho * Wo * k * k * (C / 8))), dim3(256), 0, (hipStream_t)stream,
                       (const f16*)x, ldx, n_img, H, W, C, k, pad, Ho, Wo, (f16*)out, ldo);
    return vdx_launch_status("vdx_im2col_f16");
}

// ---- LPIPS distance of one tap --------------------------------------------------------------------------------------
// out[p] (+)= 1/HW * sum_pix sum_c lin[c] * (x_p[pix][c] / (|x_p[pix]| + 1e-10) - x_{p+1}[pix][c] / (|x_{p+1}[pix]| + 1e-10))^2
// for the F-1 consecutive pairs; |.| = sqrt(sum_c x^2) in fp32.  One block per pair, 16 waves: wave w takes pixels w, w+16,
// ...; lane j channels j, j+64, ...; the two norms come from one butterfly each, the weighted squares stay in the lane
// until the end, then one butterfly per wave and the 16 wave sums are added in wave order by one thread.  No atomics: the
// same bits on every run.  An all-zero pixel gives 0 / (0 + 1e-10) = 0.
#define DIST_WAVES 16
#define DIST_MAXC 8   // C <= 64 * 8
__global__ __launch_bounds__(DIST_WAVES * 64) void lpips_distance_kernel(const f16* x, int ldx, int HW, int C, const float* lin,
                                                                         float* out, int accumulate) {
    __shared__ float part[DIST_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, p = blockIdx.x;
    const f16* a0 = x + (size_t)p * HW * ldx;
    const f16* b0 = a0 + (size_t)HW * ldx;
    float w[DIST_MAXC];
#pragma unroll
    for (int i = 0; i < DIST_MAXC; ++i) w[i] = lane + 64 * i < C ? lin[lane + 64 * i] : 0.f;
    float acc = 0.f;
    for (int pix = wave; pix < HW; pix += DIST_WAVES) {
        const f16* a = a0 + (size_t)pix * ldx;
        const f16* b = b0 + (size_t)pix * ldx;
        float va[DIST_MAXC], vb[DIST_MAXC], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int i = 0; i < DIST_MAXC; ++i) {
            const int c = lane + 64 * i;
            va[i] = c < C ? (float)a[c] : 0.f;
            vb[i] = c < C ? (float)b[c] : 0.f;
            sa += va[i] * va[i];
            sb += vb[i] * vb[i];
        }
        const float ra = 1.0f / (sqrtf(wave_sum(sa)) + 1e-10f), rb = 1.0f / (sqrtf(wave_sum(sb)) + 1e-10f);
#pragma unroll
        for (int i = 0; i < DIST_MAXC; ++i) {
            float d;
            {
#pragma clang fp contract(off)   // a fused va*ra - (vb*rb) would leave the rounding error of one product: equal frames must give exactly 0
                const float na = va[i] * ra, nb = vb[i] * rb;
                d = na - nb;
            }
            acc += w[i] * d * d;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < DIST_WAVES; ++i) s += part[i];
        s /= (float)HW;
        out[p] = accumulate ? out[p] + s : s;
    }
}
extern "C" int vdx_lpips_distance_f16(const void* x, int ldx, int F, int HW, int C, const float* lin, float* out, int accumulate,
                                      vdx_stream_t stream) {
    VDX_CHECK(x && lin && out, "lpips_distance: null pointer");
    VDX_CHECK(F >= 2 && F <= 65536 && HW > 0 && C > 0 && C <= 64 * DIST_MAXC && ldx >= C, "lpips_distance: F=%d HW=%d C=%d ldx=%d", F, HW, C, ldx);
    VDX_CHECK((long long)F * HW < (1ll << 31), "lpips_distance: too many rows");
    hipLaunchKernelGGL(lpips_distance_kernel, dim3(F - 1), dim3(DIST_WAVES * 64), 0, (hipStream_t)stream, (const f16*)x, ldx, HW, C,
                       lin, out, accumulate);
    return vdx_launch_status("vdx_lpips_distance_f16");
}

// ---- frame statistics of the authenticity gate (scoring.py:27-36) --------------------------------------------------------
// hist[f][g] = pixels of frame f whose grey level (OpenCV's 8-bit RGB2GRAY: (4899 R + 9617 G + 1868 B + 8192) >> 14) is g;
// absdiff[f] = sum over all bytes of |frame f+1 - frame f| (cv2.absdiff summed; the host divides).  Integers only: LDS
// atomics per block, then one integer atomic per non-empty bin and block — exact whatever the order.  Both outputs are
// zeroed on the stream first.
#define STATS_BANDS 32
__global__ __launch_bounds__(256) void frame_stats_kernel(const unsigned char* frames, size_t fp, int rp, int F, int H, int W,
                                                          unsigned int* hist, unsigned long long* absdiff) {
    __shared__ unsigned int h[256];
    __shared__ unsigned long long dsum;
    const int f = blockIdx.y;
    h[threadIdx.x] = 0;                                   // blockDim.x == 256
    if (threadIdx.x == 0) dsum = 0;
    __syncthreads();
    const int rows = (H + gridDim.x - 1) / gridDim.x;
    const int y0 = blockIdx.x * rows, y1 = min(H, y0 + rows);
    const unsigned char* cur = frames + (size_t)f * fp;
    const bool pair = f + 1 < F;
    unsigned int d = 0;                                   // <= 765 per pixel, a band's pixels / 256 per thread: far below 2^32
    unsigned long long dl = 0;
    const long long npx = (long long)max(y1 - y0, 0) * W;
    for (long long i = threadIdx.x; i < npx; i += blockDim.x) {
        const int y = y0 + (int)(i / W), xx = (int)(i % W);
        const unsigned char* px = cur + (size_t)y * rp + (size_t)xx * 3;
        const int r = px[0], g = px[1], b = px[2];
        atomicAdd(&h[(r * 4899 + g * 9617 + b * 1868 + 8192) >> 14], 1u);
        if (pair) {
            const unsigned char* nx = px + fp;
            d += abs(r - (int)nx[0]) + abs(g - (int)nx[1]) + abs(b - (int)nx[2]);
            if (d > 0x7fffffffu) { dl += d; d = 0; }
        }
    }
    dl += d;
    if (pair && dl) atomicAdd(&dsum, dl);
    __syncthreads();
    const unsigned int c = h[threadIdx.x];
    if (c) atomicAdd(&hist[(size_t)f * 256 + threadIdx.x], c);
    if (pair && threadIdx.x == 0 && dsum) atomicAdd(&absdiff[f], dsum);
}
extern "C" int vdx_frame_stats_u8(const void* frames, size_t frame_pitch, int row_pitch, int F, int H, int W, uint32_t* hist,
                                  uint64_t* absdiff, vdx_stream_t stream) {
    VDX_CHECK(frames && hist && (absdiff || F == 1), "frame_stats: null pointer");
    VDX_CHECK(F > 0 && F <= 65535 && H > 0 && W > 0, "frame_stats: F=%d H=%d W=%d", F, H, W);
    VDX_CHECK(row_pitch >= 3 * W && frame_pitch >= (size_t)row_pitch * H, "frame_stats: pitches too small");
    VDX_CHECK((long long)H * W < (1ll << 32), "frame_stats: a bin would not fit 32 bits");
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)F * 256 * sizeof(uint32_t), (hipStream_t)stream);
    if (e == hipSuccess && F > 1) e = hipMemsetAsync(absdiff, 0, (size_t)(F - 1) * sizeof(uint64_t), (hipStream_t)stream);
    VDX_CHECK(e == hipSuccess, "frame_stats: memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(frame_stats_kernel, dim3(H < STATS_BANDS ? H : STATS_BANDS, F), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)frames, frame_pitch, row_pitch, F, H, W, (unsigned int*)hist,
                       (unsigned long long*)absdiff);
    return vdx_launch_status("vdx_frame_stats_u8");
}
