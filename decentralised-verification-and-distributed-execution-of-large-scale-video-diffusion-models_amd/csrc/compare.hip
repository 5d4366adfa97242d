// compare.hip — full-reference comparison of two uint8 RGB clips of one shape: per frame the exact sum of squared differences
// (PSNR on the host), SSIM (Wang et al. 2004) and the per-scale cs / ssim means of MS-SSIM (Wang et al. 2003).  Nothing in the
// reference computes any of it (it never holds two clips); vdx/compare.py drives the launches and tests/compare_ref.py states
// the definition in float64 numpy.  Every R, G, B plane is a plane of its own: no grey conversion.
//
//   ssim_scale   one launch per scale over all F*3 plane pairs.  A block owns a 16 x 32 tile of the (H-10) x (W-10) map of valid
//                window positions.  It stages the 26 x 42 samples under the tile of both clips in LDS (fp32: bytes, and the 2x2
//                means of bytes, which are k / 4^s with k < 2^16, are exact there), takes the five windowed moments E[x], E[y],
//                E[x^2], E[y^2], E[xy] with the 11-tap Gaussian (sigma 1.5, float64 taps from the host) as a column pass into LDS
//                and a row pass out of it, forms
//                    cs = (2 sxy + C2) / (sx2 + sy2 + C2),   ssim = (2 mx my + C1) / (mx^2 + my^2 + C1) cs
//                at its positions and writes one partial sum of each per block (a fixed tree over the 256 threads).  At scale 0
//                it also writes the integer sum of (a - b)^2 over the bytes it owns: the tile's own 16 x 32 samples, extended to
//                the image edge in the last tile row and column, so every byte of the plane is counted exactly once.
//   down2        2x2 mean of every plane of both clips (an odd last row or column is dropped): u8 -> fp32, fp32 -> fp32; the
//                sum of four in a fixed grouping times 0.25, exact for everything that descends from bytes.
//   finalize     per frame and plane: the partials summed in a fixed order (fp64; the byte sums in uint64) over the number of
//                positions -> means [F][3][5][2] (ssim, cs) at the launch's scale, and at scale 0 sse [F].
//
// Arithmetic.  The hazard is the cancellation in E[x^2] - mx^2: E[x^2] reaches 65025 where C2 is 58.5, so in fp32 (ulp 2^-8 at
// 62500) a flat bright region with a variance of order 1 loses every digit that matters.  Like flow.hip's polyexp / update,
// everything between the fp32 LDS samples and the fp64 partials is fp64.  Measured against the float64 restatement on the MI355X
// (profiles/compare_parity.txt, per-plane means): 2.2e-16 on flat 250 +-1 planes, 2.2e-16 on perturbed noise, 2.8e-17 on
// independent noise (whose means are near 0): one or two units in the last place everywhere, which is what reordering a
// float64 sum costs, so centring the samples had nothing left to buy and was not built.  The same restatement with float32
// moments, in numpy, is off by 5.7e-4 in the SSIM map on the flat-bright input.
// The file is compiled without mul-add contraction: with x and y exchanged every operation sees the same operands (a + b, a * b
// commute; an fma(mx, mx, my * my) would not), so compare(a, b) and compare(b, a) agree bit for bit, and for a == b numerator
// and denominator are the same bits and ssim is exactly 1.  No atomics; a plane's numbers depend on that plane alone: the
// same bits on every run and however many frames share the launch.
//
// LDS per block: 2 x 26 x 42 x 4 (samples) + 5 x 16 x 42 x 8 (column moments) + 256 x 8 (reduction) = 37,664 bytes: four blocks
// of 256 threads per CU (150.6 of 160 KiB), 16 waves per CU; the halo makes a block read 2.1 samples per position, from L2.
#include "vdx_common.h"

#define CMP_TAPS 11
#define CMP_HALO (CMP_TAPS - 1)
#define CMP_TX 32
#define CMP_TY 16
#define CMP_IX (CMP_TX + CMP_HALO)
#define CMP_IY (CMP_TY + CMP_HALO)
#define CMP_THREADS 256
#define CMP_SCALES 5

struct cmp_taps {
    double w[CMP_TAPS];
};

__device__ __forceinline__ float cmp_load(const unsigned char* p) { return (float)*p; }
__device__ __forceinline__ float cmp_load(const float* p) { return *p; }

// sum over the block's 256 threads in a fixed tree; every thread gets the result.  `red` may be reused after the return.
template <class T>
__device__ __forceinline__ T cmp_block_sum(T v, T* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = CMP_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}

static inline int cmp_tiles_x(int W) { return (W - CMP_HALO + CMP_TX - 1) / CMP_TX; }
static inline int cmp_tiles_y(int H) { return (H - CMP_HALO + CMP_TY - 1) / CMP_TY; }

// plane p = 3 f + c of clip `a` begins at a + f fp_a + c cp, its sample (y, x) lies y rp_a + x xp elements further (uint8 RGB
// frames: cp 1, xp 3; packed fp32 planes: cp H W, fp 3 H W, xp 1).  grid: (tiles, planes).
template <class T>
__global__ __launch_bounds__(CMP_THREADS) void cmp_ssim_scale_kernel(const T* a, size_t fp_a, int rp_a, const T* b, size_t fp_b, int rp_b,
                                                                     size_t cp, int xp, int H, int W, int tiles_x, cmp_taps taps,
                                                                     double* part, unsigned long long* sse_part) {
    __shared__ float sa[CMP_IY * CMP_IX], sb[CMP_IY * CMP_IX];
    __shared__ double sv[5][CMP_TY * CMP_IX];
    __shared__ double red[CMP_THREADS];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, plane = blockIdx.y, ntiles = gridDim.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * CMP_TY, x0 = tx * CMP_TX;
    const bool last_y = ty == ntiles / tiles_x - 1, last_x = tx == tiles_x - 1;
    const int f = plane / 3, c = plane - 3 * f;
    const T* pa = a + (size_t)f * fp_a + (size_t)c * cp;
    const T* pb = b + (size_t)f * fp_b + (size_t)c * cp;

    unsigned long long sse = 0;
    for (int i = tid; i < CMP_IY * CMP_IX; i += CMP_THREADS) {
        const int r = i / CMP_IX, q = i - r * CMP_IX;
        const int y = y0 + r, x = x0 + q;
        float va = 0.f, vb = 0.f;
        if (y < H && x < W) {                                             // samples past the image feed no valid position
            va = cmp_load(pa + (size_t)y * rp_a + (size_t)x * xp);
            vb = cmp_load(pb + (size_t)y * rp_b + (size_t)x * xp);
            if (sse_part && (r < CMP_TY || last_y) && (q < CMP_TX || last_x)) {
                const int d = (int)va - (int)vb;
                sse += (unsigned long long)(d * d);
            }
        }
        sa[i] = va;
        sb[i] = vb;
    }
    __syncthreads();

    for (int i = tid; i < CMP_TY * CMP_IX; i += CMP_THREADS) {            // column pass: rows r .. r + 10 of column q
        const int r = i / CMP_IX, q = i - r * CMP_IX;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
        for (int k = 0; k < CMP_TAPS; ++k) {
            const double x = (double)sa[(r + k) * CMP_IX + q], y = (double)sb[(r + k) * CMP_IX + q], w = taps.w[k];
            m0 += w * x;
            m1 += w * y;
            m2 += w * (x * x);
            m3 += w * (y * y);
            m4 += w * (x * y);
        }
        sv[0][i] = m0, sv[1][i] = m1, sv[2][i] = m2, sv[3][i] = m3, sv[4][i] = m4;
    }
    __syncthreads();

    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double acc_s = 0.0, acc_c = 0.0;
#pragma unroll
    for (int j = 0; j < CMP_TY * CMP_TX / CMP_THREADS; ++j) {            // row pass: columns q .. q + 10 of row r
        const int o = tid + j * CMP_THREADS;
        const int r = o / CMP_TX, q = o - r * CMP_TX;
        double m[5];
#pragma unroll
        for (int n = 0; n < 5; ++n) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < CMP_TAPS; ++k) s += taps.w[k] * sv[n][r * CMP_IX + q + k];
            m[n] = s;
        }
        const double mx = m[0], my = m[1];
        const double mxy = mx * my, mxx = mx * mx, myy = my * my;
        const double vx = m[2] - mxx, vy = m[3] - myy, vxy = m[4] - mxy;
        const double cs = (2.0 * vxy + C2) / (vx + vy + C2);
        const double lum = (2.0 * mxy + C1) / (mxx + myy + C1);
        if (y0 + r < H - CMP_HALO && x0 + q < W - CMP_HALO) {
            acc_s += lum * cs;
            acc_c += cs;
        }
    }
    const double bs = cmp_block_sum(acc_s, red);
    const double bc = cmp_block_sum(acc_c, red);
    const size_t slot = (size_t)plane * ntiles + tile;
    if (tid == 0) {
        part[2 * slot] = bs;
        part[2 * slot + 1] = bc;
    }
    if (sse_part) {
        const unsigned long long be = cmp_block_sum(sse, (unsigned long long*)red);
        if (tid == 0) sse_part[slot] = be;
    }
}

template <class T>
__global__ __launch_bounds__(256) void cmp_down2_kernel(const T* in0, size_t fp0, int rp0, const T* in1, size_t fp1, int rp1, size_t cp,
                                                        int xp, int h, int w, long long total, float* out0, float* out1) {
    const T* in = blockIdx.y ? in1 : in0;
    const size_t fp = blockIdx.y ? fp1 : fp0;
    const int rp = blockIdx.y ? rp1 : rp0;
    float* out = blockIdx.y ? out1 : out0;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % w);
        const long long py = idx / w;
        const int y = (int)(py % h);
        const long long plane = py / h;
        const T* p = in + (size_t)(plane / 3) * fp + (size_t)(plane % 3) * cp + (size_t)(2 * y) * rp + (size_t)(2 * x) * xp;
        out[idx] = ((cmp_load(p) + cmp_load(p + xp)) + (cmp_load(p + rp) + cmp_load(p + rp + xp))) * 0.25f;
    }
}

// grid: F blocks.  part: fp64 [F*3][ntiles][2], sse_part: uint64 [F*3][ntiles] or NULL.
__global__ __launch_bounds__(CMP_THREADS) void cmp_finalize_kernel(const double* part, const unsigned long long* sse_part, int ntiles,
                                                                   double count, int scale, double* means, unsigned long long* sse) {
    __shared__ double red[CMP_THREADS];
    const int tid = threadIdx.x, f = blockIdx.x;
    unsigned long long e = 0;
    for (int c = 0; c < 3; ++c) {
        const size_t base = (size_t)(3 * f + c) * ntiles;
        double s = 0.0, cs = 0.0;
        for (int i = tid; i < ntiles; i += CMP_THREADS) {
            s += part[2 * (base + i)];
            cs += part[2 * (base + i) + 1];
            if (sse_part) e += sse_part[base + i];
        }
        const double S = cmp_block_sum(s, red), Cs = cmp_block_sum(cs, red);
        if (tid == 0) {
            double* m = means + ((size_t)(3 * f + c) * CMP_SCALES + scale) * 2;
            m[0] = S / count;
            m[1] = Cs / count;
        }
    }
    if (sse_part) {
        const unsigned long long E = cmp_block_sum(e, (unsigned long long*)red);
        if (tid == 0) sse[f] = E;
    }
}

// ---- entries --------------------------------------------------------------------------------------------------------------
#define CMP_MAX_PLANES 65535                          // gridDim.y

static int cmp_check_size(const char* what, int n_planes, int H, int W) {
    VDX_CHECK(n_planes >= 1 && n_planes <= CMP_MAX_PLANES, "%s: %d planes (1..%d)", what, n_planes, CMP_MAX_PLANES);
    VDX_CHECK(H >= CMP_TAPS && W >= CMP_TAPS && (long long)H * W < (1ll << 28), "%s: H=%d W=%d (both >= %d, H*W < 2^28)", what, H, W,
              CMP_TAPS);
    return 0;
}

static int cmp_taps_from(const char* what, const double* taps, cmp_taps& t) {
    VDX_CHECK(taps, "%s: null taps", what);
    for (int k = 0; k < CMP_TAPS; ++k) {
        VDX_CHECK(taps[k] >= 0.0 && taps[k] <= 1.0, "%s: tap %d is not a weight", what, k);
        t.w[k] = taps[k];
    }
    return 0;
}

extern "C" int vdx_compare_tiles(int H, int W) {
    if (H < CMP_TAPS || W < CMP_TAPS || (long long)H * W >= (1ll << 28)) return 0;
    return cmp_tiles_x(W) * cmp_tiles_y(H);
}

extern "C" int vdx_compare_ssim_scale_u8(const void* a, size_t a_frame_pitch, int a_row_pitch, const void* b, size_t b_frame_pitch,
                                         int b_row_pitch, int F, int H, int W, const double* taps, double* partials,
                                         uint64_t* sse_partials, vdx_stream_t stream) {
    VDX_CHECK(a && b && partials && sse_partials, "compare_ssim_scale_u8: null pointer");
    VDX_CHECK(F >= 1 && F <= CMP_MAX_PLANES / 3, "compare_ssim_scale_u8: F=%d (1..%d)", F, CMP_MAX_PLANES / 3);
    if (cmp_check_size("compare_ssim_scale_u8", 3 * F, H, W)) return -1;
    VDX_CHECK(a_row_pitch >= 3 * W && a_frame_pitch >= (size_t)a_row_pitch * H && b_row_pitch >= 3 * W &&
                  b_frame_pitch >= (size_t)b_row_pitch * H, "compare_ssim_scale_u8: pitches too small");
    cmp_taps t;
    if (cmp_taps_from("compare_ssim_scale_u8", taps, t)) return -1;
    hipLaunchKernelGGL(cmp_ssim_scale_kernel<unsigned char>, dim3(cmp_tiles_x(W) * cmp_tiles_y(H), 3 * F), dim3(CMP_THREADS), 0,
                       (hipStream_t)stream, (const unsigned char*)a, a_frame_pitch, a_row_pitch, (const unsigned char*)b, b_frame_pitch,
                       b_row_pitch, (size_t)1, 3, H, W, cmp_tiles_x(W), t, partials, (unsigned long long*)sse_partials);
    return vdx_launch_status("vdx_compare_ssim_scale_u8");
}

extern "C" int vdx_compare_ssim_scale_f32(const float* a, const float* b, int n_planes, int H, int W, const double* taps,
                                          double* partials, vdx_stream_t stream) {
    VDX_CHECK(a && b && partials, "compare_ssim_scale_f32: null pointer");
    if (cmp_check_size("compare_ssim_scale_f32", n_planes, H, W)) return -1;
    cmp_taps t;
    if (cmp_taps_from("compare_ssim_scale_f32", taps, t)) return -1;
    const size_t hw = (size_t)H * W;
    hipLaunchKernelGGL(cmp_ssim_scale_kernel<float>, dim3(cmp_tiles_x(W) * cmp_tiles_y(H), n_planes), dim3(CMP_THREADS), 0,
                       (hipStream_t)stream, a, 3 * hw, W, b, 3 * hw, W, hw, 1, H, W, cmp_tiles_x(W), t, partials,
                       (unsigned long long*)nullptr);
    return vdx_launch_status("vdx_compare_ssim_scale_f32");
}

static inline int cmp_down2_grid(long long n) {
    const long long blocks = (n + 255) / 256;
    return (int)(blocks > 2048 ? 2048 : blocks);
}

extern "C" int vdx_compare_down2_u8(const void* a, size_t a_frame_pitch, int a_row_pitch, const void* b, size_t b_frame_pitch,
                                    int b_row_pitch, int F, int H, int W, float* out_a, float* out_b, vdx_stream_t stream) {
    VDX_CHECK(a && out_a && (b != nullptr) == (out_b != nullptr), "compare_down2_u8: null pointer");
    VDX_CHECK(F >= 1 && F <= CMP_MAX_PLANES / 3 && H >= 2 && W >= 2 && (long long)H * W < (1ll << 28), "compare_down2_u8: F=%d H=%d W=%d",
              F, H, W);
    VDX_CHECK(a_row_pitch >= 3 * W && a_frame_pitch >= (size_t)a_row_pitch * H, "compare_down2_u8: pitches of a too small");
    VDX_CHECK(!b || (b_row_pitch >= 3 * W && b_frame_pitch >= (size_t)b_row_pitch * H), "compare_down2_u8: pitches of b too small");
    const int h = H / 2, w = W / 2;
    const long long total = 3ll * F * h * w;
    hipLaunchKernelGGL(cmp_down2_kernel<unsigned char>, dim3(cmp_down2_grid(total), b ? 2 : 1), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)a, a_frame_pitch, a_row_pitch, (const unsigned char*)b, b_frame_pitch, b_row_pitch, (size_t)1,
                       3, h, w, total, out_a, out_b);
    return vdx_launch_status("vdx_compare_down2_u8");
}

extern "C" int vdx_compare_down2_f32(const float* a, const float* b, int n_planes, int H, int W, float* out_a, float* out_b,
                                     vdx_stream_t stream) {
    VDX_CHECK(a && out_a && (b != nullptr) == (out_b != nullptr), "compare_down2_f32: null pointer");
    VDX_CHECK(a != out_a && b != out_a && a != out_b && (!b || b != out_b), "compare_down2_f32: input and output alias");
    VDX_CHECK(n_planes >= 1 && n_planes <= CMP_MAX_PLANES && H >= 2 && W >= 2 && (long long)H * W < (1ll << 28),
              "compare_down2_f32: n=%d H=%d W=%d", n_planes, H, W);
    const int h = H / 2, w = W / 2;
    const size_t hw = (size_t)H * W;
    const long long total = (long long)n_planes * h * w;
    hipLaunchKernelGGL(cmp_down2_kernel<float>, dim3(cmp_down2_grid(total), b ? 2 : 1), dim3(256), 0, (hipStream_t)stream, a, 3 * hw, W, b,
                       3 * hw, W, hw, 1, h, w, total, out_a, out_b);
    return vdx_launch_status("vdx_compare_down2_f32");
}

extern "C" int vdx_compare_finalize(const double* partials, const uint64_t* sse_partials, int F, int n_tiles, double count, int scale,
                                    double* means, uint64_t* sse, vdx_stream_t stream) {
    VDX_CHECK(partials && means && (sse_partials != nullptr) == (sse != nullptr), "compare_finalize: null pointer");
    VDX_CHECK(F >= 1 && F <= CMP_MAX_PLANES / 3 && n_tiles >= 1 && n_tiles < (1 << 24), "compare_finalize: F=%d n_tiles=%d", F, n_tiles);
    VDX_CHECK(scale >= 0 && scale < CMP_SCALES && count >= 1.0, "compare_finalize: scale=%d count=%g", scale, count);
    hipLaunchKernelGGL(cmp_finalize_kernel, dim3(F), dim3(CMP_THREADS), 0, (hipStream_t)stream, partials,
                       (const unsigned long long*)sse_partials, n_tiles, count, scale, means, (unsigned long long*)sse);
    return vdx_launch_status("vdx_compare_finalize");
}
