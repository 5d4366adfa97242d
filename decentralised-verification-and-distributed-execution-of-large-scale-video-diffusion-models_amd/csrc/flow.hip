// flow.hip — Farneback dense optical flow on the device, batched over the frame pairs of a clip, and the two numbers built
// on it: MD-VQS temporal consistency (InferNet/template/validator/scoring.py:311-339) and the result row's `flow_err`
// (Distribution/strategies/fsdp_chunked_coherent.py:236-246).  The algorithm is vdx/compat/cv2_shim.py's
// `calcOpticalFlowFarneback` (pyr_scale 0.5, winsize 15, poly_n 5, poly_sigma 1.2, flags 0; levels and iterations free) stage
// by stage; vdx/flow.py drives the launches.  Every plane in memory is fp32.  grey, corr1d, resize, abs_sum and remap compute in
// fp32 (remap's sums in integers); polyexp and update compute in fp64 between their fp32 loads and stores, because the 2 x 2
// systems of a straight edge on a flat background are nearly singular.  Every sum runs in a fixed order and no floating-point
// atomic is used: the same bits on every run, and a pair's flow does not depend on how many pairs the batch holds.
//
//   grey         uint8 RGB -> fp32 grey, OpenCV's 14-bit weights
//   corr1d       1-D correlation along one axis, mirror (reflect-101) border: the pyramid's Gaussian blur, taps from the host
//   resize       bilinear, half-pixel centres, clamped (`_resize_linear`): pyramid levels (1 channel), flow upsampling (2, x2)
//   polyexp      per frame and level: six separable 11-tap correlations -> inv(G) rows -> bx, by, axx, ayy, axy (fp64 inside)
//   update       one displacement iteration for every pair in one launch; the five window products live in LDS only (fp64)
//   abs_sum      per pair sum |flow| (TC), two fixed-order stages
//   remap        warp prev by the flow (bilinear, constant-0 border, round half to even), sum |warp - next| as integers
#include "vdx_common.h"

#define FLOW_POLY_R 5                                 // poly_n
#define FLOW_POLY_TAPS (2 * FLOW_POLY_R + 1)
#define FLOW_WIN 15                                   // winsize
#define FLOW_WIN_R (FLOW_WIN / 2)

static inline int flow_grid(long long n) {            // memory-bound, grid-stride: at most 8 blocks per CU
    const long long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// reflect-101 index ("mirror": d c b | a b c d | c b a), any distance from the image
__device__ __forceinline__ int flow_mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// source position of output index d when n_in samples are resized to n_out: src = (d + 0.5) n_in / n_out - 0.5 clipped to
// [0, n_in - 1], in exact integer arithmetic -> (i0, i1 = min(i0 + 1, n_in - 1), fraction rounded once to fp32)
__device__ __forceinline__ void flow_resize_src(int d, int n_in, int n_out, int& i0, int& i1, float& f) {
    const long long num = (long long)(2 * d + 1) * n_in - n_out;         // src * 2 n_out
    const long long den = 2ll * n_out;
    if (num <= 0) {
        i0 = 0;
        f = 0.f;
    } else {
        i0 = (int)(num / den);
        f = (float)(num - (long long)i0 * den) / (float)den;
    }
    if (i0 >= n_in - 1) {
        i0 = n_in - 1;
        f = 0.f;
    }
    i1 = min(i0 + 1, n_in - 1);
}

// ---- grey ------------------------------------------------------------------------------------------------------------
// bgr = 0: COLOR_RGB2GRAY of RGB pixels (scoring.py's TC as vdx/mdvqs.py states it); bgr = 1: COLOR_BGR2GRAY applied to the
// same bytes, i.e. channel 0 takes the blue weight (vdx/metrics.py:59 does that to the RGB frames, like the reference).
__global__ __launch_bounds__(256) void flow_grey_kernel(const unsigned char* frames, size_t fp, int rp, int H, int W, long long total,
                                                        int bgr, float* out) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const long long fy = idx / W;
        const int y = (int)(fy % H);
        const long long f = fy / H;
        const unsigned char* px = frames + (size_t)f * fp + (size_t)y * rp + (size_t)x * 3;
        const int c0 = px[0], g = px[1], c2 = px[2];
        const int r = bgr ? c2 : c0, b = bgr ? c0 : c2;
        out[idx] = (float)((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14);
    }
}
extern "C" int vdx_flow_grey_u8(const void* frames, size_t frame_pitch, int row_pitch, int F, int H, int W, int bgr, float* out,
                                vdx_stream_t stream) {
    VDX_CHECK(frames && out, "flow_grey: null pointer");
    VDX_CHECK(F > 0 && F <= 65536 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "flow_grey: F=%d H=%d W=%d", F, H, W);
    VDX_CHECK(row_pitch >= 3 * W && frame_pitch >= (size_t)row_pitch * H, "flow_grey: pitches too small");
    const long long total = (long long)F * H * W;
    hipLaunchKernelGGL(flow_grey_kernel, dim3(flow_grid(total)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)frames,
                       frame_pitch, row_pitch, H, W, total, bgr != 0, out);
    return vdx_launch_status("vdx_flow_grey_u8");
}

// ---- 1-D correlation, mirror border ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_corr1d_kernel(const float* in, float* out, long long total, int H, int W, const float* taps,
                                                          int radius, int axis) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const long long ny = idx / W;
        const int y = (int)(ny % H);
        const float* img = in + (size_t)(ny / H) * H * W;
        float acc = 0.f;
        if (axis == 0)
            for (int k = -radius; k <= radius; ++k) acc += taps[k + radius] * img[(size_t)flow_mirror(y + k, H) * W + x];
        else
            for (int k = -radius; k <= radius; ++k) acc += taps[k + radius] * img[(size_t)y * W + flow_mirror(x + k, W)];
        out[idx] = acc;
    }
}
extern "C" int vdx_flow_corr1d_f32(const float* in, float* out, int n_img, int H, int W, const float* taps, int radius, int axis,
                                   vdx_stream_t stream) {
    VDX_CHECK(in && out && in != out && taps, "flow_corr1d: null or aliased pointers");
    VDX_CHECK(n_img > 0 && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "flow_corr1d: n=%d H=%d W=%d", n_img, H, W);
    VDX_CHECK(radius >= 0 && radius <= 4096 && (axis == 0 || axis == 1), "flow_corr1d: radius=%d axis=%d", radius, axis);
    const long long total = (long long)n_img * H * W;
    hipLaunchKernelGGL(flow_corr1d_kernel, dim3(flow_grid(total)), dim3(256), 0, (hipStream_t)stream, in, out, total, H, W, taps, radius,
                       axis);
    return vdx_launch_status("vdx_flow_corr1d_f32");
}

// ---- bilinear resize of channels-last fp32 images ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_resize_kernel(const float* in, int Hi, int Wi, int C, float* out, int Ho, int Wo,
                                                          long long total, float mul) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C);
        const long long px = idx / C;
        const int x = (int)(px % Wo);
        const long long ny = px / Wo;
        const int y = (int)(ny % Ho);
        const float* img = in + (size_t)(ny / Ho) * Hi * Wi * C + c;
        int x0, x1, y0, y1;
        float fx, fy;
        flow_resize_src(x, Wi, Wo, x0, x1, fx);
        flow_resize_src(y, Hi, Ho, y0, y1, fy);
        const float a = img[((size_t)y0 * Wi + x0) * C], b = img[((size_t)y0 * Wi + x1) * C];
        const float cc = img[((size_t)y1 * Wi + x0) * C], d = img[((size_t)y1 * Wi + x1) * C];
        out[idx] = ((a * (1.f - fx) + b * fx) * (1.f - fy) + (cc * (1.f - fx) + d * fx) * fy) * mul;
    }
}
extern "C" int vdx_flow_resize_f32(const float* in, int n_img, int Hi, int Wi, int C, float* out, int Ho, int Wo, float mul,
                                   vdx_stream_t stream) {
    VDX_CHECK(in && out && in != out, "flow_resize: null or aliased pointers");
    VDX_CHECK(n_img > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && (C == 1 || C == 2), "flow_resize: n=%d %dx%d -> %dx%d C=%d", n_img, Hi,
              Wi, Ho, Wo, C);
    VDX_CHECK((long long)Hi * Wi * C < (1ll << 31) && (long long)Ho * Wo * C < (1ll << 31), "flow_resize: image too large");
    const long long total = (long long)n_img * Ho * Wo * C;
    hipLaunchKernelGGL(flow_resize_kernel, dim3(flow_grid(total)), dim3(256), 0, (hipStream_t)stream, in, Hi, Wi, C, out, Ho, Wo, total,
                       mul);
    return vdx_launch_status("vdx_flow_resize_f32");
}

// ---- polynomial expansion ---------------------------------------------------------------------------------------------
// `_poly_exp`: with k0 = g, k1 = g x, k2 = g x^2 (x = -5..5) the moments m = (k0 k0, k0 k1, k1 k0, k0 k2, k2 k0, k1 k1) as
// (row kernel) x (column kernel) correlations — columns first, then rows, mirror border — and r = inv(G) m; rows 1..5 of
// inv(G) give bx, by, axx, ayy, axy.  One 16 x 64 tile per block: the image tile with its halo of 5 in LDS (fp32, the input's
// own values), the three column passes in LDS as doubles (halo rows included: a mirrored row of a pass is the pass of the
// mirrored row), the row passes and the 5 x 6 product in double registers.  Every product and sum is fp64 with float64 tables:
// along a straight edge the planes feed 2 x 2 systems whose determinant cancels to ~1e-7 of its terms, and fp32 sums here moved
// such flows by a pixel.  Each result is rounded once to fp32.  out: [n][5][H][W].  LDS 47.6 KB: three workgroups per CU.
struct flow_poly_tab {
    double k[3][FLOW_POLY_TAPS];
    double ig[5][6];
};
#define POLY_TH 16
#define POLY_TW 64
#define POLY_IH (POLY_TH + 2 * FLOW_POLY_R)
#define POLY_IW (POLY_TW + 2 * FLOW_POLY_R)
__global__ __launch_bounds__(256) void flow_polyexp_kernel(const float* in, int H, int W, flow_poly_tab tab, float* out) {
    __shared__ float img[POLY_IH][POLY_IW];
    __shared__ double t[3][POLY_IH][POLY_TW];
    const int x0 = blockIdx.x * POLY_TW, y0 = blockIdx.y * POLY_TH;
    const float* src = in + (size_t)blockIdx.z * H * W;
    for (int i = threadIdx.x; i < POLY_IH * POLY_IW; i += 256) {
        const int ly = i / POLY_IW, lx = i - ly * POLY_IW;
        img[ly][lx] = src[(size_t)flow_mirror(y0 + ly - FLOW_POLY_R, H) * W + flow_mirror(x0 + lx - FLOW_POLY_R, W)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < POLY_IH * POLY_TW; i += 256) {
        const int ly = i / POLY_TW, lx = i - ly * POLY_TW;
        double s0 = 0., s1 = 0., s2 = 0.;
#pragma unroll
        for (int k = 0; k < FLOW_POLY_TAPS; ++k) {
            const double v = (double)img[ly][lx + k];
            s0 += tab.k[0][k] * v;
            s1 += tab.k[1][k] * v;
            s2 += tab.k[2][k] * v;
        }
        t[0][ly][lx] = s0;
        t[1][ly][lx] = s1;
        t[2][ly][lx] = s2;
    }
    __syncthreads();
    float* dst = out + (size_t)blockIdx.z * 5 * H * W;
    for (int i = threadIdx.x; i < POLY_TH * POLY_TW; i += 256) {
        const int ly = i / POLY_TW, lx = i - ly * POLY_TW;
        const int y = y0 + ly, x = x0 + lx;
        double m[6] = {0., 0., 0., 0., 0., 0.};                       // 1, x, y, xx, yy, xy
#pragma unroll
        for (int k = 0; k < FLOW_POLY_TAPS; ++k) {
            const double a = t[0][ly + k][lx], b = t[1][ly + k][lx], c = t[2][ly + k][lx];
            m[0] += tab.k[0][k] * a;
            m[2] += tab.k[1][k] * a;
            m[4] += tab.k[2][k] * a;
            m[1] += tab.k[0][k] * b;
            m[5] += tab.k[1][k] * b;
            m[3] += tab.k[0][k] * c;
        }
        if (y < H && x < W) {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                double r = 0.;
#pragma unroll
                for (int q = 0; q < 6; ++q) r += tab.ig[j][q] * m[q];
                dst[(size_t)j * H * W + (size_t)y * W + x] = (float)r;
            }
        }
    }
}
extern "C" int vdx_flow_polyexp_f32(const float* img, int n_img, int H, int W, const double* taps_host, const double* inv_g_host,
                                    float* out, vdx_stream_t stream) {
    VDX_CHECK(img && out && taps_host && inv_g_host, "flow_polyexp: null pointer");
    VDX_CHECK(n_img > 0 && n_img <= 65535 && H > 0 && W > 0 && (long long)H * W * 5 < (1ll << 31), "flow_polyexp: n=%d H=%d W=%d", n_img,
              H, W);
    flow_poly_tab tab;
    for (int i = 0; i < 3 * FLOW_POLY_TAPS; ++i) tab.k[i / FLOW_POLY_TAPS][i % FLOW_POLY_TAPS] = taps_host[i];
    for (int i = 0; i < 30; ++i) tab.ig[i / 6][i % 6] = inv_g_host[i];
    const dim3 grid((W + POLY_TW - 1) / POLY_TW, (H + POLY_TH - 1) / POLY_TH, n_img);
    VDX_CHECK(grid.y <= 65535, "flow_polyexp: H=%d too tall", H);
    hipLaunchKernelGGL(flow_polyexp_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, H, W, tab, out);
    return vdx_launch_status("vdx_flow_polyexp_f32");
}

// ---- one displacement update, all pairs ------------------------------------------------------------------------------------
// `_update_flow` with the box window.  Pair p takes R0 = expansion of frame p*step, R1 = of frame p*step + 1.  Per
// UPD_TH x 32 tile: the five products of every pixel of the tile and its halo of 7 (mirrored into the image) are formed from
// R0 at the pixel and R1 sampled bilinearly at the pixel + its flow (coordinates clamped, `_sample`) and staged in LDS; the
// 15 x 15 box mean runs there as 15 rows then 15 columns, each divided by 15; the 2 x 2 solve writes the new flow.  The product
// planes never reach memory.  R and the flows are fp32 in memory; everything between the loads and the final store is fp64
// (samples, products, both box passes, determinant, solve): det = g0 g2 - g1^2 + 1e-3 cancels to nothing in fp32 where the
// window sees one straight edge.  LDS: (5 x 46 x 47 + 5 x 32 x 47) doubles = 143 KB, so one workgroup per CU, of 1024 threads.
// Measured on an MI355X, temporal consistency of 24 frames of 576 x 1024 (fp32 kernels: 3.35 ms): this shape 5.40 ms; the same tile
// with 256 threads 12.3 ms; a 16 x 32 tile (84 KB, still one workgroup per CU) 9.2 ms with 512 threads, 13.4 ms with 256.
#define UPD_TH 32
#define UPD_TW 32
#define UPD_NT 1024                                   // threads: 16 waves hide the gather's latency in the one resident workgroup
#define UPD_SH (UPD_TH + 2 * FLOW_WIN_R)
#define UPD_SW (UPD_TW + 2 * FLOW_WIN_R)              // 46
#define UPD_LD (UPD_SW + 1)                           // odd row stride
#define UPD_LDS_BYTES ((5 * UPD_SH * UPD_LD + 5 * UPD_TH * UPD_LD) * (int)sizeof(double))
__device__ __forceinline__ double flow_bilerp(const float* p, int i00, int i01, int i10, int i11, double fx, double fy) {
    return ((double)p[i00] * (1. - fx) + (double)p[i01] * fx) * (1. - fy) + ((double)p[i10] * (1. - fx) + (double)p[i11] * fx) * fy;
}
__global__ __launch_bounds__(UPD_NT) void flow_update_kernel(const float* R, const float* fin, float* fout, int step, int H, int W) {
    extern __shared__ double lds[];
    double* comp = lds;                               // [5][UPD_SH][UPD_LD]
    double* vs = lds + 5 * UPD_SH * UPD_LD;           // [5][UPD_TH][UPD_LD]
    const int p = blockIdx.z, x0 = blockIdx.x * UPD_TW, y0 = blockIdx.y * UPD_TH;
    const size_t hw = (size_t)H * W;
    const float* R0 = R + (size_t)p * step * 5 * hw;
    const float* R1 = R0 + 5 * hw;
    const float* f0 = fin + (size_t)p * hw * 2;
    for (int i = threadIdx.x; i < UPD_SH * UPD_SW; i += UPD_NT) {
        const int ly = i / UPD_SW, lx = i - ly * UPD_SW;
        const int gy = flow_mirror(y0 + ly - FLOW_WIN_R, H), gx = flow_mirror(x0 + lx - FLOW_WIN_R, W);
        const int o = gy * W + gx;
        const double dx = (double)f0[2 * (size_t)o], dy = (double)f0[2 * (size_t)o + 1];
        const double sx = fmin(fmax((double)gx + dx, 0.), (double)(W - 1));
        const double sy = fmin(fmax((double)gy + dy, 0.), (double)(H - 1));
        const double flx = floor(sx), fly = floor(sy);
        const int ix = (int)flx, iy = (int)fly;       // a NaN flow clamps to 0 above (fmax), so both are in range
        const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
        const double fx = sx - flx, fy = sy - fly;
        const int i00 = iy * W + ix, i01 = iy * W + ix1, i10 = iy1 * W + ix, i11 = iy1 * W + ix1;
        const double bx1 = flow_bilerp(R1, i00, i01, i10, i11, fx, fy);
        const double by1 = flow_bilerp(R1 + hw, i00, i01, i10, i11, fx, fy);
        const double axx1 = flow_bilerp(R1 + 2 * hw, i00, i01, i10, i11, fx, fy);
        const double ayy1 = flow_bilerp(R1 + 3 * hw, i00, i01, i10, i11, fx, fy);
        const double axy1 = flow_bilerp(R1 + 4 * hw, i00, i01, i10, i11, fx, fy);
        const double bx0 = R0[o], by0 = R0[hw + o], axx0 = R0[2 * hw + o], ayy0 = R0[3 * hw + o], axy0 = R0[4 * hw + o];
        const double a11 = 0.5 * (axx0 + axx1), a22 = 0.5 * (ayy0 + ayy1), a12 = 0.25 * (axy0 + axy1);
        const double dbx = -0.5 * (bx1 - bx0) + a11 * dx + a12 * dy;
        const double dby = -0.5 * (by1 - by0) + a12 * dx + a22 * dy;
        const int l = ly * UPD_LD + lx;
        comp[l] = a11 * a11 + a12 * a12;
        comp[UPD_SH * UPD_LD + l] = a11 * a12 + a12 * a22;
        comp[2 * UPD_SH * UPD_LD + l] = a12 * a12 + a22 * a22;
        comp[3 * UPD_SH * UPD_LD + l] = a11 * dbx + a12 * dby;
        comp[4 * UPD_SH * UPD_LD + l] = a12 * dbx + a22 * dby;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < UPD_TH * UPD_SW; i += UPD_NT) {        // 15 rows, top to bottom
        const int r = i / UPD_SW, c = i - r * UPD_SW;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double* col = comp + q * UPD_SH * UPD_LD + r * UPD_LD + c;
            double s = 0.;
#pragma unroll
            for (int k = 0; k < FLOW_WIN; ++k) s += col[k * UPD_LD];
            vs[q * UPD_TH * UPD_LD + r * UPD_LD + c] = s / (double)FLOW_WIN;
        }
    }
    __syncthreads();
    float* out = fout + (size_t)p * hw * 2;
    for (int i = threadIdx.x; i < UPD_TH * UPD_TW; i += UPD_NT) {        // 15 columns, left to right, and the solve
        const int r = i / UPD_TW, c = i - r * UPD_TW;
        const int y = y0 + r, x = x0 + c;
        double g[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double* row = vs + q * UPD_TH * UPD_LD + r * UPD_LD + c;
            double s = 0.;
#pragma unroll
            for (int k = 0; k < FLOW_WIN; ++k) s += row[k];
            g[q] = s / (double)FLOW_WIN;
        }
        if (y < H && x < W) {
            const double det = g[0] * g[2] - g[1] * g[1] + 1e-3;
            const size_t o = ((size_t)y * W + x) * 2;
            out[o] = (float)((g[2] * g[3] - g[1] * g[4]) / det);
            out[o + 1] = (float)((g[0] * g[4] - g[1] * g[3]) / det);
        }
    }
}
extern "C" int vdx_flow_update_f32(const float* R, const float* flow_in, float* flow_out, int P, int step, int H, int W,
                                   vdx_stream_t stream) {
    VDX_CHECK(R && flow_in && flow_out && flow_in != flow_out, "flow_update: null or aliased pointers");
    VDX_CHECK(P > 0 && P <= 65535 && (step == 1 || step == 2), "flow_update: P=%d step=%d", P, step);
    VDX_CHECK(H >= 2 && W >= 2 && (long long)H * W * 5 < (1ll << 31), "flow_update: H=%d W=%d", H, W);
    static const hipError_t reserved = vdx_reserve_lds(UPD_LDS_BYTES, flow_update_kernel);
    VDX_CHECK(reserved == hipSuccess, "flow_update: cannot reserve %d bytes of LDS: %s", UPD_LDS_BYTES, hipGetErrorString(reserved));
    const dim3 grid((W + UPD_TW - 1) / UPD_TW, (H + UPD_TH - 1) / UPD_TH, P);
    VDX_CHECK(grid.y <= 65535, "flow_update: H=%d too tall", H);
    hipLaunchKernelGGL(flow_update_kernel, grid, dim3(UPD_NT), UPD_LDS_BYTES, (hipStream_t)stream, R, flow_in, flow_out, step, H, W);
    return vdx_launch_status("vdx_flow_update_f32");
}

// ---- per pair sum |flow| --------------------------------------------------------------------------------------------
// Stage 1: block (b, p) sums elements [b*chunk, (b+1)*chunk) of pair p, chunk = ceil(n / 64): lane-strided partial sums, one
// butterfly per wave, the 4 wave sums added in wave order.  Stage 2: one thread per pair adds its 64 partials in order.
#define ABS_BLOCKS 64
__global__ __launch_bounds__(256) void flow_abs_partial_kernel(const float* flow, long long n, long long chunk, float* partial) {
    __shared__ float part[4];
    const float* src = flow + (size_t)blockIdx.y * n;
    const long long i0 = (long long)blockIdx.x * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
    float s = 0.f;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) s += fabsf(src[i]);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * ABS_BLOCKS + blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}
__global__ __launch_bounds__(64) void flow_abs_final_kernel(const float* partial, int P, float* out) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    float s = 0.f;
    for (int b = 0; b < ABS_BLOCKS; ++b) s += partial[(size_t)p * ABS_BLOCKS + b];
    out[p] = s;
}
extern "C" int vdx_flow_abs_sum_f32(const float* flow, int P, size_t n, float* workspace, float* out, vdx_stream_t stream) {
    VDX_CHECK(flow && workspace && out, "flow_abs_sum: null pointer");
    VDX_CHECK(P > 0 && P <= 65535 && n > 0 && n < ((size_t)1 << 40), "flow_abs_sum: P=%d n=%zu", P, n);
    const long long chunk = ((long long)n + ABS_BLOCKS - 1) / ABS_BLOCKS;
    hipLaunchKernelGGL(flow_abs_partial_kernel, dim3(ABS_BLOCKS, P), dim3(256), 0, (hipStream_t)stream, flow, (long long)n, chunk,
                       workspace);
    hipLaunchKernelGGL(flow_abs_final_kernel, dim3((P + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const float*)workspace, P, out);
    return vdx_launch_status("vdx_flow_abs_sum_f32");
}

// ---- remap + absolute difference -----------------------------------------------------------------------------------------
// metrics.py:61-65: map = float32(pixel index + flow); cv2.remap(prev, map, INTER_LINEAR) with a constant-0 border, rounded
// half to even and clipped to uint8; then |warp - next| summed over all bytes.  The sums are integers (one 64-bit integer
// atomic per wave): exact whatever the order.  `warped` (optional) receives the warped frames, packed.
#define REMAP_BLOCKS 128
__global__ __launch_bounds__(256) void flow_remap_kernel(const unsigned char* frames, size_t fp, int rp, const float* flow, int step,
                                                         int H, int W, unsigned long long* absdiff, unsigned char* warped) {
    const int p = blockIdx.y;
    const unsigned char* prev = frames + (size_t)p * step * fp;
    const unsigned char* next = prev + fp;
    const float* fl = flow + (size_t)p * H * W * 2;
    const long long npx = (long long)H * W;
    unsigned long long d = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        const float mx = (float)x + fl[2 * i], my = (float)y + fl[2 * i + 1];
        int v[3] = {0, 0, 0};
        if (fabsf(mx) < 1e9f && fabsf(my) < 1e9f) {                      // NaN / inf / far away: every tap is outside -> 0
            const float flx = floorf(mx), fly = floorf(my);
            const int ix = (int)flx, iy = (int)fly;
            const float fx = mx - flx, fy = my - fly;
            const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy), w10 = (1.f - fx) * fy, w11 = fx * fy;
            const bool okx0 = (unsigned)ix < (unsigned)W, okx1 = (unsigned)(ix + 1) < (unsigned)W;
            const bool oky0 = (unsigned)iy < (unsigned)H, oky1 = (unsigned)(iy + 1) < (unsigned)H;
            const int cx0 = okx0 ? ix : 0, cx1 = okx1 ? ix + 1 : 0, cy0 = oky0 ? iy : 0, cy1 = oky1 ? iy + 1 : 0;   // loads stay in bounds
            const unsigned char* r0 = prev + (size_t)cy0 * rp;
            const unsigned char* r1 = prev + (size_t)cy1 * rp;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t00 = okx0 && oky0 ? (float)r0[cx0 * 3 + c] : 0.f, t01 = okx1 && oky0 ? (float)r0[cx1 * 3 + c] : 0.f;
                const float t10 = okx0 && oky1 ? (float)r1[cx0 * 3 + c] : 0.f, t11 = okx1 && oky1 ? (float)r1[cx1 * 3 + c] : 0.f;
                const float acc = (t00 * w00 + t01 * w01) + (t10 * w10 + t11 * w11);
                v[c] = (int)fminf(fmaxf(rintf(acc), 0.f), 255.f);
            }
        }
        const unsigned char* nx = next + (size_t)y * rp + (size_t)x * 3;
        d += (unsigned)(abs(v[0] - (int)nx[0]) + abs(v[1] - (int)nx[1]) + abs(v[2] - (int)nx[2]));
        if (warped) {
            unsigned char* w = warped + ((size_t)p * npx + i) * 3;
            w[0] = (unsigned char)v[0];
            w[1] = (unsigned char)v[1];
            w[2] = (unsigned char)v[2];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    if ((threadIdx.x & 63) == 0 && d) atomicAdd(&absdiff[p], d);
}
extern "C" int vdx_flow_remap_absdiff_u8(const void* frames, size_t frame_pitch, int row_pitch, const float* flow, int P, int step,
                                         int H, int W, uint64_t* absdiff, void* warped, vdx_stream_t stream) {
    VDX_CHECK(frames && flow && absdiff, "flow_remap: null pointer");
    VDX_CHECK(P > 0 && P <= 65535 && (step == 1 || step == 2), "flow_remap: P=%d step=%d", P, step);
    VDX_CHECK(H > 0 && W > 0 && (long long)H * W < (1ll << 30), "flow_remap: H=%d W=%d", H, W);
    VDX_CHECK(row_pitch >= 3 * W && frame_pitch >= (size_t)row_pitch * H, "flow_remap: pitches too small");
    const hipError_t e = hipMemsetAsync(absdiff, 0, (size_t)P * sizeof(uint64_t), (hipStream_t)stream);
    VDX_CHECK(e == hipSuccess, "flow_remap: memset failed: %s", hipGetErrorString(e));
    const long long blocks = ((long long)H * W + 255) / 256;
    hipLaunchKernelGGL(flow_remap_kernel, dim3((int)(blocks < REMAP_BLOCKS ? blocks : REMAP_BLOCKS), P), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)frames, frame_pitch, row_pitch, flow, step, H, W, (unsigned long long*)absdiff,
                       (unsigned char*)warped);
    return vdx_launch_status("vdx_flow_remap_absdiff_u8");
}
