// freeu.hip — FreeU (Si et al. 2023; diffusers' enable_freeu, unpinned) on the UNet's row layout (no reference counterpart: the
// reference never touches the up path).  vdx/unet3d.py calls both kernels before every ResNet of up blocks 0 and 1;
// tests/freeu_ref.py states the definition in float64 with torch.fft and the tests pin these kernels to it.
//
// The skip filter.  For one image's plane x (H, W) of one channel and a scale s, diffusers' fourier_filter with threshold 1 is
//
//   out = fp16( Re ifft2( ifftshift( fftshift(fft2(x)) . M ) ) ),      M = 1 except M[H/2 - 1 : H/2 + 1, W/2 - 1 : W/2 + 1] = s
//
// Under fftshift index N / 2 is frequency 0 and N / 2 - 1 is frequency -1, so M differs from 1 at the frequencies
// K_H x K_W with K_N = {0, N - 1} (one element for N = 1; the whole axis for N = 2), and
//
//   out[y, x] = fp16( x[y, x] + (s - 1) / (H W) . Re sum_{ky in K_H, kx in K_W} X(ky, kx) e^{+2 pi i (ky y / H + kx x / W)} )
//   X(ky, kx) = sum_{y, x} x[y, x] e^{-2 pi i (ky y / H + kx x / W)}
//
// which is what runs: at most four complex coefficients per plane, no FFT.  Frequency -1 is scaled without +1, so the sum is
// not real and the real part is taken.
// One block owns one image and FU_CT consecutive channels of the rows [n_img][H W][C]: lanes along the channels (the unit
// stride), the block's four waves along the positions.  Pass 1: wave g sums the positions g, g + 4, ... in ascending order
// into four fp64 accumulators per lane; the four partial sums meet in LDS and every lane adds them in the order of g.  Pass 2:
// the same lanes read their elements again (the tile was just read: L2), add the correction in fp64 and round once to fp16.
// A block reads and writes only its own elements and has read all of them before it writes one, so out == x is allowed.
// The plane never lies in LDS: no plane size is refused and there is one path for all of them.
// Twiddles are one host-built table per axis, e^(-2 pi i j / N) evaluated in float64, indexed by (k n) mod N in integers
// ((N - 1) n mod N = (N - n) mod N): no angle is formed on the device.  The sums are fp64 because the result must round to the
// restatement's fp16 value and fp32 sums of this length miss it by several ulp where it is near zero (csrc/freeinit.hip).
// No atomics, one fixed summation order per plane whatever n_img is: the same bits on every run and for any batching.  No
// index or branch depends on the data: NaN and inf run like any value and stay inside their plane.
// An element whose corrected fp64 value equals its input keeps the input's bits (s = 1: the identity, -0 included).
//
// The backbone scale.  fp16(fp32(x) fp32(b)) on channels [0, C / 2) of every row, in place: torch's half-by-scalar multiply.
#include "vdx_common.h"

#define FU_THREADS 256
#define FU_CT 64                                      // channels of a block: one per lane of a wave
#define FU_GROUPS (FU_THREADS / FU_CT)                // waves of a block, along the positions

// e^{-2 pi i k n / N} for k = N - 1 (frequency -1) at position n: entry (N - n) mod N of the axis' table
__device__ __forceinline__ double2 fu_twiddle(const double2* tw, int n, int N) { return tw[n == 0 ? 0 : N - n]; }

__global__ __launch_bounds__(FU_THREADS) void fu_filter_kernel(const f16* x, size_t ldx, const double2* tw_h, const double2* tw_w, int H,
                                                               int W, int C, int ctiles, double coef, f16* out, size_t ldo) {
    __shared__ double part[FU_GROUPS][7][FU_CT];
    const int lane = threadIdx.x & (FU_CT - 1), g = threadIdx.x / FU_CT;
    const int img = blockIdx.x / ctiles, c = (blockIdx.x - img * ctiles) * FU_CT + lane;
    const int P = H * W;
    const bool in = c < C;
    const size_t row0 = (size_t)img * P;
    // pass 1: X(0, 0) (real), X(0, -1), X(-1, 0), X(-1, -1) over this wave's positions
    double s00 = 0.0, s01r = 0.0, s01i = 0.0, s10r = 0.0, s10i = 0.0, s11r = 0.0, s11i = 0.0;
    for (int p = g; p < P; p += FU_GROUPS) {
        const int py = p / W, px = p - py * W;
        const double2 wy = fu_twiddle(tw_h, py, H), wx = fu_twiddle(tw_w, px, W);
        const double wr = wy.x * wx.x - wy.y * wx.y, wi = wy.x * wx.y + wy.y * wx.x;
        const double a = in ? (double)(float)x[(row0 + p) * ldx + c] : 0.0;
        s00 += a;
        s01r = fma(a, wx.x, s01r), s01i = fma(a, wx.y, s01i);
        s10r = fma(a, wy.x, s10r), s10i = fma(a, wy.y, s10i);
        s11r = fma(a, wr, s11r), s11i = fma(a, wi, s11i);
    }
    part[g][0][lane] = s00, part[g][1][lane] = s01r, part[g][2][lane] = s01i, part[g][3][lane] = s10r;
    part[g][4][lane] = s10i, part[g][5][lane] = s11r, part[g][6][lane] = s11i;
    __syncthreads();
    double S[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        double v = part[0][k][lane];
#pragma unroll
        for (int j = 1; j < FU_GROUPS; ++j) v += part[j][k][lane];
        S[k] = v;
    }
    // an axis of length 1 has the one frequency 0: its "-1" is the same coefficient and is not counted again
    const bool hx = W > 1, hy = H > 1;
    // pass 2: Re(X conj(w)) = X.re w.re + X.im w.im with w the forward twiddle of the position
    for (int p = g; p < P; p += FU_GROUPS) {
        const int py = p / W, px = p - py * W;
        const double2 wy = fu_twiddle(tw_h, py, H), wx = fu_twiddle(tw_w, px, W);
        const double wr = wy.x * wx.x - wy.y * wx.y, wi = wy.x * wx.y + wy.y * wx.x;
        if (in) {
            const f16 v = x[(row0 + p) * ldx + c];
            const double a = (double)(float)v;
            double corr = S[0];
            if (hx) corr += fma(S[1], wx.x, S[2] * wx.y);
            if (hy) corr += fma(S[3], wy.x, S[4] * wy.y);
            if (hx && hy) corr += fma(S[5], wr, S[6] * wi);
            const double r = fma(corr, coef, a);
            out[(row0 + p) * ldo + c] = r == a ? v : (f16)r;
        }
    }
}

// fp16(fp32(x) b).  The product is kept out of the compiler's sight before it is rounded: folded into one mixed-precision fma
// with a +0 addend, -0 b came out as +0.
__device__ __forceinline__ f16 fu_scaled(f16 x, float b) {
    float p = (float)x * b;
    asm volatile("" : "+v"(p));
    return (f16)p;
}

// channels [0, half) of every row; VEC: eight channels per lane (half % 8 == 0, ld % 8 == 0, x 16-byte aligned)
template <bool VEC>
__global__ __launch_bounds__(FU_THREADS) void fu_scale_kernel(f16* x, size_t ld, size_t rows, int half, float b) {
    const int per_row = VEC ? half / 8 : half;
    const size_t n = rows * per_row;
    for (size_t i = (size_t)blockIdx.x * FU_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * FU_THREADS) {
        const size_t r = i / per_row;
        const int j = (int)(i - r * per_row);
        if (VEC) {
            f16x8* const q = (f16x8*)(x + r * ld) + j;
            f16x8 v = *q;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = fu_scaled(v[k], b);
            *q = v;
        } else {
            f16* const q = x + r * ld + j;
            *q = fu_scaled(*q, b);
        }
    }
}

extern "C" int vdx_freeu_filter_f16(const void* x, int ldx, const double* tw_h, const double* tw_w, int n_img, int H, int W, int C,
                                    double s, void* out, int ldo, vdx_stream_t stream) {
    VDX_CHECK(n_img >= 1 && H >= 1 && W >= 1 && C >= 1, "freeu_filter: n_img=%d H=%d W=%d C=%d (each at least 1)", n_img, H, W, C);
    VDX_CHECK((long long)H * W <= 0x7fffffffll, "freeu_filter: a plane of %d x %d positions", H, W);
    VDX_CHECK(x && out && tw_h && tw_w, "freeu_filter: null pointer");
    VDX_CHECK(ldx >= C && ldo >= C, "freeu_filter: row strides %d, %d below C=%d", ldx, ldo, C);
    VDX_CHECK((size_t)tw_h % 16 == 0 && (size_t)tw_w % 16 == 0, "freeu_filter: twiddle tables must be 16-byte aligned");
    VDX_CHECK(s == s && s - s == 0.0, "freeu_filter: s must be finite");
    const int ctiles = (C + FU_CT - 1) / FU_CT;
    VDX_CHECK((long long)n_img * ctiles <= 0x7fffffffll, "freeu_filter: %d images x %d channel tiles", n_img, ctiles);
    const double coef = (s - 1.0) / ((double)H * (double)W);
    hipLaunchKernelGGL(fu_filter_kernel, dim3(n_img * ctiles), dim3(FU_THREADS), 0, (hipStream_t)stream, (const f16*)x, (size_t)ldx,
                       (const double2*)tw_h, (const double2*)tw_w, H, W, C, ctiles, coef, (f16*)out, (size_t)ldo);
    return vdx_launch_status("vdx_freeu_filter_f16");
}

extern "C" int vdx_freeu_scale_f16(void* x, int ld, size_t rows, int C, float b, vdx_stream_t stream) {
    VDX_CHECK(rows >= 1 && C >= 1 && ld >= C, "freeu_scale: rows=%zu C=%d ld=%d", rows, C, ld);
    VDX_CHECK(x, "freeu_scale: null pointer");
    VDX_CHECK(b == b && b - b == 0.0f && b > 0.0f, "freeu_scale: b must be finite and positive");
    const int half = C / 2;
    if (half == 0) return 0;                                       // C = 1: no channel below C / 2
    const bool vec = half % 8 == 0 && ld % 8 == 0 && (size_t)x % 16 == 0;
    const size_t n = rows * (size_t)(vec ? half / 8 : half);
    const size_t blocks = (n + FU_THREADS - 1) / FU_THREADS, cap = (size_t)vdx_num_cus() * 16;
    const int grid = (int)(blocks < cap ? blocks : cap);
    if (vec)
        hipLaunchKernelGGL(fu_scale_kernel<true>, dim3(grid), dim3(FU_THREADS), 0, (hipStream_t)stream, (f16*)x, (size_t)ld, rows, half, b);
    else
        hipLaunchKernelGGL(fu_scale_kernel<false>, dim3(grid), dim3(FU_THREADS), 0, (hipStream_t)stream, (f16*)x, (size_t)ld, rows, half,
                           b);
    return vdx_launch_status("vdx_freeu_scale_f16");
}
