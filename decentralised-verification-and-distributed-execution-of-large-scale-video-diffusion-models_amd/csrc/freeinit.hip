// freeinit.hip — the frequency mix of FreeInit (Wu et al. 2023; diffusers' free_init_utils) for a batch of 3-D volumes (no
// reference counterpart: the reference samples once from white noise).  vdx/freeinit.py drives it; tests/freeinit_ref.py states
// the definition in float64 with torch.fft and the tests pin these kernels to it.  For one volume z (fp16) and eta (fp32) of
// extent (T, h, w) and a filter table H (fp32, fftshift-ed coordinates):
//
//   out = fp16( Re ifftn( ifftshift( fftshift(fftn(z)) H + fftshift(fftn(eta)) (1 - H) ) ) )
//       = fp16( eta + Re IDFT3( H' . DFT3(z - eta) ) / (T h w) ),       H'[k] = H[(k + N / 2) mod N] on every axis
//
// The second form is what runs: separable direct DFTs, five launches over one complex workspace of the volumes' size, each in
// place.  The arithmetic and the workspace are fp64: the result must round to the restatement's fp16 value, and where it is
// near zero fp16's spacing is 2^-24 = 6e-8, while fp32 sums of this length are off by 3e-7 (measured: 6 to 9 fp16 ulp at such
// elements of the (24, 72, 128) volume, 1.2e-3 to 1.7e-3 of all elements rounding to another value).  The transforms are about
// 3 GFLOP at that volume, at a rate the vector units sustain in fp64 as in fp32.
//   1. d = z - eta, DFT along w      (real in, complex out)
//   2. DFT along h
//   3. DFT along T, times H', inverse DFT along T          (one kernel: the T column never leaves LDS in between)
//   4. inverse DFT along h
//   5. inverse DFT along w, real part only, eta + sum / (T h w), fp16
// A block stages a tile of TC lines of its axis in LDS as x[n][line] (row stride TC + 1 elements: the transposing accesses of
// the w passes, lanes along n, then step an odd number of elements and spread over the banks instead of meeting one; the
// compute reads, lanes along the line, are consecutive).  Lanes own lines and lane groups own output frequencies k, so the twiddle
// of a step is one address per group (a broadcast) and the line data one conflict-free read.  Twiddles are one host-built
// table per axis length, e^(-2 pi i j / N) evaluated in float64, indexed by (k n) mod N kept as a running integer: no angle
// is ever formed on the device.  N TC <= 1024 elements per buffer and two buffers: at most 56 KiB of LDS, two or more
// blocks per CU.
// Every output is one sum over its own line in ascending n with one accumulator, no atomics: the same bits on every run,
// for any number of volumes and whichever tile a line falls in.  No index or branch depends on the data.
#include "vdx_common.h"

#define FI_THREADS 256
#define FI_MAX_N 512                                  // per axis
#define FI_TILE_ELEMS 1024                            // N * TC of one LDS buffer
#define FI_MAX_ELEMS (1ll << 30)                      // n_vol * T * h * w

static inline int fi_tile_lines(int N) {              // a power of two, 64 .. 2
    int tc = 64;
    while (tc > 1 && N * tc > FI_TILE_ELEMS) tc >>= 1;
    return tc;
}
static inline size_t fi_lds_bytes(int N, int TC) { return ((size_t)N + 2 * (size_t)N * (TC + 1)) * sizeof(double2); }

// the tile of a block: element (n, line) lies at base + n * sn + line * sp, for line < nlines
struct fi_tile {
    size_t base, sn, sp;
    int nlines;
};
// an axis of stride `inner` inside `outer` slabs: the lines are the `inner` positions of a slab, TC consecutive ones per tile
__device__ __forceinline__ fi_tile fi_tile_strided(int N, int TC, int inner, int& first) {
    const int tiles = (inner + TC - 1) / TC;
    const int o = blockIdx.x / tiles;
    first = (blockIdx.x - o * tiles) * TC;
    fi_tile t;
    t.base = (size_t)o * N * inner + first, t.sn = (size_t)inner, t.sp = 1, t.nlines = min(TC, inner - first);
    return t;
}
// the contiguous axis: the lines are rows of N, TC consecutive rows per tile
__device__ __forceinline__ fi_tile fi_tile_rows(int N, int TC, size_t rows) {
    const size_t r0 = (size_t)blockIdx.x * TC;
    fi_tile t;
    t.base = r0 * N, t.sn = 1, t.sp = (size_t)N, t.nlines = (int)min((size_t)TC, rows - r0);
    return t;
}
// f(n, line, address, inside) for every element of the TC-line tile, lanes along the unit stride in memory
template <class F>
__device__ __forceinline__ void fi_for_each(const fi_tile& t, int N, int TC, F f) {
    if (t.sp == 1) {
        for (int i = threadIdx.x; i < N * TC; i += FI_THREADS) {
            const int line = i & (TC - 1), n = i / TC;
            f(n, line, t.base + (size_t)n * t.sn + line, line < t.nlines);
        }
    } else {
        for (int i = threadIdx.x; i < N * TC; i += FI_THREADS) {
            const int line = i / N, n = i - line * N;
            f(n, line, t.base + (size_t)line * t.sp + n, line < t.nlines);
        }
    }
}
__device__ __forceinline__ void fi_load_twiddles(double2* tw, const double2* tw_g, int N) {
    for (int i = threadIdx.x; i < N; i += FI_THREADS) tw[i] = tw_g[i];
}

// y[k][line] = sum_n x[n][line] w^(k n), w = tw[1] (forward) or its conjugate (INV); g(k, line) scales the result
template <bool INV, class G>
__device__ __forceinline__ void fi_dft_cc(const double2* x, double2* y, const double2* tw, int N, int TC, G g) {
    const int TCP = TC + 1, line = threadIdx.x & (TC - 1);
    for (int k = threadIdx.x / TC; k < N; k += FI_THREADS / TC) {
        double re = 0.0, im = 0.0;
        int j = 0;                                                       // (k n) mod N
        for (int n = 0; n < N; ++n) {
            const double2 a = x[n * TCP + line], c = tw[j];
            const double s = INV ? -c.y : c.y;
            re = fma(a.x, c.x, re), re = fma(-a.y, s, re);
            im = fma(a.x, s, im), im = fma(a.y, c.x, im);
            j += k;
            if (j >= N) j -= N;
        }
        const double m = g(k, line);
        y[k * TCP + line] = make_double2(re * m, im * m);
    }
}
// real input xr[n][line] -> complex y, forward
__device__ __forceinline__ void fi_dft_rc(const double* xr, double2* y, const double2* tw, int N, int TC) {
    const int TCP = TC + 1, line = threadIdx.x & (TC - 1);
    for (int k = threadIdx.x / TC; k < N; k += FI_THREADS / TC) {
        double re = 0.0, im = 0.0;
        int j = 0;
        for (int n = 0; n < N; ++n) {
            const double a = xr[n * TCP + line];
            const double2 c = tw[j];
            re = fma(a, c.x, re), im = fma(a, c.y, im);
            j += k;
            if (j >= N) j -= N;
        }
        y[k * TCP + line] = make_double2(re, im);
    }
}
// complex input -> the real part of the inverse, yr[k][line]
__device__ __forceinline__ void fi_dft_cr(const double2* x, double* yr, const double2* tw, int N, int TC) {
    const int TCP = TC + 1, line = threadIdx.x & (TC - 1);
    for (int k = threadIdx.x / TC; k < N; k += FI_THREADS / TC) {
        double re = 0.0;
        int j = 0;
        for (int n = 0; n < N; ++n) {
            const double2 a = x[n * TCP + line], c = tw[j];
            re = fma(a.x, c.x, re), re = fma(a.y, c.y, re);             // Re (a conj(c')) with c' = (c.x, -c.y)
            j += k;
            if (j >= N) j -= N;
        }
        yr[k * TCP + line] = re;
    }
}

#define FI_LDS(N, TC)                                                           \
    extern __shared__ __attribute__((aligned(16))) unsigned char fi_lds[];      \
    double2* const tw = (double2*)fi_lds;                                         \
    double2* const xa = tw + (N);                                                \
    double2* const xb = xa + (size_t)(N) * ((TC) + 1)

// 1. d = z - eta and the forward DFT along w: rows of w, real in, complex out
__global__ __launch_bounds__(FI_THREADS) void fi_fwd_w_kernel(const f16* z, const float* eta, const double2* tw_g, int N, int TC,
                                                              size_t rows, double2* ws) {
    FI_LDS(N, TC);
    const int TCP = TC + 1;
    double* const xr = (double*)xa;
    fi_load_twiddles(tw, tw_g, N);
    const fi_tile t = fi_tile_rows(N, TC, rows);
    fi_for_each(t, N, TC, [&](int n, int line, size_t a, bool in) { xr[n * TCP + line] = in ? (double)(float)z[a] - (double)eta[a] : 0.0; });
    __syncthreads();
    fi_dft_rc(xr, xb, tw, N, TC);
    __syncthreads();
    fi_for_each(t, N, TC, [&](int n, int line, size_t a, bool in) {
        if (in) ws[a] = xb[n * TCP + line];
    });
}

// 2. and 4. the DFT along h, forward or inverse, in place: `outer` slabs of (N, inner)
template <bool INV>
__global__ __launch_bounds__(FI_THREADS) void fi_axis_kernel(double2* ws, const double2* tw_g, int N, int TC, int inner) {
    FI_LDS(N, TC);
    const int TCP = TC + 1;
    fi_load_twiddles(tw, tw_g, N);
    int first;
    const fi_tile t = fi_tile_strided(N, TC, inner, first);
    fi_for_each(t, N, TC, [&](int n, int line, size_t a, bool in) { xa[n * TCP + line] = in ? ws[a] : make_double2(0.0, 0.0); });
    __syncthreads();
    fi_dft_cc<INV>(xa, xb, tw, N, TC, [](int, int) { return 1.0; });
    __syncthreads();
    fi_for_each(t, N, TC, [&](int n, int line, size_t a, bool in) {
        if (in) ws[a] = xb[n * TCP + line];
    });
}

// 3. forward DFT along T, times H' = ifftshift(H), inverse DFT along T, in place: per volume (T, h w)
__global__ __launch_bounds__(FI_THREADS) void fi_t_filter_kernel(double2* ws, const double2* tw_g, const float* filt, int T, int TC, int h,
                                                                 int w) {
    FI_LDS(T, TC);
    const int TCP = TC + 1, hw = h * w;
    fi_load_twiddles(tw, tw_g, T);
    int first;
    const fi_tile t = fi_tile_strided(T, TC, hw, first);
    fi_for_each(t, T, TC, [&](int n, int line, size_t a, bool in) { xa[n * TCP + line] = in ? ws[a] : make_double2(0.0, 0.0); });
    __syncthreads();
    const int p = min(first + (int)(threadIdx.x & (TC - 1)), hw - 1);      // this lane's (ky, kx); lines past the slab are not stored
    int fy = p / w + h / 2, fx = p % w + w / 2;
    if (fy >= h) fy -= h;
    if (fx >= w) fx -= w;
    const float* const frow = filt + (size_t)fy * w + fx;
    fi_dft_cc<false>(xa, xb, tw, T, TC, [&](int k, int) {
        int ft = k + T / 2;
        if (ft >= T) ft -= T;
        return (double)frow[(size_t)ft * hw];
    });
    __syncthreads();
    fi_dft_cc<true>(xb, xa, tw, T, TC, [](int, int) { return 1.0; });
    __syncthreads();
    fi_for_each(t, T, TC, [&](int n, int line, size_t a, bool in) {
        if (in) ws[a] = xa[n * TCP + line];
    });
}

// 5. the real part of the inverse DFT along w, eta + sum * scale, fp16
__global__ __launch_bounds__(FI_THREADS) void fi_inv_w_kernel(const double2* ws, const float* eta, const double2* tw_g, int N, int TC,
                                                              size_t rows, double scale, f16* out) {
    FI_LDS(N, TC);
    const int TCP = TC + 1;
    double* const yr = (double*)xb;
    fi_load_twiddles(tw, tw_g, N);
    const fi_tile t = fi_tile_rows(N, TC, rows);
    fi_for_each(t, N, TC, [&](int n, int line, size_t a, bool in) { xa[n * TCP + line] = in ? ws[a] : make_double2(0.0, 0.0); });
    __syncthreads();
    fi_dft_cr(xa, yr, tw, N, TC);
    __syncthreads();
    fi_for_each(t, N, TC, [&](int n, int line, size_t a, bool in) {
        if (in) out[a] = (f16)fma(yr[n * TCP + line], scale, (double)eta[a]);
    });
}

static inline bool fi_sizes_ok(int n_vol, int T, int h, int w) {
    return n_vol >= 1 && T >= 1 && h >= 1 && w >= 1 && T <= FI_MAX_N && h <= FI_MAX_N && w <= FI_MAX_N &&
           (long long)n_vol * T * h * w <= FI_MAX_ELEMS;
}

extern "C" size_t vdx_freeinit_workspace(int n_vol, int T, int h, int w) {
    return fi_sizes_ok(n_vol, T, h, w) ? (size_t)n_vol * T * h * w * sizeof(double2) : 0;
}

extern "C" int vdx_freeinit_mix_f16(const void* z_t, const float* eta, const float* filt, const double* tw_t, const double* tw_h,
                                    const double* tw_w, int n_vol, int T, int h, int w, void* workspace, size_t workspace_bytes,
                                    void* out, vdx_stream_t stream) {
    VDX_CHECK(fi_sizes_ok(n_vol, T, h, w), "freeinit_mix: n_vol=%d T=%d h=%d w=%d (each axis 1..%d, at most 2^30 elements)", n_vol, T, h,
              w, FI_MAX_N);
    VDX_CHECK(z_t && eta && filt && tw_t && tw_h && tw_w && workspace && out, "freeinit_mix: null pointer");
    VDX_CHECK(workspace_bytes >= vdx_freeinit_workspace(n_vol, T, h, w), "freeinit_mix: workspace of %zu bytes is too small",
              workspace_bytes);
    VDX_CHECK((size_t)workspace % 16 == 0 && (size_t)tw_t % 16 == 0 && (size_t)tw_h % 16 == 0 && (size_t)tw_w % 16 == 0,
              "freeinit_mix: workspace and twiddle tables must be 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    double2* const ws = (double2*)workspace;
    const size_t rows = (size_t)n_vol * T * h;
    const int tc_w = fi_tile_lines(w), tc_h = fi_tile_lines(h), tc_t = fi_tile_lines(T);
    const int grid_w = (int)((rows + tc_w - 1) / tc_w);
    const int grid_h = n_vol * T * ((w + tc_h - 1) / tc_h);
    const int grid_t = n_vol * ((h * w + tc_t - 1) / tc_t);
    hipLaunchKernelGGL(fi_fwd_w_kernel, dim3(grid_w), dim3(FI_THREADS), fi_lds_bytes(w, tc_w), s, (const f16*)z_t, eta,
                       (const double2*)tw_w, w, tc_w, rows, ws);
    if (h > 1)                                                            // a DFT of length 1 is the identity
        hipLaunchKernelGGL(fi_axis_kernel<false>, dim3(grid_h), dim3(FI_THREADS), fi_lds_bytes(h, tc_h), s, ws, (const double2*)tw_h, h,
                           tc_h, w);
    hipLaunchKernelGGL(fi_t_filter_kernel, dim3(grid_t), dim3(FI_THREADS), fi_lds_bytes(T, tc_t), s, ws, (const double2*)tw_t, filt, T,
                       tc_t, h, w);
    if (h > 1)
        hipLaunchKernelGGL(fi_axis_kernel<true>, dim3(grid_h), dim3(FI_THREADS), fi_lds_bytes(h, tc_h), s, ws, (const double2*)tw_h, h,
                           tc_h, w);
    const double scale = 1.0 / ((double)T * h * w);
    hipLaunchKernelGGL(fi_inv_w_kernel, dim3(grid_w), dim3(FI_THREADS), fi_lds_bytes(w, tc_w), s, (const double2*)ws, eta,
                       (const double2*)tw_w, w, tc_w, rows, scale, (f16*)out);
    return vdx_launch_status("vdx_freeinit_mix_f16");
}
