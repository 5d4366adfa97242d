// rescale.hip — classifier-free guidance with the CFG rescale of Lin et al. 2023 (section 3.4 of "Common Diffusion Noise Schedules
// and Sample Steps are Flawed"; diffusers `rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale)`), fused into the
// sampler steps.  Opt-in (`DiffuserConfig.guidance_rescale`, vdx/scheduler.py); without it nothing here runs.  A "sample" is what
// one scheduler step advances: a window's latent, or with co-denoising the whole clip's.  fp16 tensors, every line a rounding:
//
//   g    = rn16(u + rn16(gs * rn16(c - u)))                                   the combine of every fused step (step_chains.h)
//   S1c, S2c, S1g, S2g = sum c, sum c*c, sum g, sum g*g                       fp64 sums over the sample's N elements
//   var(x) = (N*S2 - S1*S1) / (N*(N - 1))                                     fp64, every operation rounded on its own (no fma):
//                                                                             the unbiased variance, exactly 0 for a constant x
//   sd_c = rn16(sqrt(var(c))),  sd_g = rn16(sqrt(var(g)))                     fp64 sqrt, ONE rounding to fp16
//   r    = rn16(fp32(sd_c) / fp32(sd_g))                                      one scalar per sample
//   g'   = rn16(rn16(phi * rn16(g * r)) + rn16(phi1 * g))                     phi = fp32(rescale), phi1 = fp32(1 - rescale)
// and g' takes g's place in the DDIM / DPM-Solver++ tail (step_chains.h).  Nothing is clamped and nothing branches on data: N = 1,
// sd_g = 0, a NaN or an infinity give the NaN or infinity the lines above give, in that sample only.
//
// Two launches per step, and r never leaves the device:
//   1. statistics: every block adds its elements into four fp64 sums (per lane in a fixed stride order, the wave's 64 lanes by
//      a shuffle tree, the four waves through LDS in ascending order) and writes ONE row [4] of `partials`.  The number of rows
//      is a function of the shapes alone and at most 256; there are no atomics and no "last block".
//   2. step: every block fetches the rows (<= 8 KiB out of L2, one per lane), adds them in ascending order, forms sd_c, sd_g and r itself, and runs the
//      element chain.  Block 0 also leaves [sd_c, sd_g, r] in `stats_out` when one is given (tests read it; the loop never does).
// The same order of additions on every run and every rank: the same bits.
//
// The co-fused variants take the windows' raw UNet outputs as codenoise.hip's steps do, fuse U and Cc through the same function
// (cofuse_common.h) in both launches, and take the statistics of the fused Cc and of g(U, Cc) over the whole clip.  Their step is
// codenoise.hip's kernel and launcher (cofuse_common.h `cofuse_step_kernel`, `cofuse_launch`) with `rescale_guidance` as its policy.
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"
#include "cofuse_common.h"

#define RESCALE_MAX_ROWS 256

struct rescale_args {
    const double* partials;     // [rows][4]: S1c, S2c, S1g, S2g of each statistics block
    f16* stats_out;             // [3] or null
    int rows;
    double n;                   // N, exact in fp64 (the launchers bound it)
    float phi, phi1;
};

// one element into a lane's four sums; c*c and g*g are exact in fp32 (11-bit significands, no overflow)
__device__ __forceinline__ void stat_acc(double (&a)[4], float u, float c, float gs) {
    const float g = (float)cfg_combine(u, c, gs);
    a[0] += (double)c;
    a[1] += (double)__fmul_rn(c, c);
    a[2] += (double)g;
    a[3] += (double)__fmul_rn(g, g);
}

// the block's 256 lanes' sums -> row[4]: a shuffle tree inside each wave, then the four waves in ascending order
__device__ __forceinline__ void block_row(double (&a)[4], double* row) {
    __shared__ double w[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a[q] += __shfl_down(a[q], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < 4; ++q) w[threadIdx.x >> 6][q] = a[q];
    __syncthreads();
    if (threadIdx.x < 4) row[threadIdx.x] = ((w[0][threadIdx.x] + w[1][threadIdx.x]) + w[2][threadIdx.x]) + w[3][threadIdx.x];
}

// every block of a step kernel: the rows through LDS, added in ascending order (lane q adds column q), then sd_c, sd_g and r.
// Called by all 256 lanes before any of them leaves.
__device__ __forceinline__ float rescale_ratio(const rescale_args& ra) {
    __shared__ double rowbuf[RESCALE_MAX_ROWS][4];
    __shared__ double s[4];
    __shared__ float ratio;
    if ((int)threadIdx.x < ra.rows) {                             // lane t fetches row t (rows <= 256 lanes): the loads go out together
#pragma unroll
        for (int q = 0; q < 4; ++q) rowbuf[threadIdx.x][q] = ra.partials[threadIdx.x * 4 + q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double acc = rowbuf[0][threadIdx.x];
#pragma unroll 8
        for (int row = 1; row < ra.rows; ++row) acc += rowbuf[row][threadIdx.x];
        s[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double den = ra.n * (ra.n - 1.0);
        const f16 sd_c = (f16)sqrt((ra.n * s[1] - s[0] * s[0]) / den);
        const f16 sd_g = (f16)sqrt((ra.n * s[3] - s[2] * s[2]) / den);
        const f16 r = rn16(__fdiv_rn((float)sd_c, (float)sd_g));
        ratio = (float)r;
        if (ra.stats_out && blockIdx.x == 0) {
            ra.stats_out[0] = sd_c;
            ra.stats_out[1] = sd_g;
            ra.stats_out[2] = r;
        }
    }
    __syncthreads();
    return ratio;
}

// g -> g' -> the sampler's tail.  MODE 0: DDIM; 1: DPM-Solver++ first order; 2: second order
template <int MODE>
__device__ __forceinline__ void rescale_step_elem(float u, float c, float x, float x0p, float r, const rescale_args& ra,
                                                  const ddim_coef& kd, const dpm_coef& kp, f16& x0_out, f16& out) {
    const f16 g = cfg_combine(u, c, MODE == 0 ? kd.gs : kp.gs);
    const f16 g2 = cfg_rescale_elem(g, r, ra.phi, ra.phi1);
    if (MODE == 0) out = ddim_tail(g2, x, kd);
    else dpm_tail<MODE == 2>(g2, x, x0p, kp, x0_out, out);
}

// the guidance policy of the co-fused step (cofuse_common.h `cofuse_step_kernel`): the block's r, then g' in g's place
struct rescale_guidance {
    rescale_args ra;
    __device__ __forceinline__ float prologue() const { return rescale_ratio(ra); }
    template <int MODE>
    __device__ __forceinline__ void elem(float u, float c, float x, float x0p, float r, const ddim_coef& kd, const dpm_coef& kp, f16& x0,
                                         f16& o) const {
        rescale_step_elem<MODE>(u, c, x, x0p, r, ra, kd, kp, x0, o);
    }
};

// ---- one sample in one buffer: eps2 = [u; c], n elements each, E halves per access (n is a multiple of E) ---------------------
template <int E>
__global__ __launch_bounds__(256) void rescale_stats_kernel(const f16* eps, float gs, double* partials, size_t n) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    const size_t nv = n / E, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
        f16 u[E], c[E];
        load_halves<E>(eps + v * E, u);
        load_halves<E>(eps + n + v * E, c);
#pragma unroll
        for (int j = 0; j < E; ++j) stat_acc(a, (float)u[j], (float)c[j], gs);
    }
    block_row(a, partials + (size_t)blockIdx.x * 4);
}

template <int MODE, int E>
__global__ __launch_bounds__(256) void rescale_step_kernel(const f16* eps, const f16* lat, const f16* x0_prev, f16* x0_out, f16* out,
                                                           ddim_coef kd, dpm_coef kp, rescale_args ra, size_t n) {
    const float r = rescale_ratio(ra);
    const size_t nv = n / E, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
        const size_t i = v * E;
        f16 u[E], c[E], x[E], xp[E], o[E], x0[E];
        load_halves<E>(eps + i, u);
        load_halves<E>(eps + n + i, c);
        load_halves<E>(lat + i, x);
        if (MODE == 2) load_halves<E>(x0_prev + i, xp);
#pragma unroll
        for (int j = 0; j < E; ++j)
            rescale_step_elem<MODE>((float)u[j], (float)c[j], (float)x[j], MODE == 2 ? (float)xp[j] : 0.f, r, ra, kd, kp, x0[j], o[j]);
        if (MODE != 0) store_halves<E>(x0_out + i, x0);
        store_halves<E>(out + i, o);
    }
}

static inline int rescale_width(size_t n) { return n % 8 == 0 ? 8 : n % 4 == 0 ? 4 : 1; }

// rows of `partials` = blocks of the statistics launch: a function of n alone
static inline int rescale_rows(size_t n) {
    const size_t nv = n / rescale_width(n), want = (nv + 255) / 256;
    return (int)(want < RESCALE_MAX_ROWS ? want : RESCALE_MAX_ROWS);
}

static inline int rescale_check_phi(const char* what, float phi, float phi1) {
    VDX_CHECK(phi >= 0.f && phi <= 1.f && phi1 >= 0.f && phi1 <= 1.f, "%s: guidance rescale %g (and 1 - it, %g) must lie in [0, 1]",
              what, (double)phi, (double)phi1);
    return 0;
}

extern "C" int vdx_cfg_rescale_rows(size_t n) { return n > 0 && n <= ((size_t)1 << 40) ? rescale_rows(n) : 0; }

extern "C" int vdx_cfg_rescale_stats_f16(const void* eps2, size_t n, float guidance, double* partials, vdx_stream_t stream) {
    const char* what = "vdx_cfg_rescale_stats_f16";
    VDX_CHECK(eps2 && partials && n > 0, "%s: bad arguments", what);
    VDX_CHECK(n <= ((size_t)1 << 40), "%s: n too large", what);
    VDX_CHECK(((uintptr_t)eps2 & 15) == 0 && ((uintptr_t)partials & 15) == 0, "%s: pointer not 16-byte aligned", what);
    const int rows = rescale_rows(n);
    VDX_CHECK(!co_overlap(partials, (size_t)rows * 4 * sizeof(double), eps2, 2 * n * sizeof(f16)), "%s: partials overlap eps2", what);
    const dim3 grid((unsigned)rows), block(256);
    const hipStream_t s = (hipStream_t)stream;
    const f16* e = (const f16*)eps2;
    switch (rescale_width(n)) {
    case 8: hipLaunchKernelGGL(rescale_stats_kernel<8>, grid, block, 0, s, e, guidance, partials, n); break;
    case 4: hipLaunchKernelGGL(rescale_stats_kernel<4>, grid, block, 0, s, e, guidance, partials, n); break;
    default: hipLaunchKernelGGL(rescale_stats_kernel<1>, grid, block, 0, s, e, guidance, partials, n); break;
    }
    return vdx_launch_status(what);
}

static int rescale_step_launch(const char* what, int mode, const void* eps2, const void* lat, const void* x0_prev, void* x0_out,
                               void* lat_out, const double* partials, void* stats_out, float phi, float phi1, ddim_coef kd,
                               dpm_coef kp, size_t n, vdx_stream_t stream) {
    VDX_CHECK(eps2 && lat && lat_out && partials && n > 0 && (mode == 0 || x0_out), "%s: bad arguments", what);
    VDX_CHECK(n <= ((size_t)1 << 40), "%s: n too large", what);
    if (int rc = rescale_check_phi(what, phi, phi1)) return rc;
    const size_t nb = n * sizeof(f16);
    for (const void* p : {eps2, lat, x0_prev, (const void*)x0_out, (const void*)lat_out, (const void*)partials, (const void*)stats_out})
        VDX_CHECK(((uintptr_t)p & 15) == 0, "%s: pointer not 16-byte aligned", what);
    const int rows = rescale_rows(n);
    const size_t pb = (size_t)rows * 4 * sizeof(double), sb = 3 * sizeof(f16);
    // a lane reads its elements before it writes them, and writes nobody else's: lat_out == lat is fine, nothing else may share
    VDX_CHECK(lat_out == lat || !co_overlap(lat_out, nb, lat, nb), "%s: lat_out overlaps lat without being lat", what);
    VDX_CHECK(!co_overlap(lat_out, nb, eps2, 2 * nb) && !co_overlap(lat_out, nb, partials, pb), "%s: lat_out overlaps an input", what);
    if (stats_out)
        VDX_CHECK(!co_overlap(stats_out, sb, eps2, 2 * nb) && !co_overlap(stats_out, sb, lat, nb) && !co_overlap(stats_out, sb, lat_out, nb) &&
                      !co_overlap(stats_out, sb, partials, pb) && (!x0_prev || !co_overlap(stats_out, sb, x0_prev, nb)) &&
                      (!x0_out || !co_overlap(stats_out, sb, x0_out, nb)),
                  "%s: stats_out overlaps another buffer", what);
    if (mode != 0) {
        VDX_CHECK(!x0_prev || x0_out != x0_prev, "%s: x0_out must not be x0_prev (ping-pong two history buffers)", what);
        VDX_CHECK(!co_overlap(x0_out, nb, lat_out, nb) && !co_overlap(x0_out, nb, lat, nb) && !co_overlap(x0_out, nb, eps2, 2 * nb) &&
                      !co_overlap(x0_out, nb, partials, pb),
                  "%s: x0_out overlaps an input or lat_out", what);
        VDX_CHECK(!x0_prev || (!co_overlap(x0_prev, nb, x0_out, nb) && !co_overlap(x0_prev, nb, lat_out, nb)),
                  "%s: x0_prev overlaps an output", what);
    }
    const int e = rescale_width(n);
    const size_t nv = n / e, want = (nv + 255) / 256;
    const dim3 grid((unsigned)(want < 4096 ? want : 4096)), block(256);
    const hipStream_t s = (hipStream_t)stream;
    const rescale_args ra = {partials, (f16*)stats_out, rows, (double)n, phi, phi1};
    const f16 *ep = (const f16*)eps2, *x = (const f16*)lat, *p = (const f16*)x0_prev;
    f16 *z = (f16*)x0_out, *o = (f16*)lat_out;
    step_dispatch(mode, x0_prev, e, [&](auto m, auto ee) {
        hipLaunchKernelGGL((rescale_step_kernel<decltype(m)::value, decltype(ee)::value>), grid, block, 0, s, ep, x, p, z, o, kd, kp, ra, n);
    });
    return vdx_launch_status(what);
}

extern "C" int vdx_cfg_rescale_ddim_step_f16(const void* eps2, const void* lat, void* lat_out, const double* partials, void* stats_out,
                                             float guidance, float phi, float phi1, float sqrt_one_minus_at, float sqrt_at,
                                             float sqrt_aprev, float sqrt_one_minus_aprev, size_t n, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return rescale_step_launch("vdx_cfg_rescale_ddim_step_f16", 0, eps2, lat, nullptr, nullptr, lat_out, partials, stats_out, phi, phi1,
                               kd, dpm_coef{}, n, stream);
}

extern "C" int vdx_cfg_rescale_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                                            const double* partials, void* stats_out, float guidance, float phi, float phi1, float c_s0,
                                            float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, size_t n,
                                            vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return rescale_step_launch("vdx_cfg_rescale_dpm_step_f16", 1, eps2, lat, x0_prev, x0_out, lat_out, partials, stats_out, phi, phi1,
                               ddim_coef{}, kp, n, stream);
}

// ---- co-denoising: the sample is the whole clip, its noise fused from the windows' outputs ------------------------------------
// Statistics: block b takes the (c, t) lines b, b + rows, ...; a lane the elements p = (lane + 256 j) E of each.  rows = min(C T,
// 256): the partial of a block depends on the shapes and the table alone.
template <int E>
__global__ __launch_bounds__(256) void cofuse_stats_kernel(const f16* win, cofuse_tab tab, int K, const float* wn, float gs,
                                                           double* partials, int C, int T, int HW) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    const unsigned lines = (unsigned)C * (unsigned)T;
    for (unsigned line = blockIdx.x; line < lines; line += gridDim.x) {
        const int c = (int)(line / (unsigned)T), t = (int)(line - (unsigned)c * (unsigned)T);
        for (int p = (int)threadIdx.x * E; p < HW; p += 256 * E) {
            float uf[E], cf[E];
            cofuse_uc<E>(win, tab, K, wn, C, T, HW, c, t, p, uf, cf);
#pragma unroll
            for (int j = 0; j < E; ++j) stat_acc(a, uf[j], cf[j], gs);
        }
    }
    block_row(a, partials + (size_t)blockIdx.x * 4);
}

static inline int cofuse_rescale_rows(int C, int T) {
    const size_t lines = (size_t)C * T;
    return (int)(lines < RESCALE_MAX_ROWS ? lines : RESCALE_MAX_ROWS);
}

extern "C" int vdx_cofuse_cfg_rescale_rows(int C, int T) {
    return C > 0 && T > 0 && (size_t)C * T <= (size_t)1 << 30 ? cofuse_rescale_rows(C, T) : 0;
}

extern "C" int vdx_cofuse_cfg_rescale_stats_f16(const void* windows, size_t windows_elems, const int64_t* win_off, const int* win_start,
                                                const int* win_len, int K, const float* wn, float guidance, double* partials, int C,
                                                int T, int HW, vdx_stream_t stream) {
    const char* what = "vdx_cofuse_cfg_rescale_stats_f16";
    cofuse_tab tab;
    int e;
    if (int rc = cofuse_check(what, 0, false, nullptr, windows, windows_elems, win_off, win_start, win_len, K, wn, nullptr, nullptr,
                              nullptr, C, T, HW, tab, e))
        return rc;
    VDX_CHECK(partials && ((uintptr_t)partials & 15) == 0, "%s: partials must be a 16-byte aligned pointer", what);
    const int rows = cofuse_rescale_rows(C, T);
    const size_t pb = (size_t)rows * 4 * sizeof(double);
    VDX_CHECK(!co_overlap(partials, pb, windows, windows_elems * sizeof(f16)) && !co_overlap(partials, pb, wn, (size_t)K * T * sizeof(float)),
              "%s: partials overlap an input", what);
    const dim3 grid((unsigned)rows), block(256);
    const hipStream_t st = (hipStream_t)stream;
    const f16* ww = (const f16*)windows;
    if (e == 8) hipLaunchKernelGGL(cofuse_stats_kernel<8>, grid, block, 0, st, ww, tab, K, wn, guidance, partials, C, T, HW);
    else if (e == 4) hipLaunchKernelGGL(cofuse_stats_kernel<4>, grid, block, 0, st, ww, tab, K, wn, guidance, partials, C, T, HW);
    else hipLaunchKernelGGL(cofuse_stats_kernel<1>, grid, block, 0, st, ww, tab, K, wn, guidance, partials, C, T, HW);
    return vdx_launch_status(what);
}

static int cofuse_rescale_launch(const char* what, int mode, const void* z, const void* windows, size_t windows_elems,
                                 const int64_t* win_off, const int* win_start, const int* win_len, int K, const float* wn,
                                 const void* x0_prev, void* x0_out, void* lat_out, const double* partials, void* stats_out, float phi,
                                 float phi1, ddim_coef kd, dpm_coef kp, int C, int T, int HW, vdx_stream_t stream) {
    cofuse_tab tab;
    int e;
    if (int rc = cofuse_check(what, mode, true, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev, x0_out, lat_out,
                              C, T, HW, tab, e))
        return rc;
    if (int rc = rescale_check_phi(what, phi, phi1)) return rc;
    VDX_CHECK(partials && ((uintptr_t)partials & 15) == 0 && ((uintptr_t)stats_out & 15) == 0,
              "%s: partials must be a 16-byte aligned pointer, stats_out one or null", what);
    const int rows = cofuse_rescale_rows(C, T);
    const size_t nb = (size_t)C * T * HW * sizeof(f16), pb = (size_t)rows * 4 * sizeof(double), sb = 3 * sizeof(f16);
    const size_t wb = windows_elems * sizeof(f16);
    VDX_CHECK(!co_overlap(partials, pb, lat_out, nb) && (!x0_out || !co_overlap(partials, pb, x0_out, nb)),
              "%s: partials overlap an output", what);
    if (stats_out)
        VDX_CHECK(!co_overlap(stats_out, sb, z, nb) && !co_overlap(stats_out, sb, lat_out, nb) && !co_overlap(stats_out, sb, windows, wb) &&
                      !co_overlap(stats_out, sb, wn, (size_t)K * T * sizeof(float)) && !co_overlap(stats_out, sb, partials, pb) &&
                      (!x0_prev || !co_overlap(stats_out, sb, x0_prev, nb)) && (!x0_out || !co_overlap(stats_out, sb, x0_out, nb)),
                  "%s: stats_out overlaps another buffer", what);
    const rescale_args ra = {partials, (f16*)stats_out, rows, (double)((size_t)C * T * HW), phi, phi1};
    return cofuse_launch<false>(what, mode, z, windows, tab, e, K, wn, x0_prev, x0_out, lat_out, kd, kp, rescale_guidance{ra}, C, T, HW,
                                stream);
}

extern "C" int vdx_cofuse_cfg_rescale_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                                    const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                                    const double* partials, void* stats_out, float guidance, float phi, float phi1,
                                                    float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                                    float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return cofuse_rescale_launch("vdx_cofuse_cfg_rescale_ddim_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len, K, wn,
                                 nullptr, nullptr, lat_out, partials, stats_out, phi, phi1, kd, dpm_coef{}, C, T, HW, stream);
}

extern "C" int vdx_cofuse_cfg_rescale_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                                   const int* win_start, const int* win_len, int K, const float* wn,
                                                   const void* x0_prev, void* x0_out, void* lat_out, const double* partials,
                                                   void* stats_out, float guidance, float phi, float phi1, float c_s0, float c_inv_a0,
                                                   float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW,
                                                   vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return cofuse_rescale_launch("vdx_cofuse_cfg_rescale_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len, K, wn,
                                 x0_prev, x0_out, lat_out, partials, stats_out, phi, phi1, ddim_coef{}, kp, C, T, HW, stream);
}
