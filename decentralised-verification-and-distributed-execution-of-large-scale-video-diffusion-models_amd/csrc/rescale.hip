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

// every block of a step kernel: the rows through LDS, added in ascending order (lane q adds column q), then sd_c, sd_g and r.
// Called by all 256 lanes before any of them leaves.  Block 0 of a grid whose y is 1 (the rescaled steps have ONE channel, the sample)
// also leaves the three scalars in `stats_out`.
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
        if (ra.stats_out && blockIdx.x == 0 && blockIdx.y == 0) {
            ra.stats_out[0] = sd_c;
            ra.stats_out[1] = sd_g;
            ra.stats_out[2] = r;
        }
    }
    __syncthreads();
    return ratio;
}

// the guidance policy of every rescaled step (step_common.h `direct_step_kernel`, cofuse_common.h `cofuse_step_kernel`): the block's
// r is its state, then g -> g' -> the sampler's tail
struct rescale_guidance {
    rescale_args ra;
    typedef float state;
    static constexpr bool uses_c = true;
    __device__ __forceinline__ state prologue(int) const { return rescale_ratio(ra); }
    template <int MODE>
    __device__ __forceinline__ void elem(float u, float c, float x, float x0p, const state& r, const ddim_coef& kd, const dpm_coef& kp,
                                         f16& x0, f16& o) const {
        const f16 g = cfg_combine(u, c, MODE == 0 ? kd.gs : kp.gs);
        const f16 g2 = cfg_rescale_elem(g, r, ra.phi, ra.phi1);
        if (MODE == 0) o = ddim_tail(g2, x, kd);
        else dpm_tail<MODE == 2>(g2, x, x0p, kp, x0, o);
    }
};

// ---- the statistics pass, over either noise source ---------------------------------------------------------------------------------
// The sample is ONE channel of the source: block b adds what the source hands it, in the source's order, into row b.  One buffer
// (`direct_source`): rows = the blocks of n / E vectors, at most 256.  Co-fused (`cofuse_source`, the clip as C T lines): rows =
// min(C T, 256).  Either way a block's partial depends on the shapes (and the table) alone.
template <class Src>
__global__ __launch_bounds__(256) void rescale_stats_kernel(Src src, float gs, double* partials) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    src.each(0, blockIdx.x, gridDim.x, [&](size_t, const f16 (&uf)[Src::width], const f16 (&cf)[Src::width]) {
#pragma unroll
        for (int j = 0; j < Src::width; ++j) stat_acc(a, (float)uf[j], (float)cf[j], gs);
    });
    block_row(a, partials + (size_t)blockIdx.x * 4);
}

// the launch of both statistics entries, whose own checks have passed: `src(E)` makes the noise source of access width E
template <class MakeSrc, size_t N>
static int rescale_stats_launch(const char* what, int e, int rows, MakeSrc&& src, float guidance, double* partials,
                                const co_buf (&inputs)[N], vdx_stream_t stream) {
    VDX_CHECK(partials && ((uintptr_t)partials & 15) == 0, "%s: partials must be a 16-byte aligned pointer", what);
    for (const co_buf& in : inputs)
        VDX_CHECK(!co_overlap(partials, (size_t)rows * 4 * sizeof(double), in.p, in.bytes), "%s: partials overlap an input", what);
    width_dispatch(e, [&](auto ee) {
        auto s = src(ee);
        hipLaunchKernelGGL(rescale_stats_kernel<decltype(s)>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, s, guidance, partials);
    });
    return vdx_launch_status(what);
}

static inline int rescale_check_phi(const char* what, float phi, float phi1) {
    VDX_CHECK(phi >= 0.f && phi <= 1.f && phi1 >= 0.f && phi1 <= 1.f, "%s: guidance rescale %g (and 1 - it, %g) must lie in [0, 1]",
              what, (double)phi, (double)phi1);
    return 0;
}

// stats_out is written (by one block): it may touch none of `bufs` (a null one is skipped)
template <size_t N>
static inline int rescale_stats_out_free(const char* what, const void* stats_out, const co_buf (&bufs)[N]) {
    if (stats_out)
        for (const co_buf& b : bufs)
            VDX_CHECK(!b.p || !co_overlap(stats_out, 3 * sizeof(f16), b.p, b.bytes), "%s: stats_out overlaps another buffer", what);
    return 0;
}

// ---- one sample in one buffer: eps2 = [u; c], n elements each, E halves per access (n is a multiple of E) ---------------------
static inline int rescale_width(size_t n) { return n % 8 == 0 ? 8 : n % 4 == 0 ? 4 : 1; }

// rows of `partials` = blocks of the statistics launch: a function of n alone
static inline int rescale_rows(size_t n) {
    const size_t nv = n / rescale_width(n), want = (nv + 255) / 256;
    return (int)(want < RESCALE_MAX_ROWS ? want : RESCALE_MAX_ROWS);
}

extern "C" int vdx_cfg_rescale_rows(size_t n) { return n > 0 && n <= ((size_t)1 << 40) ? rescale_rows(n) : 0; }

extern "C" int vdx_cfg_rescale_stats_f16(const void* eps2, size_t n, float guidance, double* partials, vdx_stream_t stream) {
    const char* what = "vdx_cfg_rescale_stats_f16";
    VDX_CHECK(eps2 && n > 0, "%s: bad arguments", what);
    VDX_CHECK(n <= ((size_t)1 << 40), "%s: n too large", what);
    VDX_CHECK(((uintptr_t)eps2 & 15) == 0, "%s: pointer not 16-byte aligned", what);
    const co_buf inputs[] = {{eps2, 2 * n * sizeof(f16)}};
    const auto src = [&](auto ee) { return direct_source<decltype(ee)::value>{(const f16*)eps2, n, n}; };
    return rescale_stats_launch(what, rescale_width(n), rescale_rows(n), src, guidance, partials, inputs, stream);
}

static int rescale_step_launch(const char* what, int mode, const void* eps2, const void* lat, const void* x0_prev, void* x0_out,
                               void* lat_out, const double* partials, void* stats_out, float phi, float phi1, ddim_coef kd,
                               dpm_coef kp, size_t n, vdx_stream_t stream) {
    VDX_CHECK(partials && n > 0, "%s: bad arguments", what);
    VDX_CHECK(n <= ((size_t)1 << 40), "%s: n too large", what);
    if (int rc = rescale_check_phi(what, phi, phi1)) return rc;
    const int rows = rescale_rows(n);
    const size_t nb = n * sizeof(f16), pb = (size_t)rows * 4 * sizeof(double);
    const co_buf extra[] = {{partials, pb}, {stats_out, 3 * sizeof(f16)}}, read[] = {{eps2, 2 * nb}, {lat, nb}, {partials, pb}, {x0_prev, nb}};
    if (int rc = rescale_stats_out_free(what, stats_out, read)) return rc;
    const rescale_args ra = {partials, (f16*)stats_out, rows, (double)n, phi, phi1};
    return direct_launch(what, mode, false, eps2, lat, x0_prev, x0_out, lat_out, extra, kd, kp, rescale_guidance{ra}, 1, n, 4096, stream);
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
    const co_buf inputs[] = {{windows, windows_elems * sizeof(f16)}, {wn, (size_t)K * T * sizeof(float)}};
    const auto src = [&](auto ee) {
        return cofuse_source<decltype(ee)::value>{(const f16*)windows, tab, K, wn, C, T, HW, (unsigned)C * (unsigned)T};
    };
    return rescale_stats_launch(what, e, cofuse_rescale_rows(C, T), src, guidance, partials, inputs, stream);
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
    const size_t nb = (size_t)C * T * HW * sizeof(f16), pb = (size_t)rows * 4 * sizeof(double);
    VDX_CHECK(!co_overlap(partials, pb, lat_out, nb) && (!x0_out || !co_overlap(partials, pb, x0_out, nb)),
              "%s: partials overlap an output", what);
    const co_buf all[] = {{z, nb}, {lat_out, nb}, {windows, windows_elems * sizeof(f16)}, {wn, (size_t)K * T * sizeof(float)},
                          {partials, pb}, {x0_prev, nb}, {x0_out, nb}};
    if (int rc = rescale_stats_out_free(what, stats_out, all)) return rc;
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
