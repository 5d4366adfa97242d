// dynthresh.hip — dynamic thresholding of the guided noise with a mimic scale (the "Dynamic Thresholding (CFG Scale Fix)" of the
// A1111 / ComfyUI world: Imagen's dynamic thresholding moved from pixels to the guided noise), fused into the sampler steps.
// Opt-in (`DiffuserConfig.cfg_mimic`, vdx/scheduler.py); without it nothing here runs.  Restated, not pinned externally: the lines
// below ARE the specification (tests/dynthresh_ref.py).  A "sample" is what one scheduler step advances: a window's latent, or
// with co-denoising the whole clip's, shape (C, T, h, w); M = T h w; a channel is the M elements of one c.  fp16 tensors, every
// line a rounding; gs the guidance scale, ms the mimic scale, q the percentile in (0, 1]:
//
//   g   = cfg_combine(u, c, gs)        l = cfg_combine(u, c, ms)                the combine of every fused step (step_chains.h), twice
//   Sg[ch] = sum g,  Sl[ch] = sum l                                             fp64 sums over the channel, fixed order
//   mg  = fp16(Sg / M),  ml = fp16(Sl / M)                                      one fp64 division, ONE rounding to fp16
//   d   = rn16(g - mg)                 e = rn16(l - ml)
//   ref_lo = max over the channel of |e|, compared as the integer bits(e) & 0x7fff (a NaN pattern is above infinity's and wins)
//   a[0..M-1] = the channel's bits(d) & 0x7fff in ascending integer order
//   pos = q (M - 1) in float64,  k = floor(pos),  f = fp32(pos - k),  lo = a[k],  hi = a[min(k + 1, M - 1)]
//   ref_hi = lo's bits when f == 0, else rn16(lo + rn32(f * rn32(hi - lo)))
//   s   = whichever of ref_lo, ref_hi has the larger bit pattern
//   dc  = d > s ? s : (d < -s ? -s : d)                                         float compares: a NaN d stays NaN
//   g'  = rn16(rn16(rn16(dc / s) * ref_lo) + mg)                                a division, no reciprocal (step_chains.h `cfg_mimic_elem`)
// and g' takes g's place in the DDIM / DPM-Solver++ tail.  Nothing else is clamped and nothing branches on data: a constant channel
// has s = 0 and gives the NaN the lines give; NaN and infinity stay in their channel of their sample.
//
// The quantile needs no sort: |x| of an fp16 has 32 768 bit patterns, so a histogram over them, built with integer atomics, holds
// the exact order statistics whatever order the adds arrive in.  Four launches per step, and nothing leaves the device:
//   1. sums: rescale.hip's scheme per channel (per lane in a fixed stride order, the wave's 64 lanes by a shuffle tree, the four
//      waves through LDS in ascending order, ONE row [Sg, Sl] per block; the rows per channel are a function of the shapes alone,
//      <= 64; no atomics, no "last block").  It also zeroes this step's histogram and max words: the workspace may hold anything.
//   2. histogram: every block adds its channel's rows in ascending order, forms mg and ml, recomputes g, l, d, e per element, counts
//      bits(d) & 0x7fff into hist[C][32768] (global bins; a lane adds a run of equal bins at once, as gif.hip's histogram does) and
//      folds bits(e) & 0x7fff into maxbits[C] (one atomicMax per wave).
//   3. select: one block per channel scans the 32 768 counts for a[k] and a[min(k + 1, M - 1)] (k and f come from the host) and
//      writes scal[ch] = (mg, ref_lo, ref_hi, s), four halves.
//   4. step: per element g and d again, `cfg_mimic_elem`, the sampler's tail.
// The workspace, `vdx_cfg_mimic_ws_bytes(C, T, HW)` bytes from a 16-byte aligned base, every part at a multiple of 16:
//   scal f16 [C][4] | maxbits u32 [C] | partials f64 [C][64][2] | hist u32 [C][32768]
//
// The co-fused variants take the windows' raw UNet outputs as codenoise.hip's steps do, fuse U and Cc through the same function
// (cofuse_common.h) in launches 1, 2 and 4, and take the statistics over the whole clip.  Their step is codenoise.hip's kernel and
// launcher (`cofuse_step_kernel`, `cofuse_launch`) with `mimic_guidance` as its policy: a block owns one (c, t) line, so the
// channel's scalars are uniform over it.
#include <cmath>
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"
#include "cofuse_common.h"

#define MIMIC_BINS 32768
#define MIMIC_MAX_ROWS 64

struct mimic_ws {
    f16* scal;                  // [C][4]: mg, ref_lo, ref_hi, s
    uint32_t* maxbits;          // [C]
    double* partials;           // [C][MIMIC_MAX_ROWS][2]: Sg, Sl of each sums block
    uint32_t* hist;             // [C][MIMIC_BINS]
};

static inline size_t mimic_up16(size_t v) { return (v + 15) & ~(size_t)15; }

static inline size_t mimic_layout(void* base, int C, mimic_ws& w) {
    char* p = (char*)base;
    const size_t o_max = mimic_up16((size_t)C * 4 * sizeof(f16));
    const size_t o_part = o_max + mimic_up16((size_t)C * sizeof(uint32_t));
    const size_t o_hist = o_part + (size_t)C * MIMIC_MAX_ROWS * 2 * sizeof(double);
    w.scal = (f16*)p;
    w.maxbits = (uint32_t*)(p + o_max);
    w.partials = (double*)(p + o_part);
    w.hist = (uint32_t*)(p + o_hist);
    return o_hist + (size_t)C * MIMIC_BINS * sizeof(uint32_t);
}

__device__ __forceinline__ uint32_t abs_bits(f16 h) { return (uint32_t)(__builtin_bit_cast(unsigned short, h) & 0x7fffu); }
__device__ __forceinline__ f16 half_of_bits(uint32_t b) { return __builtin_bit_cast(f16, (unsigned short)b); }

// one element into a lane's two sums
__device__ __forceinline__ void sum_acc(double (&a)[2], float u, float c, float gs, float ms) {
    a[0] += (double)(float)cfg_combine(u, c, gs);
    a[1] += (double)(float)cfg_combine(u, c, ms);
}

// one element's two bins: bits(d) & 0x7fff and bits(e) & 0x7fff
__device__ __forceinline__ void mimic_bins(float u, float c, float gs, float ms, float mg, float ml, uint32_t& db, uint32_t& eb) {
    const f16 g = cfg_combine(u, c, gs), l = cfg_combine(u, c, ms);
    db = abs_bits(rn16(__fsub_rn((float)g, mg)));
    eb = abs_bits(rn16(__fsub_rn((float)l, ml)));
}

// the block's 256 lanes' sums -> row[2]: a shuffle tree inside each wave, then the four waves in ascending order
__device__ __forceinline__ void block_row2(double (&a)[2], double* row) {
    __shared__ double w[4][2];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a[q] += __shfl_down(a[q], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < 2; ++q) w[threadIdx.x >> 6][q] = a[q];
    __syncthreads();
    if (threadIdx.x < 2) row[threadIdx.x] = ((w[0][threadIdx.x] + w[1][threadIdx.x]) + w[2][threadIdx.x]) + w[3][threadIdx.x];
}

// the sums launch's second duty: block x of `nx` of channel ch zeroes its share of the channel's bins, block 0 the max word
__device__ __forceinline__ void mimic_zero(const mimic_ws& w, unsigned ch, unsigned x, unsigned nx) {
    uint32_t* h = w.hist + (size_t)ch * MIMIC_BINS;
    for (unsigned b = x * 256u + threadIdx.x; b < MIMIC_BINS; b += nx * 256u) h[b] = 0u;
    if (x == 0 && threadIdx.x == 0) w.maxbits[ch] = 0u;
}

// every block of launches 2 and 3: the channel's rows through LDS, added in ascending order (lane q adds column q), then the two
// means.  Called by all 256 lanes before any of them leaves.
__device__ __forceinline__ void channel_means(const double* rows, int nrows, double m, float& mg, float& ml) {
    __shared__ double rowbuf[MIMIC_MAX_ROWS][2];
    __shared__ float mean[2];
    if ((int)threadIdx.x < nrows) {
        rowbuf[threadIdx.x][0] = rows[threadIdx.x * 2];
        rowbuf[threadIdx.x][1] = rows[threadIdx.x * 2 + 1];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double acc = rowbuf[0][threadIdx.x];
        for (int row = 1; row < nrows; ++row) acc += rowbuf[row][threadIdx.x];
        mean[threadIdx.x] = (float)(f16)(acc / m);                // one fp64 division, ONE rounding to fp16
    }
    __syncthreads();
    mg = mean[0];
    ml = mean[1];
}

// a lane's E bins into the channel's histogram, a run of equal bins in one add; its E max candidates into mx
template <int E>
__device__ __forceinline__ void hist_add(uint32_t* h, const uint32_t (&db)[E], const uint32_t (&eb)[E], uint32_t& mx) {
    uint32_t run = db[0], len = 1;
    mx = eb[0] > mx ? eb[0] : mx;
#pragma unroll
    for (int j = 1; j < E; ++j) {
        mx = eb[j] > mx ? eb[j] : mx;
        if (db[j] == run) {
            ++len;
        } else {
            atomicAdd(h + run, len);
            run = db[j];
            len = 1;
        }
    }
    atomicAdd(h + run, len);
}

// the lanes' maxima -> the channel's word: a shuffle tree inside each wave (all 64 lanes arrive), one integer atomicMax per wave
__device__ __forceinline__ void max_fold(uint32_t* word, uint32_t mx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(word, mx);
}

// ---- one sample in one buffer: eps2 = [u; c], C channels of M elements each, E halves per access (M is a multiple of E) --------
// grid (rows, C): block x of channel y takes the vectors x * 256 + lane + j * rows * 256
template <int E>
__global__ __launch_bounds__(256) void mimic_sums_kernel(const f16* eps, float gs, float ms, mimic_ws w, size_t M, size_t n) {
    const unsigned ch = blockIdx.y;
    mimic_zero(w, ch, blockIdx.x, gridDim.x);
    double a[2] = {0.0, 0.0};
    const f16* up = eps + (size_t)ch * M;
    const size_t nv = M / E, stride = (size_t)gridDim.x * 256;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) {
        f16 u[E], c[E];
        load_halves<E>(up + v * E, u);
        load_halves<E>(up + n + v * E, c);
#pragma unroll
        for (int j = 0; j < E; ++j) sum_acc(a, (float)u[j], (float)c[j], gs, ms);
    }
    block_row2(a, w.partials + ((size_t)ch * MIMIC_MAX_ROWS + blockIdx.x) * 2);
}

template <int E>
__global__ __launch_bounds__(256) void mimic_hist_kernel(const f16* eps, float gs, float ms, mimic_ws w, int nrows, size_t M, size_t n) {
    const unsigned ch = blockIdx.y;
    float mg, ml;
    channel_means(w.partials + (size_t)ch * MIMIC_MAX_ROWS * 2, nrows, (double)M, mg, ml);
    uint32_t* h = w.hist + (size_t)ch * MIMIC_BINS;
    uint32_t mx = 0;
    const f16* up = eps + (size_t)ch * M;
    const size_t nv = M / E, stride = (size_t)gridDim.x * 256;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) {
        f16 u[E], c[E];
        load_halves<E>(up + v * E, u);
        load_halves<E>(up + n + v * E, c);
        uint32_t db[E], eb[E];
#pragma unroll
        for (int j = 0; j < E; ++j) mimic_bins((float)u[j], (float)c[j], gs, ms, mg, ml, db[j], eb[j]);
        hist_add<E>(h, db, eb, mx);
    }
    max_fold(w.maxbits + ch, mx);
}

// one block per channel: lane t owns the bins [128 t, 128 t + 128); an inclusive scan of the lanes' totals through LDS, then the
// lanes that hold ranks k and k2 walk their bins.  The counts add up to M < 2^32, so no prefix wraps.
__global__ __launch_bounds__(256) void mimic_select_kernel(mimic_ws w, int nrows, double m, uint32_t k, uint32_t k2, float f) {
    __shared__ uint32_t scan[256];
    __shared__ uint32_t sel[2];
    const unsigned ch = blockIdx.x;
    float mg, ml;
    channel_means(w.partials + (size_t)ch * MIMIC_MAX_ROWS * 2, nrows, m, mg, ml);
    const uint32_t* h = w.hist + (size_t)ch * MIMIC_BINS + threadIdx.x * 128u;
    uint32_t total = 0;
    for (int i = 0; i < 32; ++i) {
        const u32x4 v = ((const u32x4*)h)[i];
        total += (v[0] + v[1]) + (v[2] + v[3]);
    }
    scan[threadIdx.x] = total;
    __syncthreads();
    for (unsigned off = 1; off < 256; off <<= 1) {
        const uint32_t add = threadIdx.x >= off ? scan[threadIdx.x - off] : 0u;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    const uint32_t before = scan[threadIdx.x] - total;            // the elements in the bins below this lane's
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t rank = r == 0 ? k : k2;
        if (total != 0u && rank >= before && rank - before < total) {
            uint32_t cum = before, b = 0;
            for (; b < 127u; ++b) {                               // the last bin is what is left: b never leaves the lane's 128
                cum += h[b];
                if (rank < cum) break;
            }
            sel[r] = threadIdx.x * 128u + b;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t lo_bits = sel[0], hi_bits = sel[1], ref_lo_bits = w.maxbits[ch] & 0x7fffu;
        const float lo = (float)half_of_bits(lo_bits), hi = (float)half_of_bits(hi_bits);
        f16 ref_hi = half_of_bits(lo_bits);
        if (f != 0.f) {
            float t = __fsub_rn(hi, lo);
            asm volatile("" : "+v"(t));
            t = __fmul_rn(f, t);
            asm volatile("" : "+v"(t));
            ref_hi = rn16(__fadd_rn(lo, t));
        }
        const uint32_t ref_hi_bits = (uint32_t)__builtin_bit_cast(unsigned short, ref_hi);
        f16* sc = w.scal + (size_t)ch * 4;
        sc[0] = (f16)mg;
        sc[1] = half_of_bits(ref_lo_bits);
        sc[2] = ref_hi;
        sc[3] = ref_hi_bits > ref_lo_bits ? ref_hi : half_of_bits(ref_lo_bits);
    }
}

// g -> d -> g' -> the sampler's tail.  MODE 0: DDIM; 1: DPM-Solver++ first order; 2: second order
template <int MODE>
__device__ __forceinline__ void mimic_step_elem(float u, float c, float x, float x0p, float mg, float ref_lo, float s,
                                                const ddim_coef& kd, const dpm_coef& kp, f16& x0_out, f16& out) {
    const f16 g = cfg_combine(u, c, MODE == 0 ? kd.gs : kp.gs);
    const f16 d = rn16(__fsub_rn((float)g, mg));
    const f16 g2 = cfg_mimic_elem(d, s, ref_lo, mg);
    if (MODE == 0) out = ddim_tail(g2, x, kd);
    else dpm_tail<MODE == 2>(g2, x, x0p, kp, x0_out, out);
}

template <int MODE, int E>
__global__ __launch_bounds__(256) void mimic_step_kernel(const f16* eps, const f16* lat, const f16* x0_prev, f16* x0_out, f16* out,
                                                         ddim_coef kd, dpm_coef kp, const f16* scal, size_t M, size_t n) {
    const unsigned ch = blockIdx.y;
    const f16* sc = scal + (size_t)ch * 4;
    const float mg = (float)sc[0], ref_lo = (float)sc[1], s = (float)sc[3];
    const size_t base = (size_t)ch * M, nv = M / E, stride = (size_t)gridDim.x * 256;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += stride) {
        const size_t i = base + v * E;
        f16 u[E], c[E], x[E], xp[E], o[E], x0[E];
        load_halves<E>(eps + i, u);
        load_halves<E>(eps + n + i, c);
        load_halves<E>(lat + i, x);
        if (MODE == 2) load_halves<E>(x0_prev + i, xp);
#pragma unroll
        for (int j = 0; j < E; ++j)
            mimic_step_elem<MODE>((float)u[j], (float)c[j], (float)x[j], MODE == 2 ? (float)xp[j] : 0.f, mg, ref_lo, s, kd, kp, x0[j], o[j]);
        if (MODE != 0) store_halves<E>(x0_out + i, x0);
        store_halves<E>(out + i, o);
    }
}

// the guidance policy of the co-fused step (cofuse_common.h `cofuse_step_kernel`): a block owns one (c, t) line, so `prologue`
// hands the block's channel (as the bits of its float) to `elem`, which reads that channel's scalars: uniform loads
struct mimic_guidance {
    const f16* scal;
    unsigned tiles_per_line, T;
    __device__ __forceinline__ float prologue() const { return __uint_as_float(blockIdx.x / tiles_per_line / T); }
    template <int MODE>
    __device__ __forceinline__ void elem(float u, float c, float x, float x0p, float r, const ddim_coef& kd, const dpm_coef& kp, f16& x0,
                                         f16& o) const {
        const f16* sc = scal + (size_t)__float_as_uint(r) * 4;
        mimic_step_elem<MODE>(u, c, x, x0p, (float)sc[0], (float)sc[1], (float)sc[3], kd, kp, x0, o);
    }
};

static inline int mimic_width(size_t M) { return M % 8 == 0 ? 8 : M % 4 == 0 ? 4 : 1; }

// rows of `partials` per channel = blocks per channel of the sums launch: a function of M alone
static inline int mimic_rows(size_t M) {
    const size_t nv = M / mimic_width(M), want = (nv + 255) / 256;
    return (int)(want < MIMIC_MAX_ROWS ? want : MIMIC_MAX_ROWS);
}

static inline bool mimic_shape_ok(int C, int T, int HW) {
    return C > 0 && C <= 65535 && T > 0 && HW > 0 && (size_t)T * HW < ((size_t)1 << 32) && (size_t)C * T * HW <= ((size_t)1 << 40);
}

// what every statistics entry checks of its scalars: the scale, and the rank (k, f) against M
static int mimic_check_rank(const char* what, float mimic, size_t k, float f, size_t M) {
    VDX_CHECK(std::isfinite(mimic) && mimic > 0.f, "%s: mimic scale %g must be finite and > 0", what, (double)mimic);
    VDX_CHECK(k <= M - 1, "%s: rank k = %zu must lie in [0, M - 1], M = %zu", what, k, M);
    VDX_CHECK(f >= 0.f && f < 1.f, "%s: the rank's fraction f = %g must lie in [0, 1)", what, (double)f);
    return 0;
}

extern "C" size_t vdx_cfg_mimic_ws_bytes(int C, int T, int HW) {
    mimic_ws w;
    return mimic_shape_ok(C, T, HW) ? mimic_layout(nullptr, C, w) : 0;
}

// `stages`: bit 0 the sums, bit 1 the histogram, bit 2 the select; 7 is the statistics pass, anything else is for tests and the
// benchmark, which run one launch at a time on what the launches before it left in the workspace
extern "C" int vdx_cfg_mimic_stats_f16(const void* eps2, int C, int T, int HW, float guidance, float mimic, size_t k, float f, void* ws,
                                       int stages, vdx_stream_t stream) {
    const char* what = "vdx_cfg_mimic_stats_f16";
    VDX_CHECK(eps2 && ws, "%s: null pointer", what);
    VDX_CHECK(mimic_shape_ok(C, T, HW), "%s: bad shape C=%d T=%d HW=%d (a channel holds fewer than 2^32 elements)", what, C, T, HW);
    VDX_CHECK(stages >= 1 && stages <= 7, "%s: stages %d is not a set of launches 1 | 2 | 4", what, stages);
    const size_t M = (size_t)T * HW, n = (size_t)C * M;
    if (int rc = mimic_check_rank(what, mimic, k, f, M)) return rc;
    VDX_CHECK(((uintptr_t)eps2 & 15) == 0 && ((uintptr_t)ws & 15) == 0, "%s: pointer not 16-byte aligned", what);
    mimic_ws w;
    const size_t wb = mimic_layout(ws, C, w);
    VDX_CHECK(!co_overlap(ws, wb, eps2, 2 * n * sizeof(f16)), "%s: the workspace overlaps eps2", what);
    const int e = mimic_width(M), rows = mimic_rows(M);
    const size_t nv = M / e, want = (nv + 255) / 256;
    const hipStream_t s = (hipStream_t)stream;
    const f16* ep = (const f16*)eps2;
    const dim3 block(256), sgrid((unsigned)rows, (unsigned)C), hgrid((unsigned)(want < 1024 ? want : 1024), (unsigned)C);
    if (stages & 1) {
        if (e == 8) hipLaunchKernelGGL(mimic_sums_kernel<8>, sgrid, block, 0, s, ep, guidance, mimic, w, M, n);
        else if (e == 4) hipLaunchKernelGGL(mimic_sums_kernel<4>, sgrid, block, 0, s, ep, guidance, mimic, w, M, n);
        else hipLaunchKernelGGL(mimic_sums_kernel<1>, sgrid, block, 0, s, ep, guidance, mimic, w, M, n);
    }
    if (stages & 2) {
        if (e == 8) hipLaunchKernelGGL(mimic_hist_kernel<8>, hgrid, block, 0, s, ep, guidance, mimic, w, rows, M, n);
        else if (e == 4) hipLaunchKernelGGL(mimic_hist_kernel<4>, hgrid, block, 0, s, ep, guidance, mimic, w, rows, M, n);
        else hipLaunchKernelGGL(mimic_hist_kernel<1>, hgrid, block, 0, s, ep, guidance, mimic, w, rows, M, n);
    }
    if (stages & 4) {
        const size_t k2 = k + 1 < M ? k + 1 : M - 1;
        hipLaunchKernelGGL(mimic_select_kernel, dim3((unsigned)C), block, 0, s, w, rows, (double)M, (uint32_t)k, (uint32_t)k2, f);
    }
    return vdx_launch_status(what);
}

static int mimic_step_launch(const char* what, int mode, const void* eps2, const void* lat, const void* x0_prev, void* x0_out,
                             void* lat_out, const void* ws, ddim_coef kd, dpm_coef kp, int C, int T, int HW, vdx_stream_t stream) {
    VDX_CHECK(eps2 && lat && lat_out && ws && (mode == 0 || x0_out), "%s: bad arguments", what);
    VDX_CHECK(mimic_shape_ok(C, T, HW), "%s: bad shape C=%d T=%d HW=%d (a channel holds fewer than 2^32 elements)", what, C, T, HW);
    const size_t M = (size_t)T * HW, n = (size_t)C * M, nb = n * sizeof(f16);
    for (const void* p : {eps2, lat, x0_prev, (const void*)x0_out, (const void*)lat_out, ws})
        VDX_CHECK(((uintptr_t)p & 15) == 0, "%s: pointer not 16-byte aligned", what);
    mimic_ws w;
    const size_t wb = mimic_layout((void*)ws, C, w);
    // a lane reads its elements before it writes them, and writes nobody else's: lat_out == lat is fine, nothing else may share
    VDX_CHECK(lat_out == lat || !co_overlap(lat_out, nb, lat, nb), "%s: lat_out overlaps lat without being lat", what);
    VDX_CHECK(!co_overlap(lat_out, nb, eps2, 2 * nb) && !co_overlap(lat_out, nb, ws, wb), "%s: lat_out overlaps an input", what);
    VDX_CHECK(!co_overlap(ws, wb, eps2, 2 * nb) && !co_overlap(ws, wb, lat, nb) && (!x0_prev || !co_overlap(ws, wb, x0_prev, nb)),
              "%s: the workspace overlaps another buffer", what);
    if (mode != 0) {
        VDX_CHECK(!x0_prev || x0_out != x0_prev, "%s: x0_out must not be x0_prev (ping-pong two history buffers)", what);
        VDX_CHECK(!co_overlap(x0_out, nb, lat_out, nb) && !co_overlap(x0_out, nb, lat, nb) && !co_overlap(x0_out, nb, eps2, 2 * nb) &&
                      !co_overlap(x0_out, nb, ws, wb),
                  "%s: x0_out overlaps an input or lat_out", what);
        VDX_CHECK(!x0_prev || (!co_overlap(x0_prev, nb, x0_out, nb) && !co_overlap(x0_prev, nb, lat_out, nb)),
                  "%s: x0_prev overlaps an output", what);
    }
    const int e = mimic_width(M);
    const size_t nv = M / e, want = (nv + 255) / 256;
    const dim3 grid((unsigned)(want < 1024 ? want : 1024), (unsigned)C), block(256);
    const hipStream_t s = (hipStream_t)stream;
    const f16 *ep = (const f16*)eps2, *x = (const f16*)lat, *p = (const f16*)x0_prev, *sc = w.scal;
    f16 *z = (f16*)x0_out, *o = (f16*)lat_out;
    step_dispatch(mode, x0_prev, e, [&](auto m, auto ee) {
        hipLaunchKernelGGL((mimic_step_kernel<decltype(m)::value, decltype(ee)::value>), grid, block, 0, s, ep, x, p, z, o, kd, kp, sc, M, n);
    });
    return vdx_launch_status(what);
}

extern "C" int vdx_cfg_mimic_ddim_step_f16(const void* eps2, const void* lat, void* lat_out, const void* ws, float guidance,
                                           float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float sqrt_one_minus_aprev, int C,
                                           int T, int HW, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return mimic_step_launch("vdx_cfg_mimic_ddim_step_f16", 0, eps2, lat, nullptr, nullptr, lat_out, ws, kd, dpm_coef{}, C, T, HW, stream);
}

extern "C" int vdx_cfg_mimic_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                                          const void* ws, float guidance, float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1,
                                          float c_inv_r0, int C, int T, int HW, vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return mimic_step_launch("vdx_cfg_mimic_dpm_step_f16", 1, eps2, lat, x0_prev, x0_out, lat_out, ws, ddim_coef{}, kp, C, T, HW, stream);
}

// ---- co-denoising: the sample is the whole clip, its noise fused from the windows' outputs ------------------------------------
// grid (rows, C): block x of channel y takes the (y, t) lines t = x, x + rows, ...; a lane the elements p = (lane + 256 j) E of
// each.  rows = min(T, 64) for the sums: the partial of a block depends on the shapes and the table alone.
template <int E>
__global__ __launch_bounds__(256) void cofuse_mimic_sums_kernel(const f16* win, cofuse_tab tab, int K, const float* wn, float gs, float ms,
                                                                mimic_ws w, int C, int T, int HW) {
    const unsigned ch = blockIdx.y;
    mimic_zero(w, ch, blockIdx.x, gridDim.x);
    double a[2] = {0.0, 0.0};
    for (int t = (int)blockIdx.x; t < T; t += (int)gridDim.x) {
        for (int p = (int)threadIdx.x * E; p < HW; p += 256 * E) {
            float uf[E], cf[E];
            cofuse_uc<E>(win, tab, K, wn, C, T, HW, (int)ch, t, p, uf, cf);
#pragma unroll
            for (int j = 0; j < E; ++j) sum_acc(a, uf[j], cf[j], gs, ms);
        }
    }
    block_row2(a, w.partials + ((size_t)ch * MIMIC_MAX_ROWS + blockIdx.x) * 2);
}

template <int E>
__global__ __launch_bounds__(256) void cofuse_mimic_hist_kernel(const f16* win, cofuse_tab tab, int K, const float* wn, float gs, float ms,
                                                                mimic_ws w, int nrows, int C, int T, int HW) {
    const unsigned ch = blockIdx.y;
    float mg, ml;
    channel_means(w.partials + (size_t)ch * MIMIC_MAX_ROWS * 2, nrows, (double)((size_t)T * HW), mg, ml);
    uint32_t* h = w.hist + (size_t)ch * MIMIC_BINS;
    uint32_t mx = 0;
    for (int t = (int)blockIdx.x; t < T; t += (int)gridDim.x) {
        for (int p = (int)threadIdx.x * E; p < HW; p += 256 * E) {
            float uf[E], cf[E];
            cofuse_uc<E>(win, tab, K, wn, C, T, HW, (int)ch, t, p, uf, cf);
            uint32_t db[E], eb[E];
#pragma unroll
            for (int j = 0; j < E; ++j) mimic_bins(uf[j], cf[j], gs, ms, mg, ml, db[j], eb[j]);
            hist_add<E>(h, db, eb, mx);
        }
    }
    max_fold(w.maxbits + ch, mx);
}

static inline int cofuse_mimic_rows(int T) { return T < MIMIC_MAX_ROWS ? T : MIMIC_MAX_ROWS; }

extern "C" size_t vdx_cofuse_cfg_mimic_ws_bytes(int C, int T, int HW) { return vdx_cfg_mimic_ws_bytes(C, T, HW); }

extern "C" int vdx_cofuse_cfg_mimic_stats_f16(const void* windows, size_t windows_elems, const int64_t* win_off, const int* win_start,
                                              const int* win_len, int K, const float* wn, float guidance, float mimic, size_t k, float f,
                                              void* ws, int stages, int C, int T, int HW, vdx_stream_t stream) {
    const char* what = "vdx_cofuse_cfg_mimic_stats_f16";
    cofuse_tab tab;
    int e;
    if (int rc = cofuse_check(what, 0, false, nullptr, windows, windows_elems, win_off, win_start, win_len, K, wn, nullptr, nullptr,
                              nullptr, C, T, HW, tab, e))
        return rc;
    VDX_CHECK(mimic_shape_ok(C, T, HW), "%s: bad shape C=%d T=%d HW=%d (a channel holds fewer than 2^32 elements)", what, C, T, HW);
    VDX_CHECK(stages >= 1 && stages <= 7, "%s: stages %d is not a set of launches 1 | 2 | 4", what, stages);
    const size_t M = (size_t)T * HW;
    if (int rc = mimic_check_rank(what, mimic, k, f, M)) return rc;
    VDX_CHECK(ws && ((uintptr_t)ws & 15) == 0, "%s: the workspace must be a 16-byte aligned pointer", what);
    mimic_ws w;
    const size_t wb = mimic_layout(ws, C, w);
    VDX_CHECK(!co_overlap(ws, wb, windows, windows_elems * sizeof(f16)) && !co_overlap(ws, wb, wn, (size_t)K * T * sizeof(float)),
              "%s: the workspace overlaps an input", what);
    const int rows = cofuse_mimic_rows(T);
    const dim3 block(256), sgrid((unsigned)rows, (unsigned)C), hgrid((unsigned)(T < 1024 ? T : 1024), (unsigned)C);
    const hipStream_t st = (hipStream_t)stream;
    const f16* ww = (const f16*)windows;
    if (stages & 1) {
        if (e == 8) hipLaunchKernelGGL(cofuse_mimic_sums_kernel<8>, sgrid, block, 0, st, ww, tab, K, wn, guidance, mimic, w, C, T, HW);
        else if (e == 4) hipLaunchKernelGGL(cofuse_mimic_sums_kernel<4>, sgrid, block, 0, st, ww, tab, K, wn, guidance, mimic, w, C, T, HW);
        else hipLaunchKernelGGL(cofuse_mimic_sums_kernel<1>, sgrid, block, 0, st, ww, tab, K, wn, guidance, mimic, w, C, T, HW);
    }
    if (stages & 2) {
        if (e == 8) hipLaunchKernelGGL(cofuse_mimic_hist_kernel<8>, hgrid, block, 0, st, ww, tab, K, wn, guidance, mimic, w, rows, C, T, HW);
        else if (e == 4) hipLaunchKernelGGL(cofuse_mimic_hist_kernel<4>, hgrid, block, 0, st, ww, tab, K, wn, guidance, mimic, w, rows, C, T, HW);
        else hipLaunchKernelGGL(cofuse_mimic_hist_kernel<1>, hgrid, block, 0, st, ww, tab, K, wn, guidance, mimic, w, rows, C, T, HW);
    }
    if (stages & 4) {
        const size_t k2 = k + 1 < M ? k + 1 : M - 1;
        hipLaunchKernelGGL(mimic_select_kernel, dim3((unsigned)C), block, 0, st, w, rows, (double)M, (uint32_t)k, (uint32_t)k2, f);
    }
    return vdx_launch_status(what);
}

static int cofuse_mimic_launch(const char* what, int mode, const void* z, const void* windows, size_t windows_elems,
                               const int64_t* win_off, const int* win_start, const int* win_len, int K, const float* wn,
                               const void* x0_prev, void* x0_out, void* lat_out, const void* ws, ddim_coef kd, dpm_coef kp, int C, int T,
                               int HW, vdx_stream_t stream) {
    cofuse_tab tab;
    int e;
    if (int rc = cofuse_check(what, mode, true, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev, x0_out, lat_out,
                              C, T, HW, tab, e))
        return rc;
    VDX_CHECK(mimic_shape_ok(C, T, HW), "%s: bad shape C=%d T=%d HW=%d (a channel holds fewer than 2^32 elements)", what, C, T, HW);
    VDX_CHECK(ws && ((uintptr_t)ws & 15) == 0, "%s: the workspace must be a 16-byte aligned pointer", what);
    mimic_ws w;
    const size_t wb = mimic_layout((void*)ws, C, w);
    const size_t nb = (size_t)C * T * HW * sizeof(f16);
    VDX_CHECK(!co_overlap(ws, wb, lat_out, nb) && (!x0_out || !co_overlap(ws, wb, x0_out, nb)), "%s: the workspace overlaps an output",
              what);
    VDX_CHECK(!co_overlap(ws, wb, z, nb) && !co_overlap(ws, wb, windows, windows_elems * sizeof(f16)) &&
                  !co_overlap(ws, wb, wn, (size_t)K * T * sizeof(float)) && (!x0_prev || !co_overlap(ws, wb, x0_prev, nb)),
              "%s: the workspace overlaps an input", what);
    const size_t per_tile = 256 * (size_t)e;                      // `cofuse_launch`'s block map: the policy finds its channel by it
    const unsigned tiles_per_line = (unsigned)(((size_t)HW + per_tile - 1) / per_tile);
    return cofuse_launch<false>(what, mode, z, windows, tab, e, K, wn, x0_prev, x0_out, lat_out, kd, kp,
                                mimic_guidance{w.scal, tiles_per_line, (unsigned)T}, C, T, HW, stream);
}

extern "C" int vdx_cofuse_cfg_mimic_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                                  const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                                  const void* ws, float guidance, float sqrt_one_minus_at, float sqrt_at,
                                                  float sqrt_aprev, float sqrt_one_minus_aprev, int C, int T, int HW,
                                                  vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return cofuse_mimic_launch("vdx_cofuse_cfg_mimic_ddim_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len, K, wn,
                               nullptr, nullptr, lat_out, ws, kd, dpm_coef{}, C, T, HW, stream);
}

extern "C" int vdx_cofuse_cfg_mimic_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                                 const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev,
                                                 void* x0_out, void* lat_out, const void* ws, float guidance, float c_s0, float c_inv_a0,
                                                 float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW,
                                                 vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return cofuse_mimic_launch("vdx_cofuse_cfg_mimic_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len, K, wn,
                               x0_prev, x0_out, lat_out, ws, ddim_coef{}, kp, C, T, HW, stream);
}
