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

// ---- launches 1 and 2, over either noise source ------------------------------------------------------------------------------------
// grid (blocks, C): block x of channel y adds what the source hands it, in the source's order.  One buffer (`direct_source`, eps2 =
// [u; c], channels of M elements): the vectors x * 256 + lane + j * blocks * 256; the sums launch has min(vectors / 256, 64) blocks.
// Co-fused (`cofuse_source`, T lines a channel): the (y, t) lines t = x, x + blocks, ...; the sums launch has min(T, 64) blocks.
// Either way a block's partial depends on the shapes (and the table) alone.
template <class Src>
__global__ __launch_bounds__(256) void mimic_sums_kernel(Src src, float gs, float ms, mimic_ws w) {
    const unsigned ch = blockIdx.y;
    mimic_zero(w, ch, blockIdx.x, gridDim.x);
    double a[2] = {0.0, 0.0};
    src.each(ch, blockIdx.x, gridDim.x, [&](size_t, const f16 (&uf)[Src::width], const f16 (&cf)[Src::width]) {
#pragma unroll
        for (int j = 0; j < Src::width; ++j) sum_acc(a, (float)uf[j], (float)cf[j], gs, ms);
    });
    block_row(a, w.partials + ((size_t)ch * MIMIC_MAX_ROWS + blockIdx.x) * 2);
}

template <class Src>
__global__ __launch_bounds__(256) void mimic_hist_kernel(Src src, float gs, float ms, mimic_ws w, int nrows, double m) {
    const unsigned ch = blockIdx.y;
    float mg, ml;
    channel_means(w.partials + (size_t)ch * MIMIC_MAX_ROWS * 2, nrows, m, mg, ml);
    uint32_t* h = w.hist + (size_t)ch * MIMIC_BINS;
    uint32_t mx = 0;
    src.each(ch, blockIdx.x, gridDim.x, [&](size_t, const f16 (&uf)[Src::width], const f16 (&cf)[Src::width]) {
        uint32_t db[Src::width], eb[Src::width];
#pragma unroll
        for (int j = 0; j < Src::width; ++j) mimic_bins((float)uf[j], (float)cf[j], gs, ms, mg, ml, db[j], eb[j]);
        hist_add<Src::width>(h, db, eb, mx);
    });
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

// the guidance policy of every thresholded step (step_common.h `direct_step_kernel`, cofuse_common.h `cofuse_step_kernel`): the
// block's channel's scalars are its state (uniform loads, once per block), then g -> d -> g' -> the sampler's tail
struct mimic_guidance {
    const f16* scal;
    struct state {
        float mg, ref_lo, s;
    };
    static constexpr bool uses_c = true;
    __device__ __forceinline__ state prologue(int channel) const {
        const f16* sc = scal + (size_t)channel * 4;
        const auto uniform = [](f16 h) {                          // the same for every lane: kept in a scalar register
            return __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint((float)h)));
        };
        return {uniform(sc[0]), uniform(sc[1]), uniform(sc[3])};
    }
    template <int MODE>
    __device__ __forceinline__ void elem(float u, float c, float x, float x0p, const state& st, const ddim_coef& kd, const dpm_coef& kp,
                                         f16& x0, f16& o) const {
        const f16 g = cfg_combine(u, c, MODE == 0 ? kd.gs : kp.gs);
        const f16 d = rn16(__fsub_rn((float)g, st.mg));
        const f16 g2 = cfg_mimic_elem(d, st.s, st.ref_lo, st.mg);
        if (MODE == 0) o = ddim_tail(g2, x, kd);
        else dpm_tail<MODE == 2>(g2, x, x0p, kp, x0, o);
    }
};

static inline int mimic_width(size_t M) { return M % 8 == 0 ? 8 : M % 4 == 0 ? 4 : 1; }

static inline bool mimic_shape_ok(int C, int T, int HW) {
    return C > 0 && C <= 65535 && T > 0 && HW > 0 && (size_t)T * HW < ((size_t)1 << 32) && (size_t)C * T * HW <= ((size_t)1 << 40);
}

extern "C" size_t vdx_cfg_mimic_ws_bytes(int C, int T, int HW) {
    mimic_ws w;
    return mimic_shape_ok(C, T, HW) ? mimic_layout(nullptr, C, w) : 0;
}

extern "C" size_t vdx_cofuse_cfg_mimic_ws_bytes(int C, int T, int HW) { return vdx_cfg_mimic_ws_bytes(C, T, HW); }

// The statistics pass of both entries, whose checks of their noise have passed: the scalars and the workspace, then the launches.
// `src(E)` makes the noise source of access width E; `rows` / `hblocks`: the blocks a channel gets in the sums / histogram launch.
// `stages`: bit 0 the sums, bit 1 the histogram, bit 2 the select; 7 is the statistics pass, anything else is for tests and the
// benchmark, which run one launch at a time on what the launches before it left in the workspace.
template <class MakeSrc, size_t N>
static int mimic_stats_launch(const char* what, int e, MakeSrc&& src, const co_buf (&inputs)[N], float guidance, float mimic, size_t k,
                              float f, void* ws, int stages, int rows, size_t hblocks, int C, int T, int HW, vdx_stream_t stream) {
    VDX_CHECK(mimic_shape_ok(C, T, HW), "%s: bad shape C=%d T=%d HW=%d (a channel holds fewer than 2^32 elements)", what, C, T, HW);
    VDX_CHECK(stages >= 1 && stages <= 7, "%s: stages %d is not a set of launches 1 | 2 | 4", what, stages);
    const size_t M = (size_t)T * HW;
    VDX_CHECK(std::isfinite(mimic) && mimic > 0.f, "%s: mimic scale %g must be finite and > 0", what, (double)mimic);
    VDX_CHECK(k <= M - 1, "%s: rank k = %zu must lie in [0, M - 1], M = %zu", what, k, M);
    VDX_CHECK(f >= 0.f && f < 1.f, "%s: the rank's fraction f = %g must lie in [0, 1)", what, (double)f);
    VDX_CHECK(ws, "%s: null pointer", what);
    VDX_CHECK(((uintptr_t)ws & 15) == 0, "%s: the workspace must be a 16-byte aligned pointer", what);
    mimic_ws w;
    const size_t wb = mimic_layout(ws, C, w);
    for (const co_buf& in : inputs) VDX_CHECK(!co_overlap(ws, wb, in.p, in.bytes), "%s: the workspace overlaps an input", what);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 block(256), sgrid((unsigned)rows, (unsigned)C), hgrid((unsigned)(hblocks < 1024 ? hblocks : 1024), (unsigned)C);
    width_dispatch(e, [&](auto ee) {
        auto sr = src(ee);
        if (stages & 1) hipLaunchKernelGGL(mimic_sums_kernel<decltype(sr)>, sgrid, block, 0, s, sr, guidance, mimic, w);
        if (stages & 2) hipLaunchKernelGGL(mimic_hist_kernel<decltype(sr)>, hgrid, block, 0, s, sr, guidance, mimic, w, rows, (double)M);
    });
    if (stages & 4) {
        const size_t k2 = k + 1 < M ? k + 1 : M - 1;
        hipLaunchKernelGGL(mimic_select_kernel, dim3((unsigned)C), block, 0, s, w, rows, (double)M, (uint32_t)k, (uint32_t)k2, f);
    }
    return vdx_launch_status(what);
}

// ---- one sample in one buffer: eps2 = [u; c], C channels of M = T HW elements each, E halves per access (M is a multiple of E) --
extern "C" int vdx_cfg_mimic_stats_f16(const void* eps2, int C, int T, int HW, float guidance, float mimic, size_t k, float f, void* ws,
                                       int stages, vdx_stream_t stream) {
    const char* what = "vdx_cfg_mimic_stats_f16";
    VDX_CHECK(eps2, "%s: null pointer", what);
    VDX_CHECK(((uintptr_t)eps2 & 15) == 0, "%s: pointer not 16-byte aligned", what);
    const size_t M = (size_t)T * HW, n = (size_t)C * M;
    const int e = mimic_width(M);
    const size_t want = (M / e + 255) / 256;                      // rows of `partials` per channel: a function of M alone, <= 64
    const co_buf inputs[] = {{eps2, 2 * n * sizeof(f16)}};
    const auto src = [&](auto ee) { return direct_source<decltype(ee)::value>{(const f16*)eps2, M, n}; };
    return mimic_stats_launch(what, e, src, inputs, guidance, mimic, k, f, ws, stages, (int)(want < MIMIC_MAX_ROWS ? want : MIMIC_MAX_ROWS),
                              want, C, T, HW, stream);
}

static int mimic_step_launch(const char* what, int mode, const void* eps2, const void* lat, const void* x0_prev, void* x0_out,
                             void* lat_out, const void* ws, ddim_coef kd, dpm_coef kp, int C, int T, int HW, vdx_stream_t stream) {
    VDX_CHECK(ws, "%s: bad arguments", what);
    VDX_CHECK(mimic_shape_ok(C, T, HW), "%s: bad shape C=%d T=%d HW=%d (a channel holds fewer than 2^32 elements)", what, C, T, HW);
    const size_t M = (size_t)T * HW, nb = (size_t)C * M * sizeof(f16);
    mimic_ws w;
    const co_buf extra[] = {{ws, mimic_layout((void*)ws, C, w)}}, read[] = {{eps2, 2 * nb}, {lat, nb}, {x0_prev, nb}};
    for (const co_buf& in : read)
        VDX_CHECK(!in.p || !co_overlap(ws, extra[0].bytes, in.p, in.bytes), "%s: the workspace overlaps another buffer", what);
    return direct_launch(what, mode, false, eps2, lat, x0_prev, x0_out, lat_out, extra, kd, kp, mimic_guidance{w.scal}, (unsigned)C, M, 1024,
                         stream);
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
extern "C" int vdx_cofuse_cfg_mimic_stats_f16(const void* windows, size_t windows_elems, const int64_t* win_off, const int* win_start,
                                              const int* win_len, int K, const float* wn, float guidance, float mimic, size_t k, float f,
                                              void* ws, int stages, int C, int T, int HW, vdx_stream_t stream) {
    const char* what = "vdx_cofuse_cfg_mimic_stats_f16";
    cofuse_tab tab;
    int e;
    if (int rc = cofuse_check(what, 0, false, nullptr, windows, windows_elems, win_off, win_start, win_len, K, wn, nullptr, nullptr,
                              nullptr, C, T, HW, tab, e))
        return rc;
    const co_buf inputs[] = {{windows, windows_elems * sizeof(f16)}, {wn, (size_t)K * T * sizeof(float)}};
    const auto src = [&](auto ee) { return cofuse_source<decltype(ee)::value>{(const f16*)windows, tab, K, wn, C, T, HW, (unsigned)T}; };
    return mimic_stats_launch(what, e, src, inputs, guidance, mimic, k, f, ws, stages, T < MIMIC_MAX_ROWS ? T : MIMIC_MAX_ROWS, (size_t)T, C,
                              T, HW, stream);
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
    return cofuse_launch<false>(what, mode, z, windows, tab, e, K, wn, x0_prev, x0_out, lat_out, kd, kp, mimic_guidance{w.scal}, C, T, HW,
                                stream);
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
