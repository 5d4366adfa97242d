// cofuse_common.h — what the co-fused whole-clip steps share on top of step_common.h: the window table, the fp32 fuse of the windows'
// noise (as a function and as the statistics passes' noise source), the ONE line-per-block step kernel with its launcher, and the
// host checks.  codenoise.hip (the plain co-denoising steps, flat and ring), rescale.hip and dynthresh.hip (the same steps with CFG
// rescale / dynamic thresholding and their statistics passes) and cotile.hip (the row-per-block tiled steps) all go through these,
// so the variants cannot drift apart.  A variant is a guidance policy (what turns the fused u, c into the guided noise), the RING
// flag, the table type (`costride_tab`: a frame stride per row), or a block map of its own that ends in `cofuse_tail`.
#pragma once
#include <cstdint>
#include <type_traits>

#include "vdx_common.h"
#include "step_chains.h"   // rn16
#include "step_common.h"   // the vector accesses, the policies, the tail, the dispatch, the aliasing check

#define COFUSE_MAX_WINDOWS 64

// the window table, by value in the kernel arguments (1 KiB): uniform reads, and the host has checked every row
struct cofuse_tab {
    long long off[COFUSE_MAX_WINDOWS];     // element offset of window k's (2,C,L_k,h,w) block from the base pointer
    int s[COFUSE_MAX_WINDOWS];             // first frame
    int len[COFUSE_MAX_WINDOWS];           // L_k
};

// the table of the strided steps (vdx_costride_*): row k holds the frames s_k + f * d_k, f in [0, L_k).  1.25 KiB by value, well
// inside the 4 KiB of kernel arguments; the flat and ring steps keep the 1 KiB table above
struct costride_tab : cofuse_tab {
    int d[COFUSE_MAX_WINDOWS];             // frame stride, >= 1
};
template <class Tab> constexpr bool co_strided = std::is_same<Tab, costride_tab>::value;

// x = fp16(x + fp16(weight * ctx)) on E elements: the ctx term of every UNet-input kernel, with `cfg_input_kernel`'s two roundings
template <int E>
__device__ __forceinline__ void add_ctx(f16 (&x)[E], const f16* ctx, float weight) {
    f16 cx[E];
    load_halves<E>(ctx, cx);
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const f16 t = rn16(__fmul_rn((float)cx[j], weight));      // fp16(cw * ctx)
        x[j] = rn16(__fadd_rn((float)x[j], (float)t));            // fp16(x + t)
    }
}

// acc = first ? w * x : acc + w * x, the product and the sum rounded separately (blend_acc_kernel's guard: no fma_mix)
__device__ __forceinline__ float fuse_term(float acc, float w, float x, bool first) {
    float prod = __fmul_rn(w, x);
    asm volatile("" : "+v"(prod));
    return first ? prod : __fadd_rn(acc, prod);
}

// U, Cc of the E elements at (c, t, p) fused over the windows that hold frame t, k ascending, then rounded to fp16.  t is uniform over a block, so the window loop, the table reads and the weights are too.
// RING (the vdx_coloop_* steps): window k holds the frames (s_k + f) mod T, f in [0, L_k), with 0 <= s_k < T and L_k <= T, so the one
// wrap is a compare and an add; the default leaves the plain instantiations as they were.
// A `costride_tab` (the vdx_costride_* steps): window k holds frame t as its frame q / d_k where q = t - s_k >= 0, q % d_k == 0 and
// q / d_k < L_k: one unsigned division per window, on block-uniform integers.
template <int E, bool RING = false, class Tab = cofuse_tab>
__device__ __forceinline__ void cofuse_uc(const f16* win, const Tab& tab, int K, const float* wn, int C, int T, int HW, int c,
                                          int t, int p, f16 (&uf)[E], f16 (&cf)[E]) {
    float U[E], Cc[E];
#pragma unroll
    for (int j = 0; j < E; ++j) U[j] = Cc[j] = 0.f;
    bool first = true;
    for (int k = 0; k < K; ++k) {
        int f = t - tab.s[k];
        const int L = tab.len[k];
        if constexpr (co_strided<Tab>) {
            if (f < 0) continue;
            const unsigned d = (unsigned)tab.d[k], q = (unsigned)f / d;
            if (q * d != (unsigned)f || q >= (unsigned)L) continue;
            f = (int)q;
        } else if constexpr (RING) {
            if (f < 0) f += T;
            if (f >= L) continue;
        } else {
            if (f < 0 || f >= L) continue;
        }
        const float w = wn[(size_t)k * T + t];
        const f16* up = win + tab.off[k] + ((size_t)c * L + f) * HW + p;
        const f16* cp = up + (size_t)C * L * HW;
        f16 u[E], cc[E];
        load_halves<E>(up, u);
        load_halves<E>(cp, cc);
#pragma unroll
        for (int j = 0; j < E; ++j) {
            U[j] = fuse_term(U[j], w, (float)u[j], first);
            Cc[j] = fuse_term(Cc[j], w, (float)cc[j], first);
        }
        first = false;
    }
#pragma unroll
    for (int j = 0; j < E; ++j) {
        uf[j] = rn16(U[j]);
        cf[j] = rn16(Cc[j]);
    }
}

// The co-fused noise source of the statistics passes (step_common.h `direct_source` is the one-buffer one): a channel is `lines`
// consecutive (c, t) lines of the clip (T of them: a latent channel; C * T: the whole clip as one).  Block x of nx of channel ch
// takes the channel's lines x, x + nx, ...; a lane the elements p = (lane + 256 j) E of each.
template <int E>
struct cofuse_source {
    static constexpr int width = E;
    const f16* win;
    cofuse_tab tab;
    int K;
    const float* wn;
    int C, T, HW;
    unsigned lines;
    template <class F>
    __device__ __forceinline__ void each(unsigned ch, unsigned x, unsigned nx, F&& f) const {
        for (unsigned l = x; l < lines; l += nx) {
            const unsigned line = ch * lines + l;
            const int c = (int)(line / (unsigned)T), t = (int)(line - (unsigned)c * (unsigned)T);
            for (int p = (int)threadIdx.x * E; p < HW; p += 256 * E) {
                f16 uf[E], cf[E];
                cofuse_uc<E>(win, tab, K, wn, C, T, HW, c, t, p, uf, cf);
                f((size_t)line * HW + p, uf, cf);
            }
        }
    }
};

// ---- the step itself ---------------------------------------------------------------------------------------------------------------
// Block map: a block works on ONE (c, t) line of h*w elements (tiles of 256 lanes x E elements): see codenoise.hip.
template <int MODE, int E, bool RING, class G, class Tab = cofuse_tab, class Z = no_noise>
__global__ __launch_bounds__(256) void cofuse_step_kernel(const f16* z, const f16* win, Tab tab, int K, const float* wn,
                                                          const f16* x0_prev, f16* x0_out, f16* out, ddim_coef kd, dpm_coef kp, G g,
                                                          int C, int T, int HW, unsigned tiles_per_line, Z nz) {
    const unsigned line = blockIdx.x / tiles_per_line, tile = blockIdx.x - line * tiles_per_line;
    const int c = (int)(line / (unsigned)T), t = (int)(line - (unsigned)c * (unsigned)T);
    const typename G::state st = g.prologue(c);                   // all 256 lanes, before any of them leaves
    const int p = (int)((tile * 256u + threadIdx.x) * (unsigned)E);
    if (p >= HW) return;                                          // HW is a multiple of E: a lane's E elements are all inside
    f16 uf[E], cf[E];
    cofuse_uc<E, RING, Tab>(win, tab, K, wn, C, T, HW, c, t, p, uf, cf);   // uniform over the block: t is
    cofuse_tail<MODE, E>(z, x0_prev, x0_out, out, (size_t)line * HW + p, uf, cf, g, st, kd, kp, nz);
}

// the launch of a line-per-block step whose arguments `cofuse_check` has passed (it gave `tab` and `e`).  `nz`: the noise policy of
// a stochastic step; the sample is the clip, so an element's index is its logical one and E stays (a lane's i is a multiple of E)
template <bool RING, class G, class Tab, class Z = no_noise>
static int cofuse_launch(const char* what, int mode, const void* z, const void* windows, const Tab& tab, int e, int K,
                         const float* wn, const void* x0_prev, void* x0_out, void* lat_out, ddim_coef kd, dpm_coef kp, G g, int C, int T,
                         int HW, vdx_stream_t stream, Z nz = Z{}) {
    const size_t per_tile = 256 * (size_t)e;
    const size_t tiles_per_line = ((size_t)HW + per_tile - 1) / per_tile;
    const size_t blocks = tiles_per_line * C * T;
    VDX_CHECK(blocks <= 0x7fffffffull, "%s: %zu blocks exceed the grid", what, blocks);
    step_dispatch(mode, x0_prev, e, [&](auto m, auto ee) {
        hipLaunchKernelGGL((cofuse_step_kernel<decltype(m)::value, decltype(ee)::value, RING, G, Tab, Z>), dim3((unsigned)blocks), dim3(256), 0,
                           (hipStream_t)stream, (const f16*)z, (const f16*)windows, tab, K, wn, (const f16*)x0_prev, (f16*)x0_out,
                           (f16*)lat_out, kd, kp, g, C, T, HW, (unsigned)tiles_per_line, nz);
    });
    return vdx_launch_status(what);
}

// ---- the host checks ---------------------------------------------------------------------------------------------------------------
// The time-window table of a step: every row (off, s, L) against T and the buffer, `e` narrowed to what every offset allows, and
// every frame in some window.  `ring`: a row means the frames (s + f) mod T, so 0 <= s < T and 1 <= L <= T replace s + L <= T, and
// a frame is held under that rule.  `need(k, L, elems)` gives the elements window k occupies from its offset (it may refuse the row).
// `win_stride` (read for a `costride_tab` only, never with `ring`): a row means the frames s + f * d, so d >= 1 and
// s + (L - 1) * d < T, formed in 64 bits, replace s + L <= T, and a frame is held under that rule.
template <class Tab, class Need>
static inline int cofuse_windows(const char* what, bool ring, size_t windows_elems, const int64_t* win_off, const int* win_start,
                                 const int* win_len, int K, int T, Need&& need, Tab& tab, int& e, const int* win_stride = nullptr) {
    for (int k = 0; k < K; ++k) {
        const long long off = (long long)win_off[k];
        const int s = win_start[k], L = win_len[k];
        if constexpr (co_strided<Tab>) {
            const int d = win_stride[k];
            VDX_CHECK(d >= 1 && L >= 1 && s >= 0 && (long long)s + ((long long)L - 1) * d < T,
                      "%s: window %d holds the frames %d + f * %d, f < %d, of %d frames", what, k, s, d, L, T);
            tab.d[k] = d;
        } else {
            VDX_CHECK(L >= 1 && s >= 0 && s < T && L <= (ring ? T : T - s), "%s: window %d covers [%d, %d + %d) of %d frames", what, k,
                      s, s, L, T);
        }
        size_t elems = 0;
        if (int rc = need(k, L, elems)) return rc;
        VDX_CHECK(off >= 0 && (size_t)off <= windows_elems && elems <= windows_elems - (size_t)off,
                  "%s: window %d (offset %lld, %zu elements) leaves the buffer of %zu elements", what, k, off, elems, windows_elems);
        co_narrow(e, off);
        tab.off[k] = off;
        tab.s[k] = s;
        tab.len[k] = L;
    }
    for (int t = 0; t < T; ++t) {                                 // a frame nobody predicts has no noise to step with
        bool hit = false;
        for (int k = 0; k < K && !hit; ++k) {
            int f = t - tab.s[k];
            if (ring && f < 0) f += T;
            if constexpr (co_strided<Tab>) hit = f >= 0 && f % tab.d[k] == 0 && f / tab.d[k] < tab.len[k];
            else hit = f >= 0 && f < tab.len[k];
        }
        VDX_CHECK(hit, "%s: frame %d is in no window", what, t);
    }
    return 0;
}

// Every check of a line-per-block co-fused step, before a launch -> 0 and the table `tab` and the access width `e` (8, 4 or 1
// halves), else the error.  mode 0: DDIM (no x0 history); otherwise DPM-Solver++.  `writes` false: a statistics pass, which reads
// no latent and writes none (z, x0_prev, x0_out and lat_out are then not looked at beyond their alignment).  `Tab` a
// `costride_tab`: `win_stride` is the rows' fourth column.
template <class Tab>
static inline int cofuse_check(const char* what, int mode, bool writes, const void* z, const void* windows, size_t windows_elems,
                               const int64_t* win_off, const int* win_start, const int* win_len, int K, const float* wn,
                               const void* x0_prev, void* x0_out, void* lat_out, int C, int T, int HW, Tab& tab, int& e,
                               bool ring = false, const int* win_stride = nullptr) {
    VDX_CHECK((z || !writes) && windows && win_off && win_start && win_len && wn && (lat_out || !writes) &&
                  (win_stride || !co_strided<Tab>), "%s: null pointer", what);
    VDX_CHECK(C > 0 && T > 0 && HW > 0 && HW <= 1 << 30, "%s: bad shape C=%d T=%d HW=%d", what, C, T, HW);
    VDX_CHECK(K >= 1 && K <= COFUSE_MAX_WINDOWS, "%s: %d windows, 1..%d are supported", what, K, COFUSE_MAX_WINDOWS);
    VDX_CHECK(mode == 0 || !writes || x0_out, "%s: x0_out is null", what);
    const size_t n = (size_t)C * T * HW;
    VDX_CHECK((size_t)C * T <= (size_t)1 << 30 && n <= (size_t)1 << 40, "%s: latent too large", what);
    for (const void* ptr : {z, windows, (const void*)wn, x0_prev, (const void*)x0_out, (const void*)lat_out})
        VDX_CHECK(((uintptr_t)ptr & 15) == 0, "%s: pointer not 16-byte aligned", what);
    tab = Tab{};
    e = HW % 8 == 0 ? 8 : HW % 4 == 0 ? 4 : 1;
    const auto need = [&](int, int L, size_t& elems) {
        elems = 2 * (size_t)C * L * HW;
        return 0;
    };
    if (int rc = cofuse_windows(what, ring, windows_elems, win_off, win_start, win_len, K, T, need, tab, e, win_stride)) return rc;
    if (!writes) return 0;
    const co_buf inputs[] = {{windows, windows_elems * sizeof(f16)}, {wn, (size_t)K * T * sizeof(float)}};
    return cofuse_alias(what, mode, z, x0_prev, x0_out, lat_out, n * sizeof(f16), inputs, "an input or lat_out", "an input or lat_out");
}
