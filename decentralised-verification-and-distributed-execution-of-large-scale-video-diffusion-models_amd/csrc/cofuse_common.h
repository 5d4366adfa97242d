// cofuse_common.h — what the co-fused whole-clip steps share: the window table, the fp32 fuse of the windows' noise, the vector
// accesses and the host checks.  codenoise.hip (the plain co-denoising steps) and rescale.hip (the same steps with CFG rescale and
// their statistics pass) both fuse U and Cc through these, so the two cannot drift apart.
#pragma once
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"   // rn16

#define COFUSE_MAX_WINDOWS 64

// the window table, by value in the kernel arguments (1 KiB): uniform reads, and the host has checked every row
struct cofuse_tab {
    long long off[COFUSE_MAX_WINDOWS];     // element offset of window k's (2,C,L_k,h,w) block from the base pointer
    int s[COFUSE_MAX_WINDOWS];             // first frame
    int len[COFUSE_MAX_WINDOWS];           // L_k
};

template <int E> struct halves;
template <> struct halves<8> { typedef f16x8 type; };
template <> struct halves<4> { typedef f16x4 type; };
template <> struct halves<1> { typedef f16 type; };

template <int E>
__device__ __forceinline__ void load_halves(const f16* p, f16 (&v)[E]) {
    if constexpr (E == 1) {
        v[0] = p[0];
    } else {
        const typename halves<E>::type h = *(const typename halves<E>::type*)p;
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] = h[j];
    }
}
template <int E>
__device__ __forceinline__ void store_halves(f16* p, const f16 (&v)[E]) {
    if constexpr (E == 1) {
        p[0] = v[0];
    } else {
        typename halves<E>::type h;
#pragma unroll
        for (int j = 0; j < E; ++j) h[j] = v[j];
        *(typename halves<E>::type*)p = h;
    }
}

// acc = first ? w * x : acc + w * x, the product and the sum rounded separately (blend_acc_kernel's guard: no fma_mix)
__device__ __forceinline__ float fuse_term(float acc, float w, float x, bool first) {
    float prod = __fmul_rn(w, x);
    asm volatile("" : "+v"(prod));
    return first ? prod : __fadd_rn(acc, prod);
}

// U, Cc of the E elements at (c, t, p) fused over the windows that hold frame t, k ascending, then rounded to fp16 (returned as
// the floats the chains take).  t is uniform over a block, so the window loop, the table reads and the weights are too.
// RING (coloop.hip): window k holds the frames (s_k + f) mod T, f in [0, L_k), with 0 <= s_k < T and L_k <= T, so the one
// wrap is a compare and an add; the default leaves the plain instantiations as they were.
template <int E, bool RING = false>
__device__ __forceinline__ void cofuse_uc(const f16* win, const cofuse_tab& tab, int K, const float* wn, int C, int T, int HW, int c,
                                          int t, int p, float (&uf)[E], float (&cf)[E]) {
    float U[E], Cc[E];
#pragma unroll
    for (int j = 0; j < E; ++j) U[j] = Cc[j] = 0.f;
    bool first = true;
    for (int k = 0; k < K; ++k) {
        int f = t - tab.s[k];
        const int L = tab.len[k];
        if constexpr (RING) {
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
        uf[j] = (float)rn16(U[j]);
        cf[j] = (float)rn16(Cc[j]);
    }
}

static inline bool co_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// Every check of a co-fused step, before a launch -> 0 and the table `tab` and the access width `e` (8, 4 or 1 halves), else the
// error.  mode 0: DDIM (no x0 history); otherwise DPM-Solver++.  `writes` false: a statistics pass, which reads
// no latent and writes none (z, x0_prev, x0_out and lat_out are then not looked at beyond their alignment).  `ring`
// (coloop.hip): a row (off, s, L) means the frames (s + f) mod T, so 0 <= s < T and 1 <= L <= T replace s + L <= T, and a
// frame is held under that rule; everything else, the choice of `e` included, is the same.
static inline int cofuse_check(const char* what, int mode, bool writes, const void* z, const void* windows, size_t windows_elems,
                               const int64_t* win_off, const int* win_start, const int* win_len, int K, const float* wn,
                               const void* x0_prev, void* x0_out, void* lat_out, int C, int T, int HW, cofuse_tab& tab, int& e,
                               bool ring = false) {
    VDX_CHECK((z || !writes) && windows && win_off && win_start && win_len && wn && (lat_out || !writes), "%s: null pointer", what);
    VDX_CHECK(C > 0 && T > 0 && HW > 0 && HW <= 1 << 30, "%s: bad shape C=%d T=%d HW=%d", what, C, T, HW);
    VDX_CHECK(K >= 1 && K <= COFUSE_MAX_WINDOWS, "%s: %d windows, 1..%d are supported", what, K, COFUSE_MAX_WINDOWS);
    VDX_CHECK(mode == 0 || !writes || x0_out, "%s: x0_out is null", what);
    const size_t n = (size_t)C * T * HW, nb = n * sizeof(f16);
    VDX_CHECK((size_t)C * T <= (size_t)1 << 30 && n <= (size_t)1 << 40, "%s: latent too large", what);
    for (const void* ptr : {z, windows, (const void*)wn, x0_prev, (const void*)x0_out, (const void*)lat_out})
        VDX_CHECK(((uintptr_t)ptr & 15) == 0, "%s: pointer not 16-byte aligned", what);
    tab = cofuse_tab{};
    e = HW % 8 == 0 ? 8 : HW % 4 == 0 ? 4 : 1;
    for (int k = 0; k < K; ++k) {
        const long long off = (long long)win_off[k];
        const int s = win_start[k], L = win_len[k];
        VDX_CHECK(L >= 1 && s >= 0 && s < T && L <= (ring ? T : T - s), "%s: window %d covers [%d, %d + %d) of %d frames", what, k, s, s,
                  L, T);
        const size_t need = 2 * (size_t)C * L * HW;
        VDX_CHECK(off >= 0 && (size_t)off <= windows_elems && need <= windows_elems - (size_t)off,
                  "%s: window %d (offset %lld, %zu elements) leaves the buffer of %zu elements", what, k, off, need, windows_elems);
        if (e == 8 && off % 8) e = off % 4 ? 1 : 4;
        if (e == 4 && off % 4) e = 1;
        tab.off[k] = off;
        tab.s[k] = s;
        tab.len[k] = L;
    }
    for (int t = 0; t < T; ++t) {                                 // a frame nobody predicts has no noise to step with
        bool hit = false;
        for (int k = 0; k < K && !hit; ++k) {
            int f = t - tab.s[k];
            if (ring && f < 0) f += T;
            hit = f >= 0 && f < tab.len[k];
        }
        VDX_CHECK(hit, "%s: frame %d is in no window", what, t);
    }
    if (!writes) return 0;
    const size_t wb = windows_elems * sizeof(f16);
    VDX_CHECK(lat_out == z || !co_overlap(lat_out, nb, z, nb), "%s: lat_out overlaps z without being z", what);
    VDX_CHECK(!co_overlap(lat_out, nb, windows, wb) && !co_overlap(lat_out, nb, wn, (size_t)K * T * sizeof(float)),
              "%s: lat_out overlaps an input", what);
    if (mode != 0) {
        VDX_CHECK(!x0_prev || x0_out != x0_prev, "%s: x0_out must not be x0_prev (ping-pong two history buffers)", what);
        VDX_CHECK(!co_overlap(x0_out, nb, lat_out, nb) && !co_overlap(x0_out, nb, z, nb) && !co_overlap(x0_out, nb, windows, wb) &&
                      !co_overlap(x0_out, nb, wn, (size_t)K * T * sizeof(float)),
                  "%s: x0_out overlaps an input or lat_out", what);
        VDX_CHECK(!x0_prev || (!co_overlap(x0_prev, nb, x0_out, nb) && !co_overlap(x0_prev, nb, lat_out, nb)),
                  "%s: x0_prev overlaps an output", what);
    }
    return 0;
}
