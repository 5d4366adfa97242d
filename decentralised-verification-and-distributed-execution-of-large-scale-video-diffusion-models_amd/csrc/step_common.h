// step_common.h — what every fused sampler step shares, whichever way its noise arrives: the vector accesses, the guidance policies
// that need no statistics, the tail from (u, c) to the stores, the mode / width dispatch, the ONE aliasing check, and the ONE
// one-buffer step kernel with its launcher.  A step is a noise source (eps2 = [u; c] in one buffer: here; fused from the windows'
// UNet outputs: cofuse_common.h), a guidance policy (none, plain CFG: here; CFG rescale: rescale.hip; dynamic thresholding:
// dynthresh.hip) and a sampler tail (step_chains.h), so no combination is written out twice.
#pragma once
#include <cstdint>
#include <type_traits>

#include "vdx_common.h"
#include "step_chains.h"

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

// ---- guidance policies -------------------------------------------------------------------------------------------------------------
// A guidance policy turns the (u, c) of one element into the new latent (and x0).  `prologue(channel)` is called by all 256 lanes of
// a block before any of them leaves and gives the block's `state` (the kernel finds the channel: no policy looks at the block map);
// `elem<MODE>` is the chain of step_chains.h, once per element.  MODE 0: DDIM; 1: DPM-Solver++ first order; 2: second order.
// `uses_c`: whether a one-buffer step has a conditional half to read.
struct no_state {};

// the sampler alone, g = u: the caller did the combine (`vdx_ddim_step_f16`, `vdx_dpm_step_f16`)
struct no_guidance {
    typedef no_state state;
    static constexpr bool uses_c = false;
    __device__ __forceinline__ state prologue(int) const { return {}; }
    template <int MODE>
    __device__ __forceinline__ void elem(float u, float, float x, float x0p, const state&, const ddim_coef& kd, const dpm_coef& kp,
                                         f16& x0, f16& o) const {
        if (MODE == 0) o = ddim_tail((f16)u, x, kd);
        else dpm_elem<false, MODE == 2>(u, 0.f, x, x0p, kp, x0, o);
    }
};

// plain classifier-free guidance
struct cfg_guidance {
    typedef no_state state;
    static constexpr bool uses_c = true;
    __device__ __forceinline__ state prologue(int) const { return {}; }
    template <int MODE>
    __device__ __forceinline__ void elem(float u, float c, float x, float x0p, const state&, const ddim_coef& kd, const dpm_coef& kp,
                                         f16& x0, f16& o) const {
        if (MODE == 0) o = cfg_ddim_elem(u, c, x, kd);
        else dpm_elem<true, MODE == 2>(u, c, x, x0p, kp, x0, o);
    }
};

// ---- noise policies ----------------------------------------------------------------------------------------------------------------
// What a stochastic sampler adds after the tail: `draws` false, nothing (every deterministic step: the policy is empty, no argument
// is read and no branch taken); true (step_noise.h `philox_noise`): `draw<E>(i, w)` gives the N(0, 1) of the lane's E elements at
// i, `c_n` their factor, and the tail ends in step_chains.h's `noise_term`.  `narrow(e)`: what the host takes off the access width.
struct no_noise {
    static constexpr bool draws = false;
    void narrow(int&) const {}
};

// the tail of every step kernel: a lane's E elements at i, from their (u, c) to the stores
template <int MODE, int E, class G, class Z = no_noise>
__device__ __forceinline__ void cofuse_tail(const f16* z, const f16* x0_prev, f16* x0_out, f16* out, size_t i, const f16 (&uf)[E],
                                            const f16 (&cf)[E], const G& g, const typename G::state& st, const ddim_coef& kd,
                                            const dpm_coef& kp, const Z& nz = Z{}) {
    f16 x[E], xp[E];
    load_halves<E>(z + i, x);
    if (MODE == 2) load_halves<E>(x0_prev + i, xp);
    f16 o[E], x0[E];
#pragma unroll
    for (int j = 0; j < E; ++j) g.template elem<MODE>((float)uf[j], (float)cf[j], (float)x[j], MODE == 2 ? (float)xp[j] : 0.f, st, kd, kp, x0[j], o[j]);
    if constexpr (Z::draws) {
        f16 w[E];
        nz.template draw<E>(i, w);
#pragma unroll
        for (int j = 0; j < E; ++j) o[j] = noise_term(o[j], w[j], nz.c_n);
    }
    if (MODE != 0) store_halves<E>(x0_out + i, x0);
    store_halves<E>(out + i, o);
}

// ---- the one-buffer noise source ---------------------------------------------------------------------------------------------------
// eps2 = [u; c], each half `n` elements in channels of M (a multiple of E).  Block x of nx of channel ch grid-strides over the
// channel's vectors: x * 256 + lane + j * nx * 256.  `each` hands f the vector's index in a half and its (u, c).
template <int E, bool CFG = true>
struct direct_source {
    static constexpr int width = E;
    const f16* eps;
    size_t M, n;
    template <class F>
    __device__ __forceinline__ void each(unsigned ch, unsigned x, unsigned nx, F&& f) const {
        const size_t base = (size_t)ch * M, nv = M / E, stride = (size_t)nx * 256;
        for (size_t v = (size_t)x * 256 + threadIdx.x; v < nv; v += stride) {
            const size_t i = base + v * E;
            f16 u[E], c[E];
            load_halves<E>(eps + i, u);
            if (CFG) load_halves<E>(eps + n + i, c);
            f(i, u, CFG ? c : u);                                 // without a conditional half, c is u and nobody reads it
        }
    }
};

// A statistics block's 256 lanes' Q fp64 sums -> row[Q]: a shuffle tree inside each wave, then the four waves in ascending order
template <int Q>
__device__ __forceinline__ void block_row(double (&a)[Q], double* row) {
    __shared__ double w[4][Q];
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a[q] += __shfl_down(a[q], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < Q; ++q) w[threadIdx.x >> 6][q] = a[q];
    __syncthreads();
    if (threadIdx.x < Q) row[threadIdx.x] = ((w[0][threadIdx.x] + w[1][threadIdx.x]) + w[2][threadIdx.x]) + w[3][threadIdx.x];
}

// THE one-buffer step kernel.  grid (x, nchan): block (x, y) takes the vectors of the elements [y * M, (y + 1) * M).  Every element is
// read and written by one lane only, so `out` may be `lat`, and the result does not depend on the grid.
template <int MODE, int E, class G, class Z = no_noise>
__global__ __launch_bounds__(256) void direct_step_kernel(direct_source<E, G::uses_c> src, const f16* lat, const f16* x0_prev, f16* x0_out,
                                                          f16* out, ddim_coef kd, dpm_coef kp, G g, Z nz) {
    const typename G::state st = g.prologue((int)blockIdx.y);     // all 256 lanes, before any of them leaves
    src.each(blockIdx.y, blockIdx.x, gridDim.x, [&](size_t i, const f16 (&uf)[E], const f16 (&cf)[E]) {
        cofuse_tail<MODE, E>(lat, x0_prev, x0_out, out, i, uf, cf, g, st, kd, kp, nz);
    });
}

// ---- dispatch ----------------------------------------------------------------------------------------------------------------------
// go(E) as an integral constant, for an access width of 8, 4 or 1 halves
template <class F>
static inline void width_dispatch(int e, F&& go) {
    if (e == 8) go(std::integral_constant<int, 8>{});
    else if (e == 4) go(std::integral_constant<int, 4>{});
    else go(std::integral_constant<int, 1>{});
}

// go(MODE, E) as integral constants, for the one rule of the mode and an access width of 8, 4 or 1 halves
template <class F>
static inline void step_dispatch(int mode, const void* x0_prev, int e, F&& go) {
    switch (mode == 0 ? 0 : x0_prev ? 2 : 1) {
    case 0: width_dispatch(e, [&](auto ee) { go(std::integral_constant<int, 0>{}, ee); }); break;
    case 1: width_dispatch(e, [&](auto ee) { go(std::integral_constant<int, 1>{}, ee); }); break;
    default: width_dispatch(e, [&](auto ee) { go(std::integral_constant<int, 2>{}, ee); }); break;
    }
}

// ---- the host checks ---------------------------------------------------------------------------------------------------------------
static inline bool co_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// the widest access (8, 4 or 1 halves, at most `e`) that still divides v
static inline void co_narrow(int& e, long long v) {
    if (e == 8 && v % 8) e = v % 4 ? 1 : 4;
    if (e == 4 && v % 4) e = 1;
}

struct co_buf {
    const void* p;
    size_t bytes;
};

// What a step's outputs (nb bytes each) may share: lat_out may be the latent z itself (a lane reads its elements before it writes
// them, and writes nobody else's); otherwise no output touches z, another output, x0_prev or one of `inputs` (a null one is
// skipped).  `x0_z` / `x0_in` end the message of an x0_out that overlaps z or lat_out / one of `inputs`.
template <size_t N>
static inline int cofuse_alias(const char* what, int mode, const void* z, const void* x0_prev, const void* x0_out, const void* lat_out,
                               size_t nb, const co_buf (&inputs)[N], const char* x0_z, const char* x0_in) {
    VDX_CHECK(lat_out == z || !co_overlap(lat_out, nb, z, nb), "%s: lat_out overlaps the latent without being it", what);
    for (const co_buf& in : inputs) VDX_CHECK(!in.p || !co_overlap(lat_out, nb, in.p, in.bytes), "%s: lat_out overlaps an input", what);
    if (mode == 0) return 0;
    VDX_CHECK(!x0_prev || x0_out != x0_prev, "%s: x0_out must not be x0_prev (ping-pong two history buffers)", what);
    VDX_CHECK(!co_overlap(x0_out, nb, lat_out, nb) && !co_overlap(x0_out, nb, z, nb), "%s: x0_out overlaps %s", what, x0_z);
    for (const co_buf& in : inputs) VDX_CHECK(!in.p || !co_overlap(x0_out, nb, in.p, in.bytes), "%s: x0_out overlaps %s", what, x0_in);
    VDX_CHECK(!x0_prev || (!co_overlap(x0_prev, nb, x0_out, nb) && !co_overlap(x0_prev, nb, lat_out, nb)),
              "%s: x0_prev overlaps an output", what);
    return 0;
}

// THE launch of a one-buffer step: `eps` = [u; c] (u alone for `no_guidance`) of n = nchan * M elements a half, mode 0 DDIM (no x0
// history), otherwise DPM-Solver++.  `extra`: the policy's buffers, which join eps as inputs of the aliasing check.  E is the widest
// of 8, 4, 1 that divides M (and so n, where the conditional half starts); `lenient` (the two DDIM entries, which take any fp16
// tensor): the widest that the pointers' alignment allows as well, else every pointer must be 16-byte aligned.  `cap`: the blocks a
// channel gets at most; beyond it a lane strides.  `nz`: the noise policy (a stochastic step; it narrows E to what its map allows).
template <class G, size_t N, class Z = no_noise>
static int direct_launch(const char* what, int mode, bool lenient, const void* eps, const void* lat, const void* x0_prev, void* x0_out,
                         void* lat_out, const co_buf (&extra)[N], ddim_coef kd, dpm_coef kp, G g, unsigned nchan, size_t M, unsigned cap,
                         vdx_stream_t stream, Z nz = Z{}) {
    const size_t n = (size_t)nchan * M, nb = n * sizeof(f16);
    VDX_CHECK(eps && lat && lat_out && n > 0 && (mode == 0 || x0_out), "%s: bad arguments", what);
    VDX_CHECK(n <= ((size_t)1 << 40), "%s: n too large", what);
    co_buf inputs[N + 1] = {{eps, G::uses_c ? 2 * nb : nb}};
    const void* ptrs[N + 5] = {eps, lat, x0_prev, x0_out, lat_out};
    for (size_t k = 0; k < N; ++k) ptrs[k + 5] = (inputs[k + 1] = extra[k]).p;
    int e = 8;
    co_narrow(e, (long long)M);
    for (const void* p : ptrs) {
        if (lenient) co_narrow(e, (long long)((uintptr_t)p / sizeof(f16)));
        else VDX_CHECK(((uintptr_t)p & 15) == 0, "%s: pointer not 16-byte aligned", what);
    }
    nz.narrow(e);
    if (int rc = cofuse_alias(what, mode, lat, x0_prev, x0_out, lat_out, nb, inputs, "an input or lat_out", "an input or lat_out")) return rc;
    const size_t want = (M / e + 255) / 256;
    const dim3 grid((unsigned)(want < cap ? want : cap), nchan), block(256);
    step_dispatch(mode, x0_prev, e, [&](auto m, auto ee) {
        constexpr int E = decltype(ee)::value;
        hipLaunchKernelGGL((direct_step_kernel<decltype(m)::value, E, G, Z>), grid, block, 0, (hipStream_t)stream,
                           direct_source<E, G::uses_c>{(const f16*)eps, M, n}, (const f16*)lat, (const f16*)x0_prev, (f16*)x0_out,
                           (f16*)lat_out, kd, kp, g, nz);
    });
    return vdx_launch_status(what);
}
