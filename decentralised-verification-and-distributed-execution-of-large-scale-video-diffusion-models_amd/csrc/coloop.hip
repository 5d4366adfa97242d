// coloop.hip — seamless looping for temporal co-denoising: the windows of codenoise.hip placed on a RING (AnimateDiff's
// `closed_loop` context option; MultiDiffusion along time with periodic windows; no reference counterpart, opt-in:
// vdx/codenoise.py `loop_plan`, `DiffuserConfig.loop`).  A window row (off, s, L) means the frames (s + f) mod T, f in [0, L),
// with 0 <= s < T and 1 <= L <= T: the last window wraps over the clip's end into its first frames, so frames T-1 and 0 are
// denoised together in one UNet call at every step, like any other neighbouring pair.
//
//   vdx_cfg_input_loop_f16         `vdx_cfg_input_window_f16` reading frame (s + f) mod T: the contiguous (2,C,L,h,w) UNet input
//                                  in one launch; the ctx term keeps `cfg_input_kernel`'s two roundings.
//   vdx_coloop_cfg_ddim_step_f16   `vdx_cofuse_cfg_ddim_step_f16` / `vdx_cofuse_cfg_dpm_step_f16` with the modular rule: per
//   vdx_coloop_cfg_dpm_step_f16    (c, t) line, for k ascending, f = t - s_k, f += T if f < 0, the window is skipped if f >= L_k.
//                                  The fuse is `cofuse_uc` itself (cofuse_common.h, its RING flag), term for term, then the
//                                  unchanged chains of step_chains.h.
// A table in which no window wraps gives the bits of the vdx_cofuse_* step.  The wrap is a compare and an add / subtract on a
// block-uniform (step) or per-vector (input) integer, never a division.  Block map, access widths, aliasing (lat_out may be
// z), no atomics, no data-dependent index, NaN / inf staying in their element: all as codenoise.hip states them.
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"
#include "cofuse_common.h"

// MODE 0: DDIM; 1: DPM-Solver++ first order; 2: second order
template <int MODE, int E>
__global__ __launch_bounds__(256) void coloop_kernel(const f16* z, const f16* win, cofuse_tab tab, int K, const float* wn,
                                                     const f16* x0_prev, f16* x0_out, f16* out, ddim_coef kd, dpm_coef kp,
                                                     int C, int T, int HW, unsigned tiles_per_line) {
    const unsigned line = blockIdx.x / tiles_per_line, tile = blockIdx.x - line * tiles_per_line;
    const int c = (int)(line / (unsigned)T), t = (int)(line - (unsigned)c * (unsigned)T);
    const int p = (int)((tile * 256u + threadIdx.x) * (unsigned)E);
    if (p >= HW) return;                                          // HW is a multiple of E: a lane's E elements are all inside
    float uf[E], cf[E];
    cofuse_uc<E, true>(win, tab, K, wn, C, T, HW, c, t, p, uf, cf);   // uniform over the block: t is
    const size_t i = (size_t)line * HW + p;
    f16 x[E], xp[E];
    load_halves<E>(z + i, x);
    if (MODE == 2) load_halves<E>(x0_prev + i, xp);
    f16 o[E], x0[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        if (MODE == 0) o[j] = cfg_ddim_elem(uf[j], cf[j], (float)x[j], kd);
        else dpm_elem<true, MODE == 2>(uf[j], cf[j], (float)x[j], MODE == 2 ? (float)xp[j] : 0.f, kp, x0[j], o[j]);
    }
    if (MODE != 0) store_halves<E>(x0_out + i, x0);
    store_halves<E>(out + i, o);
}

static int coloop_launch(const char* what, int mode, const void* z, const void* windows, size_t windows_elems,
                         const int64_t* win_off, const int* win_start, const int* win_len, int K, const float* wn,
                         const void* x0_prev, void* x0_out, void* lat_out, ddim_coef kd, dpm_coef kp, int C, int T, int HW,
                         vdx_stream_t stream) {
    cofuse_tab tab;
    int e;
    if (int rc = cofuse_check(what, mode, true, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev, x0_out, lat_out,
                              C, T, HW, tab, e, /*ring=*/true))
        return rc;
    const size_t per_tile = 256 * (size_t)e;
    const size_t tiles_per_line = ((size_t)HW + per_tile - 1) / per_tile;
    const size_t blocks = tiles_per_line * C * T;
    VDX_CHECK(blocks <= 0x7fffffffull, "%s: %zu blocks exceed the grid", what, blocks);
    const dim3 grid((unsigned)blocks), block(256);
    const hipStream_t st = (hipStream_t)stream;
    const f16 *zz = (const f16*)z, *ww = (const f16*)windows, *pp = (const f16*)x0_prev;
    f16 *xo = (f16*)x0_out, *oo = (f16*)lat_out;
    const unsigned tpl = (unsigned)tiles_per_line;
#define COLOOP_GO(M, EE) hipLaunchKernelGGL((coloop_kernel<M, EE>), grid, block, 0, st, zz, ww, tab, K, wn, pp, xo, oo, kd, kp, C, T, HW, tpl)
#define COLOOP_E(M)                  \
    do {                             \
        if (e == 8) COLOOP_GO(M, 8); \
        else if (e == 4) COLOOP_GO(M, 4); \
        else COLOOP_GO(M, 1);        \
    } while (0)
    if (mode == 0) COLOOP_E(0);
    else if (!x0_prev) COLOOP_E(1);
    else COLOOP_E(2);
#undef COLOOP_E
#undef COLOOP_GO
    return vdx_launch_status(what);
}

extern "C" int vdx_coloop_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                            const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                            float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                            float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return coloop_launch("vdx_coloop_cfg_ddim_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len, K, wn, nullptr,
                         nullptr, lat_out, kd, dpm_coef{}, C, T, HW, stream);
}

extern "C" int vdx_coloop_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                           const int* win_start, const int* win_len, int K, const float* wn,
                                           const void* x0_prev, void* x0_out, void* lat_out, float guidance, float c_s0,
                                           float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW,
                                           vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return coloop_launch("vdx_coloop_cfg_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev,
                         x0_out, lat_out, ddim_coef{}, kp, C, T, HW, stream);
}

// ---- the UNet input of one ring window, straight out of the whole-clip latent ---------------------------------------------
//   x = cat([z[:, :, (s + arange(L)) % T]]*2);  x = x + context_weight * ctx.repeat(1,1,L,1,1)     (cfg_input_kernel's expression)
template <int E>
__global__ __launch_bounds__(256) void cfg_input_loop_kernel(const f16* z, const f16* ctx, float weight, f16* x2, int C, int T,
                                                             int HW, int s, int L) {
    const int hv = HW / E;                                        // vectors per line
    const size_t nv = (size_t)C * L * hv, n = (size_t)C * L * HW;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(v % hv) * E;
        const int f = (int)((v / hv) % L);
        const int c = (int)(v / ((size_t)hv * L));
        int t = s + f;                                            // s < T and f < L <= T: one wrap at most
        if (t >= T) t -= T;
        f16 o[E];
        load_halves<E>(z + ((size_t)c * T + t) * HW + p, o);
        if (ctx) {
            f16 cx[E];
            load_halves<E>(ctx + (size_t)c * HW + p, cx);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const f16 w = rn16(__fmul_rn((float)cx[j], weight));   // fp16(cw * ctx)
                o[j] = rn16(__fadd_rn((float)o[j], (float)w));         // fp16(x + t)
            }
        }
        const size_t d = ((size_t)c * L + f) * HW + p;
        store_halves<E>(x2 + d, o);
        store_halves<E>(x2 + n + d, o);
    }
}

extern "C" int vdx_cfg_input_loop_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int HW, int s, int L,
                                      vdx_stream_t stream) {
    VDX_CHECK(z && x2 && C > 0 && T > 0 && HW > 0 && HW <= 1 << 30, "cfg_input_loop: bad arguments");
    VDX_CHECK(0 <= s && s < T && 1 <= L && L <= T, "cfg_input_loop: bad ring window start %d, length %d of %d frames", s, L, T);
    for (const void* ptr : {z, ctx, (const void*)x2}) VDX_CHECK(((uintptr_t)ptr & 15) == 0, "cfg_input_loop: pointer not 16-byte aligned");
    const size_t n = (size_t)C * L * HW;
    VDX_CHECK(!co_overlap(x2, 2 * n * sizeof(f16), z, (size_t)C * T * HW * sizeof(f16)), "cfg_input_loop: x2 overlaps z");
    const int E = HW % 8 == 0 ? 8 : 1;                            // every line of z, ctx and both halves of x2 is then 16-byte aligned
    const size_t nv = n / E;
    VDX_CHECK((nv + 255) / 256 <= 0x7fffffffull, "cfg_input_loop: window too large");
    const unsigned blocks = (unsigned)((nv + 255) / 256);         // no cap: one vector per lane
    const hipStream_t st = (hipStream_t)stream;
    if (E == 8)
        hipLaunchKernelGGL(cfg_input_loop_kernel<8>, dim3(blocks), dim3(256), 0, st, (const f16*)z, (const f16*)ctx, weight,
                           (f16*)x2, C, T, HW, s, L);
    else
        hipLaunchKernelGGL(cfg_input_loop_kernel<1>, dim3(blocks), dim3(256), 0, st, (const f16*)z, (const f16*)ctx, weight,
                           (f16*)x2, C, T, HW, s, L);
    return vdx_launch_status("vdx_cfg_input_loop_f16");
}
