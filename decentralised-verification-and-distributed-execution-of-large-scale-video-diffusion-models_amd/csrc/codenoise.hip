// codenoise.hip — temporal co-denoising (MultiDiffusion along time; Gen-L-Video's "temporal co-denoising"; no reference
// counterpart, opt-in: vdx/codenoise.py, `DiffuserConfig.co_denoise`).  ONE latent z (1,C,T,h,w) for the whole clip; at every
// step each window k predicts noise for its frames [s_k, s_k + L_k), the predictions are averaged per frame with normalised
// weights wn[k][t] (they sum to 1 over the windows that hold frame t), and ONE scheduler step advances the whole clip.
//
//   vdx_cfg_input_window_f16       `vdx_cfg_input_f16` reading frames [s, e) out of z: the contiguous (2,C,e-s,h,w) UNet input
//                                  in one launch, no slice copy; the ctx term has `cfg_input_kernel`'s two roundings.
//   vdx_cofuse_cfg_ddim_step_f16   per element (c, t, p), over the windows k (ascending) with s_k <= t < s_k + L_k:
//   vdx_cofuse_cfg_dpm_step_f16        U = sum_k wn[k][t] * fp32(u_k),  Cc = sum_k wn[k][t] * fp32(c_k)
//                                  every product one fp32 rounding, every add another (no fma; the sum STARTS with the first
//                                  product, nothing is added to a zero), then u = rn16(U), c = rn16(Cc), and from there the
//                                  chain of `vdx_cfg_ddim_step_f16` / `vdx_cfg_dpm_step_f16` itself (step_chains.h).
// A frame that one window covers has wn = 1.0f: 1.0f * fp32(u) is u, rn16 gives the fp16 bits back, and the new latent has
// the bits the plain fused step gives that window.
//
// Block map: a block works on ONE (c, t) line of h*w elements (tiles of 256 lanes x E elements), so the window loop, the
// table reads and the weights are uniform over the block (scalar loads, no divergence).  E = 8 (16-byte accesses) where
// every line of z and of every window buffer starts on a 16-byte boundary (h*w and every window offset a multiple of 8),
// E = 4 (8-byte) where they are multiples of 4, else E = 1: a line is then a whole number of vectors and there is no tail.
// An element is read and written by one lane only: lat_out may be z, nothing is atomic, no index depends on data, and a NaN
// or an infinity stays in its element.  Frames outside a window's [s_k, s_k + L_k) are never read, whatever wn holds there.
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"
#include "cofuse_common.h"   // the window table, the fuse, the host checks: shared with rescale.hip

// MODE 0: DDIM; 1: DPM-Solver++ first order; 2: second order
template <int MODE, int E>
__global__ __launch_bounds__(256) void cofuse_kernel(const f16* z, const f16* win, cofuse_tab tab, int K, const float* wn,
                                                     const f16* x0_prev, f16* x0_out, f16* out, ddim_coef kd, dpm_coef kp,
                                                     int C, int T, int HW, unsigned tiles_per_line) {
    const unsigned line = blockIdx.x / tiles_per_line, tile = blockIdx.x - line * tiles_per_line;
    const int c = (int)(line / (unsigned)T), t = (int)(line - (unsigned)c * (unsigned)T);
    const int p = (int)((tile * 256u + threadIdx.x) * (unsigned)E);
    if (p >= HW) return;                                          // HW is a multiple of E: a lane's E elements are all inside
    float uf[E], cf[E];
    cofuse_uc<E>(win, tab, K, wn, C, T, HW, c, t, p, uf, cf);      // uniform over the block: t is
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

static int cofuse_launch(const char* what, int mode, const void* z, const void* windows, size_t windows_elems,
                         const int64_t* win_off, const int* win_start, const int* win_len, int K, const float* wn,
                         const void* x0_prev, void* x0_out, void* lat_out, ddim_coef kd, dpm_coef kp, int C, int T, int HW,
                         vdx_stream_t stream) {
    cofuse_tab tab;
    int e;
    if (int rc = cofuse_check(what, mode, true, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev, x0_out, lat_out,
                              C, T, HW, tab, e))
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
#define COFUSE_GO(M, EE) hipLaunchKernelGGL((cofuse_kernel<M, EE>), grid, block, 0, st, zz, ww, tab, K, wn, pp, xo, oo, kd, kp, C, T, HW, tpl)
#define COFUSE_E(M)                  \
    do {                             \
        if (e == 8) COFUSE_GO(M, 8); \
        else if (e == 4) COFUSE_GO(M, 4); \
        else COFUSE_GO(M, 1);        \
    } while (0)
    if (mode == 0) COFUSE_E(0);
    else if (!x0_prev) COFUSE_E(1);
    else COFUSE_E(2);
#undef COFUSE_E
#undef COFUSE_GO
    return vdx_launch_status(what);
}

extern "C" int vdx_cofuse_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                            const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                            float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                            float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return cofuse_launch("vdx_cofuse_cfg_ddim_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len, K, wn, nullptr,
                         nullptr, lat_out, kd, dpm_coef{}, C, T, HW, stream);
}

extern "C" int vdx_cofuse_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                           const int* win_start, const int* win_len, int K, const float* wn,
                                           const void* x0_prev, void* x0_out, void* lat_out, float guidance, float c_s0,
                                           float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW,
                                           vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return cofuse_launch("vdx_cofuse_cfg_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev,
                         x0_out, lat_out, ddim_coef{}, kp, C, T, HW, stream);
}

// ---- the UNet input of one window, straight out of the whole-clip latent ------------------------------------------------
//   x = cat([z[:, :, s:e]]*2);  x = x + context_weight * ctx.repeat(1,1,e-s,1,1)          (cfg_input_kernel's expression)
template <int E>
__global__ __launch_bounds__(256) void cfg_input_window_kernel(const f16* z, const f16* ctx, float weight, f16* x2, int C, int T,
                                                               int HW, int s, int L) {
    const int hv = HW / E;                                        // vectors per line
    const size_t nv = (size_t)C * L * hv, n = (size_t)C * L * HW;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(v % hv) * E;
        const int f = (int)((v / hv) % L);
        const int c = (int)(v / ((size_t)hv * L));
        f16 o[E];
        load_halves<E>(z + ((size_t)c * T + s + f) * HW + p, o);
        if (ctx) {
            f16 cx[E];
            load_halves<E>(ctx + (size_t)c * HW + p, cx);
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const f16 t = rn16(__fmul_rn((float)cx[j], weight));   // fp16(cw * ctx)
                o[j] = rn16(__fadd_rn((float)o[j], (float)t));         // fp16(x + t)
            }
        }
        const size_t d = ((size_t)c * L + f) * HW + p;
        store_halves<E>(x2 + d, o);
        store_halves<E>(x2 + n + d, o);
    }
}

extern "C" int vdx_cfg_input_window_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int HW, int s,
                                        int e, vdx_stream_t stream) {
    VDX_CHECK(z && x2 && C > 0 && T > 0 && HW > 0 && HW <= 1 << 30, "cfg_input_window: bad arguments");
    VDX_CHECK(0 <= s && s < e && e <= T, "cfg_input_window: bad range [%d,%d) of %d", s, e, T);
    for (const void* ptr : {z, ctx, (const void*)x2}) VDX_CHECK(((uintptr_t)ptr & 15) == 0, "cfg_input_window: pointer not 16-byte aligned");
    const int L = e - s;
    const size_t n = (size_t)C * L * HW;
    VDX_CHECK(!co_overlap(x2, 2 * n * sizeof(f16), z, (size_t)C * T * HW * sizeof(f16)), "cfg_input_window: x2 overlaps z");
    const int E = HW % 8 == 0 ? 8 : 1;                            // every line of z, ctx and both halves of x2 is then 16-byte aligned
    const size_t nv = n / E;
    VDX_CHECK((nv + 255) / 256 <= 0x7fffffffull, "cfg_input_window: window too large");
    const unsigned blocks = (unsigned)((nv + 255) / 256);         // no cap: one vector per lane
    const hipStream_t st = (hipStream_t)stream;
    if (E == 8)
        hipLaunchKernelGGL(cfg_input_window_kernel<8>, dim3(blocks), dim3(256), 0, st, (const f16*)z, (const f16*)ctx, weight,
                           (f16*)x2, C, T, HW, s, L);
    else
        hipLaunchKernelGGL(cfg_input_window_kernel<1>, dim3(blocks), dim3(256), 0, st, (const f16*)z, (const f16*)ctx, weight,
                           (f16*)x2, C, T, HW, s, L);
    return vdx_launch_status("vdx_cfg_input_window_f16");
}
