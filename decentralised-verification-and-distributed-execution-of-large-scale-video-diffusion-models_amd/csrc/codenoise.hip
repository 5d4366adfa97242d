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
// Seamless looping (AnimateDiff's `closed_loop` context option; vdx/codenoise.py `loop_plan`, `DiffuserConfig.loop`) places the
// same windows on a RING: a row (off, s, L) means the frames (s + f) mod T, f in [0, L), with 0 <= s < T and 1 <= L <= T, so the
// last window wraps over the clip's end into its first frames and frames T-1 and 0 are denoised together in one UNet call.
//
//   vdx_cfg_input_loop_f16         `vdx_cfg_input_window_f16` reading frame (s + f) mod T: the (2,C,L,h,w) UNet input.
//   vdx_coloop_cfg_ddim_step_f16   the vdx_cofuse_* steps with the modular rule: per (c, t) line, for k ascending, f = t - s_k,
//   vdx_coloop_cfg_dpm_step_f16    f += T if f < 0, the window is skipped if f >= L_k.
// These are the same kernels with the RING flag set (`cofuse_step_kernel`, `cfg_input_window_kernel`): a table in which no
// window wraps gives the bits of the vdx_cofuse_* step.  The wrap is a compare and an add / subtract on a block-uniform (step) or
// per-vector (input) integer, never a division.
//
// Strided context windows (AnimateDiff-Evolved's `context_stride`, the "uniform" schedule; vdx/codenoise.py `stride_plan`,
// `DiffuserConfig.context_stride`; no reference counterpart) add windows that take every d-th frame: a row (off, s, L, d) means the
// frames s + f * d, f in [0, L), with d >= 1 and s + (L - 1) * d < T, so frames further apart than a window share a UNet call.
//
//   vdx_cfg_input_stride_f16        `vdx_cfg_input_window_f16` reading frame s + f * d: the (2,C,L,h,w) UNet input.
//   vdx_costride_cfg_ddim_step_f16  the vdx_cofuse_* steps with the strided rule: per (c, t) line, for k ascending, q = t - s_k;
//   vdx_costride_cfg_dpm_step_f16   window k enters with its frame q / d_k if q >= 0, q % d_k == 0 and q / d_k < L_k.
// Again the same kernels: `cofuse_step_kernel` with a `costride_tab` (the table with a fourth column, 1.25 KiB by value) and
// `cfg_input_window_kernel` with the STRIDE flag.  A table whose strides are all 1 gives the bits of the vdx_cofuse_* step.  The
// division is one unsigned division per window on block-uniform integers (step); the input kernel multiplies.
//
// Block map (cofuse_common.h `cofuse_step_kernel`): a block works on ONE (c, t) line of h*w elements (tiles of 256 lanes x E
// elements), so the window loop, the table reads and the weights are uniform over the block (scalar loads, no divergence).
// E = 8 (16-byte accesses) where every line of z and of every window buffer starts on a 16-byte boundary (h*w and every window
// offset a multiple of 8), E = 4 (8-byte) where they are multiples of 4, else E = 1: a line is then a whole number of vectors
// and there is no tail.  An element is read and written by one lane only: lat_out may be z, nothing is atomic, no index depends
// on data, and a NaN or an infinity stays in its element.  Frames outside a window are never read, whatever wn holds there.
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"
#include "cofuse_common.h"   // the window table, the fuse, the step kernel and its launcher, the host checks
#include "step_noise.h"      // the stochastic steps' noise policy

template <bool RING, class Tab = cofuse_tab>
static int cofuse_plain(const char* what, int mode, const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                        const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev, void* x0_out,
                        void* lat_out, ddim_coef kd, dpm_coef kp, int C, int T, int HW, vdx_stream_t stream,
                        const int* win_stride = nullptr) {
    Tab tab;
    int e;
    if (int rc = cofuse_check(what, mode, true, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev, x0_out, lat_out,
                              C, T, HW, tab, e, RING, win_stride))
        return rc;
    return cofuse_launch<RING>(what, mode, z, windows, tab, e, K, wn, x0_prev, x0_out, lat_out, kd, kp, cfg_guidance{}, C, T, HW, stream);
}

// the stochastic forms of the flat steps (dpm.hip states the coefficients): `cofuse_plain<false>` with the "philox" noise policy
// of step_noise.h.  The sample is the clip, so an element's index is its logical one.
static int cofuse_noise(const char* what, int mode, const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                        const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev, void* x0_out,
                        void* lat_out, ddim_coef kd, dpm_coef kp, float c_n, size_t seed, size_t noise_stream, int C, int T, int HW,
                        vdx_stream_t stream) {
    cofuse_tab tab;
    int e;
    if (int rc = cofuse_check(what, mode, true, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev, x0_out, lat_out,
                              C, T, HW, tab, e))
        return rc;
    philox_noise nz;
    if (int rc = philox_noise_of(what, seed, noise_stream, c_n, C, T, HW, 0, T, nz)) return rc;
    return cofuse_launch<false>(what, mode, z, windows, tab, e, K, wn, x0_prev, x0_out, lat_out, kd, kp, cfg_guidance{}, C, T, HW, stream,
                                nz);
}

extern "C" int vdx_cofuse_cfg_ddim_eta_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                                const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                                float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev, float dir_coef,
                                                float c_n, size_t seed, size_t noise_stream, int C, int T, int HW, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, dir_coef};
    return cofuse_noise("vdx_cofuse_cfg_ddim_eta_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len, K, wn, nullptr,
                        nullptr, lat_out, kd, dpm_coef{}, c_n, seed, noise_stream, C, T, HW, stream);
}

extern "C" int vdx_cofuse_cfg_sde_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                               const int* win_start, const int* win_len, int K, const float* wn, const void* x0_prev,
                                               void* x0_out, void* lat_out, float guidance, float c_s0, float c_inv_a0, float c_x,
                                               float c_d0, float c_d1, float c_inv_r0, float c_n, size_t seed, size_t noise_stream, int C,
                                               int T, int HW, vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return cofuse_noise("vdx_cofuse_cfg_sde_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev,
                        x0_out, lat_out, ddim_coef{}, kp, c_n, seed, noise_stream, C, T, HW, stream);
}

extern "C" int vdx_cofuse_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                            const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                            float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                            float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return cofuse_plain<false>("vdx_cofuse_cfg_ddim_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len, K, wn, nullptr,
                               nullptr, lat_out, kd, dpm_coef{}, C, T, HW, stream);
}

extern "C" int vdx_cofuse_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                           const int* win_start, const int* win_len, int K, const float* wn,
                                           const void* x0_prev, void* x0_out, void* lat_out, float guidance, float c_s0,
                                           float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW,
                                           vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return cofuse_plain<false>("vdx_cofuse_cfg_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev,
                               x0_out, lat_out, ddim_coef{}, kp, C, T, HW, stream);
}

extern "C" int vdx_coloop_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                            const int* win_start, const int* win_len, int K, const float* wn, void* lat_out,
                                            float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                            float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return cofuse_plain<true>("vdx_coloop_cfg_ddim_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len, K, wn, nullptr,
                              nullptr, lat_out, kd, dpm_coef{}, C, T, HW, stream);
}

extern "C" int vdx_coloop_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                           const int* win_start, const int* win_len, int K, const float* wn,
                                           const void* x0_prev, void* x0_out, void* lat_out, float guidance, float c_s0,
                                           float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW,
                                           vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return cofuse_plain<true>("vdx_coloop_cfg_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len, K, wn, x0_prev,
                              x0_out, lat_out, ddim_coef{}, kp, C, T, HW, stream);
}

extern "C" int vdx_costride_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                              const int* win_start, const int* win_len, const int* win_stride, int K, const float* wn,
                                              void* lat_out, float guidance, float sqrt_one_minus_at, float sqrt_at, float sqrt_aprev,
                                              float sqrt_one_minus_aprev, int C, int T, int HW, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return cofuse_plain<false, costride_tab>("vdx_costride_cfg_ddim_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len,
                                             K, wn, nullptr, nullptr, lat_out, kd, dpm_coef{}, C, T, HW, stream, win_stride);
}

extern "C" int vdx_costride_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                             const int* win_start, const int* win_len, const int* win_stride, int K, const float* wn,
                                             const void* x0_prev, void* x0_out, void* lat_out, float guidance, float c_s0,
                                             float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int HW,
                                             vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return cofuse_plain<false, costride_tab>("vdx_costride_cfg_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len,
                                             K, wn, x0_prev, x0_out, lat_out, ddim_coef{}, kp, C, T, HW, stream, win_stride);
}

// ---- the UNet input of one window, straight out of the whole-clip latent ------------------------------------------------
//   x = cat([z[:, :, s:e]]*2);  x = x + context_weight * ctx.repeat(1,1,e-s,1,1)          (cfg_input_kernel's expression)
// RING: z[:, :, (s + arange(L)) % T] instead;  STRIDE: z[:, :, s + d * arange(L)] (d is 1 and unread otherwise)
template <int E, bool RING, bool STRIDE>
__global__ __launch_bounds__(256) void cfg_input_window_kernel(const f16* z, const f16* ctx, float weight, f16* x2, int C, int T,
                                                               int HW, int s, int L, int d) {
    const int hv = HW / E;                                        // vectors per line
    const size_t nv = (size_t)C * L * hv, n = (size_t)C * L * HW;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(v % hv) * E;
        const int f = (int)((v / hv) % L);
        const int c = (int)(v / ((size_t)hv * L));
        int t = STRIDE ? s + f * d : s + f;                       // the host checked s + (L - 1) * d < T
        if constexpr (RING) {
            if (t >= T) t -= T;                                   // s < T and f < L <= T: one wrap at most
        }
        f16 o[E];
        load_halves<E>(z + ((size_t)c * T + t) * HW + p, o);
        if (ctx) add_ctx<E>(o, ctx + (size_t)c * HW + p, weight);
        const size_t dst = ((size_t)c * L + f) * HW + p;
        store_halves<E>(x2 + dst, o);
        store_halves<E>(x2 + n + dst, o);
    }
}

// `last`: the range's end e (flat) or the window's length L (ring, strided); `d`: the frame stride (strided), else 1
template <bool RING, bool STRIDE = false>
static int cfg_input_launch(const char* what, const char* symbol, const void* z, const void* ctx, float weight, void* x2, int C, int T,
                            int HW, int s, int last, vdx_stream_t stream, int d = 1) {
    VDX_CHECK(z && x2 && C > 0 && T > 0 && HW > 0 && HW <= 1 << 30, "%s: bad arguments", what);
    if (STRIDE)
        VDX_CHECK(d >= 1 && 0 <= s && 1 <= last && (long long)s + ((long long)last - 1) * d < T,
                  "%s: bad strided window start %d, length %d, stride %d of %d frames", what, s, last, d, T);
    else if (RING) VDX_CHECK(0 <= s && s < T && 1 <= last && last <= T, "%s: bad ring window start %d, length %d of %d frames", what, s, last, T);
    else VDX_CHECK(0 <= s && s < last && last <= T, "%s: bad range [%d,%d) of %d", what, s, last, T);
    for (const void* ptr : {z, ctx, (const void*)x2}) VDX_CHECK(((uintptr_t)ptr & 15) == 0, "%s: pointer not 16-byte aligned", what);
    const int L = RING || STRIDE ? last : last - s;
    const size_t n = (size_t)C * L * HW;
    VDX_CHECK(!co_overlap(x2, 2 * n * sizeof(f16), z, (size_t)C * T * HW * sizeof(f16)), "%s: x2 overlaps z", what);
    const int E = HW % 8 == 0 ? 8 : 1;                            // every line of z, ctx and both halves of x2 is then 16-byte aligned
    const size_t nv = n / E;
    VDX_CHECK((nv + 255) / 256 <= 0x7fffffffull, "%s: window too large", what);
    const unsigned blocks = (unsigned)((nv + 255) / 256);         // no cap: one vector per lane
    const hipStream_t st = (hipStream_t)stream;
    if (E == 8)
        hipLaunchKernelGGL((cfg_input_window_kernel<8, RING, STRIDE>), dim3(blocks), dim3(256), 0, st, (const f16*)z, (const f16*)ctx,
                           weight, (f16*)x2, C, T, HW, s, L, d);
    else
        hipLaunchKernelGGL((cfg_input_window_kernel<1, RING, STRIDE>), dim3(blocks), dim3(256), 0, st, (const f16*)z, (const f16*)ctx,
                           weight, (f16*)x2, C, T, HW, s, L, d);
    return vdx_launch_status(symbol);
}

extern "C" int vdx_cfg_input_stride_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int HW, int s, int L,
                                        int d, vdx_stream_t stream) {
    return cfg_input_launch<false, true>("cfg_input_stride", "vdx_cfg_input_stride_f16", z, ctx, weight, x2, C, T, HW, s, L, stream, d);
}

extern "C" int vdx_cfg_input_window_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int HW, int s,
                                        int e, vdx_stream_t stream) {
    return cfg_input_launch<false>("cfg_input_window", "vdx_cfg_input_window_f16", z, ctx, weight, x2, C, T, HW, s, e, stream);
}

extern "C" int vdx_cfg_input_loop_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int HW, int s, int L,
                                      vdx_stream_t stream) {
    return cfg_input_launch<true>("cfg_input_loop", "vdx_cfg_input_loop_f16", z, ctx, weight, x2, C, T, HW, s, L, stream);
}
