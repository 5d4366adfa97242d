// dpm.hip — the plain one-buffer sampler steps, four deterministic and (at the end of the file) their four stochastic forms: DDIM (`DDIMScheduler.step`, eta 0) and DPM-Solver++ (2M, midpoint; vdx/scheduler.py
// `DPMSolverMultistepScheduler`), each alone and fused with the classifier-free-guidance combine.  What diffusers' schedulers run as
// about a dozen elementwise launches per step is one pass here (reads 2n + n (+ n) halves, writes n or 2n), through the one-buffer
// step kernel and launcher of step_common.h with `cfg_guidance` / `no_guidance`; the chains are step_chains.h's.
//
// Rounding: the coefficients are fp32 scalars the host evaluated, every TENSOR operation rounds to fp16, in the order the expression
// is written, and `/ a` is `* (1/a)` (torch-GPU divides by a host scalar that way).
//
// DDIM (fsdp_chunked_coherent.py:141-142):   u, c = noise.chunk(2);  lat = sched.step(u + gs*(c-u), t, lat).prev_sample
// The two DDIM entries take any fp16 tensors: the access narrows to what n and the pointers' alignment allow, down to one half.
//
// DPM-Solver++: with e the (guided) model output, x the sample, (s0, a0) from sigma_i, (st, at) from sigma_{i+1},
// h = lambda_t - lambda_0, k = at * (exp(-h) - 1):
//     x0  = (x - s0*e) / a0                                  stored: the next step's history
//     x'  = (st/s0)*x - k*x0                                 first order (no history, solver_order 1, the last step)
//     x'  = (st/s0)*x - k*x0 - (0.5*k) * ((1/r0) * (x0 - x0_prev))        second order, r0 = (lambda_0 - lambda_1) / h
// The C ABI takes c_x = st/s0, c_d0 = -k, c_d1 = -(0.5*k), c_inv_r0 = 1/r0 and ADDS: x' = c_x*x + c_d0*x0 + c_d1*D1.  In IEEE
// arithmetic a - b is a + (-b) and fp16(-k*y) is -fp16(k*y), so these are the bits of the subtractions above (on the last
// step, sigma 0, c_x = 0 and c_d0 = 1, and x' is x0).  The two DPM entries want 16-byte aligned pointers.
#include <cstdint>

#include "vdx_common.h"
#include "step_common.h"
#include "step_noise.h"    // the stochastic forms' noise policy

static const co_buf no_extra[] = {{nullptr, 0}};

extern "C" int vdx_cfg_ddim_step_f16(const void* eps2, const void* lat, void* lat_out, float guidance, float sqrt_one_minus_at,
                                     float sqrt_at, float sqrt_aprev, float sqrt_one_minus_aprev, size_t n, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return direct_launch("vdx_cfg_ddim_step_f16", 0, true, eps2, lat, nullptr, nullptr, lat_out, no_extra, kd, dpm_coef{}, cfg_guidance{},
                         1, n, 4096, stream);
}

// the caller did the CFG combine (the unchanged reference script)
extern "C" int vdx_ddim_step_f16(const void* eps, const void* lat, void* lat_out, float sqrt_one_minus_at, float sqrt_at,
                                 float sqrt_aprev, float sqrt_one_minus_aprev, size_t n, vdx_stream_t stream) {
    const ddim_coef kd = {0.f, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return direct_launch("vdx_ddim_step_f16", 0, true, eps, lat, nullptr, nullptr, lat_out, no_extra, kd, dpm_coef{}, no_guidance{}, 1, n,
                         4096, stream);
}

extern "C" int vdx_cfg_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                                    float guidance, float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1,
                                    float c_inv_r0, size_t n, vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return direct_launch("vdx_cfg_dpm_step_f16", 1, false, eps2, lat, x0_prev, x0_out, lat_out, no_extra, ddim_coef{}, kp, cfg_guidance{},
                         1, n, 4096, stream);
}

extern "C" int vdx_dpm_step_f16(const void* eps, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                                float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, size_t n,
                                vdx_stream_t stream) {
    const dpm_coef kp = {0.f, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return direct_launch("vdx_dpm_step_f16", 1, false, eps, lat, x0_prev, x0_out, lat_out, no_extra, ddim_coef{}, kp, no_guidance{}, 1, n,
                         4096, stream);
}

// ---- the stochastic forms: DDIM with eta > 0 and SDE-DPM-Solver++ (2M, midpoint) ------------------------------------------------------
// The same kernel with the "philox" noise policy (step_noise.h): the deterministic tail with other host coefficients, then
// lat' = fp16(lat' + fp16(c_n * w)), w the portable generator's N(0, 1) at the element's place in the whole clip (1,C,T,h,w), of
// which the sample (1,C,L,h,w) is the frames [s, s + L).  One launch, nchan = C and M = L * HW; nothing but the draw is new.
//   DDIM, eta in (0, 1]:   std = eta * sqrt(((1-a_prev)/(1-a_t)) * (1 - a_t/a_prev)); the tail's sqrt(1-a_prev) is
//                          sqrt(1 - a_prev - std^2) (`dir_coef`), c_n = std
//   SDE-DPM-Solver++:      c_x = (st/s0)*exp(-h), c_d0 = at*(1 - exp(-2h)), c_d1 = 0.5*c_d0, c_n = st*sqrt(1 - exp(-2h))
template <class G>
static int direct_noise(const char* what, int mode, const void* eps, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                        ddim_coef kd, dpm_coef kp, float c_n, size_t seed, size_t noise_stream, int C, int T, int HW, int s, int L,
                        vdx_stream_t stream) {
    philox_noise nz;
    if (int rc = philox_noise_of(what, seed, noise_stream, c_n, C, T, HW, s, L, nz)) return rc;
    return direct_launch(what, mode, mode == 0, eps, lat, x0_prev, x0_out, lat_out, no_extra, kd, kp, G{}, (unsigned)C, (size_t)L * HW,
                         4096, stream, nz);
}

extern "C" int vdx_cfg_ddim_eta_step_f16(const void* eps2, const void* lat, void* lat_out, float guidance, float sqrt_one_minus_at,
                                         float sqrt_at, float sqrt_aprev, float dir_coef, float c_n, size_t seed, size_t noise_stream,
                                         int C, int T, int HW, int s, int L, vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, dir_coef};
    return direct_noise<cfg_guidance>("vdx_cfg_ddim_eta_step_f16", 0, eps2, lat, nullptr, nullptr, lat_out, kd, dpm_coef{}, c_n, seed,
                                      noise_stream, C, T, HW, s, L, stream);
}

extern "C" int vdx_ddim_eta_step_f16(const void* eps, const void* lat, void* lat_out, float sqrt_one_minus_at, float sqrt_at,
                                     float sqrt_aprev, float dir_coef, float c_n, size_t seed, size_t noise_stream, int C, int T, int HW,
                                     int s, int L, vdx_stream_t stream) {
    const ddim_coef kd = {0.f, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, dir_coef};
    return direct_noise<no_guidance>("vdx_ddim_eta_step_f16", 0, eps, lat, nullptr, nullptr, lat_out, kd, dpm_coef{}, c_n, seed,
                                     noise_stream, C, T, HW, s, L, stream);
}

extern "C" int vdx_cfg_sde_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                                        float guidance, float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0,
                                        float c_n, size_t seed, size_t noise_stream, int C, int T, int HW, int s, int L,
                                        vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return direct_noise<cfg_guidance>("vdx_cfg_sde_dpm_step_f16", 1, eps2, lat, x0_prev, x0_out, lat_out, ddim_coef{}, kp, c_n, seed,
                                      noise_stream, C, T, HW, s, L, stream);
}

extern "C" int vdx_sde_dpm_step_f16(const void* eps, const void* lat, const void* x0_prev, void* x0_out, void* lat_out, float c_s0,
                                    float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, float c_n, size_t seed,
                                    size_t noise_stream, int C, int T, int HW, int s, int L, vdx_stream_t stream) {
    const dpm_coef kp = {0.f, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return direct_noise<no_guidance>("vdx_sde_dpm_step_f16", 1, eps, lat, x0_prev, x0_out, lat_out, ddim_coef{}, kp, c_n, seed,
                                     noise_stream, C, T, HW, s, L, stream);
}
