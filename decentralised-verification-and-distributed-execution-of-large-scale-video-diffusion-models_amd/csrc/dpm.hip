// dpm.hip — the DPM-Solver++ (2M, midpoint) sample update of vdx/scheduler.py `DPMSolverMultistepScheduler`, fused
// with the classifier-free-guidance combine: what diffusers' `DPMSolverMultistepScheduler.step` runs as about a dozen
// elementwise launches per step is one pass here (reads 2n + n (+ n) halves, writes 2n).
//
// Rounding is `cfg_ddim_kernel`'s (elementwise.hip): the coefficients are fp32 scalars the host evaluated, every TENSOR
// operation rounds to fp16, in the order the expression is written, and `/ a0` is `* (1/a0)` (torch-GPU divides by a
// host scalar that way).  With e the (guided) model output, x the sample, (s0, a0) from sigma_i, (st, at) from
// sigma_{i+1}, h = lambda_t - lambda_0, k = at * (exp(-h) - 1):
//     x0  = (x - s0*e) / a0                                  stored: the next step's history
//     x'  = (st/s0)*x - k*x0                                 first order (no history, solver_order 1, the last step)
//     x'  = (st/s0)*x - k*x0 - (0.5*k) * ((1/r0) * (x0 - x0_prev))        second order, r0 = (lambda_0 - lambda_1) / h
// The C ABI takes c_x = st/s0, c_d0 = -k, c_d1 = -(0.5*k), c_inv_r0 = 1/r0 and ADDS: x' = c_x*x + c_d0*x0 + c_d1*D1.  In IEEE
// arithmetic a - b is a + (-b) and fp16(-k*y) is -fp16(k*y), so these are the bits of the subtractions above (on the last
// step, sigma 0, c_x = 0 and c_d0 = 1, and x' is x0).
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"   // rn16, dpm_coef, dpm_elem: shared with codenoise.hip

// 8 halves of the conditional half of eps2, which starts n halves behind a 16-byte boundary: one 16-byte load where n is a
// multiple of 8 (`al`, the same for every lane), else element by element.  Every other pointer is 16-byte aligned (checked).
__device__ __forceinline__ f16x8 load8(const f16* p, bool al) {
    if (al) return *(const f16x8*)p;
    f16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p[j];
    return v;
}

// Elements [0, 8*(n/8)) in groups of 8 per lane, the tail [8*(n/8), n) one per lane, in the same launch.  Every element is
// read and written by one lane only, so `out` may be `lat`, and the result does not depend on the grid.
template <bool CFG, bool O2>
__global__ __launch_bounds__(256) void dpm_kernel(const f16* eps, const f16* lat, const f16* x0_prev, f16* x0_out,
                                                  f16* out, dpm_coef k, size_t n, bool c_al) {
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t nv = n >> 3;
    const f16* epc = eps + n;                                     // the conditional half of eps2 (CFG only)
    for (size_t v = gid; v < nv; v += stride) {
        const size_t i = v << 3;
        const f16x8 u8 = *(const f16x8*)(eps + i), x8 = *(const f16x8*)(lat + i);
        f16x8 c8 = u8, p8 = u8;
        if (CFG) c8 = load8(epc + i, c_al);
        if (O2) p8 = *(const f16x8*)(x0_prev + i);
        f16x8 o8, z8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            f16 z, o;
            dpm_elem<CFG, O2>((float)u8[j], (float)c8[j], (float)x8[j], (float)p8[j], k, z, o);
            z8[j] = z;
            o8[j] = o;
        }
        *(f16x8*)(x0_out + i) = z8;
        *(f16x8*)(out + i) = o8;
    }
    for (size_t i = (nv << 3) + gid; i < n; i += stride) {
        f16 z, o;
        dpm_elem<CFG, O2>((float)eps[i], CFG ? (float)epc[i] : 0.f, (float)lat[i], O2 ? (float)x0_prev[i] : 0.f, k, z, o);
        x0_out[i] = z;
        out[i] = o;
    }
}

static inline bool dpm_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

static int dpm_launch(const char* what, bool cfg, const void* eps, const void* lat, const void* x0_prev, void* x0_out,
                      void* lat_out, dpm_coef k, size_t n, vdx_stream_t stream) {
    VDX_CHECK(eps && lat && x0_out && lat_out && n > 0, "%s: bad arguments", what);
    VDX_CHECK(n <= ((size_t)1 << 40), "%s: n too large", what);
    const size_t nb = n * sizeof(f16), neps = cfg ? 2 * nb : nb;
    const void* ptrs[5] = {eps, lat, x0_prev, x0_out, lat_out};
    for (const void* p : ptrs) VDX_CHECK(((uintptr_t)p & 15) == 0, "%s: pointer not 16-byte aligned", what);
    // a lane reads its elements before it writes them, and writes nobody else's: lat_out == lat is fine.  Everything
    // else that shares memory would be read after it was overwritten by another lane, or hold two results.
    VDX_CHECK(!x0_prev || x0_out != x0_prev, "%s: x0_out must not be x0_prev (ping-pong two history buffers)", what);
    VDX_CHECK(lat_out == lat || !dpm_overlap(lat_out, nb, lat, nb), "%s: lat_out overlaps lat without being lat", what);
    VDX_CHECK(!dpm_overlap(x0_out, nb, lat_out, nb) && !dpm_overlap(x0_out, nb, lat, nb) &&
                  !dpm_overlap(x0_out, nb, eps, neps) && !dpm_overlap(lat_out, nb, eps, neps),
              "%s: outputs overlap an input or each other", what);
    VDX_CHECK(!x0_prev || (!dpm_overlap(x0_prev, nb, x0_out, nb) && !dpm_overlap(x0_prev, nb, lat_out, nb)),
              "%s: x0_prev overlaps an output", what);
    const bool al = (n & 7) == 0;                                 // eps2's second half starts on a 16-byte boundary
    const size_t nv = n >> 3, want = nv ? (nv + 255) / 256 : 1;
    const dim3 grid((unsigned)(want < 4096 ? want : 4096)), block(256);
    const hipStream_t s = (hipStream_t)stream;
    const f16 *e = (const f16*)eps, *x = (const f16*)lat, *p = (const f16*)x0_prev;
    f16 *z = (f16*)x0_out, *o = (f16*)lat_out;
    if (cfg && x0_prev) hipLaunchKernelGGL((dpm_kernel<true, true>), grid, block, 0, s, e, x, p, z, o, k, n, al);
    else if (cfg) hipLaunchKernelGGL((dpm_kernel<true, false>), grid, block, 0, s, e, x, p, z, o, k, n, al);
    else if (x0_prev) hipLaunchKernelGGL((dpm_kernel<false, true>), grid, block, 0, s, e, x, p, z, o, k, n, al);
    else hipLaunchKernelGGL((dpm_kernel<false, false>), grid, block, 0, s, e, x, p, z, o, k, n, al);
    return vdx_launch_status(what);
}

extern "C" int vdx_cfg_dpm_step_f16(const void* eps2, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                                    float guidance, float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1,
                                    float c_inv_r0, size_t n, vdx_stream_t stream) {
    const dpm_coef k = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return dpm_launch("vdx_cfg_dpm_step_f16", true, eps2, lat, x0_prev, x0_out, lat_out, k, n, stream);
}

extern "C" int vdx_dpm_step_f16(const void* eps, const void* lat, const void* x0_prev, void* x0_out, void* lat_out,
                                float c_s0, float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, size_t n,
                                vdx_stream_t stream) {
    const dpm_coef k = {0.f, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return dpm_launch("vdx_dpm_step_f16", false, eps, lat, x0_prev, x0_out, lat_out, k, n, stream);
}
