// step_chains.h — the per-element rounding chains of the fused CFG + sampler steps, written once: the guidance policies of
// step_common.h (the plain steps of dpm.hip and codenoise.hip), rescale.hip (`cfg_rescale_elem` between the combine and the tails)
// and dynthresh.hip (`cfg_mimic_elem` likewise) all call these, so they cannot drift apart; likewise `add_noise`'s chain for
// vid2vid.hip and inpaint.hip (the masked step re-noises the kept cells with exactly video-to-video's start).  Every function is
// __forceinline__: a kernel that calls one compiles to the instructions it had when the chain was written in its loop.
#pragma once
#include "vdx_common.h"

// fp32 -> fp16 as its own rounding step: the empty asm keeps hipcc from fusing the preceding fp32
// op and this conversion into v_fma_mixlo_f16 (one rounding), so results match torch's
// "compute in fp32, then cast" for fp16 tensors bit for bit.
__device__ __forceinline__ f16 rn16(float x) {
    asm volatile("" : "+v"(x));
    return (f16)x;
}

// ---- DDIMScheduler.add_noise (diffusers; vid2vid.hip `vdx_add_noise_f16`, inpaint.hip `vdx_mask_renoise_f16`) ----------------
//   x_t = sqrt(a_t) * x0 + sqrt(1 - a_t) * noise        fp16 tensors, fp16-valued 0-d coefficients: every op rounds to fp16
__device__ __forceinline__ f16 add_noise_elem(float x0, float noise, float sa, float s1) {
    const f16 a = rn16(__fmul_rn(sa, x0));                // sqrt(a_t) * x0
    const f16 b = rn16(__fmul_rn(s1, noise));             // sqrt(1-a_t) * noise
    return rn16(__fadd_rn((float)a, (float)b));
}

// ---- fsdp_chunked_coherent.py:141-142 -------------------------------------------------------
//   u, c = noise.chunk(2);  lat = sched.step(u + gs*(c-u), t, lat).prev_sample     (DDIM, eta 0)
// DDIMScheduler.step with fp32 0-d coefficients and fp16 tensors: every tensor op rounds to fp16.
// `sa` is 1/sqrt(a_t): torch-GPU divides by a CPU scalar by multiplying with its reciprocal.
struct ddim_coef {
    float gs, s1, sa, sp, s1p;
};
// the classifier-free-guidance combine both samplers start with:  g = u + gs*(c - u)
__device__ __forceinline__ f16 cfg_combine(float u, float c, float gs) {
    const f16 t1 = rn16(__fsub_rn(c, u));                 // c - u
    const f16 t2 = rn16(__fmul_rn(gs, (float)t1));        // gs * (c - u)
    return rn16(__fadd_rn(u, (float)t2));                 // u + gs*(c-u)
}
// the DDIM step on a (guided) noise g
__device__ __forceinline__ f16 ddim_tail(f16 g, float x, const ddim_coef& k) {
    const f16 a1 = rn16(__fmul_rn(k.s1, (float)g));       // sqrt(1-a_t) * eps
    const f16 a2 = rn16(__fsub_rn(x, (float)a1));         // sample - ...
    const f16 x0 = rn16(__fmul_rn((float)a2, k.sa));      // * (1/sqrt(a_t)): torch-GPU divides by a CPU scalar this way
    const f16 d = rn16(__fmul_rn(k.s1p, (float)g));       // sqrt(1-a_prev) * eps
    const f16 b1 = rn16(__fmul_rn(k.sp, (float)x0));      // sqrt(a_prev) * x0
    return rn16(__fadd_rn((float)b1, (float)d));
}
__device__ __forceinline__ f16 cfg_ddim_elem(float u, float c, float x, const ddim_coef& k) {
    return ddim_tail(cfg_combine(u, c, k.gs), x, k);
}

// ---- CFG rescale (Lin et al. 2023, section 3.4; diffusers `rescale_noise_cfg`; rescale.hip states the statistics) ------------
//   g' = phi * (g * r) + (1 - phi) * g        r = std(c) / std(g), one fp16-valued scalar per sample; phi1 = fp32(1 - phi)
__device__ __forceinline__ f16 cfg_rescale_elem(f16 g, float r, float phi, float phi1) {
    const f16 h1 = rn16(__fmul_rn((float)g, r));          // g * r
    const f16 h2 = rn16(__fmul_rn(phi, (float)h1));       // phi * (g * r)
    const f16 h3 = rn16(__fmul_rn(phi1, (float)g));       // (1 - phi) * g
    return rn16(__fadd_rn((float)h2, (float)h3));
}

// ---- dynamic thresholding with a mimic scale (dynthresh.hip states the statistics) -------------------------------------------
//   dc = clamp(d, -s, s),  g' = ((dc / s) * ref_lo) + mg      d = g - mg, the guided noise less its channel's mean; s, ref_lo, mg:
//   the channel's fp16-valued scalars.  The compares are float compares (a NaN d stays NaN), the division is a division.
__device__ __forceinline__ f16 cfg_mimic_elem(f16 d, float s, float ref_lo, float mg) {
    const float df = (float)d;
    const float dc = df > s ? s : (df < -s ? -s : df);
    const f16 h1 = rn16(__fdiv_rn(dc, s));                // dc / s
    const f16 h2 = rn16(__fmul_rn((float)h1, ref_lo));    // (dc / s) * ref_lo
    return rn16(__fadd_rn((float)h2, mg));
}

// ---- DPM-Solver++ (2M, midpoint): dpm.hip's header states the expression ----------------------
struct dpm_coef {
    float gs, s0, inv_a0, cx, d0, d1, inv_r0;
};

// the DPM-Solver++ step on a (guided) noise g
template <bool O2>
__device__ __forceinline__ void dpm_tail(f16 g, float x, float x0p, const dpm_coef& k, f16& x0_out, f16& out) {
    const f16 a1 = rn16(__fmul_rn(k.s0, (float)g));               // s0 * e
    const f16 a2 = rn16(__fsub_rn(x, (float)a1));                 // x - s0*e
    const f16 x0 = rn16(__fmul_rn((float)a2, k.inv_a0));          // / a0
    const f16 A = rn16(__fmul_rn(k.cx, x));                       // (st/s0) * x
    const f16 B = rn16(__fmul_rn(k.d0, (float)x0));               // -(at*(exp(-h)-1)) * x0
    f16 r = rn16(__fadd_rn((float)A, (float)B));
    if (O2) {
        const f16 dx = rn16(__fsub_rn((float)x0, x0p));           // x0 - x0_prev
        const f16 d1 = rn16(__fmul_rn(k.inv_r0, (float)dx));      // D1 = (1/r0) * (x0 - x0_prev)
        const f16 C = rn16(__fmul_rn(k.d1, (float)d1));           // -(0.5*at*(exp(-h)-1)) * D1
        r = rn16(__fadd_rn((float)r, (float)C));
    }
    x0_out = x0;
    out = r;
}

template <bool CFG, bool O2>
__device__ __forceinline__ void dpm_elem(float u, float c, float x, float x0p, const dpm_coef& k, f16& x0_out, f16& out) {
    dpm_tail<O2>(CFG ? cfg_combine(u, c, k.gs) : (f16)u, x, x0p, k, x0_out, out);
}

// ---- the stochastic samplers' one extra link (DDIM with eta > 0; SDE-DPM-Solver++): after the tail, out = out + c_n * w ---------
//   w: the step's N(0, 1) draw for this element (fp16), c_n: the host's fp32 scalar (DDIM: eta's std; SDE: st * sqrt(1 - exp(-2h)))
__device__ __forceinline__ f16 noise_term(f16 out, f16 w, float c_n) {
    const f16 n1 = rn16(__fmul_rn(c_n, (float)w));        // c_n * w
    return rn16(__fadd_rn((float)out, (float)n1));
}
