// step_noise.h — the "philox" noise policy of the stochastic sampler steps (step_common.h states what a noise policy is): DDIM with
// eta > 0 and SDE-DPM-Solver++ are the deterministic tail run with other host coefficients plus `c_n * w`, and w is the portable
// generator's N(0, 1) (noise_common.h) drawn inside the step kernel: no buffer of noise, no second launch.
//
// w of an element is what `vdx_noise_f16` holds for the LOGICAL tensor (1,C,T,h,w) of the whole clip at that element's place in the
// clip, under the step's seed and stream, with sigma 1: a sample that is the frames [s, s + L) of the clip adds, to the frames it
// shares with another sample, the noise that one adds.  The kernel's index i runs over the sample (C, L, HW); its channel is
// blockIdx.y (the one-buffer launch: nchan = C, M = L * HW), so
//     logical = i + blockIdx.y * (T - L) * HW + s * HW
// and where the sample is the clip (the co-denoising step, whose grid has no y) both offsets are 0 and logical = i.
//
// Width: where `skip` and `base` are multiples of 4 (of 8 for the 16-byte access: `co_narrow`) every vector of 4 starts a Philox
// block, and a lane computes one block per four elements, two for a width of 8.  Otherwise the host narrows the access to 1 and
// each element computes its block and picks its word pair, as noise.hip's `noise_elem_kernel` does.  All index arithmetic is
// 64-bit; no atomics, no data-dependent address, no state.  Every file that includes this is built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#include "vdx_common.h"
#include "noise_common.h"
#include "step_common.h"

struct philox_noise {
    static constexpr bool draws = true;
    philox_key key;
    float c_n;
    uint64_t skip, base;         // (T - L) * HW and s * HW

    void narrow(int& e) const {
        co_narrow(e, (long long)skip);
        co_narrow(e, (long long)base);
    }

    template <int E>
    __device__ __forceinline__ void draw(size_t i, f16 (&w)[E]) const {
        const uint64_t l = (uint64_t)i + (uint64_t)blockIdx.y * skip + base;
        if constexpr (E == 1) {
            uint32_t x[4];
            philox4x32_10(l >> 2, key, x);
            const bool hi = (l & 2) != 0;
            double n0, n1;
            noise_box_muller(hi ? x[2] : x[0], hi ? x[3] : x[1], n0, n1);
            w[0] = noise_out<f16>((l & 1) ? n1 : n0, 1.0f);
        } else {
#pragma unroll
            for (int b = 0; b < E / 4; ++b) {                     // l is a multiple of 4: block b serves the elements 4b .. 4b + 3
                uint32_t x[4];
                philox4x32_10((l >> 2) + b, key, x);
                double n[4];
                noise_box_muller(x[0], x[1], n[0], n[1]);
                noise_box_muller(x[2], x[3], n[2], n[3]);
#pragma unroll
                for (int k = 0; k < 4; ++k) w[4 * b + k] = noise_out<f16>(n[k], 1.0f);
            }
        }
    }
};

// The host checks of a stochastic step -> 0 and the policy, else the error: c_n finite, the sample the frames [s, s + L) of a clip
// (1,C,T,h,w) of fewer than 2^63 elements.  seed and stream are 64-bit values passed as size_t.
static inline int philox_noise_of(const char* what, size_t seed, size_t stream, float c_n, int C, int T, int HW, int s, int L,
                                  philox_noise& nz) {
    VDX_CHECK(std::isfinite(c_n), "%s: c_n must be finite", what);
    VDX_CHECK(C > 0 && T > 0 && HW > 0, "%s: bad clip shape C=%d T=%d HW=%d", what, C, T, HW);
    VDX_CHECK(s >= 0 && L >= 1 && s <= T && L <= T - s, "%s: the frames [%d, %d + %d) leave the clip of %d frames", what, s, s, L, T);
    VDX_CHECK((uint64_t)C * (uint64_t)T <= ((((uint64_t)1 << 63) - 1) / (uint64_t)HW),
              "%s: the clip must have fewer than 2^63 elements", what);
    nz.key = {(uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), (uint32_t)stream, (uint32_t)((uint64_t)stream >> 32)};
    nz.c_n = c_n;
    nz.skip = (uint64_t)(T - L) * (uint64_t)HW;
    nz.base = (uint64_t)s * (uint64_t)HW;
    return 0;
}
