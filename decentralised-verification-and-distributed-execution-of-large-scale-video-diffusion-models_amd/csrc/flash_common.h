// flash_common.h — the parts of the flash attention tile that flash.hip, flash_win.hip and flash_frames.hip share: the softmax
// state (lazy monotone offset, four max / sum chains), the transposed V read and the per-lane-row store.
// profiles/r04_flash.md has the measurements behind each; flash.hip's header comment the layout they assume.
#pragma once
#include "attn_common.h"

typedef const __attribute__((address_space(1))) void* fl_gptr_t;
typedef __attribute__((address_space(3))) void* fl_lptr_t;

// exchange with lane ^ 32 without LDS: v_permlane32_swap of (x, x) leaves the low half's value in a, the high half's in b
__device__ __forceinline__ float max_xor32(float x) {
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}

// The softmax state of a wave's QB sub-blocks and one tile's vector work.
// The offset m is LAZY and MONOTONE.  r_run is the row's running maximum over all tiles so far, measured against the
// offset in use.  The offset stays put (and, while it is 0, its MFMA is skipped) as long as r_run lies in (-4, 10]:
// p = exp2(S') <= 2^10 is exact-enough fp16 with fp32 sums, and a running maximum >= 2^-4 keeps the terms that matter out
// of fp16 subnormals.  When r_run leaves the window the offset is re-centred ON THE RUNNING maximum (rounded to fp16; only
// consistency between p and l matters), never on the current tile's: after the first unmasked tile r_run >= -4 always
// holds, so from then on the offset only RISES (alpha <= 2^-10) and a row moves at most (score range / 10) times.  The one
// downward move possible is the first one (first tile all below -4): nothing has been accumulated yet, so it rescales
// nothing (alpha = 1) — exp2(-d) would overflow there for scores below -128 (0 * inf = NaN).  Tiles far below the running
// maximum simply underflow to p = 0, as they do in an fp32 softmax.
// ABL: flash.hip's timing-only lab builds leave parts of the vector work out (WRONG RESULTS); the product is ABL = 0.
enum { FL_SOFT_NOMAX = 1, FL_SOFT_NOEXP = 2, FL_SOFT_NOSUM = 4 };
template <int QB, int ABL = 0>
struct FlSoft {
    float r_run[QB];              // running row maximum relative to the offset in use
    float l_run[QB][2];           // my half of the row sum, as two partial sums (element pair e of a tile goes to sum e & 1):
                                  // with the QB sub-blocks interleaved that is four independent dot2c chains
    f16x8 negm[QB];               // [-m, 0, ...]: the offset's column of "Q" (m: the offset in use, exp2 units, an fp16 number);
                                  // EVERY lane holds -m in element 0 — the k-step's "K" row e0 is zero for lane half 1, so
                                  // what half 1 of this operand holds does not matter, and m is read back from here
    bool offset_on;               // wave-uniform: some row of this wave has a non-zero offset
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            r_run[qb] = NEG_BIG;
            l_run[qb][0] = l_run[qb][1] = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) negm[qb][j] = (f16)0.0f;
        }
        offset_on = false;
    }
    static __device__ __forceinline__ f16x8 e0(int h) {        // [1, 0, ...]: the offset's row of "K"
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (f16)((j == 0 && h == 0) ? 1.0f : 0.0f);
        return v;
    }
    // s_acc (scores minus the offset in use, masked by the caller) -> pf (fp16 probabilities, the B operand of P.V)
    __device__ __forceinline__ void tile(f32x16 (&s_acc)[QB][2], f32x16 (&o_acc)[QB][2], f16x8 (&pf)[QB][4], int h) {
        bool move[QB], any_move = false;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            if constexpr ((ABL & FL_SOFT_NOMAX) != 0) {
                move[qb] = false;
                continue;
            }
            float mc[4] = {NEG_BIG, NEG_BIG, NEG_BIG, NEG_BIG};      // four independent v_max3 chains
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int j = 0; j < 16; j += 2) mc[(j >> 1) & 3] = fmaxf(fmaxf(mc[(j >> 1) & 3], s_acc[qb][kb][j]), s_acc[qb][kb][j + 1]);
            const float m = fmaxf(fmaxf(mc[0], mc[1]), fmaxf(mc[2], mc[3]));
            r_run[qb] = fmaxf(r_run[qb], max_xor32(m));
            // outside (-4, 10] and not "every tile so far masked" (nothing to centre on): bitwise, no short-circuit branches
            move[qb] = (fabsf(r_run[qb] - 3.0f) > 7.0f) & (r_run[qb] > -1.0e29f);
            any_move |= move[qb];
        }
        if (__builtin_amdgcn_ballot_w64(any_move) != 0) {            // rare
            bool nonzero = false;
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                // the fp16 offset enters the contraction as an MFMA operand: keep it finite (an infinite one
                // times the zero rows of its k-step would poison every score with NaN)
                const float m_old = -(float)negm[qb][0];
                const float tgt = fminf(fmaxf(m_old + (move[qb] ? r_run[qb] : 0.f), -60000.0f), 60000.0f);
                const float m_new = (float)(f16)tgt;
                const float d = m_new - m_old;                       // shift actually applied
                negm[qb][0] = (f16)(-m_new);
                r_run[qb] -= d;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int j = 0; j < 16; ++j) s_acc[qb][kb][j] -= d;
                const float alpha = d > 0.f ? __builtin_amdgcn_exp2f(-d) : 1.0f;   // d < 0: first move, O = l = 0
                l_run[qb][0] *= alpha;
                l_run[qb][1] *= alpha;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    o_acc[qb][0][j] *= alpha;
                    o_acc[qb][1][j] *= alpha;
                }
                nonzero |= m_new != 0.f;
            }
            offset_on = __builtin_amdgcn_ballot_w64(nonzero) != 0;
        }
        // p = exp2(S') packed to fp16 pairs, row sums by dot2
        f16x2 one2;
        one2[0] = one2[1] = (f16)1.0f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int j = 0; j < 16; j += 2)
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) {
                    f16x2 pp;
                    if constexpr ((ABL & FL_SOFT_NOEXP) != 0) {
                        pp[0] = (f16)s_acc[qb][kb][j];
                        pp[1] = (f16)s_acc[qb][kb][j + 1];
                    } else {
                        pp[0] = (f16)__builtin_amdgcn_exp2f(s_acc[qb][kb][j]);
                        pp[1] = (f16)__builtin_amdgcn_exp2f(s_acc[qb][kb][j + 1]);
                    }
                    if constexpr ((ABL & FL_SOFT_NOSUM) == 0)
                        l_run[qb][(j >> 1) & 1] = __builtin_amdgcn_fdot2(pp, one2, l_run[qb][(j >> 1) & 1], false);
                    pf[qb][kb * 2 + (j >> 3)][j & 7] = pp[0];
                    pf[qb][kb * 2 + (j >> 3)][(j & 7) + 1] = pp[1];
                }
    }
    __device__ __forceinline__ float row_sum(int qb) const {
        const float l = l_run[qb][0] + l_run[qb][1];
        return l + __shfl_xor(l, 32, 64);
    }
};

// transposed-read address of a lane inside a V tile (VROW), for d block 0; d block 1 = ^ 64.  Lane 4q+p of a 16-lane group
// supplies row q, d columns 4p..4p+3 of a block of 4 keys x 16 d and receives column (lane & 15) of the 4 rows:
// group (lane >> 4) & 1 takes d 16..31 of the d block, lane half h keys 8h.. of the operand's 16.
__device__ __forceinline__ int fl_tr_addr(int lane) {
    const int h = lane >> 5, tq = (lane >> 2) & 3, tp = lane & 3, tg = (lane >> 4) & 1;
    return (8 * h + tq) * 128 + (((2 * tg + (tp >> 1)) ^ ((tq >> 1) << 2)) << 4) + 8 * (tp & 1);
}
__device__ __forceinline__ f16x8 fl_read_vtr(const char* vb) {      // keys 16kk + 8h + (0..3 | 4..7) of d = 32db + (lane & 31)
    typedef short s16x4v __attribute__((__vector_size__(8)));
    typedef __attribute__((address_space(3))) s16x4v* ltr_t;
    struct TrPair { s16x4v lo, hi; } pr;
    pr.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)vb);
    pr.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)(vb + 512));
    return __builtin_bit_cast(f16x8, pr);
}

// epilogue of the kernels whose query rows are given per lane (flash_win.hip, flash_frames.hip): O[query][d], lane = query;
// pair lanes (l, l^32) to emit 16-byte stores (flash.hip fl_store with the row given per lane); rows with ok false are not stored
template <int QB>
__device__ __forceinline__ void fl_store_rows(const FlSoft<QB>& st, const f32x16 (&o_acc)[QB][2], int h, f16* const (&dst)[QB], const bool (&ok)[QB]) {
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const float inv = 1.0f / st.row_sum(qb);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                // register group g holds d = 32*db + 8*g + 4*h + (0..3)
                f16x4 mine[2];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) mine[u][j] = (f16)(o_acc[qb][db][4 * (g + u) + j] * inv);
                const f16x4 send = h ? mine[0] : mine[1];
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                u32x2 sb = __builtin_bit_cast(u32x2, send), rb;
                rb[0] = __shfl_xor(sb[0], 32, 64);
                rb[1] = __shfl_xor(sb[1], 32, 64);
                const f16x4 recv = __builtin_bit_cast(f16x4, rb);
                f16x8 o;
                const f16x4 lo = h ? recv : mine[0], hi = h ? mine[1] : recv;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o[j] = lo[j];
                    o[4 + j] = hi[j];
                }
                if (ok[qb]) *(f16x8*)(dst[qb] + 32 * db + 8 * (g + h)) = o;
            }
        }
    }
}
