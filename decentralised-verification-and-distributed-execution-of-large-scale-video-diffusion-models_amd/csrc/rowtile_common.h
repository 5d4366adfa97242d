// rowtile_common.h — the machinery the fused sub-block kernels share: K7, second design (tattn2.hip), K5 (xattn.hip) and
// K8 with its proj_out tail (ff_fused.hip).  All three are persistent kernels of 4 waves that hold 192 rows (48 per wave,
// private to it) as a LayerNorm-ed fp16 MFMA-operand image in LDS, stream their weights through a ring of 8 KB units
// beside it, and end in the same output projection (three column groups, bias as the initial accumulator, fp16 residual).
// What a kernel does BETWEEN the image and the projection, its step schedule and its wait model are its own.
//
// Everything here is __forceinline__: a kernel that calls it emits the instructions it emitted when the code stood in its
// own file (profiles/rowtile_refactor.md).  Lab / ablation macros are the kernels' business: none is named here, a kernel
// wraps the function it wants to cut out.
#pragma once
#include "vdx_common.h"
#include <utility>

// Explicit address spaces.  LDS addresses as 32-bit arithmetic: a constant term then folds into the DS offset field.
// Explicit global pointers: a pointer the optimiser cannot trace becomes a FLAT access, which counts on both counters and
// completes out of order — the counted waits below need vmcnt alone, in order.
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((address_space(3))) char lchar;
typedef __attribute__((address_space(3))) f16x8 lf16x8;
typedef __attribute__((address_space(3))) f16x4 lf16x4;
typedef __attribute__((address_space(1))) f16 gf16;
typedef __attribute__((address_space(1))) f16x8 gf16x8;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) float gf32;

// workgroup barrier the COMPILER also treats as a memory barrier (LLVM models s_barrier as touching no memory: LDS reads
// of a stage could be scheduled above the barrier that publishes it)
__device__ __forceinline__ void wg_barrier() {
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Stores of rows that do not exist (last tile) go here, and their residual loads come from here, so that every tile
// issues the same instructions and the counted s_waitcnt of the next step stays exact.
static __device__ __attribute__((aligned(16))) u32x4 g_dump_page[64 + 64];     // lane * 16 bytes + up to 2 * INNER bytes of column offset

__device__ __forceinline__ float dpp_add8(float v) {        // sum over the 8 lanes that share a row (lane & ~7)
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    return v;
}
// Value of lanes l, l^16, l^32, l^48 combined (the four lane quads that hold one query's keys): two VALU swaps, no LDS.
// v_permlane16_swap exchanges the odd 16-lane rows of its first operand with the even rows of its second;
// v_permlane32_swap the upper half of the first with the lower half of the second.  Fed the same value twice, the two
// results together hold the value of both partners in every lane.  Inline asm, not the builtins: hipcc (ROCm 7.2) folds
// `r[0] op r[1]` of the builtin to `r[0] op r[0]` (seen in the ISA as v_add_f32 v, a0, a0 — the reduction is then a
// no-op).  The s_nop covers the VALU-write -> permlane-read hazard (2 wait states), which nothing pads inside asm.
__device__ __forceinline__ void swap16(float& a, float& b) { asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void swap32(float& a, float& b) { asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ float quad_max(float v) {
    float a = v, b = v;
    swap16(a, b);
    a = fmaxf(a, b);
    b = a;
    swap32(a, b);
    return fmaxf(a, b);
}
__device__ __forceinline__ float quad_sum(float v) {
    float a = v, b = v;
    swap16(a, b);
    a = a + b;
    b = a;
    swap32(a, b);
    return a + b;
}

template <int INNER>
struct RowTile {
    static constexpr int ROWS = 192;
    static constexpr int RB = INNER * 2;                  // bytes of one row of the image
    static constexpr int XB = ROWS * RB;
    static constexpr int UB = 8192, NU = 5;               // ring: NU units of UB bytes
    static constexpr int LDS_BYTES = XB + NU * UB;
    static constexpr int NPS = 6;                         // P0 passes of 8 rows
    static constexpr int PPP = 8 * RB / 1024;             // DMA pieces per pass
    static constexpr int NCB = INNER / 64;                // column blocks of 64 channels (= PPP: one DMA piece each)
    static constexpr int RBB = NCB * 1024;                // bytes of one row block (8 rows)
    static constexpr int NCGF = INNER / 128;              // full 128-column groups of the output projection
    static constexpr int NCG = (INNER + 127) / 128;
    static_assert(INNER % 128 == 0 || INNER % 128 == 64, "geometry");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
    static_assert(PPP == NCB && XB == 24 * RBB, "a DMA piece is one (row block, column block): 8 rows x 128 bytes");
    static_assert(NCG == 3 && NPS == 6 && NCB == 5, "the row prefetch schedule below is written for three column groups of five steps");

    struct Frag {
        f16x8 w[8], x[3];
    };

    char* smem;
    lchar* lds;                                  // the same, as an LDS pointer
    int lane, n16, q4, wave;
    int woffb, xb[2];                            // LDS byte addresses: weight fragment base, row-image fragment bases (k step parity)

    __device__ __forceinline__ RowTile(char* s) : smem(s), lds((lchar*)s) {}

    // a value the optimiser cannot see through: loads addressed with it are neither hoisted out of the tile loop nor
    // merged — every source-level load below is exactly one instruction per tile (the wait counts rely on it)
    __device__ static __forceinline__ int opaque(int v) {
        asm volatile("" : "+v"(v));
        return v;
    }

    __device__ __forceinline__ void set_lane_constants() {
        n16 = lane & 15;
        q4 = lane >> 4;
        const int g = (0x1320 >> (4 * (n16 >> 2))) & 3;          // g = [0, 2, 3, 1][n >> 2]
        woffb = XB + n16 * 64 + ((q4 ^ g) << 4);
        const int rr = n16 & 7, xrow = (wave * 6 + (n16 >> 3)) * RBB + rr * 128;
        xb[0] = xrow + ((q4 ^ rr) << 4);
        xb[1] = xrow + (((4 + q4) ^ rr) << 4);
    }

    // ---- The weight ring: unit U, at global address `unit`, goes to slot U % NU, two 1 KB pieces per wave.
    template <int U>
    __device__ __forceinline__ void issue_unit(const char* unit) {
        const char* src = unit + (2 * wave) * 1024 + lane * 16;
        char* dst = smem + XB + (U % NU) * UB + (2 * wave) * 1024;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(src + 1024), (lptr_t)(dst + 1024), 16, 0, 0);
    }
    // units U0 .. U1-1.  Where a unit comes FROM is the kernel's business: src(std::integral_constant<int, U>) returns
    // unit U's global address.
    template <int U0, int U1, class Src>
    __device__ __forceinline__ void issue_range(Src src) {
        if constexpr (U0 < U1) {
            issue_unit<U0>(src(std::integral_constant<int, U0>{}));
            issue_range<U0 + 1, U1>(src);
        }
    }
    __device__ __forceinline__ f16x8 wfrag(int unit, int tile) const {
        return *(const lf16x8*)(lds + woffb + ((unit % NU) * UB + tile * 1024));
    }

    // ---- The row image.  LDS layout: [row block of 8 rows][column block of 64 channels][8 rows][128 bytes]; inside the
    // 128 bytes of a row the 16-byte chunk c sits at position c ^ (row & 7).  A (row block, column block) is 1 KB = one
    // LDS-DMA piece whose lane L carries row L >> 3, position L & 7: the per-lane SOURCE address does the row gather (a
    // row's frames may be far apart) and the XOR; the column block is an immediate offset.  For the MFMA fragment reads
    // (16 rows x 16 bytes per lane quad) the XOR makes every ds_read_b128 lane group hit 16 distinct slots of the
    // 256-byte bank row; the in-place normalisation reads and writes whole pieces.
    //
    // Pass PS (8 rows of the wave's 48) -> the wave's part of the image, by LDS-DMA.  This lane carries local row
    // 8*PS + (lane >> 3); the kernel says where that row starts in t and whether it exists (any valid row if not).  Rows that
    // do not exist read the zero page (their values must stay finite: a masked key still multiplies a zero probability).
    // (ff_fused.hip's K8::issue_rows is this function written out, see there: a fix here goes there too.)
    template <int PS>
    __device__ __forceinline__ void issue_rows(const char* row, bool ok) {
        const char* rowp = row + (((lane & 7) ^ (lane >> 3)) << 4);
        const char* zp = (const char*)g_zero_page;
        const char* src = ok ? rowp : zp;
        const int cstep = ok ? 128 : 0;
        char* dst = smem + (wave * 6 + PS) * RBB;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + cb * cstep), (lptr_t)(dst + cb * 1024), 16, 0, 0);
    }
    // P0 of pass PS, in place: centre and scale the 8 rows (8 lanes per row, one chunk of every column block per lane).
    // fp32 statistics: the mean from the row sum, the variance from the squares of (x - mean_h) with mean_h the mean
    // rounded to fp16 (the differences are then exact to fp16 relative precision, whatever the mean) corrected by
    // (mean - mean_h)^2; the result x * rstd - mean * rstd is formed in fp32 and rounded once.  gamma / beta live in
    // the weights.
    template <int PS>
    __device__ __forceinline__ void p0_pass(float eps) {
        lchar* base = lds + (wave * 6 + PS) * RBB + lane * 16;
        f16x8 v[NCB];
#pragma unroll
        for (int j = 0; j < NCB; ++j) v[j] = *(const lf16x8*)(base + 1024 * j);
        const f16x2 ones = (f16x2){(f16)1.f, (f16)1.f};
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NCB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) sum = __builtin_amdgcn_fdot2((f16x2){v[j][2 * e], v[j][2 * e + 1]}, ones, sum, false);
        sum = dpp_add8(sum);
        const float mean = sum * (1.0f / INNER);
        const f16 mh = (f16)mean;
        const float dm = mean - (float)mh;
        const f16x2 nm = (f16x2){(f16)-mh, (f16)-mh};
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NCB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f16x2 d = (f16x2){v[j][2 * e], v[j][2 * e + 1]} + nm;
                ss = __builtin_amdgcn_fdot2(d, d, ss, false);
            }
        ss = dpp_add8(ss);
        const float var = fmaxf(ss * (1.0f / INNER) - dm * dm, 0.f);
        const float rstd = rsqrtf(var + eps);
        const float nmr = -mean * rstd;
#pragma unroll
        for (int j = 0; j < NCB; ++j) {
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (f16)fmaf((float)v[j][e], rstd, nmr);
            *(lf16x8*)(base + 1024 * j) = o;
        }
    }
    // row-image fragment: row 16*i + n16 of the wave's group, chunk 4*ks + q4: row block 2i + (n16 >> 3), column block
    // ks >> 1, position (4*(ks & 1) + q4) ^ (n16 & 7): xb[ks & 1] + a constant
    __device__ __forceinline__ f16x8 xfrag(int i, int ks) const {
        return *(const lf16x8*)(lds + xb[ks & 1] + (2 * i * RBB + 1024 * (ks >> 1)));
    }

    // issue order of a half step (a compile-time directive): one memory instruction after every MFMA until they are
    // used up — NVM vector-memory instructions first, then NDS LDS reads
    template <int NVM, int NDS>
    __device__ static __forceinline__ void pin_after_mfma() {
#pragma unroll
        for (int g = 0; g < NVM; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
#pragma unroll
        for (int g = 0; g < NDS; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
    }

    // ---- The output projection: NCG column groups (128 columns, the last 64) of N K-64 steps each; group c runs in the
    // kernel's steps [C0 + c*N, C0 + (c+1)*N).  The counts below are the vector-memory instructions of step s that a
    // kernel's wait model adds up.  While the projection runs (it reads no row image) the rows of the NEXT tile are
    // fetched and normalised behind its MFMAs.  They are requested right AFTER the first column group's epilogue and
    // have landed before the second one's: an epilogue consumes plain loads, in front of which hipcc waits vmcnt(0) —
    // every DMA in flight at that point, HBM-latency row pieces included, would be waited for.  Passes 0-2 in the second
    // group's first step, passes 3-5 in the step after it.
    static constexpr int nt_of(int c) { return c < NCGF ? 8 : 4; }                                  // 16-column tiles of group c
    static constexpr int op_xp(int s, int c0, int n) { return s == c0 + n || s == c0 + n + 1 ? 3 * PPP : 0; }      // row pieces issued in step s
    // P0 passes normalised in the first half of step s: bit ps of the result.  Each at least two step waits after its
    // pieces were issued (the waits retire every older DMA), none in the last step of the second column group.
    static constexpr int op_p0_mask(int s, int c0, int n) {
        const int r = s - (c0 + n);
        return r == 3 ? 0x03 : r == 5 ? 0x04 : r == 6 ? 0x08 : r == 7 ? 0x10 : r == 8 ? 0x20 : 0;
    }
    static constexpr int op_bias(int s, int c0, int n) {      // bias of column group c: one step before the group starts
        for (int c = 0; c < NCG; ++c) if (s == c0 + c * n - 1) return nt_of(c);
        return 0;
    }
    static constexpr int op_res(int s, int c0, int n) {       // residual rows of column group c: at the top of its second step
        for (int c = 0; c < NCG; ++c) if (s == c0 + c * n + 1) return 3 * nt_of(c) / 2;
        return 0;
    }
    static constexpr int op_st(int s, int c0, int n) {        // stores of the epilogue that ran at the end of step s
        for (int c = 0; c < NCG; ++c) if (s == c0 + c * n + n - 1) return 3 * nt_of(c) / 2;
        return 0;
    }
    template <int MASK, int... PS>
    __device__ __forceinline__ void p0_passes(float eps, std::integer_sequence<int, PS...>) {
        ((MASK >> PS & 1 ? p0_pass<PS>(eps) : void()), ...);
    }
    template <int MASK>
    __device__ __forceinline__ void p0_passes(float eps) { p0_passes<MASK>(eps, std::make_integer_sequence<int, NPS>{}); }
    // weight fragments of half KK (one MFMA k step) of a step of group C whose first unit is u0: a full group has one
    // unit (8 tiles) per half, the last group one unit for both.  wf(unit, tile) reads a fragment: wfrag, or a kernel's
    // wrapper of it
    template <int C, int KK, class W>
    __device__ static __forceinline__ void read_out_half(Frag& f, int u0, W wf) {
        if constexpr (C < NCGF) {
#pragma unroll
            for (int j = 0; j < 8; ++j) f.w[j] = wf(u0 + KK, j);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) f.w[j] = wf(u0, 4 * KK + j);
        }
    }
    template <int C, int KK>
    __device__ __forceinline__ void read_out_half(Frag& f, int u0) const {
        read_out_half<C, KK>(f, u0, [this](int unit, int tile) { return wfrag(unit, tile); });
    }
    // its MFMAs: [column][row] accumulators, b = the B operands of the three row tiles; Z: the group's first half starts
    // from the bias
    template <int C, bool Z>
    __device__ static __forceinline__ void mma_out(f32x4 (&acc)[3][8], const Frag& f, const f16x8& b0, const f16x8& b1, const f16x8& b2,
                                                   const f32x4 (&bv)[8]) {
#pragma unroll
        for (int j = 0; j < nt_of(C); ++j) {
            acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.w[j], b0, Z ? bv[j] : acc[0][j], 0, 0, 0);
            acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.w[j], b1, Z ? bv[j] : acc[1][j], 0, 0, 0);
            acc[2][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.w[j], b2, Z ? bv[j] : acc[2][j], 0, 0, 0);
        }
    }
    // output bias of column group C: the initial accumulator of the projection (tile 2a + jj, register e: column
    // 32a + 8*q4 + 4*jj + e of the group)
    template <int C>
    __device__ __forceinline__ void load_bias(f32x4 (&bv)[8], const float* bias) const {
        const int o = opaque(C * 128 + 8 * q4);
#pragma unroll
        for (int j = 0; j < nt_of(C); ++j) bv[j] = *(const gf32x4*)((const gf32*)bias + o + 32 * (j / 2) + 4 * (j % 2));
    }
    // residual rows of column group C: requested at the top of the group's second K step (HBM latency), consumed after it.
    // rowp: this lane's three rows (+ 8*q4), or the dump page
    template <int C>
    __device__ static __forceinline__ void load_residual(f16x8 (&rv)[3][4], const gf16* const (&rowp)[3]) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const gf16* src = rowp[i] + opaque(0);
#pragma unroll
            for (int a = 0; a < nt_of(C) / 2; ++a) rv[i][a] = *(const gf16x8*)(src + C * 128 + 32 * a);
        }
    }
    // tile pair (2a, 2a+1) gives this lane 8 consecutive columns 32a + 8*q4 .. +7 of row n16 (+16i).  The projection
    // (bias included: it was the initial accumulator) is rounded to fp16 and the residual added in fp16 — the
    // reference's order (to_out returns fp16, `attn_output + hidden_states` is an fp16 add).
    __device__ static __forceinline__ f16x8 round_add_residual(const f32x4& a0, const f32x4& a1, const f16x8& r) {
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = (f16)a0[e];
            o[4 + e] = (f16)a1[e];
        }
        return o + r;
    }
    template <int C>
    __device__ static __forceinline__ void epilogue(const f32x4 (&acc)[3][8], const f16x8 (&rv)[3][4], gf16* const (&outp)[3]) {
#pragma unroll
        for (int a = 0; a < nt_of(C) / 2; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i)
                *(gf16x8*)(outp[i] + C * 128 + 32 * a) = round_add_residual(acc[i][2 * a], acc[i][2 * a + 1], rv[i][a]);
    }
};
