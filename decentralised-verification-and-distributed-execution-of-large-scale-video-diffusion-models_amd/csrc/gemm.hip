// gemm.hip — fp16 GEMM / implicit-GEMM family on the gfx950 matrix cores.
//
//   out[M][N] = epilogue( gather(A)[M][K] . W[N][K]^T )
//
// One kernel template serves every contraction of the 3D-UNet:
//   MODE 0  plain rows (Linear, 1x1 shortcut conv; optional 2-source channel concat)
//   MODE 1  3x3 conv, pad 1 (or (0,1,0,1) at stride 2: Downsample2D(padding=0)), stride 1|2, optional nearest-x2
//           upsample folded into the gather; or its PHASE form (upsample = 3): four 2x2 convs on the source image, one
//           per output parity, K = 4*C instead of 9*C (the Stager's setup below)
//   MODE 2  temporal 3-tap conv (Conv3d (3,1,1)), zero padded at the chunk's first/last frame
// Data layout: activations channels-last rows [pixels][C] so a K-slice of 64 channels of one
// row is one 128-byte line; weights [N][K] with K = tap*C + c.
//
// Tiling: BM x BN x 64 block tile, waves own 64x64 (16 accumulators of v_mfma_f32_16x16x32_f16).
// Staging is LDS-DMA (global_load_lds_dwordx4): every lane supplies its own 16-byte SOURCE
// address — which is what makes the conv gathers, the zero padding (source = a 128-byte zero
// page), the concat and the N/M tails free — while the LDS image stays lane-linear (1 KiB = 8 rows
// of 128 B per wave-instruction).  The XOR swizzle that makes every ds_read_b128 conflict-free is
// therefore applied to the source chunk index and to the read address, never to the destination.
// LDS is double-buffered with ONE barrier per K-tile: tile k+1 streams in while tile k feeds the
// MFMAs.  The MFMA is issued with the weight fragment as the A operand, so a lane ends up holding
// 8 consecutive output channels of one row -> 16-byte epilogue stores.
#include "gemm_common.h"
#include "lab.h"
#include <stdlib.h>
#include <string.h>

#ifdef VDX_STAMPS   // diagnostic build only (make stamps): per-block phase clocks, never in the product library
#define STAMP_MAX 32768
VDX_STAMP_BUFFER_AS(g_stamps, STAMP_MAX * 8, vdx_debug_read_stamps(void* dst, int nblocks), (size_t)nblocks * 64)
#define STAMP(i) st_[i] = __builtin_amdgcn_s_memtime()
#else
#define STAMP(i)
#endif

// ---- staging of one output tile's K tiles (LDS-DMA) -------------------------------------------
// Issue slot `it` (of IT per operand) fills, with its DMA instruction i, 16-byte slot it&7 of physical LDS
// row prow + i*RPP.  Slot s of physical row r must hold data chunk s ^ (r & 7); RPP is a multiple of 8, so
// the chunk is the same for every i.  Rows past M (and weight rows past N) are CLAMPED to the last valid
// row: their products land in accumulators the epilogue never stores.
//
// SPLIT (8-wave blocks): waves 0-3 stage the activation rows, waves 4-7 the weight rows, 256 issue slots
// each.  Waves w and w+4 share a SIMD; a DMA instruction costs its wave ~60-100 issue cycles, and with
// all eight waves issuing their share at the top of a K tile the matrix pipe sat idle for that long in
// every K tile (measured: DMA-only 1.0 us and MFMA-only 1.65 us per K tile, together 2.1 us).  Now the
// activation waves issue at the top while their partners run MFMAs, and the weight waves issue between
// their two K halves while the activation waves run MFMAs.  The weights are L2-resident (0.2-0.4 us to
// land), so half a K tile of lead is enough for them; the activation rows, which may come from HBM, keep
// the full K tile of lead.
template <int BM, int BN, int NT, int MODE, bool SPLIT, bool UPS2 = false>
struct Stager {
    static constexpr int IT = SPLIT ? NT / 2 : NT;        // issue slots per operand
    static constexpr int RPP = IT / 8;                    // LDS rows covered by one DMA instruction of all slots
    static constexpr int ACH = BM / RPP, BCH = BN / RPP;  // DMA instructions per slot and K tile: A rows, W rows
    static constexpr int STAGE = (BM + BN) * 128;
    static_assert(BM % RPP == 0 && BN % RPP == 0 && RPP % 32 == 0, "tile shape");
    static_assert(!SPLIT || NT == 512, "SPLIT pairs wave w with wave w+4");
    int d0[ACH], d1[ACH];   // MODE 0: source row | MODE 1: image base row, (y+1)<<16|(x+1) | MODE 2: row, frame
    int wrow0, csw, iwave;
    int tap, kc, kw;        // the NEXT K tile to be issued (kw = its first weight column)
    int ky, kx, tw;         // MODE 1: its tap as (row, column) of the tw x tw window (tw = p.tapw) — wave-uniform counters
    const f16* wb;          // weight table of this tile (MODE 1 phase form: the tile's phase)

    __device__ __forceinline__ void setup(const GemmP& p, int tid, int m0, int n0) {
        const int it = SPLIT ? (tid & (IT - 1)) : tid;
        const int prow = it >> 3;
        iwave = __builtin_amdgcn_readfirstlane(it >> 6);
        csw = ((it & 7) ^ (prow & 7)) * 8;    // element offset of the data chunk this slot fetches
        // MODE 1 phase form (p.ph_pad > 0): nearest-x2 + conv3x3 = four 2x2 convs on the SOURCE image, one per output
        // parity (a, b).  Rows are virtual and phase-major: v -> phase v / ph_pad, source pixel v % ph_pad (valid below
        // ph_src; clamped for the gather, never stored).  ph_pad is a multiple of 256 and tiles start at multiples of
        // their height, so a tile has ONE phase: its weight table is p.w + phase*N*K, and tap (ty, tx) of output
        // (2i+a, 2j+b) reads source (i + a - 1 + ty, j + b - 1 + tx) — the (y+1, x+1) of d1 moved by (a, b).  The zero
        // padding of the upsampled image is the zero padding of the source image.  (p.h_out, p.w_out are the source's.)
        int ph_a = 0, ph_b = 0, ph_m0 = 0;
        wb = p.w;
        if (MODE == 1 && p.ph_pad) {
            const int phase = m0 / p.ph_pad;
            ph_a = phase >> 1;
            ph_b = phase & 1;
            ph_m0 = phase * p.ph_pad;
            wb = p.w + (size_t)phase * p.N * p.K;
        }
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            int mm = min(m0 + prow + i * RPP, p.M - 1);
            if (MODE == 1 && p.ph_pad) mm = min(mm - ph_m0, p.ph_src - 1);
            if (MODE == 0) {
                d0[i] = mm;
                d1[i] = 0;
            } else if (MODE == 1) {
                const int per = p.h_out * p.w_out;
                const int n = mm / per, rem = mm - n * per;
                const int yo = rem / p.w_out, xo = rem - yo * p.w_out;
                d0[i] = n * p.h_in * p.w_in;
                d1[i] = ((yo * p.stride + p.pad_shift + ph_a) << 16) | (xo * p.stride + p.pad_shift + ph_b);
            } else {
                d0[i] = mm;
                d1[i] = (mm / p.hw) % p.frames;
            }
        }
        // Physical LDS row pr holds weight row 8q+4b+j where pr = 16b+4q+j inside each 32-row group, so
        // that after the MFMA a lane owns 8 consecutive output columns (RPP % 32 == 0: same for every i).
        wrow0 = n0 + ((((prow >> 2) & 3) << 3) | (((prow >> 4) & 1) << 2) | (prow & 3)) + (prow & ~31);
        tap = kc = kw = 0;
        ky = kx = 0;
        tw = p.tapw;
    }
    // weight rows of the next K tile -> stage buffer `buf`
    __device__ __forceinline__ void issue_w(const GemmP& p, char* smem, int buf) {
        char* sb = smem + buf * STAGE + BM * 128 + iwave * 1024;
#pragma unroll
        for (int i = 0; i < BCH; ++i) {
            const int r = min(wrow0 + i * RPP, p.N - 1);
            __builtin_amdgcn_global_load_lds((gptr_t)(wb + (size_t)r * p.K + kw + csw), (lptr_t)(sb + i * RPP * 128), 16, 0, 0);
        }
    }
    // (gathered) activation rows of the next K tile -> stage buffer `buf`
    __device__ __forceinline__ void issue_a(const GemmP& p, char* smem, int buf) {
        const f16* zp = (const f16*)g_zero_page;
        char* sa = smem + buf * STAGE + iwave * 1024;
        if (MODE == 0) {
            const bool first = kc < p.c1;
            const f16* base = first ? p.a + kc + csw : p.a2 + (kc - p.c1) + csw;
            const int ld = first ? p.lda : p.lda2;
#pragma unroll
            for (int i = 0; i < ACH; ++i)
                __builtin_amdgcn_global_load_lds((gptr_t)(base + (size_t)d0[i] * ld), (lptr_t)(sa + i * RPP * 128), 16, 0, 0);
        } else if (MODE == 1) {
            const int hlim = p.h_up, wlim = p.w_up;
#pragma unroll
            for (int i = 0; i < ACH; ++i) {
                int y = (d1[i] >> 16) + ky - 1, x = (d1[i] & 0xffff) + kx - 1;
                const bool ok = (unsigned)y < (unsigned)hlim && (unsigned)x < (unsigned)wlim;
                if (UPS2) {                   // explicit target size (latent not divisible by 8): F.interpolate(size=, "nearest")
                    y = min((int)((float)y * p.usy), p.h_in - 1);
                    x = min((int)((float)x * p.usx), p.w_in - 1);
                } else {                      // (its own instantiation: the float index math costs the issue-bound K loop 11 %)
                    y >>= p.ups;
                    x >>= p.ups;
                }
                const f16* src = p.a + (size_t)(d0[i] + y * p.w_in + x) * p.lda + kc + csw;
                __builtin_amdgcn_global_load_lds((gptr_t)(ok ? src : zp), (lptr_t)(sa + i * RPP * 128), 16, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < ACH; ++i) {
                const int f = d1[i] + tap - 1;
                const bool ok = (unsigned)f < (unsigned)p.frames;
                const f16* src = p.a + (size_t)(d0[i] + (tap - 1) * p.hw) * p.lda + kc + csw;
                __builtin_amdgcn_global_load_lds((gptr_t)(ok ? src : zp), (lptr_t)(sa + i * RPP * 128), 16, 0, 0);
            }
        }
    }
    // start the K walk at K tile kt (split-K slices)
    __device__ __forceinline__ void seek(int kt) {
        kw = kt * 64;
        if (MODE == 0) {
            kc = kw;
        } else {
            constexpr int T = MODE == 1 ? 9 : 3;      // (split-K slices: never the phase form)
            const int slice = kt / T;
            tap = kt - slice * T;
            kc = slice * 64;
            if (MODE == 1) {
                ky = tap / 3;
                kx = tap - ky * 3;
            }
        }
    }
    __device__ __forceinline__ void advance() {
        // K order of the gathers is (64-channel slice, tap, channel): all taps of one channel slice are
        // consumed back to back, so the shifted re-reads of the same source pixels hit the XCD's L2
        // (tap-major order streamed ~0.5 MB per CU between re-uses and thrashed it: 7.5x re-fetch).
        // MODE 1 walks a tw x tw window (3: the nine taps; 2: the phase form's four) with scalar counters: the
        // window is run-time, the lanes never branch on it.
        kw += 64;
        if (MODE == 0) {
            kc += 64;
        } else if (MODE == 1) {
            if (++kx == tw) {
                kx = 0;
                if (++ky == tw) {
                    ky = 0;
                    kc += 64;
                }
            }
        } else if (++tap == 3) {
            tap = 0;
            kc += 64;
        }
    }
};

// VAR: 0 the product kernels | 1 a split-K slice (p.ksplit > 1) | 2 the 3x3 gather with nearest-to-size upsampling.
// (Variants 1 and 2 are their own instantiations so that the kernels of every ordinary step stay exactly the round-2
// code: run-time `ksplit` / `ups == 2` branches in the one template cost the 3x3-conv kernel 11 % — 894 -> 995 us per
// launch in the XL step, profiles/r03_kernel_stats.csv history.)
template <int BM, int BN, int WM, int WN, int MODE, bool GEGLU, bool SPLIT, int VAR>
__global__ __launch_bounds__(WM* WN * 64) void gemm_kernel(const GemmP p) {
    constexpr int NT = WM * WN * 64;
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 16, TN = WTN / 16;
    constexpr bool KS = VAR == 1;
#ifdef VDX_GEMM_PLAIN_LOOP                  // timing build (tools/gemm_abl.sh): the K loop without the rolling fragment prefetch
    constexpr bool defined_gemm_plain_loop = true;
#else
    constexpr bool defined_gemm_plain_loop = false;
#endif
    typedef Stager<BM, BN, NT, MODE, SPLIT, VAR == 2> Stage;
    constexpr int STAGE = Stage::STAGE;
    static_assert(TN % 2 == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
#ifdef VDX_STAMPS
    unsigned long long st_[4];
    const unsigned long long r0_ = __builtin_amdgcn_s_memrealtime();
    STAMP(0);
#endif
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int frow = lane & 15, fq = lane >> 4;
    const int nk = p.K >> 6;
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    // split-K (p.ksplit > 1): block = (tile, slice); the slices of a tile are neighbours, so they share an XCD's L2
    int kt_lo = 0, kt_hi = nk, slab = 0;
    if (KS) {
        slab = bid;
        const int sl = bid % p.ksplit;
        bid /= p.ksplit;
        kt_lo = sl * nk / p.ksplit;
        kt_hi = (sl + 1) * nk / p.ksplit;
    }
    int mt_, nt_;
    gemm_tile_of(bid, p.ntm, p.ntn, mt_, nt_);
    const int m0 = p.m_begin + mt_ * BM, n0 = nt_ * BN;
    const bool does_a = !SPLIT || wave < 4, does_w = !SPLIT || wave >= 4;

    float2* gelu = (float2*)(smem + 2 * STAGE);    // GEGLU: table behind the stage buffers (first barrier publishes it)
    if (GEGLU) gelu_tab_init(gelu, tid, NT);
    Stage sg;
    sg.setup(p, tid, m0, n0);
    if (KS && kt_lo) sg.seek(kt_lo);
    if (does_w) sg.issue_w(p, smem, 0);
    if (does_a) sg.issue_a(p, smem, 0);
    sg.advance();

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();                      // LDS-DMA in flight: the barrier's fence waits vmcnt(0)
    STAMP(1);
    for (int kt = KS ? kt_lo : 0; kt < (KS ? kt_hi : nk); ++kt) {
        const int cur = KS ? (kt - kt_lo) & 1 : kt & 1;
        const bool more = kt + 1 < (KS ? kt_hi : nk);
#if !VDX_ABL_IS(2)   // diagnostic ablation 2: no DMA inside the K loop
        // buffer cur^1 was last read before the previous barrier
#if !VDX_ABL_IS(5)    // ablation 5: no activation DMA in the loop
        if (more && does_a) sg.issue_a(p, smem, cur ^ 1);
#endif
#if !VDX_ABL_IS(6)    // ablation 6: no weight DMA in the loop
        if (more && !SPLIT) sg.issue_w(p, smem, cur ^ 1);
#endif
#endif
        const char* As = smem + cur * STAGE;
        const char* Bs = As + BM * 128;
#if !defined(VDX_STAMPS) || VDX_ABL_IS(7)       // (the stamped builds keep the plain loop below unless ablation 7 asks for this one)
        if constexpr (TM == 4 && TN == 10 && !defined_gemm_plain_loop) {
            // ---- the 64x160 wave tile: ROLLING fragment prefetch.  A K half is two groups of 20 MFMAs (column tiles 0-4, 5-9)
            // walked column-major, so a weight fragment is dead after four MFMAs and the read of the fragment that takes its
            // place — the next group's, the next K half's — is issued right behind them, into the same registers: the LDS
            // latency of all but the K tile's first nine reads (nothing can be read before the barrier) and the four
            // activation fragments of the second K half (SPLIT: the nine of either K half) runs under MFMAs.  hipcc on its own reads a group's fragments,
            // drains the LDS queue, issues the 20 MFMAs, four times per K tile; the order here is pinned by
            // sched_group_barrier.  Same MFMAs on the same accumulators in the same K order: same bits.
            f16x8 af[TM], bf[5];
            const int arow = (wm * WTM + frow) * 128, brow = (wn * WTN + frow) * 128, sw = frow & 7;   // (tile rows are multiples of 16: row & 7 = frow & 7)
            auto rdA = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[i] = *(const f16x8*)(As + arow + i * 2048 + (((ks * 4 + fq) ^ sw) << 4));
            };
            auto rdB = [&](int j, int ks, int g) __attribute__((always_inline)) {
                bf[j] = *(const f16x8*)(Bs + brow + (g * 5 + j) * 2048 + (((ks * 4 + fq) ^ sw) << 4));
            };
            auto mm4 = [&](int j, int g) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    acc[i][g * 5 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][g * 5 + j], 0, 0, 0);
            };
            rdA(0);
#pragma unroll
            for (int j = 0; j < 5; ++j) rdB(j, 0, 0);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                mm4(j, 0);
                rdB(j, 0, 1);
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 9, 0);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            if constexpr (!SPLIT) {
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    mm4(j, 1);
                    rdB(j, 1, 0);
                }
                rdA(1);
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
            } else {
                // (the gathers' weight-staging waves issue their DMA between the K halves: no fragment is carried across —
                // the staging descriptors and 36 live fragment registers do not fit beside the accumulators)
#pragma unroll
                for (int j = 0; j < 5; ++j) mm4(j, 1);
                __builtin_amdgcn_sched_group_barrier(0x008, 20, 0);
                if (more && does_w) sg.issue_w(p, smem, cur ^ 1);
                rdA(1);
#pragma unroll
                for (int j = 0; j < 5; ++j) rdB(j, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 9, 0);
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                mm4(j, 0);
                rdB(j, 1, 1);
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) mm4(j, 1);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 20, 0);
        } else
#endif
#if VDX_ABL_IS(1)         // diagnostic ablation 1: DMA only, no LDS reads / MFMA
        if (false)
#endif
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#if !(VDX_ABL_IS(2) || VDX_ABL_IS(6))
            if (SPLIT && ks == 1 && more && does_w) sg.issue_w(p, smem, cur ^ 1);
#endif
            f16x8 af[TM];
            const int c = ks * 4 + fq;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * WTM + i * 16 + frow;
                af[i] = *(const f16x8*)(As + row * 128 + ((c ^ (row & 7)) << 4));
            }
            // weight fragments in groups of <= 5 (bounds live registers on the 160-wide wave tile)
            constexpr int NG = TN > 5 ? 2 : 1, GS = TN / NG;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                f16x8 bf[GS];
#pragma unroll
                for (int j = 0; j < GS; ++j) {
                    const int row = wn * WTN + (g * GS + j) * 16 + frow;
                    bf[j] = *(const f16x8*)(Bs + row * 128 + ((c ^ (row & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < GS; ++j)
                        acc[i][g * GS + j] =
                            __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][g * GS + j], 0, 0, 0);
            }
        }
        if (more) sg.advance();
        __syncthreads();                  // next K tile landed (vmcnt(0)) and this one is fully read
    }

    STAMP(2);
    if (KS) {
        // this slice's fp32 accumulators -> its slab, in register order ([accumulator][thread][4]: 16-byte coalesced
        // stores); vdx_gemm_reduce_kernel adds the slabs of a tile in slice order and runs the epilogue
        float* dst = p.partial + (size_t)slab * (NT * TM * TN * 4) + tid * 4;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) *(f32x4*)(dst + (i * TN + j) * NT * 4) = acc[i][j];
        return;
    }
    gemm_epilogue<TM, TN, GEGLU, MODE == 1>(p, acc, m0 + wm * WTM, n0 + wn * WTN, frow, fq, gelu);
#ifdef VDX_STAMPS
    __builtin_amdgcn_s_waitcnt(0);        // stores drained
    STAMP(3);
    if (tid == 0 && blockIdx.x < STAMP_MAX) {
        unsigned long long* d = g_stamps + (size_t)blockIdx.x * 8;
        for (int i = 0; i < 4; ++i) d[i] = st_[i];
        d[4] = r0_;
        d[5] = __builtin_amdgcn_s_memrealtime();
        d[6] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
               ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
        d[7] = (unsigned long long)bid;
    }
#endif
}

// ---- host side ------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, int MODE, bool GEGLU, bool SPLIT = false, int VAR = 0>
static int launch(const GemmP& p, const GemmSink& to) {
    if (to.name)
        return snprintf(to.name, GEMM_NAME_MAX, "gemm_kernel<%d, %d, %d, %d, %d, %s, %s, %d>", BM, BN, WM, WN, MODE, tf(GEGLU), tf(SPLIT), VAR), 0;
    constexpr int lds = 2 * (BM + BN) * 128 + (GEGLU ? GELU_TAB_BYTES : 0);
    auto kern = gemm_kernel<BM, BN, WM, WN, MODE, GEGLU, SPLIT, VAR>;
    // one-time LDS opt-in; a function-local static is initialised exactly once even under concurrent callers
    static const hipError_t attr_rc = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr_rc != hipSuccess) return vdx_fail("gemm: cannot reserve %d bytes of LDS", lds);
    GemmP q = p;
    q.ntn = (p.N + BN - 1) / BN;
    const int ntm = (p.M - p.m_begin + BM - 1) / BM;
    q.ntm = ntm;
    hipLaunchKernelGGL(kern, dim3(ntm * q.ntn), dim3(WM * WN * 64), lds, to.st, q);
    return vdx_launch_status("vdx_gemm_f16");
}

// ---- split-K tails -----------------------------------------------------------------------------
// A product whose 256x320 tiles do not fill a whole number of rounds of 256 ends in a mostly idle round.  Its tail
// (fewer than half a round of tiles) can instead be computed as `ksplit` K slices per tile — all CUs busy for 1/ksplit
// of a tile time — followed by this reduction: one wave per (tile, wave of the tile) sums the slices' fp32 slabs in
// slice order (fixed: deterministic) and runs the SAME epilogue code on the sum.  The 16-frame windows of BASELINE
// cfg4 / cfg5 are where it pays (level 2: 288 tiles = 1.125 rounds).  It changes the summation order of those rows
// (K slices accumulated separately, then added), so it is a per-call opt-in (vdx_gemm_args.ksplit).
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64) void gemm_reduce_kernel(const GemmP p) {
    constexpr int NT = WM * WN * 64, WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
    const int lane = threadIdx.x;
    const int wave = blockIdx.x % (WM * WN), tile = blockIdx.x / (WM * WN);
    int mt_, nt_;
    gemm_tile_of(tile, p.ntm, p.ntn, mt_, nt_);
    const int m0 = p.m_begin + mt_ * BM, n0 = nt_ * BN;
    f32x4 acc[TM][TN];
    const float* src = p.partial + (size_t)tile * p.ksplit * (NT * TM * TN * 4) + (wave * 64 + lane) * 4;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = *(const f32x4*)(src + (i * TN + j) * NT * 4);
    for (int sl = 1; sl < p.ksplit; ++sl) {
        const float* s2 = src + (size_t)sl * (NT * TM * TN * 4);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const f32x4 v = *(const f32x4*)(s2 + (i * TN + j) * NT * 4);
                acc[i][j] = acc[i][j] + v;
            }
    }
    gemm_epilogue<TM, TN, false>(p, acc, m0 + (wave / WN) * WTM, n0 + (wave % WN) * WTN, lane & 15, lane >> 4);
}

static constexpr size_t KSPLIT_SLAB_BYTES = 256 * 320 * 4;     // fp32 accumulators of one 256x320 tile

template <int MODE>
static int launch_ksplit(const GemmP& p, const GemmSink& to) {     // (p.ksplit slices per tile, slabs in p.partial: gemm_prepare)
    constexpr int BM = 256, BN = 320, WM = 4, WN = 2, VAR = 1;
    constexpr bool GEGLU = false, SPLIT = MODE != 0;
    if (to.name)
        return snprintf(to.name, GEMM_NAME_MAX, "gemm_kernel<%d, %d, %d, %d, %d, %s, %s, %d> split-K + reduce", BM, BN, WM, WN, MODE, tf(GEGLU), tf(SPLIT), VAR), 0;
    constexpr int lds = 2 * (BM + BN) * 128;
    auto kern = gemm_kernel<BM, BN, WM, WN, MODE, GEGLU, SPLIT, VAR>;
    static const hipError_t attr_rc = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr_rc != hipSuccess) return vdx_fail("gemm: cannot reserve %d bytes of LDS", lds);
    GemmP q = p;
    q.ntn = (p.N + BN - 1) / BN;
    q.ntm = (p.M - p.m_begin + BM - 1) / BM;
    const int tiles = q.ntm * q.ntn;
    hipLaunchKernelGGL(kern, dim3(tiles * q.ksplit), dim3(WM * WN * 64), lds, to.st, q);
    hipLaunchKernelGGL((gemm_reduce_kernel<BM, BN, WM, WN>), dim3(tiles * WM * WN), dim3(64), 0, to.st, q);
    return vdx_launch_status("vdx_gemm_f16 (split-K tail)");
}

// Kernel choice.  `force` (vdx_gemm_args.epilogue bits 8..11, a testing/tuning knob) pins a
// variant: 1 = 128x128 two-stage (eight waves; 9 = four waves), 2 = 256x320 two-stage (K-step 64), 3 = 256x320 four-stage ring
// (K-step 32), 4 = 128x320 two-stage ring with two blocks per CU, 8 = 128x320 four-stage ring with eight
// 32x160 waves, 5 = 256x64, 6 = variant 2 without the
// split staging roles (every wave issues its share of both operands at the top of the K tile); 7 = the
// weights-stationary short-K kernels of gemm_ws.hip.
//
// Channel widths of this UNet are multiples of 320: the 320-wide tiles (64x160 per wave) halve LDS/L2 bytes per MFMA
// against 128x128.  Widths that are not multiples of 320 (transformer_in: 512/1536/4096) still take the 320-wide tile
// when the masked tail wastes < 25 % of the last column of tiles.  Among the candidates a launch costs
// (rounds of 256 tiles) x (time of one tile); tile times relative to the 256x320 tile (= 10), fitted to
// tools/gemm_bench.py at 24 / 16 / 12 frames (profiles/r02_tools.txt): 128x320 as eight 32x160 waves 8 (half the
// work at 62 % of the efficiency), 128x128 3 (a fifth of the work at 67 %).  The 16-frame windows of BASELINE cfg4/5
// are where this matters: M = 18 432 rows at level 2 is 288 tiles of 256x320 = two rounds for 1.125 rounds of work,
// and the 128x128 kernel (5.6 rounds of small tiles) is 10-16 % faster there; level 3 at 16 / 12 frames likewise.
// K-32 rings lose to K-64 on every large shape (profiles/r01_gemm_variants.txt).
struct TileChoice {
    int v;            // variant
    long long cost;   // in tenths of a 256x320 tile time
};
static int nt320_of(int N) { return (N + 319) / 320; }
// N fills 320-wide tiles: the masked tail wastes < 25 % of the last column of tiles
static bool fills320(int N) { return nt320_of(N) * 320 * 4 <= N * 5; }
static bool fits320(long long rows, int N) { return fills320(N) && rows >= 1024; }   // (swapped V^T products have M = C)
// ring_ok = false (the phase-form gather, which only the tiled gemm_kernel families carry): variant 8 is not a candidate
static TileChoice choose_tile(long long rows, int N, bool ring_ok = true) {
    const int nt320 = nt320_of(N);
    const long long t1 = ((rows + 127) / 128) * ((N + 127) / 128);
    const long long c1 = 3 * ((t1 + 255) / 256);
    if (!fits320(rows, N)) return TileChoice{N > 64 ? 1 : 5, c1};
    const long long t256 = ((rows + 255) / 256) * nt320, t128 = ((rows + 127) / 128) * nt320;
    const long long c2 = 10 * ((t256 + 255) / 256), c8 = 8 * ((t128 + 255) / 256);
    if (c2 <= c1 && (c2 <= c8 || !ring_ok)) return TileChoice{2, c2};
    return c8 <= c1 && ring_ok ? TileChoice{8, c8} : TileChoice{1, c1};
}
// Row at which to split a product into [begin, split) on 256x320 tiles (whole rounds of 256) + [split, end) on whatever
// suits the rest, or 0: the last round of a 256x320 launch is otherwise as slow as a full one however few tiles it has.
static int choose_split(int begin, int end, int N, bool ring_ok = true) {
    const long long rows = end - begin;
    const TileChoice whole = choose_tile(rows, N, ring_ok);
    const int nt320 = nt320_of(N);
    // (also when the WHOLE product prefers small tiles — 18 432 rows x 1280: 288 big tiles = two rounds for 1.125 — whole
    // rounds of big tiles + a small-tile tail can still win: one round at 1.2 PFLOP/s + 160 small tiles)
    if (whole.v != 2 && !fits320(rows, N)) return 0;
    const long long t256 = ((rows + 255) / 256) * nt320;
    const long long full = t256 / 256;
    // The main launch is EXACT-FIT: `full` rounds of one tile per CU.  Beside a collective whose channel kernels hold a few CUs
    // (a multi-GPU run) it runs a whole round more: +12...+38 % on the 100 launches of exactly 256 tiles a 16-frame window has
    // (profiles/r06_rccl_contention.md, section 2b).  With a reserve in force (vdx_set_reserved_cus; 0 on one GPU: nothing
    // changes) a round of the main launch fills only the unreserved CUs and the tail takes the rows that are left.  Everything
    // else stays priced on the full chip: pricing ALL rounds on the reserved count changes tile families everywhere (+6.5 %).
    const long long nc = vdx_grid_cus() < 256 ? vdx_grid_cus() : 256;
    if (full == 0 || (t256 % 256 == 0 && nc == 256)) return 0;
    const long long mt_main = full * nc / nt320;                  // m tiles of the main launch (<= `full` rounds)
    if (mt_main == 0) return 0;
    const int split = begin + (int)(mt_main * 256);
    if (split >= end) return 0;
    const TileChoice tail = choose_tile(end - split, N, ring_ok);
    const long long cost = 10 * ((mt_main * nt320 + 255) / 256) + tail.cost + 1;   // + 1: the second launch's ramp
    return cost * 100 <= whole.cost * 94 ? split : 0;      // (measured in the step at 24 / 16 / 12 frames: 94 >= 100 >= 104 > 110)
}

// The ROUTE of a call: everything that selects the template instantiation it runs.  gemm_route decides it once, from the
// prepared arguments; vdx_gemm_f16 launches from it, vdx_gemm_kernel_name names from it, vdx_gemm_plan reports it and
// vdx_gemm_plan_ksplit asks it (gemm_run below: the one switch from a route to its instantiation).
struct GemmRoute {
    int v;          // kernel variant as listed above: 1 2 5 6 9 gemm_kernel, 3 4 8 gemm_ring_kernel, 7 gemm_ws_kernel
    int ws;         // v == 7: the weights-stationary shape family (its residual / weight-set flags come from p.res / p.wset_rows)
    int mode;       // MODE (a GEGLU product is plain)
    bool geglu;     // GEGLU
    int var;        // VAR: 0 | 1 split-K slices + reduction (p.ksplit > 1; v == 2) | 2 the upsample-to-size gather
    bool phase;     // the phase-form gather (upsample = 3): VAR 0 of the tiled gemm_kernel families only (v in 1 2 5 6 9)
    bool forced;    // the caller pinned the variant
    bool whole;     // the call covers the whole product (row_begin / row_end unset or [0, M))
};
// Rows the kernels walk, and the unit of row_begin / row_end.  The phase form (conv3x3, upsample = 3) walks 4 phases of the
// source pixels padded to whole 256-row tiles; everything else walks the M output rows.
static bool gemm_is_phase(const vdx_gemm_args* a) { return a->mode == VDX_GEMM_CONV3X3 && a->upsample == 3; }
static int gemm_rows(const vdx_gemm_args* a) { return gemm_is_phase(a) ? 4 * ((a->M / 4 + 255) / 256 * 256) : a->M; }

static int gemm_route(const vdx_gemm_args* a, const GemmP& p, GemmRoute& r) {
    const int force = (a->epilogue >> 8) & 15;   // kernel variant override (0 = automatic)
    r = GemmRoute{};
    r.geglu = (a->epilogue & VDX_EPI_GEGLU) != 0;
    r.mode = a->mode;
    r.forced = force != 0;
    r.phase = p.ph_pad != 0;
    r.whole = a->row_begin == 0 && (a->row_end == 0 || a->row_end == gemm_rows(a));
    if (r.phase) {
        VDX_CHECK(force == 0 || force == 1 || force == 2 || force == 5 || force == 6 || force == 9,
                  "gemm: the phase-form gather (upsample = 3) runs on the tiled kernels only (variant %d)", force);
        VDX_CHECK(a->ksplit <= 1, "gemm: the phase-form gather (upsample = 3) takes no split-K (ksplit = %d)", a->ksplit);
    }
    r.var = p.ksplit > 1 ? 1 : (a->mode == VDX_GEMM_CONV3X3 && a->upsample == 2) ? 2 : 0;
    // short-K Linear layers on many rows (levels 0/1, transformer_in): weights-stationary streaming kernels
    // (variant 7 pins them); they walk whole products only
    if (r.whole && (force == 7 || (force == 0 && a->M >= 16384))) {
        r.ws = vdx_gemm_ws_family(p, a->mode, r.geglu);
        VDX_CHECK(r.ws || force != 7, "gemm: variant 7 (weights-stationary) needs plain single-source rows, K in {320, 512, 640}, N %% 32 == 0, M %% 64 == 0");
    } else {
        VDX_CHECK(force != 7, "gemm: variant 7 (weights-stationary) computes whole products (row_begin / row_end unset)");
    }
    if (a->wset_rows != 0) {        // a weight set per row range (GroupNorm folded into the Linear): weights-stationary kernels only
        VDX_CHECK(a->wset_rows > 0 && a->wset_bias && a->M % a->wset_rows == 0, "gemm: wset_rows=%d needs wset_bias and M %% wset_rows == 0", a->wset_rows);
        VDX_CHECK(!a->bias && !a->bias2 && !a->residual && !r.geglu && a->mode == VDX_GEMM_PLAIN && a->ksplit <= 1,
                  "gemm: weight sets take no bias / bias2 / residual / GEGLU / split-K (fold them into wset_bias)");
        if (!r.ws && r.whole) r.ws = vdx_gemm_ws_family(p, a->mode, r.geglu);      // (also below the automatic row threshold)
        VDX_CHECK(r.ws == 1 || r.ws == 2 || r.ws == 4, "gemm: weight sets run on the weights-stationary kernels (K = 320 / 640, whole products)");
        VDX_CHECK(a->wset_rows % 64 == 0, "gemm: wset_rows must be a multiple of 64");
    }
    if (r.var == 1) {               // a pinned split-K call: the 256x320 tile, whatever else the shape would take
        VDX_CHECK(!r.geglu && (force == 0 || force == 2), "gemm: split-K runs the 256x320 tile without GEGLU");
        VDX_CHECK(a->ksplit <= 16 && (p.K >> 6) / a->ksplit >= 2, "gemm: ksplit %d leaves fewer than two K tiles per slice (K = %d)", a->ksplit, p.K);
        VDX_CHECK(fills320(p.N), "gemm: split-K needs N = %d to fill 320-wide tiles", p.N);
        // the split-K kernels are VAR = 1: their gather shifts by p.ups (0 | 1) and has no nearest-to-size source map
        VDX_CHECK(a->upsample != 2, "gemm: split-K does not take the upsample-to-size gather (upsample = 2)");
        VDX_CHECK(a->pad_mode == 0, "gemm: split-K does not take the (0,1,0,1) padding (pad_mode = 1)");
        r.ws = 0;
        r.v = 2;
    } else if (r.ws) {
        r.v = 7;
    } else {
        r.v = force ? force : choose_tile(p.M - p.m_begin, p.N, !r.phase).v;
    }
    return 0;
}

template <int MODE, bool GEGLU>
static int pick_tile(const GemmP& p, const GemmRoute& r, const GemmSink& to) {
    if constexpr (MODE == 1 && !GEGLU) {
        if (r.var == 2)     // nearest-to-size gather: two instantiations of its own (latents not divisible by 8 only)
            return r.v == 1 ? launch<128, 128, 2, 2, 1, false, false, 2>(p, to) : launch<256, 320, 4, 2, 1, false, true, 2>(p, to);
    }
    switch (r.v) {
        case 1: return launch<128, 128, 4, 2, MODE, GEGLU>(p, to);     // EIGHT waves of 32x64: two waves per SIMD (3-10 % over four 64x64 waves on the tails, same bits)
        case 2: return launch<256, 320, 4, 2, MODE, GEGLU, MODE != 0>(p, to);   // split roles pay on the gathers only
        case 6: return launch<256, 320, 4, 2, MODE, GEGLU, false>(p, to);
        case 3: return vdx_gemm_ring_launch(p, MODE, GEGLU, 0, to);
        case 4: return vdx_gemm_ring_launch(p, MODE, GEGLU, 1, to);
        case 8: return vdx_gemm_ring_launch(p, MODE, GEGLU, 2, to);
        case 5: return launch<256, 64, 4, 1, MODE, GEGLU>(p, to);
        case 9: return launch<128, 128, 2, 2, MODE, GEGLU>(p, to);     // the four-wave form (64x64 per wave), kept for comparison
    }
    return vdx_fail("gemm: unknown kernel variant %d", r.v);
}
// route -> its instantiation: launched on to.st, or (to.name) only named, by the launch template itself
static int gemm_run(const GemmP& p, const GemmRoute& r, const GemmSink& to) {
    if (r.var == 1) {
        switch (r.mode) {
            case VDX_GEMM_PLAIN: return launch_ksplit<0>(p, to);
            case VDX_GEMM_CONV3X3: return launch_ksplit<1>(p, to);
            default: return launch_ksplit<2>(p, to);
        }
    }
    if (r.v == 7) return vdx_gemm_ws_launch(p, r.ws, r.geglu, to);
    if (r.geglu) return pick_tile<0, true>(p, r, to);
    switch (r.mode) {
        case VDX_GEMM_PLAIN: return pick_tile<0, false>(p, r, to);
        case VDX_GEMM_CONV3X3: return pick_tile<1, false>(p, r, to);
        default: return pick_tile<2, false>(p, r, to);
    }
}

// validation + the kernel-side parameter block + the route, shared by the launch, the name and the plans
static int gemm_prepare(const vdx_gemm_args* a, GemmP& p, GemmRoute& r) {
    VDX_CHECK(a && a->a && a->w && a->out, "gemm: null pointer");
    VDX_CHECK(a->M > 0 && a->N > 0 && a->K > 0, "gemm: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
    const bool phase = gemm_is_phase(a);
    // (the phase form runs on the tiled kernels only, which mask columns in groups of 8)
    VDX_CHECK(a->N % (phase ? 8 : 64) == 0 && a->K % 64 == 0, "gemm: N=%d must be a multiple of %d and K=%d of 64", a->N, phase ? 8 : 64, a->K);
    VDX_CHECK(a->c1 > 0 && a->c1 % 64 == 0 && a->c2 % 64 == 0, "gemm: c1=%d c2=%d must be multiples of 64", a->c1, a->c2);
    VDX_CHECK((a->c2 == 0) == (a->a2 == nullptr), "gemm: a2/c2 mismatch");
    const int taps = phase ? 4 : a->mode == VDX_GEMM_CONV3X3 ? 9 : a->mode == VDX_GEMM_TCONV3 ? 3 : 1;
    VDX_CHECK(a->K == taps * (a->c1 + a->c2), "gemm: K=%d != taps*(c1+c2)=%d", a->K, taps * (a->c1 + a->c2));
    VDX_CHECK(a->lda % 8 == 0 && a->ldo % 8 == 0 && (a->a2 == nullptr || a->lda2 % 8 == 0) &&
                  (a->residual == nullptr || a->ldr % 8 == 0),
              "gemm: leading dimensions must be multiples of 8 elements");
    VDX_CHECK(a->lda >= a->c1, "gemm: lda < c1");
    p.a = (const f16*)a->a; p.a2 = (const f16*)a->a2; p.w = (const f16*)a->w;
    p.bias = (const f16*)a->bias; p.bias2 = (const f16*)a->bias2; p.res = (const f16*)a->residual;
    p.out = (f16*)a->out;
    const int rows = gemm_rows(a);
    VDX_CHECK(a->row_begin >= 0 && (a->row_end == 0 || (a->row_end > a->row_begin && a->row_end <= rows)) && a->row_begin < rows,
              "gemm: rows [%d, %d) of %d", a->row_begin, a->row_end, rows);
    // (kernels mask rows >= p.M: the end of the row range; geometry checks below use the whole product's a->M)
    p.M = a->row_end ? a->row_end : rows; p.m_begin = a->row_begin; p.N = a->N; p.K = a->K; p.c1 = a->c1; p.c2 = a->c2;
    p.lda = a->lda; p.lda2 = a->lda2; p.ldo = a->ldo; p.ldr = a->ldr;
    p.h_in = a->h_in; p.w_in = a->w_in; p.h_out = a->h_out; p.w_out = a->w_out;
    p.stride = a->stride; p.pad_shift = a->pad_mode; p.ups = a->upsample;     // (the gathers shift by ups: 0 | 1; ups == 2 runs the VAR = 2 kernels)
    p.h_up = a->upsample == 1 ? 2 * a->h_in : a->upsample == 2 ? a->h_out : a->h_in;
    p.w_up = a->upsample == 1 ? 2 * a->w_in : a->upsample == 2 ? a->w_out : a->w_in;
    p.tapw = 3; p.ph_src = 0; p.ph_pad = 0;
    if (phase) {        // four 2x2 convs on the source image: no shift, the source's own limits, its own grid of pixels
        p.ups = 0; p.tapw = 2;
        p.h_out = a->h_in; p.w_out = a->w_in;
        p.ph_src = a->M / 4; p.ph_pad = rows / 4;
    }
    p.usy = a->h_in > 0 && p.h_up > 0 ? (float)a->h_in / (float)p.h_up : 1.0f;
    p.usx = a->w_in > 0 && p.w_up > 0 ? (float)a->w_in / (float)p.w_up : 1.0f;
    p.frames = a->frames; p.hw = a->hw; p.rpb2 = a->rows_per_bias2 > 0 ? a->rows_per_bias2 : 1;
    p.ldb2 = a->ldb2 > 0 ? a->ldb2 : a->N;
    VDX_CHECK(p.ldb2 % 8 == 0, "gemm: ldb2 must be a multiple of 8");
    p.ntn = 0; p.ntm = 0;
    p.ksplit = a->ksplit > 1 ? a->ksplit : 0; p.partial = a->ksplit > 1 ? (float*)a->workspace : nullptr;
    p.wset_rows = a->wset_rows; p.wset_bias = a->wset_bias;
    const bool geglu = (a->epilogue & VDX_EPI_GEGLU) != 0;
    if (geglu) {
        VDX_CHECK(a->mode == VDX_GEMM_PLAIN && !a->bias2 && !a->residual, "gemm: GEGLU epilogue is plain-mode only");
        VDX_CHECK(a->ldo % 4 == 0, "gemm: GEGLU ldo must be a multiple of 4");
    }
    switch (a->mode) {
        case VDX_GEMM_PLAIN:
            VDX_CHECK(a->pad_mode == 0, "gemm: pad_mode is a conv3x3 setting");
            break;
        case VDX_GEMM_CONV3X3:
            VDX_CHECK(!geglu, "gemm: GEGLU epilogue is plain-mode only");
            VDX_CHECK(a->c2 == 0, "gemm: conv3x3 takes one source");
            VDX_CHECK(a->stride == 1 || a->stride == 2, "gemm: stride %d", a->stride);
            VDX_CHECK(a->h_in > 0 && a->w_in > 0 && a->h_out > 0 && a->w_out > 0, "gemm: conv geometry");
            VDX_CHECK(a->M % (a->h_out * a->w_out) == 0, "gemm: M=%d not a whole number of %dx%d images", a->M, a->h_out, a->w_out);
            if (phase) {
                VDX_CHECK(a->stride == 1 && a->pad_mode == 0, "gemm: the phase-form gather (upsample = 3) needs stride 1 and pad_mode 0 (stride %d, pad_mode %d)", a->stride, a->pad_mode);
                VDX_CHECK(a->h_out == 2 * a->h_in && a->w_out == 2 * a->w_in, "gemm: the phase-form gather (upsample = 3) is an exact x2: %dx%d -> %dx%d", a->h_in, a->w_in, a->h_out, a->w_out);
                VDX_CHECK(!a->bias2 && !a->residual && !a->a2, "gemm: the phase-form gather (upsample = 3) takes no bias2 / residual / second source");
                VDX_CHECK(a->row_begin % 256 == 0, "gemm: the phase-form gather (upsample = 3) starts at whole 256-row tiles (row_begin %d)", a->row_begin);
                VDX_CHECK(a->wset_rows == 0, "gemm: the phase-form gather (upsample = 3) takes no weight sets");
            } else {
                VDX_CHECK(a->upsample >= 0 && a->upsample <= 2 && (a->upsample == 0 || a->stride == 1), "gemm: upsample %d with stride %d", a->upsample, a->stride);
                VDX_CHECK(a->upsample != 2 || (a->h_out >= a->h_in && a->w_out >= a->w_in), "gemm: upsample-to-size target smaller than the source");
                VDX_CHECK(a->pad_mode == 0 || a->pad_mode == 1, "gemm: pad_mode %d", a->pad_mode);
                VDX_CHECK(a->pad_mode == 0 || (a->stride == 2 && a->upsample == 0),
                          "gemm: pad_mode 1 (pad (0,1,0,1)) needs stride 2 and no upsample (stride %d, upsample %d)", a->stride, a->upsample);
                const int he = p.h_up, we = p.w_up;
                if (a->pad_mode == 1)       // F.pad(x, (0,1,0,1)) + conv3x3 stride 2: (h + 1 - 3) / 2 + 1 = h / 2
                    VDX_CHECK(a->h_out == he / 2 && a->w_out == we / 2 && a->h_out > 0 && a->w_out > 0,
                              "gemm: conv output %dx%d inconsistent with input %dx%d, pad (0,1,0,1) stride 2", a->h_out, a->w_out, he, we);
                else
                    VDX_CHECK(a->h_out == (he + 2 - 3) / a->stride + 1 && a->w_out == (we + 2 - 3) / a->stride + 1,
                              "gemm: conv output %dx%d inconsistent with input %dx%d stride %d", a->h_out, a->w_out, he, we, a->stride);
            }
            break;
        case VDX_GEMM_TCONV3:
            VDX_CHECK(a->pad_mode == 0, "gemm: pad_mode is a conv3x3 setting");
            VDX_CHECK(!geglu, "gemm: GEGLU epilogue is plain-mode only");
            VDX_CHECK(a->c2 == 0, "gemm: tconv3 takes one source");
            VDX_CHECK(a->frames > 0 && a->hw > 0 && a->M % (a->frames * a->hw) == 0, "gemm: tconv geometry M=%d F=%d HW=%d", a->M, a->frames, a->hw);
            break;
        default:
            return vdx_fail("gemm: unknown mode %d", a->mode);
    }
    return gemm_route(a, p, r);
}

extern "C" int vdx_gemm_f16(const vdx_gemm_args* a, vdx_stream_t stream) {
    GemmP p;
    GemmRoute r;
    if (const int rc = gemm_prepare(a, p, r)) return rc;
    if (r.var == 1) {
        const long long tiles = (long long)((p.M - p.m_begin + 255) / 256) * nt320_of(p.N);
        VDX_CHECK(a->workspace && (uintptr_t)a->workspace % 16 == 0, "gemm: split-K needs a 16-byte aligned workspace");
        VDX_CHECK(tiles * a->ksplit <= (1 << 20), "gemm: split-K grid too large");
        VDX_CHECK(a->workspace_bytes >= (size_t)tiles * a->ksplit * KSPLIT_SLAB_BYTES,
                  "gemm: split-K workspace of %zu bytes is smaller than %lld tiles x %d slices x %d bytes", a->workspace_bytes, tiles,
                  a->ksplit, (int)KSPLIT_SLAB_BYTES);
    }
    return gemm_run(p, r, GemmSink{(hipStream_t)stream, nullptr});
}

// Host-only, no GPU needed.  Runs ALL of vdx_gemm_f16's validation of shape, flags and geometry (gemm_prepare: a call it
// refuses has no name) except the split-K workspace's alignment and size, which select nothing; pointers are only tested
// for null.
extern "C" int vdx_gemm_kernel_name(const vdx_gemm_args* a, char* buf, size_t n) {
    VDX_CHECK(buf, "gemm_kernel_name: null buffer");
    GemmP p;
    GemmRoute r;
    if (const int rc = gemm_prepare(a, p, r)) return rc;
    char name[GEMM_NAME_MAX];
    if (const int rc = gemm_run(p, r, GemmSink{nullptr, name})) return rc;
    VDX_CHECK(strlen(name) < n, "gemm_kernel_name: \"%s\" does not fit a buffer of %zu bytes", name, n);
    memcpy(buf, name, strlen(name) + 1);
    return 0;
}

extern "C" int vdx_gemm_plan(const vdx_gemm_args* a, int32_t* variant, int32_t* split_row) {
    VDX_CHECK(variant && split_row, "gemm_plan: null pointer");
    GemmP p;
    GemmRoute r;
    if (const int rc = gemm_prepare(a, p, r)) return rc;
    *variant = r.v;
    *split_row = r.forced || r.v == 7 || r.var == 1 ? 0 : choose_split(p.m_begin, p.M, p.N, !r.phase);
    return 0;
}

// Split-K plan for a whole product (row_begin = row_end = 0): *split_row / *ksplit / *workspace_bytes such that rows
// [0, split_row) as one ordinary call and rows [split_row, M) as one call with vdx_gemm_args.ksplit = *ksplit (and a
// workspace of that many bytes) are expected to be faster than vdx_gemm_plan's best; *ksplit = 0: no.
extern "C" int vdx_gemm_plan_ksplit(const vdx_gemm_args* a, int32_t* split_row, int32_t* ksplit, size_t* workspace_bytes) {
    VDX_CHECK(split_row && ksplit && workspace_bytes, "gemm_plan_ksplit: null pointer");
    GemmP p;
    GemmRoute r;
    if (const int rc = gemm_prepare(a, p, r)) return rc;
    *split_row = 0; *ksplit = 0; *workspace_bytes = 0;
    if (r.v == 7 || r.geglu || r.forced || !r.whole) return 0;
    if (a->pad_mode != 0) return 0;     // gemm_route refuses split-K with pad_mode = 1
    if (a->upsample >= 2) return 0;     // no split-K instantiation carries the nearest-to-size gather or the phase form (gemm_route refuses them)
    const long long rows = p.M;
    const int nt320 = nt320_of(p.N), nk = p.K >> 6;
    if (!fits320(rows, p.N)) return 0;
    const long long t256 = ((rows + 255) / 256) * nt320, full = t256 / 256;
    if (full == 0 || t256 % 256 == 0) return 0;
    const long long mt_main = full * 256 / nt320;                      // (on all 256 CUs: unlike choose_split, a reserve — vdx_grid_cus() — does not shrink this main launch)
    const long long split = mt_main * 256;
    if (split >= rows) return 0;
    const long long t = ((rows - split + 255) / 256) * nt320;          // tiles of the tail
    int S = (int)(128 / t);            // (t * S <= 128 slabs of 327 680 bytes: the workspace stays <= 42 MB)
    if (S > 8) S = 8;
    if (S > nk / 4) S = nk / 4;
    if (S < 2) return 0;
    // costs in HUNDREDTHS of a 256x320 tile time (choose_tile counts tenths).  Slab traffic + reduction + its launch:
    // ~ 25 us at 128 slabs (measured: 2048 x 1280 x 11520 as 32 tiles x 8 slices 90 us for 54 us of slices), against a
    // tile time of 0.0375 us per unit of K (fitted at 1.1 PFLOP/s); a second launch ~ a tenth of a tile.
    const long long main_c = 100 * ((mt_main * nt320 + 255) / 256);
    const long long cost = main_c + (100 + S - 1) / S + (5 + 20 * t * S / 128) * 100 * 1000 / (37 * p.K) + 10;
    // what vdx_gemm_plan would do: the whole product on its best tile, or whole rounds + a tail on small tiles
    long long best = 10 * choose_tile(rows, p.N).cost;
    const long long two = main_c + 10 * choose_tile(rows - split, p.N).cost + 10;
    if (two < best) best = two;
    if (cost * 100 > best * 97) return 0;
    *split_row = (int32_t)split;
    *ksplit = S;
    *workspace_bytes = (size_t)t * S * KSPLIT_SLAB_BYTES;
    return 0;
}

// Lab variants of this translation unit are compiled in only under the switches that lab.h lists for it.
extern "C" int vdx_lab_gemm(void) { return VDX_LAB_GEMM; }
