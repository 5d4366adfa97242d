// tome.hip — Token Merging for Stable Diffusion (Bolya & Hoffman, CVPRW 2023; the tomesd package's
// bipartite_soft_matching_random2d, unpinned) on the UNet's rows [n_img][S][C] fp16 (no reference counterpart;
// UNet3DConditionModel.enable_tome, the job's --tome, vdx/tome.py).  tests/tome_ref.py states the definition; include/vdx.h
// "Token merging" has the contract.  Four steps, each one launch (the match has a small pre-pass):
//
//   match    score[i][j] = <t[src i], t[dst j]> inv[src i] inv[dst j] on MFMA, reduced to (max, argmax) per source in registers:
//            the n_src x n_dst score matrix (1.5 GB per call at 48 images of 72 x 128) never reaches memory.
//   select   the r sources with the largest maxima (ties: lower i; NaN last), the merged layout's row of every token and the
//            CSR list of every destination's merged sources.
//   merge    the merged rows of a tensor: unmerged sources copied, destinations averaged with their sources.
//   unmerge  every token reads its merged row back and adds the residual.
//
// The match kernel.  A workgroup of four waves owns 128 sources of one image; wave w owns rows 32 w .. 32 w + 31 and keeps
// their A fragments of v_mfma_f32_32x32x16_f16 in registers for the whole kernel (lane l: row l & 31, channels 16 ks + 8 (l >> 5)
// .. + 7 of k-step ks, gathered through src_idx: C / 4 VGPRs, 80 at C = 320).  The destinations stream through LDS in tiles
// of 32 NT rows gathered through dst_idx, B fragments read with the same (row, channel) map, so the two operands agree on
// the order of k whatever the hardware's order inside a step is.  LDS rows are C + 8 halves: the row stride is an odd number of
// 16-byte units and the ds_read_b128 of 16 consecutive rows falls on 16 different bank groups.  The accumulator has the
// destination on the lane (column l & 31) and 16 sources in the registers (row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)): each lane
// keeps a running (max, idx) per register, compared with `>` while its j ascend, so the lowest j of equal scores stays; the 32
// lanes of a half combine at the end with (greater, or equal and lower j).  A NaN score compares false and never wins; the
// index starts at 0 and is only assigned a j < n_dst.  Two instantiations: C <= 320 (20 k-steps, tiles of 64 destinations, two
// workgroups per CU) and C <= 1280 (80 k-steps, tiles of 32).
// No atomics on floats anywhere; every result is a function of its own image alone, in one fixed order.  Every index read
// from memory is clamped to its range as an integer before it addresses anything.
#include "vdx_common.h"

#define TM_THREADS 256
#define TM_BM 128                                     // sources of a match workgroup: 32 per wave
#define TS_THREADS 1024                               // the select workgroup: one per image
#define TS_WAVES (TS_THREADS / 64)
#define TM_LDS_MAX (160 * 1024)

__device__ __forceinline__ int tm_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// inv[row] = 1 / sqrt(sum_c fp32(t[row][c])^2): one wave per row, lane l sums the channels 8 l + 512 n .. + 7 in ascending
// order, then the butterfly.  A zero row gives infinity, taken as it comes.
__global__ __launch_bounds__(TM_THREADS) void tm_inv_norm_kernel(const f16* t, size_t ld, int C, size_t rows, float* inv) {
    const size_t row = (size_t)blockIdx.x * (TM_THREADS / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.0f;
    for (int c = lane * 8; c < C; c += 512) {
        const f16x8 v = *(const f16x8*)(t + row * ld + c);
#pragma unroll
        for (int k = 0; k < 8; ++k) s = fmaf((float)v[k], (float)v[k], s);
    }
    s = wave_sum(s);
    if (lane == 0) inv[row] = 1.0f / sqrtf(s);
}

template <int KS, int NT>
__global__ __launch_bounds__(TM_THREADS) void tm_match_kernel(const f16* t, size_t ld, const int* src_idx, const int* dst_idx,
                                                              const float* inv, int S, int n_src, int n_dst, int C, int tiles_per_img,
                                                              float* node_max, int* node_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tm_smem[];
    constexpr int BN = 32 * NT;
    const int ldl = C + 8;
    f16* const dl = (f16*)tm_smem;                                // [BN][ldl]
    float* const dinv = (float*)(tm_smem + (size_t)BN * ldl * 2); // [BN]
    const int img = blockIdx.x / tiles_per_img, tile = blockIdx.x - img * tiles_per_img;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const size_t row0 = (size_t)img * S;
    const int ks_n = C / 16, chunks = C / 8;
    const int i0 = tile * TM_BM + wave * 32;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    f16x8 a[KS];
    {
        const bool ok = i0 + r < n_src;
        const int p = tm_clamp(ok ? src_idx[i0 + r] : 0, 0, S - 1);
        const f16* const ap = t + (row0 + p) * ld + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = (ok && ks < ks_n) ? *(const f16x8*)(ap + 16 * ks) : zero;
    }
    float invs[16], best[16];
    int bidx[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = i0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        invs[reg] = i < n_src ? inv[row0 + tm_clamp(src_idx[i], 0, S - 1)] : 0.0f;
        best[reg] = -INFINITY;
        bidx[reg] = 0;
    }
    for (int j0 = 0; j0 < n_dst; j0 += BN) {
        __syncthreads();                                          // the previous tile has been read
        for (int e = threadIdx.x; e < BN * chunks; e += TM_THREADS) {
            const int rr = e / chunks, ch = e - rr * chunks;
            f16x8 v = zero;
            if (j0 + rr < n_dst) v = *(const f16x8*)(t + (row0 + tm_clamp(dst_idx[j0 + rr], 0, S - 1)) * ld + ch * 8);
            *(f16x8*)(dl + rr * ldl + ch * 8) = v;
        }
        if (threadIdx.x < BN) {
            const int j = j0 + threadIdx.x;
            dinv[threadIdx.x] = j < n_dst ? inv[row0 + tm_clamp(dst_idx[j], 0, S - 1)] : 0.0f;
        }
        __syncthreads();
        f32x16 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) acc[nt][reg] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks < ks_n) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const f16x8 b = *(const f16x8*)(dl + (nt * 32 + r) * ldl + 16 * ks + 8 * h);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks], b, acc[nt], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int j = j0 + nt * 32 + r;
            if (j < n_dst) {
                const float d = dinv[nt * 32 + r];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float s = acc[nt][reg] * invs[reg] * d;
                    if (s > best[reg]) best[reg] = s, bidx[reg] = j;
                }
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        float v = best[reg];
        int ix = bidx[reg];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(ix, o, 64);
            if (ov > v || (ov == v && oi < ix)) v = ov, ix = oi;
        }
        const int i = i0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (r == 0 && i < n_src) {
            node_max[(size_t)img * n_src + i] = v;
            node_idx[(size_t)img * n_src + i] = ix;
        }
    }
}

// ---- select --------------------------------------------------------------------------------
// fp32 -> a uint32 whose unsigned order is the value's: NaN lowest (0), then -inf .. +inf; -0 and +0 share a key.
__device__ __forceinline__ unsigned tm_orderable(float v) {
    unsigned b = __float_as_uint(v);
    if (v != v) return 0u;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// bitonic sort of K[0, n) (n a power of two) in LDS by the whole workgroup; DESC: largest first.  Every pass ends with a
// barrier; n = 1 has no pass and no barrier: the caller has one before the call and needs none after (nothing moved).
template <bool DESC>
__device__ __forceinline__ void tm_bitonic(unsigned long long* K, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = threadIdx.x; e < n; e += TS_THREADS) {
                const int l = e ^ j;
                if (l > e) {
                    const bool up = ((e & k) == 0) != DESC;
                    const unsigned long long x = K[e], y = K[l];
                    if ((x > y) == up) K[e] = y, K[l] = x;
                }
            }
            __syncthreads();
        }
    }
}

// exclusive prefix of v over the workgroup's threads (in thread order) and the total
__device__ __forceinline__ int tm_block_scan(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(incl, o, 64);
        if (lane >= o) incl += n;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) {
        const int s = wsum[w];
        base += w < wave ? s : 0;
        tot += s;
    }
    total = tot;
    return base + incl - v;
}

// One workgroup per image.  LDS: K[n2] 64-bit keys (n2 = n_src rounded up to a power of two), cnt[n_dst], flag[n_src].
// 1. keys (orderable(node_max) << 32 | ~i) sorted largest first: the first r are the merged sources (flag).
// 2. a scan over i of the unmerged flags gives every unmerged source its row; a merged one reads its destination's.
// 3. the merged sources' keys (j << 32 | i) sorted ascending are the CSR items; the counts (integer LDS atomics: the sum
//    does not depend on their order) scanned over j are the offsets.
__global__ __launch_bounds__(TS_THREADS) void tm_select_kernel(const float* node_max, const int* node_idx, const int* src_idx,
                                                               const int* dst_idx, int S, int n_src, int n_dst, int r, int n2, int* slot,
                                                               int* off, int* items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tm_smem[];
    __shared__ int wsum[TS_WAVES];
    unsigned long long* const K = (unsigned long long*)tm_smem;
    int* const cnt = (int*)(tm_smem + (size_t)n2 * 8);
    unsigned char* const flag = (unsigned char*)(cnt + n_dst);
    const int img = blockIdx.x, tid = threadIdx.x;
    node_max += (size_t)img * n_src, node_idx += (size_t)img * n_src;
    slot += (size_t)img * S, off += (size_t)img * (n_dst + 1), items += (size_t)img * r;
    const int n_unm = n_src - r;

    for (int i = tid; i < n2; i += TS_THREADS)
        K[i] = i < n_src ? ((unsigned long long)tm_orderable(node_max[i]) << 32) | (unsigned)(0xffffffffu - (unsigned)i) : 0ull;
    for (int i = tid; i < n_src; i += TS_THREADS) flag[i] = 0;
    for (int j = tid; j < n_dst; j += TS_THREADS) cnt[j] = 0;
    __syncthreads();
    tm_bitonic<true>(K, n2);
    for (int k = tid; k < r; k += TS_THREADS) flag[0xffffffffu - (unsigned)K[k]] = 1;
    __syncthreads();
    // the merged keys overwrite K: every thread is past its reads of K
    const int L = (n_src + TS_THREADS - 1) / TS_THREADS;
    const int ib = tid * L < n_src ? tid * L : n_src, ie = ib + L < n_src ? ib + L : n_src;
    int mine = 0, total;
    for (int i = ib; i < ie; ++i) mine += flag[i] ? 0 : 1;
    int pos = tm_block_scan(mine, wsum, total);
    int n2m = 1;
    while (n2m < r) n2m <<= 1;
    for (int i = ib; i < ie; ++i) {
        const int p = tm_clamp(src_idx[i], 0, S - 1);
        if (flag[i]) {
            const int j = tm_clamp(node_idx[i], 0, n_dst - 1);
            slot[p] = n_unm + j;
            K[i - pos] = ((unsigned long long)(unsigned)j << 32) | (unsigned)i;       // i - pos merged sources lie before i
            atomicAdd(&cnt[j], 1);
        } else {
            slot[p] = pos++;
        }
    }
    for (int k = r + tid; k < n2m; k += TS_THREADS) K[k] = ~0ull;
    for (int j = tid; j < n_dst; j += TS_THREADS) slot[tm_clamp(dst_idx[j], 0, S - 1)] = n_unm + j;
    __syncthreads();
    tm_bitonic<false>(K, n2m);
    for (int k = tid; k < r; k += TS_THREADS) items[k] = (int)(unsigned)K[k];
    const int Ld = (n_dst + TS_THREADS - 1) / TS_THREADS;
    const int jb = tid * Ld < n_dst ? tid * Ld : n_dst, je = jb + Ld < n_dst ? jb + Ld : n_dst;
    mine = 0;
    for (int j = jb; j < je; ++j) mine += cnt[j];
    pos = tm_block_scan(mine, wsum, total);
    for (int j = jb; j < je; ++j) off[j] = pos, pos += cnt[j];
    if (tid == 0) off[n_dst] = r;
}

// ---- merge / unmerge -----------------------------------------------------------------------
// One wave per source or destination of an image; lanes along the channels, 16 bytes each.
__global__ __launch_bounds__(TM_THREADS) void tm_merge_kernel(const f16* y, size_t ldy, const int* src_idx, const int* dst_idx,
                                                              const int* slot, const int* off, const int* items, int S, int n_src, int n_dst,
                                                              int r, int C, size_t work, f16* out, size_t ldo) {
    const size_t w = (size_t)blockIdx.x * (TM_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= work) return;
    const int lane = threadIdx.x & 63;
    const int per = n_src + n_dst, n_unm = n_src - r;
    const size_t img = w / per;
    const int k = (int)(w - img * per);
    const f16* const yi = y + img * S * ldy;
    f16* const oi = out + img * (size_t)(n_unm + n_dst) * ldo;
    if (k < n_src) {
        const int p = tm_clamp(src_idx[k], 0, S - 1), q = slot[img * S + p];
        if (q < 0 || q >= n_unm) return;                          // merged: it lives in its destination's row
        for (int c = lane * 8; c < C; c += 512) *(f16x8*)(oi + (size_t)q * ldo + c) = *(const f16x8*)(yi + (size_t)p * ldy + c);
        return;
    }
    const int j = k - n_src;
    const int p = tm_clamp(dst_idx[j], 0, S - 1);
    const int* const offi = off + img * (n_dst + 1);
    const int b = tm_clamp(offi[j], 0, r), e = tm_clamp(offi[j + 1], b, r);
    const float div = (float)(1 + (e - b));
    for (int c = lane * 8; c < C; c += 512) {
        const f16x8 v = *(const f16x8*)(yi + (size_t)p * ldy + c);
        float acc[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[x] = (float)v[x];
        for (int m = b; m < e; ++m) {
            const int i = tm_clamp(items[img * r + m], 0, n_src - 1);
            const f16x8 s = *(const f16x8*)(yi + (size_t)tm_clamp(src_idx[i], 0, S - 1) * ldy + c);
#pragma unroll
            for (int x = 0; x < 8; ++x) acc[x] += (float)s[x];
        }
        f16x8 o;
#pragma unroll
        for (int x = 0; x < 8; ++x) o[x] = (f16)(acc[x] / div);
        *(f16x8*)(oi + (size_t)(n_unm + j) * ldo + c) = o;
    }
}

__global__ __launch_bounds__(TM_THREADS) void tm_unmerge_add_kernel(const f16* x, size_t ldx, const int* slot, const f16* t, size_t ldt,
                                                                    int S, int Sm, int chunks, size_t n, f16* out, size_t ldo) {
    for (size_t e = (size_t)blockIdx.x * TM_THREADS + threadIdx.x; e < n; e += (size_t)gridDim.x * TM_THREADS) {
        const size_t row = e / chunks;
        const int c = (int)(e - row * chunks) * 8;
        const size_t img = row / S;
        const int q = tm_clamp(slot[row], 0, Sm - 1);
        const f16x8 a = *(const f16x8*)(x + (img * Sm + q) * ldx + c), b = *(const f16x8*)(t + row * ldt + c);
        f16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (f16)((float)a[k] + (float)b[k]);
        *(f16x8*)(out + row * ldo + c) = o;
    }
}

// ---- entry points ----------------------------------------------------------------------------
static int tm_check_plan(const vdx_tome_args* a, const char* what) {
    VDX_CHECK(a, "%s: null argument struct", what);
    VDX_CHECK(a->n_img >= 1 && a->S >= 1 && a->n_src >= 1 && a->n_dst >= 1, "%s: n_img=%d S=%d n_src=%d n_dst=%d (each at least 1)", what,
              a->n_img, a->S, a->n_src, a->n_dst);
    VDX_CHECK((long long)a->n_src + a->n_dst == a->S, "%s: n_src=%d + n_dst=%d != S=%d", what, a->n_src, a->n_dst, a->S);
    VDX_CHECK(a->r >= 1 && a->r <= a->n_src, "%s: r=%d outside [1, n_src=%d]", what, a->r, a->n_src);
    VDX_CHECK((long long)a->n_img * a->S <= 0x7fffffffll / 4, "%s: %d images of %d tokens", what, a->n_img, a->S);
    VDX_CHECK(a->src_idx && a->dst_idx, "%s: null table", what);
    return 0;
}
static int tm_check_rows(const void* p, int ld, int C, const char* what, const char* name) {
    VDX_CHECK(p, "%s: %s is null", what, name);
    VDX_CHECK((size_t)p % 16 == 0 && ld % 8 == 0 && ld >= C, "%s: %s needs a 16-byte aligned pointer and a row stride %d >= C=%d that is a multiple of 8",
              what, name, ld, C);
    return 0;
}
#define TM_TRY(x)             \
    do {                      \
        if ((x) != 0) return -1; \
    } while (0)

extern "C" int vdx_tome_match_f16(const vdx_tome_args* a, const void* t, int ld, vdx_stream_t stream) {
    TM_TRY(tm_check_plan(a, "tome_match"));
    const int C = a->C;
    VDX_CHECK(C >= 64 && C % 64 == 0 && C <= 1280, "tome_match: C=%d (a multiple of 64 up to 1280)", C);
    TM_TRY(tm_check_rows(t, ld, C, "tome_match", "t"));
    VDX_CHECK(a->inv && a->node_max && a->node_idx, "tome_match: null inv / node_max / node_idx");
    const size_t rows = (size_t)a->n_img * a->S;
    hipLaunchKernelGGL(tm_inv_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(TM_THREADS), 0, (hipStream_t)stream, (const f16*)t,
                       (size_t)ld, C, rows, a->inv);
    const int tiles = (a->n_src + TM_BM - 1) / TM_BM;
    VDX_CHECK((long long)a->n_img * tiles <= 0x7fffffffll, "tome_match: %d images x %d tiles", a->n_img, tiles);
    const bool small = C <= 320;
    const int bn = small ? 64 : 32;
    const int lds = bn * (C + 8) * 2 + bn * 4;
    static const hipError_t reserved = vdx_reserve_lds(32 * (1280 + 8) * 2 + 32 * 4, tm_match_kernel<20, 2>, tm_match_kernel<80, 1>);
    VDX_CHECK(reserved == hipSuccess, "tome_match: cannot reserve LDS: %s", hipGetErrorString(reserved));
    if (small)
        hipLaunchKernelGGL((tm_match_kernel<20, 2>), dim3(a->n_img * tiles), dim3(TM_THREADS), lds, (hipStream_t)stream, (const f16*)t,
                           (size_t)ld, a->src_idx, a->dst_idx, a->inv, a->S, a->n_src, a->n_dst, C, tiles, a->node_max, a->node_idx);
    else
        hipLaunchKernelGGL((tm_match_kernel<80, 1>), dim3(a->n_img * tiles), dim3(TM_THREADS), lds, (hipStream_t)stream, (const f16*)t,
                           (size_t)ld, a->src_idx, a->dst_idx, a->inv, a->S, a->n_src, a->n_dst, C, tiles, a->node_max, a->node_idx);
    return vdx_launch_status("vdx_tome_match_f16");
}

extern "C" size_t vdx_tome_select_lds(int n_src, int n_dst) {
    if (n_src < 1 || n_dst < 1) return 0;
    size_t n2 = 1;
    while (n2 < (size_t)n_src) n2 <<= 1;
    return n2 * 8 + (size_t)n_dst * 4 + (((size_t)n_src + 15) & ~(size_t)15);
}

extern "C" int vdx_tome_select(const vdx_tome_args* a, vdx_stream_t stream) {
    TM_TRY(tm_check_plan(a, "tome_select"));
    VDX_CHECK(a->node_max && a->node_idx && a->slot && a->off && a->items, "tome_select: null node_max / node_idx / slot / off / items");
    const size_t lds = vdx_tome_select_lds(a->n_src, a->n_dst);
    VDX_CHECK(lds <= TM_LDS_MAX - 256, "tome_select: %d sources and %d destinations need %zu bytes of LDS (at most %d)", a->n_src, a->n_dst,
              lds, TM_LDS_MAX - 256);
    int n2 = 1;
    while (n2 < a->n_src) n2 <<= 1;
    static const hipError_t reserved = vdx_reserve_lds(TM_LDS_MAX - 256, tm_select_kernel);
    VDX_CHECK(reserved == hipSuccess, "tome_select: cannot reserve LDS: %s", hipGetErrorString(reserved));
    hipLaunchKernelGGL(tm_select_kernel, dim3(a->n_img), dim3(TS_THREADS), lds, (hipStream_t)stream, a->node_max, a->node_idx, a->src_idx,
                       a->dst_idx, a->S, a->n_src, a->n_dst, a->r, n2, a->slot, a->off, a->items);
    return vdx_launch_status("vdx_tome_select");
}

extern "C" int vdx_tome_merge_f16(const vdx_tome_args* a, const void* y, int ldy, void* out, int ldo, vdx_stream_t stream) {
    TM_TRY(tm_check_plan(a, "tome_merge"));
    const int C = a->C;
    VDX_CHECK(C >= 8 && C % 8 == 0, "tome_merge: C=%d (a multiple of 8)", C);
    TM_TRY(tm_check_rows(y, ldy, C, "tome_merge", "y"));
    TM_TRY(tm_check_rows(out, ldo, C, "tome_merge", "out"));
    VDX_CHECK(a->slot && a->off && a->items, "tome_merge: null slot / off / items");
    const size_t work = (size_t)a->n_img * a->S;
    hipLaunchKernelGGL(tm_merge_kernel, dim3((unsigned)((work + 3) / 4)), dim3(TM_THREADS), 0, (hipStream_t)stream, (const f16*)y, (size_t)ldy,
                       a->src_idx, a->dst_idx, a->slot, a->off, a->items, a->S, a->n_src, a->n_dst, a->r, C, work, (f16*)out, (size_t)ldo);
    return vdx_launch_status("vdx_tome_merge_f16");
}

extern "C" int vdx_tome_unmerge_add_f16(const vdx_tome_args* a, const void* x, int ldx, const void* t, int ldt, void* out, int ldo,
                                        vdx_stream_t stream) {
    TM_TRY(tm_check_plan(a, "tome_unmerge_add"));
    const int C = a->C;
    VDX_CHECK(C >= 8 && C % 8 == 0, "tome_unmerge_add: C=%d (a multiple of 8)", C);
    TM_TRY(tm_check_rows(x, ldx, C, "tome_unmerge_add", "x"));
    TM_TRY(tm_check_rows(t, ldt, C, "tome_unmerge_add", "t"));
    TM_TRY(tm_check_rows(out, ldo, C, "tome_unmerge_add", "out"));
    VDX_CHECK(a->slot, "tome_unmerge_add: null slot");
    const int chunks = C / 8;
    const size_t n = (size_t)a->n_img * a->S * chunks;
    const size_t blocks = (n + TM_THREADS - 1) / TM_THREADS, cap = (size_t)vdx_num_cus() * 16;
    hipLaunchKernelGGL(tm_unmerge_add_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(TM_THREADS), 0, (hipStream_t)stream,
                       (const f16*)x, (size_t)ldx, a->slot, (const f16*)t, (size_t)ldt, a->S, a->S - a->r, chunks, n, (f16*)out, (size_t)ldo);
    return vdx_launch_status("vdx_tome_unmerge_add_f16");
}
