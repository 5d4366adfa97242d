// flash_i8.hip — spatial self-attention with an INT8 score product (SageAttention, Zhang et al., ICLR 2025, restated;
// DESIGN.md §30): Q.K^T on v_mfma_i32_32x32x32_i8, softmax and P.V exactly as flash.hip does them (flash_common.h).
//
// Two parts.  The PRE-PASS (vdx_attn_quant_i8, two launches) turns the q and k column blocks of one q|k|v projection into
// packed int8 workspaces: per (image, head) the key mean over the image's S keys is taken in fp32 in a fixed order and
// subtracted (softmax does not see it: q.kbar is constant along a row), q is multiplied by scale*log2(e), and every block of
// 64 consecutive tokens gets one scale delta = amax / 127 and its values rint(x / delta) clamped to +-127.  The layout is
//     q8, k8 : int8 [n_img][heads][S_pad][64]      S_pad = ceil(S / 64) 64, tail rows zero
//     dq, dk : fp32 [n_img][heads][S_pad / 64]
// so a K tile of 64 keys is ONE contiguous 4 KB run: the main kernel stages it with one LDS-DMA instruction per wave, half
// the bytes and a quarter of the address arithmetic of the fp16 tile, and needs no bounds check (the tail is zeros).
//
// The MAIN kernel (vdx_flash_attn_i8_f16) keeps flash.hip's work split — a wave owns QB sub-blocks of 32 queries, 256-thread
// blocks, two per CU, K / V tiles of 64 keys through two LDS stages — and its transposed tile S^T = K.Q^T, so everything
// after the scores (FlSoft, the accumulator-as-operand P, V transposed by ds_read_b64_tr_b16, the store) is shared code.
// What is its own:
//   * a 32 x 32 score block is TWO v_mfma_i32_32x32x32_i8 (k = 64) where fp16 issues four 32x32x16; the i32 accumulator has
//     the f32 one's lane layout, so acc_key / pi_row hold unchanged;
//   * a 64-token quantisation block is a key tile, and a wave's queries lie inside one block, so delta_q delta_k is
//     wave-uniform per tile: the score is fma(float(S^), delta_q delta_k, -m) — the scale and the softmax offset in one
//     instruction per score beside the convert.  (The fp16 kernel folds -m into the contraction by one more MFMA; an integer
//     contraction cannot carry it.)
//   * K in LDS: [64 key][64 B], 16-byte chunk c of row r at chunk c ^ ((r >> 2) & 3).  A fragment read takes, per 16 lanes,
//     16 different rows at one chunk index: row r starts at bank 16 (r & 3), so r & 3 picks the quarter of the 64 banks and
//     (r >> 2) & 3 the 4-bank slot inside it: 16 lanes x 16 B cover the 64 banks once.  The DMA writes rows in order, lane l
//     of wave w to row 16 w + l / 4, slot l & 3, and fetches data chunk (l & 3) ^ ((row >> 2) & 3) for it.
// No atomics; every result depends on its own (image, head) only, in a fixed order: the same bits on every run and for any
// n_img.  NaN or inf in q or k makes the block's delta NaN (the amax is taken on the bit patterns, where NaN is the largest),
// which makes the scores of that block NaN: it surfaces in the rows of its own (image, head) and nowhere else.
#include "flash_common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// ---- the workspace ------------------------------------------------------------------------------------------------------
struct FlI8Layout {
    size_t q8, k8, dq, dk, mean, total;   // byte offsets; `mean`: the pre-pass's key means, fp32 [n_img][heads][64]
    int S_pad, nb;
    long long pairs;
};
static inline bool fl_i8_layout(int n_img, int S, int heads, FlI8Layout& w) {
    if (n_img < 1 || S < 1 || heads < 1 || S > (1 << 24)) return false;
    w.pairs = (long long)n_img * heads;
    w.nb = (S + 63) / 64;
    w.S_pad = w.nb * 64;
    if (w.pairs * w.nb >= (1ll << 31) || w.pairs * 4 * ((S + 127) / 128) >= (1ll << 31)) return false;   // the grids
    const size_t a = (size_t)w.pairs * w.S_pad * 64, b = ((size_t)w.pairs * w.nb * 4 + 15) / 16 * 16;
    w.q8 = 0; w.k8 = a; w.dq = 2 * a; w.dk = 2 * a + b; w.mean = 2 * a + 2 * b;
    w.total = w.mean + (size_t)w.pairs * 64 * 4;
    return true;
}

// do the byte ranges [a, a + na) and [b, b + nb) meet?
static inline bool fl_i8_meet(const void* a, size_t na, const void* b, size_t nb) {
    return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na;
}
static inline size_t fl_i8_rows_bytes(long long rows, int ld, int cols) { return (size_t)((rows - 1) * ld + cols) * sizeof(f16); }

// ---- pre-pass 1: key means ----------------------------------------------------------------------------------------------
// One block per (image, head).  Thread (g, ch) = (tid / 8, tid % 8) adds channels 8 ch .. 8 ch + 7 of rows g, g + 32, ... in
// ascending order; the 32 partial sums of a channel are then added in ascending g, and the total divided by S (IEEE).
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void attn_kmean_kernel(const f16* __restrict__ k, int ldk, int S, int heads, float* __restrict__ mean) {
    __shared__ float part[32][64];
    const int pair = blockIdx.x, head = pair % heads, img = pair / heads;
    const int g = threadIdx.x >> 3, ch = threadIdx.x & 7;
    const f16* src = k + (size_t)img * S * ldk + head * 64 + ch * 8;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll 4
    for (int r = g; r < S; r += 32) {
        const f16x8 x = *(const f16x8*)(src + (size_t)r * ldk);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)x[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[g][ch * 8 + j] = acc[j];
    __syncthreads();
    if (threadIdx.x < 64) {
        float t = 0.f;
        for (int i = 0; i < 32; ++i) t += part[i][threadIdx.x];
        mean[(size_t)pair * 64 + threadIdx.x] = t / (float)S;
    }
}

// ---- pre-pass 2: quantise -----------------------------------------------------------------------------------------------
struct FlI8QuantP {
    const f16 *q, *k;
    const float* mean;
    signed char *q8, *k8;
    float *dq, *dk;
    int ldq, ldk, S, S_pad, nb, heads;
    float c;                       // scale * log2(e)
};

__device__ __forceinline__ unsigned fl_i8_wave_max(unsigned m) {     // max is order-free: the bits do not depend on the tree
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off, 64));
    return m;
}
// 8 values -> 8 int8 of rint(x / delta) clamped to +-127 (IEEE division, round-half-even)
__device__ __forceinline__ uint2 fl_i8_pack(const float (&x)[8], float delta) {
    unsigned w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float r = fminf(fmaxf(rintf(x[j] / delta), -127.0f), 127.0f);
        w[j >> 2] |= ((unsigned)(int)r & 0xffu) << (8 * (j & 3));
    }
    return make_uint2(w[0], w[1]);
}

// One block per (image, head, 64-token block).  Thread (r, ch) = (tid / 8, tid % 8) holds channels 8 ch .. 8 ch + 7 of the
// block's rows r and r + 32, of q and of k, read 16 bytes at a time; rows past S are zeros and take no part in the amax.
__global__ __launch_bounds__(256) void attn_quant_i8_kernel(const FlI8QuantP p) {
    __shared__ unsigned red[2][4];
    const int blk = blockIdx.x % p.nb, pair = blockIdx.x / p.nb, head = pair % p.heads, img = pair / p.heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ch = tid & 7, r0 = tid >> 3;
    float mean[8];
    {
        const f32x4* mp = (const f32x4*)(p.mean + (size_t)pair * 64 + ch * 8);
        const f32x4 m0 = mp[0], m1 = mp[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mean[j] = m0[j];
            mean[4 + j] = m1[j];
        }
    }
    float xq[2][8], xk[2][8];
    unsigned mq = 0u, mk = 0u;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int row = blk * 64 + r0 + 32 * u;
        const bool ok = row < p.S;
        const size_t grow = (size_t)img * p.S + (ok ? row : p.S - 1);
        const f16x8 qv = *(const f16x8*)(p.q + grow * p.ldq + head * 64 + ch * 8);
        const f16x8 kv = *(const f16x8*)(p.k + grow * p.ldk + head * 64 + ch * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            xq[u][j] = ok ? (float)qv[j] * p.c : 0.f;
            xk[u][j] = ok ? (float)kv[j] - mean[j] : 0.f;
            mq = max(mq, __float_as_uint(xq[u][j]) & 0x7fffffffu);   // |x| as bits: monotone for finite values, NaN above inf
            mk = max(mk, __float_as_uint(xk[u][j]) & 0x7fffffffu);
        }
    }
    mq = fl_i8_wave_max(mq);
    mk = fl_i8_wave_max(mk);
    if (lane == 0) {
        red[0][wave] = mq;
        red[1][wave] = mk;
    }
    __syncthreads();
    mq = max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3]));
    mk = max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3]));
    const float aq = __uint_as_float(mq), ak = __uint_as_float(mk);
    const float dq = aq == 0.f ? 1.0f : aq / 127.0f, dk = ak == 0.f ? 1.0f : ak / 127.0f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const size_t at = ((size_t)pair * p.S_pad + blk * 64 + r0 + 32 * u) * 64 + ch * 8;       // tail rows: zeros
        *(uint2*)(p.q8 + at) = fl_i8_pack(xq[u], dq);
        *(uint2*)(p.k8 + at) = fl_i8_pack(xk[u], dk);
    }
    if (tid == 0) {
        p.dq[(size_t)pair * p.nb + blk] = dq;
        p.dk[(size_t)pair * p.nb + blk] = dk;
    }
}
#pragma clang fp contract(fast)

// ---- the main kernel ----------------------------------------------------------------------------------------------------
struct FlI8P {
    const signed char *q8, *k8;
    const float *dq, *dk;
    const f16* v;
    f16* out;
    int ldv, ldo;
    int S, S_pad, nb, heads;
    int xcd;           // XCD-aware block order in use (npairs % 8 == 0), as flash.hip
    int nqb, npairs;
};

template <int QB>
__global__ __launch_bounds__(256) void flash_attn_i8_kernel(const FlI8P p) {
    // LDS: 2 stages x { K tile [64 key][64 B int8] (chunk c of row r at c ^ ((r >> 2) & 3)), V tile [64 key][64 d] fp16
    // (chunk c of row r at c ^ (4 * ((r >> 1) & 1)), flash.hip's VROW layout) } = 2 x 12 KB
    constexpr int STAGE = 4096 + 8192;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    int pair, qblk;
    if (p.xcd) {                                       // all query blocks of a pair on one XCD (flash.hip fl_block_map)
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        pair = (slot / p.nqb) * 8 + xcd;
        qblk = slot % p.nqb;
    } else {
        pair = blockIdx.x / p.nqb;
        qblk = blockIdx.x % p.nqb;
    }
    const int head = pair % p.heads, img = pair / p.heads;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int q0 = (qblk * 4 + wv) * (32 * QB);

    // ---- Q fragments (B operand of S^T = K.Q^T): lane = query column, 16 bytes of d = 32 ks + 16 h ..; rows past S_pad clamp
    i32x4 qf[QB][2];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int qr = min(q0 + qb * 32 + r32, p.S_pad - 1);
        const signed char* src = p.q8 + ((size_t)pair * p.S_pad + qr) * 64 + 16 * h;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[qb][ks] = *(const i32x4*)(src + 32 * ks);
    }
    // a wave's queries lie in one 64-token block: its delta_q is wave-uniform
    const float dqw = p.dq[(size_t)pair * p.nb + min(q0 >> 6, p.nb - 1)];
    const float* dkp = p.dk + (size_t)pair * p.nb;

    // ---- staging by LDS-DMA: per tile and wave ONE K piece (rows 16 wv .. + 15 of the packed tile) and two V pieces
    const f16* zp = (const f16*)g_zero_page;
    const int k_row = tid >> 2;
    const signed char* kptr = p.k8 + ((size_t)pair * p.S_pad + k_row) * 64 + (((tid & 3) ^ ((k_row >> 2) & 3)) << 4);
    const int st_row0 = tid >> 3, st_row1 = st_row0 + 32;
    const int chv = (tid & 7) ^ (((st_row0 >> 1) & 1) << 2);
    const f16* vptr0 = p.v + ((size_t)img * p.S + st_row0) * p.ldv + head * 64 + chv * 8;
    const f16* vptr1 = p.v + ((size_t)img * p.S + st_row1) * p.ldv + head * 64 + chv * 8;
    const size_t vstep = (size_t)64 * p.ldv;
    auto issue = [&](int t, int buf) {
        char* sk = smem + buf * STAGE + wv * 1024;
        const int k0 = t * 64;
        const f16 *v0p = vptr0, *v1p = vptr1;
        if (k0 + 64 > p.S) {                                          // the image's last tile (wave-uniform): rows past S are zeros
            if (k0 + st_row0 >= p.S) v0p = zp;
            if (k0 + st_row1 >= p.S) v1p = zp;
        }
        __builtin_amdgcn_global_load_lds((fl_gptr_t)kptr, (fl_lptr_t)sk, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)v0p, (fl_lptr_t)(sk + 4096), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)v1p, (fl_lptr_t)(sk + 4096 + 4096), 16, 0, 0);
        kptr += 4096;
        vptr0 += vstep;
        vptr1 += vstep;
    };

    f32x16 o_acc[QB][2];
    FlSoft<QB> st;
    st.init();
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int j = 0; j < 16; ++j) o_acc[qb][0][j] = o_acc[qb][1][j] = 0.f;

    const int krow = pi_row(r32);
    const int tr0 = fl_tr_addr(lane), tr1 = tr0 ^ 64;
    const int ntiles = p.nb;
    issue(0, 0);
    __syncthreads();                       // LDS-DMA in flight: the barrier's fence waits vmcnt(0)
    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) issue(t + 1, cur ^ 1);   // buffer cur^1 was last read before the previous barrier
        const char* Ks = smem + cur * STAGE;
        const char* Vs = Ks + 4096;
        const int k0 = t * 64;
        const float dd = dqw * dkp[t];               // delta_q delta_k of this (query block, key tile)

        // ---- S' = float(K^ . Q^^T) dd - m : two 32-key blocks, two k = 32 steps each, a K fragment feeds QB sub-blocks
        f32x16 s_acc[QB][2];
        i32x16 zero16;
#pragma unroll
        for (int j = 0; j < 16; ++j) zero16[j] = 0;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int row = kb * 32 + krow;
            i32x16 si[QB];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int c = 2 * ks + h;
                const i32x4 kf = *(const i32x4*)(Ks + row * 64 + ((c ^ ((row >> 2) & 3)) << 4));
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
                    si[qb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf, qf[qb][ks], ks == 0 ? zero16 : si[qb], 0, 0, 0);
            }
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                const float nm = (float)st.negm[qb][0];              // - (the offset in use); 0 until a row first moves
#pragma unroll
                for (int j = 0; j < 16; ++j) s_acc[qb][kb][j] = __builtin_fmaf((float)si[qb][j], dd, nm);
            }
        }
        if (k0 + 64 > p.S) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (k0 + kb * 32 + acc_key(j, h) >= p.S) s_acc[qb][kb][j] = NEG_BIG;
        }
        // ---- row maxima, p = exp2(S') packed to fp16 pairs, row sums; O^T += V^T . P^T  (flash.hip's, VROW)
        f16x8 pf[QB][4];
        st.tile(s_acc, o_acc, pf, h);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {  // keys 16*kk + 8*h .. +7
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                const f16x8 vf = fl_read_vtr(Vs + (db ? tr1 : tr0) + kk * 2048);
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
                    o_acc[qb][db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[qb][kk], o_acc[qb][db], 0, 0, 0);
            }
        }
        __syncthreads();                   // next tile landed (vmcnt(0)) and this one is fully read
    }
    f16* dst[QB];
    bool ok[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int qi = q0 + qb * 32 + r32;
        dst[qb] = p.out + ((size_t)img * p.S + min(qi, p.S - 1)) * p.ldo + head * 64;
        ok[qb] = qi < p.S;                                           // query rows past S are not stored
    }
    fl_store_rows<QB>(st, o_acc, h, dst, ok);
}

// ---- host entry points --------------------------------------------------------------------------------------------------
extern "C" size_t vdx_attn_quant_i8_workspace(int n_img, int S, int heads) {
    FlI8Layout w;
    return fl_i8_layout(n_img, S, heads, w) ? w.total : 0;
}

extern "C" int vdx_attn_quant_i8(const void* q, int ldq, const void* k, int ldk, int n_img, int S, int heads, float scale,
                                 void* workspace, size_t workspace_bytes, vdx_stream_t stream) {
    VDX_CHECK(q && k && workspace, "attn_quant_i8: null pointer");
    FlI8Layout w;
    VDX_CHECK(fl_i8_layout(n_img, S, heads, w), "attn_quant_i8: n_img=%d S=%d heads=%d is empty or too large", n_img, S, heads);
    const int inner = heads * 64;
    VDX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldq >= inner && ldk >= inner,
              "attn_quant_i8: leading dims must be multiples of 8 and at least heads * 64 = %d (head dimension 64 only)", inner);
    VDX_CHECK((uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && (uintptr_t)workspace % 16 == 0, "attn_quant_i8: pointers must be 16-byte aligned");
    VDX_CHECK(workspace_bytes >= w.total, "attn_quant_i8: workspace of %zu bytes is below the %zu needed", workspace_bytes, w.total);
    const long long rows = (long long)n_img * S;
    VDX_CHECK(rows < (1ll << 31), "attn_quant_i8: %lld rows are more than 2^31", rows);
    VDX_CHECK(!fl_i8_meet(workspace, w.total, q, fl_i8_rows_bytes(rows, ldq, inner)) &&
              !fl_i8_meet(workspace, w.total, k, fl_i8_rows_bytes(rows, ldk, inner)), "attn_quant_i8: the workspace overlaps q or k");
    char* ws = (char*)workspace;
    float* mean = (float*)(ws + w.mean);
    hipLaunchKernelGGL(attn_kmean_kernel, dim3((unsigned)w.pairs), dim3(256), 0, (hipStream_t)stream, (const f16*)k, ldk, S, heads, mean);
    FlI8QuantP p;
    p.q = (const f16*)q; p.k = (const f16*)k; p.mean = mean;
    p.q8 = (signed char*)(ws + w.q8); p.k8 = (signed char*)(ws + w.k8);
    p.dq = (float*)(ws + w.dq); p.dk = (float*)(ws + w.dk);
    p.ldq = ldq; p.ldk = ldk; p.S = S; p.S_pad = w.S_pad; p.nb = w.nb; p.heads = heads;
    p.c = scale * 1.44269504088896341f;
    hipLaunchKernelGGL(attn_quant_i8_kernel, dim3((unsigned)(w.pairs * w.nb)), dim3(256), 0, (hipStream_t)stream, p);
    return vdx_launch_status("vdx_attn_quant_i8");
}

extern "C" int vdx_flash_attn_i8_f16(const void* workspace, size_t workspace_bytes, const void* v, int ldv, void* out, int ldo,
                                     int n_img, int S, int heads, vdx_stream_t stream) {
    VDX_CHECK(workspace && v && out, "flash_attn_i8: null pointer");
    FlI8Layout w;
    VDX_CHECK(fl_i8_layout(n_img, S, heads, w), "flash_attn_i8: n_img=%d S=%d heads=%d is empty or too large", n_img, S, heads);
    const int inner = heads * 64;
    VDX_CHECK(ldv % 8 == 0 && ldo % 8 == 0 && ldv >= inner && ldo >= inner,
              "flash_attn_i8: leading dims must be multiples of 8 and at least heads * 64 = %d (head dimension 64 only)", inner);
    VDX_CHECK((uintptr_t)workspace % 16 == 0 && (uintptr_t)v % 16 == 0 && (uintptr_t)out % 16 == 0, "flash_attn_i8: pointers must be 16-byte aligned");
    VDX_CHECK(workspace_bytes >= w.total, "flash_attn_i8: workspace of %zu bytes is below the %zu needed", workspace_bytes, w.total);
    const long long rows = (long long)n_img * S;
    VDX_CHECK(rows < (1ll << 31), "flash_attn_i8: %lld rows are more than 2^31", rows);
    const size_t ob = fl_i8_rows_bytes(rows, ldo, inner);
    VDX_CHECK(!fl_i8_meet(out, ob, v, fl_i8_rows_bytes(rows, ldv, inner)) && !fl_i8_meet(out, ob, workspace, w.total),
              "flash_attn_i8: out overlaps v or the workspace (an image's keys are read by all of its query blocks)");
    const char* ws = (const char*)workspace;
    FlI8P p;
    p.q8 = (const signed char*)(ws + w.q8); p.k8 = (const signed char*)(ws + w.k8);
    p.dq = (const float*)(ws + w.dq); p.dk = (const float*)(ws + w.dk);
    p.v = (const f16*)v; p.out = (f16*)out; p.ldv = ldv; p.ldo = ldo;
    p.S = S; p.S_pad = w.S_pad; p.nb = w.nb; p.heads = heads;
    p.npairs = (int)w.pairs;
    p.xcd = p.npairs % 8 == 0 ? 1 : 0;
    const bool two = S >= 512;                         // flash.hip's rule: 64 queries per wave when the sequence fills the chip
    p.nqb = two ? (S + 255) / 256 : (S + 127) / 128;
    if (two) hipLaunchKernelGGL((flash_attn_i8_kernel<2>), dim3((unsigned)(p.nqb * p.npairs)), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((flash_attn_i8_kernel<1>), dim3((unsigned)(p.nqb * p.npairs)), dim3(256), 0, (hipStream_t)stream, p);
    return vdx_launch_status("vdx_flash_attn_i8_f16");
}
