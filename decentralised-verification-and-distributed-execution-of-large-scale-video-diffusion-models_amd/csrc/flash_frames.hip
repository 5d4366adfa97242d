// flash_frames.hip — cross-frame attention: the spatial self-attention of frame f of a sample with its keys and values
// taken from R REFERENCE FRAMES of the same sample, named by a table refs[F][R].  Text2Video-Zero's
// first-frame attention, Tune-A-Video's sparse-causal attention and "extended" attention are tables.  q, k, v and out are
// the row matrices [n_samples * F * S][ld] of flash.hip's row layout; key j (0 <= j < R S) of query image (b, f) is row
//     (b F + refs[f][j / S]) S + j % S
// and the rows are read where they lie: nothing is gathered or concatenated around the kernel.  The tile is flash.hip's
// (flash_common.h): transposed scores, lazy monotone softmax offset folded into the score contraction, four max / sum
// chains, V transposed by ds_read_b64_tr_b16, the same LDS swizzles, LDS-DMA staging in two stages.  This kernel's own:
//   * ONE PACKED KEY STREAM.  The R frames are one sequence of R S keys and the tiles of 64 keys run straight across
//     the frame seams, so only the LAST tile of the stream is masked (S = 45, R = 2: 2 tiles, not 2 x 1 padded ones of
//     which each is a third empty; S = 144, R = 3: 7 tiles, not 9).  A lane carries each of its two staged keys as
//     (segment, offset): per tile offset += 64, then while offset >= S: offset -= S, segment++ (the loop runs at most R
//     times in the kernel's life, since it stops at segment == R).  There is no division, and the row base of a
//     segment is a select among R <= 4 bases that the block computed once from its table row: no data-dependent
//     address beyond that select, every table entry clamped to 0 .. F - 1 on top of the host's check;
//   * keys R S .. of the last tile are exactly the keys with segment == R: they are staged from the zero page and
//     masked.  No lane ever forms a load outside the R referenced frames of its own sample (and, for q, outside its
//     own frame: query lanes past S read the frame's last row and store nothing);
//   * waves whose 32 QB queries all lie past S keep staging and keep the barriers but skip the tile's matrix and
//     vector work (flash_win.hip's rule);
//   * BLOCK MAP.  A unit is a (sample, head, frame): nqb query blocks that stream the same R S keys.  The U units, in
//     (sample, head)-major, frame-minor order, are cut into 8 CONTIGUOUS runs of ceil(U / 8), one per XCD (block L runs on
//     XCD L % 8; the grid is rounded up and the surplus blocks leave at once).  Every XCD gets the same work whatever the
//     number of (sample, head) pairs — dealing whole pairs by pair % 8, HyperTile's rule, was measured first and left
//     6 of 8 XCDs idle half the time at level 0, where a CFG batch has 10 pairs — and a run still holds
//     the consecutive frames of one pair (two at a run's seam) in ascending order, a frame's query blocks next to each
//     other: the blocks resident together stream the same anchor frame (2.4 MB of K and V per pair at level 0) from that
//     XCD's L2, and frames f and f + 1 share the moving reference too (f - 1 | f for one, f | f + 1 for the other).
// No atomics; a query's result depends on its own row and its R S keys only, in a fixed order: the same bits on every
// run and for any n_samples.
#include "flash_common.h"

#define FL_FRAMES_MAX_R 4

struct FlFramesP {
    const f16 *q, *k, *v;
    f16* out;
    const int* refs;               // device int32 [F][R]
    int ldq, ldk, ldv, ldo;
    int S, F, R, heads;
    int nqb, units, upx;           // query blocks per frame; units = n_samples * heads * F; units per XCD = ceil(units / 8)
    float c;                       // scale * log2(e)
};

__device__ __forceinline__ f32x16 fl_frames_mfma(const f16x8 a, const f16x8 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

template <int QB>
__global__ __launch_bounds__(256) void flash_attn_frames_kernel(const FlFramesP p) {
    // LDS: 2 stages x { K tile [64 key][64 d] (chunk c of row r at c ^ ((r >> 1) & 7)), V tile [64 key][64 d] (chunk c of
    // row r at c ^ (4 * ((r >> 1) & 1))) }, 128-B rows: flash_attn_kernel<QB, false, true>'s layout
    __shared__ __attribute__((aligned(16))) char smem[2 * 16384];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    // ---- block -> (unit, query block): blocks L and L + 8 share an XCD, which owns units upx (L % 8) .. + upx - 1
    const int slot = blockIdx.x >> 3;
    const int unit = (blockIdx.x & 7) * p.upx + slot / p.nqb, qblk = slot % p.nqb;
    if (slot / p.nqb >= p.upx || unit >= p.units) return;            // block-uniform, before any barrier
    const int pair = unit / p.F, frame = unit % p.F;                 // ascending frames, a frame's blocks adjacent
    const int head = pair % p.heads, sample = pair / p.heads;
    const int img0 = sample * p.F;                                   // the sample's first image
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int q0 = (qblk * 4 + wv) * (32 * QB);
    const bool active = q0 < p.S;                                    // wave-uniform: some query of this wave exists

    // ---- the frame's table row -> the first row of every segment (uniform: scalar loads, clamped)
    int seg_row[FL_FRAMES_MAX_R];
#pragma unroll
    for (int s = 0; s < FL_FRAMES_MAX_R; ++s) {
        const int ref = p.refs[frame * p.R + min(s, p.R - 1)];
        seg_row[s] = (img0 + min(max(ref, 0), p.F - 1)) * p.S;
    }

    // ---- Q fragments (B operand of S^T = K.Q^T): lane = query column, pre-scaled; the lane's rows are kept for the store
    f16x8 qf[QB][4];
    int qrow[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        qrow[qb] = (img0 + frame) * p.S + min(q0 + qb * 32 + r32, p.S - 1);
        const f16* src = p.q + (size_t)qrow[qb] * p.ldq + head * 64 + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const f16x8 raw = *(const f16x8*)(src + 16 * ks);
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[qb][ks][j] = (f16)((float)raw[j] * p.c);
        }
    }

    // ---- staging by LDS-DMA: per tile a lane fetches one 16-byte chunk of keys st_row0 and st_row0 + 32 of the tile, for
    // K and for V.  (sg, so): the segment and the offset inside it of those two keys in the CURRENT tile to issue;
    // sg == R: the key is past the stream's end.
    const f16* zp = (const f16*)g_zero_page;
    const int st_row0 = tid >> 3;
    const int chk0 = ((tid & 7) ^ ((st_row0 >> 1) & 7)) * 8, chk1 = ((tid & 7) ^ (((st_row0 + 32) >> 1) & 7)) * 8;
    const int chv = ((tid & 7) ^ (((st_row0 >> 1) & 1) << 2)) * 8;
    const f16 *kb0 = p.k + head * 64 + chk0, *kb1 = p.k + head * 64 + chk1, *vb = p.v + head * 64 + chv;
    int sg[2], so[2];
    auto wrap = [&](int u) {
        while (so[u] >= p.S && sg[u] < p.R) {
            so[u] -= p.S;
            ++sg[u];
        }
    };
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        sg[u] = 0;
        so[u] = st_row0 + 32 * u;
        wrap(u);
    }
    auto seg_base = [&](int s) {                                     // a select among the R bases, no indexed memory
        return s == 0 ? seg_row[0] : s == 1 ? seg_row[1] : s == 2 ? seg_row[2] : seg_row[3];
    };
    auto issue = [&](int buf) {
        char* sk = smem + buf * 16384 + wv * 1024;
        const int r0 = seg_base(sg[0]) + so[0], r1 = seg_base(sg[1]) + so[1];
        const f16 *k0p = kb0 + (size_t)r0 * p.ldk, *k1p = kb1 + (size_t)r1 * p.ldk;
        const f16 *v0p = vb + (size_t)r0 * p.ldv, *v1p = vb + (size_t)r1 * p.ldv;
        if (sg[0] >= p.R) k0p = v0p = zp;                            // keys R S ..: zeros, masked below
        if (sg[1] >= p.R) k1p = v1p = zp;
        __builtin_amdgcn_global_load_lds((fl_gptr_t)k0p, (fl_lptr_t)sk, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)k1p, (fl_lptr_t)(sk + 4096), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)v0p, (fl_lptr_t)(sk + 8192), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)v1p, (fl_lptr_t)(sk + 8192 + 4096), 16, 0, 0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {                                // 64 keys on
            so[u] += 64;
            wrap(u);
        }
    };

    f32x16 o_acc[QB][2];
    FlSoft<QB> st;
    st.init();
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int j = 0; j < 16; ++j) o_acc[qb][0][j] = o_acc[qb][1][j] = 0.f;

    const f16x8 e0 = FlSoft<QB>::e0(h);
    const int krow = pi_row(r32);
    const int tr0 = fl_tr_addr(lane), tr1 = tr0 ^ 64;
    const int T = p.R * p.S, ntiles = (T + 63) >> 6;
    issue(0);
    __syncthreads();                       // LDS-DMA in flight: the barrier's fence waits vmcnt(0)
    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) issue(cur ^ 1);          // buffer cur^1 was last read before the previous barrier
        if (active) {
            const char* Ks = smem + cur * 16384;
            const char* Vs = Ks + 8192;
            const int k0 = t * 64;
            // ---- S' = K . Q^T - m : two 32-key blocks, each K fragment feeds QB sub-blocks
            f32x16 s_acc[QB][2], zero16;
#pragma unroll
            for (int j = 0; j < 16; ++j) zero16[j] = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int row = kb * 32 + krow;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int c = 2 * ks + h;
                    const f16x8 kf = *(const f16x8*)(Ks + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb)
                        s_acc[qb][kb] = fl_frames_mfma(kf, qf[qb][ks], ks == 0 ? zero16 : s_acc[qb][kb]);
                }
                if (st.offset_on) {
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb)
                        s_acc[qb][kb] = fl_frames_mfma(e0, st.negm[qb], s_acc[qb][kb]);   // - m
                }
            }
            if (k0 + 64 > T) {                       // the stream's last tile (wave-uniform)
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int j = 0; j < 16; ++j)
                            if (k0 + kb * 32 + acc_key(j, h) >= T) s_acc[qb][kb][j] = NEG_BIG;
            }
            // ---- row maxima, p = exp2(S') packed to fp16 pairs, row sums; O^T += V^T . P^T
            f16x8 pf[QB][4];
            st.tile(s_acc, o_acc, pf, h);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {  // keys 16*kk + 8*h .. +7
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const f16x8 vf = fl_read_vtr(Vs + (db ? tr1 : tr0) + kk * 2048);
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) o_acc[qb][db] = fl_frames_mfma(vf, pf[qb][kk], o_acc[qb][db]);
                }
            }
        }
        __syncthreads();                   // next tile landed (vmcnt(0)) and this one is fully read
    }
    if (active) {
        f16* dst[QB];
        bool ok[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            dst[qb] = p.out + (size_t)qrow[qb] * p.ldo + head * 64;
            ok[qb] = q0 + qb * 32 + r32 < p.S;                       // query rows past S are not stored
        }
        fl_store_rows<QB>(st, o_acc, h, dst, ok);
    }
}

// How many queries a wave owns: flash_win.hip's rule on the frame's tokens (64 from S = 512 on, 32 below).
static inline int fl_frames_qb(int S) { return S >= 512 ? 2 : 1; }

// the byte range [first, last) of a row matrix of `rows` rows of `cols` fp16 at leading dimension ld
static inline bool fl_frames_overlap(const void* a, int lda, const void* b, int ldb, long long rows, int cols) {
    const char *a0 = (const char*)a, *b0 = (const char*)b;
    const char *a1 = a0 + ((rows - 1) * lda + cols) * (long long)sizeof(f16), *b1 = b0 + ((rows - 1) * ldb + cols) * (long long)sizeof(f16);
    return a0 < b1 && b0 < a1;
}

extern "C" int vdx_flash_attn_frames_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                                         void* out, int ldo, int n_samples, int F, int S, int heads,
                                         const int* refs, int R, float scale, vdx_stream_t stream) {
    VDX_CHECK(n_samples > 0 && F > 0 && S > 0 && heads > 0, "flash_attn_frames: empty problem");
    VDX_CHECK(R >= 1 && R <= FL_FRAMES_MAX_R, "flash_attn_frames: %d reference frames per frame (1 .. %d)", R, FL_FRAMES_MAX_R);
    VDX_CHECK(q && k && v && out && refs, "flash_attn_frames: null pointer");
    VDX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "flash_attn_frames: leading dims must be multiples of 8");
    const int inner = heads * 64;
    VDX_CHECK(ldq >= inner && ldk >= inner && ldv >= inner && ldo >= inner, "flash_attn_frames: a leading dim below heads * 64 = %d", inner);
    const long long rows = (long long)n_samples * F * S;
    VDX_CHECK(rows < (1ll << 30), "flash_attn_frames: %lld rows are more than 2^30", rows);
    VDX_CHECK((long long)R * S <= (1 << 20), "flash_attn_frames: %lld keys per query are more than 2^20", (long long)R * S);
    VDX_CHECK(!fl_frames_overlap(out, ldo, q, ldq, rows, inner) && !fl_frames_overlap(out, ldo, k, ldk, rows, inner) &&
                  !fl_frames_overlap(out, ldo, v, ldv, rows, inner),
              "flash_attn_frames: out overlaps q, k or v (a frame's rows are keys of other frames' blocks still running)");
    FlFramesP p;
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.out = (f16*)out; p.refs = refs;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.S = S; p.F = F; p.R = R; p.heads = heads;
    p.c = scale * 1.44269504088896341f;
    const int qbs = fl_frames_qb(S);
    const long long units = (long long)n_samples * heads * F;
    p.nqb = (S + 128 * qbs - 1) / (128 * qbs);
    const long long blocks = (units + 7) / 8 * 8 * p.nqb;
    VDX_CHECK(blocks < (1ll << 31), "flash_attn_frames: grid too large");
    p.units = (int)units; p.upx = (int)((units + 7) / 8);
    if (qbs == 2) hipLaunchKernelGGL((flash_attn_frames_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((flash_attn_frames_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return vdx_launch_status("vdx_flash_attn_frames_f16");
}
