// flash_kvdown.hip — ToDo, token downsampling (Smith et al. 2024): the spatial self-attention of a frame with the queries at
// full resolution and the keys and values taken from every s-th row and column of the token grid, read IN PLACE in the row
// layout [n_img * hh * ww][C].  With kh = hh / s, kw = ww / s (floors), Tk = kh kw, key j of image n is row
//     n hh ww + (j / kw) s ww + (j % kw) s
// which is F.interpolate(scale_factor = 1 / s, mode = "nearest") of the token grid; rows and columns from kh s and kw s on
// are never keys.  Nothing is gathered around the kernel.  The tile is flash.hip's (flash_common.h): transposed scores, lazy
// monotone softmax offset folded into the score contraction, four max / sum chains, V transposed by ds_read_b64_tr_b16, the
// same LDS swizzles, LDS-DMA staging in two stages.  What is this kernel's own:
//   * the two sides of the product are addressed differently.  QUERIES are the image's S = hh ww rows as they lie: no map, a
//     lane's row is n S + its query index and a wave's Q fragments are loaded once.  KEYS go through the strided map, which
//     costs no division: a staged key's (y, x) at kernel entry comes from one multiplication by 1 / kw (exact for
//     Tk <= 2^20, fl_kvd_split), and the rows of the NEXT tile from the carried x — x += 64 % kw, one compare, one select —
//     with the row step of 64 keys, (64 / kw) s ww + (64 % kw) s, and the run wrap, s (ww - kw), as launch constants;
//   * keys Tk.. of the last tile are staged from the zero page and masked: no lane ever loads from a row that is not a key,
//     from the skipped tail rows or columns or from the next image; query lanes past S read the image's last row and store
//     nothing, and waves whose queries all lie past S keep staging and the barriers but skip the tile's work;
//   * blocks are dealt to XCDs by pair: all query blocks of an (image, head) pair run on XCD pair % 8 (the grid is rounded
//     up to a multiple of 8 pairs; the surplus blocks leave before any barrier), so a pair's Tk 256 bytes of K and V (590 KB
//     at 72 x 128, s = 2; nqb = 36 blocks re-read them) stay in that XCD's 4 MB L2 and come from HBM once;
//   * the queries per wave follow flash.hip's rule on (S, Tk), so the tile order and every rounding are those of
//     vdx_flash_attn_rows_f16 on the gathered keys: the two give the same bits (tests/test_kvdown_gpu.py).
// No atomics; a query's result depends on its own row and its image's Tk keys only, in a fixed order: the same bits on every
// run and for any n_img.  Keeping the pair's whole K / V in LDS is priced and rejected in DESIGN.md §28.
#include "flash_common.h"

struct FlKvdP {
    const f16 *q, *k, *v;
    f16* out;
    int ldq, ldk, ldv, ldo;
    int S, Tk, kw, heads;          // tokens per image; keys per image; keys per key-grid row
    int xstep, ystep;              // rows between neighbouring keys of a run: s; between key-grid rows: s ww
    int rstep, dx, wrap;           // 64 keys on: rstep = (64 / kw) s ww + (64 % kw) s rows, x += dx = 64 % kw; a run wrap adds s (ww - kw) rows
    int nqb, npairs;               // query blocks per pair; pairs = n_img * heads
    float inv_kw;                  // 1 / kw
    float c;                       // scale * log2(e)
};

__device__ __forceinline__ f32x16 fl_kvd_mfma(const f16x8 a, const f16x8 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// key j -> (y, x) = (j / kw, j % kw) without a division (flash_win.hip fl_win_split): (j + 0.5) / kw is at least 0.5 / kw away
// from an integer and the fp32 product is off by less than (j / kw) 2^-22, so the floor is exact while j < Tk <= 2^20 (the
// launcher's check; the caller clamps j to Tk - 1)
__device__ __forceinline__ void fl_kvd_split(const FlKvdP& p, int j, int& y, int& x) {
    y = (int)(((float)j + 0.5f) * p.inv_kw);
    x = j - y * p.kw;
}

template <int QB>
__global__ __launch_bounds__(256) void flash_attn_kvdown_kernel(const FlKvdP p) {
    // LDS: 2 stages x { K tile [64 key][64 d] (chunk c of row r at c ^ ((r >> 1) & 7)), V tile [64 key][64 d] (chunk c of
    // row r at c ^ (4 * ((r >> 1) & 1))) }, 128-B rows: flash_attn_kernel<QB, false, true>'s layout
    __shared__ __attribute__((aligned(16))) char smem[2 * 16384];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    // ---- block -> (pair, query block): pair % 8 is the XCD (blocks L and L + 8 share one); surplus pairs leave
    const int slot = blockIdx.x >> 3;
    const int pair = (slot / p.nqb) * 8 + (blockIdx.x & 7), qblk = slot % p.nqb;
    if (pair >= p.npairs) return;                                    // block-uniform, before any barrier
    const int head = pair % p.heads, base = (pair / p.heads) * p.S;  // the image's first row
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int q0 = (qblk * 4 + wv) * (32 * QB);
    const bool active = q0 < p.S;                                    // wave-uniform: some query of this wave exists

    // ---- Q fragments (B operand of S^T = K.Q^T): lane = query column, pre-scaled; consecutive rows, no map
    f16x8 qf[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const f16* src = p.q + (size_t)(base + min(q0 + qb * 32 + r32, p.S - 1)) * p.ldq + head * 64 + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const f16x8 raw = *(const f16x8*)(src + 16 * ks);
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[qb][ks][j] = (f16)((float)raw[j] * p.c);
        }
    }

    // ---- staging by LDS-DMA: per tile a lane fetches one 16-byte chunk of keys st_row0 and st_row0 + 32 of the tile, for K
    // and for V.  (sx, sr): the carried key-grid x and the row of those two keys in the CURRENT tile to issue.
    const f16* zp = (const f16*)g_zero_page;
    const int st_row0 = tid >> 3;
    const int chk0 = ((tid & 7) ^ ((st_row0 >> 1) & 7)) * 8, chk1 = ((tid & 7) ^ (((st_row0 + 32) >> 1) & 7)) * 8;
    const int chv = ((tid & 7) ^ (((st_row0 >> 1) & 1) << 2)) * 8;
    const f16 *kb0 = p.k + head * 64 + chk0, *kb1 = p.k + head * 64 + chk1, *vb = p.v + head * 64 + chv;
    // A key below Tk has a row below 2^30 and so has its successor 64 keys on if that is a key; the carried row of a key past
    // Tk (one step further, twice at the most) is never used and wraps harmlessly as an unsigned.
    int sx[2];
    unsigned sr[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        int y;
        fl_kvd_split(p, min(st_row0 + 32 * u, p.Tk - 1), y, sx[u]);
        sr[u] = (unsigned)(base + y * p.ystep + sx[u] * p.xstep);
    }
    auto issue = [&](int t, int buf) {
        char* sk = smem + buf * 16384 + wv * 1024;
        const int k0 = t * 64;
        // keys Tk.. (only in the last tile) are zeros: their carried row is never turned into an address
        const bool in0 = k0 + st_row0 < p.Tk, in1 = k0 + st_row0 + 32 < p.Tk;
        const f16 *k0p = in0 ? kb0 + (size_t)sr[0] * p.ldk : zp, *k1p = in1 ? kb1 + (size_t)sr[1] * p.ldk : zp;
        const f16 *v0p = in0 ? vb + (size_t)sr[0] * p.ldv : zp, *v1p = in1 ? vb + (size_t)sr[1] * p.ldv : zp;
        __builtin_amdgcn_global_load_lds((fl_gptr_t)k0p, (fl_lptr_t)sk, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)k1p, (fl_lptr_t)(sk + 4096), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)v0p, (fl_lptr_t)(sk + 8192), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)v1p, (fl_lptr_t)(sk + 8192 + 4096), 16, 0, 0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {                                // 64 keys on
            sx[u] += p.dx;
            const bool w = sx[u] >= p.kw;
            sx[u] -= w ? p.kw : 0;
            sr[u] += p.rstep + (w ? p.wrap : 0);
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
    const int ntiles = (p.Tk + 63) >> 6;
    issue(0, 0);
    __syncthreads();                       // LDS-DMA in flight: the barrier's fence waits vmcnt(0)
    for (int t = 0; t < ntiles; ++t) {
        const int cur = t & 1;
        if (t + 1 < ntiles) issue(t + 1, cur ^ 1);   // buffer cur^1 was last read before the previous barrier
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
                        s_acc[qb][kb] = fl_kvd_mfma(kf, qf[qb][ks], ks == 0 ? zero16 : s_acc[qb][kb]);
                }
                if (st.offset_on) {
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb)
                        s_acc[qb][kb] = fl_kvd_mfma(e0, st.negm[qb], s_acc[qb][kb]);   // - m
                }
            }
            if (k0 + 64 > p.Tk) {                    // the image's last tile (wave-uniform)
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int j = 0; j < 16; ++j)
                            if (k0 + kb * 32 + acc_key(j, h) >= p.Tk) s_acc[qb][kb][j] = NEG_BIG;
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
                    for (int qb = 0; qb < QB; ++qb) o_acc[qb][db] = fl_kvd_mfma(vf, pf[qb][kk], o_acc[qb][db]);
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
            const int qi = q0 + qb * 32 + r32;
            dst[qb] = p.out + (size_t)(base + min(qi, p.S - 1)) * p.ldo + head * 64;
            ok[qb] = qi < p.S;                                       // query rows past S are not stored
        }
        fl_store_rows<QB>(st, o_acc, h, dst, ok);
    }
}

// How many queries a wave owns: flash.hip's rule (flash_launch's `two`) on the image's S queries and Tk keys, so that this
// kernel and vdx_flash_attn_rows_f16 on the gathered keys run the same instantiation of the tile.
static inline int fl_kvd_qb(int S, int Tk) { return S >= 512 && Tk >= 256 ? 2 : 1; }

// do the byte ranges of two row matrices of `rows` rows of `cols` fp16 meet?
static inline bool fl_kvd_overlap(const void* a, int lda, const void* b, int ldb, long long rows, int cols) {
    const char *a0 = (const char*)a, *b0 = (const char*)b;
    const char *a1 = a0 + ((rows - 1) * lda + cols) * (long long)sizeof(f16), *b1 = b0 + ((rows - 1) * ldb + cols) * (long long)sizeof(f16);
    return a0 < b1 && b0 < a1;
}

extern "C" int vdx_flash_attn_kvdown_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                                         void* out, int ldo, int n_img, int hh, int ww, int s,
                                         int heads, float scale, vdx_stream_t stream) {
    VDX_CHECK(q && k && v && out, "flash_attn_kvdown: null pointer");
    VDX_CHECK(n_img > 0 && hh > 0 && ww > 0 && heads > 0, "flash_attn_kvdown: empty problem");
    VDX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "flash_attn_kvdown: leading dims must be multiples of 8");
    const int inner = heads * 64;
    VDX_CHECK(ldq >= inner && ldk >= inner && ldv >= inner && ldo >= inner, "flash_attn_kvdown: a leading dim below heads * 64 = %d", inner);
    VDX_CHECK(s >= 2, "flash_attn_kvdown: factor %d; 1 is the plain attention (vdx_flash_attn_rows_f16)", s);
    VDX_CHECK(hh / s >= 1 && ww / s >= 1, "flash_attn_kvdown: factor %d leaves no key in %d x %d tokens", s, hh, ww);
    const long long rows = (long long)n_img * hh * ww;
    VDX_CHECK(rows < (1ll << 30), "flash_attn_kvdown: %lld rows are more than 2^30", rows);
    const int kh = hh / s, kw = ww / s;
    VDX_CHECK((long long)kh * kw <= (1 << 20), "flash_attn_kvdown: %d x %d keys per image are more than 2^20", kh, kw);
    VDX_CHECK(!fl_kvd_overlap(out, ldo, k, ldk, rows, inner) && !fl_kvd_overlap(out, ldo, v, ldv, rows, inner),
              "flash_attn_kvdown: out overlaps k or v (an image's key rows are read by all of its query blocks)");
    FlKvdP p;
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.out = (f16*)out;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.S = hh * ww; p.Tk = kh * kw; p.kw = kw; p.heads = heads;
    p.xstep = s; p.ystep = s * ww;
    // the 64-key row step is the distance between two key rows of one image (< 2^30) when there is a second tile; unused otherwise
    p.dx = 64 % kw; p.rstep = p.Tk > 64 ? (64 / kw) * p.ystep + p.dx * s : 0; p.wrap = s * (ww - kw);
    p.inv_kw = 1.0f / (float)kw;
    p.c = scale * 1.44269504088896341f;
    const int qbs = fl_kvd_qb(p.S, p.Tk);
    const long long npairs = (long long)n_img * heads;
    p.nqb = (p.S + 128 * qbs - 1) / (128 * qbs);
    const long long blocks = (npairs + 7) / 8 * 8 * p.nqb;
    VDX_CHECK(blocks < (1ll << 31), "flash_attn_kvdown: grid too large");
    p.npairs = (int)npairs;
    if (qbs == 2) hipLaunchKernelGGL((flash_attn_kvdown_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((flash_attn_kvdown_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return vdx_launch_status("vdx_flash_attn_kvdown_f16");
}
