// flash_win.hip — HyperTile: the spatial self-attention of a frame computed inside the windows of an ny x nx grid, read and
// written IN PLACE in the row layout [n_img * hh * ww][C].  A window's T = th * tw tokens are th runs of tw
// rows that lie ww rows apart, so every access to q, k, v and out goes through the row map
//     token i of window (n, wy, wx)  ->  row  n hh ww + (wy th + i / tw) ww + wx tw + i % tw
// and nothing is gathered or scattered around the kernel.  The tile itself is flash.hip's (flash_common.h): transposed scores,
// lazy monotone softmax offset folded into the score contraction, four max / sum chains, V transposed by ds_read_b64_tr_b16,
// the same LDS swizzles.  What is this kernel's own:
//   * the map costs no division anywhere: a token's (y, x) at kernel entry comes from one multiplication by 1 / tw (exact for
//     T <= 2^20, fl_win_split), and the staging rows of the NEXT tile from the carried x — x += 64 % tw, one compare, one
//     select — with the row stride of 64 tokens and the run-wrap stride as launch constants: 5 integer operations per staged
//     row per tile, two staged rows per lane, plus one 64-bit multiply-add per LDS-DMA source pointer;
//   * keys T.. of a window's last tile are staged from the zero page and masked: no lane ever forms a load from a row of the
//     neighbouring window or the next image; query lanes past T read the window's last row and store nothing;
//   * waves whose 32 QB queries all lie past T keep staging and keep the barriers but skip the tile's matrix and vector
//     work, so a block's tail costs a SIMD nothing but its share of the DMA;
//   * blocks are dealt to XCDs by pair: all query blocks of a (window, head) pair run on XCD pair % 8, whatever the pair
//     count (the grid is rounded up to a multiple of 8 pairs; the surplus blocks leave at once), so a window's K / V tiles
//     are re-read from that XCD's L2 and come from HBM once.
// The whole-window-resident alternative (K and V of T <= 576 tokens held in 147 KB of LDS) is rejected in DESIGN.md §26.
#include "flash_common.h"

struct FlWinP {
    const f16 *q, *k, *v;
    f16* out;
    int ldq, ldk, ldv, ldo;
    int ww, tw, T;                 // row length of the image, of a window; tokens per window
    int nx, ny, heads;
    int img_rows, band_rows;       // hh * ww; th * ww
    int rstep, dx, wrap;           // 64 tokens on: rstep = (64 / tw) ww + 64 % tw rows, x += dx = 64 % tw; a run wrap adds ww - tw rows
    int nqb, npairs;               // query blocks per pair; pairs = n_img * ny * nx * heads
    float inv_tw;                  // 1 / tw
    float c;                       // scale * log2(e)
};

__device__ __forceinline__ f32x16 fl_win_mfma(const f16x8 a, const f16x8 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// token i -> (y, x) = (i / tw, i % tw) without a division: (i + 0.5) / tw is at least 0.5 / tw away from an integer and the fp32
// product is off by less than th 2^-22, so the floor is exact while th tw = T <= 2^20 (the launcher's check)
__device__ __forceinline__ void fl_win_split(const FlWinP& p, int i, int& y, int& x) {
    y = (int)(((float)i + 0.5f) * p.inv_tw);
    x = i - y * p.tw;
}

template <int QB>
__global__ __launch_bounds__(256) void flash_attn_win_kernel(const FlWinP p) {
    // LDS: 2 stages x { K tile [64 key][64 d] (chunk c of row r at c ^ ((r >> 1) & 7)), V tile [64 key][64 d] (chunk c of
    // row r at c ^ (4 * ((r >> 1) & 1))) }, 128-B rows: flash_attn_kernel<QB, false, true>'s layout
    __shared__ __attribute__((aligned(16))) char smem[2 * 16384];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, h = lane >> 5;
    // ---- block -> (pair, query block): pair % 8 is the XCD (blocks L and L + 8 share one); surplus pairs leave
    const int slot = blockIdx.x >> 3;
    const int pair = (slot / p.nqb) * 8 + (blockIdx.x & 7), qblk = slot % p.nqb;
    if (pair >= p.npairs) return;                                    // block-uniform, before any barrier
    const int head = pair % p.heads, win = pair / p.heads;
    const int wx = win % p.nx, wyn = win / p.nx;
    const int base = (wyn / p.ny) * p.img_rows + (wyn % p.ny) * p.band_rows + wx * p.tw;   // the window's first row
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int q0 = (qblk * 4 + wv) * (32 * QB);
    const bool active = q0 < p.T;                                    // wave-uniform: some query of this wave exists

    // ---- Q fragments (B operand of S^T = K.Q^T): lane = query column, pre-scaled; the lane's rows are kept for the store
    f16x8 qf[QB][4];
    int qrow[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        int y, x;
        fl_win_split(p, min(q0 + qb * 32 + r32, p.T - 1), y, x);
        qrow[qb] = base + y * p.ww + x;
        const f16* src = p.q + (size_t)qrow[qb] * p.ldq + head * 64 + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const f16x8 raw = *(const f16x8*)(src + 16 * ks);
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[qb][ks][j] = (f16)((float)raw[j] * p.c);
        }
    }

    // ---- staging by LDS-DMA: per tile a lane fetches one 16-byte chunk of key rows st_row0 and st_row0 + 32, for K and
    // for V.  (sx, sr): the carried x and row of those two keys in the CURRENT tile to issue.
    const f16* zp = (const f16*)g_zero_page;
    const int st_row0 = tid >> 3;
    const int chk0 = ((tid & 7) ^ ((st_row0 >> 1) & 7)) * 8, chk1 = ((tid & 7) ^ (((st_row0 + 32) >> 1) & 7)) * 8;
    const int chv = ((tid & 7) ^ (((st_row0 >> 1) & 1) << 2)) * 8;
    const f16 *kb0 = p.k + head * 64 + chk0, *kb1 = p.k + head * 64 + chk1, *vb = p.v + head * 64 + chv;
    int sx[2], sr[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        int y;
        fl_win_split(p, st_row0 + 32 * u, y, sx[u]);
        sr[u] = base + y * p.ww + sx[u];
    }
    auto issue = [&](int t, int buf) {
        char* sk = smem + buf * 16384 + wv * 1024;
        const int k0 = t * 64;
        const f16 *k0p = kb0 + (size_t)sr[0] * p.ldk, *k1p = kb1 + (size_t)sr[1] * p.ldk;
        const f16 *v0p = vb + (size_t)sr[0] * p.ldv, *v1p = vb + (size_t)sr[1] * p.ldv;
        if (k0 + 64 > p.T) {                                         // the window's last tile (wave-uniform): keys T.. are zeros
            if (k0 + st_row0 >= p.T) k0p = v0p = zp;
            if (k0 + st_row0 + 32 >= p.T) k1p = v1p = zp;
        }
        __builtin_amdgcn_global_load_lds((fl_gptr_t)k0p, (fl_lptr_t)sk, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)k1p, (fl_lptr_t)(sk + 4096), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)v0p, (fl_lptr_t)(sk + 8192), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((fl_gptr_t)v1p, (fl_lptr_t)(sk + 8192 + 4096), 16, 0, 0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {                                // 64 tokens on
            sx[u] += p.dx;
            const bool w = sx[u] >= p.tw;
            sx[u] -= w ? p.tw : 0;
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
    const int ntiles = (p.T + 63) >> 6;
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
                        s_acc[qb][kb] = (ks & 1) ? fl_win_mfma(kf, qf[qb][ks], s_acc[qb][kb]) : fl_win_mfma(kf, qf[qb][ks], ks == 0 ? zero16 : s_acc[qb][kb]);
                }
                if (st.offset_on) {
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb)
                        s_acc[qb][kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(e0, st.negm[qb], s_acc[qb][kb], 0, 0, 0);   // - m
                }
            }
            if (k0 + 64 > p.T) {
#pragma unroll
                for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int j = 0; j < 16; ++j)
                            if (k0 + kb * 32 + acc_key(j, h) >= p.T) s_acc[qb][kb][j] = NEG_BIG;
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
                    for (int qb = 0; qb < QB; ++qb)
                        o_acc[qb][db] = (kk & 1) ? fl_win_mfma(vf, pf[qb][kk], o_acc[qb][db]) : fl_win_mfma(vf, pf[qb][kk], o_acc[qb][db]);
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
            ok[qb] = q0 + qb * 32 + r32 < p.T;                       // query rows past T are not stored
        }
        fl_store_rows<QB>(st, o_acc, h, dst, ok);
    }
}

// How many queries a wave owns: 64 from T = 512 on, where a K fragment read feeds two MFMAs and the idle
// tail of a window's last block is at most an eighth of it; 32 below, where T = 144 would leave a quarter of 64-query waves idle.
static inline int fl_win_qb(int T) { return T >= 512 ? 2 : 1; }

extern "C" int vdx_flash_attn_win_f16(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                                      void* out, int ldo, int n_img, int hh, int ww, int ny, int nx,
                                      int heads, float scale, vdx_stream_t stream) {
    VDX_CHECK(q && k && v && out, "flash_attn_win: null pointer");
    VDX_CHECK(n_img > 0 && hh > 0 && ww > 0 && ny > 0 && nx > 0 && heads > 0, "flash_attn_win: empty problem");
    VDX_CHECK(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "flash_attn_win: leading dims must be multiples of 8");
    VDX_CHECK(hh % ny == 0 && ww % nx == 0, "flash_attn_win: the %d x %d grid does not divide the %d x %d tokens", ny, nx, hh, ww);
    VDX_CHECK(ny > 1 || nx > 1, "flash_attn_win: a 1 x 1 grid is the plain attention (vdx_flash_attn_rows_f16)");
    VDX_CHECK((long long)n_img * hh * ww < (1ll << 30), "flash_attn_win: %lld rows are more than 2^30", (long long)n_img * hh * ww);
    FlWinP p;
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.out = (f16*)out;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    const int th = hh / ny, tw = ww / nx;
    VDX_CHECK((long long)th * tw <= (1 << 20), "flash_attn_win: windows of %d x %d tokens are more than 2^20", th, tw);
    p.ww = ww; p.tw = tw; p.T = th * tw;
    p.nx = nx; p.ny = ny; p.heads = heads;
    p.img_rows = hh * ww; p.band_rows = th * ww;
    p.dx = 64 % tw; p.rstep = (64 / tw) * ww + p.dx; p.wrap = ww - tw;
    p.inv_tw = 1.0f / (float)tw;
    p.c = scale * 1.44269504088896341f;
    const int qbs = fl_win_qb(p.T);
    const long long npairs = (long long)n_img * ny * nx * heads;
    p.nqb = (p.T + 128 * qbs - 1) / (128 * qbs);
    const long long blocks = (npairs + 7) / 8 * 8 * p.nqb;
    VDX_CHECK(blocks < (1ll << 31), "flash_attn_win: grid too large");
    p.npairs = (int)npairs;
    if (qbs == 2) hipLaunchKernelGGL((flash_attn_win_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((flash_attn_win_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return vdx_launch_status("vdx_flash_attn_win_f16");
}
