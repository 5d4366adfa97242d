// freelong.hip — FreeLong (Lu et al., "FreeLong: Training-Free Long Video Generation with SpectralBlend Temporal Attention",
// NeurIPS 2024, restated and unpinned) on the UNet's rows (no reference counterpart: the reference makes a long clip from
// whole-UNet windows only).  vdx/unet3d.py calls the core in every temporal transformer while `enable_free_long` is set and
// F > window.  tests/freelong_ref.py states the definition, DESIGN.md §29 the reasons for what follows.
//
// temporal_attn_blend_kernel: spectrally blended temporal attention.  For one (b, pixel, head) item with q, k, v the F x 64
//   blocks of vdx_temporal_attn_f16's qkv rows, a radius r and a matrix Lp [F][F]:
//
//     S   = scale Q K^T
//     Zg  = softmax(S) V                        over all F keys
//     Zl  = softmax(S + M) V                    M[t][j] = 0 where |t - j| <= r, else -inf
//     out = fp16( Zl + Lp fp16(Zg - Zl) )       Lp along the frame axis
//
//   Work split.  A block holds FL_IPB(F) whole items, a wave owns 32 consecutive frames of one item: their queries, their rows
//   of Zg, Zl and D = Zg - Zl, and after the blend their output rows.  Everything a wave computes is TRANSPOSED, frames on the
//   lanes: S^T = K Q^T, Z^T = V^T P^T, out^T = D^T Lp^T on v_mfma_f32_32x32x16_f16.  A lane then holds one frame's scores
//   (16 keys per 32-key tile, the other 16 in lane ^ 32) and 32 of its 64 output columns, so both softmaxes' maxima and sums,
//   the normalisation of Z, D, the add of Zl and the final rounding never move a value between lanes but for one xor-32
//   exchange per maximum and sum; S^T's accumulator registers are P^T's B operand as they stand (pi, attn_common.h).
//   Scores.  All ceil(F / 32) score tiles of the wave are held at once (64 fp32 registers at F = 128; the kernel is compiled
//   per tile count), key slots >= F masked to NEG_BIG before the maxima, their k operands zeros.  Two exact two-pass
//   softmaxes read the same registers: the global one under the maximum of all keys, the local one under the maximum of the
//   band's keys (NOT the global maximum: a band far below a distant peak would round to zero in fp16).  P = exp2(..) <= 1 is
//   rounded to fp16 unnormalised, the sums are of the fp32 values, Z is scaled by 1 / sum after the products.  A key tile
//   wholly outside [t0 - r, t0 + 31 + r] costs the local side nothing: no exponentials, no MFMAs.
//   Blend.  Each wave rounds its D rows to fp16 and writes them into the item's LDS image DT[64][FP + 8] (transposed, so that
//   the blend's A operand is one 16-byte read; frames >= F written as zeros).  One barrier.  out^T = D^T Lp^T takes
//   ceil(F / 16) k-steps per 32 columns; Lp^T's B operand is the wave's own 32 rows of Lp, 16 contiguous bytes per lane and
//   k-step straight from global memory (L2: the matrix is shared by every item), issued before the barrier, entries at or past
//   F zeros.  Zl stays in fp32 registers across the barrier.
//   LDS image per item slot, FP = 32 ceil(F / 32): K[F][72] (rows of 64 padded by 16 bytes), VT[64][FP + 8] (v transposed
//   while it is staged: V^T's A operand is one 16-byte read where freenoise.hip gathers eight halfs; columns >= F zeros),
//   DT[64][FP + 8].  58 KB per block at most (F = 32, four items).
//   No atomics and one fixed order: the same bits on every run and for any B and HW.  No index is computed from data: NaN and
//   inf stay inside their (pixel, head).
#include "attn_common.h"

#define FL_THREADS 256
#define FL_WAVES (FL_THREADS / 64)
#define FL_LDK 72                                     // halfs per K row: 64 + 8 of padding

// items of a block: as many as give every wave one 32-frame block (at three blocks the fourth wave idles)
static inline int fl_ipb(int nqb) { return nqb == 1 ? 4 : nqb == 2 ? 2 : 1; }

struct BlendP {
    const f16* qkv;
    f16* out;
    const f16* lp;
    int ldqkv, ldo, B, F, HW, heads, ipb, r, lpvec, ovec;
    float c;
    long long items;
};

template <int NKB>                                    // NKB = ceil(F / 32): key tiles = query blocks of an item
__global__ __launch_bounds__(FL_THREADS) void temporal_attn_blend_kernel(const BlendP p) {
    extern __shared__ __attribute__((aligned(16))) f16 fl_lds[];
    constexpr int FP = 32 * NKB, LDT = FP + 8;
    const int lane = threadIdx.x & 63, r32 = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    const int inner = p.heads * 64;
    const int F = p.F;
    const size_t fstride = (size_t)p.HW * p.ldqkv;     // one frame further, in halfs
    const int slot_halfs = F * FL_LDK + 2 * 64 * LDT;
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // ---- stage the items' k blocks as they lie and their v blocks transposed: HBM -> LDS, once -------------------------------
    for (int slot = 0; slot < p.ipb; ++slot) {
        const long long item = (long long)blockIdx.x * p.ipb + slot;
        if (item >= p.items) break;
        const int head = (int)(item % p.heads);
        const long long bp = item / p.heads;
        const int pix = (int)(bp % p.HW), b = (int)(bp / p.HW);
        const f16* kbase = p.qkv + ((size_t)b * F * p.HW + pix) * p.ldqkv + inner + head * 64;
        f16* Kd = fl_lds + slot * slot_halfs;
        f16* VTd = Kd + F * FL_LDK;
        for (int c = threadIdx.x; c < 2 * FP * 8; c += FL_THREADS) {
            const int c8 = c & 7, row = c >> 3;
            const int m = row >= FP ? 1 : 0, f = row - m * FP;      // m: 0 = k, 1 = v
            if (m == 0) {
                if (f < F) *(f16x8*)(Kd + f * FL_LDK + c8 * 8) = *(const f16x8*)(kbase + (size_t)f * fstride + c8 * 8);
            } else {
                f16x8 v = zero8;
                if (f < F) v = *(const f16x8*)(kbase + (size_t)f * fstride + inner + c8 * 8);
#pragma unroll
                for (int i = 0; i < 8; ++i) VTd[(c8 * 8 + i) * LDT + f] = v[i];
            }
        }
    }
    __syncthreads();

    // ---- a wave per (item, block of 32 frames); NKB * ipb <= 4, so a wave has at most one --------------------------------------
    const int slot = wave / NKB, qblk = wave - slot * NKB;
    const long long item = (long long)blockIdx.x * p.ipb + slot;
    const bool active = slot < p.ipb && item < p.items;            // wave-uniform; idle waves only meet the barrier
    const int head = active ? (int)(item % p.heads) : 0;
    const long long bp = active ? item / p.heads : 0;
    const int pix = (int)(bp % p.HW), b = (int)(bp / p.HW);
    const size_t row0 = (size_t)b * F * p.HW + pix;                 // frame f lives at row0 + f*HW
    const f16* Ks = fl_lds + (active ? slot : 0) * slot_halfs;
    const f16* VTs = Ks + F * FL_LDK;
    f16* DTs = (f16*)VTs + 64 * LDT;
    const int qf0 = qblk * 32, t = qf0 + r32;                       // this lane's frame
    const int nks = (F + 15) >> 4;                                  // k-steps of 16 frames that hold a frame of the clip

    f32x16 zl[2];                                                   // Zl^T: lane = frame t, register j of [db] = column
    f16x8 lpf[2 * NKB];                                             //   32 db + 8 (j >> 2) + 4 h + (j & 3)
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int j = 0; j < 16; ++j) zl[db][j] = 0.f;

    if (active) {
        // B operand of S^T = K.Q^T: lane = query frame, from HBM (each q row belongs to one wave)
        f16x8 qf[4];
        {
            const f16* qsrc = p.qkv + (row0 + (size_t)(t < F ? t : 0) * p.HW) * p.ldqkv + head * 64 + 8 * h;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[ks] = t < F ? *(const f16x8*)(qsrc + 16 * ks) : zero8;
        }
        // every score tile of these 32 queries; A operand: K rows fed through pi, slots >= F zeros
        f32x16 s[NKB];
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const int kk = 32 * kb + pi_row(r32);
            const bool ok = kb < NKB - 1 || kk < F;                 // F > 32 (NKB - 1): only the last tile has slots >= F
            const f16* ksrc = Ks + (ok ? kk : 0) * FL_LDK + 8 * h;
#pragma unroll
            for (int j = 0; j < 16; ++j) s[kb][j] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const f16x8 ld = *(const f16x8*)(ksrc + 16 * ks);
                s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ok ? ld : zero8, qf[ks], s[kb], 0, 0, 0);
            }
        }
        // both maxima of row t: all keys < F, and the band's (never empty for t < F: r >= 1 holds t itself)
        // |key - t| <= r as one unsigned compare: (key - t + r) <= 2 r
        float mg = NEG_BIG, ml = NEG_BIG;
        const unsigned r2 = 2u * (unsigned)p.r;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            // wave-uniform: the band of some query of this wave meets the tile
            const bool reach = !(32 * kb + 31 < qf0 - p.r || 32 * kb > qf0 + 31 + p.r);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int key = 32 * kb + acc_key(j, h);
                if (kb == NKB - 1 && key >= F) s[kb][j] = NEG_BIG;
                mg = fmaxf(mg, s[kb][j]);
                if (reach) ml = fmaxf(ml, (unsigned)(key - t + p.r) <= r2 ? s[kb][j] : NEG_BIG);
            }
        }
        mg = fmaxf(mg, __shfl_xor(mg, 32, 64));
        ml = fmaxf(ml, __shfl_xor(ml, 32, 64));
        const float mgc = mg * p.c, mlc = ml * p.c;
        float rsg = 0.f, rsl = 0.f;
        f32x16 zg[2];
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int j = 0; j < 16; ++j) zg[db][j] = 0.f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const bool two = kb < NKB - 1 || 32 * kb + 16 < F;                    // k-step 1 holds keys 32 kb + 16 ..: all masked otherwise
            // A operand of Z^T = V^T.P^T: lane = column d, eight consecutive keys: one 16-byte read of the transposed image
            f16x8 vf[2][2];
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) vf[db][ks] = *(const f16x8*)(VTs + (32 * db + r32) * LDT + 32 * kb + 16 * ks + 8 * h);
            f16x8 pf[2];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float e = __builtin_amdgcn_exp2f(s[kb][j] * p.c - mgc);
                rsg += e;
                pf[j >> 3][j & 7] = (f16)e;
            }
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                zg[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[db][0], pf[0], zg[db], 0, 0, 0);
                if (two) zg[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[db][1], pf[1], zg[db], 0, 0, 0);
            }
            // the local side: only the tiles the band of some query of this wave reaches (wave-uniform)
            if (32 * kb + 31 < qf0 - p.r || 32 * kb > qf0 + 31 + p.r) continue;
            int tb = t;                                             // opaque copy: the band's lane masks are formed again here, tile
            asm volatile("" : "+v"(tb));                            // by tile, not kept in scalar registers since the maxima
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float e = __builtin_amdgcn_exp2f(s[kb][j] * p.c - mlc);
                const float el = (unsigned)(32 * kb + acc_key(j, h) - tb + p.r) <= r2 ? e : 0.f;
                rsl += el;
                pf[j >> 3][j & 7] = (f16)el;
            }
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                zl[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[db][0], pf[0], zl[db], 0, 0, 0);
                if (two) zl[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[db][1], pf[1], zl[db], 0, 0, 0);
            }
        }
        const float invg = 1.0f / (rsg + __shfl_xor(rsg, 32, 64));
        const float invl = 1.0f / (rsl + __shfl_xor(rsl, 32, 64));
        // D = fp16(Zg - Zl) of frame t into DT[column][t]; frames >= F (a padded query's rows hold no data) as zeros
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                zl[db][j] *= invl;
                const float d = zg[db][j] * invg - zl[db][j];
                DTs[(32 * db + 8 * (j >> 2) + 4 * h + (j & 3)) * LDT + t] = t < F ? (f16)d : (f16)0;
            }
        // B operand of out^T = D^T.Lp^T: lane = output frame t, eight consecutive source frames of row t of Lp; loaded here,
        // where the scores' and Zg's registers are free, and not a moment earlier
        __builtin_amdgcn_sched_barrier(0);
        const f16* lrow = p.lp + (size_t)(t < F ? t : 0) * F + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 2 * NKB; ++ks) {
            lpf[ks] = zero8;
            if (ks >= nks) continue;
            if (p.lpvec) {                                          // F % 8 == 0: a chunk of eight lies wholly below F or not at all
                if (t < F && 16 * ks + 8 * h < F) lpf[ks] = *(const f16x8*)(lrow + 16 * ks);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (t < F && 16 * ks + 8 * h + j < F) lpf[ks][j] = lrow[16 * ks + j];
            }
        }
    }
    __syncthreads();
    if (!active) return;

    // ---- out^T = Zl^T + D^T.Lp^T: k-steps over the source frames in ascending order, one rounding, 8 bytes per store ----------
#pragma unroll
    for (int db = 0; db < 2; ++db) {
        f32x16 o;
#pragma unroll
        for (int j = 0; j < 16; ++j) o[j] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2 * NKB; ++ks) {
            if (ks >= nks) continue;
            const f16x8 df = *(const f16x8*)(DTs + (32 * db + r32) * LDT + 16 * ks + 8 * h);
            o = __builtin_amdgcn_mfma_f32_32x32x16_f16(df, lpf[ks], o, 0, 0, 0);
        }
        if (t >= F) continue;
        f16* dst = p.out + (row0 + (size_t)t * p.HW) * p.ldo + head * 64 + 32 * db + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f16x4 w;
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = (f16)(zl[db][4 * g + i] + o[4 * g + i]);
            if (p.ovec)
                *(f16x4*)(dst + 8 * g) = w;
            else
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[8 * g + i] = w[i];
        }
    }
}

extern "C" int vdx_temporal_attn_blend_f16(const void* qkv, int ldqkv, void* out, int ldo, int B, int F, int HW, int heads,
                                           float scale, int r, const void* lp, vdx_stream_t stream) {
    VDX_CHECK(qkv && out && lp, "temporal_attn_blend: null pointer");
    VDX_CHECK(B > 0 && F > 0 && HW > 0 && heads > 0, "temporal_attn_blend: empty problem");
    VDX_CHECK(F >= 2 && F <= 128, "temporal_attn_blend: F=%d frames outside [2, 128]", F);
    VDX_CHECK(r >= 1, "temporal_attn_blend: band radius r=%d below 1", r);
    VDX_CHECK(ldqkv % 8 == 0 && ldqkv >= 3 * heads * 64 && ldo >= heads * 64, "temporal_attn_blend: bad leading dims");
    VDX_CHECK((size_t)qkv % 16 == 0, "temporal_attn_blend: qkv must be 16-byte aligned");
    VDX_CHECK((size_t)out % 2 == 0 && (size_t)lp % 2 == 0, "temporal_attn_blend: out and lp must be 2-byte aligned");
    const size_t M = (size_t)B * F * HW;
    const char *a = (const char*)qkv, *o = (const char*)out;
    const size_t qbytes = ((M - 1) * ldqkv + 3 * heads * 64) * sizeof(f16), obytes = ((M - 1) * ldo + heads * 64) * sizeof(f16);
    VDX_CHECK(a + qbytes <= o || o + obytes <= a, "temporal_attn_blend: out may not alias qkv");
    BlendP p;
    p.qkv = (const f16*)qkv; p.out = (f16*)out; p.lp = (const f16*)lp; p.ldqkv = ldqkv; p.ldo = ldo;
    p.B = B; p.F = F; p.HW = HW; p.heads = heads;
    p.r = r < F ? r : F;                                            // |t - j| < F: a larger radius is the same band
    p.lpvec = F % 8 == 0 && (size_t)lp % 16 == 0;
    p.ovec = ldo % 4 == 0 && (size_t)out % 8 == 0;
    const int nkb = (F + 31) / 32;
    p.ipb = fl_ipb(nkb);
    p.c = scale * 1.44269504088896341f;
    p.items = (long long)B * HW * heads;
    const long long blocks = (p.items + p.ipb - 1) / p.ipb;
    VDX_CHECK(blocks < (1ll << 31), "temporal_attn_blend: too many items");
    const size_t lds = (size_t)p.ipb * (F * FL_LDK + 2 * 64 * (32 * nkb + 8)) * sizeof(f16);          // 58 KB at most (F = 32)
    const dim3 grid((unsigned)blocks), block(FL_THREADS);
    switch (nkb) {
        case 1: hipLaunchKernelGGL(temporal_attn_blend_kernel<1>, grid, block, lds, (hipStream_t)stream, p); break;
        case 2: hipLaunchKernelGGL(temporal_attn_blend_kernel<2>, grid, block, lds, (hipStream_t)stream, p); break;
        case 3: hipLaunchKernelGGL(temporal_attn_blend_kernel<3>, grid, block, lds, (hipStream_t)stream, p); break;
        default: hipLaunchKernelGGL(temporal_attn_blend_kernel<4>, grid, block, lds, (hipStream_t)stream, p); break;
    }
    return vdx_launch_status("vdx_temporal_attn_blend_f16");
}
