// travel.hip — prompt travel: per-frame text for the UNet's cross-attentions (no reference counterpart: the reference encodes one
// prompt per job; AnimateDiff-Evolved's batch prompt schedule is the idea, restated in vdx/travel.py and tests/travel_ref.py).
//
// text_travel.  A job holds n_keys CLIP embeddings keys[k] (N, D) and, per clip frame t, a plan row (lo[t], hi[t], w[t]) built on
// the host (vdx/travel.py `travel_plan`).  One launch writes one window's UNet text out (2, L, N, D):
//
//   out[0][f] = uncond                                                                    every frame, bit for bit
//   out[1][f] = keys[lo[t]]                                     where w[t] == 0 or lo[t] == hi[t]: a select, never 0 . b
//             = fp16( fp32( fp32(1 - w[t]) . fp32(a) ) + fp32( w[t] . fp32(b) ) )         a = keys[lo[t]], b = keys[hi[t]]
//   t = s + f d, and with `ring` t - T where that is >= T (one compare and one subtract, as cfg_input_loop takes its frames)
//
// The file is compiled without mul + add contraction: both products and the sum are rounded to fp32 on their own, which is what
// the torch restatement evaluates.  lo and hi come from device memory and are clamped to [0, n_keys) as integers before they
// index anything (the host checks them too), t to [0, T).  A NaN or inf in a key stays in the elements that read that key: no
// branch or index depends on a key's values.  A block owns one (item, frame) and a slice of its N D elements: 16 bytes per lane
// where D % 8 == 0 (N D is then a multiple of 8 and every row of every tensor 16-byte aligned), else one element per lane.  No
// atomics, no reduction: the same bits on every run.
//
// pack_kv.  packing.pack_k5_kv as one launch: the text keys k_rows [n_items text_pad][inner] and the transposed values vt
// [inner][n_items text_pad] of n_items K/V items -> K5's fragment blobs [n_items][heads][3 . 4096] fp16 (csrc/xattn.hip):
//
//   unit 0, 1 (5120 + 5120 elements)   K at (((kt 4 + j) 4 + q4) 16 + n16) 4 + e  = k_rows[item text_pad + kt 16 + n16][64 h + 16 j + 4 q4 + e]
//                                      V at 5120 + (((kt 4 + dt) 4 + q4) 16 + n16) 4 + e = vt[64 h + 16 dt + n16][item text_pad + kt 16 + 4 q4 + e]
//   the rest up to 3 . 4096            zero
//
// A pure permutation whose contiguous runs are the fragments' 4 elements (e): 8 bytes of a key row for K, 8 bytes of a vt row for
// V.  A lane owns 16 bytes of the output — the runs of n16 = 2 n8 and 2 n8 + 1 — which it fills with two 8-byte loads and stores
// with one 16-byte store; consecutive lanes store consecutive 16 bytes.  On the read side a wave's 64 lanes cover, for K, 64
// contiguous bytes of each of 16 key rows (the block's next wave the other 64 of the same 128-byte lines), for V 32 contiguous
// bytes of each of 32 vt rows (the rest of those lines in the block's next iterations): every line is fetched from HBM once and
// its other reads hit L2, so going through LDS to widen the loads to 16 bytes would add a barrier and save no HBM byte.  (A blob
// is 24 KB per head, 3.9 MB at 32 items: the launch is the cost, not the bytes.)  Every index is a function of the block's and the
// lane's position only.  No atomics.
#include "vdx_common.h"

#define TV_THREADS 256

// fp16(fp32(w1 a) + fp32(wt b)).  The products are kept out of the compiler's sight before they are added (csrc/freeu.hip: folded
// into a mixed-precision fma with a +0 addend, a -0 product came out as +0).
__device__ __forceinline__ f16 tv_blend(f16 a, f16 b, float w1, float wt) {
    float pa = w1 * (float)a, pb = wt * (float)b;
    asm volatile("" : "+v"(pa), "+v"(pb));
    return (f16)(pa + pb);
}

template <bool VEC>
__global__ __launch_bounds__(TV_THREADS) void text_travel_kernel(const f16* keys, int n_keys, const f16* uncond, const int* lo,
                                                                 const int* hi, const float* w, int T, int s, int L, int d, int ring,
                                                                 size_t nd, f16* out) {
    const int item = blockIdx.y / L, f = blockIdx.y - item * L;
    const size_t per = VEC ? nd / 8 : nd;
    const size_t i = (size_t)blockIdx.x * TV_THREADS + threadIdx.x;
    if (i >= per) return;
    f16* const o = out + ((size_t)item * L + f) * nd;
    if (item == 0) {
        if (VEC) ((f16x8*)o)[i] = ((const f16x8*)uncond)[i];
        else o[i] = uncond[i];
        return;
    }
    int t = s + f * d;
    if (ring && t >= T) t -= T;
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    int a_i = lo[t], b_i = hi[t];
    a_i = a_i < 0 ? 0 : (a_i >= n_keys ? n_keys - 1 : a_i);
    b_i = b_i < 0 ? 0 : (b_i >= n_keys ? n_keys - 1 : b_i);
    const float wt = w[t];
    const float w1 = 1.0f - wt;
    const bool keep = wt == 0.0f || a_i == b_i;
    const f16* const a = keys + (size_t)a_i * nd;
    const f16* const b = keys + (size_t)b_i * nd;
    if (VEC) {
        const f16x8 va = ((const f16x8*)a)[i];
        f16x8 r = va;
        if (!keep) {
            const f16x8 vb = ((const f16x8*)b)[i];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                r[k] = tv_blend(va[k], vb[k], w1, wt);
            }
        }
        ((f16x8*)o)[i] = r;
    } else {
        const f16 va = a[i];
        f16 r = va;
        if (!keep) {
            r = tv_blend(va, b[i], w1, wt);
        }
        o[i] = r;
    }
}

extern "C" int vdx_text_travel_f16(const void* keys, int n_keys, const void* uncond, const int32_t* lo, const int32_t* hi,
                                   const float* w, int T, int s, int L, int d, int ring, int N, int D, void* out,
                                   vdx_stream_t stream) {
    VDX_CHECK(keys && uncond && lo && hi && w && out, "text_travel: null pointer");
    VDX_CHECK(n_keys >= 1 && T >= 1 && N >= 1 && D >= 1, "text_travel: n_keys=%d T=%d N=%d D=%d (each at least 1)", n_keys, T, N, D);
    VDX_CHECK(L >= 1 && d >= 1 && s >= 0 && s < T, "text_travel: bad window start %d, length %d, stride %d of %d frames", s, L, d, T);
    const long long last = (long long)s + (long long)(L - 1) * d;
    VDX_CHECK(ring ? last < 2ll * T : last < T, "text_travel: window (%d, %d, %d)%s leaves the %d frames", s, L, d, ring ? " on the ring" : "", T);
    VDX_CHECK((long long)N * D <= 0x7fffffffll && 2ll * L <= 65535, "text_travel: N D = %lld elements, 2 L = %d rows", (long long)N * D, 2 * L);
    const bool vec = D % 8 == 0;
    VDX_CHECK(!vec || ((size_t)keys % 16 == 0 && (size_t)uncond % 16 == 0 && (size_t)out % 16 == 0),
              "text_travel: keys, uncond and out must be 16-byte aligned");
    const size_t nd = (size_t)N * D, per = vec ? nd / 8 : nd;
    const dim3 grid((unsigned)((per + TV_THREADS - 1) / TV_THREADS), (unsigned)(2 * L));
    if (vec)
        hipLaunchKernelGGL(text_travel_kernel<true>, grid, dim3(TV_THREADS), 0, (hipStream_t)stream, (const f16*)keys, n_keys, (const f16*)uncond,
                           lo, hi, w, T, s, L, d, ring, nd, (f16*)out);
    else
        hipLaunchKernelGGL(text_travel_kernel<false>, grid, dim3(TV_THREADS), 0, (hipStream_t)stream, (const f16*)keys, n_keys, (const f16*)uncond,
                           lo, hi, w, T, s, L, d, ring, nd, (f16*)out);
    return vdx_launch_status("vdx_text_travel_f16");
}

#define PK_UNIT 4096                     // elements of one of K5's 8 KB units
#define PK_HALF 5120                     // elements of K (and of V) per head: 5 key tiles x 4 x 4 x 16 x 4
#define PK_KEYS 80                       // key slots of a blob: 16 x K5's five key tiles

__global__ __launch_bounds__(TV_THREADS) void pack_kv_kernel(const f16* k, size_t ldk, const f16* vt, size_t ldvt, int heads, int text_pad,
                                                             f16* out) {
    const int item = blockIdx.x / heads, h = blockIdx.x - item * heads;
    f16* const o = out + (size_t)blockIdx.x * (3 * PK_UNIT);
    const size_t col0 = (size_t)item * text_pad;                          // the item's first key: a row of k, a column of vt
    for (int c = threadIdx.x; c < 3 * PK_UNIT / 8; c += TV_THREADS) {
        f16x4 r0 = {0, 0, 0, 0}, r1 = r0;
        if (c < 2 * PK_HALF / 8) {
            const bool isv = c >= PK_HALF / 8;
            const int cc = isv ? c - PK_HALF / 8 : c;
            const int n8 = cc & 7, q4 = (cc >> 3) & 3, j = (cc >> 5) & 3, kt = cc >> 7;
            if (!isv) {
                const f16* const p = k + (col0 + kt * 16 + 2 * n8) * ldk + 64 * h + 16 * j + 4 * q4;
                r0 = *(const f16x4*)p, r1 = *(const f16x4*)(p + ldk);
            } else {
                const f16* const p = vt + (size_t)(64 * h + 16 * j + 2 * n8) * ldvt + col0 + kt * 16 + 4 * q4;
                r0 = *(const f16x4*)p, r1 = *(const f16x4*)(p + ldvt);
            }
        }
        f16x8 v;
        v[0] = r0[0], v[1] = r0[1], v[2] = r0[2], v[3] = r0[3], v[4] = r1[0], v[5] = r1[1], v[6] = r1[2], v[7] = r1[3];
        ((f16x8*)o)[c] = v;
    }
}

extern "C" int vdx_cross_attn_block_pack_kv_f16(const void* k_rows, int ldk, const void* vt, int ldvt, int n_items, int text_pad,
                                                int inner, void* out, vdx_stream_t stream) {
    VDX_CHECK(k_rows && vt && out, "cross_attn_block_pack_kv: null pointer");
    VDX_CHECK(vdx_cross_attn_block_supported(inner, 1), "cross_attn_block_pack_kv: inner=%d not supported (inner 320)", inner);
    VDX_CHECK(vdx_cross_attn_block_kv_bytes(inner) == (size_t)(inner / 64) * 3 * PK_UNIT * sizeof(f16),
              "cross_attn_block_pack_kv: the fused kernel's blob is not [heads][3][4096]");
    VDX_CHECK(n_items >= 1 && text_pad >= PK_KEYS && text_pad % 4 == 0, "cross_attn_block_pack_kv: n_items=%d text_pad=%d (at least %d, a multiple of 4)",
              n_items, text_pad, PK_KEYS);
    VDX_CHECK((long long)n_items * text_pad <= 0x7fffffffll && (long long)n_items * (inner / 64) <= 0x7fffffffll, "cross_attn_block_pack_kv: too many items");
    VDX_CHECK(ldk >= inner && ldk % 4 == 0 && ldvt % 4 == 0 && (long long)ldvt >= (long long)n_items * text_pad,
              "cross_attn_block_pack_kv: bad leading dims %d, %d", ldk, ldvt);
    VDX_CHECK((size_t)k_rows % 8 == 0 && (size_t)vt % 8 == 0 && (size_t)out % 16 == 0, "cross_attn_block_pack_kv: k_rows and vt must be 8-byte, out 16-byte aligned");
    const int heads = inner / 64;
    hipLaunchKernelGGL(pack_kv_kernel, dim3(n_items * heads), dim3(TV_THREADS), 0, (hipStream_t)stream, (const f16*)k_rows, (size_t)ldk,
                       (const f16*)vt, (size_t)ldvt, heads, text_pad, (f16*)out);
    return vdx_launch_status("vdx_cross_attn_block_pack_kv_f16");
}
