// lora.hip — LoRA adapters merged into a weight in the diffusers layout, before the loader packs it (diffusers' load_lora_weights /
// set_adapters / fuse_lora and peft's merge, unpinned; no reference counterpart: the reference loads one checkpoint and never
// changes it.  vdx/lora.py reads the adapters, tests/lora_ref.py restates the expression).
//
// lora_merge.  W fp16 [n_out][n_in] (conv weights flattened over their input axes), per adapter a = 0..A-1 (1 <= A <= 8) up_a fp32
// [n_out][R_a], down_a fp32 [R_a][n_in] (1 <= R_a <= 512) and the scalar s_a.  Per element, every product and every sum rounded to
// fp32 on its own (the file is compiled without mul + add contraction):
//
//   acc_a = 0.0f;  for r = 0 .. R_a-1 ascending:  acc_a = acc_a + (up_a[o][r] * down_a[r][i])
//   d     = 0.0f;  for a = 0 .. A-1  ascending:   d = d + (s_a * acc_a)
//   out[o][i] = fp16_rn( fp32(W[o][i]) + d )
//
// VALU fp32 on purpose, not MFMA.  The merge runs once per change of adapters and is bound by reading and writing W (2 R flops per
// 4 bytes of W: far below the VALU's rate at every rank a file holds); an MFMA would sum a rank block in an order of its own and in
// one rounding per block.  The fixed order above is what lets a torch loop pin the result bit for bit, and what makes every rank of
// a job merge the same bits for itself, with no collective.
//
// A block of 256 lanes owns a tile of LM_TO = 32 rows by LM_TI = 256 columns of W; a lane owns 4 rows by 8 consecutive columns, 32
// sums in registers, and reads its elements of W once, at the start, so those loads fly under the staging.  The tile's `up` rows
// and `down` columns go through LDS in chunks of LM_RC = 32 ranks: up [32][32] and down [32][256] fp32, 36 KB.  A wave holds two
// row groups, so an `up` read is two addresses, broadcast.  A lane's 8 `down` columns are stored as two 16-byte slots 512 bytes
// apart (column c at slot (c / 4) % 2, word (c / 8) 4 + c % 4), so the 16 lanes of a ds_read_b128 group read 256 consecutive
// bytes: no bank conflict; the staging writes whole slots.  Along n_in every global access is 16 bytes where n_in % 8 == 0 and W,
// out and every `down` are 16-byte aligned, 8 bytes where n_in % 4 == 0 (8-byte aligned), else one element; `up` is read one
// element a lane, consecutive lanes along the rank.  Tail tiles are predicated: a row or column outside W is staged as zero and
// never stored; a short last chunk runs its own length, so no term is added that the expression does not have.  No atomics, no
// reduction across lanes and no index that depends on a value: a NaN or inf in W, up or down stays in the elements the expression
// gives it, and the bits are the same on every run.  `out` may be W: a lane reads its own elements before it writes them and no
// other lane touches them.
#include "vdx_common.h"

#pragma clang fp contract(off)

#define LM_THREADS 256
#define LM_TO 32
#define LM_TI 256
#define LM_RC 32
#define LM_MAX_A 8
#define LM_MAX_R 512

struct LmAdapters {
    const float* up[LM_MAX_A];
    const float* down[LM_MAX_A];
    int R[LM_MAX_A];
    float s[LM_MAX_A];
};

template <int N>
struct LmF32;
template <>
struct LmF32<4> {
    typedef f32x4 type;
};
template <>
struct LmF32<2> {
    typedef float type __attribute__((ext_vector_type(2)));
};

// a lane's 8 elements of one row, `p` at the first of them, column i of n_in: V elements per access, whole accesses inside the row
template <int V>
__device__ __forceinline__ void lm_load_row(const f16* p, int i, int n_in, f16 (&w)[8]) {
    if (V == 8) {
        if (i < n_in) {
            const f16x8 v = *(const f16x8*)p;
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = v[k];
        }
    } else if (V == 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (i + 4 * h < n_in) {
                const f16x4 v = *(const f16x4*)(p + 4 * h);
#pragma unroll
                for (int k = 0; k < 4; ++k) w[4 * h + k] = v[k];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i + k < n_in) w[k] = p[k];
        }
    }
}

template <int V>
__device__ __forceinline__ void lm_store_row(f16* p, int i, int n_in, const f16 (&w)[8]) {
    if (V == 8) {
        if (i < n_in) {
            f16x8 v;
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = w[k];
            *(f16x8*)p = v;
        }
    } else if (V == 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (i + 4 * h < n_in) {
                f16x4 v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = w[4 * h + k];
                *(f16x4*)(p + 4 * h) = v;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (i + k < n_in) p[k] = w[k];
        }
    }
}

// word of column c (0 .. LM_TI) in a row of the `down` image: a lane's columns 8 tx .. 8 tx + 7 are words 4 tx .. and 128 + 4 tx ..
__device__ __forceinline__ int lm_word(int c) { return ((c >> 2) & 1) * (LM_TI / 2) + (c >> 3) * 4 + (c & 3); }

// V: elements of W per global access (8, 4 or 1); `down` is staged V / 2 floats per access (4, 2) or one
template <int V>
__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(const f16* W, LmAdapters ad, int A, int n_out, int n_in, unsigned tiles_i,
                                                                f16* out) {
    __shared__ __attribute__((aligned(16))) float up_s[LM_TO][LM_RC];
    __shared__ __attribute__((aligned(16))) float down_s[LM_RC][LM_TI];
    constexpr int DV = V == 8 ? 4 : (V == 4 ? 2 : 1);
    const int tid = (int)threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int o0 = (int)(blockIdx.x / tiles_i) * LM_TO, i0 = (int)(blockIdx.x % tiles_i) * LM_TI;       // < n_out, < n_in: no overflow
    const int ol = o0 + ty * 4, il = i0 + tx * 8;                          // the lane's first row and column

    f16 w[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < 8; ++k) w[j][k] = (f16)0.0f;
        if (ol + j < n_out && il < n_in) lm_load_row<V>(W + (size_t)(ol + j) * n_in + il, il, n_in, w[j]);
    }

    float d[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) d[j][k] = 0.0f;

    for (int a = 0; a < A; ++a) {
        const float* const up = ad.up[a];
        const float* const down = ad.down[a];
        const int R = ad.R[a];
        const float s = ad.s[a];
        float acc[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[j][k] = 0.0f;
        for (int r0 = 0; r0 < R; r0 += LM_RC) {
            const int rc = R - r0 < LM_RC ? R - r0 : LM_RC;
            __syncthreads();                                               // the chunk before has been read
            for (int e = tid; e < LM_TO * LM_RC; e += LM_THREADS) {
                const int row = e / LM_RC, r = e % LM_RC;
                float v = 0.0f;
                if (o0 + row < n_out && r < rc) v = up[(size_t)(o0 + row) * R + r0 + r];
                up_s[row][r] = v;
            }
            for (int e = tid; e < LM_RC * (LM_TI / DV); e += LM_THREADS) {
                const int r = e / (LM_TI / DV), c = (e % (LM_TI / DV)) * DV;
                float* const dst = &down_s[r][lm_word(c)];
                const bool in = r < rc && i0 + c < n_in;                   // n_in % (2 DV) == 0 on the vector paths: whole accesses
                const float* const src = down + (size_t)(r0 + (in ? r : 0)) * n_in + (in ? i0 + c : 0);
                if (DV == 1) {
                    *dst = in ? *src : 0.0f;
                } else {
                    typedef typename LmF32<(DV == 1 ? 2 : DV)>::type vec;
                    vec v = {};
                    if (in) v = *(const vec*)src;
                    *(vec*)dst = v;
                }
            }
            __syncthreads();
            for (int r = 0; r < rc; ++r) {
                const f32x4 lo = *(const f32x4*)&down_s[r][4 * tx], hi = *(const f32x4*)&down_s[r][LM_TI / 2 + 4 * tx];
                const float dn[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float u = up_s[ty * 4 + j][r];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float t = u * dn[k];
                        acc[j][k] = acc[j][k] + t;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float t = s * acc[j][k];
                d[j][k] = d[j][k] + t;
            }
    }

#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (ol + j < n_out && il < n_in) {
            f16 y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] = (f16)((float)w[j][k] + d[j][k]);
            lm_store_row<V>(out + (size_t)(ol + j) * n_in + il, il, n_in, y);
        }
    }
}

extern "C" int vdx_lora_merge_f16(const void* W, int n_out, int n_in, int A, const float* const* up, const float* const* down,
                                  const int32_t* rank, const float* scale, void* out, vdx_stream_t stream) {
    VDX_CHECK(W && out && up && down && rank && scale, "lora_merge: null pointer");
    VDX_CHECK(A >= 1 && A <= LM_MAX_A, "lora_merge: %d adapters (1 to %d)", A, LM_MAX_A);
    VDX_CHECK(n_out >= 1 && n_in >= 1, "lora_merge: n_out=%d n_in=%d (each at least 1)", n_out, n_in);
    VDX_CHECK(n_out <= 0x7fffffff - LM_TO && n_in <= 0x7fffffff - LM_TI, "lora_merge: n_out=%d n_in=%d: a tile's last row or column passes 2^31", n_out, n_in);
    LmAdapters ad;
    bool a16 = (size_t)W % 16 == 0 && (size_t)out % 16 == 0, a8 = (size_t)W % 8 == 0 && (size_t)out % 8 == 0;
    for (int a = 0; a < LM_MAX_A; ++a) {
        const bool on = a < A;
        ad.up[a] = on ? up[a] : nullptr;
        ad.down[a] = on ? down[a] : nullptr;
        ad.R[a] = on ? rank[a] : 0;
        ad.s[a] = on ? scale[a] : 0.0f;
        if (!on) continue;
        VDX_CHECK(ad.up[a] && ad.down[a], "lora_merge: adapter %d: null pointer", a);
        VDX_CHECK(ad.R[a] >= 1 && ad.R[a] <= LM_MAX_R, "lora_merge: adapter %d: rank %d (1 to %d)", a, ad.R[a], LM_MAX_R);
        VDX_CHECK(ad.s[a] == ad.s[a] && ad.s[a] - ad.s[a] == 0.0f, "lora_merge: adapter %d: the scale is not finite", a);
        VDX_CHECK((size_t)ad.up[a] % 4 == 0 && (size_t)ad.down[a] % 4 == 0, "lora_merge: adapter %d: up and down must be 4-byte aligned", a);
        a16 = a16 && (size_t)ad.down[a] % 16 == 0;
        a8 = a8 && (size_t)ad.down[a] % 8 == 0;
    }
    VDX_CHECK((size_t)W % 2 == 0 && (size_t)out % 2 == 0, "lora_merge: W and out must be 2-byte aligned");
    const int V = (n_in % 8 == 0 && a16) ? 8 : ((n_in % 4 == 0 && a8) ? 4 : 1);
    const unsigned long long tiles_i = ((unsigned long long)n_in + LM_TI - 1) / LM_TI, tiles_o = ((unsigned long long)n_out + LM_TO - 1) / LM_TO;
    VDX_CHECK(tiles_i * tiles_o <= 0x7fffffffull, "lora_merge: %llu tiles, at most 2^31 - 1", tiles_i * tiles_o);
    const dim3 grid((unsigned)(tiles_i * tiles_o)), block(LM_THREADS);
    if (V == 8)
        hipLaunchKernelGGL(lora_merge_kernel<8>, grid, block, 0, (hipStream_t)stream, (const f16*)W, ad, A, n_out, n_in, (unsigned)tiles_i, (f16*)out);
    else if (V == 4)
        hipLaunchKernelGGL(lora_merge_kernel<4>, grid, block, 0, (hipStream_t)stream, (const f16*)W, ad, A, n_out, n_in, (unsigned)tiles_i, (f16*)out);
    else
        hipLaunchKernelGGL(lora_merge_kernel<1>, grid, block, 0, (hipStream_t)stream, (const f16*)W, ad, A, n_out, n_in, (unsigned)tiles_i, (f16*)out);
    return vdx_launch_status("vdx_lora_merge_f16");
}
