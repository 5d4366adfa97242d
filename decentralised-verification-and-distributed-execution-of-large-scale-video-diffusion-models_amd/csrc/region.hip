// region.hip — regional prompts: the per-pixel blend of a spatial transformer's cross-attention sub-block evaluated once per
// text (no reference counterpart: the reference conditions every pixel on one prompt; "attention couple" / regional conditioning
// is the idea, restated in vdx/region.py and tests/region_ref.py).
//
// region_blend.  A window of L frames of S pixels holds, per text j = 0..n_in-1, the rows sub_j [L S][C] of
// `t + attn2(norm2(t), text_j)`; the level's table w [T][S][n_in] fp32 (vdx/region.py `region_plan`) gives each clip frame's
// pixel its weights.  Row (f, p) of the window is the clip frame tau = s + f d (with `ring` tau - T where that is >= T):
//
//   out[row] = sub_j[row]                                      where w[tau][p][j] == 1.0f (the first such j): a select, its bits
//            = fp16( (( t_a + t_b ) + t_c ) ... )              t_j = fp32( w[tau][p][j] . fp32(sub_j[row]) ), ascending j over the
//                                                              j with w != 0 only; the first such term starts the sum
//            = +0                                              where no weight is non-zero (never from `region_plan`: they sum to 1)
//
// The file is compiled without mul + add contraction: every product and every sum is rounded to fp32 on its own, which is what
// the torch restatement evaluates.  A term whose weight is 0 is skipped, not multiplied: its input is not read, and a NaN there
// never reaches the row.  An input the host passes as NULL (a text with no weight on any cell of the window, not launched) is
// skipped whatever the table holds.  A NaN or inf in a weighted input stays in its element: no branch or index depends on an
// input's values.  tau is formed from integers and clamped to [0, T) before it indexes the table.
//
// A block owns whole rows: groups of consecutive rows (about 1024 lanes of work each), never a part of a row, so no row's weights
// are read by two blocks.  A lane owns 16 bytes of one row where C % 8 == 0, 8 bytes where C % 4 == 0, else one element;
// consecutive lanes own consecutive bytes of the group's contiguous rows, so a wave reads 1 KB lines of each input.  A row's weights
// are the same address in every lane that works on the row, so the j loop and the zero / one tests are uniform over a row; a wave
// spans 64 . 8 / C rows (12.8 at C = 320), and only a wave whose rows differ in their zero pattern, along a region's edge,
// diverges.  A lane first reads its row's n_in weights, then issues the loads of every weighted input (up to eight 16-byte loads in
// flight), then sums.  `out` may alias input 0 (or any one input): a lane reads its own elements of every input before it writes
// them.  No atomics, no reduction across lanes: the same bits on every run and for any split of the rows into calls.
#include "vdx_common.h"

#define RB_THREADS 256
#define RB_MAX_IN 8

struct RbInputs {
    const f16* p[RB_MAX_IN];
};

// fp32(acc + fp32(w x)): the product is kept out of the compiler's sight before it is added (csrc/travel.hip tv_blend).
__device__ __forceinline__ float rb_term(float w, f16 x) {
    float t = w * (float)x;
    asm volatile("" : "+v"(t));
    return t;
}

template <int V>
struct RbVec;
template <>
struct RbVec<8> {
    typedef f16x8 type;
};
template <>
struct RbVec<4> {
    typedef f16x4 type;
};

template <int V>
__device__ __forceinline__ void rb_row(const RbInputs& in, int n_in, const float* wrow, size_t e, f16* out) {
    typedef typename RbVec<V>::type vec;
    float w[RB_MAX_IN];
    int one = -1;
#pragma unroll
    for (int j = RB_MAX_IN - 1; j >= 0; --j) {
        w[j] = (j < n_in && in.p[j] != nullptr) ? wrow[j] : 0.0f;
        if (w[j] == 1.0f) one = j;                    // descending: the first such j is kept
    }
    vec x[RB_MAX_IN];
#pragma unroll
    for (int j = 0; j < RB_MAX_IN; ++j) {
        const bool take = one < 0 ? w[j] != 0.0f : j == one;
        if (take) x[j] = ((const vec*)in.p[j])[e];
    }
    vec r = {};
    if (one >= 0) {
#pragma unroll
        for (int j = 0; j < RB_MAX_IN; ++j) {
            if (j == one) r = x[j];
        }
    } else {
        float acc[V];
        bool first = true;
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0.0f;
#pragma unroll
        for (int j = 0; j < RB_MAX_IN; ++j) {
            if (w[j] != 0.0f) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float t = rb_term(w[j], x[j][k]);
                    acc[k] = first ? t : acc[k] + t;
                }
                first = false;
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) r[k] = (f16)acc[k];
    }
    ((vec*)out)[e] = r;
}

// the scalar form of rb_row: one element per lane
__device__ __forceinline__ void rb_row1(const RbInputs& in, int n_in, const float* wrow, size_t e, f16* out) {
    float w[RB_MAX_IN];
    int one = -1;
#pragma unroll
    for (int j = RB_MAX_IN - 1; j >= 0; --j) {
        w[j] = (j < n_in && in.p[j] != nullptr) ? wrow[j] : 0.0f;
        if (w[j] == 1.0f) one = j;
    }
    f16 r = (f16)0.0f;
    if (one >= 0) {
#pragma unroll
        for (int j = 0; j < RB_MAX_IN; ++j) {
            if (j == one) r = in.p[j][e];
        }
    } else {
        float acc = 0.0f;
        bool first = true;
#pragma unroll
        for (int j = 0; j < RB_MAX_IN; ++j) {
            if (w[j] != 0.0f) {
                const float t = rb_term(w[j], in.p[j][e]);
                acc = first ? t : acc + t;
                first = false;
            }
        }
        r = (f16)acc;
    }
    out[e] = r;
}

// V elements per lane, `per_row` = C / V lanes per row.  A block owns whole rows: `rpb` consecutive rows at a time (a row group, about
// RB_GROUP lanes of work; the last group of the image may be shorter), which its 256 lanes walk 16 bytes apart, and the grid walks
// the groups with its stride.  No row is shared between two blocks.
#define RB_GROUP 1024
template <int V>
__global__ __launch_bounds__(RB_THREADS) void region_blend_kernel(RbInputs in, int n_in, const float* table, int T, int s, int d, int ring,
                                                                  int S, unsigned per_row, unsigned rows, unsigned rpb, f16* out) {
    const unsigned groups = (rows + rpb - 1) / rpb;
    for (unsigned g = blockIdx.x; g < groups; g += gridDim.x) {
        const unsigned r0 = g * rpb;
        const unsigned nr = rows - r0 < rpb ? rows - r0 : rpb;
        const unsigned n = nr * per_row;                                 // rows per_row < 2^32 (the launcher checks)
        const size_t e0 = (size_t)r0 * per_row;
        for (unsigned i = threadIdx.x; i < n; i += RB_THREADS) {
            const unsigned row = r0 + i / per_row;
            const int f = (int)(row / (unsigned)S), p = (int)(row - (unsigned)f * (unsigned)S);
            int tau = s + f * d;
            if (ring && tau >= T) tau -= T;
            tau = tau < 0 ? 0 : (tau >= T ? T - 1 : tau);
            const float* const wrow = table + ((size_t)tau * S + p) * n_in;
            if (V == 1) rb_row1(in, n_in, wrow, e0 + i, out);
            else rb_row<(V == 1 ? 4 : V)>(in, n_in, wrow, e0 + i, out);
        }
    }
}

extern "C" int vdx_region_blend_f16(const void* const* in, int n_in, const float* table, int T, int s, int L, int d, int ring, int S,
                                    int C, void* out, vdx_stream_t stream) {
    VDX_CHECK(in && table && out, "region_blend: null pointer");
    VDX_CHECK(n_in >= 1 && n_in <= RB_MAX_IN, "region_blend: %d inputs (1 to %d: the base text and at most %d regions)", n_in, RB_MAX_IN, RB_MAX_IN - 1);
    VDX_CHECK(T >= 1 && S >= 1 && C >= 1, "region_blend: T=%d S=%d C=%d (each at least 1)", T, S, C);
    VDX_CHECK(L >= 1 && d >= 1 && s >= 0 && s < T, "region_blend: bad window start %d, length %d, stride %d of %d frames", s, L, d, T);
    const long long last = (long long)s + (long long)(L - 1) * d;
    VDX_CHECK(ring ? last < 2ll * T : last < T, "region_blend: window (%d, %d, %d)%s leaves the %d frames", s, L, d, ring ? " on the ring" : "", T);
    VDX_CHECK((long long)L * S <= 0x7fffffffll && (long long)T * S <= 0x7fffffffll, "region_blend: L S = %lld, T S = %lld rows", (long long)L * S,
              (long long)T * S);
    const int V = C % 8 == 0 ? 8 : (C % 4 == 0 ? 4 : 1);
    const size_t align = V == 1 ? 2 : (size_t)V * 2;
    RbInputs a;
    int any = 0;
    for (int j = 0; j < RB_MAX_IN; ++j) {
        a.p[j] = j < n_in ? (const f16*)in[j] : nullptr;
        if (a.p[j]) {
            any = 1;
            VDX_CHECK((size_t)a.p[j] % align == 0, "region_blend: input %d must be %zu-byte aligned at C = %d", j, align, C);
        }
    }
    VDX_CHECK(any, "region_blend: every input is NULL");
    VDX_CHECK((size_t)out % align == 0 && (size_t)table % 4 == 0, "region_blend: out must be %zu-byte, the table 4-byte aligned", align);
    const unsigned per_row = (unsigned)(C / V), rows = (unsigned)((long long)L * S);
    VDX_CHECK((unsigned long long)rows * per_row <= 0xffffffffull, "region_blend: %llu lanes of work, at most 2^32 - 1", (unsigned long long)rows * per_row);
    const unsigned rpb = per_row >= RB_GROUP ? 1u : RB_GROUP / per_row;    // whole rows per block and round
    size_t blocks = ((size_t)rows + rpb - 1) / rpb;
    const size_t cap = (size_t)vdx_num_cus() * 16;                 // beyond that a block walks on with the grid's stride
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks), block(RB_THREADS);
    if (V == 8)
        hipLaunchKernelGGL(region_blend_kernel<8>, grid, block, 0, (hipStream_t)stream, a, n_in, table, T, s, d, ring, S, per_row, rows, rpb, (f16*)out);
    else if (V == 4)
        hipLaunchKernelGGL(region_blend_kernel<4>, grid, block, 0, (hipStream_t)stream, a, n_in, table, T, s, d, ring, S, per_row, rows, rpb, (f16*)out);
    else
        hipLaunchKernelGGL(region_blend_kernel<1>, grid, block, 0, (hipStream_t)stream, a, n_in, table, T, s, d, ring, S, per_row, rows, rpb, (f16*)out);
    return vdx_launch_status("vdx_region_blend_f16");
}
