// prompt.hip — prompt emphasis on the text encoder's output: A1111's `(text:1.3)` weights with mean restoration (the web UI's
// "Original" emphasis: multiply every token's hidden state by its weight, then scale the sequence so that its mean is what it was;
// unpinned, no reference counterpart: the reference encodes one plain prompt.  vdx/prompt.py parses and chunks the text,
// tests/prompt_ref.py restates the expression).
//
// prompt_weight.  z fp16 [n_seq][n_tok][D], the CLIP last hidden state, one sequence per (text, 75-token chunk); w fp32
// [n_seq][n_tok].  Per sequence s, every product rounded on its own (the file is compiled without mul + add contraction, and each
// fp32 -> fp16 conversion is `rn16`, a rounding of its own):
//
//   y[t][d]   = fp16( fp32(z[t][d]) * w[t] )
//   m0 = sum z,  m1 = sum y         fp64 sums over the sequence's n_tok D elements, in the order stated below
//   r         = fp32( m0 / m1 )     the quotient in fp64
//   out[t][d] = fp16( fp32(y[t][d]) * r )
//
// One block of PW_THREADS lanes owns one sequence: one launch, no atomics, no hand-off between blocks.  The block passes twice
// over its n_tok D <= 77 x 1024 halves (154 KB: the second pass reads what the first left in cache): pass 1 forms the two sums,
// pass 2 forms y again and stores out.  Nothing is stored before every lane of the block has finished pass 1 and a lane reads its
// own elements before it writes them, so `out` may be z.
//
// The order of the sums.  With V elements per access (below), lane l owns the accesses a = l, l + PW_THREADS, l + 2 PW_THREADS, ...
// of the sequence's n_tok D / V, and adds their elements to its two fp64 partials access by access, ascending, element by element,
// ascending.  The PW_THREADS partials then meet in LDS in a binary tree: for h = PW_THREADS / 2, ..., 1: p[l] = p[l] + p[l + h] for
// l < h.  (Where |z| <= 64 the sums of at most 77 x 1024 fp16 values are exact in fp64, 47 bits, and the order does not show.)
//
// V = 8 (16 bytes a lane) where D % 8 == 0 and z and out are 16-byte aligned, V = 4 (8 bytes) where D % 4 == 0 and they are 8-byte
// aligned, else V = 1 (2 bytes).  D % V == 0, so an access lies inside one token and takes one weight.  No branch on data: m1 = 0,
// a NaN or an infinity give what the lines above give, in that sequence and no other.
#include "step_chains.h"

#pragma clang fp contract(off)

#define PW_THREADS 1024
#define PW_MAX_TOK 77

template <int V>
struct PwVec;
template <>
struct PwVec<8> {
    typedef f16x8 type;
};
template <>
struct PwVec<4> {
    typedef f16x4 type;
};

template <int V>
__device__ __forceinline__ void pw_load(const f16* p, f16 (&v)[V]) {
    if constexpr (V == 1) {
        v[0] = *p;
    } else {
        const typename PwVec<V>::type x = *(const typename PwVec<V>::type*)p;
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = x[k];
    }
}

template <int V>
__device__ __forceinline__ void pw_store(f16* p, const f16 (&v)[V]) {
    if constexpr (V == 1) {
        *p = v[0];
    } else {
        typename PwVec<V>::type x;
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] = v[k];
        *(typename PwVec<V>::type*)p = x;
    }
}

template <int V>
__global__ __launch_bounds__(PW_THREADS) void prompt_weight_kernel(const f16* z, const float* w, f16* out, int n_tok, int D) {
    __shared__ double p0[PW_THREADS], p1[PW_THREADS];
    __shared__ float ws[PW_MAX_TOK];
    const int tid = (int)threadIdx.x;
    const int n = n_tok * D;                                       // <= 77 x 2^20 (host check): no overflow
    const size_t base = (size_t)blockIdx.x * (size_t)n;
    const f16* const zs = z + base;
    f16* const os = out + base;
    if (tid < n_tok) ws[tid] = w[(size_t)blockIdx.x * n_tok + tid];
    __syncthreads();

    double m0 = 0.0, m1 = 0.0;
    for (int e = tid * V; e < n; e += PW_THREADS * V) {
        f16 v[V];
        pw_load<V>(zs + e, v);
        const float wt = ws[e / D];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const f16 y = rn16(__fmul_rn((float)v[k], wt));
            m0 = m0 + (double)v[k];
            m1 = m1 + (double)y;
        }
    }
    p0[tid] = m0;
    p1[tid] = m1;
    __syncthreads();
    for (int h = PW_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            p0[tid] = p0[tid] + p0[tid + h];
            p1[tid] = p1[tid] + p1[tid + h];
        }
        __syncthreads();
    }
    const float r = (float)(p0[0] / p1[0]);                         // every lane has finished pass 1: the barrier above

    for (int e = tid * V; e < n; e += PW_THREADS * V) {
        f16 v[V], o[V];
        pw_load<V>(zs + e, v);
        const float wt = ws[e / D];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const f16 y = rn16(__fmul_rn((float)v[k], wt));
            o[k] = rn16(__fmul_rn((float)y, r));
        }
        pw_store<V>(os + e, o);
    }
}

extern "C" int vdx_prompt_weight_f16(const void* z, const float* w, void* out, int n_seq, int n_tok, int D, vdx_stream_t stream) {
    VDX_CHECK(z && w && out, "prompt_weight: null pointer");
    VDX_CHECK(n_seq >= 1 && n_seq <= 0x7fffffff / PW_MAX_TOK, "prompt_weight: n_seq=%d (at least 1)", n_seq);
    VDX_CHECK(n_tok >= 1 && n_tok <= PW_MAX_TOK, "prompt_weight: n_tok=%d (1 to %d)", n_tok, PW_MAX_TOK);
    VDX_CHECK(D >= 1 && D <= (1 << 20), "prompt_weight: D=%d (1 to 2^20)", D);
    VDX_CHECK((size_t)z % 2 == 0 && (size_t)out % 2 == 0 && (size_t)w % 4 == 0, "prompt_weight: z and out must be 2-byte, w 4-byte aligned");
    const bool a16 = (size_t)z % 16 == 0 && (size_t)out % 16 == 0, a8 = (size_t)z % 8 == 0 && (size_t)out % 8 == 0;
    const int V = (D % 8 == 0 && a16) ? 8 : ((D % 4 == 0 && a8) ? 4 : 1);
    const dim3 grid((unsigned)n_seq), block(PW_THREADS);
    if (V == 8)
        hipLaunchKernelGGL(prompt_weight_kernel<8>, grid, block, 0, (hipStream_t)stream, (const f16*)z, w, (f16*)out, n_tok, D);
    else if (V == 4)
        hipLaunchKernelGGL(prompt_weight_kernel<4>, grid, block, 0, (hipStream_t)stream, (const f16*)z, w, (f16*)out, n_tok, D);
    else
        hipLaunchKernelGGL(prompt_weight_kernel<1>, grid, block, 0, (hipStream_t)stream, (const f16*)z, w, (f16*)out, n_tok, D);
    return vdx_launch_status("vdx_prompt_weight_f16");
}
