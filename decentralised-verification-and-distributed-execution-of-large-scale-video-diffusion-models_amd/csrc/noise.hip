// noise.hip — the portable seeded noise generator "philox4x32-10/v1" (vdx/noise.py, ops.philox_normal; no reference counterpart:
// the reference draws from torch's stream, fsdp_chunked_coherent.py:180-182).  Opt-in (`DiffuserConfig.seed` / `.noise`); without it
// nothing here runs.  Element i of stream s under seed k is a pure function of (k, s, i): i is the C-order linear index in the LOGICAL
// tensor, whatever box of it a call fills.  tests/noise_ref.py is the definition, op for op:
//
//   bits     Philox4x32-10 (Salmon et al., SC'11): key (k lo, k hi), counter (q lo, q hi, s lo, s hi), q = i >> 2; the block's words
//            x0..x3 serve the elements 4q..4q + 3
//   normals  Box-Muller in fp64 on (x0, x1) -> elements 4q, 4q + 1 and on (x2, x3) -> 4q + 2, 4q + 3:
//            u = (xa + 0.5) 2^-32, r = sqrt(-2 ln u), the angle (xb + 0.5) 2^-32 of a turn, (r cos, r sin);  |n| <= 6.77
//   ln       u = m 2^e by the exponent bits, m in [1/2, 1); m < sqrt(1/2): m = 2m, e = e - 1;  t = (m - 1) / (m + 1), z = t t,
//            ln m = 2t + 2t (z P(z)), P = Horner over 1/3 .. 1/23;  ln u = e LN2 + ln m
//   sin/cos  octant o = xb >> 29, j = xb & (2^29 - 1), odd octants reflect in integers (j = 2^29 - 1 - j);
//            theta = ((j + 0.5) 2^-29) (pi/4);  s = theta + (theta z) S(z), c = 1 + z C(z), z = theta theta (Taylor, degrees 17 / 18);
//            octants 1, 2, 5, 6 swap s and c; the cosine is negative in octants 2..5, the sine in 4..7
//   output   fp32: fp32(n).  fp16: fp16(fp32(fp16(n)) fp32(sigma)): what `base *= sigma` gives a torch fp16 tensor
//
// Every + - * / sqrt is one IEEE fp64 operation rounded on its own: this file is built with -ffp-contract=off, and no math-library
// ln, sin or cos is called (two libraries do not agree to the last bit).  No atomics, no data-dependent address, no state.
//
// Two forms.  Fast: the box's rows start and end on Philox blocks (the logical index of the box's first element and, with more than
// one row, the row length and the logical row pitch are multiples of 4): a lane computes one block and stores its four outputs at
// once, 8 bytes of fp16 or 16 of fp32; a single row may end in a ragged block, stored element by element.  General: a lane per
// output decodes its logical index, computes that block and picks its word pair.  Trailing axes the box covers whole are merged
// into one row on the host, so a frame range of a clip is one row and takes the fast form.  All index arithmetic is 64-bit.
#include <cmath>
#include <cstdint>

#include "vdx_common.h"
#include "noise_common.h"   // the device side: philox4x32_10, noise_ln, noise_cos_sin, noise_box_muller, noise_out

struct noise_args : philox_key {     // seed and stream, low and high words
    uint64_t base;               // logical index of the box's first element
    uint64_t ext[4];             // the box's extents along the axes above the (merged) row, outermost first, padded with 1
    uint64_t pitch[4];           // those axes' logical strides in elements
    uint64_t row;                // the row's length in the box
    uint64_t n;                  // outputs
    float sigma;
};

// logical index of the first element of box row `r`
NOISE_HD uint64_t noise_row_base(uint64_t r, const noise_args& a) {
    const uint64_t i3 = r % a.ext[3];
    r /= a.ext[3];
    const uint64_t i2 = r % a.ext[2];
    r /= a.ext[2];
    const uint64_t i1 = r % a.ext[1];
    const uint64_t i0 = r / a.ext[1];
    return a.base + i0 * a.pitch[0] + i1 * a.pitch[1] + i2 * a.pitch[2] + i3 * a.pitch[3];
}

// fast form: group g is the outputs 4g .. 4g + 3, one Philox block
template <class T>
__global__ __launch_bounds__(256) void noise_block_kernel(T* out, noise_args a) {
    typedef T vec4 __attribute__((ext_vector_type(4)));
    const uint64_t groups = (a.n + 3) >> 2, per_row = (a.row + 3) >> 2, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint64_t r = g / per_row, col = (g - r * per_row) << 2;
        const uint64_t i = noise_row_base(r, a) + col;
        uint32_t x[4];
        philox4x32_10(i >> 2, a, x);
        double n[4];
        noise_box_muller(x[0], x[1], n[0], n[1]);
        noise_box_muller(x[2], x[3], n[2], n[3]);
        const uint64_t o = g << 2;
        if (o + 4 <= a.n) {
            vec4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = noise_out<T>(n[k], a.sigma);
            *(vec4*)(out + o) = v;
        } else {                                                          // the ragged last block of a single row
            for (int k = 0; k < 4; ++k)
                if (o + k < a.n) out[o + k] = noise_out<T>(n[k], a.sigma);
        }
    }
}

// general form: a lane per output
template <class T>
__global__ __launch_bounds__(256) void noise_elem_kernel(T* out, noise_args a) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.n; o += stride) {
        const uint64_t r = o / a.row, col = o - r * a.row;
        const uint64_t i = noise_row_base(r, a) + col;
        uint32_t x[4];
        philox4x32_10(i >> 2, a, x);
        const bool hi = (i & 2) != 0;
        double n0, n1;
        noise_box_muller(hi ? x[2] : x[0], hi ? x[3] : x[1], n0, n1);
        out[o] = noise_out<T>((i & 1) ? n1 : n0, a.sigma);
    }
}

// the host's checks and the merge of whole trailing axes -> the kernel's arguments and its form (1: fast)
static int noise_plan(const char* what, size_t seed, size_t stream, int ndim, const size_t* shape, const size_t* start,
                      const size_t* extent, float sigma, noise_args& a, int& fast) {
    VDX_CHECK(ndim >= 1 && ndim <= 5 && shape && start && extent, "%s: 1 to 5 axes, with shape, start and extent", what);
    VDX_CHECK(std::isfinite(sigma), "%s: sigma must be finite", what);
    uint64_t total = 1, n = 1;
    for (int d = 0; d < ndim; ++d) {
        VDX_CHECK(shape[d] >= 1 && extent[d] >= 1, "%s: axis %d: shape %zu and extent %zu must be >= 1", what, d, shape[d], extent[d]);
        VDX_CHECK(extent[d] <= shape[d] && start[d] <= shape[d] - extent[d], "%s: axis %d: the box [%zu, +%zu) leaves the shape %zu", what,
                  d, start[d], extent[d], shape[d]);
        VDX_CHECK(shape[d] <= (((uint64_t)1 << 63) - 1) / total, "%s: the logical tensor must have fewer than 2^63 elements", what);
        total *= shape[d];
        n *= extent[d];
    }
    // merge from the innermost axis outwards: an axis the box covers whole joins the row of the axis above it
    uint64_t sh[5], st[5], ex[5];
    int m = 0;                                                           // merged axes, innermost first
    uint64_t row_shape = shape[ndim - 1], row_start = start[ndim - 1], row_ext = extent[ndim - 1];
    int d = ndim - 2;
    for (; d >= 0 && row_ext == row_shape; --d) {
        row_start = start[d] * row_shape;
        row_ext = extent[d] * row_shape;
        row_shape = shape[d] * row_shape;
    }
    sh[m] = row_shape, st[m] = row_start, ex[m] = row_ext, ++m;
    for (; d >= 0; --d) sh[m] = shape[d], st[m] = start[d], ex[m] = extent[d], ++m;
    a.k0 = (uint32_t)seed, a.k1 = (uint32_t)((uint64_t)seed >> 32);
    a.s0 = (uint32_t)stream, a.s1 = (uint32_t)((uint64_t)stream >> 32);
    a.row = ex[0];
    a.n = n;
    a.sigma = sigma;
    a.base = st[0];
    bool pitch4 = true;
    for (int k = 0; k < 4; ++k) {                                        // ext / pitch: outermost first, padded with 1 / 0
        const int src = 4 - k;                                           // merged axis (1..4, innermost first) of slot k
        if (src < m) {
            uint64_t p = sh[0];
            for (int q = 1; q < src; ++q) p *= sh[q];
            a.ext[k] = ex[src], a.pitch[k] = p, a.base += st[src] * p;
            if (ex[src] > 1 && (p & 3)) pitch4 = false;
        } else {
            a.ext[k] = 1, a.pitch[k] = 0;
        }
    }
    const uint64_t rows = n / a.row;
    fast = (a.base & 3) == 0 && (rows == 1 || ((a.row & 3) == 0 && pitch4));
    return 0;
}

template <class T>
static int noise_launch(const char* what, size_t seed, size_t stream, int ndim, const size_t* shape, const size_t* start,
                        const size_t* extent, float sigma, void* out, vdx_stream_t hs) {
    noise_args a;
    int fast;
    if (int rc = noise_plan(what, seed, stream, ndim, shape, start, extent, sigma, a, fast)) return rc;
    VDX_CHECK(out && ((uintptr_t)out & 15) == 0, "%s: out must be a 16-byte aligned pointer", what);
    const uint64_t work = fast ? (a.n + 3) >> 2 : a.n, want = (work + 255) / 256;
    const dim3 grid((unsigned)(want < 65536 ? want : 65536)), block(256);
    if (fast) hipLaunchKernelGGL(noise_block_kernel<T>, grid, block, 0, (hipStream_t)hs, (T*)out, a);
    else hipLaunchKernelGGL(noise_elem_kernel<T>, grid, block, 0, (hipStream_t)hs, (T*)out, a);
    return vdx_launch_status(what);
}

extern "C" int vdx_noise_f16(size_t seed, size_t stream, int ndim, const size_t* shape, const size_t* start, const size_t* extent,
                             float sigma, void* out, vdx_stream_t hs) {
    return noise_launch<f16>("vdx_noise_f16", seed, stream, ndim, shape, start, extent, sigma, out, hs);
}

extern "C" int vdx_noise_f32(size_t seed, size_t stream, int ndim, const size_t* shape, const size_t* start, const size_t* extent,
                             void* out, vdx_stream_t hs) {
    return noise_launch<float>("vdx_noise_f32", seed, stream, ndim, shape, start, extent, 1.0f, out, hs);
}

extern "C" int vdx_noise_form(int ndim, const size_t* shape, const size_t* start, const size_t* extent) {
    noise_args a;
    int fast;
    if (noise_plan("vdx_noise_form", 0, 0, ndim, shape, start, extent, 1.0f, a, fast)) return -1;
    return fast;
}
