// inpaint.hip — masked video-to-video (no reference counterpart, opt-in: vdx/inpaint.py, `DiffuserConfig.mask` / `keep_frames`):
// hold part of an existing clip fixed and generate the rest (the replacement method of Ho et al. 2022; RePaint; diffusers'
// inpainting branch for 4-channel UNets).  The mask is binary, so every kernel here is a SELECT between two values' bits:
// nothing is multiplied by the mask, there is no 0 * inf, -0 keeps its sign and a NaN or an infinity stays in its element.
//
//   vdx_mask_renoise_f16     after a scheduler step, in place on a window's latent z (1,C,L,h,w):  m == 1: z keeps its bits;
//                            m == 0: z takes known's, known = add_noise(x0, base, t_next) (step_chains.h `add_noise_elem`, the
//                            chain of `vdx_add_noise_f16` itself), or x0's own bits with `last`.  x0, base (1,C,T,h,w) and
//                            m (T,h,w) are the CLIP's tensors, read at frame s + f: no slice copies.
//   vdx_mask_paste_f32       the same select on the fp32 blended latent (1,C,T,h,w): m ? z : float(x0)
//   vdx_mask_to_latent_u8    pixel mask (T,H,W) -> latent mask (T,H/8,W/8) in {0,1}: pixel (8y, 8x), or any of the cell's 64
//   vdx_mask_composite_u8    out = mask ? generated : original on uint8 (T,H,W,3) frames
//
// Block map of the two latent kernels: a block works on ONE (c, f) line of h*w elements (tiles of 256 lanes x E elements), so
// the frame offset is uniform over the block and no index depends on data.  E = 8 / 4 / 1 by h*w % 8, % 4: every line of z, x0,
// base and every mask row then starts on a vector boundary whatever s is (the frame offset moves all of them by multiples of
// h*w), a line is a whole number of vectors and there is no tail.  An element is read and written by one lane: no atomics.
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"

namespace {

template <int N> struct bits_of;                                  // an unsigned integer of N bytes
template <> struct bits_of<1> { typedef uint8_t type; };
template <> struct bits_of<2> { typedef uint16_t type; };
template <> struct bits_of<4> { typedef uint32_t type; };

// E values of B bytes each as one access of E*B bytes (1, 2, 4, 8 or 16), moved as integers: bits in, bits out
template <typename U, int E>
struct vec {
    typedef U type __attribute__((ext_vector_type(E)));
};
template <typename U, int E>
__device__ __forceinline__ void load_bits(const void* p, U (&v)[E]) {
    if constexpr (E == 1) {
        v[0] = *(const U*)p;
    } else {
        const typename vec<U, E>::type h = *(const typename vec<U, E>::type*)p;
#pragma unroll
        for (int j = 0; j < E; ++j) v[j] = h[j];
    }
}
template <typename U, int E>
__device__ __forceinline__ void store_bits(void* p, const U (&v)[E]) {
    if constexpr (E == 1) {
        *(U*)p = v[0];
    } else {
        typename vec<U, E>::type h;
#pragma unroll
        for (int j = 0; j < E; ++j) h[j] = v[j];
        *(typename vec<U, E>::type*)p = h;
    }
}

// Z = f16: the step's select (NOISE: known = add_noise chain; else known = x0).  Z = float: the paste (known = float(x0)).
// z (C, L, HW) in place; x0, base (C, T, HW) and m (T, HW) read at frame s + f.
template <typename Z, int E, bool NOISE>
__global__ __launch_bounds__(256) void mask_select_kernel(Z* z, const f16* x0, const f16* base, const uint8_t* m, float sa,
                                                          float s1, int T, int s, int L, int HW, unsigned tiles_per_line) {
    typedef typename bits_of<sizeof(Z)>::type ZB;
    const unsigned line = blockIdx.x / tiles_per_line, tile = blockIdx.x - line * tiles_per_line;
    const int c = (int)(line / (unsigned)L), f = (int)(line - (unsigned)c * (unsigned)L);
    const int p = (int)((tile * 256u + threadIdx.x) * (unsigned)E);
    if (p >= HW) return;                                          // HW is a multiple of E: a lane's E elements are all inside
    uint8_t mk[E];
    load_bits<uint8_t, E>(m + (size_t)(s + f) * HW + p, mk);
    bool all = true;
#pragma unroll
    for (int j = 0; j < E; ++j) all = all && mk[j] != 0;
    if (all) return;                                              // nothing kept here: z is neither read nor written
    const size_t iz = (size_t)line * HW + p, ic = ((size_t)c * T + s + f) * HW + p;
    ZB zb[E];
    uint16_t xb[E];
    load_bits<ZB, E>(z + iz, zb);
    load_bits<uint16_t, E>(x0 + ic, xb);
    uint16_t nb[E];
    if (NOISE) load_bits<uint16_t, E>(base + ic, nb);
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const f16 x = __builtin_bit_cast(f16, xb[j]);
        ZB known;
        if constexpr (sizeof(Z) == 4) {
            known = __builtin_bit_cast(ZB, (float)x);                                   // fp16 -> fp32 is exact
        } else if (NOISE) {
            known = __builtin_bit_cast(ZB, add_noise_elem((float)x, (float)__builtin_bit_cast(f16, nb[j]), sa, s1));
        } else {
            known = xb[j];
        }
        zb[j] = mk[j] ? zb[j] : known;
    }
    store_bits<ZB, E>(z + iz, zb);
}

// ---- pixel mask -> latent mask: one thread per latent cell ---------------------------------------------------------------
template <bool ANY>
__global__ __launch_bounds__(256) void mask_to_latent_kernel(const uint8_t* px, uint8_t* out, int T, int h, int w) {
    const size_t total = (size_t)T * h * w, W = (size_t)w * 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % w);
        const size_t ty = i / w;                                  // t * h + y: the cell's first pixel row is 8 * (t*h + y)
        const uint8_t* cell = px + ty * 8 * W + (size_t)x * 8;
        uint32_t any;
        if (ANY) {
            any = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) {                         // W % 8 == 0 and px 8-byte aligned: every cell row is
                const uint2 v = *(const uint2*)(cell + r * W);
                any |= v.x | v.y;
            }
        } else {
            any = cell[0];                                        // F.interpolate(mode="nearest") at the exact factor 8
        }
        out[i] = any ? 1 : 0;
    }
}

// ---- out = mask ? generated : original, P pixels (3P bytes) per thread ----------------------------------------------------
template <int P>
__global__ __launch_bounds__(256) void mask_composite_kernel(const uint8_t* gen, const uint8_t* orig, const uint8_t* m,
                                                             uint8_t* out, size_t groups) {
    typedef uint32_t W;                                           // the vector paths move 4-byte words
    constexpr int NW = P == 16 ? 4 : 1;                           // words per colour-third / per mask group
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        if constexpr (P == 1) {
            const bool k = m[g] != 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) out[g * 3 + j] = k ? gen[g * 3 + j] : orig[g * 3 + j];
        } else {
            W mw[NW], gw[3 * NW], ow[3 * NW];
            load_bits<W, NW>(m + g * P, mw);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                W a[NW], b[NW];
                load_bits<W, NW>(gen + g * 3 * P + (size_t)q * P, a);
                load_bits<W, NW>(orig + g * 3 * P + (size_t)q * P, b);
#pragma unroll
                for (int j = 0; j < NW; ++j) gw[q * NW + j] = a[j], ow[q * NW + j] = b[j];
            }
#pragma unroll
            for (int i = 0; i < 3 * NW; ++i) {                    // byte b of the 3P belongs to pixel b / 3
                uint32_t sel = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int px = (i * 4 + k) / 3;
                    const uint32_t mb = (mw[px / 4] >> (8 * (px % 4))) & 0xffu;
                    sel |= (mb ? 0xffu : 0u) << (8 * k);
                }
                gw[i] = (gw[i] & sel) | (ow[i] & ~sel);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                W a[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) a[j] = gw[q * NW + j];
                store_bits<W, NW>(out + g * 3 * P + (size_t)q * P, a);
            }
        }
    }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

int grid_for(size_t total) {
    const size_t b = (total + 255) / 256;
    return (int)(b < 65536 ? (b > 0 ? b : 1) : 65536);
}

// shared checks and launch of the two latent selects; zbytes = sizeof an element of z
template <typename Z>
int select_launch(const char* what, Z* z, const void* x0, const void* base, const void* m, float sa, float s1, bool noise, int C,
                  int T, int HW, int s, int L, vdx_stream_t stream) {
    VDX_CHECK(z && x0 && m && (!noise || base), "%s: null pointer", what);
    VDX_CHECK(C > 0 && T > 0 && HW > 0 && HW <= 1 << 30, "%s: bad shape C=%d T_clip=%d HW=%d", what, C, T, HW);
    VDX_CHECK(L >= 1 && s >= 0 && s < T && L <= T - s, "%s: window [%d, %d + %d) leaves the clip's %d frames", what, s, s, L, T);
    VDX_CHECK((size_t)C * T <= (size_t)1 << 30 && (size_t)C * T * HW <= (size_t)1 << 40, "%s: latent too large", what);
    for (const void* ptr : {(const void*)z, x0, base, m}) VDX_CHECK(((uintptr_t)ptr & 15) == 0, "%s: pointer not 16-byte aligned", what);
    const size_t nz = (size_t)C * L * HW * sizeof(Z), nc = (size_t)C * T * HW * sizeof(f16);
    VDX_CHECK(!overlap(z, nz, x0, nc) && !(base && overlap(z, nz, base, nc)) && !overlap(z, nz, m, (size_t)T * HW),
              "%s: z overlaps an input", what);
    constexpr int EMAX = sizeof(Z) == 2 ? 8 : 4;                  // 16 bytes of z per lane
    const int e = HW % EMAX == 0 ? EMAX : (EMAX == 8 && HW % 4 == 0) ? 4 : 1;
    const size_t per_tile = 256 * (size_t)e;
    const size_t tiles_per_line = ((size_t)HW + per_tile - 1) / per_tile;
    const size_t blocks = tiles_per_line * C * L;
    VDX_CHECK(blocks <= 0x7fffffffull, "%s: %zu blocks exceed the grid", what, blocks);
    const dim3 grid((unsigned)blocks), block(256);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned tpl = (unsigned)tiles_per_line;
    const f16 *xx = (const f16*)x0, *bb = (const f16*)base;
    const uint8_t* mm = (const uint8_t*)m;
#define SELECT_GO(EE, N) hipLaunchKernelGGL((mask_select_kernel<Z, EE, N>), grid, block, 0, st, z, xx, bb, mm, sa, s1, T, s, L, HW, tpl)
    if constexpr (sizeof(Z) == 2) {
        if (noise) {
            if (e == 8) SELECT_GO(8, true);
            else if (e == 4) SELECT_GO(4, true);
            else SELECT_GO(1, true);
        } else {
            if (e == 8) SELECT_GO(8, false);
            else if (e == 4) SELECT_GO(4, false);
            else SELECT_GO(1, false);
        }
    } else {
        if (e == 4) SELECT_GO(4, false);
        else SELECT_GO(1, false);
    }
#undef SELECT_GO
    return vdx_launch_status(what);
}

}  // namespace

extern "C" int vdx_mask_renoise_f16(void* z, const void* x0, const void* base, const void* mask, float sqrt_ab, float sqrt_1mab,
                                    int last, int C, int T_clip, int HW, int s, int L, vdx_stream_t stream) {
    return select_launch<f16>("vdx_mask_renoise_f16", (f16*)z, x0, base, mask, sqrt_ab, sqrt_1mab, !last, C, T_clip, HW, s, L,
                              stream);
}

extern "C" int vdx_mask_paste_f32(float* z, const void* x0, const void* mask, int C, int T, int HW, vdx_stream_t stream) {
    return select_launch<float>("vdx_mask_paste_f32", z, x0, nullptr, mask, 0.f, 0.f, false, C, T, HW, 0, T, stream);
}

extern "C" int vdx_mask_to_latent_u8(const void* pixel_mask, void* latent_mask, int T, int H, int W, int any,
                                     vdx_stream_t stream) {
    VDX_CHECK(pixel_mask && latent_mask, "mask_to_latent: null pointer");
    VDX_CHECK(T > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "mask_to_latent: T=%d H=%d W=%d (H and W must be multiples of 8)",
              T, H, W);
    VDX_CHECK(any == 0 || any == 1, "mask_to_latent: rule %d (0: nearest, 1: any)", any);
    VDX_CHECK(((uintptr_t)pixel_mask & 7) == 0, "mask_to_latent: pixel_mask must be 8-byte aligned");
    const size_t n = (size_t)T * H * W;
    VDX_CHECK(!overlap(latent_mask, n / 64, pixel_mask, n), "mask_to_latent: the masks overlap");
    const dim3 grid(grid_for(n / 64)), block(256);
    if (any)
        hipLaunchKernelGGL(mask_to_latent_kernel<true>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)pixel_mask,
                           (uint8_t*)latent_mask, T, H / 8, W / 8);
    else
        hipLaunchKernelGGL(mask_to_latent_kernel<false>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)pixel_mask,
                           (uint8_t*)latent_mask, T, H / 8, W / 8);
    return vdx_launch_status("vdx_mask_to_latent_u8");
}

extern "C" int vdx_mask_composite_u8(const void* generated, const void* original, const void* mask, void* out, int T, int H,
                                     int W, vdx_stream_t stream) {
    VDX_CHECK(generated && original && mask && out, "mask_composite: null pointer");
    VDX_CHECK(T > 0 && H > 0 && W > 0, "mask_composite: T=%d H=%d W=%d", T, H, W);
    const size_t n = (size_t)T * H * W;
    VDX_CHECK(out == generated || !overlap(out, 3 * n, generated, 3 * n), "mask_composite: out overlaps generated without being it");
    VDX_CHECK(!overlap(out, 3 * n, original, 3 * n) && !overlap(out, 3 * n, mask, n), "mask_composite: out overlaps an input");
    uintptr_t bits = 0;
    for (const void* ptr : {generated, original, mask, (const void*)out}) bits |= (uintptr_t)ptr;
    // a group of P pixels starts on a P-byte boundary of the mask and a 3P-byte boundary of the frames wherever 3 W bytes of
    // a row are a multiple of 3P (rows are packed, so then every row, and every frame, starts on such a boundary too)
    const int P = (W % 16 == 0 && (bits & 15) == 0) ? 16 : (W % 4 == 0 && (bits & 3) == 0) ? 4 : 1;
    const size_t groups = n / P;
    const dim3 grid(grid_for(groups)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    const uint8_t *g = (const uint8_t*)generated, *o = (const uint8_t*)original, *m = (const uint8_t*)mask;
    if (P == 16) hipLaunchKernelGGL(mask_composite_kernel<16>, grid, block, 0, st, g, o, m, (uint8_t*)out, groups);
    else if (P == 4) hipLaunchKernelGGL(mask_composite_kernel<4>, grid, block, 0, st, g, o, m, (uint8_t*)out, groups);
    else hipLaunchKernelGGL(mask_composite_kernel<1>, grid, block, 0, st, g, o, m, (uint8_t*)out, groups);
    return vdx_launch_status("vdx_mask_composite_u8");
}
