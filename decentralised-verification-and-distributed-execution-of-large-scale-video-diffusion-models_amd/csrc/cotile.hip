// cotile.hip — spatially tiled co-denoising (MultiDiffusion, Bar-Tal et al. 2023, in its original form along space, on top of
// codenoise.hip's form along time; no reference counterpart, opt-in: vdx/codenoise.py, `DiffuserConfig.tile`).  ONE latent z
// (1,C,T,H,W) for the whole clip; a window is the Cartesian product of a time window kt (frames [s, s + L)), a row band ky (rows
// [y0, y0 + th)) and a column band kx (columns [x0, x0 + tw)); every window is a UNet call on a (2,C,L,th,tw) crop.
//
//   vdx_cfg_input_tile_f16         `vdx_cfg_input_window_f16` additionally cropped to the tile's rows and columns of z and of ctx:
//                                  the contiguous (2,C,L,th,tw) UNet input in one launch; the ctx term has its two roundings.
//   vdx_cotile_cfg_ddim_step_f16   per element (c, t, y, x), over the windows that hold it, in ascending (kt, ky, kx):
//   vdx_cotile_cfg_dpm_step_f16        w = fp32(fp32(wn[kt][t] * wyn[ky][y]) * wxn[kx][x])
//                                      U = sum w * fp32(u_k),  Cc = sum w * fp32(c_k)
//                                  every product one fp32 rounding, every add another (no fma; the sum STARTS with the first
//                                  product), then u = rn16(U), c = rn16(Cc) and the chains of step_chains.h, unchanged.
// With one spatial tile wyn = wxn = 1.0f, w = wn[kt][t], and the bits are those of codenoise.hip's cofuse kernels.
//
// Block map: a block works on ONE (c, t, y) row (segments of blockDim lanes x E elements), so the (kt, ky) loops, the table reads
// and the weight wn * wyn are uniform over the block.  In the kx loop a lane is inside column band kx or it is not (a predicate);
// the address it then reads is linear in its own x: nothing is indexed by data.  E = 8 (16-byte accesses) where every row
// segment of z and of every window starts on a 16-byte boundary (W, tw, every x0, every window offset and the tile stride
// multiples of 8), E = 4 (8-byte) for multiples of 4, else E = 1: a vector then lies wholly inside a column band or wholly
// outside.  An element is read and written by one lane only: lat_out may be z, nothing is atomic, and a NaN or an infinity stays
// in its element.  Cells outside a window's box are never read, whatever the weights hold there.
#include <cstdint>

#include "vdx_common.h"
#include "step_chains.h"
#include "cofuse_common.h"   // the vector accesses, fuse_term, the step tail and dispatch, the window-table and aliasing checks

#define COTILE_MAX_TILES 64

// the window table, by value in the kernel arguments (1.5 KiB): uniform reads, and the host has checked every row
struct cotile_tab {
    long long off[COFUSE_MAX_WINDOWS];     // element offset of time window kt's tile (0, 0) from the base pointer
    int s[COFUSE_MAX_WINDOWS];             // first frame
    int len[COFUSE_MAX_WINDOWS];           // L_kt
    int y0[COTILE_MAX_TILES];              // first row of band ky
    int x0[COTILE_MAX_TILES];              // first column of band kx
};

struct cotile_geom {
    int Kt, ny, nx, th, tw;
    long long stride;                      // elements from tile (ky, kx) to tile (ky, kx + 1) of one time window
    int C, T, H, W;
};

// MODE 0: DDIM; 1: DPM-Solver++ first order; 2: second order
template <int MODE, int E>
__global__ __launch_bounds__(256) void cotile_kernel(const f16* z, const f16* win, cotile_tab tab, cotile_geom g, const float* wn,
                                                     const float* wyn, const float* wxn, const f16* x0_prev, f16* x0_out, f16* out,
                                                     ddim_coef kd, dpm_coef kp, unsigned segs_per_row) {
    const unsigned row = blockIdx.x / segs_per_row, seg = blockIdx.x - row * segs_per_row;
    const unsigned ct = row / (unsigned)g.H;
    const int y = (int)(row - ct * (unsigned)g.H);
    const int c = (int)(ct / (unsigned)g.T), t = (int)(ct - (unsigned)c * (unsigned)g.T);
    const int x = (int)((seg * blockDim.x + threadIdx.x) * (unsigned)E);
    const cfg_guidance guide{};
    const cfg_guidance::state st = guide.prologue(c);             // all lanes, before any of them leaves
    if (x >= g.W) return;                                        // W is a multiple of E: a lane's E elements are all inside
    float U[E], Cc[E];
#pragma unroll
    for (int j = 0; j < E; ++j) U[j] = Cc[j] = 0.f;
    bool first = true;                                            // per lane: which kx comes first depends on x
    const size_t plane = (size_t)g.th * g.tw;
    for (int kt = 0; kt < g.Kt; ++kt) {                           // uniform over the block
        const int f = t - tab.s[kt], L = tab.len[kt];
        if (f < 0 || f >= L) continue;
        const float wt = wn[(size_t)kt * g.T + t];
        const size_t half = (size_t)g.C * L * plane;              // from u to c inside a window's block
        for (int ky = 0; ky < g.ny; ++ky) {                       // uniform over the block
            const int r = y - tab.y0[ky];
            if (r < 0 || r >= g.th) continue;
            const float wty = __fmul_rn(wt, wyn[(size_t)ky * g.H + y]);
            const f16* rowp = win + tab.off[kt] + (long long)ky * g.nx * g.stride + ((size_t)c * L + f) * plane + (size_t)r * g.tw;
            for (int kx = 0; kx < g.nx; ++kx) {
                const int q = x - tab.x0[kx];
                if (q < 0 || q >= g.tw) continue;                 // tw and x0 are multiples of E: all E elements are inside, or none
                const f16* up = rowp + (long long)kx * g.stride + q;
                const float* wp = wxn + (size_t)kx * g.W + x;
                f16 u[E], cc[E];
                load_halves<E>(up, u);
                load_halves<E>(up + half, cc);
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const float w = __fmul_rn(wty, wp[j]);
                    U[j] = fuse_term(U[j], w, (float)u[j], first);
                    Cc[j] = fuse_term(Cc[j], w, (float)cc[j], first);
                }
                first = false;
            }
        }
    }
    f16 uf[E], cf[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        uf[j] = rn16(U[j]);
        cf[j] = rn16(Cc[j]);
    }
    cofuse_tail<MODE, E>(z, x0_prev, x0_out, out, (size_t)row * g.W + x, uf, cf, guide, st, kd, kp);
}

// every band of `n0` inside [0, N), and every cell of [0, N) in some band
static int cotile_axis(const char* what, const char* axis, const int* n0, int n, int size, int N, int* dst) {
    VDX_CHECK(n0 && n >= 1 && n <= COTILE_MAX_TILES, "%s: %d %s bands, 1..%d are supported", what, n, axis, COTILE_MAX_TILES);
    VDX_CHECK(size >= 1 && size <= N, "%s: a %s band of %d cells does not fit %d", what, axis, size, N);
    for (int k = 0; k < n; ++k) {
        VDX_CHECK(n0[k] >= 0 && n0[k] <= N - size, "%s: %s band %d = [%d, %d + %d) leaves the %d cells", what, axis, k, n0[k], n0[k], size, N);
        dst[k] = n0[k];
    }
    for (int p = 0; p < N; ++p) {
        bool hit = false;
        for (int k = 0; k < n && !hit; ++k) hit = p >= n0[k] && p - n0[k] < size;
        VDX_CHECK(hit, "%s: %s cell %d is in no band", what, axis, p);
    }
    return 0;
}

static int cotile_launch(const char* what, int mode, const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                         const int* win_start, const int* win_len, int Kt, const float* wn, size_t tile_stride, const int* tile_y0,
                         int ny, const float* wyn, const int* tile_x0, int nx, const float* wxn, int th, int tw, const void* x0_prev,
                         void* x0_out, void* lat_out, ddim_coef kd, dpm_coef kp, int C, int T, int H, int W, vdx_stream_t stream) {
    VDX_CHECK(z && windows && win_off && win_start && win_len && wn && wyn && wxn && lat_out, "%s: null pointer", what);
    VDX_CHECK(C > 0 && T > 0 && H > 0 && W > 0 && (size_t)H * W <= (size_t)1 << 30, "%s: bad shape C=%d T=%d H=%d W=%d", what, C, T, H, W);
    VDX_CHECK(Kt >= 1 && Kt <= COFUSE_MAX_WINDOWS, "%s: %d time windows, 1..%d are supported", what, Kt, COFUSE_MAX_WINDOWS);
    VDX_CHECK(ny >= 1 && nx >= 1 && (long long)ny * nx <= COTILE_MAX_TILES, "%s: %d x %d tiles, at most %d are supported", what, ny, nx,
              COTILE_MAX_TILES);
    VDX_CHECK(mode == 0 || x0_out, "%s: x0_out is null", what);
    const size_t n = (size_t)C * T * H * W, nb = n * sizeof(f16);
    VDX_CHECK((size_t)C * T * H <= (size_t)1 << 30 && n <= (size_t)1 << 40, "%s: latent too large", what);
    for (const void* ptr : {z, windows, (const void*)wn, (const void*)wyn, (const void*)wxn, x0_prev, (const void*)x0_out, (const void*)lat_out})
        VDX_CHECK(((uintptr_t)ptr & 15) == 0, "%s: pointer not 16-byte aligned", what);
    cotile_tab tab = {};
    if (int rc = cotile_axis(what, "row", tile_y0, ny, th, H, tab.y0)) return rc;
    if (int rc = cotile_axis(what, "column", tile_x0, nx, tw, W, tab.x0)) return rc;
    const size_t plane = (size_t)th * tw;
    const int ntile = ny * nx;
    VDX_CHECK(tile_stride <= (size_t)1 << 40, "%s: bad tile stride %zu", what, tile_stride);
    int e = W % 8 == 0 && tw % 8 == 0 ? 8 : W % 4 == 0 && tw % 4 == 0 ? 4 : 1;
    for (int k = 0; k < nx; ++k) co_narrow(e, tab.x0[k]);         // and by every window offset, below
    if (ntile > 1) co_narrow(e, (long long)tile_stride);
    const auto need = [&](int k, int L, size_t& elems) {
        const size_t block = 2 * (size_t)C * L * plane;           // one tile's (2,C,L,th,tw)
        VDX_CHECK(ntile == 1 || tile_stride >= block, "%s: window %d: tiles of %zu elements overlap at stride %zu", what, k, block,
                  tile_stride);
        elems = (size_t)(ntile - 1) * tile_stride + block;
        return 0;
    };
    if (int rc = cofuse_windows(what, false, windows_elems, win_off, win_start, win_len, Kt, T, need, tab, e)) return rc;
    const co_buf inputs[] = {{windows, windows_elems * sizeof(f16)}, {wn, (size_t)Kt * T * sizeof(float)},
                             {wyn, (size_t)ny * H * sizeof(float)}, {wxn, (size_t)nx * W * sizeof(float)}};
    if (int rc = cofuse_alias(what, mode, z, x0_prev, x0_out, lat_out, nb, inputs, "z or lat_out", "an input")) return rc;
    const unsigned vecs = (unsigned)(W / e);                      // vectors per row
    const unsigned threads = vecs >= 256 ? 256u : (vecs + 63u) / 64u * 64u;
    const size_t segs = (vecs + threads - 1) / threads;
    const size_t blocks = segs * C * T * H;
    VDX_CHECK(blocks <= 0x7fffffffull, "%s: %zu blocks exceed the grid", what, blocks);
    const cotile_geom g = {Kt, ny, nx, th, tw, (long long)tile_stride, C, T, H, W};
    step_dispatch(mode, x0_prev, e, [&](auto m, auto ee) {
        hipLaunchKernelGGL((cotile_kernel<decltype(m)::value, decltype(ee)::value>), dim3((unsigned)blocks), dim3(threads), 0,
                           (hipStream_t)stream, (const f16*)z, (const f16*)windows, tab, g, wn, wyn, wxn, (const f16*)x0_prev,
                           (f16*)x0_out, (f16*)lat_out, kd, kp, (unsigned)segs);
    });
    return vdx_launch_status(what);
}

extern "C" int vdx_cotile_cfg_ddim_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                            const int* win_start, const int* win_len, int Kt, const float* wn, size_t tile_stride,
                                            const int* tile_y0, int ny, const float* wyn, const int* tile_x0, int nx, const float* wxn,
                                            int th, int tw, void* lat_out, float guidance, float sqrt_one_minus_at, float sqrt_at,
                                            float sqrt_aprev, float sqrt_one_minus_aprev, int C, int T, int H, int W,
                                            vdx_stream_t stream) {
    const ddim_coef kd = {guidance, sqrt_one_minus_at, 1.0f / sqrt_at, sqrt_aprev, sqrt_one_minus_aprev};
    return cotile_launch("vdx_cotile_cfg_ddim_step_f16", 0, z, windows, windows_elems, win_off, win_start, win_len, Kt, wn, tile_stride,
                         tile_y0, ny, wyn, tile_x0, nx, wxn, th, tw, nullptr, nullptr, lat_out, kd, dpm_coef{}, C, T, H, W, stream);
}

extern "C" int vdx_cotile_cfg_dpm_step_f16(const void* z, const void* windows, size_t windows_elems, const int64_t* win_off,
                                           const int* win_start, const int* win_len, int Kt, const float* wn, size_t tile_stride,
                                           const int* tile_y0, int ny, const float* wyn, const int* tile_x0, int nx, const float* wxn,
                                           int th, int tw, const void* x0_prev, void* x0_out, void* lat_out, float guidance, float c_s0,
                                           float c_inv_a0, float c_x, float c_d0, float c_d1, float c_inv_r0, int C, int T, int H, int W,
                                           vdx_stream_t stream) {
    const dpm_coef kp = {guidance, c_s0, c_inv_a0, c_x, c_d0, c_d1, c_inv_r0};
    return cotile_launch("vdx_cotile_cfg_dpm_step_f16", 1, z, windows, windows_elems, win_off, win_start, win_len, Kt, wn, tile_stride,
                         tile_y0, ny, wyn, tile_x0, nx, wxn, th, tw, x0_prev, x0_out, lat_out, ddim_coef{}, kp, C, T, H, W, stream);
}

// ---- the UNet input of one tile of one window, straight out of the whole-clip latent -------------------------------------------
//   x = cat([z[:, :, s:e, y0:y0+th, x0:x0+tw]]*2);  x = x + context_weight * ctx[..., y0:y0+th, x0:x0+tw]   (cfg_input_kernel's expression)
template <int E>
__global__ __launch_bounds__(256) void cfg_input_tile_kernel(const f16* z, const f16* ctx, float weight, f16* x2, int C, int T, int H, int W,
                                                             int s, int L, int y0, int th, int x0, int tw) {
    const int rv = tw / E;                                        // vectors per tile row
    const size_t nv = (size_t)C * L * th * rv, n = (size_t)C * L * th * tw;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(v % rv) * E;
        size_t rest = v / rv;
        const int r = (int)(rest % th);
        rest /= th;
        const int f = (int)(rest % L);
        const int c = (int)(rest / L);
        const size_t at = (size_t)(y0 + r) * W + x0 + q;          // inside one frame of z, or of ctx
        f16 o[E];
        load_halves<E>(z + ((size_t)c * T + s + f) * H * W + at, o);
        if (ctx) add_ctx<E>(o, ctx + (size_t)c * H * W + at, weight);
        const size_t d = (((size_t)c * L + f) * th + r) * tw + q;
        store_halves<E>(x2 + d, o);
        store_halves<E>(x2 + n + d, o);
    }
}

extern "C" int vdx_cfg_input_tile_f16(const void* z, const void* ctx, float weight, void* x2, int C, int T, int H, int W, int s, int e,
                                      int y0, int th, int x0, int tw, vdx_stream_t stream) {
    VDX_CHECK(z && x2 && C > 0 && T > 0 && H > 0 && W > 0 && (size_t)H * W <= (size_t)1 << 30, "cfg_input_tile: bad arguments");
    VDX_CHECK(0 <= s && s < e && e <= T, "cfg_input_tile: bad range [%d,%d) of %d", s, e, T);
    VDX_CHECK(th >= 1 && th <= H && y0 >= 0 && y0 <= H - th, "cfg_input_tile: rows [%d, %d + %d) leave the %d rows", y0, y0, th, H);
    VDX_CHECK(tw >= 1 && tw <= W && x0 >= 0 && x0 <= W - tw, "cfg_input_tile: columns [%d, %d + %d) leave the %d columns", x0, x0, tw, W);
    for (const void* ptr : {z, ctx, (const void*)x2}) VDX_CHECK(((uintptr_t)ptr & 15) == 0, "cfg_input_tile: pointer not 16-byte aligned");
    const int L = e - s;
    const size_t n = (size_t)C * L * th * tw;
    VDX_CHECK(!co_overlap(x2, 2 * n * sizeof(f16), z, (size_t)C * T * H * W * sizeof(f16)), "cfg_input_tile: x2 overlaps z");
    VDX_CHECK(!ctx || !co_overlap(x2, 2 * n * sizeof(f16), ctx, (size_t)C * H * W * sizeof(f16)), "cfg_input_tile: x2 overlaps ctx");
    // every row segment of z, ctx and both halves of x2 on a 16-byte (8-byte) boundary
    const int E = W % 8 == 0 && tw % 8 == 0 && x0 % 8 == 0 ? 8 : W % 4 == 0 && tw % 4 == 0 && x0 % 4 == 0 ? 4 : 1;
    const size_t nv = n / E;
    VDX_CHECK((nv + 255) / 256 <= 0x7fffffffull, "cfg_input_tile: tile too large");
    const unsigned blocks = (unsigned)((nv + 255) / 256);         // no cap: one vector per lane
    const hipStream_t st = (hipStream_t)stream;
#define TILE_GO(EE) \
    hipLaunchKernelGGL(cfg_input_tile_kernel<EE>, dim3(blocks), dim3(256), 0, st, (const f16*)z, (const f16*)ctx, weight, (f16*)x2, C, T, H, W, s, L, y0, th, x0, tw)
    if (E == 8) TILE_GO(8);
    else if (E == 4) TILE_GO(4);
    else TILE_GO(1);
#undef TILE_GO
    return vdx_launch_status("vdx_cfg_input_tile_f16");
}
