// deflicker.hip — motion-compensated temporal filtering of a uint8 RGB clip along its Farneback flows (no reference counterpart:
// the reference writes the decoded frames as they are).  vdx/deflicker.py drives it; tests/deflicker_ref.py states the
// definition in float64 numpy and the tests pin this kernel to it.  For frame t, its neighbours n = t-1 and t+1 (those that
// exist; with `loop` both always do, mod F), the flow f that leaves frame t towards n (fba[t-1] towards t-1, fab[t] towards
// t+1), and a pixel q = (x, y):
//
//   c   = (x + f(q).x, y + f(q).y), each clamped to [0, W-1] / [0, H-1] by fmin(fmax(., 0), hi): NaN -> 0, +inf -> hi
//   Wn(q) = bilinear sample of frame n at c, per channel: (v00 (1-fx) + v01 fx) (1-fy) + (v10 (1-fx) + v11 fx) fy
//   en(q) = ((I(q).r - Wn(q).r)^2 + (I(q).g - Wn(q).g)^2) + (I(q).b - Wn(q).b)^2
//   dn(p) = (the sum of en over the 3 x 3 patch around p, row-major, coordinates clamped to the frame) / 27
//   wn(p) = 1 / (1 + dn(p) / (sigma sigma)), 0 for a neighbour that does not exist
//   out(p) = (I(p) + strength (w- W-(p) + w+ W+(p))) / (1 + strength (w- + w+)), then floor(out + 0.5) clamped to [0, 255]
//
// fp32 in exactly this grouping (the file is compiled without mul-add contraction).
//
// How the work is split.  A block of 256 threads owns a 32 x 16 tile of one output frame; the grid is (tiles x, tiles y, F), one
// launch per pass.  The patch sum needs en on the tile and a one-pixel halo, 34 x 18 positions.  Every position is warped ONCE
// per block, by its own flow: a thread warps its two tile pixels (rows ty and ty + 8), keeps I, W- and W+ of both in registers
// for the blend, and writes only the two scalars e-, e+ to LDS; the first 100 threads then do the same for one halo position
// each and keep nothing.  After one barrier a thread forms its two pixels' nine-tap sums from LDS (18 LDS reads per neighbour
// instead of nine warps = 36 global gathers), the weights and the blend in registers, and stores three bytes per pixel.  LDS
// holds 2 x 34 x 18 floats (4.8 KB), not the colour tiles: only the centre of a patch needs colours, and its owner has them.
// Positions past the frame's edge are clamped into it before anything is read (border replicate), so a partial tile, H = 1 or
// W = 1 read nothing outside; every gather index is an integer clamped to the frame after the float was clamped, so no flow
// value (huge, NaN, inf) can address outside the frames.  A missing neighbour is a branch on t alone, uniform over the block.
// No atomics, no reduction across threads: the same bytes on every run and whatever the batch holds.  There is no matrix
// product in this arithmetic (a gather, nine adds and two divisions per pixel and neighbour), so no MFMA.
#include "vdx_common.h"

#define DFK_TW 32                                     // tile width = threads per row
#define DFK_TH 16                                     // tile height = 2 rows per thread
#define DFK_LW (DFK_TW + 2)                           // tile + halo
#define DFK_LH (DFK_TH + 2)
#define DFK_RING (DFK_LW * DFK_LH - DFK_TW * DFK_TH)  // 100 halo positions

// clamp to [0, hi]: fmaxf / fminf return the other operand for a NaN, so NaN -> 0, +inf -> hi, -inf -> 0
__device__ __forceinline__ float dfk_clamp(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }

// frame `img` sampled at (x, y) + f, border replicate -> s[3]
__device__ __forceinline__ void dfk_warp(const unsigned char* img, int rp, int H, int W, int x, int y, float2 f, float s[3]) {
    const float cx = dfk_clamp((float)x + f.x, (float)(W - 1)), cy = dfk_clamp((float)y + f.y, (float)(H - 1));
    const float flx = floorf(cx), fly = floorf(cy);
    const int x0 = min(max((int)flx, 0), W - 1), y0 = min(max((int)fly, 0), H - 1);      // a no-op for a clamped float: the guard
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = cx - flx, fy = cy - fly, gx = 1.f - fx, gy = 1.f - fy;
    const unsigned char* r0 = img + (size_t)y0 * rp;
    const unsigned char* r1 = img + (size_t)y1 * rp;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        s[c] = ((float)r0[x0 * 3 + c] * gx + (float)r0[x1 * 3 + c] * fx) * gy + ((float)r1[x0 * 3 + c] * gx + (float)r1[x1 * 3 + c] * fx) * fy;
}

struct dfk_frame {                                    // what a block needs of its frame and the two neighbours
    const unsigned char *cur, *prev, *next;           // prev / next: NULL for a neighbour that does not exist
    const float2 *fprev, *fnext;                      // the flows that leave `cur` towards them
    int rp, H, W;
};

// one position (x, y), already inside the frame: I, W-, W+ and the two squared distances (0 for a missing neighbour)
__device__ __forceinline__ void dfk_position(const dfk_frame& fr, int x, int y, float I[3], float wm[3], float wp[3], float& em, float& ep) {
    const unsigned char* px = fr.cur + (size_t)y * fr.rp + (size_t)x * 3;
    I[0] = (float)px[0], I[1] = (float)px[1], I[2] = (float)px[2];
    const size_t o = (size_t)y * fr.W + x;
    em = ep = 0.f;
    wm[0] = wm[1] = wm[2] = wp[0] = wp[1] = wp[2] = 0.f;
    if (fr.prev) {                                    // uniform over the block
        dfk_warp(fr.prev, fr.rp, fr.H, fr.W, x, y, fr.fprev[o], wm);
        const float d0 = I[0] - wm[0], d1 = I[1] - wm[1], d2 = I[2] - wm[2];
        em = (d0 * d0 + d1 * d1) + d2 * d2;
    }
    if (fr.next) {
        dfk_warp(fr.next, fr.rp, fr.H, fr.W, x, y, fr.fnext[o], wp);
        const float d0 = I[0] - wp[0], d1 = I[1] - wp[1], d2 = I[2] - wp[2];
        ep = (d0 * d0 + d1 * d1) + d2 * d2;
    }
}

__device__ __forceinline__ float dfk_patch(const float* e, int lx, int ly) {      // the 3 x 3 sum around (lx, ly), row-major
    float s = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) s = s + e[(ly + dy) * DFK_LW + (lx + dx)];
    return s;
}

__global__ __launch_bounds__(DFK_TW * DFK_TH / 2) void deflicker_kernel(const unsigned char* frames, size_t fp, int rp, const float2* fab,
                                                                       const float2* fba, int F, int H, int W, int loop, float strength,
                                                                       float sigma, unsigned char* out, size_t ofp) {
    __shared__ float e_prev[DFK_LW * DFK_LH], e_next[DFK_LW * DFK_LH];
    const int t = blockIdx.z, bx = blockIdx.x * DFK_TW, by = blockIdx.y * DFK_TH;
    const int tid = threadIdx.x, tx = tid % DFK_TW, ty = tid / DFK_TW;
    const size_t plane = (size_t)H * W;
    const bool has_prev = loop || t > 0, has_next = loop || t < F - 1;
    const int tp = t > 0 ? t - 1 : F - 1, tn = t < F - 1 ? t + 1 : 0;                  // the neighbours' frames; fba[tp], fab[t] lead there
    dfk_frame fr;
    fr.cur = frames + (size_t)t * fp;
    fr.prev = has_prev ? frames + (size_t)tp * fp : nullptr;
    fr.next = has_next ? frames + (size_t)tn * fp : nullptr;
    fr.fprev = has_prev ? fba + (size_t)tp * plane : nullptr;
    fr.fnext = has_next ? fab + (size_t)t * plane : nullptr;
    fr.rp = rp, fr.H = H, fr.W = W;

    float I[2][3], wm[2][3], wp[2][3];
#pragma unroll
    for (int j = 0; j < 2; ++j) {                                                    // this thread's two tile pixels
        const int ly = ty + j * (DFK_TH / 2) + 1, lx = tx + 1;
        const int x = min(bx + tx, W - 1), y = min(by + ly - 1, H - 1);
        float em, ep;
        dfk_position(fr, x, y, I[j], wm[j], wp[j], em, ep);
        e_prev[ly * DFK_LW + lx] = em;
        e_next[ly * DFK_LW + lx] = ep;
    }
    if (tid < DFK_RING) {                                                            // one halo position: waves 0 and 1 only
        int lx, ly;
        if (tid < 2 * DFK_LW) {                                                      // the top and the bottom row, corners included
            ly = tid < DFK_LW ? 0 : DFK_LH - 1;
            lx = tid < DFK_LW ? tid : tid - DFK_LW;
        } else {                                                                     // the left and the right column between them
            const int k = tid - 2 * DFK_LW;
            lx = k < DFK_TH ? 0 : DFK_LW - 1;
            ly = (k < DFK_TH ? k : k - DFK_TH) + 1;
        }
        const int x = min(max(bx + lx - 1, 0), W - 1), y = min(max(by + ly - 1, 0), H - 1);
        float a[3], b[3], c[3], em, ep;
        dfk_position(fr, x, y, a, b, c, em, ep);
        e_prev[ly * DFK_LW + lx] = em;
        e_next[ly * DFK_LW + lx] = ep;
    }
    __syncthreads();

    const float s2 = sigma * sigma;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ly = ty + j * (DFK_TH / 2) + 1, lx = tx + 1;
        const int x = bx + tx, y = by + ly - 1;
        if (x >= W || y >= H) continue;
        const float dm = dfk_patch(e_prev, lx, ly) / 27.f, dp = dfk_patch(e_next, lx, ly) / 27.f;
        const float w_m = has_prev ? 1.f / (1.f + dm / s2) : 0.f;
        const float w_p = has_next ? 1.f / (1.f + dp / s2) : 0.f;
        const float den = 1.f + strength * (w_m + w_p);
        unsigned char* dst = out + (size_t)t * ofp + ((size_t)y * W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float o = (I[j][c] + strength * (w_m * wm[j][c] + w_p * wp[j][c])) / den;
            dst[c] = (unsigned char)fminf(fmaxf(floorf(o + 0.5f), 0.f), 255.f);
        }
    }
}

extern "C" int vdx_deflicker_u8(const void* frames, size_t frame_pitch, int row_pitch, const float* fab, const float* fba, int F, int H,
                                int W, int loop, float strength, float sigma, void* out, size_t out_frame_pitch, vdx_stream_t stream) {
    VDX_CHECK(frames && out, "deflicker: null pointer");
    VDX_CHECK(F >= 1 && F <= 65535, "deflicker: F=%d", F);
    VDX_CHECK(H > 0 && W > 0 && (long long)H * W < (1ll << 30), "deflicker: H=%d W=%d", H, W);
    VDX_CHECK((long long)row_pitch >= 3ll * W && frame_pitch >= (size_t)row_pitch * H, "deflicker: pitches too small");
    VDX_CHECK(out_frame_pitch >= (size_t)3 * W * H, "deflicker: out_frame_pitch too small");
    VDX_CHECK(loop == 0 || loop == 1, "deflicker: loop=%d", loop);
    VDX_CHECK((fab && fba) || (F == 1 && !loop), "deflicker: null flow pointer");          // F - 1 + loop flows each: none for one frame
    VDX_CHECK((size_t)fab % 8 == 0 && (size_t)fba % 8 == 0, "deflicker: flow pointers must be 8-byte aligned");
    VDX_CHECK(strength > 0.f && strength <= 1.f, "deflicker: strength=%g outside (0, 1]", (double)strength);
    VDX_CHECK(sigma > 0.f && sigma <= 3.0e38f, "deflicker: sigma=%g must be finite and > 0", (double)sigma);
    {                                                                                      // out must not alias the frames it reads
        const unsigned char *a = (const unsigned char*)frames, *b = (const unsigned char*)out;
        const size_t na = (size_t)(F - 1) * frame_pitch + (size_t)(H - 1) * row_pitch + (size_t)3 * W;
        const size_t nb = (size_t)(F - 1) * out_frame_pitch + (size_t)3 * W * H;
        VDX_CHECK(a + na <= b || b + nb <= a, "deflicker: out overlaps the frames");
    }
    const int tiles_x = (W + DFK_TW - 1) / DFK_TW, tiles_y = (H + DFK_TH - 1) / DFK_TH;
    VDX_CHECK(tiles_y <= 65535, "deflicker: H=%d", H);
    hipLaunchKernelGGL(deflicker_kernel, dim3(tiles_x, tiles_y, F), dim3(DFK_TW * DFK_TH / 2), 0, (hipStream_t)stream,
                       (const unsigned char*)frames, frame_pitch, row_pitch, (const float2*)fab, (const float2*)fba, F, H, W, loop, strength,
                       sigma, (unsigned char*)out, out_frame_pitch);
    return vdx_launch_status("vdx_deflicker_u8");
}
