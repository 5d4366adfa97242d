// interp.hip — motion-compensated frame interpolation of a uint8 RGB clip from its Farneback flows (no reference counterpart:
// the reference writes the generated frames as they are).  vdx/interp.py drives it; tests/interp_ref.py states the expression in
// float64 numpy and the tests pin this kernel to it.  For consecutive frames A = f[i], B = f[i+1], flows Fab (A -> B) and Fba
// (B -> A), a factor N and k = 1 .. N-1, with t = k / N and a = (N - k) / N (both quotients of integers, so that (A, B, k) and
// (B, A, N - k) are the same arithmetic), at output pixel x:
//
//   gA = (t t) Fba(x) - (a t) Fab(x)        gB = (a a) Fab(x) - (a t) Fba(x)            Super SloMo's intermediate flows
//   a non-finite g is taken as 0; p = x + g; c = p clamped to [0, W-1] x [0, H-1]
//   S  = bilinear sample of the frame at c (border replicate)
//   cf = bilinear sample of the frame's own flow at c;  r = cf + bilinear sample of the other flow at clamp(c + cf)
//   v  = 1 / (1 + |r|^2), 0 when |r|^2 is not finite; times 1e-6 when g was not finite or p lies outside
//        [-0.5, W-0.5] x [-0.5, H-0.5]
//   wA = a vA, wB = t vB; when wA + wB is not positive, wA = a and wB = t;  out = (wA SA + wB SB) / (wA + wB)
//   byte = floor(out + 0.5) clamped to [0, 255]
//
// fp32 in exactly this grouping (the file is compiled without mul-add contraction).  One launch writes the whole output clip,
// the originals at i N included; no atomic, no reduction: the same bits on every run and whatever the batch holds.  A thread
// owns four pixels of a row (12 bytes: three dwords where the address allows), loads their flows once and loops over k.
// Every gather address is formed from integer coordinates clamped to the frame, and the float is clamped before it is
// converted, so no flow value (huge, NaN, inf) can address outside the frames.
#include "vdx_common.h"

#define INTERP_RUN 4                                  // pixels per thread

struct interp_tap {
    int x0, x1, y0, y1;
    float fx, fy;
};

// clamp to [0, hi]: fmaxf / fminf return the other operand for a NaN, so NaN -> 0, +inf -> hi, -inf -> 0
__device__ __forceinline__ float interp_clamp(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }

__device__ __forceinline__ interp_tap interp_taps(float cx, float cy, int W, int H) {     // cx, cy already clamped
    interp_tap t;
    const float flx = floorf(cx), fly = floorf(cy);
    t.x0 = min(max((int)flx, 0), W - 1);              // the integer clamp is a no-op for a clamped float: kept as the guard
    t.y0 = min(max((int)fly, 0), H - 1);
    t.x1 = min(t.x0 + 1, W - 1);
    t.y1 = min(t.y0 + 1, H - 1);
    t.fx = cx - flx;
    t.fy = cy - fly;
    return t;
}

__device__ __forceinline__ float interp_lerp2(float v00, float v01, float v10, float v11, float fx, float fy) {
    const float gx = 1.f - fx, gy = 1.f - fy;
    return (v00 * gx + v01 * fx) * gy + (v10 * gx + v11 * fx) * fy;
}

__device__ __forceinline__ float2 interp_flow_at(const float2* fl, int W, const interp_tap& t) {
    const float2 a = fl[(size_t)t.y0 * W + t.x0], b = fl[(size_t)t.y0 * W + t.x1];
    const float2 c = fl[(size_t)t.y1 * W + t.x0], d = fl[(size_t)t.y1 * W + t.x1];
    return make_float2(interp_lerp2(a.x, b.x, c.x, d.x, t.fx, t.fy), interp_lerp2(a.y, b.y, c.y, d.y, t.fx, t.fy));
}

// one side of the blend: the sample of `img` at x + g and its weight before the time factor.  `own` is the flow that leaves
// `img`, `other` the flow that comes back to it.
__device__ __forceinline__ void interp_side(const unsigned char* img, int rp, const float2* own, const float2* other, int H, int W,
                                            int x, int y, float gx, float gy, float s[3], float& v) {
    const bool fin = isfinite(gx) && isfinite(gy);
    const float px = (float)x + (fin ? gx : 0.f), py = (float)y + (fin ? gy : 0.f);
    const bool inside = fin && px >= -0.5f && px <= (float)W - 0.5f && py >= -0.5f && py <= (float)H - 0.5f;
    const float cx = interp_clamp(px, (float)(W - 1)), cy = interp_clamp(py, (float)(H - 1));
    const interp_tap t = interp_taps(cx, cy, W, H);
    const unsigned char* r0 = img + (size_t)t.y0 * rp;
    const unsigned char* r1 = img + (size_t)t.y1 * rp;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        s[c] = interp_lerp2((float)r0[t.x0 * 3 + c], (float)r0[t.x1 * 3 + c], (float)r1[t.x0 * 3 + c], (float)r1[t.x1 * 3 + c], t.fx, t.fy);
    const float2 cf = interp_flow_at(own, W, t);
    const interp_tap q = interp_taps(interp_clamp(cx + cf.x, (float)(W - 1)), interp_clamp(cy + cf.y, (float)(H - 1)), W, H);
    const float2 back = interp_flow_at(other, W, q);
    const float rx = cf.x + back.x, ry = cf.y + back.y;
    const float n2 = rx * rx + ry * ry;
    v = isfinite(n2) ? 1.f / (1.f + n2) : 0.f;
    if (!inside) v = v * 1e-6f;
}

__device__ __forceinline__ void interp_store(unsigned char* dst, const unsigned char* b, int n) {
    if (n == INTERP_RUN && ((size_t)dst & 3) == 0) {
        unsigned int* d = (unsigned int*)dst;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d[j] = (unsigned)b[4 * j] | (unsigned)b[4 * j + 1] << 8 | (unsigned)b[4 * j + 2] << 16 | (unsigned)b[4 * j + 3] << 24;
    } else {
        for (int j = 0; j < 3 * n; ++j) dst[j] = b[j];
    }
}

__global__ __launch_bounds__(256) void interp_frames_kernel(const unsigned char* frames, size_t fp, int rp, const float2* fab,
                                                            const float2* fba, int F, int H, int W, int N, int groups,
                                                            long long total, unsigned char* out, size_t ofp) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(idx % groups);
        const long long fy = idx / groups;
        const int y = (int)(fy % H);
        const int i = (int)(fy / H);                                      // frame i, and the pair (i, i + 1) when i < F - 1
        const int x0 = g * INTERP_RUN;
        const int n = min(INTERP_RUN, W - x0);
        const unsigned char* A = frames + (size_t)i * fp;
        unsigned char bytes[3 * INTERP_RUN];
        // the original, byte for byte, at output frame i N
        const unsigned char* src = A + (size_t)y * rp + (size_t)x0 * 3;
        if (n == INTERP_RUN && ((size_t)src & 3) == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned int w = ((const unsigned int*)src)[j];
                bytes[4 * j] = (unsigned char)w, bytes[4 * j + 1] = (unsigned char)(w >> 8);
                bytes[4 * j + 2] = (unsigned char)(w >> 16), bytes[4 * j + 3] = (unsigned char)(w >> 24);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3 * INTERP_RUN; ++j) bytes[j] = j < 3 * n ? src[j] : 0;
        }
        interp_store(out + (size_t)i * N * ofp + ((size_t)y * W + x0) * 3, bytes, n);
        if (i >= F - 1 || N < 2) continue;
        const unsigned char* B = A + fp;
        const float2* ab = fab + (size_t)i * H * W;
        const float2* ba = fba + (size_t)i * H * W;
        float2 uab[INTERP_RUN], uba[INTERP_RUN];                         // this thread's flows: loaded once, used for every k
#pragma unroll
        for (int j = 0; j < INTERP_RUN; ++j) {
            const size_t o = (size_t)y * W + min(x0 + j, W - 1);
            uab[j] = ab[o];
            uba[j] = ba[o];
        }
        for (int k = 1; k < N; ++k) {
            const float t = (float)k / (float)N, a = (float)(N - k) / (float)N;
            const float tt = t * t, aa = a * a, at = a * t;
#pragma unroll
            for (int j = 0; j < INTERP_RUN; ++j) {
                if (j >= n) break;
                float sa[3], sb[3], va, vb;
                interp_side(A, rp, ab, ba, H, W, x0 + j, y, tt * uba[j].x - at * uab[j].x, tt * uba[j].y - at * uab[j].y, sa, va);
                interp_side(B, rp, ba, ab, H, W, x0 + j, y, aa * uab[j].x - at * uba[j].x, aa * uab[j].y - at * uba[j].y, sb, vb);
                float wa = a * va, wb = t * vb;
                if (!(wa + wb > 0.f)) {                                   // both sides invisible: the plain blend of the samples
                    wa = a;
                    wb = t;
                }
                const float den = wa + wb;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float o = (wa * sa[c] + wb * sb[c]) / den;
                    bytes[3 * j + c] = (unsigned char)fminf(fmaxf(floorf(o + 0.5f), 0.f), 255.f);
                }
            }
            interp_store(out + ((size_t)i * N + k) * ofp + ((size_t)y * W + x0) * 3, bytes, n);
        }
    }
}

extern "C" int vdx_interp_frames_u8(const void* frames, size_t frame_pitch, int row_pitch, const float* fab, const float* fba, int F,
                                    int H, int W, int N, void* out, size_t out_frame_pitch, vdx_stream_t stream) {
    VDX_CHECK(frames && out, "interp_frames: null pointer");
    VDX_CHECK(F >= 1 && F <= 65536, "interp_frames: F=%d", F);
    VDX_CHECK(N >= 1 && N <= 64, "interp_frames: N=%d", N);
    VDX_CHECK(H > 0 && W > 0 && (long long)H * W < (1ll << 30), "interp_frames: H=%d W=%d", H, W);
    VDX_CHECK(row_pitch >= 3 * W && frame_pitch >= (size_t)row_pitch * H, "interp_frames: pitches too small");
    VDX_CHECK(out_frame_pitch >= (size_t)3 * W * H, "interp_frames: out_frame_pitch too small");
    VDX_CHECK(fab && fba, "interp_frames: null flow pointer");
    VDX_CHECK((size_t)fab % 8 == 0 && (size_t)fba % 8 == 0, "interp_frames: flow pointers must be 8-byte aligned");
    const int groups = (W + INTERP_RUN - 1) / INTERP_RUN;
    const long long total = (long long)F * H * groups;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(interp_frames_kernel, dim3((int)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)frames, frame_pitch, row_pitch, (const float2*)fab, (const float2*)fba, F, H, W, N, groups,
                       total, (unsigned char*)out, out_frame_pitch);
    return vdx_launch_status("vdx_interp_frames_u8");
}
