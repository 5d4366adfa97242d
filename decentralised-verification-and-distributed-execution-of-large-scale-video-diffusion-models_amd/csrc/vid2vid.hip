// vid2vid.hip — the front end of video-to-video refinement (diffusers VideoToVideoSDPipeline, Zeroscope v2 XL's second stage):
// Pillow's resize of the first-stage frames, the [-1, 1] map written straight into the encoder's conv_in operand, the
// diagonal-Gaussian posterior -> scaled latent, and DDIMScheduler.add_noise.  The encoder's convolutions, GroupNorms and
// attention run on the UNet's kernels (vdx/vae.py); the (0,1,0,1) padding of its Downsample2D is gemm.hip's pad_mode 1.
// Every element-wise map here rounds to fp16 after each op, as the torch evaluation it restates does.
#include "vdx_common.h"
#include "step_chains.h"

namespace {

// fp32 -> fp16 as its own rounding step: the empty asm keeps hipcc from narrowing the fp32 op before it to fp16 and fusing
// it with the next one (v_fma_mixlo_f16 / v_fma_f16: one rounding where torch has two), as elementwise.hip's rn16 does
__device__ __forceinline__ f16 h16(float x) {
    asm volatile("" : "+v"(x));
    return (f16)x;
}

__device__ __forceinline__ int clip8_22(int acc) {     // Pillow's clip8 at PRECISION_BITS = 22
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---- Pillow ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc (one thread per output pixel, 3 channels) ----
__global__ __launch_bounds__(256) void resample_h_kernel(const unsigned char* in, size_t ifp, int irp, int F, int H, int Wi,
                                                         const int2* bounds, const int32_t* coeffs, int ksize, int Wo,
                                                         unsigned char* out, size_t ofp, int orp) {
    const long long total = (long long)F * H * Wo;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(idx % Wo);
        const long long fy = idx / Wo;
        const int y = (int)(fy % H), f = (int)(fy / H);
        const unsigned char* row = in + (size_t)f * ifp + (size_t)y * irp;
        const int2 b = bounds[ox];
        const int n = min(b.y, ksize);
        const int32_t* k = coeffs + (size_t)ox * ksize;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int j = 0; j < n; ++j) {
            const unsigned char* px = row + (size_t)min(max(b.x + j, 0), Wi - 1) * 3;
            const int kj = k[j];
            a0 += (int)px[0] * kj;
            a1 += (int)px[1] * kj;
            a2 += (int)px[2] * kj;
        }
        unsigned char* o = out + (size_t)f * ofp + (size_t)y * orp + (size_t)ox * 3;
        o[0] = (unsigned char)clip8_22(a0);
        o[1] = (unsigned char)clip8_22(a1);
        o[2] = (unsigned char)clip8_22(a2);
    }
}

__global__ __launch_bounds__(256) void resample_v_kernel(const unsigned char* in, size_t ifp, int irp, int F, int Hi, int W,
                                                         const int2* bounds, const int32_t* coeffs, int ksize, int Ho,
                                                         unsigned char* out, size_t ofp, int orp) {
    const long long total = (long long)F * Ho * W;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % W);
        const long long fy = idx / W;
        const int oy = (int)(fy % Ho), f = (int)(fy / Ho);
        const unsigned char* col = in + (size_t)f * ifp + (size_t)x * 3;
        const int2 b = bounds[oy];
        const int n = min(b.y, ksize);
        const int32_t* k = coeffs + (size_t)oy * ksize;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int j = 0; j < n; ++j) {
            const unsigned char* px = col + (size_t)min(max(b.x + j, 0), Hi - 1) * irp;
            const int kj = k[j];
            a0 += (int)px[0] * kj;
            a1 += (int)px[1] * kj;
            a2 += (int)px[2] * kj;
        }
        unsigned char* o = out + (size_t)f * ofp + (size_t)oy * orp + (size_t)x * 3;
        o[0] = (unsigned char)clip8_22(a0);
        o[1] = (unsigned char)clip8_22(a1);
        o[2] = (unsigned char)clip8_22(a2);
    }
}

// ---- uint8 frames -> conv_in im2col rows: one thread per output row, 8 x 16-byte stores ---------------------------------
__global__ __launch_bounds__(256) void frames_to_conv_in_kernel(const unsigned char* frames, size_t fp, int rp, int F, int H,
                                                                int W, const f16* lut, f16* out, int ldo) {
    __shared__ f16 tab[256];
    tab[threadIdx.x] = lut[threadIdx.x];            // blockDim.x == 256
    __syncthreads();
    const long long total = (long long)F * H * W;
    for (long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x; pix < total; pix += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(pix % W);
        const long long fy = pix / W;
        const int y = (int)(fy % H), f = (int)(fy / H);
        const unsigned char* img = frames + (size_t)f * fp;
        f16 v[32];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const bool ok = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const unsigned char* px = img + (size_t)(ok ? yy : 0) * rp + (size_t)(ok ? xx : 0) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[tap * 3 + c] = ok ? tab[px[c]] : (f16)0.f;   // the conv pads the normalised image
        }
#pragma unroll
        for (int j = 27; j < 32; ++j) v[j] = (f16)0.f;
        f16* o = out + (size_t)pix * ldo;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f16x8 w;
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = v[q * 8 + j];
            *(f16x8*)(o + q * 8) = w;
        }
        const f16x8 z = {};
#pragma unroll
        for (int q = 4; q < 8; ++q) *(f16x8*)(o + q * 8) = z;
    }
}

// ---- DiagonalGaussianDistribution -> scaled latent ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void posterior_kernel(const f16* m, int ld, int n, int hw, const f16* eps, int mode_only,
                                                        float scale, f16* out, size_t cs, size_t fs) {
    const long long total = (long long)n * 4 * hw;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int p = (int)(idx % hw);
        const long long ic = idx / hw;
        const int c = (int)(ic % 4), i = (int)(ic / 4);
        const f16* row = m + ((size_t)i * hw + p) * ld;
        f16 x = row[c];
        if (!mode_only) {
            const float lv = fminf(fmaxf((float)row[4 + c], -30.f), 20.f);          // clamp: exact in fp16
            const f16 half_lv = h16(__fmul_rn(0.5f, lv));
            const f16 sd = h16(expf((float)half_lv));
            const f16 se = h16(__fmul_rn((float)sd, (float)eps[idx]));           // eps (n,4,h,w): flat index = idx
            x = h16(__fadd_rn((float)x, (float)se));
        }
        out[(size_t)c * cs + (size_t)i * fs + p] = h16(__fmul_rn((float)x, scale));
    }
}

__global__ __launch_bounds__(256) void add_noise_kernel(const f16* x0, const f16* noise, f16* out, float sa, float s1, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        out[i] = add_noise_elem((float)x0[i], (float)noise[i], sa, s1);     // step_chains.h: shared with inpaint.hip
    }
}

int grid_for(long long total) {
    const long long b = (total + 255) / 256;
    return (int)(b < 65536 ? (b > 0 ? b : 1) : 65536);
}

}  // namespace

extern "C" int vdx_resample_h_u8(const void* in, size_t in_frame_pitch, int in_row_pitch, int F, int H, int Wi,
                                 const int32_t* bounds, const int32_t* coeffs, int ksize, int Wo, void* out,
                                 size_t out_frame_pitch, int out_row_pitch, vdx_stream_t stream) {
    VDX_CHECK(in && out && bounds && coeffs, "resample_h: null pointer");
    VDX_CHECK(F > 0 && H > 0 && Wi > 0 && Wo > 0 && ksize > 0, "resample_h: F=%d H=%d Wi=%d Wo=%d ksize=%d", F, H, Wi, Wo, ksize);
    VDX_CHECK(in_row_pitch >= 3 * Wi && in_frame_pitch >= (size_t)in_row_pitch * H, "resample_h: input pitches too small");
    VDX_CHECK(out_row_pitch >= 3 * Wo && out_frame_pitch >= (size_t)out_row_pitch * H, "resample_h: output pitches too small");
    hipLaunchKernelGGL(resample_h_kernel, dim3(grid_for((long long)F * H * Wo)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)in, in_frame_pitch, in_row_pitch, F, H, Wi, (const int2*)bounds, coeffs, ksize, Wo,
                       (unsigned char*)out, out_frame_pitch, out_row_pitch);
    return vdx_launch_status("vdx_resample_h_u8");
}

extern "C" int vdx_resample_v_u8(const void* in, size_t in_frame_pitch, int in_row_pitch, int F, int Hi, int W,
                                 const int32_t* bounds, const int32_t* coeffs, int ksize, int Ho, void* out,
                                 size_t out_frame_pitch, int out_row_pitch, vdx_stream_t stream) {
    VDX_CHECK(in && out && bounds && coeffs, "resample_v: null pointer");
    VDX_CHECK(F > 0 && Hi > 0 && W > 0 && Ho > 0 && ksize > 0, "resample_v: F=%d Hi=%d W=%d Ho=%d ksize=%d", F, Hi, W, Ho, ksize);
    VDX_CHECK(in_row_pitch >= 3 * W && in_frame_pitch >= (size_t)in_row_pitch * Hi, "resample_v: input pitches too small");
    VDX_CHECK(out_row_pitch >= 3 * W && out_frame_pitch >= (size_t)out_row_pitch * Ho, "resample_v: output pitches too small");
    hipLaunchKernelGGL(resample_v_kernel, dim3(grid_for((long long)F * Ho * W)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)in, in_frame_pitch, in_row_pitch, F, Hi, W, (const int2*)bounds, coeffs, ksize, Ho,
                       (unsigned char*)out, out_frame_pitch, out_row_pitch);
    return vdx_launch_status("vdx_resample_v_u8");
}

extern "C" int vdx_frames_to_conv_in_u8(const void* frames, size_t frame_pitch, int row_pitch, int F, int H, int W,
                                        const void* lut_f16, void* out_rows, int ldo, vdx_stream_t stream) {
    VDX_CHECK(frames && lut_f16 && out_rows, "frames_to_conv_in: null pointer");
    VDX_CHECK(F > 0 && H > 0 && W > 0, "frames_to_conv_in: F=%d H=%d W=%d", F, H, W);
    VDX_CHECK(row_pitch >= 3 * W && frame_pitch >= (size_t)row_pitch * H, "frames_to_conv_in: pitches too small");
    VDX_CHECK(ldo >= 64 && ldo % 8 == 0, "frames_to_conv_in: ldo=%d (needs >= 64, a multiple of 8)", ldo);
    VDX_CHECK(((uintptr_t)out_rows & 15) == 0, "frames_to_conv_in: out_rows must be 16-byte aligned (16-byte stores)");
    hipLaunchKernelGGL(frames_to_conv_in_kernel, dim3(grid_for((long long)F * H * W)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)frames, frame_pitch, row_pitch, F, H, W, (const f16*)lut_f16, (f16*)out_rows, ldo);
    return vdx_launch_status("vdx_frames_to_conv_in_u8");
}

extern "C" int vdx_vae_posterior_f16(const void* moments, int ld, int n, int hw, const void* eps, int mode_only, float scale,
                                     void* out, size_t out_c_stride, size_t out_f_stride, vdx_stream_t stream) {
    VDX_CHECK(moments && out && (mode_only || eps), "vae_posterior: null pointer");
    VDX_CHECK(n > 0 && hw > 0 && ld >= 8, "vae_posterior: n=%d hw=%d ld=%d", n, hw, ld);
    hipLaunchKernelGGL(posterior_kernel, dim3(grid_for((long long)n * 4 * hw)), dim3(256), 0, (hipStream_t)stream,
                       (const f16*)moments, ld, n, hw, (const f16*)eps, mode_only, scale, (f16*)out, out_c_stride, out_f_stride);
    return vdx_launch_status("vdx_vae_posterior_f16");
}

extern "C" int vdx_add_noise_f16(const void* x0, const void* noise, void* out, float sqrt_ab, float sqrt_1mab, size_t n,
                                 vdx_stream_t stream) {
    VDX_CHECK(x0 && noise && out && n > 0, "add_noise: bad arguments");
    hipLaunchKernelGGL(add_noise_kernel, dim3(grid_for((long long)n)), dim3(256), 0, (hipStream_t)stream, (const f16*)x0,
                       (const f16*)noise, (f16*)out, sqrt_ab, sqrt_1mab, n);
    return vdx_launch_status("vdx_add_noise_f16");
}
