// freenoise.hip — FreeNoise (Qiu et al., "FreeNoise: Tuning-Free Longer Video Diffusion via Noise Rescheduling", ICLR 2024;
// diffusers' enable_free_noise(context_length, context_stride, weighting_scheme, noise_type), restated and unpinned) on the
// UNet's rows (no reference counterpart: the reference makes a long clip from whole-UNet windows only).  vdx/unet3d.py calls
// the attention core in every temporal transformer while `enable_free_noise` is set and F > context_length; vdx/pipeline.py
// calls the gather once per job, on the start noise.  tests/freenoise_ref.py states both definitions.
//
// temporal_attn_windows_kernel: window-fused temporal attention.  For one (b, pixel, head) item with q, k, v the F x 64 blocks
//   of vdx_temporal_attn_f16's qkv rows, windows i = 0 .. n-1 of L frames at s_i = min(i S, F - L), n = ceil((F - L) / S) + 1:
//
//     O_i    = softmax(scale Q_i K_i^T) V_i                                  over window i's L frames only
//     out[t] = fp16( sum_{i : s_i <= t < s_i + L} wn[i][t - s_i] O_i[t - s_i] )   fp32, ascending i, one rounding
//
//   Work split.  A block holds FN_IPB(F) whole items; it copies their k and v blocks from HBM to LDS once, 16 bytes per lane,
//   and every window of every wave reads its operands from there: an element of k or v is read from HBM once although its
//   frame sits in up to ceil(L / S) windows.  A wave owns 32 consecutive OUTPUT frames of one item.  It reads their q rows from
//   HBM straight into the B operand's registers (no other wave needs them) and then visits, in ascending i, the windows that
//   touch its frames.  Per window: S^T = K_i Q^T is one 32x32 tile of v_mfma_f32_32x32x16_f16 with the wave's own 32 frames as
//   the queries and the window's L <= 32 frames as the key slots; key slots >= L are masked to NEG_BIG before the row maximum
//   and their k and v operands are zeros, not what follows in LDS; the softmax is complete in registers, P is normalised and
//   rounded to fp16, O = P V is four more MFMAs.  O's rows are the wave's output frames whatever s_i is, so no row ever moves
//   between lanes or registers: a row t inside the window adds wn[i][t - s_i] O[t] to its fp32 accumulator (a product, then an
//   add, each rounded on its own), a row outside it is left alone by a select.  Each output row is written once, at the end.
//   LDS image.  Per item slot: K[F][FN_LD] then V[F][FN_LD] fp16, FN_LD = 72: rows of 64 padded by 16 bytes so the 16-byte
//   operand reads of 32 consecutive rows spread over the banks.  2 * 144 F bytes per item, 36 KB per block at most.
//   No atomics and one fixed order: the same bits on every run and for any B and HW.  No index is computed from data: NaN and
//   inf stay inside their (pixel, head), and inside the query rows and windows that hold them.
//
// frame_gather_kernel: dst[c][t] = src[c][idx[t]] on a (1, C, T, h, w) latent, the start noise's rescheduling.
#include "attn_common.h"

#define FN_THREADS 256
#define FN_WAVES (FN_THREADS / 64)
#define FN_LD 72                                      // halfs per LDS row: 64 + 8 of padding

// items of a block: as many as keep every wave busy with one 32-frame output block each
static inline int fn_ipb(int nqb) { return nqb == 1 ? 4 : nqb == 2 ? 2 : 1; }

struct WinP {
    const f16* qkv;
    f16* out;
    const float* wn;
    int ldqkv, ldo, B, F, HW, heads, nqb, ipb, L, S, n;
    float c;
    long long items;
};

__global__ __launch_bounds__(FN_THREADS) void temporal_attn_windows_kernel(const WinP p) {
    extern __shared__ __attribute__((aligned(16))) f16 fn_lds[];
    const int lane = threadIdx.x & 63, r32 = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    const int inner = p.heads * 64;
    const int F = p.F, L = p.L;
    const size_t fstride = (size_t)p.HW * p.ldqkv;     // one frame further, in halfs
    const int slot_halfs = 2 * F * FN_LD;
    const f16* zp = (const f16*)g_zero_page;

    // ---- stage the items' k and v blocks: HBM -> LDS, once ------------------------------------------------------------------
    for (int slot = 0; slot < p.ipb; ++slot) {
        const long long item = (long long)blockIdx.x * p.ipb + slot;
        if (item >= p.items) break;
        const int head = (int)(item % p.heads);
        const long long bp = item / p.heads;
        const int pix = (int)(bp % p.HW), b = (int)(bp / p.HW);
        const f16* kbase = p.qkv + ((size_t)b * F * p.HW + pix) * p.ldqkv + inner + head * 64;
        f16* dstb = fn_lds + slot * slot_halfs;
        for (int c = threadIdx.x; c < 2 * F * 8; c += FN_THREADS) {
            const int c8 = c & 7, r = c >> 3;
            const int m = r >= F ? 1 : 0, f = r - m * F;            // m: 0 = k, 1 = v
            *(f16x8*)(dstb + r * FN_LD + c8 * 8) = *(const f16x8*)(kbase + (size_t)f * fstride + m * inner + c8 * 8);
        }
    }
    __syncthreads();

    // ---- a wave per (item, block of 32 output frames) ------------------------------------------------------------------------
    for (int u = wave; u < p.ipb * p.nqb; u += FN_WAVES) {
        const int slot = u / p.nqb, qblk = u - slot * p.nqb;
        const long long item = (long long)blockIdx.x * p.ipb + slot;
        if (item >= p.items) continue;
        const int head = (int)(item % p.heads);
        const long long bp = item / p.heads;
        const int pix = (int)(bp % p.HW), b = (int)(bp / p.HW);
        const size_t row0 = (size_t)b * F * p.HW + pix;             // frame f lives at row0 + f*HW
        const f16* Ks = fn_lds + slot * slot_halfs;
        const f16* Vs = Ks + F * FN_LD;
        const int qf0 = qblk * 32;                                  // first output (= query) frame of this wave

        // B operand of S^T = K.Q^T: lane = query frame, from HBM (each q row belongs to one wave)
        f16x8 qf[4];
        {
            const int qr = qf0 + r32;
            const f16* qsrc = p.qkv + (row0 + (size_t)qr * p.HW) * p.ldqkv + head * 64 + 8 * h;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const f16x8*)(qr < F ? qsrc + 16 * ks : zp);
        }
        f32x16 acc[2];
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[db][j] = 0.f;

        for (int i = 0; i < p.n; ++i) {
            const int si = min(i * p.S, F - L);                     // si + L <= F: every key slot < L is a frame of the clip
            if (si >= qf0 + 32 || si + L <= qf0) continue;          // wave-uniform: the window touches none of these frames
            // A operand: K rows of the window fed through pi (attn_common.h); slots >= L are zeros
            f32x16 s_acc;
            {
                const int kk = pi_row(r32);
                const bool ok = kk < L;
                const f16* ksrc = Ks + (si + (ok ? kk : 0)) * FN_LD + 8 * h;
                const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 16; ++j) s_acc[j] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const f16x8 ld = *(const f16x8*)(ksrc + 16 * ks);
                    s_acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ok ? ld : zero, qf[ks], s_acc, 0, 0, 0);
                }
            }
            // V as B operand of O = P.V: lane = column d, element j of k-step s = V[si + 16s + 8h + j][d]; slots >= L zeros
            const int nks = L > 16 ? 2 : 1;                         // k-step 1 holds slots 16..31: all masked when L <= 16
            f16x8 vf[2][2];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int key = 16 * s + 8 * h + j;
                    const bool ok = key < L;
                    const f16* src = Vs + (si + (ok ? key : 0)) * FN_LD + r32;
                    const f16 a = src[0], c = src[32];
                    vf[0][s][j] = ok ? a : (f16)0;
                    vf[1][s][j] = ok ? c : (f16)0;
                }
            // complete softmax over the window's L keys, in registers; P normalised before the second product
            float mx = NEG_BIG;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (acc_key(j, h) >= L) s_acc[j] = NEG_BIG;
                mx = fmaxf(mx, s_acc[j]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mc = mx * p.c;
            float rs = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                s_acc[j] = __builtin_amdgcn_exp2f(s_acc[j] * p.c - mc);
                rs += s_acc[j];
            }
            const float inv = 1.0f / (rs + __shfl_xor(rs, 32, 64));
            f16x8 pf[2];
#pragma unroll
            for (int j = 0; j < 16; ++j) pf[j >> 3][j & 7] = (f16)(s_acc[j] * inv);
            // O = P.V (rows = this wave's output frames), then acc += wn[i][t - si] * O on the rows inside the window
            const float* wrow = p.wn + (size_t)i * L;
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                f32x16 o;
#pragma unroll
                for (int j = 0; j < 16; ++j) o[j] = 0.f;
                o = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf[0], vf[db][0], o, 0, 0, 0);
                if (nks == 2) o = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf[1], vf[db][1], o, 0, 0, 0);
                // C layout: col = lane&31 = d, row(reg) = (reg&3) + 8*(reg>>2) + 4*h = output frame - qf0
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int rel = qf0 + (j & 3) + 8 * (j >> 2) + 4 * h - si;
                    const bool in = rel >= 0 && rel < L;
                    const float w = wrow[in ? rel : 0];
                    const float prod = w * o[j];
                    const float sum = acc[db][j] + prod;
                    acc[db][j] = in ? sum : acc[db][j];
                }
            }
        }
        // every frame of the clip lies in a window (S <= L, the last one ends at F): each row below was accumulated
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            f16* dst = p.out + row0 * p.ldo + head * 64 + 32 * db + r32;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int f = qf0 + (j & 3) + 8 * (j >> 2) + 4 * h;
                if (f < F) dst[(size_t)f * p.HW * p.ldo] = (f16)acc[db][j];
            }
        }
    }
}

extern "C" int vdx_temporal_attn_windows_f16(const void* qkv, int ldqkv, void* out, int ldo, int B, int F, int HW, int heads,
                                             float scale, int L, int S, const float* wn, vdx_stream_t stream) {
    VDX_CHECK(qkv && out && wn, "temporal_attn_windows: null pointer");
    VDX_CHECK(B > 0 && F > 0 && HW > 0 && heads > 0, "temporal_attn_windows: empty problem");
    VDX_CHECK(L >= 2 && L <= 32, "temporal_attn_windows: context length L=%d outside [2, 32]", L);
    VDX_CHECK(S >= 1 && S <= L, "temporal_attn_windows: context stride S=%d outside [1, L=%d]", S, L);
    VDX_CHECK(F > L && F <= 128, "temporal_attn_windows: F=%d frames outside (L=%d, 128]", F, L);
    VDX_CHECK(ldqkv % 8 == 0 && ldqkv >= 3 * heads * 64 && ldo >= heads * 64, "temporal_attn_windows: bad leading dims");
    VDX_CHECK((size_t)qkv % 16 == 0, "temporal_attn_windows: qkv must be 16-byte aligned");
    WinP p;
    p.qkv = (const f16*)qkv; p.out = (f16*)out; p.wn = wn; p.ldqkv = ldqkv; p.ldo = ldo;
    p.B = B; p.F = F; p.HW = HW; p.heads = heads; p.L = L; p.S = S;
    p.n = (F - L + S - 1) / S + 1;
    p.nqb = (F + 31) / 32;
    p.ipb = fn_ipb(p.nqb);
    p.c = scale * 1.44269504088896341f;
    p.items = (long long)B * HW * heads;
    const long long blocks = (p.items + p.ipb - 1) / p.ipb;
    VDX_CHECK(blocks < (1ll << 31), "temporal_attn_windows: too many items");
    const size_t lds = (size_t)p.ipb * 2 * F * FN_LD * sizeof(f16);          // 36 KB at most (F = 32, 64, 128)
    hipLaunchKernelGGL(temporal_attn_windows_kernel, dim3((unsigned)blocks), dim3(FN_THREADS), lds, (hipStream_t)stream, p);
    return vdx_launch_status("vdx_temporal_attn_windows_f16");
}

// VEC: eight elements per lane (HW % 8 == 0, both pointers 16-byte aligned)
template <bool VEC>
__global__ __launch_bounds__(FN_THREADS) void frame_gather_kernel(const f16* src, f16* dst, const int* idx, int T, size_t HW, size_t n) {
    const size_t per = VEC ? HW / 8 : HW;
    for (size_t i = (size_t)blockIdx.x * FN_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * FN_THREADS) {
        const size_t ct = i / per, q = i - ct * per;
        const size_t c = ct / T;
        const int t = (int)(ct - c * T);
        const int s = min(max(idx[t], 0), T - 1);                  // the host has checked the table: never moves a valid index
        const size_t from = (c * T + s) * HW, to = ct * HW;
        if (VEC)
            *((f16x8*)(dst + to) + q) = *((const f16x8*)(src + from) + q);
        else
            dst[to + q] = src[from + q];
    }
}

extern "C" int vdx_frame_gather_f16(const void* src, void* dst, const int32_t* idx, int C, int T, int HW, vdx_stream_t stream) {
    VDX_CHECK(src && dst && idx, "frame_gather: null pointer");
    VDX_CHECK(C >= 1 && T >= 1 && HW >= 1, "frame_gather: C=%d T=%d HW=%d (each at least 1)", C, T, HW);
    const size_t bytes = (size_t)C * T * HW * sizeof(f16);
    const char *a = (const char*)src, *b = (const char*)dst;
    VDX_CHECK(a + bytes <= b || b + bytes <= a, "frame_gather: dst may not overlap src");
    const bool vec = HW % 8 == 0 && (size_t)src % 16 == 0 && (size_t)dst % 16 == 0;
    const size_t n = (size_t)C * T * (vec ? HW / 8 : HW);
    const size_t blocks = (n + FN_THREADS - 1) / FN_THREADS, cap = (size_t)vdx_num_cus() * 16;
    const int grid = (int)(blocks < cap ? blocks : cap);
    if (vec)
        hipLaunchKernelGGL(frame_gather_kernel<true>, dim3(grid), dim3(FN_THREADS), 0, (hipStream_t)stream, (const f16*)src, (f16*)dst,
                           (const int*)idx, T, (size_t)HW, n);
    else
        hipLaunchKernelGGL(frame_gather_kernel<false>, dim3(grid), dim3(FN_THREADS), 0, (hipStream_t)stream, (const f16*)src, (f16*)dst,
                           (const int*)idx, T, (size_t)HW, n);
    return vdx_launch_status("vdx_frame_gather_f16");
}
