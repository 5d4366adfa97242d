// mjpeg.hip — baseline JPEG decode of a whole Motion-JPEG clip on the device: the read side of the validator's
// `cv2.VideoCapture(video_path)` (InferNet/template/validator/scoring.py:16, :110, :230, :272, :314) for the files
// vdx/compat/cv2_shim.py:199-289 writes.  Three stages, integers only, no atomics: the same bits on every run and for any
// number of frames per launch, and the bits of libjpeg's own decode (slow-integer IDCT, h2v2 "fancy" upsampling, the 16-bit
// fixed-point YCbCr -> RGB), which is what Pillow returns, for every frame whose coefficients lie in the range 8-bit samples
// produce; stage 2 flags the frames outside it (MJ_DOMAIN_* below), where decoders disagree, and the host refuses them.
// The host (vdx/video.py) walks the markers, builds the Huffman lookups from the stream's DHT segments and cuts the scan at
// its restart markers; nothing here trusts what it built beyond the checks below: the entropy bytes come from another machine.
#include "vdx_common.h"
#include "mjpeg_common.h"

#define MJ_HUFF_WORDS 384        // one Huffman table: 512 x u16 9-bit lookahead | maxcode[17] | valoff[17] | 256 symbols | pad
#define MJ_FAST_BITS 9
#define MJ_MAXCODE 256           // word offsets inside a table
#define MJ_VALOFF 273
#define MJ_SYMS 290

enum { MJ_OK = 0, MJ_ERR_DATA_END = 1, MJ_ERR_COEF_INDEX = 2, MJ_ERR_BAD_CODE = 3, MJ_ERR_DC_SIZE = 4, MJ_ERR_SEGMENT = 5 };

extern "C" size_t vdx_mjpeg_workspace(int F, int W, int H, int layout) {
    MjLayout L;
    if (F <= 0 || F > 65535 || mj_layout(W, H, layout, &L) != 0) return 0;
    const size_t samples = (size_t)F * L.bpf * 64;
    return mj_round(samples * 2) + mj_round(samples);            // int16 coefficients | uint8 component planes
}

// ---- stage 1: entropy decode ----------------------------------------------------------------------------------------------
// One lane per segment (a restart interval, or the whole scan of a frame without DRI); blockIdx.y is the frame, whose four
// Huffman tables the block stages in LDS.  Coefficients go de-zigzagged to [frame][block][64] int16, zeroed on the stream
// before the launch, so a lane stores the non-zero ones only.
//
// What bounds every access:
//   * bytes: the reader loads the aligned word holding byte `pos` only while pos < end, and end <= nbytes (clamped here;
//     the buffer holds nbytes, a multiple of 4).  Past the end it feeds zero bits and counts them; a symbol that consumed one
//     of them ends the lane with MJ_ERR_DATA_END;
//   * tables: lookups index LDS with 9 or at most 8 masked bits;
//   * coefficients: k is compared with 63 before the store, the block index follows from the MCU number alone, and the MCU
//     range is clamped to the frame's MCU count.
struct MjBits {
    const uint32_t* words;
    uint32_t pos, end, cur, cur_idx;
    unsigned long long buf;
    int bits, pad;
};
__device__ __forceinline__ uint32_t mj_byte(MjBits& b, uint32_t p) {        // p < end <= nbytes
    const uint32_t idx = p >> 2;
    if (idx != b.cur_idx) {
        b.cur = b.words[idx];
        b.cur_idx = idx;
    }
    return (b.cur >> ((p & 3) * 8)) & 255u;
}
__device__ __forceinline__ void mj_refill(MjBits& b) {
    while (b.bits <= 56) {
        uint32_t v = 0;
        if (b.pos < b.end) {
            v = mj_byte(b, b.pos++);
            if (v == 0xFF) {
                if (b.pos < b.end && mj_byte(b, b.pos) == 0) ++b.pos;      // FF 00: a stuffed FF
                else { b.pos = b.end; v = 0; b.pad += 8; }                 // a marker inside the segment: the data ends here
            }
        } else {
            b.pad += 8;
        }
        b.buf |= (unsigned long long)v << (56 - b.bits);
        b.bits += 8;
    }
}
__device__ __forceinline__ void mj_skip(MjBits& b, int n) { b.buf <<= n; b.bits -= n; }
// one Huffman symbol from table t (LDS); -1 when no code of up to 16 bits matches.  Needs >= 16 bits in the buffer.
__device__ __forceinline__ int mj_symbol(MjBits& b, const uint32_t* t) {
    const uint32_t peek = (uint32_t)(b.buf >> 48);
    const uint32_t fi = peek >> (16 - MJ_FAST_BITS);                        // < 512
    const uint32_t e = (t[fi >> 1] >> ((fi & 1) * 16)) & 0xFFFFu;
    if (e) {
        mj_skip(b, (int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int l = MJ_FAST_BITS + 1; l <= 16; ++l) {
        const int code = (int)(peek >> (16 - l));
        if (code <= (int)t[MJ_MAXCODE + l]) {
            const uint32_t i = (t[MJ_VALOFF + l] + (uint32_t)code) & 255u;
            mj_skip(b, l);
            return (int)((t[MJ_SYMS + (i >> 2)] >> ((i & 3) * 8)) & 255u);
        }
    }
    return -1;
}
__device__ __forceinline__ int mj_receive_extend(MjBits& b, int s) {        // 1 <= s <= 15
    const int v = (int)(b.buf >> (64 - s));
    mj_skip(b, s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

__global__ __launch_bounds__(64) void mjpeg_entropy_kernel(const uint32_t* data, uint32_t nbytes, const int* seg_off, const int* segs,
                                                           int nseg, int spb, const uint32_t* huff, const int* sel, MjLayout L,
                                                           short* coef, uint32_t* err) {
    __shared__ uint32_t tab[4 * MJ_HUFF_WORDS];
    const int f = blockIdx.y;
    for (int i = threadIdx.x; i < 4 * MJ_HUFF_WORDS; i += blockDim.x) tab[i] = huff[(size_t)f * 4 * MJ_HUFF_WORDS + i];
    __syncthreads();
    if ((int)threadIdx.x >= spb) return;
    const int s0 = min(max(seg_off[f], 0), nseg), s1 = min(max(seg_off[f + 1], s0), nseg);
    const int s = s0 + blockIdx.x * spb + threadIdx.x;
    if (s >= s1) return;

    MjBits b;
    b.words = data;
    b.end = min((uint32_t)segs[4 * s + 1], nbytes);
    b.pos = min((uint32_t)segs[4 * s], b.end);
    b.cur = 0;
    b.cur_idx = 0xFFFFFFFFu;
    b.buf = 0;
    b.bits = 0;
    b.pad = 0;
    const uint32_t m0 = min((uint32_t)segs[4 * s + 2], (uint32_t)L.nmcu);
    const uint32_t mc = min((uint32_t)segs[4 * s + 3], (uint32_t)L.nmcu - m0);
    if (m0 != (uint32_t)segs[4 * s + 2] || mc != (uint32_t)segs[4 * s + 3] || b.pos != (uint32_t)segs[4 * s] ||
        b.end != (uint32_t)segs[4 * s + 1]) {
        err[s] = MJ_ERR_SEGMENT;                                            // a row of the segment table outside the clip
        return;
    }
    short* fcoef = coef + (size_t)f * L.bpf * 64;
    int pred[3] = {0, 0, 0};                                                // DC prediction restarts with the segment
    for (uint32_t m = m0; m < m0 + mc; ++m) {
        const int my = (int)(m / (uint32_t)L.mcux), mx = (int)(m % (uint32_t)L.mcux);
        for (int c = 0; c < L.ncomp; ++c) {
            const int sc = sel[f * 3 + c];
            const uint32_t* dct = tab + (sc & 1) * MJ_HUFF_WORDS;
            const uint32_t* act = tab + (2 + ((sc >> 4) & 1)) * MJ_HUFF_WORDS;
            for (int by = 0; by < L.v[c]; ++by)
                for (int bx = 0; bx < L.h[c]; ++bx) {
                    short* blk = fcoef + (size_t)(L.boff[c] + (my * L.v[c] + by) * L.bw[c] + mx * L.h[c] + bx) * 64;
                    uint32_t code = MJ_OK;
                    // DC
                    if (b.bits < 32) mj_refill(b);
                    int sym = mj_symbol(b, dct);
                    if (sym < 0) code = MJ_ERR_BAD_CODE;
                    else if (sym > 15) code = MJ_ERR_DC_SIZE;
                    else {
                        if (sym) pred[c] += mj_receive_extend(b, sym);
                        if (b.pad > b.bits) code = MJ_ERR_DATA_END;
                    }
                    if (code == MJ_OK) {
                        if (pred[c]) blk[0] = (short)pred[c];
                        // AC
                        int k = 1;
                        while (k < 64) {
                            if (b.bits < 32) mj_refill(b);
                            sym = mj_symbol(b, act);
                            if (sym < 0) { code = MJ_ERR_BAD_CODE; break; }
                            const int r = sym >> 4, sz = sym & 15;
                            int val = 0;
                            if (sz == 0) {
                                if (b.pad > b.bits) { code = MJ_ERR_DATA_END; break; }
                                if (r != 15) break;                           // EOB
                                k += 16;                                      // ZRL
                                continue;
                            }
                            k += r;
                            val = mj_receive_extend(b, sz);
                            if (b.pad > b.bits) { code = MJ_ERR_DATA_END; break; }
                            if (k > 63) { code = MJ_ERR_COEF_INDEX; break; }   // before the store
                            blk[mj_natural[k]] = (short)val;
                            ++k;
                        }
                    }
                    if (code != MJ_OK) {
                        err[s] = code | ((m - m0) << 8);
                        return;
                    }
                }
        }
    }
    err[s] = MJ_OK;
}

extern "C" int vdx_mjpeg_entropy(const void* data, size_t nbytes, const int32_t* seg_off, const int32_t* segs, int nseg,
                                 int max_segs_per_frame, const void* huff, const int32_t* sel, int F, int W, int H, int layout,
                                 void* workspace, uint32_t* err, vdx_stream_t stream) {
    MjLayout L;
    VDX_CHECK(data && seg_off && segs && huff && sel && workspace && err, "mjpeg_entropy: null pointer");
    VDX_CHECK(F > 0 && F <= 65535 && mj_layout(W, H, layout, &L) == 0, "mjpeg_entropy: F=%d W=%d H=%d layout=%d", F, W, H, layout);
    VDX_CHECK(nbytes > 0 && nbytes % 4 == 0 && nbytes < (1ull << 31), "mjpeg_entropy: nbytes=%zu (a multiple of 4 below 2^31)", nbytes);
    VDX_CHECK(nseg >= F && max_segs_per_frame >= 1 && max_segs_per_frame <= nseg, "mjpeg_entropy: nseg=%d, %d per frame at most", nseg,
              max_segs_per_frame);
    VDX_CHECK((long long)F * L.bpf < (1ll << 25), "mjpeg_entropy: the clip has too many blocks");
    VDX_CHECK((((uintptr_t)data | (uintptr_t)huff | (uintptr_t)seg_off | (uintptr_t)segs | (uintptr_t)sel | (uintptr_t)err) & 3) == 0 &&
                  ((uintptr_t)workspace & 15) == 0,
              "mjpeg_entropy: misaligned pointer");
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)F * L.bpf * 64 * 2, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(err, 0xFF, (size_t)nseg * 4, (hipStream_t)stream);   // a segment no lane visits reads as an error
    VDX_CHECK(e == hipSuccess, "mjpeg_entropy: memset failed: %s", hipGetErrorString(e));
    // segments per block: spread the lanes over the CUs (a lane's time is latency, not issue slots), 64 per block at most
    int spb = (int)(((long long)F * max_segs_per_frame + vdx_num_cus() - 1) / vdx_num_cus());
    spb = spb < 1 ? 1 : (spb > 64 ? 64 : spb);
    hipLaunchKernelGGL(mjpeg_entropy_kernel, dim3((max_segs_per_frame + spb - 1) / spb, F), dim3(64), 0, (hipStream_t)stream,
                       (const uint32_t*)data, (uint32_t)nbytes, seg_off, segs, nseg, spb, (const uint32_t*)huff, sel, L,
                       (short*)workspace, err);
    return vdx_launch_status("vdx_mjpeg_entropy");
}

// ---- stage 2: dequantise + slow-integer IDCT --------------------------------------------------------------------------------
// The "islow" algorithm (Loeffler, Ligtenberg, Moschytz 1989, as in the Independent JPEG Group's decoder): 13-bit constants,
// pass 1 over columns keeps 2 extra bits, pass 2 over rows removes them with the factor 8; int32 (the file is built with
// -fwrapv: absurd coefficients of a corrupt stream wrap, they are never undefined).
#define MJ_CONST_BITS 13
#define MJ_PASS1_BITS 2
// The domain of the claim "the bits of libjpeg's decode".  An encoder that started from 8-bit samples leaves dequantised
// products, pass-1 values and pre-limit samples far inside these bounds.  Outside them libjpeg's C code (this arithmetic: int32,
// then a range-limit table indexed with 10 masked bits), libjpeg-turbo's 16-bit SIMD lanes and other decoders return different
// pixels for the same bytes, so there is nothing to be bit-equal to: the kernel sets the frame's word in `flags` and the host
// refuses the frame.  A frame is outside when a product c * q or a pass-1 value leaves [-B - 1, B] for its bound B below, or a
// pass-2 result before the range limit leaves [-512, 511] (tests/test_video_host.py measures the bounds against Pillow;
// profiles/mjpeg_domain.txt).
#define MJ_DOMAIN_PRODUCT 32767
#define MJ_DOMAIN_PASS1 32767
__device__ __forceinline__ void mj_idct8(const int* in, int* out, int shift) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 + z3 * -15137;
    int tmp3 = z1 + z2 * 6270;
    z2 = in[0];
    z3 = in[4];
    int tmp0 = (z2 + z3) << MJ_CONST_BITS;
    int tmp1 = (z2 - z3) << MJ_CONST_BITS;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 *= -16069;
    z4 *= -3196;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int rnd = 1 << (shift - 1);
    out[0] = (tmp10 + tmp3 + rnd) >> shift;
    out[7] = (tmp10 - tmp3 + rnd) >> shift;
    out[1] = (tmp11 + tmp2 + rnd) >> shift;
    out[6] = (tmp11 - tmp2 + rnd) >> shift;
    out[2] = (tmp12 + tmp1 + rnd) >> shift;
    out[5] = (tmp12 - tmp1 + rnd) >> shift;
    out[3] = (tmp13 + tmp0 + rnd) >> shift;
    out[4] = (tmp13 - tmp0 + rnd) >> shift;
}

// 256 threads = 32 blocks of 8x8.  Load: lane (block L>>3, row L&7) moves its row (16 bytes) to LDS.  Pass 1: the same lane
// takes COLUMN L&7 and leaves 8 int32 in LDS.  Pass 2: lane (row L>>3, block L&7 of the wave's eight) takes a row and writes 8
// bytes of the component plane, so one store instruction of a wave covers 8 rows of 64 contiguous bytes.
// LDS strides: raw int16 block 72 (a column read of a half-wave touches 4 x 4 distinct banks); workspace int32 row 9, block 76
// (12 b + 9 i + c is a bijection of (b < 8, i < 4) onto the 32 banks for every c).
#define MJ_RAW_STRIDE 72
#define MJ_WS_ROW 9
#define MJ_WS_BLK 76
__global__ __launch_bounds__(256) void mjpeg_idct_kernel(const short* coef, const unsigned short* quant, MjLayout L, long long nblocks,
                                                         unsigned char* planes, uint32_t* flags) {
    __shared__ __attribute__((aligned(16))) short raw[32 * MJ_RAW_STRIDE];
    __shared__ int ws[32 * MJ_WS_BLK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        const int lb = wave * 8 + (lane >> 3), j = lane & 7;
        const long long g = (long long)blockIdx.x * 32 + lb;
        u32x4 row = {0, 0, 0, 0};
        if (g < nblocks) row = *(const u32x4*)(coef + (size_t)g * 64 + j * 8);
        *(u32x4*)(raw + lb * MJ_RAW_STRIDE + j * 8) = row;
        __syncthreads();
        int in[8], out[8];
        if (g < nblocks) {
            const int f = (int)(g / L.bpf), bi = (int)(g % L.bpf);
            const int c = L.ncomp == 3 ? (bi >= L.boff[1]) + (bi >= L.boff[2]) : 0;
            const unsigned short* q = quant + ((size_t)f * 3 + c) * 64 + j;
#pragma unroll
            for (int r = 0; r < 8; ++r) in[r] = (int)raw[lb * MJ_RAW_STRIDE + r * 8 + j] * (int)q[r * 8];
            mj_idct8(in, out, MJ_CONST_BITS - MJ_PASS1_BITS);
            bool outside = false;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                ws[lb * MJ_WS_BLK + r * MJ_WS_ROW + j] = out[r];
                outside |= in[r] < -MJ_DOMAIN_PRODUCT - 1 || in[r] > MJ_DOMAIN_PRODUCT || out[r] < -MJ_DOMAIN_PASS1 - 1 ||
                           out[r] > MJ_DOMAIN_PASS1;
            }
            if (outside) flags[f] = 1;                                      // every writer stores the same word: no atomic
        }
        __syncthreads();
    }
    const int lb = wave * 8 + (lane & 7), i = lane >> 3;
    const long long g = (long long)blockIdx.x * 32 + lb;
    if (g >= nblocks) return;
    int in[8], out[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = ws[lb * MJ_WS_BLK + i * MJ_WS_ROW + c];
    mj_idct8(in, out, MJ_CONST_BITS + MJ_PASS1_BITS + 3);
    uint32_t px[2] = {0, 0};
    bool outside = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        // the decoder's range-limit table is indexed with 10 masked bits: sign-extend them, then +128 and clamp
        const int s = ((out[c] & 1023) ^ 512) - 512;
        outside |= s != out[c];                                             // outside [-512, 511]: the table is no clamp there
        px[c >> 2] |= (uint32_t)min(max(s + 128, 0), 255) << ((c & 3) * 8);
    }
    const int f = (int)(g / L.bpf), bi = (int)(g % L.bpf);
    if (outside) flags[f] = 1;
    const int c = L.ncomp == 3 ? (bi >= L.boff[1]) + (bi >= L.boff[2]) : 0;
    const int rel = bi - L.boff[c], by = rel / L.bw[c], bx = rel - by * L.bw[c];
    unsigned char* dst = planes + ((size_t)f * L.bpf + L.boff[c]) * 64 + (size_t)(by * 8 + i) * (L.bw[c] * 8) + bx * 8;
    *(uint2*)dst = make_uint2(px[0], px[1]);
}

extern "C" int vdx_mjpeg_idct(const void* quant_u16, int F, int W, int H, int layout, void* workspace, uint32_t* flags,
                              vdx_stream_t stream) {
    MjLayout L;
    VDX_CHECK(quant_u16 && workspace && flags, "mjpeg_idct: null pointer");
    VDX_CHECK(F > 0 && F <= 65535 && mj_layout(W, H, layout, &L) == 0, "mjpeg_idct: F=%d W=%d H=%d layout=%d", F, W, H, layout);
    VDX_CHECK((long long)F * L.bpf < (1ll << 25), "mjpeg_idct: the clip has too many blocks");
    VDX_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)quant_u16 & 1) == 0 && ((uintptr_t)flags & 3) == 0,
              "mjpeg_idct: misaligned pointer");
    const hipError_t e = hipMemsetAsync(flags, 0, (size_t)F * 4, (hipStream_t)stream);
    VDX_CHECK(e == hipSuccess, "mjpeg_idct: memset failed: %s", hipGetErrorString(e));
    const long long nb = (long long)F * L.bpf;
    unsigned char* planes = (unsigned char*)workspace + mj_round((size_t)nb * 64 * 2);
    hipLaunchKernelGGL(mjpeg_idct_kernel, dim3((unsigned)((nb + 31) / 32)), dim3(256), 0, (hipStream_t)stream, (const short*)workspace,
                       (const unsigned short*)quant_u16, L, nb, planes, flags);
    return vdx_launch_status("vdx_mjpeg_idct");
}

// ---- stage 3: chroma upsampling + colour conversion ----------------------------------------------------------------------
// h2v2 "fancy" (triangle) upsampling: vertically 3 near + far, horizontally (3 this + neighbour + 8 | 7) >> 4 for the left /
// right output of a chroma column, (4 this + 8 | 7) >> 4 at the first / last column; "far" and the edge columns replicate at
// the component's true size CW x CH = ceil(W/2) x ceil(H/2), not at the padded MCU extent.
__device__ __forceinline__ int mj_up420(const unsigned char* p, int pitch, int CW, int CH, int x, int y) {
    const int cy = y >> 1, cx = x >> 1;
    const int fy = (y & 1) ? min(cy + 1, CH - 1) : max(cy - 1, 0);
    const unsigned char *near = p + (size_t)cy * pitch, *far = p + (size_t)fy * pitch;
    const int cur = 3 * near[cx] + far[cx];
    if (x & 1) {
        if (cx == CW - 1) return (cur * 4 + 7) >> 4;
        return (cur * 3 + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    }
    if (cx == 0) return (cur * 4 + 8) >> 4;
    return (cur * 3 + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}
// R = Y + 1.40200 Cr, G = Y - 0.34414 Cb - 0.71414 Cr, B = Y + 1.77200 Cb with the constants scaled by 2^16 and rounded,
// one half added before the shift (for G: once, to the sum), then the clamp.  Returns R | G << 8 | B << 16.
__device__ __forceinline__ uint32_t mj_rgb(int y, int cb, int cr) {
    cb -= 128;
    cr -= 128;
    const int r = y + ((91881 * cr + 32768) >> 16);
    const int g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int b = y + ((116130 * cb + 32768) >> 16);
    return (uint32_t)min(max(r, 0), 255) | ((uint32_t)min(max(g, 0), 255) << 8) | ((uint32_t)min(max(b, 0), 255) << 16);
}
// One thread per 4 pixels of a row.  W % 4 == 0: three 4-byte stores (every row then starts on a 4-byte boundary);
// otherwise byte stores.
__global__ __launch_bounds__(256) void mjpeg_color_kernel(const unsigned char* planes, MjLayout L, int F, int W, int H, int layout,
                                                          unsigned char* out) {
    const int W4 = (W + 3) / 4;
    const long long total = (long long)F * H * W4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x0 = (int)(idx % W4) * 4;
        const long long fy = idx / W4;
        const int y = (int)(fy % H), f = (int)(fy / H);
        const unsigned char* fp = planes + (size_t)f * L.bpf * 64;
        const unsigned char* yp = fp + (size_t)y * (L.bw[0] * 8);
        const int n = min(4, W - x0);
        if (layout == 0) {
            unsigned char* o = out + ((size_t)f * H + y) * W + x0;
            if (n == 4 && W % 4 == 0) *(uint32_t*)o = *(const uint32_t*)(yp + x0);
            else
                for (int i = 0; i < n; ++i) o[i] = yp[x0 + i];
            continue;
        }
        const unsigned char* cbp = fp + (size_t)L.boff[1] * 64;
        const unsigned char* crp = fp + (size_t)L.boff[2] * 64;
        const int cpitch = L.bw[1] * 8;
        uint32_t px[4] = {0, 0, 0, 0};
        for (int i = 0; i < n; ++i) {
            const int x = x0 + i;
            int cb, cr;
            if (layout == 2) {
                cb = mj_up420(cbp, cpitch, (W + 1) / 2, (H + 1) / 2, x, y);
                cr = mj_up420(crp, cpitch, (W + 1) / 2, (H + 1) / 2, x, y);
            } else {
                cb = cbp[(size_t)y * cpitch + x];
                cr = crp[(size_t)y * cpitch + x];
            }
            px[i] = mj_rgb(yp[x], cb, cr);
        }
        unsigned char* o = out + (((size_t)f * H + y) * W + x0) * 3;
        if (W % 4 == 0) {
            uint32_t* o4 = (uint32_t*)o;
            o4[0] = px[0] | (px[1] << 24);
            o4[1] = (px[1] >> 8) | (px[2] << 16);
            o4[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
            for (int i = 0; i < n; ++i) {
                o[3 * i] = (unsigned char)px[i];
                o[3 * i + 1] = (unsigned char)(px[i] >> 8);
                o[3 * i + 2] = (unsigned char)(px[i] >> 16);
            }
        }
    }
}

extern "C" int vdx_mjpeg_color(const void* workspace, int F, int W, int H, int layout, void* out, vdx_stream_t stream) {
    MjLayout L;
    VDX_CHECK(workspace && out, "mjpeg_color: null pointer");
    VDX_CHECK(F > 0 && F <= 65535 && mj_layout(W, H, layout, &L) == 0, "mjpeg_color: F=%d W=%d H=%d layout=%d", F, W, H, layout);
    VDX_CHECK((long long)F * L.bpf < (1ll << 25), "mjpeg_color: the clip has too many blocks");
    // libjpeg switches to box replication when the chroma rows hold two samples or fewer: not implemented, refused
    VDX_CHECK(layout != 2 || W >= 5, "mjpeg_color: 4:2:0 frames %d wide are not supported (5 or more)", W);
    VDX_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 3) == 0, "mjpeg_color: misaligned pointer");
    const long long nb = (long long)F * L.bpf;
    const unsigned char* planes = (const unsigned char*)workspace + mj_round((size_t)nb * 64 * 2);
    const long long total = (long long)F * H * ((W + 3) / 4);
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(mjpeg_color_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks))), dim3(256), 0,
                       (hipStream_t)stream, planes, L, F, W, H, layout, (unsigned char*)out);
    return vdx_launch_status("vdx_mjpeg_color");
}
