// mjpeg_enc.hip — baseline JPEG encode of a whole clip on the device: the write side of the job's `cv2.VideoWriter`
// (fsdp_chunked_coherent.py:250-253; vdx/compat/cv2_shim.py VideoWriter.write is the host path this restates).  From uint8
// frames to the bytes libjpeg writes for them as Pillow drives it (quality-scaled Annex K tables, 4:2:0 or grey, baseline,
// the standard Huffman tables), byte for byte (tests/test_video_enc_gpu.py; tests/mjpeg_enc_ref.py is the definition in
// numpy).  Integers only.  The only atomics are integer ORs into words zeroed on the stream, so the bytes are the same on
// every run and for any number of frames per call.
//
//   stage 1  vdx_mjpeg_enc_color    RGB -> Y, Cb, Cr (16-bit fixed point), h2v2 downsample, edge replication -> component planes
//   stage 2  vdx_mjpeg_enc_fdct     - 128, slow-integer forward DCT, quantise -> int16 coefficients in the READER's layout
//   stage 3  vdx_mjpeg_enc_entropy  bits per block | scan per restart interval | emit | stuffed bytes per slot | scan per frame
//   stage 4  vdx_mjpeg_enc_pack     header + stuffed segments + RSTn + EOI of every frame, back to back
//
// What bounds every access of stages 3 and 4: a block costs at most 1658 bits (below), so restart interval s of a frame, which
// starts at block b0 in scan order, owns the MJE_SLOT_BYTES * (its blocks) bytes of `raw` from slot b0 and cannot outgrow
// them; the packed stream is sized by the host from the lengths stage 3 counted, and stage 4 checks every store against
// that size all the same.
#include "vdx_common.h"
#include "mjpeg_common.h"

// One luma block: DC code <= 9 bits + 11 value bits; each of the 63 AC coefficients <= 16 + 10 bits (a ZRL is 11 bits for 16
// coefficients: cheaper).  20 + 63 * 26 = 1658 bits; the up to 7 padding bits of a segment fit the last block's slot too:
// ceil(n * 1658 / 8) <= 208 n.  A chroma block stays below that: its DC code is up to 11 bits, but run 0 / size 10 has a
// 12-bit code, and a 16-bit code needs a run, which halves the coefficients coded: 22 + 63 * 22 = 1408 bits at most
// (tests/mjpeg_enc_ref.py `coef_sets` reaches both).  Sizes are clamped to 11 / 10 in the coder, so the bound holds for ANY
// int16 coefficients; from 8-bit samples nothing is ever clamped: |DC| <= 64 * 128 * 8 / 8 = 1024 (a difference of at most
// 2047: size 11) and |AC| <= 1020 (the largest basis sum, 8, times 127.5) before the division by q >= 1.
#define MJE_SLOT_BYTES 208
#define MJE_SLOT_WORDS 52
#define MJE_TABLE_WORDS 272      // per table id: 16 DC words by size, 256 AC words by run << 4 | size; length << 16 | code

struct MjeWs {
    size_t coef, planes, bits, segbits, slots, raw, total;
};
// coefficients and planes lie where vdx_mjpeg_workspace puts them, so the reader's stages run on this workspace as it is
static void mje_ws(int F, const MjLayout& L, MjeWs* w) {
    const size_t nb = (size_t)F * L.bpf;
    w->coef = 0;                                                  // int16 [F][bpf][64]
    w->planes = mj_round(nb * 128);                               // uint8 [F][bpf * 64]
    w->bits = w->planes + mj_round(nb * 64);                      // uint32 [F][bpf], scan order: bits, then bit offset in the segment
    w->segbits = w->bits + mj_round(nb * 4);                      // uint32 [F][nmcu]: bits of every restart interval
    w->slots = w->segbits + mj_round((size_t)F * L.nmcu * 4);     // uint32 [F][bpf]: stuffed bytes of a slot, then their offset
    w->raw = w->slots + mj_round(nb * 4);                         // uint32 [F][bpf][52]: the unstuffed bit stream, MSB first
    w->total = w->raw + mj_round(nb * MJE_SLOT_BYTES);
}
static int mje_args(int F, int W, int H, int layout, MjLayout* L) {
    if (F <= 0 || F > 65535 || layout == 1 || mj_layout(W, H, layout, L) != 0) return -1;
    if ((long long)F * L->bpf >= (1ll << 25)) return -1;
    if ((long long)L->bpf * (MJE_SLOT_BYTES * 8) >= (1ll << 31)) return -1;      // bit offsets inside a frame are uint32
    return 0;
}
#define MJE_ARGS(name)                                                                                                  \
    MjLayout L;                                                                                                         \
    VDX_CHECK(mje_args(F, W, H, layout, &L) == 0, name ": F=%d W=%d H=%d layout=%d (0 or 2) is outside what the encoder takes", F, W, \
              H, layout);                                                                                               \
    MjeWs ws;                                                                                                           \
    mje_ws(F, L, &ws)

extern "C" size_t vdx_mjpeg_enc_workspace(int F, int W, int H, int layout) {
    MjLayout L;
    if (mje_args(F, W, H, layout, &L) != 0) return 0;
    MjeWs ws;
    mje_ws(F, L, &ws);
    return ws.total;
}

extern "C" int vdx_mjpeg_enc_offsets(int F, int W, int H, int layout, size_t* offsets) {
    VDX_CHECK(offsets, "mjpeg_enc_offsets: null pointer");
    MJE_ARGS("mjpeg_enc_offsets");
    const size_t o[6] = {ws.coef, ws.planes, ws.bits, ws.segbits, ws.slots, ws.raw};
    for (int i = 0; i < 6; ++i) offsets[i] = o[i];
    return 0;
}

// ---- stage 1: colour conversion + downsampling ----------------------------------------------------------------------------
// libjpeg's tables: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; Cb, Cr with FIX(0.16874) ... and the offset
// (128 << 16) + 32767.  The h2v2 downsample adds 1, 2, 1, 2, ... along the output columns to the 2x2 sum before >> 2.
// Edges: the last column is replicated at full resolution; a row pair the bottom edge cuts is completed with the last row;
// chroma rows below ceil(H / 2) repeat the last DOWNSAMPLED row, luma rows below H the last row.
__device__ __forceinline__ int mje_y(const unsigned char* p) { return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16; }
__device__ __forceinline__ int mje_cb(const unsigned char* p) {
    return (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int mje_cr(const unsigned char* p) {
    return (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16;
}
// one thread per chroma sample: the 2x2 luma samples above it and one sample of Cb and of Cr
__global__ __launch_bounds__(256) void mje_color420_kernel(const unsigned char* frames, MjLayout L, int F, int W, int H,
                                                           unsigned char* planes) {
    const int CPW = L.bw[1] * 8, CPH = L.bh[1] * 8, PW = L.bw[0] * 8, CH = (H + 1) >> 1;
    const long long total = (long long)F * CPH * CPW;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % CPW);
        const long long t = idx / CPW;
        const int i = (int)(t % CPH), f = (int)(t / CPH);
        const unsigned char* fr = frames + (size_t)f * H * W * 3;
        unsigned char* fp = planes + (size_t)f * L.bpf * 64;
        const size_t c0 = (size_t)min(2 * j, W - 1) * 3, c1 = (size_t)min(2 * j + 1, W - 1) * 3;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const unsigned char* row = fr + (size_t)min(2 * i + dy, H - 1) * W * 3;
            *(unsigned short*)(fp + (size_t)(2 * i + dy) * PW + 2 * j) = (unsigned short)(mje_y(row + c0) | (mje_y(row + c1) << 8));
        }
        const int ii = min(i, CH - 1);
        const unsigned char* r0 = fr + (size_t)min(2 * ii, H - 1) * W * 3;
        const unsigned char* r1 = fr + (size_t)min(2 * ii + 1, H - 1) * W * 3;
        const int bias = 1 + (j & 1);
        fp[(size_t)L.boff[1] * 64 + (size_t)i * CPW + j] =
            (unsigned char)((mje_cb(r0 + c0) + mje_cb(r0 + c1) + mje_cb(r1 + c0) + mje_cb(r1 + c1) + bias) >> 2);
        fp[(size_t)L.boff[2] * 64 + (size_t)i * CPW + j] =
            (unsigned char)((mje_cr(r0 + c0) + mje_cr(r0 + c1) + mje_cr(r1 + c0) + mje_cr(r1 + c1) + bias) >> 2);
    }
}
// grey: one thread per 4 samples of the padded plane
__global__ __launch_bounds__(256) void mje_grey_kernel(const unsigned char* frames, MjLayout L, int F, int W, int H,
                                                       unsigned char* planes) {
    const int PW = L.bw[0] * 8, PH = L.bh[0] * 8, PW4 = PW / 4;
    const long long total = (long long)F * PH * PW4;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x0 = (int)(idx % PW4) * 4;
        const long long t = idx / PW4;
        const int y = (int)(t % PH), f = (int)(t / PH);
        const unsigned char* row = frames + ((size_t)f * H + min(y, H - 1)) * W;
        uint32_t px = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) px |= (uint32_t)row[min(x0 + k, W - 1)] << (8 * k);
        *(uint32_t*)(planes + (size_t)f * L.bpf * 64 + (size_t)y * PW + x0) = px;
    }
}

extern "C" int vdx_mjpeg_enc_color(const void* frames, int F, int W, int H, int layout, void* workspace, vdx_stream_t stream) {
    VDX_CHECK(frames && workspace, "mjpeg_enc_color: null pointer");
    MJE_ARGS("mjpeg_enc_color");
    VDX_CHECK(((uintptr_t)workspace & 15) == 0, "mjpeg_enc_color: misaligned workspace");
    unsigned char* planes = (unsigned char*)workspace + ws.planes;
    const long long total = layout == 2 ? (long long)F * L.bh[1] * 8 * L.bw[1] * 8 : (long long)F * L.bh[0] * 8 * L.bw[0] * 2;
    long long blocks = (total + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks);
    if (layout == 2)
        hipLaunchKernelGGL(mje_color420_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)frames, L,
                           F, W, H, planes);
    else
        hipLaunchKernelGGL(mje_grey_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)frames, L, F,
                           W, H, planes);
    return vdx_launch_status("vdx_mjpeg_enc_color");
}

// ---- stage 2: forward DCT + quantisation -------------------------------------------------------------------------------------
// The "islow" forward transform (Loeffler, Ligtenberg, Moschytz 1989, as in the Independent JPEG Group's encoder), the inverse
// of mjpeg.hip's mj_idct8: 13-bit constants; pass 1 over rows keeps 2 extra bits, pass 2 over columns removes them and leaves
// the result scaled by 8, which the quantiser's divisor 8 q takes out.  int32 cannot overflow from 8-bit samples.
template <bool FIRST>
__device__ __forceinline__ void mje_fdct8(const int* d, int* o) {
    constexpr int SH = FIRST ? 13 - 2 : 13 + 2, RND = 1 << (SH - 1);
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        o[0] = (tmp10 + tmp11) * 4;
        o[4] = (tmp10 - tmp11) * 4;
    } else {
        o[0] = (tmp10 + tmp11 + 2) >> 2;
        o[4] = (tmp10 - tmp11 + 2) >> 2;
    }
    int z1 = (tmp12 + tmp13) * 4433;
    o[2] = (z1 + tmp13 * 6270 + RND) >> SH;
    o[6] = (z1 + tmp12 * -15137 + RND) >> SH;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    tmp4 *= 2446;
    tmp5 *= 16819;
    tmp6 *= 25172;
    tmp7 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[7] = (tmp4 + z1 + z3 + RND) >> SH;
    o[5] = (tmp5 + z2 + z4 + RND) >> SH;
    o[3] = (tmp6 + z2 + z3 + RND) >> SH;
    o[1] = (tmp7 + z1 + z4 + RND) >> SH;
}

// 256 threads = 32 blocks of 8x8; lane (block L >> 3, j = L & 7) transforms row j, then column j, then stores row j of the
// quantised block (16 bytes).  A luma block of a 4:2:0 frame wholly outside ceil(extent / 8) blocks is one of libjpeg's dummy
// blocks: AC zero, DC that of the last real block before it in its MCU's order (0,0) (0,1) (1,0) (1,1); its lanes transform
// that block's samples and keep the DC alone.
#define MJE_WS_ROW 9
#define MJE_WS_BLK 76
#define MJE_ST_STRIDE 72
__global__ __launch_bounds__(256) void mje_fdct_kernel(const unsigned char* planes, const unsigned short* quant, MjLayout L, int W,
                                                       int H, int layout, long long nblocks, short* coef) {
    __shared__ int ws[32 * MJE_WS_BLK];
    __shared__ __attribute__((aligned(16))) short st[32 * MJE_ST_STRIDE];
    const int lb = threadIdx.x >> 3, j = threadIdx.x & 7;
    const long long g = (long long)blockIdx.x * 32 + lb;
    const bool live = g < nblocks;
    int c = 0;
    bool dummy = false;
    int d[8], o[8];
    if (live) {
        const int f = (int)(g / L.bpf), bi = (int)(g % L.bpf);
        c = L.ncomp == 3 ? (bi >= L.boff[1]) + (bi >= L.boff[2]) : 0;
        const int rel = bi - L.boff[c], by = rel / L.bw[c], bx = rel - by * L.bw[c];
        int sy = by, sx = bx;
        if (layout == 2 && c == 0) {
            const int rbh = (H + 7) >> 3, rbw = (W + 7) >> 3;                // the real blocks; bh, bw are even and at most one more
            if (by >= rbh) {
                sy = by - 1;
                sx = (bx | 1) < rbw ? (bx | 1) : (bx | 1) - 1;
            } else if (bx >= rbw) {
                sx = bx - 1;
            }
            dummy = sy != by || sx != bx;
        }
        const uint2 px = *(const uint2*)(planes + ((size_t)f * L.bpf + L.boff[c]) * 64 + (size_t)(sy * 8 + j) * (L.bw[c] * 8) + sx * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int)(((k < 4 ? px.x : px.y) >> ((k & 3) * 8)) & 255u) - 128;
        mje_fdct8<true>(d, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[lb * MJE_WS_BLK + j * MJE_WS_ROW + k] = o[k];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = ws[lb * MJE_WS_BLK + r * MJE_WS_ROW + j];
        mje_fdct8<false>(d, o);
        const unsigned short* q = quant + (c ? 64 : 0) + j;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            // sign(v) * ((|v| + (8q >> 1)) / 8q): an exact integer quotient
            const unsigned dv = 8u * q[r * 8];
            const unsigned t = ((unsigned)abs(o[r]) + (dv >> 1)) / dv;
            int v = o[r] < 0 ? -(int)t : (int)t;
            if (dummy && (r | j)) v = 0;
            st[lb * MJE_ST_STRIDE + r * 8 + j] = (short)v;
        }
    }
    __syncthreads();
    if (live) *(u32x4*)(coef + (size_t)g * 64 + j * 8) = *(const u32x4*)(st + lb * MJE_ST_STRIDE + j * 8);
}

extern "C" int vdx_mjpeg_enc_fdct(const void* quant_u16, int F, int W, int H, int layout, void* workspace, vdx_stream_t stream) {
    VDX_CHECK(quant_u16 && workspace, "mjpeg_enc_fdct: null pointer");
    MJE_ARGS("mjpeg_enc_fdct");
    VDX_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)quant_u16 & 1) == 0, "mjpeg_enc_fdct: misaligned pointer");
    const long long nb = (long long)F * L.bpf;
    hipLaunchKernelGGL(mje_fdct_kernel, dim3((unsigned)((nb + 31) / 32)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)workspace + ws.planes, (const unsigned short*)quant_u16, L, W, H, layout, nb,
                       (short*)((char*)workspace + ws.coef));
    return vdx_launch_status("vdx_mjpeg_enc_fdct");
}

// ---- stage 3: entropy coding -------------------------------------------------------------------------------------------------
// Scan order: MCU after MCU, inside an MCU component after component, a 2x2 luma group row-major.  Block i of that order is
// block k = i % bpm of MCU m = i / bpm; a restart interval (segment) is `step` MCUs, the whole frame without DRI.
struct MjeScan {
    int bpm, step, nseg, luma;           // blocks per MCU, MCUs per segment, segments per frame, luma blocks per MCU
};
static MjeScan mje_scan(const MjLayout& L, int restart_interval) {
    MjeScan s;
    s.luma = L.h[0] * L.v[0];
    s.bpm = s.luma + (L.ncomp == 3 ? 2 : 0);
    s.step = restart_interval > 0 && restart_interval < L.nmcu ? restart_interval : L.nmcu;
    s.nseg = (L.nmcu + s.step - 1) / s.step;
    return s;
}
// the block's index in the coefficient workspace, and its component
__device__ __forceinline__ int mje_widx(const MjLayout& L, const MjeScan& S, int m, int k, int* comp) {
    const int my = m / L.mcux, mx = m - my * L.mcux;
    const int c = k < S.luma ? 0 : k - S.luma + 1;
    const int by = c ? 0 : k / L.h[0], bx = c ? 0 : k - by * L.h[0];
    *comp = c;
    return L.boff[c] + (my * L.v[c] + by) * L.bw[c] + mx * L.h[c] + bx;
}

// The codes of one block into a sink (the bit counter or the bit writer: one definition of the stream for both).
template <class Sink>
__device__ __forceinline__ void mje_code_block(const short* blk, int pred, const uint32_t* tab, Sink& s) {
    const int diff = (int)blk[0] - pred;
    int size = min(32 - __clz(abs(diff)), 11);
    uint32_t e = tab[size];
    s.put(e & 0xFFFFu, (int)(e >> 16));
    if (size) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1u), size);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[mj_natural[k]];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            e = tab[16 + 0xF0];                                             // ZRL
            s.put(e & 0xFFFFu, (int)(e >> 16));
            run -= 16;
        }
        size = min(32 - __clz(abs(v)), 10);
        e = tab[16 + ((run << 4) | size)];
        s.put(e & 0xFFFFu, (int)(e >> 16));
        s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u), size);
        run = 0;
    }
    if (run > 0) {
        e = tab[16];                                                        // EOB
        s.put(e & 0xFFFFu, (int)(e >> 16));
    }
}
struct MjeCount {
    uint32_t n;
    __device__ __forceinline__ void put(uint32_t, int len) { n += (uint32_t)len; }
};
// Bits go MSB first into 32-bit words.  Neighbouring blocks share a word, so every store is an atomic OR into memory zeroed on
// the stream before the launch: no result depends on the order of the stores.
struct MjeEmit {
    uint32_t* w;
    unsigned long long acc;
    int n;                                                                  // < 32 between puts
    __device__ __forceinline__ void put(uint32_t code, int len) {           // len <= 16
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            atomicOr(w++, (uint32_t)(acc >> (n - 32)));
            n -= 32;
            acc &= (1ull << n) - 1ull;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(w, (uint32_t)(acc << (32 - n)));
    }
};

// What a thread needs to code block i of frame f: the coefficients, the DC prediction (the previous block of the component
// in the same segment, else 0) and the component's tables.
__device__ __forceinline__ const short* mje_block_of(const short* fcoef, const MjLayout& L, const MjeScan& S, int i, int* pred,
                                                     int* table) {
    const int m = i / S.bpm, k = i - m * S.bpm;
    int c, pc;
    const short* blk = fcoef + (size_t)mje_widx(L, S, m, k, &c) * 64;
    *table = c ? 1 : 0;
    if (c == 0 && k > 0) *pred = fcoef[(size_t)mje_widx(L, S, m, k - 1, &pc) * 64];
    else if (m % S.step == 0) *pred = 0;
    else *pred = fcoef[(size_t)mje_widx(L, S, m - 1, c ? k : S.luma - 1, &pc) * 64];
    return blk;
}

__global__ __launch_bounds__(256) void mje_count_kernel(const short* coef, const uint32_t* tables, MjLayout L, MjeScan S,
                                                        uint32_t* bits) {
    __shared__ uint32_t tab[2 * MJE_TABLE_WORDS];
    for (int t = threadIdx.x; t < 2 * MJE_TABLE_WORDS; t += blockDim.x) tab[t] = tables[t];
    __syncthreads();
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.bpf) return;
    int pred, table;
    const short* blk = mje_block_of(coef + (size_t)f * L.bpf * 64, L, S, i, &pred, &table);
    MjeCount s = {0};
    mje_code_block(blk, pred, tab + table * MJE_TABLE_WORDS, s);
    bits[(size_t)f * L.bpf + i] = s.n;
}

// exclusive scan of one value per thread over the 256 threads of a block; *total is the sum
__device__ __forceinline__ uint32_t mje_exscan256(uint32_t v, uint32_t* sh, uint32_t* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t t = tid >= off ? sh[tid - off] : 0u;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const uint32_t incl = sh[tid];
    *total = sh[255];
    __syncthreads();
    return incl - v;
}
// values[f][lo .. hi) -> their exclusive prefix sums in place, sums[...] = the total (+ `extra`); one block per range:
// blockIdx.x is the segment (nseg > 0) or the range is the whole frame
__global__ __launch_bounds__(256) void mje_scan_kernel(uint32_t* values, int bpf, int span, uint32_t* sums, int sums_pitch,
                                                       uint32_t extra) {
    __shared__ uint32_t sh[256];
    const int f = blockIdx.y, lo = blockIdx.x * span, hi = min(lo + span, bpf);
    uint32_t* v = values + (size_t)f * bpf;
    uint32_t carry = 0;
    for (int base = lo; base < hi; base += 256) {
        const int i = base + threadIdx.x;
        uint32_t total;
        const uint32_t ex = mje_exscan256(i < hi ? v[i] : 0u, sh, &total);
        if (i < hi) v[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) sums[(size_t)f * sums_pitch + blockIdx.x] = carry + extra;
}

__global__ __launch_bounds__(256) void mje_emit_kernel(const short* coef, const uint32_t* tables, MjLayout L, MjeScan S,
                                                       const uint32_t* bits, uint32_t* raw) {
    __shared__ uint32_t tab[2 * MJE_TABLE_WORDS];
    for (int t = threadIdx.x; t < 2 * MJE_TABLE_WORDS; t += blockDim.x) tab[t] = tables[t];
    __syncthreads();
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.bpf) return;
    int pred, table;
    const short* blk = mje_block_of(coef + (size_t)f * L.bpf * 64, L, S, i, &pred, &table);
    const int span = S.step * S.bpm, lo = i / span * span, hi = min(lo + span, L.bpf);
    const uint32_t at = bits[(size_t)f * L.bpf + i];                        // < 1658 * span: inside the segment's slots
    MjeEmit s;
    s.w = raw + ((size_t)f * L.bpf + lo) * MJE_SLOT_WORDS + (at >> 5);
    s.acc = 0;
    s.n = (int)(at & 31u);
    const MjeEmit start = s;
    mje_code_block(blk, pred, tab + table * MJE_TABLE_WORDS, s);
    if (i == hi - 1) {                                                      // the segment ends here: 1-bits up to the byte
        const int total = (int)((s.w - start.w) * 32 + s.n);               // bits from the start of the first word
        const int pad = -total & 7;
        if (pad) s.put((1u << pad) - 1u, pad);
    }
    s.finish();
}

// byte b of a segment whose words start at `w`
__device__ __forceinline__ uint32_t mje_raw_byte(const uint32_t* w, uint32_t b) { return (w[b >> 2] >> (24 - 8 * (b & 3))) & 255u; }

// slot j of a segment holds its bytes [208 j, 208 (j + 1)) as far as the segment reaches; -> what they take in the file: every
// FF is followed by 00, and the first slot of every segment but the first is preceded by the RSTn marker
__global__ __launch_bounds__(256) void mje_stuff_count_kernel(const uint32_t* raw, const uint32_t* segbits, MjLayout L, MjeScan S,
                                                              uint32_t* slots) {
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.bpf) return;
    const int span = S.step * S.bpm, s = i / span, lo = s * span, j = i - lo;
    const uint32_t nbytes = (segbits[(size_t)f * L.nmcu + s] + 7u) >> 3;
    const uint32_t b0 = (uint32_t)j * MJE_SLOT_BYTES, b1 = min(b0 + MJE_SLOT_BYTES, nbytes);
    const uint32_t* w = raw + ((size_t)f * L.bpf + lo) * MJE_SLOT_WORDS;
    uint32_t n = j == 0 && s > 0 ? 2u : 0u;
    for (uint32_t b = b0; b < b1; ++b) n += mje_raw_byte(w, b) == 0xFFu ? 2u : 1u;
    slots[(size_t)f * L.bpf + i] = n;
}

extern "C" int vdx_mjpeg_enc_entropy(const void* tables, int F, int W, int H, int layout, int restart_interval, int header_bytes,
                                     void* workspace, int32_t* lengths, vdx_stream_t stream) {
    VDX_CHECK(tables && workspace && lengths, "mjpeg_enc_entropy: null pointer");
    MJE_ARGS("mjpeg_enc_entropy");
    VDX_CHECK(restart_interval >= 0 && restart_interval <= 65535 && header_bytes >= 0 && header_bytes < (1 << 16),
              "mjpeg_enc_entropy: restart_interval=%d header_bytes=%d", restart_interval, header_bytes);
    VDX_CHECK(((uintptr_t)workspace & 15) == 0 && (((uintptr_t)tables | (uintptr_t)lengths) & 3) == 0, "mjpeg_enc_entropy: misaligned pointer");
    const MjeScan S = mje_scan(L, restart_interval);
    char* base = (char*)workspace;
    const short* coef = (const short*)(base + ws.coef);
    uint32_t *bits = (uint32_t*)(base + ws.bits), *segbits = (uint32_t*)(base + ws.segbits), *slots = (uint32_t*)(base + ws.slots),
             *raw = (uint32_t*)(base + ws.raw);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 per_block((L.bpf + 255) / 256, F);
    const hipError_t e = hipMemsetAsync(raw, 0, (size_t)F * L.bpf * MJE_SLOT_BYTES, st);
    VDX_CHECK(e == hipSuccess, "mjpeg_enc_entropy: memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(mje_count_kernel, per_block, dim3(256), 0, st, coef, (const uint32_t*)tables, L, S, bits);
    hipLaunchKernelGGL(mje_scan_kernel, dim3(S.nseg, F), dim3(256), 0, st, bits, L.bpf, S.step * S.bpm, segbits, L.nmcu, 0u);
    hipLaunchKernelGGL(mje_emit_kernel, per_block, dim3(256), 0, st, coef, (const uint32_t*)tables, L, S, (const uint32_t*)bits, raw);
    hipLaunchKernelGGL(mje_stuff_count_kernel, per_block, dim3(256), 0, st, (const uint32_t*)raw, (const uint32_t*)segbits, L, S, slots);
    // a frame: header, the stuffed segments with their markers, EOI
    hipLaunchKernelGGL(mje_scan_kernel, dim3(1, F), dim3(256), 0, st, slots, L.bpf, L.bpf, (uint32_t*)lengths, 1,
                       (uint32_t)header_bytes + 2u);
    return vdx_launch_status("vdx_mjpeg_enc_entropy");
}

// ---- stage 4: the file bytes ------------------------------------------------------------------------------------------------
// Every slot's bytes go to the offset the scan gave them; a thread owns its output range, so plain byte stores do.
__device__ __forceinline__ void mje_store(unsigned char* out, size_t out_bytes, size_t at, uint32_t v) {
    if (at < out_bytes) out[at] = (unsigned char)v;
}
__global__ __launch_bounds__(256) void mje_pack_kernel(const uint32_t* raw, const uint32_t* segbits, const uint32_t* slots,
                                                       const int32_t* lengths, const unsigned char* header, int header_bytes,
                                                       MjLayout L, MjeScan S, unsigned char* out, size_t out_bytes) {
    __shared__ unsigned long long frame_at;
    const int f = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (threadIdx.x == 0) {
        unsigned long long at = 0;
        for (int g = 0; g < f; ++g) at += (unsigned long long)max(lengths[g], 0);
        frame_at = at;
    }
    __syncthreads();
    const size_t base = (size_t)frame_at;
    if (blockIdx.x == 0)
        for (int t = threadIdx.x; t < header_bytes; t += blockDim.x) mje_store(out, out_bytes, base + t, header[t]);
    if (i >= L.bpf) return;
    const int span = S.step * S.bpm, s = i / span, lo = s * span, j = i - lo;
    const uint32_t nbytes = (segbits[(size_t)f * L.nmcu + s] + 7u) >> 3;
    const uint32_t b0 = (uint32_t)j * MJE_SLOT_BYTES, b1 = min(b0 + MJE_SLOT_BYTES, nbytes);
    const uint32_t* w = raw + ((size_t)f * L.bpf + lo) * MJE_SLOT_WORDS;
    size_t at = base + header_bytes + slots[(size_t)f * L.bpf + i];
    if (j == 0 && s > 0) {
        mje_store(out, out_bytes, at++, 0xFFu);
        mje_store(out, out_bytes, at++, 0xD0u + ((uint32_t)(s - 1) & 7u));
    }
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t v = mje_raw_byte(w, b);
        mje_store(out, out_bytes, at++, v);
        if (v == 0xFFu) mje_store(out, out_bytes, at++, 0u);
    }
    if (i == L.bpf - 1) {
        mje_store(out, out_bytes, at++, 0xFFu);
        mje_store(out, out_bytes, at++, 0xD9u);
    }
}

extern "C" int vdx_mjpeg_enc_pack(const void* header, int header_bytes, int F, int W, int H, int layout, int restart_interval,
                                  const void* workspace, const int32_t* lengths, void* out, size_t out_bytes, vdx_stream_t stream) {
    VDX_CHECK(header && workspace && lengths && out, "mjpeg_enc_pack: null pointer");
    MJE_ARGS("mjpeg_enc_pack");
    VDX_CHECK(restart_interval >= 0 && restart_interval <= 65535 && header_bytes >= 0 && header_bytes < (1 << 16),
              "mjpeg_enc_pack: restart_interval=%d header_bytes=%d", restart_interval, header_bytes);
    VDX_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)lengths & 3) == 0, "mjpeg_enc_pack: misaligned pointer");
    const MjeScan S = mje_scan(L, restart_interval);
    const char* base = (const char*)workspace;
    hipLaunchKernelGGL(mje_pack_kernel, dim3((L.bpf + 255) / 256, F), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t*)(base + ws.raw), (const uint32_t*)(base + ws.segbits), (const uint32_t*)(base + ws.slots), lengths,
                       (const unsigned char*)header, header_bytes, L, S, (unsigned char*)out, out_bytes);
    return vdx_launch_status("vdx_mjpeg_enc_pack");
}
