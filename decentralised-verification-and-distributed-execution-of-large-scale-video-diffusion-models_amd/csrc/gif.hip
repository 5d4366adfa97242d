// gif.hip — an animated GIF89a of a whole clip on the device (no reference counterpart; vdx/gif.py writes the headers and
// cuts the palette on the host, tests/gif_ref.py is the definition in numpy).  From uint8 RGB frames to the data sub-blocks of
// every frame's image.  Integers only.  The only atomics are integer adds (the histogram) and integer ORs into words zeroed
// on the stream (the strips' bits), so the bytes are the same on every run and for any number of frames per call.
//
//   stage 1  vdx_gif_hist_u8   pixels per 5-5-5 bin over the whole clip (one global colour table)
//   stage 2  (host)            median cut of the histogram -> at most 256 colours (vdx/gif.py `median_cut`)
//   stage 3  vdx_gif_lut       nearest palette entry of every bin centre
//   stage 4  vdx_gif_index_u8  ordered dither, bin, LUT -> one palette index per pixel
//   stage 5  vdx_gif_lzw       LZW per strip of rows into the strip's own slot | scan per frame | bits to their offset
//   stage 6  vdx_gif_pack      every frame's byte stream as data sub-blocks, back to back
//
// What bounds every access of stages 5 and 6: a strip of n pixels emits at most n data codes (a code consumes at least one
// pixel), one CLEAR per 3838 of them (the table takes 4096 - 258 entries between resets), its opening CLEAR and its closing
// CLEAR / EOI, each at most 12 bits: 12 (n + n / 3838 + 3) bits, the slot (gif_geo).  A frame's stream is at most its strips'
// slots; the packed bytes are sized by the host from the lengths stage 5 counted.  Every store is checked against those sizes
// all the same, every table index is masked, and every loop has a bound that no pixel, table entry or count can move.
#include "vdx_common.h"

#define GIF_BINS 32768
#define GIF_CLEAR 256u
#define GIF_EOI 257u
#define GIF_FIRST 258u                // the first free code of an empty table
#define GIF_CODES 4096u
#define GIF_TABLE_SLOTS 8192          // open-addressed, a power of two: at most 3838 of them are ever taken
#define GIF_EMPTY 0xFFFFFFFFu         // no entry is this: an entry's code is above its prefix, so prefix 4095 never occurs
#define GIF_CHUNK 256                 // pixels a wave stages in LDS at a time
#define GIF_LANES 64                  // a workgroup of the LZW kernel is exactly one wave

static inline size_t gif_round(size_t n) { return (n + 255) & ~(size_t)255; }

// ---- stage 1: histogram ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gif_bin(uint32_t r, uint32_t g, uint32_t b) { return ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3); }

// a thread walks 8 consecutive pixels and adds a run of equal bins at once (a flat clip is then 1/8 of the atomics)
__global__ __launch_bounds__(256) void gif_hist_kernel(const unsigned char* frames, size_t frame_pitch, int row_pitch, int H, int W,
                                                       unsigned long long total, uint32_t* hist) {
    const unsigned long long groups = (total + 7) / 8;
    for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups;
         g += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long p0 = g * 8;
        int x = (int)(p0 % (unsigned)W);
        const unsigned long long t = p0 / (unsigned)W;
        int y = (int)(t % (unsigned)H);
        unsigned long long f = t / (unsigned)H;
        const int cnt = (int)min(8ull, total - p0);
        uint32_t run = 0, len = 0;
        for (int k = 0; k < cnt; ++k) {
            const unsigned char* p = frames + f * frame_pitch + (size_t)y * row_pitch + (size_t)x * 3;
            const uint32_t bin = gif_bin(p[0], p[1], p[2]);
            if (len && bin != run) {
                atomicAdd(hist + run, len);
                len = 0;
            }
            run = bin;
            ++len;
            if (++x == W) {
                x = 0;
                if (++y == H) {
                    y = 0;
                    ++f;
                }
            }
        }
        if (len) atomicAdd(hist + run, len);
    }
}

extern "C" int vdx_gif_hist_u8(const void* frames, size_t frame_pitch, int row_pitch, int T, int H, int W, uint32_t* hist,
                               vdx_stream_t stream) {
    VDX_CHECK(frames && hist, "gif_hist: null pointer");
    VDX_CHECK(T >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "gif_hist: T=%d H=%d W=%d", T, H, W);
    const unsigned long long total = (unsigned long long)T * H * W;
    VDX_CHECK(total < (1ull << 32), "gif_hist: %llu pixels do not fit the uint32 counts (2^32 or more)", total);
    VDX_CHECK(row_pitch >= 3 * W && frame_pitch >= (size_t)row_pitch * H, "gif_hist: pitches %zu / %d overlap", frame_pitch, row_pitch);
    VDX_CHECK(((uintptr_t)hist & 3) == 0, "gif_hist: misaligned histogram");
    const hipError_t e = hipMemsetAsync(hist, 0, GIF_BINS * sizeof(uint32_t), (hipStream_t)stream);
    VDX_CHECK(e == hipSuccess, "gif_hist: memset failed: %s", hipGetErrorString(e));
    unsigned long long blocks = ((total + 7) / 8 + 255) / 256;
    blocks = blocks > 8192 ? 8192 : blocks;
    hipLaunchKernelGGL(gif_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)frames,
                       frame_pitch, row_pitch, H, W, total, hist);
    return vdx_launch_status("vdx_gif_hist_u8");
}

// ---- stage 3: nearest palette entry of every bin centre ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gif_lut_kernel(const unsigned char* palette, int n, unsigned char* lut) {
    __shared__ int pal[256 * 3];
    for (int i = threadIdx.x; i < n * 3; i += blockDim.x) pal[i] = palette[i];
    __syncthreads();
    const int bin = blockIdx.x * blockDim.x + threadIdx.x;
    if (bin >= GIF_BINS) return;
    const int r = ((bin >> 10) << 3) | 4, g = (((bin >> 5) & 31) << 3) | 4, b = ((bin & 31) << 3) | 4;
    int best = 0, bd = 0x7FFFFFFF;
    for (int i = 0; i < n; ++i) {
        const int dr = r - pal[3 * i], dg = g - pal[3 * i + 1], db = b - pal[3 * i + 2];
        const int d = dr * dr + dg * dg + db * db;
        if (d < bd) {                                                       // strict: a tie stays with the lowest index
            bd = d;
            best = i;
        }
    }
    lut[bin] = (unsigned char)best;
}

extern "C" int vdx_gif_lut(const void* palette, int n, void* lut, vdx_stream_t stream) {
    VDX_CHECK(palette && lut, "gif_lut: null pointer");
    VDX_CHECK(n >= 1 && n <= 256, "gif_lut: a palette of %d entries (1..256)", n);
    hipLaunchKernelGGL(gif_lut_kernel, dim3(GIF_BINS / 256), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)palette, n,
                       (unsigned char*)lut);
    return vdx_launch_status("vdx_gif_lut");
}

// ---- stage 4: dither, bin, LUT -------------------------------------------------------------------------------------------------
// the standard 8x8 Bayer matrix, 0..63
static __device__ const unsigned char gif_bayer8[64] = {0,  32, 8,  40, 2,  34, 10, 42, 48, 16, 56, 24, 50, 18, 58, 26, 12, 44, 4,  36, 14, 46,
                                                        6,  38, 60, 28, 52, 20, 62, 30, 54, 22, 3,  35, 11, 43, 1,  33, 9,  41, 51, 19, 59, 27,
                                                        49, 17, 57, 25, 15, 47, 7,  39, 13, 45, 5,  37, 63, 31, 55, 23, 61, 29, 53, 21};

__global__ __launch_bounds__(256) void gif_index_kernel(const unsigned char* frames, size_t frame_pitch, int row_pitch, int H, int W,
                                                        unsigned long long total, const unsigned char* lut, int dither, unsigned char* out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % (unsigned)W);
        const unsigned long long t = i / (unsigned)W;
        const int y = (int)(t % (unsigned)H);
        const unsigned long long f = t / (unsigned)H;
        const unsigned char* p = frames + f * frame_pitch + (size_t)y * row_pitch + (size_t)x * 3;
        const int d = dither ? (((int)gif_bayer8[(y & 7) * 8 + (x & 7)] * 8 + 4) >> 6) - 4 : 0;       // -4 .. 3: half a bin
        const uint32_t r = (uint32_t)min(max((int)p[0] + d, 0), 255), g = (uint32_t)min(max((int)p[1] + d, 0), 255),
                       b = (uint32_t)min(max((int)p[2] + d, 0), 255);
        out[i] = lut[gif_bin(r, g, b) & (GIF_BINS - 1)];
    }
}

extern "C" int vdx_gif_index_u8(const void* frames, size_t frame_pitch, int row_pitch, int T, int H, int W, const void* lut, int dither,
                                void* out, vdx_stream_t stream) {
    VDX_CHECK(frames && lut && out, "gif_index: null pointer");
    VDX_CHECK(T >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535, "gif_index: T=%d H=%d W=%d", T, H, W);
    VDX_CHECK(dither == 0 || dither == 1, "gif_index: dither=%d (0: none, 1: bayer)", dither);
    const unsigned long long total = (unsigned long long)T * H * W;
    VDX_CHECK(total < (1ull << 32), "gif_index: %llu pixels (2^32 or more)", total);
    VDX_CHECK(row_pitch >= 3 * W && frame_pitch >= (size_t)row_pitch * H, "gif_index: pitches %zu / %d overlap", frame_pitch, row_pitch);
    unsigned long long blocks = (total + 255) / 256;
    blocks = blocks > 16384 ? 16384 : blocks;
    hipLaunchKernelGGL(gif_index_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)frames,
                       frame_pitch, row_pitch, H, W, total, (const unsigned char*)lut, dither, (unsigned char*)out);
    return vdx_launch_status("vdx_gif_index_u8");
}

// ---- stage 5: LZW ----------------------------------------------------------------------------------------------------------------
struct GifGeo {
    int rows, nstrips;                   // rows of a strip (the last may be shorter), strips of a frame
    unsigned slot_words;                 // 32-bit words of a strip's slot
    size_t frame_words;                  // words of a frame's stream: its strips' slots
    size_t sbits, soff, fbits, slots, stream, foff, total;
};
static int gif_geo(int T, int H, int W, int strip_rows, GifGeo* g) {
    if (T < 1 || T > 65535 || H < 1 || H > 65535 || W < 1 || W > 65535 || strip_rows < 1) return -1;
    if ((unsigned long long)T * H * W >= (1ull << 32)) return -1;
    g->rows = strip_rows < H ? strip_rows : H;
    g->nstrips = (H + g->rows - 1) / g->rows;
    const unsigned long long n = (unsigned long long)g->rows * W;
    const unsigned long long words = (12ull * (n + n / 3838 + 3) + 31) / 32;
    const unsigned long long fw = words * g->nstrips;
    if (fw >= (1ull << 27)) return -1;                                      // bit offsets inside a frame are uint32
    g->slot_words = (unsigned)words;
    g->frame_words = (size_t)fw;
    const size_t ns = (size_t)T * g->nstrips;
    g->sbits = 0;                                                           // uint32 [T][nstrips]: bits of every strip
    g->soff = gif_round(ns * 4);                                            // uint32 [T][nstrips]: their bit offset in the frame
    g->fbits = g->soff + gif_round(ns * 4);                                 // uint32 [T]: bits of every frame
    g->slots = g->fbits + gif_round((size_t)T * 4);                         // uint32 [T][nstrips][slot_words], LSB first
    g->stream = g->slots + gif_round(ns * g->slot_words * 4);               // uint32 [T][frame_words], LSB first
    g->foff = g->stream + gif_round((size_t)T * g->frame_words * 4);       // uint64 [T]: byte offset of every frame's sub-blocks
    g->total = g->foff + gif_round((size_t)T * 8);
    return 0;
}
#define GIF_ARGS(name)                                                                                                           \
    GifGeo G;                                                                                                                    \
    VDX_CHECK(gif_geo(T, H, W, strip_rows, &G) == 0, name ": T=%d H=%d W=%d strip_rows=%d is outside what the encoder takes", T, \
              H, W, strip_rows)

extern "C" size_t vdx_gif_lzw_workspace(int T, int H, int W, int strip_rows) {
    GifGeo G;
    return gif_geo(T, H, W, strip_rows, &G) == 0 ? G.total : 0;
}

extern "C" int vdx_gif_lzw_offsets(int T, int H, int W, int strip_rows, size_t* offsets) {
    VDX_CHECK(offsets, "gif_lzw_offsets: null pointer");
    GIF_ARGS("gif_lzw_offsets");
    const size_t o[8] = {G.sbits, G.soff, G.fbits, G.slots, G.stream, G.foff, (size_t)G.nstrips, (size_t)G.slot_words};
    for (int i = 0; i < 8; ++i) offsets[i] = o[i];
    return 0;
}

// Codes go LSB first into 32-bit words of the strip's own slot: plain stores of lane 0, each checked against the slot.
struct GifBits {
    uint32_t* out;
    unsigned cap, w;
    unsigned long long acc;
    int n;                                                                  // < 32 between puts
    bool store;
    __device__ __forceinline__ void put(uint32_t code, int width) {         // width <= 12
        acc |= (unsigned long long)code << n;
        n += width;
        if (n >= 32) {
            if (store && w < cap) out[w] = (uint32_t)acc;
            ++w;
            acc >>= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ uint32_t finish() {
        if (n > 0 && store && w < cap) out[w] = (uint32_t)acc;
        return w * 32u + (uint32_t)n;
    }
};

// One strip per workgroup of one wave.  LZW is a chain: every step needs the code the step before found, so the 64 lanes walk
// the strip together, each holding the same state; the control flow is uniform, the lanes share the staging of the pixels and
// the clearing of the table, and lane 0 stores.  The dictionary is an open-addressed table in LDS, 8192 words of
// (prefix << 8 | byte) << 12 | code; with the 256 staged pixels a workgroup holds 33 024 bytes of LDS, so FOUR strips share a
// compute unit's 160 KiB (five would need 165 120 bytes).
static_assert(GIF_LANES == 64, "the LZW kernel's lanes keep one state in lockstep: a workgroup must be one gfx950 wave (wave64)");
__global__ __launch_bounds__(GIF_LANES) void gif_lzw_kernel(const unsigned char* idx, int H, int W, int rows, unsigned slot_words,
                                                     uint32_t* slots, uint32_t* sbits) {
    __shared__ uint32_t tab[GIF_TABLE_SLOTS];
    __shared__ unsigned char px[GIF_CHUNK];
    const int s = blockIdx.x, f = blockIdx.y, nstrips = gridDim.x, lane = threadIdx.x;
    const int r0 = s * rows, n = min(rows, H - r0) * W;                     // >= 1 pixel
    const unsigned char* src = idx + ((size_t)f * H + r0) * W;
    for (int i = lane; i < GIF_TABLE_SLOTS; i += GIF_LANES) tab[i] = GIF_EMPTY;
    GifBits b = {slots + ((size_t)f * nstrips + s) * slot_words, slot_words, 0u, 0ull, 0, lane == 0};
    uint32_t width = 9, nxt = GIF_FIRST, p = 0;
    __syncthreads();
    if (s == 0) b.put(GIF_CLEAR, 9);
    for (int base = 0; base < n; base += GIF_CHUNK) {
        const int m = min(GIF_CHUNK, n - base);
        __syncthreads();
        for (int k = lane; k < m; k += GIF_LANES) px[k] = src[base + k];
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const uint32_t c = px[k];
            if (base + k == 0) {
                p = c;
                continue;
            }
            const uint32_t key = (p << 8) | c;                              // 20 bits
            const uint32_t h = (key * 0x9E3779B1u) >> 19;                   // 13 bits
            uint32_t found = GIF_EMPTY, at = GIF_EMPTY;
            for (int j = 0; j < GIF_TABLE_SLOTS; ++j) {                     // bounded by the slots, whatever the table holds
                const uint32_t i = (h + (uint32_t)j) & (GIF_TABLE_SLOTS - 1);
                const uint32_t e = tab[i];
                if (e == GIF_EMPTY) {
                    at = i;
                    break;
                }
                if ((e >> 12) == key) {
                    found = e & (GIF_CODES - 1);
                    break;
                }
            }
            if (found != GIF_EMPTY) {
                p = found;
                continue;
            }
            b.put(p, (int)width);
            if (nxt < GIF_CODES) {
                // lane 0 stores, every lane probes the table at the next pixel: the barrier orders the two (the branch is
                // uniform; with one wave per workgroup it costs next to nothing)
                if (lane == 0 && at != GIF_EMPTY) tab[at] = (key << 12) | nxt;
                __syncthreads();
                ++nxt;
                if (nxt > (1u << width) && width < 12) ++width;
            } else {                                                        // the table is full: CLEAR, and start again
                b.put(GIF_CLEAR, (int)width);
                __syncthreads();
                for (int i = lane; i < GIF_TABLE_SLOTS; i += GIF_LANES) tab[i] = GIF_EMPTY;
                __syncthreads();
                nxt = GIF_FIRST;
                width = 9;
            }
            p = c;
        }
    }
    b.put(p, (int)width);
    if (nxt < GIF_CODES) {                                                  // the decoder adds an entry after this code too
        ++nxt;
        if (nxt > (1u << width) && width < 12) ++width;
    }
    b.put(s == nstrips - 1 ? GIF_EOI : GIF_CLEAR, (int)width);
    const uint32_t bits = b.finish();
    if (lane == 0) sbits[(size_t)f * nstrips + s] = bits;
}

// exclusive scan of one value per thread over the 256 threads of a block; *total is the sum
__device__ __forceinline__ uint32_t gif_exscan256(uint32_t v, uint32_t* sh, uint32_t* total) {
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
// one block per frame: the strips' bit offsets, the frame's bits, and what its sub-blocks take in the file.  A strip's bits
// are clamped to its slot, so the sum stays below 2^32 whatever `sbits` holds.
__global__ __launch_bounds__(256) void gif_scan_kernel(const uint32_t* sbits, int nstrips, unsigned slot_words, uint32_t* soff,
                                                       uint32_t* fbits, int32_t* lengths) {
    __shared__ uint32_t sh[256];
    const int f = blockIdx.x;
    uint32_t carry = 0;
    for (int base = 0; base < nstrips; base += 256) {
        const int i = base + threadIdx.x;
        uint32_t total;
        const uint32_t v = i < nstrips ? min(sbits[(size_t)f * nstrips + i], slot_words * 32u) : 0u;
        const uint32_t ex = gif_exscan256(v, sh, &total);
        if (i < nstrips) soff[(size_t)f * nstrips + i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        fbits[f] = carry;
        const uint32_t L = (carry + 7u) >> 3;
        lengths[f] = (int32_t)(L + (L + 254u) / 255u + 1u);
    }
}

// one wave: the byte offset of every frame's sub-blocks in the packed output, the exclusive sums of `lengths` in 64 bits.  Lane l
// owns frames [l * per, (l + 1) * per); a negative length counts as 0.
__global__ __launch_bounds__(64) void gif_frame_offsets_kernel(const int32_t* lengths, int T, unsigned long long* foff) {
    __shared__ unsigned long long part[64];
    const int lane = threadIdx.x, per = (T + 63) / 64, lo = min(lane * per, T), hi = min(lo + per, T);
    unsigned long long sum = 0;
    for (int f = lo; f < hi; ++f) sum += (unsigned long long)max(lengths[f], 0);
    part[lane] = sum;
    __syncthreads();
    unsigned long long at = 0;
    for (int l = 0; l < lane; ++l) at += part[l];
    for (int f = lo; f < hi; ++f) {
        foff[f] = at;
        at += (unsigned long long)max(lengths[f], 0);
    }
}

// word w of strip s to its bit offset in the frame's stream.  Neighbouring strips share a word, so every store is an atomic
// OR into memory zeroed on the stream before the launch: no result depends on the order of the stores.
__global__ __launch_bounds__(256) void gif_merge_kernel(const uint32_t* slots, const uint32_t* sbits, const uint32_t* soff, int nstrips,
                                                        unsigned slot_words, size_t frame_words, uint32_t* stream) {
    const unsigned w = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y, f = blockIdx.z;
    const size_t si = (size_t)f * nstrips + s;
    const uint32_t bits = min(sbits[si], slot_words * 32u);
    if (w >= slot_words || w * 32u >= bits) return;
    uint32_t v = slots[si * slot_words + w];
    if (bits - w * 32u < 32u) v &= (1u << (bits - w * 32u)) - 1u;
    const uint32_t at = soff[si] + w * 32u, sh = at & 31u;
    const size_t o = at >> 5;
    uint32_t* dst = stream + (size_t)f * frame_words;
    if (o < frame_words) atomicOr(dst + o, v << sh);
    if (sh && (v >> (32u - sh)) && o + 1 < frame_words) atomicOr(dst + o + 1, v >> (32u - sh));
}

extern "C" int vdx_gif_lzw(const void* idx, int T, int H, int W, int strip_rows, void* workspace, int32_t* lengths,
                           vdx_stream_t stream) {
    VDX_CHECK(idx && workspace && lengths, "gif_lzw: null pointer");
    GIF_ARGS("gif_lzw");
    VDX_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)lengths & 3) == 0, "gif_lzw: misaligned pointer");
    char* base = (char*)workspace;
    uint32_t *sbits = (uint32_t*)(base + G.sbits), *soff = (uint32_t*)(base + G.soff), *fbits = (uint32_t*)(base + G.fbits),
             *slots = (uint32_t*)(base + G.slots), *out = (uint32_t*)(base + G.stream);
    unsigned long long* foff = (unsigned long long*)(base + G.foff);
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(out, 0, (size_t)T * G.frame_words * 4, st);
    VDX_CHECK(e == hipSuccess, "gif_lzw: memset failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(gif_lzw_kernel, dim3(G.nstrips, T), dim3(GIF_LANES), 0, st, (const unsigned char*)idx, H, W, G.rows, G.slot_words, slots,
                       sbits);
    hipLaunchKernelGGL(gif_scan_kernel, dim3(T), dim3(256), 0, st, (const uint32_t*)sbits, G.nstrips, G.slot_words, soff, fbits, lengths);
    hipLaunchKernelGGL(gif_frame_offsets_kernel, dim3(1), dim3(64), 0, st, (const int32_t*)lengths, T, foff);
    hipLaunchKernelGGL(gif_merge_kernel, dim3((G.slot_words + 255) / 256, G.nstrips, T), dim3(256), 0, st, (const uint32_t*)slots,
                       (const uint32_t*)sbits, (const uint32_t*)soff, G.nstrips, G.slot_words, G.frame_words, out);
    return vdx_launch_status("vdx_gif_lzw");
}

// ---- stage 6: data sub-blocks ------------------------------------------------------------------------------------------------
// Byte b of a frame's L stream bytes lies behind b / 255 + 1 length bytes; a thread owns its output bytes, so plain stores do.
__device__ __forceinline__ void gif_store(unsigned char* out, size_t out_bytes, size_t at, uint32_t v) {
    if (at < out_bytes) out[at] = (unsigned char)v;
}
__global__ __launch_bounds__(256) void gif_pack_kernel(const uint32_t* stream, const uint32_t* fbits, const unsigned long long* foff,
                                                       size_t frame_words, unsigned char* out, size_t out_bytes) {
    const int f = blockIdx.y;
    const size_t base = (size_t)foff[f];
    const size_t L = min(((size_t)fbits[f] + 7) >> 3, frame_words * 4);
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L) return;
    const uint32_t v = (stream[(size_t)f * frame_words + (b >> 2)] >> (8 * (b & 3))) & 255u;
    const size_t k = b / 255;
    gif_store(out, out_bytes, base + b + k + 1, v);
    if (b == k * 255) gif_store(out, out_bytes, base + k * 256, (uint32_t)min((size_t)255, L - b));
    if (b == L - 1) gif_store(out, out_bytes, base + L + (L + 254) / 255, 0u);
}

extern "C" int vdx_gif_pack(const void* workspace, int T, int H, int W, int strip_rows, void* out, size_t out_bytes,
                            vdx_stream_t stream) {
    VDX_CHECK(workspace && out, "gif_pack: null pointer");
    GIF_ARGS("gif_pack");
    VDX_CHECK(((uintptr_t)workspace & 15) == 0, "gif_pack: misaligned workspace");
    const char* base = (const char*)workspace;
    const size_t blocks = (G.frame_words * 4 + 255) / 256;                  // < 2^21
    hipLaunchKernelGGL(gif_pack_kernel, dim3((unsigned)blocks, T), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)(base + G.stream),
                       (const uint32_t*)(base + G.fbits), (const unsigned long long*)(base + G.foff), G.frame_words, (unsigned char*)out,
                       out_bytes);
    return vdx_launch_status("vdx_gif_pack");
}
