// Block geometry shared by the Motion-JPEG reader (mjpeg.hip) and writer (mjpeg_enc.hip).
#pragma once
#include "vdx_common.h"

// Block geometry of one frame.  layout 0: one component; 1: three components 1x1 (4:4:4); 2: 2x2, 1x1, 1x1 (4:2:0).
// Component c holds bw[c] x bh[c] blocks (the padded MCU extent) from block boff[c] of the frame; bpf blocks per frame.
struct MjLayout {
    int ncomp, mcux, mcuy, nmcu, bpf;
    int h[3], v[3], bw[3], bh[3], boff[3];
};

static int mj_layout(int W, int H, int layout, MjLayout* L) {
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || layout < 0 || layout > 2) return -1;
    const int hmax = layout == 2 ? 2 : 1;
    L->ncomp = layout == 0 ? 1 : 3;
    L->mcux = (W + 8 * hmax - 1) / (8 * hmax);
    L->mcuy = (H + 8 * hmax - 1) / (8 * hmax);
    L->nmcu = L->mcux * L->mcuy;
    int off = 0;
    for (int c = 0; c < 3; ++c) {
        const int s = (c == 0 && c < L->ncomp) ? hmax : (c < L->ncomp ? 1 : 0);
        L->h[c] = L->v[c] = s;
        L->bw[c] = L->mcux * s;
        L->bh[c] = L->mcuy * s;
        L->boff[c] = off;
        off += L->bw[c] * L->bh[c];
    }
    L->bpf = off;
    return 0;
}

static inline size_t mj_round(size_t n) { return (n + 255) & ~(size_t)255; }

// natural (row-major) index of the k-th coefficient in zigzag (file) order
static __device__ const unsigned char mj_natural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
