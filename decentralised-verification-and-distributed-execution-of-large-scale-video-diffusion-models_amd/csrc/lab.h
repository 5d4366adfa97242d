// lab.h — the one list of lab switches, and what the stamped builds share.
//
// Lab variants of a translation unit (phase stamps, ablations: timing only, some give WRONG results) are compiled in only
// under the -D switches below.  A unit built with one of its switches reports its bit through vdx_lab_<unit>();
// vdx_build_flags() (common.hip) ORs the eight and vdx/_lib.py refuses to load a non-zero library as the product
// (VERDICT r4 item 7b).  Every macro that a unit's sources test with #if / #ifdef / #ifndef / defined() stands in that unit's
// list here and nowhere else (tests/test_host.py compares the two, both ways).  Bits as include/vdx.h documents them.
#pragma once

// gemm.hip
#if defined(VDX_STAMPS)              /* per-block phase clocks (make stamps, tools/gemm_stamps.py) */ \
    || (defined(VDX_ABL) && VDX_ABL) /* =n: the K loop without one of its parts, under VDX_STAMPS */  \
    || defined(VDX_GEMM_PLAIN_LOOP)  /* the K loop without the rolling fragment prefetch (tools/gemm_abl.sh) */
#define VDX_LAB_GEMM 1
#else
#define VDX_LAB_GEMM 0
#endif

// gemm_ws.hip
#if defined(VDX_STAMPS)    /* per-block cycle totals of wave 0 (tools/ws_stamps.py) */ \
    || defined(VDX_WS_NS3) /* a 3-deep ring where the product takes 4 */
#define VDX_LAB_GEMM_WS 2
#else
#define VDX_LAB_GEMM_WS 0
#endif

// tattn_fused.hip (K7, first design)
#if defined(VDX_STAMPS)       /* per-block phase cycle totals of one wave (tools/k7_stamps.py) */ \
    || defined(K7_ABL_NOP0)   /* rows from a register pattern instead of memory */             \
    || defined(K7_ABL_NOMFMA) /* one MFMA column per step instead of all */                    \
    || defined(K7_ABL_NOEPI) || defined(K7_ABL_NODMA) || defined(K7_ABL_NOATT) /* without the epilogue / weight DMA / attention */
#define VDX_LAB_TATTN_FUSED 4
#else
#define VDX_LAB_TATTN_FUSED 0
#endif

// tattn2.hip (K7, second design)
#if defined(K7B_STAMPS)                        /* cycle totals per (step kind, segment) of wave 0 (tools/k7b_stamps.py) */ \
    || defined(K7B_SS) || defined(K7B_SE)      /* =a, =b: K7B_STAMPS restricted to steps a..b (tools/k7b_stamps_range.py) */ \
    || defined(K7B_SHFL)                       /* quad reductions by ds_bpermute instead of the permlane swaps */          \
    || defined(K7B_ABL_NOROWS) || defined(K7B_ABL_NOEPI) || defined(K7B_ABL_NOATT) || defined(K7B_ABL_NOWDMA) /* without the row gather / epilogue / attention / weight DMA */
#define VDX_LAB_TATTN2 8
#else
#define VDX_LAB_TATTN2 0
#endif

// flash.hip (the switches are described at the top of that file and in profiles/r04_flash.md)
#if defined(FL_STAMPS)                                                                                              \
    || defined(FL_ABL_NOEXP) || defined(FL_ABL_MFMA16) || defined(FL_ABL_NOVREAD) || defined(FL_ABL_NOSUM)           \
    || defined(FL_ABL_NOMAX) || defined(FL_ABL_NOKREAD) || defined(FL_ABL_NODMA) || defined(FL_ABL_NOBAR)
#define VDX_LAB_FLASH 16
#else
#define VDX_LAB_FLASH 0
#endif

// ff_fused.hip (K8): what each part of the tile costs (tools/k8_abl.sh)
#if defined(K8_ABL_NOWDMA) || defined(K8_ABL_NOLDSX) || defined(K8_ABL_NOLDSW) || defined(K8_ABL_NOGEGLU) || defined(K8_ABL_NOBAR)
#define VDX_LAB_FF_FUSED 32
#else
#define VDX_LAB_FF_FUSED 0
#endif

// conv_fused.hip (K1, tools/k1_abl.sh)
#if defined(K1_ABL_NOPIN)     /* hipcc's own order of the reads and MFMAs */ \
    || defined(K1_ABL_NONORM) /* later slices are not normalised */
#define VDX_LAB_CONV_FUSED 64
#else
#define VDX_LAB_CONV_FUSED 0
#endif

// xattn.hip (K5)
#if defined(K5_ABL_NOATT) /* without the attention step's register work */
#define VDX_LAB_XATTN 128
#else
#define VDX_LAB_XATTN 0
#endif

// gemm.hip's ablation ladder: VDX_ABL only acts in a stamped build
#if defined(VDX_STAMPS) && defined(VDX_ABL)
#define VDX_ABL_IS(n) (VDX_ABL == (n))
#else
#define VDX_ABL_IS(n) 0
#endif

// ---- stamps: cycle sums that a kernel leaves in a device buffer, and the host reads back --------------------------------
#if defined(VDX_STAMPS) || defined(K7B_STAMPS) || defined(FL_STAMPS)
#include <hip/hip_runtime.h>
// buf[n] (u64) and its exported reader.  SIG is the reader's name and argument list, the first argument being `void* dst`;
// BYTES is how much of the buffer, from its start, that call copies to dst.
#define VDX_STAMP_BUFFER_AS(buf, n, SIG, BYTES)                                                                      \
    static __device__ unsigned long long buf[n];                                                                     \
    extern "C" int SIG {                                                                                             \
        const size_t bytes_ = (size_t)(BYTES);                                                                       \
        return dst && bytes_ <= sizeof(buf) && hipMemcpyFromSymbol(dst, HIP_SYMBOL(buf), bytes_) == hipSuccess ? 0 : -1; \
    }
// the usual reader: reader(void* dst) copies the whole buffer
#define VDX_STAMP_BUFFER(buf, reader, n) VDX_STAMP_BUFFER_AS(buf, n, reader(void* dst), sizeof(buf))
// the accumulate step: sum += now - last; last = now
#define VDX_STAMP_ACC(sum, last) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); (sum) += now_ - (last); (last) = now_; }
#endif
