// xattn.hip — K5: the cross-attention sub-block of diffusers' BasicTransformerBlock (Transformer2DModel, level 0 of the
// UNet; reached from fsdp_chunked_coherent.py:140) as ONE kernel:
//
//     t' = t + to_out( softmax( q K^T / 8 ) V ),   q = LayerNorm(t) . W_q^T,   K, V = the sample's text keys / values (77 x inner)
//
// Un-fused this is LayerNorm, a q GEMM, the flash kernel on 77 keys and an output GEMM + residual: four round trips of a
// [442 368][320] tensor per block.  Here a row is read once and written once.  The kernel is rowtile_common.h's machinery
// — the one tattn2.hip (K7, second design) is built on — with the roles changed:
//   * rows: 192 consecutive rows per tile (4 waves x 48), never straddling two batch items; centred / scaled in LDS,
//     LayerNorm's affine and the softmax scale folded into W_q on the host (packing.pack_k5);
//   * per head: five K-64 steps project q (24 MFMAs each), then ONE attention step: the head's text keys and values — 80
//     key slots, 2 x 10 KB in MFMA-fragment order, packed once per prompt (packing.pack_k5_kv) — arrive as three units of
//     the same weight ring; the scores S^T = K q^T (key on the registers, query on the lane), the softmax over the 80 slots
//     (slots >= kv_len masked) and O^T = V^T P^T run in registers; O^T is the B operand of the output projection as it
//     stands (tattn2's permuted W_o);
//   * the output projection, bias, residual, epilogue, the prefetch of the next tile's rows behind the projection and the
//     5-unit weight ring are rowtile_common.h's; the counted s_waitcnt scheme is tattn2's (see the comments there).
// Built for inner 320 (level 0: 5 cross-attentions per forward).
#include "rowtile_common.h"
#include "lab.h"

namespace {

struct K5P {
    const f16* t;        // [M][ldt] rows
    f16* out;            // [M][ldo]
    const char* wq;      // [head][5 units][8192 B]: q0 .. q4 (a unit: 64 weight rows x 64 k as 8 tiles: tile 4*kk + j)
    const char* wo;      // [cg A: head x 2 units][cg B: head x 2 units][cg C: head x 1 unit]
    const char* kv;      // [item][head][3 units]: K fragments [kt 5][j 4][lane][8 B], V fragments [kt 5][dt 4][lane][8 B], pad
    const float* bq;     // [inner]  c . W_q . beta
    const float* bo2;    // [inner]  b_o
    int ldt, ldo;
    int B, S;            // batch items, rows per item
    int tps;             // tiles per batch item = ceil(S / 192): a tile never straddles two batch items
    int ntiles;          // B * tps
    int kv_len;          // text tokens (<= 80): key slots kv_len .. 79 are masked
    float eps;
};

template <int INNER>
struct K5 : RowTile<INNER> {
    typedef RowTile<INNER> RT;
    using RT::XB, RT::UB, RT::NU, RT::NPS, RT::NCGF, RT::NCG, RT::ROWS, RT::nt_of, RT::opaque;
    using RT::lds, RT::lane, RT::n16, RT::q4, RT::wave, RT::wfrag, RT::xfrag;
    using typename RT::Frag;
    static constexpr int KS = INNER / 32;                 // MFMA k steps over the model width
    static constexpr int HEADS = INNER / 64;
    static constexpr int KM = KS / 2;                     // K-64 steps over the model width
    static constexpr int KVU = 3;                         // units of one head's keys + values
    static constexpr int KT = 5;                          // key tiles of 16 slots
    static constexpr int HSTEPS = KM + 1;                 // steps of one head: KM of q, one of attention
    static constexpr int P1S = HEADS * HSTEPS;
    static constexpr int NSTEP = P1S + NCG * HEADS;       // the output projection contracts head by head (K = 64)
    static constexpr int UPH = KM + KVU;                  // units of one head in the stream
    static_assert(KS % 2 == 0, "geometry");
    static_assert(KVU <= NU && 2 * KT * 4 * 512 <= KVU * UB, "a head's keys and values must fit its units and the ring");

    // ---- the static schedule of a tile (tattn2.hip): step s consumes units [ub(s), ub(s+1)) of the weight stream
    static constexpr int kind(int s) { return s < P1S ? ((s % HSTEPS) < KM ? 0 : 1) : 2; }        // 0 q, 1 attention, 2 out
    static constexpr int ub1(int s) {
        if (s <= P1S) return UPH * (s / HSTEPS) + (s % HSTEPS);                 // q steps: one unit each; the attention step: KVU
        const int v = s - P1S, c = v / HEADS, m = v % HEADS;
        return UPH * HEADS + (c < NCGF ? 2 * HEADS * c + 2 * m : 2 * HEADS * NCGF + (v - NCGF * HEADS));
    }
    static constexpr int NUNITS = ub1(NSTEP);
    static constexpr int ub(int s) { return s <= NSTEP ? ub1(s) : NUNITS + ub1(s - NSTEP); }
    static constexpr int hm(int s) { return ub(s + 1) + NU; }
    static_assert(NUNITS % NU == 0, "the ring position of a unit must not depend on the tile");
    static_assert(ub1(HSTEPS) == UPH && ub1(KM + 1) - ub1(KM) == KVU, "the attention step owns the head's KVU units");

    // ---- every vector-memory instruction a wave issues, in order (tattn2.hip): the step's s_waitcnt vmcnt(N) is exact
    // (the output projection and the row prefetch behind it: rowtile_common.h, groups of HEADS steps from step P1S)
    static constexpr int RS0 = P1S + HEADS;
    static constexpr int xp(int s) { return RT::op_xp(s, P1S, HEADS); }
    static constexpr int p0_mask_of(int s) { return RT::op_p0_mask(s, P1S, HEADS); }
    // q bias of the next head: loaded at the top of the head's attention step (its q accumulators are dead by then)
    static constexpr int n_bq(int s) { return kind(s) == 1 && s + 1 < P1S ? 4 : (s == NSTEP - 1 ? 4 : 0); }
    static constexpr int n_bias(int s) { return RT::op_bias(s, P1S, HEADS); }
    static constexpr int n_res(int s) { return RT::op_res(s, P1S, HEADS); }
    static constexpr int n_st(int s) { return RT::op_st(s, P1S, HEADS); }
    static constexpr int prev(int s) { return s == 0 ? NSTEP - 1 : s - 1; }
    static constexpr int younger(int s) { return xp(prev(s)) + n_st(prev(s)) + n_bq(s) + n_bias(s) + n_res(s); }
    static constexpr int inflight(int s) { return 2 * (hm(s - 1) - ub(s + 2)) + younger(s); }

    struct State {
        Frag fa, fb;
        f32x4 aq[3][4];                          // q^T: [d][row]
        f32x4 acc[3][8];                         // output projection: [col][row]
        f16x8 oh[HEADS][3][2];                   // the heads' outputs as B operands: [time slot][row tile][k step of the head]
        f32x4 bqv[4];
        f16x4 qh[3][4];                          // q of the current head as fp16 MFMA operands
        f16x4 kf[KT][4], vh[KT][4];              // the head's K and V fragments (read once, before the step's barrier frees their units)
        f16x4 pt[3][KT];                         // P^T of the current head: [query tile][key tile]
        f16x8 rv[3][4];                          // residual rows of the current column group
        f32x4 bv[8];                             // its output bias, the projection's initial accumulator
        const gf16* resp[3];
        gf16* outp[3];
    };

    const K5P& p;
    int rot, rotn;                               // head walking order of this / the next tile (tattn2.hip: a function of the tile's position in its item)
    int kvoff;                                   // LDS byte offset of this lane inside a fragment block: lane * 8
    int tb, tg, tbn, tgn;                        // this wave's (batch item, 48-row group inside it) in this tile / the next tile

    __device__ __forceinline__ K5(const K5P& p_, char* s) : RT(s), p(p_) {}

    // ---- weight stream
    template <int U>
    __device__ __forceinline__ const char* unit_src() const {
        constexpr int u = U % NUNITS;
        const bool nx = U >= NUNITS;                      // (the stream runs on into the next tile)
        const int r = nx ? rotn : rot;
        if constexpr (u < UPH * HEADS) {
            constexpr int hs = u / UPH, w = u % UPH;
            int h = hs + r;
            if (h >= HEADS) h -= HEADS;
            if constexpr (w < KM) return p.wq + (size_t)(h * KM + w) * UB;
            else {
                int item = nx ? tbn : tb;                 // (past the last tile: any valid item; the data is never used)
                if (item >= p.B) item = 0;
                return p.kv + ((size_t)(item * HEADS + h) * KVU + (w - KM)) * UB;
            }
        } else {
            constexpr int v = u - UPH * HEADS;
            if constexpr (v < 2 * HEADS * NCGF) {
                constexpr int cg = v / (2 * HEADS), rr = v % (2 * HEADS), hs = rr / 2, kk = rr % 2;
                int h = hs + r;
                if (h >= HEADS) h -= HEADS;
                return p.wo + (size_t)(cg * 2 * HEADS + h * 2 + kk) * UB;
            } else {
                constexpr int hs = v - 2 * HEADS * NCGF;
                int h = hs + r;
                if (h >= HEADS) h -= HEADS;
                return p.wo + (size_t)(2 * HEADS * NCGF + h) * UB;
            }
        }
    }
    template <int U0, int U1>
    __device__ __forceinline__ void issue_range() {
        RT::template issue_range<U0, U1>([this](auto u) { return unit_src<decltype(u)::value>(); });
    }

    // global row index of local row r (0..47) of row group g4 of batch item b and whether it exists
    __device__ __forceinline__ bool grow_of(int b, int g4, int r, long long& gr) const {
        const int pix = g4 * 48 + r;
        const bool ok = b < p.B && pix < p.S;
        gr = ok ? (long long)b * p.S + pix : 0ll;
        return ok;
    }

    // ---- the row image (rowtile_common.h)
    template <int PS>
    __device__ __forceinline__ void issue_rows(int b, int g4) {
        long long gr;
        const bool ok = grow_of(b, g4, 8 * PS + (lane >> 3), gr);
        RT::template issue_rows<PS>((const char*)(p.t + gr * p.ldt), ok);
    }
    // fragment block BLK (512 bytes: 64 lanes x 8) of the head whose first K|V unit is U0: byte BLK * 512 of the head's stream
    template <int U0, int BLK>
    __device__ __forceinline__ f16x4 kvfrag() const {
        constexpr int byte = BLK * 512, u = U0 + byte / UB, o = byte % UB;
        return *(const lf16x4*)(lds + kvoff + (XB + (u % NU) * UB + o));
    }

    // fragments of half KK (one MFMA k step) of step S (S may be NSTEP: step 0 of the next tile)
    template <int S_, int KK>
    __device__ __forceinline__ void read_half(Frag& f) const {
        constexpr int S = S_ % NSTEP;
        constexpr int kd = kind(S), u0 = ub(S);
        if constexpr (kd == 0) {
            constexpr int m = S % HSTEPS;
#pragma unroll
            for (int j = 0; j < 4; ++j) f.w[j] = wfrag(u0, 4 * KK + j);
#pragma unroll
            for (int i = 0; i < 3; ++i) f.x[i] = xfrag(i, 2 * m + KK);
        } else if constexpr (kd == 2) {
            RT::template read_out_half<(S - P1S) / HEADS, KK>(f, u0);
        }
    }

    // the MFMAs of half KK of step S (q steps and output steps; the attention step has its own body)
    template <int S, int KK, int NDS, int NVM>
    __device__ __forceinline__ void mma_half(State& st, const Frag& f) {
        constexpr int kd = kind(S);
        if constexpr (kd == 0) {
            constexpr bool Z = (S % HSTEPS) == 0 && KK == 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    st.aq[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.w[j], f.x[i], Z ? st.bqv[j] : st.aq[i][j], 0, 0, 0);
        } else if constexpr (kd == 2) {
            constexpr int v = S - P1S, c = v / HEADS, hs = v % HEADS;
            RT::template mma_out<c, hs == 0 && KK == 0>(st.acc, f, st.oh[hs][0][KK], st.oh[hs][1][KK], st.oh[hs][2][KK], st.bv);
        }
        if constexpr (kd != 1) RT::template pin_after_mfma<NVM, NDS>();
    }
    static constexpr int nds(int s_) {
        const int s = s_ % NSTEP;
        return kind(s) == 0 ? 7 : kind(s) == 1 ? 0 : nt_of((s - P1S) / HEADS);
    }

    // ---- attention of the head in time slot HS on the wave's 48 rows, all in registers.
    // First half of the attention step (before the step's barrier lets the ring overwrite the head's units): q as fp16
    // operands, the V fragments into registers, the scores against the K fragments in LDS, the softmax -> P^T as fp16.
    template <int S>
    __device__ __forceinline__ void attn_first(State& st) {
        constexpr int u0 = ub(S);
#ifdef K5_ABL_NOATT        /* lab build (timing only, wrong results): what the attention step's register work costs */
        for (int qt = 0; qt < 3; ++qt) for (int kk = 0; kk < 2; ++kk) for (int e = 0; e < 8; ++e) st.oh[S / HSTEPS][qt][kk][e] = (f16)st.aq[qt][2 * kk + (e >> 2)][e & 3];
        return;
#endif
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) st.qh[i][j][e] = (f16)st.aq[i][j][e];
        read_kv<u0>(st, std::make_integer_sequence<int, KT * 4>{});      // 40 ds_read_b64, all in flight together
        scores<0>(st);
        scores<1>(st);
        scores<2>(st);
    }
    template <int U0, int... B>
    __device__ __forceinline__ void read_kv(State& st, std::integer_sequence<int, B...>) {
        ((st.kf[B / 4][B % 4] = kvfrag<U0, B>()), ...);
        ((st.vh[B / 4][B % 4] = kvfrag<U0, KT * 4 + B>()), ...);
    }
    // scores of query tile QT: S^T = K q^T (query on the lane, the lane's keys of tile kt: 16*kt + 4*q4 + e)
    template <int QT>
    __device__ __forceinline__ void scores(State& st) {
        f32x4 sc[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            sc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) sc[kt] = __builtin_amdgcn_mfma_f32_16x16x16f16(st.kf[kt][j], st.qh[QT][j], sc[kt], 0, 0, 0);
        }
        const int kl = p.kv_len - 4 * q4;                 // key slot 16*kt + 4*q4 + e exists iff 16*kt + e < kl
        float mx = -1.0e30f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            if (16 * kt + 16 > p.kv_len) {                // (wave-uniform: only the tiles that hold padded slots pay for the mask)
#pragma unroll
                for (int e = 0; e < 4; ++e) sc[kt][e] = 16 * kt + e < kl ? sc[kt][e] : -1.0e30f;      // exp2 below gives exactly 0
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, sc[kt][e]);
        }
        mx = quad_max(mx);
        float rs = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sc[kt][e] = __builtin_amdgcn_exp2f(sc[kt][e] - mx);         // (the scale is in W_q)
                rs += sc[kt][e];
            }
        rs = quad_sum(rs);
        const float inv = 1.0f / rs;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int e = 0; e < 4; ++e) st.pt[QT][kt][e] = (f16)(sc[kt][e] * inv);
    }
    // second half: O^T[d][query] = V^T P^T: lane = query row, registers e = d 16*dt + 4*q4 + e; two d tiles side by side
    // are one B operand of the output projection (k index of W_o permuted to match: packing.pack_k5)
    template <int HS>
    __device__ __forceinline__ void attn_pv(State& st) {
#ifdef K5_ABL_NOATT
        return;
#endif
#pragma unroll
        for (int qt = 0; qt < 3; ++qt)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                f32x4 o0 = (f32x4){0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    o0 = __builtin_amdgcn_mfma_f32_16x16x16f16(st.vh[kt][2 * kk], st.pt[qt][kt], o0, 0, 0, 0);
                    o1 = __builtin_amdgcn_mfma_f32_16x16x16f16(st.vh[kt][2 * kk + 1], st.pt[qt][kt], o1, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    st.oh[HS][qt][kk][e] = (f16)o0[e];
                    st.oh[HS][qt][kk][4 + e] = (f16)o1[e];
                }
            }
    }

    template <int HS, bool NEXT_TILE = false>
    __device__ __forceinline__ void load_bq(State& st) {
        int h = HS + (NEXT_TILE ? rotn : rot);
        if (h >= HEADS) h -= HEADS;
        const int o = opaque(h * 64 + 4 * q4);
#pragma unroll
        for (int j = 0; j < 4; ++j) st.bqv[j] = *(const gf32x4*)((const __attribute__((address_space(1))) float*)p.bq + o + 16 * j);
    }
    template <int C>
    __device__ __forceinline__ void load_bias(State& st) { RT::template load_bias<C>(st.bv, p.bo2); }
    template <int C>
    __device__ __forceinline__ void load_residual(State& st) { RT::template load_residual<C>(st.rv, st.resp); }
    template <int C>
    __device__ __forceinline__ void epilogue(State& st) { RT::template epilogue<C>(st.acc, st.rv, st.outp); }

    // ---- one step of the tile.  At its top the fragments of its first half are in registers (st.fa).
    template <int S>
    __device__ __forceinline__ void step(State& st) {
        constexpr int kd = kind(S);
        if constexpr (n_bq(S) > 0) load_bq<(S == NSTEP - 1 ? 0 : S / HSTEPS + 1), S == NSTEP - 1>(st);
        if constexpr (n_bias(S) > 0) load_bias<(S + 1 - P1S) / HEADS>(st);
        if constexpr (n_res(S) > 0) load_residual<(S - P1S) / HEADS>(st);
        RT::template p0_passes<p0_mask_of(S)>(p.eps);
        if constexpr (kd == 1) {
            attn_first<S>(st);
        } else {
            read_half<S, 1>(st.fb);
            mma_half<S, 0, nds(S), 0>(st, st.fa);
        }
        // the units of step S+1 have landed for everyone, and nobody reads the units of step S any more
        __builtin_amdgcn_sched_barrier(0);
        wait_vm<inflight(S)>();
        __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt(0): my reads of step S's units are done
        asm volatile("" ::: "memory");
        wg_barrier();
        issue_range<hm(S - 1), hm(S)>();
        if constexpr (xp(S) > 0) {
            issue_rows<3 * (S - RS0)>(tbn, tgn);
            issue_rows<3 * (S - RS0) + 1>(tbn, tgn);
            issue_rows<3 * (S - RS0) + 2>(tbn, tgn);
        }
        read_half<S + 1, 0>(st.fa);
        if constexpr (kd == 1) {
            attn_pv<S / HSTEPS>(st);
        } else {
            mma_half<S, 1, nds(S + 1), 2 * (hm(S) - hm(S - 1)) + xp(S)>(st, st.fb);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (n_st(S) > 0) epilogue<(S - P1S) / HEADS>(st);
    }
    template <int... S>
    __device__ __forceinline__ void steps(State& st, std::integer_sequence<int, S...>) {
        (step<S>(st), ...);
    }
    template <int... PS>
    __device__ __forceinline__ void first_rows(std::integer_sequence<int, PS...>) {
        (issue_rows<PS>(tb, tg), ...);
        wait_vm<0>();
        RT::template p0_passes<(1 << NPS) - 1>(p.eps);
    }

    __device__ __forceinline__ void set_lane_constants() {
        RT::set_lane_constants();
        kvoff = lane * 8;
    }

    // tile -> (batch item, this wave's 48-row group inside it, head rotation); tiles are aligned to batch items
    __device__ __forceinline__ void set_tile(int tile, int& b, int& g4, int& r) const {
        b = tile / p.tps;
        const int tt = tile - b * p.tps;
        g4 = tt * 4 + wave;
        r = tt % HEADS;
    }

    __device__ __forceinline__ void run() {
        const int tid = threadIdx.x;
        lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        set_lane_constants();
        int tile = blockIdx.x;
        set_tile(tile, tb, tg, rot);
        rotn = rot;
        tbn = tb;
        tgn = tg;
        State st;
        issue_range<0, NU>();
        load_bq<0>(st);
        first_rows(std::make_integer_sequence<int, NPS>{});
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wg_barrier();
        read_half<0, 0>(st.fa);

        for (;;) {
            asm volatile("" : "+v"(lane));
            asm volatile("" : "+s"(wave));
            set_lane_constants();
            const int next = tile + gridDim.x;
            set_tile(next, tbn, tgn, rotn);      // (past the last tile: every row reads the zero page)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                long long gr;
                const bool ok = grow_of(tb, tg, 16 * i + n16, gr);
                gf16* dump = (gf16*)g_dump_page + lane * 8;
                const gf16* rp = (const gf16*)p.t + gr * p.ldt + 8 * q4;
                gf16* op = (gf16*)p.out + gr * p.ldo + 8 * q4;
                st.resp[i] = ok ? rp : dump;
                st.outp[i] = ok ? op : dump;
            }
            steps(st, std::make_integer_sequence<int, NSTEP>{});
            if (next >= p.ntiles) break;
            tile = next;
            tb = tbn;
            tg = tgn;
            rot = rotn;
        }
        wait_vm<0>();        // (the stream ran on into a tile that does not exist: let its copies land before the LDS is released)
    }
};

template <int INNER>
__global__ __launch_bounds__(256, 1) void xattn_kernel(const K5P p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    K5<INNER> k(p, smem);
    k.run();
}

}  // namespace

extern "C" int vdx_cross_attn_block_supported(int inner, int kv_len) {
    return inner == 320 && kv_len >= 1 && kv_len <= 16 * K5<320>::KT;
}
// bytes of the static blob (vdx/packing.py pack_k5): q units, output-projection units, fp32 q bias, fp32 output bias
extern "C" size_t vdx_cross_attn_block_pack_bytes(int inner) {
    if (inner != 320) return 0;
    typedef K5<320> T;
    return (size_t)(T::NUNITS - T::HEADS * T::KVU) * T::UB + 2 * 320 * sizeof(float);
}
// bytes of the per-prompt key / value blob of ONE batch item (vdx/packing.py pack_k5_kv)
extern "C" size_t vdx_cross_attn_block_kv_bytes(int inner) {
    if (inner != 320) return 0;
    return (size_t)K5<320>::HEADS * K5<320>::KVU * K5<320>::UB;
}

extern "C" int vdx_cross_attn_block_f16(const void* t, int ldt, const void* packed, const void* kv_packed, int kv_len, float eps,
                                        void* out, int ldo, int n_items, int rows_per_item, int inner, vdx_stream_t stream) {
    VDX_CHECK(t && packed && kv_packed && out, "cross_attn_block: null pointer");
    VDX_CHECK(n_items > 0 && rows_per_item > 0, "cross_attn_block: empty problem");
    VDX_CHECK(vdx_cross_attn_block_supported(inner, kv_len), "cross_attn_block: inner=%d kv_len=%d not supported (inner 320, 1..80 keys)", inner, kv_len);
    VDX_CHECK(ldt % 8 == 0 && ldo % 8 == 0 && ldt >= inner && ldo >= inner, "cross_attn_block: bad leading dims");
    VDX_CHECK((long long)n_items * rows_per_item < (1ll << 31), "cross_attn_block: too many rows");
    VDX_CHECK(((uintptr_t)t % 16 == 0) && ((uintptr_t)out % 16 == 0) && ((uintptr_t)packed % 16 == 0) && ((uintptr_t)kv_packed % 16 == 0),
              "cross_attn_block: pointers must be 16-byte aligned");
    VDX_CHECK(t != out, "cross_attn_block: out may not alias t (a tile's residual is read after other tiles were written)");
    typedef K5<320> T;
    K5P p;
    p.t = (const f16*)t; p.out = (f16*)out;
    p.wq = (const char*)packed;
    p.wo = p.wq + (size_t)T::KM * T::HEADS * T::UB;
    p.bq = (const float*)(p.wq + (size_t)(T::NUNITS - T::HEADS * T::KVU) * T::UB);
    p.bo2 = p.bq + 320;
    p.kv = (const char*)kv_packed;
    p.ldt = ldt; p.ldo = ldo; p.B = n_items; p.S = rows_per_item;
    p.tps = (rows_per_item + T::ROWS - 1) / T::ROWS;
    p.ntiles = n_items * p.tps;
    p.kv_len = kv_len;
    p.eps = eps;
    constexpr int lds = T::LDS_BYTES;
    static const hipError_t attr_rc = vdx_reserve_lds(lds, xattn_kernel<320>);
    if (attr_rc != hipSuccess) return vdx_fail("cross_attn_block: cannot reserve %d bytes of LDS", lds);
    const int grid = vdx_persistent_grid(p.ntiles);
    hipLaunchKernelGGL(xattn_kernel<320>, dim3(grid), dim3(256), lds, (hipStream_t)stream, p);
    return vdx_launch_status("vdx_cross_attn_block_f16");
}

// Lab variants of this translation unit are compiled in only under the switches that lab.h lists for it.
extern "C" int vdx_lab_xattn(void) { return VDX_LAB_XATTN; }
