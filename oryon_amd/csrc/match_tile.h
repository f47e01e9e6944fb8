// The exact matcher's two all-pairs tile walks as templates over what is done with a finished tile: how the query rows stream past a
// workgroup's 128 anchor columns and through the fp32 MFMA.  They are match_f32_kernel's and match_f32_regb_kernel's loops (match.hip)
// statement for statement, so the distances have K1's bits; the scan with exclusion discs (match_disc.h: K1r, match_second.hip, and K1n,
// match_next.hip) is built on them.  K1 and K1m (match_mutual.hip) still carry their own text of the loops: instantiated from here,
// each was 0.3 - 0.9 % slower at C_pad 32 (measured).
// The formulation, the geometry, the LDS image and the LDS-DMA are explained here, once, for all three.
// What a kernel does with a FINISHED tile of dot products - its fold - is the caller's:
//
//     struct Fold {
//         void prefetch(int qt);      // the loads of query tile qt have just been issued: fetch what the fold needs of that tile (registers)
//         void publish();             // ... and hand it to the workgroup (LDS) in front of the barrier that publishes the tile itself
//         void tile(acc, int qt);     // all k of query tile qt are in acc: fold it and leave acc zero
//     };
//
// A fold that needs nothing but the accumulators leaves prefetch / publish empty.  The walks hold barriers: every thread of the
// workgroup calls them with the same span.
//
// Formulation:  S = Q^ * A^T  (rows = query descriptors, columns = anchor descriptors), both operands already gathered + normalised into
// k-contiguous [N, C] rows by K0.  One workgroup owns a 128-anchor column panel and streams the query rows past it.  In the C/D layout
// of v_mfma_f32_32x32x2_f32 a lane owns ONE column (= one anchor) and 16 rows (= 16 queries), so a running reduction over queries is
// lane-local: no cross-lane traffic until the very end (lane l <-> l+32; in the staged walk also the two waves that share columns).
// The f32-input MFMA is an exact k-ordered fmaf chain, and both walks feed it k in the natural order.
#pragma once
#include "common.h"
#include "match_common.h"

namespace oryon {

constexpr int MT = ORYON_MATCH_TILE;  // 128 queries x 128 anchors per workgroup step
constexpr int BK = 32;                // k-tile
constexpr int LD = BK + 1;            // padded LDS row: ds_read_b32 of a 32-row column is conflict-free
constexpr int MATCH_THREADS = 256;
constexpr int TILE_FLOATS = MT * LD;
constexpr int ROW_NONE = 0x7fffffff;  // the index of a running (distance, index) that has no row yet: lex_min lets any row replace it

// query tiles [begin, end) of split `split` of S over nq rows in tiles of `rows`
struct TileSpan {
    int begin, end;
};
__device__ __forceinline__ TileSpan split_span(int nq, int rows, int S, int split)
{
    const int nqt = (nq + rows - 1) / rows;
    const int qt_per = (nqt + S - 1) / S;
    const int qt_begin = split * qt_per;
    return {qt_begin, (qt_begin + qt_per < nqt) ? qt_begin + qt_per : nqt};
}

// launch grids of a scan with T anchor panels per pair and S query splits; blocks are dealt to the 8 XCDs round-robin (blockIdx & 7).
// Anchor-stationary walk: (pair, split) units are dealt to the XCDs and all T anchor panels of a unit sit on ONE XCD, so a unit's query
// stream is fetched once per XCD and shared through that XCD's L2; several splits per pair keep the tail of the launch short.
inline int regb_groups(int B, int T, int S) { return ((B * S + 7) / 8) * 8 * T; }
// staged walk: XCD x gets the pairs {x, x+8, ...}, which keeps every panel and split of a pair on one L2
inline int staged_groups(int B, int T, int S) { return ((B + 7) / 8) * 8 * T * S; }

// the per-split (distance, index) rows [B, S, cap_a] that a split scan leaves for its merge, carved from base; -> bytes (0 when S == 1)
struct SplitWs {
    float *ws_dist;
    int32_t *ws_idx;
};
inline size_t carve_split(void *base, SplitWs &w, int B, int cap_a, int S, size_t start = 0)      // start: what the caller carved in front
{
    Carver carve(base, start);
    const size_t split_rows = S > 1 ? (size_t)B * S * cap_a : 0;
    carve(w.ws_dist, split_rows);
    carve(w.ws_idx, split_rows);
    return carve.end;
}

// ------------------------------------------------------------------------------------------------ wide descriptors (LDS-staged)
// Operands that do not fit the register file (e.g. C = 512): both are staged through LDS in k-tiles of 32, 128 query rows x 128 anchor
// rows per step.
// smem: 4 * TILE_FLOATS floats, [buf][Q|A][128][33].  ap: the panel's first anchor row, qp: the pair's first query row.
// Wave grid 2 (query halves, wm) x 2 (anchor halves, wn): acc[mi][ni] is the block of query rows wm*64 + mi*32.. and anchor columns
// wn*64 + ni*32..
template <class Fold>
__device__ __forceinline__ void match_staged_walk(float *smem, const float *ap, const float *qp, int Cp,
                                                  TileSpan span, Fold &fold)
{
    const int qt_begin = span.begin, qt_end = span.end;
    const int KT = Cp / BK;
    const int nit = (qt_end > qt_begin) ? (qt_end - qt_begin) * KT : 0;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;  // wave grid: 2 (query halves) x 2 (anchor halves)
    const int l31 = lane & 31, hi = lane >> 5;

    float4 rq[4], ra[4];
    auto gload = [&](int it) {
        const int qt = qt_begin + it / KT, kt = it % KT;
        const float *qb = qp + (size_t)qt * MT * Cp + kt * BK;
        const float *ab = ap + kt * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = t + MATCH_THREADS * i, row = f >> 3, c4 = f & 7;
            rq[i] = *reinterpret_cast<const float4 *>(qb + (size_t)row * Cp + c4 * 4);
            ra[i] = *reinterpret_cast<const float4 *>(ab + (size_t)row * Cp + c4 * 4);
        }
    };
    auto lstore = [&](int buf) {
        float *Qs = smem + buf * 2 * TILE_FLOATS, *As = Qs + TILE_FLOATS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = t + MATCH_THREADS * i, row = f >> 3, c4 = f & 7;
            float *q = Qs + row * LD + c4 * 4, *a = As + row * LD + c4 * 4;
            q[0] = rq[i].x; q[1] = rq[i].y; q[2] = rq[i].z; q[3] = rq[i].w;
            a[0] = ra[i].x; a[1] = ra[i].y; a[2] = ra[i].z; a[3] = ra[i].w;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.0f;

    if (nit > 0) {
        gload(0);
        fold.prefetch(qt_begin);
        lstore(0);
        fold.publish();
    }
    __syncthreads();

    for (int it = 0; it < nit; ++it) {
        const int cur = it & 1;
        const bool more = it + 1 < nit;
        const bool opens = more && (it + 1) % KT == 0;      // the next step is the first of a new query tile
        if (more) gload(it + 1);
        if (opens) fold.prefetch(qt_begin + (it + 1) / KT);

        // rows hold k in the permuted order written by K0 (position 8g+4h+j <- k = 8g+2j+h): MFMA step ks
        // (k = 2ks + hi) sits at position 8*(ks/4) + 4*hi + ks%4
        const float *Qs = smem + cur * 2 * TILE_FLOATS + (wm * 64 + l31) * LD + 4 * hi;
        const float *As = smem + cur * 2 * TILE_FLOATS + TILE_FLOATS + (wn * 64 + l31) * LD + 4 * hi;
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            const int kp = 8 * (ks >> 2) + (ks & 3);
            const float q0 = Qs[kp], q1 = Qs[32 * LD + kp];
            const float b0 = As[kp], b1 = As[32 * LD + kp];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(q0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(q0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(q1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(q1, b1, acc[1][1], 0, 0, 0);
        }

        // dot products of this query tile are complete: fold them
        if ((it % KT) == KT - 1) fold.tile(acc, qt_begin + it / KT);
        if (more) lstore(cur ^ 1);
        if (opens) fold.publish();
        __syncthreads();
    }
}

// The end of a staged kernel: each lane's two columns (ni) hold a running (distance, index) over ITS query rows.  Lane l and l+32 hold
// the same anchor column (different query rows), waves (wm=0, wn) and (wm=1, wn) hold the same columns: merged through LDS (the tiles
// are free now).  Thread t < MT leaves with column t's result in (d, i).  Holds a barrier.
__device__ __forceinline__ void staged_columns(float *smem, float (&best)[2], int (&bidx)[2], float &d, int &i)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const float od = __shfl_xor(best[ni], 32);
        const int oi = __shfl_xor(bidx[ni], 32);
        lex_min(best[ni], bidx[ni], od, oi);
    }
    float *sd = smem;
    int *si = reinterpret_cast<int *>(smem + 2 * MT);
    if (hi == 0) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            sd[wm * MT + wn * 64 + ni * 32 + l31] = best[ni];
            si[wm * MT + wn * 64 + ni * 32 + l31] = bidx[ni];
        }
    }
    __syncthreads();
    d = INFINITY;
    i = ROW_NONE;
    if (t < MT) {
        d = sd[t];
        i = si[t];
        lex_min(d, i, sd[MT + t], si[MT + t]);
    }
}

// ------------------------------------------------------------------------------------------------ C_pad 32 / 64 / 128 / 256
// Anchor-stationary.  Every wave keeps ITS 32 anchor rows - the MFMA B operand for the whole K range - in registers for the life of the
// workgroup, so the only thing that moves is the query stream:  HBM/L2 -> LDS by LDS-DMA (global_load_lds, 16 B per lane, no staging
// VGPRs), LDS -> MFMA A operand by ds_read_b128.
//   * LDS tile = 32 KB = ROWS query rows x KH floats, double-buffered (64 KB -> 2 workgroups per CU); ROWS = 64 and KH = 128 for
//     C_pad >= 128 (C_pad = 256 takes two k-parts per query tile).  A wave always runs 128 MFMAs (8192 cycles) per barrier, on
//     NACC = ROWS/32 >= 2 accumulators issued round-robin so that back-to-back MFMAs are independent.
//   * The k-permuted row layout written by K0 (position 8g+4h+j holds k = 8g+2j+h) makes one 16-byte access deliver what lane (i, h)
//     feeds to four consecutive MFMA steps, while the accumulation order stays the natural k order (bit-exact vs the oracle).
//   * LDS image: 256-byte lines, 16-byte slots XOR-swizzled with the row index: slot = chunk ^ (row & 15).  The DMA writes lane-linearly
//     (hardware constraint) from a per-lane pre-swizzled SOURCE address; the ds_read_b128 of a 16-lane group then hits 16 distinct slots
//     (rows distinct mod 16): conflict-free.
template <int CP> struct RegbGeom {
    static constexpr int RB = CP * 4;                          // source row bytes
    static constexpr int ROWS = CP >= 128 ? 64 : 8192 / CP;    // query rows per LDS tile
    static constexpr int KH = 8192 / ROWS;                     // k extent of one LDS tile
    static constexpr int KP = CP / KH;                         // k-parts per query tile (1 or 2)
    static constexpr int NACC = ROWS / 32;                     // 32x32 accumulators per wave
    static constexpr int NGT = KH / 8;                         // 8-wide k groups per LDS tile
    static constexpr int TILE_BYTES = 32768;
    static constexpr int NI = 8;                               // DMA wave-instructions per wave per tile (1 KB each)
    static constexpr int RG = NACC >= 4 ? 2 : 3;               // fragment ring depth, in k groups
    static constexpr bool NARROW = KH < 64;                    // two 128-byte rows share one 256-byte line
    static constexpr int LPR = NARROW ? 1 : KH * 4 / 256;      // 256-byte lines per tile row
    static_assert(NACC * NGT == 32 && KP * NGT * 8 == CP, "tile geometry");
};

// smem: 2 * TILE_BYTES, 256-byte aligned.  arow: THIS lane's anchor row (row wave*32 + l31 of the panel) + 4*hi.  qp: the pair's first
// query row.  acc[m]: query rows m*32.. of the tile against the wave's 32 anchor columns.
template <int CP, class Fold>
__device__ __forceinline__ void match_regb_walk(char *smem, const float *arow, const char *qp, TileSpan span,
                                                Fold &fold)
{
    using G = RegbGeom<CP>;
    constexpr int RB = G::RB, ROWS = G::ROWS, KH = G::KH, KP = G::KP, NACC = G::NACC, NGT = G::NGT, TILE_BYTES = G::TILE_BYTES;
    constexpr int NI = G::NI, RG = G::RG, LPR = G::LPR;
    constexpr bool NARROW = G::NARROW;
    const int qt_begin = span.begin, qt_end = span.end;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;

    // B operand: this lane's anchor row, positions 8g + 4*hi .. +3  (k = 8g + hi, +2, +4, +6)
    float4 breg[CP / 8];
#pragma unroll
    for (int g = 0; g < CP / 8; ++g) breg[g] = *reinterpret_cast<const float4 *>(arow + 8 * g);

    // LDS-DMA source offsets (bytes relative to the tile's first row / k-part), one per wave-instruction
    unsigned dma_off[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int line = (wave * NI + j) * 4 + (lane >> 4), sl = lane & 15;
        if (NARROW) {
            const int cc = sl ^ (line & 15);
            dma_off[j] = (unsigned)((line * 2 + (cc >> 3)) * RB + (cc & 7) * 16);
        } else {
            const int row = line / LPR;
            const int cc = sl ^ (row & 15);
            dma_off[j] = (unsigned)(row * RB + ((line % LPR) * 16 + cc) * 16);
        }
    }
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto issue = [&](int qt, int kp, int buf) {
        const char *qb = qp + (size_t)qt * ROWS * RB + kp * KH * 4;   // wave-uniform
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            char *dst = smem + buf * TILE_BYTES + (wave_u * NI + j) * 1024;
            unsigned off = dma_off[j];
            asm volatile("" : "+v"(off));      // scalar base + this 32-bit lane offset, not NI 64-bit lane pointers carried round the loop
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(qb + off),
                                             (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        }
    };

    // fragment (g, m): tile row m*32 + l31, chunk 2g + hi.
    //   wide  : byte = row*KH*4 + (chunk>>4)*256 + (((chunk&15) ^ (row&15)) << 4),   row&15 == l31&15
    //   narrow: line = row>>1 = m*16 + (l31>>1), byte = line*256 + ((((l31&1)*8 + chunk) ^ (line&15)) << 4)
    const unsigned rd_base = NARROW ? (unsigned)((l31 >> 1) * 256) : (unsigned)(l31 * KH * 4);
    const unsigned rd_key = NARROW ? (unsigned)(((l31 & 1) * 8 + hi) ^ ((l31 >> 1) & 15)) : (unsigned)(hi ^ (l31 & 15));
    auto rd = [&](int g, int m, unsigned tile) -> float4 {
        unsigned key = rd_key;
        asm volatile("" : "+v"(key));      // keep the 2-VALU address arithmetic here instead of 32 hoisted VGPRs
        const unsigned imm = NARROW ? (unsigned)(m * 4096) : (unsigned)(m * 32 * KH * 4 + (g >> 3) * 256);
        const unsigned off = rd_base + ((key ^ (2u * (g & 7))) << 4) + imm + tile;
        return *reinterpret_cast<const float4 *>(smem + off);
    };

    f32x16 acc[NACC];
#pragma unroll
    for (int m = 0; m < NACC; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;

    if (qt_end > qt_begin) {
        issue(qt_begin, 0, 0);
        fold.prefetch(qt_begin);
        fold.publish();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int buf = 0;
    for (int qt = qt_begin; qt < qt_end; ++qt) {
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            const bool opens = kp == KP - 1 && qt + 1 < qt_end;      // this step issues the first k-part of the next query tile
            if (kp + 1 < KP) issue(qt, kp + 1, buf ^ 1);
            else if (qt + 1 < qt_end) issue(qt + 1, 0, buf ^ 1);
            if (opens) fold.prefetch(qt + 1);
            const unsigned tile = buf * TILE_BYTES;
            float4 ring[RG][NACC];
#pragma unroll
            for (int g = 0; g < RG - 1; ++g)
#pragma unroll
                for (int m = 0; m < NACC; ++m) ring[g][m] = rd(g, m, tile);
#pragma unroll
            for (int g = 0; g < NGT; ++g) {
                // reads of group g+RG-1 go out first (their ring slot was freed by group g-1), then the 4*NACC MFMAs of
                // group g, accumulators round-robin so consecutive MFMAs are independent
                if (g + RG - 1 < NGT) {
#pragma unroll
                    for (int m = 0; m < NACC; ++m) ring[(g + RG - 1) % RG][m] = rd(g + RG - 1, m, tile);
                }
                const float4 bv = breg[kp * NGT + g];
#pragma unroll
                for (int m = 0; m < NACC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[g % RG][m].x, bv.x, acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < NACC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[g % RG][m].y, bv.y, acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < NACC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[g % RG][m].z, bv.z, acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < NACC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[g % RG][m].w, bv.w, acc[m], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (kp == KP - 1) fold.tile(acc, qt);
            if (opens) fold.publish();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            buf ^= 1;
        }
    }
}

}  // namespace oryon
