// K1s: cosine nearest neighbour with an fp16-MFMA SCREENING pass and an exact fp32 re-scoring pass.
//
// Same contract as K1 (utils/pcd.py:202-205: dist = 0.5*(1-cos), row amin/argmin, < threshold) for every
// anchor row that can possibly be valid, at a fraction of the fp32-MFMA cost:
//
//   screen  s16_ij = a16_i . q16_j on v_mfma_f32_32x32x16_f16 (IEEE-half copies of the unit rows, fp32 accumulate);
//           per anchor the maximum max_i, the 16-row slice it lies in and the best maximum of any other slice are kept (MODE 2).
//   pass 1  every j with s16_ij >= max_i - MARGIN goes to anchor i's candidate list: from the winning slice alone where the
//           runner-up slice is further than MARGIN away (match_decide_kernel), else by the same products again over the compacted
//           ambiguous anchors (MODE 1).  Rows with max_i < (1 - 2*threshold) - DELTA can never pass the threshold: no candidates,
//           valid = 0.
//   pass 2  candidates are re-scored with the canonical fp32 fmaf chain of K1 (bit-exact vs the oracle) and the first
//           index of the smallest distance wins.  Lists that overflow (duplicate-heavy inputs) flag their anchor panel,
//           which is then recomputed by the exact fp32 kernel (match_f32_regb_kernel) - still no host round trip.
//
// Why this is exact.  For unit rows |a16.q16 - a.q| <= DELTA with
//   DELTA = (2^-10 + 2^-22) * sum|a_k q_k|   (two half roundings per product, sum|a_k q_k| <= |a||q| = 1)
//         + 2 * C * 2^-24                     (fp32 accumulation of the MFMA and of the canonical chain)  ~= 1.04e-3  (C <= 512).
// If j* minimises the exact distance then a.q_j* >= max_j a.q_j - 2^-23 (dist is a monotone rounding of the dot), hence
// s16_ij* >= max_j s16_ij - 2*DELTA - 2^-23: every exact minimiser - including every tied one - is in the list, and pass 2
// returns exactly what the full fp32 scan returns.  MARGIN = 2.2e-3 > 2*DELTA + 2^-23.
// Subnormal half inputs (|x| < 2^-14, common in unit rows of 256+ channels) are honoured by v_mfma_f32_32x32x16_f16 on gfx950
// (tools/probe_mfma_f16_denorm.hip, measured), and K0's float->half conversion keeps them, so they round with an absolute
// error <= 2^-25 each: <= 2 * 2^-25 * sqrt(C) ~= 1.3e-6 in the dot product, inside the slack of SCREEN_DELTA.
#include <hip/hip_fp16.h>
#include <stdlib.h>
#include <type_traits>
#include "common.h"
#include "match_common.h"
#include "screen_tile.h"
#include "match_exact.h"

namespace oryon {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr float SCREEN_DELTA = 1.05e-3f;
constexpr float SCREEN_MARGIN = 2.2e-3f;
constexpr int SCREEN_CAP = 64;          // candidate slots per anchor
constexpr int screen_tile_bytes(int CP) { return CP == 512 ? 65536 : 32768; }

// Out-of-line candidate append (pass 1 slow path, taken by a few % of the tiles): keeping it out of the kernel body
// keeps the hot loop's register allocation identical to pass 0.  vals: this lane's NV scores of one anchor column.
template <int NV>
__device__ __noinline__ void emit_candidates(const float *vals, float thr, int qlane, size_t arow, int32_t *cnt, int32_t *cand)
{
    for (int e = 0; e < NV; ++e)
        if (vals[e] >= thr) {
            const int r = e & 15, qb = e >> 4;
            const int sl = atomicAdd(&cnt[arow], 1);
            if (sl < SCREEN_CAP) cand[arow * SCREEN_CAP + sl] = qlane + qb * 32 + (r & 3) + 8 * (r >> 2);
        }
}

template <int CP, int MODE>   // MODE 2: the pass over all anchors (slice maxima); MODE 1: the candidate pass over the ambiguous ones
__global__ __launch_bounds__(256, CP == 512 ? 1 : 2) void match_f16_screen_kernel(
    const __half *__restrict__ a16, const __half *__restrict__ q16, int B, int cap_a, int cap_q,
    const int32_t *__restrict__ n_a, const int32_t *__restrict__ n_q, int T, int S, float valid_cut,
    float *__restrict__ ws_max /*[B,S_thr|S,cap_a]*/, int32_t *__restrict__ cnt /*[B,cap_a]*/, int32_t *__restrict__ cand,
    int S_thr, const int32_t *__restrict__ row_map, int32_t *__restrict__ ws_i1, float *__restrict__ ws_m2)
{
    constexpr int RB = CP * 2;                   // row bytes
    constexpr int TILE_BYTES = screen_tile_bytes(CP);   // 32 KB; 64 KB at C=512 (one workgroup per CU, 512 registers per lane)
    constexpr int ROWS = TILE_BYTES / RB;        // query rows per LDS tile (64 at C=256 and C=512)
    constexpr int NQB = ROWS / 32;               // query blocks per tile
    constexpr int NAB = 2;                       // anchor blocks per wave
    constexpr int NKS = CP / 16;                 // MFMA k-steps
    constexpr int NI = TILE_BYTES / 4096;        // 1 KB DMA instructions per wave and tile
    constexpr int LPR = RB / 256;                // 256-byte lines per row
    static_assert(NQB * NKS * 1024 == TILE_BYTES && NQB >= 1 && LPR >= 1, "tile geometry");
    char *smem;
    if constexpr (2 * TILE_BYTES > 65536) {      // beyond the static LDS limit: dynamic, sized by the launcher
        extern __shared__ __attribute__((aligned(256))) char smem_dyn[];
        smem = smem_dyn;
    } else {
        __shared__ __attribute__((aligned(256))) char smem_st[2 * TILE_BYTES];
        smem = smem_st;
    }

    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int unit = (slot / T) * 8 + xcd;
    if (unit >= B * S) return;
    const int panel = slot % T;
    const int p = unit / S, split = unit % S;
    const int na = n_a[p], nq = n_q[p];
    const int a0 = panel * MT16;
    if (a0 >= na) return;
    const int nqt = (nq + ROWS - 1) / ROWS;
    const int qt_per = (nqt + S - 1) / S;
    const int qt_begin = split * qt_per;
    const int qt_end = (qt_begin + qt_per < nqt) ? qt_begin + qt_per : nqt;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const char *qp = reinterpret_cast<const char *>(q16 + (size_t)p * cap_q * CP);

    // stationary B operand: anchors a0 + wave*64 + ab*32 + l31, k-step s -> halves 16s + 8hi .. +7
    half8 breg[NAB][NKS];
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab) {
        const __half *arow = a16 + ((size_t)p * cap_a + a0 + wave * 64 + ab * 32 + l31) * CP + 8 * hi;
#pragma unroll
        for (int s = 0; s < NKS; ++s) breg[ab][s] = *reinterpret_cast<const half8 *>(arow + 16 * s);
    }

    unsigned dma_off[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int line = (wave * NI + j) * 4 + (lane >> 4), sl = lane & 15;
        const int row = line / LPR;
        const int cc = sl ^ (row & 15);
        dma_off[j] = (unsigned)(row * RB + ((line % LPR) * 16 + cc) * 16);
    }
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto issue = [&](int qt, int buf) {
        const char *qb = qp + (size_t)qt * TILE_BYTES;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            char *dst = smem + buf * TILE_BYTES + (wave_u * NI + j) * 1024;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(qb + dma_off[j]),
                                             (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        }
    };
    // swizzled operand addresses: 8 per-lane offsets in registers, the rest immediates / one add per tile (VALU and MFMA issue
    // serialise on a SIMD: every VALU instruction taken out of the loop is MFMA time)
    unsigned koff[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) koff[c] = (unsigned)(l31 * RB) + ((((unsigned)(hi ^ (l31 & 15))) ^ (2u * c)) << 4);
    auto rd = [&](int s, int qb, unsigned tile) -> half8 {
        return *reinterpret_cast<const half8 *>(smem + koff[s & 7] + tile + (unsigned)(qb * 32 * RB + (s >> 3) * 256));
    };

    f32x16 acc[NQB][NAB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
        for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[qb][ab][r] = 0.0f;

    float runmax[NAB], thr[NAB], run2[NAB];
    int runidx[NAB];
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab) {
        runmax[ab] = -INFINITY;
        run2[ab] = -INFINITY;
        runidx[ab] = 0;
        thr[ab] = INFINITY;
        if (MODE == 1) {
            const int a = a0 + wave * 64 + ab * 32 + l31;
            float m = -INFINITY;
            for (int s = 0; s < S_thr; ++s) m = fmaxf(m, ws_max[((size_t)p * S_thr + s) * cap_a + a]);
            thr[ab] = (a < na && m >= valid_cut) ? m - SCREEN_MARGIN : INFINITY;
        }
    }

    if (qt_end > qt_begin) issue(qt_begin, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int buf = 0;
    for (int qt = qt_begin; qt < qt_end; ++qt) {
        if (qt + 1 < qt_end) issue(qt + 1, buf ^ 1);
        const unsigned tile = buf * TILE_BYTES;
        half8 ring[2][NQB];
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) ring[0][qb] = rd(0, qb, tile);
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            if (s + 1 < NKS) {
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) ring[(s + 1) & 1][qb] = rd(s + 1, qb, tile);
            }
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                for (int ab = 0; ab < NAB; ++ab)
                    acc[qb][ab] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ring[s & 1][qb], breg[ab][s], acc[qb][ab], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // epilogue: lane owns anchor column (ab, l31); rows of the C/D block are queries.
        // Rows >= n_q of the last tile need no masking: K0 zero-fills them, so they score exactly 0, which can neither
        // reach valid_cut (> 0 for thresholds < 0.5) nor a candidate threshold; pass 2 ignores indices >= n_q anyway.
        const int qlane = qt * ROWS + 4 * hi;
#pragma unroll
        for (int ab = 0; ab < NAB; ++ab) {
            float m = -INFINITY;
            if (MODE != 2) {
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) m = fmaxf(m, acc[qb][ab][r]);
            }
            if (MODE == 2) {
                // per (tile, query block) SLICE maxima only: running (m1, slice id of m1, m2 = best slice maximum other than
                // m1's slice).  16 rows of one lane half form a slice; what happens INSIDE the winning slice is resolved by
                // match_decide_kernel, which re-scores just those 16 rows.
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) {
                    float x = acc[qb][ab][0];
#pragma unroll
                    for (int r = 1; r < 16; ++r) x = fmaxf(x, acc[qb][ab][r]);
                    const bool improved = x > runmax[ab];
                    run2[ab] = fmaxf(fminf(runmax[ab], x), run2[ab]);
                    runmax[ab] = fmaxf(runmax[ab], x);
                    runidx[ab] = improved ? ((qt * NQB + qb) * 2 + hi) : runidx[ab];
                }
            } else if (__any(m >= thr[ab])) {
                float vals[NQB * 16];
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) vals[qb * 16 + r] = acc[qb][ab][r];
                const int acol = a0 + wave * 64 + ab * 32 + l31;
                const int aout = (row_map && acol < na) ? row_map[(size_t)p * cap_a + acol] : acol;
                emit_candidates<NQB * 16>(vals, thr[ab], qlane, (size_t)p * cap_a + aout, cnt, cand);
            }
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[qb][ab][r] = 0.0f;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
    }
    // (cap_a is a multiple of this kernel's 256-anchor panels: the helper's a < cap_a holds for every lane)
    if (MODE == 2) screen_merge_store<NAB>(runmax, run2, runidx, a0 + wave * 64 + l31, hi, (size_t)p * S + split, cap_a, ws_max, ws_i1, ws_m2);
}

// Single-pass strategy, step 2 (one wave per anchor): merge the per-split (m1, slice of m1, m2) triples and decide
//   m1 < valid_cut        -> can never be valid                                        (no candidates)
//   m1 - m2 > MARGIN      -> every index within MARGIN of m1 lies in m1's 16-row slice: those 16 rows are re-scored here
//                            from the fp16 rows (fp32 accumulate) and the ones within MARGIN (+ recomputation slack) become
//                            the candidates
//   otherwise             -> ambiguous: appended to the pair's list; a second, compacted screening pass collects every
//                            index within MARGIN for these anchors only.
template <int ROWS_TILE>
__global__ __launch_bounds__(256) void match_decide_kernel(const __half *__restrict__ a16, const __half *__restrict__ q16, int Cp,
                                                            int cap_a, int cap_q, const int32_t *__restrict__ n_a,
                                                            const int32_t *__restrict__ n_q, int S, float valid_cut,
                                                            const float *__restrict__ ws_m1, const int32_t *__restrict__ ws_i1,
                                                            const float *__restrict__ ws_m2, float *__restrict__ m_final,
                                                            int32_t *__restrict__ cnt, int32_t *__restrict__ cand,
                                                            int32_t *__restrict__ n_amb, int32_t *__restrict__ amb_idx,
                                                            const float *__restrict__ a_scale8, const float *__restrict__ eps_a8,
                                                            const float *__restrict__ eps_q8, float cut0, float sqrt_c, float c_true,
                                                            const int8_t *__restrict__ a8, const int8_t *__restrict__ q8,
                                                            const float *__restrict__ q_scale8)
{
    // a_scale8 != nullptr: the (m1, slice, m2) triples come from the INT8 screening pass (K1s8) in units of 2^-E_a per anchor
    // slice; margin and validity cut then follow the per-anchor int8 bound DELTA8 (match_exact.h: i8_bound).  The slice ids do not
    // depend on ROWS_TILE: sid >> 1 = tile * (ROWS_TILE / 32) + block is the 32-row query block either way (slice_row).
    // 16 anchors per wave: an empty launch (the fp16 stage behind K1s8 usually has nothing to do) costs 5 k workgroups, not 80 k
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int n_anchors = n_a[p];
    const float valid_cut_in = valid_cut;
    auto one_anchor = [&](const int a) {
    float valid_cut = valid_cut_in;
    const size_t arow = (size_t)p * cap_a + a;
    float m1, m2;
    int sid;
    merge_split_triples(ws_m1, ws_i1, ws_m2, p, S, cap_a, a, m1, sid, m2);
    float margin = SCREEN_MARGIN, sa = 1.0f;
    if (a_scale8) {
        sa = a_scale8[(size_t)p * (cap_a / 16) + anchor_scale_slot(a)];           // 2^-E of the anchor's slice
        m1 *= sa;                                             // exact: power of two
        m2 *= sa;
        (void)eps_a8;
        const ScreenBound b = i8_bound(sa, eps_q8[p], sqrt_c, c_true);
        margin = b.margin();                                  // degenerate scales (not usable): +inf, -inf - left to the fp16 pass
        valid_cut = b.usable() ? b.cannot_line(cut0) : -INFINITY;
    }
    if (lane == 0) m_final[arow] = m1;
    if (!(m1 >= valid_cut)) {
        if (a_scale8 && lane == 0) cnt[arow] = -1;            // int8 mode: "cannot be valid" is carried by the count
        return;
    }
    if (!(m1 - m2 > margin)) {
        if (lane == 0) {
            const int sl = atomicAdd(&n_amb[p], 1);
            amb_idx[(size_t)p * cap_a + sl] = a;
        }
        return;
    }
    // the 16 rows of the winning slice re-scored by the wave (match_exact.h: 4 lanes per row), the hits become the candidates
    const int seg = lane & 3;
    const int q = slice_row(sid, lane >> 2);
    const int nq = n_q[p];
    bool hit;
    if (a_scale8) {
        // int8 mode: every row within the int8 margin of the slice maximum (= m1 exactly) goes to the exact fp32 re-scoring
        const int idot = slice_score_i8(a8 + arow * Cp, q8 + (size_t)p * cap_q * Cp, q, Cp, q < nq);
        const float s8 = (float)idot * q_scale8[(size_t)p * (cap_q / 16) + sid] * sa;
        hit = (seg == 0) && (q < nq) && (s8 >= m1 - margin);
    } else {
        const float sdot = slice_score_f16(a16 + arow * Cp, q16 + (size_t)p * cap_q * Cp, q, Cp, q < nq);
        hit = (seg == 0) && (q < nq) && (sdot >= m1 - SCREEN_MARGIN - 4e-5f);
    }
    const unsigned long long b = __ballot(hit);
    if (hit) cand[arow * SCREEN_CAP + __popcll(b & ((1ull << lane) - 1ull))] = q;
    if (lane == 0) cnt[arow] = __popcll(b);
    };
    for (int g = 0; g < 16; ++g) {
        const int a = (blockIdx.x * 16 + g) * 4 + (threadIdx.x >> 6);
        if (a >= n_anchors) break;
        one_anchor(a);
    }
}

// gather the fp16 rows (and thresholds) of the ambiguous anchors into a dense panel layout for the second pass
__global__ __launch_bounds__(256) void match_compact_kernel(const __half *__restrict__ a16, int Cp, int cap_a,
                                                             const int32_t *__restrict__ n_amb, const int32_t *__restrict__ amb_idx,
                                                             const float *__restrict__ m_final, __half *__restrict__ a16c,
                                                             float *__restrict__ amb_max)
{
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int n_sl = n_amb[p];
    for (int g = 0; g < 16; ++g) {
    const int sl = (blockIdx.x * 16 + g) * 4 + (threadIdx.x >> 6);
    if (sl >= n_sl) break;
    const int a = amb_idx[(size_t)p * cap_a + sl];
    const uint4 *src = reinterpret_cast<const uint4 *>(a16 + ((size_t)p * cap_a + a) * Cp);
    uint4 *dst = reinterpret_cast<uint4 *>(a16c + ((size_t)p * cap_a + sl) * Cp);
    for (int i = lane; i < Cp / 8; i += 64) dst[i] = src[i];
    if (lane == 0) amb_max[(size_t)p * cap_a + sl] = m_final[(size_t)p * cap_a + a];
    }
}

// pass 2: L lanes per anchor row, candidates strided over them; canonical fp32 chain on the k-permuted fp32 rows.  Almost
// every anchor has ONE candidate and the chain is a serial 256-step fmaf per (anchor, candidate): few lanes per anchor keep
// more lanes of a wave busy.
// The body of both entries, which differ in cand_dot(ar, jj): the canonical dot product of the anchor row at ar with query row jj.  CUT
// (the fp16 screen): rows whose screening maximum screen_max(arow, a) lies below valid_cut are not re-scored; behind the int8 screen the
// count -1 carries that and the maximum is read for the estimate only.  need_f32 (may be null): raised for the pair with an overflow.
template <int L, bool CUT, class ScreenMax, class CandDot>
__device__ __forceinline__ void rescore_rows(const float *__restrict__ a_hat, int Cp, int cap_a, const int32_t *__restrict__ n_a,
                                             const int32_t *__restrict__ n_q, float thr, float valid_cut, const int32_t *__restrict__ cnt,
                                             const int32_t *__restrict__ cand, float *__restrict__ min_dist, int32_t *__restrict__ argmin,
                                             uint8_t *__restrict__ valid, uint8_t *__restrict__ row_flag, int32_t *__restrict__ panel_flag,
                                             int32_t *__restrict__ need_f32, ScreenMax screen_max, CandDot cand_dot)
{
    const int p = blockIdx.y;
    const int a = blockIdx.x * (256 / L) + (threadIdx.x / L), sub = threadIdx.x % L;
    const bool live = a < n_a[p];
    const size_t arow = (size_t)p * cap_a + (live ? a : 0);
    float m16 = -INFINITY;
    if (CUT && live) m16 = screen_max(arow, a);
    const int c_raw = live ? cnt[arow] : 0;
    const bool possible = live && (!CUT || m16 >= valid_cut) && c_raw >= 0;      // count -1: ruled out by the int8 stage
    const int c = possible ? c_raw : 0;
    const bool overflow = c > SCREEN_CAP;
    float d = INFINITY;
    int j = 0x7fffffff;
    if (!overflow) {
        const float *ar = a_hat + arow * Cp;
        const int nq_p = n_q[p];
        for (int ci = sub; ci < c; ci += L) {
            const int jj = cand[arow * SCREEN_CAP + ci];
            if (jj >= nq_p) continue;                     // zero-padded query rows can never be the answer
            lex_min(d, j, dist_from_dot(cand_dot(ar, jj)), jj);
        }
    }
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) {
        const float od = __shfl_xor(d, off);
        const int oj = __shfl_xor(j, off);
        lex_min(d, j, od, oj);
    }
    if (!live || sub != 0) return;
    if (!possible) {                    // cannot reach the threshold: report the screening estimate, valid = 0
        min_dist[arow] = dist_from_dot(CUT ? m16 : screen_max(arow, a));
        argmin[arow] = 0;
        valid[arow] = 0;
    } else if (overflow) {              // list overflow: the exact fp32 kernel recomputes this anchor's panel
        row_flag[arow] = 1;
        panel_flag[(size_t)p * (cap_a / ORYON_MATCH_TILE) + a / ORYON_MATCH_TILE] = 1;
        if (need_f32) need_f32[p] = 1;
    } else {
        min_dist[arow] = d;
        argmin[arow] = j;
        valid[arow] = (d < thr) ? 1 : 0;
    }
}

template <int L>
__global__ __launch_bounds__(256) void match_rescore_kernel(const float *__restrict__ a_hat, const float *__restrict__ q_hat,
                                                             int Cp, int cap_a, int cap_q, const int32_t *__restrict__ n_a,
                                                             const int32_t *__restrict__ n_q, int S, float thr, float valid_cut,
                                                             const float *__restrict__ ws_max, const float *__restrict__ m_final,
                                                             const int32_t *__restrict__ cnt,
                                                             const int32_t *__restrict__ cand, float *__restrict__ min_dist,
                                                             int32_t *__restrict__ argmin, uint8_t *__restrict__ valid,
                                                             uint8_t *__restrict__ row_flag, int32_t *__restrict__ panel_flag)
{
    const int p = blockIdx.y;
    rescore_rows<L, true>(
        a_hat, Cp, cap_a, n_a, n_q, thr, valid_cut, cnt, cand, min_dist, argmin, valid, row_flag, panel_flag, nullptr,
        [&](size_t arow, int a) {
            if (m_final) return m_final[arow];
            float m16 = -INFINITY;
            for (int s = 0; s < S; ++s) m16 = fmaxf(m16, ws_max[((size_t)p * S + s) * cap_a + a]);
            return m16;
        },
        [&](const float *ar, int jj) {                    // materialised query rows, k-permuted like the anchors'
            const float *qr = q_hat + ((size_t)p * cap_q + jj) * Cp;
            float dot = 0.0f;
            for (int g = 0; g < Cp; g += 8) {
                const float4 a0 = *reinterpret_cast<const float4 *>(ar + g), a1 = *reinterpret_cast<const float4 *>(ar + g + 4);
                float x[8];
                kperm_group_natural(*reinterpret_cast<const float4 *>(qr + g), *reinterpret_cast<const float4 *>(qr + g + 4), x);
                dot = chain_step8(a0, a1, x, dot);
            }
            return dot;
        });
}

// pass 2 for the K1s8 path fed by K0v3 (gather8.hip), which writes NO fp32 copy of the query rows: a candidate's canonical unit
// values are recovered on the fly as x_k / d from the raw descriptor map and the row norm d K0 stored (the same IEEE division K0's
// fp32 rows come from, so the chain below is bit for bit the one match_rescore_kernel runs on materialised rows).  Anchor rows are
// the materialised, k-permuted fp32 rows (5000 per pair).  Candidates of neighbouring anchors are neighbouring query pixels on real
// (and synthetic) rigid pairs, so the strided 4-byte reads of an NCHW map share their 64-byte sectors across a wave.
template <int L, bool NHWC>
__global__ __launch_bounds__(256) void match_rescore_raw_kernel(
    const float *__restrict__ a_hat, const float *__restrict__ feat_q, int C_true, int HW, const int32_t *__restrict__ roi_q,
    int roi_stride, const float *__restrict__ norm_q, int Cp, int cap_a, int cap_q, const int32_t *__restrict__ n_a,
    const int32_t *__restrict__ n_q, float thr, const float *__restrict__ m_final, const int32_t *__restrict__ cnt,
    const int32_t *__restrict__ cand, float *__restrict__ min_dist, int32_t *__restrict__ argmin, uint8_t *__restrict__ valid,
    uint8_t *__restrict__ row_flag, int32_t *__restrict__ panel_flag, int32_t *__restrict__ need_f32, int round_f16)
{
    const int p = blockIdx.y;
    const float *fq = feat_q + (size_t)p * C_true * HW;
    rescore_rows<L, false>(
        a_hat, Cp, cap_a, n_a, n_q, thr, 0.0f, cnt, cand, min_dist, argmin, valid, row_flag, panel_flag, need_f32,
        [&](size_t arow, int) { return m_final[arow]; },
        [&](const float *ar, int jj) {
            const int pix = roi_q[(size_t)p * roi_stride + jj];
            const float dq = norm_q[(size_t)p * cap_q + jj];
            float dot = 0.0f;
            for (int g = 0; g < C_true; g += 8) {
                const float4 a0 = *reinterpret_cast<const float4 *>(ar + g), a1 = *reinterpret_cast<const float4 *>(ar + g + 4);
                float x[8];
                if constexpr (NHWC) {
                    if (g + 8 <= C_true) {
                        const float4 q0 = *reinterpret_cast<const float4 *>(fq + (size_t)pix * C_true + g);
                        const float4 q1 = *reinterpret_cast<const float4 *>(fq + (size_t)pix * C_true + g + 4);
                        x[0] = q0.x; x[1] = q0.y; x[2] = q0.z; x[3] = q0.w; x[4] = q1.x; x[5] = q1.y; x[6] = q1.z; x[7] = q1.w;
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) x[e] = g + e < C_true ? fq[(size_t)pix * C_true + g + e] : 0.0f;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[e] = g + e < C_true ? fq[(size_t)(g + e) * HW + pix] : 0.0f;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = unit_value(x[e], dq, round_f16);
                dot = chain_step8(a0, a1, x, dot);
            }
            // channels C_true .. Cp-1 are zero on both sides: fma(0, 0, dot) leaves dot unchanged, nothing to add
            return dot;
        });
}

// pairs that need materialised fp32 query rows: undecided anchors (fp16 stage) or an overflowed candidate list (exact panel scan)
__global__ void match_need_f32_kernel(int B, const int32_t *__restrict__ n_amb, int32_t *__restrict__ need_f32)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < B && n_amb[p] > 0) need_f32[p] = 1;
}

// ------------------------------------------------------------------------------------------------ K1s8: int8 pre-screen
// The same single-pass (m1, slice, m2) screening as MODE 2 above on v_mfma_i32_32x32x32_i8 - twice the fp16 matrix rate on
// gfx950 (3.4 POP/s sustained vs 1.7 PFLOP/s, tools/probe_mfma_rates.hip), half the operand bytes, 128 query rows per 32 KB
// tile.  K0 writes q = rint(x^ * 2^E) with one exponent per 16-row slice, so inside a slice the integer maximum IS the score
// maximum and the epilogue costs what the fp16 one costs: integer max tree, one convert, one multiply by the slice's 2^-E.
// Accumulation is exact (|sum| <= 512 * 127^2 < 2^24).
//
// Bound: with ea = 2^-(E_a+1), eq = max over the pair's query slices of 2^-(E_q+1):
//   |s8_ij - a^_i.q^_j| <= ea*|q^_j|_1 + eq*|a^_i|_1 + C*ea*eq <= (ea + eq)*sqrt(C) + C*ea*eq =: DELTA8_i   (unit rows: |x|_1 <= sqrt(C)).
// match_decide_kernel then decides per anchor exactly as for fp16, with DELTA8_i in place of DELTA:
//   m1 < (1-2thr) - DELTA8      -> cannot be valid
//   m1 - m2 > 2*DELTA8          -> every exact minimiser lies in m1's slice: its 16 rows are re-scored in fp16, candidates -> exact
//                                  fp32 re-scoring (unchanged)
//   otherwise                   -> the anchor is handed to the fp16 screening (compacted set, complete K1s pipeline), so the int8
//                                  stage can only ever lose time, never exactness.
typedef int i32x16 __attribute__((ext_vector_type(16)));

template <int CP>
__global__ __launch_bounds__(256, CP == 512 ? 1 : 2) void match_i8_screen_kernel(
    const int8_t *__restrict__ a8, const int8_t *__restrict__ q8, const float *__restrict__ q_scale, int B, int cap_a, int cap_q,
    const int32_t *__restrict__ n_a, const int32_t *__restrict__ n_q, int T, int S, float *__restrict__ ws_max,
    int32_t *__restrict__ ws_i1, float *__restrict__ ws_m2)
{
    constexpr int RB = CP;                       // row bytes
    constexpr int TILE_BYTES = screen8_tile_bytes(CP);
    constexpr int NQB = 4, NAB = 2;
    constexpr int NKS = CP / 32;                 // MFMA k-steps
    constexpr int NI = TILE_BYTES / 4096;
    char *smem;
    if constexpr (2 * TILE_BYTES > 65536) {
        extern __shared__ __attribute__((aligned(256))) char smem_dyn8[];
        smem = smem_dyn8;
    } else {
        __shared__ __attribute__((aligned(256))) char smem_st8[2 * TILE_BYTES];
        smem = smem_st8;
    }
    ScreenUnit u;
    if (!screen_unit_decode(u, MT16, B, T, S, n_a, n_q)) return;
    const int p = u.p, split = u.split, a0 = u.a0;
    int qt_begin, qt_end;
    screen_split_tiles(u, S, qt_begin, qt_end);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const char *qp = reinterpret_cast<const char *>(q8) + (size_t)p * cap_q * RB;
    const float2 *qs = reinterpret_cast<const float2 *>(q_scale + (size_t)p * (cap_q / 16));    // (h = 0, h = 1) per 32-row block

    // stationary B operand: anchors a0 + wave*64 + ab*32 + l31, k-step s -> bytes 32s + 16hi .. +15
    i32x4 breg[NAB][NKS];
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab) {
        const char *arow = reinterpret_cast<const char *>(a8) + ((size_t)p * cap_a + a0 + wave * 64 + ab * 32 + l31) * RB + 16 * hi;
#pragma unroll
        for (int s = 0; s < NKS; ++s) breg[ab][s] = *reinterpret_cast<const i32x4 *>(arow + 32 * s);
    }
    unsigned dma_off[NI];
    screen_dma_offsets<RB>(dma_off, wave * NI, lane);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto issue = [&](int qt, int buf) {
        const char *qb = qp + (size_t)qt * TILE_BYTES;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            char *dst = smem + buf * TILE_BYTES + (wave_u * NI + j) * 1024;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(qb + dma_off[j]),
                                             (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        }
    };
    // swizzled operand addresses: 8 per-lane offsets (one per 16-byte chunk pair of a 256-byte line) live in registers, everything
    // else (query block, line, tile) is an immediate or one add per tile - VALU and MFMA issue serialise on a SIMD of this chip
    // (tools/probe_mfma_valu_overlap.hip), so every VALU instruction taken out of the loop is MFMA time
    unsigned koff[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) koff[c] = (unsigned)(l31 * RB) + ((((unsigned)(hi ^ (l31 & 15))) ^ (2u * c)) << 4);
    auto rd = [&](int s, int qb, unsigned tile) -> i32x4 {
        return *reinterpret_cast<const i32x4 *>(smem + koff[s & 7] + tile + (unsigned)(qb * 32 * RB + (s >> 3) * 256));
    };

    i32x16 acc[NQB][NAB];
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
        for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[qb][ab][r] = 0;
    float runmax[NAB], run2[NAB];
    int runidx[NAB];
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab) { runmax[ab] = -INFINITY; run2[ab] = -INFINITY; runidx[ab] = 0; }

    if (qt_end > qt_begin) issue(qt_begin, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0;
    for (int qt = qt_begin; qt < qt_end; ++qt) {
        if (qt + 1 < qt_end) issue(qt + 1, buf ^ 1);
        float2 sc2[NQB];
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) sc2[qb] = qs[qt * NQB + qb];
        const unsigned tile = buf * TILE_BYTES;
        i32x4 ring[2][NQB];
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) ring[0][qb] = rd(0, qb, tile);
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            if (s + 1 < NKS) {
#pragma unroll
                for (int qb = 0; qb < NQB; ++qb) ring[(s + 1) & 1][qb] = rd(s + 1, qb, tile);
            }
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
                for (int ab = 0; ab < NAB; ++ab)
                    acc[qb][ab] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ring[s & 1][qb], breg[ab][s], acc[qb][ab], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // epilogue: slice maxima.  Zero-padded rows score exactly 0 and cannot reach any cut (> 0).
#pragma unroll
        for (int ab = 0; ab < NAB; ++ab) {
#pragma unroll
            for (int qb = 0; qb < NQB; ++qb) {
                int xi = acc[qb][ab][0];
#pragma unroll
                for (int r = 1; r < 16; ++r) xi = max(xi, acc[qb][ab][r]);
                const float x = (float)xi * (hi ? sc2[qb].y : sc2[qb].x);
                const bool improved = x > runmax[ab];
                run2[ab] = fmaxf(fminf(runmax[ab], x), run2[ab]);
                runmax[ab] = fmaxf(runmax[ab], x);
                runidx[ab] = improved ? ((qt * NQB + qb) * 2 + hi) : runidx[ab];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[qb][ab][r] = 0;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
    }
    // (cap_a is a multiple of this kernel's 256-anchor panels: the helper's a < cap_a holds for every lane)
    screen_merge_store<NAB>(runmax, run2, runidx, a0 + wave * 64 + l31, hi, (size_t)p * S + split, cap_a, ws_max, ws_i1, ws_m2);
}

// Round-2 restructuring of the int8 screening loop (same operands, same outputs, same tiles as match_i8_screen_kernel).
// Round 1 ran all 8 (query block, anchor block) accumulators of a tile through the k loop together, then reduced them: ~180 VALU +
// 128 accumulator zeroings per 64 MFMAs, none of which overlapped matrix work (PMC: 68 % MFMA-pipe utilisation).  Here a query
// block's TWO anchor-block chains (8 k-steps each, alternating so no MFMA waits on its predecessor's accumulator) run to completion
// before the next query block starts, so
//   * the slice-maximum epilogue of query block qb-1 (2 x {v_max3 tree, convert, scale, running (m1, slice, m2) update}) is issued
//     in the shadow of query block qb's 16 MFMAs - the matrix pipe executes 32 cycles per MFMA, the wave issues one every ~32;
//   * accumulators start from the inline constant 0 (first MFMA of a chain takes C = 0): no zeroing;
//   * 4 accumulators are live instead of 8, which pays for a double-buffered A operand (the 8 ds_read_b128 of query block qb+1
//     also issue under qb's MFMAs).
// sched_group_barrier pins the interleave (1 MFMA : 2 VALU : <=1 LDS read) in the emitted code.
// WAVES = 8: 512 anchors per workgroup - the eight waves share ONE query-tile stream (half the L2 -> LDS bytes, DMA issues and LDS footprint per
// anchor of two 4-wave workgroups on a CU); T is then the number of 512-anchor panels.
template <int CP, int VAR = 0, int WAVES = 4>     // VAR != 0: timing ablations only (ORYON_SCREEN8_ABLATE): 1 no epilogue, 2 no DMA / barrier, 8 DMA spread over two blocks
__global__ __launch_bounds__(64 * WAVES, CP == 512 ? 1 : 2) void match_i8_screen_v2_kernel(
    const int8_t *__restrict__ a8, const int8_t *__restrict__ q8, const float *__restrict__ q_scale, int B, int cap_a, int cap_q,
    const int32_t *__restrict__ n_a, const int32_t *__restrict__ n_q, int T, int S, float *__restrict__ ws_max,
    int32_t *__restrict__ ws_i1, float *__restrict__ ws_m2)
{
    constexpr int RB = CP;
    constexpr int TILE_BYTES = screen8_tile_bytes(CP);
    constexpr int NQB = 4, NAB = 2;
    constexpr int NKS = CP / 32;
    constexpr int NI = TILE_BYTES / (1024 * WAVES);
    char *smem;
    if constexpr (2 * TILE_BYTES > 65536) {
        extern __shared__ __attribute__((aligned(256))) char smem_dyn8b[];
        smem = smem_dyn8b;
    } else {
        __shared__ __attribute__((aligned(256))) char smem_st8b[2 * TILE_BYTES];
        smem = smem_st8b;
    }
    ScreenUnit u;
    if (!screen_unit_decode(u, 64 * WAVES, B, T, S, n_a, n_q)) return;
    const int p = u.p, split = u.split, a0 = u.a0;
    int qt_begin, qt_end;
    screen_split_tiles(u, S, qt_begin, qt_end);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const unsigned hi_mask = 0u - (unsigned)hi;
    const char *qp = reinterpret_cast<const char *>(q8) + (size_t)p * cap_q * RB;
    const float2 *qs = reinterpret_cast<const float2 *>(q_scale + (size_t)p * (cap_q / 16));

    i32x4 breg[NAB][NKS];
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab) {
        const int arow_i = a0 + wave * 64 + ab * 32 + l31;              // WAVES = 8: the last panel may reach past cap_a (a multiple of 256)
        const char *arow = reinterpret_cast<const char *>(a8) + ((size_t)p * cap_a + (arow_i < cap_a ? arow_i : cap_a - 1)) * RB + 16 * hi;
#pragma unroll
        for (int s = 0; s < NKS; ++s) breg[ab][s] = *reinterpret_cast<const i32x4 *>(arow + 32 * s);
    }
    unsigned dma_off[NI];
    screen_dma_offsets<RB>(dma_off, wave * NI, lane);
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto issue_one = [&](int qt, int buf, int j) {
        const char *qb = qp + (size_t)qt * TILE_BYTES;
        char *dst = smem + buf * TILE_BYTES + (wave_u * NI + j) * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(qb + dma_off[j]),
                                         (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
    };
    unsigned koff[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) koff[c] = (unsigned)(l31 * RB) + ((((unsigned)(hi ^ (l31 & 15))) ^ (2u * c)) << 4);
    auto rd = [&](int s, int qb, unsigned tile) -> i32x4 {
        return *reinterpret_cast<const i32x4 *>(smem + koff[s & 7] + tile + (unsigned)(qb * 32 * RB + (s >> 3) * 256));
    };

    float runmax[NAB], run2[NAB];
    int runidx[NAB];
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab) { runmax[ab] = -INFINITY; run2[ab] = -INFINITY; runidx[ab] = 0; }
    // slice epilogue of one finished 32x32 block: integer maximum of the lane's 16 rows (exact: one exponent per slice), one
    // convert, one multiply, running (best, slice of best, best other slice)
    auto reduce_block = [&](const i32x16 &c, float sc, int sid, int ab) {
        int m0 = max(max(c[0], c[1]), c[2]), m1 = max(max(c[3], c[4]), c[5]), m2 = max(max(c[6], c[7]), c[8]);
        int m3 = max(max(c[9], c[10]), c[11]), m4 = max(max(c[12], c[13]), c[14]);
        int xi = max(max(max(m0, m1), m2), max(max(m3, m4), c[15]));
        const float x = (float)xi * sc;
        const bool improved = x > runmax[ab];
        run2[ab] = fmaxf(fminf(runmax[ab], x), run2[ab]);
        runmax[ab] = fmaxf(runmax[ab], x);
        runidx[ab] = improved ? sid : runidx[ab];
    };
    const i32x16 zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    if (qt_end > qt_begin) {
#pragma unroll
        for (int j = 0; j < NI; ++j) issue_one(qt_begin, 0, j);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    i32x4 areg[NKS];
#pragma unroll
    for (int s = 0; s < NKS; ++s) areg[s] = rd(s, 0, 0u);
    // finished accumulators of the previous query block, reduced under the next block's MFMAs.  The steady-state loop has no branch:
    // before the first block `prev` is a dummy that can never win (score -2^30), and the last tile re-issues its own DMA into the idle
    // buffer instead of testing for "one more tile".
    i32x16 prev[NAB];
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
        for (int r = 0; r < 16; ++r) prev[ab][r] = -(1 << 30);
    float prev_sc = 1.0f;
    int prev_sid = 0;
    int buf = 0;
    for (int qt = qt_begin; qt < qt_end; ++qt) {
        const unsigned tile = buf * TILE_BYTES;
        const int qt_next = qt + 1 < qt_end ? qt + 1 : qt;
        float2 sc2[NQB];
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) sc2[qb] = qs[qt * NQB + qb];
        // ONE A-operand buffer: after both anchor blocks have consumed k-step s of query block qb, areg[s] is re-loaded with k-step s of
        // query block qb+1 (needed 16 MFMAs ~ 500 cycles later)
#pragma unroll
        for (int qb = 0; qb < NQB; ++qb) {
            i32x16 acc[NAB];
            // the whole next tile is requested under the FIRST query block's MFMAs: ~1500 cycles before the wait at the tile's end
            // (spreading the 8 requests over the four blocks left the last ones ~500 cycles, less than an L2 miss: +4 %)
            if (!(VAR & 2) && (((VAR & 8) && qb < 2) || (!(VAR & 8) && qb == 0))) {
#pragma unroll
                for (int j = ((VAR & 8) ? qb * (NI / 2) : 0); j < ((VAR & 8) ? (qb + 1) * (NI / 2) : NI); ++j) issue_one(qt_next, buf ^ 1, j);
            }
#pragma unroll
            for (int s = 0; s < NKS; ++s) {
#pragma unroll
                for (int ab = 0; ab < NAB; ++ab)
                    acc[ab] = __builtin_amdgcn_mfma_i32_32x32x32_i8(areg[s], breg[ab][s], s == 0 ? zero16 : acc[ab], 0, 0, 0);
                if (qb + 1 < NQB) areg[s] = rd(s, qb + 1, tile);
            }
            if (!(VAR & 1)) {
#pragma unroll
                for (int ab = 0; ab < NAB; ++ab) reduce_block(prev[ab], prev_sc, prev_sid, ab);
            } else {
#pragma unroll
                for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
                    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(prev[ab][r]));
            }
            // pin the interleave: per MFMA pair two VALU of the previous block's epilogue and one LDS read of the next A operand
#pragma unroll
            for (int i = 0; i < NKS; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                if (qb + 1 < NQB) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
#pragma unroll
            for (int ab = 0; ab < NAB; ++ab) prev[ab] = acc[ab];
            // lane half hi picks .x / .y with bit masks: written as `hi ? .y : .x` the compiler indexes the float2 array dynamically,
            // moves it to LDS (one 32-byte slot per thread) and reads it back with 8-way bank-conflicting ds_read_b32 - 1.1e8
            // SQ_LDS_BANK_CONFLICT cycles per launch in the round-1 / early round-2 counters
            {
                const unsigned ux = __builtin_bit_cast(unsigned, sc2[qb].x), uy = __builtin_bit_cast(unsigned, sc2[qb].y);
                prev_sc = __builtin_bit_cast(float, (ux & ~hi_mask) | (uy & hi_mask));
            }
            prev_sid = (qt * NQB + qb) * 2 + hi;
        }
        if (!(VAR & 2)) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            buf ^= 1;
        }
        // first A operand of the next tile (its DMA has landed: barrier above)
#pragma unroll
        for (int s = 0; s < NKS; ++s) areg[s] = rd(s, 0, buf * TILE_BYTES);
    }
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab) reduce_block(prev[ab], prev_sc, prev_sid, ab);
    screen_merge_store<NAB>(runmax, run2, runidx, a0 + wave * 64 + l31, hi, (size_t)p * S + split, cap_a, ws_max, ws_i1, ws_m2);
}


// K1s6, the MX-fp6 screen (round 3), lives in screen_mx6.hip (own translation unit: compiled with -fno-honor-nans)

// fp32 rows (k permuted inside groups of 8: position 8g+4h+j holds k = 8g+2j+h) -> fp16 rows in natural k order, the values K0's
// fp16 output would hold.  One lane per group of 8.
__device__ __forceinline__ uint4 half_group_from_permuted(const float4 lo, const float4 hi4)
{
    union { __half h[8]; uint4 u; } pk;
    pk.h[0] = __float2half_rn(lo.x); pk.h[1] = __float2half_rn(hi4.x);
    pk.h[2] = __float2half_rn(lo.y); pk.h[3] = __float2half_rn(hi4.y);
    pk.h[4] = __float2half_rn(lo.z); pk.h[5] = __float2half_rn(hi4.z);
    pk.h[6] = __float2half_rn(lo.w); pk.h[7] = __float2half_rn(hi4.w);
    return pk.u;
}

// query-side fp16 copies for the fp16 pipeline, made only for pairs that have undecided anchors (flag-gated on the device)
__global__ __launch_bounds__(256) void match_make_q16_kernel(const float *__restrict__ q_hat, int Cp, int cap_q,
                                                              const int32_t *__restrict__ n_q, const int32_t *__restrict__ n_amb,
                                                              __half *__restrict__ q16)
{
    const int p = blockIdx.y;
    if (n_amb[p] == 0) return;
    const int n_fill = (n_q[p] + 255) / 256 * 256;
    const size_t groups = (size_t)n_fill * (Cp / 8);
    const float4 *src = reinterpret_cast<const float4 *>(q_hat + (size_t)p * cap_q * Cp);
    uint4 *dst = reinterpret_cast<uint4 *>(q16 + (size_t)p * cap_q * Cp);
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256)
        dst[g] = half_group_from_permuted(src[2 * g], src[2 * g + 1]);
}

// gather the rows of the anchors the int8 stage could not decide into dense panels for the fp16 pipeline (fp32 copy + fp16 copy)
__global__ __launch_bounds__(256) void match_compact8_kernel(const float *__restrict__ a_hat, const __half *__restrict__ a16, int Cp,
                                                              int cap_a, const int32_t *__restrict__ n_amb,
                                                              const int32_t *__restrict__ amb_idx, float *__restrict__ a_hat_c,
                                                              __half *__restrict__ a16_c)
{
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int n_fill = (n_amb[p] + 255) / 256 * 256;               // the fp16 kernels read whole 256-anchor panels: zero-fill the tail
    for (int g = 0; g < 16; ++g) {
    const int sl = (blockIdx.x * 16 + g) * 4 + (threadIdx.x >> 6);
    if (sl >= n_fill) break;
    uint4 *d32 = reinterpret_cast<uint4 *>(a_hat_c + ((size_t)p * cap_a + sl) * Cp);
    uint4 *d16 = reinterpret_cast<uint4 *>(a16_c + ((size_t)p * cap_a + sl) * Cp);
    if (sl >= n_amb[p]) {
        for (int i = lane; i < Cp / 4; i += 64) d32[i] = make_uint4(0, 0, 0, 0);
        for (int i = lane; i < Cp / 8; i += 64) d16[i] = make_uint4(0, 0, 0, 0);
        continue;
    }
    const int a = amb_idx[(size_t)p * cap_a + sl];
    const uint4 *s32 = reinterpret_cast<const uint4 *>(a_hat + ((size_t)p * cap_a + a) * Cp);
    (void)a16;
    for (int i = lane; i < Cp / 4; i += 64) d32[i] = s32[i];
    const float4 *f32 = reinterpret_cast<const float4 *>(s32);
    for (int g = lane; g < Cp / 8; g += 64) d16[g] = half_group_from_permuted(f32[2 * g], f32[2 * g + 1]);
    }
}

__global__ __launch_bounds__(256) void match_scatter8_kernel(int cap_a, const int32_t *__restrict__ n_amb,
                                                              const int32_t *__restrict__ amb_idx, const float *__restrict__ md_c,
                                                              const int32_t *__restrict__ am_c, const uint8_t *__restrict__ va_c,
                                                              float *__restrict__ min_dist, int32_t *__restrict__ argmin,
                                                              uint8_t *__restrict__ valid)
{
    const int p = blockIdx.y, sl = blockIdx.x * 256 + threadIdx.x;
    if (sl >= n_amb[p]) return;
    const size_t src = (size_t)p * cap_a + sl, dst = (size_t)p * cap_a + amb_idx[src];
    min_dist[dst] = md_c[src];
    argmin[dst] = am_c[src];
    valid[dst] = va_c[src];
}

int pick_split16(int B, int T)
{
    int S = (8192 + B * T - 1) / (B * T);
    if (S < 1) S = 1;
    if (S > 16) S = 16;
    return S;
}

static size_t carve_screen(void *base, ScreenWs &w, int B, int C, int cap_a, int S)
{
    Carver carve(base);
    const size_t rows = (size_t)B * cap_a;
    carve(w.ws_max, rows * S);
    carve(w.ws_m2, rows * S);
    carve(w.ws_i1, rows * S);
    carve(w.m_final, rows);
    carve(w.amb_max, rows);
    carve(w.amb_idx, rows);
    carve(w.a16c, rows * C);
    carve(w.cand, rows * SCREEN_CAP);
    w.zero_off = carve.off;
    carve(w.cnt, rows);
    carve(w.row_flag, rows);
    carve(w.panel_flag, (size_t)B * (cap_a / ORYON_MATCH_TILE));
    carve(w.n_amb, (size_t)B);
    w.zero_bytes = carve.off - w.zero_off;
    return carve.off;
}

static size_t carve_screen8(void *base, Screen8Ws &w, int B, int C, int cap_a, int cap_q, int S)
{
    Carver carve(base, carve_screen(base, w, B, C, cap_a, S));
    const size_t rows = (size_t)B * cap_a;
    carve(w.q16, (size_t)B * cap_q * C);
    carve(w.a_hat_c, rows * C);
    carve(w.md_c, rows);
    carve(w.am_c, rows);
    carve(w.va_c, rows);
    ScreenWs inner;                                                 // the nested K1s call carves this region itself
    w.nested_bytes = carve_screen(nullptr, inner, B, C, cap_a, S);
    carve(w.nested, w.nested_bytes);
    return carve.off;
}

size_t carve_screen8_raw(void *base, Screen8RawWs &w, int B, int C, int cap_a, int cap_q, int S)
{
    Carver carve(base, carve_screen8(base, w, B, C, cap_a, cap_q, S));
    carve(w.q_hat, (size_t)B * cap_q * C);
    carve(w.q8_scratch, (size_t)B * cap_q * C);                     // the fall-back pass rewrites the same int8 rows here
    carve(w.scale_scratch, (size_t)B * (cap_q / 16));
    carve(w.eps_scratch, (size_t)B);
    carve(w.need_f32, (size_t)B);
    return carve.off;
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_match_screened_workspace_bytes(int B, int C, int cap_a)
{
    if (B <= 0 || C <= 0 || cap_a <= 0 || cap_a % MT16) return 0;
    ScreenWs w;
    return carve_screen(nullptr, w, B, C, cap_a, pick_split16(B, cap_a / MT16));
}

namespace {
struct Screen16Args {       // the arguments of match_f16_screen_kernel
    const __half *a16, *q16;
    int B, cap_a, cap_q;
    const int32_t *n_a, *n_q;
    int T, S;
    float valid_cut;
    float *ws_max;
    int32_t *cnt, *cand;
    int S_thr;
    const int32_t *row_map;
    int32_t *ws_i1;
    float *ws_m2;
};

// one launcher per descriptor width; C = 512 needs 2 x 64 KB of dynamic LDS (opt-in above 64 KB)
template <int CP, int MODE>
void launch_screen(int groups, hipStream_t st, const Screen16Args &k)
{
    constexpr size_t dyn = 2 * screen_tile_bytes(CP) > 65536 ? 2 * screen_tile_bytes(CP) : 0;
    if (dyn) allow_dynamic_lds(reinterpret_cast<const void *>(&match_f16_screen_kernel<CP, MODE>), (int)dyn);
    hipLaunchKernelGGL((match_f16_screen_kernel<CP, MODE>), dim3(groups), dim3(256), dyn, st, k.a16, k.q16, k.B, k.cap_a, k.cap_q, k.n_a,
                       k.n_q, k.T, k.S, k.valid_cut, k.ws_max, k.cnt, k.cand, k.S_thr, k.row_map, k.ws_i1, k.ws_m2);
}

using Screen16Fn = void (*)(int, hipStream_t, const Screen16Args &);

void launch_screen16(int C, int mode, int groups, hipStream_t st, const Screen16Args &k)
{
    static const Screen16Fn by_width[3][2] = {{launch_screen<128, 1>, launch_screen<128, 2>},
                                              {launch_screen<256, 1>, launch_screen<256, 2>},
                                              {launch_screen<512, 1>, launch_screen<512, 2>}};
    by_width[C == 128 ? 0 : C == 256 ? 1 : 2][mode - 1](groups, st, k);
}
}  // namespace

extern "C" int oryon_match_screened(const float *a_hat, const float *q_hat, const void *a_f16, const void *q_f16, int B, int C,
                                    int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, float *min_dist,
                                    int32_t *argmin, uint8_t *valid, void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(a_hat && q_hat && a_f16 && q_f16 && n_a && n_q && min_dist && argmin && valid);
    ORYON_CHECK_ARG(B >= 0 && (C == 128 || C == 256 || C == 512) && cap_a > 0 && cap_a % MT16 == 0 && cap_q > 0 && cap_q % 256 == 0);
    ORYON_CHECK_ARG(threshold > 0.0f && threshold <= 0.5f);
    if (B == 0) return ORYON_OK;
    const int T = cap_a / MT16;
    const int S = pick_split16(B, T);
    ScreenWs w;
    const size_t need = carve_screen(workspace, w, B, C, cap_a, S);
    ORYON_CHECK_WORKSPACE("oryon_match_screened: ", workspace, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    ORYON_CHECK_HIP(hipMemsetAsync(static_cast<char *>(workspace) + w.zero_off, 0, w.zero_bytes, st));
    // rows whose best fp16 score is below this can never satisfy 0.5*(1-dot) < threshold
    const float valid_cut = (1.0f - 2.0f * threshold) - SCREEN_DELTA - 1e-6f;
    const int groups = ((B * S + 7) / 8) * 8 * T;
    const __half *a16 = static_cast<const __half *>(a_f16), *q16 = static_cast<const __half *>(q_f16);
    Screen16Args all;           // the pass over all anchors
    all.a16 = a16;
    all.q16 = q16;
    all.B = B;
    all.cap_a = cap_a;
    all.cap_q = cap_q;
    all.n_a = n_a;
    all.n_q = n_q;
    all.T = T;
    all.S = S;
    all.valid_cut = valid_cut;
    all.ws_max = w.ws_max;
    all.cnt = w.cnt;
    all.cand = w.cand;
    all.S_thr = S;
    all.row_map = nullptr;
    all.ws_i1 = w.ws_i1;
    all.ws_m2 = w.ws_m2;
    // single screening pass keeping (max, argmax, second max) per anchor; anchors whose runner-up is within MARGIN of the
    // maximum (duplicates, smooth descriptor fields) go through a second, compacted candidate pass
    profile_begin(st, C == 256 ? "match_f16_screen_kernel<256, 2>" : C == 512 ? "match_f16_screen_kernel<512, 2>" : "match_f16_screen_kernel<128, 2>");
    launch_screen16(C, 2, groups, st, all);
    profile_end(st);
    ORYON_CHECK_LAUNCH();
    hipLaunchKernelGGL(C >= 256 ? match_decide_kernel<64> : match_decide_kernel<128>, dim3(cap_a / 64, B), dim3(256), 0, st, a16, q16, C,
                       cap_a, cap_q, n_a, n_q, S, valid_cut, w.ws_max, w.ws_i1, w.ws_m2, w.m_final, w.cnt, w.cand, w.n_amb, w.amb_idx,
                       nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(match_compact_kernel, dim3(cap_a / 64, B), dim3(256), 0, st, a16, C, cap_a, w.n_amb, w.amb_idx, w.m_final,
                       w.a16c, w.amb_max);
    Screen16Args amb = all;     // the candidate pass over the compacted ambiguous anchors
    amb.a16 = w.a16c;
    amb.n_a = w.n_amb;
    amb.ws_max = w.amb_max;
    amb.S_thr = 1;
    amb.row_map = w.amb_idx;
    amb.ws_i1 = nullptr;
    amb.ws_m2 = nullptr;
    launch_screen16(C, 1, groups, st, amb);
    ORYON_CHECK_LAUNCH();
    // 4 lanes per anchor: 16 -> 394 us, 8 -> 230, 4 -> 184, 2 -> 175, 1 -> 200 us at cfg2 (almost every anchor has one candidate)
    hipLaunchKernelGGL((match_rescore_kernel<4>), dim3(cap_a / 64, B), dim3(256), 0, st, a_hat, q_hat, C, cap_a, cap_q, n_a, n_q, S,
                       threshold, valid_cut, w.ws_max, w.m_final, w.cnt, w.cand, min_dist, argmin, valid, w.row_flag, w.panel_flag);
    ORYON_CHECK_LAUNCH();
    // exact recomputation of the (rare) panels whose candidate lists overflowed; exits immediately elsewhere
    return match_f32_flagged(a_hat, q_hat, B, C, cap_a, cap_q, n_a, n_q, threshold, min_dist, argmin, valid, w.panel_flag,
                             w.row_flag, stream);
}


// ------------------------------------------------------------------------------------------------ K1s8: host steps and entry points
namespace {
// the kernel launch_screen8<CP> dispatches under the current development switches (for oryon_dominant_kernel)
const char *screen8_name(int CP)
{
    const int variant = dev_env_int("ORYON_SCREEN8_VARIANT", 2);
    const int ablate = dev_env_int("ORYON_SCREEN8_ABLATE", 0);
    const int waves = dev_env_int("ORYON_SCREEN8_WAVES", 8);
    if (variant == 1) return CP == 256 ? "match_i8_screen_kernel<256>" : "match_i8_screen_kernel<512>";
    if (ablate && CP == 256) return "match_i8_screen_v2_kernel<256, ABLATED> (timing ablation: results are wrong)";
    if (waves == 8 && CP == 256) return "match_i8_screen_v2_kernel<256, 0, 8>";
    return CP == 256 ? "match_i8_screen_v2_kernel<256, 0, 4>" : "match_i8_screen_v2_kernel<512, 0, 4>";
}

template <int CP>
void launch_screen8(int groups, hipStream_t st, const int8_t *a8, const int8_t *q8, const float *q_scale, int B, int cap_a, int cap_q,
                    const int32_t *n_a, const int32_t *n_q, int T, int S, float *ws_max, int32_t *ws_i1, float *ws_m2)
{
    constexpr size_t dyn = 2 * screen8_tile_bytes(CP) > 65536 ? 2 * screen8_tile_bytes(CP) : 0;
    auto launch = [&](auto kernel, int grid, int block, size_t lds, int tiles) {
        if (lds) allow_dynamic_lds(reinterpret_cast<const void *>(kernel), (int)lds);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, st, a8, q8, q_scale, B, cap_a, cap_q, n_a, n_q, tiles, S, ws_max, ws_i1,
                           ws_m2);
    };
    static const int variant = dev_env_int("ORYON_SCREEN8_VARIANT", 2);
    if (variant == 1) return launch(match_i8_screen_kernel<CP>, groups, 256, dyn, T);                 // round-1 loop (kept for A/B timing)
    static const int ablate = dev_env_int("ORYON_SCREEN8_ABLATE", 0);
    if (ablate && CP == 256) {
        switch (ablate) {
        case 1: return launch(match_i8_screen_v2_kernel<256, 1>, groups, 256, 0, T);
        case 2: return launch(match_i8_screen_v2_kernel<256, 2>, groups, 256, 0, T);
        case 3: return launch(match_i8_screen_v2_kernel<256, 3>, groups, 256, 0, T);
        default: return launch(match_i8_screen_v2_kernel<256, 8>, groups, 256, 0, T);
        }
    }
    static const int waves = dev_env_int("ORYON_SCREEN8_WAVES", 8);
    if (waves == 8 && CP == 256) {
        const int T8 = (cap_a + 511) / 512;
        return launch(match_i8_screen_v2_kernel<256, 0, 8>, groups / T * T8, 512, 0, T8);
    }
    launch(match_i8_screen_v2_kernel<CP>, groups, 256, dyn, T);
}
}  // namespace

namespace oryon {
void screen8_step(const Screen8Args &m, int S, const int32_t *n_a, const ScreenWs &w)
{
    hipStream_t st = as_stream(m.stream);
    const int T = m.cap_a / MT16, groups = ((m.B * S + 7) / 8) * 8 * T;
    profile_begin(st, screen8_name(m.C));
    (m.C == 256 ? launch_screen8<256> : launch_screen8<512>)(groups, st, m.a_i8, m.q_i8, m.q_scale, m.B, m.cap_a, m.cap_q, n_a, m.n_q, T, S,
                                                             w.ws_max, w.ws_i1, w.ws_m2);
    profile_end(st);
}

void decide8_step(const Screen8Args &m, int S, const int32_t *n_a, const ScreenWs &w)
{
    const float cut0 = 1.0f - 2.0f * m.threshold;
    const float valid_cut16 = cut0 - SCREEN_DELTA - 1e-6f;
    hipLaunchKernelGGL((match_decide_kernel<128>), dim3(m.cap_a / 64, m.B), dim3(256), 0, as_stream(m.stream),
                       static_cast<const __half *>(nullptr), static_cast<const __half *>(nullptr), m.C, m.cap_a, m.cap_q, n_a, m.n_q, S,
                       valid_cut16, w.ws_max, w.ws_i1, w.ws_m2, w.m_final, w.cnt, w.cand, w.n_amb, w.amb_idx, m.a_scale, nullptr, m.q_eps_max,
                       cut0, sqrtf((float)m.C_true), (float)m.C_true, m.a_i8, m.q_i8, m.q_scale);
}

void rescore_raw_step(const Screen8Args &m, const int32_t *n_a, int rescore_lanes, const Screen8RawWs &w)
{
    const bool nhwc = m.layout == ORYON_LAYOUT_NHWC;
    const int lanes = (rescore_lanes == 1 || rescore_lanes == 4) ? rescore_lanes : 2;
    auto rescore = lanes == 1   ? (nhwc ? match_rescore_raw_kernel<1, true> : match_rescore_raw_kernel<1, false>)
                   : lanes == 4 ? (nhwc ? match_rescore_raw_kernel<4, true> : match_rescore_raw_kernel<4, false>)
                                : (nhwc ? match_rescore_raw_kernel<2, true> : match_rescore_raw_kernel<2, false>);
    hipLaunchKernelGGL(rescore, dim3(m.cap_a / (256 / lanes), m.B), dim3(256), 0, as_stream(m.stream), m.a_hat, m.feat_q, m.C_true, m.HW,
                       m.roi_q, m.roi_stride_q, m.q_norm, m.C, m.cap_a, m.cap_q, n_a, m.n_q, m.threshold, w.m_final, w.cnt, w.cand,
                       m.min_dist, m.argmin, m.valid, w.row_flag, w.panel_flag, w.need_f32, m.round_f16);
}

int screen16_fallback(const Screen8Args &m, const float *q_hat, const Screen8Ws &w, const char *who)
{
    hipStream_t st = as_stream(m.stream);
    hipLaunchKernelGGL(match_compact8_kernel, dim3(m.cap_a / 64, m.B), dim3(256), 0, st, m.a_hat, static_cast<const __half *>(nullptr), m.C,
                       m.cap_a, w.n_amb, w.amb_idx, w.a_hat_c, w.a16c);
    hipLaunchKernelGGL(match_make_q16_kernel, dim3(64, m.B), dim3(256), 0, st, q_hat, m.C, m.cap_q, m.n_q, w.n_amb, w.q16);
    int rc = check_launch(who);
    if (rc) return rc;
    rc = oryon_match_screened(w.a_hat_c, q_hat, w.a16c, w.q16, m.B, m.C, m.cap_a, m.cap_q, w.n_amb, m.n_q, m.threshold, w.md_c,
                              w.am_c, w.va_c, w.nested, w.nested_bytes, m.stream);
    if (rc) return rc;
    hipLaunchKernelGGL(match_scatter8_kernel, dim3(m.cap_a / 256, m.B), dim3(256), 0, st, m.cap_a, w.n_amb, w.amb_idx, w.md_c, w.am_c,
                       w.va_c, m.min_dist, m.argmin, m.valid);
    return check_launch(who);
}

// Both rare, both gated per pair on the device: pairs with undecided anchors or an overflowed candidate list get their canonical fp32
// query rows materialised now - the price round 1 paid for EVERY pair - and then take the round-1 route.
int raw_fallbacks(const Screen8Args &m, const int32_t *n_a, const Screen8RawWs &w, const char *who, const char *entry)
{
    hipStream_t st = as_stream(m.stream);
    hipLaunchKernelGGL(match_need_f32_kernel, dim3((m.B + 255) / 256), dim3(256), 0, st, m.B, w.n_amb, w.need_f32);
    int rc = gather_q8_launch(m.feat_q, m.B, m.C_true, m.HW, m.layout, m.roi_q, m.roi_stride_q, m.n_q, w.need_f32, m.cap_q, m.C, w.q8_scratch,
                              w.scale_scratch, w.eps_scratch, nullptr, w.q_hat, 1, m.round_f16, st);
    if (rc) { set_error("%s: fall-back gather launch failed", entry); return rc; }
    rc = match_f32_flagged(m.a_hat, w.q_hat, m.B, m.C, m.cap_a, m.cap_q, n_a, m.n_q, m.threshold, m.min_dist, m.argmin, m.valid, w.panel_flag,
                           w.row_flag, m.stream);
    if (rc) return rc;
    return screen16_fallback(m, w.q_hat, w, who);
}
}  // namespace oryon

extern "C" size_t oryon_match_screened8_workspace_bytes(int B, int C, int cap_a, int cap_q)
{
    if (B <= 0 || C <= 0 || cap_a <= 0 || cap_a % MT16 || cap_q <= 0) return 0;
    Screen8Ws w;
    return carve_screen8(nullptr, w, B, C, cap_a, cap_q, pick_split16(B, cap_a / MT16));
}

extern "C" int oryon_match_screened8(const float *a_hat, const float *q_hat, const int8_t *a_i8, const int8_t *q_i8, const float *a_scale, const float *q_scale, const float *q_eps_max, int B,
                                     int C_true, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold,
                                     float *min_dist, int32_t *argmin, uint8_t *valid, int32_t *n_undecided, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(a_hat && q_hat && a_i8 && q_i8 && a_scale && q_scale && q_eps_max && n_a && n_q);
    ORYON_CHECK_ARG(min_dist && argmin && valid && B >= 0 && (C == 256 || C == 512) && C_true > 0 && C_true <= C);
    ORYON_CHECK_ARG(cap_a > 0 && cap_a % MT16 == 0 && cap_q > 0 && cap_q % 256 == 0 && threshold > 0.0f && threshold <= 0.5f);
    if (B == 0) return ORYON_OK;
    const int S = pick_split16(B, cap_a / MT16);
    Screen8Ws w;
    const size_t need = carve_screen8(workspace, w, B, C, cap_a, cap_q, S);
    ORYON_CHECK_WORKSPACE("oryon_match_screened8: ", workspace, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    Screen8Args m;                 // the query rows are fp32 rows here (q_hat): no raw map
    m.a_hat = a_hat;
    m.a_i8 = a_i8;
    m.q_i8 = q_i8;
    m.a_scale = a_scale;
    m.q_scale = q_scale;
    m.q_eps_max = q_eps_max;
    m.B = B;
    m.C_true = C_true;
    m.C = C;
    m.cap_a = cap_a;
    m.cap_q = cap_q;
    m.n_q = n_q;
    m.threshold = threshold;
    m.min_dist = min_dist;
    m.argmin = argmin;
    m.valid = valid;
    m.stream = stream;
    ORYON_CHECK_HIP(hipMemsetAsync(static_cast<char *>(workspace) + w.zero_off, 0, w.zero_bytes, st));
    screen8_step(m, S, n_a, w);
    ORYON_CHECK_LAUNCH();
    decide8_step(m, S, n_a, w);
    ORYON_CHECK_LAUNCH();
    hipLaunchKernelGGL((match_rescore_kernel<4>), dim3(cap_a / 64, B), dim3(256), 0, st, a_hat, q_hat, C, cap_a, cap_q, n_a, n_q, S,
                       threshold, -INFINITY, w.ws_max, w.m_final, w.cnt, w.cand, min_dist, argmin, valid, w.row_flag, w.panel_flag);
    ORYON_CHECK_LAUNCH();
    int rc = match_f32_flagged(a_hat, q_hat, B, C, cap_a, cap_q, n_a, n_q, threshold, min_dist, argmin, valid, w.panel_flag, w.row_flag,
                               stream);
    if (rc) return rc;
    if (n_undecided) ORYON_CHECK_HIP(hipMemcpyAsync(n_undecided, w.n_amb, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return screen16_fallback(m, q_hat, w, __func__);
}

// ------------------------------------------------------------------------------------------------ K1s8 on K0v3 operands (no fp32 query rows)
extern "C" size_t oryon_match_screened8_raw_workspace_bytes(int B, int C, int cap_a, int cap_q)
{
    if (B <= 0 || C <= 0 || cap_a <= 0 || cap_a % MT16 || cap_q <= 0) return 0;
    Screen8RawWs w;
    return carve_screen8_raw(nullptr, w, B, C, cap_a, cap_q, pick_split16(B, cap_a / MT16));
}

extern "C" int oryon_match_screened8_raw(const float *a_hat, const int8_t *a_i8, const float *a_scale, const float *feat_q, int C_true,
                                         int HW, int layout, const int32_t *roi_q, int roi_stride, const float *q_norm,
                                         const int8_t *q_i8, const float *q_scale, const float *q_eps_max, int B, int C, int cap_a,
                                         int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, float *min_dist,
                                         int32_t *argmin, uint8_t *valid, int32_t *n_undecided, int round_f16, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(a_hat && a_i8 && a_scale && feat_q && roi_q && q_norm && q_i8 && q_scale && q_eps_max && n_a && n_q);
    ORYON_CHECK_ARG(min_dist && argmin && valid && B >= 0 && (C == 256 || C == 512) && C_true > 0 && C_true <= C && HW > 0);
    ORYON_CHECK_ARG(layout == ORYON_LAYOUT_NCHW || layout == ORYON_LAYOUT_NHWC);
    ORYON_CHECK_ARG(cap_a > 0 && cap_a % MT16 == 0 && cap_q > 0 && cap_q % 256 == 0 && threshold > 0.0f && threshold <= 0.5f);
    if (B == 0) return ORYON_OK;
    const int S = pick_split16(B, cap_a / MT16);
    Screen8RawWs w;
    const size_t need = carve_screen8_raw(workspace, w, B, C, cap_a, cap_q, S);
    ORYON_CHECK_WORKSPACE("oryon_match_screened8_raw: ", workspace, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    Screen8Args m;
    m.a_hat = a_hat;
    m.a_i8 = a_i8;
    m.q_i8 = q_i8;
    m.a_scale = a_scale;
    m.q_scale = q_scale;
    m.q_eps_max = q_eps_max;
    m.B = B;
    m.C_true = C_true;
    m.C = C;
    m.cap_a = cap_a;
    m.cap_q = cap_q;
    m.n_q = n_q;
    m.threshold = threshold;
    m.feat_q = feat_q;
    m.HW = HW;
    m.layout = layout;
    m.roi_q = roi_q;
    m.roi_stride_q = roi_stride;
    m.q_norm = q_norm;
    m.round_f16 = round_f16;
    m.min_dist = min_dist;
    m.argmin = argmin;
    m.valid = valid;
    m.stream = stream;
    ORYON_CHECK_HIP(hipMemsetAsync(static_cast<char *>(workspace) + w.zero_off, 0, w.zero_bytes, st));
    ORYON_CHECK_HIP(hipMemsetAsync(w.need_f32, 0, (size_t)B * sizeof(int32_t), st));
    screen8_step(m, S, n_a, w);
    ORYON_CHECK_LAUNCH();
    decide8_step(m, S, n_a, w);
    ORYON_CHECK_LAUNCH();
    static const int resc_l = dev_env_int("ORYON_RESCORE_LANES", 2);
    rescore_raw_step(m, n_a, resc_l, w);
    ORYON_CHECK_LAUNCH();
    if (n_undecided) ORYON_CHECK_HIP(hipMemcpyAsync(n_undecided, w.n_amb, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return raw_fallbacks(m, n_a, w, __func__, __func__);
}
