// The decision side of the matcher, one definition each: what turns the low-precision screens' (m1, slice, m2) triples into results that
// equal the exact fp32 scan bit for bit - the k-permuted row FORMAT, the SLICE geometry and its re-score, the merge of per-split
// TRIPLES, the screen BOUNDS and the canonical CHAIN.  Used by match16.hip, match_corrs.hip and match_x3.hip; K0's write sites
// (gather8.hip, roi.hip) take the format's index from here.  A change to a constant of a bound, to the tie rule or to the row format is
// made HERE.  The producer side (the screens' tile loop) is screen_tile.h.  Inline device code only.  Not for screen_mx6.hip, which is
// compiled without NaN semantics: the fmaxf / fminf below rely on them.
#pragma once
#include <hip/hip_fp16.h>
#include "common.h"
#include "x3.h"

namespace oryon {

// ------------------------------------------------------------------------------------------------ format: k-permuted fp32 rows
// K0's fp32 unit rows (and every compacted copy) are permuted inside groups of 8 channels: position 8g + 4h + j holds channel
// k = 8g + 2j + h, i.e. the first float4 of a group holds k = 8g + {0,2,4,6}, the second k = 8g + {1,3,5,7} (the operand order of K1's
// fp32 MFMA).  Constant arguments fold at compile time.
__host__ __device__ constexpr int kperm_k(int g, int hh, int jj) { return 8 * g + 2 * jj + hh; }
// the two float4 of one permuted group -> its eight values in natural k order
__device__ __forceinline__ void kperm_group_natural(const float4 a0, const float4 a1, float (&v)[8])
{
    v[kperm_k(0, 0, 0)] = a0.x; v[kperm_k(0, 0, 1)] = a0.y; v[kperm_k(0, 0, 2)] = a0.z; v[kperm_k(0, 0, 3)] = a0.w;
    v[kperm_k(0, 1, 0)] = a1.x; v[kperm_k(0, 1, 1)] = a1.y; v[kperm_k(0, 1, 2)] = a1.z; v[kperm_k(0, 1, 3)] = a1.w;
}
// one wave: a permuted row -> natural order in LDS (A [Cp])
__device__ __forceinline__ void wave_unpermute_row(float *A, const float *__restrict__ row, int Cp)
{
    for (int pos = threadIdx.x & 63; pos < Cp; pos += 64) A[kperm_k(pos >> 3, (pos >> 2) & 1, pos & 3)] = row[pos];
}

// ------------------------------------------------------------------------------------------------ slices
// The screens report the winner as a SLICE: sid = 2 * (32-row query block) + lane half, the 16 query rows one accumulator column of a
// 32x32 MFMA block holds in one lane (x3.h: crow) - the geometry of the screens' output, not of any one kernel's accumulator map.
__device__ __forceinline__ int slice_row(int sid, int r) { return (sid >> 1) * 32 + crow(r, sid & 1); }
// K0's int8 rows carry one power-of-two scale 2^-E per such slice of the ANCHOR rows too: slot of anchor row a in [cap_a / 16]
__device__ __forceinline__ int anchor_scale_slot(int a) { return (a >> 5) * 2 + ((a >> 2) & 1); }
// Re-score of a slice by one wave: 16 rows x 4 lanes, lane = 4 r + seg, row q = slice_row(sid, r) of q_rows [cap_q, Cp], seg a quarter
// of K; the partial sums meet over xor 1, 2 (all four lanes of a row hold the sum).  live = q < n_q.  Hit thresholds stay with the callers.
// int8 rows: the very integers the screening pass accumulated, so the slice maximum reproduces m1 exactly
__device__ __forceinline__ int slice_score_i8(const int8_t *__restrict__ a_row, const int8_t *__restrict__ q_rows, int q, int Cp, bool live)
{
    const int seg = threadIdx.x & 3;
    int idot = 0;
    if (live) {
        const uint4 *ar = reinterpret_cast<const uint4 *>(a_row) + seg * (Cp / 64);
        const uint4 *qr = reinterpret_cast<const uint4 *>(q_rows + (size_t)q * Cp) + seg * (Cp / 64);
        for (int i0 = 0; i0 < Cp / 64; ++i0) {
            const uint4 av = ar[i0], qv = qr[i0];
            const int *ai = reinterpret_cast<const int *>(&av), *qi = reinterpret_cast<const int *>(&qv);
#pragma unroll
            for (int e = 0; e < 4; ++e) idot = __builtin_amdgcn_sdot4(ai[e], qi[e], idot, false);
        }
    }
    idot += __shfl_xor(idot, 1);
    return idot + __shfl_xor(idot, 2);
}
// fp16 rows, fp32 accumulate (Cp a multiple of 128: four 16-byte loads in flight per operand)
__device__ __forceinline__ float slice_score_f16(const __half *__restrict__ a_row, const __half *__restrict__ q_rows, int q, int Cp, bool live)
{
    const int seg = threadIdx.x & 3;
    float sdot = 0.0f;
    if (live) {
        const uint4 *ar = reinterpret_cast<const uint4 *>(a_row) + seg * (Cp / 32);
        const uint4 *qr = reinterpret_cast<const uint4 *>(q_rows + (size_t)q * Cp) + seg * (Cp / 32);
        for (int i0 = 0; i0 < Cp / 32; i0 += 4) {
            uint4 av[4], qv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { av[u] = ar[i0 + u]; qv[u] = qr[i0 + u]; }
            const __half2 *ah = reinterpret_cast<const __half2 *>(av), *qh = reinterpret_cast<const __half2 *>(qv);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float2 x = __half22float2(ah[e]), y = __half22float2(qh[e]);
                sdot = fmaf(x.x, y.x, sdot);
                sdot = fmaf(x.y, y.y, sdot);
            }
        }
    }
    sdot += __shfl_xor(sdot, 1);
    return sdot + __shfl_xor(sdot, 2);
}
typedef float f32x32r __attribute__((ext_vector_type(32)));
typedef unsigned u32x6r __attribute__((ext_vector_type(6)));
// dequantised dot product of two mx6 slots (32 channels): codes decoded by the conversion instruction (exact: multiples of 1/8 up to
// 7.5), 32 exact products summed in fp32 (every partial sum is a multiple of 1/64 below 2^11: exact), times both block exponents
__device__ __forceinline__ float mx6_block_dot(const uint4 a_lo, const uint4 a_up, const uint4 q_lo, const uint4 q_up)
{
    const u32x6r ca = {a_lo.x, a_lo.y, a_lo.z, a_lo.w, a_up.x, a_up.y}, cq = {q_lo.x, q_lo.y, q_lo.z, q_lo.w, q_up.x, q_up.y};
    const f32x32r fa = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(ca, 1.0f), fq = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(cq, 1.0f);
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) sum = __fmaf_rn(fa[i], fq[i], sum);
    return sum * ldexpf(1.0f, (int)(a_up.z & 255u) + (int)(q_up.z & 255u) - 254);
}
// mx6 rows: the very operands the screen multiplied (software sum: another order of additions than the MFMA's, inside the bound's slack)
__device__ __forceinline__ float slice_score_mx6(const int8_t *__restrict__ a_row, const int8_t *__restrict__ q_rows, int q, int Cp, bool live)
{
    const int seg = threadIdx.x & 3;
    float s6 = 0.0f;
    if (live) {
        const uint4 *ar = reinterpret_cast<const uint4 *>(a_row) + seg * (Cp / 64);
        const uint4 *qr = reinterpret_cast<const uint4 *>(q_rows + (size_t)q * Cp) + seg * (Cp / 64);
        for (int b = 0; b < Cp / 128; ++b) s6 += mx6_block_dot(ar[2 * b], ar[2 * b + 1], qr[2 * b], qr[2 * b + 1]);
    }
    s6 += __shfl_xor(s6, 1);
    return s6 + __shfl_xor(s6, 2);
}

// ------------------------------------------------------------------------------------------------ triples
// Merge of one row's per-split (m1, slice of m1, m2) triples; element (split s, row) at (p S + s) cap + row.  m2: the best score outside
// m1's slice as far as the splits know.  Ties go to the lowest split, i.e. the lowest slice, however the tiles were dealt to the splits.
__device__ __forceinline__ void merge_split_triples(const float *__restrict__ ws_m1, const int32_t *__restrict__ ws_i1,
                                                    const float *__restrict__ ws_m2, int p, int S, int cap, int row, float &m1, int &sid, float &m2)
{
    m1 = m2 = -INFINITY;
    int s_best = -1;
    // (the slice id is fetched once, from the split that won: the 2 S loads of the loop do not depend on one another)
#pragma unroll 4
    for (int s = 0; s < S; ++s) {
        const size_t o = ((size_t)p * S + s) * cap + row;
        const float x1 = ws_m1[o], x2 = ws_m2[o];
        m2 = fmaxf(fminf(m1, x1), fmaxf(m2, x2));
        if (x1 > m1) { m1 = x1; s_best = s; }
    }
    sid = s_best >= 0 ? ws_i1[((size_t)p * S + s_best) * cap + row] : 0;
}

// ------------------------------------------------------------------------------------------------ bounds
// |screen score - a^.q^| <= delta for every (anchor, query) of the row.  With cut0 = 1 - 2 thr, the score at the distance threshold:
// m1 < cut0 - delta cannot be valid, m1 > cut0 + delta is valid for sure (whatever the argmin), m1 - m2 > 2 delta has every exact
// minimiser in m1's slice - each with a little slack for the roundings of the comparison itself.  A bound of 0.2 or more (degenerate
// scales) decides nothing: !usable(), margin() = +inf leaves the argmin to the next stage; the lines mean something under usable() only.
struct ScreenBound {
    float delta;
    __device__ __forceinline__ bool usable() const { return delta < 0.2f; }
    __device__ __forceinline__ float margin() const { return usable() ? 2.0f * delta + 2e-7f : INFINITY; }
    __device__ __forceinline__ float cannot_line(float cut0) const { return cut0 - delta - 1e-6f; }      // not m1 >= this: cannot be valid
    __device__ __forceinline__ float sure_line(float cut0) const { return cut0 + delta + 1e-5f; }        // m1 > this: valid for sure
    // a PARTIAL scan's maximum (the cascades' windows and bands) above this settles the row: the complete m1 >= it passes sure_line too
    __device__ __forceinline__ float settled_line(float cut0) const { return cut0 + delta + 2e-5f; }
};
// MX-fp6 screen: scores are dequantised dot products; ea / eq are the pair's largest measured row error |e|_2 of the anchor / query rows
// (K0, FMT = 1): |s6 - a^.q^| <= |ea| + |eq| + |ea||eq| + fp32 accumulation of <= 512 products in the MFMA and in the chain (<= 7e-5)
__device__ __forceinline__ ScreenBound mx6_bound(float ea, float eq) { return {ea + eq + ea * eq + 1.2e-4f}; }
// int8 screen: sa = 2^-E of the anchor's slice (the caller scales m1, m2 by it: exact, a power of two), eps_q the pair's largest query
// 2^-(E+1).  K0's rounding: |q 2^-E - x^| <= 2^-(E+1) * (1 + 4.6e-5)  (gather8.hip: q = rint(x * RN(2^E / d))), so
// |s8 - a^.q^| <= ea*|q^|_1 + eq*|a^|_1 + C*ea*eq <= (ea + eq)*sqrt(C) + C*ea*eq  (unit rows: |x|_1 <= sqrt(C)) + the exact scan's fp32 slack
__device__ __forceinline__ ScreenBound i8_bound(float sa, float eps_q, float sqrt_c, float c_true)
{
    const float ea = 0.50003f * sa, eq = 1.00006f * eps_q;
    return {(ea + eq) * sqrt_c + c_true * ea * eq + 4e-5f};
}

// ------------------------------------------------------------------------------------------------ the canonical chain
// The exact scan's distance of (anchor, query): unit values u_k = x_k / d (IEEE division of the raw map's value, rounded to float16 first
// under round_f16 and zero beyond C_true, by the row norm K0 stored), ONE fp32 fma chain over k = 0, 1, 2, .., distance 0.5 - 0.5 dot in one
// fma, minimum by lex_min's first-index rule (match_common.h).  Where K0 wrote no fp32 row a consumer forms the values: the same bits.
__device__ __forceinline__ float unit_value(float x, float d, int round_f16) { return __fdiv_rn(round_f16 ? __half2float(__float2half_rn(x)) : x, d); }
// channel k of the row at pixel pix of one map ([C_true, HW], or channels-last)
template <bool NHWC>
__device__ __forceinline__ float raw_unit(const float *__restrict__ map, int pix, float d, int k, int C_true, int HW, int round_f16)
{
    const float x = k >= C_true ? 0.0f : NHWC ? map[(size_t)pix * C_true + k] : map[(size_t)k * HW + pix];
    return unit_value(x, d, round_f16);
}
// eight steps of the chain: one permuted group of an anchor row against eight natural-order query values
__device__ __forceinline__ float chain_step8(const float4 a0, const float4 a1, const float (&x)[8], float dot)
{
    float a[8];
    kperm_group_natural(a0, a1, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = __fmaf_rn(a[e], x[e], dot);
    return dot;
}
__device__ __forceinline__ float dist_from_dot(float dot) { return __fmaf_rn(-0.5f, dot, 0.5f); }

// One wave, one candidate: the query row (pixel pix of map fq, norm dq) formed into Q [Cp], then the chain against the anchor row A [Cp]
// (both LDS, natural order, broadcast reads) in every lane; -> the distance.  The fences order Q's reuse from one candidate to the next.
template <bool NHWC>
__device__ __forceinline__ float wave_exact_dist(const float *A, float *Q, const float *__restrict__ fq, int pix, float dq, int Cp, int C_true,
                                                 int HW, int round_f16)
{
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int k = threadIdx.x & 63; k < Cp; k += 64) Q[k] = raw_unit<NHWC>(fq, pix, dq, k, C_true, HW, round_f16);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float dot = 0.0f;
    for (int k = 0; k < C_true; k += 8) {
        float av[8], qv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { av[e] = A[k + e]; qv[e] = Q[k + e]; }
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (k + e < C_true) dot = __fmaf_rn(av[e], qv[e], dot);
    }
    return dist_from_dot(dot);
}

}  // namespace oryon
