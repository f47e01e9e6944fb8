// K1r: the ratio test with an exclusion disc.  For every anchor row i the best query row OUTSIDE a disc of `radius` pixels around the
// pixel of its nearest query row argmin[i] (K1's or K1m's output), and keep[i] = gate[i] && min_dist[i] <= ratio * second_dist[i]
// (include/oryon_hip.h has the definition).  radius 1 excludes the best pixel alone: Lowe's ratio test.
//
// The second minimum depends on each anchor's own argmin, so it is a second all-pairs scan: K1's two tile walks (match_tile.h) with a
// masked fold.
//   * a lane owns one anchor column (the C/D layout of the 32x32x2 MFMA); it keeps that anchor's (y*, x*) and its running
//     (second, index) in registers;
//   * the packed pixels (y << 16 | x) of a tile's query rows are staged in LDS with the tile: fetched when the tile's loads are issued,
//     stored in front of the barrier that publishes the tile, double buffered by tile parity.  All lanes of a half-wave hold the same
//     query rows, so the fold's reads of them are broadcasts (four consecutive rows per ds_read_b128);
//   * K1's skip stands in front of the mask: the tile's largest dot product decides whether ANY lane of the wave can improve its running
//     second; only then is the tile walked, four query rows at a time: the unmasked `d < second` for the whole wave first, the four
//     pixels and the integer test only when some lane passes.  Once the running second has settled only the rows inside an anchor's
//     own disc (at most ~pi r^2, those nearer than the second) pass the first test again;
//   * unused query rows are masked by index (K0 zero-fills only to the next multiple of 256); anchor columns >= n_a compute garbage in
//     their own lane and are not written;
//   * query splits merge as K1's do, by (distance, index); keep is written by whichever launch finishes a row: the scan when S == 1,
//     the merge otherwise.
#include "common.h"
#include "match_common.h"
#include "match_tile.h"
#include "match_disc.h"

namespace oryon {

__device__ __forceinline__ uint8_t ratio_keep(const uint8_t *__restrict__ gate, size_t o, float md, float ratio, float second)
{
    return ((!gate || gate[o]) && md <= __fmul_rn(ratio, second)) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ C_pad 32 / 64 / 128 / 256
template <int CP> struct SecondFoldRegb : PixelStage<RegbGeom<CP>::ROWS> {
    static constexpr int ROWS = RegbGeom<CP>::ROWS, NACC = RegbGeom<CP>::NACC;
    int ys, xs, r;
    float second = INFINITY;
    int sidx = 0x7fffffff;
    __device__ __forceinline__ void tile(f32x16 (&acc)[NACC], int qt)
    {
        const int hi = (threadIdx.x & 63) >> 5;
        const int qlane = qt * ROWS + 4 * hi;
        const bool full = (qt + 1) * ROWS <= this->nq;
        float mx = acc[0][0];
#pragma unroll
        for (int m = 0; m < NACC; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) mx = fmaxf(mx, acc[m][e]);
        const bool improves = __fmaf_rn(-0.5f, mx, 0.5f) < second;      // unmasked: a row inside the disc may raise a false alarm
        if (!full || __any(improves)) {
            const unsigned *px = this->rows(qt) + 4 * hi;
#pragma unroll
            for (int m = 0; m < NACC; ++m)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    // four consecutive query rows: the unmasked test first, for the whole wave; their pixels are read and the integer
                    // test made only when some lane passes it
                    const int q0 = qlane + m * 32 + 8 * r4;
                    float d[4];
                    bool pass = false;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        d[e] = __fmaf_rn(-0.5f, acc[m][4 * r4 + e], 0.5f);
                        if (!full) d[e] = (q0 + e < this->nq) ? d[e] : INFINITY;
                        pass = pass || d[e] < second;
                    }
                    if (!__any(pass)) continue;
                    // accumulator registers 4 r4 .. 4 r4 + 3 hold rows 4 hi + 8 r4 + 0 .. 3 of block m
                    const uint4 pk4 = *reinterpret_cast<const uint4 *>(px + m * 32 + 8 * r4);
                    const unsigned pk[4] = {pk4.x, pk4.y, pk4.z, pk4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool better = d[e] < second && outside_disc(pk[e], ys, xs, r);   // strict: first (smallest) candidate index wins ties
                        second = better ? d[e] : second;
                        sidx = better ? q0 + e : sidx;
                    }
                }
        }
#pragma unroll
        for (int m = 0; m < NACC; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][e] = 0.0f;
    }
};

template <int CP>
__global__ __launch_bounds__(MATCH_THREADS, 2) void match_second_regb_kernel(
    const float *__restrict__ a_hat, const float *__restrict__ q_hat, int B, int cap_a, int cap_q, const int32_t *__restrict__ n_a,
    const int32_t *__restrict__ n_q, const int32_t *__restrict__ roi_q, int roi_stride_q, int W_q, int radius,
    const float *__restrict__ min_dist, const int32_t *__restrict__ argmin, const uint8_t *__restrict__ gate, float ratio, int T, int S,
    float *__restrict__ second_dist, int32_t *__restrict__ second_argmin, uint8_t *__restrict__ keep, float *__restrict__ ws_dist,
    int32_t *__restrict__ ws_idx)
{
    constexpr int ROWS = RegbGeom<CP>::ROWS;
    __shared__ __attribute__((aligned(256))) char smem[2 * RegbGeom<CP>::TILE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned pix[2 * ROWS];

    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int unit = (slot / T) * 8 + xcd;              // (pair, split) unit; all T panels of a unit share an XCD
    if (unit >= B * S) return;
    const int panel = slot % T;
    const int p = unit / S, split = unit % S;
    const int na = n_a[p], nq = n_q[p];
    const int a0 = panel * MT;
    if (a0 >= na) return;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int a = a0 + wave * 32 + l31;                 // this lane's anchor row
    const int32_t *roi = roi_q + (size_t)p * roi_stride_q;
    SecondFoldRegb<CP> fold;
    fold.pix = pix;
    fold.roi = roi;
    fold.nq = nq;
    fold.W = W_q;
    fold.r = radius;
    star_pixel(argmin + (size_t)p * cap_a, roi, a, na, nq, W_q, fold.ys, fold.xs);
    match_regb_walk<CP>(smem, a_hat + ((size_t)p * cap_a + a) * CP + 4 * hi, reinterpret_cast<const char *>(q_hat + (size_t)p * cap_q * CP),
                        split_span(nq, ROWS, S, split), fold);
    float second = fold.second;
    int sidx = fold.sidx;
    {
        const float od = __shfl_xor(second, 32);
        const int oi = __shfl_xor(sidx, 32);
        lex_min(second, sidx, od, oi);
    }
    if (hi == 0 && a < na) {
        if (S == 1) {
            const size_t o = (size_t)p * cap_a + a;
            second_dist[o] = second;
            second_argmin[o] = (sidx == 0x7fffffff) ? 0 : sidx;
            keep[o] = ratio_keep(gate, o, min_dist[o], ratio, second);
        } else {
            const size_t o = ((size_t)p * S + split) * cap_a + a;
            ws_dist[o] = second;
            ws_idx[o] = sidx;
        }
    }
}

// ------------------------------------------------------------------------------------------------ wider descriptors (LDS-staged)
struct SecondFoldStaged : PixelStage<MT> {
    int ys[2], xs[2], r;                    // the lane's two anchor columns (ni)
    float second[2] = {INFINITY, INFINITY};
    int sidx[2] = {0x7fffffff, 0x7fffffff};
    __device__ __forceinline__ void tile(f32x16 (&acc)[2][2], int qt)
    {
        const int wm = threadIdx.x >> 7, hi = (threadIdx.x & 63) >> 5;
        const int qrow = wm * 64 + 4 * hi;
        const bool full = (qt + 1) * MT <= nq;
        bool improves = false;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            float mx = acc[0][ni][0];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int e = 0; e < 16; ++e) mx = fmaxf(mx, acc[mi][ni][e]);
            improves = improves || __fmaf_rn(-0.5f, mx, 0.5f) < second[ni];
        }
        if (!full || __any(improves)) {
            const unsigned *px = rows(qt) + qrow;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int q0 = qt * MT + qrow + mi * 32 + 8 * r4;
                    float d[2][4];
                    bool pass = false;
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            d[ni][e] = __fmaf_rn(-0.5f, acc[mi][ni][4 * r4 + e], 0.5f);
                            if (!full) d[ni][e] = (q0 + e < nq) ? d[ni][e] : INFINITY;
                            pass = pass || d[ni][e] < second[ni];
                        }
                    if (!__any(pass)) continue;
                    const uint4 pk4 = *reinterpret_cast<const uint4 *>(px + mi * 32 + 8 * r4);
                    const unsigned pk[4] = {pk4.x, pk4.y, pk4.z, pk4.w};
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool better = d[ni][e] < second[ni] && outside_disc(pk[e], ys[ni], xs[ni], r);
                            second[ni] = better ? d[ni][e] : second[ni];
                            sidx[ni] = better ? q0 + e : sidx[ni];
                        }
                }
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.0f;
    }
};

__global__ __launch_bounds__(MATCH_THREADS, 2) void match_second_staged_kernel(
    const float *__restrict__ a_hat, const float *__restrict__ q_hat, int B, int Cp, int cap_a, int cap_q, const int32_t *__restrict__ n_a,
    const int32_t *__restrict__ n_q, const int32_t *__restrict__ roi_q, int roi_stride_q, int W_q, int radius,
    const float *__restrict__ min_dist, const int32_t *__restrict__ argmin, const uint8_t *__restrict__ gate, float ratio, int T, int S,
    float *__restrict__ second_dist, int32_t *__restrict__ second_argmin, uint8_t *__restrict__ keep, float *__restrict__ ws_dist,
    int32_t *__restrict__ ws_idx)
{
    __shared__ float smem[4 * TILE_FLOATS];  // [buf][Q|A][128][33]
    __shared__ __attribute__((aligned(16))) unsigned pix[2 * MT];

    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int per_pair = T * S;
    const int p = (slot / per_pair) * 8 + xcd;
    if (p >= B) return;
    const int rem = slot % per_pair;
    const int panel = rem / S, split = rem % S;
    const int na = n_a[p], nq = n_q[p];
    const int a0 = panel * MT;
    if (a0 >= na) return;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wn = wave & 1, l31 = lane & 31;
    const int32_t *roi = roi_q + (size_t)p * roi_stride_q;
    SecondFoldStaged fold;
    fold.pix = pix;
    fold.roi = roi;
    fold.nq = nq;
    fold.W = W_q;
    fold.r = radius;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
        star_pixel(argmin + (size_t)p * cap_a, roi, a0 + wn * 64 + ni * 32 + l31, na, nq, W_q, fold.ys[ni], fold.xs[ni]);
    match_staged_walk(smem, a_hat + ((size_t)p * cap_a + a0) * Cp, q_hat + (size_t)p * cap_q * Cp, Cp, split_span(nq, MT, S, split), fold);

    float d;
    int i;
    staged_columns(smem, fold.second, fold.sidx, d, i);
    if (t < MT && a0 + t < na) {
        if (S == 1) {
            const size_t o = (size_t)p * cap_a + a0 + t;
            second_dist[o] = d;
            second_argmin[o] = (i == 0x7fffffff) ? 0 : i;
            keep[o] = ratio_keep(gate, o, min_dist[o], ratio, d);
        } else {
            const size_t o = ((size_t)p * S + split) * cap_a + a0 + t;
            ws_dist[o] = d;
            ws_idx[o] = i;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the merge of the query splits
__global__ void match_second_merge_kernel(const float *__restrict__ ws_dist, const int32_t *__restrict__ ws_idx, int S, int cap_a,
                                          const int32_t *__restrict__ n_a, const float *__restrict__ min_dist,
                                          const uint8_t *__restrict__ gate, float ratio, float *__restrict__ second_dist,
                                          int32_t *__restrict__ second_argmin, uint8_t *__restrict__ keep)
{
    const int p = blockIdx.y;
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_a[p]) return;
    float d = INFINITY;
    int i = 0x7fffffff;
    for (int s = 0; s < S; ++s) {
        const size_t o = ((size_t)p * S + s) * cap_a + a;
        lex_min(d, i, ws_dist[o], ws_idx[o]);
    }
    const size_t o = (size_t)p * cap_a + a;
    second_dist[o] = d;
    second_argmin[o] = (i == 0x7fffffff) ? 0 : i;
    keep[o] = ratio_keep(gate, o, min_dist[o], ratio, d);
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_match_second_workspace_bytes(int B, int cap_a)
{
    if (B <= 0 || cap_a <= 0) return 0;
    SplitWs w;
    return carve_split(nullptr, w, B, cap_a, match_f32_split(B, cap_a / MT));
}

extern "C" int oryon_match_second_f32(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q, const int32_t *n_a,
                                      const int32_t *n_q, const int32_t *roi_q, int roi_stride_q, int W_q, int radius,
                                      const float *min_dist, const int32_t *argmin, const uint8_t *gate, float ratio, float *second_dist,
                                      int32_t *second_argmin, uint8_t *keep, void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(a_hat && q_hat && n_a && n_q && roi_q);
    ORYON_CHECK_ARG(min_dist && argmin);
    ORYON_CHECK_ARG(second_dist && second_argmin && keep);
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);
    ORYON_CHECK_ARG(C > 0 && C % BK == 0);
    ORYON_CHECK_ARG(cap_a > 0 && cap_a % MT == 0);
    ORYON_CHECK_ARG(cap_q > 0 && cap_q % MT == 0);
    ORYON_CHECK_ARG(C != 32 || cap_q % 256 == 0);       // the C_pad 32 kernel streams the query rows in tiles of 256
    ORYON_CHECK_ARG(roi_stride_q > 0);
    ORYON_CHECK_ARG(W_q >= 1 && W_q <= 65535);          // a pixel packs into one word: y << 16 | x
    ORYON_CHECK_ARG(radius >= 1 && radius <= 1024);
    ORYON_CHECK_ARG(ratio > 0.0f && ratio <= 1.0f);     // a NaN fails both
    if (B == 0) return ORYON_OK;
    const int T = cap_a / MT;
    const int S = match_f32_split(B, T);
    SplitWs w;
    const size_t need = carve_split(workspace, w, B, cap_a, S);
    if (need) ORYON_CHECK_WORKSPACE("oryon_match_second_f32: ", workspace, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const int groups = staged_groups(B, T, S), groups_regb = regb_groups(B, T, S);
#define LAUNCH_REGB(CPV)                                                                                                          \
    hipLaunchKernelGGL((match_second_regb_kernel<CPV>), dim3(groups_regb), dim3(MATCH_THREADS), 0, st, a_hat, q_hat, B, cap_a, cap_q, \
                       n_a, n_q, roi_q, roi_stride_q, W_q, radius, min_dist, argmin, gate, ratio, T, S, second_dist, second_argmin,  \
                       keep, w.ws_dist, w.ws_idx)
    if (C == 32) LAUNCH_REGB(32);
    else if (C == 64) LAUNCH_REGB(64);
    else if (C == 128) LAUNCH_REGB(128);
    else if (C == 256) LAUNCH_REGB(256);
    else
        hipLaunchKernelGGL(match_second_staged_kernel, dim3(groups), dim3(MATCH_THREADS), 0, st, a_hat, q_hat, B, C, cap_a, cap_q, n_a, n_q,
                           roi_q, roi_stride_q, W_q, radius, min_dist, argmin, gate, ratio, T, S, second_dist, second_argmin, keep,
                           w.ws_dist, w.ws_idx);
#undef LAUNCH_REGB
    ORYON_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(match_second_merge_kernel, dim3(cap_a / 256 + 1, B), dim3(256), 0, st, w.ws_dist, w.ws_idx, S, cap_a, n_a,
                           min_dist, gate, ratio, second_dist, second_argmin, keep);
        ORYON_CHECK_LAUNCH();
    }
    return ORYON_OK;
}
