// K1n: one rank scan of the one-to-many matcher.  For every anchor row i the best query row OUTSIDE the discs of `radius` pixels round
// the pixels of up to three earlier ranks prev[0..n_prev)[i] (include/oryon_hip.h has the definition).  n_prev = 1 is K1r's second
// minimum; the K - 1 calls of oryon_topk_corrs (post.hip) walk the ranks 2..K of the DRAWN anchor rows.
//
// It is K1r's scan (match_second.hip) with more than one centre: the same two tile walks (match_tile.h), the same pixel stage
// (match_disc.h), the same skip in front of the mask - the wave-wide unmasked `d < running` first, the pixels and the integer tests
// only when some lane passes - and the same merge of the query splits by (distance, index).  What differs:
//   * a lane keeps three (y*, x*) centres per anchor column; a centre that is not there (n_prev < 3, an index outside [0, n_q)) is
//     PIX_NONE, which every pixel is outside of, so the fold always makes three integer tests and has one instantiation per width;
//   * there is no keep: the rank's (distance, index) is the output, with index -1 and INFINITY where no row is left.
#include "common.h"
#include "match_common.h"
#include "match_tile.h"
#include "match_disc.h"

namespace oryon {

constexpr int NEXT_PREV_MAX = 3;
constexpr int NEXT_NONE = 0x7fffffff;

struct Centres {
    int ys[NEXT_PREV_MAX], xs[NEXT_PREV_MAX];
    __device__ __forceinline__ bool outside(unsigned pk, int r) const
    {
        return outside_disc(pk, ys[0], xs[0], r) && outside_disc(pk, ys[1], xs[1], r) && outside_disc(pk, ys[2], xs[2], r);
    }
};
// prev: plane-major [n_prev][B, cap_a]; prev_p points at pair p's row of plane 0
__device__ __forceinline__ void load_centres(Centres &c, const int32_t *__restrict__ prev_p, size_t plane, int n_prev,
                                             const int32_t *__restrict__ roi, int a, int na, int nq, int W)
{
#pragma unroll
    for (int k = 0; k < NEXT_PREV_MAX; ++k) {
        c.ys[k] = c.xs[k] = PIX_NONE;
        if (k < n_prev) star_pixel(prev_p + k * plane, roi, a, na, nq, W, c.ys[k], c.xs[k]);
    }
}

// ------------------------------------------------------------------------------------------------ C_pad 32 / 64 / 128 / 256
template <int CP> struct NextFoldRegb : PixelStage<RegbGeom<CP>::ROWS> {
    static constexpr int ROWS = RegbGeom<CP>::ROWS, NACC = RegbGeom<CP>::NACC;
    Centres c;
    int r;
    float best = INFINITY;
    int bidx = NEXT_NONE;
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
        const bool improves = __fmaf_rn(-0.5f, mx, 0.5f) < best;        // unmasked: a row inside a disc may raise a false alarm
        if (!full || __any(improves)) {
            const unsigned *px = this->rows(qt) + 4 * hi;
#pragma unroll
            for (int m = 0; m < NACC; ++m)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    // four consecutive query rows: the unmasked test first, for the whole wave; their pixels are read and the integer
                    // tests made only when some lane passes it
                    const int q0 = qlane + m * 32 + 8 * r4;
                    float d[4];
                    bool pass = false;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        d[e] = __fmaf_rn(-0.5f, acc[m][4 * r4 + e], 0.5f);
                        if (!full) d[e] = (q0 + e < this->nq) ? d[e] : INFINITY;
                        pass = pass || d[e] < best;
                    }
                    if (!__any(pass)) continue;
                    const uint4 pk4 = *reinterpret_cast<const uint4 *>(px + m * 32 + 8 * r4);
                    const unsigned pk[4] = {pk4.x, pk4.y, pk4.z, pk4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool better = d[e] < best && c.outside(pk[e], r);        // strict: first (smallest) candidate index wins ties
                        best = better ? d[e] : best;
                        bidx = better ? q0 + e : bidx;
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
__global__ __launch_bounds__(MATCH_THREADS, 2) void match_next_regb_kernel(
    const float *__restrict__ a_hat, const float *__restrict__ q_hat, int B, int cap_a, int cap_q, const int32_t *__restrict__ n_a,
    const int32_t *__restrict__ n_q, const int32_t *__restrict__ roi_q, int roi_stride_q, int W_q, int radius,
    const int32_t *__restrict__ prev, int n_prev, int T, int S, float *__restrict__ next_dist, int32_t *__restrict__ next_argmin,
    float *__restrict__ ws_dist, int32_t *__restrict__ ws_idx)
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
    NextFoldRegb<CP> fold;
    fold.pix = pix;
    fold.roi = roi;
    fold.nq = nq;
    fold.W = W_q;
    fold.r = radius;
    load_centres(fold.c, prev + (size_t)p * cap_a, (size_t)B * cap_a, n_prev, roi, a, na, nq, W_q);
    match_regb_walk<CP>(smem, a_hat + ((size_t)p * cap_a + a) * CP + 4 * hi, reinterpret_cast<const char *>(q_hat + (size_t)p * cap_q * CP),
                        split_span(nq, ROWS, S, split), fold);
    float best = fold.best;
    int bidx = fold.bidx;
    {
        const float od = __shfl_xor(best, 32);
        const int oi = __shfl_xor(bidx, 32);
        lex_min(best, bidx, od, oi);
    }
    if (hi == 0 && a < na) {
        if (S == 1) {
            const size_t o = (size_t)p * cap_a + a;
            next_dist[o] = best;
            next_argmin[o] = (bidx == NEXT_NONE) ? -1 : bidx;
        } else {
            const size_t o = ((size_t)p * S + split) * cap_a + a;
            ws_dist[o] = best;
            ws_idx[o] = bidx;
        }
    }
}

// ------------------------------------------------------------------------------------------------ wider descriptors (LDS-staged)
struct NextFoldStaged : PixelStage<MT> {
    Centres c[2];                           // the lane's two anchor columns (ni)
    int r;
    float best[2] = {INFINITY, INFINITY};
    int bidx[2] = {NEXT_NONE, NEXT_NONE};
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
            improves = improves || __fmaf_rn(-0.5f, mx, 0.5f) < best[ni];
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
                            pass = pass || d[ni][e] < best[ni];
                        }
                    if (!__any(pass)) continue;
                    const uint4 pk4 = *reinterpret_cast<const uint4 *>(px + mi * 32 + 8 * r4);
                    const unsigned pk[4] = {pk4.x, pk4.y, pk4.z, pk4.w};
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool better = d[ni][e] < best[ni] && c[ni].outside(pk[e], r);
                            best[ni] = better ? d[ni][e] : best[ni];
                            bidx[ni] = better ? q0 + e : bidx[ni];
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

__global__ __launch_bounds__(MATCH_THREADS, 2) void match_next_staged_kernel(
    const float *__restrict__ a_hat, const float *__restrict__ q_hat, int B, int Cp, int cap_a, int cap_q, const int32_t *__restrict__ n_a,
    const int32_t *__restrict__ n_q, const int32_t *__restrict__ roi_q, int roi_stride_q, int W_q, int radius,
    const int32_t *__restrict__ prev, int n_prev, int T, int S, float *__restrict__ next_dist, int32_t *__restrict__ next_argmin,
    float *__restrict__ ws_dist, int32_t *__restrict__ ws_idx)
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
    NextFoldStaged fold;
    fold.pix = pix;
    fold.roi = roi;
    fold.nq = nq;
    fold.W = W_q;
    fold.r = radius;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
        load_centres(fold.c[ni], prev + (size_t)p * cap_a, (size_t)B * cap_a, n_prev, roi, a0 + wn * 64 + ni * 32 + l31, na, nq, W_q);
    match_staged_walk(smem, a_hat + ((size_t)p * cap_a + a0) * Cp, q_hat + (size_t)p * cap_q * Cp, Cp, split_span(nq, MT, S, split), fold);

    float d;
    int i;
    staged_columns(smem, fold.best, fold.bidx, d, i);
    if (t < MT && a0 + t < na) {
        if (S == 1) {
            const size_t o = (size_t)p * cap_a + a0 + t;
            next_dist[o] = d;
            next_argmin[o] = (i == NEXT_NONE) ? -1 : i;
        } else {
            const size_t o = ((size_t)p * S + split) * cap_a + a0 + t;
            ws_dist[o] = d;
            ws_idx[o] = i;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the merge of the query splits
__global__ void match_next_merge_kernel(const float *__restrict__ ws_dist, const int32_t *__restrict__ ws_idx, int S, int cap_a,
                                        const int32_t *__restrict__ n_a, float *__restrict__ next_dist, int32_t *__restrict__ next_argmin)
{
    const int p = blockIdx.y;
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_a[p] || a >= cap_a) return;
    float d = INFINITY;
    int i = NEXT_NONE;
    for (int s = 0; s < S; ++s) {
        const size_t o = ((size_t)p * S + s) * cap_a + a;
        lex_min(d, i, ws_dist[o], ws_idx[o]);
    }
    const size_t o = (size_t)p * cap_a + a;
    next_dist[o] = d;
    next_argmin[o] = (i == NEXT_NONE) ? -1 : i;
}

size_t match_next_split_bytes(int B, int cap_a, size_t start)
{
    SplitWs w;
    return carve_split(nullptr, w, B, cap_a, match_f32_split(B, cap_a / MT), start);
}

// the launches of one rank scan, arguments checked by the caller; split buffers carved from workspace at ws_start
int match_next_launch(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q,
                      const int32_t *roi_q, int roi_stride_q, int W_q, int radius, const int32_t *prev, int n_prev, float *next_dist,
                      int32_t *next_argmin, void *workspace, size_t ws_start, hipStream_t st)
{
    const int T = cap_a / MT;
    const int S = match_f32_split(B, T);
    SplitWs w;
    carve_split(workspace, w, B, cap_a, S, ws_start);
    const int groups = staged_groups(B, T, S), groups_regb = regb_groups(B, T, S);
#define LAUNCH_REGB(CPV)                                                                                                        \
    hipLaunchKernelGGL((match_next_regb_kernel<CPV>), dim3(groups_regb), dim3(MATCH_THREADS), 0, st, a_hat, q_hat, B, cap_a, cap_q, \
                       n_a, n_q, roi_q, roi_stride_q, W_q, radius, prev, n_prev, T, S, next_dist, next_argmin, w.ws_dist, w.ws_idx)
    if (C == 32) LAUNCH_REGB(32);
    else if (C == 64) LAUNCH_REGB(64);
    else if (C == 128) LAUNCH_REGB(128);
    else if (C == 256) LAUNCH_REGB(256);
    else
        hipLaunchKernelGGL(match_next_staged_kernel, dim3(groups), dim3(MATCH_THREADS), 0, st, a_hat, q_hat, B, C, cap_a, cap_q, n_a, n_q,
                           roi_q, roi_stride_q, W_q, radius, prev, n_prev, T, S, next_dist, next_argmin, w.ws_dist, w.ws_idx);
#undef LAUNCH_REGB
    if (hipGetLastError() != hipSuccess) return ORYON_ERR_HIP;
    if (S > 1) {
        hipLaunchKernelGGL(match_next_merge_kernel, dim3(cap_a / 256 + 1, B), dim3(256), 0, st, w.ws_dist, w.ws_idx, S, cap_a, n_a, next_dist,
                           next_argmin);
        if (hipGetLastError() != hipSuccess) return ORYON_ERR_HIP;
    }
    return ORYON_OK;
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_match_next_workspace_bytes(int B, int cap_a)
{
    if (B <= 0 || cap_a <= 0) return 0;
    return match_next_split_bytes(B, cap_a, 0);
}

extern "C" int oryon_match_next_f32(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q, const int32_t *n_a,
                                    const int32_t *n_q, const int32_t *roi_q, int roi_stride_q, int W_q, int radius,
                                    const int32_t *prev_argmin, int n_prev, float *next_dist, int32_t *next_argmin, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(a_hat && q_hat && n_a && n_q && roi_q);
    ORYON_CHECK_ARG(prev_argmin);
    ORYON_CHECK_ARG(next_dist && next_argmin);
    ORYON_CHECK_ARG(n_prev >= 1 && n_prev <= NEXT_PREV_MAX);
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);
    ORYON_CHECK_ARG(C > 0 && C % BK == 0);
    ORYON_CHECK_ARG(cap_a > 0 && cap_a % MT == 0);
    ORYON_CHECK_ARG(cap_q > 0 && cap_q % MT == 0);
    ORYON_CHECK_ARG(C != 32 || cap_q % 256 == 0);       // the C_pad 32 kernel streams the query rows in tiles of 256
    ORYON_CHECK_ARG(roi_stride_q > 0);
    ORYON_CHECK_ARG(W_q >= 1 && W_q <= 65535);          // a pixel packs into one word: y << 16 | x
    ORYON_CHECK_ARG(radius >= 1 && radius <= 1024);
    if (B == 0) return ORYON_OK;
    const size_t need = match_next_split_bytes(B, cap_a, 0);
    if (need) ORYON_CHECK_WORKSPACE("oryon_match_next_f32: ", workspace, workspace_bytes, need);
    if (match_next_launch(a_hat, q_hat, B, C, cap_a, cap_q, n_a, n_q, roi_q, roi_stride_q, W_q, radius, prev_argmin, n_prev, next_dist,
                          next_argmin, workspace, 0, as_stream(stream)) != ORYON_OK) {
        set_error("%s: launch failed", __func__);
        return ORYON_ERR_HIP;
    }
    return ORYON_OK;
}
