// The scan with exclusion discs, once, for K1r (match_second.hip: one centre per anchor, the ratio test) and K1n (match_next.hip: three
// centres, one rank of the one-to-many matcher): for every anchor row the best query row OUTSIDE the discs of `radius` pixels round the
// pixels of NC earlier query rows of that anchor.  The files keep what is their own: what a finished row turns into (Out::row) and the
// C entries.  Here: a query row's pixel packed into one word, the integer disc rule, the pixel stage of a query tile in LDS, an
// anchor's centres, the two masked folds, the two scan kernels, the merge of the query splits, the launcher and the common argument
// checks.
//
// The result depends on each anchor's own earlier rows, so it is a second all-pairs scan: K1's two tile walks (match_tile.h) with a
// masked fold.
//   * a lane owns one anchor column (the C/D layout of the 32x32x2 MFMA); it keeps that anchor's NC (y*, x*) centres and its running
//     (distance, index) in registers;
//   * the packed pixels (y << 16 | x) of a tile's query rows are staged in LDS with the tile: fetched when the tile's loads are issued,
//     stored in front of the barrier that publishes the tile, double buffered by tile parity.  All lanes of a half-wave hold the same
//     query rows, so the fold's reads of them are broadcasts (four consecutive rows per ds_read_b128);
//   * K1's skip stands in front of the mask: the tile's largest dot product decides whether ANY lane of the wave can improve its running
//     distance; only then is the tile walked, four query rows at a time: the unmasked `d < running` for the whole wave first, the four
//     pixels and the integer tests only when some lane passes.  Once the running distance has settled only the rows inside an anchor's
//     own discs (at most ~pi r^2 each, those nearer than the running distance) pass the first test again;
//   * unused query rows are masked by index (K0 zero-fills only to the next multiple of 256); anchor columns >= n_a compute garbage in
//     their own lane and are not written;
//   * a centre that is not there (an index outside [0, n_q); with NC > 1 also a plane >= n_prev) is PIX_NONE, which every pixel is
//     outside of, so a fold always makes NC integer tests and has one instantiation per width and NC;
//   * query splits merge as K1's do, by (distance, index); a row is finished (Out::row) by whichever launch has its last word: the scan
//     when S == 1, the merge otherwise.
#pragma once
#include "common.h"
#include "match_common.h"
#include "match_tile.h"

namespace oryon {

constexpr int PIX_NONE = -(1 << 20);       // an anchor without a nearest row (n_q == 0, or an index outside the pair): nothing is excluded

__device__ __forceinline__ unsigned pack_pixel(int idx, int W) { const int y = idx / W; return ((unsigned)y << 16) | (unsigned)(idx - y * W); }
// (y - y*)^2 + (x - x*)^2 >= r^2 in integers; r <= 1024, so the squares are formed only where they cannot overflow
__device__ __forceinline__ bool outside_disc(unsigned pk, int ys, int xs, int r)
{
    const int dy = abs((int)(pk >> 16) - ys), dx = abs((int)(pk & 0xffffu) - xs);
    return dy >= r || dx >= r || dy * dy + dx * dx >= r * r;
}

// what the folds share: the pixel stage of a tile of ROWS query rows (thread t < ROWS owns row t) and an anchor's (y*, x*)
template <int ROWS> struct PixelStage {
    unsigned *pix;                          // LDS [2][ROWS]
    const int32_t *roi;                     // the pair's query pixel list
    int nq, W;
    unsigned pre = 0;
    int slot = 0;
    __device__ __forceinline__ void prefetch(int qt)
    {
        const int t = threadIdx.x, q = qt * ROWS + t;
        slot = (qt & 1) * ROWS + t;
        if (t < ROWS) pre = (q < nq) ? pack_pixel(roi[q], W) : 0u;
    }
    __device__ __forceinline__ void publish()
    {
        if ((int)threadIdx.x < ROWS) pix[slot] = pre;
    }
    __device__ __forceinline__ const unsigned *rows(int qt) const { return pix + (qt & 1) * ROWS; }
};
__device__ __forceinline__ void star_pixel(const int32_t *__restrict__ argmin_p, const int32_t *__restrict__ roi, int a, int na, int nq, int W,
                                           int &ys, int &xs)
{
    ys = xs = PIX_NONE;
    if (a < na) {
        const int j = argmin_p[a];
        if (j >= 0 && j < nq) {
            const unsigned pk = pack_pixel(roi[j], W);
            ys = (int)(pk >> 16);
            xs = (int)(pk & 0xffffu);
        }
    }
}

// An anchor column's NC centres are two plain arrays in its fold, ys[NC] and xs[NC]; the staged fold keeps its two columns' as
// ys[2][NC], xs[2][NC].  The order of these members is felt in the generated fold: with one {ys, xs} struct per column the compiler
// made the last disc test of the one-centre staged fold two selects instead of a branch (profiles/r19_disc_scan_one_copy.md).
template <int NC> __device__ __forceinline__ bool outside_centres(unsigned pk, const int (&ys)[NC], const int (&xs)[NC], int r)
{
    // one centre: the call itself, so that `d < running && outside_disc(..)` stays a short-circuit (as the loop below with NC = 1 the
    // compiler turns it into straight-line selects: another kernel)
    if constexpr (NC == 1) return outside_disc(pk, ys[0], xs[0], r);
    bool o = true;
#pragma unroll
    for (int k = 0; k < NC; ++k) o = o && outside_disc(pk, ys[k], xs[k], r);
    return o;
}
// the centres of anchor row a.  prev: plane-major [n_prev][B, cap_a]; prev_p points at pair p's row of plane 0.  One centre is always there
template <int NC>
__device__ __forceinline__ void load_centres(int (&ys)[NC], int (&xs)[NC], const int32_t *__restrict__ prev_p, size_t plane, int n_prev,
                                             const int32_t *__restrict__ roi, int a, int na, int nq, int W)
{
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        ys[k] = xs[k] = PIX_NONE;
        if (NC == 1 || k < n_prev) star_pixel(prev_p + k * plane, roi, a, na, nq, W, ys[k], xs[k]);
    }
}

// the operands of a scan, by value; T, S and the split buffers are the launcher's
struct DiscArgs {
    const float *a_hat, *q_hat;
    int B, C, cap_a, cap_q;
    const int32_t *n_a, *n_q, *roi_q;
    int roi_stride_q, W_q, radius;
    const int32_t *prev;                    // the centres' query rows, plane-major [n_prev][B, cap_a]
    int n_prev;
    int T = 0, S = 0;
    float *ws_dist = nullptr;
    int32_t *ws_idx = nullptr;
};

// ------------------------------------------------------------------------------------------------ C_pad 32 / 64 / 128 / 256
template <int CP, int NC> struct DiscFoldRegb : PixelStage<RegbGeom<CP>::ROWS> {
    static constexpr int ROWS = RegbGeom<CP>::ROWS, NACC = RegbGeom<CP>::NACC;
    int ys[NC], xs[NC], r;
    float best = INFINITY;
    int bidx = ROW_NONE;
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
                    // accumulator registers 4 r4 .. 4 r4 + 3 hold rows 4 hi + 8 r4 + 0 .. 3 of block m
                    const uint4 pk4 = *reinterpret_cast<const uint4 *>(px + m * 32 + 8 * r4);
                    const unsigned pk[4] = {pk4.x, pk4.y, pk4.z, pk4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool better = d[e] < best && outside_centres(pk[e], ys, xs, r);      // strict: first (smallest) candidate index wins ties
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

template <int CP, int NC, class Out> __global__ __launch_bounds__(MATCH_THREADS, 2) void match_disc_regb_kernel(const DiscArgs g, const Out out)
{
    constexpr int ROWS = RegbGeom<CP>::ROWS;
    __shared__ __attribute__((aligned(256))) char smem[2 * RegbGeom<CP>::TILE_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned pix[2 * ROWS];

    const int T = g.T, S = g.S, cap_a = g.cap_a;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int unit = (slot / T) * 8 + xcd;              // (pair, split) unit; all T panels of a unit share an XCD
    if (unit >= g.B * S) return;
    const int panel = slot % T;
    const int p = unit / S, split = unit % S;
    const int na = g.n_a[p], nq = g.n_q[p];
    const int a0 = panel * MT;
    if (a0 >= na) return;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const int a = a0 + wave * 32 + l31;                 // this lane's anchor row
    const int32_t *roi = g.roi_q + (size_t)p * g.roi_stride_q;
    DiscFoldRegb<CP, NC> fold;
    fold.pix = pix;
    fold.roi = roi;
    fold.nq = nq;
    fold.W = g.W_q;
    fold.r = g.radius;
    load_centres(fold.ys, fold.xs, g.prev + (size_t)p * cap_a, (size_t)g.B * cap_a, g.n_prev, roi, a, na, nq, g.W_q);
    match_regb_walk<CP>(smem, g.a_hat + ((size_t)p * cap_a + a) * CP + 4 * hi,
                        reinterpret_cast<const char *>(g.q_hat + (size_t)p * g.cap_q * CP), split_span(nq, ROWS, S, split), fold);
    float best = fold.best;
    int bidx = fold.bidx;
    {
        const float od = __shfl_xor(best, 32);
        const int oi = __shfl_xor(bidx, 32);
        lex_min(best, bidx, od, oi);
    }
    if (hi == 0 && a < na) {
        if (S == 1) {
            out.row((size_t)p * cap_a + a, best, bidx);
        } else {
            const size_t o = ((size_t)p * S + split) * cap_a + a;
            g.ws_dist[o] = best;
            g.ws_idx[o] = bidx;
        }
    }
}

// ------------------------------------------------------------------------------------------------ wider descriptors (LDS-staged)
template <int NC> struct DiscFoldStaged : PixelStage<MT> {
    int ys[2][NC], xs[2][NC], r;            // the lane's two anchor columns (ni)
    float best[2] = {INFINITY, INFINITY};
    int bidx[2] = {ROW_NONE, ROW_NONE};
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
                            const bool better = d[ni][e] < best[ni] && outside_centres(pk[e], ys[ni], xs[ni], r);
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

template <int NC, class Out> __global__ __launch_bounds__(MATCH_THREADS, 2) void match_disc_staged_kernel(const DiscArgs g, const Out out)
{
    __shared__ float smem[4 * TILE_FLOATS];  // [buf][Q|A][128][33]
    __shared__ __attribute__((aligned(16))) unsigned pix[2 * MT];

    const int T = g.T, S = g.S, Cp = g.C, cap_a = g.cap_a;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int per_pair = T * S;
    const int p = (slot / per_pair) * 8 + xcd;
    if (p >= g.B) return;
    const int rem = slot % per_pair;
    const int panel = rem / S, split = rem % S;
    const int na = g.n_a[p], nq = g.n_q[p];
    const int a0 = panel * MT;
    if (a0 >= na) return;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wn = wave & 1, l31 = lane & 31;
    const int32_t *roi = g.roi_q + (size_t)p * g.roi_stride_q;
    DiscFoldStaged<NC> fold;
    fold.pix = pix;
    fold.roi = roi;
    fold.nq = nq;
    fold.W = g.W_q;
    fold.r = g.radius;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
        load_centres(fold.ys[ni], fold.xs[ni], g.prev + (size_t)p * cap_a, (size_t)g.B * cap_a, g.n_prev, roi, a0 + wn * 64 + ni * 32 + l31, na, nq,
                     g.W_q);
    match_staged_walk(smem, g.a_hat + ((size_t)p * cap_a + a0) * Cp, g.q_hat + (size_t)p * g.cap_q * Cp, Cp, split_span(nq, MT, S, split),
                      fold);

    float d;
    int i;
    staged_columns(smem, fold.best, fold.bidx, d, i);
    if (t < MT && a0 + t < na) {
        if (S == 1) {
            out.row((size_t)p * cap_a + a0 + t, d, i);
        } else {
            const size_t o = ((size_t)p * S + split) * cap_a + a0 + t;
            g.ws_dist[o] = d;
            g.ws_idx[o] = i;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the merge of the query splits
template <class Out>
__global__ void match_disc_merge_kernel(const float *__restrict__ ws_dist, const int32_t *__restrict__ ws_idx, int S, int cap_a,
                                        const int32_t *__restrict__ n_a, const Out out)
{
    const int p = blockIdx.y;
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_a[p] || a >= cap_a) return;
    float d = INFINITY;
    int i = ROW_NONE;
    for (int s = 0; s < S; ++s) {
        const size_t o = ((size_t)p * S + s) * cap_a + a;
        lex_min(d, i, ws_dist[o], ws_idx[o]);
    }
    out.row((size_t)p * cap_a + a, d, i);
}

// ------------------------------------------------------------------------------------------------ host side
// where the query-split buffers of a scan end when they are carved at start
inline size_t match_disc_split_bytes(int B, int cap_a, size_t start)
{
    SplitWs w;
    return carve_split(nullptr, w, B, cap_a, match_f32_split(B, cap_a / MT), start);
}

// the launches of one scan, arguments checked by the caller; split buffers carved from workspace at ws_start
template <int NC, class Out> hipError_t match_disc_launch(DiscArgs g, const Out &out, void *workspace, size_t ws_start, hipStream_t st)
{
    g.T = g.cap_a / MT;
    g.S = match_f32_split(g.B, g.T);
    SplitWs w;
    carve_split(workspace, w, g.B, g.cap_a, g.S, ws_start);
    g.ws_dist = w.ws_dist;
    g.ws_idx = w.ws_idx;
#define LAUNCH_REGB(CPV) \
    hipLaunchKernelGGL((match_disc_regb_kernel<CPV, NC, Out>), dim3(regb_groups(g.B, g.T, g.S)), dim3(MATCH_THREADS), 0, st, g, out)
    if (g.C == 32) LAUNCH_REGB(32);
    else if (g.C == 64) LAUNCH_REGB(64);
    else if (g.C == 128) LAUNCH_REGB(128);
    else if (g.C == 256) LAUNCH_REGB(256);
    else hipLaunchKernelGGL((match_disc_staged_kernel<NC, Out>), dim3(staged_groups(g.B, g.T, g.S)), dim3(MATCH_THREADS), 0, st, g, out);
#undef LAUNCH_REGB
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && g.S > 1) {
        hipLaunchKernelGGL((match_disc_merge_kernel<Out>), dim3(g.cap_a / 256 + 1, g.B), dim3(256), 0, st, g.ws_dist, g.ws_idx, g.S, g.cap_a,
                           g.n_a, out);
        e = hipGetLastError();
    }
    return e;
}

// the argument checks both C entries make, expanded inside the entry (its name and the conditions' texts are what the refusal says);
// dist, idx: the entry's two output rows
#define ORYON_CHECK_DISC_ARGS(dist, idx)                                                                                          \
    ORYON_CHECK_ARG(a_hat && q_hat && n_a && n_q && roi_q);                                                                       \
    ORYON_CHECK_ARG(dist && idx);                                                                                                 \
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);                                                                                        \
    ORYON_CHECK_ARG(C > 0 && C % BK == 0);                                                                                        \
    ORYON_CHECK_ARG(cap_a > 0 && cap_a % MT == 0);                                                                                \
    ORYON_CHECK_ARG(cap_q > 0 && cap_q % MT == 0);                                                                                \
    ORYON_CHECK_ARG(C != 32 || cap_q % 256 == 0);       /* the C_pad 32 kernel streams the query rows in tiles of 256 */          \
    ORYON_CHECK_ARG(roi_stride_q > 0);                                                                                            \
    ORYON_CHECK_ARG(W_q >= 1 && W_q <= 65535);          /* a pixel packs into one word: y << 16 | x */                            \
    ORYON_CHECK_ARG(radius >= 1 && radius <= 1024)

}  // namespace oryon
