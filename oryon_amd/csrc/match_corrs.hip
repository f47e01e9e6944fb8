// The lazy matcher: int8 / MX-fp6 screen -> validity of every anchor -> sampled correspondences (oryon_match_corrs_*).
// Kernels of the tail, its workspace and host sequence, and the C entries.  The screens, K1s and the host steps of K1s8 it is built
// from are in match16.hip / screen_mx6.hip; the second level in match_x3.hip; the exact scan in match.hip; the sampler in post.hip.
#include <hip/hip_fp16.h>
#include "common.h"
#include "match_common.h"
#include "match_exact.h"

// ------------------------------------------------------------------------------------------------ lazy tail: K1s8 -> sampled correspondences
// The batched engine consumes the matcher through oryon_select_corrs only: it needs the VALID FLAG of every anchor and the argmin of the
// <= max_corrs anchors that get sampled (utils/pcd.py:205-214).  The int8 bound decides validity outright for almost every anchor:
//     m1 - DELTA8 > 1 - 2 thr   =>  the exact distance is below the threshold   (valid, whatever the argmin)
//     m1 + DELTA8 < 1 - 2 thr   =>  it is not                                   (as before)
// so candidate generation (16 int8 rows per anchor) and exact re-scoring (256 strided reads per candidate) are deferred to the sampled
// anchors - 500 per pair instead of 5000.  Anchors whose validity the bound cannot settle are resolved (exactly) before the sampling;
// a pair in which a possibly-valid anchor is AMBIGUOUS (runner-up slice within the int8 margin: its argmin needs the fp16 stage) takes
// the eager route of oryon_match_screened8_raw for all of its anchors.  Outputs are what select(match_screened8_raw(...)) gives,
// bit for bit: same valid set, same sampled rows (the sampling keys depend on the valid set only), same argmin for every sampled row.
namespace oryon {
// INVALID / VALID: settled by the int8 bound.  UNCERTAIN: unambiguous winner slice, validity not settled (resolved from that slice before
// the sampling).  AMB_VALID: validity settled (valid) but the runner-up slice is within the int8 margin - the exact argmin is computed
// only if the row gets sampled.  AMB_UNCERTAIN: neither settled - resolved before the sampling.  Both AMB kinds are resolved by the EXACT
// fp32 scan (K1) on a compacted list of just those anchor rows against the pair's materialised fp32 query rows.
constexpr uint8_t LZ_INVALID = 0, LZ_VALID = 1, LZ_UNCERTAIN = 2, LZ_AMB_VALID = 3, LZ_RESOLVED = 4, LZ_AMB_UNCERTAIN = 5;
// row classes of the default route's cascade (described in front of its kernels, further down)
constexpr uint8_t DC_COMPLETE = 0, DC_SETTLED = 1, DC_OPEN = 2;

// The default-route cascade's open rows, for the decide pass: a row of class DC_OPEN has its list slot in r_i1 (written by
// match_dc_settle_rows_kernel) and its complete triples per split in the [B, S, cap_a] arrays m1 / i1 / m2, indexed by that slot (the
// open rows' scan).  The decide pass merges them - as every other merge here: the maximum, the second-largest slice maximum, ties to
// the lowest slice id - and stores the merged triple to r_m1 / r_i1 / r_m2, the rows' merged arrays, for the later readers.
// cls == nullptr: no such rows.  r_* are the arrays the decide pass reads its S = 1 triples from: no __restrict__ on either side.
struct DcOpenRows {
    const uint8_t *cls = nullptr;
    int S = 0;
    const float *m1 = nullptr;
    const int32_t *i1 = nullptr;
    const float *m2 = nullptr;
    float *r_m1 = nullptr;
    int32_t *r_i1 = nullptr;
    float *r_m2 = nullptr;
};

// one anchor row: merge the per-split (m1, slice, m2) triples and classify; -> the row is ambiguous (lazy route only)
__device__ __forceinline__ bool decide_lite_row(
    int cap_a, int p, int a, int S, const float *ws_m1, const int32_t *ws_i1,
    const float *ws_m2, const DcOpenRows &open, const float *__restrict__ a_scale8, const float *__restrict__ eps_q8, float cut0, float sqrt_c,
    float c_true, int force_eager, int fmt, int x3, float *__restrict__ m_final, int32_t *__restrict__ sid_final, float *__restrict__ margin_out,
    uint8_t *__restrict__ state, uint8_t *__restrict__ valid, float *__restrict__ min_dist, int32_t *__restrict__ argmin,
    int32_t *__restrict__ pair_eager, int32_t *__restrict__ n_unc, int32_t *__restrict__ unc_idx, int32_t *__restrict__ n_ambu,
    int32_t *__restrict__ ambu_idx, int32_t *__restrict__ need_f32_lazy)
{
    const size_t arow = (size_t)p * cap_a + a;
    float m1, m2;
    int sid;
    if (open.cls && open.cls[arow] == DC_OPEN) {
        merge_split_triples(open.m1, open.i1, open.m2, p, open.S, cap_a, open.r_i1[arow], m1, sid, m2);
        open.r_m1[arow] = m1;
        open.r_i1[arow] = sid;
        open.r_m2[arow] = m2;
    } else
        merge_split_triples(ws_m1, ws_i1, ws_m2, p, S, cap_a, a, m1, sid, m2);
    ScreenBound b;
    if (fmt == 1) b = mx6_bound(a_scale8[p], eps_q8[p]);      // the pair's largest anchor / query row error
    else {
        const float sa = a_scale8[(size_t)p * (cap_a / 16) + anchor_scale_slot(a)];
        m1 *= sa;
        m2 *= sa;
        b = i8_bound(sa, eps_q8[p], sqrt_c, c_true);
    }
    const bool usable = b.usable();
    const float margin = b.margin();
    m_final[arow] = m1;
    sid_final[arow] = sid;
    margin_out[arow] = margin;
    uint8_t st;
    const bool certain_valid = usable && m1 > b.sure_line(cut0);
    if (usable && !(m1 >= b.cannot_line(cut0))) st = LZ_INVALID;
    else if (!(m1 - m2 > margin)) st = certain_valid ? LZ_AMB_VALID : LZ_AMB_UNCERTAIN;
    else if (certain_valid) st = LZ_VALID;
    else st = LZ_UNCERTAIN;
    state[arow] = st;
    // provisional outputs: the distance is the screening estimate until (unless) the row is resolved exactly
    min_dist[arow] = dist_from_dot(m1);
    argmin[arow] = 0;
    valid[arow] = (st == LZ_VALID || st == LZ_AMB_VALID) ? 1 : 0;
    if (force_eager) { pair_eager[p] = 1; return false; }
    if (st == LZ_UNCERTAIN) unc_idx[(size_t)p * cap_a + atomicAdd(&n_unc[p], 1)] = a;
    if (st == LZ_AMB_UNCERTAIN) ambu_idx[(size_t)p * cap_a + atomicAdd(&n_ambu[p], 1)] = a;
    if (st == LZ_AMB_VALID || st == LZ_AMB_UNCERTAIN) {
        // this pair's fp32 query rows get materialised (device-gated launch) - with the fp16x3 second level (x3) only when an
        // ambiguous anchor's VALIDITY is open too: the sampled valid ones are then resolved from hi / lo half rows made later
        if (st == LZ_AMB_UNCERTAIN || !x3) need_f32_lazy[p] = 1;
        return true;
    }
    return false;
}

// one THREAD per anchor.  n_amb_part [B, gridDim.x]: every workgroup's count of ambiguous rows, one plain store each (zero for a
// workgroup past n_a), summed by the two readers.  One add per wave on a word per pair - ~80 adds on one address, since round 10 made
// most rows ambiguous-valid - was 26 of this kernel's 32 us at 64 x 5000 rows (round 13: 31.9 us with the add, 5.9 us with it compiled
// out).  n_unc / n_ambu keep their returning adds: they index lists, and such rows are rare
__global__ __launch_bounds__(256) void match_decide_lite_kernel(
    int cap_a, const int32_t *__restrict__ n_a, int S, const float *ws_m1, const int32_t *ws_i1,
    const float *ws_m2, const DcOpenRows open, const float *__restrict__ a_scale8, const float *__restrict__ eps_q8, float cut0, float sqrt_c,
    float c_true, int force_eager, int fmt, int x3, float *__restrict__ m_final, int32_t *__restrict__ sid_final, float *__restrict__ margin_out,
    uint8_t *__restrict__ state, uint8_t *__restrict__ valid, float *__restrict__ min_dist, int32_t *__restrict__ argmin,
    int32_t *__restrict__ pair_eager, int32_t *__restrict__ n_unc, int32_t *__restrict__ unc_idx, int32_t *__restrict__ n_ambu,
    int32_t *__restrict__ ambu_idx, int32_t *__restrict__ need_f32_lazy, int32_t *__restrict__ n_amb_part)
{
    __shared__ int s_amb[4];
    const int p = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
    bool amb = false;
    if (a < n_a[p])
        amb = decide_lite_row(cap_a, p, a, S, ws_m1, ws_i1, ws_m2, open, a_scale8, eps_q8, cut0, sqrt_c, c_true, force_eager, fmt, x3, m_final, sid_final,
                              margin_out, state, valid, min_dist, argmin, pair_eager, n_unc, unc_idx, n_ambu, ambu_idx, need_f32_lazy);
    if (force_eager) return;                                    // (the eager route reads no such count)
    const unsigned long long amb_lanes = __ballot(amb);
    if ((threadIdx.x & 63) == 0) s_amb[threadIdx.x >> 6] = __popcll(amb_lanes);
    __syncthreads();
    if (threadIdx.x == 0) n_amb_part[(size_t)p * gridDim.x + blockIdx.x] = s_amb[0] + s_amb[1] + s_amb[2] + s_amb[3];
}

// sum of a pair's parts (match_decide_lite_kernel)
__device__ __forceinline__ int amb_total(const int32_t *__restrict__ n_amb_part, int n_parts, int p)
{
    int tot = 0;
    for (int i = 0; i < n_parts; ++i) tot += n_amb_part[(size_t)p * n_parts + i];
    return tot;
}

__global__ void match_mask_counts_kernel(int B, const int32_t *__restrict__ n_a, const int32_t *__restrict__ pair_eager,
                                         int32_t *__restrict__ n_a_eager, int32_t *__restrict__ n_a_lazy)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    n_a_eager[p] = pair_eager[p] ? n_a[p] : 0;
    n_a_lazy[p] = pair_eager[p] ? 0 : n_a[p];
}

__global__ void match_cascade_counts_kernel(int B, const int32_t *__restrict__ n_amb_part, int n_parts, const int32_t *__restrict__ n_after,
                                            const int32_t *__restrict__ n_before, int32_t *__restrict__ out)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    const long long tot = amb_total(n_amb_part, n_parts, p), nb = n_before[p], na = n_after[p];
    out[p] = nb > 0 ? (int32_t)(tot * na / nb) : (int32_t)tot;
}

__global__ void match_sum_counts_kernel(int B, const int32_t *__restrict__ a, const int32_t *__restrict__ n_amb_part, int n_parts,
                                        int32_t *__restrict__ out)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < B) out[p] = a[p] + amb_total(n_amb_part, n_parts, p);
}

// fp32 anchor rows of a work list -> dense panels for the exact scan (rows [count, round_up(count, 128)) zero-filled)
__global__ __launch_bounds__(256) void match_compact_f32_kernel(const float *__restrict__ a_hat, int Cp, int cap_a, int cap_c,
                                                                 const int32_t *__restrict__ count, const int32_t *__restrict__ idx,
                                                                 int idx_stride, float *__restrict__ a_c)
{
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int n = count[p] < cap_c ? count[p] : cap_c;
    const int n_fill = (n + 127) / 128 * 128;
    for (int g = 0; g < 16; ++g) {
        const int sl = (blockIdx.x * 16 + g) * 4 + (threadIdx.x >> 6);
        if (sl >= n_fill || sl >= cap_c) break;
        uint4 *d = reinterpret_cast<uint4 *>(a_c + ((size_t)p * cap_c + sl) * Cp);
        if (sl >= n) {
            for (int i = lane; i < Cp / 4; i += 64) d[i] = make_uint4(0, 0, 0, 0);
            continue;
        }
        const uint4 *src = reinterpret_cast<const uint4 *>(a_hat + ((size_t)p * cap_a + idx[(size_t)p * idx_stride + sl]) * Cp);
        for (int i = lane; i < Cp / 4; i += 64) d[i] = src[i];
    }
}

// results of an exact scan on a compacted work list -> the anchors' rows; the rows are marked RESOLVED (argmin / min_dist exact)
__global__ __launch_bounds__(256) void match_scatter_exact_kernel(int cap_a, int cap_c, const int32_t *__restrict__ count,
                                                                   const int32_t *__restrict__ idx, int idx_stride,
                                                                   const float *__restrict__ md_c, const int32_t *__restrict__ am_c,
                                                                   const uint8_t *__restrict__ va_c, float *__restrict__ min_dist,
                                                                   int32_t *__restrict__ argmin, uint8_t *__restrict__ valid,
                                                                   uint8_t *__restrict__ state)
{
    const int p = blockIdx.y, sl = blockIdx.x * 256 + threadIdx.x;
    const int n = count[p] < cap_c ? count[p] : cap_c;
    if (sl >= n) return;
    const size_t src = (size_t)p * cap_c + sl, dst = (size_t)p * cap_a + idx[(size_t)p * idx_stride + sl];
    min_dist[dst] = md_c[src];
    argmin[dst] = am_c[src];
    valid[dst] = va_c[src];
    state[dst] = LZ_RESOLVED;
}

// (the sampled slots whose anchor row is AMB_VALID - argmin still unknown - are listed for the second level by the kernels that hold the
// data: list_sampled_amb, match_common.h, called by the sampler and by match_decide_sampled_kernel)

// ---- validity cascade, second pass (round 6; oryon_match_corrs_mx6_x3).  The first screening pass stops a panel once its anchors are all
// valid for sure and leaves their runner-up open (match_mx6_screen_w4_kernel<.., EXIT>); the sampled ones among them (the list of
// list_sampled_amb, <= corr_rows per pair) get the COMPLETE screen here: their operand rows compacted into one panel per pair,
// the same kernel over all query tiles, and the (m1, slice, m2) triples merged back into the per-anchor arrays - a row whose winner turns
// out unambiguous becomes LZ_VALID (resolved from its winning slice like any other), the others keep LZ_AMB_VALID with their true winning
// slice as the second level's seed.
// the line a partial maximum must exceed to settle its row as valid for sure (match_exact.h); a_err / q_err: K0's (FMT = 1) per pair
__device__ __forceinline__ float dc_sure_line(const float *__restrict__ a_err, const float *__restrict__ q_err, int p, float cut0)
{
    const ScreenBound b = mx6_bound(a_err[p], q_err[p]);
    return b.usable() ? b.settled_line(cut0) : INFINITY;
}

// after the windowed first launch: is every live anchor of a 1024-row panel valid for sure already (its best score over the splits' windows
// above dc_sure_line)?  Then gate = 0 and its runner-ups read +inf (no margin: a partial scan rules nothing out);
// otherwise gate = 1: the gated launch scans everything for this panel and overwrites the triples.
__global__ __launch_bounds__(256) void match_panel_settle_kernel(int cap_a, int T8, int S, const int32_t *__restrict__ n_a,
                                                                  const float *__restrict__ ws_m1, float *__restrict__ ws_m2,
                                                                  const float *__restrict__ a_err, const float *__restrict__ q_err,
                                                                  float cut0, int32_t *__restrict__ gate)
{
    __shared__ int bad;
    const int p = blockIdx.y, panel = blockIdx.x, t = threadIdx.x;
    const int na = n_a[p], a0 = panel * 1024;
    if (a0 >= na) return;
    if (t == 0) bad = 0;
    __syncthreads();
    const float thr = dc_sure_line(a_err, q_err, p, cut0);
    int mine = 0;
    for (int a = a0 + t; a < a0 + 1024 && a < na; a += 256) {
        float m1 = -INFINITY;
        for (int s_ = 0; s_ < S; ++s_) m1 = fmaxf(m1, ws_m1[((size_t)p * S + s_) * cap_a + a]);
        mine |= !(m1 > thr);
    }
    if (mine) atomicOr(&bad, 1);
    __syncthreads();
    const int open = bad;
    if (t == 0) gate[p * T8 + panel] = open;
    if (!open)
        for (int a = a0 + t; a < a0 + 1024 && a < na; a += 256)
            for (int s_ = 0; s_ < S; ++s_) ws_m2[((size_t)p * S + s_) * cap_a + a] = INFINITY;
}

// One workgroup per pair, a thread per row of the sampled panel: the rows' decisions, then - behind a barrier - the second level's list of
// the rows that stay ambiguous (list_sampled_amb; count / idx are that list's own n_list / list, rebuilt in place).
constexpr int DS_THREADS = 512;
__global__ __launch_bounds__(DS_THREADS) void match_decide_sampled_kernel(int cap_a, int cap_c, int S, const int32_t *count,
                                                                           const int32_t *idx, int idx_stride,
                                                                           const float *__restrict__ ws_m1, const int32_t *__restrict__ ws_i1,
                                                                           const float *__restrict__ ws_m2, const float *__restrict__ a_err,
                                                                           const float *__restrict__ q_err, float *__restrict__ m_final,
                                                                           int32_t *__restrict__ sid_final, float *__restrict__ margin_out,
                                                                           uint8_t *state, int32_t *mark,
                                                                           int32_t *__restrict__ count_before, float *__restrict__ min_dist,
                                                                           const int32_t *__restrict__ pair_eager, const int32_t *__restrict__ n_sel,
                                                                           const int32_t *__restrict__ sel_rows, const SampledAmbList amb)
{
    __shared__ int s_wave[DS_THREADS / 64];
    const int p = blockIdx.x;
    const int n = count[p] < cap_c ? count[p] : cap_c;
    if (threadIdx.x == 0) count_before[p] = n;
    for (int sl = threadIdx.x; sl < n; sl += DS_THREADS) {
        const int a = idx[(size_t)p * idx_stride + sl];
        float m1, m2;
        int sid;
        merge_split_triples(ws_m1, ws_i1, ws_m2, p, S, cap_c, sl, m1, sid, m2);
        const float margin = mx6_bound(a_err[p], q_err[p]).margin();
        const size_t arow = (size_t)p * cap_a + a;
        m_final[arow] = m1;                                            // the complete scan's maximum (>= the partial one that settled validity)
        sid_final[arow] = sid;
        margin_out[arow] = margin;
        // default-route cascade: the provisional distance of a settled row came from its witness inside the band; the estimate a sampled
        // row reports is the complete scan's, as on the plain route
        if (min_dist) min_dist[arow] = dist_from_dot(m1);
        if (m1 - m2 > margin) {                                        // unambiguous after all: no second level for this row
            state[arow] = LZ_VALID;
            mark[arow] = 0;
        }
    }
    if (pair_eager[p]) return;
    list_sampled_amb(amb, p, cap_a, n_sel[p], sel_rows, idx_stride, s_wave);
}

// ---- validity cascade of the DEFAULT route, at anchor granularity (oryon_match_corrs_mx6[_araw], C_pad 256; DESIGN "default-route cascade").
// The result needs the validity of every anchor (one witness query within the threshold) and the complete (m1, slice, m2) of the sampled
// ones only.  On descriptors without the hard route's smoothness no whole panel settles, but row-major neighbours still match row-major
// neighbours, so the tiles a panel's matches lie in are LEARNED: a probe of every DC stride-th anchor gets the complete screen, the range
// of the probe's winning tiles (+ slack) is the panel's band - narrowed per 512-row half to the range of the half's own probe rows -, the
// band pass settles the rows that find their witness there, and only the
// rows left open (no counterpart at all, or a match outside the band) get the complete scan, compacted into dense 512-row panels.
// A row is COMPLETE (true triple over all tiles: probe rows, rows of a panel whose band is "all tiles", open rows after their scan) or
// SETTLED (partial maximum above dc_sure_line: valid for sure, m2 = +inf i.e. argmin open, as match_panel_settle_kernel
// leaves the rows of a settled panel).  Scores of an (anchor, query) pair do not depend on the panel the anchor row sits in, and the
// merged triple not on how the tiles are dealt to splits (ties go to the lowest slice either way): complete triples are today's.
// (DC_COMPLETE / DC_SETTLED / DC_OPEN: at the head of the file, for the decide pass)
constexpr int DC_SLACK = 2;            // tiles added at either end of a learned band
constexpr int DC_MIN_SURE = 8;          // a panel with fewer valid-for-sure probe rows scans all tiles
constexpr int DC_BAND_CAP_NUM = 1, DC_BAND_CAP_DEN = 2;     // ... and so does one whose band exceeds this share of the pair's tiles

// (the probe - rows 0, stride, 2 stride, .. of every pair - has no list: the list screen's stride mode forms it and its count)

// one workgroup per (1024-row panel, pair): the panel's probe rows get their complete triples, the panel its band [first, count) and
// each of its two 512-row halves a sub-band inside it: band[p][2 panel + h] (what the band pass scans and the settle pass looks up).
// The panel's band - and with it the decision to scan all tiles - is formed from all its sure probe rows as before the halves existed:
// stats[p][3] is the sum of these parent widths.  A half of an "all tiles" panel, or one with fewer than DC_MIN_SURE sure probe rows of
// its own, takes the panel's band; every other half the range of its own rows' winning tiles + slack, clipped to the panel's band.
// sub_stats (dev build's sweeps): stats[p][3] sums the halves' widths instead.
__global__ __launch_bounds__(256) void match_dc_probe_band_kernel(int cap_a, int T8, int stride, int S, const int32_t *__restrict__ n_a,
                                                                   const int32_t *__restrict__ n_q, const float *__restrict__ cs_m1,
                                                                   const int32_t *__restrict__ cs_i1, const float *__restrict__ cs_m2,
                                                                   const float *__restrict__ a_err, const float *__restrict__ q_err, float cut0,
                                                                   float *__restrict__ r_m1, int32_t *__restrict__ r_i1, float *__restrict__ r_m2,
                                                                   int32_t *__restrict__ band, int32_t *__restrict__ stats, int slack, int sub_stats)
{
    __shared__ int lo[2], hi[2], cnt[2];
    const int p = blockIdx.y, panel = blockIdx.x, t = threadIdx.x;
    const int na = n_a[p], a0 = panel * 1024;
    if (a0 >= na) return;
    if (t < 2) { lo[t] = 0x7fffffff; hi[t] = -1; cnt[t] = 0; }
    __syncthreads();
    const int a1 = a0 + 1024 < na ? a0 + 1024 : na;
    const int k_lo = (a0 + stride - 1) / stride;
    int k_hi = (a1 + stride - 1) / stride;
    k_hi = k_hi < MX6_SAMPLED_PANEL ? k_hi : MX6_SAMPLED_PANEL;
    const float line = dc_sure_line(a_err, q_err, p, cut0);
    for (int k = k_lo + t; k < k_hi; k += 256) {
        float m1, m2;
        int sid;
        merge_split_triples(cs_m1, cs_i1, cs_m2, p, S, MX6_SAMPLED_PANEL, k, m1, sid, m2);
        const size_t arow = (size_t)p * cap_a + (size_t)k * stride;
        r_m1[arow] = m1;
        r_i1[arow] = sid;
        r_m2[arow] = m2;
        if (m1 > line) {
            const int h = (k * stride - a0) >> 9;       // the row's 512-row half of the panel
            atomicMin(&lo[h], sid >> 3);                // 8 slices of 16 rows per 128-row tile
            atomicMax(&hi[h], sid >> 3);
            atomicAdd(&cnt[h], 1);
        }
    }
    __syncthreads();
    if (t == 0) {
        const int nqt = (n_q[p] + 127) / 128;
        const int plo = lo[0] < lo[1] ? lo[0] : lo[1], phi = hi[0] > hi[1] ? hi[0] : hi[1];
        int first = plo - slack < 0 ? 0 : plo - slack, end = phi + slack + 1 < nqt ? phi + slack + 1 : nqt;
        const bool all = cnt[0] + cnt[1] < DC_MIN_SURE || (long long)(end - first) * DC_BAND_CAP_DEN > (long long)nqt * DC_BAND_CAP_NUM;
        if (all) { first = 0; end = nqt; }
        int sub_sum = 0;
        for (int h = 0; h < 2; ++h) {
            int f = first, e = end;
            if (!all && cnt[h] >= DC_MIN_SURE) {
                f = lo[h] - slack > first ? lo[h] - slack : first;
                e = hi[h] + slack + 1 < end ? hi[h] + slack + 1 : end;
            }
            band[((p * T8 + panel) * 2 + h) * 2] = f;
            band[((p * T8 + panel) * 2 + h) * 2 + 1] = e - f;
            if (a0 + 512 * h < na) sub_sum += e - f;
        }
        atomicAdd(&stats[p * 4 + 3], sub_stats ? sub_sum : end - first);
        if (panel == 0) stats[p * 4 + 0] = (na + stride - 1) / stride < MX6_SAMPLED_PANEL ? (na + stride - 1) / stride : MX6_SAMPLED_PANEL;
    }
}

// one workgroup per pair, after the band pass: every row that is no probe row gets its class and (unless open) its triple; the open rows
// are listed in ascending order.  A lane owns one row per iteration (a = i blockDim + t: the [B, S, cap_a] triples are read coalesced),
// and a block-wide ordered scan of the iteration's open flags (the scan of block_scan_counts_sel, post.hip, on wave ballots) places them
// behind the earlier iterations'.  The next iteration's triple and band are loaded before this one's barrier.
constexpr int DC_SETTLE_THREADS = 1024;
__global__ __launch_bounds__(DC_SETTLE_THREADS) void match_dc_settle_rows_kernel(int cap_a, int T8, int stride, int S, const int32_t *__restrict__ n_a,
                                                                    const int32_t *__restrict__ n_q, const float *__restrict__ ws_m1,
                                                                    const int32_t *__restrict__ ws_i1, const float *__restrict__ ws_m2,
                                                                    const float *__restrict__ a_err, const float *__restrict__ q_err, float cut0,
                                                                    const int32_t *__restrict__ band, float *__restrict__ r_m1,
                                                                    int32_t *__restrict__ r_i1, float *__restrict__ r_m2, uint8_t *__restrict__ cls,
                                                                    int32_t *__restrict__ n_open, int32_t *__restrict__ open_idx,
                                                                    int32_t *__restrict__ stats)
{
    constexpr int NW = DC_SETTLE_THREADS / 64;
    __shared__ int wave_cnt[2][NW], wave_settled[NW];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int na = n_a[p] < cap_a ? n_a[p] : cap_a, nqt = (n_q[p] + 127) / 128;
    const float line = dc_sure_line(a_err, q_err, p, cut0);
    uint8_t *cl = cls + (size_t)p * cap_a;
    // merged triple of row a over the band pass's splits, and whether its half's band is "all tiles" (its parent panel's then: a learned
    // band is at most DC_BAND_CAP of the tiles)
    auto fetch = [&](int a, float &m1, int &sid, float &m2, bool &all) {
        if (a >= na) return;
        const int32_t *b = band + ((size_t)p * T8 * 2 + (a >> 9)) * 2;
        all = b[0] == 0 && b[1] == nqt;
        merge_split_triples(ws_m1, ws_i1, ws_m2, p, S, cap_a, a, m1, sid, m2);
    };
    float m1 = 0.0f, m2 = 0.0f, m1_n = 0.0f, m2_n = 0.0f;
    int sid = 0, sid_n = 0, base = 0, settled = 0;
    bool all = false, all_n = false;
    fetch(t, m1, sid, m2, all);
    for (int a0 = 0, it = 0; a0 < na; a0 += DC_SETTLE_THREADS, ++it) {
        const int a = a0 + t;
        fetch(a + DC_SETTLE_THREADS, m1_n, sid_n, m2_n, all_n);
        bool open = false, sett = false;
        if (a < na) {
            const size_t arow = (size_t)p * cap_a + a;
            uint8_t c = DC_COMPLETE;
            const bool probe = a % stride == 0 && a / stride < MX6_SAMPLED_PANEL;       // probe row: triple written by the probe
            if (!probe) {
                if (all) c = DC_COMPLETE;
                else if (m1 > line) { c = DC_SETTLED; m2 = INFINITY; sett = true; }     // no margin: a partial scan rules nothing out
                else { c = DC_OPEN; open = true; }
                if (c != DC_OPEN) { r_m1[arow] = m1; r_i1[arow] = sid; r_m2[arow] = m2; }
            }
            cl[a] = c;
        }
        const unsigned long long open_lanes = __ballot(open);
        settled += __popcll(__ballot(sett));
        if (lane == 0) wave_cnt[it & 1][wave] = __popcll(open_lanes);
        __syncthreads();                        // (two buffers: the writes of iteration it + 2 lie behind the barrier of it + 1)
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int c = wave_cnt[it & 1][w];
            before += w < wave ? c : 0;
            tot += c;
        }
        if (open) {
            // the row's slot also goes where its slice id will stand (DcOpenRows): the decide pass merges the open rows' scan from there
            const int slot = base + before + __popcll(open_lanes & ((1ull << lane) - 1ull));
            open_idx[(size_t)p * cap_a + slot] = a;
            r_i1[(size_t)p * cap_a + a] = slot;
        }
        base += tot;
        m1 = m1_n; sid = sid_n; m2 = m2_n; all = all_n;
    }
    if (lane == 0) wave_settled[wave] = settled;
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int w = 0; w < NW; ++w) s += wave_settled[w];
        n_open[p] = base;
        stats[p * 4 + 1] = s;
        stats[p * 4 + 2] = base;
    }
}

// (the complete triples of the open rows - scanned as compacted rows: [B, S, cap_a] indexed by list slot - reach the rows' merged arrays
// in match_decide_lite_kernel, the next reader of every row: DcOpenRows)

// Exact resolution of ONE unambiguous anchor by one wave: candidates = rows of the winning 16-row slice within the int8 margin of its
// maximum (slice_score_* of match_exact.h on the screen's own operand rows), then the canonical fp32 chain per candidate on x_k / d read
// from the raw map (wave_exact_dist).  Returns (distance, first index of the minimum) in lane 0.
// Anchor rows on demand (the `_araw` entries): where K0 wrote no fp32 unit rows (a_hat == nullptr), a consumer forms the row itself from
// the raw anchor map with K0's norm in a_norm (match_exact.h: raw_unit), bit for bit the value K0 would have stored.
struct AnchorRaw {
    const float *feat_a;        // [B, C_true, HW] (or channels-last), the map K0 gathered the anchors from
    const int32_t *roi_a;       // [B, roi_stride] pixel of every anchor row
    const float *a_norm;        // [B, cap_a] K0's row norms
    int roi_stride;
};

template <bool NHWC, bool NEED_DIST = true, int FMT = 0>
__device__ __forceinline__ void resolve_anchor(int p, int a, const float *__restrict__ a_hat, const AnchorRaw &araw, const int8_t *__restrict__ a8,
                                               const int8_t *__restrict__ q8, const float *__restrict__ q_scale8,
                                               const float *__restrict__ a_scale8, const float *__restrict__ feat_q, int C_true, int HW,
                                               const int32_t *__restrict__ roi_q, int roi_stride, const float *__restrict__ norm_q,
                                               int Cp, int cap_a, int cap_q, int nq, float m1, int sid, float margin, float *lds /*[2*Cp]*/,
                                               int round_f16, float &d_out, int &j_out)
{
    const int lane = threadIdx.x & 63;
    const size_t arow = (size_t)p * cap_a + a;
    const int seg = lane & 3;
    const int q = slice_row(sid, lane >> 2);
    bool hit;
    if constexpr (FMT == 1) {
        // mx6 rows: candidates = rows within the margin of the SLICE maximum (every exact minimiser is one and scores >= max - 2 delta)
        const float s6 = slice_score_mx6(a8 + arow * Cp, q8 + (size_t)p * cap_q * Cp, q, Cp, q < nq);
        float mx = (q < nq) ? s6 : -INFINITY;
#pragma unroll
        for (int off = 4; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        hit = (seg == 0) && (q < nq) && (s6 >= mx - margin - 4e-5f);
        (void)m1;
    } else {
        const float sa = a_scale8[(size_t)p * (cap_a / 16) + anchor_scale_slot(a)];
        const int idot = slice_score_i8(a8 + arow * Cp, q8 + (size_t)p * cap_q * Cp, q, Cp, q < nq);
        const float s8 = (float)idot * q_scale8[(size_t)p * (cap_q / 16) + sid] * sa;
        hit = (seg == 0) && (q < nq) && (s8 >= m1 - margin);
    }
    unsigned long long hits = __ballot(hit);
    if (!NEED_DIST && __popcll(hits) == 1) {
        // a single row inside the int8 margin IS the argmin (every other row is provably farther): no fp32 work, and none of the 256
        // scattered 4-byte reads of its raw descriptor (the NCHW gather is what bounds this kernel: one 64-byte sector per channel)
        j_out = __shfl(q, __ffsll((long long)hits) - 1);
        d_out = __builtin_nanf("");
        return;
    }
    // anchor row (k-permuted) -> natural order in LDS
    float *A = lds, *Q = lds + Cp;
    if (a_hat) {
        wave_unpermute_row(A, a_hat + arow * Cp, Cp);
    } else {
        // no materialised row: the same values from the raw map (one pass, Cp / 64 independent loads per lane), natural order as they come
        const float *fa = araw.feat_a + (size_t)p * C_true * HW;
        const int pix_a = araw.roi_a[(size_t)p * araw.roi_stride + a];
        const float da = araw.a_norm[arow];
        for (int k = lane; k < Cp; k += 64) A[k] = raw_unit<NHWC>(fa, pix_a, da, k, C_true, HW, round_f16);
    }
    float d = INFINITY;
    int j = 0x7fffffff;
    const float *fq = feat_q + (size_t)p * C_true * HW;
    while (hits) {
        const int src = __ffsll((long long)hits) - 1;
        hits &= hits - 1;
        const int jj = __shfl(q, src);
        const int pix = roi_q[(size_t)p * roi_stride + jj];
        const float dq = norm_q[(size_t)p * cap_q + jj];
        lex_min(d, j, wave_exact_dist<NHWC>(A, Q, fq, pix, dq, Cp, C_true, HW, round_f16), jj);
    }
    d_out = d;
    j_out = j;
}

// match_compact_f32_kernel for the `_araw` entries: the listed anchors' fp32 unit rows formed from the raw map (raw_unit) and
// written in the k-permuted order K0's rows have (match_exact.h: kperm_k), which is what K1 / K1x3 read.  One wave
// per row, one 16-byte store per lane: lane i of a pass owns positions 4i .. 4i + 3 = (g, h) = (i >> 1, i & 1), j = 0 .. 3.
template <bool NHWC>
__global__ __launch_bounds__(256) void match_compact_raw_kernel(const AnchorRaw araw, int C_true, int HW, int round_f16, int Cp, int cap_a,
                                                                 int cap_c, const int32_t *__restrict__ count, const int32_t *__restrict__ idx,
                                                                 int idx_stride, float *__restrict__ a_c)
{
    const int p = blockIdx.y, lane = threadIdx.x & 63;
    const int n = count[p] < cap_c ? count[p] : cap_c;
    const int n_fill = (n + 127) / 128 * 128;
    const float *fa = araw.feat_a + (size_t)p * C_true * HW;
    for (int g = 0; g < 16; ++g) {
        const int sl = (blockIdx.x * 16 + g) * 4 + (threadIdx.x >> 6);
        if (sl >= n_fill || sl >= cap_c) break;
        float4 *d = reinterpret_cast<float4 *>(a_c + ((size_t)p * cap_c + sl) * Cp);
        if (sl >= n) {
            for (int i = lane; i < Cp / 4; i += 64) d[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const int a = idx[(size_t)p * idx_stride + sl];
        const int pix = araw.roi_a[(size_t)p * araw.roi_stride + a];
        const float da = araw.a_norm[(size_t)p * cap_a + a];
        for (int i = lane; i < Cp / 4; i += 64) {
            const int g = i >> 1, hh = i & 1;
            float4 q;
            q.x = raw_unit<NHWC>(fa, pix, da, kperm_k(g, hh, 0), C_true, HW, round_f16);
            q.y = raw_unit<NHWC>(fa, pix, da, kperm_k(g, hh, 1), C_true, HW, round_f16);
            q.z = raw_unit<NHWC>(fa, pix, da, kperm_k(g, hh, 2), C_true, HW, round_f16);
            q.w = raw_unit<NHWC>(fa, pix, da, kperm_k(g, hh, 3), C_true, HW, round_f16);
            d[i] = q;
        }
    }
}

// anchors whose VALIDITY the int8 bound could not settle (pairs on the lazy route only): exact distance now, before the sampling
template <bool NHWC, int FMT = 0>
__global__ __launch_bounds__(256) void match_resolve_uncertain_kernel(
    const float *__restrict__ a_hat, const AnchorRaw araw, const int8_t *__restrict__ a8, const int8_t *__restrict__ q8, const float *__restrict__ q_scale8,
    const float *__restrict__ a_scale8, const float *__restrict__ feat_q, int C_true, int HW, const int32_t *__restrict__ roi_q,
    int roi_stride, const float *__restrict__ norm_q, int Cp, int cap_a, int cap_q, const int32_t *__restrict__ n_q, float thr,
    const float *__restrict__ m_final, const int32_t *__restrict__ sid_final, const float *__restrict__ margin_in,
    const int32_t *__restrict__ n_unc, const int32_t *__restrict__ unc_idx, const int32_t *__restrict__ pair_eager,
    uint8_t *__restrict__ state, uint8_t *__restrict__ valid, float *__restrict__ min_dist, int32_t *__restrict__ argmin, int round_f16)
{
    extern __shared__ float lds_res[];
    const int p = blockIdx.y;
    if (pair_eager[p]) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = n_unc[p];
    for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
        const int a = unc_idx[(size_t)p * cap_a + i];
        const size_t arow = (size_t)p * cap_a + a;
        float d;
        int j;
        resolve_anchor<NHWC, true, FMT>(p, a, a_hat, araw, a8, q8, q_scale8, a_scale8, feat_q, C_true, HW, roi_q, roi_stride, norm_q, Cp, cap_a, cap_q, n_q[p],
                             m_final[arow], sid_final[arow], margin_in[arow], lds_res + wave * 2 * Cp, round_f16, d, j);
        if (lane == 0) {
            min_dist[arow] = d;
            argmin[arow] = j;
            valid[arow] = (d < thr) ? 1 : 0;
            state[arow] = LZ_RESOLVED;
        }
    }
}

// the sampled rows of the lazy pairs: exact argmin -> query half of the correspondence
template <bool NHWC, int FMT = 0>
__global__ __launch_bounds__(256) void match_resolve_selected_kernel(
    const float *__restrict__ a_hat, const AnchorRaw araw, const int8_t *__restrict__ a8, const int8_t *__restrict__ q8, const float *__restrict__ q_scale8,
    const float *__restrict__ a_scale8, const float *__restrict__ feat_q, int C_true, int HW, const int32_t *__restrict__ roi_q,
    int roi_stride, const float *__restrict__ norm_q, int Cp, int cap_a, int cap_q, const int32_t *__restrict__ n_q, int W,
    const float *__restrict__ m_final, const int32_t *__restrict__ sid_final, const float *__restrict__ margin_in,
    const uint8_t *__restrict__ state, const int32_t *__restrict__ pair_eager, const int32_t *__restrict__ n_sel,
    const int32_t *__restrict__ sel_rows, int corr_rows, float *__restrict__ min_dist, int32_t *__restrict__ argmin,
    int32_t *__restrict__ corrs, int round_f16)
{
    extern __shared__ float lds_res[];
    const int p = blockIdx.y;
    if (pair_eager[p]) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = blockIdx.x * 4 + wave;
    if (slot >= n_sel[p]) return;
    const int a = sel_rows[(size_t)p * corr_rows + slot];
    const size_t arow = (size_t)p * cap_a + a;
    float d = 0.0f;
    int j;
    if (state[arow] == LZ_RESOLVED) {
        j = argmin[arow];
    } else {
        resolve_anchor<NHWC, false, FMT>(p, a, a_hat, araw, a8, q8, q_scale8, a_scale8, feat_q, C_true, HW, roi_q, roi_stride, norm_q, Cp, cap_a, cap_q,
                                    n_q[p], m_final[arow], sid_final[arow], margin_in[arow], lds_res + wave * 2 * Cp, round_f16, d, j);
        if (lane == 0) {                                                // same values from every slot that drew this row
            argmin[arow] = j;
            if (d == d) min_dist[arow] = d;                             // NaN: single candidate, the distance was never needed
        }
    }
    if (lane == 0) {
        j = (j < 0 || j >= n_q[p]) ? 0 : j;                            // cannot happen for a row that passed the validity cut
        const int pq = roi_q[(size_t)p * roi_stride + j];
        corrs[((size_t)p * corr_rows + slot) * 4 + 2] = pq / W;
        corrs[((size_t)p * corr_rows + slot) * 4 + 3] = pq % W;
    }
}
}  // namespace oryon

using namespace oryon;

namespace {
struct LazyWs : Screen8RawWs {
    float *margin;
    int32_t *sid_final, *pair_eager, *n_unc, *unc_idx, *n_a_eager, *n_a_lazy, *sel_rows, *scratch;
    int32_t *n_ambu, *ambu_idx, *n_ambv, *ambv_idx, *need_f32_lazy, *n_amb_room, *mark;
    int32_t *n_amb_part;                // [B, cap_a / 256] ambiguous rows per workgroup of match_decide_lite_kernel: ScreenWs' panel_flag
                                        // ([B, cap_a / 128], zeroed every call), which only the eager route's exact recomputation uses
    void *exact_ws;
    size_t exact_ws_bytes;
    // K1x3 (C_pad 256): hi / lo anchor rows, the overflow fall-back's compact rows and outputs, candidate lists
    __half *x3_ah, *x3_al;
    float *x3_a_ovf, *x3_md_o;
    int32_t *x3_am_o;
    uint8_t *x3_va_o;
    void *x3_scratch;
    uint8_t *state;
    // validity cascade (hard route, C_pad 256): the sampled anchors' mx6 rows as one 512-row panel per pair + the second pass's triples
    uint8_t *cs_panel;                  // null where the shape has no cascade (C_pad 512, or corr_rows beyond the panel)
    float *cs_max, *cs_m2;
    int32_t *cs_i1;
    int32_t *n_ambv0, *cs_gate;
    // validity cascade of the default route (C_pad 256, three panels or more): merged per-row triples and classes, the probe and open
    // lists, the panels' bands, the open rows' operands as dense 512-row panels, the per-split triples of its band and open passes;
    // counters (zeroed every call).  All of it lives INSIDE q16 - the fp16 query rows of the eager route's fall-back, which no lazy step
    // touches - so the workspace's size and layout are what they were
    bool dc_ok;                         // false where the shape has no such cascade (or q16 is too small for its buffers)
    uint8_t *dc_rows;
    float *dc_m1, *dc_m2, *dc_ws_m1, *dc_ws_m2;
    int32_t *dc_i1, *dc_ws_i1, *dc_probe_room, *dc_open_idx, *dc_band, *dc_n_probe, *dc_n_open, *dc_stats;
    uint8_t *dc_cls;
    size_t dc_zero_bytes;               // the counters, at the start of q16
    size_t lazy_zero_off, lazy_zero_bytes;      // the second zeroed region (ScreenWs has the first) ..
    size_t x3_zero_bytes;                       // .. which the head of x3_scratch continues when the second level is K1x3
};

// list capacity of the second level: distinct sampled rows <= min(max_corrs, n_a)
int sampled_cap(int corr_rows, int cap_a)
{
    const int cap_s0 = (corr_rows + 127) / 128 * 128;
    return cap_s0 < cap_a ? cap_s0 : cap_a;
}

// The default route's cascade is chosen by shape alone: three 1024-row panels or more (below that the 512-row probe is no small
// fraction of the anchors; the sample-first first stage has one panel), the second pass's 512-row panel large enough for the sample
bool dc_shape(int C, int cap_a, int corr_rows) { return C == 256 && corr_rows <= MX6_SAMPLED_PANEL && mx6_panels_per_pair(cap_a) >= 3; }
// the probe takes every 10th anchor, fewer where they would not fit its one 512-row panel
int dc_probe_stride(int cap_a)
{
    const int s = (cap_a + MX6_SAMPLED_PANEL - 1) / MX6_SAMPLED_PANEL;
    return s > 10 ? s : 10;
}
// splits of the band pass (4-wave workgroups over 512-row halves, two per CU: ~2.5 per place) and of the open rows' scan (the same kernel geometry)
int dc_band_splits(int B, int cap_a)
{
    const int u = B * 2 * mx6_panels_per_pair(cap_a), s = (1280 + u - 1) / u;
    return s < 1 ? 1 : s > 16 ? 16 : s;
}
int dc_open_splits(int B)
{
    const int s = (1024 + B - 1) / B;
    return s < 1 ? 1 : s > 16 ? 16 : s;
}
size_t carve_dc(void *base, LazyWs &w, int B, int C, int cap_a)
{
    Carver carve(base);
    const size_t rows = (size_t)B * cap_a, pairs = (size_t)B;
    const size_t S = 16;                                    // the most either pass uses (dc_band_splits, dc_open_splits)
    // the counters first: q16 begins where ScreenWs' zeroed region ends, so one fill clears both (match_corrs_lazy_impl)
    carve(w.dc_n_probe, pairs);
    carve(w.dc_n_open, pairs);
    carve(w.dc_stats, pairs * 4);
    w.dc_zero_bytes = carve.off;
    carve(w.dc_rows, rows * C);
    carve(w.dc_m1, rows);
    carve(w.dc_m2, rows);
    carve(w.dc_i1, rows);
    carve(w.dc_cls, rows);
    carve(w.dc_open_idx, rows);
    carve(w.dc_probe_room, pairs * MX6_SAMPLED_PANEL);                    // (the probe's index list until round 13: the shape gate's sum stays)
    carve(w.dc_band, pairs * mx6_panels_per_pair(cap_a) * 2 * 2);         // [first, count) per 512-row half of every 1024-row panel
    carve(w.dc_ws_m1, rows * S);
    carve(w.dc_ws_m2, rows * S);
    carve(w.dc_ws_i1, rows * S);
    return carve.off;
}

size_t carve_lazy(void *base, LazyWs &w, int B, int C, int cap_a, int cap_q, int S, int corr_rows)
{
    Carver carve(base, carve_screen8_raw(base, w, B, C, cap_a, cap_q, S));
    const size_t rows = (size_t)B * cap_a, pairs = (size_t)B;
    carve(w.margin, rows);
    carve(w.sid_final, rows);
    carve(w.unc_idx, rows);
    carve(w.state, rows);
    carve(w.sel_rows, pairs * corr_rows);
    carve(w.scratch, rows);
    carve(w.n_a_eager, pairs);
    carve(w.n_a_lazy, pairs);
    carve(w.ambu_idx, rows);
    carve(w.ambv_idx, pairs * corr_rows);
    const size_t cap_s = sampled_cap(corr_rows, cap_a);
    const size_t e1 = oryon_match_workspace_bytes(B, cap_a), e2 = oryon_match_workspace_bytes(B, (int)cap_s);
    w.exact_ws_bytes = e1 > e2 ? e1 : e2;                                  // split-merge scratch of the exact scan (either list capacity)
    carve(w.exact_ws, w.exact_ws_bytes > 16 ? w.exact_ws_bytes : 16);
    carve(w.x3_ah, pairs * cap_s * C);
    carve(w.x3_al, pairs * cap_s * C);
    carve(w.x3_a_ovf, pairs * cap_s * C);
    carve(w.x3_md_o, pairs * cap_s);
    carve(w.x3_am_o, pairs * cap_s);
    carve(w.x3_va_o, pairs * cap_s);
    const bool cascade = C == 256 && corr_rows <= MX6_SAMPLED_PANEL;
    const size_t triples = cascade ? pairs * mx6_sampled_splits(B) * MX6_SAMPLED_PANEL : 4;      // 16-byte placeholders without it
    carve(w.cs_panel, cascade ? pairs * MX6_SAMPLED_PANEL * C : 16);
    if (!cascade) w.cs_panel = nullptr;
    carve(w.cs_max, triples);
    carve(w.cs_m2, triples);
    carve(w.cs_i1, triples);
    carve(w.n_ambv0, pairs);
    carve(w.cs_gate, pairs * mx6_panels_per_pair(cap_a));
    w.dc_ok = false;
    w.dc_stats = nullptr;
    if (dc_shape(C, cap_a, corr_rows)) {
        LazyWs sized;
        if (carve_dc(nullptr, sized, B, C, cap_a) <= (size_t)B * cap_q * C * sizeof(__half)) {
            carve_dc(w.q16, w, B, C, cap_a);
            w.dc_ok = true;
        }
    }
    w.lazy_zero_off = carve.off;
    carve(w.pair_eager, pairs);
    carve(w.n_unc, pairs);
    carve(w.n_ambu, pairs);
    carve(w.n_ambv, pairs);
    carve(w.need_f32_lazy, pairs);
    carve(w.n_amb_room, pairs);                                            // (the per-pair count until round 13: the size is pinned)
    w.n_amb_part = w.panel_flag;
    carve(w.mark, rows);
    w.lazy_zero_bytes = carve.off - w.lazy_zero_off;
    // the second level's scratch last: what it needs zeroed is at its start (match_x3_zero_bytes), i.e. right behind `mark` - one fill
    w.x3_zero_bytes = match_x3_zero_bytes(B, (int)cap_s, 8);
    carve(w.x3_scratch, match_x3_scratch_bytes(B, (int)cap_s, 8, cap_q));
    return carve.off;
}
}  // namespace

extern "C" size_t oryon_match_corrs_i8_workspace_bytes(int B, int C, int cap_a, int cap_q, int corr_rows)
{
    if (B <= 0 || C <= 0 || cap_a <= 0 || cap_a % MT16 || cap_q <= 0 || corr_rows <= 0) return 0;
    LazyWs w;
    return carve_lazy(nullptr, w, B, C, cap_a, cap_q, pick_split16(B, cap_a / MT16), corr_rows);
}

int32_t *oryon::match_dc_stats(void *workspace, int B, int C, int cap_a, int cap_q, int corr_rows)
{
    LazyWs w;
    carve_lazy(workspace, w, B, C, cap_a, cap_q, pick_split16(B, cap_a / MT16), corr_rows);
    return w.dc_ok ? w.dc_stats : nullptr;
}

namespace {
constexpr const char *IMPL = "match_corrs_lazy_impl";       // the name launch failures of its two routes are reported under

// the second level's list of the sampled rows that are ambiguous-valid: what the sampler (lazy route) and the sampled rows' decide pass build
SampledAmbList sampled_amb_list(const LazyWs &w)
{
    SampledAmbList L;
    L.state = w.state;
    L.want = LZ_AMB_VALID;
    L.mark = w.mark;
    L.n_list = w.n_ambv;
    L.list = w.ambv_idx;
    return L;
}

int select_step(const MatchCorrsArgs &m, const LazyWs &w, hipStream_t st, const SampledAmbList &amb = SampledAmbList())
{
    const int rc = select_corrs_launch(m.roi_a, m.roi_q, m.roi_stride_a, m.roi_stride_q, m.n_a, m.n_q, m.argmin, m.valid, m.cap_a, m.B, m.W,
                                       m.max_corrs, m.corr_rows, m.seed, m.pair_key, w.scratch, m.corrs, m.n_valid, m.n_sel, m.status,
                                       w.sel_rows, w.pair_eager, st, amb);
    if (rc) set_error("oryon_match_corrs_i8: select launch failed");
    return rc;
}

// ---- eager route: the complete tail of oryon_match_screened8_raw for every pair (pair_eager is set only by force_eager since the
// ambiguous anchors of lazy pairs are resolved by compacted exact scans), then the sampler on the complete outputs
int eager_route(const MatchCorrsArgs &m, const LazyWs &w, int S)
{
    decide8_step(m, S, w.n_a_eager, w);
    rescore_raw_step(m, w.n_a_eager, 2, w);
    int rc = check_launch(IMPL);
    if (rc) return rc;
    if ((rc = raw_fallbacks(m, w.n_a_eager, w, IMPL, "oryon_match_corrs_i8"))) return rc;
    return select_step(m, w, as_stream(m.stream));
}

// anchor rows of a work list -> dense fp32 panels in w.a_hat_c (the launch geometry of match_compact_f32_kernel; rows from the raw map
// where K0 wrote none)
void compact_anchors(const MatchCorrsArgs &m, const AnchorRaw &araw, const LazyWs &w, hipStream_t st, int cap_c, const int32_t *count,
                     const int32_t *idx, int idx_stride)
{
    const dim3 grid((cap_c + 63) / 64, m.B);
    if (m.a_hat)
        hipLaunchKernelGGL(match_compact_f32_kernel, grid, dim3(256), 0, st, m.a_hat, m.C, m.cap_a, cap_c, count, idx, idx_stride, w.a_hat_c);
    else
        hipLaunchKernelGGL(m.layout == ORYON_LAYOUT_NHWC ? match_compact_raw_kernel<true> : match_compact_raw_kernel<false>, grid, dim3(256), 0,
                           st, araw, m.C_true, m.HW, m.round_f16, m.C, m.cap_a, cap_c, count, idx, idx_stride, w.a_hat_c);
}

int lazy_route(const MatchCorrsArgs &m, const LazyWs &w, hipStream_t st, int use_x3, bool cascade, bool dc)
{
    const int B = m.B, C = m.C, cap_a = m.cap_a, cap_q = m.cap_q, corr_rows = m.corr_rows;
    const bool nhwc = m.layout == ORYON_LAYOUT_NHWC;
    const AnchorRaw araw = {m.feat_a, m.roi_a, m.a_norm, m.roi_stride_a};
    // (1) pairs with ambiguous possibly-valid anchors get their fp32 query rows (device-gated, as on the eager route)
    int rc = gather_q8_launch(m.feat_q, B, m.C_true, m.HW, m.layout, m.roi_q, m.roi_stride_q, m.n_q, w.need_f32_lazy, cap_q, C, w.q8_scratch,
                              w.scale_scratch, w.eps_scratch, nullptr, w.q_hat, 1, m.round_f16, st);
    if (rc) { set_error("oryon_match_corrs_i8: lazy fp32 gather launch failed"); return rc; }
    // (2) ambiguous anchors whose VALIDITY is open: exact fp32 scan (K1) of exactly those rows, before the sampling
    compact_anchors(m, araw, w, st, cap_a, w.n_ambu, w.ambu_idx, cap_a);
    if ((rc = check_launch(IMPL))) return rc;
    rc = oryon_match_f32(w.a_hat_c, w.q_hat, B, C, cap_a, cap_q, w.n_ambu, m.n_q, m.threshold, w.md_c, w.am_c, w.va_c, w.exact_ws,
                         w.exact_ws_bytes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(match_scatter_exact_kernel, dim3(cap_a / 256, B), dim3(256), 0, st, cap_a, cap_a, w.n_ambu, w.ambu_idx, cap_a, w.md_c,
                       w.am_c, w.va_c, m.min_dist, m.argmin, m.valid, w.state);
    if ((rc = check_launch(IMPL))) return rc;
    // (3) unambiguous anchors whose validity is open: exact distance from the winning slice's candidates
    const size_t lds_res = (size_t)4 * 2 * C * sizeof(float);
    auto resolve_uncertain = m.fmt == 1 ? (nhwc ? match_resolve_uncertain_kernel<true, 1> : match_resolve_uncertain_kernel<false, 1>)
                                        : (nhwc ? match_resolve_uncertain_kernel<true, 0> : match_resolve_uncertain_kernel<false, 0>);
    hipLaunchKernelGGL(resolve_uncertain, dim3(64, B), dim3(256), lds_res, st, m.a_hat, araw, m.a_i8, m.q_i8, m.q_scale, m.a_scale, m.feat_q,
                       m.C_true, m.HW, m.roi_q, m.roi_stride_q, m.q_norm, C, cap_a, cap_q, m.n_q, m.threshold, w.m_final, w.sid_final, w.margin,
                       w.n_unc, w.unc_idx, w.pair_eager, w.state, m.valid, m.min_dist, m.argmin, m.round_f16);
    if ((rc = check_launch(IMPL))) return rc;
    // (4) the sampling, on the exact valid set; its workgroups also list the sampled rows that are ambiguous (n_ambv, ambv_idx)
    const SampledAmbList amb = sampled_amb_list(w);
    if ((rc = select_step(m, w, st, amb))) return rc;
    // (5) sampled rows that are ambiguous (valid for sure, argmin open): exact fp32 scan of just those <= max_corrs rows per pair
    const int cap_s = sampled_cap(corr_rows, cap_a);
    if (cascade) {
        // second pass: the complete screen for the listed rows (one 512-row panel per pair), triples merged back, list rebuilt
        const int csS = mx6_sampled_splits(B);
        // (the screen reads the listed rows in place, through the list: cs_panel keeps its room, unused)
        launch_screen_mx6_list512(st, reinterpret_cast<const uint8_t *>(m.a_i8), reinterpret_cast<const uint8_t *>(m.q_i8), B, cap_a, MX6_SAMPLED_PANEL,
                                  cap_q, w.n_ambv, w.ambv_idx, corr_rows, 0, m.n_q, csS, w.cs_max, w.cs_i1, w.cs_m2, m.C_true);
        hipLaunchKernelGGL(match_decide_sampled_kernel, dim3(B), dim3(DS_THREADS), 0, st, cap_a, MX6_SAMPLED_PANEL, csS,
                           w.n_ambv, w.ambv_idx, corr_rows, w.cs_max, w.cs_i1, w.cs_m2, m.a_scale, m.q_eps_max, w.m_final, w.sid_final,
                           w.margin, w.state, w.mark, w.n_ambv0, dc ? m.min_dist : nullptr, w.pair_eager, m.n_sel, w.sel_rows, amb);
        if ((rc = check_launch(IMPL))) return rc;
    }
    compact_anchors(m, araw, w, st, cap_s, w.n_ambv, w.ambv_idx, corr_rows);
    if ((rc = check_launch(IMPL))) return rc;
    if (use_x3) {
        // K1x3: hi / lo half query rows into the (now free) fp32-row area, fp16x3 scan with candidate lists, exact chain on the few
        // candidates; anchors whose lists overflowed (duplicate crowds) fall back to the exact scan on fp32 rows materialised for their pair
        __half *qh = reinterpret_cast<__half *>(w.q_hat), *ql = qh + (size_t)B * cap_q * C;
        int32_t *n_ovf = nullptr, *ovf_idx = nullptr;
        rc = match_x3_resolve(w.a_hat_c, w.n_ambv, cap_s, m.feat_q, m.C_true, m.HW, m.layout, m.roi_q, m.roi_stride_q, m.q_norm, m.n_q, B, cap_q,
                              m.threshold, m.round_f16, qh, ql, w.x3_ah, w.x3_al, w.x3_scratch, w.md_c, w.am_c, w.va_c, &n_ovf, &ovf_idx,
                              w.ambv_idx, corr_rows, w.sid_final, cap_a, static_cast<const __half *>(m.q_hi_lo), m.q_lo_sq_max, st);
        if (rc) { set_error("oryon_match_corrs: fp16x3 second-level launch failed"); return rc; }
        // fp32 query rows for the pairs with overflowed anchors only: the gather's per-map gate reads n_ovf itself
        rc = gather_q8_launch(m.feat_q, B, m.C_true, m.HW, m.layout, m.roi_q, m.roi_stride_q, m.n_q, n_ovf, cap_q, C, w.q8_scratch,
                              w.scale_scratch, w.eps_scratch, nullptr, w.q_hat, 1, m.round_f16, st);
        if (rc) { set_error("oryon_match_corrs: overflow fp32 gather launch failed"); return rc; }
        hipLaunchKernelGGL(match_compact_f32_kernel, dim3((cap_s + 63) / 64, B), dim3(256), 0, st, w.a_hat_c, C, cap_s, cap_s, n_ovf, ovf_idx,
                           cap_s, w.x3_a_ovf);
        if ((rc = check_launch(IMPL))) return rc;
        rc = oryon_match_f32(w.x3_a_ovf, w.q_hat, B, C, cap_s, cap_q, n_ovf, m.n_q, m.threshold, w.x3_md_o, w.x3_am_o, w.x3_va_o, w.exact_ws,
                             w.exact_ws_bytes, st);
        if (rc) return rc;
        match_x3_scatter_ovf(B, cap_s, n_ovf, ovf_idx, w.x3_md_o, w.x3_am_o, w.x3_va_o, w.md_c, w.am_c, w.va_c, st);
    } else {
        rc = oryon_match_f32(w.a_hat_c, w.q_hat, B, C, cap_s, cap_q, w.n_ambv, m.n_q, m.threshold, w.md_c, w.am_c, w.va_c, w.exact_ws,
                             w.exact_ws_bytes, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(match_scatter_exact_kernel, dim3((cap_s + 255) / 256, B), dim3(256), 0, st, cap_a, cap_s, w.n_ambv, w.ambv_idx,
                       corr_rows, w.md_c, w.am_c, w.va_c, m.min_dist, m.argmin, m.valid, w.state);
    if ((rc = check_launch(IMPL))) return rc;
    // (6) query half of every sampled correspondence: resolved rows read their argmin, the others get it from their winning slice
    auto resolve_selected = m.fmt == 1 ? (nhwc ? match_resolve_selected_kernel<true, 1> : match_resolve_selected_kernel<false, 1>)
                                       : (nhwc ? match_resolve_selected_kernel<true, 0> : match_resolve_selected_kernel<false, 0>);
    hipLaunchKernelGGL(resolve_selected, dim3((m.max_corrs + 3) / 4, B), dim3(256), lds_res, st, m.a_hat, araw, m.a_i8, m.q_i8, m.q_scale,
                       m.a_scale, m.feat_q, m.C_true, m.HW, m.roi_q, m.roi_stride_q, m.q_norm, C, cap_a, cap_q, m.n_q, m.W, w.m_final,
                       w.sid_final, w.margin, w.state, w.pair_eager, m.n_sel, w.sel_rows, corr_rows, m.min_dist, m.argmin, m.corrs,
                       m.round_f16);
    if ((rc = check_launch(IMPL))) return rc;
    if (m.n_undecided && cascade) {
        // cascade: the first pass calls every anchor of a panel that stopped early "ambiguous"; the feedback the engine steers by is that
        // count scaled by the share of the SAMPLED ambiguous rows which the complete second pass left ambiguous
        hipLaunchKernelGGL(match_cascade_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, w.n_amb_part, cap_a / 256, w.n_ambv, w.n_ambv0,
                           m.n_undecided);
        if ((rc = check_launch(IMPL))) return rc;
    } else if (m.n_undecided) {
        // anchors the int8 stage could not fully decide: the fp16-stage anchors of eager pairs + the ambiguous anchors of lazy pairs
        hipLaunchKernelGGL(match_sum_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, w.n_amb, w.n_amb_part, cap_a / 256,
                           m.n_undecided);
        if ((rc = check_launch(IMPL))) return rc;
    }
    return ORYON_OK;
}
}  // namespace

// fmt 0: int8 rows (a_scale / q_scale per 16-row slice, q_eps_max per pair).  fmt 1: mx6 rows in a_i8 / q_i8, a_scale = the largest
// anchor-row error norm per pair [B], q_eps_max = the largest query-row error norm per pair [B], q_scale unused; lazy route only.
int oryon::match_corrs_lazy_impl(const MatchCorrsArgs &m)
{
    // a_hat == nullptr (the `_araw` entries): the anchors' fp32 unit rows are formed on demand from feat_a / roi_a / a_norm.  Only the
    // lazy route can do that: the eager tail reads whole pairs of rows
    ORYON_CHECK_ARG((m.a_hat || (m.feat_a && m.a_norm && !m.force_eager)) && m.a_i8 && m.a_scale && m.feat_q && m.roi_a && m.roi_q && m.q_norm && m.q_i8 && m.q_eps_max && m.n_a && m.n_q);
    ORYON_CHECK_ARG((m.fmt == 0 || m.fmt == 1) && (m.fmt == 1 || m.q_scale) && !(m.fmt == 1 && m.force_eager));
    ORYON_CHECK_ARG(!m.q_hi_lo || (m.q_lo_sq_max && m.C == 256));
    ORYON_CHECK_ARG(m.min_dist && m.argmin && m.valid && m.corrs && m.n_valid && m.n_sel && m.status);
    ORYON_CHECK_ARG(m.B >= 0 && (m.C == 256 || m.C == 512) && m.C_true > 0 && m.C_true <= m.C && m.HW > 0 && m.W > 0 && m.max_corrs > 0 && m.corr_rows >= m.max_corrs);
    ORYON_CHECK_ARG(m.layout == ORYON_LAYOUT_NCHW || m.layout == ORYON_LAYOUT_NHWC);
    ORYON_CHECK_ARG(m.cap_a > 0 && m.cap_a % MT16 == 0 && m.cap_q > 0 && m.cap_q % 256 == 0 && m.threshold > 0.0f && m.threshold <= 0.5f);
    if (m.B == 0) return ORYON_OK;
    const int B = m.B, C = m.C, cap_a = m.cap_a, cap_q = m.cap_q;
    const int T = cap_a / MT16;
    const int S = pick_split16(B, T);
    LazyWs w;
    const size_t need = carve_lazy(m.workspace, w, B, C, cap_a, cap_q, S, m.corr_rows);
    ORYON_CHECK_WORKSPACE("oryon_match_corrs_i8: ", m.workspace, m.workspace_bytes, need);
    hipStream_t st = as_stream(m.stream);
    const float cut0 = 1.0f - 2.0f * m.threshold;
    // second level for the sampled anchors no screen can separate: fp16x3 two-sweep scan (K1x3, match_x3.hip; C_pad 256) instead of the
    // exact fp32 scan - same results, hard-descriptor step 9.8 -> 8.5 ms; ~30 us of empty launches per step when no anchor needs it.
    // ORYON_AMB_X3=0 keeps the exact scan (the tests run both settings).
    static const bool x3_env = dev_env_int("ORYON_AMB_X3", 1) != 0;
    const int use_x3 = (x3_env && C == 256 && !m.force_eager) ? 1 : 0;
    // Two fills per call.  ScreenWs' zeroed region runs on into the cascade's counters at the start of q16 (carve_dc; on fmt 1 they read
    // zero after any other route), the lazy tail's into what match_x3_resolve wants zeroed at the head of its scratch (carve_lazy)
    ORYON_CHECK_HIP(hipMemsetAsync(static_cast<char *>(m.workspace) + w.zero_off, 0, w.zero_bytes + (w.dc_ok && m.fmt == 1 ? w.dc_zero_bytes : 0), st));
    if (m.force_eager) ORYON_CHECK_HIP(hipMemsetAsync(w.need_f32, 0, (size_t)B * sizeof(int32_t), st));     // only the eager route reads it
    ORYON_CHECK_HIP(hipMemsetAsync(static_cast<char *>(m.workspace) + w.lazy_zero_off, 0, w.lazy_zero_bytes + (use_x3 ? w.x3_zero_bytes : 0), st));
    // validity cascade (round 6): on the route the engine takes once its feedback says "hard" (q_hi_lo given: K0 wrote the hi / lo rows),
    // the screen stops a panel whose anchors are all valid for sure, and a second, complete pass serves the sampled anchors only
    const bool cascade = m.fmt == 1 && use_x3 && m.q_hi_lo != nullptr && w.cs_panel != nullptr;
    // the default route's own cascade, at anchor granularity (kernels above: match_dc_*): by shape and the caller's knob alone
    const bool dc = m.cascade != 0 && m.fmt == 1 && use_x3 && m.q_hi_lo == nullptr && w.cs_panel != nullptr && w.dc_ok;
    int S_dec = S;                                                          // what match_decide_lite_kernel merges: the splits' triples ..
    const float *dec_m1 = w.ws_max, *dec_m2 = w.ws_m2;
    const int32_t *dec_i1 = w.ws_i1;
    DcOpenRows dc_open;
    if (m.fmt == 1) {
        const uint8_t *a6 = reinterpret_cast<const uint8_t *>(m.a_i8), *q6 = reinterpret_cast<const uint8_t *>(m.q_i8);
        const int groups = ((B * S + 7) / 8) * 8 * T;
        profile_begin(st, screen_mx6_name(C));
        if (cascade) {
            // first pass of the cascade: two tiles per (panel, split) near the panel's own place in the map, then the complete scan for the
            // panels that still hold an anchor whose validity is open (device-gated: the others return at once)
            const int T8 = mx6_panels_per_pair(cap_a);
            launch_screen_mx6(C, groups, T, st, a6, q6, B, cap_a, cap_q, m.n_a, m.n_q, S, w.ws_max, w.ws_i1, w.ws_m2, m.C_true, 1, nullptr, 2);
            hipLaunchKernelGGL(match_panel_settle_kernel, dim3(T8, B), dim3(256), 0, st, cap_a, T8, S, m.n_a, w.ws_max, w.ws_m2, m.a_scale,
                               m.q_eps_max, cut0, w.cs_gate);
            launch_screen_mx6(C, groups, T, st, a6, q6, B, cap_a, cap_q, m.n_a, m.n_q, S, w.ws_max, w.ws_i1, w.ws_m2, m.C_true, 1, w.cs_gate, 0);
        } else if (dc) {
            const int T8 = mx6_panels_per_pair(cap_a), stride = dc_probe_stride(cap_a), csS = mx6_sampled_splits(B);
            const int Sb = dc_band_splits(B, cap_a), So = dc_open_splits(B);
            static const int sub_stats = dev_env_int("ORYON_DC_SUB_STATS", 0);     // stats[3] = the halves' widths (sweeps: the sub-bands' share)
            // (1) probe: every stride-th anchor, read in place as one list panel per pair, screened completely; triples and bands
            //     (rows 0, stride, 2 stride, ..: <= MX6_SAMPLED_PANEL of them, stride >= cap_a / 512; the screen forms the list's length
            //     from n_a itself, as match_dc_probe_band_kernel does: dc_n_probe keeps its room, unwritten)
            launch_screen_mx6_list512(st, a6, q6, B, cap_a, MX6_SAMPLED_PANEL, cap_q, m.n_a, nullptr, 0, stride, m.n_q, csS, w.cs_max, w.cs_i1,
                                      w.cs_m2, m.C_true);
            hipLaunchKernelGGL(match_dc_probe_band_kernel, dim3(T8, B), dim3(256), 0, st, cap_a, T8, stride, csS, m.n_a, m.n_q, w.cs_max, w.cs_i1,
                               w.cs_m2, m.a_scale, m.q_eps_max, cut0, w.dc_m1, w.dc_i1, w.dc_m2, w.dc_band, w.dc_stats, DC_SLACK, sub_stats);
            // (2) band pass over all rows, each 512-row half in its own sub-band, (3) classes, merged triples, ordered list of the open rows
            launch_screen_mx6_band512(st, a6, q6, B, cap_a, cap_q, m.n_a, m.n_q, Sb, w.dc_ws_m1, w.dc_ws_i1, w.dc_ws_m2, m.C_true, w.dc_band, 2 * T8);
            hipLaunchKernelGGL(match_dc_settle_rows_kernel, dim3(B), dim3(DC_SETTLE_THREADS), 0, st, cap_a, T8, stride, Sb, m.n_a, m.n_q, w.dc_ws_m1, w.dc_ws_i1,
                               w.dc_ws_m2, m.a_scale, m.q_eps_max, cut0, w.dc_band, w.dc_m1, w.dc_i1, w.dc_m2, w.dc_cls, w.dc_n_open, w.dc_open_idx,
                               w.dc_stats);
            // (4) complete scan of the open rows in 512-row list panels, read in place through open_idx (count-gated); their triples are
            //     merged by the decide pass.  dc_rows keeps its room, unused
            launch_screen_mx6_list512(st, a6, q6, B, cap_a, cap_a, cap_q, w.dc_n_open, w.dc_open_idx, cap_a, 0, m.n_q, So, w.dc_ws_m1, w.dc_ws_i1,
                                      w.dc_ws_m2, m.C_true);
            S_dec = 1;                                                      // .. or the rows' merged ones; the open rows' So triples are
            dec_m1 = w.dc_m1; dec_i1 = w.dc_i1; dec_m2 = w.dc_m2;           //    merged by the decide pass itself, from their list slots
            dc_open.cls = w.dc_cls;
            dc_open.S = So;
            dc_open.m1 = w.dc_ws_m1; dc_open.i1 = w.dc_ws_i1; dc_open.m2 = w.dc_ws_m2;
            dc_open.r_m1 = w.dc_m1; dc_open.r_i1 = w.dc_i1; dc_open.r_m2 = w.dc_m2;
        } else {
            launch_screen_mx6(C, groups, T, st, a6, q6, B, cap_a, cap_q, m.n_a, m.n_q, S, w.ws_max, w.ws_i1, w.ws_m2, m.C_true);
        }
        profile_end(st);
    } else {
        screen8_step(m, S, m.n_a, w);
    }
    ORYON_CHECK_LAUNCH();
    hipLaunchKernelGGL(match_decide_lite_kernel, dim3(cap_a / 256, B), dim3(256), 0, st, cap_a, m.n_a, S_dec, dec_m1, dec_i1, dec_m2, dc_open, m.a_scale,
                       m.q_eps_max, cut0, sqrtf((float)m.C_true), (float)m.C_true, m.force_eager, m.fmt, use_x3, w.m_final, w.sid_final, w.margin,
                       w.state, m.valid, m.min_dist, m.argmin, w.pair_eager, w.n_unc, w.unc_idx, w.n_ambu, w.ambu_idx, w.need_f32_lazy,
                       w.n_amb_part);
    if (m.force_eager)      // n_a_eager / n_a_lazy: read by eager_route alone
        hipLaunchKernelGGL(match_mask_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, m.n_a, w.pair_eager, w.n_a_eager, w.n_a_lazy);
    ORYON_CHECK_LAUNCH();
    if (!m.force_eager) return lazy_route(m, w, st, use_x3, cascade || dc, dc);
    const int rc = eager_route(m, w, S);
    if (rc) return rc;
    if (m.n_undecided) ORYON_CHECK_HIP(hipMemcpyAsync(m.n_undecided, w.n_amb, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return ORYON_OK;
}

// ------------------------------------------------------------------------------------------------ C entries
// Each keeps its own argument check, names its operands in a MatchCorrsArgs and calls the one implementation.
namespace {
// the arguments all six entries have, under these names and in this order; the operands that differ by entry are set by name there
MatchCorrsArgs shared_args(const float *feat_q, int C_true, int HW, int layout, const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q,
                           int roi_stride_q, const float *q_norm, int B, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q,
                           float threshold, int W, int max_corrs, int corr_rows, uint64_t seed, const int64_t *pair_key, float *min_dist,
                           int32_t *argmin, uint8_t *valid, int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status,
                           int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes, void *stream)
{
    MatchCorrsArgs m;
    m.feat_q = feat_q;
    m.C_true = C_true;
    m.HW = HW;
    m.layout = layout;
    m.roi_a = roi_a;
    m.roi_stride_a = roi_stride_a;
    m.roi_q = roi_q;
    m.roi_stride_q = roi_stride_q;
    m.q_norm = q_norm;
    m.B = B;
    m.C = C;
    m.cap_a = cap_a;
    m.cap_q = cap_q;
    m.n_a = n_a;
    m.n_q = n_q;
    m.threshold = threshold;
    m.W = W;
    m.max_corrs = max_corrs;
    m.corr_rows = corr_rows;
    m.seed = seed;
    m.pair_key = pair_key;
    m.min_dist = min_dist;
    m.argmin = argmin;
    m.valid = valid;
    m.corrs = corrs;
    m.n_valid = n_valid;
    m.n_sel = n_sel;
    m.status = status;
    m.n_undecided = n_undecided;
    m.round_f16 = round_f16;
    m.workspace = workspace;
    m.workspace_bytes = workspace_bytes;
    m.stream = stream;
    return m;
}
}  // namespace

extern "C" int oryon_match_corrs_i8(const float *a_hat, const int8_t *a_i8, const float *a_scale, const float *feat_q, int C_true, int HW,
                                    int layout, const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q, int roi_stride_q,
                                    const float *q_norm, const int8_t *q_i8, const float *q_scale, const float *q_eps_max, int B, int C,
                                    int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, int W, int max_corrs,
                                    int corr_rows, uint64_t seed, const int64_t *pair_key, int force_eager, float *min_dist,
                                    int32_t *argmin, uint8_t *valid, int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status,
                                    int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(a_scale && q_scale);
    MatchCorrsArgs m = shared_args(feat_q, C_true, HW, layout, roi_a, roi_stride_a, roi_q, roi_stride_q, q_norm, B, C, cap_a, cap_q, n_a, n_q,
                                   threshold, W, max_corrs, corr_rows, seed, pair_key, min_dist, argmin, valid, corrs, n_valid, n_sel, status,
                                   n_undecided, round_f16, workspace, workspace_bytes, stream);
    m.a_hat = a_hat;
    m.a_i8 = a_i8;
    m.a_scale = a_scale;
    m.q_i8 = q_i8;
    m.q_scale = q_scale;
    m.q_eps_max = q_eps_max;
    m.force_eager = force_eager;
    return match_corrs_lazy_impl(m);
}

extern "C" int oryon_match_corrs_mx6(const float *a_hat, const uint8_t *a_mx6, const float *a_err_max, const float *feat_q, int C_true, int HW,
                                     int layout, const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q, int roi_stride_q,
                                     const float *q_norm, const uint8_t *q_mx6, const float *q_err_max, int B, int C, int cap_a, int cap_q,
                                     const int32_t *n_a, const int32_t *n_q, float threshold, int W, int max_corrs, int corr_rows,
                                     uint64_t seed, const int64_t *pair_key, float *min_dist, int32_t *argmin, uint8_t *valid,
                                     int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status, int32_t *n_undecided, int round_f16,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(a_err_max && q_err_max);
    MatchCorrsArgs m = shared_args(feat_q, C_true, HW, layout, roi_a, roi_stride_a, roi_q, roi_stride_q, q_norm, B, C, cap_a, cap_q, n_a, n_q,
                                   threshold, W, max_corrs, corr_rows, seed, pair_key, min_dist, argmin, valid, corrs, n_valid, n_sel, status,
                                   n_undecided, round_f16, workspace, workspace_bytes, stream);
    m.a_hat = a_hat;
    m.fmt = 1;
    m.a_i8 = reinterpret_cast<const int8_t *>(a_mx6);
    m.a_scale = a_err_max;
    m.q_i8 = reinterpret_cast<const int8_t *>(q_mx6);
    m.q_eps_max = q_err_max;
    return match_corrs_lazy_impl(m);
}

extern "C" int oryon_match_corrs_mx6_x3(const float *a_hat, const uint8_t *a_mx6, const float *a_err_max, const float *feat_q, int C_true, int HW,
                                        int layout, const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q, int roi_stride_q,
                                        const float *q_norm, const uint8_t *q_mx6, const float *q_err_max, const void *q_hi_lo_f16,
                                        const float *q_lo_sq_max, int B, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q,
                                        float threshold, int W, int max_corrs, int corr_rows, uint64_t seed, const int64_t *pair_key,
                                        float *min_dist, int32_t *argmin, uint8_t *valid, int32_t *corrs, int32_t *n_valid, int32_t *n_sel,
                                        int32_t *status, int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes,
                                        void *stream)
{
    ORYON_CHECK_ARG(a_err_max && q_err_max && q_hi_lo_f16 && q_lo_sq_max && C == 256);
    MatchCorrsArgs m = shared_args(feat_q, C_true, HW, layout, roi_a, roi_stride_a, roi_q, roi_stride_q, q_norm, B, C, cap_a, cap_q, n_a, n_q,
                                   threshold, W, max_corrs, corr_rows, seed, pair_key, min_dist, argmin, valid, corrs, n_valid, n_sel, status,
                                   n_undecided, round_f16, workspace, workspace_bytes, stream);
    m.a_hat = a_hat;
    m.fmt = 1;
    m.a_i8 = reinterpret_cast<const int8_t *>(a_mx6);
    m.a_scale = a_err_max;
    m.q_i8 = reinterpret_cast<const int8_t *>(q_mx6);
    m.q_eps_max = q_err_max;
    m.q_hi_lo = q_hi_lo_f16;
    m.q_lo_sq_max = q_lo_sq_max;
    return match_corrs_lazy_impl(m);
}

// ---- the same three entries WITHOUT materialised fp32 anchor rows: feat_a / a_norm (K0's row_norm of the anchor pass) in place of a_hat.
// The few rows the lazy tail needs are formed on demand (AnchorRaw above).  Lazy route only: the eager tail (force_eager of
// oryon_match_corrs_i8) reads whole pairs of rows and stays with the materialised ones.
extern "C" int oryon_match_corrs_i8_araw(const float *feat_a, const float *a_norm, const int8_t *a_i8, const float *a_scale, const float *feat_q,
                                         int C_true, int HW, int layout, const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q,
                                         int roi_stride_q, const float *q_norm, const int8_t *q_i8, const float *q_scale, const float *q_eps_max,
                                         int B, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, int W,
                                         int max_corrs, int corr_rows, uint64_t seed, const int64_t *pair_key, float *min_dist, int32_t *argmin,
                                         uint8_t *valid, int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status,
                                         int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(feat_a && a_norm && a_scale && q_scale);
    MatchCorrsArgs m = shared_args(feat_q, C_true, HW, layout, roi_a, roi_stride_a, roi_q, roi_stride_q, q_norm, B, C, cap_a, cap_q, n_a, n_q,
                                   threshold, W, max_corrs, corr_rows, seed, pair_key, min_dist, argmin, valid, corrs, n_valid, n_sel, status,
                                   n_undecided, round_f16, workspace, workspace_bytes, stream);
    m.feat_a = feat_a;
    m.a_norm = a_norm;
    m.a_i8 = a_i8;
    m.a_scale = a_scale;
    m.q_i8 = q_i8;
    m.q_scale = q_scale;
    m.q_eps_max = q_eps_max;
    return match_corrs_lazy_impl(m);
}

extern "C" int oryon_match_corrs_mx6_araw(const float *feat_a, const float *a_norm, const uint8_t *a_mx6, const float *a_err_max,
                                          const float *feat_q, int C_true, int HW, int layout, const int32_t *roi_a, int roi_stride_a,
                                          const int32_t *roi_q, int roi_stride_q, const float *q_norm, const uint8_t *q_mx6, const float *q_err_max,
                                          int B, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, int W,
                                          int max_corrs, int corr_rows, uint64_t seed, const int64_t *pair_key, float *min_dist, int32_t *argmin,
                                          uint8_t *valid, int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status, int32_t *n_undecided,
                                          int round_f16, void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(feat_a && a_norm && a_err_max && q_err_max);
    MatchCorrsArgs m = shared_args(feat_q, C_true, HW, layout, roi_a, roi_stride_a, roi_q, roi_stride_q, q_norm, B, C, cap_a, cap_q, n_a, n_q,
                                   threshold, W, max_corrs, corr_rows, seed, pair_key, min_dist, argmin, valid, corrs, n_valid, n_sel, status,
                                   n_undecided, round_f16, workspace, workspace_bytes, stream);
    m.feat_a = feat_a;
    m.a_norm = a_norm;
    m.fmt = 1;
    m.a_i8 = reinterpret_cast<const int8_t *>(a_mx6);
    m.a_scale = a_err_max;
    m.q_i8 = reinterpret_cast<const int8_t *>(q_mx6);
    m.q_eps_max = q_err_max;
    return match_corrs_lazy_impl(m);
}

extern "C" int oryon_match_corrs_mx6_x3_araw(const float *feat_a, const float *a_norm, const uint8_t *a_mx6, const float *a_err_max,
                                             const float *feat_q, int C_true, int HW, int layout, const int32_t *roi_a, int roi_stride_a,
                                             const int32_t *roi_q, int roi_stride_q, const float *q_norm, const uint8_t *q_mx6,
                                             const float *q_err_max, const void *q_hi_lo_f16, const float *q_lo_sq_max, int B, int C, int cap_a,
                                             int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, int W, int max_corrs,
                                             int corr_rows, uint64_t seed, const int64_t *pair_key, float *min_dist, int32_t *argmin,
                                             uint8_t *valid, int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status,
                                             int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(feat_a && a_norm && a_err_max && q_err_max && q_hi_lo_f16 && q_lo_sq_max && C == 256);
    MatchCorrsArgs m = shared_args(feat_q, C_true, HW, layout, roi_a, roi_stride_a, roi_q, roi_stride_q, q_norm, B, C, cap_a, cap_q, n_a, n_q,
                                   threshold, W, max_corrs, corr_rows, seed, pair_key, min_dist, argmin, valid, corrs, n_valid, n_sel, status,
                                   n_undecided, round_f16, workspace, workspace_bytes, stream);
    m.feat_a = feat_a;
    m.a_norm = a_norm;
    m.fmt = 1;
    m.a_i8 = reinterpret_cast<const int8_t *>(a_mx6);
    m.a_scale = a_err_max;
    m.q_i8 = reinterpret_cast<const int8_t *>(q_mx6);
    m.q_eps_max = q_err_max;
    m.q_hi_lo = q_hi_lo_f16;
    m.q_lo_sq_max = q_lo_sq_max;
    return match_corrs_lazy_impl(m);
}
