// K1n: one rank scan of the one-to-many matcher.  For every anchor row i the best query row OUTSIDE the discs of `radius` pixels round
// the pixels of up to three earlier ranks prev[0..n_prev)[i] (include/oryon_hip.h has the definition).  n_prev = 1 is K1r's second
// minimum; the K - 1 calls of oryon_topk_corrs (post.hip) walk the ranks 2..K of the DRAWN anchor rows.
//
// The scan is match_disc.h's with THREE centres per anchor column, whatever n_prev is (a centre that is not there excludes nothing); the
// fold, the kernels and the merge of the query splits are explained there.  This file's own:
//   * what a finished row turns into: the rank's (distance, index), with index -1 and INFINITY where no row is left; there is no keep;
//   * the checks of prev_argmin and n_prev;
//   * the launches without the checks, for oryon_topk_corrs.
#include "common.h"
#include "match_common.h"
#include "match_tile.h"
#include "match_disc.h"

namespace oryon {

constexpr int NEXT_PREV_MAX = 3;

struct RankOut {
    float *next_dist;
    int32_t *next_argmin;
    __device__ __forceinline__ void row(size_t o, float best, int bidx) const
    {
        next_dist[o] = best;
        next_argmin[o] = (bidx == ROW_NONE) ? -1 : bidx;
    }
};

size_t match_next_split_bytes(int B, int cap_a, size_t start) { return match_disc_split_bytes(B, cap_a, start); }

// the launches of one rank scan, arguments checked by the caller; split buffers carved from workspace at ws_start
int match_next_launch(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q,
                      const int32_t *roi_q, int roi_stride_q, int W_q, int radius, const int32_t *prev, int n_prev, float *next_dist,
                      int32_t *next_argmin, void *workspace, size_t ws_start, hipStream_t st)
{
    const DiscArgs g = {a_hat, q_hat, B, C, cap_a, cap_q, n_a, n_q, roi_q, roi_stride_q, W_q, radius, prev, n_prev};
    const RankOut out = {next_dist, next_argmin};
    return match_disc_launch<NEXT_PREV_MAX>(g, out, workspace, ws_start, st) == hipSuccess ? ORYON_OK : ORYON_ERR_HIP;
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
    ORYON_CHECK_DISC_ARGS(next_dist, next_argmin);
    ORYON_CHECK_ARG(prev_argmin);
    ORYON_CHECK_ARG(n_prev >= 1 && n_prev <= NEXT_PREV_MAX);
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
