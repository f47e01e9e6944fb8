// K1r: the ratio test with an exclusion disc.  For every anchor row i the best query row OUTSIDE a disc of `radius` pixels around the
// pixel of its nearest query row argmin[i] (K1's or K1m's output), and keep[i] = gate[i] && min_dist[i] <= ratio * second_dist[i]
// (include/oryon_hip.h has the definition).  radius 1 excludes the best pixel alone: Lowe's ratio test.
//
// The scan is match_disc.h's with ONE centre per anchor column, argmin's pixel; the fold, the kernels and the merge of the query splits
// are explained there.  This file's own:
//   * what a finished row turns into: second_dist, second_argmin (0 where no row is left) and keep, written by whichever launch
//     finishes the row: the scan when the shape is unsplit, the merge otherwise;
//   * the checks of min_dist, argmin, ratio and keep.
#include "common.h"
#include "match_common.h"
#include "match_tile.h"
#include "match_disc.h"

namespace oryon {

struct RatioOut {
    const float *min_dist;
    const uint8_t *gate;
    float ratio;
    float *second_dist;
    int32_t *second_argmin;
    uint8_t *keep;
    __device__ __forceinline__ void row(size_t o, float second, int sidx) const
    {
        second_dist[o] = second;
        second_argmin[o] = (sidx == ROW_NONE) ? 0 : sidx;
        keep[o] = ((!gate || gate[o]) && min_dist[o] <= __fmul_rn(ratio, second)) ? 1 : 0;
    }
};

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_match_second_workspace_bytes(int B, int cap_a)
{
    if (B <= 0 || cap_a <= 0) return 0;
    return match_disc_split_bytes(B, cap_a, 0);
}

extern "C" int oryon_match_second_f32(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q, const int32_t *n_a,
                                      const int32_t *n_q, const int32_t *roi_q, int roi_stride_q, int W_q, int radius,
                                      const float *min_dist, const int32_t *argmin, const uint8_t *gate, float ratio, float *second_dist,
                                      int32_t *second_argmin, uint8_t *keep, void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_DISC_ARGS(second_dist, second_argmin);
    ORYON_CHECK_ARG(min_dist && argmin);
    ORYON_CHECK_ARG(keep);
    ORYON_CHECK_ARG(ratio > 0.0f && ratio <= 1.0f);     // a NaN fails both
    if (B == 0) return ORYON_OK;
    const size_t need = match_disc_split_bytes(B, cap_a, 0);
    if (need) ORYON_CHECK_WORKSPACE("oryon_match_second_f32: ", workspace, workspace_bytes, need);
    const DiscArgs g = {a_hat, q_hat, B, C, cap_a, cap_q, n_a, n_q, roi_q, roi_stride_q, W_q, radius, argmin, 1};
    const RatioOut out = {min_dist, gate, ratio, second_dist, second_argmin, keep};
    const hipError_t e = match_disc_launch<1>(g, out, workspace, 0, as_stream(stream));
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", __func__, hipGetErrorString(e));
        return ORYON_ERR_HIP;
    }
    return ORYON_OK;
}
