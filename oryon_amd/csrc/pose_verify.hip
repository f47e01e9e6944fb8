// Depth-consistency verification of K candidate poses per pair (test.verify): every source row, moved by a candidate, projects into the
// query's depth map and is classified against the depth and the mask it finds there - behind the camera, outside the map, no depth,
// behind the measured surface, in front of it, on the surface beside the object, on the object - and the candidate with the most rows on
// the object is selected.  The access pattern is icp_plane.hip's projective association: no search, one gathered fp32 depth read and at
// most one mask read per row and candidate.
//
// The arithmetic is DEFINED (include/oryon_hip.h, oryon_pose_verify; DESIGN.md "Depth-consistency pose verification";
// tests/pose_verify_restatement.py is its numpy statement): float64 without contraction, + - * / and floor only, and no floating-point
// sum over rows at all - the counts are integers - so every output equals the statement's exactly.  The move and the projection are
// icp_common.h's, the very text icp_plane.hip compiles.
//
// Two launches, nothing read back, no atomics: a workgroup's class counts come from wave-wide ballots, the waves' counts are added
// through LDS in ascending order and one K x 7 int32 record per workgroup goes into the workspace; one wave per pair then sums the
// records in ascending block order, writes counts and applies the integer selection rule.  A pair with a failure status costs its
// workgroups the fill of their outputs (counts 0, cls -1, best 0) and nothing else.
#include "icp_common.h"                  // first, as the refiners do: everything from here on is compiled without contraction

namespace oryon {

constexpr int PV_CLASSES = ORYON_POSE_VERIFY_CLASSES;
constexpr int PV_MAX_POSES = ORYON_POSE_VERIFY_MAX_POSES;
enum : int { PV_BEHIND = 0, PV_OUTSIDE = 1, PV_UNKNOWN = 2, PV_OCCLUDED = 3, PV_VIOLATION = 4, PV_OFF = 5, PV_HIT = 6 };
static_assert(PV_CLASSES == 7 && PV_MAX_POSES * 12 <= ICP_THREADS && PV_MAX_POSES * PV_CLASSES <= ICP_THREADS, "one lane per staged number");

// grid (row blocks, B).  One source row per lane, loaded once and moved by each of the K candidates in turn; the candidates' twelve
// numbers each are staged in LDS, widened.  Every depth and mask read lies inside the map: px and py are tested against [0, W - 1] x
// [0, H - 1] in float64 BEFORE they become integers.  records [B, gridDim.x, K, 7]: a block past the pair's rows writes none
// (pose_verify_select_kernel reads the blocks below ceil(n_src / ICP_THREADS) only).  cls [B, K, cap_src] or NULL: every row below
// cap_src is written by the lane that owns it, -1 where the pair has no such row.
__global__ __launch_bounds__(ICP_THREADS) void pose_verify_classify_kernel(const double *__restrict__ src, const int32_t *__restrict__ n_src,
                                                                           int cap_src, const float *__restrict__ depth,
                                                                           const int32_t *__restrict__ mask, int H, int W,
                                                                           const double *__restrict__ cam9, const float *__restrict__ poses,
                                                                           int K, double tol, const int32_t *__restrict__ status_in,
                                                                           int32_t *__restrict__ records, int32_t *__restrict__ cls)
{
    __shared__ double Tk[PV_MAX_POSES * 12];
    __shared__ int32_t wave_counts[ICP_WAVES][PV_MAX_POSES * PV_CLASSES];
    const int b = blockIdx.y;
    const int row0 = blockIdx.x * ICP_THREADS;
    const int r = row0 + (int)threadIdx.x;
    const int ns = (status_in && status_in[b] != 0) ? 0 : icp_count(n_src, b, cap_src);       // a failed pair: no row is read
    if (row0 >= ns) {                                        // uniform over the workgroup: no record, cls = -1
        if (cls && r < cap_src)
            for (int k = 0; k < K; ++k) cls[((size_t)b * K + k) * cap_src + r] = -1;
        return;
    }
    if ((int)threadIdx.x < K * 12) {
        const int k = (int)threadIdx.x / 12, q = (int)threadIdx.x % 12;
        Tk[threadIdx.x] = (double)poses[((size_t)b * K + k) * 16 + q];
    }
    const bool live = r < ns;                                // rows beyond n are never read
    const double *A = src + (size_t)b * cap_src * 3;
    const double x = live ? A[(size_t)r * 3 + 0] : 0.0, y = live ? A[(size_t)r * 3 + 1] : 0.0, z = live ? A[(size_t)r * 3 + 2] : 0.0;
    const double *Kc = cam9 + (size_t)b * 9;
    const double fx = Kc[0], cx = Kc[2], fy = Kc[4], cy = Kc[5];
    const float *D = depth + (size_t)b * H * W;
    const int32_t *M = mask + (size_t)b * H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();

    for (int k = 0; k < K; ++k) {
        const double *T = Tk + k * 12;
        const double s[3] = {icp_move(T, x, y, z), icp_move(T + 4, x, y, z), icp_move(T + 8, x, y, z)};
        int c = PV_BEHIND;
        if (live && s[2] > 0.0) {                            // a NaN row fails here
            double fpx, fpy;
            icp_project(s, fx, cx, fy, cy, fpx, fpy);
            c = PV_OUTSIDE;
            if (fpx >= 0.0 && fpx <= (double)(W - 1) && fpy >= 0.0 && fpy <= (double)(H - 1)) {      // NaN and inf fail
                const int p = (int)fpy * W + (int)fpx;
                const float zf = D[p];
                c = PV_UNKNOWN;
                if (zf > 0.0f && zf < __builtin_huge_valf()) {
                    const double d = s[2] - (double)zf / 1000.0;
                    if (d > tol) c = PV_OCCLUDED;
                    else if (-d > tol) c = PV_VIOLATION;
                    else c = M[p] == 1 ? PV_HIT : PV_OFF;
                }
            }
        }
        if (cls && r < cap_src) cls[((size_t)b * K + k) * cap_src + r] = live ? c : -1;
#pragma unroll
        for (int q = 0; q < PV_CLASSES; ++q) {
            const int n = __popcll(__ballot(live && c == q));
            if (lane == 0) wave_counts[wave][k * PV_CLASSES + q] = n;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < K * PV_CLASSES) {
        int32_t a = wave_counts[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < ICP_WAVES; ++w) a += wave_counts[w][threadIdx.x];
        records[((size_t)b * gridDim.x + blockIdx.x) * (K * PV_CLASSES) + threadIdx.x] = a;
    }
}

// One wave per pair: the records of the blocks that hold rows summed in ascending order (integers: the order cannot matter, it is fixed
// all the same), counts written, and lane 0 applies the selection rule - most HITs, then fewest BEHIND + VIOLATION + OFF, then the
// smallest k.
__global__ __launch_bounds__(64) void pose_verify_select_kernel(const int32_t *__restrict__ n_src, int cap_src, int K, int n_blocks,
                                                                const int32_t *__restrict__ status_in, const int32_t *__restrict__ records,
                                                                int32_t *__restrict__ counts, int32_t *__restrict__ best)
{
    __shared__ int32_t tot[PV_MAX_POSES * PV_CLASSES];
    const int b = blockIdx.x;
    const int KC = K * PV_CLASSES;
    if (status_in && status_in[b] != 0) {                    // uniform: all counts 0, best 0
        for (int e = threadIdx.x; e < KC; e += 64) counts[(size_t)b * KC + e] = 0;
        if (threadIdx.x == 0) best[b] = 0;
        return;
    }
    const int used = (icp_count(n_src, b, cap_src) + ICP_THREADS - 1) / ICP_THREADS;
    for (int e = threadIdx.x; e < KC; e += 64) {
        int32_t a = 0;
        for (int blk = 0; blk < used; ++blk) a += records[((size_t)b * n_blocks + blk) * KC + e];
        tot[e] = a;
        counts[(size_t)b * KC + e] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int at = 0, hit = tot[PV_HIT], bad = tot[PV_BEHIND] + tot[PV_VIOLATION] + tot[PV_OFF];
    for (int k = 1; k < K; ++k) {
        const int32_t *t = tot + k * PV_CLASSES;
        const int h = t[PV_HIT], bd = t[PV_BEHIND] + t[PV_VIOLATION] + t[PV_OFF];
        if (h > hit || (h == hit && bd < bad)) {             // strictly better only: the smallest k wins a full tie
            at = k; hit = h; bad = bd;
        }
    }
    best[b] = at;
}

static size_t pose_verify_carve(void *workspace, int B, int cap_src, int K, int32_t *&records)
{
    Carver carve(workspace);
    carve(records, (size_t)B * ceil_div(cap_src, ICP_THREADS) * K * PV_CLASSES);
    return carve.off;
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_pose_verify_workspace_bytes(int B, int cap_src, int K)
{
    if (!(B >= 1 && B <= 65535 && cap_src >= 1 && cap_src <= ICP_MAX_ROWS && K >= 1 && K <= PV_MAX_POSES)) return 0;
    int32_t *records;
    return pose_verify_carve(nullptr, B, cap_src, K, records);
}

extern "C" int oryon_pose_verify(const double *src, const int32_t *n_src, int cap_src, const float *depth, const int32_t *mask, int H, int W,
                                 const double *cam9, int B, const float *poses, int K, double tol, const int32_t *status_in, void *workspace,
                                 size_t workspace_bytes, int32_t *counts, int32_t *best, int32_t *cls, void *stream)
{
    ORYON_CHECK_ARG(src && n_src && depth && mask && cam9 && poses);
    ORYON_CHECK_ARG(counts && best);                                                  // status_in and cls may be NULL
    ORYON_CHECK_ARG(aligned8(src) && aligned8(cam9));
    ORYON_CHECK_ARG(K >= 1 && K <= PV_MAX_POSES);
    ORYON_CHECK_ARG(tol >= 0.0);                                                      // NaN fails; +inf leaves OFF and HIT only
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);
    ORYON_CHECK_ARG(cap_src >= 1 && cap_src <= ICP_MAX_ROWS);
    ORYON_CHECK_ARG(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31));
    ORYON_CHECK_ARG(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0);
    if (B == 0) return ORYON_OK;
    int32_t *records;
    const size_t need = pose_verify_carve(workspace, B, cap_src, K, records);
    ORYON_CHECK_ARG(workspace_bytes >= need);
    hipStream_t st = as_stream(stream);
    const int n_blocks = ceil_div(cap_src, ICP_THREADS);
    hipLaunchKernelGGL(pose_verify_classify_kernel, dim3(n_blocks, B), dim3(ICP_THREADS), 0, st, src, n_src, cap_src, depth, mask, H, W, cam9,
                       poses, K, tol, status_in, records, cls);
    hipLaunchKernelGGL(pose_verify_select_kernel, dim3(B), dim3(64), 0, st, n_src, cap_src, K, n_blocks, status_in, records, counts, best);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
