// ICP pose refinement of B pairs of object clouds (test.refine = icp): the reference's utils/geo6d.py:157-208 `icp` over
// nearest_neighbor (:22-38, sklearn) and best_fit_transform_icp (:122-155), batched, with nothing read back between iterations.
//
// The arithmetic is DEFINED (include/oryon_hip.h, oryon_icp_refine; DESIGN.md "ICP refinement"; tests/icp_restatement.py is its numpy
// statement): float64 without contraction.  Per pair, state T_k (T_0 = the solver's fp32 pose, widened), prev = 0; per iteration
//   move      s_i = ((R0 x + R1 y) + R2 z) + t per coordinate, [R | t] of T_k
//   nearest   d2_ij = ((dx dx + dy dy) + dz dz), j ascending, strict <: the first minimiser; dist_i = sqrt(d2_i)
//   keep      rows with a neighbour and dist_i <= max_dist; m of them.  m < 3: the pair is done, T_k stays
//   fit       dT = best_fit_transform_icp(s_kept, dst[j]_kept): plain means, H = sum (s - c_s)(d - c_d)^T,
//             R = V diag(1, 1, det(V U^T)) U^T (kabsch.h), t = c_d - R c_s
//   update    T_{k+1} = dT T_k; done when |prev - mean(dist_kept)| < tolerance (this update applied), else prev = mean
// The state, the FIXED order of the sums over rows (no float atomics: every output is bit-stable across runs, streams and batch
// position), the done flag and the end of an update are icp_common.h's, shared with icp_plane.hip.
//
// Two launches per iteration, all max_iter iterations enqueued by the host.  A pair that is done has its workgroups return at once.
#include "icp_common.h"                  // first: kabsch.h stays under the default contraction
#include "nn_tile.h"

namespace oryon {

constexpr int ICP_REC = 17;                  // a partial record: sum s' [3] | sum d' [3] | sum s' d'^T [9] | sum dist | count
static_assert(ICP_WAVES * ICP_REC <= 3 * NN_TILE, "the waves' records reuse the tile");

// One wave per pair: the done flag of pairs that do not start, the origin (lane-strided sums, xor butterfly: a fixed order) and
// icp_init_tail.  origin: the target's centroid - the moments are accumulated about it (s' = s - origin, d' = d - origin), so that
// H = sum s' d'^T - m c_s' c_d'^T does not cancel at coordinates around 1 m with a spread of around 5 cm.
__global__ __launch_bounds__(64) void icp_init_kernel(const double *__restrict__ dst, const int32_t *__restrict__ n_src, int cap_src,
                                                      const int32_t *__restrict__ n_dst, int cap_dst, const float *__restrict__ T_init,
                                                      const int32_t *__restrict__ status_in, IcpState *__restrict__ state, float *__restrict__ T,
                                                      double *__restrict__ T64, int32_t *__restrict__ iters, double *__restrict__ mean_err,
                                                      int32_t *__restrict__ n_kept, int32_t *__restrict__ idx, int32_t *__restrict__ status_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int ns = icp_count(n_src, b, cap_src), nd = icp_count(n_dst, b, cap_dst);
    const int st = status_in ? status_in[b] : 0;
    const bool done = st != 0 || ns < 3 || nd == 0;
    double o[3] = {0.0, 0.0, 0.0};
    if (!done) {
        const double *Q = dst + (size_t)b * cap_dst * 3;
        for (int j = lane; j < nd; j += 64) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double q = Q[(size_t)j * 3 + c];
                o[c] += isfinite(q) ? q : 0.0;               // any finite origin near the cloud serves; a NaN row must not poison it
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = wave_sum(o[c]) / (double)nd;
    }
    icp_init_tail(b, lane, cap_src, done, st, o, T_init, state, T, T64, iters, mean_err, n_kept, idx, status_out);
}

// grid (row blocks, B).  A workgroup moves its ICP_THREADS source rows by T_k once, into registers, walks the pair's target cloud
// (nearest_walk_f64) and reduces its kept rows to one record of ICP_REC sums, partials [B, n_blocks, ICP_REC].  A block past the pair's
// rows writes nothing (icp_update_kernel reads the blocks below ceil(n_src / ICP_THREADS) only).
// PAIRED (oryon_icp_best_fit): no walk - row i's neighbour is row i of dst, the correspondences are the caller's.
template <bool PAIRED>
__global__ __launch_bounds__(ICP_THREADS) void icp_nearest_kernel(const double *__restrict__ src, const int32_t *__restrict__ n_src, int cap_src,
                                                                  const double *__restrict__ dst, const int32_t *__restrict__ n_dst, int cap_dst,
                                                                  const IcpState *__restrict__ state, double max_dist,
                                                                  double *__restrict__ partials, int32_t *__restrict__ idx)
{
    extern __shared__ __align__(16) double icp_tile[];       // [3][NN_TILE]: x | y | z; afterwards the waves' records
    const int b = blockIdx.y;
    const IcpState &S = state[b];
    if (S.done) return;                                      // read once, before any barrier; nothing writes it during this launch: uniform
    const int ns = icp_count(n_src, b, cap_src), nd = icp_count(n_dst, b, cap_dst);
    const int row0 = blockIdx.x * ICP_THREADS;
    if (row0 >= ns) return;                                  // uniform over the workgroup
    const double *A = src + (size_t)b * cap_src * 3, *Q = dst + (size_t)b * cap_dst * 3;
    const int r = row0 + (int)threadIdx.x;
    const bool live = r < ns;                                // rows beyond n are never read
    const double x = live ? A[(size_t)r * 3 + 0] : 0.0, y = live ? A[(size_t)r * 3 + 1] : 0.0, z = live ? A[(size_t)r * 3 + 2] : 0.0;
    const double *T = S.T;
    const double ax[1] = {icp_move(T, x, y, z)}, ay[1] = {icp_move(T + 4, x, y, z)}, az[1] = {icp_move(T + 8, x, y, z)};
    double best[1];
    int bi[1];
    if (PAIRED) {
        bi[0] = live && r < nd ? r : -1;
        const int jr = max(bi[0], 0);
        const double dx = ax[0] - Q[(size_t)jr * 3 + 0], dy = ay[0] - Q[(size_t)jr * 3 + 1], dz = az[0] - Q[(size_t)jr * 3 + 2];
        best[0] = ((dx * dx + dy * dy) + dz * dz);
    } else {
        nearest_walk_f64<1, ICP_THREADS>(Q, nd, icp_tile, ax, ay, az, best, bi);
    }
    const int j = bi[0];
    if (live && idx) idx[(size_t)b * cap_src + r] = j;
    const double dist = sqrt(best[0]);
    const bool kept = live && j >= 0 && dist <= max_dist;    // a row whose every distance is NaN has no neighbour and is dropped
    double v[ICP_REC];
#pragma unroll
    for (int q = 0; q < ICP_REC; ++q) v[q] = 0.0;
    if (kept) {
        const double s[3] = {ax[0] - S.origin[0], ay[0] - S.origin[1], az[0] - S.origin[2]};
        const double d[3] = {Q[(size_t)j * 3 + 0] - S.origin[0], Q[(size_t)j * 3 + 1] - S.origin[1], Q[(size_t)j * 3 + 2] - S.origin[2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = s[c];
            v[3 + c] = d[c];
#pragma unroll
            for (int e = 0; e < 3; ++e) v[6 + c * 3 + e] = s[c] * d[e];
        }
        v[15] = dist;
        v[16] = 1.0;
    }
    __syncthreads();                                         // every wave has left the last tile
    icp_block_record<ICP_REC>(v, icp_tile, partials, b);
}

// One wave per pair: the records summed in ascending block order (lane q sums entry q), then lane 0 fits dT (kabsch.h), composes
// T_{k+1} = dT T_k, decides convergence and writes the pair's outputs.
__global__ __launch_bounds__(64) void icp_update_kernel(const int32_t *__restrict__ n_src, int cap_src, IcpState *__restrict__ state,
                                                        const double *__restrict__ partials, int n_blocks, int k, double tolerance,
                                                        float *__restrict__ T_out, double *__restrict__ T64, int32_t *__restrict__ iters,
                                                        double *__restrict__ mean_err, int32_t *__restrict__ n_kept)
{
    __shared__ double acc[ICP_REC];
    const int b = blockIdx.x;
    IcpState &S = state[b];
    if (S.done) return;                                      // uniform: only lane 0 writes it, after the barrier
    icp_sum_records<ICP_REC>(partials, b, n_blocks, n_src, cap_src, acc);
    if (threadIdx.x != 0) return;
    const double m = acc[16];
    if (n_kept) n_kept[b] = (int32_t)m;
    if (m < 3.0) {                                           // too few rows for a fit: T_k stays
        S.done = 1;
        return;
    }
    const double mean = acc[15] / m;
    double cs[3], cd[3], H[9], R[9], t[3], Tn[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) { cs[c] = acc[c] / m; cd[c] = acc[3 + c] / m; }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 3; ++e) H[c * 3 + e] = acc[6 + c * 3 + e] - acc[c] * cd[e];
    rotation_from_covariance(H, R);
#pragma unroll
    for (int c = 0; c < 3; ++c) { cs[c] += S.origin[c]; cd[c] += S.origin[c]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = cd[c] - ((R[c * 3] * cs[0] + R[c * 3 + 1] * cs[1]) + R[c * 3 + 2] * cs[2]);
    icp_compose(R, t, S.T, Tn);
    icp_commit(S, b, k, Tn, mean, tolerance, T_out, T64, iters, mean_err);
}

static inline bool icp_shape_ok(int B, int cap_src, int cap_dst)
{
    return B >= 1 && B <= 65535 && cap_src >= 1 && cap_src <= ICP_MAX_ROWS && cap_dst >= 1 && cap_dst <= ICP_MAX_ROWS;
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_icp_workspace_bytes(int B, int cap_src, int cap_dst)
{
    if (!icp_shape_ok(B, cap_src, cap_dst)) return 0;
    return icp_carve(nullptr, B, cap_src, ICP_REC).bytes;
}

// The launches of both entries.  paired: one iteration over the caller's correspondences.
static int icp_enqueue(const char *who, bool paired, const double *src, const int32_t *n_src, int cap_src, const double *dst, const int32_t *n_dst,
                       int cap_dst, int B, const float *T_init, int max_iter, double tolerance, double max_dist, const int32_t *status_in,
                       const IcpWorkspace &w, float *T, double *T64, int32_t *iters, double *mean_err, int32_t *n_kept, int32_t *idx,
                       int32_t *status_out, hipStream_t st)
{
    const int n_blocks = ceil_div(cap_src, ICP_THREADS);
    hipLaunchKernelGGL(icp_init_kernel, dim3(B), dim3(64), 0, st, dst, n_src, cap_src, n_dst, cap_dst, T_init, status_in, w.state, T, T64, iters,
                       mean_err, n_kept, idx, status_out);
    for (int k = 0; k < max_iter; ++k) {
        if (paired)
            hipLaunchKernelGGL(icp_nearest_kernel<true>, dim3(n_blocks, B), dim3(ICP_THREADS), NN_TILE_BYTES, st, src, n_src, cap_src, dst, n_dst,
                               cap_dst, w.state, max_dist, w.partials, idx);
        else
            hipLaunchKernelGGL(icp_nearest_kernel<false>, dim3(n_blocks, B), dim3(ICP_THREADS), NN_TILE_BYTES, st, src, n_src, cap_src, dst, n_dst,
                               cap_dst, w.state, max_dist, w.partials, idx);
        hipLaunchKernelGGL(icp_update_kernel, dim3(B), dim3(64), 0, st, n_src, cap_src, w.state, w.partials, n_blocks, k, tolerance, T, T64, iters,
                           mean_err, n_kept);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return ORYON_ERR_HIP;
    }
    return ORYON_OK;
}

extern "C" int oryon_icp_refine(const double *src, const int32_t *n_src, int cap_src, const double *dst, const int32_t *n_dst, int cap_dst,
                                int B, const float *T_init, int max_iter, double tolerance, double max_dist, const int32_t *status_in,
                                void *workspace, size_t workspace_bytes, float *T, double *T64, int32_t *iters, double *mean_err,
                                int32_t *n_kept, int32_t *idx, int32_t *status_out, void *stream)
{
    ORYON_CHECK_ARG(src && n_src && dst && n_dst && T_init && workspace);
    ORYON_CHECK_ARG(T && iters && mean_err && n_kept && status_out);                  // T64, idx and status_in may be NULL
    ORYON_CHECK_ARG(aligned8(src) && aligned8(dst) && aligned8(T64) && aligned8(mean_err));
    ORYON_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0);
    ORYON_CHECK_ARG(max_iter >= 1 && max_iter <= ICP_MAX_ITER);
    ORYON_CHECK_ARG(tolerance >= 0.0);                                                // NaN fails
    ORYON_CHECK_ARG(max_dist >= 0.0);                                                 // NaN fails; +inf keeps every row
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);
    ORYON_CHECK_ARG(cap_src >= 1 && cap_src <= ICP_MAX_ROWS && cap_dst >= 1 && cap_dst <= ICP_MAX_ROWS);
    if (B == 0) return ORYON_OK;
    const IcpWorkspace w = icp_carve(workspace, B, cap_src, ICP_REC);
    ORYON_CHECK_ARG(workspace_bytes >= w.bytes);
    return icp_enqueue(__func__, false, src, n_src, cap_src, dst, n_dst, cap_dst, B, T_init, max_iter, tolerance, max_dist, status_in, w, T, T64,
                       iters, mean_err, n_kept, idx, status_out, as_stream(stream));
}

extern "C" int oryon_icp_best_fit(const double *A, const double *Bp, const int32_t *n, int cap, int B, void *workspace, size_t workspace_bytes,
                                  float *T, double *T64, int32_t *fitted, double *mean_err, void *stream)
{
    ORYON_CHECK_ARG(A && Bp && n && workspace && T && fitted && mean_err);            // T64 may be NULL
    ORYON_CHECK_ARG(aligned8(A) && aligned8(Bp) && aligned8(T64) && aligned8(mean_err));
    ORYON_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0);
    ORYON_CHECK_ARG(B >= 0 && B <= 65535 && cap >= 1 && cap <= ICP_MAX_ROWS);
    if (B == 0) return ORYON_OK;
    const IcpWorkspace w = icp_carve(workspace, B, cap, ICP_REC);
    ORYON_CHECK_ARG(workspace_bytes >= w.bytes);
    return icp_enqueue(__func__, true, A, n, cap, Bp, n, cap, B, nullptr, 1, 0.0, __builtin_inf(), nullptr, w, T, T64, fitted, mean_err, nullptr,
                       nullptr, nullptr, as_stream(stream));
}
