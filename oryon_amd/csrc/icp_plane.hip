// Point-to-plane ICP of B source clouds onto the queries' DEPTH MAPS (test.refine = icp_plane): projective association - the neighbour of
// a moved source point is the pixel it projects to - and a point-to-plane error against the normal of that pixel, two central differences
// of the lifted map.  No search: an iteration is O(n) per pair, five gathered fp32 depth reads and one mask read per source row.  No
// vertex or normal map is stored (at 480 x 640 that would be 7 MB per pair): a row lifts the five pixels it needs.
//
// The arithmetic is DEFINED (include/oryon_hip.h, oryon_icp_plane_refine; DESIGN.md "Point-to-plane ICP on the depth map";
// tests/icp_plane_restatement.py is its numpy statement): float64 without contraction, + - * / sqrt and floor only.  Per pair, state T_k
// (T_0 = the solver's fp32 pose, widened), prev = 0, origin o = the mean of the source rows moved by T_0; per iteration
//   move       s = ((R0 x + R1 y) + R2 z) + t per coordinate, [R | t] of T_k; dropped unless s.z > 0
//   associate  u = (fx s.x) / s.z + cx, v alike, px = floor(u + 0.5), py = floor(v + 0.5); dropped unless 1 <= px <= W - 2,
//              1 <= py <= H - 2, mask[py, px] == 1 and depth[py, px] > 0
//   normal     the four neighbours have depth > 0 and |z_nb - z_c| <= normal_jump * 1000; a = V(px+1, py) - V(px-1, py),
//              b = V(px, py+1) - V(px, py-1), c = a x b, l = |c| > 0 and finite, n = c / l  (V: g1's lift, depth_lift.h)
//   gate       e = s - V(px, py), kept when |e| <= max_dist; m rows kept, m < 6: the pair is done, T_k stays
//   sums       r = n . e, J = [(s - o) x n, n]: A = sum J J^T (21 unique), g = sum J r (6), sum |r|, the count - 29 sums
//   solve      A x = -g by an unblocked Cholesky in a fixed order; a pivot not > 1e-12 max_i A_ii: the pair is done, T_k stays
//   update     R = Cayley(x[0:3]) (no sin, no cos), dT: p -> R (p - o) + o + x[3:6], T_{k+1} = dT T_k; done when
//              |prev - mean |r|| < tolerance (this update applied), else prev = mean |r|
// The state, the FIXED order of the sums over rows (no atomics: every output is bit-stable across runs, streams and batch position), the
// done flag and the end of an update are icp_common.h's, shared with icp.hip.
//
// Two launches per iteration, all max_iter iterations enqueued by the host, nothing read back.  A pair that is done has its workgroups
// return at once.
#include "icp_common.h"                  // first: kabsch.h stays under the default contraction
#include "depth_lift.h"

namespace oryon {

constexpr int ICPP_REC = 29;                 // a partial record: A's upper triangle, row-major [21] | g [6] | sum |r| | count
constexpr int ICPP_MIN_ROWS = 6;             // fewer kept rows than unknowns: no solve
static_assert(ICPP_REC == ORYON_ICP_PLANE_REC, "include/oryon_hip.h states the workspace formula");

// One wave per pair: the done flag of pairs that do not start, the origin (lane-strided sums, xor butterfly: a fixed order) and
// icp_init_tail.  origin: the mean of the source rows moved by T_0 - the 6 x 6 system is formed about it.
__global__ __launch_bounds__(64) void icp_plane_init_kernel(const double *__restrict__ src, const int32_t *__restrict__ n_src, int cap_src,
                                                            const float *__restrict__ T_init, const int32_t *__restrict__ status_in,
                                                            IcpState *__restrict__ state, float *__restrict__ T, double *__restrict__ T64,
                                                            int32_t *__restrict__ iters, double *__restrict__ mean_err,
                                                            int32_t *__restrict__ n_kept, int32_t *__restrict__ idx,
                                                            int32_t *__restrict__ status_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int ns = icp_count(n_src, b, cap_src);
    const int st = status_in ? status_in[b] : 0;
    const bool done = st != 0 || ns < ICPP_MIN_ROWS;
    double o[3] = {0.0, 0.0, 0.0};
    if (!done) {
        double T0[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) T0[q] = (double)T_init[(size_t)b * 16 + q];
        const double *A = src + (size_t)b * cap_src * 3;
        for (int i = lane; i < ns; i += 64) {
            const double x = A[(size_t)i * 3 + 0], y = A[(size_t)i * 3 + 1], z = A[(size_t)i * 3 + 2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double s = icp_move(T0 + c * 4, x, y, z);
                o[c] += isfinite(s) ? s : 0.0;               // any finite origin near the cloud serves; a NaN row must not poison it
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = wave_sum(o[c]) / (double)ns;
    }
    icp_init_tail(b, lane, cap_src, done, st, o, T_init, state, T, T64, iters, mean_err, n_kept, idx, status_out);
}

// grid (row blocks, B).  One source row per lane: moved by T_k, projected, tested, its pixel's normal formed from four lifted neighbours,
// gated, and its 29 products reduced with the workgroup's to one record, partials [B, n_blocks, ICPP_REC].  Every depth and mask read
// lies inside the map: px and py are tested against [1, W - 2] x [1, H - 2] in float64 BEFORE they become integers.  A block past the
// pair's rows writes nothing (icp_plane_update_kernel reads the blocks below ceil(n_src / ICP_THREADS) only).
__global__ __launch_bounds__(ICP_THREADS) void icp_plane_assoc_kernel(const double *__restrict__ src, const int32_t *__restrict__ n_src,
                                                                      int cap_src, const float *__restrict__ depth,
                                                                      const int32_t *__restrict__ mask, int H, int W,
                                                                      const double *__restrict__ cam9, const IcpState *__restrict__ state,
                                                                      double max_dist, double jump_mm, double *__restrict__ partials,
                                                                      int32_t *__restrict__ idx)
{
    __shared__ double rec[ICP_WAVES * ICPP_REC];
    const int b = blockIdx.y;
    const IcpState &S = state[b];
    if (S.done) return;                                      // nothing writes it during this launch: uniform
    const int ns = icp_count(n_src, b, cap_src);
    const int row0 = blockIdx.x * ICP_THREADS;
    if (row0 >= ns) return;                                  // uniform over the workgroup
    const int r = row0 + (int)threadIdx.x;
    const bool live = r < ns;                                // rows beyond n are never read
    const double *A = src + (size_t)b * cap_src * 3;
    const double x = live ? A[(size_t)r * 3 + 0] : 0.0, y = live ? A[(size_t)r * 3 + 1] : 0.0, z = live ? A[(size_t)r * 3 + 2] : 0.0;
    const double *T = S.T;
    const double s[3] = {icp_move(T, x, y, z), icp_move(T + 4, x, y, z), icp_move(T + 8, x, y, z)};
    const double *K = cam9 + (size_t)b * 9;
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    const float cxf = (float)cx, cyf = (float)cy;
    const float *D = depth + (size_t)b * H * W;
    const int32_t *M = mask + (size_t)b * H * W;

    bool kept = live && s[2] > 0.0;                          // a NaN row fails here
    int pix = -1;
    double v[ICPP_REC];
#pragma unroll
    for (int q = 0; q < ICPP_REC; ++q) v[q] = 0.0;
    if (kept) {
        double fpx, fpy;
        icp_project(s, fx, cx, fy, cy, fpx, fpy);
        kept = fpx >= 1.0 && fpx <= (double)(W - 2) && fpy >= 1.0 && fpy <= (double)(H - 2);      // NaN and inf fail
        if (kept) {
            const int px = (int)fpx, py = (int)fpy, p = py * W + px;
            const double zc = (double)D[p];
            kept = M[p] == 1 && zc > 0.0;
            if (kept) {
                const double zxp = (double)D[p + 1], zxm = (double)D[p - 1], zyp = (double)D[p + W], zym = (double)D[p - W];
                kept = zxp > 0.0 && zxm > 0.0 && zyp > 0.0 && zym > 0.0 && fabs(zxp - zc) <= jump_mm && fabs(zxm - zc) <= jump_mm &&
                       fabs(zyp - zc) <= jump_mm && fabs(zym - zc) <= jump_mm;
                if (kept) {
                    double vxp[3], vxm[3], vyp[3], vym[3], d[3];
                    depth_lift_f64(px + 1, py, zxp, fx, cxf, fy, cyf, vxp);
                    depth_lift_f64(px - 1, py, zxm, fx, cxf, fy, cyf, vxm);
                    depth_lift_f64(px, py + 1, zyp, fx, cxf, fy, cyf, vyp);
                    depth_lift_f64(px, py - 1, zym, fx, cxf, fy, cyf, vym);
                    depth_lift_f64(px, py, zc, fx, cxf, fy, cyf, d);
                    const double a[3] = {vxp[0] - vxm[0], vxp[1] - vxm[1], vxp[2] - vxm[2]};
                    const double bb[3] = {vyp[0] - vym[0], vyp[1] - vym[1], vyp[2] - vym[2]};
                    const double c[3] = {a[1] * bb[2] - a[2] * bb[1], a[2] * bb[0] - a[0] * bb[2], a[0] * bb[1] - a[1] * bb[0]};
                    const double l = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
                    const double e[3] = {s[0] - d[0], s[1] - d[1], s[2] - d[2]};
                    const double dist = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
                    kept = l > 0.0 && isfinite(l) && dist <= max_dist;
                    if (kept) {
                        const double n[3] = {c[0] / l, c[1] / l, c[2] / l};
                        const double res = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
                        const double q[3] = {s[0] - S.origin[0], s[1] - S.origin[1], s[2] - S.origin[2]};
                        const double J[6] = {q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0], n[0], n[1], n[2]};
                        int at = 0;
#pragma unroll
                        for (int i = 0; i < 6; ++i)
#pragma unroll
                            for (int j = i; j < 6; ++j) v[at++] = J[i] * J[j];
#pragma unroll
                        for (int i = 0; i < 6; ++i) v[21 + i] = J[i] * res;
                        v[27] = fabs(res);
                        v[28] = 1.0;
                        pix = p;
                    }
                }
            }
        }
    }
    if (live && idx) idx[(size_t)b * cap_src + r] = pix;
    icp_block_record<ICPP_REC>(v, rec, partials, b);
}

// the record's index of A[i][j], i <= j: the upper triangle, row-major
__host__ __device__ constexpr int icpp_at(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }
static_assert(icpp_at(0, 0) == 0 && icpp_at(1, 1) == 6 && icpp_at(5, 5) == 20, "21 entries");

// One wave per pair: the records summed in ascending block order (lane q sums entry q), then lane 0 solves the 6 x 6 system, composes
// T_{k+1} = dT T_k, decides convergence and writes the pair's outputs.
__global__ __launch_bounds__(64) void icp_plane_update_kernel(const int32_t *__restrict__ n_src, int cap_src, IcpState *__restrict__ state,
                                                              const double *__restrict__ partials, int n_blocks, int k, double tolerance,
                                                              float *__restrict__ T_out, double *__restrict__ T64, int32_t *__restrict__ iters,
                                                              double *__restrict__ mean_err, int32_t *__restrict__ n_kept)
{
    __shared__ double acc[ICPP_REC];
    const int b = blockIdx.x;
    IcpState &S = state[b];
    if (S.done) return;                                      // uniform: only lane 0 writes it, after the barrier
    icp_sum_records<ICPP_REC>(partials, b, n_blocks, n_src, cap_src, acc);
    if (threadIdx.x != 0) return;
    const double m = acc[28];
    n_kept[b] = (int32_t)m;
    if (m < (double)ICPP_MIN_ROWS) {                         // fewer rows than unknowns: T_k stays
        S.done = 1;
        return;
    }
    const double mean = acc[27] / m;
    // unblocked Cholesky A = L L^T, column by column; every index is a compile-time constant: registers, no scratch
    double top = acc[icpp_at(0, 0)];
#pragma unroll
    for (int i = 1; i < 6; ++i) top = fmax(top, acc[icpp_at(i, i)]);
    const double floor_ = 1e-12 * top;
    double L[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = acc[icpp_at(j, j)];
#pragma unroll
        for (int q = 0; q < j; ++q) d = d - L[j][q] * L[j][q];
        ok = ok && d > floor_;                               // a NaN pivot fails
        L[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double w = acc[icpp_at(j, i)];
#pragma unroll
            for (int q = 0; q < j; ++q) w = w - L[i][q] * L[j][q];
            L[i][j] = w / L[j][j];
        }
    }
    if (!ok) {                                               // the first failed pivot ends the pair; what followed it is discarded
        S.done = 1;
        return;
    }
    double yv[6], xv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double w = -acc[21 + i];
#pragma unroll
        for (int q = 0; q < i; ++q) w = w - L[i][q] * yv[q];
        yv[i] = w / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double w = yv[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) w = w - L[q][i] * xv[q];
        xv[i] = w / L[i][i];
    }
    // Cayley: R = I + 2 / (1 + a.a) ([a]x + [a]x^2), a = omega / 2, [a]x^2 = a a^T - (a.a) I
    const double a[3] = {xv[0] / 2.0, xv[1] / 2.0, xv[2] / 2.0};
    const double aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double f = 2.0 / (1.0 + aa);
    const double Kx[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
    double R[9], t[3], Tn[12];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double sq = a[i] * a[j] - (i == j ? aa : 0.0);
            R[i * 3 + j] = (i == j ? 1.0 : 0.0) + f * (Kx[i * 3 + j] + sq);
        }
    const double *o = S.origin;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                            // dT: p -> R (p - o) + o + x[3:6]
        const double Ro = (R[c * 3] * o[0] + R[c * 3 + 1] * o[1]) + R[c * 3 + 2] * o[2];
        t[c] = (o[c] - Ro) + xv[3 + c];
    }
    icp_compose(R, t, S.T, Tn);
    icp_commit(S, b, k, Tn, mean, tolerance, T_out, T64, iters, mean_err);
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_icp_plane_workspace_bytes(int B, int cap_src)
{
    if (!(B >= 1 && B <= 65535 && cap_src >= 1 && cap_src <= ICP_MAX_ROWS)) return 0;
    return icp_carve(nullptr, B, cap_src, ICPP_REC).bytes;
}

extern "C" int oryon_icp_plane_refine(const double *src, const int32_t *n_src, int cap_src, const float *depth, const int32_t *mask, int H, int W,
                                      const double *cam9, int B, const float *T_init, int max_iter, double tolerance, double max_dist,
                                      double normal_jump, const int32_t *status_in, void *workspace, size_t workspace_bytes, float *T,
                                      double *T64, int32_t *iters, double *mean_err, int32_t *n_kept, int32_t *idx, int32_t *status_out,
                                      void *stream)
{
    ORYON_CHECK_ARG(src && n_src && depth && mask && cam9 && T_init && workspace);
    ORYON_CHECK_ARG(T && iters && mean_err && n_kept && status_out);                  // T64, idx and status_in may be NULL
    ORYON_CHECK_ARG(aligned8(src) && aligned8(cam9) && aligned8(T64) && aligned8(mean_err));
    ORYON_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0);
    ORYON_CHECK_ARG(max_iter >= 1 && max_iter <= ICP_MAX_ITER);
    ORYON_CHECK_ARG(tolerance >= 0.0);                                                // NaN fails
    ORYON_CHECK_ARG(max_dist >= 0.0);                                                 // NaN fails; +inf keeps every associated row
    ORYON_CHECK_ARG(normal_jump >= 0.0);                                              // NaN fails; +inf accepts every step
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);
    ORYON_CHECK_ARG(cap_src >= 1 && cap_src <= ICP_MAX_ROWS);
    ORYON_CHECK_ARG(H >= 3 && W >= 3 && (long long)H * W < (1ll << 31));
    if (B == 0) return ORYON_OK;
    const IcpWorkspace w = icp_carve(workspace, B, cap_src, ICPP_REC);
    ORYON_CHECK_ARG(workspace_bytes >= w.bytes);
    hipStream_t st = as_stream(stream);
    const int n_blocks = ceil_div(cap_src, ICP_THREADS);
    const double jump_mm = normal_jump * 1000.0;
    hipLaunchKernelGGL(icp_plane_init_kernel, dim3(B), dim3(64), 0, st, src, n_src, cap_src, T_init, status_in, w.state, T, T64, iters, mean_err,
                       n_kept, idx, status_out);
    for (int k = 0; k < max_iter; ++k) {
        hipLaunchKernelGGL(icp_plane_assoc_kernel, dim3(n_blocks, B), dim3(ICP_THREADS), 0, st, src, n_src, cap_src, depth, mask, H, W, cam9,
                           w.state, max_dist, jump_mm, w.partials, idx);
        hipLaunchKernelGGL(icp_plane_update_kernel, dim3(B), dim3(64), 0, st, n_src, cap_src, w.state, w.partials, n_blocks, k, tolerance, T, T64,
                           iters, mean_err, n_kept);
    }
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
