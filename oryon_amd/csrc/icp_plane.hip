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
//              b = V(px, py+1) - V(px, py-1), c = a x b, l = |c| > 0 and finite, n = c / l  (V: g1's lift, csrc/gt_corrs.hip)
//   gate       e = s - V(px, py), kept when |e| <= max_dist; m rows kept, m < 6: the pair is done, T_k stays
//   sums       r = n . e, J = [(s - o) x n, n]: A = sum J J^T (21 unique), g = sum J r (6), sum |r|, the count - 29 sums
//   solve      A x = -g by an unblocked Cholesky in a fixed order; a pivot not > 1e-12 max_i A_ii: the pair is done, T_k stays
//   update     R = Cayley(x[0:3]) (no sin, no cos), dT: p -> R (p - o) + o + x[3:6], T_{k+1} = dT T_k; done when
//              |prev - mean |r|| < tolerance (this update applied), else prev = mean |r|
// The order of the sums over rows is not part of the definition but it is FIXED, as in icp.hip: a workgroup's rows are reduced by an xor
// butterfly inside each wave and over the waves in ascending order, the workgroups' records in ascending block order.  No atomics:
// every output is bit-stable across runs, streams and batch position.
//
// Two launches per iteration, all max_iter iterations enqueued by the host, nothing read back.  A pair that is done has its workgroups
// return at once.  No workgroup waits on another inside a launch: launch boundaries are the only cross-workgroup ordering.
#include "common.h"
#include "kabsch.h"

#pragma clang fp contract(off)

namespace oryon {

constexpr int ICPP_THREADS = 256;            // source rows of a workgroup, one per lane
constexpr int ICPP_WAVES = ICPP_THREADS / 64;
constexpr int ICPP_MAX_ROWS = ORYON_ICP_MAX_ROWS;
constexpr int ICPP_MAX_ITER = ORYON_ICP_MAX_ITER;
constexpr int ICPP_REC = 29;                 // a partial record: A's upper triangle, row-major [21] | g [6] | sum |r| | count
constexpr int ICPP_MIN_ROWS = 6;             // fewer kept rows than unknowns: no solve
static_assert(ICPP_REC == ORYON_ICP_PLANE_REC, "include/oryon_hip.h states the workspace formula");

struct IcpPlaneState {
    double T[12];                            // rows of [R | t] of T_k
    double prev;
    double origin[3];                        // the mean of the source rows moved by T_0: the 6 x 6 system is formed about it
    int32_t done, pad;
};
static_assert(sizeof(IcpPlaneState) == ORYON_ICP_STATE_BYTES, "include/oryon_hip.h states the workspace formula");

__device__ __forceinline__ int icpp_count(const int32_t *__restrict__ n, int b, int cap) { return max(0, min(n[b], cap)); }

// g1's lift (gt_corrs.hip): the pixel-minus-centre difference is an fp32 one
__device__ __forceinline__ void icpp_lift(int x, int y, double z, double fx, float cxf, double fy, float cyf, double v[3])
{
    const float dxf = (float)x - cxf, dyf = (float)y - cyf;
    v[0] = (((double)dxf * z) / fx) / 1000.0;
    v[1] = (((double)dyf * z) / fy) / 1000.0;
    v[2] = z / 1000.0;
}

// One wave per pair: T_0 widened (and written out, so a pair that never iterates returns it), the done flag of pairs that do not start,
// the origin (lane-strided sums of the rows moved by T_0, xor butterfly: a fixed order), idx = -1.
__global__ __launch_bounds__(64) void icp_plane_init_kernel(const double *__restrict__ src, const int32_t *__restrict__ n_src, int cap_src,
                                                            const float *__restrict__ T_init, const int32_t *__restrict__ status_in,
                                                            IcpPlaneState *__restrict__ state, float *__restrict__ T, double *__restrict__ T64,
                                                            int32_t *__restrict__ iters, double *__restrict__ mean_err,
                                                            int32_t *__restrict__ n_kept, int32_t *__restrict__ idx,
                                                            int32_t *__restrict__ status_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const int ns = icpp_count(n_src, b, cap_src);
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
                const double s = ((T0[c * 4] * x + T0[c * 4 + 1] * y) + T0[c * 4 + 2] * z) + T0[c * 4 + 3];
                o[c] += isfinite(s) ? s : 0.0;               // any finite origin near the cloud serves; a NaN row must not poison it
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = wave_sum(o[c]) / (double)ns;
    }
    if (idx)
        for (int i = lane; i < cap_src; i += 64) idx[(size_t)b * cap_src + i] = -1;
    if (lane < 16) {
        const float v = T_init[(size_t)b * 16 + lane];
        T[(size_t)b * 16 + lane] = v;                        // the last row stays T_init's
        if (lane < 12) {
            state[b].T[lane] = (double)v;
            if (T64) T64[(size_t)b * 12 + lane] = (double)v;
        }
    }
    if (lane == 0) {
        IcpPlaneState &S = state[b];
        S.prev = 0.0;
        S.origin[0] = o[0]; S.origin[1] = o[1]; S.origin[2] = o[2];
        S.done = done ? 1 : 0;
        S.pad = 0;
        iters[b] = 0;
        mean_err[b] = 0.0;
        n_kept[b] = 0;
        status_out[b] = st;
    }
}

// grid (row blocks, B).  One source row per lane: moved by T_k, projected, tested, its pixel's normal formed from four lifted neighbours,
// gated, and its 29 products reduced with the workgroup's to one record, partials [B, n_blocks, ICPP_REC].  Every depth and mask read
// lies inside the map: px and py are tested against [1, W - 2] x [1, H - 2] in float64 BEFORE they become integers.  A block past the
// pair's rows writes nothing (icp_plane_update_kernel reads the blocks below ceil(n_src / ICPP_THREADS) only).
__global__ __launch_bounds__(ICPP_THREADS) void icp_plane_assoc_kernel(const double *__restrict__ src, const int32_t *__restrict__ n_src,
                                                                       int cap_src, const float *__restrict__ depth,
                                                                       const int32_t *__restrict__ mask, int H, int W,
                                                                       const double *__restrict__ cam9, const IcpPlaneState *__restrict__ state,
                                                                       double max_dist, double jump_mm, double *__restrict__ partials,
                                                                       int32_t *__restrict__ idx)
{
    __shared__ double rec[ICPP_WAVES * ICPP_REC];
    const int b = blockIdx.y;
    const IcpPlaneState &S = state[b];
    if (S.done) return;                                      // nothing writes it during this launch: uniform
    const int ns = icpp_count(n_src, b, cap_src);
    const int row0 = blockIdx.x * ICPP_THREADS;
    if (row0 >= ns) return;                                  // uniform over the workgroup
    const int r = row0 + (int)threadIdx.x;
    const bool live = r < ns;                                // rows beyond n are never read
    const double *A = src + (size_t)b * cap_src * 3;
    const double x = live ? A[(size_t)r * 3 + 0] : 0.0, y = live ? A[(size_t)r * 3 + 1] : 0.0, z = live ? A[(size_t)r * 3 + 2] : 0.0;
    const double *T = S.T;
    const double s[3] = {((T[0] * x + T[1] * y) + T[2] * z) + T[3], ((T[4] * x + T[5] * y) + T[6] * z) + T[7],
                         ((T[8] * x + T[9] * y) + T[10] * z) + T[11]};
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
        const double u = (fx * s[0]) / s[2] + cx, w = (fy * s[1]) / s[2] + cy;
        const double fpx = floor(u + 0.5), fpy = floor(w + 0.5);
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
                    icpp_lift(px + 1, py, zxp, fx, cxf, fy, cyf, vxp);
                    icpp_lift(px - 1, py, zxm, fx, cxf, fy, cyf, vxm);
                    icpp_lift(px, py + 1, zyp, fx, cxf, fy, cyf, vyp);
                    icpp_lift(px, py - 1, zym, fx, cxf, fy, cyf, vym);
                    icpp_lift(px, py, zc, fx, cxf, fy, cyf, d);
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
#pragma unroll
    for (int q = 0; q < ICPP_REC; ++q) v[q] = wave_sum(v[q]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < ICPP_REC; ++q) rec[wave * ICPP_REC + q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < ICPP_REC) {
        double a = rec[threadIdx.x];
#pragma unroll
        for (int w = 1; w < ICPP_WAVES; ++w) a += rec[w * ICPP_REC + threadIdx.x];
        partials[((size_t)b * gridDim.x + blockIdx.x) * ICPP_REC + threadIdx.x] = a;
    }
}

// the record's index of A[i][j], i <= j: the upper triangle, row-major
__host__ __device__ constexpr int icpp_at(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }
static_assert(icpp_at(0, 0) == 0 && icpp_at(1, 1) == 6 && icpp_at(5, 5) == 20, "21 entries");

// One wave per pair: the records summed in ascending block order (lane q sums entry q), then lane 0 solves the 6 x 6 system, composes
// T_{k+1} = dT T_k, decides convergence and writes the pair's outputs.
__global__ __launch_bounds__(64) void icp_plane_update_kernel(const int32_t *__restrict__ n_src, int cap_src, IcpPlaneState *__restrict__ state,
                                                              const double *__restrict__ partials, int n_blocks, int k, double tolerance,
                                                              float *__restrict__ T_out, double *__restrict__ T64, int32_t *__restrict__ iters,
                                                              double *__restrict__ mean_err, int32_t *__restrict__ n_kept)
{
    __shared__ double acc[ICPP_REC];
    const int b = blockIdx.x;
    IcpPlaneState &S = state[b];
    if (S.done) return;                                      // uniform: only lane 0 writes it, after the barrier
    const int used = (icpp_count(n_src, b, cap_src) + ICPP_THREADS - 1) / ICPP_THREADS;
    if (threadIdx.x < ICPP_REC) {
        double a = 0.0;
        for (int blk = 0; blk < used; ++blk) a += partials[((size_t)b * n_blocks + blk) * ICPP_REC + threadIdx.x];
        acc[threadIdx.x] = a;
    }
    __syncthreads();
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
    double R[9], Tn[12];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double sq = a[i] * a[j] - (i == j ? aa : 0.0);
            R[i * 3 + j] = (i == j ? 1.0 : 0.0) + f * (Kx[i * 3 + j] + sq);
        }
    const double *o = S.origin;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) Tn[c * 4 + e] = (R[c * 3] * S.T[e] + R[c * 3 + 1] * S.T[4 + e]) + R[c * 3 + 2] * S.T[8 + e];
        const double Ro = (R[c * 3] * o[0] + R[c * 3 + 1] * o[1]) + R[c * 3 + 2] * o[2];
        Tn[c * 4 + 3] += (o[c] - Ro) + xv[3 + c];
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        S.T[q] = Tn[q];
        if (T64) T64[(size_t)b * 12 + q] = Tn[q];
        T_out[(size_t)b * 16 + q] = (float)Tn[q];
    }
    iters[b] = k + 1;
    mean_err[b] = mean;
    if (fabs(S.prev - mean) < tolerance) S.done = 1;
    else S.prev = mean;
}

static inline size_t icpp_align256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline bool icpp_aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

struct IcpPlaneWorkspace {
    IcpPlaneState *state;
    double *partials;
    size_t bytes;
};

static IcpPlaneWorkspace icpp_carve(void *workspace, int B, int cap_src)
{
    IcpPlaneWorkspace w;
    char *p = static_cast<char *>(workspace);
    size_t at = 0;
    auto take = [&](size_t n) { char *r = p ? p + at : nullptr; at += icpp_align256(n); return r; };
    w.state = reinterpret_cast<IcpPlaneState *>(take((size_t)B * sizeof(IcpPlaneState)));
    w.partials = reinterpret_cast<double *>(take((size_t)B * ceil_div(cap_src, ICPP_THREADS) * ICPP_REC * sizeof(double)));
    w.bytes = at;
    return w;
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_icp_plane_workspace_bytes(int B, int cap_src)
{
    if (!(B >= 1 && B <= 65535 && cap_src >= 1 && cap_src <= ICPP_MAX_ROWS)) return 0;
    return icpp_carve(nullptr, B, cap_src).bytes;
}

extern "C" int oryon_icp_plane_refine(const double *src, const int32_t *n_src, int cap_src, const float *depth, const int32_t *mask, int H, int W,
                                      const double *cam9, int B, const float *T_init, int max_iter, double tolerance, double max_dist,
                                      double normal_jump, const int32_t *status_in, void *workspace, size_t workspace_bytes, float *T,
                                      double *T64, int32_t *iters, double *mean_err, int32_t *n_kept, int32_t *idx, int32_t *status_out,
                                      void *stream)
{
    ORYON_CHECK_ARG(src && n_src && depth && mask && cam9 && T_init && workspace);
    ORYON_CHECK_ARG(T && iters && mean_err && n_kept && status_out);                  // T64, idx and status_in may be NULL
    ORYON_CHECK_ARG(icpp_aligned8(src) && icpp_aligned8(cam9) && icpp_aligned8(T64) && icpp_aligned8(mean_err));
    ORYON_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0);
    ORYON_CHECK_ARG(max_iter >= 1 && max_iter <= ICPP_MAX_ITER);
    ORYON_CHECK_ARG(tolerance >= 0.0);                                                // NaN fails
    ORYON_CHECK_ARG(max_dist >= 0.0);                                                 // NaN fails; +inf keeps every associated row
    ORYON_CHECK_ARG(normal_jump >= 0.0);                                              // NaN fails; +inf accepts every step
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);
    ORYON_CHECK_ARG(cap_src >= 1 && cap_src <= ICPP_MAX_ROWS);
    ORYON_CHECK_ARG(H >= 3 && W >= 3 && (long long)H * W < (1ll << 31));
    if (B == 0) return ORYON_OK;
    const IcpPlaneWorkspace w = icpp_carve(workspace, B, cap_src);
    ORYON_CHECK_ARG(workspace_bytes >= w.bytes);
    hipStream_t st = as_stream(stream);
    const int n_blocks = ceil_div(cap_src, ICPP_THREADS);
    const double jump_mm = normal_jump * 1000.0;
    hipLaunchKernelGGL(icp_plane_init_kernel, dim3(B), dim3(64), 0, st, src, n_src, cap_src, T_init, status_in, w.state, T, T64, iters, mean_err,
                       n_kept, idx, status_out);
    for (int k = 0; k < max_iter; ++k) {
        hipLaunchKernelGGL(icp_plane_assoc_kernel, dim3(n_blocks, B), dim3(ICPP_THREADS), 0, st, src, n_src, cap_src, depth, mask, H, W, cam9,
                           w.state, max_dist, jump_mm, w.partials, idx);
        hipLaunchKernelGGL(icp_plane_update_kernel, dim3(B), dim3(64), 0, st, n_src, cap_src, w.state, w.partials, n_blocks, k, tolerance, T, T64,
                           iters, mean_err, n_kept);
    }
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
