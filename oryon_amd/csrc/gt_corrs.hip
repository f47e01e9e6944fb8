// Ground-truth correspondences of an RGB-D pair with known poses: lift the object's pixels of both views, move the anchor cloud into
// the query camera, find every anchor point's nearest query point (all pairs, float64) and keep the rows within a threshold.
// Replaces, for the fixed-split builder (oryon_amd/pairs.py, make_split.py):
//   utils/data/toyl.py:237-278 / utils/data/nocs.py  get_pcd + filter_pcd over utils/pcd.py:44-74 lift_pcd
//   scripts/data/make_toyl_test.py:31-45, :212-213    np_transform by pose_q @ inv(pose_a)
//   scripts/data/make_toyl_test.py:68-77              torch.cdist (20 000 x 20 000 float64, 3.2 GB), amin, argmin, min_dist <= threshold
// The 20 000-per-side and max_corrs draws (torch.multinomial) stay in Python, in the reference's order.
//
// The arithmetic is DEFINED (include/oryon_hip.h, oryon_gt_corrs; DESIGN.md "Ground-truth correspondences"): float64, no contraction,
// sums left to right, so that tests/gt_corrs_restatement.py - the same sequence of correctly rounded operations in numpy - agrees bit
// for bit.  No kernel here allocates, synchronises or uses an atomic: every output is bit-stable.
//   lift       depth_lift.h: X = (double(fp32(x) - fp32(cx)) * z) / fx / 1000, Y alike with (y, cy, fy), Z = z / 1000;
//              z = double(depth[pixel]) in millimetres.  Zero depth lifts to the origin and is kept.
//   transform  p' = ((R0 x + R1 y) + R2 z) + t per output coordinate (anchor side only).
//   nearest    d2_j = ((dx dx + dy dy) + dz dz), j ascending, strict <: the first minimiser (torch.argmin).  NaN never wins.
//   keep       sqrt(d2) <= threshold, rows written in anchor order.
#include "common.h"
#include "nn_tile.h"
#include "depth_lift.h"

#pragma clang fp contract(off)

namespace oryon {

constexpr int GTC_THREADS = 256;
constexpr int GTC_TILE = NN_TILE;            // query points per LDS tile (nn_tile.h): 3 x 1024 float64 = 24 KB
constexpr int GTC_KEEP_THREADS = 1024;
constexpr int GTC_KEEP_WAVES = GTC_KEEP_THREADS / 64;

__device__ __forceinline__ bool gtc_skip(const int32_t *__restrict__ status, int b) { return status && status[b] != 0; }

// pix [B,cap] linear indices into the H x W image -> xyz [B,cap,3] float64 (metres), yx [B,cap,2] int32.  pose [B,12] or nullptr.
__global__ __launch_bounds__(GTC_THREADS) void gtc_lift_kernel(const float *__restrict__ depth, int HW, int W, const int32_t *__restrict__ pix,
                                                               const int32_t *__restrict__ count, int cap, const double *__restrict__ cam9,
                                                               const double *__restrict__ pose, const int32_t *__restrict__ status,
                                                               double *__restrict__ xyz, int32_t *__restrict__ yx)
{
    const int b = blockIdx.y;
    if (gtc_skip(status, b)) return;
    const int n = min(count[b], cap);
    const int i = blockIdx.x * GTC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int p = pix[(size_t)b * cap + i];
    const bool inside = (uint32_t)p < (uint32_t)HW;          // a pixel outside the image reads no depth: it lifts like a zero-depth one
    const int y = inside ? p / W : 0, x = inside ? p - y * W : 0;
    const double z = inside ? (double)depth[(size_t)b * HW + p] : 0.0;
    const double *K = cam9 + (size_t)b * 9;
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    double V[3];
    depth_lift_f64(x, y, z, fx, (float)cx, fy, (float)cy, V);
    double X = V[0], Y = V[1], Z = V[2];
    if (pose) {
        const double *T = pose + (size_t)b * 12;
        const double x2 = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
        const double y2 = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
        const double z2 = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
        X = x2; Y = y2; Z = z2;
    }
    double *o = xyz + ((size_t)b * cap + i) * 3;
    o[0] = X; o[1] = Y; o[2] = Z;
    int32_t *q = yx + ((size_t)b * cap + i) * 2;
    q[0] = y; q[1] = x;
}

// The hot path.  A workgroup owns GTC_THREADS * PPL anchor points of one pair (PPL per lane, in registers) and walks the pair's query
// cloud in order through LDS tiles of GTC_TILE points (nearest_walk_f64, nn_tile.h: broadcast LDS reads, ascending order, strict <, so
// the first minimiser wins).  idx = -1 and d2 = +inf when no query point compares below +inf (n_dst = 0).
template <int PPL>
__global__ __launch_bounds__(GTC_THREADS) void pcd_nearest_f64_kernel(const double *__restrict__ src, const int32_t *__restrict__ n_src, int cap_src,
                                                                      const double *__restrict__ dst, const int32_t *__restrict__ n_dst, int cap_dst,
                                                                      const int32_t *__restrict__ status, int32_t *__restrict__ idx,
                                                                      double *__restrict__ d2)
{
    extern __shared__ __align__(16) double gtc_tile[];       // [3][GTC_TILE]: x | y | z
    const int b = blockIdx.y;
    if (gtc_skip(status, b)) return;
    const int na = min(n_src[b], cap_src), nq = min(n_dst[b], cap_dst);
    const int row0 = blockIdx.x * (GTC_THREADS * PPL);
    if (row0 >= na) return;                                  // uniform over the workgroup: no barrier is skipped by a part of it
    const double *A = src + (size_t)b * cap_src * 3, *Q = dst + (size_t)b * cap_dst * 3;
    double ax[PPL], ay[PPL], az[PPL], best[PPL];
    int bi[PPL];
#pragma unroll
    for (int u = 0; u < PPL; ++u) {
        const int r = row0 + u * GTC_THREADS + (int)threadIdx.x;
        const bool live = r < na;                            // rows beyond n are never read
        ax[u] = live ? A[(size_t)r * 3 + 0] : 0.0;
        ay[u] = live ? A[(size_t)r * 3 + 1] : 0.0;
        az[u] = live ? A[(size_t)r * 3 + 2] : 0.0;
    }
    nearest_walk_f64<PPL, GTC_THREADS>(Q, nq, gtc_tile, ax, ay, az, best, bi);
#pragma unroll
    for (int u = 0; u < PPL; ++u) {
        const int r = row0 + u * GTC_THREADS + (int)threadIdx.x;
        if (r < na) {
            idx[(size_t)b * cap_src + r] = bi[u];
            d2[(size_t)b * cap_src + r] = best[u];
        }
    }
}

// One workgroup per pair: rows with sqrt(d2) <= threshold, compacted in anchor order by a ballot + prefix sum over the waves (the
// ordered compaction of roi.hip's masks).  corrs [B,cap_a,4] = (y_a, x_a, y_q, x_q); n_corr [B]; a pair with a non-zero status keeps nothing.
__global__ __launch_bounds__(GTC_KEEP_THREADS) void gtc_keep_kernel(const int32_t *__restrict__ idx, const double *__restrict__ d2,
                                                                    const int32_t *__restrict__ n_a, int cap_a, const int32_t *__restrict__ n_q,
                                                                    int cap_q, const int32_t *__restrict__ yx_a, const int32_t *__restrict__ yx_q,
                                                                    double threshold, const int32_t *__restrict__ status,
                                                                    int32_t *__restrict__ corrs, int32_t *__restrict__ n_corr)
{
    __shared__ int s_wave[GTC_KEEP_WAVES];
    const int b = blockIdx.x;
    if (gtc_skip(status, b)) {
        if (threadIdx.x == 0) n_corr[b] = 0;
        return;
    }
    const int na = min(n_a[b], cap_a), nq = min(n_q[b], cap_q);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int i0 = 0; i0 < na; i0 += GTC_KEEP_THREADS) {
        const int i = i0 + (int)threadIdx.x;
        int j = -1;
        bool keep = false;
        if (i < na) {
            j = idx[(size_t)b * cap_a + i];
            keep = (uint32_t)j < (uint32_t)nq && sqrt(d2[(size_t)b * cap_a + i]) <= threshold;
        }
        const unsigned long long vote = __ballot(keep);
        const int before = __popcll(vote & ((1ull << lane) - 1ull));
        __syncthreads();                                     // the previous chunk's readers of s_wave are done
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < GTC_KEEP_WAVES; ++w) {
            const int c = s_wave[w];
            off += (w < wave) ? c : 0;
            total += c;
        }
        if (keep) {
            const int32_t *a = yx_a + ((size_t)b * cap_a + i) * 2, *q = yx_q + ((size_t)b * cap_q + j) * 2;
            int32_t *o = corrs + ((size_t)b * cap_a + base + off + before) * 4;
            o[0] = a[0]; o[1] = a[1]; o[2] = q[0]; o[3] = q[1];
        }
        base += total;
    }
    if (threadIdx.x == 0) n_corr[b] = base;
}


static void launch_lift(const float *depth, int B, int H, int W, const int32_t *pix, const int32_t *n, int cap, const double *cam9,
                        const double *pose, const int32_t *status, double *xyz, int32_t *yx, hipStream_t st)
{
    hipLaunchKernelGGL(gtc_lift_kernel, dim3(ceil_div(cap, GTC_THREADS), B), dim3(GTC_THREADS), 0, st, depth, H * W, W, pix, n, cap, cam9, pose,
                       status, xyz, yx);
}

static void launch_nearest(const double *src, const int32_t *n_src, const double *dst, const int32_t *n_dst, int B, int cap_src, int cap_dst,
                           const int32_t *status, int32_t *idx, double *d2, hipStream_t st)
{
    const size_t lds = 3 * (size_t)GTC_TILE * sizeof(double);
    // One anchor point per lane.  Two per lane (development build only, ORYON_GTC_PPL=2; tools/time_gt_corrs.py --ppl 2) measured the
    // same at 64 pairs (8.95 vs 9.05 ms at 20 000 x 20 000) and 1.8 x slower at one pair (1.46 vs 0.82 ms: half the workgroups).
#ifdef ORYON_DEV
    static const int ppl = dev_env_int("ORYON_GTC_PPL", 1);
    if (ppl == 2) {
        hipLaunchKernelGGL((pcd_nearest_f64_kernel<2>), dim3(ceil_div(cap_src, GTC_THREADS * 2), B), dim3(GTC_THREADS), lds, st, src, n_src, cap_src,
                           dst, n_dst, cap_dst, status, idx, d2);
        return;
    }
#endif
    hipLaunchKernelGGL((pcd_nearest_f64_kernel<1>), dim3(ceil_div(cap_src, GTC_THREADS), B), dim3(GTC_THREADS), lds, st, src, n_src, cap_src, dst,
                       n_dst, cap_dst, status, idx, d2);
}

struct GtcWorkspace {
    double *xyz_a, *xyz_q, *d2;
    int32_t *yx_a, *yx_q, *idx;
    size_t bytes;
};

static GtcWorkspace gtc_carve(void *workspace, int B, int cap_a, int cap_q)
{
    GtcWorkspace w;
    Carver carve(workspace);
    carve(w.xyz_a, (size_t)B * cap_a * 3);
    carve(w.xyz_q, (size_t)B * cap_q * 3);
    carve(w.d2, (size_t)B * cap_a);
    carve(w.yx_a, (size_t)B * cap_a * 2);
    carve(w.yx_q, (size_t)B * cap_q * 2);
    carve(w.idx, (size_t)B * cap_a);
    w.bytes = carve.off;
    return w;
}

}  // namespace oryon

using namespace oryon;

extern "C" int oryon_gtc_lift(const float *depth, int B, int H, int W, const int32_t *pix, const int32_t *n, int cap, const double *cam9,
                              const double *pose, double *xyz, int32_t *yx, void *stream)
{
    ORYON_CHECK_ARG(depth && pix && n && cam9 && xyz && yx);                          // pose may be NULL: no transform
    ORYON_CHECK_ARG(aligned8(cam9) && aligned8(pose) && aligned8(xyz));
    ORYON_CHECK_ARG(B >= 0 && B <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff && cap >= 1);
    if (B == 0) return ORYON_OK;
    launch_lift(depth, B, H, W, pix, n, cap, cam9, pose, nullptr, xyz, yx, as_stream(stream));
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_pcd_nearest_f64(const double *src, const int32_t *n_src, const double *dst, const int32_t *n_dst, int B, int cap_src,
                                     int cap_dst, int32_t *idx, double *d2, void *stream)
{
    ORYON_CHECK_ARG(src && n_src && dst && n_dst && idx && d2);
    ORYON_CHECK_ARG(aligned8(src) && aligned8(dst) && aligned8(d2));
    ORYON_CHECK_ARG(B >= 0 && B <= 65535 && cap_src >= 1 && cap_dst >= 1);
    if (B == 0) return ORYON_OK;
    launch_nearest(src, n_src, dst, n_dst, B, cap_src, cap_dst, nullptr, idx, d2, as_stream(stream));
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" size_t oryon_gt_corrs_workspace_bytes(int B, int cap_a, int cap_q)
{
    if (B <= 0 || B > 65535 || cap_a <= 0 || cap_q <= 0) return 0;
    return gtc_carve(nullptr, B, cap_a, cap_q).bytes;
}

extern "C" int oryon_gt_corrs(const float *depth_a, const float *depth_q, int B, int HA, int WA, int HQ, int WQ, const int32_t *pix_a,
                              const int32_t *n_a, int cap_a, const int32_t *pix_q, const int32_t *n_q, int cap_q, const double *cam_a,
                              const double *cam_q, const double *pose_aq, double threshold, const int32_t *status_in, void *workspace,
                              size_t workspace_bytes, int32_t *corrs, int32_t *n_corr, int32_t *idx, double *d2, void *stream)
{
    ORYON_CHECK_ARG(depth_a && depth_q && pix_a && n_a && pix_q && n_q && cam_a && cam_q && pose_aq && workspace && corrs && n_corr);
    ORYON_CHECK_ARG(aligned8(cam_a) && aligned8(cam_q) && aligned8(pose_aq) && aligned8(d2));   // idx / d2 may be NULL
    ORYON_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255) == 0);
    ORYON_CHECK_ARG(threshold >= 0.0);                                                // NaN fails
    ORYON_CHECK_ARG(B >= 0 && B <= 65535 && cap_a >= 1 && cap_q >= 1);
    ORYON_CHECK_ARG(HA >= 1 && WA >= 1 && HQ >= 1 && WQ >= 1 && (int64_t)HA * WA <= 0x7fffffff && (int64_t)HQ * WQ <= 0x7fffffff);
    if (B == 0) return ORYON_OK;
    const GtcWorkspace w = gtc_carve(workspace, B, cap_a, cap_q);
    ORYON_CHECK_ARG(workspace_bytes >= w.bytes);
    hipStream_t st = as_stream(stream);
    int32_t *idx_out = idx ? idx : w.idx;
    double *d2_out = d2 ? d2 : w.d2;
    launch_lift(depth_a, B, HA, WA, pix_a, n_a, cap_a, cam_a, pose_aq, status_in, w.xyz_a, w.yx_a, st);
    launch_lift(depth_q, B, HQ, WQ, pix_q, n_q, cap_q, cam_q, nullptr, status_in, w.xyz_q, w.yx_q, st);
    launch_nearest(w.xyz_a, n_a, w.xyz_q, n_q, B, cap_a, cap_q, status_in, idx_out, d2_out, st);
    hipLaunchKernelGGL(gtc_keep_kernel, dim3(B), dim3(GTC_KEEP_THREADS), 0, st, idx_out, d2_out, n_a, cap_a, n_q, cap_q, w.yx_a, w.yx_q, threshold,
                       status_in, corrs, n_corr);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
