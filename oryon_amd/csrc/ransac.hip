// RANSAC pose solver (test.solver = ransac): best_fit_transform_with_RANSAC of utils/geo6d.py:40-120 as pipeline.py:462-466 calls it
// (max_iter = 10000, fix_percent = 0.9999, match_err = 0.001), for B pairs in two launches and no host round trip.
//
// The reference is a sequential loop, but every iteration only READS the points, so its meaning is parallel:
//   hypothesis 0        = best_fit_transform over all n rows; hypothesis k >= 1 = best_fit_transform over the four rows of draw k-1
//   iterations evaluate hypotheses 0 .. max_iter-1 (the last draw is made and never evaluated)
//   count_k             = #{i : |R a_i + t - b_i| <= match_err}, in float64
//   some count_k > fix_percent * n (float64 product)  -> the FIRST such k; the result is best_fit_transform over its inliers
//   otherwise           -> the hypothesis of the largest count, lowest k on ties, as it is (no refit)
//   every count 0, or n < 4 -> the 3x4 zero matrix (the caller places it in eye(4): last row 0 0 0 1)
// best_fit_transform: plain means (no +1e-6), H = sum (a - ca)(b - cb)^T, R = V diag(1,1,det) U^T (the reflection fix on the last
// row of Vt), t = cb - R ca: rotation_from_covariance of kabsch.h, in fp64 registers.
//
//   ransac_score_kernel  : grid (ceil(max_iter / 256), B), one lane = one hypothesis.  The block stages the pair's rows in LDS in a
//       frame centred on the pair's centroids (fp32, 24 bytes per correspondence), every lane fits its transform in fp64 and walks
//       the n rows: all lanes read the same LDS address (broadcast).  A point is tested in fp32 against two thresholds that bracket
//       match_err by a bound on the fp32 evaluation's error; the rare point between them is decided in fp64 on the original
//       coordinates - so the classification IS the float64 one, at fp32 cost.  Per block: max of (count << 32 | ~k) and min of the
//       exceeding k by wave shuffles and LDS, then ONE 64-bit atomicMax and one 32-bit atomicMin per block - integer atomics only,
//       nothing depends on arrival order.  The lane that holds the block's key stores its transform's 12 doubles next to it, so the
//       finish kernel never rebuilds (and never re-rounds) a transform.
//   ransac_finish_kernel : one wave per pair: exit -> mask the inliers of the stored transform, 0/1-weighted plain-mean Kabsch over
//       them; best-of-K -> the stored winner; no inlier anywhere or n < 4 -> the zero pose; status_in != 0 -> identity, status passed
//       through (what oryon_pointdsc_register does).
#include "common.h"
#include "kabsch.h"

namespace oryon {
namespace {
constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_MAX_ROWS = 2048;                 // 6 fp32 per row in LDS: 48 KB
constexpr unsigned RS_NO_EXIT = 0xFFFFFFFFu;

struct RansacWs {
    unsigned long long *best;       // [B]  max over hypotheses of count << 32 | (0xFFFFFFFF - k); 0 = no hypothesis has an inlier
    unsigned *first_exit;           // [B]  lowest k with count_k > fix_percent * n; RS_NO_EXIT = none
    double *rt_best, *rt_exit;      // [B, nblk, 12]  the 3x4 transform behind each block's key / exit candidate
};

inline int n_blocks(int max_iter) { return (max_iter + RS_THREADS - 1) / RS_THREADS; }

size_t carve_ransac(int B, int max_iter, void *base, RansacWs *ws)
{
    const size_t per = (size_t)B * n_blocks(max_iter) * 12;
    Carver carve(base);
    RansacWs w;
    carve(w.best, B);
    carve(w.first_exit, B);
    carve(w.rt_best, per);
    carve(w.rt_exit, per);
    if (ws) *ws = w;
    return carve.off;
}

// Squared float64 residual of one correspondence under RT (3x4 row-major).  Explicit fma: the scoring kernel's fallback and the
// finish kernel's inlier mask round identically whatever the compiler contracts elsewhere.
__device__ __forceinline__ double residual2_f64(const double RT[12], const float *__restrict__ a, const float *__restrict__ b)
{
    const double ax = a[0], ay = a[1], az = a[2];
    const double dx = fma(RT[0], ax, fma(RT[1], ay, fma(RT[2], az, RT[3]))) - (double)b[0];
    const double dy = fma(RT[4], ax, fma(RT[5], ay, fma(RT[6], az, RT[7]))) - (double)b[1];
    const double dz = fma(RT[8], ax, fma(RT[9], ay, fma(RT[10], az, RT[11]))) - (double)b[2];
    return fma(dx, dx, fma(dy, dy, dz * dz));
}

// best_fit_transform (utils/geo6d.py:40-73) from the sums of its rows: plain means, den = sw
__device__ inline void rigid_from_sums(const KabschAcc &s, double RT[12])
{
    double ca[3], cb[3], H[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) { ca[i] = s.sa[i] / s.sw; cb[i] = s.sb[i] / s.sw; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) H[i * 3 + j] = s.sab[i * 3 + j] - ca[i] * s.sb[j];
    rotation_from_covariance(H, R);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) RT[i * 4 + j] = R[i * 3 + j];
        RT[i * 4 + 3] = cb[i] - (R[i * 3] * ca[0] + R[i * 3 + 1] * ca[1] + R[i * 3 + 2] * ca[2]);
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(v >> 32), off), lo = __shfl_xor((unsigned)v, off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

__global__ void ransac_init_kernel(RansacWs ws, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) {
        ws.best[i] = 0ull;
        ws.first_exit[i] = RS_NO_EXIT;
    }
}

__global__ __launch_bounds__(RS_THREADS) void ransac_score_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                                  const int32_t *__restrict__ n_rows, int n_cap, int max_iter,
                                                                  double match_err, double fix_percent,
                                                                  const int32_t *__restrict__ sample_idx, uint64_t seed,
                                                                  const int64_t *__restrict__ pair_key,
                                                                  const int32_t *__restrict__ status_in, RansacWs ws,
                                                                  int32_t *__restrict__ counts)
{
    extern __shared__ float2 s_pts[];           // [n][3]: (ax ay) (az bx) (by bz) of a - ca, b - cb in fp32: one address per row, broadcast
    __shared__ double s_sum[RS_WAVES][16];
    __shared__ float s_mag[RS_WAVES][2];
    __shared__ unsigned long long s_key[RS_WAVES];
    __shared__ unsigned s_exit[RS_WAVES];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned k = blockIdx.x * RS_THREADS + t;
    const bool active = k < (unsigned)max_iter;
    int n = n_rows[b];
    n = n > n_cap ? n_cap : n;
    if (n < 4 || (status_in && status_in[b] != ORYON_PAIR_OK)) {      // the finish kernel writes these pairs' poses
        if (counts && active) counts[(size_t)b * max_iter + k] = 0;
        return;
    }
    const float *A = src + (size_t)b * n_cap * 3, *Bp = tgt + (size_t)b * n_cap * 3;

    // sums over all rows: the centroids every lane centres on, and hypothesis 0
    KabschAcc tot;
    tot.clear();
    for (int i = t; i < n; i += RS_THREADS) tot.add(A[3 * i], A[3 * i + 1], A[3 * i + 2], Bp[3 * i], Bp[3 * i + 1], Bp[3 * i + 2], 1.0f);
    tot.wave_reduce();
    if (lane == 0) {
        s_sum[wave][0] = tot.sw;
#pragma unroll
        for (int i = 0; i < 3; ++i) { s_sum[wave][1 + i] = tot.sa[i]; s_sum[wave][4 + i] = tot.sb[i]; }
#pragma unroll
        for (int i = 0; i < 9; ++i) s_sum[wave][7 + i] = tot.sab[i];
    }
    __syncthreads();
    {
        double v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = (s_sum[0][i] + s_sum[1][i]) + (s_sum[2][i] + s_sum[3][i]);
        tot.sw = v[0];
#pragma unroll
        for (int i = 0; i < 3; ++i) { tot.sa[i] = v[1 + i]; tot.sb[i] = v[4 + i]; }
#pragma unroll
        for (int i = 0; i < 9; ++i) tot.sab[i] = v[7 + i];
    }
    double ca[3], cb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { ca[i] = tot.sa[i] / tot.sw; cb[i] = tot.sb[i] / tot.sw; }
    float mag_a = 0.0f, mag_b = 0.0f;
    for (int i = t; i < n; i += RS_THREADS) {
        float a[3], q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[c] = (float)((double)A[3 * i + c] - ca[c]);
            q[c] = (float)((double)Bp[3 * i + c] - cb[c]);
            mag_a = fmaxf(mag_a, fabsf(a[c]));
            mag_b = fmaxf(mag_b, fabsf(q[c]));
        }
        s_pts[3 * i] = make_float2(a[0], a[1]);
        s_pts[3 * i + 1] = make_float2(a[2], q[0]);
        s_pts[3 * i + 2] = make_float2(q[1], q[2]);
    }
    mag_a = wave_max_f32(mag_a);
    mag_b = wave_max_f32(mag_b);
    if (lane == 0) { s_mag[wave][0] = mag_a; s_mag[wave][1] = mag_b; }
    __syncthreads();
    mag_a = fmaxf(fmaxf(s_mag[0][0], s_mag[1][0]), fmaxf(s_mag[2][0], s_mag[3][0]));
    mag_b = fmaxf(fmaxf(s_mag[0][1], s_mag[1][1]), fmaxf(s_mag[2][1], s_mag[3][1]));

    // this lane's hypothesis (lanes past max_iter walk the rows with hypothesis 0 and publish nothing)
    KabschAcc h = tot;
    if (active && k > 0) {
        h.clear();
        const uint64_t key = pair_key ? (uint64_t)pair_key[b] : (uint64_t)b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned r;
            if (sample_idx) r = (unsigned)sample_idx[((size_t)b * max_iter + (k - 1)) * 4 + j];
            else r = (unsigned)(((uint64_t)rng_u32(seed, key, 3u, 4u * (k - 1) + (unsigned)j) * (uint64_t)n) >> 32);
            r = r < (unsigned)n ? r : (unsigned)(n - 1);
            h.add(A[3 * r], A[3 * r + 1], A[3 * r + 2], Bp[3 * r], Bp[3 * r + 1], Bp[3 * r + 2], 1.0f);
        }
    }
    double RT[12];
    rigid_from_sums(h, RT);

    // the same transform in the centred frame, in fp32, and the band around match_err inside which fp32 cannot decide.
    // With u = 2^-24: rounding of the centred rows, of R and t, and of the three fma + one subtraction per component moves a
    // component by at most 11 u S, S = 3 max|a| + max|b| + max|t| (every partial sum is below S), the distance by sqrt(3) times
    // that: < 20 u S.  The band is 32 u (S + match_err); the thresholds are squared in fp64 and moved outwards by 2e-6 relative,
    // which covers their own rounding to fp32 and that of the fp32 sum of squares (4 u relative).
    float Rf[9], tf[3];
    double t_mag = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double tc = RT[i * 4 + 3] + (RT[i * 4] * ca[0] + RT[i * 4 + 1] * ca[1] + RT[i * 4 + 2] * ca[2]) - cb[i];
        tf[i] = (float)tc;
        t_mag = fmax(t_mag, fabs(tc));
#pragma unroll
        for (int j = 0; j < 3; ++j) Rf[i * 3 + j] = (float)RT[i * 4 + j];
    }
    const double band = 32.0 * 5.9604644775390625e-8 * (3.0 * (double)mag_a + (double)mag_b + t_mag + match_err);
    const double e_lo = match_err - band, e_hi = match_err + band;
    const float lo = e_lo > 0.0 ? (float)(e_lo * e_lo * (1.0 - 2e-6)) : -1.0f;
    const float hi = (float)(e_hi * e_hi * (1.0 + 2e-6));
    const double thr2 = match_err * match_err;

    int cnt = 0;
    float2 q0 = s_pts[0], q1 = s_pts[1], q2 = s_pts[2];
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
        const float2 p0 = q0, p1 = q1, p2 = q2;                                            // ax ay | az bx | by bz
        const int nx = i + 1 < n ? i + 1 : i;                                              // the next row's reads are in flight during this row's test
        q0 = s_pts[3 * nx]; q1 = s_pts[3 * nx + 1]; q2 = s_pts[3 * nx + 2];
        const float dx = fmaf(Rf[0], p0.x, fmaf(Rf[1], p0.y, fmaf(Rf[2], p1.x, tf[0]))) - p1.y;
        const float dy = fmaf(Rf[3], p0.x, fmaf(Rf[4], p0.y, fmaf(Rf[5], p1.x, tf[1]))) - p2.x;
        const float dz = fmaf(Rf[6], p0.x, fmaf(Rf[7], p0.y, fmaf(Rf[8], p1.x, tf[2]))) - p2.y;
        const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
        const bool inlier = d2 < lo;
        cnt += inlier ? 1 : 0;
        if (!inlier && !(d2 > hi)) cnt += residual2_f64(RT, A + 3 * i, Bp + 3 * i) <= thr2 ? 1 : 0;      // undecided in fp32 (or NaN): float64
    }
    if (counts && active) counts[(size_t)b * max_iter + k] = cnt;

    const bool exceeds = active && (double)cnt > fix_percent * (double)n;
    const unsigned long long my_key = (active && cnt > 0) ? ((unsigned long long)(unsigned)cnt << 32) | (0xFFFFFFFFu - k) : 0ull;
    const unsigned my_exit = exceeds ? k : RS_NO_EXIT;
    const unsigned long long wk = wave_max_u64(my_key);
    const unsigned we = wave_min_u32(my_exit);
    if (lane == 0) { s_key[wave] = wk; s_exit[wave] = we; }
    __syncthreads();
    unsigned long long bk = s_key[0];
    unsigned be = s_exit[0];
#pragma unroll
    for (int w = 1; w < RS_WAVES; ++w) {
        bk = s_key[w] > bk ? s_key[w] : bk;
        be = s_exit[w] < be ? s_exit[w] : be;
    }
    const size_t slot = ((size_t)b * gridDim.x + blockIdx.x) * 12;
    if (my_key != 0ull && my_key == bk) {          // keys are distinct: exactly one lane
#pragma unroll
        for (int i = 0; i < 12; ++i) ws.rt_best[slot + i] = RT[i];
    }
    if (exceeds && my_exit == be) {
#pragma unroll
        for (int i = 0; i < 12; ++i) ws.rt_exit[slot + i] = RT[i];
    }
    if (t == 0) {
        if (bk != 0ull) atomicMax(&ws.best[b], bk);
        if (be != RS_NO_EXIT) atomicMin(&ws.first_exit[b], be);
    }
}

__global__ __launch_bounds__(64) void ransac_finish_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                           const int32_t *__restrict__ n_rows, int n_cap, int nblk, double match_err,
                                                           const int32_t *__restrict__ status_in, RansacWs ws, float *__restrict__ T,
                                                           int32_t *__restrict__ winner, int32_t *__restrict__ exited,
                                                           int32_t *__restrict__ status_out)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    float *Tb = T + (size_t)b * 16;
    const int st = status_in ? status_in[b] : ORYON_PAIR_OK;
    int n = n_rows[b];
    n = n > n_cap ? n_cap : n;
    int win = -1, ex = 0;
    if (st != ORYON_PAIR_OK) {                     // failure path of the reference: identity pose (pipeline.py:341,350)
        if (lane < 16) Tb[lane] = (lane % 5 == 0) ? 1.0f : 0.0f;
    } else {
        double RT[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) RT[i] = 0.0;
        const unsigned fe = n >= 4 ? ws.first_exit[b] : RS_NO_EXIT;
        const unsigned long long key = n >= 4 ? ws.best[b] : 0ull;
        if (fe != RS_NO_EXIT) {
            // geo6d.py:105-107: refit over the inliers of the first hypothesis whose count exceeds fix_percent * n
            const double *P = ws.rt_exit + ((size_t)b * nblk + fe / RS_THREADS) * 12;
            double M[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = P[i];
            const float *A = src + (size_t)b * n_cap * 3, *Bp = tgt + (size_t)b * n_cap * 3;
            const double thr2 = match_err * match_err;
            KabschAcc acc;
            acc.clear();
            for (int i = lane; i < n; i += 64)
                if (residual2_f64(M, A + 3 * i, Bp + 3 * i) <= thr2) acc.add(A[3 * i], A[3 * i + 1], A[3 * i + 2], Bp[3 * i], Bp[3 * i + 1], Bp[3 * i + 2], 1.0f);
            acc.wave_reduce();
            if (acc.sw > 0.0) rigid_from_sums(acc, RT);
            win = (int)fe;
            ex = 1;
        } else if (key != 0ull) {
            const unsigned kbest = 0xFFFFFFFFu - (unsigned)key;
            const double *P = ws.rt_best + ((size_t)b * nblk + kbest / RS_THREADS) * 12;
#pragma unroll
            for (int i = 0; i < 12; ++i) RT[i] = P[i];
            win = (int)kbest;
        }
        if (lane < 12) {
            float v = 0.0f;
#pragma unroll
            for (int i = 0; i < 12; ++i) v = lane == i ? (float)RT[i] : v;
            Tb[lane] = v;
        } else if (lane < 16) Tb[lane] = lane == 15 ? 1.0f : 0.0f;
    }
    if (lane == 0) {
        if (winner) winner[b] = win;
        if (exited) exited[b] = ex;
        if (status_out) status_out[b] = st;
    }
}
}  // namespace
}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_ransac_workspace_bytes(int B, int n_cap, int max_iter)
{
    if (B <= 0 || n_cap <= 0 || n_cap > RS_MAX_ROWS || max_iter <= 0) return 0;
    return carve_ransac(B, max_iter, nullptr, nullptr);
}

extern "C" int oryon_ransac_register(const float *src, const float *tgt, const int32_t *n, int B, int n_cap, int max_iter, double match_err,
                                     double fix_percent, const int32_t *sample_idx, uint64_t seed, const int64_t *pair_key,
                                     const int32_t *status_in, void *workspace, size_t workspace_bytes, float *T, int32_t *winner,
                                     int32_t *exited, int32_t *counts, int32_t *status_out, void *stream)
{
    ORYON_CHECK_ARG(B >= 0 && B <= 65535 && n_cap > 0 && max_iter > 0 && match_err >= 0.0);
    if (n_cap > RS_MAX_ROWS) { set_error("%s: n_cap = %d exceeds %d rows per pair (LDS budget of the scoring kernel)", __func__, n_cap, RS_MAX_ROWS); return ORYON_ERR_INVALID_ARG; }
    if (B == 0) return ORYON_OK;
    ORYON_CHECK_ARG(src && tgt && n && T);
    RansacWs ws;
    ORYON_CHECK_WORKSPACE("ransac ", workspace, workspace_bytes, carve_ransac(B, max_iter, nullptr, nullptr));
    carve_ransac(B, max_iter, workspace, &ws);
    hipStream_t st = as_stream(stream);
    const int nblk = n_blocks(max_iter);
    hipLaunchKernelGGL(ransac_init_kernel, dim3((B + 255) / 256), dim3(256), 0, st, ws, B);
    ORYON_CHECK_LAUNCH();
    profile_begin(st, "ransac_score_kernel");
    hipLaunchKernelGGL(ransac_score_kernel, dim3(nblk, B), dim3(RS_THREADS), (size_t)n_cap * 6 * sizeof(float), st, src, tgt, n, n_cap, max_iter,
                       match_err, fix_percent, sample_idx, seed, pair_key, status_in, ws, counts);
    profile_end(st);
    ORYON_CHECK_LAUNCH();
    hipLaunchKernelGGL(ransac_finish_kernel, dim3(B), dim3(64), 0, st, src, tgt, n, n_cap, nblk, match_err, status_in, ws, T, winner, exited,
                       status_out);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
