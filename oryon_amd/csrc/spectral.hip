// Spectral pose solver (test.solver = spectral): a registration that needs no weights and no random numbers.  The learned parts of
// PointDSC - the confidence of every correspondence and the per-seed neighbour lists - are replaced by spectral matching on the
// spatial-compatibility matrix (the `cal_leading_eigenvector(M, method='power')` line PointDSC.py:170 keeps commented out) and by
// second-order spatial compatibility (SC^2, Chen et al., CVPR 2022); seeds, per-seed power iteration, weighted Kabsch, hypothesis
// scoring and refinement are PointDSC's own kernels (pdsc_solver.hip), unchanged.
//
// THE DEFINITION, for one pair (src, tgt [n_cap,3] fp32 metres, n rows used; rows >= n are never read):
//   S1  hard compatibility, float64, bit-packed.  For i != j, both < n: a = |s_i - s_j|, b = |t_i - t_j|, each
//       sqrt((dx dx + dy dy) + dz dz) on the fp32 inputs widened to float64, every operation correctly rounded in that order, no fused
//       multiply-add; C_ij = |a - b| < (double) inlier_threshold.  Diagonal 0; rows and columns >= n are 0.  Bit j & 31 of word j >> 5 of
//       row i.  numpy float64 reproduces these bits.
//   S2  confidence, fp32.  M_ij = max(0, 1 - d^2 / sigma_d^2), d = sqrt_rn(|s_i - s_j|^2) - sqrt_rn(|t_i - t_j|^2), M_ii = 0 (the spatial
//       factor of PointDSC.py:151-153).  v = 1, then EXACTLY num_iterations times u = M v, v = u / (|u|_2 + 1e-6) (PointDSC.py:349-353);
//       conf = v.  There is no allclose exit here, on purpose: it would save a few of ten iterations and make the result depend on an
//       fp32 near-tie.  The summation order is fixed (below), so conf is the same bits in every run, batch position and stream.
//   S3  seeds: PointDSC's NMS seeds (pdsc_run_seeds, PointDSC.py:199-217) on conf with nms_radius and ratio; S = int(n ratio).  S = 0
//       (n < 10 at ratio 0.1) fails as under PointDSC: identity pose, ORYON_PAIR_NO_CORR.
//   S4  consensus sets, integer.  For seed s: score_j = C_sj popcount(row_s & row_j) (= (C . (C C))_sj).  The set is the seed, then the
//       k' - 1 rows j != s of the highest score, ties by ascending j; k' = min(k, n - 1).
//   S5  local matrix [k,k]: S2's expression between the members of the set, zero diagonal.
//   S6-S8  pdsc_power_kernel, pdsc_seed_solve_kernel, pdsc_seed_select_kernel (PointDSC.py:280-336 with the joint early exit); the
//       inlier threshold is inlier_threshold.
//   S9  pdsc_refine_kernel with tau = inlier_threshold (not the reference's two-dataset table 0.10 / 1.2 of PointDSC.py:415-418, which
//       means nothing at object scale); status handling as there.
// The defaults (inlier_threshold = sigma_d = 0.01, nms_radius = 0.02) are object-scale and were chosen from ONE synthetic experiment
// (planted motions of a 0.3 m cube of points, 1 mm noise, 50-90 % outliers; PointDSC's 0.10 m values leave 69 % of all pairs
// "compatible" there and up to 3 degrees of error).  Nothing about them has been measured on real data.
//
// Kernels:
//   spectral_compat_kernel  grid (n_cap/64 column chunks, n_cap/64 row tiles, B).  A lane keeps ONE column's six coordinates in float64
//       registers, a wave walks 16 rows (row coordinates: uniform loads), one __ballot per row = the row's two words of the chunk.
//   spectral_matvec_kernel  grid (n_cap/32, B), one launch per iteration: M is recomputed from the pair's points in LDS (28 bytes per
//       row) instead of being stored (n_cap^2 floats per pair).  Eight lanes per row, each a contiguous eighth of the columns in
//       ascending order (one fmaf chain), combined as ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7)).  Every workgroup first
//       renormalises the previous iterate itself: |u|^2 by 256 threads striding the rows in ascending order, a wave xor-reduction,
//       (w0 + w1) + (w2 + w3) - the same bits in every workgroup, so no launch and no atomics for the norm.  The kernel is bound by
//       its VALU work (two correctly rounded square roots per entry), not by occupancy: four lanes per row measured 29 us per launch
//       at 64 pairs x 500 rows, eight 27 us.
//   spectral_conf_kernel    grid (B): the last normalisation; rows >= n of conf are written 0.
//   spectral_sets_kernel    grid (S_cap, B): scores by popcount over 128-bit pieces of the two bit rows, ranks by counting over
//       composite keys score << 12 | (4095 - j) (distinct, so the order is total; a thread keeps its 2, 4 or 8 rows' counts in
//       registers and reads the keys four at a time from one LDS address), then the k' x k' matrix.
// Measured (tools/time_spectral.py, 64 pairs x 500 rows, 80 % outliers, one MI355X): 0.47 ms per call; DESIGN.md section 7f.
#include "common.h"
#include "pdsc.h"

// everything below is evaluated as written: S1 is specified without contraction, and the fp32 stages are pinned by explicit fmaf
#pragma clang fp contract(off)

namespace oryon {
namespace {
constexpr int SP_MAX_ROWS = 2048;
constexpr int SP_MAX_K = PDSC_MAX_K - 1;
constexpr int SP_MV_LANES = 8, SP_MV_ROWS = 256 / SP_MV_LANES;     // spectral_matvec_kernel: lanes per row, rows per workgroup

struct SpectralWs {
    uint32_t *compat;     // [B,n_cap,n_cap/32]
    float *u0, *u1;       // [B,n_cap] un-normalised iterates (ping-pong)
    float *conf;          // [B,n_cap]
    float *seed_key;      // [B,n_cap]
    int32_t *seeds;       // [B,S_cap]
    int32_t *n_seeds;     // [B]
    int32_t *sets;        // [B,S_cap,k]
    float *Mmat;          // [B,S_cap,k,k]
    float *v_hist;        // [B,S_cap,PDSC_MAX_IT,PDSC_MAX_K]
    int32_t *close_hist;  // [B,S_cap,PDSC_MAX_IT]
    float *seed_T;        // [B,S_cap,16]
    float *fitness;       // [B,S_cap]
    int32_t *best;        // [B]
    float *T0;            // [B,16]
    float *T;             // [B,16] (stages without a T output)
    int S_cap;
};

bool supported(const oryon_spectral_config_t *c, int B, int n_cap)
{
    return c && B >= 1 && B <= 65535 && n_cap > 0 && n_cap % 128 == 0 && n_cap <= SP_MAX_ROWS && c->k >= 2 && c->k <= SP_MAX_K &&
           c->num_iterations >= 1 && c->num_iterations <= PDSC_MAX_IT && c->ratio > 0.0f && c->ratio <= 1.0f && c->inlier_threshold > 0.0f &&
           c->sigma_d > 0.0f && c->nms_radius >= 0.0f;
}

int seed_cap(const oryon_spectral_config_t &c, int n_cap) { return (int)((double)n_cap * (double)c.ratio) + 1; }

size_t carve_spectral(const oryon_spectral_config_t &c, int B, int n_cap, void *base, SpectralWs *ws)
{
    Carver carve(base);
    const size_t rows = (size_t)B * n_cap, S_cap = (size_t)seed_cap(c, n_cap), seeds = (size_t)B * S_cap, k = (size_t)c.k;
    SpectralWs w;
    carve(w.compat, rows * (n_cap / 32));
    carve(w.u0, rows);
    carve(w.u1, rows);
    carve(w.conf, rows);
    carve(w.seed_key, rows);
    carve(w.seeds, seeds);
    carve(w.n_seeds, (size_t)B);
    carve(w.sets, seeds * k);
    carve(w.Mmat, seeds * k * k);
    carve(w.v_hist, seeds * PDSC_MAX_IT * PDSC_MAX_K);
    carve(w.close_hist, seeds * PDSC_MAX_IT);
    carve(w.seed_T, seeds * 16);
    carve(w.fitness, seeds);
    carve(w.best, (size_t)B);
    carve(w.T0, (size_t)B * 16);
    carve(w.T, (size_t)B * 16);
    w.S_cap = (int)S_cap;
    if (ws) *ws = w;
    return carve.off;
}

__device__ __forceinline__ int rows_of(const int32_t *__restrict__ n_rows, int b, int n_cap)
{
    const int n = n_rows[b];
    return n < 0 ? 0 : (n > n_cap ? n_cap : n);
}

// ------------------------------------------------------------------------------------------------ S1
__global__ __launch_bounds__(256) void spectral_compat_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                               const int32_t *__restrict__ n_rows, int n_cap, double tau,
                                                               uint32_t *__restrict__ compat)
{
    const int b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = rows_of(n_rows, b, n_cap);
    const int j = blockIdx.x * 64 + lane;
    const bool j_in = j < n;
    const float *sp = src + (size_t)b * n_cap * 3, *tp = tgt + (size_t)b * n_cap * 3;
    double sj[3] = {0.0, 0.0, 0.0}, tj[3] = {0.0, 0.0, 0.0};
    if (j_in) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { sj[d] = (double)sp[3 * j + d]; tj[d] = (double)tp[3 * j + d]; }
    }
    const int i0 = blockIdx.y * 64 + wave * 16;                  // this wave's 16 rows (wave-uniform)
    unsigned long long mine = 0ull;                              // lane r keeps row i0 + r's 64 bits
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + r;
        bool c = false;
        if (i < n) {                                             // uniform: rows >= n are never read
            const double six = (double)sp[3 * i], siy = (double)sp[3 * i + 1], siz = (double)sp[3 * i + 2];
            const double tix = (double)tp[3 * i], tiy = (double)tp[3 * i + 1], tiz = (double)tp[3 * i + 2];
            if (j_in && j != i) {
                const double dx = six - sj[0], dy = siy - sj[1], dz = siz - sj[2];
                const double ex = tix - tj[0], ey = tiy - tj[1], ez = tiz - tj[2];
                const double a = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
                const double q = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey)), __dmul_rn(ez, ez)));
                c = fabs(a - q) < tau;
            }
        }
        const unsigned long long bits = __ballot(c);
        if (lane == r) mine = bits;
    }
    if (lane < 16) {
        // words 2 chunk, 2 chunk + 1 of row i0 + lane: 8-byte aligned (n_cap / 32 is a multiple of 4)
        uint32_t *row = compat + ((size_t)b * n_cap + i0 + lane) * (n_cap / 32) + 2 * blockIdx.x;
        *reinterpret_cast<uint2 *>(row) = make_uint2((uint32_t)mine, (uint32_t)(mine >> 32));
    }
}

// ------------------------------------------------------------------------------------------------ S2
// M_ij of the definition between two rows held as (x, y, z) of both sides
__device__ __forceinline__ float spatial_factor(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                                 float dx_, float dy_, float dz_, float inv_sigma2)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float ex = cx - dx_, ey = cy - dy_, ez = cz - dz_;
    const float df = sqrt_rn(dx * dx + dy * dy + dz * dz) - sqrt_rn(ex * ex + ey * ey + ez * ez);
    const float m = 1.0f - df * df * inv_sigma2;
    return m > 0.0f ? m : 0.0f;
}

// |u|^2 over rows < n in a fixed order: thread t sums rows t, t + 256, .. ascending; xor-reduction inside a wave; (w0 + w1) + (w2 + w3).
// All 256 threads call it; red is 4 floats of LDS.  Contains two barriers.
__device__ __forceinline__ float block_norm2(const float *__restrict__ u, int n, float *red)
{
    const int t = threadIdx.x;
    float sq = 0.0f;
    for (int j = t; j < n; j += 256) sq = fmaf(u[j], u[j], sq);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = sq;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void spectral_matvec_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                               const int32_t *__restrict__ n_rows, int n_cap, float inv_sigma2,
                                                               const float *__restrict__ u_prev /* NULL: v = 1 */,
                                                               float *__restrict__ u_next)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];   // no static LDS in this kernel: the float4 array starts 16-byte aligned
    float4 *ps = reinterpret_cast<float4 *>(sm);                 // [n_cap] s_j and v_j
    float *tx = sm + 4 * n_cap, *ty = tx + n_cap, *tz = ty + n_cap;
    float *red = tz + n_cap;                                     // [4]
    const int b = blockIdx.y, t = threadIdx.x;
    const int n = rows_of(n_rows, b, n_cap);
    if ((int)blockIdx.x * SP_MV_ROWS >= n) return;               // the whole workgroup: no barrier is skipped by a part of it
    const float *sp = src + (size_t)b * n_cap * 3, *tp = tgt + (size_t)b * n_cap * 3;
    const float *up = u_prev ? u_prev + (size_t)b * n_cap : nullptr;
    float den = 1.0f;
    if (up) den = sqrt_rn(block_norm2(up, n, red)) + 1e-6f;
    for (int j = t; j < n; j += 256) {
        ps[j] = make_float4(sp[3 * j], sp[3 * j + 1], sp[3 * j + 2], up ? up[j] / den : 1.0f);
        tx[j] = tp[3 * j]; ty[j] = tp[3 * j + 1]; tz[j] = tp[3 * j + 2];
    }
    __syncthreads();
    const int i = blockIdx.x * SP_MV_ROWS + t / SP_MV_LANES, part = t % SP_MV_LANES;
    float acc = 0.0f;
    if (i < n) {
        const float4 me = ps[i];
        const float mx = tx[i], my = ty[i], mz = tz[i];
        const int per = (n + SP_MV_LANES - 1) / SP_MV_LANES, j0 = part * per, j1 = (j0 + per < n) ? j0 + per : n;
        for (int j = j0; j < j1; ++j) {
            const float4 o = ps[j];
            const float m = spatial_factor(me.x, me.y, me.z, o.x, o.y, o.z, mx, my, mz, tx[j], ty[j], tz[j], inv_sigma2);
            acc = fmaf(j == i ? 0.0f : m, o.w, acc);
        }
    }
    acc += __shfl_xor(acc, 1);                                   // q0 + q1 | q2 + q3 | q4 + q5 | q6 + q7
    acc += __shfl_xor(acc, 2);                                   // (q0 + q1) + (q2 + q3) | (q4 + q5) + (q6 + q7)
    acc += __shfl_xor(acc, 4);
    if (i < n && part == 0) u_next[(size_t)b * n_cap + i] = acc;
}

__global__ __launch_bounds__(256) void spectral_conf_kernel(const float *__restrict__ u, const int32_t *__restrict__ n_rows, int n_cap,
                                                             float *__restrict__ conf)
{
    __shared__ float red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = rows_of(n_rows, b, n_cap);
    const float *up = u + (size_t)b * n_cap;
    const float den = sqrt_rn(block_norm2(up, n, red)) + 1e-6f;
    for (int j = t; j < n_cap; j += 256) conf[(size_t)b * n_cap + j] = j < n ? up[j] / den : 0.0f;
}

// ------------------------------------------------------------------------------------------------ S4 + S5
// keys [n] (padded to a multiple of four with the lowest int, which is above no key) -> kidx[1 + rank] = row for ranks < k' - 1 among
// the rows other than the seed.  The keys come four at a time from one LDS address for the whole wave.
template <int U>
__device__ __forceinline__ void rank_rows(const int *keys, int n, int seed, int kk, int *kidx)
{
    const int t = threadIdx.x;
    int my[U], rk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = t + 256 * u;
        my[u] = j < n ? keys[j] : 0x7fffffff;
        rk[u] = 0;
    }
    const int4 *k4 = reinterpret_cast<const int4 *>(keys);
    for (int q = 0; q < (n + 3) / 4; ++q) {
        const int4 kv = k4[q];
#pragma unroll
        for (int u = 0; u < U; ++u)
            rk[u] += (kv.x > my[u] ? 1 : 0) + (kv.y > my[u] ? 1 : 0) + (kv.z > my[u] ? 1 : 0) + (kv.w > my[u] ? 1 : 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int j = t + 256 * u;
        if (j < n && j != seed && rk[u] < kk - 1) kidx[1 + rk[u]] = j;
    }
}

__global__ __launch_bounds__(256) void spectral_sets_kernel(const float *__restrict__ src, const float *__restrict__ tgt,
                                                             const int32_t *__restrict__ n_rows, int n_cap,
                                                             const uint32_t *__restrict__ compat, const int32_t *__restrict__ seeds,
                                                             const int32_t *__restrict__ n_seeds, int S_cap, int k_cfg, float inv_sigma2,
                                                             int32_t *__restrict__ sets, float *__restrict__ Mmat,
                                                             int32_t *__restrict__ scores /* [B,S_cap,n_cap] or NULL */)
{
    extern __shared__ __attribute__((aligned(16))) int smi[];
    int *keys = smi;                                             // [n_cap]
    uint32_t *row_s = reinterpret_cast<uint32_t *>(keys + n_cap);      // [n_cap / 32], 16-byte aligned (n_cap % 128 == 0)
    int *kidx = reinterpret_cast<int *>(row_s + n_cap / 32);     // [PDSC_MAX_K]
    float *kc = reinterpret_cast<float *>(kidx + PDSC_MAX_K);    // [PDSC_MAX_K][6]
    const int b = blockIdx.y, slot = blockIdx.x, t = threadIdx.x;
    if (slot >= n_seeds[b]) return;
    const int n = rows_of(n_rows, b, n_cap);
    const int W = n_cap / 32;
    const int kk = k_cfg < n - 1 ? k_cfg : n - 1;                // k' (the tail kernels compute the same)
    const int seed = seeds[(size_t)b * S_cap + slot];
    const uint32_t *cb = compat + (size_t)b * n_cap * W;
    for (int w = t; w < W; w += 256) row_s[w] = cb[(size_t)seed * W + w];
    __syncthreads();
    for (int j = t; j < n_cap; j += 256) {
        int sc = 0;
        if (j < n && j != seed && ((row_s[j >> 5] >> (j & 31)) & 1u)) {
            const uint4 *rj = reinterpret_cast<const uint4 *>(cb + (size_t)j * W), *rs = reinterpret_cast<const uint4 *>(row_s);
            for (int q = 0; q < W / 4; ++q) {
                const uint4 x = rj[q], y = rs[q];
                sc += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
            }
        }
        if (scores) scores[((size_t)b * S_cap + slot) * n_cap + j] = sc;
        // descending score, ties by ascending row: distinct keys, the seed itself below every other row
        if (j < n) keys[j] = j == seed ? -1 : ((sc << 12) | (4095 - j));
        else if (j < ((n + 3) & ~3)) keys[j] = (int)0x80000000;  // the padding rank_rows reads: greater than no key
    }
    if (t < PDSC_MAX_K) kidx[t] = -1;
    __syncthreads();
    // rank counting: rank_j = #{j' : key_j' > key_j}; a thread owns rows t, t + 256, .. : 2, 4 or 8 of them by the pair's size
    if (n <= 512) rank_rows<2>(keys, n, seed, kk, kidx);
    else if (n <= 1024) rank_rows<4>(keys, n, seed, kk, kidx);
    else rank_rows<8>(keys, n, seed, kk, kidx);
    if (t == 0 && kk >= 1) kidx[0] = seed;
    __syncthreads();
    if (t < k_cfg) sets[((size_t)b * S_cap + slot) * k_cfg + t] = t < kk ? kidx[t] : -1;
    for (int e = t; e < kk * 3; e += 256) {
        const int a = e / 3, d = e % 3;
        kc[a * 6 + d] = src[((size_t)b * n_cap + kidx[a]) * 3 + d];
        kc[a * 6 + 3 + d] = tgt[((size_t)b * n_cap + kidx[a]) * 3 + d];
    }
    __syncthreads();
    float *Mo = Mmat + ((size_t)b * S_cap + slot) * k_cfg * k_cfg;
    for (int e = t; e < k_cfg * k_cfg; e += 256) {
        const int a = e / k_cfg, c = e % k_cfg;
        float v = 0.0f;
        if (a < kk && c < kk && a != c) {
            const float *pa = kc + a * 6, *pb = kc + c * 6;
            v = spatial_factor(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], pa[3], pa[4], pa[5], pb[3], pb[4], pb[5], inv_sigma2);
        }
        Mo[e] = v;
    }
}

struct SpectralOut {
    uint32_t *compat;
    float *conf;
    int32_t *seeds, *n_seeds, *sets, *scores;
    float *Mmat;
    int32_t *close;
    float *seed_T, *fitness;
    int32_t *best;
    float *T0;
};

int run_spectral(const char *who, const oryon_spectral_config_t &c, const float *src, const float *tgt, const int32_t *n, int B, int n_cap,
                 const int32_t *status_in, const SpectralWs &ws, float *T, uint8_t *labels, int32_t *status_out, const SpectralOut *out,
                 hipStream_t st)
{
    const int S_cap = ws.S_cap, k = c.k, nit = c.num_iterations;
    const float inv_sigma2 = 1.0f / (c.sigma_d * c.sigma_d);
    hipLaunchKernelGGL(spectral_compat_kernel, dim3(n_cap / 64, n_cap / 64, B), dim3(256), 0, st, src, tgt, n, n_cap, (double)c.inlier_threshold,
                       ws.compat);
    float *u[2] = {ws.u0, ws.u1};
    for (int it = 0; it < nit; ++it)
        hipLaunchKernelGGL(spectral_matvec_kernel, dim3(n_cap / SP_MV_ROWS, B), dim3(256), ((size_t)7 * n_cap + 4) * sizeof(float), st, src, tgt, n, n_cap,
                           inv_sigma2, it ? u[(it - 1) & 1] : nullptr, u[it & 1]);
    hipLaunchKernelGGL(spectral_conf_kernel, dim3(B), dim3(256), 0, st, u[(nit - 1) & 1], n, n_cap, ws.conf);
    if (hipGetLastError() != hipSuccess) { set_error("%s: confidence launch failed", who); return ORYON_ERR_HIP; }
    PdscModel M;
    memset(&M.cfg, 0, sizeof(M.cfg));
    M.cfg.ratio = c.ratio;
    M.cfg.nms_radius = c.nms_radius;
    int rc = pdsc_run_seeds(M, src, ws.conf, n, B, n_cap, S_cap, ws.seeds, ws.n_seeds, ws.seed_key, st);
    if (rc) { set_error("%s: seeds launch failed", who); return rc; }
    const size_t sh = ((size_t)n_cap + n_cap / 32 + PDSC_MAX_K + PDSC_MAX_K * 6) * sizeof(int);
    hipLaunchKernelGGL(spectral_sets_kernel, dim3(S_cap, B), dim3(256), sh, st, src, tgt, n, n_cap, ws.compat, ws.seeds, ws.n_seeds, S_cap, k,
                       inv_sigma2, ws.sets, ws.Mmat, out ? out->scores : nullptr);
    if (hipGetLastError() != hipSuccess) { set_error("%s: consensus-set launch failed", who); return ORYON_ERR_HIP; }
    rc = pdsc_run_tail(src, tgt, n, ws.n_seeds, B, n_cap, S_cap, k, nit, c.inlier_threshold, ws.sets, ws.Mmat, ws.v_hist, ws.close_hist,
                       ws.seed_T, ws.fitness, ws.best, ws.T0, labels, st);
    if (rc) { set_error("%s: hypotheses launch failed", who); return rc; }
    rc = pdsc_run_refine_tau(src, tgt, n, B, n_cap, c.inlier_threshold, ws.T0, status_in, ws.n_seeds, T ? T : ws.T, status_out, st);
    if (rc) { set_error("%s: refine launch failed", who); return rc; }
    if (out) {
        const size_t rows = (size_t)B * n_cap, seeds = (size_t)B * S_cap;
        auto copy = [&](void *dst, const void *from, size_t bytes) {
            return dst ? hipMemcpyAsync(dst, from, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
        };
        ORYON_CHECK_HIP(copy(out->compat, ws.compat, rows * (n_cap / 32) * sizeof(uint32_t)));
        ORYON_CHECK_HIP(copy(out->conf, ws.conf, rows * sizeof(float)));
        ORYON_CHECK_HIP(copy(out->seeds, ws.seeds, seeds * sizeof(int32_t)));
        ORYON_CHECK_HIP(copy(out->n_seeds, ws.n_seeds, (size_t)B * sizeof(int32_t)));
        ORYON_CHECK_HIP(copy(out->sets, ws.sets, seeds * k * sizeof(int32_t)));
        ORYON_CHECK_HIP(copy(out->Mmat, ws.Mmat, seeds * k * k * sizeof(float)));
        ORYON_CHECK_HIP(copy(out->close, ws.close_hist, seeds * nit * sizeof(int32_t)));
        ORYON_CHECK_HIP(copy(out->seed_T, ws.seed_T, seeds * 16 * sizeof(float)));
        ORYON_CHECK_HIP(copy(out->fitness, ws.fitness, seeds * sizeof(float)));
        ORYON_CHECK_HIP(copy(out->best, ws.best, (size_t)B * sizeof(int32_t)));
        ORYON_CHECK_HIP(copy(out->T0, ws.T0, (size_t)B * 16 * sizeof(float)));
    }
    return ORYON_OK;
}
}  // namespace
}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_spectral_workspace_bytes(const oryon_spectral_config_t *cfg, int B, int n_cap)
{
    if (!supported(cfg, B, n_cap)) return 0;
    return carve_spectral(*cfg, B, n_cap, nullptr, nullptr);
}

// argument checks of both entries, before any launch; every rejection names its check
#define SPECTRAL_COMMON_CHECKS()                                                                                                     \
    ORYON_CHECK_ARG(cfg);                                                                                                            \
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);                                                                                           \
    ORYON_CHECK_ARG(n_cap > 0 && n_cap % 128 == 0);                                                                                  \
    if (n_cap > SP_MAX_ROWS) { set_error("%s: n_cap = %d exceeds %d rows per pair (LDS budget of the confidence kernel)", __func__, n_cap, SP_MAX_ROWS); return ORYON_ERR_INVALID_ARG; } \
    ORYON_CHECK_ARG(cfg->k >= 2 && cfg->k <= 63);                                                                                    \
    ORYON_CHECK_ARG(cfg->num_iterations >= 1 && cfg->num_iterations <= 16);                                                          \
    ORYON_CHECK_ARG(cfg->ratio > 0.0f && cfg->ratio <= 1.0f);                                                                        \
    ORYON_CHECK_ARG(cfg->inlier_threshold > 0.0f && cfg->sigma_d > 0.0f && cfg->nms_radius >= 0.0f);                                 \
    if (B == 0) return ORYON_OK;                                                                                                     \
    ORYON_CHECK_ARG(src && tgt && n);                                                                                                \
    SpectralWs ws;                                                                                                                   \
    ORYON_CHECK_WORKSPACE("%s: spectral ", workspace, workspace_bytes, carve_spectral(*cfg, B, n_cap, nullptr, nullptr), __func__);  \
    carve_spectral(*cfg, B, n_cap, workspace, &ws);

extern "C" int oryon_spectral_register(const oryon_spectral_config_t *cfg, const float *src, const float *tgt, const int32_t *n, int B,
                                       int n_cap, const int32_t *status_in, void *workspace, size_t workspace_bytes, float *T,
                                       uint8_t *labels, int32_t *status_out, void *stream)
{
    SPECTRAL_COMMON_CHECKS();
    ORYON_CHECK_ARG(T);
    return run_spectral(__func__, *cfg, src, tgt, n, B, n_cap, status_in, ws, T, labels, status_out, nullptr, as_stream(stream));
}

extern "C" int oryon_spectral_stages(const oryon_spectral_config_t *cfg, const float *src, const float *tgt, const int32_t *n, int B,
                                     int n_cap, const int32_t *status_in, void *workspace, size_t workspace_bytes, uint32_t *compat,
                                     float *conf, int32_t *seeds, int32_t *n_seeds, int32_t *sets, int32_t *scores, float *Mmat,
                                     int32_t *close, float *seed_T, float *fitness, int32_t *best, float *T0, float *T,
                                     int32_t *status_out, void *stream)
{
    SPECTRAL_COMMON_CHECKS();
    const SpectralOut out{compat, conf, seeds, n_seeds, sets, scores, Mmat, close, seed_T, fitness, best, T0};
    return run_spectral(__func__, *cfg, src, tgt, n, B, n_cap, status_in, ws, T, nullptr, status_out, &out, as_stream(stream));
}
