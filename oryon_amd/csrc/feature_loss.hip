// Validation step: the contrastive terms of FeatureLoss.forward (losses.py:64-141) and the sums behind its dice mask loss
// (losses.py:40-62, utils/losses/dice.py:27-89), for a whole batch in four launches and no host round trip.
//
// Everything is fp32 and follows the reference as it runs on the CPU; the cosine is the matcher's form (rows divided by
// max(|x|, 1e-8) with the k-ordered fmaf norm of gather_normalise_kernel, then a k-ordered fmaf dot product).
//
//   feature_loss_kernel        : grid (ceil(n_corr / 64), side, pair), 256 threads.  The block gathers its 64 positives from the NCHW map
//       and keeps their unit rows in LDS as [C][64].  pool_mode 0 (hardest negatives, losses.py:165-220): the pool (every pixel in
//       row-major order, or the 2000 sampled pixels of the pool table) is streamed through LDS in tiles of 64 unit rows [C][64]; a thread
//       owns 4 positives x 4 candidates (two ds_read_b128 per channel feed 16 fmaf) and keeps the running minimum of
//           cost = 0.5 (1 - cos) + 1e6 relu(neg_kernel - sqrt(dy^2 + dx^2 + 1e-7))          (losses.py:205-211, utils/pcd.py:22-25)
//       per positive, evaluated in fp32 exactly as written (no contraction, correctly rounded sqrt); ties go to the lowest pool
//       position: strict < inside a thread, which walks the pool in ascending order, and (cost, position) order when the sixteen
//       threads of a positive are merged.  pool_mode 1 (losses.py:222-263, loss.hard_negatives = False): pool[n] IS the negative of
//       positive n.  The side-0 blocks also write d_pos (losses.py:91).  Plain FMAs, not the fp32 MFMA chain of match.hip: both run at
//       the same peak on this part, and the 4 x 4 register tile needs 16 accumulators where the 32x32x2 MFMA needs its operands in
//       the MFMA lane layout (an LDS image per k pair); the kernel is bound by the pool gather at C = 32 either way.
//   feature_loss_finish_kernel : one wave per pair: mean_n relu(d_pos - pos_margin), mean_n relu(neg_margin - d_neg) per side
//       (losses.py:95-101) in a fixed order (lane-strided float64 sums, xor-shuffle tree) -> pair_terms [B,3].
//   feature_loss_batch_kernel  : one wave: the means over the pairs with valid == 1 (losses.py:103-111), 0 when there is none.
//   mask_dice_kernel           : one block per image, one pass: sum p, sum p^2, sum p t, sum t with p = sigmoid(2x) (the softmax over
//       (x, -x) of dice.py:69-78) in float64 by a fixed-order tree, the thresholded mask (the expression of mask_from_logits_kernel)
//       and the intersection / union counts of mask_iou (utils/metrics.py:18-40).
// No float atomics anywhere: every output is a pure function of the pair's inputs, whatever the stream or the batch around it.
#include "common.h"

#pragma clang fp contract(off)

namespace oryon {
namespace {
constexpr int FL_THREADS = 256;
constexpr int FL_TP = 64;                  // positives per block
constexpr int FL_TJ = 64;                  // pool candidates per LDS tile
constexpr int FL_MAX_C = 256;              // dynamic LDS = 2 * 64 * C floats = 128 KB at C = 256
constexpr int MD_THREADS = 512;

// 64 rows of the NCHW map `f` at the pixels pix[0..63] (-1: a row of zeros) -> dst [C][64] as unit rows.  Called by the whole block.
__device__ __forceinline__ void load_unit_rows(const float *__restrict__ f, int C, size_t HW, const int *pix, float *dst, float *s_d)
{
    const int t = threadIdx.x;
    for (int i = t; i < C * 64; i += FL_THREADS) {
        const int p = pix[i & 63];
        dst[i] = p >= 0 ? f[(size_t)(i >> 6) * HW + p] : 0.0f;
    }
    __syncthreads();
    if (t < 64) {
        float n2 = 0.0f;
        for (int k = 0; k < C; ++k) {
            const float v = dst[k * 64 + t];
            n2 = __fmaf_rn(v, v, n2);
        }
        const float d = sqrt_rn(n2);
        s_d[t] = d < 1e-8f ? 1e-8f : d;
    }
    __syncthreads();
    for (int i = t; i < C * 64; i += FL_THREADS) dst[i] = __fdiv_rn(dst[i], s_d[i & 63]);
    __syncthreads();
}

// 0.5 (1 - <a_t, b_t>) of column t of two [C][64] images (threads 0..63)
__device__ __forceinline__ float column_distance(const float *a, const float *b, int C, int t)
{
    float acc = 0.0f;
    for (int k = 0; k < C; ++k) acc = __fmaf_rn(a[k * 64 + t], b[k * 64 + t], acc);
    return 0.5f * (1.0f - acc);
}

__device__ __forceinline__ bool better(float c, int j, float c0, int j0) { return c < c0 || (c == c0 && j < j0); }

__global__ __launch_bounds__(FL_THREADS) void feature_loss_kernel(const float *__restrict__ feat_a, const float *__restrict__ feat_q, int C,
                                                                  int FH, int FW, const int32_t *__restrict__ corrs, int n_corr,
                                                                  const int32_t *__restrict__ valid, const int32_t *__restrict__ pool,
                                                                  int n_pool, int pool_mode, float neg_kernel, float *__restrict__ d_pos,
                                                                  float *__restrict__ d_neg, int32_t *__restrict__ neg_idx)
{
    extern __shared__ float4 fl_smem[];
    float *s_pos = reinterpret_cast<float *>(fl_smem), *s_pool = s_pos + (size_t)C * FL_TP;
    __shared__ float s_d[64];
    __shared__ int s_pix[FL_TP], s_py[FL_TP], s_px[FL_TP];
    __shared__ int s_cpix[FL_TJ];
    __shared__ float s_cy[FL_TJ], s_cx[FL_TJ];
    __shared__ float s_rc[4][FL_TP], s_rd[4][FL_TP];
    __shared__ int s_rj[4][FL_TP];

    const int t = threadIdx.x, side = blockIdx.y, b = blockIdx.z, p0 = blockIdx.x * FL_TP;
    const int HW = FH * FW;
    const size_t out_row = ((size_t)b * 2 + side) * n_corr;
    if (valid[b] != 1) {                                    // losses.py:158,189: the pair is left at zero
        if (t < FL_TP && p0 + t < n_corr) {
            d_neg[out_row + p0 + t] = 0.0f;
            neg_idx[out_row + p0 + t] = 0;
            if (side == 0) d_pos[(size_t)b * n_corr + p0 + t] = 0.0f;
        }
        return;
    }
    const float *f = (side == 0 ? feat_a : feat_q) + (size_t)b * C * HW;
    if (t < FL_TP) {
        const int n = p0 + t;
        int pix = -1, y = 0, x = 0;
        if (n < n_corr) {
            const int32_t *c = corrs + ((size_t)b * n_corr + n) * 4 + 2 * side;
            y = min(max(c[0], 0), FH - 1);
            x = min(max(c[1], 0), FW - 1);
            pix = y * FW + x;
        }
        s_pix[t] = pix; s_py[t] = y; s_px[t] = x;
    }
    __syncthreads();
    load_unit_rows(f, C, HW, s_pix, s_pos, s_d);

    const int32_t *pl = pool ? pool + ((size_t)b * 2 + side) * n_pool : nullptr;
    if (pool_mode == 0) {
        const int P = pool ? n_pool : HW;
        const int tp = t & 15, tj = t >> 4;                 // positives 4 tp .. 4 tp + 3, candidates 4 tj .. 4 tj + 3 of the tile
        float best_c[4], best_d[4], py[4], px[4];
        int best_j[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            best_c[i] = INFINITY; best_d[i] = 0.0f; best_j[i] = -1;
            py[i] = (float)s_py[4 * tp + i]; px[i] = (float)s_px[4 * tp + i];
        }
        for (int j0 = 0; j0 < P; j0 += FL_TJ) {
            if (t < FL_TJ) {
                const int j = j0 + t;
                int pix = -1;
                if (j < P) {
                    pix = pl ? pl[j] : j;
                    if (pix < 0 || pix >= HW) pix = -1;     // a position that names no pixel never wins
                }
                s_cpix[t] = pix;
                s_cy[t] = (float)(pix >= 0 ? pix / FW : 0);
                s_cx[t] = (float)(pix >= 0 ? pix % FW : 0);
            }
            __syncthreads();
            load_unit_rows(f, C, HW, s_cpix, s_pool, s_d);
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
            const float4 *A4 = reinterpret_cast<const float4 *>(s_pos) + tp, *Q4 = reinterpret_cast<const float4 *>(s_pool) + tj;
#pragma unroll 4
            for (int k = 0; k < C; ++k) {
                const float4 a = A4[k * 16], q = Q4[k * 16];
                const float av[4] = {a.x, a.y, a.z, a.w}, qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __fmaf_rn(av[i], qv[j], acc[i][j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cj = 4 * tj + j;
                if (s_cpix[cj] < 0) continue;
                const float cy = s_cy[cj], cx = s_cx[cj];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d = 0.5f * (1.0f - acc[i][j]);
                    const float dy = py[i] - cy, dx = px[i] - cx;
                    const float pd = sqrt_rn((dy * dy + dx * dx) + 1e-7f);
                    const float cost = d + 1e6f * fmaxf(neg_kernel - pd, 0.0f);
                    if (cost < best_c[i]) { best_c[i] = cost; best_d[i] = d; best_j[i] = j0 + cj; }
                }
            }
            __syncthreads();                                // the next tile overwrites s_pool / s_cpix
        }
        // merge the sixteen threads of a positive: lanes l, l ^ 16, l ^ 32 of a wave, then the four waves through LDS
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                const float oc = __shfl_xor(best_c[i], off), od = __shfl_xor(best_d[i], off);
                const int oj = __shfl_xor(best_j[i], off);
                if (oj >= 0 && (best_j[i] < 0 || better(oc, oj, best_c[i], best_j[i]))) { best_c[i] = oc; best_d[i] = od; best_j[i] = oj; }
            }
            if ((t & 63) < 16) { s_rc[t >> 6][4 * tp + i] = best_c[i]; s_rd[t >> 6][4 * tp + i] = best_d[i]; s_rj[t >> 6][4 * tp + i] = best_j[i]; }
        }
        __syncthreads();
        if (t < FL_TP && p0 + t < n_corr) {
            float c = s_rc[0][t], d = s_rd[0][t];
            int j = s_rj[0][t];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const int oj = s_rj[w][t];
                if (oj >= 0 && (j < 0 || better(s_rc[w][t], oj, c, j))) { c = s_rc[w][t]; d = s_rd[w][t]; j = oj; }
            }
            // j < 0: no candidate had a comparable cost (an empty pool, or NaN descriptors): NaN, pixel 0
            d_neg[out_row + p0 + t] = j >= 0 ? d : NAN;
            neg_idx[out_row + p0 + t] = j >= 0 ? (pl ? pl[j] : j) : 0;
        }
        __syncthreads();
    } else {
        if (t < FL_TP) {
            const int n = p0 + t;
            int pix = n < n_corr ? pl[n] : -1;
            if (pix < 0 || pix >= HW) pix = -1;
            s_cpix[t] = pix;
        }
        __syncthreads();
        load_unit_rows(f, C, HW, s_cpix, s_pool, s_d);
        if (t < FL_TP && p0 + t < n_corr) {
            d_neg[out_row + p0 + t] = column_distance(s_pos, s_pool, C, t);      // a position that names no pixel: a zero row, 0.5
            neg_idx[out_row + p0 + t] = s_cpix[t];
        }
        __syncthreads();
    }

    if (side == 0) {                                        // losses.py:91: the positive term, against the query map
        if (t < FL_TP) {
            const int n = p0 + t;
            int pix = -1;
            if (n < n_corr) {
                const int32_t *c = corrs + ((size_t)b * n_corr + n) * 4 + 2;
                pix = min(max(c[0], 0), FH - 1) * FW + min(max(c[1], 0), FW - 1);
            }
            s_cpix[t] = pix;
        }
        __syncthreads();
        load_unit_rows(feat_q + (size_t)b * C * HW, C, HW, s_cpix, s_pool, s_d);
        if (t < FL_TP && p0 + t < n_corr) d_pos[(size_t)b * n_corr + p0 + t] = column_distance(s_pos, s_pool, C, t);
    }
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(64) void feature_loss_finish_kernel(const float *__restrict__ d_pos, const float *__restrict__ d_neg,
                                                                 const int32_t *__restrict__ valid, int n_corr, float pos_margin,
                                                                 float neg_margin, float *__restrict__ pair_terms, double *__restrict__ pair_sums)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    if (valid[b] == 1) {
        const float *dp = d_pos + (size_t)b * n_corr, *da = d_neg + (size_t)b * 2 * n_corr, *dq = da + n_corr;
        for (int n = lane; n < n_corr; n += 64) {
            s[0] += (double)fmaxf(dp[n] - pos_margin, 0.0f);
            s[1] += (double)fmaxf(neg_margin - da[n], 0.0f);
            s[2] += (double)fmaxf(neg_margin - dq[n], 0.0f);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = wave_sum_f64(s[i]) / (double)n_corr;
    }
    if (lane < 3) {
        const double v = lane == 0 ? s[0] : lane == 1 ? s[1] : s[2];
        pair_sums[(size_t)b * 3 + lane] = v;
        pair_terms[(size_t)b * 3 + lane] = (float)v;
    }
}

__global__ __launch_bounds__(64) void feature_loss_batch_kernel(const double *__restrict__ pair_sums, const int32_t *__restrict__ valid, int B,
                                                                float *__restrict__ losses)
{
    const int lane = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    for (int b = lane; b < B; b += 64)
        if (valid[b] == 1) {
            ++cnt;
#pragma unroll
            for (int i = 0; i < 3; ++i) s[i] += pair_sums[(size_t)b * 3 + i];
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
#pragma unroll
    for (int i = 0; i < 3; ++i) s[i] = wave_sum_f64(s[i]);
    if (lane < 3) {
        const double v = lane == 0 ? s[0] : lane == 1 ? s[1] : s[2];
        losses[lane] = cnt > 0 ? (float)(v / (double)cnt) : 0.0f;
    }
}

__global__ __launch_bounds__(MD_THREADS) void mask_dice_kernel(const float *__restrict__ logits, const int32_t *__restrict__ gt, int HW, float thr,
                                                               double *__restrict__ sums, int32_t *__restrict__ mask, int32_t *__restrict__ counts)
{
    __shared__ double s_s[MD_THREADS / 64][4];
    __shared__ int s_c[MD_THREADS / 64][2];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float *x = logits + (size_t)b * HW;
    const int32_t *g = gt + (size_t)b * HW;
    int32_t *m = mask + (size_t)b * HW;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int inter = 0, uni = 0;
    for (int i = t; i < HW; i += MD_THREADS) {
        const float xi = x[i];
        const bool tg = g[i] != 0;
        const double p = 1.0 / (1.0 + exp(-2.0 * (double)xi));
        s[0] += p;
        s[1] += p * p;
        s[2] += tg ? p : 0.0;
        s[3] += tg ? 1.0 : 0.0;
        const float sg = 1.0f / (1.0f + expf(-xi));         // mask_from_logits_kernel's expression
        const bool on = sg > thr;
        m[i] = on ? 1 : 0;
        inter += (on && tg) ? 1 : 0;
        uni += (on || tg) ? 1 : 0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = wave_sum_f64(s[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        inter += __shfl_xor(inter, off);
        uni += __shfl_xor(uni, off);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s_s[wave][i] = s[i];
        s_c[wave][0] = inter; s_c[wave][1] = uni;
    }
    __syncthreads();
    if (t < 4) {
        double v = s_s[0][t];
        for (int w = 1; w < MD_THREADS / 64; ++w) v += s_s[w][t];
        sums[(size_t)b * 4 + t] = v;
    } else if (t < 6) {
        int v = 0;
        for (int w = 0; w < MD_THREADS / 64; ++w) v += s_c[w][t - 4];
        counts[(size_t)b * 2 + (t - 4)] = v;
    }
}
}  // namespace
}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_feature_loss_workspace_bytes(int B, int n_corr, int n_pool)
{
    if (B <= 0 || B > 65535 || n_corr <= 0 || n_pool < 0) return 0;
    return align256((size_t)B * 3 * sizeof(double));           // the pairs' float64 means between the finish and the batch kernel
}

extern "C" int oryon_feature_loss(const float *feat_a, const float *feat_q, int B, int C, int FH, int FW, const int32_t *corrs, int n_corr,
                                  const int32_t *valid, const int32_t *pool, int n_pool, int pool_mode, float pos_margin, float neg_margin,
                                  float neg_kernel, void *workspace, size_t workspace_bytes, float *d_pos, float *d_neg, int32_t *neg_idx,
                                  float *pair_terms, float *losses, void *stream)
{
    ORYON_CHECK_ARG(B >= 0 && B <= 65535 && C > 0 && FH > 0 && FW > 0 && n_corr > 0 && n_pool >= 0);
    ORYON_CHECK_ARG((int64_t)FH * FW <= 0x7fffffff);
    ORYON_CHECK_ARG(pool_mode == 0 || pool_mode == 1);
    if (C > FL_MAX_C) { set_error("%s: C = %d exceeds %d channels (LDS budget of the positives' and the pool tile's unit rows)", __func__, C, FL_MAX_C); return ORYON_ERR_INVALID_ARG; }
    ORYON_CHECK_ARG(pool ? n_pool > 0 : pool_mode == 0);
    ORYON_CHECK_ARG(pool_mode == 0 || n_pool == n_corr);
    ORYON_CHECK_ARG(losses);
    hipStream_t st = as_stream(stream);
    if (B == 0) {                                           // losses.py:108-111
        ORYON_CHECK_HIP(hipMemsetAsync(losses, 0, 3 * sizeof(float), st));
        return ORYON_OK;
    }
    ORYON_CHECK_ARG(feat_a && feat_q && corrs && valid && d_pos && d_neg && neg_idx && pair_terms);
    ORYON_CHECK_WORKSPACE("feature-loss ", workspace, workspace_bytes, oryon_feature_loss_workspace_bytes(B, n_corr, n_pool));
    double *pair_sums = static_cast<double *>(workspace);
    const size_t dyn = (size_t)C * (FL_TP + FL_TJ) * sizeof(float);
    // the opt-in is made once per (kernel, device), so it is for the largest C, not for this call's: the next call may have more channels
    allow_dynamic_lds(reinterpret_cast<const void *>(&feature_loss_kernel), (int)(FL_MAX_C * (FL_TP + FL_TJ) * sizeof(float)));
    hipLaunchKernelGGL(feature_loss_kernel, dim3(ceil_div(n_corr, FL_TP), 2, B), dim3(FL_THREADS), dyn, st, feat_a, feat_q, C, FH, FW, corrs, n_corr,
                       valid, pool, n_pool, pool_mode, neg_kernel, d_pos, d_neg, neg_idx);
    ORYON_CHECK_LAUNCH();
    hipLaunchKernelGGL(feature_loss_finish_kernel, dim3(B), dim3(64), 0, st, d_pos, d_neg, valid, n_corr, pos_margin, neg_margin, pair_terms, pair_sums);
    ORYON_CHECK_LAUNCH();
    hipLaunchKernelGGL(feature_loss_batch_kernel, dim3(1), dim3(64), 0, st, pair_sums, valid, B, losses);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_mask_dice_sums(const float *logits, const int32_t *gt, int B, int H, int W, float threshold, double *sums, int32_t *mask,
                                    int32_t *counts, void *stream)
{
    ORYON_CHECK_ARG(B >= 0 && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff);
    if (B == 0) return ORYON_OK;
    ORYON_CHECK_ARG(logits && gt && sums && mask && counts);
    hipLaunchKernelGGL(mask_dice_kernel, dim3(B), dim3(MD_THREADS), 0, as_stream(stream), logits, gt, H * W, threshold, sums, mask, counts);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
