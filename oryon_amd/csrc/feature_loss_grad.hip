// Training step: the backward pass of the contrastive terms of FeatureLoss.forward (losses.py:64-141) and of its dice mask loss
// (losses.py:40-62, utils/losses/dice.py:27-89).  Definition: include/oryon_hip.h, oryon_feature_loss_grad / oryon_mask_dice_grad.
//
// The map gradient is a scatter of 2 N C-vectors per (pair, side) into an NCHW map with repeated pixels.  It is done without float
// atomics, in two launches and one memset, so the bytes of the result depend on nothing but the pair's inputs:
//
//   feature_loss_grad_rows_kernel    : grid (ceil(N / 64), side, pair), 64 threads, one thread per correspondence n.  The thread reads
//       its three descriptors (u: the side's positive, v: the other side's positive, w: the side's negative) from the NCHW maps
//       twice: once for |u|^2, |v|^2, |w|^2, <u,v>, <u,w> (float64, k-ordered fma), once to form the two contribution vectors
//           slot n     = alpha d d_pos / d u + beta d d(u,w) / d u            slot N + n = beta d d(u,w) / d w
//       in float64, rounded once to fp32, into the workspace as [C][2 N] (lanes write neighbouring slots).  A row that the strict
//       margin test on the forward's own fp32 d_pos / d_neg leaves out contributes zeros.  V, the number of pairs with valid == 1,
//       is counted by every block itself (an integer count: the same in every block).
//   feature_loss_grad_scatter_kernel : grid (ceil(2 N / 256), side, pair), 256 threads, one thread per slot.  The block holds the
//       (pair, side)'s 2 N pixel keys in LDS; a slot owns its pixel if no lower slot has the same key; every slot finds the next
//       higher slot of its key (a chain in LDS).  The owner walks its chain once per channel - ascending slot order, fp32 adds - and
//       stores the sum into the map, which a memset on the same stream has zeroed.  Every pixel has exactly one writer.
//   mask_dice_grad_kernel            : element-wise, float64 per element from the forward's four float64 sums, stored as fp32.
#include "common.h"

#pragma clang fp contract(off)

namespace oryon {
namespace {
constexpr int FG_ROWS = 64;                // correspondences per block of the rows kernel
constexpr int FG_SLOTS = 256;              // slots per block of the scatter kernel
constexpr int FG_MAX_C = 256;
constexpr int FG_MAX_N = 4096;             // 2 N keys + 2 N links in LDS: 16 N bytes = 64 KB
constexpr double FG_EPS = 1e-8;

__device__ __forceinline__ int clamped_pixel(const int32_t *c, int FH, int FW)
{
    return min(max(c[0], 0), FH - 1) * FW + min(max(c[1], 0), FW - 1);
}

__global__ __launch_bounds__(FG_ROWS) void feature_loss_grad_rows_kernel(const float *__restrict__ feat_a, const float *__restrict__ feat_q, int B, int C,
                                                                         int FH, int FW, const int32_t *__restrict__ corrs, int n_corr,
                                                                         const int32_t *__restrict__ valid, const int32_t *__restrict__ neg_idx,
                                                                         const float *__restrict__ d_pos, const float *__restrict__ d_neg,
                                                                         const float *__restrict__ g, float pos_margin, float neg_margin,
                                                                         float *__restrict__ rows)
{
    const int t = threadIdx.x, side = blockIdx.y, b = blockIdx.z, n = blockIdx.x * FG_ROWS + t;
    if (valid[b] != 1) return;                              // the map stays zero, the scatter kernel leaves it alone too
    int V = 0;
    for (int i = t; i < B; i += FG_ROWS) V += valid[i] == 1 ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) V += __shfl_xor(V, off);
    if (n >= n_corr) return;

    const size_t HW = (size_t)FH * FW;
    const int32_t *c = corrs + ((size_t)b * n_corr + n) * 4;
    const float *fu = (side == 0 ? feat_a : feat_q) + (size_t)b * C * HW;
    const float *fv = (side == 0 ? feat_q : feat_a) + (size_t)b * C * HW;
    const float *pu = fu + clamped_pixel(c + 2 * side, FH, FW);
    const float *pv = fv + clamped_pixel(c + 2 * (1 - side), FH, FW);
    const size_t row = ((size_t)b * 2 + side) * n_corr + n;
    const int wi = neg_idx[row];
    const bool has_w = wi >= 0 && (size_t)wi < HW;          // a negative that names no pixel is a row of zeros (the forward's rule)
    const float *pw = fu + (has_w ? wi : 0);

    double uu = 0.0, vv = 0.0, ww = 0.0, uv = 0.0, uw = 0.0;
    for (int k = 0; k < C; ++k) {
        const double u = (double)pu[k * HW], v = (double)pv[k * HW], w = has_w ? (double)pw[k * HW] : 0.0;
        uu = fma(u, u, uu); vv = fma(v, v, vv); ww = fma(w, w, ww);
        uv = fma(u, v, uv); uw = fma(u, w, uw);
    }
    const double lu = sqrt(uu), lv = sqrt(vv), lw = sqrt(ww);
    const double nu = fmax(lu, FG_EPS), nv = fmax(lv, FG_EPS), nw = fmax(lw, FG_EPS);
    // a clamped norm is a constant: no projection term
    const double proj_u = lu >= FG_EPS ? 1.0 : 0.0, proj_w = lw >= FG_EPS ? 1.0 : 0.0;
    const double c_uv = uv / (nu * nv), c_uw = uw / (nu * nw);

    // strict relu subgradients, on the forward's own fp32 values and in the forward's fp32 subtraction
    const bool act_pos = d_pos[(size_t)b * n_corr + n] - pos_margin > 0.0f;
    const bool act_neg = neg_margin - d_neg[row] > 0.0f;
    const double vn = (double)V * (double)n_corr;
    // d = 0.5 (1 - cos): the -0.5 goes into the coefficients
    const double ca = act_pos ? -0.5 * ((double)g[0] / vn) : 0.0;
    const double cb = act_neg ? 0.5 * ((double)g[1 + side] / vn) : 0.0;

    float *out = rows + ((size_t)b * 2 + side) * C * 2 * n_corr;
    const size_t stride = 2 * (size_t)n_corr;
    for (int k = 0; k < C; ++k) {
        const double uh = (double)pu[k * HW] / nu, vh = (double)pv[k * HW] / nv, wh = has_w ? (double)pw[k * HW] / nw : 0.0;
        const double t_pos = act_pos ? ca * ((vh - proj_u * c_uv * uh) / nu) : 0.0;
        const double t_neg = act_neg ? cb * ((wh - proj_u * c_uw * uh) / nu) : 0.0;
        const double t_w = act_neg ? cb * ((uh - proj_w * c_uw * wh) / nw) : 0.0;
        out[k * stride + n] = (float)(t_pos + t_neg);
        out[k * stride + n_corr + n] = (float)t_w;
    }
}

__global__ __launch_bounds__(FG_SLOTS) void feature_loss_grad_scatter_kernel(const float *__restrict__ rows, int C, int FH, int FW,
                                                                            const int32_t *__restrict__ corrs, int n_corr,
                                                                            const int32_t *__restrict__ valid, const int32_t *__restrict__ neg_idx,
                                                                            float *__restrict__ grad_a, float *__restrict__ grad_q)
{
    extern __shared__ int fg_smem[];
    const int t = threadIdx.x, side = blockIdx.y, b = blockIdx.z, S = 2 * n_corr;
    if (valid[b] != 1) return;
    int *s_key = fg_smem, *s_next = fg_smem + S;
    const int HW = FH * FW;
    for (int i = t; i < S; i += FG_SLOTS) {
        int key;
        if (i < n_corr) {
            key = clamped_pixel(corrs + ((size_t)b * n_corr + i) * 4 + 2 * side, FH, FW);
        } else {
            key = neg_idx[((size_t)b * 2 + side) * n_corr + (i - n_corr)];
            if (key < 0 || key >= HW) key = -1;
        }
        s_key[i] = key;
    }
    __syncthreads();
    const int j = blockIdx.x * FG_SLOTS + t;
    const int key = j < S ? s_key[j] : -1;
    bool owner = key >= 0;
    if (key >= 0) {
        for (int i = 0; i < j; ++i) owner = owner && s_key[i] != key;
        int nx = -1;
        for (int i = j + 1; i < S; ++i)
            if (s_key[i] == key) { nx = i; break; }
        s_next[j] = nx;
    }
    __syncthreads();                                        // a chain may run into the slots of another wave of this block ...
    if (!owner) return;
    // ... and into slots of other blocks: those links are recomputed here, by the owner alone (rare: only chains that leave the block)
    const int hi = min((int)(blockIdx.x + 1) * FG_SLOTS, S);
    const float *src = rows + ((size_t)b * 2 + side) * C * S;
    float *dst = (side == 0 ? grad_a : grad_q) + (size_t)b * C * HW + key;
    for (int k = 0; k < C; ++k) {
        const float *r = src + (size_t)k * S;
        float acc = r[j];
        int i = s_next[j];
        while (i >= 0) {
            acc = acc + r[i];
            if (i < hi) {
                i = s_next[i];
            } else {                                        // past this block's slots: scan on
                int nx = -1;
                for (int m = i + 1; m < S; ++m)
                    if (s_key[m] == key) { nx = m; break; }
                i = nx;
            }
        }
        dst[(size_t)k * HW] = acc;
    }
}

__global__ __launch_bounds__(256) void mask_dice_grad_kernel(const float *__restrict__ logits, const int32_t *__restrict__ gt, int B, int HW,
                                                             const double *__restrict__ sums, const float *__restrict__ g_mask,
                                                             float *__restrict__ grad)
{
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const double hw = (double)HW;
    const double sp = sums[b * 4 + 0], spp = sums[b * 4 + 1], spt = sums[b * 4 + 2], st = sums[b * 4 + 3];
    const double Df = spp + st + 1.0, Nf = spt + 1.0;
    const double Db = (hw - 2.0 * sp + spp) + (hw - st) + 1.0, Nb = (hw - sp - st + spt) + 1.0;
    const size_t at = (size_t)b * HW + i;
    const double p = 1.0 / (1.0 + exp(-2.0 * (double)logits[at])), q = 1.0 - p;
    const double tg = gt[at] != 0 ? 1.0 : 0.0, ug = 1.0 - tg;
    const double fg = -tg / Df + 2.0 * p * Nf / (Df * Df);
    const double bg = -ug / Db + 2.0 * q * Nb / (Db * Db);
    grad[at] = (float)((double)g_mask[0] * (0.25 / (double)B) * 2.0 * p * q * (fg - bg));
}
}  // namespace
}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_feature_loss_grad_workspace_bytes(int B, int C, int n_corr)
{
    if (B <= 0 || B > 65535 || C <= 0 || C > FG_MAX_C || n_corr <= 0 || n_corr > FG_MAX_N) return 0;
    return align256((size_t)B * 2 * C * 2 * n_corr * sizeof(float));      // the 2 N contribution vectors of every (pair, side)
}

extern "C" int oryon_feature_loss_grad(const float *feat_a, const float *feat_q, int B, int C, int FH, int FW, const int32_t *corrs, int n_corr,
                                       const int32_t *valid, const int32_t *neg_idx, const float *d_pos, const float *d_neg, const float *g,
                                       float pos_margin, float neg_margin, void *workspace, size_t workspace_bytes, float *grad_a,
                                       float *grad_q, void *stream)
{
    ORYON_CHECK_ARG(B >= 0 && B <= 65535 && C > 0 && FH > 0 && FW > 0 && n_corr > 0);
    ORYON_CHECK_ARG((int64_t)FH * FW <= 0x7fffffff);
    if (C > FG_MAX_C) { set_error("%s: C = %d exceeds %d channels (the forward's range)", __func__, C, FG_MAX_C); return ORYON_ERR_INVALID_ARG; }
    if (n_corr > FG_MAX_N) { set_error("%s: n_corr = %d exceeds %d correspondences (LDS budget of the pixel keys)", __func__, n_corr, FG_MAX_N); return ORYON_ERR_INVALID_ARG; }
    if (B == 0) return ORYON_OK;
    ORYON_CHECK_ARG(feat_a && feat_q && corrs && valid && neg_idx && d_pos && d_neg && g && grad_a && grad_q);
    ORYON_CHECK_WORKSPACE("feature-loss gradient ", workspace, workspace_bytes, oryon_feature_loss_grad_workspace_bytes(B, C, n_corr));
    hipStream_t st = as_stream(stream);
    const size_t map_bytes = (size_t)B * C * FH * FW * sizeof(float);
    ORYON_CHECK_HIP(hipMemsetAsync(grad_a, 0, map_bytes, st));
    ORYON_CHECK_HIP(hipMemsetAsync(grad_q, 0, map_bytes, st));
    float *rows = static_cast<float *>(workspace);
    hipLaunchKernelGGL(feature_loss_grad_rows_kernel, dim3(ceil_div(n_corr, FG_ROWS), 2, B), dim3(FG_ROWS), 0, st, feat_a, feat_q, B, C, FH, FW,
                       corrs, n_corr, valid, neg_idx, d_pos, d_neg, g, pos_margin, neg_margin, rows);
    ORYON_CHECK_LAUNCH();
    const size_t dyn = (size_t)4 * n_corr * sizeof(int);
    hipLaunchKernelGGL(feature_loss_grad_scatter_kernel, dim3(ceil_div(2 * n_corr, FG_SLOTS), 2, B), dim3(FG_SLOTS), dyn, st, rows, C, FH, FW,
                       corrs, n_corr, valid, neg_idx, grad_a, grad_q);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_mask_dice_grad(const float *logits, const int32_t *gt, int B, int H, int W, const double *sums, const float *g_mask,
                                    float *grad_logits, void *stream)
{
    ORYON_CHECK_ARG(B >= 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff);
    if (B == 0) return ORYON_OK;
    ORYON_CHECK_ARG(logits && gt && sums && g_mask && grad_logits);
    hipLaunchKernelGGL(mask_dice_grad_kernel, dim3(ceil_div(H * W, 256), B), dim3(256), 0, as_stream(stream), logits, gt, B, H * W, sums, g_mask,
                       grad_logits);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
