// Sub-pixel refinement of the selected correspondences (test.subpixel; no counterpart in the reference) and K2 with the offsets.
//   oryon_subpix_refine      the facet fit: a least-squares quadratic through the cosine distance of the anchor descriptor to the 3 x 3
//                            query pixels around the matched one, its minimum as a (dy, dx) offset, three gates (include/oryon_hip.h).
//                            One wave per row, lanes over channels, float64 partial sums, xor butterfly: every lane ends with the same
//                            nineteen sums, in an order that depends on C alone - not on the batch position, the stream or the layout.
//   oryon_lift_pairs_subpix  lift_pairs_kernel (post.hip) on float query coordinates: bilinear depth where the four neighbours agree,
//                            the pixel K2 reads otherwise; one rounding per operation in the order the header states (K2's _rn
//                            intrinsics where no product meets a sum, uncontracted plain operators in the bilinear form).
// Both are latency-bound post-passes on <= 2048 rows per pair.  The map is addressed as base + c * chan_stride + pixel * pix_stride, so the
// two layouts share one kernel: on NHWC the lanes of a load read 256 contiguous bytes, on NCHW every lane reads its own channel plane -
// one cache line per (channel, map row), three neighbours of a row from the same line - which is what that layout costs.
#include "common.h"

#pragma clang fp contract(off)

namespace oryon {

constexpr int SUBPIX_WAVES = 4;                     // rows per workgroup of the fit
constexpr int SUBPIX_THREADS = SUBPIX_WAVES * 64;
constexpr int SUBPIX_SUMS = 19;                     // <a, q_p> and <q_p, q_p> of the nine pixels, <a, a>
constexpr double SUBPIX_EPS = 1e-8;

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (ceil(n_cap / SUBPIX_WAVES), B).  Every row below n_cap is written: zeros past the count and for skipped pairs.
__global__ __launch_bounds__(SUBPIX_THREADS) void subpix_fit_kernel(
    const float *__restrict__ feat_a, const float *__restrict__ feat_q, int C, int FH, int FW, long chan_stride, long pix_stride,
    const int32_t *__restrict__ corrs, const int32_t *__restrict__ n_corr, const int32_t *__restrict__ status, int n_cap, double curv_min,
    float *__restrict__ offsets, uint8_t *__restrict__ flags)
{
    const int p = blockIdx.y;
    const int row = blockIdx.x * SUBPIX_WAVES + (int)(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n_cap) return;
    const size_t o = (size_t)p * n_cap + row;
    const bool skip = status && status[p] != ORYON_PAIR_OK;
    const int n = n_corr ? min(max(n_corr[p], 0), n_cap) : n_cap;
    if (skip || row >= n) {
        if (lane == 0) { offsets[2 * o] = 0.0f; offsets[2 * o + 1] = 0.0f; flags[o] = 0; }
        return;
    }
    const int4 cc = *reinterpret_cast<const int4 *>(corrs + o * 4);
    const int ya = cc.x, xa = cc.y, yq = cc.z, xq = cc.w;
    // border: the stencil would leave the query map (an anchor pixel outside its map reads nothing either)
    if (yq < 1 || yq > FH - 2 || xq < 1 || xq > FW - 2 || ya < 0 || ya >= FH || xa < 0 || xa >= FW) {
        if (lane == 0) { offsets[2 * o] = 0.0f; offsets[2 * o + 1] = 0.0f; flags[o] = 1; }
        return;
    }
    const size_t map = (size_t)p * C * FH * FW;
    const float *a = feat_a + map + ((size_t)ya * FW + xa) * pix_stride;
    const float *q = feat_q + map + ((size_t)(yq - 1) * FW + (xq - 1)) * pix_stride;       // the stencil's top-left pixel
    double s[SUBPIX_SUMS];
#pragma unroll
    for (int k = 0; k < SUBPIX_SUMS; ++k) s[k] = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double av = (double)a[(size_t)c * chan_stride];
        const float *qc = q + (size_t)c * chan_stride;
        s[18] += av * av;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double qv = (double)qc[((size_t)i * FW + j) * pix_stride];
                s[i * 3 + j] += av * qv;
                s[9 + i * 3 + j] += qv * qv;
            }
    }
#pragma unroll
    for (int k = 0; k < SUBPIX_SUMS; ++k) s[k] = wave_sum_f64(s[k]);
    if (lane != 0) return;
    const double na = fmax(sqrt(s[18]), SUBPIX_EPS);
    double f[3][3];                                   // f[i + 1][j + 1] = d(y_q + i, x_q + j)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) f[i][j] = 0.5 * (1.0 - s[i * 3 + j] / (na * fmax(sqrt(s[9 + i * 3 + j]), SUBPIX_EPS)));
    double gx = 0.0, gy = 0.0, hxx = 0.0, hyy = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gx += f[k][2] - f[k][0];
        gy += f[2][k] - f[0][k];
        hxx += f[k][2] - 2.0 * f[k][1] + f[k][0];
        hyy += f[2][k] - 2.0 * f[1][k] + f[0][k];
    }
    gx /= 6.0; gy /= 6.0; hxx /= 3.0; hyy /= 3.0;
    const double hxy = (f[2][2] - f[2][0] - f[0][2] + f[0][0]) / 4.0;
    const double dh = hxx - hyy;
    const double lmin = (hxx + hyy) / 2.0 - sqrt(dh * dh / 4.0 + hxy * hxy);
    const double det = hxx * hyy - hxy * hxy;
    const double ox = -(hyy * gx - hxy * gy) / det, oy = -(hxx * gy - hxy * gx) / det;
    int flag = 0;
    if (lmin < curv_min) flag = 2;
    else if (!(fmax(fabs(ox), fabs(oy)) <= 1.0)) flag = 3;        // a NaN (non-finite descriptors, det = 0) is outside as well
    float dy = 0.0f, dx = 0.0f;
    if (flag == 0) {
        dy = (float)fmin(fmax(oy, -0.5), 0.5);
        dx = (float)fmin(fmax(ox, -0.5), 0.5);
    }
    offsets[2 * o] = dy;
    offsets[2 * o + 1] = dx;
    flags[o] = (uint8_t)flag;
}

// One workgroup per pair: the rows per flag value below the count (integers: no order to fix).
__global__ __launch_bounds__(256) void subpix_count_kernel(const uint8_t *__restrict__ flags, const int32_t *__restrict__ n_corr,
                                                           const int32_t *__restrict__ status, int n_cap, int32_t *__restrict__ counts)
{
    __shared__ int s_cnt[4][4];
    const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool skip = status && status[p] != ORYON_PAIR_OK;
    const int n = skip ? 0 : (n_corr ? min(max(n_corr[p], 0), n_cap) : n_cap);
    int c[4] = {0, 0, 0, 0};
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        const int fl = i < n ? (int)flags[(size_t)p * n_cap + i] : -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] += __popcll(__ballot(fl == k));
    }
    if (lane == 0)
        for (int k = 0; k < 4; ++k) s_cnt[wave][k] = c[k];
    __syncthreads();
    if (threadIdx.x < 4) counts[p * 4 + threadIdx.x] = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
}

// The depth at float image coordinates (y, x) inside [0, H) x [0, W): bilinear over the four pixels around it when they exist, are
// all measured and lie within `jump` of each other, else the pixel K2 reads (a zero depth included).
__device__ __forceinline__ float subpix_depth(const float *__restrict__ d, int H, int W, float y, float x, float jump)
{
    const int i0 = (int)y, j0 = (int)x;
    const float z00 = d[(size_t)i0 * W + j0];
    if (i0 + 1 < H && j0 + 1 < W) {
        const float z01 = d[(size_t)i0 * W + j0 + 1], z10 = d[(size_t)(i0 + 1) * W + j0], z11 = d[(size_t)(i0 + 1) * W + j0 + 1];
        const float lo = fminf(fminf(z00, z01), fminf(z10, z11)), hi = fmaxf(fmaxf(z00, z01), fmaxf(z10, z11));
        if (z00 > 0.0f && z01 > 0.0f && z10 > 0.0f && z11 > 0.0f && hi - lo <= jump) {
            // plain operators, not __fmul_rn / __fadd_rn: those are inline functions of the HIP headers, compiled outside this file's
            // `fp contract(off)`, and a product of theirs next to a sum of theirs is fused into v_fmac_f32 once inlined (seen in the
            // ISA and as one-ulp differences on the device); operations written here carry no contraction flag
            const float fy = y - (float)i0, fx = x - (float)j0;
            const float gy = 1.0f - fy, gx = 1.0f - fx;
            const float top = gx * z00 + fx * z01;
            const float bot = gx * z10 + fx * z11;
            return gy * top + fy * bot;
        }
    }
    return z00;
}

__device__ __forceinline__ void subpix_pinhole(float *__restrict__ out, float y, float x, float z, float fx, float cx, float fy, float cy)
{
    out[0] = __fdiv_rn(__fdiv_rn(__fmul_rn(__fsub_rn(x, cx), z), fx), 1000.0f);
    out[1] = __fdiv_rn(__fdiv_rn(__fmul_rn(__fsub_rn(y, cy), z), fy), 1000.0f);
    out[2] = __fdiv_rn(z, 1000.0f);
}

// K2 with the offsets: lift_pairs_kernel's workgroup per pair, compaction and zero tail (post.hip).
__global__ __launch_bounds__(512) void lift_pairs_subpix_kernel(
    const int32_t *__restrict__ corrs, const float *__restrict__ offsets, const int32_t *__restrict__ n_corr, int n_cap, float sya,
    float sxa, float syq, float sxq, const float *__restrict__ depth_a, int HA, int WA, const float *__restrict__ depth_q, int HQ, int WQ,
    const float *__restrict__ cam_a, const float *__restrict__ cam_q, const int32_t *__restrict__ status, float jump,
    float *__restrict__ pcd_a, float *__restrict__ pcd_q, int32_t *__restrict__ n_out)
{
    __shared__ int s_wave[8];
    const int p = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *oa = pcd_a + (size_t)p * n_cap * 3, *oq = pcd_q + (size_t)p * n_cap * 3;
    auto zero_from = [&](int first) {
        for (int e = first * 3 + (int)threadIdx.x; e < n_cap * 3; e += (int)blockDim.x) { oa[e] = 0.0f; oq[e] = 0.0f; }
    };
    if (status && status[p] != ORYON_PAIR_OK) {
        if (threadIdx.x == 0) n_out[p] = 0;
        zero_from(0);
        return;
    }
    const int n = n_corr ? min(max(n_corr[p], 0), n_cap) : n_cap;
    const int32_t *c = corrs + (size_t)p * n_cap * 4;
    const float *off = offsets ? offsets + (size_t)p * n_cap * 2 : nullptr;
    const float *da = depth_a + (size_t)p * HA * WA, *dq = depth_q + (size_t)p * HQ * WQ;
    const float fxa = cam_a[p * 9 + 0], cxa = cam_a[p * 9 + 2], fya = cam_a[p * 9 + 4], cya = cam_a[p * 9 + 5];
    const float fxq = cam_q[p * 9 + 0], cxq = cam_q[p * 9 + 2], fyq = cam_q[p * 9 + 4], cyq = cam_q[p * 9 + 5];
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += blockDim.x) {
        const int i = i0 + threadIdx.x;
        bool ok = false;
        float ya = 0, xa = 0, yq = 0, xq = 0;
        if (i < n) {
            const int4 cc = *reinterpret_cast<const int4 *>(c + (size_t)i * 4);
            const float dy = off ? off[2 * i] : 0.0f, dx = off ? off[2 * i + 1] : 0.0f;
            ya = __fmul_rn((float)cc.x, sya); xa = __fmul_rn((float)cc.y, sxa);
            yq = __fmul_rn(__fadd_rn((float)cc.z, dy), syq); xq = __fmul_rn(__fadd_rn((float)cc.w, dx), sxq);
            // a NaN offset fails every comparison: the row is dropped before anything is indexed with it
            ok = ya >= 0.0f && ya < (float)HA && xa >= 0.0f && xa < (float)WA && yq >= 0.0f && yq < (float)HQ &&
                 xq >= 0.0f && xq < (float)WQ;
        }
        // ordered rank of the kept rows (block_rank_sel of post.hip)
        const unsigned long long b = __ballot(ok);
        __syncthreads();
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int r = __popcll(b & ((1ull << lane) - 1ull)), tot = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) {
            const int cw = s_wave[w];
            r += (w < wave) ? cw : 0;
            tot += cw;
        }
        if (ok) {
            const int o = (base + r) * 3;
            subpix_pinhole(oa + o, ya, xa, subpix_depth(da, HA, WA, ya, xa, jump), fxa, cxa, fya, cya);
            subpix_pinhole(oq + o, yq, xq, subpix_depth(dq, HQ, WQ, yq, xq, jump), fxq, cxq, fyq, cyq);
        }
        base += tot;
    }
    if (threadIdx.x == 0) n_out[p] = base;
    zero_from(base);
}

}  // namespace oryon

using namespace oryon;

extern "C" int oryon_subpix_refine(const float *feat_a, const float *feat_q, int B, int C, int FH, int FW, int layout, const int32_t *corrs,
                                   const int32_t *n_corr, const int32_t *status, int n_cap, float curv_min, float *offsets, uint8_t *flags,
                                   int32_t *counts, void *stream)
{
    ORYON_CHECK_ARG(feat_a && feat_q);
    ORYON_CHECK_ARG(corrs);
    ORYON_CHECK_ARG(offsets && flags && counts);
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);
    ORYON_CHECK_ARG(C >= 1);
    ORYON_CHECK_ARG(C <= 512);
    ORYON_CHECK_ARG(FH >= 1 && FW >= 1 && (long long)FH * FW <= (1ll << 30));
    ORYON_CHECK_ARG(layout == ORYON_LAYOUT_NCHW || layout == ORYON_LAYOUT_NHWC);
    ORYON_CHECK_ARG(n_cap >= 1 && n_cap <= (1 << 24));
    ORYON_CHECK_ARG(curv_min >= 0.0f);                   // a NaN fails too
    if (B == 0) return ORYON_OK;
    const bool nhwc = layout == ORYON_LAYOUT_NHWC;
    const long chan_stride = nhwc ? 1 : (long)FH * FW, pix_stride = nhwc ? C : 1;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(subpix_fit_kernel, dim3(ceil_div(n_cap, SUBPIX_WAVES), B), dim3(SUBPIX_THREADS), 0, st, feat_a, feat_q, C, FH, FW,
                       chan_stride, pix_stride, corrs, n_corr, status, n_cap, (double)curv_min, offsets, flags);
    ORYON_CHECK_LAUNCH();
    hipLaunchKernelGGL(subpix_count_kernel, dim3(B), dim3(256), 0, st, flags, n_corr, status, n_cap, counts);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_lift_pairs_subpix(const int32_t *corrs, const float *offsets, const int32_t *n_corr, int B, int n_cap, int FH, int FW,
                                       const float *depth_a, int HA, int WA, const float *depth_q, int HQ, int WQ, const float *cam_a,
                                       const float *cam_q, const int32_t *status, float depth_jump_mm, float *pcd_a, float *pcd_q,
                                       int32_t *n_out, void *stream)
{
    ORYON_CHECK_ARG(corrs);
    ORYON_CHECK_ARG(depth_a && depth_q && cam_a && cam_q);
    ORYON_CHECK_ARG(pcd_a && pcd_q && n_out);
    ORYON_CHECK_ARG(B >= 0 && n_cap > 0 && FH > 0 && FW > 0 && HA > 0 && WA > 0 && HQ > 0 && WQ > 0);
    ORYON_CHECK_ARG(depth_jump_mm >= 0.0f);              // a NaN fails too
    if (B == 0) return ORYON_OK;
    const float sya = (float)HA / (float)FH, sxa = (float)WA / (float)FW;
    const float syq = (float)HQ / (float)FH, sxq = (float)WQ / (float)FW;
    hipLaunchKernelGGL(lift_pairs_subpix_kernel, dim3(B), dim3(512), 0, as_stream(stream), corrs, offsets, n_corr, n_cap, sya, sxa, syq, sxq,
                       depth_a, HA, WA, depth_q, HQ, WQ, cam_a, cam_q, status, depth_jump_mm, pcd_a, pcd_q, n_out);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
