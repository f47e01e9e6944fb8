// K-1a: the training augmentations of the reference (datasets.py:98-114 build_augs, utils/augmentations.py:17-127: ColorJitter x2, hflip,
// vflip - per sample, on dataloader workers, on a float64 [3,480,640] tensor) fused into the K-1 resizes of preproc.hip for a whole batch.
//
//   rgb    uint8 [n,HI,WI,3] + per-image table -> fp32 [n,3,HO,WO]: two launches.
//            pass 1  rgb_gray_mean_kernel      the contrast op blends with the mean of gray(image as it is when the op runs).  The ops
//                                              ahead of it are pointwise, so that mean is ONE reduction over the source pixels pushed
//                                              through that prefix: per thread a strided fp64 sum, per block a fixed LDS tree, one fp64
//                                              partial per block (MEAN_BLOCKS per image, written by every block of an image that has a
//                                              contrast op; the other images' blocks leave at once).  No float atomics: bit-stable.
//            pass 2  rgb_augment_resize_kernel rgb_resize_bilinear_kernel's resampling (same make_tap<double>, same evaluation order, one
//                                              rounding), each of the four taps read through the mirrored index and pushed through the
//                                              whole colour chain first; adds the image's partials in index order for the mean.
//                                              Only touched texels are processed, no sensor-resolution float image exists.
//   depth / mask: resize_bilinear_f32_kernel / mask_resize_nearest_kernel (preproc.hip, roi.hip) reading through the mirrored index.
//
// The colour arithmetic is DEFINED (DESIGN.md "7b"), transcribed from torchvision's tensor path: fp64 blends, the hue stage in fp32,
// every operation correctly rounded and uncontracted (the pragma inside each colour function; the library builds with correctly rounded
// fp32 divide), so the op sequence is the one of the numpy statement tests/augment_restatement.py.  The resampling itself is compiled
// like preproc.hip's (default contraction): an all-off table gives oryon_rgb_resize_bilinear's bytes.
//
// Table (include/oryon_hip.h): ORYON_AUG_STRIDE doubles per image - [0] flip bits, [1] reserved, then ORYON_AUG_SLOTS (op id, factor)
// pairs in execution order; an id outside 0..3 is an empty slot.
#include "common.h"
#include "resample.h"

namespace oryon {
namespace {

constexpr int AUG_SLOTS = ORYON_AUG_SLOTS, AUG_STRIDE = ORYON_AUG_STRIDE;
constexpr int MEAN_BLOCKS = 64, MEAN_THREADS = 256;
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };

__device__ __forceinline__ int slot_op(const double *__restrict__ T, int k)
{
    const double id = T[2 + 2 * k];
    return id == 0.0 ? 0 : id == 1.0 ? 1 : id == 2.0 ? 2 : id == 3.0 ? 3 : -1;
}

// index of the contrast slot, AUG_SLOTS when the image has none (at most one per image, by the table's contract)
__device__ __forceinline__ int contrast_slot(const double *__restrict__ T)
{
    int at = AUG_SLOTS;
    for (int k = AUG_SLOTS - 1; k >= 0; --k)
        if (slot_op(T, k) == OP_CONTRAST) at = k;
    return at;
}

__device__ __forceinline__ double gray_of(double r, double g, double b)
{
#pragma clang fp contract(off)
    return (0.2989 * r + 0.587 * g) + 0.114 * b;
}

__device__ __forceinline__ double blend(double a, double b, double f)
{
#pragma clang fp contract(off)
    const double v = f * a + (1.0 - f) * b;
    return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

__device__ __forceinline__ float clamp01f(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// torchvision's adjust_hue on one pixel: fp32 rgb -> hsv, h <- (h + f) mod 1, hsv -> rgb, back to fp64.
__device__ __forceinline__ void hue_shift(double (&px)[3], float f)
{
#pragma clang fp contract(off)
    const float r = (float)px[0], g = (float)px[1], b = (float)px[2];
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.0f : maxc);
    const float d = eqc ? 1.0f : cr;
    const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
    // exactly one of the three masks holds; the masked-out terms are zeros, so the sum is the live term
    float hs;
    if (maxc == r) hs = bc - gc;
    else if (maxc == g) hs = (2.0f + rc) - bc;
    else hs = (4.0f + gc) - rc;
    float h = hs / 6.0f + 1.0f;
    h = h - truncf(h);                                  // fmod(h, 1) for h > 0: exact
    float t = h + f;
    t = t - truncf(t);                                  // fmod(t, 1): exact; torch's remainder adds the divisor to a negative result
    if (t < 0.0f) t = t + 1.0f;
    const float h6 = t * 6.0f;
    const float fl = floorf(h6);
    const float fr = h6 - fl;
    const int i = (int)fl % 6;
    const float v = maxc;
    const float p = clamp01f(v * (1.0f - s));
    const float q = clamp01f(v * (1.0f - s * fr));
    const float u = clamp01f(v * (1.0f - s * (1.0f - fr)));
    const float ro = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? u : v;
    const float go = i == 0 ? u : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
    const float bo = i == 0 ? p : i == 1 ? p : i == 2 ? u : i == 3 ? v : i == 4 ? v : q;
    px[0] = (double)ro, px[1] = (double)go, px[2] = (double)bo;
}

// Slots [0, end) of one image's chain on NT pixels.  The slot loop is not unrolled and branches wave-uniformly (the table row is the
// block's); the pixels stay in registers (static indices only).
template <int NT>
__device__ __forceinline__ void colour_chain(double (&px)[NT][3], const double *__restrict__ T, int end, double mean)
{
#pragma unroll 1
    for (int k = 0; k < end; ++k) {
        const int op = slot_op(T, k);
        if (op < 0) continue;
        const double f = T[3 + 2 * k];
        if (op == OP_BRIGHTNESS) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int c = 0; c < 3; ++c) px[t][c] = blend(px[t][c], 0.0, f);
        } else if (op == OP_CONTRAST) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int c = 0; c < 3; ++c) px[t][c] = blend(px[t][c], mean, f);
        } else if (op == OP_SATURATION) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double gr = gray_of(px[t][0], px[t][1], px[t][2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) px[t][c] = blend(px[t][c], gr, f);
            }
        } else {
#pragma unroll
            for (int t = 0; t < NT; ++t) hue_shift(px[t], (float)f);
        }
    }
}

__global__ __launch_bounds__(MEAN_THREADS) void rgb_gray_mean_kernel(const uint8_t *__restrict__ in, const double *__restrict__ table,
                                                                      int HI, int WI, double *__restrict__ partial)
{
    __shared__ double s_sum[MEAN_THREADS];
    const int m = blockIdx.y;
    const double *T = table + (size_t)m * AUG_STRIDE;
    const int end = contrast_slot(T);
    if (end == AUG_SLOTS) return;                        // the whole block: T is the block's
    const uint8_t *img = in + (size_t)m * HI * WI * 3;
    double acc = 0.0;
    for (int p = blockIdx.x * MEAN_THREADS + threadIdx.x; p < HI * WI; p += MEAN_BLOCKS * MEAN_THREADS) {
        double px[1][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) px[0][c] = img[(size_t)p * 3 + c] / 255.0;
        colour_chain<1>(px, T, end, 0.0);
        acc += gray_of(px[0][0], px[0][1], px[0][2]);
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int w = MEAN_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)m * MEAN_BLOCKS + blockIdx.x] = s_sum[0];
}

__global__ __launch_bounds__(256) void rgb_augment_resize_kernel(const uint8_t *__restrict__ in, const double *__restrict__ table,
                                                                  const double *__restrict__ partial, int HI, int WI, int HO, int WO,
                                                                  float *__restrict__ out)
{
    const int m = blockIdx.y;
    const double *T = table + (size_t)m * AUG_STRIDE;
    const int flip = (int)T[0];
    const bool hflip = flip & ORYON_AUG_HFLIP, vflip = flip & ORYON_AUG_VFLIP;
    double mean = 0.0;
    if (contrast_slot(T) < AUG_SLOTS) {
        for (int i = 0; i < MEAN_BLOCKS; ++i) mean += partial[(size_t)m * MEAN_BLOCKS + i];
        mean = mean / (double)(HI * WI);
    }
    const double sy = (double)HI / (double)HO, sx = (double)WI / (double)WO;
    const uint8_t *img = in + (size_t)m * HI * WI * 3;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HO * WO; p += gridDim.x * blockDim.x) {
        const int y = p / WO, x = p % WO;
        const Tap<double> ty = make_tap<double>(y, sy, HI), tx = make_tap<double>(x, sx, WI);
        const int y0 = vflip ? HI - 1 - ty.i0 : ty.i0, y1 = vflip ? HI - 1 - ty.i1 : ty.i1;
        const int x0 = hflip ? WI - 1 - tx.i0 : tx.i0, x1 = hflip ? WI - 1 - tx.i1 : tx.i1;
        const uint8_t *r0 = img + ((size_t)y0 * WI) * 3, *r1 = img + ((size_t)y1 * WI) * 3;
        double px[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            px[0][c] = r0[x0 * 3 + c] / 255.0, px[1][c] = r0[x1 * 3 + c] / 255.0;
            px[2][c] = r1[x0 * 3 + c] / 255.0, px[3][c] = r1[x1 * 3 + c] / 255.0;
        }
        colour_chain<4>(px, T, AUG_SLOTS, mean);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double a = px[0][c], b = px[1][c], cc = px[2][c], d = px[3][c];
            const double v = ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * cc + tx.l1 * d);
            out[((size_t)m * 3 + c) * HO * WO + p] = (float)v;
        }
    }
}

// resize_bilinear_f32_kernel (preproc.hip) on the flipped image
__global__ __launch_bounds__(256) void resize_bilinear_f32_flip_kernel(const float *__restrict__ in, const double *__restrict__ table,
                                                                        int HI, int WI, int HO, int WO, int round_output,
                                                                        float *__restrict__ out)
{
    const int m = blockIdx.y;
    const int flip = (int)table[(size_t)m * AUG_STRIDE];
    const bool hflip = flip & ORYON_AUG_HFLIP, vflip = flip & ORYON_AUG_VFLIP;
    const float sy = (float)HI / (float)HO, sx = (float)WI / (float)WO;
    const float *img = in + (size_t)m * HI * WI;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HO * WO; p += gridDim.x * blockDim.x) {
        const int y = p / WO, x = p % WO;
        const Tap<float> ty = make_tap<float>(y, sy, HI), tx = make_tap<float>(x, sx, WI);
        const int y0 = vflip ? HI - 1 - ty.i0 : ty.i0, y1 = vflip ? HI - 1 - ty.i1 : ty.i1;
        const int x0 = hflip ? WI - 1 - tx.i0 : tx.i0, x1 = hflip ? WI - 1 - tx.i1 : tx.i1;
        const float a = img[(size_t)y0 * WI + x0], b = img[(size_t)y0 * WI + x1];
        const float c = img[(size_t)y1 * WI + x0], d = img[(size_t)y1 * WI + x1];
        const float top = __fmaf_rn(b, tx.l1, __fmul_rn(a, tx.l0));
        const float bot = __fmaf_rn(d, tx.l1, __fmul_rn(c, tx.l0));
        float v = __fmaf_rn(bot, ty.l1, __fmul_rn(top, ty.l0));
        if (round_output) v = rintf(v);
        out[(size_t)m * HO * WO + p] = v;
    }
}

// mask_resize_nearest_kernel (roi.hip) on the flipped mask
__global__ __launch_bounds__(256) void mask_resize_nearest_flip_kernel(const uint8_t *__restrict__ in, const double *__restrict__ table,
                                                                        int HI, int WI, int HO, int WO, int32_t *__restrict__ out)
{
    const int m = blockIdx.y;
    const int flip = (int)table[(size_t)m * AUG_STRIDE];
    const bool hflip = flip & ORYON_AUG_HFLIP, vflip = flip & ORYON_AUG_VFLIP;
    const float sy = (float)HI / (float)HO, sx = (float)WI / (float)WO;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HO * WO; p += gridDim.x * blockDim.x) {
        const int y = p / WO, x = p % WO;
        int ys = (int)floorf((float)y * sy), xs = (int)floorf((float)x * sx);
        ys = ys < HI - 1 ? ys : HI - 1;
        xs = xs < WI - 1 ? xs : WI - 1;
        if (vflip) ys = HI - 1 - ys;
        if (hflip) xs = WI - 1 - xs;
        out[(size_t)m * HO * WO + p] = (int32_t)in[((size_t)m * HI + ys) * WI + xs];
    }
}

bool sizes_ok(int HI, int WI, int HO, int WO)
{
    return HI > 0 && WI > 0 && HO > 0 && WO > 0 && (int64_t)HI * WI <= INT32_MAX / 4 && (int64_t)HO * WO <= INT32_MAX / 4;
}

}  // namespace
}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_rgb_augment_workspace_bytes(int n)
{
    return n > 0 ? (size_t)n * MEAN_BLOCKS * sizeof(double) : 0;
}

extern "C" int oryon_rgb_augment_resize(const uint8_t *rgb_hwc, const double *table, int n, int HI, int WI, int HO, int WO,
                                        void *workspace, size_t workspace_bytes, float *out, void *stream)
{
    ORYON_CHECK_ARG(n >= 0);
    if (n == 0) return ORYON_OK;
    ORYON_CHECK_ARG(rgb_hwc && table && workspace && out && sizes_ok(HI, WI, HO, WO));
    ORYON_CHECK_ARG(((uintptr_t)table & 7) == 0 && ((uintptr_t)workspace & 7) == 0);
    if (workspace_bytes < oryon_rgb_augment_workspace_bytes(n)) {
        set_error("%s: workspace of %zu bytes, %zu needed", __func__, workspace_bytes, oryon_rgb_augment_workspace_bytes(n));
        return ORYON_ERR_WORKSPACE;
    }
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(rgb_gray_mean_kernel, dim3(MEAN_BLOCKS, n), dim3(MEAN_THREADS), 0, as_stream(stream), rgb_hwc, table, HI, WI, partial);
    ORYON_CHECK_LAUNCH();
    const int bx = ceil_div(HO * WO, 256) < 256 ? ceil_div(HO * WO, 256) : 256;
    hipLaunchKernelGGL(rgb_augment_resize_kernel, dim3(bx, n), dim3(256), 0, as_stream(stream), rgb_hwc, table, partial, HI, WI, HO, WO, out);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_resize_bilinear_f32_flip(const float *in, const double *table, int n, int HI, int WI, int HO, int WO, int round_output,
                                              float *out, void *stream)
{
    ORYON_CHECK_ARG(n >= 0);
    if (n == 0) return ORYON_OK;
    ORYON_CHECK_ARG(in && table && out && sizes_ok(HI, WI, HO, WO) && ((uintptr_t)table & 7) == 0);
    const int bx = ceil_div(HO * WO, 256) < 256 ? ceil_div(HO * WO, 256) : 256;
    hipLaunchKernelGGL(resize_bilinear_f32_flip_kernel, dim3(bx, n), dim3(256), 0, as_stream(stream), in, table, HI, WI, HO, WO, round_output,
                       out);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_mask_resize_nearest_flip(const uint8_t *mask_in, const double *table, int n_maps, int HI, int WI, int HO, int WO,
                                              int32_t *mask_out, void *stream)
{
    ORYON_CHECK_ARG(n_maps >= 0);
    if (n_maps == 0) return ORYON_OK;
    ORYON_CHECK_ARG(mask_in && table && mask_out && sizes_ok(HI, WI, HO, WO) && ((uintptr_t)table & 7) == 0);
    const int bx = ceil_div(HO * WO, 256) < 64 ? ceil_div(HO * WO, 256) : 64;
    hipLaunchKernelGGL(mask_resize_nearest_flip_kernel, dim3(bx, n_maps), dim3(256), 0, as_stream(stream), mask_in, table, HI, WI, HO, WO,
                       mask_out);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
