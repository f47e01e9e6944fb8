// The evaluator's float16 pose rounding (utils/evaluator.py:258-266), shared by the MSSD / MSPD kernels (evaluate.hip) and VSD (vsd.hip).
#pragma once
#include <hip/hip_fp16.h>
#include "common.h"

namespace oryon {

__device__ __forceinline__ double round_to_half(double d)
{
    // numpy's float64 -> float16 cast rounds once (to nearest even).  Going through float would round twice, so the intermediate
    // float is made by ROUND-TO-ODD (truncate, set the last bit if inexact): a following round-to-nearest to 11 bits is then exact.
    float f = (float)d;
    const double back = (double)f;
    if (back != d) {
        unsigned u = __float_as_uint(f);
        if (fabs(back) > fabs(d)) u -= 1u;              // undo a rounding away from zero (sign-magnitude: one step towards zero)
        u |= 1u;
        f = __uint_as_float(u);
    }
    return (double)__half2float(__float2half_rn(f));
}

struct Pose34 { double m[12]; };

__device__ __forceinline__ Pose34 pose_f16_mm(const double *P)          // [4,4] row-major, metres -> R16 | half(t16 * 1000)
{
    Pose34 o;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o.m[4 * r + c] = round_to_half(P[4 * r + c]);
        const float t16 = (float)round_to_half(P[4 * r + 3]);
        o.m[4 * r + 3] = (double)__half2float(__float2half_rn(__fmul_rn(t16, 1000.0f)));
    }
    return o;
}

}  // namespace oryon
