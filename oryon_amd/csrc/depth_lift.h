// The float64 lift of a depth pixel, as g1 defines it (include/oryon_hip.h, oryon_gt_corrs): shared by gt_corrs.hip (gtc_lift_kernel)
// and icp_plane.hip (the vertices under a normal), which g3's definition holds to the same arithmetic.
//   X = (double(fp32(x) - fp32(cx)) * z) / fx / 1000, Y alike with (y, cy, fy), Z = z / 1000;  z in millimetres, the result in metres.
// The pixel-minus-centre difference is taken in fp32: the reference's xmap / ymap are float32 tensors and cx a 0-dim float64 one, which
// torch's promotion rules leave in float32.  No contraction.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace oryon {

__device__ __forceinline__ void depth_lift_f64(int x, int y, double z, double fx, float cxf, double fy, float cyf, double v[3])
{
    const float dxf = (float)x - cxf, dyf = (float)y - cyf;
    v[0] = (((double)dxf * z) / fx) / 1000.0;
    v[1] = (((double)dyf * z) / fy) / 1000.0;
    v[2] = z / 1000.0;
}

}  // namespace oryon
