// The all-pairs float64 nearest-neighbour tile walk, shared by gt_corrs.hip (pcd_nearest_f64_kernel) and icp.hip (icp_nearest_kernel).
// A workgroup of THREADS lanes holds PPL points per lane in registers and walks one cloud in ascending order through LDS tiles of
// NN_TILE points, float64 structure-of-arrays: in the inner loop every lane of a wave reads the SAME address, which the LDS serves as a
// broadcast (no bank conflicts).  d2_j = ((dx dx + dy dy) + dz dz) without contraction, strict <: the first minimiser wins, a NaN never
// does; bi = -1 and best = +inf when no point compares below +inf.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace oryon {

constexpr int NN_TILE = 1024;                // points per LDS tile: 3 x 1024 float64 = 24 KB
constexpr size_t NN_TILE_BYTES = 3 * (size_t)NN_TILE * sizeof(double);

// Q: the [nq,3] rows of the walked cloud.  tile: [3][NN_TILE] doubles of LDS (x | y | z).  Every thread of the workgroup must call this
// (it holds barriers); the tile may be reused after a __syncthreads().
template <int PPL, int THREADS>
__device__ __forceinline__ void nearest_walk_f64(const double *__restrict__ Q, int nq, double *tile, const double (&ax)[PPL],
                                                 const double (&ay)[PPL], const double (&az)[PPL], double (&best)[PPL], int (&bi)[PPL])
{
    const double *sx = tile, *sy = tile + NN_TILE, *sz = tile + 2 * NN_TILE;
#pragma unroll
    for (int u = 0; u < PPL; ++u) {
        best[u] = __longlong_as_double(0x7ff0000000000000ll);
        bi[u] = -1;
    }
    for (int t0 = 0; t0 < nq; t0 += NN_TILE) {
        const int m = min(NN_TILE, nq - t0);
        __syncthreads();                                     // the previous tile has been consumed
        for (int e = threadIdx.x; e < 3 * m; e += THREADS) {
            const int pnt = e / 3, c = e - pnt * 3;          // coalesced read of the [m,3] rows, transposed into the three planes
            tile[c * NN_TILE + pnt] = Q[(size_t)t0 * 3 + e];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const double qx = sx[j], qy = sy[j], qz = sz[j];
#pragma unroll
            for (int u = 0; u < PPL; ++u) {
                const double dx = ax[u] - qx, dy = ay[u] - qy, dz = az[u] - qz;
                const double d = ((dx * dx + dy * dy) + dz * dz);
                const bool lt = d < best[u];
                best[u] = lt ? d : best[u];
                bi[u] = lt ? t0 + j : bi[u];
            }
        }
    }
}

}  // namespace oryon
