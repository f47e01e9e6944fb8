// What the ICP refiners (icp.hip: point-to-point, icp_plane.hip: point-to-plane on the depth map) share: the per-pair state, the fixed
// order of the row sums, the end of an update and the workspace.  A refiner is three kernels - init, rows -> one record per workgroup,
// records -> T_{k+1} - and the host enqueues init and then max_iter times the other two, reading nothing back.  The protocol:
//   state      IcpState, one per pair, in the workspace.  done is set by the init kernel (the pair does not start) or by lane 0 of an
//              update (too few rows, no solve, or converged) and never cleared.  Every kernel after init reads it ONCE, before any
//              barrier, and returns on it; nothing writes it during a row launch and only lane 0 of the pair's own update workgroup,
//              after that workgroup's barrier, during an update launch: the test is uniform over a workgroup.
//   sums       a workgroup's rows: an xor butterfly inside each wave, lane 0 of each wave to LDS, the waves added in ascending order
//              (icp_block_record); a pair's records: ascending block order (icp_sum_records).  No atomics.  The order is not part of
//              either refiner's definition but it is FIXED: every output is bit-stable across runs, streams and batch position.
//   ordering   no workgroup waits on another inside a launch: launch boundaries are the only cross-workgroup ordering.
// Include this FIRST: kabsch.h (rotation_from_covariance, wave_sum) is compiled under the compiler's default contraction - post.hip,
// pdsc_solver.hip and ransac.hip compile it so - and everything from here on without.  A contract(off) in front of kabsch.h would
// change the last bits of icp.hip's rotations.
#pragma once
#include "common.h"
#include "kabsch.h"

#pragma clang fp contract(off)

namespace oryon {

constexpr int ICP_THREADS = 256;             // source rows of a workgroup, one per lane: 64 pairs x 2048 rows = 512 workgroups on 256 CUs
constexpr int ICP_WAVES = ICP_THREADS / 64;
constexpr int ICP_MAX_ROWS = ORYON_ICP_MAX_ROWS;     // the derived error bar of the row sums assumes it
constexpr int ICP_MAX_ITER = ORYON_ICP_MAX_ITER;     // two launches each

struct IcpState {
    double T[12];                            // rows of [R | t] of T_k
    double prev;
    double origin[3];                        // a point near the cloud, computed once by the init kernel: the sums are formed about it
    int32_t done, pad;
};
static_assert(sizeof(IcpState) == ORYON_ICP_STATE_BYTES, "include/oryon_hip.h states the workspace formula");

__device__ __forceinline__ int icp_count(const int32_t *__restrict__ n, int b, int cap) { return max(0, min(n[b], cap)); }

// one coordinate of a moved point; row: four entries of [R | t]
__device__ __forceinline__ double icp_move(const double *row, double x, double y, double z)
{
    return ((row[0] * x + row[1] * y) + row[2] * z) + row[3];
}

// The pixel a moved point s (s[2] > 0) projects to, as g3's step 2 states it: u = (fx s.x) / s.z + cx, v alike, fpx = floor(u + 0.5),
// fpy = floor(v + 0.5) - still float64.  The caller tests them against its window BEFORE converting (a NaN or an infinity fails such a
// test), so no read leaves the map.  One text for icp_plane.hip and pose_verify.hip.
__device__ __forceinline__ void icp_project(const double (&s)[3], double fx, double cx, double fy, double cy, double &fpx, double &fpy)
{
    const double u = (fx * s[0]) / s[2] + cx, w = (fy * s[1]) / s[2] + cy;
    fpx = floor(u + 0.5);
    fpy = floor(w + 0.5);
}

// The end of an init kernel (one wave per pair): idx = -1, T_0 widened into the state and written out (so a pair that never iterates
// returns it), the done flag of a pair that does not start, the counters zeroed.  T_init NULL: the identity.  T64, n_kept, idx and
// status_out may be NULL.
__device__ __forceinline__ void icp_init_tail(int b, int lane, int cap_src, bool done, int st, const double (&o)[3],
                                              const float *__restrict__ T_init, IcpState *__restrict__ state, float *__restrict__ T,
                                              double *__restrict__ T64, int32_t *__restrict__ iters, double *__restrict__ mean_err,
                                              int32_t *__restrict__ n_kept, int32_t *__restrict__ idx, int32_t *__restrict__ status_out)
{
    if (idx)
        for (int i = lane; i < cap_src; i += 64) idx[(size_t)b * cap_src + i] = -1;
    if (lane < 16) {
        const float v = T_init ? T_init[(size_t)b * 16 + lane] : ((lane & 3) == (lane >> 2) ? 1.0f : 0.0f);
        T[(size_t)b * 16 + lane] = v;                        // the last row stays T_init's
        if (lane < 12) {
            state[b].T[lane] = (double)v;
            if (T64) T64[(size_t)b * 12 + lane] = (double)v;
        }
    }
    if (lane == 0) {
        IcpState &S = state[b];
        S.prev = 0.0;
        S.origin[0] = o[0]; S.origin[1] = o[1]; S.origin[2] = o[2];
        S.done = done ? 1 : 0;
        S.pad = 0;
        iters[b] = 0;
        mean_err[b] = 0.0;
        if (n_kept) n_kept[b] = 0;
        if (status_out) status_out[b] = st;
    }
}

// The rows of a workgroup of ICP_THREADS lanes (v: a lane's REC terms) reduced to the record of block blockIdx.x of pair b, partials
// [B, gridDim.x, REC].  lds: ICP_WAVES * REC doubles that no wave still reads.  Every thread of the workgroup must call this.
template <int REC>
__device__ __forceinline__ void icp_block_record(double (&v)[REC], double *lds, double *__restrict__ partials, int b)
{
#pragma unroll
    for (int q = 0; q < REC; ++q) v[q] = wave_sum(v[q]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < REC; ++q) lds[wave * REC + q] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < REC) {
        double a = lds[threadIdx.x];
#pragma unroll
        for (int w = 1; w < ICP_WAVES; ++w) a += lds[w * REC + threadIdx.x];
        partials[((size_t)b * gridDim.x + blockIdx.x) * REC + threadIdx.x] = a;
    }
}

// The records of pair b summed into acc [REC] (LDS) by one wave: the blocks that hold rows, in ascending order, lane q sums entry q.
// A block past the pair's rows wrote no record and is not read.  Ends in the barrier.
template <int REC>
__device__ __forceinline__ void icp_sum_records(const double *__restrict__ partials, int b, int n_blocks, const int32_t *__restrict__ n_src,
                                                int cap_src, double *acc)
{
    const int used = (icp_count(n_src, b, cap_src) + ICP_THREADS - 1) / ICP_THREADS;
    if (threadIdx.x < REC) {
        double a = 0.0;
        for (int blk = 0; blk < used; ++blk) a += partials[((size_t)b * n_blocks + blk) * REC + threadIdx.x];
        acc[threadIdx.x] = a;
    }
    __syncthreads();
}

// Tn = [R | t] T_k, rows of 3 x 4
__device__ __forceinline__ void icp_compose(const double (&R)[9], const double (&t)[3], const double *Tk, double (&Tn)[12])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) Tn[c * 4 + e] = (R[c * 3] * Tk[e] + R[c * 3 + 1] * Tk[4 + e]) + R[c * 3 + 2] * Tk[8 + e];
        Tn[c * 4 + 3] += t[c];
    }
}

// The end of update k that moved the pair (lane 0): T_{k+1} stored and written out, T = float32(T64), and the convergence rule - done
// when |prev - mean| < tolerance, this update applied; else prev = mean.
__device__ __forceinline__ void icp_commit(IcpState &S, int b, int k, const double (&Tn)[12], double mean, double tolerance,
                                           float *__restrict__ T_out, double *__restrict__ T64, int32_t *__restrict__ iters,
                                           double *__restrict__ mean_err)
{
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        S.T[q] = Tn[q];
        if (T64) T64[(size_t)b * 12 + q] = Tn[q];
        T_out[(size_t)b * 16 + q] = (float)Tn[q];
    }
    iters[b] = k + 1;
    mean_err[b] = mean;
    if (fabs(S.prev - mean) < tolerance) S.done = 1;
    else S.prev = mean;
}

struct IcpWorkspace {
    IcpState *state;
    double *partials;                        // [B, ceil(cap_src / ICP_THREADS), rec]
    size_t bytes;
};

// workspace NULL: the size only
static IcpWorkspace icp_carve(void *workspace, int B, int cap_src, int rec)
{
    IcpWorkspace w;
    Carver carve(workspace);
    carve(w.state, B);
    carve(w.partials, (size_t)B * ceil_div(cap_src, ICP_THREADS) * rec);
    w.bytes = carve.off;
    return w;
}

}  // namespace oryon
