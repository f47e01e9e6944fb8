// K1m: mutual nearest neighbours in ONE all-pairs scan on the fp32 matrix cores of gfx950.
//
// For every anchor row i the nearest query row (exactly K1, csrc/match.hip), for every query row j the nearest ANCHOR row (exactly K1
// with the roles swapped), and mutual[i] = valid[i] && rev_argmin[argmin[i]] == i.  The product tile S = Q^ A^T is the same in both
// directions and the f32-input MFMA is an exact k-ordered fmaf chain that does not care which operand is called "anchor", so every
// distance the swapped call would compute already sits in this scan's accumulators with the same bits: the scan reduces each tile
// along BOTH axes.
//
//   * anchor direction (lane-local): in the 32x32x2 MFMA's C/D layout a lane owns one anchor column and 16 query rows; the running
//     (min, argmin) over queries stays in the lane, as in K1.
//   * query direction (cross-lane): the minimum of an accumulator register over the 32 lanes of a half-wave is the minimum over 32
//     anchors of one query row, taken on the distance's order-preserving integer image.  Four DPP steps reduce inside a 16-lane row, one v_permlane16_swap joins the two rows of the half;
//     the index is the lowest lane of a ballot of d == row_min (lowest lane = lowest anchor index = the first-index tie rule).
//     Anchor columns >= n_a and query rows >= n_q are masked by INDEX before either reduction: K0 zero-fills rows only up to the
//     next multiple of 256, the rest of a torch.empty buffer is garbage.
//   * across waves of a workgroup: 64-bit ds_min on an order-preserving (distance, index) key per query row of the tile (LDS, double
//     buffered over the barriers the tile loop already has);
//   * across the T = cap_a / 128 anchor panels: one 64-bit global atomicMin (agent scope) per (query row, panel) on keys[B, cap_q].
//     An integer minimum does not depend on the order of arrival: the result is bit-stable.  One atomic per (query row, panel) is
//     B n_q T 8 B - 1 GB at B = 64, n_q = 50176, T = 40 against 8 TFLOP of matrix work.
//   * a join pass unpacks the keys into rev_min_dist / rev_argmin, merges K1's query splits and writes mutual.
//
// The key: distances can be a few ulps below zero, -0.0 cannot occur (fma(-0.5, 1, 0.5) is +0).  u = bits ^ (sign ? ~0 : 0x80000000) is
// monotone in `<` on all non-NaN floats; key = u << 32 | index orders lexicographically by (distance, index), which is what K1's
// strict `<` in ascending index order computes.
//
// The tile loops, the LDS image and the LDS-DMA of the two kernels below are the two walks of match_tile.h (where they are explained),
// kept here as this file's own text: instantiated from the header the C_pad 32 kernel was slower.  What differs from K1
// is the fold of a finished tile and the hand-over at the end.
#include "common.h"
#include "match_common.h"
#include "match_tile.h"

namespace oryon {

constexpr unsigned long long KEY_NONE = ~0ull;       // above every key of a finite or infinite distance

// the order-preserving image of a distance: u(x) < u(y) as unsigned <=> x < y as floats (no NaN, no -0.0)
__device__ __forceinline__ unsigned dist_key(float d)
{
    const int b = __float_as_int(d);
    return (unsigned)b ^ ((unsigned)(b >> 31) | 0x80000000u);
}
__device__ __forceinline__ unsigned long long rev_key(unsigned dkey, int idx) { return ((unsigned long long)dkey << 32) | (unsigned)idx; }
__device__ __forceinline__ void rev_unkey(unsigned long long key, float &d, int &idx)
{
    const unsigned u = (unsigned)(key >> 32);
    d = __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
    idx = (int)(unsigned)key;
    if (key == KEY_NONE || d == INFINITY) {          // no anchor row, or none with a finite distance: what K1's strict `<` leaves
        d = INFINITY;
        idx = 0;
    }
}

template <int CTRL> __device__ __forceinline__ unsigned dpp_mov(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
// minimum of v over the 32 lanes of this lane's half-wave, in every lane of the half.  On distance keys, not floats: an integer
// minimum needs no NaN quieting in front of it and folds its DPP operand into the instruction.
__device__ __forceinline__ unsigned half_min(unsigned v)
{
    v = min(v, dpp_mov<0xB1>(v));          // quad_perm [1,0,3,2]
    v = min(v, dpp_mov<0x4E>(v));          // quad_perm [2,3,0,1]
    v = min(v, dpp_mov<0x141>(v));         // row_half_mirror
    v = min(v, dpp_mov<0x140>(v));         // row_mirror
    // rows (0,1) and (2,3): v_permlane16_swap exchanges the odd rows of its first operand with the even rows of its second
    const auto sw = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return min(sw[0], sw[1]);
}
// lowest set lane of this lane's half of a ballot (-1: none)
__device__ __forceinline__ int half_first(unsigned long long ballot, int hi)
{
    const unsigned b = hi ? (unsigned)(ballot >> 32) : (unsigned)ballot;
    return __ffs(b) - 1;
}
// query row (inside its 32-row block) that accumulator register r holds in half-wave hi
__device__ __forceinline__ int acc_row(int r, int hi) { return 4 * hi + (r & 3) + 8 * (r >> 2); }

// a finished tile's per-query keys leave the workgroup: called by all threads behind the barrier that closes the LDS minima
__device__ __forceinline__ void rev_flush(unsigned long long *red, int rows, int q0, int nq, unsigned long long *keys_p)
{
    const int t = threadIdx.x;
    if (t < rows) {
        const unsigned long long k = red[t];
        red[t] = KEY_NONE;
        if (q0 + t < nq) atomicMin(keys_p + q0 + t, k);
    }
}

// ------------------------------------------------------------------------------------------------ C_pad 32 / 64 / 128 / 256
template <int CP>
__global__ __launch_bounds__(MATCH_THREADS, 2) void match_mutual_regb_kernel(
    const float *__restrict__ a_hat, const float *__restrict__ q_hat, int B, int cap_a, int cap_q,
    const int32_t *__restrict__ n_a, const int32_t *__restrict__ n_q, float thr, int T, int S,
    float *__restrict__ min_dist, int32_t *__restrict__ argmin, uint8_t *__restrict__ valid,
    float *__restrict__ ws_dist, int32_t *__restrict__ ws_idx, unsigned long long *__restrict__ keys)
{
    constexpr int RB = CP * 4;
    constexpr int ROWS = CP >= 128 ? 64 : 8192 / CP;
    constexpr int KH = 8192 / ROWS;
    constexpr int KP = CP / KH;
    constexpr int NACC = ROWS / 32;
    constexpr int NGT = KH / 8;
    constexpr int TILE_BYTES = 32768;
    constexpr int NI = 8;
    constexpr int RG = NACC >= 4 ? 2 : 3;
    constexpr bool NARROW = KH < 64;
    constexpr int LPR = NARROW ? 1 : KH * 4 / 256;
    static_assert(NACC * NGT == 32 && KP * NGT * 8 == CP && ROWS <= MATCH_THREADS, "tile geometry");
    __shared__ __attribute__((aligned(256))) char smem[2 * TILE_BYTES];
    __shared__ unsigned long long red[2][ROWS];         // per-query minima of a tile over the workgroup's 128 anchors

    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int unit = (slot / T) * 8 + xcd;
    if (unit >= B * S) return;
    const int panel = slot % T;
    const int p = unit / S, split = unit % S;
    const int na = n_a[p], nq = n_q[p];
    const int a0 = panel * MT;
    if (a0 >= na) return;
    const int nqt = (nq + ROWS - 1) / ROWS;
    const int qt_per = (nqt + S - 1) / S;
    const int qt_begin = split * qt_per;
    const int qt_end = (qt_begin + qt_per < nqt) ? qt_begin + qt_per : nqt;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, hi = lane >> 5;
    const char *qp = reinterpret_cast<const char *>(q_hat + (size_t)p * cap_q * CP);
    unsigned long long *keys_p = keys + (size_t)p * cap_q;
    const int a = a0 + wave * 32 + l31;                 // this lane's anchor row
    const bool a_ok = a < na;
    const bool full_a = a0 + MT <= na;

    if (t < ROWS) red[0][t] = red[1][t] = KEY_NONE;

    float4 breg[CP / 8];
    {
        const float *arow = a_hat + ((size_t)p * cap_a + a) * CP + 4 * hi;
#pragma unroll
        for (int g = 0; g < CP / 8; ++g) breg[g] = *reinterpret_cast<const float4 *>(arow + 8 * g);
    }

    unsigned dma_off[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const int line = (wave * NI + j) * 4 + (lane >> 4), sl = lane & 15;
        if (NARROW) {
            const int cc = sl ^ (line & 15);
            dma_off[j] = (unsigned)((line * 2 + (cc >> 3)) * RB + (cc & 7) * 16);
        } else {
            const int row = line / LPR;
            const int cc = sl ^ (row & 15);
            dma_off[j] = (unsigned)(row * RB + ((line % LPR) * 16 + cc) * 16);
        }
    }
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    auto issue = [&](int qt, int kp, int buf) {
        const char *qb = qp + (size_t)qt * ROWS * RB + kp * KH * 4;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            char *dst = smem + buf * TILE_BYTES + (wave_u * NI + j) * 1024;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(qb + dma_off[j]),
                                             (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        }
    };

    const unsigned rd_base = NARROW ? (unsigned)((l31 >> 1) * 256) : (unsigned)(l31 * KH * 4);
    const unsigned rd_key = NARROW ? (unsigned)(((l31 & 1) * 8 + hi) ^ ((l31 >> 1) & 15)) : (unsigned)(hi ^ (l31 & 15));
    auto rd = [&](int g, int m, unsigned tile) -> float4 {
        unsigned key = rd_key;
        asm volatile("" : "+v"(key));
        const unsigned imm = NARROW ? (unsigned)(m * 4096) : (unsigned)(m * 32 * KH * 4 + (g >> 3) * 256);
        const unsigned off = rd_base + ((key ^ (2u * (g & 7))) << 4) + imm + tile;
        return *reinterpret_cast<const float4 *>(smem + off);
    };

    f32x16 acc[NACC];
#pragma unroll
    for (int m = 0; m < NACC; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;
    float best = INFINITY;
    int bidx = 0x7fffffff;

    if (qt_end > qt_begin) issue(qt_begin, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int buf = 0, fb = 0;
    for (int qt = qt_begin; qt < qt_end; ++qt) {
#pragma unroll
        for (int kp = 0; kp < KP; ++kp) {
            if (kp + 1 < KP) issue(qt, kp + 1, buf ^ 1);
            else if (qt + 1 < qt_end) issue(qt + 1, 0, buf ^ 1);
            const unsigned tile = buf * TILE_BYTES;
            float4 ring[RG][NACC];
#pragma unroll
            for (int g = 0; g < RG - 1; ++g)
#pragma unroll
                for (int m = 0; m < NACC; ++m) ring[g][m] = rd(g, m, tile);
#pragma unroll
            for (int g = 0; g < NGT; ++g) {
                if (g + RG - 1 < NGT) {
#pragma unroll
                    for (int m = 0; m < NACC; ++m) ring[(g + RG - 1) % RG][m] = rd(g + RG - 1, m, tile);
                }
                const float4 bv = breg[kp * NGT + g];
#pragma unroll
                for (int m = 0; m < NACC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[g % RG][m].x, bv.x, acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < NACC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[g % RG][m].y, bv.y, acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < NACC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[g % RG][m].z, bv.z, acc[m], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < NACC; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(ring[g % RG][m].w, bv.w, acc[m], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (kp == KP - 1) {
                const int q0 = qt * ROWS;
                const bool masked = !(full_a && q0 + ROWS <= nq);
                // one 32x32 block at a time: distances (rows and columns outside the pair masked by index), the anchor direction in
                // the lane, the query direction across the half-wave
#pragma unroll
                for (int m = 0; m < NACC; ++m) {
                    float d[16];
                    float mn = INFINITY;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        d[r] = __fmaf_rn(-0.5f, acc[m][r], 0.5f);
                        if (masked) d[r] = (a_ok && q0 + m * 32 + acc_row(r, hi) < nq) ? d[r] : INFINITY;
                        acc[m][r] = 0.0f;
                        mn = fminf(mn, d[r]);
                    }
                    // the exact first-index search only when some lane of the wave improves (ever rarer as the minimum settles)
                    if (__any(mn < best)) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const bool better = d[r] < best;     // strict: first (smallest) query index wins ties
                            best = better ? d[r] : best;
                            bidx = better ? q0 + m * 32 + acc_row(r, hi) : bidx;
                        }
                    }
                    // row minimum over this wave's 32 anchors; lane l31 == r of each half keeps row r's result
                    unsigned rk = 0u;
                    int ri = 0;
                    int lsel = l31;
                    asm volatile("" : "+v"(lsel));          // the sixteen lane == r masks are made here, not kept in scalar registers across the loop
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned u = dist_key(d[r]);
                        const unsigned rm = half_min(u);
                        const int first = half_first(__ballot(u == rm), hi);
                        rk = (lsel == r) ? rm : rk;
                        ri = (lsel == r) ? first : ri;
                    }
                    const int ql = m * 32 + acc_row(l31 & 15, hi);
                    if (l31 < 16 && q0 + ql < nq) atomicMin(&red[fb][ql], rev_key(rk, a0 + wave * 32 + ri));
                    __builtin_amdgcn_sched_barrier(0);      // one block's reduction at a time: its temporaries do not pile up
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kp == KP - 1) {
                rev_flush(red[fb], ROWS, qt * ROWS, nq, keys_p);
                fb ^= 1;
            }
            buf ^= 1;
        }
    }
    {
        const float od = __shfl_xor(best, 32);
        const int oi = __shfl_xor(bidx, 32);
        lex_min(best, bidx, od, oi);
    }
    if (hi == 0 && a_ok) {
        if (S == 1) {
            const size_t o = (size_t)p * cap_a + a;
            min_dist[o] = best;
            argmin[o] = (bidx == 0x7fffffff) ? 0 : bidx;
            valid[o] = (best < thr) ? 1 : 0;
        } else {
            const size_t o = ((size_t)p * S + split) * cap_a + a;
            ws_dist[o] = best;
            ws_idx[o] = bidx;
        }
    }
}

// ------------------------------------------------------------------------------------------------ wider descriptors (LDS-staged)
__global__ __launch_bounds__(MATCH_THREADS, 2) void match_mutual_staged_kernel(
    const float *__restrict__ a_hat, const float *__restrict__ q_hat, int B, int Cp, int cap_a, int cap_q,
    const int32_t *__restrict__ n_a, const int32_t *__restrict__ n_q, float thr, int T, int S,
    float *__restrict__ min_dist, int32_t *__restrict__ argmin, uint8_t *__restrict__ valid,
    float *__restrict__ ws_dist, int32_t *__restrict__ ws_idx, unsigned long long *__restrict__ keys)
{
    __shared__ float smem[4 * TILE_FLOATS];
    __shared__ unsigned long long red[2][MT];

    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int per_pair = T * S;
    const int p = (slot / per_pair) * 8 + xcd;
    if (p >= B) return;
    const int rem = slot % per_pair;
    const int panel = rem / S, split = rem % S;
    const int na = n_a[p], nq = n_q[p];
    const int a0 = panel * MT;
    if (a0 >= na) return;

    const int nqt = (nq + MT - 1) / MT;
    const int qt_per = (nqt + S - 1) / S;
    const int qt_begin = split * qt_per;
    const int qt_end = (qt_begin + qt_per < nqt) ? qt_begin + qt_per : nqt;
    const int KT = Cp / BK;
    const int nit = (qt_end > qt_begin) ? (qt_end - qt_begin) * KT : 0;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, hi = lane >> 5;

    const float *ap = a_hat + ((size_t)p * cap_a + a0) * Cp;
    const float *qp = q_hat + (size_t)p * cap_q * Cp;
    unsigned long long *keys_p = keys + (size_t)p * cap_q;
    const bool a_ok[2] = {a0 + wn * 64 + l31 < na, a0 + wn * 64 + 32 + l31 < na};
    const bool full_a = a0 + MT <= na;

    if (t < MT) red[0][t] = red[1][t] = KEY_NONE;

    float4 rq[4], ra[4];
    auto gload = [&](int it) {
        const int qt = qt_begin + it / KT, kt = it % KT;
        const float *qb = qp + (size_t)qt * MT * Cp + kt * BK;
        const float *ab = ap + kt * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = t + MATCH_THREADS * i, row = f >> 3, c4 = f & 7;
            rq[i] = *reinterpret_cast<const float4 *>(qb + (size_t)row * Cp + c4 * 4);
            ra[i] = *reinterpret_cast<const float4 *>(ab + (size_t)row * Cp + c4 * 4);
        }
    };
    auto lstore = [&](int buf) {
        float *Qs = smem + buf * 2 * TILE_FLOATS, *As = Qs + TILE_FLOATS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = t + MATCH_THREADS * i, row = f >> 3, c4 = f & 7;
            float *q = Qs + row * LD + c4 * 4, *a = As + row * LD + c4 * 4;
            q[0] = rq[i].x; q[1] = rq[i].y; q[2] = rq[i].z; q[3] = rq[i].w;
            a[0] = ra[i].x; a[1] = ra[i].y; a[2] = ra[i].z; a[3] = ra[i].w;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.0f;

    float best[2] = {INFINITY, INFINITY};
    int bidx[2] = {0x7fffffff, 0x7fffffff};

    if (nit > 0) {
        gload(0);
        lstore(0);
    }
    __syncthreads();

    int fb = 0;
    for (int it = 0; it < nit; ++it) {
        const int cur = it & 1;
        const bool more = it + 1 < nit;
        const bool fold = (it % KT) == KT - 1;
        const int q0 = (qt_begin + it / KT) * MT;
        if (more) gload(it + 1);

        const float *Qs = smem + cur * 2 * TILE_FLOATS + (wm * 64 + l31) * LD + 4 * hi;
        const float *As = smem + cur * 2 * TILE_FLOATS + TILE_FLOATS + (wn * 64 + l31) * LD + 4 * hi;
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            const int kp = 8 * (ks >> 2) + (ks & 3);
            const float q0v = Qs[kp], q1v = Qs[32 * LD + kp];
            const float b0 = As[kp], b1 = As[32 * LD + kp];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(q0v, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(q0v, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(q1v, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(q1v, b1, acc[1][1], 0, 0, 0);
        }

        if (fold) {
            const bool masked = !(full_a && q0 + MT <= nq);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                unsigned rk = 0u;
                int ri = 0;
                int lsel = l31;
                asm volatile("" : "+v"(lsel));              // the sixteen lane == r masks are made here, not kept in scalar registers across the loop
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int q = q0 + wm * 64 + mi * 32 + acc_row(r, hi);
                    float d[2];
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        d[ni] = __fmaf_rn(-0.5f, acc[mi][ni][r], 0.5f);
                        if (masked) d[ni] = (a_ok[ni] && q < nq) ? d[ni] : INFINITY;
                        const bool better = d[ni] < best[ni];   // strict: first (smallest) query index wins ties
                        best[ni] = better ? d[ni] : best[ni];
                        bidx[ni] = better ? q : bidx[ni];
                        acc[mi][ni][r] = 0.0f;
                    }
                    // the two accumulators share the query row: fold them in the lane, then across the half-wave; the lower
                    // anchor block wins ties whatever the lane
                    const unsigned u0 = dist_key(d[0]), u1 = dist_key(d[1]);
                    const unsigned rm = half_min(min(u0, u1));
                    const int f0 = half_first(__ballot(u0 == rm), hi), f1 = half_first(__ballot(u1 == rm), hi);
                    rk = (lsel == r) ? rm : rk;
                    ri = (lsel == r) ? (f0 >= 0 ? f0 : 32 + f1) : ri;
                    if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // a few rows' ballots in flight, not all sixteen (scalar registers)
                }
                const int ql = wm * 64 + mi * 32 + acc_row(l31 & 15, hi);
                if (l31 < 16 && q0 + ql < nq) atomicMin(&red[fb][ql], rev_key(rk, a0 + wn * 64 + ri));
            }
        }
        if (more) lstore(cur ^ 1);
        __syncthreads();
        if (fold) {
            rev_flush(red[fb], MT, q0, nq, keys_p);
            fb ^= 1;
        }
    }

#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const float od = __shfl_xor(best[ni], 32);
        const int oi = __shfl_xor(bidx[ni], 32);
        lex_min(best[ni], bidx[ni], od, oi);
    }
    float *sd = smem;
    int *si = reinterpret_cast<int *>(smem + 2 * MT);
    if (hi == 0) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            sd[wm * MT + wn * 64 + ni * 32 + l31] = best[ni];
            si[wm * MT + wn * 64 + ni * 32 + l31] = bidx[ni];
        }
    }
    __syncthreads();
    if (t < MT && a0 + t < na) {
        float d = sd[t];
        int i = si[t];
        lex_min(d, i, sd[MT + t], si[MT + t]);
        if (S == 1) {
            const size_t o = (size_t)p * cap_a + a0 + t;
            min_dist[o] = d;
            argmin[o] = (i == 0x7fffffff) ? 0 : i;
            valid[o] = (d < thr) ? 1 : 0;
        } else {
            const size_t o = ((size_t)p * S + split) * cap_a + a0 + t;
            ws_dist[o] = d;
            ws_idx[o] = i;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the join
// thread i of pair p: query row i's key -> rev_min_dist / rev_argmin; anchor row i's splits merged (S > 1) or read back (S == 1), and
// mutual from the key of ITS nearest query row.
__global__ void match_mutual_join_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ ws_dist,
                                         const int32_t *__restrict__ ws_idx, int S, int cap_a, int cap_q, const int32_t *__restrict__ n_a,
                                         const int32_t *__restrict__ n_q, float thr, float *__restrict__ min_dist,
                                         int32_t *__restrict__ argmin, uint8_t *__restrict__ valid, float *__restrict__ rev_min_dist,
                                         int32_t *__restrict__ rev_argmin, uint8_t *__restrict__ mutual)
{
    const int p = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int na = n_a[p], nq = n_q[p];
    const unsigned long long *keys_p = keys + (size_t)p * cap_q;
    if (i < nq) {
        float d;
        int j;
        rev_unkey(keys_p[i], d, j);
        rev_min_dist[(size_t)p * cap_q + i] = d;
        rev_argmin[(size_t)p * cap_q + i] = j;
    }
    if (i < na) {
        const size_t o = (size_t)p * cap_a + i;
        float d;
        int j;
        if (S > 1) {
            d = INFINITY;
            j = 0x7fffffff;
            for (int s = 0; s < S; ++s) {
                const size_t w = ((size_t)p * S + s) * cap_a + i;
                lex_min(d, j, ws_dist[w], ws_idx[w]);
            }
            j = (j == 0x7fffffff) ? 0 : j;
            min_dist[o] = d;
            argmin[o] = j;
            valid[o] = (d < thr) ? 1 : 0;
        } else {
            d = min_dist[o];
            j = argmin[o];
        }
        uint8_t m = 0;
        if (d < thr && j < nq) {                      // a valid row has a finite distance, so nq > 0 and its query row has a key
            float rd_;
            int ri;
            rev_unkey(keys_p[j], rd_, ri);
            m = (ri == i) ? 1 : 0;
        }
        mutual[o] = m;
    }
}

struct MutualWs : SplitWs {
    unsigned long long *keys;
};
static size_t carve_mutual(void *base, MutualWs &w, int B, int cap_a, int cap_q, int S)
{
    Carver carve(base);
    carve(w.keys, (size_t)B * cap_q);
    return carve_split(base, w, B, cap_a, S, carve.off);
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_match_mutual_workspace_bytes(int B, int cap_a, int cap_q)
{
    if (B <= 0 || cap_a <= 0 || cap_q <= 0) return 0;
    MutualWs w;
    return carve_mutual(nullptr, w, B, cap_a, cap_q, match_f32_split(B, cap_a / MT));
}

extern "C" int oryon_match_mutual_f32(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q, const int32_t *n_a,
                                      const int32_t *n_q, float threshold, float *min_dist, int32_t *argmin, uint8_t *valid,
                                      float *rev_min_dist, int32_t *rev_argmin, uint8_t *mutual, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    ORYON_CHECK_ARG(a_hat && q_hat && n_a && n_q);
    ORYON_CHECK_ARG(min_dist && argmin && valid && rev_min_dist && rev_argmin && mutual);
    ORYON_CHECK_ARG(B >= 0 && B <= 65535);
    ORYON_CHECK_ARG(C > 0 && C % BK == 0);
    ORYON_CHECK_ARG(cap_a > 0 && cap_a % MT == 0);
    ORYON_CHECK_ARG(cap_q > 0 && cap_q % MT == 0);
    ORYON_CHECK_ARG(C != 32 || cap_q % 256 == 0);       // the C_pad 32 kernel streams the query rows in tiles of 256
    if (B == 0) return ORYON_OK;
    const int T = cap_a / MT;
    const int S = match_f32_split(B, T);
    MutualWs w;
    const size_t need = carve_mutual(workspace, w, B, cap_a, cap_q, S);
    ORYON_CHECK_WORKSPACE("oryon_match_mutual_f32: ", workspace, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    ORYON_CHECK_HIP(hipMemsetAsync(w.keys, 0xff, (size_t)B * cap_q * sizeof(unsigned long long), st));     // KEY_NONE
    const int groups = staged_groups(B, T, S), groups_regb = regb_groups(B, T, S);
#define LAUNCH_REGB(CPV)                                                                                                       \
    hipLaunchKernelGGL((match_mutual_regb_kernel<CPV>), dim3(groups_regb), dim3(MATCH_THREADS), 0, st, a_hat, q_hat, B, cap_a, cap_q, \
                       n_a, n_q, threshold, T, S, min_dist, argmin, valid, w.ws_dist, w.ws_idx, w.keys)
    if (C == 32) LAUNCH_REGB(32);
    else if (C == 64) LAUNCH_REGB(64);
    else if (C == 128) LAUNCH_REGB(128);
    else if (C == 256) LAUNCH_REGB(256);
    else
        hipLaunchKernelGGL(match_mutual_staged_kernel, dim3(groups), dim3(MATCH_THREADS), 0, st, a_hat, q_hat, B, C, cap_a, cap_q, n_a, n_q,
                           threshold, T, S, min_dist, argmin, valid, w.ws_dist, w.ws_idx, w.keys);
#undef LAUNCH_REGB
    ORYON_CHECK_LAUNCH();
    const int rows = cap_a > cap_q ? cap_a : cap_q;
    hipLaunchKernelGGL(match_mutual_join_kernel, dim3(rows / 256 + 1, B), dim3(256), 0, st, w.keys, w.ws_dist, w.ws_idx, S, cap_a, cap_q,
                       n_a, n_q, threshold, min_dist, argmin, valid, rev_min_dist, rev_argmin, mutual);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
