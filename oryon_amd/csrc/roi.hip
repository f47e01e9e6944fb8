// K0 family: masks -> ROI lists -> (subsample) -> gathered, L2-normalised descriptor rows.
// Replaces utils/pcd.py:184-193, losses.py:58-59, pipeline.py:408-411 of the reference (see include/oryon_hip.h).
// All of this is HBM-bound integer/gather work: coalesced row-major scans, wave ballots for the ordered
// compaction, an LDS transpose so the [N,C] descriptor rows are written in 128-byte runs.
#include <hip/hip_fp16.h>
#include <stdlib.h>
#include "common.h"
#include "match_common.h"
#include "match_exact.h"

namespace oryon {

constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_WAVES = SCAN_THREADS / 64;

// Ordered (stable) block compaction step: every thread contributes `flag`; returns this thread's output
// slot (valid when flag) relative to the chunk start and the chunk total through `total`.
__device__ __forceinline__ int block_rank(bool flag, int *s_wave /*[SCAN_WAVES]*/, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();                       // previous user of s_wave is done
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
        const int c = s_wave[w];
        base += (w < wave) ? c : 0;
        tot += c;
    }
    total = tot;
    return base + before;
}

// Ordered block scan of per-thread COUNTS (exclusive): this thread's offset inside the chunk, the chunk total through `total`.
__device__ __forceinline__ int block_scan_counts(int cnt, int *s_wave /*[SCAN_WAVES]*/, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o);
        incl += (lane >= o) ? v : 0;
    }
    __syncthreads();                       // previous user of s_wave is done
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
        const int c = s_wave[w];
        base += (w < wave) ? c : 0;
        tot += c;
    }
    total = tot;
    return base + incl - cnt;
}

// `chunks` workgroups per map, EIGHT consecutive pixels per thread and scan step (two 16-byte loads), and RC_STEPS scan steps settled
// behind ONE pair of barriers: a 224 x 224 map (7 steps of 8192 pixels) has all its loads in flight at once and one hand-over of the
// wave totals through LDS instead of seven dependent load -> scan -> barrier rounds.
// Chunk c of a map compacts the pixels [c CL, (c + 1) CL) (CL = ceil(HW / chunks) rounded up to eight); where its entries start in the
// map's list it counts for itself, with a store-free pass over the pixels in front of its own: the ROI stores (up to 64 predicated
// 4-byte stores per thread) are what the kernel's time goes to, a second read of half a mask costs a few microseconds.  The launches
// deal 256 workgroups or fewer: the 64 + 64 maps of a cfg2 step get two chunks each.
// Up to two mask sets per launch: the workgroups of the second half of the grid take the second one (the engine's K0 section compacts
// the anchor and the query masks of a step with one launch).  zero0 / zero1 (may be NULL): one word per map that the map's first
// workgroup clears - the error-norm word of the gather that follows on the same stream.
constexpr int RC_STEPS = 8;
inline int roi_compact_chunks(int maps) { return maps >= 256 ? 1 : (256 / maps < 4 ? 256 / maps : 4); }
__global__ __launch_bounds__(SCAN_THREADS) void roi_compact_kernel(const int32_t *__restrict__ mask0, const int32_t *__restrict__ mask1,
                                                                    int n_maps, int chunks, int HW, int32_t *__restrict__ roi0,
                                                                    int32_t *__restrict__ roi1, int32_t *__restrict__ count0,
                                                                    int32_t *__restrict__ count1, float *__restrict__ zero0,
                                                                    float *__restrict__ zero1)
{
    __shared__ __align__(16) int s_wave[RC_STEPS][SCAN_WAVES];
    const int chunk = (int)blockIdx.x % chunks, map = (int)blockIdx.x / chunks;
    const bool second = map >= n_maps;
    const int m = second ? map - n_maps : map;
    const int32_t *mk = (second ? mask1 : mask0) + (size_t)m * HW;
    int32_t *out = (second ? roi1 : roi0) + (size_t)m * HW;
    float *zero = second ? zero1 : zero0;
    const int CL = ((HW + chunks - 1) / chunks + 7) / 8 * 8;
    const int first = chunk * CL < HW ? chunk * CL : HW, end = first + CL < HW ? first + CL : HW;
    const bool vec = (HW % 4 == 0) && ((reinterpret_cast<uintptr_t>(mk) & 15) == 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    if (first > 0) {
        // ROI pixels in front of this chunk (first is a multiple of eight, or HW for a chunk that lies beyond a small map's end)
        int mine = 0;
        for (int p = (int)threadIdx.x * 8; p < first; p += SCAN_THREADS * 8) {
            if (vec && p + 8 <= first) {
                const int4 a = *reinterpret_cast<const int4 *>(mk + p), b = *reinterpret_cast<const int4 *>(mk + p + 4);
                mine += (a.x == 1) + (a.y == 1) + (a.z == 1) + (a.w == 1) + (b.x == 1) + (b.y == 1) + (b.z == 1) + (b.w == 1);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) mine += (p + e < first && mk[p + e] == 1) ? 1 : 0;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        if (lane == 0) s_wave[0][wave] = mine;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < SCAN_WAVES; ++w) base += s_wave[0][w];
    }
    for (int p0 = first; p0 < end; p0 += RC_STEPS * SCAN_THREADS * 8) {
        unsigned bits[RC_STEPS];
#pragma unroll
        for (int s = 0; s < RC_STEPS; ++s) {
            const int p = p0 + (s * SCAN_THREADS + (int)threadIdx.x) * 8;
            int v[8];
            if (vec && p + 8 <= end) {
                const int4 a = *reinterpret_cast<const int4 *>(mk + p), b = *reinterpret_cast<const int4 *>(mk + p + 4);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (p + e < end) ? mk[p + e] : 0;
            }
            unsigned bt = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) bt |= (v[e] == 1 ? 1u : 0u) << e;
            bits[s] = bt;
        }
        // inclusive scan inside the wave, every step on its own (independent chains)
        int incl[RC_STEPS];
#pragma unroll
        for (int s = 0; s < RC_STEPS; ++s) incl[s] = __popc(bits[s]);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
            for (int s = 0; s < RC_STEPS; ++s) {
                const int v = __shfl_up(incl[s], o);
                incl[s] += (lane >= o) ? v : 0;
            }
        }
        __syncthreads();                       // the previous group's readers of s_wave are done
        if (lane == 63) {
#pragma unroll
            for (int s = 0; s < RC_STEPS; ++s) s_wave[s][wave] = incl[s];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < RC_STEPS; ++s) {
            int before = 0, tot = 0;
#pragma unroll
            for (int w4 = 0; w4 < SCAN_WAVES; w4 += 4) {
                const int4 c = *reinterpret_cast<const int4 *>(&s_wave[s][w4]);
                before += (w4 + 0 < wave ? c.x : 0) + (w4 + 1 < wave ? c.y : 0) + (w4 + 2 < wave ? c.z : 0) + (w4 + 3 < wave ? c.w : 0);
                tot += c.x + c.y + c.z + c.w;
            }
            const int p = p0 + (s * SCAN_THREADS + (int)threadIdx.x) * 8;
            int o = base + before + incl[s] - __popc(bits[s]);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (bits[s] & (1u << e)) out[o++] = p + e;
            base += tot;
        }
    }
    if (threadIdx.x == 0) {
        if (chunk == chunks - 1) (second ? count1 : count0)[m] = base;
        if (zero && chunk == 0) zero[m] = 0.0f;
    }
}

__global__ void mask_from_logits_kernel(const float *__restrict__ logits, int64_t n, float thr, int32_t *__restrict__ mask)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float s = 1.0f / (1.0f + expf(-logits[i]));
        mask[i] = s > thr ? 1 : 0;
    }
}

__global__ void mask_resize_nearest_kernel(const uint8_t *__restrict__ in, int HI, int WI, int HO, int WO,
                                           int32_t *__restrict__ out)
{
    const int m = blockIdx.y;
    const float sy = (float)HI / (float)HO, sx = (float)WI / (float)WO;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HO * WO; p += gridDim.x * blockDim.x) {
        const int y = p / WO, x = p % WO;
        int ys = (int)floorf((float)y * sy), xs = (int)floorf((float)x * sx);
        ys = ys < HI - 1 ? ys : HI - 1;
        xs = xs < WI - 1 ? xs : WI - 1;
        out[(size_t)m * HO * WO + p] = (int32_t)in[((size_t)m * HI + ys) * WI + xs];
    }
}

// Subsample without replacement: keep the max_keep smallest 32-bit keys (ties by index), in ROI order.
__global__ __launch_bounds__(SCAN_THREADS) void roi_subsample_kernel(int32_t *__restrict__ roi, int32_t *__restrict__ count,
                                                                      int roi_stride, int max_keep, uint64_t seed,
                                                                      const int64_t *__restrict__ map_key)
{
    __shared__ int s_wave[SCAN_WAVES];
    __shared__ __align__(16) unsigned s_hist[256];
    __shared__ unsigned s_prefix, s_remaining;
    const int m = blockIdx.x;
    const int n = count[m];
    if (n <= max_keep) return;
    const uint64_t key = map_key ? (uint64_t)map_key[m] : (uint64_t)m;
    int32_t *r = roi + (size_t)m * roi_stride;

    if (threadIdx.x == 0) { s_prefix = 0u; s_remaining = (unsigned)max_keep; }
    // radix select, most significant byte first
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (threadIdx.x < 256) s_hist[threadIdx.x] = 0u;
        __syncthreads();
        const unsigned prefix = s_prefix;
        const unsigned hi_mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = threadIdx.x; i < n; i += SCAN_THREADS) {
            const unsigned k = rng_u32(seed, key, 0u, (uint32_t)i);
            if ((k & hi_mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 0xFFu], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {                                     // the bin walk, by the first wave (common.h)
            const unsigned rem = s_remaining;
            unsigned cum;
            const int b = radix_pick(s_hist, rem, cum);
            if (threadIdx.x == 0) {
                s_remaining = rem - cum;
                s_prefix = prefix | ((unsigned)b << shift);
            }
        }
        __syncthreads();
    }
    const unsigned T = s_prefix;
    const int ties_to_take = (int)s_remaining;
    int kept = 0, ties_seen = 0;
    // eight consecutive entries per thread and scan step (as roi_compact_kernel): 2 steps for 12.5 k entries instead of 13
    for (int i0 = 0; i0 < n; i0 += SCAN_THREADS * 8) {
        const int i = i0 + (int)threadIdx.x * 8;
        int32_t v[8];
        unsigned below = 0u, tie = 0u;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool in = i + e < n;
            const unsigned k = in ? rng_u32(seed, key, 0u, (uint32_t)(i + e)) : 0xFFFFFFFFu;
            v[e] = in ? r[i + e] : 0;
            below |= (in && k < T ? 1u : 0u) << e;
            tie |= (in && k == T ? 1u : 0u) << e;
        }
        int tie_total;
        int tie_rank = ties_seen + block_scan_counts(__popc(tie), s_wave, tie_total);
        unsigned keep = below;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (tie & (1u << e)) { if (tie_rank < ties_to_take) keep |= 1u << e; ++tie_rank; }
        int keep_total;
        int pos = kept + block_scan_counts(__popc(keep), s_wave, keep_total);
        // all reads of this chunk (v) happened before the scans' barriers -> in-place write is safe
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (keep & (1u << e)) r[pos++] = v[e];
        kept += keep_total;
        ties_seen += tie_total;
    }
    if (threadIdx.x == 0) count[m] = kept;
}

// Gather + normalise.  One thread per ROI row for the (canonical, k-ordered) norm; the scaled values go
// through an LDS transpose so global stores are 128-byte runs of one descriptor row.
constexpr int GN_ROWS = 256;
constexpr int GN_KT = 32;
__global__ __launch_bounds__(GN_ROWS) void gather_normalise_kernel(const float *__restrict__ feat, int C, int HW,
                                                                    const int32_t *__restrict__ roi, int roi_stride,
                                                                    const int32_t *__restrict__ count, int rows_cap,
                                                                    int Cp, float *__restrict__ out,
                                                                    __half *__restrict__ out16)
{
    __shared__ float tile[GN_ROWS * (GN_KT + 1)];
    const int m = blockIdx.y;
    const int n = count[m];
    const int row0 = blockIdx.x * GN_ROWS;
    if (row0 >= n) return;                       // only the last partially filled block zero-fills
    const int t = threadIdx.x;
    const int row = row0 + t;
    const bool live = row < n;
    const float *f = feat + (size_t)m * C * HW;
    const int pix = live ? roi[(size_t)m * roi_stride + row] : 0;
    float n2 = 0.0f;
    if (live)
        for (int k = 0; k < C; ++k) {
            const float v = f[(size_t)k * HW + pix];
            n2 = __fmaf_rn(v, v, n2);
        }
    float d = sqrt_rn(n2);
    d = d < 1e-8f ? 1e-8f : d;
    float *o = out + ((size_t)m * rows_cap + row0) * Cp;
    for (int k0 = 0; k0 < Cp; k0 += GN_KT) {
#pragma unroll 8
        for (int kk = 0; kk < GN_KT; ++kk) {
            const float v = (live && k0 + kk < C) ? __fdiv_rn(f[(size_t)(k0 + kk) * HW + pix], d) : 0.0f;
            tile[t * (GN_KT + 1) + kk] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < (GN_ROWS * GN_KT / 4) / GN_ROWS; ++i) {
            const int fidx = t + GN_ROWS * i;
            const int r = fidx / (GN_KT / 4), c4 = fidx % (GN_KT / 4);
            // k-permuted row layout consumed by K1 (match_exact.h: kperm_k), c4 = 2g + h
            const int kg = c4 >> 1, kh = c4 & 1;
            float4 v;
            v.x = tile[r * (GN_KT + 1) + kperm_k(kg, kh, 0)];
            v.y = tile[r * (GN_KT + 1) + kperm_k(kg, kh, 1)];
            v.z = tile[r * (GN_KT + 1) + kperm_k(kg, kh, 2)];
            v.w = tile[r * (GN_KT + 1) + kperm_k(kg, kh, 3)];
            *reinterpret_cast<float4 *>(o + (size_t)r * Cp + k0 + c4 * 4) = v;
        }
        if (out16) {
            // fp16 copy of the same unit rows in NATURAL k order (operand of the screening pass K1s): 8 halves per store
            __half *o16 = out16 + ((size_t)m * rows_cap + row0) * Cp;
#pragma unroll
            for (int i = 0; i < (GN_ROWS * GN_KT / 8) / GN_ROWS; ++i) {
                const int fidx = t + GN_ROWS * i;
                const int r = fidx / (GN_KT / 8), c8 = fidx % (GN_KT / 8);
                union { __half h[8]; uint4 u; } pk;
#pragma unroll
                for (int e = 0; e < 8; ++e) pk.h[e] = __float2half_rn(tile[r * (GN_KT + 1) + c8 * 8 + e]);
                *reinterpret_cast<uint4 *>(o16 + (size_t)r * Cp + k0 + c8 * 8) = pk.u;
            }
        }
        __syncthreads();
    }
}

// Second-generation gather + normalise (C_pad <= 512).  A workgroup owns ROWS ROI rows of one map and keeps their raw channel
// values in LDS ([k][row], one float of padding per k), so the channel-planar map is read from HBM exactly once:
//   load    all 4 waves, lane = row: every channel is one 128/256-byte run (each in its own DRAM page - this phase runs at
//           ~3.7 TB/s on its own and bounds the kernel), NL loads in flight per lane
//   norm    wave 0 runs the canonical k-ordered fmaf chain per row out of LDS (bit-exact vs the oracle)
//   store   all waves divide and write FULL 128-byte lines: fp32 rows k-permuted in 16-byte chunks, fp16 rows in natural
//           order (64-byte partial-line stores cost 3x per byte on this memory system, measured)
// Phases of different workgroups overlap on a CU (4 workgroups at C_pad = 256); a register-staged software pipeline inside a
// persistent workgroup (next tile's loads in flight under norm + stores) measured only 5-7 % faster on the same GPU and was
// not kept.
// (callers pad row capacities to 256: the zero-fill granularity)
template <int NL, int ROWS>        // NL: channel loads in flight per lane; ROWS: ROI rows per workgroup (32 or 64)
__global__ __launch_bounds__(256) void gather_normalise_v2_kernel(const float *__restrict__ feat, int C, int HW,
                                                                   const int32_t *__restrict__ roi, int roi_stride,
                                                                   const int32_t *__restrict__ count, int rows_cap, int Cp,
                                                                   float *__restrict__ out, __half *__restrict__ out16)
{
    constexpr int LD = ROWS + 1;
    constexpr int CPW = 64 / ROWS;             // channels one wave instruction covers (1 or 2)
    constexpr int KSTEP = 4 * CPW;             // channel stride between a lane's consecutive values
    constexpr int NRG = ROWS / 8;              // 8-row groups; waves beyond NRG split the k range instead
    constexpr int KSPLIT = NRG >= 4 ? 1 : 4 / NRG;
    extern __shared__ float raw[];             // [Cp][LD] raw values, then sd[ROWS] norms
    float *sd = raw + (size_t)Cp * LD;
    const int m = blockIdx.y;
    const int n = count[m];
    const int row0 = blockIdx.x * ROWS;
    // zero-fill contract: rows [n, round_up(n, 256)) must be written as zeros
    const int n_fill = (n + 255) / 256 * 256;
    if (row0 >= n_fill) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float *f = feat + (size_t)m * C * HW;
    const int lrow = lane & (ROWS - 1);
    const int kfirst = wave * CPW + lane / ROWS;
    const int my_row = row0 + lrow;
    const bool live = my_row < n;
    const int pix = live ? roi[(size_t)m * roi_stride + my_row] : 0;
    for (int kb = kfirst; kb < Cp; kb += KSTEP * NL) {
        float v[NL];
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int k = kb + KSTEP * u;
            v[u] = (live && k < C) ? f[(size_t)k * HW + pix] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int k = kb + KSTEP * u;
            if (k < Cp) raw[k * LD + lrow] = v[u];
        }
    }
    __syncthreads();
    if (wave == 0 && lane < ROWS) {
        float n2 = 0.0f;
        for (int k0 = 0; k0 < C; k0 += 16) {
            float x[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) x[u] = (k0 + u < C) ? raw[(k0 + u) * LD + lane] : 0.0f;
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (k0 + u < C) n2 = __fmaf_rn(x[u], x[u], n2);
        }
        float d = sqrt_rn(n2);
        sd[lane] = d < 1e-8f ? 1e-8f : d;
    }
    __syncthreads();
    float *o = out + ((size_t)m * rows_cap + row0) * Cp;
    // fp32, k-permuted: lane -> (row_sub 0..7, chunk c4 0..7) of a 32-wide k group; 8 rows x 128 bytes per instruction
    for (int rg = wave % NRG; rg < NRG; rg += 4) {
        const int r = rg * 8 + (lane >> 3), c4 = lane & 7;
        const float d = sd[r];
        const int kg = c4 >> 1, kh = c4 & 1;        // the chunk's (g, h) of the k-permuted format (match_exact.h)
        for (int k0 = 32 * (wave / NRG); k0 < Cp; k0 += 32 * KSPLIT) {
            float4 q;
            q.x = __fdiv_rn(raw[(k0 + kperm_k(kg, kh, 0)) * LD + r], d);
            q.y = __fdiv_rn(raw[(k0 + kperm_k(kg, kh, 1)) * LD + r], d);
            q.z = __fdiv_rn(raw[(k0 + kperm_k(kg, kh, 2)) * LD + r], d);
            q.w = __fdiv_rn(raw[(k0 + kperm_k(kg, kh, 3)) * LD + r], d);
            *reinterpret_cast<float4 *>(o + (size_t)r * Cp + k0 + c4 * 4) = q;
        }
    }
    if (out16) {
        __half *o16 = out16 + ((size_t)m * rows_cap + row0) * Cp;
        if (Cp >= 64) {
            // fp16, natural order: lane -> (row_sub 0..7, chunk c8 0..7) of a 64-wide k group
            for (int rg = wave % NRG; rg < NRG; rg += 4) {
                const int r = rg * 8 + (lane >> 3), c8 = lane & 7;
                const float d = sd[r];
                for (int k0 = 64 * (wave / NRG); k0 < Cp; k0 += 64 * KSPLIT) {
                    if (k0 + c8 * 8 >= Cp) continue;
                    union { __half h[8]; uint4 u; } pk;
#pragma unroll
                    for (int e = 0; e < 8; ++e) pk.h[e] = __float2half_rn(__fdiv_rn(raw[(k0 + c8 * 8 + e) * LD + r], d));
                    *reinterpret_cast<uint4 *>(o16 + (size_t)r * Cp + k0 + c8 * 8) = pk.u;
                }
            }
        } else {
            // 64-byte rows are adjacent in memory: lane -> (row_sub 0..15, chunk c8 0..3), one contiguous 1 KB run
            constexpr int NRG16 = ROWS / 16;
            const int r = (wave % NRG16) * 16 + (lane >> 2), c8 = lane & 3;
            const float d = sd[r];
            if (wave < NRG16) {
                union { __half h[8]; uint4 u; } pk;
#pragma unroll
                for (int e = 0; e < 8; ++e) pk.h[e] = __float2half_rn(__fdiv_rn(raw[(c8 * 8 + e) * LD + r], d));
                *reinterpret_cast<uint4 *>(o16 + (size_t)r * Cp + c8 * 8) = pk.u;
            }
        }
    }
}

// K0 with the int8 copies for K1s8 (C_pad 256 / 512, 32-row tiles): everything gather_normalise_v2_kernel<.,32> writes, plus
//   out8   [n_maps, rows_cap, Cp] int8:  q = rint(x^ * 2^E), |q| <= 127, with ONE exponent E per 16-row slice of the screening
//          kernel's accumulator layout (rows {0-3,8-11,16-19,24-27} + 4*h of each 32-row block, h = 0/1), so that the
//          integer maximum over a slice is also its score maximum
//   scale  [n_maps, rows_cap/16] fp32 = 2^-E per slice (slice id = (row / 32) * 2 + h)
//   eps_max[n_maps] fp32 = max over the map's slices of 2^-(E+1), the per-element quantisation bound (atomic max on the bits)
// x^ is the canonical fp32 value (fdiv), so |q * 2^-E - x^| <= 2^-(E+1) exactly as match16.hip's error analysis needs.
template <int NL>
__global__ __launch_bounds__(256) void gather_normalise_q8_kernel(const float *__restrict__ feat, int C, int HW,
                                                                   const int32_t *__restrict__ roi, int roi_stride,
                                                                   const int32_t *__restrict__ count, int rows_cap, int Cp,
                                                                   float *__restrict__ out, __half *__restrict__ out16,
                                                                   int8_t *__restrict__ out8, float *__restrict__ scale,
                                                                   unsigned *__restrict__ eps_max)
{
    constexpr int ROWS = 32, LD = ROWS + 1, CPW = 2, KSTEP = 8;
    extern __shared__ float raw[];             // [Cp][LD] raw values -> unit values, then sd[ROWS] norms, smax[2] slice maxima
    float *sd = raw + (size_t)Cp * LD;
    unsigned *smax = reinterpret_cast<unsigned *>(sd + ROWS);
    const int m = blockIdx.y;
    const int n = count[m];
    const int row0 = blockIdx.x * ROWS;
    const int n_fill = (n + 255) / 256 * 256;
    if (row0 >= n_fill) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float *f = feat + (size_t)m * C * HW;
    const int lrow = lane & (ROWS - 1);
    const int kfirst = wave * CPW + lane / ROWS;
    const int my_row = row0 + lrow;
    const bool live = my_row < n;
    const int pix = live ? roi[(size_t)m * roi_stride + my_row] : 0;
    if (t < 2) smax[t] = 0u;
    for (int kb = kfirst; kb < Cp; kb += KSTEP * NL) {
        float v[NL];
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int k = kb + KSTEP * u;
            v[u] = (live && k < C) ? f[(size_t)k * HW + pix] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int k = kb + KSTEP * u;
            if (k < Cp) raw[k * LD + lrow] = v[u];
        }
    }
    __syncthreads();
    if (wave == 0 && lane < ROWS) {
        float n2 = 0.0f;
        for (int k0 = 0; k0 < C; k0 += 16) {
            float x[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) x[u] = (k0 + u < C) ? raw[(k0 + u) * LD + lane] : 0.0f;
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (k0 + u < C) n2 = __fmaf_rn(x[u], x[u], n2);
        }
        float d = sqrt_rn(n2);
        sd[lane] = d < 1e-8f ? 1e-8f : d;
    }
    __syncthreads();
    float *o = out + ((size_t)m * rows_cap + row0) * Cp;
    // fp32, k-permuted, and the unit value written back in place: lane -> (row_sub 0..7, chunk c4 0..7) of a 32-wide k group,
    // wave = 8-row group.  The slice maximum of |x^| rides along.
    {
        const int r = wave * 8 + (lane >> 3), c4 = lane & 7;
        const float d = sd[r];
        const int kg = c4 >> 1, kh = c4 & 1;        // the chunk's (g, h) of the k-permuted format (match_exact.h)
        float mx = 0.0f;
        for (int k0 = 0; k0 < Cp; k0 += 32) {
            float4 q;
            q.x = __fdiv_rn(raw[(k0 + kperm_k(kg, kh, 0)) * LD + r], d);
            q.y = __fdiv_rn(raw[(k0 + kperm_k(kg, kh, 1)) * LD + r], d);
            q.z = __fdiv_rn(raw[(k0 + kperm_k(kg, kh, 2)) * LD + r], d);
            q.w = __fdiv_rn(raw[(k0 + kperm_k(kg, kh, 3)) * LD + r], d);
            raw[(k0 + kperm_k(kg, kh, 0)) * LD + r] = q.x;
            raw[(k0 + kperm_k(kg, kh, 1)) * LD + r] = q.y;
            raw[(k0 + kperm_k(kg, kh, 2)) * LD + r] = q.z;
            raw[(k0 + kperm_k(kg, kh, 3)) * LD + r] = q.w;
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(q.x), fabsf(q.y))), fmaxf(fabsf(q.z), fabsf(q.w)));
            *reinterpret_cast<float4 *>(o + (size_t)r * Cp + k0 + c4 * 4) = q;
        }
        // a wave covers rows 8w..8w+7: lanes 0-31 belong to slice h = 0, lanes 32-63 to h = 1 -> reduce inside each half, one
        // LDS atomic per half-wave (non-negative floats order like their bit patterns)
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        if ((lane & 31) == 0) atomicMax(&smax[lane >> 5], __float_as_uint(mx));
    }
    __syncthreads();
    // slice exponents: 2^E * max|x^| <= 127
    float sc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float mxs = __uint_as_float(smax[h]);
        int E = mxs > 0.0f ? ilogbf(127.0f / mxs) : 30;
        E = E > 30 ? 30 : (E < 0 ? 0 : E);
        sc[h] = ldexpf(1.0f, E);
        if (t == h) {
            scale[(size_t)m * (rows_cap / 16) + (row0 / 32) * 2 + h] = ldexpf(1.0f, -E);
            if (row0 < n) atomicMax(&eps_max[m], __float_as_uint(ldexpf(1.0f, -E - 1)));
        }
    }
    {
        // fp16 (optional), natural order: lane -> (row_sub 0..7, chunk c8 0..7) of a 64-wide k group: 8 rows x one 128-byte line
        __half *o16 = out16 + ((size_t)m * rows_cap + row0) * Cp;
        const int r = wave * 8 + (lane >> 3), c8 = lane & 7;
        if (out16)
        for (int k0 = 0; k0 < Cp; k0 += 64) {
            union { __half h[8]; uint4 u; } pk;
#pragma unroll
            for (int e = 0; e < 8; ++e) pk.h[e] = __float2half_rn(raw[(k0 + c8 * 8 + e) * LD + r]);
            *reinterpret_cast<uint4 *>(o16 + (size_t)r * Cp + k0 + c8 * 8) = pk.u;
        }
        // int8, natural order: lane -> (row_sub 0..7, chunk c16 0..7) of a 128-wide k group: 8 rows x one 128-byte line
        int8_t *o8 = out8 + ((size_t)m * rows_cap + row0) * Cp;
        const float s8 = sc[(r >> 2) & 1];
        for (int k0 = 0; k0 < Cp; k0 += 128) {
            union { int8_t b[16]; uint4 u; } pk;
#pragma unroll
            for (int e = 0; e < 16; ++e) pk.b[e] = (int8_t)(int)rintf(raw[(k0 + c8 * 16 + e) * LD + r] * s8);
            *reinterpret_cast<uint4 *>(o8 + (size_t)r * Cp + k0 + c8 * 16) = pk.u;
        }
    }
}

// the engine's K0 section (match_common.h): both mask sets of a step in one launch; zero_a / zero_q as the kernel's zero0 / zero1
int roi_compact_pair_launch(const int32_t *mask_a, const int32_t *mask_q, int n_maps, int HW, int32_t *roi_a, int32_t *roi_q,
                            int32_t *n_a, int32_t *n_q, float *zero_a, float *zero_q, hipStream_t st)
{
    if (n_maps == 0) return ORYON_OK;
    const int chunks = roi_compact_chunks(2 * n_maps);
    hipLaunchKernelGGL(roi_compact_kernel, dim3(2 * n_maps * chunks), dim3(SCAN_THREADS), 0, st, mask_a, mask_q, n_maps, chunks, HW, roi_a, roi_q,
                       n_a, n_q, zero_a, zero_q);
    return hipGetLastError() == hipSuccess ? ORYON_OK : ORYON_ERR_HIP;
}

}  // namespace oryon

using namespace oryon;

extern "C" int oryon_roi_compact(const int32_t *mask, int n_maps, int HW, int32_t *roi, int32_t *count, void *stream)
{
    ORYON_CHECK_ARG(mask && roi && count && n_maps >= 0 && HW > 0);
    if (n_maps == 0) return ORYON_OK;
    const int chunks = roi_compact_chunks(n_maps);
    hipLaunchKernelGGL(roi_compact_kernel, dim3(n_maps * chunks), dim3(SCAN_THREADS), 0, as_stream(stream), mask, nullptr, n_maps, chunks, HW, roi,
                       nullptr, count, nullptr, nullptr, nullptr);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_mask_from_logits(const float *logits, int64_t n, float threshold, int32_t *mask, void *stream)
{
    ORYON_CHECK_ARG(logits && mask && n >= 0);
    if (n == 0) return ORYON_OK;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(mask_from_logits_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), logits, n, threshold, mask);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_mask_resize_nearest(const uint8_t *mask_in, int n_maps, int HI, int WI, int HO, int WO,
                                         int32_t *mask_out, void *stream)
{
    ORYON_CHECK_ARG(mask_in && mask_out && n_maps >= 0 && HI > 0 && WI > 0 && HO > 0 && WO > 0);
    if (n_maps == 0) return ORYON_OK;
    const int bx = ceil_div(HO * WO, 256) < 64 ? ceil_div(HO * WO, 256) : 64;
    hipLaunchKernelGGL(mask_resize_nearest_kernel, dim3(bx, n_maps), dim3(256), 0, as_stream(stream), mask_in, HI, WI, HO,
                       WO, mask_out);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_roi_subsample(int32_t *roi, int32_t *count, int n_maps, int roi_stride, int max_keep, uint64_t seed,
                                   const int64_t *map_key, void *stream)
{
    ORYON_CHECK_ARG(roi && count && n_maps >= 0 && roi_stride > 0 && max_keep > 0);
    if (n_maps == 0) return ORYON_OK;
    hipLaunchKernelGGL(roi_subsample_kernel, dim3(n_maps), dim3(SCAN_THREADS), 0, as_stream(stream), roi, count, roi_stride,
                       max_keep, seed, map_key);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_gather_normalise_q8(const float *feat, int n_maps, int C, int HW, const int32_t *roi, int roi_stride,
                                         const int32_t *count, int rows_cap, int C_pad, float *out, void *out_f16, int8_t *out_i8,
                                         float *slice_scale, float *eps_max, void *stream)
{
    ORYON_CHECK_ARG(feat && roi && count && out && out_i8 && slice_scale && eps_max);      // out_f16 may be NULL
    ORYON_CHECK_ARG(n_maps >= 0 && C > 0 && HW > 0 && roi_stride > 0 && C_pad >= C && (C_pad == 256 || C_pad == 512));
    ORYON_CHECK_ARG(rows_cap > 0 && rows_cap % 256 == 0);
    if (n_maps == 0) return ORYON_OK;
    hipStream_t st = as_stream(stream);
    ORYON_CHECK_HIP(hipMemsetAsync(eps_max, 0, (size_t)n_maps * sizeof(float), st));
    const size_t sh = ((size_t)C_pad * 33 + 32 + 8) * sizeof(float);
    allow_dynamic_lds(reinterpret_cast<const void *>(gather_normalise_q8_kernel<16>), 160 * 1024);   // 8 / 16 / 32 loads in flight measure the same
    hipLaunchKernelGGL((gather_normalise_q8_kernel<16>), dim3(rows_cap / 32, n_maps), dim3(256), sh, st, feat, C, HW, roi, roi_stride, count,
                       rows_cap, C_pad, out, static_cast<__half *>(out_f16), out_i8, slice_scale, reinterpret_cast<unsigned *>(eps_max));
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" int oryon_gather_normalise_f32(const float *feat, int n_maps, int C, int HW, const int32_t *roi, int roi_stride,
                                          const int32_t *count, int rows_cap, int C_pad, float *out, void *out_f16,
                                          void *stream)
{
    ORYON_CHECK_ARG(feat && roi && count && out && n_maps >= 0 && C > 0 && HW > 0 && roi_stride > 0);
    ORYON_CHECK_ARG(C_pad >= C && C_pad % GN_KT == 0);
    ORYON_CHECK_ARG(rows_cap > 0 && rows_cap % GN_ROWS == 0);
    if (n_maps == 0) return ORYON_OK;
    if (C_pad <= 512) {
        constexpr int rows = 32;
        const size_t sh = ((size_t)C_pad * (rows + 1) + 64) * sizeof(float);
#define LAUNCH_G2(NLV, RV)                                                                                                 \
    do {                                                                                                                   \
        allow_dynamic_lds(reinterpret_cast<const void *>(gather_normalise_v2_kernel<NLV, RV>), 160 * 1024);              \
        hipLaunchKernelGGL((gather_normalise_v2_kernel<NLV, RV>), dim3(rows_cap / RV, n_maps), dim3(256), sh, as_stream(stream), feat, \
                           C, HW, roi, roi_stride, count, rows_cap, C_pad, out, static_cast<__half *>(out_f16));          \
    } while (0)
        LAUNCH_G2(16, rows);
#undef LAUNCH_G2
    } else {
        hipLaunchKernelGGL(gather_normalise_kernel, dim3(rows_cap / GN_ROWS, n_maps), dim3(GN_ROWS), 0, as_stream(stream), feat,
                           C, HW, roi, roi_stride, count, rows_cap, C_pad, out, static_cast<__half *>(out_f16));
    }
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
