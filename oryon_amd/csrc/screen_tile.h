// What the screen kernels of match16.hip (K1s, K1s8) and screen_mx6.hip (K1s6) share: the 128-row query tile of 8-bit rows, the decode of a
// workgroup into (pair, query split, anchor panel), the DMA offsets of the swizzled tile and the merge of the two lane halves' running
// (m1, slice, m2) into the per-split triples.  Operand reads (koff, rd), the block reductions and the loops differ by format and stay with
// their kernels.  Inline code only: it is compiled with the flags of the file that includes it (screen_mx6.hip: -fno-honor-nans).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oryon {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int SCREEN8_ROWS = 128;                                          // query rows per tile of the int8 / MX-fp6 screens
constexpr int screen8_tile_bytes(int CP) { return CP * SCREEN8_ROWS; }     // one byte per channel (mx6: 24 code bytes + exponent + padding per 32)

// Workgroup -> (pair p, query split, anchor panel of panel_rows anchors, first anchor a0).  Units (p, split) go round the eight XCDs
// (blockIdx.x & 7), T panels per unit.  False: nothing to do - a unit beyond B * S or a panel beyond the pair's anchors - and the
// workgroup returns.
struct ScreenUnit {
    int p, split, panel, a0, na, nq;
};
__device__ __forceinline__ bool screen_unit_decode(ScreenUnit &u, int panel_rows, int B, int T, int S, const int32_t *__restrict__ n_a,
                                                   const int32_t *__restrict__ n_q)
{
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int unit = (slot / T) * 8 + xcd;
    if (unit >= B * S) return false;
    u.panel = slot % T;
    u.p = unit / S;
    u.split = unit % S;
    u.na = n_a[u.p];
    u.nq = n_q[u.p];
    u.a0 = u.panel * panel_rows;
    return u.a0 < u.na;
}
// the unit's share [qt_begin, qt_end) of the pair's ceil(n_q / 128) query tiles, dealt evenly to the S splits
__device__ __forceinline__ void screen_split_tiles(const ScreenUnit &u, int S, int &qt_begin, int &qt_end)
{
    const int nqt = (u.nq + SCREEN8_ROWS - 1) / SCREEN8_ROWS;
    const int qt_per = (nqt + S - 1) / S;
    qt_begin = u.split * qt_per;
    qt_end = (qt_begin + qt_per < nqt) ? qt_begin + qt_per : nqt;
}

// Byte offsets, inside a tile of RB-byte rows in global memory, of the 16 bytes this lane moves in the wave's DMA instructions
// first .. first + N - 1 (a wave's NI instructions are wave * NI ..).  One instruction moves four 256-byte lines (4 * 256 / RB rows) to
// consecutive LDS; the lane fetches the 16-byte chunk that belongs at its place of the swizzled image: chunk (sl ^ (row & 15)) of the line.
template <int RB, int N>
__device__ __forceinline__ void screen_dma_offsets(unsigned (&off)[N], int first, int lane)
{
    constexpr int LPR = RB / 256;                // 256-byte lines per row
    static_assert(LPR >= 1, "rows are whole 256-byte lines");
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int line = (first + j) * 4 + (lane >> 4), sl = lane & 15;
        const int row = line / LPR;
        off[j] = (unsigned)(row * RB + (((line % LPR) * 16 + (sl ^ (row & 15))) << 4));
    }
}

// The two lane halves of a wave hold the running (best, slice of best, best of the other slices) of the same NAB anchor columns over
// different query rows: merge them and store the split's triples at [(p * S + split) * cap_a + a] for the anchors a = a_lane + 32 ab
// (a_lane: the lane's anchor of block 0; unit = p * S + split).  Anchors of a last panel that reaches past cap_a are not stored.
template <int NAB>
__device__ __forceinline__ void screen_merge_store(const float (&runmax)[NAB], const float (&run2)[NAB], const int (&runidx)[NAB], int a_lane,
                                                   int hi, size_t unit, int cap_a, float *__restrict__ ws_max, int32_t *__restrict__ ws_i1,
                                                   float *__restrict__ ws_m2)
{
#pragma unroll
    for (int ab = 0; ab < NAB; ++ab) {
        const float om1 = __shfl_xor(runmax[ab], 32), om2 = __shfl_xor(run2[ab], 32);
        const int oi1 = __shfl_xor(runidx[ab], 32);
        const float m1 = fmaxf(runmax[ab], om1);
        const float m2 = fmaxf(fminf(runmax[ab], om1), fmaxf(run2[ab], om2));
        const int i1 = (om1 > runmax[ab]) ? oi1 : runidx[ab];
        const int a = a_lane + ab * 32;
        if (hi == 0 && a < cap_a) {
            const size_t o = unit * cap_a + a;
            ws_max[o] = m1;
            ws_i1[o] = i1;
            ws_m2[o] = m2;
        }
    }
}

}  // namespace oryon
