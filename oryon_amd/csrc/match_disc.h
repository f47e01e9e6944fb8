// The exclusion disc of K1r (match_second.hip) and K1n (match_next.hip): a query row's pixel packed into one word, the integer disc
// rule, the pixel stage of a query tile in LDS and an anchor's centre pixel.
#pragma once
#include "common.h"
#include "match_tile.h"

namespace oryon {

constexpr int PIX_NONE = -(1 << 20);       // an anchor without a nearest row (n_q == 0, or an index outside the pair): nothing is excluded

__device__ __forceinline__ unsigned pack_pixel(int idx, int W) { const int y = idx / W; return ((unsigned)y << 16) | (unsigned)(idx - y * W); }
// (y - y*)^2 + (x - x*)^2 >= r^2 in integers; r <= 1024, so the squares are formed only where they cannot overflow
__device__ __forceinline__ bool outside_disc(unsigned pk, int ys, int xs, int r)
{
    const int dy = abs((int)(pk >> 16) - ys), dx = abs((int)(pk & 0xffffu) - xs);
    return dy >= r || dx >= r || dy * dy + dx * dx >= r * r;
}

// what the folds share: the pixel stage of a tile of ROWS query rows (thread t < ROWS owns row t) and an anchor's (y*, x*)
template <int ROWS> struct PixelStage {
    unsigned *pix;                          // LDS [2][ROWS]
    const int32_t *roi;                     // the pair's query pixel list
    int nq, W;
    unsigned pre = 0;
    int slot = 0;
    __device__ __forceinline__ void prefetch(int qt)
    {
        const int t = threadIdx.x, q = qt * ROWS + t;
        slot = (qt & 1) * ROWS + t;
        if (t < ROWS) pre = (q < nq) ? pack_pixel(roi[q], W) : 0u;
    }
    __device__ __forceinline__ void publish()
    {
        if ((int)threadIdx.x < ROWS) pix[slot] = pre;
    }
    __device__ __forceinline__ const unsigned *rows(int qt) const { return pix + (qt & 1) * ROWS; }
};
__device__ __forceinline__ void star_pixel(const int32_t *__restrict__ argmin_p, const int32_t *__restrict__ roi, int a, int na, int nq, int W,
                                           int &ys, int &xs)
{
    ys = xs = PIX_NONE;
    if (a < na) {
        const int j = argmin_p[a];
        if (j >= 0 && j < nq) {
            const unsigned pk = pack_pixel(roi[j], W);
            ys = (int)(pk >> 16);
            xs = (int)(pk & 0xffffu);
        }
    }
}

}  // namespace oryon
