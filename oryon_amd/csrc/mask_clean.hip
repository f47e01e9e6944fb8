// Mask clean-up (test.mask_clean): connected-component labelling of binary object masks - fill the enclosed holes, then keep every
// component, the largest one, or those within a fraction of the largest.  The statement everything is tested against is
// include/oryon_hip.h, block h1 (tests/mask_clean_restatement.py is its numpy statement).  Everything is integer, and the
// label of a component - the smallest linear index among its pixels - is a property of the partition, not of the schedule: out, labels
// and stats are identical bytes across routes, launch geometries and runs.
//
// One algorithm, two homes for its state.  A union-find forest with one parent per PIXEL, parent <= pixel always:
//   init     a wave owns 64 consecutive pixels; the starts of the horizontal runs inside them come from one ballot and every pixel
//            starts as the child of its run's start, so a row segment is one tree before the first union
//   merge    the run pieces are joined to the left across the wave boundary and to the row above (x - 1, x, x + 1 for the foreground's
//            8-connectivity, x for the holes' 4-connectivity; a pixel whose left neighbour makes the same join leaves it to that one)
//            by an atomicMin union: the larger root becomes the child of the smaller, so the root is the component's smallest index
//   flatten  every pixel becomes the child of its root (one find per run piece, handed to its lanes by a shuffle)
//   areas    one integer atomicAdd of the piece's length per run piece; the largest area and, on a tie, the smallest label are ONE
//            64-bit atomicMax of (area << 32 | ~label)
// The hole pass is the same forest over the NON-foreground with 4-connectivity, run before the foreground pass: the border's background
// pixels are all joined to the first of them, and a background pixel whose root is not that tree's root is enclosed.
//
// LDS route (H * W <= ORYON_MASK_CLEAN_LDS_PIXELS): one 1024-lane workgroup per map, every pass separated by a workgroup barrier, the
// state in LDS from the first pass to the write-out: u16 parents (2 bytes a pixel: 128 KiB at 65 536 pixels - an index below 65 536 IS
// sixteen bits; whatever the map's shape), the foreground and the keep decisions as one bit a pixel each, and the area counters of a
// WINDOW of labels (whatever is left of the 160 KiB), swept over the label range.  LDS has no 16-bit atomicMin: it is a compare-and-swap
// on the 32-bit word that holds the label.  Global route: the same passes as launches, u32 parents, the foreground in `out` itself and one
// area counter per pixel in the workspace; a kernel boundary is the only grid-wide barrier.  Nowhere does a workgroup wait for memory
// another workgroup writes, and no pass is repeated until nothing changes.
#include "common.h"

namespace oryon {

constexpr int MC_STATS = ORYON_MASK_CLEAN_STATS;
constexpr int MC_LDS_PIXELS = ORYON_MASK_CLEAN_LDS_PIXELS;
constexpr int MC_LDS_BYTES = 160 * 1024;                 // what one workgroup may declare on gfx950
constexpr int MC_LDS_THREADS = 1024;
constexpr int MC_THREADS = 256, MC_MAX_BLOCKS = 512;     // global route: grid (min(ceil(HW / 256), 512), n_maps)
constexpr int MC_SCALARS = 16;                           // per map, uint32: the indices below; S_KEY is a uint64 (8-byte aligned)
enum : int { S_BORDER = 0, S_NCOMP = 1, S_FILLED = 2, S_KEPTC = 3, S_KEPTP = 4, S_TOTAL = 5, S_KEY = 6 };
constexpr uint32_t MC_NONE = 0xffffffffu;
static_assert(MC_STATS == 6 && MC_LDS_PIXELS <= 65536, "u16 labels hold indices below 65536");

using mc_mask_t = unsigned long long;                    // one bit per lane of a wave

template <class Lab> __device__ __forceinline__ uint32_t lab_load(const Lab *L, uint32_t i) { return __atomic_load_n(&L[i], __ATOMIC_RELAXED); }
__device__ __forceinline__ uint32_t lab_min(uint32_t *L, uint32_t i, uint32_t v) { return atomicMin(&L[i], v); }
// atomicMin on a 16-bit label: compare-and-swap on the aligned 32-bit word around it -> the label's previous value
__device__ __forceinline__ uint32_t lab_min(uint16_t *L, uint32_t i, uint32_t v)
{
    unsigned *w = reinterpret_cast<unsigned *>(L) + (i >> 1);
    const int sh = (int)(i & 1u) * 16;
    unsigned cur = __atomic_load_n(w, __ATOMIC_RELAXED);
    while (true) {                                       // terminates: a failed swap means another lane lowered a label of this word
        const uint32_t old = (cur >> sh) & 0xffffu;
        if (old <= v) return old;
        const unsigned prev = atomicCAS(w, cur, (cur & ~(0xffffu << sh)) | (v << sh));
        if (prev == cur) return old;
        cur = prev;
    }
}

template <class Lab> __device__ __forceinline__ uint32_t cc_find(const Lab *L, uint32_t p)
{
    uint32_t q;
    while ((q = lab_load(L, p)) != p) p = q;             // terminates: parents strictly decrease
    return p;
}

template <class Lab> __device__ __forceinline__ void cc_union(Lab *L, uint32_t a, uint32_t b)
{
    while (true) {                                       // terminates: parents strictly decrease, so does max(a, b) every round
        a = cc_find(L, a);
        b = cc_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = lab_min(L, a, b);
        if (old == a) return;                            // a was still a root: it is b's child now
        a = old;                                         // another lane gave a a parent first: that parent's tree and b remain
    }
}

// The foreground of a pixel: a bit in LDS, or `out` itself.
struct FgBits {
    const mc_mask_t *w;
    __device__ __forceinline__ bool operator()(uint32_t p) const { return (w[p >> 6] >> (p & 63u)) & 1ull; }
};
struct FgInts {
    const int32_t *o;
    __device__ __forceinline__ bool operator()(uint32_t p) const { return o[p] == 1; }
};

// Run pieces inside a wave's 64 consecutive pixels.  `in`: the lane's pixel belongs to the class being labelled (false beyond the map).
// A piece starts at lane 0, at x == 0 and after a pixel outside the class.  Every lane calls these (ballots).
__device__ __forceinline__ int piece_start(bool in, uint32_t x, int lane)
{
    const mc_mask_t m = __ballot(in);
    const mc_mask_t b = __ballot(in && (lane == 0 || x == 0 || !((m >> (lane - 1)) & 1ull)));
    return 63 - __clzll((long long)(b & (~0ull >> (63 - lane))));       // meaningful on the lanes with `in`
}
__device__ __forceinline__ int piece_len(bool in, uint32_t x, int start)           // of the piece that starts at lane `start`
{
    const mc_mask_t ends = __ballot(!in || x == 0);
    const mc_mask_t after = start >= 63 ? 0ull : ends & (~0ull << (start + 1));
    return (after ? __ffsll((long long)after) - 1 : 64) - start;
}
// the root of the lane's piece: one find, by the lane the piece starts at
template <class Lab> __device__ __forceinline__ uint32_t piece_root(const Lab *L, uint32_t p, bool in, int start, int lane)
{
    uint32_t r = 0;
    if (in && start == lane) r = cc_find(L, p);
    return __shfl(r, in ? start : lane);
}

template <class Lab> __device__ __forceinline__ void cc_init(Lab *L, uint32_t p, uint32_t x, int lane, bool in)
{
    const int s = piece_start(in, x, lane);
    if (in) L[p] = (Lab)(p - (uint32_t)(lane - s));
}

// The unions of one pixel of the class (hole: the non-foreground, 4-connected; else the foreground, 8-connected).  A join that the left
// neighbour makes as well - it is in the class and so is the pixel above it - is left to that neighbour.
template <class Lab, class Fg>
__device__ __forceinline__ void cc_merge(Lab *L, const Fg &fg, bool hole, uint32_t p, uint32_t x, uint32_t y, uint32_t H, uint32_t W, int lane,
                                         uint32_t border_root)
{
    const bool left = x > 0 && fg(p - 1) != hole;
    if (left && lane == 0) cc_union(L, p, p - 1);        // the pieces stop at the wave's first lane
    if (y > 0) {
        const bool up = fg(p - W) != hole;
        const bool ul = x > 0 && fg(p - W - 1) != hole;
        if (up) {
            if (!(left && ul)) cc_union(L, p, p - W);
        } else if (!hole) {
            if (ul && !left) cc_union(L, p, p - W - 1);
            if (x + 1 < W && fg(p - W + 1)) cc_union(L, p, p - W + 1);
        }
    }
    if (hole && (x == 0 || y == 0 || x + 1 == W || y + 1 == H)) cc_union(L, p, border_root);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    return v;
}
// A lane's walk over its wave's chunks - 64 consecutive pixels, 64-aligned, `step` pixels apart: x and y follow without a division per pixel.
struct McWalk {
    uint32_t base, p, x, y, step, dx, dy, W;
    __device__ __forceinline__ McWalk(uint32_t first, uint32_t step_, uint32_t W_, int lane)
        : base(first), p(first + (uint32_t)lane), x(p % W_), y(p / W_), step(step_), dx(step_ % W_), dy(step_ / W_), W(W_) {}
    __device__ __forceinline__ void next()
    {
        base += step; p += step; x += dx; y += dy;
        if (x >= W) { x -= W; ++y; }                     // x + dx < 2 W
    }
};

// largest area first, then the smallest label
__device__ __forceinline__ unsigned long long area_key(uint32_t area, uint32_t label) { return ((unsigned long long)area << 32) | (MC_NONE - label); }
__device__ __forceinline__ bool area_kept(uint32_t area, uint32_t a_max, int frac_q16)
{
    return (long long)area * 65536 >= (long long)frac_q16 * (long long)a_max;
}

// ------------------------------------------------------------------------------------------------------------------ LDS route
// grid n_maps x 1024.  Dynamic LDS: fg bits | keep bits (ceil(HW / 64) words each) | 16 scalars | CW area counters | u16 labels.
__global__ __launch_bounds__(MC_LDS_THREADS) void mask_clean_lds_kernel(const int32_t *__restrict__ mask, int Hi, int Wi, int mode, int frac_q16,
                                                                        int fill, uint32_t CW, int32_t *__restrict__ out,
                                                                        int32_t *__restrict__ labels, int32_t *__restrict__ stats)
{
    extern __shared__ mc_mask_t mc_lds[];
    const uint32_t H = Hi, W = Wi, HW = H * W, NW = (HW + 63u) >> 6;
    mc_mask_t *bits = mc_lds, *keep = mc_lds + NW;
    uint32_t *scal = reinterpret_cast<uint32_t *>(keep + NW), *cnt = scal + MC_SCALARS;
    uint16_t *L = reinterpret_cast<uint16_t *>(cnt + CW);
    const FgBits fg{bits};
    mask += (size_t)blockIdx.x * HW;
    out += (size_t)blockIdx.x * HW;
    if (labels) labels += (size_t)blockIdx.x * HW;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63;
    const uint32_t first = (tid >> 6) * 64u, step = nthr;                // a wave's chunks: 64 consecutive pixels, 64-aligned

    for (uint32_t base = first; base < HW; base += step) {
        const uint32_t p = base + lane;
        const mc_mask_t m = __ballot(p < HW && mask[p] == 1);
        if (lane == 0) { bits[base >> 6] = m; keep[base >> 6] = 0ull; }
    }
    if (tid < MC_SCALARS) scal[tid] = 0u;
    __syncthreads();

    if (fill) {                                                          // step 1: the 4-connected components of the non-foreground
        for (McWalk w(first, step, W, lane); w.base < HW; w.next()) {
            const uint32_t p = w.p, x = w.x, y = w.y;
            const bool in = p < HW && !fg(p);
            cc_init(L, p, x, lane, in);
            if (in && (x == 0 || y == 0 || x + 1 == W || y + 1 == H)) atomicMax(&scal[S_BORDER], MC_NONE - p);
        }
        __syncthreads();
        const uint32_t border = MC_NONE - scal[S_BORDER];                // the first background pixel of the border (unused without one)
        for (McWalk w(first, step, W, lane); w.base < HW; w.next())
            if (w.p < HW && !fg(w.p)) cc_merge(L, fg, true, w.p, w.x, w.y, H, W, lane, border);
        __syncthreads();
        const uint32_t outside = scal[S_BORDER] ? cc_find(L, border) : MC_NONE;
        uint32_t filled = 0;
        for (McWalk w(first, step, W, lane); w.base < HW; w.next()) {
            const uint32_t p = w.p;
            const bool in = p < HW && !fg(p);
            const int s = piece_start(in, w.x, lane);
            const uint32_t r = piece_root(L, p, in, s, lane);
            const mc_mask_t holes = __ballot(in && r != outside);
            if (lane == 0 && holes) { bits[w.base >> 6] |= holes; filled += __popcll(holes); }      // the word is this wave's own
        }
        if (filled) atomicAdd(&scal[S_FILLED], filled);
        __syncthreads();
    }

    for (McWalk w(first, step, W, lane); w.base < HW; w.next())        // step 2: the 8-connected components of the foreground
        cc_init(L, w.p, w.x, lane, w.p < HW && fg(w.p));
    __syncthreads();
    for (McWalk w(first, step, W, lane); w.base < HW; w.next())
        if (w.p < HW && fg(w.p)) cc_merge(L, fg, false, w.p, w.x, w.y, H, W, lane, 0u);
    __syncthreads();
    for (McWalk w(first, step, W, lane); w.base < HW; w.next()) {      // flatten
        const uint32_t p = w.p;
        const bool in = p < HW && fg(p);
        const int s = piece_start(in, w.x, lane);
        const uint32_t r = piece_root(L, p, in, s, lane);
        if (in) L[p] = (uint16_t)r;
    }
    __syncthreads();

    // areas, a window of CW labels at a time: components, the pixel total and (largest area, smallest label)
    const auto count_window = [&](uint32_t w0) {                       // cnt[l - w0] = the area of every root l in [w0, w0 + CW)
        for (uint32_t i = tid; i < CW; i += nthr) cnt[i] = 0u;
        __syncthreads();
        for (McWalk w(first, step, W, lane); w.base < HW; w.next()) {
            const uint32_t p = w.p, x = w.x;
            const bool in = p < HW && fg(p);
            const int s = piece_start(in, x, lane);
            const int len = piece_len(in, x, s);
            if (in && s == lane) {
                const uint32_t r = L[p];
                if (r - w0 < CW) atomicAdd(&cnt[r - w0], (uint32_t)len);
            }
        }
        __syncthreads();
    };
    uint32_t nc = 0, tot = 0;
    unsigned long long key = 0ull;
    for (uint32_t w0 = 0; w0 < HW; w0 += CW) {
        count_window(w0);
        for (uint32_t i = tid; i < CW; i += nthr) {
            const uint32_t p = w0 + i;
            if (p < HW && fg(p) && L[p] == p) {
                const uint32_t a = cnt[i];
                const unsigned long long k = area_key(a, p);
                ++nc; tot += a; key = k > key ? k : key;
            }
        }
        __syncthreads();
    }
    nc = wave_sum(nc); tot = wave_sum(tot); key = wave_max(key);
    if (lane == 0 && nc) {
        atomicAdd(&scal[S_NCOMP], nc);
        atomicAdd(&scal[S_TOTAL], tot);
        atomicMax(reinterpret_cast<unsigned long long *>(&scal[S_KEY]), key);
    }
    __syncthreads();
    const uint32_t ncomp = scal[S_NCOMP], total = scal[S_TOTAL];
    key = *reinterpret_cast<const unsigned long long *>(&scal[S_KEY]);
    const uint32_t a_max = (uint32_t)(key >> 32), best = MC_NONE - (uint32_t)key;

    uint32_t keptc = mode == 0 ? ncomp : (ncomp ? 1u : 0u), keptp = mode == 0 ? total : a_max;
    if (mode == 2) {                                                     // the areas again, now that a_max is known: the keep bits
        uint32_t kc = 0, kp = 0;
        for (uint32_t w0 = 0; w0 < HW; w0 += CW) {
            count_window(w0);
            for (uint32_t i = tid; i < CW; i += nthr) {                  // a root's counter becomes its decision; every other one is unread
                const uint32_t p = w0 + i;
                if (p < HW && fg(p) && L[p] == p) {
                    const uint32_t a = cnt[i];
                    const bool k = area_kept(a, a_max, frac_q16);
                    cnt[i] = k ? 1u : 0u;
                    if (k) { ++kc; kp += a; }
                }
            }
            __syncthreads();
            for (uint32_t base = first; base < HW; base += step) {
                const uint32_t p = base + lane;
                bool k = false;
                if (p < HW && fg(p)) {
                    const uint32_t r = L[p];
                    k = r - w0 < CW && cnt[r - w0] != 0u;
                }
                const mc_mask_t km = __ballot(k);
                if (lane == 0 && km) keep[base >> 6] |= km;
            }
            __syncthreads();
        }
        kc = wave_sum(kc); kp = wave_sum(kp);
        if (lane == 0 && kc) { atomicAdd(&scal[S_KEPTC], kc); atomicAdd(&scal[S_KEPTP], kp); }
        __syncthreads();
        keptc = scal[S_KEPTC]; keptp = scal[S_KEPTP];
    }

    for (uint32_t p = tid; p < HW; p += nthr) {
        const bool f = fg(p);
        const uint32_t l = L[p];
        const bool k = f && (mode == 0 || (mode == 1 ? l == best : (bool)((keep[p >> 6] >> (p & 63u)) & 1ull)));
        out[p] = k ? 1 : 0;
        if (labels) labels[p] = f ? (int32_t)l : -1;
    }
    if (stats && tid < MC_STATS) {
        const uint32_t v[MC_STATS] = {ncomp, a_max, keptc, keptp, total - keptp, scal[S_FILLED]};
        stats[(size_t)blockIdx.x * MC_STATS + tid] = (int32_t)v[tid];
    }
}

// ------------------------------------------------------------------------------------------------------------------ global route
// grid (blocks, n_maps) x 256; a wave's chunks are 64 consecutive pixels, 64-aligned, dealt round-robin over the map's waves.  Per map in
// the workspace: LH, LF (hole and foreground parents), area [HW] uint32 and 16 scalars (zeroed by the host's memset before the first launch).
struct McMap {
    uint32_t H, W, HW, first, step;
    int lane;
    size_t off;                                                          // the map's first pixel
    __device__ __forceinline__ McMap(int Hi, int Wi)
        : H(Hi), W(Wi), HW(H * W), first((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64u), step(gridDim.x * blockDim.x),
          lane(threadIdx.x & 63), off((size_t)blockIdx.y * HW) {}
};

// out = (mask == 1), area = 0, and the first init: the hole pass's (with the border's first background pixel) or the foreground's
__global__ __launch_bounds__(MC_THREADS) void mask_clean_load_kernel(const int32_t *__restrict__ mask, int Hi, int Wi, int fill,
                                                                     int32_t *__restrict__ out, uint32_t *__restrict__ LH,
                                                                     uint32_t *__restrict__ LF, uint32_t *__restrict__ area,
                                                                     uint32_t *__restrict__ scal)
{
    const McMap m(Hi, Wi);
    mask += m.off; out += m.off; area += m.off;
    uint32_t *L = (fill ? LH : LF) + m.off;
    scal += (size_t)blockIdx.y * MC_SCALARS;
    for (McWalk w(m.first, m.step, m.W, m.lane); w.base < m.HW; w.next()) {
        const uint32_t p = w.p, x = w.x, y = w.y;
        const bool valid = p < m.HW, f = valid && mask[p] == 1;
        if (valid) { out[p] = f ? 1 : 0; area[p] = 0u; }
        const bool in = valid && (f != (bool)fill);
        cc_init(L, p, x, m.lane, in);
        if (fill && in && (x == 0 || y == 0 || x + 1 == m.W || y + 1 == m.H)) atomicMax(&scal[S_BORDER], MC_NONE - p);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mask_clean_merge_kernel(const int32_t *__restrict__ out, int Hi, int Wi, int hole,
                                                                      uint32_t *__restrict__ L, const uint32_t *__restrict__ scal)
{
    const McMap m(Hi, Wi);
    const FgInts fg{out + m.off};
    L += m.off;
    const uint32_t border = MC_NONE - scal[(size_t)blockIdx.y * MC_SCALARS + S_BORDER];
    for (McWalk w(m.first, m.step, m.W, m.lane); w.base < m.HW; w.next())
        if (w.p < m.HW && fg(w.p) != (bool)hole) cc_merge(L, fg, (bool)hole, w.p, w.x, w.y, m.H, m.W, m.lane, border);
}

// the enclosed background becomes foreground (out = 1), and the foreground's init on the result
__global__ __launch_bounds__(MC_THREADS) void mask_clean_fill_kernel(int32_t *__restrict__ out, int Hi, int Wi, const uint32_t *__restrict__ LH,
                                                                     uint32_t *__restrict__ LF, uint32_t *__restrict__ scal)
{
    const McMap m(Hi, Wi);
    out += m.off; LH += m.off; LF += m.off;
    scal += (size_t)blockIdx.y * MC_SCALARS;
    const uint32_t outside = scal[S_BORDER] ? cc_find(LH, MC_NONE - scal[S_BORDER]) : MC_NONE;
    for (McWalk w(m.first, m.step, m.W, m.lane); w.base < m.HW; w.next()) {
        const uint32_t p = w.p, x = w.x;
        const bool valid = p < m.HW, f = valid && out[p] == 1, in = valid && !f;
        const int s = piece_start(in, x, m.lane);
        const uint32_t r = piece_root(LH, p, in, s, m.lane);
        const bool hole = in && r != outside;
        const mc_mask_t holes = __ballot(hole);
        if (hole) out[p] = 1;                                            // nothing in this launch reads another pixel's `out`
        if (m.lane == 0 && holes) atomicAdd(&scal[S_FILLED], (uint32_t)__popcll(holes));
        cc_init(LF, p, x, m.lane, f || hole);
    }
}

// flatten, and the areas: one atomicAdd per run piece
__global__ __launch_bounds__(MC_THREADS) void mask_clean_count_kernel(const int32_t *__restrict__ out, int Hi, int Wi, uint32_t *__restrict__ LF,
                                                                      uint32_t *__restrict__ area)
{
    const McMap m(Hi, Wi);
    out += m.off; LF += m.off; area += m.off;
    for (McWalk w(m.first, m.step, m.W, m.lane); w.base < m.HW; w.next()) {
        const uint32_t p = w.p, x = w.x;
        const bool in = p < m.HW && out[p] == 1;
        const int s = piece_start(in, x, m.lane);
        const int len = piece_len(in, x, s);
        const uint32_t r = piece_root(LF, p, in, s, m.lane);
        if (in) LF[p] = r;
        if (in && s == m.lane) atomicAdd(&area[r], (uint32_t)len);
    }
}

// components, the pixel total and (largest area, smallest label) over the roots
__global__ __launch_bounds__(MC_THREADS) void mask_clean_fold_kernel(const int32_t *__restrict__ out, int Hi, int Wi, const uint32_t *__restrict__ LF,
                                                                     const uint32_t *__restrict__ area, uint32_t *__restrict__ scal)
{
    const McMap m(Hi, Wi);
    out += m.off; LF += m.off; area += m.off;
    scal += (size_t)blockIdx.y * MC_SCALARS;
    for (uint32_t base = m.first; base < m.HW; base += m.step) {
        const uint32_t p = base + m.lane;
        const bool root = p < m.HW && out[p] == 1 && LF[p] == p;
        const uint32_t a = root ? area[p] : 0u;
        const uint32_t nc = (uint32_t)__popcll(__ballot(root)), tot = wave_sum(a);
        const unsigned long long key = wave_max(root ? area_key(a, p) : 0ull);
        if (m.lane == 0 && nc) {
            atomicAdd(&scal[S_NCOMP], nc);
            atomicAdd(&scal[S_TOTAL], tot);
            atomicMax(reinterpret_cast<unsigned long long *>(&scal[S_KEY]), key);
        }
    }
}

// selection and the write of out and labels; the kept components and pixels are counted over the roots
__global__ __launch_bounds__(MC_THREADS) void mask_clean_write_kernel(int32_t *__restrict__ out, int Hi, int Wi, int mode, int frac_q16,
                                                                      const uint32_t *__restrict__ LF, const uint32_t *__restrict__ area,
                                                                      uint32_t *__restrict__ scal, int32_t *__restrict__ labels)
{
    const McMap m(Hi, Wi);
    out += m.off; LF += m.off; area += m.off;
    if (labels) labels += m.off;
    scal += (size_t)blockIdx.y * MC_SCALARS;
    const unsigned long long key = *reinterpret_cast<const unsigned long long *>(&scal[S_KEY]);
    const uint32_t a_max = (uint32_t)(key >> 32), best = MC_NONE - (uint32_t)key;
    for (uint32_t base = m.first; base < m.HW; base += m.step) {
        const uint32_t p = base + m.lane;
        const bool valid = p < m.HW, f = valid && out[p] == 1;
        const uint32_t l = f ? LF[p] : 0u;
        const bool k = f && (mode == 0 || (mode == 1 ? l == best : area_kept(area[l], a_max, frac_q16)));
        if (valid) {
            out[p] = k ? 1 : 0;                                          // a lane reads and writes its own pixel only
            if (labels) labels[p] = f ? (int32_t)l : -1;
        }
        const bool root = k && l == p;
        const uint32_t kc = (uint32_t)__popcll(__ballot(root)), kp = wave_sum(root ? area[p] : 0u);
        if (m.lane == 0 && kc) { atomicAdd(&scal[S_KEPTC], kc); atomicAdd(&scal[S_KEPTP], kp); }
    }
}

__global__ __launch_bounds__(64) void mask_clean_stats_kernel(const uint32_t *__restrict__ scal, int n_maps, int32_t *__restrict__ stats)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n_maps) return;
    const uint32_t *s = scal + (size_t)b * MC_SCALARS;
    const uint32_t a_max = (uint32_t)(*reinterpret_cast<const unsigned long long *>(&s[S_KEY]) >> 32);
    const uint32_t v[MC_STATS] = {s[S_NCOMP], a_max, s[S_KEPTC], s[S_KEPTP], s[S_TOTAL] - s[S_KEPTP], s[S_FILLED]};
    for (int i = 0; i < MC_STATS; ++i) stats[(size_t)b * MC_STATS + i] = (int32_t)v[i];
}

static bool mask_clean_on_lds(int H, int W, int route) { return route == 1 || (route == 0 && (long long)H * W <= MC_LDS_PIXELS); }

// The LDS route reads none of the workspace: its one block of scalars is there so that every route takes a real buffer.
static size_t mask_clean_carve(void *workspace, int n_maps, int H, int W, int route, uint32_t *&scal, uint32_t *&LH, uint32_t *&LF, uint32_t *&area)
{
    const size_t px = mask_clean_on_lds(H, W, route) ? 0 : (size_t)n_maps * H * W;
    Carver carve(workspace);
    carve(scal, (size_t)(n_maps > 0 ? n_maps : 1) * MC_SCALARS);                      // never empty: n_maps == 0 still names a size
    carve(LH, px);
    carve(LF, px);
    carve(area, px);
    return carve.off;
}

// dynamic LDS of the LDS route for HW pixels, and the width CW of its area window
static int mask_clean_lds_bytes(uint32_t HW, uint32_t &CW)
{
    const uint32_t fixed = 2u * ((HW + 63u) >> 6) * 8u + MC_SCALARS * 4u, lab = 2u * ((HW + 1u) & ~1u);
    const uint32_t room = ((uint32_t)MC_LDS_BYTES - fixed - lab) / 4u;
    CW = HW < room ? HW : room;
    return (int)(fixed + 4u * CW + lab);
}
static_assert(2u * (MC_LDS_PIXELS / 64u) * 8u + MC_SCALARS * 4u + 2u * MC_LDS_PIXELS + 4u * 1024u <= (uint32_t)MC_LDS_BYTES, "an area window of >= 1024 labels");

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_mask_clean_workspace_bytes(int n_maps, int H, int W, int route)
{
    if (!(n_maps >= 0 && n_maps <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) && route >= 0 && route <= 2)) return 0;
    if (route == 1 && (long long)H * W > MC_LDS_PIXELS) return 0;
    uint32_t *scal, *LH, *LF, *area;
    return mask_clean_carve(nullptr, n_maps, H, W, route, scal, LH, LF, area);
}

extern "C" int oryon_mask_clean(const int32_t *mask, int n_maps, int H, int W, int mode, int frac_q16, int fill_holes, int route, int32_t *out,
                                int32_t *labels, int32_t *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    ORYON_CHECK_ARG(mask && out);                                                     // labels and stats may be NULL
    ORYON_CHECK_ARG(out != mask);
    ORYON_CHECK_ARG(n_maps >= 0 && n_maps <= 65535);
    ORYON_CHECK_ARG(H >= 1 && W >= 1 && (long long)H * W < (1ll << 31));
    ORYON_CHECK_ARG(mode >= 0 && mode <= 2);
    ORYON_CHECK_ARG(frac_q16 >= 0 && frac_q16 <= 65536);
    ORYON_CHECK_ARG(route >= 0 && route <= 2);
    ORYON_CHECK_ARG(route != 1 || (long long)H * W <= ORYON_MASK_CLEAN_LDS_PIXELS);
    ORYON_CHECK_ARG(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0);
    uint32_t *scal, *LH, *LF, *area;
    const size_t need = mask_clean_carve(workspace, n_maps, H, W, route, scal, LH, LF, area);
    ORYON_CHECK_ARG(workspace_bytes >= need);
    if (n_maps == 0) return ORYON_OK;
    hipStream_t st = as_stream(stream);
    const int fill = fill_holes ? 1 : 0;
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    if (mask_clean_on_lds(H, W, route)) {
        uint32_t CW;
        const int lds = mask_clean_lds_bytes(HW, CW);
        allow_dynamic_lds(reinterpret_cast<const void *>(mask_clean_lds_kernel), MC_LDS_BYTES);
        hipLaunchKernelGGL(mask_clean_lds_kernel, dim3(n_maps), dim3(MC_LDS_THREADS), lds, st, mask, H, W, mode, frac_q16, fill, CW, out, labels,
                           stats);
        ORYON_CHECK_LAUNCH();
        return ORYON_OK;
    }
    const uint32_t want = (HW + MC_THREADS - 1) / MC_THREADS;
    const dim3 grid(want < (uint32_t)MC_MAX_BLOCKS ? want : MC_MAX_BLOCKS, n_maps), block(MC_THREADS);
    ORYON_CHECK_HIP(hipMemsetAsync(scal, 0, (size_t)n_maps * MC_SCALARS * sizeof(uint32_t), st));
    hipLaunchKernelGGL(mask_clean_load_kernel, grid, block, 0, st, mask, H, W, fill, out, LH, LF, area, scal);
    if (fill) {
        hipLaunchKernelGGL(mask_clean_merge_kernel, grid, block, 0, st, out, H, W, 1, LH, scal);
        hipLaunchKernelGGL(mask_clean_fill_kernel, grid, block, 0, st, out, H, W, LH, LF, scal);
    }
    hipLaunchKernelGGL(mask_clean_merge_kernel, grid, block, 0, st, out, H, W, 0, LF, scal);
    hipLaunchKernelGGL(mask_clean_count_kernel, grid, block, 0, st, out, H, W, LF, area);
    hipLaunchKernelGGL(mask_clean_fold_kernel, grid, block, 0, st, out, H, W, LF, area, scal);
    hipLaunchKernelGGL(mask_clean_write_kernel, grid, block, 0, st, out, H, W, mode, frac_q16, LF, area, scal, labels);
    if (stats) hipLaunchKernelGGL(mask_clean_stats_kernel, dim3(ceil_div(n_maps, 64)), dim3(64), 0, st, scal, n_maps, stats);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
