// Device building blocks of the fp16x3 PointDSC encoder kernels (pdsc_encoder.hip): one definition each of what pdsc_mlp3_x3_kernel,
// pdsc_pcn_qkv_x3_kernel, pdsc_att_chain_x3_kernel and pdsc_attention_x3_img8_kernel share.  Everything is inlined into its kernel;
// the order of the products (hi*hi, hi*lo, lo*hi, accumulators alternating), the sched_barriers and the layouts are part of each block.
// The hi / lo split, the vector types and crow() are the fp16x3 family's: x3.h.
#pragma once
#include "common.h"
#include "pdsc.h"
#include "x3.h"

namespace oryon {

// the attention kernels' tile: 128 queries per workgroup, key tiles of 64
constexpr int ATT_Q = 128, ATT_KT = 64;

// ---- LDS-DMA: PIECES pieces of 1 KB, global -> LDS, PER_WAVE per wave, lane-linear.  `wave_u` is the wave's index among the WAVES that
// copy (wave-uniform: readfirstlane).  The caller waits (vmcnt) and synchronises.
template <int PIECES, int WAVES, int PER_WAVE = PIECES / WAVES>
__device__ __forceinline__ void dma_pieces(const char *src, char *lds, int wave_u, int lane)
{
    static_assert(PER_WAVE * WAVES >= PIECES, "pieces per wave");
#pragma unroll
    for (int j = 0; j < PER_WAVE; ++j) {
        const int piece = wave_u * PER_WAVE + j;
        if (PER_WAVE * WAVES == PIECES || piece < PIECES)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + piece * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) void *)(lds + piece * 1024), 16, 0, 0);
    }
}
// the 80 KB fc_message weight image (PDSC_MLP_*), 80 / WAVES pieces per wave
template <int WAVES>
__device__ __forceinline__ void dma_mlp_image(const char *img, char *lds, int wave_u, int lane)
{
    dma_pieces<PDSC_MLP_IMG_BYTES / 1024, WAVES>(img, lds, wave_u, lane);
}
// chunk `chunk` (PointCN | q | k | v | PointCN') of a layer's PointCN + q|k|v image into a 64 KB weight area, 64 / WAVES pieces per wave.
// The "idle waves only" form of pdsc_att_chain_x3_kernel is WAVES = 4 with wave_u counted among the key-half-1 waves.
template <int WAVES>
__device__ __forceinline__ void dma_pq_chunk(const char *pq_img, int chunk, char *area, int wave_u, int lane)
{
    dma_pieces<PDSC_PQ_CHUNK_BYTES / 1024, WAVES>(pq_img + (size_t)chunk * PDSC_PQ_CHUNK_BYTES, area, wave_u, lane);
}
// the K / V image of the 64-key tile at key j0 into a tile buffer, by the 8 waves of the image-fed attention kernels: 64 pieces as 9 per
// wave with the last wave taking one (8 per wave would be the even split; kept as the kernels were measured)
__device__ __forceinline__ void dma_kv_tile(const char *pair_img, int j0, char *buf, int wave_u, int lane)
{
    constexpr int PIECES = PDSC_KV_TILE_BYTES / 1024;
    dma_pieces<PIECES, 8, PIECES / 8 + 1>(pair_img + (size_t)(j0 / ATT_KT) * PDSC_KV_TILE_BYTES, buf, wave_u, lane);
}

// ---- A-operand fragments of a weight matrix in LDS: lane (row l31 of block rb, half hi), k-step s_ -> 8 halves.
// 256-byte rows (128 input channels: fc_message W1, PointCN, q, k, v): slot ^ (row & 15)
struct Frag256 {
    const char *lds;
    int l31, hi;
    __device__ __forceinline__ f16x8 operator()(int base, int rb, int s_) const
    {
        const int o = rb * 32 + l31;
        return *reinterpret_cast<const f16x8 *>(lds + base + o * 256 + (((2 * s_ + hi) ^ (o & 15)) << 4));
    }
};
// 128-byte rows (64 input channels: fc_message W2, W3): slot ^ ((row >> 1) & 7)
struct Frag128 {
    const char *lds;
    int l31, hi;
    __device__ __forceinline__ f16x8 operator()(int base, int rb, int s_) const
    {
        const int o = rb * 32 + l31;
        return *reinterpret_cast<const f16x8 *>(lds + base + o * 128 + (((2 * s_ + hi) ^ ((o >> 1) & 7)) << 4));
    }
};

// Two 32-row output blocks (rb0, rb0 + 1) over NS k-steps: the four weight fragments of step s+1 are requested before the six MFMAs of
// step s (left alone the compiler reads each fragment right before its first use: one exposed LDS latency per fragment), and
// sched_barrier keeps it that way.  The two accumulators alternate, per accumulator the order is hi*hi, hi*lo, lo*hi.
// SWAP = false: the weights are the A operand (accumulator: lane = point, registers = channels); SWAP = true: the activations are
// (lane = channel, registers = points crow(r, hi)) - the same fragments either way, the 32x32x16 A and B register layouts are mirror images.
template <int NS, bool SWAP, class Frag>
__device__ __forceinline__ void two_blocks(const Frag &frag, int base_h, int base_l, int rb0, const f16x8 *bh, const f16x8 *bl, f32x16 (&acc)[2])
{
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    f16x8 w[2][2][2];                             // [buffer][block][hi | lo]
#pragma unroll
    for (int i = 0; i < 2; ++i) { w[0][i][0] = frag(base_h, rb0 + i, 0); w[0][i][1] = frag(base_l, rb0 + i, 0); }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) {
        const int cur = s_ & 1;
        if (s_ + 1 < NS) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { w[cur ^ 1][i][0] = frag(base_h, rb0 + i, s_ + 1); w[cur ^ 1][i][1] = frag(base_l, rb0 + i, s_ + 1); }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!SWAP) {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[cur][0][0], bh[s_], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[cur][1][0], bh[s_], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[cur][0][0], bl[s_], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[cur][1][0], bl[s_], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[cur][0][1], bh[s_], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[cur][1][1], bh[s_], acc[1], 0, 0, 0);
        } else {
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s_], w[cur][0][0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s_], w[cur][1][0], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[s_], w[cur][0][0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[s_], w[cur][1][0], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s_], w[cur][0][1], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s_], w[cur][1][1], acc[1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- bias sources: a float4 for lane half `hi` (channels off + 4 hi .. + 3) at a WAVE-UNIFORM offset `off` (a multiple of 8).
// Global memory: both halves come through the scalar cache (uniform address -> s_load, lgkmcnt) and the lane picks one.  Round 6: as
// vector loads (address + 16 hi) they sat on the vector-memory counter between the epilogue's stores, and the compiler's s_waitcnt
// vmcnt(0) in front of each use made every store of the per-point chain wait for the acknowledgement of the one before it - 5 to 8 us
// per 16 KB of output (the phase clocks of ORYON_PDSC_CLOCKS).
__device__ __forceinline__ float4 bias4(const float *__restrict__ b, int off, int hi)
{
    const float4 lo = *reinterpret_cast<const float4 *>(b + off), up = *reinterpret_cast<const float4 *>(b + off + 4);
    return hi ? up : lo;
}
struct BiasGlobal {
    const float *b;
    __device__ __forceinline__ float4 operator()(int off, int hi) const { return bias4(b, off, hi); }
};
// Global memory as per-lane vector loads (address + 4 hi floats): pdsc_mlp3_x3_kernel, whose chain has no store in front of its
// epilogue for the loads to queue behind - there the scalar form measured 0.3 to 1 us slower per launch (a cold scalar cache in front
// of each of its two next_operand calls)
struct BiasVector {
    const float *b;
    __device__ __forceinline__ float4 operator()(int off, int hi) const { return *reinterpret_cast<const float4 *>(b + off + 4 * hi); }
};
// LDS (pdsc_att_chain_x3_kernel): FOUR planes of 192 floats (plane e = element e of every channel quad), so that a lane's quad is four
// broadcasting ds_read_b32 - neither the vector-memory counter the chain's stores sit on nor a cold scalar cache in front of every epilogue
struct BiasLds {
    const float *planes;
    __device__ __forceinline__ float4 operator()(int off, int hi) const
    {
        const int q = (off >> 2) + hi;
        return make_float4(planes[q], planes[192 + q], planes[384 + q], planes[576 + q]);
    }
};

// bias + ReLU + hi / lo split of two 32-channel accumulator blocks -> the 4 B fragments (k-steps) of the next layer;
// the blocks' biases start at channel `off` of `bias`
template <class Bias>
__device__ __forceinline__ void next_operand(const f32x16 (&acc)[2], const Bias &bias, int off, int hi, f16x8 (&oh)[4], f16x8 (&ol)[4])
{
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            uint4 uh, ul;
            unsigned *ph = &uh.x, *pl = &ul.x;
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {                 // registers 8 j + 4 g2 .. + 3: channels rb*32 + 8 (2 j + g2) + 4 hi + 0..3
                const float4 bv = bias(off + rb * 32 + 8 * (2 * j + g2), hi);
                const int r0 = 8 * j + 4 * g2;
                const float v0 = fmaxf(acc[rb][r0] + bv.x, 0.0f), v1 = fmaxf(acc[rb][r0 + 1] + bv.y, 0.0f);
                const float v2 = fmaxf(acc[rb][r0 + 2] + bv.z, 0.0f), v3 = fmaxf(acc[rb][r0 + 3] + bv.w, 0.0f);
                split2(v0, v1, ph[2 * g2], pl[2 * g2]);
                split2(v2, v3, ph[2 * g2 + 1], pl[2 * g2 + 1]);
            }
            oh[rb * 2 + j] = __builtin_bit_cast(f16x8, uh);
            ol[rb * 2 + j] = __builtin_bit_cast(f16x8, ul);
        }
}

// The 128 floats of this lane's row as eight B-operand fragments: channels 16 s + 8 hi .. + 7 of k-step s, split into hi / lo.
// All sixteen loads are issued before the first split.
__device__ __forceinline__ void load_split_row(const float *row, int hi, f16x8 (&xh)[8], f16x8 (&xl)[8])
{
    const float4 *xp = reinterpret_cast<const float4 *>(row);
    float4 raw[16];
#pragma unroll
    for (int s_ = 0; s_ < 8; ++s_) { raw[2 * s_] = xp[4 * s_ + 2 * hi]; raw[2 * s_ + 1] = xp[4 * s_ + 2 * hi + 1]; }
#pragma unroll
    for (int s_ = 0; s_ < 8; ++s_) {
        uint4 uh, ul;
        split2(raw[2 * s_].x, raw[2 * s_].y, uh.x, ul.x);
        split2(raw[2 * s_].z, raw[2 * s_].w, uh.y, ul.y);
        split2(raw[2 * s_ + 1].x, raw[2 * s_ + 1].y, uh.z, ul.z);
        split2(raw[2 * s_ + 1].z, raw[2 * s_ + 1].w, uh.w, ul.w);
        xh[s_] = __builtin_bit_cast(f16x8, uh);
        xl[s_] = __builtin_bit_cast(f16x8, ul);
    }
}

// ---- the image-fed 8-wave attention (pdsc_attention_x3_img8_kernel, pdsc_att_chain_x3_kernel): wave = (query block, key half kb)
// XCD-aware block map: the query blocks of one pair read the same K / V tile images, so they go to ONE XCD (linear block id mod 8) and
// share the images through its L2 (with the plain (query block, pair) grid a pair's four blocks landed on four XCDs and each fetched
// the pair's 540 KB of images for itself).  The grid's z extent is B rounded up to a multiple of 8.
__device__ __forceinline__ void att8_block_map(int &b, int &qblk)
{
    const int lin = blockIdx.x + gridDim.x * blockIdx.z;
    b = (lin / 8 / (int)gridDim.x) * 8 + (lin & 7);
    qblk = (lin / 8) % (int)gridDim.x;
}
// the SC values of this wave's 32 keys of the tile at key j0 (sc_q: the lane's slot in its query block's first tile, pdsc_sc_kernel's
// layout); query blocks past n have no SC tiles: masked
__device__ __forceinline__ void fetch_sc(const float4 *sc_q, bool q_live, int kb, int j0, float4 (&scv)[4])
{
    const float4 *sp = sc_q + (size_t)(j0 / ATT_KT) * 8 * 64 + (size_t)kb * 4 * 64;
#pragma unroll
    for (int v4 = 0; v4 < 4; ++v4) scv[v4] = q_live ? sp[(size_t)v4 * 64] : make_float4(-1.f, -1.f, -1.f, -1.f);
}
// K fragments (hi | lo) of key `key` of a tile image for k-step s_; V fragment of (key octet, channel) of a V plane
__device__ __forceinline__ void read_k(const char *tile, int key, int s_, int hi, f16x8 (&kf)[2])
{
    kf[0] = *reinterpret_cast<const f16x8 *>(reinterpret_cast<const _Float16 *>(tile) + pdsc_k_img_elem(key, 2 * s_ + hi));
    kf[1] = *reinterpret_cast<const f16x8 *>(reinterpret_cast<const _Float16 *>(tile + PDSC_KV_KL) + pdsc_k_img_elem(key, 2 * s_ + hi));
}
__device__ __forceinline__ f16x8 read_v(const char *v_plane, int oct, int ch)
{
    return *reinterpret_cast<const f16x8 *>(reinterpret_cast<const _Float16 *>(v_plane) + ((size_t)oct * 128 + ch) * 8);
}
// ... and their writers (pdsc_pcn_qkv_x3_kernel, pdsc_att_chain_x3_kernel), already split into hi / lo:
// k from the un-swapped product (lane = key): channels cc .. cc + 3 of `key` (0..63), one 8-byte piece per plane
__device__ __forceinline__ void store_k(char *tile, float4 k, int key, int cc)
{
    uint2 uh, ul;
    split2(k.x, k.y, uh.x, ul.x);
    split2(k.z, k.w, uh.y, ul.y);
    const size_t off = (size_t)pdsc_k_img_elem(key, cc >> 3) * 2 + (cc & 7) * 2;
    *reinterpret_cast<uint2 *>(tile + off) = uh;
    *reinterpret_cast<uint2 *>(tile + PDSC_KV_KL + off) = ul;
}
// v from the swapped one (lane = channel ch, registers 8 t2 .. 8 t2 + 7 = the 8 keys of octet (kb, t2, hi)) + the channel's bias:
// one 16-byte piece per octet and plane
__device__ __forceinline__ void store_v(char *tile, const f32x16 &acc, float bv, int kb, int ch, int hi)
{
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        uint4 uh, ul;
        split2(acc[8 * t2 + 0] + bv, acc[8 * t2 + 1] + bv, uh.x, ul.x);
        split2(acc[8 * t2 + 2] + bv, acc[8 * t2 + 3] + bv, uh.y, ul.y);
        split2(acc[8 * t2 + 4] + bv, acc[8 * t2 + 5] + bv, uh.z, ul.z);
        split2(acc[8 * t2 + 6] + bv, acc[8 * t2 + 7] + bv, uh.w, ul.w);
        const int oct = (kb * 2 + t2) * 2 + hi;
        *reinterpret_cast<uint4 *>(tile + PDSC_KV_VH + ((size_t)oct * 128 + ch) * 16) = uh;
        *reinterpret_cast<uint4 *>(tile + PDSC_KV_VL + ((size_t)oct * 128 + ch) * 16) = ul;
    }
}

}  // namespace oryon
