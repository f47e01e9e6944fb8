// Shared bits of the matcher translation units (match.hip, match16.hip, match_corrs.hip, screen_mx6.hip, match_x3.hip).
#pragma once
#include <hip/hip_fp16.h>
#include "common.h"

namespace oryon {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// lexicographic (distance, index) minimum: smaller distance, then smaller index (first-index tie rule of torch.argmin)
__device__ __forceinline__ void lex_min(float &d, int &i, float od, int oi)
{
    const bool take = (od < d) || (od == d && oi < i);
    d = take ? od : d;
    i = take ? oi : i;
}

// Exact fp32 recomputation (K1) of the anchor panels flagged in panel_flag [B, cap_a/128]; only rows with row_flag set
// are written.  Used by the screened matcher when a candidate list overflows.
int match_f32_flagged(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q, const int32_t *n_a,
                      const int32_t *n_q, float threshold, float *min_dist, int32_t *argmin, uint8_t *valid,
                      const int32_t *panel_flag, const uint8_t *row_flag, void *stream);

// K1's query splits S for a call with T anchor panels per pair (match.hip; K1m sizes its split buffers by the same rule)
int match_f32_split(int B, int T);

// K1x3 (match_x3.hip): fp32-grade scan of a compacted anchor list on the fp16 matrix pipe; see the file's header
size_t match_x3_scratch_bytes(int B, int cap_s, int S, int cap_q);
size_t match_x3_zero_bytes(int B, int cap_s, int S);         // the head of that scratch the caller zeroes before match_x3_resolve
int match_x3_resolve(const float *a_c, const int32_t *n_c, int cap_s, const float *feat_q, int C_true, int HW, int layout,
                     const int32_t *roi_q, int roi_stride_q, const float *q_norm, const int32_t *n_q, int B, int cap_q, float threshold,
                     int round_f16, __half *qh, __half *ql, __half *ah, __half *al, void *scratch, float *md_c, int32_t *am_c, uint8_t *va_c,
                     int32_t **n_ovf_out, int32_t **ovf_idx_out, const int32_t *orig_idx, int orig_stride, const int32_t *sid_final, int cap_a,
                     const __half *q_hi_lo_pre, const float *q_lo_sq_max_pre, hipStream_t st);
void match_x3_scatter_ovf(int B, int cap_s, const int32_t *n_ovf, const int32_t *ovf_idx, const float *md_o, const int32_t *am_o,
                          const uint8_t *va_o, float *md_c, int32_t *am_c, uint8_t *va_c, hipStream_t st);

const char *screen_mx6_name(int C);
// screen_mx6.hip: K1s6 launch (C = 256 / 512); groups / T as sized for 256-anchor panels by the caller
void launch_screen_mx6(int C, int groups, int T, hipStream_t st, const uint8_t *a6, const uint8_t *q6, int B, int cap_a, int cap_q,
                       const int32_t *n_a, const int32_t *n_q, int S, float *ws_max, int32_t *ws_i1, float *ws_m2, int C_true,
                       int cascade = 0, const int32_t *gate = nullptr, int win = 0);
inline int mx6_panels_per_pair(int cap_a) { return (cap_a + 1023) / 1024; }     // panels of the 8-wave C_pad 256 screen (the cascade's gate is [B, that])
// the complete screen of a LIST of a pair's cap_src anchor rows, read in place (C_pad 256): list slot i is row idx[p idx_stride + i] with
// count[p] rows listed, or (idx == nullptr) row i stride with ceil(count[p] / stride) rows; at most cap_list rows, T = ceil(cap_list / 512)
// panels per pair, S query splits; triples come out as [B, S, cap_list] by list slot.  The cascades' probe (stride), open rows (cap_list
// = cap_a) and sampled rows (cap_list = MX6_SAMPLED_PANEL: the second pass of either validity cascade)
void launch_screen_mx6_list512(hipStream_t st, const uint8_t *a6, const uint8_t *q6, int B, int cap_src, int cap_list, int cap_q,
                               const int32_t *count, const int32_t *idx, int idx_stride, int stride, const int32_t *n_q, int S, float *ws_max,
                               int32_t *ws_i1, float *ws_m2, int C_true);
// band pass of the default route's cascade: the anchors in 512-row panels, panel k of pair p over the tiles [first, first + count) that
// band[(p band_T + k) 2 ..] names, dealt evenly to S four-wave workgroups; triples come out as [B, S, cap_a]
void launch_screen_mx6_band512(hipStream_t st, const uint8_t *a6, const uint8_t *q6, int B, int cap_a, int cap_q, const int32_t *n_a,
                               const int32_t *n_q, int S, float *ws_max, int32_t *ws_i1, float *ws_m2, int C_true, const int32_t *band, int band_T);
constexpr int MX6_SAMPLED_PANEL = 512;        // rows of that panel (>= the sampled rows of a pair: corr_rows <= 512 on this route)
inline int mx6_sampled_splits(int B) { int s = (512 + B - 1) / B; return s < 1 ? 1 : s > 16 ? 16 : s; }      // ~512 four-wave workgroups

// ------------------------------------------------------------------------------------------------ workspaces of the screened matchers
// (carved with common.h's Carver; the carve_* functions return the size)
constexpr int MT16 = 256;               // anchors per workgroup of the screens (4 waves x 2 blocks of 32)

// K1s (oryon_match_screened).  [zero_off, zero_off + zero_bytes) of the allocation is zeroed at the start of every call
struct ScreenWs {
    float *ws_max, *ws_m2, *m_final, *amb_max;
    int32_t *ws_i1, *cnt, *cand, *panel_flag, *n_amb, *amb_idx;
    __half *a16c;
    uint8_t *row_flag;
    size_t zero_off, zero_bytes;
};
// K1s8: + the fp16 fall-back's operands and outputs for the undecided anchors, and the workspace of its nested K1s call
struct Screen8Ws : ScreenWs {
    __half *q16;
    float *a_hat_c, *md_c;
    int32_t *am_c;
    uint8_t *va_c;
    void *nested;
    size_t nested_bytes;
};
// K1s8 on K0v3 operands: + the fp32 query rows (and the scratch of the gather that makes them) of the pairs that need a fall-back
struct Screen8RawWs : Screen8Ws {
    float *q_hat, *scale_scratch, *eps_scratch;
    int8_t *q8_scratch;
    int32_t *need_f32;
};
int pick_split16(int B, int T);         // query splits S of a call with T anchor panels per pair
size_t carve_screen8_raw(void *base, Screen8RawWs &w, int B, int C, int cap_a, int cap_q, int S);

// gather8.hip: K0v3 on the maps map_enable flags (device-gated)
int gather_q8_launch(const float *feat, int n_maps, int C, int HW, int layout, const int32_t *roi, int roi_stride, const int32_t *count,
                     const int32_t *map_enable, int rows_cap, int C_pad, int8_t *out8, float *scale, float *eps, float *norm,
                     float *out32, int lanes_per_row, int round_f16, hipStream_t st, int fmt = 0, void *aux = nullptr);
// gather8.hip: oryon_gather_mx6 without its fill of err_max - for a caller whose stream has already cleared those n_maps words
int gather_mx6_prezeroed(const float *feat, int n_maps, int C, int HW, int layout, const int32_t *roi, int roi_stride, const int32_t *count,
                         int rows_cap, int C_pad, uint8_t *out_mx6, float *err_max, float *row_norm, float *out_f32, int round_f16,
                         hipStream_t st);
// roi.hip: oryon_roi_compact on the anchor and the query masks of a step in ONE launch (grid 2 n_maps); the workgroup of map m also stores
// 0 to zero_a[m] / zero_q[m] (either may be NULL): the err_max words of the gathers that follow on the same stream
int roi_compact_pair_launch(const int32_t *mask_a, const int32_t *mask_q, int n_maps, int HW, int32_t *roi_a, int32_t *roi_q,
                            int32_t *n_a, int32_t *n_q, float *zero_a, float *zero_q, hipStream_t st);
// The sampled slots whose anchor row is in state `want` (ambiguous-valid: argmin still unknown) -> work list of the second level
// (K1x3 / exact scan), built by the one workgroup of pair p that holds the data: the sampler right after it wrote sel_rows, the sampled
// rows' decide pass right after it wrote their states.  state == nullptr: no list.
// The list comes out in ASCENDING anchor-row order, i.e. in image order: neighbouring anchors share a wave of match_x3_scan_kernel,
// their matches are neighbours in the query map, and the scan can skip the query tiles none of a wave's anchors can match (it is also
// deterministic).  A row drawn several times (sampling with replacement) is marked - and listed - once.
struct SampledAmbList {
    const uint8_t *state = nullptr;     // [B, cap_a]
    uint8_t want = 0;
    int32_t *mark = nullptr;            // [B, cap_a], zero where no earlier list of this call marked the row
    int32_t *n_list = nullptr;          // [B]
    int32_t *list = nullptr;            // [B, corr_rows]
};
// Called by ALL threads of the workgroup (blockDim.x a multiple of 64, at most 1024; s_wave holds blockDim.x / 64 words).  What the
// workgroup itself wrote before the call (sel_rows, state, mark) is read behind a barrier.
__device__ __forceinline__ void list_sampled_amb(const SampledAmbList &L, int p, int cap_a, int n, const int32_t *sel_rows, int corr_rows,
                                                 int *s_wave)
{
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6;
    const uint8_t *st = L.state + (size_t)p * cap_a;
    int32_t *mk = L.mark + (size_t)p * cap_a;
    __threadfence_block();
    __syncthreads();
    for (int s = t; s < n; s += nt) {
        const int a = sel_rows[(size_t)p * corr_rows + s];
        if (st[a] == L.want) mk[a] = 1;
    }
    __threadfence_block();
    __syncthreads();
    // ordered compaction in ONE scan: thread t owns the consecutive rows [t R, (t + 1) R), R a multiple of four (its mark words are
    // 16-byte loads), counts its marks, the block scans the counts
    const int R = ((cap_a + nt - 1) / nt + 3) / 4 * 4;
    const bool vec = cap_a % 4 == 0 && (reinterpret_cast<uintptr_t>(mk) & 15) == 0;
    auto marks4 = [&](int a) -> unsigned {          // bit e: row a + e is marked
        if (vec && a + 4 <= cap_a) {
            const int4 v = *reinterpret_cast<const int4 *>(mk + a);
            return (v.x != 0 ? 1u : 0u) | (v.y != 0 ? 2u : 0u) | (v.z != 0 ? 4u : 0u) | (v.w != 0 ? 8u : 0u);
        }
        unsigned b = 0u;
        for (int e = 0; e < 4; ++e) b |= (a + e < cap_a && mk[a + e] != 0 ? 1u : 0u) << e;
        return b;
    };
    int mine = 0;
    for (int i = 0; i < R; i += 4) mine += __popc(marks4(t * R + i));
    int incl = mine;                                            // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int off0 = incl - mine;
    for (int w = 0; w < wave; ++w) off0 += s_wave[w];
    if (mine)
        for (int i = 0; i < R; i += 4) {
            const unsigned b = marks4(t * R + i);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (b & (1u << e)) L.list[(size_t)p * corr_rows + off0++] = t * R + i + e;
        }
    if (t == nt - 1) L.n_list[p] = off0;
}

// post.hip: the sampler; sel_rows / pair_eager as the lazy matcher uses them; amb (lazy route only): the sampler's workgroups also build
// the list of list_sampled_amb from the rows they just drew
int select_corrs_launch(const int32_t *roi_a, const int32_t *roi_q, int roi_stride_a, int roi_stride_q, const int32_t *n_a,
                        const int32_t *n_q, const int32_t *argmin, const uint8_t *valid, int cap_a, int B, int W, int max_corrs,
                        int corr_rows, uint64_t seed, const int64_t *pair_key, int32_t *scratch, int32_t *corrs, int32_t *n_valid,
                        int32_t *n_sel, int32_t *status, int32_t *sel_rows, const int32_t *pair_eager, hipStream_t st,
                        const SampledAmbList &amb = SampledAmbList());

// match_next.hip: the launches of one rank scan (oryon_match_next_f32 behind its argument checks) for oryon_topk_corrs; the query-split
// buffers are carved from workspace at ws_start, match_next_split_bytes is where they end
size_t match_next_split_bytes(int B, int cap_a, size_t start);
int match_next_launch(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q,
                      const int32_t *roi_q, int roi_stride_q, int W_q, int radius, const int32_t *prev, int n_prev, float *next_dist,
                      int32_t *next_argmin, void *workspace, size_t ws_start, hipStream_t st);

// ------------------------------------------------------------------------------------------------ host steps of K1s8 (match16.hip)
// What the steps below read: oryon_match_screened8 and oryon_match_screened8_raw fill one, MatchCorrsArgs extends it.
struct Screen8Args {
    const float *a_hat = nullptr;       // fp32 unit rows of the anchors (k-permuted)
    const int8_t *a_i8 = nullptr;
    const int8_t *q_i8 = nullptr;
    const float *a_scale = nullptr;
    const float *q_scale = nullptr;
    const float *q_eps_max = nullptr;
    int B = 0;
    int C_true = 0;
    int C = 0;
    int cap_a = 0;
    int cap_q = 0;
    const int32_t *n_q = nullptr;
    float threshold = 0.0f;
    // the query rows as K0v3 leaves them (raw map + pixel + norm of every row): rescore_raw_step and raw_fallbacks only
    const float *feat_q = nullptr;
    int HW = 0;
    int layout = 0;
    const int32_t *roi_q = nullptr;
    int roi_stride_q = 0;
    const float *q_norm = nullptr;
    int round_f16 = 0;
    // per-anchor outputs
    float *min_dist = nullptr;
    int32_t *argmin = nullptr;
    uint8_t *valid = nullptr;
    void *stream = nullptr;
};
// oryon_match_screened8, oryon_match_screened8_raw and the eager route of the lazy matcher are sequences of these.  The single-launch
// steps leave the launch check to the caller; the others check with the caller's name (who), so the error texts stay what they were.
inline int check_launch(const char *who)       // ORYON_CHECK_LAUNCH with a given name in place of __func__
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return ORYON_OK;
    set_error("%s: launch failed: %s", who, hipGetErrorString(e));
    return ORYON_ERR_HIP;
}
// the int8 screen (between the profile events): per-split (max, slice, runner-up) of every anchor
void screen8_step(const Screen8Args &m, int S, const int32_t *n_a, const ScreenWs &w);
// match_decide_kernel on those triples: candidates of the decided anchors, list of the undecided ones
void decide8_step(const Screen8Args &m, int S, const int32_t *n_a, const ScreenWs &w);
// exact re-scoring of the candidates from the raw query map, rescore_lanes lanes per anchor
void rescore_raw_step(const Screen8Args &m, const int32_t *n_a, int rescore_lanes, const Screen8RawWs &w);
// anchors the int8 stage could not decide: complete fp16 pipeline (K1s) on the compacted set against q_hat, results scattered back
// (the fp16 operands are made here, and only for pairs that have such anchors: K0 does not write fp16 rows for this path)
int screen16_fallback(const Screen8Args &m, const float *q_hat, const Screen8Ws &w, const char *who);
// both fall-backs of the raw route on fp32 query rows materialised for the pairs that need them: overflowed candidate lists
// (exact scan), then screen16_fallback.  entry: the C entry named in the gather's error text
int raw_fallbacks(const Screen8Args &m, const int32_t *n_a, const Screen8RawWs &w, const char *who, const char *entry);

// ------------------------------------------------------------------------------------------------ the lazy matcher (match_corrs.hip)
// What the six oryon_match_corrs_* entries and the engine fill; pointers left null are operands the route does not have.
// Of Screen8Args: a_i8 / q_i8 hold mx6 slots when fmt == 1; a_scale is per 16-row slice (fmt 0) or the largest anchor-row error norm
// per pair (fmt 1); q_scale is fmt 0 only; q_eps_max per pair (fmt 1: the largest query-row error norm); a_hat may be null when
// feat_a + a_norm are given (rows formed on demand, lazy route only).
struct MatchCorrsArgs : Screen8Args {
    const float *feat_a = nullptr;      // raw anchor map and K0's anchor norms, in place of a_hat
    const float *a_norm = nullptr;
    const int32_t *roi_a = nullptr;     // pixel of every anchor row
    int roi_stride_a = 0;
    const void *q_hi_lo = nullptr;      // K0's hi / lo half query rows for the fp16x3 second level (C == 256), with q_lo_sq_max
    const float *q_lo_sq_max = nullptr;
    const int32_t *n_a = nullptr;
    // sampling
    int W = 0;
    int max_corrs = 0;
    int corr_rows = 0;
    uint64_t seed = 0;
    const int64_t *pair_key = nullptr;
    // outputs (n_undecided optional)
    int32_t *corrs = nullptr;
    int32_t *n_valid = nullptr;
    int32_t *n_sel = nullptr;
    int32_t *status = nullptr;
    int32_t *n_undecided = nullptr;
    void *workspace = nullptr;
    size_t workspace_bytes = 0;
    int fmt = 0;                        // 0: int8 rows, 1: mx6 rows (lazy route only)
    int force_eager = 0;                // complete min_dist / argmin arrays from whole fp32 rows (needs a_hat)
    int cascade = 1;                    // default route, fmt 1, C 256: 1 = anchor-granular validity cascade where the shape has one, 0 = plain full screen
};
int match_corrs_lazy_impl(const MatchCorrsArgs &m);
// the default-route cascade's per-pair counters [B, 4] (probe rows, settled rows, open rows, band tiles) inside a matcher workspace of
// that shape; all zero after a call that took another route
int32_t *match_dc_stats(void *workspace, int B, int C, int cap_a, int cap_q, int corr_rows);

}  // namespace oryon
