/* liboryon_hip.so — C ABI of the MI355X-native Oryon hot path (gfx950 only).
 *
 * The reference (jcorsetti/oryon) is pure Python/PyTorch and has no FFI; its boundary for this path is a
 * set of Python callables.  Each entry point below replaces the PyTorch expression(s) cited next to it
 * (file:line into the reference tree) and is what a ctypes binding on the reference side would load
 * (INTEGRATION.md shows that binding).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; the caller owns all buffers;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all calls are asynchronous on
 *     it, never synchronise, never allocate (except the handle constructors: oryon_pointdsc_create/_finalize,
 *     oryon_engine_create, oryon_decoder_create - the last one also waits for its packing launches once);
 *   - return value: ORYON_OK or a negative ORYON_ERR_*; nothing throws; oryon_last_error() gives text;
 *   - per-pair outcomes (no mask / no correspondences) are DATA, reported in `status` arrays with the
 *     reference's own failure semantics (pipeline.py:335-350), not error codes;
 *   - thread-safe for distinct streams.  Global state of the library, all of it per device or per thread: the last-error string
 *     (thread local); the step engine's stream pool (eight HIP streams per device, created under a mutex on first use or by
 *     oryon_engine_warm_streams, shared by every engine of the process and never destroyed); the fp16x3 range-flag word per device
 *     (oryon_x3_range_flag); the profile-event pair armed by oryon_profile_events (thread local).
 */
#ifndef ORYON_HIP_H
#define ORYON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORYON_OK 0
#define ORYON_ERR_INVALID_ARG (-1)
#define ORYON_ERR_HIP (-2)
#define ORYON_ERR_WORKSPACE (-3)
#define ORYON_ERR_NO_DEVICE (-4)
#define ORYON_ERR_STATE (-5)

/* per-pair status values (pipeline.py:316-350: invalid detection / matcher returned None / pose ok) */
#define ORYON_PAIR_OK 0
#define ORYON_PAIR_NO_MASK 1
#define ORYON_PAIR_NO_CORR 2

/* matcher tile geometry the padded capacities must respect */
#define ORYON_MATCH_TILE 128

const char *oryon_version(void);
const char *oryon_last_error(void);
/* Measurement hook used by bench.py: the two hipEvent_t handles (created by the caller) are recorded on the launch
 * stream immediately before / after the DOMINANT kernel launch of the next oryon_match_f32 / oryon_match_screened call
 * made by this thread (match_f32_regb_kernel, resp. the match_f16_screen_kernel screening pass), then forgotten. */
int oryon_profile_events(void *start_event, void *stop_event);
/* Name (template arguments included) of the kernel the events above bracketed most recently; "" before the first armed call. */
const char *oryon_dominant_kernel(void);
/* ORYON_OK iff device `device` exists and is gfx950. */
int oryon_device_check(int device);

/* K-1 batched image pre-processing in front of the network: what the reference does per sample on dataloader workers
 *     (utils/data/common.py:49 `rgb.transpose(2,0,1)/255.`, utils/augmentations.py:137-139 resize to dataset.img_size,
 *     datasets.py:204 `.to(float32)`).  Resampling = torch upsample_bilinear2d, align_corners=False.
 * rgb_hwc [n,HI,WI,3] uint8 -> out [n,3,HO,WO] fp32 (fp64 arithmetic, one rounding, like the reference's float64 tensor).
 * in [n,HI,WI] fp32 -> out [n,HO,WO] fp32 (fp32 arithmetic; round_output != 0 rounds half-to-even as torchvision does
 * for integer images such as the depth map). */
int oryon_rgb_resize_bilinear(const uint8_t *rgb_hwc, int n, int HI, int WI, int HO, int WO, float *out, void *stream);
int oryon_resize_bilinear_f32(const float *in, int n, int HI, int WI, int HO, int WO, int round_output, float *out, void *stream);

/* K-1a the reference's training augmentations (datasets.py:98-114 build_augs; utils/augmentations.py:17-127: random_jitter,
 *     random_brightness, horizontal_flip, vertical_flip, each per sample in front of the resize) fused into the K-1 resizes.
 * table [n, ORYON_AUG_STRIDE] float64, one row per image, 8-byte aligned:
 *     [0]          flip bits as a number: ORYON_AUG_HFLIP | ORYON_AUG_VFLIP (the image is mirrored in x / in y before the resize)
 *     [1]          reserved, 0
 *     [2+2k, 3+2k] slot k < ORYON_AUG_SLOTS of the colour chain, in execution order: op id (0 brightness, 1 contrast, 2 saturation, 3 hue;
 *                  anything else, e.g. -1: empty slot) and its factor.  At most ONE contrast slot per image (two ColorJitter applications
 *                  of the reference never hold more: random_brightness has no contrast); with more, all of them use the first one's mean.
 *     Arithmetic (DESIGN.md "7b", transcribed from torchvision's tensor path; x = pixel / 255. in float64 like the reference's tensor):
 *     gray = (0.2989 r + 0.587 g) + 0.114 b;  blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1);  brightness blend(x, 0, f);  contrast
 *     blend(x, mean over the image of gray(x as it is when the op runs), f);  saturation blend(x, gray(x), f);  hue: to fp32, rgb -> hsv,
 *     h <- (h + f) mod 1, hsv -> rgb, back to float64.  No contraction, correctly rounded divisions.
 * oryon_rgb_augment_resize: rgb_hwc [n,HI,WI,3] uint8 -> out [n,3,HO,WO] fp32 = oryon_rgb_resize_bilinear of the flipped, colour-jittered
 *     image (each touched texel goes through the chain in front of the interpolation; one rounding to fp32).  Two launches: the per-image
 *     gray mean for images with a contrast slot (fp64, fixed reduction tree, no float atomics: bit-stable), then the resize.  A table
 *     of zero flip bits and empty slots gives oryon_rgb_resize_bilinear's output bit for bit.  workspace: 8-byte aligned,
 *     oryon_rgb_augment_workspace_bytes(n) bytes, written and read by this call only.  HI*WI and HO*WO below 2^29.
 * oryon_resize_bilinear_f32_flip / oryon_mask_resize_nearest_flip: oryon_resize_bilinear_f32 / oryon_mask_resize_nearest applied to the
 *     image flipped as entry [0] of its table row says (the same table; nothing else of it is read), bit for bit. */
#define ORYON_AUG_SLOTS 8
#define ORYON_AUG_STRIDE 18
#define ORYON_AUG_HFLIP 1
#define ORYON_AUG_VFLIP 2
size_t oryon_rgb_augment_workspace_bytes(int n);
int oryon_rgb_augment_resize(const uint8_t *rgb_hwc, const double *table, int n, int HI, int WI, int HO, int WO,
                             void *workspace, size_t workspace_bytes, float *out, void *stream);
int oryon_resize_bilinear_f32_flip(const float *in, const double *table, int n, int HI, int WI, int HO, int WO, int round_output,
                                   float *out, void *stream);
int oryon_mask_resize_nearest_flip(const uint8_t *mask_in, const double *table, int n_maps, int HI, int WI, int HO, int WO,
                                   int32_t *mask_out, void *stream);

/* K1' the reference's fp16 matcher branch (corrs_device='cuda', utils/pcd.py:195-197) casts the descriptors to float16 first:
 *     out[i] = float(half(in[i])) (round to nearest even; may alias).  The exact matcher then runs on the rounded values. */
int oryon_round_to_f16_f32(const float *in, float *out, int64_t n, void *stream);

/* B1  QuickGELU of the CLIP residual blocks, y = x * sigmoid(1.702 x)  (third-party clip model.py, loaded at
 *     models/vlm.py:19), fused into one pass for bf16 activations: x, y [n] bf16 (16-byte aligned, may alias).
 *     Arithmetic in fp32, one rounding.  The fp32 backbone path keeps torch's own ops. */
int oryon_quick_gelu_bf16(const void *x, void *y, int64_t n, void *stream);

/* B2  residual add + LayerNorm of the CLIP residual stream (clip model.py ResidualAttentionBlock.forward:
 *     x = x + attention(ln_1(x)); x = x + mlp(ln_2(x)); torch.nn.LayerNorm semantics, biased variance), bf16 inference only:
 *         s = bf16(x + delta)   -> x_out   (delta == NULL: s = x, x_out not written)
 *         h = bf16((s - mean(s)) * rsqrt(var(s) + eps) * gamma + beta) -> h_out          statistics in fp32 over the rounded s
 *     x, delta, x_out, h_out [rows, D] bf16, gamma / beta [D] bf16; D % 8 == 0, D <= 4096; 16-byte aligned; x_out may alias x
 *     or delta, h_out must not alias an input. */
int oryon_add_layernorm_bf16(const void *x, const void *delta, const void *gamma, const void *beta, int64_t rows, int D, float eps,
                             void *x_out, void *h_out, void *stream);
/*     fp32 twin for the fp32 / fp16x3 inference path (same formula without the bf16 roundings; D % 4 == 0, D <= 2048). */
int oryon_add_layernorm_f32(const float *x, const float *delta, const float *gamma, const float *beta, int64_t rows, int D, float eps,
                            float *x_out, float *h_out, void *stream);

/* B3  shifted-window attention of the Swin guidance backbone (torchvision swin_transformer.shifted_window_attention, the
 *     swin_b feature extractor of net.py:60-75), window 7, head dim 32, bf16 inference: everything between the q|k|v Linear and
 *     the output projection in one kernel (pad, cyclic shift, window partition, q scale, QK^T + relative position bias + shift
 *     mask, softmax, PV, window merge, reverse shift, crop).
 *     qkv     [B, H, W, 3C] bf16: the q|k|v Linear applied to the un-windowed tokens (it commutes with the partition)
 *     pad_qkv [3C] bf16: q|k|v of a zero-padded token = the Linear's bias (zeros if it has none)
 *     bias_t  [heads, 49 (key), 49 (query)] fp32: relative_position_bias_table[relative_position_index], key-major
 *     out     [B, H, W, C] bf16;  C == heads * 32, heads <= 8, 0 <= shift < 7 (torchvision passes 0 or 3) */
int oryon_swin_window_attention_bf16(const void *qkv, const void *pad_qkv, const float *bias_t, int B, int H, int W, int C, int heads,
                                     int shift, void *out, void *stream);
/* the same operation on fp32 tensors (fp32 evaluation of the guidance tower): both products on the fp16 matrix pipe with error-compensated
 * operands (fp32-grade, ~1e-6 relative; round 4 - the fp32-VALU form of the bf16 kernel took twice as long), fp32 bias / mask / softmax */
int oryon_swin_window_attention_f32(const float *qkv, const float *pad_qkv, const float *bias_t, int B, int H, int W, int C, int heads,
                                    int shift, float *out, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K0  mask -> ROI.   Replaces torch.nonzero(mask == 1) (utils/pcd.py:184-185) and the validity test
 *     count_nonzero(mask == 1) > 0 (pipeline.py:391-393).
 * mask  [n_maps, HW] int32        roi [n_maps, HW] int32 (linear pixel index y*W+x, row-major order)
 * count [n_maps] int32
 */
int oryon_roi_compact(const int32_t *mask, int n_maps, int HW, int32_t *roi, int32_t *count, void *stream);

/* K0  sigmoid(logit) > threshold -> {0,1} int32 mask.  Replaces losses.py:58-59 (test.mask == predicted). */
int oryon_mask_from_logits(const float *logits, int64_t n, float threshold, int32_t *mask, void *stream);

/* K0  legacy-nearest resize of an integer mask to the feature-map grid (src = floor(dst * in/out) computed
 *     with the fp32 scale, as torch F.interpolate(mode='nearest') does).  Replaces pipeline.py:408-411. */
int oryon_mask_resize_nearest(const uint8_t *mask_in, int n_maps, int HI, int WI, int HO, int WO,
                              int32_t *mask_out, void *stream);

/* K0  device-side subsample WITHOUT replacement to at most max_keep entries per map, keeping row-major
 *     order.  Counter-based RNG keyed by (seed, map_key[m], element) so the result is independent of how
 *     maps are sharded over GPUs.  Stands in for torch_sample_select (utils/misc.py:242-254, called at
 *     utils/pcd.py:187-190) in the batched path; the drop-in Python facade keeps the host torch RNG.
 * map_key [n_maps] int64 (e.g. global pair index), may be NULL (then the map index is used). */
int oryon_roi_subsample(int32_t *roi, int32_t *count, int n_maps, int roi_stride, int max_keep, uint64_t seed,
                        const int64_t *map_key, void *stream);

/* K0  gather the ROI descriptors of channel-planar maps and L2-normalise them.
 *     Replaces feats[:, roi[:,0], roi[:,1]].T (utils/pcd.py:192-193) and the x / max(|x|, 1e-8) half of
 *     cosine_similarity (utils/pcd.py:28).
 * feat [n_maps, C, HW] fp32; roi [n_maps, roi_stride]; out [n_maps, rows_cap, C_pad] fp32, row-major; rows
 * >= count[m] up to the next multiple of 256 and columns C..C_pad-1 are zero-filled (zero columns do not
 * change the fmaf chain).  C_pad is a multiple of 32 (>= C), rows_cap a multiple of 256.
 * Layout note: inside every group of 8 columns the fp32 rows are stored k-permuted (position 8g+4h+j holds
 * k = 8g+2j+h, the order the MFMA operands consume 16-byte chunks in); consumers are K1 and K1s only.
 * out_f16 (may be NULL): [n_maps, rows_cap, C_pad] IEEE half copy of the same unit rows (round-to-nearest), natural k
 * order - the operand of the screening pass of oryon_match_screened. */
int oryon_gather_normalise_f32(const float *feat, int n_maps, int C, int HW, const int32_t *roi, int roi_stride,
                               const int32_t *count, int rows_cap, int C_pad, float *out, void *out_f16, void *stream);

/* K1  cosine nearest neighbour: for every anchor row the query row minimising 0.5*(1 - a^.q^).
 *     Replaces pdist(...,'inv_norm_cosine') + amin + argmin + (min_dist < th) (utils/pcd.py:202-205)
 *     without materialising [N1,N2] (the reference materialises [N1,N2,C]).
 * a_hat [B, cap_a, C], q_hat [B, cap_q, C]  (outputs of oryon_gather_normalise_f32; caps multiples of
 * ORYON_MATCH_TILE), n_a/n_q [B] int32 on device.
 * min_dist [B,cap_a] fp32, argmin [B,cap_a] int32 (first index on ties), valid [B,cap_a] uint8.
 * Arithmetic: exact fp32 — dot = k-ordered fmaf chain (v_mfma_f32_32x32x2_f32), dist = fma(-0.5,dot,0.5).
 * workspace: oryon_match_workspace_bytes(B, cap_a) bytes (used only when the launch splits the query range). */
size_t oryon_match_workspace_bytes(int B, int cap_a);
int oryon_match_f32(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q,
                    const int32_t *n_a, const int32_t *n_q, float threshold, float *min_dist, int32_t *argmin,
                    uint8_t *valid, void *workspace, size_t workspace_bytes, void *stream);

/* K1m mutual nearest neighbours: both directions of K1 from ONE all-pairs scan (csrc/match_mutual.hip).
 *     min_dist / argmin / valid [B,cap_a]: exactly what oryon_match_f32(a_hat, q_hat, ...) writes (rows < n_a).
 *     rev_min_dist / rev_argmin [B,cap_q]: exactly what oryon_match_f32(q_hat, a_hat, ...) - the roles swapped - writes for
 *     row j < n_q: the minimum over the n_a anchor rows passed in (first anchor index on ties).
 *     mutual [B,cap_a] uint8: valid[i] && rev_argmin[argmin[i]] == i.  The argmin of a pair's mutual rows are pairwise distinct,
 *     and on a mutual row rev_min_dist[argmin[i]] has the bits of min_dist[i].
 * Pairs with n_a == 0 or n_q == 0 get what the two calls leave (INFINITY, index 0, valid 0) and mutual 0; rows >= n_a / >= n_q of
 * the outputs are not written, rows >= n_a / >= n_q of the INPUTS are never used (masked by index in both directions).
 * C a multiple of 32, caps multiples of ORYON_MATCH_TILE (cap_q of 256 when C == 32), B <= 65535.
 * workspace: oryon_match_mutual_workspace_bytes(B, cap_a, cap_q) = ORYON_MATCH_MUTUAL_KEY_WORDS 8-byte words per query row
 * (B cap_q of them: the (distance, index) keys the anchor panels meet in with a 64-bit atomic minimum) + oryon_match_workspace_bytes(B,
 * cap_a) for K1's query splits; no per-panel slab. */
#define ORYON_MATCH_MUTUAL_KEY_WORDS 1
size_t oryon_match_mutual_workspace_bytes(int B, int cap_a, int cap_q);
int oryon_match_mutual_f32(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q,
                           const int32_t *n_a, const int32_t *n_q, float threshold,
                           float *min_dist, int32_t *argmin, uint8_t *valid,
                           float *rev_min_dist, int32_t *rev_argmin, uint8_t *mutual,
                           void *workspace, size_t workspace_bytes, void *stream);

/* K1r the ratio test with an exclusion disc: a second all-pairs scan with a per-anchor spatial mask (csrc/match_second.hip).
 *     dist(i, j) = fma(-0.5, dot(a_i, q_j), 0.5), the dot product K1's k-ordered fmaf chain: the bits of oryon_match_f32.
 *     roi_q[p roi_stride_q + j] is the linear pixel index of query row j in a map W_q wide (as oryon_select_corrs reads it);
 *     (y*, x*) is the pixel of roi_q[argmin[i]], (y_j, x_j) that of roi_q[j].
 *     Candidates of row i: all j < n_q with (y_j - y*)^2 + (x_j - x*)^2 >= radius^2 (integers; the rule of the training loss, which
 *     excludes pixel distance < neg_kernel).  radius = 1 excludes exactly the best row's own pixel (and rows sharing it).
 *     second_dist / second_argmin [B,cap_a]: the minimum of dist(i, j) over the candidates, first query index on ties; INFINITY and
 *     index 0 when there is no candidate (n_q == 0 included).  Written for every row i < n_a whatever the gate says; rows >= n_a are
 *     not written, rows >= n_a / >= n_q of the INPUTS are never used (masked by index).
 *     keep [B,cap_a] uint8 = gate[i] && min_dist[i] <= __fmul_rn(ratio, second_dist[i]).  gate [B,cap_a] uint8 is K1's valid or
 *     K1m's mutual; NULL counts as all ones.  second_dist = INFINITY keeps the row (no competitor).  The candidates are a subset
 *     of the rows K1 minimised over, with the same bits, so second_dist >= min_dist and ratio = 1 returns keep == gate.
 *     min_dist / argmin are the outputs of oryon_match_f32 or oryon_match_mutual_f32 on the same operands.
 * 1 <= radius <= 1024, 0 < ratio <= 1, 1 <= W_q <= 65535 and every pixel's row index <= 65535 (a pixel packs into y << 16 | x).
 * C a multiple of 32, caps multiples of ORYON_MATCH_TILE (cap_q of 256 when C == 32), B <= 65535; B == 0 returns ORYON_OK.
 * workspace: oryon_match_second_workspace_bytes(B, cap_a): K1's query-split buffers. */
size_t oryon_match_second_workspace_bytes(int B, int cap_a);
int oryon_match_second_f32(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q,
                           const int32_t *n_a, const int32_t *n_q,
                           const int32_t *roi_q, int roi_stride_q, int W_q, int radius,
                           const float *min_dist, const int32_t *argmin, const uint8_t *gate, float ratio,
                           float *second_dist, int32_t *second_argmin, uint8_t *keep,
                           void *workspace, size_t workspace_bytes, void *stream);

/* K1n one rank of the one-to-many matcher: the best query row outside the discs round up to three earlier ranks
 *     (csrc/match_next.hip).  The ranks of anchor row i of a pair:
 *       c_1 = argmin[i], d_1 = min_dist[i]: K1's outputs.
 *       dist(i, j) = fma(-0.5, dot(a_i, q_j), 0.5), the dot product K1's k-ordered fmaf chain: the bits of oryon_match_f32 and
 *       oryon_match_second_f32.
 *       For r = 2..K the candidates are the rows j < n_q whose pixel lies outside the disc of `radius` round the pixel of EVERY
 *       earlier rank c_1 .. c_{r-1}: dy^2 + dx^2 >= radius^2 in integers (K1r's rule).  An earlier rank whose index is not in
 *       [0, n_q) excludes nothing.
 *       d_r is the minimum of dist(i, j) over the candidates, c_r the first query index on ties; with no candidate d_r = INFINITY
 *       and c_r = -1, and so for every later rank.  The candidate sets are nested, so d_r >= d_{r-1}.
 *     One call is one rank: prev_argmin holds n_prev = r - 1 planes (1..3) of [B, cap_a] int32, plane-major (plane k at
 *     prev_argmin + k B cap_a), next_dist / next_argmin [B, cap_a] receive (d_r, c_r).  With a [K, B, cap_a] table whose plane 0 is
 *     argmin, rank r reads planes 0 .. r-2 and writes plane r-1.  n_prev = 1 gives oryon_match_second_f32's second_dist bit for
 *     bit (its second_argmin too, but for -1 where that one writes 0 for "none").
 *     Rows >= n_a are not written, rows >= n_a / >= n_q of the inputs are never used.  Other operands, limits and the workspace
 *     (oryon_match_next_workspace_bytes(B, cap_a): K1's query-split buffers) are oryon_match_second_f32's. */
size_t oryon_match_next_workspace_bytes(int B, int cap_a);
int oryon_match_next_f32(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q,
                         const int32_t *n_a, const int32_t *n_q,
                         const int32_t *roi_q, int roi_stride_q, int W_q, int radius,
                         const int32_t *prev_argmin, int n_prev, float *next_dist, int32_t *next_argmin,
                         void *workspace, size_t workspace_bytes, void *stream);

/* K1s same contract as oryon_match_f32 for every anchor row that can reach the threshold, computed as an fp16-MFMA
 *     screening pass (v_mfma_f32_32x32x16_f16 on the IEEE-half copies written by oryon_gather_normalise_f32) followed by
 *     an exact fp32 re-scoring of the surviving candidates with K1's canonical fmaf chain.  A proven error bound on the
 *     screening scores (csrc/match16.hip) guarantees that every exact minimiser is a candidate, so on rows with
 *     valid == 1 `min_dist` / `argmin` are bit-identical to oryon_match_f32, and `valid` is identical on every row.
 *     Rows that provably cannot reach the threshold get valid = 0, argmin = 0 and the screening estimate as min_dist.
 * C (padded) must be 128, 256 or 512, cap_a a multiple of 256; a_f16 / q_f16 are the half copies [B, cap, C]. */
size_t oryon_match_screened_workspace_bytes(int B, int C, int cap_a);
int oryon_match_screened(const float *a_hat, const float *q_hat, const void *a_f16, const void *q_f16, int B, int C,
                         int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, float *min_dist,
                         int32_t *argmin, uint8_t *valid, void *workspace, size_t workspace_bytes, void *stream);

/* K1s8 the same contract again with an INT8 pre-screen (v_mfma_i32_32x32x32_i8: twice the fp16 matrix rate) in front of K1s:
 *     oryon_gather_normalise_q8 additionally writes int8 rows q = rint(x^ * 2^E) with one exponent per 16-row slice of the
 *     screening kernel's accumulator layout (slice_scale = 2^-E, eps_max = largest 2^-(E+1) of the map).  Anchors whose int8
 *     maximum is decided within the proven int8 bound go straight to fp16 slice re-scoring + exact fp32 re-scoring; every other
 *     anchor runs through the complete K1s pipeline on a compacted set.  Outputs are therefore identical to oryon_match_screened
 *     (and to oryon_match_f32 on valid rows) for every input; only the run time depends on the data.  C_pad 256 or 512.
 *     The fp16 operands of that second stage are derived from the fp32 rows inside the call, and only for pairs that need
 *     them, so out_f16 of oryon_gather_normalise_q8 may be NULL on this path.
 *     C_true = number of real channels (<= C_pad), used in the bound. */
int oryon_gather_normalise_q8(const float *feat, int n_maps, int C, int HW, const int32_t *roi, int roi_stride, const int32_t *count,
                              int rows_cap, int C_pad, float *out, void *out_f16, int8_t *out_i8, float *slice_scale, float *eps_max,
                              void *stream);
size_t oryon_match_screened8_workspace_bytes(int B, int C, int cap_a, int cap_q);
int oryon_match_screened8(const float *a_hat, const float *q_hat, const int8_t *a_i8, const int8_t *q_i8, const float *a_scale, const float *q_scale, const float *q_eps_max, int B, int C_true,
                          int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, float *min_dist,
                          int32_t *argmin, uint8_t *valid, int32_t *n_undecided /* [B] or NULL: anchors handed to the fp16 stage */,
                          void *workspace, size_t workspace_bytes, void *stream);

/* K0v3 + K1s8 without an fp32 copy of the query rows (round 2; csrc/gather8.hip).
 *     Replaces the same reference lines as oryon_gather_normalise_q8 / oryon_match_screened8 (utils/pcd.py:192-193, :28-29, :202-205).
 *     oryon_gather_q8 reads the raw descriptors of the ROI rows once - from a channel-planar [n_maps,C,H,W] map (ORYON_LAYOUT_NCHW, what
 *     net.py:162-167 returns) or from a channels_last [n_maps,H,W,C] map (ORYON_LAYOUT_NHWC, zero-copy view of a torch channels_last
 *     tensor) - and writes the int8 rows, the per-slice scales, eps_max, the canonical row norm d (row_norm [n_maps, rows_cap], may be
 *     NULL) and, only when out_f32 != NULL, the canonical fp32 unit rows (k-permuted, as oryon_gather_normalise_f32 writes them).
 *     oryon_match_screened8_raw is oryon_match_screened8 for such operands: anchors come as materialised fp32 + int8 rows, queries as
 *     int8 rows + row norms + the raw map itself; the exact re-scoring pass recovers a candidate's canonical unit values x_k / d from
 *     the raw map, so its outputs are bit for bit those of oryon_match_screened8.  Pairs that need the fp32 query rows after all
 *     (anchors the int8 stage could not decide, overflowed candidate lists) get them materialised inside the call, gated on the device.
 *     Rows [n, round_up(n,256)) of every output are zero rows; rows beyond are not written.
 *     round_f16 != 0 selects the reference's half-descriptor branch (utils/pcd.py:195-197, `corrs_device='cuda'`: feats.half() before
 *     pdist): every raw descriptor value is rounded to the nearest float16 on the way in, in all three calls alike; the arithmetic on
 *     the rounded values is unchanged (fp32), which is what BASELINE configs[4] ("fp16 descriptors") runs. */
#define ORYON_LAYOUT_NCHW 0
#define ORYON_LAYOUT_NHWC 1
int oryon_gather_q8(const float *feat, int n_maps, int C, int HW, int layout, const int32_t *roi, int roi_stride, const int32_t *count,
                    int rows_cap, int C_pad, int8_t *out_i8, float *slice_scale, float *eps_max, float *row_norm, float *out_f32,
                    int round_f16, void *stream);
size_t oryon_match_screened8_raw_workspace_bytes(int B, int C, int cap_a, int cap_q);
int oryon_match_screened8_raw(const float *a_hat, const int8_t *a_i8, const float *a_scale, const float *feat_q, int C_true, int HW,
                              int layout, const int32_t *roi_q, int roi_stride, const float *q_norm, const int8_t *q_i8,
                              const float *q_scale, const float *q_eps_max, int B, int C, int cap_a, int cap_q, const int32_t *n_a,
                              const int32_t *n_q, float threshold, float *min_dist, int32_t *argmin, uint8_t *valid,
                              int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes, void *stream);

/* K1s8 + K1b fused and LAZY (round 2): from the K0v3 operands straight to the sampled correspondences of every pair
 * (utils/pcd.py:202-214).  The int8 bound settles the validity flag of almost every anchor without its argmin; candidate generation
 * and exact re-scoring then run for the <= max_corrs sampled anchors only.  Anchors whose validity the bound cannot settle are resolved
 * exactly before the sampling.  AMBIGUOUS anchors (runner-up slice within the int8 margin of the best one) are resolved by the exact
 * fp32 scan K1 on a compacted list of just those rows - before the sampling if their validity is open, after it (sampled rows only)
 * if the bound already proves them valid - against fp32 query rows materialised for that pair inside the call.  force_eager != 0
 * sends every pair through the complete tail of oryon_match_screened8_raw instead (all of min_dist / argmin exact).  corrs / n_valid / n_sel / status are exactly what oryon_select_corrs returns on the outputs of
 * oryon_match_screened8_raw.  valid [B,cap_a] is exact on every row; argmin is exact on sampled rows and on every row of an eager
 * pair; min_dist is exact on every row of an eager pair and on the sampled / resolved rows that needed an fp32 comparison (more than one
 * candidate inside the int8 margin, or validity open); elsewhere both hold the screening estimate / 0. */
size_t oryon_match_corrs_i8_workspace_bytes(int B, int C, int cap_a, int cap_q, int corr_rows);
int oryon_match_corrs_i8(const float *a_hat, const int8_t *a_i8, const float *a_scale, const float *feat_q, int C_true, int HW, int layout,
                         const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q, int roi_stride_q, const float *q_norm,
                         const int8_t *q_i8, const float *q_scale, const float *q_eps_max, int B, int C, int cap_a, int cap_q,
                         const int32_t *n_a, const int32_t *n_q, float threshold, int W, int max_corrs, int corr_rows, uint64_t seed,
                         const int64_t *pair_key, int force_eager, float *min_dist, int32_t *argmin, uint8_t *valid, int32_t *corrs,
                         int32_t *n_valid, int32_t *n_sel, int32_t *status, int32_t *n_undecided, int round_f16, void *workspace,
                         size_t workspace_bytes, void *stream);

/* K0 + K1s6 (round 3): the same lazy matcher with an MX-fp6 screen in place of the int8 one.  Replaces the same reference lines
 * (utils/pcd.py:192-193, :28-29, :202-214); the results are those of oryon_match_corrs_i8 bit for bit (every decision the screen takes is
 * backed by a proven bound, everything else is resolved exactly), only the dominant kernel changes: v_mfma_scale_f32_32x32x64_f8f6f4
 * multiplies 64 channels per instruction at the int8 instruction's rate.
 *     oryon_gather_mx6 writes, per ROI row and 32-channel block, one 32-byte slot: bytes 0-23 = 32 fp6 (e2m3) codes of x^ / 2^e (element t
 *     at bits [6t, 6t+6)), byte 24 = e + 127 (E8M0), bytes 25-31 = 0 - rows of C_pad bytes, like the int8 rows; the block exponent puts the
 *     block's largest magnitude into (3.75, 7.5].  err_max [n_maps] receives the largest MEASURED quantisation error |x^ - dequant|_2 over
 *     the map's live rows; row_norm / out_f32 as oryon_gather_q8.
 *     oryon_match_corrs_mx6 = oryon_match_corrs_i8 on such operands (lazy route only): |s6 - a^.q^| <= |ea| + |eq| + |ea||eq| + 1.2e-4 with
 *     ea / eq the pair's a_err_max / q_err_max decides validity and unambiguity; the winning slice's 16 rows are re-scored from the mx6
 *     slots, candidates inside the margin of the slice maximum go to the exact fp32 chain on the raw map.  Workspace:
 *     oryon_match_corrs_i8_workspace_bytes. */
int oryon_gather_mx6(const float *feat, int n_maps, int C, int HW, int layout, const int32_t *roi, int roi_stride, const int32_t *count,
                     int rows_cap, int C_pad, uint8_t *out_mx6, float *err_max, float *row_norm, float *out_f32, int round_f16, void *stream);
int oryon_match_corrs_mx6(const float *a_hat, const uint8_t *a_mx6, const float *a_err_max, const float *feat_q, int C_true, int HW, int layout,
                          const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q, int roi_stride_q, const float *q_norm,
                          const uint8_t *q_mx6, const float *q_err_max, int B, int C, int cap_a, int cap_q, const int32_t *n_a,
                          const int32_t *n_q, float threshold, int W, int max_corrs, int corr_rows, uint64_t seed, const int64_t *pair_key,
                          float *min_dist, int32_t *argmin, uint8_t *valid, int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status,
                          int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes, void *stream);

/* K0 + K1x3 operands in ONE pass (round 4).  On descriptor fields where the screen cannot separate a sampled anchor's near-ties (smooth decoder
 * outputs) the matcher needs the query rows once more as error-compensated half rows (hi = half(u), lo = half(u - hi) of the canonical unit
 * row u) for its fp16x3 second level - a second read of the maps inside oryon_match_corrs_mx6.  oryon_gather_mx6_x3 writes them in the same
 * pass as the mx6 slots (replaces the same reference lines as oryon_gather_mx6, utils/pcd.py:192-193, :28-29): hi_lo_f16 = [2][n_maps,
 * rows_cap, 256] halves (all hi rows, then all lo rows), lo_sq_max [n_maps] = largest |u - hi|^2 of the map's rows.  C_pad = 256 only.
 * oryon_match_corrs_mx6_x3 = oryon_match_corrs_mx6 that takes those rows instead of making them: same corrs / n_valid / n_sel / status /
 * valid, bit for bit.  Since round 6 its screen runs as a VALIDITY CASCADE (this is the route of maps on which every anchor is valid and
 * ambiguous, where the full screen bought nothing but validity): (1) a windowed launch - two query tiles per (1024-anchor panel, query
 * split), placed where the panel sits in its own map; a panel all of whose anchors are thereby valid for sure (one witness above
 * 1 - 2 thr + the proven bound suffices: utils/pcd.py:204 is "min over queries < threshold") is settled, its runner-ups read "open";
 * (2) the complete scan for the other panels only (device-gated); (3) after the sampling, the complete screen for the <= max_corrs
 * sampled rows whose argmin is open (one 512-row panel per pair), which gives them their true winning slice - rows that turn out
 * unambiguous are resolved from it, the others go to the fp16x3 second level with it as their seed.  corr_rows <= 512.  min_dist of rows
 * that were neither sampled nor resolved holds the estimate of the scan that settled them (here possibly a partial one); n_undecided =
 * the first pass's count scaled by the share of sampled rows that stayed ambiguous after (3) (the engine's route feedback). */
int oryon_gather_mx6_x3(const float *feat, int n_maps, int C, int HW, int layout, const int32_t *roi, int roi_stride, const int32_t *count,
                        int rows_cap, int C_pad, uint8_t *out_mx6, float *err_max, float *row_norm, void *hi_lo_f16, float *lo_sq_max,
                        int round_f16, void *stream);
int oryon_match_corrs_mx6_x3(const float *a_hat, const uint8_t *a_mx6, const float *a_err_max, const float *feat_q, int C_true, int HW, int layout,
                             const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q, int roi_stride_q, const float *q_norm,
                             const uint8_t *q_mx6, const float *q_err_max, const void *q_hi_lo_f16, const float *q_lo_sq_max, int B, int C,
                             int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, int W, int max_corrs, int corr_rows,
                             uint64_t seed, const int64_t *pair_key, float *min_dist, int32_t *argmin, uint8_t *valid, int32_t *corrs,
                             int32_t *n_valid, int32_t *n_sel, int32_t *status, int32_t *n_undecided, int round_f16, void *workspace,
                             size_t workspace_bytes, void *stream);

/* Anchor rows on demand.  The three lazy matchers above read the anchors' fp32 unit rows a_hat [B, cap_a, C] - which K0 has to write, 1 KB
 * per anchor at C = 256, 80 % of what its anchor pass stores - for a few hundred rows per pair only: the sampled rows with more than one
 * candidate, the rows whose validity the screen leaves open and the ambiguous rows' compacted lists.  The `_araw` entries take the raw
 * anchor map instead (feat_a, the map the anchor operands were gathered from - same C_true / HW / layout as feat_q - and a_norm [B, cap_a],
 * the row_norm output of the anchor pass) and form those rows themselves, exactly as K0 does: x_k at pixel roi_a[row] (rounded to float16
 * first under round_f16, zero for k >= C_true) divided by a_norm[row], correctly rounded - bit for bit the value K0 stores.  K0 is then
 * called with out_f32 = NULL for the anchors.  Every output equals that of the entry without the suffix, bit for bit (utils/pcd.py:202-214
 * as there).  Lazy route only: there is no force_eager (the eager tail reads whole pairs of rows - oryon_match_corrs_i8 on materialised
 * rows keeps that).  Workspace: oryon_match_corrs_i8_workspace_bytes. */
int oryon_match_corrs_i8_araw(const float *feat_a, const float *a_norm, const int8_t *a_i8, const float *a_scale, const float *feat_q, int C_true,
                              int HW, int layout, const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q, int roi_stride_q,
                              const float *q_norm, const int8_t *q_i8, const float *q_scale, const float *q_eps_max, int B, int C, int cap_a,
                              int cap_q, const int32_t *n_a, const int32_t *n_q, float threshold, int W, int max_corrs, int corr_rows,
                              uint64_t seed, const int64_t *pair_key, float *min_dist, int32_t *argmin, uint8_t *valid, int32_t *corrs,
                              int32_t *n_valid, int32_t *n_sel, int32_t *status, int32_t *n_undecided, int round_f16, void *workspace,
                              size_t workspace_bytes, void *stream);
int oryon_match_corrs_mx6_araw(const float *feat_a, const float *a_norm, const uint8_t *a_mx6, const float *a_err_max, const float *feat_q,
                               int C_true, int HW, int layout, const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q, int roi_stride_q,
                               const float *q_norm, const uint8_t *q_mx6, const float *q_err_max, int B, int C, int cap_a, int cap_q,
                               const int32_t *n_a, const int32_t *n_q, float threshold, int W, int max_corrs, int corr_rows, uint64_t seed,
                               const int64_t *pair_key, float *min_dist, int32_t *argmin, uint8_t *valid, int32_t *corrs, int32_t *n_valid,
                               int32_t *n_sel, int32_t *status, int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes,
                               void *stream);
int oryon_match_corrs_mx6_x3_araw(const float *feat_a, const float *a_norm, const uint8_t *a_mx6, const float *a_err_max, const float *feat_q,
                                  int C_true, int HW, int layout, const int32_t *roi_a, int roi_stride_a, const int32_t *roi_q,
                                  int roi_stride_q, const float *q_norm, const uint8_t *q_mx6, const float *q_err_max, const void *q_hi_lo_f16,
                                  const float *q_lo_sq_max, int B, int C, int cap_a, int cap_q, const int32_t *n_a, const int32_t *n_q,
                                  float threshold, int W, int max_corrs, int corr_rows, uint64_t seed, const int64_t *pair_key, float *min_dist,
                                  int32_t *argmin, uint8_t *valid, int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status,
                                  int32_t *n_undecided, int round_f16, void *workspace, size_t workspace_bytes, void *stream);

/* "Sample first" (optional engine schedule, off by default).  Only max_corrs correspondences per pair leave the matcher
 * (utils/pcd.py:205-214), drawn uniformly from the valid anchor rows - so a uniformly random first-stage subset of the anchors that
 * already holds >= max_corrs valid rows yields an identically distributed sample.  The engine runs the matcher on such a subset;
 * oryon_sample_first_gate computes, on the device, which pairs must be redone on all of their anchors (n_a2 = n_a where the first stage
 * found fewer than max_corrs valid rows although anchors were left out, else 0 - every second-stage launch then sees no anchors for the
 * other pairs) and oryon_sample_first_merge copies the second stage's rows / counts / status over the first stage's for those pairs. */
int oryon_sample_first_gate(const int32_t *n_valid1, const int32_t *n_a1, const int32_t *n_a, int B, int max_corrs, int32_t *n_a2,
                            void *stream);
int oryon_sample_first_merge(const int32_t *n_a2, const int32_t *corrs2, const int32_t *n_valid2, const int32_t *n_sel2,
                             const int32_t *status2, int B, int corr_rows, int32_t *corrs1, int32_t *n_valid1, int32_t *n_sel1,
                             int32_t *status1, void *stream);

/* K1b turn matcher outputs into sampled correspondences (device RNG; batched path only).
 *     Replaces utils/pcd.py:205-214: keep rows with valid, need more than one, sample exactly max_corrs
 *     (with replacement iff fewer are available).
 * corrs [B, corr_rows, 4] int32 (y1,x1,y2,x2 in feature-map coordinates; corr_rows >= max_corrs is the row
 * stride per pair, rows >= max_corrs are left untouched), n_valid [B] (rows under the threshold), n_sel [B]
 * (max_corrs or 0; may be NULL), status [B] (ORYON_PAIR_OK / ORYON_PAIR_NO_MASK when n_a or n_q is 0 /
 * ORYON_PAIR_NO_CORR when <= 1 valid row).  scratch [B, cap_a] int32 (ordered list of valid anchor rows). */
int oryon_select_corrs(const int32_t *roi_a, const int32_t *roi_q, int roi_stride_a, int roi_stride_q,
                       const int32_t *n_a, const int32_t *n_q, const int32_t *argmin, const uint8_t *valid, int cap_a,
                       int B, int W, int max_corrs, int corr_rows, uint64_t seed, const int64_t *pair_key,
                       int32_t *scratch, int32_t *corrs, int32_t *n_valid, int32_t *n_sel, int32_t *status, void *stream);

/* K1k one-to-many correspondences: the sampler of oryon_select_corrs, then up to K rows per drawn anchor (csrc/post.hip).
 *     The sampler draws anchors exactly as oryon_select_corrs does on the same arguments (same gate `valid`, same keys, same slots),
 *     so n_valid / n_sel / status are that call's and slot s holds anchor row i_s.  The drawn rows of a_hat are gathered into
 *     [B, cap_s, C], cap_s = round_up(max_corrs, ORYON_MATCH_TILE), and K - 1 rank scans (oryon_match_next_f32's definition) run on
 *     those cap_s rows only.  Slot s then emits
 *       its rank-1 row (the row oryon_select_corrs writes), always;
 *       its rank-r row, r >= 2: (y, x) of the anchor, (y, x) of query row c_r - iff c_r >= 0, d_r < threshold (K1's comparison for
 *       `valid`, the same float) and d_r <= __fadd_rn(d_1, margin).
 *     Rows come out in (slot, rank) order, compacted: corrs [B, corr_rows, 4] int32, corr_rows >= K max_corrs; rank [B, corr_rows]
 *     uint8 (1..K); n_rows [B] <= K max_corrs; rows >= n_rows[b] of corrs and rank are left untouched.
 *     margin >= 0 is an additive slack on the cosine distance, INFINITY switches it off.  1 <= K <= 4, 1 <= radius <= 1024,
 *     1 <= W <= 65535 (one map width for both sides, as oryon_select_corrs); the shape limits of oryon_match_second_f32.
 *     min_dist / argmin / valid [B, cap_a]: oryon_match_f32 on the same operands with `threshold`.
 *     Optional outputs (NULL = not wanted, K > 1 only): sel_rows [B, cap_s] (anchor row of every slot), cand_dist / cand_argmin
 *     [K, B, cap_s] (rank r in plane r - 1; slots >= n_sel not written).  n_sel may be NULL.
 *     K = 1 launches the sampler alone, straight into corrs: the bytes of oryon_select_corrs.  rank and n_rows may then both be
 *     NULL; given, one more small launch fills them (all ones, n_sel).
 *     No allocation, no synchronisation; workspace: oryon_topk_corrs_workspace_bytes(B, C, cap_a, max_corrs, K). */
size_t oryon_topk_corrs_workspace_bytes(int B, int C, int cap_a, int max_corrs, int K);
int oryon_topk_corrs(const float *a_hat, const float *q_hat, int B, int C, int cap_a, int cap_q,
                     const int32_t *roi_a, const int32_t *roi_q, int roi_stride_a, int roi_stride_q,
                     const int32_t *n_a, const int32_t *n_q,
                     const float *min_dist, const int32_t *argmin, const uint8_t *valid, float threshold,
                     int W, int max_corrs, int corr_rows, uint64_t seed, const int64_t *pair_key,
                     int K, int radius, float margin,
                     int32_t *corrs, uint8_t *rank, int32_t *n_valid, int32_t *n_sel, int32_t *status, int32_t *n_rows,
                     int32_t *sel_rows, float *cand_dist, int32_t *cand_argmin,
                     void *workspace, size_t workspace_bytes, void *stream);

/* K2  scale (y,x) to the original image, keep rows inside both images, truncate, gather depth, pin-hole
 *     lift, /1000.  Replaces pipeline.py:447-460 + utils/coordinates.py:5-48 + utils/pcd.py:44-74.
 * corrs [B, n_cap, 4] int32; n_corr [B] (clamped to [0, n_cap]) or NULL (then n_cap rows each); depth_* [B,H*,W*] fp32 millimetres;
 * cam_* [B,9] fp32 (row-major K, already rounded from the reference's fp64); status [B] may be NULL
 * (pairs whose status != ORYON_PAIR_OK are skipped and get n_out = 0).
 * pcd_a/pcd_q [B, n_cap, 3] fp32 metres, compacted over valid rows in order, rows >= n_out zeroed; n_out [B]. */
int oryon_lift_pairs(const int32_t *corrs, const int32_t *n_corr, int B, int n_cap, int FH, int FW,
                     const float *depth_a, int HA, int WA, const float *depth_q, int HQ, int WQ,
                     const float *cam_a, const float *cam_q, const int32_t *status, float *pcd_a, float *pcd_q,
                     int32_t *n_out, void *stream);

/* K1x sub-pixel refinement of selected correspondences (csrc/match_subpix.hip; no counterpart in the reference): where, between the
 *     pixels of the query map, the descriptor distance to the anchor is smallest.  A pure post-pass on the rows a sampler selected.
 * feat_a / feat_q [B, C, FH, FW] fp32, C <= 512, in `layout` (ORYON_LAYOUT_NCHW | ORYON_LAYOUT_NHWC); corrs [B, n_cap, 4] int32
 * (y_a, x_a, y_q, x_q); n_corr [B] (clamped to [0, n_cap]) or NULL (n_cap rows each); status [B] or NULL (pairs whose status !=
 * ORYON_PAIR_OK do no work); curv_min >= 0.
 *     All in float64 on the fp32 inputs.  With eps = 1e-8 and u^ = u / max(|u|, eps):
 *       f(i, j) = 0.5 (1 - <a^, q^>) for the query pixel (y_q + i, x_q + j), i, j in {-1, 0, 1} - whether the query mask holds it or not;
 *     the least-squares quadratic through the nine values (facet model):
 *       g_x  = sum_i (f(i,1) - f(i,-1)) / 6                  g_y  = sum_j (f(1,j) - f(-1,j)) / 6
 *       h_xx = sum_i (f(i,1) - 2 f(i,0) + f(i,-1)) / 3       h_yy = sum_j (f(1,j) - 2 f(0,j) + f(-1,j)) / 3
 *       h_xy = (f(1,1) - f(1,-1) - f(-1,1) + f(-1,-1)) / 4
 *       l_min = (h_xx + h_yy) / 2 - sqrt((h_xx - h_yy)^2 / 4 + h_xy^2),   o = -H^-1 g.
 *     flags [B, n_cap] uint8, in this order:
 *       1 border:  y_q outside [1, FH - 2] or x_q outside [1, FW - 2] (or the anchor pixel outside its map: nothing is read)
 *       2 flat or not a minimum:  l_min < curv_min
 *       3 outside:  not max(|o_x|, |o_y|) <= 1 (a NaN lands here)
 *       0 refined: otherwise; o clamped to [-0.5, 0.5] per axis.
 *     offsets [B, n_cap, 2] fp32 (dy, dx): the clamped o of flag 0, zero for flags 1 to 3.  counts [B, 4] int32: rows per flag value.
 *     Rows >= n_corr[b] and skipped pairs: offsets and flags zero, not counted.
 *     The channel sums run in an order fixed by C alone: the bytes do not depend on the batch position, the stream, the run or the
 *     layout.  Two launches, no allocation, no synchronisation, no atomics. */
int oryon_subpix_refine(const float *feat_a, const float *feat_q, int B, int C, int FH, int FW, int layout, const int32_t *corrs,
                        const int32_t *n_corr, const int32_t *status, int n_cap, float curv_min, float *offsets, uint8_t *flags,
                        int32_t *counts, void *stream);

/* K2x K2 on refined query coordinates: oryon_lift_pairs' arguments plus offsets [B, n_cap, 2] fp32 (dy, dx on the query side, in
 *     feature-map pixels; NULL = zeros) and depth_jump_mm >= 0; the same outputs, compaction and zero tail.
 *     Every operation is one correctly rounded fp32 operation, in this order, nothing contracted (s_* = K2's scale factors):
 *       y_a' = float(y_a) * s_ya, x_a' alike;   y_q' = (float(y_q) + dy) * s_yq, x_q' alike;
 *       a row is kept when 0 <= y' < H and 0 <= x' < W on both sides (K2's rule on the refined coordinates; a NaN offset drops the row);
 *       per side, i0 = (int)y', j0 = (int)x', f_y = y' - i0, f_x = x' - j0, z00 = depth[i0, j0], z01 = depth[i0, j0 + 1], z10 =
 *       depth[i0 + 1, j0], z11 = depth[i0 + 1, j0 + 1]:
 *         if i0 + 1 < H, j0 + 1 < W, all four > 0 and max - min <= depth_jump_mm:
 *           z = (1 - f_y) * ((1 - f_x) * z00 + f_x * z01) + f_y * ((1 - f_x) * z10 + f_x * z11)
 *         else z = z00: the pixel K2 reads, a zero depth included, as the reference does;
 *       X = ((x' - cx) * z) / fx / 1000, Y = ((y' - cy) * z) / fy / 1000, Z = z / 1000 on the FLOAT coordinates.
 *     Pixel (i, j) stands for the point (i, j), not (i + 0.5, j + 0.5): the reference's convention (none), kept on purpose. */
int oryon_lift_pairs_subpix(const int32_t *corrs, const float *offsets, const int32_t *n_corr, int B, int n_cap, int FH, int FW,
                            const float *depth_a, int HA, int WA, const float *depth_q, int HQ, int WQ, const float *cam_a,
                            const float *cam_q, const int32_t *status, float depth_jump_mm, float *pcd_a, float *pcd_q, int32_t *n_out,
                            void *stream);

/* K2' lift_pcd itself (utils/pcd.py:35-81 with xy_idxs): selected pixels of ONE depth map [H,W] fp32 ->
 *     [n,3] fp32 in the depth's unit (millimetres), X = ((x - cx) * z) / fx etc., no fma contraction.
 *     x_idx / y_idx [n] int32 must be inside the image (the reference would raise an IndexError). */
int oryon_lift_points(const float *depth, int H, int W, const float *cam9, const int32_t *x_idx, const int32_t *y_idx,
                      int n, float *out, void *stream);

/* K8  batched weighted Kabsch with an in-kernel 3x3 SVD (one-sided Jacobi, fp64 internal).
 *     Replaces rigid_transform_3d (models/pointdsc/common.py:7-45) incl. its H.cpu() -> LAPACK round trip.
 * A,B [nb, m, 3] fp32; w [nb, m] fp32 or NULL (all ones); negative weights count as 0 (common.py:20).
 * T [nb, 16] fp32 row-major 4x4. */
int oryon_kabsch_batched(const float *A, const float *B, const float *w, int nb, int m, float *T, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * K3-K10  PointDSC registration (models/pointdsc/PointDSC.py:128-197, inference branch, wrapped as
 *         utils/pointdsc/init.py:10-29 does: corr_pos = cat(src,tgt) - mean).
 */
typedef struct oryon_pointdsc oryon_pointdsc_t;

typedef struct {
    int in_dim;             /* 6 */
    int num_layers;         /* release config: 12 */
    int num_channels;       /* 128 (32, 64 or 128 supported) */
    int num_iterations;     /* power-iteration cap, 10 */
    float ratio;            /* seeds = int(n * ratio), 0.1 */
    float inlier_threshold; /* 0.10 */
    float sigma_d;          /* 0.10 (sigma_spat) */
    int k;                  /* 40 */
    float nms_radius;       /* 0.10 */
} oryon_pointdsc_config_t;

int oryon_pointdsc_create(oryon_pointdsc_t **handle, const oryon_pointdsc_config_t *cfg);
void oryon_pointdsc_destroy(oryon_pointdsc_t *handle);
/* Load one tensor by its reference state-dict name (models/pointdsc/PointDSC.py:9-25,49-63,97-113), fp32
 * host data.  Unknown names -> ORYON_ERR_INVALID_ARG; num_batches_tracked is accepted and ignored. */
int oryon_pointdsc_load_param(oryon_pointdsc_t *handle, const char *name, const float *data_host, int64_t numel);
/* Fold eval-mode BatchNorm into the preceding conv, upload to the current device. */
int oryon_pointdsc_finalize(oryon_pointdsc_t *handle, void *stream);
size_t oryon_pointdsc_workspace_bytes(const oryon_pointdsc_t *handle, int B, int n_cap);
/* src,tgt [B, n_cap, 3] fp32 metres; n [B] int32 (rows actually used, <= n_cap); status_in [B] or NULL.
 * T [B,16] fp32 (identity for pairs that fail, as pipeline.py:341/350), labels [B,n_cap] uint8 or NULL,
 * status_out [B] int32 or NULL. */
int oryon_pointdsc_register(oryon_pointdsc_t *handle, const float *src, const float *tgt, const int32_t *n, int B,
                            int n_cap, const int32_t *status_in, void *workspace, size_t workspace_bytes, float *T,
                            uint8_t *labels, int32_t *status_out, void *stream);
/* Stage-level views for parity tests (same kernels as oryon_pointdsc_register):
 *   encode : corr features [B,n_cap,C] + confidence [B,n_cap]
 *   seeds  : NMS seeds [B, S_cap] int32 + n_seeds [B]
 *   hypotheses : given seeds, per-seed transforms [B,S_cap,16], fitness [B,S_cap], best [B]
 *   refine : post_refinement of given transforms */
int oryon_pointdsc_encode(oryon_pointdsc_t *handle, const float *src, const float *tgt, const int32_t *n, int B,
                          int n_cap, void *workspace, size_t workspace_bytes, float *feat, float *confidence,
                          void *stream);
int oryon_pointdsc_seeds(oryon_pointdsc_t *handle, const float *src, const float *confidence, const int32_t *n, int B,
                         int n_cap, int S_cap, int32_t *seeds, int32_t *n_seeds, void *stream);
int oryon_pointdsc_hypotheses(oryon_pointdsc_t *handle, const float *src, const float *tgt, const float *feat,
                              const int32_t *n, const int32_t *seeds, const int32_t *n_seeds, int B, int n_cap,
                              int S_cap, void *workspace, size_t workspace_bytes, float *seed_T, float *fitness,
                              int32_t *best, void *stream);
int oryon_pointdsc_refine(oryon_pointdsc_t *handle, const float *src, const float *tgt, const int32_t *n, int B,
                          int n_cap, const float *T_in, float *T_out, uint8_t *labels, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * RANSAC pose solver (test.solver = ransac): best_fit_transform_with_RANSAC (utils/geo6d.py:40-120) as pipeline.py:462-466 calls
 *         it (max_iter = 10000, fix_percent = 0.9999, match_err = 0.001), for B pairs, two kernels, no allocation, no synchronisation.
 * Hypothesis numbering: hypothesis 0 is best_fit_transform over all n rows; hypothesis k >= 1 is best_fit_transform over the four rows
 *         of draw k - 1.  Iterations evaluate hypotheses 0 .. max_iter - 1 (the reference makes the last draw and never evaluates it).
 *         count_k = number of rows with |R a + t - b| <= match_err, classified as float64 classifies them.  If some count_k exceeds
 *         fix_percent * n (float64 product) the FIRST such k is taken and the result is best_fit_transform over its inliers
 *         (exited = 1); otherwise the hypothesis of the largest count wins, lowest k on ties, without a refit.  If every count is 0 or
 *         n < 4 the 3x4 result is zero (T = rows of zeros over 0 0 0 1, as eye(4) with the zero matrix placed in it; winner = -1).
 * src,tgt [B, n_cap, 3] fp32 metres (n_cap <= 2048; rows >= n[b] are never read); n [B] int32; status_in [B] or NULL: pairs with a
 *         non-zero status get the identity and pass the status on, exactly as oryon_pointdsc_register does.
 * sample_idx [B, max_iter, 4] int32, rows in [0, n[b]) (row max_iter - 1 is unused), or NULL = device RNG: row k, column j is
 *         (rng_u32(seed, key, 3, 4 k + j) * (uint64_t) n) >> 32 with key = pair_key[b] (NULL: b), so results depend on the global pair
 *         index, never on sharding.
 * T [B,16] fp32; winner [B] or NULL: the chosen hypothesis, -1 = none; exited [B] or NULL; counts [B, max_iter] or NULL. */
size_t oryon_ransac_workspace_bytes(int B, int n_cap, int max_iter);
int oryon_ransac_register(const float *src, const float *tgt, const int32_t *n, int B, int n_cap, int max_iter, double match_err,
                          double fix_percent, const int32_t *sample_idx, uint64_t seed, const int64_t *pair_key,
                          const int32_t *status_in, void *workspace, size_t workspace_bytes, float *T, int32_t *winner,
                          int32_t *exited, int32_t *counts, int32_t *status_out, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Spectral pose solver (test.solver = spectral): no weights, no random numbers.  PointDSC's learned confidence and neighbour lists are
 *         replaced by spectral matching on the spatial-compatibility matrix and by second-order spatial compatibility (SC^2, Chen et
 *         al., CVPR 2022); seeds, per-seed power iteration, weighted Kabsch, scoring and refinement are PointDSC's kernels.  The
 *         definition, stage by stage (S1-S9), is the header comment of csrc/spectral.hip; in short, per pair:
 *         C_ij = | |s_i - s_j| - |t_i - t_j| | < inlier_threshold in float64 (bit-packed, zero diagonal); conf = the iterate after
 *         EXACTLY num_iterations steps v <- M v / (|M v| + 1e-6) from v = 1, M_ij = max(0, 1 - (|s_i - s_j| - |t_i - t_j|)^2 / sigma_d^2)
 *         in fp32 (no early exit: the bits do not depend on a near-tie); NMS seeds on conf, S = int(n ratio); the set of seed s = s, then
 *         the k' - 1 rows j != s of the highest C_sj popcount(row_s & row_j), ties by ascending j, k' = min(k, n - 1); the k' x k' matrix
 *         of M between its members; then PointDSC's hypotheses and its refinement with tau = inlier_threshold.
 * The defaults below are object-scale (metres) and come from one synthetic experiment (planted motions of a 0.3 m cube of points, 1 mm
 *         noise, 50-90 % outliers), not from real data.
 * No allocation, no synchronisation, no float atomics; every output is the same bytes in every run, batch position and stream. */
typedef struct {
    int num_iterations;     /* 10 (1..16): power-iteration steps of the confidence (exact) and cap of the per-seed iteration */
    float ratio;            /* 0.1: seeds = int(n * ratio) */
    float inlier_threshold; /* 0.01 */
    float sigma_d;          /* 0.01 */
    int k;                  /* 40 (2..63) */
    float nms_radius;       /* 0.02 */
} oryon_spectral_config_t;
/* 0 for unsupported shapes; supported: B >= 1, n_cap % 128 == 0, n_cap <= 2048, 2 <= k <= 63, 1 <= num_iterations <= 16 (and
 * 0 < ratio <= 1, positive thresholds). */
size_t oryon_spectral_workspace_bytes(const oryon_spectral_config_t *cfg, int B, int n_cap);
/* The contract of oryon_pointdsc_register: src,tgt [B,n_cap,3] fp32 metres (rows >= n[b] are never read); n [B] int32; status_in [B] or
 * NULL: pairs with a non-zero status get the identity and pass the status on; a pair without a seed (int(n ratio) == 0) or with n < 2
 * gets the identity and ORYON_PAIR_NO_CORR.  T [B,16] fp32, labels [B,n_cap] uint8 or NULL (inliers of the best hypothesis),
 * status_out [B] or NULL. */
int oryon_spectral_register(const oryon_spectral_config_t *cfg, const float *src, const float *tgt, const int32_t *n, int B, int n_cap,
                            const int32_t *status_in, void *workspace, size_t workspace_bytes, float *T, uint8_t *labels,
                            int32_t *status_out, void *stream);
/* The same kernels with every intermediate as an optional output (NULL = not wanted), S_cap = int(n_cap ratio) + 1:
 *   compat [B,n_cap,n_cap/32] uint32 (bit j & 31 of word j >> 5 of row i); conf [B,n_cap] (rows >= n: 0); seeds [B,S_cap], n_seeds [B];
 *   sets [B,S_cap,k] (entries >= k': -1); scores [B,S_cap,n_cap] int32 (0 at the seed and at columns >= n); Mmat [B,S_cap,k,k] (zero
 *   outside k' x k'); close [B,S_cap,num_iterations] int32: the per-seed closeness flags of the power iteration (the hypotheses use
 *   the first iteration at which every seed of the pair is close, else the last); seed_T [B,S_cap,16], fitness [B,S_cap], best [B]
 *   (-1: no seed), T0 [B,16] (the best hypothesis, before the refinement), T [B,16], status_out [B].  Of the per-seed outputs (seeds,
 *   sets, scores, Mmat, close, seed_T, fitness) only the first n_seeds[b] entries of pair b are specified. */
int oryon_spectral_stages(const oryon_spectral_config_t *cfg, const float *src, const float *tgt, const int32_t *n, int B, int n_cap,
                          const int32_t *status_in, void *workspace, size_t workspace_bytes, uint32_t *compat, float *conf,
                          int32_t *seeds, int32_t *n_seeds, int32_t *sets, int32_t *scores, float *Mmat, int32_t *close, float *seed_T,
                          float *fitness, int32_t *best, float *T0, float *T, int32_t *status_out, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Validation step: the contrastive terms of FeatureLoss.forward (losses.py:64-141) for B pairs in three launches, no allocation, no
 *         synchronisation, no float atomics (every output is bit-stable across runs, streams and batch shapes).  fp32 throughout, as the
 *         reference runs on the CPU; cosine in the matcher's form (rows / max(|x|, 1e-8), then a dot product).
 * feat_a, feat_q [B,C,FH,FW] fp32 (C <= 256); corrs [B,n_corr,4] int32 (y_a,x_a,y_q,x_q) in FEATURE-MAP pixels, i.e. after
 *         rescale_coords and the clamp of losses.py:77-78 (out-of-map values are clamped to the map); valid [B] int32: pairs whose value
 *         is not 1 do no work and write zeros (losses.py:158,189).
 * pool_mode 0, the hardest negative (losses.py:165-220): pool [B,2,n_pool] int32 linear pixel indices (side 0 = anchor map, 1 = query
 *         map: the torch_sample_select draw of losses.py:196-199), or NULL = every pixel of the map in row-major order.  The negative of
 *         positive n is the argmin over pool positions j of
 *             0.5 (1 - cos(pos[n], map[pool[j]])) + 1e6 relu(neg_kernel - sqrt(dy^2 + dx^2 + 1e-7))       (losses.py:205-211)
 *         in the reference's fp32 expression (correctly rounded sqrt, no contraction), lowest j on ties (torch.argmin); entries outside
 *         [0, FH*FW) never win.
 * pool_mode 1, loss.hard_negatives = False (losses.py:222-263): pool [B,2,n_corr] holds THE negative of every positive (the
 *         torch.randint draw of losses.py:254); no exclusion disc.
 * d_pos [B,n_corr] = 0.5 (1 - cos(pos_a, pos_q)) (losses.py:91); d_neg [B,2,n_corr] the same against the chosen negative
 *         (losses.py:92-93); neg_idx [B,2,n_corr] its linear pixel index (losses.py:214-218); pair_terms [B,3] = mean_n relu(d_pos -
 *         pos_margin), mean_n relu(neg_margin - d_neg) for the anchor and the query side (losses.py:95-101); losses [3] = their means
 *         over the pairs with valid == 1, zeros when there is none (losses.py:103-111). */
size_t oryon_feature_loss_workspace_bytes(int B, int n_corr, int n_pool);
int oryon_feature_loss(const float *feat_a, const float *feat_q, int B, int C, int FH, int FW, const int32_t *corrs, int n_corr,
                       const int32_t *valid, const int32_t *pool, int n_pool, int pool_mode, float pos_margin, float neg_margin,
                       float neg_kernel, void *workspace, size_t workspace_bytes, float *d_pos, float *d_neg, int32_t *neg_idx,
                       float *pair_terms, float *losses, void *stream);
/* The sums behind the dice mask loss (losses.py:40-62 with mask_type 'dice'; utils/losses/dice.py:27-89), one pass per image.
 * logits [B,H,W] fp32; gt [B,H,W] int32 at the logits' size (non-zero = object).  sums [B,4] float64 = sum p, sum p^2, sum p t, sum t
 *         with p = sigmoid(2 x), the softmax over (x, -x) of dice.py:69-78, by a fixed-order tree; mask [B,H,W] int32 = sigmoid(x) >
 *         threshold (losses.py:59, the expression of oryon_mask_from_logits); counts [B,2] int32 = |mask and gt|, |mask or gt|
 *         (utils/metrics.py:32-36). */
int oryon_mask_dice_sums(const float *logits, const int32_t *gt, int B, int H, int W, float threshold, double *sums, int32_t *mask,
                         int32_t *counts, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Training step: the backward pass of the two entries above (what torch autograd does to losses.py:64-141 and utils/losses/dice.py:27-89
 *         in the reference's training_step, pipeline.py:170-181).  Two launches and two memsets for the maps, one launch for a mask; no
 *         allocation, no synchronisation, no float atomics: the bytes of every output depend on the pair's inputs and on g alone.
 * Notation: eps = 1e-8, u^ = u / max(|u|, eps), d(u,v) = 0.5 (1 - <u^, v^>), V = number of pairs with valid == 1, N = n_corr.
 * g [3] fp32 ON THE DEVICE: the upstream gradients (g_pos, g_neg_a, g_neg_q) of the three entries of `losses`; never read by the host.
 * Cosine: for |u| >= eps, d<u^,v^>/du = (v^ - <u^,v^> u^) / |u|; for |u| < eps the clamped norm is a constant and d/du = v^ / eps
 *         without the projection term; a zero partner v has v^ = 0 and gives no gradient (torch's cosine_similarity, losses.py:91-93).
 * Margins: the relu subgradient is strict.  A row contributes through d_pos only if d_pos - pos_margin > 0 and through d_neg_s only if
 *         neg_margin - d_neg_s > 0, both subtractions in fp32 on the forward's own d_pos / d_neg (losses.py:95-101), so backward and
 *         forward never disagree about a row.  alpha_n = g_pos / (V N), beta_{s,n} = -g_neg_s / (V N) (the means of losses.py:95-111).
 * Negatives: neg_idx [B,2,N] (the forward's) is a constant, the argmin is not differentiated; the negative's descriptor is a gather
 *         from the same map, so gradient flows to its pixel.  An index outside [0, FH*FW) names no pixel: a zero row, no gradient.
 * Per pair b and side s, with u_n the side's positive, v_n the other side's positive, w_n the side's negative, 2 N slots:
 *         slot n     at the positive's pixel = alpha_n d d_pos/d u_n + beta_{s,n} d d(u_n,w_n)/d u_n  (added in that order)
 *         slot N + n at the negative's pixel = beta_{s,n} d d(u_n,w_n)/d w_n
 *         (each evaluated in float64 from the fp32 maps and rounded once to fp32).  grad_s[b,:,y,x] = the sum of the slots at that
 *         pixel in ascending slot order, in fp32; every other element is exactly 0; a pair with valid != 1 gets an all-zero map.
 * feat_a, feat_q, corrs, valid as oryon_feature_loss takes them (C <= 256, n_corr <= 4096); grad_a, grad_q [B,C,FH,FW] fp32.
 * workspace: oryon_feature_loss_grad_workspace_bytes(B, C, n_corr) bytes (the 2 N contribution vectors of every pair and side). */
size_t oryon_feature_loss_grad_workspace_bytes(int B, int C, int n_corr);
int oryon_feature_loss_grad(const float *feat_a, const float *feat_q, int B, int C, int FH, int FW, const int32_t *corrs, int n_corr,
                            const int32_t *valid, const int32_t *neg_idx, const float *d_pos, const float *d_neg, const float *g,
                            float pos_margin, float neg_margin, void *workspace, size_t workspace_bytes, float *grad_a, float *grad_q,
                            void *stream);
/* Backward of the dice mask loss (utils/losses/dice.py:27-89 with weight [0.5, 0.5] as losses.py:40-62 builds it) of B images.
 * logits, gt as oryon_mask_dice_sums takes them; sums [B,4] float64 = that call's output; g_mask [1] fp32 ON THE DEVICE.
 * With p = sigmoid(2x), q = 1 - p, u = 1 - t, D_f = S_pp + S_t + 1, D_b = S_qq + S_u + 1 (S_qq, S_u, S_qu from the four sums and H W):
 *     grad_logits_i = g_mask (0.25 / B) 2 p_i q_i [(-t_i / D_f + 2 p_i (S_pt + 1) / D_f^2) - (-u_i / D_b + 2 q_i (S_qu + 1) / D_b^2)]
 * evaluated in float64, stored as fp32, for all B images (validity does not enter).  grad_logits [B,H,W] fp32. */
int oryon_mask_dice_grad(const float *logits, const int32_t *gt, int B, int H, int W, const double *sums, const float *g_mask,
                         float *grad_logits, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * The whole batched step as ONE call (round 3): what the per-sample loop of FPM_Pipeline.test_step does for every pair of a batch
 * (pipeline.py:313-355: is_detection_valid -> get_featmap_corrs [utils/pcd.py:177-216] -> get_pose [pipeline.py:429-472:
 * scale / validate / lift, get_pointdsc_pose]), for B pairs, enqueued from C++ on streams and events the engine owns, over a
 * persistent arena the caller hands over once (the streams come from a per-device pool that lives as long as the process: every engine of
 * a process runs on the same four streams, so a re-created engine keeps the hardware queues of the first).  oryon_engine_submit issues,
 * without allocating or synchronising,
 *     gather stream : oryon_roi_compact x2, oryon_roi_subsample, oryon_gather_q8 x2                       (K0)
 *     match stream  : oryon_match_corrs_i8, oryon_lift_pairs                                               (K1s8 + K1b, K2)
 *     reg stream    : oryon_pointdsc_register                                                              (K3-K10)
 * with exactly the arguments oryon_amd/engine.py passes to those entry points, so results are identical bit for bit.  The K0
 * outputs alternate between two buffer sets, everything else a step produces between n_slots result slots, registrations between
 * two streams: K0 of step k+1 and the registrations of steps k-1, k-2 overlap the matching of step k.
 * Route: the screened lazy matcher (C <= 512, 0 < dist_th <= 0.5; descriptors narrower than 256 channels - the reference's own
 *          C = 32 @ 192^2, configs/config.yaml:34-35 - are zero-padded to the 256-channel operand rows by K0, which changes no result);
 *          wider descriptors / other thresholds stay with the per-call entry points.
 *
 * overlap: 0 = everything on the caller's stream (no engine streams), 1 = match on an engine stream, registration on one stream
 *          per slot, 2 = additionally K0 on its own stream (n_slots >= 2 for overlap >= 1).
 * Per-pair results live in the arena: oryon_engine_buffer gives offset / size of a slot's named buffer ("pose" [B,16] fp32,
 *          "status_out", "n_valid_out", "n_lift_out" [B] i32, "n_valid", "n_lift", "n_a", "n_q", "n_und" [B] i32, "corrs" [B,n_cap,4] i32, "pcd_a", "pcd_q"
 *          [B,n_cap,3] fp32, "roi_a", "roi_q" [B,FH*FW] i32, "min_dist", "argmin", "valid" [B,cap_a], ...); a slot's buffers are valid
 *          from oryon_engine_wait(slot) until the n_slots-th next submit.
 *          Slot lifetime, precisely: that submit orders the overwrite of "pose" / "status_out" / "n_valid_out" / "n_lift_out" (the
 *          protected block: written on the registration stream; the last two are the step's "n_valid" / "n_lift" copied there) after
 *          everything queued on caller_stream before it, whatever inputs_resident says.  K0 and the matcher overwrite the slot's OTHER buffers (ROI lists,
 *          counts, matcher outputs, correspondences, lifted points) without waiting for caller_stream when inputs_resident != 0: a
 *          caller that may still have reads of those queued when the slot comes round again passes inputs_resident = 0 for that submit.
 *          "corrs" rows >= the pair's n_sel are undefined (a re-used slot keeps an earlier step's rows there; K2 reads n_sel rows).
 * oryon_engine_submit returns the slot index (>= 0) or a negative error.  inputs_resident != 0: the inputs were complete before
 *          the call (nothing pending on caller_stream produces them), so K0 need not wait for the caller's stream.  The caller
 *          must not overwrite the inputs before oryon_engine_wait(slot, stream) has been passed on the stream that overwrites them.
 * Measurement: oryon_engine_set_timing(1) brackets the three sections and the screening kernel of every step with HIP events;
 *          oryon_engine_timing(step) (step = 0-based index of the submit, one of the last 64) -> {gather, match+lift, screening
 *          kernel, registration} durations in ms and the start / end of the match and registration sections relative to the start
 *          of the gather (valid once the step has completed).
 *          oryon_engine_host_stats: host time spent inside oryon_engine_submit.
 * Hardware queues: with overlap == 2 the engine owns four streams; the HIP runtime maps all streams of the process onto
 *          GPU_MAX_HW_QUEUES (default 4) hardware queues, and streams that share one execute in submission order.  Run the host
 *          process with GPU_MAX_HW_QUEUES >= 6 (the Python package sets 8 at import) or the two registration streams serialise. */
typedef struct oryon_engine oryon_engine_t;
typedef struct {
    int B, C, FH, FW;        /* pairs per step; descriptor maps [B,C,FH,FW] */
    int HA, WA, HQ, WQ;      /* depth maps [B,HA,WA] / [B,HQ,WQ] fp32 millimetres */
    int layout;              /* ORYON_LAYOUT_NCHW | ORYON_LAYOUT_NHWC */
    float dist_th;           /* test.dist_th (0.25) */
    int n_corrs;             /* test.n_corrs (500) */
    int src_sampling;        /* test.src_sampling (5000); 0 = keep every ROI pixel */
    uint64_t seed;
    int round_f16;           /* the reference's half-descriptor branch (utils/pcd.py:195-197) */
    int n_slots;             /* result slots: a step's results stay readable until the n_slots-th next submit (6; <= 8) */
    int overlap;             /* see above (2) */
    int gather_sets;         /* K0 output sets: K0 may run this many steps ahead of the matcher minus one (<= 4, <= n_slots).  2 is the Python binding's
                                default since round 5: a third set adds 3.4 ms of queueing to a step's latency (14.1 -> 10.7 ms at cfg2) and no throughput */
    int reg_streams;         /* registration streams the steps alternate over (2; <= 4) */
    int reg_lag;             /* > 0: the matcher of step k waits for the registration of step k - reg_lag (< n_slots); 0 = never (default) */
    int screen;              /* 0 = int8 screen (oryon_gather_q8 + oryon_match_corrs_i8_araw), 1 = MX-fp6 screen (oryon_gather_mx6 +
                                oryon_match_corrs_mx6_araw); steps submitted with force_eager take the int8 route on materialised fp32
                                anchor rows (oryon_match_corrs_i8); their K0 and that of the hard route (x3_prefetch below,
                                oryon_match_corrs_mx6_x3) are the only ones that write those rows */
    int sample_first;        /* 0 = off (default).  N > 0: the "sample first" schedule (see oryon_sample_first_gate): the matcher first
                                sees a uniformly random N-anchor subset per pair; pairs whose subset holds fewer than n_corrs valid rows are
                                redone on all anchors, gated on the device.  Same distribution of the sampled correspondences, not the same
                                sample as the default schedule; steps submitted with force_eager ignore it */
    int x3_prefetch;         /* 1 (default in the Python binding): when the steps that completed most recently left more than a quarter of their
                                anchors to the second level (n_und, read back through pinned memory without a synchronisation), K0 writes the
                                query rows' hi / lo halves in its own pass (oryon_gather_mx6_x3) and the matcher skips its second read of the maps
                                (oryon_match_corrs_mx6_x3).  Results are unchanged; C <= 256 and the MX-fp6 screen only.  0 = never */
    int stream_roles;        /* which of the device's eight pooled streams (numbered in creation order) serve as match / gather / registration 0 /
                                registration 1: four decimal digits, each 0..7.  0 = the library's default (2345).  The HIP runtime multiplexes a
                                process's streams onto a few hardware queues (the arbitration between them is undocumented; found by measurement):
                                the placement alone moves the pipelined step by up to 30 % at 64 pairs and 70 % at 16, and which placements
                                are good depends on what else the process created first (DESIGN.md "stream placement": the default is
                                the one that stayed within 2 % of the best both in a plain process and behind an RCCL communicator).  A
                                host calls oryon_engine_warm_streams() before it creates other streams, and measures the candidates on its
                                own process with oryon_engine_set_stream_roles (oryon_amd.engine.MatchPoseEngine.tune_stream_roles does).
                                Results never
                                depend on it */
    int screen_cascade;      /* 1 (default in the Python binding): on the default route of the MX-fp6 screen (C <= 256, three 1024-anchor panels or
                                more, not under sample_first) the matcher screens a probe of the anchors completely, learns per panel the band of
                                query tiles its matches lie in, settles the validity of the other anchors inside that band and scans completely
                                only the anchors left open and the sampled ones (DESIGN.md "default-route cascade").  Results are unchanged.
                                0 = the plain full screen.  (It stands in front of the solver fields, whose place at the end of the struct is
                                pinned; the matcher entries oryon_match_corrs_mx6[_araw] themselves always take the cascade where the shape has one) */
    int solver;              /* 0 = PointDSC (default: everything above), 1 = RANSAC: the registration stream calls oryon_ransac_register with
                                the step's pair_key and cfg.seed instead of oryon_pointdsc_register; oryon_engine_arena_bytes /
                                oryon_engine_create then accept a NULL PointDSC handle and the arena holds the RANSAC workspace in place of
                                PointDSC's.  Streams, slots and every other buffer are the same */
    int ransac_max_iter;     /* solver == 1: 10000 (pipeline.py:463) */
    float ransac_match_err;  /* 0.001.  The engine passes this float, widened, as oryon_ransac_register's double match_err: 0.001f is
                                0.0010000000475, not the double 0.001 (a caller that wants the engine's results from the entry point itself
                                passes the same rounded value; oryon_amd/engine.py does) */
    float ransac_fix_percent; /* 0.9999, widened the same way */
} oryon_engine_config_t;
size_t oryon_engine_config_bytes(void);      /* sizeof(oryon_engine_config_t) in the built library: a binding's mirror of the struct must match */
size_t oryon_engine_arena_bytes(const oryon_engine_config_t *cfg, const oryon_pointdsc_t *solver);
int oryon_engine_create(oryon_engine_t **handle, const oryon_engine_config_t *cfg, oryon_pointdsc_t *solver, void *arena,
                        size_t arena_bytes);
void oryon_engine_destroy(oryon_engine_t *handle);
/* Creates the current device's stream pool now (idempotent, thread-safe; every new stream runs one empty kernel, which binds its hardware
 * queue): call it once per process BEFORE anything else creates HIP streams on the device - torch.distributed.init_process_group("nccl",
 * device_id=...) creates RCCL's - so that the engine's streams are the process's first (run_test.py:31 launches one process per GPU).
 * That alone does not make every placement equally good behind a communicator (measured, see cfg.stream_roles): the default one is. */
int oryon_engine_warm_streams(void);
/* Re-assigns a live engine's streams (same digits as cfg.stream_roles; 0 = default).  Drains the engine's streams first (synchronises
 * the host with the steps in flight): a tuning aid for warm-up, not for the steady state.  oryon_engine_stream_roles reads the placement. */
int oryon_engine_set_stream_roles(oryon_engine_t *handle, int roles);
int oryon_engine_stream_roles(const oryon_engine_t *handle, int *roles);
int oryon_engine_buffer(const oryon_engine_t *handle, int slot, const char *name, size_t *offset, size_t *bytes);
int oryon_engine_geometry(const oryon_engine_t *handle, int *cap_a, int *cap_q, int *c_pad, int *n_cap);
/* feat_* [B,C,FH,FW] fp32 in cfg.layout; mask_* [B,FH*FW] int32 (== 1 selects); depth_* fp32; cam_* [B,9] fp32; pair_key [B] int64 or NULL */
int oryon_engine_submit(oryon_engine_t *handle, const float *feat_a, const float *feat_q, const int32_t *mask_a, const int32_t *mask_q,
                        const float *depth_a, const float *depth_q, const float *cam_a, const float *cam_q, const int64_t *pair_key,
                        int force_eager, int inputs_resident, void *caller_stream);
int oryon_engine_wait(oryon_engine_t *handle, int slot, void *caller_stream);
int oryon_engine_set_timing(oryon_engine_t *handle, int enable);
int oryon_engine_timing(oryon_engine_t *handle, int64_t step, float *out8);
/* ms from timing event `event_a` of step `step_a` to event `event_b` of step `step_b` (events per step: 0/1 gather begin / end,
 * 2/3 match + lift begin / end, 4/5 screening kernel begin / end, 6/7 registration begin / end): timelines across steps. */
int oryon_engine_elapsed(oryon_engine_t *handle, int64_t step_a, int event_a, int64_t step_b, int event_b, float *ms);
/* ms the two K0 gather launches (queries, anchors: the HBM-bound kernels of the matcher) of step `step` took, i.e. the gather section
 * without the ROI kernels in front of it (timing must have been on; the step must have completed) */
int oryon_engine_gather_ms(oryon_engine_t *handle, int64_t step, float *ms);
int oryon_engine_host_stats(const oryon_engine_t *handle, int64_t *n_submit, double *submit_ms_total, double *submit_ms_last);
/* number of submits so far whose K0 pass wrote the hi / lo rows (cfg.x3_prefetch) */
int oryon_engine_x3_steps(const oryon_engine_t *handle, int64_t *n_steps);
/* the default-route cascade of the most recent submit (cfg.screen_cascade), read-only, for tests and tuning: out[B][4] (host memory) =
 * per pair the probe rows, the rows settled inside their panel's band, the rows left open (scanned completely) and the band's query
 * tiles summed over the pair's live panels.  All zero when that submit took another route.  Synchronises the device. */
int oryon_engine_cascade_stats(oryon_engine_t *handle, int32_t *out);
/* the engine's own feedback, for callers that want the statistic without queueing reads of slot buffers (round 5): sums of the newest
 * COMPLETED step's per-pair counts of anchors the screen left to the second level ("n_und") and of anchors ("n_a") - the pinned-memory
 * copies the x3_prefetch decision is made from (MX-fp6 screen only).  *step = that step's submit index, -1 when none has completed yet.
 * Never waits: an event query per slot. */
int oryon_engine_feedback(oryon_engine_t *handle, int64_t *step, int64_t *n_undecided, int64_t *n_anchors);

/* B4  error-compensated fp16x3 linear layer for the frozen fp32 towers (CLIP ViT-L/14@336, Swin) of Oryon.forward
 *     (net.py:142-167, models/vlm.py:43-61; the reference evaluates them with fp32 torch linears):
 *         C[M,N] = act(A[M,K] * W[N,K]^T + bias[N]),   W = W_hi + W_lo (two fp16 matrices made once by oryon_split_f16x3)
 *     with every product accumulated as Ahi*Whi + Ahi*Wlo + Alo*Whi on the fp16 matrix pipe (fp32 accumulate): ~2^-22 relative, i.e.
 *     fp32-grade results at ~3x the fp32-MFMA rate.  act: 0 = none, 1 = QuickGELU x*sigmoid(1.702x) (CLIP), 2 = GELU x*Phi(x) with erf (Swin's nn.GELU), fused
 *     into the epilogue.
 *     K % 32 == 0, N % 256 == 0 (N % 128 == 0 when K >= 64), N * K < 2^30, |values| < 65504.
 *     W_lo == NULL (K >= 64 only) declares that every weight IS an fp16 value (its low half would be all zeros: what `clip.load` leaves in
 *     the reference's CLIPEncoder, models/vlm.py:19-22 - an fp16 checkpoint widened to fp32): the Ahi*Wlo products are left out, two
 *     instead of three MFMAs per product, results bit-identical to passing a zero W_lo. */
int oryon_split_f16x3(const float *x, int64_t n, void *hi_f16, void *lo_f16, void *stream);
/* Range check of the fp16x3 path (round 5; per stream since round 6).  The PRODUCERS of every tensor the fp16x3 kernels split - the B4
 * linear (both kernels; the in-place residual form checks its own finished sum, and the residual value its atomics leave in C is
 * checked by the fused residual-add + LayerNorm pass that reads it next, oryon_add_layernorm_f32), the 24 x 24 and decoder
 * convolutions / up-convolutions - OR 1 into a flag word when one of their finished values is not a finite value below
 * 60000 in magnitude: that is what an operand beyond float16's range (|x| >= 65520: hi = inf) produces in every product it enters, and
 * what an output that the NEXT kernel could not split looks like.  The attention kernels (B5, the Swin / fusion window attentions) and
 * the single-slab persistent decoder convolutions carry no check of their own: their q | k | v operands are outputs of checked linears
 * (an overflowing operand has raised the flag already, and their own outputs are convex combinations of checked v rows), the
 * convolutions' inputs are checked up-convolution outputs and GroupNorm-normalised maps, and whatever they produce goes through a
 * checked linear / convolution next (tests/test_backbone_pins.py::test_fp16x3_overflow_behind_an_unchecked_kernel_is_flagged_by_the_next executes
 * that argument).
 * The word belongs to (device, stream): a launch raises the word of the stream it runs on, oryon_x3_range_flag(stream) reads that word
 * after everything queued on `stream` (synchronises that stream: once per forward, not per layer) and clears it when reset != 0;
 * value_out == NULL only queues the clear (and allocates the device's flag table at the first call - make that call at initialisation so
 * that no launch allocates, e.g. under graph capture).  Forwards on different streams, threads or model instances do not see each
 * other's flags.  oryon_amd.net.Oryon.forward clears its stream's word before the forward, reads it after, and re-evaluates a flagged
 * forward with the fp32 torch modules. */
int oryon_x3_range_flag(int *value_out, int reset, void *stream);
int oryon_linear_f16x3(const float *A, int M, int K, const void *W_hi, const void *W_lo, const float *bias, int N, int act, float *C,
                       void *stream);
/* C[M,N] += A W^T + bias (no activation; K >= 64, N % 128 == 0, N * K < 2^30): the towers' residual update x = x + linear(h)
 * (clip's ResidualAttentionBlock: x + attn(ln_1(x)), x + mlp(ln_2(x)); torchvision's SwinTransformerBlock the same) done by the linear
 * itself - every element of C receives ONE fire-and-forget fp32 atomic add of its finished sum, i.e. exactly the rounding of the separate
 * add, in a fixed order (no two lanes touch the same element) - so that the LayerNorm pass which follows reads one tensor, not two.
 * C must not alias A. */
int oryon_linear_f16x3_acc(const float *A, int M, int K, const void *W_hi, const void *W_lo, const float *bias, int N, float *C,
                           void *stream);

/* B5  multi-head self-attention of the frozen CLIP image tower (clip's ResidualAttentionBlock.attention reached through
 *     models/vlm.py:46-56; nn.MultiheadAttention without mask) in fp32-grade arithmetic on the fp16 matrix pipe (both products
 *     error-compensated like B4, flash-style, fp32 softmax): qkv [N, L, 3*heads*64] fp32 = the in_proj output, out [N, L, heads*64]. */
int oryon_mha_f16x3(const float *qkv, int N, int L, int heads, int head_dim, float *out, void *stream);

/* f3  pose-accuracy metrics on the device for a batch of pairs.
 *     Replaces utils/metrics.py:194-220 (compute_add / compute_adds, with the FLOAT16 model transform of utils/pcd.py:127-133) and
 *     utils/metrics.py:222-259 (compute_RT_distances) of the reference's evaluator (utils/evaluator.py:206-256).
 * pred_pose / gt_pose [B,16] row-major 4x4 (metres); model_pts [sum M, 3] fp32 (metres) with pts_offset [n_models+1] (prefix sums) and
 * model_of_pair [B] (NULL: every pair uses model 0); max_pts = largest model; workspace [B,2] fp32.
 * out [B,4] = (ADD, ADD-S, rotation error in degrees, translation error in centimetres). */
int oryon_pose_metrics(const float *pred_pose, const float *gt_pose, int B, const float *model_pts, const int32_t *pts_offset, int n_models,
                       int max_pts, const int32_t *model_of_pair, float *workspace, float *out, void *stream);

/* f3  the BOP errors the reference's evaluator reports next to ADD(-S): MSSD (maximum symmetry-aware surface distance, millimetres)
 *     and MSPD (maximum symmetry-aware projection distance, pixels) for a batch of pairs.
 *     Replaces utils/evaluator.py:258-275 (both poses rounded to FLOAT16, translation = half(t) * 1000 in half arithmetic) +
 *     bop_toolkit_lib/pose_error.py:370-427 (my_mssd, my_mspd: float64 arithmetic on the rounded poses).
 * pred_pose / gt_pose [B,16] float64 row-major 4x4 (metres; float64 so that the half rounding sees the caller's values, whatever their
 * type); K [B,9] float64 (the query camera); model_pts_mm [sum M, 3] float64 MILLIMETRES (what the evaluator holds) with pts_offset
 * [n_models+1]; syms [sum S, 12] float64 = the models' symmetry sets as row-major 3x4 [R|t] (bop_toolkit_lib/misc.py:43-90,
 * format_sym_set :402-411; the identity included) with sym_offset [n_models+1]; max_syms = largest set; model_of_pair [B] or NULL.
 * max_points: 3 = what the reference computes (its np_transform, pose_error.py:339-352, slices `pts[:, :3]` on the POINT axis of a
 * [1,N,3] array, so my_mssd / my_mspd see the first three model points only); 0 = every point (the BOP definition).
 * workspace: oryon_pose_bop_workspace_bytes(B, max_syms).  out [B,2] float64 = (MSSD error, MSPD error). */
size_t oryon_pose_bop_workspace_bytes(int B, int max_syms);
int oryon_pose_bop_errors(const double *pred_pose, const double *gt_pose, const double *K, int B, const double *model_pts_mm,
                          const int32_t *pts_offset, const double *syms, const int32_t *sym_offset, int n_models, int max_syms,
                          const int32_t *model_of_pair, int max_points, double *workspace, double *out, void *stream);

/* f3  depth render of triangle meshes for N images (image = pose x camera x model) of one size H x W.
 *     Replaces bop_toolkit_lib/renderer_vispy.py:512-617 (render_object(..)['depth']: the OpenGL depth pass of the reference's VSD,
 *     which needs vispy + EGL + a GL driver) with a rasteriser whose arithmetic is DEFINED (csrc/vsd.hip header) and restated
 *     in numpy (oryon_amd/evaluation.py rasterize_depth): both give the same bits.
 * pose [N,16] fp32 row-major 4x4 (rotation, translation in MILLIMETRES); K [N,9] fp32 (fx = K[0], cx = K[2], fy = K[4], cy = K[5] are
 * read); verts_mm [sum V,3] fp32 with vert_offset [n_models+1]; faces [sum F,3] int32, zero-based and local to their model, with
 * face_offset [n_models+1]; max_faces = largest model; model_of_image [N] or NULL (every image shows model 0).
 * Output pixel (row r, column c) samples the projection at (u, v) = (c + 0.5, r + 0.5); both windings are drawn, the nearest surface
 * wins, background 0, depth = eye-space Z in millimetres, perspective-correct.  A triangle with a vertex at Z <= 0 (or further than 2^15
 * pixels from the origin) is dropped whole - no near-plane clipping; the reference's 16 / 24-bit z-buffer quantisation is not
 * reproduced.  workspace: oryon_render_depth_workspace_bytes(N, max_faces); its first two uint32 hold, after the call, the number of
 * triangles drawn by the one-wave-per-triangle route and by the one-thread-per-triangle route.  depth [N,H,W] fp32. */
size_t oryon_render_depth_workspace_bytes(int N, int max_faces);
int oryon_render_depth(const float *pose, const float *K, int N, const float *verts_mm, const int32_t *vert_offset, const int32_t *faces,
                       const int32_t *face_offset, int n_models, int max_faces, const int32_t *model_of_image, int H, int W, void *workspace,
                       float *depth, void *stream);

/* f3  the integer counts behind VSD for B pairs: renders the model at the estimated and at the ground-truth pose (as oryon_render_depth)
 *     and counts, against the test depth image, the pixels of the two bop19 visibility masks.
 *     Replaces utils/evaluator.py:263-266 + :281-283 (float16 pose rounding, the call) and bop_toolkit_lib/pose_error.py:17-93 (vsd,
 *     'step' cost, normalised by the diameter), misc.py:143-163 (depth_im_to_dist_im_fast, float64) and visibility.py (bop19, the
 *     difference taken in fp32).
 * pred_pose / gt_pose [B,16] float64 (metres; rounded to float16 inside like oryon_pose_bop_errors); K [B,9] float64; depth_test
 * [B,H,W] fp32 millimetres (0 = no measurement); mesh arguments as oryon_render_depth, model_of_pair [B] or NULL; diameter_mm [B]
 * float64; delta (millimetres; compared in fp32); taus [n_tau] float64, n_tau <= 16.
 * workspace: oryon_vsd_workspace_bytes(B, H, W, max_faces).  counts [B, 2 + n_tau] int32 = (n_union, n_inter, n_cost[tau]...); the
 * error at tau is (n_cost + n_union - n_inter) / n_union, or 1 when n_union is 0. */
size_t oryon_vsd_workspace_bytes(int B, int H, int W, int max_faces);
int oryon_vsd_counts(const double *pred_pose, const double *gt_pose, const double *K, const float *depth_test, int B, int H, int W,
                     const float *verts_mm, const int32_t *vert_offset, const int32_t *faces, const int32_t *face_offset, int n_models,
                     int max_faces, const int32_t *model_of_pair, const double *diameter_mm, double delta, const double *taus, int n_tau,
                     void *workspace, int32_t *counts, void *stream);

/* g1  ground-truth pixel correspondences of B RGB-D pairs with known poses (csrc/gt_corrs.hip): what the reference's data-preparation
 *     scripts store as annots.pkl 'corrs'.  Replaces scripts/data/make_toyl_test.py:47-85 + :175-243 (make_nocs_test.py alike): lift the
 *     object's pixels of both views (utils/data/toyl.py:237-278 get_pcd + filter_pcd over utils/pcd.py:44-74), move the anchor cloud by
 *     pose_q @ inv(pose_a), torch.cdist in float64 (a 20 000 x 20 000 matrix, 3.2 GB), amin / argmin, min_dist <= threshold.
 * DEFINITION.  All arithmetic is float64 without contraction, sums left to right, unless noted; tests/gt_corrs_restatement.py is the
 * same sequence of correctly rounded operations in numpy and agrees bit for bit.
 *   lift       pixel p of the list -> y = p / W, x = p % W, z = double(depth[p]) (fp32 millimetres),
 *              X = (double(fp32(x) - fp32(cx)) * z) / fx / 1000,  Y = (double(fp32(y) - fp32(cy)) * z) / fy / 1000,  Z = z / 1000.
 *              The difference is an fp32 one: the reference's xmap / ymap are float32 tensors and cx / cy 0-dim float64 tensors, which
 *              torch's promotion leaves in float32 (an all-float64 lift differs by up to 1.7e-5 mm).  fx = cam9[0], cx = cam9[2],
 *              fy = cam9[4], cy = cam9[5].  A zero-depth pixel lifts to the origin and is KEPT, as in the reference; a list entry
 *              outside [0, H W) reads no depth and lifts like a zero-depth pixel (0, 0).
 *   transform  anchor side only: p' = ((R0 x + R1 y) + R2 z) + t per coordinate, pose_aq [B,12] float64 = the rows [R | t] of
 *              pose_q @ inv(pose_a), translation in metres (formed by the caller, in numpy, as make_toyl_test.py:212 does).
 *   nearest    for every anchor row i: d2_j = ((dx dx + dy dy) + dz dz) over the query rows j = 0 .. n_q - 1, idx_i = the FIRST minimiser
 *              (lowest j on ties: torch.argmin), d2_i its value.  A NaN distance never wins; idx = -1, d2 = +inf when no row compares
 *              below +inf (n_q = 0).  The reference's cdist uses the matmul form above 25 rows; the two can differ in the last bits of
 *              a distance, never in an index unless two candidates lie within ~1e-12 (relative) of each other.
 *   keep       row i is kept when sqrt(d2_i) <= threshold; kept rows are written in anchor (list) order as (y_a, x_a, y_q, x_q).
 * The reference's draws (at most 20 000 points per side, at most max_corrs kept rows; torch.multinomial) are the caller's: the lists
 * arrive already drawn, in drawn order (oryon_amd/pairs.py).
 * Counts n [B] are DEVICE arrays; a count above its capacity is read as the capacity and rows beyond the count are never read.
 * float64 pointers must be 8-byte aligned.  No entry allocates, synchronises or uses atomics: outputs are bit-stable.
 *
 * oryon_gtc_lift: the lift (+ transform when pose is not NULL) alone.  depth [B,H,W] fp32; pix [B,cap] int32; cam9 [B,9] float64 ->
 *   xyz [B,cap,3] float64 metres, yx [B,cap,2] int32 (rows < n[b] written).
 * oryon_pcd_nearest_f64: the nearest stage alone.  src [B,cap_src,3], dst [B,cap_dst,3] float64 -> idx [B,cap_src] int32,
 *   d2 [B,cap_src] float64 (rows < n_src[b] written).
 * oryon_gt_corrs: the whole routine.  depth_a [B,HA,WA], depth_q [B,HQ,WQ]; pix_a [B,cap_a], pix_q [B,cap_q]; cam_a, cam_q [B,9];
 *   threshold in metres (>= 0); status_in [B] or NULL: a pair with a non-zero status is skipped and gets n_corr = 0.
 *   workspace: oryon_gt_corrs_workspace_bytes(B, cap_a, cap_q) bytes (0 = unsupported shape), 256-byte aligned.
 *   corrs [B,cap_a,4] int32 (rows < n_corr[b] written), n_corr [B]; idx / d2 [B,cap_a] or NULL: the nearest stage's outputs. */
int oryon_gtc_lift(const float *depth, int B, int H, int W, const int32_t *pix, const int32_t *n, int cap, const double *cam9,
                   const double *pose, double *xyz, int32_t *yx, void *stream);
int oryon_pcd_nearest_f64(const double *src, const int32_t *n_src, const double *dst, const int32_t *n_dst, int B, int cap_src,
                          int cap_dst, int32_t *idx, double *d2, void *stream);
size_t oryon_gt_corrs_workspace_bytes(int B, int cap_a, int cap_q);
int oryon_gt_corrs(const float *depth_a, const float *depth_q, int B, int HA, int WA, int HQ, int WQ, const int32_t *pix_a,
                   const int32_t *n_a, int cap_a, const int32_t *pix_q, const int32_t *n_q, int cap_q, const double *cam_a,
                   const double *cam_q, const double *pose_aq, double threshold, const int32_t *status_in, void *workspace,
                   size_t workspace_bytes, int32_t *corrs, int32_t *n_corr, int32_t *idx, double *d2, void *stream);

/* g2  ICP pose refinement of B pairs of object clouds (csrc/icp.hip; test.refine = icp): the reference's utils/geo6d.py:157-208 `icp`
 *     over nearest_neighbor (:22-38, sklearn's NearestNeighbors) and best_fit_transform_icp (:122-155), batched, with nothing read back.
 * DEFINITION.  For each pair: a source cloud src [n_s,3] and a target cloud dst [n_d,3], float64 metres, of ANY two sizes (the
 * reference asserts equal sizes but does not need them); an initial pose T_0 [4,4], which arrives as fp32 and is widened; max_iter,
 * tolerance and max_dist (+inf = the reference's behaviour).  All arithmetic is float64 without contraction;
 * tests/icp_restatement.py is its numpy statement.  State: T_k, prev = 0.0, not done.  For k = 0 .. max_iter - 1, while not done:
 *   1 move      s_i = ((R0 x + R1 y) + R2 z) + t per coordinate, [R | t] of T_k, applied to src_i.
 *   2 nearest   d2_ij = ((dx dx + dy dy) + dz dz); j_i = the FIRST minimiser over j ascending (strict <; a NaN never wins, and a row
 *               whose every distance is NaN has no neighbour, j_i = -1); dist_i = sqrt(d2_i).
 *   3 keep      row i is kept when it has a neighbour and dist_i <= max_dist; m = the number kept.  m < 3 (or n_d = 0): the pair is
 *               done and T_k stays.  Otherwise mean_k = the mean of dist_i over the kept rows.
 *   4 fit       dT = best_fit_transform_icp(s_kept, dst[j]_kept): plain means c_s, c_d as centroids, H = sum (s - c_s)(d - c_d)^T,
 *               R = V diag(1, 1, det(V U^T)) U^T for H = U S V^T, t = c_d - R c_s.
 *   5 update    T_{k+1} = dT T_k.
 *   6 converge  |prev - mean_k| < tolerance: the pair is done, with this iteration's update applied (as in the reference); otherwise
 *               prev = mean_k.
 * The result is T_K.  The reference carries the moved cloud along and ends with best_fit_transform_icp(A, moved A); as the moved
 * cloud is a rigid image of A the two agree to rounding (tests/golden/icp_*.npz: 3.4e-15) - provided T_0 is rigid: the reference's last
 * fit returns the nearest rigid transform, so it differs from T_K by as much as an fp32-rounded T_0 is off a rigid one (~6e-8).
 * A pair with status_in != 0, n_s < 3 or n_d = 0 returns T_0 unchanged with iters = 0.
 * The ORDER of the sums over rows is not part of the definition, but it is fixed (rows of a 256-row block by an xor butterfly in each
 * wave, waves then blocks ascending; moments taken about the target's centroid): no float atomics, outputs bit-stable across runs,
 * streams and batch position.  Against the restatement the pose agrees to ~1e-13 (bar 1e-9), indices and iters exactly
 * wherever best and second-best neighbour and |prev - mean| and the tolerance are further apart than rounding.
 *
 * oryon_icp_refine: src [B,cap_src,3], dst [B,cap_dst,3] float64; n_src, n_dst [B] DEVICE counts: a count above its capacity is read
 *   as the capacity (below 0 as 0) and rows beyond the count are never read.  1 <= cap_src, cap_dst <= ORYON_ICP_MAX_ROWS, B <= 65535,
 *   1 <= max_iter <= ORYON_ICP_MAX_ITER (two launches per iteration, all enqueued at once; a finished pair's workgroups return at
 *   once), tolerance >= 0, max_dist >= 0.  T_init [B,16] fp32 row-major 4x4.  status_in [B] or NULL.
 *   workspace: oryon_icp_workspace_bytes(B, cap_src, cap_dst) bytes (0 = unsupported shape), 256-byte aligned
 *     = align256(B * ORYON_ICP_STATE_BYTES) + align256(B * ceil(cap_src / 256) * 17 * 8).
 *   T [B,16] fp32: rows 0-2 exactly float32(T64), row 3 T_init's.  T64 [B,12] float64 rows of [R | t], or NULL.  iters [B]: updates
 *   applied.  mean_err [B]: mean_k of the last update applied (0.0 when none).  n_kept [B]: m of the last executed iteration (0 when
 *   none).  idx [B,cap_src] or NULL: the last executed iteration's neighbours, -1 for a row without one, beyond n_s or of a pair
 *   that never iterated.  status_out [B] = status_in (0 when NULL).  float64 pointers must be 8-byte aligned. */
#define ORYON_ICP_MAX_ROWS 8192
#define ORYON_ICP_MAX_ITER 1000
#define ORYON_ICP_STATE_BYTES 136
size_t oryon_icp_workspace_bytes(int B, int cap_src, int cap_dst);
int oryon_icp_refine(const double *src, const int32_t *n_src, int cap_src, const double *dst, const int32_t *n_dst, int cap_dst, int B,
                     const float *T_init, int max_iter, double tolerance, double max_dist, const int32_t *status_in, void *workspace,
                     size_t workspace_bytes, float *T, double *T64, int32_t *iters, double *mean_err, int32_t *n_kept, int32_t *idx,
                     int32_t *status_out, void *stream);
/* oryon_icp_best_fit: step 4 alone over the CALLER's correspondences (best_fit_transform_icp, geo6d.py:122-155): row i of A [B,cap,3]
 *   corresponds to row i of Bp [B,cap,3], float64, n [B] device counts -> T [B,16] fp32 (= float32(T64), last row 0 0 0 1), T64 [B,12] or
 *   NULL, fitted [B] = 1, or 0 with the identity when n < 3; mean_err [B] = the mean distance of the pairs BEFORE the fit.  One
 *   iteration of the same kernels with the neighbour search replaced by j_i = i.  workspace: oryon_icp_workspace_bytes(B, cap, cap). */
int oryon_icp_best_fit(const double *A, const double *Bp, const int32_t *n, int cap, int B, void *workspace, size_t workspace_bytes, float *T,
                       double *T64, int32_t *fitted, double *mean_err, void *stream);

/* g3  Point-to-plane ICP of B source clouds onto the queries' depth maps (csrc/icp_plane.hip; test.refine = icp_plane): projective
 *     association and a point-to-plane error.  The target is never a loose cloud here but an organised depth map, so a normal is two
 *     central differences and the neighbour of a moved source point is the pixel it projects to: no search, O(n) per iteration.
 * DEFINITION.  All arithmetic is float64 without contraction; only + - * / sqrt (and floor) are used, so the device and
 * tests/icp_plane_restatement.py, its numpy statement, differ by the order of the sums over rows alone.  Per pair: a source cloud
 * src [n_s,3] float64 metres (the anchor's object cloud); the target as an organised map, depth [H,W] fp32 millimetres, mask [H,W] int32
 * (1 = object) and cam9 float64 (fx = cam9[0], cx = cam9[2], fy = cam9[4], cy = cam9[5]); T_0, fp32 4x4, widened; max_iter, tolerance,
 * max_dist and normal_jump, the last two in metres.  The lift V(x, y) of pixel (x, y) with depth z is exactly g1's:
 *   X = ((double(float(x) - float(cx)) z) / fx) / 1000, Y alike with (y, cy, fy), Z = z / 1000.
 * State: T_k, prev = 0.0, not done.  The origin o is the mean of the source rows moved by T_0 (a non-finite coordinate counts as 0),
 * computed once: the 6 x 6 system is formed about it, which keeps it well conditioned at coordinates around 1 m.  A pair with
 * status_in != 0 or n_s < 6 returns T_0 with iters = 0.  For k = 0 .. max_iter - 1, while not done:
 *   1 move       s = ((R0 x + R1 y) + R2 z) + t per coordinate, [R | t] of T_k.
 *   2 associate  the row is dropped unless s.z > 0.  u = (fx s.x) / s.z + cx, v = (fy s.y) / s.z + cy, px = floor(u + 0.5),
 *                py = floor(v + 0.5).  Dropped unless 1 <= px <= W - 2, 1 <= py <= H - 2, mask[py,px] == 1 and depth[py,px] > 0.
 *   3 normal     each of the four neighbours (px +- 1, py), (px, py +- 1) must have depth > 0 and |z_nb - z_c| <= normal_jump * 1000,
 *                otherwise the row is dropped.  a = V(px+1,py) - V(px-1,py), b = V(px,py+1) - V(px,py-1), c = a x b,
 *                l = sqrt((cx^2 + cy^2) + cz^2); dropped unless l > 0 and finite; n = c / l.  Nothing below depends on the sign of n.
 *   4 gate       d = V(px,py), e = s - d, dist = sqrt((ex^2 + ey^2) + ez^2); the row is kept when dist <= max_dist; m rows are kept.
 *                m < 6: the pair is done and T_k stays.
 *   5 sums       r = (nx ex + ny ey) + nz ez, J = [(s - o) x n, n]; A = sum J J^T (21 unique sums), g = sum J r (6), sum |r| and the
 *                count: 29 sums.  mean_k = sum |r| / m.
 *   6 solve      A x = -g by an unblocked Cholesky written out in a fixed order (column j: d = A_jj - sum_{q<j} L_jq^2, q ascending;
 *                L_ij = (A_ij - sum_{q<j} L_iq L_jq) / L_jj; forward then backward substitution, each sum ascending).  A pivot d
 *                that is not > 1e-12 max_i A_ii: the pair is done and T_k stays.  omega = x[0:3], v = x[3:6].  The rotation is the
 *                Cayley map - no sin, no cos: a = omega / 2, R = I + 2 / (1 + a.a) ([a]x + [a]x^2) with [a]x^2 = a a^T - (a.a) I.
 *                dT: p -> R (p - o) + o + v, i.e. t = (o - R o) + v; T_{k+1} = dT T_k.  |prev - mean_k| < tolerance: the pair is
 *                done, with this update applied (as g2 does); otherwise prev = mean_k.
 * The ORDER of the sums over rows is not part of the definition, but it is fixed exactly as g2's is: no atomics, outputs bit-stable
 * across runs, streams and batch position.
 *
 * oryon_icp_plane_refine: src [B,cap_src,3] float64; n_src [B] DEVICE counts (above the capacity: read as the capacity; rows beyond the
 *   count are never read); depth [B,H,W] fp32, mask [B,H,W] int32, cam9 [B,9] float64; T_init [B,16] fp32; status_in [B] or NULL.
 *   1 <= cap_src <= ORYON_ICP_MAX_ROWS, 1 <= max_iter <= ORYON_ICP_MAX_ITER (two launches per iteration, all enqueued at once; a
 *   finished pair's workgroups return at once), B <= 65535, H, W >= 3, H W < 2^31, tolerance, max_dist, normal_jump >= 0.
 *   workspace: oryon_icp_plane_workspace_bytes(B, cap_src) bytes (0 = unsupported shape), 256-byte aligned
 *     = align256(B * ORYON_ICP_STATE_BYTES) + align256(B * ceil(cap_src / 256) * ORYON_ICP_PLANE_REC * 8).
 *   Outputs as oryon_icp_refine's: T [B,16] fp32, rows 0-2 exactly float32(T64), row 3 T_init's; T64 [B,12] or NULL; iters [B] updates
 *   applied; mean_err [B] mean_k of the last update applied (0.0 when none); n_kept [B] m of the last executed iteration; idx
 *   [B,cap_src] or NULL: py W + px of the last executed iteration for a kept row, -1 otherwise; status_out [B] = status_in (0 when
 *   NULL).  float64 pointers must be 8-byte aligned. */
#define ORYON_ICP_PLANE_REC 29
size_t oryon_icp_plane_workspace_bytes(int B, int cap_src);
int oryon_icp_plane_refine(const double *src, const int32_t *n_src, int cap_src, const float *depth, const int32_t *mask, int H, int W,
                           const double *cam9, int B, const float *T_init, int max_iter, double tolerance, double max_dist,
                           double normal_jump, const int32_t *status_in, void *workspace, size_t workspace_bytes, float *T, double *T64,
                           int32_t *iters, double *mean_err, int32_t *n_kept, int32_t *idx, int32_t *status_out, void *stream);

/* g4  Depth-consistency verification of K candidate poses per pair (csrc/pose_verify.hip; test.verify): every source point, moved by a
 *     candidate, is classified against the query's depth map, and the candidate the measurements agree with most is selected.  It
 *     needs no ground truth and no mesh.  The reference has no counterpart.
 * DEFINITION.  All arithmetic is float64 without contraction; only + - * / and floor are used and NO sum over rows is formed in floating
 * point, so the device and tests/pose_verify_restatement.py, its numpy statement, agree EXACTLY in every output.  Per pair: a source
 * cloud src [n_s,3] float64 metres (the anchor's object cloud, anchor camera frame); the target as in g3: depth [H,W] fp32 millimetres,
 * mask [H,W] int32 (1 = object), cam9 float64 (fx = cam9[0], cx = cam9[2], fy = cam9[4], cy = cam9[5]); K candidate poses, fp32 4x4,
 * widened, of which only rows 0-2 are read; tol in metres.  Every source row gets, for every candidate, exactly one class, decided by
 * these tests in this order; a comparison is exactly as written, and a NaN fails every comparison:
 *   0 BEHIND     s = ((R0 x + R1 y) + R2 z) + t per coordinate (g3 step 1); BEHIND unless s.z > 0.
 *   1 OUTSIDE    u = (fx s.x) / s.z + cx, v = (fy s.y) / s.z + cy, px = floor(u + 0.5), py = floor(v + 0.5) (g3 step 2); OUTSIDE unless
 *                0 <= px <= W - 1 and 0 <= py <= H - 1, tested in float64 before any conversion to an integer: no read leaves the map.
 *                The whole image is valid here, not g3's window without the one-pixel border.
 *   2 UNKNOWN    z = depth[py,px]; UNKNOWN unless 0 < z < +inf.
 *   3 OCCLUDED   d = s.z - double(z) / 1000; OCCLUDED when d > tol: the point lies behind the measured surface (self-occlusion or an
 *                occluder).  Neutral.
 *   4 VIOLATION  -d > tol: the point floats in front of a surface the sensor saw - free space violated.
 *   5 OFF        otherwise, and mask[py,px] != 1: agrees with the depth, but not on the object.
 *   6 HIT        otherwise, and mask[py,px] == 1.
 * counts[k][c] = the number of rows of class c under candidate k; the counts of a candidate sum to n_s.
 * SELECTION, in integers only: best = the candidate with the largest counts[k][HIT]; ties go to the smallest
 * counts[k][BEHIND] + counts[k][VIOLATION] + counts[k][OFF], then to the smallest k.  A pair with status_in != 0 gets all counts 0,
 * cls = -1 and best = 0; a pair with n_s = 0 gets the same counts and best = 0.  (The score a caller reports, counts[HIT] / max(n_s, 1),
 * is formed outside: the candidates of a pair share n_s, so the selection never divides.)
 *
 * oryon_pose_verify: src [B,cap_src,3] float64; n_src [B] DEVICE counts, read as in g3 (above the capacity: the capacity; below 0: 0;
 *   rows beyond the count are never read); depth [B,H,W] fp32, mask [B,H,W] int32, cam9 [B,9] float64; poses [B,K,16] fp32; status_in [B]
 *   or NULL.  1 <= K <= ORYON_POSE_VERIFY_MAX_POSES, 1 <= cap_src <= ORYON_ICP_MAX_ROWS, 0 <= B <= 65535 (B == 0: nothing to do, returns
 *   ORYON_OK), H, W >= 1, H W < 2^31, tol >= 0 (a NaN is rejected).  Every check precedes every launch and every dereference.
 *   workspace: oryon_pose_verify_workspace_bytes(B, cap_src, K) bytes (0 = unsupported shape), 256-byte aligned
 *     = align256(B * ceil(cap_src / 256) * K * ORYON_POSE_VERIFY_CLASSES * 4).
 *   Outputs: counts [B,K,7] int32; best [B] int32; cls [B,K,cap_src] int32 or NULL: the class of every row under every candidate, -1
 *   beyond the pair's count (and everywhere for a pair with status_in != 0).  Two launches, no atomics, nothing read back: outputs are
 *   identical bytes across runs, streams and batch position.  float64 pointers must be 8-byte aligned. */
#define ORYON_POSE_VERIFY_CLASSES 7
#define ORYON_POSE_VERIFY_MAX_POSES 16
size_t oryon_pose_verify_workspace_bytes(int B, int cap_src, int K);
int oryon_pose_verify(const double *src, const int32_t *n_src, int cap_src, const float *depth, const int32_t *mask, int H, int W,
                      const double *cam9, int B, const float *poses /* [B,K,16] */, int K, double tol, const int32_t *status_in,
                      void *workspace, size_t workspace_bytes, int32_t *counts /* [B,K,7] */, int32_t *best /* [B] */,
                      int32_t *cls /* [B,K,cap_src] or NULL: class per row, -1 beyond the count */, void *stream);

/* h1  Mask clean-up by connected components (csrc/mask_clean.hip; test.mask_clean): fill the enclosed holes of a binary object mask, then
 *     keep every component, the largest one, or those within a fraction of the largest.  The reference has no counterpart.
 * DEFINITION (tests/mask_clean_restatement.py is its numpy statement).  mask [n, H, W] int32, foreground = (mask == 1); out [n, H, W]
 * int32 holds 0 or 1; every map on its own, in two steps, in integers only:
 *   1 (fill_holes != 0)  the 4-connected components of the NON-foreground; a component with no pixel in the first or last row or column
 *     becomes foreground, and `filled` counts those pixels.  (4-connectivity: the dual of the foreground's 8-connectivity.)
 *   2 the 8-connected components of the foreground after step 1.  A component's label is the smallest linear index y * W + x among its
 *     pixels, its area is its pixel count, A_max the largest area.  mode 0 (all): keep every component.  mode 1 (largest): keep exactly
 *     one component, the one of area A_max with the smallest label.  mode 2 (area): keep every component with
 *     (int64) area * 65536 >= (int64) frac_q16 * A_max; the caller forms frac_q16 = clamp(rint(frac * 65536), 0, 65536) once.
 * An empty mask gives out = 0 and stats = 0.  labels [n, H, W] int32 or NULL: the step-2 label of every foreground pixel BEFORE the
 * selection, -1 on the background.  stats [n, ORYON_MASK_CLEAN_STATS] int32 or NULL = {components, A_max, kept components, kept pixels,
 * removed pixels, filled pixels}.  All three are fully determined by the input: identical bytes across routes, runs and streams.
 *
 * oryon_mask_clean: route 0 = the LDS route where H * W <= ORYON_MASK_CLEAN_LDS_PIXELS (one workgroup per map, one launch, the union-find
 *   state in LDS throughout), else the global route (the same passes as 5 launches, 7 with fill_holes, one more for stats, behind one
 *   memset of 64 bytes a map; the state in the workspace); route 1 / 2 force one.  0 <= n_maps <= 65535 (0: nothing to do, returns
 *   ORYON_OK), H, W >= 1, H W < 2^31, out != mask.  Every check precedes every HIP call and every dereference.  Integer atomics only,
 *   nothing read back, no allocation.
 *   workspace: oryon_mask_clean_workspace_bytes(n_maps, H, W, route) bytes (0 = rejected arguments), 256-byte aligned
 *     = align256(64 max(n_maps, 1)), and on the global route + 3 align256(4 n_maps H W). */
#define ORYON_MASK_CLEAN_STATS 6
#define ORYON_MASK_CLEAN_LDS_PIXELS 65536          /* what the LDS route holds: 256 x 256, in any shape */
/* mode: 0 all, 1 largest, 2 area.  route: 0 auto (LDS where H*W fits), 1 LDS, 2 global */
size_t oryon_mask_clean_workspace_bytes(int n_maps, int H, int W, int route);
int oryon_mask_clean(const int32_t *mask, int n_maps, int H, int W, int mode, int frac_q16, int fill_holes, int route, int32_t *out,
                     int32_t *labels /* may be NULL */, int32_t *stats /* may be NULL */, void *workspace, size_t workspace_bytes,
                     void *stream);

/* a5  StandardDecoder.forward (models/decoder.py:82-108) on the device, fp32 in / fp32 out, for the decoder the reference builds
 *     (get_decoder, models/decoder.py:119-125: input_dim 128, decoder_dims [64, 32], extra_upsampling, guidance projections 256->32 and
 *     128->16): three Up blocks (ConvTranspose2d 2x2 s2 -> cat guidance -> (conv3x3 - GroupNorm(C/16) - ReLU) x 2, :9-42), the two
 *     guidance projections (conv3x3 + bias + ReLU, :66-72) and the 3x3 head (:80).  Replaces the cuDNN / MIOpen convolutions and the
 *     separate GroupNorm / ReLU / cat / clone passes of the reference graph: every convolution is an implicit GEMM on the fp16 matrix
 *     pipe with error-compensated (hi + lo) operands - fp32-grade, see csrc/decoder.hip - GroupNorm + ReLU are applied by the next
 *     layer's loader, the statistics are reduced in a fixed order (bit-reproducible).
 * Weights: DEVICE pointers to the module's fp32 parameters in torch layout (state-dict names in the comments); oryon_decoder_create packs
 * them (a few small launches on `stream`, then one synchronise: the caller's tensors are not referenced afterwards). */
typedef struct oryon_decoder oryon_decoder_t;
typedef struct {
    const float *gp_w[2], *gp_b[2];   /* decoder_guidance_projection.{0,1}.0.{weight,bias}: [32,256,3,3] [32]; [16,128,3,3] [16] */
    const float *up_w[3], *up_b[3];   /* decoder{1,2,3}.up.{weight,bias}: [128,96,2,2] [96]; [64,48,2,2] [48]; [32,32,2,2] [32] */
    const float *c1_w[3];             /* decoder{1,2,3}.conv.double_conv.0.weight: [64,128,3,3]; [32,64,3,3]; [32,32,3,3] */
    const float *n1_g[3], *n1_b[3];   /* ....double_conv.1.{weight,bias}: [64]; [32]; [32] */
    const float *c2_w[3];             /* ....double_conv.3.weight: [64,64,3,3]; [32,32,3,3]; [32,32,3,3] */
    const float *n2_g[3], *n2_b[3];   /* ....double_conv.4.{weight,bias} */
    const float *head_w, *head_b;     /* head.{weight,bias}: [1,32,3,3] [1] */
} oryon_decoder_weights_t;
int oryon_decoder_create(const oryon_decoder_weights_t *weights, oryon_decoder_t **handle, void *stream);
void oryon_decoder_destroy(oryon_decoder_t *handle);
/* x [n_img, 128, h, w] NCHW (= rearrange(fusion output, 'B C T H W -> (B T) C H W'), :93), g2 [n_img, 256, 2h, 2w], g3 [n_img, 128, 4h, 4w]
 * (guidance[1:], :86; guidance_layout = ORYON_LAYOUT_NCHW, or ORYON_LAYOUT_NHWC for [n_img, 2h, 2w, 256] / [n_img, 4h, 4w, 128] - the Swin
 * tower's own token layout, of which net.py:72-75 returns permuted views), h % 8 == 0, w % 8 == 0 (the reference: 24 x 24) -> featmap [n_img, 32, 8h, 8w] NCHW, logits [n_img, 8h, 8w].
 * workspace: oryon_decoder_workspace_bytes(n_img, h, w) bytes (0 = unsupported shape), 256-byte aligned, no other requirements; three
 * activation buffers at the offsets oryon_decoder_workspace_layout reports (tests read intermediates there).
 * stop_after: 0 = the whole module; k = 3 i + j (debug / tests): return after block i's cat buffer (j = 1), first (j = 2) or second
 * (j = 3) convolution - raw NHWC outputs in buffers 0, 1, 2. */
int64_t oryon_decoder_workspace_bytes(int n_img, int h, int w);
int oryon_decoder_workspace_layout(int n_img, int h, int w, int64_t *offsets3);
int oryon_decoder_forward(const oryon_decoder_t *handle, const float *x, const float *g2, const float *g3, int n_img, int h, int w,
                          void *workspace, int64_t workspace_bytes, float *featmap, float *logits, int guidance_layout, int stop_after, void *stream);

/* a4  window attention of ImageTextFusion's guided Swin blocks (models/fusion.py:75-103 inside :173-213) on un-windowed tokens:
 *     qk [B, H, W, 2C] fp32 (the q projection, then the k projection of [x | guidance]), v [B, H, W, C] fp32 -> out [B, H, W, C] fp32 =
 *     roll(-shift) -> 12 x 12 windows -> softmax(q k^T / sqrt(32) + shift mask) v per head -> windows back -> roll(+shift), one kernel;
 *     both products on the fp16 matrix pipe with error-compensated operands (fp32-grade, ~1e-6), fp32 softmax.  head_dim 32 (C == heads * 32), window == 12, H % 12 == 0, W % 12 == 0 (the reference: 24 x 24, 4 heads). */
int oryon_fusion_window_attention_f32(const float *qk, const float *v, int B, int H, int W, int C, int heads, int window, int shift,
                                      float *out, void *stream);

/* a4  the two convolutions of ImageTextFusion on its 24 x 24 maps (models/fusion.py:562 + :595-600: conv1 7x7 pad 3 on the cost volume;
 *     :566-570 + :614-615: guidance_projection 3x3 pad 1 + ReLU) as implicit GEMMs on the fp16 matrix pipe with error-compensated operands
 *     (fp32-grade).  x [n, 24, 24, cin] fp32 NHWC -> y [n, 24, 24, cout] fp32 NHWC = act(conv(x, w) + bias); ksize 3 or 7 (stride 1, padding
 *     ksize / 2), cout % 64 == 0, cin % 4 == 0.  `image`: the weights packed once by oryon_conv24_pack_f16x3 from torch's [cout, cin, k, k]
 *     layout into oryon_conv24_image_bytes(cout, cin, ksize) bytes (0 = unsupported shape). */
int64_t oryon_conv24_image_bytes(int cout, int cin, int ksize);
int oryon_conv24_pack_f16x3(const float *w, int cout, int cin, int ksize, void *image, void *stream);
int oryon_conv24_f16x3(const float *x, int n, int cin, const void *image, const float *bias, int cout, int ksize, int relu, float *y, void *stream);

/* a4  the class-aggregation layer of the fusion module's aggregator (models/fusion.py:300-332 around the LinearAttention of :240-266) for the
 *     reference's single prompt axis (T = 1) on 24 x 24 maps with 128 channels, 4 heads, 6 x 6 pooling, 128-wide text guidance: AvgPool ->
 *     LayerNorm -> q | k from [tokens | text guidance], v -> elu + 1 linear attention -> residual -> LayerNorm -> MLP 128 -> 512 -> 128 (ReLU)
 *     -> residual -> bilinear upsampling (align_corners) -> residual on the map, one kernel, fp32 arithmetic.
 *     x [B, 24, 24, 128] fp32 NHWC, text_guidance [B, 128] fp32 -> out [B, 24, 24, 128] fp32 NHWC.  Weights: device pointers, torch layouts
 *     (norm1 / norm2: [128]; attention.q / .k: [128, 256] + [128]; attention.v: [128, 128] + [128]; MLP.0: [512, 128] + [512]; MLP.2: [128, 512] + [128]). */
typedef struct {
    const float *ln1_w, *ln1_b, *wq, *bq, *wk, *bk, *wv, *bv, *ln2_w, *ln2_b, *w1, *b1, *w2, *b2;
} oryon_fusion_class_weights_t;
int oryon_fusion_class_layer_f32(const float *x, const float *text_guidance, const oryon_fusion_class_weights_t *weights, int B, float *out,
                                 void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ORYON_HIP_H */
