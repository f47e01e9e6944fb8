// VSD (Visible Surface Discrepancy) on the device: a depth rasteriser and the visibility / cost counting kernel.
// Replaces, for the evaluator's VSD / AR columns (utils/evaluator.py:281-288):
//   bop_toolkit_lib/renderer_vispy.py:512-617   render_object(..)['depth']: the OpenGL depth render of the model at a pose
//   bop_toolkit_lib/misc.py:143-163             depth_im_to_dist_im_fast
//   bop_toolkit_lib/visibility.py               the bop19 visibility masks
//   bop_toolkit_lib/pose_error.py:17-93         vsd, 'step' cost, distances normalised by the diameter
//
// The rasteriser is DEFINED (DESIGN.md "VSD: the rasterisation definition"), not fitted to a driver: oryon_amd/evaluation.py
// rasterize_depth is the same sequence of correctly rounded operations in numpy and the two agree bit for bit.
//   vertex   fp32, no contraction, sums left to right: Xc = ((r00 x + r01 y) + r02 z) + t0 (Yc, Zc alike), u = fx (Xc / Zc) + cx,
//            v = fy (Yc / Zc) + cy, iz = 1 / Zc.  Output pixel (row r, column c) samples (u, v) = (c + 0.5, r + 0.5): the reference's
//            'y_down' projection plus the row flip after glReadPixels.
//   snap     x = rint(256 u), y = rint(256 v) (round half to even) into int32.
//   drop     a triangle with a vertex whose Zc is not a positive finite number (no near-plane clipping: the reference's near plane
//            is the pose's bounding-box minimum and its projection is degenerate when that is <= 0), with a vertex whose |u| or
//            |v| exceeds 2^15 pixels, with zero area, or with a vertex index outside its model.
//   cover    int64 edge functions at the sample (256 c + 128, 256 r + 128); the triangle is first oriented to positive area by
//            exchanging its second and third vertex (both windings are drawn: cull_face=False); top-left fill rule in the y-down frame
//            (a sample ON an edge belongs to the triangle when the edge runs upwards, or is horizontal and runs to the right).
//   depth    l_i = float(w_i) / float(w_0 + w_1 + w_2) for i = 1, 2, inv = (iz_0 + l_1 (iz_1 - iz_0)) + l_2 (iz_2 - iz_0), depth = 1 / inv:
//            the eye-space Z in millimetres, perspective-correct (what the reference recovers with mult / (dep + addi)).  Written
//            from vertex 0 so that a triangle of constant Z renders exactly 1 / iz whatever the rounding of the weights.  A sample
//            whose inv does not come out positive (rounding, on a sliver spanning ~2^23 in depth) is not drawn.
//   z-buffer atomicMin on the bit pattern of the positive fp32 depth (GL_LESS; order-independent, so the image is bit-stable),
//            cleared to all-ones, which reads back as the background 0.
// The reference's z-buffer quantisation (a gloo.RenderBuffer depth format of 16 or 24 bits, chosen by the driver) is NOT reproduced:
// the output is the exact interpolated depth.
//
// Work distribution: one thread per (triangle, image) sets the triangle up and draws it if its pixel box is at most 8 x 8 (BOP
// meshes: nearly all of them); larger triangles go to a queue in the workspace and a second launch draws each with one wave, lanes
// striding the box.  Coverage and depth do not depend on the route.  The vertex transform is fused into the set-up.
#include "common.h"
#include "pose_f16.h"

#pragma clang fp contract(off)

namespace oryon {

constexpr int VSD_SMALL_BOX = 8;             // pixel box side up to which the set-up thread draws the triangle itself
constexpr int VSD_HEADER_BYTES = 256;        // workspace header: uint32 counters {queued (large) triangles, triangles drawn by the small route}
constexpr int VSD_MAX_TAU = 16;
constexpr uint32_t VSD_EMPTY = 0xffffffffu;

struct Tri {
    int32_t x0, y0, x1, y1, x2, y2;          // snapped to 1/256 pixel, oriented to positive area
    float iz0, iz1, iz2;
    float area;                              // float(w0 + w1 + w2)
    int cmin, cmax, rmin, rmax;              // pixel box, clipped to the image
};

__device__ __forceinline__ bool project_vertex(const float *P, float fx, float fy, float cx, float cy, const float *p, int32_t &x, int32_t &y,
                                               float &iz)
{
    const float X = ((P[0] * p[0] + P[1] * p[1]) + P[2] * p[2]) + P[3];
    const float Y = ((P[4] * p[0] + P[5] * p[1]) + P[6] * p[2]) + P[7];
    const float Z = ((P[8] * p[0] + P[9] * p[1]) + P[10] * p[2]) + P[11];
    if (!(Z > 0.0f && Z <= 3.402823466e38f)) return false;
    const float su = (fx * (X / Z) + cx) * 256.0f, sv = (fy * (Y / Z) + cy) * 256.0f;
    if (!(fabsf(su) <= 8388608.0f && fabsf(sv) <= 8388608.0f)) return false;          // 2^15 pixels; NaN fails
    x = (int32_t)rintf(su);
    y = (int32_t)rintf(sv);
    iz = 1.0f / Z;
    return true;
}

struct Mesh {
    const float *verts;
    const int32_t *vert_offset, *faces, *face_offset, *model_of_image;
    int n_models, max_faces;                 // max_faces: what the queue was sized for; faces of a model beyond it are not drawn
};

// false: the triangle draws nothing
__device__ __forceinline__ bool setup_triangle(const float *__restrict__ pose, const float *__restrict__ Kc, const Mesh &mesh, int n, int f,
                                               int H, int W, Tri &t)
{
    const int model = mesh.model_of_image ? mesh.model_of_image[n] : 0;
    if ((uint32_t)model >= (uint32_t)mesh.n_models) return false;
    const int v0 = mesh.vert_offset[model], V = mesh.vert_offset[model + 1] - v0;
    const int32_t *idx = mesh.faces + ((size_t)mesh.face_offset[model] + f) * 3;
    const int32_t a = idx[0], b = idx[1], c = idx[2];
    if ((uint32_t)a >= (uint32_t)V || (uint32_t)b >= (uint32_t)V || (uint32_t)c >= (uint32_t)V) return false;
    const float *P = pose + (size_t)n * 16, *K = Kc + (size_t)n * 9;
    const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    if (!project_vertex(P, fx, fy, cx, cy, mesh.verts + (size_t)(v0 + a) * 3, t.x0, t.y0, t.iz0)) return false;
    if (!project_vertex(P, fx, fy, cx, cy, mesh.verts + (size_t)(v0 + b) * 3, t.x1, t.y1, t.iz1)) return false;
    if (!project_vertex(P, fx, fy, cx, cy, mesh.verts + (size_t)(v0 + c) * 3, t.x2, t.y2, t.iz2)) return false;
    int64_t area = (int64_t)(t.x1 - t.x0) * (t.y2 - t.y0) - (int64_t)(t.y1 - t.y0) * (t.x2 - t.x0);
    if (area == 0) return false;
    if (area < 0) {
        int32_t s = t.x1; t.x1 = t.x2; t.x2 = s;
        s = t.y1; t.y1 = t.y2; t.y2 = s;
        const float z = t.iz1; t.iz1 = t.iz2; t.iz2 = z;
        area = -area;
    }
    t.area = (float)area;
    // pixels whose sample 256 c + 128 lies inside [min, max] of the snapped coordinates (>> 8 floors: arithmetic shift)
    const int32_t xmin = min(t.x0, min(t.x1, t.x2)), xmax = max(t.x0, max(t.x1, t.x2));
    const int32_t ymin = min(t.y0, min(t.y1, t.y2)), ymax = max(t.y0, max(t.y1, t.y2));
    t.cmin = max((xmin + 127) >> 8, 0);
    t.cmax = min((xmax - 128) >> 8, W - 1);
    t.rmin = max((ymin + 127) >> 8, 0);
    t.rmax = min((ymax - 128) >> 8, H - 1);
    return t.cmin <= t.cmax && t.rmin <= t.rmax;
}

// edge a -> b at sample p; a sample on the edge counts when the edge is a top or a left one
__device__ __forceinline__ bool edge_inside(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py, int64_t &w)
{
    const int32_t dx = bx - ax, dy = by - ay;
    w = (int64_t)dx * (py - ay) - (int64_t)dy * (px - ax);
    const bool top_left = dy < 0 || (dy == 0 && dx > 0);
    return w > 0 || (w == 0 && top_left);
}

__device__ __forceinline__ void shade(const Tri &t, int r, int c, uint32_t *__restrict__ zimg, int W)
{
    const int32_t px = c * 256 + 128, py = r * 256 + 128;
    int64_t w0, w1, w2;
    const bool in0 = edge_inside(t.x1, t.y1, t.x2, t.y2, px, py, w0);
    const bool in1 = edge_inside(t.x2, t.y2, t.x0, t.y0, px, py, w1);
    const bool in2 = edge_inside(t.x0, t.y0, t.x1, t.y1, px, py, w2);
    if (!(in0 && in1 && in2)) return;
    const float l1 = (float)w1 / t.area, l2 = (float)w2 / t.area;
    const float inv = (t.iz0 + l1 * (t.iz1 - t.iz0)) + l2 * (t.iz2 - t.iz0);
    if (!(inv > 0.0f)) return;               // a sliver whose vertex depths differ by ~2^23: the rounded sum can leave (0, inf); not drawn
    atomicMin(&zimg[(size_t)r * W + c], __float_as_uint(1.0f / inv));
}

__global__ __launch_bounds__(256) void vsd_raster_setup_kernel(const float *__restrict__ pose, const float *__restrict__ Kc, Mesh mesh, int H, int W,
                                                               uint32_t *__restrict__ zbuf, uint32_t *__restrict__ counters,
                                                               uint2 *__restrict__ queue)
{
    const int n = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    const int model = mesh.model_of_image ? mesh.model_of_image[n] : 0;
    const int F = (uint32_t)model < (uint32_t)mesh.n_models ? min(mesh.face_offset[model + 1] - mesh.face_offset[model], mesh.max_faces) : 0;
    Tri t;
    const bool live = f < F && setup_triangle(pose, Kc, mesh, n, f, H, W, t);
    const bool small = live && (t.cmax - t.cmin) < VSD_SMALL_BOX && (t.rmax - t.rmin) < VSD_SMALL_BOX;
    const unsigned long long vote = __ballot(small);
    if (vote != 0ull && (int)(threadIdx.x & 63) == __ffsll((long long)vote) - 1) atomicAdd(&counters[1], (uint32_t)__popcll(vote));
    if (small) {
        uint32_t *zimg = zbuf + (size_t)n * H * W;
        for (int r = t.rmin; r <= t.rmax; ++r)
            for (int c = t.cmin; c <= t.cmax; ++c) shade(t, r, c, zimg, W);
    } else if (live) {
        queue[atomicAdd(&counters[0], 1u)] = make_uint2((uint32_t)n, (uint32_t)f);           // at most N * max_faces entries: the queue's size
    }
}

// one wave per queued triangle, lanes striding its pixel box
__global__ __launch_bounds__(256) void vsd_raster_large_kernel(const float *__restrict__ pose, const float *__restrict__ Kc, Mesh mesh, int H, int W,
                                                               uint32_t *__restrict__ zbuf, const uint32_t *__restrict__ counters,
                                                               const uint2 *__restrict__ queue)
{
    const uint32_t count = counters[0];
    const uint32_t waves = gridDim.x * 4u, lane = threadIdx.x & 63u;
    for (uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6); q < count; q += waves) {
        const uint2 e = queue[q];
        Tri t;
        if (!setup_triangle(pose, Kc, mesh, (int)e.x, (int)e.y, H, W, t)) continue;
        uint32_t *zimg = zbuf + (size_t)e.x * H * W;
        const int bw = t.cmax - t.cmin + 1, total = bw * (t.rmax - t.rmin + 1);
        for (int k = (int)lane; k < total; k += 64) shade(t, t.rmin + k / bw, t.cmin + k % bw, zimg, W);
    }
}

// cleared z-buffer entries -> background 0 (in place: the z-buffer IS the depth image)
__global__ void vsd_resolve_kernel(uint32_t *__restrict__ zbuf, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && zbuf[i] == VSD_EMPTY) zbuf[i] = 0u;
}

// the evaluator's float16 rounding of both poses (pose_f16_mm) -> the fp32 poses, cameras and models of the 2B images (2p: estimate,
// 2p + 1: ground truth); float16 values and their products with 1000 rounded to half are exact in fp32
__global__ void vsd_prepare_kernel(int B, const double *__restrict__ pred, const double *__restrict__ gt, const double *__restrict__ Kc,
                                   const int32_t *__restrict__ model_of_pair, float *__restrict__ pose32, float *__restrict__ K32,
                                   int32_t *__restrict__ model_of_image)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= 2 * B) return;
    const int p = n >> 1;
    const Pose34 T = pose_f16_mm(((n & 1) ? gt : pred) + (size_t)p * 16);
    float *o = pose32 + (size_t)n * 16;
    for (int k = 0; k < 12; ++k) o[k] = (float)T.m[k];
    o[12] = o[13] = o[14] = 0.0f;
    o[15] = 1.0f;
    for (int k = 0; k < 9; ++k) K32[(size_t)n * 9 + k] = (float)Kc[(size_t)p * 9 + k];
    model_of_image[n] = model_of_pair ? model_of_pair[p] : 0;
}

__device__ __forceinline__ double dist_of_depth(float d, double px, double py)         // misc.py:158-161, float64, the reference's order
{
    const double a = px * (double)d, b = py * (double)d, c = (double)d;
    return sqrt((a * a + b * b) + c * c);
}

// counts[p] = (n_union, n_inter, n_cost[tau]) over the pixels of pair p
__global__ __launch_bounds__(256) void vsd_score_kernel(const uint32_t *__restrict__ zbuf /*[2B,H,W]*/, const float *__restrict__ depth_test,
                                                        const double *__restrict__ Kc, int H, int W, const double *__restrict__ diameter,
                                                        float delta, const double *__restrict__ taus, int n_tau, int32_t *__restrict__ counts)
{
    __shared__ int32_t red[4][2 + VSD_MAX_TAU];
    const int p = blockIdx.y;
    const double *K = Kc + (size_t)p * 9;
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5], diam = diameter[p];
    const size_t HW = (size_t)H * W;
    const uint32_t *zest = zbuf + (size_t)(2 * p) * HW, *zgt = zest + HW;
    const float *dt = depth_test + (size_t)p * HW;
    int32_t acc[2 + VSD_MAX_TAU];
#pragma unroll
    for (int k = 0; k < 2 + VSD_MAX_TAU; ++k) acc[k] = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (int)HW; i += gridDim.x * 256) {
        const uint32_t be = zest[i], bg = zgt[i];
        if (be == VSD_EMPTY && bg == VSD_EMPTY) continue;                              // neither mask can hold the pixel (model > 0)
        const int r = i / W, c = i - r * W;
        const double px = ((double)c - cx) / fx, py = ((double)r - cy) / fy;
        const double dist_test = dist_of_depth(dt[i], px, py);
        const double dist_est = dist_of_depth(be == VSD_EMPTY ? 0.0f : __uint_as_float(be), px, py);
        const double dist_gt = dist_of_depth(bg == VSD_EMPTY ? 0.0f : __uint_as_float(bg), px, py);
        // visibility.py:35-37 (bop19): the difference is taken in fp32
        const bool no_test = dist_test == 0.0;
        const bool vis_gt = ((float)dist_gt - (float)dist_test <= delta || no_test) && dist_gt > 0.0;
        bool vis_est = ((float)dist_est - (float)dist_test <= delta || no_test) && dist_est > 0.0;
        vis_est = vis_est || (vis_gt && dist_est > 0.0);                               // visibility.py:73-74
        acc[0] += (vis_gt || vis_est) ? 1 : 0;
        if (vis_gt && vis_est) {
            acc[1] += 1;
            const double d = fabs(dist_gt - dist_est) / diam;
#pragma unroll
            for (int k = 0; k < VSD_MAX_TAU; ++k)
                if (k < n_tau) acc[2 + k] += (d >= taus[k]) ? 1 : 0;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 2 + VSD_MAX_TAU; ++k) {
        int32_t v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 + n_tau) {
        const int k = threadIdx.x;
        const int32_t v = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        if (v != 0) atomicAdd(&counts[(size_t)p * (2 + n_tau) + k], v);
    }
}

// render workspace: header (the counters) | queue of the large triangles [N, max_faces], which is not padded
static size_t carve_render(void *base, int N, int max_faces, uint32_t *&counters, uint2 *&queue)
{
    Carver carve(base);
    carve(counters, VSD_HEADER_BYTES / sizeof(uint32_t));
    carve(queue, (size_t)N * max_faces);
    return carve.end;
}

// z-buffer cleared and filled; zbuf [N,H,W] holds depth bit patterns, VSD_EMPTY where nothing was drawn
static int rasterise(const float *pose, const float *K, int N, const Mesh &mesh, int max_faces, int H, int W, void *workspace, uint32_t *zbuf,
                     hipStream_t st)
{
    uint32_t *counters;
    uint2 *queue;
    carve_render(workspace, N, max_faces, counters, queue);
    ORYON_CHECK_HIP(hipMemsetAsync(counters, 0, VSD_HEADER_BYTES, st));
    ORYON_CHECK_HIP(hipMemsetAsync(zbuf, 0xff, (size_t)N * H * W * sizeof(uint32_t), st));
    hipLaunchKernelGGL(vsd_raster_setup_kernel, dim3(ceil_div(max_faces, 256), N), dim3(256), 0, st, pose, K, mesh, H, W, zbuf, counters, queue);
    const size_t waves = (size_t)N * max_faces;
    const int blocks = (int)(waves < 4096 ? (waves + 3) / 4 : 1024);
    hipLaunchKernelGGL(vsd_raster_large_kernel, dim3(blocks), dim3(256), 0, st, pose, K, mesh, H, W, zbuf, counters, queue);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

// workspace of oryon_vsd_counts: render workspace (header first) | fp32 poses [2B,16] | fp32 K [2B,9] | model_of_image [2B] | z-buffers [2B,H,W]
struct VsdWs {
    void *render;
    float *pose32, *K32;
    int32_t *model_of_image;
    uint32_t *zbuf;
};
static size_t carve_vsd(void *base, VsdWs &w, int B, int H, int W, int max_faces)
{
    const size_t N = 2 * (size_t)B;
    uint32_t *counters;
    uint2 *queue;
    Carver carve(base);
    carve(w.render, carve_render(nullptr, (int)N, max_faces, counters, queue));
    carve(w.pose32, N * 16);
    carve(w.K32, N * 9);
    carve(w.model_of_image, N);
    carve(w.zbuf, N * H * W);
    return carve.off;
}

}  // namespace oryon

using namespace oryon;

extern "C" size_t oryon_render_depth_workspace_bytes(int N, int max_faces)
{
    uint32_t *counters;
    uint2 *queue;
    return N > 0 && max_faces > 0 ? carve_render(nullptr, N, max_faces, counters, queue) : 0;
}

extern "C" int oryon_render_depth(const float *pose, const float *K, int N, const float *verts_mm, const int32_t *vert_offset, const int32_t *faces,
                                  const int32_t *face_offset, int n_models, int max_faces, const int32_t *model_of_image, int H, int W,
                                  void *workspace, float *depth, void *stream)
{
    ORYON_CHECK_ARG(pose && K && verts_mm && vert_offset && faces && face_offset && workspace && depth);
    ORYON_CHECK_ARG(N >= 0 && N <= 65535 && n_models >= 1 && max_faces >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768);
    if (N == 0) return ORYON_OK;
    hipStream_t st = as_stream(stream);
    const Mesh mesh{verts_mm, vert_offset, faces, face_offset, model_of_image, n_models, max_faces};
    uint32_t *zbuf = reinterpret_cast<uint32_t *>(depth);
    const int rc = rasterise(pose, K, N, mesh, max_faces, H, W, workspace, zbuf, st);
    if (rc != ORYON_OK) return rc;
    const size_t n = (size_t)N * H * W;
    hipLaunchKernelGGL(vsd_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, zbuf, n);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}

extern "C" size_t oryon_vsd_workspace_bytes(int B, int H, int W, int max_faces)
{
    if (B <= 0 || H <= 0 || W <= 0 || max_faces <= 0) return 0;
    VsdWs w;
    return carve_vsd(nullptr, w, B, H, W, max_faces);
}

extern "C" int oryon_vsd_counts(const double *pred_pose, const double *gt_pose, const double *K, const float *depth_test, int B, int H, int W,
                                const float *verts_mm, const int32_t *vert_offset, const int32_t *faces, const int32_t *face_offset, int n_models,
                                int max_faces, const int32_t *model_of_pair, const double *diameter_mm, double delta, const double *taus, int n_tau,
                                void *workspace, int32_t *counts, void *stream)
{
    ORYON_CHECK_ARG(pred_pose && gt_pose && K && depth_test && verts_mm && vert_offset && faces && face_offset && diameter_mm && taus);
    ORYON_CHECK_ARG(workspace && counts && B >= 0 && 2 * (int64_t)B <= 65535 && n_models >= 1 && max_faces >= 1);
    ORYON_CHECK_ARG(H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && n_tau >= 1 && n_tau <= VSD_MAX_TAU);
    if (B == 0) return ORYON_OK;
    hipStream_t st = as_stream(stream);
    const int N = 2 * B;
    VsdWs w;
    carve_vsd(workspace, w, B, H, W, max_faces);
    hipLaunchKernelGGL(vsd_prepare_kernel, dim3(ceil_div(N, 128)), dim3(128), 0, st, B, pred_pose, gt_pose, K, model_of_pair, w.pose32, w.K32,
                       w.model_of_image);
    const Mesh mesh{verts_mm, vert_offset, faces, face_offset, w.model_of_image, n_models, max_faces};
    const int rc = rasterise(w.pose32, w.K32, N, mesh, max_faces, H, W, w.render, w.zbuf, st);
    if (rc != ORYON_OK) return rc;
    ORYON_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * (2 + n_tau) * sizeof(int32_t), st));
    const int blocks = min(ceil_div(H * W, 1024), 256);
    hipLaunchKernelGGL(vsd_score_kernel, dim3(blocks, B), dim3(256), 0, st, w.zbuf, depth_test, K, H, W, diameter_mm, (float)delta, taus, n_tau,
                       counts);
    ORYON_CHECK_LAUNCH();
    return ORYON_OK;
}
