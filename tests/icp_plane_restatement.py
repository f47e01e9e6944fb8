"""The float64 numpy statement of point-to-plane ICP on the query's depth map, written from its definition (include/oryon_hip.h,
oryon_icp_plane_refine; DESIGN.md "Point-to-plane ICP on the depth map") and from nothing else, and the builder of the synthetic
fixtures its tests share.  Only + - * / sqrt and floor are used, one correctly rounded operation at a time, so the device kernels
(csrc/icp_plane.hip) differ from it by the order of the sums over rows alone - except for the discrete results (pixels, kept rows,
iteration counts), which the margins recorded here determine.  Shared by tests/test_icp_plane_restatement.py (CPU) and
tests/test_gpu_icp_plane.py."""
import numpy as np

MAX_ITER, TOLERANCE, MAX_DIST, NORMAL_JUMP = 20, 1e-5, 0.02, 0.02
MIN_ROWS = 6                   # fewer kept rows than unknowns: no solve
PIVOT_FLOOR = 1e-12            # a Cholesky pivot must exceed this times the largest diagonal entry of A
# the 21 unique entries of A in the order of the record: row-major upper triangle
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]


def transform(T, x):
    """s = ((R0 x + R1 y) + R2 z) + t per coordinate; T [3|4,4] float64, x [n,3] float64."""
    T = np.asarray(T, dtype=np.float64)
    return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], axis=1)


def lift(x, y, z, cam9):
    """g1's lift of integer pixels (x, y) with depth z (float64 holding fp32 millimetres): the pixel-minus-centre difference in fp32."""
    fx, cx, fy, cy = cam9[0], cam9[2], cam9[4], cam9[5]
    dx = (np.asarray(x).astype(np.float32) - np.float32(cx)).astype(np.float64)
    dy = (np.asarray(y).astype(np.float32) - np.float32(cy)).astype(np.float64)
    return np.stack([((dx * z) / fx) / 1000.0, ((dy * z) / fy) / 1000.0, z / 1000.0], axis=-1)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def norm3(e):
    return np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])


def origin_of(T0, src):
    """The mean of the source rows moved by T_0 (a non-finite coordinate counts as 0, so that one bad row cannot poison it)."""
    s = transform(T0, src)
    return np.where(np.isfinite(s), s, 0.0).sum(axis=0) / float(src.shape[0])


def associate(T, src, depth, mask, cam9, o, max_dist=MAX_DIST, normal_jump=NORMAL_JUMP):
    """Steps 1-5 of one iteration, per row.  -> dict(kept [n] bool, pix [n] int32 (py W + px of a kept row, -1 otherwise), J [m,6],
    r [m], s [n,3], drops = how many rows left at each test, stage [n] = the test at which each row left (px, py: its pixel once it
    is inside), and the margins of the discrete decisions: frac_gap (u + .5 and v + .5
    from an integer, rows in front of the camera), dist_gap (metres), jump_gap (millimetres))."""
    H, W = depth.shape
    fx, cx, fy, cy = cam9[0], cam9[2], cam9[4], cam9[5]
    n = src.shape[0]
    s = transform(T, src)
    drops = dict(behind=0, outside=0, mask=0, depth=0, normal=0, dist=0)
    with np.errstate(all="ignore"):
        front = s[:, 2] > 0
        drops["behind"] = int((~front).sum())
        u = (fx * s[:, 0]) / s[:, 2] + cx
        v = (fy * s[:, 1]) / s[:, 2] + cy
        fpx, fpy = np.floor(u + 0.5), np.floor(v + 0.5)
        inside = front & (fpx >= 1.0) & (fpx <= float(W - 2)) & (fpy >= 1.0) & (fpy <= float(H - 2))
        fu, fv = (u + 0.5) - fpx, (v + 0.5) - fpy
        near = front & np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e6) & (np.abs(v) < 1e6)
        frac_gap = float(min(np.minimum(fu, 1.0 - fu)[near].min(), np.minimum(fv, 1.0 - fv)[near].min())) if near.any() else np.inf
    drops["outside"] = int((front & ~inside).sum())
    px, py = np.where(inside, fpx, 1.0).astype(np.int64), np.where(inside, fpy, 1.0).astype(np.int64)
    on = inside & (mask[py, px] == 1)
    drops["mask"] = int((inside & ~on).sum())
    zc = depth[py, px].astype(np.float64)
    has = on & (zc > 0)
    drops["depth"] = int((on & ~has).sum())
    jump = normal_jump * 1000.0
    ok = has.copy()
    jump_gap = np.inf
    V = {}
    for name, (ddx, ddy) in dict(xp=(1, 0), xm=(-1, 0), yp=(0, 1), ym=(0, -1)).items():
        zn = depth[py + ddy, px + ddx].astype(np.float64)
        dz = np.abs(zn - zc)
        there = has & (zn > 0)
        if there.any():
            jump_gap = min(jump_gap, float(np.abs(dz[there] - jump).min()))
        ok &= (zn > 0) & (dz <= jump)
        V[name] = lift(px + ddx, py + ddy, zn, cam9)
    c = cross(V["xp"] - V["xm"], V["yp"] - V["ym"])
    ln = norm3(c)
    with np.errstate(all="ignore"):
        ok &= (ln > 0) & np.isfinite(ln)
        nrm = c / ln[:, None]
    drops["normal"] = int((has & ~ok).sum())
    e = s - lift(px, py, zc, cam9)
    dist = norm3(e)
    kept = ok & (dist <= max_dist)
    drops["dist"] = int((ok & ~kept).sum())
    dist_gap = float(np.abs(dist[ok] - max_dist).min()) if ok.any() and np.isfinite(max_dist) else np.inf
    nk, ek, pk = nrm[kept], e[kept], s[kept] - o
    r = (nk[:, 0] * ek[:, 0] + nk[:, 1] * ek[:, 1]) + nk[:, 2] * ek[:, 2]
    J = np.concatenate([cross(pk, nk), nk], axis=1)
    pix = np.where(kept, py * W + px, -1).astype(np.int32)
    # where each row left: 0 behind, 1 outside or border, 2 mask 0, 3 no depth, 4 no normal, 5 beyond max_dist, 6 kept
    stage = front.astype(int) + inside + on + has + ok + kept
    return dict(kept=kept, pix=pix, J=J, r=r, s=s, drops=drops, stage=stage, px=px, py=py, frac_gap=frac_gap, dist_gap=dist_gap, jump_gap=jump_gap)


def normal_equations(J, r):
    """-> A [6,6] (symmetric, from its 21 unique sums), g [6], sum |r|."""
    A = np.zeros((6, 6))
    for i, j in UPPER:
        A[i, j] = A[j, i] = float(np.sum(J[:, i] * J[:, j]))
    g = np.array([float(np.sum(J[:, i] * r)) for i in range(6)])
    return A, g, float(np.sum(np.abs(r)))


def cholesky_solve(A, g):
    """A x = -g by an unblocked Cholesky in a fixed order -> (x [6] or None when a pivot fails, the smallest pivot / max_i A_ii)."""
    top = max(A[i, i] for i in range(6))
    L = np.zeros((6, 6))
    ratio = np.inf
    for j in range(6):
        d = A[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        ratio = min(ratio, d / top if top > 0 else -np.inf)
        if not d > PIVOT_FLOOR * top:
            return None, ratio
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            v = A[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    y, x = np.zeros(6), np.zeros(6)
    for i in range(6):
        v = -g[i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v / L[i, i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k, i] * x[k]
        x[i] = v / L[i, i]
    return x, ratio


def cayley(w):
    """R = I + 2 / (1 + a.a) ([a]x + [a]x^2), a = w / 2; [a]x^2 = a a^T - (a.a) I."""
    a = [w[0] / 2.0, w[1] / 2.0, w[2] / 2.0]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    f = 2.0 / (1.0 + aa)
    K = [[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]]
    R = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            sq = a[i] * a[j] - (aa if i == j else 0.0)
            R[i, j] = (1.0 if i == j else 0.0) + f * (K[i][j] + sq)
    return R


def compose(x, o, T):
    """dT T for dT: p -> R (p - o) + o + v with R = cayley(x[0:3]), v = x[3:6]; T [3,4] -> [3,4]."""
    R = cayley(x[:3])
    Tn = np.zeros((3, 4))
    for c in range(3):
        for e in range(4):
            Tn[c, e] = (R[c, 0] * T[0, e] + R[c, 1] * T[1, e]) + R[c, 2] * T[2, e]
        Ro = (R[c, 0] * o[0] + R[c, 1] * o[1]) + R[c, 2] * o[2]
        Tn[c, 3] += (o[c] - Ro) + x[3 + c]
    return Tn


def icp_plane(src, depth, mask, cam9, T0=None, max_iter=MAX_ITER, tolerance=TOLERANCE, max_dist=MAX_DIST, normal_jump=NORMAL_JUMP,
              status_in=0, n_s=None):
    """One pair.  src [cap,3] float64 with n_s rows in use (None = all), depth [H,W] fp32 millimetres, mask [H,W] (1 = object),
    cam9 [9] float64, T0 [4,4] (None = identity; arrives as fp32 and is widened).
    -> dict(T [3,4] float64, iters, mean_err, n_kept, idx [n_s] int32 (the last executed iteration's pixels, -1 = not kept), idx_seq,
            n_kept_seq, drops (summed over the iterations), cond (the largest cond(A) solved), x_seq, and the smallest margins:
            frac_gap, dist_gap, jump_gap, conv_gap, pivot_gap (pivot ratio minus 1e-12), rows_gap (m - 6 over the solved iterations))."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    src = src if n_s is None else src[:max(0, min(int(n_s), src.shape[0]))]
    depth, mask, cam9 = np.asarray(depth, dtype=np.float32), np.asarray(mask), np.asarray(cam9, dtype=np.float64).reshape(9)
    T4 = np.eye(4) if T0 is None else np.asarray(np.asarray(T0, dtype=np.float32), dtype=np.float64).reshape(4, 4)
    T = T4[:3].copy()
    out = dict(T=T, iters=0, mean_err=0.0, n_kept=0, idx=np.full(src.shape[0], -1, dtype=np.int32), idx_seq=[], n_kept_seq=[], x_seq=[],
               drops=dict(behind=0, outside=0, mask=0, depth=0, normal=0, dist=0), cond=0.0, frac_gap=np.inf, dist_gap=np.inf,
               jump_gap=np.inf, conv_gap=np.inf, pivot_gap=np.inf, rows_gap=np.inf)
    if status_in != 0 or src.shape[0] < MIN_ROWS:
        return out
    o = origin_of(T, src)
    out["origin"] = o
    prev = 0.0
    for _k in range(int(max_iter)):
        a = associate(T, src, depth, mask, cam9, o, max_dist, normal_jump)
        m = int(a["kept"].sum())
        out["idx"], out["n_kept"] = a["pix"], m
        out["idx_seq"].append(a["pix"])
        out["n_kept_seq"].append(m)
        for k in out["drops"]:
            out["drops"][k] += a["drops"][k]
        for k in ("frac_gap", "dist_gap", "jump_gap"):
            out[k] = min(out[k], a[k])
        out["rows_gap"] = min(out["rows_gap"], m - MIN_ROWS if m >= MIN_ROWS else MIN_ROWS - 1 - m)
        if m < MIN_ROWS:
            break
        A, g, sum_abs = normal_equations(a["J"], a["r"])
        mean = sum_abs / float(m)
        x, ratio = cholesky_solve(A, g)
        out["pivot_gap"] = min(out["pivot_gap"], abs(ratio - PIVOT_FLOOR))
        if x is None:
            break
        out["cond"] = max(out["cond"], float(np.linalg.cond(A)))
        out["x_seq"].append(x)
        T = compose(x, o, T)
        out["T"], out["iters"], out["mean_err"] = T, out["iters"] + 1, mean
        out["conv_gap"] = min(out["conv_gap"], abs(abs(prev - mean) - tolerance))
        if abs(prev - mean) < tolerance:
            break
        prev = mean
    return out


# ------------------------------------------------------------------------------------------------------------------ fixtures
# pair -> (H, W, n_s, seed).  The smallest shapes that still take every branch: one row past a 256-row block, the block exactly, one
# short of it, more than one block, and a pair below six rows that never starts.
FIXTURES = {1: (48, 48, 300, 11), 2: (40, 56, 257, 12), 3: (56, 40, 256, 13), 4: (48, 48, 255, 14), 5: (48, 48, 5, 15)}


def rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def surface_mm(x, y, W):
    """The query's analytic height field in millimetres: bumpy, tilted, with a 45 mm step at x > 0.7 W."""
    return 400.0 + 25.0 * np.sin(0.23 * x + 0.3) * np.cos(0.19 * y) + 0.4 * x + 12.0 * np.cos(0.31 * (x + y)) + 45.0 * (x > 0.7 * W)


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


_cache = {}


def fixture(k):
    """-> dict(src [n_s,3] float64, depth [H,W] fp32 mm, mask [H,W] int32, cam9 [9] float64 (fp32 values), T0 [4,4] fp32, T_gt [4,4],
    centre [3] = the object's centre in the query camera).  Built once per process and shared: treat it as read-only."""
    if k in _cache:
        return _cache[k]
    H, W, n, seed = FIXTURES[k]
    rng = np.random.default_rng(seed)
    f = 150.0
    cam9 = np.array([f, 0.0, W / 2 - 0.37, 0.0, f - 2.5, H / 2 + 0.21, 0.0, 0.0, 1.0], dtype=np.float32).astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ellipse = ((xx - W / 2) / (0.46 * W)) ** 2 + ((yy - H / 2) / (0.40 * H)) ** 2 <= 1.0
    strip = (yy >= 1) & (yy <= 3)                                       # depth outside the mask: projects, but mask 0
    depth = np.where(ellipse | strip, surface_mm(xx, yy, W), 0.0).astype(np.float32)
    mask = ellipse.astype(np.int32)
    depth[H // 2 + 2:H // 2 + 4, W // 2 - 7:W // 2 - 5] = 0.0            # a hole inside the mask: mask 1, no depth
    # the source: sub-pixel samples of the same surface (some beyond the image and the mask), moved by inv(T_gt)
    x, y = rng.uniform(-4.0, W + 3.0, n), rng.uniform(-4.0, H + 3.0, n)
    z = surface_mm(x, y, W)
    q = np.stack([(x - cam9[2]) * z / cam9[0] / 1000.0, (y - cam9[5]) * z / cam9[4] / 1000.0, z / 1000.0], axis=1)
    T_gt = rigid(rot(rng.normal(size=3), 0.5), np.array([0.03, -0.02, 0.05]) + rng.normal(size=3) * 0.01)
    P = rigid(rot(rng.normal(size=3), np.deg2rad(4.0)), rng.normal(size=3) * 0.009 / np.sqrt(3.0))
    obj = ellipse & (depth > 0)
    centre = lift(xx[obj].astype(np.int64), yy[obj].astype(np.int64), depth[obj].astype(np.float64), cam9).mean(axis=0)
    P[:3, 3] += centre - P[:3, :3] @ centre                             # the 4 degrees turn about the object, as a solver's error does
    T0 = (P @ T_gt).astype(np.float32)
    inv = np.linalg.inv(T_gt)
    src = q @ inv[:3, :3].T + inv[:3, 3]
    if n >= MIN_ROWS:                                                   # one hand-placed row that T_0 moves behind the camera
        inv0 = np.linalg.inv(T0.astype(np.float64))
        src[n // 2] = inv0[:3, :3] @ np.array([0.01, 0.02, -0.3]) + inv0[:3, 3]
    _cache[k] = dict(name=f"pair{k}", src=np.ascontiguousarray(src), depth=depth, mask=mask, cam9=cam9, T0=T0, T_gt=T_gt, centre=centre,
                     H=H, W=W)
    return _cache[k]


def pose_error(T, T_gt, centre):
    """-> (rotation angle in degrees, translation in metres at the object's centre) of T against T_gt."""
    T4 = np.eye(4)
    T4[:3] = np.asarray(T, dtype=np.float64)[:3]
    D = T4 @ np.linalg.inv(T_gt)
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(D[:3, :3] @ centre + D[:3, 3] - centre))
