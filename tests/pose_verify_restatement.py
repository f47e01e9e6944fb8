"""The float64 numpy statement of depth-consistency pose verification, written from its definition (include/oryon_hip.h, block g4,
oryon_pose_verify) and from nothing else, a per-row pure-Python loop over the same definition, the integer selection rule, and the
builder of the candidate poses its tests share.  Only + - * / and floor are used, one correctly rounded operation at a time, and no
floating-point sum over rows exists, so the device kernels (csrc/pose_verify.hip) must reproduce every output EXACTLY; the margins
recorded here (u + .5 and v + .5 from an integer, | |d| - tol |) say how far every discrete decision of the fixtures stands from its
threshold.  Shared by tests/test_pose_verify_restatement.py (CPU) and tests/test_gpu_pose_verify.py.  The fixtures are
tests/icp_plane_restatement.py's."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_plane_restatement as P  # noqa: E402

CLASSES = 7
BEHIND, OUTSIDE, UNKNOWN, OCCLUDED, VIOLATION, OFF, HIT = range(CLASSES)
MAX_POSES = 16
TOLS = (0.005, 0.01)


def widen(poses):
    """[K,4,4] (or [4,4]) as the entry sees it: fp32 values, widened."""
    T = np.asarray(np.asarray(poses, dtype=np.float32), dtype=np.float64)
    return T.reshape(-1, 4, 4)


def classify(src, depth, mask, cam9, poses, tol):
    """One pair, vectorised over the rows.  src [n,3] float64, depth [H,W] fp32 millimetres, mask [H,W], cam9 [9] float64, poses
    [K,4,4] -> dict(cls [K,n] int32, counts [K,7] int32, frac_gap (pixels: u + .5 and v + .5 from an integer, over the rows in front of
    the camera), tol_gap (metres: | |d| - tol | over the rows that reach the depth test))."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    depth, mask, cam9 = np.asarray(depth, dtype=np.float32), np.asarray(mask), np.asarray(cam9, dtype=np.float64).reshape(9)
    H, W = depth.shape
    fx, cx, fy, cy = cam9[0], cam9[2], cam9[4], cam9[5]
    T = widen(poses)
    n = src.shape[0]
    cls = np.zeros((T.shape[0], n), dtype=np.int32)
    frac_gap, tol_gap = np.inf, np.inf
    for k in range(T.shape[0]):
        s = np.stack([((T[k, r, 0] * src[:, 0] + T[k, r, 1] * src[:, 1]) + T[k, r, 2] * src[:, 2]) + T[k, r, 3] for r in range(3)], axis=1)
        with np.errstate(all="ignore"):
            front = s[:, 2] > 0
            u = (fx * s[:, 0]) / s[:, 2] + cx
            v = (fy * s[:, 1]) / s[:, 2] + cy
            fpx, fpy = np.floor(u + 0.5), np.floor(v + 0.5)
            inside = front & (fpx >= 0.0) & (fpx <= float(W - 1)) & (fpy >= 0.0) & (fpy <= float(H - 1))
            near = front & np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e6) & (np.abs(v) < 1e6)
            if near.any():
                fu, fv = ((u + 0.5) - fpx)[near], ((v + 0.5) - fpy)[near]
                frac_gap = min(frac_gap, float(np.minimum(fu, 1.0 - fu).min()), float(np.minimum(fv, 1.0 - fv).min()))
        px, py = np.where(inside, fpx, 0.0).astype(np.int64), np.where(inside, fpy, 0.0).astype(np.int64)
        zf = depth[py, px]
        known = inside & (zf > np.float32(0.0)) & (zf < np.float32(np.inf))
        with np.errstate(all="ignore"):
            d = s[:, 2] - zf.astype(np.float64) / 1000.0
            occluded = known & (d > tol)
            violation = known & ~occluded & (-d > tol)
            if known.any():
                tol_gap = min(tol_gap, float(np.abs(np.abs(d[known]) - tol).min()))
        agrees = known & ~occluded & ~violation
        hit = agrees & (mask[py, px] == 1)
        c = np.full(n, BEHIND, dtype=np.int32)
        c[front] = OUTSIDE
        c[inside] = UNKNOWN
        c[occluded] = OCCLUDED
        c[violation] = VIOLATION
        c[agrees] = OFF
        c[hit] = HIT
        cls[k] = c
    counts = np.stack([np.bincount(cls[k], minlength=CLASSES)[:CLASSES] for k in range(T.shape[0])]).astype(np.int32)
    return dict(cls=cls, counts=counts, frac_gap=frac_gap, tol_gap=tol_gap)


def classify_row(x, depth, mask, cam9, T, tol):
    """The class of ONE row under ONE candidate, in Python floats (IEEE float64, one operation at a time): the definition read top down."""
    H, W = depth.shape
    fx, cx, fy, cy = float(cam9[0]), float(cam9[2]), float(cam9[4]), float(cam9[5])
    s = [((float(T[r][0]) * x[0] + float(T[r][1]) * x[1]) + float(T[r][2]) * x[2]) + float(T[r][3]) for r in range(3)]
    if not s[2] > 0:
        return BEHIND
    u, v = (fx * s[0]) / s[2] + cx, (fy * s[1]) / s[2] + cy
    if not (math.isfinite(u) and math.isfinite(v)):              # floor of a NaN or an infinity: fails the window test below
        return OUTSIDE
    px, py = math.floor(u + 0.5), math.floor(v + 0.5)
    if not (0 <= px <= W - 1 and 0 <= py <= H - 1):
        return OUTSIDE
    z = float(depth[py, px])
    if not (0 < z < math.inf):
        return UNKNOWN
    d = s[2] - z / 1000.0
    if d > tol:
        return OCCLUDED
    if -d > tol:
        return VIOLATION
    return HIT if int(mask[py, px]) == 1 else OFF


def classify_loop(src, depth, mask, cam9, poses, tol):
    """classify() row by row -> dict(cls [K,n], counts [K,7])."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    depth = np.asarray(depth, dtype=np.float32)
    T = widen(poses)
    cls = np.zeros((T.shape[0], src.shape[0]), dtype=np.int32)
    counts = np.zeros((T.shape[0], CLASSES), dtype=np.int32)
    for k in range(T.shape[0]):
        Tk = [[float(e) for e in row] for row in T[k][:3]]
        for i in range(src.shape[0]):
            c = classify_row([float(e) for e in src[i]], depth, mask, cam9, Tk, float(tol))
            cls[k, i] = c
            counts[k, c] += 1
    return dict(cls=cls, counts=counts)


def select(counts):
    """The selection rule on a [K,7] integer table: most HITs, then fewest BEHIND + VIOLATION + OFF, then the smallest k."""
    best = 0
    for k in range(1, len(counts)):
        h, b = int(counts[k][HIT]), int(counts[k][BEHIND]) + int(counts[k][VIOLATION]) + int(counts[k][OFF])
        h0, b0 = int(counts[best][HIT]), int(counts[best][BEHIND]) + int(counts[best][VIOLATION]) + int(counts[best][OFF])
        if h > h0 or (h == h0 and b < b0):
            best = k
    return best


def verify(src, depth, mask, cam9, poses, tol, status_in=0, n_s=None, cap=None):
    """One pair as the entry returns it.  src [cap,3] with n_s rows in use (None = all; above the capacity: the capacity, below 0: 0)
    -> dict(counts [K,7] int32, best, cls [K,cap] int32 (-1 beyond the count), score [K], frac_gap, tol_gap)."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    cap = src.shape[0] if cap is None else cap
    n = src.shape[0] if n_s is None else max(0, min(int(n_s), src.shape[0]))
    K = widen(poses).shape[0]
    cls = np.full((K, cap), -1, dtype=np.int32)
    if status_in != 0 or n == 0:
        return dict(counts=np.zeros((K, CLASSES), dtype=np.int32), best=0, cls=cls, score=np.zeros(K), frac_gap=np.inf, tol_gap=np.inf)
    r = classify(src[:n], depth, mask, cam9, poses, tol)
    cls[:, :n] = r["cls"]
    return dict(counts=r["counts"], best=select(r["counts"]), cls=cls, score=r["counts"][:, HIT] / float(max(n, 1)), frac_gap=r["frac_gap"],
                tol_gap=r["tol_gap"])


# ------------------------------------------------------------------------------------------------------------------ candidates
CANDIDATES = ("T0", "T_gt", "far", "near")


def shifted(T, dz):
    out = np.array(T, dtype=np.float32)
    out[2, 3] = np.float32(out[2, 3] + np.float32(dz))
    return out


def candidates(f):
    """For fixture f = icp_plane_restatement.fixture(k): T0 (the solver-like start, 4 degrees off), float32(T_gt), `far` (T0 pushed
    0.5 m away: every row lands behind the surface or outside) and `near` (T0 pulled 0.08 m towards the camera: every row floats in
    front of the surface) -> [4,4,4] fp32."""
    return np.stack([np.array(f["T0"], dtype=np.float32), np.asarray(f["T_gt"]).astype(np.float32), shifted(f["T0"], 0.5), shifted(f["T0"], -0.08)])


def sixteen(f):
    """K = 16: the four candidates and twelve small perturbations of them (a translation of a few millimetres each, fixed)."""
    base = candidates(f)
    rng = np.random.default_rng(1600)
    out = [b for b in base]
    for j in range(12):
        T = np.array(base[j % 4], dtype=np.float32)
        T[:3, 3] += rng.uniform(-0.004, 0.004, 3).astype(np.float32)
        out.append(T)
    return np.stack(out)


_cache = {}


def restated(k, tol, which="four"):
    """verify() of fixture k at its own shape under the four (or sixteen) candidates: computed once per process and shared."""
    key = (k, tol, which)
    if key not in _cache:
        f = P.fixture(k)
        _cache[key] = verify(f["src"], f["depth"], f["mask"], f["cam9"], candidates(f) if which == "four" else sixteen(f), tol)
    return _cache[key]
