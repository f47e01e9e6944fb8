"""The float64 numpy statement of ICP refinement, written from its definition (include/oryon_hip.h, oryon_icp_refine; DESIGN.md "ICP
refinement") and from nothing else.  The order of the sums over rows is NOT part of the definition, so this agrees with the device
kernels (csrc/icp.hip) to rounding, not bit for bit - except for the neighbour indices and the iteration count, which the fixtures'
asserted margins determine.  Shared by tests/test_icp_restatement.py (CPU, against the reference's recorded results),
tests/test_gpu_icp.py and `tools/gen_goldens.py icp`."""
import numpy as np

MAX_ITER, TOLERANCE = 20, 1e-3
FINE_TOLERANCE = 1e-6          # every golden is recorded at its own tolerance and at this one


def transform(T, x):
    """s = ((R0 x + R1 y) + R2 z) + t per coordinate; T [3|4,4] float64, x [n,3] float64."""
    T = np.asarray(T, dtype=np.float64)
    return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], axis=1)


def nearest(s, dst, chunk=256):
    """-> (idx [n] int32 first minimiser or -1, d2 [n], d2 of the best OTHER column [n]).  NaN never wins (strict <)."""
    n, m = s.shape[0], dst.shape[0]
    idx, d2, d2b = np.full(n, -1, dtype=np.int32), np.full(n, np.inf), np.full(n, np.inf)
    for r0 in range(0, n if m > 0 else 0, chunk):
        a = s[r0:r0 + chunk]
        dx, dy, dz = (a[:, None, c] - dst[None, :, c] for c in range(3))
        d = ((dx * dx + dy * dy) + dz * dz)
        d = np.where(np.isnan(d), np.inf, d)                    # a NaN compares below nothing
        j = np.argmin(d, axis=1)
        rows = np.arange(a.shape[0])
        won = d[rows, j] < np.inf
        idx[r0:r0 + chunk], d2[r0:r0 + chunk] = np.where(won, j, -1), d[rows, j]
        if m > 1:
            d[rows, j] = np.inf
            d2b[r0:r0 + chunk] = d.min(axis=1)
    return idx, d2, d2b


def rotation_from_covariance(H):
    """R = V diag(1, 1, det(V U^T)) U^T for H = U S V^T; also the singular values."""
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    d = np.linalg.det(V @ U.T)
    return V @ np.diag([1.0, 1.0, 1.0 if d >= 0 else -1.0]) @ U.T, S, d


def best_fit_transform_icp(A, B, want_svd=False):
    """geo6d.py:122-155 -> [4,4] float64: plain means, H = sum (a - cA)(b - cB)^T, R as above, t = cB - R cA."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    cA, cB = A.mean(axis=0), B.mean(axis=0)
    H = (A - cA).T @ (B - cB)
    R, S, d = rotation_from_covariance(H)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = cB - R @ cA
    return (T, S, d) if want_svd else T


def icp(src, dst, T0=None, max_iter=MAX_ITER, tolerance=TOLERANCE, max_dist=np.inf, status_in=0, n_s=None, n_d=None):
    """One pair.  src [cap_s,3], dst [cap_d,3] float64 with n_s / n_d rows in use (None = all; a count above the capacity is read as
    the capacity, rows beyond a count are never read), T0 [4,4] (None = identity; arrives as fp32 and is widened).
    -> dict(T [4,4] float64, iters, mean_err, n_kept, idx [n_s] int32 = the last executed iteration's neighbours (-1 = none),
            idx_seq (one array per executed iteration), n_kept_seq, and the margins by which its decisions stand: nn_gap = the smallest
            relative gap between a row's best and second-best d2, conv_gap = the smallest | |prev - mean| - tolerance |, keep_gap = the
            smallest relative | dist - max_dist |, sv_ratio = the smallest s2 / s1 of an H; det_negative = fits with det(V U^T) < 0)."""
    src, dst = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(dst, dtype=np.float64).reshape(-1, 3)
    src = src if n_s is None else src[:max(0, min(int(n_s), src.shape[0]))]
    dst = dst if n_d is None else dst[:max(0, min(int(n_d), dst.shape[0]))]
    T = np.eye(4) if T0 is None else np.asarray(np.asarray(T0, dtype=np.float32), dtype=np.float64).reshape(4, 4).copy()
    out = dict(T=T, iters=0, mean_err=0.0, n_kept=0, idx=np.full(src.shape[0], -1, dtype=np.int32), idx_seq=[], nn_gap=np.inf,
               conv_gap=np.inf, sv_ratio=np.inf, det_negative=0, keep_gap=np.inf, n_kept_seq=[])
    if status_in != 0 or src.shape[0] < 3 or dst.shape[0] == 0:
        return out
    prev = 0.0
    for _k in range(int(max_iter)):
        s = transform(T, src)
        idx, d2, d2b = nearest(s, dst)
        dist = np.sqrt(d2)
        kept = (idx >= 0) & (dist <= max_dist)
        m = int(kept.sum())
        out["idx"], out["n_kept"] = idx, m
        out["idx_seq"].append(idx)
        out["n_kept_seq"].append(m)
        if np.isfinite(max_dist) and (idx >= 0).any():
            out["keep_gap"] = min(out["keep_gap"], float(np.min(np.abs(dist[idx >= 0] - max_dist)) / max(max_dist, 1e-300)))
        fin = kept & np.isfinite(d2b) & (d2b > 0)
        if fin.any():
            out["nn_gap"] = min(out["nn_gap"], float(np.min((d2b[fin] - d2[fin]) / d2b[fin])))
        if m < 3:
            break
        mean = float(np.mean(dist[kept]))
        dT, S, d = best_fit_transform_icp(s[kept], dst[idx[kept]], want_svd=True)
        out["sv_ratio"] = min(out["sv_ratio"], float(S[1] / S[0]) if S[0] > 0 else 0.0)
        out["det_negative"] += int(d < 0)
        T = dT @ T
        out["T"], out["iters"], out["mean_err"] = T, out["iters"] + 1, mean
        out["conv_gap"] = min(out["conv_gap"], abs(abs(prev - mean) - tolerance))
        if abs(prev - mean) < tolerance:
            break
        prev = mean
    return out


# ------------------------------------------------------------------------------------------------------------------ golden fixtures
# name -> dict(seed, n, kind, tolerance).  `tools/gen_goldens.py icp` runs the reference's icp on golden_case() and records its result
# (tests/golden/icp_<name>.npz holds the clouds too: they are small).  Equal sizes: the reference asserts them.
GOLDEN_CASES = {
    "identity": dict(seed=21, n=256, kind="identity", tolerance=1e-3),        # identity start, converges early
    "all20": dict(seed=22, n=400, kind="far", tolerance=1e-6),                # every one of the 20 iterations runs
    "noisy": dict(seed=23, n=700, kind="noisy", tolerance=1e-3),              # target = moved source + noise
    "permuted": dict(seed=24, n=300, kind="permuted", tolerance=1e-3),        # target rows shuffled
    "near": dict(seed=25, n=64, kind="near", tolerance=1e-3),                 # a start near the truth
    "mirrored": dict(seed=26, n=128, kind="mirrored", tolerance=1e-3),        # the det < 0 branch of one dT
}


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def object_cloud(rng, n, centre=(0.05, -0.03, 0.9)):
    """n points of a bumpy, anisotropic blob of ~10 x 6 x 4 cm about 0.9 m from the camera: the coordinates (around 1 m) and spread
    (around 5 cm) of an object's depth pixels."""
    u = rng.normal(size=(n, 3)) * np.array([0.05, 0.03, 0.02])
    u[:, 2] += 0.01 * np.sin(u[:, 0] * 60.0) + 0.008 * np.cos(u[:, 1] * 45.0)
    return u + np.asarray(centre)


def golden_case(name):
    """-> (A [n,3], B [n,3], init_pose [4,4] float64 holding fp32 values, or None, tolerance)."""
    c = GOLDEN_CASES[name]
    rng = np.random.default_rng(c["seed"])
    n, kind = c["n"], c["kind"]
    A = object_cloud(rng, n)
    Rt, tt = _rot(rng.normal(size=3), 0.12), rng.normal(size=3) * 0.01
    centre = A.mean(axis=0)
    B = (A - centre) @ Rt.T + centre + tt
    init = None
    if kind == "identity":
        pass
    elif kind == "far":
        # the same surface sampled elsewhere and moved further: no exact fixed point, the mean keeps creeping for 20 iterations
        Rt = _rot(rng.normal(size=3), 0.45)
        B = (object_cloud(rng, n) - centre) @ Rt.T + centre + 3.0 * tt
    elif kind == "noisy":
        B = B + rng.normal(size=B.shape) * 0.002
    elif kind == "permuted":
        B = B[rng.permutation(n)]
    elif kind == "near":
        # the truth is a quarter turn about z and a little more; the start is the quarter turn alone.  Its rotation is a signed
        # permutation, i.e. EXACTLY orthonormal as fp32: the reference ends with a fit of A onto the moved cloud, which equals the
        # composed T_K only when T_0 is rigid (an fp32-rounded general rotation is orthonormal to ~6e-8, and the two then differ by
        # as much - DESIGN.md "ICP refinement")
        Rq = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        B = (A - centre) @ (Rt @ Rq).T + centre + tt
        init = np.eye(4)
        init[:3, :3], init[:3, 3] = Rq, centre - Rq @ centre
    elif kind == "mirrored":
        # a nearly flat cloud against its mirror image through that plane: the best orthogonal fit of the first matching is a
        # reflection, which the det(V U^T) correction turns into the nearest rotation
        A = A.copy()
        A[:, 2] = centre[2] + (A[:, 2] - centre[2]) * 0.15
        B = A.copy()
        B[:, 2] = 2.0 * centre[2] - B[:, 2]
        B = B + tt * 0.2
    else:
        raise KeyError(kind)
    if init is not None:
        init = init.astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(A), np.ascontiguousarray(B), init, c["tolerance"]
