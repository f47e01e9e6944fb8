"""Float64 numpy restatement of the RANSAC pose solver's meaning, with the index table as an INPUT (helper of the test_*ransac*
files and of tools/gen_goldens.py gen_ransac; not a test module).

The reference (utils/geo6d.py:40-120) is a sequential loop; what it computes is

    hypothesis 0      = the least-squares fit over all n rows; hypothesis k >= 1 = the fit over the four rows of draw k - 1
    iterations evaluate hypotheses 0 .. max_iter - 1 (the last draw is made, never evaluated)
    count_k           = #{i : |R a_i + t - b_i| <= match_err}
    first k with count_k > fix_percent * n  -> the fit over that hypothesis's inliers (exit)
    otherwise         -> the hypothesis with the largest count, lowest k on ties, as it is
    every count 0, or n < 4 -> zeros

and that is what `restate` evaluates, all hypotheses at once."""
import numpy as np

G = 1e-6          # metres: a point whose float64 error is further than this from match_err must be classified as float64 does


def fit(A, B):
    """Least-squares rigid transform of rows A onto rows B: plain means, SVD of the covariance, reflection fixed on the last row
    of Vt -> [3,4].  Batched over leading dimensions."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ca, cb = A.mean(-2, keepdims=True), B.mean(-2, keepdims=True)
    H = np.swapaxes(A - ca, -1, -2) @ (B - cb)
    U, _, Vt = np.linalg.svd(H)
    R = np.swapaxes(Vt, -1, -2) @ np.swapaxes(U, -1, -2)
    flip = np.linalg.det(R) < 0
    Vt = Vt.copy()
    Vt[..., 2, :] *= np.where(flip, -1.0, 1.0)[..., None]
    R = np.swapaxes(Vt, -1, -2) @ np.swapaxes(U, -1, -2)
    t = cb[..., 0, :] - np.einsum("...ij,...j->...i", R, ca[..., 0, :])
    return np.concatenate([R, t[..., None]], -1)


def errors(RT, A, B):
    """[K,3,4] x [n,3] -> [K,n] float64 distances |R a + t - b|."""
    P = np.einsum("kij,nj->kni", RT[:, :, :3], np.asarray(A, np.float64)) + RT[:, None, :, 3]
    return np.linalg.norm(P - np.asarray(B, np.float64)[None], axis=-1)


def rank_deficient(idx, max_iter):
    """[max_iter] bool: hypothesis k >= 1 whose draw names fewer than 3 distinct rows (its rotation is free about a line)."""
    bad = np.zeros(max_iter, bool)
    for k in range(1, max_iter):
        bad[k] = len(set(idx[k - 1].tolist())) < 3
    return bad


def restate(A, B, idx, max_iter, match_err, fix_percent):
    """-> dict(pose [3,4] float64, winner (int, -1 = none), exited (bool), counts [max_iter] int64, err [max_iter, n])."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    n = A.shape[0]
    zero = dict(pose=np.zeros((3, 4)), winner=-1, exited=False, counts=np.zeros(max_iter, np.int64), err=None)
    if n < 4:
        return zero
    idx = np.asarray(idx)[:max_iter - 1]
    RT = np.concatenate([fit(A, B)[None], fit(A[idx], B[idx])], 0) if max_iter > 1 else fit(A, B)[None]
    err = errors(RT, A, B)
    inl = err <= match_err
    counts = inl.sum(1)
    out = dict(counts=counts, err=err)
    over = np.nonzero(counts > fix_percent * n)[0]
    if len(over):
        k = int(over[0])
        return dict(out, pose=fit(A[inl[k]], B[inl[k]]), winner=k, exited=True)
    if counts.max() == 0:
        return dict(zero, counts=counts, err=err)
    k = int(np.argmax(counts))                    # first of the largest
    return dict(out, pose=RT[k], winner=k, exited=False)


# ------------------------------------------------------------------------------------------------ the device's counter RNG
M64 = (1 << 64) - 1


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rng_u32(seed, key, stream, i):
    return mix64((mix64((seed ^ (key * 0xD1B54A32D192ED03)) & M64) + ((stream << 32) | i)) & M64) >> 32


def device_sample_idx(seed, key, n, max_iter):
    """[max_iter, 4] int32: row k, column j = (rng_u32(seed, key, 3, 4 k + j) * n) >> 32."""
    return np.array([[(rng_u32(seed, key, 3, 4 * k + j) * n) >> 32 for j in range(4)] for k in range(max_iter)], np.int32)
