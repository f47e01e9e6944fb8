"""numpy statement of the sub-pixel refinement (include/oryon_hip.h: oryon_subpix_refine, oryon_lift_pairs_subpix; csrc/match_subpix.hip).

    facet_fit(f, curv_min)                           float64: the quadratic through 3 x 3 values -> (flag, (dy, dx), gate quantities)
    refine(feat_a, feat_q, corrs, curv_min)          float64 on float32 maps [C,FH,FW]: offsets [n,2] float32, flags [n] uint8, gates [n,2]
    lift_pairs_subpix(...)                           float32, one operation per rounding: (pcd_a, pcd_q, keep, bilinear_a, bilinear_q)
    shifted_fields(...) / nearest_rows(...)          the smooth-field experiment: a query map that is the anchor field shifted by a
                                                     known fraction of a pixel, and its exhaustive nearest neighbours
The device side is compared with these in tests/test_gpu_subpix.py; tests/test_subpix_restatement.py checks them on their own."""
import numpy as np

EPS = 1e-8
F32 = np.float32


def facet_fit(f, curv_min):
    """f [3,3] float64, f[i + 1, j + 1] = d(y_q + i, x_q + j) -> (flag in {0, 2, 3}, (dy, dx) clamped (zeros unless flag 0),
    (l_min - curv_min, 1 - max|o|): the two gate quantities)."""
    f = np.asarray(f, dtype=np.float64)
    gx = (f[:, 2] - f[:, 0]).sum() / 6.0
    gy = (f[2, :] - f[0, :]).sum() / 6.0
    hxx = (f[:, 2] - 2.0 * f[:, 1] + f[:, 0]).sum() / 3.0
    hyy = (f[2, :] - 2.0 * f[1, :] + f[0, :]).sum() / 3.0
    hxy = (f[2, 2] - f[2, 0] - f[0, 2] + f[0, 0]) / 4.0
    lmin = (hxx + hyy) / 2.0 - np.sqrt((hxx - hyy) ** 2 / 4.0 + hxy * hxy)
    with np.errstate(all="ignore"):
        det = hxx * hyy - hxy * hxy
        ox = -(hyy * gx - hxy * gy) / det
        oy = -(hxx * gy - hxy * gx) / det
        far = max(abs(ox), abs(oy))
    if lmin < curv_min:
        return 2, (0.0, 0.0), (lmin - curv_min, np.nan)
    if not far <= 1.0:
        return 3, (0.0, 0.0), (lmin - curv_min, 1.0 - far)
    return 0, (float(np.clip(oy, -0.5, 0.5)), float(np.clip(ox, -0.5, 0.5))), (lmin - curv_min, 1.0 - far)


def unit(u):
    u = np.asarray(u, dtype=np.float64)
    return u / max(np.sqrt((u * u).sum()), EPS)


def stencil(feat_a, feat_q, row):
    """The nine cosine distances of one interior row, float64."""
    ya, xa, yq, xq = (int(v) for v in row)
    a = unit(feat_a[:, ya, xa])
    return np.array([[0.5 * (1.0 - (a * unit(feat_q[:, yq + i, xq + j])).sum()) for j in (-1, 0, 1)] for i in (-1, 0, 1)])


def refine(feat_a, feat_q, corrs, curv_min):
    """feat_* [C,FH,FW] float32, corrs [n,4] -> offsets [n,2] float32, flags [n] uint8, gates [n,2] float64 (NaN where not evaluated)."""
    C, FH, FW = feat_a.shape
    n = len(corrs)
    offsets, flags, gates = np.zeros((n, 2), F32), np.zeros((n,), np.uint8), np.full((n, 2), np.nan)
    for r, (ya, xa, yq, xq) in enumerate(np.asarray(corrs).tolist()):
        if not (1 <= yq <= FH - 2 and 1 <= xq <= FW - 2 and 0 <= ya < FH and 0 <= xa < FW):
            flags[r] = 1
            continue
        flag, off, gate = facet_fit(stencil(feat_a, feat_q, (ya, xa, yq, xq)), curv_min)
        flags[r], offsets[r], gates[r] = flag, np.asarray(off, dtype=np.float64).astype(F32), gate
    return offsets, flags, gates


def counts(flags, n):
    return np.bincount(np.asarray(flags[:n], dtype=np.int64), minlength=4).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the lift, float32
def _depth_at(d, y, x, jump):
    """(z, whether the bilinear branch was taken) at float32 coordinates inside the image."""
    H, W = d.shape
    i0, j0 = int(y), int(x)
    z00 = d[i0, j0]
    if i0 + 1 < H and j0 + 1 < W:
        z01, z10, z11 = d[i0, j0 + 1], d[i0 + 1, j0], d[i0 + 1, j0 + 1]
        zs = (z00, z01, z10, z11)
        if all(z > 0 for z in zs) and F32(max(zs) - min(zs)) <= jump:
            fy, fx = F32(y - F32(i0)), F32(x - F32(j0))
            gy, gx = F32(F32(1) - fy), F32(F32(1) - fx)
            top = F32(F32(gx * z00) + F32(fx * z01))
            bot = F32(F32(gx * z10) + F32(fx * z11))
            return F32(F32(gy * top) + F32(fy * bot)), True
    return z00, False


def _pinhole(y, x, z, fx, cx, fy, cy):
    k = F32(1000)
    return [F32(F32(F32(F32(x - cx) * z) / fx) / k), F32(F32(F32(F32(y - cy) * z) / fy) / k), F32(z / k)]


def lift_pairs_subpix(corrs, offsets, feat_hw, depth_a, depth_q, cam_a, cam_q, depth_jump_mm):
    """corrs [n,4] int, offsets [n,2] float32 or None, depth_* [H,W] float32 mm, cam_* [9] float32 -> (pcd_a [m,3], pcd_q [m,3] float32
    metres of the kept rows in order, keep [n] bool, bil_a [m], bil_q [m] bool: where the bilinear branch was taken)."""
    FH, FW = feat_hw
    (HA, WA), (HQ, WQ) = depth_a.shape, depth_q.shape
    sya, sxa, syq, sxq = F32(F32(HA) / F32(FH)), F32(F32(WA) / F32(FW)), F32(F32(HQ) / F32(FH)), F32(F32(WQ) / F32(FW))
    jump = F32(depth_jump_mm)
    ca, cq = np.asarray(cam_a, F32), np.asarray(cam_q, F32)
    depth_a, depth_q = np.asarray(depth_a, F32), np.asarray(depth_q, F32)
    pa, pq, keep, ba, bq = [], [], [], [], []
    with np.errstate(all="ignore"):
        for r, (y1, x1, y2, x2) in enumerate(np.asarray(corrs).tolist()):
            dy, dx = (F32(0), F32(0)) if offsets is None else (F32(offsets[r][0]), F32(offsets[r][1]))
            ya, xa = F32(F32(y1) * sya), F32(F32(x1) * sxa)
            yq, xq = F32(F32(F32(y2) + dy) * syq), F32(F32(F32(x2) + dx) * sxq)
            ok = bool(ya >= 0 and ya < F32(HA) and xa >= 0 and xa < F32(WA) and yq >= 0 and yq < F32(HQ) and xq >= 0 and xq < F32(WQ))
            keep.append(ok)
            if not ok:
                continue
            za, bila = _depth_at(depth_a, ya, xa, jump)
            zq, bilq = _depth_at(depth_q, yq, xq, jump)
            pa.append(_pinhole(ya, xa, za, ca[0], ca[2], ca[4], ca[5]))
            pq.append(_pinhole(yq, xq, zq, cq[0], cq[2], cq[4], cq[5]))
            ba.append(bila)
            bq.append(bilq)
    return (np.array(pa, F32).reshape(-1, 3), np.array(pq, F32).reshape(-1, 3), np.array(keep, bool), np.array(ba, bool), np.array(bq, bool))


# ------------------------------------------------------------------------------------------------ the smooth-field experiment
def shifted_fields(C=32, H=24, W=24, period=32.0, shift=(0.3, -0.2), seed=0, terms=4):
    """(anchor map, query map) [C,H,W] float32: every channel a sum of `terms` sinusoids of period >= `period` pixels; the query map is
    the anchor FIELD evaluated at (y - sy, x - sx): the anchor's pixel (y, x) lies at (y + sy, x + sx) of the query map."""
    rng = np.random.default_rng(seed)
    kmax = 2.0 * np.pi / period
    ky, kx = rng.uniform(-kmax, kmax, (C, terms)), rng.uniform(-kmax, kmax, (C, terms))
    ph, amp = rng.uniform(0, 2 * np.pi, (C, terms)), rng.uniform(0.5, 1.0, (C, terms))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def field(y, x):
        return (amp[:, :, None, None] * np.sin(ky[:, :, None, None] * y[None, None] + kx[:, :, None, None] * x[None, None]
                                               + ph[:, :, None, None])).sum(1)
    return field(yy, xx).astype(F32), field(yy - shift[0], xx - shift[1]).astype(F32)


def nearest_rows(feat_a, feat_q, margin=3):
    """Exhaustive float64 nearest neighbour (cosine) of every anchor pixel at least `margin` from the border -> corrs [n,4] int32."""
    C, H, W = feat_a.shape
    a = feat_a.reshape(C, -1).astype(np.float64)
    q = feat_q.reshape(C, -1).astype(np.float64)
    a, q = a / np.maximum(np.linalg.norm(a, axis=0), EPS), q / np.maximum(np.linalg.norm(q, axis=0), EPS)
    ys, xs = np.meshgrid(np.arange(margin, H - margin), np.arange(margin, W - margin), indexing="ij")
    idx = (ys * W + xs).reshape(-1)
    best = np.argmax(a[:, idx].T @ q, axis=1)
    return np.stack([idx // W, idx % W, best // W, best % W], axis=1).astype(np.int32)


def position_rms(corrs, offsets, shift):
    """RMS distance of (y_q + dy, x_q + dx) from the true position (y_a + sy, x_a + sx), in pixels."""
    c = np.asarray(corrs, dtype=np.float64)
    off = np.zeros((len(c), 2)) if offsets is None else np.asarray(offsets, dtype=np.float64)
    ey, ex = c[:, 2] + off[:, 0] - (c[:, 0] + shift[0]), c[:, 3] + off[:, 1] - (c[:, 1] + shift[1])
    return float(np.sqrt((ey * ey + ex * ex).mean()))
