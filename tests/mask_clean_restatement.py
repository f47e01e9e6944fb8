"""Mask clean-up (csrc/mask_clean.hip, include/oryon_hip.h block h1) restated in plain numpy and Python: a flood fill with an explicit
stack, one pixel at a time, in raster order - so the first pixel of a component the scan meets is its smallest linear index, its label.
Nothing here is shared with the kernels; the GPU tests ask for exact equality of out, labels and stats with what this returns.

    clean(mask [H,W] or [n,H,W], mode, frac_q16, fill_holes) -> out, labels (same shape, int32), stats [.., 6] int32
    frac_q16(frac)                                             the host's one rounding of test.mask_clean_frac
    cases()                                                    name -> [H,W] int32 map: the shapes both test files walk"""
import numpy as np

MODES = {"all": 0, "largest": 1, "area": 2}
STATS = ("components", "a_max", "kept_components", "kept_pixels", "removed_pixels", "filled_pixels")
N8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))


def frac_q16(frac: float) -> int:
    return int(min(max(np.rint(float(frac) * 65536.0), 0), 65536))


def components(member: np.ndarray, neighbours):
    """member [H,W] bool -> (labels [H,W] int32: the smallest linear index of the pixel's component, -1 outside; {label: area})."""
    H, W = member.shape
    m = member.tolist()
    lab = [[-1] * W for _ in range(H)]
    areas = {}
    for y in range(H):
        for x in range(W):
            if not m[y][x] or lab[y][x] >= 0:
                continue
            label, area, stack = y * W + x, 0, [(y, x)]
            lab[y][x] = label
            while stack:
                cy, cx = stack.pop()
                area += 1
                for dy, dx in neighbours:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and m[ny][nx] and lab[ny][nx] < 0:
                        lab[ny][nx] = label
                        stack.append((ny, nx))
            areas[label] = area
    return np.array(lab, dtype=np.int32).reshape(H, W), areas


def holes(fg: np.ndarray) -> np.ndarray:
    """The non-foreground pixels whose 4-connected component has no pixel in the first or last row or column."""
    lab, areas = components(~fg, N4)
    border = set(lab[0].tolist()) | set(lab[-1].tolist()) | set(lab[:, 0].tolist()) | set(lab[:, -1].tolist())
    enclosed = [l for l in areas if l not in border]
    return np.isin(lab, enclosed) & ~fg


def clean_one(mask: np.ndarray, mode: int, fq16: int, fill_holes: bool):
    fg = np.asarray(mask) == 1
    filled = 0
    if fill_holes:
        h = holes(fg)
        filled = int(h.sum())
        fg = fg | h
    lab, areas = components(fg, N8)
    if not areas:
        return np.zeros(fg.shape, np.int32), lab, np.zeros(6, np.int32)
    a_max = max(areas.values())
    if mode == 0:
        kept = sorted(areas)
    elif mode == 1:
        kept = [min(l for l, a in areas.items() if a == a_max)]
    elif mode == 2:
        kept = [l for l, a in sorted(areas.items()) if a * 65536 >= fq16 * a_max]
    else:
        raise ValueError(mode)
    out = (np.isin(lab, kept) & fg).astype(np.int32)
    kept_px = sum(areas[l] for l in kept)
    assert kept_px == int(out.sum())
    stats = np.array([len(areas), a_max, len(kept), kept_px, int(fg.sum()) - kept_px, filled], dtype=np.int32)
    return out, lab, stats


def clean(mask: np.ndarray, mode: int = 1, fq16: int = 16384, fill_holes: bool = False):
    mask = np.asarray(mask)
    if mask.ndim == 2:
        return clean_one(mask, mode, fq16, fill_holes)
    parts = [clean_one(m, mode, fq16, fill_holes) for m in mask]
    return tuple(np.stack([p[i] for p in parts]) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------------- the cases
def _z(H, W):
    return np.zeros((H, W), dtype=np.int32)


def ring(m, y0, x0, y1, x1):
    """A one-pixel frame with the corners (y0, x0) and (y1, x1), both inside."""
    m[y0, x0:x1 + 1] = 1
    m[y1, x0:x1 + 1] = 1
    m[y0:y1 + 1, x0] = 1
    m[y0:y1 + 1, x1] = 1
    return m


def serpentine(H=64, W=64):
    """One one-pixel-wide path through the whole map: every second row is full, the rows between hold the turn."""
    m = _z(H, W)
    m[0::2, :] = 1
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def blobs(H, W, seed, n=6, other_values=False):
    """Random rectangles and single pixels from a fixed seed; other_values: sprinkle 2 and -1, which are NOT foreground."""
    r = np.random.default_rng(seed)
    m = _z(H, W)
    for _ in range(n):
        y, x = int(r.integers(0, H)), int(r.integers(0, W))
        h, w = int(r.integers(1, max(2, H // 3))), int(r.integers(1, max(2, W // 3)))
        m[y:y + h, x:x + w] = 1
    m[r.random((H, W)) < 0.04] = 1
    m[r.random((H, W)) < 0.05] = 0
    if other_values:
        m[r.random((H, W)) < 0.03] = 2
        m[r.random((H, W)) < 0.03] = -1
    return m


def cases():
    c = {}
    c["empty"] = _z(7, 9)
    c["full"] = _z(7, 9) + 1
    c["single"] = _z(5, 6)
    c["single"][3, 4] = 1
    c["single_corner"] = _z(5, 6)
    c["single_corner"][4, 5] = 1
    c["row"] = (np.arange(150) % 7 < 4).astype(np.int32)[None, :]                      # H = 1
    c["column"] = (np.arange(150) % 5 != 2).astype(np.int32)[:, None]                  # W = 1
    m = blobs(9, 70, 3, other_values=True)                                             # 70: runs straddle lane 63 / 64 of a wave
    m[0, 60:68] = 1
    m[1, 50:70] = 1
    m[2, 0:8] = 1
    c["w70"] = m
    m = _z(8, 8)                                                                       # two blobs that touch only diagonally
    m[1:4, 1:4] = 1
    m[4:7, 4:7] = 1
    c["diagonal"] = m
    m = _z(10, 10)                                                                     # two enclosed holes that touch only diagonally:
    m[1:9, 1:9] = 1                                                                    # two components for the hole pass
    m[3:5, 3:5] = 0
    m[5:7, 5:7] = 0
    c["diagonal_holes"] = m
    m = c["diagonal_holes"].copy()                                                     # one of them leaks to the border through a channel:
    m[5:7, 7:10] = 0                                                                   # the other one is still enclosed (4-connectivity)
    c["diagonal_leak"] = m
    c["checkerboard"] = ((np.add.outer(np.arange(8), np.arange(9))) % 2).astype(np.int32)
    m = _z(10, 7)                                                                      # a U whose arms join only in the last row
    m[:, 1] = 1
    m[:, 5] = 1
    m[9, 1:6] = 1
    c["u"] = m
    c["serpentine"] = serpentine()
    c["ring"] = ring(_z(9, 11), 2, 2, 6, 8)
    m = ring(ring(ring(_z(21, 23), 1, 1, 19, 21), 4, 4, 16, 18), 7, 7, 13, 15)         # holes inside holes
    m[10, 11] = 1                                                                      # and an island in the innermost hole
    c["nested_rings"] = m
    m = ring(_z(9, 11), 2, 0, 6, 6)                                                    # a ring cut by the border: its hole touches
    m[3:6, 0] = 0                                                                      # column 0 and is not filled
    c["ring_at_border"] = m
    m = _z(9, 12)                                                                      # two components of area 6, one of area 4
    m[1:3, 1:4] = 1
    m[1:3, 7:10] = 1
    m[6:8, 3:5] = 1
    c["tie"] = m
    m = _z(9, 12)                                                                      # three-way tie, the first one in the last position
    m[6:8, 9:11] = 1
    m[1:3, 5:7] = 1
    m[4:6, 0:2] = 1
    c["tie3"] = m
    m = _z(8, 16)                                                                      # areas 8, 4, 2: frac 0.5 puts the 4 exactly on
    m[0:2, 0:4] = 1                                                                    # the integer threshold (4 * 65536 == 32768 * 8)
    m[4:6, 6:8] = 1
    m[7, 12:14] = 1
    c["thresholds"] = m
    return c


FRACS = (0.0, 0.25, 0.5, 0.5 + 1.0 / 65536.0, 1.0)              # 0.5 keeps the component on the threshold, the next one drops it


def batch5(H=16, W=20):
    """Five different maps of one shape: batch indexing."""
    return np.stack([blobs(H, W, 100 + i, other_values=(i == 2)) for i in range(5)])
