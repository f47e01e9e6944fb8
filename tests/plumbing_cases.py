"""Seeded inputs of the plumbing sweep (tests/test_plumbing_restatement.py on the CPU, tests/test_gpu_plumbing.py on the device), built once
per process and never written to.  Every builder says what its case is for."""
import functools

import numpy as np

import plumbing_restatement as pr

# ------------------------------------------------------------------------------------------------------------------ K-1 resizes
# (HI, WI), (HO, WO), images per call, what the shape is for
RESIZE = {
    "golden_96x128_to_56x56": ((96, 128), (56, 56), 3, "the shape of the recorded fixture"),
    "up_37x53_to_64x48": ((37, 53), (64, 48), 3, "up-sampling, non-square: an unclamped i1 reads the next image's first row"),
    "mixed_64x48_to_37x53": ((64, 48), (37, 53), 3, "down in y, up in x: swapped scales"),
    "identity_31x29": ((31, 29), (31, 29), 3, "identity: l1 = 0 everywhere, the output is the input"),
    "up8_5x3_to_40x56": ((5, 3), (40, 56), 3, "large up-sampling: most outputs sit in the clamped border cells"),
    "up8_5x3_to_40x56_n70": ((5, 3), (40, 56), 70, "the same with 70 images: the image index of the grid's y axis"),
    "line_1x7_to_9x1": ((1, 7), (9, 1), 3, "one-pixel axes on both sides: i1 = i0 on a one-row image"),
    "extreme_200x11_to_13x170": ((200, 11), (13, 170), 3, "ratio 15.4 down against 15.5 up"),
    "near_identity_30x40_to_31x41": ((30, 40), (31, 41), 3, "scale just under 1: src crosses every integer once"),
    "two_trips_300x300_to_260x260": ((300, 300), (260, 260), 3, "67600 outputs > 256 x 256: the second grid-stride trip"),
    "production_480x640_to_224x224": ((480, 640), (224, 224), 1, "the production size, once"),
}
DYADIC = {
    "dyadic_6x5_to_12x10": ((6, 5), (12, 10), 3, "scale 1/2: weights 1/4, 3/4"),
    "dyadic_9x7_to_36x28": ((9, 7), (36, 28), 3, "scale 1/4: weights in eighths"),
    "dyadic_12x10_to_6x5": ((12, 10), (6, 5), 3, "scale 2: weights 1/2"),
}
BAND_CAP = 0.05          # at most this share of a rounded-depth case's pixels may lie within the bar of a rounding tie


def _rng(name, salt):
    return np.random.default_rng([salt] + [ord(c) for c in name])


@functools.lru_cache(maxsize=None)
def rgb_images(name):
    """uint8 [n,HI,WI,3], every channel of every image its own noise: a wrong HWC -> CHW stride or image offset lands in other data."""
    (HI, WI), _, n, _ = RESIZE[name]
    x = _rng(name, 1).integers(0, 256, size=(n, HI, WI, 3), dtype=np.uint8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def depth_float(name):
    """float32 [n,HI,WI], float-valued millimetres: a slope per image plus noise of 30 mm (the unrounded resize on non-integers)."""
    (HI, WI), _, n, _ = RESIZE[name]
    r = _rng(name, 2)
    yy, xx = np.mgrid[0:HI, 0:WI]
    x = np.stack([600.0 + 150.0 * i + 1.7 * xx - 0.9 * yy + r.uniform(-30.0, 30.0, size=(HI, WI)) for i in range(n)]).astype(np.float32)
    x.setflags(write=False)
    return x


def _integer_depth(r, HI, WI, i):
    yy, xx = np.mgrid[0:HI, 0:WI]
    d = 700.0 + 40.0 * (i % 8) + 3.0 * (i // 8) + 0.8 * xx + 0.5 * yy + 25.0 * np.sin(xx / 9.0 + i) + 15.0 * np.cos(yy / 7.0)
    d[:, WI // 2:] += 250.0                                                     # a depth step
    d = np.rint(d) + r.integers(-2, 3, size=(HI, WI))                           # sensor noise of +-2 mm
    d[HI // 4:max(HI // 4 + 1, HI // 2), WI // 4:max(WI // 4 + 1, WI // 2 - 1)] = 0.0      # a hole (no return)
    return d


@functools.lru_cache(maxsize=None)
def depth_int(name):
    """float32 [n,HI,WI], integer-valued millimetres as a sensor gives them: a plane plus a sinusoid plus a 250 mm step plus +-2 noise,
    and a zero hole (what DeviceCollate resizes with round_output=1)."""
    (HI, WI), _, n, _ = RESIZE[name]
    r = _rng(name, 3)
    x = np.stack([_integer_depth(r, HI, WI, i) for i in range(n)]).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def dyadic_depth(name):
    """float32 [n,HI,WI], integers below 4096 at a power-of-two scale: scale, src, the weights and every product are exact in float32, so
    the kernel's output is the float64 statement bit for bit and every rounding tie is a true tie."""
    (HI, WI), _, n, _ = DYADIC[name]
    x = _rng(name, 4).integers(0, 4096, size=(n, HI, WI)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def masks(name):
    """uint8 [n,HI,WI] over {0, 1, 2, 255} (instance ids and the background value), blocks with pixel noise on top."""
    (HI, WI), _, n, _ = RESIZE[name]
    r = _rng(name, 5)
    vals = np.array([0, 1, 2, 255], dtype=np.uint8)
    coarse = r.integers(0, 4, size=(n, (HI + 3) // 4, (WI + 3) // 4))
    m = np.repeat(np.repeat(coarse, 4, axis=1), 4, axis=2)[:, :HI, :WI]
    noise = r.random((n, HI, WI)) < 0.2
    m = np.where(noise, r.integers(0, 4, size=(n, HI, WI)), m)
    out = vals[m]
    out.setflags(write=False)
    return out


def band(want64, tol):
    """The pixels whose float64 value is within the bar of a rounding tie."""
    return np.abs((want64 - np.floor(want64)) - 0.5) <= tol


# ------------------------------------------------------------------------------------------------------------------ roi_compact
# H, W of the maps; the kernel takes 8 pixels per thread and 8192 per scan step, 16-byte loads when HW % 4 == 0 and the map is aligned
COMPACT = {
    "1x1": (1, 1, "the smallest map"),
    "1x7": (1, 7, "one short of a thread's 8 pixels"),
    "1x8": (1, 8, "exactly one thread"),
    "1x9": (1, 9, "one pixel on the second thread"),
    "31x37": (31, 37, "odd HW = 1147: maps 1.. are misaligned, the scalar path"),
    "64x128": (64, 128, "HW = 8192: exactly one scan step"),
    "1x8193": (1, 8193, "odd, one pixel in the second step: the carried base"),
    "2x4098": (2, 4098, "HW = 8196: 16-byte path with a partial second step"),
    "130x63": (130, 63, "HW = 8190: just under one step, HW % 4 != 0"),
    "224x224": (224, 224, "the production map: seven steps"),
}


@functools.lru_cache(maxsize=None)
def compact_masks(name):
    """int32 [5,H,W]: all ones, all zeros, a single 1 at the last pixel, random at p = 0.5, random over {-1, 0, 1, 2, 255} (only 1 counts)."""
    H, W, _ = COMPACT[name]
    r = _rng(name, 6)
    m = np.zeros((5, H, W), dtype=np.int32)
    m[0] = 1
    m[2, -1, -1] = 1
    m[3] = r.random((H, W)) < 0.5
    m[4] = np.array([-1, 0, 1, 2, 255], dtype=np.int32)[r.integers(0, 5, size=(H, W))]
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------------------------------------------------------ K2 lifts
# feature grid, depth map of the anchor side, of the query side
LIFT_GRIDS = {
    "g192": ((192, 192), (375, 501), (240, 320)),      # the non-square fixture's sizes
    "g48": ((48, 64), (480, 640), (480, 640)),         # a coarse grid onto sensor resolution
    "gid": ((240, 320), (240, 320), (480, 640)),       # scale 1 on the anchor side: y = FH-1 is the depth map's last row
}
LIFT_CAPS = (1, 300, 512, 513, 1300)                   # the kernel walks 512 rows per chunk
LIFT_B = 4
LIFT = {f"{g}_cap{c}_{k}": (g, c, k) for g in LIFT_GRIDS for c in LIFT_CAPS for k in ("valid", "mixed")}


@functools.lru_cache(maxsize=None)
def lift_scene(grid):
    """Per grid: B = 4 depth maps per side and cameras, all different.  Pairs 0, 1 carry integer millimetres with 5 % zero pixels, pairs
    2, 3 float depths."""
    _, hwa, hwq = LIFT_GRIDS[grid]
    r = _rng(grid, 7)
    out = {}
    for side, (H, W) in (("a", hwa), ("q", hwq)):
        d = r.uniform(400.0, 1500.0, size=(LIFT_B, H, W))
        d[:2] = np.rint(d[:2])
        d[:2][r.random((2, H, W)) < 0.05] = 0.0
        cam = np.zeros((LIFT_B, 9))
        cam[:, 0], cam[:, 4] = r.uniform(500.0, 620.0, LIFT_B), r.uniform(500.0, 620.0, LIFT_B)
        cam[:, 2], cam[:, 5] = W / 2.0 + r.uniform(-9.0, 9.0, LIFT_B), H / 2.0 + r.uniform(-9.0, 9.0, LIFT_B)
        cam[:, 8] = 1.0
        out["depth_" + side], out["cam_" + side] = d.astype(np.float32), cam.astype(np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lift_corrs(name):
    """int32 [4, n_cap, 4] rows (ya, xa, yq, xq).  'valid': every row inside the grid.  'mixed': about a third of the rows carry a coordinate
    out of the grid in one of the four columns - -1, another negative, FH or FW exactly, or more - and must be dropped, the survivors kept
    in order; both kinds hold rows on the grid's last row and column (the largest y', x' that are kept)."""
    grid, cap, kind = LIFT[name]
    (FH, FW), _, _ = LIFT_GRIDS[grid]
    r = _rng(name, 8)
    c = np.stack([r.integers(0, FH, (LIFT_B, cap)), r.integers(0, FW, (LIFT_B, cap)),
                  r.integers(0, FH, (LIFT_B, cap)), r.integers(0, FW, (LIFT_B, cap))], axis=-1)
    edge = r.random((LIFT_B, cap)) < 0.1
    c[..., 0] = np.where(edge, FH - 1, c[..., 0])
    c[..., 1] = np.where(edge & (r.random((LIFT_B, cap)) < 0.5), FW - 1, c[..., 1])
    c[..., 3] = np.where(edge, FW - 1, c[..., 3])
    if kind == "mixed" and cap < 4:
        c[1, 0, 0] = -1                                                         # too few rows for a draw: one of the four is dropped
    elif kind == "mixed":
        bad = r.random((LIFT_B, cap)) < 0.35
        col = r.integers(0, 4, (LIFT_B, cap))
        lim = np.where(col % 2 == 0, FH, FW)
        what = r.integers(0, 4, (LIFT_B, cap))
        val = np.choose(what, [np.full(lim.shape, -1), -r.integers(2, 50, lim.shape), lim, lim + r.integers(1, 50, lim.shape)])
        for k in range(4):
            c[..., k] = np.where(bad & (col == k), val, c[..., k])
        c[:, 1, 0], c[:, 2, 3], c[:, 3, 2] = FH, FW, -1                         # the three named values, in every pair
        c[:, 1, 1:], c[:, 2, :3], c[:, 3, :2], c[:, 3, 3] = 0, 0, 0, 0
    if cap >= 4:
        c[:, 0] = (FH - 1, FW - 1, FH - 1, FW - 1)                              # the grid's last cell on both sides, first row of each pair
    c = c.astype(np.int32)
    c.setflags(write=False)
    return c


def lift_counts(cap):
    """The two runs of a lift case: (n_corr [4], status [4]).  Run 0: n_corr over {n_cap, n_cap/2, 1, 0}.  Run 1: every pair full and pair 2
    with a status != 0, which gives n_out = 0 and zero rows whatever its n_corr."""
    return ((np.array([cap, cap // 2, min(1, cap), 0], dtype=np.int32), np.zeros(4, dtype=np.int32)),
            (np.full(4, cap, dtype=np.int32), np.array([0, 0, 3, 0], dtype=np.int32)))


@functools.lru_cache(maxsize=None)
def lift_want(name):
    """Per pair the statement on ALL n_cap rows: (pcd_a, pcd_q, keep); the first n rows of a pair give keep[:n] and the first keep[:n].sum()
    points."""
    grid, cap, _ = LIFT[name]
    s, c = lift_scene(grid), lift_corrs(name)
    return [pr.lift_pairs(c[p], LIFT_GRIDS[grid][0], s["depth_a"][p], s["depth_q"][p], s["cam_a"][p], s["cam_q"][p]) for p in range(LIFT_B)]


LIFT_POINTS_N = (0, 1, 255, 256, 257, 300000)           # 300000 > 1024 blocks x 256 threads: the loop's second trip


@functools.lru_cache(maxsize=None)
def lift_points_case(n):
    """One 480 x 640 float depth map with zeros, a camera and n pixels (x, y) as int64, the image corners among them."""
    r = _rng("lift_points", 9 + n)
    d = r.uniform(300.0, 2000.0, size=(480, 640)).astype(np.float32)
    d[r.random((480, 640)) < 0.05] = 0.0
    cam = np.array([591.0125, 0, 322.525, 0, 590.16775, 244.11084, 0, 0, 1], dtype=np.float32)
    x, y = r.integers(0, 640, n), r.integers(0, 480, n)
    if n >= 4:
        x[:4], y[:4] = (0, 639, 0, 639), (0, 0, 479, 479)
    return d, cam, x.astype(np.int64), y.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ pose metrics
POSE_M = (1, 255, 256, 257, 1023, 1024, 1025, 2500)     # 256 points per block, 1024 ground-truth points per LDS tile
POSE_PAIRS = ("equal", "small", "deg170", "deg180", "scaled", "shift")
MULTI_SIZES = (2500, 1, 300, 0)                          # one call over four models, the last one empty
MULTI_MODEL_OF_PAIR = (0, 1, 2, 3, 0, 2)


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


@functools.lru_cache(maxsize=None)
def pose_pairs():
    """(pred, gt) float32 [6,4,4], metres: equal poses; a 2-degree / 5 mm perturbation; 170 degrees; exactly 180 degrees about the x axis
    (gt = the identity rotation, so every entry is exact); the predicted rotation block scaled by 1.3 (the determinant rescale of the
    rotation error); a pure translation."""
    R0, t0 = _rot([0.3, -0.5, 0.8], 37.0), np.array([0.05, -0.03, 0.8])

    def pose(R, t):
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = R, t
        return P
    gt = [pose(R0, t0)] * 6
    gt[3] = pose(np.eye(3), t0)
    pred = [pose(R0, t0), pose(_rot([1, 2, -1], 2.0) @ R0, t0 + 0.005 * np.array([0.6, 0.0, 0.8])), pose(_rot([-1, 1, 3], 170.0) @ R0, t0),
            pose(np.diag([1.0, -1.0, -1.0]), t0), pose(1.3 * (_rot([2, 1, 1], 10.0) @ R0), t0), pose(R0, t0 + np.array([0.01, -0.02, 0.03]))]
    pred, gt = np.stack(pred).astype(np.float32), np.stack(gt).astype(np.float32)
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def model(M, salt=0):
    """float32 [M,3]: an object of 20 x 14 x 8 cm around its origin, metres."""
    p = (_rng("model", 100 + M + 7919 * salt).uniform(-1.0, 1.0, size=(M, 3)) * np.array([0.10, 0.07, 0.04])).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def pose_want(M, salt=0):
    """float64 [6,2]: (ADD, ADD-S) of the statement for model(M) under the six pairs."""
    pred, gt = pose_pairs()
    return np.array([pr.pose_stats(model(M, salt), pred[i].astype(np.float64), gt[i].astype(np.float64)) for i in range(len(POSE_PAIRS))])


@functools.lru_cache(maxsize=None)
def rt_want():
    """float64 ([6] degrees, [6] centimetres) from evaluation.compute_RT_distances on the float32 poses."""
    from oryon_amd import evaluation
    pred, gt = pose_pairs()
    return evaluation.compute_RT_distances(pred.astype(np.float64), gt.astype(np.float64))
