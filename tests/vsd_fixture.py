"""What tests/test_vsd.py and tests/test_gpu_vsd.py share: the golden file of the reference's VSD run (tests/golden/g11_vsd.npz,
written by `tools/gen_goldens.py vsd`), the closed-form meshes of oryon_amd/synth.py and the test depth images, each built once."""
import functools
import os

import numpy as np

from oryon_amd import evaluation as ev
from oryon_amd import synth

GOLD = os.path.join(os.path.dirname(__file__), "golden", "g11_vsd.npz")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLD))


@functools.lru_cache(maxsize=None)
def objects():
    """cls -> {'pts', 'faces', 'diameter', 'syms'} as evaluate_batch wants them (no symmetries: the identity alone)."""
    objs = synth.vsd_objects()
    for o in objs.values():
        o["syms"] = ev.format_sym_set(ev.get_symmetry_transformations({}))
    return objs


def pose_mm(pose_m):
    """[4,4] float32 in millimetres after the evaluator's float16 rounding: what the renderer is handed."""
    R, t = ev._pose_f16_mm(pose_m)
    P = np.eye(4, dtype=np.float32)
    P[:3, :3], P[:3, 3] = R.astype(np.float32), t[:, 0].astype(np.float32)
    return P


@functools.lru_cache(maxsize=None)
def test_depths():
    """The [8,480,640] float32 test depth images of the golden's pairs (read-only)."""
    g, objs = golden(), objects()
    H, W = (int(x) for x in g["hw"])
    out = np.stack([synth.vsd_test_depth(ev.rasterize_depth(pose_mm(g["gt"][i]), g["K"], objs[c]["pts"], objs[c]["faces"], H, W))
                    for i, c in enumerate(g["cls"].tolist())])
    out.setflags(write=False)
    return out


test_depths.__test__ = False


def small_camera(H, W):
    """A camera for a small H x W image that keeps the fixtures' objects (about 60 mm across at 0.4 m) inside it."""
    return np.array([[1.1 * W, 0.0, W / 2.0 + 0.3], [0.0, 1.1 * W, H / 2.0 - 0.2], [0.0, 0.0, 1.0]])
