"""One sha256 per case over the raw bytes of every output of the ICP refiners (ops.icp_refine, ops.icp_best_fit, ops.icp_plane_refine):
what a change to csrc/icp.hip, csrc/icp_plane.hip or csrc/icp_common.h that means to keep the arithmetic is compared by.  GPU box.

    python tools/dump_icp_outputs.py            # one JSON line: {case: sha256}

Run it on a build of each of the two commits and compare the lines.  The hashes are NOT goldens: kabsch.h is compiled under the
compiler's default contraction, so the last bits of a rotation belong to the toolchain, not to the definition - they are equal between
two builds by one compiler, nothing more.  The inputs are the packers and fixtures of tests/test_gpu_icp.py and
tests/test_gpu_icp_plane.py (the smallest shapes at which the kernels change phase) and tools/time_icp.py's (the shape that is timed)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import test_gpu_icp as P2P  # noqa: E402
import test_gpu_icp_plane as PLANE  # noqa: E402
import time_icp  # noqa: E402
from oryon_amd import ops  # noqa: E402

KEYS = ("T", "T64", "iters", "mean_err", "n_kept", "idx", "status")


def digest(out, keys=KEYS):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for k in keys:
        h.update(np.ascontiguousarray(out[k].cpu().numpy()).tobytes())
    return h.hexdigest()


def cases():
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    shapes = [(3, 40), (63, P2P.TILE), (64, P2P.TILE + 1), (65, 2 * P2P.TILE + 1), (P2P.ROWS + 1, 300), (2 * P2P.ROWS + 1, 700),
              (2 * P2P.ROWS + 1, 2 * P2P.TILE + 1)]
    pk = P2P.pack([P2P._moved(rng, ns, nd) for ns, nd in shapes])
    refine = lambda pk, **kw: ops.icp_refine(pk["src"], pk["dst"], pk["n_src"], pk["n_dst"], pk["T_init"], status=pk["status"], want_idx=True, **kw)
    yield "icp_shapes", digest(refine(pk, max_iter=20, tolerance=1e-4))

    pairs = [P2P.golden(n) for n in sorted(P2P.R.GOLDEN_CASES)]
    pairs.insert(3, dict(P2P.golden("noisy"), name="failed", status=2, T0=np.diag([1.0, 1.0, 1.0, 1.0]) + np.eye(4, k=3) * 0.25))
    yield "icp_goldens_1e-6", digest(refine(P2P.pack(pairs, cap_s=768, cap_d=800), max_iter=20, tolerance=1e-6))

    pk = P2P.pack([P2P._moved(np.random.default_rng(77), 513, 513)])
    paired = ops.icp_best_fit(pk["src"], pk["dst"], pk["n_src"])
    yield "icp_best_fit_513", digest(paired, ("T", "T64", "fitted", "mean_err"))

    pk = PLANE.pack(PLANE.batch_pairs(), cap=PLANE.CAP)
    plane = lambda pk, **kw: ops.icp_plane_refine(pk["src"], pk["n_src"], pk["depth"], pk["mask"], pk["cam9"], pk["T_init"], status=pk["status"],
                                                  want_idx=True, **kw)
    yield "plane_fixtures_1e-5", digest(plane(pk, max_iter=20, tolerance=1e-5))
    yield "plane_fixtures_0", digest(plane(pk, max_iter=20, tolerance=0.0))

    B, N = 8, 2048
    n = torch.full((B,), N, dtype=torch.int32, device=dev)
    src, dst = time_icp.clouds(B, N, dev)
    T0 = torch.eye(4, dtype=torch.float32, device=dev).repeat(B, 1, 1).contiguous()
    yield "icp_timed_8x2048x20", digest(ops.icp_refine(src, dst, n, n, T0, max_iter=20, tolerance=0.0, want_idx=True))
    src, depth, mask, cam9, T0 = time_icp.plane_inputs(B, N, dev)
    yield "plane_timed_8x2048x20", digest(ops.icp_plane_refine(src, n, depth, mask, cam9, T0, max_iter=20, tolerance=0.0, want_idx=True))


if __name__ == "__main__":
    print(json.dumps(dict(cases())))
