"""One sha256 per case over the raw bytes of the matcher's outputs: what a change to csrc/match_exact.h, csrc/match16.hip,
csrc/match_corrs.hip or csrc/match_x3.hip that means to keep every bit is compared by.  GPU box.

    python tools/dump_match_outputs.py            # one JSON line: {case: sha256}

Run it on a build of each of the two commits and compare the lines.  Per case: corrs, n_valid, n_sel, status, n_undecided and, on the
rows below a pair's anchor count (the others are written by no entry), valid, argmin, min_dist.  The lazy entries run through
tests/test_gpu_anchor_rows_on_demand.py's _old_vs_new, which also asserts that the entry on materialised anchor rows and the `_araw`
entry agree: one hash stands for both.  Inputs: that file's three kinds of pair (Gaussian, smooth, near-duplicates) at C = 256, with
channels-last maps, with float16-rounded values and at C = 96; the crowds and the smooth field of
tests/test_gpu_matcher.py::test_k0v3_duplicates_overflow_and_undecided through the eager int8 and fp16 matchers; one batch of the
headline shape."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gpu_anchor_rows_on_demand as T  # noqa: E402
from oryon_amd import ops  # noqa: E402
from oryon_amd.synth import make_pair  # noqa: E402


def digest(whole, per_row, n_a):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for x in whole:
        h.update(np.ascontiguousarray(x.cpu().numpy()).tobytes())
    for x in per_row:
        for b, n in enumerate(n_a.tolist()):
            h.update(np.ascontiguousarray(x[b, :n].cpu().numpy()).tobytes())
    return h.hexdigest()


def lazy(name, pairs, routes, **kw):
    fa, fq, ma, mq = T._stack(pairs)
    res, (_, na, _) = T._old_vs_new(fa, fq, ma, mq, 256, routes, **kw)
    for route in routes:
        (corrs, n_valid, n_sel, status, md, am, va), und = res[route]
        yield f"{name}_{route}", digest((corrs, n_valid, n_sel, status, und), (va, am, md), na)


def crowd_inputs(C, dev):
    """tests/test_gpu_matcher.py::test_k0v3_duplicates_overflow_and_undecided: a pair with duplicate crowds (candidate lists overflow), a
    plain pair, a smooth field (most anchors undecided by the int8 stage)."""
    g = torch.Generator(device=dev).manual_seed(5)
    H = 40
    base = torch.randn(C, 200, generator=g, device=dev)
    idx = torch.randint(0, 200, (H * H,), generator=g, device=dev)
    fq0 = base[:, idx].reshape(C, H, H).contiguous()
    fa0 = (base[:, idx.flip(0)] + 0.02 * torch.randn(C, H * H, generator=g, device=dev)).reshape(C, H, H).contiguous()
    crowd = fq0[:, 0, 0].clone()
    fq0[:, :4, :] = crowd[:, None, None]
    fa0[:, 0, :8] = crowd[:, None] + 0.001
    fq1 = torch.randn(C, H, H, generator=g, device=dev)
    fa1 = fq1.flip(-1) + 0.05 * torch.randn(C, H, H, generator=g, device=dev)
    basis = torch.randn(C, 6, generator=g, device=dev)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, H, device=dev), indexing="ij")
    coef = torch.stack([torch.ones_like(xx), xx, yy, xx * yy, torch.sin(3 * xx), torch.cos(3 * yy)])
    fq2 = torch.einsum("ck,khw->chw", basis, coef) + 0.01 * torch.randn(C, H, H, generator=g, device=dev)
    fa2 = fq2 + 0.005 * torch.randn(C, H, H, generator=g, device=dev)
    ones = torch.ones((3, H, H), dtype=torch.int32, device=dev)
    return torch.stack((fa0, fa1, fa2)), torch.stack((fq0, fq1, fq2)), ones


def cases():
    dev = "cuda"
    for name, C, kw in (("mixed64", 256, {}), ("mixed64_channels_last", 256, dict(channels_last=True)),
                        ("mixed64_round_f16", 256, dict(round_f16=True)), ("mixed64_c96", 96, {})):
        yield from lazy(name, T._mixed(64, C, dev), ("mx6", "i8", "x3"), **kw)

    fa, fq, ones = crowd_inputs(256, dev)
    roi_a, na = ops.roi_compact(ones)
    roi_q, nq = ops.roi_compact(ones)
    cap = ops.round_up(int(na.max()), 256)
    a8, a_sc, _, _, a_hat = ops.gather_q8(fa, roi_a, na, cap, 256, want_f32=True)
    q8, q_sc, q_eps, q_norm, _ = ops.gather_q8(fq, roi_q, nq, cap, 256)
    und = torch.zeros((3,), dtype=torch.int32, device=dev)
    md, am, va = ops.match_screened8_raw(a_hat, a8, a_sc, fq, roi_q, q_norm, q8, q_sc, q_eps, na, nq, 0.25, n_undecided=und)
    yield "crowds_screened8_raw", digest((und,), (va, am, md), na)
    a32, a16 = ops.gather_normalise(fa, roi_a, na, cap, c_pad=256, want_f16=True)
    q32, q16 = ops.gather_normalise(fq, roi_q, nq, cap, c_pad=256, want_f16=True)
    md, am, va = ops.match_screened(a32, q32, a16, q16, na, nq, 0.25)
    yield "crowds_screened", digest((), (va, am, md), na)

    yield from lazy("cfg2_8x224", [make_pair(i, 224, 224, 256, device=dev) for i in range(8)], ("mx6",), subsample=5000)


if __name__ == "__main__":
    print(json.dumps(dict(cases())))
