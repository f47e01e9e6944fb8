"""K1 (ops.match, csrc/match.hip) against the C oracle at every width, i.e. through every instantiation of its two tile loops.  The
K1m and K1r tests use K1 as their yardstick and K1r runs a copy of K1's loops (csrc/match_tile.h), so a slip in the layout contract they
share with K0 could move kernel and yardstick alike: this is K1's yardstick outside the library.  min_dist compares as uint32, argmin and valid compare equal.

Rows are gathered by K0 from [B, C, 1, HW] maps (roi = 0 .. n-1) as tests/test_gpu_match_mutual.py does and the rows >= n are overwritten
with NaN; the oracle normalises the same maps itself (oracle/oryon_oracle.c)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_match_mutual import random_maps, rows_from_maps  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = [32, 64, 128, 256, 512, 96]     # the four anchor-stationary instantiations, the staged kernel at a padded and an un-padded width


def oracle_rows(feat_a, feat_q, na, nq, thr):
    """-> (min_dist, argmin, valid) of one pair's maps [C, 1, HW] on their first na / nq pixels"""
    from oracle import c_oracle
    return c_oracle.match_lin(feat_a.numpy(), feat_q.numpy(), np.arange(na, dtype=np.int32), np.arange(nq, dtype=np.int32), thr)


def compare(got, p, n, want, tag):
    md, am, va = (t[p, :n].cpu().numpy() for t in got)
    assert np.array_equal(md.view(np.uint32), want[0].view(np.uint32)), tag + ": min_dist"
    assert np.array_equal(am, want[1]), tag + ": argmin"
    assert np.array_equal(va, want[2]), tag + ": valid"


@pytest.mark.parametrize("C", WIDTHS)
def test_split_scan_equals_the_oracle(C):
    """Three pairs in row capacities 512 / 512: a panel edge (n_a 129), a 64-row and a 256-row query tile edge (n_q 65, 257), an empty
    anchor side.  B = 3 runs split."""
    from oryon_amd import _lib, ops
    na, nq = [129, 300, 0], [257, 65, 300]
    assert _lib.lib().oryon_match_workspace_bytes(3, 512) == 3 * 16 * 512 * 8         # K1's own statement: S = 16
    fa, fq = random_maps(3, C, 300, 300, 31 + C)
    a_hat, q_hat, n_a, n_q = rows_from_maps(fa, fq, na, nq, 512, 512)
    assert a_hat.shape[2] == (C + 31) // 32 * 32
    want = [oracle_rows(fa[p], fq[p], na[p], nq[p], 0.25) for p in range(3)]
    thr = float(np.median(want[0][0]))                  # cuts about half of pair 0's rows; from the oracle, not from the code under test
    want = [oracle_rows(fa[p], fq[p], na[p], nq[p], thr) for p in range(3)]
    assert 0 < want[0][2].sum() < 129
    got = ops.match(a_hat, q_hat, n_a, n_q, thr)
    torch.cuda.synchronize()
    for p in range(3):
        compare(got, p, na[p], want[p], f"C {C}, pair {p} (n_a {na[p]}, n_q {nq[p]})")


@pytest.mark.parametrize("C", [32, 96])                 # the anchor-stationary and the LDS-staged kernel
def test_unsplit_scan_equals_the_oracle(C):
    """B T >= 8192 -> no query split: the scan writes the outputs itself.  Counts as test_unsplit_launch_shape_many_pairs draws them; the
    oracle scores the first and the last two pairs (the ends of the blockIdx -> pair map)."""
    from oryon_amd import _lib, ops
    B, cap_a, cap_q = 512, 2048, 256
    assert _lib.lib().oryon_match_workspace_bytes(B, cap_a) == 0
    g = torch.Generator(device=DEV).manual_seed(5 + C)
    fa = torch.randn(B, C, 1, cap_a, generator=g, device=DEV)
    fq = torch.randn(B, C, 1, cap_q, generator=g, device=DEV)
    n_a = torch.randint(0, 300, (B,), generator=g, device=DEV, dtype=torch.int32)
    n_a[::7] = torch.randint(1800, cap_a + 1, (len(n_a[::7]),), generator=g, device=DEV, dtype=torch.int32)
    n_q = torch.randint(0, 65, (B,), generator=g, device=DEV, dtype=torch.int32)
    n_a[-1], n_q[-1], n_q[-2] = 2048, 64, 33            # the last pairs are not empty whatever the draw
    na, nq = n_a.cpu().tolist(), n_q.cpu().tolist()
    a_hat, q_hat, n_a, n_q = rows_from_maps(fa, fq, na, nq, cap_a, cap_q)
    thr = 0.25 if C == 32 else 0.4
    got = ops.match(a_hat, q_hat, n_a, n_q, thr)
    torch.cuda.synchronize()
    for p in (0, B - 2, B - 1):
        fq_p = torch.zeros(C, 1, cap_a)                 # the oracle reads both maps with one size
        fq_p[:, :, :cap_q] = fq[p].cpu()
        compare(got, p, na[p], oracle_rows(fa[p].cpu(), fq_p, na[p], nq[p], thr), f"C {C}, pair {p} (n_a {na[p]}, n_q {nq[p]})")
    assert got[2][B - 1, :na[B - 1]].any()


@pytest.mark.parametrize("C", [256, 512])               # match_f32_flagged launches match_f32_regb_kernel<256> / match_f32_kernel
def test_flagged_recompute_equals_the_oracle(C):
    """The screened matcher (ops.match_screened) hands the panels whose candidate lists overflow to K1's flagged recompute
    (match16.hip: a list holds SCREEN_CAP = 64 candidates).  A query descriptor repeated 168 times and eight anchors on it, as
    test_screened_matcher_duplicates_and_overflow builds them: every copy ties for the maximum, so those anchors' lists overflow by
    construction.  The library exposes no count of flagged panels, so what is asserted is the outcome on those rows - the oracle's bits,
    first index on ties - not that the flagged launch produced it."""
    from oryon_amd import ops
    H = 24
    g = torch.Generator().manual_seed(9 + C)
    fq = torch.randn(1, C, H, H, generator=g)
    fa = torch.randn(1, C, H, H, generator=g)
    crowd = fq[0, :, 0, 0].clone()
    fq[0, :, :7, :] = crowd[:, None, None]
    fa[0, :, 0, :8] = crowd[:, None] + 0.001
    ones = torch.ones((1, H, H), dtype=torch.int32, device=DEV)
    roi_a, na = ops.roi_compact(ones)
    roi_q, nq = ops.roi_compact(ones)
    cap = ops.round_up(H * H, 256)
    a_hat, a16 = ops.gather_normalise(fa.to(DEV), roi_a, na, cap, c_pad=C, want_f16=True)
    q_hat, q16 = ops.gather_normalise(fq.to(DEV), roi_q, nq, cap, c_pad=C, want_f16=True)
    md, am, va = ops.match_screened(a_hat, q_hat, a16, q16, na, nq, 0.25)
    torch.cuda.synchronize()
    want = oracle_rows(fa[0].reshape(C, 1, H * H), fq[0].reshape(C, 1, H * H), H * H, H * H, 0.25)
    assert want[2][:8].all() and not want[1][:8].any() and not want[2][8:].any()
    assert np.array_equal(va[0, :H * H].cpu().numpy(), want[2])
    compare((md, am, va), 0, 8, tuple(w[:8] for w in want), f"C {C}, the anchors on the crowd")
