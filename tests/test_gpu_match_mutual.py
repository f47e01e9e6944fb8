"""GPU tests of the mutual nearest-neighbour matcher (csrc/match_mutual.hip) through oryon_match_mutual_f32 / ops.match_mutual.

The yardstick is the EXISTING kernel: the forward outputs must equal ops.match(a_hat, q_hat, ...) and the reverse outputs
ops.match(q_hat, a_hat, n_q, n_a, ...) - the roles swapped - byte for byte on the rows of the pair, `mutual` must equal the numpy
statement of its definition (tests/mutual_restatement.py) applied to those, and for C = 32 and 256 the reverse direction is also checked
against the C oracle with the roles swapped.  Inputs sit in padded buffers whose tail ROWS (>= n_a / >= n_q) hold NaN; outputs sit in
guarded buffers holding a sentinel, and the guards and the unwritten tail rows must keep it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutual_restatement as mr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
SENT = {torch.float32: -12345.0, torch.int32: -7, torch.uint8: 0xAB}
NA = (300, 1, 127, 128, 129)             # ragged counts around the 128-row panel edge
NQ = (700, 1, 63, 64, 65, 257)           # ... and around the 64 / 128 / 256-row query tiles


def guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENT[dtype], dtype=dtype, device=DEV)
    return buf[:n].view(*shape), buf


def counts(B):
    """n_a / n_q of a batch of B pairs: every edge size once B allows it, one pair without anchors and one without queries."""
    na = [NA[i % len(NA)] for i in range(B)]
    nq = [NQ[i % len(NQ)] for i in range(B)]
    if B >= 3:
        na[1], nq[2] = 0, 0
    return na, nq


def rows_from_maps(feat_a, feat_q, na, nq, cap_a, cap_q):
    """K0 on [B,C,1,HW] maps with roi = 0..n-1 -> (a_hat, q_hat, n_a, n_q) on the device, the rows >= n overwritten with NaN."""
    from oryon_amd import ops
    B = feat_a.shape[0]

    def one(feat, n, cap):
        roi = torch.arange(feat.shape[3], dtype=torch.int32, device=DEV).repeat(B, 1).contiguous()
        cnt = torch.tensor(n, dtype=torch.int32, device=DEV)
        hat = ops.gather_normalise(feat.to(DEV).contiguous(), roi, cnt, cap)
        for p in range(B):
            hat[p, n[p]:] = float("nan")
        return hat, cnt
    a_hat, n_a = one(feat_a, na, cap_a)
    q_hat, n_q = one(feat_q, nq, cap_q)
    return a_hat, q_hat, n_a, n_q


def random_maps(B, C, hw_a, hw_q, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, 1, hw_a, generator=g), torch.randn(B, C, 1, hw_q, generator=g)


def run_mutual(a_hat, q_hat, n_a, n_q, thr):
    """oryon_match_mutual_f32 into guarded, sentinel-filled buffers -> dict of numpy arrays; guards and tail rows are checked here."""
    from oryon_amd import _lib
    L = _lib.lib()
    B, cap_a, Cp = a_hat.shape
    cap_q = q_hat.shape[1]
    spec = dict(min_dist=(torch.float32, cap_a), argmin=(torch.int32, cap_a), valid=(torch.uint8, cap_a),
                rev_min_dist=(torch.float32, cap_q), rev_argmin=(torch.int32, cap_q), mutual=(torch.uint8, cap_a))
    bufs = {k: guarded((B, cap), dt) for k, (dt, cap) in spec.items()}
    wsb = L.oryon_match_mutual_workspace_bytes(B, cap_a, cap_q)
    ws, ws_buf = guarded((wsb,), torch.uint8)
    v = {k: b[0] for k, b in bufs.items()}
    _lib.check(L.oryon_match_mutual_f32(_lib.ptr(a_hat), _lib.ptr(q_hat), B, Cp, cap_a, cap_q, _lib.ptr(n_a), _lib.ptr(n_q), float(thr),
                                        _lib.ptr(v["min_dist"]), _lib.ptr(v["argmin"]), _lib.ptr(v["valid"]), _lib.ptr(v["rev_min_dist"]),
                                        _lib.ptr(v["rev_argmin"]), _lib.ptr(v["mutual"]), _lib.ptr(ws), wsb, _lib.stream_ptr(DEV)),
               "oryon_match_mutual_f32")
    torch.cuda.synchronize()
    na, nq = n_a.cpu().tolist(), n_q.cpu().tolist()
    assert bool((ws_buf[wsb:] == SENT[torch.uint8]).all()), "workspace: wrote past its end"
    out = {}
    for k, (view, buf) in bufs.items():
        assert bool((buf[view.numel():] == SENT[buf.dtype]).all()), f"{k}: wrote past its end"
        n = nq if k.startswith("rev_") else na
        for p in range(B):
            assert bool((view[p, n[p]:] == SENT[buf.dtype]).all()), f"{k}: pair {p} wrote rows >= its count"
        out[k] = view.cpu().numpy()
    return out


def yardstick(a_hat, q_hat, n_a, n_q, thr):
    """The existing kernel in both directions (NaN tail rows and all)."""
    from oryon_amd import ops
    f = [t.cpu().numpy() for t in ops.match(a_hat, q_hat, n_a, n_q, thr)]
    r = [t.cpu().numpy() for t in ops.match(q_hat, a_hat, n_q, n_a, thr)]
    return f, r


def check(a_hat, q_hat, n_a, n_q, thr, got=None):
    """-> the outputs, after comparing them with the yardstick and the restatement pair by pair."""
    got = run_mutual(a_hat, q_hat, n_a, n_q, thr) if got is None else got
    (md, am, va), (rmd, ram, _) = yardstick(a_hat, q_hat, n_a, n_q, thr)
    na, nq = n_a.cpu().tolist(), n_q.cpu().tolist()
    for p in range(len(na)):
        a, q = na[p], nq[p]
        tag = f"pair {p} (n_a {a}, n_q {q})"
        assert np.array_equal(got["min_dist"][p, :a].view(np.uint32), md[p, :a].view(np.uint32)), tag + ": min_dist"
        assert np.array_equal(got["argmin"][p, :a], am[p, :a]), tag + ": argmin"
        assert np.array_equal(got["valid"][p, :a], va[p, :a]), tag + ": valid"
        assert np.array_equal(got["rev_min_dist"][p, :q].view(np.uint32), rmd[p, :q].view(np.uint32)), tag + ": rev_min_dist"
        assert np.array_equal(got["rev_argmin"][p, :q], ram[p, :q]), tag + ": rev_argmin"
        want = mr.mutual_flags(am[p, :a], va[p, :a], ram[p, :q])
        assert np.array_equal(got["mutual"][p, :a].astype(bool), want), tag + ": mutual"
        assert set(np.unique(got["mutual"][p, :a]).tolist()) <= {0, 1}
        m = got["mutual"][p, :a].astype(bool)
        hit = got["argmin"][p, :a][m]
        assert len(set(hit.tolist())) == int(m.sum()), tag + ": two mutual rows share a query row"
        assert np.array_equal(got["rev_min_dist"][p][hit].view(np.uint32), got["min_dist"][p, :a][m].view(np.uint32)), tag
        if a == 0 or q == 0:
            assert not m.any()
            assert np.all(np.isinf(got["rev_min_dist"][p, :q])) and not got["rev_argmin"][p, :q].any() if a == 0 else True
            assert np.all(np.isinf(got["min_dist"][p, :a])) and not got["argmin"][p, :a].any() and not got["valid"][p, :a].any() if q == 0 else True
    return got


_cache = {}


def median_threshold(a_hat, q_hat, n_a, n_q):
    """A threshold that cuts about half of pair 0's rows - random descriptors sit further apart the wider they are, a fixed 0.25 would
    leave no valid row at C >= 64.  Taken from the EXISTING kernel's distances, never from the code under test."""
    (md, _, _), _ = yardstick(a_hat, q_hat, n_a, n_q, 0.25)
    return float(np.median(md[0, :int(n_a[0])]))


def ragged(B, C, seed=0):
    """-> (a_hat, q_hat, n_a, n_q, thr) of a batch with the edge counts; built once per (B, C)."""
    key = (B, C, seed)
    if key not in _cache:
        na, nq = counts(B)
        fa, fq = random_maps(B, C, 300, 700, 100 * C + B + seed)
        r = rows_from_maps(fa, fq, na, nq, 512, 768)
        _cache[key] = r + (median_threshold(*r),)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ widths, pair counts, ragged edges
@pytest.mark.parametrize("B", [1, 3, 9])                                 # 9 crosses the p = slot * 8 + xcd pair mapping
@pytest.mark.parametrize("C", [32, 64, 128, 256, 512, 33, 96])           # every width path; 33 -> 64 and 96 un-padded / staged narrow
def test_both_directions_equal_the_existing_kernel(B, C):
    a_hat, q_hat, n_a, n_q, thr = ragged(B, C)
    assert a_hat.shape[2] == (C + 31) // 32 * 32
    got = check(a_hat, q_hat, n_a, n_q, thr)
    assert 0 < got["mutual"][0, :300].sum() < got["valid"][0, :300].sum() < 300      # the case is not vacuous


def test_unsplit_launch_shape_many_pairs():
    """B T >= 8192 -> no query split (S = 1): the scan stores the forward direction itself and the join reads it back.  Rows are made
    directly (unit rows of random normals): the yardstick runs on the same rows."""
    from oryon_amd import _lib
    B, cap_a, cap_q = 512, 2048, 256
    assert _lib.lib().oryon_match_workspace_bytes(B, cap_a) == 0         # K1's own statement that this shape is unsplit
    assert _lib.lib().oryon_match_mutual_workspace_bytes(B, cap_a, cap_q) == B * cap_q * 8
    g = torch.Generator(device=DEV).manual_seed(5)
    for C in (32, 96):                                                   # the register-resident and the LDS-staged kernel
        a_hat = torch.nn.functional.normalize(torch.randn(B, cap_a, C, generator=g, device=DEV), dim=2)
        q_hat = torch.nn.functional.normalize(torch.randn(B, cap_q, C, generator=g, device=DEV), dim=2)
        n_a = torch.randint(0, 300, (B,), generator=g, device=DEV, dtype=torch.int32)
        n_a[::7] = torch.randint(1800, cap_a + 1, (len(n_a[::7]),), generator=g, device=DEV, dtype=torch.int32)
        n_q = torch.randint(0, 65, (B,), generator=g, device=DEV, dtype=torch.int32)
        rows_a = torch.arange(cap_a, device=DEV)[None, :, None] >= n_a[:, None, None]
        rows_q = torch.arange(cap_q, device=DEV)[None, :, None] >= n_q[:, None, None]
        a_hat = torch.where(rows_a, torch.full_like(a_hat, float("nan")), a_hat).contiguous()
        q_hat = torch.where(rows_q, torch.full_like(q_hat, float("nan")), q_hat).contiguous()
        check(a_hat, q_hat, n_a, n_q, 0.25 if C == 32 else 0.4)


@pytest.mark.parametrize("C", [32, 256])
def test_reverse_direction_against_the_c_oracle(C):
    from oracle import c_oracle
    na, nq = [129, 300], [257, 65]
    fa, fq = random_maps(2, C, 300, 300, 7 + C)
    a_hat, q_hat, n_a, n_q = rows_from_maps(fa, fq, na, nq, 512, 512)
    thr = median_threshold(a_hat, q_hat, n_a, n_q)
    got = check(a_hat, q_hat, n_a, n_q, thr)
    assert got["mutual"][0, :129].any() and got["mutual"][1, :300].any()
    for p in range(2):
        ra, rq = np.arange(na[p], dtype=np.int32), np.arange(nq[p], dtype=np.int32)
        rmd, ram, _ = c_oracle.match_lin(fq[p].numpy(), fa[p].numpy(), rq, ra, thr)           # roles swapped
        assert np.array_equal(got["rev_min_dist"][p, :nq[p]].view(np.uint32), rmd.view(np.uint32))
        assert np.array_equal(got["rev_argmin"][p, :nq[p]], ram)
        md, am, va = c_oracle.match_lin(fa[p].numpy(), fq[p].numpy(), ra, rq, thr)
        assert np.array_equal(got["mutual"][p, :na[p]].astype(bool), mr.mutual_flags(am, va, ram))


# ------------------------------------------------------------------------------------------------ exact ties
@pytest.mark.parametrize("C", [32, 128, 512])
def test_one_descriptor_on_each_side_only_row_zero_is_mutual(C):
    g = torch.Generator().manual_seed(C)
    fa = torch.randn(1, C, 1, 1, generator=g).expand(1, C, 1, 300).contiguous()
    fq = torch.randn(1, C, 1, 1, generator=g).expand(1, C, 1, 700).contiguous()
    got = check(*rows_from_maps(fa, fq, [300], [700], 512, 768), 1.5)
    assert got["valid"][0, :300].all() and not got["argmin"][0, :300].any() and not got["rev_argmin"][0, :700].any()
    assert got["mutual"][0, :300].tolist() == [1] + [0] * 299


@pytest.mark.parametrize("C", [64, 256, 512])
def test_duplicate_blocks_across_panel_and_half_wave_edges_lowest_index_wins(C):
    """Blocks of identical anchors (and, nearly on top of them, identical queries) that straddle a 128-row panel edge and the
    31/32 and 63/64 lane-half edges: every anchor of a block matches the block's FIRST query row, every query its FIRST anchor row."""
    g = torch.Generator().manual_seed(11 + C)
    fa, fq = random_maps(1, C, 300, 300, 11 + C)
    blocks = ((120, 136), (28, 37), (60, 68), (250, 262))
    for lo, hi in blocks:
        x = torch.randn(C, generator=g)
        fa[0, :, 0, lo:hi] = x[:, None]
        fq[0, :, 0, lo:hi] = (x + 0.01 * torch.randn(C, generator=g))[:, None]
    got = check(*rows_from_maps(fa, fq, [300], [300], 512, 512), 0.45)
    for lo, hi in blocks:
        assert (got["argmin"][0, lo:hi] == lo).all() and (got["rev_argmin"][0, lo:hi] == lo).all()
        assert got["mutual"][0, lo:hi].tolist() == [1] + [0] * (hi - lo - 1)


# ------------------------------------------------------------------------------------------------ the many-to-one crowd
@pytest.mark.parametrize("C", [32, 256])
def test_a_crowd_on_one_query_pixel_keeps_one_row(C):
    g = torch.Generator().manual_seed(3 + C)
    fa, fq = random_maps(1, C, 300, 700, 3 + C)
    crowd = torch.arange(100, 140)                                       # 40 distinct anchors around query row 5, across a panel edge
    fa[0, :, 0, crowd] = fq[0, :, 0, 5][:, None] + 0.05 * torch.randn(C, len(crowd), generator=g)
    got = check(*rows_from_maps(fa, fq, [300], [700], 512, 768), 0.25)
    assert (got["argmin"][0, crowd.numpy()] == 5).all() and got["valid"][0, crowd.numpy()].all()
    assert int(got["mutual"][0, crowd.numpy()].sum()) == 1
    assert 100 <= got["rev_argmin"][0, 5] < 140 and got["mutual"][0, got["rev_argmin"][0, 5]] == 1


# ------------------------------------------------------------------------------------------------ thresholds
def test_thresholds_cut_valid_and_mutual_follows():
    a_hat, q_hat, n_a, n_q, cut = ragged(3, 64)                          # cut: from the existing kernel, about half of pair 0's rows
    some = check(a_hat, q_hat, n_a, n_q, cut)
    none = check(a_hat, q_hat, n_a, n_q, 0.0)
    every = check(a_hat, q_hat, n_a, n_q, 1.5)
    assert 0 < some["valid"][0, :300].sum() < 300 and not none["valid"][0, :300].any() and every["valid"][0, :300].all()
    assert not none["mutual"][0, :300].any()
    assert not (some["mutual"][0, :300] & ~some["valid"][0, :300].astype(bool)).any()            # mutual is a subset of valid
    assert (some["mutual"][0, :300] <= every["mutual"][0, :300]).all() and some["mutual"][0, :300].sum() < every["mutual"][0, :300].sum()
    for k in ("rev_min_dist", "rev_argmin", "min_dist", "argmin"):      # the threshold touches valid and mutual only
        assert np.array_equal(some[k][0, :300], every[k][0, :300])


# ------------------------------------------------------------------------------------------------ repeatability, the façade
@pytest.mark.parametrize("C", [32, 256, 512])
def test_runs_positions_and_streams_give_the_same_bytes(C):
    a_hat, q_hat, n_a, n_q, thr = ragged(9, C)
    one = run_mutual(a_hat, q_hat, n_a, n_q, thr)
    two = run_mutual(a_hat, q_hat, n_a, n_q, thr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        three = run_mutual(a_hat, q_hat, n_a, n_q, thr)
    for k in one:
        assert one[k].tobytes() == two[k].tobytes() == three[k].tobytes(), k
    na, nq = counts(9)
    for p in (0, 4, 8):                                                  # a pair alone (another split count) against its place in the batch
        alone = run_mutual(a_hat[p:p + 1].contiguous(), q_hat[p:p + 1].contiguous(), n_a[p:p + 1].contiguous(), n_q[p:p + 1].contiguous(), thr)
        for k in one:
            n = nq[p] if k.startswith("rev_") else na[p]
            assert alone[k][0, :n].tobytes() == one[k][p, :n].tobytes(), (k, p)


def test_ops_match_mutual_is_the_entry_point():
    from oryon_amd import ops
    a_hat, q_hat, n_a, n_q, thr = ragged(3, 128)
    want = run_mutual(a_hat, q_hat, n_a, n_q, thr)
    got = ops.match_mutual(a_hat, q_hat, n_a, n_q, thr)
    names = ("min_dist", "argmin", "valid", "rev_min_dist", "rev_argmin", "mutual")
    assert len(got) == 6 and [t.dtype for t in got] == [torch.float32, torch.int32, torch.uint8, torch.float32, torch.int32, torch.uint8]
    na, nq = counts(3)
    for k, t in zip(names, got):
        for p in range(3):
            n = nq[p] if k.startswith("rev_") else na[p]
            assert t[p, :n].cpu().numpy().tobytes() == want[k][p, :n].tobytes(), (k, p)
