"""GPU tests of the rank scan of the one-to-many matcher (csrc/match_next.hip) through oryon_match_next_f32 / ops.match_next.

The yardsticks are the EXISTING kernels, on the shapes and the guarded, sentinel-filled, NaN-padded buffers of
tests/test_gpu_match_second.py (its Case objects are shared, so K0 and K1 run once per shape for both files):
  * n_prev = 1 is K1r's second minimum: next_dist must equal ops.match_second's second_dist byte for byte, next_argmin its
    second_argmin but for -1 where that one writes 0 for "none";
  * n_prev = 2, 3: one batch of one-anchor pairs whose query rows are the candidates of that anchor (outside the discs round ALL
    earlier ranks), compacted in order; ops.match runs once on it.  K1's distance bits do not depend on a row's position, so
    next_dist must equal that min_dist byte for byte and next_argmin its argmin mapped back through the compaction table."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_match_second as ms  # noqa: E402    (Case, guarded, the shared cases; its tests are not re-exported)
import topk_restatement as tr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = ms.DEV
SENT = ms.SENT
CAP_A, CAP_Q = ms.CAP_A, ms.CAP_Q
assert (CAP_A, CAP_Q) == (512, 768)
WIDTHS = [32, 64, 128, 256, 512]                    # the four register-resident instantiations and the staged kernel


def run_next(c, r, prev, sl=slice(None), order=None):
    """oryon_match_next_f32 into guarded, sentinel-filled buffers -> dict of numpy arrays; guards and unwritten rows are checked here.
    prev [n_prev, B, cap_a] int32 on the device.  order: a permutation of the (sliced) batch, undone on the way out."""
    from oryon_amd import _lib
    L = _lib.lib()
    a_hat, q_hat, n_a, n_q, roi_q = (t[sl] for t in (c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q))
    prev = prev[:, sl]
    if order is not None:
        idx = torch.tensor(order, device=DEV)
        a_hat, q_hat, n_a, n_q, roi_q, prev = a_hat[idx], q_hat[idx], n_a[idx], n_q[idx], roi_q[idx], prev[:, idx]
    a_hat, q_hat, n_a, n_q, roi_q, prev = (t.contiguous() for t in (a_hat, q_hat, n_a, n_q, roi_q, prev))
    B, cap_a, Cp = a_hat.shape
    bufs = {"next_dist": ms.guarded((B, cap_a), torch.float32), "next_argmin": ms.guarded((B, cap_a), torch.int32)}
    wsb = L.oryon_match_next_workspace_bytes(B, cap_a)
    ws, ws_buf = ms.guarded((max(wsb, 16),), torch.uint8)
    v = {k: b[0] for k, b in bufs.items()}
    _lib.check(L.oryon_match_next_f32(_lib.ptr(a_hat), _lib.ptr(q_hat), B, Cp, cap_a, q_hat.shape[1], _lib.ptr(n_a), _lib.ptr(n_q),
                                      _lib.ptr(roi_q), roi_q.shape[1], c.W, r, _lib.ptr(prev), prev.shape[0], _lib.ptr(v["next_dist"]),
                                      _lib.ptr(v["next_argmin"]), _lib.ptr(ws), wsb, _lib.stream_ptr(DEV)), "oryon_match_next_f32")
    torch.cuda.synchronize()
    na = n_a.cpu().tolist()
    assert bool((ws_buf[max(wsb, 16):] == SENT[torch.uint8]).all()), "workspace: wrote past its end"
    out = {"split": wsb > 0}
    for k, (view, buf) in bufs.items():
        assert bool((buf[view.numel():] == SENT[buf.dtype]).all()), f"{k}: wrote past its end"
        for p in range(B):
            assert bool((view[p, na[p]:] == SENT[buf.dtype]).all()), f"{k}: pair {p} wrote rows >= its count"
        res = view.cpu().numpy()
        if order is not None:
            back = np.empty_like(res)
            back[np.asarray(order)] = res
            res = back
        out[k] = res
    return out


_chains = {}


def chain(c, r, K=4):
    """Ranks 2..K of every row by K - 1 calls, each reading the planes before it: -> (table [K,B,cap_a] i32 on the device, plane 0 =
    K1's argmin; [None, rank 2, rank 3, ...] results of run_next)."""
    key = (id(c), r, K)
    if key not in _chains:
        table = torch.full((K,) + tuple(c.am.shape), -5, dtype=torch.int32, device=DEV)
        table[0] = c.am
        got = [None]
        for k in range(1, K):
            g = run_next(c, r, table[:k])
            table[k] = torch.from_numpy(g["next_argmin"]).to(DEV)
            got.append(g)
        _chains[key] = (table, got)
    return _chains[key]


def candidates(c, p, prev_idx, r):
    """query rows of pair p outside the discs round the pixels of every index in prev_idx that names a row of the pair"""
    nq = c.nq[p]
    roi = c.roi_np[p, :nq].astype(np.int64)
    y, x = roi // c.W, roi % c.W
    ok = np.ones(nq, dtype=bool)
    for j in prev_idx:
        if 0 <= j < nq:
            ok &= (y - y[j]) ** 2 + (x - x[j]) ** 2 >= r * r
    return np.nonzero(ok)[0]


def yardstick(c, r, prev_np):
    """prev_np [n_prev, B, cap_a] -> {(p, i): (dist f32 scalar, index or -1)} from ONE call of the existing kernel ops.match."""
    from oryon_amd import ops
    todo = [(p, i) for p in range(c.B) for i in c.rows_under_test(p)]
    cands = [candidates(c, p, prev_np[:, p, i].tolist(), r) for p, i in todo]
    Bp, Cp = len(todo), c.a_hat.shape[2]
    a = torch.full((Bp, 128, Cp), float("nan"), device=DEV)
    q = torch.full((Bp, c.q_hat.shape[1], Cp), float("nan"), device=DEV)
    for b, ((p, i), js) in enumerate(zip(todo, cands)):
        a[b, 0] = c.a_hat[p, i]
        q[b, :len(js)] = c.q_hat[p, torch.from_numpy(js).to(DEV)]
    n_a = torch.ones(Bp, dtype=torch.int32, device=DEV)
    n_q = torch.tensor([len(js) for js in cands], dtype=torch.int32, device=DEV)
    md, am, _ = ops.match(a, q, n_a, n_q, 0.25)
    md, am = md[:, 0].cpu().numpy(), am[:, 0].cpu().numpy()
    out = {}
    for b, ((p, i), js) in enumerate(zip(todo, cands)):
        assert len(js) or np.isinf(md[b])
        out[(p, i)] = (md[b], int(js[am[b]]) if len(js) and np.isfinite(md[b]) else -1)
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def check_invariants(c, r, prev_np, got, tag):
    """what the definition implies for EVERY row: the index names a row of the pair outside all discs, (inf, -1) go together"""
    for p in range(c.B):
        n, nq = c.na[p], c.nq[p]
        d, j = got["next_dist"][p, :n], got["next_argmin"][p, :n]
        fin = np.isfinite(d)
        assert (j[~fin] == -1).all() and (j[fin] >= 0).all() and (j[fin] < max(nq, 1)).all(), tag
        if not nq:
            assert not fin.any(), tag
            continue
        roi = c.roi_np[p].astype(np.int64)
        for k in range(prev_np.shape[0]):
            pj = prev_np[k, p, :n]
            live = fin & (pj >= 0) & (pj < nq)
            dy, dx = roi[j[live]] // c.W - roi[pj[live]] // c.W, roi[j[live]] % c.W - roi[pj[live]] % c.W
            assert (dy * dy + dx * dx >= r * r).all(), f"{tag} pair {p}: an index inside the disc of rank {k + 1}"


# ------------------------------------------------------------------------------------------------ n_prev = 1: K1r's second minimum
def _equals_match_second(c, r, got=None):
    from oryon_amd import ops
    got = run_next(c, r, c.am[None]) if got is None else got
    sd, sa, _ = ops.match_second(c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q, c.W, r, c.md, c.am, None, 1.0)
    sd, sa = sd.cpu().numpy(), sa.cpu().numpy()
    for p in range(c.B):
        n = c.na[p]
        assert got["next_dist"][p, :n].tobytes() == sd[p, :n].tobytes(), f"C {c.C} r {r} pair {p}: next_dist is not second_dist"
        want = np.where(np.isinf(sd[p, :n]), -1, sa[p, :n])
        assert np.array_equal(got["next_argmin"][p, :n], want), f"C {c.C} r {r} pair {p}: next_argmin"
    return got


@pytest.mark.parametrize("r", [1, 5, 20])
@pytest.mark.parametrize("name", ["edges", "tiles"])
@pytest.mark.parametrize("C", WIDTHS)
def test_one_earlier_rank_is_the_second_minimum_of_the_existing_kernel(C, name, r):
    c = ms.case(C, name)
    got = _equals_match_second(c, r)
    assert got["split"]                                                   # B T = 12 < 8192: the query range is split, a merge ran
    check_invariants(c, r, c.am.cpu().numpy()[None], got, f"C {C} {name} r {r}")
    if name == "edges":
        assert np.isfinite(got["next_dist"][0, :300]).all()


# ------------------------------------------------------------------------------------------------ n_prev = 2, 3
@pytest.mark.parametrize("r", [1, 5, 20])
@pytest.mark.parametrize("C", WIDTHS)
def test_two_and_three_earlier_ranks_equal_the_existing_kernel_on_the_candidates(C, r):
    for name in ("edges", "tiles"):
        c = ms.case(C, name)
        table, got = chain(c, r)
        prev_np = table.cpu().numpy()
        for k in (2, 3):                                                  # n_prev = k: rank k + 1
            yard = yardstick(c, r, prev_np[:k])
            g = got[k]
            for (p, i), (want_d, want_j) in yard.items():
                tag = f"C {C} {name} r {r} n_prev {k} pair {p} row {i}"
                assert bits(g["next_dist"][p, i:i + 1])[0] == bits([want_d])[0], tag + ": next_dist"
                assert g["next_argmin"][p, i] == want_j, tag + f": next_argmin {g['next_argmin'][p, i]} != {want_j}"
            check_invariants(c, r, prev_np[:k], g, f"C {C} {name} r {r} n_prev {k}")
        for p in range(c.B):                                              # nested candidate sets: the ranks do not decrease
            n = c.na[p]
            d = [c.md[p, :n].cpu().numpy()] + [got[k]["next_dist"][p, :n] for k in (1, 2, 3)]
            if c.nq[p]:
                assert all((d[k + 1] >= d[k]).all() for k in range(3)), (C, name, r, p)
        if name == "edges" and r == 20:                                   # discs of 20 px in a ~30 x 31 map: some rows run out of candidates
            d4 = got[3]["next_dist"][0, :300]
            assert np.isinf(d4).any()
            gone = np.isinf(got[2]["next_dist"][0, :300])                 # ... and stay out: (inf, -1) from there on
            assert np.isinf(d4[gone]).all() and (got[3]["next_argmin"][0, :300][gone] == -1).all()


@pytest.mark.parametrize("C", [32, 512])
def test_the_chain_is_the_restatement_on_the_kernels_own_distances(C):
    """All rows of a pair at once against the numpy statement of the ranks.  The distance matrix is formed in float64 by torch (not
    K1's chain), so only rows whose forty best distances are more than 1e-5 apart - beyond what the two chains can differ by - are
    compared: the indices exactly, the distances to 2e-6."""
    c = ms.case(C, "edges")
    r = 5
    table, got = chain(c, r)
    n, nq = c.na[0], c.nq[0]
    a = torch.nan_to_num(c.a_hat[0, :n]).double()
    q = torch.nan_to_num(c.q_hat[0, :nq]).double()
    dist = (0.5 - 0.5 * (a @ q.T)).cpu().numpy()                          # the k-permutation is the same on both sides
    cd, ca = tr.ranks(dist, c.roi_np[0, :nq], c.W, r, 4)
    srt = np.sort(dist, axis=1)
    clear = (srt[:, 1:40] - srt[:, :39]).min(axis=1) > 1e-5               # no near-tie among the forty best: the order is beyond doubt
    assert clear.sum() > 50
    for k in (1, 2, 3):
        assert np.array_equal(got[k]["next_argmin"][0, :n][clear], ca[k][clear]), (C, k)
        assert np.allclose(got[k]["next_dist"][0, :n][clear], cd[k][clear], atol=2e-6, rtol=0)


# ------------------------------------------------------------------------------------------------ indices that name no row
@pytest.mark.parametrize("C", [32, 128, 512])
def test_an_earlier_rank_outside_the_pair_excludes_nothing(C):
    c = ms.case(C, "edges")
    r = 5
    one = run_next(c, r, c.am[None])
    none = torch.full_like(c.am, -1)
    past = (c.n_q[:, None] + 5).expand_as(c.am).contiguous()
    at_nq = c.n_q[:, None].expand_as(c.am).contiguous()
    for prev in (torch.stack([c.am, none, past]), torch.stack([none, c.am]), torch.stack([at_nq, none, c.am])):
        g = run_next(c, r, prev)
        for k in ("next_dist", "next_argmin"):
            assert g[k].tobytes() == one[k].tobytes(), (C, k)
    # nothing excluded at all: the scan is K1's - min_dist and argmin of the existing kernel, byte for byte
    free = run_next(c, r, torch.stack([none, past]))
    md, am = c.md.cpu().numpy(), c.am.cpu().numpy()
    for p in range(c.B):
        n = c.na[p]
        if c.nq[p]:
            assert free["next_dist"][p, :n].tobytes() == md[p, :n].tobytes() and np.array_equal(free["next_argmin"][p, :n], am[p, :n])
        else:
            assert np.isinf(free["next_dist"][p, :n]).all() and (free["next_argmin"][p, :n] == -1).all()


# ------------------------------------------------------------------------------------------------ the unsplit launch (S == 1)
@pytest.mark.parametrize("C", [32, 96])                                   # the register-resident and the LDS-staged kernel
def test_unsplit_launch_gives_the_bytes_of_the_split_one(C):
    """B T >= 8192 -> no query split: the scan itself writes the rank.  B = 4 pairs in a 262144-row capacity (2048 panels each, all
    but the first few leave at once); the same rows in the 512-row capacity take the split route.  Both must give the same bytes,
    for one, two and three earlier ranks."""
    from oryon_amd import _lib
    small = ms.case(C, "edges") if C == 32 else ms.Case(C, [300, 0, 129], [700, 255, 0], 31, 4242)
    big_cap = 2048 * 128
    L = _lib.lib()
    assert L.oryon_match_next_workspace_bytes(4, big_cap) == 0 and L.oryon_match_next_workspace_bytes(4, CAP_A) > 0
    r = 5
    table, got = chain(small, r)
    order = [0, 1, 2, 0]                                                  # four pairs: the three of the case and the first again
    big = ms.Case.__new__(ms.Case)
    big.W, big.C = small.W, C
    idx = torch.tensor(order, device=DEV)
    Cp = small.a_hat.shape[2]
    big.a_hat = torch.full((4, big_cap, Cp), float("nan"), device=DEV)
    big.a_hat[:, :CAP_A] = small.a_hat[idx]
    big.q_hat, big.roi_q, big.n_a, big.n_q = small.q_hat[idx].contiguous(), small.roi_q[idx].contiguous(), small.n_a[idx], small.n_q[idx]
    big_table = torch.full((4, 4, big_cap), -5, dtype=torch.int32, device=DEV)
    big_table[:, :, :CAP_A] = table[:, idx]
    for k in (1, 2, 3):
        g = run_next(big, r, big_table[:k])
        assert not g["split"] and got[k]["split"]                         # both routes occurred
        for b, p in enumerate(order):
            n = small.na[p]
            for key in ("next_dist", "next_argmin"):
                assert g[key][b, :n].tobytes() == got[k][key][p, :n].tobytes(), (C, k, b, key)
    del big


# ------------------------------------------------------------------------------------------------ repeatability, the entry point
@pytest.mark.parametrize("C", [32, 256, 512])
def test_runs_streams_batch_order_and_single_pairs_give_the_same_bytes(C):
    c = ms.case(C, "edges")
    r = 5
    table, got = chain(c, r)
    for k in (1, 3):
        prev = table[:k]
        one = got[k]
        two = run_next(c, r, prev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            three = run_next(c, r, prev)
        torch.cuda.current_stream().wait_stream(side)
        rev = run_next(c, r, prev, order=[2, 1, 0])
        for key in ("next_dist", "next_argmin"):
            assert one[key].tobytes() == two[key].tobytes() == three[key].tobytes(), (k, key)
            for p in range(c.B):
                assert rev[key][p, :c.na[p]].tobytes() == one[key][p, :c.na[p]].tobytes(), (k, key, p, "reversed batch")
        for p in (0, 2):                                                  # a pair alone (another split count) against its place in the ragged batch
            alone = run_next(c, r, prev, slice(p, p + 1))
            for key in ("next_dist", "next_argmin"):
                assert alone[key][0, :c.na[p]].tobytes() == one[key][p, :c.na[p]].tobytes(), (k, key, p)


def test_ops_match_next_is_the_entry_point():
    from oryon_amd import ops
    c = ms.case(128, "edges")
    table, got = chain(c, 5)
    d, j = ops.match_next(c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q, c.W, 5, table[:2])
    assert d.dtype == torch.float32 and j.dtype == torch.int32 and d.shape == j.shape == c.am.shape
    for p in range(3):
        assert d[p, :c.na[p]].cpu().numpy().tobytes() == got[2]["next_dist"][p, :c.na[p]].tobytes()
        assert j[p, :c.na[p]].cpu().numpy().tobytes() == got[2]["next_argmin"][p, :c.na[p]].tobytes()
    # into the next plane of a table, and what it would have to convert is refused
    plane_d, plane_j = torch.zeros_like(d), torch.zeros_like(j)
    ops.match_next(c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q, c.W, 5, table[:2], out=(plane_d, plane_j))
    assert torch.equal(plane_j[0, :300], j[0, :300])
    with pytest.raises(AssertionError):
        ops.match_next(c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q, c.W, 5, table[:2].long())
    with pytest.raises(AssertionError):
        ops.match_next(c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q.long(), c.W, 5, table[:2])
    with pytest.raises(AssertionError):
        ops.match_next(c.a_hat.half(), c.q_hat.half(), c.n_a, c.n_q, c.roi_q, c.W, 5, table[:2])
    with pytest.raises(AssertionError):
        ops.match_next(c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q, c.W, 5, c.am)          # a plane without its leading axis
