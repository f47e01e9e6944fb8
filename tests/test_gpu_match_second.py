"""GPU tests of the ratio test with an exclusion disc (csrc/match_second.hip) through oryon_match_second_f32 / ops.match_second.

The yardstick is the EXISTING kernel.  For the anchor rows under test one batch is built whose pair b holds anchor row i_b alone and
the query rows that are candidates of i_b (outside the disc round the pixel of its nearest row), compacted in order; ops.match runs
once on it.  K1's distance bits do not depend on a row's position, so second_dist must equal that min_dist byte for byte and
second_argmin its argmin mapped back through the compaction table.  At C = 32 and 256 the C oracle scores the same rows on the reduced
pixel list.  keep must equal the numpy statement (tests/ratio_restatement.py) applied to those.  Inputs sit in padded buffers whose
unused rows hold NaN (pixel lists: a huge index); outputs sit in guarded, sentinel-filled buffers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ratio_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
SENT = {torch.float32: -12345.0, torch.int32: -7, torch.uint8: 0xAB}
CAP_A, CAP_Q = 512, 768
COUNTS = {                                   # (n_a, n_q) per pair: the panel edge 127 / 128 / 129, the query tiles 255 / 256 / 257, empty sides
    "edges": ([300, 0, 129], [700, 255, 0]),
    "tiles": ([127, 128, 1], [257, 256, 1]),
    "one": ([300], [700]),
}


def guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENT[dtype], dtype=dtype, device=DEV)
    return buf[:n].view(*shape), buf


class Case:
    """A batch: anchors [B,C,1,300] with roi 0..n-1, a query MAP [B,C,H,W] with a ragged, row-major pixel list; K0's rows with NaN in
    every unused row; the existing kernel's min_dist / argmin / valid on them."""

    def __init__(self, C, na, nq, W, seed, edit=None):
        from oryon_amd import ops
        B = len(na)
        g = torch.Generator().manual_seed(seed)
        self.C, self.B, self.W, self.na, self.nq = C, B, W, na, nq
        self.H = H = (max(nq) * 13 // 10) // W + 2                    # ~75 % of the pixels are in the list: discs cut real holes
        self.fa = torch.randn(B, C, 1, 300, generator=g)
        self.fq = torch.randn(B, C, H, W, generator=g)
        roi = torch.full((B, CAP_Q), 0x7FFFFFF0, dtype=torch.int32)     # unused entries: an index far outside the map
        for p in range(B):
            roi[p, :nq[p]] = torch.sort(torch.randperm(H * W, generator=g)[:nq[p]])[0].to(torch.int32)
        self.roi_np = roi.numpy().copy()
        if edit:
            edit(self)
        self.roi_q = roi.to(DEV)
        self.n_a = torch.tensor(na, dtype=torch.int32, device=DEV)
        self.n_q = torch.tensor(nq, dtype=torch.int32, device=DEV)
        roi_a = torch.arange(300, dtype=torch.int32, device=DEV).repeat(B, 1).contiguous()
        self.a_hat = ops.gather_normalise(self.fa.to(DEV).contiguous(), roi_a, self.n_a, CAP_A)
        safe = self.roi_q.clamp(max=H * W - 1).contiguous()
        self.q_hat = ops.gather_normalise(self.fq.to(DEV).contiguous(), safe, self.n_q, CAP_Q)
        for p in range(B):
            self.a_hat[p, na[p]:] = float("nan")
            self.q_hat[p, nq[p]:] = float("nan")
        assert self.a_hat.shape[2] == (C + 31) // 32 * 32
        md, _, _ = ops.match(self.a_hat, self.q_hat, self.n_a, self.n_q, 0.25)
        live = [md[p, :na[p]] for p in range(B) if na[p] and nq[p]]
        self.thr = float(torch.cat(live).median()) if live else 0.25     # about half the rows valid; from the EXISTING kernel
        self.md, self.am, self.va = ops.match(self.a_hat, self.q_hat, self.n_a, self.n_q, self.thr)
        for p in range(B):                                               # rows >= n_a of the inputs are never read
            self.md[p, na[p]:] = float("nan")
            self.am[p, na[p]:] = -5
        self._yard = {}

    def candidates(self, p, i, r):
        roi = self.roi_np[p, :self.nq[p]].astype(np.int64)
        y, x = roi // self.W, roi % self.W
        if getattr(self, "_am_np", None) is None:
            self._am_np = self.am.cpu().numpy()
        j0 = int(self._am_np[p, i])
        return np.nonzero((y - y[j0]) ** 2 + (x - x[j0]) ** 2 >= r * r)[0]

    def rows_under_test(self, p):
        n = self.na[p]
        fixed = [0, 1, 31, 32, 33, 63, 64, 95, 96, 126, 127, 128, 129, 255, 256, n - 1]
        extra = np.random.default_rng(n).integers(0, max(n, 1), 6).tolist()
        return sorted({i for i in fixed + extra if 0 <= i < n}) if self.nq[p] else []

    def yardstick(self, r):
        """-> {(p, i): (second_dist f32 scalar, second_argmin)} from ONE call of the existing kernel."""
        from oryon_amd import ops
        if r in self._yard:
            return self._yard[r]
        todo = [(p, i) for p in range(self.B) for i in self.rows_under_test(p)]
        cands = [self.candidates(p, i, r) for p, i in todo]
        Bp, Cp = len(todo), self.a_hat.shape[2]
        a = torch.full((Bp, 128, Cp), float("nan"), device=DEV)
        q = torch.full((Bp, self.q_hat.shape[1], Cp), float("nan"), device=DEV)
        for b, ((p, i), js) in enumerate(zip(todo, cands)):
            a[b, 0] = self.a_hat[p, i]
            q[b, :len(js)] = self.q_hat[p, torch.from_numpy(js).to(DEV)]
        n_a = torch.ones(Bp, dtype=torch.int32, device=DEV)
        n_q = torch.tensor([len(js) for js in cands], dtype=torch.int32, device=DEV)
        md, am, _ = ops.match(a, q, n_a, n_q, 0.25)
        md, am = md[:, 0].cpu().numpy(), am[:, 0].cpu().numpy()
        out = {}
        for b, ((p, i), js) in enumerate(zip(todo, cands)):
            out[(p, i)] = (md[b], int(js[am[b]]) if len(js) and np.isfinite(md[b]) else 0)
            assert len(js) or np.isinf(md[b])
        self._yard[r] = out
        return out


def run_second(c, r, gate, ratio, sl=slice(None)):
    """oryon_match_second_f32 into guarded, sentinel-filled buffers -> dict of numpy arrays; guards and unwritten rows are checked here."""
    from oryon_amd import _lib
    L = _lib.lib()
    a_hat, q_hat, n_a, n_q, roi_q, md, am = (t[sl].contiguous() for t in (c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q, c.md, c.am))
    gate = None if gate is None else gate[sl].contiguous()
    B, cap_a, Cp = a_hat.shape
    spec = dict(second_dist=torch.float32, second_argmin=torch.int32, keep=torch.uint8)
    bufs = {k: guarded((B, cap_a), dt) for k, dt in spec.items()}
    wsb = L.oryon_match_second_workspace_bytes(B, cap_a)
    ws, ws_buf = guarded((max(wsb, 16),), torch.uint8)
    v = {k: b[0] for k, b in bufs.items()}
    _lib.check(L.oryon_match_second_f32(_lib.ptr(a_hat), _lib.ptr(q_hat), B, Cp, cap_a, q_hat.shape[1], _lib.ptr(n_a), _lib.ptr(n_q),
                                        _lib.ptr(roi_q), roi_q.shape[1], c.W, r, _lib.ptr(md), _lib.ptr(am), _lib.ptr(gate), float(ratio),
                                        _lib.ptr(v["second_dist"]), _lib.ptr(v["second_argmin"]), _lib.ptr(v["keep"]), _lib.ptr(ws), wsb,
                                        _lib.stream_ptr(DEV)), "oryon_match_second_f32")
    torch.cuda.synchronize()
    na = n_a.cpu().tolist()
    assert bool((ws_buf[max(wsb, 16):] == SENT[torch.uint8]).all()), "workspace: wrote past its end"
    out = {}
    for k, (view, buf) in bufs.items():
        assert bool((buf[view.numel():] == SENT[buf.dtype]).all()), f"{k}: wrote past its end"
        for p in range(B):
            assert bool((view[p, na[p]:] == SENT[buf.dtype]).all()), f"{k}: pair {p} wrote rows >= its count"
        out[k] = view.cpu().numpy()
    return out


def check(c, r, gate, ratio, got=None):
    got = run_second(c, r, gate, ratio) if got is None else got
    yard = c.yardstick(r)
    md, am = c.md.cpu().numpy(), c.am.cpu().numpy()
    g = None if gate is None else gate.cpu().numpy()
    for p in range(c.B):
        n = c.na[p]
        sd, sa, kp = got["second_dist"][p, :n], got["second_argmin"][p, :n], got["keep"][p, :n]
        tag = f"C {c.C} r {r} pair {p} (n_a {n}, n_q {c.nq[p]})"
        for i in c.rows_under_test(p):
            want_d, want_j = yard[(p, i)]
            assert sd[i:i + 1].view(np.uint32)[0] == np.array([want_d], dtype=np.float32).view(np.uint32)[0], f"{tag} row {i}: second_dist"
            assert sa[i] == want_j, f"{tag} row {i}: second_argmin {sa[i]} != {want_j}"
        # every row: the statement of keep on the outputs, and what the definition implies for them
        gp = None if g is None else g[p, :n]
        assert np.array_equal(kp.astype(bool), rr.keep_flags(md[p, :n], sd, gp, ratio)), tag + ": keep"
        assert set(np.unique(kp).tolist()) <= {0, 1}
        assert (sd >= md[p, :n]).all(), tag + ": a candidate beats the minimum"
        fin = np.isfinite(sd)
        assert not sa[~fin].any()
        if c.nq[p]:
            roi = c.roi_np[p].astype(np.int64)
            dy, dx = roi[sa[fin]] // c.W - roi[am[p, :n][fin]] // c.W, roi[sa[fin]] % c.W - roi[am[p, :n][fin]] % c.W
            assert (sa[fin] < c.nq[p]).all() and (dy * dy + dx * dx >= r * r).all(), tag + ": second_argmin inside the disc"
        else:
            assert not fin.any() and np.array_equal(kp.astype(bool), np.ones(n, bool) if gp is None else gp.astype(bool))
    return got


def ratio_from_the_existing_kernel(c, r):
    """A ratio that cuts about half of the rows under test: the median of min_dist / second over the yardstick's finite rows."""
    md = c.md.cpu().numpy()
    q = [md[p, i] / d for (p, i), (d, _) in c.yardstick(r).items() if np.isfinite(d) and d > 0]
    return float(np.clip(np.median(q), 0.05, 0.999)) if q else 0.8


_cases = {}


def case(C, name, W=31):
    key = (C, name, W)
    if key not in _cases:
        na, nq = COUNTS[name]
        _cases[key] = Case(C, na, nq, W, 1000 * C + len(name) + W)
    return _cases[key]


# ------------------------------------------------------------------------------------------------ widths, ragged counts, radii, gates
@pytest.mark.parametrize("name", ["edges", "tiles"])
@pytest.mark.parametrize("C", [32, 64, 128, 256, 512, 33, 96])           # every width path; 33 -> 64 and 96 un-padded / staged narrow
def test_second_minimum_equals_the_existing_kernel_on_the_candidates(C, name):
    from oryon_amd import ops
    c = case(C, name)
    r = 5
    ratio = ratio_from_the_existing_kernel(c, r)
    got = check(c, r, c.va, ratio)
    if name == "edges":
        k, v = got["keep"][0, :300].astype(bool), c.va[0, :300].cpu().numpy().astype(bool)
        assert 0 < k.sum() < v.sum() < 300                               # the case is not vacuous
    # gate = NULL and gate = mutual (from ops.match_mutual): second_* do not depend on the gate, keep follows it
    none = check(c, r, None, ratio)
    mut = ops.match_mutual(c.a_hat, c.q_hat, c.n_a, c.n_q, c.thr)[5]
    mu = check(c, r, mut, ratio)
    for k in ("second_dist", "second_argmin"):
        assert got[k].tobytes() == none[k].tobytes() == mu[k].tobytes()
    # ratio = 1: keep == gate byte for byte
    one = check(c, r, c.va, 1.0)
    for p in range(c.B):
        assert one["keep"][p, :c.na[p]].tobytes() == c.va[p, :c.na[p]].cpu().numpy().tobytes()


@pytest.mark.parametrize("r", [1, 2, 64])
@pytest.mark.parametrize("C,W", [(32, 24), (256, 40), (512, 31), (96, 37)])
def test_radii_one_pair_with_a_split_query_range(C, W, r):
    from oryon_amd import _lib
    c = case(C, "one", W)
    assert _lib.lib().oryon_match_workspace_bytes(1, CAP_A) > 0 and c.nq[0] > 2 * 256      # K1 splits this shape: several splits hold tiles
    ratio = ratio_from_the_existing_kernel(c, r)
    got = check(c, r, c.va, ratio)
    sd, sa = got["second_dist"][0, :300], got["second_argmin"][0, :300]
    if r == 64:                                                          # the disc covers the map: no candidate
        assert c.H < 46 and W < 46
        assert np.isinf(sd).all() and not sa.any()
        assert got["keep"][0, :300].tobytes() == c.va[0, :300].cpu().numpy().tobytes()
    else:
        assert np.isfinite(sd).all()
    if r == 1:                                                           # the classic test: only the best row itself is excluded
        assert (sa != c.am[0, :300].cpu().numpy()).all()


def test_a_single_query_row_has_no_competitor():
    c = case(64, "tiles")                                                # pair 2: n_a = n_q = 1
    got = check(c, 1, c.va, 0.5)
    assert np.isinf(got["second_dist"][2, 0]) and got["second_argmin"][2, 0] == 0 and got["keep"][2, 0] == c.va[2, 0].item()


def test_unsplit_launch_shape_many_pairs():
    """B T >= 8192 -> no query split (S = 1): the scan itself writes second_* and keep.  Rows are made directly (unit rows of random
    normals): the yardstick runs on the same rows."""
    from oryon_amd import _lib, ops
    B, cap_a, cap_q, W = 512, 2048, 256, 24
    assert _lib.lib().oryon_match_workspace_bytes(B, cap_a) == 0 and _lib.lib().oryon_match_second_workspace_bytes(B, cap_a) == 0
    g = torch.Generator(device=DEV).manual_seed(5)
    gc = torch.Generator().manual_seed(6)
    for C in (32, 96):                                                   # the register-resident and the LDS-staged kernel
        c = Case.__new__(Case)
        c.C, c.B, c.W, c.H, c._yard = C, B, W, 12, {}
        n_a = torch.randint(0, 300, (B,), generator=g, device=DEV, dtype=torch.int32)
        n_a[::7] = torch.randint(1800, cap_a + 1, (len(n_a[::7]),), generator=g, device=DEV, dtype=torch.int32)
        n_q = torch.randint(0, 257, (B,), generator=g, device=DEV, dtype=torch.int32)
        c.na, c.nq, c.n_a, c.n_q = n_a.cpu().tolist(), n_q.cpu().tolist(), n_a, n_q
        roi = torch.full((B, cap_q), 0x7FFFFFF0, dtype=torch.int32)
        for p in range(B):
            roi[p, :c.nq[p]] = torch.sort(torch.randperm(W * c.H, generator=gc)[:c.nq[p]])[0].to(torch.int32)
        c.roi_np, c.roi_q = roi.numpy().copy(), roi.to(DEV)
        a_hat = torch.nn.functional.normalize(torch.randn(B, cap_a, C, generator=g, device=DEV), dim=2)
        q_hat = torch.nn.functional.normalize(torch.randn(B, cap_q, C, generator=g, device=DEV), dim=2)
        rows_a = torch.arange(cap_a, device=DEV)[None, :, None] >= n_a[:, None, None]
        rows_q = torch.arange(cap_q, device=DEV)[None, :, None] >= n_q[:, None, None]
        c.a_hat = torch.where(rows_a, torch.full_like(a_hat, float("nan")), a_hat).contiguous()
        c.q_hat = torch.where(rows_q, torch.full_like(q_hat, float("nan")), q_hat).contiguous()
        c.thr = 0.25 if C == 32 else 0.4
        c.md, c.am, c.va = ops.match(c.a_hat, c.q_hat, n_a, n_q, c.thr)
        # the yardstick's rows: a few pairs (a large one, an empty one if the draw has one), a few rows of each
        pairs = [0, 7, 8, 300, 511] + [p for p in range(B) if c.nq[p] == 0][:1]
        c.rows_under_test = lambda p, c=c, pairs=pairs: ([i for i in (0, 1, 127, 128, c.na[p] - 1) if 0 <= i < c.na[p]]
                                                          if p in pairs and c.nq[p] else [])
        check(c, 3, c.va, 0.9)


@pytest.mark.parametrize("C", [32, 256])
def test_against_the_c_oracle_on_the_reduced_pixel_list(C):
    from oracle import c_oracle
    c = case(C, "edges")
    r = 5
    got = check(c, r, c.va, 0.9)
    ra = np.arange(300, dtype=np.int32)
    for p in (0, 2):
        for i in c.rows_under_test(p)[::3]:
            js = c.candidates(p, i, r)
            if not len(js):
                continue
            fa = torch.zeros(C, c.H * c.W)                                # the oracle takes two maps of one size: the anchors' padded
            fa[:, :300] = c.fa[p, :, 0]
            md, am, _ = c_oracle.match_lin(fa.reshape(C, c.H, c.W).numpy(), c.fq[p].numpy(), ra, c.roi_np[p, js], 0.25, anchor_rows=[i])
            assert got["second_dist"][p, i:i + 1].view(np.uint32)[0] == md.view(np.uint32)[0], (p, i)
            assert got["second_argmin"][p, i] == js[am[0]], (p, i)


# ------------------------------------------------------------------------------------------------ exact ties
def _pixel_dist2(c, p, j, k):
    a, b = int(c.roi_np[p, j]), int(c.roi_np[p, k])
    return (a // c.W - b // c.W) ** 2 + (a % c.W - b % c.W) ** 2


@pytest.mark.parametrize("C", [32, 128, 512])
def test_copies_of_the_best_row_inside_and_outside_the_disc(C):
    r = 5
    picked = {}

    def edit(c):
        g = torch.Generator().manual_seed(77 + C)
        roi = c.roi_np[0, :700].astype(np.int64)
        y, x = roi // c.W, roi % c.W
        fq = c.fq[0].reshape(C, -1)
        # anchor 10 -> query row 400 with a copy INSIDE the disc only; anchor 200 -> query row 300 with copies inside and OUTSIDE
        for i, j in ((10, 400), (200, 300)):
            d2 = (y - y[j]) ** 2 + (x - x[j]) ** 2
            inside = int(np.nonzero((d2 > 0) & (d2 < r * r) & (np.arange(700) > j))[0][0])
            outside = int(np.nonzero((d2 >= r * r) & (np.arange(700) > j + 130))[0][0])
            c.fa[0, :, 0, i] = fq[:, roi[j]] + 0.02 * torch.randn(C, generator=g)
            fq[:, roi[inside]] = fq[:, roi[j]]
            if i == 200:
                fq[:, roi[outside]] = fq[:, roi[j]]
            picked[i] = (j, inside, outside)
        c.fq[0] = fq.reshape(C, c.H, c.W)

    c = Case(C, [300], [700], 31, 500 + C, edit)
    got = check(c, r, c.va, 0.999)
    md, am = c.md[0].cpu().numpy(), c.am[0].cpu().numpy()
    j, inside, outside = picked[10]
    assert am[10] == j and md[10] > 0 and _pixel_dist2(c, 0, j, inside) < r * r
    assert got["second_dist"][0, 10] > md[10] and got["second_argmin"][0, 10] not in (j, inside)       # the copy inside is excluded
    j, inside, outside = picked[200]
    assert am[200] == j and md[200] > 0 and _pixel_dist2(c, 0, j, outside) >= r * r
    assert got["second_dist"][0, 200:201].view(np.uint32)[0] == md[200:201].view(np.uint32)[0]         # the copy outside: the same bits
    assert got["second_argmin"][0, 200] == outside
    assert c.va[0, 200].item() == 1 and got["keep"][0, 200] == 0                                        # rejected at any ratio < 1
    assert run_second(c, r, c.va, 1.0)["keep"][0, 200] == 1


@pytest.mark.parametrize("C", [32, 64, 256, 512])
def test_equal_candidates_go_to_the_first_index_across_tile_and_split_edges(C):
    r = 2
    pairs = {20: (60, 70), 21: (120, 130), 22: (250, 260), 150: (383, 384)}      # anchor -> two equal query rows across a 64 / 128 / 256 / split edge
    best = {20: 500, 21: 520, 22: 540, 150: 560}

    def edit(c):
        g = torch.Generator().manual_seed(99 + C)
        roi = c.roi_np[0, :700].astype(np.int64)
        fq = c.fq[0].reshape(C, -1)
        for i, (j1, j2) in pairs.items():
            x = torch.randn(C, generator=g)
            c.fa[0, :, 0, i] = x
            fq[:, roi[best[i]]] = x + 0.02 * torch.randn(C, generator=g)
            fq[:, roi[j1]] = fq[:, roi[j2]] = x + 0.2 * torch.randn(C, generator=g)
        c.fq[0] = fq.reshape(C, c.H, c.W)

    c = Case(C, [300], [700], 31, 900 + C, edit)
    got = check(c, r, None, 0.9)
    am = c.am[0].cpu().numpy()
    for i, (j1, j2) in pairs.items():
        assert am[i] == best[i] and _pixel_dist2(c, 0, best[i], j1) >= r * r and _pixel_dist2(c, 0, best[i], j2) >= r * r
        assert got["second_argmin"][0, i] == j1, (i, got["second_argmin"][0, i])


# ------------------------------------------------------------------------------------------------ repeatability, the entry point
@pytest.mark.parametrize("C", [32, 256, 512])
def test_runs_positions_and_streams_give_the_same_bytes(C):
    c = case(C, "edges")
    one = run_second(c, 5, c.va, 0.9)
    two = run_second(c, 5, c.va, 0.9)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        three = run_second(c, 5, c.va, 0.9)
    for k in one:
        assert one[k].tobytes() == two[k].tobytes() == three[k].tobytes(), k
    for p in (0, 2):                                                     # a pair alone (another split count) against its place in the batch
        alone = run_second(c, 5, c.va, 0.9, slice(p, p + 1))
        for k in one:
            assert alone[k][0, :c.na[p]].tobytes() == one[k][p, :c.na[p]].tobytes(), (k, p)


def test_ops_match_second_is_the_entry_point():
    from oryon_amd import ops
    c = case(128, "edges")
    want = run_second(c, 5, c.va, 0.9)
    got = ops.match_second(c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q, c.W, 5, c.md, c.am, c.va, 0.9)
    assert len(got) == 3 and [t.dtype for t in got] == [torch.float32, torch.int32, torch.uint8]
    for k, t in zip(("second_dist", "second_argmin", "keep"), got):
        for p in range(3):
            assert t[p, :c.na[p]].cpu().numpy().tobytes() == want[k][p, :c.na[p]].tobytes(), (k, p)
    free = ops.match_second(c.a_hat, c.q_hat, c.n_a, c.n_q, c.roi_q, c.W, 5, c.md, c.am, None, 0.9)[2]
    assert bool((free[0, :300] >= got[2][0, :300]).all())
