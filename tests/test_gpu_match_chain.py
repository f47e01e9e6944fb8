"""The small kernels between the screens on the match stream: both radix selects (post.hip select_corrs_kernel, roi.hip
roi_subsample_kernel: one bin walk, common.h radix_pick, done by a wave), the matcher's merged zero fills and its launches folded into
their neighbours (match_corrs.hip, match_x3.hip, gather8.hip).

References are Python restatements of the rule, not another HIP path.  Selection: "the max smallest keys among the n entries, ties to the
lower index, emitted in order", keys = rng_u32(seed, key, stream, i) with i the entry's position (csrc/common.h; the scalar statement is
tests/ransac_restatement.py's, the array form below is checked against it).  Matcher: the C oracle's exact scan, and the same call on
another workspace / in another batch."""
import numpy as np
import pytest
import torch

from ransac_restatement import rng_u32

pytestmark = pytest.mark.gpu

SEED = 0x5EED1234ABCD
OK, NO_MASK, NO_CORR = 0, 1, 2


def mix64_np(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def keys_np(seed, key, stream, n):
    """[n] uint32: rng_u32(seed, key, stream, i) for i < n"""
    with np.errstate(over="ignore"):
        base = mix64_np(np.array([seed], np.uint64) ^ (np.array([key], np.uint64) * np.uint64(0xD1B54A32D192ED03)))
        ctr = (np.uint64(stream) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        return (mix64_np(base + ctr) >> np.uint64(32)).astype(np.uint32)


def test_array_keys_are_the_scalar_restatement():
    for seed, key, stream in ((SEED, 0, 0), (SEED, 12345, 1), (1, 2**40 + 3, 2)):
        k = keys_np(seed, key, stream, 40)
        assert [int(v) for v in k] == [rng_u32(seed, key, stream, i) for i in range(40)]


def smallest_in_order(keys, keep):
    """positions of the `keep` smallest keys, ties to the lower position, ascending"""
    return np.sort(np.argsort(keys, kind="stable")[:keep])


# ------------------------------------------------------------------------------------------------------------------ select_corrs
CAP_A, W_MAP, N_PAIRS = 1024, 40, 64


def _select_case(nv, case):
    g = np.random.default_rng(100 + case)
    roi_a = np.stack([np.sort(g.choice(W_MAP * W_MAP, CAP_A, replace=False)) for _ in range(N_PAIRS)]).astype(np.int32)
    roi_q = np.stack([np.sort(g.choice(W_MAP * W_MAP, CAP_A, replace=False)) for _ in range(N_PAIRS)]).astype(np.int32)
    n_q = g.integers(CAP_A // 2, CAP_A + 1, N_PAIRS).astype(np.int32)
    argmin = (g.integers(0, 1 << 30, (N_PAIRS, CAP_A)) % n_q[:, None]).astype(np.int32)
    valid = np.zeros((N_PAIRS, CAP_A), np.uint8)
    for p in range(N_PAIRS):
        valid[p, g.choice(CAP_A, nv, replace=False)] = 1
    key = (np.arange(N_PAIRS, dtype=np.int64) * 7919 + 1000003 * case)
    return roi_a, roi_q, n_q, argmin, valid, key


def _select_restated(roi_a, roi_q, argmin, valid, key, max_corrs):
    corrs = np.zeros((N_PAIRS, max_corrs, 4), np.int32)
    n_valid, n_sel, status = (np.zeros(N_PAIRS, np.int32) for _ in range(3))
    for p in range(N_PAIRS):
        rows = np.nonzero(valid[p])[0]
        nv = len(rows)
        n_valid[p] = nv
        status[p] = OK if nv > 1 else NO_CORR
        if nv <= 1:
            continue
        n_sel[p] = max_corrs
        if nv < max_corrs:          # with replacement: max_corrs uniform draws
            pick = (keys_np(SEED, int(key[p]), 2, max_corrs).astype(np.uint64) * np.uint64(nv)) >> np.uint64(32)
            sel = rows[pick.astype(np.int64)]
        else:
            sel = rows[smallest_in_order(keys_np(SEED, int(key[p]), 1, nv), max_corrs)]
        pa, pq = roi_a[p, sel], roi_q[p, argmin[p, sel]]
        corrs[p] = np.stack([pa // W_MAP, pa % W_MAP, pq // W_MAP, pq % W_MAP], 1)
    return corrs, n_valid, n_sel, status


@pytest.mark.parametrize("max_corrs", [500, 1])
@pytest.mark.parametrize("nv", [0, 1, 2, 499, 500, 501, 1000, 1023])
def test_select_corrs_equals_the_restatement(nv, max_corrs):
    from oryon_amd import ops
    roi_a, roi_q, n_q, argmin, valid, key = _select_case(nv, nv * 2 + (max_corrs == 1))
    dev = "cuda"
    t = lambda a: torch.from_numpy(a).to(dev)
    n_a = torch.full((N_PAIRS,), CAP_A, dtype=torch.int32, device=dev)
    corrs, n_valid, n_sel, status = ops.select_corrs(t(roi_a), t(roi_q), n_a, t(n_q), t(argmin), t(valid), W_MAP, max_corrs, SEED, t(key))
    want = _select_restated(roi_a, roi_q, argmin, valid, key, max_corrs)
    for name, got, ref in zip(("corrs", "n_valid", "n_sel", "status"), (corrs, n_valid, n_sel, status), want):
        assert np.array_equal(got.cpu().numpy(), ref), (name, nv, max_corrs)
    # (64 pair keys per case: the walks end in many different bins - the first occupied one at max_corrs = 1, the last at nv = max_corrs)


# ---------------------------------------------------------------------------------------------------------------- roi_subsample_
@pytest.mark.parametrize("n,max_keep", [(4999, 5000), (5000, 5000), (5001, 5000), (12544, 5000), (50176, 5000), (7, 8), (8, 8), (9, 8)])
def test_roi_subsample_equals_the_restatement(n, max_keep):
    from oryon_amd import ops
    n_maps, stride = 16, n + 3
    g = np.random.default_rng(n)
    roi = np.stack([np.sort(g.choice(4 * n + 64, stride, replace=False)) for _ in range(n_maps)]).astype(np.int32)
    key = np.arange(n_maps, dtype=np.int64) * 104729 + n
    roi_d = torch.from_numpy(roi).cuda()
    count = torch.full((n_maps,), n, dtype=torch.int32, device="cuda")
    ops.roi_subsample_(roi_d, count, max_keep, SEED, torch.from_numpy(key).cuda())
    got, got_n = roi_d.cpu().numpy(), count.cpu().numpy()
    if n <= max_keep:
        assert np.array_equal(got, roi) and (got_n == n).all(), "a list at or below max_keep is left untouched"
        return
    assert (got_n == max_keep).all(), got_n
    for m in range(n_maps):
        keep = smallest_in_order(keys_np(SEED, int(key[m]), 0, n), max_keep)
        assert np.array_equal(got[m, :max_keep], roi[m, keep]), (n, m)


# --------------------------------------------------------------------------------------------- the default-route matcher, cascade on
H, C = 96, 256                       # 2304 anchors of the centred mask: cap_a = 2304 > 2048, three panels - the cascade's shape gate
MAX_CORRS, CORR_ROWS, THR = 500, 512, 0.25
NAMES = ("corrs", "n_valid", "n_sel", "status", "min_dist", "argmin", "valid")
_cache = {}


def _pairs():
    """two Gaussian pairs and a smooth one (the second level does real work for it beside two pairs that skip it); built once"""
    if "pairs" not in _cache:
        from oryon_amd.synth import make_pair
        _cache["pairs"] = [make_pair(900, H, H, C, device="cuda"), make_pair(901, H, H, C, device="cuda"),
                           make_pair(700, H, H, C, device="cuda", smooth=0.02)]
    return _cache["pairs"]


def _match(pairs, keys, poison=None):
    """oryon_match_corrs_mx6_araw on K0's operands of these pairs -> dict of the outputs, n_undecided and the ROI lists.
    poison: byte the (cached, per-stream) workspace is filled with before the call."""
    from oryon_amd import ops, _lib
    st = lambda k: torch.stack([p[k] for p in pairs]).contiguous()
    fa, fq = st("feat_a"), st("feat_q")
    roi_a, na = ops.roi_compact(st("mask_a"))
    roi_q, nq = ops.roi_compact(st("mask_q"))
    cap_a, cap_q = ops.round_up(int(na.max()), 256), ops.round_up(int(nq.max()), 256)
    assert cap_a > 2048
    a6, a_err, a_norm, _ = ops.gather_mx6(fa, roi_a, na, cap_a, C)
    q6, q_err, q_norm, _ = ops.gather_mx6(fq, roi_q, nq, cap_q, C)
    B = len(pairs)
    und = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    key = torch.tensor(keys, dtype=torch.int64, device="cuda")
    if poison is not None:
        wsb = _lib.lib().oryon_match_corrs_i8_workspace_bytes(B, C, cap_a, cap_q, CORR_ROWS)
        with ops._raw_ws_lock:
            ops._cached_raw_ws(torch.device("cuda", torch.cuda.current_device()), wsb).fill_(poison)
    out = ops._match_corrs("oryon_match_corrs_mx6_araw", None, fa, a_norm, a6, (a_err,), fq, roi_a, roi_q, q_norm, q6, (q_err,), na, nq, THR, H,
                           MAX_CORRS, SEED, key, CORR_ROWS, und, False, cached_ws=poison is not None)
    torch.cuda.synchronize()
    r = dict(zip(NAMES, (o.cpu().numpy() for o in out)))
    r.update(n_undecided=und.cpu().numpy(), n_a=na.cpu().numpy(), n_q=nq.cpu().numpy(), roi_a=roi_a.cpu().numpy(), roi_q=roi_q.cpu().numpy())
    return r


def _same_pair(x, bx, y, by, what):
    """pair bx of result x against pair by of result y: every output over the pair's live rows, bit for bit"""
    n = int(x["n_a"][bx])
    assert n == int(y["n_a"][by])
    for k in ("n_valid", "n_sel", "status", "n_undecided"):
        assert x[k][bx] == y[k][by], (what, k, x[k][bx], y[k][by])
    ns = int(x["n_sel"][bx])
    assert np.array_equal(x["corrs"][bx, :ns], y["corrs"][by, :ns]), (what, "corrs")
    assert np.array_equal(x["valid"][bx, :n], y["valid"][by, :n]), (what, "valid")
    assert np.array_equal(x["argmin"][bx, :n], y["argmin"][by, :n]), (what, "argmin")
    assert np.array_equal(x["min_dist"][bx, :n].view(np.uint32), y["min_dist"][by, :n].view(np.uint32)), (what, "min_dist")


KEYS3 = (900, 901, 700)


def test_poisoned_workspace_changes_nothing():
    """what the call needs zeroed it zeroes itself: a region the merged fills miss shows as a difference (or a count gone wild)"""
    pairs = _pairs()
    r0, r1 = _match(pairs, KEYS3, poison=0), _match(pairs, KEYS3, poison=0xFF)
    for b in range(3):
        _same_pair(r0, b, r1, b, f"pair {b}, zeroed against 0xFF workspace")
    assert (r0["status"] == OK).all() and (r0["n_sel"] == MAX_CORRS).all()
    assert (r0["n_undecided"] >= 0).all() and (r0["n_undecided"] <= r0["n_a"]).all(), r0["n_undecided"]


def test_batch_of_three_equals_three_batches_of_one_and_the_oracle():
    from oracle import c_oracle
    pairs = _pairs()
    r3 = _match(pairs, KEYS3)
    for b in range(3):
        r1 = _match([pairs[b]], [KEYS3[b]])
        _same_pair(r3, b, r1, 0, f"pair {b}, batch of three against batch of one")
    print("n_undecided", r3["n_undecided"].tolist(), "n_valid", r3["n_valid"].tolist())
    assert r3["n_undecided"][2] > 0, "the smooth pair keeps ambiguous rows after the complete pass: the second level ran for it"
    for b, p in enumerate(pairs):
        n_a, n_q = int(r3["n_a"][b]), int(r3["n_q"][b])
        roi_a, roi_q = r3["roi_a"][b, :n_a], r3["roi_q"][b, :n_q]
        _, am, va = c_oracle.match_lin(p["feat_a"].cpu().numpy(), p["feat_q"].cpu().numpy(), roi_a, roi_q, THR)
        assert np.array_equal(r3["valid"][b, :n_a].astype(bool), va.astype(bool)), f"pair {b}: valid set differs from the C oracle"
        rows = np.nonzero(va)[0]
        assert int(r3["n_valid"][b]) == len(rows) >= MAX_CORRS, "the pairs of this test sample without replacement"
        sel = rows[smallest_in_order(keys_np(SEED, KEYS3[b], 1, len(rows)), MAX_CORRS)]
        pa, pq = roi_a[sel], roi_q[am[sel]]
        want = np.stack([pa // H, pa % H, pq // H, pq % H], 1)
        assert np.array_equal(r3["corrs"][b, :MAX_CORRS], want), f"pair {b}: corrs differ from (oracle valid set, restated draw, oracle argmin)"
