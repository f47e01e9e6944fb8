"""Anchor rows on demand: the `_araw` matcher entries (oryon_match_corrs_i8_araw / _mx6_araw / _mx6_x3_araw) take the raw anchor map and
K0's anchor norms instead of the materialised fp32 unit rows a_hat, and must return what the entries without the suffix return on the
same K0 outputs - corrs, n_valid, n_sel, status, valid, min_dist, argmin - bit for bit (NaN positions included).  Rows at or beyond a
pair's anchor count are written by neither entry and are left out of the comparison."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("oryon_match_corrs_i8_araw", "oryon_match_corrs_mx6_araw", "oryon_match_corrs_mx6_x3_araw")
NAMES = ("corrs", "n_valid", "n_sel", "status", "min_dist", "argmin", "valid")


def test_new_entries_are_declared_bound_and_exported():
    from oryon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "oryon_hip.h")).read()
    declared = set(re.findall(r"\b(oryon_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/oryon_hip.h"
        assert name in _lib.EXPORTS, f"{name} has no ctypes prototype in oryon_amd/_lib.py"
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        for name in NEW:
            assert hasattr(L, name), f"{name} is not exported by the built library"
        # no launch is reached without the map / the norms, and the lazy-only entries have no force_eager to offer
        assert L.oryon_match_corrs_mx6_araw(*([None] * 5), 256, 16, 0, None, 16, None, 16, None, None, None, 1, 256, 256, 256, None, None, 0.25,
                                            4, 8, 8, 0, *([None] * 9), 0, None, 0, None) == -1
        assert b"invalid argument" in L.oryon_last_error()


def test_touched_kernels_do_not_spill():
    """The anchor pass the engine launches now (gather_mx6_v4_kernel<false, false>) and every kernel that forms anchor rows on demand keep
    their working set in registers - the mechanism of test_hot_kernels_do_not_spill (tools/check_kernel_resources.py on the built objects)."""
    import glob
    import sys
    if not glob.glob(os.path.join(ROOT, "oryon_amd", "csrc", "*.o")):
        pytest.skip("objects not built in this tree")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_kernel_resources as ckr
    rows = ckr.report()
    if not rows:
        pytest.skip("LLVM object tools not available")
    touched = ("gather_mx6_v4_kernelILb0ELb0E", "gather_mx6_v4_kernelILb1ELb0E", "gather_mx6_v4_kernelILb0ELb1E",
               "match_resolve_selected_kernelILb0ELi0E", "match_resolve_selected_kernelILb0ELi1E", "match_resolve_selected_kernelILb1ELi0E",
               "match_resolve_selected_kernelILb1ELi1E", "match_resolve_uncertain_kernelILb0ELi0E", "match_resolve_uncertain_kernelILb0ELi1E",
               "match_resolve_uncertain_kernelILb1ELi0E", "match_resolve_uncertain_kernelILb1ELi1E", "match_compact_raw_kernelILb0E",
               "match_compact_raw_kernelILb1E", "match_compact_f32_kernel")
    seen = set()
    for k in rows:
        for t in touched:
            if t in k["name"]:
                seen.add(t)
                assert k["spill"] == 0 and k["scratch"] == 0, f"{k['name']}: {k['spill']} spilled registers, {k['scratch']} B of scratch per lane"
    assert seen == set(touched), sorted(set(touched) - seen)


# ------------------------------------------------------------------------------------------------------------------------------ inputs
def _stack(pairs):
    st = lambda k: torch.stack([p[k] for p in pairs]).contiguous()
    return st("feat_a"), st("feat_q"), st("mask_a"), st("mask_q")


def _near_duplicate_pair(index, H, W, C, dev):
    """A Gaussian pair of the generator with (a) every 16th query pixel copied, + 1e-3 N(0,1), onto the pixel 8 further on: the anchor that
    matches the original now has two query rows no 6- / 8-bit screen separates (ambiguous), and (b) 1.7 N(0,1) added to the anchors of the
    lower half of the anchor mask: their best cosine sits at 1 / sqrt(1 + 1.7^2) = 0.507, on the validity cut 1 - 2 x 0.25 (validity open:
    resolved exactly before the sampling)."""
    from oryon_amd.synth import make_pair
    p = make_pair(index, H, W, C, device=dev)
    g = torch.Generator(device=dev).manual_seed(4242 + index)
    fq = p["feat_q"].reshape(C, H * W).clone()
    src = torch.arange(0, H * W - 8, 16, device=dev)
    fq[:, src + 8] = fq[:, src] + 1e-3 * torch.randn(C, src.numel(), generator=g, device=dev)
    fa = p["feat_a"].clone()
    fa[:, H // 2:, :] += 1.7 * torch.randn(C, H - H // 2, W, generator=g, device=dev)
    return dict(p, feat_a=fa, feat_q=fq.reshape(C, H, W))


def _mixed(H, C, dev, smooth_index=500):
    from oryon_amd.synth import make_pair
    return [make_pair(11, H, H, C, device=dev), make_pair(smooth_index, H, H, C, device=dev, smooth=0.02), _near_duplicate_pair(12, H, H, C, dev)]


# ---------------------------------------------------------------------------------------------------------------------------- the check
def _gather_mx6_x3(feat, roi, count, rows_cap, round_f16):
    """oryon_gather_mx6_x3 (C_pad 256): -> (mx6 rows, err_max, row_norm, hi | lo half rows, lo_sq_max)."""
    from oryon_amd import _lib, ops
    dev = feat.device
    feat, layout = ops.map_layout(feat)
    n, C, H, W = feat.shape
    out6 = torch.empty((n, rows_cap, 256), dtype=torch.uint8, device=dev)
    err = torch.empty((n,), dtype=torch.float32, device=dev)
    norm = torch.empty((n, rows_cap), dtype=torch.float32, device=dev)
    hilo = torch.zeros((2, n, rows_cap, 256), dtype=torch.float16, device=dev)
    lo_max = torch.empty((n,), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().oryon_gather_mx6_x3(feat.data_ptr(), n, C, H * W, layout, _lib.ptr(roi), roi.shape[1], _lib.ptr(count), rows_cap, 256,
                                              _lib.ptr(out6), _lib.ptr(err), _lib.ptr(norm), _lib.ptr(hilo), _lib.ptr(lo_max), int(round_f16),
                                              _lib.stream_ptr(dev)), "oryon_gather_mx6_x3")
    return out6, err, norm, hilo, lo_max


def _match_corrs_mx6_x3(a_hat, a6, a_err, feat_q, roi_a, roi_q, q_norm, q6, q_err, hilo, lo_max, n_a, n_q, thr, W, max_corrs, seed, key, corr_rows,
                        und, round_f16):
    """oryon_match_corrs_mx6_x3, the entry on materialised anchor rows (oryon_amd.ops has no wrapper: only the engine calls it)."""
    from oryon_amd import _lib, ops
    dev = a_hat.device
    feat_q, layout = ops.map_layout(feat_q)
    B, cap_a, Cp = a_hat.shape
    cap_q = q6.shape[1]
    C_true, HW = feat_q.shape[1], feat_q.shape[2] * feat_q.shape[3]
    P = _lib.ptr
    md = torch.empty((B, cap_a), dtype=torch.float32, device=dev)
    am = torch.empty((B, cap_a), dtype=torch.int32, device=dev)
    va = torch.empty((B, cap_a), dtype=torch.uint8, device=dev)
    corrs = torch.zeros((B, corr_rows, 4), dtype=torch.int32, device=dev)
    n_valid, n_sel, status = (torch.empty((B,), dtype=torch.int32, device=dev) for _ in range(3))
    ws = torch.empty((max(_lib.lib().oryon_match_corrs_i8_workspace_bytes(B, Cp, cap_a, cap_q, corr_rows), 16),), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().oryon_match_corrs_mx6_x3(P(a_hat), P(a6), P(a_err), feat_q.data_ptr(), C_true, HW, layout, P(roi_a), roi_a.shape[1],
                                                   P(roi_q), roi_q.shape[1], P(q_norm), P(q6), P(q_err), P(hilo), P(lo_max), B, Cp, cap_a, cap_q,
                                                   P(n_a), P(n_q), float(thr), int(W), int(max_corrs), corr_rows, int(seed), P(key), P(md), P(am),
                                                   P(va), P(corrs), P(n_valid), P(n_sel), P(status), P(und), int(round_f16), P(ws), ws.numel(),
                                                   _lib.stream_ptr(dev)), "oryon_match_corrs_mx6_x3")
    return corrs, n_valid, n_sel, status, md, am, va


def _same(old, new, n_a, what):
    """Every output equal, NaN positions included; per-anchor arrays on the rows either entry writes (row < n_a of the pair)."""
    cap_a = old[4].shape[1]
    live = torch.arange(cap_a, device=n_a.device)[None, :] < n_a[:, None]
    for name, x, y in zip(NAMES, old, new):
        if x.dim() == 2 and x.shape[1] == cap_a and name != "corrs":
            x, y = torch.where(live, x, torch.zeros_like(x)), torch.where(live, y, torch.zeros_like(y))
        if x.is_floating_point():
            assert torch.equal(torch.isnan(x), torch.isnan(y)), f"{what}: {name} has NaNs in different places"
            x, y = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)
        assert torch.equal(x, y), f"{what}: {name} differs ({int((x != y).sum())} elements)"


def _old_vs_new(fa, fq, ma, mq, C_pad, routes, thr=0.25, max_corrs=500, subsample=None, channels_last=False, round_f16=False):
    """One K0 pass per operand format, then the entry on a_hat and the `_araw` entry on (feat_a, a_norm) with the same operands.
    Returns {route: (outputs of the new entry, n_undecided)} and the exact (min_dist, argmin) of every anchor."""
    from oryon_amd import ops
    dev = fa.device
    roi_a, na = ops.roi_compact(ma)
    roi_q, nq = ops.roi_compact(mq)
    if subsample:
        ops.roi_subsample_(roi_a, na, subsample, seed=3)
    B, C, H, W = fa.shape
    cap_a = ops.round_up(max(1, int(na.max())), 256)
    cap_q = ops.round_up(max(1, int(nq.max())), 256)
    if channels_last:
        fa, fq = fa.contiguous(memory_format=torch.channels_last), fq.contiguous(memory_format=torch.channels_last)
    key = torch.arange(40, 40 + B, dtype=torch.int64, device=dev)
    rows = ops.round_up(max_corrs, 128)
    kw = dict(corr_rows=rows, round_f16=round_f16)
    und = lambda: torch.zeros((B,), dtype=torch.int32, device=dev)
    res = {}
    if "i8" in routes:
        a8, a_sc, _, a_norm, a_hat = ops.gather_q8(fa, roi_a, na, cap_a, C_pad, want_f32=True, round_f16=round_f16)
        q8, q_sc, q_eps, q_norm, _ = ops.gather_q8(fq, roi_q, nq, cap_q, C_pad, round_f16=round_f16)
        u0, u1 = und(), und()
        old = ops.match_corrs_i8(a_hat, a8, a_sc, fq, roi_a, roi_q, q_norm, q8, q_sc, q_eps, na, nq, thr, W, max_corrs, 1, key, n_undecided=u0, **kw)
        new = ops.match_corrs_i8_araw(fa, a_norm, a8, a_sc, fq, roi_a, roi_q, q_norm, q8, q_sc, q_eps, na, nq, thr, W, max_corrs, 1, key,
                                      n_undecided=u1, **kw)
        _same(old, new, na, "i8")
        assert torch.equal(u0, u1)
        res["i8"] = (new, u1)
    if "mx6" in routes or "x3" in routes:
        a6, a_err, a_norm, a_hat = ops.gather_mx6(fa, roi_a, na, cap_a, C_pad, want_f32=True, round_f16=round_f16)
        a6n, a_errn, a_normn, _ = ops.gather_mx6(fa, roi_a, na, cap_a, C_pad, want_f32=False, round_f16=round_f16)
        live = torch.arange(cap_a, device=dev)[None, :] < na[:, None]
        # the anchor pass without fp32 rows (what the engine launches now) leaves the same operands and norms
        assert torch.equal(a6n[live], a6[live]) and torch.equal(a_normn[live], a_norm[live]) and torch.equal(a_errn, a_err)
    if "mx6" in routes:
        q6, q_err, q_norm, _ = ops.gather_mx6(fq, roi_q, nq, cap_q, C_pad, round_f16=round_f16)
        u0, u1 = und(), und()
        old = ops.match_corrs_mx6(a_hat, a6, a_err, fq, roi_a, roi_q, q_norm, q6, q_err, na, nq, thr, W, max_corrs, 1, key, n_undecided=u0, **kw)
        new = ops.match_corrs_mx6_araw(fa, a_normn, a6n, a_errn, fq, roi_a, roi_q, q_norm, q6, q_err, na, nq, thr, W, max_corrs, 1, key,
                                       n_undecided=u1, **kw)
        _same(old, new, na, "mx6")
        assert torch.equal(u0, u1)
        res["mx6"] = (new, u1)
    if "x3" in routes:
        q6, q_err, q_norm, hilo, lo_max = _gather_mx6_x3(fq, roi_q, nq, cap_q, round_f16)
        u0, u1 = und(), und()
        old = _match_corrs_mx6_x3(a_hat, a6, a_err, fq, roi_a, roi_q, q_norm, q6, q_err, hilo, lo_max, na, nq, thr, W, max_corrs, 1, key, rows, u0,
                                  round_f16)
        new = ops.match_corrs_mx6_x3_araw(fa, a_normn, a6n, a_errn, fq, roi_a, roi_q, q_norm, q6, q_err, hilo, lo_max, na, nq, thr, W, max_corrs, 1,
                                          key, n_undecided=u1, **kw)
        _same(old, new, na, "x3")
        assert torch.equal(u0, u1)
        res["x3"] = (new, u1)
    return res, (roi_a, na, W)


# ------------------------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.gpu
def test_cfg2_size_pairs():
    """8 pairs of the headline shape: 224 x 224, C = 256, 5000 anchors per pair."""
    from oryon_amd.synth import make_pair
    fa, fq, ma, mq = _stack([make_pair(i, 224, 224, 256, device="cuda") for i in range(8)])
    res, _ = _old_vs_new(fa, fq, ma, mq, 256, ("mx6", "i8"), subsample=5000)
    assert res["mx6"][0][3].tolist() == [0] * 8 and res["mx6"][0][2].tolist() == [500] * 8


@pytest.mark.gpu
def test_wide_maps_c512():
    """2 pairs at 384 x 384 with C = 512 (C_pad 512: K0v3 with two lanes per row, the 512-channel screens)."""
    from oryon_amd.synth import make_pair
    fa, fq, ma, mq = _stack([make_pair(20 + i, 384, 384, 512, device="cuda") for i in range(2)])
    res, _ = _old_vs_new(fa, fq, ma, mq, 512, ("mx6", "i8"), subsample=5000)
    assert res["mx6"][0][3].tolist() == [0, 0]


@pytest.mark.gpu
def test_smooth_rank8_batch_takes_the_x3_route():
    """Smooth rank-8 fields: every sampled anchor is ambiguous, the compacted rows feed K1x3 (and the cascade's second pass on the x3 entry)."""
    from oryon_amd.synth import make_pair
    fa, fq, ma, mq = _stack([make_pair(500 + i, 96, 96, 256, device="cuda", smooth=0.02) for i in range(3)])
    res, _ = _old_vs_new(fa, fq, ma, mq, 256, ("x3", "mx6", "i8"))
    for route in ("x3", "mx6"):
        (corrs, n_valid, n_sel, status, md, am, va), und = res[route]
        assert status.tolist() == [0, 0, 0] and int(und.min()) > 100, (route, und.tolist())       # the second level had work on every pair


@pytest.mark.gpu
def test_near_duplicate_query_rows_fill_the_uncertain_and_ambiguous_lists():
    """The pair of _near_duplicate_pair: match_resolve_uncertain_kernel and both compacted lists have work, i.e. every reader of anchor rows
    on the lazy route runs on rows formed from the raw map."""
    from oryon_amd import ops
    dev = "cuda"
    H = 64
    pairs = [_near_duplicate_pair(12, H, H, 256, dev), _near_duplicate_pair(13, H, H, 256, dev)]
    fa, fq, ma, mq = _stack(pairs)
    res, (roi_a, na, W) = _old_vs_new(fa, fq, ma, mq, 256, ("mx6", "i8", "x3"))
    # the exact answer for every anchor, from materialised fp32 rows of both sides
    cap_a, cap_q = ops.round_up(int(na.max()), 256), ops.round_up(H * H, 256)
    roi_q, nq = ops.roi_compact(mq)
    cap_q = ops.round_up(int(nq.max()), 256)
    _, _, _, _, a_hat = ops.gather_q8(fa, roi_a, na, cap_a, 256, want_f32=True)
    _, _, _, _, q_hat = ops.gather_q8(fq, roi_q, nq, cap_q, 256, want_f32=True)
    md0, am0, va0 = ops.match(a_hat, q_hat, na, nq, 0.25)
    for route in ("mx6", "i8"):
        (corrs, n_valid, n_sel, status, md, am, va), und = res[route]
        for b in range(2):
            n = int(na[b])
            assert torch.equal(va[b, :n], va0[b, :n])
            # ambiguous anchors (AMB_VALID + AMB_UNCERTAIN of match_decide_lite_kernel): the lists the compaction kernels read
            n_amb = int(und[b])
            assert n_amb > 0, f"{route}: no ambiguous anchor in pair {b}"
            # rows that hold the exact (distance, argmin) although they were not sampled were resolved BEFORE the sampling: the ambiguous
            # ones with open validity (compacted exact scan) and the unambiguous ones with open validity (match_resolve_uncertain_kernel).
            # More of them than there are ambiguous rows altogether: the latter list is not empty
            sampled = torch.zeros(cap_a, dtype=torch.bool, device=dev)
            pix = corrs[b, : int(n_sel[b]), 0].long() * W + corrs[b, : int(n_sel[b]), 1].long()
            sampled[torch.searchsorted(roi_a[b, :n].long(), pix)] = True
            early = (~sampled[:n]) & (md[b, :n].view(torch.int32) == md0[b, :n].view(torch.int32)) & (am[b, :n] == am0[b, :n]) & (am0[b, :n] != 0)
            assert int(early.sum()) > n_amb, f"{route}: pair {b}: {int(early.sum())} rows resolved before the sampling, {n_amb} ambiguous"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["round_f16", "channels_last", "c96"])
def test_variants(variant):
    """The same three kinds of pair (Gaussian, smooth, near-duplicates) with the raw values rounded to float16 first, with channels-last
    maps, and with C = 96 (rows padded to C_pad 256: the channels beyond C are zeros in K0's rows and in the rows formed on demand)."""
    C = 96 if variant == "c96" else 256
    fa, fq, ma, mq = _stack(_mixed(64, C, "cuda"))
    res, _ = _old_vs_new(fa, fq, ma, mq, 256, ("mx6", "i8", "x3"), channels_last=variant == "channels_last", round_f16=variant == "round_f16")
    assert int(res["mx6"][1][1]) > 100 and int(res["mx6"][1][2]) > 0                  # the smooth and the near-duplicate pair were ambiguous


@pytest.mark.gpu
@pytest.mark.parametrize("C,channels_last,round_f16", [(100, False, False), (100, True, True), (36, True, False)])
def test_entries_vs_c_oracle_at_odd_widths(C, channels_last, round_f16):
    """Widths that are no multiple of 8, where the canonical chain's k + e < C predicate and the channels-last tail are live: every route's
    `_araw` entry (equal to the a_hat entry inside _old_vs_new) against the C oracle's exact scan of the same ROI rows - an independent
    chain, which the old-against-new comparison above is not.  Every anchor row and every sampled row is checked."""
    import numpy as np
    from oracle import c_oracle
    from oryon_amd import ops
    H, n_corrs = 48, 256
    pairs = _mixed(H, C, "cuda")
    fa, fq, ma, mq = _stack(pairs)
    res, (roi_a, na, W) = _old_vs_new(fa, fq, ma, mq, 256, ("mx6", "i8", "x3"), max_corrs=n_corrs, channels_last=channels_last,
                                      round_f16=round_f16)
    roi_q, nq = ops.roi_compact(mq)
    roi_a, roi_q, na, nq = roi_a.cpu().numpy(), roi_q.cpu().numpy(), na.tolist(), nq.tolist()
    # under round_f16 the entries round the raw values to float16 first: the oracle gets the maps rounded to half and back
    as_seen = (lambda x: x.half().float()) if round_f16 else (lambda x: x)
    ref = [c_oracle.match_lin(as_seen(fa[b]).cpu().numpy(), as_seen(fq[b]).cpu().numpy(), roi_a[b, : na[b]], roi_q[b, : nq[b]], 0.25)
           for b in range(len(pairs))]
    for route in ("mx6", "i8", "x3"):
        (corrs, n_valid, n_sel, status, md, am, va), und = res[route]
        corrs, md, am, va = corrs.cpu().numpy().astype(np.int64), md.cpu().numpy(), am.cpu().numpy(), va.cpu().numpy()
        assert n_sel.tolist() == [n_corrs] * len(pairs) and status.tolist() == [0] * len(pairs), (route, n_sel.tolist(), status.tolist())
        for b, (md0, am0, va0) in enumerate(ref):
            n, what = na[b], f"{route}, pair {b}"
            assert np.array_equal(va[b, :n].astype(bool), va0.astype(bool)), f"{what}: valid set differs from the C oracle"
            assert int(n_valid[b]) == int(va0.sum()), what
            lin_a = corrs[b, :n_corrs, 0] * W + corrs[b, :n_corrs, 1]
            row = np.searchsorted(roi_a[b, :n], lin_a)
            assert np.array_equal(roi_a[b, :n][row], lin_a), f"{what}: a sampled anchor pixel is not in the anchor ROI"
            assert np.array_equal(am[b, row], am0[row]), f"{what}: argmin of a sampled row differs from the oracle"
            assert np.array_equal(corrs[b, :n_corrs, 2] * W + corrs[b, :n_corrs, 3], roi_q[b, : nq[b]][am0[row]]), \
                f"{what}: a sampled correspondence's query pixel is not the oracle's argmin"
            # exact, or (rows the bound settled alone carry the screen's estimate) within the screens' bound of the truth: the rule of
            # _check_pair in test_gpu_default_route_vs_oracle.py
            exact = md[b, row].view(np.uint32) == md0[row].view(np.uint32)
            assert np.all(exact | (np.abs(md[b, row] - md0[row]) < 0.05)), f"{what}: min_dist of a sampled row is off"
        if route != "i8":
            assert int(und[1]) > 0, f"{route}: the smooth pair had nothing for the second level"
