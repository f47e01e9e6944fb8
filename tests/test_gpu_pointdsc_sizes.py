"""PointDSC above 512 rows per pair and at the configurations no other test builds, against the float64 restatement
(tests/pdsc_restatement.py) on seeded inputs (tests/pdsc_sizes_cases.py).

The host code of pdsc_solver.hip picks kernels, template instances and LDS sizes by n_cap, S_cap = int(n_cap * ratio) + 1, k and C; the
cases are the smallest sizes that select each of them (DESIGN.md "PointDSC above 512 rows" holds the table).  Every test first asserts,
on the CPU, that its inputs sit away from the decision boundaries the restatement reports (conditions on the inputs, not tolerances), and
takes as its bar the project's own bar or four times the error of the fp32 oracle against float64 on the same inputs, whichever is larger
- never anything read from the kernel's output.  Padding rows are NaN, so a read past n shows."""
import functools

import numpy as np
import pytest
import torch

import pdsc_restatement as rs
import pdsc_sizes_cases as cases
from oracle import oryon_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEFAULT = dict(num_iterations=10, ratio=0.1, sigma_d=0.1, k=40, nms_radius=0.1, inlier_threshold=0.1)
CASE_SEED = {4096: 3}            # generator seed per size where seed 0 misses a condition on the inputs (asserted by every test)
LOOSE = 1e-5                     # a seed whose k-th and (k+1)-th neighbour are closer than this has no decided neighbour list


def case(n, **kw):
    return cases.make_case(n, CASE_SEED.get(n, 0), **kw)


def bar(project, oracle_error):
    """The project's bar, or 4 x the fp32 oracle's own error against float64 (a different but equally valid summation order)."""
    return max(project, 4.0 * float(oracle_error))


@functools.lru_cache(maxsize=None)
def model(C=128, L=1, **kw):
    from oryon_amd.pointdsc import PointDSC
    cfg = dict(DEFAULT, **kw)
    m = PointDSC(in_dim=6, num_layers=L, num_channels=C, **cfg)
    m.load_state_dict(orc.analytic_pointdsc_params(L, C, seed=1), strict=True)
    return m.eval()


def pad(rows, n_cap, dtype=torch.float32):
    """list of [n_i, ...] arrays -> [B, n_cap, ...] on the device, NaN behind every pair's rows."""
    out = torch.full((len(rows), n_cap) + tuple(rows[0].shape[1:]), float("nan"), dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = torch.as_tensor(np.asarray(r), dtype=dtype)
    return out.to(DEV)


def counts(ns):
    return torch.tensor(list(ns), dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------- 1. seeds
@functools.lru_cache(maxsize=None)
def ref_seeds(n, radius=0.1, ratio=0.1):
    c = cases.make_case(n, CASE_SEED.get(n, 0), radius=radius)
    sd = rs.seeds(c["src"], c["conf"], radius, cases.seed_count(n, ratio))
    assert sd["gap"] >= cases.GAP, sd["gap"]                    # condition on the inputs
    return c, sd


def gpu_seeds(m, cs, n_cap, conf=None):
    seeds, n_seeds = m.pick_seeds_batched(pad([c["src"] for c in cs], n_cap), pad(conf or [c["conf"] for c in cs], n_cap),
                                          counts(c["n"] for c in cs))
    return seeds.cpu().numpy().astype(np.int64), n_seeds.cpu().numpy()


@pytest.mark.parametrize("n_cap,n", [(640, 513), (640, 640), (1024, 1024), (2048, 1537), (2048, 2048), (2176, 2049), (2176, 2176), (4096, 4096)])
def test_seeds_equal_the_restatement(n_cap, n):
    """n > 512: second and later passes of both 512-row loops of pdsc_seeds_fused_kernel; n_cap > 2048: pdsc_seed_keys_kernel +
    pdsc_seed_rank_kernel (bitonic, P = 4096)."""
    c, sd = ref_seeds(n)
    assert 0 < sd["local_max"].sum() < n                        # the NMS decides something
    got, n_seeds = gpu_seeds(model(), [c], n_cap)
    S = len(sd["seeds"])
    assert int(n_seeds[0]) == S
    assert np.array_equal(got[0, :S], sd["seeds"]), int(np.argmax(got[0, :S] != sd["seeds"]))


@pytest.mark.parametrize("n_cap", [640, 2176])
def test_seeds_ragged_batch_equals_single_pair_calls(n_cap):
    m = model()
    cs = [ref_seeds(n)[0] for n in (n_cap, 513, 7)]
    got, n_seeds = gpu_seeds(m, cs, n_cap)
    for b, c in enumerate(cs):
        one, n1 = gpu_seeds(m, [c], n_cap)
        S = cases.seed_count(c["n"], 0.1)
        assert int(n_seeds[b]) == int(n1[0]) == S
        assert np.array_equal(got[b, :S], one[0, :S])
        assert np.array_equal(got[b, :S], ref_seeds(c["n"])[1]["seeds"])


@pytest.mark.parametrize("radius,ratio", [(0.0, 0.1), (0.1, 0.25), (0.0, 0.25)])
@pytest.mark.parametrize("n", [513, 640])
def test_seeds_at_radius_zero_and_ratio_quarter(n, radius, ratio):
    """nms_radius = 0: every row is a local maximum (the fused kernel's search for the squared radius starts from 0)."""
    c, sd = ref_seeds(n, radius, ratio)
    if radius == 0.0:
        assert sd["local_max"].all()
    got, n_seeds = gpu_seeds(model(nms_radius=radius, ratio=ratio), [c], 640)
    S = cases.seed_count(n, ratio)
    assert int(n_seeds[0]) == S == len(sd["seeds"])
    assert np.array_equal(got[0, :S], sd["seeds"])


@pytest.mark.parametrize("n_cap", [2048, 2176])
def test_seeds_with_nan_confidences_are_distinct_rows(n_cap):
    """The two routes rank a NaN confidence differently and the reference defines no order: only that the list is a list of rows."""
    c, _ = ref_seeds(n_cap)
    conf = c["conf"].copy()
    conf[[3, 700, n_cap - 1]] = np.nan
    got, n_seeds = gpu_seeds(model(), [c], n_cap, conf=[conf])
    S = cases.seed_count(n_cap, 0.1)
    assert int(n_seeds[0]) == S
    assert len(set(got[0, :S].tolist())) == S and got[0, :S].min() >= 0 and got[0, :S].max() < n_cap


# ---------------------------------------------------------------------------------------------- 2. hypotheses
@functools.lru_cache(maxsize=None)
def ref_hyp(n, C=128, scale=1.0, **kw):
    """(case, restatement seeds, float64 hypotheses, fp32 oracle hypotheses) with the conditions on the inputs asserted."""
    cfg = dict(DEFAULT, **kw)
    c = case(n, C=C, scale=scale)
    sd = rs.seeds(c["src"], c["conf"], cfg["nms_radius"], cases.seed_count(n, cfg["ratio"]))
    hyp = rs.hypotheses(sd["seeds"], c["feat"], c["src"], c["tgt"], 1.0, cfg["sigma_d"], cfg["k"], cfg["num_iterations"], cfg["inlier_threshold"])
    assert all(abs(x) >= 1e-6 for x in hyp["margins"]), hyp["margins"]
    assert (hyp["kgap"] < LOOSE).mean() <= 0.03
    assert hyp["near"].max() <= 2, hyp["near"].max()
    t = {k: torch.from_numpy(c[k]) for k in ("src", "tgt", "feat")}
    o = orc.seed_hypotheses(torch.from_numpy(sd["seeds"]), torch.nn.functional.normalize(t["feat"], p=2, dim=-1), t["src"], t["tgt"], 1.0,
                            cfg["sigma_d"], cfg["k"], cfg["num_iterations"], cfg["inlier_threshold"])
    return c, sd, hyp, dict(T=o["seed_trans"].numpy().astype(np.float64), fitness=o["fitness"].numpy().astype(np.float64))


def check_hypotheses(m, n_cap, n, C=128, scale=1.0, **kw):
    c, sd, hyp, o = ref_hyp(n, C, scale, **kw)
    S, S_cap = len(sd["seeds"]), m.seed_cap(n_cap)
    seeds = torch.zeros((1, S_cap), dtype=torch.int32, device=DEV)
    seeds[0, :S] = torch.from_numpy(sd["seeds"].astype(np.int32)).to(DEV)
    seed_T, fitness, best = m.hypotheses(pad([c["src"]], n_cap), pad([c["tgt"]], n_cap), pad([c["feat"]], n_cap), counts([n]), seeds, counts([S]))
    seed_T, fitness, b = seed_T[0].cpu().numpy().astype(np.float64), fitness[0].cpu().numpy().astype(np.float64), int(best[0])
    assert np.isfinite(seed_T).all() and np.isfinite(fitness).all()            # the slots past n_seeds included
    tight = hyp["kgap"] >= LOOSE
    err = np.abs(seed_T[:S] - hyp["T"]).reshape(S, -1).max(1)
    o_err = np.abs(o["T"] - hyp["T"]).reshape(S, -1).max(1)
    f_err, of_err = np.abs(fitness[:S] - hyp["fitness"]), np.abs(o["fitness"] - hyp["fitness"])
    print(f"hypotheses n_cap={n_cap} n={n} C={C} {kw}: S={S} loose={int((~tight).sum())} near<={int(hyp['near'].max())} "
          f"kernel |dT|={err[tight].max():.2e} (fp32 oracle {o_err[tight].max():.2e}) kernel |dfit|*n={f_err.max() * n:.2f} (oracle {of_err.max() * n:.2f})")
    assert err[tight].max() < bar(1e-5, o_err[tight].max()), int(np.argmax(np.where(tight, err, 0)))
    # a fitness moves only by the rows the restatement itself finds within 1e-5 of the threshold (where the neighbour list is decided)
    assert (f_err[tight] <= hyp["near"][tight] / n + 1e-6).all()
    assert f_err.max() <= bar(2.5 / n, of_err.max())
    assert np.abs(np.linalg.det(seed_T[:S, :3, :3]) - 1).max() < 1e-5
    assert np.array_equal(seed_T[:S, 3], np.tile([0.0, 0, 0, 1], (S, 1)))
    assert b == int(np.argmax(fitness[:S])) and fitness[b] == fitness[:S].max()
    assert hyp["fitness"][b] >= hyp["fitness"].max() - bar(2.5 / n, of_err.max())
    return seed_T[b]


def test_hypotheses_large_lds_launch_after_a_small_first_call():
    """n_cap = 512 first, n_cap = 1024 second, in one process: at 1024 pdsc_seed_dist_mfma_kernel asks for 66 048 bytes of dynamic LDS
    (S_cap = 103 -> 4 seed tiles x 32 x 129 floats), above 64 KB and twice what allow_dynamic_lds recorded for this kernel at the
    512-row call before it.  A refused launch would come back as an error code from the entry (OryonError here), never as a fault.
    Measured on the MI355X: the launch is accepted and computes the restatement's result."""
    check_hypotheses(model(), 512, 500)
    check_hypotheses(model(), 1024, 1024)


@pytest.mark.parametrize("C,n_cap,n", [(128, 640, 640), (128, 640, 513), (128, 1024, 1024), (128, 1152, 1152), (128, 1152, 1025),
                                       (128, 1280, 1280), (128, 2176, 2176), (128, 4096, 4096), (32, 640, 640)])
def test_hypotheses_equal_the_restatement(C, n_cap, n):
    """640 / 1024: pdsc_hyp_fused_kernel<4>; 1152: pdsc_seed_dist_kernel<128> + pdsc_knn_matrix_kernel(dist_pre); 1280 and up:
    pdsc_knn_matrix_kernel with its own distances; 4096: its 4096-entry sort (68 864 bytes of LDS); C = 32: the same kernel, other C."""
    check_hypotheses(model(C=C), n_cap, n, C=C)


# ---------------------------------------------------------------------------------------------- 3. configurations (n_cap = 256, n = 200)
def refine_check(m, cs, n_cap, thr, angle=0.08, shift=0.03):
    """Refinement of every pair of `cs` from a perturbed ground truth, batched; returns the device result [B,4,4] (float64)."""
    # (a pair of a few rows starts closer: all of its rigid rows have to be inside tau, or the fit is rank-deficient)
    T0 = [cases.perturbed(c["T_gt"], c["n"], *((angle, shift) if c["n"] >= 50 else (0.02, 0.005))) for c in cs]
    T = m.refine(pad([c["src"] for c in cs], n_cap), pad([c["tgt"] for c in cs], n_cap), counts(c["n"] for c in cs),
                 torch.from_numpy(np.stack(T0)).to(DEV)).cpu().numpy().astype(np.float64)
    for b, c in enumerate(cs):
        ref = rs.refine(T0[b], c["src"], c["tgt"], thr)
        assert ref["near"] <= 2 and ref["iterations"] >= 1 and ref["min_inliers"] >= 4          # conditions on the inputs
        o = orc.post_refinement(torch.from_numpy(T0[b]), torch.from_numpy(c["src"]), torch.from_numpy(c["tgt"]), thr).numpy()
        err, o_err = np.abs(T[b] - ref["T"]).max(), np.abs(o - ref["T"]).max()
        print(f"refine n_cap={n_cap} n={c['n']} thr={thr}: tau={ref['tau']:.2f} iterations={ref['iterations']} kernel |dT|={err:.2e} (fp32 oracle {o_err:.2e})")
        assert err < bar(2e-5, o_err)
        assert abs(np.linalg.det(T[b, :3, :3]) - 1) < 1e-5
    return T


CONFIGS = {"k8": dict(k=8), "k63": dict(k=63), "k64": dict(k=64), "it1": dict(num_iterations=1), "it16": dict(num_iterations=16),
           "ratio025": dict(ratio=0.25), "ratio1": dict(ratio=1.0), "thr005": dict(inlier_threshold=0.05)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configurations(name):
    """k = 64 alone leaves the fused route, k = 63 fills every lane of its top-64 selection, k strides Mmat / knn; num_iterations indexes
    v_hist / close_hist (16 = the maximum); ratio = 1.0 gives S_cap = 257: the unfused route at a small size; inlier_threshold = 0.05 takes
    tau = 1.2 (on a cloud of side 4, so that residuals on both sides of 1.2 occur)."""
    kw = CONFIGS[name]
    scale = 4.0 if name == "thr005" else 1.0
    m = model(**kw)
    check_hypotheses(m, 256, 200, scale=scale, **kw)
    c = case(200, scale=scale)
    thr = kw.get("inlier_threshold", 0.1)
    if name == "thr005":
        T0 = cases.perturbed(c["T_gt"], 200, 0.08, 0.03 * scale).astype(np.float64)
        d = rs.residuals(T0[None], c["src"].astype(np.float64), c["tgt"].astype(np.float64))[0]
        assert (d > 1.2).sum() > 10 and (d < 1.2).sum() > 10          # tau = 1.2 decides something
    refine_check(m, [c], 256, thr, shift=0.03 * scale)


def test_seventeen_iterations_are_refused_by_create():
    from oryon_amd._lib import OryonError
    m = model(num_iterations=17)
    with pytest.raises(OryonError, match="num_iterations = 17 exceeds the 16 iterates"):
        m.refine(pad([case(200)["src"]], 256), pad([case(200)["tgt"]], 256), counts([200]), torch.eye(4, device=DEV)[None])


# ---------------------------------------------------------------------------------------------- 4. refine
@pytest.mark.parametrize("thr", [0.10, 0.05])
@pytest.mark.parametrize("n_cap", [640, 2176, 4096])
def test_refine_equals_the_restatement(n_cap, thr):
    refine_check(model(inlier_threshold=thr), [case(n_cap)], n_cap, thr)


@pytest.mark.parametrize("thr", [0.10, 0.05])
def test_refine_ragged_batch_equals_single_pair_calls(thr):
    m = model(inlier_threshold=thr)
    cs = [case(640), case(513), case(7)]
    T = refine_check(m, cs, 640, thr)
    for b, c in enumerate(cs):
        assert np.array_equal(T[b], refine_check(m, [c], 640, thr)[0])


def test_register_keeps_identity_for_failed_pairs():
    """status_in != 0 (the pair failed upstream) and a pair too small for a seed: identity pose, status kept / set, neighbours untouched."""
    m = model(L=3)
    cs = [case(640), case(513), case(640), case(7)]
    src, tgt, n = pad([c["src"] for c in cs], 640), pad([c["tgt"] for c in cs], 640), counts(c["n"] for c in cs)
    T, _, st = m.register(src, tgt, n, torch.tensor([0, 2, 1, 0], dtype=torch.int32, device=DEV))
    assert st.cpu().tolist() == [0, 2, 1, 2]
    eye = torch.eye(4, device=DEV)
    assert all(torch.equal(T[b], eye) for b in (1, 2, 3))
    T1, _, st1 = m.register(src[:1].contiguous(), tgt[:1].contiguous(), n[:1].contiguous())
    assert int(st1[0]) == 0 and torch.equal(T1[0], T[0])


# ---------------------------------------------------------------------------------------------- 5. encoder and register (L = 3, C = 128)
@functools.lru_cache(maxsize=None)
def ref_encoder(n):
    c = case(n)
    P = orc.analytic_pointdsc_params(3, 128, seed=1)
    feat, conf = rs.encoder(c["src"], c["tgt"], P, 3)
    s, t = torch.from_numpy(c["src"]), torch.from_numpy(c["tgt"])
    cp = torch.cat([s, t], dim=-1)
    o_feat = orc.encoder_forward(cp - cp.mean(0), orc.sc_matrix(s, t, 0.1)[0], P, 3)
    return c, feat, conf, o_feat.numpy(), orc.confidence_head(o_feat, P).numpy()


def check_encoder(feat_gpu, conf_gpu, n):
    _, feat, conf, o_feat, o_conf = ref_encoder(n)
    fs, cs_ = np.abs(feat).max(), max(1.0, np.abs(conf).max())
    f_err, c_err = np.abs(feat_gpu[:n].cpu().numpy() - feat).max(), np.abs(conf_gpu[:n].cpu().numpy() - conf).max()
    of_err, oc_err = np.abs(o_feat - feat).max(), np.abs(o_conf - conf).max()
    print(f"encoder n={n}: kernel |dfeat|/scale={f_err / fs:.2e} (fp32 oracle {of_err / fs:.2e}) kernel |dconf|={c_err:.2e} (oracle {oc_err:.2e})")
    assert f_err < bar(1e-4 * fs, of_err)
    assert c_err < bar(1e-4 * cs_, oc_err)


@pytest.mark.parametrize("n_cap,n", [(640, 513), (640, 640), (1024, 1024)])
def test_encoder_single_pair_above_512_rows(n_cap, n):
    """B = 1: the key-split fused route (four key splits of pdsc_attention_x3_kernel, more key tiles per workgroup than any other test)."""
    c = case(n)
    feat, conf = model(L=3).encode(pad([c["src"]], n_cap), pad([c["tgt"]], n_cap), counts([n]))
    check_encoder(feat[0], conf[0], n)


def test_encoder_chain_route_at_1024_rows():
    """B = 32 at n_cap = 1024: 256 query blocks, no key split, n_cap % 256 == 0 -> pdsc_att_chain_x3_kernel with 16 key tiles per pair.
    Ragged n from 11 to 1024; three pairs against float64; copies of one pair at batch positions 0, 9 and 31 bit-equal."""
    rng = np.random.default_rng(5)
    ns = [int(x) for x in rng.integers(11, 1025, 32)]
    ns[0], ns[1], ns[2], ns[9], ns[31] = 1024, 513, 11, 1024, 1024
    src, tgt = [], []
    for b, k in enumerate(ns):
        if k in (1024, 513, 11) and b in (0, 1, 2, 9, 31):
            src.append(case(k)["src"]), tgt.append(case(k)["tgt"])
        else:
            s = rng.random((k, 3)).astype(np.float32)
            src.append(s), tgt.append((s + 0.02 * rng.normal(size=(k, 3))).astype(np.float32))
    feat, conf = model(L=3).encode(pad(src, 1024), pad(tgt, 1024), counts(ns))
    for b in (0, 1, 2):
        check_encoder(feat[b], conf[b], ns[b])
    for b in (9, 31):
        assert torch.equal(feat[0], feat[b]) and torch.equal(conf[0], conf[b])
    for b, k in enumerate(ns):
        assert torch.isfinite(feat[b, :k]).all() and torch.isfinite(conf[b, :k]).all()


@functools.lru_cache(maxsize=None)
def ref_register(n):
    c = case(n)
    P = orc.analytic_pointdsc_params(3, 128, seed=1)
    cfg = dict(DEFAULT, num_layers=3)
    r = rs.register(c["src"], c["tgt"], P, cfg)
    o = orc.pointdsc_forward(torch.from_numpy(c["src"]), torch.from_numpy(c["tgt"]), P, cfg).numpy()
    return c, r, o


@pytest.mark.parametrize("n_cap,n", [(640, 513), (1024, 1024), (1152, 1025), (2176, 2176)])
def test_register_equals_the_restatement_pipeline(n_cap, n):
    c, r, o = ref_register(n)
    T, _, st = model(L=3).register(pad([c["src"]], n_cap), pad([c["tgt"]], n_cap), counts([n]))
    T = T[0].cpu().numpy().astype(np.float64)
    err, o_err = np.abs(T - r["T"]).max(), np.abs(o - r["T"]).max()
    print(f"register n_cap={n_cap} n={n}: kernel |dT|={err:.2e} (fp32 oracle {o_err:.2e}), vs the generating pose {np.abs(T - c['T_gt']).max():.2e}")
    assert int(st[0]) == 0
    assert err < bar(1e-4, o_err)
    assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-5
