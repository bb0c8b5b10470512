"""The evaluator's tables without a GPU: the rule of tests/hpe_ref.py against the imported reference's
golden (tests/golden/make_golden_hpe.py), the properties the rule states, and the surfaces -- the C entry's declaration, binding
and refusals, the Python layer's ValueErrors that need no device tensor, the opt-in switch of A2JModelLightning.  The kernel
against the rule, bit for bit, and the ValueErrors of ops.hpe_accumulate (they need device tensors): tests/test_hpe_gpu.py."""
import ctypes as C
import inspect
import math
import re
import subprocess

import numpy as np
import pytest

import hpe_cases
import hpe_ref as H

# The rule's largest deviation from the reference's align_w_scale on the fixture, measured here with scipy 1.15.3 / numpy 2.2.6
# (LAPACK's gesdd against the ten Jacobi sweeps, both in fp64): 2.28e-13 mm on the aligned coordinates (values up to ~1000 mm:
# about one ulp) and 1.84e-13 mm on the pa distances.  Four times the measured value is asserted; the margin covers another
# LAPACK build's last bits.
PA_ALIGNED_MEASURED, PA_DIST_MEASURED = 2.28e-13, 1.84e-13
GUARD = max(1e-6, 1000.0 * PA_ALIGNED_MEASURED)            # mm: no reference pa distance may lie this close to a threshold
MPJPE_BOUND = 2.0 ** -21 + 1e-9                            # mm: half the fixed-point quantum (derived) + the host's fp64 means


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "hpe_metrics.npz")


@pytest.fixture(scope="module")
def ruled(golden):
    """the rule on the golden's inputs, once"""
    return H.accumulate(golden["pred"], golden["gt"], golden["thresholds"])


def _bytes(state):
    return b"".join(np.ascontiguousarray(state[k]).tobytes() for k in ("hist", "sum", "n"))


def test_the_golden_meets_its_conditions(golden):
    assert golden["sv_ratio"].min() > 1e-3 and golden["reflected"].sum() >= 3
    gap = np.abs(golden["dist"][:, 2, :, None] - golden["thresholds"][None, None, :]).min()
    assert gap > GUARD and float(golden["guard"]) >= GUARD, (gap, GUARD)
    assert np.array_equal(golden["thresholds"], np.linspace(0, 50, 100))
    for name in ("ab", "rr", "pa"):                        # a curve that is neither all 0 nor all 1
        assert 0.0 < golden["pck_" + name][10] < golden["pck_" + name][-1] <= 1.0


def test_the_rule_against_the_reference(golden, ruled):
    """ab and rr distances and every PCK count: equal to the reference's, bit for bit (numpy sums three squares in the order
    the rule writes).  pa: within four times the deviation measured on this fixture -- aligned 2.28e-13 mm, distances 1.84e-13 mm
    -- and, as no distance lies within GUARD of a threshold, every PCK count equal too.  MPJPE within 2^-21 mm + 1e-9 mm (measured:
    8.2e-10, 2.8e-9, 1.1e-8 mm), AUC within 1e-12 (measured: 0)."""
    state, dist, aligned = ruled
    assert np.array_equal(dist[:, 0], golden["dist"][:, 0]) and np.array_equal(dist[:, 1], golden["dist"][:, 1])
    dev_al, dev_d = np.abs(aligned - golden["aligned"]).max(), np.abs(dist[:, 2] - golden["dist"][:, 2]).max()
    print(f"pa: aligned deviates by {dev_al:.3e} mm, distances by {dev_d:.3e} mm")
    assert dev_al <= 4 * PA_ALIGNED_MEASURED and dev_d <= 4 * PA_DIST_MEASURED, (dev_al, dev_d)
    res = H.compute(state, golden["thresholds"])
    assert res["fed"] == golden["pred"].shape[0] and res["skipped"] == 0
    for a, name in enumerate(("ab", "rr", "pa")):
        counts = np.cumsum(state["hist"][a], axis=1)[:, :-1]
        assert np.array_equal(counts, golden["count_" + name]), name
        key = H.NAMES[a]
        print(name, "mpjpe off by", res[key]["mpjpe"] - float(golden["mean_" + name]), "auc off by", res[key]["auc"] - float(golden["auc_" + name]))
        assert abs(res[key]["mpjpe"] - float(golden["mean_" + name])) <= MPJPE_BOUND
        assert abs(res[key]["auc"] - float(golden["auc_" + name])) <= 1e-12
        assert np.abs(res["pck"][a] - golden["pck_" + name]).max() <= 1e-12
    assert np.array_equal(res["thresholds"], golden["thresholds"]) and res["pck"].shape == (3, 100)


def test_the_packages_compute_is_the_rules(ruled, golden):
    from hn_amd import metrics
    state = ruled[0]
    want, got = H.compute(state, golden["thresholds"]), metrics.compute(state, golden["thresholds"])
    assert metrics.NAMES == H.NAMES and metrics.Q20 == H.Q20
    for name in H.NAMES:
        assert got[name] == want[name]
    assert np.array_equal(got["pck"], want["pck"]) and (got["fed"], got["skipped"]) == (want["fed"], want["skipped"])


def test_the_thresholds_are_inclusive():
    """EvalUtil counts data <= threshold: a distance of 0 counts at threshold 0, one of exactly 50.0 at the last threshold, one
    of sqrt(2500.25) at none.  Checked on the ab and rr tables (the pa distance of these samples is not an exact number)."""
    thr = np.linspace(0.0, 50.0, 100)
    gt = np.round(np.random.RandomState(3).uniform(-200, 200, (3, 21, 3))).astype(np.float32)
    gt[:, :, 2] += 600
    pred = gt.copy()
    pred[1] -= np.array([30.0, 40.0, 0.0], np.float32)
    pred[2] -= np.array([30.0, 40.0, 0.5], np.float32)
    for i, (first, last) in enumerate(((1, 1), (0, 1), (0, 0))):
        state, dist, _ = H.accumulate(pred[i:i + 1], gt[i:i + 1], thr)
        res = H.compute(state, thr)
        assert np.all(dist[0, 0] == (0.0, 50.0, math.sqrt(2500.25))[i])
        assert np.all(dist[0, 1] == 0.0)                                    # every joint moved alike: root-relative error 0
        assert res["pck"][0, 0] == first and res["pck"][0, -1] == last and res["pck"][1, 0] == 1.0
        assert state["hist"][0, :, (0, 99, 100)[i]].sum() == 21
    both = H.accumulate(pred, gt, thr)[0]
    assert np.all(np.cumsum(both["hist"][0], axis=1)[:, 99] == 2) and abs(H.compute(both, thr)["pck"][0, -1] - 2.0 / 3.0) < 1e-15


def test_any_split_and_any_order_give_the_same_bytes():
    thr = hpe_cases.thresholds(100)
    pred, gt, valid, kinds = hpe_cases.batch(40, 21, seed=5)
    assert set(kinds) == set(hpe_cases.KINDS)
    whole, _, _ = H.accumulate(pred, gt, thr, valid=valid)
    rng = np.random.RandomState(6)
    for cuts in ((1,), (7, 20), (13,), tuple(range(1, 40))):
        perm = rng.permutation(40)
        state = None
        for part in np.split(perm, cuts):
            state, _, _ = H.accumulate(pred[part], gt[part], thr, state=state, valid=valid[part])
        assert _bytes(state) == _bytes(whole), cuts
    # merge == one pass; the inputs of a merge are not changed
    a, _, _ = H.accumulate(pred[:11], gt[:11], thr, valid=valid[:11])
    b, _, _ = H.accumulate(pred[11:], gt[11:], thr, valid=valid[11:])
    before = _bytes(a)
    assert _bytes(H.merge(a, b)) == _bytes(whole) and _bytes(a) == before
    assert whole["n"].tolist() == [40 - sum(k in hpe_cases.SKIPPED for k in kinds), sum(k in hpe_cases.SKIPPED for k in kinds)]
    assert np.all(whole["hist"].sum(axis=2) == whole["n"][0])               # every fed sample is in exactly one bin per joint


def test_skipped_samples_are_counted_and_add_nothing():
    thr = hpe_cases.thresholds(100)
    pred, gt, valid, kinds = hpe_cases.batch(24, 21, seed=7)
    keep = np.array([k not in hpe_cases.SKIPPED for k in kinds])
    state, dist, aligned = H.accumulate(pred, gt, thr, valid=valid)
    kept, _, _ = H.accumulate(pred[keep], gt[keep], thr)
    assert state["n"].tolist() == [int(keep.sum()), int((~keep).sum())] and kept["n"].tolist() == [int(keep.sum()), 0]
    assert np.array_equal(state["hist"], kept["hist"]) and np.array_equal(state["sum"], kept["sum"])
    assert np.isnan(dist[~keep]).all() and np.isnan(aligned[~keep]).all()
    assert np.isfinite(dist[keep]).all() and np.isfinite(aligned[keep]).all()
    # the limit itself: 2^20 is skipped, the fp32 just below it is fed
    below = np.nextafter(np.float32(2.0 ** 20), np.float32(0))
    for value, fed in ((np.float32(2.0 ** 20), 0), (np.float32(-2.0 ** 20), 0), (below, 1), (-below, 1)):
        p = pred[:1].copy()
        p[0, 4, 1] = value
        assert H.accumulate(p, gt[:1], thr)[0]["n"].tolist() == [fed, 1 - fed], value


def test_nothing_fed_gives_nan_not_an_exception():
    thr = hpe_cases.thresholds(100)
    for state in (H.new_state(21, 100), H.accumulate(np.zeros((2, 21, 3), np.float32), np.zeros((2, 21, 3), np.float32), thr,
                                                     valid=np.zeros((2,), np.int32))[0]):
        res = H.compute(state, thr)
        assert res["fed"] == 0 and res["pck"].shape == (3, 100) and np.isnan(res["pck"]).all()
        assert all(math.isnan(res[name][key]) for name in H.NAMES for key in ("mpjpe", "auc"))
    empty, dist, aligned = H.accumulate(np.zeros((0, 21, 3), np.float32), np.zeros((0, 21, 3), np.float32), thr)
    assert empty["n"].tolist() == [0, 0] and dist.shape == (0, 3, 21) and aligned.shape == (0, 21, 3)


@pytest.mark.parametrize("j", [1, 2, 3, 21, 64])
def test_rank_deficient_sets_give_finite_output(j):
    """all prediction joints equal, collinear sets, coplanar ground truth, J = 1 (and 2, 3): the completion rule keeps R finite
    and orthogonal, so `aligned` and the distances are finite; where M vanishes the aligned set is the ground truth's centre"""
    thr = hpe_cases.thresholds(100)
    pred, gt, valid, kinds = hpe_cases.batch(12, j, seed=11 + j)
    state, dist, aligned = H.accumulate(pred, gt, thr, valid=valid)
    keep = np.array([k not in hpe_cases.SKIPPED for k in kinds])
    assert np.isfinite(aligned[keep]).all() and np.isfinite(dist[keep]).all()
    assert np.abs(aligned[keep]).max() < 2000.0                             # near the hands, not merely finite
    for i in np.nonzero(keep)[0]:
        m, _a, _b, _s1, t1 = H.procrustes_matrix(gt[i].astype(np.float64), pred[i].astype(np.float64))
        r, s, sigma = H.rotation(m)
        r = np.array(r)
        assert np.abs(r @ r.T - np.eye(3)).max() < 1e-12, (kinds[i], sigma)
        if kinds[i] == "equal" or j == 1:
            assert np.abs(aligned[i] - np.array(t1)).max() < 1e-3, kinds[i]
    # the three completions, each reached: 2 live columns, 1 live column, none
    for m, live in (([[2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], 2), ([[0.0, 0.0, 0.0], [0.0, 0.0, 3.0], [0.0, 0.0, 0.0]], 1),
                    ([[0.0] * 3] * 3, 0), ([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [-1.0, -2.0, -3.0]], 1)):
        r, s, sigma = H.rotation(m)
        assert sum(x > 0 and x > H.LIVE * max(sigma) for x in sigma) == live
        r = np.array(r)
        assert np.isfinite(r).all() and np.abs(r @ r.T - np.eye(3)).max() < 1e-12
        assert abs(s - np.linalg.svd(np.array(m), compute_uv=False).sum()) < 1e-12


def test_the_sweep_count_has_margin():
    """hpe_ref.SWEEPS = 10 against the convergence measured here (2000 matrices of the five families of the docstring's 20000):
    after 5 sweeps no column pair is further from orthogonal than 1e-15 and R moves by less than 1e-14 until sweep 10; R and s
    agree with LAPACK's to 1e-13 on the well-conditioned family."""
    rng = np.random.RandomState(1)
    worst_off = worst_move = worst_lapack = 0.0
    for i in range(2000):
        u, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        v, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        kind = i % 5
        if kind == 0:
            sv = rng.uniform(0.1, 1, 3)
        elif kind == 1:
            sv = np.array([1, 10 ** -rng.uniform(0, 6), 10 ** -rng.uniform(0, 12)])
        elif kind == 2:
            sv = np.array([1, 1, 1]) + rng.normal(size=3) * 1e-9
        elif kind == 3:
            sv = np.array([1, 1 - 1e-14 * rng.randint(0, 50), 10 ** -rng.uniform(0, 3)])
        else:
            sv = rng.uniform(0, 1, 3) ** 8
        m = ((u * sv) @ v.T * 10 ** rng.uniform(-3, 0)).tolist()
        g, _ = H.jacobi(m, 5)
        for p, q in H.PAIRS:
            alpha, beta = sum(g[r][p] ** 2 for r in range(3)), sum(g[r][q] ** 2 for r in range(3))
            gamma = sum(g[r][p] * g[r][q] for r in range(3))
            if alpha > 0 and beta > 0:
                worst_off = max(worst_off, abs(gamma) / math.sqrt(alpha * beta))
        r5, r10 = np.array(H.rotation(m, 5)[0]), np.array(H.rotation(m, H.SWEEPS)[0])
        worst_move = max(worst_move, np.abs(r5 - r10).max())
        if kind == 0:
            uu, ss, vt = np.linalg.svd(np.array(m))
            r, s, _ = H.rotation(m)
            worst_lapack = max(worst_lapack, np.abs(np.array(r) - uu @ vt).max(), abs(s - ss.sum()) / ss.sum())
    print(f"after 5 sweeps: off-orthogonality {worst_off:.2e}, R moves {worst_move:.2e} until sweep {H.SWEEPS}; LAPACK {worst_lapack:.2e}")
    assert H.SWEEPS == 10 and worst_off < 1e-15 and worst_move < 1e-14 and worst_lapack < 1e-13


# --------------------------------------------------------------------------------------------------------------- the surfaces
def test_the_entry_is_declared_exported_and_bound():
    from hn_amd import _lib, build, ops
    build.build_library()
    text = re.sub(r"/\*.*?\*/", "", (build.REPO_ROOT / "include" / "handnet_hip.h").read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.lib_path())], capture_output=True, text=True, check=True).stdout
    name = "hn_hpe_accumulate_f32"
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert proto and name in _lib.SIGNATURES
    params = [p.strip() for p in proto.group(1).split(",")]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and len(params) == len(args) == 13
    for p, a in zip(params, args):
        assert (a is C.c_void_p) if "*" in p else (p.startswith("int ") and a is C.c_int), p
    assert re.search(r" T %s\b" % name, out)
    lib = _lib.load()
    assert lib.hn_abi_version() == 36 == _lib.ABI_VERSION                  # a function added, no struct touched
    assert build.EXTRA_FLAGS["hpe_metrics.hip"][0] == "-ffp-contract=off"
    rows = (build.CSRC / "build" / "hpe_metrics.resources.txt").read_text().splitlines()
    assert len(rows) == 1 and "hpe_accumulate_kernel" in rows[0]           # one launch does everything
    assert " vgpr_spill 0 " in rows[0] and rows[0].endswith("sgpr_spill 0") and " scratch 0 " in rows[0]
    assert ops.HPE_WAVES_PER_GROUP == hpe_cases.WAVES
    assert "constexpr int kWaves = %d;" % hpe_cases.WAVES in (build.CSRC / "hpe_metrics.hip").read_text()
    assert "constexpr int kSweeps = %d;" % H.SWEEPS in (build.CSRC / "hpe_metrics.hip").read_text()


def test_the_entry_checks_its_arguments_before_any_launch():
    """no GPU here: every refusal comes back as HN_ERR_ARG with a message under the entry's name, before the device is touched;
    an empty batch is a successful no-op (with or without the sample pointers)"""
    from hn_amd import _lib
    lib = _lib.load()
    P = 4096        # stands for a device address

    def call(s=8, j=21, t=100, **ptrs):
        p = dict(pred=P, gt=P, valid=P, thr=P, hist=P, sum=P, n=P, dist=P, aligned=P)
        p.update(ptrs)
        return lib.hn_hpe_accumulate_f32(p["pred"], p["gt"], p["valid"], s, j, p["thr"], t, p["hist"], p["sum"], p["n"], p["dist"],
                                         p["aligned"], None)
    refusals = [(dict([(name, None)]), b"null pointer") for name in ("pred", "gt", "thr", "hist", "sum", "n")]
    refusals += [(dict(s=-1), b"s = -1"), (dict(j=0), b"j = 0"), (dict(j=65), b"j = 65"), (dict(j=-3), b"j = -3"),
                 (dict(t=0), b"t = 0"), (dict(t=1025), b"t = 1025"), (dict(t=-1), b"t = -1"),
                 (dict(thr=P + 4), b"aligned to 8"), (dict(hist=P + 4), b"aligned to 8"), (dict(sum=P + 2), b"aligned to 8"),
                 (dict(n=P + 1), b"aligned to 8"), (dict(dist=P + 4), b"aligned to 8"), (dict(aligned=P + 4), b"aligned to 8"),
                 (dict(pred=P + 2), b"aligned to 4"), (dict(gt=P + 1), b"aligned to 4"), (dict(valid=P + 3), b"aligned to 4"),
                 (dict(s=0, j=0), b"j = 0"), (dict(s=0, hist=None), b"null pointer")]
    for kw, word in refusals:
        assert call(**kw) == 1, kw
        err = lib.hn_last_error()
        assert err.startswith(b"hn_hpe_accumulate_f32: ") and word in err, (kw, err)
    assert call(s=0) == 0 and call(s=0, pred=None, gt=None, valid=None, dist=None, aligned=None) == 0


def test_the_python_layer_refuses_without_a_device():
    import torch
    from hn_amd import metrics, ops
    for joints, steps in ((0, 100), (65, 100), (21, 0), (21, 1025)):
        with pytest.raises(ValueError, match="joints 1..64"):
            ops.hpe_state(joints, steps, "cpu")
    st = ops.hpe_state(21, 100, "cpu")
    assert st.hist.shape == (3, 21, 101) and st.sum.shape == (3, 21) and st.n.shape == (2,) and st.flat.dtype == torch.int64
    assert st.flat.numel() == 3 * 21 * 101 + 3 * 21 + 2 and st.hist.data_ptr() == st.flat.data_ptr() and not st.flat.any()
    with pytest.raises(ValueError, match="accumulates on a GPU"):
        metrics.HPEMetrics("cpu")
    for lo, hi in ((1.0, 0.0), (0.0, float("inf")), (float("nan"), 50.0)):
        with pytest.raises(ValueError, match="finite and non-decreasing"):
            metrics.HPEMetrics("cuda:0", val_min=lo, val_max=hi)
    with pytest.raises(RuntimeError, match="must live on the GPU"):         # no CPU fall-back
        ops.hpe_accumulate(torch.zeros(1, 21, 3), torch.zeros(1, 21, 3), torch.zeros(100, dtype=torch.float64))


def test_device_metrics_is_opt_in():
    from a2j.a2j import A2JModelLightning
    names = list(inspect.signature(A2JModelLightning.__init__).parameters)
    assert names == ["self", "num_classes", "crop_height", "crop_width", "is_3D", "is_RGBD", "spatial_factor", "display_freq", "output_dir"]
    assert "enable" in inspect.signature(A2JModelLightning.device_metrics).parameters
    net = A2JModelLightning()
    assert net._hpe_metrics is None and net.hpe_results is None            # off as constructed
    with pytest.raises(ImportError, match="dex_ycb_toolkit"):
        net.test_epoch_end([])
    assert net.device_metrics() is net and net._hpe_metrics is False        # on; the accumulator is built with the first batch
    assert net.device_metrics(False)._hpe_metrics is None
    with pytest.raises(ImportError, match="dex_ycb_toolkit"):
        net.test_epoch_end([])
