"""The evaluator's tables on the device (csrc/hpe_metrics.hip) against the rule of tests/hpe_ref.py, bit for
bit: the state (hist, sum, n) and the two optional fp64 outputs, through ops.hpe_accumulate and through the C entry, at every
shape of hpe_cases.SHAPES; the golden's reference numbers through HPEMetrics.compute(); the evaluation loop end to end with
A2JModelLightning.device_metrics(True)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import hpe_cases
import hpe_ref as H
from test_hpe_cpu import MPJPE_BOUND, PA_ALIGNED_MEASURED, PA_DIST_MEASURED

pytestmark = pytest.mark.gpu

_RULED = {}


def _case(shape):
    """the batch of a shape and the rule on it, computed once and shared"""
    if shape not in _RULED:
        s, j, t = shape
        pred, gt, valid, kinds = hpe_cases.batch(s, j, seed=100 + s + j)
        thr = hpe_cases.thresholds(t)
        _RULED[shape] = (pred, gt, valid, thr, kinds) + H.accumulate(pred, gt, thr, valid=valid)
    return _RULED[shape]


def _bits(x):
    """fp64 as its bytes: NaN rows compare too"""
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _same_state(state, want):
    return all(np.array_equal(getattr(state, k).cpu().numpy(), want[k]) for k in ("hist", "sum", "n"))


@pytest.mark.parametrize("shape", hpe_cases.SHAPES, ids=lambda s: "S%d-J%d-T%d" % s)
def test_the_kernel_equals_the_rule_bit_for_bit(shape):
    from hn_amd import _lib, ops
    pred, gt, valid, thr, kinds, want, want_dist, want_aligned = _case(shape)
    s, j, t = shape
    if s >= len(hpe_cases.KINDS):
        assert set(kinds) == set(hpe_cases.KINDS)                          # reflected, skipped and rank-deficient rows are in
    d_pred, d_gt, d_valid, d_thr = (torch.from_numpy(x).cuda() for x in (pred, gt, valid, thr))
    lib = _lib.load()
    for _ in range(2):                                                      # twice: the same bytes
        got = ops.hpe_accumulate(d_pred, d_gt, d_thr, valid=d_valid, want_dist=True, want_aligned=True)
        assert _same_state(got.state, want)
        assert tuple(got.dist.shape) == (s, 3, j) and tuple(got.aligned.shape) == (s, j, 3)
        assert np.array_equal(_bits(got.dist.cpu().numpy()), _bits(want_dist))
        assert np.array_equal(_bits(got.aligned.cpu().numpy()), _bits(want_aligned))
        # the C entry, into 0xFF-filled optional outputs: every row is written
        state = ops.hpe_state(j, t, "cuda")
        dist = torch.full((s, 3, j), -1, dtype=torch.int64, device="cuda").view(torch.float64)
        aligned = torch.full((s, j, 3), -1, dtype=torch.int64, device="cuda").view(torch.float64)
        status = lib.hn_hpe_accumulate_f32(d_pred.data_ptr(), d_gt.data_ptr(), d_valid.data_ptr(), s, j, d_thr.data_ptr(), t,
                                           state.hist.data_ptr(), state.sum.data_ptr(), state.n.data_ptr(), dist.data_ptr(),
                                           aligned.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert status == 0, lib.hn_last_error()
        assert _same_state(state, want)
        assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want_dist))
        assert np.array_equal(_bits(aligned.cpu().numpy()), _bits(want_aligned))
    # without the optional outputs and without `valid`: the state of the rule without `valid`
    plain = ops.hpe_accumulate(d_pred, d_gt, d_thr)
    assert plain.dist is None and plain.aligned is None
    assert _same_state(plain.state, H.accumulate(pred, gt, thr)[0])


def test_two_batches_into_one_state_equal_one_batch_of_both():
    from hn_amd import ops
    pred, gt, valid, thr, _kinds, want, _d, _a = _case((257, 21, 100))
    d_pred, d_gt, d_valid, d_thr = (torch.from_numpy(x).cuda() for x in (pred, gt, valid, thr))
    state = None
    for lo, hi in ((0, 100), (100, 257)):
        state = ops.hpe_accumulate(d_pred[lo:hi], d_gt[lo:hi], d_thr, state=state, valid=d_valid[lo:hi]).state
    assert _same_state(state, want)
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(3)).cuda()
    again = ops.hpe_accumulate(d_pred[perm].contiguous(), d_gt[perm].contiguous(), d_thr, valid=d_valid[perm].contiguous()).state
    assert torch.equal(again.flat, state.flat)


def test_the_goldens_reference_numbers_through_hpemetrics(golden_dir):
    """HPEMetrics on the golden's inputs in batches of 16 against the imported reference's get_measures(0, 50, 100): the bounds
    of tests/test_hpe_cpu.py (MPJPE 2^-21 + 1e-9 mm, AUC and PCK 1e-12, every PCK count equal), ops.procrustes_align within four
    times the rule's measured deviation from the reference's align_w_scale; merge of two shards == one pass; reset."""
    from hn_amd import ops
    from hn_amd.metrics import HPEMetrics
    g = np.load(golden_dir / "hpe_metrics.npz")
    pred, gt = torch.from_numpy(g["pred"]).cuda(), torch.from_numpy(g["gt"]).cuda()
    m = HPEMetrics("cuda:0")
    assert np.array_equal(m.thresholds, g["thresholds"])
    for lo in range(0, pred.shape[0], 16):
        m.update(pred[lo:lo + 16], gt[lo:lo + 16])
    res = m.compute()
    state = m.state()
    assert res["fed"] == pred.shape[0] and res["skipped"] == 0
    for a, name in enumerate(("ab", "rr", "pa")):
        key = H.NAMES[a]
        assert np.array_equal(np.cumsum(state["hist"][a], axis=1)[:, :-1], g["count_" + name]), name
        assert abs(res[key]["mpjpe"] - float(g["mean_" + name])) <= MPJPE_BOUND and abs(res[key]["auc"] - float(g["auc_" + name])) <= 1e-12
        assert np.abs(res["pck"][a] - g["pck_" + name]).max() <= 1e-12
    aligned = ops.procrustes_align(gt, pred).cpu().numpy()
    assert np.abs(aligned - g["aligned"]).max() <= 4 * PA_ALIGNED_MEASURED
    got = ops.hpe_accumulate(pred, gt, torch.from_numpy(g["thresholds"]).cuda(), want_dist=True)
    assert np.array_equal(got.dist.cpu().numpy()[:, :2], g["dist"][:, :2])                       # ab and rr: the reference's bits
    assert np.abs(got.dist.cpu().numpy()[:, 2] - g["dist"][:, 2]).max() <= 4 * PA_DIST_MEASURED
    # two shards, merged: the same bytes as one pass; a state of another shape is refused; reset
    a, b = HPEMetrics("cuda:0"), HPEMetrics("cuda:0")
    a.update(pred[:20], gt[:20])
    b.update(pred[20:], gt[20:])
    a.merge(b)
    assert all(np.array_equal(a.state()[k], state[k]) for k in state)
    b.merge(a.state())
    assert b.state()["n"].tolist() == [pred.shape[0] + pred.shape[0] - 20, 0]
    with pytest.raises(ValueError, match="does not fit"):
        a.merge(HPEMetrics("cuda:0", steps=50))
    a.reset()
    assert not a.state()["hist"].any() and a.state()["n"].tolist() == [0, 0] and math.isnan(a.compute()["procrustes"]["auc"])


def test_the_op_checks_its_tensors():
    from hn_amd import ops
    pred, gt = torch.zeros((4, 21, 3), device="cuda"), torch.zeros((4, 21, 3), device="cuda")
    thr = torch.linspace(0, 50, 100, dtype=torch.float64, device="cuda")
    ok = ops.hpe_accumulate(pred, gt, thr)
    assert ok.state.n.tolist() == [4, 0]
    bad = [(dict(pred=pred[:, :, :2].contiguous()), "one shape"), (dict(pred=pred.reshape(4, 63)), "one shape"),
           (dict(gt=gt[:3].contiguous()), "one shape"), (dict(pred=torch.zeros((4, 65, 3), device="cuda"), gt=torch.zeros((4, 65, 3), device="cuda")), "65 joints"),
           (dict(pred=torch.zeros((4, 0, 3), device="cuda"), gt=torch.zeros((4, 0, 3), device="cuda")), "0 joints"),
           (dict(thr=thr.reshape(10, 10)), r"fp64 \[T\]"), (dict(thr=thr[:0]), r"fp64 \[T\]"),
           (dict(thr=torch.zeros(1025, dtype=torch.float64, device="cuda")), r"fp64 \[T\]"),
           (dict(valid=torch.ones(3, dtype=torch.int32, device="cuda")), "one value per sample"),
           (dict(state=ops.hpe_state(21, 50, "cuda")), "state.hist"), (dict(state=ops.hpe_state(20, 100, "cuda")), "state.hist"),
           (dict(pred=pred.transpose(0, 1).contiguous().transpose(0, 1)), "contiguous"), (dict(thr=thr[::2]), "contiguous")]
    for kw, word in bad:
        args = dict(pred=pred, gt=gt, thr=thr, state=None, valid=None)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            ops.hpe_accumulate(args["pred"], args["gt"], args["thr"], state=args["state"], valid=args["valid"])
    with pytest.raises(TypeError):
        ops.hpe_accumulate(pred, gt, thr.float())
    with pytest.raises(TypeError):
        ops.hpe_accumulate(pred.double(), gt, thr)
    assert ok.state.n.tolist() == [4, 0]                                    # no refused call touched a state


def _eval_batch(k, seed):
    """What datasets3d/a2jdataset.py:293 hands the loop: (depth crop, gt uvd, id, colour crop, float32 box, float32 paras,
    combined)."""
    from hn_amd import synth
    g = torch.Generator().manual_seed(seed)
    im = synth.make_crops(k, 176, seed=seed)
    gt = torch.rand((k, 21, 3), generator=g) * torch.tensor([176.0, 176.0, 0.8]) + torch.tensor([0.0, 0.0, 0.4])
    x1, y1 = torch.rand((k,), generator=g) * 380, torch.rand((k,), generator=g) * 260
    box = torch.stack([x1, y1, x1 + 40 + torch.rand((k,), generator=g) * 200, y1 + 40 + torch.rand((k,), generator=g) * 170], dim=1)
    paras = torch.tensor([[617.343, 617.343, 312.42, 241.42]]).repeat(k, 1) + torch.rand((k, 4), generator=g) * 20
    ids = torch.arange(100 * seed, 100 * seed + k, dtype=torch.int64).reshape(k, 1)
    return im, gt, ids, None, box.float(), paras.float(), None


def _rule_on(lines, batches):
    """the rule on what the loop wrote: the float32 values parsed back from its text lines, and the stand-alone conversion of the
    batches' ground truth"""
    from hn_amd import ops
    pred = np.stack([np.array(l.split(",")[1:], dtype=np.float32).reshape(21, 3) for l in lines])
    gt = np.concatenate([ops.convert_joints_samples(b[1].cuda().contiguous(), b[4].cuda(), b[5].cuda(), want_image=False)[1].cpu().numpy()
                         for b in batches])
    thr = np.linspace(0.0, 50.0, 100)
    state, _, _ = H.accumulate(pred, gt, thr)
    return state, H.compute(state, thr)


def test_the_evaluation_loop_end_to_end(tmp_path, a2j_sd):
    """A2JModelLightning with device_metrics(True): test_step on a batch of 1 and of 5, test_epoch_end == the rule on the text
    file's float32 values and ops.convert_joints_samples of the ground truth (same state bytes, same dict); the text file and
    the logged RMSE byte-equal to the run with metrics off; off, test_epoch_end still raises ImportError; a second epoch starts
    from zero."""
    from a2j.a2j import A2JModelLightning
    net = A2JModelLightning(output_dir=str(tmp_path / "off"))
    net.a2j.load_state_dict(a2j_sd, strict=False)
    net = net.cuda().eval()
    batches = [_eval_batch(1, seed=41), _eval_batch(5, seed=42)]
    for step, batch in enumerate(batches):
        net.test_step(batch, step)
    assert net._hpe_metrics is None
    with pytest.raises(ImportError):
        net.test_epoch_end([])
    off_text = (tmp_path / "off" / "a2j_test_metrics" / "s0_test_0.txt").read_bytes()
    off_rmse = list(net.logged["test_rmse"])
    assert list(net.logged) == ["test_rmse"] and net.hpe_results is None

    assert net.device_metrics(True) is net
    net.output_dir = str(tmp_path / "on")
    net.logged.clear()
    for step, batch in enumerate(batches):
        net.test_step(batch, step)
    path = tmp_path / "on" / "a2j_test_metrics" / "s0_test_0.txt"
    assert path.read_bytes() == off_text and net.logged["test_rmse"] == off_rmse and list(net.logged) == ["test_rmse"]
    want_state, want = _rule_on(path.read_text().splitlines(), batches)
    got_state = net._hpe_metrics.state()
    assert want_state["n"].tolist() == [6, 0]
    assert all(got_state[k].tobytes() == want_state[k].tobytes() for k in ("hist", "sum", "n"))
    res = net.test_epoch_end([])
    assert res is net.hpe_results
    for name in H.NAMES:
        assert res[name] == want[name] and math.isfinite(res[name]["mpjpe"]) and 0.0 <= res[name]["auc"] <= 1.0
        assert net.logged[f"test_{name}_mpjpe"] == [want[name]["mpjpe"]] and net.logged[f"test_{name}_auc"] == [want[name]["auc"]]
    assert np.array_equal(res["pck"], want["pck"]) and (res["fed"], res["skipped"]) == (6, 0)
    assert len(net.logged) == 7                                             # the RMSE and the six scalars
    # the second epoch starts from zero
    assert net._hpe_metrics.state()["n"].tolist() == [0, 0] and not net._hpe_metrics.state()["hist"].any()
    extra = _eval_batch(3, seed=43)
    net.test_step(extra, 0)
    want_state, want = _rule_on(path.read_text().splitlines()[6:], [extra])
    res2 = net.test_epoch_end([])
    assert res2["fed"] == 3 and all(res2[name] == want[name] for name in H.NAMES)
    # and off again: the toolkit is asked for, as before
    net.device_metrics(False)
    with pytest.raises(ImportError):
        net.test_epoch_end([])
