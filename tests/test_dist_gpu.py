"""N > 1 on the real engine (GPU box): two ranks sharing cuda:0 (gloo rehearsal; an 8-GPU node is not available to
the tests) must reproduce the single-process batch, and `bench.py --gpus 2` must launch its own two ranks."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_equal_single_process_batch(tmp_path, fcos_sd, a2j_sd):
    """2 ranks x 16 frames == 1 rank x 32 frames through HandNetEngine: crop boxes and has_hand bit-for-bit,
    keypoints <= 2.5e-4 (the contract is 1e-3 against the reference; a 16-frame batch may pick other conv tiles / split-K plans, i.e. another fp32 summation
    order, than the 32-frame batch)."""
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    total, world = 32, 2
    port = _free_port()
    out_file = tmp_path / "gathered.pt"
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(REPO / "tests" / "dist_worker.py"), str(total), "gloo",
                                       str(out_file)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    kp, box, has, w = torch.load(out_file)
    assert w == world and kp.shape == (total, 21, 3)
    eng = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    ref = eng.forward_device(synth.make_rgb(total, seed=1000).cuda(), synth.make_depth(total, seed=2000).cuda())
    assert torch.equal(box, ref.crop_box.cpu())
    assert torch.equal(has, ref.has_hand.cpu())
    assert (kp - ref.keypoints.cpu()).abs().max().item() <= 2.5e-4   # (14 ulps at 100 px: other split-K plans, i.e. another fp32 summation order)


def test_rccl_single_rank_gather(tmp_path, fcos_sd, a2j_sd):
    """The RCCL leg on the one GPU this box has: a single-rank "nccl" process group (ncclCommInitRank on the device,
    all_gather_into_tensor of the packed uint8 records on the current stream) around the real engine; what comes back
    equals the in-process result bit for bit."""
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    total = 8
    out_file = tmp_path / "gathered_rccl.pt"
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(REPO / "tests" / "dist_worker.py"), str(total), "nccl", str(out_file)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    kp, box, has, w = torch.load(out_file)
    assert w == 1 and kp.shape == (total, 21, 3)
    eng = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    ref = eng.forward_device(synth.make_rgb(total, seed=1000).cuda(), synth.make_depth(total, seed=2000).cuda())
    assert torch.equal(box, ref.crop_box.cpu()) and torch.equal(has, ref.has_hand.cpu())
    assert torch.equal(kp, ref.keypoints.cpu())


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` without a torchrun environment starts two ranks itself (never a silent
    single-GPU run) and rank 0 prints one JSON line with n_gpus = 2."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--share-gpu", "--dist-backend", "gloo",
                        "--steps", "2", "--warmup", "1", "--batch", "4", "--no-cpu-baseline", "--no-roofline"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 8 and line["config"]["rccl_ranks"] == 2
    assert line["config"]["collective_backend"] == "gloo" and line["value"] > 0


def test_bench_refuses_world_size_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stdout + r.stderr)


def test_bench_line_contract():
    """The one JSON line of the driver contract: metric / value / unit / n_gpus / steps / warmup / ms_per_step /
    higher_is_better / scaling / vs_baseline / dtype / data / config.workload, plus (--full) the roofline and cpu_baseline
    objects with their required keys; clock sampled in-kernel; parity figures over the CPU sample."""
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--cpu-frames", "2", "--full"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "other_configs", "dropin", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["vs_baseline"] is None
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 2 * 2 / (d["ms_per_step"] * 2e-3)) < 0.02 * d["value"]
    roof = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "kernel", "clock_mhz"):
        assert k in roof, k
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and roof["peak"] == 2500.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert 400.0 < roof["clock_mhz"] < 2600.0                       # s_memtime / s_memrealtime under load
    # batch 2 != the profiled batch 32 (or, between collections, a PMC file of an older kernel revision): never paired
    # (... or, on a box whose timing puts another kernel first at this small batch, "this run's dominant kernel is ...")
    assert roof["traffic"] is None and any(why in roof["traffic_source"] for why in
                                           ("launches/step", "another revision", "dominant kernel"))
    assert set(roof["stages"]) >= {"resnet34_body", "fpn", "towers", "head_outputs", "a2j_trunk", "a2j_heads"}
    oc = d["other_configs"]
    assert set(oc) == {"a2j_b64", "fcos_b16", "pipeline_b1", "pipeline_b32_f32", "pose2mesh_b1", "pose2mesh_b32", "live_b1", "crop_mesh_b1"}
    assert oc["pose2mesh_b1"]["unit"] == "meshes/s" and oc["pose2mesh_b32"]["value"] > oc["pose2mesh_b1"]["value"] > 0
    live = oc["live_b1"]
    assert 0 < oc["crop_mesh_b1"]["ms_per_step"] < live["ms_per_step"] and oc["crop_mesh_b1"]["unit"] == "crops/s"
    assert live["frames_with_hand"] == 1 and live["mesh_vertices"] > 700 and live["ms_per_step"] > oc["pipeline_b1"]["ms_per_step"]
    oc = {k: v for k, v in oc.items() if k not in ("pose2mesh_b1", "pose2mesh_b32", "live_b1", "crop_mesh_b1")}
    for name, unit in (("a2j_b64", "crops/s"), ("fcos_b16", "frames/s"), ("pipeline_b1", "frames/s"), ("pipeline_b32_f32", "frames/s")):
        assert oc[name]["unit"] == unit and oc[name]["value"] > 0 and oc[name]["ms_per_step"] > 0
        assert 0 < oc[name]["frac"] < 1 and "conv_igemm" in oc[name]["kernel"]
        assert "median" in oc[name]["timing"] and oc[name]["ms_per_step_worst_group"] >= oc[name]["ms_per_step"]
    assert all(oc[k]["hipgraph"] is True for k in oc if k != "pipeline_b32_f32")
    assert oc["pipeline_b1"]["ms_per_step"] < 200.0   # (2.2 ms alone; 28 ms next to a load process)
    # the exact-f32 leg: the reference's own arithmetic beside the split-fp16 headline, priced against the f32-MFMA peak
    f32 = oc["pipeline_b32_f32"]
    assert "conv_igemm_f32" in f32["kernel"] and f32["peak_tflops"] == 157.3 and f32["dtype"].startswith("f32")
    assert abs(f32["frac"] - f32["achieved_tflops"] / 157.3) < 1e-3
    # BASELINE config 2 / 3 in their own parity terms, taken on the outputs of the timed steps
    pa = oc["a2j_b64"]["parity"]
    assert pa["crops"] == 16 and pa["keypoints_within_tolerance"] is True and pa["max_abs_uvd_diff"] < 1e-3 and pa["mm_epe"] < 0.05
    pf = oc["fcos_b16"]["parity"]
    assert pf["frames"] == 2 and pf["matched_survivors"] > 0 and pf["label_equality_rate"] == 1.0
    assert pf["survivor_index_set_equal_frames"] == 2 and pf["min_box_iou"] > 0.999
    # the live chain's own parity: the captured step's host record against the oracle's chain on the same frame
    pl = live["parity"]
    assert pl["frames"] == 1 and pl["crop_box_identical"] == 1 and pl["mesh_within_tolerance"] is True
    assert pl["max_abs_keypoint_diff"] < 1e-3 and pl["max_abs_xyz_diff_mm"] < 2e-2 and pl["max_abs_mesh_vertex_diff"] < 2e-3
    dr = d["dropin"]
    assert dr["batch1"]["frames_per_s"] > 0 and dr["batch2"]["frames_per_s"] > 0 and "HandNet.forward" in dr["call"]
    cpu = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample", "parity"):
        assert k in cpu, k
    assert cpu["kind"] == "port" and cpu["cores"] >= 1 and cpu["parity"]["frames"] == 2
    assert "ONE pass" in cpu["sample"] and cpu["batch1"]["value"] > 0 and "median of 5" in cpu["batch1"]["sample"]
    assert cpu["parity"]["keypoints_within_tolerance"] is True
    assert cpu["live_batch1"]["value"] > 0 and 0 < cpu["live_batch1"]["lifter_ms"] < cpu["live_batch1"]["ms_per_frame"]


def test_bench_plain_run_dumps_what_the_engine_returns(tmp_path, fcos_sd, a2j_sd):
    """The plain line (no --full): the headline only, the other objects null; --dump-outputs holds the last timed step's
    results, bit for bit what the same engine returns for the same seeded frames in this process."""
    import numpy as np
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "frames/s"
    assert d["roofline"] is None and d["other_configs"] is None and d["dropin"] is None and d["cpu_baseline"] is None
    eng = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    ref = eng.forward_device(synth.make_rgb(2, seed=1000).cuda(), synth.make_depth(2, seed=2000).cuda())
    torch.cuda.synchronize()
    for name in ("keypoints", "crop_box", "has_hand", "crops_nhwc"):
        got, want = np.load(out / f"{name}.npy"), getattr(ref, name).cpu().numpy()
        assert got.dtype in (np.float32, np.float64) and got.shape == want.shape, name
        assert np.array_equal(got, want.astype(got.dtype), equal_nan=True), name
    cnt = ref.detections.count.cpu().numpy()
    boxes = np.load(out / "detections_boxes.npy")
    for i, k in enumerate(cnt):
        assert np.array_equal(boxes[i, :k], ref.detections.boxes[i, :k].cpu().numpy()) and not boxes[i, k:].any()


def test_four_ranks_equal_single_process_batch(tmp_path, fcos_sd, a2j_sd):
    """4 ranks x 8 frames == 1 x 32 frames through the real engine (crop boxes / has_hand bit-for-bit).  Four, not
    eight: the GPU box's process guard allows six GPU-touching processes (this test process is one of them); the
    8-rank rendezvous / sharding / record plumbing runs on gloo in tests/test_dist_cpu.py."""
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    total, world = 32, 4
    port = _free_port()
    out_file = tmp_path / "gathered4.pt"
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(REPO / "tests" / "dist_worker.py"), str(total), "gloo",
                                       str(out_file)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    kp, box, has, w = torch.load(out_file)
    assert w == world and kp.shape == (total, 21, 3)
    eng = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    ref = eng.forward_device(synth.make_rgb(total, seed=1000).cuda(), synth.make_depth(total, seed=2000).cuda())
    assert torch.equal(box, ref.crop_box.cpu()) and torch.equal(has, ref.has_hand.cpu())
    assert (kp - ref.keypoints.cpu()).abs().max().item() <= 2.5e-4   # (14 ulps at 100 px: other split-K plans, i.e. another fp32 summation order)


def test_bench_four_rank_rehearsal_with_a_failed_first_attempt():
    """`bench.py --gpus 4 --share-gpu --dist-backend gloo --batch 8`: the self-launch path at a world size > 2 (global
    batch 32 as 4 x 8) on the REAL engine, one JSON line from rank 0 -- with the launch ladder exercised: rank 3's process
    group "cannot start" on the first attempt (injected: what a host with the other IPC-handle mode looks like), the three
    ranks waiting in the rendezvous are stopped by pid, ONE fresh set runs with HSA_ENABLE_IPC_MODE_LEGACY unset and the line
    says so.  N > 1 replays the step from a hipGraph by default and reports every rank's own time per step.
    FOUR is the largest world this box rehearses: its process guard allows six processes with the device open (this test
    process and the four workers; the supervisor never opens the device)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "HN_BENCH_WORKER")}
    env["HN_BENCH_INJECT_INIT_FAILURE"] = "3:0"
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "4", "--share-gpu", "--dist-backend", "gloo",
                        "--steps", "2", "--warmup", "1", "--batch", "8", "--no-cpu-baseline", "--no-roofline"],
                       env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    cfg = line["config"]
    assert line["n_gpus"] == 4 and cfg["global_batch"] == 32 and cfg["rccl_ranks"] == 4
    assert "HSA_ENABLE_IPC_MODE_LEGACY unset" in cfg["ipc_mode"] and "attempt 2 of 2" in cfg["ipc_mode"]
    assert cfg["hipgraph"] is True
    assert len(cfg["devices"]) == 4 and len(set(cfg["devices"])) == 1 and ":" in cfg["devices"][0]   # --share-gpu: one PCI bus id
    lo, med, hi = line["rank_ms"]["min_median_max"]
    assert len(line["rank_ms"]["per_rank"]) == 4 and 0 < lo <= med <= hi


def test_bench_under_real_torchrun():
    """The driver's launch form on the REAL engine: `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr
    127.0.0.1 --master-port P bench.py --gpus 2 ...` (two ranks sharing the GPU, gloo).  Each process torchrun starts
    supervises the fresh worker of its own rank; the workers rendezvous through the job's shared file:// store; rank 0
    prints the line.  (GPU-touching processes: this test, two workers.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "HN_BENCH_WORKER")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(_free_port()), str(REPO / "bench.py"), "--gpus", "2", "--share-gpu",
                        "--dist-backend", "gloo", "--steps", "2", "--warmup", "1", "--batch", "4", "--no-cpu-baseline",
                        "--no-roofline"], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout + r.stderr
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["config"]["rccl_ranks"] == 2 and "attempt 1 of 2" in line["config"]["ipc_mode"]
    assert line["config"]["hipgraph"] is True and len(line["rank_ms"]["per_rank"]) == 2


def test_stages_are_repeatable_next_to_a_second_process(fcos_sd, a2j_sd):
    """Round 4: with a second process at work on the same card the SLP-vectorised blend of the tiled preprocess kernel
    (`v_pk_fma_f32 ... op_sel:[0,1,0]`) returned wrong values in lanes 48-63 of ~3 % of its waves -- alone on the card the same
    binary is exact (profiles/NOTEBOOK.md, tools/probes/pk_opsel_probe.hip).  The library is built without such instructions now
    (hn_amd/build.py); this test keeps a load process on the card and asserts that the preprocess equals its per-pixel form on
    every call and that the whole pipeline is bit-identical from call to call."""
    from hn_amd import ops, synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import IMAGE_MEAN, IMAGE_STD, FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    load = subprocess.Popen([sys.executable, str(REPO / "tests" / "card_load.py"), "90"], stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    try:
        line = ""
        while "loading" not in line:
            line = load.stdout.readline()
            assert line or load.poll() is None, "the load process ended before it produced work"
        rgb = synth.make_rgb(16, seed=1000).cuda()
        args = (rgb, 799, 1066, 800, 1088, IMAGE_MEAN, IMAGE_STD)
        ops.set_form("preprocess_generic", True)
        try:
            ref = ops.fcos_preprocess_split(*args)
        finally:
            ops.set_form("preprocess_generic", False)
        for _ in range(8):
            assert torch.equal(ops.fcos_preprocess_split(*args), ref)
        eng = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
        depth = synth.make_depth(16, seed=2000).cuda()
        first = eng.forward_device(rgb, depth)
        for _ in range(5):
            out = eng.forward_device(rgb, depth)
            assert torch.equal(out.crop_box, first.crop_box)
            assert torch.equal(out.keypoints.view(torch.int32), first.keypoints.view(torch.int32))
        assert load.poll() is None, "the load process ended before the checks did: nothing shared the card"
    finally:
        load.kill()
        load.wait()


def test_bench_ladder_with_a_real_rccl_initialisation_failure():
    """A REAL (not injected) RCCL failure: two ranks on the SAME GPU with the nccl backend -- RCCL refuses duplicate devices when
    the communicator is created.  Both rungs of the ladder must run and fail on the backend's own error, bench.py must exit
    non-zero with that error text and without a JSON line: never a gloo fallback, never a single-rank result."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "HN_BENCH_WORKER")}
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--share-gpu", "--dist-backend", "nccl",
                        "--steps", "1", "--warmup", "0", "--batch", "2", "--no-cpu-baseline", "--no-roofline", "--init-timeout", "60"],
                       env=env, capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode != 0, out
    assert not any(l.startswith("{") for l in r.stdout.splitlines()), r.stdout
    assert "attempt 1 failed to initialise" in r.stderr and "attempt 2 failed to initialise" in r.stderr, out
    assert "HSA_ENABLE_IPC_MODE_LEGACY unset" in r.stderr


def _reference_tuple(eng, total):
    """handnet_pipeline.HandNet.forward's tuple for the whole batch from ONE single-process step of the same engines."""
    from hn_amd import synth
    out = eng.forward_device(synth.make_rgb(total, seed=1000).cuda(), synth.make_depth(total, seed=2000).cuda())
    mask = out.has_hand != 0
    return out.keypoints.cpu(), out.crops_nhwc[..., 0].unsqueeze(1)[mask].cpu(), out.crop_box[mask].cpu()


def test_sharded_handnet_two_ranks_sharing_the_card(tmp_path, fcos_sd, a2j_sd):
    """hn_amd.dist.ShardedHandNet (BASELINE config 5's callable) on the REAL engine: two ranks sharing cuda:0 (gloo: the
    records travel through the host) each return the reference's tuple over the GLOBAL batch -- crop boxes and depth crops
    bit-for-bit the single-process step's, keypoints within the batch-size summation-order difference."""
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    total, world = 16, 2
    port = _free_port()
    out_file = tmp_path / "sharded.pt"
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(REPO / "tests" / "dist_worker.py"), str(total), "gloo",
                                       str(out_file), "sharded"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    eng = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    kp, depth_batch, crops = _reference_tuple(eng, total)
    for rank in range(world):
        g_kp, g_depth, g_crops, w, _cap, _note = torch.load(str(out_file) + f".rank{rank}")
        assert w == world and tuple(g_kp.shape) == (total, 21, 3)
        assert torch.equal(g_crops, crops) and torch.equal(g_depth, depth_batch)
        assert (g_kp - kp).abs().max().item() <= 2.5e-4


def test_sharded_handnet_rccl_single_rank_with_the_gather_in_the_graph(tmp_path, fcos_sd, a2j_sd):
    """The RCCL leg on the one GPU of this box: a single-rank "nccl" group; from the third call on ShardedHandNet replays the
    step AND both collectives (records, depth crops) from ONE hipGraph when RCCL lets itself be captured (the worker asserts
    that replayed results equal the eager ones) -- or says why not and keeps the gather eager.  Results are the in-process
    step's bit for bit either way."""
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    total = 8
    out_file = tmp_path / "sharded_rccl.pt"
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(REPO / "tests" / "dist_worker.py"), str(total), "nccl", str(out_file), "sharded"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    g_kp, g_depth, g_crops, w, captured, note = torch.load(str(out_file) + ".rank0")
    print("ShardedHandNet on a single-rank RCCL group:", note)
    assert w == 1 and captured in (True, False) and note
    eng = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    kp, depth_batch, crops = _reference_tuple(eng, total)
    assert torch.equal(g_crops, crops) and torch.equal(g_depth, depth_batch) and torch.equal(g_kp, kp)


def test_sharded_handnet_rgbd_engine_without_a_group_equals_the_engine_step(fcos_sd, a2j_rgbd_sd):
    """The RGB-D model (4-channel crops, [2,1,0,3] order) through ShardedHandNet without a process group (world 1: the records
    take the same pack -> "gather" -> unpack path): the tuple is the engine step's own -- keypoints and crop boxes bit for
    bit, depth_batch = the four-channel crops -- eager and replayed (the third call captures)."""
    from hn_amd import dist as hdist
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    eng = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_rgbd_sd, rgbd=True, device="cuda"), 3)
    n = 4
    rgb = synth.make_rgb(n, seed=1000).cuda()
    rgbd = torch.cat([rgb, synth.make_depth(n, seed=2000).cuda()], dim=1)
    ref = eng.forward_device(rgb, rgbd)
    mask = ref.has_hand != 0
    assert int(mask.sum()) == n
    net = hdist.ShardedHandNet(eng, gather_depth=True, rgbd=True)
    for call in range(5):
        kp, depth_batch, crops = net([rgb[i] for i in range(n)], depth_images=rgbd)
        assert kp.device.type == "cpu" and torch.equal(kp, ref.keypoints.cpu()) and torch.equal(crops, ref.crop_box)
        assert tuple(depth_batch.shape) == (n, 4, 176, 176) and torch.equal(depth_batch, ref.crops_nhwc.permute(0, 3, 1, 2))
    assert net.gather_captured is True and "ONE hipGraph" in net.capture_note
    # use_graph="step" (what bench.py --gpus N times by default): the engine's own captured step, the gather eager behind it
    step = hdist.ShardedHandNet(eng, gather_depth=True, rgbd=True, use_graph="step")
    for call in range(3):
        kp, depth_batch, crops = step([rgb[i] for i in range(n)], depth_images=rgbd)
        assert torch.equal(kp, ref.keypoints.cpu()) and torch.equal(crops, ref.crop_box)
        assert torch.equal(depth_batch, ref.crops_nhwc.permute(0, 3, 1, 2))
    assert step.gather_captured is None and "eagerly" in step.capture_note and eng.graph_count() >= 1
