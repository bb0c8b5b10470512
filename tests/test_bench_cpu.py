"""bench.py's plain run and --dump-outputs on CPU, with the stub engine (--stub-engine: records are a pure function of
(rank, frame), frame i of rank r has keypoints[i, 0, 0] == crop_box[i, 0] == 100 r + i)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "HN_BENCH_WORKER")}
    r = subprocess.run([sys.executable, str(REPO / "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {p.name[:-4]: np.load(p) for p in sorted(Path(d).glob("*.npy"))}


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """--steps sets the timed steps and ms_per_step is their time; the plain line leaves the --full objects null; the dump
    holds the step's results as float32 / float64, the same from run to run."""
    runs = []
    for i in range(2):
        d = _bench(["--gpus", "1", "--stub-engine", "--steps", "5", "--warmup", "2", "--batch", "4",
                    "--dump-outputs", str(tmp_path / f"run{i}")])
        assert d["steps"] == 5 and d["warmup"] == 2 and d["ms_per_step"] >= 2.0     # (the stub's step sleeps 2 ms)
        assert abs(d["value"] - 4 * 5 / (d["ms_per_step"] * 5e-3)) < 0.02 * d["value"]
        assert d["roofline"] is None and d["other_configs"] is None and d["dropin"] is None and d["cpu_baseline"] is None
        runs.append(_load(tmp_path / f"run{i}"))
    a, b = runs
    assert set(a) >= {"keypoints", "crop_box", "has_hand"} and set(a) == set(b)
    for name, arr in a.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert np.array_equal(arr, b[name]), name
    assert a["keypoints"].shape == (4, 21, 3) and a["keypoints"].dtype == np.float32
    assert a["crop_box"].dtype == np.float64 and a["crop_box"][:, 0].tolist() == [0, 1, 2, 3]
    assert a["has_hand"].tolist() == [1, 1, 1, 1]


def test_dump_above_64_mb_is_a_seeded_sample_of_rows(tmp_path):
    """160 frames of 176 x 176 x 4 crops are 79 MB: every array keeps the same seeded rows, their indices beside them."""
    out = tmp_path / "dump"
    _bench(["--gpus", "1", "--stub-engine", "--steps", "1", "--warmup", "0", "--batch", "160", "--dump-outputs", str(out)])
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
    a = _load(out)
    rows = a["keypoints.rows"]
    assert 1 <= len(rows) < 160 and np.array_equal(rows, a["crop_box.rows"]) and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["keypoints"][:, 0, 0], rows) and np.array_equal(a["crop_box"][:, 0], rows)
    assert a["crops_nhwc"].shape == (len(rows), 176, 176, 4)


def test_dump_of_two_ranks_holds_the_global_batch(tmp_path):
    out = tmp_path / "dump"
    _bench(["--gpus", "2", "--stub-engine", "--dist-backend", "gloo", "--steps", "2", "--warmup", "1", "--batch", "4",
            "--init-timeout", "60", "--dump-outputs", str(out)])
    a = _load(out)
    assert a["keypoints"].shape == (8, 21, 3)
    assert a["crop_box"][:, 0].tolist() == [0, 1, 2, 3, 100, 101, 102, 103]
