#!/usr/bin/env python3 -B
"""Golden vectors for the A2J criterion by IMPORTING the reference.

Runs only in the build container (needs /root/reference).  The function under test is the reference's own
`a2j.anchor.A2J_loss.forward` (a2j/anchor.py:99-153), which imports cleanly (numpy and torch only) and runs in float64: an exact
oracle for tests/loss_ref.py's rule.

    python -B tests/golden/make_golden_loss.py      ->  tests/golden/a2j_loss.npz

Two configurations, as A2JModel builds the criterion (P_h = P_w = None: the 4 x 4 anchors of a cell): shape [11, 11], stride 16,
spatialFactor 0.5 (the model's) and a non-square shape [3, 5], stride 8, spatialFactor 0.1.  The heads are seeded and stored as
their seed only (tests/test_loss_cpu.py regenerates them, as tests/test_agg_cpu.py does for a2j_post_process.npz), in the
reference's layout [B, (w * fh + h) * 16 + a, J]; the ground truth = the reference's own post_process in float64 plus a seeded
offset on both sides of the smooth-L1 knee, stored.  The criterion runs in float64 and in float32, on the whole batch and sample
by sample (a batch of one: its mean over the samples is the sample's value).
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
sys.dont_write_bytecode = True

CONFIGS = {"a": dict(seed=20261020, k=4, shape=(11, 11), stride=16, joints=21, spatial_factor=0.5),
           "b": dict(seed=20261021, k=3, shape=(3, 5), stride=8, joints=7, spatial_factor=0.1)}


def heads(seed, k, shape, joints):
    """the seeded heads in the reference's layout (float32 values); tests/test_loss_cpu.py holds the same lines"""
    gen = torch.Generator().manual_seed(int(seed))
    n = shape[0] * shape[1] * 16
    cls = torch.randn((k, n, joints), generator=gen) * 2.0
    reg = torch.randn((k, n, joints, 2), generator=gen) * 8.0
    dep = 0.8 + 0.2 * torch.randn((k, n, joints), generator=gen)
    return cls, reg, dep


def main():
    sys.path.insert(0, str(REF))
    from a2j.anchor import A2J_loss, post_process            # the reference's own
    out = {}
    for name, c in CONFIGS.items():
        cls, reg, dep = heads(c["seed"], c["k"], c["shape"], c["joints"])
        post = post_process(shape=list(c["shape"]), stride=c["stride"], P_h=None, P_w=None).double()
        crit = A2J_loss(shape=list(c["shape"]), thres=[16.0, 32.0], stride=c["stride"], spatialFactor=c["spatial_factor"],
                        img_shape=[c["shape"][0] * c["stride"], c["shape"][1] * c["stride"]], P_h=None, P_w=None)
        kp = post((cls.double(), reg.double(), dep.double()))
        rng = np.random.default_rng(c["seed"])
        n = c["k"] * c["joints"]
        uv = np.resize(np.array([0.25, 0.9, 1.5, 6.0]), 2 * n)
        rng.shuffle(uv)
        dd = np.resize(np.array([0.01, 0.2]), n)
        rng.shuffle(dd)
        off = np.concatenate([(uv * rng.choice([-1.0, 1.0], 2 * n)).reshape(c["k"], c["joints"], 2),
                              (dd * rng.choice([-1.0, 1.0], n)).reshape(c["k"], c["joints"], 1)], -1)
        gt = (kp + torch.from_numpy(off)).float()
        out.update({f"{name}_seed": np.int64(c["seed"]), f"{name}_k": np.int64(c["k"]), f"{name}_shape": np.array(c["shape"], np.int64),
                    f"{name}_stride": np.int64(c["stride"]), f"{name}_joints": np.int64(c["joints"]),
                    f"{name}_spatial_factor": np.float64(c["spatial_factor"]), f"{name}_gt": gt.numpy()})
        for tag, cast in (("f64", torch.float64), ("f32", torch.float32)):
            m = crit.to(cast)
            h = tuple(t.to(cast) for t in (cls, reg, dep))
            a, r = m(h, gt.to(cast))
            assert a.shape == (1,) and r.shape == (1,)
            rows = [m(tuple(t[i:i + 1] for t in h), gt[i:i + 1].to(cast)) for i in range(c["k"])]
            out[f"{name}_{tag}_batch"] = np.array([a.item(), r.item()], np.float64)
            out[f"{name}_{tag}_sample"] = np.array([[x.item(), y.item()] for x, y in rows], np.float64)
        print(name, "batch f64", out[f"{name}_f64_batch"], "f32 - f64", out[f"{name}_f32_batch"] - out[f"{name}_f64_batch"])
    np.savez_compressed(HERE / "a2j_loss.npz", **out)
    print("wrote", HERE / "a2j_loss.npz")


if __name__ == "__main__":
    main()
