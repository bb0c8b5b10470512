#!/usr/bin/env python3 -B
"""Golden vectors for the A2J criterion's backward by IMPORTING the reference.

Runs only in the build container (needs /root/reference).  The function under test is the reference's own
`a2j.anchor.A2J_loss.forward` (a2j/anchor.py:99-153) in float64 with torch's autograd behind it: the scalar
wa * anchor_mean + wr * (reg_loss_factor * regression_mean) is differentiated with `.backward()`, an exact oracle for
tests/loss_grad_ref.py's rule.

    python -B tests/golden/make_golden_loss_grad.py      ->  tests/golden/a2j_loss_grad.npz

Three configurations (P_h = P_w = None: the 4 x 4 anchors of a cell), heads seeded and stored as their seed only, in the
reference's layout [B, (w * fh + h) * 16 + a, J] (tests/golden/make_golden_loss.py heads(); tests/test_loss_grad_cpu.py
regenerates them), ground truth = the reference's own post_process in float64 plus a seeded offset, stored:
  t: k = 2, shape [2, 3], stride 8, J = 3, spatialFactor 0.5, upstream (0.7, 1.9): the three gradients in float64;
  n: k = 3, shape [3, 5], stride 8, J = 7, spatialFactor 0.1, upstream (1, 1), ONE NaN in gt: the three gradients rounded to
     float32 (for the file's size; their NaN masks are what pins the reference's behaviour) and, as for m, their float64 sums;
  m: k = 2, shape [11, 11], stride 16, J = 21, spatialFactor 0.5, upstream (1, 1), the model's: eight seeded directional
     derivatives sum(grad * direction) per head and sum |grad| per head, in float64 (NaN entries left out of the sums of n).
The directions are seeded too: direction d of head h is randn of the head's shape from seed dir_seed + 8 * h + d.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
sys.dont_write_bytecode = True

REG_LOSS_FACTOR = 3.0
DIRECTIONS = 8
CONFIGS = {"t": dict(seed=20261101, k=2, shape=(2, 3), stride=8, joints=3, spatial_factor=0.5, upstream=(0.7, 1.9)),
           "n": dict(seed=20261102, k=3, shape=(3, 5), stride=8, joints=7, spatial_factor=0.1, upstream=(1.0, 1.0), nan_at=(1, 2, 0)),
           "m": dict(seed=20261103, k=2, shape=(11, 11), stride=16, joints=21, spatial_factor=0.5, upstream=(1.0, 1.0))}


def heads(seed, k, shape, joints):
    """tests/golden/make_golden_loss.py's lines"""
    gen = torch.Generator().manual_seed(int(seed))
    n = shape[0] * shape[1] * 16
    cls = torch.randn((k, n, joints), generator=gen) * 2.0
    reg = torch.randn((k, n, joints, 2), generator=gen) * 8.0
    dep = 0.8 + 0.2 * torch.randn((k, n, joints), generator=gen)
    return cls, reg, dep


def directional(grads, seed):
    """([3, DIRECTIONS] sums of grad * direction, [3] sums of |grad|) in float64, NaN entries left out"""
    dots, mags = np.empty((3, DIRECTIONS)), np.empty((3,))
    for h, g in enumerate(grads):
        ok = ~torch.isnan(g)
        mags[h] = g[ok].abs().sum().item()
        for d in range(DIRECTIONS):
            v = torch.randn(g.shape, generator=torch.Generator().manual_seed(int(seed) + 8 * h + d), dtype=torch.float64)
            dots[h, d] = (g[ok] * v[ok]).sum().item()
    return dots, mags


def main():
    sys.path.insert(0, str(REF))
    from a2j.anchor import A2J_loss, post_process            # the reference's own
    out = {"reg_loss_factor": np.float64(REG_LOSS_FACTOR), "directions": np.int64(DIRECTIONS)}
    for name, c in CONFIGS.items():
        cls, reg, dep = (t.double().requires_grad_(True) for t in heads(c["seed"], c["k"], c["shape"], c["joints"]))
        post = post_process(shape=list(c["shape"]), stride=c["stride"], P_h=None, P_w=None).double()
        crit = A2J_loss(shape=list(c["shape"]), thres=[16.0, 32.0], stride=c["stride"], spatialFactor=c["spatial_factor"],
                        img_shape=[c["shape"][0] * c["stride"], c["shape"][1] * c["stride"]], P_h=None, P_w=None).double()
        with torch.no_grad():
            kp = post((cls, reg, dep))
        rng = np.random.default_rng(c["seed"])
        n = c["k"] * c["joints"]
        uv = np.resize(np.array([0.25, 0.9, 1.5, 6.0]), 2 * n)
        rng.shuffle(uv)
        dd = np.resize(np.array([0.01, 0.2]), n)
        rng.shuffle(dd)
        off = np.concatenate([(uv * rng.choice([-1.0, 1.0], 2 * n)).reshape(c["k"], c["joints"], 2),
                              (dd * rng.choice([-1.0, 1.0], n)).reshape(c["k"], c["joints"], 1)], -1)
        gt = (kp + torch.from_numpy(off)).float()
        if "nan_at" in c:
            gt[c["nan_at"]] = float("nan")
        a, r = crit((cls, reg, dep), gt.double())
        wa, wr = c["upstream"]
        (wa * a + wr * (REG_LOSS_FACTOR * r)).sum().backward()
        grads = [t.grad.detach() for t in (cls, reg, dep)]
        out.update({f"{name}_seed": np.int64(c["seed"]), f"{name}_k": np.int64(c["k"]), f"{name}_shape": np.array(c["shape"], np.int64),
                    f"{name}_stride": np.int64(c["stride"]), f"{name}_joints": np.int64(c["joints"]),
                    f"{name}_spatial_factor": np.float64(c["spatial_factor"]), f"{name}_upstream": np.array(c["upstream"], np.float64),
                    f"{name}_gt": gt.numpy(), f"{name}_dir_seed": np.int64(c["seed"] + 1000)})
        if name != "m":
            cast = np.float64 if name == "t" else np.float32
            for key, g in zip(("d_cls", "d_reg", "d_dep"), grads):
                out[f"{name}_{key}"] = g.numpy().astype(cast)
        if name != "t":
            out[f"{name}_dots"], out[f"{name}_mags"] = directional(grads, c["seed"] + 1000)
        print(name, "NaN entries per head", [int(torch.isnan(g).sum()) for g in grads], "sum |grad|", [float(g[~torch.isnan(g)].abs().sum()) for g in grads])
    np.savez_compressed(HERE / "a2j_loss_grad.npz", **out)
    print("wrote", HERE / "a2j_loss_grad.npz", (HERE / "a2j_loss_grad.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
