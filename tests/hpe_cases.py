"""Inputs for the evaluator's tables (tests/hpe_ref.py): batches that hold, besides hand-like samples, every kind of row the rule
names -- reflected and scaled predictions, skipped samples (valid = 0, a NaN, an inf, a value of 2^20), rank-deficient sets (all
prediction joints equal, collinear sets, coplanar ground truth) and the exact-threshold samples.  Shared by the CPU and the GPU
tests; row i of a batch is of kind KINDS[i % len(KINDS)], so a batch of 12 and more holds them all and the small ones the first."""
import numpy as np

KINDS = ("plain", "reflected", "invalid", "equal", "collinear", "coplanar", "nan", "inf", "limit", "same", "exact50", "above50")
SKIPPED = ("invalid", "nan", "inf", "limit")
WAVES = 4                  # samples per workgroup of the kernel (hn_amd.ops.HPE_WAVES_PER_GROUP; the CPU test pins the two together)
# (S, J, T) of the GPU comparison: one sample; three; one workgroup's waves; that + 1; many workgroups with a tail; one joint and
# one threshold; every lane a joint and an odd threshold count; the empty batch
SHAPES = ((1, 21, 100), (3, 21, 100), (WAVES, 21, 100), (WAVES + 1, 21, 100), (257, 21, 100), (5, 1, 1), (5, 64, 101), (0, 21, 100))


def thresholds(t):
    return np.linspace(0.0, 50.0, t) if t > 1 else np.array([25.0])


def batch(s, j, seed):
    """-> pred fp32 [s,j,3], gt fp32 [s,j,3], valid int32 [s], kinds (a list of s names)"""
    rng = np.random.RandomState(seed)
    pred, gt = np.zeros((s, j, 3), np.float32), np.zeros((s, j, 3), np.float32)
    valid = np.ones((s,), np.int32)
    kinds = [KINDS[i % len(KINDS)] for i in range(s)]
    for i, kind in enumerate(kinds):
        centre = np.array([rng.uniform(-250, 250), rng.uniform(-250, 250), rng.uniform(350, 950)])
        hand = centre + rng.uniform(-0.5, 0.5, (j, 3)) * rng.uniform(60, 120, 3)
        noisy = hand + rng.normal(0, rng.uniform(2, 40) / np.sqrt(3.0), (j, 3))
        if kind == "reflected":
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            if np.linalg.det(q) > 0:
                q[:, 0] = -q[:, 0]
            noisy = (hand - hand.mean(0)) @ q.T * rng.uniform(0.5, 1.8) + centre + rng.uniform(-80, 80, 3) + rng.normal(0, 2, (j, 3))
        elif kind == "equal":
            noisy = np.tile(centre + rng.uniform(-30, 30, 3), (j, 1))
        elif kind == "collinear":
            step = rng.normal(size=3)
            hand = centre + np.arange(j)[:, None] * step * 4.0
            noisy = centre + 7.0 + np.arange(j)[:, None] * rng.normal(size=3) * 4.0
        elif kind == "coplanar":
            hand[:, 2] = np.float32(centre[2])
        elif kind == "same":
            noisy = hand
        elif kind in ("exact50", "above50"):
            hand = np.round(hand)                                # integers: the differences below are exact in fp32 and fp64
            noisy = hand - np.array([30.0, 40.0, 0.0 if kind == "exact50" else 0.5])
        gt[i], pred[i] = hand.astype(np.float32), noisy.astype(np.float32)
        if kind == "invalid":
            valid[i] = 0
        elif kind == "nan":
            pred[i, rng.randint(j), rng.randint(3)] = np.nan
        elif kind == "inf":
            gt[i, rng.randint(j), rng.randint(3)] = -np.inf
        elif kind == "limit":
            pred[i, rng.randint(j), rng.randint(3)] = np.float32(2.0 ** 20)
    return pred, gt, valid, kinds
