"""One FCOS tower layer at batch-32 shapes: does the GroupNorm apply pass hide in the tails of the tower convolutions?
    grouped + pass   the lock-step schedule: ONE grouped launch (cls + reg, three levels each) and the stand-alone apply pass
    grouped / pass   its two parts alone
    cls + reg        the two towers as two launches, no carried pass (the cost of un-grouping)
    cls + reg carry  the two launches, each carrying the other tower's half of the pass (the carried schedule's layer)
Minimum of two rounds of 20 repetitions each, HIP events around a round.  argv[1] = batch (default 32)."""
import sys
from pathlib import Path
from types import SimpleNamespace as NS
R = Path(__file__).resolve().parents[3]
sys.path.insert(0, str(R / "handnet-pipeline_amd"))
import torch
from hn_amd import ops
from hn_amd.weights import split_f16x3

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
dims = ((100, 136), (50, 68), (25, 34))
L = len(dims)
g = torch.Generator().manual_seed(0)
a = [ops.to_split(torch.randn((n, h, w, 512), generator=g).cuda()) for h, w in dims]          # this layer's operand
a2 = [torch.empty_like(x) for x in a]                                                        # the next layer's
raw = [torch.randn((n, h, w, 512), generator=g).cuda() for h, w in dims]                      # a finished layer output
y = [torch.empty((n, h, w, 512), device="cuda") for h, w in dims]
parts = [torch.empty((ops.gn_rows32_scratch_floats(n * h * w, 512),), device="cuda") for h, w in dims]
aff = [((torch.rand((n, 512), generator=g) + 0.5).cuda(), (torch.randn((n, 512), generator=g) * 0.1).cuda()) for _ in dims]
cws = []
for _ in range(2):
    wt = torch.randn((256, 3, 3, 256), generator=g) * 0.03
    cws.append(NS(w=wt.cuda(), bias=torch.zeros((256,)).cuda(), w16=split_f16x3(wt).cuda()))
blocks = lambda xs, k: [x[:, :, :, 8 * k:8 * (k + 1)] for x in xs]   # noqa: E731
half = lambda xs, k: [x[..., 256 * k:256 * (k + 1)] for x in xs]     # noqa: E731
tabs = lambda k: [(sc[:, 256 * k:256 * (k + 1)], sh[:, 256 * k:256 * (k + 1)]) for sc, sh in aff]   # noqa: E731


def grouped():
    ops.conv2d_nhwc_grouped(blocks(a, 0) + blocks(a, 1), [cws[0]] * L + [cws[1]] * L, pad=1, outs=y + y,
                            out_channel_offsets=[0] * L + [256] * L,
                            gn=[(p, 0) for p in parts] + [(p, 32) for p in parts], gn_units=64)


def apply_pass():
    ops.to_split_levels(raw, aff, relu=True, outs=a2)


def tower(k, carry):
    job = (half(raw, 1 - k), tabs(1 - k), blocks(a2, 1 - k), True) if carry else None
    ops.conv2d_nhwc_grouped(blocks(a, k), [cws[k]] * L, pad=1, outs=y, out_channel_offsets=[256 * k] * L,
                            gn=[(p, 32 * k) for p in parts], gn_units=64, carry=job)


def timed(fn, reps=20, rounds=2):
    for _ in range(3):
        fn()
    best = 1e9
    for _ in range(rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best * 1e3


if not ops.conv2d_nhwc_grouped(blocks(a, 0), [cws[0]] * L, pad=1, carry_query=True):
    print(f"batch {n}: the tower launch would not carry (another tile form): the engine keeps the lock-step schedule")
    sys.exit(0)
rows = [("grouped + pass", lambda: (grouped(), apply_pass())), ("grouped", grouped), ("pass", apply_pass),
        ("cls + reg", lambda: (tower(0, False), tower(1, False))), ("cls + reg carry", lambda: (tower(0, True), tower(1, True)))]
res = {name: timed(fn) for name, fn in rows}
print(f"tower layer, batch {n}, levels {dims}: us per layer (min of 2 rounds x 20)")
for name, _ in rows:
    print(f"  {name:16s} {res[name]:8.1f}")
chunks = sum(n * -(-h * w // 64) for h, w in dims)
print(f"  carried pair - plain pair: {res['cls + reg carry'] - res['cls + reg']:+.1f} us for {chunks} chunks per launch;"
      f" against grouped + pass: {res['cls + reg carry'] - res['grouped + pass']:+.1f} us")
