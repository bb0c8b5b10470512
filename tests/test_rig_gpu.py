"""The rig frame on the GPU (csrc/rig_ops.hip through ops.rig_fuse, and the live_hands step with extrinsics=) against the rule
in numpy float32 (tests/rig_ref.py), bit for bit: no tolerance appears in this file."""
import functools

import numpy as np
import pytest
import torch

import rig_cases as rc
import rig_ref as rr
from hn_amd.ops import RIG_FIELDS          # (the eight outputs, in the order the step delivers them)

pytestmark = pytest.mark.gpu

LIFTER_OUTPUT_SCALE = 0.01       # the hand-sized lifter of tests/test_render_gpu.py (its last graph convolution x 0.01)


def _bytes(a):
    return np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a).tobytes()


# ---------------------------------------------------------------------------------------------------------------- op level
@functools.lru_cache(maxsize=None)
def _case(kind, n, k, v, handed):
    """(inputs, what the rule makes of them): worked out once, shared, never changed"""
    case = rc.edge_case(n, k, v) if kind == "edges" else rc.random_case(n, k, v, rc.SEEDS[n, k, v], handed=handed)
    if kind == "edges" and not handed:
        case = case._replace(side=None)
    want = rr.rig_fuse(case.xyz_mm, case.mesh, case.has_hand, case.lifted, case.score, rr.table(case.ext), case.k,
                       radius=case.radius, side=case.side)
    return case, want


def _device_run(case, fill=0xFF):
    """ops.rig_fuse into buffers pre-filled with 0xFF bytes -> the eight outputs on the host"""
    from hn_amd import ops
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    s, v = case.xyz_mm.shape[0], case.mesh.shape[1]
    n = s // case.k
    shapes = dict(rig_xyz=(n, case.k, 21, 3), rig_mesh=(n, case.k, v, 3), rig_hand=(n, case.k), rig_count=(1,), rig_views=(s,),
                  rig_seed=(s,), fused_xyz=(s, 21, 3), fused_mesh=(s, v, 3))
    bufs = {}
    for name in RIG_FIELDS:
        dtype = torch.float32 if name.endswith(("xyz", "mesh")) else torch.int32
        raw = torch.full((int(np.prod(shapes[name])) * 4,), fill, dtype=torch.uint8, device="cuda")
        bufs[name] = raw.view(dtype).view(shapes[name])
    table = torch.from_numpy(ops.rig_extrinsics(case.ext, n)).cuda()
    out = ops.rig_fuse(d(case.xyz_mm), d(case.mesh), d(case.has_hand), d(case.lifted), d(case.score), table, case.k, case.radius,
                       side=None if case.side is None else d(case.side), out=ops.RigFused(**bufs))
    torch.cuda.synchronize()
    for name in RIG_FIELDS:
        assert getattr(out, name).data_ptr() == bufs[name].data_ptr()
    return {name: bufs[name].cpu() for name in RIG_FIELDS}


def _check(got, want, tag):
    for name in RIG_FIELDS:
        w = getattr(want, name)
        w = np.array([w], np.int32) if name == "rig_count" else w
        g = got[name].numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, name, g.shape, w.shape, g.dtype, w.dtype)
        differ = int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).sum())
        print(f"{tag}: {name} {g.shape}: {differ} words differ")
        assert differ == 0, (tag, name, differ)


CASES = [("random", n, k, v, handed) for (n, k, v) in rc.SHAPES for handed in (False, True)] + [
    ("edges", n, k, v, handed) for (n, k, v) in rc.SHAPES[1:] for handed in (False, True)]


@pytest.mark.parametrize("kind,n,k,v,handed", CASES)
def test_op_against_the_rule(kind, n, k, v, handed):
    """ops.rig_fuse at (N, K, V) = (1,1,5), (3,2,5), (4,16,778) and (16,16,7) -- the 256-slot limit --, on seeded rigs (lifted
    slots, has_hand 1 but not lifted, has_hand 2, empty slots; NaN and inf in every invalid row; rig hands of three and more
    cameras) and on the edge scene (the tie, d2 == r2 and the next float above, the side gate on and off, a slot that is not
    lifted): all eight outputs equal rig_ref bit for bit, written into buffers pre-filled with 0xFF bytes; a second run into
    buffers pre-filled with 0x00 gives the same bytes."""
    case, want = _case(kind, n, k, v, handed)
    got = _device_run(case)
    _check(got, want, f"{kind} {n}x{k}x{v} handed={handed}")
    again = _device_run(case, fill=0x00)
    for name in RIG_FIELDS:
        assert _bytes(again[name]) == _bytes(got[name]), name
    if kind == "edges":
        groups = {key: g for key, g in rc.EDGE_GROUPS.items() if key[0] < n}
        if not handed and n >= 4:
            groups[(3, 0)] = 1                                     # (without the gate the hand at B's place joins B)
        for (cam, slot), g in groups.items():
            assert int(got["rig_hand"][cam, slot]) == g, (cam, slot)


def test_a_nan_centre_seeds_alone_on_the_device():
    """a lifted slot whose joints hold a NaN: its centre is NaN, it joins nothing and nothing joins it -- the integer outputs
    equal the rule's exactly; the float outputs too, NaN for NaN (which NaN a sum of NaNs is, is not part of the rule)"""
    case, _want = _case("edges", 4, 16, 778, True)
    xyz = case.xyz_mm.copy()
    xyz[case.k, 3, 2] = np.nan                                     # camera 1, slot 0: the tie's winner
    case = case._replace(xyz_mm=xyz)
    want = rr.rig_fuse(case.xyz_mm, case.mesh, case.has_hand, case.lifted, case.score, rr.table(case.ext), case.k,
                       radius=case.radius, side=case.side)
    got = _device_run(case)
    assert want.rig_hand[1, 0] != 0 and want.rig_hand[1, 1] == 0 and want.rig_views[want.rig_hand[1, 0]] == 1
    for name in ("rig_hand", "rig_views", "rig_seed"):
        assert np.array_equal(got[name].numpy(), getattr(want, name)), name
    assert int(got["rig_count"]) == want.rig_count
    for name in ("rig_xyz", "rig_mesh", "fused_xyz", "fused_mesh"):
        assert np.array_equal(got[name].numpy(), getattr(want, name), equal_nan=True), name
    assert torch.isnan(got["rig_xyz"][1, 0]).any() and torch.isnan(got["fused_xyz"][int(want.rig_hand[1, 0])]).any()


def test_the_op_refuses_bad_arguments():
    from hn_amd import ops
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    i = lambda *shape: z(*shape, dtype=torch.int32)  # noqa: E731
    table = torch.from_numpy(ops.rig_extrinsics(rc.extrinsics(2, seed=1))).cuda()
    good = dict(xyz_mm=z(4, 21, 3), mesh=z(4, 5, 3), has_hand=i(4), lifted=i(4), score=z(4), extrinsics_table=table, k=2)
    assert ops.rig_fuse(**good).rig_count.tolist() == [0]
    for kw in (dict(k=3), dict(extrinsics_table=table[:1].contiguous()), dict(extrinsics_table=table.double()), dict(lifted=i(3)),
               dict(score=z(5)), dict(side=i(2)), dict(mesh=z(3, 5, 3)), dict(radius=0.0), dict(radius=float("nan")),
               dict(xyz_mm=z(17 * 16, 21, 3), mesh=z(17 * 16, 5, 3), k=16)):
        with pytest.raises((ValueError, TypeError)):
            ops.rig_fuse(**{**good, **kw})
    with pytest.raises(TypeError):
        ops.rig_fuse(**{**good, "has_hand": z(4)})


# ------------------------------------------------------------------------------------------------------------ whole steps
@pytest.fixture(scope="module")
def lifter(golden_dir):
    from hn_amd import synth
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from oracle import pose2mesh_ref
    from test_render_gpu import _synthetic_faces
    g = np.load(golden_dir / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    p2m_sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    last = max(int(key.split(".")[2]) for key in p2m_sd if key.startswith("pose2mesh.cl."))
    for key in (f"pose2mesh.cl.{last}.weight", f"pose2mesh.cl.{last}.bias"):
        p2m_sd[key] = p2m_sd[key] * LIFTER_OUTPUT_SCALE
    return Pose2MeshEngine(p2m_sd, graphs, device="cuda"), g["perm_reverse"][:778], _synthetic_faces()


@pytest.fixture(scope="module")
def net(fcos_sd, a2j_sd):
    from test_render_gpu import _net
    return _net(fcos_sd, a2j_sd)


PARAS = (617.343, 617.343, 312.42, 241.42)
IDENTITY = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (2, 1, 1))
APART = IDENTITY.copy()
APART[1, 0, 3] = 1.0                                  # camera 1 stands a metre to the side


@functools.lru_cache(maxsize=None)
def _pair(steps=1):
    """the live tests' synthetic frame, twice: two cameras that see the same picture"""
    from hn_amd import synth
    out = []
    for t in range(steps):
        rgb, depth = synth.make_rgb(1, seed=1000 + 10 * t).cuda(), synth.make_depth(1, seed=2000 + 10 * t).cuda()
        out.append((rgb.repeat(2, 1, 1, 1).contiguous(), depth.repeat(2, 1, 1, 1).contiguous()))
    return out


def _run_steps(eng, inputs):
    """the engine's eager step on every input in turn -> (the reads, a copy of the last host buffer)"""
    if getattr(eng, "track", None) is not None:
        eng.track_reset()
    reads = []
    with torch.inference_mode():
        for rgb, depth in inputs:
            out = eng.forward_device(rgb, depth)
            torch.cuda.synchronize()
            reads.append(out.read())
    return reads, out.host.clone(), out


def _rule(r, ext, k, radius=rr.RIG_RADIUS, smooth=False, handed=False):
    """rig_ref on a step's own read() values"""
    n = r.keypoints.shape[0]
    xyz, mesh = (r.smooth_xyz, r.smooth_mesh) if smooth else (r.xyz_mm, r.mesh)
    return rr.rig_fuse(xyz.numpy().reshape(n * k, 21, 3), mesh.numpy().reshape(n * k, -1, 3), r.has_hand.numpy().reshape(-1),
                       r.lifted.numpy().reshape(-1).astype(np.int32), r.score.numpy().reshape(-1), rr.table(ext), k, radius=radius,
                       side=r.side.numpy().reshape(-1) if handed else None)


def _check_read(r, want, tag):
    for name in RIG_FIELDS:
        g, w = getattr(r, name), getattr(want, name)
        if name == "rig_count":
            print(f"{tag}: rig_count {g} (rule {w})")
            assert type(g) is int and g == w, (tag, g, w)
            continue
        g = g.numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, name)
        differ = int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).sum())
        print(f"{tag}: {name}: {differ} words differ")
        assert differ == 0, (tag, name, differ)


def _same_fields(a, b, names):
    for f in names:
        x, y = getattr(a, f), getattr(b, f)
        assert torch.equal(x, y) if torch.is_tensor(x) else x == y, f


def test_live_step_fuses_the_pair_and_keeps_the_prefix(net, lifter):
    """The same frame as two cameras, max_hands = 2.  Identity extrinsics: every lifted slot of frame 0 is fused with its copy
    (rig_views 2, rig_hand equal across the frames) and all eight read() fields equal rig_ref on the step's own read() values.
    Camera 1 a metre to the side: nothing fuses, rig_count is the number of lifted slots.  The host buffer up to the size of
    the step without extrinsics equals that step's buffer byte for byte; the device views are the read()'s values."""
    lift, perm, _faces = lifter
    inputs = _pair()
    plain_eng = net.live_hands(lift, PARAS, max_hands=2, perm_reverse=perm)
    (plain,), plain_host, _o = _run_steps(plain_eng, inputs)
    eng = net.live_hands(lift, PARAS, max_hands=2, perm_reverse=perm, extrinsics=IDENTITY)
    (r,), host, out = _run_steps(eng, inputs)
    lifted = r.lifted.numpy()
    print(f"lifted {lifted.tolist()}, has_hand {r.has_hand.tolist()}, rig_hand {r.rig_hand.tolist()}, views {r.rig_views.tolist()}")
    assert lifted[0].any() and np.array_equal(lifted[0], lifted[1])
    _check_read(r, _rule(r, IDENTITY, 2), "fused pair")
    assert r.rig_count == int(lifted[0].sum()) and torch.equal(r.rig_hand[0], r.rig_hand[1])
    for kk in range(2):
        g = int(r.rig_hand[0, kk])
        assert (g >= 0) == bool(lifted[0, kk])
        if g >= 0:
            assert int(r.rig_views[g]) == 2 and int(r.rig_seed[g]) == kk
    # the prefix: what the step without the option hands out, where it hands it out
    assert host.numel() == out.layout.nbytes > plain_host.numel() == plain_eng._layout(2).nbytes
    assert torch.equal(host[:plain_host.numel()], plain_host)
    assert type(r)._fields == type(plain)._fields + RIG_FIELDS
    _same_fields(r, plain, type(plain)._fields)
    for name in RIG_FIELDS:
        dev, got = getattr(out, name).cpu(), getattr(r, name)
        assert (int(dev) == got) if name == "rig_count" else torch.equal(dev, got), name
    assert tuple(out.rig_xyz.shape) == (2, 2, 21, 3) and tuple(out.fused_mesh.shape) == (4, 778, 3)
    # a metre apart
    (far,), _h, _o = _run_steps(net.live_hands(lift, PARAS, max_hands=2, perm_reverse=perm, extrinsics=APART), inputs)
    _check_read(far, _rule(far, APART, 2), "separated pair")
    assert far.rig_count == int(far.lifted.sum()) == 2 * r.rig_count and int(far.rig_views.max()) == 1
    assert torch.equal(far.rig_xyz[0], r.rig_xyz[0]) and not torch.equal(far.rig_xyz[1], r.rig_xyz[1])
    _same_fields(far, plain, type(plain)._fields)


def test_capture_and_set_extrinsics(net, lifter):
    """The captured rig step's host buffer equals the eager step's; after set_extrinsics the SAME graph's next replay gives what
    a fresh engine built with the new extrinsics gives; an engine without extrinsics has no set_extrinsics; N + 1 frames raise."""
    lift, perm, _faces = lifter
    (rgb, depth), = _pair()
    make = lambda e: net.live_hands(lift, PARAS, max_hands=2, perm_reverse=perm, extrinsics=e)  # noqa: E731
    eng = make(IDENTITY)
    _reads, eager_host, _o = _run_steps(eng, [(rgb, depth)])
    with torch.inference_mode():
        run, s_img, s_dep, out = eng.graphed(rgb, depth)
        s_img.copy_(rgb)
        s_dep.copy_(depth)
        run()
        torch.cuda.synchronize()
        assert torch.equal(out.host, eager_host)
        fused = out.read()
        graphs, graph, table = len(eng._graphs), next(iter(eng._graphs.values()))[0], eng.extrinsics.data_ptr()
        new = rc.extrinsics(2, seed=12)
        eng.set_extrinsics(new)
        run()
        torch.cuda.synchronize()
        moved, moved_host = out.read(), out.host.clone()
        assert len(eng._graphs) == graphs and next(iter(eng._graphs.values()))[0] is graph and eng.extrinsics.data_ptr() == table
        with pytest.raises(ValueError, match="3 frames"):
            eng.forward_device(torch.cat([rgb, rgb[:1]]), torch.cat([depth, depth[:1]]))
    assert not torch.equal(moved.rig_xyz, fused.rig_xyz) and torch.equal(moved.xyz_mm, fused.xyz_mm)
    _check_read(moved, _rule(moved, new, 2), "after set_extrinsics")
    _reads, fresh_host, _o = _run_steps(make(new), [(rgb, depth)])
    assert torch.equal(moved_host, fresh_host)
    with pytest.raises(ValueError, match="built with extrinsics"):
        net.live_hands(lift, PARAS, max_hands=2, perm_reverse=perm).set_extrinsics(new)


def test_combined_options(net, lifter):
    """track, smooth, faces, occlude and handed with the rig, two steps: the rig outputs equal rig_ref on smooth_xyz and
    smooth_mesh (the side gate on), rig_seed points at slots with a track id, and every other field equals the same step
    without extrinsics."""
    lift, perm, faces = lifter
    inputs = _pair(steps=2)
    opts = dict(max_hands=2, perm_reverse=perm, faces=faces, track=True, smooth=True, occlude=True, handed=True)
    plain, _h, _o = _run_steps(net.live_hands(lift, PARAS, **opts), inputs)
    rig, _h, _o = _run_steps(net.live_hands(lift, PARAS, extrinsics=IDENTITY, **opts), inputs)
    for t in range(2):
        r, p = rig[t], plain[t]
        assert type(r)._fields == type(p)._fields + RIG_FIELDS
        _same_fields(r, p, type(p)._fields)
        _check_read(r, _rule(r, IDENTITY, 2, smooth=True, handed=True), f"combined, step {t}")
        ids = r.track_id.reshape(-1)
        for g in range(r.rig_count):
            assert int(ids[int(r.rig_seed[g])]) != 0
        assert r.rig_count == len({int(g) for g in r.rig_hand.reshape(-1) if g >= 0})
    assert bool(rig[0].lifted.any()) and rig[0].rig_count >= 1
