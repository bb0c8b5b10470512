"""The occluded overlay on the GPU (csrc/mesh_raster.hip with its switch, ops.mesh_render(scene_depth=), the live engines'
occlude=) against the numpy statement of the rule (tests/occlude_ref.py): overlay, silhouette and coverage on the pixels that
are neither depth fights nor threshold pixels, the slot on those that are, and the counters against the GPU's own silhouette
exactly."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import occlude_ref as oc
import raster_ref as rr

pytestmark = pytest.mark.gpu

LIVE_PARAS = (617.343, 617.343, 312.42, 241.42)
AMBIGUOUS_CAP = 0.01            # left-out pixels (depth fights + threshold pixels) per covered pixel: test_render_gpu.py's cap
THRESHOLD_CAP = 0.001           # threshold pixels alone
BOTH_KINDS = 100                # every scene has at least this many hidden and this many shown pixels


# ------------------------------------------------------------------------------------------------------------ op level
def _scenes():
    """name -> (meshes [K,V,3] of ONE frame, faces, paras, (h, w), (centre Z, half depth) of the mesh nearest the middle)"""
    big = rr.scenes()
    out = {}
    m, f, _l, paras, hw = big["partly outside the frame"]          # 203 x 301: no multiples of the tile, two borders crossed
    out["203x301 partly outside"] = (m[0], f, paras, hw, (0.5, 0.04))
    small, fs = rr.ellipsoid((0.004, -0.002, 0.5), (0.035, 0.03, 0.02), rings=9, segs=11)
    out["48x64"] = (small[None], fs, (300.0, 300.0, 32.0, 24.0), (48, 64), (0.5, 0.02))
    m, f, _l, paras, hw = big["two interpenetrating ellipsoids"]
    out["480x640 two slots"] = (m[0], f, paras, hw, (0.55, 0.04))
    return out


SCENES = _scenes()
MAPS = ("plane", "noise", "holes", "constant at a face's Z")


@functools.lru_cache(maxsize=None)
def _raster(name):
    """The scene's raster and colours, worked out once and shared (nothing changes them)."""
    meshes, faces, paras, (h, w), _z = SCENES[name]
    return rr.rasterize(meshes, faces, paras, h, w)


def _depth_map(name, kind):
    """(depth fp32 [h,w], margin) of a scene: the maps where the rule can go wrong"""
    _m, _f, _p, (h, w), (zc, dz) = SCENES[name]
    ras, _c = _raster(name)
    rng = np.random.default_rng(len(name) * 7 + len(kind))
    cols = np.arange(w, dtype=np.float32)[None, :].repeat(h, 0)
    covered = ras.face >= 0
    if kind == "plane":        # tilted across the width, cutting through the mesh: over the covered columns D + margin runs from
        cc = np.nonzero(covered.any(axis=0))[0]                # the nearest to the farthest of the drawn depths
        lo, hi = float(ras.z1[covered].min()), float(ras.z1[covered].max())
        step = np.float32((hi - lo) / max(1, cc[-1] - cc[0]))
        return (np.float32(lo - 0.01) + step * (cols - np.float32(cc[0]))).astype(np.float32), 0.01
    if kind == "noise":
        return rng.uniform(zc - 3 * dz, zc + 2 * dz, (h, w)).astype(np.float32), 0.03
    if kind == "holes":        # a map that hides the whole mesh, with holes of every kind over it
        d = np.full((h, w), zc - 4 * dz, np.float32)
        pick = rng.integers(0, 8, (h, w))
        for value, bad in ((1, 0.0), (2, np.nan), (3, np.inf), (4, -0.25)):
            d[pick == value] = bad
        return d, 0.03
    # a constant map exactly at the fp32 Z the kernel's nearest face has somewhere in the middle of the mesh, margin 0
    rows, cs = np.nonzero(covered)
    i = len(rows) // 2
    return np.full((h, w), np.float32(ras.z1[rows[i], cs[i]]), np.float32), 0.0


def _gpu(meshes, faces, paras, frame, depth, margin, lifted=None, scratch=None, coverage=None, silhouette=None, zout=False):
    """one frame (or N) through ops.mesh_render(scene_depth=) -> numpy (overlay, silhouette, coverage[, mesh Z])"""
    from hn_amd import ops
    m = torch.from_numpy(np.ascontiguousarray(meshes)).cuda()
    k = m.shape[-3] if m.dim() == 4 else m.shape[0]
    fr = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
    d = torch.from_numpy(np.ascontiguousarray(depth)).cuda()
    lf = None if lifted is None else torch.from_numpy(np.asarray(lifted, np.int32).reshape(-1)).cuda()
    z = torch.full(tuple(fr.shape[:3] if fr.dtype == torch.uint8 else (fr.shape[0],) + tuple(fr.shape[2:])), -1.0,
                   device="cuda") if zout else None
    img, sil, cov = ops.mesh_render(m, faces, paras, fr, lifted=lf, k=k, scratch=scratch, depth_out=z, scene_depth=d,
                                    margin=margin, silhouette_out=silhouette, coverage_out=coverage)
    torch.cuda.synchronize()
    res = (img.cpu().numpy(), sil.cpu().numpy(), cov.cpu().numpy())
    return res + (z.cpu().numpy(),) if zout else res


def _compare(tag, got_img, got_sil, got_cov, want, frame, slots, fights_cap=AMBIGUOUS_CAP):
    """One frame against the helper.  Returns (covered, hidden, left out) pixel counts.  fights_cap: the largest share of
    left-out pixels among the covered ones -- the op-level scenes are chosen to stay within it; None for the live steps'
    synthetic mesh, a triangle soup whose faces cross one another (tests/test_render_gpu.py's _check_overlay caps nothing
    there either): its depth fights are compared like everyone's, against the nearest and the second-nearest face.  Threshold
    pixels are capped in both."""
    f8 = rr.frame_u8(frame)
    out = want.fights | want.threshold
    clear = ~out
    n_cov, n_out, n_thr = int(want.covered.sum()), int((want.covered & out).sum()), int(want.threshold.sum())
    shown = want.covered & ~want.hidden
    lev = int(np.abs(got_img[clear & shown].astype(np.int64) - want.image[clear & shown].astype(np.int64)).max()) \
        if (clear & shown).any() else 0
    mine = oc.count(got_sil, slots)
    print(f"{tag}: covered {n_cov}, hidden {int(want.hidden.sum())}, depth fights {int(want.fights.sum())}, threshold pixels "
          f"{n_thr}, left out {n_out} ({n_out / max(1, n_cov):.3%}), colour max diff {lev}, coverage {got_cov.tolist()} "
          f"(helper {want.coverage.tolist()})")
    assert fights_cap is None or n_out <= fights_cap * n_cov, f"{tag}: too many pixels left out"
    assert n_thr <= THRESHOLD_CAP * n_cov, f"{tag}: too many threshold pixels"
    assert np.array_equal(got_sil[clear], want.silhouette[clear]), \
        f"{tag}: silhouette differs on {int((got_sil[clear] != want.silhouette[clear]).sum())} clear pixels"
    assert lev <= 1, f"{tag}: colour off by {lev} levels"
    not_drawn = clear & ~shown                   # uncovered, or hidden: the frame's own bytes, exactly
    assert np.array_equal(got_img[not_drawn], f8[not_drawn]), f"{tag}: a hidden or uncovered pixel is not the frame's"
    # the left-out pixels: covered all the same (coverage is exact), by the nearest or the second-nearest face's slot, and
    # drawn accordingly
    who = (got_sil[out].astype(np.int64) & 0x7F) - 1
    assert np.array_equal(got_sil[out] != 0, want.covered[out])
    assert (((who == want.slot[out]) | ((who == want.slot2[out]) & (want.slot2[out] >= 0))) | ~want.covered[out]).all(), tag
    flagged = (got_sil & oc.HIDDEN) != 0
    assert np.array_equal(got_img[flagged], f8[flagged]), f"{tag}: a pixel flagged hidden is not the frame's"
    assert np.array_equal(got_cov, mine), f"{tag}: coverage {got_cov.tolist()} but the silhouette counts {mine.tolist()}"
    assert int(np.abs(got_cov.astype(np.int64) - want.coverage).max()) <= n_out, f"{tag}: coverage off the helper's by more than the left-out pixels"
    return n_cov, int(want.hidden.sum()), n_out


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_matches_the_rule(name, kind):
    """Overlay within one colour level, silhouette equal and hidden pixels the frame's own bytes on every pixel that is neither
    a depth fight nor a threshold pixel; on those, the silhouette's slot is the nearest or the second-nearest face's; they are
    at most 1 % (threshold pixels alone: 0.1 %) of the covered pixels; coverage equals the counts of the GPU's own silhouette
    exactly and the helper's within the left-out pixels; at least 100 pixels hidden and 100 shown; two runs bit-identical; bgr8
    and fp32 frames, and an RGBD-shaped depth tensor, give the same three outputs."""
    meshes, faces, paras, (h, w), _z = SCENES[name]
    k = meshes.shape[0]
    depth, margin = _depth_map(name, kind)
    bgr = rr.frame_bgr8(1, h, w, seed=len(name) + len(kind))
    ras, colours = _raster(name)
    want = oc.occlude(ras, colours, bgr[0], depth, margin, k, len(faces))
    img, sil, cov = _gpu(meshes[None], faces, paras, bgr, depth[None, None], margin)
    assert img.shape == (1, h, w, 3) and sil.shape == (1, h, w) and sil.dtype == np.uint8 and cov.shape == (k, 2)
    n_cov, n_hidden, _out = _compare(f"{name} / {kind}", img[0], sil[0], cov, want, bgr[0], k)
    assert n_hidden >= BOTH_KINDS and n_cov - n_hidden >= BOTH_KINDS, f"{name} / {kind}: hidden {n_hidden} of {n_cov}"
    again = _gpu(meshes[None], faces, paras, bgr, depth[None, None], margin)
    assert all(np.array_equal(a, b) for a, b in zip(again, (img, sil, cov)))                     # two runs: bit-identical
    f32 = np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))
    as_f32 = _gpu(meshes[None], faces, paras, f32, depth[None], margin)                          # ([N,H,W] depth as well)
    assert all(np.array_equal(a, b) for a, b in zip(as_f32, (img, sil, cov)))
    rgbd = np.concatenate([f32, depth[None, None]], axis=1)
    rgbd[:, :3] += 5.0                                                    # (only channel 3 may be read)
    as_rgbd = _gpu(meshes[None], faces, paras, bgr, rgbd, margin)
    assert all(np.array_equal(a, b) for a, b in zip(as_rgbd, (img, sil, cov)))


def test_a_margin_that_hides_nothing_is_the_plain_overlay():
    """margin = +1e3 reproduces ops.mesh_render without scene_depth bit for bit (image and mesh Z), and no silhouette byte has
    its flag set; margin = -1e3 leaves the frame on every covered pixel whose depth is valid; the mesh Z does not depend on the
    margin."""
    from hn_amd import ops
    name = "203x301 partly outside"
    meshes, faces, paras, (h, w), _z = SCENES[name]
    depth, _m = _depth_map(name, "holes")
    bgr = rr.frame_bgr8(1, h, w, seed=3)
    m, fr = torch.from_numpy(meshes).cuda(), torch.from_numpy(bgr).cuda()
    z = torch.full((1, h, w), -1.0, device="cuda")
    plain = ops.mesh_render(m, faces, paras, fr, k=2, depth_out=z)
    img, sil, cov, z2 = _gpu(meshes[None], faces, paras, bgr, depth[None, None], 1e3, zout=True)
    assert np.array_equal(img, plain.cpu().numpy()) and np.array_equal(z2, z.cpu().numpy())
    assert not (sil & oc.HIDDEN).any() and np.array_equal(sil != 0, z2 > 0) and (cov[:, 0] == cov[:, 1]).all()
    img, sil, cov, z3 = _gpu(meshes[None], faces, paras, bgr, depth[None, None], -1e3, zout=True)
    hide = (z2[0] > 0) & oc.valid_depth(depth)
    assert hide.sum() >= BOTH_KINDS and ((z2[0] > 0) & ~hide).sum() >= BOTH_KINDS
    assert np.array_equal((sil[0] & oc.HIDDEN) != 0, hide) and np.array_equal(img[0][hide], rr.frame_u8(bgr[0])[hide])
    assert np.array_equal(img[0][~hide], plain.cpu().numpy()[0][~hide]) and np.array_equal(z3, z2)


def test_slots_that_are_not_lifted_count_nothing():
    """Two frames of two slots into a scratch, a silhouette and counters that a full run has just filled: with lifted = 0
    everywhere the overlay is the frame, the silhouette and the counters are zero; with one slot lifted per frame the other
    slot's counters are (0, 0) and the silhouette holds the lifted slot's id alone."""
    from hn_amd import ops
    meshes, faces, paras, (h, w), (zc, dz) = SCENES["480x640 two slots"]
    two = np.stack([meshes, meshes[::-1]])
    bgr = rr.frame_bgr8(2, h, w, seed=8)
    depth = np.random.default_rng(2).uniform(zc - 3 * dz, zc + 2 * dz, (2, 1, h, w)).astype(np.float32)
    scratch = torch.empty((ops.mesh_render_scratch_bytes(4, faces.shape[0]),), dtype=torch.uint8, device="cuda")
    cov_t = torch.full((4, 2), -7, dtype=torch.int32, device="cuda")
    sil_t = torch.full((2, h, w), 9, dtype=torch.uint8, device="cuda")
    full = _gpu(two, faces, paras, bgr, depth, 0.03, np.ones(4), scratch, cov_t, sil_t)
    assert (full[2][:, 0] > 5000).all() and (full[2][:, 1] >= BOTH_KINDS).all() and (full[2][:, 0] - full[2][:, 1] >= BOTH_KINDS).all()
    assert np.array_equal(np.concatenate([oc.count(full[1][i], 2) for i in range(2)]), full[2])
    none = _gpu(two, faces, paras, bgr, depth, 0.03, np.zeros(4), scratch, cov_t, sil_t)
    assert np.array_equal(none[0], np.stack([rr.frame_u8(b) for b in bgr])) and not none[1].any() and not none[2].any()
    full = _gpu(two, faces, paras, bgr, depth, 0.03, np.ones(4), scratch, cov_t, sil_t)
    some = _gpu(two, faces, paras, bgr, depth, 0.03, np.array([1, 0, 0, 1]), scratch, cov_t, sil_t)
    assert (some[2][[1, 2]] == 0).all() and (some[2][[0, 3], 0] > 5000).all()
    assert set(np.unique(some[1][0] & 0x7F).tolist()) == {0, 1} and set(np.unique(some[1][1] & 0x7F).tolist()) == {0, 2}
    assert np.array_equal(np.concatenate([oc.count(some[1][i], 2) for i in range(2)]), some[2])
    # the slot drawn alone covers at least what it won against the other one
    assert (some[2][[0, 3], 0] >= full[2][[0, 3], 0]).all()


def test_python_layer_refusals_on_the_gpu():
    from hn_amd import ops
    meshes, faces, paras, (h, w), _z = SCENES["48x64"]
    m, fr = torch.from_numpy(meshes).cuda(), torch.from_numpy(rr.frame_bgr8(1, h, w, 1)).cuda()
    d = torch.ones((1, 1, h, w), device="cuda")
    with pytest.raises(ValueError, match="scene_depth"):
        ops.mesh_render(m, faces, paras, fr, scene_depth=torch.ones((1, 1, h, w + 1), device="cuda"))
    with pytest.raises(ValueError, match="scene_depth"):
        ops.mesh_render(m, faces, paras, fr, scene_depth=torch.ones((1, 2, h, w), device="cuda"))
    with pytest.raises(TypeError, match="scene_depth"):
        ops.mesh_render(m, faces, paras, fr, scene_depth=d.double())
    with pytest.raises(RuntimeError, match="scene_depth"):
        ops.mesh_render(m, faces, paras, fr, scene_depth=d.cpu())
    with pytest.raises(ValueError, match="occlude_margin"):
        ops.mesh_render(m, faces, paras, fr, scene_depth=d, margin=float("nan"))
    with pytest.raises(ValueError, match="silhouette_out"):
        ops.mesh_render(m, faces, paras, fr, scene_depth=d, silhouette_out=torch.zeros((1, h, w + 1), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="coverage_out"):
        ops.mesh_render(m, faces, paras, fr, scene_depth=d, coverage_out=torch.zeros((2, 2), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="give scene_depth"):
        ops.mesh_render(m, faces, paras, fr, coverage_out=torch.zeros((1, 2), dtype=torch.int32, device="cuda"))


def test_c_abi_on_raw_pointers():
    """hn_mesh_render_occluded_u8 through ctypes on raw device pointers (an RGBD tensor's channel 3 by address and stride)
    equals ops.mesh_render(scene_depth=); a refused call launches nothing; out_coverage may be NULL."""
    from hn_amd import _lib, ops
    lib = _lib.load()
    meshes, f, paras_t, (h, w), (zc, dz) = SCENES["203x301 partly outside"]
    mesh, faces = torch.from_numpy(meshes).cuda(), torch.from_numpy(f).cuda()
    bgr = torch.from_numpy(rr.frame_bgr8(1, h, w, seed=9)).cuda()
    rgbd = torch.rand((1, 4, h, w), generator=torch.Generator().manual_seed(4)).cuda()
    rgbd[:, 3] = zc - 3 * dz + 5 * dz * rgbd[:, 3]
    want = ops.mesh_render(mesh, faces, paras_t, bgr, k=2, scene_depth=rgbd, margin=0.02)
    need = lib.hn_mesh_render_scratch_bytes(2, f.shape[0])
    scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
    out = torch.full((1, h, w, 3), 7, dtype=torch.uint8, device="cuda")
    sil = torch.full((1, h, w), 7, dtype=torch.uint8, device="cuda")
    cov = torch.full((2, 2), 7, dtype=torch.int32, device="cuda")
    paras = (C.c_float * 4)(*paras_t)
    stream = torch.cuda.current_stream().cuda_stream

    def call(stride=4 * h * w, sil_p=sil.data_ptr(), cov_p=cov.data_ptr()):
        return lib.hn_mesh_render_occluded_u8(mesh.data_ptr(), faces.data_ptr(), None, None, 2, 777, f.shape[0], 2, paras,
                                              bgr.data_ptr(), _lib.FRAME_U8_BGR_HWC, h, w, rgbd.data_ptr() + 3 * h * w * 4, stride,
                                              0.02, scratch.data_ptr(), need, out.data_ptr(), None, sil_p, cov_p, stream)
    assert call(stride=h * w - 1) == 1 and b"depth_frame_stride" in lib.hn_last_error()
    assert call(sil_p=None) == 1 and b"out_silhouette" in lib.hn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((sil == 7).all()) and bool((cov == 7).all())          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want[0]) and torch.equal(sil, want[1]) and torch.equal(cov, want[2])
    assert int(cov[:, 1].min()) >= BOTH_KINDS and int((cov[:, 0] - cov[:, 1]).min()) >= BOTH_KINDS
    out.fill_(7); sil.fill_(7); cov.fill_(7)
    assert call(cov_p=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want[0]) and torch.equal(sil, want[1]) and bool((cov == 7).all())


# ---------------------------------------------------------------------------------------------------- the live engines
H, W = 480, 640
# (the recipe of tests/test_render_gpu.py: the seeded lifter's last graph convolution scaled by 0.01, so that the mesh is
# hand-sized and projects into the frame; a lifted frame then draws at least DRAWN_FLOOR pixels)
DRAWN_FLOOR = 1000
LIFTER_OUTPUT_SCALE = 0.01


def _synthetic_faces(seed=7, nv=778):
    from scipy.spatial import Delaunay
    pts = np.random.default_rng(seed).random((nv, 2))
    return Delaunay(pts).simplices.astype(np.int64)


@pytest.fixture(scope="module")
def parts(golden_dir, fcos_sd, a2j_sd):
    from hn_amd import synth
    from hn_amd.a2j_engine import A2JEngine
    from hn_amd.fcos_engine import FCOSEngine
    from hn_amd.pipeline import HandNetEngine
    from hn_amd.pose2mesh_engine import Pose2MeshEngine
    from oracle import pose2mesh_ref
    g = np.load(golden_dir / "pose2mesh_forward.npz")
    graphs = pose2mesh_ref.load_graphs(g)
    p2m_sd = synth.make_pose2mesh_state_dict(seed=int(g["weight_seed"]), graph_sizes=[m.shape[0] for m in graphs])
    last = max(int(key.split(".")[2]) for key in p2m_sd if key.startswith("pose2mesh.cl."))
    for key in (f"pose2mesh.cl.{last}.weight", f"pose2mesh.cl.{last}.bias"):
        p2m_sd[key] = p2m_sd[key] * LIFTER_OUTPUT_SCALE
    hand = HandNetEngine(FCOSEngine(fcos_sd, 3, device="cuda"), A2JEngine(a2j_sd, device="cuda"), 3)
    lifter = Pose2MeshEngine(p2m_sd, graphs, device="cuda")
    return hand, lifter, g["perm_reverse"][:778], _synthetic_faces()


@pytest.fixture(scope="module")
def inputs():
    from hn_amd import synth
    return synth.make_rgb(2, seed=1000).cuda(), synth.make_depth(2, seed=2000).cuda()     # depth: per-pixel noise, 0.3-1.5 m


def _run(eng, rgb, depth, graphed=False):
    if graphed:
        run, s_img, s_dep, out = eng.graphed(rgb, depth)
        s_img.copy_(rgb)
        s_dep.copy_(depth)
        run()
    else:
        out = eng.forward_device(rgb, depth)
    torch.cuda.synchronize()
    return out, out.read()


def _same(a, b, fields, tag=""):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        if torch.is_tensor(x):      # (bit for bit, NaN included)
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (tag, f)
        elif isinstance(x, (list, tuple)) and x and torch.is_tensor(x[0]):
            assert all(torch.equal(p, q) for p, q in zip(x, y)), (tag, f)
        else:
            assert x == y, (tag, f)


def _check_step(tag, r, mesh, lifted, frames, depth, faces, margin=0.03, both=True):
    """read().overlay / .silhouette / .coverage against the helper applied to the mesh the step drew, its lifted flags, the
    input frames and the input depth, frame by frame.  Returns the (covered, hidden) pixel counts per frame."""
    n, k = lifted.shape
    cov = r.coverage.numpy().reshape(n, k, 2)
    seen = []
    for i in range(n):
        want = oc.render(mesh[i], faces, LIVE_PARAS, frames[i], depth[i], margin, lifted[i])
        n_cov, n_hidden, _o = _compare(f"{tag}: frame {i}", r.overlay[i].numpy(), r.silhouette[i].numpy(), cov[i], want, frames[i], k,
                                       fights_cap=None)
        if lifted[i].any():
            assert n_cov >= DRAWN_FLOOR, f"{tag}: frame {i}: only {n_cov} pixels drawn"
            if both:       # the synthetic depth is noise in 0.3-1.5 m: the default margin gives both kinds of pixel
                assert n_hidden >= BOTH_KINDS and n_cov - n_hidden >= BOTH_KINDS, (tag, i, n_cov, n_hidden)
        else:
            assert n_cov == 0 and not cov[i].any()
        seen.append((n_cov, n_hidden))
    return seen


def _net(fcos_sd, a2j_sd):
    import types
    from handnet_pipeline.handnet_pipeline import HandNet
    net = HandNet(types.SimpleNamespace(pretrained_fcos="-", pretrained_a2j="-"), num_classes=3)
    net.detector.load_state_dict(fcos_sd, strict=False)
    net.a2j.load_state_dict(a2j_sd, strict=False)
    return net.cuda().eval()


def test_live_steps_end_to_end(parts, inputs, fcos_sd, a2j_sd):
    """live_hands(max_hands=2, faces=, occlude=True), live and live_hands(max_hands=1) on the synthetic pipeline: overlay,
    silhouette and coverage equal the helper applied to read().mesh, .lifted, the input frame and the input depth, with hidden
    and shown pixels in every frame; every field that exists without the option is bit for bit what the same engine without
    occlude returns (the overlay excepted, which the option changes); margin +1e3 gives that engine's overlay bit for bit and
    margin -1e3 leaves the frame on every covered pixel (the synthetic depth is valid everywhere); the device tensors are on
    the output object."""
    _hand, lifter, perm, faces = parts
    rgb, depth = inputs
    net = _net(fcos_sd, a2j_sd)
    frames, dmap = rgb.cpu().numpy(), depth.cpu().numpy()[:, 0]
    kw = dict(perm_reverse=perm, faces=faces)
    with torch.inference_mode():
        out, r = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, occlude=True, **kw), rgb, depth)
        _o, plain = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, **kw), rgb, depth)
        _o, none = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, occlude=True, occlude_margin=1e3, **kw), rgb, depth)
        _o, every = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=2, occlude=True, occlude_margin=-1e3, **kw), rgb, depth)
    assert r._fields == plain._fields + ("silhouette", "coverage") and "silhouette" not in plain._fields
    assert _o.silhouette is not None and tuple(r.silhouette.shape) == (2, H, W) and tuple(r.coverage.shape) == (2, 2, 2)
    assert r.silhouette.dtype == torch.uint8 and r.coverage.dtype == torch.int32
    assert torch.equal(out.overlay.cpu(), r.overlay) and torch.equal(out.silhouette.cpu(), r.silhouette)
    assert torch.equal(out.coverage.cpu(), r.coverage)
    _same(plain, r, [f for f in plain._fields if f != "overlay"], "K = 2")
    assert bool(r.lifted[:, 0].all())
    _check_step("live_hands K = 2", r, r.mesh.numpy(), r.lifted.numpy(), frames, dmap, faces)
    assert not torch.equal(r.overlay, plain.overlay)
    _same(plain, none, plain._fields, "margin +1e3")
    assert not bool((none.silhouette & 0x80).any()) and torch.equal(none.coverage[..., 0], none.coverage[..., 1])
    assert torch.equal(none.coverage[..., 0], r.coverage[..., 0]) and torch.equal(none.silhouette, r.silhouette & 0x7F)
    on = every.silhouette != 0
    assert torch.equal(on, r.silhouette != 0) and bool(((every.silhouette & 0x80) != 0)[on].all()) and not bool(every.coverage[..., 1].any())
    f8 = torch.from_numpy(np.stack([rr.frame_u8(f) for f in frames]))
    assert torch.equal(every.overlay, f8)
    with torch.inference_mode():
        o1, one = _run(net.live(lifter, LIVE_PARAS, occlude=True, **kw), rgb, depth)
        _o, one_plain = _run(net.live(lifter, LIVE_PARAS, **kw), rgb, depth)
        _o, k1 = _run(net.live_hands(lifter, LIVE_PARAS, max_hands=1, occlude=True, **kw), rgb, depth)
    assert len(one) == 9 and one._fields == one_plain._fields + ("silhouette", "coverage") and tuple(one.coverage.shape) == (2, 2)
    assert torch.equal(o1.coverage.cpu(), one.coverage) and torch.equal(o1.silhouette.cpu(), one.silhouette)
    _same(one_plain, one, [f for f in one_plain._fields if f != "overlay"], "live")
    _check_step("live", one, one.mesh.numpy()[:, None], (one.has_hand.numpy() != 0)[:, None], frames, dmap, faces)
    assert tuple(k1.coverage.shape) == (2, 1, 2)
    assert torch.equal(one.overlay, k1.overlay) and torch.equal(one.silhouette, k1.silhouette)
    assert torch.equal(one.coverage, k1.coverage[:, 0])
    assert not torch.equal(one.silhouette, r.silhouette)          # one hand is not two


def test_graph_replay_raw_feeds_and_holes(parts):
    """One engine, one frame: the captured step equals the eager one; forward_raw with 16UC1 (millimetres) equals the fp32
    feed of the same data.  Then holes are cut into the depth map where the mesh is hidden: as zeros through 16UC1 and as NaN
    through 32FC1 each equals the fp32 feed of the same data, no hole hides the mesh, and overlay, silhouette and coverage
    follow the helper applied to the mesh that comes back."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, occlude=True)
    rng = np.random.default_rng(23)
    bgr = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
    mm = rng.integers(300, 1500, size=(1, H, W)).astype(np.uint16)
    rgb = torch.from_numpy(np.ascontiguousarray(bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / 255.0).cuda()
    metres = mm.astype(np.float32) / np.float32(1000.0)
    _o, e = _run(eng, rgb, torch.from_numpy(metres).unsqueeze(1).cuda())
    _o, g = _run(eng, rgb, torch.from_numpy(metres).unsqueeze(1).cuda(), graphed=True)
    raw = eng.forward_raw(torch.from_numpy(bgr), torch.from_numpy(mm))
    torch.cuda.synchronize()
    _same(e, g, e._fields, "graph replay")
    _same(e, raw.read(), e._fields, "16UC1")
    (n_cov, n_hidden), = _check_step("replay", g, g.mesh.numpy(), g.lifted.numpy(), rgb.cpu().numpy(), metres, faces)
    # holes, cut where the mesh is hidden.  Zeros (16UC1) go anywhere: the pose network reads a zero like any other depth, so
    # the mesh may move, and the helper is applied to the mesh that comes back.  NaN (32FC1) would spread through the pose
    # network's convolutions, so those holes keep 8 px away from every crop box of the frame -- the crop is all the networks see
    # of the depth map -- and where the mesh has no hidden pixel out there, they lie on the hidden pixels' rows outside the boxes.
    sil = g.silhouette[0].numpy()
    hidden = (sil & 0x80) != 0
    far = np.ones((H, W), bool)
    for x1, y1, x2, y2 in g.crop_box[0].numpy().reshape(-1, 4).tolist():
        far[max(0, int(y1) - 8):int(y2) + 8, max(0, int(x1) - 8):int(x2) + 8] = False
    outside = far & hidden if (far & hidden).any() else far & hidden.any(axis=1)[:, None]
    print(f"holes: {int(hidden.sum())} hidden pixels, {int((far & hidden).sum())} of them outside the crop boxes "
          f"{g.crop_box[0].tolist()}; NaN holes {int(outside.sum())}")
    assert hidden.any()
    mm_h, nan_h = mm.copy(), metres.copy()
    mm_h[0][hidden], nan_h[0][outside] = 0, np.nan
    zero_h = mm_h.astype(np.float32) / np.float32(1000.0)
    for tag, raw_depth, fp32, holes in (("16UC1 zeros", mm_h, zero_h, hidden), ("32FC1 NaN", nan_h, nan_h, outside)):
        _o, want = _run(eng, rgb, torch.from_numpy(fp32).unsqueeze(1).cuda())
        got = eng.forward_raw(torch.from_numpy(bgr), torch.from_numpy(raw_depth))
        torch.cuda.synchronize()
        got = got.read()
        _same(want, got, want._fields, tag)
        s = got.silhouette[0].numpy()
        assert not (s[holes] & 0x80).any(), f"{tag}: a hole hides the mesh"
        _check_step(tag, got, got.mesh.numpy(), got.lifted.numpy(), rgb.cpu().numpy(), fp32, faces, both=False)


def test_left_is_the_plain_step_on_mirrored_inputs(parts, inputs):
    """left=True: overlay, silhouette and coverage -- all in the mirrored frame -- equal the plain occluded step on frames and
    depth flipped along the width."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs[0][:1], inputs[1][:1]
    _o, left = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, left=True, occlude=True), rgb, depth)
    _o, want = _run(LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, occlude=True),
                    rgb.flip(3).contiguous(), depth.flip(3).contiguous())
    _same(want, left, want._fields, "left")
    assert int(left.coverage[..., 0].sum()) >= DRAWN_FLOOR and int((left.coverage[..., 0] - left.coverage[..., 1]).sum()) >= BOTH_KINDS


def test_a_smoothed_step_tests_the_mesh_it_draws(parts, inputs):
    """track=True, smooth=True: the step draws smooth_mesh, and it is smooth_mesh that is tested against the depth map -- on
    the second step, where the filter's output is no longer the raw mesh."""
    from hn_amd.live import LiveHandsEngine
    hand, lifter, perm, faces = parts
    rgb, depth = inputs
    eng = LiveHandsEngine(hand, lifter, LIVE_PARAS, 2, True, perm, faces=faces, track=True, smooth=True, occlude=True)
    eng.track_reset()
    _run(eng, rgb[:1], depth[:1])
    nearer = (depth[:1] * 0.97).contiguous()      # (the same colour frame: the detector, and so the tracks, stay; the hands move)
    _o, r = _run(eng, rgb[:1], nearer)
    assert r._fields[-4:] == ("smooth_xyz", "smooth_mesh", "silhouette", "coverage")
    assert bool(r.lifted.any()) and not torch.equal(r.smooth_mesh, r.mesh)
    _check_step("smoothed", r, r.smooth_mesh.numpy(), r.lifted.numpy(), rgb[:1].cpu().numpy(), nearer.cpu().numpy()[:, 0], faces,
                both=False)
    assert int(r.coverage[..., 0].sum()) >= DRAWN_FLOOR
    eng.track_reset()
