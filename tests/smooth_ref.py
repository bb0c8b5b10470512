"""The smoothed live step's filter (smooth=) restated in numpy: a One Euro filter (Casiez et al. 2012) per
coordinate, in float32 with one rounding per operation and the operations in the order the kernel's contract gives
(include/handnet_hip.h, hn_mesh_finish_smooth_f32), so that the device's words can be compared bit for bit; `dtype=np.float64`
gives the same formulas in double precision (the twin the fp32 arithmetic is bounded against).

State: one record of four int32 words per element -- {xh, dxh as fp32 bits, track id, 0}; all zeros is the empty filter."""
import numpy as np

TWO_PI = np.float32(6.2831855)
WORDS = 4


def empty_state(slots, joints, v):
    return np.zeros((slots, joints + v, 3, WORDS), np.int32)


def one_euro(x, xp, dxp, dt, min_cutoff, beta, d_cutoff, dtype=np.float32):
    """One filter step on arrays (or scalars): the value x, the previous filtered value xp and derivative dxp -> (xh, edx).
    Every operand is converted to `dtype` first (float64: from its float32 value); one numpy operation per line of the rule."""
    f = dtype
    x, xp, dxp = (np.asarray(a, np.float32).astype(f) for a in (x, xp, dxp))
    dt, min_cutoff, beta, d_cutoff, two_pi, one = (f(np.float32(a)) for a in (dt, min_cutoff, beta, d_cutoff, TWO_PI, 1))
    with np.errstate(all="ignore"):
        rd = (two_pi * d_cutoff) * dt
        ad = rd / (rd + one)
        dx = (x - xp) / dt
        edx = dxp + ad * (dx - dxp)
        fc = min_cutoff + beta * np.abs(edx)
        r = (two_pi * fc) * dt
        a = r / (r + one)
        xh = xp + a * (x - xp)
    return xh, edx


def step(state, x, gate, tid, dt, min_cutoff, beta, d_cutoff):
    """The rule on one block of elements.  state int32 [..., 4] (not changed), x float32 [...], gate bool and tid int32
    broadcastable to x -> (output float32 [...], the new state)."""
    x = np.asarray(x, np.float32)
    gate = np.broadcast_to(np.asarray(gate, bool), x.shape)
    tid = np.broadcast_to(np.asarray(tid, np.int32), x.shape)
    sxh, sdx = state[..., 0].copy().view(np.float32), state[..., 1].copy().view(np.float32)
    sid = state[..., 2]
    xh, edx = one_euro(x, sxh, sdx, dt, min_cutoff, beta, d_cutoff)
    finite_x = np.isfinite(x)
    init = (sid == 0) | (sid != tid) | (tid == 0) | ~np.isfinite(sxh) | ~np.isfinite(sdx)
    live = gate & finite_x                              # rules 3 and 4: the record is kept
    out = np.where(gate, np.where(finite_x & ~init, xh, x), np.float32(0)).astype(np.float32)      # rule 1: 0; rule 2: x
    new = np.zeros_like(state)
    new[..., 0] = np.where(live, np.where(init, x, xh), np.float32(0)).astype(np.float32).view(np.int32)
    new[..., 1] = np.where(live & ~init, edx, np.float32(0)).astype(np.float32).view(np.int32)
    new[..., 2] = np.where(live, tid, 0)
    return out, new


def step_slots(state, xyz_mm, mesh, has_hand, lifted, track_id, dt, min_cutoff=1.0, beta=0.007, d_cutoff=1.0):
    """One step of every slot: state [slots, J + V, 3, 4], xyz_mm [slots, J, 3] (gate: has_hand == 1), mesh [slots, V, 3] -- the
    final mesh, zeros where not lifted -- (gate: lifted == 1), track_id [slots] -> (smooth_xyz, smooth_mesh, the new state).
    The vertices' beta is float32(1000 * beta): beta is stated for mm/s, the mesh is in metres."""
    j = xyz_mm.shape[1]
    tid = np.asarray(track_id, np.int32).reshape(-1, 1, 1)
    g_xyz = (np.asarray(has_hand).reshape(-1, 1, 1) == 1)
    g_mesh = (np.asarray(lifted).reshape(-1, 1, 1) == 1)
    x_xyz = np.where(g_xyz, np.asarray(xyz_mm, np.float32), np.float32(0)).astype(np.float32)
    sx, new_j = step(state[:, :j], x_xyz, g_xyz, tid, dt, min_cutoff, beta, d_cutoff)
    sm, new_v = step(state[:, j:], np.asarray(mesh, np.float32), g_mesh, tid, dt, min_cutoff, np.float32(beta * 1000.0), d_cutoff)
    return sx, sm, np.concatenate([new_j, new_v], axis=1)
