"""The definition of slam2d_search_points and slam2d_refine_points (include/slam2d.h) in NumPy, for the tests: the valid points, the
rotated offsets ``(c qx) - (s qy)``, ``(s qx) + (c qy)`` of a heading, tests/score_yardstick.py's cell step (``quotients``, the
1e9 guard in front of ``astype(int)``) for the endpoints, the cost with ``outside_cost``, and for the two calls the lattice and
packing of tests/lattice_yardstick.py and the move, centre-first offsets and packing of tests/refine_yardstick.py.  Cosines and
sines of the HEADINGS are optional, as in the other yardsticks: tables for ``costs`` and ``search_points``, a ``sincos`` function
(angles -> (cos, sin)) for ``refine_points``, asked for the seeds' headings (only with a motion) and then for every seed's
candidate headings [N, nth], in that order."""
import numpy as np

import lattice_yardstick as lyard
import mcl_yardstick as mcl
import refine_yardstick as ryard
import score_yardstick as yard


def valid(points):
    """bool [M]: both coordinates finite."""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    return np.isfinite(q[:, 0]) & np.isfinite(q[:, 1])


def offsets(points, cos, sin):
    """(ex, ey), each [valid]: R(heading) q of the valid points in point order, from the heading's ``cos`` and ``sin`` -- two
    rounded products and one rounded subtract or add per component."""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    q = q[valid(q)]
    c, s = np.float64(cos), np.float64(sin)
    with np.errstate(invalid="ignore", over="ignore"):
        return (c * q[:, 0]) - (s * q[:, 1]), (s * q[:, 0]) + (c * q[:, 1])


def cells(field_shape, frame, step, x, y, ex, ey):
    """(inside, cx, cy), each [..., valid], for positions ``x``, ``y`` of any one shape: steps 3-4 of slam2d_score_poses.  A
    quotient that fails the guard is never converted (its cell reads 0 here and is not inside)."""
    fh, fw = field_shape
    with np.errstate(invalid="ignore", over="ignore"):
        px, py = np.asarray(x, dtype=np.float64)[..., None] + ex, np.asarray(y, dtype=np.float64)[..., None] + ey
        qx, qy = yard.quotients(px, py, frame[0], frame[1], step)
        ok = (np.abs(qx) < 1e9) & (np.abs(qy) < 1e9)          # the guard, before astype(int): a NaN fails it
    cx, cy = np.where(ok, qx, 0.0).astype(int), np.where(ok, qy, 0.0).astype(int)      # truncation
    inside = ok & (cx >= 0) & (cx < fw) & (cy >= 0) & (cy < fh)
    return inside, cx, cy


def costs(field, frame, step, poses, points, outside_cost, cos=None, sin=None):
    """(cost, inside, valid) of the poses [..., 3] whose headings take ``cos`` / ``sin`` of the same leading shape (None:
    NumPy's): uint64, int64 [...], and the number of valid points (an int: it does not depend on the pose)."""
    poses = np.asarray(poses, dtype=np.float64)
    lead = poses.shape[:-1]
    P = poses.reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        c = np.cos(P[:, 2]) if cos is None else np.asarray(cos, dtype=np.float64).reshape(-1)
        s = np.sin(P[:, 2]) if sin is None else np.asarray(sin, dtype=np.float64).reshape(-1)
    n_valid = int(valid(points).sum())
    cost64 = np.asarray(field).astype(np.uint64)
    cost, n_in = np.empty(len(P), dtype=np.uint64), np.empty(len(P), dtype=np.int64)
    # poses of one heading (the same cos and sin bits) share their offsets
    key = np.stack([c, s], axis=1).view(np.uint64)
    uniq, inverse = np.unique(key, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    for u, (cb, sb) in enumerate(uniq.view(np.float64)):
        sel = np.flatnonzero(inverse == u)
        ex, ey = offsets(points, cb, sb)
        inside, cx, cy = cells(cost64.shape, frame, step, P[sel, 0], P[sel, 1], ex, ey)
        vals = cost64[np.where(inside, cy, 0), np.where(inside, cx, 0)]
        n_in[sel] = inside.sum(axis=-1)
        cost[sel] = np.where(inside, vals, np.uint64(0)).sum(axis=-1, dtype=np.uint64) + \
            (n_valid - n_in[sel]).astype(np.uint64) * np.uint64(outside_cost)
    return cost.reshape(lead), n_in.reshape(lead), n_valid


def search_points(field, frame, step, lat, points, outside_cost, cos=None, sin=None):
    """The image slam2d_search_points writes, uint64 [ny, nx].  ``cos`` / ``sin``: None or [nth] tables of the lattice's headings
    (``lattice_yardstick.axes(lat)[2]``)."""
    P = lyard.poses(lat)
    nth, ny, nx = P.shape[:3]
    rep = lambda t: None if t is None else np.broadcast_to(np.asarray(t, dtype=np.float64).reshape(nth, 1, 1), (nth, ny, nx))
    return lyard.pack(costs(field, frame, step, P, points, outside_cost, rep(cos), rep(sin))[0])


def refine_points(field, frame, step, seeds, radii, steps, points, outside_cost, motion=None, sincos=mcl.numpy_sincos):
    """One slam2d_refine_points: (words uint64 [N, 2], poses [N, 3]).  ``points``: [M, 2] (one set for all seeds) or [N, M, 2]."""
    seeds = np.array(seeds, dtype=np.float64).reshape(-1, 3)
    points = np.asarray(points, dtype=np.float64)
    moved = ryard.move(seeds, motion) if motion is None else ryard.move(seeds, motion, *sincos(seeds[:, 2].copy()))
    hc, hs = sincos(np.array([ryard.axes(m, radii, steps)[2] for m in moved]))                    # [N, nth]
    words = np.empty((len(seeds), 2), dtype=np.uint64)
    poses = np.empty((len(seeds), 3))
    for n, m in enumerate(moved):
        C = ryard.candidates(m, radii, steps)                  # [nth, ny, nx, 3]
        rep = lambda t: np.broadcast_to(np.asarray(t).reshape(-1, 1, 1), C.shape[:3])
        cost = costs(field, frame, step, C, points if points.ndim == 2 else points[n], outside_cost, rep(hc[n]), rep(hs[n]))[0]
        words[n] = ryard.pack(cost)
        poses[n] = C.reshape(-1, 3)[int(ryard.index_of(words[n])[0])]
    return words, poses


def refine_stages(field, frame, step, seeds, stages, points, outside_cost, motion=None, sincos=mcl.numpy_sincos):
    """The stages ((rx, ry, rt), (dx, dy, dth)) chained, the motion in the first: (words uint64 [N, stages, 2], poses [N, 3])."""
    poses = np.array(seeds, dtype=np.float64).reshape(-1, 3)
    words = []
    for i, (radii, steps) in enumerate(stages):
        w, poses = refine_points(field, frame, step, poses, radii, steps, points, outside_cost, motion if i == 0 else None, sincos)
        words.append(w)
    return np.stack(words, axis=1), poses
