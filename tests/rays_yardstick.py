"""The definitions of slam2d_cast_rays and slam2d_score_rays (include/slam2d.h) in NumPy, for the tests: the ray walked sample by
sample -- vectorised over rays, a loop over k, NO skipping --, and the cost composed from tests/score_yardstick.py for the
endpoint part (slots 6, 3, 4 of its rows, as tests/lattice_yardstick.py forms slam2d_search_lattice's cost).  ``occ`` is the
occupied image [fh, fw] (bool) of the slot, ``frame`` = (xlo, ylo), ``lidar`` = (fov, beams, max_range); the GPU tests hand in the
DEVICE's occupied image and frame record, and the device's cos / sin of the very beam angles.  ``skip_walk`` restates the
kernel's skip rule, for the host tests and the profile note's sample counts."""
import numpy as np

import score_yardstick as yard

RAYS_STRIDE = 8
HIT, LEFT, NONE = 0, 1, 2


def trig(poses, lidar, cos=None, sin=None):
    """([N, beams] cos, sin) of the poses' beam angles: the tables given, else NumPy's."""
    if cos is not None:
        return np.asarray(cos, dtype=np.float64), np.asarray(sin, dtype=np.float64)
    fov, beams, _ = lidar
    with np.errstate(invalid="ignore"):
        a = np.array([yard.beam_angles(th, fov, beams) for th in np.asarray(poses, dtype=np.float64).reshape(-1, 3)[:, 2]])
        return np.cos(a), np.sin(a)


def sample(shape, frame, step, x, y, c, s, k):
    """(inside, cy, cx) of sample k (an int, or an int array shaped like the rays) of the rays from (x, y) along (c, s): every
    operation rounded, in the header's order.  cy / cx are 0 where the sample is not inside."""
    fh, fw = shape
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(k, dtype=np.float64) * step
        px, py = x + c * t, y + s * t
        qx, qy = (px - frame[0]) / step, (py - frame[1]) / step
        ok = (qx >= 0) & (qx < 1e9) & (qy >= 0) & (qy < 1e9)   # a NaN fails; note the 0 <=
    cx, cy = np.zeros(ok.shape, dtype=np.int64), np.zeros(ok.shape, dtype=np.int64)
    cx[ok], cy[ok] = qx[ok].astype(np.int64), qy[ok].astype(np.int64)          # only guarded quotients are converted
    inside = ok & (cx < fw) & (cy < fh)
    return inside, np.where(inside, cy, 0), np.where(inside, cx, 0)


def walk(occ, frame, step, x, y, c, s, limit):
    """(kind, k), int64 arrays shaped like the rays: every ray walked sample by sample up to its ``limit`` (an int array of that
    shape, entries >= 0; a ray with limit < 0 is not walked: NONE at 0)."""
    occ = np.asarray(occ, dtype=bool)
    x, y, c, s = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (x, y, c, s)))
    limit = np.broadcast_to(np.asarray(limit, dtype=np.int64), x.shape)
    kind = np.full(x.shape, NONE, dtype=np.int64)
    kk = np.maximum(limit + 1, 0)
    live = limit >= 0
    for k in range(int(limit.max(initial=-1)) + 1):
        live = live & (k <= limit)
        if not live.any():
            break
        inside, cy, cx = sample(occ.shape, frame, step, x, y, c, s, k)
        left = live & ~inside
        hit = live & inside & occ[cy, cx]
        kind[left], kind[hit] = LEFT, HIT
        kk[left | hit] = k
        live = live & ~(left | hit)
    return kind, kk


def words(kind, k):
    """kind << 30 | k as slam2d_cast_rays writes it (uint32)."""
    return ((np.asarray(kind, dtype=np.uint32) << np.uint32(30)) | np.asarray(k, dtype=np.uint32)).astype(np.uint32)


def cast(occ, frame, step, lidar, poses, K, cos=None, sin=None):
    """The words of slam2d_cast_rays: uint32 [N, beams]."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    c, s = trig(poses, lidar, cos, sin)
    kind, k = walk(occ, frame, step, poses[:, 0:1], poses[:, 1:2], c, s, np.full(c.shape, int(K), dtype=np.int64))
    return words(kind, k)


def beam_limits(ranges, step, max_range, margin):
    """(checked, kend) per beam: a beam IN RANGE is CHECKED iff r / step lies in [0, 1e9); kend = (int64)(r / step) - margin
    (-1 where not checked)."""
    r = np.asarray(ranges, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = r / step
        checked = (r < max_range) & (q >= 0) & (q < 1e9)
    kend = np.full(r.shape, -1, dtype=np.int64)
    kend[checked] = q[checked].astype(np.int64) - int(margin)
    return checked, kend


def score(occ, field, frame, step, lidar, poses, ranges, margin, outside_cost, through_cost, cos=None, sin=None):
    """The rows of slam2d_score_rays: float64 [N, RAYS_STRIDE].  ``field``: uint32 [fh, fw] costs; ``ranges``: [beams] or [N, beams]."""
    fov, beams, max_range = lidar
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    c, s = trig(poses, lidar, cos, sin)
    ends = yard.score_poses(field, frame, 1.0, step, poses, ranges, fov, max_range, c, s)
    sum_b = ends[:, 6].astype(np.uint64)                       # (below 2^53: exact in the double)
    inside, in_range = ends[:, 3].astype(np.int64), ends[:, 4].astype(np.int64)
    checked, kend = beam_limits(np.broadcast_to(ranges, c.shape), step, max_range, margin)
    kind, k = walk(occ, frame, step, poses[:, 0:1], poses[:, 1:2], c, s, kend)
    through = (kend >= 0) & (kind == HIT)
    depth = np.where(through, kend - k, 0).sum(axis=1)
    n_thr = through.sum(axis=1).astype(np.int64)
    cost = sum_b + (in_range - inside).astype(np.uint64) * np.uint64(outside_cost) + n_thr.astype(np.uint64) * np.uint64(through_cost)
    out = np.zeros((len(poses), RAYS_STRIDE))
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = cost.astype(np.float64), sum_b.astype(np.float64), inside, in_range
    out[:, 4], out[:, 5], out[:, 6] = n_thr, checked.sum(axis=1), depth
    return out


def isqrt(v):
    """floor(sqrt(v)) of non-negative integers below 2^52, exactly."""
    v = np.asarray(v, dtype=np.int64)
    d = np.sqrt(v.astype(np.float64)).astype(np.int64)
    d = np.where(d * d > v, d - 1, d)
    return np.where((d + 1) * (d + 1) <= v, d + 1, d)


def skip_walk(dist2, frame, step, x, y, c, s, limit):
    """(kind, k, examined): the kernel's walk restated.  A ray whose sample 0 is not inside is LEFT at 0.  Else the inside
    samples are one interval of k (every operation of the sample formula is monotone in k): its end k_exit <= limit + 1 is found
    by bisection, and the walk runs on [0, k_exit) -- at an examined sample in a cell of squared distance v > 0 the next examined
    sample is k + max(1, isqrt(v) - 1); v == 0 is a HIT.  Without a HIT the ray is LEFT at k_exit, or NONE where k_exit is
    limit + 1.  ``dist2`` [fh, fw]: 0 iff occupied, any other value a lower bound on the true squared distance.  ``examined``:
    cells read per ray."""
    dist2 = np.asarray(dist2, dtype=np.int64)
    x, y, c, s = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (x, y, c, s)))
    limit = np.broadcast_to(np.asarray(limit, dtype=np.int64), x.shape)
    at = lambda k: sample(dist2.shape, frame, step, x, y, c, s, k)
    kind = np.full(x.shape, NONE, dtype=np.int64)
    kk = np.maximum(limit + 1, 0)
    examined = np.zeros(x.shape, dtype=np.int64)
    live = (limit >= 0) & at(0)[0]
    left0 = (limit >= 0) & ~live
    kind[left0], kk[left0] = LEFT, 0
    lo, hi = np.zeros(x.shape, dtype=np.int64), np.where(live, limit + 1, 1)
    while (hi - lo > 1).any():
        go, mid = hi - lo > 1, (lo + hi) // 2
        inside = at(mid)[0]
        lo, hi = np.where(go & inside, mid, lo), np.where(go & ~inside, mid, hi)
    k_exit = hi
    leaves = live & (k_exit <= limit)
    kind[leaves], kk[leaves] = LEFT, k_exit[leaves]
    k = np.zeros(x.shape, dtype=np.int64)
    while live.any():
        inside, cy, cx = at(k)
        assert inside[live].all(), "a sample below k_exit is inside"
        v = dist2[cy, cx]
        examined[live] += 1
        hit = live & (v == 0)
        kind[hit], kk[hit] = HIT, k[hit]
        live = live & ~hit
        k = np.where(live, k + np.maximum(1, isqrt(v) - 1), k)
        live = live & (k < k_exit)
    return kind, kk, examined
