"""The definition of slam2d_refine_poses (include/slam2d.h) in NumPy, for the tests, built on tests/score_yardstick.py for the
cost and tests/mcl_yardstick.py for the move (its ``move`` at amplitude 0 and noise 0): the centre-first offsets, a seed's
candidates materialised, every one scored by ``score_poses``, of its rows slot 6 (sum_b), 3 (inside) and 4 (in range) formed into
the cost, and the packed 64-bit minimum with its nearest-the-seed tie-break.  Cosines and sines are optional, as in the other
yardsticks: ``refine`` takes a ``sincos`` function (angles -> (cos, sin)) and asks it for the seeds' headings (only with a
motion), then for the beam angles of every seed's candidate headings, in that order."""
import numpy as np

import mcl_yardstick as mcl
import score_yardstick as yard

INDEX_BITS = 20


def offsets(r):
    """int64 [2 r + 1]: off(j) = ((j + 1) >> 1) * (+1 if j is odd else -1) -- 0, +1, -1, +2, -2, ..."""
    return np.array([((j + 1) >> 1) * (1 if j & 1 else -1) for j in range(2 * int(r) + 1)], dtype=np.int64)


def move(seeds, motion, cos=None, sin=None):
    """The moved seeds [N, 3]: slam2d_mcl_step's move without noise; ``motion`` None: the seeds themselves, bit for bit."""
    p = np.array(seeds, dtype=np.float64).reshape(-1, 3)
    if motion is None:
        return p
    return mcl.move(p, motion, (0.0, 0.0, 0.0), np.zeros((len(p), 3)), cos, sin)


def axes(seed, radii, steps):
    """(xs [nx], ys [ny], thetas [nth]) about the MOVED seed: a rounded product, then an add."""
    x, y, th = (np.float64(v) for v in seed)
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(c + offsets(r).astype(np.float64) * np.float64(d) for c, r, d in zip((x, y, th), radii, steps))


def candidates(seed, radii, steps):
    """[nth, ny, nx, 3]: candidate (jt, jy, jx) of the moved seed; its flat index is (jt * ny + jy) * nx + jx."""
    xs, ys, ths = axes(seed, radii, steps)
    gt, gy, gx = np.meshgrid(ths, ys, xs, indexing="ij")
    return np.stack([gx, gy, gt], axis=-1)


def beam_angles(seed, radii, steps, fov, beams):
    """[nth, beams]: the beam angles of every candidate heading of the moved seed (for the device's cos / sin tables)."""
    return np.array([yard.beam_angles(th, fov, beams) for th in axes(seed, radii, steps)[2]])


def costs(field, frame, cost_scale, step, seed, radii, steps, ranges, fov, max_range, outside_cost, cos=None, sin=None):
    """(cost, inside, in_range) of the moved seed's candidates, each [nth, ny, nx] (uint64, int64, int64).  ``cos`` / ``sin``: None
    or [nth, beams] tables of ``beam_angles``."""
    C = candidates(seed, radii, steps)
    nth, ny, nx = C.shape[:3]
    per = ny * nx
    rows = yard.score_poses(field, frame, cost_scale, step, C.reshape(-1, 3), np.asarray(ranges, dtype=np.float64), fov, max_range,
                            None if cos is None else np.repeat(np.asarray(cos), per, axis=0),
                            None if sin is None else np.repeat(np.asarray(sin), per, axis=0))
    sum_b = rows[:, 6].astype(np.uint64)                       # (below 2^53: exact in the double)
    inside, in_range = rows[:, 3].astype(np.int64), rows[:, 4].astype(np.int64)
    cost = sum_b + (in_range - inside).astype(np.uint64) * np.uint64(outside_cost)
    return cost.reshape(nth, ny, nx), inside.reshape(nth, ny, nx), in_range.reshape(nth, ny, nx)


def pack(cost):
    """The two words of one seed, uint64 [2]: the minimum over the candidates of cost << 20 | f -- the lowest flat index among
    equal costs, which is the candidate nearest the seed -- and cost(0)."""
    flat = np.asarray(cost, dtype=np.uint64).reshape(-1)
    assert flat.size <= 1 << INDEX_BITS and int(flat.max()) < 1 << 44
    return np.array([((flat << np.uint64(INDEX_BITS)) | np.arange(flat.size, dtype=np.uint64)).min(), flat[0]], dtype=np.uint64)


def index_of(words):
    return (np.asarray(words, dtype=np.uint64).reshape(-1, 2)[:, 0] & np.uint64((1 << INDEX_BITS) - 1)).astype(np.int64)


def cost_of(words):
    return np.asarray(words, dtype=np.uint64).reshape(-1, 2)[:, 0] >> np.uint64(INDEX_BITS)


def refine(field, frame, cost_scale, step, seeds, radii, steps, ranges, fov, max_range, outside_cost, motion=None, sincos=mcl.numpy_sincos):
    """One slam2d_refine_poses: (words uint64 [N, 2], poses [N, 3]).  ``ranges``: [beams] (one scan for all seeds) or [N, beams]."""
    seeds = np.array(seeds, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    moved = move(seeds, motion) if motion is None else move(seeds, motion, *sincos(seeds[:, 2].copy()))
    beams = ranges.shape[-1]
    bc, bs = sincos(np.array([beam_angles(m, radii, steps, fov, beams) for m in moved]))           # [N, nth, beams]
    words = np.empty((len(seeds), 2), dtype=np.uint64)
    poses = np.empty((len(seeds), 3))
    for n, m in enumerate(moved):
        cost = costs(field, frame, cost_scale, step, m, radii, steps, ranges if ranges.ndim == 1 else ranges[n], fov, max_range,
                     outside_cost, bc[n], bs[n])[0]
        words[n] = pack(cost)
        poses[n] = candidates(m, radii, steps).reshape(-1, 3)[int(index_of(words[n])[0])]
    return words, poses


def refine_stages(field, frame, cost_scale, step, seeds, stages, ranges, fov, max_range, outside_cost, motion=None, sincos=mcl.numpy_sincos):
    """The stages ((rx, ry, rt), (dx, dy, dth)) chained, the motion in the first: (words uint64 [N, stages, 2], poses [N, 3])."""
    poses = np.array(seeds, dtype=np.float64).reshape(-1, 3)
    words = []
    for i, (radii, steps) in enumerate(stages):
        w, poses = refine(field, frame, cost_scale, step, poses, radii, steps, ranges, fov, max_range, outside_cost,
                          motion if i == 0 else None, sincos)
        words.append(w)
    return np.stack(words, axis=1), poses
