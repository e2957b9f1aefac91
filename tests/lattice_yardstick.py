"""The definition of slam2d_search_lattice (include/slam2d.h) in NumPy, for the tests, built on tests/score_yardstick.py: the
lattice's poses materialised, every one scored by ``score_poses``, and of its rows slot 6 (sum_b), 3 (inside) and 4 (in range)
formed into the cost, the packed 64-bit minimum over the headings and with it the lowest-heading tie-break."""
import numpy as np

import score_yardstick as yard


def axes(lat):
    """(xs [nx], ys [ny], thetas [nth]) of lat = (nx, ny, nth, x0, dx, y0, dy, th0, dth): a rounded product, then an add."""
    nx, ny, nth, x0, dx, y0, dy, th0, dth = lat
    with np.errstate(invalid="ignore", over="ignore"):
        return x0 + np.arange(nx) * dx, y0 + np.arange(ny) * dy, th0 + np.arange(nth) * dth


def poses(lat):
    """[nth, ny, nx, 3]: pose (it, iy, ix) of the lattice."""
    xs, ys, ths = axes(lat)
    gt, gy, gx = np.meshgrid(ths, ys, xs, indexing="ij")
    return np.stack([gx, gy, gt], axis=-1)


def beam_angles(lat, fov, beams):
    """[nth, beams]: the beam angles of every heading of the lattice (for the device's cos / sin tables)."""
    return np.array([yard.beam_angles(th, fov, beams) for th in axes(lat)[2]])


def costs(field, frame, cost_scale, step, lat, ranges, fov, max_range, outside_cost, cos=None, sin=None):
    """(cost, inside, in_range), each [nth, ny, nx] (uint64, int64, int64).  ``cos`` / ``sin``: None or [nth, beams] tables of
    ``beam_angles``."""
    P = poses(lat)
    nth, ny, nx = P.shape[:3]
    per = ny * nx
    rows = yard.score_poses(field, frame, cost_scale, step, P.reshape(-1, 3), np.asarray(ranges, dtype=np.float64), fov, max_range,
                            None if cos is None else np.repeat(np.asarray(cos), per, axis=0),
                            None if sin is None else np.repeat(np.asarray(sin), per, axis=0))
    sum_b = rows[:, 6].astype(np.uint64)                       # (below 2^53: exact in the double)
    inside, in_range = rows[:, 3].astype(np.int64), rows[:, 4].astype(np.int64)
    cost = sum_b + (in_range - inside).astype(np.uint64) * np.uint64(outside_cost)
    return cost.reshape(nth, ny, nx), inside.reshape(nth, ny, nx), in_range.reshape(nth, ny, nx)


def pack(cost):
    """[ny, nx] uint64 words: the minimum over the headings of cost << 16 | it -- the lowest heading among equal costs."""
    nth = cost.shape[0]
    assert nth <= 65536 and int(cost.max()) < 1 << 48
    it = np.arange(nth, dtype=np.uint64).reshape(-1, 1, 1)
    return ((cost.astype(np.uint64) << np.uint64(16)) | it).min(axis=0)


def search_lattice(field, frame, cost_scale, step, lat, ranges, fov, max_range, outside_cost, cos=None, sin=None):
    """The image slam2d_search_lattice writes: uint64 [ny, nx]."""
    return pack(costs(field, frame, cost_scale, step, lat, ranges, fov, max_range, outside_cost, cos, sin)[0])
