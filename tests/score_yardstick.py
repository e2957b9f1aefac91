"""The definition of slam2d_score_poses (include/slam2d.h) in NumPy, for the tests: the score of a scan at free poses in a search
field, built from the oracle's own expressions -- MatcherOracle.covertMeasureToXY for the beam endpoints
(Utils/ScanMatcher_OGBased.py:81-89) and the field-index expression of :173-176, ``((p - lo) / step).astype(int)``, as
MatcherOracle.unique_cells applies it -- with np.unique (:120) for the set and the sum of :129-130 in the field's integers."""
import numpy as np

from oracle import slam_oracle as so

SCORE_STRIDE = 8


class _Lidar:
    """What MatcherOracle.covertMeasureToXY reads of its grid."""

    def __init__(self, fov, beams, max_range):
        self.lidarFOV, self.numSamplesPerRev, self.lidarMaxRange = fov, beams, max_range


def beam_angles(theta, fov, beams):
    """The beam angles of a pose as covertMeasureToXY forms them (:82-83)."""
    with np.errstate(invalid="ignore"):
        return np.linspace(theta - fov / 2, theta + fov / 2, num=beams)


def endpoints(x, y, theta, ranges, fov, beams, max_range, cos=None, sin=None):
    """(keep, px, py): the beams in range (:84) and their endpoints (:87-88).  With ``cos`` / ``sin`` tables ([beams], of
    ``beam_angles``) the same expression takes them in place of np.cos / np.sin; without, the oracle's method itself runs."""
    ranges = np.asarray(ranges, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = ranges < max_range
        if cos is None:
            px, py = so.MatcherOracle.covertMeasureToXY(type("M", (), {"og": _Lidar(fov, beams, max_range)})(), x, y, theta, ranges)
        else:
            px, py = x + np.asarray(cos)[keep] * ranges[keep], y + np.asarray(sin)[keep] * ranges[keep]
    return keep, px, py


def quotients(px, py, xlo, ylo, step):
    """The field-index quotients before truncation (:174-175)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (px - xlo) / step, (py - ylo) / step


def score_pose(field, frame, cost_scale, step, pose, ranges, fov, max_range, cos=None, sin=None):
    """One row of slam2d_score_poses.  ``field``: uint32 [fh, fw] costs; ``frame``: (xlo, ylo)."""
    fh, fw = field.shape
    x, y, theta = (float(v) for v in pose)
    beams = len(ranges)
    keep, px, py = endpoints(x, y, theta, ranges, fov, beams, max_range, cos, sin)
    qx, qy = quotients(px, py, frame[0], frame[1], step)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(qx) < 1e9) & (np.abs(qy) < 1e9)          # the guard, before astype(int): a NaN fails it
    cx, cy = qx[ok].astype(int), qy[ok].astype(int)           # :174-175, truncation
    inside = (cx >= 0) & (cx < fw) & (cy >= 0) & (cy < fh)
    cx, cy = cx[inside], cy[inside]
    cells = np.unique(np.column_stack((cx, cy)), axis=0) if cx.size else np.zeros((0, 2), dtype=int)      # :120
    cost = field.astype(np.uint64)
    sum_u = int(cost[cells[:, 1], cells[:, 0]].sum(dtype=np.uint64))
    sum_b = int(cost[cy, cx].sum(dtype=np.uint64))
    inv = 1.0 / cost_scale
    return np.array([-(float(sum_u) * inv), len(cells), -(float(sum_b) * inv), cx.size, int(keep.sum()), float(sum_u), float(sum_b), 0.0])


def score_poses(field, frame, cost_scale, step, poses, ranges, fov, max_range, cos=None, sin=None):
    """[N, SCORE_STRIDE].  ``ranges``: [beams] (one scan for all poses) or [N, beams]; ``cos`` / ``sin``: None or [N, beams]."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    out = np.empty((len(poses), SCORE_STRIDE))
    for n, pose in enumerate(poses):
        out[n] = score_pose(field, frame, cost_scale, step, pose, ranges if ranges.ndim == 1 else ranges[n], fov, max_range,
                            None if cos is None else cos[n], None if sin is None else sin[n])
    return out


def min_distance_to_integer(field_frame, step, poses, ranges, fov, max_range):
    """The smallest distance of any guarded quotient of these inputs from an integer: where it is well above the difference
    between two libms' cos / sin, every truncation is the same with either."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    best = np.inf
    for n, (x, y, theta) in enumerate(poses):
        r = ranges if ranges.ndim == 1 else ranges[n]
        _, px, py = endpoints(x, y, theta, r, fov, len(r), max_range)
        for q in quotients(px, py, field_frame[0], field_frame[1], step):
            with np.errstate(invalid="ignore"):
                q = q[np.abs(q) < 1e9]
            if q.size:
                best = min(best, float(np.abs(q - np.rint(q)).min()))
    return best
