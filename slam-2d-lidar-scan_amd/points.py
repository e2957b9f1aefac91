"""Point sets in the robot's frame -- x forward, y to the left, metres -- for ``ScanMatcher.searchPoints``, ``refinePoints`` and
``Tracker.step_points`` (include/slam2d.h, slam2d_search_points): a scan as points, a driver's own beam angles, a sensor mounted
off the robot's origin, several scans joined by their odometry.  Host NumPy: input preparation.  A row with a NaN or an infinity
is an invalid point, which the searches drop as they drop a beam out of range."""
import math

import numpy as np

from . import _lib

MAX_POINTS = _lib.MAX_POINTS


def _mount(mount):
    mx, my, mth = (float(v) for v in mount)
    return mx, my, mth


def polar_points(ranges, angles, max_range, mount=(0, 0, 0), sincos=None):
    """``[beams, 2]``: beam b of a sensor mounted at ``mount = (mx, my, mth)`` in the robot's frame, at the angle ``angles[b]`` in
    the SENSOR's frame, as the point ``(mx, my) + (cos(a) r, sin(a) r)`` with ``a = mth + angles[b]``; NaN rows for beams not
    in range (``not r < max_range``).  ``sincos``: None (NumPy's) or a function angles -> (cos, sin)."""
    r = np.asarray(ranges, dtype=np.float64).reshape(-1)
    mx, my, mth = _mount(mount)
    a = mth + np.asarray(angles, dtype=np.float64).reshape(-1)
    if a.shape != r.shape:
        raise ValueError(f"{a.size} angles for {r.size} ranges")
    return _polar(r, a, max_range, mx, my, sincos)


def _polar(r, a, max_range, mx, my, sincos):
    c, s = (np.cos(a), np.sin(a)) if sincos is None else sincos(a)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = r < max_range                                   # NaN and +inf are out, 0 and negative ranges are in
        q = np.stack([mx + np.asarray(c) * r, my + np.asarray(s) * r], axis=1)
    q[~keep] = np.nan
    return q


def scan_points(ranges, fov, max_range, mount=(0, 0, 0), sincos=None):
    """``[beams, 2]``: a scan of the grid's own fan as points.  Beam b is at the fan's angle for heading ``mount[2]`` -- step 1 of
    slam2d_score_poses, ``numpy.linspace(mount[2] - fov / 2, mount[2] + fov / 2, beams)`` --, its point ``mount[:2] + (cos(a_b)
    r_b, sin(a_b) r_b)``; NaN rows for beams not in range.  With the default mount and the cos / sin the scan forms use, a
    pose of heading exactly 0 costs what the scan costs there, bit for bit."""
    r = np.asarray(ranges, dtype=np.float64).reshape(-1)
    mx, my, mth = _mount(mount)
    return _polar(r, np.linspace(mth - fov / 2, mth + fov / 2, num=len(r)), max_range, mx, my, sincos)


def decimation(valid, max_points):
    """(stride, kept): with more valid points than ``max_points`` every ``ceil(valid / max_points)``-th one is kept, from the
    first: ``kept = arange(0, valid, stride)``."""
    valid, max_points = int(valid), int(max_points)
    if max_points < 1:
        raise ValueError(f"max_points wants at least 1, not {max_points}")
    stride = max(1, -(-valid // max_points))
    return stride, np.arange(0, valid, stride)


def merge_scans(readings, max_points=MAX_POINTS, *, fov, max_range, mount=(0, 0, 0)):
    """The points of K readings (dicts of x, y, theta -- the RAW odometry pose -- and range) in the frame of the LAST reading's
    pose: each scan as ``scan_points``, carried through its own odometry pose into the world and back through the last one,
    in the order of the readings and of their beams, invalid points left out.  Returns ``(points [m, 2], stride)``, m <=
    ``max_points`` (``decimation``).  Odometry drifts: join the last few scans, not a long history."""
    if not len(readings):
        raise ValueError("no readings")
    last = readings[-1]
    xl, yl, tl = float(last["x"]), float(last["y"]), float(last["theta"])
    cl, sl = math.cos(tl), math.sin(tl)
    parts = []
    for rd in readings:
        q = scan_points(rd["range"], fov, max_range, mount)
        q = q[np.isfinite(q).all(axis=1)]
        t = float(rd["theta"])
        c, s = math.cos(t), math.sin(t)
        wx = float(rd["x"]) + c * q[:, 0] - s * q[:, 1] - xl
        wy = float(rd["y"]) + s * q[:, 0] + c * q[:, 1] - yl
        parts.append(np.stack([cl * wx + sl * wy, cl * wy - sl * wx], axis=1))
    pts = np.concatenate(parts)
    pts = pts[np.isfinite(pts).all(axis=1)]
    stride, kept = decimation(len(pts), max_points)
    return np.ascontiguousarray(pts[kept]), stride


def reach(points):
    """The largest |q| of a valid point (0 without one)."""
    q = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    q = q[np.isfinite(q).all(axis=1)]
    return float(np.hypot(q[:, 0], q[:, 1]).max()) if len(q) else 0.0
