"""The definition of slam2d_predict_scan (include/slam2d.h) evaluated in NumPy from oracle.slam_oracle.GridOracle's own tables: the
yardstick of tests/test_predict_host.py and tests/test_gpu_predict.py.  A helper module, not a test."""
import numpy as np

from oracle import slam_oracle as so


def predict(og, pose, r_min=0.0, r_max=None):
    """``og``: a GridOracle (or ``oracle_of`` a device grid).  Returns (first, far, cells) per beam: r_hit (+inf without a hit),
    r_far (-inf), n_hit."""
    lut, B = og.lut, og.numSamplesPerRev
    S, W, unit, R = lut.num_spokes, lut.width, og.unitGridSize, og.lidarMaxRange
    r_max = R if r_max is None else r_max
    first, far, cells = np.full(B, np.inf), np.full(B, -np.inf), np.zeros(B, dtype=np.int64)
    x, y, theta = (np.float64(v) for v in pose)
    with np.errstate(all="ignore"):
        quotients = [theta / (2 * np.pi) * S] + [((p + e) - lim[0]) / unit
                                                 for p, lim in ((x, og.mapXLim), (y, og.mapYLim)) for e in (lut.xs[0], lut.xs[-1])]
    if not (np.isfinite([x, y, theta]).all() and all(abs(q) < 1e9 for q in quotients)):
        return first, far, cells                                       # such a pose sees nothing
    occupied = 2 * og.visited > og.total
    rows, cols = occupied.shape
    offset = int(np.rint(quotients[0]))
    wall = og.wallThickness / 2 + og.wallThickness / 2
    r_flat = lut.r.ravel()
    for b in range(B):
        c = lut.cells_of((og.spokesStartIdx + offset + b) % S)
        r = r_flat[c]
        mx, my = og.convertRealXYToMapIdx(x + lut.xs[c % W], y + lut.xs[c // W])
        hit = (mx >= 0) & (mx < cols) & (my >= 0) & (my < rows) & (r > r_min) & (r < r_max)
        hit[hit] = occupied[my[hit], mx[hit]]
        if hit.any():
            first[b] = r[hit].min()
            in_wall = hit & (r < first[b] + wall)
            far[b], cells[b] = r[in_wall].max(), in_wall.sum()
    return first, far, cells


def predict_many(og, poses, r_min=0.0, r_max=None):
    out = [predict(og, p, r_min, r_max) for p in poses]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def oracle_of(visited, total, lim_x, lim_y, unit, fov, beams, max_range, wall):
    """A GridOracle around downloaded count arrays and limits (a device grid, a particle's map): its tables and its index rule."""
    og = so.GridOracle(1, 1, {"x": 0.0, "y": 0.0}, unit, fov, beams, max_range, wall, lut=_lut(unit, max_range, fov, beams))
    og.visited, og.total = np.asarray(visited, dtype=np.float64), np.asarray(total, dtype=np.float64)
    og.mapXLim, og.mapYLim = list(lim_x), list(lim_y)
    return og


_LUTS = {}


def _lut(unit, max_range, fov, beams):
    key = (float(unit), float(max_range), float(fov), int(beams))
    if key not in _LUTS:
        _LUTS[key] = so.SpokeLUT(unit, max_range, fov, beams)
    return _LUTS[key]


def beam_walls(og, reading):
    """What one updateOccupancyGrid at ``reading`` writes as a wall, beam by beam, from the oracle's own update=False variant (one
    beam's range at a time, the others out of reach): a list of the tabulated radii of each beam's occupied window cells."""
    lut, B, R = og.lut, og.numSamplesPerRev, og.lidarMaxRange
    step = (lut.xs[-1] - lut.xs[0]) / (lut.width - 1)
    out = []
    for b in range(B):
        rng = np.full(B, 1e9)
        rng[b] = reading["range"][b]
        _, _, ox, oy = og.updateOccupancyGrid(dict(reading, range=rng), update=False)
        j = np.rint((ox - reading["x"] + R) / step).astype(int)
        i = np.rint((oy - reading["y"] + R) / step).astype(int)
        out.append(lut.r[i, j])
    return out
