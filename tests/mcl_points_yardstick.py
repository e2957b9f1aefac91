"""The definitions of slam2d_mcl_step_points, slam2d_mcl_step_adaptive_points and slam2d_score_points (include/slam2d.h) in NumPy,
for the tests, composed from the yardsticks that exist: the noise, the move, the weights, the resampler and the report words of
tests/mcl_yardstick.py, the reference ancestors, the pose bins and the sized resampling of tests/mcl_adapt_yardstick.py, and the
point cost of tests/points_yardstick.py (``costs``, ``cells``).  Nothing is restated here but the order of the steps.  ``step`` and
``step_adaptive`` take a ``sincos`` function (angles -> (cos, sin)) and ask it for the headings of the poses and then for the
headings of the MOVED poses -- the one pair per particle that the WEIGH step and the report's sums share."""
import numpy as np

import mcl_adapt_yardstick as ada
import mcl_yardstick as mcl
import points_yardstick as pyard

REPORT, ADAPT_REPORT, SCORE_STRIDE = mcl.REPORT, ada.REPORT, 8


def _moved_and_costs(field, frame, step_len, poses, motion, amp, seed, scan, points, outside_cost, sincos):
    """Steps a-c up to the costs: (moved [N, 3], cost uint64 [N], valid, (cos, sin) of the moved headings)."""
    g = mcl.noise(len(poses), seed, scan)
    moved = mcl.move(poses, motion, amp, g, *sincos(poses[:, 2].copy()))
    mc, ms = sincos(moved[:, 2].copy())
    cost, _, valid = pyard.costs(field, frame, step_len, moved, points, outside_cost, mc, ms)
    return moved, cost, valid, (mc, ms)


def step(field, frame, step_len, poses, motion, amp, seed, scan, points, outside_cost, lut, shift, sincos=mcl.numpy_sincos):
    """One slam2d_mcl_step_points: ``mcl_yardstick.step``'s dict -- ``moved`` [N, 3], ``cost``, ``w``, ``ancestors`` int32 [N],
    ``out`` [N, 3] and ``report`` uint64 [16], whose word 5 is the number of valid points."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    moved, cost, valid, cs = _moved_and_costs(field, frame, step_len, poses, motion, amp, seed, scan, points, outside_cost, sincos)
    w, cmin, best = mcl.weights(cost, lut, shift)
    anc, W, u0 = mcl.resample(w, mcl.resample_word(seed, scan))
    rep = mcl.report(cost, w, W, u0, valid, moved, anc, *cs)
    return dict(moved=moved, cost=cost, w=w, ancestors=anc, out=moved[anc], report=rep)


def step_adaptive(field, frame, step_len, poses, n_in, n_cap, motion, amp, seed, scan, points, outside_cost, lut, shift, bins, ntab,
                  sincos=mcl.numpy_sincos):
    """One slam2d_mcl_step_adaptive_points: ``mcl_adapt_yardstick.step``'s dict over the first N = min(max(n_in, 1), n_cap) poses."""
    N = min(max(int(n_in), 1), int(n_cap))
    poses = np.asarray(poses, dtype=np.float64)[:N, :3].copy()
    moved, cost, valid, cs = _moved_and_costs(field, frame, step_len, poses, motion, amp, seed, scan, points, outside_cost, sincos)
    w, cmin, best = mcl.weights(cost, lut, shift)
    r = mcl.resample_word(seed, scan)
    ref = ada.reference_ancestors(w, r)
    kbins = len(np.unique(ada.bins_of(moved[ref], bins)))
    n_out = ada.size_of(kbins, ntab, n_cap)
    anc, W, u0 = ada.resample_to(w, r, n_out)
    rep = np.zeros(ADAPT_REPORT, dtype=np.uint64)
    rep[:16] = mcl.report(cost, w, W, u0, valid, moved, anc, *cs)
    rep[16], rep[17], rep[18], rep[19] = N, n_out, kbins, len(ref)
    return dict(N=N, moved=moved, cost=cost, w=w, reference=ref, kbins=kbins, n_out=n_out, ancestors=anc, out=moved[anc], report=rep)


def score_points(field, frame, cost_scale, step_len, poses, points, cos=None, sin=None):
    """slam2d_score_points' rows [N, 8]: sum_u and |U| over the SET of cells of the inside points, sum_b, inside and valid.
    ``points``: [M, 2] (one set for every pose) or [N, M, 2]; ``cos`` / ``sin``: None (NumPy's) or [N], of the poses' headings."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    points = np.asarray(points, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = np.cos(poses[:, 2]) if cos is None else np.asarray(cos, dtype=np.float64).reshape(-1)
        s = np.sin(poses[:, 2]) if sin is None else np.asarray(sin, dtype=np.float64).reshape(-1)
    cost64 = np.asarray(field).astype(np.uint64)
    inv = 1.0 / cost_scale
    out = np.empty((len(poses), SCORE_STRIDE))
    for n, (x, y, _) in enumerate(poses):
        pts = points if points.ndim == 2 else points[n]
        ex, ey = pyard.offsets(pts, c[n], s[n])
        inside, cx, cy = pyard.cells(cost64.shape, frame, step_len, x, y, ex, ey)
        cx, cy = cx[inside], cy[inside]
        cells = np.unique(np.column_stack((cx, cy)), axis=0) if cx.size else np.zeros((0, 2), dtype=int)
        sum_u = int(cost64[cells[:, 1], cells[:, 0]].sum(dtype=np.uint64))
        sum_b = int(cost64[cy, cx].sum(dtype=np.uint64))
        out[n] = [-(float(sum_u) * inv), len(cells), -(float(sum_b) * inv), cx.size, int(pyard.valid(pts).sum()), float(sum_u), float(sum_b), 0.0]
    return out
