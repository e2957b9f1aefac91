"""The definition of slam2d_mcl_step_adaptive (include/slam2d.h) in NumPy, for the tests, built on tests/mcl_yardstick.py: the
noise, the move, the costs, the weights and the resampler's word are that file's, over the N live particles; added here are the
reference ancestors (one ceiling division per particle, in Python integers: the products reach 2^64), the pose bins (one true
division per component, the guard in front of every conversion), the table's count and the resampling to that many offspring.
``step`` takes the same ``sincos`` hook as ``mcl_yardstick.step`` and asks it for the same three sets of angles."""
from collections import namedtuple

import numpy as np

import mcl_yardstick as mcl
import score_yardstick as yard

REPORT = 24
Bins = namedtuple("Bins", "x0 y0 cell turn nx ny nth")


def bins_of(moved, bins):
    """The pose bin of every row of ``moved`` [n, 3] (int64): (it * ny + iy) * nx + ix, or nx * ny * nth where the pose is not
    binnable.  No quotient that fails the guard is converted to an integer."""
    b = Bins(*bins)
    m = np.asarray(moved, dtype=np.float64).reshape(-1, 3)
    n_bins = int(b.nx) * int(b.ny) * int(b.nth)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        qx = (m[:, 0] - np.float64(b.x0)) / np.float64(b.cell)
        qy = (m[:, 1] - np.float64(b.y0)) / np.float64(b.cell)
        qt = m[:, 2] / np.float64(b.turn)
        ok = (np.abs(qx) < 1e9) & (np.abs(qy) < 1e9) & (np.abs(qt) < 1e9)      # (a NaN fails)
    out = np.full(len(m), n_bins, dtype=np.int64)
    ix, iy, it = (np.floor(q[ok]).astype(np.int64) for q in (qx, qy, qt))
    inside = (ix >= 0) & (ix < b.nx) & (iy >= 0) & (iy < b.ny)
    it = it % np.int64(b.nth)                                  # (non-negative: Python's %)
    out[np.flatnonzero(ok)[inside]] = ((it * b.ny + iy) * b.nx + ix)[inside]
    return out


def reference_ancestors(w, r):
    """The distinct ancestors of mcl_yardstick.resample(w, r), ascending (int64), without resampling: n is one iff the least k
    with k * W + u0 >= C_(n-1) * N is below N and has k * W + u0 < C_n * N.  W == 0: every n."""
    w = [int(v) for v in np.asarray(w, dtype=np.uint64)]
    N = len(w)
    W = sum(w)
    if W == 0:
        return np.arange(N, dtype=np.int64)
    u0 = (int(r) * W) >> 32
    out, before = [], 0
    for n in range(N):
        lo, hi = before * N, (before + w[n]) * N
        k = -((u0 - lo) // W) if lo > u0 else 0                # ceil((lo - u0) / W)
        if k < N and k * W + u0 < hi:
            out.append(n)
        before += w[n]
    return np.array(out, dtype=np.int64)


def resample_to(w, r, n_out):
    """(ancestors int32 [n_out], W, u0): systematic resampling of the N weights to ``n_out`` offspring, t_j = floor((j * W + u0) /
    n_out); W == 0: a_j = j mod N."""
    w = np.asarray(w, dtype=np.uint64)
    N, n_out = len(w), int(n_out)
    C = np.cumsum(w, dtype=np.uint64)
    W = int(C[-1])
    u0 = (int(r) * W) >> 32
    if W == 0:
        return (np.arange(n_out) % N).astype(np.int32), 0, 0
    t = np.array([(j * W + u0) // n_out for j in range(n_out)], dtype=np.uint64)
    return np.searchsorted(C, t, side="right").astype(np.int32), W, u0


def size_of(kbins, ntab, n_cap):
    ntab = np.asarray(ntab, dtype=np.uint32)
    return min(max(int(ntab[min(int(kbins), len(ntab) - 1)]), 1), int(n_cap))


def step(field, frame, cost_scale, step_len, poses, n_in, n_cap, motion, amp, seed, scan, ranges, fov, max_range, outside_cost, lut, shift,
         bins, ntab, sincos=mcl.numpy_sincos):
    """One slam2d_mcl_step_adaptive.  ``poses``: [n_cap or more, 3], of which the first N = min(max(n_in, 1), n_cap) are read.
    Dict of ``N``, ``moved`` [N, 3], ``cost``, ``w``, ``reference`` (the set A, ascending), ``kbins``, ``n_out``, ``ancestors``
    int32 [n_out], ``out`` [n_out, 3] and ``report`` uint64 [24]."""
    N = min(max(int(n_in), 1), int(n_cap))
    poses = np.asarray(poses, dtype=np.float64)[:N, :3].copy()
    ranges = np.asarray(ranges, dtype=np.float64)
    B = len(ranges)
    g = mcl.noise(N, seed, scan)
    moved = mcl.move(poses, motion, amp, g, *sincos(poses[:, 2].copy()))
    bc, bs = sincos(np.array([yard.beam_angles(th, fov, B) for th in moved[:, 2]]))
    cost, in_range = mcl.costs(field, frame, cost_scale, step_len, moved, ranges, fov, max_range, outside_cost, bc, bs)
    w, cmin, best = mcl.weights(cost, lut, shift)
    r = mcl.resample_word(seed, scan)
    ref = reference_ancestors(w, r)
    kbins = len(np.unique(bins_of(moved[ref], bins)))
    n_out = size_of(kbins, ntab, n_cap)
    anc, W, u0 = resample_to(w, r, n_out)
    rep = np.zeros(REPORT, dtype=np.uint64)
    rep[:16] = mcl.report(cost, w, W, u0, in_range, moved, anc, *sincos(moved[:, 2].copy()))
    rep[16], rep[17], rep[18], rep[19] = N, n_out, kbins, len(ref)
    return dict(N=N, moved=moved, cost=cost, w=w, reference=ref, kbins=kbins, n_out=n_out, ancestors=anc, out=moved[anc], report=rep)
