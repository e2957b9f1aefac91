"""The definition of slam2d_mcl_step (include/slam2d.h) in NumPy, for the tests, built on tests/score_yardstick.py: Philox4x32-10,
the Irwin-Hall noise, the move, the cost of slam2d_search_lattice, the integer weights, the integer systematic resampler and the
sixteen report words.  Every operation is an integer one or one rounded IEEE operation at a time, so the device's bits are
these bits; the products k * W and r * W are Python integers.  Cosines and sines are optional arguments, as in the other
yardsticks: ``step`` takes a ``sincos`` function (angles -> (cos, sin)) and asks it for the headings of the poses, the beam
angles of the moved poses and the headings of the moved poses, in that order."""
import math

import numpy as np

import score_yardstick as yard

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
MAX_WEIGHT = 0xffffff
REPORT = 16


def philox(counter, key):
    """Philox4x32-10.  ``counter``: four words (scalars or arrays that broadcast), ``key``: two; returns uint32 [..., 4]."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = (int(v) & 0xffffffff for v in key)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]    # (32 x 32 bits: exact in 64)
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return np.stack(c, axis=-1).astype(np.uint32)


def split(v):
    v = int(v) & 0xffffffffffffffff
    return v & 0xffffffff, v >> 32


def noise(N, seed, scan, draws=(0, 1, 2)):
    """g [N, len(draws)]: draw j of particle n is the sum of the four words of counter (n, j, scan) as int32, times 2^-31."""
    n = np.arange(N, dtype=np.uint64).reshape(-1, 1)
    j = np.asarray(draws, dtype=np.uint64).reshape(1, -1)
    out = philox((n, j, split(scan)[0], split(scan)[1]), split(seed))
    S = out.view(np.int32).astype(np.int64).sum(axis=-1)
    return S.astype(np.float64) * 2.0 ** -31


def resample_word(seed, scan):
    return int(philox((0xffffffff, 0, split(scan)[0], split(scan)[1]), split(seed))[0])


def move(poses, motion, amp, g, cos=None, sin=None):
    """The moved poses [N, 3]: each product and sum rounded, in the header's order.  ``cos`` / ``sin``: None or [N], of the headings."""
    p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    x, y, th = p[:, 0], p[:, 1], p[:, 2]
    dfwd, dside, dturn = (np.float64(v) for v in motion)
    a0, a1, a2 = (np.float64(v) for v in amp)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = dfwd + a0 * g[:, 0]
        fy = dside + a1 * g[:, 1]
        c = np.cos(th) if cos is None else np.asarray(cos, dtype=np.float64)
        s = np.sin(th) if sin is None else np.asarray(sin, dtype=np.float64)
        nx = (x + c * fx) - s * fy
        ny = (y + s * fx) + c * fy
        nth = (th + dturn) + a2 * g[:, 2]
    return np.stack([nx, ny, nth], axis=1)


def costs(field, frame, cost_scale, step_len, moved, ranges, fov, max_range, outside_cost, cos=None, sin=None):
    """(cost uint64 [N], in_range): sum_b + (in_range - inside) * outside_cost of slam2d_score_poses' rows at the moved poses."""
    rows = yard.score_poses(field, frame, cost_scale, step_len, moved, np.asarray(ranges, dtype=np.float64), fov, max_range, cos, sin)
    sum_b = rows[:, 6].astype(np.uint64)                       # (below 2^53: exact in the double)
    inside, in_range = rows[:, 3].astype(np.int64), rows[:, 4].astype(np.int64)
    return sum_b + (in_range - inside).astype(np.uint64) * np.uint64(outside_cost), int(in_range[0])


def weights(cost, lut, shift):
    """(w uint64 [N], cmin, best): the table's weight of every cost above the minimum; best is the lowest index of the minimum."""
    cost = np.asarray(cost, dtype=np.uint64)
    lut = np.asarray(lut, dtype=np.uint32)
    cmin = cost.min()
    idx = np.minimum((cost - cmin) >> np.uint64(shift), np.uint64(len(lut) - 1)).astype(np.int64)
    return np.minimum(lut[idx].astype(np.uint64), np.uint64(MAX_WEIGHT)), int(cmin), int(np.argmin(cost))


def resample(w, r):
    """(ancestors int32 [N], W, u0): systematic resampling in integers; W == 0: the identity."""
    w = np.asarray(w, dtype=np.uint64)
    N = len(w)
    C = np.cumsum(w, dtype=np.uint64)
    W = int(C[-1])
    u0 = (int(r) * W) >> 32
    assert u0 == (W >> 32) * int(r) + (((W & 0xffffffff) * int(r)) >> 32)
    if W == 0:
        return np.arange(N, dtype=np.int32), 0, 0
    t = np.array([(k * W + u0) // N for k in range(N)], dtype=np.uint64)       # (Python integers: k * W reaches 2^64)
    return np.searchsorted(C, t, side="right").astype(np.int32), W, u0          # the least n with t < C[n]


def report(cost, w, W, u0, in_range, moved, ancestors, cos=None, sin=None):
    """The sixteen words (uint64).  ``cos`` / ``sin``: None or [N], of the MOVED poses' headings."""
    rep = np.zeros(REPORT, dtype=np.uint64)
    best = int(np.argmin(cost))
    rep[0], rep[1], rep[2], rep[3], rep[4], rep[5] = cost.min(), best, W, int((np.asarray(w) > 0).sum()), u0, in_range
    rep[6] = len(np.unique(ancestors))
    rep[7:10] = moved[best].view(np.uint64)
    off = moved[ancestors]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(off[:, 0]) < 2.0 ** 20) & (np.abs(off[:, 1]) < 2.0 ** 20) & np.isfinite(off[:, 2])
        c = (np.cos(moved[:, 2]) if cos is None else np.asarray(cos, dtype=np.float64))[ancestors][ok]
        s = (np.sin(moved[:, 2]) if sin is None else np.asarray(sin, dtype=np.float64))[ancestors][ok]
    rep[10] = int(ok.sum())
    sums = [np.rint(off[ok, 0] * 65536.0), np.rint(off[ok, 1] * 65536.0), np.rint(c * 2.0 ** 30), np.rint(s * 2.0 ** 30)]
    rep[11:15] = np.array([v.astype(np.int64).sum(dtype=np.int64) for v in sums], dtype=np.int64).view(np.uint64)
    return rep


def numpy_sincos(angles):
    with np.errstate(invalid="ignore"):
        return np.cos(angles), np.sin(angles)


def step(field, frame, cost_scale, step_len, poses, motion, amp, seed, scan, ranges, fov, max_range, outside_cost, lut, shift,
         sincos=numpy_sincos):
    """One slam2d_mcl_step: dict of ``moved`` [N, 3], ``cost``, ``w``, ``ancestors`` int32 [N], ``out`` [N, 3] (the resampled
    set) and ``report`` uint64 [16]."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    N, B = len(poses), len(ranges)
    g = noise(N, seed, scan)
    moved = move(poses, motion, amp, g, *sincos(poses[:, 2].copy()))
    bc, bs = sincos(np.array([yard.beam_angles(th, fov, B) for th in moved[:, 2]]))
    cost, in_range = costs(field, frame, cost_scale, step_len, moved, ranges, fov, max_range, outside_cost, bc, bs)
    w, cmin, best = weights(cost, lut, shift)
    anc, W, u0 = resample(w, resample_word(seed, scan))
    rep = report(cost, w, W, u0, in_range, moved, anc, *sincos(moved[:, 2].copy()))
    return dict(moved=moved, cost=cost, w=w, ancestors=anc, out=moved[anc], report=rep)


def mean_pose(rep):
    """(x, y, theta) of report words 10-14; NaNs where no offspring counts."""
    rep = np.asarray(rep, dtype=np.uint64)
    M = int(rep[10])
    sx, sy, sc, ss = (int(v) for v in rep[11:15].view(np.int64))
    if M == 0:
        return (float("nan"),) * 3
    return sx / (65536.0 * M), sy / (65536.0 * M), math.atan2(float(ss), float(sc))
