"""The definition of slam2d_field_build_distance (include/slam2d.h) in NumPy alone: the squared Euclidean distance, in cells,
from every cell of an image to its nearest occupied cell, clamped at a cap, and the field a table makes of it.  Integers
throughout; the tests compare with np.array_equal.

``dist2`` is the separable form the header describes (a column pass by running maxima and minima of the occupied row index, a
row pass as a loop over offsets of whole-array minima); ``all_pairs`` is the definition itself, for small images.
``likelihood_table`` restates engine.likelihood_table."""
import math

import numpy as np

FAR = 1 << 40                                                  # an index no image reaches


def reach(cap):
    """R = ceil(sqrt(cap)): a result below the cap has its wall fewer than R rows and fewer than R columns away."""
    r = math.isqrt(int(cap))
    return r if r * r == cap else r + 1


def column_pass(occ, R):
    """g [fh, fw] int64: rows from a cell to the nearest occupied cell of its column, saturated at R + 1."""
    occ = np.asarray(occ, dtype=bool)
    rows = np.arange(occ.shape[0], dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(occ, rows, -FAR), axis=0)             # the last occupied row at or above
    below = np.minimum.accumulate(np.where(occ, rows, FAR)[::-1], axis=0)[::-1]      # the first at or below
    return np.minimum(np.minimum(rows - above, below - rows), R + 1)


def dist2(occ, cap):
    """k [fh, fw] int64 = min(cap, min over occupied (a, b) of (a - i)^2 + (b - j)^2); the cap where nothing is occupied."""
    occ = np.asarray(occ, dtype=bool)
    cap = int(cap)
    R = reach(cap)
    g2 = column_pass(occ, R) ** 2
    fw = occ.shape[1]
    best = np.full(occ.shape, cap, dtype=np.int64)
    for o in range(-R, R + 1):
        lo, hi = max(0, -o), min(fw, fw - o)                   # columns j with 0 <= j + o < fw
        if lo < hi:
            best[:, lo:hi] = np.minimum(best[:, lo:hi], o * o + g2[:, lo + o:hi + o])
    return best


def all_pairs(occ, cap):
    """The same by the definition: every cell against every occupied cell."""
    occ = np.asarray(occ, dtype=bool)
    a, b = np.nonzero(occ)
    out = np.full(occ.shape, int(cap), dtype=np.int64)
    for i in range(occ.shape[0]):
        for j in range(occ.shape[1]):
            if len(a):
                out[i, j] = min(int(cap), int(((a - i) ** 2 + (b - j) ** 2).min()))
    return out


def field_from(occ, lut):
    """The field of the call: lut[k], k clamped at len(lut) - 1."""
    lut = np.asarray(lut)
    return lut[dist2(occ, len(lut) - 1)]


def cost_scale_for(c_max):
    """engine.cost_scale_for(-c_max) for a finite c_max > 0: 2^k, k <= 31, with c_max * 2^k < 2^32."""
    return float(2.0 ** min(31, int(math.floor(math.log2(4294967295.0 / c_max)))))


def likelihood_table(step, sigma, z_hit=0.95, z_rand=0.05, max_dist=None, limit=65536):
    """(lut uint32 [n], cost_scale): lut[i] = rint(cost(i) * cost_scale), cost(i) = log(z_hit + z_rand) - log(z_hit *
    exp(-(i * step^2) / (2 sigma^2)) + z_rand); n the least length >= 2 whose last entry is rint(c_max * cost_scale), c_max =
    log(z_hit + z_rand) - log(z_rand); with max_dist at most floor((max_dist / step)^2) + 2, the last entry forced."""
    c_max = math.log(z_hit + z_rand) - math.log(z_rand)
    scale = cost_scale_for(c_max)
    saturated = np.rint(c_max * scale)
    longest = limit + 1 if max_dist is None else min(limit + 1, math.floor((max_dist / step) ** 2) + 2)
    i = np.arange(longest, dtype=np.float64)
    lut = np.rint((math.log(z_hit + z_rand) - np.log(z_hit * np.exp(-(i * (step * step)) / (2.0 * sigma * sigma)) + z_rand)) * scale)
    n = next((k + 1 for k in range(1, longest) if lut[k] == saturated), longest)
    if n > limit:
        raise ValueError("too long")
    lut = lut[:n].copy()
    lut[-1] = saturated
    return lut.astype(np.uint32), scale
