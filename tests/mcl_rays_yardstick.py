"""The definitions of slam2d_mcl_step_rays and slam2d_mcl_step_adaptive_rays (include/slam2d.h) in NumPy, for the tests, composed
from tests/mcl_yardstick.py (noise, move, endpoint costs, weights, resampler, report), tests/mcl_adapt_yardstick.py (reference
ancestors, bins, the table's count) and tests/rays_yardstick.py (``walk`` -- the ray sample by sample, NO skipping --,
``beam_limits``).  Written here: which beams are CAST, the per-beam THROUGH mask of the moved poses, the charge and word 15.
``occ`` is the occupied image [fh, fw] (bool) of the slot; the other arguments are the plain yardsticks'.  ``step`` and
``step_adaptive`` take the same ``sincos`` hook as ``mcl_yardstick.step`` and ask it for the same three sets of angles in the same
order: the headings of the poses, the beam angles of the moved poses, the headings of the moved poses."""
import numpy as np

import mcl_adapt_yardstick as adapt
import mcl_yardstick as mcl
import rays_yardstick as rays
import score_yardstick as yard


def cast_beams(beams, stride, phase):
    """The CAST beams, ascending: b % stride == phase."""
    b = np.arange(int(beams), dtype=np.int64)
    return b[b % int(stride) == int(phase)]


def through_mask(occ, frame, step_len, moved, ranges, max_range, stride, phase, margin, cos, sin):
    """bool [N, beams]: beam b of moved pose n is THROUGH -- CAST, CHECKED, kend >= 0 and its ray HIT at some k <= kend.  ``cos`` /
    ``sin``: [N, beams] of the moved poses' beam angles."""
    moved = np.asarray(moved, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    out = np.zeros((len(moved), len(ranges)), dtype=bool)
    cast = cast_beams(len(ranges), stride, phase)
    if not len(cast):
        return out
    c, s = np.asarray(cos, dtype=np.float64)[:, cast], np.asarray(sin, dtype=np.float64)[:, cast]
    _, kend = rays.beam_limits(np.broadcast_to(ranges[cast], c.shape), step_len, max_range, margin)
    kind, _ = rays.walk(occ, frame, step_len, moved[:, 0:1], moved[:, 1:2], c, s, kend)      # (a HIT lies at k <= its limit, kend)
    out[:, cast] = (kend >= 0) & (kind == rays.HIT)
    return out


def charged(cost, through, through_cost):
    """cost_n + through_n * through_cost (uint64)."""
    return np.asarray(cost, dtype=np.uint64) + np.asarray(through, dtype=np.uint64) * np.uint64(through_cost)


def _weigh(occ, field, frame, cost_scale, step_len, poses, motion, amp, seed, scan, ranges, fov, max_range, outside_cost, stride, phase, margin,
           through_cost, sincos):
    """Steps a-c over ``poses``: (moved, cost with the charge, in_range, through [N])."""
    N, B = len(poses), len(ranges)
    g = mcl.noise(N, seed, scan)
    moved = mcl.move(poses, motion, amp, g, *sincos(poses[:, 2].copy()))
    bc, bs = sincos(np.array([yard.beam_angles(th, fov, B) for th in moved[:, 2]]))
    cost, in_range = mcl.costs(field, frame, cost_scale, step_len, moved, ranges, fov, max_range, outside_cost, bc, bs)
    through = through_mask(occ, frame, step_len, moved, ranges, max_range, stride, phase, margin, bc, bs).sum(axis=1).astype(np.int64)
    return moved, charged(cost, through, through_cost), in_range, through


def step(occ, field, frame, cost_scale, step_len, poses, motion, amp, seed, scan, ranges, fov, max_range, outside_cost, stride, phase, margin,
         through_cost, lut, shift, sincos=mcl.numpy_sincos):
    """One slam2d_mcl_step_rays: ``mcl_yardstick.step``'s dict on the charged cost, ``through`` int64 [N] of the MOVED particles,
    and word 15 of ``report`` = their sum."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    moved, cost, in_range, through = _weigh(occ, field, frame, cost_scale, step_len, poses, motion, amp, seed, scan, ranges, fov, max_range,
                                            outside_cost, stride, phase, margin, through_cost, sincos)
    w, cmin, best = mcl.weights(cost, lut, shift)
    anc, W, u0 = mcl.resample(w, mcl.resample_word(seed, scan))
    rep = mcl.report(cost, w, W, u0, in_range, moved, anc, *sincos(moved[:, 2].copy()))
    rep[15] = int(through.sum())
    return dict(moved=moved, cost=cost, w=w, ancestors=anc, out=moved[anc], report=rep, through=through)


def step_adaptive(occ, field, frame, cost_scale, step_len, poses, n_in, n_cap, motion, amp, seed, scan, ranges, fov, max_range, outside_cost,
                  stride, phase, margin, through_cost, lut, shift, bins, ntab, sincos=mcl.numpy_sincos):
    """One slam2d_mcl_step_adaptive_rays: ``mcl_adapt_yardstick.step``'s dict on the charged cost, ``through`` int64 [N] over the
    N live particles, and word 15 = their sum."""
    N = min(max(int(n_in), 1), int(n_cap))
    poses = np.asarray(poses, dtype=np.float64)[:N, :3].copy()
    ranges = np.asarray(ranges, dtype=np.float64)
    moved, cost, in_range, through = _weigh(occ, field, frame, cost_scale, step_len, poses, motion, amp, seed, scan, ranges, fov, max_range,
                                            outside_cost, stride, phase, margin, through_cost, sincos)
    w, cmin, best = mcl.weights(cost, lut, shift)
    r = mcl.resample_word(seed, scan)
    ref = adapt.reference_ancestors(w, r)
    kbins = len(np.unique(adapt.bins_of(moved[ref], bins)))
    n_out = adapt.size_of(kbins, ntab, n_cap)
    anc, W, u0 = adapt.resample_to(w, r, n_out)
    rep = np.zeros(adapt.REPORT, dtype=np.uint64)
    rep[:16] = mcl.report(cost, w, W, u0, in_range, moved, anc, *sincos(moved[:, 2].copy()))
    rep[15] = int(through.sum())
    rep[16], rep[17], rep[18], rep[19] = N, n_out, kbins, len(ref)
    return dict(N=N, moved=moved, cost=cost, w=w, reference=ref, kbins=kbins, n_out=n_out, ancestors=anc, out=moved[anc], report=rep,
                through=through)
