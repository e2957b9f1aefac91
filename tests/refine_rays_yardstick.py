"""The definition of slam2d_refine_poses_rays (include/slam2d.h) in NumPy, for the tests, composed from tests/refine_yardstick.py
(move, candidates, endpoint costs, pack), tests/mcl_rays_yardstick.py (``through_mask`` -- which beams are CAST, CHECKED, kend and
the HIT -- and ``charged``) and, through it, tests/rays_yardstick.py's ``walk``: the ray sample by sample, NO skipping.  Written
here: the THROUGH count of every candidate of a moved seed, the charged words and the winner's count.  ``occ`` is the occupied image
[fh, fw] (bool) of the slot; the other arguments are ``refine_yardstick``'s.  ``refine`` takes the same ``sincos`` hook and asks it
for the same angles in the same order: the seeds' headings (only with a motion), then the beam angles of every seed's candidate
headings."""
import numpy as np

import mcl_rays_yardstick as mclr
import refine_yardstick as ryard


def through(occ, frame, step, seed, radii, steps, ranges, max_range, stride, phase, margin, cos, sin):
    """int64 [nth, ny, nx]: the THROUGH beams of every candidate of the moved ``seed``.  ``cos`` / ``sin``: [nth, beams] tables of
    ``refine_yardstick.beam_angles`` -- a candidate's ray runs along its heading's own a_b."""
    C = ryard.candidates(seed, radii, steps)
    nth, ny, nx = C.shape[:3]
    per = ny * nx
    mask = mclr.through_mask(occ, frame, step, C.reshape(-1, 3), np.asarray(ranges, dtype=np.float64), max_range, stride, phase, margin,
                             np.repeat(np.asarray(cos), per, axis=0), np.repeat(np.asarray(sin), per, axis=0))
    return mask.sum(axis=1).astype(np.int64).reshape(nth, ny, nx)


def costs(occ, field, frame, cost_scale, step, seed, radii, steps, ranges, fov, max_range, outside_cost, stride, phase, margin, through_cost,
          cos, sin):
    """(charged cost uint64, through int64, endpoint cost uint64) of the moved seed's candidates, each [nth, ny, nx]."""
    ends = ryard.costs(field, frame, cost_scale, step, seed, radii, steps, ranges, fov, max_range, outside_cost, cos, sin)[0]
    thr = through(occ, frame, step, seed, radii, steps, ranges, max_range, stride, phase, margin, cos, sin)
    return mclr.charged(ends, thr, through_cost), thr, ends


def refine(occ, field, frame, cost_scale, step, seeds, radii, steps, ranges, fov, max_range, outside_cost, stride, phase, margin, through_cost,
           motion=None, sincos=ryard.mcl.numpy_sincos):
    """One slam2d_refine_poses_rays: (words uint64 [N, 2], poses [N, 3], through int64 [N] of the winners).  ``ranges``: [beams] (one
    scan for all seeds) or [N, beams]."""
    seeds = np.array(seeds, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    moved = ryard.move(seeds, motion) if motion is None else ryard.move(seeds, motion, *sincos(seeds[:, 2].copy()))
    beams = ranges.shape[-1]
    bc, bs = sincos(np.array([ryard.beam_angles(m, radii, steps, fov, beams) for m in moved]))           # [N, nth, beams]
    words = np.empty((len(seeds), 2), dtype=np.uint64)
    poses = np.empty((len(seeds), 3))
    thr = np.empty(len(seeds), dtype=np.int64)
    for n, m in enumerate(moved):
        cost, t, _ = costs(occ, field, frame, cost_scale, step, m, radii, steps, ranges if ranges.ndim == 1 else ranges[n], fov, max_range,
                           outside_cost, stride, phase, margin, through_cost, bc[n], bs[n])
        words[n] = ryard.pack(cost)
        f = int(ryard.index_of(words[n])[0])
        poses[n] = ryard.candidates(m, radii, steps).reshape(-1, 3)[f]
        thr[n] = t.reshape(-1)[f]
    return words, poses, thr


def refine_stages(occ, field, frame, cost_scale, step, seeds, stages, ranges, fov, max_range, outside_cost, stride, phase, margin, through_cost,
                  motion=None, sincos=ryard.mcl.numpy_sincos):
    """The stages chained, the motion in the first, one phase for all: (words uint64 [N, stages, 2], poses [N, 3], through int64
    [N, stages])."""
    poses = np.array(seeds, dtype=np.float64).reshape(-1, 3)
    words, thr = [], []
    for i, (radii, steps) in enumerate(stages):
        w, poses, t = refine(occ, field, frame, cost_scale, step, poses, radii, steps, ranges, fov, max_range, outside_cost, stride, phase,
                             margin, through_cost, motion if i == 0 else None, sincos)
        words.append(w)
        thr.append(t)
    return np.stack(words, axis=1), poses, np.stack(thr, axis=1)


def pruning_share(cost, ends):
    """The share of a seed's candidates that exact pruning would still cast: those whose endpoint word is at most the charged minimum."""
    idx = np.arange(cost.size, dtype=np.uint64)
    charged_min = ((cost.reshape(-1) << np.uint64(ryard.INDEX_BITS)) | idx).min()
    return float((((ends.reshape(-1) << np.uint64(ryard.INDEX_BITS)) | idx) <= charged_min).mean())
