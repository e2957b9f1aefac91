#!/usr/bin/env python3
"""Time slam2d_refine_poses_rays on the device against slam2d_refine_poses in the same build, a Tracker with and without ``rays``
over a log, and the existing refinement calls of any build of the library (profiles/r27_refine_rays.md).

    python tools/refine_rays_time.py [--out FILE] [--seeds N ...] [--strides S ...]
    python tools/refine_rays_time.py --existing [--lib PATH] [--out FILE]
    python tools/refine_rays_time.py --pruning                  (no GPU: the yardstick on the room of tests/test_mcl_rays_host.py)

The world, lidar (180 beams over pi, 4 m) and 40-scan log of examples/localise.py, a Tracker's own covering level of its window (a
289 x 289 blurred field) and the squared distances it keeps with ``rays``.  For N = 1, 4 096 and 65 536 seeds about the walk's
first pose (up to 0.25 m and 0.05 rad off, its scan for all of them) and the default stages (729 + 125 candidates per seed), the
device time of both stages of slam2d_refine_poses and of slam2d_refine_poses_rays at strides 1, 4 and 8 (phase 0, the default
margin, through_cost = stride * outside_cost within 32 bits, d_through wanted), stage 2 from stage 1's poses on the device.
Device times are from HIP events (slam2d_timer_*) around blocks of back-to-back calls of about 0.1 s in one process, a warm-up
block first, the median of seven blocks with their range; a call of more than 0.3 s is timed as three blocks of one call.  Then
Tracker.run with and without ``rays`` over the 40 scans, wall time per scan end to end, the median of seven runs after a warm-up.
--existing times slam2d_refine_poses and slam2d_refine_points alone -- symbols every build has -- in the library at PATH (default:
this tree's): run it on the parent's build twice and on this build once, in one session, and compare the spreads.
Prints one JSON line per measurement.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "examples"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
NEW = ("slam2d_refine_rays_work", "slam2d_refine_poses_rays")


def timed(L, call, engine):
    """(median, min, max, calls per block) ms per call of ``call(stream)``: ``search_lattice_time.timed_blocks``, or -- a call of
    more than 0.3 s -- three blocks of one call after the first."""
    from search_lattice_time import timed_blocks
    timer = L.slam2d_timer_create()
    s = engine._stream()
    _lib.check(L.slam2d_timer_start(timer, s), "timer")
    call(s)
    _lib.check(L.slam2d_timer_stop(timer, s), "timer")
    ms = C.c_float()
    _lib.check(L.slam2d_timer_elapsed_ms(timer, C.byref(ms)), "timer")
    if ms.value <= 300.0:
        L.slam2d_timer_destroy(timer)
        return timed_blocks(L, call, 1e-3)
    t = []
    for _ in range(3):
        _lib.check(L.slam2d_timer_start(timer, s), "timer")
        call(s)
        _lib.check(L.slam2d_timer_stop(timer, s), "timer")
        _lib.check(L.slam2d_timer_elapsed_ms(timer, C.byref(ms)), "timer")
        t.append(ms.value)
    L.slam2d_timer_destroy(timer)
    t.sort()
    return t[1], t[0], t[2], 1


def scene(pkg, rays):
    import localise
    true, log, grid, window = localise.synthetic(40)
    og = pkg.map_from_poses(true, **grid)
    sm = pkg.ScanMatcher(og, *localise.SM_PARAMS)
    tr = pkg.Tracker(sm, window, rays=rays)
    walk = np.array([[r["x"], r["y"], r["theta"]] for r in true])
    scans = np.array([r["range"] for r in true], dtype=np.float64)
    return true, log, window, og, sm, tr, walk, scans


def measure(N, tr, walk, scans, strides, emit):
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
    L, eng, lv = _lib.lib(), tr.eng, tr.level
    stages = matcher.default_stages(lv.step)
    outside = tr.outside_cost
    B = scans.shape[1]
    rs = np.random.RandomState(N)
    seeds = walk[0] + rs.uniform(-1, 1, (N, 3)) * (0.25, 0.25, 0.05)
    d_seed = eng.to_device(seeds)
    d_pose = [d_seed.clone(), torch.empty((N, 3), dtype=torch.float64, device=eng.device)]
    d_rng = eng.to_device(scans[0])
    work = torch.empty(L.slam2d_refine_work(N), dtype=torch.int64, device=eng.device)
    words = torch.empty((len(stages), N, 2), dtype=torch.int64, device=eng.device)
    thr = torch.empty((len(stages), N), dtype=torch.int32, device=eng.device)
    margin = matcher.ray_margin(tr.matcher.og.wallThickness, lv.step)

    def plain(s):
        for i, (radii, steps) in enumerate(stages):
            _lib.check(L.slam2d_refine_poses(C.byref(eng.lidar_c), C.byref(lv.c), 0, N, d_pose[i & 1].data_ptr(), d_pose[1 - (i & 1)].data_ptr(), 3,
                                             d_rng.data_ptr(), 0, None, *radii, *steps, outside, work.data_ptr(), words[i].data_ptr(), s),
                       "slam2d_refine_poses")

    def charged(stride):
        def call(s):
            for i, (radii, steps) in enumerate(stages):
                _lib.check(L.slam2d_refine_poses_rays(C.byref(eng.lidar_c), C.byref(lv.c), 0, tr.d_dist2.data_ptr(), N, d_pose[i & 1].data_ptr(),
                                                      d_pose[1 - (i & 1)].data_ptr(), 3, d_rng.data_ptr(), 0, None, *radii, *steps, outside, stride, 0,
                                                      margin, min(stride * outside, 2 ** 32 - 1), thr[i].data_ptr(), work.data_ptr(),
                                                      words[i].data_ptr(), s), "slam2d_refine_poses_rays")
        return call

    per = [int(np.prod([2 * r + 1 for r in radii])) for radii, _ in stages]
    common = dict(N=N, beams=B, candidates=per, margin=margin)
    med, lo, hi, calls = timed(L, plain, engine)
    base = med
    emit(dict(what="slam2d_refine_poses, both stages", **common, calls_per_block=calls, ms_per_call=round(med, 5), ms_min=round(lo, 5),
              ms_max=round(hi, 5)))
    torch.cuda.synchronize()
    plain_words = words.clone()
    for stride in strides:
        d_pose[0].copy_(d_seed)
        med, lo, hi, calls = timed(L, charged(stride), engine)
        torch.cuda.synchronize()
        moved = int((words[0, :, 0] != plain_words[0, :, 0]).sum())
        emit(dict(what="slam2d_refine_poses_rays, both stages", **common, stride=stride, cast_beams=len(range(0, B, stride)), calls_per_block=calls,
                  ms_per_call=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5), times_the_plain_call=round(med / base, 2),
                  seeds_whose_first_word_changed=moved, through_mean=[round(float(thr[i].double().mean()), 3) for i in range(len(stages))]))


def track(pkg, sm, window, true, log, stride, emit):
    def wall(f, n=7):
        f()                                                    # warm-up
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(1e3 * (time.perf_counter() - t0) / len(log))
        ts.sort()
        return [round(v, 4) for v in (ts[len(ts) // 2], ts[0], ts[-1])]

    start = (true[0]["x"], true[0]["y"], true[0]["theta"])
    out = {}
    res = {}
    for name, rays in (("plain", None), ("rays", dict(stride=stride))):
        tr = pkg.Tracker(sm, window, rays=rays)

        def run():
            tr.set_pose(start)
            tr.scan = 0
            out[name] = tr.run(log)
        res[name] = wall(run)
    err = lambda reps: [float(np.hypot(r.pose[0] - t["x"], r.pose[1] - t["y"])) for r, t in zip(reps, true)]
    ep, er = err(out["plain"]), err(out["rays"])
    emit(dict(what="Tracker.run end to end, wall ms per scan (median, min, max of 7 runs)", scans=len(log), stride=stride,
              plain_ms_per_scan=res["plain"], rays_ms_per_scan=res["rays"],
              plain_error_m=dict(mean=round(float(np.mean(ep)), 4), max=round(max(ep), 4)),
              rays_error_m=dict(mean=round(float(np.mean(er)), 4), max=round(max(er), 4)),
              through_last_stage_sum=int(sum(int(r.through[-1]) for r in out["rays"]))))


def existing(pkg, emit, seeds):
    """slam2d_refine_poses and slam2d_refine_points, both default stages, in whatever build is loaded."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
    points = importlib.import_module("slam-2d-lidar-scan_amd.points")
    true, log, window, og, sm, tr, walk, scans = scene(pkg, None)
    L, eng, lv = _lib.lib(), tr.eng, tr.level
    stages = matcher.default_stages(lv.step)
    pts = points.scan_points(scans[0], og.lidarFOV, og.lidarMaxRange)
    pts = np.ascontiguousarray(pts[np.isfinite(pts).all(axis=1)])
    for N in seeds:
        rs = np.random.RandomState(N)
        d_pose = [eng.to_device(walk[0] + rs.uniform(-1, 1, (N, 3)) * (0.25, 0.25, 0.05)), torch.empty((N, 3), dtype=torch.float64, device=eng.device)]
        d_rng, d_pts = eng.to_device(scans[0]), eng.to_device(pts)
        work = torch.empty(L.slam2d_refine_work(N), dtype=torch.int64, device=eng.device)
        words = torch.empty((len(stages), N, 2), dtype=torch.int64, device=eng.device)

        def scan_form(s):
            for i, (radii, steps) in enumerate(stages):
                _lib.check(L.slam2d_refine_poses(C.byref(eng.lidar_c), C.byref(lv.c), 0, N, d_pose[i & 1].data_ptr(), d_pose[1 - (i & 1)].data_ptr(), 3,
                                                 d_rng.data_ptr(), 0, None, *radii, *steps, tr.outside_cost, work.data_ptr(), words[i].data_ptr(), s),
                           "slam2d_refine_poses")

        def point_form(s):
            for i, (radii, steps) in enumerate(stages):
                _lib.check(L.slam2d_refine_points(C.byref(lv.c), 0, N, d_pose[i & 1].data_ptr(), d_pose[1 - (i & 1)].data_ptr(), 3, d_pts.data_ptr(), 2,
                                                  len(pts), 0, None, *radii, *steps, tr.outside_cost, work.data_ptr(), words[i].data_ptr(), s),
                           "slam2d_refine_points")

        for what, call in (("slam2d_refine_poses, both stages", scan_form), ("slam2d_refine_points, both stages", point_form)):
            med, lo, hi, calls = timed(L, call, engine)
            emit(dict(what=what, lib=_lib.LIB_PATH, N=N, calls_per_block=calls, ms_per_call=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5)))


def pruning(emit):
    """What exact pruning would leave to cast, on the yardstick: the share of a seed's candidates whose endpoint word is at most the
    charged minimum, for seeds about the two poses of tests/test_mcl_rays_host.py's room and the default stages' first lattice."""
    import distance_yardstick as dyard
    import rays_yardstick as rays
    import refine_rays_yardstick as rr
    import refine_yardstick as ryard
    from test_mcl_rays_host import BEAMS, BEHIND, FOV, FRAME, FRONT, MARGIN, R, STEP
    occ = np.zeros((40, 40), dtype=bool)
    occ[:, 20:22] = True
    field = dyard.field_from(occ, np.array([0, 1000, 2000, 3000], dtype=np.uint32)).astype(np.uint32)
    words = rays.cast(occ, FRAME, STEP, (FOV, BEAMS, R), np.array([FRONT]), 29)[0]
    ranges = np.where(words >> np.uint32(30) == rays.HIT, (words & np.uint32(0x3fffffff)) * STEP, R)
    radii, steps = (4, 4, 4), (STEP, STEP, 0.02)
    rs = np.random.RandomState(1)
    for name, at in (("front", FRONT), ("behind", BEHIND)):
        shares = []
        for _ in range(8):
            seed = np.array(at) + rs.uniform(-1, 1, 3) * (0.25, 0.25, 0.05)
            c, s = ryard.mcl.numpy_sincos(ryard.beam_angles(seed, radii, steps, FOV, BEAMS))
            cost, _, ends = rr.costs(occ, field, FRAME, 1.0, STEP, seed, radii, steps, ranges, FOV, R, 3000, 4, 0, MARGIN, 4 * 3000, c, s)
            shares.append(rr.pruning_share(cost, ends))
        emit(dict(what="share of candidates exact pruning would still cast", seeds_about=name, candidates=729, stride=4,
                  mean=round(float(np.mean(shares)), 4), min=round(min(shares), 4), max=round(max(shares), 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 4096, 65536])
    ap.add_argument("--strides", type=int, nargs="*", default=[1, 4, 8])
    ap.add_argument("--existing", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--pruning", action="store_true")
    args = ap.parse_args()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.pruning:
        return pruning(emit)
    if args.lib:
        if not args.existing:
            ap.error("--lib goes with --existing")
        _lib.LIB_PATH = os.path.abspath(args.lib)
        for name in NEW:                                       # (a build from before this call exports neither)
            _lib.SIGNATURES.pop(name, None)
    import torch
    pkg = importlib.import_module("slam-2d-lidar-scan_amd")
    if args.existing:
        return existing(pkg, emit, args.seeds)
    true, log, window, og, sm, tr, walk, scans = scene(pkg, dict(stride=4))
    fr = tr.level.frames()[0]
    emit(dict(what="scene", field=[int(fr["fh"]), int(fr["fw"])], beams=scans.shape[1],
              in_range_mean=round(float((scans < og.lidarMaxRange).sum(axis=1).mean()), 1), device=torch.cuda.get_device_name(0)))
    for N in args.seeds:
        measure(N, tr, walk, scans, args.strides, emit)
    track(pkg, sm, window, true, log, 4, emit)


if __name__ == "__main__":
    main()
