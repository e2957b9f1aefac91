#!/usr/bin/env python3
"""Time slam2d_search_points against slam2d_search_lattice and slam2d_refine_points against slam2d_refine_poses on the device, in
one build and one process (profiles/r21_points.md).

    python tools/points_time.py [--out FILE]

The mapped synthetic world, lidar (180 beams over pi, 4 m), window and lattice of examples/relocalise.py -- 161 x 161 positions x
120 headings over the matcher's fine covering level, full field build:
  * the search of one scan by slam2d_search_lattice, and of the same scan as points (points.scan_points: M = 180 rows, the beams
    out of range NaN) by slam2d_search_points;
  * the same two at ONE position (1 x 1 x 120: the table launch and a search of fifteen blocks -- what the tables cost);
  * slam2d_search_points of the last four scans merged through the odometry (points.merge_scans);
  * both stages of the default refinement by slam2d_refine_poses and by slam2d_refine_points, N = 1, 4 096 and 65 536 seeds about
    the scan's pose.
Device times are from HIP events (slam2d_timer_*) around blocks of back-to-back calls of about 0.1 s.  The two forms of a pair
take turns block by block -- a warm-up block each, then seven of each --: the median with its range, which is the run-to-run
spread the comparison has to be read against.  Prints one JSON line per measurement.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "examples")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
points = importlib.import_module("slam-2d-lidar-scan_amd.points")


def alternating_blocks(L, calls, blocks=7):
    """{name: (median, min, max, calls per block)} ms per call of every ``calls[name](stream)``: blocks of about 0.1 s, the names
    taking turns, one warm-up block of each first."""
    timer = L.slam2d_timer_create()
    s = engine._stream()

    def block(call, n):
        _lib.check(L.slam2d_timer_start(timer, s), "timer")
        for _ in range(n):
            call(s)
        _lib.check(L.slam2d_timer_stop(timer, s), "timer")
        ms = C.c_float()
        _lib.check(L.slam2d_timer_elapsed_ms(timer, C.byref(ms)), "timer")
        return ms.value / n

    per = {name: max(3, min(2000, int(100.0 / max(block(call, 3), 1e-3)))) for name, call in calls.items()}
    t = {name: [] for name in calls}
    for _ in range(blocks):
        for name, call in calls.items():
            t[name].append(block(call, per[name]))
    L.slam2d_timer_destroy(timer)
    return {name: (sorted(v)[len(v) // 2], min(v), max(v), per[name]) for name, v in t.items()}


def report(emit, what, res, **common):
    for name, (med, lo, hi, n) in res.items():
        emit(dict(what=what, call=name, **common, calls_per_block=n, ms_per_call=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seeds", type=int, nargs="*", default=[1, 4096, 65536])
    args = ap.parse_args()
    pkg = importlib.import_module("slam-2d-lidar-scan_amd")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import relocalise
    og, picks, window, log = relocalise.synthetic_log(pkg, 3)
    sm = pkg.ScanMatcher(og, *relocalise.SM_PARAMS)
    L = _lib.lib()
    r = picks[1]
    i = next(k for k, q in enumerate(log) if q is r)
    rng = np.asarray(r["range"], dtype=np.float64)
    sm.searchPoses(rng, window, step=0.1, headings=120)        # builds the covering level's field
    lv, lat, eng = sm.last_cover["level"], sm.last_cover["lattice"], og.engine()
    free = sm.outside_cost_of(lv)
    fr = lv.frames()[0]
    one = points.scan_points(rng, og.lidarFOV, og.lidarMaxRange)
    four, stride = points.merge_scans(log[i - 3:i + 1], fov=og.lidarFOV, max_range=og.lidarMaxRange)
    emit(dict(what="scene", field=[int(fr["fh"]), int(fr["fw"])], beams=len(rng), in_range=int((rng < og.lidarMaxRange).sum()),
              merged_points=len(four), merged_stride=stride, device=torch.cuda.get_device_name(0)))
    d_rng, d_one, d_four = eng.to_device(rng), eng.to_device(one), eng.to_device(four)
    work = torch.empty(2 * 120 * max(len(four), len(rng)), dtype=torch.int64, device=eng.device)
    out = {k: torch.empty((lat.ny, lat.nx), dtype=torch.int64, device=eng.device) for k in ("scan", "points", "merged")}

    def scan_search(nx, ny, x0, y0):
        return lambda s: _lib.check(L.slam2d_search_lattice(C.byref(eng.lidar_c), C.byref(lv.c), 0, nx, ny, lat.nth, x0, lat.dx, y0, lat.dy,
                                                            lat.th0, lat.dth, d_rng.data_ptr(), free, work.data_ptr(), out["scan"].data_ptr(), s),
                                    "slam2d_search_lattice")

    def points_search(nx, ny, x0, y0, d_pts, key):
        return lambda s: _lib.check(L.slam2d_search_points(C.byref(lv.c), 0, nx, ny, lat.nth, x0, lat.dx, y0, lat.dy, lat.th0, lat.dth,
                                                           d_pts.data_ptr(), 2, d_pts.shape[0], free, work.data_ptr(), out[key].data_ptr(), s),
                                    "slam2d_search_points")

    full = (lat.nx, lat.ny, lat.x0, lat.y0)
    res = alternating_blocks(L, {"slam2d_search_lattice": scan_search(*full), "slam2d_search_points, the same scan as points": points_search(*full, d_one, "points"),
                                 "slam2d_search_points, four scans merged": points_search(*full, d_four, "merged")})
    report(emit, "search, the lattice of examples/relocalise.py", res, lattice=[lat.nx, lat.ny, lat.nth], points=[len(rng), len(one), len(four)])
    differ = int((out["scan"] != out["points"]).sum().item())
    emit(dict(what="words that differ between the scan form and the same scan as points (two roundings apart off heading 0)", words=lat.nx * lat.ny,
              differ=differ, same_best_position=int(torch.argmin(out["scan"])) == int(torch.argmin(out["points"]))))
    mid = (1, 1, float(r["x"]), float(r["y"]))
    res = alternating_blocks(L, {"slam2d_search_lattice": scan_search(*mid), "slam2d_search_points, the same scan as points": points_search(*mid, d_one, "points"),
                                 "slam2d_search_points, four scans merged": points_search(*mid, d_four, "merged")})
    report(emit, "search at one position: the table launch and fifteen blocks", res, lattice=[1, 1, lat.nth], points=[len(rng), len(one), len(four)])

    stages = matcher.default_stages(lv.step)
    for N in args.seeds:
        rs = np.random.RandomState(N)
        seeds = np.array([r["x"], r["y"], r["theta"]]) + rs.uniform(-1, 1, (N, 3)) * (0.25, 0.25, 0.05)
        d_pose = [eng.to_device(seeds), torch.empty((N, 3), dtype=torch.float64, device=eng.device)]
        rwork = torch.empty(L.slam2d_refine_work(N), dtype=torch.int64, device=eng.device)
        words = torch.empty((len(stages), N, 2), dtype=torch.int64, device=eng.device)

        def refine_scan(s):
            for k, (radii, steps) in enumerate(stages):
                _lib.check(L.slam2d_refine_poses(C.byref(eng.lidar_c), C.byref(lv.c), 0, N, d_pose[k & 1].data_ptr(), d_pose[1 - (k & 1)].data_ptr(), 3,
                                                 d_rng.data_ptr(), 0, None, *radii, *steps, free, rwork.data_ptr(), words[k].data_ptr(), s),
                           "slam2d_refine_poses")

        def refine_pts(d_pts):
            def call(s):
                for k, (radii, steps) in enumerate(stages):
                    _lib.check(L.slam2d_refine_points(C.byref(lv.c), 0, N, d_pose[k & 1].data_ptr(), d_pose[1 - (k & 1)].data_ptr(), 3, d_pts.data_ptr(), 2,
                                                      d_pts.shape[0], 0, None, *radii, *steps, free, rwork.data_ptr(), words[k].data_ptr(), s),
                               "slam2d_refine_points")
            return call

        res = alternating_blocks(L, {"slam2d_refine_poses": refine_scan, "slam2d_refine_points, the same scan as points": refine_pts(d_one),
                                     "slam2d_refine_points, four scans merged": refine_pts(d_four)})
        report(emit, "refine, both default stages", res, N=N, points=[len(rng), len(one), len(four)],
               stages=[[list(a), list(b)] for a, b in stages])
        del d_pose, rwork, words


if __name__ == "__main__":
    main()
