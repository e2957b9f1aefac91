#!/usr/bin/env python3
"""Time slam2d_search_lattice on the device against slam2d_score_poses on the same poses (profiles/r12_search_lattice.md).

    python tools/search_lattice_time.py [--out FILE]

Three lattices, each over the matcher's fine covering level of its window, full field build, one scan:
  * the lattice of examples/relocalise.py (161 x 161 positions x 120 headings, 180 beams, its mapped synthetic world);
  * config 2's lidar (0.1 m cells, 34.5 m, 180 beams over pi) over a 20 m window of the synthetic 100 m world, 0.1 m x 120 headings;
  * config 5's lidar (0.05 m cells, 30 m, 1081 beams over 1.5 pi) over the same window, 0.1 m x 120 headings.
For each: the time of ONE call of slam2d_search_lattice (both its launches) and of ONE launch of slam2d_score_poses on the
materialised poses of the same lattice -- same process, same field, same stream -- from HIP events (slam2d_timer_*) around
blocks of back-to-back calls of about 0.1 s, a warm-up block first, the median of seven blocks with their range; that the two
give the same image; and the wall time of ScanMatcher.searchPoses and of ScanMatcher.scorePoses + the host's arg-max, end to
end (field build, transfers and decoding included), the median of five calls.  Prints one JSON line per measurement.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "examples")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")


def timed_blocks(L, call, ms_guess, blocks=7):
    """(median, min, max) ms per call of ``call(stream)`` over ``blocks`` blocks of about 0.1 s, one warm-up block first."""
    timer = L.slam2d_timer_create()
    s = engine._stream()

    def block(calls):
        _lib.check(L.slam2d_timer_start(timer, s), "timer")
        for _ in range(calls):
            call(s)
        _lib.check(L.slam2d_timer_stop(timer, s), "timer")
        ms = C.c_float()
        _lib.check(L.slam2d_timer_elapsed_ms(timer, C.byref(ms)), "timer")
        return ms.value / calls

    first = block(3)                                           # warm-up, and the size of a block
    calls = max(3, min(2000, int(100.0 / max(first, ms_guess))))
    t = sorted(block(calls) for _ in range(blocks))
    L.slam2d_timer_destroy(timer)
    return t[len(t) // 2], t[0], t[-1], calls


def lattice_poses(lat):
    gt, gy, gx = np.meshgrid(lat.thetas, lat.ys, lat.xs, indexing="ij")
    return np.stack([gx, gy, gt], axis=-1).reshape(-1, 3)


def measure(name, og, sm, rng, window, step, headings, emit):
    L = _lib.lib()
    res = sm.searchPoses(rng, window, step=step, headings=headings)      # builds the covering level's field
    lv, lat, eng = sm.last_cover["level"], sm.last_cover["lattice"], og.engine()
    free = int(engine.encode_cost(lv.floor_value, lv.cost_scale))
    B, N = len(rng), lat.nx * lat.ny * lat.nth
    d_rng = eng.to_device(rng)
    poses = lattice_poses(lat)
    d_pose = eng.to_device(poses)
    rows = torch.empty((N, _lib.SCORE_STRIDE), dtype=torch.float64, device=eng.device)
    n = L.slam2d_search_lattice_work(C.byref(eng.lidar_c), lat.nx, lat.ny, lat.nth)
    work = torch.empty(n, dtype=torch.int64, device=eng.device)
    out = torch.empty((lat.ny, lat.nx), dtype=torch.int64, device=eng.device)

    def search(s):
        _lib.check(L.slam2d_search_lattice(C.byref(eng.lidar_c), C.byref(lv.c), 0, lat.nx, lat.ny, lat.nth, lat.x0, lat.dx, lat.y0, lat.dy,
                                           lat.th0, lat.dth, d_rng.data_ptr(), free, work.data_ptr(), out.data_ptr(), s), "slam2d_search_lattice")

    def score(s):
        _lib.check(L.slam2d_score_poses(C.byref(eng.lidar_c), C.byref(lv.c), 0, N, d_pose.data_ptr(), 3, d_rng.data_ptr(), 0,
                                        rows.data_ptr(), s), "slam2d_score_poses")

    fr = lv.frames()[0]
    common = dict(lidar=name, beams=B, in_range=int((rng < og.lidarMaxRange).sum()), lattice=[lat.nx, lat.ny, lat.nth], poses=N,
                  step=lat.dx, field=[int(fr["fh"]), int(fr["fw"])])
    t = {}
    for what, call in (("slam2d_search_lattice", search), ("slam2d_score_poses", score)):
        med, lo, hi, calls = timed_blocks(L, call, 1e-3)
        t[what] = med
        emit(dict(what=what, **common, calls_per_block=calls, ms_per_call=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5),
                  ns_per_pose_beam=round(1e6 * med / (N * B), 5)))
    # the same image from either
    cost = rows[:, 6].to(torch.int64) + (rows[:, 4] - rows[:, 3]).to(torch.int64) * free
    it = torch.arange(lat.nth, dtype=torch.int64, device=eng.device).reshape(-1, 1, 1)
    image = ((cost.reshape(lat.nth, lat.ny, lat.nx) << 16) | it).min(dim=0).values
    same = bool(torch.equal(image, out))
    emit(dict(what="search image == image of the score_poses rows", **common, equal=same,
              launch_ratio_score_over_search=round(t["slam2d_score_poses"] / t["slam2d_search_lattice"], 3)))
    del rows, d_pose, cost, image

    # end to end, wall time
    def wall(f, n=5):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(1e3 * (time.perf_counter() - t0))
        return sorted(ts)

    def by_score_poses():
        s = sm.scorePoses(poses, rng, window=window)
        return int(np.argmax(np.where(s["inside"] > 0, s["beam_score"], -np.inf)))

    by_score_poses()                                           # (warm-up of this path's level)
    a = wall(lambda: sm.searchPoses(rng, window, step=step, headings=headings))
    b = wall(by_score_poses)
    emit(dict(what="end to end, wall ms", **common, searchPoses_ms=[round(v, 2) for v in (a[len(a) // 2], a[0], a[-1])],
              scorePoses_argmax_ms=[round(v, 2) for v in (b[len(b) // 2], b[0], b[-1])]))
    return same


def world_case(pkg, name, unit, R, fov, beams, emit):
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    size = 100
    origin = (-size / 2, -size / 2)
    world = synth.make_world(size, unit, seed=2, n_boxes=40)
    og = pkg.OccupancyGrid(size, size, {"x": 0.0, "y": 0.0}, unit, fov, beams, R, 5 * unit)
    og.set_counts(*synth.counts_from_world(world))
    true = synth.free_pose_near(world, unit, origin, np.random.RandomState(4), spread=2.0)
    rng = synth.raycast(world, unit, origin, true, fov, beams, R)
    sm = pkg.ScanMatcher(og, 0.7, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 5)
    return measure(name, og, sm, rng, (0.0, 0.0, 10.0), 0.1, 120, emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
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
    og, readings, window = relocalise.synthetic(pkg, 3)
    sm = pkg.ScanMatcher(og, *relocalise.SM_PARAMS)
    ok = measure("relocalise", og, sm, np.asarray(readings[1]["range"], dtype=np.float64), window, 0.1, 120, emit)
    ok &= world_case(pkg, "config 2", 0.1, 34.5, np.pi, 180, emit)
    ok &= world_case(pkg, "config 5", 0.05, 30.0, 1.5 * np.pi, 1081, emit)
    if not ok:
        raise SystemExit("the search image differs from the image of the score_poses rows")


if __name__ == "__main__":
    main()
