#!/usr/bin/env python3
"""Time slam2d_score_poses on the device (profiles/r11_score_poses.md).

    python tools/score_poses_time.py [--out FILE]

For the test lattice (17 x 17 x 24 poses + 1, 60 beams, the covering level of tests/test_gpu_score.py) and for 10^5 and 10^6
seeded poses at config 2's lidar (0.1 m cells, 34.5 m, 180 beams over pi) and config 5's (0.05 m cells, 30 m, 1081 beams over
1.5 pi), each in the matcher's fine covering level of a 20 m window in the synthetic 100 m world: the time of ONE launch from HIP
events (slam2d_timer_*) around blocks of back-to-back launches on one stream, a warm-up block first, the median of seven blocks
with their range; ns per pose-beam; mean |U| and inside beams per pose.  Then, for orientation, the NumPy yardstick
(tests/score_yardstick.py) looped over poses on this host's CPU, in poses/s.  Prints one JSON line per measurement.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed_blocks(L, eng, lv, d_pose, N, d_rng, calls, blocks=7):
    _lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    out = torch.empty((N, _lib.SCORE_STRIDE), dtype=torch.float64, device=eng.device)
    timer = L.slam2d_timer_create()
    s = engine._stream()

    def block():
        _lib.check(L.slam2d_timer_start(timer, s), "timer")
        for _ in range(calls):
            _lib.check(L.slam2d_score_poses(C.byref(eng.lidar_c), C.byref(lv.c), 0, N, d_pose.data_ptr(), 3, d_rng.data_ptr(), 0,
                                            out.data_ptr(), s), "slam2d_score_poses")
        _lib.check(L.slam2d_timer_stop(timer, s), "timer")
        ms = C.c_float()
        _lib.check(L.slam2d_timer_elapsed_ms(timer, C.byref(ms)), "timer")
        return ms.value / calls

    block()                                                    # warm-up
    t = sorted(block() for _ in range(blocks))
    L.slam2d_timer_destroy(timer)
    return t[len(t) // 2], t[0], t[-1], out


def measure(pkg, name, og, sm, poses, rng, window, emit):
    L = importlib.import_module("slam-2d-lidar-scan_amd._lib").lib()
    first = sm.scorePoses(poses[:64], rng, window=window)      # builds the covering level's field
    lv, eng = sm.last_cover["level"], og.engine()
    d_rng = eng.to_device(rng)
    B = len(rng)
    for N in sorted({len(poses), *[n for n in (100_000, 1_000_000) if n < len(poses)]}):
        d_pose = eng.to_device(poses[:N])
        calls = max(3, min(2000, int(1e10 / (N * B))))      # ~0.1 s per block
        med, lo, hi, out = timed_blocks(L, eng, lv, d_pose, N, d_rng, calls)
        rows = eng.score_host(out)
        emit(dict(what="slam2d_score_poses", lidar=name, beams=B, poses=N, field=[int(lv.frames()[0]["fh"]), int(lv.frames()[0]["fw"])],
                  calls_per_block=calls, ms_per_launch=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5),
                  ns_per_pose_beam=round(1e6 * med / (N * B), 4), poses_per_s=round(N / (1e-3 * med)),
                  mean_cells=round(float(rows["cells"].mean()), 1), mean_inside=round(float(rows["inside"].mean()), 1),
                  in_range=int(rows["in_range"][0])))
    assert np.array_equal(first["score"], eng.score_host(out)["score"][:64])


def world_case(pkg, name, unit, R, fov, beams, n_poses, emit):
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    size = 100
    origin = (-size / 2, -size / 2)
    world = synth.make_world(size, unit, seed=2, n_boxes=40)
    og = pkg.OccupancyGrid(size, size, {"x": 0.0, "y": 0.0}, unit, fov, beams, R, 5 * unit)
    og.set_counts(*synth.counts_from_world(world))
    rs = np.random.RandomState(4)
    true = synth.free_pose_near(world, unit, origin, rs, spread=2.0)
    rng = synth.raycast(world, unit, origin, true, fov, beams, R)
    poses = np.column_stack([rs.uniform(-10, 10, n_poses), rs.uniform(-10, 10, n_poses), rs.uniform(-np.pi, np.pi, n_poses)])
    poses[0] = true
    sm = pkg.ScanMatcher(og, 0.7, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 5)
    measure(pkg, name, og, sm, poses, rng, (0.0, 0.0, 10.0), emit)
    return og, sm, poses, rng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-poses", type=int, default=1_000_000)
    args = ap.parse_args()
    pkg = importlib.import_module("slam-2d-lidar-scan_amd")
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    # the test lattice
    import test_score_host as H
    world, walk, scans = H.walk()
    og = pkg.OccupancyGrid(H.SIZE, H.SIZE, H.INIT, H.UNIT, H.FOV, H.BEAMS, H.R, H.WALL)
    og.set_counts(*synth.counts_from_world(world))
    sm = pkg.ScanMatcher(og, 0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)
    measure(pkg, "test lattice", og, sm, np.vstack([H.lattice(), walk[5]]), scans[5], (0.0, 0.0, 8.0), emit)

    world_case(pkg, "config 2", 0.1, 34.5, np.pi, 180, args.max_poses, emit)
    og, sm, poses, rng = world_case(pkg, "config 5", 0.05, 30.0, 1.5 * np.pi, 1081, args.max_poses, emit)

    # the CPU yardstick on this host, on the device's own field of the last case
    import score_yardstick as yard
    lv = sm.last_cover["level"]
    fr = lv.frames()[0]
    field = lv.field_cost(0)
    for B, r in ((1081, rng), (180, rng[::6][:180])):
        n = 400
        t0 = time.perf_counter()
        yard.score_poses(field, (float(fr["xlo"]), float(fr["ylo"])), lv.c.cost_scale, lv.step, poses[:n], r, 1.5 * np.pi, 30.0)
        dt = time.perf_counter() - t0
        emit(dict(what="NumPy yardstick, one CPU thread", beams=B, poses=n, poses_per_s=round(n / dt)))


if __name__ == "__main__":
    main()
