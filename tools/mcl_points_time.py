#!/usr/bin/env python3
"""Device time of slam2d_mcl_step_points against slam2d_mcl_step and of slam2d_score_points against slam2d_score_poses on the same
poses, in one build and one process, and Localiser.run_points against Localiser.run: the figures of profiles/r24_mcl_points.md.

    python tools/mcl_points_time.py [--quick] [--prof] [--out mcl_points_time.json]

The scene and the method of tools/mcl_step_time.py (profiles/r13_mcl_step.md): the 289 x 289 field, scan 0 of the walk at 180
beams, N normal draws about its pose, HIP events around blocks of back-to-back calls, the two forms of a pair alternating in
groups of three blocks.  The scan handed in as points is points.scan_points of it (180 rows, the beams out of range NaN); the
merged set is the last four scans of examples/relocalise.py's log at its second pick, as in profiles/r21_points.md, weighed by
particles about that pick's pose.
--quick: two calls per block; --prof: the device part at N = 4 096 and 65 536 only, two calls per block, for a run under
rocprofv3 --kernel-trace --stats."""
import importlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "examples")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

pkg = importlib.import_module("slam-2d-lidar-scan_amd")
engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
points = importlib.import_module("slam-2d-lidar-scan_amd.points")
synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")

SIZE, UNIT, R, FOV, BEAMS, WALL = 20, 0.1, 4.0, np.pi, 180, 0.5
ORIGIN = (-SIZE / 2, -SIZE / 2)
SMP = (0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)
WINDOW = (0.0, 0.0, 8.0)
PROF = "--prof" in sys.argv
QUICK = "--quick" in sys.argv or PROF

world = synth.make_world(SIZE, UNIT, seed=3, n_boxes=25)
walk = np.array(synth.random_walk(world, UNIT, ORIGIN, 12, seed=5))
scan0 = synth.raycast(world, UNIT, ORIGIN, walk[0], FOV, BEAMS, R)
long_walk = np.array(synth.random_walk(world, UNIT, ORIGIN, 40, seed=5))         # examples/relocalise.py's log: its second pick is scan 20
last_four = [dict(x=p[0], y=p[1], theta=p[2], range=synth.raycast(world, UNIT, ORIGIN, p, FOV, BEAMS, R)) for p in long_walk[17:21]]
merged, merged_stride = points.merge_scans(last_four, fov=FOV, max_range=R)
og = pkg.OccupancyGrid(SIZE, SIZE, {"x": 0.0, "y": 0.0}, UNIT, FOV, BEAMS, R, WALL)
og.set_counts(*synth.counts_from_world(world))
sm = pkg.ScanMatcher(og, *SMP)
lv = sm.covering_level("fine", WINDOW[2], shared=False)
og.checkAndExapndOG([-lv.reach, lv.reach], [-lv.reach, lv.reach])
eng = og.engine()
eng.field_build(lv, eng.to_device([[0.0, 0.0]]), 2)
eng.take_flags()
free = int(engine.encode_cost(lv.floor_value, lv.cost_scale))
lut, shift = engine.weight_table(lv.c.cost_scale, 64.0)
d_lut = torch.from_numpy(lut.view(np.int32).copy()).to(eng.device)
d_rep = torch.empty(16, dtype=torch.int64, device=eng.device)
d_scan0, d_scan20 = eng.to_device(scan0), eng.to_device(np.asarray(last_four[-1]["range"]))
d_one, d_four = eng.to_device(points.scan_points(scan0, FOV, R)), eng.to_device(merged)
out = {"scene": dict(in_range=int((scan0 < R).sum()), merged_points=len(merged), merged_stride=merged_stride,
                     device=torch.cuda.get_device_name(0)), "device_ms": {}, "run_ms_per_step": {}}
print(out["scene"], flush=True)


def timed(fn, reps, blocks):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return ms


def alternate(calls, reps):
    """{name: ms per call of every block}: the calls take turns in groups of three blocks, four rounds."""
    res = {name: [] for name in calls}
    with engine.pinned_stream():
        for _ in range(2 if QUICK else 4):
            for name, fn in calls.items():
                res[name] += timed(fn, reps, 3)
    return res


def record(key, res, reps, **more):
    out["device_ms"][key] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), blocks=len(v), calls_per_block=reps) for k, v in res.items()}
    out["device_ms"][key].update(more)
    print(key, {k: round(statistics.median(v), 4) for k, v in res.items()}, more, flush=True)


for N, reps in ((4096, 200), (65536, 40), (1 << 20, 6)):
    if PROF and N > 65536:
        continue
    if QUICK:
        reps = 2
    rs = np.random.RandomState(N)
    spread = np.array([0.3, 0.3, 0.2])
    d_in = eng.to_device(walk[0] + rs.standard_normal((N, 3)) * spread)
    d_in20 = eng.to_device(long_walk[20] + rs.standard_normal((N, 3)) * spread)
    d_out = torch.empty((N, 3), dtype=torch.float64, device=eng.device)
    args = ((0.0, 0.0, 0.0), (0.02, 0.02, 0.01), 1, 2)
    calls = {"mcl_step": lambda: eng.mcl_step(lv, 0, d_in, d_out, N, *args, d_scan0, free, d_lut, shift, d_rep),
             "mcl_step_points": lambda: eng.mcl_step_points(lv, 0, d_in, d_out, N, *args, d_one, BEAMS, free, d_lut, shift, d_rep),
             "mcl_step, scan 20": lambda: eng.mcl_step(lv, 0, d_in20, d_out, N, *args, d_scan20, free, d_lut, shift, d_rep),
             "mcl_step_points, four scans merged": lambda: eng.mcl_step_points(lv, 0, d_in20, d_out, N, *args, d_four, len(merged), free, d_lut,
                                                                              shift, d_rep)}
    distinct = {}
    for name, fn in calls.items():                             # (what each resampling keeps: the download synchronises)
        fn()
        distinct[name] = engine.mcl_report_host(d_rep)["distinct"]
    record(str(N), alternate(calls, reps), reps, distinct=distinct)
    if N == 65536:
        record("score, 65536", alternate({"score_poses": lambda: eng.score_poses(lv, 0, d_in, 3, N, d_scan0, 0),
                                          "score_points": lambda: eng.score_points(lv, 0, d_in, 3, N, d_one, BEAMS, 0),
                                          "score_points, four scans merged": lambda: eng.score_points(lv, 0, d_in20, 3, N, d_four, len(merged), 0)},
                                         reps), reps)

if PROF:
    sys.exit(0)

# Localiser.run against Localiser.run_points over the 40 scans of examples/localise.py: wall time on the host per step, the
# upload of the log and the one download included
import localise as example  # noqa: E402
true, log, grid, window = example.synthetic(40)
og2 = pkg.map_from_poses(true, **grid)
sm2 = pkg.ScanMatcher(og2, *example.SM_PARAMS)
sets1 = [points.scan_points(r["range"], grid["lidarFOV"], grid["lidarMaxRange"]) for r in log]
sets4 = [points.merge_scans(log[max(0, i - 3):i + 1], fov=grid["lidarFOV"], max_range=grid["lidarMaxRange"])[0] for i in range(len(log))]
motions = [localise.odometry_motion(log[i - 1], log[i]) if i else (0.0, 0.0, 0.0) for i in range(len(log))]
for N in (4096, 65536):
    loc = pkg.Localiser(sm2, window, particles=N, sigma=(0.03, 0.03, 0.02), temperature=64.0, seed=1)
    routes = {"run": lambda: loc.run(log), "run_points, one scan": lambda: loc.run_points(sets1, motions),
              "run_points, four scans merged": lambda: loc.run_points(sets4, motions)}
    ms, err = {k: [] for k in routes}, {}
    for rnd in range(2 if QUICK else 6):                       # (the first round warms up)
        for name, fn in routes.items():
            loc.scan = 0
            loc.seed_at((true[0]["x"], true[0]["y"], true[0]["theta"]), (0.1, 0.1, 0.05))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reports = fn()
            dt = (time.perf_counter() - t0) / len(log) * 1e3
            if rnd:
                ms[name].append(dt)
            x, y, _ = reports[-1]["mean_pose"]
            err[name] = float(np.hypot(x - true[-1]["x"], y - true[-1]["y"]))
    out["run_ms_per_step"][str(N)] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), last_pose_error_m=err[k]) for k, v in ms.items()}
    out["run_ms_per_step"][str(N)]["largest_set"] = max(len(q) for q in sets4)
    print(N, out["run_ms_per_step"][str(N)], flush=True)

if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(out, open(path, "w"), indent=1)
print("done")
