#!/usr/bin/env python3
"""Device time of slam2d_mcl_step against slam2d_score_poses on the same poses, and Localiser.step against the host route
(score_poses rows, a download, NumPy systematic resampling): the figures of profiles/r13_mcl_step.md.

    python tools/mcl_step_time.py [--quick] [--prof] [--out mcl_step_time.json]

--quick: two calls per block; --prof: the device part only, for a run under rocprofv3 --kernel-trace --stats."""
import importlib
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

pkg = importlib.import_module("slam-2d-lidar-scan_amd")
engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

SIZE, UNIT, R, FOV, BEAMS, WALL = 20, 0.1, 4.0, np.pi, 180, 0.5
ORIGIN = (-SIZE / 2, -SIZE / 2)
SMP = (0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)
WINDOW = (0.0, 0.0, 8.0)
PROF = "--prof" in sys.argv
QUICK = "--quick" in sys.argv or PROF

world = synth.make_world(SIZE, UNIT, seed=3, n_boxes=25)
walk = np.array(synth.random_walk(world, UNIT, ORIGIN, 12, seed=5))
scans = np.array([synth.raycast(world, UNIT, ORIGIN, p, FOV, BEAMS, R) for p in walk])
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
d_rng = eng.to_device(scans[0])
d_rep = torch.empty(16, dtype=torch.int64, device=eng.device)
out = {"device_ms": {}, "end_to_end_ms": {}}


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


for N, reps in ((4096, 200), (65536, 40), (1 << 20, 6)):
    if QUICK:
        reps = 2
    rs = np.random.RandomState(N)
    cloud = walk[0] + rs.standard_normal((N, 3)) * np.array([0.3, 0.3, 0.2])
    d_in, d_out = eng.to_device(cloud), torch.empty((N, 3), dtype=torch.float64, device=eng.device)
    step = lambda: eng.mcl_step(lv, 0, d_in, d_out, N, (0.0, 0.0, 0.0), (0.02, 0.02, 0.01), 1, 2, d_rng, free, d_lut, shift, d_rep)
    score = lambda: eng.score_poses(lv, 0, d_in, 3, N, d_rng, 0)
    with engine.pinned_stream():
        res = {"mcl_step": [], "score_poses": []}
        for rnd in range(2 if QUICK else 4):                   # alternate the two in one process
            res["mcl_step"] += timed(step, reps, 3)
            res["score_poses"] += timed(score, reps, 3)
    rep = engine.mcl_report_host(d_rep)
    out["device_ms"][str(N)] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), blocks=len(v), calls_per_block=reps) for k, v in res.items()}
    out["device_ms"][str(N)]["distinct"] = rep["distinct"]
    print(N, {k: round(statistics.median(v), 4) for k, v in res.items()}, "distinct", rep["distinct"], flush=True)

if PROF:
    sys.exit(0)

# end to end per scan: Localiser.step against scorePoses rows + download + NumPy systematic resampling + upload
for N in (4096, 65536):
    loc = pkg.Localiser(sm, WINDOW, particles=N, sigma=(0.03, 0.03, 0.02), temperature=64.0, seed=3)
    loc.seed_at(walk[0], (0.1, 0.1, 0.05))
    motions = [(0.0, 0.0, 0.0)] + [importlib.import_module("slam-2d-lidar-scan_amd.localise").odometry_motion(walk[i - 1], walk[i]) for i in range(1, len(walk))]
    loops = 1 if QUICK else 5

    def device_route():
        loc.seed_at(walk[0], (0.1, 0.1, 0.05))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(len(walk)):
            est = loc.step(scans[i], motions[i])
        return (time.perf_counter() - t0) / len(walk) * 1e3, est

    def host_route():
        rs = np.random.RandomState(1)
        cur = walk[0] + rs.standard_normal((N, 3)) * np.array([0.1, 0.1, 0.05])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(len(walk)):
            f, s, t = motions[i]
            fx, fy = f + 0.03 * rs.standard_normal(N), s + 0.03 * rs.standard_normal(N)
            c, sn = np.cos(cur[:, 2]), np.sin(cur[:, 2])
            cur = np.column_stack([cur[:, 0] + c * fx - sn * fy, cur[:, 1] + sn * fx + c * fy, cur[:, 2] + t + 0.02 * rs.standard_normal(N)])
            rows = eng.score_poses(lv, 0, eng.to_device(cur), 3, N, eng.to_device(scans[i]), 0).cpu().numpy()
            cost = rows[:, 6] + (rows[:, 4] - rows[:, 3]) * free
            w = np.exp(-(cost - cost.min()) / (lv.c.cost_scale * 64.0))
            C = np.cumsum(w)
            anc = np.minimum(np.searchsorted(C, (np.arange(N) + rs.uniform()) * (C[-1] / N), side="right"), N - 1)
            cur = cur[anc]
        return (time.perf_counter() - t0) / len(walk) * 1e3, cur.mean(axis=0)

    device_route(), host_route()
    dv, hv = [], []
    for _ in range(loops):
        dv.append(device_route()[0])
        hv.append(host_route()[0])
    est, mean = device_route()[1], host_route()[1]
    out["end_to_end_ms"][str(N)] = dict(localiser_step=dict(median=statistics.median(dv), min=min(dv), max=max(dv)),
                                        host_route=dict(median=statistics.median(hv), min=min(hv), max=max(hv)),
                                        error_m=dict(localiser=math.hypot(est["mean_pose"][0] - walk[-1][0], est["mean_pose"][1] - walk[-1][1]),
                                                     host=math.hypot(mean[0] - walk[-1][0], mean[1] - walk[-1][1])))
    print(N, out["end_to_end_ms"][str(N)], flush=True)

if "--out" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
print("done")
