#!/usr/bin/env python3
"""Device time of slam2d_score_rays against slam2d_score_poses on the same poses, of slam2d_cast_rays at full range, and the
samples the skip rule examines per ray against the plain walk's: the figures of profiles/r25_cast_rays.md.

    python tools/rays_time.py [--quick] [--out rays_time.json]

--quick: two calls per block.  The scene of tools/mcl_step_time.py (180 beams, scan 0 of the walk, the 289 x 289 covering
field), filled by ONE distance build with the likelihood table (sigma 0.2 m), which leaves the field and the squared distances."""
import importlib
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rays_yardstick as ryard  # noqa: E402

pkg = importlib.import_module("slam-2d-lidar-scan_amd")
engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")

SIZE, UNIT, R, FOV, BEAMS, WALL = 20, 0.1, 4.0, np.pi, 180, 0.5
ORIGIN = (-SIZE / 2, -SIZE / 2)
SMP = (0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)
WINDOW = (0.0, 0.0, 8.0)
QUICK = "--quick" in sys.argv
K = math.ceil(R / UNIT)
MARGIN = matcher.ray_margin(WALL, UNIT)

world = synth.make_world(SIZE, UNIT, seed=3, n_boxes=25)
walk = np.array(synth.random_walk(world, UNIT, ORIGIN, 12, seed=5))
scans = np.array([synth.raycast(world, UNIT, ORIGIN, p, FOV, BEAMS, R) for p in walk])
og = pkg.OccupancyGrid(SIZE, SIZE, {"x": 0.0, "y": 0.0}, UNIT, FOV, BEAMS, R, WALL)
og.set_counts(*synth.counts_from_world(world))
sm = pkg.ScanMatcher(og, *SMP)
lv = sm.covering_level("fine", WINDOW[2], shared=False)
og.checkAndExapndOG([-lv.reach, lv.reach], [-lv.reach, lv.reach])
eng = og.engine()
table = engine.likelihood_table(UNIT, 0.2)
d2 = eng.field_build_distance(lv, eng.to_device([[0.0, 0.0]]), 2, table, dist2=True)
eng.take_flags()
free = int(table[0][-1])
d_rng = eng.to_device(scans[0])
out = {"scene": dict(beams=BEAMS, in_range=int((scans[0] < R).sum()), K=K, margin=MARGIN, table=len(table[0])), "device_ms": {}}


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


for N, reps in ((4096, 200), (65536, 40)):
    if QUICK:
        reps = 2
    rs = np.random.RandomState(N)
    cloud = walk[0] + rs.standard_normal((N, 3)) * np.array([0.3, 0.3, 0.2])
    d_in = eng.to_device(cloud)
    calls = dict(score_rays=lambda: eng.score_rays(lv, 0, d2, d_in, 3, N, d_rng, 0, MARGIN, free, free),
                 score_poses=lambda: eng.score_poses(lv, 0, d_in, 3, N, d_rng, 0),
                 cast_rays=lambda: eng.cast_rays(lv, 0, d2, d_in, 3, N, K))
    with engine.pinned_stream():
        res = {k: [] for k in calls}
        for rnd in range(2 if QUICK else 4):                   # alternate the three in one process
            for k, fn in calls.items():
                res[k] += timed(fn, reps, 3)
    rows = eng.rays_host(calls["score_rays"](), lv.cost_scale)
    out["device_ms"][str(N)] = {k: dict(median=statistics.median(v), min=min(v), max=max(v), blocks=len(v), calls_per_block=reps) for k, v in res.items()}
    out["device_ms"][str(N)]["through_mean"] = float(rows["through"].mean())
    print(N, {k: round(statistics.median(v), 4) for k, v in res.items()}, "through per pose", round(float(rows["through"].mean()), 2), flush=True)

# examined samples per ray, counted by the NumPy restatement of the skip rule on the device's own images, 4 096 poses
N = 4096
rs = np.random.RandomState(N)
cloud = walk[0] + rs.standard_normal((N, 3)) * np.array([0.3, 0.3, 0.2])
fr = lv.frames()[0]
frame, fh, fw = (float(fr["xlo"]), float(fr["ylo"])), int(fr["fh"]), int(fr["fw"])
dist2 = d2[0, :fh, :fw].cpu().numpy().astype(np.int64)
c, s = ryard.trig(cloud, (FOV, BEAMS, R))
x, y = cloud[:, 0:1], cloud[:, 1:2]
kind, k, examined = ryard.skip_walk(dist2, frame, UNIT, x, y, c, s, np.full(c.shape, K))
words = eng.cast_rays(lv, 0, d2, eng.to_device(cloud), 3, N, K).cpu().numpy().view(np.uint32)
agree = float((ryard.words(kind, k) == words).mean())          # (NumPy's cos / sin here: a ray in a million may differ by a cell)
plain = np.minimum(k, K) + 1
_, kend = ryard.beam_limits(np.broadcast_to(scans[0], c.shape), UNIT, R, MARGIN)
_, k2, examined2 = ryard.skip_walk(dist2, frame, UNIT, x, y, c, s, kend)
asked = kend >= 0
out["samples"] = dict(cast=dict(examined=float(examined.mean()), plain=float(plain.mean())),
                      score=dict(examined=float(examined2[asked].mean()), plain=float((np.minimum(k2, kend) + 1)[asked].mean()),
                                 asked_per_pose=float(asked.sum(axis=1).mean())),
                      words_equal_numpy_trig=agree, capped_cells=float((dist2 == len(table[0]) - 1).mean()))
print(out["samples"], flush=True)
if "--out" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
print("done")
