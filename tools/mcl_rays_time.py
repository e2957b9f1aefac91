#!/usr/bin/env python3
"""Device time of slam2d_mcl_step_rays at strides 1, 4 and 8 against slam2d_mcl_step on the same particles, of the adaptive pair
at 4096 live particles, and Localiser.run over the log of examples/localise.py with and without ``rays``: the figures of
profiles/r26_mcl_rays.md.

    python tools/mcl_rays_time.py [--quick] [--out mcl_rays_time.json]

The scene of tools/mcl_step_time.py (profiles/r13_mcl_step.md) with the distance build of tools/rays_time.py
(profiles/r25_cast_rays.md).  HIP events around blocks of back-to-back calls, twelve blocks per call, the calls under comparison
alternating in one process; median with min .. max.  --quick: two calls per block."""
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
matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

SIZE, UNIT, R, FOV, BEAMS, WALL = 20, 0.1, 4.0, np.pi, 180, 0.5
ORIGIN = (-SIZE / 2, -SIZE / 2)
SMP = (0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)
WINDOW = (0.0, 0.0, 8.0)
MARGIN = matcher.ray_margin(WALL, UNIT)
STRIDES = (1, 4, 8)
QUICK = "--quick" in sys.argv

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
lut, shift = engine.weight_table(lv.c.cost_scale, 64.0)
d_lut = torch.from_numpy(lut.view(np.int32).copy()).to(eng.device)
d_rng = eng.to_device(scans[0])
MOTION, AMP = (0.0, 0.0, 0.0), (0.02, 0.02, 0.01)
out = {"scene": dict(beams=BEAMS, in_range=int((scans[0] < R).sum()), margin=MARGIN, table=len(table[0])), "device_ms": {}, "adaptive_ms": {},
       "localiser_run_ms": {}}


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
    """Twelve blocks of every call, three at a time, the calls taking turns."""
    res = {k: [] for k in calls}
    with engine.pinned_stream():
        for _ in range(2 if QUICK else 4):
            for k, fn in calls.items():
                res[k] += timed(fn, reps, 3)
    return res


def summary(res, reps):
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v), blocks=len(v), calls_per_block=reps) for k, v in res.items()}


def through_cost(stride):
    return min(stride * free, 2 ** 32 - 1)


for N, reps in ((4096, 200), (65536, 40)):
    if QUICK:
        reps = 2
    rs = np.random.RandomState(N)
    cloud = walk[0] + rs.standard_normal((N, 3)) * np.array([0.3, 0.3, 0.2])
    d_in, d_out = eng.to_device(cloud), torch.empty((N, 3), dtype=torch.float64, device=eng.device)
    d_rep = {k: torch.empty(16, dtype=torch.int64, device=eng.device) for k in ("mcl_step",) + tuple(f"rays_stride_{s}" for s in STRIDES)}
    calls = {"mcl_step": lambda: eng.mcl_step(lv, 0, d_in, d_out, N, MOTION, AMP, 1, 2, d_rng, free, d_lut, shift, d_rep["mcl_step"])}
    for s in STRIDES:
        calls[f"rays_stride_{s}"] = (lambda s=s: eng.mcl_step_rays(lv, 0, d2, d_in, d_out, N, MOTION, AMP, 1, 2, d_rng, free, s, 0, MARGIN,
                                                                   through_cost(s), d_lut, shift, d_rep[f"rays_stride_{s}"]))
    res = alternate(calls, reps)
    out["device_ms"][str(N)] = summary(res, reps)
    for s in STRIDES:
        rep = engine.mcl_rays_report_host(d_rep[f"rays_stride_{s}"])
        out["device_ms"][str(N)][f"rays_stride_{s}"].update(through_per_particle=rep["through"] / N, distinct=rep["distinct"])
    out["device_ms"][str(N)]["mcl_step"]["distinct"] = engine.mcl_report_host(d_rep["mcl_step"])["distinct"]
    print(N, {k: round(statistics.median(v), 4) for k, v in res.items()},
          "through per particle", {s: round(out["device_ms"][str(N)][f"rays_stride_{s}"]["through_per_particle"], 2) for s in STRIDES}, flush=True)

# the adaptive pair: 4096 live particles of a capacity of 65536, a table that keeps the count
N, CAP = 4096, 65536
reps = 2 if QUICK else 200
rs = np.random.RandomState(N)
cloud = np.zeros((CAP, 3))
cloud[:N] = walk[0] + rs.standard_normal((N, 3)) * np.array([0.3, 0.3, 0.2])
d_in, d_out = eng.to_device(cloud), torch.empty((CAP, 3), dtype=torch.float64, device=eng.device)
bins = _lib.Slam2dMclBins(x0=-8.0, y0=-8.0, cell=0.5, turn=2 * np.pi / 36, nx=32, ny=32, nth=36)
d_ntab = torch.full((64,), N, dtype=torch.int32, device=eng.device)
d_count, d_count_out = torch.full((1,), N, dtype=torch.int32, device=eng.device), torch.empty(1, dtype=torch.int32, device=eng.device)
d_rep = {k: torch.empty(24, dtype=torch.int64, device=eng.device) for k in ("adaptive", "adaptive_rays_stride_4")}
res = alternate({
    "adaptive": lambda: eng.mcl_step_adaptive(lv, 0, d_in, d_out, CAP, d_count, MOTION, AMP, 1, 2, d_rng, free, d_lut, shift, bins, d_ntab,
                                              d_rep["adaptive"], d_count_out=d_count_out),
    "adaptive_rays_stride_4": lambda: eng.mcl_step_adaptive_rays(lv, 0, d2, d_in, d_out, CAP, d_count, MOTION, AMP, 1, 2, d_rng, free, 4, 0, MARGIN,
                                                                 through_cost(4), d_lut, shift, bins, d_ntab, d_rep["adaptive_rays_stride_4"],
                                                                 d_count_out=d_count_out)}, reps)
out["adaptive_ms"] = summary(res, reps)
rep = engine.mcl_rays_report_host(d_rep["adaptive_rays_stride_4"])
out["adaptive_ms"]["adaptive_rays_stride_4"].update(through_per_particle=rep["through"] / rep["n_in"], n_in=rep["n_in"], n_out=rep["n_out"])
print("adaptive, 4096 live of 65536", {k: round(statistics.median(v), 4) for k, v in res.items()}, flush=True)

# Localiser.run over the log of examples/localise.py, seeded around the search's peaks, with and without rays
example = importlib.import_module("localise")
true, log, grid, window = example.synthetic(40)
og2 = pkg.map_from_poses(true, **grid)
sm2 = pkg.ScanMatcher(og2, *example.SM_PARAMS)
peaks = sm2.searchPoses(log[0], window, headings=120, top=4)["peaks"]
locs = {name: pkg.Localiser(sm2, window, particles=4096, sigma=(0.03, 0.03, 0.02), temperature=64.0, seed=1, rays=rays)
        for name, rays in (("plain", None), ("rays_stride_4", dict(stride=4)))}
ms = {k: [] for k in locs}
for rnd in range(2 if QUICK else 13):                          # (the first round warms up and is dropped)
    for name, loc in locs.items():
        loc.scan = 0
        loc.seed_from_peaks(peaks, (0.1, 0.1, 0.05))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reports = loc.run(log)
        if rnd:
            ms[name].append((time.perf_counter() - t0) / len(log) * 1e3)
        err = float(np.hypot(reports[-1]["mean_pose"][0] - true[-1]["x"], reports[-1]["mean_pose"][1] - true[-1]["y"]))
        out["localiser_run_ms"].setdefault(name, {}).update(final_error_m=err, through_per_particle=[r.get("through", 0) / 4096 for r in reports])
for name, v in ms.items():
    out["localiser_run_ms"][name].update(median=statistics.median(v), min=min(v), max=max(v), rounds=len(v), scans=len(log))
    print("Localiser.run", name, "ms per scan", round(statistics.median(v), 4), f"({min(v):.4f} .. {max(v):.4f})",
          "final error", round(out["localiser_run_ms"][name]["final_error_m"], 3), flush=True)

if "--out" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
print("done")
