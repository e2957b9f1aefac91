#!/usr/bin/env python3
"""Device time of slam2d_mcl_step_adaptive against slam2d_mcl_step, and Localiser.run adaptive against fixed from a uniform
seeding: the figures of profiles/r18_mcl_adaptive.md.

    python tools/mcl_adaptive_time.py [--quick] [--prof] [--baseline-lib libslam2d_hip.so of another commit] [--out FILE.json]

--quick: two calls per block and a short log; --prof: the device part only, for a run under rocprofv3 --kernel-trace --stats.
--baseline-lib: take slam2d_mcl_step from that library (the parent commit's, built beside this one) in the same process."""
import ctypes
import importlib
import json
import math
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
synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

SIZE, UNIT, R, FOV, BEAMS, WALL = 20, 0.1, 4.0, np.pi, 180, 0.5
ORIGIN = (-SIZE / 2, -SIZE / 2)
SMP = (0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)
WINDOW = (0.0, 0.0, 8.0)
PROF = "--prof" in sys.argv
QUICK = "--quick" in sys.argv or PROF
arg = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None

# the scene of profiles/r13_mcl_step.md
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
d_rep = torch.empty(24, dtype=torch.int64, device=eng.device)
BINS = _lib.Slam2dMclBins(x0=-8.0, y0=-8.0, cell=0.5, turn=2 * math.pi / 36, nx=32, ny=32, nth=36)      # 0.5 m x 10 degrees over the window
ONE_BIN = _lib.Slam2dMclBins(x0=-8.0, y0=-8.0, cell=16.0, turn=2 * math.pi, nx=1, ny=1, nth=1)          # a bitmap of one word
MOTION, AMP = (0.0, 0.0, 0.0), (0.02, 0.02, 0.01)
out = {"device_ms": {}, "end_to_end": {}}

base = None
if arg("--baseline-lib"):
    base = ctypes.CDLL(os.path.abspath(arg("--baseline-lib")))
    for name in ("slam2d_mcl_step", "slam2d_mcl_work"):
        getattr(base, name).restype, getattr(base, name).argtypes = _lib.SIGNATURES[name]
    assert not hasattr(base, "slam2d_mcl_step_adaptive"), "the baseline library has the new symbol: not the parent commit's"


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


def cloud(N):
    rs = np.random.RandomState(N)
    return walk[0] + rs.standard_normal((N, 3)) * np.array([0.3, 0.3, 0.2])


def plain_call(N):
    d_in, d_out = eng.to_device(cloud(N)), torch.empty((N, 3), dtype=torch.float64, device=eng.device)
    if base is None:
        return lambda: eng.mcl_step(lv, 0, d_in, d_out, N, MOTION, AMP, 1, 2, d_rng, free, d_lut, shift, d_rep)
    work = torch.empty(int(base.slam2d_mcl_work(N)), dtype=torch.int64, device=eng.device)
    m, a = (ctypes.c_double * 3)(*MOTION), (ctypes.c_double * 3)(*AMP)
    return lambda: _lib.check(base.slam2d_mcl_step(ctypes.byref(eng.lidar_c), ctypes.byref(lv.c), 0, N, d_in.data_ptr(), d_out.data_ptr(), 3, m, a,
                                                   1, 2, d_rng.data_ptr(), free, d_lut.data_ptr(), d_lut.numel(), shift, None, work.data_ptr(),
                                                   d_rep.data_ptr(), engine._stream()), "baseline slam2d_mcl_step")


def adaptive_call(n_cap, N, bins):
    """A constant table that returns N: the count word stays at N, every call does the same work."""
    poses = np.full((n_cap, 3), np.nan)
    poses[:N] = cloud(N)
    d_in, d_out = eng.to_device(poses), torch.empty((n_cap, 3), dtype=torch.float64, device=eng.device)
    d_n = torch.full((1,), N, dtype=torch.int32, device=eng.device)
    d_ntab = torch.full((1,), N, dtype=torch.int32, device=eng.device)
    return lambda: eng.mcl_step_adaptive(lv, 0, d_in, d_out, n_cap, d_n, MOTION, AMP, 1, 2, d_rng, free, d_lut, shift, bins, d_ntab, d_rep)


CAP = 1 << 20
cases = [("plain 4096", 200, lambda: plain_call(4096)), ("adaptive 4096 of 4096", 200, lambda: adaptive_call(4096, 4096, BINS)),
         ("adaptive 4096 of 2^20", 200, lambda: adaptive_call(CAP, 4096, BINS)), ("adaptive 4096 of 2^20, one bin", 200, lambda: adaptive_call(CAP, 4096, ONE_BIN)),
         ("adaptive 4096 of 4096, one bin", 200, lambda: adaptive_call(4096, 4096, ONE_BIN)),
         ("plain 2^20", 6, lambda: plain_call(CAP)), ("adaptive 2^20 of 2^20", 6, lambda: adaptive_call(CAP, CAP, BINS)),
         ("adaptive 2^20 of 2^20, one bin", 6, lambda: adaptive_call(CAP, CAP, ONE_BIN))]
with engine.pinned_stream():
    fns = [(name, 2 if QUICK else reps, make()) for name, reps, make in cases]
    res = {name: [] for name, _, _ in fns}
    for rnd in range(2 if QUICK else 4):                       # all cases alternate in one process, three blocks at a time
        for name, reps, fn in fns:
            res[name] += timed(fn, reps, 3)
            if name.startswith("adaptive"):
                rep = engine.mcl_adapt_report_host(d_rep)
                res.setdefault(name + " report", dict(n_in=rep["n_in"], n_out=rep["n_out"], bins=rep["bins"], reference_distinct=rep["reference_distinct"]))
for name, v in res.items():
    if isinstance(v, dict):
        out["device_ms"][name] = v
        continue
    out["device_ms"][name] = dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v), blocks=len(v))
    print(f"{name:34s} median {statistics.median(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}", res.get(name + " report", ""), flush=True)
out["baseline_lib"] = arg("--baseline-lib") or "this commit's"

if not PROF:
    # end to end: the example's log from a uniform seeding, adaptive against fixed
    example = importlib.import_module("localise")
    true, log, grid, window = example.synthetic(12 if QUICK else 40)
    og2 = pkg.map_from_poses(true, **grid)
    sm2 = pkg.ScanMatcher(og2, *example.SM_PARAMS)
    cap = 1 << 18
    for name, kw in (("fixed", dict()), ("adaptive", dict(adaptive=dict()))):
        loc = pkg.Localiser(sm2, window, particles=cap, sigma=(0.03, 0.03, 0.02), temperature=64.0, seed=1, **kw)
        times = []
        for _ in range(1 if QUICK else 5):
            loc.scan = 0
            loc.seed_uniform()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reports = loc.run(log)
            times.append(time.perf_counter() - t0)
        err = [math.hypot(rep["mean_pose"][0] - r["x"], rep["mean_pose"][1] - r["y"]) for r, rep in zip(true, reports)]
        within = next((i for i in range(len(err)) if all(e < grid["unitGridSize"] for e in err[i:])), None)
        out["end_to_end"][name] = dict(total_ms=dict(median=1e3 * statistics.median(times), min=1e3 * min(times), max=1e3 * max(times)),
                                       scans=len(log), error_m=[round(e, 3) for e in err], within_one_cell_from_scan=within,
                                       counts=[rep.get("n_out", cap) for rep in reports], bins=[rep.get("bins") for rep in reports],
                                       distinct=[rep["distinct"] for rep in reports])
        print(name, json.dumps(out["end_to_end"][name]), flush=True)

if arg("--out"):
    json.dump(out, open(arg("--out"), "w"), indent=1)
print("done")
