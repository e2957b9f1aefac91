#!/usr/bin/env python3
"""Device time of slam2d_field_build_distance against slam2d_field_build on the same level and frames, and what the likelihood
field buys the search and the filter: the figures of profiles/r19_distance_field.md.

    python tools/distance_field_time.py [--quick] [--no-localise] [--out distance_field_time.json]

Timing: HIP events around every call, the median of 20 calls after 3 warm-ups, each contender in a block of its own (the full
build in its steady state: consecutive full builds of one level).  Frames: the 289 x 289 frame of the tests (unit 0.1 m) and the
covering frame of examples/localise.py at the reference's unit of 0.02 m (1441 x 1441); tables of R = 15, 72 and 256; 1 and 16
slots.  Then, in the world of examples/relocalise.py and examples/localise.py: the coarsest lattice step at which searchPoses
still has the true pose among its top 5 peaks, and the scan at which a uniformly seeded Localiser first comes within one cell
of the true pose, blurred field against likelihood field."""
import ctypes as C
import importlib
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

pkg = importlib.import_module("slam-2d-lidar-scan_amd")
engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

SIZE, R, FOV, BEAMS = 20, 4.0, np.pi, 180
ORIGIN = (-SIZE / 2, -SIZE / 2)
SMP = (0.7, 0.25, 1, 1.0, 1.0, 0.3, 0.15, 5)                  # as the examples
WINDOW = (0.0, 0.0, 8.0)
QUICK = "--quick" in sys.argv
CALLS, WARM = (3, 1) if QUICK else (20, 3)
TABLES = {15: 208, 72: 5171, 256: 65536}                       # R -> entries (likelihood_table(0.1, 0.2), (0.02, 0.2), the longest)
out = {"device_us": [], "search": {}, "localise": {}}


def per_call_us(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b))
    return statistics.median(us), min(us), max(us)


def builds(unit, P):
    dev = torch.device("cuda:0")
    lidar = engine.LidarModel.get(unit, R, FOV, BEAMS, 3 * unit)
    _, _, sigma, move_sigma, max_move_dev, turn_sigma, miss, factor = SMP
    kw = dict(step=unit, sigma=sigma, miss_prob=miss ** (2 / factor), search_radius_ctor=matcher.covering_radius(WINDOW[2], R, unit, unit),
              radius=unit, half_rad=0.0, fine=True, move_sigma=move_sigma, max_move_dev=max_move_dev, turn_sigma=turn_sigma)
    lv = engine.SearchLevel(lidar, P, dev, bnb=False, **kw)
    world = synth.make_world(SIZE, unit, seed=3, n_boxes=25)
    m = engine.MapState.create(SIZE, SIZE, {"x": 0.0, "y": 0.0}, unit, dev)
    m.upload(*synth.counts_from_world(world))
    m.ensure_contains([-lv.reach, lv.reach], [-lv.reach, lv.reach], unit)
    eng = engine.ParticleEngine(lidar, [m] + [m.clone() for _ in range(P - 1)], dev)
    d_c = eng.to_device([[0.0, 0.0]] * P)
    eng.refresh_bits()
    L, s = eng.L, engine._stream()
    args = (C.byref(eng.lidar_c), C.byref(lv.c), eng.d_maps.data_ptr(), P, d_c.data_ptr(), 2)

    def full_build():                                          # both contenders at the C ABI: the host's part is a stamp and a call
        lv.next_generation()
        _lib.check(L.slam2d_field_build(*args, eng.flags.data_ptr(), s), "slam2d_field_build")

    full = per_call_us(full_build)
    fr = lv.frames()[0]
    row = dict(unit=unit, P=P, frame=[int(fr["fh"]), int(fr["fw"])], field_build_us=full)
    for radius, n in TABLES.items():
        d_lut = torch.from_numpy(np.minimum(np.arange(n, dtype=np.uint64) * 1000, 0xffffffff).astype(np.uint32).view(np.int32)).to(dev)

        def distance_build():
            lv.next_generation()
            _lib.check(L.slam2d_field_build_distance(*args, d_lut.data_ptr(), n, None, eng.flags.data_ptr(), s), "slam2d_field_build_distance")

        row[f"distance_R{radius}_us"] = per_call_us(distance_build)
    eng.take_flags()
    out["device_us"].append(row)
    print(row, flush=True)


for unit in (0.1, 0.02):
    for P in (1, 16):
        builds(unit, P)

if "--no-localise" not in sys.argv:
    unit = 0.1
    world = synth.make_world(SIZE, unit, seed=3, n_boxes=25)
    walk = np.array(synth.random_walk(world, unit, ORIGIN, 40, seed=5))
    scans = [synth.raycast(world, unit, ORIGIN, p, FOV, BEAMS, R) for p in walk]
    true = [{"x": p[0], "y": p[1], "theta": p[2], "range": r} for p, r in zip(walk, scans)]
    og = pkg.map_from_poses(true, mapXLength=SIZE, mapYLength=SIZE, unitGridSize=unit, lidarFOV=FOV, lidarMaxRange=R, wallThickness=3 * unit)
    sm = pkg.ScanMatcher(og, *SMP)
    fields = {"blurred": None, "likelihood": dict(sigma=0.2)}
    # the coarsest lattice step that still has the true pose among the top 5 peaks (within a step and a heading step of it)
    for name, lik in fields.items():
        res = {}
        for step in (0.1, 0.2, 0.3, 0.4, 0.5, 0.75, 1.0, 1.5):
            hits = 0
            for k in (5, 15, 25, 35):
                found = sm.searchPoses(true[k], WINDOW, step=step, headings=120, top=5, likelihood=lik)
                hits += any(max(abs(q.x - walk[k][0]), abs(q.y - walk[k][1])) <= step and
                            abs((q.theta - walk[k][2] + math.pi) % (2 * math.pi) - math.pi) <= 2 * math.pi / 120 + 1e-9 for q in found["peaks"])
            res[str(step)] = hits
        out["search"][name] = res
        print("search: scans of 4 whose true pose is among the top 5 peaks, by lattice step", name, res, flush=True)
    # a uniformly seeded set: the first scan whose mean pose is within one cell of the true pose
    for name, lik in fields.items():
        res = {}
        for bits in (14, 16, 18):
            loc = pkg.Localiser(sm, WINDOW, particles=1 << bits, sigma=(0.03, 0.03, 0.02), temperature=64.0, seed=1, likelihood=lik)
            loc.seed_uniform()
            reports = loc.run(true)
            off = [math.hypot(rep["mean_pose"][0] - t["x"], rep["mean_pose"][1] - t["y"]) for rep, t in zip(reports, true)]
            first = next((i for i, d in enumerate(off) if d <= unit), None)
            res[f"2^{bits}"] = dict(first_scan_within_one_cell=first, off_at_last_scan_m=off[-1])
        out["localise"][name] = res
        print("localise: seed_uniform", name, res, flush=True)

if "--out" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
print("done")
