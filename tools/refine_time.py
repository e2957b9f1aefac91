#!/usr/bin/env python3
"""Time slam2d_refine_poses on the device against slam2d_score_poses over the materialised candidates of the same seeds, and a
Tracker against a Localiser over a log (profiles/r20_refine_poses.md).

    python tools/refine_time.py [--out FILE]

The world, lidar (180 beams over pi, 4 m) and 40-scan log of examples/localise.py, the matcher's fine covering level of its
window (a 289 x 289 field), full field build.  For N = 1, 4 096 and 65 536 seeds about the walk's first pose (up to 0.25 m and 0.05
rad off, its scan for all of them) and the default stages ((4, 4, 4) at (0.1 m, 0.1 m, 0.02 rad), then (2, 2, 2) at half and a
quarter of that: 729 + 125 candidates per seed):
  * the device time of the two calls of slam2d_refine_poses (three launches each), stage 2 from stage 1's poses on the device;
  * the device time of the parent's only batched way: ONE launch of slam2d_score_poses per stage over the materialised candidates
    of the same seeds (stage 2's about the poses stage 1 found), and, apart, the wall time of what that way needs besides -- the
    download of its rows and the host's arg-min per seed;
  * that both give the same words.
Device times are from HIP events (slam2d_timer_*) around blocks of back-to-back calls of about 0.1 s in one process, a warm-up
block first, the median of seven blocks with their range.  Then Tracker.run and Localiser.run (4 096 particles) over the 40
scans, wall time per scan end to end (uploads and the one download included), the median of seven runs after a warm-up run.
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
sys.path[:0] = [REPO, os.path.join(REPO, "examples"), os.path.join(REPO, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
from search_lattice_time import timed_blocks  # noqa: E402


def candidates(d_seed, radii, steps):
    """[N, nth * ny * nx, 3] on the device: the candidates of every seed in the order of their flat index (a rounded product, then
    an add, as the call forms them)."""
    ox, oy, ot = (torch.from_numpy(engine.refine_offsets(r).astype(np.float64)).to(d_seed.device) * float(s) for r, s in zip(radii, steps))
    gt, gy, gx = torch.meshgrid(ot, oy, ox, indexing="ij")
    off = torch.stack([gx, gy, gt], dim=-1).reshape(1, -1, 3)
    return (d_seed.reshape(-1, 1, 3) + off).contiguous()


def words_of(rows, N, outside):
    """[N, 2] int64 on the device from slam2d_score_poses' rows of the candidates: cost << 20 | f minimised, and cost(0)."""
    cost = (rows[:, 6].to(torch.int64) + (rows[:, 4] - rows[:, 3]).to(torch.int64) * outside).reshape(N, -1)
    f = torch.arange(cost.shape[1], dtype=torch.int64, device=rows.device).reshape(1, -1)
    return torch.stack([((cost << 20) | f).min(dim=1).values, cost[:, 0]], dim=1)


def measure(N, eng, lv, walk, scans, stages, outside, emit):
    L = _lib.lib()
    B = scans.shape[1]
    rs = np.random.RandomState(N)
    seeds = walk[0] + rs.uniform(-1, 1, (N, 3)) * (0.25, 0.25, 0.05)
    d_pose = [eng.to_device(seeds), torch.empty((N, 3), dtype=torch.float64, device=eng.device)]
    d_rng = eng.to_device(scans[0])
    work = torch.empty(L.slam2d_refine_work(N), dtype=torch.int64, device=eng.device)
    words = torch.empty((len(stages), N, 2), dtype=torch.int64, device=eng.device)

    def refine(s):
        for i, (radii, steps) in enumerate(stages):
            _lib.check(L.slam2d_refine_poses(C.byref(eng.lidar_c), C.byref(lv.c), 0, N, d_pose[i & 1].data_ptr(), d_pose[1 - (i & 1)].data_ptr(), 3,
                                             d_rng.data_ptr(), 0, None, *radii, *steps, outside, work.data_ptr(), words[i].data_ptr(), s),
                       "slam2d_refine_poses")

    refine(engine._stream())
    torch.cuda.synchronize()
    # the other route: the candidates of both stages materialised, stage 2's about the poses stage 1 left in d_pose[1]
    d_seed = eng.to_device(seeds)
    cands = [candidates(d_seed, *stages[0]), candidates(d_pose[1].clone(), *stages[1])]
    per = [c.shape[1] for c in cands]
    rows = [torch.empty((N * n, _lib.SCORE_STRIDE), dtype=torch.float64, device=eng.device) for n in per]

    def score(s):
        for c, r in zip(cands, rows):
            _lib.check(L.slam2d_score_poses(C.byref(eng.lidar_c), C.byref(lv.c), 0, c.shape[0] * c.shape[1], c.data_ptr(), 3, d_rng.data_ptr(), 0,
                                            r.data_ptr(), s), "slam2d_score_poses")

    common = dict(N=N, beams=B, candidates=per, stages=[[list(r), list(s)] for r, s in stages])
    t = {}
    for what, call in (("slam2d_refine_poses, both stages", refine), ("slam2d_score_poses over the candidates, both stages", score)):
        med, lo, hi, calls = timed_blocks(L, call, 1e-3)
        t[what] = med
        emit(dict(what=what, **common, calls_per_block=calls, ms_per_call=round(med, 5), ms_min=round(lo, 5), ms_max=round(hi, 5),
                  ns_per_candidate_beam=round(1e6 * med / (N * sum(per) * B), 5)))
    torch.cuda.synchronize()
    d_pose[0].copy_(d_seed)                # the same words from either (stage 1 from the seeds; stage 2 from stage 1's poses)
    refine(engine._stream())
    same = all(bool(torch.equal(words_of(r, N, outside), words[i])) for i, r in enumerate(rows))
    # what the other route needs besides its launches: the rows on the host and the arg-min there
    t0 = time.perf_counter()
    for r, n in zip(rows, per):
        h = r.cpu().numpy()
        cost = h[:, 6].astype(np.uint64) + (h[:, 4] - h[:, 3]).astype(np.uint64) * np.uint64(outside)
        cost.reshape(N, n).argmin(axis=1)
    host_ms = 1e3 * (time.perf_counter() - t0)
    ratio = t["slam2d_score_poses over the candidates, both stages"] / t["slam2d_refine_poses, both stages"]
    emit(dict(what="the same words from either; the other route's download and host arg-min, wall ms (once)", **common, equal=same, host_argmin_ms=round(host_ms, 2), launch_ratio_score_over_refine=round(ratio, 3)))
    return same


def track(pkg, sm, window, true, log, emit):
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
    tr = pkg.Tracker(sm, window)
    loc = pkg.Localiser(sm, window, particles=4096, sigma=(0.03, 0.03, 0.02), temperature=64.0, seed=1)
    out = {}

    def run_tracker():
        tr.set_pose(start)
        out["tracker"] = tr.run(log)

    def run_localiser():
        loc.scan = 0
        loc.seed_at(start, (0.1, 0.1, 0.05))
        out["localiser"] = loc.run(log)

    a, b = wall(run_tracker), wall(run_localiser)
    err = lambda poses: [float(np.hypot(p[0] - r["x"], p[1] - r["y"])) for p, r in zip(poses, true)]
    et, el = err([r.pose for r in out["tracker"]]), err([r["mean_pose"] for r in out["localiser"]])
    emit(dict(what="a log end to end, wall ms per scan (median, min, max of 7 runs)", scans=len(log), beams=len(log[0]["range"]),
              tracker_run_ms_per_scan=a, localiser_run_4096_ms_per_scan=b,
              tracker_error_m=dict(mean=round(float(np.mean(et)), 4), max=round(max(et), 4)),
              localiser_error_m=dict(mean=round(float(np.mean(el)), 4), max=round(max(el), 4))))


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

    import localise
    true, log, grid, window = localise.synthetic(40)
    og = pkg.map_from_poses(true, **grid)
    sm = pkg.ScanMatcher(og, *localise.SM_PARAMS)
    walk = np.array([[r["x"], r["y"], r["theta"]] for r in true])
    scans = np.array([r["range"] for r in true], dtype=np.float64)
    sm.refinePoses(walk[:1], scans[0], window=window)          # builds the covering level's field
    lv, eng = sm.last_cover["level"], og.engine()
    fr = lv.frames()[0]
    emit(dict(what="scene", field=[int(fr["fh"]), int(fr["fw"])], beams=scans.shape[1], in_range_mean=round(float((scans < og.lidarMaxRange).sum(axis=1).mean()), 1),
              device=torch.cuda.get_device_name(0)))
    stages = matcher.default_stages(lv.step)
    ok = True
    for N in args.seeds:
        ok &= measure(N, eng, lv, walk, scans, stages, sm.outside_cost_of(lv), emit)
    track(pkg, sm, window, true, log, emit)
    if not ok:
        raise SystemExit("the words of slam2d_refine_poses differ from those of the score_poses rows")


if __name__ == "__main__":
    main()
