#!/usr/bin/env python3
"""Goldens of the checks that once ran against a live checkout of the reference (tests/test_oracle_vs_reference.py and the
text-log test of tests/test_host_logic.py), so that those tests run from this repository alone:

* ``vs_reference.npz``: the reference's scan-matching flow (14 Intel scans, one matcher) and its FastSLAM flow (3 particles x
  9 scans, a resample after scan 6), poses, confidences, weights, trajectories and count maps (codec.pack_counts);
* ``csail_gfs_excerpt.npz``: the bytes of the head of the reference's CSAIL log (``gfs``) and of the JSON its own
  DataPreprocess/preprocess_gfs.py writes for it (``processed_json``; RUN in a scratch directory laid out the way its relative
  paths expect).

Only data the reference's programs read or wrote is stored, none of their text.  Usage: python tests/golden/make_golden_reference_checks.py <reference checkout>
"""
import contextlib
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import codec  # noqa: E402

REF_SM = (1.4, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 5)
N_SCANMATCH, N_FASTSLAM, FASTSLAM_PARTICLES, FASTSLAM_RESAMPLE_AT, FASTSLAM_SEED = 14, 9, 3, 6, 3
GFS_READINGS = 24


def intel_readings():
    z = np.load(os.path.join(HERE, "intel_gfs.npz"))
    rng = z["range_cm"].astype(np.float64) / 100.0
    return [{"x": float(p[0]), "y": float(p[1]), "theta": float(p[2]), "range": list(map(float, r))} for p, r in zip(z["pose"], rng)]


def flows(ref):
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path[:0] = [ref, os.path.join(ref, "Algorithm")]
    from Utils.OccupancyGrid import OccupancyGrid
    from Utils.ScanMatcher_OGBased import ScanMatcher
    import Utils.ScanMatcher_OGBased as sm_mod
    import FastSlam
    readings = intel_readings()
    out = {}
    # the scan-matching flow (Utils/ScanMatcher_OGBased.py's own driver loop)
    r0 = readings[0]
    og = OccupancyGrid(10, 10, r0, 0.02, np.pi, 180, 10, 0.1)
    sm = ScanMatcher(og, *REF_SM)
    xs, ys, poses, confs = [], [], [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for count, raw in enumerate(readings[:N_SCANMATCH], start=1):
            if count == 1:
                pr = pm = None
                matched, conf = raw, 1
            else:
                est, dist, psi, rawth = sm_mod.updateEstimatedPose(raw, prev_m, prev_r, pr, pm)
                matched, conf = sm.matchScan(est, dist, psi, count)
                pr, pm = rawth, sm_mod.getMovingTheta(matched, xs, ys)
            og.updateOccupancyGrid(matched)
            xs.append(matched["x"]); ys.append(matched["y"])
            prev_m, prev_r = matched, raw
            poses.append((matched["x"], matched["y"], matched["theta"])); confs.append(conf)
    out.update(sm_poses=np.array(poses, dtype=np.float64), sm_confs=np.array(confs, dtype=np.float64),
               sm_counts=codec.pack_counts(og.occupancyGridVisited, og.occupancyGridTotal),
               sm_X=np.asarray(og.OccupancyGridX[0], dtype=np.float64), sm_Y=np.asarray(og.OccupancyGridY[:, 0], dtype=np.float64))
    # the FastSLAM flow (Algorithm/FastSlam.py's ParticleFilter)
    u = 0.02
    ogP = [20, 20, readings[0], u, np.pi, 10, 180, 5 * u]
    np.random.seed(FASTSLAM_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        pf = FastSlam.ParticleFilter(FASTSLAM_PARTICLES, ogP, list(REF_SM))
        wr = []
        for c, r in enumerate(readings[:N_FASTSLAM], start=1):
            pf.updateParticles(r, c)
            pf.weightUnbalanced()
            wr.append([p.weight for p in pf.particles])
            if c == FASTSLAM_RESAMPLE_AT:
                pf.resample()
    out["fs_weights"] = np.array(wr, dtype=np.float64)
    for i, p in enumerate(pf.particles):
        out[f"fs_counts_{i}"] = codec.pack_counts(p.og.occupancyGridVisited, p.og.occupancyGridTotal)
        out[f"fs_xtraj_{i}"] = np.array(p.xTrajectory, dtype=np.float64)
    return out


def gfs_excerpt(ref):
    lines, n = [], 0
    with open(os.path.join(ref, "DataSet", "RawData", "csail.corrected.gfs")) as f:
        for line in f:
            lines.append(line)
            n += line.startswith("LASER_READING")
            if n == GFS_READINGS:
                break
    with tempfile.TemporaryDirectory() as tmp:
        for d in ("DataPreprocess", os.path.join("DataSet", "RawData"), os.path.join("DataSet", "PreprocessedData")):
            os.makedirs(os.path.join(tmp, d))
        with open(os.path.join(tmp, "DataSet", "RawData", "csail.corrected.gfs"), "w") as f:
            f.writelines(lines)
        subprocess.run([sys.executable, "-B", os.path.join(ref, "DataPreprocess", "preprocess_gfs.py")],
                       cwd=os.path.join(tmp, "DataPreprocess"), check=True)
        with open(os.path.join(tmp, "DataSet", "PreprocessedData", "csail_gfs"), "rb") as f:
            processed = f.read()
    np.savez_compressed(os.path.join(HERE, "csail_gfs_excerpt.npz"), gfs=np.frombuffer("".join(lines).encode(), np.uint8),
                        processed_json=np.frombuffer(processed, np.uint8))


def main():
    ref = os.path.abspath(sys.argv[1])
    gfs_excerpt(ref)
    np.savez_compressed(os.path.join(HERE, "vs_reference.npz"), **flows(ref))
    print("written")


if __name__ == "__main__":
    main()
