#!/usr/bin/env python3
"""Generate tests/golden/mapping.npz by importing the reference: its ``Utils/OccupancyGrid.py:main`` flow (mapping from the
recorded poses) on the raw Intel log -- 10 m starting map centred on the first pose, unitGridSize 0.02, lidarFOV pi,
lidarMaxRange 10, wallThickness 7 * 0.02, all 910 scans.

Runs ONLY in the development container (needs the reference checkout); the fixture it writes is committed next to it.
Recorded: the growth sequence, the final shape and limits, and SHA-256 of the float64 bytes of occupancyGridVisited /
occupancyGridTotal after scans 1, 50, 200 and 910 (the final arrays are 4458 x 4458 float64: hashes, not arrays).

    python tests/golden/make_golden_mapping.py
"""
import hashlib
import json
import os
import sys
import time

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SLAM2D_REFERENCE", "/root/reference")
sys.path[:0] = [REF, HERE]

import numpy as np  # noqa: E402
from Utils.OccupancyGrid import OccupancyGrid  # noqa: E402  (reference)

CHECKPOINTS = (1, 50, 200, 910)
PARAMS = dict(mapXLength=10, mapYLength=10, unitGridSize=0.02, lidarFOV=np.pi, lidarMaxRange=10)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def load_intel():
    d = json.load(open(os.path.join(REF, "DataSet/PreprocessedData/intel_gfs")))["map"]
    return [d[k] for k in sorted(d.keys())]


def check_fixture(readings):
    """The committed intel_gfs.npz decodes to exactly these readings (the tests run from it)."""
    z = np.load(os.path.join(HERE, "intel_gfs.npz"))
    assert len(readings) == len(z["pose"])
    for r, p, cm in zip(readings, z["pose"], z["range_cm"]):
        assert (r["x"], r["y"], r["theta"]) == tuple(map(float, p))
        assert list(map(float, cm.astype(np.float64) / 100.0)) == [float(v) for v in r["range"]]


def main():
    readings = load_intel()
    check_fixture(readings)
    p = PARAMS
    unit = p["unitGridSize"]
    og = OccupancyGrid(p["mapXLength"], p["mapYLength"], readings[0], unit, p["lidarFOV"], len(readings[0]["range"]),
                       p["lidarMaxRange"], 7 * unit)
    growth = []
    expand = og.expandOccupancyGrid

    def logged(direction):                      # (records the step, then runs the reference's method unchanged)
        rows, cols = og.occupancyGridVisited.shape
        growth.append((direction, int(cols / 5) if direction in (1, 2) else int(rows / 5)))
        expand(direction)
    og.expandOccupancyGrid = logged

    out = {}
    t0 = time.time()
    for n, r in enumerate(readings, 1):
        og.updateOccupancyGrid(r)
        if n in CHECKPOINTS:
            out[f"visited_sha_{n}"] = np.array(digest(og.occupancyGridVisited))
            out[f"total_sha_{n}"] = np.array(digest(og.occupancyGridTotal))
            out[f"shape_{n}"] = np.array(og.occupancyGridVisited.shape, dtype=np.int64)
            out[f"lim_{n}"] = np.array([og.mapXLim[0], og.mapXLim[1], og.mapYLim[0], og.mapYLim[1]])
            out[f"growth_count_{n}"] = np.array(len(growth))
    seconds = time.time() - t0
    out["growth"] = np.array(growth, dtype=np.int64).reshape(-1, 2)
    out["params"] = np.array([p["mapXLength"], p["mapYLength"], unit, p["lidarFOV"], p["lidarMaxRange"], 7 * unit])
    out["checkpoints"] = np.array(CHECKPOINTS, dtype=np.int64)
    out["reference_seconds"] = np.array(seconds)
    path = os.path.join(HERE, "mapping.npz")
    np.savez_compressed(path, **out)
    print(f"mapping.npz: {os.path.getsize(path)} bytes; shape {og.occupancyGridVisited.shape}, {len(growth)} growth steps, "
          f"reference {seconds:.1f} s ({1e3 * seconds / len(readings):.1f} ms per scan)")


if __name__ == "__main__":
    main()
