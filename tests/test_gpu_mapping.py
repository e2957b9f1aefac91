"""Mapping from known poses on the MI355X (slam2d_occ_extent + slam2d_map_scans): OccupancyGrid.updateOccupancyGrid at
half-cell poses, OccupancyGrid.update_many and map_from_poses against the oracle and the reference's fixture."""
import hashlib
import importlib

import numpy as np
import pytest

from conftest import load_golden
from oracle import slam_oracle as so

pytestmark = pytest.mark.gpu

UNIT, R, FOV, BEAMS = 0.02, 10, np.pi, 180
WALL = 7 * UNIT


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _pair(pkg, length, init, unit=UNIT, wall=WALL):
    og = pkg.OccupancyGrid(length, length, init, unit, FOV, BEAMS, R, wall)
    ref = so.GridOracle(length, length, init, unit, FOV, BEAMS, R, wall)
    return og, ref


def _same(og, ref, what=""):
    v, t = og.occupancyGridVisited, og.occupancyGridTotal
    assert v.shape == ref.visited.shape, what
    assert np.array_equal(t, ref.total), (what, int((t != ref.total).sum()))
    assert np.array_equal(v, ref.visited), (what, int((v != ref.visited).sum()))
    assert og.mapXLim == ref.mapXLim and og.mapYLim == ref.mapYLim, what
    assert og.map.growth_log == ref.growth_log, what


def _half_cell(v):
    return abs(abs(v - np.floor(v)) - 0.5) < 1e-6


def test_half_cell_poses_through_the_dropin(pkg, intel_readings):
    """Ten raw Intel scans whose pose sits on a half cell at 0.02 and one synthetic pose on a half cell on both axes at 0.1,
    each through updateOccupancyGrid on a pre-sized map: the reference's counts after every scan (a statement adds once
    per element; statements add up)."""
    first = intel_readings[0]
    og, ref = _pair(pkg, 50, first)
    picked = []
    for n, r in enumerate(intel_readings):
        if len(picked) == 10:
            break
        ax, ay = (r["x"] - ref.mapXLim[0]) / UNIT, (r["y"] - ref.mapYLim[0]) / UNIT
        inside = r["x"] - R >= ref.mapXLim[0] and r["x"] + R <= ref.mapXLim[1] and \
            r["y"] - R >= ref.mapYLim[0] and r["y"] + R <= ref.mapYLim[1]
        if inside and (_half_cell(ax) or _half_cell(ay)):
            picked.append(n)
    assert len(picked) == 10
    for n in picked:
        og.updateOccupancyGrid(intel_readings[n])
        ref.updateOccupancyGrid(intel_readings[n])
        _same(og, ref, f"scan {n}")
    assert not ref.growth_log

    og, ref = _pair(pkg, 30, {"x": 0.0, "y": 0.0}, unit=0.1, wall=0.5)
    k = 113
    reading = dict(intel_readings[5], x=ref.mapXLim[0] + (k + 0.5) * 0.1, y=ref.mapYLim[0] + (k + 0.5) * 0.1)
    assert _half_cell((reading["x"] - ref.mapXLim[0]) / 0.1) and _half_cell((reading["y"] - ref.mapYLim[0]) / 0.1)
    og.updateOccupancyGrid(reading)
    ref.updateOccupancyGrid(reading)
    _same(og, ref, "synthetic (k + 0.5) unit pose")


def test_update_many_first_200_scans_from_the_10m_start(pkg, intel_readings):
    readings = intel_readings[:200]
    ref = so.GridOracle(10, 10, readings[0], UNIT, FOV, BEAMS, R, WALL)
    for r in readings:
        ref.updateOccupancyGrid(r)
    assert ref.growth_log                               # (growth and scan 1's stale indices are part of it)
    results = []
    for chunks in ([200], [1, 7, 50, 142], [200]):
        og = pkg.OccupancyGrid(10, 10, readings[0], UNIT, FOV, BEAMS, R, WALL)
        a = 0
        for c in chunks:
            og.update_many(readings[a:a + c])
            a += c
        _same(og, ref, f"chunks {chunks}")
        results.append((og.occupancyGridVisited, og.occupancyGridTotal, og.version))
    for v, t, _ in results[1:]:
        assert np.array_equal(v, results[0][0]) and np.array_equal(t, results[0][1])
    assert results[0][2] > 0                            # (growth bumped the grid's version)


def test_map_from_poses_whole_intel_log(pkg, intel_readings):
    z = load_golden("mapping.npz")
    og = pkg.map_from_poses(intel_readings)
    assert og.unitGridSize == UNIT and og.wallThickness == WALL
    assert og.map.growth_log == [tuple(g) for g in z["growth"].tolist()]
    assert og.occupancyGridVisited.shape == tuple(z["shape_910"])
    assert [og.mapXLim[0], og.mapXLim[1], og.mapYLim[0], og.mapYLim[1]] == z["lim_910"].tolist()
    assert _digest(og.occupancyGridVisited) == str(z["visited_sha_910"])
    assert _digest(og.occupancyGridTotal) == str(z["total_sha_910"])
    # the checkpoints on the way, in chunks
    og = pkg.map_from_poses(intel_readings[:1])
    assert _digest(og.occupancyGridTotal) == str(z["total_sha_1"])
    og.update_many(intel_readings[1:50])
    assert _digest(og.occupancyGridVisited) == str(z["visited_sha_50"]) and _digest(og.occupancyGridTotal) == str(z["total_sha_50"])
    og.update_many(intel_readings[50:200])
    assert _digest(og.occupancyGridVisited) == str(z["visited_sha_200"]) and _digest(og.occupancyGridTotal) == str(z["total_sha_200"])


def test_update_many_near_the_16_bit_limit(pkg, intel_readings):
    lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    readings = intel_readings[:40]
    og, ref = _pair(pkg, 40, readings[0], unit=0.1, wall=0.5)
    rs = np.random.RandomState(3)
    t = np.full(ref.total.shape, lib.COUNT_LIMIT - 4.0)
    t -= rs.randint(0, 4, size=t.shape)
    v = np.floor(t * rs.uniform(0.0, 1.0, size=t.shape))
    og.set_counts(v, t)
    ref.visited[:], ref.total[:] = v, t
    assert not og.map.wide
    og.update_many(readings)
    for r in readings:
        ref.updateOccupancyGrid(r)
    assert og.map.wide                                  # promoted before the launch
    assert int(ref.total.max()) > lib.COUNT_LIMIT       # (a 16-bit map would have carried)
    _same(og, ref, "near COUNT_LIMIT")
    assert not og.engine().take_flags().any()


def test_dropin_keeps_todays_kernel_off_half_cells(pkg, intel_readings):
    """Ground-truth poses (off the lattice, no half cell) and a lattice pose: updateOccupancyGrid keeps k_grid_update and
    the oracle's counts."""
    gt = load_golden("intel_corrected_pose.npz")["pose"]
    og, ref = _pair(pkg, 50, intel_readings[0])
    for n in (3, 40, 77, 150):
        r = dict(intel_readings[n], x=float(gt[n, 0]), y=float(gt[n, 1]), theta=float(gt[n, 2]))
        assert not og._needs_exact(r["x"], r["y"])
        og.updateOccupancyGrid(r)
        ref.updateOccupancyGrid(r)
        _same(og, ref, f"ground truth {n}")
    r = dict(intel_readings[9], x=ref.mapXLim[0] + 1000 * UNIT, y=ref.mapYLim[0] + 1100 * UNIT)
    assert not og._needs_exact(r["x"], r["y"])
    og.updateOccupancyGrid(r)
    ref.updateOccupancyGrid(r)
    _same(og, ref, "lattice pose")
