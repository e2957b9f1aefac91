"""The CPU oracle against the reference on lidar inputs the default-sensor fixtures never hold
(tests/golden/make_golden_sensor_edges.py -> sensor_edges.npz): NaN / inf / 0 / negative / subnormal ranges, ranges whose
wall edge sits exactly on a cell radius or on the radial band boundary, beam counts next to each other, fields of view from
pi/2 to 2 pi, ranges that are no whole number of cells, headings in [-4 pi, 4 pi], half-cell poses, growth inside the update.
CPU only; bit for bit, as test_oracle_golden.py is for the default sensor."""
import hashlib

import numpy as np
import pytest

import codec
import sensor_edges as se
from conftest import load_golden
from oracle import slam_oracle as so

Z = load_golden("sensor_edges.npz")
N_UPDATE, N_MATCH = int(Z["n_update"]), int(Z["n_match"])


def _sensor(a):
    unit, R, wall, fov, beams, size_m = a
    return dict(unit=float(unit), R=float(R), wall=float(wall), fov=float(fov), beams=int(beams), size_m=float(size_m))


def _update_case(n):
    pre = f"u{n}_"
    s = _sensor(Z[pre + "sensor"])
    x, y, th = Z[pre + "pose"]
    reading = {"x": float(x), "y": float(y), "theta": float(th), "range": Z[pre + "ranges"]}
    kind = se.POSE_KINDS[int(Z[pre + "case"][2])]
    return pre, s, reading, kind, se.describe(s, reading, list(Z[pre + "plant_kinds"]), Z[pre + "plant_beams"])


def test_fixture_holds_what_it_should():
    """Every sensor x pose kind is there (nothing the reference could not run), every planted kind occurs, the two on-radius
    ranges do put a wall edge exactly on the radius of a cell their beam owns, and the generator is reproducible from its
    seeds (the helper the GPU tests build further cases with is the one that made the fixture)."""
    assert N_UPDATE == len(se.SENSORS) * len(se.POSE_KINDS) and N_MATCH == len(se.SENSORS) + 2
    assert len(Z["left_out"]) * 10 <= N_UPDATE + N_MATCH + len(Z["left_out"])
    seen = set()
    for n in range(N_UPDATE):
        pre, s, reading, kind, what = _update_case(n)
        seed, i, k, half_theta = (int(v) for v in Z[pre + "case"])
        s2, lut, r2, kinds, pbeams = se.update_case(seed, i, kind, bool(half_theta))
        assert s2 == s and (r2["x"], r2["y"], r2["theta"]) == (reading["x"], reading["y"], reading["theta"]), what
        assert np.array_equal(r2["range"], reading["range"], equal_nan=True) and kinds == list(Z[pre + "plant_kinds"]), what
        seen.update(kinds)
        own = set(se.owned_cells(lut, reading["theta"]))       # (beam, radius) pairs
        for kname, b in zip(kinds, pbeams):
            rg = reading["range"][b]
            if kname == "lo_on_radius":
                assert (int(b), rg - s["wall"] / 2) in own, what
            if kname == "hi_on_radius":
                assert (int(b), rg + s["wall"] / 2) in own, what
        if half_theta:
            v = reading["theta"] / (2 * np.pi) * lut.num_spokes
            assert abs(abs(v - np.floor(v)) - 0.5) < 1e-9, what
    assert seen == set(se.PLANT_KINDS)


@pytest.mark.parametrize("n", range(N_UPDATE))
def test_update_exact(n):
    """GridOracle.updateOccupancyGrid == the reference's, counts and limits; update_cell_major too where the window lies
    inside the map and the pose is off the half cell (one window cell per map cell)."""
    pre, s, reading, kind, what = _update_case(n)
    lut = se.lut_of(s)
    og = se.grid_of(s, lut)
    twin = se.grid_of(s, lut)
    og.updateOccupancyGrid(dict(reading))
    want = Z[pre + "after"]
    after = codec.pack_counts(og.visited, og.total)
    assert after.shape == want.shape, what
    bad = np.argwhere(after != want)
    assert bad.size == 0, f"{len(bad)} cells differ, first (row, col) {bad[0]}: {what}"
    assert [og.mapXLim[0], og.mapXLim[1], og.mapYLim[0], og.mapYLim[1]] == list(Z[pre + "lims"]), what
    assert (og.growth_log != []) == (want.shape != twin.visited.shape)
    if kind in ("off", "on"):
        twin.update_cell_major(dict(reading))
        bad = np.argwhere(codec.pack_counts(twin.visited, twin.total) != want)
        assert bad.size == 0, f"cell-major: {len(bad)} cells differ, first (row, col) {bad[0]}: {what}"


@pytest.mark.parametrize("n", range(N_MATCH))
def test_match_exact(n):
    """covertMeasureToXY, frameSearchSpace and searchToMatch of MatcherOracle == the reference's with the planted ranges
    (and with a scan of nothing but NaN / inf / >= max): endpoints, field, cube, arg-max, confidence, pose."""
    pre = f"m{n}_"
    s = _sensor(Z[pre + "sensor"])
    only_non = int(Z[pre + "case"][2])
    est, ranges = tuple(float(v) for v in Z[pre + "est"]), Z[pre + "ranges"]       # (everything from the fixture: no generator code)
    what = se.describe(s, {"x": est[0], "y": est[1], "theta": est[2], "range": ranges}, list(Z[pre + "plant_kinds"]), Z[pre + "plant_beams"])
    og = se.grid_of(s)
    og.visited, og.total = codec.unpack_counts(Z[pre + "map"])
    assert og.visited.shape == (len(og.Y), len(og.X))
    a = Z[pre + "sm"]
    sm = so.MatcherOracle(og, a[0], a[1], a[2], a[3], a[4], a[5], a[6], int(a[7]))
    px, py = sm.covertMeasureToXY(est[0], est[1], est[2], ranges)
    assert np.array_equal(px, Z[pre + "px"]) and np.array_equal(py, Z[pre + "py"]), what
    assert (len(px) == 0) == bool(only_non)
    xr, yr, prob = sm.frameSearchSpace(est[0], est[1], s["unit"], a[2], a[6])
    assert og.growth_log == []
    assert np.array_equal(np.array(xr), Z[pre + "xr"]) and np.array_equal(np.array(yr), Z[pre + "yr"])
    assert list(prob.shape) == list(Z[pre + "prob_shape"]) and prob.min() == Z[pre + "prob_floor"]
    assert hashlib.sha256(np.ascontiguousarray(prob).tobytes()).digest() == Z[pre + "prob_sha"].tobytes(), what
    dist, psi = Z[pre + "prior"]
    matched, cube, conf = sm.searchToMatch(prob, est[0], est[1], est[2], ranges, xr, yr, a[0], a[1], s["unit"], float(dist),
                                           float(psi), fineSearch=False, matchMax=True)
    assert np.array_equal(cube, Z[pre + "cube"]), what
    assert int(cube.argmax()) == int(Z[pre + "pick"]) and conf == Z[pre + "conf"], what
    assert [matched["x"], matched["y"], matched["theta"]] == list(Z[pre + "matched"]), what
