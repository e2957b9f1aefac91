"""The map update and the matcher on the MI355X with lidar inputs the default-sensor fixtures never hold
(tests/golden/sensor_edges.py: NaN / inf / 0 / negative / subnormal ranges, wall edges exactly on a cell radius and on the
radial band boundary, beam counts next to the launch-shape thresholds, fields of view from pi/2 to 2 pi, window steps that
are not the map unit, headings in [-4 pi, 4 pi], half-cell poses, growth inside the update) against the CPU oracle, which
tests/test_oracle_sensor_edges.py pins to the reference on the same inputs.  Counts, limits, growth logs, cell lists and
arg-max bit-exact; cubes and confidences at test_gpu_parity.py's bars.  Needs an MI355X: run with ``-m gpu``."""
import ctypes as C
import importlib

import numpy as np
import pytest

import codec
import sensor_edges as se
from conftest import load_golden
from oracle import slam_oracle as so
from test_gpu_parity import RTOL, RTOL_TIGHT

pytestmark = pytest.mark.gpu
E = importlib.import_module("slam-2d-lidar-scan_amd.engine")
DEVICE = "cuda:0"

# every sensor of the fixture, then the first one's geometry at beam counts next to the launch-shape thresholds
SENSOR_CASES = [(i, None) for i in range(len(se.SENSORS))] + [(0, b) for b in se.EXTRA_BEAMS]
SENSOR_IDS = [f"s{i}" if b is None else f"b{b}" for i, b in SENSOR_CASES]


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


def _ogP(s):
    return [s["size_m"], s["size_m"], {"x": 0.0, "y": 0.0}, s["unit"], s["fov"], s["R"], s["beams"], s["wall"]]


def _engine(s, P, wide=False):
    lidar = E.LidarModel.get(s["unit"], s["R"], s["fov"], s["beams"], s["wall"])
    maps = [E.MapState.create(s["size_m"], s["size_m"], {"x": 0.0, "y": 0.0}, s["unit"], DEVICE) for _ in range(P)]
    if wide:
        for m in maps:
            m.promote()
    return E.ParticleEngine(lidar, maps, DEVICE)


def _assert_counts(m, og, what):
    gv, gt = m.download()
    assert gv.shape == og.visited.shape, what
    bad = np.argwhere((gv != og.visited) | (gt != og.total))
    assert bad.size == 0, (f"{len(bad)} cells differ, first (row, col) {bad[0]}: got {gv[tuple(bad[0])]:.0f}/{gt[tuple(bad[0])]:.0f} "
                           f"want {og.visited[tuple(bad[0])]:.0f}/{og.total[tuple(bad[0])]:.0f}; {what}")
    return gv, gt


def _assert_bits(m, gv, gt, what):
    """The occupancy bits the update kernel maintains incrementally == 2 * visited > total of the downloaded counts."""
    bits = m.bits.cpu().numpy().view(np.uint32)
    got = ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(m.rows, -1)[:, :m.cols].astype(bool)
    assert np.array_equal(got, 2 * gv > gt), what


def _unit_step(s):
    return E.LidarModel.get(s["unit"], s["R"], s["fov"], s["beams"], s["wall"]).xs_step() == s["unit"]


# ---------------------------------------------------------------------------------------------------------------------------
# B.1  k_grid_update itself
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 9, 17])
@pytest.mark.parametrize("case", SENSOR_CASES, ids=SENSOR_IDS)
def test_grid_update_matches_oracle(pkg, case, P):
    """slam2d_grid_update (and its fused forms with the normaliser) for P particles at DIFFERENT poses in one launch, two scans
    with the planted ranges, narrow and 64-bit maps, against GridOracle.update_cell_major per particle; the occupancy bits
    after each update.  Poses: off and on the lattice for a window step equal to the unit; for the other sensors also on half
    cells -- there every window column keeps a map index of its own (asserted on the oracle's indices first), so the kernel's
    non-lattice index path and its exact-division fallback are compared, not the drop-in's detour."""
    import torch
    i, beams = case
    seed = 41000 + 100 * SENSOR_CASES.index(case) + P
    rs = np.random.RandomState(seed)
    s = se.sensor(i, beams)
    lut = se.lut_of(s)
    unit_step = _unit_step(s)
    kinds = ("off", "on") if unit_step else ("off", "on", "half_x", "half_xy")
    oracles = [se.grid_of(s, lut) for _ in range(P)]
    engines = dict(narrow=_engine(s, P), wide=_engine(s, P, wide=True), fused=_engine(s, P), fused_local=_engine(s, P))
    st = {k: dict(logw=torch.full((P,), -np.log(P), dtype=torch.float64, device=DEVICE), w=torch.zeros(P, dtype=torch.float64, device=DEVICE),
                  stats=torch.zeros(2, dtype=torch.float64, device=DEVICE), part=torch.zeros(3, dtype=torch.float64, device=DEVICE))
          for k in ("fused", "fused_local")}
    for scan in range(2):
        poses = [se.pose_of(rs, s, oracles[0], kinds[(p + scan) % len(kinds)],
                            se.half_integer_theta(rs, lut) if p % 4 == 3 else None) for p in range(P)]
        ranges = se.random_ranges(rs, s)
        pk, pb = se.plant(rs, s, lut, poses[0][2], ranges)
        whats = []
        for p, (x, y, th) in enumerate(poses):
            reading = {"x": x, "y": y, "theta": th, "range": ranges}
            what = f"seed {seed} scan {scan} particle {p}: " + se.describe(s, reading, pk, pb)
            xi, yi = oracles[p].convertRealXYToMapIdx(x + lut.xs, y + lut.xs)
            assert len(np.unique(xi)) == lut.width and len(np.unique(yi)) == lut.width, "premise: one map index per window column; " + what
            oracles[p].update_cell_major(reading)
            whats.append(what)
        conf = rs.normal(-30.0, 5.0, P)
        for name, eng in engines.items():
            d_pose, d_rng = eng.to_device(np.array(poses)), eng.to_device(ranges)
            if name == "fused":
                d_conf = eng.to_device(conf)
                eng.grid_update_weights(d_pose, 3, d_rng, st[name]["logw"], d_conf.data_ptr(), 1, st[name]["w"], st[name]["stats"])
            elif name == "fused_local":
                d_conf = eng.to_device(conf)
                eng.grid_update_weights_local(d_pose, 3, d_rng, st[name]["logw"], d_conf.data_ptr(), 1, st[name]["part"])
            else:
                eng.grid_update(d_pose, 3, d_rng)
            flags = eng.take_flags()
            assert not flags.any(), (name, flags, whats[0])
            for p in range(P):
                gv, gt = _assert_counts(eng.maps[p], oracles[p], f"{name}: {whats[p]}")
                _assert_bits(eng.maps[p], gv, gt, f"{name} bits: {whats[p]}")
        for p in range(P):              # the fused launches: the same arrays as the separate call, padding included
            for name in ("fused", "fused_local"):
                assert torch.equal(engines["narrow"].maps[p].cells, engines[name].maps[p].cells), f"{name}: {whats[p]}"
                assert torch.equal(engines["narrow"].maps[p].bits, engines[name].maps[p].bits), f"{name}: {whats[p]}"


@pytest.mark.parametrize("n", [5 * i + se.POSE_KINDS.index("grow") for i in range(len(se.SENSORS))],
                         ids=[f"s{i}" for i in range(len(se.SENSORS))])
def test_grid_update_stale_index_launch_matches_reference(pkg, n):
    """The pose that makes the map grow on both low sides INSIDE the update, through slam2d_grid_update's stale-index launch
    (LidarModel.grow_for_update's per-beam shifts), narrow and 64-bit maps: the reference's own counts and limits from the
    fixture, and the oracle's growth log."""
    z = load_golden("sensor_edges.npz")
    pre = f"u{n}_"
    unit, R, wall, fov, beams, size_m = z[pre + "sensor"]
    s = dict(unit=float(unit), R=float(R), wall=float(wall), fov=float(fov), beams=int(beams), size_m=float(size_m))
    x, y, th = (float(v) for v in z[pre + "pose"])
    ranges = z[pre + "ranges"]
    reading = {"x": x, "y": y, "theta": th, "range": ranges}
    what = se.describe(s, reading, list(z[pre + "plant_kinds"]), z[pre + "plant_beams"])
    og = se.grid_of(s)
    og.updateOccupancyGrid(dict(reading))
    want_v, want_t = codec.unpack_counts(z[pre + "after"])
    assert np.array_equal(og.visited, want_v) and np.array_equal(og.total, want_t)
    for wide in (False, True):
        eng = _engine(s, 1, wide=wide)
        m = eng.maps[0]
        shifts = eng.lidar.grow_for_update(m, x, y, th, ranges)
        assert (shifts is not None) == bool(og.growth_log), what
        eng.refresh_bits()
        eng.grid_update(eng.to_device([[x, y, th]]), 3, eng.to_device(ranges),
                        None if shifts is None else eng.to_device(shifts[None], dtype=np.int32))
        flags = eng.take_flags()
        assert not flags.any(), (flags, what)
        assert m.growth_log == og.growth_log, what
        assert [m.lim_x[0], m.lim_x[1], m.lim_y[0], m.lim_y[1]] == list(z[pre + "lims"]), what
        _assert_counts(m, og, f"wide={wide}: {what}")


# ---------------------------------------------------------------------------------------------------------------------------
# B.2  k_occ_extent / k_map_scans
# ---------------------------------------------------------------------------------------------------------------------------
def _five_readings(seed, i, beams):
    """One reading of every pose kind (off / on the lattice, half cell on one and on both axes, growing), planted ranges."""
    out = []
    for k, kind in enumerate(se.POSE_KINDS):
        s, lut, reading, kinds, pbeams = se.update_case(seed + k, i, kind, half_theta=k % 2 == 1, beams=beams)
        out.append((reading, se.describe(s, reading, kinds, pbeams)))
    return s, out


@pytest.mark.parametrize("case", SENSOR_CASES, ids=SENSOR_IDS)
def test_update_many_and_extents_match_oracle(pkg, case):
    """OccupancyGrid.update_many (slam2d_occ_extent + slam2d_map_scans) over one reading of every pose kind -- half cells
    and the growing pose included -- with the planted ranges == ``for r in readings: oracle.updateOccupancyGrid(r)``: counts,
    limits, growth log; the extents of every beam's occupied points == LidarModel.occ_extents_host; map_from_poses the same
    from a map centred on the first pose."""
    import torch
    i, beams = case
    seed = 52000 + 10 * SENSOR_CASES.index(case)
    s, rd = _five_readings(seed, i, beams)
    readings = [r for r, _ in rd]
    what = " | ".join(w for _, w in rd)
    og = pkg.OccupancyGrid(*_ogP(s)[:4], s["fov"], s["beams"], s["R"], s["wall"])
    ref = se.grid_of(s)
    og.update_many(readings)
    for r in readings:
        ref.updateOccupancyGrid(dict(r))
    assert og.map.growth_log == ref.growth_log and (ref.growth_log or s["beams"] <= 3), what
    assert og.mapXLim == ref.mapXLim and og.mapYLim == ref.mapYLim, what
    _assert_counts(og.map, ref, what)
    # extents
    eng = og.engine()
    poses = np.array([[r["x"], r["y"], r["theta"]] for r in readings])
    ranges = np.array([r["range"] for r in readings])
    d_pose, d_rng = eng.to_device(poses), eng.to_device(ranges)
    d_ext = torch.empty((len(readings), s["beams"], 4), dtype=torch.float64, device=og.device)
    E._lib.check(E._lib.lib().slam2d_occ_extent(C.byref(eng.lidar_c), len(readings), E._ptr(d_pose), 3, E._ptr(d_rng), E._ptr(d_ext),
                                                E._stream()), "slam2d_occ_extent")
    got = d_ext.cpu().numpy()
    want = og.lidar.occ_extents_host(poses, ranges)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, f"extent of (scan, beam) {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}; {what}"
    # map_from_poses: the same scans into a map centred on the first pose
    first = readings[1]
    rest = [readings[1], readings[2], readings[3], readings[0]]
    og2 = pkg.map_from_poses(rest, s["size_m"], s["size_m"], s["unit"], s["fov"], s["R"], s["wall"])
    ref2 = so.GridOracle(s["size_m"], s["size_m"], {"x": first["x"], "y": first["y"]}, s["unit"], s["fov"], s["beams"], s["R"], s["wall"])
    for r in rest:
        ref2.updateOccupancyGrid(dict(r))
    assert og2.map.growth_log == ref2.growth_log and og2.mapXLim == ref2.mapXLim and og2.mapYLim == ref2.mapYLim, what
    _assert_counts(og2.map, ref2, "map_from_poses: " + what)


# ---------------------------------------------------------------------------------------------------------------------------
# B.3  the matcher
# ---------------------------------------------------------------------------------------------------------------------------
# path: (bnb, prune, environment, search radius in cells, Slam2dLevel.bnb_levels the path must end up with).  Two-level bounds
# need a cube edge of at least 17 poses (8 cells), the angle bounds one of at most 5 (2 cells); everything else runs 9 x 9.
MATCH_PATHS = {"full": (False, False, {}, 4, 0), "lazy": (False, False, {}, 4, 0), "pruned": (False, True, {}, 4, 0),
               "bnb": (True, False, {"SLAM2D_BNB_LEVELS": "1"}, 4, 1), "bnb_pruned": (True, True, {"SLAM2D_BNB_LEVELS": "1"}, 4, 1),
               "bnb_two_level": (True, False, {"SLAM2D_BNB_LEVELS": "2"}, 8, 2), "angle_bounds": (True, False, {}, 2, 3)}
MATCH_CASES = [(i, None, False) for i in range(len(se.SENSORS))] + [(0, None, True), (4, None, True)] + \
              [(0, b, False) for b in se.EXTRA_BEAMS]
MATCH_IDS = [(f"s{i}" if b is None else f"b{b}") + ("_only_non_returns" if o else "") for i, b, o in MATCH_CASES]


@pytest.mark.parametrize("path", sorted(MATCH_PATHS))
@pytest.mark.parametrize("case", MATCH_CASES, ids=MATCH_IDS)
def test_match_matches_oracle(pkg, case, path, monkeypatch):
    """One search level on a mapped synthetic world with the planted ranges (and with a scan of nothing but NaN / inf /
    >= max) through the full sweep, the lazy match, the prior-pruned match and the branch and bound variants (one level of
    pose-tile bounds, with pruning, two levels, the angle bounds) -- each asserted to be the path that ran --, two particles
    (one without a heading prior), against MatcherOracle.searchToMatch: arg-max, pose, confidence; the per-angle cell lists
    and the cube where the path produces them."""
    i, beams, only_non = case
    bnb, prune, env, cells, levels = MATCH_PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seed = 63000 + MATCH_CASES.index(case)
    s, lut, (v, t), est0, ranges, kinds, pbeams = se.matcher_case(seed, i, beams=beams, only_non_returns=only_non)
    smP = list(se.sm_params(s, cells))
    unit = s["unit"]
    est = np.array([est0, (est0[0] - unit, est0[1] + 2 * unit, est0[2] - 0.8 * s["fov"] / s["beams"])])
    dist, psi = 2.2 * unit, [0.3, None]
    what = se.describe(s, {"x": est0[0], "y": est0[1], "theta": est0[2], "range": ranges}, kinds, pbeams) + f"; path {path}"
    ogo = se.grid_of(s, lut)
    ogo.visited[:], ogo.total[:] = v, t
    smo = so.MatcherOracle(ogo, *smP)
    pf = pkg.ParticleFilter(2, _ogP(s), smP, growable=False, rng=np.random.RandomState(0), bnb=bnb)
    for m in pf.engine.maps:
        m.upload(v, t)
    eng, lv = pf.engine, pf.coarse
    assert lv.nx == 2 * cells + 1 and lv.bnb_levels == levels and lv.bnb == (levels in (1, 2)), (lv.nx, lv.bnb, lv.bnb_levels, path)
    d_est, d_rng, d_psi = eng.to_device(est), eng.to_device(ranges), eng.to_device(eng.psi_table(psi))
    if path == "full":
        eng.field_build(lv, d_est, 3)
        eng.sweep(lv, d_est, 3, d_rng, dist, d_psi, None, pf.m_coarse)
    else:
        eng.match(lv, d_est, 3, d_rng, dist, d_psi, None, pf.m_coarse, prune=prune)
    flags = eng.take_flags()
    assert not (flags & E._lib.FATAL_FLAGS).any(), (flags, what)
    got = eng.read_matches(pf.m_coarse)
    for p in range(2):
        xr, yr, prob = smo.frameSearchSpace(est[p, 0], est[p, 1], unit, smP[2], smP[6])
        mo, cube, conf = smo.searchToMatch(prob, est[p, 0], est[p, 1], est[p, 2], ranges, xr, yr, smP[0], smP[1], unit, dist, psi[p],
                                           fineSearch=False, matchMax=True)
        assert ogo.growth_log == []
        assert cube.shape == (lv.ntheta, lv.nx, lv.nx), what
        px, py = smo.covertMeasureToXY(est[p, 0], est[p, 1], est[p, 2], ranges)
        assert (len(px) == 0) == only_non
        for it, th in enumerate(smo.theta_range(smP[1])):
            cells = smo.unique_cells(est[p, 0], est[p, 1], px, py, th, xr[0], yr[0], unit)
            cy, cx = lv.cells_of(p, it)
            assert sorted(zip(cx.tolist(), cy.tolist())) == sorted(map(tuple, cells.tolist())), f"particle {p} theta {it}: {what}"
        assert int(got["argmax"][p]) == int(cube.argmax()), f"particle {p}: {what}"
        assert (got["x"][p], got["y"][p], got["theta"][p]) == (mo["x"], mo["y"], mo["theta"]), f"particle {p}: {what}"
        # the confidence is a sum of exp(score): its RELATIVE error is the scores' ABSOLUTE error, i.e. up to |score| (~ 100
        # here) times the cube's relative bar -- the suite's bar for confidences is RTOL (test_sweep_matches_reference)
        np.testing.assert_allclose(got["confidence"][p], conf, rtol=RTOL, err_msg=what)
        if path in ("full", "lazy"):
            np.testing.assert_allclose(lv.cube(p), cube, rtol=RTOL_TIGHT, atol=0, err_msg=what)


# ---------------------------------------------------------------------------------------------------------------------------
# B.4  the batched filter where the window does not sit on the map's lattice
# ---------------------------------------------------------------------------------------------------------------------------
def _filter_scans(s, n, seed):
    """A short seeded walk with raycast scans in a synthetic world the size of the map, the first pose on the map's centre."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world = synth.make_world(s["size_m"], s["unit"], seed=seed, n_boxes=6)
    origin = (-s["size_m"] / 2, -s["size_m"] / 2)
    rs = np.random.RandomState(seed)
    out, pose = [], np.array([0.0, 0.0, 0.3])
    for k in range(n):
        ranges = synth.raycast(world, s["unit"], origin, tuple(pose), s["fov"], s["beams"], s["R"])
        out.append({"x": float(pose[0] + 0.02 * k), "y": float(pose[1] - 0.01 * k), "theta": float(pose[2]), "range": ranges})
        pose = pose + np.array([0.35 * np.cos(pose[2]), 0.35 * np.sin(pose[2]), rs.uniform(-0.1, 0.1)])
    return out


def _filter_sm(s):
    """7 x 7 coarse poses at two cells, 5 x 5 fine ones, a handful of angles."""
    return [6 * s["unit"], 0.1, 2, 0.1, 0.25, 0.3, 0.15, 2]


def _run_filter(pkg, s, readings, seed, P=3):
    pf = pkg.ParticleFilter(P, _ogP(s), _filter_sm(s), rng=np.random.RandomState(seed))
    out = []
    for count, raw in enumerate(readings, start=1):
        pf.updateParticles(raw, count)
        pf.weightUnbalanced()
        out.append((pf.prev_matched.copy(), np.array(pf.weights, dtype=np.float64)))
    maps = [codec.pack_counts(*m.download()) for m in pf.engine.maps]
    return out, maps, [(m.lim_x[0], m.lim_x[1], m.lim_y[0], m.lim_y[1]) for m in pf.engine.maps]


def _oracle_filter(s, readings, seed, P=3):
    pfo = so.ParticleFilterOracle(P, _ogP(s), _filter_sm(s), rng=np.random.RandomState(seed))
    out = []
    for count, raw in enumerate(readings, start=1):
        pfo.updateParticles(raw, count)
        pfo.weightUnbalanced()
        out.append((np.array([[p.prevMatchedReading[k] for k in ("x", "y", "theta")] for p in pfo.particles]),
                    np.array([p.weight for p in pfo.particles], dtype=np.float64)))
    return out, pfo


def test_batched_filter_on_a_non_unit_window_step_matches_oracle(pkg):
    """A ParticleFilter whose lidar range is no whole number of cells (0.07 m / 3 m: every map index through k_grid_update's
    non-lattice path): four scans against ParticleFilterOracle -- matched poses and final maps identical, weights within the
    bar -- and two runs identical."""
    s = dict(se.sensor(7), beams=90, size_m=30.1)            # int(30.1 / 0.07) = 430 cells: the window lies inside the map
    assert not _unit_step(s)
    readings = _filter_scans(s, 4, seed=7)
    want, pfo = _oracle_filter(s, readings, seed=3)
    runs = [_run_filter(pkg, s, readings, seed=3) for _ in range(2)]
    for (got, maps, lims) in runs:
        for k, ((gm, gw), (wm, ww)) in enumerate(zip(got, want)):
            assert np.array_equal(gm, wm), f"scan {k + 1}: {gm} vs {wm}"
            np.testing.assert_allclose(gw, ww, rtol=RTOL, err_msg=f"scan {k + 1}")
        for p, po in enumerate(pfo.particles):
            assert lims[p] == (po.og.mapXLim[0], po.og.mapXLim[1], po.og.mapYLim[0], po.og.mapYLim[1])
            bad = np.argwhere(maps[p] != codec.pack_counts(po.og.visited, po.og.total))
            assert bad.size == 0, f"particle {p}: {len(bad)} cells differ, first {bad[0]}"
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_batched_filter_refuses_a_first_pose_on_a_half_cell(pkg):
    """A map with an ODD number of cells per side (15 m at 0.2 m: 75) puts the first scan of every particle on a half cell on
    both axes, where rint's ties-to-even sends two window columns to one map index: the reference adds once per statement
    there (Utils/OccupancyGrid.py:149-152) and a per-cell update cannot (the matched poses then stay on half cells).  The
    batched filter refuses on the host, before anything is launched, every time; OccupancyGrid.updateOccupancyGrid
    (slam2d_map_scans) is exact at the same pose."""
    s = dict(unit=0.2, R=3.0, wall=0.6, fov=np.pi, beams=90, size_m=15)
    assert int(s["size_m"] / s["unit"]) % 2 == 1 and _unit_step(s)
    readings = _filter_scans(s, 3, seed=5)
    for _ in range(2):
        pf = pkg.ParticleFilter(3, _ogP(s), _filter_sm(s), rng=np.random.RandomState(3))
        with pytest.raises(E._lib.Slam2dError, match="half cell"):
            pf.updateParticles(readings[0], 1)
        for m in pf.engine.maps:                                    # nothing was written
            gv, gt = m.download()
            assert (gv == 1).all() and (gt == 2).all()
    og = pkg.OccupancyGrid(*_ogP(s)[:4], s["fov"], s["beams"], s["R"], s["wall"])
    ref = se.grid_of(s)
    og.updateOccupancyGrid(readings[0])
    ref.updateOccupancyGrid(dict(readings[0]))
    assert og.map.growth_log == ref.growth_log
    _assert_counts(og.map, ref, "drop-in at the half-cell pose")


@pytest.mark.parametrize("mode", ["plain", "stale_index", "fused"])
def test_grid_update_flags_a_particle_on_a_half_cell_and_leaves_its_map(pkg, mode):
    """slam2d_grid_update with particles on a half cell (one axis, both axes) between particles that are not: the former get
    SLAM2D_F_UPDATE_CELL_COLLISION and keep their maps bit for bit, the latter are updated as the oracle says -- twice the
    same.  Also through the stale-index launch (zero shifts) and the fused launch with the normaliser."""
    import torch
    s = se.sensor(0)
    lut = se.lut_of(s)
    rs = np.random.RandomState(77)
    kinds = ["off", "half_x", "on", "half_xy", "off"]
    P = len(kinds)
    og0 = se.grid_of(s, lut)
    poses = [se.pose_of(rs, s, og0, k) for k in kinds]
    ranges = se.random_ranges(rs, s)
    se.plant(rs, s, lut, poses[0][2], ranges)
    for _ in range(2):
        eng = _engine(s, P)
        d_pose, d_rng = eng.to_device(np.array(poses)), eng.to_device(ranges)
        if mode == "fused":
            logw = torch.full((P,), -np.log(P), dtype=torch.float64, device=DEVICE)
            eng.grid_update_weights(d_pose, 3, d_rng, logw, eng.to_device(np.zeros(P)).data_ptr(), 1,
                                    torch.zeros(P, dtype=torch.float64, device=DEVICE), torch.zeros(2, dtype=torch.float64, device=DEVICE))
        else:
            shift = np.zeros((P, s["beams"], 6), dtype=np.int32)
            shift[:, :, 4], shift[:, :, 5] = eng.maps[0].cols, eng.maps[0].rows
            eng.grid_update(d_pose, 3, d_rng, eng.to_device(shift, dtype=np.int32) if mode == "stale_index" else None)
        flags = eng.take_flags(fatal=0)
        for p, kind in enumerate(kinds):
            x, y, th = poses[p]
            og = se.grid_of(s, lut)
            if kind.startswith("half"):
                assert flags[p] == E._lib.F_UPDATE_CELL_COLLISION, (mode, p, flags)
            else:
                assert flags[p] == 0, (mode, p, flags)
                og.update_cell_major({"x": x, "y": y, "theta": th, "range": ranges})
            _assert_counts(eng.maps[p], og, f"{mode}: particle {p} ({kind}) pose {poses[p]}")
    with pytest.raises(E._lib.Slam2dError, match="half cell"):
        eng.grid_update(d_pose, 3, d_rng)
        eng.take_flags()


@pytest.mark.parametrize("mode", ["plain", "stale_index", "fused"])
def test_grid_update_flags_a_particle_without_a_map_index_and_leaves_its_map(pkg, mode):
    """slam2d_grid_update with a particle at x = NaN and one at x = 2e8 (map-index quotient 2e9: neighbouring window columns stay
    distinct there, so the collision test does not fire) between particles off and on the lattice: the former two have no map
    index an int can hold, get exactly SLAM2D_F_UPDATE_OUTSIDE_MAP and keep their maps bit for bit -- cell (0, 0) and the last
    column, where a converted NaN or a wrapped -1 would land, included; the latter two are updated as the oracle says -- twice
    the same.  Also through the stale-index launch (zero shifts, Python's wrap applied) and the fused launch."""
    import torch
    s = se.sensor(0)
    lut = se.lut_of(s)
    rs = np.random.RandomState(78)
    kinds = ["off", "nan_x", "huge_x", "on"]
    P = len(kinds)
    og0 = se.grid_of(s, lut)
    poses = [se.pose_of(rs, s, og0, "off" if k.endswith("_x") else k) for k in kinds]
    poses[1] = (float("nan"),) + poses[1][1:]
    poses[2] = (2e8,) + poses[2][1:]
    ranges = se.random_ranges(rs, s)
    se.plant(rs, s, lut, poses[0][2], ranges)
    for _ in range(2):
        eng = _engine(s, P)
        d_pose, d_rng = eng.to_device(np.array(poses)), eng.to_device(ranges)
        if mode == "fused":
            logw = torch.full((P,), -np.log(P), dtype=torch.float64, device=DEVICE)
            eng.grid_update_weights(d_pose, 3, d_rng, logw, eng.to_device(np.zeros(P)).data_ptr(), 1,
                                    torch.zeros(P, dtype=torch.float64, device=DEVICE), torch.zeros(2, dtype=torch.float64, device=DEVICE))
        else:
            shift = np.zeros((P, s["beams"], 6), dtype=np.int32)
            shift[:, :, 4], shift[:, :, 5] = eng.maps[0].cols, eng.maps[0].rows
            eng.grid_update(d_pose, 3, d_rng, eng.to_device(shift, dtype=np.int32) if mode == "stale_index" else None)
        flags = eng.take_flags(fatal=0)
        for p, kind in enumerate(kinds):
            x, y, th = poses[p]
            og = se.grid_of(s, lut)
            if kind.endswith("_x"):
                assert flags[p] == E._lib.F_UPDATE_OUTSIDE_MAP, (mode, p, flags)
            else:
                assert flags[p] == 0, (mode, p, flags)
                og.update_cell_major({"x": x, "y": y, "theta": th, "range": ranges})
            _assert_counts(eng.maps[p], og, f"{mode}: particle {p} ({kind}) pose {poses[p]}")
