"""slam2d_predict_scan on the MI355X against the definition in NumPy (tests/predict_yardstick.py): every comparison is
np.array_equal on first, far and cells, +-inf included -- the result is a min, a max and a count of tabulated radii, so there is
no tolerance.  Base lidar: unit 0.1 m, range 4 m, FOV pi, 60 beams, wall 0.5: an 81 x 81 window, 120 spokes, 4 radial bands."""
import ctypes
import importlib

import numpy as np
import pytest

import predict_yardstick as yard
from oracle import slam_oracle as so
from test_predict_host import check_round_trip, scan_ranges

pytestmark = pytest.mark.gpu

UNIT, R, FOV, BEAMS, WALL = 0.1, 4.0, np.pi, 60, 0.5
SIZE = 20
ORIGIN = (-SIZE / 2, -SIZE / 2)
INIT = {"x": 0.0, "y": 0.0}


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


def _same(got, want, what=""):
    first, far, cells = want
    assert got["first"].shape == first.shape, what
    assert np.array_equal(got["cells"], cells), (what, np.argwhere(got["cells"] != cells)[:5].tolist())
    assert np.array_equal(got["first"], first), (what, np.argwhere(got["first"] != first)[:5].tolist())
    assert np.array_equal(got["far"], far), (what, np.argwhere(got["far"] != far)[:5].tolist())
    assert np.array_equal(got["hit"], cells > 0), what
    assert not np.isnan(got["first"]).any() and not np.isnan(got["far"]).any(), what


def _oracle_of_grid(og, fov=FOV, beams=BEAMS, max_range=R, unit=UNIT, wall=WALL):
    return yard.oracle_of(og.occupancyGridVisited, og.occupancyGridTotal, og.mapXLim, og.mapYLim, unit, fov, beams, max_range, wall)


def _walk():
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world = synth.make_world(SIZE, UNIT, seed=3, n_boxes=25)
    poses = synth.random_walk(world, UNIT, ORIGIN, 12, seed=5)
    readings = [{"x": p[0], "y": p[1], "theta": p[2], "range": synth.raycast(world, UNIT, ORIGIN, p, FOV, BEAMS, R)} for p in poses]
    return world, poses, readings


@pytest.fixture(scope="module")
def scene():
    """The structured map of case 1 -- twelve oracle updates along a seeded walk -- and the walk itself, computed once."""
    world, poses, readings = _walk()
    ref = so.GridOracle(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    for r in readings:
        ref.updateOccupancyGrid(r)
    assert not ref.growth_log
    return dict(world=world, poses=poses, readings=readings, ref=ref)


@pytest.fixture(scope="module")
def world_grid(pkg, scene):
    """The whole synthetic world as a well-mapped grid on the device, and its oracle twin (cases 3 and 4)."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    v, t = synth.counts_from_world(scene["world"])
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    og.set_counts(v, t)
    ref = so.GridOracle(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    ref.visited, ref.total = v, t
    return og, ref


def tie_headings(S, ks=(3, -4, 10, 27, -31, 58)):
    """Headings at which theta / (2 pi) * S sits exactly on k + 0.5 in floating point: rint's ties-to-even decides the spoke."""
    out = []
    for k in ks:
        th = (k + 0.5) * (2 * np.pi) / S
        for cand in (th, np.nextafter(th, np.inf), np.nextafter(th, -np.inf)):
            if cand / (2 * np.pi) * S == k + 0.5:
                out.append(float(cand))
                break
    return out


def case1_poses(walk, S):
    x0, y0, _ = walk[0]
    poses = [tuple(p) for p in walk]
    poses += [(p[0] + 0.037, p[1] - 0.012, p[2]) for p in walk]                      # off the lattice
    poses += [(walk[3][0] + 0.05, walk[3][1], walk[3][2])]                          # onto a half cell
    poses += [(x0, y0, th) for th in (np.pi, -np.pi, np.nextafter(np.pi, 0), np.nextafter(-np.pi, 0), np.pi - 1e-9, -np.pi + 1e-9)]
    poses += [(x0, y0, 7.0), (x0, y0, 2 * np.pi + 0.4), (x0, y0, -7.3), (x0, y0, -4 * np.pi - 0.2)]   # beyond +-2 pi
    ties = tie_headings(S)
    assert len(ties) >= 3
    poses += [(x0, y0, th) for th in ties]
    return np.array(poses, dtype=np.float64)


def test_case1_structured_map_many_poses_one_launch(pkg, scene):
    ref = scene["ref"]
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    og.set_counts(ref.visited, ref.total)
    poses = case1_poses(scene["poses"], ref.lut.num_spokes)
    assert 36 <= len(poses) <= 48
    got = og.predictScans(poses)
    want = yard.predict_many(ref, poses)
    assert want[2].sum() > 20 * len(poses)                    # (the map holds walls: most beams see one)
    _same(got, want, "structured map")
    one = og.predictScan({"x": poses[5][0], "y": poses[5][1], "theta": poses[5][2], "range": None})
    _same(one, tuple(w[5] for w in want), "predictScan of a reading")
    hit = want[2][5] > 0
    assert np.array_equal(one["range"][hit], (want[0][5][hit] + want[1][5][hit]) / 2) and (one["range"][~hit] == R).all()
    assert (og.predictScan(poses[5], no_return=-1.0)["range"][~hit] == -1.0).all()


def test_case2_one_map_per_pose(pkg):
    """map_stride 1: three maps of different shape and limits -- one grown on a low side, one promoted to 64-bit cells -- one pose each."""
    import torch
    eng_mod = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    dev = torch.device("cuda:0")
    lidar = eng_mod.LidarModel.get(UNIT, R, FOV, BEAMS, WALL)
    maps = [eng_mod.MapState.create(20, 20, {"x": 0.0, "y": 0.0}, UNIT, dev),
            eng_mod.MapState.create(12, 12, {"x": 1.33, "y": -0.4}, UNIT, dev),
            eng_mod.MapState.create(16, 16, {"x": -2.0, "y": 0.5}, UNIT, dev)]
    maps[1].ensure_contains(np.array([maps[1].lim_x[0] - 0.3]), np.array([0.0]), UNIT)        # grows on the low x side
    assert maps[1].growth_log and maps[1].growth_log[0][0] == 1
    rs = np.random.RandomState(2)
    for k, m in enumerate(maps):
        occ = rs.uniform(size=(m.rows, m.cols)) < 0.03
        v, t = np.where(occ, 7.0, 1.0), np.where(occ, 8.0, 5.0)
        if k == 2:                                                                    # counts beyond 16 bits: 64-bit cells
            v[occ], t[occ] = 70001.0, 80000.0
        m.upload(v, t)
    assert maps[2].wide and not maps[0].wide
    assert len({(m.rows, m.cols) for m in maps}) == 3
    eng = eng_mod.ParticleEngine(lidar, maps, dev)
    poses = np.array([[0.3, -0.7, 0.4], [1.0, 0.25, -2.0], [-2.51, 1.0, 3.0]])
    got = eng.predict_host(eng.predict_scan(eng.to_device(poses), 3))
    assert got["first"].shape == (3, BEAMS)
    for k, m in enumerate(maps):
        v, t = m.download()
        ref = yard.oracle_of(v, t, m.lim_x, m.lim_y, UNIT, FOV, BEAMS, R, WALL)
        want = yard.predict(ref, poses[k])
        assert want[2].sum() > 0
        _same({key: val[k] for key, val in got.items()}, want, f"map {k}")
    assert lib.PREDICT_STRIDE == 4


def _raw_predict(pkg, lidar_c, beams, eng, poses):
    """The C call itself with a given lidar descriptor: every pose in the engine's map 0."""
    import torch
    lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    eng.refresh_bits()
    d_pose = eng.to_device(poses)
    out = torch.empty((len(poses), beams, lib.PREDICT_STRIDE), dtype=torch.float64, device=eng.device)
    rc = lib.lib().slam2d_predict_scan(ctypes.byref(lidar_c), ctypes.c_void_p(eng.d_maps.data_ptr()), 0, len(poses),
                                       ctypes.c_void_p(d_pose.data_ptr()), 3, 0.0, float(lidar_c.max_range),
                                       ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return eng.predict_host(out)


SHAPE_POSES = np.array([[0.3, -0.7, 0.4], [-3.1, 2.2, -1.9], [4.44, 4.01, 2.5], [5.0, -5.0, 0.0]])


@pytest.mark.parametrize("beams,fov,max_range", [(3, FOV, R), (4, FOV, R), (5, FOV, R), (181, FOV, R), (60, 2 * np.pi, R),
                                                 (60, FOV, 3.97)])
def test_case3_launch_shapes(pkg, world_grid, beams, fov, max_range):
    """Beam counts round the four-beams-per-block edge, a lidar that uses every spoke, and one whose window step is not the map
    unit (range 3.97 m: the per-cell index path).  The lidars of 3 and 4 beams (and of one, below) have spokes so wide that a wall
    spreads over more chunks of cells than the kernel keeps in registers: some of their beams take its second walk."""
    _, ref0 = world_grid
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, fov, beams, max_range, WALL)
    og.set_counts(ref0.visited, ref0.total)
    if max_range != R:
        assert og.lidar.xs_step() != UNIT
    ref = yard.oracle_of(ref0.visited, ref0.total, ref0.mapXLim, ref0.mapYLim, UNIT, fov, beams, max_range, WALL)
    want = yard.predict_many(ref, SHAPE_POSES)
    assert want[2].sum() > 0
    _same(og.predictScans(SHAPE_POSES), want, f"{beams} beams, fov {fov}, range {max_range}")


def test_case3_one_beam(pkg, world_grid):
    """A lidar of ONE beam over pi: two spokes.  The Python model refuses fewer than two beams, so the descriptor is that of the
    two-beam lidar over 2 pi -- the same two spokes, hence the same tables -- with the one-beam lidar's beams, FOV and start spoke."""
    _, ref0 = world_grid
    two = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, 2 * np.pi, 2, R, WALL)
    two.set_counts(ref0.visited, ref0.total)
    ref = yard.oracle_of(ref0.visited, ref0.total, ref0.mapXLim, ref0.mapYLim, UNIT, FOV, 1, R, WALL)
    assert ref.lut.num_spokes == 2 == two.lidar.num_spokes and np.array_equal(ref.lut.bin, two.lidar.bin)
    eng = two.engine()
    lidar_c = type(eng.lidar_c).from_buffer_copy(eng.lidar_c)
    lidar_c.beams, lidar_c.fov, lidar_c.spoke_start = 1, FOV, ref.spokesStartIdx
    got = _raw_predict(pkg, lidar_c, 1, eng, SHAPE_POSES)
    want = yard.predict_many(ref, SHAPE_POSES)
    assert want[2].sum() > 0
    _same(got, want, "one beam")


def test_case4_edges_of_the_map_and_poses_that_see_nothing(pkg, world_grid):
    og, ref = world_grid
    poses = np.array([[9.0, 0.3, 0.2],                       # 1 m inside the border: part of the window is outside, those cells are free
                      [-9.0, -9.0, 2.4],
                      [0.3, 9.0, -1.2],
                      [110.0, 0.0, 0.0],                     # 100 m outside the map
                      [np.nan, 0.0, 0.0], [0.3, np.nan, 0.2], [0.3, -0.7, np.nan],
                      [np.inf, 0.0, 0.0], [0.3, -np.inf, 0.2], [0.3, -0.7, np.inf], [0.3, -0.7, -np.inf],
                      [1e13, 0.0, 0.0], [0.3, -0.7, 1e12],    # a quotient that is not below 1e9
                      [0.3, -0.7, 0.4]])
    got = og.predictScans(poses)
    want = yard.predict_many(ref, poses)
    _same(got, want, "edges")
    for k in (0, 1, 2, 13):
        assert got["cells"][k].sum() > 0, k
    for k in range(3, 13):
        assert not got["hit"][k].any() and np.isinf(got["first"][k]).all() and (got["far"][k] == -np.inf).all(), k
    alone = og.predictScans(poses[[0, 13]])                   # the poses next to the bad ones are what they are alone
    for key in ("first", "far", "cells"):
        assert np.array_equal(alone[key], got[key][[0, 13]])


def test_case4_range_windows(pkg, world_grid):
    og, ref = world_grid
    for r_min, r_max in ((1.0, 2.0), (0.0, 2.0), (1.0, None), (3.2, 3.7)):
        got = og.predictScans(SHAPE_POSES, r_min=r_min, r_max=r_max)
        want = yard.predict_many(ref, SHAPE_POSES, r_min, r_max)
        _same(got, want, f"window ({r_min}, {r_max})")
        assert (want[0][want[2] > 0] > r_min).all() and (want[1][want[2] > 0] < (R if r_max is None else r_max)).all()


def test_case4_a_cell_exactly_on_the_window_limit_is_not_a_hit(pkg):
    ref = so.GridOracle(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    pose, beam = (0.3, -0.7, 0.3), 23
    lut = ref.lut
    spoke = (ref.spokesStartIdx + int(np.rint(pose[2] / (2 * np.pi) * lut.num_spokes)) + beam) % lut.num_spokes
    c = lut.cells_of(spoke)
    k = c[np.argmin(np.abs(lut.r.ravel()[c] - 1.5))]
    r0 = lut.r.ravel()[k]
    mx, my = ref.convertRealXYToMapIdx(pose[0] + lut.xs[k % lut.width], pose[1] + lut.xs[k // lut.width])
    ref.visited[my, mx], ref.total[my, mx] = 7.0, 8.0          # the one occupied cell of the map
    og.set_counts(ref.visited, ref.total)
    for r_min, r_max, hit in ((r0, R, False), (np.nextafter(r0, 0), R, True), (0.0, r0, False), (0.0, np.nextafter(r0, 9), True)):
        got = og.predictScan(pose, r_min=r_min, r_max=r_max)
        _same(got, yard.predict(ref, pose, r_min, r_max), f"({r_min}, {r_max})")
        assert got["cells"].sum() == (1 if hit else 0)
        if hit:
            assert got["cells"][beam] == 1 and got["first"][beam] == r0 == got["far"][beam]


def test_case5_bits_through_the_real_update_paths(pkg, scene):
    """The occupancy bits as k_grid_update keeps them (six updateOccupancyGrid calls) and as a refresh rebuilds them (update_many)."""
    readings = scene["readings"][:6]
    poses = np.array([[r["x"], r["y"], r["theta"]] for r in readings] + [[r["x"] + 0.037, r["y"] - 0.012, r["theta"] + 0.5] for r in readings])
    a = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    for r in readings:
        a.updateOccupancyGrid(r)
    got_a = a.predictScans(poses)
    b = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    b.update_many(readings)
    got_b = b.predictScans(poses)
    for og, got, what in ((a, got_a, "updateOccupancyGrid"), (b, got_b, "update_many")):
        want = yard.predict_many(_oracle_of_grid(og), poses)
        assert want[2].sum() > 20 * len(poses)
        _same(got, want, what)
    res = a.scanResidual(readings[5])
    pred = a.predictScan(readings[5])
    rng = np.asarray(readings[5]["range"])
    valid = pred["hit"] & (rng < R)
    assert valid.any() and np.array_equal(res[valid], (rng - pred["range"])[valid]) and np.isnan(res[~valid]).all()


@pytest.mark.parametrize("theta", [0.0, 0.3, -2.9, 3.1, 7.0])
def test_case6_round_trip_on_the_device(pkg, theta):
    """tests/test_predict_host.py's property with the update and the prediction both on the GPU."""
    reading = {"x": 0.3, "y": -0.7, "theta": theta, "range": scan_ranges()}
    walls = yard.beam_walls(so.GridOracle(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL), reading)
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    og.updateOccupancyGrid(reading)
    got = og.predictScan(reading)
    assert check_round_trip(walls, got["first"], got["far"], got["cells"]) >= 20


def test_case7_filter_particles_in_their_own_maps(pkg, intel_readings):
    lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    u, P = 0.02, 3
    ogP = [30, 30, intel_readings[0], u, np.pi, 10, 180, 5 * u]
    pf = pkg.ParticleFilter(P, ogP, [1.4, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 5], rng=np.random.RandomState(4))
    with pytest.raises(lib.Slam2dError):
        pf.predict_scans()                                     # no scan yet: no matched poses
    for count, raw in enumerate(intel_readings[:3], start=1):
        pf.updateParticles(raw, count)
    got = pf.predict_scans()
    assert got["first"].shape == (P, 180)
    for p in range(P):
        m = pf.engine.maps[p]
        v, t = m.download()
        ref = yard.oracle_of(v, t, m.lim_x, m.lim_y, u, np.pi, 180, 10, 5 * u)
        want = yard.predict(ref, pf.prev_matched[p])
        assert want[2].sum() > 180
        _same({k: a[p] for k, a in got.items()}, want, f"particle {p}")
    again = pf.predict_scans()
    for k in ("first", "far", "cells", "range"):
        assert again[k].tobytes() == got[k].tobytes(), k
    given = pf.predict_scans(poses=pf.prev_matched)
    assert given["first"].tobytes() == got["first"].tobytes() and given["cells"].tobytes() == got["cells"].tobytes()
    seen = []

    def on_scan(count, f, unb):
        with pytest.raises(lib.Slam2dError):
            f.predict_scans()                                  # a pipelined scan may be in flight: it raises, it does not race
        seen.append(count)
    pf.run(intel_readings[3:6], first_count=4, on_scan=on_scan)
    assert seen == [4, 5, 6]
    after = pf.predict_scans()                                 # valid again once run() has returned
    m = pf.engine.maps[0]
    v, t = m.download()
    _same({k: a[0] for k, a in after.items()},
          yard.predict(yard.oracle_of(v, t, m.lim_x, m.lim_y, u, np.pi, 180, 10, 5 * u), pf.prev_matched[0]), "after run()")
