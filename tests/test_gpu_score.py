"""slam2d_score_poses on the MI355X against the definition in NumPy (tests/score_yardstick.py): every comparison is
np.array_equal on all eight slots.  The yardstick reads the DEVICE's field and frame (SearchLevel.field_cost, frames()) and the
device's cos / sin of the very beam angles (slam2d_device_sincos), and the result is an integer sum over a set of cells: there is
no tolerance.  Lidar and world of tests/test_score_host.py: unit 0.1 m, range 4 m, FOV pi, 60 beams; the covering level of a
window of half-edge 8 m: reach 14.4 m, a 289 x 289 field, 19 x 19 tiles."""
import ctypes
import importlib

import numpy as np
import pytest

import score_yardstick as yard
from test_score_host import BEAMS, COVER, FOV, INIT, R, SIZE, UNIT, WALL, lattice, walk

pytestmark = pytest.mark.gpu

SMP = (0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)                 # scan sigma 1 cell, fine miss probability 0.15 ** (2 / 1)
WINDOW = (0.0, 0.0, 8.0)
# every beam count at which the launch changes shape: the hash set doubles where 1.5 * beams passes a power of two (64 slots at
# least), and above 1365 beams (4096 slots) a block holds two poses instead of four
HASH_EDGES = [42, 43, 85, 86, 170, 171, 341, 342, 682, 683, 1365, 1366]


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


def device_sincos(eng, angles):
    import torch
    _lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    a = eng.to_device(np.ascontiguousarray(angles, dtype=np.float64).reshape(-1))
    c, s = torch.empty_like(a), torch.empty_like(a)
    _lib.check(eng.L.slam2d_device_sincos(a.data_ptr(), a.numel(), c.data_ptr(), s.data_ptr(), engine._stream()), "sincos")
    return c.cpu().numpy().reshape(np.shape(angles)), s.cpu().numpy().reshape(np.shape(angles))


@pytest.fixture(scope="module")
def scene(pkg):
    """The well-mapped world on the device, its matcher, and the covering level's field as one full build left it -- downloaded
    once and shared; the walk and its ray-cast scans."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world, poses, scans = walk()
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    og.set_counts(*synth.counts_from_world(world))
    sm = pkg.ScanMatcher(og, *SMP)
    first = sm.scorePoses(poses, scans[0], window=WINDOW)      # builds the field
    lv = sm.last_cover["level"]
    fr = lv.frames()[0]
    field = lv.field_cost(0).copy()
    assert lv.tmax == 19 and field.shape == (289, 289) and sm.last_cover["window"] == WINDOW
    assert (field > 0).any() and (field == 0).any()            # free space and walls
    return dict(og=og, sm=sm, lv=lv, eng=og.engine(), field=field, frame=(float(fr["xlo"]), float(fr["ylo"])), poses=poses,
                scans=scans, first=first)


def expect(scene, poses, ranges, device_trig=True, lv=None, field=None, frame=None):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    lv = lv or scene["lv"]
    cos = sin = None
    if device_trig:
        cos, sin = device_sincos(scene["eng"], np.array([yard.beam_angles(p[2], FOV, ranges.shape[-1]) for p in poses]))
    return yard.score_poses(scene["field"] if field is None else field, frame or scene["frame"], lv.c.cost_scale, lv.step, poses, ranges,
                            FOV, R, cos, sin)


def launch(scene, poses, ranges, beams=None, pose_stride=3, ranges_stride=None):
    """slam2d_score_poses on the scene's field: through ParticleEngine.score_poses, or -- another beam count than the grid's --
    at the C ABI with a copy of the lidar descriptor (the call reads only beams, fov and max_range of it)."""
    import torch
    _lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng, lv = scene["eng"], scene["lv"]
    poses = np.asarray(poses, dtype=np.float64)
    ranges = np.asarray(ranges, dtype=np.float64)
    N = len(poses)
    if ranges_stride is None:
        ranges_stride = 0 if ranges.ndim == 1 else ranges.shape[1]
    d_pose, d_rng = eng.to_device(poses), eng.to_device(ranges)
    if beams is None:
        return eng.score_poses(lv, 0, d_pose, pose_stride, N, d_rng, ranges_stride)
    lid = _lib.Slam2dLidar.from_buffer_copy(eng.lidar_c)
    lid.beams = beams
    out = torch.empty((N, _lib.SCORE_STRIDE), dtype=torch.float64, device=eng.device)
    _lib.check(eng.L.slam2d_score_poses(ctypes.byref(lid), ctypes.byref(lv.c), 0, N, d_pose.data_ptr(), pose_stride, d_rng.data_ptr(),
                                        ranges_stride, out.data_ptr(), engine._stream()), "slam2d_score_poses")
    return out


def same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:6].tolist(), got[got != want][:6], want[got != want][:6])


def case1_poses(scene):
    walk_, (xlo, ylo) = scene["poses"], scene["frame"]
    x0, y0, th0 = walk_[0]
    poses = [tuple(p) for p in walk_]
    poses += [(p[0] + 0.037, p[1] - 0.012, p[2] + 0.01) for p in walk_]                  # off the lattice
    # headings +-pi and their neighbours, off the lattice (on it the first beam, straight along an axis, ends ON a cell border: below)
    poses += [(x0 + 0.037, y0 - 0.012, th) for th in (np.pi, -np.pi, np.nextafter(np.pi, 0), np.nextafter(-np.pi, 0), np.pi - 1e-9, -np.pi + 1e-9)]
    poses += [(p[0] - 0.05, p[1] + 0.05, p[2] - 0.5) for p in walk_[:5]]                   # on half cells, turned
    poses += [(x0, y0, 7.0), (x0, y0, 2 * np.pi + 0.4), (x0, y0, -7.3), (x0, y0, -4 * np.pi - 0.2), (x0, y0, 300.0)]      # beyond +-2 pi
    # the pose itself on a border between cells of the field, on one axis and on both, and in the middle of a cell
    poses += [(xlo + 131 * UNIT, y0, 0.3), (x0, ylo + 152 * UNIT, -1.1), (xlo + 140 * UNIT, ylo + 160 * UNIT, 2.0),
              (xlo + 144.5 * UNIT, ylo + 139.5 * UNIT, -2.6), (xlo + UNIT * 150, ylo + UNIT * 150, 0.7)]
    return np.array(poses, dtype=np.float64)


def test_case1_one_scan_hand_picked_poses(scene):
    poses, rng = case1_poses(scene), scene["scans"][0]
    assert 40 <= len(poses) <= 48
    rows = launch(scene, poses, rng)
    want = expect(scene, poses, rng)
    assert (want[:, 3] > 20).all() and want[:, 5].max() > 0
    same(rows, want, "case 1")
    # scorePoses and the engine call agree (the fixture's call scored the walk)
    got = scene["sm"].scorePoses(poses, {"x": 0, "y": 0, "theta": 0, "range": rng}, window=WINDOW)
    dec = scene["eng"].score_host(rows)
    assert set(got) == {"score", "cells", "beam_score", "inside", "in_range", "outside"}
    for k in got:
        assert np.array_equal(got[k], dec[k]), k
    assert np.array_equal(got["score"], want[:, 0]) and np.array_equal(got["outside"], (want[:, 4] - want[:, 3]).astype(np.int64))
    for k in got:
        assert np.array_equal(scene["first"][k], got[k][:12]), k
    # NumPy's own cos / sin: equal wherever no quotient sits next to an integer -- asserted first, on the host
    assert yard.min_distance_to_integer(scene["frame"], UNIT, poses, rng, FOV, R) > 1e-9
    same(rows, expect(scene, poses, rng, device_trig=False), "case 1, NumPy's cos / sin")


def test_endpoints_on_cell_borders(scene):
    """Lattice poses with headings along the axes and ranges in whole cells: the outer beams end ON borders between cells (the
    quotient is an integer give or take an ulp), where only the exact operations of the definition -- the division included --
    give the yardstick's cell."""
    x0, y0, _ = scene["poses"][0]
    poses = np.array([(x0, y0, th) for th in (np.pi, -np.pi, 0.0, np.pi / 2, -np.pi / 2, 2 * np.pi, -3 * np.pi)] +
                     [(x0 + 0.3, y0 - 1.1, th) for th in (np.pi, 0.0, np.pi / 2)])
    rng = np.tile([1.0, 2.0, 0.5, 3.0, 0.1, 2.5], BEAMS // 6)
    assert yard.min_distance_to_integer(scene["frame"], UNIT, poses, rng, FOV, R) < 1e-9
    want = expect(scene, poses, rng)
    assert (want[:, 3] == BEAMS).all()
    same(launch(scene, poses, rng), want, "endpoints on cell borders")


def test_case2_a_scan_per_pose(scene):
    walk_, scans = scene["poses"], scene["scans"]
    poses = np.array([tuple(p) for p in walk_] + [(p[0] + 0.21, p[1] - 0.33, p[2] + 0.05) for p in walk_] +
                     [(p[0], p[1], p[2] + np.pi / 3) for p in walk_])
    rng = np.vstack([scans, scans, scans])
    assert poses.shape == (36, 3) and rng.shape == (36, BEAMS)
    want = expect(scene, poses, rng)
    same(launch(scene, poses, rng), want, "case 2")
    assert (want[:12, 0] > want[24:, 0]).all()                 # (a scan fits its own pose better than the pose turned by 60 degrees)
    # strides beyond the minimum: poses in rows of five doubles, scans in rows of beams + 3
    wide_p = np.full((36, 5), np.nan)
    wide_p[:, :3] = poses
    wide_r = np.full((36, BEAMS + 3), 0.5)
    wide_r[:, :BEAMS] = rng
    same(launch(scene, wide_p, wide_r, pose_stride=5, ranges_stride=BEAMS + 3), want, "case 2, wide strides")


def test_case3_range_edges(scene):
    pose, base = scene["poses"][0], scene["scans"][0]
    planted = base.copy()
    for b, v in {3: np.nan, 9: np.inf, 14: R, 20: np.nextafter(R, np.inf), 26: 0.0, 31: -0.7, 40: np.nextafter(R, 0), 44: -np.inf,
                 50: -0.0, 55: 1e-300, 57: -3.9}.items():
        planted[b] = v
    rng = np.vstack([planted, np.full(BEAMS, 1.5 * R), np.full(BEAMS, np.nan), np.full(BEAMS, np.inf), np.full(BEAMS, R),
                     np.zeros(BEAMS), np.full(BEAMS, -0.5), np.full(BEAMS, np.nextafter(R, 0)), base])
    poses = np.tile(pose, (len(rng), 1))
    want = expect(scene, poses, rng)
    assert not want[1:5].any()                                 # out of range, NaN, inf, == max_range: nothing in range, every slot zero
    assert (want[5:8, 4] == BEAMS).all() and (want[5:8, 3] == BEAMS).all()
    assert want[0, 3] == want[0, 4] - 1                        # (-inf is in range and fails the guard)
    same(launch(scene, poses, rng), want, "case 3")
    same(launch(scene, poses[1:2], rng[1]), want[1:2], "case 3, one all-out-of-range scan for all poses")


def test_case4_borders_and_poses_that_see_nothing(scene):
    (xlo, ylo), walk_ = scene["frame"], scene["poses"]
    edge = [(xlo + 1.0, 0.0, np.pi), (xlo + 28.0, 0.0, 0.0), (0.0, ylo + 0.5, -np.pi / 2), (0.0, ylo + 28.3, np.pi / 2),
            (xlo + 0.04, ylo + 0.04, 0.8), (xlo + 28.85, ylo + 28.85, -2.4), (xlo - 0.05, ylo - 0.05, 0.7), (xlo - 2.0, 0.0, 0.0)]
    blind = [(40.0, 40.0, 0.3), (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, np.nan), (0.0, 0.0, -np.inf), (-np.inf, np.nan, np.inf),
             (1e12, 0.0, 0.0), (0.0, -1e12, 1.0), (1e300, 1e300, 0.0), (-1e9 * UNIT, 0.0, 0.0), (0.0, 0.0, 1e12), (3e9, -3e9, 0.0)]
    good = [tuple(p) for p in walk_]
    poses = []
    for i in range(12):                                        # a good pose between any two others
        poses += [edge[i % len(edge)], good[i], blind[i]]
    poses = np.array(poses)
    rng = np.full(BEAMS, 3.0)
    rng[::7] = 0.6
    want = expect(scene, poses, rng)
    w = want.reshape(12, 3, -1)
    assert (w[:7, 0, 4] - w[:7, 0, 3] > 0).all() and (w[:7, 0, 3] > 0).all()      # at the border: beams inside and outside
    assert w[7, 0, 3] > 0                                                          # from outside, looking in
    assert not w[:10, 2][:, [0, 1, 2, 3, 5, 6, 7]].any() and (w[:, 2, 4] == BEAMS).all()      # blind poses: zeros, beams still in range
    got = launch(scene, poses, rng)
    same(got, want, "case 4")
    # the neighbours' rows are what a launch of the good poses alone gives
    same(launch(scene, np.array(good), rng), got.cpu().numpy().reshape(12, 3, -1)[:, 1], "case 4, neighbours")


def test_case5_a_scan_folded_into_one_or_two_cells(scene):
    (xlo, ylo), field = scene["frame"], scene["field"]
    free = np.argwhere(field[100:200, 100:200] == field.max()) + 100
    wall = np.argwhere(field[100:200, 100:200] == 0) + 100
    assert len(free) > 10 and len(wall) > 10
    cells = [tuple(free[0]), tuple(free[len(free) // 2]), tuple(wall[0]), tuple(wall[-1]), tuple(free[-1])]
    centre = np.array([(xlo + (cx + 0.5) * UNIT, ylo + (cy + 0.5) * UNIT, 0.4 * i) for i, (cy, cx) in enumerate(cells)])
    border = np.array([(xlo + cx * UNIT, ylo + (cy + 0.5) * UNIT, np.pi / 2) for cy, cx in cells])     # on the border of two columns, looking along it
    poses = np.vstack([centre, border])
    for rng in (np.full(BEAMS, 0.03), np.zeros(BEAMS)):
        want = expect(scene, poses, rng)
        assert (want[:5, 1] == 1).all() and (want[:, 3] == BEAMS).all() and (want[:, 1] <= 2).all()
        for row, (cy, cx) in zip(want[:5], cells):
            assert row[5] == float(field[cy, cx]) and row[6] == BEAMS * float(field[cy, cx])      # sum_b = inside x cost
        same(launch(scene, poses, rng), want, "case 5")
    assert (expect(scene, border, np.full(BEAMS, 0.03))[:, 1] == 2).any()


@pytest.mark.parametrize("beams", sorted({1, 2, 63, 64, 65, 257, 1081, 2048, *HASH_EDGES}))
def test_case6_beam_counts(scene, beams):
    rs = np.random.RandomState(beams)
    walk_ = scene["poses"]
    poses = np.array([tuple(p) for p in walk_] + [(p[0] + rs.uniform(-0.5, 0.5), p[1] + rs.uniform(-0.5, 0.5), rs.uniform(-4, 4)) for p in walk_[:8]])
    assert len(poses) == 20
    one = rs.uniform(0.2, 1.1 * R, beams)
    want = expect(scene, poses, one)
    if beams > 2:
        assert 0 < want[0, 4] < beams
    if beams >= 1081:
        assert (want[:, 1] < want[:, 3]).all()                 # neighbouring beams share cells
    same(launch(scene, poses, one, beams=beams), want, f"{beams} beams, one scan")
    each = rs.uniform(0.2, 1.1 * R, (20, beams))
    same(launch(scene, poses, each, beams=beams), expect(scene, poses, each), f"{beams} beams, a scan per pose")


def test_case7_the_lattice_in_one_launch(scene):
    poses = np.vstack([lattice(), scene["poses"][5]])
    assert len(poses) == 17 * 17 * 24 + 1
    rng = scene["scans"][5]
    want = expect(scene, poses, rng)
    got = scene["sm"].scorePoses(poses, rng, window=WINDOW)
    same(np.column_stack([got["score"], got["cells"], got["beam_score"], got["inside"], got["in_range"]]), want[:, :5], "case 7")
    same(launch(scene, poses, rng), want, "case 7, rows")
    assert int(np.argmax(got["beam_score"])) == len(poses) - 1                      # (the true pose of the scan)
    # the bounding box of the poses frames the same field as the window
    box = scene["sm"].scorePoses(poses, rng)
    assert scene["sm"].last_cover["window"] == WINDOW
    for k in got:
        assert np.array_equal(got[k], box[k]), k


def test_case8_same_bytes_and_permutation(scene):
    poses = np.vstack([lattice(8), case1_poses(scene), [(np.nan, 0.0, 0.0)]])
    rng = scene["scans"][3]
    a = launch(scene, poses, rng).cpu().numpy()
    b = launch(scene, poses, rng).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    perm = np.random.RandomState(8).permutation(len(poses))
    c = launch(scene, poses[perm], rng).cpu().numpy()
    assert c.tobytes() == a[perm].tobytes()
    each = np.tile(rng, (len(poses), 1))
    assert launch(scene, poses, each).cpu().numpy().tobytes() == a.tobytes()      # a scan per pose, the same scan


def test_the_coarse_level_and_a_frame_of_its_own(pkg, scene):
    """scorePoses at the matcher's coarse configuration, framed on the poses' bounding box: its own level, field and frame."""
    sm = pkg.ScanMatcher(scene["og"], 0.7, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 5)
    poses, rng = scene["poses"], scene["scans"]
    got = sm.scorePoses(poses, rng, level="coarse")
    lv = sm.last_cover["level"]
    assert lv is not scene["lv"] and lv.step == 5 * UNIT
    cx, cy, half = sm.last_cover["window"]
    assert lv.reach >= half + R
    fr = lv.frames()[0]
    want = expect(scene, poses, rng, lv=lv, field=lv.field_cost(0), frame=(float(fr["xlo"]), float(fr["ylo"])))
    assert np.array_equal(got["score"], want[:, 0]) and np.array_equal(got["cells"], want[:, 1].astype(np.int64))
    assert np.array_equal(got["beam_score"], want[:, 2]) and np.array_equal(got["inside"], want[:, 3].astype(np.int64))
    with pytest.raises(ValueError, match="window"):
        sm.scorePoses(poses, rng, level="fine", window=(0.0, 0.0, 500.0))
    with pytest.raises(ValueError):
        sm.scorePoses(poses, rng[:5])
