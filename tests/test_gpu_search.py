"""slam2d_search_lattice on the MI355X against the definition in NumPy (tests/lattice_yardstick.py, built on
tests/score_yardstick.py): every comparison is np.array_equal on the 64-bit words.  The yardstick reads the DEVICE's field and
frame and the device's cos / sin of the lattice's beam angles (slam2d_device_sincos); the result is a minimum of integer sums:
there is no tolerance.  World, lidar and the 289 x 289 field of tests/test_gpu_score.py."""
import ctypes
import importlib

import numpy as np
import pytest

import lattice_yardstick as lyard
import score_yardstick as yard
from test_score_host import BEAMS, FOV, INIT, R, SIZE, UNIT, WALL, walk

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

SMP = (0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)                 # as tests/test_gpu_score.py
WINDOW = (0.0, 0.0, 8.0)
SEARCH_CHUNK = _lib.SEARCH_CHUNK                               # headings per block row of the search launch, where positions are few
SEARCH_WAVES = _lib.SEARCH_WAVES                               # waves of 64 positions from which on a launch has one block row
assert (SEARCH_CHUNK, SEARCH_WAVES) == (8, 4096)


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


def device_sincos(eng, angles):
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    a = eng.to_device(np.ascontiguousarray(angles, dtype=np.float64).reshape(-1))
    c, s = torch.empty_like(a), torch.empty_like(a)
    _lib.check(eng.L.slam2d_device_sincos(a.data_ptr(), a.numel(), c.data_ptr(), s.data_ptr(), engine._stream()), "sincos")
    return c.cpu().numpy().reshape(np.shape(angles)), s.cpu().numpy().reshape(np.shape(angles))


@pytest.fixture(scope="module")
def scene(pkg):
    """The well-mapped world on the device, its matcher, and the covering level's field as one full build left it -- downloaded
    once and shared; the walk and its ray-cast scans."""
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world, poses, scans = walk()
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    og.set_counts(*synth.counts_from_world(world))
    sm = pkg.ScanMatcher(og, *SMP)
    sm.scorePoses(poses, scans[0], window=WINDOW)              # builds the field
    lv = sm.last_cover["level"]
    fr = lv.frames()[0]
    field = lv.field_cost(0).copy()
    assert field.shape == (289, 289) and (field > 0).any() and (field == 0).any()
    free = int(engine.encode_cost(lv.floor_value, lv.cost_scale))      # the default outside cost: free space as the field encodes it
    return dict(og=og, sm=sm, lv=lv, eng=og.engine(), field=field, frame=(float(fr["xlo"]), float(fr["ylo"])), poses=poses,
                scans=scans, free=free)


def parts(scene, lat, ranges, outside):
    """The yardstick's (cost, inside, in_range) [nth, ny, nx] with the device's cos / sin."""
    ranges = np.asarray(ranges, dtype=np.float64)
    cos, sin = device_sincos(scene["eng"], lyard.beam_angles(lat, FOV, len(ranges)))
    return lyard.costs(scene["field"], scene["frame"], scene["lv"].c.cost_scale, scene["lv"].step, lat, ranges, FOV, R, outside, cos, sin)


def expect(scene, lat, ranges, outside):
    return lyard.pack(parts(scene, lat, ranges, outside)[0])


def launch(scene, lat, ranges, outside, beams=None, poison=False):
    """slam2d_search_lattice on the scene's field: through ParticleEngine.search_lattice, or at the C ABI with buffers of its
    own -- for another beam count than the grid's (a copy of the lidar descriptor: the call reads only beams, fov and max_range
    of it) or to hand it poisoned buffers.  The image as uint64 [ny, nx] on the host."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng, lv = scene["eng"], scene["lv"]
    d_rng = eng.to_device(np.asarray(ranges, dtype=np.float64))
    if beams is None and not poison:
        return eng.search_lattice(lv, 0, lat, d_rng, outside).cpu().numpy().view(np.uint64)
    lid = _lib.Slam2dLidar.from_buffer_copy(eng.lidar_c)
    lid.beams = len(ranges) if beams is None else beams
    nx, ny, nth = lat[:3]
    n = eng.L.slam2d_search_lattice_work(ctypes.byref(lid), nx, ny, nth)
    assert n == 2 * nth * lid.beams
    work = torch.full((n,), -1, dtype=torch.int64, device=eng.device)         # (0xff bytes: NaNs as doubles)
    out = torch.full((ny, nx), -1, dtype=torch.int64, device=eng.device)
    _lib.check(eng.L.slam2d_search_lattice(ctypes.byref(lid), ctypes.byref(lv.c), 0, nx, ny, nth, *[float(v) for v in lat[3:]],
                                           d_rng.data_ptr(), outside, work.data_ptr(), out.data_ptr(), engine._stream()),
               "slam2d_search_lattice")
    return out.cpu().numpy().view(np.uint64)


def same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, what
    bad = got != want
    assert np.array_equal(got, want), (what, np.argwhere(bad)[:6].tolist(), [hex(v) for v in got[bad][:6]], [hex(v) for v in want[bad][:6]])


def headings(words):
    return (words & np.uint64(0xffff)).astype(np.int64)


def around(scene, k, nx, ny, nth, dx=UNIT, dy=UNIT, th0=None, dth=0.37):
    """A lattice about pose k of the walk, off the cells: its position near the middle, headings from th0 (default: the pose's,
    a few steps back)."""
    x, y, th = scene["poses"][k]
    return (nx, ny, nth, x - (nx // 2) * dx + 0.037, dx, y - (ny // 2) * dy - 0.012, dy, th - (nth // 2) * dth if th0 is None else th0, dth)


@pytest.fixture(scope="module")
def main_case(scene):
    lat = around(scene, 0, 65, 5, 7)
    rng = scene["scans"][0]
    want = expect(scene, lat, rng, scene["free"])
    return lat, rng, want


def test_main_case(scene, main_case):
    lat, rng, want = main_case
    # on the yardstick first: at least three different winning headings, and not all of them heading 0
    assert len(np.unique(headings(want))) >= 3 and (headings(want) != 0).any()
    assert yard.min_distance_to_integer(scene["frame"], UNIT, [(lat[3], lat[5], 0.0)], np.zeros(1), FOV, R) > 1e-3     # off-cell x0, y0
    same(launch(scene, lat, rng, scene["free"]), want, "main case")


@pytest.mark.parametrize("ny", [1, 3])
@pytest.mark.parametrize("nx", [1, 63, 64, 65, 130])
def test_launch_shapes(scene, nx, ny):
    for nth in (1, 2):
        lat = around(scene, 3, nx, ny, nth, dx=0.07, dy=0.23, dth=2.9)
        same(launch(scene, lat, scene["scans"][3], scene["free"]), expect(scene, lat, scene["scans"][3], scene["free"]), f"{nx} x {ny} x {nth}")


@pytest.mark.parametrize("nth", [SEARCH_CHUNK - 1, SEARCH_CHUNK, SEARCH_CHUNK + 1, 2 * SEARCH_CHUNK + 1])
def test_heading_chunks(scene, nth):
    """Few positions: the search launch has a block row per SEARCH_CHUNK headings -- one, one, two and three rows."""
    dth = 2 * np.pi / nth
    lat = around(scene, 7, 5, 3, nth, dx=0.3, dy=0.4, th0=scene["poses"][7][2] - (nth - 1) * dth, dth=dth)      # the pose's own heading last
    want = expect(scene, lat, scene["scans"][7], scene["free"])
    if nth > SEARCH_CHUNK:
        assert (headings(want) >= SEARCH_CHUNK).any() and (headings(want) < SEARCH_CHUNK).any()      # winners in more than one row
    same(launch(scene, lat, scene["scans"][7], scene["free"]), want, f"{nth} headings")


@pytest.mark.parametrize("beams", [1, 2, 63, 64, 65, 130])
def test_beam_counts(scene, beams):
    rs = np.random.RandomState(beams)
    rng = rs.uniform(0.2, 1.1 * R, beams)
    lat = around(scene, 2, 9, 2, 3, dx=0.21, dy=0.5, dth=1.9)
    cost, inside, in_range = parts(scene, lat, rng, scene["free"])
    if beams > 2:
        assert 0 < in_range.max() < beams
    same(launch(scene, lat, rng, scene["free"], beams=beams), lyard.pack(cost), f"{beams} beams")


def test_ties_take_the_lowest_heading(scene):
    lat = around(scene, 4, 70, 2, 5, th0=0.8, dth=0.0)
    want = expect(scene, lat, scene["scans"][4], scene["free"])
    assert (headings(want) == 0).all() and (want >> np.uint64(16)).max() > 0
    same(launch(scene, lat, scene["scans"][4], scene["free"]), want, "dth = 0")


def test_endpoints_on_cell_borders(scene):
    """Positions on the corners of field cells, headings along the axes, ranges in whole cells: the quotients sit on integers
    give or take an ulp, where only the definition's own operations -- the division included -- give the yardstick's cell."""
    xlo, ylo = scene["frame"]
    lat = (66, 2, 5, xlo + 110 * UNIT, UNIT, ylo + 150 * UNIT, UNIT, -np.pi, np.pi / 2)
    rng = np.tile([1.0, 2.0, 0.5, 3.0, 0.1, 2.5], BEAMS // 6)
    assert yard.min_distance_to_integer(scene["frame"], UNIT, lyard.poses(lat).reshape(-1, 3), rng, FOV, R) < 1e-9
    cost, inside, in_range = parts(scene, lat, rng, scene["free"])
    assert (inside == BEAMS).all()
    same(launch(scene, lat, rng, scene["free"]), lyard.pack(cost), "cell borders")


def test_a_lattice_across_the_edge_of_the_field(scene):
    xlo, ylo = scene["frame"]
    lat = (40, 3, 6, xlo - 1.03, 0.1, ylo + 9.02, 4.1, -np.pi, np.pi / 3)
    rng = scene["scans"][6]
    want = {}
    for outside in (0, scene["free"], 2 ** 32 - 1):
        cost, inside, in_range = parts(scene, lat, rng, outside)
        want[outside] = lyard.pack(cost)
    assert (inside < in_range).any() and (inside == in_range).any() and (inside == 0).any()
    assert (headings(want[0]) != headings(want[scene["free"]])).any()              # the penalty changes the winning heading
    assert int(want[2 ** 32 - 1].max() >> np.uint64(16)) > 2 ** 37             # (sums beyond 32 bits)
    for outside in want:
        same(launch(scene, lat, rng, outside), want[outside], f"outside_cost {outside}")


def test_degenerate_scans(scene):
    lat = around(scene, 1, 67, 2, 3)
    none = np.full(BEAMS, R)
    assert not expect(scene, lat, none, scene["free"]).any()
    got = launch(scene, lat, none, scene["free"])
    assert got.shape == (2, 67) and not got.any()              # nothing in range: every word 0
    for n in (3, 7):                                           # (fewer beams in range than one trip of the unrolled loop; one trip and three)
        few = none.copy()
        few[5:5 + 2 * n:2] = scene["scans"][1][5:5 + 2 * n:2].clip(0.3, 3.5)
        cost, inside, in_range = parts(scene, lat, few, scene["free"])
        assert (in_range == n).all() and (inside == n).all()
        same(launch(scene, lat, few, scene["free"]), lyard.pack(cost), f"{n} beams in range")
    rng = scene["scans"][1].copy()
    for b, v in {3: np.nan, 9: np.inf, 14: R, 20: np.nextafter(R, np.inf), 26: 0.0, 31: -0.7, 40: np.nextafter(R, 0), 44: -np.inf,
                 50: -0.0, 55: 1e-300, 57: -3.9}.items():
        rng[b] = v
    cost, inside, in_range = parts(scene, lat, rng, scene["free"])
    assert (inside < in_range).all()                           # (-inf is in range and ends nowhere: it pays outside_cost)
    same(launch(scene, lat, rng, scene["free"]), lyard.pack(cost), "planted ranges")


@pytest.mark.parametrize("which, value", [(3, np.nan), (5, np.inf), (7, np.nan), (3, -np.inf), (7, np.inf)])
def test_degenerate_lattices(scene, which, value):
    lat = list(around(scene, 1, 67, 2, 3))
    lat[which] = value
    rng = scene["scans"][1]
    in_range = int((rng < R).sum())
    want = expect(scene, tuple(lat), rng, 1000)
    assert (want == np.uint64((in_range * 1000) << 16)).all()  # no inside beam at any heading: heading 0
    same(launch(scene, tuple(lat), rng, 1000), want, f"lattice number {which} = {value}")


def score_poses_image(scene, lat, rng, outside):
    """The image from slam2d_score_poses' rows of the materialised lattice (slots 6, 3 and 4), formed on the device."""
    import torch
    eng = scene["eng"]
    nx, ny, nth = lat[:3]
    d_pose = eng.to_device(lyard.poses(lat).reshape(-1, 3))
    rows = eng.score_poses(scene["lv"], 0, d_pose, 3, nth * ny * nx, eng.to_device(rng), 0)
    cost = rows[:, 6].to(torch.int64) + (rows[:, 4] - rows[:, 3]).to(torch.int64) * outside
    it = torch.arange(nth, dtype=torch.int64, device=eng.device).reshape(-1, 1, 1)
    return ((cost.reshape(nth, ny, nx) << 16) | it).min(dim=0).values.cpu().numpy().view(np.uint64)


def test_agreement_with_score_poses_on_the_device(scene, main_case):
    lat, rng, want = main_case
    same(score_poses_image(scene, lat, rng, scene["free"]), want, "slam2d_score_poses on the main case's poses")


@pytest.mark.parametrize("nx, ny, nth", [(513, 256, 2 * SEARCH_CHUNK + 2), (1024, 257, SEARCH_CHUNK + 1)])
def test_windows_that_fill_the_card(scene, nx, ny, nth):
    """Half of SEARCH_WAVES waves of positions and more: two block rows of nine headings; all of them: one row of all headings.
    Too many poses for the NumPy yardstick: against slam2d_score_poses on the same poses, which the main case ties to it."""
    waves = -(-nx * ny // 64)
    rows = -(-SEARCH_WAVES // waves)
    assert (rows, -(-nth // rows)) == ((2, SEARCH_CHUNK + 1) if nx == 513 else (1, nth))
    lat = (nx, ny, nth, -7.93, 0.031 * 513 / nx, -7.71, 0.06, -np.pi, 2 * np.pi / nth)
    rng = scene["scans"][8]
    want = score_poses_image(scene, lat, rng, scene["free"])
    if rows == 2:
        assert (headings(want) > SEARCH_CHUNK).any() and (headings(want) <= SEARCH_CHUNK).any()      # winners in both rows
    assert len(np.unique(headings(want))) > 2
    same(launch(scene, lat, rng, scene["free"]), want, f"{nx} x {ny} x {nth}")


def test_same_bits_with_poisoned_buffers(scene, main_case):
    lat, rng, want = main_case
    a = launch(scene, lat, rng, scene["free"], poison=True)
    b = launch(scene, lat, rng, scene["free"], poison=True)
    assert a.tobytes() == b.tobytes()
    same(a, want, "poisoned d_work and d_out")


def test_on_another_stream_behind_a_field_build(scene, main_case):
    import torch
    lat, rng, want = main_case
    eng, lv = scene["eng"], scene["lv"]
    d_centre, d_rng = eng.to_device([[WINDOW[0], WINDOW[1]]]), eng.to_device(rng)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng.field_build(lv, d_centre, 2)
        words = eng.search_lattice(lv, 0, lat, d_rng, scene["free"])
        side.synchronize()
        got = words.cpu().numpy().view(np.uint64)
    torch.cuda.synchronize()
    assert not int(eng.take_flags()[0])
    same(got, want, "side stream")


def test_search_poses(pkg, scene):
    """ScanMatcher.searchPoses is the engine call decoded, and its first peak is the lattice pose nearest the pose the scan was
    taken at."""
    k = 4
    x, y, th = scene["poses"][k]
    rng = scene["scans"][k]
    sm = scene["sm"]
    window = (round(float(x), 1), round(float(y), 1), 0.2)
    res = sm.searchPoses({"x": 0, "y": 0, "theta": 0, "range": rng}, window, headings=72, top=3, separation=0.1)
    lv, lat = sm.last_cover["level"], sm.last_cover["lattice"]
    assert lv is not scene["lv"] and lat[:3] == (5, 5, 72) and sm.last_cover["window"] == window
    assert set(res) == {"cost", "heading", "score", "xs", "ys", "thetas", "peaks"}
    # the engine call, decoded
    eng = scene["og"].engine()
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    free = int(engine.encode_cost(lv.floor_value, lv.cost_scale))
    dec = eng.search_host(eng.search_lattice(lv, 0, lat, eng.to_device(rng), free), lat, lv.c.cost_scale)
    for key in dec:
        assert np.array_equal(res[key], dec[key]), key
    # the yardstick on this level's own field
    fr = lv.frames()[0]
    cos, sin = device_sincos(eng, lyard.beam_angles(lat, FOV, BEAMS))
    cost = lyard.costs(lv.field_cost(0), (float(fr["xlo"]), float(fr["ylo"])), lv.c.cost_scale, lv.step, lat, rng, FOV, R, free, cos, sin)[0]
    want = lyard.pack(cost)
    assert np.array_equal((res["cost"] << np.uint64(16)) | res["heading"].astype(np.uint64), want)
    # on the yardstick first: its arg-min is the lattice pose nearest the true pose
    it, iy, ix = np.unravel_index(int(np.argmin(cost)), cost.shape)
    assert (cost == cost.min()).sum() == 1
    turn = np.abs((res["thetas"] - th + np.pi) % (2 * np.pi) - np.pi)
    assert (ix, iy, it) == (int(np.argmin(np.abs(res["xs"] - x))), int(np.argmin(np.abs(res["ys"] - y))), int(np.argmin(turn)))
    p = res["peaks"][0]
    assert (p.x, p.y, p.theta, p.cost) == (res["xs"][ix], res["ys"][iy], res["thetas"][it], int(cost.min()))
    assert p.score == res["score"][iy, ix] == -(float(cost.min()) * (1.0 / lv.c.cost_scale))
    assert len(res["peaks"]) == 3 and all(max(abs(q.x - p.x), abs(q.y - p.y)) > 0.15 for q in res["peaks"][1:])
    assert [q.cost for q in res["peaks"]] == sorted(q.cost for q in res["peaks"])
    with pytest.raises(ValueError):
        sm.searchPoses(rng[:5], window)
