"""slam2d_mcl_step on the MI355X against the definition in NumPy (tests/mcl_yardstick.py, built on tests/score_yardstick.py): every
comparison is np.array_equal on bits -- the resampled poses, the ancestors and all sixteen report words.  The yardstick reads the
DEVICE's field and frame and the device's cos / sin (slam2d_device_sincos) of the particles' headings and of the beam angles of
the moved poses; everything else in the definition is an integer operation or one rounded operation: there is no tolerance.
World and 289 x 289 field of tests/test_gpu_search.py, at 180 beams."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import mcl_yardstick as mcl
from test_score_host import FOV, INIT, ORIGIN, R, SIZE, UNIT, WALL

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

BEAMS = 180
SMP = (0.7, 0.25, 1, 0.1, 0.25, 0.3, 0.15, 1)                 # as tests/test_gpu_search.py
WINDOW = (0.0, 0.0, 8.0)
K = _lib.MCL_SCAN_BLOCK                                        # particles one block of the scan launch covers
assert K == 1024
TEMPERATURE = 64.0                                             # of the weight table of most cases: several survivors at the spreads below
AMP = (0.02, 0.015, 0.01)
MOTIONS = [(0.11, -0.02, 0.05), (0.0, 0.0, 0.0), (-0.07, 0.04, -0.3), (0.25, 0.0, 0.012), (0.03, 0.09, 1.1)]


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
    """The well-mapped world on the device, a matcher on it, a covering level of the test's own with its field built in full --
    downloaded once and shared --, the walk and its scans ray-cast at 180 beams, the weight table."""
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world = synth.make_world(SIZE, UNIT, seed=3, n_boxes=25)
    poses = np.array(synth.random_walk(world, UNIT, ORIGIN, 12, seed=5))
    scans = np.array([synth.raycast(world, UNIT, ORIGIN, p, FOV, BEAMS, R) for p in poses])
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    og.set_counts(*synth.counts_from_world(world))
    sm = pkg.ScanMatcher(og, *SMP)
    lv = sm.covering_level("fine", WINDOW[2], shared=False)
    og.checkAndExapndOG([WINDOW[0] - lv.reach, WINDOW[0] + lv.reach], [WINDOW[1] - lv.reach, WINDOW[1] + lv.reach])
    eng = og.engine()
    eng.field_build(lv, eng.to_device([[WINDOW[0], WINDOW[1]]]), 2)
    assert not int(eng.take_flags()[0])
    fr = lv.frames()[0]
    field = lv.field_cost(0).copy()
    assert field.shape == (289, 289) and (field > 0).any() and (field == 0).any()
    free = int(engine.encode_cost(lv.floor_value, lv.cost_scale))
    lut, shift = engine.weight_table(lv.c.cost_scale, TEMPERATURE)
    return dict(og=og, sm=sm, lv=lv, eng=eng, field=field, frame=(float(fr["xlo"]), float(fr["ylo"])), poses=poses, scans=scans, free=free,
                lut=lut, shift=shift, sincos=lambda a: device_sincos(eng, a))


def cloud(scene, k, N, spread=(0.06, 0.06, 0.04), seed=0):
    """N poses about pose k of the walk."""
    rs = np.random.RandomState(1000 * k + N + seed)
    return scene["poses"][k] + rs.standard_normal((N, 3)) * np.array(spread)


def expect(scene, poses, motion, amp, seed, scan, ranges, outside=None, lut=None, shift=None, fov=FOV):
    poses = np.asarray(poses, dtype=np.float64)
    return mcl.step(scene["field"], scene["frame"], scene["lv"].c.cost_scale, scene["lv"].step, poses[:, :3], motion, amp, seed, scan, ranges,
                    fov, R, scene["free"] if outside is None else outside, scene["lut"] if lut is None else lut,
                    scene["shift"] if shift is None else shift, scene["sincos"])


def launch(scene, poses, motion, amp, seed, scan, ranges, outside=None, lut=None, shift=None, ancestor=True):
    """slam2d_mcl_step at the C ABI with buffers of its own, all of them poisoned with 0xff bytes; the lidar descriptor is a copy
    with the scan's beam count (the call reads only beams, fov and max_range of it).  ``poses``: [N, stride].  Returns dict of
    ``out`` [N, stride] (float64), ``ancestors`` (None without), ``report`` (uint64 [16])."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng, lv = scene["eng"], scene["lv"]
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    N, stride = poses.shape
    lid = _lib.Slam2dLidar.from_buffer_copy(eng.lidar_c)
    lid.beams = len(ranges)
    lut = scene["lut"] if lut is None else np.asarray(lut, dtype=np.uint32)
    d_in, d_rng = eng.to_device(poses), eng.to_device(np.asarray(ranges, dtype=np.float64))
    d_lut = torch.from_numpy(lut.view(np.int32).copy()).to(eng.device)
    n = eng.L.slam2d_mcl_work(N)
    assert n == 5 * N + 1032
    full = lambda shape, dt: torch.full(shape, -1, dtype=dt, device=eng.device)
    work, rep, out = full((n,), torch.int64), full((_lib.MCL_REPORT,), torch.int64), full((N, stride), torch.int64)
    anc = full((N,), torch.int32) if ancestor else None
    _lib.check(eng.L.slam2d_mcl_step(ctypes.byref(lid), ctypes.byref(lv.c), 0, N, d_in.data_ptr(), out.data_ptr(), stride,
                                     (ctypes.c_double * 3)(*motion), (ctypes.c_double * 3)(*amp), seed, scan, d_rng.data_ptr(),
                                     scene["free"] if outside is None else outside, d_lut.data_ptr(), len(lut),
                                     scene["shift"] if shift is None else shift, None if anc is None else anc.data_ptr(),
                                     work.data_ptr(), rep.data_ptr(), engine._stream()), "slam2d_mcl_step")
    return dict(out=out.cpu().numpy().view(np.float64), ancestors=None if anc is None else anc.cpu().numpy(),
                report=rep.cpu().numpy().view(np.uint64))


def same(got, want, what=""):
    """Bits: the poses as 64-bit words (a NaN equals itself), the ancestors, the sixteen words."""
    g, w = np.ascontiguousarray(got["out"][:, :3]).view(np.uint64), np.ascontiguousarray(want["out"]).view(np.uint64)
    assert np.array_equal(got["report"], want["report"]), (what, [hex(v) for v in got["report"]], [hex(v) for v in want["report"]])
    if got["ancestors"] is not None:
        bad = np.flatnonzero(got["ancestors"] != want["ancestors"])
        assert got["ancestors"].dtype == np.int32 and not bad.size, (what, bad[:6].tolist(), got["ancestors"][bad[:6]], want["ancestors"][bad[:6]])
    assert np.array_equal(g, w), (what, np.argwhere(g != w)[:6].tolist())


def lively(res, N):
    """On the yardstick first: the case resamples for real -- more than one survivor, fewer than all, more than one weight."""
    rep = res["report"]
    assert 1 < int(rep[6]) < N and int(rep[3]) > 1 and len(np.unique(res["w"])) > 2 and int(rep[10]) == N, [int(v) for v in rep]


def test_one_step(scene):
    N = 257
    poses, rng = cloud(scene, 0, N), scene["scans"][0]
    want = expect(scene, poses, MOTIONS[0], AMP, 7, 3, rng)
    lively(want, N)
    assert int(want["report"][5]) == int((rng < R).sum()) > 40
    got = launch(scene, poses, MOTIONS[0], AMP, 7, 3, rng)
    same(got, want, "N = 257")
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    assert engine.mcl_report_host(got["report"])["mean_pose"] == mcl.mean_pose(want["report"])


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, K - 1, K, K + 1, 2 * K + 1])
def test_scan_block_boundaries(scene, N):
    """One scan block, one block to the last particle, two blocks (the second with one particle: from K + 1 on the block sums are
    scanned too), three."""
    rng = scene["scans"][2]
    for seed in range(40):                                     # (the first cloud whose LAST particle survives on the yardstick, where blocks are joined)
        poses = cloud(scene, 2, N, seed=seed)
        want = expect(scene, poses, MOTIONS[3], AMP, 0xfeedfacecafebeef, (1 << 40) + N, rng)
        if N <= K or want["ancestors"].max() == N - 1:
            break
    if N > 64:
        lively(want, N)
    if N > K:
        assert want["ancestors"].max() == N - 1 and want["ancestors"].min() < K    # survivors in the first and in the last scan block
    same(launch(scene, poses, MOTIONS[3], AMP, 0xfeedfacecafebeef, (1 << 40) + N, rng), want, f"N = {N}")


def test_five_chained_steps(scene):
    """Ping-pong: every step's resampled set is the next one's input, with another motion, scan and scan number."""
    N = 300
    cur_want = cur_got = cloud(scene, 3, N, spread=(0.1, 0.1, 0.05))
    for i, motion in enumerate(MOTIONS):
        rng = scene["scans"][3 + i]
        want = expect(scene, cur_want, motion, AMP, 99, 40 + i, rng)
        got = launch(scene, cur_got, motion, AMP, 99, 40 + i, rng)
        same(got, want, f"step {i}")
        cur_want, cur_got = want["out"], got["out"]
    assert int(want["report"][6]) > 1


def test_localiser_run_against_the_chain(pkg, scene):
    """Localiser.run on a log is the chain of engine calls on the same inputs, and the yardstick's chain on the Localiser's own
    field; Localiser.step continues it."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    N, S = 130, 4
    phi, true = 0.1, scene["poses"]                            # raw odometry: the walk in a frame of its own (turned and shifted)
    raw = np.column_stack([math.cos(phi) * true[:, 0] - math.sin(phi) * true[:, 1] + 0.4,
                           math.sin(phi) * true[:, 0] + math.cos(phi) * true[:, 1] - 0.3, true[:, 2] + phi])
    readings = [dict(x=float(p[0]), y=float(p[1]), theta=float(p[2]), range=list(map(float, r))) for p, r in zip(raw, scene["scans"])]
    sigma = (0.03, 0.02, 0.015)
    loc = pkg.Localiser(scene["sm"], WINDOW, particles=N, sigma=sigma, temperature=TEMPERATURE, seed=5)
    assert loc.level is not scene["lv"] and loc.outside_cost == scene["free"] and loc.shift == scene["shift"]
    assert np.array_equal(loc.level.field_cost(0), scene["field"])                  # the same static map, the same window: the same field
    start = loc.seed_at(scene["poses"][0], (0.05, 0.05, 0.03))
    assert np.array_equal(loc.poses(), start) and start.shape == (N, 3) and np.abs(start - scene["poses"][0]).max() < 0.2
    reports = loc.run(readings[:S])
    final = loc.poses()
    # the chain through ParticleEngine.mcl_step, and the yardstick's
    eng, lv = loc.eng, loc.level
    amp = [v / math.sqrt(4.0 / 3.0) for v in sigma]
    bufs = [eng.to_device(start), torch.empty((N, 3), dtype=torch.float64, device=eng.device)]
    d_rep = torch.empty(16, dtype=torch.int64, device=eng.device)
    d_lut = torch.from_numpy(scene["lut"].view(np.int32).copy()).to(eng.device)
    cur = start
    for i in range(S):
        motion = localise.odometry_motion(readings[i - 1], readings[i]) if i else (0.0, 0.0, 0.0)
        eng.mcl_step(lv, 0, bufs[i & 1], bufs[1 - (i & 1)], N, motion, amp, 5, i, eng.to_device(scene["scans"][i]), scene["free"], d_lut,
                     scene["shift"], d_rep)
        want = expect(scene, cur, motion, amp, 5, i, scene["scans"][i])
        cur = want["out"]
        words = d_rep.cpu().numpy().view(np.uint64)
        assert np.array_equal(words, want["report"]), i
        assert reports[i] == engine.mcl_report_host(words), i
        assert np.array_equal(bufs[1 - (i & 1)].cpu().numpy().view(np.uint64), cur.view(np.uint64)), i
    assert np.array_equal(final.view(np.uint64), np.ascontiguousarray(cur).view(np.uint64))
    # one more scan through step(): one call, the report decoded
    motion = localise.odometry_motion(readings[S - 1], readings[S])
    est = loc.step(readings[S], motion)
    want = expect(scene, cur, motion, amp, 5, S, scene["scans"][S])
    assert est["mean_pose"] == mcl.mean_pose(want["report"]) and est["distinct"] == int(want["report"][6])
    assert np.array_equal(loc.poses().view(np.uint64), np.ascontiguousarray(want["out"]).view(np.uint64))
    x, y, th = est["mean_pose"]
    assert math.hypot(x - scene["poses"][S][0], y - scene["poses"][S][1]) < 0.15     # (it tracks: the walk's true pose)
    # the other seedings draw from the same generator, host-side
    peaks = [(1.0, 2.0, 0.5), (-3.0, 0.5, -1.0), (0.0, 0.0, 3.0)]
    p = loc.seed_from_peaks(peaks, 0.1)
    assert all(np.abs(p[i::3] - np.array(peaks[i])).max() < 0.4 for i in range(3))
    u = loc.seed_uniform()
    assert np.abs(u[:, :2]).max() <= 8.0 and np.abs(u[:, 2]).max() <= math.pi and len(np.unique(u[:, 0])) == N
    with pytest.raises(ValueError):
        loc.step(scene["scans"][0][:5], (0, 0, 0))


def test_same_bits_on_every_call_and_other_bits_for_another_key(scene):
    N = 200
    poses, rng = cloud(scene, 5, N), scene["scans"][5]
    a = launch(scene, poses, MOTIONS[2], AMP, 11, 22, rng)
    b = launch(scene, poses, MOTIONS[2], AMP, 11, 22, rng)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    same(a, expect(scene, poses, MOTIONS[2], AMP, 11, 22, rng), "poisoned buffers")
    for seed, scan in ((12, 22), (11, 23), (11 + (1 << 32), 22), (11, 22 + (1 << 32))):        # (the high halves count too)
        c = launch(scene, poses, MOTIONS[2], AMP, seed, scan, rng)
        assert c["out"].tobytes() != a["out"].tobytes(), (seed, scan)
        same(c, expect(scene, poses, MOTIONS[2], AMP, seed, scan, rng), f"seed {seed}, scan {scan}")


def test_no_noise_is_the_closed_form_move(scene):
    N = 150
    poses, rng = cloud(scene, 6, N), scene["scans"][6]
    motion = MOTIONS[4]
    got = launch(scene, poses, motion, (0.0, 0.0, 0.0), 3, 4, rng)
    c, s = scene["sincos"](poses[:, 2].copy())
    x = (poses[:, 0] + c * motion[0]) - s * motion[1]
    y = (poses[:, 1] + s * motion[0]) + c * motion[1]
    closed = np.stack([x, y, poses[:, 2] + motion[2]], axis=1)
    assert np.array_equal(got["out"], closed[got["ancestors"]])
    # ... whatever the generator does: any g gives the same moved poses at amplitude 0
    assert np.array_equal(mcl.move(poses, motion, (0.0, 0.0, 0.0), np.full((N, 3), 3.9), c, s), closed)
    same(got, expect(scene, poses, motion, (0.0, 0.0, 0.0), 3, 4, rng), "amp = 0")


def test_a_scan_without_a_beam_in_range(scene):
    N = 140
    poses = cloud(scene, 1, N)
    rng = np.full(BEAMS, R)
    rng[::7], rng[3::11] = np.nan, np.inf
    want = expect(scene, poses, MOTIONS[0], AMP, 1, 1, rng)
    assert not want["cost"].any() and np.array_equal(want["ancestors"], np.arange(N)) and int(want["report"][5]) == 0
    assert [int(v) for v in want["report"][:4]] == [0, 0, N * 0xffffff, N] and int(want["report"][6]) == N
    same(launch(scene, poses, MOTIONS[0], AMP, 1, 1, rng), want, "nothing in range")


def test_a_table_of_one_entry_keeps_the_minimum_and_ties_go_in_index_order(scene):
    """Only lut[0] != 0: only particles at the minimum cost survive.  Four copies of one pose among the others, no noise: the
    copies tie, and where they hold the minimum they share the offspring in index order."""
    N = 96
    rng = scene["scans"][4]
    poses = cloud(scene, 4, N, spread=(0.3, 0.3, 0.2))
    lut = np.zeros(64, dtype=np.uint32)
    lut[0] = 1000
    first = expect(scene, poses, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0, 0, rng, lut=lut, shift=0)
    best = int(first["report"][1])
    tied = sorted({best, 5, 40, 77, 95})
    poses[tied] = poses[best]
    want = expect(scene, poses, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0, 0, rng, lut=lut, shift=0)
    assert np.flatnonzero(want["w"]).tolist() == tied and int(want["report"][1]) == tied[0] and int(want["report"][3]) == len(tied)
    assert sorted(set(want["ancestors"].tolist())) == tied and (np.diff(want["ancestors"]) >= 0).all()
    assert np.ptp(np.bincount(want["ancestors"], minlength=N)[tied]) <= 1
    same(launch(scene, poses, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0, 0, rng, lut=lut, shift=0), want, "one entry")


def test_an_all_zero_table_is_the_identity(scene):
    N = 70
    poses, rng = cloud(scene, 7, N), scene["scans"][7]
    lut = np.zeros(16, dtype=np.uint32)
    want = expect(scene, poses, MOTIONS[1], AMP, 8, 9, rng, lut=lut, shift=5)
    assert np.array_equal(want["ancestors"], np.arange(N)) and [int(v) for v in want["report"][2:5]] == [0, 0, 0] and int(want["report"][6]) == N
    same(launch(scene, poses, MOTIONS[1], AMP, 8, 9, rng, lut=lut, shift=5), want, "all-zero table")


BAD = [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.1), (0.5, 0.5, np.nan), (0.5, 0.5, -np.inf), (1e12, 0.0, 0.0), (0.0, -1e12, 0.3), (1e300, 1e300, 0.0),
       (-np.inf, np.nan, np.inf), (40.0, 40.0, 0.3), (-14.0, 0.0, 3.0), (0.0, 14.2, 1.5), (2.0 ** 20 + 1, 0.0, 0.0), (0.0, -(2.0 ** 20) - 1, 0.0)]


@pytest.mark.parametrize("table", ["weights", "flat"])
def test_degenerate_poses_among_good_ones(scene, table):
    """NaN, inf, 1e12 and poses outside the field, mixed among good ones: nothing faults, the counts match.  With the weight
    table the good ones take the offspring; with a flat one every pose is its own offspring and M leaves out exactly those
    whose moved pose is non-finite or beyond 2^20."""
    N = 90
    rng = scene["scans"][8]
    poses = cloud(scene, 8, N)
    where = np.arange(len(BAD)) * 6 + 2
    poses[where] = BAD
    lut, shift = (None, None) if table == "weights" else (np.array([5], dtype=np.uint32), 0)
    want = expect(scene, poses, MOTIONS[0], AMP, 21, 22, rng, lut=lut, shift=shift)
    in_range = int((rng < R).sum())
    assert (want["cost"][where[:8]] == in_range * scene["free"]).all()               # a non-finite or far pose: no inside beam
    assert want["cost"][where[8]] == in_range * scene["free"]                         # (wholly outside the field)
    if table == "flat":
        assert np.array_equal(want["ancestors"], np.arange(N)) and int(want["report"][10]) == N - 10      # (8 non-finite or 1e12, 2 at 2^20)
    else:
        assert not np.isin(want["ancestors"], where[:9]).any() and int(want["report"][10]) == N
    same(launch(scene, poses, MOTIONS[0], AMP, 21, 22, rng, lut=lut, shift=shift), want, table)


def test_a_pose_stride_of_five_and_no_ancestors(scene):
    N = 77
    rng = scene["scans"][9]
    poses = np.hstack([cloud(scene, 9, N), np.full((N, 2), 123.0)])
    want = expect(scene, poses, MOTIONS[2], AMP, 31, 32, rng)
    got = launch(scene, poses, MOTIONS[2], AMP, 31, 32, rng)
    same(got, want, "stride 5")
    assert (got["out"][:, 3:].view(np.uint64) == np.uint64(0xffffffffffffffff)).all()          # slots 3 and 4: as they were
    none = launch(scene, poses, MOTIONS[2], AMP, 31, 32, rng, ancestor=False)
    assert none["ancestors"] is None
    same(none, want, "d_ancestor = NULL")


def test_more_beams_than_one_trip_of_the_beam_loop(scene):
    """1081 beams: 17 trips of 64 -- eight pairs and a single, partial one; N = 66 is a partial last block of the scoring launch."""
    N, B = 66, 1081
    rs = np.random.RandomState(1081)
    rng = rs.uniform(0.2, 1.15 * R, B)
    poses = cloud(scene, 10, N)
    lut, shift = importlib.import_module("slam-2d-lidar-scan_amd.engine").weight_table(scene["lv"].c.cost_scale, 64.0)
    want = expect(scene, poses, MOTIONS[0], AMP, 41, 42, rng, lut=lut, shift=shift)
    assert 0 < int(want["report"][5]) < B and int(want["report"][0]) > 1 << 32        # (sums beyond 32 bits)
    same(launch(scene, poses, MOTIONS[0], AMP, 41, 42, rng, lut=lut, shift=shift), want, "1081 beams")


@pytest.mark.parametrize("beams", [1, 2, 63, 64, 65, 128, 129, 192])
def test_beam_counts(scene, beams):
    """One trip of the beam loop, partial and full; a pair of trips; a pair and a single."""
    N = 40
    rs = np.random.RandomState(beams)
    rng = rs.uniform(0.2, 1.1 * R, beams)
    poses = cloud(scene, 11, N)
    lut, shift = importlib.import_module("slam-2d-lidar-scan_amd.engine").weight_table(scene["lv"].c.cost_scale, 64.0 if beams > 2 else 1.0)
    want = expect(scene, poses, MOTIONS[0], AMP, 51, beams, rng, lut=lut, shift=shift)
    if beams > 2:
        assert 0 < int(want["report"][5]) < beams and int(want["report"][6]) > 1
    same(launch(scene, poses, MOTIONS[0], AMP, 51, beams, rng, lut=lut, shift=shift), want, f"{beams} beams")
