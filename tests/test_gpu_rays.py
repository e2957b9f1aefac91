"""slam2d_cast_rays and slam2d_score_rays on the MI355X against their definition in NumPy (tests/rays_yardstick.py: the ray walked
sample by sample, no skipping): every comparison is np.array_equal.  The yardstick reads the DEVICE's occupied image, field and
frame record and the device's cos / sin of the very beam angles; the results are integers, there is no tolerance.  Scene of
tests/test_gpu_distance.py: unit 0.1 m, range 4 m, FOV pi, 60 beams, the 289 x 289 covering field of a window of half-edge 8 m."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import distance_yardstick as dyard
import lattice_yardstick as lyard
import rays_yardstick as ryard
import score_yardstick as syard
import test_gpu_distance as tdist
import test_gpu_field_slots as tfs
import test_gpu_score as tscore
from test_score_host import BEAMS, FOV, INIT, ORIGIN, R, SIZE, UNIT, WALL, walk

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

WINDOW = tdist.WINDOW
FMAX, FPITCH = tdist.FMAX, tdist.FPITCH
LIK = tdist.LIK
KMAX = math.ceil(R / UNIT)                                     # 40: the samples of a beam of full range
HIT, LEFT, NONE = ryard.HIT << 30, ryard.LEFT << 30, ryard.NONE << 30


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


@pytest.fixture(scope="module")
def engine():
    return importlib.import_module("slam-2d-lidar-scan_amd.engine")


@pytest.fixture(scope="module")
def scene(pkg, engine):
    """The well-mapped world, a covering level of its own filled by ONE distance build with the likelihood table, and what
    that left on the device, downloaded once: occupied image, frame, field, squared distances."""
    world, poses, scans = walk()
    og, sm, lv = tdist.new_grid(pkg, world)
    eng = og.engine()
    centre = eng.to_device([[WINDOW[0], WINDOW[1]]])
    table = engine.likelihood_table(UNIT, LIK["sigma"])
    d2 = eng.field_build_distance(lv, centre, 2, table, dist2=True)
    assert not eng.take_flags(fatal=0xffffffff).any()
    occ, _ = tdist.device_occ(lv)
    fr = lv.frames()[0]
    assert occ.shape == (289, 289) and 1000 < occ.sum() < occ.size // 4
    s = dict(og=og, sm=sm, lv=lv, eng=eng, world=world, poses=poses, scans=scans, centre=centre, table=table, d2=d2, occ=occ,
             frame=(float(fr["xlo"]), float(fr["ylo"])), field=lv.field_cost(0).copy(), free=int(table[0][-1]))
    s["list64"] = pose_list(s)
    return s


def pose_list(s):
    """The 64 poses of cases 1 and 5 and what each is there for; the specials first, the walk, random poses to fill."""
    (xlo, ylo), occ = s["frame"], s["occ"]
    at = lambda j, i, th: (xlo + j * UNIT, ylo + i * UNIT, th)
    i0, j0 = np.argwhere(occ)[len(np.argwhere(occ)) // 2]
    x0, y0, _ = s["poses"][0]
    jc, ic = int((x0 - xlo) / UNIT), int((y0 - ylo) / UNIT)
    assert not occ[ic - 1:ic + 2, jc - 1:jc + 2].any()
    poses = [at(j0 + 0.5, i0 + 0.5, 0.3)]                                                 # 0: in an occupied cell
    poses += [(xlo - 3.0, y0, 0.0), (xlo + 40.0, ylo + 40.0, -2.0)]                        # 1-2: outside the frame
    poses += [at(-0.5, 100.0, 0.0), at(100.0, -0.5, 1.5), at(-0.25, -0.75, 0.8)]           # 3-5: quotients in (-1, 0)
    poses += [at(289.0, 100.0, 3.0), at(288.999, 100.0, 3.0), at(100.0, 289.0, -1.5), at(100.0, 288.999, -1.5)]      # 6-9: the high edge
    poses += [(math.nan, y0, 0.0), (x0, math.inf, 0.0), (x0, y0, math.nan), (x0, -math.inf, math.inf)]               # 10-13
    poses += [at(jc + 0.5, ic + 0.5, m * (math.pi / 4)) for m in range(-4, 5)]             # 14-22: from a cell's centre
    poses += [at(jc, ic, m * (math.pi / 4)) for m in range(-4, 5)]                         # 23-31: from a cell's corner
    poses += [tuple(p) for p in s["poses"]]                                                # 32-43: the walk
    rs = np.random.RandomState(7)
    poses += [(xlo + rs.uniform(0, 28.9), ylo + rs.uniform(0, 28.9), rs.uniform(-math.pi, math.pi)) for _ in range(64 - len(poses))]
    assert len(poses) == 64
    return np.array(poses, dtype=np.float64)


def lidar_of(eng, beams):
    """A copy of the engine's descriptor with another beam count (the calls read only beams, fov, max_range of it)."""
    lid = _lib.Slam2dLidar.from_buffer_copy(eng.lidar_c)
    lid.beams = beams
    return lid


def strided(eng, poses, stride):
    """The poses on the device at ``stride`` doubles apiece, junk between them."""
    rows = np.full((len(poses), stride), 1e300)
    rows[:, :3] = poses
    return eng.to_device(rows)


def cast_call(s, d2, poses, K, beams=BEAMS, stride=3, lvc=None, p_field=0):
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = s["eng"]
    lid = lidar_of(eng, beams)
    out = torch.full((len(poses), beams), -1, dtype=torch.int32, device=eng.device)
    d_pose = strided(eng, poses, stride)                                             # (named: alive until the words are back)
    _lib.check(eng.L.slam2d_cast_rays(ctypes.byref(lid), ctypes.byref(lvc or s["lv"].c), p_field, d2.data_ptr(), len(poses),
                                      d_pose.data_ptr(), stride, K, out.data_ptr(), engine._stream()), "slam2d_cast_rays")
    return out.cpu().numpy().view(np.uint32)


def trig(s, poses, beams=BEAMS):
    return tscore.device_sincos(s["eng"], np.array([syard.beam_angles(p[2], FOV, beams) for p in np.asarray(poses).reshape(-1, 3)]))


def want_cast(s, poses, K, beams=BEAMS, occ=None, frame=None):
    c, sn = trig(s, poses, beams)
    return ryard.cast(s["occ"] if occ is None else occ, frame or s["frame"], UNIT, (FOV, beams, R), poses, K, c, sn)


def same(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:6].tolist(), got[got != want][:6], want[got != want][:6])


# ---- 1. the cast against the yardstick ----
@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, KMAX])
def test_cast_against_the_yardstick(scene, K):
    poses = scene["list64"]
    want = want_cast(scene, poses, K)
    same(cast_call(scene, scene["d2"], poses, K), want, "64 poses")
    same(cast_call(scene, scene["d2"], poses, K, stride=5), want, "stride 5")
    for n in (0, 3, 32):
        same(cast_call(scene, scene["d2"], poses[n:n + 1], K), want[n:n + 1], f"pose {n} alone")
    same(cast_call(scene, scene["d2"], poses[32:33], K, stride=5), want[32:33], "one pose, stride 5")
    # what the list is there for
    assert (want[0] == HIT).all()                                                          # in an occupied cell: HIT at 0
    assert (want[1:6] == LEFT).all() and (want[10:14] == LEFT).all()                       # outside, (-1, 0), non-finite: LEFT at 0
    assert (want[7] != LEFT).any() and (want[9] != LEFT).any()                             # just inside the high edge (6, 8: on it)
    kinds = want >> np.uint32(30)
    assert (kinds == ryard.NONE).any() or K >= 63
    if K >= 63:
        assert (kinds[32:44] == ryard.HIT).any()
        assert ((kinds[14:32] == ryard.HIT) & ((want[14:32] & np.uint32(0x3fffffff)) > 3)).any()
        assert (kinds == ryard.LEFT).sum() >= 9 * BEAMS


def test_the_endpoint_rule_counts_the_same_points_inside(scene):
    """A quotient in (-1, 0) is outside for a ray and cell 0 for an endpoint: slam2d_score_poses with zero ranges at poses 3-5."""
    eng, lv = scene["eng"], scene["lv"]
    poses = scene["list64"][3:6]
    rows = eng.score_poses(lv, 0, eng.to_device(poses), 3, 3, eng.to_device(np.zeros(BEAMS)), 0).cpu().numpy()
    assert (rows[:, 3] == BEAMS).all()
    assert (cast_call(scene, scene["d2"], poses, KMAX) == LEFT).all()


# ---- 2. beam counts ----
@pytest.mark.parametrize("beams", [1, 2, 63, 64, 65, 180, 300])
def test_beam_counts(scene, beams):
    poses = scene["list64"][[0, 3, 7, 12, 15, 24, 32, 37, 44, 50]]
    want = want_cast(scene, poses, KMAX, beams)
    same(cast_call(scene, scene["d2"], poses, KMAX, beams), want, beams)
    assert len(set((want >> np.uint32(30)).ravel().tolist())) >= 2
    rng = np.random.RandomState(beams).uniform(0.2, 4.5, (len(poses), beams))
    c, sn = trig(scene, poses, beams)
    want = ryard.score(scene["occ"], scene["field"], scene["frame"], UNIT, (FOV, beams, R), poses, rng, 1, scene["free"], 7001, c, sn)
    same(score_call(scene, scene["d2"], poses, rng, 1, scene["free"], 7001, beams), want, beams)
    assert want[:, 4].max() > 0


# ---- 3. the cap changes the skips, never the answer ----
def test_every_table_length_gives_the_same_rays(scene):
    eng, sm = scene["eng"], scene["sm"]
    poses, rng = scene["list64"], scene["scans"][3]
    lv2 = sm.covering_level("fine", WINDOW[2], shared=False)
    want = want_cast(scene, poses, KMAX)
    c, sn = trig(scene, poses)
    want_rows = ryard.score(scene["occ"], scene["field"], scene["frame"], UNIT, (FOV, BEAMS, R), poses, rng, 0, scene["free"], 99, c, sn)
    caps = set()
    for which in (2, 3, 4, "identity"):
        lut = tdist.table_of(which, None)
        d2 = eng.field_build_distance(lv2, scene["centre"], 2, (lut, 1.0), dist2=True)
        assert np.array_equal(tdist.device_occ(lv2)[0], scene["occ"]) and lv2.frames()[0].tobytes() == scene["lv"].frames()[0].tobytes()
        caps.add(int(d2[0, :289, :289].max()))
        same(cast_call(scene, d2, poses, KMAX), want, which)
        same(score_call(scene, d2, poses, rng, 0, scene["free"], 99), want_rows, which)      # (the scene's field, this image)
    assert caps == {1, 2, 3, int(dyard.dist2(scene["occ"], 65535).max())}


# ---- 4. an empty image, a frame of one cell, slot 2 of three ----
def test_an_empty_image(pkg, scene):
    og, sm, lv = tdist.new_grid(pkg)
    eng = og.engine()
    d2 = eng.field_build_distance(lv, eng.to_device([[WINDOW[0], WINDOW[1]]]), 2, (tdist.IDENTITY, 1.0), dist2=True)
    occ, _ = tdist.device_occ(lv)
    fr = lv.frames()[0]
    frame = (float(fr["xlo"]), float(fr["ylo"]))
    assert not occ.any() and frame == scene["frame"] and (d2[0, :289, :289] == 65535).all()
    poses = scene["list64"]
    s = dict(scene, eng=eng, lv=lv)
    for K in (3, KMAX, 500):
        want = want_cast(s, poses, K, occ=occ)
        same(cast_call(s, d2, poses, K), want, K)
        kinds = set((want >> np.uint32(30)).ravel().tolist())
        assert kinds == ({ryard.LEFT, ryard.NONE} if K < 500 else {ryard.LEFT})            # 500 samples cross the whole frame


@pytest.mark.parametrize("occupied", [False, True])
def test_a_frame_of_one_cell(pkg, scene, occupied):
    import torch
    og, sm, lv = tdist.new_grid(pkg)
    eng = og.engine()
    eng.field_build_distance(lv, eng.to_device([[WINDOW[0], WINDOW[1]]]), 2, (tdist.IDENTITY, 1.0))
    xlo, ylo = tfs.CRAFTED[2][:2]
    records = lv.frames().copy()
    records[0]["xlo"], records[0]["ylo"], records[0]["fh"], records[0]["fw"] = xlo, ylo, 1, 1
    lv.t["frames"].copy_(torch.from_numpy(records.view(np.uint8).reshape(1, -1)))
    d2 = torch.zeros((1, FMAX, FPITCH), dtype=torch.int32, device=eng.device)              # every other cell reads as a wall
    d2[0, 0, 0] = 0 if occupied else 65535
    rs = np.random.RandomState(3)
    poses = [(xlo + rs.uniform(-0.1, 0.2), ylo + rs.uniform(-0.1, 0.2), rs.uniform(-math.pi, math.pi)) for _ in range(24)]
    poses += [(xlo + 0.05, ylo + 0.05, 0.3), (xlo, ylo, 0.0), (xlo + UNIT, ylo, 0.0), (xlo + 0.099, ylo + 0.099, -2.0)]
    poses = np.array(poses)
    s = dict(scene, eng=eng, lv=lv)
    occ = np.array([[occupied]])
    for K in (0, 1, KMAX):
        want = want_cast(s, poses, K, occ=occ, frame=(xlo, ylo))
        same(cast_call(s, d2, poses, K), want, K)
        kinds = set((want >> np.uint32(30)).ravel().tolist())
        # (a diagonal sample 1 may still lie in the cell; forty samples on, none does)
        assert kinds == {ryard.HIT, ryard.LEFT} if occupied else kinds == {ryard.LEFT} if K == KMAX else {ryard.LEFT} <= kinds <= {ryard.LEFT, ryard.NONE}
        assert occupied or K > 0 or ryard.NONE in kinds
    rng = rs.uniform(0.0, 0.5, (len(poses), BEAMS))
    lv.t["field"].fill_(12345)
    c, sn = trig(s, poses)
    want = ryard.score(occ, np.array([[12345]], dtype=np.uint32), (xlo, ylo), UNIT, (FOV, BEAMS, R), poses, rng, 0, 11, 13, c, sn)
    same(score_call(s, d2, poses, rng, 0, 11, 13), want, "score")
    assert (want[:, 2] > 0).any() and (want[:, 4] > 0).any() == occupied


def test_slot_2_of_a_level_of_three(pkg, engine, scene):
    import torch
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    dev = torch.device("cuda:0")
    lidar = engine.LidarModel.get(UNIT, R, FOV, BEAMS, WALL)
    lv = engine.SearchLevel(lidar, tfs.P, dev, bnb=False, **tfs.level_kw())
    maps = []
    for seed, (cx, cy) in zip(tfs.SEEDS, tfs.CENTRES):
        m = engine.MapState.create(SIZE, SIZE, INIT, UNIT, dev)
        m.upload(*synth.counts_from_world(synth.make_world(SIZE, UNIT, seed=seed, n_boxes=25)))
        m.ensure_contains([cx - lv.reach, cx + lv.reach], [cy - lv.reach, cy + lv.reach], UNIT)
        maps.append(m)
    eng = engine.ParticleEngine(lidar, maps, dev)
    table = engine.likelihood_table(UNIT, LIK["sigma"])
    d2 = eng.field_build_distance(lv, eng.to_device(tfs.CENTRES), 2, table, dist2=True)
    assert not eng.take_flags(fatal=0xffffffff).any()
    s = dict(scene, eng=eng, lv=lv)
    fr = lv.frames()
    rs = np.random.RandomState(11)
    rng = scene["scans"][5]
    for p in range(tfs.P):
        occ, _ = tdist.device_occ(lv, p)
        frame = (float(fr[p]["xlo"]), float(fr[p]["ylo"]))
        assert occ.shape == tfs.SIZES[p]
        poses = np.array([(frame[0] + rs.uniform(0, 28.8), frame[1] + rs.uniform(0, 28.8), rs.uniform(-math.pi, math.pi)) for _ in range(32)])
        want = want_cast(s, poses, KMAX, occ=occ, frame=frame)
        same(cast_call(s, d2, poses, KMAX, p_field=p), want, f"slot {p}")
        same(eng.cast_rays(lv, p, d2, eng.to_device(poses), 3, len(poses), KMAX).cpu().numpy().view(np.uint32), want, f"engine, slot {p}")
        c, sn = trig(s, poses)
        want_rows = ryard.score(occ, lv.field_cost(p), frame, UNIT, (FOV, BEAMS, R), poses, rng, 1, scene["free"], 5, c, sn)
        same(score_call(s, d2, poses, rng, 1, scene["free"], 5, p_field=p), want_rows, f"score, slot {p}")
        # the same poses in either other slot's image give other words: a wrong offset cannot pass
        c, sn = trig(s, poses)
        on = lambda q: ryard.cast(tdist.device_occ(lv, q)[0][:288, :288], frame, UNIT, (FOV, BEAMS, R), poses, KMAX, c, sn)
        assert all(not np.array_equal(on(q), on(p)) for q in range(tfs.P) if q != p)
    with pytest.raises(ValueError):
        eng.cast_rays(lv, 3, d2, eng.to_device(poses), 3, len(poses), KMAX)
    with pytest.raises(ValueError):
        eng.score_rays(lv, -1, d2, eng.to_device(poses), 3, len(poses), eng.to_device(rng), 0, 1, 1, 1)


# ---- 5. the score, all eight slots ----
def score_call(s, d2, poses, ranges, margin, outside_cost, through_cost, beams=BEAMS, stride=3, p_field=0):
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = s["eng"]
    lid = lidar_of(eng, beams)
    ranges = np.asarray(ranges, dtype=np.float64)
    out = torch.full((len(poses), _lib.RAYS_STRIDE), -1.0, dtype=torch.float64, device=eng.device)
    d_pose, d_rng = strided(eng, poses, stride), eng.to_device(ranges)               # (named: alive until the rows are back)
    _lib.check(eng.L.slam2d_score_rays(ctypes.byref(lid), ctypes.byref(s["lv"].c), p_field, d2.data_ptr(), len(poses),
                                       d_pose.data_ptr(), stride, d_rng.data_ptr(),
                                       0 if ranges.ndim == 1 else ranges.shape[1], margin, outside_cost, through_cost, out.data_ptr(),
                                       engine._stream()), "slam2d_score_rays")
    return out.cpu().numpy()


def crafted_scans(scans):
    """One scan and 64 scans with what a range can be: NaN, inf, 0, -0, negative, out of range, exactly on k * step."""
    one = np.array(scans[2], dtype=np.float64)
    one[[1, 7, 13, 19, 25, 31, 37, 43, 49, 55]] = [math.nan, math.inf, 0.0, -0.5, 17 * UNIT, 3 * UNIT, -0.0, np.float64(29) * UNIT, 4.0, 1e12]
    per = np.array([scans[n % len(scans)] for n in range(64)], dtype=np.float64)
    rs = np.random.RandomState(2)
    for n in range(64):
        b = rs.choice(BEAMS, 8, replace=False)
        per[n, b] = [math.nan, math.inf, 0.0, -rs.uniform(0, 2), rs.randint(0, 40) * UNIT, np.float64(rs.randint(0, 40)) * UNIT, -math.inf, rs.uniform(0, 4)]
    return one, per


@pytest.mark.parametrize("margin", [0, 1, 3, 50])
def test_score_against_the_yardstick(scene, margin):
    poses = scene["list64"]
    one, per = crafted_scans(scene["scans"])
    c, sn = trig(scene, poses)
    for what, rng in (("one scan", one), ("a scan per pose", per)):
        want = ryard.score(scene["occ"], scene["field"], scene["frame"], UNIT, (FOV, BEAMS, R), poses, rng, margin, scene["free"], 654321, c, sn)
        same(score_call(scene, scene["d2"], poses, rng, margin, scene["free"], 654321), want, what)
        same(score_call(scene, scene["d2"], poses, rng, margin, scene["free"], 654321, stride=5), want, what + ", stride 5")
        assert (want[:, 3] > want[:, 5]).all() and (want[:, 5] > 20).all()                 # negative ranges are in range, never checked
        assert (want[10:14, 2] == 0).all() and (want[10:14, 4] == 0).all() and (want[10:14, 5] > 20).all()      # non-finite poses
        if margin == 50:
            assert (want[:, 4] == 0).all() and (want[:, 6] == 0).all()                     # larger than every range
        else:
            kend = ryard.beam_limits(np.broadcast_to(rng, (64, BEAMS)), UNIT, R, margin)[1]
            assert want[0, 4] == (kend[0] >= 0).sum() > 20                                   # from inside a wall: every beam that is asked
            assert (want[32:44, 4] < want[32:44, 5]).all() and want[:, 6].max() > 10


# ---- 6. equivalences on the device ----
def test_equivalences_on_the_device(scene):
    eng, lv = scene["eng"], scene["lv"]
    poses = scene["list64"]
    one, per = crafted_scans(scene["scans"])
    for rng in (one, per):
        rows = score_call(scene, scene["d2"], poses, rng, 1, scene["free"], 0)
        ends = eng.score_poses(lv, 0, eng.to_device(poses), 3, 64, eng.to_device(rng), 0 if rng.ndim == 1 else BEAMS).cpu().numpy()
        assert np.array_equal(rows[:, 1:4], ends[:, [6, 3, 4]])
        # `through` is what the words of the cast say
        words = cast_call(scene, scene["d2"], poses, KMAX)
        _, kend = ryard.beam_limits(np.broadcast_to(rng, (64, BEAMS)), UNIT, R, 1)
        through = (kend >= 0) & (words >> np.uint32(30) == ryard.HIT) & ((words & np.uint32(0x3fffffff)).astype(np.int64) <= kend)
        assert kend.max() <= KMAX and np.array_equal(rows[:, 4], through.sum(axis=1)) and through.any()
    # a dyadic lattice materialised as poses: with through_cost = 0 the cost is slam2d_search_lattice's
    x0, y0, _ = scene["poses"][4]
    lat = (9, 7, 8, float(x0) - 1.0, 0.25, float(y0) - 0.75, 0.25, -2.0, 0.5)
    P = lyard.poses(lat).reshape(-1, 3)
    words = eng.search_host(eng.search_lattice(lv, 0, lat, eng.to_device(one), scene["free"]), lat, lv.c.cost_scale)
    rows = score_call(scene, scene["d2"], P, one, 2, scene["free"], 0)
    cost = rows[:, 0].astype(np.uint64).reshape(8, 7, 9)
    packed = lyard.pack(cost)
    assert np.array_equal(words["cost"], packed >> np.uint64(16)) and np.array_equal(words["heading"], (packed & np.uint64(0xffff)).astype(np.int64))
    charged = score_call(scene, scene["d2"], P, one, 2, scene["free"], 1000)
    assert np.array_equal(charged[:, 0], rows[:, 0] + 1000 * rows[:, 4]) and np.array_equal(charged[:, 1:], rows[:, 1:]) and rows[:, 4].max() > 0


# ---- 7. the same call twice ----
def test_the_same_call_twice_gives_the_same_bits(scene):
    poses = scene["list64"]
    _, per = crafted_scans(scene["scans"])
    a, b = (cast_call(scene, scene["d2"], poses, KMAX) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    a, b = (score_call(scene, scene["d2"], poses, per, 1, scene["free"], 77) for _ in range(2))
    assert a.tobytes() == b.tobytes()


# ---- 8. the Python surface ----
def test_cast_scans(scene):
    sm, eng = scene["sm"], scene["eng"]
    poses = scene["list64"]
    got = sm.castScans(poses, window=WINDOW)
    lvd = sm.last_cover["level"]
    assert set(got) == {"kind", "k", "range"} and len(lvd.distance_table[0]) == 65536 and sm.last_cover["window"] == WINDOW
    occ, _ = tdist.device_occ(lvd)
    assert np.array_equal(occ, scene["occ"])
    want = eng.cast_host(want_cast(scene, poses, KMAX), UNIT)
    for k in want:
        assert got[k].shape == (64, BEAMS) and np.array_equal(got[k], want[k]), k
    assert np.isinf(got["range"]).any() and (got["range"][got["kind"] == 0] == got["k"][got["kind"] == 0] * UNIT).all()
    short = sm.castScans(poses[32:44], window=WINDOW, max_range=1.25)                        # ceil(1.25 / 0.1) = 13 samples
    want = eng.cast_host(want_cast(scene, poses[32:44], 13), UNIT)
    assert np.array_equal(short["k"], want["k"]) and np.array_equal(short["kind"], want["kind"]) and short["k"].max() <= 14
    with pytest.raises(ValueError):
        sm.castScans(np.zeros((0, 3)))


@pytest.mark.parametrize("likelihood", [LIK, None])
def test_score_rays(scene, engine, likelihood):
    matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
    sm, eng = scene["sm"], scene["eng"]
    poses = scene["list64"]
    one, per = crafted_scans(scene["scans"])
    c, sn = trig(scene, poses)
    for rng in (one, per):
        got = sm.scoreRays(poses, rng, window=WINDOW, likelihood=likelihood)
        lv = sm.last_cover["level"]
        free = int(scene["table"][0][-1]) if likelihood else int(engine.encode_cost(lv.floor_value, lv.cost_scale))
        assert sm.last_cover["margin"] == matcher.ray_margin(WALL, UNIT) == 6
        assert sm.last_cover["outside_cost"] == sm.last_cover["through_cost"] == free == sm.outside_cost_of(lv)
        assert lv is sm.covering_level("fine", WINDOW[2], likelihood=likelihood)
        field = lv.field_cost(0)
        if likelihood:
            assert np.array_equal(field, scene["field"])
        else:
            assert not np.array_equal(field, scene["field"]) and lv.cost_scale == engine.cost_scale_for(lv.floor_value)
        want = eng.rays_host(ryard.score(scene["occ"], field, scene["frame"], UNIT, (FOV, BEAMS, R), poses, rng, 6, free, free, c, sn), lv.cost_scale)
        assert set(got) == set(want) == {"cost", "score", "beam_score", "inside", "in_range", "outside", "through", "checked", "depth"}
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    # the keywords reach the call
    got = sm.scoreRays(poses, one, window=WINDOW, likelihood=likelihood, margin=0, through_cost=3, outside_cost=5)
    want = eng.rays_host(ryard.score(scene["occ"], field, scene["frame"], UNIT, (FOV, BEAMS, R), poses, one, 0, 5, 3, c, sn), lv.cost_scale)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert got["through"].max() > 0
    with pytest.raises(ValueError):
        sm.scoreRays(poses, one, window=WINDOW, margin=-1)
    # scorePoses and searchPoses are as they were: the endpoint part of the rows is scorePoses'
    ends = sm.scorePoses(poses, one, window=WINDOW, likelihood=likelihood)
    assert np.array_equal(ends["inside"], got["inside"]) and np.array_equal(ends["in_range"], got["in_range"])


# ---- 9. a pose on the wrong side of a wall ----
def wrong_side(world, poses, scans):
    """(n, displaced pose, through at the true pose, through displaced): walk pose n moved along its shortest beam across the wall
    that beam ends on, chosen with the yardstick on the WORLD's image (a world cell is centred on its lattice point) so that the
    yardstick itself counts more beams through walls at the displaced pose."""
    frame = (ORIGIN[0] - UNIT / 2, ORIGIN[1] - UNIT / 2)
    zeros = np.zeros(world.shape, dtype=np.uint32)
    margin = math.ceil(WALL / UNIT) + 1
    for n, (pose, rng) in enumerate(zip(poses, scans)):
        b = int(np.argmin(rng))
        a = syard.beam_angles(pose[2], FOV, BEAMS)[b]
        for d in np.arange(0.4, 1.6, 0.1):
            q = (pose[0] + (rng[b] + d) * math.cos(a), pose[1] + (rng[b] + d) * math.sin(a), pose[2])
            j, i = int((q[0] - frame[0]) / UNIT), int((q[1] - frame[1]) / UNIT)
            if world[i - 1:i + 2, j - 1:j + 2].any():
                continue
            rows = ryard.score(world, zeros, frame, UNIT, (FOV, BEAMS, R), np.array([pose, q]), rng, margin, 0, 0)
            if rows[1, 4] > rows[0, 4] + 5:
                return n, q, int(rows[0, 4]), int(rows[1, 4])
    raise AssertionError("no displacement found")


def test_a_pose_across_the_nearest_wall_pays_for_its_beams(scene):
    sm = scene["sm"]
    n, q, t_true, t_moved = wrong_side(scene["world"], scene["poses"], scene["scans"])
    assert t_moved > t_true
    poses, rng = np.array([scene["poses"][n], q]), scene["scans"][n]
    got = sm.scoreRays(poses, rng, window=WINDOW, likelihood=LIK)
    c, sn = trig(scene, poses)
    want = ryard.score(scene["occ"], scene["field"], scene["frame"], UNIT, (FOV, BEAMS, R), poses, rng, 6, scene["free"], scene["free"], c, sn)
    assert np.array_equal(got["through"], want[:, 4]) and np.array_equal(got["cost"], want[:, 0].astype(np.uint64))
    print(f"through: {int(got['through'][0])} at the true pose {n}, {int(got['through'][1])} across the wall "
          f"(the world's image: {t_true}, {t_moved}); endpoint cost {int(want[0, 1])} vs {int(want[1, 1])}")
    assert got["through"][1] > got["through"][0]
