"""slam2d_mcl_step_rays and slam2d_mcl_step_adaptive_rays on the MI355X against their definition in NumPy
(tests/mcl_rays_yardstick.py: the plain steps' yardsticks plus the ray walked sample by sample, no skipping) and against the
device's own slam2d_mcl_step, slam2d_mcl_step_adaptive and slam2d_score_rays: every comparison is np.array_equal on bits -- the
poses as 64-bit words, the ancestors, d_through, all 16 / 24 report words --, every buffer poisoned with 0xff first.  Scene of
tests/test_gpu_rays.py: ONE distance build with the likelihood table leaves field, frame, squared distances and the device's
occupied image, which the yardstick reads together with the device's cos / sin.  The scans of other beam counts are ray-cast on
the host in the same world."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import mcl_adapt_yardstick as ada
import mcl_rays_yardstick as mray
import mcl_yardstick as mcl
import rays_yardstick as ryard
import test_gpu_mcl as tmcl
import test_gpu_mcl_adapt as tada
import test_gpu_rays as trays
from test_gpu_rays import engine, pkg, scene  # noqa: F401  (the module-scoped fixtures: this module's own instances)
from test_score_host import FOV, ORIGIN, R, UNIT, WALL

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
engine_mod = importlib.import_module("slam-2d-lidar-scan_amd.engine")

POISON = np.uint64(0xffffffffffffffff)
TC4 = 2 ** 32 - 1                                              # the charge at stride 4 (below)
WINDOW = trays.WINDOW
MARGIN = math.ceil(WALL / UNIT) + 1                            # matcher.ray_margin(WALL, UNIT) = 6: the default
AMP = tmcl.AMP
MOTION = tmcl.MOTIONS[0]
# The weights.  A cloud half about a pose of the walk and half about that pose moved across its nearest wall (wrong_side): the
# endpoint cost of the two halves differs by tens of the field's saturation cost c_max = log(20) (a beam that ends in free
# space), so a temperature of 24 keeps both halves alive on the endpoints alone; the charge per through beam that a cast beam
# stands for is c_max (Localiser's default: min(stride * outside_cost, 2^32 - 1), and c_max is 0.75 * 2^32 in the field's
# integers), so the displaced half -- tens of through beams at stride 1 -- loses weight by several temperatures and the
# resampling changes.
TEMPERATURE = 24.0
SPREAD = (0.08, 0.08, 0.05)
CASES = [(180, 4, 0), (180, 4, 3), (180, 1, 0), (180, 7, 5), (64, 1, 0), (65, 1, 0), (256, 4, 0), (257, 4, 0), (257, 4, 3), (1, 1, 0), (2, 4, 2)]


def cast_count(beams, stride, phase):
    return (beams - 1 - phase) // stride + 1 if phase < beams else 0


assert [cast_count(*c) for c in CASES] == [45, 45, 180, 25, 64, 65, 64, 65, 64, 1, 0]      # J = 64 | 65: one ray trip | two


# ---- the inputs ----
def stage(s):
    """What the cases share, made once per scene: the wrong-side pair of the walk, the weight table, the charge."""
    if "pair" not in s:
        n, q, _, _ = trays.wrong_side(s["world"], s["poses"], s["scans"])
        lut, shift = engine_mod.weight_table(s["lv"].c.cost_scale, TEMPERATURE)
        s.update(pair=(n, np.array(s["poses"][n], dtype=np.float64), np.array(q, dtype=np.float64)), wlut=lut, shift=shift,
                 charge=s["free"], sincos=lambda a: trays.tscore.device_sincos(s["eng"], a), scans_of={})
        assert s["charge"] < 2 ** 32 < 2 * s["charge"]          # (so every stride above 1 charges 2^32 - 1)
    return s


def scan_of(s, beams, k=None):
    """The scan of ``beams`` beams at pose k of the walk (default: the pair's), ray-cast in the world on the host."""
    k = s["pair"][0] if k is None else k
    if (beams, k) not in s["scans_of"]:
        s["scans_of"][beams, k] = np.asarray(synth.raycast(s["world"], UNIT, ORIGIN, s["poses"][k], FOV, beams, R), dtype=np.float64)
    return s["scans_of"][beams, k]


def cloud(s, N, seed=0, spread=SPREAD):
    """N poses: the even ones about the pair's true pose, the odd ones about the pose across the wall."""
    _, true, moved = s["pair"]
    rs = np.random.RandomState(100 * N + seed)
    return np.where(np.arange(N)[:, None] % 2 == 0, true, moved) + rs.standard_normal((N, 3)) * np.array(spread)


def expect(s, poses, ranges, stride, phase, margin, through_cost, motion=MOTION, amp=AMP, seed=7, scan=3):
    poses = np.asarray(poses, dtype=np.float64)
    return mray.step(s["occ"], s["field"], s["frame"], s["lv"].c.cost_scale, UNIT, poses[:, :3], motion, amp, seed, scan, ranges, FOV, R, s["free"],
                     stride, phase, margin, through_cost, s["wlut"], s["shift"], s["sincos"])


def _buffers(s, poses, ranges):
    import torch
    eng = s["eng"]
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    lid = _lib.Slam2dLidar.from_buffer_copy(eng.lidar_c)
    lid.beams = len(ranges)
    full = lambda shape, dt: torch.full(shape, -1, dtype=dt, device=eng.device)
    d_lut = torch.from_numpy(s["wlut"].view(np.int32).copy()).to(eng.device)
    return torch, eng, poses, lid, full, eng.to_device(poses), eng.to_device(np.asarray(ranges, dtype=np.float64)), d_lut


def launch(s, poses, ranges, stride, phase, margin, through_cost, motion=MOTION, amp=AMP, seed=7, scan=3, ancestor=True, through=True):
    """slam2d_mcl_step_rays at the C ABI with buffers of its own, all of them poisoned with 0xff bytes.  ``poses``: [N, stride].
    Returns dict of ``out`` [N, stride] (float64), ``ancestors``, ``through`` (None without), ``report`` (uint64 [16])."""
    torch, eng, poses, lid, full, d_in, d_rng, d_lut = _buffers(s, poses, ranges)
    N, pstride = poses.shape
    n = eng.L.slam2d_mcl_rays_work(N)
    assert n == 5 * N + 1032
    work, rep, out = full((n,), torch.int64), full((_lib.MCL_REPORT,), torch.int64), full((N, pstride), torch.int64)
    anc, thr = full((N,), torch.int32) if ancestor else None, full((N,), torch.int32) if through else None
    _lib.check(eng.L.slam2d_mcl_step_rays(ctypes.byref(lid), ctypes.byref(s["lv"].c), 0, s["d2"].data_ptr(), N, d_in.data_ptr(), out.data_ptr(),
                                          pstride, (ctypes.c_double * 3)(*motion), (ctypes.c_double * 3)(*amp), seed, scan, d_rng.data_ptr(),
                                          s["free"], stride, phase, margin, through_cost, d_lut.data_ptr(), len(s["wlut"]), s["shift"],
                                          None if anc is None else anc.data_ptr(), None if thr is None else thr.data_ptr(), work.data_ptr(),
                                          rep.data_ptr(), engine_mod._stream()), "slam2d_mcl_step_rays")
    return dict(out=out.cpu().numpy().view(np.float64), ancestors=None if anc is None else anc.cpu().numpy(),
                through=None if thr is None else thr.cpu().numpy(), report=rep.cpu().numpy().view(np.uint64))


def same(got, want, what=""):
    """tests/test_gpu_mcl.py's ``same`` -- poses, ancestors, the sixteen words, word 15 among them -- and d_through."""
    tmcl.same(got, want, what)
    if got["through"] is not None:
        assert got["through"].dtype == np.int32 and np.array_equal(got["through"].astype(np.int64), want["through"]), (
            what, np.flatnonzero(got["through"] != want["through"])[:6].tolist())
    assert int(got["report"][15]) == int(want["through"].sum()), what


def charged_for_real(s, want, poses, ranges, stride, phase, margin):
    """On the yardstick, before a device comparison that claims to test the charge: the case resamples for real, the cloud holds
    particles with and without through beams, and the charge changes the resampling.  (At margin 0 no particle is without: a beam
    that ends on a wall's face meets the wall's first cell at or before sample floor(r / step), so it is through at the true pose
    too.  There the counts have to differ among the particles: more than eight different ones.)"""
    N = len(poses)
    tmcl.lively(want, N)
    if margin:
        assert (want["through"] == 0).any() and (want["through"] > 0).any(), np.bincount(want["through"])[:8]
    else:
        assert len(np.unique(want["through"])) > 8, np.bincount(want["through"])
    free = expect(s, poses, ranges, stride, phase, margin, 0)
    assert np.array_equal(free["through"], want["through"]) and not np.array_equal(free["ancestors"], want["ancestors"])


# ---- 1. against the yardstick ----
@pytest.mark.parametrize("margin", [0, MARGIN])
@pytest.mark.parametrize("beams, stride, phase", CASES)
def test_against_the_yardstick(scene, beams, stride, phase, margin):
    s = stage(scene)
    ranges = scan_of(s, beams)
    through_cost = min(stride * s["charge"], 2 ** 32 - 1)
    poses = cloud(s, 257)                                      # crosses the four-wave blocks; one scan block
    want = expect(s, poses, ranges, stride, phase, margin, through_cost)
    if cast_count(beams, stride, phase) >= 25:
        charged_for_real(s, want, poses, ranges, stride, phase, margin)
    elif not cast_count(beams, stride, phase):
        assert not want["through"].any()
    same(launch(s, poses, ranges, stride, phase, margin, through_cost), want, "N = 257")
    for n in (0, 1):                                           # N = 1: a true pose, a displaced one
        one = expect(s, poses[n:n + 1], ranges, stride, phase, margin, through_cost)
        same(launch(s, poses[n:n + 1], ranges, stride, phase, margin, through_cost), one, f"particle {n} alone")


@pytest.mark.parametrize("margin", [0, 1, MARGIN])
def test_crafted_scans(scene, margin):
    """NaN, inf, 0, -0, negative, out-of-range and on-the-lattice ranges (tests/test_gpu_rays.py), at 60 beams and every phase of
    stride 4: a negative range is in range and never checked, a NaN is neither."""
    s = stage(scene)
    one, _ = trays.crafted_scans(s["scans"])
    poses = cloud(s, 130, seed=1)
    seen = np.zeros(130, dtype=np.int64)
    for phase in range(4):
        want = expect(s, poses, one, 4, phase, margin, TC4)
        same(launch(s, poses, one, 4, phase, margin, TC4), want, f"phase {phase}")
        seen += want["through"]
    all_beams = expect(s, poses, one, 1, 0, margin, s["charge"])
    assert np.array_equal(seen, all_beams["through"]) and seen.max() > 0     # the phases share the beams out
    same(launch(s, poses, one, 1, 0, margin, s["charge"]), all_beams, "stride 1")


def test_a_nan_pose_a_far_pose_a_pose_stride_of_five_and_null_outputs(scene):
    s = stage(scene)
    N = 90
    ranges = scan_of(s, 180)
    poses = np.hstack([cloud(s, N, seed=2), np.full((N, 2), 123.0)])
    poses[7, 1], poses[20, :3], poses[33, 2] = np.nan, (400.0, -300.0, 0.5), np.inf
    want = expect(s, poses, ranges, 4, 1, MARGIN, TC4)
    in_range = int((ranges < R).sum())
    assert (want["through"][[7, 20, 33]] == 0).all() and (want["cost"][[7, 20, 33]] == in_range * s["free"]).all()
    assert not np.isin(want["ancestors"], [7, 20, 33]).any() and (want["through"] > 0).any()
    got = launch(s, poses, ranges, 4, 1, MARGIN, TC4)
    same(got, want, "stride 5")
    assert (got["out"][:, 3:].view(np.uint64) == POISON).all()                 # slots 3 and 4: as they were
    for kw in (dict(ancestor=False), dict(through=False), dict(ancestor=False, through=False)):
        none = launch(s, poses, ranges, 4, 1, MARGIN, TC4, **kw)
        assert (none["ancestors"] is None) == (not kw.get("ancestor", True)) and (none["through"] is None) == (not kw.get("through", True))
        same(none, want, str(kw))


# ---- 2. the equivalences, device against device ----
def plain_scene(s):
    """The scene as tests/test_gpu_mcl.py's ``launch`` reads it."""
    return dict(eng=s["eng"], lv=s["lv"], lut=s["wlut"], shift=s["shift"], free=s["free"])


@pytest.mark.parametrize("N", [257, 1025, 4097])
def test_without_a_charge_or_a_cast_beam_it_is_slam2d_mcl_step(scene, N):
    """Equivalence (i): poses, ancestors and words 0-14 of slam2d_mcl_step itself; 1025 is two scan blocks."""
    s = stage(scene)
    ranges = scan_of(s, 180)
    poses = cloud(s, N, seed=3)
    plain = tmcl.launch(plain_scene(s), poses, MOTION, AMP, 7, 3, ranges)
    assert 1 < int(plain["report"][6]) < N
    for what, (stride, phase, cost) in dict(free=(4, 2, 0), none_cast=(2048, 180, 12345), last_phase=(181, 180, 999)).items():
        got = launch(s, poses, ranges, stride, phase, MARGIN, cost)
        assert got["out"].tobytes() == plain["out"].tobytes() and np.array_equal(got["ancestors"], plain["ancestors"]), what
        assert np.array_equal(got["report"][:15], plain["report"][:15]), what
        assert int(got["report"][15]) == int(got["through"].astype(np.int64).sum()) and (got["through"] >= 0).all(), what
        assert (int(got["report"][15]) > 0) == (what == "free"), what


def test_at_stride_1_without_motion_it_is_slam2d_score_rays(scene):
    """Equivalence (ii): word 0 the minimum of slam2d_score_rays' cost over the input poses, word 1 the lowest index that
    attains it, d_through its slot 4."""
    s = stage(scene)
    N = 1025
    ranges = scan_of(s, 180)
    poses = cloud(s, N, seed=4)
    poses[600] = poses[3]                                      # (a tie somewhere: the lowest index wins)
    rows = trays.score_call(s, s["d2"], poses, ranges, MARGIN, s["free"], s["charge"], beams=180)
    got = launch(s, poses, ranges, 1, 0, MARGIN, s["charge"], motion=(0.0, 0.0, 0.0), amp=(0.0, 0.0, 0.0))
    assert np.array_equal(got["through"].astype(np.float64), rows[:, 4]) and rows[:, 4].min() == 0 and rows[:, 4].max() > 5
    assert int(got["report"][0]) == int(rows[:, 0].min()) and int(got["report"][1]) == int(np.argmin(rows[:, 0]))
    assert int(got["report"][15]) == int(rows[:, 4].sum()) and int(got["report"][5]) == int(rows[0, 3])


def test_the_same_call_twice_gives_the_same_bytes(scene):
    s = stage(scene)
    ranges, poses = scan_of(s, 180), cloud(s, 300, seed=5)
    a, b = (launch(s, poses, ranges, 4, 1, MARGIN, TC4) for _ in range(2))
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


# ---- 3. the two poses either side of a wall ----
@pytest.mark.parametrize("stride", [1, 4])
def test_the_pose_across_the_wall_has_more_beams_through(scene, stride):
    s = stage(scene)
    n, true, moved = s["pair"]
    poses, ranges = np.array([true, moved]), s["scans"][n]
    through_cost = min(stride * s["free"], 2 ** 32 - 1)
    for phase in range(stride):
        want = expect(s, poses, ranges, stride, phase, MARGIN, through_cost, motion=(0.0, 0.0, 0.0), amp=(0.0, 0.0, 0.0))
        assert want["through"][1] > want["through"][0], (phase, want["through"])               # on the yardstick first
        got = launch(s, poses, ranges, stride, phase, MARGIN, through_cost, motion=(0.0, 0.0, 0.0), amp=(0.0, 0.0, 0.0))
        same(got, want, f"stride {stride}, phase {phase}")
        assert got["through"][1] > got["through"][0]
        print(f"stride {stride}, phase {phase}: through {got['through'][0]} at the true pose, {got['through'][1]} across the wall")


# ---- 4. the adaptive step ----
BINS = tada.BINS
TAB3 = tada.TAB3


def expect_adaptive(s, poses, n_in, n_cap, ranges, stride, phase, margin, through_cost, ntab=TAB3, seed=7, scan=3):
    return mray.step_adaptive(s["occ"], s["field"], s["frame"], s["lv"].c.cost_scale, UNIT, np.asarray(poses, dtype=np.float64)[:, :3], n_in, n_cap,
                              MOTION, AMP, seed, scan, ranges, FOV, R, s["free"], stride, phase, margin, through_cost, s["wlut"], s["shift"],
                              BINS, ntab, s["sincos"])


def launch_adaptive(s, poses, n_in, ranges, stride, phase, margin, through_cost, ntab=TAB3, seed=7, scan=3):
    """slam2d_mcl_step_adaptive_rays at the C ABI, every buffer poisoned; tests/test_gpu_mcl_adapt.py's dict plus ``through``."""
    torch, eng, poses, lid, full, d_in, d_rng, d_lut = _buffers(s, poses, ranges)
    n_cap, pstride = poses.shape
    ntab = np.ascontiguousarray(ntab, dtype=np.uint32)
    cb = tada.c_bins(BINS)
    d_ntab = torch.from_numpy(ntab.view(np.int32).copy()).to(eng.device)
    d_n_in = torch.from_numpy(np.array([n_in], dtype=np.uint32).view(np.int32)).to(eng.device)
    n = eng.L.slam2d_mcl_adapt_rays_work(n_cap, ctypes.byref(cb))
    assert n == eng.L.slam2d_mcl_adapt_work(n_cap, ctypes.byref(cb)) > 0
    work, rep, out = full((n,), torch.int64), full((_lib.MCL_ADAPT_REPORT,), torch.int64), full((n_cap, pstride), torch.int64)
    anc, thr, d_n_out = full((n_cap,), torch.int32), full((n_cap,), torch.int32), full((1,), torch.int32)
    _lib.check(eng.L.slam2d_mcl_step_adaptive_rays(ctypes.byref(lid), ctypes.byref(s["lv"].c), 0, s["d2"].data_ptr(), n_cap, d_n_in.data_ptr(),
                                                   d_n_out.data_ptr(), d_in.data_ptr(), out.data_ptr(), pstride, (ctypes.c_double * 3)(*MOTION),
                                                   (ctypes.c_double * 3)(*AMP), seed, scan, d_rng.data_ptr(), s["free"], stride, phase, margin,
                                                   through_cost, d_lut.data_ptr(), len(s["wlut"]), s["shift"], ctypes.byref(cb),
                                                   d_ntab.data_ptr(), len(ntab), anc.data_ptr(), thr.data_ptr(), work.data_ptr(), rep.data_ptr(),
                                                   engine_mod._stream()), "slam2d_mcl_step_adaptive_rays")
    return dict(out=out.cpu().numpy().view(np.uint64), ancestors=anc.cpu().numpy(), through=thr.cpu().numpy(),
                report=rep.cpu().numpy().view(np.uint64), n_out=int(d_n_out.cpu().numpy().view(np.uint32)[0]))


def test_the_adaptive_step_against_the_yardstick(scene):
    s = stage(scene)
    n_cap, n_in = 257, 200
    ranges = scan_of(s, 180)
    poses = tada.padded(cloud(s, n_in, seed=6), n_cap)
    want = expect_adaptive(s, poses, n_in, n_cap, ranges, 4, 2, MARGIN, TC4)
    tada.for_real(want)
    assert (want["through"] == 0).any() and (want["through"] > 0).any()
    free = expect_adaptive(s, poses, n_in, n_cap, ranges, 4, 2, MARGIN, 0)
    assert not np.array_equal(free["ancestors"], want["ancestors"])
    got = launch_adaptive(s, poses, n_in, ranges, 4, 2, MARGIN, TC4)
    tada.same(got, want, "200 of 257")
    assert np.array_equal(got["through"][:n_in].astype(np.int64), want["through"]) and (got["through"][n_in:] == -1).all()   # rows >= N: the poison
    assert int(got["report"][15]) == int(want["through"].sum())


def test_a_constant_table_at_the_capacity_is_slam2d_mcl_step_rays(scene):
    """Equivalence (iii), device against device."""
    s = stage(scene)
    N = 1025
    ranges = scan_of(s, 180)
    poses = cloud(s, N, seed=8)
    plain = launch(s, poses, ranges, 4, 3, MARGIN, TC4)
    got = launch_adaptive(s, poses, N, ranges, 4, 3, MARGIN, TC4, ntab=np.full(64, N, dtype=np.uint32))
    assert got["n_out"] == N and got["out"].tobytes() == plain["out"].view(np.uint64).tobytes()
    assert np.array_equal(got["ancestors"], plain["ancestors"]) and np.array_equal(got["through"], plain["through"])
    assert np.array_equal(got["report"][:16], plain["report"]) and int(got["report"][19]) == int(got["report"][6]) and int(got["report"][15]) > 0


# ---- 5. Localiser ----
def readings_of(s, S=4):
    phi, true = 0.1, np.asarray(s["poses"])                    # raw odometry: the walk in a frame of its own (turned and shifted)
    raw = np.column_stack([math.cos(phi) * true[:, 0] - math.sin(phi) * true[:, 1] + 0.4,
                           math.sin(phi) * true[:, 0] + math.cos(phi) * true[:, 1] - 0.3, true[:, 2] + phi])
    return [dict(x=float(p[0]), y=float(p[1]), theta=float(p[2]), range=list(map(float, r))) for p, r in zip(raw[:S], s["scans"][:S])]


def test_a_localiser_with_a_free_charge_is_the_localiser_without(pkg, scene):
    s = stage(scene)
    readings = readings_of(s)
    reports = []
    for rays in (None, dict(through_cost=0)):
        loc = pkg.Localiser(s["sm"], WINDOW, particles=130, temperature=TEMPERATURE, seed=5, likelihood=trays.LIK, rays=rays)
        assert (loc.rays is None) == (rays is None) and hasattr(loc, "d_dist2") == (rays is not None)
        loc.seed_at(s["poses"][0], (0.3, 0.3, 0.1))
        reports.append((loc.run(readings), loc.poses()))
    (plain, p_plain), (charged, p_charged) = reports
    assert all("through" not in r for r in plain) and all(r["through"] > 0 for r in charged)
    assert [{k: v for k, v in r.items() if k != "through"} for r in charged] == plain
    assert p_plain.tobytes() == p_charged.tobytes()
    with pytest.raises(ValueError, match="rays"):
        loc.step_points(np.zeros((4, 2)), (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="rays"):
        loc.run_points([np.zeros((4, 2))], [(0.0, 0.0, 0.0)])
    with pytest.raises(ValueError, match="rays"):
        pkg.Localiser(s["sm"], WINDOW, particles=16, rays=dict(stride=0))


@pytest.mark.parametrize("likelihood", [trays.LIK, None])
@pytest.mark.parametrize("adaptive", [None, dict(n_min=64)])
def test_localiser_run_is_the_chain_of_engine_calls_with_rotating_phases(pkg, scene, likelihood, adaptive):
    import torch
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    s = stage(scene)
    N, S = 130, 4
    readings = readings_of(s, S)
    sigma = (0.03, 0.02, 0.015)
    make = lambda: pkg.Localiser(s["sm"], WINDOW, particles=N, sigma=sigma, temperature=TEMPERATURE, seed=5, likelihood=likelihood, adaptive=adaptive,
                                 rays=dict(stride=4))
    loc = make()
    assert loc.rays == dict(stride=4, margin=MARGIN, through_cost=min(4 * loc.outside_cost, 2 ** 32 - 1), rotate=True)
    fr = loc.level.frames()[0]
    assert (float(fr["xlo"]), float(fr["ylo"])) == s["frame"] and np.array_equal(trays.tdist.device_occ(loc.level)[0], s["occ"]) if likelihood else True
    start = loc.seed_at(s["poses"][0], (0.3, 0.3, 0.1))
    reports = loc.run(readings)
    final = loc.poses()
    # the hand-driven loop on the Localiser's own field and distances: phases 0, 1, 2, 3
    eng, lv = loc.eng, loc.level
    amp = [v / math.sqrt(4.0 / 3.0) for v in sigma]
    bufs = [eng.to_device(start), torch.zeros((N, 3), dtype=torch.float64, device=eng.device)]
    d_rep = torch.empty(loc.d_report.numel(), dtype=torch.int64, device=eng.device)
    d_count = torch.full((1,), N, dtype=torch.int32, device=eng.device)
    for i in range(S):
        motion = localise.odometry_motion(readings[i - 1], readings[i]) if i else (0.0, 0.0, 0.0)
        charge = (4, i % 4, MARGIN, loc.rays["through_cost"])
        d_rng = eng.to_device(np.asarray(readings[i]["range"]))
        if adaptive is None:
            eng.mcl_step_rays(lv, 0, loc.d_dist2, bufs[i & 1], bufs[1 - (i & 1)], N, motion, amp, 5, i, d_rng, loc.outside_cost, *charge, loc.d_lut,
                              loc.shift, d_rep)
        else:
            eng.mcl_step_adaptive_rays(lv, 0, loc.d_dist2, bufs[i & 1], bufs[1 - (i & 1)], N, d_count, motion, amp, 5, i, d_rng, loc.outside_cost,
                                       *charge, loc.d_lut, loc.shift, loc.bins, loc.d_ntab, d_rep)
        assert reports[i] == engine_mod.mcl_rays_report_host(d_rep), i
    assert sum(r["through"] for r in reports) > 0
    n = int(d_count.cpu()[0]) if adaptive else N
    assert bufs[S & 1][:n].cpu().numpy().tobytes() == final.tobytes()
    # run equals four steps
    again = make()
    again.seed_at(s["poses"][0], (0.3, 0.3, 0.1))
    steps = [again.step(readings[i], localise.odometry_motion(readings[i - 1], readings[i]) if i else (0.0, 0.0, 0.0)) for i in range(S)]
    assert steps == reports and again.poses().tobytes() == final.tobytes()
    # rotate=False keeps phase 0: the first scan agrees, a later one casts other beams
    fixed = pkg.Localiser(s["sm"], WINDOW, particles=N, sigma=sigma, temperature=TEMPERATURE, seed=5, likelihood=likelihood, adaptive=adaptive,
                          rays=dict(stride=4, rotate=False))
    fixed.seed_at(s["poses"][0], (0.3, 0.3, 0.1))
    other = fixed.run(readings)
    assert other[0] == reports[0] and [r["through"] for r in other] != [r["through"] for r in reports]
