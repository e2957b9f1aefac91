"""slam2d_refine_poses_rays on the MI355X against its definition in NumPy (tests/refine_rays_yardstick.py: every candidate's rays
walked sample by sample, no skipping): every comparison is equality on the bits of the 64-bit words, the poses and the through
counts.  The yardstick reads the DEVICE's occupied image, field and frame record and the device's cos / sin of the very beam angles;
the result is a minimum of integer sums: there is no tolerance.  Scene and fixtures of tests/test_gpu_rays.py (unit 0.1 m, range
4 m, FOV pi, the 289 x 289 covering field of a window of half-edge 8 m, filled by ONE distance build with the likelihood table);
scans of another beam count than the grid's 60 are ray-cast in the same world.  Every call is made at the C ABI with buffers of its
own, poisoned with 0xff bytes, unless a test says otherwise."""
import ctypes
import importlib

import numpy as np
import pytest

import refine_rays_yardstick as rr
import refine_yardstick as ryard
import test_gpu_distance as tdist
import test_gpu_field_slots as tfs
import test_gpu_rays as trays
import test_gpu_score as tscore
from test_gpu_rays import engine, pkg, scene  # noqa: F401  (module-scoped fixtures)
from test_score_host import BEAMS, FOV, INIT, ORIGIN, R, SIZE, UNIT, WALL

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")

WINDOW, LIK = trays.WINDOW, trays.LIK
RADII, STEPS = (3, 2, 2), (0.07, 0.05, 0.013)
TABLE, BLOCKS = _lib.REFINE_TABLE, _lib.REFINE_BLOCKS         # the search launch's shape: slam2d_refine_poses' own
assert (TABLE, BLOCKS) == (2048, 1024)


def chunk(N, nth, beams):
    """Headings per block row of the search launch, as include/slam2d.h states it: the plain call's (the second table enlarges
    the block's LDS instead)."""
    return min(max(1, TABLE // beams), -(-nth // -(-BLOCKS // N)))


def charge_of(outside, stride):
    """``ray_options``' default charge: a cast beam stands for ``stride`` beams, within 32 bits."""
    return min(stride * int(outside), 2 ** 32 - 1)


def sincos_of(s):
    return lambda a: tscore.device_sincos(s["eng"], a)


def expect(s, seeds, radii, steps, ranges, outside, stride, phase, margin, through_cost, motion=None, occ=None, field=None, frame=None):
    """The yardstick's (words [N, 2], poses [N, 3], through [N]) with the device's cos / sin; equal seeds (with one scan) are
    computed once."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    if ranges.ndim == 1:
        uniq, inverse = np.unique(seeds.view(np.uint64), axis=0, return_inverse=True)
        seeds_u, inverse = uniq.view(np.float64), inverse.reshape(-1)
    else:
        seeds_u, inverse = seeds, np.arange(len(seeds))
    w, p, t = rr.refine(s["occ"] if occ is None else occ, s["field"] if field is None else field, s["frame"] if frame is None else frame,
                        1.0, UNIT, seeds_u, radii, steps, ranges, FOV, R, outside, stride, phase, margin, through_cost, motion, sincos_of(s))
    return w[inverse], p[inverse], t[inverse]


def launch(s, seeds, radii, steps, ranges, outside, stride, phase, margin, through_cost, motion=None, lvc=None, p=0, d2=None, pose_stride=3,
           ranges_stride=None, beams=None, through=True):
    """slam2d_refine_poses_rays at the C ABI, every buffer of its own and poisoned with 0xff bytes: (words uint64 [N, 2], the output
    pose buffer float64 [N, pose_stride], through int64 [N] -- None where d_through is NULL)."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = s["eng"]
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    N = len(seeds)
    assert 0 <= int(outside) < 2 ** 32 and 0 <= int(through_cost) < 2 ** 32        # (what the call takes: ctypes would truncate)
    lid = trays.lidar_of(eng, ranges.shape[-1] if beams is None else beams)
    if ranges_stride is None:
        ranges_stride = 0 if ranges.ndim == 1 else ranges.shape[-1]
    rows = np.full((N, pose_stride), np.nan)
    rows[:, :3] = seeds
    d_in, d_rng = eng.to_device(rows), eng.to_device(ranges)
    full = lambda n, dt=torch.int64: torch.full((n,), -1, dtype=dt, device=eng.device)
    n_work = eng.L.slam2d_refine_rays_work(N)
    assert n_work == 3 * N
    work, out, d_out, d_thr = full(n_work), full(2 * N), full(N * pose_stride), full(N, torch.int32)
    d2 = s["d2"] if d2 is None else d2
    _lib.check(eng.L.slam2d_refine_poses_rays(ctypes.byref(lid), ctypes.byref(s["lv"].c if lvc is None else lvc), p, d2.data_ptr(), N,
                                              d_in.data_ptr(), d_out.data_ptr(), pose_stride, d_rng.data_ptr(), ranges_stride,
                                              None if motion is None else (ctypes.c_double * 3)(*motion), *[int(r) for r in radii],
                                              *[float(v) for v in steps], int(outside), stride, phase, margin, int(through_cost),
                                              d_thr.data_ptr() if through else None, work.data_ptr(), out.data_ptr(), engine._stream()),
               "slam2d_refine_poses_rays")
    thr = d_thr.cpu().numpy()
    if not through:
        assert (thr == -1).all()                               # NULL: nothing is written anywhere else for it
    return (out.cpu().numpy().view(np.uint64).reshape(N, 2), d_out.cpu().numpy().view(np.float64).reshape(N, pose_stride),
            thr.view(np.uint32).astype(np.int64) if through else None)


def same(got, want, what=""):
    words, poses, thr = got
    want_words, want_poses, want_thr = want
    assert words.shape == want_words.shape and words.dtype == want_words.dtype == np.uint64, what
    bad = (words != want_words).any(axis=1)
    assert np.array_equal(words, want_words), (what, np.flatnonzero(bad)[:6].tolist(), [[hex(v) for v in w] for w in words[bad][:3]],
                                               [[hex(v) for v in w] for w in want_words[bad][:3]])
    finite = np.isfinite(want_poses).all(axis=1)
    assert poses[:, :3][finite].tobytes() == want_poses[finite].tobytes(), (what, "pose bits")
    assert np.array_equal(poses[:, :3], want_poses, equal_nan=True), (what, "poses")
    if poses.shape[1] > 3:                                     # the other slots of the stride are untouched: still 0xff bytes
        assert (poses[:, 3:].view(np.uint64) == np.uint64(2 ** 64 - 1)).all(), (what, "stride")
    if thr is not None:
        assert np.array_equal(thr, want_thr), (what, "through", thr[:8], want_thr[:8])


def seeds_near(s, ks, seed=1, spread=(0.25, 0.25, 0.05)):
    """Seeds near walk poses ks, displaced by up to ``spread``, off the cells."""
    rs = np.random.RandomState(seed)
    ks = np.asarray(ks)
    return s["poses"][ks] + rs.uniform(-1, 1, (len(ks), 3)) * np.array(spread) + (0.0037, -0.0012, 0.0)


KS = [0, 3, 5, 7, 11]


def main_inputs(world, poses, scans, beams):
    """Seven seeds and a scan each, of ``beams`` beams ray-cast in the world at the walk pose the seed belongs to: five near walk
    poses KS -- the fourth on its pose but for a nudge off the cells --, walk pose n moved across its nearest wall (``wrong_side``
    of tests/test_gpu_rays.py) with pose n's scan, and the walk pose with the most room about it with its scan cut to 0.4 m: no
    candidate of that seed sends a beam through anything."""
    n, q, _, _ = trays.wrong_side(world, poses, scans)
    s = dict(poses=np.asarray(poses))
    seeds = seeds_near(s, KS)
    seeds[3] = s["poses"][7] + (0.0037, -0.0012, 0.0)
    roomy = int(np.argmax(np.min(scans, axis=1)))
    assert np.min(scans[roomy]) > 1.0
    seeds = np.vstack([seeds, np.array(q) + (0.0037, -0.0012, 0.0), s["poses"][roomy] + (0.0037, -0.0012, 0.0)])
    rng = np.array([synth.raycast(world, UNIT, ORIGIN, tuple(s["poses"][k]), FOV, beams, R) for k in KS + [n, roomy]])
    rng[-1] = np.minimum(rng[-1], 0.4)
    return seeds, rng


def charged_for_real(plain, charged, what):
    """What keeps a case from passing vacuously, on the yardstick: the charge moves a winner and leaves one, and the winners' through
    counts hold both 0 and a positive value.  (At margin 0 the counts differ from candidate to candidate even at a true pose, as
    tests/test_gpu_mcl_rays.py notes.)"""
    a, b = ryard.index_of(plain[0]), ryard.index_of(charged[0])
    print(f"{what}: winners {a.tolist()} -> {b.tolist()}, through {plain[2].tolist()} -> {charged[2].tolist()}")
    assert (a != b).any() and (a == b).any(), (what, a, b)
    assert (charged[2] == 0).any() and (charged[2] > 0).any(), (what, charged[2])


# ---- 1. against the yardstick: beam counts, strides and phases ----
@pytest.mark.parametrize("beams, stride, phase", [(180, 4, 0), (180, 4, 3), (180, 1, 0), (180, 7, 5), (64, 1, 0), (65, 1, 0), (257, 4, 3),
                                                  (1, 1, 0), (2, 4, 2)])
def test_against_the_yardstick(scene, beams, stride, phase):
    """The kept beams are about 45, 180, 26, 64, 65 and 64, then 1 and 0 (phase 2 of 2 beams: no beam is cast)."""
    seeds, rng = main_inputs(scene["world"], scene["poses"], scene["scans"], beams)
    charge = charge_of(scene["free"], stride)
    want = expect(scene, seeds, RADII, STEPS, rng, scene["free"], stride, phase, 0, charge)
    if beams >= 64:
        charged_for_real(expect(scene, seeds, RADII, STEPS, rng, scene["free"], stride, phase, 0, 0), want, (beams, stride, phase))
    if phase >= beams:
        assert not want[2].any()
    same(launch(scene, seeds, RADII, STEPS, rng, scene["free"], stride, phase, 0, charge), want, (beams, stride, phase))
    assert chunk(len(seeds), 5, beams) == 1                   # a block row per heading: a seed's winner may be any block's


# ---- 2. seeds, positions per heading, headings per block row ----
@pytest.mark.parametrize("N", [1, 2, 65, 257])
def test_seed_counts(scene, N):
    seeds = np.tile(seeds_near(scene, [1, 2, 4, 6, 7, 9, 10], seed=N), (N // 7 + 1, 1))[:N]
    rng = scene["scans"][2]
    args = ((1, 1, 1), (0.1, 0.1, 0.02), rng, scene["free"], 4, 1, 0, charge_of(scene["free"], 4))
    want = expect(scene, seeds, *args)
    assert want[2].max() > 0
    same(launch(scene, seeds, *args), want, f"{N} seeds")


@pytest.mark.parametrize("rx, ry", [(31, 0), (32, 0), (127, 0), (128, 0), (3, 4)])
def test_positions_around_the_wave_and_block_size(scene, rx, ry):
    """63, 65, 255 and 257 positions per heading, three headings: the last wave of a block's candidates is not full, and a wave
    holds lanes of two headings; 63 in a 7 x 9 patch."""
    seeds = seeds_near(scene, [3, 8], seed=rx)
    rng = scene["scans"][3]
    args = ((rx, ry, 1), (0.0123, 0.0171, 0.02), rng, scene["free"], 4, 2, 0, charge_of(scene["free"], 4))
    want = expect(scene, seeds, *args)
    assert (ryard.index_of(want[0]) != 0).any()
    same(launch(scene, seeds, *args), want, f"radii ({rx}, {ry}, 1)")


@pytest.mark.parametrize("N, beams, rt", [(1024, 512, 1), (1024, 512, 2), (512, BEAMS, 4)])
def test_heading_chunks(scene, N, beams, rt):
    """Either side of hc: with 512 beams a block's table holds 4 headings -- nth = 3 is one row of 3, nth = 5 is 4 + 1 --; 512 seeds
    of 60 beams want two rows: 9 headings as 5 + 4."""
    nth = 2 * rt + 1
    hc = chunk(N, nth, beams)
    assert (hc, -(-nth // hc)) == {(1024, 512, 1): (3, 1), (1024, 512, 2): (4, 2), (512, BEAMS, 4): (5, 2)}[(N, beams, rt)]
    rng = synth.raycast(scene["world"], UNIT, ORIGIN, tuple(scene["poses"][7]), FOV, beams, R) if beams != BEAMS else scene["scans"][7]
    seeds = seeds_near(scene, [7, 2, 9, 4, 7, 1, 7, 10], seed=rt) + np.array([0, 0, 0.25]) * (np.arange(8) % 2).reshape(-1, 1)
    seeds = np.tile(seeds, (N // 8, 1))
    args = ((1, 0, rt), (0.1, 0.1, 0.05), rng, scene["free"], 4, 0, 0, charge_of(scene["free"], 4))
    want = expect(scene, seeds, *args)
    jt = ryard.index_of(want[0]) // 3
    if nth > hc:
        assert (jt >= hc).any() and (jt < hc).any(), jt[:8]    # winners in more than one block row
    same(launch(scene, seeds, *args), want, f"{N} seeds, {beams} beams, {nth} headings")


# ---- 3. margins, strides of the buffers, a scan per seed ----
@pytest.fixture(scope="module")
def main60(scene):
    return main_inputs(scene["world"], scene["poses"], scene["scans"], BEAMS)


@pytest.mark.parametrize("margin", [0, 6, 50])
def test_margins(scene, main60, margin):
    seeds, rng = main60
    args = (RADII, STEPS, rng, scene["free"], 2, 1, margin, charge_of(scene["free"], 2))
    want = expect(scene, seeds, *args)
    assert (want[2].max() > 0) == (margin < 50)                # 50: beyond every range
    same(launch(scene, seeds, *args), want, f"margin {margin}")


def test_pose_stride_5_and_a_scan_per_seed_in_padded_rows(scene, main60):
    seeds, rng = main60
    args = (scene["free"], 4, 3, 0, charge_of(scene["free"], 4))
    want = expect(scene, seeds, RADII, STEPS, rng, *args)
    per = np.full((len(seeds), BEAMS + 3), np.nan)
    per[:, :BEAMS] = rng
    same(launch(scene, seeds, RADII, STEPS, per, *args, pose_stride=5, ranges_stride=BEAMS + 3, beams=BEAMS), want, "pose stride 5, rows of beams + 3")
    one = expect(scene, seeds, RADII, STEPS, rng[2], *args)
    assert not np.array_equal(one[0], want[0]) and np.array_equal(one[0][2], want[0][2])
    same(launch(scene, seeds, RADII, STEPS, rng[2], *args, pose_stride=5), one, "one scan for all seeds")
    same(launch(scene, seeds, RADII, STEPS, rng[2], *args, through=False), (one[0], one[1], None), "d_through NULL")
    motion = (0.21, -0.04, 0.03)
    same(launch(scene, seeds, RADII, STEPS, rng, *args, motion=motion), expect(scene, seeds, RADII, STEPS, rng, *args, motion=motion), "motion")


def test_degenerate_seeds(scene):
    x, y, th = scene["poses"][1]
    rng = scene["scans"][1]
    in_range = int((rng < R).sum())
    xlo, ylo = scene["frame"]
    seeds = np.array([(np.nan, y, th), (x, np.inf, th), (x, y, np.nan), (1e12, y, th), (xlo - 3.0, y, 0.0), (xlo + 40.0, ylo + 40.0, -2.0),
                      (x + 0.031, y - 0.017, th)])
    args = (RADII, STEPS, rng, 1000, 1, 0, 0, 777)
    want = expect(scene, seeds, *args)
    assert (want[0][:4] == [np.uint64(in_range * 1000) << np.uint64(20), in_range * 1000]).all() and not want[2][:6].any()
    assert ryard.cost_of(want[0])[6] != in_range * 1000      # (the last seed is an ordinary one)
    same(launch(scene, seeds, *args), want, "non-finite seeds and seeds outside the frame")


def test_the_ceiling(scene):
    """2048 beams at stride 1, both costs 2^32 - 1, three candidates: the largest block (80 KiB of LDS) and the largest cost."""
    beams = _lib.MAX_BEAMS
    k = 5
    rng = synth.raycast(scene["world"], UNIT, ORIGIN, tuple(scene["poses"][k]), FOV, beams, R)
    seeds = seeds_near(scene, [k], spread=(0.3, 0.3, 0.05))
    args = ((1, 0, 0), (0.3, 0.1, 0.1), rng, 2 ** 32 - 1, 1, 0, 0, 2 ** 32 - 1)
    want = expect(scene, seeds, *args)
    assert want[2][0] > 0 and int(ryard.cost_of(want[0])[0]) > 2 ** 32
    same(launch(scene, seeds, *args), want, "2048 beams")


# ---- 4. slot 2 of a level of three ----
def test_slot_2_of_a_level_of_three(pkg, engine, scene):
    import torch
    dev = torch.device("cuda:0")
    lidar = engine.LidarModel.get(UNIT, R, FOV, BEAMS, WALL)
    lv = engine.SearchLevel(lidar, tfs.P, dev, bnb=False, **tfs.level_kw())
    worlds = [synth.make_world(SIZE, UNIT, seed=sd, n_boxes=25) for sd in tfs.SEEDS]
    maps = []
    for world, (cx, cy) in zip(worlds, tfs.CENTRES):
        m = engine.MapState.create(SIZE, SIZE, INIT, UNIT, dev)
        m.upload(*synth.counts_from_world(world))
        m.ensure_contains([cx - lv.reach, cx + lv.reach], [cy - lv.reach, cy + lv.reach], UNIT)
        maps.append(m)
    eng = engine.ParticleEngine(lidar, maps, dev)
    d2 = eng.field_build_distance(lv, eng.to_device(tfs.CENTRES), 2, engine.likelihood_table(UNIT, LIK["sigma"]), dist2=True)
    assert not eng.take_flags(fatal=0xffffffff).any()
    p = 2
    fr = lv.frames()
    occ, _ = tdist.device_occ(lv, p)
    frame = (float(fr[p]["xlo"]), float(fr[p]["ylo"]))
    assert occ.shape == tfs.SIZES[p] == (288, 289)
    walk = np.array(synth.random_walk(worlds[p], UNIT, tfs.ORIGIN, 12, seed=5))
    rng = synth.raycast(worlds[p], UNIT, tfs.ORIGIN, walk[2], FOV, BEAMS, R)
    seeds = walk[[1, 2, 3]] + (0.231, -0.122, 0.01)
    s = dict(scene, eng=eng, lv=lv)
    args = (RADII, STEPS, rng, scene["free"], 2, 0, 0, charge_of(scene["free"], 2))
    on = lambda q: expect(s, seeds, *args, occ=tdist.device_occ(lv, q)[0][:288, :288], field=lv.field_cost(q)[:288, :288].copy(),
                          frame=(float(fr[q]["xlo"]), float(fr[q]["ylo"])))
    want = expect(s, seeds, *args, occ=occ, field=lv.field_cost(p).copy(), frame=frame)
    assert all(not np.array_equal(on(q)[0], want[0]) for q in (0, 1)) and want[2].max() > 0      # a wrong offset cannot pass
    same(launch(s, seeds, *args, lvc=lv.c, p=p, d2=d2), want, "slot 2")
    d_thr = torch.full((len(seeds),), -1, dtype=torch.int32, device=dev)
    d_out = eng.to_device(np.zeros_like(seeds))
    words = eng.refine_poses_rays(lv, p, d2, eng.to_device(seeds), d_out, len(seeds), 3, eng.to_device(rng), 0, *args[:2], *args[3:], d_through=d_thr)
    assert np.array_equal(words.cpu().numpy().view(np.uint64), want[0]) and d_out.cpu().numpy().tobytes() == want[1].tobytes()
    assert np.array_equal(d_thr.cpu().numpy(), want[2])       # ParticleEngine.refine_poses_rays, the same call
    with pytest.raises(ValueError):
        eng.refine_poses_rays(lv, 3, d2, eng.to_device(seeds), d_out, len(seeds), 3, eng.to_device(rng), 0, *args[:2], *args[3:])
    with pytest.raises(ValueError):
        eng.refine_poses_rays(lv, p, d2, eng.to_device(seeds), d_out, len(seeds), 3, eng.to_device(rng), 0, *args[:2], *args[3:], d_through=d_thr[:2])


# ---- 5. the equivalences on the device, and the same call twice ----
def plain_call(s, seeds, radii, steps, ranges, outside, motion=None):
    """slam2d_refine_poses through the engine: (words, poses)."""
    eng = s["eng"]
    ranges = np.asarray(ranges, dtype=np.float64)
    d_out = eng.to_device(np.zeros((len(seeds), 3)))
    words = eng.refine_poses(s["lv"], 0, eng.to_device(seeds), d_out, len(seeds), 3, eng.to_device(ranges), 0 if ranges.ndim == 1 else ranges.shape[1],
                             radii, steps, outside, motion=motion)
    return words.cpu().numpy().view(np.uint64), d_out.cpu().numpy()


def test_without_a_charge_the_call_is_slam2d_refine_poses(scene, main60):
    seeds, rng = main60
    motion = (0.11, -0.03, 0.02)
    words, poses = plain_call(scene, seeds, RADII, STEPS, rng, scene["free"], motion)
    assert (ryard.index_of(words) != 0).any()
    for what, (stride, phase, margin, charge) in {"through_cost 0": (1, 0, 0, 0), "no cast beam": (64, 60, 0, 12345), "a margin beyond every range": (1, 0, 50, 12345),
                                                   "through_cost 0, stride 4": (4, 3, 6, 0)}.items():
        got = launch(scene, seeds, RADII, STEPS, rng, scene["free"], stride, phase, margin, charge, motion=motion)
        assert got[0].tobytes() == words.tobytes() and got[1].tobytes() == poses.tobytes(), what
        assert (got[2].max() > 0) == (what.startswith("through_cost 0")), what           # the count is the winner's all the same


def test_at_stride_1_the_cost_is_slam2d_score_rays_on_the_device(scene, main60):
    """No host trigonometry: the candidates materialised as poses and scored by slam2d_score_rays, same margin and costs."""
    seeds, rng = main60
    margin, charge = 1, 54321
    words, poses, thr = launch(scene, seeds, RADII, STEPS, rng, scene["free"], 1, 0, margin, charge)
    for n, m in enumerate(seeds):
        C = ryard.candidates(m, RADII, STEPS).reshape(-1, 3)
        rows = trays.score_call(scene, scene["d2"], C, rng[n], margin, scene["free"], charge)
        assert np.array_equal(words[n], ryard.pack(rows[:, 0].astype(np.uint64))), n
        f = int(ryard.index_of(words[n])[0])
        assert int(words[n, 1]) == int(rows[0, 0]) and thr[n] == int(rows[f, 4]) and poses[n].tobytes() == C[f].tobytes(), n
    assert thr.max() > 0


def test_the_same_call_twice_gives_the_same_bits(scene, main60):
    seeds, rng = main60
    a, b = (launch(scene, seeds, RADII, STEPS, rng, scene["free"], 4, 1, 0, charge_of(scene["free"], 4), pose_stride=5) for _ in range(2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 6. the Python surface ----
STAGES = (((2, 2, 2), (0.1, 0.1, 0.02)), ((1, 1, 1), (0.05, 0.05, 0.01)))


def cover_of(lv, d2):
    """(occupied image, field, frame) of slot 0 of a covering level and its squared distances: 0 means occupied, nothing else does."""
    fr = lv.frames()[0]
    fh, fw = int(fr["fh"]), int(fr["fw"])
    return (d2[0, :fh, :fw] == 0).cpu().numpy(), lv.field_cost(0).copy(), (float(fr["xlo"]), float(fr["ylo"]))


@pytest.mark.parametrize("likelihood", [LIK, None])
def test_refine_poses_with_rays(scene, main60, likelihood):
    """ScanMatcher.refinePoses(rays=...) is the stages chained on the covering level's own field and the squared distances of
    scoreRays, decoded; without ``rays`` the result is as it was."""
    sm = scene["sm"]
    seeds, rng = main60
    rays = dict(stride=2, phase=1, margin=0)
    res = sm.refinePoses(seeds, rng, stages=STAGES, window=WINDOW, likelihood=likelihood, rays=rays)
    lv = sm.last_cover["level"]
    free = sm.outside_cost_of(lv)
    assert sm.last_cover["rays"] == dict(stride=2, phase=1, margin=0, through_cost=charge_of(free, 2)) and sm.last_cover["outside_cost"] == free
    assert set(res) == {"poses", "cost", "score", "start_cost", "offsets", "through"} and res["through"].shape == (len(seeds), 2)
    field = lv.field_cost(0).copy()
    assert np.array_equal(field, scene["field"]) == (likelihood is not None)
    eng = scene["og"].engine()
    s = dict(scene, eng=eng)
    w, p, t = rr.refine_stages(scene["occ"], field, scene["frame"], 1.0, UNIT, seeds, STAGES, rng, FOV, R, free, 2, 1, 0, charge_of(free, 2),
                               sincos=sincos_of(s))
    assert res["poses"].tobytes() == p.tobytes() and np.array_equal(res["through"], t) and t.max() > 0
    assert np.array_equal(res["cost"], ryard.cost_of(w[:, -1])) and np.array_equal(res["start_cost"], w[:, 0, 1])
    for i, (radii, steps) in enumerate(STAGES):
        assert np.array_equal(res["offsets"][:, i], eng.refine_host(w[:, i], radii, steps, lv.c.cost_scale)["offsets"])
    plain = sm.refinePoses(seeds, rng, stages=STAGES, window=WINDOW, likelihood=likelihood)
    assert set(plain) == {"poses", "cost", "score", "start_cost", "offsets"} and "rays" not in sm.last_cover
    wp, pp = ryard.refine_stages(field, scene["frame"], 1.0, UNIT, seeds, STAGES, rng, FOV, R, free, sincos=sincos_of(s))
    assert plain["poses"].tobytes() == pp.tobytes() and np.array_equal(plain["cost"], ryard.cost_of(wp[:, -1]))
    assert not np.array_equal(plain["poses"], res["poses"])
    with pytest.raises(ValueError, match="rays"):
        sm.refinePoses(seeds, rng, window=WINDOW, rays=dict(stride=2, phase=2))


@pytest.mark.parametrize("likelihood", [LIK, None])
def test_the_tracker_with_rays_scan_by_scan_and_as_a_log(pkg, scene, likelihood):
    """Tracker(rays=...).step over the walk against the yardstick started from the device's previous pose, the phase rotating with
    the scan; Tracker.run over the same log gives the steps' bits; without ``rays`` a Tracker reports as it did."""
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    sm, poses, scans = scene["sm"], scene["poses"], scene["scans"]
    odo = poses + np.arange(len(poses)).reshape(-1, 1) * (0.02, -0.015, 0.01)          # a raw odometry that drifts
    readings = [dict(x=float(o[0]), y=float(o[1]), theta=float(o[2]), range=scans[k]) for k, o in enumerate(odo)]
    rays = dict(stride=3, margin=0)
    tr = pkg.Tracker(sm, WINDOW, stages=STAGES, likelihood=likelihood, rays=rays)
    assert tr.rays == dict(stride=3, margin=0, through_cost=charge_of(tr.outside_cost, 3), rotate=True)
    lv, eng = tr.level, tr.eng
    occ, field, frame = cover_of(lv, tr.d_dist2)
    assert np.array_equal(occ, scene["occ"]) and frame == scene["frame"]
    s = dict(scene, eng=eng)
    tr.set_pose(poses[0])
    reports = []
    for k in range(len(poses)):
        prev = np.array(tr.pose())
        motion = localise.odometry_motion(readings[k - 1], readings[k]) if k else None
        rep = tr.step(readings[k], motion)
        w, want, t = rr.refine_stages(occ, field, frame, 1.0, UNIT, prev, STAGES, scans[k], FOV, R, tr.outside_cost, 3, k % 3, 0,
                                      charge_of(tr.outside_cost, 3), motion, sincos_of(s))
        assert isinstance(rep, localise.TrackRaysReport) and np.array(rep.pose).tobytes() == want[0].tobytes() == np.array(tr.pose()).tobytes(), k
        assert (rep.cost, rep.start_cost) == (int(ryard.cost_of(w[:, -1])[0]), int(w[0, 0, 1])) and np.array_equal(rep.through, t[0]), k
        reports.append(rep)
    assert any(r.offsets.any() for r in reports) and any(r.through.any() for r in reports)
    again = pkg.Tracker(sm, WINDOW, stages=STAGES, likelihood=likelihood, rays=rays)
    again.set_pose(poses[0])
    log = again.run(readings)
    assert len(log) == len(reports) and again.pose() == tr.pose()
    for a, b in zip(log, reports):
        assert np.array(a.pose).tobytes() == np.array(b.pose).tobytes() and (a.cost, a.start_cost) == (b.cost, b.start_cost)
        assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.through, b.through)
    with pytest.raises(ValueError, match="rays"):
        tr.step_points(np.zeros((3, 2)), None)
    plain = pkg.Tracker(sm, WINDOW, stages=STAGES, likelihood=likelihood)
    plain.set_pose(poses[0])
    rep = plain.step(readings[0], None)
    assert isinstance(rep, localise.TrackReport) and plain.d_report.numel() == 3 + 2 * len(STAGES) and not hasattr(plain, "d_dist2")
