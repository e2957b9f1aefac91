"""slam2d_refine_poses on the MI355X against the definition in NumPy (tests/refine_yardstick.py, built on tests/score_yardstick.py
and tests/mcl_yardstick.py): every comparison is np.array_equal on the 64-bit words and on the bits of the poses (equal_nan for
non-finite seeds).  The yardstick reads the DEVICE's field and frame and the device's cos / sin (slam2d_device_sincos); the
result is a minimum of integer sums and three rounded operations: there is no tolerance.  World, lidar and the 289 x 289 field of
tests/test_gpu_search.py.  Every call is made at the C ABI with poisoned buffers of its own unless a test says otherwise."""
import ctypes
import importlib

import numpy as np
import pytest

import mcl_yardstick as mcl
import refine_yardstick as ryard
import score_yardstick as yard
import test_gpu_field_slots as tslots
import test_gpu_search as tsearch
from test_gpu_search import pkg, scene  # noqa: F401  (module-scoped fixtures: the world on the device, its field downloaded once)
from test_score_host import BEAMS, FOV, INIT, R, SIZE, UNIT, WALL

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

RADII, STEPS = (3, 2, 2), (0.07, 0.05, 0.013)
TABLE, BLOCKS = _lib.REFINE_TABLE, _lib.REFINE_BLOCKS         # the search launch's shape: headings per block row, seeds that fill the card
assert (TABLE, BLOCKS) == (2048, 1024)


def chunk(N, nth, beams):
    """Headings per block row of the search launch, as include/slam2d.h states it."""
    return min(max(1, TABLE // beams), -(-nth // -(-BLOCKS // N)))


def sincos_of(scene):
    return lambda a: tsearch.device_sincos(scene["eng"], a)


def expect(scene, seeds, radii, steps, ranges, outside, motion=None, field=None, frame=None, scale=None, step=UNIT, fov=FOV, max_range=R):
    """The yardstick's (words [N, 2], poses [N, 3]) with the device's cos / sin; equal seeds (with one scan) are computed once."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    field = scene["field"] if field is None else field
    frame = scene["frame"] if frame is None else frame
    scale = scene["lv"].c.cost_scale if scale is None else scale
    if ranges.ndim == 1:
        uniq, inverse = np.unique(seeds.view(np.uint64), axis=0, return_inverse=True)
        seeds_u = uniq.view(np.float64)
    else:
        seeds_u, inverse = seeds, np.arange(len(seeds))
    words, poses = ryard.refine(field, frame, scale, step, seeds_u, radii, steps, ranges, fov, max_range, outside, motion, sincos_of(scene))
    return words[inverse.reshape(-1)], poses[inverse.reshape(-1)]


def launch(scene, seeds, radii, steps, ranges, outside, motion=None, level=None, p=0, beams=None, pose_stride=3, ranges_stride=None):
    """slam2d_refine_poses at the C ABI, every buffer of its own and poisoned with 0xff bytes: (words uint64 [N, 2], the output
    pose buffer float64 [N, pose_stride])."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = scene["eng"]
    lvc = scene["lv"].c if level is None else level
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges, dtype=np.float64)
    N = len(seeds)
    lid = _lib.Slam2dLidar.from_buffer_copy(eng.lidar_c)
    lid.beams = ranges.shape[-1] if beams is None else beams
    if ranges_stride is None:
        ranges_stride = 0 if ranges.ndim == 1 else ranges.shape[-1]
    rows = np.full((N, pose_stride), np.nan)
    rows[:, :3] = seeds
    d_in, d_rng = eng.to_device(rows), eng.to_device(ranges)
    full = lambda n: torch.full((n,), -1, dtype=torch.int64, device=eng.device)
    n_work = eng.L.slam2d_refine_work(N)
    assert n_work == 3 * N
    work, out, d_out = full(n_work), full(2 * N), full(N * pose_stride)
    _lib.check(eng.L.slam2d_refine_poses(ctypes.byref(lid), ctypes.byref(lvc), p, N, d_in.data_ptr(), d_out.data_ptr(), pose_stride,
                                         d_rng.data_ptr(), ranges_stride, None if motion is None else (ctypes.c_double * 3)(*motion),
                                         *[int(r) for r in radii], *[float(s) for s in steps], int(outside), work.data_ptr(), out.data_ptr(),
                                         engine._stream()), "slam2d_refine_poses")
    return out.cpu().numpy().view(np.uint64).reshape(N, 2), d_out.cpu().numpy().view(np.float64).reshape(N, pose_stride)


def same(got, want, what=""):
    words, poses = got
    want_words, want_poses = want
    assert words.shape == want_words.shape and words.dtype == want_words.dtype == np.uint64, what
    bad = (words != want_words).any(axis=1)
    assert np.array_equal(words, want_words), (what, np.flatnonzero(bad)[:6].tolist(), [[hex(v) for v in w] for w in words[bad][:3]],
                                               [[hex(v) for v in w] for w in want_words[bad][:3]])
    finite = np.isfinite(want_poses).all(axis=1)
    assert poses[:, :3][finite].tobytes() == want_poses[finite].tobytes(), (what, "pose bits")
    assert np.array_equal(poses[:, :3], want_poses, equal_nan=True), (what, "poses")
    if poses.shape[1] > 3:                                     # the other slots of the stride are untouched: still 0xff bytes
        assert (poses[:, 3:].view(np.uint64) == np.uint64(2 ** 64 - 1)).all(), (what, "stride")


def seeds_near(scene, ks, seed=1, spread=(0.25, 0.25, 0.05)):
    """Seeds near walk poses ks, displaced by up to ``spread``, off the cells."""
    rs = np.random.RandomState(seed)
    ks = np.asarray(ks)
    return scene["poses"][ks] + rs.uniform(-1, 1, (len(ks), 3)) * np.array(spread) + (0.0037, -0.0012, 0.0)


@pytest.fixture(scope="module")
def main_case(scene):
    """Five seeds near walk poses, a scan each; the fourth sits on its pose (but for the nudge off the cells), where its own scan
    costs nothing: the seed itself wins there."""
    ks = [0, 3, 5, 7, 11]
    seeds = seeds_near(scene, ks)
    seeds[3] = scene["poses"][7] + (0.0037, -0.0012, 0.0)
    rng = scene["scans"][ks]
    return seeds, rng, expect(scene, seeds, RADII, STEPS, rng, scene["free"])


def test_main_case(scene, main_case):
    seeds, rng, want = main_case
    idx = ryard.index_of(want[0])
    # on the yardstick first: at least three different winners, the seed itself among them and another candidate too
    assert len(np.unique(idx)) >= 3 and (idx == 0).any() and (idx != 0).any(), idx
    assert yard.min_distance_to_integer(scene["frame"], UNIT, [(s[0], s[1], 0.0) for s in seeds], np.zeros(1), FOV, R) > 1e-5     # off the cells
    same(launch(scene, seeds, RADII, STEPS, rng, scene["free"]), want, "main case")


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257])
def test_seed_counts(scene, N):
    """Three headings: a block row each while the seeds do not fill the card (N * 3 blocks)."""
    assert chunk(N, 3, BEAMS) == 1
    seeds = np.tile(seeds_near(scene, [1, 2, 4, 6, 7, 9, 10], seed=N), (N // 7 + 1, 1))[:N]
    rng = scene["scans"][2]
    want = expect(scene, seeds, (1, 1, 1), (0.1, 0.1, 0.02), rng, scene["free"])
    same(launch(scene, seeds, (1, 1, 1), (0.1, 0.1, 0.02), rng, scene["free"]), want, f"{N} seeds")


@pytest.mark.parametrize("rx, ry", [(31, 0), (32, 0), (127, 0), (128, 0), (0, 32), (3, 4)])
def test_positions_around_the_block_size(scene, rx, ry):
    """63, 65, 255 and 257 positions of one heading on the 256 threads of a block; a column; 63 in a 7 x 9 patch."""
    seeds = seeds_near(scene, [3, 8], seed=rx)
    rng = scene["scans"][3]
    steps = (0.0123, 0.0171, 0.02)
    want = expect(scene, seeds, (rx, ry, 0), steps, rng, scene["free"])
    assert (ryard.index_of(want[0]) != 0).any()
    same(launch(scene, seeds, (rx, ry, 0), steps, rng, scene["free"]), want, f"radii ({rx}, {ry}, 0)")


@pytest.mark.parametrize("N, beams, rt", [(1024, 512, 1), (1024, 512, 2), (1024, 512, 4), (512, BEAMS, 4), (1024, BEAMS, 17), (2048, 700, 2)])
def test_heading_chunks(scene, N, beams, rt):
    """The headings of a block row, where the seeds fill the card or half of it.  nth = 2 rt + 1 is odd, so of C - 1, C, C + 1 and
    2 C + 1 about an even chunk size C the odd ones exist: with 512 beams a block's table holds C = 4 headings -- nth = 3 (one row
    of 3), 5 (4 + 1) and 9 (4 + 4 + 1); 512 seeds want two rows: 9 headings as 5 + 4; with 60 beams C = 34: nth = 35 as 34 + 1;
    with 700 beams C = 2: nth = 5 as 2 + 2 + 1."""
    nth = 2 * rt + 1
    hc = chunk(N, nth, beams)
    assert (hc, -(-nth // hc)) == {(1024, 512, 1): (3, 1), (1024, 512, 2): (4, 2), (1024, 512, 4): (4, 3), (512, BEAMS, 4): (5, 2),
                                    (1024, BEAMS, 17): (34, 2), (2048, 700, 2): (2, 3)}[(N, beams, rt)]
    rs = np.random.RandomState(beams + rt)
    rng = rs.uniform(0.2, 1.1 * R, beams) if beams != BEAMS else scene["scans"][7]
    # eight seeds, every other one turned by a quarter of a radian: winners near the seed's heading and at the far end of the headings
    seeds = seeds_near(scene, [7, 2, 9, 4, 7, 1, 7, 10], seed=rt) + np.array([0, 0, 0.25]) * (np.arange(8) % 2).reshape(-1, 1)
    seeds = np.tile(seeds, (N // 8, 1))
    dth = 0.05 if rt < 10 else 0.011
    radii, steps = ((0, 0, rt), (0.1, 0.1, dth)) if rt == 17 or beams != BEAMS else ((1, 0, rt), (0.1, 0.1, dth))
    want = expect(scene, seeds, radii, steps, rng, scene["free"])
    jt = ryard.index_of(want[0]) // (2 * radii[0] + 1)
    if nth > hc:
        assert (jt >= hc).any() and (jt < hc).any(), jt[:8]    # winners in more than one block row
    same(launch(scene, seeds, radii, steps, rng, scene["free"], beams=beams), want, f"{N} seeds, {beams} beams, {nth} headings")


def test_the_seed_alone(scene):
    seeds = seeds_near(scene, [0, 4, 8])
    rng = scene["scans"][4]
    want = expect(scene, seeds, (0, 0, 0), (0.1, 0.1, 0.02), rng, scene["free"])
    assert (ryard.index_of(want[0]) == 0).all() and (want[0][:, 1] == ryard.cost_of(want[0])).all() and want[1].tobytes() == seeds.tobytes()
    same(launch(scene, seeds, (0, 0, 0), (0.1, 0.1, 0.02), rng, scene["free"]), want, "radii 0")
    for steps in ((0.0, 0.0, 0.0), (-0.07, -0.05, -0.013)):    # steps 0: every candidate is the seed, index 0 wins; negative: mirrored
        want = expect(scene, seeds, RADII, steps, rng, scene["free"])
        same(launch(scene, seeds, RADII, steps, rng, scene["free"]), want, f"steps {steps}")
    assert (ryard.index_of(expect(scene, seeds, RADII, (0.0, 0.0, 0.0), rng, scene["free"])[0]) == 0).all()


@pytest.mark.parametrize("beams", [1, 63, 64, 65, 2048])
def test_beam_counts(scene, beams):
    rs = np.random.RandomState(beams)
    rng = rs.uniform(0.2, 1.1 * R, beams)
    seeds = seeds_near(scene, [2, 6, 10], seed=beams)
    want = expect(scene, seeds, (1, 1, 2), (0.1, 0.1, 0.03), rng, scene["free"])
    if beams > 2:
        assert 0 < int((rng < R).sum()) < beams
    same(launch(scene, seeds, (1, 1, 2), (0.1, 0.1, 0.03), rng, scene["free"], beams=beams), want, f"{beams} beams")


def test_a_scan_per_seed(scene, main_case):
    seeds, rng, want = main_case
    per = np.full((len(seeds), BEAMS + 3), np.nan)
    per[:, :BEAMS] = rng
    same(launch(scene, seeds, RADII, STEPS, per, scene["free"], beams=BEAMS, ranges_stride=BEAMS + 3), want, "a scan per seed, rows of beams + 3")
    one = expect(scene, seeds, RADII, STEPS, rng[2], scene["free"])
    assert not np.array_equal(one[0], want[0]) and np.array_equal(one[0][2], want[0][2])
    same(launch(scene, seeds, RADII, STEPS, rng[2], scene["free"]), one, "one scan for all seeds")
    padded = np.full((len(seeds), BEAMS + 3), np.nan)
    padded[:, :BEAMS] = rng[2]
    same(launch(scene, seeds, RADII, STEPS, padded, scene["free"], beams=BEAMS, ranges_stride=BEAMS + 3), one, "the same scan in every row")


@pytest.mark.parametrize("pose_stride", [3, 5])
def test_pose_strides_and_poisoned_buffers(scene, main_case, pose_stride):
    seeds, rng, want = main_case
    a = launch(scene, seeds, RADII, STEPS, rng, scene["free"], pose_stride=pose_stride)
    b = launch(scene, seeds, RADII, STEPS, rng, scene["free"], pose_stride=pose_stride)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()       # two calls, the same bytes
    same(a, want, f"pose_stride {pose_stride}")


def test_degenerate_seeds(scene):
    x, y, th = scene["poses"][1]
    rng = scene["scans"][1]
    in_range = int((rng < R).sum())
    seeds = np.array([(np.nan, y, th), (x, np.inf, th), (x, y, np.nan), (x, y, -np.inf), (1e12, y, th), (x, -1e12, th), (-np.inf, np.nan, th),
                      (x, y, np.inf), (x + 0.031, y - 0.017, th)])
    want = expect(scene, seeds, RADII, STEPS, rng, 1000)
    assert (want[0][:8] == [np.uint64(in_range * 1000) << np.uint64(20), in_range * 1000]).all()     # no inside beam anywhere: candidate 0
    assert ryard.cost_of(want[0])[8] != in_range * 1000      # (the last seed is an ordinary one: its beams end in the field)
    same(launch(scene, seeds, RADII, STEPS, rng, 1000), want, "non-finite and far seeds")


def test_degenerate_scans(scene):
    seeds = seeds_near(scene, [1, 6])
    none = np.full(BEAMS, R)
    got = launch(scene, seeds, RADII, STEPS, none, scene["free"])
    assert not got[0].any() and got[1].tobytes() == seeds.tobytes()            # nothing in range: cost 0, candidate 0, the seed's bits
    same(got, expect(scene, seeds, RADII, STEPS, none, scene["free"]), "no beam in range")
    for n in (3, 7):                                           # (fewer beams in range than one trip of the unrolled loop; one trip and three)
        few = none.copy()
        few[5:5 + 2 * n:2] = scene["scans"][1][5:5 + 2 * n:2].clip(0.3, 3.5)
        same(launch(scene, seeds, RADII, STEPS, few, scene["free"]), expect(scene, seeds, RADII, STEPS, few, scene["free"]), f"{n} beams in range")
    rng = scene["scans"][1].copy()
    for b, v in {3: np.nan, 9: np.inf, 14: R, 20: np.nextafter(R, np.inf), 26: 0.0, 31: -0.7, 40: np.nextafter(R, 0), 44: -np.inf,
                 50: -0.0, 55: 1e-300, 57: -3.9}.items():
        rng[b] = v
    want = expect(scene, seeds, RADII, STEPS, rng, scene["free"])
    assert (ryard.cost_of(want[0]) >= scene["free"]).all()    # (-inf is in range and ends nowhere: it pays outside_cost)
    same(launch(scene, seeds, RADII, STEPS, rng, scene["free"]), want, "planted ranges")


def test_seeds_at_the_edges_of_the_field(scene):
    """Seeds within two cells of the right and top edges and their corner, on either side, for a scan of short ranges, and a metre
    or two away for a whole scan (edge_poses of tests/test_gpu_field_slots.py): beams end on both sides of every edge."""
    close, far = tslots.edge_poses(scene["frame"], *scene["field"].shape)
    rs = np.random.RandomState(5)
    short = rs.uniform(0.02, 0.5, BEAMS)
    for seeds, rng, what in ((np.array(close), short, "close"), (np.array(far), scene["scans"][0], "far")):
        inside = np.array([ryard.costs(scene["field"], scene["frame"], scene["lv"].c.cost_scale, UNIT, s, (1, 1, 1), (0.1, 0.1, 0.3), rng, FOV, R, 0)[1]
                           for s in seeds])
        in_range = int((rng < R).sum())
        assert (inside < in_range).any() and (inside > 0).any() and ((inside > 0) & (inside < in_range)).any(), what
        for outside in (0, scene["free"], 2 ** 32 - 1):
            want = expect(scene, seeds, (1, 1, 1), (0.1, 0.1, 0.3), rng, outside)
            same(launch(scene, seeds, (1, 1, 1), (0.1, 0.1, 0.3), rng, outside), want, f"{what}, outside_cost {outside}")


def test_motion(scene, main_case):
    seeds, rng, _ = main_case
    motion = (0.21, -0.04, 0.03)
    want = expect(scene, seeds, RADII, STEPS, rng, scene["free"], motion=motion)
    got = launch(scene, seeds, RADII, STEPS, rng, scene["free"], motion=motion)
    same(got, want, "motion")
    # the same call without a motion on seeds moved by slam2d_mcl_step's move (no noise), the device's cos / sin
    moved = mcl.move(seeds, motion, (0.0, 0.0, 0.0), np.zeros((len(seeds), 3)), *sincos_of(scene)(seeds[:, 2].copy()))
    assert not np.array_equal(moved, seeds)
    again = launch(scene, moved, RADII, STEPS, rng, scene["free"])
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    zero = launch(scene, seeds, RADII, STEPS, rng, scene["free"], motion=(0.0, 0.0, 0.0))
    same(zero, expect(scene, seeds, RADII, STEPS, rng, scene["free"], motion=(0.0, 0.0, 0.0)), "a motion of zero")


def score_poses_words(scene, moved, radii, steps, rng, outside, level=None, p=0):
    """The words from slam2d_score_poses' rows (slots 6, 3 and 4) of the materialised candidates: no host trigonometry."""
    import torch
    eng = scene["eng"]
    words = []
    rng = np.asarray(rng, dtype=np.float64)
    for n, m in enumerate(moved):
        C = ryard.candidates(m, radii, steps).reshape(-1, 3)
        rows = eng.score_poses(scene["lv"] if level is None else level, p, eng.to_device(C), 3, len(C), eng.to_device(rng if rng.ndim == 1 else rng[n]), 0)
        cost = (rows[:, 6].to(torch.int64) + (rows[:, 4] - rows[:, 3]).to(torch.int64) * outside).cpu().numpy().astype(np.uint64)
        words.append(ryard.pack(cost))
    return np.array(words)


def test_agreement_with_score_poses_on_the_device(scene, main_case):
    seeds, rng, want = main_case
    assert np.array_equal(score_poses_words(scene, seeds, RADII, STEPS, rng, scene["free"]), want[0])
    assert np.array_equal(launch(scene, seeds, RADII, STEPS, rng, scene["free"])[0], want[0])


def test_the_largest_accepted_calls(scene):
    """2^20 - 1 candidates of one seed (1025 x 33 x 31: 2^20 itself has no odd factors) and 2^20 seeds of one candidate: too many
    poses for the NumPy yardstick, so against slam2d_score_poses on the same poses, which the main case ties to it."""
    import torch
    eng = scene["eng"]
    rng = scene["scans"][9]
    seed = seeds_near(scene, [9])
    radii, steps = (512, 16, 15), (0.0021, 0.013, 0.004)
    want = score_poses_words(scene, seed, radii, steps, rng, scene["free"])
    words, poses = launch(scene, seed, radii, steps, rng, scene["free"])
    assert np.array_equal(words, want) and ryard.index_of(words)[0] > 1025 * 33
    assert poses.tobytes() == ryard.candidates(seed[0], radii, steps).reshape(-1, 3)[ryard.index_of(words)[0]].tobytes()
    N = 1 << 20
    seeds = ryard.candidates(seed[0], radii, steps).reshape(-1, 3)
    seeds = np.vstack([seeds, seeds[:1]])
    rows = eng.score_poses(scene["lv"], 0, eng.to_device(seeds), 3, N, eng.to_device(rng), 0)
    cost = (rows[:, 6].to(torch.int64) + (rows[:, 4] - rows[:, 3]).to(torch.int64) * scene["free"]).cpu().numpy().astype(np.uint64)
    words, poses = launch(scene, seeds, (0, 0, 0), (0.1, 0.1, 0.1), rng, scene["free"])
    assert np.array_equal(words[:, 0], cost << np.uint64(20)) and np.array_equal(words[:, 1], cost) and poses.tobytes() == seeds.tobytes()


@pytest.fixture(scope="module")
def level_of_three(pkg):
    """The level of three of tests/test_gpu_field_slots.py, built as there: three maps of different content, frames of 289 x 289,
    289 x 288 and 288 x 289 cells."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    dev = torch.device("cuda:0")
    lidar = engine.LidarModel.get(UNIT, R, FOV, BEAMS, WALL)
    lv = engine.SearchLevel(lidar, tslots.P, dev, bnb=False, **tslots.level_kw())
    worlds = [synth.make_world(SIZE, UNIT, seed=s, n_boxes=25) for s in tslots.SEEDS]
    maps = []
    for world, (cx, cy) in zip(worlds, tslots.CENTRES):
        m = engine.MapState.create(SIZE, SIZE, INIT, UNIT, dev)
        m.upload(*synth.counts_from_world(world))
        m.ensure_contains([cx - lv.reach, cx + lv.reach], [cy - lv.reach, cy + lv.reach], UNIT)
        maps.append(m)
    eng = engine.ParticleEngine(lidar, maps, dev)
    eng.field_build(lv, eng.to_device(tslots.CENTRES), 2)
    assert not eng.take_flags(fatal=0xffffffff).any()
    fr = lv.frames()
    assert [(int(f["fh"]), int(f["fw"])) for f in fr] == list(tslots.SIZES)
    return dict(eng=eng, lv=lv, maps=maps, worlds=worlds, frames=fr, free=int(engine.encode_cost(lv.floor_value, lv.cost_scale)))


def test_slot_two_of_a_level_of_three(scene, level_of_three):
    """p_field = 2 and a frame that is not square (288 x 289): the slot's own frame record, image and clipped size."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    b = level_of_three
    lv, p = b["lv"], 2
    field = lv.field_cost(p).copy()
    frame = (float(b["frames"][p]["xlo"]), float(b["frames"][p]["ylo"]))
    assert field.shape == tslots.SIZES[p] == (288, 289)
    walk = np.array(synth.random_walk(b["worlds"][p], UNIT, tslots.ORIGIN, 12, seed=5))
    rng = synth.raycast(b["worlds"][p], UNIT, tslots.ORIGIN, walk[2], FOV, BEAMS, R)
    close, far = tslots.edge_poses(frame, *field.shape)
    seeds = np.vstack([walk[[1, 2, 3]] + (0.031, -0.022, 0.01), np.array(close[:4] + far[:2])])
    sub = dict(eng=b["eng"], lv=lv, field=field, frame=frame)
    want = expect(sub, seeds, RADII, STEPS, rng, b["free"])
    others = [expect(sub, seeds, RADII, STEPS, rng, b["free"], field=lv.field_cost(q).copy(),
                     frame=(float(b["frames"][q]["xlo"]), float(b["frames"][q]["ylo"])))[0] for q in (0, 1)]
    assert all(not np.array_equal(o, want[0]) for o in others) and (ryard.index_of(want[0]) != 0).any()
    same(launch(sub, seeds, RADII, STEPS, rng, b["free"], level=lv.c, p=p), want, "slot 2")
    words = b["eng"].refine_poses(lv, p, b["eng"].to_device(seeds), b["eng"].to_device(np.zeros_like(seeds)), len(seeds), 3, b["eng"].to_device(rng), 0,
                                  RADII, STEPS, b["free"])
    assert np.array_equal(words.cpu().numpy().view(np.uint64), want[0])        # ParticleEngine.refine_poses, the same call
    with pytest.raises(ValueError):
        b["eng"].refine_poses(lv, 3, b["eng"].to_device(seeds), b["eng"].to_device(np.zeros_like(seeds)), len(seeds), 3, b["eng"].to_device(rng), 0,
                              RADII, STEPS, b["free"])


def test_a_distance_field_with_its_own_cost_scale(scene):
    """A level filled by slam2d_field_build_distance from the likelihood table, at a cost scale of the caller's own; the table's last
    entry as the outside cost."""
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    sm, eng = scene["sm"], scene["og"].engine()
    lv = sm.covering_level("fine", tsearch.WINDOW[2], shared=False)
    lut = engine.likelihood_table(UNIT, 0.2)[0]
    own_scale = 3.0 * 2.0 ** 20
    eng.field_build_distance(lv, eng.to_device([[tsearch.WINDOW[0], tsearch.WINDOW[1]]]), 2, (lut, own_scale))
    assert not int(eng.take_flags()[0])
    fr = lv.frames()[0]
    sub = dict(eng=eng, lv=lv, field=lv.field_cost(0).copy(), frame=(float(fr["xlo"]), float(fr["ylo"])))
    outside = int(lut[-1])
    assert lv.c.cost_scale == own_scale != scene["lv"].c.cost_scale and not np.array_equal(sub["field"], scene["field"])
    assert set(np.unique(sub["field"]).tolist()) <= set(lut.tolist())
    seeds = seeds_near(scene, [0, 3, 5, 8, 11])
    rng = scene["scans"][5]
    want = expect(sub, seeds, RADII, STEPS, rng, outside)
    assert (ryard.index_of(want[0]) != 0).any()
    same(launch(sub, seeds, RADII, STEPS, rng, outside, level=lv.c), want, "distance field")
    dec = eng.refine_host(want[0], RADII, STEPS, lv.c.cost_scale)
    assert np.array_equal(dec["score"], -(ryard.cost_of(want[0]).astype(np.float64) / own_scale))


def test_refine_poses_end_to_end(scene):
    """ScanMatcher.refinePoses is the stages chained on the covering level's own field, decoded."""
    matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
    sm = scene["sm"]
    seeds = seeds_near(scene, [4, 5, 6], spread=(0.2, 0.2, 0.04))
    rng = scene["scans"][5]
    res = sm.refinePoses(seeds, {"x": 0, "y": 0, "theta": 0, "range": rng}, window=tsearch.WINDOW)
    lv = sm.last_cover["level"]
    assert set(res) == {"poses", "cost", "score", "start_cost", "offsets"} and sm.last_cover["stages"] == matcher.default_stages(UNIT)
    fr = lv.frames()[0]
    eng = scene["og"].engine()
    free = sm.outside_cost_of(lv)
    words, poses = ryard.refine_stages(lv.field_cost(0), (float(fr["xlo"]), float(fr["ylo"])), lv.c.cost_scale, lv.step, seeds,
                                       matcher.default_stages(UNIT), rng, FOV, R, free, sincos=lambda a: tsearch.device_sincos(eng, a))
    assert res["poses"].tobytes() == poses.tobytes()
    assert np.array_equal(res["cost"], ryard.cost_of(words[:, -1])) and np.array_equal(res["start_cost"], words[:, 0, 1])
    assert np.array_equal(res["score"], -(ryard.cost_of(words[:, -1]).astype(np.float64) / lv.c.cost_scale))
    for i, (radii, steps) in enumerate(matcher.default_stages(UNIT)):
        assert np.array_equal(res["offsets"][:, i], eng.refine_host(words[:, i], radii, steps, lv.c.cost_scale)["offsets"])
    assert (res["offsets"] != 0).any() and (res["cost"] <= res["start_cost"]).all()
    # a scan per seed, and stages of the caller's own
    per = sm.refinePoses(seeds, scene["scans"][[4, 5, 6]], stages=[(RADII, STEPS)], window=tsearch.WINDOW)
    w1, p1 = ryard.refine(lv.field_cost(0), (float(fr["xlo"]), float(fr["ylo"])), lv.c.cost_scale, lv.step, seeds, RADII, STEPS,
                          scene["scans"][[4, 5, 6]], FOV, R, free, sincos=lambda a: tsearch.device_sincos(eng, a))
    assert per["poses"].tobytes() == p1.tobytes() and np.array_equal(per["cost"], ryard.cost_of(w1)) and per["offsets"].shape == (3, 1, 3)
    with pytest.raises(ValueError):
        sm.refinePoses(seeds, rng[:5])


def test_the_tracker_scan_by_scan_and_as_a_log(pkg, scene):
    """Tracker.step over the walk against the yardstick started from the device's previous pose; Tracker.run over the same log
    gives the same bytes as the steps."""
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    sm, poses, scans = scene["sm"], scene["poses"], scene["scans"]
    odo = poses + np.arange(len(poses)).reshape(-1, 1) * (0.02, -0.015, 0.01)          # a raw odometry that drifts
    readings = [dict(x=float(o[0]), y=float(o[1]), theta=float(o[2]), range=scans[k]) for k, o in enumerate(odo)]
    tr = pkg.Tracker(sm, tsearch.WINDOW)
    lv, eng = tr.level, tr.eng
    fr = lv.frames()[0]
    field, frame = lv.field_cost(0).copy(), (float(fr["xlo"]), float(fr["ylo"]))
    sincos = lambda a: tsearch.device_sincos(eng, a)
    assert tr.set_pose(poses[0]).tobytes() == poses[0].tobytes() and tr.pose() == tuple(poses[0])
    reports = []
    for k in range(len(poses)):
        prev = np.array(tr.pose())
        motion = localise.odometry_motion(readings[k - 1], readings[k]) if k else None
        rep = tr.step(readings[k], motion)
        words, want = ryard.refine_stages(field, frame, lv.c.cost_scale, lv.step, prev, tr.stages, scans[k], FOV, R, tr.outside_cost, motion, sincos)
        assert np.array(rep.pose).tobytes() == want[0].tobytes() == np.array(tr.pose()).tobytes(), k
        assert (rep.cost, rep.start_cost) == (int(ryard.cost_of(words[:, -1])[0]), int(words[0, 0, 1])), k
        for i, (radii, steps) in enumerate(tr.stages):
            assert np.array_equal(rep.offsets[i], eng.refine_host(words[:, i], radii, steps, lv.c.cost_scale)["offsets"][0]), (k, i)
        reports.append(rep)
    assert any(r.offsets.any() for r in reports)
    again = pkg.Tracker(sm, tsearch.WINDOW)
    again.set_pose(poses[0])
    log = again.run(readings)
    assert len(log) == len(reports)
    for a, b in zip(log, reports):
        assert np.array(a.pose).tobytes() == np.array(b.pose).tobytes() and (a.cost, a.start_cost) == (b.cost, b.start_cost)
        assert np.array_equal(a.offsets, b.offsets)
    assert again.pose() == tr.pose()
