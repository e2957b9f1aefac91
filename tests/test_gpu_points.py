"""slam2d_search_points and slam2d_refine_points on the MI355X against the definition in NumPy (tests/points_yardstick.py): every
comparison is np.array_equal on the 64-bit words and on the bits of the poses.  The yardstick reads the DEVICE's field and the
device's cos / sin of the headings (slam2d_device_sincos); the result is a minimum of integer sums and a few rounded operations:
there is no tolerance.  The field is hand-made -- about 40 x 40 cells of random costs in slot 0 and slot 2 of a level of three,
each with a frame of its own -- and the points lie on both sides of all four of its edges; outside_cost is never 0 unless a
test says so.  Every call is made at the C ABI with poisoned buffers of its own unless a test says otherwise."""
import ctypes
import importlib

import numpy as np
import pytest

import lattice_yardstick as lyard
import points_yardstick as pyard
import refine_yardstick as ryard
import score_yardstick as yard
import test_gpu_search as tsearch
from test_gpu_search import device_sincos, pkg, scene  # noqa: F401  (scene: the 289 x 289 field, for the Tracker alone)
from test_score_host import BEAMS, FOV, R, UNIT

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
points = importlib.import_module("slam-2d-lidar-scan_amd.points")

STEP = 0.1
LIDAR = (STEP, 1.5, np.pi, 60, 0.5)                            # unit, max range, fov, beams, wall: the scan form's, for the cross-checks
SHAPES = {0: (40, 40), 2: (37, 41)}                            # (fh, fw) of the two slots that hold a field
FRAMES = {0: (-2.0, -1.5), 2: (-1.7, -2.1)}                    # (xlo, ylo)
OUTSIDE = 77777
MS = [1, 63, 64, 65, 255, 256, 257, 1024, 1025, 2048]          # the compaction's wave and block boundaries, REFINE_TABLE / M = 2 and 1
TABLE, BLOCKS, CHUNK = _lib.REFINE_TABLE, _lib.REFINE_BLOCKS, _lib.SEARCH_CHUNK
assert (TABLE, BLOCKS, CHUNK) == (2048, 1024, 8)
BAD = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, np.inf), (-np.inf, 0.5), (0.5, -np.inf)]


@pytest.fixture(scope="module")
def ctx(pkg):
    """A level of three with hand-made fields in slots 0 and 2 (SearchLevel.set_field, the frame records written beside them);
    slot 1 keeps a field of one cost that none of the tests may see."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    dev = torch.device("cuda:0")
    lidar = engine.LidarModel.get(*LIDAR)
    lv = engine.SearchLevel(lidar, 3, dev, bnb=False, step=STEP, sigma=1.0, miss_prob=0.15 ** 2, search_radius_ctor=0.35, radius=STEP,
                            half_rad=0.0, fine=True, move_sigma=0.1, max_move_dev=0.25, turn_sigma=0.3)
    assert lv.fmax == 42
    maps = [engine.MapState.create(4, 4, {"x": 0.0, "y": 0.0}, STEP, dev) for _ in range(3)]
    eng = engine.ParticleEngine(lidar, maps, dev)
    fr = lv.frames()
    rs = np.random.RandomState(7)
    for p in range(3):
        fh, fw = SHAPES.get(p, (42, 42))
        prob = -rs.uniform(0.0, 6.0, (fh, fw)) if p in SHAPES else np.full((fh, fw), -3.0)
        prob[0, 0] = -6.0                                      # the same minimum, so the same cost scale, in every slot
        lv.set_field(prob, p)
        xlo, ylo = FRAMES.get(p, (-2.1, -2.1))
        fr[p]["xlo"], fr[p]["ylo"], fr[p]["xhi"], fr[p]["yhi"] = xlo, ylo, xlo + fw * STEP, ylo + fh * STEP
        fr[p]["fh"], fr[p]["fw"] = fh, fw
    lv.t["frames"].copy_(torch.from_numpy(fr.view(np.uint8).reshape(3, -1)))
    fields = {p: lv.field_cost(p).copy() for p in SHAPES}
    assert all(fields[p].shape == SHAPES[p] and len(np.unique(fields[p])) > 1000 for p in SHAPES)
    return dict(eng=eng, lv=lv, fields=fields, maps=maps)


# ---- inputs ----
def cloud(M, seed, invalid=()):
    """M points over [-2.6, 2.6]^2 -- from a pose near the middle of either frame they end in the field and beyond each of its
    four edges --, the rows ``invalid`` taken by the non-finite pairs of BAD in turn."""
    rs = np.random.RandomState(seed)
    q = rs.uniform(-2.6, 2.6, (M, 2))
    for i, k in enumerate(invalid):
        q[k] = BAD[i % len(BAD)]
    return q


def lattice(nx, ny, nth, p=0, dth=0.37, dx=0.013, dy=0.017):
    """A lattice about the middle of slot p's frame, off the cells."""
    xlo, ylo = FRAMES[p]
    fh, fw = SHAPES[p]
    return (nx, ny, nth, xlo + 0.5 * fw * STEP - (nx // 2) * dx + 0.0031, dx, ylo + 0.5 * fh * STEP - (ny // 2) * dy - 0.0017, dy, -0.9, dth)


def seeds_in(p, n, seed):
    xlo, ylo = FRAMES[p]
    fh, fw = SHAPES[p]
    rs = np.random.RandomState(seed)
    return np.array([xlo + 0.5 * fw * STEP, ylo + 0.5 * fh * STEP, 0.0]) + rs.uniform(-1, 1, (n, 3)) * (0.6, 0.6, 3.0)


# ---- the yardstick with the device's cos / sin ----
def expect_search(ctx, p, lat, pts, outside=OUTSIDE):
    c, s = device_sincos(ctx["eng"], lyard.axes(lat)[2])
    return pyard.search_points(ctx["fields"][p], FRAMES[p], STEP, lat, pts, outside, c, s)


def expect_refine(ctx, p, seeds, radii, steps, pts, outside=OUTSIDE, motion=None):
    """(words [N, 2], poses [N, 3]); equal seeds (with one set) are computed once."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    pts = np.asarray(pts, dtype=np.float64)
    if pts.ndim == 2:
        uniq, inverse = np.unique(seeds.view(np.uint64), axis=0, return_inverse=True)
        seeds_u = uniq.view(np.float64)
    else:
        seeds_u, inverse = seeds, np.arange(len(seeds))
    words, poses = pyard.refine_points(ctx["fields"][p], FRAMES[p], STEP, seeds_u, radii, steps, pts, outside, motion,
                                       lambda a: device_sincos(ctx["eng"], a))
    return words[inverse.reshape(-1)], poses[inverse.reshape(-1)]


# ---- the calls at the C ABI, every buffer of its own and poisoned with 0xff bytes ----
def rows_of(pts, point_stride):
    """The points in rows of ``point_stride`` doubles, the other slots NaN."""
    pts = np.asarray(pts, dtype=np.float64)
    rows = np.full(pts.shape[:-1] + (point_stride,), np.nan)
    rows[..., :2] = pts
    return rows


def launch_search(ctx, p, lat, pts, outside=OUTSIDE, point_stride=2, level=None):
    """The image as uint64 [ny, nx]; ``level``: the Slam2dLevel whose slot p is read (default: the context's level)."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = ctx["eng"]
    lvc = ctx["lv"].c if level is None else level
    nx, ny, nth = lat[:3]
    M = len(pts)
    n = eng.L.slam2d_search_points_work(M, nx, ny, nth)
    assert n == 2 * nth * M
    d_pts = eng.to_device(rows_of(pts, point_stride))
    work = torch.full((n,), -1, dtype=torch.int64, device=eng.device)         # (0xff bytes: NaNs as doubles)
    out = torch.full((ny, nx), -1, dtype=torch.int64, device=eng.device)
    _lib.check(eng.L.slam2d_search_points(ctypes.byref(lvc), p, nx, ny, nth, *[float(v) for v in lat[3:]], d_pts.data_ptr(), point_stride, M,
                                          int(outside), work.data_ptr(), out.data_ptr(), engine._stream()), "slam2d_search_points")
    return out.cpu().numpy().view(np.uint64)


def launch_refine(ctx, p, seeds, radii, steps, pts, outside=OUTSIDE, motion=None, pose_stride=3, point_stride=2, pad=0, level=None):
    """(words uint64 [N, 2], the output pose buffer float64 [N, pose_stride]); ``pts`` [M, 2]: set_stride 0; [N, M, 2]: a set per
    seed, ``pad`` doubles between the sets; ``level``: the Slam2dLevel whose slot p is read (default: the context's level)."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = ctx["eng"]
    lvc = ctx["lv"].c if level is None else level
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 3)
    pts = np.asarray(pts, dtype=np.float64)
    N, M = len(seeds), pts.shape[-2]
    rows = rows_of(pts, point_stride)
    set_stride = 0
    if pts.ndim == 3:
        set_stride = M * point_stride + pad
        rows = np.concatenate([rows.reshape(N, -1), np.full((N, pad), np.nan)], axis=1)
    poses = np.full((N, pose_stride), np.nan)
    poses[:, :3] = seeds
    d_in, d_pts = eng.to_device(poses), eng.to_device(rows)
    full = lambda n: torch.full((n,), -1, dtype=torch.int64, device=eng.device)
    work, out, d_out = full(eng.L.slam2d_refine_work(N)), full(2 * N), full(N * pose_stride)
    _lib.check(eng.L.slam2d_refine_points(ctypes.byref(lvc), p, N, d_in.data_ptr(), d_out.data_ptr(), pose_stride, d_pts.data_ptr(), point_stride,
                                          M, set_stride, None if motion is None else (ctypes.c_double * 3)(*motion), *[int(r) for r in radii],
                                          *[float(s) for s in steps], int(outside), work.data_ptr(), out.data_ptr(), engine._stream()),
               "slam2d_refine_points")
    return out.cpu().numpy().view(np.uint64).reshape(N, 2), d_out.cpu().numpy().view(np.float64).reshape(N, pose_stride)


def same_image(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, what
    bad = got != want
    assert np.array_equal(got, want), (what, np.argwhere(bad)[:6].tolist(), [hex(v) for v in got[bad][:6]], [hex(v) for v in want[bad][:6]])


def same_refine(got, want, what=""):
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


def chunk(N, nth, M):
    """Headings per block row of the refinement's search launch, as include/slam2d.h states it."""
    return min(max(1, TABLE // M), -(-nth // -(-BLOCKS // N)))


# ---- the main case, on the yardstick first ----
def test_main_case(ctx):
    for p in (0, 2):
        lat = lattice(9, 7, 5, p)
        pts = cloud(100, 3 + p, invalid=(7, 40))
        want = expect_search(ctx, p, lat, pts)
        P = lyard.poses(lat)
        c, s = device_sincos(ctx["eng"], lyard.axes(lat)[2])
        rep = lambda t: np.broadcast_to(t.reshape(-1, 1, 1), P.shape[:3])
        cost, n_in, n_valid = pyard.costs(ctx["fields"][p], FRAMES[p], STEP, P, pts, OUTSIDE, rep(c), rep(s))
        assert n_valid == 98 and 10 < n_in.min() and n_in.max() < 90       # points inside and outside at every pose
        # ... and beyond each of the four edges, at the middle pose and heading
        ex, ey = pyard.offsets(pts, c[2], s[2])
        px, py = P[2, 3, 4, 0] + ex, P[2, 3, 4, 1] + ey
        fh, fw = SHAPES[p]
        assert (px < FRAMES[p][0]).any() and (px > FRAMES[p][0] + fw * STEP).any() and (py < FRAMES[p][1]).any() and (py > FRAMES[p][1] + fh * STEP).any()
        assert len(np.unique(want & np.uint64(0xffff))) >= 3
        same_image(launch_search(ctx, p, lat, pts), want, f"slot {p}")
        other = pyard.search_points(ctx["fields"][2 - p], FRAMES[2 - p], STEP, lat, pts, OUTSIDE, c, s)
        assert not np.array_equal(other, want)                 # (the other slot's field and frame give another image)
        seeds = seeds_in(p, 5, 11 + p)
        radii, steps = (3, 2, 2), (0.07, 0.05, 0.11)
        want = expect_refine(ctx, p, seeds, radii, steps, pts)
        assert len(np.unique(ryard.index_of(want[0]))) >= 3
        same_refine(launch_refine(ctx, p, seeds, radii, steps, pts), want, f"slot {p}")


def test_through_the_engine(ctx):
    """ParticleEngine.search_points / refine_points are the same calls; slots beyond the level are refused."""
    eng, lv = ctx["eng"], ctx["lv"]
    p, lat, pts = 2, lattice(9, 7, 5, 2), cloud(100, 5, invalid=(7, 40))
    words = eng.search_points(lv, p, lat, eng.to_device(pts), len(pts), OUTSIDE)
    same_image(words.cpu().numpy().view(np.uint64), expect_search(ctx, p, lat, pts), "search_points")
    dec = eng.search_host(words, lat, lv.c.cost_scale)
    assert np.array_equal(dec["cost"], expect_search(ctx, p, lat, pts) >> np.uint64(16))
    seeds, radii, steps = seeds_in(p, 4, 2), (2, 2, 1), (0.07, 0.05, 0.11)
    d_out = eng.to_device(np.zeros_like(seeds))
    words = eng.refine_points(lv, p, eng.to_device(seeds), d_out, len(seeds), 3, eng.to_device(pts), len(pts), 0, radii, steps, OUTSIDE)
    want = expect_refine(ctx, p, seeds, radii, steps, pts)
    assert np.array_equal(words.cpu().numpy().view(np.uint64), want[0]) and d_out.cpu().numpy().tobytes() == want[1].tobytes()
    with pytest.raises(ValueError):
        eng.search_points(lv, 3, lat, eng.to_device(pts), len(pts), OUTSIDE)
    with pytest.raises(ValueError):
        eng.refine_points(lv, 3, eng.to_device(seeds), d_out, len(seeds), 3, eng.to_device(pts), len(pts), 0, radii, steps, OUTSIDE)
    with pytest.raises(ValueError):
        eng.search_points(lv, 0, lat, eng.to_device(pts), len(pts) + 1, OUTSIDE)       # more points than the buffer holds


# ---- the point counts: the compaction's wave and block boundaries, the table's headings per block ----
@pytest.mark.parametrize("M", MS)
def test_point_counts(ctx, M):
    """Invalid points in slot 0, in the last slot and on each side of every wave boundary the set reaches.  The refinement runs
    512 seeds (four different ones) of three headings: two block rows per seed, two headings in the first -- but from 1025 points
    on a block's table holds one heading only."""
    invalid = sorted({k for k in (0, 63, 64, 127, 128, 255, 256, 1023, 1024, M - 1) if 0 <= k < M}) if M > 1 else ()
    pts = cloud(M, M, invalid)
    p = 0 if M % 2 else 2
    lat = lattice(5, 3, 3, p)
    if M > 1:
        assert 0 < int(pyard.valid(pts).sum()) < M
        same_image(launch_search(ctx, p, lat, pts), expect_search(ctx, p, lat, pts), f"{M} points")
    full = cloud(M, M + 1)
    same_image(launch_search(ctx, p, lat, full, point_stride=3), expect_search(ctx, p, lat, full), f"{M} points, all valid, rows of 3")
    assert chunk(512, 3, M) == (2 if M <= 1024 else 1)
    seeds = np.tile(seeds_in(p, 4, M), (128, 1))
    radii, steps = (1, 1, 1), (0.09, 0.07, 0.4)
    for q, what in ((pts, "planted"), (full, "all valid")):
        want = expect_refine(ctx, p, seeds, radii, steps, q)
        same_refine(launch_refine(ctx, p, seeds, radii, steps, q), want, f"{M} points, {what}")


@pytest.mark.parametrize("M, n_valid", [(67, 64), (67, 65), (67, 66), (67, 67), (9, 0), (9, 1), (9, 2), (9, 3), (300, 5), (2048, 2047)])
def test_valid_counts_and_the_unrolled_loop(ctx, M, n_valid):
    """4 k, 4 k + 1, 4 k + 2 and 4 k + 3 valid points (SEARCH_UNROLL's remainder), fewer than one trip, none at all."""
    rs = np.random.RandomState(M + n_valid)
    invalid = rs.permutation(M)[:M - n_valid]
    pts = cloud(M, n_valid, invalid)
    assert int(pyard.valid(pts).sum()) == n_valid
    lat = lattice(5, 3, 3)
    want = expect_search(ctx, 0, lat, pts)
    same_image(launch_search(ctx, 0, lat, pts), want, f"{n_valid} of {M}")
    seeds = seeds_in(0, 3, M)
    wr = expect_refine(ctx, 0, seeds, (1, 1, 1), (0.09, 0.07, 0.4), pts)
    got = launch_refine(ctx, 0, seeds, (1, 1, 1), (0.09, 0.07, 0.4), pts)
    same_refine(got, wr, f"{n_valid} of {M}")
    if n_valid == 0:                                           # nothing valid: cost 0, heading 0, candidate 0, the seed's bits
        assert not want.any() and not got[0].any() and got[1].tobytes() == seeds.tobytes()


def test_invalid_points_everywhere_and_of_every_kind(ctx):
    """Each non-finite pair alone among valid points, on either side of the wave boundary; the six of them in a row."""
    lat = lattice(5, 3, 3)
    base = cloud(130, 1)
    for k in (62, 63, 64, 65):
        for bad in BAD:
            pts = base.copy()
            pts[k] = bad
            same_image(launch_search(ctx, 0, lat, pts), expect_search(ctx, 0, lat, np.delete(base, k, axis=0)), f"{bad} in slot {k}")
    pts = base.copy()
    pts[60:66] = BAD
    same_image(launch_search(ctx, 0, lat, pts), expect_search(ctx, 0, lat, pts), "six in a row")
    # valid points that end nowhere: far away, and so large that the rotation overflows
    far = np.vstack([base[:20], [[4e3, 1.0], [1e300, -1e300], [1.5e308, 1.5e308], [-1.7e308, 1.0]]])
    want = expect_search(ctx, 0, lat, far)
    assert ((want >> np.uint64(16)) >= 4 * OUTSIDE).all()
    same_image(launch_search(ctx, 0, lat, far), want, "far and huge points")
    seeds = seeds_in(0, 3, 9)
    same_refine(launch_refine(ctx, 0, seeds, (1, 1, 1), (0.09, 0.07, 0.4), far), expect_refine(ctx, 0, seeds, (1, 1, 1), (0.09, 0.07, 0.4), far), "far")


# ---- the search's launch shapes ----
@pytest.mark.parametrize("nx, ny", [(1, 1), (255, 1), (16, 16), (257, 1), (1, 257), (51, 5)])
def test_positions_around_the_block_size(ctx, nx, ny):
    pts = cloud(37, nx + ny, invalid=(0, 36))
    for nth in (1, 2):
        lat = lattice(nx, ny, nth, 0, dth=2.9)
        same_image(launch_search(ctx, 0, lat, pts), expect_search(ctx, 0, lat, pts), f"{nx} x {ny} x {nth}")


@pytest.mark.parametrize("nth", [1, CHUNK - 1, CHUNK, CHUNK + 1, 40])
def test_heading_rows(ctx, nth):
    """Few positions: a block row per SEARCH_CHUNK headings -- one row up to 8 headings, two for 9, five for 40."""
    pts = cloud(37, nth, invalid=(5,))
    lat = lattice(11, 9, nth, 2, dth=2 * np.pi / nth, dx=0.11, dy=0.13)
    want = expect_search(ctx, 2, lat, pts)
    if nth > CHUNK:
        h = (want & np.uint64(0xffff)).astype(int)
        assert (h >= CHUNK).any() and (h < CHUNK).any()        # winners in more than one row
    a = launch_search(ctx, 2, lat, pts)
    b = launch_search(ctx, 2, lat, pts)
    assert a.tobytes() == b.tobytes()                          # two calls, garbage in d_out and d_work in front of each: the same bits
    same_image(a, want, f"{nth} headings")


def test_outside_costs_and_degenerate_lattices(ctx):
    pts = cloud(50, 4, invalid=(3,))
    lat = lattice(7, 5, 3)
    for outside in (0, 1, 2 ** 32 - 1):
        same_image(launch_search(ctx, 0, lat, pts, outside), expect_search(ctx, 0, lat, pts, outside), f"outside_cost {outside}")
    for bad in ((np.nan, lat[5], lat[7]), (lat[3], np.inf, lat[7]), (lat[3], lat[5], np.nan), (1e12, lat[5], lat[7]), (lat[3], lat[5], -np.inf)):
        l2 = lat[:3] + (bad[0], lat[4], bad[1], lat[6], bad[2], lat[8])
        want = expect_search(ctx, 0, l2, pts)
        assert (want == np.uint64((49 * OUTSIDE) << 16)).all()  # no point inside: every valid one pays, heading 0
        same_image(launch_search(ctx, 0, l2, pts), want, f"lattice from {bad}")
    for steps in ((0.0, 0.0, 0.0), (-0.013, -0.017, -0.37)):
        l2 = lat[:4] + (steps[0], lat[5], steps[1], lat[7], steps[2])
        same_image(launch_search(ctx, 0, l2, pts), expect_search(ctx, 0, l2, pts), f"steps {steps}")


# ---- the refinement's launch shapes ----
@pytest.mark.parametrize("N", [1, 3, 1025])
def test_seed_counts(ctx, N):
    """3 x 3 x 3 candidates and 8 points: one seed has a block per heading, 1025 seeds have one block each with all three."""
    assert chunk(N, 3, 8) == (1 if N < 1025 else 3)
    pts = cloud(8, N, invalid=(2,))
    seeds = np.tile(seeds_in(0, 7, N), (N // 7 + 1, 1))[:N]
    radii, steps = (1, 1, 1), (0.09, 0.07, 0.4)
    want = expect_refine(ctx, 0, seeds, radii, steps, pts)
    same_refine(launch_refine(ctx, 0, seeds, radii, steps, pts), want, f"{N} seeds")
    # a set per seed, of another valid count each (0 .. 8), sets 16 + 5 doubles apart
    per = np.stack([cloud(8, 100 + n % 9, invalid=tuple(range(n % 9))) for n in range(N)])
    assert sorted({int(pyard.valid(s).sum()) for s in per}) == list(range(max(0, 9 - N), 9))
    want = expect_refine(ctx, 0, seeds, radii, steps, per)
    got = launch_refine(ctx, 0, seeds, radii, steps, per, pad=5)
    same_refine(got, want, f"{N} seeds, a set each")
    if N > 1:
        assert not np.array_equal(want[0], expect_refine(ctx, 0, seeds, radii, steps, per[0])[0])


def test_many_headings_of_few_points(ctx):
    """301 headings of 3 points in one block: the headings' cos / sin in three passes of 128."""
    assert chunk(1024, 301, 3) == 301
    pts = cloud(3, 8)
    seeds = np.tile(seeds_in(2, 8, 3), (128, 1))
    radii, steps = (0, 0, 150), (0.1, 0.1, 0.02)
    want = expect_refine(ctx, 2, seeds, radii, steps, pts)
    jt = ryard.index_of(want[0])
    assert (jt >= 128).any() and len(np.unique(jt)) > 1
    same_refine(launch_refine(ctx, 2, seeds, radii, steps, pts), want, "301 headings")


def test_two_stages_with_a_motion_and_poisoned_strides(ctx):
    """The first stage moves the seeds, the second starts from the first one's poses (the ping-pong of the callers); pose rows
    of five doubles and point rows of three."""
    pts = cloud(90, 6, invalid=(0, 89))
    seeds = seeds_in(2, 6, 4)
    stages = (((2, 2, 2), (0.1, 0.1, 0.2)), ((2, 2, 2), (0.05, 0.05, 0.05)))
    motion = (0.21, -0.04, 0.3)
    sincos = lambda a: device_sincos(ctx["eng"], a)
    want_words, want_poses = pyard.refine_stages(ctx["fields"][2], FRAMES[2], STEP, seeds, stages, pts, OUTSIDE, motion, sincos)
    first = launch_refine(ctx, 2, seeds, *stages[0], pts, motion=motion, pose_stride=5, point_stride=3)
    same_refine(first, expect_refine(ctx, 2, seeds, *stages[0], pts, motion=motion), "first stage")
    assert not np.array_equal(first[0], expect_refine(ctx, 2, seeds, *stages[0], pts)[0])      # (the motion matters)
    second = launch_refine(ctx, 2, first[1][:, :3], *stages[1], pts, pose_stride=5, point_stride=3)
    assert np.array_equal(first[0], want_words[:, 0]) and np.array_equal(second[0], want_words[:, 1])
    assert second[1][:, :3].tobytes() == want_poses.tobytes()
    again = launch_refine(ctx, 2, seeds, *stages[0], pts, motion=motion, pose_stride=5, point_stride=3)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()       # two calls, the same bytes


def test_degenerate_seeds(ctx):
    pts = cloud(40, 2, invalid=(11,))
    x, y, th = seeds_in(0, 1, 1)[0]
    seeds = np.array([(np.nan, y, th), (x, np.inf, th), (x, y, np.nan), (x, y, -np.inf), (1e12, y, th), (x, -1e12, th), (-np.inf, np.nan, th),
                      (x, y, np.inf), (x, y, th)])
    radii, steps = (2, 1, 2), (0.07, 0.05, 0.11)
    want = expect_refine(ctx, 0, seeds, radii, steps, pts)
    assert (want[0][:8] == [np.uint64(39 * OUTSIDE) << np.uint64(20), 39 * OUTSIDE]).all()       # no point inside anywhere: f = 0
    assert ryard.cost_of(want[0])[8] != 39 * OUTSIDE
    same_refine(launch_refine(ctx, 0, seeds, radii, steps, pts), want, "non-finite and far seeds")
    for steps in ((0.0, 0.0, 0.0), (-0.07, -0.05, -0.11)):
        same_refine(launch_refine(ctx, 0, seeds[8:], radii, steps, pts), expect_refine(ctx, 0, seeds[8:], radii, steps, pts), f"steps {steps}")
    assert (ryard.index_of(expect_refine(ctx, 0, seeds[8:], radii, (0.0, 0.0, 0.0), pts)[0]) == 0).all()


# ---- cross-checks ----
def test_the_search_and_the_refinement_agree_on_a_dyadic_lattice(ctx):
    """x0, y0, th0 and the seed multiples of 2^-6, steps of 2^-3 m and 2^-6 rad: a candidate's coordinates have the same bits by
    x0 + ix * dx and by seed + off(j) * dx, so the refinement's winning cost is the minimum of the search image over the same
    candidates, and its winner is a pose where the image attains it."""
    pts = cloud(120, 12, invalid=(64,))
    dx, dth = 2.0 ** -3, 2.0 ** -6
    for p, (x0, y0, th0) in ((0, (-0.5, -0.25, 0.25)), (2, (-0.375, -0.75, -1.0 + 3 * 2.0 ** -6))):
        lat = (5, 7, 9, x0, dx, y0, dx, th0, dth)
        img = launch_search(ctx, p, lat, pts)
        same_image(img, expect_search(ctx, p, lat, pts), "dyadic lattice")
        seed = np.array([[x0 + 2 * dx, y0 + 3 * dx, th0 + 4 * dth]])
        words, poses = launch_refine(ctx, p, seed, (2, 3, 4), (dx, dx, dth), pts)
        same_refine((words, poses), expect_refine(ctx, p, seed, (2, 3, 4), (dx, dx, dth), pts), "dyadic seed")
        cost = img >> np.uint64(16)
        assert ryard.cost_of(words)[0] == cost.min()
        ix, iy, it = (poses[0, :3] - (x0, y0, th0)) / (dx, dx, dth)
        assert (ix, iy, it) == (int(ix), int(iy), int(it)) and cost[int(iy), int(ix)] == cost.min()
        assert (img[int(iy), int(ix)] & np.uint64(0xffff)) <= int(it)          # (the image keeps the LOWEST heading among equals)


def scan_form(ctx, ranges):
    """The lidar descriptor of the scan forms for this many beams, the ranges on the device, and the scan as points with the
    device's cos / sin of the beam angles at heading 0."""
    eng = ctx["eng"]
    lid = _lib.Slam2dLidar.from_buffer_copy(eng.lidar_c)
    lid.beams = len(ranges)
    pts = points.scan_points(ranges, LIDAR[2], LIDAR[1], sincos=lambda a: device_sincos(eng, a))
    return lid, eng.to_device(ranges), pts


@pytest.mark.parametrize("beams", [60, 257])
def test_against_the_scan_forms_at_heading_zero(ctx, beams):
    """One heading, th0 = 0: slam2d_search_points of scan_points(ranges) writes slam2d_search_lattice's words; rt = 0 and seeds of
    heading 0: slam2d_refine_points' words and poses are slam2d_refine_poses'."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng, lv = ctx["eng"], ctx["lv"]
    rs = np.random.RandomState(beams)
    rng = rs.uniform(0.05, 1.3 * LIDAR[1], beams)              # about a quarter out of range; the longest end beyond the field
    rng[[4, 17]] = np.nan, np.inf
    lid, d_rng, pts = scan_form(ctx, rng)
    assert np.array_equal(pyard.valid(pts), rng < LIDAR[1]) and 0 < int(pyard.valid(pts).sum()) < beams
    sc, ss = device_sincos(eng, np.zeros(1))
    assert (sc[0], ss[0]) == (1.0, 0.0)
    for p in (0, 2):
        lat = lattice(21, 13, 1, p)
        lat = lat[:7] + (0.0, 0.3)
        n = eng.L.slam2d_search_lattice_work(ctypes.byref(lid), 21, 13, 1)
        work = torch.full((n,), -1, dtype=torch.int64, device=eng.device)
        out = torch.full((13, 21), -1, dtype=torch.int64, device=eng.device)
        _lib.check(eng.L.slam2d_search_lattice(ctypes.byref(lid), ctypes.byref(lv.c), p, 21, 13, 1, *[float(v) for v in lat[3:]], d_rng.data_ptr(),
                                               OUTSIDE, work.data_ptr(), out.data_ptr(), engine._stream()), "slam2d_search_lattice")
        scan_words = out.cpu().numpy().view(np.uint64)
        assert len(np.unique(scan_words)) > 100
        same_image(launch_search(ctx, p, lat, pts), scan_words, f"slot {p}: the scan form's words")
        seeds = seeds_in(p, 6, beams)
        seeds[:, 2] = 0.0
        radii, steps = (4, 3, 0), (0.05, 0.07, 0.02)
        d_in, d_out = eng.to_device(seeds), torch.full((6, 3), -1.0, dtype=torch.float64, device=eng.device)
        words = torch.full((6, 2), -1, dtype=torch.int64, device=eng.device)
        rwork = torch.full((18,), -1, dtype=torch.int64, device=eng.device)
        _lib.check(eng.L.slam2d_refine_poses(ctypes.byref(lid), ctypes.byref(lv.c), p, 6, d_in.data_ptr(), d_out.data_ptr(), 3, d_rng.data_ptr(), 0,
                                             None, *radii, *steps, OUTSIDE, rwork.data_ptr(), words.data_ptr(), engine._stream()),
                   "slam2d_refine_poses")
        want = words.cpu().numpy().view(np.uint64), d_out.cpu().numpy()
        assert (ryard.index_of(want[0]) != 0).any()
        same_refine(launch_refine(ctx, p, seeds, radii, steps, pts), want, f"slot {p}: the scan form's words and poses")


def test_the_tracker_takes_points(pkg, scene):
    """Tracker.step_points with scan_points of a scan returns the bits of Tracker.step where the two definitions coincide: a pose
    of heading 0 and stages without headings of their own (rt = 0; at any other heading the scan form takes the cosine of the
    beam's angle and the point form rotates the point: two roundings apart)."""
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    sm, poses, scans = scene["sm"], scene["poses"], scene["scans"]
    stages = (((4, 4, 0), (UNIT, UNIT, 0.02)), ((2, 2, 0), (UNIT / 2, UNIT / 2, 0.005)))
    a, b = pkg.Tracker(sm, tsearch.WINDOW, stages=stages), pkg.Tracker(sm, tsearch.WINDOW, stages=stages)
    eng = a.eng
    moved = 0
    for k, motion in ((2, None), (5, (0.13, -0.06, 0.0)), (8, (0.0, 0.0, 0.0))):
        rng = scans[k]
        start = (poses[k][0] + 0.17, poses[k][1] - 0.12, 0.0)  # (not the heading the scan was taken at: any scan will do for equal bits)
        pts = points.scan_points(rng, FOV, R, sincos=lambda t: device_sincos(eng, t))
        a.set_pose(start)
        b.set_pose(start)
        ra, rb = a.step(rng, motion), b.step_points(pts, motion)
        assert isinstance(rb, localise.TrackReport)
        assert np.array(ra.pose).tobytes() == np.array(rb.pose).tobytes() and (ra.cost, ra.start_cost) == (rb.cost, rb.start_cost), k
        assert np.array_equal(ra.offsets, rb.offsets) and a.pose() == b.pose()
        moved += int(ra.offsets.any())
    assert moved
    with pytest.raises(ValueError):
        b.step_points(np.zeros((3, 3)), None)


def test_search_points_and_refine_points_end_to_end(pkg, scene):
    """ScanMatcher.searchPoints / refinePoints on the covering level's own field: the yardstick's words, decoded as searchPoses
    and refinePoses decode theirs; points within lidarMaxRange share the scan forms' cached level."""
    matcher = importlib.import_module("slam-2d-lidar-scan_amd.matcher")
    sm, poses, scans = scene["sm"], scene["poses"], scene["scans"]
    eng = scene["og"].engine()
    sincos = lambda t: device_sincos(eng, t)
    readings = [dict(x=float(poses[k][0]), y=float(poses[k][1]), theta=float(poses[k][2]), range=scans[k]) for k in (4, 5)]
    pts, stride = points.merge_scans(readings, fov=FOV, max_range=R)
    assert stride == 1 and len(pts) > BEAMS // 2
    window = (float(poses[5][0]), float(poses[5][1]), 1.0)
    res = sm.searchPoints(pts, window, step=0.25, headings=16)
    lv, lat = sm.last_cover["level"], sm.last_cover["lattice"]
    assert lv is sm.covering_level("fine", 1.0 + max(0.0, points.reach(pts) - R))      # the cached covering level of searchPoses
    fr = lv.frames()[0]
    field, frame = lv.field_cost(0).copy(), (float(fr["xlo"]), float(fr["ylo"]))
    free = sm.outside_cost_of(lv)
    want = pyard.search_points(field, frame, lv.step, lat, pts, free, *sincos(lyard.axes(lat)[2]))
    assert np.array_equal(res["cost"], want >> np.uint64(16)) and np.array_equal(res["heading"], (want & np.uint64(0xffff)).astype(np.int64))
    assert set(res) == {"cost", "heading", "score", "xs", "ys", "thetas", "peaks"} and res["peaks"][0].cost == int(res["cost"].min())
    seeds = poses[[5, 5]] + ((0.12, -0.09, 0.03), (-0.2, 0.1, -0.05))
    out = sm.refinePoints(seeds, pts, window=window)
    words, want_poses = pyard.refine_stages(field, frame, lv.step, seeds, matcher.default_stages(UNIT), pts, free, sincos=sincos)
    assert out["poses"].tobytes() == want_poses.tobytes() and np.array_equal(out["cost"], ryard.cost_of(words[:, -1]))
    assert np.array_equal(out["start_cost"], words[:, 0, 1]) and out["offsets"].shape == (2, 2, 3) and out["offsets"].any()
    per = sm.refinePoints(seeds, np.stack([pts, pts[::-1]]), stages=[((2, 2, 1), (0.1, 0.1, 0.02))], window=window)
    w1, p1 = pyard.refine_points(field, frame, lv.step, seeds, (2, 2, 1), (0.1, 0.1, 0.02), np.stack([pts, pts[::-1]]), free, sincos=sincos)
    assert per["poses"].tobytes() == p1.tobytes() and np.array_equal(per["cost"], ryard.cost_of(w1))
    for bad in (pts[:, :1], np.zeros((0, 2)), np.zeros((_lib.MAX_POINTS + 1, 2))):
        with pytest.raises(ValueError):
            sm.searchPoints(bad, window)
    with pytest.raises(ValueError):
        sm.refinePoints(seeds, np.stack([pts, pts, pts]))
