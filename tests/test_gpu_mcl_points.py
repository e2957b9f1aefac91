"""slam2d_mcl_step_points, slam2d_mcl_step_adaptive_points and slam2d_score_points on the MI355X against their definitions in NumPy
(tests/mcl_points_yardstick.py) and against the scan forms on the device: every comparison is np.array_equal on bits -- the
resampled poses, the ancestors, the report words, the eight slots of a score row.  The yardstick reads the DEVICE's field and the
device's cos / sin (slam2d_device_sincos) of the particles' headings before and after the move; everything else in the
definition is an integer operation or one rounded operation: there is no tolerance.  The field is the hand-made one of
tests/test_gpu_points.py, rebuilt here -- about 40 x 40 cells of random costs in slots 0 and 2 of a level of three, each with a
frame of its own, slot 1 a decoy --, the points lie over [-2.6, 2.6]^2, so they end beyond all four edges, and outside_cost is not
0.  Every call is made at the C ABI with buffers of its own, poisoned with 0xff bytes.  The Python layer alone runs on the
289 x 289 scene of tests/test_gpu_search.py."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import mcl_adapt_yardstick as ada
import mcl_points_yardstick as mpy
import points_yardstick as pyard
import test_gpu_mcl_adapt as tada
import test_gpu_search as tsearch
from test_gpu_mcl import same as same_step
from test_gpu_points import BAD, FRAMES, LIDAR, OUTSIDE, SHAPES, STEP, cloud, rows_of, scan_form, seeds_in
from test_gpu_search import device_sincos, pkg, scene  # noqa: F401  (scene: the 289 x 289 field, for the Python layer alone)
from test_score_host import FOV, R

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
points = importlib.import_module("slam-2d-lidar-scan_amd.points")

K = _lib.MCL_SCAN_BLOCK                                        # particles one block of the scan launch covers
assert K == 1024
POISON = np.uint64(0xffffffffffffffff)
MS = [1, 63, 64, 65, 127, 128, 129, 2048]                      # the wave's trip of 64 points and the pairs of trips of MCL_UNROLL
NS = [1, 3, 4, 5, 15, 16, 17, K - 1, K, K + 1, 2 * K + 1]      # 4 and 16 particles per scoring block (MCL_WAVES; the point forms' MCLP_WAVES),
#                                                                MCL_SCAN_BLOCK per scan block
AMP = (0.02, 0.015, 0.01)
MOTION = (0.11, -0.02, 0.05)
N_CAP = 2 * K + 1
TAB3 = (3 * np.arange(4096)).astype(np.uint32)                 # tab[k] = 3 k: shrinks a set of several particles per bin


def bins_of(p):
    """0.5 m x 0.5 m x 60 degrees over slot p's frame and a margin: the particles of seeds_in take a few dozen of them, several
    to a bin."""
    return ada.Bins(FRAMES[p][0] - 0.1, FRAMES[p][1] - 0.1, 0.5, 2 * math.pi / 6, 9, 9, 6)


@pytest.fixture(scope="module")
def ctx(pkg):
    """As tests/test_gpu_points.py builds it: a level of three with hand-made fields in slots 0 and 2 (SearchLevel.set_field, the
    frame records written beside them); slot 1 keeps a field of one cost that none of the tests may see."""
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
    return dict(eng=eng, lv=lv, fields=fields, maps=maps, sincos=lambda a: device_sincos(eng, a), tables={})


def table(ctx, M):
    """(lut, shift) of a temperature that grows with the set: the costs of poses a few cells apart differ by about sqrt(M) cells'
    worth, and a case wants several survivors."""
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    t = max(3.0, 1.5 * math.sqrt(M))
    if t not in ctx["tables"]:
        ctx["tables"][t] = engine.weight_table(ctx["lv"].c.cost_scale, t)
    return ctx["tables"][t]


def planted(M, seed, first=0):
    """cloud(M) with the six non-finite pairs of BAD, from the ``first``-th on, in rows 0, 63, 64 and M - 1 where the set has them
    (a set of one point keeps it)."""
    q = cloud(M, seed)
    for i, k in enumerate(sorted({k for k in (0, 63, 64, M - 1) if 0 <= k < M} if M > 1 else ())):
        q[k] = BAD[(first + i) % len(BAD)]
    return q


def strided(poses, stride):
    """The poses in rows of ``stride`` doubles, the other slots NaN."""
    out = np.full((len(poses), stride), np.nan)
    out[:, :3] = poses
    return out


# ---- the yardstick with the device's field and cos / sin ----
def expect_step(ctx, p, poses, motion, amp, seed, scan, pts, tab, outside=OUTSIDE):
    return mpy.step(ctx["fields"][p], FRAMES[p], STEP, np.asarray(poses, dtype=np.float64)[:, :3], motion, amp, seed, scan, pts, outside, *tab,
                    ctx["sincos"])


def expect_adaptive(ctx, p, poses, n_in, motion, amp, seed, scan, pts, tab, ntab=TAB3, outside=OUTSIDE):
    poses = np.asarray(poses, dtype=np.float64)
    return mpy.step_adaptive(ctx["fields"][p], FRAMES[p], STEP, poses[:, :3], n_in, len(poses), motion, amp, seed, scan, pts, outside, *tab,
                             bins_of(p), ntab, ctx["sincos"])


def expect_score(ctx, p, poses, pts):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    return mpy.score_points(ctx["fields"][p], FRAMES[p], ctx["lv"].c.cost_scale, STEP, poses, pts, *ctx["sincos"](poses[:, 2].copy()))


# ---- the calls at the C ABI, every buffer of its own and poisoned with 0xff bytes ----
def _full(eng, shape, dt):
    import torch
    return torch.full(shape, -1, dtype=dt, device=eng.device)


def _lut_on(eng, lut):
    import torch
    return torch.from_numpy(np.asarray(lut, dtype=np.uint32).view(np.int32).copy()).to(eng.device)


def launch_step(ctx, p, poses, motion, amp, seed, scan, pts, tab, outside=OUTSIDE, point_stride=2, ancestor=True):
    """slam2d_mcl_step_points on slot p.  ``poses``: [N, stride].  The dict tests/test_gpu_mcl.py compares: ``out`` [N, stride]
    (float64), ``ancestors`` (None without), ``report`` (uint64 [16]); the slots of the stride beyond the pose are still poison."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = ctx["eng"]
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    (N, stride), M, (lut, shift) = poses.shape, len(pts), tab
    d_in, d_pts, d_lut = eng.to_device(poses), eng.to_device(rows_of(pts, point_stride)), _lut_on(eng, lut)
    n = eng.L.slam2d_mcl_points_work(N)
    assert n == 7 * N + 1032
    work, rep, out = _full(eng, (n,), torch.int64), _full(eng, (_lib.MCL_REPORT,), torch.int64), _full(eng, (N, stride), torch.int64)
    anc = _full(eng, (N,), torch.int32) if ancestor else None
    _lib.check(eng.L.slam2d_mcl_step_points(ctypes.byref(ctx["lv"].c), p, N, d_in.data_ptr(), out.data_ptr(), stride, (ctypes.c_double * 3)(*motion),
                                            (ctypes.c_double * 3)(*amp), seed, scan, d_pts.data_ptr(), point_stride, M, int(outside),
                                            d_lut.data_ptr(), len(lut), shift, None if anc is None else anc.data_ptr(), work.data_ptr(),
                                            rep.data_ptr(), engine._stream()), "slam2d_mcl_step_points")
    words = out.cpu().numpy().view(np.uint64)
    assert (words[:, 3:] == POISON).all()
    return dict(out=words.view(np.float64), ancestors=None if anc is None else anc.cpu().numpy(), report=rep.cpu().numpy().view(np.uint64))


def launch_scan_step(ctx, p, poses, motion, amp, seed, scan, lid, d_rng, tab, outside=OUTSIDE):
    """slam2d_mcl_step on slot p for the scan ``d_rng`` of the lidar descriptor ``lid`` (scan_form): the same dict."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = ctx["eng"]
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    (N, stride), (lut, shift) = poses.shape, tab
    d_in, d_lut = eng.to_device(poses), _lut_on(eng, lut)
    work, rep = _full(eng, (eng.L.slam2d_mcl_work(N),), torch.int64), _full(eng, (_lib.MCL_REPORT,), torch.int64)
    out, anc = _full(eng, (N, stride), torch.int64), _full(eng, (N,), torch.int32)
    _lib.check(eng.L.slam2d_mcl_step(ctypes.byref(lid), ctypes.byref(ctx["lv"].c), p, N, d_in.data_ptr(), out.data_ptr(), stride,
                                     (ctypes.c_double * 3)(*motion), (ctypes.c_double * 3)(*amp), seed, scan, d_rng.data_ptr(), int(outside),
                                     d_lut.data_ptr(), len(lut), shift, anc.data_ptr(), work.data_ptr(), rep.data_ptr(), engine._stream()),
               "slam2d_mcl_step")
    return dict(out=out.cpu().numpy().view(np.float64), ancestors=anc.cpu().numpy(), report=rep.cpu().numpy().view(np.uint64))


def launch_adaptive(ctx, p, poses, n_in, motion, amp, seed, scan, pts, tab, ntab=TAB3, outside=OUTSIDE, point_stride=2):
    """slam2d_mcl_step_adaptive_points on slot p.  ``poses``: [n_cap, stride].  The dict tests/test_gpu_mcl_adapt.py compares:
    ``out`` [n_cap, stride] as uint64 words, ``ancestors`` [n_cap], ``report`` (uint64 [24]), ``n_out``."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = ctx["eng"]
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    (n_cap, stride), M, (lut, shift) = poses.shape, len(pts), tab
    ntab = np.ascontiguousarray(ntab, dtype=np.uint32)
    cb = tada.c_bins(bins_of(p))
    d_in, d_pts, d_lut, d_ntab = eng.to_device(poses), eng.to_device(rows_of(pts, point_stride)), _lut_on(eng, lut), _lut_on(eng, ntab)
    d_n_in = torch.from_numpy(np.array([n_in], dtype=np.uint32).view(np.int32)).to(eng.device)
    n = eng.L.slam2d_mcl_adapt_points_work(n_cap, ctypes.byref(cb))
    assert n == 7 * n_cap + 1032 + (cb.nx * cb.ny * cb.nth + 64) // 64 + 8
    work, rep = _full(eng, (n,), torch.int64), _full(eng, (_lib.MCL_ADAPT_REPORT,), torch.int64)
    out, anc, d_n_out = _full(eng, (n_cap, stride), torch.int64), _full(eng, (n_cap,), torch.int32), _full(eng, (1,), torch.int32)
    _lib.check(eng.L.slam2d_mcl_step_adaptive_points(ctypes.byref(ctx["lv"].c), p, n_cap, d_n_in.data_ptr(), d_n_out.data_ptr(), d_in.data_ptr(),
                                                     out.data_ptr(), stride, (ctypes.c_double * 3)(*motion), (ctypes.c_double * 3)(*amp), seed, scan,
                                                     d_pts.data_ptr(), point_stride, M, int(outside), d_lut.data_ptr(), len(lut), shift,
                                                     ctypes.byref(cb), d_ntab.data_ptr(), len(ntab), anc.data_ptr(), work.data_ptr(), rep.data_ptr(),
                                                     engine._stream()), "slam2d_mcl_step_adaptive_points")
    assert int(d_n_in.cpu().numpy().view(np.uint32)[0]) == n_in                       # (the input word is only read)
    return dict(out=out.cpu().numpy().view(np.uint64), ancestors=anc.cpu().numpy(), report=rep.cpu().numpy().view(np.uint64),
                n_out=int(d_n_out.cpu().numpy().view(np.uint32)[0]))


def launch_score(ctx, p, poses, pts, pose_stride=3, point_stride=2, pad=0):
    """slam2d_score_points on slot p: the rows [N, 8].  ``pts`` [M, 2]: set_stride 0; [N, M, 2]: a set per pose, ``pad`` doubles
    between the sets."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = ctx["eng"]
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    pts = np.asarray(pts, dtype=np.float64)
    N, M = len(poses), pts.shape[-2]
    rows, set_stride = rows_of(pts, point_stride), 0
    if pts.ndim == 3:
        set_stride = M * point_stride + pad
        rows = np.concatenate([rows.reshape(N, -1), np.full((N, pad), np.nan)], axis=1)
    d_pose, d_pts = eng.to_device(strided(poses, pose_stride)), eng.to_device(rows)
    out = _full(eng, (N, _lib.SCORE_STRIDE), torch.int64)
    _lib.check(eng.L.slam2d_score_points(ctypes.byref(ctx["lv"].c), p, N, d_pose.data_ptr(), pose_stride, d_pts.data_ptr(), point_stride, M,
                                         set_stride, out.data_ptr(), engine._stream()), "slam2d_score_points")
    return out.cpu().numpy().view(np.float64)


def same_rows(got, want, what=""):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (what, np.argwhere(got != want)[:6].tolist(), got[got != want][:6],
                                                                          want[got != want][:6])


def lively(res, N):
    """On the yardstick first: the case resamples for real -- more than one survivor, fewer than all, more than one weight."""
    rep = res["report"]
    assert 1 < int(rep[6]) < N and int(rep[3]) > 1 and len(np.unique(res["w"])) > 2 and int(rep[10]) == N, [int(v) for v in rep]


# ---- slam2d_mcl_step_points against the yardstick ----
def test_one_step_in_both_slots(ctx):
    N, pts = 257, cloud(100, 3, invalid=(7, 40))
    tab = table(ctx, 100)
    for p in (0, 2):
        poses = seeds_in(p, N, 11 + p)
        want = expect_step(ctx, p, poses, MOTION, AMP, 7, 3, pts, tab)
        lively(want, N)
        assert int(want["report"][5]) == 98 and want["cost"].min() > 10 * OUTSIDE        # points outside the field at every pose
        same_step(launch_step(ctx, p, poses, MOTION, AMP, 7, 3, pts, tab), want, f"slot {p}")
        other = expect_step(ctx, 2 - p, poses, MOTION, AMP, 7, 3, pts, tab)
        assert not np.array_equal(other["cost"], want["cost"])   # (the other slot's field and frame give other costs)


@pytest.mark.parametrize("M", MS)
def test_point_counts(ctx, M):
    """Every trip count of the point loop around its boundaries, with each of the six non-finite pairs in rows 0, 63, 64 and M - 1
    where the set has them -- twice, so that every pair has been in a row --, and with all points valid in rows of three doubles."""
    N, p, tab = 70, 0 if M % 2 else 2, table(ctx, M)
    poses = seeds_in(p, N, M)
    for first in (0, 3):
        pts = planted(M, M + first, first)
        assert 0 < int(pyard.valid(pts).sum()) == M - (0 if M == 1 else len({0, 63, 64, M - 1} & set(range(M))))
        want = expect_step(ctx, p, poses, MOTION, AMP, 5, M, pts, tab)
        same_step(launch_step(ctx, p, poses, MOTION, AMP, 5, M, pts, tab), want, f"{M} points, pairs from {first}")
    if M >= 63:
        lively(want, N)
    full = cloud(M, M + 1)
    same_step(launch_step(ctx, p, poses, MOTION, AMP, 5, M, full, tab, point_stride=3), expect_step(ctx, p, poses, MOTION, AMP, 5, M, full, tab),
              f"{M} points, all valid, rows of 3")


def test_a_set_without_a_valid_point(ctx):
    """Cost 0 at every pose: every weight is d_lut[0], best = 0, word 5 = 0, and every particle is its own offspring."""
    N, tab = 70, table(ctx, 9)
    poses = seeds_in(0, N, 1)
    none = np.array(BAD + BAD[:3])
    for amp in (AMP, (0.0, 0.0, 0.0)):
        want = expect_step(ctx, 0, poses, MOTION, amp, 9, 1, none, tab)
        rep = want["report"]
        assert [int(rep[i]) for i in (0, 1, 5)] == [0, 0, 0] and int(rep[2]) == N * int(tab[0][0]) and int(rep[3]) == int(rep[6]) == N
        assert np.array_equal(want["ancestors"], np.arange(N))
        same_step(launch_step(ctx, 0, poses, MOTION, amp, 9, 1, none, tab), want, f"no valid point, amp {amp}")


@pytest.mark.parametrize("N", NS)
def test_particle_counts(ctx, N):
    """One scoring block and its last wave, one scan block to its last particle, two and three scan blocks -- in both slots."""
    pts, tab = cloud(90, N, invalid=(0, 89)), table(ctx, 90)
    for p in (0, 2):
        poses = seeds_in(p, N, N + p)
        want = expect_step(ctx, p, poses, MOTION, AMP, 0xfeedfacecafebeef, (1 << 40) + N, pts, tab)
        if N > K:                                              # the best pose goes last, where the scan blocks are joined: it survives there
            poses[[int(want["report"][1]), N - 1]] = poses[[N - 1, int(want["report"][1])]]
            want = expect_step(ctx, p, poses, MOTION, AMP, 0xfeedfacecafebeef, (1 << 40) + N, pts, tab)
            assert want["ancestors"].max() == N - 1 and want["ancestors"].min() < K    # survivors in the first scan block and in the last
        if N > 64:
            lively(want, N)
        same_step(launch_step(ctx, p, poses, MOTION, AMP, 0xfeedfacecafebeef, (1 << 40) + N, pts, tab), want, f"N = {N}, slot {p}")


def test_strides_with_nan_in_the_unread_slots(ctx):
    """Pose rows of five doubles and point rows of three, every unread slot a NaN: the bits of rows of three and two, and the
    output's unread slots untouched; without d_ancestor the rest is the same."""
    N, pts, tab = 130, cloud(77, 2, invalid=(5,)), table(ctx, 77)
    poses = seeds_in(2, N, 4)
    want = expect_step(ctx, 2, poses, MOTION, AMP, 3, 8, pts, tab)
    lively(want, N)
    for pose_stride in (3, 5):
        for point_stride in (2, 3):
            got = launch_step(ctx, 2, strided(poses, pose_stride), MOTION, AMP, 3, 8, pts, tab, point_stride=point_stride)
            assert got["out"].shape == (N, pose_stride)
            same_step(got, want, f"rows of {pose_stride} and {point_stride}")
    got = launch_step(ctx, 2, strided(poses, 5), MOTION, AMP, 3, 8, pts, tab, point_stride=3, ancestor=False)
    assert got["ancestors"] is None
    same_step(got, want, "no d_ancestor")


def test_poses_with_a_component_that_is_not_finite(ctx):
    """No point of such a pose is inside: it costs valid * outside_cost, keeps its weight's share, and is left out of the sums."""
    N, pts, tab = 96, cloud(60, 6, invalid=(3,)), table(ctx, 60)
    poses = seeds_in(0, N, 2)
    x, y, th = poses[0]
    bad = [(np.nan, y, th), (x, np.inf, th), (x, y, np.nan), (x, y, -np.inf), (1e12, y, th), (-np.inf, np.nan, th)]
    poses[10:10 + len(bad)] = bad
    for amp in (AMP, (0.0, 0.0, 0.0)):
        want = expect_step(ctx, 0, poses, MOTION, amp, 21, 5, pts, tab)
        assert (want["cost"][10:16] == 59 * OUTSIDE).all() and want["cost"][:10].min() > 59 * OUTSIDE
        assert set(range(10, 16)) <= set(want["ancestors"].tolist()) and int(want["report"][10]) < N     # they survive: the cheapest poses
        same_step(launch_step(ctx, 0, poses, MOTION, amp, 21, 5, pts, tab), want, f"bad poses, amp {amp}")


def test_without_noise_and_without_motion(ctx):
    N, pts, tab = 130, cloud(64, 8), table(ctx, 64)
    poses = seeds_in(2, N, 9)
    for motion, amp in ((MOTION, (0.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), AMP), ((-0.07, 0.04, -0.3), (0.0, 0.03, 0.0))):
        want = expect_step(ctx, 2, poses, motion, amp, 1, 2, pts, tab)
        same_step(launch_step(ctx, 2, poses, motion, amp, 1, 2, pts, tab), want, f"motion {motion}, amp {amp}")
    assert want["moved"][:, 0].tobytes() != poses[:, 0].tobytes()


def test_two_scans_ping_ponged_and_the_same_call_twice(ctx):
    """The resampled set of scan number s is the input of s + 1, with another set of points; every call twice: the same bytes,
    whatever garbage d_work, d_report and the outputs held."""
    N, tab = 300, table(ctx, 120)
    cur_want = cur_got = seeds_in(0, N, 6)
    for i, (motion, M) in enumerate(((MOTION, 120), ((0.03, 0.09, 1.1), 131))):
        pts = cloud(M, 40 + i, invalid=(64,))
        given = cur_want
        want = expect_step(ctx, 0, given, motion, AMP, 99, 40 + i, pts, tab)
        got = launch_step(ctx, 0, cur_got, motion, AMP, 99, 40 + i, pts, tab)
        again = launch_step(ctx, 0, cur_got, motion, AMP, 99, 40 + i, pts, tab)
        assert all(got[k].tobytes() == again[k].tobytes() for k in got), i
        same_step(got, want, f"scan {40 + i}")
        cur_want, cur_got = want["out"], got["out"]
    assert int(want["report"][6]) > 1
    assert not np.array_equal(want["report"], expect_step(ctx, 0, given, (0.03, 0.09, 1.1), AMP, 99, 40, pts, tab)["report"])   # (the scan number matters)


# ---- the anchor to the scan form ----
def test_at_heading_zero_the_step_is_slam2d_mcl_step_on_the_scan(ctx):
    """Particles of heading exactly 0, no turn and no heading noise, the set scan_points(ranges) with the device's cos / sin of the
    beam angles: the poses, the ancestors and all sixteen words of slam2d_mcl_step on the same field at 60 beams -- word 5 too:
    the valid points are the beams in range."""
    N, beams = 200, 60
    rs = np.random.RandomState(beams)
    rng = rs.uniform(0.05, 1.3 * LIDAR[1], beams)              # about a quarter out of range; the longest end beyond the field
    rng[[4, 17]] = np.nan, np.inf
    lid, d_rng, pts = scan_form(ctx, rng)
    assert np.array_equal(pyard.valid(pts), rng < LIDAR[1]) and 0 < int(pyard.valid(pts).sum()) < beams
    tab = table(ctx, beams)
    for p in (0, 2):
        poses = seeds_in(p, N, 5 + p)
        poses[:, 2] = 0.0
        motion, amp = (0.11, -0.02, 0.0), (0.02, 0.015, 0.0)
        want = launch_scan_step(ctx, p, poses, motion, amp, 13, 6, lid, d_rng, tab)
        assert 1 < int(want["report"][6]) < N and int(want["report"][5]) == int((rng < LIDAR[1]).sum())
        got = launch_step(ctx, p, poses, motion, amp, 13, 6, pts, tab)
        assert np.array_equal(got["report"], want["report"]), ([hex(v) for v in got["report"]], [hex(v) for v in want["report"]])
        assert np.array_equal(got["ancestors"], want["ancestors"]) and got["out"].tobytes() == want["out"].tobytes(), p
        same_step(got, expect_step(ctx, p, poses, motion, amp, 13, 6, pts, tab), f"slot {p}: the yardstick too")


# ---- slam2d_mcl_step_adaptive_points ----
@pytest.mark.parametrize("n_in", [1, K - 1, K + 1, N_CAP])
def test_adaptive_live_counts(ctx, n_in):
    """Live counts in buffers of capacity 2049: poses beyond the count are 0xff bytes that no result may hold, rows beyond N_out
    stay poisoned."""
    p = 0 if n_in % 2 else 2
    pts, tab = cloud(90, n_in, invalid=(0, 64)), table(ctx, 90)
    poses = tada.padded(seeds_in(p, n_in, n_in), N_CAP)
    want = expect_adaptive(ctx, p, poses, n_in, MOTION, AMP, 17, n_in, pts, tab)
    assert want["N"] == n_in and int(want["report"][5]) == 88
    if n_in > 1:
        assert 1 < want["kbins"] < len(want["reference"]) < n_in and want["n_out"] == 3 * want["kbins"] != n_in
    tada.same(launch_adaptive(ctx, p, poses, n_in, MOTION, AMP, 17, n_in, pts, tab), want, f"{n_in} live of {N_CAP}")
    # rows of five doubles and point rows of three
    got = launch_adaptive(ctx, p, tada.padded(poses[:, :3], N_CAP, 5), n_in, MOTION, AMP, 17, n_in, pts, tab, point_stride=3)
    tada.same(got, want, f"{n_in} live of {N_CAP}, rows of 5 and 3")


@pytest.mark.parametrize("N", [5, K + 1])
def test_a_constant_table_at_the_capacity_is_the_plain_step(ctx, N):
    """*d_n_in == n_cap and a table that returns n_cap: the poses, the ancestors and words 0-15 of slam2d_mcl_step_points(N = n_cap)
    ON THE DEVICE, bit for bit; word 19 is word 6."""
    pts, tab = cloud(129, N, invalid=(128,)), table(ctx, 129)
    poses = seeds_in(2, N, N)
    plain = launch_step(ctx, 2, poses, MOTION, AMP, 3, N, pts, tab)
    got = launch_adaptive(ctx, 2, poses, N, MOTION, AMP, 3, N, pts, tab, ntab=[N])
    assert got["n_out"] == N and np.array_equal(got["report"][:16], plain["report"])
    assert np.array_equal(got["ancestors"], plain["ancestors"]) and np.array_equal(got["out"], plain["out"].view(np.uint64))
    assert [int(v) for v in got["report"][16:18]] == [N, N] and got["report"][19] == got["report"][6] and not got["report"][20:].any()
    tada.same(got, expect_adaptive(ctx, 2, poses, N, MOTION, AMP, 3, N, pts, tab, ntab=[N]), f"N = {N}")


# ---- slam2d_score_points ----
@pytest.mark.parametrize("M", MS)
def test_score_points(ctx, M):
    """All eight slots, one set for every pose and a set per pose (of another valid count each, the sets a few doubles apart), 1,
    4, 5 and 9 poses: one block and its last wave, two blocks, three -- and from 1366 points on two poses per block."""
    p = 0 if M % 2 else 2
    pts = planted(M, M)
    for N in (1, 4, 5, 9):
        poses = seeds_in(p, N, M + N)
        want = expect_score(ctx, p, poses, pts)
        same_rows(launch_score(ctx, p, poses, pts), want, f"{M} points, {N} poses, one set")
        if M > 1:
            assert (want[:, 4] == pyard.valid(pts).sum()).all() and (want[:, 3] < want[:, 4]).all() and (want[:, 3] > 0).any()
        per = np.stack([cloud(M, 100 * N + n, invalid=tuple(range(min(n, M - 1)))) for n in range(N)])
        want = expect_score(ctx, p, poses, per)
        assert list(want[:, 4]) == [M - min(n, M - 1) for n in range(N)]
        same_rows(launch_score(ctx, p, poses, per, pose_stride=5, point_stride=3, pad=5), want, f"{M} points, {N} poses, a set each")
    if M >= 127:
        assert (want[:, 1] < want[:, 3]).any()                 # (points that share a cell: the set is smaller than the count)


def test_score_of_a_set_in_one_cell_and_of_poses_that_are_not_finite(ctx):
    x, y, th = seeds_in(0, 1, 3)[0]
    for M in (1, 64, 200):
        one = np.tile([[0.3, -0.2]], (M, 1))
        want = expect_score(ctx, 0, [(x, y, th)], one)
        c, s = ctx["sincos"](np.array([th]))
        inside, cx, cy = pyard.cells(SHAPES[0], FRAMES[0], STEP, x, y, *pyard.offsets(one[:1], c[0], s[0]))
        cost = float(ctx["fields"][0][cy[0], cx[0]])
        assert inside.all() and list(want[0, [1, 3, 4]]) == [1, M, M] and want[0, 6] == M * want[0, 5] == M * cost > 0
        same_rows(launch_score(ctx, 0, [(x, y, th)], one), want, f"{M} points in one cell")
    pts = cloud(40, 2, invalid=(11,))
    poses = np.array([(np.nan, y, th), (x, np.inf, th), (x, y, np.nan), (x, y, -np.inf), (1e12, y, th), (x, y, th)])
    want = expect_score(ctx, 0, poses, pts)
    assert not want[:5, [0, 1, 2, 3, 5, 6]].any() and (want[:, 4] == 39).all() and want[5, 3] > 0
    same_rows(launch_score(ctx, 0, poses, pts), want, "poses that are not finite")


def test_at_heading_zero_the_score_is_slam2d_score_poses_on_the_scan(ctx):
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng, lv = ctx["eng"], ctx["lv"]
    rs = np.random.RandomState(61)
    rng = rs.uniform(0.05, 1.3 * LIDAR[1], 60)
    rng[[4, 17]] = np.nan, np.inf
    lid, d_rng, pts = scan_form(ctx, rng)
    for p in (0, 2):
        poses = seeds_in(p, 9, 7 + p)
        poses[:, 2] = 0.0
        poses[:3, 0] += 1.9                                    # (towards the field's edge: the beams ahead end beyond it)
        out = torch.full((9, _lib.SCORE_STRIDE), -1, dtype=torch.int64, device=eng.device)
        _lib.check(eng.L.slam2d_score_poses(ctypes.byref(lid), ctypes.byref(lv.c), p, 9, eng.to_device(poses).data_ptr(), 3, d_rng.data_ptr(), 0,
                                            out.data_ptr(), engine._stream()), "slam2d_score_poses")
        want = out.cpu().numpy().view(np.float64)
        assert (want[:, 4] == (rng < LIDAR[1]).sum()).all() and (want[:, 3] > 0).any() and (want[:, 3] < want[:, 4]).any()
        same_rows(launch_score(ctx, p, poses, pts), want, f"slot {p}: the scan form's rows")


# ---- the Python layer, on the 289 x 289 scene ----
def merged_sets(scene, count):
    """``count`` point sets of unequal length: the last one, two or three scans of the walk merged through its poses."""
    poses, scans = scene["poses"], scene["scans"]
    readings = [dict(x=float(p[0]), y=float(p[1]), theta=float(p[2]), range=s) for p, s in zip(poses, scans)]
    sets = [points.merge_scans(readings[max(0, i - i % 3):i + 1], fov=FOV, max_range=R)[0] for i in range(count)]
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    motions = [localise.odometry_motion(readings[i - 1], readings[i]) if i else (0.0, 0.0, 0.0) for i in range(count)]
    return sets, motions


def test_localiser_step_points_is_the_engine_call(pkg, scene):
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    N, sigma = 130, (0.03, 0.02, 0.015)
    loc = pkg.Localiser(scene["sm"], tsearch.WINDOW, particles=N, sigma=sigma, temperature=64.0, seed=5)
    start = loc.seed_at(scene["poses"][0], (0.05, 0.05, 0.03))
    sets, motions = merged_sets(scene, 2)
    rep = loc.step_points(sets[1], motions[1])
    eng, lv = loc.eng, loc.level
    d_out, d_rep = torch.empty((N, 3), dtype=torch.float64, device=eng.device), torch.empty(16, dtype=torch.int64, device=eng.device)
    eng.mcl_step_points(lv, 0, eng.to_device(start), d_out, N, motions[1], loc.amp, 5, 0, eng.to_device(sets[1]), len(sets[1]), loc.outside_cost,
                        loc.d_lut, loc.shift, d_rep)
    assert rep == engine.mcl_report_host(d_rep) and loc.poses().tobytes() == d_out.cpu().numpy().tobytes()
    assert rep["in_range"] == len(sets[1]) > 60 and loc.scan == 1
    # ... and the yardstick's on the Localiser's own field
    fr = lv.frames()[0]
    want = mpy.step(lv.field_cost(0), (float(fr["xlo"]), float(fr["ylo"])), lv.step, start, motions[1], loc.amp, 5, 0, sets[1], loc.outside_cost,
                    loc.d_lut.cpu().numpy().view(np.uint32), loc.shift, lambda a: device_sincos(eng, a))
    assert np.array_equal(d_rep.cpu().numpy().view(np.uint64), want["report"]) and loc.poses().tobytes() == want["out"].tobytes()


@pytest.mark.parametrize("adaptive", [None, dict(n_min=40, bin_xy=0.1, bin_theta=math.radians(5.0))])
def test_run_points_is_six_step_points_calls(pkg, scene, adaptive):
    N, sigma = 300, (0.03, 0.02, 0.015)
    a, b = (pkg.Localiser(scene["sm"], tsearch.WINDOW, particles=N, sigma=sigma, temperature=64.0, seed=9, adaptive=adaptive) for _ in range(2))
    for loc in (a, b):
        loc.seed_at(scene["poses"][0], (0.05, 0.05, 0.03))
    sets, motions = merged_sets(scene, 6)
    assert len({len(s) for s in sets}) >= 3
    reports = a.run_points(sets, motions)
    steps = [b.step_points(s, m) for s, m in zip(sets, motions)]
    assert reports == steps and a.poses().tobytes() == b.poses().tobytes() and a.scan == b.scan == 6
    assert [r["in_range"] for r in reports] == [len(s) for s in sets]
    if adaptive is not None:
        assert a.count == b.count == reports[-1]["n_out"] and [r["n_in"] for r in reports[1:]] == [r["n_out"] for r in reports[:-1]]


def test_score_points_of_the_matcher_is_the_engine_call(pkg, scene):
    sm, eng = scene["sm"], scene["eng"]
    sets, _ = merged_sets(scene, 6)
    pts = sets[5]
    poses = scene["poses"][[5, 5, 4]] + ((0.0, 0.0, 0.0), (0.12, -0.09, 0.03), (0.0, 0.0, 0.0))
    res = sm.scorePoints(poses, pts, window=tsearch.WINDOW)
    lv = sm.last_cover["level"]
    assert lv is sm.points_level("fine", tsearch.WINDOW[2], pts)
    rows = eng.score_points(lv, 0, eng.to_device(poses), 3, 3, eng.to_device(pts), len(pts), 0)
    want = eng.score_host(rows)
    assert set(res) == {"score", "cells", "beam_score", "inside", "valid", "outside"} and (res["valid"] == len(pts)).all()
    assert all(np.array_equal(res[k], want["in_range" if k == "valid" else k]) for k in res)
    assert res["score"][0] > res["score"][2] and res["inside"][0] > 60      # the pose the last scan was taken at fits best
    fr = lv.frames()[0]
    yard_rows = mpy.score_points(lv.field_cost(0), (float(fr["xlo"]), float(fr["ylo"])), lv.c.cost_scale, lv.step, poses, pts,
                                 *device_sincos(eng, poses[:, 2].copy()))
    assert rows.cpu().numpy().tobytes() == yard_rows.tobytes()
    per = sm.scorePoints(poses, np.stack([pts, pts[::-1], pts]), window=tsearch.WINDOW)
    assert all(np.array_equal(per[k], res[k]) for k in res)     # (a set is a set: its order does not matter)
