"""slam2d_mcl_step_adaptive on the MI355X against its definition in NumPy (tests/mcl_adapt_yardstick.py) and against
slam2d_mcl_step on the device: every comparison is np.array_equal on bits -- the poses of rows < N_out, the poison of 0xff bytes
intact in rows >= N_out, the ancestors, the 24 report words and the count word.  Scene of tests/test_gpu_mcl.py (its constants
are imported, its field is built here as its ``scene`` fixture builds it); the yardstick reads the DEVICE's field, frame and
cos / sin, so there is no tolerance."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import mcl_adapt_yardstick as ada
import mcl_yardstick as mcl
from test_gpu_mcl import AMP, BAD, BEAMS, K, MOTIONS, SMP, TEMPERATURE, WINDOW
from test_gpu_mcl import launch as plain_launch
from test_score_host import FOV, INIT, ORIGIN, R, SIZE, UNIT, WALL

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

POISON = np.uint64(0xffffffffffffffff)
TWO_PI = 2 * math.pi
# 0.1 m x 0.1 m x 10 degrees over the window: a cloud of the spreads below holds several particles per bin, and several bins
BINS = ada.Bins(WINDOW[0] - WINDOW[2], WINDOW[1] - WINDOW[2], 0.1, TWO_PI / 36, 160, 160, 36)
TAB3 = (3 * np.arange(4096)).astype(np.uint32)                 # tab[k] = 3 k: shrinks a set of several particles per bin
TAB_POW = (1 << np.minimum(np.arange(64), 20)).astype(np.uint32)           # tab[k] = 2^k: doubles with every bin, grows any set of a dozen bins


def device_sincos(eng, angles):
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    a = eng.to_device(np.ascontiguousarray(angles, dtype=np.float64).reshape(-1))
    c, s = torch.empty_like(a), torch.empty_like(a)
    _lib.check(eng.L.slam2d_device_sincos(a.data_ptr(), a.numel(), c.data_ptr(), s.data_ptr(), engine._stream()), "sincos")
    return c.cpu().numpy().reshape(np.shape(angles)), s.cpu().numpy().reshape(np.shape(angles))


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


@pytest.fixture(scope="module")
def scene(pkg):
    """As tests/test_gpu_mcl.py builds it: the well-mapped world on the device, a matcher on it, a covering level with its field
    built in full -- downloaded once and shared --, the walk and its scans at 180 beams, the weight table."""
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


def padded(poses, n_cap, stride=3):
    """[n_cap, stride] float64: the poses in front, every other byte 0xff -- rows beyond the live count are NaNs no result may hold."""
    out = np.full((n_cap, stride), POISON, dtype=np.uint64).view(np.float64)
    out[:len(poses), :3] = poses
    return out


def expect(scene, poses, n_in, n_cap, motion, amp, seed, scan, ranges, bins=BINS, ntab=TAB3, outside=None, lut=None, shift=None):
    return ada.step(scene["field"], scene["frame"], scene["lv"].c.cost_scale, scene["lv"].step, np.asarray(poses, dtype=np.float64)[:, :3], n_in,
                    n_cap, motion, amp, seed, scan, ranges, FOV, R, scene["free"] if outside is None else outside,
                    scene["lut"] if lut is None else lut, scene["shift"] if shift is None else shift, bins, ntab, scene["sincos"])


def c_bins(bins):
    b = ada.Bins(*bins)
    return _lib.Slam2dMclBins(x0=b.x0, y0=b.y0, cell=b.cell, turn=b.turn, nx=b.nx, ny=b.ny, nth=b.nth)


def launch(scene, poses, n_in, motion, amp, seed, scan, ranges, bins=BINS, ntab=TAB3, outside=None, lut=None, shift=None, ancestor=True,
           level=None, p=0):
    """slam2d_mcl_step_adaptive at the C ABI with buffers of its own, all of them poisoned with 0xff bytes (the output count
    word too: another word than the input's).  ``poses``: [n_cap, stride], ``n_in``: the input count word; ``level``, ``p``: the
    Slam2dLevel and its field slot (default: slot 0 of the scene's level).  Returns dict of
    ``out`` [n_cap, stride] as uint64 words, ``ancestors`` ([n_cap]; None without), ``report`` (uint64 [24]), ``n_out``."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng = scene["eng"]
    lvc = scene["lv"].c if level is None else level
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    n_cap, stride = poses.shape
    lid = _lib.Slam2dLidar.from_buffer_copy(eng.lidar_c)
    lid.beams = len(ranges)
    lut = scene["lut"] if lut is None else np.asarray(lut, dtype=np.uint32)
    ntab = np.ascontiguousarray(ntab, dtype=np.uint32)
    cb = c_bins(bins)
    d_in, d_rng = eng.to_device(poses), eng.to_device(np.asarray(ranges, dtype=np.float64))
    d_lut = torch.from_numpy(lut.view(np.int32).copy()).to(eng.device)
    d_ntab = torch.from_numpy(ntab.view(np.int32).copy()).to(eng.device)
    d_n_in = torch.from_numpy(np.array([n_in], dtype=np.uint32).view(np.int32)).to(eng.device)
    n = eng.L.slam2d_mcl_adapt_work(n_cap, ctypes.byref(cb))
    assert n == 5 * n_cap + 1032 + (cb.nx * cb.ny * cb.nth + 64) // 64 + 8
    full = lambda shape, dt: torch.full(shape, -1, dtype=dt, device=eng.device)
    work, rep, out = full((n,), torch.int64), full((_lib.MCL_ADAPT_REPORT,), torch.int64), full((n_cap, stride), torch.int64)
    anc, d_n_out = full((n_cap,), torch.int32) if ancestor else None, full((1,), torch.int32)
    _lib.check(eng.L.slam2d_mcl_step_adaptive(ctypes.byref(lid), ctypes.byref(lvc), p, n_cap, d_n_in.data_ptr(), d_n_out.data_ptr(),
                                              d_in.data_ptr(), out.data_ptr(), stride, (ctypes.c_double * 3)(*motion), (ctypes.c_double * 3)(*amp),
                                              seed, scan, d_rng.data_ptr(), scene["free"] if outside is None else outside, d_lut.data_ptr(),
                                              len(lut), scene["shift"] if shift is None else shift, ctypes.byref(cb), d_ntab.data_ptr(), len(ntab),
                                              None if anc is None else anc.data_ptr(), work.data_ptr(), rep.data_ptr(), engine._stream()),
               "slam2d_mcl_step_adaptive")
    assert int(d_n_in.cpu().numpy().view(np.uint32)[0]) == n_in                       # (the input word is only read)
    return dict(out=out.cpu().numpy().view(np.uint64), ancestors=None if anc is None else anc.cpu().numpy(),
                report=rep.cpu().numpy().view(np.uint64), n_out=int(d_n_out.cpu().numpy().view(np.uint32)[0]))


def same(got, want, what=""):
    """Bits: the count word, the 24 words, the first N_out poses as 64-bit words (a NaN equals itself) and ancestors; behind
    them, and in the slots of the stride beyond the pose, the poison as it was."""
    n_out = want["n_out"]
    assert got["n_out"] == n_out, (what, got["n_out"], n_out)
    assert np.array_equal(got["report"], want["report"]), (what, [hex(v) for v in got["report"]], [hex(v) for v in want["report"]])
    if got["ancestors"] is not None:
        bad = np.flatnonzero(got["ancestors"][:n_out] != want["ancestors"])
        assert got["ancestors"].dtype == np.int32 and not bad.size, (what, bad[:6].tolist(), got["ancestors"][bad[:6]], want["ancestors"][bad[:6]])
        assert (got["ancestors"][n_out:] == -1).all(), what
    g, w = got["out"][:n_out, :3], np.ascontiguousarray(want["out"]).view(np.uint64)
    assert np.array_equal(g, w), (what, np.argwhere(g != w)[:6].tolist())
    assert (got["out"][n_out:] == POISON).all() and (got["out"][:, 3:] == POISON).all(), what


def for_real(res):
    """On the yardstick first: the reference resampling has more than one bin, several members per bin, fewer than all."""
    assert 1 < res["kbins"] < len(res["reference"]) < res["N"], (res["kbins"], len(res["reference"]), res["N"])


# ---- 1. equivalence ----
@pytest.mark.parametrize("N", [1, 64, 65, K - 1, K, K + 1, 2 * K + 1, 8193])
def test_a_constant_table_at_the_capacity_is_slam2d_mcl_step(scene, N):
    """*d_n_in == n_cap and a table that returns n_cap: the poses, the ancestors and words 0-15 of slam2d_mcl_step(N = n_cap) ON
    THE DEVICE, bit for bit; word 19 is word 6; and all of it is the yardstick's.  N = 8193 is one particle beyond the scoring
    launch's grid (MCLA_SCORE_BLOCKS blocks of four waves): its stride loop takes a second trip."""
    rng = scene["scans"][2]
    poses = cloud(scene, 2, N)
    args = (MOTIONS[3], AMP, 0xfeedfacecafebeef, (1 << 40) + N, rng)
    plain = plain_launch(scene, poses, *args)
    got = launch(scene, poses, N, *args, ntab=[N])
    assert got["n_out"] == N and np.array_equal(got["report"][:16], plain["report"])
    assert np.array_equal(got["ancestors"], plain["ancestors"]) and np.array_equal(got["out"], plain["out"].view(np.uint64))
    assert [int(v) for v in got["report"][16:18]] == [N, N] and got["report"][19] == got["report"][6] and not got["report"][20:].any()
    same(got, expect(scene, poses, N, N, *args, ntab=[N]), f"N = {N}")


def test_the_stride_loops_beyond_their_first_trip(scene):
    """N = n_cap = 262144 + 257 and a constant table [N]: the second trip of every grid of MCLA_BLOCKS blocks of 256 threads and
    the third of the reference launch's (MCLA_REF_BLOCKS).  On the device only -- the yardstick takes a minute at this size --:
    the poses, the ancestors and words 0-15 of slam2d_mcl_step(N) bit for bit, the counts, word 19 is word 6, no padding word set."""
    N = 1024 * 256 + 257
    rng = scene["scans"][2]
    poses = cloud(scene, 2, N)
    args = (MOTIONS[3], AMP, 0xfeedfacecafebeef, (1 << 40) + N, rng)
    plain = plain_launch(scene, poses, *args)
    got = launch(scene, poses, N, *args, ntab=[N])
    assert got["n_out"] == N and np.array_equal(got["report"][:16], plain["report"])
    assert np.array_equal(got["ancestors"], plain["ancestors"]) and np.array_equal(got["out"], plain["out"].view(np.uint64))
    assert [int(v) for v in got["report"][16:18]] == [N, N] and got["report"][19] == got["report"][6] and not got["report"][20:].any()


# ---- 2. a live count below the capacity ----
@pytest.mark.parametrize("n_cap, n_in", [(2 * K + 1, 1), (2 * K + 1, K), (2 * K + 1, K + 1), (4 * K, 300), (2 * K + 1, 0), (300, 301),
                                         (300, 0xffffffff)])
def test_a_live_count_below_the_capacity(scene, n_cap, n_in):
    """The rows beyond the live count hold NaNs of 0xff bytes that no result may show; a count word of 0 is 1, one beyond the
    capacity is the capacity."""
    N = min(max(n_in, 1), n_cap)
    rng = scene["scans"][2]
    poses = padded(cloud(scene, 2, N), n_cap)
    args = (MOTIONS[3], AMP, 0xfeedfacecafebeef, (1 << 40) + N, rng)
    want = expect(scene, poses, n_in, n_cap, *args)
    assert want["N"] == N and int(want["report"][16]) == N and not np.isnan(want["out"]).any() and int(want["report"][10]) == want["n_out"]
    if N >= 300:
        for_real(want)
        assert want["n_out"] == 3 * want["kbins"] < N
    same(launch(scene, poses, n_in, *args), want, f"n_cap = {n_cap}, *d_n_in = {n_in}")


# ---- 3. shrink and grow for real ----
@pytest.mark.parametrize("N, n_cap, table", [(300, 4 * K, "3k"), (300, 4 * K, "2^k"), (300, 4 * K, "ones"), (K + 1, 2 * K + 1, "2^k"),
                                             (K + 1, 2 * K + 1, "3k")])
def test_the_count_shrinks_and_grows(scene, N, n_cap, table):
    """tab[k] = 3 k shrinks the set, tab[k] = 2^k grows it -- at N = 1025 to the capacity, with ancestors from both scan blocks --,
    a table of ones leaves one pose.  The first cloud of at most 40 whose yardstick result is such a case."""
    ntab = {"3k": TAB3, "2^k": TAB_POW, "ones": np.ones(8, dtype=np.uint32)}[table]
    rng = scene["scans"][2]
    args = (MOTIONS[3], AMP, 0xfeedfacecafebeef, (1 << 40) + N, rng)
    for seed in range(40):
        poses = padded(cloud(scene, 2, N, seed=seed), n_cap)
        want = expect(scene, poses, N, n_cap, *args, ntab=ntab)
        k, A, n_out = want["kbins"], len(want["reference"]), want["n_out"]
        ok = 1 < k < A < N and n_out != N
        if table == "3k":
            ok = ok and n_out == 3 * k < N
        elif table == "ones":
            ok = ok and n_out == 1
        elif N > K:
            ok = ok and n_out == n_cap and want["ancestors"].min() < K <= want["ancestors"].max()
        else:
            ok = ok and N < n_out == min(1 << k, n_cap)
        if ok:
            break
    assert ok, (table, k, A, N, n_out)
    same(launch(scene, poses, N, *args, ntab=ntab), want, f"N = {N}, {table}")


# ---- 4. bins ----
def around(scene, k, cell, nx, ny, nth):
    """nx x ny bins of ``cell`` metres with pose k of the walk at their centre."""
    p = scene["poses"][k]
    return ada.Bins(p[0] - 0.5 * nx * cell, p[1] - 0.5 * ny * cell, cell, TWO_PI / nth, nx, ny, nth)


@pytest.mark.parametrize("name", ["large", "small", "1 x 1 x 1", "one heading", "64 bits", "65 bits"])
def test_bin_shapes(scene, name):
    N, n_cap = 200, 256
    rng = scene["scans"][4]
    args = (MOTIONS[0], AMP, 17, 18, rng)
    # (of 2, 3 or 5 heading bins, the count whose bin edges are farthest from the walk's heading at pose 4: the cloud stays inside one)
    edge = lambda nth: abs((scene["poses"][4][2] / (TWO_PI / nth)) % 1.0 - 0.5)
    bins = {"large": around(scene, 4, 4.0, 3, 3, min((2, 3, 5), key=edge)),
            "small": around(scene, 4, 0.001, 4096, 4096, 4), "1 x 1 x 1": ada.Bins(-8.0, -8.0, 16.0, TWO_PI, 1, 1, 1),
            "one heading": BINS._replace(nth=1, turn=TWO_PI), "64 bits": around(scene, 4, 0.1, 7, 3, 3), "65 bits": around(scene, 4, 0.1, 4, 4, 4)}[name]
    for seed in range(40):
        poses = padded(cloud(scene, 4, N, seed=seed), n_cap)
        want = expect(scene, poses, N, n_cap, *args, bins=bins)
        k, A = want["kbins"], len(want["reference"])
        outside = int((ada.bins_of(want["moved"][want["reference"]], bins) == bins.nx * bins.ny * bins.nth).sum())
        if name in ("large", "1 x 1 x 1"):
            ok = k == 1 < A and outside == 0
        elif name == "small":
            ok = k == A > 8 and outside == 0                   # 2^26 bins: every member of A in a bin of its own
        elif name == "one heading":
            ok = 1 < k < A and outside == 0
        else:                                                  # 63 bins + the outside one in one word; 64 bins, the outside one in a word of its own
            ok = 2 < k < A and 0 < outside < A
        if ok:
            break
    assert ok, (name, k, A, outside)
    assert want["n_out"] == min(3 * k, n_cap)
    same(launch(scene, poses, N, *args, bins=bins), want, name)


def test_degenerate_poses_share_the_outside_bin(scene):
    """tests/test_gpu_mcl.py's BAD poses among good ones under a flat table: every pose is in A, and every bad one -- not finite,
    beyond the guard or outside the window -- is in the one outside bin."""
    N, n_cap = 90, 128
    rng = scene["scans"][8]
    poses = cloud(scene, 8, N)
    where = np.arange(len(BAD)) * 6 + 2
    poses[where] = BAD
    poses = padded(poses, n_cap)
    args = (MOTIONS[0], AMP, 21, 22, rng)
    kw = dict(lut=np.array([5], dtype=np.uint32), shift=0)
    want = expect(scene, poses, N, n_cap, *args, **kw)
    b = ada.bins_of(want["moved"], BINS)
    n_bins = BINS.nx * BINS.ny * BINS.nth
    assert len(want["reference"]) == N and (b[where] == n_bins).all() and (np.delete(b, where) < n_bins).all()
    assert want["kbins"] == len(np.unique(np.delete(b, where))) + 1 > 2
    same(launch(scene, poses, N, *args, **kw), want, "bad poses")


def test_four_copies_of_one_pose_are_one_bin(scene):
    N, n_cap = 96, 100
    rng = scene["scans"][4]
    poses = cloud(scene, 4, N, spread=(0.3, 0.3, 0.2))
    bins = around(scene, 4, 0.001, 4096, 4096, 4)
    args = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0, 0, rng)
    kw = dict(lut=np.array([5], dtype=np.uint32), shift=0, bins=bins)
    alone = expect(scene, padded(poses, n_cap), N, n_cap, *args, **kw)
    assert alone["kbins"] == len(alone["reference"]) == N      # every pose in a bin of its own
    poses[[5, 40, 77, 95]] = poses[17]
    want = expect(scene, padded(poses, n_cap), N, n_cap, *args, **kw)
    assert len(want["reference"]) == N and want["kbins"] == N - 4
    same(launch(scene, padded(poses, n_cap), N, *args, **kw), want, "copies")


# ---- 5. W == 0 ----
@pytest.mark.parametrize("n_out", [150, 33])
def test_an_all_zero_weight_table(scene, n_out):
    """W == 0: A is every particle, a_j = j mod N, for more offspring than particles and for fewer."""
    N, n_cap = 70, 200
    rng = scene["scans"][7]
    poses = padded(cloud(scene, 7, N), n_cap)
    args = (MOTIONS[1], AMP, 8, 9, rng)
    kw = dict(lut=np.zeros(16, dtype=np.uint32), shift=5, ntab=[n_out])
    want = expect(scene, poses, N, n_cap, *args, **kw)
    assert [int(v) for v in want["report"][2:5]] == [0, 0, 0] and len(want["reference"]) == N == int(want["report"][19])
    assert np.array_equal(want["ancestors"], np.arange(n_out) % N) and int(want["report"][6]) == min(N, n_out) and want["n_out"] == n_out
    same(launch(scene, poses, N, *args, **kw), want, f"W = 0, N_out = {n_out}")


# ---- 6. chained, one count word ----
def test_three_chained_calls_share_one_count_word(scene):
    """Three calls enqueued with no synchronisation between them, one word as d_n_in and d_n_out, ping-pong buffers: the count
    goes from 2049 to a few hundred to a few dozen, as the yardstick's chain has it."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng, lv = scene["eng"], scene["lv"]
    n_cap = 2 * K + 1
    k = np.arange(4096)
    ntab = np.where(k >= 32, 12 * k, 2 * k).astype(np.uint32)   # a dozen per bin for a wide set (32 bins or more), two for a narrow one
    start = cloud(scene, 3, n_cap, spread=(0.1, 0.1, 0.05))
    wants, cur, n = [], start, n_cap
    for i in range(3):
        want = expect(scene, padded(cur, n_cap), n, n_cap, MOTIONS[i], AMP, 99, 40 + i, scene["scans"][3 + i], ntab=ntab)
        wants.append(want)
        cur, n = want["out"], want["n_out"]
    counts = [w["n_out"] for w in wants]
    assert n_cap > counts[0] >= 100 > counts[2] >= 12 and counts[0] > counts[1], counts
    full = lambda shape, dt: torch.full(shape, -1, dtype=dt, device=eng.device)
    bufs = [eng.to_device(padded(start, n_cap)), full((n_cap, 3), torch.int64).view(torch.float64)]
    d_n = torch.full((1,), n_cap, dtype=torch.int32, device=eng.device)
    d_rng = eng.to_device(scene["scans"][3:6])
    d_lut = torch.from_numpy(scene["lut"].view(np.int32).copy()).to(eng.device)
    d_ntab = torch.from_numpy(ntab.view(np.int32).copy()).to(eng.device)
    d_rep, d_anc = full((3, _lib.MCL_ADAPT_REPORT), torch.int64), full((3, n_cap), torch.int32)
    for i in range(3):                                         # (enqueued back to back: nothing is downloaded in between)
        eng.mcl_step_adaptive(lv, 0, bufs[i & 1], bufs[1 - (i & 1)], n_cap, d_n, MOTIONS[i], AMP, 99, 40 + i, d_rng[i], scene["free"], d_lut,
                              scene["shift"], c_bins(BINS), d_ntab, d_rep[i], d_anc[i])
    rep, anc = d_rep.cpu().numpy().view(np.uint64), d_anc.cpu().numpy()
    for i, want in enumerate(wants):
        assert np.array_equal(rep[i], want["report"]), (i, [hex(v) for v in rep[i]], [hex(v) for v in want["report"]])
        assert np.array_equal(anc[i][:want["n_out"]], want["ancestors"]) and (anc[i][want["n_out"]:] == -1).all(), i
    assert int(d_n.cpu()[0]) == counts[2]
    last = bufs[1].cpu().numpy().view(np.uint64)               # (the third call wrote where the first did)
    assert np.array_equal(last[:counts[2]], np.ascontiguousarray(wants[2]["out"]).view(np.uint64))
    assert np.array_equal(last[counts[2]:counts[0]], np.ascontiguousarray(wants[0]["out"]).view(np.uint64)[counts[2]:])
    assert (last[counts[0]:] == POISON).all()


# ---- 7. stride, no ancestors ----
def test_a_pose_stride_of_five_and_no_ancestors(scene):
    N, n_cap = 77, 90
    rng = scene["scans"][9]
    poses = padded(cloud(scene, 9, N), n_cap, stride=5)
    poses[:N, 3:] = 123.0
    args = (MOTIONS[2], AMP, 31, 32, rng)
    want = expect(scene, poses, N, n_cap, *args)
    assert want["n_out"] not in (1, N, n_cap)
    got = launch(scene, poses, N, *args)
    assert got["out"].shape == (n_cap, 5)
    same(got, want, "stride 5")                                # (slots 3 and 4 of every row: as they were)
    none = launch(scene, poses, N, *args, ancestor=False)
    assert none["ancestors"] is None
    same(none, want, "d_ancestor = NULL")


# ---- 8. the Localiser ----
def readings_of(scene):
    phi, true = 0.1, scene["poses"]                            # raw odometry: the walk in a frame of its own (turned and shifted)
    raw = np.column_stack([math.cos(phi) * true[:, 0] - math.sin(phi) * true[:, 1] + 0.4,
                           math.sin(phi) * true[:, 0] + math.cos(phi) * true[:, 1] - 0.3, true[:, 2] + phi])
    return [dict(x=float(p[0]), y=float(p[1]), theta=float(p[2]), range=list(map(float, r))) for p, r in zip(raw, scene["scans"])]


def test_adaptive_localiser_run_against_the_chain(pkg, scene):
    """Localiser(adaptive=...).run on four scans is the chain of engine calls on the same inputs and the yardstick's chain; the
    count and the shape of poses() follow; step() continues it."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    cap, S = 700, 4
    readings = readings_of(scene)
    sigma = (0.03, 0.02, 0.015)
    opt = dict(n_min=20, bin_xy=0.1, bin_theta=math.radians(10), epsilon=0.3, z=1.0)
    loc = pkg.Localiser(scene["sm"], WINDOW, particles=cap, sigma=sigma, temperature=TEMPERATURE, seed=5, adaptive=opt)
    assert np.array_equal(loc.level.field_cost(0), scene["field"]) and loc.count == cap
    b = loc.bins
    bins = ada.Bins(b.x0, b.y0, b.cell, b.turn, b.nx, b.ny, b.nth)
    assert bins == ada.Bins(-8.0, -8.0, 0.1, TWO_PI / 36, 160, 160, 36)
    ntab = engine.kld_table(0.3, 1.0, 20, cap)
    assert np.array_equal(loc.ntab, ntab) and ntab[0] == 20 and ntab.max() == cap
    start = loc.seed_at(scene["poses"][0], (0.05, 0.05, 0.03), count=600)
    assert start.shape == (600, 3) and loc.count == 600 and np.array_equal(loc.poses(), start)
    reports = loc.run(readings[:S])
    final = loc.poses()
    # the chain through ParticleEngine.mcl_step_adaptive, and the yardstick's
    eng, lv = loc.eng, loc.level
    amp = [v / math.sqrt(4.0 / 3.0) for v in sigma]
    bufs = [eng.to_device(padded(start, cap)), torch.full((cap, 3), -1, dtype=torch.int64, device=eng.device).view(torch.float64)]
    d_n = torch.full((1,), 600, dtype=torch.int32, device=eng.device)
    d_rep = torch.empty(24, dtype=torch.int64, device=eng.device)
    d_lut = torch.from_numpy(scene["lut"].view(np.int32).copy()).to(eng.device)
    d_ntab = torch.from_numpy(ntab.view(np.int32).copy()).to(eng.device)
    cur, n, counts = start, 600, []
    for i in range(S):
        motion = localise.odometry_motion(readings[i - 1], readings[i]) if i else (0.0, 0.0, 0.0)
        eng.mcl_step_adaptive(lv, 0, bufs[i & 1], bufs[1 - (i & 1)], cap, d_n, motion, amp, 5, i, eng.to_device(scene["scans"][i]), scene["free"],
                              d_lut, scene["shift"], c_bins(bins), d_ntab, d_rep)
        want = expect(scene, padded(cur, cap), n, cap, motion, amp, 5, i, scene["scans"][i], bins=bins, ntab=ntab)
        cur, n = want["out"], want["n_out"]
        counts.append(n)
        words = d_rep.cpu().numpy().view(np.uint64)
        assert np.array_equal(words, want["report"]), i
        assert reports[i] == engine.mcl_adapt_report_host(words) and reports[i]["n_out"] == n, i
        assert np.array_equal(bufs[1 - (i & 1)].cpu().numpy().view(np.uint64)[:n], np.ascontiguousarray(cur).view(np.uint64)), i
        assert int(d_n.cpu()[0]) == n
    assert len(set(counts)) > 1 and all(20 <= c < cap for c in counts), counts       # (the count moves, within the table's range)
    assert loc.count == n and final.shape == (n, 3)
    assert np.array_equal(final.view(np.uint64), np.ascontiguousarray(cur).view(np.uint64))
    # one more scan through step(): one call, the report decoded
    motion = localise.odometry_motion(readings[S - 1], readings[S])
    est = loc.step(readings[S], motion)
    want = expect(scene, padded(cur, cap), n, cap, motion, amp, 5, S, scene["scans"][S], bins=bins, ntab=ntab)
    assert est["mean_pose"] == mcl.mean_pose(want["report"][:16]) and (est["n_in"], est["n_out"]) == (n, want["n_out"])
    assert (est["bins"], est["reference_distinct"]) == (want["kbins"], len(want["reference"]))
    assert loc.count == want["n_out"] and np.array_equal(loc.poses().view(np.uint64), np.ascontiguousarray(want["out"]).view(np.uint64))
    x, y, th = est["mean_pose"]
    assert math.hypot(x - scene["poses"][S][0], y - scene["poses"][S][1]) < 0.15     # (it tracks: the walk's true pose)
    # the seedings take any count from 1 to the capacity and set the word
    assert loc.seed_uniform(count=1).shape == (1, 3) and loc.count == 1 and loc.poses().shape == (1, 3)
    u = loc.seed_uniform()
    assert u.shape == (cap, 3) and loc.count == cap and np.abs(u[:, :2]).max() <= 8.0
    p = loc.seed_from_peaks([(1.0, 2.0, 0.5), (-3.0, 0.5, -1.0)], 0.1, count=31)
    assert p.shape == (31, 3) and loc.count == 31
    assert loc.set_poses(np.zeros((5, 3))).shape == (5, 3) and loc.count == 5
    for bad in (0, cap + 1):
        with pytest.raises(ValueError):
            loc.seed_uniform(count=bad)
    with pytest.raises(ValueError):
        loc.set_poses(np.zeros((cap + 1, 3)))
    with pytest.raises(ValueError):
        pkg.Localiser(scene["sm"], WINDOW, particles=64, adaptive=dict(bins=3))


def test_adaptive_none_is_the_localiser_as_it_was(pkg, scene):
    """Localiser(adaptive=None) and Localiser() run the plain step: the same reports, sixteen words each, and the same poses, which
    are the plain yardstick's chain."""
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    N, S = 130, 2
    readings = readings_of(scene)
    sigma = (0.03, 0.02, 0.015)
    runs = []
    for kw in (dict(), dict(adaptive=None)):
        loc = pkg.Localiser(scene["sm"], WINDOW, particles=N, sigma=sigma, temperature=TEMPERATURE, seed=5, **kw)
        start = loc.seed_at(scene["poses"][0], (0.05, 0.05, 0.03))
        assert loc.adaptive is None and loc.count == N and loc.d_report.numel() == 16
        runs.append((start, loc.run(readings[:S]), loc.poses()))
        with pytest.raises(ValueError):
            loc.seed_uniform(count=N - 1)                      # (a set of fixed size)
        with pytest.raises(ValueError):
            loc.set_poses(np.zeros((N - 1, 3)))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])
    amp = [v / math.sqrt(4.0 / 3.0) for v in sigma]
    cur = runs[0][0]
    for i in range(S):
        motion = localise.odometry_motion(readings[i - 1], readings[i]) if i else (0.0, 0.0, 0.0)
        want = mcl.step(scene["field"], scene["frame"], scene["lv"].c.cost_scale, scene["lv"].step, cur, motion, amp, 5, i, scene["scans"][i], FOV, R,
                        scene["free"], scene["lut"], scene["shift"], scene["sincos"])
        assert "n_out" not in runs[1][1][i] and runs[1][1][i]["W"] == int(want["report"][2]) and runs[1][1][i]["distinct"] == int(want["report"][6])
        cur = want["out"]
    assert runs[1][2].shape == (N, 3) and np.array_equal(runs[1][2].view(np.uint64), np.ascontiguousarray(cur).view(np.uint64))


# ---- 9. determinism ----
def test_same_bits_on_every_call(scene):
    N, n_cap = 200, 333
    poses, rng = padded(cloud(scene, 5, N), n_cap), scene["scans"][5]
    a = launch(scene, poses, N, MOTIONS[2], AMP, 11, 22, rng)
    b = launch(scene, poses, N, MOTIONS[2], AMP, 11, 22, rng)
    for key in ("out", "ancestors", "report"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["n_out"] == b["n_out"]
    want = expect(scene, poses, N, n_cap, MOTIONS[2], AMP, 11, 22, rng)
    for_real(want)
    same(a, want, "poisoned buffers")
