"""What ParticleEngine's seven localisation wrappers hand to the library, without a GPU: score_poses, search_lattice, refine_poses,
search_points, refine_points, mcl_step and mcl_step_adaptive run on an engine made without its constructor, on CPU tensors, against a
recorder in the library's place.  The recorder forwards the ``*_work`` sizes to the real library (host-only) and writes every other
call down instead of making it: each argument's value and type, each pointer, the kept scratch, every refusal and the returned
tensors are pinned here; the decode round trips are tests/test_{refine,search,score,mcl,mcl_adapt,points}_host.py's."""
import ctypes
import importlib
import math
import types

import numpy as np
import pytest
import torch

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")

B, P, N, M = 60, 3, 5, 7
LAT = (5, 4, 8, 1, 0.1, 2, 0.2, -3, 0.25)                      # nx ny nth x0 dx y0 dy th0 dth, whole numbers among them
LAT_ARGS = [5, 4, 8, 1.0, 0.1, 2.0, 0.2, -3.0, 0.25]
N_CAP = 98
MASK = 0xffffffffffffffff
_REF = type(ctypes.byref(ctypes.c_int()))
f64, i64, i32 = torch.float64, torch.int64, torch.int32


class Recorder:
    """The library's stand-in: the work sizes are the real ones, every other call is recorded and answered with ``rc``."""

    def __init__(self, real):
        self.real, self.calls, self.rc = real, [], 0

    def __getattr__(self, name):
        if name.endswith("_work"):
            return getattr(self.real, name)

        def call(*args):
            self.calls.append((name, args))
            return self.rc
        return call


@pytest.fixture
def eng(monkeypatch):
    _lib.build_library()
    monkeypatch.setattr(engine, "_PINNED_STREAM", ctypes.c_void_p(0))          # no CUDA stream is looked up
    e = object.__new__(engine.ParticleEngine)
    e.device = torch.device("cpu")
    e.lidar_c = _lib.Slam2dLidar(unit=0.1, max_range=4.0, fov=math.pi, beams=B)
    e.L = Recorder(_lib.lib())
    return e


@pytest.fixture
def level():
    return types.SimpleNamespace(P=P, c=_lib.Slam2dLevel())


def zeros(n, dtype=f64):
    return torch.zeros(n, dtype=dtype)


def _value(a):
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    if isinstance(a, _REF):
        return a._obj
    if isinstance(a, ctypes.Array):
        return list(a)
    return a


def the_call(eng, name):
    """The arguments of the one call recorded since the last look: pointers as integers, references as their objects."""
    assert [c[0] for c in eng.L.calls] == [name]
    args = [_value(a) for a in eng.L.calls[0][1]]
    eng.L.calls.clear()
    return args


def same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, ctypes.Structure):
            assert g is w, i
        else:
            assert type(g) is type(w) and g == w, (i, g, w)
            if isinstance(w, list):
                assert all(type(v) is float for v in g), (i, g)


def refused(eng, exc, match, fn, *args, **kw):
    with pytest.raises(exc, match=match):
        fn(*args, **kw)
    assert eng.L.calls == []


def slots_refused(eng, level, call):
    """``call(p_field)`` with slot -1 and slot P."""
    for p in (-1, P):
        refused(eng, ValueError, f"field slot {p} of a level of {P}", call, p)


def library_refuses(eng, name, call):
    eng.L.rc = -1
    with pytest.raises(_lib.Slam2dError, match=name + ": argument error -1"):
        call()
    assert [c[0] for c in eng.L.calls] == [name]
    eng.L.calls.clear()
    eng.L.rc = 0


def scratch_grows(eng, attr, name, work_at, sizes, call):
    """``call(k)`` at a large, a smaller and a larger size ``sizes[k]`` words: the scratch is kept, kept, then a new one."""
    ptrs = []
    for k, n in enumerate(sizes):
        call(k)
        ptrs.append(the_call(eng, name)[work_at])
        w = getattr(eng, attr)
        assert ptrs[-1] == w.data_ptr() and w.dtype == i64 and w.dim() == 1 and w.device.type == "cpu"
        assert w.numel() == max(sizes[:k + 1])
    assert sizes[1] < sizes[0] < sizes[2] and ptrs[1] == ptrs[0] != ptrs[2]


# ---- slam2d_score_poses ----
@pytest.mark.parametrize("pose_stride", [3, 5])
@pytest.mark.parametrize("per_pose", [False, True])
def test_score_poses(eng, level, pose_stride, per_pose):
    d_pose, d_rng = zeros(N * pose_stride), zeros(N * B if per_pose else B)
    out = eng.score_poses(level, 1, d_pose, pose_stride, N, d_rng, B if per_pose else 0)
    assert out.shape == (N, _lib.SCORE_STRIDE) and out.dtype == f64 and out.device.type == "cpu"
    same(the_call(eng, "slam2d_score_poses"),
         [eng.lidar_c, level.c, 1, N, d_pose.data_ptr(), pose_stride, d_rng.data_ptr(), B if per_pose else 0, out.data_ptr(), 0])
    slots_refused(eng, level, lambda p: eng.score_poses(level, p, d_pose, pose_stride, N, d_rng, 0))
    library_refuses(eng, "slam2d_score_poses", lambda: eng.score_poses(level, 0, d_pose, pose_stride, N, d_rng, 0))


# ---- slam2d_search_lattice / slam2d_search_points ----
def test_search_lattice(eng, level):
    d_rng = zeros(B)
    out = eng.search_lattice(level, 2, LAT, d_rng, np.int64(1234))
    assert out.shape == (4, 5) and out.dtype == i64 and out.device.type == "cpu"
    work = eng._search_work
    assert work.numel() == 2 * 8 * B and work.dtype == i64
    same(the_call(eng, "slam2d_search_lattice"), [eng.lidar_c, level.c, 2] + LAT_ARGS + [d_rng.data_ptr(), 1234, work.data_ptr(), out.data_ptr(), 0])
    lat = lambda nth: engine.Lattice(*LAT)._replace(nth=nth)
    scratch_grows(eng, "_search_work", "slam2d_search_lattice", 14, [2 * 8 * B, 2 * 3 * B, 2 * 9 * B],
                  lambda k: eng.search_lattice(level, 0, lat((8, 3, 9)[k]), d_rng, 0))
    slots_refused(eng, level, lambda p: eng.search_lattice(level, p, LAT, d_rng, 0))
    refused(eng, _lib.Slam2dError, "slam2d_search_lattice_work: argument error -1", eng.search_lattice, level, 0, lat(0), d_rng, 0)
    library_refuses(eng, "slam2d_search_lattice", lambda: eng.search_lattice(level, 0, LAT, d_rng, 0))


@pytest.mark.parametrize("point_stride", [2, 3])
def test_search_points(eng, level, point_stride):
    d_pts = zeros((M - 1) * point_stride + 2)
    kw = {} if point_stride == 2 else dict(point_stride=np.int64(point_stride))
    out = eng.search_points(level, 1, LAT, d_pts, np.int64(M), np.int64(77), **kw)
    assert out.shape == (4, 5) and out.dtype == i64 and out.device.type == "cpu"
    work = eng._search_work
    assert work.numel() == 2 * 8 * M and work.dtype == i64
    same(the_call(eng, "slam2d_search_points"),
         [level.c, 1] + LAT_ARGS + [d_pts.data_ptr(), point_stride, M, 77, work.data_ptr(), out.data_ptr(), 0])
    big = zeros(40 * point_stride)
    scratch_grows(eng, "_search_work", "slam2d_search_points", 15, [2 * 8 * M, 2 * 8 * 2, 2 * 8 * 9],
                  lambda k: eng.search_points(level, 0, LAT, big, (M, 2, 9)[k], 0, **kw))
    slots_refused(eng, level, lambda p: eng.search_points(level, p, LAT, d_pts, M, 0, **kw))
    refused(eng, ValueError, f"want {M} points, 1 doubles apart", eng.search_points, level, 0, LAT, d_pts, M, 0, point_stride=1)
    refused(eng, ValueError, f"want {M} points, {point_stride} doubles apart", eng.search_points, level, 0, LAT, d_pts[:-1], M, 0, **kw)
    refused(eng, _lib.Slam2dError, "slam2d_search_points_work: argument error -1", eng.search_points, level, 0, LAT, d_pts, 0, 0, **kw)
    library_refuses(eng, "slam2d_search_points", lambda: eng.search_points(level, 0, LAT, d_pts, M, 0, **kw))


def test_the_searches_share_one_scratch(eng, level):
    eng.search_lattice(level, 0, LAT, zeros(B), 0)
    first = the_call(eng, "slam2d_search_lattice")[14]
    eng.search_points(level, 0, LAT, zeros(2 * M), M, 0)                       # 2 * 8 * 7 words: fits the lattice's 2 * 8 * 60
    assert the_call(eng, "slam2d_search_points")[15] == first == eng._search_work.data_ptr()
    eng.search_points(level, 0, LAT, zeros(2 * 100), 100, 0)                   # ... and 2 * 8 * 100 do not
    grown = the_call(eng, "slam2d_search_points")[15]
    eng.search_lattice(level, 0, LAT, zeros(B), 0)
    assert the_call(eng, "slam2d_search_lattice")[14] == grown != first


# ---- slam2d_refine_poses / slam2d_refine_points ----
RADII, STEPS = (np.int64(3), 2.0, 1), (1, 0.05, np.float32(0.5))
REFINE_TAIL = [3, 2, 1, 1.0, 0.05, 0.5]


@pytest.mark.parametrize("pose_stride", [3, 5])
@pytest.mark.parametrize("per_seed", [False, True])
def test_refine_poses(eng, level, pose_stride, per_seed):
    need = (N - 1) * pose_stride + 3
    d_in, d_out, d_rng = zeros(need), zeros(need), zeros(N * B if per_seed else B)
    rs = B if per_seed else 0
    out = eng.refine_poses(level, 1, d_in, d_out, N, pose_stride, d_rng, rs, RADII, STEPS, np.int64(9))
    assert out.shape == (N, _lib.REFINE_STRIDE) and out.dtype == i64 and out.device.type == "cpu"
    work = eng._refine_work
    assert work.numel() == 3 * N and work.dtype == i64
    same(the_call(eng, "slam2d_refine_poses"), [eng.lidar_c, level.c, 1, N, d_in.data_ptr(), d_out.data_ptr(), pose_stride, d_rng.data_ptr(), rs,
                                               None] + REFINE_TAIL + [9, work.data_ptr(), out.data_ptr(), 0])
    words = zeros((3, N, _lib.REFINE_STRIDE), i64)[1]
    assert eng.refine_poses(level, 0, d_in, d_out, N, pose_stride, d_rng, rs, RADII, STEPS, 9, motion=(1, 0.25, -0.5), d_words=words) is words
    got = the_call(eng, "slam2d_refine_poses")
    assert got[9] == [1.0, 0.25, -0.5] and all(type(v) is float for v in got[9]) and got[17:19] == [work.data_ptr(), words.data_ptr()]
    call = lambda p=0, a=d_in, b=d_out, n=N, **kw: eng.refine_poses(level, p, a, b, n, pose_stride, d_rng, rs, RADII, STEPS, 9, **kw)
    slots_refused(eng, level, call)
    pair = f"want two buffers of {N} poses, {pose_stride} doubles apart"
    refused(eng, ValueError, pair, call, a=d_in[:-1])
    refused(eng, ValueError, pair, call, b=d_out[:-1])
    refused(eng, ValueError, f"d_words wants {N} x 2 64-bit words", call, d_words=zeros(2 * N - 1, i64))
    refused(eng, ValueError, f"d_words wants {N} x 2 64-bit words", call, d_words=zeros(2 * N, i32))
    refused(eng, _lib.Slam2dError, "slam2d_refine_work: argument error -1", call, n=0)
    library_refuses(eng, "slam2d_refine_poses", call)


@pytest.mark.parametrize("pose_stride", [3, 5])
@pytest.mark.parametrize("point_stride", [2, 3])
@pytest.mark.parametrize("per_seed", [False, True])
def test_refine_points(eng, level, pose_stride, point_stride, per_seed):
    need = (N - 1) * pose_stride + 3
    set_stride = M * point_stride if per_seed else 0
    d_in, d_out, d_pts = zeros(need), zeros(need), zeros((N - 1) * set_stride + (M - 1) * point_stride + 2)
    kw = {} if point_stride == 2 else dict(point_stride=np.int64(point_stride))
    out = eng.refine_points(level, 2, d_in, d_out, N, pose_stride, d_pts, np.int64(M), np.int64(set_stride), RADII, STEPS, np.int64(9), **kw)
    assert out.shape == (N, _lib.REFINE_STRIDE) and out.dtype == i64 and out.device.type == "cpu"
    work = eng._refine_work
    assert work.numel() == 3 * N and work.dtype == i64
    same(the_call(eng, "slam2d_refine_points"), [level.c, 2, N, d_in.data_ptr(), d_out.data_ptr(), pose_stride, d_pts.data_ptr(), point_stride, M,
                                                set_stride, None] + REFINE_TAIL + [9, work.data_ptr(), out.data_ptr(), 0])
    words = zeros((3, N, _lib.REFINE_STRIDE), i64)[2]
    assert eng.refine_points(level, 0, d_in, d_out, N, pose_stride, d_pts, M, set_stride, RADII, STEPS, 9, (1, 0.25, -0.5), words, **kw) is words
    got = the_call(eng, "slam2d_refine_points")
    assert got[10] == [1.0, 0.25, -0.5] and all(type(v) is float for v in got[10]) and got[18:20] == [work.data_ptr(), words.data_ptr()]

    def call(p=0, a=d_in, b=d_out, n=N, pts=d_pts, m=M, **more):
        return eng.refine_points(level, p, a, b, n, pose_stride, pts, m, set_stride, RADII, STEPS, 9, **{**kw, **more})
    slots_refused(eng, level, call)
    pair = f"want two buffers of {N} poses, {pose_stride} doubles apart"
    refused(eng, ValueError, pair, call, a=d_in[:-1])
    refused(eng, ValueError, pair, call, b=d_out[:-1])
    refused(eng, ValueError, f"want {M} points, {point_stride} doubles apart, sets {set_stride} apart", call, pts=d_pts[:-1])
    refused(eng, ValueError, f"want {M} points, 1 doubles apart", call, point_stride=1)
    refused(eng, ValueError, "want 0 points", call, m=0)
    refused(eng, ValueError, f"d_words wants {N} x 2 64-bit words", call, d_words=zeros(2 * N - 1, i64))
    refused(eng, ValueError, f"d_words wants {N} x 2 64-bit words", call, d_words=zeros(2 * N, i32))
    refused(eng, _lib.Slam2dError, "slam2d_refine_work: argument error -1", call, n=0)
    library_refuses(eng, "slam2d_refine_points", call)


def test_the_refinements_share_one_scratch(eng, level):
    poses = lambda n: (zeros(3 * n), zeros(3 * n), n, 3)
    scratch_grows(eng, "_refine_work", "slam2d_refine_poses", 17, [3 * N, 3 * 2, 3 * 11],
                  lambda k: eng.refine_poses(level, 0, *poses((N, 2, 11)[k]), zeros(B), 0, RADII, STEPS, 0))
    first = eng._refine_work.data_ptr()
    eng.refine_points(level, 0, *poses(N), zeros(2 * M), M, 0, RADII, STEPS, 0)
    assert the_call(eng, "slam2d_refine_points")[18] == first
    scratch_grows(eng, "_refine_work", "slam2d_refine_points", 18, [3 * 12, 3 * 2, 3 * 13],
                  lambda k: eng.refine_points(level, 0, *poses((12, 2, 13)[k]), zeros(2 * M), M, 0, RADII, STEPS, 0))
    grown = eng._refine_work.data_ptr()
    eng.refine_poses(level, 0, *poses(N), zeros(B), 0, RADII, STEPS, 0)
    assert the_call(eng, "slam2d_refine_poses")[17] == grown != first


# ---- slam2d_mcl_step / slam2d_mcl_step_adaptive ----
MOTION, AMP = (1, 0.25, -0.5), (np.float32(0.5), 2, 0.125)
MOTION_ARGS, AMP_ARGS = [1.0, 0.25, -0.5], [0.5, 2.0, 0.125]


def mcl_buffers(n, stride):
    shape = (n, stride) if stride != 3 else (3 * n,)                          # one dimension: three doubles per pose
    return torch.zeros(shape, dtype=f64), torch.zeros(shape, dtype=f64)


@pytest.mark.parametrize("stride", [3, 5])
@pytest.mark.parametrize("ancestor", [False, True])
def test_mcl_step(eng, level, stride, ancestor):
    d_in, d_out = mcl_buffers(N, stride)
    d_rng, d_lut, d_rep = zeros(B), zeros(4096, i32), zeros(_lib.MCL_REPORT, i64)
    d_anc = zeros(N, i32) if ancestor else None
    assert eng.mcl_step(level, 1, d_in, d_out, N, MOTION, AMP, -1, 2 ** 64 + 5, d_rng, np.int64(9), d_lut, np.int64(7), d_rep, d_anc) is None
    work = eng._mcl_work
    assert work.numel() == 5 * N + 1032 and work.dtype == i64
    same(the_call(eng, "slam2d_mcl_step"),
         [eng.lidar_c, level.c, 1, N, d_in.data_ptr(), d_out.data_ptr(), stride, MOTION_ARGS, AMP_ARGS, MASK, 5, d_rng.data_ptr(), 9,
          d_lut.data_ptr(), 4096, 7, d_anc.data_ptr() if ancestor else 0, work.data_ptr(), d_rep.data_ptr(), 0])
    call = lambda p=0, a=d_in, b=d_out, n=N, rep=d_rep, anc=d_anc: eng.mcl_step(level, p, a, b, n, MOTION, AMP, 1, 2, d_rng, 9, d_lut, 7, rep, anc)
    scratch_grows(eng, "_mcl_work", "slam2d_mcl_step", 17, [5 * N + 1032, 5 * 2 + 1032, 5 * 9 + 1032],
                  lambda k: call(0, *mcl_buffers((N, 2, 9)[k], stride), (N, 2, 9)[k], d_rep, None))
    slots_refused(eng, level, call)
    pair = f"want two buffers of {N} poses of one row length"
    refused(eng, ValueError, pair, call, a=d_in[:-1])
    refused(eng, ValueError, pair, call, b=d_out[:-1])
    refused(eng, ValueError, pair, call, b=torch.zeros((N, 4), dtype=f64))
    refused(eng, ValueError, "d_report wants 16 words, d_ancestor N", call, rep=d_rep[:-1])
    refused(eng, ValueError, "d_report wants 16 words, d_ancestor N", call, anc=zeros(N - 1, i32))
    refused(eng, _lib.Slam2dError, "slam2d_mcl_work: argument error -1", call, n=0)
    library_refuses(eng, "slam2d_mcl_step", call)


@pytest.mark.parametrize("stride", [3, 5])
@pytest.mark.parametrize("ancestor", [False, True])
@pytest.mark.parametrize("count_out", [False, True])
def test_mcl_step_adaptive(eng, level, stride, ancestor, count_out):
    d_in, d_out = mcl_buffers(N_CAP, stride)
    d_rng, d_lut, d_ntab, d_rep = zeros(B), zeros(4096, i32), zeros(300, i32), zeros(_lib.MCL_ADAPT_REPORT, i64)
    d_count, d_cout = zeros(1, i32), zeros(1, i32) if count_out else None
    d_anc = zeros(N_CAP, i32) if ancestor else None
    bins = _lib.Slam2dMclBins(x0=-1.0, y0=-1.0, cell=0.5, turn=2 * math.pi / 5, nx=4, ny=4, nth=5)
    base = 5 * N_CAP + 1032 + (4 * 4 * 5 + 64) // 64 + 8                       # include/slam2d.h: slam2d_mcl_adapt_work

    def call(p=0, a=d_in, b=d_out, n=N_CAP, cnt=d_count, rep=d_rep, anc=d_anc, cout=d_cout, bins=bins):
        return eng.mcl_step_adaptive(level, p, a, b, n, cnt, MOTION, AMP, -1, 2 ** 64 + 5, d_rng, np.int64(9), d_lut, np.int64(7), bins, d_ntab, rep,
                                     anc, cout)
    assert call(1) is None
    work = eng._mcl_adapt_work
    assert work.numel() == base and work.dtype == i64
    same(the_call(eng, "slam2d_mcl_step_adaptive"),
         [eng.lidar_c, level.c, 1, N_CAP, d_count.data_ptr(), (d_cout if count_out else d_count).data_ptr(), d_in.data_ptr(), d_out.data_ptr(),
          stride, MOTION_ARGS, AMP_ARGS, MASK, 5, d_rng.data_ptr(), 9, d_lut.data_ptr(), 4096, 7, bins, d_ntab.data_ptr(), 300,
          d_anc.data_ptr() if ancestor else 0, work.data_ptr(), d_rep.data_ptr(), 0])
    caps = (N_CAP, 2, N_CAP + 3)
    scratch_grows(eng, "_mcl_adapt_work", "slam2d_mcl_step_adaptive", 22, [base + 5 * (c - N_CAP) for c in caps],
                  lambda k: call(0, *mcl_buffers(caps[k], stride), caps[k], anc=None))
    assert not hasattr(eng, "_mcl_work")                                       # (the two steps keep a scratch each)
    slots_refused(eng, level, call)
    pair = f"want two buffers of {N_CAP} poses of one row length"
    refused(eng, ValueError, pair, call, a=d_in[:-1])
    refused(eng, ValueError, pair, call, b=d_out[:-1])
    refused(eng, ValueError, pair, call, b=torch.zeros((N_CAP, 4), dtype=f64))
    refused(eng, ValueError, "d_report wants 24 words, d_ancestor n_cap", call, rep=d_rep[:-1])
    refused(eng, ValueError, "d_report wants 24 words, d_ancestor n_cap", call, anc=zeros(N_CAP - 1, i32))
    refused(eng, ValueError, "d_count wants one 32-bit word", call, cnt=zeros(1, i64))
    refused(eng, ValueError, "d_count wants one 32-bit word", call, cout=zeros(1, torch.int16))
    refused(eng, ValueError, "d_count wants one 32-bit word", call, cnt=zeros(0, i32))
    refused(eng, _lib.Slam2dError, "slam2d_mcl_adapt_work: argument error -1", call, n=0)
    refused(eng, _lib.Slam2dError, "slam2d_mcl_adapt_work: argument error -1", call, bins=_lib.Slam2dMclBins())
    library_refuses(eng, "slam2d_mcl_step_adaptive", call)


# ---- the decoders' one definition ----
def test_refine_host_has_one_definition():
    words = np.array([[(17 << 20) | 3, 40], [(5 << 20) | 0, 5]], dtype=np.uint64)
    a = engine.refine_host(words, (1, 1, 0), (0.1, 0.1, 0.01), 4.0)
    b = engine.ParticleEngine.refine_host(torch.from_numpy(words.view(np.int64)), (1, 1, 0), (0.1, 0.1, 0.01), 4.0)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert a["cost"].tolist() == [17, 5] and a["index"].tolist() == [3, 0] and a["moved"].tolist() == [True, False]
