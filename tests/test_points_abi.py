"""slam2d_search_points / slam2d_search_points_work / slam2d_refine_points at the C ABI, without a GPU: exported and bound, the
header's declarations, the work sizes, every argument error refused before any HIP call (a NULL stream and fake pointers: a call
that returns has made none), and the accepted edges shown on the checks that come before the sizes.  No kernel is launched."""
import ctypes
import importlib
import os
import re

import pytest

from conftest import REPO

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

FAKE, FAKE2 = 4096, 8192                                       # never dereferenced: every call below is refused first
NAN, INF = float("nan"), float("inf")
NAMES = ("slam2d_search_points", "slam2d_search_points_work", "slam2d_refine_points")


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _level(**kw):
    d = dict(step=0.1, reach=14.4, cost_scale=float(2 ** 28), fmax=290, fpitch=304, field=FAKE, frames=FAKE)
    d.update(kw)
    return _lib.Slam2dLevel(**d)


BIG = dict(fmax=23200, fpitch=23200)                           # an image beyond slam2d_field_build's own limit


def _vp(v):
    return None if v is None else ctypes.c_void_p(v)


def _search(L, level="ok", p_field=0, nx=9, ny=7, nth=5, x0=0.0, dx=0.1, y0=0.0, dy=0.1, th0=0.0, dth=0.2, d_points=FAKE, point_stride=2,
            M=60, outside_cost=1000, d_work=FAKE, d_out=FAKE):
    lv = _level() if level == "ok" else level
    return L.slam2d_search_points(None if lv is None else ctypes.byref(lv), p_field, nx, ny, nth, x0, dx, y0, dy, th0, dth, _vp(d_points),
                                  point_stride, M, outside_cost, _vp(d_work), _vp(d_out), None)


def _refine(L, level="ok", p_field=0, N=5, d_pose_in=FAKE, d_pose_out=FAKE2, pose_stride=3, d_points=FAKE, point_stride=2, M=60, set_stride=0,
            motion=None, rx=3, ry=2, rt=2, dx=0.07, dy=0.05, dth=0.013, outside_cost=1000, d_work=FAKE, d_out=FAKE):
    lv = _level() if level == "ok" else level
    return L.slam2d_refine_points(None if lv is None else ctypes.byref(lv), p_field, N, _vp(d_pose_in), _vp(d_pose_out), pose_stride,
                                  _vp(d_points), point_stride, M, set_stride, None if motion is None else (ctypes.c_double * 3)(*motion),
                                  rx, ry, rt, dx, dy, dth, outside_cost, _vp(d_work), _vp(d_out), None)


CALLS = pytest.mark.parametrize("call", [_search, _refine], ids=["search", "refine"])


def test_symbols_exported_and_bound(L):
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert L.slam2d_search_points_work.restype is ctypes.c_int64
    assert L.slam2d_search_points.restype is ctypes.c_int and L.slam2d_refine_points.restype is ctypes.c_int
    assert L.slam2d_abi_version() == 18                        # added symbols: the ABI number stays


def test_prototypes_match_the_header():
    text = open(os.path.join(REPO, "include", "slam2d.h")).read()
    ctype = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}
    res = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name in NAMES:
        m = re.search(r"^(int|int64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", text, re.M)
        assert m, name
        want = []
        for arg in re.sub(r"/\*.*?\*/", " ", m.group(2), flags=re.S).split(","):
            arg = " ".join(arg.split())
            assert "Slam2dLidar" not in arg                    # neither call takes a lidar
            if "Slam2dLevel*" in arg:
                want.append(ctypes.POINTER(_lib.Slam2dLevel))
            elif arg.endswith("[3]"):
                want.append(ctypes.POINTER(ctype[arg.split()[-2]]))            # (const double motion[3]: a pointer to doubles)
            elif "*" in arg:
                want.append(ctypes.c_void_p)
            else:
                want.append(ctype[arg.split()[0]])
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res[m.group(1)] and got_args == want, name
    assert int(re.search(r"#define\s+SLAM2D_ABI_VERSION\s+(\d+)", text).group(1)) == 18
    assert re.search(r"#define\s+SLAM2D_MAX_POINTS\s+SLAM2D_MAX_BEAMS\b", text)
    assert _lib.MAX_POINTS == _lib.MAX_BEAMS == 2048 == _lib.REFINE_TABLE      # one heading of the largest set fits a block's table


def test_the_work_sizes(L):
    work = L.slam2d_search_points_work
    for M, nx, ny, nth in ((1, 1, 1, 1), (60, 9, 7, 5), (180, 161, 161, 120), (2048, 1, 1, 65536), (2048, 46340, 46340, 1), (7, 2 ** 31 - 1, 1, 3)):
        assert work(M, nx, ny, nth) == 2 * nth * M, (M, nx, ny, nth)
    for bad in ((0, 9, 7, 5), (-1, 9, 7, 5), (2049, 9, 7, 5), (60, 0, 7, 5), (60, 9, 0, 5), (60, 9, 7, 0), (60, -9, 7, 5), (60, 9, 7, 65537)):
        assert work(*bad) == -1, bad
    assert work(60, 2 ** 16, 2 ** 15, 5) == -2 and work(60, 2 ** 31 - 1, 2 ** 31 - 1, 5) == -2             # nx * ny >= 2^31
    assert work(0, 2 ** 16, 2 ** 15, 5) == -1                  # a bad argument is named before a size
    # the refinement's scratch is slam2d_refine_work's: the moved seeds
    assert L.slam2d_refine_work(5) == 15


@CALLS
def test_null_pointers_are_refused(L, call):
    assert call(L, level=None) == -1
    assert call(L, level=_level(field=None)) == -1             # a level without a field
    assert call(L, level=_level(frames=None)) == -1            # ... without frames
    names = ("d_points", "d_out", "d_work") + (("d_pose_in", "d_pose_out") if call is _refine else ())
    for name in names:
        assert call(L, **{name: None}) == -1, name


def test_overlapping_pose_buffers_are_refused(L):
    assert _refine(L, d_pose_in=FAKE, d_pose_out=FAKE) == -1


@CALLS
@pytest.mark.parametrize("kw", [dict(p_field=-1), dict(M=0), dict(M=-1), dict(M=_lib.MAX_POINTS + 1), dict(point_stride=1), dict(point_stride=0),
                                dict(point_stride=-2), dict(dx=NAN), dict(dx=INF), dict(dy=NAN), dict(dy=-INF), dict(dth=NAN), dict(dth=INF)])
def test_numbers_both_calls_refuse(L, call, kw):
    assert call(L, **kw) == -1


@pytest.mark.parametrize("kw", [dict(nx=0), dict(ny=0), dict(nth=0), dict(nx=-1), dict(ny=-5), dict(nth=-1), dict(nth=65537)])
def test_numbers_the_search_refuses(L, kw):
    assert _search(L, **kw) == -1


@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-3), dict(pose_stride=2), dict(pose_stride=0), dict(set_stride=119), dict(set_stride=1),
                                dict(set_stride=-120), dict(point_stride=3, set_stride=179), dict(rx=-1), dict(ry=-1), dict(rt=-1),
                                dict(rx=-2 ** 31), dict(motion=(NAN, 0.0, 0.0)), dict(motion=(0.0, INF, 0.0)), dict(motion=(0.0, 0.0, -INF))])
def test_numbers_the_refinement_refuses(L, kw):
    assert _refine(L, **kw) == -1


@CALLS
@pytest.mark.parametrize("kw", [dict(step=0.0), dict(step=-0.1), dict(step=NAN), dict(cost_scale=0.0), dict(cost_scale=-1.0),
                                dict(cost_scale=NAN), dict(fmax=0), dict(fmax=290, fpitch=289)])
def test_level_parameters_are_refused(L, call, kw):
    assert call(L, level=_level(**kw)) == -1


def test_what_does_not_fit_is_too_large(L):
    assert _search(L, nx=2 ** 16, ny=2 ** 15) == -2            # nx * ny = 2^31
    assert _search(L, nx=2 ** 31 - 1, ny=2 ** 31 - 1) == -2
    assert _search(L, level=_level(**BIG)) == -2 and _refine(L, level=_level(**BIG)) == -2
    assert _refine(L, rx=511, ry=511, rt=1) == -2              # 1023 * 1023 * 3
    assert _refine(L, rx=512, ry=512, rt=0) == -2              # 1025 * 1025 = 2^20 + 2049
    assert _refine(L, rx=0, ry=0, rt=2 ** 19) == -2            # 2^20 + 1 candidates
    assert _refine(L, rx=2 ** 31 - 1, ry=2 ** 31 - 1, rt=2 ** 31 - 1) == -2    # (the product in 64 bits, factor by factor)
    assert _refine(L, N=_lib.REFINE_MAX_BLOCKS + 1) == -2
    # 2^20 seeds of 60 points: 34 headings to a block, so 8 * 34 headings stay within the launch and 8 * 34 + 1 do not
    assert _lib.REFINE_TABLE // 60 == 34 and _lib.REFINE_MAX_BLOCKS == 8 << 20
    assert _refine(L, N=1 << 20, rx=0, ry=0, rt=(8 * 34) // 2) == -2
    # ... and of 2048 points one heading to a block: nine headings do not fit
    assert _refine(L, N=1 << 20, M=2048, rx=0, ry=0, rt=4) == -2
    # a bad argument is named before a size
    assert _search(L, nx=2 ** 16, ny=2 ** 15, dx=NAN) == -1 and _search(L, nx=2 ** 16, ny=2 ** 15, M=0) == -1
    assert _search(L, level=_level(**BIG), d_work=None) == -1 and _search(L, level=_level(**BIG), nth=0) == -1
    assert _refine(L, rx=2 ** 31 - 1, ry=2 ** 31 - 1, dx=NAN) == -1
    assert _refine(L, level=_level(**BIG), d_work=None) == -1 and _refine(L, level=_level(**BIG), set_stride=7) == -1
    assert _refine(L, N=_lib.REFINE_MAX_BLOCKS + 1, motion=(0.0, NAN, 0.0)) == -1


def test_the_accepted_edges_are_no_argument_errors(L):
    """An accepted call reaches HIP, which these fake pointers must not.  So the edges are shown on a level whose image is beyond
    the build's limit: every SLAM2D_E_BADARG comes before any SLAM2D_E_TOOLARGE, so -2 here means that no argument check refused
    them (and -1 with one pointer taken away, that the checks did run).  That they are accepted in full is
    tests/test_gpu_points.py's."""
    big = _level(**BIG)
    for call in (_search, _refine):
        ok = lambda **kw: call(L, level=big, **kw) == -2 and call(L, level=big, d_out=None, **kw) == -1
        assert ok()
        assert ok(M=1) and ok(M=_lib.MAX_POINTS) and ok(point_stride=5)
        assert ok(dx=0.0, dy=0.0, dth=0.0) and ok(dx=-0.07, dy=-0.05, dth=-0.013)
        assert ok(outside_cost=0) and ok(outside_cost=2 ** 32 - 1)
        assert not ok(M=0) and not ok(dx=NAN)                  # (`ok` can fail)
    ok = lambda **kw: _search(L, level=big, **kw) == -2 and _search(L, level=big, d_out=None, **kw) == -1
    assert ok(nx=1, ny=1, nth=1) and ok(nth=65536) and ok(nx=46340, ny=46340) and ok(x0=NAN, y0=INF, th0=-INF)
    ok = lambda **kw: _refine(L, level=big, **kw) == -2 and _refine(L, level=big, d_out=None, **kw) == -1
    assert ok(rx=0, ry=0, rt=0) and ok(rx=512, ry=16, rt=15) and ok(rx=0, ry=0, rt=2 ** 19 - 1)
    assert ok(N=1, rx=7, ry=7, rt=0) and ok(N=1 << 20) and ok(N=1 << 20, rt=0) and ok(N=1 << 20, M=2048, rt=3)
    assert ok(pose_stride=5, set_stride=120) and ok(set_stride=123, motion=(0.1, -0.02, 0.03)) and ok(point_stride=3, set_stride=180)
