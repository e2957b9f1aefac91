"""slam2d_score_points, slam2d_mcl_step_points, slam2d_mcl_step_adaptive_points and their two work sizes at the C ABI, without a
GPU: exported, bound and declared, the work sizes against the header's formulas, and every refusal of include/slam2d.h before any
HIP call (a NULL stream and fake pointers: a call that returns has made none) -- the level cases of slam2d_score_poses, the
point cases of slam2d_refine_points, the particle, table, motion and bins cases of the scan forms.  No kernel is launched."""
import ctypes
import importlib
import os
import re

import pytest

from conftest import REPO

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

FAKE = 4096                                                    # never dereferenced: every call below is refused first
NAN, INF = float("nan"), float("inf")
MAXN, MAXB = 1 << 20, 1 << 26
NAMES = ("slam2d_score_points", "slam2d_mcl_points_work", "slam2d_mcl_step_points", "slam2d_mcl_adapt_points_work",
         "slam2d_mcl_step_adaptive_points")
BIG = dict(fmax=23200, fpitch=23200)                           # an image beyond slam2d_field_build's own limit


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _level(**kw):
    d = dict(step=0.1, reach=14.4, cost_scale=float(2 ** 28), fmax=290, fpitch=304, field=FAKE, frames=FAKE)
    d.update(kw)
    return _lib.Slam2dLevel(**d)


def _bins(**kw):
    d = dict(x0=-8.0, y0=-8.0, cell=0.5, turn=2 * 3.141592653589793 / 36, nx=32, ny=32, nth=36)
    d.update(kw)
    return _lib.Slam2dMclBins(**d)


_vp = lambda v: None if v is None else ctypes.c_void_p(v)
_arr = lambda v: None if v is None else (ctypes.c_double * 3)(*v)
_ref = lambda v: None if v is None else ctypes.byref(v)


def _score(L, level="ok", p_field=0, N=5, d_pose=FAKE, pose_stride=3, d_points=FAKE, point_stride=2, M=60, set_stride=0, d_out=FAKE):
    lv = _level() if level == "ok" else level
    return L.slam2d_score_points(_ref(lv), p_field, N, _vp(d_pose), pose_stride, _vp(d_points), point_stride, M, set_stride, _vp(d_out), None)


def _step(L, level="ok", p_field=0, N=3, d_in=FAKE, d_out=2 * FAKE, pose_stride=3, motion=(0.1, 0.0, 0.02), amp=(0.01, 0.01, 0.01), seed=1, scan=2,
          d_points=FAKE, point_stride=2, M=60, outside=1000, d_lut=FAKE, lut_n=4096, lut_shift=21, d_anc=FAKE, d_work=FAKE, d_report=FAKE):
    lv = _level() if level == "ok" else level
    return L.slam2d_mcl_step_points(_ref(lv), p_field, N, _vp(d_in), _vp(d_out), pose_stride, _arr(motion), _arr(amp), seed, scan, _vp(d_points),
                                    point_stride, M, outside, _vp(d_lut), lut_n, lut_shift, _vp(d_anc), _vp(d_work), _vp(d_report), None)


def _adaptive(L, level="ok", p_field=0, N=3, d_n_in=3 * FAKE, d_n_out=3 * FAKE, d_in=FAKE, d_out=2 * FAKE, pose_stride=3, motion=(0.1, 0.0, 0.02),
              amp=(0.01, 0.01, 0.01), seed=1, scan=2, d_points=FAKE, point_stride=2, M=60, outside=1000, d_lut=FAKE, lut_n=4096, lut_shift=21,
              bins="ok", d_ntab=FAKE, ntab_n=4096, d_anc=FAKE, d_work=FAKE, d_report=FAKE):
    """(``N`` is the capacity n_cap: one name for the cases the two steps share.)"""
    lv = _level() if level == "ok" else level
    bn = _bins() if bins == "ok" else bins
    return L.slam2d_mcl_step_adaptive_points(_ref(lv), p_field, N, _vp(d_n_in), _vp(d_n_out), _vp(d_in), _vp(d_out), pose_stride, _arr(motion),
                                             _arr(amp), seed, scan, _vp(d_points), point_stride, M, outside, _vp(d_lut), lut_n, lut_shift, _ref(bn),
                                             _vp(d_ntab), ntab_n, _vp(d_anc), _vp(d_work), _vp(d_report), None)


ALL = pytest.mark.parametrize("call", [_score, _step, _adaptive], ids=["score", "step", "adaptive"])
STEPS = pytest.mark.parametrize("call", [_step, _adaptive], ids=["step", "adaptive"])


def test_symbols_exported_and_bound(L):
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert getattr(L, name).restype is (ctypes.c_int64 if name.endswith("_work") else ctypes.c_int)
    assert L.slam2d_abi_version() == _lib.ABI_VERSION == 18    # added symbols: the ABI number stays


def test_prototypes_match_the_header():
    text = open(os.path.join(REPO, "include", "slam2d.h")).read()
    ctype = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}
    res = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name in NAMES:
        m = re.search(r"^(int|int64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", text, re.M)
        assert m, name
        want = []
        for arg in re.sub(r"/\*.*?\*/", " ", m.group(2), flags=re.S).split(","):
            arg = " ".join(arg.split())
            assert "Slam2dLidar" not in arg                    # none of the calls takes a lidar
            if "Slam2dLevel*" in arg:
                want.append(ctypes.POINTER(_lib.Slam2dLevel))
            elif "Slam2dMclBins*" in arg:
                want.append(ctypes.POINTER(_lib.Slam2dMclBins))
            elif arg.endswith("[3]"):
                want.append(ctypes.POINTER(ctype[arg.split()[-2]]))            # (const double motion[3]: a pointer to doubles)
            elif "*" in arg:
                want.append(ctypes.c_void_p)
            else:
                want.append(ctype[arg.split()[0]])
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res[m.group(1)] and got_args == want, name
    assert int(re.search(r"#define\s+SLAM2D_ABI_VERSION\s+(\d+)", text).group(1)) == 18
    assert "no point form" not in text


def test_the_work_sizes(L):
    """slam2d_mcl_work(N) + 2 N, and slam2d_mcl_adapt_work(n_cap, bins) + 2 n_cap: the cos / sin of the moved headings."""
    for n in (1, 1024, MAXN):
        assert L.slam2d_mcl_points_work(n) == 5 * n + 1032 + 2 * n == L.slam2d_mcl_work(n) + 2 * n, n
        for shape in (dict(nx=1, ny=1, nth=1), dict(nx=32, ny=32, nth=36), dict(nx=4, ny=4, nth=4)):
            n_bins = shape["nx"] * shape["ny"] * shape["nth"]
            got = L.slam2d_mcl_adapt_points_work(n, ctypes.byref(_bins(**shape)))
            assert got == 5 * n + 1032 + (n_bins + 64) // 64 + 8 + 2 * n == L.slam2d_mcl_adapt_work(n, ctypes.byref(_bins(**shape))) + 2 * n, (n, shape)
    assert L.slam2d_mcl_points_work(MAXN + 1) == -2 and L.slam2d_mcl_adapt_points_work(MAXN + 1, ctypes.byref(_bins())) == -2
    assert L.slam2d_mcl_points_work(2 ** 31 - 1) == -2
    for n in (0, -1, -2 ** 31):
        assert L.slam2d_mcl_points_work(n) == -1 and L.slam2d_mcl_adapt_points_work(n, ctypes.byref(_bins())) == -1, n
    assert L.slam2d_mcl_adapt_points_work(5, None) == -1
    assert L.slam2d_mcl_adapt_points_work(5, ctypes.byref(_bins(cell=0.0))) == -1
    assert L.slam2d_mcl_adapt_points_work(MAXN + 1, ctypes.byref(_bins(nx=0))) == -1           # an argument error comes first
    assert L.slam2d_mcl_adapt_points_work(5, ctypes.byref(_bins(nx=MAXB + 1, ny=1, nth=1))) == -2


# ---- the level cases of slam2d_score_poses ----
@ALL
def test_a_level_that_cannot_be_read_is_refused(L, call):
    assert call(L, level=None) == -1
    assert call(L, level=_level(field=None)) == -1
    assert call(L, level=_level(frames=None)) == -1
    assert call(L, p_field=-1) == -1


@ALL
@pytest.mark.parametrize("kw", [dict(step=0.0), dict(step=-0.1), dict(step=NAN), dict(cost_scale=0.0), dict(cost_scale=-1.0),
                                dict(cost_scale=NAN), dict(fmax=0), dict(fmax=290, fpitch=289)])
def test_level_parameters_are_refused(L, call, kw):
    assert call(L, level=_level(**kw)) == -1


# ---- the point cases of slam2d_refine_points ----
@ALL
@pytest.mark.parametrize("kw", [dict(M=0), dict(M=-1), dict(M=_lib.MAX_POINTS + 1), dict(point_stride=1), dict(point_stride=0),
                                dict(point_stride=-2), dict(d_points=None)])
def test_point_sets_are_refused(L, call, kw):
    assert call(L, **kw) == -1
    assert call(L, level=_level(**BIG), **kw) == -1            # ... before any size


@pytest.mark.parametrize("kw", [dict(set_stride=119), dict(set_stride=1), dict(set_stride=-120), dict(point_stride=3, set_stride=179)])
def test_set_strides_the_score_refuses(L, kw):
    assert _score(L, **kw) == -1


@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-3), dict(pose_stride=2), dict(pose_stride=0), dict(d_pose=None), dict(d_out=None)])
def test_poses_the_score_refuses(L, kw):
    assert _score(L, **kw) == -1


# ---- the particle, table and motion cases of slam2d_mcl_step ----
@STEPS
@pytest.mark.parametrize("what", ["d_in", "d_out", "motion", "amp", "d_lut", "d_work", "d_report"])
def test_null_pointers_of_the_steps_are_refused(L, call, what):
    assert call(L, **{what: None}) == -1


@STEPS
def test_ping_pong_wants_two_buffers(L, call):
    assert call(L, d_in=FAKE, d_out=FAKE) == -1


@STEPS
@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-1), dict(N=-2 ** 31), dict(pose_stride=2), dict(pose_stride=0), dict(pose_stride=-3),
                                dict(lut_n=0), dict(lut_n=-1), dict(lut_n=65537), dict(lut_shift=-1), dict(lut_shift=44), dict(lut_shift=64)])
def test_counts_strides_and_table_shapes_are_refused(L, call, kw):
    assert call(L, **kw) == -1


@STEPS
@pytest.mark.parametrize("which", ["motion", "amp"])
@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_non_finite_motion_and_amplitudes_are_refused(L, call, which, i, bad):
    v = [0.1, 0.0, 0.02]
    v[i] = bad
    assert call(L, **{which: tuple(v)}) == -1


# ---- the count, table and bins cases of slam2d_mcl_step_adaptive ----
@pytest.mark.parametrize("kw", [dict(d_n_in=None), dict(d_n_out=None), dict(d_ntab=None), dict(bins=None), dict(ntab_n=0), dict(ntab_n=-1),
                                dict(ntab_n=65537)])
def test_counts_and_tables_the_adaptive_step_refuses(L, kw):
    assert _adaptive(L, **kw) == -1


@pytest.mark.parametrize("kw", [dict(nx=0), dict(ny=0), dict(nth=0), dict(nx=-5), dict(ny=-2 ** 31), dict(nth=-1), dict(cell=0.0), dict(cell=-0.5),
                                dict(cell=NAN), dict(turn=0.0), dict(turn=-1.0), dict(turn=NAN), dict(x0=NAN), dict(x0=INF), dict(x0=-INF),
                                dict(y0=NAN), dict(y0=INF), dict(y0=-INF)])
def test_bins_are_refused(L, kw):
    assert _adaptive(L, bins=_bins(**kw)) == -1
    assert _adaptive(L, bins=_bins(**kw), N=MAXN + 1) == -1


# ---- sizes, and the accepted edges ----
def test_too_large(L):
    assert _score(L, level=_level(**BIG)) == -2 and _step(L, level=_level(**BIG)) == -2 and _adaptive(L, level=_level(**BIG)) == -2
    assert _step(L, N=MAXN + 1) == -2 and _adaptive(L, N=MAXN + 1) == -2 and _step(L, N=2 ** 31 - 1) == -2
    assert _adaptive(L, bins=_bins(nx=MAXB + 1, ny=1, nth=1)) == -2 and _adaptive(L, bins=_bins(nx=4096, ny=4096, nth=5)) == -2
    assert _score(L, N=2 ** 31 - 1, M=2048) == -2              # two poses per block of 128 threads: 2^36 threads
    # an argument error comes first, whichever size is too large beside it
    assert _step(L, N=MAXN + 1, pose_stride=2) == -1 and _step(L, N=MAXN + 1, M=0) == -1 and _step(L, level=_level(**BIG), d_report=None) == -1
    assert _adaptive(L, N=MAXN + 1, point_stride=1) == -1 and _adaptive(L, bins=_bins(nx=MAXB + 1), d_ntab=None) == -1
    assert _score(L, level=_level(**BIG), set_stride=7) == -1 and _score(L, N=2 ** 31 - 1, M=2048, pose_stride=2) == -1


def test_the_accepted_edges_are_no_argument_errors(L):
    """An accepted call reaches HIP, which these fake pointers must not.  So the edges are shown beside a size that is too large:
    every SLAM2D_E_BADARG comes before any SLAM2D_E_TOOLARGE, so -2 here means that no argument check refused them (and -1 with
    one pointer taken away, that the checks did run).  That they are accepted in full is tests/test_gpu_mcl_points.py's."""
    big = _level(**BIG)
    ok = lambda **kw: _score(L, level=big, **kw) == -2 and _score(L, level=big, d_out=None, **kw) == -1
    assert ok() and ok(M=1) and ok(M=_lib.MAX_POINTS) and ok(point_stride=5) and ok(N=1) and ok(pose_stride=7)
    assert ok(set_stride=120) and ok(set_stride=123) and ok(point_stride=3, set_stride=180) and not ok(M=0)
    for call in (_step, _adaptive):
        ok = lambda **kw: call(L, N=MAXN + 1, **kw) == -2 and call(L, N=MAXN + 1, d_report=None, **kw) == -1
        assert ok() and ok(d_anc=None) and ok(M=1) and ok(M=_lib.MAX_POINTS) and ok(point_stride=5) and ok(pose_stride=7)
        assert ok(lut_n=1, lut_shift=0) and ok(lut_n=65536, lut_shift=43, amp=(0.0, 0.0, 0.0)) and ok(outside=0) and ok(outside=2 ** 32 - 1)
        assert not ok(M=0) and not ok(lut_n=0)                 # (`ok` can fail)
    assert _adaptive(L, N=MAXN + 1, d_n_in=5 * FAKE, d_n_out=6 * FAKE, ntab_n=1) == -2
    assert _adaptive(L, N=MAXN + 1, bins=_bins(nx=4096, ny=4096, nth=4, cell=1e-300, turn=1e300, x0=-1e300, y0=1e300), ntab_n=65536) == -2
