"""slam2d_cast_rays and slam2d_score_rays at the C ABI, without a GPU: exported and bound, the header's constants mirrored,
argument errors refused before any HIP call.  No kernel is launched."""
import ctypes
import importlib
import os
import re

import pytest

from conftest import REPO

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

FAKE = 4096                                                    # never dereferenced: every call below is refused first
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _lidar(**kw):
    """A host-built descriptor: parameters only (the calls read beams, fov, max_range)."""
    d = dict(unit=0.1, max_range=4.0, fov=3.141592653589793, beams=60)
    d.update(kw)
    return _lib.Slam2dLidar(**d)


def _level(**kw):
    """A host-built level: parameters only, no device memory behind its pointers."""
    d = dict(step=0.1, reach=14.4, cost_scale=float(2 ** 28), fmax=290, fpitch=304, field=FAKE, frames=FAKE)
    d.update(kw)
    return _lib.Slam2dLevel(**d)


def _vp(v):
    return None if v is None else ctypes.c_void_p(v)


def _cast(L, lidar="ok", level="ok", p_field=0, d_dist2=FAKE, N=3, d_pose=FAKE, pose_stride=3, K=40, d_out=FAKE):
    lid = _lidar() if lidar == "ok" else lidar
    lv = _level() if level == "ok" else level
    return L.slam2d_cast_rays(None if lid is None else ctypes.byref(lid), None if lv is None else ctypes.byref(lv), p_field, _vp(d_dist2), N,
                              _vp(d_pose), pose_stride, K, _vp(d_out), None)


def _score(L, lidar="ok", level="ok", p_field=0, d_dist2=FAKE, N=3, d_pose=FAKE, pose_stride=3, d_ranges=FAKE, ranges_stride=0, margin=2,
           outside_cost=5, through_cost=5, d_out=FAKE):
    lid = _lidar() if lidar == "ok" else lidar
    lv = _level() if level == "ok" else level
    return L.slam2d_score_rays(None if lid is None else ctypes.byref(lid), None if lv is None else ctypes.byref(lv), p_field, _vp(d_dist2), N,
                               _vp(d_pose), pose_stride, _vp(d_ranges), ranges_stride, margin, outside_cost, through_cost, _vp(d_out), None)


BOTH = [_cast, _score]


def test_symbols_exported_and_bound(L):
    for name in ("slam2d_cast_rays", "slam2d_score_rays"):
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert _lib.RAYS_STRIDE == 8 and (_lib.RAY_HIT, _lib.RAY_LEFT, _lib.RAY_NONE) == (0, 1, 2) and _lib.RAY_MAX_K == 1 << 20
    assert L.slam2d_abi_version() == 18                        # added symbols: the ABI number stays


def test_header_constants_and_declarations():
    text = open(os.path.join(REPO, "include", "slam2d.h")).read()
    assert int(re.search(r"#define\s+SLAM2D_RAYS_STRIDE\s+(\d+)", text).group(1)) == _lib.RAYS_STRIDE
    for name, value in (("HIT", _lib.RAY_HIT), ("LEFT", _lib.RAY_LEFT), ("NONE", _lib.RAY_NONE)):
        assert int(re.search(rf"#define\s+SLAM2D_RAY_{name}\s+(\d+)u", text).group(1)) == value
    assert re.search(r"#define\s+SLAM2D_RAY_MAX_K\s+\(1 << 20\)", text)
    assert re.search(r"int\s+slam2d_cast_rays\s*\(", text) and re.search(r"int\s+slam2d_score_rays\s*\(", text)
    assert int(re.search(r"#define\s+SLAM2D_ABI_VERSION\s+(\d+)", text).group(1)) == 18


@pytest.mark.parametrize("call", BOTH)
def test_null_pointers_are_refused(L, call):
    assert call(L, lidar=None) == -1
    assert call(L, level=None) == -1
    assert call(L, d_dist2=None) == -1
    assert call(L, d_pose=None) == -1
    assert call(L, d_out=None) == -1
    assert call(L, level=_level(frames=None)) == -1           # a level without frames


def test_what_only_one_of_them_reads(L):
    assert _score(L, d_ranges=None) == -1
    assert _score(L, level=_level(field=None)) == -1          # the score reads the field ...
    assert _cast(L, level=_level(field=None), N=2 ** 31 - 1) == -2      # ... the cast does not: it gets as far as the launch's size
    assert _cast(L, level=_level(cost_scale=NAN), N=2 ** 31 - 1) == -2  # neither reads cost_scale
    assert _score(L, level=_level(cost_scale=0.0), N=2 ** 31 - 1) == -2


@pytest.mark.parametrize("call", BOTH)
@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-2), dict(p_field=-1), dict(pose_stride=2), dict(pose_stride=0), dict(pose_stride=-3)])
def test_counts_and_strides_are_refused(L, call, kw):
    assert call(L, **kw) == -1


@pytest.mark.parametrize("kw", [dict(ranges_stride=1), dict(ranges_stride=59), dict(ranges_stride=-1), dict(ranges_stride=-60), dict(margin=-1),
                                dict(margin=-2 ** 31)])
def test_score_strides_and_margin_are_refused(L, kw):
    assert _score(L, **kw) == -1


def test_sample_limits(L):
    assert _cast(L, K=-1) == -1
    assert _cast(L, K=-2 ** 31) == -1
    assert _cast(L, K=1 << 20) == -2
    assert _cast(L, K=2 ** 31 - 1) == -2
    assert _cast(L, K=(1 << 20) - 1, N=2 ** 31 - 1) == -2      # the largest K passes: the launch's size is what refuses this call
    assert _cast(L, K=1 << 20, N=0) == -1                      # every BADARG comes before a TOOLARGE


@pytest.mark.parametrize("call", BOTH)
@pytest.mark.parametrize("beams", [0, -1, _lib.MAX_BEAMS + 1])
def test_beam_counts_are_refused(L, call, beams):
    assert call(L, lidar=_lidar(beams=beams)) == -1


@pytest.mark.parametrize("call", BOTH)
@pytest.mark.parametrize("max_range", [0.0, -4.0, NAN])
def test_a_lidar_without_a_range_is_refused(L, call, max_range):
    assert call(L, lidar=_lidar(max_range=max_range)) == -1


@pytest.mark.parametrize("call", BOTH)
@pytest.mark.parametrize("kw", [dict(step=0.0), dict(step=-0.1), dict(step=NAN), dict(fmax=0), dict(fmax=290, fpitch=289)])
def test_level_parameters_are_refused(L, call, kw):
    assert call(L, level=_level(**kw)) == -1


def test_a_launch_that_does_not_fit_is_too_large(L):
    # the cast: a wave per 64 beams of a pose, four waves per block of 256 threads, fewer than 2^32 threads per launch
    assert _cast(L, N=2 ** 26) == -2                           # 60 beams: one wave per pose
    assert _cast(L, lidar=_lidar(beams=65), N=2 ** 25) == -2   # two
    assert _cast(L, lidar=_lidar(beams=_lib.MAX_BEAMS), N=2 ** 21) == -2
    # the score: a wave per pose
    assert _score(L, N=2 ** 26) == -2
    assert _score(L, N=2 ** 31 - 1) == -2
    for call in BOTH:
        assert call(L, level=_level(fmax=23200, fpitch=23200)) == -2     # an image beyond slam2d_field_build's own limit
        assert call(L, level=_level(fmax=23200, fpitch=23200), N=0) == -1
