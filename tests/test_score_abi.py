"""slam2d_score_poses at the C ABI, without a GPU: exported and bound, the header's constant mirrored, argument errors refused
before any HIP call.  No kernel is launched."""
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
    """A host-built descriptor: parameters only (the call reads beams, fov, max_range)."""
    d = dict(unit=0.1, max_range=4.0, fov=3.141592653589793, beams=60)
    d.update(kw)
    return _lib.Slam2dLidar(**d)


def _level(**kw):
    """A host-built level: parameters only, no device memory behind its pointers."""
    d = dict(step=0.1, reach=14.4, cost_scale=float(2 ** 28), fmax=290, fpitch=304, field=FAKE, frames=FAKE)
    d.update(kw)
    return _lib.Slam2dLevel(**d)


def _call(L, lidar="ok", level="ok", p_field=0, N=3, d_pose=FAKE, pose_stride=3, d_ranges=FAKE, ranges_stride=0, d_out=FAKE):
    lid = _lidar() if lidar == "ok" else lidar
    lv = _level() if level == "ok" else level
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    return L.slam2d_score_poses(None if lid is None else ctypes.byref(lid), None if lv is None else ctypes.byref(lv), p_field, N,
                                vp(d_pose), pose_stride, vp(d_ranges), ranges_stride, vp(d_out), None)


def test_symbol_exported_and_bound(L):
    assert hasattr(L, "slam2d_score_poses"), "slam2d_score_poses is not exported"
    assert "slam2d_score_poses" in _lib.SIGNATURES, "slam2d_score_poses has no ctypes signature"
    assert _lib.SCORE_STRIDE == 8
    assert L.slam2d_abi_version() == 18                        # an added symbol: the ABI number stays


def test_header_constant_and_declaration():
    text = open(os.path.join(REPO, "include", "slam2d.h")).read()
    assert int(re.search(r"#define\s+SLAM2D_SCORE_STRIDE\s+(\d+)", text).group(1)) == _lib.SCORE_STRIDE
    assert re.search(r"int\s+slam2d_score_poses\s*\(", text)
    assert int(re.search(r"#define\s+SLAM2D_ABI_VERSION\s+(\d+)", text).group(1)) == 18


def test_null_pointers_are_refused(L):
    assert _call(L, lidar=None) == -1
    assert _call(L, level=None) == -1
    assert _call(L, d_pose=None) == -1
    assert _call(L, d_ranges=None) == -1
    assert _call(L, d_out=None) == -1
    assert _call(L, level=_level(field=None)) == -1            # a level without a field
    assert _call(L, level=_level(frames=None)) == -1           # ... without frames


@pytest.mark.parametrize("kw", [dict(N=0), dict(N=-2), dict(p_field=-1), dict(pose_stride=2), dict(pose_stride=0), dict(pose_stride=-3),
                                dict(ranges_stride=1), dict(ranges_stride=59), dict(ranges_stride=-1), dict(ranges_stride=-60)])
def test_counts_and_strides_are_refused(L, kw):
    assert _call(L, **kw) == -1


@pytest.mark.parametrize("beams", [0, -1, _lib.MAX_BEAMS + 1])
def test_beam_counts_are_refused(L, beams):
    assert _call(L, lidar=_lidar(beams=beams), ranges_stride=0) == -1
    assert _call(L, lidar=_lidar(beams=beams), ranges_stride=4096) == -1


@pytest.mark.parametrize("max_range", [0.0, -4.0, NAN])
def test_a_lidar_without_a_range_is_refused(L, max_range):
    assert _call(L, lidar=_lidar(max_range=max_range)) == -1


@pytest.mark.parametrize("kw", [dict(step=0.0), dict(step=-0.1), dict(step=NAN), dict(cost_scale=0.0), dict(cost_scale=-1.0),
                                dict(cost_scale=NAN), dict(fmax=0), dict(fmax=290, fpitch=289)])
def test_level_parameters_are_refused(L, kw):
    assert _call(L, level=_level(**kw)) == -1


def test_a_launch_that_does_not_fit_is_too_large(L):
    # four poses per block of 256 threads (two per 128 above 1365 beams), fewer than 2^32 threads per launch
    assert _call(L, N=2 ** 26) == -2
    assert _call(L, N=2 ** 31 - 1) == -2
    assert _call(L, lidar=_lidar(beams=_lib.MAX_BEAMS), N=2 ** 26) == -2
    assert _call(L, level=_level(fmax=23200, fpitch=23200)) == -2          # an image beyond slam2d_field_build's own limit
