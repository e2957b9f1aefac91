"""slam2d_search_lattice / slam2d_search_lattice_work at the C ABI, without a GPU: exported and bound, the header's declarations,
the work size, and every argument error refused before any HIP call.  No kernel is launched."""
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
    d = dict(unit=0.1, max_range=4.0, fov=3.141592653589793, beams=60)
    d.update(kw)
    return _lib.Slam2dLidar(**d)


def _level(**kw):
    d = dict(step=0.1, reach=14.4, cost_scale=float(2 ** 28), fmax=290, fpitch=304, field=FAKE, frames=FAKE)
    d.update(kw)
    return _lib.Slam2dLevel(**d)


def _call(L, lidar="ok", level="ok", p_field=0, nx=65, ny=5, nth=7, x0=-3.2, dx=0.1, y0=0.4, dy=0.1, th0=0.3, dth=0.9,
          d_ranges=FAKE, outside_cost=1000, d_work=FAKE, d_out=FAKE):
    lid = _lidar() if lidar == "ok" else lidar
    lv = _level() if level == "ok" else level
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    return L.slam2d_search_lattice(None if lid is None else ctypes.byref(lid), None if lv is None else ctypes.byref(lv), p_field,
                                   nx, ny, nth, x0, dx, y0, dy, th0, dth, vp(d_ranges), outside_cost, vp(d_work), vp(d_out), None)


def _work(L, nx=65, ny=5, nth=7, **kw):
    return L.slam2d_search_lattice_work(ctypes.byref(_lidar(**kw)), nx, ny, nth)


def test_symbols_exported_and_bound(L):
    for name in ("slam2d_search_lattice", "slam2d_search_lattice_work"):
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert L.slam2d_search_lattice_work.restype is ctypes.c_int64
    assert L.slam2d_search_lattice.restype is ctypes.c_int
    assert L.slam2d_abi_version() == 18                        # added symbols: the ABI number stays


def test_prototypes_match_the_header():
    text = open(os.path.join(REPO, "include", "slam2d.h")).read()
    ctype = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}
    res = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name in ("slam2d_search_lattice", "slam2d_search_lattice_work"):
        m = re.search(r"^(int|int64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", text, re.M)
        assert m, name
        want = []
        for arg in m.group(2).split(","):
            arg = " ".join(arg.split())
            if "Slam2dLidar*" in arg:
                want.append(ctypes.POINTER(_lib.Slam2dLidar))
            elif "Slam2dLevel*" in arg:
                want.append(ctypes.POINTER(_lib.Slam2dLevel))
            elif "*" in arg:
                want.append(ctypes.c_void_p)
            else:
                want.append(ctype[arg.split()[0]])
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res[m.group(1)] and got_args == want, name
    assert int(re.search(r"#define\s+SLAM2D_ABI_VERSION\s+(\d+)", text).group(1)) == 18


def test_the_work_size(L):
    # the endpoint table: one (cos * r, sin * r) pair of doubles per heading and beam, whatever the window
    assert _work(L) == 2 * 7 * 60
    assert _work(L, nx=1, ny=1, nth=1, beams=1) == 2
    assert _work(L, nx=161, ny=161, nth=120, beams=180) == 2 * 120 * 180
    assert _work(L, nx=3, ny=9000, nth=65536, beams=_lib.MAX_BEAMS) == 2 * 65536 * _lib.MAX_BEAMS
    assert _work(L, nx=46340, ny=46340, nth=2) == 2 * 2 * 60   # (nx * ny just below 2^31)


def test_the_work_size_refuses(L):
    assert L.slam2d_search_lattice_work(None, 65, 5, 7) == -1
    for kw in (dict(nx=0), dict(ny=0), dict(nth=0), dict(nx=-3), dict(ny=-1), dict(nth=-7), dict(nth=65537), dict(beams=0),
               dict(beams=-1), dict(beams=_lib.MAX_BEAMS + 1)):
        assert _work(L, **kw) == -1, kw
    assert _work(L, nx=65536, ny=32768) == -2                  # nx * ny == 2^31
    assert _work(L, nx=2 ** 31 - 1, ny=2 ** 31 - 1) == -2


def test_an_acceptable_call_would_reach_hip(L):
    """The arguments every case below starts from pass every check: nothing is refused but what the case changes.  (Shown on
    the work size, which shares the lattice's checks and makes no HIP call.)"""
    assert _work(L) > 0


def test_null_pointers_are_refused(L):
    assert _call(L, lidar=None) == -1
    assert _call(L, level=None) == -1
    assert _call(L, d_ranges=None) == -1
    assert _call(L, d_out=None) == -1
    assert _call(L, d_work=None) == -1                         # (the work size is > 0)
    assert _call(L, level=_level(field=None)) == -1            # a level without a field
    assert _call(L, level=_level(frames=None)) == -1           # ... without frames


@pytest.mark.parametrize("kw", [dict(p_field=-1), dict(nx=0), dict(nx=-1), dict(ny=0), dict(ny=-5), dict(nth=0), dict(nth=-1),
                                dict(nth=65537), dict(dx=NAN), dict(dx=INF), dict(dy=NAN), dict(dy=-INF), dict(dth=NAN), dict(dth=INF)])
def test_lattice_numbers_are_refused(L, kw):
    assert _call(L, **kw) == -1


@pytest.mark.parametrize("beams", [0, -1, _lib.MAX_BEAMS + 1])
def test_beam_counts_are_refused(L, beams):
    assert _call(L, lidar=_lidar(beams=beams)) == -1


@pytest.mark.parametrize("max_range", [0.0, -4.0, NAN])
def test_a_lidar_without_a_range_is_refused(L, max_range):
    assert _call(L, lidar=_lidar(max_range=max_range)) == -1


@pytest.mark.parametrize("kw", [dict(step=0.0), dict(step=-0.1), dict(step=NAN), dict(cost_scale=0.0), dict(cost_scale=-1.0),
                                dict(cost_scale=NAN), dict(fmax=0), dict(fmax=290, fpitch=289)])
def test_level_parameters_are_refused(L, kw):
    assert _call(L, level=_level(**kw)) == -1


def test_what_does_not_fit_is_too_large(L):
    assert _call(L, nx=65536, ny=32768) == -2                  # nx * ny == 2^31
    assert _call(L, nx=2 ** 31 - 1, ny=2) == -2
    assert _call(L, level=_level(fmax=23200, fpitch=23200)) == -2          # an image beyond slam2d_field_build's own limit
    # a bad argument is named before a size: the NULL work buffer of a lattice that is also too large
    assert _call(L, nx=65536, ny=32768, dx=NAN) == -1
