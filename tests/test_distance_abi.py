"""slam2d_field_build_distance at the C ABI, without a GPU: exported and bound, the header's declaration, and every argument
error refused before any HIP call.  No kernel is launched."""
import ctypes
import importlib
import os
import re

import pytest

from conftest import REPO

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

FAKE = 4096                                                    # never dereferenced: every call below is refused first
NAN = float("nan")
NAME = "slam2d_field_build_distance"
P, FMAX, FPITCH, TMAX = 2, 290, 304, 19


@pytest.fixture(scope="module")
def L():
    _lib.build_library()
    return _lib.lib()


def _lidar(**kw):
    d = dict(unit=0.1, max_range=4.0, fov=3.141592653589793, beams=60)
    d.update(kw)
    return _lib.Slam2dLidar(**d)


def _level(**kw):
    """A level slam2d_field_build accepts for P particles: the flags follow the image (occ_gen == 0: one memset clears both)."""
    d = dict(step=0.1, reach=14.4, cost_scale=float(2 ** 28), blur_radius=4, fmax=FMAX, fpitch=FPITCH, wmax=291, ncell=1, ntheta=1,
             tmax=TMAX, frames=FAKE, axis_x=FAKE, axis_y=FAKE, field=FAKE, occ=FAKE, tilemask=FAKE + P * FMAX * FPITCH, tilestate=FAKE,
             tilemin=FAKE, tilemax=FAKE, tilelist=FAKE, tilecount=FAKE, occ_gen=0)
    d.update(kw)
    return _lib.Slam2dLevel(**d)


def _args(lidar="ok", level="ok", d_maps=FAKE, n=P, d_centre=FAKE, stride=2, d_lut=FAKE, lut_n=208, d_dist2=None, d_flags=FAKE):
    lid = _lidar() if lidar == "ok" else lidar
    lv = _level() if level == "ok" else level
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    return lid, lv, vp, (d_maps, n, d_centre, stride, d_lut, lut_n, d_dist2, d_flags)


def _call(L, **kw):
    lid, lv, vp, (d_maps, n, d_centre, stride, d_lut, lut_n, d_dist2, d_flags) = _args(**kw)
    return L.slam2d_field_build_distance(None if lid is None else ctypes.byref(lid), None if lv is None else ctypes.byref(lv), vp(d_maps), n,
                                         vp(d_centre), stride, vp(d_lut), lut_n, vp(d_dist2), vp(d_flags), None)


def _full(L, **kw):
    """slam2d_field_build on the arguments the two calls share."""
    kw = {k: v for k, v in kw.items() if k not in ("d_lut", "lut_n", "d_dist2")}
    lid, lv, vp, (d_maps, n, d_centre, stride, _, _, _, d_flags) = _args(**kw)
    return L.slam2d_field_build(None if lid is None else ctypes.byref(lid), None if lv is None else ctypes.byref(lv), vp(d_maps), n,
                                vp(d_centre), stride, vp(d_flags), None)


def test_symbol_exported_and_bound(L):
    assert hasattr(L, NAME), f"{NAME} is not exported"
    assert NAME in _lib.SIGNATURES, f"{NAME} has no ctypes signature"
    assert L.slam2d_field_build_distance.restype is ctypes.c_int
    assert _lib.DISTANCE_MAX_TABLE == 65536
    assert L.slam2d_abi_version() == 18 and _lib.ABI_VERSION == 18      # an added symbol: the ABI number stays


def test_prototype_matches_the_header():
    text = open(os.path.join(REPO, "include", "slam2d.h")).read()
    ctype = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", text, re.M)
    assert m, NAME
    want = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if "Slam2dLidar*" in arg:
            want.append(ctypes.POINTER(_lib.Slam2dLidar))
        elif "Slam2dLevel*" in arg:
            want.append(ctypes.POINTER(_lib.Slam2dLevel))
        elif "*" in arg:
            want.append(ctypes.c_void_p)
        else:
            want.append(ctype[arg.split()[0]])
    names = [" ".join(a.split()).split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["lidar", "level", "d_maps", "P", "d_centre", "centre_stride", "d_lut", "lut_n", "d_dist2", "d_flags", "stream"]
    got_res, got_args = _lib.SIGNATURES[NAME]
    assert got_res is ctypes.c_int and got_args == want
    assert int(re.search(r"#define\s+SLAM2D_ABI_VERSION\s+(\d+)", text).group(1)) == 18
    assert int(re.search(r"#define\s+SLAM2D_DISTANCE_MAX_TABLE\s+(\d+)", text).group(1)) == _lib.DISTANCE_MAX_TABLE


def test_the_table_is_checked(L):
    assert _call(L, d_lut=None) == -1
    for n in (0, -1, -2 ** 31, _lib.DISTANCE_MAX_TABLE + 1, 2 ** 31 - 1):
        assert _call(L, lut_n=n) == -1, n


# what slam2d_field_build refuses, and with which code: asserted on slam2d_field_build itself wherever it refuses before a launch
SHARED = [
    (dict(lidar=None), -1), (dict(level=None), -1), (dict(n=0), -1), (dict(n=-3), -1),
    (dict(d_maps=None), -1), (dict(d_centre=None), -1), (dict(d_flags=None), -1), (dict(stride=1), -1), (dict(stride=0), -1),
    (dict(level=_level(blur_radius=-1)), -2), (dict(level=_level(blur_radius=_lib.MAX_BLUR_RADIUS + 1)), -2),
    (dict(lidar=_lidar(beams=1)), -2), (dict(lidar=_lidar(beams=_lib.MAX_BEAMS + 1)), -2),
    (dict(level=_level(fmax=0)), -1), (dict(level=_level(fpitch=FMAX - 1)), -1), (dict(level=_level(wmax=0)), -1),
    (dict(level=_level(ncell=-1)), -1), (dict(level=_level(ntheta=0)), -1),
    (dict(level=_level(cost_scale=0.0)), -1), (dict(level=_level(cost_scale=-1.0)), -1), (dict(level=_level(cost_scale=NAN)), -1),
    (dict(level=_level(fmax=23200, fpitch=23200)), -2),
    (dict(level=_level(occ=None)), -1), (dict(level=_level(tilemask=None)), -1), (dict(level=_level(tilemask=FAKE)), -1),
    (dict(level=_level(tilestate=None)), -1), (dict(level=_level(tilemin=None)), -1), (dict(level=_level(tilemax=None)), -1),
    (dict(level=_level(tilelist=None)), -1), (dict(level=_level(tilecount=None)), -1),
    (dict(level=_level(tmax=168)), -2),                        # 168^2 = 28224 tiles
]


@pytest.mark.parametrize("case", range(len(SHARED)))
def test_what_the_full_build_refuses_is_refused_alike(L, case):
    kw, code = SHARED[case]
    assert _full(L, **kw) == code, "slam2d_field_build"
    assert _call(L, **kw) == code


@pytest.mark.parametrize("kw", [dict(frames=None), dict(axis_x=None), dict(axis_y=None), dict(field=None), dict(occ_gen=-1), dict(occ_gen=256)])
def test_a_level_the_call_could_not_write_is_refused(L, kw):
    assert _call(L, level=_level(**kw)) == -1


def test_a_level_of_stamps_need_not_keep_its_flags_behind_its_image(L):
    """With generation stamps nothing is cleared, so the flags may lie anywhere (a view of a level): the same check as the
    full build's -- shown on a call that is refused later, for its table."""
    assert _call(L, level=_level(occ_gen=0, tilemask=FAKE), lut_n=0) == -1
    assert _call(L, level=_level(occ_gen=7, tilemask=FAKE), lut_n=0) == -1
    assert _call(L, level=_level(occ_gen=0, tilemask=FAKE)) == -1


def test_a_bad_argument_is_named_before_a_size(L):
    assert _call(L, level=_level(tmax=168), d_lut=None) == -1
    assert _call(L, level=_level(tmax=168), lut_n=0) == -1
