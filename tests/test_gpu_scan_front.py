"""The scan front end of slam2d_match held to its definition (Utils/ScanMatcher_OGBased.py:21-37,173-176) and its two launch
forms held to each other: below 512 beams and below 128 particles per launch the frame, the axis tables and the occupied-cell
scatter are block roles of k_endpoints' launch (k_endpoints<192> up to 192 beams, three waves and 24 map rows per scatter block;
<256> beyond, 32 rows); from 128 particles per launch k_frame_axis and k_occ_scatter are launches of their own.  Both write
frames, axis_x, axis_y, the flag words, the occupied field bytes and the flags of the 8 x 8-cell blocks: compared here exactly,
between the forms and against a NumPy statement of :29-37 on the downloaded map and frame.  Needs an MI355X: ``-m gpu``.

Every particle looks at the wrap fixture's lidar (unit 0.1, range 5, search radius 1: a window of 130 map columns and rows -- five
32-cell words across, a row count that is a multiple of neither 24 nor 32 and more than either form's block takes -- and a field
of 131 x 131 cells)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_parity import _wrap_grid    # (the map grown on the high side comes from that file's builder)

pytestmark = pytest.mark.gpu
E = importlib.import_module("slam-2d-lidar-scan_amd.engine")
_lib = E._lib

MERGED_P, SEPARATE_P = 9, 128


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


WALL_EVERY = 13                       # map B: row r is a wall where r % 13 == 5; rows 4 and 6 (mod 13) hold one occupied cell each
# (x, y, theta) of the nine particles; 0, 1, 8 on the map grown on the high side (the golden's own window centres), the rest on map B
EST = np.array([[20.0, 2.0, 0.3], [18.03, 21.0, 0.6], [0.3, -0.4, 0.1], [-1.1, 2.0, -0.7], [3.23, 1.07, 2.0],
                [9.0, 0.0, 0.4], [-8.4, -8.4, 1.1], [0.0, 8.1, -2.5], [22.0, 19.0, 0.9]])
ON_WRAP_MAP = (0, 1, 8)
OVER_THE_EDGE = 5                     # x + reach = 15.5 beyond map B's last column at 15.0


def _map_b(pkg_, device):
    """30 m x 30 m at 0.1 m: walls over the whole width (whole 32-bit words, occupied on both sides of every window) next to
    rows with one isolated cell, 20 % occupied cells elsewhere."""
    m = E.MapState.create(30, 30, {"x": 0.0, "y": 0.0}, 0.1, device)
    rs = np.random.RandomState(17)
    occ = rs.random_sample((m.rows, m.cols)) < 0.2
    r = np.arange(m.rows)
    occ[r % WALL_EVERY == 5] = True
    for lone in (4, 6):
        rows = r[r % WALL_EVERY == lone]
        occ[rows] = False
        occ[rows, (37 * rows + 11) % m.cols] = True
    m.upload(np.where(occ, 2, 1), np.full(occ.shape, 2))            # visited / total > 0.5 where occupied (:29-31)
    return m


def _scatter_launches(eng, level, est, ranges, out):
    """One slam2d_match; how many k_occ_scatter and k_endpoints launches the profiler hooks counted in it."""
    L = _lib.lib()
    _lib.check(L.slam2d_prof_enable((1 << _lib.STAGE_SCATTER) | (1 << _lib.STAGE_ENDPOINTS), 8), "slam2d_prof_enable")
    eng.match(level, eng.to_device(est), 3, eng.to_device(ranges), 0.3, None, None, out)
    n = {}
    for st in (_lib.STAGE_SCATTER, _lib.STAGE_ENDPOINTS):
        tot, cnt = C.c_double(0), C.c_int32(0)
        _lib.check(L.slam2d_prof_collect(st, C.byref(tot), C.byref(cnt)), "slam2d_prof_collect")
        n[st] = cnt.value
    L.slam2d_prof_disable()
    return n[_lib.STAGE_SCATTER], n[_lib.STAGE_ENDPOINTS]


def _front_outputs(pkg_, beams, P):
    """The front end's outputs for the nine particles, matched P at a time (the others look at map B from particle 2's pose)."""
    import torch
    z = load_golden("edges.npz")
    unit, R, fov, _, wall = z["wrap_cfg"]
    smP = list(z["wrap_sm"][:7]) + [int(z["wrap_sm"][7])]
    pf = pkg_.ParticleFilter(P, [10, 10, {"x": 0.0, "y": 0.0}, unit, fov, R, beams, wall], smP, growable=False,
                             rng=np.random.RandomState(0), bnb=False)
    eng, level = pf.engine, pf.coarse
    grown, map_b = _wrap_grid(pkg_, z).map, _map_b(pkg_, eng.device)
    assert grown.growth_log == [] and grown.device == eng.device
    for p in range(P):
        eng.maps[p] = grown if p in ON_WRAP_MAP else map_b
    est = np.tile(EST[2], (P, 1))
    est[:MERGED_P] = EST
    ranges = 4.93 - 0.4 * (np.arange(beams) % 5 == 0)
    # a first build somewhere else: what it leaves in the images carries the previous generation's stamp and must not count
    eng.match(level, eng.to_device(est + [1.3, -0.7, 0.0]), 3, eng.to_device(ranges), 0.3, None, None, pf.m_coarse)
    torch.cuda.synchronize()
    stale = level.c.occ_gen
    eng.flags.zero_()
    launches = _scatter_launches(eng, level, est, ranges, pf.m_coarse)
    torch.cuda.synchronize()
    flags = eng.flags.cpu().numpy().view(np.uint32)[:MERGED_P].copy()       # (before take_flags, which clears and raises)
    eng.flags.zero_()
    stamp = level.c.occ_gen
    assert stamp not in (0, stale)
    occ = level.t["occ"].cpu().numpy()
    image = level.fmax * level.fpitch
    fb = (occ.size - P * image) // P                                        # the block flags of all particles follow the images
    assert fb * P == occ.size - P * image and fb % (2 * level.tmax) == 0
    maps = []
    for p in range(MERGED_P):
        v, t = eng.maps[p].download()
        maps.append((v / t > 0.5, eng.maps[p].X.copy(), eng.maps[p].Y.copy()))
    return dict(
        launches=launches, flags=flags, frames=level.frames()[:MERGED_P].copy(), step=level.step, maps=maps,
        axis_x=level.t["axis_x"][:MERGED_P].cpu().numpy(), axis_y=level.t["axis_y"][:MERGED_P].cpu().numpy(),
        cells=[occ[p * image:(p + 1) * image].reshape(level.fmax, level.fpitch) == stamp for p in range(MERGED_P)],
        blocks=[occ[P * image + p * fb:P * image + (p + 1) * fb].reshape(2 * level.tmax, -1) == stamp for p in range(MERGED_P)])


_CACHE = {}


@pytest.fixture(params=[90, 234])
def forms(request, pkg):
    """(merged, separate) outputs at 90 beams (k_endpoints<192>) and at 234 (<256>), computed once per beam count."""
    beams = request.param
    if beams not in _CACHE:
        _CACHE[beams] = (_front_outputs(pkg, beams, MERGED_P), _front_outputs(pkg, beams, SEPARATE_P))
    merged, separate = _CACHE[beams]
    # which form ran: slam2d_match's rule restated, and the launches the profiler hooks saw
    assert not (beams >= 512 or MERGED_P >= 128) and (beams >= 512 or SEPARATE_P >= 128)
    assert merged["launches"] == (0, 1) and separate["launches"] == (1, 1)
    return merged, separate


def _axis_definition(coord, lo, step, dim):
    """:32-37 for one axis: truncated index, Python's negative wrap, -1 where NumPy would raise."""
    idx = ((coord - lo) / step).astype(int)
    idx = np.where(idx < 0, idx + dim, idx)
    return np.where((idx < 0) | (idx >= dim), -1, idx)


def _definition(out, p):
    """(axis_x, axis_y, occupied field cells, occupied 8 x 8 blocks) of particle p from its downloaded map and frame."""
    occ, X, Y = out["maps"][p]
    fr = out["frames"][p]
    ax = _axis_definition(X[fr["mx0"]:fr["mx1"]], fr["xlo"], out["step"], fr["fw"])
    ay = _axis_definition(Y[fr["my0"]:fr["my1"]], fr["ylo"], out["step"], fr["fh"])
    rows, cols = np.nonzero(occ[fr["my0"]:fr["my1"], fr["mx0"]:fr["mx1"]])
    fy, fx = ay[rows], ax[cols]
    keep = (fy >= 0) & (fx >= 0)
    cells = np.zeros_like(out["cells"][p])
    cells[fy[keep], fx[keep]] = True
    blocks = np.zeros_like(out["blocks"][p])
    blocks[fy[keep] >> 3, fx[keep] >> 3] = True
    return ax, ay, cells, blocks


def test_the_maps_hold_what_the_scatter_can_get_wrong(forms):
    """The cases the maps were built for are there, in the windows the device chose."""
    out = forms[0]
    lone_rows = walls = 0
    for p in range(MERGED_P):
        occ, X, Y = out["maps"][p]
        fr = out["frames"][p]
        mx0, mx1, my0, my1 = (int(fr[k]) for k in ("mx0", "mx1", "my0", "my1"))
        if p == OVER_THE_EDGE:
            assert mx1 == occ.shape[1] and mx1 - mx0 < 130                    # clipped at the map's last column
            continue
        assert (mx1 - mx0, my1 - my0) == (130, 130) and (my1 - my0) % 24 and (my1 - my0) % 32
        if p in ON_WRAP_MAP:
            continue
        assert mx0 % 32 and mx1 % 32                                          # partial first and last words
        assert occ[my0:my1, mx0 - 1].any() and occ[my0:my1, mx1].any()        # occupied just outside, both sides
        win = occ[my0:my1, mx0:mx1]
        walls += int(win.all(axis=1).sum())
        lone_rows += int((win.sum(axis=1) == 1).sum())
        wall_at = np.nonzero(win.all(axis=1))[0]
        assert ((mx1 >> 5) - ((mx0 + 31) >> 5)) >= 2 and len(wall_at) >= 9    # whole words of a wall, in every block of rows
    assert walls and lone_rows
    wrapped = sum(int((((X[fr["mx0"]:fr["mx1"]] - fr["xlo"]) / out["step"]).astype(int) < 0).sum())
                  for (occ, X, Y), fr in ((out["maps"][p], out["frames"][p]) for p in ON_WRAP_MAP))
    assert wrapped > 0                                                        # leading columns with a negative index


def test_both_forms_write_the_same_front_end(forms):
    merged, separate = forms
    assert merged["frames"].tobytes() == separate["frames"].tobytes()
    assert np.array_equal(merged["flags"], separate["flags"])
    for p in range(MERGED_P):
        fr = merged["frames"][p]
        ncol, nrow = fr["mx1"] - fr["mx0"], fr["my1"] - fr["my0"]
        assert np.array_equal(merged["axis_x"][p, :ncol], separate["axis_x"][p, :ncol])
        assert np.array_equal(merged["axis_y"][p, :nrow], separate["axis_y"][p, :nrow])
        assert np.array_equal(merged["cells"][p], separate["cells"][p])
        assert np.array_equal(merged["blocks"][p], separate["blocks"][p])


@pytest.mark.parametrize("form", [0, 1], ids=["merged", "separate"])
def test_front_end_matches_its_definition(forms, form):
    out = forms[form]
    for p in range(MERGED_P):
        ax, ay, cells, blocks = _definition(out, p)
        assert np.array_equal(out["axis_x"][p, :len(ax)], ax) and np.array_equal(out["axis_y"][p, :len(ay)], ay)
        assert cells.any()
        got, want = out["cells"][p], cells
        assert np.array_equal(got, want), (p, int((got & ~want).sum()), int((want & ~got).sum()))
        assert np.array_equal(out["blocks"][p], blocks), p
        if p in ON_WRAP_MAP[:2]:
            fh, fw = out["frames"][p]["fh"], out["frames"][p]["fw"]
            assert cells[:fh, fw - 3:fw].any() or cells[fh - 3:fh, :fw].any()    # the wrapped cells are in the last columns / rows


@pytest.mark.parametrize("form", [0, 1], ids=["merged", "separate"])
def test_window_over_the_edge_is_flagged_for_that_particle_only(forms, form):
    flags = forms[form]["flags"]
    outside = (flags & _lib.F_WINDOW_OUTSIDE_MAP) != 0
    assert outside.tolist() == [p == OVER_THE_EDGE for p in range(MERGED_P)]
    assert not (flags & _lib.F_FIELD_INDEX).any()
