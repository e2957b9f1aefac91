"""The bound kernels that tests/test_gpu_bound_shapes.py does not hold to their definitions (csrc/slam2d.hip): the two levels
k_bound1 / k_seed / k_bound2 (Slam2dLevel.bnb == 2), the angle bounds k_abound / k_aseed / k_sweep_small (bnb == 3), k_bound
(bnb == 1 without the byte image) and the refresh of the bound minima in k_blur_check_redo (gmin2_dirty: the row-wise form and
the 6 x 6-entry form that also writes gmin3d).  Needs an MI355X: run with ``-m gpu``.

Worlds, scans, estimates and the twin are those of test_gpu_bound_shapes.py: every case drives a bound filter and a brute-force
twin (``bnb=False``) with the same inputs.  The definitions (tests/bound_yardstick.py) are taken over the device's OWN images
as they lie in memory after the match -- under the lazy build they hold values of earlier frames outside the needed tiles --
and admissibility is checked against the twin's exact scores, with no tolerance: the kernels' own + 1e-9 is their allowance.

Under two levels Slam2dLevel.bounds depends on the timing by design (every k_bound2 wave reads bnb_best once while other waves
raise it): an entry is either -inf or the definition, it MUST be the definition where its parent's level-1 bound reaches the
cube's largest score less the margin, and it MUST be -inf where the parent lies below the seed's threshold -- no more is
asserted, and no two runs are compared.  seed_key, bounds1 and the final bnb_best do not depend on it
(bound_yardstick.replay_two_level says why).

The host-visible conditions that pick the kernels, their lane layouts and the list lengths are asserted from the level and
from downloaded device state: without them a case could silently exercise another path.
"""
import importlib
import math

import numpy as np
import pytest

import bound_yardstick as yard
from test_gpu_bound_shapes import (BEAM_TABLE_MIN, BNB_MARGIN, FOV, POSES, UNIT, UNSCORED, _assert_plan, _cdiv, _check_oracle, _check_scored,
                                   _close_wall_scan, _estimates, _match_both, _pair, _psi, _real_scan, _staggered_scan)
from test_gpu_parity import _prior_nan_direction

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
PARTIAL = np.dtype([("max", "f8"), ("sumexp", "f8"), ("argmax", "i4"), ("has_nan", "i4")])       # Slam2dPartial
# a (cos, sin) pair no angle produces, a cosine one ulp above 1: thetaWeight is NaN on the pose row through the estimate
# (tests/test_gpu_moments.py::test_case8_nan_heading_prior).  For cubes of 5 x 5 poses _prior_nan_direction finds no direction
# a / hypot(a, b), b / hypot(a, b) (nor does its search up to a, b < 300 over every pose of the plane).
NAN_PAIR = (1.0000000000000002, 0.0)
BIG = dict(unit=0.05, max_range=22.0, size_m=52)        # 0.05 m cells under a 22 m lidar: lists of more than 1024 cells


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


def _margins(stats, name, U, best):
    """Smallest and largest U - best over the finite pairs of one admissibility check, kept per check for the record."""
    ok = np.isfinite(U) & np.isfinite(best)
    if ok.any():
        d = (U - best)[ok]
        lo, hi = stats.get(name, (np.inf, -np.inf))
        stats[name] = (min(lo, float(d.min())), max(hi, float(d.max())))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _top(cube):
    """The largest non-NaN score of a cube (-inf if there is none)."""
    c = np.asarray(cube, dtype=np.float64)
    c = c[~np.isnan(c)]
    return float(c.max()) if c.size else -np.inf


# ---------------------------------------------------------------------------------------------------------------------
# A, B: two levels
# ---------------------------------------------------------------------------------------------------------------------
def _assert_two_level(lv, nb1, nq1, L, C):
    """k_bound1 / k_seed / k_bound2 take the level, in this lane layout of k_bound1 (lane = (cell group g < C, tile row,
    quad of tile columns): L = nb1 * nq1 lanes per cell, C = 64 / L cells per load instruction)."""
    assert lv.bnb and lv.bnb_levels == 2 and lv.c.bnb == 2 and "gmin3d" in lv.t and "gmin2b" not in lv.t and not lv.c.gmin2b
    assert lv.nx >= 17 and lv.ntheta <= 256 and lv.kmax <= 2048
    got = (_cdiv(lv.nx, 8), _cdiv(_cdiv(lv.nx, 8), 4))
    assert got == (nb1, nq1) and got[0] * got[1] == L and 64 // L == C, (got, L, C)


def _check_two_level(tag, sc, out, stats):
    """Checks 1 to 6 of the two-level bounds for every particle; returns (the number of 4 x 4 tiles with a NaN score, the
    replays [(seed_key, seed_best, final_best)])."""
    lv, P = sc["lv"], sc["P"]
    nx, ntheta, scale = lv.nx, lv.ntheta, lv.c.cost_scale
    gp, nbt, nb1 = 4 * lv.tmax, _cdiv(nx, 4), _cdiv(nx, 8)
    nbq4 = 4 * _cdiv(nbt, 4)
    assert out["bounds"].shape == (P, ntheta, nbt, nbq4) and out["bounds1"].shape == (P, ntheta, 64)
    nan_tiles, replays = 0, []
    for p in range(P):
        pcells, kcount, pmax = out["pcells"][p], out["kcount"][p], out["tile_pmax"][p]
        cube = out["twin"]["cube"][p].reshape(ntheta, nx, nx)
        # 1. the two packings of a cell name the same block
        for it in range(ntheta):
            K = int(kcount[it])
            e = pcells[it, :K].astype(np.int64) >> 2
            Y0, X0 = yard.decode_p3(out["p3cells"][p, it, :K], gp)
            assert np.array_equal(Y0, e // gp) and np.array_equal(X0, e % gp), f"{tag} p{p} angle {it}: p3cells"
        # 2. level 1 against its definition over the device's own gmin3d, all 64 entries
        g3 = yard.unphase(out["gmin3d"][p].view(np.uint32), gp)
        gmin2 = out["gmin2"][p].view(np.uint32)
        U1 = out["bounds1"][p].reshape(ntheta, 8, 8)
        want1 = yard.tile1_bounds(g3, pcells, kcount, pmax, scale, gp, nx)
        assert np.array_equal(U1, want1), f"{tag} p{p}: bounds1 differ from the definition at (angle, R, C1) {np.argwhere(U1 != want1)[:8].tolist()}"
        # 3. ... and against the twin's exact scores
        best1, nan1 = yard.tile_max(cube, nx, nb1, size=8)
        B1 = U1[:, :nb1, :nb1]
        assert (B1 >= best1).all(), f"{tag} p{p}: level-1 bound below an exact score at {np.argwhere(B1 < best1)[:8].tolist()}, by up to {(best1 - B1).max():.3g}"
        assert (B1[nan1] == np.inf).all(), f"{tag} p{p}: an 8 x 8 tile with a NaN score has a finite bound"
        _margins(stats, "level 1", B1, best1)
        # 4. the seed's key
        D = yard.tile_bounds32(gmin2, pcells, kcount, pmax, scale, gp, nbt)
        key, seed_best, final_best = yard.replay_two_level(U1, D, pmax, cube, nx)
        got_key = int(out["seed_key"][p:p + 1].view(np.uint64)[0])
        assert got_key == int(key), f"{tag} p{p}: seed_key {got_key:#x}, replayed {int(key):#x}"
        # 5. level 2: -inf or the definition, by the parent's bound
        B = out["bounds"][p]
        assert (B[:, :, nbt:] == -np.inf).all(), f"{tag} p{p}: padding columns"
        Bv = B[:, :, :nbt]
        is_def, is_cut = _bits(Bv) == _bits(D), Bv == -np.inf
        assert (is_def | is_cut).all(), f"{tag} p{p}: a level-2 bound that is neither -inf nor the definition at {np.argwhere(~(is_def | is_cut))[:8].tolist()}"
        ar = np.arange(nbt) >> 1
        parent = U1[:, ar[:, None], ar[None, :]]
        top = _top(cube)
        must = parent >= top - BNB_MARGIN
        assert is_def[must].all(), f"{tag} p{p}: a child of a surviving level-1 tile without its bound at {np.argwhere(must & ~is_def)[:8].tolist()}"
        never = parent < seed_best - BNB_MARGIN
        assert is_cut[never].all(), f"{tag} p{p}: a child of a cut level-1 tile with a bound at {np.argwhere(never & ~is_cut)[:8].tolist()}"
        best2, nan2 = yard.tile_max(cube, nx, nbt)
        assert (Bv[~is_cut] >= best2[~is_cut]).all(), f"{tag} p{p}: level-2 bound below an exact score"
        assert (Bv[nan2] == np.inf).all(), f"{tag} p{p}: a 4 x 4 tile with a NaN score without a +inf bound"
        _margins(stats, "level 2", np.where(is_cut, np.nan, Bv), best2)
        nan_tiles += int(nan2.sum())
        # 6. the threshold k_exact_select works with
        got = float(yard.unorder_bits(out["bnb_best"][p:p + 1].view(np.uint64))[0])
        print(f"{tag} p{p}: seed angle {(int(key) >> 6) & 0xFF} tile {int(key) & 63}, seed_best {seed_best:.6g}, bnb_best {got:.6g}, "
              f"replayed {final_best:.6g}, cube's best {top:.6g}; level-2 bounds stored {int((~is_cut).sum())}, required {int(must.sum())}, "
              f"allowed {int((~never).sum())} of {is_cut.size}")
        assert seed_best <= got <= top, f"{tag} p{p}: bnb_best {got} outside [{seed_best}, {top}]"
        assert _bits([got])[0] == _bits([final_best])[0], f"{tag} p{p}: bnb_best {got!r}, replayed {final_best!r}"
        replays.append((int(key), seed_best, final_best))
    return nan_tiles, replays


# ncell: (nb1, nq1, L, C) of k_bound1
TWO_LEVEL = {8: (3, 1, 3, 21),       # nx 17: 63 lanes busy, one idle; nbt 5
             15: (4, 1, 4, 16),      # nx 31: every lane busy; nbt 8, no child outside the cube
             16: (5, 2, 10, 6),      # nx 33: nbt 9 is odd, the last level-1 row and column have children outside the cube
             24: (7, 2, 14, 4),      # nx 49: eight idle lanes; nbt 13
             31: (8, 2, 16, 4)}      # nx 63: nb1 8, all 64 level-1 tiles inside


@pytest.mark.parametrize("beams", [90, 512])
@pytest.mark.parametrize("ncell", sorted(TWO_LEVEL))
def test_two_levels_against_their_definitions(pkg, monkeypatch, ncell, beams):
    """k_bound1 -> k_seed -> k_bound2 at P = 9 (a particle index passes 8 in xcd_particle) and 7 angles, in every lane layout
    of k_bound1 the accepted cubes have.  Three scans with moved estimates on one level -- the real one, the staggered one
    under the NaN heading prior, the close wall -- each matched by arg-max and by a draw; checks 1 to 7 for all nine particles,
    the oracle for particles 0 and 8 (its draw on the scans without a NaN prior only: np.random.choice takes no NaN
    probabilities).  512 beams: some list must exceed 6 * 16 * 4 cells (a second round of k_bound1's loop at its smallest C),
    some must have at most 16 (children_bounds: slices without a cell)."""
    monkeypatch.setenv("SLAM2D_BNB_LEVELS", "2")
    P = 9
    sc = _pair(pkg, P, beams, ncell, 2.9)
    lv = sc["lv"]
    assert lv.ntheta == 7 and lv.nx == 2 * ncell + 1 and _cdiv(P, 8) * 8 > P
    _assert_two_level(lv, *TWO_LEVEL[ncell])
    nbt = _cdiv(lv.nx, 4)
    assert (nbt % 2 == 1) == (ncell in (8, 16, 24))                     # children outside the cube
    nan_cs = _prior_nan_direction(lv.ncell, lv.step, 0.4, 0.25)
    rs = np.random.RandomState(ncell * 1000 + beams)
    stats, nan_tiles, kmin, kmax = {}, 0, 1 << 30, 0
    for s, scan, nan_prior in ((1, _real_scan, False), (2, _staggered_scan, True), (2, _close_wall_scan, False)):
        ranges = scan(sc, s)
        est = _estimates(P, s, UNIT, s + (scan is _close_wall_scan))
        psi = np.tile(nan_cs, (P, 1)) if nan_prior else _psi(P, s)
        for uni in (None, rs.random_sample(P)):
            tag = f"two-level {ncell}-{beams} {scan.__name__} {'argmax' if uni is None else 'draw'}"
            out = _match_both(sc, est, ranges, psi, uni)
            n, _ = _check_two_level(tag, sc, out, stats)
            _check_scored(tag, sc, out, nan_prior)
            if uni is None or not nan_prior:
                _check_oracle(tag, sc, out, est, ranges, psi, uni, (0, 8))
            assert (n > 0) == nan_prior, tag
            nan_tiles += n
            kmin, kmax = min(kmin, int(out["kcount"].min())), max(kmax, int(out["kcount"].max()))
    print(f"two-level {ncell}-{beams}: cells per angle {kmin} .. {kmax}; (smallest, largest) bound - best score: {stats}")
    assert nan_tiles > 0
    if beams >= BEAM_TABLE_MIN:
        assert kmax > 6 * 16 * 4 and kmin <= 16, (kmin, kmax)


def test_two_levels_list_beyond_one_pass_of_the_seed(pkg, monkeypatch):
    """k_seed walks a list 1024 cells at a time: 2048 beams at 0.05 m cells under a 22 m lidar, where the staggered scan puts
    some 1500 distinct cells on every angle (the 5 m lidar of the other cases bounds a list at 616).  P = 2, 17 x 17 poses,
    seven angles; checks 1 to 7 against the twin.  A particle's level holds 986 x 992 field costs (3.9 MB), its occupancy image
    (1 MB), gmin, gmin2 and gmin3d of 248 x 248 entries (0.74 MB together), two lists of 7 x 2048 offsets and their p3cells
    (172 KB): some 6 MB."""
    monkeypatch.setenv("SLAM2D_BNB_LEVELS", "2")
    P = 2
    sc = _pair(pkg, P, 2048, 8, 2.9, **BIG)
    lv = sc["lv"]
    assert lv.ntheta == 7 and lv.nx == 17 and lv.kmax == 2048 and lv.tmax == 62
    _assert_two_level(lv, *TWO_LEVEL[8])
    stats = {}
    for s, scan in ((1, _real_scan), (2, _staggered_scan)):
        ranges = scan(sc, s)
        est = _estimates(P, s, sc["unit"], s)
        for uni in (None, np.random.RandomState(s).random_sample(P)):
            tag = f"two-level long lists {scan.__name__} {'argmax' if uni is None else 'draw'}"
            out = _match_both(sc, est, ranges, _psi(P, s), uni)
            _, replays = _check_two_level(tag, sc, out, stats)
            _check_scored(tag, sc, out)
    for p, (key, _, _) in enumerate(replays):                           # (the staggered scan's)
        K = int(out["kcount"][p, (key >> 6) & 0xFF])
        print(f"two-level long lists p{p}: seed angle {(key >> 6) & 0xFF} with {K} cells; all angles {out['kcount'][p].tolist()}")
        assert key and K > 1024
    print(f"two-level long lists: (smallest, largest) bound - best score: {stats}")


# ---------------------------------------------------------------------------------------------------------------------
# C: angle bounds
# ---------------------------------------------------------------------------------------------------------------------
def _check_angle(tag, sc, out, stats):
    """Every check of the angle bounds for every particle; returns the number of planes left unscored."""
    lv, P = sc["lv"], sc["P"]
    ntheta, npose, gp = lv.ntheta, lv.nx ** 2, 4 * lv.tmax
    assert out["bounds"].shape == (P, ntheta) and lv.npartial == ntheta
    mb, mt = out["bnb"]["m"], out["twin"]["m"]
    for k in ("argmax", "pick", "x", "y", "theta"):
        assert np.array_equal(mb[k], mt[k]), f"{tag}: {k}"
    np.testing.assert_allclose(mb["log_confidence"], mt["log_confidence"], rtol=1e-10, equal_nan=True)
    skipped = 0
    for p in range(P):
        U = out["bounds"][p]
        want = yard.angle_bounds(out["gmin2"][p].view(np.uint32), out["pcells"][p], out["kcount"][p], out["prior"][p], lv.c.cost_scale,
                                 gp, lv.fine)
        assert np.array_equal(U, want), f"{tag} p{p}: bounds {U.tolist()} differ from the definition {want.tolist()}"
        planes = out["twin"]["cube"][p].reshape(ntheta, npose)
        has_nan = np.isnan(planes).any(axis=1)
        best = np.where(np.isnan(planes), -np.inf, planes).max(axis=1)
        assert (U >= best).all(), f"{tag} p{p}: bound below an exact score at angles {np.flatnonzero(U < best).tolist()}"
        assert (U[has_nan] == np.inf).all(), f"{tag} p{p}: a plane with a NaN score has a finite bound"
        _margins(stats, "angle", U, best)
        key, seed_it, seed_best = yard.replay_angle(U, planes)
        got_key = int(out["seed_key"][p:p + 1].view(np.uint64)[0])
        assert got_key == int(key), f"{tag} p{p}: seed_key {got_key:#x}, replayed {int(key):#x}"
        got_best = int(out["bnb_best"][p:p + 1].view(np.uint64)[0])
        assert got_best == int(yard.order_bits(seed_best)), f"{tag} p{p}: bnb_best {float(yard.unorder_bits(np.uint64(got_best)))!r}, replayed {seed_best!r}"
        scored = U >= seed_best - BNB_MARGIN
        assert scored[int(mb["argmax"][p]) // npose] and scored[int(mb["pick"][p]) // npose]
        got = out["bnb"]["cube"][p].reshape(ntheta, npose)
        parts = out["partials"][p].reshape(-1).view(PARTIAL)[:ntheta]
        for it in range(ntheta):
            if scored[it]:
                ok = ~np.isnan(planes[it])
                assert np.array_equal(np.isnan(got[it]), ~ok) and np.array_equal(_bits(got[it][ok]), _bits(planes[it][ok])), \
                    f"{tag} p{p} angle {it}: a scored plane differs from the sweep's"
            else:
                assert (got[it] == UNSCORED).all(), f"{tag} p{p} angle {it}: a plane below the threshold was written"
                pt = parts[it]
                assert (pt["max"], pt["sumexp"], pt["argmax"], pt["has_nan"]) == (-np.inf, 0.0, INT_MAX, 0), f"{tag} p{p} angle {it}: {pt}"
        skipped += int((~scored).sum())
        print(f"{tag} p{p}: seed angle {seed_it}, best {seed_best:.6g}, bounds {U.min():.6g} .. {U.max():.6g}, {int((~scored).sum())} of {ntheta} planes skipped, "
              f"{int(out['kcount'][p].min())} .. {int(out['kcount'][p].max())} cells")
    return skipped


def _near_estimates(P, s, unit, k, astep):
    """P estimates for scan s as a level of 3 x 3 or 5 x 5 poses needs them: within a cell of the scan's true pose, each with a
    sub-cell offset of its own, and at a heading from which one of the level's angles ((i - h.9) steps, i = 0, 1, ...) is the
    true one.  (_estimates start from the pose of the scan before, four cells away: such a level never reaches the walls from
    there and no plane stands out; and half a step off the true heading the far endpoints of a 22 m scan sit half a cell off
    their walls, enough cost for the field's fixed-point rounding to move the confidence by 1.2e-9.)"""
    pose = POSES[s]
    return np.array([[pose[0] + unit * ((2 * p + k) % 3 - 1) + unit * 0.093 * (p + 1) / (P + 1),
                      pose[1] + unit * ((3 * p + 2 * k) % 3 - 1) - unit * 0.071 * (p + 1) / (P + 1),
                      pose[2] + astep * (0.9 - (p % 5 - 2))] for p in range(P)])


def _on_wall_scan(sc, s):
    """The real scan of POSES[s] without the returns that, seen from that pose, end on a cell of the fine level's field with a
    cost: one beam in sixteen grazes a wall or ends beside a corner.  Every cell of the remaining 770 returns costs exactly 0 at
    the true pose.  With them in, the best pose of the 1081-beam case scores -130 over some forty such cells and the
    fixed-point rounding of their costs alone moves the confidence by 2.5e-9 relative (measured), past the 1e-9 that the
    confidence bound grants the field: the thin-wall effect of tests/test_gpu_bound_shapes.py::_world, from another cause."""
    r = _real_scan(sc, s)
    smo, (x, y, th) = sc["smo"], POSES[s]
    _, _, sigma, _, _, _, miss, cf = sc["smP"]
    xr, yr, prob = smo.frameSearchSpace(x, y, sc["unit"], sigma, miss ** (2 / cf))
    ang = np.linspace(th - FOV / 2, th + FOV / 2, len(r))
    hit = r < sc["max_range"]
    cx = ((x + r * np.cos(ang) - xr[0]) / sc["unit"]).astype(int)
    cy = ((y + r * np.sin(ang) - yr[0]) / sc["unit"]).astype(int)
    cost = np.zeros(len(r), dtype=bool)
    cost[hit] = prob[cy[hit], cx[hit]] < 0
    assert 0 < cost.sum() < len(r) // 8
    return np.where(cost, 1.5 * sc["max_range"], r)


def _assert_angle(lv, P, nx, ntheta, blocks_per_particle):
    """k_abound / k_aseed / k_sweep_small(pruned) take the level: the small-cube path behind angle bounds."""
    assert not lv.bnb and lv.abound and lv.bnb_levels == 3 and lv.c.bnb == 3 and lv.c.seed_key and lv.c.gmin2 and "tile_pmax" not in lv.t
    assert (lv.nx, lv.ntheta) == (nx, ntheta) and lv.nx * _cdiv(lv.nx, 4) <= 32            # nslot <= 32
    assert _cdiv(lv.ntheta, 16) == blocks_per_particle and _cdiv(P, 8) * 8 > P          # blocks of k_abound: ABOUND_WAVES angles each


ANGLE = {"fine5": dict(beams=37, ncell=4, half=2.9, cf=2, level="fine", nx=5, ntheta=7, blocks=1, world={}, kmin=0, skips=False),
         "coarse5": dict(beams=90, ncell=2, half=7.9, cf=1, level="coarse", nx=5, ntheta=17, blocks=2, world={}, kmin=0, skips=False),
         "coarse5_wide": dict(beams=90, ncell=2, half=31.9, cf=1, level="coarse", nx=5, ntheta=65, blocks=5, world={}, kmin=0, skips=True),
         "fine3_long_lists": dict(beams=1081, ncell=4, half=2.9, cf=1, level="fine", nx=3, ntheta=7, blocks=1, world=BIG, kmin=512, skips=True)}


@pytest.mark.parametrize("case", sorted(ANGLE))
def test_angle_bounds_against_their_definition(pkg, case):
    """k_abound -> k_aseed -> k_sweep_small(pruned) at P = 9.  fine5: the fine level of 5 x 5 poses behind a coarse factor of 2,
    pmx = 0, one partial block of 16 angles.  coarse5: a coarse level of 5 x 5 poses, 17 angles -- the second block holds one --
    with a real heading prior and with NAN_PAIR on the staggered scan; nothing is skipped there (the bounds of 75 cells span
    25), so coarse5_wide has 65 angles, five blocks, and some 200 skipped planes.  fine3_long_lists: 3 x 3 poses behind 1081
    beams at 0.05 m cells under a 22 m lidar: lists of more than 512 cells in every match (asserted), the second round of
    k_abound's 64 x 8 loop; the scans are _on_wall_scan and the staggered one, whose scores near -1650 leave the reference
    without a draw (a confidence of 0).  Estimates are _near_estimates: these levels reach one or two cells.  After every
    match, for every particle: the bounds equal the definition bit for bit and dominate the twin's planes; seed_key and
    bnb_best equal the replay's; exactly the planes with U >= best - 30 are scored, bit-equal to the twin's, every other
    plane's cube untouched and its partial "nothing here".  The match equals the twin's, and the oracle's for particles 0
    and 8: confidence within ntheta * 25 * exp(-30) + 1e-9 relative."""
    c = ANGLE[case]
    P = 9
    sc = _pair(pkg, P, c["beams"], c["ncell"], c["half"], cf=c["cf"], level=c["level"], **c["world"])
    lv = sc["lv"]
    _assert_angle(lv, P, c["nx"], c["ntheta"], c["blocks"])
    assert lv.fine == (c["level"] == "fine")
    tol = lv.ntheta * 25 * math.exp(-BNB_MARGIN) + 1e-9
    rs = np.random.RandomState(len(case))
    stats, skipped, nan_planes, kmax = {}, 0, 0, 0
    scans = ((1, _real_scan, False), (2, _staggered_scan, not lv.fine), (2, _close_wall_scan, False))
    if c["world"]:
        scans = ((1, _on_wall_scan, False), (2, _staggered_scan, False))
    for s, scan, nan_prior in scans:
        ranges = scan(sc, s)
        k = s + (scan is _close_wall_scan)
        est = _near_estimates(P, s, sc["unit"], k, math.pi / c["beams"])
        psi = None if lv.fine else (np.tile(NAN_PAIR, (P, 1)) if nan_prior else _psi(P, s))
        for uni in (None, rs.random_sample(P)):
            tag = f"angle {case} {scan.__name__} {'argmax' if uni is None else 'draw'}"
            out = _match_both(sc, est, ranges, psi, uni)
            skipped += _check_angle(tag, sc, out, stats)
            n = int(np.isnan(out["twin"]["cube"]).reshape(P * lv.ntheta, -1).any(axis=1).sum())
            assert (n > 0) == nan_prior, tag
            nan_planes += n
            # the reference has a draw only where its probabilities are numbers: no NaN prior, and a best score whose
            # exponential is a normal double (a staggered scan of 800 cells misses the walls by -3000)
            if uni is None or (not nan_prior and out["twin"]["m"]["best_score"][[0, 8]].min() > -700.0):
                _check_oracle(tag, sc, out, est, ranges, psi, uni, (0, 8), tol=tol)
            assert int(out["kcount"].max()) > c["kmin"], (tag, out["kcount"].max(axis=1).tolist())
            kmax = max(kmax, int(out["kcount"].max()))
    print(f"angle {case}: {skipped} planes skipped, {nan_planes} NaN planes, longest list {kmax}; (smallest, largest) bound - best score: {stats}")
    assert (nan_planes > 0) == (not lv.fine) and (skipped > 0 or not c["skips"])


# ---------------------------------------------------------------------------------------------------------------------
# D: k_bound
# ---------------------------------------------------------------------------------------------------------------------
def _check_bound32(tag, sc, out, stats):
    lv, P = sc["lv"], sc["P"]
    gp, nbt = 4 * lv.tmax, _cdiv(lv.nx, 4)
    nbq4 = 4 * _cdiv(nbt, 4)
    assert out["bounds"].shape == (P, lv.ntheta, nbt, nbq4)
    nan_tiles = 0
    for p in range(P):
        U = out["bounds"][p]
        want = yard.tile_bounds32(out["gmin2"][p].view(np.uint32), out["pcells"][p], out["kcount"][p], out["tile_pmax"][p], lv.c.cost_scale, gp, nbt)
        assert np.array_equal(U[:, :, :nbt], want), f"{tag} p{p}: bounds differ from the definition at (angle, tile row, tile column) {np.argwhere(U[:, :, :nbt] != want)[:8].tolist()}"
        assert (U[:, :, nbt:] == -np.inf).all(), f"{tag} p{p}: padding columns"
        if lv.c.theta_umax:
            assert np.array_equal(out["theta_umax"][p], U[:, :, :nbt].max(axis=(1, 2))), f"{tag} p{p}: theta_umax"
        best, has_nan = yard.tile_max(out["twin"]["cube"][p], lv.nx, nbt)
        bad = U[:, :, :nbt] < best
        assert not bad.any(), f"{tag} p{p}: bound below an exact score at {np.argwhere(bad)[:8].tolist()}, by up to {(best - U[:, :, :nbt])[bad].max():.3g}"
        assert (U[:, :, :nbt][has_nan] == np.inf).all(), f"{tag} p{p}: a tile with a NaN score has a finite bound"
        _margins(stats, "k_bound", U[:, :, :nbt], best)
        nan_tiles += int(has_nan.sum())
    return nan_tiles


@pytest.mark.parametrize("ncell,beams", [(16, 90), (31, 90), (16, 512)])
def test_k_bound_against_its_definition(pkg, monkeypatch, ncell, beams):
    """k_bound (one level, the 32-bit minima from global memory: the level without its byte image, as
    tests/test_gpu_moments.py::test_case11 takes it away) at P = 9 and 7 angles.  ncell 16: nbt 9, three lanes per tile row,
    27 lanes busy; ncell 31: nbt 16 = nbq4, all 64 lanes.  512 beams: lists of more than 64 cells (a second round of the
    list), of a length that is no multiple of 32, and one whose last 64 cells end in the first batch of 32 (the second is
    skipped).  The same scans, checks and oracle as the two-level cases, with bounds that are the definition everywhere."""
    monkeypatch.setenv("SLAM2D_BNB_LEVELS", "1")
    P = 9
    sc = _pair(pkg, P, beams, ncell, 2.9)
    lv = sc["lv"]
    assert lv.bnb and lv.bnb_levels == 1 and lv.c.bnb == 1 and lv.c.gmin2b and lv.ntheta == 7
    lv.c.gmin2b = None
    assert not lv.c.gmin2b and lv.c.gmin2 and lv.c.theta_umax
    nbt = _cdiv(lv.nx, 4)
    nq = _cdiv(nbt, 4)
    assert (nbt, nq, nbt * nq) == {16: (9, 3, 27), 31: (16, 4, 64)}[ncell]
    nan_cs = _prior_nan_direction(lv.ncell, lv.step, 0.4, 0.25)
    rs = np.random.RandomState(ncell + beams)
    stats, nan_tiles, met = {}, 0, set()
    for s, scan, nan_prior in ((1, _real_scan, False), (2, _staggered_scan, True), (2, _close_wall_scan, False)):
        ranges = scan(sc, s)
        est = _estimates(P, s, UNIT, s + (scan is _close_wall_scan))
        psi = np.tile(nan_cs, (P, 1)) if nan_prior else _psi(P, s)
        for uni in (None, rs.random_sample(P)):
            tag = f"k_bound {ncell}-{beams} {scan.__name__} {'argmax' if uni is None else 'draw'}"
            out = _match_both(sc, est, ranges, psi, uni)
            n = _check_bound32(tag, sc, out, stats)
            _check_scored(tag, sc, out, nan_prior)
            if uni is None or not nan_prior:
                _check_oracle(tag, sc, out, est, ranges, psi, uni, (0, 8))
            assert (n > 0) == nan_prior, tag
            nan_tiles += n
            K = out["kcount"]
            met |= ({"long"} if ((K > 64) & (K % 32 != 0)).any() else set()) | ({"half"} if ((K > 64) & (K % 64 > 0) & (K % 64 <= 32)).any() else set())
    print(f"k_bound {ncell}-{beams}: list conditions met {sorted(met)}; (smallest, largest) bound - best score: {stats}")
    assert nan_tiles > 0
    if beams >= BEAM_TABLE_MIN:
        assert met == {"long", "half"}, sorted(met)


# ---------------------------------------------------------------------------------------------------------------------
# E: the bound minima behind k_blur_check_redo
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["entries_6x6_two_levels", "rowwise_one_level_512"])
def test_refreshed_minima_equal_host_recompute(pkg, monkeypatch, form):
    """gmin2_dirty inside k_blur_check_redo, in the style of tests/test_gpu_bound_refresh.py::test_device_minima_equal_host_
    recompute (which covers the copy of this arithmetic in k_bound_lds's prologue).  entries_6x6_two_levels: bnb == 2, 6 x 6
    entries per listed tile, gmin3d beside gmin2.  rowwise_one_level_512: bnb == 1 at 512 beams, where the sweeps skip
    constant patches (sweep_skips), so the refresh is NOT folded into k_bound_lds: 5 x 5 entries per tile, a row per thread,
    tiles on the image's border entry by entry.  Seven scans, P = 3, every range 4.85 to 4.95 m under the 5 m lidar and the
    heading a quarter turn further at every scan: the needed tiles reach the first and the last tile row and column of the
    image (some 142 field cells a side, nine tiles; an endpoint's window reaches 49 + 15 cells from the centre at 71).  After every scan,
    for every entry within the reach of a listed tile: gmin2 == min2x2(gmin) >> 12, the byte image >> 24, gmin3d ==
    min3x3(gmin) >> 12, bit for bit; and the whole of each image equals a host copy updated at those entries only."""
    two = form == "entries_6x6_two_levels"
    monkeypatch.setenv("SLAM2D_BNB_LEVELS", "2" if two else "1")
    P, beams = 3, 90 if two else 512
    sc = _pair(pkg, P, beams, 15, 2.9)
    pf, lv = sc["bnb"], sc["lv"]
    eng = pf.engine
    if two:
        _assert_two_level(lv, *TWO_LEVEL[15])
    else:
        _assert_plan(lv, P, 1, True)
        assert lv.c.freerow and lv.tmax <= 64 and lv.kmax >= 512          # sweep_skips: fold_field_check says no
    gp, tmax, lo = 4 * lv.tmax, lv.tmax, 2 if two else 1
    assert tmax == 9 and 136 < lv.fmax <= 144
    names = ["gmin2"] + (["gmin3d"] if two else ["gmin2b"])
    running = {k: lv.t[k].cpu().numpy().copy() for k in names}          # zeros: the images as allocated
    assert not any(v.any() for v in running.values())
    ranges = 4.9 + 0.05 * np.sin(np.arange(beams))
    seen, touched = set(), 0
    for s in range(7):
        est = np.array([[0.2 * s - 0.7 + 0.1 * p + 0.013 * (p + 1), -0.3 + 0.1 * ((3 * s + p) % 5) - 0.021 * (p + 1), 0.1 + s * math.pi / 2 + 0.2 * p]
                        for p in range(P)])
        psi = np.tile([math.cos(0.3), math.sin(0.3)], (P, 1))
        eng.match(lv, eng.to_device(est), 3, eng.to_device(ranges), 0.4, eng.to_device(psi), None, pf.m_coarse)
        eng.take_flags()
        assert np.all(lv.frames()["min_known"] == 1)                     # frames with a free tile: the dirty-entry refresh
        gmin = lv.t["gmin"].cpu().numpy().view(np.uint32)
        now = {k: lv.t[k].cpu().numpy() for k in names}
        lists, counts = lv.t["tilelist"].cpu().numpy(), lv.t["tilecount"].cpu().numpy()
        for p in range(P):
            nb, nf = int(counts[p, 0]), int(counts[p, 1])
            tiles = np.concatenate([lists[p, 0, :nb], lists[p, 1, :nf]])
            assert nb + nf > 0 and tiles.min() >= 0 and tiles.max() < tmax * tmax
            mask = np.zeros((gp, gp), dtype=bool)
            for t in tiles:
                ty, tx = divmod(int(t), tmax)
                mask[max(4 * ty - lo, 0):min(4 * ty + 4, gp), max(4 * tx - lo, 0):min(4 * tx + 4, gp)] = True
                seen |= {n for n, on in (("first row", ty == 0), ("first column", tx == 0), ("last row", ty == tmax - 1), ("last column", tx == tmax - 1)) if on}
            touched += int(mask.sum())
            m2 = yard.min2x2(gmin[p])
            want = {"gmin2": m2 >> 12, "gmin2b": (m2 >> 24).astype(np.uint8), "gmin3d": yard.min3x3(gmin[p]) >> 12}
            for k in names:
                got = now[k][p]
                img = yard.unphase(got.view(np.uint32), gp) if k == "gmin3d" else (got[:, :gp] if k == "gmin2b" else got.view(np.uint32))
                assert np.array_equal(img[mask], want[k][mask]), f"{form} scan {s} particle {p}: {k} at {np.argwhere(mask & (img != want[k]))[:8].tolist()}"
                run = running[k][p]
                if k == "gmin3d":                                       # the host copy in the device's layout: entry (Y, X) -> its phase plane
                    Y, X = np.nonzero(mask)
                    run[((Y & 1) << 1) | (X & 1), Y >> 1, X >> 1] = want[k][mask].astype(np.uint32).view(np.int32)
                elif k == "gmin2b":
                    run[:, :gp][mask] = want[k][mask]
                else:
                    run[mask] = want[k][mask].astype(np.uint32).view(np.int32)
                assert np.array_equal(got, run), f"{form} scan {s} particle {p}: {k} changed outside the listed tiles' reach"
    print(f"{form}: {touched} entries refreshed, border tiles listed: {sorted(seen)}")
    assert touched > 0 and all(v.any() for v in running.values())
    assert seen == {"first row", "first column", "last row", "last column"}, sorted(seen)
