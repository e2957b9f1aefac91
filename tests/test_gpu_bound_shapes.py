"""k_bound_lds<NSET, RLE> at every tile-set width, list form and launch shape (csrc/slam2d.hip: bound_lds_plan), on the smallest
cubes that reach them.  Needs an MI355X: run with ``-m gpu``.

Every case drives a branch-and-bound filter and a brute-force twin (``bnb=False``: the whole cube is left in ``t["cube"]``) with
the same inputs and compares, after every match,

1. the stored bounds with the definition (tests/bound_yardstick.py: a plain sum over the list in the byte image as it lies in
   memory), ``np.array_equal``; padding columns -inf; theta_umax the angle's largest bound;
2. the bounds with the twin's exact scores: U >= every score of the tile, no tolerance (the kernel's own + 1e-9 is its stated
   allowance, the bytes are floors of block minima); +inf over a tile that holds a NaN score;
3. the bounds with the oracle's cube, less the project's score bound eps = 2 K_max / cost_scale + 1e-9
   (tests/test_gpu_moments.py::_check_b);
4. the match with the twin's (arg-max, pick and pose equal, log-confidence within 1e-10) and with the oracle's (arg-max and
   pose equal; confidence within n_poses * exp(-BNB_MARGIN) + 1e-9 relative: what the skipped poses may add,
   tests/test_gpu_moments.py::test_case6_consistent_with_the_match, for this cube's size);
5. every pose the exact stage scored in this match with the twin's cube, bit for bit.

The host-visible conditions that pick the instantiation are asserted first (_assert_plan): without them a case could silently
exercise another one.
"""
import importlib
import math
import os

import numpy as np
import pytest

import bound_yardstick as yard
from oracle import slam_oracle as so
from test_gpu_moments import _PairPriorOracle
from test_gpu_parity import _prior_nan_direction

pytestmark = pytest.mark.gpu

UNIT, R_MAX, FOV, WALL, SIZE_M = 0.1, 5.0, np.pi, 0.5, 20
DIST = 0.4
BNB_MARGIN = 30.0                   # SLAM2D_BNB_MARGIN (include/slam2d.h)
BEAM_TABLE_MIN = 512                # SLAM2D_BEAM_TABLE_MIN (csrc/slam2d.hip): run-length lists from here
UNSCORED = 1.0                      # no score is positive: what the cube holds before a match wherever that match stores nothing
# true poses of three consecutive scans (on the map lattice, inside the free centre of synth.make_world), ~0.4 m apart
POSES = [(0.2, -0.3, 0.5), (0.5, 0.0, 0.6), (0.8, 0.2, 0.75)]

# id: (ncell, NSET)   nx = 2 ncell + 1, nbt = cdiv(nx, 4), NSET = cdiv(nbt^2, 64)
SHAPES = {"s1": (15, 1),     # 31, 8: 64 tiles, every lane of the one set valid
          "s2": (16, 2),     # 33, 9: 81 tiles, 17 lanes valid in the second set
          "s3": (22, 3),     # 45, 12: 144 tiles, 16 lanes valid in the third
          "s4a": (26, 4),    # 53, 14: 196 tiles, 4 lanes valid in the fourth
          "s4b": (31, 4)}    # 63, 16: 256 tiles, all four sets full, nbq4 == nbt, tile index 255, the largest cube accepted


def _cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


_WORLDS = {}


def _world(size_m, unit, seed=7, n_boxes=10):
    """(world, visited, total) of one synthetic map, made once per module run and never changed.  Walls 0.6 m thick: under the
    blur of two cells a thinner wall stays below half the floor value and no endpoint on it scores 0."""
    key = (size_m, unit, seed, n_boxes)
    if key not in _WORLDS:
        synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
        world = synth.make_world(size_m, unit, seed=seed, n_boxes=n_boxes, wall_cells=int(round(0.6 / unit)))
        _WORLDS[key] = (world,) + tuple(synth.counts_from_world(world))
    return _WORLDS[key]


def _plan(lv, P):
    """bound_lds_plan (csrc/slam2d.hip) in Python: which instantiation takes the level's bounds, in which launch shape."""
    nbt, gp, lp = (lv.nx + 3) // 4, 4 * lv.tmax, lv.c.g2b_pitch
    image = (gp * lp + 15) & ~15
    rle = lv.kmax >= BEAM_TABLE_MIN and image + nbt * lp < 65536
    bpp = max(1, min(min(4, lv.ntheta), (256 if rle else 128) // P))
    tpb = _cdiv(lv.ntheta, bpp)
    return dict(nset=_cdiv(nbt * nbt, 64), rle=rle, bpp=bpp, tpb=tpb, nw=_cdiv(tpb, _cdiv(tpb, 16)), image=image)


def _assert_plan(lv, P, nset, rle):
    """The host-visible conditions under which slam2d_match bounds this level by k_bound_lds<nset, rle> (bound_lds_plan), and
    whether the refresh of the bound minima is folded into it (fold_field_check: not where the sweep skips constant patches).
    Returns the plan."""
    assert lv.bnb and lv.bnb_levels == 1 and "gmin2b" in lv.t and lv.c.bnb == 1 and lv.c.gmin2b and lv.c.sync
    assert os.environ.get("SLAM2D_BOUND_LDS", "1") != "0"
    gp, lp, nbt = 4 * lv.tmax, lv.c.g2b_pitch, (lv.nx + 3) // 4
    assert lp >= gp and lp % 16 == 0 and lv.kmax <= 2048
    assert gp * lp <= 160 * 1024 - 512                                   # the image fits a CU's LDS
    pl = _plan(lv, P)
    assert _cdiv(nbt * nbt, 64) == nset == pl["nset"]
    assert (lv.kmax >= BEAM_TABLE_MIN and pl["image"] + nbt * lp < 65536) == rle == pl["rle"]
    skips = bool(lv.c.freerow) and lv.tmax <= 64 and lv.kmax >= BEAM_TABLE_MIN        # sweep_skips
    assert skips == (lv.kmax >= BEAM_TABLE_MIN)                         # refresh = 1 below 512 beams, 0 from there
    return pl


def _pair(pkg, P, beams, ncell, half_steps, unit=UNIT, max_range=R_MAX, size_m=SIZE_M, cf=1, level="coarse"):
    """A branch-and-bound filter and its brute-force twin over P copies of one map; coarse factor cf (1), search radius
    (ncell + 0.5) * step, half_steps angular steps of heading to either side.  level: the level the checks look at -- the
    coarse one of 2 ncell + 1 poses a side, or the fine one behind it (2 cf + 1 poses a side)."""
    world, v, t = _world(size_m, unit)
    ogP = [size_m, size_m, {"x": 0.0, "y": 0.0}, unit, FOV, max_range, beams, WALL]
    smP = [(ncell + 0.5) * unit * cf, half_steps * FOV / beams, 2, 0.1, 0.25, 0.3, 0.15, cf]
    pfs = []
    for bnb in (True, False):
        pf = pkg.ParticleFilter(P, ogP, smP, growable=False, rng=np.random.RandomState(0), bnb=bnb)
        for m in pf.engine.maps:
            m.upload(v, t)
        pfs.append(pf)
    assert pfs[0].coarse.nx == 2 * ncell + 1 == pfs[1].coarse.nx and not pfs[1].coarse.bnb
    ogo = so.GridOracle(size_m, size_m, {"x": 0.0, "y": 0.0}, unit, FOV, beams, max_range, WALL)
    ogo.visited[:], ogo.total[:] = v, t
    return dict(bnb=pfs[0], twin=pfs[1], lv=getattr(pfs[0], level), level=level, P=P, world=world, unit=unit, max_range=max_range,
                beams=beams, origin=(-size_m / 2, -size_m / 2), smP=smP, smo=_PairPriorOracle(ogo, *smP))


def _estimates(P, s, unit, k):
    """P estimates for scan s: up to three cells off the pose of the scan before, each with a sub-cell offset of its own, at
    the scan's heading give or take 0.016 rad (the heading search of seven angles at 512 beams reaches 0.018)."""
    pose = POSES[s - 1]
    return np.array([[pose[0] + unit * ((2 * p + k) % 5 - 2) + unit * 0.093 * (p + 1) / (P + 1),
                      pose[1] + unit * ((3 * p + 2 * k) % 7 - 3) - unit * 0.071 * (p + 1) / (P + 1),
                      POSES[s][2] + 0.004 * (p - P // 2)] for p in range(P)])


def _real_scan(sc, s):
    """The scan of POSES[s], its returns from 0.3 m inside the wall band, as mapped walls give them."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    r = synth.raycast(sc["world"], sc["unit"], sc["origin"], POSES[s], FOV, sc["beams"], sc["max_range"])
    return np.where(r < sc["max_range"] - 0.3, r + 0.3, r)


def _staggered_scan(sc, s):
    """Far, sparse returns: the real scan with every beam pushed out by 0, 0.5, 1.0 or 1.5 m in turn (what lies beyond max_range
    is no return) -- neighbouring beams end more than a 4 x 4 block apart, so nearly every cell of a list starts a run."""
    r = _real_scan(sc, s)
    return np.where(r < sc["max_range"], r + 0.5 * (np.arange(len(r)) % 4), r)


def _close_wall_scan(sc, s):
    """Every range between 0.35 and 0.45 m: some sixteen cells in a handful of blocks (at 0.6 to 0.9 m the thirty cells of a
    list still make more than eight runs)."""
    return 0.4 + 0.05 * np.sin(np.arange(sc["beams"]) * (2 * np.pi / sc["beams"]))


_DOWNLOADS = ("bounds", "theta_umax", "gmin2b", "pcells", "kcount", "tile_pmax", "gmin2", "gmin3d", "p3cells", "bounds1", "seed_key",
              "bnb_best", "prior", "partials")


def _match_both(sc, est, ranges, psi, uni):
    """One slam2d_match of the filter and of its twin on the same inputs; everything the checks read, downloaded."""
    out = {}
    level = sc.get("level", "coarse")
    for name in ("bnb", "twin"):
        pf = sc[name]
        eng, lv = pf.engine, getattr(pf, level)
        buf = pf.m_coarse if level == "coarse" else pf.m_fine
        if name == "bnb":
            lv.t["cube"].fill_(UNSCORED)
        eng.match(lv, eng.to_device(est), 3, eng.to_device(ranges), DIST, None if psi is None else eng.to_device(psi),
                  None if uni is None else eng.to_device(uni), buf)
        eng.take_flags()
        out[name] = dict(m=eng.read_matches(buf).copy(), cube=lv.t["cube"].cpu().numpy().copy())
    lv = sc["lv"]
    for k in _DOWNLOADS:                                                 # (whichever of them the level's bound kernels have)
        if k in lv.t:
            out[k] = lv.t[k].cpu().numpy().copy()
    return out


def _check_bounds(tag, sc, out, particles=None):
    """Points 1 and 2 for every particle: the definition, bit for bit, and admissibility against the twin's exact scores.
    Returns the number of tiles that hold a NaN score."""
    lv, P = sc["lv"], sc["P"]
    gp, nbt = 4 * lv.tmax, (lv.nx + 3) // 4
    nbq4 = 4 * _cdiv(nbt, 4)
    assert out["bounds"].shape == (P, lv.ntheta, nbt, nbq4)
    nan_tiles = 0
    for p in range(P) if particles is None else particles:
        U = out["bounds"][p]
        want = yard.tile_bounds(out["gmin2b"][p], out["pcells"][p], out["kcount"][p], out["tile_pmax"][p], lv.c.cost_scale, gp, nbt)
        assert np.array_equal(U[:, :, :nbt], want), f"{tag} p{p}: bounds differ from the definition at (angle, tile row, tile column) {np.argwhere(U[:, :, :nbt] != want)[:8].tolist()}"
        assert (U[:, :, nbt:] == -np.inf).all(), f"{tag} p{p}: padding columns"
        assert np.array_equal(out["theta_umax"][p], U[:, :, :nbt].max(axis=(1, 2))), f"{tag} p{p}: theta_umax"
        best, has_nan = yard.tile_max(out["twin"]["cube"][p], lv.nx, nbt)
        bad = U[:, :, :nbt] < best
        assert not bad.any(), f"{tag} p{p}: bound below an exact score at {np.argwhere(bad)[:8].tolist()}, by up to {(best - U[:, :, :nbt])[bad].max():.3g}"
        assert (U[:, :, :nbt][has_nan] == np.inf).all(), f"{tag} p{p}: a tile with a NaN score has a finite bound"
        nan_tiles += int(has_nan.sum())
    return nan_tiles


def _check_scored(tag, sc, out, nan_prior=False):
    """Points 4 (twin) and 5 for every particle.  Without a NaN prior some pose must have been left unscored (under one the
    maximum is NaN and no tile is cut)."""
    P = sc["P"]
    mb, mt = out["bnb"]["m"], out["twin"]["m"]
    for k in ("argmax", "pick", "x", "y", "theta"):
        assert np.array_equal(mb[k], mt[k]), f"{tag}: {k}"
    np.testing.assert_allclose(mb["log_confidence"], mt["log_confidence"], rtol=1e-10, equal_nan=True)
    cb, ct = out["bnb"]["cube"].reshape(P, -1), out["twin"]["cube"].reshape(P, -1)
    for p in range(P):
        scored = cb[p] != UNSCORED
        assert scored[mb["argmax"][p]] and scored[mb["pick"][p]] and (nan_prior or not scored.all()), f"{tag} p{p}"
        assert np.array_equal(cb[p][scored], ct[p][scored], equal_nan=True), f"{tag} p{p}: a pose the match scored differs from the sweep's"
        assert np.array_equal(cb[p][scored & ~np.isnan(ct[p])].view(np.int64), ct[p][scored & ~np.isnan(ct[p])].view(np.int64))


def _check_oracle(tag, sc, out, est, ranges, psi, uni, particles, tol=None):
    """Points 3 and 4 (oracle) for the given particles; the draw's pick where uni is given.  The bounds are the level's own:
    per 4 x 4 tile, or per angle plane behind angle bounds (bnb_levels 3); under two levels a tile cut at level 1 holds -inf
    by design and is not compared.  tol: the relative bound of the confidence where it is not this cube's n_poses * exp(-30)."""
    lv = sc["lv"]
    smo = sc["smo"]
    sr, half, sigma, _, _, _, miss, cf = sc["smP"]
    fine = sc.get("level", "coarse") == "fine"
    nbt, n_poses = (lv.nx + 3) // 4, lv.ntheta * lv.nx ** 2
    if tol is None:
        tol = n_poses * math.exp(-BNB_MARGIN) + 1e-9
    m = out["bnb"]["m"]
    for p in particles:
        e = est[p]
        with np.errstate(invalid="ignore"):                              # (the heading as the (cos, sin) pair the device was given)
            if fine:
                xr, yr, prob = smo.frameSearchSpace(e[0], e[1], sc["unit"], sigma, miss ** (2 / cf))
                want, cube, conf = smo.searchToMatch(prob, e[0], e[1], e[2], ranges, xr, yr, cf * sc["unit"], half, sc["unit"], DIST,
                                                     None, fineSearch=True, matchMax=uni is None,
                                                     uniform=None if uni is None else float(uni[p]))
            else:
                xr, yr, prob = smo.frameSearchSpace(e[0], e[1], cf * sc["unit"], sigma / cf, miss)
                want, cube, conf = smo.searchToMatch(prob, e[0], e[1], e[2], ranges, xr, yr, sr, half, cf * sc["unit"], DIST,
                                                     (float(psi[p][0]), float(psi[p][1])), fineSearch=False, matchMax=uni is None,
                                                     uniform=None if uni is None else float(uni[p]))
        assert cube.shape == (lv.ntheta, lv.nx, lv.nx)
        eps = 2 * int(out["kcount"][p].max()) / lv.c.cost_scale + 1e-9      # (_check_b of tests/test_gpu_moments.py)
        if lv.bnb_levels == 3:
            flat = cube.reshape(lv.ntheta, -1)
            has_nan = np.isnan(flat).any(axis=1)
            best = np.where(np.isnan(flat), -np.inf, flat).max(axis=1)
            U = out["bounds"][p]
        else:
            best, has_nan = yard.tile_max(cube, lv.nx, nbt)
            U = out["bounds"][p][:, :, :nbt]
        cut = (U == -np.inf) if lv.bnb_levels == 2 else np.zeros(U.shape, dtype=bool)
        short = (best - eps - U)[~cut]
        print(f"{tag} p{p}: oracle's tile maxima exceed the bounds by at most {short.max():.3g} (0 allowed, eps {eps:.3g} inside); "
              f"{int(has_nan.sum())} NaN tiles")
        assert ((U >= best - eps) | cut).all() and (U[has_nan] == np.inf).all(), f"{tag} p{p}: bounds against the oracle"
        am = int(cube.argmax())
        assert int(m["argmax"][p]) == am, f"{tag} p{p}: arg-max"
        pick = am
        if uni is not None:
            flat = cube.reshape(-1)
            cdf = np.cumsum(np.exp(flat) / np.exp(flat).sum())
            pick = int((cdf / cdf[-1]).searchsorted(float(uni[p]), side="right"))
        assert int(m["pick"][p]) == pick, f"{tag} p{p}: pick"
        assert (m["x"][p], m["y"][p], m["theta"][p]) == (want["x"], want["y"], want["theta"]), f"{tag} p{p}: pose"
        got = float(m["confidence"][p])
        if np.isnan(conf):
            assert np.isnan(got)
        else:
            print(f"{tag} p{p}: confidence {got:.15g} oracle {conf:.15g} rel {abs(got - conf) / conf:.3g} bound {tol:.3g}")
            assert abs(got - conf) <= tol * conf, f"{tag} p{p}: confidence"


def _run_lengths(out, P):
    """From the lists as they lie in memory: per 64-cell chunk (one pass of an RLE wave) the number of runs of equal
    neighbouring blocks -- a run never extends over a chunk's end.  Returns the conditions met:
    a: a chunk of at most 8 runs (one gather batch), b: a chunk of more than 56 (the eighth batch), c: a last chunk of fewer
    than 64 cells, d: equal neighbours on either side of a chunk's end (they count as two runs)."""
    met = set()
    for p in range(P):
        for it in range(out["kcount"].shape[1]):
            K = int(out["kcount"][p, it])
            e = out["pcells"][p, it, :K] >> 2
            for c0 in range(0, K, 64):
                chunk = e[c0:c0 + 64]
                runs = 1 + int((chunk[1:] != chunk[:-1]).sum())
                if runs <= 8:
                    met.add("a")
                if runs > 56:
                    met.add("b")
                if len(chunk) < 64:
                    met.add("c")
                if c0 > 0 and e[c0] == e[c0 - 1]:
                    met.add("d")
    return met


def _psi(P, s):
    a = math.atan2(POSES[s][1] - POSES[s - 1][1], POSES[s][0] - POSES[s - 1][0]) + 0.013
    return np.tile([math.cos(a), math.sin(a)], (P, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the eight instantiations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beams", [90, 512])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_instantiation_at_its_smallest_shape(pkg, shape, beams):
    """k_bound_lds<NSET, beams >= 512> at P = 9 (a particle index passes 8 in xcd_particle, 16 x bpp blocks for 9 particles)
    and 7 angles (four blocks per particle, two angles per block, the last block with one).  Three scans with moved estimates
    on one level -- a real one, the staggered one under the NaN heading prior, the close wall -- each matched by arg-max and by
    a draw.  Bit-for-bit checks for all nine particles, the oracle for particles 0 and 8.  The oracle's draw is compared on
    the scans without a NaN prior only: np.random.choice takes no NaN probabilities, the reference has no draw there.
    512 beams: the lists met in these scans must hold the run-length forms (a) to (d) of _run_lengths -- the close wall gives
    (a), the staggered scan (b), the real scan (d), all of them (c); they are conditions on the inputs, checked on the lists as
    k_endpoints left them.  Measured on the MI355X: confidence within 3.1e-10 relative of the oracle's in every case (bound
    1.6e-9 at s1 to 3.6e-9 at s4b), each case 0.05 to 0.4 s."""
    ncell, nset = SHAPES[shape]
    P = 9
    sc = _pair(pkg, P, beams, ncell, 2.9)
    lv = sc["lv"]
    assert lv.ntheta == 7 and lv.nx == 2 * ncell + 1 and 36 <= 4 * lv.tmax <= 48 and 4 * lv.tmax * lv.c.g2b_pitch < 4096
    pl = _assert_plan(lv, P, nset, beams >= BEAM_TABLE_MIN)
    assert (pl["bpp"], pl["tpb"], pl["nw"]) == (4, 2, 2) and _cdiv(P, 8) * 8 > P
    nan_cs = _prior_nan_direction(lv.ncell, lv.step, DIST, 0.25)
    rs = np.random.RandomState(ncell * 1000 + beams)
    met, nan_tiles = set(), 0
    for s, scan, nan_prior in ((1, _real_scan, False), (2, _staggered_scan, True), (2, _close_wall_scan, False)):
        ranges = scan(sc, s)
        est = _estimates(P, s, UNIT, s + (scan is _close_wall_scan))
        psi = np.tile(nan_cs, (P, 1)) if nan_prior else _psi(P, s)
        for uni in (None, rs.random_sample(P)):
            tag = f"{shape}-{beams} {scan.__name__} {'argmax' if uni is None else 'draw'}"
            out = _match_both(sc, est, ranges, psi, uni)
            n = _check_bounds(tag, sc, out)
            _check_scored(tag, sc, out, nan_prior)
            if uni is None or not nan_prior:
                _check_oracle(tag, sc, out, est, ranges, psi, uni, (0, 8))
            assert (n > 0) == nan_prior, tag
            nan_tiles += n
            met |= _run_lengths(out, P)
    assert nan_tiles > 0
    print(f"{shape}-{beams}: run-length conditions met: {sorted(met)}")
    if beams >= BEAM_TABLE_MIN:
        assert met == {"a", "b", "c", "d"}, sorted(met)


# ---------------------------------------------------------------------------------------------------------------------
# launch shapes the grid above does not reach
# ---------------------------------------------------------------------------------------------------------------------
def _twin_case(pkg, tag, P, beams, ncell, half_steps, nset, rle, scans, check_particles=None, **kw):
    sc = _pair(pkg, P, beams, ncell, half_steps, **kw)
    lv = sc["lv"]
    pl = _assert_plan(lv, P, nset, rle)
    rs = np.random.RandomState(beams + ncell)
    for s, scan in scans:
        ranges = scan(sc, s)
        est = _estimates(P, s, sc["unit"], s)
        for uni in (None, rs.random_sample(P)):
            t = f"{tag} {scan.__name__} {'argmax' if uni is None else 'draw'}"
            out = _match_both(sc, est, ranges, _psi(P, s), uni)
            _check_bounds(t, sc, out, check_particles)
            _check_scored(t, sc, out)
    return sc, pl, out


@pytest.mark.parametrize("beams", [180, 512])
def test_several_angles_per_wave(pkg, beams):
    """Shape s3 with 65 angles at P = 9: four blocks per particle, 17 angles per block in two rounds of nine waves -- every wave
    but the last bounds two angles.  512 beams: an RLE wave keeps ONE seed over its angles, the better of the two."""
    sc, pl, out = _twin_case(pkg, f"tpb17-{beams}", 9, beams, 22, 31.9, 3, beams >= BEAM_TABLE_MIN, [(1, _real_scan)],
                             check_particles=(0, 3, 8))
    assert sc["lv"].ntheta == 65 and (pl["bpp"], pl["tpb"], pl["nw"]) == (4, 17, 9) and pl["tpb"] > 16


def test_cell_list_at_its_limit(pkg):
    """2048 beams (SLAM2D_MAX_BEAMS, the kmax bound_lds_plan accepts) at shape s4b, RLE: the longest lists the kernel takes."""
    sc, pl, out = _twin_case(pkg, "kmax2048", 2, 2048, 31, 2.9, 4, True, [(1, _real_scan), (2, _staggered_scan)])
    lv = sc["lv"]
    assert lv.kmax == 2048 and lv.ntheta == 7 and out["kcount"].max() > 256
    print(f"kmax2048: cells per angle {out['kcount'].min()} .. {out['kcount'].max()}, run-length conditions {sorted(_run_lengths(out, 2))}")


def test_image_beyond_64_kb(pkg):
    """Shape s3 at 0.05 m cells under a 22 m lidar: gp = 256, the byte image 72 KB -- k_bound_lds<3, false> is granted its
    dynamic LDS through hipFuncSetAttribute (grant_dynamic_lds), an instantiation other than config 2's."""
    sc, pl, out = _twin_case(pkg, "image72k", 2, 90, 22, 2.9, 3, False, [(1, _real_scan)], unit=0.05, max_range=22.0, size_m=52)
    lv = sc["lv"]
    gp, lp = 4 * lv.tmax, lv.c.g2b_pitch
    assert (lv.tmax, gp) == (64, 256) and gp * lp > 65536 and gp * lp <= 160 * 1024 - 512
    assert (out["kcount"] > 0).all() and out["gmin2b"].any()


def test_exact_select_scan_at_its_limit(pkg):
    """Shape s4b with 128 angles: 128 x 16 x 16 = 32768 bounds, 32 = XS_MAX_PER per thread of k_exact_select's scan -- the
    largest cube branch and bound accepts (SearchLevel still reports bnb)."""
    sc, pl, out = _twin_case(pkg, "per32", 2, 360, 31, 63.4, 4, False, [(1, _real_scan)])
    lv = sc["lv"]
    nbt = (lv.nx + 3) // 4
    assert lv.ntheta == 128 and lv.ntheta * nbt * 4 * _cdiv(nbt, 4) == 32768 == 1024 * 32 and lv.bnb and lv.c.bnb == 1
