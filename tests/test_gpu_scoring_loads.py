"""The loads that the scoring kernels issue ahead of their barriers (csrc/slam2d.hip): k_bound_lds<NSET <= 2, false, HOIST> requests
its first angle's kcount, pcells entry, list head and bnb_best before the staging copy; k_blur_clamp requests its first list
entry and the frame with the tile count; k_exact_select's scan gates a thread's bounds by the per-angle maxima.  Every one of them reads memory before it knows how much of it is valid, so the cases sit where that matters:
list lengths around the 64 lanes of the hoisted pcells entry, rows that are not 16-byte aligned, lists of length 0 behind lists
that were full, waves without an angle and with several, a tile list that is stale from the slot of its first entry on, and
both sides of eight bounds per thread.  Needs an MI355X: run with ``-m gpu``.

The helpers follow tests/test_gpu_bound_shapes.py (copied: a test file imports no other test file).  Checks, per match:
the stored bounds against their definition (bound_yardstick.host_bounds: a plain sum over the list in the byte image as it lies
in memory), bit for bit; every bound against the brute-force twin's exact scores of its tile (no tolerance); the match against
the twin's (arg-max, pick, pose equal, log-confidence within 1e-10) and the oracle's (arg-max and pose equal, confidence within
_conf_tol relative); every pose the exact stage scored against the twin's cube, bit for bit.
"""
import importlib
import math
import os

import numpy as np
import pytest

import bound_yardstick as yard
from oracle import slam_oracle as so

pytestmark = pytest.mark.gpu

UNIT, R_MAX, FOV, WALL, SIZE_M = 0.1, 5.0, np.pi, 0.5, 20
DIST = 0.4
BNB_MARGIN = 30.0                   # SLAM2D_BNB_MARGIN (include/slam2d.h)
BEAM_TABLE_MIN = 512                # SLAM2D_BEAM_TABLE_MIN (csrc/slam2d.hip): run-length lists from here
BL_HEAD = 256                       # list-head slot of a hoisting wave, words (csrc/slam2d.hip)
UNSCORED = 1.0                      # no score is positive: what the cube holds before a match wherever that match stores nothing
POSES = [(0.2, -0.3, 0.5), (0.5, 0.0, 0.6), (0.8, 0.2, 0.75)]


def _cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


class _PairPriorOracle(so.MatcherOracle):
    """The oracle with the heading prior handed in as the (cos, sin) pair the C ABI takes (d_psi_cs), in the oracle's own
    arithmetic (motion_priors)."""

    def motion_priors(self, ncell, step, estMovingDist, estMovingTheta, fine):
        if fine or estMovingTheta is None or not isinstance(estMovingTheta, tuple):
            return super().motion_priors(ncell, step, estMovingDist, estMovingTheta, fine)
        rv, _ = super().motion_priors(ncell, step, estMovingDist, None, fine)
        rng_ = np.arange(-ncell, ncell + 1)
        xv, yv = np.meshgrid(rng_, rng_)
        distv = np.sqrt(np.square(xv) + np.square(yv))
        distv[distv == 0] = 0.0001
        c, s = estMovingTheta
        with np.errstate(invalid="ignore"):
            thetav = np.arccos((xv * c + yv * s) / distv)
        return rv, -1 / (2 * self.turnSigma ** 2) * np.square(thetav)


_WORLDS = {}


def _world(size_m, unit, seed=7, n_boxes=10):
    """(world, visited, total) of one synthetic map, made once per module run and never changed."""
    key = (size_m, unit, seed, n_boxes)
    if key not in _WORLDS:
        synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
        world = synth.make_world(size_m, unit, seed=seed, n_boxes=n_boxes, wall_cells=int(round(0.6 / unit)))
        _WORLDS[key] = (world,) + tuple(synth.counts_from_world(world))
    return _WORLDS[key]


def _plan(lv, P):
    """bound_lds_plan (csrc/slam2d.hip) in Python: which instantiation takes the level's bounds, in which launch shape, and
    whether it is the hoisting form (short lists, one or two tile sets; its LDS: the image and a list-head slot per wave)."""
    nbt, gp, lp = (lv.nx + 3) // 4, 4 * lv.tmax, lv.c.g2b_pitch
    image = (gp * lp + 15) & ~15
    rle = lv.kmax >= BEAM_TABLE_MIN and image + nbt * lp < 65536
    bpp = max(1, min(min(4, lv.ntheta), (256 if rle else 128) // P))
    tpb = _cdiv(lv.ntheta, bpp)
    nw = _cdiv(tpb, _cdiv(tpb, 16))
    nset = _cdiv(nbt * nbt, 64)
    hoist = not rle and nset <= 2 and image + nw * BL_HEAD * 4 <= 160 * 1024 - 512
    return dict(nset=nset, rle=rle, bpp=bpp, tpb=tpb, nw=nw, image=image, hoist=hoist)


def _assert_plan(lv, P, nset, hoist=True):
    """The host-visible conditions under which slam2d_match bounds this level by k_bound_lds<nset, false> with the refresh of the
    bound minima folded into it (bound_lds_plan, fold_field_check) -- and by its hoisting form or not.  Returns the plan."""
    assert lv.bnb and lv.bnb_levels == 1 and "gmin2b" in lv.t and lv.c.bnb == 1 and lv.c.gmin2b and lv.c.sync
    assert os.environ.get("SLAM2D_BOUND_LDS", "1") != "0"
    gp, lp, nbt = 4 * lv.tmax, lv.c.g2b_pitch, (lv.nx + 3) // 4
    assert lp >= gp and lp % 16 == 0 and 0 < lv.kmax < BEAM_TABLE_MIN
    assert gp * lp <= 160 * 1024 - 512                                   # the image fits a CU's LDS
    pl = _plan(lv, P)
    assert _cdiv(nbt * nbt, 64) == nset == pl["nset"] and not pl["rle"] and pl["hoist"] == hoist
    assert not (bool(lv.c.freerow) and lv.tmax <= 64 and lv.kmax >= BEAM_TABLE_MIN)       # (sweep_skips: the refresh is folded)
    return pl


def _pair(pkg, P, beams, ncell, half_steps, twin=True):
    """A branch-and-bound filter and its brute-force twin (the whole cube is left in t["cube"]) over P copies of one map;
    search radius (ncell + 0.5) cells, half_steps angular steps of heading to either side, one level."""
    world, v, t = _world(SIZE_M, UNIT)
    ogP = [SIZE_M, SIZE_M, {"x": 0.0, "y": 0.0}, UNIT, FOV, R_MAX, beams, WALL]
    smP = [(ncell + 0.5) * UNIT, half_steps * FOV / beams, 2, 0.1, 0.25, 0.3, 0.15, 1]
    pfs = {}
    for name, bnb in (("bnb", True), ("twin", False)) if twin else (("bnb", True),):
        pf = pkg.ParticleFilter(P, ogP, smP, growable=False, rng=np.random.RandomState(0), bnb=bnb)
        for m in pf.engine.maps:
            m.upload(v, t)
        assert pf.coarse.nx == 2 * ncell + 1 and bool(pf.coarse.bnb) == bnb
        pfs[name] = pf
    ogo = so.GridOracle(SIZE_M, SIZE_M, {"x": 0.0, "y": 0.0}, UNIT, FOV, beams, R_MAX, WALL)
    ogo.visited[:], ogo.total[:] = v, t
    return dict(pfs, lv=pfs["bnb"].coarse, P=P, world=world, beams=beams, origin=(-SIZE_M / 2, -SIZE_M / 2), smP=smP,
                smo=_PairPriorOracle(ogo, *smP))


def _estimates(P, s, k):
    """P estimates for scan s: up to three cells off the pose of the scan before, each with a sub-cell offset of its own."""
    pose = POSES[s - 1]
    return np.array([[pose[0] + UNIT * ((2 * p + k) % 5 - 2) + UNIT * 0.093 * (p + 1) / (P + 1),
                      pose[1] + UNIT * ((3 * p + 2 * k) % 7 - 3) - UNIT * 0.071 * (p + 1) / (P + 1),
                      POSES[s][2] + 0.004 * ((p % 9) - 4)] for p in range(P)])


def _psi(P, s):
    a = math.atan2(POSES[s][1] - POSES[s - 1][1], POSES[s][0] - POSES[s - 1][0]) + 0.013
    return np.tile([math.cos(a), math.sin(a)], (P, 1))


def _real_scan(sc, s):
    """The scan of POSES[s], its returns from 0.3 m inside the wall band, as mapped walls give them."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    r = synth.raycast(sc["world"], UNIT, sc["origin"], POSES[s], FOV, sc["beams"], R_MAX)
    return np.where(r < R_MAX - 0.3, r + 0.3, r)


def _structure_free_scan(sc, s):
    """Every beam returns, from a range of its own between 3.6 and 4.7 m: neighbouring endpoints lie 0.12 m (90 beams) to 0.18 m
    (63) apart along the arc and up to 1.1 m apart in range, more than a 0.1 m cell -- (nearly) every beam ends in a cell of its
    own, a list is as long as the scan."""
    return np.random.RandomState(100 * sc["beams"] + s).uniform(3.6, 4.7, sc["beams"])


def _no_return_scan(sc, s):
    return np.full(sc["beams"], R_MAX)                                   # (a return is a range BELOW lidarMaxRange)


def _match_both(sc, est, ranges, psi, uni):
    """One slam2d_match of the filter and of its twin (if any) on the same inputs; what the checks read, downloaded."""
    out = {}
    for name in ("bnb", "twin"):
        if name not in sc:
            continue
        pf = sc[name]
        eng, lv = pf.engine, pf.coarse
        if name == "bnb":
            lv.t["cube"].fill_(UNSCORED)
        eng.match(lv, eng.to_device(est), 3, eng.to_device(ranges), DIST, eng.to_device(psi),
                  None if uni is None else eng.to_device(uni), pf.m_coarse)
        eng.take_flags()
        out[name] = dict(m=eng.read_matches(pf.m_coarse).copy(), cube=lv.t["cube"].cpu().numpy().copy())
    lv = sc["lv"]
    for k in ("bounds", "theta_umax", "kcount", "bnb_best"):
        out[k] = lv.t[k].cpu().numpy().copy()
    return out


def _check_bounds(tag, sc, out, particles=None):
    """The definition, bit for bit (bound_yardstick.host_bounds, from the level as the match left it), and admissibility
    against the twin's exact scores."""
    lv, P = sc["lv"], sc["P"]
    nbt = (lv.nx + 3) // 4
    nbq4 = 4 * _cdiv(nbt, 4)
    assert out["bounds"].shape == (P, lv.ntheta, nbt, nbq4)
    for p in range(P) if particles is None else particles:
        U = out["bounds"][p]
        want = yard.host_bounds(lv, p)
        assert np.array_equal(U[:, :, :nbt], want), f"{tag} p{p}: bounds differ from the definition at (angle, tile row, tile column) {np.argwhere(U[:, :, :nbt] != want)[:8].tolist()}"
        assert (U[:, :, nbt:] == -np.inf).all(), f"{tag} p{p}: padding columns"
        assert np.array_equal(out["theta_umax"][p], U[:, :, :nbt].max(axis=(1, 2))), f"{tag} p{p}: theta_umax"
        if "twin" in out:
            best, has_nan = yard.tile_max(out["twin"]["cube"][p], lv.nx, nbt)
            bad = U[:, :, :nbt] < best
            assert not has_nan.any() and not bad.any(), f"{tag} p{p}: bound below an exact score at {np.argwhere(bad)[:8].tolist()}"


def _check_scored(tag, sc, out, may_score_all=False):
    """The match and every scored pose against the twin's.  Some pose must have been left unscored, unless the scan has no
    return (every score is then its prior: whether a tile is cut depends on the priors alone)."""
    P = sc["P"]
    mb, mt = out["bnb"]["m"], out["twin"]["m"]
    for k in ("argmax", "pick", "x", "y", "theta"):
        assert np.array_equal(mb[k], mt[k]), f"{tag}: {k}"
    np.testing.assert_allclose(mb["log_confidence"], mt["log_confidence"], rtol=1e-10)
    cb, ct = out["bnb"]["cube"].reshape(P, -1), out["twin"]["cube"].reshape(P, -1)
    for p in range(P):
        scored = cb[p] != UNSCORED
        assert scored[mb["argmax"][p]] and scored[mb["pick"][p]] and (may_score_all or not scored.all()), f"{tag} p{p}"
        assert np.array_equal(cb[p][scored].view(np.int64), ct[p][scored].view(np.int64)), f"{tag} p{p}: a pose the match scored differs from the sweep's"
        # bnb_best: the largest exact score (every seed is one, and the arg-max tile's bound is the angle's largest or above the threshold)
        assert yard.unorder_bits(out["bnb_best"][p]) <= ct[p].max(), f"{tag} p{p}: bnb_best above the cube's maximum"


def _conf_tol(lv, kmax):
    """Relative bound of the confidence against the oracle's.  A score is a sum over at most kmax cells of the 32-bit fixed-point
    field, one unit = 1 / cost_scale: the project's bound of a score's error is eps = 2 kmax / cost_scale + 1e-9
    (tests/test_gpu_moments.py::_check_b), and the confidence is an exponential of scores, so eps is its relative error
    (expm1); the poses that branch and bound does not score lie more than BNB_MARGIN below the maximum and add at most
    n_poses * exp(-BNB_MARGIN) to a sum that holds exp(0) = 1 for the maximum itself."""
    return math.expm1(2 * int(kmax) / lv.c.cost_scale + 1e-9) + lv.ntheta * lv.nx ** 2 * math.exp(-BNB_MARGIN)


def _check_oracle(tag, sc, out, est, ranges, psi, uni, particles):
    lv, smo = sc["lv"], sc["smo"]
    sr, half, sigma, _, _, _, miss, cf = sc["smP"]
    tol = _conf_tol(lv, out["kcount"].max())
    m = out["bnb"]["m"]
    for p in particles:
        e = est[p]
        with np.errstate(invalid="ignore"):
            xr, yr, prob = smo.frameSearchSpace(e[0], e[1], UNIT, sigma, miss)
            want, cube, conf = smo.searchToMatch(prob, e[0], e[1], e[2], ranges, xr, yr, sr, half, UNIT, DIST,
                                                 (float(psi[p][0]), float(psi[p][1])), fineSearch=False, matchMax=uni is None,
                                                 uniform=None if uni is None else float(uni[p]))
        assert cube.shape == (lv.ntheta, lv.nx, lv.nx)
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
        print(f"{tag} p{p}: confidence {got:.15g} oracle {conf:.15g} rel {abs(got - conf) / conf:.3g} bound {tol:.3g}")
        assert abs(got - conf) <= tol * conf, f"{tag} p{p}: confidence"


# ---------------------------------------------------------------------------------------------------------------------
# k_bound_lds: list lengths at the hoist's edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beams", [63, 64, 65, 90])
@pytest.mark.parametrize("ncell,nset", [(15, 1), (16, 2)])
def test_list_lengths_at_the_hoists_edges(pkg, ncell, nset, beams):
    """Lists as long as the scan, with 63, 64, 65 and 90 beams: the hoisted pcells entry is one per lane, so 64 is the list that
    fills it, 65 the first whose loop fetches a second chunk, 63 the last with a masked lane; kmax = 90 makes rows that start at
    8 bytes modulo 16 and a list head shorter than its slot (the index is clamped to the row).  P = 9 and 7 angles: four blocks
    per particle of two waves, the last block with ONE angle -- its second wave has none and must request nothing it uses.
    Five matches on one level, by arg-max and by a draw alternately: structure-free scans before and after a scan WITHOUT a
    return (K = 0 on every angle while the rows still hold the full lists of the scan before: the clamped, unmasked loads read
    them, the masks must drop them) and the real scan (lists of other lengths).  A scan is shared
    by the particles of a launch (slam2d_match: d_ranges[beams]), so K = 0 cannot be had for one particle alone.
    Vacuous unless the structure-free scans reach K = beams (63, 64, 65) or pass 64 (90)."""
    P = 9
    sc = _pair(pkg, P, beams, ncell, 2.9)
    lv = sc["lv"]
    assert lv.ntheta == 7 and lv.kmax == beams
    pl = _assert_plan(lv, P, nset)
    assert (pl["bpp"], pl["tpb"], pl["nw"]) == (4, 2, 2) and 3 * pl["tpb"] + 1 == lv.ntheta
    rs = np.random.RandomState(beams + ncell)
    kmaxes = []
    for i, (s, scan) in enumerate(((1, _structure_free_scan), (1, _no_return_scan), (2, _structure_free_scan), (2, _real_scan),
                                   (2, _no_return_scan))):
        ranges = scan(sc, s)
        est, psi = _estimates(P, s, s + i), _psi(P, s)
        uni = None if i % 2 == 0 else rs.random_sample(P)
        tag = f"{beams}-{nset} {scan.__name__} {i}"
        out = _match_both(sc, est, ranges, psi, uni)
        K = out["kcount"]
        print(f"{tag}: cells per angle {K.min()} .. {K.max()}, angles with K == beams: {(K == beams).sum()} of {K.size}")
        if scan is _no_return_scan:
            assert (K == 0).all(), tag
        elif scan is _structure_free_scan:
            kmaxes.append(int(K.max()))
            assert (K == beams).sum() * 2 > K.size if beams < 90 else K.max() > 64, f"{tag}: vacuous, lists of {K.min()} .. {K.max()} cells"
        else:
            assert K.max() > 0, tag
        _check_bounds(tag, sc, out)
        _check_scored(tag, sc, out, may_score_all=scan is _no_return_scan)
        if scan is not _no_return_scan:
            _check_oracle(tag, sc, out, est, ranges, psi, uni, (0, 8))
    assert kmaxes and (min(kmaxes) == beams if beams < 90 else min(kmaxes) > 64)


# ---------------------------------------------------------------------------------------------------------------------
# k_bound_lds: several angles per wave against one angle per wave
# ---------------------------------------------------------------------------------------------------------------------
def test_several_angles_per_wave_equal_one_angle_per_wave(pkg):
    """36 angles.  P = 65: one block per particle of twelve waves, three angles per wave -- the first from the hoisted loads, the
    second and third loaded in the loop.  P = 1: four blocks of nine waves, one angle each, all hoisted.  Particles 0, 37 and 64
    of the large launch, each matched alone by a filter of its own with the same inputs in the same order (a level's field and
    bound image are built incrementally: what lies outside the tiles a scan needs is whatever earlier scans left there), must
    give the same bounds, per-angle maxima, threshold, match record and cube, bit for bit; the large launch is also checked
    against its brute-force twin (bounds of particles 0, 37, 64 against the definition)."""
    beams, ncell, P = 90, 16, 65
    sc = _pair(pkg, P, beams, ncell, 17.4)
    lv = sc["lv"]
    pl = _assert_plan(lv, P, 2)
    assert lv.ntheta == 36 and (pl["bpp"], pl["tpb"], pl["nw"]) == (1, 36, 12) and pl["tpb"] > 16
    picks = (0, 37, 64)
    ones = {p: _pair(pkg, 1, beams, ncell, 17.4, twin=False) for p in picks}
    for one in ones.values():
        pl1 = _assert_plan(one["lv"], 1, 2)
        assert (pl1["bpp"], pl1["tpb"], pl1["nw"]) == (4, 9, 9)
    rs = np.random.RandomState(5)
    for s, scan in ((1, _real_scan), (2, _structure_free_scan)):
        ranges = scan(sc, s)
        est, psi = _estimates(P, s, s), _psi(P, s)
        for uni in (None, rs.random_sample(P)):
            tag = f"3-per-wave {scan.__name__} {'argmax' if uni is None else 'draw'}"
            out = _match_both(sc, est, ranges, psi, uni)
            _check_bounds(tag, sc, out, picks)
            _check_scored(tag, sc, out)
            for p in picks:
                o1 = _match_both(ones[p], est[p:p + 1], ranges, psi[p:p + 1], None if uni is None else uni[p:p + 1])
                for k in ("bounds", "theta_umax", "kcount", "bnb_best"):
                    assert np.array_equal(np.atleast_1d(o1[k][0]).view(np.uint8), np.atleast_1d(out[k][p]).view(np.uint8)), f"{tag} p{p}: {k} differs from the particle matched alone"
                for k in out["bnb"]["m"].dtype.names:
                    assert np.array_equal(o1["bnb"]["m"][k][:1], out["bnb"]["m"][k][p:p + 1], equal_nan=True), f"{tag} p{p}: match record, {k}"
                assert np.array_equal(o1["bnb"]["cube"][0].view(np.int64), out["bnb"]["cube"][p].view(np.int64)), f"{tag} p{p}: cube"


# ---------------------------------------------------------------------------------------------------------------------
# k_exact_select: both sides of eight bounds per thread
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncell,nset,per", [(20, 2, 5), (31, 4, 9)])
def test_exact_select_scan_on_both_sides_of_the_gate(pkg, ncell, nset, per):
    """k_exact_select's scan with few and with many bounds per thread: 36 angles of 41 x 41 poses (config 2's cube: 11 x 12 tile
    slots, 4752 bounds, 5 per thread -- a thread's bounds lie in one or two angles) and of 63 x 63 poses (16 x 16 slots, 9216
    bounds, 9 per thread).  Eight per thread is where loading the bounds unconditionally beside the per-angle maxima was tried
    (profiles/r16_scoring_loads.md: not kept); the cases stay as the guard of whatever gates that scan.  Two scans, arg-max and
    draw; bounds, scored poses and matches against the twin for both particles, the oracle for particle 0."""
    beams, P = 90, 2
    sc = _pair(pkg, P, beams, ncell, 17.4)
    lv = sc["lv"]
    _assert_plan(lv, P, nset, hoist=nset <= 2)
    nbt = (lv.nx + 3) // 4
    ntot = lv.ntheta * nbt * 4 * _cdiv(nbt, 4)
    assert lv.ntheta == 36 and _cdiv(ntot, 1024) == per and (per <= 8) == (ncell == 20) and (ntot > 8192) == (ncell == 31)
    rs = np.random.RandomState(ncell)
    for s, scan in ((1, _real_scan), (2, _structure_free_scan)):
        ranges = scan(sc, s)
        est, psi = _estimates(P, s, s), _psi(P, s)
        for uni in (None, rs.random_sample(P)):
            tag = f"per{per} {scan.__name__} {'argmax' if uni is None else 'draw'}"
            out = _match_both(sc, est, ranges, psi, uni)
            _check_bounds(tag, sc, out)
            _check_scored(tag, sc, out)
            _check_oracle(tag, sc, out, est, ranges, psi, uni, (0,))


# ---------------------------------------------------------------------------------------------------------------------
# k_blur_clamp: a list that is stale from its first slot on
# ---------------------------------------------------------------------------------------------------------------------
def test_blur_with_a_stale_list(pkg):
    """A 30 m lidar over a map with an occupied cell every 6 cells, but for one free square (so a free tile pins the field's
    minimum: min_known, the ordinary path), 360 beams with ranges spread evenly over the half disc: more than 256 =
    SLAM2D_BLUR_BLOCKS_PER_PARTICLE tiles are needed and blurred, so some blocks walk a second list entry (the first comes with
    the count, the second is loaded in the loop).  Scan 2 matches the same level with the same inputs against an EMPTY map: the
    triage counts no tile to blur while the list still holds scan 1's entries -- every block has fetched one and must drop it.
    After either scan the field of every tile in scan 1's list equals the oracle's field, and the matches equal the oracle's
    (confidence within _conf_tol relative)."""
    E = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    unit, R, size_m, beams, wall, P = 0.1, 30.0, 80, 360, 0.5, 2
    ogP = [size_m, size_m, {"x": 0.0, "y": 0.0}, unit, np.pi, R, beams, wall]
    smP = [1.0, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 1]
    ranges = (R - 0.5) * np.sqrt(np.random.RandomState(3).uniform(0.01, 1.0, beams))
    est = np.array([[0.1, -0.2, 0.05], [0.3, 0.1, -0.1]])
    pf = pkg.ParticleFilter(P, ogP, smP, growable=False, rng=np.random.RandomState(0), bnb=True)
    lv, eng = pf.coarse, pf.engine
    _assert_plan(lv, P, 1)
    ntile = lv.tmax * lv.tmax
    assert ntile > 256
    ogo = so.GridOracle(size_m, size_m, {"x": 0.0, "y": 0.0}, unit, np.pi, beams, R, wall)
    n = ogo.visited.shape[0]
    assert ogo.visited.shape == (n, n)
    dense_v, dense_t = np.ones((n, n)), np.full((n, n), 2.0)
    dense_v[::6, ::6] += 4; dense_t[::6, ::6] += 4                       # an occupied cell every 6 cells ...
    a, b = n // 2 - 130, n // 2 - 70                                     # ... but for 6 m x 6 m some 10 m off the estimates (a 16-cell
    #                                                                      tile with a free halo inside it wherever the frame's tiles lie)
    dense_v[a:b, a:b], dense_t[a:b, a:b] = 1.0, 2.0
    listed = None
    for scan, (v, t) in enumerate(((dense_v, dense_t), (np.ones((n, n)), np.full((n, n), 5.0)))):
        ogo.visited[:], ogo.total[:] = v, t
        smo = so.MatcherOracle(ogo, *smP)
        for m in eng.maps:
            m.upload(v, t)
        eng.match(lv, eng.to_device(est), 3, eng.to_device(ranges), 0.2, None, None, pf.m_coarse)
        flags = eng.take_flags()
        got = eng.read_matches(pf.m_coarse)
        fr = lv.frames()
        counts = lv.t["tilecount"].cpu().numpy().reshape(P, 2)
        lists = lv.t["tilelist"].cpu().numpy().reshape(P, 2, ntile)
        print(f"scan {scan}: tiles to blur {counts[:, 0].tolist()}, to fill {counts[:, 1].tolist()}, flags {[int(f) for f in flags]}")
        assert all(fr[p]["min_known"] == 1 for p in range(P)) and not any(int(f) & 0x20 for f in flags)
        if scan == 0:
            assert (counts[:, 0] > 256).all(), "vacuous: no block walks a second list entry"
            listed = [lists[p, 0, :counts[p, 0]].copy() for p in range(P)]
        else:
            assert (counts[:, 0] == 0).all()
            for p in range(P):                                           # ... and the blur list is scan 1's, slot for slot
                assert np.array_equal(lists[p, 0, :len(listed[p])], listed[p])
        for p in range(P):
            xr, yr, prob = smo.frameSearchSpace(est[p, 0], est[p, 1], unit, 2, 0.15)
            assert prob.min() == lv.floor_value
            want = E.encode_cost(prob, lv.c.cost_scale)
            field = lv.field_cost(p)
            assert field.shape == want.shape
            for tl in listed[p]:
                ty, tx = divmod(int(tl), lv.tmax)
                sl = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
                assert np.array_equal(field[sl], want[sl]), f"scan {scan} p{p}: field of tile ({ty}, {tx})"
            matched, cube, conf = smo.searchToMatch(prob, est[p, 0], est[p, 1], est[p, 2], ranges, xr, yr, 1.0, 0.25, unit, 0.2,
                                                    None, fineSearch=False, matchMax=True)
            assert int(got["argmax"][p]) == int(cube.argmax()), f"scan {scan} p{p}"
            assert (got["x"][p], got["y"][p], got["theta"][p]) == (matched["x"], matched["y"], matched["theta"])
            tol = _conf_tol(lv, lv.t["kcount"][p].max().item())
            print(f"scan {scan} p{p}: confidence {got['confidence'][p]:.15g} oracle {conf:.15g} rel {abs(got['confidence'][p] - conf) / conf:.3g} bound {tol:.3g}")
            assert abs(got["confidence"][p] - conf) <= tol * conf, f"scan {scan} p{p}: confidence"
