"""Pose mean and covariance of a match over the whole cube (slam2d_match_moments, ParticleEngine.match_moments,
ScanMatcher.matchMoments, ParticleFilter.match_moments).  Needs an MI355X: run with ``-m gpu``.

Two yardsticks, both evaluated in np.longdouble inside the tests:

(a) the device's own integers -- the fixed-point field, the unique cell lists, the prior planes and the angles are downloaded,
    every score is recomputed in float64 with the library's expression, the moments in long double.  Only exp and the order of
    summation differ: a few ulp per weight over <= 7e4 terms.  Tolerances: sum w relative 1e-10, mean absolute 1e-10 * R,
    covariance absolute 1e-10 * R_i * R_j (R: the largest absolute offset of the coordinate).
(b) the oracle, which carries the reference's semantics: the moments of oracle.MatcherOracle's cube on the same map and scan.
    The field is fixed point at 1 / cost_scale, so a score is off by at most K_max * 0.5 / cost_scale (the quantised field itself
    is bit-exact against the reference's, tests/test_gpu_parity.py::test_field_build_matches_reference, which is the bar that
    suite sets for the field).  eps = 2 * K_max / cost_scale + 1e-9; sum w relative eps, mean absolute 2 eps R, covariance
    absolute 6 eps R_i R_j.
"""
import importlib
import math

import numpy as np
import pytest

from oracle import slam_oracle as so

pytestmark = pytest.mark.gpu

LD = np.longdouble
UNIT, R_MAX, FOV, WALL = 0.1, 4.0, np.pi, 0.5
DIST, PSI = 0.2, 0.3                       # est_moving_dist, a generic heading
BNB_MARGIN = 30.0


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


# ---------------------------------------------------------------------------------------------------------------------
# yardsticks
# ---------------------------------------------------------------------------------------------------------------------
def _moments(w, thetas, ncell, step):
    """Long-double moments of weights w [ntheta, nx, nx] over the offsets (dx, dy, dtheta) from the estimate."""
    w = np.asarray(w, dtype=LD)
    mv = (np.arange(-ncell, ncell + 1) * step).astype(LD)
    d = [np.broadcast_to(mv[None, None, :], w.shape), np.broadcast_to(mv[None, :, None], w.shape),
         np.broadcast_to(np.asarray(thetas, dtype=LD)[:, None, None], w.shape)]
    s = w.sum()
    mean = np.array([(w * c).sum() / s for c in d], dtype=LD)
    cov = np.array([[(w * (d[i] - mean[i]) * (d[j] - mean[j])).sum() / s for j in range(3)] for i in range(3)], dtype=LD)
    return dict(sum_w=s, mean=mean, cov=cov)


def _moments_of_scores(scores, M, thetas, ncell, step):
    return _moments(np.exp((np.asarray(scores) - M).astype(LD)), thetas, ncell, step)


def _device_scores(lv, p):
    """Yardstick (a): every score of particle p's cube from the integers the device holds, in the library's expression
    s = (-((double)sum_k field[cell_k + (iy, ix)] * (1 / cost_scale)) + rv) + tw."""
    F = lv.field_cost(p).astype(np.uint64)
    prior = lv.t["prior"][p].cpu().numpy().reshape(2, lv.nx, lv.nx)
    inv = 1.0 / lv.c.cost_scale
    ar = np.arange(lv.nx)
    out = np.empty((lv.ntheta, lv.nx, lv.nx))
    for it in range(lv.ntheta):
        cy, cx = lv.cells_of(p, it)
        y0, x0 = cy.astype(np.int64) - lv.ncell, cx.astype(np.int64) - lv.ncell
        assert (y0 >= 0).all() and (x0 >= 0).all() and (y0 + lv.nx <= F.shape[0]).all() and (x0 + lv.nx <= F.shape[1]).all()
        acc = F[y0[:, None, None] + ar[None, :, None], x0[:, None, None] + ar[None, None, :]].sum(axis=0, dtype=np.uint64)
        out[it] = (-(acc.astype(np.float64) * inv) + prior[0]) + prior[1]
    return out


class _PairPriorOracle(so.MatcherOracle):
    """The oracle with the heading prior handed in as the (cos, sin) pair the C ABI takes (d_psi_cs), in the oracle's own
    arithmetic (motion_priors): lets a test state a pair no angle produces, e.g. a cosine one ulp above 1."""

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


def _oracle_cube(scene, est, ranges, fine, psi):
    """Yardstick (b): the oracle's cube of one level for one pose estimate."""
    smo = scene["smo"]
    sr, half, sigma, _, _, _, miss, cf = scene["smP"]
    cstep = cf * UNIT
    if fine:
        xr, yr, prob = smo.frameSearchSpace(est[0], est[1], UNIT, sigma, miss ** (2 / cf))
        _, cube, _ = smo.searchToMatch(prob, est[0], est[1], est[2], ranges, xr, yr, cstep, half, UNIT, DIST, psi, fineSearch=True)
    else:
        xr, yr, prob = smo.frameSearchSpace(est[0], est[1], cstep, sigma / cf, miss)
        _, cube, _ = smo.searchToMatch(prob, est[0], est[1], est[2], ranges, xr, yr, sr, half, cstep, DIST, psi, fineSearch=False)
    return cube


def _radii(lv):
    return np.array([lv.ncell * lv.step, lv.ncell * lv.step, np.abs(lv.thetas).max()])


def _check(tag, row, want, Rv, rel_sum, mean_f, cov_f):
    """row: 16 doubles of the device; want: long-double moments.  Prints every figure as a fraction of its bound first."""
    got_cov = np.array([[row[4], row[5], row[6]], [row[5], row[7], row[8]], [row[6], row[8], row[9]]], dtype=LD)
    e_sum = abs(LD(row[0]) - want["sum_w"]) / (rel_sum * want["sum_w"])
    e_mean = np.abs(row[1:4].astype(LD) - want["mean"]) / (mean_f * Rv)
    e_cov = np.abs(got_cov - want["cov"]) / (cov_f * np.outer(Rv, Rv))
    print(f"{tag}: sum_w {float(row[0]):.12g} err/bound {float(e_sum):.3g}; mean err/bound {np.asarray(e_mean, dtype=float).round(4)}; "
          f"cov err/bound max {float(e_cov.max()):.3g}; cov diag {[float(got_cov[i, i]) for i in range(3)]}")
    assert e_sum <= 1, (tag, "sum_w", float(row[0]), float(want["sum_w"]))
    assert (e_mean <= 1).all(), (tag, "mean", row[1:4], want["mean"])
    assert (e_cov <= 1).all(), (tag, "cov", got_cov, want["cov"])


def _check_a(tag, lv, p, row, match):
    assert row[10] == match["best_score"][p] and row[11] == lv.ntheta * lv.nx ** 2 and row[12] == 0 and not row[13:].any()
    want = _moments_of_scores(_device_scores(lv, p), match["best_score"][p], lv.thetas, lv.ncell, lv.step)
    _check(f"{tag} p{p} (a)", row, want, _radii(lv), 1e-10, 1e-10, 1e-10)


def _check_b(tag, lv, p, row, cube):
    assert cube.shape == (lv.ntheta, lv.nx, lv.nx)
    kmax = int(lv.t["kcount"][p].max().item())
    eps = 2 * kmax / lv.c.cost_scale + 1e-9
    want = _moments(np.exp(cube.astype(LD) - LD(cube.max())), lv.thetas, lv.ncell, lv.step)
    _check(f"{tag} p{p} (b) eps {eps:.3g}", row, want, _radii(lv), eps, 2 * eps, 6 * eps)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _scene(pkg, P, beams, size_m, smP, seed):
    """A filter's two levels (bnb wherever applicable) over P copies of one synthetic map, one scan from a free pose and P
    distinct pose estimates around it."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world = synth.make_world(size_m, UNIT, seed=seed, n_boxes=10)
    origin = (-size_m / 2, -size_m / 2)
    v, t = synth.counts_from_world(world)
    ogP = [size_m, size_m, {"x": 0.0, "y": 0.0}, UNIT, FOV, R_MAX, beams, WALL]
    pf = pkg.ParticleFilter(P, ogP, list(smP), growable=False, rng=np.random.RandomState(0), bnb=True)
    for m in pf.engine.maps:
        m.upload(v, t)
    rs = np.random.RandomState(seed + 1)
    px, py, pth = synth.free_pose_near(world, UNIT, origin, rs, spread=0.6)
    px = origin[0] + UNIT * round((px - origin[0]) / UNIT)
    py = origin[1] + UNIT * round((py - origin[1]) / UNIT)
    ranges = synth.raycast(world, UNIT, origin, (px, py, pth), FOV, beams, R_MAX)
    assert (ranges < R_MAX).sum() > beams // 3
    est = np.array([[px + UNIT * ((p * 2) % 5 - 2), py + UNIT * ((p * 3) % 7 - 3), pth + 0.004 * (p - P // 2)] for p in range(P)])
    assert len({(round(e[0], 6), round(e[1], 6)) for e in est}) == P
    ogo = so.GridOracle(size_m, size_m, {"x": 0.0, "y": 0.0}, UNIT, FOV, beams, R_MAX, WALL)
    ogo.visited[:], ogo.total[:] = v, t
    return dict(pf=pf, eng=pf.engine, est=est, ranges=ranges, smP=smP, smo=_PairPriorOracle(ogo, *smP), P=P)


def _astep(beams):
    return FOV / beams


@pytest.fixture(scope="module")
def scene_a(pkg):
    """Cases 1, 4-9: nx = 9, ntheta = 7 at the coarse level (branch and bound), P = 3, 180 beams; the fine level is 5 x 5."""
    sc = _scene(pkg, 3, 180, 14, (0.9, 2.9 * _astep(180), 2, 0.1, 0.25, 0.3, 0.15, 2), seed=3)
    pf, eng, P = sc["pf"], sc["eng"], sc["P"]
    lv = pf.coarse
    assert (lv.nx, lv.ntheta, lv.c.bnb) == (9, 7, 1) and (pf.fine.nx, pf.fine.ntheta) == (5, 7)
    d_est, d_rng = eng.to_device(sc["est"]), eng.to_device(sc["ranges"])
    psi = np.tile([math.cos(PSI), math.sin(PSI)], (P, 1))
    d_psi = eng.to_device(psi)
    # case 1: slam2d_match, branch and bound, the coarse level's priors
    eng.match(lv, d_est, 3, d_rng, DIST, d_psi, None, pf.m_coarse)
    eng.take_flags()
    sc["match1"] = eng.read_matches(pf.m_coarse).copy()
    sc["rows1"] = eng.match_moments(lv, d_est, 3, pf.m_coarse).cpu().numpy()
    sc["rows1_again"] = eng.match_moments(lv, d_est, 3, pf.m_coarse).cpu().numpy()          # case 9
    sc["scores1"] = [_device_scores(lv, p) for p in range(P)]
    sc["want_a1"] = [_moments_of_scores(sc["scores1"][p], sc["match1"]["best_score"][p], lv.thetas, lv.ncell, lv.step) for p in range(P)]
    sc["cube_b1"] = [_oracle_cube(sc, sc["est"][p], sc["ranges"], False, PSI) for p in range(P)]
    sc["kmax1"] = [int(lv.t["kcount"][p].max().item()) for p in range(P)]
    # case 5: the same match with SLAM2D_MATCH_PRUNE_BY_PRIOR
    eng.match(lv, d_est, 3, d_rng, DIST, d_psi, None, pf.m_coarse, prune=True)
    eng.take_flags()
    sc["rows5"] = eng.match_moments(lv, d_est, 3, pf.m_coarse).cpu().numpy()
    # case 4: slam2d_field_build + slam2d_sweep
    eng.field_build(lv, d_est, 3)
    eng.sweep(lv, d_est, 3, d_rng, DIST, d_psi, None, pf.m_coarse)
    eng.take_flags()
    sc["match4"] = eng.read_matches(pf.m_coarse).copy()
    sc["rows4"] = eng.match_moments(lv, d_est, 3, pf.m_coarse).cpu().numpy()
    sc["cube4"] = [lv.cube(p).copy() for p in range(P)]
    # case 8: a NaN heading prior for particle 1 alone
    psi8 = psi.copy()
    psi8[1] = (1.0000000000000002, 0.0)
    eng.match(lv, d_est, 3, d_rng, DIST, eng.to_device(psi8), None, pf.m_coarse)
    eng.take_flags()
    sc["flags8_before"] = eng.flags.cpu().numpy().copy()
    sc["rows8"] = eng.match_moments(lv, d_est, 3, pf.m_coarse).cpu().numpy()
    sc["flags8_after"] = eng.flags.cpu().numpy().copy()
    sc["match8"] = eng.read_matches(pf.m_coarse).copy()
    sc["cube_b8"] = [_oracle_cube(sc, sc["est"][p], sc["ranges"], False, tuple(psi8[p])) for p in range(P)]
    sc["kmax8"] = [int(lv.t["kcount"][p].max().item()) for p in range(P)]
    # case 7: the fine level, no beam returns
    far = np.full(180, R_MAX)
    far[::2] = 1.5 * R_MAX
    eng.match(pf.fine, d_est, 3, eng.to_device(far), DIST, None, None, pf.m_fine)
    eng.take_flags()
    sc["kcount7"] = pf.fine.t["kcount"].cpu().numpy().copy()
    sc["rows7"] = eng.match_moments(pf.fine, d_est, 3, pf.m_fine).cpu().numpy()
    return sc


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def test_case1_after_match_with_branch_and_bound(scene_a):
    """nx = 9 (odd: the last slot of every row holds one valid pose), ntheta = 7, P = 3, 180 beams, coarse priors."""
    lv = scene_a["pf"].coarse
    for p in range(scene_a["P"]):
        row = scene_a["rows1"][p]
        assert row[10] == scene_a["match1"]["best_score"][p] and row[11] == 7 * 81 and row[12] == 0 and not row[13:].any()
        _check(f"case1 p{p} (a)", row, scene_a["want_a1"][p], _radii(lv), 1e-10, 1e-10, 1e-10)
        eps = 2 * scene_a["kmax1"][p] / lv.c.cost_scale + 1e-9
        cube = scene_a["cube_b1"][p]
        want = _moments(np.exp(cube.astype(LD) - LD(cube.max())), lv.thetas, lv.ncell, lv.step)
        _check(f"case1 p{p} (b) eps {eps:.3g}", row, want, _radii(lv), eps, 2 * eps, 6 * eps)
        # the mean pose is the estimate + the mean offset: within the cube, and not at its arg-max by construction
        assert (np.abs(row[1:4]) <= _radii(lv)).all()


def test_case2_small_cube_after_angle_bounds(pkg):
    """nx = 5 and 37 beams: the preceding match scores the fine level by k_sweep_small behind angle bounds (bnb == 3); P = 9,
    so a particle index passes 8 (the XCD interleave of the block index)."""
    sc = _scene(pkg, 9, 37, 14, (0.9, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 2), seed=5)
    pf, eng, P = sc["pf"], sc["eng"], sc["P"]
    lv = pf.fine
    assert lv.nx == 5 and lv.c.bnb == 3 and lv.nx * ((lv.nx + 3) // 4) <= 32
    d_est, d_rng = eng.to_device(sc["est"]), eng.to_device(sc["ranges"])
    d_psi = eng.to_device(np.tile([math.cos(PSI), math.sin(PSI)], (P, 1)))
    E = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    eng.match(pf.coarse, d_est, 3, d_rng, DIST, d_psi, None, pf.m_coarse)
    eng.match(lv, pf.m_coarse, E.MATCH_DOUBLES, d_rng, DIST, None, None, pf.m_fine)
    eng.take_flags()
    coarse, fine = eng.read_matches(pf.m_coarse).copy(), eng.read_matches(pf.m_fine).copy()
    rows = eng.match_moments(lv, pf.m_coarse, E.MATCH_DOUBLES, pf.m_fine).cpu().numpy()
    for p in range(P):
        _check_a("case2", lv, p, rows[p], fine)
        centre = (float(coarse["x"][p]), float(coarse["y"][p]), float(coarse["theta"][p]))
        _check_b("case2", lv, p, rows[p], _oracle_cube(sc, centre, sc["ranges"], True, PSI))


def test_case3_rows_of_41_poses(pkg):
    """nx = 41 (config 2's row length: 11 slots per row, the last with one valid pose; 8 chunks per angle), ntheta = 3, P = 1."""
    sc = _scene(pkg, 1, 180, 16, (2.05, 0.9 * _astep(180), 2, 0.1, 0.25, 0.3, 0.15, 1), seed=7)
    pf, eng = sc["pf"], sc["eng"]
    lv = pf.coarse
    assert (lv.nx, lv.ntheta) == (41, 3) and lv.c.bnb == 1
    d_est, d_rng = eng.to_device(sc["est"]), eng.to_device(sc["ranges"])
    d_psi = eng.to_device(np.array([[math.cos(PSI), math.sin(PSI)]]))
    eng.match(lv, d_est, 3, d_rng, DIST, d_psi, None, pf.m_coarse)
    eng.take_flags()
    match = eng.read_matches(pf.m_coarse).copy()
    rows = eng.match_moments(lv, d_est, 3, pf.m_coarse).cpu().numpy()
    _check_a("case3", lv, 0, rows[0], match)
    _check_b("case3", lv, 0, rows[0], _oracle_cube(sc, sc["est"][0], sc["ranges"], False, PSI))


def test_case4_after_field_build_and_sweep(scene_a):
    """The same field cells and the same lists: the rows equal case 1's bit for bit; and the stored cube -- complete after the
    brute-force sweep -- gives the same moments."""
    lv = scene_a["pf"].coarse
    assert np.array_equal(scene_a["match4"]["best_score"], scene_a["match1"]["best_score"])
    assert np.array_equal(scene_a["match4"]["argmax"], scene_a["match1"]["argmax"])
    assert scene_a["rows4"].tobytes() == scene_a["rows1"].tobytes()
    for p in range(scene_a["P"]):
        want = _moments_of_scores(scene_a["cube4"][p], scene_a["match4"]["best_score"][p], lv.thetas, lv.ncell, lv.step)
        _check(f"case4 p{p} (stored cube)", scene_a["rows4"][p], want, _radii(lv), 1e-10, 1e-10, 1e-10)


def test_case5_after_match_pruned_by_prior(scene_a):
    assert scene_a["rows5"].tobytes() == scene_a["rows1"].tobytes()


def test_case6_consistent_with_the_match(scene_a):
    """sum_w * exp(M) against Slam2dMatch.confidence: the poses branch and bound skipped are all it may lack."""
    lv = scene_a["pf"].coarse
    n = lv.ntheta * lv.nx ** 2
    tol = n * math.exp(-BNB_MARGIN) + 1e-12
    for p in range(scene_a["P"]):
        row, conf = scene_a["rows1"][p], scene_a["match1"]["confidence"][p]
        got = row[0] * math.exp(row[10])
        print(f"case6 p{p}: sum_w * exp(M) {got:.15g} confidence {conf:.15g} rel {abs(got - conf) / conf:.3g} bound {tol:.3g}")
        assert abs(got - conf) <= tol * conf
        assert abs(row[10] + math.log(row[0]) - scene_a["match1"]["log_confidence"][p]) <= 2 * tol


def test_case7_uniform_cube_closed_forms(scene_a):
    """Fine level, every range >= lidarMaxRange: no endpoint cell, every score 0, every weight 1."""
    lv = scene_a["pf"].fine
    assert not scene_a["kcount7"].any()
    n, step, th = lv.ncell, lv.step, lv.thetas.astype(LD)
    Rv = _radii(lv)
    var_t = ((th - th.mean()) ** 2).mean()
    for p in range(scene_a["P"]):
        row = scene_a["rows7"][p]
        print(f"case7 p{p}: {row[:12]}")
        assert row[0] == lv.ntheta * lv.nx ** 2 and row[10] == 0 and row[11] == lv.ntheta * lv.nx ** 2 and row[12] == 0
        assert abs(row[1]) <= 1e-12 * Rv[0] and abs(row[2]) <= 1e-12 * Rv[1]
        assert abs(LD(row[3]) - th.mean()) <= 1e-12 * Rv[2]
        cxx = step * step * n * (n + 1) / 3
        assert abs(row[4] - cxx) <= 1e-12 * cxx and abs(row[7] - cxx) <= 1e-12 * cxx
        assert abs(LD(row[9]) - var_t) <= 1e-12 * var_t
        assert abs(row[5]) <= 1e-12 * Rv[0] * Rv[1] and abs(row[6]) <= 1e-12 * Rv[0] * Rv[2] and abs(row[8]) <= 1e-12 * Rv[1] * Rv[2]


def test_case8_nan_heading_prior(scene_a):
    """d_psi_cs = (1.0000000000000002, 0.0): arccos of a quotient beyond 1 on the pose row through the estimate."""
    lv = scene_a["pf"].coarse
    nan_b = [int(np.isnan(c).sum()) for c in scene_a["cube_b8"]]
    assert nan_b[1] > 0 and nan_b[0] == 0 and nan_b[2] == 0
    rows = scene_a["rows8"]
    print(f"case8: oracle NaN entries {nan_b}, device slot 12 {rows[:, 12]}")
    assert rows[1, 12] == nan_b[1] and np.isnan(rows[1, :10]).all() and rows[1, 11] == lv.ntheta * lv.nx ** 2
    assert np.array_equal(scene_a["flags8_before"], scene_a["flags8_after"])
    for p in (0, 2):                                       # the finite priors of the same launch
        assert rows[p, 12] == 0
        eps = 2 * scene_a["kmax8"][p] / lv.c.cost_scale + 1e-9
        cube = scene_a["cube_b8"][p]
        want = _moments(np.exp(cube.astype(LD) - LD(cube.max())), lv.thetas, lv.ncell, lv.step)
        _check(f"case8 p{p} (b)", rows[p], want, _radii(lv), eps, 2 * eps, 6 * eps)


def test_case9_same_bits_on_every_call(scene_a):
    assert scene_a["rows1"].tobytes() == scene_a["rows1_again"].tobytes()


@pytest.mark.parametrize("ncell", [5, 8])
def test_case11_tile_bounds_without_the_byte_image(pkg, ncell):
    """A branch-and-bound level without Slam2dLevel.gmin2b is bounded by k_bound (the 32-bit minima, from global memory) instead
    of k_bound_lds; no other test takes that kernel.  3 particles, 3 angles, 37 beams; ncell = 5: rows of 11 poses, 33 slots in
    one chunk, the last slot of a row with 3 poses, 3 x 3 pose tiles; ncell = 8: 17 x 17, 85 slots in two chunks, 5 x 5 tiles.
    Against the oracle: arg-max, pick and pose equal; every pose the match scored within the score bound of yardstick (b),
    2 K_max / cost_scale + 1e-9; then the moments of the whole cube by both yardsticks."""
    nx = 2 * ncell + 1
    sc = _scene(pkg, 3, 37, 14, ((ncell + 0.5) * 2 * UNIT, 0.9 * _astep(37), 2, 0.1, 0.25, 0.3, 0.15, 2), seed=5)
    pf, eng, P = sc["pf"], sc["eng"], sc["P"]
    lv = pf.coarse
    assert (lv.nx, lv.ntheta, lv.c.bnb) == (nx, 3, 1) and lv.c.gmin2b
    lv.c.gmin2b = None
    d_est, d_rng = eng.to_device(sc["est"]), eng.to_device(sc["ranges"])
    d_psi = eng.to_device(np.tile([math.cos(PSI), math.sin(PSI)], (P, 1)))
    eng.match(lv, d_est, 3, d_rng, DIST, d_psi, None, pf.m_coarse)
    eng.take_flags()
    match = eng.read_matches(pf.m_coarse).copy()
    rows = eng.match_moments(lv, d_est, 3, pf.m_coarse).cpu().numpy()
    smo = sc["smo"]
    sr, half, sigma, _, _, _, miss, cf = sc["smP"]
    for p in range(P):
        est = sc["est"][p]
        xr, yr, prob = smo.frameSearchSpace(est[0], est[1], cf * UNIT, sigma / cf, miss)
        want, cube, _ = smo.searchToMatch(prob, est[0], est[1], est[2], sc["ranges"], xr, yr, sr, half, cf * UNIT, DIST, PSI)
        am = int(cube.argmax())
        assert (int(match["argmax"][p]), int(match["pick"][p])) == (am, am)
        assert (match["x"][p], match["y"][p], match["theta"][p]) == (want["x"], want["y"], want["theta"])
        dev = lv.cube(p)
        scored = dev != 0.0                                 # (a fresh level's cube is zero; a score never is)
        eps = 2 * int(lv.t["kcount"][p].max().item()) / lv.c.cost_scale + 1e-9
        err = float(np.abs(dev - cube)[scored].max())
        print(f"case11 ncell {ncell} p{p}: {int(scored.sum())} of {scored.size} poses scored, largest error {err:.3g}, bound {eps:.3g}")
        assert scored.reshape(-1)[am] and err <= eps
        _check_a("case11", lv, p, rows[p], match)
        _check_b("case11", lv, p, rows[p], cube)


# ---------------------------------------------------------------------------------------------------------------------
# case 10: the public surface
# ---------------------------------------------------------------------------------------------------------------------
SM_PUBLIC = (0.9, 2.9 * FOV / 180, 2, 0.1, 0.25, 0.3, 0.15, 2)


def _world_and_scan(seed, size_m=14):
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world = synth.make_world(size_m, UNIT, seed=seed, n_boxes=10)
    origin = (-size_m / 2, -size_m / 2)
    poses = synth.random_walk(world, UNIT, origin, 4, seed=seed + 1, step=0.2, max_radius=0.8)
    scans = [synth.raycast(world, UNIT, origin, q, FOV, 180, R_MAX) for q in poses]
    return world, poses, scans


def test_case10_scan_matcher_surface(pkg):
    E = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    _lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world, poses, scans = _world_and_scan(11)
    v, t = synth.counts_from_world(world)

    def grid():
        og = pkg.OccupancyGrid(14, 14, {"x": 0.0, "y": 0.0}, UNIT, FOV, 180, R_MAX, WALL)
        og.set_counts(v, t)
        return og, pkg.ScanMatcher(og, *SM_PUBLIC)

    og, sm = grid()
    with pytest.raises(_lib.Slam2dError):
        sm.matchMoments()                                                    # no match yet
    x, y, th = poses[1]
    est = {"x": x + UNIT, "y": y - UNIT, "theta": th + 0.01, "range": scans[1]}
    matched, conf = sm.matchScan(est, DIST, PSI, 2)
    eng, io = og.engine(), og.engine()._call_io
    for level, lv, d_est, stride, d_match, origin in (
            ("fine", sm.fine_level(), io.m_coarse, E.MATCH_DOUBLES, io.m_fine, [float(sm.last["coarse"][k]) for k in ("x", "y", "theta")]),
            ("coarse", sm.coarse_level(), io.d_in[0:3], 3, io.m_coarse, [est["x"], est["y"], est["theta"]])):
        got = sm.matchMoments(level)
        mom = lv.moments_host(eng.match_moments(lv, d_est, stride, d_match))
        assert got["pose_mean"] == tuple(origin[i] + mom["mean"][0][i] for i in range(3)), level
        assert np.array_equal(got["cov"], mom["cov"][0]) and np.array_equal(got["cov"], got["cov"].T)
        assert got["sum_w"] == mom["sum_w"][0] and mom["nan_count"][0] == 0
        assert got["log_confidence"] == float(sm.last[level]["best_score"]) + math.log(got["sum_w"])
        assert abs(got["log_confidence"] - float(sm.last[level]["log_confidence"])) <= 1e-9
        assert np.linalg.eigvalsh(got["cov"]).min() > -1e-15
    assert sm.matchMoments()["pose_mean"] == sm.matchMoments("fine")["pose_mean"]
    # another grid of the same configuration shares the levels: after ITS match this matcher's moments are gone
    og2, sm2 = grid()
    assert sm2.fine_level() is sm.fine_level()
    sm2.matchScan({"x": x, "y": y + UNIT, "theta": th, "range": scans[1]}, DIST, PSI, 2)
    for level in ("fine", "coarse"):
        with pytest.raises(_lib.Slam2dError, match="another match"):
            sm.matchMoments(level)
    assert np.isfinite(sm2.matchMoments()["cov"]).all()
    sm.matchScan(est, DIST, PSI, 2)                                            # ... and back after its own next match
    assert np.isfinite(sm.matchMoments()["cov"]).all()


def test_case10_particle_filter_surface(pkg):
    _lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    world, poses, scans = _world_and_scan(13)
    v, t = synth.counts_from_world(world)
    readings = [{"x": q[0], "y": q[1], "theta": q[2], "range": list(map(float, s))} for q, s in zip(poses, scans)]
    ogP = [14, 14, {"x": 0.0, "y": 0.0}, UNIT, FOV, R_MAX, 180, WALL]
    P = 4

    def make(groups):
        pf = pkg.ParticleFilter(P, ogP, list(SM_PUBLIC), growable=False, rng=np.random.RandomState(5), bnb=True, groups=groups)
        for m in pf.engine.maps:
            m.upload(v, t)
        return pf

    res = {}
    for groups in (1, 2):
        pf = make(groups)
        assert pf.n_groups == groups
        with pytest.raises(_lib.Slam2dError):
            pf.match_moments()                                               # nothing matched yet
        pf.updateParticles(readings[0], 1)
        pf.updateParticles(readings[1], 2)
        res[groups] = {lvl: pf.match_moments(lvl) for lvl in ("fine", "coarse")}
        mean, cov = res[groups]["fine"]
        assert mean.shape == (P, 3) and cov.shape == (P, 3, 3) and np.isfinite(mean).all() and np.isfinite(cov).all()
        assert np.array_equal(cov, cov.transpose(0, 2, 1))
        assert (np.abs(mean - pf.prev_matched) <= [2 * pf.fine.step * pf.fine.ncell] * 2 + [2 * np.abs(pf.fine.thetas).max()]).all()
        if groups == 2:
            break
        del pf
    for lvl, lv in (("fine", pf.fine), ("coarse", pf.coarse)):
        Rv = _radii(lv)
        (m1, c1), (m2, c2) = res[1][lvl], res[2][lvl]
        for p in range(P):
            assert (np.abs(m2[p] - m1[p]) <= 1e-10 * Rv).all(), (lvl, p)
            assert (np.abs(c2[p] - c1[p]) <= 1e-10 * np.outer(Rv, Rv)).all(), (lvl, p)
    # inside run() a scan's results reach the host after the next scan's speculative match has been enqueued
    seen = []

    def on_scan(count, f, unbalanced):
        try:
            f.match_moments()
            seen.append((count, None))
        except _lib.Slam2dError as e:
            seen.append((count, str(e)))

    pf = make(2)
    pf.run(readings, on_scan=on_scan)
    assert [c for c, _ in seen] == [1, 2, 3, 4]
    assert pf.stats["step_by_step"] == 1                   # (the first scan alone went through the unpipelined calls)
    for count, msg in seen:
        assert msg is not None and "speculative match" in msg and "run()" in msg, (count, msg)
