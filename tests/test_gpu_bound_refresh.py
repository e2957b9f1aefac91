"""The bound minima of a level whose bounds k_bound_lds takes (Slam2dLevel.bnb == 1 with the byte image gmin2b): that kernel's
prologue refreshes gmin2 / gmin2b for the tiles written at the build, the separate launch between the blur and the bounds is
gone.  Device state against a host recompute, independence of the launch shape (blocks per particle), and the frame without a
free tile (the blur's last block checks the minimum and redoes the clamp; the bound kernel then refreshes the whole frame).
Needs an MI355X: run with ``-m gpu``.
"""
import importlib
import os

import numpy as np
import pytest

from bound_yardstick import host_bounds as _host_bounds, min2x2 as _min2x2
from oracle import slam_oracle as so

pytestmark = pytest.mark.gpu

F_FLOOR_REDO = 0x20
# confidence against the oracle's: the 32-bit fixed-point field with exact integer sums delivers ~1e-9; poses in tiles that
# branch and bound does not score lie more than the margin (30) below the maximum, all 15 x 21 x 21 of them together add less
# than 6615 * exp(-30) = 6.2e-10 (relative)
RTOL_CONF = 1e-8


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


def _assert_check_launch_folded(lv):
    """The host-visible conditions under which slam2d_match leaves the refresh of the bound minima to k_bound_lds and does not
    launch k_blur_check_redo (csrc/slam2d.hip: fold_field_check, bound_lds_plan) -- without them the tests below would test
    the separate launch, which leaves the same memory."""
    assert lv.bnb_levels == 1 and "gmin2b" in lv.t and lv.c.bnb == 1 and lv.c.gmin2b and lv.c.sync
    assert os.environ.get("SLAM2D_BOUND_LDS", "1") != "0"
    assert not (lv.c.freerow and lv.tmax <= 64 and lv.kmax >= 512)      # no sweep of this level reads freerow (sweep_skips)
    gp, lp, nbt = 4 * lv.tmax, lv.c.g2b_pitch, (lv.nx + 3) // 4
    assert -(-nbt * nbt // 64) <= 4 and lv.kmax <= 2048                  # tile sets per lane, cell list
    assert lp >= gp and lp % 16 == 0                                     # the byte image's pitch
    assert gp * lp <= 160 * 1024 - 512                                   # ... and the image fits a CU's LDS


def _config2_filter(pkg, P, world_seed=3):
    """A config-2-shaped filter (0.1 m cells, 34.5 m / 180 beams, 41 x 41 poses per angle, one level) on a synthetic world:
    its coarse level is scored by branch and bound with the bounds' byte image."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    unit, R, fov, beams, size_m, wall = 0.1, 34.5, np.pi, 180, 90, 0.5
    smP = [2.05, 0.30, 2, 0.1, 0.25, 0.3, 0.15, 1]
    ogP = [size_m, size_m, {"x": 0.0, "y": 0.0}, unit, fov, R, beams, wall]
    world = synth.make_world(size_m, unit, seed=world_seed)
    v, t = synth.counts_from_world(world)
    pf = pkg.ParticleFilter(P, ogP, smP, growable=False, rng=np.random.RandomState(0), bnb=True)
    for m in pf.engine.maps:
        m.upload(v, t)
    lv = pf.coarse
    _assert_check_launch_folded(lv)
    return pf, world, (unit, R, fov, beams, size_m)


def test_device_minima_equal_host_recompute(pkg):
    """Consecutive scans with moving estimates on one level.  After every scan, for every entry within the 5 x 5 reach of a
    tile in the build's two lists: gmin2 == min(2 x 2 of gmin) >> 12 and gmin2b == that minimum >> 24, bit for bit; and the
    WHOLE gmin2b image equals a host image that is updated at those entries only -- nothing else is written, nothing that
    should be written is missed.  After the last scan the tile bounds equal a host recompute from that image."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    P = 3
    pf, world, (unit, R, fov, beams, size_m) = _config2_filter(pkg, P)
    lv, eng = pf.coarse, pf.engine
    origin = (-size_m / 2, -size_m / 2)
    poses = synth.random_walk(world, unit, origin, 8, seed=5, step=0.4, max_radius=2.0)
    rs = np.random.RandomState(9)
    gp, ntile = 4 * lv.tmax, lv.tmax * lv.tmax
    running = lv.t["gmin2b"].cpu().numpy().copy()                       # zeros: the image as allocated
    touched_total = 0
    for s in range(1, len(poses)):
        ranges = synth.raycast(world, unit, origin, poses[s], fov, beams, R)
        est = np.array([[poses[s - 1][0] + unit * rs.randint(-2, 3), poses[s - 1][1] + unit * rs.randint(-2, 3),
                         poses[s][2] + rs.normal(0, 0.02)] for _ in range(P)])
        psi = np.tile([np.cos(0.3), np.sin(0.3)], (P, 1))
        eng.match(lv, eng.to_device(est), 3, eng.to_device(ranges), 0.4, eng.to_device(psi),
                  eng.to_device(rs.random_sample(P)), pf.m_coarse)
        eng.take_flags()
        assert np.all(lv.frames()["min_known"] == 1)                     # frames with a free tile: the dirty-entry refresh
        gmin = lv.t["gmin"].cpu().numpy().view(np.uint32)
        gmin2 = lv.t["gmin2"].cpu().numpy().view(np.uint32)
        gmin2b = lv.t["gmin2b"].cpu().numpy()
        lists = lv.t["tilelist"].cpu().numpy()
        counts = lv.t["tilecount"].cpu().numpy()
        for p in range(P):
            nb, nf = int(counts[p, 0]), int(counts[p, 1])
            tiles = np.concatenate([lists[p, 0, :nb], lists[p, 1, :nf]])
            assert nb > 0 and tiles.min() >= 0 and tiles.max() < ntile
            want = _min2x2(gmin[p])
            mask = np.zeros((gp, gp), dtype=bool)
            for t in tiles:
                ty, tx = divmod(int(t), lv.tmax)
                mask[max(4 * ty - 1, 0):min(4 * ty + 4, gp), max(4 * tx - 1, 0):min(4 * tx + 4, gp)] = True
            touched_total += int(mask.sum())
            assert np.array_equal(gmin2[p][mask], (want >> 12)[mask]), f"scan {s} particle {p}: gmin2"
            assert np.array_equal(gmin2b[p][:, :gp][mask], (want >> 24).astype(np.uint8)[mask]), f"scan {s} particle {p}: gmin2b"
            running[p][:, :gp][mask] = (want >> 24).astype(np.uint8)[mask]
            assert np.array_equal(gmin2b[p], running[p]), f"scan {s} particle {p}: bytes outside the listed tiles' reach changed"
    assert touched_total > 0 and running.any()
    # the LDS side of the refresh: the bounds of the last scan were taken from every block's OWN patched copy of the image -- they
    # must be the bounds of the image as it now lies in memory (a block that staged the image without patching it would have
    # bounded against the previous scan's bytes)
    nbt = (lv.nx + 3) // 4
    for p in range(P):
        got_b = lv.t["bounds"][p].cpu().numpy()[:, :, :nbt]
        assert np.array_equal(got_b, _host_bounds(lv, p)), f"particle {p}: bounds do not match the refreshed image"


def test_results_independent_of_launch_shape(pkg):
    """The same 16 particles alone (four bound blocks per particle), as the first 16 of 64 (two) and as the first 16 of 128
    (one): identical matched pose, arg-max and draw, identical bounds."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    res = []
    for P in (16, 64, 128):
        pf, world, (unit, R, fov, beams, size_m) = _config2_filter(pkg, P)
        lv, eng = pf.coarse, pf.engine
        origin = (-size_m / 2, -size_m / 2)
        poses = synth.random_walk(world, unit, origin, 4, seed=5, step=0.4, max_radius=2.0)
        rs = np.random.RandomState(11)
        out = []
        for s in range(1, len(poses)):
            ranges = synth.raycast(world, unit, origin, poses[s], fov, beams, R)
            est16 = np.array([[poses[s - 1][0] + unit * rs.randint(-2, 3), poses[s - 1][1] + unit * rs.randint(-2, 3),
                               poses[s][2] + rs.normal(0, 0.02)] for _ in range(16)])
            uni16 = rs.random_sample(16)
            est = np.tile(est16, (P // 16, 1))
            est[16:, 0] += unit * (np.arange(P - 16) % 5 - 2)            # the others: nearby poses of their own
            uni = np.tile(uni16, P // 16)
            psi = np.tile([np.cos(0.3), np.sin(0.3)], (P, 1))
            eng.match(lv, eng.to_device(est), 3, eng.to_device(ranges), 0.4, eng.to_device(psi), eng.to_device(uni), pf.m_coarse)
            eng.take_flags()
            m = eng.read_matches(pf.m_coarse)[:16].copy()
            out.append((m, lv.t["bounds"][:16].cpu().numpy().copy()))
        res.append(out)
        del pf
    for other in res[1:]:
        for (m0, b0), (m1, b1) in zip(res[0], other):
            for k in ("x", "y", "theta", "argmax", "pick"):
                assert np.array_equal(m0[k], m1[k]), k
            assert np.array_equal(b0.view(np.uint8), b1.view(np.uint8))


def test_frame_without_free_tile_at_bounded_level(pkg):
    """Every 16 x 16 tile of the frame has an occupied cell nearby: no analytically known minimum.  The level is bounded (and its
    check launch folded away), so the blur's last block measures the minimum and redoes the clamp, SLAM2D_F_FLOOR_REDO is raised,
    the bound kernel refreshes the whole frame's minima -- and the matches equal the oracle's."""
    unit, R, size_m, beams, wall = 0.1, 5.0, 16, 90, 0.5
    ogP = [size_m, size_m, {"x": 0.0, "y": 0.0}, unit, np.pi, R, beams, wall]
    smP = [1.0, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 1]
    ranges = np.full(beams, 2.0) + 0.3 * np.sin(np.arange(beams))
    est = np.array([[0.1, -0.2, 0.05], [0.3, 0.1, -0.1]])
    pf = pkg.ParticleFilter(2, ogP, smP, growable=False, rng=np.random.RandomState(0), bnb=True)
    lv, eng = pf.coarse, pf.engine
    _assert_check_launch_folded(lv)
    ogo = so.GridOracle(size_m, size_m, {"x": 0.0, "y": 0.0}, unit, np.pi, beams, R, wall)
    v, t = np.ones(ogo.visited.shape), np.full(ogo.visited.shape, 2.0)
    v[::6, ::6] += 4; t[::6, ::6] += 4                                   # an occupied cell every 6 cells
    ogo.visited[:], ogo.total[:] = v, t
    smo = so.MatcherOracle(ogo, *smP)
    want = []
    for p in range(2):                                                   # on the CPU first: the input has no all-free tile
        xr, yr, prob = smo.frameSearchSpace(est[p, 0], est[p, 1], unit, 2, 0.15)
        assert prob.min() > lv.floor_value
        fh, fw = prob.shape
        for ty in range(0, fh, 16):
            for tx in range(0, fw, 16):
                assert (prob[ty:ty + 16, tx:tx + 16] > lv.floor_value).any()
        want.append((prob, smo.searchToMatch(prob, est[p, 0], est[p, 1], est[p, 2], ranges, xr, yr, 1.0, 0.25, unit, 0.2,
                                             None, fineSearch=False, matchMax=True)))
    for m in eng.maps:
        m.upload(v, t)
    eng.match(lv, eng.to_device(est), 3, eng.to_device(ranges), 0.2, None, None, pf.m_coarse)
    flags = eng.take_flags()
    assert all(int(f) & F_FLOOR_REDO for f in flags)                     # the measured minimum was used
    got = eng.read_matches(pf.m_coarse)
    fr = lv.frames()
    gp = 4 * lv.tmax
    gmin = lv.t["gmin"].cpu().numpy().view(np.uint32)
    gmin2 = lv.t["gmin2"].cpu().numpy().view(np.uint32)
    gmin2b = lv.t["gmin2b"].cpu().numpy()
    for p in range(2):
        prob, (matched, cube, conf) = want[p]
        assert fr[p]["min_known"] == 0 and fr[p]["field_min"] == prob.min()
        assert int(got["argmax"][p]) == int(cube.argmax())
        assert (got["x"][p], got["y"][p], got["theta"][p]) == (matched["x"], matched["y"], matched["theta"])
        assert got["best_score"][p] == pytest.approx(cube.max(), rel=RTOL_CONF)
        np.testing.assert_allclose(got["confidence"][p], conf, rtol=RTOL_CONF)
        # the whole frame's minima, from the block minima the redo rewrote
        rows, cols = min(gp, (int(fr[p]["fh"]) >> 2) + 2), min(gp, (int(fr[p]["fw"]) >> 2) + 2)
        m = _min2x2(gmin[p])
        assert np.array_equal(gmin2[p][:rows, :cols], (m >> 12)[:rows, :cols])
        assert np.array_equal(gmin2b[p][:rows, :cols], (m >> 24).astype(np.uint8)[:rows, :cols])
