"""The oracle against the reference's own results: its scan-matching flow and its FastSLAM flow on the bundled Intel log,
recorded from a run of the reference by tests/golden/make_golden_reference_checks.py (tests/golden/vs_reference.npz).  The
other committed golden vectors (tests/test_oracle_golden.py) pin the oracle's parts one by one."""
import numpy as np

from conftest import load_golden
from codec import unpack_counts

REF_SM = (1.4, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 5)


def test_blur_is_scipy_bit_for_bit():
    from scipy.ndimage import gaussian_filter
    from oracle import slam_oracle as so
    rs = np.random.RandomState(0)
    for shape, sigma in [((249, 249), 0.4), ((300, 211), 2.0), ((64, 50), 1.3), ((40, 33), 3.7)]:
        a = np.where(rs.rand(*shape) < 0.05, 0.0, np.log(0.15))
        assert np.array_equal(gaussian_filter(a, sigma=sigma), so.blur_reflect(a, sigma))


def test_scanmatch_flow_equals_reference(intel_readings):
    from oracle import slam_oracle as so
    ref = load_golden("vs_reference.npz")
    n = 14
    r0 = intel_readings[0]
    og_o = so.GridOracle(10, 10, r0, 0.02, np.pi, 180, 10, 0.1)
    sm_o = so.MatcherOracle(og_o, *REF_SM)
    out, oc = so.run_scanmatch_flow(intel_readings, og_o, sm_o, max_scans=n)
    assert [(m["x"], m["y"], m["theta"]) for m in out] == [tuple(p) for p in ref["sm_poses"].tolist()]
    assert list(oc) == ref["sm_confs"].tolist()
    visited, total = unpack_counts(ref["sm_counts"])
    assert np.array_equal(visited, og_o.visited) and np.array_equal(total, og_o.total)
    assert np.array_equal(ref["sm_X"], og_o.X) and np.array_equal(ref["sm_Y"], og_o.Y)


def test_fastslam_flow_equals_reference(intel_readings):
    from oracle import slam_oracle as so
    ref = load_golden("vs_reference.npz")
    u, n_particles, n = 0.02, 3, 9
    ogP = [20, 20, intel_readings[0], u, np.pi, 10, 180, 5 * u]
    np.random.seed(3)
    po = so.ParticleFilterOracle(n_particles, ogP, list(REF_SM))
    wo = []
    for c, r in enumerate(intel_readings[:n], start=1):
        po.updateParticles(r, c)
        po.weightUnbalanced()
        wo.append([p.weight for p in po.particles])
        if c == 6:
            po.resample()
    assert np.array_equal(ref["fs_weights"], np.array(wo, dtype=float))
    for i, b in enumerate(po.particles):
        visited, _ = unpack_counts(ref[f"fs_counts_{i}"])
        assert np.array_equal(visited, b.og.visited) and ref[f"fs_xtraj_{i}"].tolist() == b.xTrajectory
