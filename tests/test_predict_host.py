"""The definition of slam2d_predict_scan pinned to the reference's semantics, without a GPU: on a fresh map a prediction returns,
beam by beam, exactly the wall one updateOccupancyGrid wrote (tests/predict_yardstick.py against oracle.slam_oracle.GridOracle)."""
import numpy as np
import pytest

import predict_yardstick as yard
from oracle import slam_oracle as so

UNIT, R, FOV, BEAMS, WALL = 0.1, 4.0, np.pi, 60, 0.5
PLANTED = {0: 0.05, 17: 6.0, 31: 4.0, 47: 3.99}            # a wall round the robot, no return, exactly max range, a wall cut by r_max


def scan_ranges(seed=11):
    rng = np.random.RandomState(seed).uniform(0.3, 3.9, BEAMS)
    for b, v in PLANTED.items():
        rng[b] = v
    return rng


def check_round_trip(walls, first, far, cells, r_min=0.0, r_max=R):
    """Every beam whose wall holds a cell with r_min < r < r_max predicts that part of it: nearest, farthest, how many; every
    other beam predicts nothing.  (The window's centre cell, r = 0, belongs to spoke 0 and is never a hit: r > r_min is strict.)"""
    seen = 0
    for b, radii in enumerate(walls):
        radii = radii[(radii > r_min) & (radii < r_max)]
        if radii.size:
            assert (first[b], far[b], cells[b]) == (radii.min(), radii.max(), radii.size), b
            seen += 1
        else:
            assert (first[b], far[b], cells[b]) == (np.inf, -np.inf, 0), b
    return seen


@pytest.mark.parametrize("theta", [0.0, 0.3, -2.9, 3.1, 7.0])
def test_a_map_predicts_back_the_walls_the_update_wrote(theta):
    og = so.GridOracle(20, 20, {"x": 0.0, "y": 0.0}, UNIT, FOV, BEAMS, R, WALL)
    reading = {"x": 0.3, "y": -0.7, "theta": theta, "range": scan_ranges()}
    walls = yard.beam_walls(og, reading)
    og.updateOccupancyGrid(reading)
    assert not og.growth_log
    first, far, cells = yard.predict(og, (reading["x"], reading["y"], theta))
    seen = check_round_trip(walls, first, far, cells)
    # (short ranges leave beams without wall cells: a spoke is narrower than a cell there.  From 2 m on it is a cell wide and
    # the 5-cell wall cannot miss it; about 28 of the 60 seeded ranges lie in (2.0, 3.7))
    assert seen >= 20
    assert cells[17] == 0 and np.isinf(first[17])             # the beam without return wrote no wall inside the window
    assert cells[31] > 0 and far[31] < R                      # range == max range: the part of its wall below r_max
    assert (cells <= [len(w) for w in walls]).all()


def test_windows_and_poses_that_see_nothing():
    og = so.GridOracle(20, 20, {"x": 0.0, "y": 0.0}, UNIT, FOV, BEAMS, R, WALL)
    reading = {"x": 0.3, "y": -0.7, "theta": 0.3, "range": scan_ranges()}
    walls = yard.beam_walls(og, reading)
    og.updateOccupancyGrid(reading)
    pose = (0.3, -0.7, 0.3)
    first, far, cells = yard.predict(og, pose, r_min=1.0, r_max=2.0)
    seen = check_round_trip(walls, first, far, cells, 1.0, 2.0)
    assert 0 < seen < BEAMS
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0, 0, np.nan), (1e12, 0, 0), (0, 0, 1e9), (100.0, 0, 0)):
        first, far, cells = yard.predict(og, bad)
        assert not cells.any() and np.isinf(first).all() and (far == -np.inf).all(), bad
