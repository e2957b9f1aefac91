"""Mapping from known poses: the reference's third use (Utils/OccupancyGrid.py:main, :185-199), which builds a map by
calling ``updateOccupancyGrid`` for every scan of a log at its recorded pose -- also how a SLAM result's map is compared
against one built from ground-truth poses."""
import numpy as np

from .grid import OccupancyGrid


def map_from_poses(readings, mapXLength=10, mapYLength=10, unitGridSize=0.02, lidarFOV=np.pi, lidarMaxRange=10,
                   wallThickness=None, device=None):
    """The grid of ``Utils/OccupancyGrid.py:main``: centred on the first reading's pose (:189-193), every reading applied in
    order (OccupancyGrid.update_many: one launch per chunk of scans, the reference's counts, limits and growth exactly).
    ``readings``: dicts with 'x', 'y', 'theta' and 'range' (numSamplesPerRev = len of the first one's ranges)."""
    readings = list(readings)
    if not readings:
        raise ValueError("map_from_poses needs at least one reading")
    if wallThickness is None:
        wallThickness = 7 * unitGridSize                                     # :186
    first = readings[0]
    og = OccupancyGrid(mapXLength, mapYLength, {"x": first["x"], "y": first["y"]}, unitGridSize, lidarFOV,
                       len(first["range"]), lidarMaxRange, wallThickness, device=device)
    og.update_many(readings)
    return og
