"""``ScanMatcher`` with the reference's class surface
(Utils/ScanMatcher_OGBased.py:8-176), running the field build and the pose-cube
sweep on the GPU for one particle.

``matchScan`` is synchronous like the reference's (the caller needs the pose
before its next statement).  The batched, all-particles path is
``filter.ParticleFilter``.
"""
import collections
import contextlib
import copy
import math

import numpy as np
import torch

from . import _lib
from .engine import MATCH_DOUBLES, _MATCH_DTYPE, Lattice, ParticleEngine, SearchLevel, encode_cost, likelihood_table, pinned_stream
from .points import reach as points_reach

_level_cache = {}


class _CallBuffers:
    """Host / device staging of one synchronous matchScan call, kept with the grid's one-particle engine: a pinned input
    buffer (one H2D copy per call) and ONE device buffer holding both levels' results and the fault bits (one D2H copy and one
    synchronisation per call; the engine's flag word and match buffers are views of it)."""

    def __init__(self, eng, beams):
        dev = eng.device
        self.h_in = torch.zeros(6 + beams, dtype=torch.float64).pin_memory()
        self.d_in = torch.zeros(6 + beams, dtype=torch.float64, device=dev)
        self.d_out = torch.zeros(2 * MATCH_DOUBLES + 1, dtype=torch.float64, device=dev)
        self.h_out = torch.zeros(2 * MATCH_DOUBLES + 1, dtype=torch.float64).pin_memory()
        self.m_coarse = self.d_out[:MATCH_DOUBLES].view(1, MATCH_DOUBLES)
        self.m_fine = self.d_out[MATCH_DOUBLES:2 * MATCH_DOUBLES].view(1, MATCH_DOUBLES)
        eng.match_buf["coarse"], eng.match_buf["fine"] = self.m_coarse, self.m_fine
        eng.flags = self.d_out[2 * MATCH_DOUBLES:].view(torch.int32)[:1]         # (take_flags and the kernels use this word from now on)

    def download(self, eng):
        """Both levels' results + the fault word in one copy; raises on a fatal bit like ParticleEngine.take_flags."""
        self.h_out.copy_(self.d_out, non_blocking=True)
        torch.cuda.current_stream(eng.device).synchronize()
        host = self.h_out.numpy()
        bits = int(host[2 * MATCH_DOUBLES:].view(np.uint32)[0])
        if bits:
            eng.flags.zero_()
            if bits & _lib.FATAL_FLAGS:
                raise _lib.Slam2dError(f"particle 0: {_lib.describe_flags(bits & _lib.FATAL_FLAGS)}")
        m = host[:2 * MATCH_DOUBLES].view(_MATCH_DTYPE)
        return m[0], m[1]


def _call_buffers(eng, beams):
    io = getattr(eng, "_call_io", None)
    if io is None:
        io = eng._call_io = _CallBuffers(eng, beams)
    return io


class _Exclusive:
    """A shared workspace may serve one call at a time: the drop-in methods are synchronous (nothing is live between
    calls), and this guard turns any overlap -- two threads, a re-entrant callback -- into an error instead of silent
    corruption of another matcher's results."""

    def __init__(self, *levels):
        self.levels = levels

    def __enter__(self):
        for lv in self.levels:
            if getattr(lv, "_busy", False):
                raise _lib.Slam2dError("a ScanMatcher call is already using this configuration's shared workspace "
                                       "(the drop-in classes are synchronous and not re-entrant)")
        for lv in self.levels:
            lv._busy = True

    def __exit__(self, *exc):
        for lv in self.levels:
            lv._busy = False
        return False


def _shared_level(og, key_extra, **kw):
    """Workspaces are shared by all matchers of one configuration on one device:
    calls are synchronous and sequential, so nothing is live between calls (_Exclusive enforces it)."""
    key = (str(og.device), id(og.lidar)) + key_extra
    if key not in _level_cache:
        _level_cache[key] = SearchLevel(og.lidar, 1, og.device, bnb=False, **kw)     # whole cubes: brute-force sweep
    return _level_cache[key]


# ---- what the localisation calls take: a scan, or a set of points ----
def ranges_of(reading_or_ranges, beams, N=None):
    """A reading dict or its ranges as a contiguous float64 array: ``[beams]``, or -- with ``N`` -- also ``[N, beams]``, a scan per
    pose; ValueError otherwise."""
    rng = reading_or_ranges["range"] if isinstance(reading_or_ranges, dict) else reading_or_ranges
    rng = np.ascontiguousarray(np.asarray(rng, dtype=np.float64))
    if N is None and rng.shape != (beams,):
        raise ValueError(f"ranges of shape {rng.shape}: want ({beams},)")
    if N is not None and rng.shape not in ((beams,), (N, beams)):
        raise ValueError(f"ranges of shape {rng.shape}: want ({beams},) or ({N}, {beams})")
    return rng


def points_of(points, N=None):
    """A point set as a contiguous float64 array: ``[M, 2]``, or -- with ``N`` -- also ``[N, M, 2]``, a set per pose, 1 <= M <=
    ``_lib.MAX_POINTS``; ValueError otherwise."""
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
    if N is None and (pts.ndim != 2 or pts.shape[1] != 2 or not 1 <= len(pts) <= _lib.MAX_POINTS):
        raise ValueError(f"points of shape {pts.shape}: want (M, 2), 1 <= M <= {_lib.MAX_POINTS}")
    if N is not None and (pts.ndim not in (2, 3) or pts.shape[-1] != 2 or not 1 <= pts.shape[-2] <= _lib.MAX_POINTS or (pts.ndim == 3 and len(pts) != N)):
        raise ValueError(f"points of shape {pts.shape}: want (M, 2) or ({N}, M, 2), 1 <= M <= {_lib.MAX_POINTS}")
    return pts


# ---- the covering level of ScanMatcher.scorePoses, planned on the host ----
def covering_window(poses, window=None):
    """(cx, cy, half) of the square that ``scorePoses`` frames its field on: ``window`` as given, else the bounding box of the
    finite poses (centre, larger half-edge); (0, 0, 0) when there is none."""
    if window is not None:
        cx, cy, half = (float(v) for v in window)
        if not (math.isfinite(cx) and math.isfinite(cy) and math.isfinite(half) and half >= 0):
            raise ValueError(f"window = (cx, cy, half) wants finite numbers and half >= 0, not {window!r}")
        return cx, cy, half
    xy = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    xy = xy[np.isfinite(xy).all(axis=1), :2]
    if not len(xy):
        return 0.0, 0.0, 0.0
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    return float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2), float(max(hi[0] - lo[0], hi[1] - lo[1]) / 2)


def round_up_125(v):
    """The smallest of ..., 0.5, 1, 2, 5, 10, 20, 50, ... that is >= v (v > 0): pose sets of similar extent share one level."""
    e = math.floor(math.log10(v))
    for k in (e - 1, e, e + 1):
        for m in (1, 2, 5):
            c = m * 10.0 ** k if k >= 0 else m / 10.0 ** -k
            if c >= v:
                return c
    raise AssertionError(v)


def field_build_limits(reach, step, unit):
    """None when slam2d_field_build accepts a level of this reach, else what it refuses (check_level and check_field_args in
    csrc/slam2d.hip, and the map-window row k_occ_scatter keeps in 64 KB of LDS)."""
    fmax = int(2 * reach / step) + 2
    fpitch = -(-fmax // 16) * 16
    tmax = -(-fmax // 16)
    wmax = int(2 * reach / unit) + 3
    if fmax * fpitch >= 1 << 29:
        return f"a field of {fmax} x {fpitch} cells (fmax * fpitch must stay below 2^29)"
    if tmax * tmax > 28000:
        return f"{tmax} x {tmax} field tiles (at most 28000)"
    if wmax * 4 > 65536:
        return f"a map window of {wmax} cells per row (at most 16384)"
    return None


def covering_radius(half, max_range, step, unit):
    """The ``search_radius_ctor`` of the covering level for a window of half-edge ``half``: the level's reach, 1.1 * max_range +
    this (Utils/ScanMatcher_OGBased.py:21), is at least half + max_range, so every endpoint of an in-range beam of a pose in the
    window lies in the field.  Rounded up (round_up_125) where slam2d_field_build still accepts the level, else to whole steps;
    ValueError naming ``window`` when even that is beyond the build's limits."""
    need = max(half + max_range - 1.1 * max_range, step)
    exact = math.ceil(need / step) * step
    for ctor in (round_up_125(need), exact):
        if field_build_limits(1.1 * max_range + ctor, step, unit) is None:
            return ctor
    raise ValueError(f"window: a half-edge of {half:g} m at a step of {step:g} m needs "
                     f"{field_build_limits(1.1 * max_range + exact, step, unit)}; score a smaller window or use the coarse level")


def distance_table_of(likelihood, step):
    """(table, cache key) of a covering level's ``likelihood``: (None, ()) for None, else ``engine.likelihood_table`` at ``step``
    for a dict of ``sigma`` and, optionally, ``z_hit``, ``z_rand``, ``max_dist``."""
    if likelihood is None:
        return None, ()
    if not isinstance(likelihood, dict):
        raise ValueError(f"likelihood is None or a dict of sigma, z_hit, z_rand, max_dist, not {likelihood!r}")
    unknown = set(likelihood) - {"sigma", "z_hit", "z_rand", "max_dist"}
    if unknown or "sigma" not in likelihood:
        raise ValueError(f"likelihood wants sigma and at most z_hit, z_rand, max_dist, not {sorted(likelihood)}")
    return likelihood_table(step, **likelihood), tuple(sorted((k, None if v is None else float(v)) for k, v in likelihood.items()))


def clearance_table_of(max_dist, step):
    """(table, cache key) of ``ScanMatcher.clearance``: the identity table -- entry i is i, the field is the clamped squared
    distance itself --, as long as the call takes, or floor((max_dist / step)^2) + 2 entries."""
    n = _lib.DISTANCE_MAX_TABLE
    if max_dist is not None:
        max_dist = float(max_dist)
        if not (math.isfinite(max_dist) and max_dist > 0):
            raise ValueError(f"max_dist wants a finite positive number, not {max_dist!r}")
        n = min(n, math.floor((max_dist / step) ** 2) + 2)
    return (np.arange(n, dtype=np.uint32), 1.0), ("clearance", n)


# ---- the rays of ScanMatcher.scoreRays ----
def ray_margin(wall_thickness, step):
    """The default ``margin`` of ``scoreRays`` in samples: ceil(wallThickness / step) + 1 -- the wall the map update itself paints
    in front of an endpoint, plus one cell of discretisation.  A true pose's beams end inside it and are not THROUGH."""
    return math.ceil(float(wall_thickness) / float(step)) + 1


_same_frames = set()


def same_frames(lv, lvd):
    """``scoreRays`` without a likelihood reads the field of ``lv`` and the squared distances of ``lvd``, both just built about
    one centre: their frames have to agree in xlo, ylo, fh, fw.  Checked on the first call of a pair of cached levels (one
    small download); Slam2dError if they differ."""
    if (id(lv), id(lvd)) in _same_frames:
        return
    a, b = lv.frames()[0], lvd.frames()[0]
    differ = [k for k in ("xlo", "ylo", "fh", "fw") if a[k] != b[k]]
    if differ:
        raise _lib.Slam2dError(f"scoreRays: the field's frame and the distance image's differ in {differ}")
    if lv in _level_cache.values() and lvd in _level_cache.values():              # (cached levels live as long as the process)
        _same_frames.add((id(lv), id(lvd)))


# ---- the lattice of ScanMatcher.searchPoses and the peaks of its image, on the host ----
Peak = collections.namedtuple("Peak", "x y theta score cost")


def window_lattice(window, step, headings):
    """The ``Lattice`` of ``searchPoses``: positions every ``step`` metres over the square ``window = (cx, cy, half)``, the centre
    among them, and ``headings`` headings from -pi in steps of 2 pi / headings."""
    cx, cy, half = covering_window(None, window)
    step, headings = float(step), int(headings)
    if not (math.isfinite(step) and step > 0):
        raise ValueError(f"step wants a positive number, not {step!r}")
    if not 1 <= headings <= 65536:
        raise ValueError(f"headings wants 1 .. 65536, not {headings!r}")
    n = int(math.floor(half / step + 1e-9))
    return Lattice(2 * n + 1, 2 * n + 1, headings, cx - n * step, step, cy - n * step, step, -math.pi, 2 * math.pi / headings)


def lattice_peaks(cost, heading, top, separation_cells):
    """The ``top`` lowest-cost positions of a ``[ny, nx]`` cost image, well separated: taken greedily from the lowest cost up, a
    position only if no position already taken lies within ``separation_cells`` of it in Chebyshev distance (0: only the
    position itself); equal costs in the order of the flat index iy * nx + ix.  Returns int64 ``[k, 3]`` rows (iy, ix,
    heading[iy, ix]), k <= top."""
    cost = np.asarray(cost)
    heading = np.asarray(heading)
    if cost.ndim != 2 or heading.shape != cost.shape:
        raise ValueError(f"cost {cost.shape} and heading {heading.shape}: want two [ny, nx] images")
    sep = int(separation_cells)
    if sep < 0:
        raise ValueError("separation_cells wants >= 0")
    ny, nx = cost.shape
    free = np.ones(cost.shape, dtype=bool)
    order = np.argsort(cost, axis=None, kind="stable")                          # (stable: equal costs keep the flat order)
    peaks = []
    for flat in order:
        if len(peaks) >= top:
            break
        iy, ix = divmod(int(flat), nx)
        if not free[iy, ix]:
            continue
        peaks.append((iy, ix, int(heading[iy, ix])))
        free[max(0, iy - sep):iy + sep + 1, max(0, ix - sep):ix + sep + 1] = False
    return np.array(peaks, dtype=np.int64).reshape(-1, 3)


# ---- the stages of ScanMatcher.refinePoses and Tracker ----
def default_stages(step):
    """The stages ((rx, ry, rt), (dx, dy, dth)) of a refinement at a level of this step: four cells and 0.08 rad either way at one
    cell and 0.02 rad, then two half cells and 0.01 rad at half a cell and 0.005 rad."""
    step = float(step)
    return (((4, 4, 4), (step, step, 0.02)), ((2, 2, 2), (step / 2, step / 2, 0.005)))


def check_stages(stages, step):
    """``stages`` (None: ``default_stages(step)``) as a tuple of ((rx, ry, rt), (dx, dy, dth)) of ints >= 0 and finite floats,
    each with at most 2^20 candidates; ValueError otherwise."""
    out = []
    for st in default_stages(step) if stages is None else stages:
        try:
            (rx, ry, rt), (dx, dy, dth) = st
            radii, steps = (int(rx), int(ry), int(rt)), (float(dx), float(dy), float(dth))
        except (TypeError, ValueError):
            raise ValueError(f"a stage is ((rx, ry, rt), (dx, dy, dth)), not {st!r}") from None
        if min(radii) < 0 or radii != (rx, ry, rt) or not all(math.isfinite(v) for v in steps):
            raise ValueError(f"a stage wants whole radii >= 0 and finite steps, not {st!r}")
        if (2 * radii[0] + 1) * (2 * radii[1] + 1) * (2 * radii[2] + 1) > _lib.REFINE_MAX_CANDIDATES:
            raise ValueError(f"a stage of more than {_lib.REFINE_MAX_CANDIDATES} candidates: {st!r}")
        out.append((radii, steps))
    if not out:
        raise ValueError("no stages")
    return tuple(out)


def refine_ray_options(rays, beams, step, wall_thickness, outside_cost):
    """``refinePoses``' ``rays`` with its defaults filled in: ``stride``, ``margin`` and ``through_cost`` as ``localise.ray_options``
    fills and checks them, and ``phase`` (0) -- which beams are cast, b % stride == phase -- in place of ``rotate``.  ValueError for
    an unknown key (``rotate`` among them), a phase outside 0 .. stride - 1 and whatever ``ray_options`` refuses."""
    from .localise import ray_options                          # (localise imports this module)
    opt = dict(rays)
    if "rotate" in opt:
        raise ValueError("rays: unknown keys ['rotate'] (a refinement takes a phase)")
    phase = opt.pop("phase", 0)
    full = ray_options(opt, beams, step, wall_thickness, outside_cost)
    if int(phase) != phase or not 0 <= int(phase) < full["stride"]:
        raise ValueError(f"rays: phase wants 0 .. {full['stride'] - 1} (below the stride), not {phase!r}")
    return dict(stride=full["stride"], phase=int(phase), margin=full["margin"], through_cost=full["through_cost"])


class ScanMatcher:
    def __init__(self, og, searchRadius, searchHalfRad, scanSigmaInNumGrid, moveRSigma, maxMoveDeviation, turnSigma,
                 missMatchProbAtCoarse, coarseFactor):
        self.searchRadius = searchRadius
        self.searchHalfRad = searchHalfRad
        self.og = og
        self.scanSigmaInNumGrid = scanSigmaInNumGrid
        self.coarseFactor = coarseFactor
        self.moveRSigma = moveRSigma
        self.turnSigma = turnSigma
        self.missMatchProbAtCoarse = missMatchProbAtCoarse
        self.maxMoveDeviation = maxMoveDeviation

    # ---- level plans ----
    def _level(self, step, sigma, miss, radius, half, fine):
        key = (step, sigma, miss, self.searchRadius, radius, half, bool(fine), self.moveRSigma, self.maxMoveDeviation,
               self.turnSigma)
        return _shared_level(self.og, key, step=step, sigma=sigma, miss_prob=miss,
                             search_radius_ctor=self.searchRadius, radius=radius, half_rad=half, fine=fine,
                             move_sigma=self.moveRSigma, max_move_dev=self.maxMoveDeviation,
                             turn_sigma=self.turnSigma)

    def coarse_level(self):
        step = self.coarseFactor * self.og.unitGridSize                        # :54
        sigma = self.scanSigmaInNumGrid / self.coarseFactor                    # :55
        return self._level(step, sigma, self.missMatchProbAtCoarse, self.searchRadius, self.searchHalfRad, False)

    def fine_level(self):
        step = self.og.unitGridSize                                            # :66
        miss = self.missMatchProbAtCoarse ** (2 / self.coarseFactor)           # :69
        cstep = self.coarseFactor * self.og.unitGridSize
        return self._level(step, self.scanSigmaInNumGrid, miss, cstep, self.searchHalfRad, True)

    # ---- the two halves, on the device ----
    def _build_field(self, eng, level, d_centre, stride, cx, cy):
        """checkAndExapndOG on the host (growth is a re-allocation), then the kernels."""
        self.og.checkAndExapndOG([cx - level.reach, cx + level.reach], [cy - level.reach, cy + level.reach])   # :27
        eng = self.og.engine()
        eng.field_build(level, d_centre, stride)
        return eng

    def frameSearchSpace(self, estimatedX, estimatedY, unitLength, sigma, missMatchProbAtCoarse):
        """(:20-39)  Returns xRangeList, yRangeList, probSP (host float64 array decoded from
        the device's fixed-point field: values exact to 2^-32 relative to probMin)."""
        level = self._level(unitLength, sigma, missMatchProbAtCoarse, self.searchRadius, self.searchHalfRad, False)
        with _Exclusive(level):
            eng = self.og.engine()
            d_c = eng.to_device([[estimatedX, estimatedY]])
            eng = self._build_field(eng, level, d_c, 2, estimatedX, estimatedY)
            self.last_flags = int(eng.take_flags()[0])
            fr = level.frames()[0]
            return [fr["xlo"], fr["xhi"]], [fr["ylo"], fr["yhi"]], level.field(0)

    def matchScan(self, reading, estMovingDist, estMovingTheta, count, matchMax=True):
        """(:47-79)  Coarse then fine; returns (matchedReading, coarse confidence)."""
        rMeasure = np.asarray(reading['range'])
        if count == 1:
            return reading, 1                                                  # :51-52
        ex, ey, eth = reading['x'], reading['y'], reading['theta']
        coarse, fine = self.coarse_level(), self.fine_level()
        with _Exclusive(coarse, fine), pinned_stream():
            og = self.og
            og.checkAndExapndOG([ex - coarse.reach, ex + coarse.reach], [ey - coarse.reach, ey + coarse.reach])   # :27 (coarse window)
            eng = og.engine()
            io = _call_buffers(eng, og.numSamplesPerRev)
            # everything the call uploads in ONE pinned buffer and one copy: [x, y, theta | cos, sin of the heading | uniform | ranges]
            h = io.h_in.numpy()
            h[0:3] = (ex, ey, eth)
            h[3:5] = eng.psi_table([estMovingTheta])[0]
            if not matchMax:                        # one draw from the legacy global stream, like np.random.choice (:138)
                h[5] = np.random.random_sample()
            h[6:] = rMeasure
            io.d_in.copy_(io.h_in, non_blocking=True)
            d_est, d_psi, d_u, d_rng = io.d_in[0:3], io.d_in[3:5], None if matchMax else io.d_in[5:6], io.d_in[6:]
            m_coarse, m_fine = io.m_coarse, io.m_fine
            # The fine window is centred on the coarse result, at most (ncell + 1) coarse cells from the estimate: when the coarse
            # window widened by that much lies inside the map, the fine window cannot need growth (:27 at the fine level) and the
            # call needs no host round trip between the levels -- one synchronisation per matchScan instead of two (round 3:
            # 0.86 ms per call).  Only the tiles the sweep reads are blurred (slam2d_match): this method hands no field out.
            margin = (coarse.ncell + 1) * coarse.step
            m = og.map
            settled = not (ex - coarse.reach - margin < m.lim_x[0] or ex + coarse.reach + margin > m.lim_x[1] or
                           ey - coarse.reach - margin < m.lim_y[0] or ey + coarse.reach + margin > m.lim_y[1])
            eng.match(coarse, d_est, 3, d_rng, estMovingDist, d_psi, d_u, m_coarse)
            if not settled:
                c = io.download(eng)[0]
                og.checkAndExapndOG([float(c["x"]) - fine.reach, float(c["x"]) + fine.reach],
                                    [float(c["y"]) - fine.reach, float(c["y"]) + fine.reach])
                eng = og.engine()
            eng.match(fine, m_coarse, MATCH_DOUBLES, d_rng, estMovingDist, None, None, m_fine)
            c, f = io.download(eng)
            og._update_pending = False                                            # (the download has looked at the last update's fault bits too)
            matched = {"x": float(f["x"]), "y": float(f["y"]), "theta": float(f["theta"]), "range": rMeasure}
            self.last = dict(coarse=c.copy(), fine=f.copy())
            # the matched pose and the scan's ranges are still on the device: an updateOccupancyGrid(matched) that follows on this
            # grid (Algorithm/FastSlam.py:129-133) launches from them -- no second upload (grid.updateOccupancyGrid)
            og._last_match = dict(ref=matched, pose=(matched["x"], matched["y"], matched["theta"]), rng=rMeasure, d_pose=m_fine, d_rng=d_rng, eng=eng)
            return matched, np.float64(c["confidence"])                            # :79

    def matchMoments(self, level="fine"):
        """Pose mean and covariance of the last ``matchScan`` (count > 1) of this matcher at one of its two levels, over the
        whole pose cube (include/slam2d.h, slam2d_match_moments): ``dict(pose_mean=(x, y, theta), cov=3x3 in (m, m, rad),
        sum_w, log_confidence)`` with log_confidence = best score + log(sum_w).  Runs on the state that match left on the
        device.  The workspaces are shared by all matchers of one configuration (_shared_level): raises ``Slam2dError`` when
        the level has been used by another match since -- never another grid's moments."""
        if level not in ("fine", "coarse"):
            raise ValueError("level is 'fine' or 'coarse'")
        last = getattr(self, "last", None)
        if not last or level not in last:
            raise _lib.Slam2dError("matchMoments needs a matchScan (count > 1) of this matcher first")
        lv = self.fine_level() if level == "fine" else self.coarse_level()
        with _Exclusive(lv), pinned_stream():
            eng = self.og._engine
            io = getattr(eng, "_call_io", None) if eng is not None else None
            if io is None or not eng.built_last(lv):
                raise _lib.Slam2dError(f"the {level} level's shared workspace has been used by another match since this matcher's "
                                       "last matchScan: match again first")
            d_match = io.m_fine if level == "fine" else io.m_coarse
            d_est, stride = (io.m_coarse, MATCH_DOUBLES) if level == "fine" else (io.d_in[0:3], 3)
            rows = eng.match_moments(lv, d_est, stride, d_match)
            # one download: the rows, and the records they were computed from (another matcher of this grid and configuration
            # may have matched since: the records then are not this matcher's)
            host = torch.cat([rows.reshape(-1), io.d_out[:2 * MATCH_DOUBLES]]).cpu().numpy()
            m = host[_lib.MOMENTS_STRIDE:].view(_MATCH_DTYPE)
            for name, rec in (("coarse", m[0]), ("fine", m[1])):
                if name in last and rec.tobytes() != last[name].tobytes():
                    raise _lib.Slam2dError("another matcher of this grid has matched since this matcher's last matchScan: "
                                           "match again first")
            mom = lv.moments_host(host[:_lib.MOMENTS_STRIDE])
            est = (float(m[0]["x"]), float(m[0]["y"]), float(m[0]["theta"])) if level == "fine" else tuple(float(v) for v in io.h_in.numpy()[0:3])
            mean = mom["mean"][0]
            sum_w = float(mom["sum_w"][0])
            return dict(pose_mean=(est[0] + mean[0], est[1] + mean[1], est[2] + mean[2]), cov=mom["cov"][0], sum_w=sum_w,
                        log_confidence=float(mom["best_score"][0]) + math.log(sum_w) if sum_w > 0 else float("nan"))

    def covering_level(self, level, half, shared=True, likelihood=None):
        """The cached level whose field covers a window of half-edge ``half`` at this matcher's fine or coarse configuration
        (step, sigma and miss probability exactly as fine_level() / coarse_level() derive them), with a cube of one angle.
        ``shared=False``: a level of the caller's own, for a field that has to outlive the call (Localiser).
        ``likelihood``: None -- the blurred field -- or a dict of ``sigma`` (metres) and, optionally, ``z_hit``, ``z_rand``,
        ``max_dist``: the level carries ``engine.likelihood_table`` at its step (``lv.distance_table``) and is to be filled by
        ``ParticleEngine.field_build_distance`` (``build_cover`` does); its ``cost_scale`` becomes the table's, so a shared
        one is cached under a key of its own and never handed to a caller that expects the blurred field."""
        return self._covering_level(level, half, shared, lambda step: distance_table_of(likelihood, step))

    def _covering_level(self, level, half, shared, table_of):
        """``covering_level`` with the distance table, if any, as ``table_of(step)`` = (table, cache key)."""
        if level not in ("fine", "coarse"):
            raise ValueError("level is 'fine' or 'coarse'")
        unit = self.og.unitGridSize
        if level == "fine":
            step, sigma, miss = unit, self.scanSigmaInNumGrid, self.missMatchProbAtCoarse ** (2 / self.coarseFactor)      # :66,69
        else:
            step, sigma, miss = self.coarseFactor * unit, self.scanSigmaInNumGrid / self.coarseFactor, self.missMatchProbAtCoarse   # :54-55
        ctor = covering_radius(half, self.og.lidarMaxRange, step, unit)
        kw = dict(step=step, sigma=sigma, miss_prob=miss, search_radius_ctor=ctor, radius=step, half_rad=0.0, fine=True,
                  move_sigma=self.moveRSigma, max_move_dev=self.maxMoveDeviation, turn_sigma=self.turnSigma)
        table, table_key = table_of(step)
        if not shared:
            lv = SearchLevel(self.og.lidar, 1, self.og.device, bnb=False, **kw)
        else:
            key = ("cover", step, sigma, miss, ctor, self.moveRSigma, self.maxMoveDeviation, self.turnSigma)
            lv = _shared_level(self.og, key if table is None else key + ("distance",) + table_key, **kw)
        if table is not None:
            lv.distance_table = table
        return lv

    @staticmethod
    def build_cover(eng, lv, cx, cy, dist2=False):
        """The covering level's field around (cx, cy): the blurred build, or -- a level with a ``distance_table`` -- the
        distance build."""
        table = getattr(lv, "distance_table", None)
        if table is None:
            return eng.field_build(lv, eng.to_device([[cx, cy]]), 2)
        return eng.field_build_distance(lv, eng.to_device([[cx, cy]]), 2, table, dist2=dist2)

    @staticmethod
    def outside_cost_of(lv):
        """What a beam that leaves the covering field pays by default: free space as the blurred field encodes it, or the
        table's last entry -- such a beam is a random measurement."""
        table = getattr(lv, "distance_table", None)
        return int(encode_cost(lv.floor_value, lv.cost_scale)) if table is None else int(table[0][-1])

    @contextlib.contextmanager
    def _cover(self, lv, cx, cy, dist2=False):
        """The prologue of every call on a covering level, with the level to itself and the stream pinned: the map grown to hold
        the level's frame around (cx, cy), the grid's engine, the field built there.  Yields (engine, what ``build_cover``
        returned)."""
        with _Exclusive(lv), pinned_stream():
            self.og.checkAndExapndOG([cx - lv.reach, cx + lv.reach], [cy - lv.reach, cy + lv.reach])      # :27
            eng = self.og.engine()
            yield eng, self.build_cover(eng, lv, cx, cy, dist2=dist2)

    def _download(self, eng, name, *tensors):
        """The epilogue of the public call ``name``: its float64 or int64 result ``tensors`` and the build's fault word in ONE
        download -- as the 64-bit words they are, so rows and images arrive bit for bit --, the word cleared on the device if
        any bit is set, ``Slam2dError`` on a fatal one, else ``last_flags``.  Returns the tensors as host arrays."""
        words = [t.reshape(-1) if t.dtype == torch.int64 else t.reshape(-1).view(torch.int64) for t in tensors]
        host = torch.cat(words + [eng.flags[:1].to(torch.int64)]).cpu().numpy()
        bits = int(host[-1]) & 0xffffffff
        if bits:
            eng.flags.zero_()
            if bits & _lib.FATAL_FLAGS:
                raise _lib.Slam2dError(f"{name}: {_lib.describe_flags(bits & _lib.FATAL_FLAGS)}")
        self.last_flags = bits
        ends = np.cumsum([t.numel() for t in tensors])
        return [host[e - t.numel():e].view(np.float64 if t.dtype == torch.float64 else np.int64).reshape(tuple(t.shape)) for t, e in zip(tensors, ends)]

    def clearance(self, window, level="fine", max_dist=None):
        """How far every cell of the covering frame of ``window = (cx, cy, half)`` is from a wall: ``dict(dist, xs, ys)`` with
        ``dist`` [fh, fw] in metres -- sqrt(k) * step, k the squared distance in cells to the nearest occupied field cell of
        the frame (include/slam2d.h, slam2d_field_build_distance) --, ``xs`` [fw] and ``ys`` [fh] the cells' centres.  Distances
        are exact up to ``max_dist`` metres (default and at most: 255 cells); ``inf`` beyond, and everywhere in a frame
        without a wall.  Cells outside the frame are unknown, not walls."""
        cx, cy, half = covering_window(None, window)
        lv = self._covering_level(level, half, True, lambda step: clearance_table_of(max_dist, step))
        with self._cover(lv, cx, cy, dist2=True) as (eng, d2):
            bits = int(eng.take_flags()[0])
            self.last_flags = bits
            fr = lv.frames()[0]
            k = d2[0, :fr["fh"], :fr["fw"]].cpu().numpy().astype(np.int64)
        dist = np.sqrt(k.astype(np.float64)) * lv.step
        dist[k >= len(lv.distance_table[0]) - 1] = np.inf
        self.last_cover = dict(level=lv, window=(cx, cy, half))
        return dict(dist=dist, xs=float(fr["xlo"]) + (np.arange(int(fr["fw"])) + 0.5) * lv.step,
                    ys=float(fr["ylo"]) + (np.arange(int(fr["fh"])) + 0.5) * lv.step)

    def scorePoses(self, poses, reading_or_ranges, level="fine", window=None, likelihood=None):
        """How well a scan fits at N free poses anywhere in the map (include/slam2d.h, slam2d_score_poses): the reference's score
        of the scan -- convTotal of a fine search at zero offset, no prior (:129-130) -- at each pose ``poses[n] = (x, y,
        theta)``, in ONE launch.  ``reading_or_ranges``: a reading dict, ``[beams]`` ranges for every pose, or ``[N, beams]``, a
        scan per pose.  The field is this matcher's ``level`` ('fine' or 'coarse') built in full on a frame that covers the
        bounding box of the finite poses -- or ``window = (cx, cy, half)`` -- plus lidarMaxRange; the map grows to hold that
        frame as in frameSearchSpace (:27).  Returns a dict of [N] host arrays: ``score``, ``cells``, ``beam_score``,
        ``inside``, ``in_range``, ``outside`` (ParticleEngine.score_host); ``self.last_cover`` keeps the level and its frame.
        ``likelihood``: score against the likelihood field of ``covering_level`` instead of the blurred one.
        ValueError naming ``window`` when the frame is beyond what the field build accepts."""
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        N, B = len(poses), self.og.numSamplesPerRev
        if N == 0:
            raise ValueError("no poses")
        rng = ranges_of(reading_or_ranges, B, N)
        cx, cy, half = covering_window(poses, window)
        lv = self.covering_level(level, half, likelihood=likelihood)
        with self._cover(lv, cx, cy) as (eng, _):
            rows = eng.score_poses(lv, 0, eng.to_device(poses), 3, N, eng.to_device(rng), 0 if rng.ndim == 1 else B)
            host, = self._download(eng, "scorePoses", rows)
            self.last_cover = dict(level=lv, window=(cx, cy, half))
            return eng.score_host(host)

    def _distance_twin(self, level, half):
        """The cached distance level that stands on the frames of the blurred covering level of ``half``: ``clearance``'s."""
        return self._covering_level(level, half, True, lambda step: clearance_table_of(None, step))

    def castScans(self, poses, level="fine", window=None, max_range=None):
        """The scan the map expects at N free poses (include/slam2d.h, slam2d_cast_rays): per pose ``poses[n] = (x, y, theta)``
        and beam, a geometric ray through the occupied cells of the covering field of ``scorePoses`` (the same frame planning:
        the bounding box of the finite poses, or ``window``), sampled every field step up to ``max_range`` metres (default:
        lidarMaxRange), in ONE launch.  Returns the [N, beams] host arrays of ``ParticleEngine.cast_host``: ``kind``
        (``_lib.RAY_HIT``, ``RAY_LEFT`` the field, ``RAY_NONE`` within the range), ``k`` and ``range`` = k * step, ``inf``
        without a wall.  Unlike ``OccupancyGrid.predictScan`` the ray runs at the field's resolution with the beam's own
        heading, for any number of poses in one map.  ``self.last_cover`` keeps the distance level and its window."""
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        N = len(poses)
        if N == 0:
            raise ValueError("no poses")
        max_range = float(self.og.lidarMaxRange if max_range is None else max_range)
        if not (math.isfinite(max_range) and max_range >= 0):
            raise ValueError(f"max_range wants a finite number >= 0, not {max_range!r}")
        cx, cy, half = covering_window(poses, window)
        lvd = self._distance_twin(level, half)
        K = math.ceil(max_range / lvd.step)
        if K >= _lib.RAY_MAX_K:
            raise ValueError(f"max_range: {K} samples of {lvd.step:g} m (fewer than {_lib.RAY_MAX_K})")
        with self._cover(lvd, cx, cy, dist2=True) as (eng, d2):
            words = eng.cast_rays(lvd, 0, d2, eng.to_device(poses), 3, N, K)
            host, = self._download(eng, "castScans", words.to(torch.int64))
            self.last_cover = dict(level=lvd, window=(cx, cy, half))
            return eng.cast_host(host.astype(np.uint32), lvd.step)

    def scoreRays(self, poses, reading_or_ranges, level="fine", window=None, likelihood=None, margin=None, through_cost=None,
                  outside_cost=None):
        """``searchPoses``' cost of a scan at N free poses plus a charge for every beam that crosses a wall of the map on its
        way (include/slam2d.h, slam2d_score_rays), in ONE launch: the endpoint cost cannot tell a pose from one on the wrong side
        of a wall, this can.  ``poses``, ``reading_or_ranges``, ``level``, ``window`` and ``likelihood`` as in ``scorePoses``;
        ``outside_cost`` as in ``searchPoses``.  A beam is THROUGH when its ray meets an occupied field cell more than ``margin``
        samples (field steps) short of its measured range -- default ``ray_margin``: ceil(wallThickness / step) + 1, the wall
        the map update itself paints in front of an endpoint plus one cell of discretisation -- and pays ``through_cost``
        (default: ``outside_cost`` -- what a beam that leaves the map pays).  With ``likelihood`` one distance build gives the
        field and the squared distances the rays skip by; without, the blurred covering level gives the field and
        ``clearance``'s cached distance level of the same window the distances.  Returns the [N] host arrays of
        ``ParticleEngine.rays_host``: ``cost``, ``score``, ``beam_score``, ``inside``, ``in_range``, ``outside``, ``through``,
        ``checked``, ``depth``.  ``self.last_cover`` keeps the field's level, its window, ``margin`` and the two costs."""
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        N, B = len(poses), self.og.numSamplesPerRev
        if N == 0:
            raise ValueError("no poses")
        rng = ranges_of(reading_or_ranges, B, N)
        cx, cy, half = covering_window(poses, window)
        lv = self.covering_level(level, half, likelihood=likelihood)
        margin = ray_margin(self.og.wallThickness, lv.step) if margin is None else int(margin)
        if margin < 0:
            raise ValueError(f"margin wants a count of samples >= 0, not {margin}")
        lvd = lv if likelihood is not None else self._distance_twin(level, half)
        with self._cover(lvd, cx, cy, dist2=True) as (eng, d2), _Exclusive(*(() if lvd is lv else (lv,))):
            if lvd is not lv:
                self.build_cover(eng, lv, cx, cy)
                same_frames(lv, lvd)
            outside_cost = self.outside_cost_of(lv) if outside_cost is None else int(outside_cost)
            through_cost = outside_cost if through_cost is None else int(through_cost)
            rows = eng.score_rays(lv, 0, d2, eng.to_device(poses), 3, N, eng.to_device(rng), 0 if rng.ndim == 1 else B, margin,
                                  outside_cost, through_cost)
            host, = self._download(eng, "scoreRays", rows)
            self.last_cover = dict(level=lv, window=(cx, cy, half), margin=margin, outside_cost=outside_cost, through_cost=through_cost)
            return eng.rays_host(host, lv.cost_scale)

    def searchPoses(self, reading_or_ranges, window, step=None, headings=120, level="fine", top=5, separation=None, outside_cost=None,
                    likelihood=None):
        """Where in ``window = (cx, cy, half)`` could this scan have been taken (include/slam2d.h, slam2d_search_lattice): the
        best heading and its cost at every position of a lattice -- ``step`` metres apart (default: the level's step),
        ``headings`` headings over the full turn -- searched on the device: nothing but the scan is uploaded, one 8-byte word
        per POSITION comes back.  The field is the covering level of ``scorePoses`` for this window, built in full.  The cost
        of a pose is ``beam_score`` of ``scorePoses`` in the field's integers plus ``outside_cost`` for every in-range beam
        that ends outside the field (default: the level's free-space value as the field encodes it; with ``likelihood`` -- the
        likelihood field of ``covering_level`` instead of the blurred one -- the table's last entry).  Returns the arrays of
        ``ParticleEngine.search_host`` -- ``cost``, ``heading``, ``score`` [ny, nx], ``xs``, ``ys``, ``thetas`` -- and
        ``peaks``: up to ``top`` ``Peak(x, y, theta, score, cost)``, lowest cost first, no two within ``separation`` metres
        (default: ten lattice steps) of each other on either axis (``lattice_peaks``).  ``self.last_cover`` keeps the level,
        its window and the ``Lattice``."""
        rng = ranges_of(reading_or_ranges, self.og.numSamplesPerRev)
        window = covering_window(None, window)
        lv = self.covering_level(level, window[2], likelihood=likelihood)
        return self._search("searchPoses", lv, window, step, headings, top, separation, outside_cost,
                            lambda eng, lat, cost: eng.search_lattice(lv, 0, lat, eng.to_device(rng), cost))

    def _search(self, name, lv, window, step, headings, top, separation, outside_cost, launch):
        """The body of ``searchPoses`` and ``searchPoints`` in the covering level ``lv`` of ``window``: the lattice, the field, the
        search ``launch(eng, lattice, outside_cost)``, one download, the decoded image and its peaks."""
        cx, cy, half = window
        lat = window_lattice(window, lv.step if step is None else step, headings)
        sep = 10 if separation is None else int(round(float(separation) / lat.dx))
        if outside_cost is None:
            outside_cost = self.outside_cost_of(lv)
        with self._cover(lv, cx, cy) as (eng, _):
            host, = self._download(eng, name, launch(eng, lat, outside_cost))
            self.last_cover = dict(level=lv, window=(cx, cy, half), lattice=lat)
            res = eng.search_host(host, lat, lv.cost_scale)
        res["peaks"] = [Peak(float(res["xs"][ix]), float(res["ys"][iy]), float(res["thetas"][it]), float(res["score"][iy, ix]),
                             int(res["cost"][iy, ix])) for iy, ix, it in lattice_peaks(res["cost"], res["heading"], top, sep)]
        return res

    def refinePoses(self, poses, reading_or_ranges, stages=None, level="fine", window=None, likelihood=None, outside_cost=None, rays=None):
        """The best pose near each of N free seed poses (include/slam2d.h, slam2d_refine_poses): a local correlative search about
        every ``poses[n] = (x, y, theta)`` in the covering level of ``scorePoses`` and ``searchPoses`` -- the same frame planning
        (the bounding box of the finite seeds, or ``window``), the same ``likelihood`` and the same ``outside_cost`` default --,
        with the cost of ``searchPoses``.  ``stages``: a sequence of ((rx, ry, rt), (dx, dy, dth)) -- radii in steps, steps in
        metres and radians --, run in turn on the device, each from the poses the one before it left (None:
        ``default_stages`` of the level's step).  ``reading_or_ranges``: a reading dict, ``[beams]`` ranges for every seed, or
        ``[N, beams]``, a scan per seed.  One download.  Returns a dict of host arrays: ``poses`` [N, 3], ``cost`` (uint64, of
        the last stage's winner), ``score`` = -cost / cost_scale, ``start_cost`` (the seed's own) and ``offsets`` [N, stages, 3]
        (each stage's signed steps in x, y, theta); ``self.last_cover`` keeps the level and its window.
        ``rays``: None -- the endpoint cost alone, the path above bit for bit -- or a dict of ``stride``, ``phase`` (0), ``margin``
        and ``through_cost`` (``refine_ray_options``: the defaults of ``Localiser``'s ``rays``): every candidate of every stage
        pays ``through_cost`` for each cast beam -- b % stride == phase -- whose measured range lies more than ``margin`` samples
        beyond a wall of the map (slam2d_refine_poses_rays), so a lattice that straddles a wall does not step to its wrong side
        for nothing.  The squared distances come as in ``scoreRays``; the result gains ``through`` [N, stages], the through beams
        of each stage's winner, and ``last_cover`` the filled-in ``rays``."""
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        N, B = len(poses), self.og.numSamplesPerRev
        if N == 0:
            raise ValueError("no poses")
        rng = ranges_of(reading_or_ranges, B, N)
        window = covering_window(poses, window)
        lv = self.covering_level(level, window[2], likelihood=likelihood)
        rs = 0 if rng.ndim == 1 else B
        if rays is None:
            return self._refine("refinePoses", lv, window, poses, rng, stages, outside_cost,
                                lambda eng, a, b, d_rng, radii, steps, cost, words:
                                eng.refine_poses(lv, 0, a, b, N, 3, d_rng, rs, radii, steps, cost, d_words=words))
        if outside_cost is None:
            outside_cost = self.outside_cost_of(lv)
        opt = refine_ray_options(rays, B, lv.step, self.og.wallThickness, outside_cost)
        charge = (opt["stride"], opt["phase"], opt["margin"], opt["through_cost"])
        lvd = lv if likelihood is not None else self._distance_twin(level, window[2])
        return self._refine("refinePoses", lv, window, poses, rng, stages, outside_cost,
                            lambda eng, a, b, d_rng, radii, steps, cost, words, d2, through:
                            eng.refine_poses_rays(lv, 0, d2, a, b, N, 3, d_rng, rs, radii, steps, cost, *charge, d_words=words, d_through=through),
                            rays=opt, lvd=lvd)

    def _refine(self, name, lv, window, poses, source, stages, outside_cost, launch, rays=None, lvd=None):
        """The body of ``refinePoses`` and ``refinePoints`` in the covering level ``lv`` of ``window``: the field, the stages in
        turn -- ``launch(eng, d_in, d_out, d_source, radii, steps, outside_cost, d_words)``, ``source`` the scans or the point sets
        --, one download, the decoded words.  With ``rays`` (the filled-in options) the squared distances of ``lvd`` -- ``lv``
        itself, or the distance twin on the same frame, as in ``scoreRays`` -- and a stage's [N] through counts are ``launch``'s
        last two arguments, and the counts travel in the one download."""
        cx, cy, half = window
        N = len(poses)
        stages = check_stages(stages, lv.step)
        if outside_cost is None:
            outside_cost = self.outside_cost_of(lv)
        twin = rays is not None and lvd is not lv
        with self._cover(lvd if twin else lv, cx, cy, dist2=rays is not None) as (eng, d2), _Exclusive(*((lv,) if twin else ())):
            if twin:
                self.build_cover(eng, lv, cx, cy)
                same_frames(lv, lvd)
            d_pose = [eng.to_device(poses), torch.empty((N, 3), dtype=torch.float64, device=eng.device)]
            d_source = eng.to_device(source)
            words = torch.empty((len(stages), N, _lib.REFINE_STRIDE), dtype=torch.int64, device=eng.device)
            through = None if rays is None else torch.empty((len(stages), N), dtype=torch.int32, device=eng.device)
            for i, (radii, steps) in enumerate(stages):
                more = () if rays is None else (d2, through[i])
                launch(eng, d_pose[i & 1], d_pose[1 - (i & 1)], d_source, radii, steps, outside_cost, words[i], *more)
            # one download: the poses, the stages' words, the through counts and the build's fault word
            more = () if rays is None else (through.to(torch.int64),)
            best, w, *thr = self._download(eng, name, d_pose[len(stages) & 1], words, *more)
            self.last_cover = dict(level=lv, window=(cx, cy, half), stages=stages)
            if rays is not None:
                self.last_cover.update(rays=rays, outside_cost=outside_cost)
        dec = [ParticleEngine.refine_host(w[i], radii, steps, lv.cost_scale) for i, (radii, steps) in enumerate(stages)]
        res = dict(poses=best.copy(), cost=dec[-1]["cost"], score=dec[-1]["score"], start_cost=dec[0]["start_cost"],
                   offsets=np.stack([d["offsets"] for d in dec], axis=1))
        if rays is not None:
            res["through"] = thr[0].T.copy()
        return res

    def points_level(self, level, half, points, likelihood=None, shared=True):
        """The covering level of ``searchPoints`` / ``refinePoints``: that of ``searchPoses`` for the same window -- the same
        cached level -- while no valid point lies further from the robot than lidarMaxRange; else the level of a window wider by
        the excess, so that the points of a pose in the window still end in the field, where slam2d_field_build accepts that
        level (``field_build_limits``).  Where it does not, the far points simply pay ``outside_cost``."""
        extra = max(0.0, points_reach(points) - self.og.lidarMaxRange)
        if extra > 0.0:
            try:
                return self.covering_level(level, half + extra, shared=shared, likelihood=likelihood)
            except ValueError:
                pass
        return self.covering_level(level, half, shared=shared, likelihood=likelihood)

    def searchPoints(self, points, window, step=None, headings=120, level="fine", top=5, separation=None, outside_cost=None,
                     likelihood=None):
        """``searchPoses`` for a set of points in the robot's frame instead of one scan (include/slam2d.h, slam2d_search_points):
        ``points`` is ``[M, 2]`` -- x forward, y to the left, metres; rows with a NaN or an infinity are dropped --, M <=
        ``_lib.MAX_POINTS``: several scans joined by odometry (``points.merge_scans``), two sensors, a sensor off the robot's
        origin, a driver's own beam angles (``points.polar_points``).  The same lattice, cost, peaks and return value; the
        field is ``points_level``'s.  ``self.last_cover`` keeps the level, its window and the ``Lattice``."""
        pts = points_of(points)
        window = covering_window(None, window)
        lv = self.points_level(level, window[2], pts, likelihood)
        return self._search("searchPoints", lv, window, step, headings, top, separation, outside_cost,
                            lambda eng, lat, cost: eng.search_points(lv, 0, lat, eng.to_device(pts), len(pts), cost))

    def refinePoints(self, poses, points, stages=None, level="fine", window=None, likelihood=None, outside_cost=None):
        """``refinePoses`` for a set of points in the robot's frame instead of a scan (include/slam2d.h, slam2d_refine_points):
        ``points`` is ``[M, 2]``, one set for every seed, or ``[N, M, 2]``, a set per seed (rows with a NaN or an infinity are
        dropped, so sets of different sizes are padded with NaN rows).  The same stages, frame planning and return value; the
        field is ``points_level``'s."""
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        N = len(poses)
        if N == 0:
            raise ValueError("no poses")
        pts = points_of(points, N)
        M = pts.shape[-2]
        window = covering_window(poses, window)
        lv = self.points_level(level, window[2], pts, likelihood)
        return self._refine("refinePoints", lv, window, poses, pts, stages, outside_cost,
                            lambda eng, a, b, d_pts, radii, steps, cost, words:
                            eng.refine_points(lv, 0, a, b, N, 3, d_pts, M, 0 if pts.ndim == 2 else 2 * M, radii, steps, cost, d_words=words))

    def scorePoints(self, poses, points, level="fine", window=None, likelihood=None):
        """``scorePoses`` for a set of points in the robot's frame instead of a scan (include/slam2d.h, slam2d_score_points):
        ``points`` is ``[M, 2]``, one set for every pose, or ``[N, M, 2]``, a set per pose (rows with a NaN or an infinity are
        dropped, so sets of different sizes are padded with NaN rows).  The frame is planned as for ``refinePoints`` (the
        bounding box of the finite poses, or ``window``; the field is ``points_level``'s).  Returns ``scorePoses``' dict with
        ``valid``, the number of valid points, where that has ``in_range``."""
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        N = len(poses)
        if N == 0:
            raise ValueError("no poses")
        pts = points_of(points, N)
        M = pts.shape[-2]
        cx, cy, half = covering_window(poses, window)
        lv = self.points_level(level, half, pts, likelihood)
        with self._cover(lv, cx, cy) as (eng, _):
            rows = eng.score_points(lv, 0, eng.to_device(poses), 3, N, eng.to_device(pts), M, 0 if pts.ndim == 2 else 2 * M)
            host, = self._download(eng, "scorePoints", rows)
            self.last_cover = dict(level=lv, window=(cx, cy, half))
            res = eng.score_host(host)
        res["valid"] = res.pop("in_range")
        return res

    def searchToMatch(self, probSP, estimatedX, estimatedY, estimatedTheta, rMeasure, xRangeList, yRangeList,
                      searchRadius, searchHalfRad, unitLength, estMovingDist, estMovingTheta, fineSearch=False,
                      matchMax=True):
        """(:91-151) on a caller-supplied field (re-quantised to the device's fixed-point format)."""
        rMeasure = np.asarray(rMeasure)
        level = self._level(unitLength, 1.0, 0.5, searchRadius, searchHalfRad, fineSearch)
        with _Exclusive(level):
            return self._search_to_match(level, probSP, estimatedX, estimatedY, estimatedTheta, rMeasure, xRangeList,
                                         yRangeList, estMovingDist, estMovingTheta, matchMax)

    def _search_to_match(self, level, probSP, estimatedX, estimatedY, estimatedTheta, rMeasure, xRangeList, yRangeList,
                         estMovingDist, estMovingTheta, matchMax):
        eng = self.og.engine()
        fh, fw = probSP.shape
        if fh > level.fmax or fw > level.fmax:
            raise ValueError("field larger than this matcher's search window")
        level.set_field(probSP, 0)
        fr = level.frames()
        fr[0]["xlo"], fr[0]["xhi"], fr[0]["ylo"], fr[0]["yhi"] = xRangeList[0], xRangeList[1], yRangeList[0], yRangeList[1]
        fr[0]["fh"], fr[0]["fw"] = fh, fw
        level.t["frames"].copy_(torch.from_numpy(fr.view(np.uint8).reshape(1, -1)))
        d_est = eng.to_device([[estimatedX, estimatedY, estimatedTheta]])
        d_rng = eng.to_device(rMeasure)
        d_psi = eng.to_device(eng.psi_table([estMovingTheta]))
        d_u = None if matchMax else eng.to_device([np.random.random_sample()])
        out = eng.match_buffer("adhoc")
        eng.sweep(level, d_est, 3, d_rng, estMovingDist, d_psi, d_u, out)
        eng.take_flags()
        m = eng.read_matches(out)[0]
        matched = {"x": float(m["x"]), "y": float(m["y"]), "theta": float(m["theta"]), "range": rMeasure}
        px, py = self.covertMeasureToXY(estimatedX, estimatedY, estimatedTheta, rMeasure)
        dth = matched["theta"] - estimatedTheta
        mpx, mpy = self.rotate((estimatedX, estimatedY), (px, py), dth)
        dx, dy = matched["x"] - estimatedX, matched["y"] - estimatedY
        self.last = dict(adhoc=m.copy())
        return mpx + dx, mpy + dy, matched, level.cube(0), np.float64(m["confidence"])

    # ---- small host helpers of the reference's surface ----
    def covertMeasureToXY(self, estimatedX, estimatedY, estimatedTheta, rMeasure):      # :81-89
        og = self.og
        rads = np.linspace(estimatedTheta - og.lidarFOV / 2, estimatedTheta + og.lidarFOV / 2, num=og.numSamplesPerRev)
        keep = rMeasure < og.lidarMaxRange
        return estimatedX + np.cos(rads[keep]) * rMeasure[keep], estimatedY + np.sin(rads[keep]) * rMeasure[keep]

    def rotate(self, origin, point, angle):                                             # :162-171
        ox, oy = origin
        px, py = point
        return (ox + np.cos(angle) * (px - ox) - np.sin(angle) * (py - oy),
                oy + np.sin(angle) * (px - ox) + np.cos(angle) * (py - oy))

    def convertXYToSearchSpaceIdx(self, px, py, beginX, beginY, unitLength):            # :173-176
        return (((px - beginX) / unitLength)).astype(int), (((py - beginY) / unitLength)).astype(int)

    def __deepcopy__(self, memo):
        new = ScanMatcher.__new__(ScanMatcher)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            # og: clones the device map, alias preserved via memo; last_cover names a SHARED level (_shared_level): by reference
            setattr(new, k, v if k == "last_cover" else copy.deepcopy(v, memo))
        return new
