"""``Localiser``: Monte-Carlo localisation in a map that is already built -- follow a robot through it, scan by scan.  ``Tracker``
(below it): the same with ONE pose and a local search per scan, for a robot whose start is known.

N pose hypotheses live on the device.  One call per scan (slam2d_mcl_step, include/slam2d.h) moves them by the odometry
increment, weighs them against ONE field of the map built once, resamples them and leaves the new set where it was: a scan
costs an upload of its ranges and, if the estimate is wanted at once, a download of 128 bytes.  The step is defined in integers
and rounded IEEE operations, so a run is the same bits every time; the generator is restated here in NumPy for the host-side
seeding of the set.
"""
import collections
import math

import numpy as np
import torch

from . import _lib
from .engine import kld_table, mcl_adapt_report_host, mcl_rays_report_host, mcl_report_host, pinned_stream, refine_host, weight_table
from .matcher import check_stages, covering_window, points_of, ranges_of, ray_margin, same_frames

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xffffffff)
_IH_STD = math.sqrt(4.0 / 3.0)                                 # std of the Irwin-Hall noise g at amplitude 1
# draws of the generator: 0-2 are the step's own (include/slam2d.h); the host-side seeding takes the next ones of the same counter
_DRAW_SPREAD, _DRAW_UNIFORM = (3, 4, 5), 6


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011) as slam2d_mcl_step runs it: ``counter`` four 32-bit words (scalars or arrays that
    broadcast), ``key`` two; uint32 [..., 4]."""
    c = [v & _MASK for v in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = (int(v) & 0xffffffff for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]                  # (32 x 32 bits: exact in 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xffffffff, (k1 + _W1) & 0xffffffff
    return np.stack(c, axis=-1).astype(np.uint32)


def _words(N, draws, seed, scan):
    seed, scan = int(seed) & 0xffffffffffffffff, int(scan) & 0xffffffffffffffff
    n = np.arange(N, dtype=np.uint64).reshape(-1, 1)
    j = np.asarray(draws, dtype=np.uint64).reshape(1, -1)
    return philox4x32_10((n, j, scan & 0xffffffff, scan >> 32), (seed & 0xffffffff, seed >> 32))


def noise(N, draws, seed, scan):
    """g [N, len(draws)] of the step's definition: the four words of counter (n, draw, scan) summed as int32, times 2^-31."""
    return _words(N, draws, seed, scan).view(np.int32).astype(np.int64).sum(axis=-1).astype(np.float64) * 2.0 ** -31


def odometry_motion(prev, cur):
    """(dfwd, dside, dturn): the step from raw odometry pose ``prev`` to ``cur`` (dicts with x, y, theta, or triples), in the
    frame of ``prev``."""
    (x0, y0, t0), (x1, y1, t1) = (((p["x"], p["y"], p["theta"]) if isinstance(p, dict) else p) for p in (prev, cur))
    dx, dy = float(x1) - float(x0), float(y1) - float(y0)
    c, s = math.cos(t0), math.sin(t0)
    return c * dx + s * dy, c * dy - s * dx, float(t1) - float(t0)


def ray_options(rays, beams, step, wall_thickness, outside_cost):
    """``Localiser``'s ``rays`` with its defaults filled in: ``stride`` (4: one beam in four is cast), ``margin``
    (``matcher.ray_margin`` of the wall thickness and the field's step), ``through_cost`` (min(stride * outside_cost, 2^32 - 1): a
    cast beam stands for ``stride`` beams) and ``rotate`` (True: the phase is the scan number mod stride).  ValueError for an
    unknown key, a stride outside 1 .. beams, a margin below 0 or a through_cost outside 32 bits."""
    opt = dict(rays)
    unknown = set(opt) - {"stride", "margin", "through_cost", "rotate"}
    if unknown:
        raise ValueError(f"rays: unknown keys {sorted(unknown)}")
    stride = int(opt.get("stride", 4))
    if not 1 <= stride <= int(beams):
        raise ValueError(f"rays: stride wants 1 .. {int(beams)} (the beams), not {opt.get('stride')!r}")
    margin = int(opt.get("margin", ray_margin(wall_thickness, step)))
    if margin < 0:
        raise ValueError(f"rays: margin wants a count of samples >= 0, not {margin}")
    through_cost = int(opt.get("through_cost", min(stride * int(outside_cost), 2 ** 32 - 1)))
    if not 0 <= through_cost < 2 ** 32:
        raise ValueError(f"rays: through_cost wants 0 .. 2^32 - 1, not {through_cost}")
    return dict(stride=stride, margin=margin, through_cost=through_cost, rotate=bool(opt.get("rotate", True)))


class _OnCover:
    """What ``Localiser`` and ``Tracker`` start from: the covering field of a window, built ONCE in a level of the object's own."""

    def _plan_cover(self, matcher, window, level, likelihood, outside_cost):
        """The window, the level and the outside cost; nothing is built yet.  Returns the level."""
        self.matcher = matcher
        self.window = covering_window(None, window)
        lv = self.level = matcher.covering_level(level, self.window[2], shared=False, likelihood=likelihood)
        self.outside_cost = matcher.outside_cost_of(lv) if outside_cost is None else int(outside_cost)
        return lv

    def _build_cover(self, dist2=False):
        """The level's field (``ScanMatcher._cover``) and its fault bits.  Returns the engine's device; ``dist2``: and what the
        build returned -- a distance level's squared distances."""
        with self.matcher._cover(self.level, *self.window[:2], dist2=dist2) as (eng, built):
            self.eng = eng
            eng.take_flags()
        return (eng.device, built) if dist2 else eng.device

    def _twin_dist2(self, level):
        """The squared distances of the blurred field's frame: a copy of what the matcher's cached distance level of this window
        gives -- that level is shared, and other calls rebuild it."""
        lvd = self.matcher._distance_twin(level, self.window[2])
        with self.matcher._cover(lvd, *self.window[:2], dist2=True) as (eng, d2):
            same_frames(self.level, lvd)
            eng.take_flags()
            return d2.clone()


class Localiser(_OnCover):
    """Monte-Carlo localisation in ``matcher``'s map, taken as static.

    ``window = (cx, cy, half)``: the square the robot stays in; the constructor builds the field of ``matcher``'s ``level``
    ('fine' or 'coarse') that covers it plus lidarMaxRange ONCE, as ``ScanMatcher.searchPoses`` does (the map grows to hold
    that frame), in a level of its own.  ``particles``: the size of the set; ``sigma = (fwd, side, turn)``: the standard
    deviations of the motion noise per step (metres, metres, radians; the step's amplitudes are these / sqrt(4/3));
    ``temperature``: of the weights (``engine.weight_table``; 1.0 is the reference's soft-max); ``seed``: the generator's key;
    ``outside_cost``: what an in-range beam that ends outside the field pays (default: free space as the field encodes it).
    ``likelihood``: None, or the dict of ``ScanMatcher.covering_level``: the poses are weighed against the likelihood field --
    a table of the exact distance to the nearest wall, slam2d_field_build_distance -- instead of the blurred one, and the default
    ``outside_cost`` is the table's last entry.
    Seed the set with ``seed_at``, ``seed_from_peaks`` or ``seed_uniform``, then ``step`` or ``run``.

    ``adaptive``: None -- the set keeps its size -- or a dict of ``n_min``, ``bin_xy`` (0.5 m), ``bin_theta`` (10 degrees, in
    radians), ``epsilon`` (0.05) and ``z`` (2.326), any of them left to its default: KLD-sampling (slam2d_mcl_step_adaptive,
    ``engine.kld_table``).  ``particles`` is then the capacity and the initial count; every step counts the pose bins of
    ``bin_xy`` x ``bin_xy`` x ``bin_theta`` over the window that the resampled set occupies and resamples to as many poses as
    the table wants for that number, between ``n_min`` and the capacity.  The count lives in one device word and travels from
    call to call there; ``count`` downloads it, the reports carry it (``n_in``, ``n_out``), and the seeding calls take any
    ``count`` from 1 to the capacity.

    ``rays``: None -- the endpoint model alone, and nothing more is built or kept -- or a dict of ``stride``, ``margin``,
    ``through_cost`` and ``rotate`` (``ray_options`` has the defaults): every step charges a hypothesis ``through_cost`` for each
    cast beam -- one in ``stride``, all of them once in ``stride`` scans with ``rotate`` -- whose measured range lies more than
    ``margin`` samples beyond a wall of the map (slam2d_mcl_step_rays), so a cloud on the wrong side of a wall loses the
    resampling.  The squared wall distances the rays skip by are the Localiser's own: with ``likelihood`` what its one distance
    build returns, else a copy of what ``clearance``'s cached distance level of the same window gives.  The reports gain
    ``through`` (``engine.mcl_rays_report_host``); the point forms take no rays."""

    rays = None                                                # (the filled-in options; None: the endpoint model alone)

    def __init__(self, matcher, window, particles=4096, level="fine", sigma=(0.05, 0.05, 0.02), temperature=1.0, seed=0,
                 outside_cost=None, adaptive=None, likelihood=None, rays=None):
        self.N = int(particles)
        if not 1 <= self.N <= _lib.MCL_MAX_PARTICLES:
            raise ValueError(f"particles wants 1 .. {_lib.MCL_MAX_PARTICLES}, not {particles!r}")
        self.sigma = tuple(float(v) for v in sigma)
        if len(self.sigma) != 3 or not all(math.isfinite(v) and v >= 0 for v in self.sigma):
            raise ValueError(f"sigma = (fwd, side, turn) wants three finite numbers >= 0, not {sigma!r}")
        self.amp = tuple(v / _IH_STD for v in self.sigma)
        self.seed = int(seed) & 0xffffffffffffffff
        self.scan = 0                                          # the number of the next scan: part of the generator's counter
        lv = self._plan_cover(matcher, window, level, likelihood, outside_cost)
        self.rays = None if rays is None else ray_options(rays, matcher.og.numSamplesPerRev, lv.step, matcher.og.wallThickness, self.outside_cost)
        if self.rays is None:
            dev = self._build_cover()
        elif likelihood is not None:
            dev, self.d_dist2 = self._build_cover(dist2=True)
        else:
            dev = self._build_cover()
            self.d_dist2 = self._twin_dist2(level)
        lut, self.shift = weight_table(lv.cost_scale, temperature)          # (the distance build has put its table's scale there)
        self.d_lut = torch.from_numpy(lut.view(np.int32)).to(dev)
        self.d_pose = [torch.zeros((self.N, 3), dtype=torch.float64, device=dev) for _ in range(2)]     # ping-pong
        self.cur = 0
        self.d_ancestor = torch.empty(self.N, dtype=torch.int32, device=dev)
        self.d_report = torch.empty(_lib.MCL_REPORT, dtype=torch.int64, device=dev)
        self.d_ranges = torch.empty(matcher.og.numSamplesPerRev, dtype=torch.float64, device=dev)
        self.adaptive = None
        self._decode = mcl_report_host                          # of a report, and through its length of the step, chosen once
        if adaptive is not None:
            self._init_adaptive(dict(adaptive))
        if self.rays is not None:
            self._decode = mcl_rays_report_host                 # (either length)

    def _init_adaptive(self, opt):
        unknown = set(opt) - {"n_min", "bin_xy", "bin_theta", "epsilon", "z"}
        if unknown:
            raise ValueError(f"adaptive: unknown keys {sorted(unknown)}")
        cx, cy, half = self.window
        n_min = int(opt.get("n_min", min(self.N, 256)))
        bin_xy, bin_theta = float(opt.get("bin_xy", 0.5)), float(opt.get("bin_theta", math.radians(10.0)))
        if not (math.isfinite(bin_xy) and bin_xy > 0 and math.isfinite(bin_theta) and 0 < bin_theta <= 2 * math.pi):
            raise ValueError(f"adaptive: bin_xy wants a positive number and bin_theta one in (0, 2 pi], not {bin_xy!r}, {bin_theta!r}")
        side, nth = max(1, math.ceil(2 * half / bin_xy)), max(1, round(2 * math.pi / bin_theta))
        if side * side * nth > _lib.MCL_MAX_BINS:
            raise ValueError(f"adaptive: {side} x {side} x {nth} bins, more than {_lib.MCL_MAX_BINS}")
        epsilon, z = float(opt.get("epsilon", 0.05)), float(opt.get("z", 2.326))
        tab = kld_table(epsilon, z, n_min, self.N)
        dev = self.eng.device
        self.bins = _lib.Slam2dMclBins(x0=cx - half, y0=cy - half, cell=bin_xy, turn=2 * math.pi / nth, nx=side, ny=side, nth=nth)
        self.ntab = tab
        self.d_ntab = torch.from_numpy(tab.view(np.int32)).to(dev)
        self.d_count = torch.full((1,), self.N, dtype=torch.int32, device=dev)
        self.d_report = torch.empty(_lib.MCL_ADAPT_REPORT, dtype=torch.int64, device=dev)
        self._decode = mcl_adapt_report_host
        self.adaptive = dict(n_min=n_min, bin_xy=bin_xy, bin_theta=bin_theta, epsilon=epsilon, z=z)

    @property
    def count(self):
        """The number of live poses: the size of the set, or with ``adaptive`` the device's count word, downloaded."""
        return self.N if self.adaptive is None else int(self.d_count.cpu()[0])

    # ---- the set ----
    def set_poses(self, poses):
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 3))
        if self.adaptive is not None:
            if not 1 <= len(poses) <= self.N:
                raise ValueError(f"{len(poses)} poses for a set of 1 .. {self.N}")
            self.d_pose[self.cur][:len(poses)].copy_(torch.from_numpy(poses))
            self.d_count.fill_(len(poses))
            return poses
        if len(poses) != self.N:
            raise ValueError(f"{len(poses)} poses for a set of {self.N}")
        self.d_pose[self.cur].copy_(torch.from_numpy(poses))
        return poses

    def _seed_count(self, count):
        if count is None:
            return self.N
        if self.adaptive is None and int(count) != self.N:
            raise ValueError(f"count = {count!r}: a set of fixed size holds {self.N} (see adaptive)")
        if not 1 <= int(count) <= self.N:
            raise ValueError(f"count wants 1 .. {self.N}, not {count!r}")
        return int(count)

    def seed_at(self, pose, spread, count=None):
        """The set around ``pose`` = (x, y, theta): pose + spread * g / sqrt(4/3) per component, g the step's noise at draws 3-5 of
        the current scan number.  ``spread``: one standard deviation for all three, or (sx, sy, stheta).  ``count``: how many
        poses, with ``adaptive`` (default: the capacity).  Returns the poses."""
        return self.seed_from_peaks([pose], spread, count)

    def seed_from_peaks(self, peaks, spread, count=None):
        """The set shared out in turn among ``peaks`` -- ``Peak``s of ``ScanMatcher.searchPoses`` or (x, y, theta) triples:
        particle n around peak n mod len(peaks), spread as in ``seed_at``."""
        centres = np.array([[float(p.x), float(p.y), float(p.theta)] if hasattr(p, "theta") else [float(v) for v in p[:3]] for p in peaks])
        if not len(centres):
            raise ValueError("no peaks")
        sp = np.broadcast_to(np.asarray(spread, dtype=np.float64), (3,))
        n = self._seed_count(count)
        g = noise(n, _DRAW_SPREAD, self.seed, self.scan)
        return self.set_poses(centres[np.arange(n) % len(centres)] + (sp / _IH_STD) * g)

    def seed_uniform(self, count=None):
        """The set uniform over the window and the full turn: words 0-2 of draw 6 of the current scan number, over 2^32."""
        cx, cy, half = self.window
        u = _words(self._seed_count(count), (_DRAW_UNIFORM,), self.seed, self.scan)[:, 0, :3].astype(np.float64) * 2.0 ** -32
        return self.set_poses(np.column_stack([cx + (2 * u[:, 0] - 1) * half, cy + (2 * u[:, 1] - 1) * half, -math.pi + 2 * math.pi * u[:, 2]]))

    def poses(self):
        """The current set, downloaded: [N, 3]; with ``adaptive`` its first ``count`` rows."""
        if self.adaptive is not None:
            return self.d_pose[self.cur][:self.count].cpu().numpy()
        return self.d_pose[self.cur].cpu().numpy()

    # ---- the filter ----
    def _enqueue(self, source, motion, d_report, points=False):
        """One step on the device.  ``source``: the scan's ranges, or -- ``points`` -- the set's (d_points, M)."""
        eng, d_in, d_out = self.eng, self.d_pose[self.cur], self.d_pose[1 - self.cur]
        src = source if points else (source,)
        if self.rays is not None:
            r = self.rays
            charge = (r["stride"], self.scan % r["stride"] if r["rotate"] else 0, r["margin"], r["through_cost"])
            if self.adaptive is not None:
                eng.mcl_step_adaptive_rays(self.level, 0, self.d_dist2, d_in, d_out, self.N, self.d_count, motion, self.amp, self.seed, self.scan,
                                           *src, self.outside_cost, *charge, self.d_lut, self.shift, self.bins, self.d_ntab, d_report,
                                           self.d_ancestor)
            else:
                eng.mcl_step_rays(self.level, 0, self.d_dist2, d_in, d_out, self.N, motion, self.amp, self.seed, self.scan, *src,
                                  self.outside_cost, *charge, self.d_lut, self.shift, d_report, self.d_ancestor)
        elif self.adaptive is not None:
            step = eng.mcl_step_adaptive_points if points else eng.mcl_step_adaptive
            step(self.level, 0, d_in, d_out, self.N, self.d_count, motion, self.amp, self.seed, self.scan, *src,
                 self.outside_cost, self.d_lut, self.shift, self.bins, self.d_ntab, d_report, self.d_ancestor)
        else:
            step = eng.mcl_step_points if points else eng.mcl_step
            step(self.level, 0, d_in, d_out, self.N, motion, self.amp, self.seed, self.scan, *src, self.outside_cost, self.d_lut,
                 self.shift, d_report, self.d_ancestor)
        self.cur = 1 - self.cur
        self.scan += 1

    def step(self, reading_or_ranges, motion):
        """One scan: the set moved by ``motion`` = (dfwd, dside, dturn) in the robot's own previous frame, weighed against the scan
        and resampled.  One call, one download of 128 bytes: the report as ``engine.mcl_report_host`` decodes it --
        ``mean_pose`` is the estimate (192 bytes and ``engine.mcl_adapt_report_host`` with ``adaptive``)."""
        self.d_ranges.copy_(torch.from_numpy(ranges_of(reading_or_ranges, self.d_ranges.numel())))
        self._enqueue(self.d_ranges, motion, self.d_report)
        return self._decode(self.d_report)

    def run(self, readings):
        """A log: the motion of scan i is the step from raw odometry pose i - 1 to i in the frame of pose i - 1 (nothing for the
        first scan).  Every scan is enqueued without a synchronisation, the reports go to one [S, 16] device array ([S, 24] with
        ``adaptive``, whose count goes from call to call on the device), and ONE download ends the call.  Returns the list of
        decoded reports."""
        beams = self.d_ranges.numel()
        rng = np.stack([ranges_of(r, beams) for r in readings])
        with pinned_stream():
            d_rng = torch.from_numpy(rng).to(self.eng.device)
            d_rep = torch.empty((len(readings), self.d_report.numel()), dtype=torch.int64, device=self.eng.device)
            for i in range(len(readings)):
                self._enqueue(d_rng[i], odometry_motion(readings[i - 1], readings[i]) if i else (0.0, 0.0, 0.0), d_rep[i])
            host = d_rep.cpu().numpy()
        return [self._decode(row) for row in host]

    def _no_rays(self, name):
        if self.rays is not None:
            raise ValueError(f"{name}: a Localiser with rays takes scans only -- a point set has no single ray origin (rays=None)")

    def step_points(self, points, motion):
        """``step`` for a set of points in the robot's frame instead of a scan (slam2d_mcl_step_points, include/slam2d.h):
        ``points`` is ``[M, 2]`` -- x forward, y to the left, metres; rows with a NaN or an infinity are dropped --, M <=
        ``_lib.MAX_POINTS``, as the ``points`` module prepares them: several scans merged by odometry, two sensors, a mounted
        one.  The field is the one the constructor built: a point that ends outside it pays ``outside_cost``.  The same
        download and the same report, whose ``in_range`` is the number of valid points."""
        self._no_rays("step_points")
        pts = points_of(points)
        self._enqueue((torch.from_numpy(pts).to(self.eng.device), len(pts)), motion, self.d_report, points=True)
        return self._decode(self.d_report)

    def run_points(self, point_sets, motions):
        """A log of point sets: set i, ``[M_i, 2]``, with the motion ``motions[i]`` = (dfwd, dside, dturn) that led to it.  The
        sets may differ in length: they are padded with NaN rows to the longest.  As in ``run`` every step is enqueued without
        a synchronisation and ONE download of the reports ends the call.  Returns the list of decoded reports."""
        self._no_rays("run_points")
        sets = [points_of(p) for p in point_sets]
        motions = [tuple(float(v) for v in m) for m in motions]
        if not sets or len(motions) != len(sets) or any(len(m) != 3 for m in motions):
            raise ValueError(f"{len(sets)} point sets and {len(motions)} motions: want one motion of three numbers per set, and a set")
        M = max(len(p) for p in sets)
        pts = np.full((len(sets), M, 2), np.nan)
        for i, p in enumerate(sets):
            pts[i, :len(p)] = p
        with pinned_stream():
            d_pts = torch.from_numpy(pts).to(self.eng.device)
            d_rep = torch.empty((len(sets), self.d_report.numel()), dtype=torch.int64, device=self.eng.device)
            for i in range(len(sets)):
                self._enqueue((d_pts[i], M), motions[i], d_rep[i], points=True)
            host = d_rep.cpu().numpy()
        return [self._decode(row) for row in host]


TrackReport =collections.namedtuple("TrackReport", "pose cost start_cost offsets")
TrackRaysReport = collections.namedtuple("TrackRaysReport", "pose cost start_cost offsets through")


def track_report_host(row, stages, cost_scale, rays=False):
    """A downloaded row of a ``Tracker``'s scan -- the pose, the stages' two words as doubles' bits and, with ``rays``, the stages'
    through counts, 32-bit words two to a double -- as a ``TrackReport`` or a ``TrackRaysReport``."""
    row = np.ascontiguousarray(row, dtype=np.float64).reshape(-1)
    n = 3 + _lib.REFINE_STRIDE * len(stages)
    words = row[3:n].view(np.uint64).reshape(len(stages), _lib.REFINE_STRIDE)
    dec = [refine_host(words[i], radii, steps, cost_scale) for i, (radii, steps) in enumerate(stages)]
    head = (tuple(float(v) for v in row[:3]), int(dec[-1]["cost"][0]), int(dec[0]["start_cost"][0]), np.stack([d["offsets"][0] for d in dec]))
    if not rays:
        return TrackReport(*head)
    return TrackRaysReport(*head, row[n:].view(np.uint32)[:len(stages)].astype(np.int64))


class Tracker(_OnCover):
    """Position tracking in ``matcher``'s map, taken as static: ONE pose follows the robot, scan by scan -- the cheapest
    localisation, for a robot whose start is known (``ScanMatcher.searchPoses`` finds one).

    ``window = (cx, cy, half)``, ``level``, ``likelihood`` and ``outside_cost`` as for ``Localiser``: the constructor builds the
    covering field ONCE, in a level of its own.  ``stages``: those of ``ScanMatcher.refinePoses`` (None: ``default_stages`` of
    the level's step).  A scan moves the pose by the odometry increment and searches the stages' lattices about it
    (slam2d_refine_poses, include/slam2d.h, with N = 1; the motion goes into the first stage): the pose lives on the device
    across calls, a scan costs an upload of its ranges and, if the pose is wanted at once, a download of 24 + 16 bytes per
    stage.  Integer costs and rounded operations: a run is the same bits every time.

    ``rays``: None -- the endpoint cost alone: nothing more is built, kept or downloaded -- or a dict as for ``Localiser``
    (``ray_options``: ``stride``, ``margin``, ``through_cost``, ``rotate``): every candidate of every stage pays ``through_cost``
    for each cast beam whose measured range lies more than ``margin`` samples beyond a wall of the map
    (slam2d_refine_poses_rays), so the one pose does not step through a wall that its lattice straddles; one phase per scan --
    the scan number mod ``stride`` with ``rotate`` -- serves all its stages.  The squared distances come as ``Localiser``'s do.
    ``step`` and ``run`` then return ``TrackRaysReport``s, with ``through`` [stages]: the through beams of each stage's winner,
    four more bytes per stage in the same download; ``step_points`` takes no rays."""

    rays = None                                                # (the filled-in options; None: the endpoint cost alone)

    def __init__(self, matcher, window, level="fine", stages=None, likelihood=None, outside_cost=None, rays=None):
        lv = self._plan_cover(matcher, window, level, likelihood, outside_cost)
        self.stages = check_stages(stages, lv.step)
        self.rays = None if rays is None else ray_options(rays, matcher.og.numSamplesPerRev, lv.step, matcher.og.wallThickness, self.outside_cost)
        self.scan = 0                                          # the number of the next scan: the phase of a rotating stride
        if self.rays is None:
            dev = self._build_cover()
        elif likelihood is not None:
            dev, self.d_dist2 = self._build_cover(dist2=True)
        else:
            dev = self._build_cover()
            self.d_dist2 = self._twin_dist2(level)
        self.d_pose = [torch.zeros(3, dtype=torch.float64, device=dev) for _ in range(2)]               # ping-pong
        self.cur = 0
        self.d_ranges = torch.empty(matcher.og.numSamplesPerRev, dtype=torch.float64, device=dev)
        # what one step downloads: the pose, then the stages' words (as doubles' bits)
        # (with rays: and the stages' through counts, 32-bit words two to a double)
        self._words = 3 + _lib.REFINE_STRIDE * len(self.stages)
        self.d_report = torch.empty(self._words + (0 if self.rays is None else (len(self.stages) + 1) // 2), dtype=torch.float64, device=dev)

    def set_pose(self, pose):
        pose = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).reshape(3))
        self.d_pose[self.cur].copy_(torch.from_numpy(pose))
        return pose

    def pose(self):
        """The current pose, downloaded: (x, y, theta)."""
        return tuple(float(v) for v in self.d_pose[self.cur].cpu().numpy())

    def _enqueue(self, refine, source, motion, d_report):
        """The stages of one scan or one point set: ``refine`` is the engine's ``refine_poses`` or ``refine_points``, ``source`` its
        arguments between the pose stride and the radii.  The last stage's pose also goes to the head of ``d_report`` (a row like
        ``self.d_report``), the stages' words behind it."""
        d_words = d_report[3:self._words].view(torch.int64).view(len(self.stages), _lib.REFINE_STRIDE)
        if self.rays is not None:
            r = self.rays
            charge = (r["stride"], self.scan % r["stride"] if r["rotate"] else 0, r["margin"], r["through_cost"])
            d_through = d_report[self._words:].view(torch.int32)
        for i, (radii, steps) in enumerate(self.stages):
            if self.rays is not None:
                self.eng.refine_poses_rays(self.level, 0, self.d_dist2, self.d_pose[self.cur], self.d_pose[1 - self.cur], 1, 3, *source, radii, steps,
                                           self.outside_cost, *charge, motion=motion if i == 0 else None, d_words=d_words[i],
                                           d_through=d_through[i:i + 1])
            else:
                refine(self.level, 0, self.d_pose[self.cur], self.d_pose[1 - self.cur], 1, 3, *source, radii, steps, self.outside_cost,
                       motion=motion if i == 0 else None, d_words=d_words[i])
            self.cur = 1 - self.cur
        d_report[:3].copy_(self.d_pose[self.cur])
        self.scan += 1

    def _report(self, row):
        """A downloaded row of ``_enqueue`` as a ``TrackReport``."""
        return track_report_host(row, self.stages, self.level.cost_scale, self.rays is not None)

    def step(self, reading_or_ranges, motion):
        """One scan: the pose moved by ``motion`` = (dfwd, dside, dturn) in the robot's own previous frame (None: not moved), then
        refined against the scan.  One small download; returns ``TrackReport(pose, cost, start_cost, offsets)``: the new pose,
        its cost, the cost of the moved pose before the search and the stages' signed steps [stages, 3]."""
        self.d_ranges.copy_(torch.from_numpy(ranges_of(reading_or_ranges, self.d_ranges.numel())))
        with pinned_stream():
            self._enqueue(self.eng.refine_poses, (self.d_ranges, 0), motion, self.d_report)
            return self._report(self.d_report.cpu().numpy())

    def step_points(self, points, motion):
        """``step`` for a set of points in the robot's frame instead of a scan (slam2d_refine_points, include/slam2d.h):
        ``points`` is ``[M, 2]`` -- x forward, y to the left, metres; rows with a NaN or an infinity are dropped --, M <=
        ``_lib.MAX_POINTS``, as the ``points`` module prepares them.  The field is the one the constructor built: a point that
        ends outside it pays ``outside_cost``.  The same stages, the same download, the same ``TrackReport``."""
        if self.rays is not None:
            raise ValueError("step_points: a Tracker with rays takes scans only -- a point set has no single ray origin (rays=None)")
        pts = points_of(points)
        with pinned_stream():
            self._enqueue(self.eng.refine_points, (torch.from_numpy(pts).to(self.eng.device), len(pts), 0), motion, self.d_report)
            return self._report(self.d_report.cpu().numpy())

    def run(self, readings):
        """A log, as ``Localiser.run`` takes it: the motion of scan i is the step from raw odometry pose i - 1 to i in the frame of
        pose i - 1 (nothing for the first scan).  Every scan is enqueued without a synchronisation; ONE download of the [S, 3]
        poses and the [S, stages, 2] words ends the call.  Returns the list of ``TrackReport``s."""
        beams = self.d_ranges.numel()
        rng = np.stack([ranges_of(r, beams) for r in readings])
        with pinned_stream():
            dev = self.eng.device
            d_rng = torch.from_numpy(rng).to(dev)
            d_rep = torch.empty((len(readings), self.d_report.numel()), dtype=torch.float64, device=dev)
            for i in range(len(readings)):
                self._enqueue(self.eng.refine_poses, (d_rng[i], 0), odometry_motion(readings[i - 1], readings[i]) if i else None, d_rep[i])
            host = d_rep.cpu().numpy()
        return [self._report(row) for row in host]
