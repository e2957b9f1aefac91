"""The per-scan pose bookkeeping at its edges (Algorithm/FastSlam.py:77-120: updateEstimatedPose, getMovingTheta): ONE case
table, shared by the generator of ``bookkeeping_edges.npz`` (make_golden_bookkeeping.py), by the CPU test that holds the oracle
and the filter's host mirror to it, and by the GPU tests that hold prior_one / post_match_one of csrc/slam2d.hip to the oracle.
Every choice is seeded; nothing here imports the reference.

Post-match cases: a particle's previous matched (x, y), the fine match (x, y, theta) it moves to and the coarse record
(x, y, theta, confidence, log_confidence) that travels with it.  Prior cases: a particle's previous matched pose and heading
(NaN: none) and the raw odometry around it -- the raw readings and the previous raw heading are chosen so that the reference
itself arrives at the wanted (has_turn, raw_turn).
"""
import math
from types import SimpleNamespace

import numpy as np

SEED = 77106
LATTICE_UNITS = (0.02, 0.05, 0.1)
LATTICE_SPAN = 3                        # moves (i, j) * unit, i, j in -3 .. 3
N_RANDOM = 200
EXACT_HEADINGS = (0.0, math.pi, -math.pi, math.pi / 2, -math.pi / 2)        # (0.0 == -0.0: the sign bit is compared separately)


def heading_of(dx, dy, dist):
    """FastSlam.py:90-93 / :114-117."""
    return math.acos(dx / dist) if dy > 0 else -math.acos(dx / dist)


def _post_cases():
    rs = np.random.RandomState(SEED)
    rows = []

    def add(kind, prev, fine_xy, logc=None, direct_only=False, lattice=False):
        theta = float(rs.uniform(-400.0, 400.0))
        coarse = (fine_xy[0] + 0.1 * rs.randint(-2, 3), fine_xy[1] + 0.1 * rs.randint(-2, 3), theta + 0.01 * rs.randint(-5, 6))
        lc = float(rs.uniform(-300.0, 5.0)) if logc is None else logc
        rows.append(SimpleNamespace(kind=kind, prev=(float(prev[0]), float(prev[1])), fine=(float(fine_xy[0]), float(fine_xy[1]), theta),
                                    coarse=(float(coarse[0]), float(coarse[1]), float(coarse[2]), math.exp(lc) if lc == lc else lc, lc),
                                    direct_only=direct_only, lattice=lattice))

    add("zero", (1.7, -2.3), (1.7, -2.3))
    add("zero-negzero", (-0.0, 0.0), (0.0, -0.0))
    add("underflow", (0.0, 0.0), (1e-170, -1e-170))
    add("axis+x", (1.25, -0.75), (1.75, -0.75))
    add("axis-x", (1.25, -0.75), (0.5, -0.75))
    add("axis+y", (1.25, -0.75), (1.25, 2.0))
    add("axis-y", (1.25, -0.75), (1.25, -3.0))
    for sx in (1.0, -1.0):
        for sy in (1e-12, -1e-12):
            add("ratio", (0.0, 0.0), (sx, sy))
    for unit in LATTICE_UNITS:
        for origin in ((0.0, 0.0), (807 * 0.05, -797 * 0.05)):             # the second: ~40 m, where fine - prev is no exact multiple
            for i in range(-LATTICE_SPAN, LATTICE_SPAN + 1):
                for j in range(-LATTICE_SPAN, LATTICE_SPAN + 1):
                    add(f"lattice-{unit:g}", origin, (origin[0] + i * unit, origin[1] + j * unit), lattice=True)
    for _ in range(N_RANDOM):
        mag, phi = 10.0 ** rs.uniform(-9.0, 3.0), rs.uniform(-math.pi, math.pi)
        prev = rs.uniform(-50.0, 50.0, 2)
        add("random", prev, (prev[0] + mag * math.cos(phi), prev[1] + mag * math.sin(phi)))
    add("far", (1e6 + 0.3, -1e6 + 0.7), (1e6 + 0.4, -1e6 + 0.75))
    add("far", (1e6 + 0.3, -1e6 + 0.7), (1e6 + 0.28, -1e6 + 0.7))
    # (a NaN heading prior produces a NaN log-confidence; both make the commit's normaliser output NaN: direct calls only)
    add("logc-nan", (0.5, 0.5), (0.6, 0.4), logc=float("nan"), direct_only=True)
    add("logc-neginf", (0.5, 0.5), (0.4, 0.6), logc=-math.inf, direct_only=True)
    return rows


def _prior_cases():
    rs = np.random.RandomState(SEED + 1)
    rows = []

    def add(kind, prev_pose, heading, raw_theta, prev_raw_theta, turn=None, step=0.5, prev_raw_heading="from-turn"):
        """turn: the raw turn aimed at (None: no previous raw heading, has_turn = 0)."""
        px, py = rs.uniform(-20.0, 20.0, 2)
        phi = rs.uniform(-math.pi, math.pi)
        rx, ry = px + step * math.cos(phi), py + step * math.sin(phi)
        dx, dy = rx - px, ry - py
        dist = math.sqrt(dx ** 2 + dy ** 2)
        if prev_raw_heading == "from-turn":
            prev_raw_heading = math.nan if turn is None else heading_of(dx, dy, dist) - turn
        rows.append(SimpleNamespace(kind=kind, prev_pose=tuple(float(v) for v in prev_pose), heading=float(heading),
                                    raw=(float(rx), float(ry), float(raw_theta)), prev_raw=(float(px), float(py), float(prev_raw_theta)),
                                    prev_raw_heading=float(prev_raw_heading)))

    def pose():
        return (rs.uniform(-30.0, 30.0), rs.uniform(-30.0, 30.0), rs.uniform(-math.pi, math.pi))

    add("no-turn-first", pose(), 0.7, 0.3, 0.1, turn=None)                                   # no previous raw heading
    add("no-turn-short", pose(), -2.1, 0.3, 0.1, step=0.2, prev_raw_heading=1.0)                # raw step below 0.3 m
    add("no-turn-short-nan", pose(), math.nan, 0.3, 0.1, step=0.2, prev_raw_heading=1.0)
    add("nan-heading-first", pose(), math.nan, 0.3, 0.1, turn=None)
    add("nan-heading-turn", pose(), math.nan, 0.3, 0.1, turn=0.25)                            # the reference raises TypeError
    add("nan-heading-turn0", pose(), math.nan, -1.0, 2.0, turn=0.0)
    headings = [-math.pi, -math.pi / 2, -0.0, 0.0, 5e-324, 1e-300, math.pi / 2, math.pi] + list(rs.uniform(-math.pi, math.pi, 8))
    turns = [-2 * math.pi, -math.pi, -1.0, 0.0, 1e-9, math.pi / 2, math.pi, 2 * math.pi] + list(rs.uniform(-2 * math.pi, 2 * math.pi, 4))
    for h in headings:
        for t in turns:
            add("turn", pose(), h, rs.uniform(-math.pi, math.pi), rs.uniform(-math.pi, math.pi), turn=t)
    # the association of the estimate theta: (1e-17 + 1.0) - 1.0 = 0.0, 1e-17 + (1.0 - 1.0) = 1e-17
    add("association", (0.5, 0.5, 1e-17), 0.3, 1.0, 1.0, turn=0.5)
    add("association", (0.5, 0.5, -1e-17), 0.3, -1.0, -1.0, turn=None)
    add("association", (0.5, 0.5, 1.0), 0.3, 1e16, 1e16 + 2.0, turn=0.5)
    for _ in range(12):                                                                        # thetas up to 400 rad
        x, y, _ = pose()
        add("wound-up", (x, y, rs.uniform(-400.0, 400.0)), rs.uniform(-math.pi, math.pi), rs.uniform(-400.0, 400.0), rs.uniform(-400.0, 400.0),
            turn=rs.uniform(-2 * math.pi, 2 * math.pi))
    add("negzero-xy", (-0.0, -0.0, 0.25), 0.3, 0.2, 0.1, turn=0.5)
    add("negzero-xy", (-0.0, 0.0, -0.0), -0.0, 0.0, 0.0, turn=0.0)
    add("negzero-xy", (0.0, -0.0, -0.0), math.nan, -0.0, 0.0, turn=None)
    return rows


POST = _post_cases()
PRIOR = _prior_cases()


def post_arrays():
    """(prev [N, 2], fine [N, 3], coarse [N, 5], direct_only [N], lattice [N])"""
    return (np.array([c.prev for c in POST]), np.array([c.fine for c in POST]), np.array([c.coarse for c in POST]),
            np.array([c.direct_only for c in POST]), np.array([c.lattice for c in POST]))


def prior_arrays():
    """(prev_pose [M, 3], heading [M], raw [M, 3], prev_raw [M, 3], prev_raw_heading [M]); NaN: None"""
    return (np.array([c.prev_pose for c in PRIOR]), np.array([c.heading for c in PRIOR]), np.array([c.raw for c in PRIOR]),
            np.array([c.prev_raw for c in PRIOR]), np.array([c.prev_raw_heading for c in PRIOR]))


def none_if_nan(v):
    return None if math.isnan(v) else float(v)


def reading(xyt, ranges=()):
    return {"x": float(xyt[0]), "y": float(xyt[1]), "theta": float(xyt[2]), "range": ranges}


def raw_odometry(c):
    """(dist, raw heading or None, has_turn, raw_turn) of a prior case, as FastSlam.py:81-100 arrives at them (what the host hands
    to slam2d_prior)."""
    dx, dy = c.raw[0] - c.prev_raw[0], c.raw[1] - c.prev_raw[1]
    dist = math.sqrt(dx ** 2 + dy ** 2)
    if not dist > 0.3:
        return dist, None, 0, 0.0
    rh = heading_of(dx, dy, dist)
    if math.isnan(c.prev_raw_heading):
        return dist, rh, 0, 0.0
    return dist, rh, 1, rh - c.prev_raw_heading
