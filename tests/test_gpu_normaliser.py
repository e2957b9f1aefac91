"""The weight normaliser at its edges, on every path that holds a copy of it (csrc/slam2d.hip):

  (a) k_weights                                      slam2d_weights_normalize
  (b) k_weights_local + k_weights_merge              slam2d_weights_local / slam2d_weights_merge per shard
  (c) ... the merge that publishes                   slam2d_weights_merge_publish with a zeroed sync block
  (4) weights_local_body + normaliser_arrive         one grouped step of a ParticleFilter (slam2d_groups_commit)

against ONE plain reference in numpy.longdouble with exact (Shewchuk) summation: s = logw + logc,
w = exp(s - max s) / sum exp(s - max s), logw' = s - lse, var = sum (w - 1/N)^2.  -inf entries are weight 0 as long as one
entry is finite; a NaN entry, or -inf everywhere (the reference's 0/0), makes everything NaN on every path, shard and rank --
ParticleFilter.normalizeWeights raises after looking at its own rank's weights only.

Tolerances are those of test_weights_kernel / test_sharded_weights_kernels (the project's own figures).  One addition, for the
*dominant* family only: there max s = 0 and lse = log(sum) = log(1 + (N-1) eps) is ~N eps, while a sum of N terms in doubles is
only good to N 2^-53 relative to the sum (<= 2 here) -- so the log of the sum gets atol = 2 N 2^-53 beside its rtol of 1e-13
(everywhere else lse is tens to thousands and the rtol alone holds).
"""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import slam_oracle as so

pytestmark = pytest.mark.gpu
flt = importlib.import_module("slam-2d-lidar-scan_amd.filter")
par = importlib.import_module("slam-2d-lidar-scan_amd.parallel")

LD = np.longdouble
W_RTOL, ELW_RTOL, VAR_RTOL, VAR_ATOL, LSE_RTOL = 1e-12, 1e-10, 1e-9, 1e-15, 1e-13
SIZES = (1, 2, 255, 256, 257, 512, 513, 1000)
WORLDS = (1, 2, 3, 8)
EPS = (1e-8, 1e-14, 1e-18, 1e-25, 1e-300)


@pytest.fixture(scope="module")
def pkg():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def _fsum(values):
    """math.fsum's algorithm (Shewchuk's non-overlapping partials: no bit of any term is lost) carried in longdouble."""
    partials = []
    for x in values:
        i = 0
        for y in partials:
            if abs(x) < abs(y):
                x, y = y, x
            hi = x + y
            lo = y - (hi - x)
            if lo:
                partials[i] = lo
                i += 1
            x = hi
        partials[i:] = [x]
    return sum(partials, LD(0))


def reference(s):
    """(w, logw', var, lse) of the float64 sums s, evaluated in longdouble and rounded to float64 at the end."""
    s = np.asarray(s, dtype=np.float64)
    n = s.size
    if np.isnan(s).any() or not np.isfinite(s).any():
        return SimpleNamespace(w=np.full(n, np.nan), logw=np.full(n, np.nan), var=np.nan, lse=np.nan, nan=True)
    x = s.astype(LD)
    m = x.max()
    e = np.exp(x - m)
    total = _fsum(e)
    w = e / total
    lse = m + np.log(total)
    var = _fsum((w - LD(1) / LD(n)) ** 2)
    return SimpleNamespace(w=w.astype(np.float64), logw=(x - lse).astype(np.float64), var=float(var), lse=float(lse), nan=False)


def check(got_w, got_logw, got_stats, ref, sl, case, where):
    """One shard's (or the whole filter's) output against ref[sl]."""
    msg = f"{case.name} {where}"
    if ref.nan:
        assert np.isnan(got_w).all() and np.isnan(got_logw).all() and np.isnan(got_stats).all(), (msg, got_w, got_logw, got_stats)
        return
    w, lw = ref.w[sl], ref.logw[sl]
    # rtol alone: where the reference's weight is 0 (a -inf entry, an exp below the smallest double) the kernel's is exactly 0
    np.testing.assert_allclose(got_w, w, rtol=W_RTOL, atol=0, err_msg=msg)
    assert np.array_equal(got_logw == -np.inf, lw == -np.inf) and not np.isnan(got_logw).any(), msg
    np.testing.assert_allclose(np.exp(got_logw), w, rtol=ELW_RTOL, atol=0, err_msg=msg)
    np.testing.assert_allclose(got_stats[1], ref.lse, rtol=LSE_RTOL, atol=case.lse_atol, err_msg=msg)
    # logw' = fl(s - lse) itself (exp(logw') says nothing where it underflows): within the bar of lse above plus the subtraction's rounding
    fin = lw != -np.inf
    bound = LSE_RTOL * abs(ref.lse) + case.lse_atol + np.abs(lw[fin]) * 2.0 ** -52
    assert (np.abs(got_logw[fin] - lw[fin]) <= bound).all(), (msg, got_logw[fin] - lw[fin], bound)
    # (with equal weights the true variance is 0 and the merges' s2/s1^2 - 1/N may land a few 1e-17 BELOW zero: that is inside the
    # atol and harmless -- the resample trigger sits near (N-1)/N -- so do not "fix" it by clamping; anything below -atol fails here)
    np.testing.assert_allclose(got_stats[0], ref.var, rtol=VAR_RTOL, atol=VAR_ATOL, err_msg=msg)


# ------------------------------------------------------------------------------------------------
# the case table (written once; every case runs on paths a, b and c)
# ------------------------------------------------------------------------------------------------
def _ranges(n):
    """parallel.shard_range's ragged splits of n over every world size that leaves no rank empty."""
    return [[par.shard_range(n, world, r)[1] for r in range(world)] for world in WORLDS if world <= n]


def _spread(rs, n, quantum=None):
    logw, logc = rs.uniform(-300, -5, n), rs.uniform(-200, 1, (n, 3))
    if quantum:                     # multiples of 2^-20: shifting them by 1e4 and adding them is exact in doubles
        logw, logc = np.round(logw / quantum) * quantum, np.round(logc / quantum) * quantum
    return logw, logc


def _case(name, logw, logc1, splits, lse_atol=0.0, rs=None):
    """logc1: the log-confidences proper; they travel as column 1 of a [n, 3] array (stride 3, like the engine's match records)."""
    n = len(logw)
    logc = (rs or np.random.RandomState(n)).uniform(-200, 1, (n, 3))
    logc[:, 1] = logc1
    assert all(sum(sp) == n and min(sp) >= 1 for sp in splits), name
    return SimpleNamespace(name=name, logw=np.asarray(logw, dtype=np.float64), logc=logc, splits=splits, lse_atol=lse_atol)


def _build_cases():
    cases = []
    rs = np.random.RandomState(2024)
    for n in SIZES:                                                     # spread: the two older tests' distribution at the new sizes
        logw, logc = _spread(rs, n)
        extra = {1000: [[600, 400], [1, 299, 700], [999, 1]], 513: [[512, 1], [257, 256]]}.get(n, [])
        cases.append(_case(f"spread-{n}", logw, logc[:, 1], _ranges(n) + extra))
    for n in SIZES:                                                     # equal: every s the same number, exactly
        logw = rs.randint(-300, -5, n).astype(np.float64)
        cases.append(_case(f"equal-{n}", logw, -40.25 - logw, _ranges(n) + ([[600, 400]] if n == 1000 else [])))
    for n, places in ((2, ("first", "last")), (513, ("first", "last", "at256"))):       # dominant: one entry 0, the rest log eps
        for place in places:
            at = {"first": 0, "last": n - 1, "at256": 256}[place]
            for tag, small in [(f"{e:g}", np.log(e)) for e in EPS] + [("underflow", -800.0)]:
                s = np.full(n, small)
                s[at] = 0.0
                logw = rs.uniform(-50, 50, n)
                # (index 256 sits in the second trip of every i += 256 loop: [300, 213] keeps it in one shard of more than 256)
                cases.append(_case(f"dominant-{tag}-{n}-{place}", logw, s - logw, _ranges(n) + ([[300, 213]] if n == 513 else []),
                                   lse_atol=2 * n * 2.0 ** -53))
    for n in (257, 1000):                                               # offset: spread shifted by -1e4 / +1e4, exactly
        logw, logc = _spread(rs, n, quantum=2.0 ** -20)
        base = reference(logw + logc[:, 1])
        for tag, shift in (("minus", -1e4), ("plus", 1e4)):
            c = _case(f"offset-{tag}-{n}", logw + shift, logc[:, 1], _ranges(n))
            assert np.array_equal(c.logw + c.logc[:, 1], logw + logc[:, 1] + shift)
            assert np.array_equal(reference(c.logw + c.logc[:, 1]).w, base.w)      # the weights do not know about the shift
            cases.append(c)
    for n in (257, 1000):                                               # -inf, scattered (through either summand)
        logw, logc = _spread(rs, n)
        hit = rs.choice(n, n // 10, replace=False)
        logw[hit[::2]] = -np.inf
        logc[hit[1::2], 1] = -np.inf
        cases.append(_case(f"neginf-scattered-{n}", logw, logc[:, 1], _ranges(n)))
    # -inf, whole shards: (split, the shards that are -inf throughout)
    whole = [("first-1", [1, 40], [0]), ("last-7", [30, 7], [1]), ("first-300", [300, 300, 50], [0]), ("last-300", [50, 300], [1]),
             ("middle-7", [64, 7, 64], [1]), ("two-of-three-a", [7, 64, 300], [0, 2]), ("two-of-three-b", [1, 7, 5], [0, 1]),
             ("rank3-of-8", [par.shard_range(1000, 8, r)[1] for r in range(8)], [3])]
    for tag, split, dead in whole:
        n = sum(split)
        logw, logc = _spread(rs, n)
        first = np.concatenate(([0], np.cumsum(split)))
        for k, r in enumerate(dead):
            (logw if k % 2 == 0 else logc[:, 1])[first[r]:first[r + 1]] = -np.inf
        cases.append(_case(f"neginf-shard-{tag}", logw, logc[:, 1], [split]))
    # NaN: one NaN log-confidence -- first, last, in a shard of its own (also where that shard is otherwise ... nothing: fmax drops it)
    for tag, n, at, splits in (("first", 513, 0, _ranges(513)), ("last", 513, 512, _ranges(513)), ("own-shard", 513, 256, [[256, 1, 256]]),
                               ("own-shard-first", 13, 0, [[1, 12]]), ("own-shard-last", 301, 300, [[300, 1]])):
        logw, logc = _spread(rs, n)
        logc[at, 1] = np.nan
        cases.append(_case(f"nan-{tag}", logw, logc[:, 1], splits))
    for n in (1, 7, 513):                                               # -inf everywhere: NaN, as the reference's 0/0
        logw, logc = _spread(rs, n)
        logw[::2] = -np.inf
        logc[1::2, 1] = -np.inf
        cases.append(_case(f"all-neginf-{n}", logw, logc[:, 1], _ranges(n)))
    return cases


CASES = _build_cases()
_REF = {}


def _ref(case):
    if case.name not in _REF:
        _REF[case.name] = reference(case.logw + case.logc[:, 1])
    return _REF[case.name]


def test_the_table_holds_what_it_should():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {len(c.logw) for c in CASES if c.name.startswith("spread")} == set(SIZES)
    assert any(max(sp) > 256 for c in CASES for sp in c.splits) and any(min(sp) == 1 and len(sp) > 1 for c in CASES for sp in c.splits)
    for c in CASES:
        nan = _ref(c).nan
        assert nan == c.name.startswith(("nan-", "all-neginf")), c.name
        if c.name.startswith("neginf"):
            assert (_ref(c).w == 0).any() and np.isclose(_ref(c).w.sum(), 1.0)
        if c.name.startswith("dominant"):
            assert np.isfinite(_ref(c).logw).all() and (_ref(c).w.max() > 0.99)
    assert (_ref(next(c for c in CASES if c.name == "dominant-underflow-513-at256")).w == 0).sum() == 512


# ------------------------------------------------------------------------------------------------
# paths a, b, c through the C ABI
# ------------------------------------------------------------------------------------------------
def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _local_and_merge(L, s_or_logw, logc, split, total, publish):
    """slam2d_weights_local per shard, then a merge per shard over all partials: [(w, logw', stats, sync words or None)] per shard."""
    import torch
    world = len(split)
    first = np.concatenate(([0], np.cumsum(split)))
    d_lw = [_cuda(s_or_logw[first[r]:first[r + 1]].copy()) for r in range(world)]
    d_lc = [None if logc is None else _cuda(logc[first[r]:first[r + 1]]) for r in range(world)]
    parts = torch.zeros(3 * world, dtype=torch.float64, device="cuda")
    for r in range(world):
        flt._lib.check(L.slam2d_weights_local(flt._ptr(d_lw[r]), None if logc is None else d_lc[r].data_ptr() + 8, 3, split[r],
                                              parts.data_ptr() + 24 * r, flt._stream()), "local")
    out = []
    for r in range(world):
        d_w = torch.zeros(split[r], dtype=torch.float64, device="cuda")
        d_s = torch.zeros(2, dtype=torch.float64, device="cuda")
        sync = None
        if publish:
            sync = torch.zeros(64, dtype=torch.int32, device="cuda")
            flt._lib.check(L.slam2d_weights_merge_publish(flt._ptr(d_lw[r]), split[r], flt._ptr(parts), world, total, flt._ptr(d_w),
                                                          flt._ptr(d_s), flt._ptr(sync), flt._stream()), "merge_publish")
        else:
            flt._lib.check(L.slam2d_weights_merge(flt._ptr(d_lw[r]), split[r], flt._ptr(parts), world, total, flt._ptr(d_w),
                                                  flt._ptr(d_s), flt._stream()), "merge")
        out.append((d_w.cpu().numpy(), d_lw[r].cpu().numpy(), d_s.cpu().numpy(), None if sync is None else sync.cpu().numpy()))
    return out, parts.cpu().numpy().reshape(world, 3)


@pytest.mark.parametrize("path", ["a", "b", "c"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_normaliser_paths(pkg, case, path):
    """Every case of the table on slam2d_weights_normalize (a), slam2d_weights_local + slam2d_weights_merge over every split of
    the case (b) and slam2d_weights_local + slam2d_weights_merge_publish (c): each shard of each split gets the reference's
    weights, log-weights, variance and log of the sum of ALL particles -- what path (a) returns for the concatenated input --
    and (c) advances word 1 of its sync block by exactly one and touches no other word."""
    import torch
    L = flt._lib.lib()
    ref, n = _ref(case), len(case.logw)
    if path == "a":
        d_lw, d_lc = _cuda(case.logw.copy()), _cuda(case.logc)
        d_w = torch.zeros(n, dtype=torch.float64, device="cuda")
        d_s = torch.zeros(2, dtype=torch.float64, device="cuda")
        flt._lib.check(L.slam2d_weights_normalize(flt._ptr(d_lw), d_lc.data_ptr() + 8, 3, n, flt._ptr(d_w), flt._ptr(d_s), flt._stream()),
                       "weights")
        check(d_w.cpu().numpy(), d_lw.cpu().numpy(), d_s.cpu().numpy(), ref, slice(0, n), case, "path a")
        return
    for split in case.splits:
        out, _ = _local_and_merge(L, case.logw, case.logc, split, n, publish=(path == "c"))
        first = np.concatenate(([0], np.cumsum(split)))
        for r, (w, lw, stats, sync) in enumerate(out):
            check(w, lw, stats, ref, slice(first[r], first[r + 1]), case, f"path {path} split {split} shard {r}")
            if sync is not None:
                want = np.zeros(64, dtype=np.int32)
                want[1] = 1
                assert np.array_equal(sync, want), (case.name, split, r, sync[:4])


# ------------------------------------------------------------------------------------------------
# path 4: the merge inside the groups' update launches (normaliser_arrive), through one grouped step of a filter
# ------------------------------------------------------------------------------------------------
# BASELINE config 2 (test_gpu_parity.BNB_CASES' smallest map): one level, 41 x 41 x 36 cube, 180 beams
CFG = dict(unit=0.1, max_range=34.5, fov=np.pi, beams=180, map_m=100.0, search_radius=2.05, half_rad=0.30, sigma_cells=2, miss=0.15,
           coarse_factor=1, wall=0.5)
# (particles, groups asked for, groups formed).  ParticleFilter forms EQUAL groups only (P % groups == 0, else one group, which still
# goes through the grouped calls): there is no ragged group to test on this path -- ragged shards are what paths b and c above are
# for -- so 9 particles run in three groups and, asked for two, in one: the merge over a single partial.
GROUPINGS = [(8, 2, 2), (8, 4, 4), (9, 3, 3), (9, 2, 1)]
_SCENE = {}


def _scene():
    if not _SCENE:
        synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
        unit, size_m = CFG["unit"], CFG["map_m"]
        origin = (-size_m / 2, -size_m / 2)
        world = synth.make_world(size_m, unit, seed=0, n_boxes=60)
        poses = synth.random_walk(world, unit, origin, 2, seed=3, step=0.4, max_radius=6.0)
        _SCENE["counts"] = synth.counts_from_world(world)
        _SCENE["readings"] = [{"x": float(p[0]), "y": float(p[1]), "theta": float(p[2]),
                               "range": list(map(float, synth.raycast(world, unit, origin, p, CFG["fov"], CFG["beams"], CFG["max_range"])))}
                              for p in poses]
    return _SCENE


def _grouped_step(pkg, P, groups, logw_set, expect_raise=False):
    """A fresh synthetic filter (test_gpu_parity._synthetic_filter's few lines, with groups); scan 1 through the plain calls, then
    the log-weights are overwritten and scan 2 is ONE grouped step.  Returns what that step left: the pack the device pushed to the
    host (report, weights, statistics) and the log-weights written back."""
    import torch
    cfg, sc = CFG, _scene()
    ogP = [cfg["map_m"], cfg["map_m"], {"x": 0.0, "y": 0.0}, cfg["unit"], cfg["fov"], cfg["max_range"], cfg["beams"], cfg["wall"]]
    smP = [cfg["search_radius"], cfg["half_rad"], cfg["sigma_cells"], 0.1, 0.25, 0.3, cfg["miss"], cfg["coarse_factor"]]
    pf = pkg.ParticleFilter(P, ogP, smP, growable=False, rng=np.random.RandomState(0), groups=groups)
    assert pf.lazy_field
    pf.engine.maps[0].upload(*sc["counts"])
    for m in pf.engine.maps[1:]:
        m.cells.copy_(pf.engine.maps[0].cells)
        m.bits_valid = False
    got = {}

    def on_scan(count, f, unb):
        if count == 1 and logw_set is not None:
            f.d_logw.copy_(torch.from_numpy(logw_set))
        if count == 2:
            got.update(pack=f._h_pack.numpy().copy(), logw=f.d_logw.cpu().numpy())

    if expect_raise:
        with pytest.raises(flt._lib.Slam2dError, match="NaN"):
            pf.run(sc["readings"], on_scan=on_scan)
        torch.cuda.synchronize()
        got.update(pack=pf._h_pack.numpy().copy(), logw=pf.d_logw.cpu().numpy())
    else:
        pf.run(sc["readings"], on_scan=on_scan)
    assert pf._grp is not None and pf._grp.devsync and pf.stats["step_by_step"] == 1 and pf.stats["redo"] == 0, pf.stats
    pack = got["pack"]
    flags = pack[6 * P + 2:].view(np.uint32)[:P]
    assert not (flags & (flt._lib.FATAL_FLAGS | flt._lib.F_SCAN_VOIDED)).any(), flags
    return SimpleNamespace(pf=pf, logc=pack[:5 * P].reshape(P, 5)[:, 4].copy(), w=pack[5 * P:6 * P].copy(), stats=pack[6 * P:6 * P + 2].copy(),
                           logw=got["logw"])


_DRY = {}


def _scan_logc(pkg, P):
    """The scan's own log-confidences for P particles (fresh filters are identical: same maps, same seeded uniforms), from one dry step
    -- so that a case can aim logw + logc at the family it wants.  Whatever the step then reports is what the reference is fed."""
    if P not in _DRY:
        _DRY[P] = _grouped_step(pkg, P, 1, None).logc
    return _DRY[P]


def _grouped_targets(P, G):
    """name -> (target s [P], lse_atol, ends in NaN)"""
    rs = np.random.RandomState(100 * P + G)
    spread = rs.uniform(-300, -5, P) + rs.uniform(-200, 1, P)
    per, out = P // G, {}
    out["spread"] = (spread, 0.0, False)
    out["equal"] = (np.full(P, -40.25), 0.0, False)
    out["offset-minus"] = (spread - 1e4, 0.0, False)
    out["offset-plus"] = (spread + 1e4, 0.0, False)
    for tag, small in (("1e-18", np.log(1e-18)), ("1e-300", np.log(1e-300)), ("underflow", -800.0)):
        s = np.full(P, small)
        s[P - 1] = 0.0                                                  # the dominant particle sits in the LAST group
        out[f"dominant-{tag}"] = (s, 2 * P * 2.0 ** -53, False)
    scattered = spread.copy()
    scattered[[1, P - 2]] = -np.inf
    out["neginf-scattered"] = (scattered, 0.0, False)
    if G > 1:                                                           # (one group that is -inf throughout is the all-neginf case)
        for tag, g in (("first", 0), ("last", G - 1)):
            s = spread.copy()
            s[g * per:(g + 1) * per] = -np.inf
            out[f"neginf-group-{tag}"] = (s, 0.0, False)
    nan = spread.copy()
    nan[P // 2] = np.nan
    out["nan"] = (nan, 0.0, True)
    out["all-neginf"] = (np.full(P, -np.inf), 0.0, True)
    return out


GROUPED_FAMILIES = ["spread", "equal", "offset-minus", "offset-plus", "dominant-1e-18", "dominant-1e-300", "dominant-underflow",
                    "neginf-scattered", "neginf-group-first", "neginf-group-last", "nan", "all-neginf"]


@pytest.mark.parametrize("family", GROUPED_FAMILIES)
@pytest.mark.parametrize("P,asked,G", GROUPINGS, ids=[f"P{p}-G{g}" for p, _, g in GROUPINGS])
def test_grouped_step_merges_like_the_sharded_kernels(pkg, P, asked, G, family):
    """The on-device merge over particle groups (normaliser_arrive, every grouped step).  The log-weights are overwritten before one
    scan; expected are the reference applied to logw_set + report[:, 4] (the scan's own log-confidences, which the step
    downloads): weights, written-back log-weights, variance and log of the sum from the pack -- and the SAME BITS as
    slam2d_weights_local + slam2d_weights_merge_publish over the same numbers with shards equal to the groups, as the kernel's comment
    promises.  A NaN (or nothing but -inf) among the log-weights sets no fault bit -- the match and the update do not read them, the
    step's fault words are checked clean -- so those cases run here too: every weight and both statistics NaN, and run() raises."""
    targets = _grouped_targets(P, G)
    if family not in targets:
        assert G == 1 and family.startswith("neginf-group")
        return                                                          # (one group: that is "all-neginf", which runs)
    target, lse_atol, ends_nan = targets[family]
    logw_set = target - _scan_logc(pkg, P)                               # (-inf and NaN pass through)
    res = _grouped_step(pkg, P, asked, logw_set, expect_raise=ends_nan)
    assert res.pf.n_groups == G
    s = logw_set + res.logc                                             # the device's own addition (post_match_one), in doubles
    assert np.array_equal(np.isnan(s), np.isnan(target)) and np.array_equal(s == -np.inf, target == -np.inf)
    case = SimpleNamespace(name=f"grouped-{family}-P{P}-G{G}", lse_atol=lse_atol)
    ref = reference(s)
    assert ref.nan == ends_nan
    # the same numbers through paths b + c, shards = groups: bit for bit (first: a merge that differs from k_weights_merge shows here)
    out, _ = _local_and_merge(flt._lib.lib(), s, None, [P // G] * G, P, publish=True)
    w_bc = np.concatenate([o[0] for o in out])
    lw_bc = np.concatenate([o[1] for o in out])
    if ends_nan:
        assert np.isnan(w_bc).all() and np.isnan(lw_bc).all() and all(np.isnan(o[2]).all() for o in out)
    else:
        assert np.array_equal(res.w.view(np.uint64), w_bc.view(np.uint64)), (res.w, w_bc)
        assert np.array_equal(res.logw.view(np.uint64), lw_bc.view(np.uint64)), (res.logw, lw_bc)
        for o in out:
            assert np.array_equal(res.stats.view(np.uint64), o[2].view(np.uint64)), (res.stats, o[2])
    check(res.w, res.logw, res.stats, ref, slice(0, P), case, "path 4")


# ------------------------------------------------------------------------------------------------
# the resample decision
# ------------------------------------------------------------------------------------------------
LADDER = [(k, m) for k in list(range(8, 15)) + list(range(18, 26)) for m in (1, 3)]


def _decision_from_device_weights(w):
    """ParticleFilter.weightUnbalanced over device weights as a scan's pack delivers them: normalizeWeights' host half
    (_sequential_variance) and the trigger expression, on a filter object that is nothing but those weights."""
    import torch
    n = len(w)
    pf = object.__new__(flt.ParticleFilter)
    pf.total_particles = pf.numParticles = n
    pf.sharded, pf.step, pf._normalized_step = False, 0, 0
    pack = np.zeros(6 * n + 2)
    pack[5 * n:6 * n] = w
    pf._h_pack = torch.from_numpy(pack)
    return bool(pf.weightUnbalanced())


def _oracle_decision(weights):
    po = object.__new__(so.ParticleFilterOracle)
    po.numParticles = len(weights)
    po.particles = [SimpleNamespace(weight=float(v)) for v in weights]
    return bool(po.weightUnbalanced())


@pytest.mark.parametrize("path", ["a", "b"])
@pytest.mark.parametrize("place", ["first", "last"])
@pytest.mark.parametrize("n", [2, 6, 64])
def test_resample_decision_matches_the_oracle(pkg, n, place, path):
    """One particle at weight 0.37, the rest at 0.37 eps, eps = 1e-k and 3e-k for k in 8..14 and 18..25: the filter's decision from
    the device's weights equals oracle.ParticleFilterOracle.weightUnbalanced on the same weights in the linear domain at EVERY step
    (k in 15..17 is left out on purpose: filter.py, beside _DEGENERACY_BAND).  The ladder does cross the trigger: it fires from
    k = 18 on at N = 2 and 6 and never at N = 64."""
    import torch
    L = flt._lib.lib()
    wrong, fired = [], 0
    for k, m in LADDER:
        weights = np.full(n, 0.37 * m * 10.0 ** -k)
        weights[0 if place == "first" else n - 1] = 0.37
        logw = np.log(weights)
        if path == "a":
            d_lw = _cuda(logw.copy())
            d_w = torch.zeros(n, dtype=torch.float64, device="cuda")
            d_s = torch.zeros(2, dtype=torch.float64, device="cuda")
            flt._lib.check(L.slam2d_weights_normalize(flt._ptr(d_lw), None, 1, n, flt._ptr(d_w), flt._ptr(d_s), flt._stream()), "weights")
            w = d_w.cpu().numpy()
        else:
            world = 2 if n == 2 else 3                                  # (64 over 3 ranks: ragged)
            out, _ = _local_and_merge(L, logw, None, [par.shard_range(n, world, r)[1] for r in range(world)], n, publish=False)
            w = np.concatenate([o[0] for o in out])
        got, want = _decision_from_device_weights(w), _oracle_decision(weights)
        fired += want
        if got != want:
            wrong.append((k, m, got, want))
    assert not wrong, wrong
    assert fired == (0 if n == 64 else 16)
