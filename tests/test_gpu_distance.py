"""slam2d_field_build_distance on the MI355X against its definition in NumPy (tests/distance_yardstick.py): every comparison is
np.array_equal.  The yardstick reads the DEVICE's occupied image (the bytes equal to the generation stamp) and frame record, so
what is compared is the distance transform and the table, nothing of the front end the call shares with slam2d_field_build --
that part is compared with a twin level's full build.  World, lidar and level of tests/test_gpu_score.py: unit 0.1 m, the 289 x
289 covering field of a window of half-edge 8 m, fmax 290, fpitch 304."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import distance_yardstick as dyard
import lattice_yardstick as lyard
import mcl_yardstick as mcl
import test_gpu_field_slots as tfs
import test_gpu_mcl as tmcl
import test_gpu_score as tscore
import test_gpu_search as tsearch
from test_score_host import BEAMS, FOV, INIT, R, SIZE, UNIT, WALL, walk

pytestmark = pytest.mark.gpu

_lib = importlib.import_module("slam-2d-lidar-scan_amd._lib")

SMP = tscore.SMP
WINDOW = (0.0, 0.0, 8.0)
FMAX, FPITCH = 290, 304
LIK = dict(sigma=0.2)                                          # likelihood_table(0.1, 0.2): about 210 entries, R = 15
IDENTITY = np.arange(65536, dtype=np.uint32)                   # R = 256, wider than half the image: the cap never bites inside
SHORT = {1: [5], 2: [5, 9], 3: [0, 3, 7], 4: [1, 2, 3, 1000]}    # tables of one to four entries
FREE, WALLS = (1.0, 5.0), (7.0, 8.0)                           # (visited, total) of a free and of an occupied map cell


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return importlib.import_module("slam-2d-lidar-scan_amd")


@pytest.fixture(scope="module")
def engine():
    return importlib.import_module("slam-2d-lidar-scan_amd.engine")


def table_of(which, engine):
    if which == "likelihood":
        return engine.likelihood_table(UNIT, 0.2)[0]
    if which == "identity":
        return IDENTITY
    return np.array(SHORT[which], dtype=np.uint32)


def new_grid(pkg, world=None):
    """The grid of tests/test_gpu_score.py, grown to hold the covering frame of WINDOW; its matcher and a covering level of its own."""
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    og = pkg.OccupancyGrid(SIZE, SIZE, INIT, UNIT, FOV, BEAMS, R, WALL)
    if world is not None:
        og.set_counts(*synth.counts_from_world(world))
    sm = pkg.ScanMatcher(og, *SMP)
    lv = sm.covering_level("fine", WINDOW[2], shared=False)
    og.checkAndExapndOG([WINDOW[0] - lv.reach, WINDOW[0] + lv.reach], [WINDOW[1] - lv.reach, WINDOW[1] + lv.reach])
    return og, sm, lv


@pytest.fixture(scope="module")
def scene(pkg):
    world, poses, scans = walk()
    og, sm, lv = new_grid(pkg, world)
    assert (lv.fmax, lv.fpitch, lv.P) == (FMAX, FPITCH, 1)
    eng = og.engine()
    return dict(og=og, sm=sm, lv=lv, eng=eng, world=world, poses=poses, scans=scans, centre=eng.to_device([[WINDOW[0], WINDOW[1]]]))


def device_occ(lv, p=0):
    """(occupied [fh, fw] bool, the raw bytes) of slot p as the last build left them: a byte is a wall iff it equals the stamp."""
    fr = lv.frames()[p]
    n = lv.P * lv.fmax * lv.fpitch
    raw = lv.t["occ"][:n].view(lv.P, lv.fmax, lv.fpitch)[p, :int(fr["fh"]), :int(fr["fw"])].cpu().numpy()
    return raw == (lv.c.occ_gen or 1), raw


def raw_call(eng, lvc, P, d_centre, lut, d2=None, d_maps=None, d_flags=None):
    """The call at the C ABI; the caller has brought the occupancy bits and the stamp in step."""
    import torch
    engine = importlib.import_module("slam-2d-lidar-scan_amd.engine")
    d_lut = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.uint32).view(np.int32).copy()).to(eng.device)
    _lib.check(eng.L.slam2d_field_build_distance(ctypes.byref(eng.lidar_c), ctypes.byref(lvc), d_maps or eng.d_maps.data_ptr(), P,
                                                 d_centre.data_ptr(), 2, d_lut.data_ptr(), len(lut), None if d2 is None else d2.data_ptr(),
                                                 d_flags or eng.flags.data_ptr(), engine._stream()), "slam2d_field_build_distance")
    torch.cuda.synchronize()


def check_slot(lv, p, lut, d2, what):
    """Slot p's field and squared distances against the yardstick on the device's own occupied image."""
    occ, _ = device_occ(lv, p)
    want = dyard.dist2(occ, len(lut) - 1)
    fh, fw = occ.shape
    got2 = d2[p, :fh, :fw].cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(got2, want), (what, "dist2", np.argwhere(got2 != want)[:6].tolist())
    field = lv.field_cost(p)
    assert field.dtype == np.uint32 and np.array_equal(field, np.asarray(lut, dtype=np.uint32)[want]), (what, "field")
    return occ, want


# ---- 1. the main case ----
@pytest.mark.parametrize("which", ["likelihood", "identity", 1, 2, 3, 4])
def test_main_case(scene, engine, which):
    import torch
    eng, lv = scene["eng"], scene["lv"]
    lut = table_of(which, engine)
    if which == "likelihood":
        assert 200 <= len(lut) <= 220 and dyard.reach(len(lut) - 1) == 15
    # both images pre-filled with 0xff bytes, a guard row behind each
    big = torch.full((FMAX + 1, FPITCH), -1, dtype=torch.int32, device=eng.device)
    d2 = torch.full((FMAX + 1, FPITCH), -1, dtype=torch.int32, device=eng.device)
    keep, keep_ptr = lv.t["field"], lv.c.field
    lv.t["field"], lv.c.field = big[:FMAX].view(1, FMAX, FPITCH), big.data_ptr()
    try:
        eng.refresh_bits()
        lv.next_generation()
        raw_call(eng, lv.c, 1, scene["centre"], lut, d2)
        assert not eng.take_flags(fatal=0xffffffff).any()
        occ, want = check_slot(lv, 0, lut, d2[:FMAX].view(1, FMAX, FPITCH), which)
    finally:
        lv.t["field"], lv.c.field = keep, keep_ptr
    assert occ.shape == (289, 289) and 1000 < occ.sum() < occ.size // 4          # walls and free space
    if which == "identity":
        assert want.max() < 65535 and want.max() > 15 * 15                        # the cap never bites inside; farther than R = 15 from a wall
    if which == "likelihood":
        assert (want == len(lut) - 1).any() and (want == 0).any()
    assert (big[FMAX] == -1).all() and (d2[FMAX] == -1).all(), "guard row"
    # without d_dist2: the same field
    eng.refresh_bits()
    lv.next_generation()
    raw_call(eng, lv.c, 1, scene["centre"], lut, None)
    assert np.array_equal(lv.field_cost(0), np.asarray(lut)[want])


# ---- 2. the same front end as the full build ----
@pytest.mark.parametrize("centre", [(0.0, 0.0), (0.29, -0.41), (9.0, -3.0)])
def test_same_front_end_as_the_full_build(scene, engine, centre):
    eng, sm, lv = scene["eng"], scene["sm"], scene["lv"]
    twin = sm.covering_level("fine", WINDOW[2], shared=False)
    d_c = eng.to_device([list(centre)])
    eng.flags.zero_()
    eng.field_build(twin, d_c, 2)
    bits_full = eng.flags.cpu().numpy().copy()
    eng.flags.zero_()
    d2 = eng.field_build_distance(lv, d_c, 2, engine.likelihood_table(UNIT, 0.2), dist2=True)
    bits = eng.flags.cpu().numpy().copy()
    eng.flags.zero_()
    outside = centre == (9.0, -3.0)                            # the grid holds the frame about (0, 0) and a few metres more
    front = _lib.F_WINDOW_OUTSIDE_MAP | _lib.F_FIELD_INDEX       # (the full build's blur may add its informational bit)
    assert bits[0] & ~front == 0 and bits[0] == bits_full[0] & front and bool(bits[0] & _lib.F_WINDOW_OUTSIDE_MAP) == outside
    a, b = lv.frames()[0], twin.frames()[0]
    for name in ("xlo", "ylo", "xhi", "yhi", "cx", "cy", "fh", "fw", "mx0", "mx1", "my0", "my1"):
        assert a[name] == b[name], name
    # the members a build measures are left as the frame kernel writes them: zero bounds every field value from above
    assert (a["field_min"], a["redo"], a["min_known"], a["field_max"]) == (lv.floor_value, 0, 0, 0.0)
    nx, ny = int(a["mx1"] - a["mx0"]), int(a["my1"] - a["my0"])
    assert nx > 100 and ny > 100
    assert np.array_equal(lv.t["axis_x"][0, :nx].cpu().numpy(), twin.t["axis_x"][0, :nx].cpu().numpy())
    assert np.array_equal(lv.t["axis_y"][0, :ny].cpu().numpy(), twin.t["axis_y"][0, :ny].cpu().numpy())
    occ, occ_twin = device_occ(lv)[0], device_occ(twin)[0]
    assert occ.any() and np.array_equal(occ, occ_twin)
    # ... and the block flags: an 8 x 8 block is flagged iff it holds a wall
    fp = (2 * lv.tmax + 17) & ~15
    flags = lv.t["occ"][FMAX * FPITCH:].view(2 * lv.tmax, fp).cpu().numpy() == (lv.c.occ_gen or 1)
    fh, fw = occ.shape
    pad = np.zeros((2 * lv.tmax * 8, 2 * lv.tmax * 8), dtype=bool)
    pad[:fh, :fw] = occ
    assert np.array_equal(flags[:, :2 * lv.tmax], pad.reshape(2 * lv.tmax, 8, 2 * lv.tmax, 8).any(axis=(1, 3)))
    check_slot(lv, 0, engine.likelihood_table(UNIT, 0.2)[0], d2, centre)


# ---- 3. three slots ----
def test_three_slots_and_a_view(pkg, engine):
    import torch
    synth = importlib.import_module("slam-2d-lidar-scan_amd.synth")
    dev = torch.device("cuda:0")
    kw = tfs.level_kw()
    lidar = engine.LidarModel.get(UNIT, R, FOV, BEAMS, WALL)
    lv = engine.SearchLevel(lidar, tfs.P, dev, bnb=False, **kw)
    maps = []
    for seed, (cx, cy) in zip(tfs.SEEDS, tfs.CENTRES):
        m = engine.MapState.create(SIZE, SIZE, INIT, UNIT, dev)
        m.upload(*synth.counts_from_world(synth.make_world(SIZE, UNIT, seed=seed, n_boxes=25)))
        m.ensure_contains([cx - lv.reach, cx + lv.reach], [cy - lv.reach, cy + lv.reach], UNIT)
        maps.append(m)
    eng = engine.ParticleEngine(lidar, maps, dev)
    table = engine.likelihood_table(UNIT, 0.2)
    d_c = eng.to_device(tfs.CENTRES)
    d2 = eng.field_build_distance(lv, d_c, 2, table, dist2=True)
    assert not eng.take_flags(fatal=0xffffffff).any()
    assert [(int(f["fh"]), int(f["fw"])) for f in lv.frames()] == list(tfs.SIZES)
    assert lv.c.cost_scale == lv.cost_scale == table[1]
    occs = [check_slot(lv, p, table[0], d2, f"slot {p}")[0] for p in range(tfs.P)]
    assert not np.array_equal(occs[0][:288, :288], occs[1][:288, :288]) and not np.array_equal(occs[1][:288, :288], occs[2][:288, :288])
    # slot 1 alone, through a view of a second level of three: the bytes of the parent's slot 1, the neighbours untouched
    other = engine.SearchLevel(lidar, tfs.P, dev, bnb=False, **kw)
    other.t["field"].fill_(-1)
    other.next_generation()
    v = other.view(1, 2)
    other.sync_view(v)
    d2v = torch.full((1, FMAX, FPITCH), -1, dtype=torch.int32, device=dev)
    raw_call(eng, v, 1, d_c[1:], table[0], d2v, d_maps=eng.d_maps.data_ptr() + ctypes.sizeof(_lib.Slam2dMap), d_flags=eng.flags.data_ptr() + 4)
    assert not eng.take_flags(fatal=0xffffffff).any()
    assert other.frames()[1].tobytes() == lv.frames()[1].tobytes()
    assert np.array_equal(other.field_cost(1), lv.field_cost(1))
    fh, fw = tfs.SIZES[1]
    assert np.array_equal(d2v[0, :fh, :fw].cpu().numpy(), d2[1, :fh, :fw].cpu().numpy())
    assert (other.t["field"][0] == -1).all() and (other.t["field"][2] == -1).all()


# ---- 4. crafted maps ----
def crafted_windows(nh, nw):
    """name -> occupied image of the map window [nh, nw] (a map cell is a field cell at a step of one unit)."""
    z = lambda: np.zeros((nh, nw), dtype=bool)
    out = {"empty": z(), "corners_and_mid_edge": z(), "row": z(), "all": ~z(), "far_wall": z()}
    for i, j in ((0, 0), (0, nw - 1), (nh - 1, 0), (nh - 1, nw - 1), (0, nw // 2)):
        out["corners_and_mid_edge"][i, j] = True
    out["row"][nh // 3, :] = True
    out["checkerboard"] = (np.add.outer(np.arange(nh), np.arange(nw)) % 2).astype(bool)
    out["far_wall"][:, 1] = True                               # a wall along the left edge: farther than R from most of the frame
    return out


@pytest.fixture(scope="module")
def blank(pkg):
    og, sm, lv = new_grid(pkg)
    eng = og.engine()
    d_c = eng.to_device([[WINDOW[0], WINDOW[1]]])
    eng.field_build_distance(lv, d_c, 2, (IDENTITY, 1.0))
    fr = lv.frames()[0]
    assert not eng.take_flags(fatal=0xffffffff).any()
    return dict(og=og, lv=lv, eng=eng, centre=d_c, window=tuple(int(fr[k]) for k in ("my0", "my1", "mx0", "mx1")))


@pytest.mark.parametrize("entries", [3 * 3 + 1, 65536])          # R = 3 and R = 256
@pytest.mark.parametrize("name", sorted(crafted_windows(4, 4)))
def test_crafted_maps(blank, name, entries):
    og, lv, eng = blank["og"], blank["lv"], blank["eng"]
    my0, my1, mx0, mx1 = blank["window"]
    walls = np.zeros((og.map.rows, og.map.cols), dtype=bool)
    walls[my0:my1, mx0:mx1] = crafted_windows(my1 - my0, mx1 - mx0)[name]
    og.set_counts(np.where(walls, WALLS[0], FREE[0]), np.where(walls, WALLS[1], FREE[1]))
    lut = np.arange(entries, dtype=np.uint32) * np.uint32(3) + np.uint32(11)
    assert dyard.reach(entries - 1) == (3 if entries == 10 else 256)
    d2 = eng.field_build_distance(lv, blank["centre"], 2, (lut, 1.0), dist2=True)
    assert not eng.take_flags(fatal=0xffffffff).any()
    occ, want = check_slot(lv, 0, lut, d2, (name, entries))
    fh, fw = occ.shape
    cap = entries - 1
    # the device's image is the crafted one, folded as the frame folds a map: the truncation of (X - xlo) / step sends two
    # neighbouring map columns (rows) to one field column (row) now and then, and leaves its neighbour without any
    ii, jj = np.nonzero(occ)
    rows_hit, cols_hit = occ.any(axis=1), occ.any(axis=0)
    if name == "empty":
        assert not occ.any() and (lv.field_cost(0) == lut[-1]).all()
    elif name == "all":
        assert np.array_equal(occ, np.outer(rows_hit, cols_hit)) and rows_hit.sum() > 0.8 * fh and cols_hit.sum() > 0.8 * fw
        assert want.max() <= min(cap, 18)
    elif name == "corners_and_mid_edge":
        assert occ.sum() == 5 and ii.max() - ii.min() >= fh - 3 and jj.max() - jj.min() >= fw - 3 and (ii == ii.min()).sum() == 3
    elif name == "row":
        assert rows_hit.sum() == 1 and occ.sum() > 0.8 * fw
    elif name == "checkerboard":
        assert 0.3 * occ.size < occ.sum() < 0.8 * occ.size and want.max() <= min(cap, 18) and (want == 1).any()
    else:
        assert cols_hit.sum() == 1 and occ.sum() > 0.8 * fh and jj[0] < 4
        assert (want[:, fw - 1] == cap).all() and (want[:, jj[0] + 2] == 4).sum() > 0.8 * fh      # beyond the cap from the wall; near it


# ---- 5. a field step of two map units ----
def test_a_field_step_of_two_map_units(pkg, scene, engine):
    sm = pkg.ScanMatcher(scene["og"], 0.7, 0.25, 2, 0.1, 0.25, 0.3, 0.15, 2)          # coarseFactor 2
    res = sm.clearance(WINDOW, level="coarse")
    lv = sm.last_cover["level"]
    occ, _ = device_occ(lv)
    assert lv.step == 2 * UNIT and res["dist"].shape == occ.shape and occ.shape[0] in (144, 145) and occ.shape[1] in (144, 145)
    assert 0 < occ.sum() < scene["world"].sum()                # several map cells fold into one field cell
    k = dyard.dist2(occ, 65535)
    want = np.sqrt(k.astype(np.float64)) * lv.step
    want[k >= 65535] = np.inf
    assert np.array_equal(res["dist"], want) and np.isfinite(want).all() and want.max() > 1.0
    lut = engine.likelihood_table(lv.step, 0.3)[0]
    d2 = scene["eng"].field_build_distance(lv, scene["centre"], 2, (lut, 1.0), dist2=True)
    check_slot(lv, 0, lut, d2, "coarse")


# ---- 6. stamps ----
def test_stale_bytes_are_not_walls(pkg, engine):
    import torch
    world, _, _ = walk()
    og, sm, lv = new_grid(pkg, world)
    eng = og.engine()
    d_c = eng.to_device([[WINDOW[0], WINDOW[1]]])
    lut = engine.likelihood_table(UNIT, 0.2)[0]
    d2 = eng.field_build_distance(lv, d_c, 2, (lut, 1.0), dist2=True)
    occ_a, want_a = check_slot(lv, 0, lut, d2, "map A")
    visited, total = og.map.download()
    cols = np.arange(og.map.cols)[None, :] >= og.map.cols // 2
    gone = (2 * visited > total) & cols                         # map B: the walls of the right half removed
    og.set_counts(np.where(gone, FREE[0], visited), np.where(gone, FREE[1], total))
    d2 = eng.field_build_distance(lv, d_c, 2, (lut, 1.0), dist2=True)
    occ_b, want_b = check_slot(lv, 0, lut, d2, "map B")
    _, raw = device_occ(lv)
    assert 0 < occ_b.sum() < occ_a.sum() and not np.array_equal(want_a, want_b)
    assert ((raw != 0) & (raw != lv.c.occ_gen)).any()           # map A's bytes are still there
    field_b = lv.field_cost(0).copy()
    # occ_gen = 0 at the C ABI: image and flags cleared by the call, the stamp 1
    c0 = _lib.Slam2dLevel.from_buffer_copy(lv.c)
    c0.occ_gen = 0
    lv.t["field"].fill_(-1)
    d2z = torch.full((1, FMAX, FPITCH), -1, dtype=torch.int32, device=eng.device)
    raw_call(eng, c0, 1, d_c, lut, d2z)
    assert not eng.take_flags(fatal=0xffffffff).any()
    assert np.array_equal(lv.field_cost(0), field_b) and np.array_equal(d2z[0, :289, :289].cpu().numpy(), want_b)
    raw0 = lv.t["occ"][:FMAX * FPITCH].view(FMAX, FPITCH)[:289, :289].cpu().numpy()
    assert np.array_equal(raw0 == 1, occ_b) and set(np.unique(raw0)) == {0, 1}


# ---- 7. the slot handed back ----
def test_the_slot_is_handed_back(scene, engine):
    eng, sm, lv = scene["eng"], scene["sm"], scene["lv"]
    blurred_scale = engine.cost_scale_for(lv.floor_value)
    table = engine.likelihood_table(UNIT, 0.2)
    d_c = scene["centre"]

    def distance_then(what):
        eng.field_build_distance(lv, d_c, 2, table)
        assert lv.c.cost_scale == table[1]
        assert (lv.t["tilestate"] == 1).all() and (lv.t["freerow"] == 0).all()
        lv.c.cost_scale = lv.cost_scale = blurred_scale        # the caller's part: the blurred field at its own scale again
        return what()

    twin = sm.covering_level("fine", WINDOW[2], shared=False)
    eng.field_build(twin, d_c, 2)
    distance_then(lambda: eng.field_build(lv, d_c, 2))
    assert not eng.take_flags(fatal=0xffffffff).any()
    assert np.array_equal(lv.field_cost(0), twin.field_cost(0)) and lv.frames()[0].tobytes() == twin.frames()[0].tobytes()
    # a lazy match: the twin's Slam2dMatch
    import torch
    pose, rng = scene["poses"][2], scene["scans"][2]
    d_est, d_rng = eng.to_device([list(pose)]), eng.to_device(rng)
    out = [torch.full((1, engine.MATCH_DOUBLES), -1, dtype=torch.int64, device=eng.device).view(torch.float64) for _ in range(2)]
    fresh = sm.covering_level("fine", WINDOW[2], shared=False)
    eng.match(fresh, d_est, 3, d_rng, 0.0, None, None, out[0])
    distance_then(lambda: eng.match(lv, d_est, 3, d_rng, 0.0, None, None, out[1]))
    assert not eng.take_flags(fatal=0xffffffff).any()
    a, b = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert a.tobytes() == b.tobytes() and np.isfinite(a[0, :6]).all()


# ---- 8. the consumers on a distance slot ----
def test_consumers_on_a_distance_slot(scene, engine):
    eng, lv = scene["eng"], scene["lv"]
    lut, scale = table = engine.likelihood_table(UNIT, 0.2)
    eng.field_build_distance(lv, scene["centre"], 2, table)
    assert not eng.take_flags(fatal=0xffffffff).any()
    fr = lv.frames()[0]
    field, frame = lv.field_cost(0).copy(), (float(fr["xlo"]), float(fr["ylo"]))
    assert np.array_equal(field, dyard.field_from(device_occ(lv)[0], lut)) and lv.c.cost_scale == scale
    free = int(lut[-1])                                        # a beam that leaves the field is a random measurement
    wlut, shift = engine.weight_table(scale, tfs.TEMPERATURE)
    sincos = tfs.memo_sincos(eng)
    near = [tuple(q) for q in scene["poses"]] + [(q[0] + 0.037, q[1] - 0.012, q[2] + 0.01) for q in scene["poses"]]
    inp = tfs.slot_inputs(0, frame, 289, 289, near, list(scene["scans"]) * 2, scene["scans"])
    want = tfs.yardsticks(inp, field, frame, scale, free, wlut, shift, sincos)
    assert (want["rows"][:24, 3] > 20).all() and len(np.unique(want["rows"][:, 2])) > 20
    assert int(want["step"]["report"][6]) >= 1 and int(want["step"]["report"][10]) == len(inp["cloud"])
    got = tfs.run_all(eng, lv, 0, inp, free, wlut, shift)
    tscore.same(got["rows"], want["rows"], "slam2d_score_poses")
    tsearch.same(got["words"], want["words"], "slam2d_search_lattice")
    tmcl.same(got["step"], want["step"], "slam2d_mcl_step")


# ---- 9. the Python surface ----
def test_search_poses_with_and_without_a_likelihood(scene, engine):
    eng, sm = scene["eng"], scene["sm"]
    rng = scene["scans"][4]
    table = engine.likelihood_table(UNIT, LIK["sigma"])
    res = sm.searchPoses(rng, WINDOW, step=0.5, headings=16, likelihood=LIK)
    lv, lat = sm.last_cover["level"], sm.last_cover["lattice"]
    blurred = sm.covering_level("fine", WINDOW[2])
    assert lv is not blurred and lv.cost_scale == lv.c.cost_scale == table[1] and lv is sm.covering_level("fine", WINDOW[2], likelihood=dict(LIK))
    # ... equals the engine call on a slot built by hand
    hand = sm.covering_level("fine", WINDOW[2], shared=False)
    eng.field_build_distance(hand, scene["centre"], 2, table)
    host = eng.search_host(eng.search_lattice(hand, 0, lat, eng.to_device(rng), int(table[0][-1])), lat, table[1])
    for k in ("cost", "heading", "score"):
        assert np.array_equal(res[k], host[k]), k
    fr = hand.frames()[0]
    frame = (float(fr["xlo"]), float(fr["ylo"]))
    lc, ls = tscore.device_sincos(eng, lyard.beam_angles(lat, FOV, BEAMS))
    words = lyard.search_lattice(hand.field_cost(0), frame, table[1], UNIT, lat, rng, FOV, R, int(table[0][-1]), lc, ls)
    assert np.array_equal(res["cost"], words >> np.uint64(16)) and np.array_equal(res["heading"], tsearch.headings(words))
    assert len(res["peaks"]) == 5 and res["peaks"][0].cost == int(res["cost"].min())
    # likelihood=None: the blurred field at its own scale, as before -- the yardstick on it
    assert blurred.c.cost_scale == blurred.cost_scale == engine.cost_scale_for(blurred.floor_value)
    plain = sm.searchPoses(rng, WINDOW, step=0.5, headings=16)
    assert sm.last_cover["level"] is blurred and sm.last_cover["lattice"] == lat
    free = int(engine.encode_cost(blurred.floor_value, blurred.cost_scale))
    words = lyard.search_lattice(blurred.field_cost(0), frame, blurred.c.cost_scale, UNIT, lat, rng, FOV, R, free, lc, ls)
    assert np.array_equal(plain["cost"], words >> np.uint64(16)) and np.array_equal(plain["heading"], tsearch.headings(words))
    assert not np.array_equal(plain["cost"], res["cost"])
    # scorePoses takes the keyword too
    rows = sm.scorePoses(scene["poses"], rng, window=WINDOW, likelihood=LIK)
    c, s = tscore.device_sincos(eng, np.array([tscore.yard.beam_angles(p[2], FOV, BEAMS) for p in scene["poses"]]))
    want = tscore.yard.score_poses(hand.field_cost(0), frame, table[1], UNIT, scene["poses"], rng, FOV, R, c, s)
    assert np.array_equal(rows["score"], want[:, 0]) and np.array_equal(rows["beam_score"], want[:, 2])


@pytest.mark.parametrize("likelihood", [LIK, None])
def test_localiser_against_the_yardstick(pkg, scene, engine, likelihood):
    localise = importlib.import_module("slam-2d-lidar-scan_amd.localise")
    eng, sm = scene["eng"], scene["sm"]
    N, S, sigma = 130, 3, (0.03, 0.02, 0.015)
    readings = [dict(x=float(p[0]), y=float(p[1]), theta=float(p[2]), range=list(map(float, r))) for p, r in zip(scene["poses"], scene["scans"])]
    loc = pkg.Localiser(sm, WINDOW, particles=N, sigma=sigma, temperature=tfs.TEMPERATURE, seed=5, likelihood=likelihood)
    lv = loc.level
    fr = lv.frames()[0]
    field, frame = lv.field_cost(0).copy(), (float(fr["xlo"]), float(fr["ylo"]))
    if likelihood is None:
        scale = engine.cost_scale_for(lv.floor_value)
        free = int(engine.encode_cost(lv.floor_value, scale))
        twin = sm.covering_level("fine", WINDOW[2], shared=False)
        eng.field_build(twin, scene["centre"], 2)
        assert np.array_equal(field, twin.field_cost(0))       # the blurred field
    else:
        lut, scale = engine.likelihood_table(UNIT, likelihood["sigma"])
        free = int(lut[-1])
        assert np.array_equal(field, dyard.field_from(device_occ(lv)[0], lut))
    assert lv.c.cost_scale == lv.cost_scale == scale and loc.outside_cost == free
    wlut, shift = engine.weight_table(scale, tfs.TEMPERATURE)
    assert loc.shift == shift and np.array_equal(loc.d_lut.cpu().numpy().view(np.uint32), wlut)
    cur = loc.seed_at(scene["poses"][0], (0.05, 0.05, 0.03))
    reports = loc.run(readings[:S])
    amp = [v / math.sqrt(4.0 / 3.0) for v in sigma]
    sincos = lambda a: tscore.device_sincos(eng, a)
    for i in range(S):
        motion = localise.odometry_motion(readings[i - 1], readings[i]) if i else (0.0, 0.0, 0.0)
        want = mcl.step(field, frame, scale, UNIT, cur, motion, amp, 5, i, scene["scans"][i], FOV, R, free, wlut, shift, sincos)
        cur = want["out"]
        assert reports[i] == engine.mcl_report_host(want["report"]), i
    assert np.array_equal(loc.poses().view(np.uint64), np.ascontiguousarray(cur).view(np.uint64))


@pytest.mark.parametrize("max_dist", [None, 1.0])
def test_clearance(scene, max_dist):
    sm = scene["sm"]
    res = sm.clearance(WINDOW) if max_dist is None else sm.clearance(WINDOW, max_dist=max_dist)
    lv = sm.last_cover["level"]
    assert set(res) == {"dist", "xs", "ys"} and lv is not sm.covering_level("fine", WINDOW[2])
    cap = 65535 if max_dist is None else 101                   # floor((1.0 / 0.1)^2) + 2 entries
    assert len(lv.distance_table[0]) == cap + 1
    occ, _ = device_occ(lv)
    k = dyard.dist2(occ, cap)
    want = np.sqrt(k.astype(np.float64)) * UNIT
    want[k >= cap] = np.inf
    assert res["dist"].shape == (289, 289) and np.array_equal(res["dist"], want)
    assert np.isinf(want).any() == (max_dist is not None) and (want[occ] == 0).all() and np.isfinite(want).sum() > 1000
    fr = lv.frames()[0]
    assert np.array_equal(res["xs"], float(fr["xlo"]) + (np.arange(289) + 0.5) * UNIT) and len(res["ys"]) == 289
