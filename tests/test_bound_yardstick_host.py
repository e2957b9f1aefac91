"""The conventions of tests/bound_yardstick.py pinned without a GPU.  On a random uint32 cost field everything the device derives
for the tile bounds is built here in NumPy -- the 4 x 4 block minima (gmin), the minimum over 2 x 2 of them (gmin2), its top byte
(gmin2b) -- together with cell lists whose cells repeat blocks, random priors and every exact score in the library's expression
(-(sum * inv) + rv) + tw.  ``tile_bounds`` must dominate ``tile_max`` of those scores everywhere (a bound read one block off,
or from the wrong pitch, does not: the minima of a random field say nothing about the neighbouring block), and clearing one byte
of the image must raise exactly the bounds that read it.

The definitions of the other bound kernels (the 32-bit minima, the two levels, the angle planes) are pinned the same way on
small fields: the phase layout of gmin3d and the two packings of a cell against the device's index expressions, admissibility
of every bound against plain exact scores under a zero prior (cubes of 17, 33 and 49 poses a side with their partial tiles, a
window corner with y0 & 3 == x0 & 3 == 3), a child's bound never above its parent's, the monotone key map, and the replays of
k_bound1 -> k_seed -> k_bound2 and of k_abound -> k_aseed on hand-made bounds."""
import numpy as np
import pytest

import bound_yardstick as yard

GP, LP = 44, 48                   # entries per row of the minima (a 176 x 176-cell field), pitch of the byte image
COST_SCALE = float(2 ** 26)


def _scene(nx, seed, ntheta=3, K=40):
    rs = np.random.RandomState(seed)
    ncell, nbt = nx // 2, (nx + 3) // 4
    fh = 4 * GP
    # uint32 costs over the whole range: a ramp of 0.6 byte steps (2^24) per cell under noise of a third of a step -- a block's
    # minimum is then near its cells' costs and says nothing about the next block's
    ramp = np.add.outer(np.arange(fh), np.arange(fh)).astype(np.uint64) * 10_000_000
    F = (ramp + rs.randint(0, 2 ** 32 - int(ramp.max()), size=(fh, fh), dtype=np.uint64) // 128).astype(np.uint32)
    gmin = F.reshape(GP, 4, GP, 4).min(axis=(1, 3))
    g2 = yard.min2x2(gmin)
    img = np.zeros((GP, LP), dtype=np.uint8)
    img[:, :GP] = (g2 >> 24).astype(np.uint8)
    # cells (the field index of pose offset (0, 0): y0 = cy - ncell, as the sweep reads F[y0 + iy, x0 + ix]); groups of
    # neighbours share a 4 x 4 block, so blocks repeat within a list -- side by side and far apart
    kcount = np.array([K, K - 7, 1][:ntheta] + [K] * max(0, ntheta - 3))
    y0 = np.zeros((ntheta, K), dtype=np.int64)
    x0 = np.zeros((ntheta, K), dtype=np.int64)
    for it in range(ntheta):
        by = rs.randint(0, (fh - nx) // 4, size=K // 4 + 1)
        bx = rs.randint(0, (fh - nx) // 4, size=K // 4 + 1)
        blk = np.repeat(np.arange(K // 4 + 1), 4)[:K]
        blk[K - 3:] = 0                                                 # ... and the first block once more at the end
        y0[it] = 4 * by[blk] + rs.randint(0, 4, size=K)
        x0[it] = 4 * bx[blk] + rs.randint(0, 4, size=K)
    assert y0.max() + nx <= fh and x0.max() + nx <= fh
    pcells = (((y0 >> 2) * GP + (x0 >> 2)) * 4).astype(np.int32)
    rv = -5.0 * rs.random_sample((nx, nx))
    tw = -3.0 * rs.random_sample((nx, nx))
    prior = np.full((4 * nbt, 4 * nbt), -np.inf)
    prior[:nx, :nx] = rv + tw
    pmax = np.full((nbt, 4 * ((nbt + 3) // 4)), -np.inf)               # (padding columns as the device leaves them)
    pmax[:, :nbt] = prior.reshape(nbt, 4, nbt, 4).max(axis=(1, 3))
    inv = 1.0 / COST_SCALE
    ar = np.arange(nx)
    cube = np.empty((ntheta, nx, nx))
    for it in range(ntheta):
        k = kcount[it]
        acc = F[y0[it, :k, None, None] + ar[None, :, None], x0[it, :k, None, None] + ar[None, None, :]].sum(axis=0, dtype=np.uint64)
        cube[it] = (-(acc.astype(np.float64) * inv) + rv) + tw
    return dict(nx=nx, nbt=nbt, img=img, pcells=pcells, kcount=kcount, pmax=pmax, cube=cube, y0=y0, x0=x0, gmin=gmin, F=F)


@pytest.mark.parametrize("nx", [31, 63])
def test_bounds_dominate_every_exact_score(nx):
    sc = _scene(nx, seed=nx)
    nbt = sc["nbt"]
    U = yard.tile_bounds(sc["img"], sc["pcells"], sc["kcount"], sc["pmax"], COST_SCALE, GP, nbt)
    best, has_nan = yard.tile_max(sc["cube"], nx, nbt)
    assert U.shape == best.shape == (3, nbt, nbt) and not has_nan.any() and np.isfinite(best).all()
    assert (U >= best).all()
    # not vacuously: behind a list of one cell (angle 2) a bound exceeds the score of its tile's first pose by at most 6 cells
    # of ramp (0.15 each at this scale: block corner to window corner), the byte's floor (0.25) and the noise (0.09) -- 1.24 --
    # and that pose's prior lies below the tile's best by 8 at most, by much less in some of the 64 to 256 tiles
    gap = U - best
    print(f"nx {nx}: smallest gap per angle {gap.min(axis=(1, 2))}")
    assert gap.min() >= 0 and gap[2].min() < 2.0
    # the yardstick's indexing against the brute force over every tile, angle 0
    img = sc["img"].astype(np.int64)
    e = sc["pcells"][0, :sc["kcount"][0]].astype(np.int64) >> 2
    for by in (0, 1, nbt - 1):
        for bx in (0, nbt // 2, nbt - 1):
            s = int(sum(img[ee // GP + by, ee % GP + bx] for ee in e))
            assert U[0, by, bx] == (-((float(s) * 16777216.0) * (1.0 / COST_SCALE)) + sc["pmax"][by, bx]) + 1e-9


@pytest.mark.parametrize("nx", [31, 63])
def test_bound_one_block_off_is_not_admissible(nx):
    """The power of the check above: the same lists read one entry to the right or one row down violate it."""
    sc = _scene(nx, seed=nx)
    nbt = sc["nbt"]
    best, _ = yard.tile_max(sc["cube"], nx, nbt)
    for shift in (4, 4 * GP):
        U = yard.tile_bounds(sc["img"], sc["pcells"] + shift, sc["kcount"], sc["pmax"], COST_SCALE, GP, nbt)
        assert (U < best).any()


@pytest.mark.parametrize("nx", [31, 63])
def test_tile_max_partial_tiles_and_nan(nx):
    sc = _scene(nx, seed=nx + 1)
    nbt, cube = sc["nbt"], sc["cube"].copy()
    cube[1, nx - 1, nx - 1] = np.nan                                    # the last pose: a partial tile of 3 x 3 poses
    cube[2, 0:4, 4:8] = np.nan                                          # a whole tile
    best, has_nan = yard.tile_max(cube, nx, nbt)
    assert has_nan.sum() == 2 and has_nan[1, nbt - 1, nbt - 1] and has_nan[2, 0, 1]
    assert best[2, 0, 1] == -np.inf
    rest = cube[1, 4 * (nbt - 1):, 4 * (nbt - 1):]
    assert rest.shape == (3, 3) and best[1, nbt - 1, nbt - 1] == np.nanmax(rest)
    assert best[0, nbt - 1, 0] == cube[0, 4 * (nbt - 1):, 0:4].max() and cube[0, 4 * (nbt - 1):, 0:4].shape == (3, 4)
    assert best[0, 2, 3] == cube[0, 8:12, 12:16].max()


@pytest.mark.parametrize("nx", [31, 63])
def test_clearing_one_byte_raises_exactly_the_bounds_that_read_it(nx):
    sc = _scene(nx, seed=nx + 2)
    nbt = sc["nbt"]
    U0 = yard.tile_bounds(sc["img"], sc["pcells"], sc["kcount"], sc["pmax"], COST_SCALE, GP, nbt)
    checked = 0
    for it, k, by, bx in ((0, 0, 0, 0), (0, 5, nbt - 1, nbt - 1), (1, 3, 2, nbt - 1), (2, 0, nbt // 2, 1)):
        e = int(sc["pcells"][it, k]) >> 2
        Y, X = e // GP + by, e % GP + bx
        img = sc["img"].copy()
        if img[Y, X] == 0:
            continue
        img[Y, X] = 0
        U1 = yard.tile_bounds(img, sc["pcells"], sc["kcount"], sc["pmax"], COST_SCALE, GP, nbt)
        want = np.zeros(U0.shape, dtype=bool)
        for jt in range(len(sc["kcount"])):
            ee = sc["pcells"][jt, :sc["kcount"][jt]].astype(np.int64) >> 2
            for Y0, X0 in zip(ee // GP, ee % GP):
                if 0 <= Y - Y0 < nbt and 0 <= X - X0 < nbt:
                    want[jt, Y - Y0, X - X0] = True
        assert want[it, by, bx]
        assert np.array_equal(U1 > U0, want) and np.array_equal(U1 != U0, want)
        checked += 1
    assert checked >= 3


# ---------------------------------------------------------------------------------------------------------------------
# the 32-bit, two-level and angle definitions
# ---------------------------------------------------------------------------------------------------------------------
G2 = 24                             # entries per row of the minima of the small scenes below (a 96 x 96-cell field)


def _scene32(nx, seed, ntheta=3, K=12):
    """A random uint32 field, its 4 x 4 block minima and the images derived from them, cell lists of window corners (y0, x0)
    -- the field index of pose (0, 0); the first with y0 & 3 == x0 & 3 == 3 -- and every exact score under a zero prior."""
    rs = np.random.RandomState(seed)
    fh = 4 * G2
    F = rs.randint(0, 2 ** 32, size=(fh, fh), dtype=np.uint64).astype(np.uint32)
    gmin = F.reshape(G2, 4, G2, 4).min(axis=(1, 3))
    kcount = np.array([K, K - 5, 1][:ntheta])
    y0 = rs.randint(0, fh - nx - 8, size=(ntheta, K))
    x0 = rs.randint(0, fh - nx - 8, size=(ntheta, K))
    y0[:, 0] |= 3
    x0[:, 0] |= 3
    assert (y0 + nx <= fh).all() and (x0 + nx <= fh).all() and all(len(set((v & 3).ravel().tolist())) == 4 for v in (y0, x0))
    pcells = (((y0 >> 2) * G2 + (x0 >> 2)) * 4).astype(np.int32)
    nbt = (nx + 3) // 4
    pmax = np.full((nbt, 4 * ((nbt + 3) // 4)), -np.inf)
    pmax[:, :nbt] = 0.0
    inv = 1.0 / COST_SCALE
    ar = np.arange(nx)
    cube = np.empty((ntheta, nx, nx))
    for it in range(ntheta):
        k = kcount[it]
        acc = F[y0[it, :k, None, None] + ar[None, :, None], x0[it, :k, None, None] + ar[None, None, :]].sum(axis=0, dtype=np.uint64)
        cube[it] = -(acc.astype(np.float64) * inv)
    return dict(nx=nx, nbt=nbt, F=F, gmin=gmin, gmin2=yard.min2x2(gmin) >> 12, g3=yard.min3x3(gmin) >> 12, pcells=pcells,
                kcount=kcount, pmax=pmax, cube=cube, y0=y0, x0=x0)


def test_min3x3_against_loops():
    g = np.random.RandomState(1).randint(0, 2 ** 32, size=(7, 9), dtype=np.uint64).astype(np.uint32)
    m = yard.min3x3(g)
    assert m.shape == g.shape and m.dtype == g.dtype
    for Y in range(7):
        for X in range(9):
            assert m[Y, X] == min(g[min(Y + a, 6), min(X + b, 8)] for a in range(3) for b in range(3))
    assert (m <= yard.min2x2(g)).all() and (m < yard.min2x2(g)).any()


def test_unphase_inverts_the_device_layout():
    """The layout written entry by entry with the index expression of gmin2_entry (csrc/slam2d.hip)."""
    gp = 12
    hp = gp >> 1
    img = np.random.RandomState(2).randint(0, 2 ** 20, size=(gp, gp)).astype(np.uint32)
    flat = np.zeros(gp * gp, dtype=np.uint32)
    for Y in range(gp):
        for X in range(gp):
            flat[((((Y & 1) << 1) | (X & 1)) * hp + (Y >> 1)) * hp + (X >> 1)] = img[Y, X]
    assert np.array_equal(yard.unphase(flat, gp), img)
    assert np.array_equal(yard.unphase(flat.reshape(4, hp, hp), gp), img)
    assert not np.array_equal(yard.unphase(flat.reshape(4, hp, hp)[[0, 2, 1, 3]], gp), img)


def test_decode_p3_agrees_with_pcells():
    """Every corner (y0, x0) of a small grid, all four parities of its block (Y0, X0) included, in k_endpoints' two packings."""
    gp = 12
    hp = gp >> 1
    y0, x0 = np.meshgrid(np.arange(4 * gp), np.arange(4 * gp), indexing="ij")
    Y0, X0 = y0 >> 2, x0 >> 2
    pcells = (Y0 * gp + X0) * 4
    p3 = (((((Y0 & 1) << 1) | (X0 & 1)) * hp + (Y0 >> 1)) * hp + (X0 >> 1)) * 4
    gy, gx = yard.decode_p3(p3.astype(np.int32), gp)
    assert np.array_equal(gy, (pcells >> 2) // gp) and np.array_equal(gx, (pcells >> 2) % gp)
    assert {(int(a) & 1, int(b) & 1) for a, b in zip(gy.ravel(), gx.ravel())} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_tile_bounds32_is_tile_bounds_at_the_scale_of_the_32_bit_image():
    sc = _scene32(17, seed=3)
    U = yard.tile_bounds32(sc["gmin2"], sc["pcells"], sc["kcount"], sc["pmax"], COST_SCALE, G2, sc["nbt"])
    g = sc["gmin2"].astype(np.int64)
    for it, by, bx in ((0, 0, 0), (1, 4, 2), (2, 3, 4)):
        e = sc["pcells"][it, :sc["kcount"][it]].astype(np.int64) >> 2
        s = int(sum(g[ee // G2 + by, ee % G2 + bx] for ee in e))
        assert U[it, by, bx] == (-((float(s) * 4096.0) * (1.0 / COST_SCALE)) + 0.0) + 1e-9
    # the byte image's default is untouched: the same call without a scale multiplies by 2^24
    U8 = yard.tile_bounds(sc["gmin2"] >> 12, sc["pcells"], sc["kcount"], sc["pmax"], COST_SCALE, G2, sc["nbt"])
    assert (U8 >= U).all() and (U8 > U).any()


@pytest.mark.parametrize("nx", [17, 33, 49])
def test_level_bounds_dominate_every_exact_score(nx):
    """tile1_bounds over every pose of its 8 x 8 tile, tile_bounds32 over every pose of its 4 x 4 tile (partial tiles at all
    three sizes), and a child's bound never above its parent's.  On a field of independent uniform costs a block's minimum
    says nothing about its neighbour's: a sum read one entry off does not dominate."""
    sc = _scene32(nx, seed=nx)
    nbt, nb1 = sc["nbt"], (nx + 7) // 8
    U2 = yard.tile_bounds32(sc["gmin2"], sc["pcells"], sc["kcount"], sc["pmax"], COST_SCALE, G2, nbt)
    U1 = yard.tile1_bounds(sc["g3"], sc["pcells"], sc["kcount"], sc["pmax"], COST_SCALE, G2, nx)
    assert U1.shape == (3, 8, 8) and U2.shape == (3, nbt, nbt)
    inside = np.zeros((8, 8), dtype=bool)
    inside[:nb1, :nb1] = True
    assert np.isfinite(U1[:, inside]).all() and (U1[:, ~inside] == -np.inf).all()
    best2, _ = yard.tile_max(sc["cube"], nx, nbt)
    best1, _ = yard.tile_max(sc["cube"], nx, nb1, size=8)
    assert (U2 >= best2).all() and (U1[:, :nb1, :nb1] >= best1).all()
    for R in range(nb1):
        for C1 in range(nb1):
            kids = U2[:, 2 * R:2 * R + 2, 2 * C1:2 * C1 + 2]
            assert kids.size and (kids <= U1[:, R, C1, None, None]).all()
    for shift in (4, 4 * G2):
        assert (yard.tile_bounds32(sc["gmin2"], sc["pcells"] + shift, sc["kcount"], sc["pmax"], COST_SCALE, G2, nbt) < best2).any()


@pytest.mark.parametrize("nx", [17, 33, 49])
def test_level_1_bound_reaches_the_third_block(nx):
    """One cell with y0 & 3 == x0 & 3 == 3 on a field that costs 2^30 everywhere but at the last pose's cell of one 8 x 8 tile
    (the last VALID pose of a partial tile): that cell lies in block (Y0 + 2 R + 2, X0 + 2 C1 + 2), or + 1 where the tile is cut.
    Only the 3 x 3 minimum at exactly (Y0 + 2 R, X0 + 2 C1) sees it; the tile's bound must be 1e-9, every other tile's far lower."""
    nb1, nbt = (nx + 7) // 8, (nx + 3) // 4
    fh = 4 * G2
    y0, x0 = 7, 11
    pcells = np.array([[((y0 >> 2) * G2 + (x0 >> 2)) * 4]], dtype=np.int32)
    pmax = np.zeros((nbt, nbt))
    for R, C1 in ((0, 0), (nb1 - 1, 1), (1, nb1 - 1), (nb1 - 1, nb1 - 1)):
        dy, dx = min(8 * R + 7, nx - 1), min(8 * C1 + 7, nx - 1)
        F = np.full((fh, fh), 2 ** 30, dtype=np.uint32)
        F[y0 + dy, x0 + dx] = 0
        gmin = F.reshape(G2, 4, G2, 4).min(axis=(1, 3))
        g3 = yard.min3x3(gmin) >> 12
        U1 = yard.tile1_bounds(g3, pcells, [1], pmax, COST_SCALE, G2, nx)[0]
        want = np.full((8, 8), -np.inf)
        zy, zx = (y0 + dy) >> 2, (x0 + dx) >> 2
        for r in range(nb1):                                            # (the tiles below and to the right see that block as well)
            for c in range(nb1):
                sees = 0 <= zy - ((y0 >> 2) + 2 * r) <= 2 and 0 <= zx - ((x0 >> 2) + 2 * c) <= 2
                want[r, c] = 1e-9 if sees else (-((float(2 ** 18) * 4096.0) * (1.0 / COST_SCALE)) + 0.0) + 1e-9
        assert want[R, C1] == 1e-9 and np.array_equal(U1, want), (R, C1)
        if dy == 8 * R + 7 and dx == 8 * C1 + 7:                        # a whole tile: the 2 x 2 minima do not reach that cell
            assert yard.tile1_bounds(yard.min2x2(gmin) >> 12, pcells, [1], pmax, COST_SCALE, G2, nx)[0, R, C1] < 0
        # ... and through the device's layout: planes swapped, or the plane read at the wrong row, lose it
        hp = G2 // 2
        flat = np.zeros(G2 * G2, dtype=np.uint32)
        Y, X = np.meshgrid(np.arange(G2), np.arange(G2), indexing="ij")
        flat[((((Y & 1) << 1) | (X & 1)) * hp + (Y >> 1)) * hp + (X >> 1)] = g3
        assert np.array_equal(yard.unphase(flat, G2), g3)


def test_tile1_bounds_take_the_largest_prior_of_the_children_inside():
    sc = _scene32(17, seed=5)                                           # nbt 5, nb1 3: the last level-1 row and column have one child row / column
    pmax = sc["pmax"].copy()
    pmax[:, :5] = -np.arange(25.0).reshape(5, 5)
    pmax[4, 4] = np.inf                                                 # (a tile with a NaN prior)
    U1 = yard.tile1_bounds(sc["g3"], sc["pcells"], sc["kcount"], pmax, COST_SCALE, G2, 17)
    x = -((yard.tile_sums(sc["g3"], sc["pcells"], sc["kcount"], G2, 3, stride=2).astype(np.float64) * 4096.0) * (1.0 / COST_SCALE))
    assert U1[0, 2, 2] == np.inf and U1[0, 0, 0] == (x[0, 0, 0] + 0.0) + 1e-9
    assert U1[1, 1, 1] == (x[1, 1, 1] - 12.0) + 1e-9 and U1[2, 2, 1] == (x[2, 2, 1] - 22.0) + 1e-9 and U1[1, 0, 2] == (x[1, 0, 2] - 4.0) + 1e-9


def test_angle_bounds_dominate_every_score_of_a_5_x_5_plane():
    sc = _scene32(5, seed=7)
    prior = np.zeros((2, 25))
    U = yard.angle_bounds(sc["gmin2"], sc["pcells"], sc["kcount"], prior, COST_SCALE, G2, fine=False)
    assert U.shape == (3,) and (U >= sc["cube"].max(axis=(1, 2))).all()
    e = sc["pcells"][1, :sc["kcount"][1]].astype(np.int64) >> 2
    s = int(sc["gmin2"].astype(np.int64)[e // G2, e % G2].sum())
    assert U[1] == (-((float(s) * 4096.0) / COST_SCALE) + 0.0) + 1e-9
    assert (yard.angle_bounds(sc["gmin2"], sc["pcells"] + 4, sc["kcount"], prior, COST_SCALE, G2, fine=False) < sc["cube"].max(axis=(1, 2))).any()
    # the prior: its largest sum on a coarse level, +inf with a NaN, not read on a fine level; and a division by the scale --
    # at a scale that is no power of two the reciprocal gives other bits
    pr = prior.copy()
    pr[0] = -5.0
    pr[0, 3], pr[1, 3], pr[1, 7] = -1.0, -0.5, 3.0                      # the largest SUM is pose 3's, -1.5 (pose 7: -2)
    sums = yard.tile_sums(sc["gmin2"], sc["pcells"], sc["kcount"], G2, 1)[:, 0, 0].astype(np.float64)
    assert np.array_equal(yard.angle_bounds(sc["gmin2"], sc["pcells"], sc["kcount"], pr, COST_SCALE, G2, fine=False),
                          (-((sums * 4096.0) / COST_SCALE) - 1.5) + 1e-9)
    assert np.array_equal(yard.angle_bounds(sc["gmin2"], sc["pcells"], sc["kcount"], pr, COST_SCALE, G2, fine=True), U)
    pr[1, 11] = np.nan
    assert (yard.angle_bounds(sc["gmin2"], sc["pcells"], sc["kcount"], pr, COST_SCALE, G2, fine=False) == np.inf).all()
    differs = 0
    for scale in (3.0e7 + 7.0 * i for i in range(40)):
        Ud = yard.angle_bounds(sc["gmin2"], sc["pcells"], sc["kcount"], prior, scale, G2, fine=True)
        assert np.array_equal(Ud, (-((sums * 4096.0) / scale) + 0.0) + 1e-9)
        differs += not np.array_equal(Ud, (-((sums * 4096.0) * (1.0 / scale)) + 0.0) + 1e-9)
    assert differs > 0


def test_order_bits_is_monotone_and_invertible():
    v = np.array([-np.inf, -1e3, -0.0, 0.0, 1e-300, 1e300, np.inf])
    k = yard.order_bits(v)
    assert k.dtype == np.uint64 and (k[1:] > k[:-1]).all()
    assert np.array_equal(yard.unorder_bits(k).view(np.uint64), v.view(np.uint64))
    assert int(yard.order_bits(-np.inf)) == 0x000FFFFFFFFFFFFF and float(yard.unorder_bits(np.uint64(0x000FFFFFFFFFFFFF))) == -np.inf
    assert float(yard.unorder_bits(yard.order_bits(-57.25))) == -57.25


def _hand_made(nx=17):
    nbt = (nx + 3) // 4
    U1 = np.full((2, 8, 8), -np.inf)
    U1[0, :3, :3], U1[1, :3, :3] = -44.0, -30.0
    U1[0, 0, 0], U1[1, 1, 1] = -1.0, -2.0
    U2 = np.stack([np.full((nbt, nbt), -45.0), np.full((nbt, nbt), -35.0)])
    U2[0, 0, 1], U2[1, 2, 2] = -1.5, -2.5
    cube = np.stack([np.full((nx, nx), -50.0), np.full((nx, nx), -40.0)])
    cube[1, 9, 10] = -3.0                                               # tile (2, 2) of angle 1, child 0 of level-1 tile (1, 1)
    return U1, U2, np.zeros((nbt, 8)), cube


def test_replay_two_level_seed_angle_is_not_the_angle_of_the_maximum():
    U1, U2, pmax, cube = _hand_made()
    key, seed_best, final_best = yard.replay_two_level(U1, U2, pmax, cube, 17)
    assert int(key) == (int(yard.order_bits(-1.0)) & ~0x3FFF) | (0 << 6) | 0      # angle 0, tile 0: the best level-1 bound
    assert seed_best == -50.0                                            # its best child by U2 is (0, 1): angle 0 scores -50 everywhere
    assert final_best == -3.0                                            # angle 1's candidate (2, 2) holds the cube's maximum
    # a key's tile index is R * 8 + C1 and ties go to the lowest index; a seed tile of NaNs only leaves -inf
    U1[1, 1, 1] = U1[1, 2, 0] = -0.5
    cube[1, 8:12, 8:12] = np.nan
    key, seed_best, final_best = yard.replay_two_level(U1, U2, pmax, cube, 17)
    assert int(key) == (int(yard.order_bits(-0.5)) & ~0x3FFF) | (1 << 6) | 9
    assert seed_best == -np.inf and final_best == -50.0                 # (angle 1's candidate is that tile of NaNs again)
    # more than the margin below the seed's score no level-1 tile is opened: none of angle 1 at -34 < -3.5 - 30
    U1, U2, pmax, cube = _hand_made()
    cube[0] = -3.5
    U1[1, :3, :3], U2[1] = -34.0, -35.0
    assert yard.replay_two_level(U1, U2, pmax, cube, 17)[1:] == (-3.5, -3.5)


def test_replay_two_level_without_a_finite_best_bound():
    """Every angle's best level-1 tile is +inf (a NaN prior in it): no key, no seed; k_bound2 then scores each angle's first
    +inf child, here tiles of NaNs only."""
    U1, U2, pmax, cube = _hand_made()
    U1[:, 0, 0], U2[:, 0, 0], pmax[0, 0] = np.inf, np.inf, np.inf
    cube[:, 0:4, 0:4] = np.nan
    key, seed_best, final_best = yard.replay_two_level(U1, U2, pmax, cube, 17)
    assert int(key) == 0 and seed_best == -np.inf and final_best == -np.inf


def test_replay_angle():
    U = np.array([-7.0, -3.0, -np.inf, -3.0])
    planes = -10.0 - np.arange(4 * 25.0).reshape(4, 25)
    key, it, best = yard.replay_angle(U, planes)
    assert int(key) == (int(yard.order_bits(-3.0)) & ~0x3FFF) | 3 and it == 3 and best == -85.0
    U[0] = np.inf                                                       # a NaN plane: always the seed, and no threshold from it
    planes[0, 4] = np.nan
    key, it, best = yard.replay_angle(U, planes)
    assert int(key) == (int(yard.order_bits(1e300)) & ~0x3FFF) | 0 and it == 0 and best == -np.inf
    assert yard.replay_angle(np.full(3, -np.inf), planes[:3]) == (np.uint64(0), None, -np.inf)


def test_tile_bounds_at_the_largest_cube():
    """128 angles x 256 tiles x 360 cells (the largest cube branch and bound accepts): one vectorised gather per angle, a
    quarter of a second; against the sum taken tile by tile at three angles."""
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, size=(GP, LP)).astype(np.uint8)
    e = rs.randint(0, GP - 16, size=(128, 360)) * GP + rs.randint(0, GP - 16, size=(128, 360))
    kcount = np.full(128, 360)
    kcount[5] = 0
    U = yard.tile_bounds(img, (4 * e).astype(np.int32), kcount, np.zeros((16, 16)), COST_SCALE, GP, 16)
    assert U.shape == (128, 16, 16) and (U[5] == 1e-9).all()
    big = img.astype(np.int64)
    for it in (0, 64, 127):
        for by, bx in ((0, 0), (15, 15), (7, 12)):
            s = big[e[it] // GP + by, e[it] % GP + bx].sum()
            assert U[it, by, bx] == -((float(s) * 16777216.0) * (1.0 / COST_SCALE)) + 1e-9
