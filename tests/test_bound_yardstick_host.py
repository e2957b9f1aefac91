"""The conventions of tests/bound_yardstick.py pinned without a GPU.  On a random uint32 cost field everything the device derives
for the tile bounds is built here in NumPy -- the 4 x 4 block minima (gmin), the minimum over 2 x 2 of them (gmin2), its top byte
(gmin2b) -- together with cell lists whose cells repeat blocks, random priors and every exact score in the library's expression
(-(sum * inv) + rv) + tw.  ``tile_bounds`` must dominate ``tile_max`` of those scores everywhere (a bound read one block off,
or from the wrong pitch, does not: the minima of a random field say nothing about the neighbouring block), and clearing one byte
of the image must raise exactly the bounds that read it."""
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
