"""The definition of the tile bounds of branch and bound (include/slam2d.h, "Branch and bound") in NumPy, for the tests: what
k_bound_lds must leave in Slam2dLevel.bounds, from the byte image of the bound minima (Slam2dLevel.gmin2b) and the cell lists
as they lie in memory, by a plain sum over every cell of the list -- no runs, no batches, no padding; and what a bound has to
dominate: the largest score of each 4 x 4 pose tile of a cube.

Likewise for the other bound kernels of csrc/slam2d.hip: k_bound (tile_bounds32: the 32-bit minima gmin2), the two levels of
k_bound1 / k_seed / k_bound2 (min3x3, unphase, decode_p3, tile1_bounds, replay_two_level) and the angle bounds of k_abound /
k_aseed (angle_bounds, replay_angle).  Every sum runs over every cell of a list in int64: no batches, no lanes, and the phase
planes of gmin3d are undone (unphase) before anything is added up."""
import numpy as np

BNB_MARGIN = 30.0                   # SLAM2D_BNB_MARGIN (include/slam2d.h)


def min2x2(g):
    """min(g[Y..Y+1][X..X+1]) with the indices clamped to the image, as the device takes it."""
    gy = np.concatenate([g[1:], g[-1:]], axis=0)
    m = np.minimum(g, gy)
    mx = np.concatenate([m[:, 1:], m[:, -1:]], axis=1)
    return np.minimum(m, mx)


def tile_sums(img, pcells, kcount, gp, nbt, stride=1):
    """S[it, by, bx] = sum over the cells k < kcount[it] of img[Y0_k + stride by, X0_k + stride bx] in int64, with
    e = pcells >> 2 (pcells holds byte offsets into the 32-bit image of gp entries per row), Y0 = e // gp, X0 = e % gp."""
    img = np.asarray(img).astype(np.int64)
    pcells, kcount = np.asarray(pcells), np.asarray(kcount)
    ar = stride * np.arange(nbt)
    out = np.zeros((len(kcount), nbt, nbt), dtype=np.int64)
    for it in range(len(kcount)):
        e = pcells[it, :int(kcount[it])].astype(np.int64) >> 2
        Y0, X0 = e // gp, e % gp
        out[it] = img[Y0[:, None, None] + ar[None, :, None], X0[:, None, None] + ar[None, None, :]].sum(axis=0)
    return out


def tile_bounds(img, pcells, kcount, pmax, cost_scale, gp, nbt, image_scale=16777216.0):
    """U[it, by, bx] = (-((sum_k img[Y0_k + by, X0_k + bx]) * image_scale * (1 / cost_scale)) + pmax[by, bx]) + 1e-9 in the
    kernel's own association; image_scale is what one unit of the image stands for in field costs: 2^24 for the byte image.
    img: [rows >= gp, pitch >= gp]; pcells: [ntheta, kmax]; kcount: [ntheta]; pmax: [nbt, >= nbt] (Slam2dLevel.tile_pmax of one
    particle; its padding columns are not read)."""
    pmax = np.asarray(pmax, dtype=np.float64)[:nbt, :nbt]
    inv = 1.0 / cost_scale
    sums = tile_sums(img, pcells, kcount, gp, nbt)
    return (-((sums.astype(np.float64) * image_scale) * inv) + pmax[None]) + 1e-9


def host_bounds(lv, p):
    """The tile bounds of particle p as k_bound_lds takes them, from the byte image as it lies in memory AFTER the scan:
    U = (-((sum of the image bytes at the angle's cells, shifted to the tile) * 2^24 / scale) + tile_pmax) + 1e-9."""
    gp, nbt = 4 * lv.tmax, (lv.nx + 3) // 4
    return tile_bounds(lv.t["gmin2b"][p].cpu().numpy(), lv.t["pcells"][p].cpu().numpy(), lv.t["kcount"][p].cpu().numpy(),
                       lv.t["tile_pmax"][p].cpu().numpy(), lv.c.cost_scale, gp, nbt)


def tile_max(cube, nx, nbt, size=4):
    """Per size x size pose tile (4 x 4; 8 x 8 for level 1 of the two-level bounds) of a [ntheta, nx, nx] score cube: (the
    largest non-NaN score [ntheta, nbt, nbt] -- -inf for a tile of NaNs only --, whether the tile holds a NaN [ntheta, nbt,
    nbt]).  The partial tiles at the right and bottom edge (nx < size nbt) take their valid poses only."""
    cube = np.asarray(cube, dtype=np.float64).reshape(-1, nx, nx)
    assert size * (nbt - 1) < nx <= size * nbt
    n = size * nbt
    nan = np.isnan(cube)
    fill = np.full((cube.shape[0], n, n), -np.inf)
    fill[:, :nx, :nx] = np.where(nan, -np.inf, cube)
    has = np.zeros((cube.shape[0], n, n), dtype=bool)
    has[:, :nx, :nx] = nan
    mx = fill.reshape(-1, nbt, size, nbt, size).max(axis=(2, 4))
    return mx, has.reshape(-1, nbt, size, nbt, size).any(axis=(2, 4))


# ---------------------------------------------------------------------------------------------------------------------
# the other bound kernels: 32-bit minima, two levels, angle planes
# ---------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def min3x3(g):
    """min(g[Y..Y+2][X..X+2]) with the indices clamped to the image, as gmin2_entry takes v3."""
    n0, n1 = g.shape
    iy = np.minimum(np.arange(n0)[:, None] + np.arange(3)[None, :], n0 - 1)            # [n0, 3]
    ix = np.minimum(np.arange(n1)[:, None] + np.arange(3)[None, :], n1 - 1)
    return g[iy[:, None, :, None], ix[None, :, None, :]].min(axis=(2, 3))


def unphase(gmin3d, gp):
    """Slam2dLevel.gmin3d of one particle -- four phase planes decimated by two, entry (Y, X) at
    [(Y & 1) << 1 | (X & 1)][Y >> 1][X >> 1] -- back to a [gp, gp] image."""
    hp = gp // 2
    pl = np.asarray(gmin3d).reshape(4, hp, hp)
    Y, X = np.meshgrid(np.arange(gp), np.arange(gp), indexing="ij")
    return pl[((Y & 1) << 1) | (X & 1), Y >> 1, X >> 1]


def decode_p3(p3cells, gp):
    """(Y0, X0) of entries of Slam2dLevel.p3cells: byte offsets into the phase planes of gmin3d,
    ((((Y0 & 1) << 1 | (X0 & 1)) * hp + (Y0 >> 1)) * hp + (X0 >> 1)) * 4 with hp = gp / 2."""
    hp = gp // 2
    v = np.asarray(p3cells).astype(np.int64) >> 2
    ph, rest = v // (hp * hp), v % (hp * hp)
    return 2 * (rest // hp) + (ph >> 1), 2 * (rest % hp) + (ph & 1)


def tile_bounds32(gmin2, pcells, kcount, pmax, cost_scale, gp, nbt):
    """k_bound's bounds (children_bounds and k_seed take the same expression) from the 32-bit minima, one unit = 2^12 costs:
    U[it, by, bx] = (-((sum_k gmin2[Y0_k + by, X0_k + bx]) * 4096.0 * (1.0 / cost_scale)) + pmax[by, bx]) + 1e-9."""
    return tile_bounds(gmin2, pcells, kcount, pmax, cost_scale, gp, nbt, image_scale=4096.0)


def tile1_bounds(g3, pcells, kcount, pmax, cost_scale, gp, nx):
    """k_bound1's bounds of the 8 x 8-pose tiles, [ntheta, 8, 8], from g3 = unphase(gmin3d): for R, C1 < nb1 = cdiv(nx, 8)
    U1[it, R, C1] = (-((sum_k g3[Y0_k + 2 R, X0_k + 2 C1]) * 4096.0 * (1.0 / cost_scale)) + pm1[R, C1]) + 1e-9, pm1 the largest
    tile_pmax of the children (2 R + a, 2 C1 + b), a, b in {0, 1}, inside nbt = cdiv(nx, 4); every other entry -inf."""
    nb1, nbt = _cdiv(nx, 8), _cdiv(nx, 4)
    pm = np.full((2 * nb1, 2 * nb1), -np.inf)
    pm[:nbt, :nbt] = np.asarray(pmax, dtype=np.float64)[:nbt, :nbt]
    pm1 = pm.reshape(nb1, 2, nb1, 2).max(axis=(1, 3))
    sums = tile_sums(g3, pcells, kcount, gp, nb1, stride=2)
    out = np.full((len(kcount), 8, 8), -np.inf)
    out[:, :nb1, :nb1] = (-((sums.astype(np.float64) * 4096.0) * (1.0 / cost_scale)) + pm1[None]) + 1e-9
    return out


def angle_bounds(gmin2, pcells, kcount, prior, cost_scale, gp, fine):
    """k_abound's bound of every angle plane, [ntheta]: U[it] = (-((sum_k gmin2[Y0_k, X0_k]) * 4096.0 / cost_scale) + pmx) + 1e-9
    -- a division where the tile kernels multiply by the reciprocal --, pmx = 0 on a fine level, else the largest rv + thetaWeight
    of the plane (prior: [2, npose]), +inf if one of them is NaN."""
    pmx = 0.0
    if not fine:
        v = np.asarray(prior, dtype=np.float64)
        v = v[0].reshape(-1) + v[1].reshape(-1)
        pmx = np.inf if np.isnan(v).any() else float(v.max())
    sums = tile_sums(gmin2, pcells, kcount, gp, 1)[:, 0, 0]
    return (-((sums.astype(np.float64) * 4096.0) / cost_scale) + pmx) + 1e-9


_SIGN = np.uint64(1 << 63)


def order_bits(v):
    """The monotone map double -> uint64 of csrc/slam2d.hip (a maximum of the keys is a maximum of the values)."""
    b = np.asarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b & _SIGN, ~b, b | _SIGN)


def unorder_bits(k):
    k = np.asarray(k).astype(np.uint64)
    return np.where(k & _SIGN, k & ~_SIGN, ~k).view(np.float64)


def _tile_best(cube_it, nx, ty, tx):
    """Largest non-NaN score of the valid poses of 4 x 4 tile (ty, tx) of one plane; -inf if there is none."""
    t = np.asarray(cube_it, dtype=np.float64).reshape(nx, nx)[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4]
    t = t[~np.isnan(t)]
    return float(t.max()) if t.size else -np.inf


def replay_two_level(U1, U2, pmax, cube_exact, nx):
    """What k_bound1 -> k_seed -> k_bound2 are written to leave for one particle: (seed_key, seed_best, final_best).
    U1: tile1_bounds [ntheta, 8, 8]; U2: tile_bounds32 of the WHOLE cube [ntheta, nbt, nbt]; pmax: tile_pmax (read only to
    check U2's infinities against it); cube_exact: the brute-force twin's cube.

    seed_key (k_bound1): per angle the best level-1 tile among R, C1 < nb1 -- the largest bound, the lowest tile index
    R * 8 + C1 on ties -- contributes (order_bits(v) & ~0x3FFF) | (it << 6 | tile) if v is finite; the key is the maximum, 0 if
    no angle contributes.  seed_best (k_seed): of the key's tile the best child inside nbt by U2 (c = 0..3, the first strict
    maximum), the largest non-NaN exact score of its valid poses; -inf without a key or without such a pose.
    final_best (k_bound2): with thr0 = seed_best - 30 every angle's candidate is the first strict maximum of U2 over the
    children of the level-1 tiles with U1 >= thr0 (tiles ascending, cc = 0..3; a child outside the cube counts as -inf), and
    final_best = max(seed_best, the candidates' largest non-NaN exact scores).

    Why final_best does not depend on the timing although every k_bound2 wave reads bnb_best while other waves raise it: a
    child's bound never exceeds its parent's (gmin3d's minimum runs over a superset of the blocks, pm1 over a superset of the
    priors, and every operation of the expression is monotone), and an exact score never exceeds its tile's bound.  A wave that
    read a fresher, higher value b than seed_best skips only tiles with U1 < b - 30 and seeds with U2 < b; whatever it then
    scores in place of the loosest threshold's candidate has a bound below that candidate's, hence below b - 30.  So every score
    that a fresher threshold removes from or adds to the maximum lies below a value bnb_best had already reached: the result is
    what the loosest threshold gives."""
    U1 = np.asarray(U1, dtype=np.float64).reshape(-1, 8, 8)
    ntheta = U1.shape[0]
    nb1, nbt = _cdiv(nx, 8), _cdiv(nx, 4)
    U2 = np.asarray(U2, dtype=np.float64)[:, :nbt, :nbt]
    pm = np.asarray(pmax, dtype=np.float64)[:nbt, :nbt]
    assert U2.shape == (ntheta, nbt, nbt) and (np.isposinf(U2) == np.isposinf(pm)[None]).all() and (np.isneginf(U2) == np.isneginf(pm)[None]).all()
    cube = np.asarray(cube_exact, dtype=np.float64).reshape(ntheta, nx, nx)

    def child(R, Cx, c):
        cy, cx = 2 * R + (c >> 1), 2 * Cx + (c & 1)
        return (cy, cx) if cy < nbt and cx < nbt else None

    key = 0
    for it in range(ntheta):
        v, tile = -np.inf, None
        for R in range(nb1):
            for C1 in range(nb1):
                if tile is None or U1[it, R, C1] > v:
                    v, tile = U1[it, R, C1], R * 8 + C1
        if np.isfinite(v):
            key = max(key, (int(order_bits(v)) & ~0x3FFF) | (it << 6) | tile)
    seed_best = -np.inf
    if key:
        it, R, Cx = (key >> 6) & 0xFF, (key & 63) >> 3, key & 7
        best, ub = None, -np.inf
        for c in range(4):
            yx = child(R, Cx, c)
            if yx is not None and (best is None or U2[it][yx] > ub):
                best, ub = yx, U2[it][yx]
        if best is not None:
            seed_best = _tile_best(cube[it], nx, *best)
    final_best = seed_best
    thr0 = seed_best - BNB_MARGIN
    for it in range(ntheta):
        cand, ub = None, -np.inf
        for t1 in range(64):
            R, Cx = t1 >> 3, t1 & 7
            if not U1[it, R, Cx] >= thr0:
                continue
            for cc in range(4):
                yx = child(R, Cx, cc)
                if yx is not None and U2[it][yx] > ub:
                    cand, ub = yx, U2[it][yx]
        if cand is not None:
            final_best = max(final_best, _tile_best(cube[it], nx, *cand))
    return np.uint64(key), seed_best, final_best


def replay_angle(U, cube_exact_planes):
    """What k_abound and k_aseed leave for one particle: (seed_key, seed plane, best).  seed_key: the maximum over the angles of
    (order_bits(U[it]) & ~0x3FFF) | it, a +inf bound entering as order_bits(1e300), a -inf bound not at all; 0 without any.
    The seed plane is the key's angle; best its largest exact score -- -inf if the plane holds a NaN or the key is 0."""
    U = np.asarray(U, dtype=np.float64)
    planes = np.asarray(cube_exact_planes, dtype=np.float64).reshape(len(U), -1)
    key = 0
    for it, u in enumerate(U):
        if u == -np.inf:
            continue
        key = max(key, (int(order_bits(1e300 if u == np.inf else u)) & ~0x3FFF) | it)
    if not key:
        return np.uint64(0), None, -np.inf
    it = key & 0x3FFF
    return np.uint64(key), it, (-np.inf if np.isnan(planes[it]).any() else float(planes[it].max()))
