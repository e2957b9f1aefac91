"""The definition of the tile bounds of branch and bound (include/slam2d.h, "Branch and bound") in NumPy, for the tests: what
k_bound_lds must leave in Slam2dLevel.bounds, from the byte image of the bound minima (Slam2dLevel.gmin2b) and the cell lists
as they lie in memory, by a plain sum over every cell of the list -- no runs, no batches, no padding; and what a bound has to
dominate: the largest score of each 4 x 4 pose tile of a cube."""
import numpy as np


def min2x2(g):
    """min(g[Y..Y+1][X..X+1]) with the indices clamped to the image, as the device takes it."""
    gy = np.concatenate([g[1:], g[-1:]], axis=0)
    m = np.minimum(g, gy)
    mx = np.concatenate([m[:, 1:], m[:, -1:]], axis=1)
    return np.minimum(m, mx)


def tile_sums(img, pcells, kcount, gp, nbt):
    """S[it, by, bx] = sum over the cells k < kcount[it] of img[Y0_k + by, X0_k + bx] in int64, with e = pcells >> 2 (pcells
    holds byte offsets into the 32-bit image of gp entries per row), Y0 = e // gp, X0 = e % gp."""
    img = np.asarray(img).astype(np.int64)
    pcells, kcount = np.asarray(pcells), np.asarray(kcount)
    ar = np.arange(nbt)
    out = np.zeros((len(kcount), nbt, nbt), dtype=np.int64)
    for it in range(len(kcount)):
        e = pcells[it, :int(kcount[it])].astype(np.int64) >> 2
        Y0, X0 = e // gp, e % gp
        out[it] = img[Y0[:, None, None] + ar[None, :, None], X0[:, None, None] + ar[None, None, :]].sum(axis=0)
    return out


def tile_bounds(img, pcells, kcount, pmax, cost_scale, gp, nbt):
    """U[it, by, bx] = (-((sum_k img[Y0_k + by, X0_k + bx]) * 2^24 * (1 / cost_scale)) + pmax[by, bx]) + 1e-9 in the kernel's
    own association.  img: [rows >= gp, pitch >= gp] bytes; pcells: [ntheta, kmax]; kcount: [ntheta]; pmax: [nbt, >= nbt]
    (Slam2dLevel.tile_pmax of one particle; its padding columns are not read)."""
    pmax = np.asarray(pmax, dtype=np.float64)[:nbt, :nbt]
    inv = 1.0 / cost_scale
    sums = tile_sums(img, pcells, kcount, gp, nbt)
    return (-((sums.astype(np.float64) * 16777216.0) * inv) + pmax[None]) + 1e-9


def host_bounds(lv, p):
    """The tile bounds of particle p as k_bound_lds takes them, from the byte image as it lies in memory AFTER the scan:
    U = (-((sum of the image bytes at the angle's cells, shifted to the tile) * 2^24 / scale) + tile_pmax) + 1e-9."""
    gp, nbt = 4 * lv.tmax, (lv.nx + 3) // 4
    return tile_bounds(lv.t["gmin2b"][p].cpu().numpy(), lv.t["pcells"][p].cpu().numpy(), lv.t["kcount"][p].cpu().numpy(),
                       lv.t["tile_pmax"][p].cpu().numpy(), lv.c.cost_scale, gp, nbt)


def tile_max(cube, nx, nbt):
    """Per 4 x 4 pose tile of a [ntheta, nx, nx] score cube: (the largest non-NaN score [ntheta, nbt, nbt] -- -inf for a tile
    of NaNs only --, whether the tile holds a NaN [ntheta, nbt, nbt]).  The partial tiles at the right and bottom edge
    (nx < 4 nbt) take their valid poses only."""
    cube = np.asarray(cube, dtype=np.float64).reshape(-1, nx, nx)
    assert 4 * (nbt - 1) < nx <= 4 * nbt
    n = 4 * nbt
    nan = np.isnan(cube)
    fill = np.full((cube.shape[0], n, n), -np.inf)
    fill[:, :nx, :nx] = np.where(nan, -np.inf, cube)
    has = np.zeros((cube.shape[0], n, n), dtype=bool)
    has[:, :nx, :nx] = nan
    mx = fill.reshape(-1, nbt, 4, nbt, 4).max(axis=(2, 4))
    return mx, has.reshape(-1, nbt, 4, nbt, 4).any(axis=(2, 4))
