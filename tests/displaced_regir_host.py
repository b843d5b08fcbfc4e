"""numpy restatements for the ReGIR-over-a-displaced-set tests: the cell of a position (regir_cell_index, csrc/pathtrace.hip, in
float32: divide, saturating convert, clamp), the classification "within eps of an inner cell face", and the largest step the ray-origin
offset (oracle/orc_shared.h offsetRayOrigin) can take at a coordinate of a given size."""
import numpy as np

F32 = np.float32


def _f2u_sat(x):
    """gm_math.hip.h f2u_sat: NaN and everything <= 0 give 0, >= 2^32 gives 0xFFFFFFFF, truncation inside."""
    x = np.asarray(x, F32)
    out = np.zeros(x.shape, np.uint32)
    inside = (x > 0) & (x < F32(4294967296.0))
    out[inside] = x[inside].astype(np.uint64).astype(np.uint32)       # (float -> uint32 directly is undefined above 2^31 in C)
    out[x >= F32(4294967296.0)] = 0xFFFFFFFF
    return out


def cell_coords(pos, origin, cell_size, dims):
    """uint32[n, 3]: the clamped integer cell coordinates of float32 positions pos[n, 3]."""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    origin, cell_size = np.asarray(origin, F32), np.asarray(cell_size, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = ((pos - origin) / cell_size).astype(F32)
    i = _f2u_sat(r)
    return np.minimum(i, np.asarray(dims, np.uint32) - np.uint32(1))


def cell_index(pos, origin, cell_size, dims):
    """regir_cell_index: iz * dimX * dimY + iy * dimX + ix."""
    c = cell_coords(pos, origin, cell_size, dims).astype(np.uint64)
    return (c[:, 2] * dims[0] * dims[1] + c[:, 1] * dims[0] + c[:, 0]).astype(np.uint32)


def near_inner_face(pos, origin, cell_size, dims, eps):
    """bool[n]: the position lies within eps (world units) of a cell face that separates two cells of the grid.  The outer faces (index
    0 and dims[k]) do not count: a position beyond them clamps to the border cell on either side of them."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    origin, cell_size = np.asarray(origin, F32).astype(np.float64), np.asarray(cell_size, F32).astype(np.float64)
    near = np.zeros(len(pos), bool)
    for k in range(3):
        r = (pos[:, k] - origin[k]) / cell_size[k]
        j = np.rint(r)                                   # the nearest face index
        inner = (j >= 1) & (j <= dims[k] - 1)
        near |= inner & (np.abs(r - j) * cell_size[k] <= eps)
    return near


def neighbour_cells(pos, origin, cell_size, dims, eps):
    """For positions within eps of inner faces: every cell a point within eps (per axis) of the position can fall into, as a list of
    uint32 arrays (one per combination of -eps / +eps per axis, duplicates included)."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    out = []
    for sx in (-eps, eps):
        for sy in (-eps, eps):
            for sz in (-eps, eps):
                out.append(cell_index((pos + (sx, sy, sz)).astype(F32), origin, cell_size, dims))
    return out


def cell_count_bounds(pos, origin, cell_size, dims, eps):
    """(lo, hi, near): per cell, the number of positions surely in it (farther than eps from every inner face) and the number that may be
    in it (those, plus every position within eps of an inner face of the cell, counted for each cell it can fall into)."""
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    pos = np.asarray(pos, F32).reshape(-1, 3)
    near = near_inner_face(pos, origin, cell_size, dims, eps)
    lo = np.bincount(cell_index(pos[~near], origin, cell_size, dims), minlength=cells).astype(np.int64)
    hi = lo.copy()
    if near.any():
        cand = np.stack(neighbour_cells(pos[near], origin, cell_size, dims, eps), axis=1)
        for row in cand:
            hi[np.unique(row)] += 1
    return lo, hi, near


def max_offset_step(largest_coordinate):
    """The largest distance offsetRayOrigin moves one coordinate of a point whose coordinates are at most `largest_coordinate` in
    size: 1 / 65536 times a normal component (|p| < 1 / 32), or 256 steps of the float's integer representation away from zero, which
    are units in the last place of p or, past a power of two, of the binade above (twice as large)."""
    m = F32(abs(largest_coordinate))
    return max(1.0 / 65536.0, 256.0 * 2.0 * float(np.spacing(m)))
