"""Inputs at which the loops of K13 (k13_volume_diameters.hip) take more than one trip (test_volume_diameter_trip_cases.py
on the CPU, test_gpu_volume_diameter_trips.py on the GPU; NumPy only, not a conftest). Every other K13 input of the suite
has at most 2257 rows in a lesion's box, where every loop below takes one trip. Every comparison made with these inputs is
== on integers; test_volume_diameter_trip_cases.py asserts each property below from the golden model and the inputs.

The work list of vd_pairs_kernel. Lesion r (K10's order) has nt[r] tiles of TILE_ROWS row slots of its bounding box
(slot = (z - z0) * ny + (y - y0)); tile pair (li, lj) is the SPLIT items first[r] + (li * nt[r] + lj) * SPLIT + part of the
list, first[r] = sum of nt^2 * SPLIT over the lesions before r. The grid is min(ceil(N * ntmax^2 * SPLIT / THREADS),
PAIR_GRID) with ntmax the tiles of the VOLUME's h * d rows; a round gives every thread of every workgroup one item, so item
i is looked at in round i // (THREADS * grid), and a second round exists only above 65 536 tile pairs. A voxel pair a <= b
(raster order) is compared in the tile pair (tile of a's row, tile of b's row) only.

Which case turns which loop (all 130 x 300 x 8 cases have ONE lesion at N = 1, at connectivity 6 and 26):
  t_bar      130 x 300 x 8: a bar along z at y = 150, a bar along y in the last plane, a short bar along x at (y 290, z 129).
             Box 300 x 130 = 39 000 rows, 305 tiles, 372 100 items, grid 1024, TWO ROUNDS of the pairs loop; 20 chunks of
             vd_bound_kernel merged by the plane bound's first workgroup; ny = 300: 5 trips of the plane bound's row loop
             and 2 of vd_final_kernel's. At (1000, 1000, 1000) the major and the axial pair are (2, 0, 129) - (2, 299, 129),
             tile pair (302, 304): found in round 1 ONLY, so a better pair of round 1 has to replace round 0's. At
             (977, 1020, 3300) the major pair (2, 150, 0) - (2, 0, 129) is in round 0 and has to survive round 1, while the
             axial pair stays in round 1. The perpendicular ends at (6, 290): y >= 256, the final kernel's second trip.
  two_bars   130 x 300 x 8: the bar along z with a bar along y in the first AND the last plane. The axial maximum 299 * uy
             is attained exactly twice, in plane 0 (round 0) and in plane 129 (round 1): a tie ACROSS ROUNDS, plane 0 has to
             stay. The major diameter ties between the two diagonals, found by different workgroups of round 0:
             (2, 0, 0) - (2, 299, 129) has to win the reduction over the partial slots.
  sheets     70 x 64 x 128, N = 64: 64 L-shaped lesions in the planes x = 0, 2, ... 126 (apart at 26 too), each a bar along
             y in plane 0 and a bar along z at y = 0 of 70 - (i % 5) voxels: 33 to 35 tiles each, 299 896 items, two rounds.
             Lesions whose items lie wholly in round 0, one that straddles the boundary and several wholly in round 1; the
             binary search over first[] at count = 64; the rank order is not the raster order; vd_final_kernel's loop
             over 1024 partial slots at nmax = 64. At N = 16 the grid is 307 and one round suffices: the control, and in
             the stale-buffer order a smaller grid on the slots a larger one wrote.
  ring       130 x 300 x 8: an elliptic annulus in (y, z), two voxels thick in x: 3704 voxels, box 280 x 120 = 33 600 rows,
             263 tiles, 276 676 items, two rounds, 17 bound chunks. At (1000, 600, 1400) it is a circle of radius 84 mm:
             antipodal tile pairs all come near the maximum, so the bound keeps hundreds of tile pairs (nine times as
             many as at 1 mm isotropic) and a workgroup's survivor list holds several entries at once; on t_bar one
             tile pair survives. Its winners lie in round 0 (round 1 holds the pairs of the last 14 tiles with
             each other), so round 1 must add nothing wrong; with brute_force both rounds compare every occupied pair.
The loops with one thread or workgroup per element (init, rows, tiles) have no trips to turn; vd_bound_kernel's row loop
takes 8 trips in every full chunk here."""
import functools

import numpy as np

# include/nm03/volume_diameters_core.h
TILE_ROWS = 128        # vdcore::kTileRows: row slots per tile
# src/kernels/k13_volume_diameters.hip
SPLIT = 4              # kVdSplit: items per tile pair
THREADS = 256          # kVmThreads (volume_measure_util.h): threads of a pairs workgroup, one item each per round
PAIR_GRID = 1024       # kVdPairGrid: workgroups of the pairs launch, at most
BOUND_ROWS = 2048      # kVdBoundRows: rows per workgroup of vd_bound_kernel
FINAL_THREADS = 256    # kVdFinalThreads: the stride of vd_final_kernel's loops
PLANE_STRIDE = 64      # vd_plane_bound_kernel: a wave per plane, y += 64

ISO = (1000, 1000, 1000)
ANISO = (977, 1020, 3300)
CIRCULAR = (1000, 600, 1400)  # the ring's radii 140 (y) and 60 (z) both become 84 mm
BAR_SHAPE = (130, 300, 8)     # d, h, w
SHEETS_SHAPE = (70, 64, 128)


def _ro(m):
    m = np.ascontiguousarray(m, dtype=np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def t_bar():
    m = np.zeros(BAR_SHAPE, np.uint8)
    m[:, 150, 2] = 1
    m[129, :, 2] = 1
    m[129, 290, 2:7] = 1
    return _ro(m)


@functools.lru_cache(maxsize=None)
def two_bars():
    m = np.zeros(BAR_SHAPE, np.uint8)
    m[:, 150, 2] = 1
    m[0, :, 2] = 1
    m[129, :, 2] = 1
    return _ro(m)


@functools.lru_cache(maxsize=None)
def sheets():
    m = np.zeros(SHEETS_SHAPE, np.uint8)
    for i in range(64):
        m[0, :, 2 * i] = 1
        m[:70 - (i % 5), 0, 2 * i] = 1
    return _ro(m)


@functools.lru_cache(maxsize=None)
def ring():
    z, y, x = np.ogrid[:130, :300, :8]
    q = ((y - 149.5) / 140.0) ** 2 + ((z - 64.5) / 60.0) ** 2
    return _ro((q >= 0.93) & (q <= 1.0) & (x >= 3) & (x <= 4))


# (id, mask builder, N, spacings): volume_diameter_cases.SPACINGS, for the ring after the spacing that makes it a circle
SPACINGS = (ISO, (500, 500, 5000), ANISO)
CASES = (
    ("t_bar", t_bar, 1, SPACINGS),
    ("two_bars", two_bars, 1, SPACINGS),
    ("sheets-64", sheets, 64, SPACINGS),
    ("sheets-16", sheets, 16, SPACINGS),
    ("ring", ring, 1, (CIRCULAR,) + SPACINGS),
)


SHEETS_LATE_RANKS = tuple(range(56, 64))  # the lesions of sheets-64 whose items lie wholly in round 1 (55 straddles)


def case(name):
    """(mask, N, spacings) of a case."""
    return next((build(), n, ums) for cid, build, n, ums in CASES if cid == name)


# ---- the lesions of a mask, in plain Python ---------------------------------------------------------------
def lesions(mask, n, conn):
    """The n largest components of `mask` at connectivity 6 or 26 in measure_volume_lesions' order (voxels descending, a
    tie to the first voxel in raster order) → list of dicts: voxels, first [x, y, z], bbox [x0, y0, z0, x1, y1, z1] and
    zyx, the voxels as an int array [voxels, 3] in raster order. A flood fill over the set voxels: for masks of some
    thousand voxels."""
    steps = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
             if (dz, dy, dx) != (0, 0, 0) and (conn == 26 or abs(dz) + abs(dy) + abs(dx) == 1)]
    assert conn in (6, 26) and len(steps) == conn
    todo = {tuple(v): None for v in np.argwhere(np.asarray(mask) != 0).tolist()}  # raster order
    out = []
    while todo:
        seed = next(iter(todo))  # the first voxel left in raster order
        del todo[seed]
        comp, stack = [seed], [seed]
        while stack:
            z, y, x = stack.pop()
            for dz, dy, dx in steps:
                v = (z + dz, y + dy, x + dx)
                if v in todo:
                    del todo[v]
                    comp.append(v)
                    stack.append(v)
        zyx = np.array(sorted(comp), np.int64)
        lo, hi = zyx.min(axis=0), zyx.max(axis=0)
        out.append({"voxels": len(comp), "first": [seed[2], seed[1], seed[0]],
                    "bbox": [int(lo[2]), int(lo[1]), int(lo[0]), int(hi[2]), int(hi[1]), int(hi[0])], "zyx": zyx})
    out.sort(key=lambda l: -l["voxels"])  # stable: the components were met in the raster order of their first voxels
    return out[:n]


# ---- the work list of the pairs launch ----------------------------------------------------------------------
def box_rows(bbox):
    """(ny, nz) of a bbox [x0, y0, z0, x1, y1, z1]."""
    return bbox[4] - bbox[1] + 1, bbox[5] - bbox[2] + 1


def row_slot(bbox, y, z):
    """vdcore::Rows: the slot of row (z, y) among the rows of the lesion's bounding box."""
    ny, nz = box_rows(bbox)
    assert bbox[1] <= y <= bbox[4] and bbox[2] <= z <= bbox[5]
    return (z - bbox[2]) * ny + (y - bbox[1])


def _ceil(a, b):
    return (a + b - 1) // b


def plan(shape, bboxes, n):
    """The pairs launch of a [d, h, w] volume whose chosen lesions have `bboxes` (in order) at max_lesions = n: rows, nt,
    first (len + 1 entries, the last one = total) and bound_chunks per lesion; ntmax, total, grid, per_round, rounds."""
    d, h, w = shape
    rows = [ny * nz for ny, nz in map(box_rows, bboxes)]
    nt = [_ceil(r, TILE_ROWS) for r in rows]
    first = [0]
    for t in nt:
        first.append(first[-1] + t * t * SPLIT)
    ntmax = _ceil(h * d, TILE_ROWS)
    grid = min(_ceil(n * ntmax * ntmax * SPLIT, THREADS), PAIR_GRID)
    per_round = THREADS * grid
    return dict(rows=rows, nt=nt, first=first, bound_chunks=[_ceil(r, BOUND_ROWS) for r in rows], ntmax=ntmax,
                total=first[-1], grid=grid, per_round=per_round, rounds=_ceil(first[-1], per_round))


def pair_tiles(bbox, a, b):
    """(li, lj), li <= lj: the tiles of the rows of voxels a and b, each (x, y, z)."""
    ta, tb = (row_slot(bbox, v[1], v[2]) // TILE_ROWS for v in (a, b))
    return min(ta, tb), max(ta, tb)


def pair_round(p, r, bbox, a, b):
    """The round of the pairs loop in which the voxels a and b (each (x, y, z)) of lesion r are compared. The SPLIT items
    of a tile pair lie in one round, per_round being a multiple of SPLIT."""
    li, lj = pair_tiles(bbox, a, b)
    assert p["per_round"] % SPLIT == 0
    return (p["first"][r] + (li * p["nt"][r] + lj) * SPLIT) // p["per_round"]


def pair_workgroups(p, r, bbox, a, b):
    """The workgroups (item mod grid) that hold the SPLIT items of the tile pair of the voxels a and b of lesion r."""
    li, lj = pair_tiles(bbox, a, b)
    item = p["first"][r] + (li * p["nt"][r] + lj) * SPLIT
    return {(item + part) % p["grid"] for part in range(SPLIT)}


def round_matrix(p, r, les, bbox=None):
    """[voxels, voxels] array: pair_round of every pair of voxels of lesion r (an entry of lesions())."""
    bbox = bbox or les["bbox"]
    ny, _ = box_rows(bbox)
    tile = ((les["zyx"][:, 0] - bbox[2]) * ny + (les["zyx"][:, 1] - bbox[1])) // TILE_ROWS
    li, lj = np.minimum(tile[:, None], tile[None, :]), np.maximum(tile[:, None], tile[None, :])
    return (p["first"][r] + (li * p["nt"][r] + lj) * SPLIT) // p["per_round"]


def maximal_pairs(les, um, axial=False, where=None):
    """(d2, pairs): the largest squared distance in um^2 between two voxels of a lesion (an entry of lesions()) — inside
    one plane when `axial`, among the pairs of the bool matrix `where` when given — and every pair ((x, y, z), (x, y, z)),
    a before b in raster order, that attains it, in the raster order of (a, b): pairs[0] is the one the tie rule asks
    for. All pairs at once: for lesions of some hundred voxels."""
    zyx = les["zyx"]
    assert len(zyx) <= 2000
    u = np.array([um[2], um[1], um[0]], np.int64)
    diff = (zyx[:, None, :] - zyx[None, :, :]) * u
    d2 = (diff * diff).sum(axis=2)
    ok = np.triu(np.ones(d2.shape, bool))
    if axial:
        ok &= zyx[:, None, 0] == zyx[None, :, 0]
    if where is not None:
        ok &= where
    best = int(d2[ok].max())
    ia, ib = np.nonzero(ok & (d2 == best))  # row-major: ordered by a, then b
    return best, [(tuple(int(v) for v in zyx[i][::-1]), tuple(int(v) for v in zyx[j][::-1])) for i, j in zip(ia, ib)]


def lesion_rounds(p, r):
    """(round of the lesion's first item, round of its last one)."""
    return p["first"][r] // p["per_round"], (p["first"][r + 1] - 1) // p["per_round"]


def occupied_tile_pairs(les, bbox=None):
    """The tile pairs (I <= J) of a lesion (an entry of lesions()) both of whose tiles hold a voxel: those the bound can
    skip or keep (a pair with an empty tile is no work either way)."""
    bbox = bbox or les["bbox"]
    ny, _ = box_rows(bbox)
    slots = (les["zyx"][:, 0] - bbox[2]) * ny + (les["zyx"][:, 1] - bbox[1])
    t = len(np.unique(slots // TILE_ROWS))
    return t * (t + 1) // 2
