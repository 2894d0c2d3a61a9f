"""Inputs of the 3D-mode tests (test_volume_cases.py on the CPU, test_gpu_volume.py on the GPU; not a
conftest). Everything here is NumPy (+ scipy.ndimage inside emulate_sweeps) on the CPU.

  * maze: a one-voxel path that turns between y and z at every cell. The plane sweeps of K5 advance
    about one segment of it per sweep, far beyond any multiple of w + h + d.
  * staircase: a one-voxel path whose steps cycle through x, y, z (a 3D billiard trajectory).
  * emulate_sweeps: a model of the alternating xy / xz plane sweeps, to count the sweeps such a
    region needs under three plane orders.
  * serpentine_volume: raw planes whose band climbs through all of z, crosses over and comes back.
  * SHAPE_CASES / DILATION_RANGE / border_mask: random bands and masks at the shapes where the 3D
    kernels change path (single planes, word edges, d as the long side, the LDS / global switch).
"""
import numpy as np


# ---- tortuous regions ---------------------------------------------------------------------------
def _carve(band, cells):
    """Sets every cell (x, y, z) of a lattice path (cells at even voxel coordinates) and the voxel
    between consecutive cells."""
    px = None
    for c in cells:
        x, y, z = 2 * c[0], 2 * c[1], 2 * c[2]
        band[z, y, x] = 1
        if px is not None:
            band[(z + px[2]) // 2, (y + px[1]) // 2, (x + px[0]) // 2] = 1
        px = (x, y, z)


def maze(w, h, d, layers):
    """(band uint8 [d, h, w], seed (x, y, z), ncells): `layers` x-layers of a path over the cells
    (2i, 2j, 2k). J = (h + 1) // 2 rounded down to even rows of cells, K = (d + 1) // 2 rounded down
    to odd. A layer's path visits the strips s = 0..J/2 − 1 (two rows of cells each) with k ascending
    on even strips and descending on odd ones; at each k it visits (cur, k) then (oth, k) and swaps
    the two, starting with cur, oth = 2s, 2s + 1 — so inside a strip every step is a turn between y
    and z. Even layers run the path forward, odd layers backward; consecutive layers join by one x
    step. Under 6-connectivity the band is exactly the path."""
    J = ((h + 1) // 2) & ~1
    K = (d + 1) // 2
    K -= 1 - (K & 1)
    assert J >= 2 and K >= 1 and 1 <= layers <= (w + 1) // 2
    path = []
    for s in range(J // 2):
        cur, oth = 2 * s, 2 * s + 1
        for k in (range(K) if s % 2 == 0 else range(K - 1, -1, -1)):
            path += [(cur, k), (oth, k)]
            cur, oth = oth, cur
    cells = []
    for i in range(layers):
        cells += [(i, j, k) for (j, k) in (path if i % 2 == 0 else path[::-1])]
    band = np.zeros((d, h, w), np.uint8)
    _carve(band, cells)
    return band, (0, 0, 0), len(cells)


def staircase(w, h, d):
    """(band uint8 [d, h, w], seed, ncells): a path over the cells (2i, 2j, 2k) whose steps cycle
    through the axes x, y, z — every step turns, and three consecutive steps use all three axes. Each
    axis keeps its direction until the next cell on it is outside the lattice or already visited,
    then reverses (a billiard trajectory); the path ends where no axis can move."""
    dims = ((w + 1) // 2, (h + 1) // 2, (d + 1) // 2)
    pos, step = [0, 0, 0], [1, 1, 1]
    cells, seen = [(0, 0, 0)], {(0, 0, 0)}
    axis, blocked = 0, 0
    while blocked < 3:
        moved = False
        for sgn in (step[axis], -step[axis]):
            q = list(pos)
            q[axis] += sgn
            if 0 <= q[axis] < dims[axis] and tuple(q) not in seen:
                pos, step[axis], moved = q, sgn, True
                cells.append(tuple(q))
                seen.add(tuple(q))
                break
        blocked = 0 if moved else blocked + 1
        axis = (axis + 1) % 3
    band = np.zeros((d, h, w), np.uint8)
    _carve(band, cells)
    return band, (0, 0, 0), len(cells)


def emulate_sweeps(band, seed, conn=6, order="asc", stop_after=None):
    """Model of K5's plane sweeps: (region uint8, sweeps, converged). Sweeps alternate axis 0 (one
    plane per z) and axis 1 (one plane per y). A plane is seeded from region[p ± 1] ∧ band (the
    neighbour planes 3×3-dilated in-plane first for conn 26) and every in-plane component (4- or
    8-connected) of the band that the seeds or the plane's own region touch is filled. `order`:
    "jacobi" (every plane sees the neighbours as the previous sweep left them), "asc" / "desc"
    (planes in ascending / descending order, each seeing the planes already done in this sweep). The
    real kernel lies between these. Stops at the first sweep that changes nothing (counted, like the
    kernel's), or unconverged once `stop_after` sweeps have passed."""
    from scipy import ndimage
    assert conn in (6, 26) and order in ("jacobi", "asc", "desc")
    st2 = ndimage.generate_binary_structure(2, 2 if conn == 26 else 1)
    b = band.astype(bool)
    views, labels = [], []
    for axis in (0, 1):
        bv = np.moveaxis(b, axis, 0)
        lab = np.zeros(bv.shape, np.int32)
        base = 0
        for p in range(bv.shape[0]):  # in-plane components, numbered uniquely over the volume
            lp, k = ndimage.label(bv[p], structure=st2)
            lab[p] = np.where(lp > 0, lp + base, 0)
            base += k
        views.append(bv)
        labels.append((lab, base))
    region = np.zeros(b.shape, bool)
    x, y, z = seed
    region[z, y, x] = b[z, y, x]

    def touch(plane):
        return ndimage.binary_dilation(plane, structure=np.ones((3, 3), bool)) if conn == 26 else plane

    # Growth is monotone, so a plane whose own and neighbours' voxel counts are what they were when
    # it was last processed (in this orientation) cannot change: it is skipped.
    last = [np.full((b.shape[a], 3), -1, np.int64) for a in (0, 1)]
    sweeps = 0
    while stop_after is None or sweeps < stop_after:
        axis = sweeps & 1
        sweeps += 1
        bv, (lab, nlab) = views[axis], labels[axis]
        rv = np.moveaxis(region, axis, 0)  # a view: writes go to `region`
        n = rv.shape[0]
        src = rv.copy() if order == "jacobi" else rv
        cnt = np.concatenate(([0], src.sum(axis=(1, 2)), [0]))  # cnt[p + 1] = voxels of src[p]
        own = rv.sum(axis=(1, 2))
        changed = False
        for p in (range(n - 1, -1, -1) if order == "desc" else range(n)):
            sig = (cnt[p], own[p], cnt[p + 2])
            if tuple(last[axis][p]) == sig:
                continue
            last[axis][p] = sig
            nb = np.zeros(rv.shape[1:], bool)
            if p > 0:
                nb |= src[p - 1]
            if p + 1 < n:
                nb |= src[p + 1]
            seeds = (rv[p] | touch(nb)) & bv[p]
            hit = np.zeros(nlab + 1, bool)
            hit[lab[p][seeds]] = True
            hit[0] = False
            grown = hit[lab[p]]
            if (grown & ~rv[p]).any():
                rv[p] |= grown
                changed = True
                own[p] = rv[p].sum()
                last[axis][p, 1] = own[p]
                if order != "jacobi":
                    cnt[p + 1] = own[p]
        if not changed:
            return region.astype(np.uint8), sweeps, True
    return region.astype(np.uint8), sweeps, False


def old_sweep_cap(band):
    """The sweep limit K5 had before it was replaced by the voxel count: 4·(w + h + d)."""
    return 4 * sum(band.shape)


# The GPU maze case: d × h × w = 30 × 64 × 64, every x-layer. 512 strips; even an oracle's plane
# order needs about two sweeps per strip (one growing front, a plane is processed once per sweep).
MAZE = dict(w=64, h=64, d=30, layers=32)
MAZE_SMALL = dict(w=16, h=24, d=22, layers=1)
STAIRCASE = dict(w=70, h=26, d=21)


# ---- raw volume with a serpentine band ----------------------------------------------------------
SERPENTINE = dict(d=46, h=70, w=100)


def _serpentine_boxes(d, thick, cross):
    zs = slice(d - thick, d) if cross == "top" else slice(0, thick)
    return ((slice(None), 4, 60), (slice(None), 74, 96), (zs, 4, 96))


def serpentine_volume(d=46, h=70, w=100, thick=12, cross="top"):
    """uint16 [d, h, w]: an in-band slab (value 1500) over an out-of-band background (0). It runs
    through all of z at x 4..59, crosses over in the `thick` top (or, cross="bottom", bottom) planes
    and comes back at x 74..95; y spans 14..51. The default seeds (reference_seeds at plane d // 2)
    fall into the first leg or the background only, so growth split into z-slabs has to go to the
    crossing, across and back again. A round is a grow + boundary exchange, and voxels handed over
    at the end of a round are grown in the next, so the slab that holds the seeds needs a third
    round if the crossing lies in another slab: for two slabs that is cross="bottom" (plane d // 2
    belongs to the upper one). The median and the sharpening take a rim of one or two voxels off
    every plane's shape; the slab is ≥ `thick` voxels in y, z and x so that it stays one piece."""
    assert d >= 2 * thick and h >= 56 and w >= 100 and cross in ("top", "bottom")
    v = np.zeros((d, h, w), np.uint16)
    for zs, x0, x1 in _serpentine_boxes(d, thick, cross):
        v[zs, 14:52, x0:x1] = 1500
    return v


def serpentine_mask(d=46, h=70, w=100, thick=12, cross="top", rim=3):
    """The part of serpentine_volume's slab at least `rim` voxels inside it in-plane: what the band
    of the processed volume must contain, as one component."""
    m = np.zeros((d, h, w), bool)
    for zs, x0, x1 in _serpentine_boxes(d, thick, cross):
        m[zs, 14 + rim:52 - rim, x0 + rim:x1 - rim] = True
    return m


# ---- random bands at edge shapes ----------------------------------------------------------------
# (d, h, w), what the shape is there for, band density for conn 6 and conn 26. The densities start
# from 0.40 / 0.18 (above the 3D site-percolation thresholds 0.31 / 0.10, so that the region is a
# large cluster that still leaves band voxels unreached) and are raised where the shape is nearly
# 2D or 1D (thresholds 0.59 / 0.41 in a plane), until test_volume_cases' conditions hold.
# srg=False: morphology and border only. nseeds: planes that get a seed (default 4). saturates: cube
# sizes that fill the whole (tiny) volume.
SHAPE_CASES = (
    dict(shape=(1, 40, 70), why="one xy plane", dens=(0.62, 0.45)),
    dict(shape=(9, 1, 130), why="one xz plane, three words", dens=(0.62, 0.45)),
    dict(shape=(3, 5, 1), why="one column", dens=(0.50, 0.50), nseeds=1, saturates=(7,)),
    dict(shape=(2, 33, 64), why="exactly one word", dens=(0.50, 0.30)),
    dict(shape=(20, 20, 65), why="one bit in the last word", dens=(0.40, 0.18)),
    dict(shape=(37, 20, 63), why="one bit short of a word", dens=(0.40, 0.18)),
    dict(shape=(70, 9, 40), why="d the long side, two words of transposed xz rows", dens=(0.40, 0.18)),
    dict(shape=(130, 6, 7), why="d the long side, three words", dens=(0.45, 0.22)),
    dict(shape=(520, 8, 8), why="xz rows above 512, planes in LDS", dens=(0.45, 0.22)),
    dict(shape=(600, 8, 520), why="global scratch planes because of d", dens=(0.40, 0.18)),
    dict(shape=(4, 636, 512), why="5120 plane words (transposed): global scratch", dens=(0.45, 0.22)),
    dict(shape=(4, 637, 512), why="5120 plane words (transposed): global scratch", dens=(0.45, 0.22)),
    dict(shape=(4, 576, 512), why="w = 512: the last h with planes in LDS (147 456 B)", dens=(0.45, 0.22)),
    dict(shape=(4, 2544, 65), why="5088 plane words: the last LDS shape (162 816 B dynamic)", dens=(0.45, 0.22)),
    dict(shape=(4, 2545, 65), why="5090 plane words: the first global one", dens=(0.45, 0.22)),
    dict(shape=(3, 848, 512), why="morphology: the last LDS plane (162 816 B)", dens=(0.45, 0.22), srg=False),
    dict(shape=(3, 849, 512), why="morphology: the first global plane", dens=(0.45, 0.22), srg=False),
)


def case_id(case):
    return "x".join(str(s) for s in case["shape"])


def case_band(case, conn):
    """The case's random band (uint8 [d, h, w]) for connectivity `conn`."""
    dens = case["dens"][0 if conn == 6 else 1]
    rng = np.random.default_rng(1000 + sum(case["shape"]) + conn)
    return (rng.random(case["shape"]) < dens).astype(np.uint8)


def case_seeds(band, count=4):
    """A few band voxels (x, y, z) from different z: in up to `count` planes spread over the depth,
    the middle one of the plane's band voxels in raster order."""
    d = band.shape[0]
    seeds = []
    for z in sorted({int(t) for t in np.linspace(0, d - 1, count)}):
        ys, xs = np.nonzero(band[z])
        if len(ys):
            seeds.append((int(xs[len(xs) // 2]), int(ys[len(ys) // 2]), z))
    return seeds


def sparse_mask(shape, seed=0, every=3000):
    """Dilation input (bool [d, h, w]): about one voxel in `every`, plus the two opposite corners and
    the voxels on both sides of every word boundary of the first row — sparse enough that a 7³ cube
    around each leaves most of the volume clear, so a wrong reach at an edge shows."""
    d, h, w = shape
    m = np.random.default_rng(seed + d + h + w).random(shape) < 1.0 / every
    m[0, 0, 0] = m[d - 1, h - 1, w - 1] = True
    for x in range(63, w, 64):
        m[d // 2, h // 2, x] = True
        if x + 1 < w:
            m[d - 1, 0, x + 1] = True
    return m


# Cube sizes up to the limit and ball sizes above 7 on one shape; radius 12 already covers d = 12, so
# sizes 25 and 63 saturate z (every plane holds the same in-plane result).
DILATION_RANGE = dict(shape=(12, 40, 100), cube=(1, 9, 25, 63), ball=(9, 15), saturates_z=(25, 63))
DILATION_REJECTED = (0, 2, 8, 64, 65, 129)


def cube_dilation_ref(mask, size):
    """size³ cube dilation by scipy's separable maximum filter, out-of-volume samples ignored."""
    from scipy import ndimage
    return ndimage.maximum_filter(np.asarray(mask, bool).astype(np.uint8), size=size, mode="constant", cval=0) > 0


def ball_ref(size):
    """The digital ball of radius size // 2: offsets with dx² + dy² + dz² ≤ r²."""
    r = size // 2
    ax = np.arange(-r, r + 1)
    zz, yy, xx = np.meshgrid(ax, ax, ax, indexing="ij")
    return zz * zz + yy * yy + xx * xx <= r * r


def dilation_range_mask():
    """Four voxels placed so that even the 63-cube leaves columns clear (x = 37, 38)."""
    m = np.zeros(DILATION_RANGE["shape"], bool)
    for z, y, x in ((0, 0, 0), (2, 20, 5), (11, 3, 70), (6, 39, 99)):
        m[z, y, x] = True
    return m


# ---- border -------------------------------------------------------------------------------------
BORDER_RADII = (1, 2, 5)
BORDER_SHAPES = ((5, 70, 100), (3, 849, 512))  # LDS planes with a partial last word; global planes


def border_mask(shape, seed=0):
    """bool [d, h, w]: per plane a union of rectangles 3..40 on a side (some thinner than the widest
    erosion, some clipped by the plane's edges, one flush in the bottom-right corner) with a few
    one-voxel holes."""
    d, h, w = shape
    rng = np.random.default_rng(seed + h + w)
    m = np.zeros(shape, bool)
    for z in range(d):
        for _ in range(max(6, h * w // 4000)):
            rh, rw = rng.integers(3, 41, 2)
            y, x = rng.integers(-10, h), rng.integers(-10, w)
            m[z, max(y, 0):y + rh, max(x, 0):x + rw] = True
        m[z, h - 15:, w - 20:] = True
        ys, xs = np.nonzero(m[z])
        pick = rng.integers(0, len(ys), 5)
        m[z, ys[pick], xs[pick]] = False
    return m


# ---- where the kernels switch from LDS planes to global scratch ---------------------------------
LDS_BUDGET = 160 * 1024


def srg_plane_words(shape):
    """Words of one of the region growing's four plane buffers (k5_volume.hip, srg3d_shape): sized
    for both sweep orientations, rows of max(h, d) × ceil(w/64) words or their transpose of
    w × ceil(max(h, d)/64), rounded up to even."""
    d, h, w = shape
    rows = max(h, d)
    return (max(rows * ((w + 63) // 64), w * ((rows + 63) // 64)) + 1) & ~1


def srg_planes_global(shape):
    return srg_plane_words(shape) * 32 + 1024 > LDS_BUDGET


def morph_planes_global(shape):
    """The in-plane dilation and the border keep three planes of h × ceil(w/64) words."""
    d, h, w = shape
    return ((h * ((w + 63) // 64) + 1) & ~1) * 24 + 1024 > LDS_BUDGET
