"""Inputs of the volume-measurement tests (test_volume_measure.py on the CPU, test_gpu_volume_measure.py
on the GPU; not a conftest). Everything here is NumPy on the CPU; masks are uint8 [d, h, w].

  * SOLIDS: named solids with a known topology (components, cavities, tunnels at 6- and at
    26-connectivity): torus, hollow shell, ball, a square ring in one plane, two voxels sharing only a
    corner.
  * trivial volumes (empty, full, the 8 corner voxels), a solid whose runs start, end and cross at the
    word edges in neighbouring rows and planes, and noise at four densities, each on the shapes where
    the kernels' word arithmetic changes path.
  * the maze and the staircase of volume_cases: one-voxel paths, the deepest union chains.
"""
import numpy as np

import volume_cases as vc


def _grid(shape):
    return np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")


def torus():
    z, y, x = _grid((21, 41, 41))
    return ((np.sqrt((y - 20.0) ** 2 + (x - 20.0) ** 2) - 12.0) ** 2 + (z - 10.0) ** 2 <= 16.0).astype(np.uint8)


def _r2():
    z, y, x = _grid((21, 41, 41))
    return (z - 10) ** 2 + (y - 20) ** 2 + (x - 20) ** 2


def shell():
    r2 = _r2()
    return ((r2 >= 36) & (r2 <= 81)).astype(np.uint8)


def ball():
    return (_r2() <= 49).astype(np.uint8)


def square_ring():
    """One plane of a 5 × 20 × 70 volume: a frame two voxels thick that crosses the word edge at x = 64."""
    m = np.zeros((5, 20, 70), np.uint8)
    m[2, 4:15, 10:67] = 1
    m[2, 6:13, 12:65] = 0
    return m


def corner_pair():
    m = np.zeros((3, 3, 3), np.uint8)
    m[0, 0, 0] = m[1, 1, 1] = 1
    return m


# name → (mask builder, {connectivity: (components, cavities, tunnels)})
SOLIDS = {
    "torus": (torus, {6: (1, 0, 1), 26: (1, 0, 1)}),
    "shell": (shell, {6: (1, 1, 0), 26: (1, 1, 0)}),
    "ball": (ball, {6: (1, 0, 0), 26: (1, 0, 0)}),
    "square_ring": (square_ring, {6: (1, 0, 1), 26: (1, 0, 1)}),
    "corner_pair": (corner_pair, {6: (2, 0, 0), 26: (1, 0, 0)}),
}

# (d, h, w): one xy plane; one xz plane of three words; one column; exactly one word; one bit in the
# last word; one bit short of a word; d the long side.
SHAPES = ((1, 40, 70), (9, 1, 130), (3, 5, 1), (2, 33, 64), (20, 20, 65), (37, 20, 63), (70, 9, 40))
NOISE_SHAPE = (12, 20, 70)
DENSITIES = (0.1, 0.31, 0.5, 0.9)
GPU_EXTRA_SHAPE = (4, 130, 200)   # more words per plane (520) than one workgroup has threads
COHORT_SHAPE = (25, 256, 256)     # a cohort series: thousands of workgroups


def shape_id(shape):
    return "x".join(str(s) for s in shape)


def empty(shape):
    return np.zeros(shape, np.uint8)


def full(shape):
    return np.ones(shape, np.uint8)


def corners(shape):
    m = np.zeros(shape, np.uint8)
    d, h, w = shape
    for z in (0, d - 1):
        for y in (0, h - 1):
            for x in (0, w - 1):
                m[z, y, x] = 1
    return m


def word_edges(shape):
    """Per row a run between two of the columns 0, 62 … 66, 126 … 130, w − 2, w − 1 (those inside the
    width) plus a lone voxel on a third, the choice shifting with y and z: runs that start, end and
    cross at x = 63 / 64 / 65 and w − 1 in neighbouring rows AND planes."""
    d, h, w = shape
    marks = sorted({x for x in (0, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, w - 2, w - 1) if 0 <= x < w})
    m = np.zeros(shape, np.uint8)
    for z in range(d):
        for y in range(h):
            i = 3 * z + y
            a, b = marks[i % len(marks)], marks[(7 * i + 3) % len(marks)]
            m[z, y, min(a, b):max(a, b) + 1] = 1
            m[z, y, marks[(i + 5) % len(marks)]] = 1
    return m


def noise(shape, density):
    seed = 4000 + sum(shape) + int(round(density * 100))
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def raw_for(shape, seed=0):
    """16-bit samples of every bit pattern for a mask of `shape`."""
    return np.random.default_rng(900 + seed + sum(shape)).integers(0, 65536, shape, dtype=np.uint16)


def region_for(mask):
    """A region volume ⊆ mask with a different voxel count (every third mask voxel dropped)."""
    r = mask.copy()
    idx = np.flatnonzero(r)
    r.reshape(-1)[idx[::3]] = 0
    return r


def maze():
    return vc.maze(**vc.MAZE)[0]


def staircase():
    return vc.staircase(**vc.STAIRCASE)[0]


def shape_cases():
    """(id, mask builder) for every trivial, word-edge and noise case on every shape."""
    cases = []
    for shape in SHAPES + (NOISE_SHAPE,):
        sid = shape_id(shape)
        for name, fn in (("empty", empty), ("full", full), ("corners", corners), ("word_edges", word_edges)):
            cases.append((f"{name}-{sid}", lambda fn=fn, shape=shape: fn(shape)))
        for dens in DENSITIES:
            cases.append((f"noise{dens}-{sid}", lambda shape=shape, dens=dens: noise(shape, dens)))
    return cases


def all_cases():
    """(id, mask builder): the named solids, then shape_cases()."""
    return [(name, fn) for name, (fn, _) in SOLIDS.items()] + shape_cases()
