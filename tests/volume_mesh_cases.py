"""Masks for the surface mesh (nm03/volume_mesh.h, K15) and the integer checks of its invariants. Masks only:
the mesh does not read the samples. Every mask is built once per process and is read-only.

  single_voxel      1 x 1 x 1, set: the cube
  full              5 x 4 x 3, all set: every open face lies on the frame
  edge_touch        two voxels that share an edge: non-manifold along it
  corner_touch      two voxels that share a corner: non-manifold at it
  checkerboard      4 x 5 x 6, (x + y + z) even: every face is open, every corner mixed
  empty             nothing set: the empty mesh
  ball              a digital ball in 21 x 19 x 17
  hollow_box        a box with a cavity: an outer and an inner shell
  noise_w63 ... noise_w128   noise at widths 63, 64, 65, 127, 128: lattice rows of 64, 65, 66, 128, 129 bits
                    straddle the u64 word edges
  k14_shape         130 x 40 x 12 (w x h x d), the shape K14's tests use for more than one workgroup per axis
  many_blocks       130 x 200 x 100 noise: 60903 lattice words, at the smallest scan block (64 words) 952 block
                    totals — more than the 256 threads of the totals workgroup
"""
import functools

import numpy as np

PLACEMENTS = ("corner", "nets")
TOTALS_WORKGROUP = 256  # threads of K15's totals-scan workgroup (kMeshThreads in src/kernels/k15_volume_mesh.hip)


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    a.setflags(write=False)
    return a


def _noise(shape, seed, p=0.35):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def _ball(shape, r):
    d, h, w = shape
    z, y, x = np.mgrid[0:d, 0:h, 0:w]
    return ((x - w // 2) ** 2 + (y - h // 2) ** 2 + (z - d // 2) ** 2 <= r * r).astype(np.uint8)


def _hollow():
    m = np.zeros((9, 10, 11), np.uint8)
    m[1:8, 1:9, 1:10] = 1
    m[3:6, 3:7, 3:8] = 0
    return m


def _pair(offset):
    m = np.zeros((3, 3, 3), np.uint8)
    m[0, 0, 0] = 1
    m[offset] = 1
    return m


def _checker():
    z, y, x = np.mgrid[0:6, 0:5, 0:4]
    return ((x + y + z) % 2 == 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def all_cases():
    """List of dicts: name, mask ([D, H, W] uint8, read-only), spacing (sx, sy, sz)."""
    cs = [
        ("single_voxel", np.ones((1, 1, 1), np.uint8), (1.0, 1.0, 1.0)),
        ("full", np.ones((3, 4, 5), np.uint8), (1.0, 1.0, 1.0)),
        ("edge_touch", _pair((0, 1, 1)), (1.0, 1.0, 1.0)),
        ("corner_touch", _pair((1, 1, 1)), (1.0, 1.0, 1.0)),
        ("checkerboard", _checker(), (0.5, 0.75, 1.25)),
        ("empty", np.zeros((3, 4, 5), np.uint8), (1.0, 1.0, 1.0)),
        ("ball", _ball((17, 19, 21), 7), (0.9, 1.2, 2.5)),
        ("hollow_box", _hollow(), (1.0, 1.0, 3.0)),
    ]
    for i, w in enumerate((63, 64, 65, 127, 128)):
        cs.append((f"noise_w{w}", _noise((3, 5, w), 100 + i), (0.7, 1.3, 2.1)))
    cs.append(("k14_shape", _noise((12, 40, 130), 200, 0.3), (0.9, 1.2, 2.5)))
    cs.append(("many_blocks", _noise((100, 200, 130), 300, 0.04), (1.0, 1.0, 1.0)))  # sparse: the mesh stays small
    return tuple(dict(name=n, mask=_ro(m), spacing=s) for n, m, s in cs)


def ids(cases):
    return [c["name"] for c in cases]


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def lattice_words(shape):
    d, h, w = shape
    return ((w + 1 + 63) // 64) * (h + 1) * (d + 1)


def assert_mesh_equal(got, want):
    for k in ("width", "height", "depth", "placement", "quads_x", "quads_y", "quads_z", "voxels"):
        assert got[k] == want[k], k
    for k in ("vertices", "quads"):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, a.shape, b.dtype, b.shape)
        assert a.tobytes() == b.tobytes(), k  # floats compared as bits


def doubled_corners(mesh, spacing):
    """The integer positions 2c - 1 of a `corner` mesh: the f32 positions divided by the f32 spacing are exact
    multiples of 1/2 for the spacings used here (checked)."""
    sp = np.asarray([np.float32(spacing[0]), np.float32(spacing[1]), np.float32(np.float64(spacing[2]))], dtype=np.float32)
    v = np.asarray(mesh["vertices"], dtype=np.float64)
    two = 2.0 * v / sp.astype(np.float64)[None, :]
    n = np.rint(two).astype(np.int64)
    assert np.abs(two - n).max(initial=0.0) < 1e-4
    assert (n % 2 != 0).all()
    return n


def check_invariants(mesh, mask, corners2):
    """The invariants of nm03/volume_mesh.h in integer arithmetic. `corners2`: the vertices' 2c - 1."""
    q = np.asarray(mesh["quads"], dtype=np.int64)
    nv = len(corners2)
    assert q.size == 0 or (q.min() >= 0 and q.max() < nv)  # every corner of a quad is a vertex
    assert len(np.unique(q)) == nv  # every vertex is used
    assert len(q) == mesh["quads_x"] + mesh["quads_y"] + mesh["quads_z"]
    assert mesh["voxels"] == int(np.asarray(mask, dtype=bool).sum())
    # the vertices are the mixed corners in raster order (k, j, i)
    c = (corners2 + 1) // 2
    d, h, w = mask.shape
    key = (c[:, 2] * (h + 1) + c[:, 1]) * (w + 1) + c[:, 0]
    assert (np.diff(key) > 0).all()
    # each axis' quads are planar along it
    bounds = np.cumsum([0, mesh["quads_x"], mesh["quads_y"], mesh["quads_z"]])
    for a in range(3):
        qa = q[bounds[a]:bounds[a + 1]]
        if len(qa):
            pa = corners2[qa][:, :, a]
            assert (pa == pa[:, :1]).all()
    # closed: every directed edge as often as its reverse
    e = np.concatenate([q[:, [0, 1]], q[:, [1, 2]], q[:, [2, 3]], q[:, [3, 0]]])
    fwd = np.sort(e[:, 0] * max(nv, 1) + e[:, 1])
    rev = np.sort(e[:, 1] * max(nv, 1) + e[:, 0])
    assert np.array_equal(fwd, rev)
    # the signed volume: sum of det(v0, v1, v2) over the triangles = 48 * voxels
    tri = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
    p = corners2[tri]  # [T, 3 vertices, 3 coordinates]
    det = np.einsum("ti,ti->t", p[:, 0], np.cross(p[:, 1], p[:, 2])) if len(tri) else np.zeros(0, np.int64)
    assert int(det.sum()) == 48 * mesh["voxels"]
