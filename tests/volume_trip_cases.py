"""Inputs at which the strided loops of K14 and K16 take more than one trip (test_volume_trip_cases.py on the CPU,
test_gpu_volume_trips.py on the GPU; NumPy only, not a conftest). Every other K14 / K16 input of the suite is so small
that these loops take at most one trip. The sizes are the smallest that make them turn; every comparison made with
them is == on integers, bits and text. test_volume_trip_cases.py asserts each property below on the inputs themselves.

K16, the thickness pass (vdist_planes_kernel<kDistThickness>): at most DIST_MAX_SLOTS = 1024 workgroups of
DIST_WORDS_PER_WORKGROUP = 4 words, so above 4096 mask words a workgroup strides over the rest and keeps the best
(value, smallest raster position) across its trips. trip(word) = word // 4 // 1024. All but the last case have w = 64,
one word per row (word = z * 64 + y), and hold cubes of side 3, 5 or 7 centred at (23, 13, 4 + 64 * i), background on
all six sides: two centres 64 planes apart are the same lane of the same workgroup, one trip apart. A k-cube's centre
lies (k + 1) / 2 steps from the background: 16 000 000 um^2 for a 7-cube at 1000 um.
  tie_two_trips          73 x 64 x 64 (d, h, w), 4672 words, 2 trips: 7-cubes at i = 0, 1; the maximum is attained
                         exactly twice, once per trip, and the first one (23, 13, 4) has to stay
  winner_in_second_trip  73 x 64 x 64, 2 trips, spacing (391, 703, 6500): a 3-cube at (21, 11, 2) and a 7-cube at
                         (43, 33, 68); the maximum 2 446 096 = (4 * 391)^2 is attained in trip 1 only, first at (43, 32, 65)
  tie_three_trips        137 x 64 x 64, 8768 words, 3 trips: 7-cubes at i = 0, 1, 2; (23, 13, 4) stays through two ties
  rising                 137 x 64 x 64, 3 trips: cubes 3, 5, 7; every trip brings a better value, (23, 13, 132) wins
  falling                137 x 64 x 64, 3 trips: cubes 7, 5, 3; the first trip's value survives two worse ones
  noise_three_trips      44 x 64 x 130, three words per row, 8448 words, 3 trips: noise of density 0.97 at (600, 700, 800);
                         the single maximum 13 970 000 lies at (0, 16, 43), in trip 2

K14 (samples from a seeded integers(0, 4096) unless stated):
  vv_init_kernel runs at most VV_INIT_WORKGROUPS = 1024 workgroups of VV_THREADS = 256 threads and strides over the
  projection scratch of w * h + w * d + h * d elements; vv_point_kernel (one workgroup) strides 256 threads over the
  h * wpr words of the z-shadow and the d * wpr words of the y-shadow; vv_count_kernel (one workgroup per view) over
  the view's mask words.
  bright_full, dark_sparse  one shape, 9 x 520 x 520: 279 760 projection elements, 2 trips of the init kernel (the tail
                         of the z-projection and all of the y- and x-projections lie past the first 262 144); the
                         projection grid is 5 x 33 x 2 workgroups, so all three projections accumulate by atomics on
                         what init left; h * wpr = 4680 words, 19 trips of the point kernel; the axial views' 4680
                         words, 19 trips of the count kernel; 520 % 64 = 8, a partial last word. bright_full has
                         every sample 4095 and the mask all ones, dark_sparse samples below 100 and the mask only
                         [2:7, 300:500, 330:515]: run one after the other, an element that init misses keeps 4095 or
                         a set mask bit
  deep_point             40 x 20 x 520: d * wpr = 360 words, 2 trips of the point kernel's z loop; the mask is only
                         [31:38, 3:15, 400:515], so both z extremes are found in the second trip (word >= 256 <=> z >= 29)

with_bits_past_width sets the storage bits past the width in the last word of every row of a packed mask: the kernels
promise to ignore them, and the ops never pass any."""
import functools

import numpy as np

# src/kernels/k16_volume_distance.hip
DIST_MAX_SLOTS = 1024            # kDistMaxSlots: workgroups of the thickness pass
DIST_WORDS_PER_WORKGROUP = 4     # kDistWaves: a wave per u64 word
DIST_WORDS_PER_TRIP = DIST_MAX_SLOTS * DIST_WORDS_PER_WORKGROUP
# src/kernels/k14_volume_views.hip
VV_THREADS = 256                 # kVvThreads
VV_INIT_WORKGROUPS = 1024        # the cap of vv_init_kernel's grid
VV_INIT_ELEMENTS_PER_TRIP = VV_INIT_WORKGROUPS * VV_THREADS

ISO = (1000, 1000, 1000)
CUBE_CENTRE = (23, 13, 4)  # x, y, z of block 0
CUBE_PITCH = 64            # planes between two blocks: 64 rows of one word = 4096 words = one trip


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


def _cubes(d, blocks):
    """d x 64 x 64 with one cube per (side, (x, y, z) centre) of `blocks`."""
    m = np.zeros((d, 64, 64), np.uint8)
    for side, (x, y, z) in blocks:
        r = side // 2
        m[z - r:z + r + 1, y - r:y + r + 1, x - r:x + r + 1] = 1
    return m


def _stack(d, sides):
    x, y, z = CUBE_CENTRE
    return _cubes(d, [(s, (x, y, z + CUBE_PITCH * i)) for i, s in enumerate(sides)])


def _thickness(name, mask, um, trips, um2, at, attained_in):
    return dict(name=name, mask=_ro(mask, np.uint8), um=tuple(um), trips=trips, attained_in=tuple(attained_in),
                want={"inscribed_um2": um2, "inscribed_at": list(at), "found": True})


@functools.lru_cache(maxsize=None)
def thickness_cases():
    """Tuple of dicts: name, mask (uint8 [D, H, W], read-only), um (ux, uy, uz), trips (of the thickness loop),
    attained_in (the trips in which a mask voxel attains the maximum), want (the record's integers)."""
    noise = (np.random.RandomState(7).random_sample((44, 64, 130)) < 0.97).astype(np.uint8)
    return (
        _thickness("tie_two_trips", _stack(73, (7, 7)), ISO, 2, 16_000_000, (23, 13, 4), (0, 1)),
        _thickness("winner_in_second_trip", _cubes(73, [(3, (21, 11, 2)), (7, (43, 33, 68))]), (391, 703, 6500), 2, 2_446_096,
                   (43, 32, 65), (1,)),
        _thickness("tie_three_trips", _stack(137, (7, 7, 7)), ISO, 3, 16_000_000, (23, 13, 4), (0, 1, 2)),
        _thickness("rising", _stack(137, (3, 5, 7)), ISO, 3, 16_000_000, (23, 13, 132), (2,)),
        _thickness("falling", _stack(137, (7, 5, 3)), ISO, 3, 16_000_000, (23, 13, 4), (0,)),
        _thickness("noise_three_trips", noise, (600, 700, 800), 3, 13_970_000, (0, 16, 43), (2,)),
    )


MAP_CASES = ("tie_two_trips", "winner_in_second_trip")  # the 73-plane ones: the map is compared on them as well


def word_count(shape):
    d, h, w = shape
    return d * h * ((w + 63) // 64)


def trip_of(shape, z, y, x):
    """The trip of the thickness loop in which voxel (x, y, z) is looked at (arrays or integers)."""
    d, h, w = shape
    return ((z * h + y) * ((w + 63) // 64) + x // 64) // DIST_WORDS_PER_WORKGROUP // DIST_MAX_SLOTS


# ---- K14 ----------------------------------------------------------------------------------------------
INIT_SHAPE = (9, 520, 520)   # d, h, w
DEEP_SHAPE = (40, 20, 520)
DEEP_BOX = (slice(31, 38), slice(3, 15), slice(400, 515))
SPARSE_BOX = (slice(2, 7), slice(300, 500), slice(330, 515))


def _samples(shape, seed, hi=4096):
    return np.random.default_rng(seed).integers(0, hi, size=shape, dtype=np.int64).astype(np.uint16)


def _view(id, raw, mask, why):
    return dict(id=id, raw=_ro(raw, np.uint16), mask=_ro(mask, np.uint8), type="u16", stored_bits=16, inverted=False, at="mask",
                why=why)


@functools.lru_cache(maxsize=None)
def view_cases():
    """Dict id → case in the form of volume_view_cases (id, raw, mask, type, stored_bits, inverted, at, why)."""
    sparse = np.zeros(INIT_SHAPE, np.uint8)
    sparse[SPARSE_BOX] = 1
    deep = np.zeros(DEEP_SHAPE, np.uint8)
    deep[DEEP_BOX] = 1
    cs = (
        _view("bright_full", np.full(INIT_SHAPE, 4095, np.uint16), np.ones(INIT_SHAPE, np.uint8),
              "the brightest sample and a set mask bit in every element of the scratch"),
        _view("dark_sparse", _samples(INIT_SHAPE, 501, 100), sparse, "samples below 100 and a mask box: what init misses shows"),
        _view("deep_point", _samples(DEEP_SHAPE, 502), deep, "both z extremes of the mask in the point kernel's second trip"),
    )
    return {c["id"]: c for c in cs}


def projection_elements(shape):
    d, h, w = shape
    return w * h + w * d + h * d


def trips(n, per_trip):
    return (n + per_trip - 1) // per_trip


# ---- bits past the width ------------------------------------------------------------------------------
# The existing cases the kernels are run on with those bits set (every width here is no multiple of 64), besides dark_sparse.
PAST_WIDTH_DISTANCE = ("width_70", "noise_50", "word_edges", "full")       # volume_distance_cases
PAST_WIDTH_MESH = ("noise_w63", "noise_w65", "noise_w127", "k14_shape")    # volume_mesh_cases
PAST_WIDTH_VIEWS = ("w63", "w65", "w130")                                  # volume_view_cases


def with_bits_past_width(words, w):
    """Packed [D, H, wpr] int64 words (a NumPy array or a tensor) → a copy with every storage bit past `w` set in the
    last word of each row. Nothing to set when w is a multiple of 64."""
    out = words.clone() if hasattr(words, "clone") else np.array(words)
    r = w % 64
    if r:
        out[..., -1] |= -(1 << r)  # int64: bits r … 63
    return out
