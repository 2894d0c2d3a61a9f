"""Named test masks for the diameter tests (not a conftest): every name of measure_masks plus the masks
a lesion-geometry kernel gets wrong. build(name, h, w) → bool [h, w].

frame_and_disc: a one-pixel frame inset by one, plus a disc of larger area inside: the lesion is the
    disc, and in every row of it runs of ANOTHER component (the frame) lie left and right of its own. (On a very
    elongated plane such as 1100×70 the frame is the larger one: then it is the lesion and the disc's runs lie
    between its own.)
two_equal: two 10×10 blocks, the second one earlier in raster order: the lesion choice is the tie rule.
rect: an a×b block away from the frame: major_px2 = (a − 1)² + (b − 1)², both diagonals tied.
word_span: one lesion whose rows end at columns 63, 64, 65 and w − 1 and start at 63, 64 and 65."""
import functools

import numpy as np

import measure_masks as mm

EXTRA = ("frame_and_disc", "two_equal", "rect", "word_span")
NAMES = list(mm.NAMES) + list(EXTRA)
RECT = (7, 23)  # rows, columns of `rect`, placed at (RECT_AT[0], RECT_AT[1])
RECT_AT = (11, 40)


@functools.lru_cache(maxsize=None)
def build(name, h, w):
    """The named mask at h × w (cached: callers get a read-only array)."""
    if name not in EXTRA:
        return mm.build(name, h, w)
    m = np.zeros((h, w), bool)
    if name == "frame_and_disc":
        m[1, 1:w - 1] = m[h - 2, 1:w - 1] = True
        m[1:h - 1, 1] = m[1:h - 1, w - 2] = True
        y, x = np.mgrid[0:h, 0:w]
        m |= (y - h // 2) ** 2 + (x - w // 2 - 3) ** 2 <= (min(h, w) // 4) ** 2
    elif name == "two_equal":
        m[5:15, 60:70] = True
        m[40:50, 3:13] = True
    elif name == "rect":
        m[RECT_AT[0]:RECT_AT[0] + RECT[0], RECT_AT[1]:RECT_AT[1] + RECT[1]] = True
    elif name == "word_span":
        # consecutive rows overlap, so the runs are one component at either connectivity
        runs = [(40, 63), (50, 64), (60, 65), (63, 80), (64, 90), (65, w - 1), (0, w - 1), (0, 63), (0, 64), (0, 65)]
        for y, (a, b) in enumerate(runs, start=2):
            m[y, a:min(b, w - 1) + 1] = True
    m.setflags(write=False)
    return m


def brute_force(lesion):
    """The record's geometry from ALL lesion pixels (bool [h, w], non-empty), in NumPy: (major_px2,
    [xa, ya, xb, yb], perp_extent, [xc, yc, xd, yd]) with the record's tie-breaks."""
    pts = np.argwhere(lesion).astype(np.int64)  # (y, x) in raster = lexicographic order
    y, x = pts[:, 0], pts[:, 1]
    d2 = (y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2
    iu = np.triu_indices(len(pts), 0)  # row-major over i <= j: lexicographic in (a, b)
    k = int(np.argmax(d2[iu]))         # the first maximum
    a, b = pts[iu[0][k]], pts[iu[1][k]]
    dy, dx = b - a
    proj = -dy * x + dx * y
    c, d = pts[int(np.argmin(proj))], pts[int(np.argmax(proj))]  # the first extremes
    return (int(d2[iu][k]), [int(a[1]), int(a[0]), int(b[1]), int(b[0])], int(proj.max() - proj.min()),
            [int(c[1]), int(c[0]), int(d[1]), int(d[0])])
