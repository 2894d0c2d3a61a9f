"""Inputs of the measurement-layout tests (test_measure_layout_cases.py on the CPU,
test_gpu_measure_layouts.py on the GPU; not a conftest): the buffer layouts on which the 2D engine and the
3D VolumeRunner hand their samples and bit planes to the measurement kernels K7–K13, which the ops never
produce. Everything here is NumPy on the CPU plus the native phantom and DICOM writer; the sample formats
and the export cohorts (deep_odd, formats) are volume_export_cases'.

Stride volumes. VolumeRunner lays the planes of a volume out `ps` = w·h rounded up to 8 samples apart and
passes `ps` to K8, K10, K11 and K12 as the plane stride; the ops pass w·h. Seven volumes of five planes of
h × 131, h = 101, 102, 103, 105, 106, 107, 108: w·h % 8 = 7, 2, 5, 3, 6, 1, 4, every non-zero remainder,
so ps − w·h takes every value from 1 to 7. 131 = 2·64 + 3: three mask words per row, the last one with
three valid bits. The planes are cut from the lesion window as volume_export_cases.slice0 does; unsigned
and signed volumes alternate (one runner measures them all).

2D engine set. Twelve DICOM files in one directory for PipelineConfig(batch_size=3, streams=2): four
batches on two slots. Shapes (h × w) 101 × 131, 100 × 163, 256 × 256, 1030 × 100, 130 × 129 (w·h % 8 =
7, 4, 0, 0, 2: raw_off advances by the rounded size; 3, 3, 4, 2, 3 words per row), sample formats u16, i16,
i16_12, u16_12_garbage and u8. Two files are bad, each the middle one of its batch: a 99 × 131 slice
(below min_dim) and a file cut off inside its pixel data. The slice after a bad one differs from it and
from its other neighbour in shape and format, so a record attributed to the wrong loaded slice shows.

The phantom's lesion lies in the middle of the frame and never reaches the last columns, so every slice
and plane built here whose width is no multiple of 64 carries a band-valued bar from the centre seed to
the right edge (and 1030 × 100 a ramp-valued column across row 1024): the grown region and its
dilation then have pixels in the partial last word of a row."""
import os

import numpy as np

import large_slice_cases as lc
import volume_export_cases as xc

# ---- formats ----------------------------------------------------------------------------------------
PLAIN = "u16"  # unsigned 16-bit, no rescale: not one of volume_export_cases.FORMATS (all of which differ from it)


def format_meta(name, spacing=(1.0, 1.0)):
    """(write, meta) as volume_export_cases.format_meta gives them, also for PLAIN."""
    if name != PLAIN:
        return xc.format_meta(name, spacing)
    write = dict(type="u16", bits_stored=16, write_rescale=False, slope=1.0, intercept=0.0, spacing_x=spacing[0],
                 spacing_y=spacing[1])
    meta = dict(type="u16", stored_bits=16, slope=1.0, intercept=0.0, spacing_x=spacing[0], spacing_y=spacing[1])
    return write, meta


def format_store(name, phantom):
    return np.asarray(phantom, dtype=np.uint16) if name == PLAIN else xc.format_store(name, phantom)


BAR_VALUE = 1700  # mid-rim: inside the default band in every format used here (1400 as i16 is 0.78 normalised)
BAR_HALF = lc.BRIDGE_HALF


def barred(phantom):
    """`phantom` (uint16 [h, w] or [d, h, w]) with a bar of BAR_VALUE, 2·BAR_HALF rows high, from the centre
    column (where reference_seeds puts its first seed) to the right edge."""
    a = np.array(phantom, dtype=np.uint16)
    h, w = a.shape[-2:]
    a[..., h // 2 - BAR_HALF:h // 2 + BAR_HALF, w // 2:] = BAR_VALUE
    return a


def ramped(phantom):
    """`phantom` (uint16 [h, w], h above 1024) with a column 2·BAR_HALF wide through the centre seed over the
    whole height, rising from 1400 at the top to 1899 at the bottom (inside the band; a ramp passes the
    median and the sharpening unchanged): the region crosses row 1024, as with large_slice_cases.bridged,
    but the samples under it differ, so the percentiles and the grey levels of the slice do too."""
    a = np.array(phantom, dtype=np.uint16)
    h, w = a.shape
    a[:, w // 2 - BAR_HALF:w // 2 + BAR_HALF] = (1400 + np.arange(h) * 500 // h).astype(np.uint16)[:, None]
    return a


def touches_partial_word(mask):
    """Some set pixel of `mask` [..., h, w] lies in the last mask word of its row, and that word is partial."""
    w = mask.shape[-1]
    wpr = (w + 63) // 64
    return w % 64 != 0 and bool(np.asarray(mask)[..., 64 * (wpr - 1):].any())


# ---- stride volumes ---------------------------------------------------------------------------------
STRIDE_W = 131
STRIDE_HEIGHTS = (101, 102, 103, 105, 106, 107, 108)
STRIDE_REMAINDERS = (7, 2, 5, 3, 6, 1, 4)  # w·h % 8 in that order
STRIDE_DEPTH = 5
STRIDE_FORMATS = (PLAIN, "i16")  # alternating
STRIDE_SPACING = (0.5, 0.75, 2.5)  # x, y, z in mm: anisotropic, so K13 maximises in 500 × 750 × 2500 um
STRIDE_Z_SOURCE = "spacing_between_slices"
STRIDE_LESIONS = 4
STRIDE_LEVELS = 24


def stride_volumes(native):
    """The seven volumes as dicts id, planes (uint16 [5, h, 131], read-only), format, meta."""
    out = []
    s0 = xc.slice0(STRIDE_DEPTH)
    for i, h in enumerate(STRIDE_HEIGHTS):
        name = STRIDE_FORMATS[i % 2]
        ph = np.stack([native.phantom_slice(h, STRIDE_W, 20 + i, s0 + k, xc.NSLICES, xc.SEED) for k in range(STRIDE_DEPTH)])
        planes = np.ascontiguousarray(format_store(name, barred(ph)), dtype=np.uint16)
        planes.setflags(write=False)
        out.append(dict(id=f"h{h}", planes=planes, format=name, meta=format_meta(name)[1]))
    return out


def padded_stride(h, w):
    """VolumeRunner's plane stride in samples (src/runtime/volume.cpp: w·h rounded up to 8)."""
    return (w * h + 7) // 8 * 8


# ---- the 2D engine set ------------------------------------------------------------------------------
ENGINE_SHAPES = ((101, 131), (100, 163), (256, 256), (1030, 100), (130, 129))  # h, w
ENGINE_FORMATS = (PLAIN, "i16", "i16_12", "u16_12_garbage", "u8")
ENGINE_SPACING = (0.9, 1.2)
ENGINE_BATCH = 3
ENGINE_MAX_DIM = 1088  # 1030 rounded up to 64, as the command-line tool sizes its buffers
ENGINE_MIN_DIM = 100
SMALL, TRUNCATED = "small", "truncated"
# (h, w), format, what is wrong with the file (None: a good slice). In file order; batches are threes.
ENGINE_SLICES = (
    ((101, 131), "i16", None), ((100, 163), "u16_12_garbage", None), ((256, 256), PLAIN, None),
    ((1030, 100), PLAIN, None), ((99, 131), PLAIN, SMALL), ((130, 129), "u8", None),
    ((130, 129), "i16_12", None), ((101, 131), "u8", None), ((1030, 100), "u16_12_garbage", None),
    ((100, 163), "i16", None), ((101, 131), "i16", TRUNCATED), ((256, 256), "i16_12", None),
)
ENGINE_BAD = {4: (2, "Image dimensions too small: 131x99"),  # index → (status code, message)
              10: (1, "DICOM pixel data shorter than Rows*Columns")}
# run_array: every non-256 shape once, in a format of its own
RUN_ARRAY_CASES = (((101, 131), "i16"), ((100, 163), "u16_12_garbage"), ((1030, 100), PLAIN), ((130, 129), "u8"))


def engine_phantom(native, shape, index):
    """The unsigned phantom of slice `index` of the set at `shape`: barred unless the width is a multiple of
    64, with the ramped column where the slice is higher than 1024."""
    h, w = shape
    p = native.phantom_slice(h, w, 3 + index % 5, 12, 25, 7)
    if w % 64:
        p = barred(p)
    return ramped(p) if h > lc.WRAP else p


def engine_slice(native, index):
    """(stored words uint16 [h, w], write keywords, meta) of slice `index`."""
    shape, name, _ = ENGINE_SLICES[index]
    write, meta = format_meta(name, ENGINE_SPACING)
    return format_store(name, engine_phantom(native, shape, index)), write, meta


def write_engine_set(native, d):
    """Writes the set as d/1-K.dcm (d is created) and returns the paths in order."""
    os.makedirs(str(d))
    files = []
    for k, (shape, name, bad) in enumerate(ENGINE_SLICES):
        raw, write, _ = engine_slice(native, k)
        blob = native.dicom_bytes(raw, instance=k + 1, **write)
        if bad == TRUNCATED:
            blob = blob[:len(blob) - raw.size]  # the 16-bit pixel data ends the file: half of it is gone
        path = os.path.join(str(d), f"1-{k + 1}.dcm")
        with open(path, "wb") as f:
            f.write(blob)
        files.append(path)
    return files


def good_indices():
    return [k for k, s in enumerate(ENGINE_SLICES) if s[2] is None]


# ---- the configurations both test files use -----------------------------------------------------------
# PipelineConfig keywords of the mixed cohort run (max_dim: the default 512 would refuse the 1030-row slices)
ENGINE_CFG = dict(batch_size=ENGINE_BATCH, streams=2, threads=4, measure=True, measure_diameters=True, measure_intensity=True,
                  measure_texture=True, texture_levels=64, overlay=True, min_dim=ENGINE_MIN_DIM, max_dim=ENGINE_MAX_DIM)
MEASURE_FLAGS = ("measure", "measure_diameters", "measure_intensity", "measure_texture")
# VolumePipeline keywords of the 3D runner tests (6-connected growing, 7³ cube: the command-line defaults)
VOLUME_KW = dict(connectivity=6, dilation=7, measure=True, measure_lesions=STRIDE_LESIONS, measure_diameters=True,
                 measure_intensity=True, measure_texture=True, texture_levels=STRIDE_LEVELS)
VOLUME_RUN_KW = dict(spacing=STRIDE_SPACING, spacing_z_source=STRIDE_Z_SOURCE)
