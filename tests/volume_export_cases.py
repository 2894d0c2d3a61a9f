"""Cohorts and flag sets of the 3D export tests (test_volume_export_cases.py on the CPU,
test_gpu_volume_export.py on the GPU; not a conftest). Everything here is NumPy on the CPU plus the
native phantom and DICOM writer.

A cohort is a list of patients; a patient is a dict
    id      "PGBM-0NN"
    planes  uint16 [d, h, w]: the samples as they are stored (two's complement for signed data)
    write   keyword arguments of native.dicom_bytes (sample type, stored bits, rescale, spacing)
    meta    the same format as the golden model and VolumePipeline.run(meta=...) take it
written by write_cohort() as native.cohort_dir(root)/<id>/<series>/1-K.dcm.

  * deep      104 × 120 unsigned planes (w·h % 8 == 0, w % 4 == 0), patients of 33, 33 and 65 planes:
              the export encodes kExportSlices = 32 planes per launch (src/runtime/volume.cpp), so
              these are 2, 2 and 3 launches of 64, 2 | 64, 2 | 64, 64, 2 images on one set of
              export buffers.
  * deep_odd  101 × 131 signed planes, two patients of 33: w·h % 8 != 0 (padded plane stride), three
              mask words per row with a partial last one, per-pixel loads.
  * deep_2x   one patient of 33 signed 12-bit rescaled planes of 256²: the two launches with every
              image rendered inside the encoder (the exact-2× fit; deep and deep_odd go through K3
              canvases).
  * formats   9 planes of 120 × 104 with PixelSpacing 0.9 × 1.2 (no exact 2× fit: K3 canvases), one
              patient per sample format (FORMATS), the first plane of each constant.
  * formats_2x  the same formats, 3 planes of 256², square spacing (the fused exact-2× path).

All lesion planes are native.phantom_slice(h, w, patient, SLICE0 + k, NSLICES, seed): a window of a
long series placed where every patient has its lesion, so that the labels reach the last plane. The
phantom's enhancing rim lies at 1600–1720 (+ noise); the default band 0.74–0.91 of the normalised
value x / 10000 · 2 + 0.5 corresponds to rescaled values of 1200–2050. Every format below stores the
phantom so that its rescaled value is the phantom's (up to the format's quantisation)."""
import os

import numpy as np

EXPORT_SLICES = 32           # kExportSlices in src/runtime/volume.cpp (not exposed: asserted on the depths)
DEEP_SHAPE = (104, 120)      # h, w
DEEP_DEPTHS = (33, 33, 65)
DEEP_ODD_SHAPE = (101, 131)
DEEP_ODD_DEPTHS = (33, 33)
DEEP_2X_SHAPE = (256, 256)
DEEP_2X_DEPTH = 33
FORMATS_SHAPE = (120, 104)
FORMATS_DEPTH = 9
FORMATS_SPACING = (0.9, 1.2)  # x, y
FORMATS_2X_SHAPE = (256, 256)
FORMATS_2X_DEPTH = 3

NSLICES = 200                # length of the series the phantom planes are cut from
SEED = 41


def slice0(depth):
    """First phantom slice of a `depth`-plane window centred in the series (z = 0.5 ± depth / 400:
    inside every patient's lesion, which spans at least z = 0.25 … 0.75)."""
    return (NSLICES - depth) // 2


FLAG_SETS = (
    (),
    ("--quality", "100", "--jpeg-sampling", "444"),
    ("--quality", "10", "--jpeg-sampling", "gray"),
    ("--render-filter", "nearest"),                              # 4:2:0: the fused nearest instance
    ("--render-filter", "nearest", "--jpeg-sampling", "444"),    # labels fused, gray through canvases
    ("--median-window", "5", "--se-shape", "disc", "--dilation-size", "5", "--srg-connectivity", "26"),
)
# formats_2x runs these (the fused paths and their mixed launch)
FLAG_SETS_2X = (FLAG_SETS[0], FLAG_SETS[3], FLAG_SETS[4], FLAG_SETS[1])


def flags_id(flags):
    return "default" if not flags else "_".join(f.lstrip("-") for f in flags)


# ---- sample formats -----------------------------------------------------------------------------
def _u16(v):
    return np.asarray(v).astype(np.int64).astype(np.uint16)


def _store_neg1(p):
    """u16, slope −1, intercept 3250: stored 3250 − p (the phantom stays below 2540), value p."""
    return _u16(3250 - p)


def _quarters(p):
    """k with 2500 − 3k nearest to p, k ≥ 0: the slope −0.75 format stores 4k (value 2500 − 3k, an
    integer, so the format has a mirrored signed twin)."""
    return np.maximum(np.rint((2500 - p) / 3.0), 0).astype(np.int64)


def _store_neg075(p):
    return _u16(4 * _quarters(p))


def _store_i16(p):
    """i16, no rescale: p − 300 (air becomes negative, the rim 1300–1420)."""
    return _u16((p - 300) & 0xFFFF)


def _store_i12(p):
    """i16 with 12 stored bits, sign-extended words, intercept 500: stored p − 500 ≤ 2047."""
    return _u16(np.minimum(p - 500, 2047) & 0xFFFF)


def _store_u12(p):
    """u16 with 12 stored bits and garbage in the high nibble (every consumer masks it off)."""
    g = np.random.default_rng(int(p.sum()) & 0xFFFF).integers(0, 16, size=p.shape)
    return _u16((p & 0xFFF) | (g << 12))


def _store_u8(p):
    """8-bit samples p >> 4 with slope 16, intercept 8: value within 8 of p."""
    return _u16(np.minimum(p >> 4, 255))


def _store_pos075(p):
    """u16, slope 0.75, intercept −20: stored (p + 20) / 0.75."""
    return _u16(np.rint((p + 20) / 0.75))


# name, dicom type, stored bits, slope, intercept, store(p), constant first plane (stored word)
FORMATS = (
    ("u16_neg1", "u16", 16, -1.0, 3250.0, _store_neg1, 0),
    ("i16", "i16", 16, 1.0, 0.0, _store_i16, 0),
    ("u16_neg075", "u16", 16, -0.75, 2500.0, _store_neg075, 0xFFFF),
    ("i16_12", "i16", 12, 1.0, 500.0, _store_i12, 0),
    ("u16_12_garbage", "u16", 12, 1.0, 0.0, _store_u12, 0),
    ("u8", "u8", 8, 16.0, 8.0, _store_u8, 0),
    ("u16_pos075", "u16", 16, 0.75, -20.0, _store_pos075, 0),
)
# The order above alternates unsigned and signed as far as the formats allow (a reused runner must
# not keep the previous volume's descriptors).
FORMAT_NAMES = tuple(f[0] for f in FORMATS)
NEGATIVE_SLOPE = ("u16_neg1", "u16_neg075")


def format_meta(name, spacing=(1.0, 1.0)):
    """(write, meta) of a format: native.dicom_bytes keywords and the golden model's view (8-bit
    samples are imported as unsigned 16-bit words with 8 stored bits)."""
    _, ty, bits, slope, icpt, _, _ = FORMATS[FORMAT_NAMES.index(name)]
    rescale = slope != 1.0 or icpt != 0.0
    write = dict(type=ty, bits_stored=bits, write_rescale=rescale, slope=slope, intercept=icpt, spacing_x=spacing[0],
                 spacing_y=spacing[1])
    meta = dict(type="u16" if ty == "u8" else ty, stored_bits=bits, slope=slope, intercept=icpt, spacing_x=spacing[0],
                spacing_y=spacing[1])
    return write, meta


def format_store(name, phantom):
    """The stored words of phantom plane(s) `phantom` (uint16) in format `name`."""
    return FORMATS[FORMAT_NAMES.index(name)][5](np.asarray(phantom).astype(np.int64))


def mirrored(name, phantom):
    """The mirrored twin of a negative-slope format: the same values slope · stored + intercept as
    int16 words without a rescale (both value chains are exact in float32)."""
    _, _, _, slope, icpt, store, _ = FORMATS[FORMAT_NAMES.index(name)]
    assert slope < 0
    v = slope * store(np.asarray(phantom).astype(np.int64)).astype(np.float64) + icpt
    assert np.array_equal(v, np.rint(v)) and v.min() >= -32768 and v.max() <= 32767
    return _u16(v.astype(np.int64) & 0xFFFF)


_PLAIN = (dict(type="u16", bits_stored=16, write_rescale=False, slope=1.0, intercept=0.0, spacing_x=1.0, spacing_y=1.0),
          dict(type="u16", stored_bits=16, slope=1.0, intercept=0.0, spacing_x=1.0, spacing_y=1.0))


# ---- cohorts ------------------------------------------------------------------------------------
def _phantom_planes(native, shape, depth, patient, first=0):
    h, w = shape
    s0 = slice0(depth)
    return np.stack([native.phantom_slice(h, w, patient, s0 + k, NSLICES, SEED) for k in range(first, depth)])


def _patient(index, planes, write, meta):
    planes = np.ascontiguousarray(planes, dtype=np.uint16)
    planes.setflags(write=False)
    return dict(id=f"PGBM-{index + 1:03d}", planes=planes, write=write, meta=meta)


def deep(native, depths=DEEP_DEPTHS):
    return [_patient(i, _phantom_planes(native, DEEP_SHAPE, d, i), *_PLAIN) for i, d in enumerate(depths)]


def deep_odd(native):
    write = dict(_PLAIN[0], type="i16")
    meta = dict(_PLAIN[1], type="i16")
    return [_patient(i, _store_i16(_phantom_planes(native, DEEP_ODD_SHAPE, d, 5 + i).astype(np.int64)), write, meta)
            for i, d in enumerate(DEEP_ODD_DEPTHS)]


def deep_2x(native):
    name = "i16_12"
    planes = format_store(name, _phantom_planes(native, DEEP_2X_SHAPE, DEEP_2X_DEPTH, 8))
    return [dict(_patient(0, planes, *format_meta(name)), format=name)]


def _formats(native, shape, depth, spacing):
    out = []
    for i, (name, *_rest, const) in enumerate(FORMATS):
        lesion = format_store(name, _phantom_planes(native, shape, depth, 10 + i, first=1))
        planes = np.concatenate([np.full((1,) + tuple(shape), const, np.uint16), lesion])
        out.append(dict(_patient(i, planes, *format_meta(name, spacing)), format=name))
    return out


def formats(native):
    return _formats(native, FORMATS_SHAPE, FORMATS_DEPTH, FORMATS_SPACING)


def formats_2x(native):
    return _formats(native, FORMATS_2X_SHAPE, FORMATS_2X_DEPTH, (1.0, 1.0))


COHORTS = {"deep": deep, "deep_odd": deep_odd, "deep_2x": deep_2x, "formats": formats, "formats_2x": formats_2x}


def write_cohort(native, root, patients):
    """Writes `patients` under data root `root` (created) and returns the root with a trailing slash."""
    root = os.path.join(str(root), "")
    base = native.cohort_dir(root)
    for k, p in enumerate(patients):
        sdir = os.path.join(base, p["id"], f"{10 + k}.000000-T1post-{k:05d}")
        os.makedirs(sdir)
        for z, plane in enumerate(p["planes"]):
            with open(os.path.join(sdir, f"1-{z + 1}.dcm"), "wb") as f:
                f.write(native.dicom_bytes(plane, instance=z + 1, patient_id=p["id"], **p["write"]))
    return root


def chunks(depth):
    """The export launches of a `depth`-plane volume: ranges of plane indices."""
    return [range(z0, min(z0 + EXPORT_SLICES, depth)) for z0 in range(0, depth, EXPORT_SLICES)]


def golden_args(meta):
    """Positional (type, stored_bits, slope, intercept) of native.golden_run / golden_norm_clip."""
    return meta["type"], meta["stored_bits"], meta["slope"], meta["intercept"]
