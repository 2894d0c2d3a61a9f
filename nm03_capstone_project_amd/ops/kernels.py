"""torch wrappers of the HIP kernels. Shapes: [N, H, W] (a leading batch dim is added if missing).
Raw pixels are passed as torch.int16 / torch.uint16 tensors (16-bit storage, reinterpreted)."""
import torch

from .._native import native
from ..models.pipeline import PipelineConfig


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as3d(t):
    return t.unsqueeze(0) if t.dim() == 2 else t


def _check(t, dtypes, name):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (HIP) tensor")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} has dtype {t.dtype}, expected one of {dtypes}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


_U16 = (torch.int16, torch.uint16)


# The limits the engine's constructor enforces (engine.cpp): the kernels have no instance, tap table
# or shift width beyond them, so the wrappers reject such a configuration before any launch.
def _check_median(k):
    if int(k) not in (3, 5, 7, 9):
        raise ValueError(f"median window must be 3, 5, 7 or 9 (got {k})")


def _check_sharpen(cfg):
    if not 1 <= int(cfg.sharpen_mask) <= 15 or int(cfg.sharpen_mask) % 2 == 0:
        raise ValueError(f"sharpen mask must be odd and ≤ 15 (got {cfg.sharpen_mask})")


def _check_morph(cfg):
    if not (1 <= int(cfg.dilation_size) <= 63 and 1 <= int(cfg.erosion_size) <= 63):
        raise ValueError(f"morphology sizes must be in [1, 63] (got {cfg.dilation_size}, {cfg.erosion_size})")
    if not 0 <= int(cfg.border_radius) <= 31:
        raise ValueError(f"border radius must be in [0, 31] (got {cfg.border_radius})")


def median2d(raw, k=7, pixel_type="u16", stored_bits=16):
    """k×k median (clamp-to-edge) of raw 16-bit keys → same-shape tensor of median keys."""
    _check_median(k)
    x = _as3d(raw)
    _check(x, _U16, "raw")
    n, h, w = x.shape
    out = torch.empty_like(x)
    native().k_median(x.data_ptr(), out.data_ptr(), n, h, w, int(k), pixel_type, int(stored_bits), _stream())
    return out if raw.dim() == 3 else out[0]


def threshold(x, lo, hi):
    """BinaryThresholding: lo ≤ x ≤ hi → 1 (uint8), on an f32 CUDA tensor of any shape (K6)."""
    _check(x, (torch.float32,), "x")
    xc = x.contiguous()
    out = torch.empty(xc.shape, dtype=torch.uint8, device=xc.device)
    native().k_threshold(xc.data_ptr(), out.data_ptr(), xc.numel(), float(lo), float(hi), _stream())
    return out


def unpack_bits(words, width):
    """[N, H, wpr] int64 bit-planes → [N, H, width] bool (LSB = left-most pixel)."""
    sh = torch.arange(64, device=words.device, dtype=torch.int64)
    bits = (words.unsqueeze(-1) >> sh) & 1
    return bits.reshape(*words.shape[:-1], -1)[..., :width].bool()


def pack_bits(mask):
    """[N, H, W] bool → [N, H, ceil(W/64)] int64 words."""
    n, h, w = mask.shape
    wpr = (w + 63) // 64
    m = torch.zeros((n, h, wpr * 64), dtype=torch.int64, device=mask.device)
    m[..., :w] = mask.to(torch.int64)
    m = m.reshape(n, h, wpr, 64)
    sh = torch.arange(64, device=mask.device, dtype=torch.int64)
    return (m << sh).sum(-1)


def sharpen_band(median_keys, config: PipelineConfig = None, pixel_type="u16", stored_bits=16, slope=1.0,
                 intercept=0.0, want_sharpened=True):
    """normalise+clip(median keys) → 9×9 Gaussian unsharp mask → SRG band test.
    Returns (sharpened f32 [N,H,W] or None, band bool [N,H,W])."""
    cfg = config or PipelineConfig()
    _check_sharpen(cfg)
    x = _as3d(median_keys)
    _check(x, _U16, "median_keys")
    n, h, w = x.shape
    wpr = (w + 63) // 64
    band = torch.empty((n, h, wpr), dtype=torch.int64, device=x.device)
    sharp = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if want_sharpened else None
    native().k_sharpen_band(x.data_ptr(), band.data_ptr(), sharp.data_ptr() if sharp is not None else 0, n, h, w,
                            pixel_type, int(stored_bits), float(slope), float(intercept), cfg.pipeline_params(),
                            _stream())
    b = unpack_bits(band, w)
    if median_keys.dim() == 2:
        return (sharp[0] if sharp is not None else None), b[0]
    return sharp, b


def region_grow(band, seeds=None, config: PipelineConfig = None):
    """Seeded region growing on bool band [N,H,W] (LDS-resident ≤ 512², global-memory planes above) + dilation, erosion and the
    renderer border. Returns dict of bool tensors: region, dilated, eroded, border_region."""
    cfg = config or PipelineConfig()
    _check_morph(cfg)
    b = _as3d(band)
    if not b.is_cuda:
        raise ValueError("band must be a CUDA tensor")
    n, h, w = b.shape
    if seeds is None:
        seeds = [(x, y, 0) for (x, y) in native().reference_seeds(w, h)]
    words = pack_bits(b.bool()).contiguous()
    outs = {k: torch.zeros_like(words) for k in ("region", "dilated", "eroded", "border_region")}
    native().k_srg_morph(words.data_ptr(), outs["region"].data_ptr(), outs["dilated"].data_ptr(),
                         outs["eroded"].data_ptr(), outs["border_region"].data_ptr(), n, h, w, list(seeds),
                         cfg.pipeline_params(), int(cfg.border_radius), _stream())
    res = {k: unpack_bits(v, w) for k, v in outs.items()}
    if band.dim() == 2:
        res = {k: v[0] for k, v in res.items()}
    return res


# 3D mode (K5): the cube / ball size is odd and within the 2D engine's [1, 63] (the row shifts combine
# a word with one neighbour on each side), the connectivity is 6 or 26.
def _check_size3d(size):
    if not 1 <= int(size) <= 63 or int(size) % 2 == 0:
        raise ValueError(f"3D dilation size must be odd and in [1, 63] (got {size})")


def _check_conn3d(connectivity):
    if int(connectivity) not in (6, 26):
        raise ValueError(f"3D connectivity must be 6 or 26 (got {connectivity})")


def region_grow3d(band, seeds=(), connectivity=6, region=None):
    """3D seeded region growing (K5 plane sweeps; `connectivity` 6 or 26) on a bool band [D, H, W]
    (CUDA, every side ≤ 4096; planes that do not fit LDS run on global-memory scratch).
    `seeds` are (x, y, z) voxels; `region` (bool [D, H, W], ⊆ band) is grown further instead of
    starting from nothing — the z-slab decomposition re-grows a slab after its neighbours added
    boundary voxels. Returns (region bool [D, H, W], sweeps): the region is the fixpoint — the sweeps
    are bounded by the voxel count only, and a run that exhausted them would raise."""
    if band.dim() != 3 or not band.is_cuda:
        raise ValueError("band must be a CUDA tensor [D, H, W]")
    _check_conn3d(connectivity)
    d, h, w = band.shape
    bw = pack_bits(band.bool()).contiguous()
    rw = pack_bits(region.bool() & band.bool()).contiguous() if region is not None else torch.zeros_like(bw)
    sweeps = native().k_srg3d(bw.data_ptr(), rw.data_ptr(), w, h, d, [tuple(map(int, s)) for s in seeds],
                              int(connectivity), region is None, _stream())
    return unpack_bits(rw, w), sweeps


def dilate3d(mask, size=7, ball=False):
    """Cube dilation (size×size×size; `ball`: the digital ball of radius size//2) of a bool
    [D, H, W] CUDA mask, out-of-volume samples ignored. `size` is odd and in [1, 63]."""
    if mask.dim() != 3 or not mask.is_cuda:
        raise ValueError("mask must be a CUDA tensor [D, H, W]")
    _check_size3d(size)
    d, h, w = mask.shape
    src = pack_bits(mask.bool()).contiguous()
    dst, tmp = torch.empty_like(src), torch.empty_like(src)
    native().k_dilate3d(src.data_ptr(), dst.data_ptr(), tmp.data_ptr(), w, h, d, int(size), _stream(), bool(ball))
    return unpack_bits(dst, w)


def border3d(mask, radius=2):
    """Renderer border of every plane of a bool [D, H, W] CUDA mask: mask ∧ ¬erode of the
    (2·radius + 1)² square, in 2D per plane (out-of-plane samples ignored); radius in [0, 31]."""
    if mask.dim() != 3 or not mask.is_cuda:
        raise ValueError("mask must be a CUDA tensor [D, H, W]")
    if not 0 <= int(radius) <= 31:
        raise ValueError(f"border radius must be in [0, 31] (got {radius})")
    d, h, w = mask.shape
    src = pack_bits(mask.bool()).contiguous()
    dst = torch.empty_like(src)
    native().k_border3d(src.data_ptr(), dst.data_ptr(), w, h, d, int(radius), _stream())
    return unpack_bits(dst, w)


JPEG_SAMPLING = {"420": 0, "444": 1, "gray": 2}


def jpeg_encode(canvas, quality=75, header=True, sampling="420"):
    """GPU JPEG of uint8 gray canvases [N,H,W] (H, W multiples of 16) → list of bytes (complete
    JFIF files when header=True, else the entropy-coded segments). `sampling`: "420" (YCbCr
    4:2:0, the default), "444" (YCbCr 4:4:4) or "gray" (one component)."""
    c = _as3d(canvas)
    _check(c, (torch.uint8,), "canvas")
    n, h, w = c.shape
    samp = JPEG_SAMPLING[sampling] if isinstance(sampling, str) else int(sampling)
    segs = native().k_jpeg(c.data_ptr(), n, h, w, int(quality), _stream(), samp)
    if not header:
        return segs
    hdr = native().jpeg_header(w, h, int(quality), samp)
    return [None if s is None else hdr + s + b"\xff\xd9" for s in segs]


def jpeg_encode_rgb(canvas, quality=75, header=True, sampling="420", out_cap=0):
    """GPU colour JPEG of uint8 RGB canvases [N,H,W,3] (H, W multiples of 16) → list of bytes
    (complete JFIF files when header=True, else the entropy-coded segments). `sampling`: "420"
    (YCbCr 4:2:0, the default) or "444"; "gray" raises: one component cannot carry colour.
    `out_cap`: output bytes per image (0: the canvas size); an image that exceeds it comes back None."""
    c = canvas.unsqueeze(0) if canvas.dim() == 3 else canvas
    _check(c, (torch.uint8,), "canvas")
    if c.dim() != 4 or c.shape[3] != 3:
        raise ValueError("canvas must be [N, H, W, 3]")
    n, h, w, _ = c.shape
    samp = JPEG_SAMPLING[sampling] if isinstance(sampling, str) else int(sampling)
    if samp not in (0, 1):
        raise ValueError("a colour JPEG needs sampling '420' or '444'")
    segs = native().k_jpeg_rgb(c.data_ptr(), n, h, w, int(quality), _stream(), samp, int(out_cap))
    if not header:
        return segs
    hdr = native().jpeg_header(w, h, int(quality), samp)
    return [None if s is None else hdr + s + b"\xff\xd9" for s in segs]


def render_overlay(raw, label, border, spacing=(1.0, 1.0), out_w=512, out_h=512, pixel_type="u16", stored_bits=16,
                   slope=1.0, intercept=0.0, nearest=False, fill_a=153, border_a=255, color=(0, 255, 0)):
    """Overlay render (K3): the gray render of raw [N,H,W] (16-bit storage; window = each slice's
    min/max) with `color` blended over it at 8-bit opacity `border_a` where `border` is set, else
    `fill_a` where `label` is set (bool [N,H,W], sampled nearest) → uint8 [N, out_h, out_w, 3]."""
    x = _as3d(raw)
    _check(x, _U16, "raw")
    lab, brd = _as3d(label), _as3d(border)
    if lab.shape != x.shape or brd.shape != x.shape or not lab.is_cuda or not brd.is_cuda:
        raise ValueError("label and border must be CUDA tensors of raw's shape")
    n, h, w = x.shape
    # Raw keys (pixel_math.h key_from_raw): unsigned data masked to stored_bits, signed data
    # sign-extended and offset by 0x8000; their per-slice range is the render window.
    v = x.view(torch.int16).to(torch.int32)
    sh = 16 - int(stored_bits)
    if pixel_type == "i16":
        keys = (((v << (16 + sh)) >> (16 + sh)) + 0x8000) & 0xFFFF
    else:
        keys = (v & 0xFFFF) & (0xFFFF >> sh)
    kmin = [int(k) for k in keys.reshape(n, -1).min(dim=1).values.tolist()]
    kmax = [int(k) for k in keys.reshape(n, -1).max(dim=1).values.tolist()]
    planes = torch.stack([pack_bits(lab.bool()), pack_bits(brd.bool())]).contiguous()
    out = torch.empty((n, int(out_h), int(out_w), 3), dtype=torch.uint8, device=x.device)
    native().k_render_overlay(x.data_ptr(), planes.data_ptr(), out.data_ptr(), n, h, w, pixel_type, int(stored_bits),
                              float(slope), float(intercept), float(spacing[0]), float(spacing[1]), int(out_w), int(out_h),
                              bool(nearest), int(fill_a), int(border_a), [int(c) for c in color], kmin, kmax, _stream())
    return out if raw.dim() == 3 else out[0]


def measure_mask(dilated, region, raw, connectivity=8, pixel_type="u16", stored_bits=16):
    """Measurements of masks (K7, nm03/measure.h) → list of dicts of the record's integers: area_px,
    region_px, bbox [x0, y0, x1, y1], sum_x, sum_y, perimeter_edges, components, largest_px, holes
    (on `dilated`, components at `connectivity` 4 | 8, holes at its dual), raw_sum / raw_min / raw_max
    (the stored samples of `raw` under `dilated`) and region_px = popcount(`region`).

    `dilated`, `region` (bool) and `raw` (16-bit storage) are CUDA tensors [N, H, W] or [H, W], or
    lists of [H, W] tensors of ANY sizes: the whole batch is one launch, one workgroup per slice."""
    def as_list(t):
        if isinstance(t, (list, tuple)):
            return list(t)
        return list(_as3d(t))
    dl, rl, xl = as_list(dilated), as_list(region), as_list(raw)
    if not dl or len(rl) != len(dl) or len(xl) != len(dl):
        raise ValueError("dilated, region and raw must hold the same number of slices")
    hs, ws, dw, rw, xs = [], [], [], [], []
    for d, r, x in zip(dl, rl, xl):
        if d.dim() != 2 or r.shape != d.shape or x.shape != d.shape:
            raise ValueError("every slice needs dilated, region and raw of one [H, W] shape")
        if not (d.is_cuda and r.is_cuda):
            raise ValueError("masks must be CUDA (HIP) tensors")
        x = x.contiguous()
        _check(x, _U16, "raw")
        hs.append(int(d.shape[0]))
        ws.append(int(d.shape[1]))
        dw.append(pack_bits(d.bool().unsqueeze(0)).reshape(-1))
        rw.append(pack_bits(r.bool().unsqueeze(0)).reshape(-1))
        xs.append(x.reshape(-1).view(torch.int16))
    planes = torch.cat(dw + rw).contiguous()
    samples = torch.cat(xs).contiguous()
    return native().k_measure(planes.data_ptr(), samples.data_ptr(), hs, ws, pixel_type, int(stored_bits),
                              int(connectivity), _stream())


def measure_diameters(dilated, connectivity=8):
    """Bidimensional diameters of the lesion of masks (K7's labelling, then K9; nm03/measure.h
    SliceDiameters) → list of dicts of the record's integers: lesion_px and lesion_first [x, y] (the
    largest component at `connectivity` 4 | 8; a tie goes to the one whose first pixel in raster order
    comes first), major_px2 and major [xa, ya, xb, yb] (the pair of lesion pixels at maximum distance),
    perp_extent and perp [xc, yc, xd, yd] (the extent of the projection on the normal of b − a and the
    pixels that attain its ends). An empty mask gives zero counts and −1 coordinates.

    `dilated` is a bool CUDA tensor [N, H, W] or [H, W], or a list of [H, W] tensors of ANY sizes: the
    whole batch is one launch of each kernel, one workgroup per mask."""
    dl = list(dilated) if isinstance(dilated, (list, tuple)) else list(_as3d(dilated))
    if not dl:
        raise ValueError("no mask")
    hs, ws, dw = [], [], []
    for d in dl:
        if d.dim() != 2:
            raise ValueError("every mask must be [H, W]")
        if not d.is_cuda:
            raise ValueError("masks must be CUDA (HIP) tensors")
        hs.append(int(d.shape[0]))
        ws.append(int(d.shape[1]))
        dw.append(pack_bits(d.bool().unsqueeze(0)).reshape(-1))
    planes = torch.cat(dw).contiguous()
    # K7 also reads the samples under the mask; their values do not enter the diameters
    samples = torch.zeros(sum(h * w for h, w in zip(hs, ws)), dtype=torch.int16, device=planes.device)
    return native().k_measure_diameters(planes.data_ptr(), samples.data_ptr(), hs, ws, int(connectivity), _stream())


def measure_volume(dilated, region, raw, connectivity=26, pixel_type="u16", stored_bits=16):
    """Measurements of a volume mask (K8, nm03/measure.h VolumeMeasure) → dict of the record's integers:
    volume_vox, region_vox, bbox [x0, y0, z0, x1, y1, z1], sum_x / _y / _z, faces_x / _y / _z, components,
    largest_vox, cavities, euler (on `dilated`, components at `connectivity` 6 | 26, cavities at its
    dual), raw_sum / raw_min / raw_max (the stored samples of `raw` under `dilated`) and region_vox =
    popcount(`region`).

    `dilated`, `region` (bool) and `raw` (16-bit storage) are CUDA tensors [D, H, W] of one shape. The
    phases are separate launches of many workgroups; a volume with (W + 1)·H·D + 1 ≥ 2³² raises."""
    _check_conn3d(connectivity)
    if dilated.dim() != 3 or region.shape != dilated.shape or raw.shape != dilated.shape:
        raise ValueError("dilated, region and raw must be [D, H, W] of one shape")
    if not (dilated.is_cuda and region.is_cuda):
        raise ValueError("masks must be CUDA (HIP) tensors")
    x = raw.contiguous()
    _check(x, _U16, "raw")
    d, h, w = (int(v) for v in dilated.shape)
    if d < 1 or h < 1 or w < 1:
        raise ValueError("empty volume")
    dw = pack_bits(dilated.bool()).contiguous()
    rw = pack_bits(region.bool()).contiguous()
    return native().k_measure_volume(dw.data_ptr(), rw.data_ptr(), x.data_ptr(), w, h, d, pixel_type, int(stored_bits),
                                     int(connectivity), _stream())


def measure_volume_lesions(dilated, region, raw, max_lesions, connectivity=26, pixel_type="u16", stored_bits=16):
    """measure_volume plus one record per LESION (K10, nm03/measure.h VolumeLesion) → (record, lesions):
    `record` is measure_volume's dict; `lesions` lists the `max_lesions` (1 … 64) largest connected
    components of `dilated` at `connectivity`, largest first (a tie goes to the one whose first voxel in
    raster (z, y, x) order comes first; fewer components give a shorter list, an empty mask an empty
    one), each a dict of exact integers: voxels, first [x, y, z], bbox [x0, y0, z0, x1, y1, z1],
    sum_x / _y / _z, faces_x / _y / _z (the lesion's open voxel faces, as in the record) and
    raw_sum / raw_min / raw_max. Over all components the lesions' integers add up to the record's.

    The lesion launches run between K8's two passes, on the labelling the mask pass leaves behind."""
    _check_conn3d(connectivity)
    if not 1 <= int(max_lesions) <= 64:
        raise ValueError("max_lesions must be 1..64")
    if dilated.dim() != 3 or region.shape != dilated.shape or raw.shape != dilated.shape:
        raise ValueError("dilated, region and raw must be [D, H, W] of one shape")
    if not (dilated.is_cuda and region.is_cuda):
        raise ValueError("masks must be CUDA (HIP) tensors")
    x = raw.contiguous()
    _check(x, _U16, "raw")
    d, h, w = (int(v) for v in dilated.shape)
    if d < 1 or h < 1 or w < 1:
        raise ValueError("empty volume")
    dw = pack_bits(dilated.bool()).contiguous()
    rw = pack_bits(region.bool()).contiguous()
    rec, lesions = native().k_measure_volume_lesions(dw.data_ptr(), rw.data_ptr(), x.data_ptr(), w, h, d, int(max_lesions),
                                                     pixel_type, int(stored_bits), int(connectivity), _stream())
    return rec, lesions


def measure_volume_diameters(dilated, max_lesions, spacing_um=(1000, 1000, 1000), connectivity=26, brute_force=False):
    """The lengths of the `max_lesions` (1 … 64) largest connected components of a volume mask (K13,
    nm03/measure.h VolumeLesionDiameters) → list of dicts of exact integers, in measure_volume_lesions'
    order: major_um2 and major [xa, ya, za, xb, yb, zb] (the pair of lesion voxels at the largest distance,
    squared micrometres), axial_z, axial_um2 and axial [xa, ya, xb, yb] (the largest distance inside one
    plane), axial_perp_extent and axial_perp [xc, yc, xd, yd] (the extent of that plane's voxels on the
    normal of b − a, in index units, and the voxels at its ends). `spacing_um` is (ux, uy, uz) in integer
    micrometres; the maximisation is exact, ties go to the pair that comes first in raster order.

    `dilated` is a bool CUDA tensor [D, H, W]. Runs K8's mask pass, K10's selection and K13's seven launches.
    `brute_force` compares every tile pair instead of skipping those the bound excludes: the same records.
    A volume with (dim − 1)·u ≥ 2³¹ on an axis raises."""
    _check_conn3d(connectivity)
    if not 1 <= int(max_lesions) <= 64:
        raise ValueError("max_lesions must be 1..64")
    if dilated.dim() != 3:
        raise ValueError("dilated must be [D, H, W]")
    if not dilated.is_cuda:
        raise ValueError("masks must be CUDA (HIP) tensors")
    um = [int(v) for v in spacing_um]
    if len(um) != 3 or min(um) < 1:
        raise ValueError("spacing_um must be three integers of at least 1")
    d, h, w = (int(v) for v in dilated.shape)
    if d < 1 or h < 1 or w < 1:
        raise ValueError("empty volume")
    for dim, u, name in ((w, um[0], "(w - 1) * ux"), (h, um[1], "(h - 1) * uy"), (d, um[2], "(d - 1) * uz")):
        if (dim - 1) * u >= 2 ** 31:
            raise ValueError(f"the volume is too long to measure in micrometres: {name} = {dim - 1} * {u} must stay "
                             "below 2^31")
    dw = pack_bits(dilated.bool()).contiguous()
    # K8 and K10 also read the samples under the mask; their values do not enter the diameters
    samples = torch.zeros((d, h, w), dtype=torch.int16, device=dw.device)
    _, diameters, rest = native().k_measure_volume_diameters(dw.data_ptr(), samples.data_ptr(), w, h, d, int(max_lesions), um,
                                                             int(connectivity), bool(brute_force), _stream())
    zero = {k: ([0] * len(v) if isinstance(v, list) else 0) for r in rest[:1] for k, v in r.items()}
    if any(r != zero for r in rest):  # the kernel's contract: records past the count are zero
        raise RuntimeError("measure_volume_diameters: a record past the count is not zero")
    return diameters


def measure_intensity(dilated, raw, pixel_type="u16", stored_bits=16):
    """First-order intensity statistics of the stored samples of `raw` under masks (K11, nm03/measure.h
    IntensityStats) → list of dicts of the record's exact integers: count (= area_px), raw_sum_sq (Σ v²)
    and raw_p10 / raw_p25 / raw_p50 / raw_p75 / raw_p90, the k-th smallest sample with
    k = (p · count + 99) // 100 (nearest rank; raw_p50 is the lower median). An empty mask gives zeros.

    `dilated` (bool) and `raw` (16-bit storage) are CUDA tensors [N, H, W] or [H, W], or lists of [H, W]
    tensors of ANY sizes: the whole batch is one launch, one workgroup per mask (a two-pass radix select
    in LDS). `pixel_type` and `stored_bits` hold for every slice, or are lists with one entry per slice."""
    def as_list(t):
        if isinstance(t, (list, tuple)):
            return list(t)
        return list(_as3d(t))
    dl, xl = as_list(dilated), as_list(raw)
    if not dl or len(xl) != len(dl):
        raise ValueError("dilated and raw must hold the same number of slices")
    types = list(pixel_type) if isinstance(pixel_type, (list, tuple)) else [pixel_type] * len(dl)
    bits = [int(b) for b in stored_bits] if isinstance(stored_bits, (list, tuple)) else [int(stored_bits)] * len(dl)
    if len(types) != len(dl) or len(bits) != len(dl):
        raise ValueError("pixel_type and stored_bits lists need one entry per slice")
    if any(t not in ("u16", "i16", "u8") for t in types):
        raise ValueError("pixel_type must be u16, i16 or u8")
    if any(not 1 <= b <= 16 for b in bits):
        raise ValueError("stored_bits must be 1..16")
    hs, ws, dw, xs = [], [], [], []
    for d, x in zip(dl, xl):
        if d.dim() != 2 or x.shape != d.shape:
            raise ValueError("every slice needs dilated and raw of one [H, W] shape")
        if not d.is_cuda:
            raise ValueError("masks must be CUDA (HIP) tensors")
        x = x.contiguous()
        _check(x, _U16, "raw")
        hs.append(int(d.shape[0]))
        ws.append(int(d.shape[1]))
        dw.append(pack_bits(d.bool().unsqueeze(0)).reshape(-1))
        xs.append(x.reshape(-1).view(torch.int16))
    planes = torch.cat(dw).contiguous()
    samples = torch.cat(xs).contiguous()
    return native().k_measure_intensity(planes.data_ptr(), samples.data_ptr(), hs, ws, types, bits, _stream())


def measure_volume_intensity(dilated, raw, pixel_type="u16", stored_bits=16):
    """measure_intensity's record for a volume mask (K11's five 3D launches) → one dict: count
    (= volume_vox), raw_sum_sq and the five raw percentiles of the stored samples of `raw` under `dilated`.

    `dilated` (bool) and `raw` (16-bit storage) are CUDA tensors [D, H, W] of one shape; a volume with
    (W + 1)·H·D + 1 ≥ 2³² raises, as for measure_volume."""
    if dilated.dim() != 3 or raw.shape != dilated.shape:
        raise ValueError("dilated and raw must be [D, H, W] of one shape")
    if not dilated.is_cuda:
        raise ValueError("masks must be CUDA (HIP) tensors")
    if not 1 <= int(stored_bits) <= 16:
        raise ValueError("stored_bits must be 1..16")
    x = raw.contiguous()
    _check(x, _U16, "raw")
    d, h, w = (int(v) for v in dilated.shape)
    if d < 1 or h < 1 or w < 1:
        raise ValueError("empty volume")
    dw = pack_bits(dilated.bool()).contiguous()
    return native().k_measure_volume_intensity(dw.data_ptr(), x.data_ptr(), w, h, d, pixel_type, int(stored_bits),
                                               _stream())


def measure_texture(dilated, raw, levels=32, pixel_type="u16", stored_bits=16):
    """Grey-level co-occurrence matrices (GLCM) of the stored samples of `raw` under masks (K12,
    nm03/texture_core.h) → list of dicts: levels, key_lo, key_hi, samples, pairs and `glcm`, the
    [levels, levels] uint32 matrix. The samples are discretised to `levels` (2..64) grey levels between the
    smallest and largest of them; a pair is two mask pixels one index step apart in one of the four
    forward directions (1,0), (1,1), (0,1), (−1,1); the matrix is merged over them and symmetric, its sum
    2 · pairs. An empty mask gives zeros.

    `dilated` (bool) and `raw` (16-bit storage) are CUDA tensors [N, H, W] or [H, W], or lists of [H, W]
    tensors of ANY sizes: the whole batch is one launch, one workgroup per mask. `levels`, `pixel_type`
    and `stored_bits` hold for every slice, or are lists with one entry per slice."""
    def as_list(t):
        if isinstance(t, (list, tuple)):
            return list(t)
        return list(_as3d(t))
    dl, xl = as_list(dilated), as_list(raw)
    if not dl or len(xl) != len(dl):
        raise ValueError("dilated and raw must hold the same number of slices")
    lv = [int(v) for v in levels] if isinstance(levels, (list, tuple)) else [int(levels)] * len(dl)
    types = list(pixel_type) if isinstance(pixel_type, (list, tuple)) else [pixel_type] * len(dl)
    bits = [int(b) for b in stored_bits] if isinstance(stored_bits, (list, tuple)) else [int(stored_bits)] * len(dl)
    if len(types) != len(dl) or len(bits) != len(dl) or len(lv) != len(dl):
        raise ValueError("levels, pixel_type and stored_bits lists need one entry per slice")
    if any(t not in ("u16", "i16", "u8") for t in types):
        raise ValueError("pixel_type must be u16, i16 or u8")
    if any(not 1 <= b <= 16 for b in bits):
        raise ValueError("stored_bits must be 1..16")
    if any(not 2 <= v <= 64 for v in lv):
        raise ValueError("levels must be 2..64")
    hs, ws, dw, xs = [], [], [], []
    for d, x in zip(dl, xl):
        if d.dim() != 2 or x.shape != d.shape:
            raise ValueError("every slice needs dilated and raw of one [H, W] shape")
        if not d.is_cuda:
            raise ValueError("masks must be CUDA (HIP) tensors")
        x = x.contiguous()
        _check(x, _U16, "raw")
        hs.append(int(d.shape[0]))
        ws.append(int(d.shape[1]))
        dw.append(pack_bits(d.bool().unsqueeze(0)).reshape(-1))
        xs.append(x.reshape(-1).view(torch.int16))
    planes = torch.cat(dw).contiguous()
    samples = torch.cat(xs).contiguous()
    return native().k_measure_texture(planes.data_ptr(), samples.data_ptr(), hs, ws, lv, types, bits, _stream())


def measure_volume_texture(dilated, raw, levels=32, pixel_type="u16", stored_bits=16):
    """measure_texture's record for a volume mask (K12's four 3D launches) → one dict. The pairs are taken
    over the thirteen forward directions (dx, dy, dz) with components in {−1, 0, 1}: dz = 1, or dz = 0 and
    dy = 1, or dz = dy = 0 and dx = 1. Index steps: the voxel spacing is not consulted.

    `dilated` (bool) and `raw` (16-bit storage) are CUDA tensors [D, H, W] of one shape; a volume with
    (W + 1)·H·D + 1 ≥ 2³² raises, as for measure_volume, and so does a mask of more than 165 191 049 voxels:
    a 32-bit cell of the matrix can reach 2 · 13 · samples (nm03/texture_core.h cells_exact)."""
    if dilated.dim() != 3 or raw.shape != dilated.shape:
        raise ValueError("dilated and raw must be [D, H, W] of one shape")
    if not dilated.is_cuda:
        raise ValueError("masks must be CUDA (HIP) tensors")
    if not 1 <= int(stored_bits) <= 16:
        raise ValueError("stored_bits must be 1..16")
    if not 2 <= int(levels) <= 64:
        raise ValueError("levels must be 2..64")
    x = raw.contiguous()
    _check(x, _U16, "raw")
    d, h, w = (int(v) for v in dilated.shape)
    if d < 1 or h < 1 or w < 1:
        raise ValueError("empty volume")
    dw = pack_bits(dilated.bool()).contiguous()
    return native().k_measure_volume_texture(dw.data_ptr(), x.data_ptr(), w, h, d, int(levels), pixel_type,
                                             int(stored_bits), _stream())


def volume_views(raw, dilated, at="mask", pixel_type="u16", stored_bits=16, inverted=False, plane_stride=None, shape=None):
    """The six views of a volume that use its third axis (K14 alone, nm03/volume_views.h) → dict: width, height,
    depth, at_mode, at (x, y, z), mask_bbox ([x0, y0, z0, x1, y1, z1] or None for an empty mask), inverted and
    `views`, a dict name → {width, height, raw (uint16 [h, w]), mask (uint8 [h, w]), raw_min, raw_max, mask_px}
    for view_axial, view_coronal, view_sagittal (the planes z = at.z, y = at.y, x = at.x; the sagittal one has
    column = y, row = z) and mip_axial, mip_coronal, mip_sagittal (per pixel the sample that is largest as
    displayed along z, y, x — the smallest key when `inverted` — and the OR of the mask along the axis).

    `raw` (16-bit storage) and `dilated` (bool) are CUDA tensors [D, H, W]; `at` is "mask" (the centre of the
    mask's bounding box, the volume's centre when the mask is empty), "centre" or a voxel (x, y, z), which must
    lie inside the volume. With `plane_stride` (≥ H·W samples) and `shape` = (D, H, W), `raw` is instead a flat
    tensor whose plane z starts at sample z · plane_stride, as the 3D runner lays its planes out. Five launches
    (init, project, point, extract, count) on the current stream; the planes are copied back."""
    if dilated.dim() != 3:
        raise ValueError("dilated must be [D, H, W]")
    if not dilated.is_cuda:
        raise ValueError("masks must be CUDA (HIP) tensors")
    if not 1 <= int(stored_bits) <= 16:
        raise ValueError("stored_bits must be 1..16")
    if pixel_type not in ("u16", "i16", "u8"):
        raise ValueError("pixel_type must be u16, i16 or u8")
    d, h, w = (int(v) for v in dilated.shape)
    if d < 1 or h < 1 or w < 1:
        raise ValueError("empty volume")
    x = raw.contiguous()
    _check(x, _U16, "raw")
    if plane_stride is None:
        if tuple(raw.shape) != (d, h, w):
            raise ValueError("raw and dilated must be [D, H, W] of one shape")
        stride = h * w
    else:
        stride = int(plane_stride)
        if shape is None or tuple(int(v) for v in shape) != (d, h, w):
            raise ValueError("plane_stride needs shape = (D, H, W), the shape of dilated")
        if stride < h * w or x.numel() < (d - 1) * stride + h * w:
            raise ValueError("plane_stride must cover a plane and raw must hold every plane")
    if stride * d >= 2 ** 32:
        raise ValueError("volume too large: plane_stride * D must stay below 2^32")
    if not isinstance(at, str):
        at = tuple(int(v) for v in at)
        if len(at) != 3 or not (0 <= at[0] < w and 0 <= at[1] < h and 0 <= at[2] < d):
            raise ValueError(f"the point {at} lies outside the volume of {w} x {h} x {d}")
    elif at not in ("mask", "centre"):
        raise ValueError("at must be 'mask', 'centre' or (x, y, z)")
    dw = pack_bits(dilated.bool()).contiguous()
    return native().k_volume_views(x.data_ptr(), dw.data_ptr(), w, h, d, stride, at, pixel_type, int(stored_bits),
                                   bool(inverted), _stream())


def volume_mesh(mask, spacing=(1, 1, 1), placement="corner", scan_block=None, max_bytes=512 << 20):
    """The surface of a volume mask as a closed, indexed quad mesh (K15 alone, nm03/volume_mesh.h) → dict:
    vertices (float32 [V, 3], mm), quads (int32 [Q, 4]: the x-quads, then the y-quads, then the z-quads, each in
    raster order of their lattice position), quads_x, quads_y, quads_z, voxels, placement, width, height, depth.

    `mask` is a bool CUDA tensor [D, H, W]; `spacing` is (sx, sy, sz) in mm; `placement` is "corner" (vertices at
    the lattice corners, c − ½ in voxel index space) or "nets" (the mean of the midpoints of the window's
    crossing edges); the quads do not depend on it. `scan_block` (lattice words per block of the prefix scan,
    native().volume_mesh_scan_blocks() gives default, smallest and largest) does not change the result either.
    Four launches (classify, block totals, totals scan, downsweep), one host round trip that sizes the result
    — a mesh above `max_bytes` (12 per vertex, 16 per quad) raises RuntimeError — then vertices and quads."""
    if mask.dim() != 3:
        raise ValueError("mask must be [D, H, W]")
    if not mask.is_cuda:
        raise ValueError("masks must be CUDA (HIP) tensors")
    if placement not in ("corner", "nets"):
        raise ValueError("placement must be 'corner' or 'nets'")
    d, h, w = (int(v) for v in mask.shape)
    if d < 1 or h < 1 or w < 1:
        raise ValueError("empty volume")
    spacing = [float(v) for v in spacing]
    if len(spacing) != 3:
        raise ValueError("spacing must be (sx, sy, sz)")
    dw = pack_bits(mask.bool()).contiguous()
    return native().k_volume_mesh(dw.data_ptr(), w, h, d, spacing, placement, int(scan_block or 0), int(max_bytes), _stream())


def _distance_args(mask, spacing_um, name="mask"):
    if not hasattr(mask, "is_cuda") or not mask.is_cuda:
        raise ValueError(f"{name} must be a CUDA (HIP) tensor")
    if mask.dim() != 3:
        raise ValueError(f"{name} must be [D, H, W]")
    d, h, w = (int(v) for v in mask.shape)
    if d < 1 or h < 1 or w < 1:
        raise ValueError("empty volume")
    if w > 65535:
        raise ValueError("a row holds at most 65535 voxels")
    um = [int(v) for v in spacing_um]
    if len(um) != 3 or min(um) < 1 or max(um) > 2 ** 32 - 1:
        raise ValueError("spacing_um must be three integers of at least 1")
    err = native().volume_distance_extent_error(w, h, d, um)
    if err:
        raise ValueError(err)
    return d, h, w, um


def volume_distance(mask, spacing_um=(1000, 1000, 1000), to="foreground", cap_um=None):
    """The exact squared Euclidean distance map of a volume mask in physical space (K16, nm03/volume_distance.h)
    → int64 CUDA tensor [D, H, W]: at every voxel the smallest ((dx·ux)² + (dy·uy)² + (dz·uz)²) to a voxel of S,
    centre to centre, in squared micrometres. S is the set voxels of `mask` (`to="foreground"`) or its zero
    voxels inside the frame (`to="background"`); outside the frame is neither. The map is 0 exactly on S and
    native().NO_DISTANCE (2⁶³ − 1) everywhere when S is empty; with `cap_um` every value above cap_um² is
    NO_DISTANCE too.

    `mask` is a bool CUDA tensor [D, H, W]; `spacing_um` is (ux, uy, uz) in integer micrometres. Three launches
    (rows, columns, planes). A volume with ((w − 1)·ux)² + ((h − 1)·uy)² + ((d − 1)·uz)² ≥ 2⁶² raises."""
    if to not in ("foreground", "background"):
        raise ValueError("to must be 'foreground' or 'background'")
    d, h, w, um = _distance_args(mask, spacing_um)
    if cap_um is not None and int(cap_um) < 0:
        raise ValueError("cap_um must not be negative")
    bits = pack_bits(mask.bool()).contiguous()
    out = torch.empty((d, h, w), dtype=torch.int64, device=bits.device)
    native().k_volume_distance(bits.data_ptr(), w, h, d, um, "map", to == "background", -1 if cap_um is None else int(cap_um),
                               out.data_ptr(), _stream())
    return out


def dilate_volume_mm(mask, spacing_um=(1000, 1000, 1000), radius_um=0):
    """The margin of `radius_um` micrometres around a volume mask (K16): { p : D_mask(p) ≤ radius_um² } → bool
    CUDA tensor [D, H, W]. The ball is Euclidean in physical space; radius 0 gives the mask itself. The last
    pass stores the bits by wave ballot: no distance map is materialised."""
    d, h, w, um = _distance_args(mask, spacing_um)
    if int(radius_um) < 0:
        raise ValueError("radius_um must not be negative")
    bits = pack_bits(mask.bool()).contiguous()
    out = torch.empty_like(bits)
    native().k_volume_distance(bits.data_ptr(), w, h, d, um, "margin", False, int(radius_um), out.data_ptr(), _stream())
    return unpack_bits(out, w)


def volume_thickness(mask, spacing_um=(1000, 1000, 1000)):
    """The thickness of a volume mask (K16) → dict: inscribed_um2 (the largest squared distance of a mask voxel to
    the background of the frame), inscribed_at [x, y, z] (the voxel that attains it, the smallest raster
    (z, y, x) on a tie), found, inscribed_radius_mm = √inscribed_um2 / 1000 and thickness_mm = 2 · radius. An
    empty mask or a frame without a background voxel gives 0, [−1, −1, −1], found False and None."""
    d, h, w, um = _distance_args(mask, spacing_um)
    bits = pack_bits(mask.bool()).contiguous()
    return native().k_volume_distance(bits.data_ptr(), w, h, d, um, "thickness", True, -1, 0, _stream())


def compare_volumes(a, b, spacing_um=(1000, 1000, 1000), max_blocks=None):
    """Overlap and surface distances between two volume masks of one shape (K17, nm03/volume_compare.h) → the dict of
    integers: a_vox, b_vox, tp_vox, fp_vox, fn_vox, surface_a, surface_b (voxels with an open 6-face, outside the
    frame counting as open) and per direction n, max_um2, worst [x, y, z], sum_um, p95_um and found, suffixed _ab
    (from S(a) to S(b)) and _ba. Distances are surface to surface, centre to centre, in physical space:
    max_um2 is the largest squared distance in um², sum_um and p95_um are over ⌊√D⌋ in whole micrometres, the
    percentile by nearest rank. A direction is found when both surfaces are non-empty; otherwise its integers are
    0 and worst is [−1, −1, −1]. native().volume_compare_to_json gives the sidecar text with the derived values.

    `a`, `b`: bool CUDA tensors [D, H, W]; `spacing_um` is (ux, uy, uz) in integer micrometres. Twenty launches,
    K16's distance map twice among them. `max_blocks` lowers the cap on the workgroups of the sampling launches
    (the result does not depend on it)."""
    d, h, w, um = _distance_args(a, spacing_um, "a")
    if not hasattr(b, "is_cuda") or not b.is_cuda:
        raise ValueError("b must be a CUDA (HIP) tensor")
    if tuple(b.shape) != tuple(a.shape):
        raise ValueError("both masks must be [D, H, W] of one shape")
    if b.device != a.device:
        raise ValueError("both masks must be on one device")
    if w * h * d >= 2 ** 32:
        raise ValueError("a volume of 2^32 voxels or more cannot be compared")
    if max_blocks is not None and int(max_blocks) < 1:
        raise ValueError("max_blocks must be at least 1")
    wa = pack_bits(a.bool()).contiguous()
    wb = pack_bits(b.bool()).contiguous()
    return native().k_volume_compare(wa.data_ptr(), wb.data_ptr(), w, h, d, um, int(max_blocks or 0), _stream())


def compare_volume_lesions(a, b, max_lesions, connectivity=26, max_blocks=None):
    """Lesion-wise detection scores for two volume masks of one shape (K18, nm03/volume_compare_lesions.h) → a dict:
    connectivity, max_lesions, the totals over ALL connected components (lesions_a, hit_a, multi_a, lesions_b, hit_b,
    multi_b: a lesion is hit when it overlaps the other mask, multi when it meets at least two of its components),
    a_lesions and b_lesions (the `max_lesions` largest of each side, largest first, ties to the earlier first voxel:
    dicts of voxels, first [x, y, z], overlap_vox, partners_reported, overlap_other_vox, multi, best,
    best_overlap_vox) and table, an int64 tensor [N + 1, N + 1] of |A_i ∩ B_j| whose index N collects the unreported
    components of a side. native().volume_compare_to_json(..., lesions=…) gives the sidecar text with the derived values.

    `a`, `b`: bool CUDA tensors [D, H, W] (compare_volume_lesions_words takes their bit words). Ten launches. `max_blocks` lowers the cap on the workgroups of the
    join launch (the result does not depend on it)."""
    if not hasattr(a, "is_cuda") or not a.is_cuda:
        raise ValueError("a must be a CUDA (HIP) tensor")
    if not hasattr(b, "is_cuda") or not b.is_cuda:
        raise ValueError("b must be a CUDA (HIP) tensor")
    if a.dim() != 3 or tuple(b.shape) != tuple(a.shape):
        raise ValueError("both masks must be [D, H, W] of one shape")
    if b.device != a.device:
        raise ValueError("both masks must be on one device")
    d, h, w = (int(v) for v in a.shape)
    if min(d, h, w) < 1:
        raise ValueError("empty volume")
    wa = pack_bits(a.bool()).contiguous()
    wb = pack_bits(b.bool()).contiguous()
    return compare_volume_lesions_words(wa, wb, w, max_lesions, connectivity, max_blocks)


def compare_volume_lesions_words(wa, wb, width, max_lesions, connectivity=26, max_blocks=None):
    """compare_volume_lesions on the masks' bit words: int64 CUDA tensors [D, H, ceil(width / 64)], LSB = left-most
    voxel; bits past the width are tolerated."""
    for name, t in (("a", wa), ("b", wb)):
        if not hasattr(t, "is_cuda") or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 3:
            raise ValueError(f"{name} must be an int64 CUDA (HIP) tensor [D, H, ceil(width / 64)]")
    if tuple(wa.shape) != tuple(wb.shape) or wa.device != wb.device:
        raise ValueError("both word volumes must have one shape and one device")
    d, h, n = (int(v) for v in wa.shape)
    w = int(width)
    if min(d, h, w) < 1 or n != (w + 63) // 64:
        raise ValueError("the words must be [D, H, ceil(width / 64)]")
    if not 1 <= int(max_lesions) <= 64:
        raise ValueError("max_lesions must be 1..64")
    if int(connectivity) not in (6, 26):
        raise ValueError("connectivity must be 6 or 26")
    if (w + 1) * h * d + 1 >= 2 ** 32:
        raise ValueError("volume too large to measure: (w + 1) * h * d + 1 must stay below 2^32")
    if max_blocks is not None and int(max_blocks) < 1:
        raise ValueError("max_blocks must be at least 1")
    wa, wb = wa.contiguous(), wb.contiguous()
    res = native().k_volume_compare_lesions(wa.data_ptr(), wb.data_ptr(), w, h, d, int(max_lesions), int(connectivity),
                                            int(max_blocks or 0), _stream())
    res["table"] = torch.from_numpy(res["table"])
    return res
