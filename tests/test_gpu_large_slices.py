"""GPU tests (MI355X) on 2D slices with a side between 1025 and kMaxSliceDim = 4096: the K2 global-memory
path with rows and columns beyond its 1024 threads, K7's 64-bit sums, K9's 12-bit key fields at 0xFFF,
K11's bins and K12's cells at 2²⁴ samples, K1 / K3 / K4 on more than 16 tiles a side and at 8× minification,
and the engine end to end, in mixed batches and at its limits. Inputs and their CPU checks: large_slice_cases.py, test_large_slice_cases.py.
Every comparison is of integers, bits or bytes (the sharpen against float64 keeps param_cases.sharpen_bound)."""
import functools
import io
import os
import shutil

import numpy as np
import pytest
import torch

import diameter_masks as dm
import large_slice_cases as lc
import measure_masks as mm
import nm03_capstone_project_amd as nm
import param_cases as pcs
import texture_cases as tc
from nm03_capstone_project_amd import ops
from nm03_capstone_project_amd.ops import reference as R

from conftest import run_bin

pytestmark = pytest.mark.gpu

PIL = pytest.importorskip("PIL.Image")

META = {"type": "u16", "stored_bits": 16, "slope": 1.0, "intercept": 0.0, "spacing_x": 1.0, "spacing_y": 1.0}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert nm.native().device_count() >= 1


def _cuda16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached masks are read-only


def _ids(v):
    return v if isinstance(v, str) else None


# ---------------------------------------------------------------------------------------------
# 1. K2: region growing and morphology beyond 1024 rows / columns
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", lc.K2_SHAPES)
def test_region_grow_rows_and_columns_beyond_the_workgroup(native, shape, conn):
    """The five bands of one shape in one launch: region, dilated, eroded and border against the golden
    model, the region also against scipy's labelling."""
    h, w = lc.SHAPES[shape]
    seeds = lc.k2_seeds(native.reference_seeds(w, h), h, w)
    bands = np.stack([lc.k2_band(name, h, w) for name in lc.K2_BANDS])
    out = ops.region_grow(torch.from_numpy(bands).cuda(), seeds, nm.PipelineConfig(srg_connectivity=conn))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for i, name in enumerate(lc.K2_BANDS):
        g = native.golden_region_grow(bands[i].astype(np.uint8), seeds, conn)
        assert lc.spans_wrap(g.astype(bool), h, w) and g.sum() < bands[i].sum(), name
        want = {"region": g, "dilated": native.golden_morph(g, 3, True), "eroded": native.golden_morph(g, 3, False),
                "border_region": native.golden_border(g, 2)}
        for k, gold in want.items():
            assert np.array_equal(out[k][i], gold.astype(bool)), f"{name}: {k} differs from the golden model"
        assert np.array_equal(out["region"][i], lc.label_region(bands[i], seeds, conn)), f"{name}: region vs scipy"


@pytest.mark.parametrize("conn", [4, 8])
def test_morphology_wide_shifts_across_17_words(native, conn):
    """Dilation 63, erosion 9 and border radius 5 at 70 × 1030: shifts of up to 31 bits across the 17
    words of a row, the last one partial, in row loops that wrap."""
    h, w = lc.SHAPES["cols_wrap"]
    band = lc.morph_band(h, w)
    seeds = lc.morph_seeds(native.reference_seeds(w, h), h, w)
    d, e, r = lc.MORPH_WIDE
    cfg = nm.PipelineConfig(srg_connectivity=conn, dilation_size=d, erosion_size=e, border_radius=r)
    out = ops.region_grow(torch.from_numpy(np.array(band)).cuda(), seeds, cfg)
    g = native.golden_region_grow(band.astype(np.uint8), seeds, conn)
    rt = torch.from_numpy(lc.label_region(band, seeds, conn))
    want = {"region": (g, rt), "dilated": (native.golden_morph(g, d, True, False), R.dilate(rt, d)),
            "eroded": (native.golden_morph(g, e, False, False), R.erode(rt, e)),
            "border_region": (native.golden_border(g, r), R.border(rt, r))}
    for k, (gold, ref) in want.items():
        gold = gold.astype(bool)
        assert 0 < gold.sum() < gold.size and gold[:, lc.WRAP:].any(), f"{k}: nothing in the 17th word proves nothing"
        got = out[k].cpu().numpy()
        assert np.array_equal(got, gold), f"{k} differs from the golden model"
        assert np.array_equal(got, ref.numpy()), f"{k} differs from the PyTorch reference"


# ---------------------------------------------------------------------------------------------
# 2. K7: measurements
# ---------------------------------------------------------------------------------------------
def _measure_gpu(masks, raws, conn):
    return ops.measure_mask([_dev(k) for k in masks], [_dev(mm.region_of(k)) for k in masks],
                            [_dev(r.view(np.int16)) for r in raws], conn, "u16", 16)


def _measure_golden(native, mask, raw, conn):
    return native.golden_measure(mask.astype(np.uint8), mm.region_of(mask).astype(np.uint8), raw, "u16", 16, conn)


def _check_full(got, h, w, raw):
    want = lc.full_closed_form(h, w, raw)
    assert {k: got[k] for k in want} == want, "full mask vs its closed form"


@pytest.mark.parametrize("conn", [4, 8])
def test_measure_every_named_mask_at_the_wrap_and_limit_shapes(native, conn):
    """Every measure_masks name at 1030 × 70, 70 × 1030, 4096 × 100 and 100 × 4096 in ONE mixed-size launch."""
    cases = [(s, name) for s in lc.MEASURE_SHAPES for name in mm.NAMES]
    masks = [mm.build(name, *lc.SHAPES[s]) for s, name in cases]
    raws = [mm.raw_of(*lc.SHAPES[s]) for s, _ in cases]
    got = _measure_gpu(masks, raws, conn)
    assert len(got) == len(cases)
    for (s, name), mask, raw, g in zip(cases, masks, raws, got):
        assert g == _measure_golden(native, mask, raw, conn), (s, name)
        if name == "full":
            _check_full(g, *lc.SHAPES[s], raw)
    by = {c: g for c, g in zip(cases, got)}
    assert by[("tall_limit", "one_pixel_br")]["bbox"] == [99, 4095, 99, 4095]
    assert by[("wide_limit", "one_pixel_br")]["bbox"] == [4095, 99, 4095, 99]
    assert by[("tall_limit", "serpentine")]["components"] == 1 and by[("wide_limit", "serpentine_v")]["components"] == 1


@pytest.mark.parametrize("conn", [4, 8])
def test_measure_sum_y_beyond_32_bits(native, conn):
    h, w = lc.SHAPES["sum64"]
    masks = [mm.build(name, h, w) for name in lc.SUM64_MASKS]
    raw = mm.raw_of(h, w)
    got = _measure_gpu(masks, [raw] * len(masks), conn)
    for name, mask, g in zip(lc.SUM64_MASKS, masks, got):
        assert g == _measure_golden(native, mask, raw, conn), name
    assert got[0]["sum_y"] == 600 * (4095 * 4096 // 2) > 2 ** 32
    _check_full(got[0], h, w, raw)
    assert got[1]["components"] == (h * w // 2 if conn == 4 else 1)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("names", [("full", "frame"), ("diag_main", "diag_anti"), ("blobs_diag", "bars_far")], ids="+".join)
def test_measure_4096_square(native, names, conn):
    """The full mask (Σx = Σy ≈ 3.4e10, raw_sum ≈ 5.5e11: all three sums need more than 32 bits) and the
    sparse masks at 4096 × 4096."""
    h, w = lc.SHAPES["square_limit"]
    masks = [lc.measure_mask(name, h, w) for name in names]
    raw = mm.raw_of(h, w)
    got = _measure_gpu(masks, [raw] * len(masks), conn)
    for name, mask, g in zip(names, masks, got):
        assert g == _measure_golden(native, mask, raw, conn), name
        assert g["bbox"][2:] == [4095, 4095], name
        if name == "full":
            _check_full(g, h, w, raw)
            assert min(g["sum_x"], g["sum_y"], g["raw_sum"]) > 2 ** 32
        if name.startswith("diag"):
            assert g["components"] == (4096 if conn == 4 else 1) and g["sum_y"] == 4095 * 4096 // 2


# ---------------------------------------------------------------------------------------------
# 2b. K11 / K12: intensity and texture
# ---------------------------------------------------------------------------------------------
def test_intensity_and_texture_4096_square(native):
    """Two slices of 4096 × 4096 in ONE launch of each op. The full homogeneous one: K11 has a single bin of
    2²⁴ samples, every percentile is the value and Σv² = 2²⁴ · v²; K12 a single cell 2 · (H(W − 1) + W(H − 1) +
    2(H − 1)(W − 1)) = 134 168 580 with half as many pairs: closed forms, and the golden model. Density 0.5
    with 16-bit noise: the golden model, and the NumPy references at this size too (3.4 s of CPU, measured
    once: sort + Python-integer squares 1.4 s, np.add.at 2 s), so no smaller stand-in is needed."""
    h, w = lc.SHAPES["square_limit"]
    v = 30000
    r = np.random.default_rng(4096)
    masks = [np.ones((h, w), bool), r.random((h, w)) < 0.5]
    raws = [np.full((h, w), v, np.uint16), r.integers(0, 65536, size=(h, w)).astype(np.uint16)]
    dm_, dr = [_dev(k) for k in masks], [_cuda16(x) for x in raws]
    gi = ops.measure_intensity(dm_, dr)
    gt = ops.measure_texture(dm_, dr, [32, 64])
    assert len(gi) == len(gt) == 2
    n = h * w
    assert n == 2 ** 24
    assert gi[0] == {"count": n, "raw_sum_sq": n * v * v, **{f"raw_p{p}": v for p in (10, 25, 50, 75, 90)}}
    cell = 2 * (h * (w - 1) + w * (h - 1) + 2 * (h - 1) * (w - 1))
    assert cell == 134168580
    assert gt[0]["glcm"][0, 0] == cell and np.count_nonzero(gt[0]["glcm"]) == 1
    assert (gt[0]["samples"], gt[0]["pairs"], gt[0]["key_lo"], gt[0]["key_hi"], gt[0]["levels"]) == (n, cell // 2, v, v, 32)
    for i, levels in enumerate((32, 64)):
        assert gi[i] == native.golden_measure_intensity(masks[i], raws[i], "u16", 16), i
        assert tc.same(gt[i], native.golden_measure_texture(masks[i], raws[i], levels, "u16", 16)), i
    assert gi[1] == R.measure_intensity(masks[1], raws[1])
    assert tc.same(gt[1], R.glcm(masks[1], raws[1], 64))
    assert gt[1]["samples"] == int(masks[1].sum()) and gt[1]["pairs"] > 2 ** 23  # about a quarter of the 4 · 2²⁴ neighbour pairs


K12_LARGE_SHAPES = ("both_wrap", "rows_wrap")  # 1100 × 1040 and 1030 × 70
K12_LARGE_MASKS = ("noise_0.593", "spiral", "comb")
K12_LARGE_LEVELS = (2, 63, 64)


def test_intensity_and_texture_ragged_masks_beyond_1024_rows(native):
    """large_slice_cases' ragged bands (a line across the wrap boundary, an island near the far corner) at
    1100 × 1040 and 1030 × 70 over 16-bit noise: every (shape, mask, level count) in ONE launch of
    ops.measure_texture and every (shape, mask) in one of ops.measure_intensity, against the golden model and
    the NumPy references."""
    r = np.random.default_rng(1100)
    raw = {s: r.integers(0, 65536, size=lc.SHAPES[s]).astype(np.uint16) for s in K12_LARGE_SHAPES}
    pairs = [(s, name) for s in K12_LARGE_SHAPES for name in K12_LARGE_MASKS]
    mask = {c: lc.k2_band(c[1], *lc.SHAPES[c[0]]) for c in pairs}
    dmask, draw = {c: _dev(mask[c]) for c in pairs}, {s: _cuda16(raw[s]) for s in K12_LARGE_SHAPES}
    gi = ops.measure_intensity([dmask[c] for c in pairs], [draw[c[0]] for c in pairs])
    cases = [(c, lv) for c in pairs for lv in K12_LARGE_LEVELS]
    gt = ops.measure_texture([dmask[c] for c, _ in cases], [draw[c[0]] for c, _ in cases], [lv for _, lv in cases])
    assert len(gi) == len(pairs) and len(gt) == len(cases)
    for c, g in zip(pairs, gi):
        ys = np.nonzero(mask[c])[0]
        assert ys.min() < lc.WRAP <= ys.max(), c
        assert g == native.golden_measure_intensity(mask[c], raw[c[0]], "u16", 16), c
        assert g == R.measure_intensity(mask[c], raw[c[0]]), c
    for (c, lv), g in zip(cases, gt):
        assert tc.same(g, native.golden_measure_texture(mask[c], raw[c[0]], lv, "u16", 16)), (c, lv)
        assert tc.same(g, R.glcm(mask[c], raw[c[0]], lv)), (c, lv)
        assert g["pairs"] > 0 and g["samples"] == int(mask[c].sum()), (c, lv)


# ---------------------------------------------------------------------------------------------
# 3. K9: diameters
# ---------------------------------------------------------------------------------------------
def _diam_gpu(masks, conn):
    return [dict(r) for r in ops.measure_diameters([_dev(k) for k in masks], conn)]


def _diam_golden(native, mask, conn):
    return dict(native.golden_measure_diameters(mask.astype(np.uint8), conn))


def _geometry(rec):
    return (rec["major_px2"], rec["major"], rec["perp_extent"], rec["perp"])


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", lc.MEASURE_SHAPES)
def test_diameters_every_named_mask(native, shape, conn):
    """Every diameter_masks name of one shape in one launch against the golden model; at the wide shapes
    (at most 200 row extremes) also against the brute force over the row extremes of scipy's lesion."""
    h, w = lc.SHAPES[shape]
    masks = [dm.build(name, h, w) for name in dm.NAMES]
    got = _diam_gpu(masks, conn)
    assert len(got) == len(dm.NAMES)
    for name, mask, g in zip(dm.NAMES, masks, got):
        assert g == _diam_golden(native, mask, conn), name
        if h <= lc.WRAP:
            bf = lc.brute_force_on_extremes(name, h, w, conn)
            assert bf is None and g["lesion_px"] == 0 or _geometry(g) == bf, f"{name} vs brute force"
    by = dict(zip(dm.NAMES, got))
    far = [w - 1, h - 1]
    assert by["one_pixel_br"]["major"] == far + far and by["full"]["major"] == [0, 0] + far
    assert by["full"]["major_px2"] == (w - 1) ** 2 + (h - 1) ** 2


def test_diameters_mixed_wrap_and_limit_shapes_in_one_launch(native):
    """Masks of the four shapes in one launch equal their own launches: descriptor offsets, scratch strides."""
    cases = [("rows_wrap", "rings3"), ("wide_limit", "frame_and_disc"), ("cols_wrap", "noise_0.593"), ("tall_limit", "serpentine")]
    masks = [dm.build(name, *lc.SHAPES[s]) for s, name in cases]
    batch = _diam_gpu(masks, 8)
    for k, c in enumerate(cases):
        assert batch[k] == _diam_gpu([masks[k]], 8)[0], c
        assert batch[k] == _diam_golden(native, masks[k], 8), c
    assert len({b["major_px2"] for b in batch}) == 4


@pytest.mark.parametrize("conn", [4, 8])
def test_diameters_sum64_shape(native, conn):
    h, w = lc.SHAPES["sum64"]
    masks = [mm.build(name, h, w) for name in lc.SUM64_MASKS]
    got = _diam_gpu(masks, conn)
    for name, mask, g in zip(lc.SUM64_MASKS, masks, got):
        assert g == _diam_golden(native, mask, conn), name
    assert got[0]["major"] == [0, 0, 599, 4095] and got[0]["lesion_px"] == h * w


_SPARSE_CASES = [(name, conn) for name in lc.SPARSE for conn in lc.SPARSE_CONN[name]]


@pytest.mark.parametrize("name,conn", _SPARSE_CASES, ids=lambda v: v if isinstance(v, str) else f"c{v}")
def test_diameters_sparse_masks_at_4096_square(native, name, conn):
    """All four 12-bit fields of the pair key and both of the projection keys at 0xFFF, d² and |p| at their
    bounds: the analytic record (endpoints, tie-breaks), the golden model and the brute force over the
    row extremes."""
    h, w = lc.SHAPES["square_limit"]
    mask = lc.sparse(name)
    g = _diam_gpu([mask], conn)[0]
    assert _geometry(g) == lc.SPARSE_EXPECT[name], "vs the analytic record"
    assert g["major_px2"] == 2 * 4095 ** 2
    assert g["lesion_px"] == int(mask.sum()), "one component"
    assert g == _diam_golden(native, mask, conn)
    assert _geometry(g) == lc.brute_force_on_extremes(name, h, w, 8), "vs brute force (one component at either connectivity)"
    if name == "diag_main":
        assert g["major"] == [0, 0, 4095, 4095]
    if name == "diag_anti":
        assert g["major"] == [4095, 0, 0, 4095]
    if name == "frame":
        assert g["major"] == [0, 0, 4095, 4095], "of the two tied diagonals the one from (0, 0)"


@pytest.mark.parametrize("conn", [4, 8])
def test_diameters_full_4096_square(native, conn):
    """8192 candidates: eight trips of the candidate loop, every row array entry in use."""
    h, w = lc.SHAPES["square_limit"]
    mask = mm.build("full", h, w)
    g = _diam_gpu([mask], conn)[0]
    assert g == _diam_golden(native, mask, conn)
    assert _geometry(g) == lc.SPARSE_EXPECT["frame"], "the full square has the frame's hull"


# ---------------------------------------------------------------------------------------------
# 4. K1a median, K1b sharpen + band
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _k1_raw(shape):
    h, w = lc.SHAPES[shape]
    return np.stack([pcs.noise12(h, w, h + w), lc.edge_ramp(h, w)])


@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("shape", lc.K1_SHAPES)
def test_median_more_than_16_tiles_a_side(native, shape, k):
    raw = _k1_raw(shape)
    med = ops.median2d(_cuda16(raw), k).cpu().numpy().view(np.uint16)
    for i, name in enumerate(("noise", "ramp")):
        assert np.array_equal(med[i], native.golden_median_u16(raw[i], k)), f"{name} vs golden"
        ref = R.median(torch.from_numpy(raw[i].astype(np.float32)).cuda(), k).cpu().numpy()
        assert np.array_equal(med[i].astype(np.float32), ref), f"{name} vs PyTorch"


@pytest.mark.parametrize("mask,variant", [(9, "default"), (15, "other")], ids=["mask9", "mask15_other"])
@pytest.mark.parametrize("shape", lc.K1_SHAPES)
def test_sharpen_band_more_than_16_tiles_a_side(native, shape, mask, variant):
    """Bit-exact against the golden model (values and band), within param_cases.sharpen_bound of float64."""
    raw = _k1_raw(shape)
    keys = np.stack([native.golden_median_u16(r, 7) for r in raw])
    gain, sigma, blo, bhi = pcs.sharpen_variant(mask, variant)
    cfg = nm.PipelineConfig(sharpen_mask=mask, sharpen_gain=gain, sharpen_sigma=sigma, srg_min=blo, srg_max=bhi)
    lo, hi = np.float32(blo), np.float32(bhi)
    s, band = ops.sharpen_band(_cuda16(keys), cfg)
    s, band = s.cpu().numpy(), band.cpu().numpy()
    for i, name in enumerate(("noise", "ramp")):
        c = native.golden_norm_clip(keys[i], "u16", 16, 1.0, 0.0, cfg.pipeline_params())
        gs = native.golden_sharpen(c, gain, sigma, mask, False)
        ref = R.sharpen(torch.from_numpy(c), gain, sigma, mask).numpy()
        bound = pcs.sharpen_bound(mask, gain, np.abs(c).max())
        err_golden, err_gpu = np.abs(gs - ref).max(), np.abs(s[i] - ref).max()
        print(f"{shape} {name} mask {mask}: |golden-f64| {err_golden:.3g} |gpu-f64| {err_gpu:.3g} bound {bound:.3g}")
        assert err_golden <= bound, "the derived bound must hold for the golden model itself"
        assert np.array_equal(s[i], gs), f"{name}: sharpened differs from the golden model"
        assert np.array_equal(band[i], (gs >= lo) & (gs <= hi)), f"{name}: band"
        assert err_gpu <= bound
    assert 0 < band[0].sum() < band[0].size, "the noise slice keeps both band edges busy"
    assert band[0][:, -6:].any() or band[0][-6:].any()


# ---------------------------------------------------------------------------------------------
# 5. K3: renders at 8× minification and extreme aspect
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engine_case(shape, out_w=512, out_h=512):
    """(raw, golden_run result with measurements and overlay) of the bridged phantom of a shape."""
    n = nm.native()
    h, w = lc.SHAPES[shape]
    raw = lc.bridged(n.phantom_slice(h, w, 3, 12, 25, 7), h, w)
    cfg = _engine_cfg(out_w, out_h)
    g = n.golden_run(raw, "u16", 16, 1.0, 0.0, cfg.pipeline_params(), cfg.render_params(), 1.0, 1.0)
    assert lc.spans_wrap(g["region"].astype(bool), h, w), "the region must span the wrap boundary"
    return raw, g


def _engine_cfg(out_w=512, out_h=512, **kw):
    return nm.PipelineConfig(max_dim=lc.LIMIT, batch_size=2, streams=1, threads=2, measure=True, measure_diameters=True,
                             measure_intensity=True, measure_texture=True, overlay=True, out_width=out_w, out_height=out_h, **kw)


@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("shape,out_w,out_h", lc.RENDER_CASES, ids=_ids)
def test_render_overlay_minified(native, shape, out_w, out_h, nearest):
    """ops.render_overlay of 4096 × 100, 100 × 4096 (8× minification, a 12-pixel strip) and 1100 × 1040
    against the golden model and ops.reference.overlay."""
    h, w = lc.SHAPES[shape]
    raw, g = _engine_case(shape)
    dil = g["dilated"]
    brd = native.golden_border(dil, 2)
    assert dil.sum() > brd.sum() > 0
    lo, hi = g["window"]
    color = (0, 255, 0) if not nearest else (255, 0, 128)
    want = native.golden_render_overlay(raw.astype(np.float32), dil, brd, lo, hi, 1.0, 1.0, out_w, out_h, nearest, 153, 255,
                                        list(color))
    t_dil, t_brd = torch.from_numpy(dil.astype(bool)), torch.from_numpy(brd.astype(bool))
    got = ops.render_overlay(_cuda16(raw), t_dil.cuda(), t_brd.cuda(), out_w=out_w, out_h=out_h, nearest=nearest, color=color)
    assert got.shape == (out_h, out_w, 3) and got.dtype == torch.uint8
    got = got.cpu().numpy()
    assert np.array_equal(got, want), "vs the golden model"
    ref = R.overlay(torch.from_numpy(raw.astype(np.float32)), lo, hi, t_dil, t_brd, out_w=out_w, out_h=out_h, nearest=nearest,
                    color=color)
    assert np.array_equal(got, ref.numpy()), "vs ops.reference.overlay"
    lit = want.any(axis=2)
    if max(h, w) == lc.LIMIT:
        assert min(lit.any(axis=0).sum(), lit.any(axis=1).sum()) in (12, 13), "the strip of the extreme aspect fit"
    assert (want[..., 1] != want[..., 0]).any(), "the overlay carries colour"


# ---------------------------------------------------------------------------------------------
# 6. Engine end to end
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_pipe():
    """One engine for slices up to 4096 (batch 2, one stream), shared by the end-to-end cases."""
    return nm.SlicePipeline(_engine_cfg())


def _write_dicoms(native, d, slices):
    d.mkdir()
    files = []
    for i, a in enumerate(slices, start=1):
        f = d / f"1-{i}.dcm"
        f.write_bytes(native.dicom_bytes(a))
        files.append(str(f))
    return files


def _tree(d):
    return {os.path.relpath(os.path.join(dp, f), d): open(os.path.join(dp, f), "rb").read()
            for dp, _, fs in os.walk(d) for f in fs}


@pytest.mark.parametrize("shape", lc.ENGINE_SHAPES)
def test_engine_end_to_end_large_slice(native, big_pipe, tmp_path, shape):
    """run_array against the golden model (planes, measurements, diameters, every JPEG) and the plain
    PyTorch renders, then the export run of the same slice: the golden model's files, none of them from the
    CPU fallback encoder."""
    h, w = lc.SHAPES[shape]
    raw, ref = _engine_case(shape)
    gpu = big_pipe.run_array(raw, META)
    assert np.array_equal(gpu["sharpened"], ref["sharpened"]), "sharpened"
    for k in ("band", "region", "dilated", "eroded"):
        assert np.array_equal(gpu[k], ref[k].astype(bool)), k
    assert gpu["measure"] == ref["measure"] and dict(gpu["diameters"]) == dict(ref["diameters"])
    assert gpu["intensity"] == ref["intensity"] and tc.same(gpu["texture"], ref["texture"])
    assert ref["texture"]["pairs"] > 0 and ref["intensity"]["count"] == ref["measure"]["area_px"] > 0
    assert gpu["measure_json"] == ref["measure_json"]
    assert max(ref["diameters"]["major"]) >= lc.WRAP
    assert gpu["jpegs"][0] == ref["jpeg_original"] and gpu["jpegs"][4] == ref["jpeg_processed"]
    assert np.array_equal(gpu["overlay"], ref["overlay"]) and gpu["jpeg_overlay"] == ref["jpeg_overlay"]
    # the five canvases against the plain-PyTorch renders (on the CPU), and every JPEG against the golden
    # encoder's bytes of its canvas
    canv = [np.asarray(c) for c in gpu["canvases"]]
    lo, hi = ref["window"]
    assert np.array_equal(canv[0], R.render_gray(torch.from_numpy(raw.astype(np.float32)), lo, hi).numpy()), "original"
    sh = ref["sharpened"]
    assert np.array_equal(canv[1], native.golden_render_gray(sh, float(sh.min()), float(sh.max()), 1.0, 1.0, 512, 512)), "sharpened"
    for k, plane in ((2, "region"), (3, "eroded"), (4, "dilated")):
        lab = torch.from_numpy(ref[plane].astype(bool))
        assert np.array_equal(canv[k], R.render_labels(lab, R.border(lab, 2)).numpy()), plane
    for k in range(5):
        assert gpu["jpegs"][k] == native.jpeg_encode_gray(canv[k], 75, 0), f"JPEG {k}"
    # export run
    out = tmp_path / "out"
    out.mkdir()
    files = _write_dicoms(native, tmp_path / "in", [raw])
    st, times = big_pipe.process([(files[0], str(out))])
    assert st[0][0] == 0, st
    assert times["jpeg_fallbacks"] == 0
    assert _tree(out) == {"1-1_original.jpg": ref["jpeg_original"], "1-1_processed.jpg": ref["jpeg_processed"],
                          "1-1_overlay.jpg": ref["jpeg_overlay"], "1-1_measure.json": ref["measure_json"].encode()}


def test_engine_end_to_end_nearest_and_384x512_canvas(native):
    """1100 × 1040 into a 384 × 512 canvas with the nearest gray filter: the generic fit on both axes."""
    cfg = _engine_cfg(384, 512, render_filter=1).replace(max_dim=1152)
    h, w = lc.SHAPES["both_wrap"]
    raw = lc.bridged(native.phantom_slice(h, w, 3, 12, 25, 7), h, w)
    pipe = nm.SlicePipeline(cfg)
    gpu, ref = pipe.run_array(raw, META), pipe.golden(raw, META)
    for k in ("band", "region", "dilated", "eroded"):
        assert np.array_equal(gpu[k], ref[k].astype(bool)), k
    assert gpu["jpegs"][0] == ref["jpeg_original"] and gpu["jpegs"][4] == ref["jpeg_processed"]
    assert np.array_equal(gpu["overlay"], ref["overlay"]) and gpu["jpeg_overlay"] == ref["jpeg_overlay"]
    assert gpu["measure_json"] == ref["measure_json"]
    assert gpu["intensity"] == ref["intensity"] and tc.same(gpu["texture"], ref["texture"])
    assert ref["texture"]["pairs"] > 0
    lo, hi = ref["window"]
    want = R.render_gray(torch.from_numpy(raw.astype(np.float32)), lo, hi, 384, 512, nearest=True).numpy()
    assert np.array_equal(np.asarray(gpu["canvases"][0]), want)
    lab = torch.from_numpy(ref["dilated"].astype(bool))
    assert np.array_equal(np.asarray(gpu["canvases"][4]), R.render_labels(lab, R.border(lab, 2), out_w=384, out_h=512).numpy())
    assert PIL.open(io.BytesIO(gpu["jpegs"][0])).size == (384, 512)


# ---------------------------------------------------------------------------------------------
# 7. Mixed batch, 8. limits
# ---------------------------------------------------------------------------------------------
def test_engine_mixed_batch_with_large_slices(native, tmp_path, monkeypatch):
    """One batch of a 256² cohort slice, 1030 × 70, 70 × 1030 and 4096 × 100, with 12-bit packing on and
    off: the same statuses, byte-identical trees, and every slice the golden model's files."""
    slices = [native.phantom_slice(256, 256, 3, 12, 25, 7)]
    for shape in ("rows_wrap", "cols_wrap", "tall_limit"):
        h, w = lc.SHAPES[shape]
        slices.append(lc.bridged(native.phantom_slice(h, w, 3, 12, 25, 7), h, w))
    files = _write_dicoms(native, tmp_path / "in", slices)
    cfg = nm.PipelineConfig(max_dim=lc.LIMIT, batch_size=4, streams=1, threads=2, measure_diameters=True,
                            measure_intensity=True, measure_texture=True, min_dim=lc.MIXED_MIN_DIM)  # the 70-pixel sides are below the default minimum of 100
    runs = []
    for i, flag in enumerate(["1", "0"]):
        monkeypatch.setenv("NM03_PACK12", flag)
        out = tmp_path / f"o{i}"
        out.mkdir()
        eng = native.Engine(cfg.engine_config())
        st, times = eng.run([(f, str(out)) for f in files])
        del eng
        assert times["batches"] == 1 and times["jpeg_fallbacks"] == 0
        runs.append(([c for c, _ in st], _tree(out)))
    assert runs[0][0] == runs[1][0] == [0, 0, 0, 0]
    assert runs[0][1] == runs[1][1] and len(runs[0][1]) == 12
    for k, f in enumerate(files, start=1):
        raw, meta = native.read_slice(f)
        g = native.golden_run(raw, meta["type"], meta["stored_bits"], meta["slope"], meta["intercept"], cfg.pipeline_params(),
                              cfg.render_params(), meta["spacing_x"], meta["spacing_y"])
        assert runs[0][1][f"1-{k}_processed.jpg"] == g["jpeg_processed"], k
        assert runs[0][1][f"1-{k}_original.jpg"] == g["jpeg_original"], k
        assert runs[0][1][f"1-{k}_measure.json"].decode() == g["measure_json"], k
        if k > 1:
            assert lc.spans_wrap(g["region"].astype(bool), *raw.shape), k


def test_engine_limits(native, tmp_path):
    """A 4097-wide file is refused with the engine's message and its neighbours in the batch succeed;
    max_dim = 4097 is refused at construction; the measurement wrappers refuse a 4097 side."""
    tall = lc.ROWS_WRAP_FILE
    slices = [native.phantom_slice(256, 256, 3, 12, 25, 7), np.zeros((100, lc.LIMIT + 1), np.uint16),
              lc.bridged(native.phantom_slice(tall[0], tall[1], 3, 12, 25, 7), *tall)]
    files = _write_dicoms(native, tmp_path / "in", slices)
    out = tmp_path / "out"
    out.mkdir()
    cfg = nm.PipelineConfig(max_dim=lc.LIMIT, batch_size=3, streams=1, threads=2)
    st, _ = native.Engine(cfg.engine_config()).run([(f, str(out)) for f in files])
    assert [c for c, _ in st] == [0, 1, 0], st
    assert "4097x100 exceed the engine limit 4096" in st[1][1]
    assert sorted(p.name for p in out.iterdir()) == ["1-1_original.jpg", "1-1_processed.jpg", "1-3_original.jpg",
                                                     "1-3_processed.jpg"]
    for k in (1, 3):
        g = native.golden_run(slices[k - 1])
        assert (out / f"1-{k}_processed.jpg").read_bytes() == g["jpeg_processed"]
        assert (out / f"1-{k}_original.jpg").read_bytes() == g["jpeg_original"]
    assert lc.spans_wrap(g["region"].astype(bool), *tall)
    with pytest.raises(RuntimeError, match="max_dim above 4096"):
        native.Engine(cfg.replace(max_dim=lc.LIMIT + 1).engine_config())
    for shape in ((100, lc.LIMIT + 1), (lc.LIMIT + 1, 100)):
        z = torch.zeros(shape, dtype=torch.bool, device="cuda")
        with pytest.raises(ValueError, match="bad slice size"):
            ops.measure_mask([z], [z], [torch.zeros(shape, dtype=torch.int16, device="cuda")])
        with pytest.raises(ValueError, match="bad mask size"):
            ops.measure_diameters([z])


def test_cli_parallel_sizes_buffers_for_a_1030_row_slice(native, cohort_root, tmp_path):
    """img_processing_parallel without --max-dim on a cohort holding a 1030 × 100 slice (rows_wrap at the
    tools' minimum width) sizes its buffers from the headers (1030 rounded up to 64: max_dim 1088) and
    writes the --cpu run's tree."""
    root = tmp_path / "data"
    shutil.copytree(cohort_root, root)
    base = native.cohort_dir(str(root) + "/")
    pid = native.find_patient_dirs(base)[0]
    series, _ = native.list_patient_series(base, pid)
    h, w = lc.ROWS_WRAP_FILE
    big = lc.bridged(native.phantom_slice(h, w, 3, 12, 25, 7), h, w)
    open(os.path.join(series, "1-99.dcm"), "wb").write(native.dicom_bytes(big))
    trees = {}
    for name, extra in (("gpu", []), ("cpu", ["--cpu"])):
        out = tmp_path / name
        r = run_bin("img_processing_parallel", *extra, "--data-root", str(root), "--out", str(out), "--quiet",
                    env={"NM03_LOG": "info"}, timeout=240)
        assert r.returncode == 0, (name, r.stderr)
        if name == "gpu":
            assert "max_dim 1088" in r.stdout
        trees[name] = _tree(out)
    assert trees["gpu"] == trees["cpu"]
    g = native.golden_run(big)
    assert lc.spans_wrap(g["region"].astype(bool), h, w)
    assert trees["gpu"][os.path.join(pid, "1-99_processed.jpg")] == g["jpeg_processed"]
    assert trees["gpu"][os.path.join(pid, "1-99_original.jpg")] == g["jpeg_original"]


# ---------------------------------------------------------------------------------------------
# K4: a 1024 × 1024 canvas
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["420", "444", "gray"])
def test_jpeg_1024_canvas(native, sampling):
    """64 workgroups per image in the encoder's look-back chain (36 at 768², the largest elsewhere): a
    phantom render and a label-like canvas at quality 75. Both fit the op's 512 KiB per image, so None
    is a failure; byte-identical to the golden encoder and to libjpeg."""
    samp = {"420": 0, "444": 1, "gray": 2}[sampling]  # ops.jpeg_encode's names → jpeg::Sampling
    ph = native.phantom_slice(256, 256, 3, 12, 25, 7).astype(np.float32)
    c = np.stack([native.golden_render_gray(ph, float(ph.min()), float(ph.max()), 1.0, 1.0, 1024, 1024),
                  pcs.label_canvas(1024, 1024)])
    assert c.shape == (2, 1024, 1024) and (1024 * 1024 // 64 + 255) // 256 == 64
    outs = ops.jpeg_encode(torch.from_numpy(c).cuda(), 75, sampling=sampling)
    for i, name in enumerate(("phantom", "labels")):
        assert outs[i] is not None, f"{name}: the encoder gave up on an image within its capacity"
        assert outs[i] == native.jpeg_encode_gray(c[i], 75, samp), f"{name} vs golden"
        bio = io.BytesIO()
        if samp == 2:
            PIL.fromarray(c[i]).save(bio, format="JPEG", quality=75)
        else:
            PIL.fromarray(c[i]).convert("RGB").save(bio, format="JPEG", quality=75, subsampling=2 if samp == 0 else 0)
        assert outs[i] == bio.getvalue(), f"{name} vs Pillow"
