"""The inputs of test_gpu_large_slices.py do what large_slice_cases.py claims (CPU only): every "first
reaches" property of its shapes, asserted from the golden model or NumPy alone, and the engine
constructor's guard of its 32-bit offsets."""
import numpy as np
import pytest

import diameter_masks as dm
import large_slice_cases as lc
import measure_masks as mm
import nm03_capstone_project_amd as nm

K2_THREADS = 1024  # k2_srg_morph.hip kSrgThreads, k7 / k9: kMeasureThreads, kDiamThreads


def test_shapes_reach_their_hazards():
    """The table of the module's docstring, in numbers."""
    words = lambda v: (v + 63) // 64
    h, w = lc.SHAPES["rows_wrap"]
    assert h > K2_THREADS and words(h) == 17 and w <= K2_THREADS      # a thread owns two rows; hb = 17
    h, w = lc.SHAPES["cols_wrap"]
    assert w > K2_THREADS and words(w) == 17 and w % 64 == 6           # the column fill wraps; n = 17, partial last word
    h, w = lc.SHAPES["both_wrap"]
    assert h > K2_THREADS and w > K2_THREADS and words(h) > 16 and words(w) > 16
    h, w = lc.SHAPES["tall_limit"]
    assert h == lc.LIMIT and words(h) == 64 and -(-h // K2_THREADS) == 4 and (h - 1) & 0x800
    h, w = lc.SHAPES["wide_limit"]
    assert w == lc.LIMIT and words(w) == 64 and w % 64 == 0 and -(-w // K2_THREADS) == 4
    h, w = lc.SHAPES["sum64"]
    assert w * (h * (h - 1) // 2) > 2 ** 32 > h * (w * (w - 1) // 2)   # Σy of the full mask alone passes 32 bits
    h, w = lc.SHAPES["square_limit"]
    assert h == w == lc.LIMIT == 0xFFF + 1
    assert 2 * (lc.LIMIT - 1) ** 2 < 2 ** 25 == 2 * lc.LIMIT ** 2      # K9's d² bound holds at 4095, and only just
    assert 2 * (lc.LIMIT - 1) ** 2 < 2 ** 26                           # and the projection's
    assert (w + 1) * h + 1 < 2 ** 32                                   # K7's u32 slot indices
    assert 2 * h == 8 * K2_THREADS                                     # K9's candidate loop: 8 trips


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", lc.K2_SHAPES)
def test_k2_bands_cross_the_wrap(native, shape, conn):
    """For every band: the golden region holds pixels at and beyond row / column 1024 of every long side,
    is not empty and not the whole band, and scipy's labelling gives the same region."""
    h, w = lc.SHAPES[shape]
    seeds = lc.k2_seeds(native.reference_seeds(w, h), h, w)
    assert len(seeds) > len(native.reference_seeds(w, h))
    for name in lc.K2_BANDS:
        band = lc.k2_band(name, h, w)
        g = native.golden_region_grow(band.astype(np.uint8), seeds, conn).astype(bool)
        assert lc.spans_wrap(g, h, w), name
        assert 0 < g.sum() < band.sum(), name
        assert not (g & ~band).any(), name
        ys, xs = np.nonzero(g)
        assert ys.max() == h - 1 or h <= lc.WRAP, name   # the far-end seeds' lines
        assert xs.max() == w - 1 or w <= lc.WRAP, name
        assert np.array_equal(g, lc.label_region(band, seeds, conn)), name


@pytest.mark.parametrize("conn", [4, 8])
def test_k2_wide_morphology_band(native, conn):
    h, w = lc.SHAPES["cols_wrap"]
    band = lc.morph_band(h, w)
    seeds = lc.morph_seeds(native.reference_seeds(w, h), h, w)
    g = native.golden_region_grow(band.astype(np.uint8), seeds, conn)
    assert 0 < g.sum() < band.sum() and lc.spans_wrap(g.astype(bool), h, w)
    d, e, r = lc.MORPH_WIDE
    for name, plane in (("dilated", native.golden_morph(g, d, True, False)), ("eroded", native.golden_morph(g, e, False, False)),
                        ("border", native.golden_border(g, r))):
        assert 0 < plane.sum() < plane.size, name
        assert plane[:, lc.WRAP:].any(), name  # every plane has content in the 17th word


def test_k7_sums_pass_32_bits(native):
    """sum_y > 2³² on the full mask at sum64; sum_x, sum_y and raw_sum > 2³² on the full mask at
    square_limit; the golden model agrees with the closed forms."""
    h, w = lc.SHAPES["sum64"]
    full, raw = mm.build("full", h, w), mm.raw_of(h, w)
    g = native.golden_measure(full.astype(np.uint8), mm.region_of(full).astype(np.uint8), raw, "u16", 16, 8)
    assert g["sum_y"] > 2 ** 32 and g["raw_sum"] > 2 ** 32
    want = lc.full_closed_form(h, w, raw)
    assert {k: g[k] for k in want} == want
    for name in lc.SUM64_MASKS:
        assert mm.build(name, h, w).any(), name
    h, w = lc.SHAPES["square_limit"]
    full, raw = mm.build("full", h, w), mm.raw_of(h, w)
    g = native.golden_measure(full.astype(np.uint8), mm.region_of(full).astype(np.uint8), raw, "u16", 16, 8)
    assert g["sum_x"] > 2 ** 32 and g["sum_y"] > 2 ** 32 and g["raw_sum"] > 2 ** 32
    want = lc.full_closed_form(h, w, raw)
    assert {k: g[k] for k in want} == want
    assert g["sum_x"] == g["sum_y"] == 4096 * (4095 * 4096 // 2) and g["sum_x"] > 3.4e10


@pytest.mark.parametrize("name", lc.SPARSE)
def test_k9_sparse_masks(native, name):
    """Each sparse mask is one component at the connectivities used; its analytic record holds 4095 in
    the claimed fields; the golden model and the brute force over the row extremes both give it."""
    from scipy import ndimage
    h, w = lc.SHAPES["square_limit"]
    mask = lc.sparse(name)
    assert mask.shape == (h, w)
    major_px2, major, perp_extent, perp = lc.SPARSE_EXPECT[name]
    for conn in (4, 8):
        _, ncomp = ndimage.label(mask, structure=ndimage.generate_binary_structure(2, 2 if conn == 8 else 1))
        assert (ncomp == 1) == (conn in lc.SPARSE_CONN[name]), (name, conn)
    assert major_px2 == 2 * 4095 ** 2 and sorted(major) == [0, 0, 4095, 4095]
    assert all(mask[major[1 + 2 * k], major[2 * k]] and mask[perp[1 + 2 * k], perp[2 * k]] for k in (0, 1))
    assert (major[1], major[0]) < (major[3], major[2]), "a comes before b in (y, x) order"
    if name in ("frame", "bars_far"):
        assert sorted(perp)[-2:] == [4095, 4095]
    if name == "bars_far":
        assert perp[:2] == [4095, 4095], "the projection key holds 0xFFF in both fields and |p| = 2 · 4095²"
    for conn in lc.SPARSE_CONN[name]:
        g = native.golden_measure_diameters(mask.astype(np.uint8), conn)
        assert (g["major_px2"], g["major"], g["perp_extent"], g["perp"]) == lc.SPARSE_EXPECT[name], conn
        assert g["lesion_px"] == int(mask.sum())
    assert lc.brute_force_on_extremes(name, h, w, lc.SPARSE_CONN[name][-1]) == lc.SPARSE_EXPECT[name]


def test_frame_is_the_tie_break_case():
    """On the frame both diagonals of the square attain the maximum: the record takes a = (0, 0)."""
    f = lc.LIMIT - 1
    assert lc.SPARSE_EXPECT["frame"][1] == [0, 0, f, f] and lc.SPARSE_EXPECT["diag_anti"][1] == [f, 0, 0, f]
    m = lc.sparse("frame")
    assert m[0, 0] and m[0, f] and m[f, 0] and m[f, f]


def test_a_key_field_narrowed_to_11_bits_changes_every_sparse_record():
    """What a `& 0x7FF` in K9's unpacking would give: every expected record differs (the GPU test fails)."""
    for name, (_, major, _, perp) in lc.SPARSE_EXPECT.items():
        assert [v & 0x7FF for v in major] != major, name
    assert [v & 0x7FF for v in lc.SPARSE_EXPECT["bars_far"][3]] != lc.SPARSE_EXPECT["bars_far"][3]


def test_row_extremes_and_lesion(native):
    """row_extremes / lesion_of on a mask small enough for the full brute force."""
    for name in ("frame_and_disc", "rings3", "noise_0.593", "word_span"):
        mask = dm.build(name, 100, 100)
        for conn in (4, 8):
            les = lc.lesion_of(mask, conn)
            g = native.golden_measure_diameters(mask.astype(np.uint8), conn)
            assert int(les.sum()) == g["lesion_px"]
            ext = lc.row_extremes(les)
            assert not (ext & ~les).any() and ext.sum() <= 2 * les.any(axis=1).sum()
            assert dm.brute_force(ext) == dm.brute_force(les) == (g["major_px2"], g["major"], g["perp_extent"], g["perp"])


def test_k1_inputs():
    for shape in lc.K1_SHAPES:
        h, w = lc.SHAPES[shape]
        r = lc.edge_ramp(h, w)
        assert r.dtype == np.uint16 and r.max() < 4096
        # distinct values along the last tile column and the last tile row (tiles are 64 × 64)
        x0, y0 = (w - 1) // 64 * 64, (h - 1) // 64 * 64
        assert (np.diff(r[:, x0:].astype(int), axis=1) != 0).all() and (np.diff(r[y0:].astype(int), axis=0) != 0).all()
        assert r[0, w - 1] != r[0, x0 - 1] and r[h - 1, 0] != r[y0 - 1, 0]
        assert max(-(-w // 64), -(-h // 64)) > 16, "more than 16 tiles on a side"


@pytest.mark.parametrize("shape", lc.ENGINE_SHAPES)
def test_engine_content_spans_the_wrap(native, shape):
    """The bridged phantom's golden region spans row / column 1024 of every long side, and the dilated
    mask (what K7 and K9 measure) is a lesion with a coordinate at or above 1024."""
    h, w = lc.SHAPES[shape]
    raw = lc.bridged(native.phantom_slice(h, w, 3, 12, 25, 7), h, w)
    cfg = nm.PipelineConfig(measure=True, measure_diameters=True, overlay=True)
    g = native.golden_run(raw, "u16", 16, 1.0, 0.0, cfg.pipeline_params(), cfg.render_params(), 1.0, 1.0)
    assert lc.spans_wrap(g["region"].astype(bool), h, w)
    assert 0 < g["region"].sum() < g["band"].sum() <= h * w
    assert max(g["diameters"]["major"]) >= lc.WRAP and g["diameters"]["major_px2"] >= (max(h, w) - 1 - 2 * 40) ** 2
    assert g["measure"]["area_px"] == g["dilated"].sum() > 0


def test_file_shapes_respect_the_engine_minimum(native):
    """The 70-pixel sides of rows_wrap / cols_wrap are below the engine's default minimum, which the
    command-line tools cannot change: the shape that goes through them keeps rows_wrap's hazards."""
    assert nm.PipelineConfig().min_dim == 100
    assert min(lc.SHAPES["rows_wrap"]) == min(lc.SHAPES["cols_wrap"]) == 70 >= lc.MIXED_MIN_DIM
    h, w = lc.ROWS_WRAP_FILE
    assert h == lc.SHAPES["rows_wrap"][0] > K2_THREADS and (h + 63) // 64 == 17 and w == 100
    assert (h + 63) // 64 * 64 == 1088  # what the parallel tool sizes its buffers to
    g = native.golden_run(lc.bridged(native.phantom_slice(h, w, 3, 12, 25, 7), h, w))
    assert lc.spans_wrap(g["region"].astype(bool), h, w)
    for shape in ("rows_wrap", "cols_wrap"):
        hh, ww = lc.SHAPES[shape]
        p = nm.PipelineConfig(min_dim=lc.MIXED_MIN_DIM)
        g = native.golden_run(lc.bridged(native.phantom_slice(hh, ww, 3, 12, 25, 7), hh, ww), "u16", 16, 1.0, 0.0,
                              p.pipeline_params(), p.render_params(), 1.0, 1.0)
        assert lc.spans_wrap(g["region"].astype(bool), hh, ww), shape


# ---- the engine's 32-bit offsets ---------------------------------------------------------------------
def _host_cfg(native, **kw):
    """A host-only EngineConfig: its engine is built and run without a GPU."""
    return nm.PipelineConfig(threads=1, streams=1, host_only=True, **kw).engine_config()


def test_engine_rejects_a_batch_beyond_32_bit_offsets(native):
    """SliceDesc::raw_off / f32_off and RenderDesc::src_off are u32 element offsets into buffers of
    batch_size × max_dim² samples, JpegDesc / RenderDesc::canvas_off u32 byte offsets into the canvases:
    a configuration whose products reach 2³² is refused by the constructor, before any allocation
    (the refused ones here would need 34 GB and more), with both numbers in the message."""
    with pytest.raises(RuntimeError, match=r"batch_size 256 .* max_dim 4096"):
        native.Engine(_host_cfg(native, batch_size=256, max_dim=4096))
    with pytest.raises(RuntimeError, match=r"batch_size 1024 .* max_dim 2048"):
        native.Engine(_host_cfg(native, batch_size=1024, max_dim=2048))
    with pytest.raises(RuntimeError, match=r"2048 canvases .* 2048 x 1024"):
        native.Engine(_host_cfg(native, batch_size=1024, max_dim=64, out_width=2048, out_height=1024))
    # the overlay's canvases are three bytes per pixel: a third of the count already overflows
    ov = nm.PipelineConfig(threads=1, streams=1, batch_size=400, max_dim=64, out_width=2048, out_height=2048, overlay=True,
                           device=0)
    with pytest.raises(RuntimeError, match=r"400 overlay canvases .* 2048 x 2048"):
        native.Engine(ov.engine_config())
    with pytest.raises(RuntimeError, match="max_dim above 4096"):
        native.Engine(_host_cfg(native, batch_size=1, max_dim=4097))
