"""The JPEG stream cases (jpeg_stream_cases.py) meet their own conditions: CPU only, on the golden
encoder's bytes. Each case is libjpeg's stream (Pillow), the scan walker accounts for every bit of
it, and the branch of the GPU encoders that the case is named for is really taken — ZRL runs, DC
category 11, AC category 10, blocks without EOB, 0xFF across a part edge at every alignment and in
the padded last byte, exact half quotients, and both sides of the LDS range limit. The GPU test
(test_gpu_jpeg_streams.py) then only compares bytes. Run with -s for the walker's figures per case."""
import io

import numpy as np
import pytest

import jpeg_stream_cases as jc
import nm03_capstone_project_amd as nm
from overlay_images import pillow_jpeg

_SAMPLING = {"420": 0, "444": 1, "gray": 2}


def _pil_gray(gray, q, sampling):
    """tests/test_gpu_params.py::_pil_gray. Without Pillow only this comparison is skipped, after the
    case's other checks."""
    PIL = pytest.importorskip("PIL.Image")
    bio = io.BytesIO()
    if sampling == 2:
        PIL.fromarray(gray).save(bio, format="JPEG", quality=q)
    else:
        PIL.fromarray(gray).convert("RGB").save(bio, format="JPEG", quality=q, subsampling=2 if sampling == 0 else 0)
    return bio.getvalue()


def _gray_registry():
    """{name: (quality, image)} of every gray case, the launches' extra images included."""
    reg = {}
    for (q, shape), cases in jc.gray_cases().items():
        for name, img in cases.items():
            assert img.shape == shape and img.dtype == np.uint8
            reg[f"{name}_{shape[0]}x{shape[1]}_q{q}"] = (q, img)
    for cases in (jc.edge_cases(), jc.edge3_cases()):
        for name, img in cases.items():
            reg[name] = (100, img)
    for shape in jc.LIMIT_SHAPES:
        for name, img in jc.limit_launch(shape).items():
            assert img.shape == shape
            reg[f"limit{shape[1]}_{name}"] = (100, img)
    return reg


def _rgb_registry(sampling):
    reg = {}
    for (q, shape), cases in jc.rgb_cases(sampling).items():
        for name, img in cases.items():
            assert img.shape == shape + (3,) and img.dtype == np.uint8
            reg[f"{name}_{shape[0]}x{shape[1]}_q{q}"] = (q, img)
    for name, img in jc.rgb_limit_launch(sampling).items():
        reg[f"limit_{name}"] = (100, img)
    return reg


_GRAY = _gray_registry()
_RGB = {s: _rgb_registry(s) for s in ("420", "444")}
# the only cases with a part over the range limit
_OVER = {"limit128_binary_noise", "limit256_binary_noise", "limit_rgb_over_limit"}


@pytest.fixture(scope="module")
def walked():
    """(encoder, name, sampling) → (golden bytes, Stream, Parts), walked once."""
    native = nm.native()
    cache = {}

    def get(encoder, name, sampling):
        key = (encoder, name, sampling)
        if key not in cache:
            q, img = (_GRAY[name] if encoder == "gray" else _RGB[sampling][name])
            enc = native.jpeg_encode_gray if encoder == "gray" else native.jpeg_encode_rgb
            j = enc(img, q, _SAMPLING[sampling])
            st = jc.walk(j)
            cache[key] = (j, st, jc.parts(st, encoder))
        return cache[key]
    return get


def _pil_rgb(rgb, q, sampling):
    pytest.importorskip("PIL.Image")
    return pillow_jpeg(rgb, q, sampling)


def _check_stream(name, sampling, j, st, p, pillow):
    """`pillow`: a call that gives libjpeg's file, made last."""
    print(f"{name} {sampling}: {st.summary()} parts {p.length} al {p.al} straddle_ff {p.straddle_ff} "
          f"final {p.final_rem} {p.final_ff} bytes {len(j)}")
    # the walker's own account: every bit, the padding, the stuffing
    assert (st.total_bits + 7) // 8 == len(st.unstuffed)
    assert jc.restuff(st) == st.segment
    assert sum(st.bits) == st.total_bits and sum(p.length) == st.total_bits
    assert len(st.segment) == len(st.unstuffed) + st.ff_bytes
    assert len(st.segment) < jc.GRAY_OUT_CAP, "within the op's output capacity"
    if name not in _OVER:
        assert max(p.length) < jc.RANGE_LIMIT_BITS, "only the named cases may exceed the range limit"
    assert j == pillow(), "golden encoder vs libjpeg"


@pytest.mark.parametrize("sampling", ["gray", "420", "444"])
@pytest.mark.parametrize("name", sorted(_GRAY))
def test_gray_case_is_libjpegs_and_walks(walked, name, sampling):
    q, img = _GRAY[name]
    j, st, p = walked("gray", name, sampling)
    if sampling != "gray":
        # every MCU ends in the chroma blocks' zero bits: no part edge and no last byte can be 0xFF
        assert not any(p.straddle_ff) and not p.final_ff
    _check_stream(name, sampling, j, st, p, lambda: _pil_gray(img, q, _SAMPLING[sampling]))


@pytest.mark.parametrize("sampling", ["420", "444"])
@pytest.mark.parametrize("name", sorted(_RGB["420"]))
def test_rgb_case_is_libjpegs_and_walks(walked, name, sampling):
    assert sorted(_RGB["420"]) == sorted(_RGB["444"])
    q, img = _RGB[sampling][name]
    j, st, p = walked("rgb", name, sampling)
    assert p.mcus_per_part == (42 if sampling == "420" else 85)
    _check_stream(name, sampling, j, st, p, lambda: _pil_rgb(img, q, _SAMPLING[sampling]))


def test_part_sizes_are_the_kernels():
    assert jc.gray_mcus_per_part(4) == 64 and jc.gray_mcus_per_part(1) == 256
    assert jc.rgb_mcus_per_part(6) == 42 and jc.rgb_mcus_per_part(3) == 85
    assert jc.RANGE_LIMIT_BITS == (6912 - 2) * 32 == 221120   # kUnionWords, src/kernels/k4_jpeg.hip


@pytest.mark.parametrize("name", ["sparse_hf_a_48x80_q50", "sparse_hf_b_48x80_q50", "sparse_hf_272x400_q50"])
@pytest.mark.parametrize("sampling", ["gray", "420", "444"])
def test_sparse_hf_takes_the_zrl_loop(walked, name, sampling):
    _, st, p = walked("gray", name, sampling)
    hist = st.zrl_histogram()
    assert all(hist.get(k, 0) > 0 for k in (1, 2, 3)), hist   # the ZRL loop runs one, two and three times
    assert max(hist) == 3
    assert st.eob.count(False) >= 1, "a block must end on coefficient 63"
    assert st.ff_share() >= 0.05
    if name.startswith("sparse_hf_272"):
        assert len(p.length) == 7 and all(s % (400 // 8) for s in range(256, 1700, 256)), "parts start mid-row"


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_rgb_sparse_hf_takes_the_zrl_loop_in_chroma(walked, sampling):
    for name in ("rgb_sparse_hf_48x80_q50", "rgb_sparse_hf_parts_64x256_q50"):
        _, st, p = walked("rgb", name, sampling)
        for comps in ((0,), (1, 2)):
            z = [n for n, c in zip(st.zrl, st.comp) if c in comps]
            assert max(z) >= 1, f"{name}: no ZRL in components {comps}"
    assert len(p.length) >= 2


@pytest.mark.parametrize("sampling", ["gray", "420", "444"])
def test_dc_checker_reaches_category_11_in_both_signs_at_a_parts_first_block(walked, sampling):
    seen = set()
    for name in ("dc_checker_128x256_q100", "dc_checker_shifted_128x256_q100"):
        _, st, p = walked("gray", name, sampling)
        luma = [(cat, d) for cat, d, c in zip(st.dc_cat, st.dc_diff, st.comp) if c == 0]
        assert len(luma) == 512 and len(p.length) == 2
        assert all(cat == 11 and abs(d) == 2040 for cat, d in luma[1:])
        assert {d for _, d in luma[1:]} == {2040, -2040}
        seen.add(luma[256][1])   # the first luma block of part 1 (4:2:0: MCU 64's first), from the recomputed DC
    assert seen == {2040, -2040}, "the part's first block takes +2040 in one variant and −2040 in the other"


def test_shifted_dc_checker_has_block_255_black_and_256_white():
    img = jc.dc_checker(128, 256, 1)
    assert img[56:64, 248:256].max() == 0 and img[64:72, 0:8].min() == 255


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_rgb_dc_checker_reaches_the_chroma_extremes(walked, sampling):
    _, st, _ = walked("rgb", "rgb_dc_checker_64x256_q100", sampling)
    for comp in (1, 2):
        d = [x for x, c in zip(st.dc_diff, st.comp) if c == comp]
        # saturated complements: Cb and Cr steps of ±(255 − 0)·8 less the conversion's rounding
        assert max(d) >= 2000 and min(d) <= -2000 and max(c for c, k in zip(st.dc_cat, st.comp) if k == comp) == 11


@pytest.mark.parametrize("sampling", ["gray", "420", "444"])
def test_binary_noise_reaches_ac_category_10_and_long_blocks(walked, sampling):
    _, st, _ = walked("gray", "binary_noise_48x80_q100", sampling)
    assert max(st.ac_cat) == 10
    assert max(st.bits) > 800   # > 160 bits of LDS: (800 − 160) / 32 = 20 spill words and more


@pytest.mark.parametrize("q", jc.FLAT_LEVEL_QUALITIES)
def test_flat_levels_dc_is_rounded_half_away_from_zero(walked, q):
    """Block i is flat at level i: its unquantised DC is 8·(i − 128), and libjpeg rounds the quotient
    half away from zero. At quality 50 the divisor is 16: every odd i − 128 is an exact half."""
    _, st, _ = walked("gray", f"flat_levels_128x128_q{q}", "gray")
    d = st.quant[0][0]
    x = 8 * (np.arange(256) - 128)
    want = np.sign(x) * ((2 * np.abs(x) + d) // (2 * d))
    assert np.array_equal(np.cumsum(st.dc_diff), want)
    halves = (2 * np.abs(x)) % (2 * d) == d
    print(f"q{q}: divisor {d}, exact halves {halves.sum()} ({(halves & (x < 0)).sum()} negative)")
    if q == 50:
        assert d == 16 and halves.sum() == 128 and (halves & (x < 0)).sum() == 64
    assert max(st.ac_cat) == 0


@pytest.mark.parametrize("al", range(1, 8))
def test_straddle_puts_ff_across_the_part_edge_at_every_alignment(walked, al):
    _, st, p = walked("gray", f"straddle_{al}", "gray")
    assert len(p.length) == 2
    assert p.al[1] == al and p.straddle_ff[1]
    assert not st.eob[255] and st.dc_cat[256] == 11 and st.dc_diff[256] == 1528
    # three parts: the same edge with a successor behind it, whose output position counts that byte
    _, st3, p3 = walked("gray", f"straddle3_{al}", "gray")
    assert len(p3.length) == 3
    assert p3.al[1] == al and p3.straddle_ff[1]
    assert p3.al[2] == (al + 1) % 8 and p3.straddle_ff[2] == (al != 7)


@pytest.mark.parametrize("rem", range(1, 8))
def test_final_pads_the_last_byte_to_ff_at_every_remainder(walked, rem):
    _, st, p = walked("gray", f"final_{rem}", "gray")
    assert p.final_rem == rem and p.final_ff
    assert not st.eob[-1]
    assert st.segment[-2:] == b"\xff\x00"


def test_edge_block_ends_in_the_stored_number_of_ones(walked):
    _, st, _ = walked("gray", "straddle_7", "gray")
    bits = np.unpackbits(np.frombuffer(st.unstuffed, np.uint8))
    end = st.pos[256]
    assert bits[end - jc.EDGE_ONES:end].all() and not bits[end - jc.EDGE_ONES - 1]
    assert jc.EDGE_ONES >= 8
    assert bits[end:end + 9].tolist() == [1] * 8 + [0]   # DC category 11: 111111110


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_rgb_straddle_and_final(walked, sampling):
    _, st, p = walked("rgb", "rgb_straddle_64x256_q100", sampling)
    assert len(p.length) >= 2 and p.al[1] == 2 and p.straddle_ff[1]
    first = p.mcus_per_part * st.blocks_per_mcu
    assert st.comp[first - 1] == 2 and not st.eob[first - 1], "the part ends in a Cr block without EOB"
    assert st.comp[first] == 0 and st.dc_cat[first] >= 10, "the next part starts on a large luma step"
    _, st, p = walked("rgb", "rgb_final_64x256_q100", sampling)
    assert p.final_rem == 2 and p.final_ff and st.comp[-1] == 2 and not st.eob[-1]


_MODEL_CASES = ([f"straddle_{k}" for k in range(1, 8)] + [f"final_{k}" for k in range(1, 8)] +
                [f"straddle3_{k}" for k in range(1, 8)] + ["sparse_hf_272x400_q50", "dc_checker_shifted_128x256_q100"])


def test_stuffing_model_gives_the_segment_and_each_dropped_step_is_noticed(walked):
    """jc.stuff_model, the host model of jpeg_emit_range's stuffing steps, reproduces the golden
    segment of the edge cases whether a part sees its predecessors as aggregates or through an
    inclusive record. With one step left out, named cases differ — what the GPU test's bytes pin:
      * the look-back's `++fq`: every straddle3 image, in the aggregate view only (no two-part image
        can notice: its last part has no successor);
      * `own += strad_v == 0xFFu`: every straddle image, in either view;
      * `own += fin_v == 0xFFu`: every final image, in either view."""
    def differs(view, drop):
        out = set()
        for name in _MODEL_CASES:
            _, st, p = walked("gray", name, "gray")
            if jc.stuff_model(st, p, view, drop) != st.segment:
                out.add(name)
        return out
    for view in ("aggregate", "inclusive"):
        assert differs(view, None) == set()
        assert {f"straddle_{k}" for k in range(1, 8)} <= differs(view, "strad")
        assert {f"final_{k}" for k in range(1, 8)} <= differs(view, "fin")
    assert differs("aggregate", "fq") == {f"straddle3_{k}" for k in range(1, 8)}
    assert differs("inclusive", "fq") == set()


def test_range_limit_has_a_case_on_either_side(walked):
    _, _, under = walked("gray", "limit128_uniform_noise", "gray")
    _, _, over = walked("gray", "limit128_binary_noise", "gray")
    assert len(under.length) == 1 and len(over.length) == 1, "exactly one full part at gray sampling"
    assert under.length[0] < jc.RANGE_LIMIT_BITS < over.length[0]
    assert np.array_equal(jc.limit_launch((128, 128))["uniform_noise"], jc.gray_cases()[(100, (128, 128))]["uniform_noise"])
    for sampling in ("gray", "420", "444"):
        for size in (128, 256):
            _, _, p = walked("gray", f"limit{size}_binary_noise", sampling)
            assert min(p.length) > jc.RANGE_LIMIT_BITS
            _, _, p = walked("gray", f"limit{size}_uniform_noise", sampling)
            assert max(p.length) < jc.RANGE_LIMIT_BITS
    _, _, p = walked("gray", "limit256_straddle_3", "gray")
    assert p.al[1] == 3 and p.straddle_ff[1]


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_rgb_range_limit_has_a_case_on_either_side(walked, sampling):
    """The stored colour image has its full part over the limit (`nlocal + 2 > kRgbUnionWords`), the
    palette noise one at 90–94 % of it, and no stream comes near the launch's output capacity."""
    _, st, p = walked("rgb", "limit_rgb_over_limit", sampling)
    assert len(p.length) == (1 if sampling == "420" else 2)
    assert p.length[0] > jc.RANGE_LIMIT_BITS and (p.length[0] + 31) // 32 + 2 > jc.K_UNION_WORDS
    assert max(p.length[1:], default=0) < jc.RANGE_LIMIT_BITS
    assert len(st.segment) < jc.RGB_LIMIT_OUT_CAP // 4
    _, st, p = walked("rgb", "limit_rgb_palette_noise", sampling)
    assert 0.9 * jc.RANGE_LIMIT_BITS < p.length[0] < jc.RANGE_LIMIT_BITS
    assert len(st.segment) < jc.RGB_LIMIT_OUT_CAP // 4
    _, _, p = walked("rgb", "limit_rgb_sparse_hf", sampling)
    assert max(p.length) < jc.RANGE_LIMIT_BITS // 4


def test_engine_fixture_fallback_count(native, tmp_path):
    """The engine test's expected fallbacks: the exported images of engine_slices (as the engine reads
    them back from their DICOM files) whose golden stream has a part over the range limit — the noise
    slice's original alone, each of its 16 parts."""
    cfg = nm.PipelineConfig(batch_size=4, streams=1, threads=2, jpeg_quality=100)
    over = []
    for name, a in jc.engine_slices(native).items():
        (tmp_path / f"{name}.dcm").write_bytes(native.dicom_bytes(a))
        raw, meta = native.read_slice(str(tmp_path / f"{name}.dcm"))
        g = native.golden_run(raw, meta["type"], meta["stored_bits"], meta["slope"], meta["intercept"],
                              cfg.pipeline_params(), cfg.render_params(), meta["spacing_x"], meta["spacing_y"])
        for kind in ("original", "processed"):
            st = jc.walk(g[f"jpeg_{kind}"])
            p = jc.parts(st, "gray")
            assert len(p.length) == 16 and len(st.segment) < jc.ENGINE_OUT_CAP
            print(f"{name} {kind}: {st.summary()} longest part {max(p.length)} bytes {len(st.segment)}")
            if max(p.length) > jc.RANGE_LIMIT_BITS:
                over.append((name, kind))
                assert min(p.length) > jc.RANGE_LIMIT_BITS
    assert over == [("binary_noise", "original")]
    assert len(over) == jc.ENGINE_FALLBACKS and 0 < jc.ENGINE_FALLBACKS < 6
