"""CPU-side conditions of the non-default-parameter GPU tests (test_gpu_params.py), on the golden model
alone: the derived sharpen bound holds for the float32 golden model against the float64 reference, and
every morphology plane the GPU tests compare is neither empty nor full."""
import numpy as np
import pytest
import torch

import nm03_capstone_project_amd as nm
import param_cases as pcs
from nm03_capstone_project_amd.ops import reference as R


@pytest.mark.parametrize("variant", ["default", "other"])
@pytest.mark.parametrize("mask", pcs.SHARPEN_MASKS)
def test_golden_sharpen_within_derived_bound(native, mask, variant):
    gain, sigma, _, _ = pcs.sharpen_variant(mask, variant)
    p = nm.PipelineConfig().pipeline_params()
    for h, w in pcs.SHARPEN_SHAPES[:2]:
        for raw in (native.phantom_slice(h, w, 3, 12, 25, 7), pcs.noise12(h, w, h + w)):
            c = native.golden_norm_clip(native.golden_median_u16(raw, 7), "u16", 16, 1.0, 0.0, p)
            gs = native.golden_sharpen(c, gain, sigma, mask, False)
            ref = R.sharpen(torch.from_numpy(c), gain, sigma, mask).numpy()
            assert np.abs(gs - ref).max() <= pcs.sharpen_bound(mask, gain, np.abs(c).max())


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", pcs.MORPH_SHAPES + (pcs.MORPH_LARGE,), ids=lambda s: f"{s[0]}x{s[1]}")
def test_structured_band_planes_are_non_trivial(native, shape, conn):
    h, w = shape
    band = pcs.structured_band(h, w)
    g = native.golden_region_grow(band.astype(np.uint8), [(w - 6, 3, 0)], conn)
    planes = {"region": g}
    for d, e in (pcs.MORPH_SIZES if shape != pcs.MORPH_LARGE else ((5, 7),)):
        planes[f"dilated {d}"] = native.golden_morph(g, d, True, False)
        planes[f"eroded {e}"] = native.golden_morph(g, e, False, False)
    for r in pcs.BORDER_RADII:
        planes[f"border {r}"] = native.golden_border(g, r)
    for name, m in planes.items():
        assert 0 < int(m.astype(bool).sum()) < m.size, name
    # the diagonal chain: its first pixel hangs on the block, the other three only diagonally
    assert int(g.sum()) == int(band.sum()) - (3 if conn == 4 else 0)


# ---- configurations the GPU path does not support are rejected before anything is launched ----------
_BAD_SHARPEN = [0, 4, 17, 99]
_BAD_MORPH = [dict(dilation_size=0), dict(dilation_size=65), dict(erosion_size=64), dict(erosion_size=-3),
              dict(border_radius=32), dict(border_radius=-1)]


def test_op_wrappers_reject_unsupported_parameters():
    from nm03_capstone_project_amd import ops
    keys = torch.zeros((8, 8), dtype=torch.int16)  # a CPU tensor: the parameters are checked first
    for mask in _BAD_SHARPEN:
        with pytest.raises(ValueError, match="sharpen mask"):
            ops.sharpen_band(keys, nm.PipelineConfig(sharpen_mask=mask))
    for kw in _BAD_MORPH:
        with pytest.raises(ValueError, match="morphology sizes|border radius"):
            ops.region_grow(torch.zeros((8, 8), dtype=torch.bool), [], nm.PipelineConfig(**kw))
    for k in (1, 4, 11):
        with pytest.raises(ValueError, match="median window"):
            ops.median2d(keys, k)


@pytest.mark.parametrize("kw,message", [(dict(sharpen_mask=4), "sharpen mask"), (dict(sharpen_mask=17), "sharpen mask"),
                                        (dict(median_window=4), "median window"), (dict(dilation_size=64), "morphology sizes"),
                                        (dict(erosion_size=0), "morphology sizes"), (dict(border_radius=32), "border radius"),
                                        (dict(out_width=520), "multiple of 16")])
def test_engine_rejects_unsupported_configuration(native, kw, message):
    """The constructor refuses before it touches a device (host_only: no GPU needed here)."""
    with pytest.raises(Exception, match=message):
        native.Engine(nm.PipelineConfig(host_only=True, threads=1, streams=1, batch_size=1, **kw).engine_config())
