"""GPU tests (MI355X) of 3D mode on tortuous regions and edge shapes: K5's plane-sweep region growing,
the cube / ball dilation, the per-plane border and the z-slab decomposition against the C++ golden
model and scipy.ndimage, on the inputs of volume_cases.py (whose properties test_volume_cases.py
checks on the CPU)."""
import functools
import time

import numpy as np
import pytest
import torch

import nm03_capstone_project_amd as nm
from nm03_capstone_project_amd import ops
from nm03_capstone_project_amd.ops import reference as R

import volume_cases as vc
from conftest import run_bin

pytestmark = pytest.mark.gpu

try:
    from scipy import ndimage
except ImportError:  # the golden model is the reference that always runs
    ndimage = None


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert nm.native().device_count() >= 1


def _dev(mask):
    return torch.from_numpy(np.ascontiguousarray(mask).astype(bool)).cuda()


def _host(t):
    return t.cpu().numpy().astype(np.uint8)


def _label_ref(band, seeds, conn):
    """The seeds' components of the band by scipy's labelling (None without scipy)."""
    if ndimage is None:
        return None
    lab, _ = ndimage.label(band, structure=ndimage.generate_binary_structure(3, 3 if conn == 26 else 1))
    return np.isin(lab, [lab[z, y, x] for x, y, z in seeds if band[z, y, x]]).astype(np.uint8)


# References are computed once per input and shared (never written to).
@functools.lru_cache(maxsize=None)
def _maze():
    band, seed, _ = vc.maze(**vc.MAZE)
    band.setflags(write=False)
    return band, seed


@functools.lru_cache(maxsize=None)
def _case_ref(idx, conn):
    case = vc.SHAPE_CASES[idx]
    band = vc.case_band(case, conn)
    seeds = vc.case_seeds(band, case.get("nseeds", 4))
    ref = nm.native().golden_region_grow3d(band, seeds, conn)
    for a in (band, ref):
        a.setflags(write=False)
    return band, seeds, ref


_SRG_CASES = [i for i, c in enumerate(vc.SHAPE_CASES) if c.get("srg", True)]
_ALL_CASES = list(range(len(vc.SHAPE_CASES)))


def _cid(i):
    return vc.case_id(vc.SHAPE_CASES[i])


# ---------------------------------------------------------------------------------------------
# Tortuous regions: the sweep count is bounded by the voxel count only
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 26])
def test_maze_region_equals_golden(native, conn):
    """A path of 15 360 cells that turns between y and z at every cell (30 × 64 × 64): the region is
    the whole band, as the golden flood fill says. 6-connected it needs more sweeps than the former
    limit 4·(w + h + d) = 632, at which the kernel used to stop and report success. Measured on an
    MI355X: 14 338 sweeps for either connectivity (the workgroups of a sweep see their neighbour
    planes as the previous sweep left them, one segment per sweep), 0.17–0.21 s per call."""
    band, seed = _maze()
    ref = native.golden_region_grow3d(band, [seed], conn)
    assert np.array_equal(ref, band)
    bt = _dev(band)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reg, sweeps = ops.region_grow3d(bt, [seed], conn)
    torch.cuda.synchronize()
    print(f"maze conn {conn}: {sweeps} sweeps, {time.perf_counter() - t0:.3f} s (with bit packing)")
    got = _host(reg)
    assert np.array_equal(got, ref), f"{int(got.sum())} of {int(ref.sum())} voxels after {sweeps} sweeps"
    if conn == 6:
        assert sweeps > vc.old_sweep_cap(band)


@pytest.mark.parametrize("conn", [6, 26])
def test_maze_continued_from_the_seed_voxel(native, conn):
    """The same maze through `region=` (reset = false, no seeds): what a z-slab does after its
    neighbours added boundary voxels."""
    band, (x, y, z) = _maze()
    part = np.zeros_like(band)
    part[z, y, x] = 1
    reg, sweeps = ops.region_grow3d(_dev(band), [], conn, region=_dev(part))
    assert np.array_equal(_host(reg), band), sweeps


@pytest.mark.parametrize("conn", [6, 26])
def test_staircase_region_equals_golden(native, conn):
    """A path whose steps cycle through x, y and z (21 × 26 × 70, two words with a partial last one)."""
    band, seed, _ = vc.staircase(**vc.STAIRCASE)
    ref = native.golden_region_grow3d(band, [seed], conn)
    assert np.array_equal(ref, band)
    reg, sweeps = ops.region_grow3d(_dev(band), [seed], conn)
    print(f"staircase conn {conn}: {sweeps} sweeps")
    assert np.array_equal(_host(reg), ref), sweeps
    assert sweeps > 10  # a blob of this size is done in a handful


# ---------------------------------------------------------------------------------------------
# Shapes: single planes, word edges, d the long side, the LDS / global switch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("idx", _SRG_CASES, ids=_cid)
def test_region_grow3d_shapes_vs_golden(native, idx, conn):
    band, seeds, ref = _case_ref(idx, conn)
    assert 0 < ref.sum() < band.sum()
    lab = _label_ref(band, seeds, conn)
    assert lab is None or np.array_equal(lab, ref)
    reg, sweeps = ops.region_grow3d(_dev(band), seeds, conn)
    assert sweeps >= 2 and np.array_equal(_host(reg), ref)
    # continuing from the seed voxels alone reaches the same fixpoint
    part = np.zeros_like(band)
    for x, y, z in seeds:
        part[z, y, x] = 1
    reg2, _ = ops.region_grow3d(_dev(band), [], conn, region=_dev(part))
    assert np.array_equal(_host(reg2), ref)


def _check_dilations(native, mask, sizes, saturates=()):
    """ops.dilate3d of `mask` (bool [d, h, w]) for (size, ball) in `sizes` against the golden model
    and scipy."""
    mt = _dev(mask)
    m8 = np.ascontiguousarray(mask).astype(np.uint8)
    for size, ball in sizes:
        ref = native.golden_dilate3d(m8, size, ball)
        if ndimage is not None:
            sp = (ndimage.binary_dilation(mask.astype(bool), structure=vc.ball_ref(size)) if ball
                  else vc.cube_dilation_ref(mask, size))
            assert np.array_equal(sp.astype(np.uint8), ref), (size, ball)
        assert ref.all() == (not ball and size in saturates), (size, ball)
        got = _host(ops.dilate3d(mt, size, ball=ball))
        assert np.array_equal(got, ref), (size, ball, int(got.sum()), int(ref.sum()))


@pytest.mark.parametrize("idx", _ALL_CASES, ids=_cid)
def test_dilate3d_shapes_vs_golden(native, idx):
    """Cube sizes 1, 3, 7 and the ball of size 5 on a sparse mask (isolated voxels, the corners and
    both sides of every word boundary: each cube's reach shows) and, cube 3, on the case's region."""
    case = vc.SHAPE_CASES[idx]
    sizes = ((1, False), (3, False), (7, False), (5, True))
    _check_dilations(native, vc.sparse_mask(case["shape"]), sizes, case.get("saturates", ()))
    _, _, region = _case_ref(idx, 26)
    ref = native.golden_dilate3d(region, 3, False)
    assert np.array_equal(_host(ops.dilate3d(_dev(region), 3)), ref)


def test_dilate3d_size_range_vs_golden(native):
    """Cube sizes up to the limit 63 (radius 31: every shift below one word) and balls above 7."""
    r = vc.DILATION_RANGE
    sizes = [(s, False) for s in r["cube"]] + [(s, True) for s in r["ball"]]
    _check_dilations(native, vc.dilation_range_mask(), sizes)


# ---------------------------------------------------------------------------------------------
# Parameters the kernels do not have are rejected, not mapped or shifted out of range
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", vc.DILATION_REJECTED)
def test_dilation_sizes_outside_1_to_63_or_even_raise(native, size):
    m = _dev(vc.dilation_range_mask())
    for ball in (False, True):
        with pytest.raises(ValueError):
            ops.dilate3d(m, size, ball=ball)
    src = ops.pack_bits(m).contiguous()
    dst, tmp = torch.empty_like(src), torch.empty_like(src)
    d, h, w = m.shape
    with pytest.raises(ValueError):  # the binding itself, under the wrapper's check
        native.k_dilate3d(src.data_ptr(), dst.data_ptr(), tmp.data_ptr(), w, h, d, size,
                          torch.cuda.current_stream().cuda_stream, False)
    vol = np.stack([native.phantom_slice(40, 64, 2, z, 4, 5) for z in range(4)])
    with pytest.raises(ValueError):
        nm.VolumePipeline(connectivity=6, dilation=size).run(vol)
    runner = native.VolumeRunner(0)
    with pytest.raises(ValueError):
        runner.run(vol, native.PipelineParams(), 6, size, [])
    good = runner.run(vol, native.PipelineParams(), 6, 3, [])  # the runner is still usable
    assert np.array_equal(good["dilated"], native.golden_dilate3d(good["region"], 3))


@pytest.mark.parametrize("conn", [0, 4, 8, 18, 27])
def test_connectivity_other_than_6_or_26_raises(native, conn):
    band = _dev(vc.dilation_range_mask())
    with pytest.raises(ValueError):
        ops.region_grow3d(band, [(0, 0, 0)], conn)
    vol = np.stack([native.phantom_slice(40, 64, 2, z, 4, 5) for z in range(4)])
    with pytest.raises(ValueError):
        nm.VolumePipeline(connectivity=conn, dilation=3).run(vol)
    with pytest.raises(ValueError):
        native.VolumeRunner(0).run(vol, native.PipelineParams(), conn, 3, [])


@pytest.mark.parametrize("args,word", [(("--dilation-size", "65"), "dilation"), (("--dilation-size", "6"), "dilation"),
                                       (("--srg-connectivity", "18"), "connectivity")])
def test_cli_3d_rejects_bad_parameters(native, cohort_root, tmp_path, args, word):
    r = run_bin("img_processing_parallel", "--mode", "3d", *args, "--data-root", cohort_root, "--out",
                str(tmp_path / "o"))
    assert r.returncode != 0 and word in r.stderr and "--mode 3d" in r.stderr
    assert not list((tmp_path / "o").rglob("*.jpg"))


# ---------------------------------------------------------------------------------------------
# Per-plane border (the 3D export's outline), LDS and global-scratch planes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", vc.BORDER_RADII)
@pytest.mark.parametrize("shape", vc.BORDER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_border3d_vs_golden_and_torch(native, shape, radius):
    mask = vc.border_mask(shape)
    mt = _dev(mask)
    got = ops.border3d(mt, radius)
    for z in range(shape[0]):
        ref = native.golden_border(mask[z].astype(np.uint8), radius)
        assert 0 < ref.sum() < mask[z].sum()
        assert np.array_equal(_host(got[z]), ref), z
        assert torch.equal(got[z], R.border(mt[z], radius)), z
    with pytest.raises(ValueError):
        ops.border3d(mt, 32)


# ---------------------------------------------------------------------------------------------
# z-slabs on the GPU: a band that climbs through all of z, crosses over and comes back down
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _serpentine_ref(conn, dilation, cross):
    n = nm.native()
    vol = vc.serpentine_volume(**vc.SERPENTINE, cross=cross)
    ref = n.VolumeRunner(0).run(vol, n.PipelineParams(), conn, dilation, [])
    d, h, w = vol.shape
    seeds = [(x, y, d // 2) for x, y in n.reference_seeds(w, h)]
    region = n.golden_region_grow3d(ref["band"], seeds, conn)
    return vol, ref, region, n.golden_dilate3d(region, dilation)


@pytest.mark.parametrize("ranks,conn,dilation,cross", [(3, 26, 7, "top"), (2, 6, 7, "bottom"), (4, 6, 25, "top")],
                         ids=["3ranks-conn26", "2ranks-conn6", "4ranks-thin"])
def test_volume_slabs_serpentine_equals_volume_and_golden(native, ranks, conn, dilation, cross):
    """Rank threads on one GPU over loopback comms, 46 × 70 × 100 (two words, a partial last one: the
    slab seed kernel masks it for conn 26), uneven slabs for 3 ranks. The region reaches the second
    leg only through the crossing planes, which lie in another slab than the seeds, so the slabs
    exchange boundary planes for ≥ 3 rounds (volume_cases.serpentine_volume). Dilation 25 (radius
    12) over 4 slabs of 11–12 planes takes the generic path, halos from several ranks."""
    vol, ref, region, dilated = _serpentine_ref(conn, dilation, cross)
    core = vc.serpentine_mask(**vc.SERPENTINE, cross=cross)
    assert not (core & ~ref["band"].astype(bool)).any() and not (core & ~region.astype(bool)).any()
    assert np.array_equal(ref["region"], region) and np.array_equal(ref["dilated"], dilated)
    r = native.run_volume_slabs_threads(vol, ranks, native.PipelineParams(), conn, dilation, 0, 1)
    assert np.array_equal(r["region"], region)
    assert np.array_equal(r["dilated"], dilated)
    thin = vol.shape[0] // ranks < dilation // 2
    assert thin == (dilation == 25)
    print("rounds", r["rounds"])
    assert thin or max(r["rounds"]) >= 3, r["rounds"]


# ---------------------------------------------------------------------------------------------
# Pipeline: raw planes with a partial last word, ball structuring element above 7
# ---------------------------------------------------------------------------------------------
def test_volume_pipeline_ball9_partial_word_vs_golden(native):
    d, h, w = 5, 70, 100
    vol = np.stack([native.phantom_slice(h, w, 2, z, d, 5) for z in range(d)])
    vp = nm.VolumePipeline(nm.PipelineConfig(se_shape=1), connectivity=26, dilation=9)
    seeds = vp.default_seeds(vol)
    res = vp.run(vol, seeds)
    for z in range(d):
        assert np.array_equal(res["band"][z], native.golden_run(vol[z])["band"]), z
    region, dil = vp.golden(res["band"], seeds)
    assert 0 < region.sum() < res["band"].sum() and not dil.all()
    assert np.array_equal(res["region"], region)
    assert np.array_equal(res["dilated"], dil)
    if ndimage is not None:
        assert np.array_equal(dil.astype(bool), ndimage.binary_dilation(region.astype(bool), structure=vc.ball_ref(9)))
