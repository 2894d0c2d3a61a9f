"""CPU checks that the inputs of the 3D GPU tests (volume_cases.py → test_gpu_volume.py) do what
those tests rely on: the maze is one component that the golden flood fill covers and that a
plane-sweep scheme cannot finish within twice the old sweep limit, the sweep emulator itself is
sound, every random band gives a region that is neither empty nor everything, every dilation input
leaves room to be wrong, and the serpentine survives the per-plane preprocessing in one piece."""
import numpy as np
import pytest

import volume_cases as vc
from conftest import run_bin

ndimage = pytest.importorskip("scipy.ndimage")


def _components(mask, conn):
    return ndimage.label(mask, structure=ndimage.generate_binary_structure(3, 3 if conn == 26 else 1))


@pytest.mark.parametrize("conn", [6, 26])
def test_maze_is_one_component_and_the_golden_fills_it(native, conn):
    band, seed, ncells = vc.maze(**vc.MAZE)
    assert ncells == 15360 and band.sum() == 2 * ncells - 1  # cells + the voxels between them
    assert _components(band, conn)[1] == 1
    assert np.array_equal(native.golden_region_grow3d(band, [seed], conn), band)


@pytest.mark.parametrize("order", ["asc", "desc"])
def test_maze_outlasts_twice_the_old_sweep_cap(order):
    """What keeps the maze a test of the sweep limit: with the planes of a sweep processed in
    ascending or descending order, 2 · 4·(w + h + d) sweeps leave it unconverged (the emulator stops
    there; run to the end it took 3842 sweeps either way)."""
    band, seed, _ = vc.maze(**vc.MAZE)
    cap = vc.old_sweep_cap(band)
    assert cap == 632
    region, sweeps, converged = vc.emulate_sweeps(band, seed, 6, order, stop_after=2 * cap)
    assert not converged and sweeps == 2 * cap
    assert 0 < region.sum() < band.sum() and not (region & ~band).any()


def test_small_maze_emulator_converges_to_the_band():
    """The emulator is sound on a maze small enough to run out: all three plane orders end at the
    band (122 / 37 / 32 sweeps for jacobi / asc / desc when this was written)."""
    band, seed, _ = vc.maze(**vc.MAZE_SMALL)
    assert band.shape == (22, 24, 16)
    counts = {}
    for order in ("jacobi", "asc", "desc"):
        region, counts[order], converged = vc.emulate_sweeps(band, seed, 6, order)
        assert converged and np.array_equal(region, band), order
    print("small maze sweeps", counts)
    assert counts["jacobi"] > counts["asc"] > 2 and counts["desc"] > 2


@pytest.mark.parametrize("conn", [6, 26])
def test_emulator_equals_golden_on_a_random_band(native, conn):
    rng = np.random.default_rng(3)
    band = (rng.random((9, 14, 21)) < (0.4 if conn == 6 else 0.18)).astype(np.uint8)
    seed = vc.case_seeds(band, 1)[0]
    ref = native.golden_region_grow3d(band, [seed], conn)
    assert 0 < ref.sum() < band.sum()
    for order in ("jacobi", "asc", "desc"):
        region, _, converged = vc.emulate_sweeps(band, seed, conn, order)
        assert converged and np.array_equal(region, ref), order


def test_staircase_turns_through_all_three_axes(native):
    band, seed, ncells = vc.staircase(**vc.STAIRCASE)
    assert band.shape == (21, 26, 70) and ncells >= 400 and band.sum() == 2 * ncells - 1
    assert _components(band, 6)[1] == 1
    for conn in (6, 26):
        assert np.array_equal(native.golden_region_grow3d(band, [seed], conn), band)
    # More sweeps than a blob needs, under every plane order.
    for order in ("jacobi", "asc", "desc"):
        region, sweeps, converged = vc.emulate_sweeps(band, seed, 6, order)
        assert converged and np.array_equal(region, band) and sweeps > 30, (order, sweeps)


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("case", vc.SHAPE_CASES, ids=vc.case_id)
def test_random_band_region_is_neither_empty_nor_everything(native, case, conn):
    band = vc.case_band(case, conn)
    seeds = vc.case_seeds(band, case.get("nseeds", 4))
    assert seeds and all(band[z, y, x] for x, y, z in seeds)
    region = native.golden_region_grow3d(band, seeds, conn)
    assert not (region & ~band).any()
    assert region.sum() < band.sum(), "every band voxel reached: a kernel that floods the band would pass"
    assert region.sum() >= 0.05 * band.sum(), "hardly anything reached"
    lab, _ = _components(band, conn)
    assert np.array_equal(region.astype(bool), np.isin(lab, [lab[z, y, x] for x, y, z in seeds]))


@pytest.mark.parametrize("case", vc.SHAPE_CASES, ids=vc.case_id)
def test_shape_case_dilations_are_neither_empty_nor_full(native, case):
    m = vc.sparse_mask(case["shape"])
    for size, ball in ((1, False), (3, False), (7, False), (5, True)):
        dil = native.golden_dilate3d(m.astype(np.uint8), size, ball)
        assert dil.sum() >= m.sum() > 0
        if not ball and size in case.get("saturates", ()):
            assert dil.all()
        else:
            assert not dil.all(), (size, ball)


def test_dilation_range_inputs(native):
    m = vc.dilation_range_mask().astype(np.uint8)
    R = vc.DILATION_RANGE
    prev = m
    for size in R["cube"]:
        dil = native.golden_dilate3d(m, size, False)
        assert np.array_equal(dil.astype(bool), vc.cube_dilation_ref(m, size)), size
        assert not dil.all() and not (prev & ~dil).any() and dil.sum() >= prev.sum(), size
        assert (size in R["saturates_z"]) == all(np.array_equal(dil[z], dil[0]) for z in range(dil.shape[0])), size
        prev = dil
    for size in R["ball"]:
        dil = native.golden_dilate3d(m, size, True)
        assert np.array_equal(dil.astype(bool), ndimage.binary_dilation(m.astype(bool), structure=vc.ball_ref(size)))
        assert m.sum() < dil.sum() < native.golden_dilate3d(m, size, False).sum(), size
    assert all(s < 1 or s > 63 or s % 2 == 0 for s in vc.DILATION_REJECTED)


@pytest.mark.parametrize("shape", vc.BORDER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_border_masks_have_an_interior_at_every_radius(native, shape):
    m = vc.border_mask(shape)
    for radius in vc.BORDER_RADII:
        b = native.golden_border(m[0].astype(np.uint8), radius)
        assert 0 < b.sum() < m[0].sum(), radius  # something eroded away, something left inside


@pytest.mark.parametrize("cross", ["top", "bottom"])
def test_serpentine_band_is_one_piece_and_seeded_in_its_first_leg(native, cross):
    S = dict(vc.SERPENTINE, cross=cross)
    vol = vc.serpentine_volume(**S)
    band = np.stack([native.golden_run(vol[z])["band"] for z in range(S["d"])])
    core = vc.serpentine_mask(**S)
    assert not (core & ~band.astype(bool)).any()
    lab, _ = _components(band, 6)
    ids = np.unique(lab[core])
    assert len(ids) == 1 and ids[0] > 0  # the band contains the slab as one 6-connected component
    seeds = [(x, y, S["d"] // 2) for x, y in native.reference_seeds(S["w"], S["h"])]
    hits = [s for s in seeds if band[s[2], s[1], s[0]]]
    assert hits and all(x < 60 for x, _, _ in hits)  # none in the leg that comes back down
    region = native.golden_region_grow3d(band, seeds, 6)
    assert np.array_equal(region.astype(bool), lab == ids[0])


def test_plane_buffers_cross_the_lds_budget_where_the_cases_say():
    """The shapes named for the LDS / global switch sit on it: 5088 plane words (162 816 B of
    dynamic LDS) are the last that fit beside the 1 KiB kept for static LDS, 5090 the first that do
    not. With w = 512 the transposed plane (512 × ceil(h/64) words) is the larger one, so h = 636
    and 637 are both beyond the switch (5120 words) and h = 576 is the last LDS shape."""
    g = {vc.case_id(c): (vc.srg_plane_words(c["shape"]), vc.srg_planes_global(c["shape"]))
         for c in vc.SHAPE_CASES if c.get("srg", True)}
    assert g["4x2544x65"] == (5088, False) and g["4x2545x65"] == (5090, True)
    assert g["4x576x512"] == (4608, False) and g["4x636x512"] == (5120, True) and g["4x637x512"] == (5120, True)
    assert g["520x8x8"][1] is False and g["600x8x520"][1] is True
    assert 5088 * 32 == 162816 and 5088 * 32 + 1024 == vc.LDS_BUDGET
    assert not vc.morph_planes_global((3, 848, 512)) and vc.morph_planes_global((3, 849, 512))
    assert not vc.morph_planes_global((5, 70, 100))


@pytest.mark.parametrize("args,word", [(("--dilation-size", "65"), "dilation"), (("--dilation-size", "129"), "dilation"),
                                       (("--dilation-size", "4"), "dilation"), (("--dilation-size", "0"), "dilation"),
                                       (("--srg-connectivity", "18"), "connectivity")])
def test_cli_3d_rejects_sizes_the_kernels_do_not_have(native, cohort_root, tmp_path, args, word):
    """--mode 3d fails with a message before any volume is processed (the golden backend takes the
    GPU kernels' limits, so --cpu stays the oracle of the same command line)."""
    r = run_bin("img_processing_parallel", "--mode", "3d", "--cpu", *args, "--data-root", cohort_root, "--out",
                str(tmp_path / "o"))
    assert r.returncode != 0 and word in r.stderr and "--mode 3d" in r.stderr
    assert not list((tmp_path / "o").rglob("*.jpg"))
