"""The surface mesh (nm03/volume_mesh.h, --volume-mesh, K15) without a GPU, everything compared with ==:
  golden == NumPy reference == the kernels' per-word functions on the host, every case, both placements, several
  scan blocks; the invariants in integer arithmetic; quad counts == the faces of golden_measure_volume; nets within
  half a voxel of the corner and on the same quads; sidecar text; PLY and STL bytes re-read; anisotropic spacing;
  the --cpu CLI trees at one and two ranks; every refusal, the size cap included."""
import json
import os
import struct

import numpy as np
import pytest

import volume_mesh_cases as mc
from conftest import run_bin

CASES = mc.all_cases()
SMALL = tuple(c for c in CASES if c["name"] != "many_blocks")


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def goldens(native):
    """The golden mesh of every case and placement, computed once and shared."""
    return {(c["name"], pl): native.golden_volume_mesh(c["mask"], list(c["spacing"]), pl) for c in CASES for pl in mc.PLACEMENTS}


@pytest.mark.parametrize("c", CASES, ids=mc.ids(CASES))
def test_golden_equals_reference_equals_words(native, goldens, c):
    from nm03_capstone_project_amd.ops import reference
    default, smallest, largest = native.volume_mesh_scan_blocks()
    blocks = (0, smallest, 100, largest) if c["name"] != "many_blocks" else (0, smallest, 100)
    for pl in mc.PLACEMENTS:
        g = goldens[(c["name"], pl)]
        mc.assert_mesh_equal(dict(reference.volume_mesh(c["mask"], c["spacing"], pl), k15_s=0.0), g)
        for sb in blocks:
            mc.assert_mesh_equal(native.volume_mesh_words(c["mask"], list(c["spacing"]), pl, sb), g)


def test_many_blocks_case_outnumbers_the_totals_workgroup(native):
    _, smallest, _ = native.volume_mesh_scan_blocks()
    words = mc.lattice_words(mc.case("many_blocks")["mask"].shape)
    assert (words + smallest - 1) // smallest > mc.TOTALS_WORKGROUP
    # the word-edge cases: lattice rows of 64, 65, 66, 128 and 129 bits
    assert [mc.case(f"noise_w{w}")["mask"].shape[2] + 1 for w in (63, 64, 65, 127, 128)] == [64, 65, 66, 128, 129]


@pytest.mark.parametrize("c", CASES, ids=mc.ids(CASES))
def test_invariants(native, goldens, c):
    g = goldens[(c["name"], "corner")]
    mc.check_invariants(g, c["mask"], mc.doubled_corners(g, c["spacing"]))


def test_known_meshes(goldens):
    g = goldens[("single_voxel", "corner")]
    assert g["vertices"].tolist() == [[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)]
    assert g["quads"].tolist() == [[0, 4, 6, 2], [1, 3, 7, 5], [0, 1, 5, 4], [2, 6, 7, 3], [0, 2, 3, 1], [4, 5, 7, 6]]
    g = goldens[("full", "corner")]  # every open face lies on the frame
    assert (g["quads_x"], g["quads_y"], g["quads_z"], g["voxels"]) == (2 * 4 * 3, 2 * 5 * 3, 2 * 5 * 4, 60)
    assert len(g["vertices"]) == 6 * 5 * 4 - 4 * 3 * 2  # the lattice without its interior
    g = goldens[("empty", "corner")]
    assert g["vertices"].shape == (0, 3) and g["quads"].shape == (0, 4) and g["voxels"] == 0
    g = goldens[("checkerboard", "corner")]
    # every corner is mixed but the four frame corners whose one voxel is clear ((3, y, 0) and (0, y, 5), y = 0 and 4)
    assert len(g["vertices"]) == 5 * 6 * 7 - 4
    # every inner face is open (neighbours differ), and half of the voxels on each frame face are set
    assert (g["quads_x"], g["quads_y"], g["quads_z"]) == (3 * 5 * 6 + 30, 4 * 4 * 6 + 24, 4 * 5 * 5 + 20)
    # non-manifold: the shared edge has four quads, the shared corner two cubes' worth of edges
    g = goldens[("edge_touch", "corner")]
    q = g["quads"].astype(np.int64)
    e = np.sort(np.concatenate([q[:, [0, 1]], q[:, [1, 2]], q[:, [2, 3]], q[:, [3, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert sorted(set(counts.tolist())) == [2, 4] and (counts == 4).sum() == 1
    assert len(goldens[("corner_touch", "corner")]["vertices"]) == 15 and len(g["vertices"]) == 14
    # the hollow box has two shells: Euler characteristic V - E + F = 2 + 2
    g = goldens[("hollow_box", "corner")]
    q = g["quads"].astype(np.int64)
    e = np.unique(np.sort(np.concatenate([q[:, [0, 1]], q[:, [1, 2]], q[:, [2, 3]], q[:, [3, 0]]]), axis=1), axis=0)
    assert len(g["vertices"]) - len(e) + len(q) == 4


@pytest.mark.parametrize("c", SMALL, ids=mc.ids(SMALL))
def test_quad_counts_equal_measure_faces(native, goldens, c):
    g = goldens[(c["name"], "corner")]
    m = native.golden_measure_volume(c["mask"], c["mask"], np.zeros(c["mask"].shape, np.uint16))
    assert (g["quads_x"], g["quads_y"], g["quads_z"]) == (m["faces_x"], m["faces_y"], m["faces_z"])
    assert g["voxels"] == m["volume_vox"]


@pytest.mark.parametrize("c", CASES, ids=mc.ids(CASES))
def test_nets_stay_within_half_a_voxel_on_the_same_quads(goldens, c):
    a, b = goldens[(c["name"], "corner")], goldens[(c["name"], "nets")]
    assert a["quads"].tobytes() == b["quads"].tobytes() and a["vertices"].shape == b["vertices"].shape
    sp = np.asarray(c["spacing"], dtype=np.float64)
    off = (b["vertices"].astype(np.float64) - a["vertices"].astype(np.float64)) / sp[None, :]
    assert np.abs(off).max(initial=0.0) <= 0.5 + 1e-5
    if c["name"] in ("ball", "k14_shape"):
        assert np.abs(off).max() > 0.1  # and they do move


def test_nets_of_a_single_voxel_shrink_to_the_edge_midpoints_mean(goldens):
    # each corner of a lone voxel has three crossing edges (n = 3); two of them lie half a voxel inwards on any one
    # axis (S = 2 towards the voxel): N / (2n) = (-3 + 2) / 6 at the low corners and (3 - 2) / 6 at the high ones
    v = goldens[("single_voxel", "nets")]["vertices"]
    sixth = np.float32(1) / np.float32(6)
    want = np.asarray([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float32) * sixth
    assert v.tobytes() == want.astype(np.float32).tobytes()


def test_anisotropic_spacing_scales_each_axis(native):
    c = mc.case("ball")
    one = native.golden_volume_mesh(c["mask"], [1.0, 1.0, 1.0], "nets")
    for sp in ((0.9, 1.2, 2.5), (0.48828125, 0.48828125, 6.5), (3.0, 0.1, 0.7)):
        g = native.golden_volume_mesh(c["mask"], list(sp), "nets")
        f = np.asarray([np.float32(sp[0]), np.float32(sp[1]), np.float32(np.float64(sp[2]))], np.float32)
        assert g["vertices"].tobytes() == (one["vertices"] * f[None, :]).astype(np.float32).tobytes()
        assert g["quads"].tobytes() == one["quads"].tobytes()


# ---------------------------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------------------------
def test_sidecar_text(native, goldens):
    g = goldens[("single_voxel", "corner")]
    assert native.volume_mesh_to_json(g, "ply", 489, [1.0, 1.0, 1.0]) == (
        '{"placement":"corner","format":"ply","file":"mesh.ply","bytes":489,"vertices":8,"quads_x":2,"quads_y":2,"quads_z":2,'
        '"triangles":12,"voxels":1,"spacing":[1,1,1],"bbox_mm":[-0.5,-0.5,-0.5,0.5,0.5,0.5],"surface_mm2":6,"volume_mm3":1}')
    g = goldens[("empty", "nets")]
    assert native.volume_mesh_to_json(g, "stl", 84, [0.5, 0.25, 2.0]) == (
        '{"placement":"nets","format":"stl","file":"mesh.stl","bytes":84,"vertices":0,"quads_x":0,"quads_y":0,"quads_z":0,'
        '"triangles":0,"voxels":0,"spacing":[0.5,0.25,2],"bbox_mm":null,"surface_mm2":0,"volume_mm3":0}')
    c = mc.case("ball")
    g = goldens[("ball", "corner")]
    rec = json.loads(native.volume_mesh_to_json(g, "ply", 1, list(c["spacing"])))
    assert list(rec) == ["placement", "format", "file", "bytes", "vertices", "quads_x", "quads_y", "quads_z", "triangles", "voxels",
                         "spacing", "bbox_mm", "surface_mm2", "volume_mm3"]
    sx, sy, sz = float(np.float32(0.9)), float(np.float32(1.2)), 2.5
    assert rec["surface_mm2"] == float("%.9g" % (g["quads_x"] * sy * sz + g["quads_y"] * sx * sz + g["quads_z"] * sx * sy))
    assert rec["volume_mm3"] == float("%.9g" % (g["voxels"] * sx * sy * sz))
    v = g["vertices"]
    assert rec["bbox_mm"] == [float("%.9g" % float(x)) for x in list(v.min(axis=0)) + list(v.max(axis=0))]
    assert rec["triangles"] == 2 * len(g["quads"]) and rec["vertices"] == len(v)


@pytest.mark.parametrize("name", ["single_voxel", "empty", "ball", "noise_w65", "corner_touch"])
def test_ply_and_stl_bytes_reread(native, goldens, tmp_path, name):
    from nm03_capstone_project_amd.utils import read_volume_mesh
    for pl in mc.PLACEMENTS:
        g = goldens[(name, pl)]
        ply = native.volume_mesh_file(g, "ply")
        p = tmp_path / f"{pl}.ply"
        p.write_bytes(ply)
        rec = read_volume_mesh(str(p))
        assert rec["vertices"].tobytes() == g["vertices"].tobytes() and rec["quads"].tobytes() == g["quads"].tobytes()
        assert rec["comments"] == ["nm03 volume mesh", f"placement {pl}", "units mm"]
        q = g["quads"]
        assert rec["triangles"].tolist() == np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3).tolist()
        assert ply.startswith(b"ply\nformat binary_little_endian 1.0\n")
        stl = native.volume_mesh_file(g, "stl")
        ntri = struct.unpack_from("<I", stl, 80)[0]
        assert ntri == 2 * len(q) and len(stl) == 84 + 50 * ntri and not stl.startswith(b"solid")
        recs = np.frombuffer(stl, dtype=np.dtype([("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("a", "<u2")]), offset=84)
        assert recs["v"].tobytes() == g["vertices"][rec["triangles"].reshape(-1)].reshape(-1, 3, 3).tobytes()
        assert (recs["a"] == 0).all()
        # the normal: the f32 normalised cross product; unit length, pointing out of the set voxels
        v = recs["v"]
        e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(np.float32)
        ln = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]).astype(np.float32) + cr[:, 2] * cr[:, 2]).astype(np.float32)
        ok = ln > 0
        want = np.zeros_like(cr)
        want[ok] = (cr[ok] / ln[ok, None]).astype(np.float32)
        assert recs["n"].tobytes() == want.tobytes()
        if pl == "corner":
            assert ok.all()


def test_stl_degenerate_triangle_gets_a_zero_normal(native):
    m = dict(width=1, height=1, depth=1, placement="corner", vertices=np.zeros((4, 3), np.float32),
             quads=np.asarray([[0, 1, 2, 3]], np.int32), quads_x=1, quads_y=0, quads_z=0, voxels=0)
    stl = native.volume_mesh_file(m, "stl")
    assert struct.unpack_from("<I", stl, 80)[0] == 2
    assert stl[84:84 + 12] == b"\0" * 12 and stl[134:134 + 12] == b"\0" * 12
    with pytest.raises(ValueError):
        native.volume_mesh_file(dict(m, quads=np.asarray([[0, 1, 2, 4]], np.int32)), "ply")  # not a vertex
    with pytest.raises(ValueError):
        native.volume_mesh_file(m, "obj")


def test_size_error_names_v_q_and_the_cap(native):
    assert native.volume_mesh_size_error(8, 6, 12 * 8 + 16 * 6) == ""
    e = native.volume_mesh_size_error(8, 6, 12 * 8 + 16 * 6 - 1)
    assert "8 vertices" in e and "6 quads" in e and "191 bytes" in e and "192 bytes" in e
    e = native.volume_mesh_size_error(2 ** 31, 1, 2 ** 62)
    assert "2147483648 vertices" in e and "2^31" in e
    assert "1073741824 quads" in native.volume_mesh_size_error(1, 2 ** 30, 2 ** 62)
    assert native.volume_mesh_size_error(2 ** 31 - 1, 2 ** 30 - 1, 2 ** 62) == ""


def test_python_refusals(native):
    import nm03_capstone_project_amd as nm
    from nm03_capstone_project_amd.ops import reference
    mask = np.zeros((2, 2, 2), np.uint8)
    with pytest.raises(ValueError):
        native.golden_volume_mesh(mask, [1, 1, 1], "middle")
    with pytest.raises(ValueError):
        native.golden_volume_mesh(mask, [1, 1], "corner")
    with pytest.raises(ValueError):
        native.golden_volume_mesh(mask[0], [1, 1, 1], "corner")
    _, smallest, largest = native.volume_mesh_scan_blocks()
    for sb in (1, smallest - 1, largest + 1):
        with pytest.raises(ValueError):
            native.volume_mesh_words(mask, [1, 1, 1], "corner", sb)
    with pytest.raises(ValueError):
        reference.volume_mesh(mask, placement="middle")
    p = nm.VolumePipeline(mesh=True, mesh_placement="nets", mesh_format="stl", mesh_max_mb=3)
    assert p.mesh and (p.mesh_placement, p.mesh_format, p.mesh_max_mb) == ("nets", "stl", 3)
    assert not nm.VolumePipeline().mesh
    for kw in (dict(mesh_placement="middle"), dict(mesh_format="obj"), dict(mesh_max_mb=-1)):
        with pytest.raises(ValueError):
            nm.VolumePipeline(mesh=True, **kw)
    with pytest.raises(ValueError, match="host_only"):
        nm.VolumePipeline(nm.PipelineConfig(host_only=True), mesh=True)


# ---------------------------------------------------------------------------------------------
# CLI on the golden model
# ---------------------------------------------------------------------------------------------
MESH_FILES = ("mesh.ply", "mesh.stl", "mesh.json")


def _cli(cohort_root, out, *args, ok=True):
    r = run_bin("img_processing_parallel", "--mode", "3d", "--cpu", "--quiet", *args, "--data-root", cohort_root, "--out",
                str(out), "--json", str(out) + ".json")
    if ok:
        assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def cpu_runs(cohort_root, tmp_path_factory):
    base = tmp_path_factory.mktemp("vmcpu")
    _cli(cohort_root, base / "mesh", "--volume-mesh", "--measure-volume")
    _cli(cohort_root, base / "plain", "--measure-volume")
    return base / "mesh", base / "plain"


def test_cli_writes_the_mesh(native, cohort_root, cpu_runs):
    from nm03_capstone_project_amd.utils import read_volume_mesh
    mesh, plain = cpu_runs
    tm, tp = tree(mesh), tree(plain)
    patients = sorted({p.split(os.sep)[0] for p in tp if os.sep in p})
    assert len(patients) == 4
    # without the flag the tree has no extra file; with it, everything else is unchanged
    assert not [p for p in tp if os.path.basename(p) in MESH_FILES]
    assert {p: b for p, b in tm.items() if os.path.basename(p) not in MESH_FILES} == tp
    assert len(tm) == len(tp) + 2 * len(patients)
    nv = nq = 0
    for pid in patients:
        text = tm[os.path.join(pid, "mesh.json")].decode()
        rec = json.loads(text)
        ply = tm[os.path.join(pid, "mesh.ply")]
        assert (rec["placement"], rec["format"], rec["file"], rec["bytes"]) == ("corner", "ply", "mesh.ply", len(ply))
        m = read_volume_mesh(os.path.join(str(mesh), pid))
        assert rec["vertices"] == len(m["vertices"]) > 0 and rec["triangles"] == len(m["triangles"]) == 2 * len(m["quads"])
        vm = json.loads(tm[os.path.join(pid, "volume_measure.json")])
        assert (rec["quads_x"], rec["quads_y"], rec["quads_z"]) == (vm["faces_x"], vm["faces_y"], vm["faces_z"])
        assert rec["voxels"] == vm["volume_vox"] and rec["surface_mm2"] == vm["surface_mm2"] and rec["volume_mm3"] == vm["volume_mm3"]
        assert rec["spacing"] == [vm["spacing_x"], vm["spacing_y"], vm["spacing_z"]]
        # the file is the one writer's: the same arrays give the same bytes and the same sidecar
        md = dict(width=vm["width"], height=vm["height"], depth=vm["depth"], placement="corner", vertices=m["vertices"],
                  quads=m["quads"], quads_x=rec["quads_x"], quads_y=rec["quads_y"], quads_z=rec["quads_z"], voxels=rec["voxels"])
        assert native.volume_mesh_file(md, "ply") == ply
        assert native.volume_mesh_to_json(md, "ply", len(ply), rec["spacing"]) == text
        # closed and of the right volume, in integers
        mask = np.zeros((vm["depth"], vm["height"], vm["width"]), np.uint8)
        got = dict(md, vertices=m["vertices"])
        q = m["quads"].astype(np.int64)
        c2 = mc.doubled_corners(got, rec["spacing"])
        tri = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
        p = c2[tri]
        assert int(np.einsum("ti,ti->t", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum()) == 48 * rec["voxels"]
        assert mask.size >= rec["voxels"]
        nv += rec["vertices"]
        nq += len(m["quads"])
    run = json.load(open(str(mesh) + ".json"))
    assert run["volume_mesh"] == {"patients": 4, "vertices": nv, "quads": nq, "placement": "corner", "format": "ply"}
    assert "volume_mesh" not in json.load(open(str(plain) + ".json"))


def test_cli_two_ranks_and_other_flags(native, cohort_root, cpu_runs, tmp_path):
    from nm03_capstone_project_amd.utils import read_volume_mesh
    mesh, _ = cpu_runs
    _cli(cohort_root, tmp_path / "two", "--volume-mesh", "--measure-volume", "--gpus", "2")
    assert tree(tmp_path / "two") == tree(mesh)
    _cli(cohort_root, tmp_path / "nets", "--volume-mesh", "--volume-mesh-placement", "nets", "--volume-mesh-format", "stl",
         "--volume-mesh-max-mb", "64", "--volume-views", "--se-shape", "disc")
    t = tree(tmp_path / "nets")
    pid = sorted({p.split(os.sep)[0] for p in t if os.sep in p})[0]
    rec = json.loads(t[os.path.join(pid, "mesh.json")])
    stl = t[os.path.join(pid, "mesh.stl")]
    assert (rec["placement"], rec["format"], rec["file"], rec["bytes"]) == ("nets", "stl", "mesh.stl", len(stl))
    assert os.path.join(pid, "mesh.ply") not in t and os.path.join(pid, "views.json") in t
    assert struct.unpack_from("<I", stl, 80)[0] == rec["triangles"] and len(stl) == 84 + 50 * rec["triangles"]
    run = json.load(open(str(tmp_path / "nets") + ".json"))
    assert run["volume_mesh"]["placement"] == "nets" and run["volume_mesh"]["format"] == "stl"
    # nets and corner share their faces: the same counts as the corner run of the cube dilation differ only by the shape flag
    _cli(cohort_root, tmp_path / "netsply", "--volume-mesh", "--volume-mesh-placement", "nets")
    a, b = read_volume_mesh(os.path.join(str(tmp_path / "netsply"), pid)), read_volume_mesh(os.path.join(str(mesh), pid))
    assert a["quads"].tobytes() == b["quads"].tobytes() and a["vertices"].tobytes() != b["vertices"].tobytes()
    assert a["comments"][1] == "placement nets"


def test_cli_refusals(cohort_root, tmp_path):
    def refused(*args, which="img_processing_parallel"):
        r = run_bin(which, *args, "--cpu", "--quiet", "--data-root", cohort_root, "--out", str(tmp_path / "no"))
        assert r.returncode != 0 and not os.path.exists(tmp_path / "no"), args
        return r.stderr
    assert "--volume-mesh needs --mode 3d" in refused("--volume-mesh")
    e = refused("--mode", "3d", "--volume-mesh", "--split-volume", "--gpus", "2")
    assert "--volume-mesh is not available with --split-volume" in e and "drop --split-volume" in e and "or --volume-mesh" in e
    assert "--volume-mesh-placement needs --volume-mesh" in refused("--mode", "3d", "--volume-mesh-placement", "nets")
    assert "--volume-mesh-format needs --volume-mesh" in refused("--mode", "3d", "--volume-mesh-format", "stl")
    assert "--volume-mesh-max-mb needs --volume-mesh" in refused("--mode", "3d", "--volume-mesh-max-mb", "5")
    assert "--volume-mesh-placement must be corner or nets" in refused("--mode", "3d", "--volume-mesh", "--volume-mesh-placement", "mid")
    assert "--volume-mesh-format must be ply or stl" in refused("--mode", "3d", "--volume-mesh", "--volume-mesh-format", "obj")
    for bad in ("-1", "x", "1.5", "", "9999999"):
        assert "--volume-mesh-max-mb must be an integer" in refused("--mode", "3d", "--volume-mesh", "--volume-mesh-max-mb", bad)
    r = run_bin("nm03_bench", "--config", "cohort", "--volume-mesh", "--data-root", cohort_root)
    assert r.returncode != 0 and "--volume-mesh needs --config volume and the GPU (not --host-only)" in r.stderr
    r = run_bin("nm03_bench", "--config", "volume", "--host-only", "--volume-mesh", "--data-root", cohort_root)
    assert r.returncode != 0 and "--host-only" in r.stderr
    r = run_bin("img_processing_parallel", "--help")
    for flag in ("--volume-mesh ", "--volume-mesh-placement", "--volume-mesh-format", "--volume-mesh-max-mb"):
        assert flag in r.stdout + r.stderr


def test_cli_cap_below_the_mesh_fails_the_patient(cohort_root, cpu_runs, tmp_path):
    mesh, _ = cpu_runs
    sizes = {os.path.dirname(p): json.loads(b) for p, b in tree(mesh).items() if os.path.basename(p) == "mesh.json"}
    assert all(12 * r["vertices"] + 8 * r["triangles"] > 0 for r in sizes.values())
    r = _cli(cohort_root, tmp_path / "cap", "--volume-mesh", "--volume-mesh-max-mb", "0", ok=False)
    run = json.load(open(str(tmp_path / "cap") + ".json"))
    assert [p["ok"] for p in run["patients"]] == [False] * 4
    t = tree(tmp_path / "cap") if os.path.exists(tmp_path / "cap") else {}
    assert not [p for p in t if os.path.basename(p) in MESH_FILES]
    for pid, rec in sizes.items():
        msg = f"a mesh of {rec['vertices']} vertices and {rec['triangles'] // 2} quads takes {12 * rec['vertices'] + 8 * rec['triangles']} bytes"
        assert msg in r.stderr and "above the cap of 0 bytes" in r.stderr and "--volume-mesh" in r.stderr
    assert run["volume_mesh"]["patients"] == 0
