"""One DICOM series as a 3D volume on the MI355X: per-slice preprocessing, 6-connected 3D region
growing and a 7×7×7 dilation (BASELINE config 5), checked against the golden 3D model.

    python examples/volume_3d.py --series path/to/series_dir [--ball] [--measure] [--views DIR] [--mesh DIR] [--dilate-mm R [--compare-to-cube [--compare-lesions N]]]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import nm03_capstone_project_amd as nm  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--series", required=True)
    ap.add_argument("--ball", action="store_true", help="digital ball instead of the 7x7x7 cube")
    ap.add_argument("--measure", action="store_true",
                    help="also print the volumetry of the dilated volume (K8: mm3, components, cavities, tunnels) and "
                         "the largest lesion's diameters (K10 + K13)")
    ap.add_argument("--views", metavar="DIR",
                    help="also write the axial / coronal / sagittal planes through the lesion and the three projections "
                         "(K14): twelve JPEGs and views.json into DIR")
    ap.add_argument("--mesh", metavar="DIR",
                    help="also write the surface of the dilated mask as a closed mesh in mm (K15): mesh.ply and mesh.json "
                         "into DIR")
    ap.add_argument("--dilate-mm", type=float, metavar="R",
                    help="dilate by a Euclidean margin of R mm in physical space (K16) instead of the 7x7x7 cube, and print "
                         "the voxel counts of both and the thickness of the dilated volume")
    ap.add_argument("--compare-to-cube", action="store_true",
                    help="with --dilate-mm: also score the margin's mask against the default 7x7x7 cube's (K17) and print "
                         "Dice and the surface distances")
    ap.add_argument("--compare-lesions", type=int, default=0, metavar="N",
                    help="with --compare-to-cube: also compare the two masks lesion by lesion (K18, N reported lesions per side) "
                         "and print the totals")
    a = ap.parse_args(argv)
    margin = a.dilate_mm is not None
    if a.compare_to_cube and not margin:
        ap.error("--compare-to-cube needs --dilate-mm R")
    if a.compare_lesions and not a.compare_to_cube:
        ap.error("--compare-lesions needs --compare-to-cube")
    if not 0 <= a.compare_lesions <= 64:
        ap.error("--compare-lesions must be 1..64")
    cube_mask = None
    if a.compare_to_cube:  # the reference: a run with the default cube; `run` returns `dilated`, so it could be saved as well
        cube_mask = nm.VolumePipeline(nm.PipelineConfig(se_shape=int(a.ball)), connectivity=6, dilation=7).run_series(a.series)["dilated"]
    vp = nm.VolumePipeline(nm.PipelineConfig(se_shape=int(a.ball)), connectivity=6, dilation=7, measure=a.measure or margin,
                           measure_lesions=int(a.measure), measure_diameters=a.measure, views=bool(a.views),
                           mesh=bool(a.mesh), dilate_mm=a.dilate_mm, measure_thickness=margin, compare_to=cube_mask,
                           compare_reference="cube", compare_lesions=a.compare_lesions)
    res = vp.run_series(a.series)
    band = res["band"]
    g = nm.utils.series_geometry(a.series)
    region, dil = vp.golden(band, vp.default_seeds(band), spacing=(g["spacing_x"], g["spacing_y"], g["spacing_z"]))
    same = np.array_equal(res["region"], region) and np.array_equal(res["dilated"], dil)
    print(f"volume {tuple(band.shape)}: region {int(res['region'].sum())} voxels, dilated "
          f"{int(res['dilated'].sum())} voxels, GPU == golden: {same}")
    if margin:
        cube = nm.native().golden_dilate3d(region, 7, False)
        t = res["thickness"]
        print(f"margin of {a.dilate_mm} mm at {g['spacing_x']} x {g['spacing_y']} x {g['spacing_z']} mm: "
              f"{int(res['dilated'].sum())} voxels; the 7x7x7 cube: {int(cube.sum())} voxels")
        if t["found"]:
            print(f"thickness {t['thickness_mm']:.3f} mm (inscribed radius {t['inscribed_radius_mm']:.3f} mm at "
                  f"{tuple(t['inscribed_at'])})")
        else:
            print("thickness: none (empty mask, or no background in the frame)")
    if a.compare_to_cube:
        import json
        c = json.loads(res["compare_json"])
        if c["found_ab"]:
            print(f"margin against the cube: Dice {c['dice']:.4f}, Jaccard {c['jaccard']:.4f}, Hausdorff {c['hausdorff_mm']:.3f} mm, "
                  f"HD95 {c['hd95_mm']:.3f} mm, ASSD {c['assd_mm']:.3f} mm ({c['surface_a']} and {c['surface_b']} surface voxels)")
        else:
            print(f"margin against the cube: {c['a_vox']} and {c['b_vox']} voxels, no surface distances (an empty mask)")
        if a.compare_lesions:
            f1 = "none" if c["lesion_f1"] is None else f"{c['lesion_f1']:.4f}"
            print(f"lesions (connectivity {c['lesions_connectivity']}): margin {c['lesions_a']} ({c['hit_a']} hit, {c['multi_a']} merging), "
                  f"cube {c['lesions_b']} ({c['hit_b']} hit, {c['multi_b']} split), F1 {f1}")
    if a.measure:
        import json
        m = json.loads(res["measure_json"])
        print(f"volume {m['volume_ml']:.3f} ml ({m['volume_vox']} voxels, spacing_z {m['spacing_z']} mm from "
              f"{m['spacing_z_source']}), surface {m['surface_mm2']:.1f} mm2, {m['components']} component(s), "
              f"{m['cavities']} cavities, {m['tunnels']} tunnels")
        for les in m["lesions"][:1]:
            print(f"largest lesion: {les['voxels']} voxels, 3D diameter {les['diameter_3d_mm']:.1f} mm, axial "
                  f"{les['axial_major_mm']:.1f} x {les['axial_perp_mm']:.1f} mm in plane {les['axial_z']} "
                  f"(spacing {m['diameters_spacing_um']} um)")
    if a.views:
        os.makedirs(a.views, exist_ok=True)
        for name, data in res["views_jpeg"].items():
            with open(os.path.join(a.views, name), "wb") as f:
                f.write(data)
        with open(os.path.join(a.views, "views.json"), "w") as f:
            f.write(res["views_json"])
        print(f"views through {res['views_at']}: {len(res['views_jpeg'])} files and views.json in {a.views}")
    if a.mesh:
        os.makedirs(a.mesh, exist_ok=True)
        with open(os.path.join(a.mesh, "mesh.ply"), "wb") as f:
            f.write(res["mesh_file"])
        with open(os.path.join(a.mesh, "mesh.json"), "w") as f:
            f.write(res["mesh_json"])
        m = res["mesh"]
        print(f"mesh: {len(m['vertices'])} vertices, {len(m['quads'])} quads ({2 * len(m['quads'])} triangles) of "
              f"{m['voxels']} voxels: mesh.ply and mesh.json in {a.mesh}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
