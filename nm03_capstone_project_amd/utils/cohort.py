"""Cohort layout helpers (reference main_sequential.cpp:18-30, 93-168) and the synthetic cohort.

`Cohort` is the Python view of what the CLIs discover natively (src/io/cohort.cpp): the
T1-Post-Combined-P001-P020 directory under the data root, its PGBM-* patients, each patient's
T1post series with slices in file-number order, and the out-*/PGBM-XXX output layout
(`work_items`), which is what `Engine.run` / `SlicePipeline` consume."""
import os
from dataclasses import dataclass, field

from .._native import native


def extract_file_number(name):
    return native().extract_file_number(name)


def cohort_dir(data_root):
    return native().cohort_dir(data_root)


def test_slice_path(data_root):
    return native().test_slice_path(data_root)


def find_patient_dirs(cohort_root):
    return native().find_patient_dirs(cohort_root)


def list_patient_series(cohort_root, pid):
    return native().list_patient_series(cohort_root, pid)


def synth_cohort(data_root, patients=20, min_slices=21, max_slices=25, rows=256, cols=256, seed=20250404,
                 threads=8, test_slice=True, decoy=False, signed=False):
    """Write the synthetic T1+C cohort (20 patients × 21–25 slices of 256² by default)."""
    return native().synth_cohort(data_root, patients, min_slices, max_slices, rows, cols, seed, threads,
                                 test_slice, decoy, signed)


@dataclass
class Patient:
    pid: str
    series_dir: str
    files: list = field(default_factory=list)

    def __len__(self):
        return len(self.files)


@dataclass
class Cohort:
    """Patients with a T1post series, in the reference's discovery order. Patients without one
    are listed in `skipped` with the reason (the reference prints and continues,
    main_sequential.cpp:111-121)."""
    root: str
    patients: list = field(default_factory=list)
    skipped: list = field(default_factory=list)  # [(pid, reason)]

    @classmethod
    def discover(cls, data_root=None, cohort_root=None):
        """From a data root (…/T1-Post-Combined-P001-P020 below it) or the cohort directory itself."""
        n = native()
        root = cohort_root if cohort_root is not None else n.cohort_dir(data_root)
        c = cls(root)
        for pid in n.find_patient_dirs(root):
            try:
                series, files = n.list_patient_series(root, pid)
            except Exception as e:  # noqa: BLE001 - per-patient isolation, like the CLIs
                c.skipped.append((pid, str(e)))
                continue
            if not files:
                c.skipped.append((pid, "empty series"))
                continue
            c.patients.append(Patient(pid, series, list(files)))
        return c

    def __len__(self):
        return len(self.patients)

    def __iter__(self):
        return iter(self.patients)

    @property
    def n_slices(self):
        return sum(len(p) for p in self.patients)

    def work_items(self, out_root, create=True):
        """[(dicom path, out_root/PGBM-XXX)] in cohort order — the Engine's work list. With
        create=True the patient output directories are made (not wiped: see
        native().setup_output_dir for the reference's wipe)."""
        items = []
        for p in self.patients:
            od = os.path.join(out_root, p.pid)
            if create:
                os.makedirs(od, exist_ok=True)
            items.extend((f, od) for f in p.files)
        return items


# --measure-texture: the derived (float) columns of measurements.csv and volumes.csv; the seven integer
# columns (glcm_levels … glcm_sum_sq) come back as int like the other integers.
_GLCM_FLOATS = {"glcm_" + k for k in (
    "joint_max", "joint_avg", "joint_var", "joint_entropy", "asm", "contrast", "dissimilarity", "inv_diff", "inv_diff_moment",
    "correlation", "autocorrelation", "cluster_tendency", "cluster_shade", "cluster_prominence", "sum_entropy", "diff_entropy")}


def read_measurements(out_dir):
    """Rows of <out_dir>/measurements.csv (written by the CLIs with --measure) as dicts keyed by the
    header: one per slice (`status` "ok" or the failure's name, then empty fields) and one per patient
    with file == "TOTAL" carrying the summed area_px and area_mm2. With --measure-diameters the rows also
    have the diameter columns (lesion_px … major_angle_deg, arrays flattened), and a TOTAL row the
    patient's largest bidimensional_mm2 with the major_mm and perp_mm of that slice. With
    --measure-intensity the rows also have the 13 intensity columns (raw_sum_sq, raw_p10 … raw_p90, std,
    p10 … p90, iqr; empty in TOTAL rows), with --measure-texture the 23 glcm_ columns alike. Integer columns
    come back as int, the derived ones as float, empty fields as None."""
    import csv
    import os
    floats = {"area_mm2", "centroid_x", "centroid_y", "centroid_x_mm", "centroid_y_mm", "mean", "major_mm", "perp_mm",
              "bidimensional_mm2", "major_angle_deg", "std", "p10", "p25", "median", "p75", "p90", "iqr"} | _GLCM_FLOATS
    text = {"patient", "file", "status"}
    rows = []
    with open(os.path.join(out_dir, "measurements.csv"), newline="") as f:
        for r in csv.DictReader(f):
            rows.append({k: v if k in text else None if v == "" else float(v) if k in floats else int(v)
                         for k, v in r.items()})
    return rows


def read_volume_measurements(out_dir):
    """Rows of <out_dir>/volumes.csv (written by the 3D CLI with --measure-volume) as dicts keyed by
    the header: one per patient in plan order (`status` "ok", or "failed" and then empty fields). With
    --measure-intensity the rows also have the 13 intensity columns, with --measure-texture the 23 glcm_ ones, with
    --measure-volume-thickness inscribed_um2, inscribed_x / _y / _z (int), inscribed_radius_mm and thickness_mm (float).
    Integer columns come back as int, spacings and the derived ones as float, empty fields as None."""
    import csv
    import os
    floats = {"spacing_x", "spacing_y", "spacing_z", "volume_mm3", "volume_ml", "surface_mm2", "centroid_x",
              "centroid_y", "centroid_z", "centroid_x_mm", "centroid_y_mm", "centroid_z_mm", "mean", "std", "p10", "p25",
              "median", "p75", "p90", "iqr", "inscribed_radius_mm", "thickness_mm"} | _GLCM_FLOATS
    text = {"patient", "status", "spacing_z_source"}
    rows = []
    with open(os.path.join(out_dir, "volumes.csv"), newline="") as f:
        for r in csv.DictReader(f):
            rows.append({k: v if k in text else None if v == "" else float(v) if k in floats else int(v)
                         for k, v in r.items()})
    return rows


def read_volume_lesions(out_dir):
    """Rows of <out_dir>/lesions.csv (written by the 3D CLI with --measure-volume-lesions) as dicts keyed
    by the header: one per reported lesion, patients in plan order, `lesion` the 0-based rank (largest
    first). A failed patient has one row with its status name in `lesion` and None in every field.
    Integer columns come back as int, the derived ones as float. With --measure-volume-diameters the table
    also has the diameter columns (major_um2 … axial_perp_yd as int, diameter_3d_mm, axial_major_mm,
    axial_perp_mm and axial_bidimensional_mm2 as float; None for a lesion measured without the flag)."""
    import csv
    import os
    floats = {"volume_mm3", "volume_ml", "surface_mm2", "equivalent_diameter_mm", "centroid_x", "centroid_y", "centroid_z",
              "centroid_x_mm", "centroid_y_mm", "centroid_z_mm", "mean", "diameter_3d_mm", "axial_major_mm", "axial_perp_mm",
              "axial_bidimensional_mm2"}
    rows = []
    with open(os.path.join(out_dir, "lesions.csv"), newline="") as f:
        for r in csv.DictReader(f):
            row = {}
            for k, v in r.items():
                if k == "patient":
                    row[k] = v
                elif k == "lesion":
                    row[k] = int(v) if v.isdigit() else v
                else:
                    row[k] = None if v == "" else float(v) if k in floats else int(v)
            rows.append(row)
    return rows


VOLUME_VIEW_NAMES = ("view_axial", "view_coronal", "view_sagittal", "mip_axial", "mip_coronal", "mip_sagittal")


def read_volume_views(out_dir):
    """The views of one patient directory written by the 3D CLI with --volume-views: the parsed views.json
    (width, height, depth, at_mode, at, mask_bbox, inverted, spacing, views) with two keys added — `json`, the
    sidecar's text, and `files`, a dict of the twelve file names (<view>_original.jpg, <view>_processed.jpg
    in the sidecar's view order) → their bytes."""
    import json
    import os
    with open(os.path.join(out_dir, "views.json")) as f:
        text = f.read()
    rec = json.loads(text)
    rec["json"] = text
    rec["files"] = {}
    for v in rec["views"]:
        for kind in ("original", "processed"):
            name = f"{v['name']}_{kind}.jpg"
            with open(os.path.join(out_dir, name), "rb") as f:
                rec["files"][name] = f.read()
    return rec


def read_volume_mesh(path):
    """The mesh.ply the 3D CLI writes with --volume-mesh (binary little-endian PLY; `path` is the file or the
    patient directory that holds it) → dict: vertices (float32 [V, 3], mm), triangles (int32 [T, 3]), quads
    (int32 [T / 2, 4]: the writer stores every quad (q0, q1, q2, q3) as the triangles (q0, q1, q2) and
    (q0, q2, q3)) and comments (the header's comment lines)."""
    import os

    import numpy as np
    if os.path.isdir(path):
        path = os.path.join(path, "mesh.ply")
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary_little_endian 1.0 is read")
    counts = {}
    for ln in lines:
        parts = ln.split()
        if len(parts) == 3 and parts[0] == "element":
            counts[parts[1]] = int(parts[2])
    nv, nf = counts.get("vertex", 0), counts.get("face", 0)
    body = end + len(b"end_header\n")
    if len(data) != body + 12 * nv + 13 * nf:
        raise ValueError(f"{path}: {len(data)} bytes, expected {body + 12 * nv + 13 * nf}")
    verts = np.frombuffer(data, dtype="<f4", count=3 * nv, offset=body).reshape(nv, 3).copy()
    faces = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=nf, offset=body + 12 * nv)
    if nf and not (faces["n"] == 3).all():
        raise ValueError(f"{path}: a face is not a triangle")
    tri = faces["v"].astype(np.int32).reshape(nf, 3)
    quads = np.concatenate([tri[0::2], tri[1::2, 2:3]], axis=1) if nf else np.zeros((0, 4), dtype=np.int32)
    return {"vertices": verts, "triangles": tri, "quads": quads.astype(np.int32),
            "comments": [ln[len("comment "):] for ln in lines if ln.startswith("comment ")]}


def read_volume_comparisons(out_dir):
    """Rows of <out_dir>/comparisons.csv (written by the 3D CLI with --compare-to) as dicts keyed by the header:
    one per patient in plan order. `status` is "ok", "no_reference" (the reference tree has no mask for the
    patient) or "shape_mismatch"; the two latter leave every field None. Integer columns come back as int
    (arrays flattened: compare_spacing_um_x / _y / _z, worst_ab_x …), `reference` as text, the derived ones
    (dice … assd_mm) as float. With --compare-lesions the table has nine more columns: lesions_a … multi_b as int,
    lesion_sensitivity, lesion_precision and lesion_f1 as float."""
    import csv
    import os
    floats = {"dice", "jaccard", "sensitivity", "precision", "volume_a_mm3", "volume_b_mm3", "volume_diff_mm3", "hausdorff_mm",
              "hd95_mm", "msd_ab_mm", "msd_ba_mm", "assd_mm", "lesion_sensitivity", "lesion_precision", "lesion_f1"}
    text = {"patient", "status"}
    rows = []
    with open(os.path.join(out_dir, "comparisons.csv"), newline="") as f:
        for r in csv.DictReader(f):
            rows.append({k: v if k in text else None if v == "" else v if k == "reference" else float(v) if k in floats else int(v)
                         for k, v in r.items()})
    return rows


def read_volume_lesion_comparisons(out_dir):
    """Rows of <out_dir>/compare_lesions.csv (written by the 3D CLI with --compare-to and --compare-lesions) as dicts
    keyed by the header: one per reported lesion, side "a" before "b", patients in plan order. `patient` and `side`
    are text, every other column an int (first flattened to first_x / _y / _z; best is -1 for no partner)."""
    import csv
    import os
    text = {"patient", "side"}
    with open(os.path.join(out_dir, "compare_lesions.csv"), newline="") as f:
        return [{k: v if k in text else int(v) for k, v in r.items()} for r in csv.DictReader(f)]


def read_volume_mask(path):
    """The mask.mhd the 3D CLI writes with --volume-mask (`path` is the file or the patient directory that holds
    it) → (uint8 array [D, H, W] of 0 / 1, (sx, sy, sz) in mm). Non-zero means set, as --compare-to reads it."""
    import os

    import numpy as np
    if os.path.isdir(path):
        path = os.path.join(path, "mask.mhd")
    arr, spacing = native().mhd_read(path)
    if arr.ndim == 2:
        arr = arr[None]
    return (np.asarray(arr) != 0).astype(np.uint8), tuple(float(v) for v in spacing)
