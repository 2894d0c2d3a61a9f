"""DICOM / JPEG / cohort helpers and the synthetic T1+C cohort."""
from .cohort import (Cohort, Patient, cohort_dir, extract_file_number, find_patient_dirs,  # noqa: F401
                     list_patient_series, read_measurements, read_volume_lesions, read_volume_measurements,
                     read_volume_comparisons, read_volume_lesion_comparisons, read_volume_mask, read_volume_mesh, read_volume_views, synth_cohort,
                     test_slice_path)
from .dicom import (Slice, dicom_bytes, load_slice, parse_dicom, read_series, read_slice, series_files,  # noqa: F401
                    series_geometry)
