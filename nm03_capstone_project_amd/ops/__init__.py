"""torch-tensor entry points of the gfx950 kernels (K1a median, K1b sharpen+band, K2 SRG+morph,
K3 overlay render, K4 JPEG (gray and colour), K5 3D SRG + cube / ball dilation + per-plane border, K6 threshold, K7 mask measurements,
K8 volume measurements, K10 per-lesion volume measurements, K13 per-lesion 3D and axial diameters,
K9 lesion diameters, K11 intensity percentiles and Σ v² of slices and volumes, K12 grey-level co-occurrence
matrices of slices and volumes, K14 orthogonal planes and projections of a volume, K15 the surface
mesh of a volume mask, K16 the Euclidean distance map of a volume mask in physical space with its margin
and thickness, K17 overlap and surface distances between two volume masks, K18 lesion-wise detection scores for
two volume masks) and
plain-PyTorch fp32 references of the same ops (ops.reference).

Every wrapper takes CUDA (HIP) tensors, passes raw device pointers and the current torch stream to
the native launcher and returns torch tensors — there is no CPU/Python fallback: without the
native extension the call raises.
"""
from .kernels import (border3d, compare_volume_lesions, compare_volume_lesions_words, compare_volumes, dilate3d, dilate_volume_mm, jpeg_encode, jpeg_encode_rgb, measure_diameters, measure_intensity,  # noqa: F401
                      measure_mask, measure_texture, measure_volume, measure_volume_diameters, measure_volume_intensity,
                      measure_volume_lesions,
                      measure_volume_texture, median2d, pack_bits,
                      region_grow, region_grow3d, render_overlay, sharpen_band, threshold, unpack_bits, volume_distance, volume_mesh,
                      volume_thickness, volume_views)
from . import reference  # noqa: F401
