"""3D mode (BASELINE config 5): a series as one volume, per-slice median/sharpen/band, 6- or
26-connected seeded region growing by LDS plane sweeps, and separable cube dilation (size odd, in
[1, 63]). `run` raises ValueError for a connectivity other than 6 / 26 or a size outside that range
(the native runner checks them before any launch).

With `measure=True` every run also measures the dilated volume on the GPU (K8, nm03/measure.h
VolumeMeasure): the result gains `measure` (the record's integers) and `measure_json` (the text of the
CLI's volume_measure.json, from the one native volume_to_json). With `measure_lesions=N` (1 … 64; needs
`measure`) the K10 kernels also report the N largest connected components: the result gains `lesions`
(a list of dicts of each record's integers, largest first) and `measure_json` is the longer text with
the `lesions_max` / `lesions` keys. With `measure_intensity=True` (needs `measure`) the K11 kernels also
report the exact 10/25/50/75/90th percentile and the sum of squares of the samples under the dilated
volume: the result gains `intensity` (the record's integers) and `measure_json` carries the intensity
keys after `mean` (before the lesion keys). With `measure_texture=True` (needs `measure`) the K12 kernels
also report the grey-level co-occurrence matrix of those samples at `texture_levels` grey levels over the
thirteen forward directions: the result gains `texture` (the header integers plus `glcm`) and
`measure_json` carries the 23 texture keys after the intensity keys (before the lesion keys). With
`measure_diameters=True` (needs `measure` and `measure_lesions` ≥ 1) the K13 kernels also report every
lesion's 3D major diameter, largest axial diameter and its perpendicular, maximised in the spacing quantised
to integer micrometres: the result gains `diameters` (a list of dicts of each record's integers, in the
lesions' order) and `measure_json` carries `diameters_spacing_um` and the diameter keys of every lesion.

With `views=True` every run also exports the views that use the third axis (K14, nm03/volume_views.h): the
axial, coronal and sagittal plane through a point and the projections along z, y and x, from the volume
still on the device. `views_at` is "mask" (default: the centre of the dilated mask's bounding box, the
volume's centre when the mask is empty), "centre" or a voxel (x, y, z). The result gains `views` (a dict
name → {width, height, raw, mask, raw_min, raw_max, mask_px}), `views_at` (x, y, z), `views_json` (the text
of the CLI's views.json, from the one native writer) and `views_jpeg` (file name → the bytes of the twelve
JPEGs the CLI writes, rendered at the config's canvas, quality, sampling and filter).

With `mesh=True` every run also extracts the surface of the dilated mask as a closed, indexed quad mesh in
millimetres (K15, nm03/volume_mesh.h) from the bit planes still on the device. `mesh_placement` is "corner"
or "nets", `mesh_format` "ply" or "stl", `mesh_max_mb` the cap on 12 · V + 16 · Q bytes (a larger mesh raises
RuntimeError). The result gains `mesh` (vertices float32 [V, 3], quads int32 [Q, 4], quads_x / _y / _z,
voxels), `mesh_file` (the bytes of the CLI's mesh.ply / mesh.stl) and `mesh_json` (the text of mesh.json),
both from the one native writer.

With `dilate_mm=R` (0 … 1000) the dilation is the Euclidean margin of R millimetres around the region in
physical space (K16, nm03/volume_distance.h: { p : D_region(p) ≤ r² }, r = llround(R · 1000) µm, at the spacing
quantised to integer micrometres) instead of the cube / ball of `dilation` index steps; everything downstream
reads that mask. With `measure_thickness=True` (needs `measure`) K16 also reports the largest ball inscribed in
the dilated volume: the result gains `thickness` (inscribed_um2, inscribed_at, found, inscribed_radius_mm,
thickness_mm) and `measure_json` carries the thickness keys after the texture keys.

With `compare_to=B` (a [D, H, W] array of the volume's shape, non-zero = set) every run also scores its dilated mask
A against B (K17, nm03/volume_compare.h): overlap counts, both surfaces and, in each direction, the largest, the
summed and the 95th-percentile surface-to-surface distance in physical space. The result gains `compare` (the
record's integers, keyed as compare.json), `compare_json` (the text of the CLI's compare.json, from the one native
writer, with `compare_reference` as its `reference`) and `compare_s`. `run` returns `dilated` as it always does, so
a caller can save it (native().mhd_write) and compare a later run against it. It needs no `measure`.

With `compare_lesions=N` (1..64, needs `compare_to`) the two masks are also compared lesion by lesion (K18,
nm03/volume_compare_lesions.h) at `measure_connectivity`: the result gains `compare_lesions` (the dict of
ops.compare_volume_lesions, `table` as an int64 array) and `compare_lesions_s`, and `compare_json` is the longer text
with the lesion keys after assd_mm."""
import numpy as np

from .._native import native
from .pipeline import PipelineConfig


def _meta_args(meta):
    meta = meta or {}
    return dict(type=str(meta.get("type", "u16")), stored_bits=int(meta.get("stored_bits", 16)),
                slope=float(meta.get("slope", 1.0)), intercept=float(meta.get("intercept", 0.0)))


class VolumePipeline:
    def __init__(self, config: PipelineConfig = None, connectivity: int = 6, dilation: int = 7, measure: bool = False,
                 measure_connectivity: int = 26, measure_lesions: int = 0, measure_intensity: bool = False, measure_texture: bool = False,
                 texture_levels: int = 32, measure_diameters: bool = False, views: bool = False, views_at="mask",
                 mesh: bool = False, mesh_placement: str = "corner", mesh_format: str = "ply", mesh_max_mb: int = 512,
                 dilate_mm=None, measure_thickness: bool = False, compare_to=None, compare_reference: str = "",
                 compare_lesions: int = 0):
        self.config = config or PipelineConfig()
        self.connectivity = connectivity
        self.dilation = dilation
        self.measure = bool(measure)
        self.measure_connectivity = int(measure_connectivity)
        if self.measure_connectivity not in (6, 26):
            raise ValueError(f"3D measurement connectivity must be 6 or 26 (got {measure_connectivity})")
        self.measure_lesions = int(measure_lesions)
        if self.measure_lesions and not self.measure:
            raise ValueError("measure_lesions needs measure=True")
        if not 0 <= self.measure_lesions <= 64:
            raise ValueError(f"measure_lesions must be 0 (off) or 1..64 (got {measure_lesions})")
        self.measure_intensity = bool(measure_intensity)
        if self.measure_intensity and not self.measure:
            raise ValueError("measure_intensity needs measure=True")
        self.measure_texture = bool(measure_texture)
        self.texture_levels = int(texture_levels)
        if self.measure_texture and not self.measure:
            raise ValueError("measure_texture needs measure=True")
        if self.measure_texture and not 2 <= self.texture_levels <= 64:
            raise ValueError(f"texture_levels must be 2..64 (got {texture_levels})")
        self.measure_diameters = bool(measure_diameters)
        if self.measure_diameters and not (self.measure and self.measure_lesions >= 1):
            raise ValueError("measure_diameters needs measure=True and measure_lesions >= 1")
        self.views = bool(views)
        self.views_at = views_at if isinstance(views_at, str) else tuple(int(v) for v in views_at)
        if self.views_at not in ("mask", "centre") and not (isinstance(self.views_at, tuple) and len(self.views_at) == 3):
            raise ValueError(f"views_at must be 'mask', 'centre' or (x, y, z) (got {views_at!r})")
        if self.views and self.config.host_only:
            raise ValueError("views are extracted, rendered and encoded on the GPU: not available with host_only")
        self.mesh = bool(mesh)
        self.mesh_placement = str(mesh_placement)
        self.mesh_format = str(mesh_format)
        self.mesh_max_mb = int(mesh_max_mb)
        if self.mesh_placement not in ("corner", "nets"):
            raise ValueError(f"mesh_placement must be 'corner' or 'nets' (got {mesh_placement!r})")
        if self.mesh_format not in ("ply", "stl"):
            raise ValueError(f"mesh_format must be 'ply' or 'stl' (got {mesh_format!r})")
        if self.mesh_max_mb < 0:
            raise ValueError(f"mesh_max_mb must not be negative (got {mesh_max_mb})")
        if self.mesh and self.config.host_only:
            raise ValueError("the mesh is extracted on the GPU: not available with host_only")
        self.dilate_mm = None if dilate_mm is None else float(dilate_mm)
        if self.dilate_mm is not None and not 0.0 <= self.dilate_mm <= 1000.0:  # NaN fails both comparisons
            raise ValueError(f"dilate_mm must be a finite number in [0, 1000] (got {dilate_mm})")
        self.measure_thickness = bool(measure_thickness)
        if self.measure_thickness and not self.measure:
            raise ValueError("measure_thickness needs measure=True")
        if (self.dilate_mm is not None or self.measure_thickness) and self.config.host_only:
            raise ValueError("the distance map is computed on the GPU: not available with host_only")
        self.compare_to = None if compare_to is None else np.ascontiguousarray(np.asarray(compare_to) != 0, dtype=np.uint8)
        self.compare_reference = str(compare_reference)
        if self.compare_to is not None and self.compare_to.ndim != 3:
            raise ValueError("compare_to must be [D, H, W]")
        if self.compare_to is not None and self.config.host_only:
            raise ValueError("the comparison runs on the GPU: not available with host_only")
        self.compare_lesions = int(compare_lesions)
        if not 0 <= self.compare_lesions <= 64:
            raise ValueError(f"compare_lesions must be 0 (off) or 1..64 (got {compare_lesions})")
        if self.compare_lesions and self.compare_to is None:
            raise ValueError("compare_lesions needs compare_to")
        self._runners = {}  # device -> native VolumeRunner (buffers/stream reused across volumes)

    def default_seeds(self, volume):
        d, h, w = volume.shape
        return [(x, y, d // 2) for (x, y) in native().reference_seeds(w, h)]

    def run(self, volume, seeds=None, device=None, spacing=(1.0, 1.0, 1.0), spacing_z_source="default", meta=None):
        """`spacing` = (sx, sy, sz) in mm and `spacing_z_source` only enter `measure_json`. `meta`
        (type, stored_bits, slope, intercept as utils.read_slice gives them; default: unsigned 16-bit
        samples, no rescale) says how the samples are stored."""
        vol = np.ascontiguousarray(volume, dtype=np.uint16)
        s = list(seeds) if seeds is not None else self.default_seeds(vol)
        dev = self.config.device if device is None else device
        runner = self._runners.get(dev)
        if runner is None:
            runner = self._runners[dev] = native().VolumeRunner(dev)
        if self.views and isinstance(self.views_at, tuple):  # before anything is launched
            d, h, w = vol.shape
            x, y, z = self.views_at
            if not (0 <= x < w and 0 <= y < h and 0 <= z < d):
                raise ValueError(f"views_at: the point ({x}, {y}, {z}) lies outside the volume of {w} x {h} x {d}")
        if self.compare_to is not None:
            if self.compare_to.shape != vol.shape:  # before anything is launched
                raise ValueError(f"compare_to: shape mismatch: the reference is {self.compare_to.shape}, the volume {vol.shape}")
            res = runner.run(vol, self.config.pipeline_params(), self.connectivity, self.dilation, s, measure=self.measure,
                             measure_connectivity=self.measure_connectivity, spacing=[float(v) for v in spacing],
                             spacing_z_source=str(spacing_z_source), measure_lesions=self.measure_lesions,
                             measure_intensity=self.measure_intensity, measure_texture=self.measure_texture,
                             texture_levels=self.texture_levels, measure_diameters=self.measure_diameters,
                             dilate_um=-1 if self.dilate_mm is None else native().dilate_mm_to_um(self.dilate_mm),
                             measure_thickness=self.measure_thickness, compare_to=self.compare_to,
                             compare_reference=self.compare_reference, compare_lesions=self.compare_lesions, **_meta_args(meta))
        elif not self.measure and meta is None and self.dilate_mm is None:
            res = runner.run(vol, self.config.pipeline_params(), self.connectivity, self.dilation, s)
        elif self.dilate_mm is not None or self.measure_thickness:
            res = runner.run(vol, self.config.pipeline_params(), self.connectivity, self.dilation, s, measure=self.measure,
                             measure_connectivity=self.measure_connectivity, spacing=[float(v) for v in spacing],
                             spacing_z_source=str(spacing_z_source), measure_lesions=self.measure_lesions,
                             measure_intensity=self.measure_intensity, measure_texture=self.measure_texture,
                             texture_levels=self.texture_levels, measure_diameters=self.measure_diameters,
                             dilate_um=-1 if self.dilate_mm is None else native().dilate_mm_to_um(self.dilate_mm),
                             measure_thickness=self.measure_thickness, **_meta_args(meta))
        else:
            res = runner.run(vol, self.config.pipeline_params(), self.connectivity, self.dilation, s, measure=self.measure,
                             measure_connectivity=self.measure_connectivity, spacing=[float(v) for v in spacing],
                             spacing_z_source=str(spacing_z_source), measure_lesions=self.measure_lesions,
                             measure_intensity=self.measure_intensity, measure_texture=self.measure_texture,
                             texture_levels=self.texture_levels, measure_diameters=self.measure_diameters,
                             **_meta_args(meta))
        if self.views:  # K14 on the volume the run left on the device
            d, h, w = vol.shape
            a = _meta_args(meta)
            x = runner.export_views(w, h, d, self.config.pipeline_params(), self.config.render_params(), self.views_at,
                                    [float(v) for v in spacing], a["type"], a["stored_bits"], a["slope"], a["intercept"])
            res["views"] = x["views"]
            res["views_at"] = tuple(x["at"])
            res["views_json"] = x["views_json"]
            res["views_jpeg"] = x["views_jpeg"]
        if self.mesh:  # K15 on the dilated bit planes the run left on the device
            d, h, w = vol.shape
            sp = [float(v) for v in spacing]
            m = runner.export_mesh(w, h, d, self.mesh_placement, sp, self.mesh_max_mb << 20)
            res["mesh"] = m
            res["mesh_file"] = native().volume_mesh_file(m, self.mesh_format)
            res["mesh_json"] = native().volume_mesh_to_json(m, self.mesh_format, len(res["mesh_file"]), sp)
        return res

    def run_series(self, series_dir, seeds=None, device=None):
        """A DICOM series directory as one volume (utils.read_series: the reference's file-number
        order, every slice of one shape) through `run`. When measuring, the series' geometry
        (utils.series_geometry) and the first slice's storage format go with it."""
        from ..utils.dicom import read_series, series_geometry
        vol, slices = read_series(series_dir)
        if not self.measure and not self.views and not self.mesh and self.dilate_mm is None and self.compare_to is None:
            return self.run(vol, seeds=seeds, device=device)
        g = series_geometry(series_dir)
        return self.run(vol, seeds=seeds, device=device, spacing=(g["spacing_x"], g["spacing_y"], g["spacing_z"]),
                        spacing_z_source=g["spacing_z_source"], meta=slices[0].meta)

    def run_slabs(self, volume=None, comm=None, seeds=None, band=None, backend="gpu", gather=True, device=None):
        """The same pipeline on a volume split into z-slabs over the ranks of the native `comm` (one
        process per GPU; parallel/volume_slabs.py). Returns the whole volume's masks on every rank
        with gather=True, else this rank's slab."""
        from ..parallel.volume_slabs import run_volume_slabs
        dev = self.config.device if device is None else device
        runner = None
        if backend == "gpu":
            runner = self._runners.get(dev)
            if runner is None:
                runner = self._runners[dev] = native().VolumeRunner(dev)
        return run_volume_slabs(volume=volume, comm=comm, config=self.config, connectivity=self.connectivity,
                                dilation=self.dilation, seeds=seeds, band=band, backend=backend, gather=gather,
                                device=dev, runner=runner)

    def golden(self, band, seeds, spacing=(1.0, 1.0, 1.0)):
        """`spacing` only enters with dilate_mm: the margin is taken at the spacing quantised to micrometres."""
        n = native()
        region = n.golden_region_grow3d(band, list(seeds), self.connectivity)
        if self.dilate_mm is not None:
            um = n.volume_spacing_um(float(np.float32(spacing[0])), float(np.float32(spacing[1])), float(spacing[2]))
            return region, n.golden_dilate3d_mm(region, list(um), n.dilate_mm_to_um(self.dilate_mm))
        return region, n.golden_dilate3d(region, self.dilation, self.config.se_shape == 1)

    def golden_measure(self, dilated, region, raw, spacing=(1.0, 1.0, 1.0), spacing_z_source="default", meta=None):
        """The golden model's record of `dilated` (+ popcount of `region`) over the samples `raw`
        ([D, H, W] each) at this pipeline's measure_connectivity → (measure dict, measure_json text):
        what `run` returns under those keys when measuring. With measure_lesions the text is the longer
        one and the tuple has a third member, the list of lesion dicts (`run`'s `lesions`). With
        measure_intensity the text carries the intensity keys and the tuple's last member is the intensity
        dict (`run`'s `intensity`). With measure_texture the text carries the texture keys too and the
        texture dict (`run`'s `texture`) comes last of all. With measure_diameters the text carries the diameter
        keys as well and the list of diameter dicts (`run`'s `diameters`) is a further last member. With
        measure_thickness the text carries the thickness keys and the thickness dict (`run`'s `thickness`) is a
        further last member after all of those."""
        out = self._golden_measure_diameters(dilated, region, raw, spacing, spacing_z_source, meta)
        if not self.measure_thickness:
            return out
        n = native()
        um = n.volume_spacing_um(float(np.float32(spacing[0])), float(np.float32(spacing[1])), float(spacing[2]))
        th = n.golden_volume_thickness(np.ascontiguousarray(dilated, dtype=np.uint8), list(um))
        return (out[0], n.volume_insert_thickness_keys(out[1], th, list(um))) + tuple(out[2:]) + (th,)

    def _golden_measure_diameters(self, dilated, region, raw, spacing, spacing_z_source, meta):
        out = self._golden_measure(dilated, region, raw, spacing, spacing_z_source, meta)
        if not self.measure_diameters:
            return out
        n = native()
        um = n.volume_spacing_um(float(np.float32(spacing[0])), float(np.float32(spacing[1])), float(spacing[2]))
        dia = n.golden_measure_volume_diameters(np.ascontiguousarray(dilated, dtype=np.uint8), self.measure_lesions, list(um),
                                                self.measure_connectivity)
        a = _meta_args(meta)
        d, h, w = np.asarray(dilated).shape
        kw = {}
        if self.measure_intensity:
            kw["intensity"] = out[3]
        if self.measure_texture:
            kw["texture"] = out[-1]
        text = n.volume_measure_to_json(out[0], w, h, d, float(spacing[0]), float(spacing[1]), float(spacing[2]),
                                        str(spacing_z_source), a["slope"], a["intercept"],
                                        bool(self.config.pipeline_params().apply_rescale), self.measure_connectivity,
                                        out[2], self.measure_lesions, diameters=dia, **kw)
        return (out[0], text) + tuple(out[2:]) + (dia,)

    def _golden_measure(self, dilated, region, raw, spacing, spacing_z_source, meta):
        n = native()
        a = _meta_args(meta)
        d, h, w = np.asarray(dilated).shape
        rec = n.golden_measure_volume(np.ascontiguousarray(dilated, dtype=np.uint8),
                                      np.ascontiguousarray(region, dtype=np.uint8),
                                      np.ascontiguousarray(raw, dtype=np.uint16), a["type"], a["stored_bits"],
                                      self.measure_connectivity)
        lesions = None
        if self.measure_lesions:
            lesions = n.golden_measure_volume_lesions(np.ascontiguousarray(dilated, dtype=np.uint8),
                                                      np.ascontiguousarray(raw, dtype=np.uint16), self.measure_lesions,
                                                      a["type"], a["stored_bits"], self.measure_connectivity)
        text = n.volume_measure_to_json(rec, w, h, d, float(spacing[0]), float(spacing[1]), float(spacing[2]),
                                        str(spacing_z_source), a["slope"], a["intercept"],
                                        bool(self.config.pipeline_params().apply_rescale), self.measure_connectivity,
                                        lesions, self.measure_lesions)
        if self.measure_texture:
            dil8 = np.ascontiguousarray(dilated, dtype=np.uint8)
            raw16 = np.ascontiguousarray(raw, dtype=np.uint16)
            intensity = (n.golden_measure_volume_intensity(dil8, raw16, a["type"], a["stored_bits"])
                         if self.measure_intensity else None)
            texture = n.golden_measure_volume_texture(dil8, raw16, self.texture_levels, a["type"], a["stored_bits"])
            text = n.volume_measure_to_json(rec, w, h, d, float(spacing[0]), float(spacing[1]), float(spacing[2]),
                                            str(spacing_z_source), a["slope"], a["intercept"],
                                            bool(self.config.pipeline_params().apply_rescale), self.measure_connectivity,
                                            lesions, self.measure_lesions, intensity, texture)
            return tuple(x for x in (rec, text, lesions, intensity) if x is not None) + (texture,)
        if not self.measure_intensity:
            return (rec, text) if lesions is None else (rec, text, lesions)
        intensity = n.golden_measure_volume_intensity(np.ascontiguousarray(dilated, dtype=np.uint8),
                                                      np.ascontiguousarray(raw, dtype=np.uint16), a["type"], a["stored_bits"])
        text = n.volume_measure_to_json(rec, w, h, d, float(spacing[0]), float(spacing[1]), float(spacing[2]),
                                        str(spacing_z_source), a["slope"], a["intercept"],
                                        bool(self.config.pipeline_params().apply_rescale), self.measure_connectivity,
                                        lesions, self.measure_lesions, intensity)
        return (rec, text, intensity) if lesions is None else (rec, text, lesions, intensity)
