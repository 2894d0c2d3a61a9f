// 3D mode: series → volume → per-slice K1 (median, sharpen, band) → K5 3D SRG → cube dilation →
// per-slice K3/K4 export. See include/nm03/volume.h.
#include "nm03/volume.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>

#include "nm03/cohort.h"
#include "nm03/comm.h"
#include "nm03/golden.h"
#include "nm03/thread_pool.h"
#include "nm03/volume_slabs.h"
#include "nm03/dicom.h"
#include "nm03/gpu_types.h"
#include "nm03/jpeg.h"
#include "nm03/kernels.h"
#include "nm03/metaimage.h"

namespace nm03 {

using namespace nm03::gpu;

// Every frame of every file, stacked in file order: a series of single-frame slices, or a
// multi-frame file (one file = one volume), or a mix of both.
double series_spacing_z(const dicom::Header& first, const dicom::Header* second, std::string* source) {
  if (second && first.has_position && second->has_position) {
    double s2 = 0;
    for (int k = 0; k < 3; ++k) s2 += (second->position[k] - first.position[k]) * (second->position[k] - first.position[k]);
    if (s2 > 0) {
      *source = "position";
      return std::sqrt(s2);
    }
  }
  if (first.spacing_between_slices > 0) {
    *source = "spacing_between_slices";
    return first.spacing_between_slices;
  }
  if (first.slice_thickness > 0) {
    *source = "slice_thickness";
    return first.slice_thickness;
  }
  *source = "default";
  return 1.0;
}

SeriesGeometry series_geometry(const std::vector<std::string>& files) {
  if (files.empty()) throw SliceError("series_geometry: no files");
  SeriesGeometry g;
  std::vector<uint8_t> buf;
  size_t n = dicom::read_file_into(files[0], buf);
  const dicom::Header h0 = dicom::parse(buf.data(), n);
  g.spacing_x = h0.spacing_x;
  g.spacing_y = h0.spacing_y;
  dicom::Header h1;
  const bool two = h0.frames == 1 && files.size() > 1;  // the first two planes come from different files
  if (two) {
    n = dicom::read_file_into(files[1], buf);
    h1 = dicom::parse(buf.data(), n);
  }
  g.spacing_z = series_spacing_z(h0, two ? &h1 : nullptr, &g.spacing_z_source);
  return g;
}

VolumeInput load_volume(const std::vector<std::string>& files) {
  VolumeInput v;
  std::vector<uint8_t> buf;
  dicom::Header first;
  for (size_t z = 0; z < files.size(); ++z) {
    const size_t n = dicom::read_file_into(files[z], buf);
    dicom::Header h = dicom::parse(buf.data(), n);
    if (z == 0 || (z == 1 && first.frames == 1))
      v.spacing_z = series_spacing_z(z == 0 ? h : first, z == 0 ? nullptr : &h, &v.spacing_z_source);
    if (z == 0) {
      first = h;
      first.decoded.reset();
      v.w = h.cols;
      v.h = h.rows;
      v.type = h.type == kU8 ? kU16 : h.type;
      v.stored_bits = h.type == kU8 ? 8 : h.bits_stored;
      v.slope = h.slope;
      v.intercept = h.intercept;
      v.spacing_x = h.spacing_x;
      v.spacing_y = h.spacing_y;
      v.raw.reserve((size_t)v.w * v.h * files.size());
    } else if (h.cols != v.w || h.rows != v.h) {
      throw SliceError("volume slices differ in size: " + files[z]);
    }
    const size_t plane = (size_t)v.w * v.h;
    for (int f = 0; f < h.frames; ++f) {
      v.raw.resize(plane * (size_t)(v.d + 1));
      dicom::copy_pixels16(h, buf.data(), n, v.raw.data() + (size_t)v.d * plane, f);
      ++v.d;
    }
  }
  return v;
}

namespace {

struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  explicit DevBuf(size_t bytes) { check_hip(hipMalloc(&p, std::max<size_t>(bytes, 16)), "hipMalloc volume"); }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

PipeConsts make_consts(const PipelineParams& p, int border_radius) {
  PipeConsts pc{};
  pc.nmin = p.norm_min;
  pc.nmax = p.norm_max;
  pc.nlow = p.norm_low;
  pc.nhigh = p.norm_high;
  pc.cmin = p.clip_min;
  pc.cmax = p.clip_max;
  pc.gain = p.sharpen_gain;
  pc.band_lo = p.srg_min;
  pc.band_hi = p.srg_max;
  gaussian_taps(p.sharpen_sigma, p.sharpen_mask, pc.taps);
  pc.mask_radius = p.sharpen_mask / 2;
  pc.median_k = p.median_window;
  pc.connectivity = 4;
  pc.dilation_size = p.dilation_size;
  pc.erosion_size = p.erosion_size;
  pc.border_radius = border_radius;
  pc.se_disc = p.se_shape == kSeDisc ? 1 : 0;
  return pc;
}

struct VolumeDevice {
  int w, h, d, wpr;
  size_t words, ps;
  hipStream_t stream = nullptr;
  DevBuf raw, med, band, region, dil, tmp, desc, medt, shpt, stats, seeds, flag;
  DevBuf srg_scratch, morph_scratch;  // bit planes too large for LDS (a side > 512), else unused
  uint32_t* h_flag = nullptr;         // the region growing's control words (sweep count, error)
  uint8_t* h_tables = nullptr;  // pinned staging: descriptors, tile lists, stats (reused per run)
  size_t n_medt, n_shpt;
  // z-slab decomposition (run_slab): the two neighbour boundary planes, the added-voxel counter
  // and the halo-extended dilation buffers, allocated on first use and kept.
  std::unique_ptr<DevBuf> slab_nb, slab_added, ext, ext_dil, ext_tmp, ext_scr;
  int ext_planes = 0;
  // K8 (VolumeParams::measure): the labelling scratch, the accumulators and the pinned record,
  // allocated by the first measuring run and kept.
  std::unique_ptr<DevBuf> vm_scratch, vm_acc;
  VolumeMeasure* h_measure = nullptr;
  // K10 (VolumeParams::measure_lesions): candidate list, accumulators and the pinned records and count,
  // allocated by the first run that asks for lesions (for kMaxVolumeLesions, so any N fits) and kept.
  std::unique_ptr<DevBuf> vl_work;
  VolumeLesion* h_lesions = nullptr;  // kMaxVolumeLesions records, then the count
  // K13 (VolumeParams::measure_diameters): the work buffer for `vd_lesions` lesions (regrown when a run
  // asks for more) and the pinned records, allocated by the first run that asks for them and kept.
  std::unique_ptr<DevBuf> vd_work;
  int vd_lesions = 0;
  VolumeLesionDiameters* h_diameters = nullptr;  // kMaxVolumeLesions records
  // K11 (VolumeParams::measure_intensity): the accumulators and the pinned record, allocated by the
  // first run that asks for them and kept.
  std::unique_ptr<DevBuf> vi_acc;
  IntensityStats* h_intensity = nullptr;
  // K12 (VolumeParams::measure_texture): the accumulators and the pinned record (for 64 levels, so any
  // level count fits), allocated by the first run that asks for them and kept.
  std::unique_ptr<DevBuf> vt_acc;
  void* h_texture = nullptr;
  // K16 (VolumeParams::dilate_um / measure_thickness): the layout, the scratch of the three passes and the
  // pinned thickness record, allocated by the first run that asks for either and kept.
  VolumeDistanceLayout dist_layout;
  std::unique_ptr<DevBuf> dist_work;
  VolumeThickness* h_thickness = nullptr;
  // K17 (VolumeParams::compare): the layout, the work buffer, the reference's words on the device with their
  // pinned staging, the pinned record and the events of its timing, allocated by the first run that asks for a
  // comparison and kept.
  VolumeCompareLayout cmp_layout;
  std::unique_ptr<DevBuf> cmp_work, cmp_ref;
  uint64_t* h_cmp_ref = nullptr;
  VolumeCompare* h_compare = nullptr;
  hipEvent_t cmp_e0 = nullptr, cmp_e1 = nullptr;
  // K18 (VolumeParams::compare_lesions): the work buffer, the pinned record (sized for 64 lesions) and the events
  // of its timing, allocated by the first run that asks for the lesion-wise comparison and kept.
  std::unique_ptr<DevBuf> cl_work;
  uint8_t* h_cl_record = nullptr;
  hipEvent_t cl_e0 = nullptr, cl_e1 = nullptr;
  VolumeDevice(const VolumeInput& v)
      : w(v.w), h(v.h), d(v.d), wpr((v.w + 63) / 64), words((size_t)v.h * ((v.w + 63) / 64)),
        ps(((size_t)v.w * v.h + 7) / 8 * 8),
        raw(ps * v.d * 2), med(ps * v.d * 2), band(words * v.d * 8), region(words * v.d * 8), dil(words * v.d * 8),
        tmp(words * v.d * 8), desc(sizeof(SliceDesc) * v.d),
        medt(sizeof(TileDesc) * v.d * ((v.w + 63) / 64) * ((v.h + 63) / 64)),
        shpt(sizeof(TileDesc) * v.d * ((v.w + 63) / 64) * ((v.h + kShpTileH - 1) / kShpTileH)), stats(sizeof(SliceStats) * v.d),
        seeds(sizeof(int32_t) * 3 * kMaxSeeds), flag(sizeof(uint32_t) * kSrg3dCtlWords),
        srg_scratch(8 * srg3d_scratch_words(v.w, v.h, v.d)), morph_scratch(8 * morph3d_scratch_words(v.w, v.h, v.d)),
        n_medt((size_t)v.d * ((v.w + 63) / 64) * ((v.h + 63) / 64)),
        n_shpt((size_t)v.d * ((v.w + 63) / 64) * ((v.h + kShpTileH - 1) / kShpTileH)) {
    check_hip(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "stream");
    check_hip(hipHostMalloc((void**)&h_flag, sizeof(uint32_t) * kSrg3dCtlWords, hipHostMallocDefault),
              "hipHostMalloc flag");
    check_hip(hipHostMalloc((void**)&h_tables, table_bytes(), hipHostMallocDefault), "hipHostMalloc tables");
  }
  size_t table_bytes() const {
    return sizeof(SliceDesc) * d + sizeof(TileDesc) * (n_medt + n_shpt) + sizeof(SliceStats) * d;
  }
  ~VolumeDevice() {
    if (h_lesions) (void)hipHostFree(h_lesions);
    if (h_diameters) (void)hipHostFree(h_diameters);
    if (h_intensity) (void)hipHostFree(h_intensity);
    if (h_texture) (void)hipHostFree(h_texture);
    if (h_thickness) (void)hipHostFree(h_thickness);
    if (h_cmp_ref) (void)hipHostFree(h_cmp_ref);
    if (h_compare) (void)hipHostFree(h_compare);
    if (cmp_e0) (void)hipEventDestroy(cmp_e0);
    if (cmp_e1) (void)hipEventDestroy(cmp_e1);
    if (h_cl_record) (void)hipHostFree(h_cl_record);
    if (cl_e0) (void)hipEventDestroy(cl_e0);
    if (cl_e1) (void)hipEventDestroy(cl_e1);
    if (h_measure) (void)hipHostFree(h_measure);
    if (h_tables) (void)hipHostFree(h_tables);
    if (h_flag) (void)hipHostFree(h_flag);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// The 3D kernels' parameter limits, checked before anything is launched: the cube / ball size is odd
// and at most kMorph3dMaxSize (the 2D engine's limit), the connectivity is 6 or 26.
void check_volume_params(int connectivity, int dilation_size) {
  if (connectivity != 6 && connectivity != 26)
    throw std::invalid_argument("3D connectivity must be 6 or 26 (got " + std::to_string(connectivity) + ")");
  if (dilation_size < 1 || dilation_size > kMorph3dMaxSize || !(dilation_size & 1))
    throw std::invalid_argument("3D dilation size must be odd and in [1, " + std::to_string(kMorph3dMaxSize) +
                                "] (got " + std::to_string(dilation_size) + ")");
}

}  // namespace

static void volume_preprocess(VolumeDevice& V, const VolumeInput& v, const PipelineParams& p, const PipeConsts& pc) {
  // Tables are written into pinned staging (valid until the next run, which starts after this
  // run's final sync), so the uploads stay asynchronous.
  auto* hdesc = reinterpret_cast<SliceDesc*>(V.h_tables);
  auto* mt = reinterpret_cast<TileDesc*>(hdesc + v.d);
  auto* st = mt + V.n_medt;
  auto* stats = reinterpret_cast<SliceStats*>(st + V.n_shpt);
  size_t nm = 0, ns = 0;
  for (int z = 0; z < v.d; ++z) {
    SliceDesc& s = hdesc[z];
    std::memset(&s, 0, sizeof(s));
    s.raw_off = (uint32_t)(z * V.ps);
    s.mask_off = (uint32_t)(z * V.words);
    s.w = (uint16_t)v.w;
    s.h = (uint16_t)v.h;
    s.wpr = (uint16_t)V.wpr;
    s.type = v.type;
    s.stored_bits = (uint8_t)v.stored_bits;
    s.slope = p.apply_rescale ? v.slope : 1.f;
    s.intercept = p.apply_rescale ? v.intercept : 0.f;
    for (int ty = 0; ty < (v.h + 63) / 64; ++ty)
      for (int tx = 0; tx < (v.w + 63) / 64; ++tx) mt[nm++] = {(uint32_t)z, (uint16_t)tx, (uint16_t)ty};
    for (int ty = 0; ty < (v.h + kShpTileH - 1) / kShpTileH; ++ty)
      for (int tx = 0; tx < V.wpr; ++tx) st[ns++] = {(uint32_t)z, (uint16_t)tx, (uint16_t)ty};
    stats[z] = SliceStats{0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u};
  }
  const size_t plane = (size_t)v.w * v.h;
  if (V.ps == plane) {  // planes are contiguous on both sides: one copy
    check_hip(hipMemcpyAsync(V.raw.p, v.raw.data(), plane * v.d * 2, hipMemcpyHostToDevice, V.stream), "H2D volume");
  } else {
    for (int z = 0; z < v.d; ++z)
      check_hip(hipMemcpyAsync(V.raw.as<uint16_t>() + z * V.ps, v.raw.data() + z * plane, plane * 2,
                               hipMemcpyHostToDevice, V.stream),
                "H2D volume");
  }
  check_hip(hipMemcpyAsync(V.desc.p, hdesc, sizeof(SliceDesc) * v.d, hipMemcpyHostToDevice, V.stream), "H2D");
  check_hip(hipMemcpyAsync(V.medt.p, mt, sizeof(TileDesc) * nm, hipMemcpyHostToDevice, V.stream), "H2D");
  check_hip(hipMemcpyAsync(V.shpt.p, st, sizeof(TileDesc) * ns, hipMemcpyHostToDevice, V.stream), "H2D");
  check_hip(hipMemcpyAsync(V.stats.p, stats, sizeof(SliceStats) * v.d, hipMemcpyHostToDevice, V.stream), "H2D");
  launch_median(V.raw.as<uint16_t>(), V.med.as<uint16_t>(), V.desc.as<SliceDesc>(), V.medt.as<TileDesc>(), (int)nm,
                pc.median_k, V.stats.as<SliceStats>(), V.stream);
  launch_sharpen_band(V.med.as<uint16_t>(), V.band.as<uint64_t>(), nullptr, V.desc.as<SliceDesc>(),
                      V.shpt.as<TileDesc>(), (int)ns, pc, V.stats.as<SliceStats>(), V.stream);
}

// Enqueues seeding, region growing (convergence decided on the device) and the cube dilation; no
// host synchronisation. The sweep count is read from V.h_flag after the caller's sync.
static void volume_segment(VolumeDevice& V, const VolumeInput& v, const VolumeParams& p) {
  std::vector<int32_t> sx;
  std::vector<Seed> seeds = p.seeds;
  if (seeds.empty()) {
    seeds = reference_seeds(v.w, v.h);
    for (auto& s : seeds) s.z = v.d / 2;
  }
  for (size_t i = 0; i < seeds.size() && i < (size_t)kMaxSeeds; ++i) {
    sx.push_back(seeds[i].x);
    sx.push_back(seeds[i].y);
    sx.push_back(seeds[i].z);
  }
  check_hip(hipMemcpyAsync(V.seeds.p, sx.data(), sx.size() * 4, hipMemcpyHostToDevice, V.stream), "H2D seeds");
  srg_volume(V.band.as<uint64_t>(), V.region.as<uint64_t>(), v.w, v.h, v.d, V.seeds.as<int32_t>(),
             (int)(sx.size() / 3), p.connectivity, V.flag.as<uint32_t>(), V.h_flag,
             V.srg_scratch.as<uint64_t>(), V.stream);
  if (p.dilate_um >= 0)  // K16's margin in place of the cube / ball: three launches, region → dil
    launch_volume_margin(V.region.as<uint64_t>(), V.dist_layout, p.spacing_um, p.dilate_um, V.dist_work->p, V.dil.as<uint64_t>(),
                         V.stream);
  else
    dilate_volume(V.region.as<uint64_t>(), V.dil.as<uint64_t>(), V.tmp.as<uint64_t>(), v.w, v.h, v.d, p.dilation_size,
                  V.stream, V.morph_scratch.as<uint64_t>(), p.pipe.se_shape == kSeDisc);
}

static void unpack_volume(const DevBuf& b, const VolumeDevice& V, std::vector<uint8_t>& out) {
  std::vector<uint64_t> words(V.words * V.d);
  check_hip(hipMemcpy(words.data(), b.p, words.size() * 8, hipMemcpyDeviceToHost), "D2H mask");
  out.assign((size_t)V.w * V.h * V.d, 0);
  for (int z = 0; z < V.d; ++z)
    for (int y = 0; y < V.h; ++y)
      for (int x = 0; x < V.w; ++x)
        out[((size_t)z * V.h + y) * V.w + x] = (words[(size_t)z * V.words + (size_t)y * V.wpr + x / 64] >> (x % 64)) & 1;
}

// GPU export of a processed volume (K3/K4, like the 2D engine): per plane the original (gray render
// of the raw plane, windowed by the median kernel's per-plane stats) and the processed image (the
// 3D dilated mask with its per-plane renderer border), rendered — fused into the encoder for an
// exact 2× fit — and JPEG-encoded in chunks of kExportSlices planes. Images the GPU encoder cannot
// hold (capacity overflow, rare) are re-encoded on the host from their rendered canvas.
constexpr int kExportSlices = 32;
constexpr uint32_t kVolOutCap = 512 * 1024 + 64;  // per image, as the 2D engine

struct ExportBufs {
  int cap = 2 * kExportSlices;  // canvases per launch
  int cw = 0, ch = 0;
  DevBuf bits, canvas, tables, look, ticket, spill;
  JpegWork jw;
  uint8_t* h_tables = nullptr;
  uint8_t* h_out = nullptr;
  uint8_t* d_out = nullptr;
  int32_t* h_sizes = nullptr;
  int32_t* d_sizes = nullptr;
  size_t bits_words = 0;
  ExportBufs(int cw_, int ch_, size_t vol_words)
      : cw(cw_), ch(ch_),
        bits(2 * vol_words * 8),
        canvas((size_t)cw_ * ch_ * 2 * kExportSlices),
        tables(2 * kExportSlices * (sizeof(RenderDesc) + sizeof(JpegDesc)) + 256),
        look(6 * 8 * (size_t)2 * kExportSlices * (((size_t)cw_ * ch_ / 64 + 255) / 256)),
        ticket(4 * 2 * kExportSlices),
        spill(4 * (size_t)2 * kExportSlices * (((size_t)cw_ * ch_ / 64 + 255) / 256) * 256 * 56),
        bits_words(vol_words) {
    const size_t blocks = (size_t)cw * ch / 64;
    jw.look = look.as<uint64_t>();
    jw.look_cap = (size_t)cap * ((blocks + 255) / 256);
    jw.ticket = ticket.as<uint32_t>();
    jw.spill = spill.as<uint32_t>();
    check_hip(hipMemset(jw.ticket, 0, 4 * (size_t)cap), "memset tickets");
    check_hip(hipMemset(jw.look, 0, 6 * jw.look_cap * 8), "memset look-back");
    check_hip(hipHostMalloc((void**)&h_tables, cap * (sizeof(RenderDesc) + sizeof(JpegDesc)) + 256, hipHostMallocDefault),
              "hipHostMalloc export tables");
    check_hip(hipHostMalloc((void**)&h_out, (size_t)kVolOutCap * cap, hipHostMallocMapped), "hipHostMalloc out");
    check_hip(hipHostGetDevicePointer((void**)&d_out, h_out, 0), "device pointer out");
    check_hip(hipHostMalloc((void**)&h_sizes, 4 * (size_t)cap, hipHostMallocMapped), "hipHostMalloc sizes");
    check_hip(hipHostGetDevicePointer((void**)&d_sizes, h_sizes, 0), "device pointer sizes");
  }
  ~ExportBufs() {
    if (h_tables) (void)hipHostFree(h_tables);
    if (h_out) (void)hipHostFree(h_out);
    if (h_sizes) (void)hipHostFree(h_sizes);
  }
};

// K14 (export_views): the six views' sample and bit planes (masks, then their borders), the projection
// scratch, the head (P, box, stats, popcounts) with its pinned copy, the border operator's scratch for
// view planes too large for LDS, and the two extra events of the timing. Allocated by the first
// export_views, kept, rebuilt with the volume.
struct ViewBufs {
  VolumeViewsLayout L;
  DevBuf samples, bits, proj, head, scratch;
  VolumeViewsHead* h_head = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  static size_t scratch_words(const VolumeViewsLayout& l) {
    size_t n = 0;
    for (int i = 0; i < 3; ++i) n = std::max(n, morph3d_scratch_words(l.vw[i], l.vh[i], 2));
    return n;
  }
  explicit ViewBufs(const VolumeViewsLayout& l)
      : L(l), samples(l.samples * 2), bits(l.bit_words * 8), proj(l.proj * 4), head(sizeof(VolumeViewsHead)),
        scratch(8 * scratch_words(l)) {
    check_hip(hipHostMalloc((void**)&h_head, sizeof(VolumeViewsHead), hipHostMallocDefault), "hipHostMalloc views head");
    check_hip(hipEventCreate(&e0), "event");
    check_hip(hipEventCreate(&e1), "event");
    check_hip(hipEventCreate(&e2), "event");
  }
  ~ViewBufs() {
    if (h_head) (void)hipHostFree(h_head);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e2) (void)hipEventDestroy(e2);
  }
};

// K15 (export_mesh): the work buffer of the lattice words (bit words, counts / prefixes, block totals, head),
// the pinned head, the result buffer (positions, then quads; regrown when a mesh needs more) and the events of
// the timing. Allocated by the first export_mesh, kept, rebuilt with the volume or the scan block.
struct MeshBufs {
  VolumeMeshLayout L;
  DevBuf work;
  std::unique_ptr<DevBuf> out;
  size_t out_bytes = 0;
  VolumeMeshHead* h_head = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
  explicit MeshBufs(const VolumeMeshLayout& l) : L(l), work(l.bytes) {
    check_hip(hipHostMalloc((void**)&h_head, sizeof(VolumeMeshHead), hipHostMallocDefault), "hipHostMalloc mesh head");
    for (hipEvent_t* e : {&e0, &e1, &e2, &e3}) check_hip(hipEventCreate(e), "event");
  }
  ~MeshBufs() {
    if (h_head) (void)hipHostFree(h_head);
    for (hipEvent_t e : {e0, e1, e2, e3})
      if (e) (void)hipEventDestroy(e);
  }
};

// Device buffers, stream and events are cached across runs (allocation and stream creation cost
// more than the kernels for a 256³ volume); they are rebuilt only when the volume shape changes.
struct VolumeRunner::Impl {
  int device;
  std::unique_ptr<VolumeDevice> V;
  std::unique_ptr<ExportBufs> X;
  std::unique_ptr<ViewBufs> W;  // K14's buffers (first export_views)
  bool views_loaded = false;    // K14's code object (first export_views)
  std::unique_ptr<MeshBufs> M;  // K15's buffers (first export_mesh)
  bool mesh_loaded = false;     // K15's code object (first export_mesh)
  bool slab_volume = false;     // the volume on the device was left by run_slab
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  bool measure_loaded = false;  // K8's code object (first measuring run)
  bool lesions_loaded = false;  // K10's code object (first run that asks for lesions)
  bool diameters_loaded = false;  // K13's code object (first run that asks for diameters)
  bool intensity_loaded = false;  // K11's code object (first run that asks for the intensity statistics)
  bool texture_loaded = false;    // K12's code object (first run that asks for the texture)
  bool distance_loaded = false;   // K16's code object (first run that asks for a margin in mm, the thickness or a comparison)
  bool compare_loaded = false;    // K17's code object (first run that asks for a comparison)
  bool compare_lesions_loaded = false;  // K18's code object (first run that asks for the lesion-wise comparison)
  explicit Impl(int dev) : device(dev) {
    check_hip(hipSetDevice(device), "hipSetDevice");
    preload_kernels();  // every code object, before the first launch (kernels.h)
    check_hip(hipEventCreate(&e0), "event");
    check_hip(hipEventCreate(&e1), "event");
    check_hip(hipEventCreate(&e2), "event");
  }
  ~Impl() {
    (void)hipSetDevice(device);
    M.reset();
    W.reset();
    X.reset();
    V.reset();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e2) (void)hipEventDestroy(e2);
  }
};

VolumeRunner::VolumeRunner(int device) : impl_(std::make_unique<Impl>(device)) {}
VolumeRunner::~VolumeRunner() = default;

VolumeResult VolumeRunner::run(const VolumeInput& v, const VolumeParams& p, bool want_masks) {
  if (v.d < 1 || v.w < 1 || v.h < 1) throw SliceError("empty volume");
  check_volume_params(p.connectivity, p.dilation_size);
  Impl& I = *impl_;
  check_hip(hipSetDevice(I.device), "hipSetDevice");
  if (!I.V || I.V->w != v.w || I.V->h != v.h || I.V->d != v.d) {
    I.M.reset();
    I.W.reset();
    I.X.reset();
    I.V.reset();
    I.V = std::make_unique<VolumeDevice>(v);
  }
  I.slab_volume = false;
  VolumeDevice& V = *I.V;
  if (p.measure_lesions != 0 && !p.measure)
    throw std::invalid_argument("3D lesion measurements need measure");
  if (p.measure_lesions < 0 || p.measure_lesions > kMaxVolumeLesions)
    throw std::invalid_argument("3D lesion count must be in [1, " + std::to_string(kMaxVolumeLesions) + "] (got " +
                                std::to_string(p.measure_lesions) + ")");
  if (p.measure_diameters && (!p.measure || p.measure_lesions < 1))
    throw std::invalid_argument("3D lesion diameters need measure and a lesion count of at least 1");
  if (p.measure_diameters) {
    for (int a = 0; a < 3; ++a)
      if (p.spacing_um[a] < 1u) throw std::invalid_argument("3D lesion diameters: a spacing must be at least 1 um");
    const std::string ext = measure::volume_diameters_extent_error(v.w, v.h, v.d, p.spacing_um);
    if (!ext.empty()) throw std::invalid_argument("3D lesion diameters: " + ext);
  }
  if (p.measure_intensity && !p.measure) throw std::invalid_argument("3D intensity statistics need measure");
  if (p.measure_texture && !p.measure) throw std::invalid_argument("3D texture needs measure");
  if (p.measure_texture && (p.texture_levels < 2 || p.texture_levels > 64))
    throw std::invalid_argument("3D texture levels must be 2..64 (got " + std::to_string(p.texture_levels) + ")");
  if (p.measure_thickness && !p.measure) throw std::invalid_argument("3D thickness needs measure");
  if (p.dilate_um >= 0 || p.measure_thickness) {
    const char* who = p.dilate_um >= 0 ? "3D margin in millimetres: " : "3D thickness: ";
    if (p.dilate_um > kMaxDilateUm)
      throw std::invalid_argument("3D margin in millimetres: the radius must be at most " + std::to_string(kMaxDilateUm) +
                                  " um (got " + std::to_string(p.dilate_um) + ")");
    for (int a = 0; a < 3; ++a)
      if (p.spacing_um[a] < 1u) throw std::invalid_argument(std::string(who) + "a spacing must be at least 1 um");
    if (v.w > 65535) throw std::invalid_argument(std::string(who) + "a row holds at most 65535 voxels");
    const std::string ext = measure::volume_distance_extent_error(v.w, v.h, v.d, p.spacing_um);
    if (!ext.empty()) throw std::invalid_argument(who + ext);
  }
  if (p.compare) {
    const VolumeReference& ref = *p.compare;
    if (!ref.bits && !ref.mask) throw std::invalid_argument("3D comparison: null buffer (the reference has neither bits nor a mask)");
    if (ref.w != v.w || ref.h != v.h || ref.d != v.d)
      throw std::invalid_argument("3D comparison: shape mismatch: the reference is " + std::to_string(ref.w) + " x " +
                                  std::to_string(ref.h) + " x " + std::to_string(ref.d) + ", the volume " + std::to_string(v.w) +
                                  " x " + std::to_string(v.h) + " x " + std::to_string(v.d));
    for (int a = 0; a < 3; ++a)
      if (p.spacing_um[a] < 1u) throw std::invalid_argument("3D comparison: a spacing must be at least 1 um");
    if (v.w > 65535) throw std::invalid_argument("3D comparison: a row holds at most 65535 voxels");
    if ((uint64_t)v.w * (uint64_t)v.h * (uint64_t)v.d >= (1ull << 32))
      throw std::invalid_argument("3D comparison: a volume of 2^32 voxels or more cannot be compared");
    const std::string ext = measure::volume_distance_extent_error(v.w, v.h, v.d, p.spacing_um);
    if (!ext.empty()) throw std::invalid_argument("3D comparison: " + ext);
  }
  if (p.compare_lesions != 0) {
    if (!p.compare) throw std::invalid_argument("3D lesion comparison: compare_lesions needs a reference (compare)");
    if (p.compare_lesions < 1 || p.compare_lesions > kMaxVolumeLesions)
      throw std::invalid_argument("3D lesion comparison: compare_lesions must be 1.." + std::to_string(kMaxVolumeLesions) + " (got " +
                                  std::to_string(p.compare_lesions) + ")");
    if (p.measure_connectivity != 6 && p.measure_connectivity != 26)
      throw std::invalid_argument("3D lesion comparison: connectivity must be 6 or 26 (got " + std::to_string(p.measure_connectivity) + ")");
    if (volume_measure_scratch_words(v.w, v.h, v.d) == 0)
      throw std::invalid_argument("3D lesion comparison: volume too large to label: (w + 1) * h * d + 1 must stay below 2^32 (got " +
                                  std::to_string(v.w) + " x " + std::to_string(v.h) + " x " + std::to_string(v.d) + ")");
  }
  if (p.measure) {
    if (p.measure_connectivity != 6 && p.measure_connectivity != 26)
      throw std::invalid_argument("3D measurement connectivity must be 6 or 26 (got " +
                                  std::to_string(p.measure_connectivity) + ")");
    const size_t slots = volume_measure_scratch_words(v.w, v.h, v.d);
    if (slots == 0 || V.ps * (size_t)v.d > 0xFFFFFFFFull)
      throw std::invalid_argument("volume too large to measure: (w + 1) * h * d + 1 must stay below 2^32 (got " +
                                  std::to_string(v.w) + " x " + std::to_string(v.h) + " x " + std::to_string(v.d) + ")");
    // First use: K8's code object, before this run's first launch, while the stream is idle (the
    // previous run ended with a synchronisation); then its buffers, kept like the others.
    if (!I.measure_loaded) {
      preload_volume_measure();
      I.measure_loaded = true;
    }
    if (!V.vm_scratch) {
      V.vm_scratch = std::make_unique<DevBuf>(slots * sizeof(uint32_t));
      V.vm_acc = std::make_unique<DevBuf>(kVolumeMeasureAccWords * sizeof(uint64_t));
      check_hip(hipHostMalloc((void**)&V.h_measure, sizeof(VolumeMeasure), hipHostMallocDefault), "hipHostMalloc measure");
    }
    if (p.measure_lesions) {  // K10 alike
      if (!I.lesions_loaded) {
        preload_volume_lesions();
        I.lesions_loaded = true;
      }
      if (!V.vl_work) {
        V.vl_work = std::make_unique<DevBuf>(volume_lesions_work_bytes(v.w, v.h, v.d, kMaxVolumeLesions));
        check_hip(hipHostMalloc((void**)&V.h_lesions, sizeof(VolumeLesion) * (kMaxVolumeLesions + 1), hipHostMallocDefault),
                  "hipHostMalloc lesions");
      }
    }
    if (p.measure_diameters) {  // K13 alike; its row table grows with N
      if (!I.diameters_loaded) {
        preload_volume_diameters();
        I.diameters_loaded = true;
      }
      if (!V.vd_work || V.vd_lesions < p.measure_lesions) {
        V.vd_work.reset();
        V.vd_work = std::make_unique<DevBuf>(volume_diameters_work_bytes(v.w, v.h, v.d, p.measure_lesions));
        V.vd_lesions = p.measure_lesions;
      }
      if (!V.h_diameters)
        check_hip(hipHostMalloc((void**)&V.h_diameters, sizeof(VolumeLesionDiameters) * kMaxVolumeLesions, hipHostMallocDefault),
                  "hipHostMalloc diameters");
    }
    if (p.measure_intensity) {  // K11 alike
      if (!I.intensity_loaded) {
        preload_volume_intensity();
        I.intensity_loaded = true;
      }
      if (!V.vi_acc) {
        V.vi_acc = std::make_unique<DevBuf>(kVolumeIntensityAccBytes);
        check_hip(hipHostMalloc((void**)&V.h_intensity, sizeof(IntensityStats), hipHostMallocDefault), "hipHostMalloc intensity");
      }
    }
    if (p.measure_texture) {  // K12 alike
      if (!I.texture_loaded) {
        preload_volume_texture();
        I.texture_loaded = true;
      }
      if (!V.vt_acc) {
        V.vt_acc = std::make_unique<DevBuf>(kVolumeTextureAccBytes);
        check_hip(hipHostMalloc(&V.h_texture, glcm_record_bytes(64), hipHostMallocDefault), "hipHostMalloc texture");
      }
    }
  }
  if (p.dilate_um >= 0 || p.measure_thickness) {  // K16 alike, after every check of this run
    if (!I.distance_loaded) {
      preload_volume_distance();
      I.distance_loaded = true;
    }
    if (!V.dist_work) {
      V.dist_layout = volume_distance_layout(v.w, v.h, v.d);
      V.dist_work = std::make_unique<DevBuf>(V.dist_layout.bytes);
    }
    if (p.measure_thickness && !V.h_thickness)
      check_hip(hipHostMalloc((void**)&V.h_thickness, sizeof(VolumeThickness), hipHostMallocDefault), "hipHostMalloc thickness");
  }
  if (p.compare) {  // K17 alike, after every check of this run; it launches K16's map
    if (!I.distance_loaded) {
      preload_volume_distance();
      I.distance_loaded = true;
    }
    if (!I.compare_loaded) {
      preload_volume_compare();
      I.compare_loaded = true;
    }
    if (!V.cmp_work) {
      V.cmp_layout = volume_compare_layout(v.w, v.h, v.d);
      V.cmp_work = std::make_unique<DevBuf>(V.cmp_layout.bytes);
      V.cmp_ref = std::make_unique<DevBuf>(V.words * V.d * 8);
      check_hip(hipHostMalloc((void**)&V.h_cmp_ref, std::max<size_t>(V.words * V.d * 8, 16), hipHostMallocDefault),
                "hipHostMalloc compare reference");
      check_hip(hipHostMalloc((void**)&V.h_compare, sizeof(VolumeCompare), hipHostMallocDefault), "hipHostMalloc compare");
      check_hip(hipEventCreate(&V.cmp_e0), "event");
      check_hip(hipEventCreate(&V.cmp_e1), "event");
    }
    // The reference's words into the pinned staging (the stream is idle: the previous run ended with a sync).
    const VolumeReference& ref = *p.compare;
    const size_t nw = V.words * (size_t)V.d;
    if (ref.bits) {
      std::memcpy(V.h_cmp_ref, ref.bits, nw * 8);
    } else {
      std::memset(V.h_cmp_ref, 0, nw * 8);
      for (int z = 0; z < v.d; ++z)
        for (int y = 0; y < v.h; ++y) {
          const uint8_t* src = ref.mask + ((size_t)z * v.h + y) * v.w;
          uint64_t* row = V.h_cmp_ref + (size_t)z * V.words + (size_t)y * V.wpr;
          int x = 0;
          for (; x + 8 <= v.w; x += 8) {  // eight voxels at a time: most of a mask is empty
            uint64_t eight;
            std::memcpy(&eight, src + x, 8);
            if (!eight) continue;
            for (int b = 0; b < 8; ++b)
              if (src[x + b]) row[(x + b) >> 6] |= 1ull << ((x + b) & 63);
          }
          for (; x < v.w; ++x)
            if (src[x]) row[x >> 6] |= 1ull << (x & 63);
        }
    }
  }
  if (p.compare_lesions) {  // K18 alike; the record is sized for the largest N, the work buffer does not depend on N
    if (!I.compare_lesions_loaded) {
      preload_volume_compare_lesions();
      I.compare_lesions_loaded = true;
    }
    if (!V.cl_work) {
      V.cl_work = std::make_unique<DevBuf>(volume_compare_lesions_work_bytes(v.w, v.h, v.d, kMaxVolumeLesions));
      check_hip(hipHostMalloc((void**)&V.h_cl_record, kVolumeCompareLesionsMaxRecordBytes, hipHostMallocDefault),
                "hipHostMalloc lesion comparison");
      check_hip(hipEventCreate(&V.cl_e0), "event");
      check_hip(hipEventCreate(&V.cl_e1), "event");
    }
  }
  const PipeConsts pc = make_consts(p.pipe, 2);
  check_hip(hipEventRecord(I.e0, V.stream), "event");
  VolumeResult r;
  r.w = v.w;
  r.h = v.h;
  r.d = v.d;
  volume_preprocess(V, v, p.pipe, pc);
  volume_segment(V, v, p);
  check_hip(hipEventRecord(I.e1, V.stream), "event");
  if (p.measure) {  // timed outside the e0–e1 pair: kernels_s stays what it is
    VolumeLesionWork lw;
    if (p.measure_lesions) {
      lw.max_lesions = p.measure_lesions;
      lw.work = V.vl_work->p;
      lw.out = V.h_lesions;
      lw.out_count = reinterpret_cast<uint32_t*>(V.h_lesions + kMaxVolumeLesions);
    }
    VolumeDiametersWork dw;
    if (p.measure_diameters) {  // K13's seven launches directly after K10's
      dw.work = V.vd_work->p;
      dw.out = V.h_diameters;
      for (int a = 0; a < 3; ++a) dw.spacing_um[a] = p.spacing_um[a];
      dw.brute_force = p.diameters_brute_force;
      lw.diameters = &dw;
    }
    launch_volume_measure(V.dil.as<uint64_t>(), V.region.as<uint64_t>(), V.raw.as<uint16_t>(), V.ps, v.w, v.h, v.d,
                          (uint8_t)v.type, (uint8_t)v.stored_bits, p.measure_connectivity, V.vm_scratch->as<uint32_t>(),
                          V.vm_acc->as<uint64_t>(), V.h_measure, V.stream, p.measure_lesions ? &lw : nullptr);
    if (p.measure_intensity)  // K11's five launches after K8's last one
      launch_volume_intensity(V.dil.as<uint64_t>(), V.raw.as<uint16_t>(), V.ps, v.w, v.h, v.d, (uint8_t)v.type,
                              (uint8_t)v.stored_bits, V.vi_acc->p, V.h_intensity, V.stream);
    if (p.measure_texture)  // K12's four launches after K11's
      launch_volume_texture(V.dil.as<uint64_t>(), V.raw.as<uint16_t>(), V.ps, v.w, v.h, v.d, (uint8_t)v.type,
                            (uint8_t)v.stored_bits, p.texture_levels, V.vt_acc->p, V.h_texture, V.stream);
    if (p.measure_thickness)  // K16's four launches after K12's; its scratch is its own
      launch_volume_thickness(V.dil.as<uint64_t>(), V.dist_layout, p.spacing_um, V.dist_work->p, V.h_thickness, V.stream);
    check_hip(hipEventRecord(I.e2, V.stream), "event");
    check_hip(hipEventSynchronize(I.e2), "sync");
    r.measure = *V.h_measure;
    if (p.measure_intensity) r.intensity = *V.h_intensity;
    if (p.measure_thickness) r.thickness = *V.h_thickness;
    if (p.measure_texture) {
      r.texture = measure::glcm_from_record(V.h_texture);
      measure::check_glcm_exact(r.texture.head.samples);  // a cell may have wrapped: no result, as on the CPU
    }
    if (p.measure_lesions) {
      const uint32_t count = *lw.out_count;
      if (count > (uint32_t)p.measure_lesions) throw DeviceError("volume lesions: count out of range");
      r.lesions.assign(V.h_lesions, V.h_lesions + count);
      if (p.measure_diameters) r.diameters.assign(V.h_diameters, V.h_diameters + count);
    }
    float mms = 0;
    (void)hipEventElapsedTime(&mms, I.e1, I.e2);
    r.measure_s = mms * 1e-3;
  }
  if (p.compare) {  // K17's twenty launches after every measure launch, timed on their own
    check_hip(hipEventRecord(V.cmp_e0, V.stream), "event");
    check_hip(hipMemcpyAsync(V.cmp_ref->p, V.h_cmp_ref, V.words * (size_t)V.d * 8, hipMemcpyHostToDevice, V.stream), "H2D reference");
    launch_volume_compare(V.dil.as<uint64_t>(), V.cmp_ref->as<uint64_t>(), V.cmp_layout, p.spacing_um, V.cmp_work->p, V.h_compare,
                          V.stream);
    check_hip(hipEventRecord(V.cmp_e1, V.stream), "event");
    check_hip(hipEventSynchronize(V.cmp_e1), "sync");
    r.compare = *V.h_compare;
    float cms = 0;
    (void)hipEventElapsedTime(&cms, V.cmp_e0, V.cmp_e1);
    r.compare_s = cms * 1e-3;
  }
  if (p.compare_lesions) {  // K18's ten launches after K17's, on the masks K17 has on the device, timed on their own
    check_hip(hipEventRecord(V.cl_e0, V.stream), "event");
    launch_volume_compare_lesions(V.dil.as<uint64_t>(), V.cmp_ref->as<uint64_t>(), v.w, v.h, v.d, p.compare_lesions, p.measure_connectivity,
                                  V.cl_work->p, V.h_cl_record, V.stream);
    check_hip(hipEventRecord(V.cl_e1, V.stream), "event");
    check_hip(hipEventSynchronize(V.cl_e1), "sync");
    r.compare_lesions = measure::unpack_compare_lesions(V.h_cl_record, p.compare_lesions);
    float lms = 0;
    (void)hipEventElapsedTime(&lms, V.cl_e0, V.cl_e1);
    r.compare_lesions_s = lms * 1e-3;
  }
  check_hip(hipEventSynchronize(I.e1), "sync");
  r.sweeps = srg_volume_result(V.h_flag);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I.e0, I.e1);
  r.kernels_s = ms * 1e-3;
  if (want_masks) {
    unpack_volume(V.band, V, r.band);
    unpack_volume(V.region, V, r.region);
    unpack_volume(V.dil, V, r.dilated);
  }
  return r;
}

namespace {

// GPU backend of the z-slab decomposition: the slab's planes on the device (VolumeDevice); plane
// reads/writes are small synchronous copies (a boundary plane is 8 KiB for 256²).
class GpuSlabGrower final : public SlabGrower {
 public:
  GpuSlabGrower(VolumeDevice& V, int nseeds, int connectivity) : V_(V), nseeds_(nseeds), conn_(connectivity) {}
  int grow(bool first) override {
    srg_volume(V_.band.as<uint64_t>(), V_.region.as<uint64_t>(), V_.w, V_.h, V_.d, V_.seeds.as<int32_t>(),
               first ? nseeds_ : 0, conn_, V_.flag.as<uint32_t>(), V_.h_flag, V_.srg_scratch.as<uint64_t>(), V_.stream,
               first);
    check_hip(hipStreamSynchronize(V_.stream), "slab grow");
    return srg_volume_result(V_.h_flag);
  }
  std::vector<uint64_t> band_plane(int zl) override { return plane(V_.band, zl); }
  std::vector<uint64_t> region_plane(int zl) override { return plane(V_.region, zl); }
  void or_region_plane(int zl, const std::vector<uint64_t>& bits) override {
    std::vector<uint64_t> cur = plane(V_.region, zl);
    for (size_t i = 0; i < cur.size(); ++i) cur[i] |= bits[i];
    check_hip(hipMemcpy(V_.region.as<uint64_t>() + (size_t)zl * V_.words, cur.data(), V_.words * 8,
                        hipMemcpyHostToDevice),
              "H2D slab plane");
  }
  void dilate(int size, const std::vector<std::vector<uint64_t>>& below,
              const std::vector<std::vector<uint64_t>>& above) override {
    const int nb = (int)below.size(), na = (int)above.size(), de = nb + V_.d + na;
    const size_t wds = V_.words;
    DevBuf ext(wds * de * 8), dil(wds * de * 8), tmp(wds * de * 8), scr(8 * morph3d_scratch_words(V_.w, V_.h, de));
    for (int k = 0; k < nb; ++k)
      check_hip(hipMemcpy(ext.as<uint64_t>() + (size_t)k * wds, below[(size_t)k].data(), wds * 8, hipMemcpyHostToDevice),
                "H2D halo");
    for (int k = 0; k < na; ++k)
      check_hip(hipMemcpy(ext.as<uint64_t>() + (size_t)(nb + V_.d + k) * wds, above[(size_t)k].data(), wds * 8,
                          hipMemcpyHostToDevice),
                "H2D halo");
    check_hip(hipMemcpyAsync(ext.as<uint64_t>() + (size_t)nb * wds, V_.region.p, wds * V_.d * 8, hipMemcpyDeviceToDevice,
                             V_.stream),
              "D2D slab region");
    dilate_volume(ext.as<uint64_t>(), dil.as<uint64_t>(), tmp.as<uint64_t>(), V_.w, V_.h, de, size, V_.stream,
                  scr.as<uint64_t>(), ball);
    check_hip(hipMemcpyAsync(V_.dil.p, dil.as<uint64_t>() + (size_t)nb * wds, wds * V_.d * 8, hipMemcpyDeviceToDevice,
                             V_.stream),
              "D2D slab dilation");
    check_hip(hipStreamSynchronize(V_.stream), "slab dilation");
  }

 private:
  std::vector<uint64_t> plane(const DevBuf& b, int zl) {
    std::vector<uint64_t> v(V_.words);
    check_hip(hipMemcpy(v.data(), b.as<uint64_t>() + (size_t)zl * V_.words, V_.words * 8, hipMemcpyDeviceToHost),
              "D2H slab plane");
    return v;
  }
  VolumeDevice& V_;
  int nseeds_, conn_;
};

}  // namespace

// Device-resident z-slab growth and dilation (volume_slabs.h steps 2 and 3 on the GPU): the slab's
// boundary region planes go from V.region straight into the neighbours' device buffers
// (Comm::sendrecv_device — RCCL over xGMI, or staged through pinned memory by the host comms), the
// boundary seeding is a kernel, and the added-voxel count is all-reduced from device memory: one
// host synchronisation per round, no pageable copies. The dilation halo is received straight into
// the extended buffer around a device copy of the slab. Slabs thinner than the halo fall back to the
// generic algorithm (grow_and_dilate_slabs with GpuSlabGrower).
static SlabStats slab_grow_dilate_gpu(Comm& comm, VolumeDevice& V, int nseeds, int conn, int depth, int z0, int z1,
                                      int dilation, bool ball) {
  const int rank = comm.rank(), n = comm.size();
  const int d = z1 - z0, r = dilation / 2;
  const size_t pw = V.words, pbytes = pw * 8;
  const int below = rank > 0 ? rank - 1 : -1, above = rank + 1 < n ? rank + 1 : -1;
  SlabStats st;
  if (!V.slab_nb) {
    V.slab_nb = std::make_unique<DevBuf>(2 * pbytes);
    V.slab_added = std::make_unique<DevBuf>(8);
  }
  uint64_t* nb_below = V.slab_nb->as<uint64_t>();
  uint64_t* nb_above = nb_below + pw;
  auto* added = V.slab_added->as<int64_t>();
  uint64_t* band = V.band.as<uint64_t>();
  uint64_t* region = V.region.as<uint64_t>();
  for (bool first = true;; first = false) {
    srg_volume(band, region, V.w, V.h, d, V.seeds.as<int32_t>(), first ? nseeds : 0, conn, V.flag.as<uint32_t>(),
               V.h_flag, V.srg_scratch.as<uint64_t>(), V.stream, first);
    // My top plane goes up while the plane below my slab comes up from rank − 1; then the reverse.
    comm.sendrecv_device(region + (size_t)(d - 1) * pw, pbytes, above, nb_below, pbytes, below, V.stream);
    comm.sendrecv_device(region, pbytes, below, nb_above, pbytes, above, V.stream);
    st.exchanged_bytes += (int64_t)((above >= 0) + (below >= 0)) * (int64_t)pbytes;
    check_hip(hipMemsetAsync(added, 0, 8, V.stream), "memset added");
    auto* acc = reinterpret_cast<unsigned long long*>(added);
    if (below >= 0) launch_slab_seed(band, region, nb_below, V.w, V.h, conn == 26, acc, V.stream);
    if (above >= 0)
      launch_slab_seed(band + (size_t)(d - 1) * pw, region + (size_t)(d - 1) * pw, nb_above, V.w, V.h, conn == 26, acc,
                       V.stream);
    const int64_t total = comm.allreduce_sum_i64_device(added, V.stream);  // waits for the round
    st.sweeps += srg_volume_result(V.h_flag);
    ++st.rounds;
    if (total == 0) break;
  }
  const int rb = std::min(r, z0), ra = std::min(r, depth - z1), de = rb + d + ra;
  if (!V.ext || V.ext_planes < de) {
    const size_t bytes = pbytes * (size_t)de;
    V.ext = std::make_unique<DevBuf>(bytes);
    V.ext_dil = std::make_unique<DevBuf>(bytes);
    V.ext_tmp = std::make_unique<DevBuf>(bytes);
    V.ext_scr = std::make_unique<DevBuf>(8 * std::max<size_t>(1, morph3d_scratch_words(V.w, V.h, de)));
    V.ext_planes = de;
  }
  uint64_t* ext = V.ext->as<uint64_t>();
  if (r > 0) {
    // Top r planes up into the successor's lower halo; bottom r planes down into the predecessor's
    // upper halo (every slab holds ≥ r planes here).
    comm.sendrecv_device(region + (size_t)(d - r) * pw, above >= 0 ? (size_t)r * pbytes : 0, above, ext,
                         (size_t)rb * pbytes, below, V.stream);
    comm.sendrecv_device(region, below >= 0 ? (size_t)r * pbytes : 0, below, ext + (size_t)(rb + d) * pw,
                         (size_t)ra * pbytes, above, V.stream);
    st.exchanged_bytes += (int64_t)((above >= 0) + (below >= 0)) * r * (int64_t)pbytes;
  }
  check_hip(hipMemcpyAsync(ext + (size_t)rb * pw, region, pbytes * d, hipMemcpyDeviceToDevice, V.stream), "D2D slab");
  dilate_volume(ext, V.ext_dil->as<uint64_t>(), V.ext_tmp->as<uint64_t>(), V.w, V.h, de, dilation, V.stream,
                V.ext_scr->as<uint64_t>(), ball);
  check_hip(hipMemcpyAsync(V.dil.p, V.ext_dil->as<uint64_t>() + (size_t)rb * pw, pbytes * d, hipMemcpyDeviceToDevice,
                           V.stream),
            "D2D slab dilation");
  return st;
}

VolumeResult VolumeRunner::run_slab(Comm& comm, const VolumeInput& slab, int z0, int depth, const VolumeParams& p,
                                    bool want_masks, SlabStats* stats) {
  if (slab.d < 1 || slab.w < 1 || slab.h < 1) throw SliceError("empty slab");
  if (p.dilate_um >= 0 || p.measure_thickness)
    throw std::invalid_argument("run_slab: a margin in millimetres and the thickness are not supported on a volume split "
                                "into slabs (a margin across slabs needs a halo of its reach)");
  if (p.compare)
    throw std::invalid_argument("run_slab: comparing a volume split into slabs with a reference is not supported "
                                "(the surface distances of a slab are not those of the volume)");
  if (p.compare_lesions)
    throw std::invalid_argument("run_slab: the lesion-wise comparison of a volume split into slabs is not supported "
                                "(lesions that cross slabs need a collective)");
  if (p.measure || p.measure_lesions || p.measure_diameters || p.measure_intensity || p.measure_texture)
    throw std::invalid_argument("run_slab: measuring a volume split into slabs is not supported "
                                "(components that cross slabs need a collective)");
  check_volume_params(p.connectivity, p.dilation_size);
  Impl& I = *impl_;
  check_hip(hipSetDevice(I.device), "hipSetDevice");
  I.slab_volume = true;
  if (!I.V || I.V->w != slab.w || I.V->h != slab.h || I.V->d != slab.d) {
    I.M.reset();
    I.W.reset();
    I.X.reset();
    I.V.reset();
    I.V = std::make_unique<VolumeDevice>(slab);
  }
  VolumeDevice& V = *I.V;
  const PipeConsts pc = make_consts(p.pipe, 2);
  check_hip(hipEventRecord(I.e0, V.stream), "event");
  volume_preprocess(V, slab, p.pipe, pc);
  // Seeds in volume coordinates → this slab's (the rest belong to other ranks).
  std::vector<int32_t> sx;
  for (const Seed& s : slab_seeds(p.seeds, slab.w, slab.h, depth, z0, slab.d))
    if (sx.size() / 3 < (size_t)kMaxSeeds) {
      sx.push_back(s.x);
      sx.push_back(s.y);
      sx.push_back(s.z);
    }
  if (!sx.empty())
    check_hip(hipMemcpyAsync(V.seeds.p, sx.data(), sx.size() * 4, hipMemcpyHostToDevice, V.stream), "H2D seeds");
  const int conn = p.connectivity;
  if (depth < comm.size())
    throw std::runtime_error("z-slabs: volume depth " + std::to_string(depth) + " < " + std::to_string(comm.size()) +
                             " ranks leaves empty slabs");
  SlabStats st;
  if (depth / comm.size() >= p.dilation_size / 2) {
    st = slab_grow_dilate_gpu(comm, V, (int)(sx.size() / 3), conn, depth, z0, z0 + slab.d, p.dilation_size,
                              p.pipe.se_shape == kSeDisc);
  } else {  // slabs thinner than the dilation halo: the generic exchange (all-gather of slab ends)
    GpuSlabGrower g(V, (int)(sx.size() / 3), conn);
    g.ball = p.pipe.se_shape == kSeDisc;
    st = grow_and_dilate_slabs(comm, g, slab.w, slab.h, depth, z0, z0 + slab.d, conn, p.dilation_size);
  }
  check_hip(hipEventRecord(I.e1, V.stream), "event");
  check_hip(hipEventSynchronize(I.e1), "sync");
  VolumeResult r;
  r.w = slab.w;
  r.h = slab.h;
  r.d = slab.d;
  r.sweeps = st.sweeps;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, I.e0, I.e1);
  r.kernels_s = ms * 1e-3;
  if (stats) *stats = st;
  if (want_masks) {
    unpack_volume(V.band, V, r.band);
    unpack_volume(V.region, V, r.region);
    unpack_volume(V.dil, V, r.dilated);
  }
  return r;
}

std::vector<std::vector<uint8_t>> VolumeRunner::export_jpegs(const VolumeInput& v, const VolumeParams& p,
                                                             const RenderParams& rp, VolumeExportStats* st) {
  Impl& I = *impl_;
  if (!I.V || I.V->w != v.w || I.V->h != v.h || I.V->d != v.d) throw DeviceError("export_jpegs: run() this volume first");
  check_hip(hipSetDevice(I.device), "hipSetDevice");
  VolumeDevice& V = *I.V;
  const int cw = rp.out_width, ch = rp.out_height;
  if (cw % 16 || ch % 16) throw DeviceError("canvas size must be a multiple of 16");
  if (!I.X || I.X->cw != cw || I.X->ch != ch) {
    I.X.reset();
    I.X = std::make_unique<ExportBufs>(cw, ch, V.words * V.d);
  }
  ExportBufs& X = *I.X;
  const double t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  // Label planes = the dilated mask, border planes right behind them in one bit buffer.
  uint64_t* bits = X.bits.as<uint64_t>();
  const size_t vol_words = V.words * V.d;
  check_hip(hipMemcpyAsync(bits, V.dil.p, vol_words * 8, hipMemcpyDeviceToDevice, V.stream), "D2D labels");
  border_volume(bits, bits + vol_words, v.w, v.h, v.d, rp.border_radius, V.stream, V.morph_scratch.as<uint64_t>());
  const jpeg::Tables tables = jpeg::make_tables(rp.jpeg_quality);
  const jpeg::Sampling samp = (jpeg::Sampling)rp.jpeg_sampling;
  const std::vector<uint8_t> header = jpeg::make_header(cw, ch, tables, samp);
  const RenderGeom g = make_render_geom(v.w, v.h, v.spacing_x, v.spacing_y, cw, ch);
  const uint8_t fill = opacity_u8(rp.label_opacity), bval = opacity_u8(rp.border_opacity);
  const size_t canvas_bytes = (size_t)cw * ch;
  std::vector<std::vector<uint8_t>> files((size_t)2 * v.d);
  for (int z0 = 0; z0 < v.d; z0 += kExportSlices) {
    const int nz = std::min(kExportSlices, v.d - z0), nc = 2 * nz;
    auto* rd = reinterpret_cast<RenderDesc*>(X.h_tables);
    auto* jd = reinterpret_cast<JpegDesc*>(X.h_tables + (size_t)X.cap * sizeof(RenderDesc));
    bool any_canvas = false;
    for (int k = 0; k < nc; ++k) {
      const int z = z0 + k / 2;
      RenderDesc& r = rd[k];
      std::memset(&r, 0, sizeof(r));
      r.kind = (k & 1) ? kRenderLabels : kRenderRawGray;
      r.filter = (uint8_t)(rp.filter == kFilterNearest ? 1 : 0);
      r.type = (uint8_t)v.type;
      r.stored_bits = (uint8_t)v.stored_bits;
      r.fill = fill;
      r.border_value = bval;
      r.slice = (uint32_t)z;  // the median kernel's per-plane stats
      r.src_w = (uint16_t)v.w;
      r.src_h = (uint16_t)v.h;
      r.wpr = (uint16_t)V.wpr;
      r.ox = g.ox;
      r.oy = g.oy;
      r.invx = g.invx;
      r.invy = g.invy;
      r.slope = p.pipe.apply_rescale ? v.slope : 1.f;
      r.intercept = p.pipe.apply_rescale ? v.intercept : 0.f;
      r.src_off = (k & 1) ? (uint32_t)(z * V.words) : (uint32_t)(z * V.ps);
      r.border_off = (uint32_t)(vol_words + z * V.words);
      r.canvas_off = (uint32_t)(k * canvas_bytes);
      JpegDesc& j = jd[k];
      std::memset(&j, 0, sizeof(j));
      j.canvas_off = (uint32_t)(k * canvas_bytes);
      j.out_off = (uint64_t)k * kVolOutCap;
      j.out_cap = kVolOutCap;
      j.render = render_is_exact_2x(r, cw, ch) && (r.kind == kRenderLabels || !r.filter || jpeg_fuses_nearest(samp)) ? k : -1;
      any_canvas |= j.render < 0;
    }
    auto* d_rd = X.tables.as<uint8_t>();
    auto* d_jd = d_rd + (size_t)X.cap * sizeof(RenderDesc);
    check_hip(hipMemcpyAsync(d_rd, X.h_tables, (size_t)X.cap * (sizeof(RenderDesc) + sizeof(JpegDesc)),
                             hipMemcpyHostToDevice, V.stream),
              "H2D export tables");
    const auto* drd = reinterpret_cast<const RenderDesc*>(d_rd);
    if (any_canvas)
      launch_render(V.raw.as<uint16_t>(), nullptr, bits, V.stats.as<SliceStats>(), drd, nc, cw, ch,
                    X.canvas.as<uint8_t>(), V.stream);
    JpegRenderSrc rs;
    rs.raw = V.raw.as<uint16_t>();
    rs.bits = bits;
    rs.stats = V.stats.as<SliceStats>();
    rs.rd = drd;
    rs.nrd = nc;
    launch_jpeg(X.canvas.as<uint8_t>(), reinterpret_cast<const JpegDesc*>(d_jd), nc, cw, ch, tables.div_luma, X.jw,
                X.d_out, X.d_sizes, V.stream, &rs, samp, rp.filter == kFilterNearest && jpeg_fuses_nearest(samp));
    check_hip(hipStreamSynchronize(V.stream), "export sync");
    bool rendered = any_canvas;
    for (int k = 0; k < nc; ++k) {
      std::vector<uint8_t>& f = files[(size_t)2 * z0 + k];
      f = header;
      if (X.h_sizes[k] >= 0) {
        f.insert(f.end(), X.h_out + (size_t)k * kVolOutCap, X.h_out + (size_t)k * kVolOutCap + X.h_sizes[k]);
      } else {  // capacity overflow: host encoder on the rendered canvas
        if (!rendered) {
          launch_render(V.raw.as<uint16_t>(), nullptr, bits, V.stats.as<SliceStats>(), drd, nc, cw, ch,
                        X.canvas.as<uint8_t>(), V.stream);
          check_hip(hipStreamSynchronize(V.stream), "fallback render");
          rendered = true;
        }
        std::vector<uint8_t> canvas(canvas_bytes);
        check_hip(hipMemcpy(canvas.data(), X.canvas.as<uint8_t>() + (size_t)k * canvas_bytes, canvas_bytes,
                            hipMemcpyDeviceToHost),
                  "canvas D2H");
        const auto scan = jpeg::encode_scan_gray(canvas.data(), cw, ch, cw, tables, samp);
        f.insert(f.end(), scan.begin(), scan.end());
        if (st) ++st->jpeg_fallbacks;
      }
      f.push_back(0xFF);
      f.push_back(0xD9);
    }
  }
  if (st)
    st->export_s += std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0;
  return files;
}

VolumeViewsExport VolumeRunner::export_views(const VolumeInput& v, const VolumeParams& p, const RenderParams& rp,
                                             const ViewsAt& at, bool want_planes, VolumeExportStats* st) {
  Impl& I = *impl_;
  if (!I.V || I.V->w != v.w || I.V->h != v.h || I.V->d != v.d) throw DeviceError("export_views: run() this volume first");
  const std::string at_err = views::at_error(at, v.w, v.h, v.d);
  if (!at_err.empty()) throw std::invalid_argument("--volume-views-at: " + at_err);
  check_hip(hipSetDevice(I.device), "hipSetDevice");
  VolumeDevice& V = *I.V;
  const int cw = rp.out_width, ch = rp.out_height;
  if (cw % 16 || ch % 16) throw DeviceError("canvas size must be a multiple of 16");
  if (!I.X || I.X->cw != cw || I.X->ch != ch) {
    I.X.reset();
    I.X = std::make_unique<ExportBufs>(cw, ch, V.words * V.d);
  }
  ExportBufs& X = *I.X;
  // First use: K14's code object while the stream is idle (run() and export_jpegs() end with a
  // synchronisation), then its buffers.
  if (!I.views_loaded) {
    preload_volume_views();
    I.views_loaded = true;
  }
  if (!I.W) I.W = std::make_unique<ViewBufs>(volume_views_layout(v.w, v.h, v.d));
  ViewBufs& W = *I.W;
  const VolumeViewsLayout& L = W.L;
  const double t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  const float slope = p.pipe.apply_rescale ? v.slope : 1.f, intercept = p.pipe.apply_rescale ? v.intercept : 0.f;
  const bool inverted = slope < 0.f;
  auto* head = W.head.as<VolumeViewsHead>();
  uint64_t* bits = W.bits.as<uint64_t>();
  check_hip(hipEventRecord(W.e0, V.stream), "event");
  launch_volume_views(V.raw.as<uint16_t>(), V.ps, V.dil.as<uint64_t>(), (uint8_t)v.type, (uint8_t)v.stored_bits, inverted, at, L,
                      W.samples.as<uint16_t>(), bits, W.proj.as<uint32_t>(), head, V.stream);
  check_hip(hipEventRecord(W.e1, V.stream), "event");
  // The renderer border in each view's own image: views of one size are neighbours, a two-plane volume.
  for (int i = 0; i < 3; ++i)
    border_volume(bits + L.mask_off[i], bits + L.border_off + L.mask_off[i], L.vw[i], L.vh[i], 2, rp.border_radius, V.stream,
                  W.scratch.as<uint64_t>());
  const jpeg::Tables tables = jpeg::make_tables(rp.jpeg_quality);
  const jpeg::Sampling samp = (jpeg::Sampling)rp.jpeg_sampling;
  const std::vector<uint8_t> header = jpeg::make_header(cw, ch, tables, samp);
  const uint8_t fill = opacity_u8(rp.label_opacity), bval = opacity_u8(rp.border_opacity);
  const size_t canvas_bytes = (size_t)cw * ch;
  const int nc = 2 * kVolumeViewCount;
  auto* rd = reinterpret_cast<RenderDesc*>(X.h_tables);
  auto* jd = reinterpret_cast<JpegDesc*>(X.h_tables + (size_t)X.cap * sizeof(RenderDesc));
  bool any_canvas = false;
  for (int k = 0; k < nc; ++k) {
    const int i = k / 2;
    float su = 1.f, sv = 1.f;
    views::view_spacing(i, v.spacing_x, v.spacing_y, v.spacing_z, &su, &sv);
    const RenderGeom g = make_render_geom(L.vw[i], L.vh[i], su, sv, cw, ch);
    RenderDesc& r = rd[k];
    std::memset(&r, 0, sizeof(r));
    r.kind = (k & 1) ? kRenderLabels : kRenderRawGray;
    r.filter = (uint8_t)(rp.filter == kFilterNearest ? 1 : 0);
    r.type = (uint8_t)v.type;
    r.stored_bits = (uint8_t)v.stored_bits;
    r.fill = fill;
    r.border_value = bval;
    r.slice = (uint32_t)i;  // the view's own key min / max
    r.src_w = (uint16_t)L.vw[i];
    r.src_h = (uint16_t)L.vh[i];
    r.wpr = (uint16_t)L.wpr[i];
    r.ox = g.ox;
    r.oy = g.oy;
    r.invx = g.invx;
    r.invy = g.invy;
    r.slope = slope;
    r.intercept = intercept;
    r.src_off = (k & 1) ? L.mask_off[i] : L.sample_off[i];
    r.border_off = L.border_off + L.mask_off[i];
    r.canvas_off = (uint32_t)(k * canvas_bytes);
    JpegDesc& j = jd[k];
    std::memset(&j, 0, sizeof(j));
    j.canvas_off = (uint32_t)(k * canvas_bytes);
    j.out_off = (uint64_t)k * kVolOutCap;
    j.out_cap = kVolOutCap;
    j.render = render_is_exact_2x(r, cw, ch) && (r.kind == kRenderLabels || !r.filter || jpeg_fuses_nearest(samp)) ? k : -1;
    any_canvas |= j.render < 0;
  }
  auto* d_rd = X.tables.as<uint8_t>();
  auto* d_jd = d_rd + (size_t)X.cap * sizeof(RenderDesc);
  check_hip(hipMemcpyAsync(d_rd, X.h_tables, (size_t)X.cap * (sizeof(RenderDesc) + sizeof(JpegDesc)), hipMemcpyHostToDevice,
                           V.stream),
            "H2D view tables");
  const auto* drd = reinterpret_cast<const RenderDesc*>(d_rd);
  const SliceStats* stats = head->stats;  // device address arithmetic only
  if (any_canvas)
    launch_render(W.samples.as<uint16_t>(), nullptr, bits, stats, drd, nc, cw, ch, X.canvas.as<uint8_t>(), V.stream);
  JpegRenderSrc rs;
  rs.raw = W.samples.as<uint16_t>();
  rs.bits = bits;
  rs.stats = stats;
  rs.rd = drd;
  rs.nrd = nc;
  launch_jpeg(X.canvas.as<uint8_t>(), reinterpret_cast<const JpegDesc*>(d_jd), nc, cw, ch, tables.div_luma, X.jw, X.d_out,
              X.d_sizes, V.stream, &rs, samp, rp.filter == kFilterNearest && jpeg_fuses_nearest(samp));
  // P, the box and the per-view integers come back once, with the JPEG sizes.
  check_hip(hipMemcpyAsync(W.h_head, head, sizeof(VolumeViewsHead), hipMemcpyDeviceToHost, V.stream), "D2H views head");
  check_hip(hipEventRecord(W.e2, V.stream), "event");
  check_hip(hipStreamSynchronize(V.stream), "views sync");
  VolumeViewsExport out;
  out.files.resize((size_t)nc);
  bool rendered = any_canvas;
  for (int k = 0; k < nc; ++k) {
    std::vector<uint8_t>& f = out.files[(size_t)k];
    f = header;
    if (X.h_sizes[k] >= 0) {
      f.insert(f.end(), X.h_out + (size_t)k * kVolOutCap, X.h_out + (size_t)k * kVolOutCap + X.h_sizes[k]);
    } else {  // capacity overflow: host encoder on the rendered canvas
      if (!rendered) {
        launch_render(W.samples.as<uint16_t>(), nullptr, bits, stats, drd, nc, cw, ch, X.canvas.as<uint8_t>(), V.stream);
        check_hip(hipStreamSynchronize(V.stream), "fallback render");
        rendered = true;
      }
      std::vector<uint8_t> canvas(canvas_bytes);
      check_hip(hipMemcpy(canvas.data(), X.canvas.as<uint8_t>() + (size_t)k * canvas_bytes, canvas_bytes, hipMemcpyDeviceToHost),
                "canvas D2H");
      const auto scan = jpeg::encode_scan_gray(canvas.data(), cw, ch, cw, tables, samp);
      f.insert(f.end(), scan.begin(), scan.end());
      if (st) ++st->jpeg_fallbacks;
    }
    f.push_back(0xFF);
    f.push_back(0xD9);
  }
  const VolumeViewsHead& hh = *W.h_head;
  VolumeViews& r = out.views;
  r.w = v.w, r.h = v.h, r.d = v.d;
  r.at_mode = at.mode;
  r.inverted = inverted;
  r.has_box = hh.has_box != 0;
  for (int a = 0; a < 3; ++a) r.at[a] = hh.at[a];
  for (int a = 0; a < 6; ++a) r.box[a] = hh.box[a];
  const uint8_t type = v.type == kU8 ? (uint8_t)kU16 : (uint8_t)v.type;
  for (int i = 0; i < kVolumeViewCount; ++i) {
    VolumeView& q = r.view[i];
    q.w = L.vw[i];
    q.h = L.vh[i];
    // the smallest and the largest stored sample: keys are in value order
    q.raw_min = (int32_t)raw_value_from_key((uint16_t)hh.stats[i].key_min, type);
    q.raw_max = (int32_t)raw_value_from_key((uint16_t)hh.stats[i].key_max, type);
    q.mask_px = hh.mask_px[i];
  }
  if (want_planes) {
    std::vector<uint16_t> hs(L.samples);
    std::vector<uint64_t> hb(L.border_off);
    check_hip(hipMemcpy(hs.data(), W.samples.p, hs.size() * 2, hipMemcpyDeviceToHost), "D2H view samples");
    check_hip(hipMemcpy(hb.data(), W.bits.p, hb.size() * 8, hipMemcpyDeviceToHost), "D2H view masks");
    for (int i = 0; i < kVolumeViewCount; ++i) {
      VolumeView& q = r.view[i];
      q.raw.assign(hs.begin() + L.sample_off[i], hs.begin() + L.sample_off[i] + (size_t)q.w * q.h);
      q.mask.assign((size_t)q.w * q.h, 0);
      for (int y = 0; y < q.h; ++y)
        for (int x = 0; x < q.w; ++x)
          q.mask[(size_t)y * q.w + x] = (hb[L.mask_off[i] + (size_t)y * L.wpr[i] + x / 64] >> (x % 64)) & 1;
    }
  }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, W.e0, W.e1);
  out.k14_s = ms * 1e-3;
  (void)hipEventElapsedTime(&ms, W.e1, W.e2);
  out.render_s = ms * 1e-3;
  if (st)
    st->export_s += std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0;
  return out;
}

VolumeMesh VolumeRunner::export_mesh(const VolumeInput& v, const VolumeParams& p, int placement, uint64_t max_bytes,
                                     int scan_block) {
  (void)p;
  Impl& I = *impl_;
  if (!I.V || I.V->w != v.w || I.V->h != v.h || I.V->d != v.d) throw DeviceError("export_mesh: run() this volume first");
  if (I.slab_volume) throw DeviceError("export_mesh: the volume on the device is a z-slab: a mesh crosses the slabs");
  if (placement != kMeshCorner && placement != kMeshNets) throw std::invalid_argument("export_mesh: placement must be corner or nets");
  check_hip(hipSetDevice(I.device), "hipSetDevice");
  VolumeDevice& V = *I.V;
  const VolumeMeshLayout L = volume_mesh_layout(v.w, v.h, v.d, scan_block);
  // First use: K15's code object while the stream is idle (run() ends with a synchronisation), then its buffers.
  if (!I.mesh_loaded) {
    preload_volume_mesh();
    I.mesh_loaded = true;
  }
  if (!I.M || I.M->L.scan_block != L.scan_block) {
    I.M.reset();
    I.M = std::make_unique<MeshBufs>(L);
  }
  MeshBufs& M = *I.M;
  const uint64_t* dil = V.dil.as<uint64_t>();
  check_hip(hipEventRecord(M.e0, V.stream), "event");
  launch_volume_mesh(dil, L, M.work.p, M.h_head, V.stream);
  check_hip(hipEventRecord(M.e1, V.stream), "event");
  check_hip(hipStreamSynchronize(V.stream), "mesh totals sync");
  const VolumeMeshHead hh = *M.h_head;
  const uint64_t nv = hh.total[0], nq = hh.total[1] + hh.total[2] + hh.total[3];
  const std::string err = mesh::size_error(nv, nq, max_bytes);
  if (!err.empty()) throw std::runtime_error("--volume-mesh: " + err);
  VolumeMesh m;
  m.w = v.w, m.h = v.h, m.d = v.d;
  m.placement = placement;
  m.quads_x = hh.total[1], m.quads_y = hh.total[2], m.quads_z = hh.total[3];
  m.voxels = hh.voxels;
  m.positions.resize(3 * (size_t)nv);
  m.quads.resize(4 * (size_t)nq);
  const size_t pos_bytes = (12 * (size_t)nv + 255) / 256 * 256, need = pos_bytes + 16 * (size_t)nq;
  if (!M.out || M.out_bytes < need) {
    M.out.reset();
    M.out = std::make_unique<DevBuf>(need);
    M.out_bytes = need;
  }
  float* d_pos = M.out->as<float>();
  uint32_t* d_quads = reinterpret_cast<uint32_t*>(M.out->as<uint8_t>() + pos_bytes);
  check_hip(hipEventRecord(M.e2, V.stream), "event");
  launch_volume_mesh_emit(dil, L, M.work.p, hh, placement, v.spacing_x, v.spacing_y, (float)v.spacing_z, d_pos, d_quads, V.stream);
  check_hip(hipEventRecord(M.e3, V.stream), "event");
  if (nv) check_hip(hipMemcpyAsync(m.positions.data(), d_pos, 12 * (size_t)nv, hipMemcpyDeviceToHost, V.stream), "D2H mesh positions");
  if (nq) check_hip(hipMemcpyAsync(m.quads.data(), d_quads, 16 * (size_t)nq, hipMemcpyDeviceToHost, V.stream), "D2H mesh quads");
  check_hip(hipStreamSynchronize(V.stream), "mesh sync");
  float a = 0, b = 0;
  (void)hipEventElapsedTime(&a, M.e0, M.e1);
  (void)hipEventElapsedTime(&b, M.e2, M.e3);
  m.k15_s = (double)(a + b) * 1e-3;
  return m;
}

VolumeResult run_volume(const VolumeInput& v, const VolumeParams& p, int device, bool want_masks) {
  VolumeRunner runner(device);
  return runner.run(v, p, want_masks);
}

namespace app {

namespace {

double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct VolPatient {
  std::string id, out_dir, series_dir, error;
  bool setup_ok = false, listed = false;
  std::vector<std::string> files;
};

struct VolOutcome {
  int32_t ok = 0;
  std::string message;
  int32_t sweeps = 0;
  double gpu_s = 0, export_s = 0, wall_s = 0;
  int64_t slices = 0, fallbacks = 0;
  int32_t rounds = 0;         // --split-volume: grow/exchange rounds
  int64_t exchanged = 0;      // --split-volume: boundary + halo bytes sent
  std::string measure_json;   // --measure-volume: the sidecar text (measure::volume_to_json)
  double measure_s = 0;       // --measure-volume: GPU time of K8
  int32_t view_files = 0;     // --volume-views: view files written (12, or 0)
  int32_t mesh_files = 0;     // --volume-mesh: files written (the mesh and mesh.json: 2, or 0)
  int64_t mesh_vertices = 0, mesh_quads = 0;
  int32_t mask_files = 0;      // --volume-mask: files written (mask.mhd and mask.raw: 2, or 0)
  std::string compare_status;  // --compare-to: "ok", "no_reference" or "shape_mismatch" (empty: the patient failed)
  std::string compare_fields;  // --compare-to: the patient's fields of comparisons.csv (compare::csv_fields)
  int32_t dice_ok = 0, distances_ok = 0;
  double dice = 0, hausdorff_mm = 0, compare_s = 0;
  std::string lesion_rows;  // --compare-lesions: the patient's rows of compare_lesions.csv (compare::lesions_table_rows)
  int32_t lesion_f1_ok = 0;
  double lesion_f1 = 0, compare_lesions_s = 0;
};

// --compare-to: the reference mask of a patient, DIR/<patient>/mask.mhd, as 0 / 1 bytes (non-zero = set, whatever
// the element type). `status`: "ok", "no_reference" (no such file) or "shape_mismatch".
std::vector<uint8_t> read_reference_mask(const std::string& path, int w, int h, int d, std::string* status) {
  {
    std::ifstream probe(path, std::ios::binary);
    if (!probe) {
      *status = "no_reference";
      return {};
    }
  }
  const mhd::Image im = mhd::read(path);
  if (im.w != w || im.h != h || im.d != d) {
    *status = "shape_mismatch";
    return {};
  }
  const size_t es = mhd::element_size(im.type), n = (size_t)w * h * d;
  if (im.bytes.size() != n * es) throw std::runtime_error("--compare-to: " + path + " holds " + std::to_string(im.bytes.size()) +
                                                           " bytes, expected " + std::to_string(n * es));
  std::vector<uint8_t> m(n, 0);
  for (size_t i = 0; i < n; ++i)
    for (size_t b = 0; b < es; ++b) m[i] |= im.bytes[i * es + b] != 0;
  *status = "ok";
  return m;
}

std::vector<uint8_t> encode(const std::vector<VolPatient>& pl) {
  ByteWriter w;
  w.u32((uint32_t)pl.size());
  for (const auto& p : pl) {
    w.str(p.id);
    w.str(p.out_dir);
    w.str(p.series_dir);
    w.str(p.error);
    w.u32(p.setup_ok);
    w.u32(p.listed);
    w.u32((uint32_t)p.files.size());
    for (const auto& f : p.files) w.str(f);
  }
  return w.b;
}

std::vector<VolPatient> decode(const std::vector<uint8_t>& b) {
  ByteReader r(b.data(), b.size());
  std::vector<VolPatient> pl(r.u32());
  for (auto& p : pl) {
    p.id = r.str();
    p.out_dir = r.str();
    p.series_dir = r.str();
    p.error = r.str();
    p.setup_ok = r.u32();
    p.listed = r.u32();
    p.files.resize(r.u32());
    for (auto& f : p.files) f = r.str();
  }
  return pl;
}

void write_file(const std::string& path, const std::vector<uint8_t>& jpg) {
  // complete JPEG file (header + scan + EOI): write_jpeg_file appends the EOI itself
  jpeg::write_jpeg_file(path, {}, jpg.data(), jpg.size() - 2);
}

// Any other file, as it is.
void write_bytes(const std::string& path, const void* data, size_t n) {
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  f.write(static_cast<const char*>(data), (std::streamsize)n);
  if (!f) throw std::runtime_error("Cannot write " + path);
}

// Golden 3D path (--cpu): per-plane preprocessing on a thread pool, 3D SRG + cube dilation, host
// render + encoder — the oracle the GPU 3D export is checked against.
struct GoldenPlanes {
  std::vector<uint8_t> band;               // 0/1 voxels of every plane
  std::vector<std::vector<float>> vals;    // rescaled values per plane (original render)
};

GoldenPlanes golden_preprocess(const VolumeInput& v, const VolumeParams& vp) {
  const size_t plane = (size_t)v.w * v.h;
  GoldenPlanes g;
  g.band.assign(plane * v.d, 0);
  g.vals.resize((size_t)v.d);
  ThreadPool pool(16);
  TaskGroup tg(pool);
  for (int z = 0; z < v.d; ++z)
    tg.run([&, z] {
      golden::SliceInput si;
      si.w = v.w;
      si.h = v.h;
      si.type = v.type;
      si.stored_bits = v.stored_bits;
      si.slope = v.slope;
      si.intercept = v.intercept;
      si.spacing_x = v.spacing_x;
      si.spacing_y = v.spacing_y;
      si.raw.assign(v.raw.begin() + z * plane, v.raw.begin() + (z + 1) * plane);
      golden::SliceResult r = golden::run(si, vp.pipe, false);
      std::copy(r.band.begin(), r.band.end(), g.band.begin() + z * plane);
      g.vals[z] = golden::rescaled(si, vp.pipe);
    });
  tg.wait();
  return g;
}

// The 2·d files (original, processed per plane) of the dilated mask `dil` of volume `v`.
std::vector<std::vector<uint8_t>> golden_export(const VolumeInput& v, const std::vector<std::vector<float>>& vals,
                                                const std::vector<uint8_t>& dil, const RenderParams& rp) {
  const size_t plane = (size_t)v.w * v.h;
  const RenderGeom g = make_render_geom(v.w, v.h, v.spacing_x, v.spacing_y, rp.out_width, rp.out_height);
  std::vector<std::vector<uint8_t>> files((size_t)2 * v.d);
  for (int z = 0; z < v.d; ++z) {
    const auto mm = std::minmax_element(vals[z].begin(), vals[z].end());
    std::vector<uint8_t> lab(dil.begin() + z * plane, dil.begin() + (z + 1) * plane);
    const auto c0 = golden::render_gray(vals[z], g, *mm.first, *mm.second, rp.filter == kFilterNearest);
    const auto c1 = golden::render_labels(lab, golden::border(lab, v.w, v.h, rp.border_radius), g,
                                          opacity_u8(rp.label_opacity), opacity_u8(rp.border_opacity));
    files[2 * z] = jpeg::encode_gray(c0.data(), rp.out_width, rp.out_height, rp.out_width, rp.jpeg_quality,
                                     (jpeg::Sampling)rp.jpeg_sampling);
    files[2 * z + 1] = jpeg::encode_gray(c1.data(), rp.out_width, rp.out_height, rp.out_width, rp.jpeg_quality,
                                     (jpeg::Sampling)rp.jpeg_sampling);
  }
  return files;
}

// `measured` (optional): the record of the dilated volume by the golden model (--measure-volume), and
// with vp.measure_lesions the lesion records in `lesions`.
std::vector<std::vector<uint8_t>> golden_volume_jpegs(const VolumeInput& v, const VolumeParams& vp,
                                                      const RenderParams& rp, VolumeMeasure* measured = nullptr,
                                                      std::vector<VolumeLesion>* lesions = nullptr,
                                                      IntensityStats* intensity = nullptr,
                                                      measure::Glcm* texture = nullptr,
                                                      std::vector<VolumeLesionDiameters>* diameters = nullptr,
                                                      const ViewsAt* views_at = nullptr, VolumeViewsExport* views = nullptr,
                                                      VolumeMesh* mesh_out = nullptr, int mesh_placement = kMeshCorner,
                                                      VolumeThickness* thickness = nullptr,
                                                      std::vector<uint8_t>* dilated_out = nullptr,
                                                      VolumeCompare* compared = nullptr,
                                                      VolumeCompareLesions* compared_lesions = nullptr) {
  const GoldenPlanes gp = golden_preprocess(v, vp);
  std::vector<Seed> seeds = vp.seeds;
  if (seeds.empty()) {
    seeds = reference_seeds(v.w, v.h);
    for (auto& sd : seeds) sd.z = v.d / 2;
  }
  const auto region = golden::region_grow3d(gp.band, v.w, v.h, v.d, seeds, vp.connectivity);
  const auto dil = vp.dilate_um >= 0 ? golden::dilate3d_mm(region, v.w, v.h, v.d, vp.spacing_um, vp.dilate_um)
                                      : golden::dilate3d(region, v.w, v.h, v.d, vp.dilation_size, vp.pipe.se_shape == kSeDisc);
  if (measured && thickness && vp.measure_thickness) *thickness = golden::volume_thickness(dil, v.w, v.h, v.d, vp.spacing_um);
  if (measured) *measured = golden::measure_volume(dil, region, v, vp.measure_connectivity);
  if (measured && lesions && vp.measure_lesions)
    *lesions = golden::measure_volume_lesions(dil, v, vp.measure_connectivity, vp.measure_lesions);
  if (measured && diameters && vp.measure_lesions && vp.measure_diameters)
    *diameters = golden::measure_volume_diameters(dil, v.w, v.h, v.d, vp.measure_connectivity, vp.measure_lesions, vp.spacing_um);
  if (measured && intensity && vp.measure_intensity) *intensity = golden::measure_intensity(dil, v);
  if (measured && texture && vp.measure_texture) *texture = golden::measure_texture(dil, v, vp.texture_levels);
  if (views_at && views) {  // --volume-views: the golden views and their files (nm03/volume_views.h)
    // The projections are taken on keys; the maximum of the rescaled floats in gp.vals would render the
    // same pixels, since the rescale is monotone (tests/test_volume_views.py checks both slope signs).
    const float slope = vp.pipe.apply_rescale ? v.slope : 1.f, intercept = vp.pipe.apply_rescale ? v.intercept : 0.f;
    views->views = golden::volume_views(v.raw.data(), dil.data(), v.w, v.h, v.d, (uint8_t)v.type, v.stored_bits, slope < 0.f,
                                        *views_at);
    views->files = golden::volume_view_jpegs(views->views, (uint8_t)v.type, v.stored_bits, slope, intercept, v.spacing_x,
                                             v.spacing_y, v.spacing_z, rp);
  }
  if (compared && vp.compare) {  // --compare-to: the golden comparison with the reference's bytes (nm03/volume_compare.h)
    const std::vector<uint8_t> ref(vp.compare->mask, vp.compare->mask + (size_t)v.w * v.h * v.d);
    *compared = golden::compare_volumes(dil, ref, v.w, v.h, v.d, vp.spacing_um);
    if (compared_lesions && vp.compare_lesions)  // --compare-lesions: the golden lesion-wise comparison of the same masks
      *compared_lesions = golden::compare_volume_lesions(dil, ref, v.w, v.h, v.d, vp.compare_lesions, vp.measure_connectivity);
  }
  if (dilated_out) *dilated_out = dil;
  if (mesh_out)  // --volume-mesh: the golden mesh of the dilated mask (nm03/volume_mesh.h)
    *mesh_out = golden::volume_mesh(dil.data(), v.w, v.h, v.d, v.spacing_x, v.spacing_y, v.spacing_z, mesh_placement);
  return golden_export(v, gp.vals, dil, rp);
}

// One rank's z-slab of a volume on the golden model (--cpu --split-volume): the same
// decomposition and exchanges as the GPU slab path (volume_slabs.h), host arithmetic.
std::vector<std::vector<uint8_t>> golden_slab_jpegs(Comm& comm, const VolumeInput& slab, int z0, int depth,
                                                    const VolumeParams& vp, const RenderParams& rp, SlabStats* st) {
  GoldenPlanes gp = golden_preprocess(slab, vp);
  GoldenSlabGrower g(std::move(gp.band), slab.w, slab.h, slab.d, slab_seeds(vp.seeds, slab.w, slab.h, depth, z0, slab.d),
                     vp.connectivity);
  g.ball = vp.pipe.se_shape == kSeDisc;
  *st = grow_and_dilate_slabs(comm, g, slab.w, slab.h, depth, z0, z0 + slab.d, vp.connectivity, vp.dilation_size);
  return golden_export(slab, gp.vals, g.dilated(), rp);
}

int volume_rank(const AppConfig& cfg, int rank, int size, Comm& comm, int device) {
  const std::string base = cohort::cohort_dir(cfg.data_root);
  VolumeParams vp;
  vp.pipe = cfg.engine.pipe;
  // --srg-connectivity defaults to the 2D value 4, which stands for 6 here (run_volume_cohort
  // rejected everything but 4, 6 and 26).
  vp.connectivity = cfg.engine.pipe.srg_connectivity == 26 ? 26 : 6;
  // BASELINE config 5: 7×7×7 cube dilation unless --dilation-size was given.
  vp.dilation_size = cfg.dilation_set ? cfg.engine.pipe.dilation_size : 7;
  vp.measure = cfg.measure_volume;
  vp.measure_connectivity = cfg.measure_volume_connectivity;
  vp.measure_lesions = cfg.measure_volume_lesions;
  vp.measure_diameters = cfg.measure_volume_diameters;
  vp.measure_intensity = cfg.measure_volume_intensity;
  vp.measure_texture = cfg.measure_volume_texture;
  vp.texture_levels = cfg.engine.pipe.texture_levels;
  vp.dilate_um = cfg.dilate_um;
  vp.measure_thickness = cfg.measure_volume_thickness;
  const RenderParams& rp = cfg.engine.render;
  const double t_start = wall_now();
  // ---- plan on rank 0 -----------------------------------------------------------------------
  std::vector<uint8_t> plan_bytes;
  int64_t fatal = 0;
  std::string fatal_msg;
  if (rank == 0) {
    std::cout << "\n=== Starting 3D Volume Processing for All Patients ===\n" << std::endl;
    try {
      std::vector<VolPatient> plan;
      std::vector<std::string> pids = cohort::find_patient_dirs(base);
      std::cout << "Found " << pids.size() << " patient directories." << std::endl;
      for (const auto& pid : pids) {
        VolPatient p;
        p.id = pid;
        p.out_dir = cfg.out_dir + "/" + pid;
        try {
          cohort::setup_output_dir(p.out_dir);
          p.setup_ok = true;
          cohort::Series s = cohort::list_patient_series(base, pid);
          p.series_dir = s.series_dir;
          p.files = std::move(s.files);
          p.listed = true;
        } catch (const std::exception& e) {
          p.error = e.what();
        }
        plan.push_back(std::move(p));
      }
      plan_bytes = encode(plan);
    } catch (const std::exception& e) {
      fatal = 1;
      fatal_msg = e.what();
    }
  }
  comm.allreduce_sum_i64(&fatal, 1);
  if (fatal) {
    if (rank == 0) std::cerr << "Error finding patient directories: " << fatal_msg << std::endl;
    return 1;
  }
  comm.broadcast_bytes(plan_bytes, 0);
  const std::vector<VolPatient> plan = decode(plan_bytes);
  // ---- this rank's patients (contiguous blocks; one volume per patient) ----------------------
  const size_t lo = plan.size() * rank / size, hi = plan.size() * (rank + 1) / size;
  std::unique_ptr<VolumeRunner> runner;
  std::string setup_error;
  if (!cfg.cpu) {
    try {
      runner = std::make_unique<VolumeRunner>(device);
    } catch (const std::exception& e) {
      setup_error = e.what();
    }
  }
  std::vector<VolOutcome> mine;
  double my_wall = 0;
  auto write_planes = [&](const VolPatient& pp, int z0, int d, const std::vector<std::vector<uint8_t>>& files) {
    for (int z = 0; z < d; ++z) {
      const std::string stem = pp.out_dir + "/" + cohort::stem(pp.files[(size_t)(z0 + z)]);
      write_file(stem + "_original.jpg", files[2 * z]);
      write_file(stem + "_processed.jpg", files[2 * z + 1]);
    }
  };
  if (cfg.split_volume) {
    // Every patient's volume over ALL ranks, one z-slab each (volume_slabs.h). Failures before the
    // collective part are agreed on first; a failure inside it is fatal for the rank, and the
    // launcher's abort flag then ends the others' collectives.
    for (const VolPatient& pp : plan) {
      VolOutcome o;
      const double t0 = wall_now();
      const int depth = (int)pp.files.size();
      int z0 = 0, z1 = 0;
      VolumeInput slab;
      int64_t bad = 0;
      try {
        if (!setup_error.empty()) throw std::runtime_error(setup_error);
        if (!pp.listed) throw std::runtime_error(pp.error);
        if (depth < size)
          throw std::runtime_error("--split-volume: " + std::to_string(depth) + " planes cannot be split over " +
                                   std::to_string(size) + " ranks");
        std::tie(z0, z1) = slab_bounds(depth, rank, size);
        slab = load_volume(std::vector<std::string>(pp.files.begin() + z0, pp.files.begin() + z1));
      } catch (const std::exception& e) {
        o.message = e.what();
        bad = 1;
      }
      // Agree on failures and on the plane shape before any exchange.
      double shape[2] = {bad ? -1.0 : (double)slab.w, bad ? -1.0 : (double)slab.h};
      double nshape[2] = {-shape[0], -shape[1]};
      comm.allreduce_sum_i64(&bad, 1);
      comm.allreduce_max_f64(shape, 2);
      comm.allreduce_max_f64(nshape, 2);
      if (!bad && (shape[0] != -nshape[0] || shape[1] != -nshape[1])) {
        bad = 1;
        o.message = "volume slices differ in size across slabs";
      }
      if (!bad) {
        SlabStats st;
        std::vector<std::vector<uint8_t>> files;
        if (cfg.cpu) {
          files = golden_slab_jpegs(comm, slab, z0, depth, vp, rp, &st);
        } else {
          VolumeResult r = runner->run_slab(comm, slab, z0, depth, vp, false, &st);
          o.gpu_s = r.kernels_s;
          VolumeExportStats xs;
          files = runner->export_jpegs(slab, vp, rp, &xs);
          o.export_s = xs.export_s;
          o.fallbacks = xs.jpeg_fallbacks;
        }
        o.sweeps = st.sweeps;
        o.rounds = st.rounds;
        o.exchanged = st.exchanged_bytes;
        o.slices = slab.d;
        write_planes(pp, z0, slab.d, files);
        o.ok = 1;
      } else if (o.message.empty()) {
        o.message = "failed on another rank";
      }
      o.wall_s = wall_now() - t0;
      my_wall += o.wall_s;
      mine.push_back(std::move(o));
    }
  }
  for (size_t i = lo; i < hi && !cfg.split_volume; ++i) {
    const VolPatient& pp = plan[i];
    VolOutcome o;
    const double t0 = wall_now();
    try {
      if (!setup_error.empty()) throw std::runtime_error(setup_error);
      if (!pp.listed) throw std::runtime_error(pp.error);
      VolumeInput v = load_volume(pp.files);
      o.slices = v.d;
      std::vector<std::vector<uint8_t>> files;
      VolumeMeasure measured = {};
      std::vector<VolumeLesion> lesions;
      IntensityStats intensity = {};
      measure::Glcm texture;
      std::vector<VolumeLesionDiameters> diameters;
      if (vp.measure_diameters) {  // the spacing the lengths are maximised in: the sidecar's, in integer micrometres
        measure::volume_spacing_um((double)v.spacing_x, (double)v.spacing_y, v.spacing_z, vp.spacing_um);
        const std::string ext = measure::volume_diameters_extent_error(v.w, v.h, v.d, vp.spacing_um);
        if (!ext.empty()) throw std::runtime_error("--measure-volume-diameters: " + ext);
      }
      VolumeThickness thickness = {};
      if (vp.dilate_um >= 0 || vp.measure_thickness) {  // the spacing the distances are taken in, and the extent rule
        measure::volume_spacing_um((double)v.spacing_x, (double)v.spacing_y, v.spacing_z, vp.spacing_um);
        const std::string ext = v.w > 65535 ? std::string("a row holds at most 65535 voxels")
                                            : measure::volume_distance_extent_error(v.w, v.h, v.d, vp.spacing_um);
        if (!ext.empty())
          throw std::runtime_error(std::string(vp.dilate_um >= 0 ? "--dilate-mm: " : "--measure-volume-thickness: ") + ext);
      }
      // --compare-to: the reference of this patient, read and checked before anything runs; a missing file or another
      // shape is a status of the table, not a failure of the patient
      std::vector<uint8_t> ref_mask, dilated;
      VolumeReference ref;
      VolumeCompare compared = {};
      VolumeCompareLesions compared_lesions;
      const std::string ref_path = cfg.compare_to.empty() ? std::string() : cohort::with_slash(cfg.compare_to) + pp.id + "/mask.mhd";
      vp.compare = nullptr;
      vp.compare_lesions = 0;
      if (!cfg.compare_to.empty()) {
        ref_mask = read_reference_mask(ref_path, v.w, v.h, v.d, &o.compare_status);
        if (o.compare_status == "ok") {
          measure::volume_spacing_um((double)v.spacing_x, (double)v.spacing_y, v.spacing_z, vp.spacing_um);
          const std::string ext = v.w > 65535 ? std::string("a row holds at most 65535 voxels")
                                              : measure::volume_distance_extent_error(v.w, v.h, v.d, vp.spacing_um);
          if (!ext.empty()) throw std::runtime_error("--compare-to: " + ext);
          ref.mask = ref_mask.data();
          ref.w = v.w, ref.h = v.h, ref.d = v.d;
          vp.compare = &ref;
          if (cfg.compare_lesions) {  // --compare-lesions: K8's limit on the slots, before anything runs
            if (volume_measure_scratch_words(v.w, v.h, v.d) == 0)
              throw std::runtime_error("--compare-lesions: volume too large to label: (w + 1) * h * d + 1 must stay below 2^32");
            vp.compare_lesions = cfg.compare_lesions;
            vp.measure_connectivity = cfg.measure_volume_connectivity;
          }
        }
      }
      VolumeMesh vmesh;
      const uint64_t mesh_cap = cfg.volume_mesh_max_mb << 20;
      VolumeViewsExport vx;
      if (cfg.volume_views) {  // an explicit point outside this patient's volume fails the patient, on both backends
        const std::string err = views::at_error(cfg.volume_views_at, v.w, v.h, v.d);
        if (!err.empty()) throw std::runtime_error("--volume-views-at: " + err);
      }
      if (cfg.cpu) {
        files = golden_volume_jpegs(v, vp, rp, vp.measure ? &measured : nullptr, &lesions, &intensity, &texture, &diameters,
                                    cfg.volume_views ? &cfg.volume_views_at : nullptr, &vx, cfg.volume_mesh ? &vmesh : nullptr,
                                    cfg.volume_mesh_placement, &thickness, cfg.volume_mask ? &dilated : nullptr, &compared, &compared_lesions);
        if (cfg.volume_mesh) {  // the check export_mesh makes between its two halves
          const std::string err = mesh::size_error(vmesh.vertices(), vmesh.quad_count(), mesh_cap);
          if (!err.empty()) throw std::runtime_error("--volume-mesh: " + err);
        }
      } else {
        VolumeResult r = runner->run(v, vp, cfg.volume_mask);
        o.sweeps = r.sweeps;
        o.gpu_s = r.kernels_s;
        o.measure_s = r.measure_s;
        o.compare_s = r.compare_s;
        compared = r.compare;
        o.compare_lesions_s = r.compare_lesions_s;
        compared_lesions = std::move(r.compare_lesions);
        dilated = std::move(r.dilated);
        measured = r.measure;
        lesions = std::move(r.lesions);
        diameters = std::move(r.diameters);
        intensity = r.intensity;
        texture = std::move(r.texture);
        thickness = r.thickness;
        VolumeExportStats xs;
        files = runner->export_jpegs(v, vp, rp, &xs);
        if (cfg.volume_views) vx = runner->export_views(v, vp, rp, cfg.volume_views_at, false, &xs);
        if (cfg.volume_mesh) vmesh = runner->export_mesh(v, vp, cfg.volume_mesh_placement, mesh_cap);
        o.export_s = xs.export_s;
        o.fallbacks = xs.jpeg_fallbacks;
      }
      write_planes(pp, 0, v.d, files);
      if (cfg.volume_views) {  // after the planes: a DICOM stem that equals a view's name loses its plane file
        for (int k = 0; k < 2 * kVolumeViewCount; ++k)
          write_file(pp.out_dir + "/" + views::file_name(k / 2, k & 1), vx.files[(size_t)k]);
        const std::string text = views::to_json(vx.views, v.spacing_x, v.spacing_y, v.spacing_z);
        const std::string path = pp.out_dir + "/" + views::kSidecarName;
        std::ofstream f(path, std::ios::binary | std::ios::trunc);
        f.write(text.data(), (std::streamsize)text.size());
        if (!f) throw std::runtime_error("Cannot write " + path);
        o.view_files = 2 * kVolumeViewCount;
      }
      if (cfg.volume_mesh) {  // the mesh file and its sidecar, one writer for both backends
        const std::vector<uint8_t> bytes = mesh::file_bytes(vmesh, cfg.volume_mesh_format);
        write_bytes(pp.out_dir + "/" + mesh::file_name(cfg.volume_mesh_format), bytes.data(), bytes.size());
        const std::string text = mesh::to_json(vmesh, cfg.volume_mesh_format, bytes.size(), v.spacing_x, v.spacing_y, v.spacing_z);
        write_bytes(pp.out_dir + "/" + mesh::kSidecarName, text.data(), text.size());
        o.mesh_files = 2;
        o.mesh_vertices = (int64_t)vmesh.vertices();
        o.mesh_quads = (int64_t)vmesh.quad_count();
      }
      if (cfg.volume_mask) {  // the dilated mask as 0 / 1 bytes at the series' spacing
        mhd::write(pp.out_dir + "/mask", dilated.data(), v.w, v.h, v.d, mhd::MetType::kUChar, v.spacing_x, v.spacing_y,
                   (float)v.spacing_z);
        o.mask_files = 2;
      }
      if (vp.compare) {  // the sidecar; its table fields travel to rank 0
        const VolumeCompareLesions* cl = vp.compare_lesions ? &compared_lesions : nullptr;
        const std::string text = compare::to_json(compared, v.w, v.h, v.d, vp.spacing_um, ref_path, cl);
        write_bytes(pp.out_dir + "/compare.json", text.data(), text.size());
        o.compare_fields = compare::csv_fields(compared, v.w, v.h, v.d, vp.spacing_um, ref_path, cl);
        if (cl) {
          o.lesion_rows = compare::lesions_table_rows(pp.id, compared_lesions);
          const compare::LesionsDerived lv = compare::derive_lesions(compared_lesions);
          o.lesion_f1_ok = lv.f1_ok, o.lesion_f1 = lv.f1;
        }
        const compare::Derived dv = compare::derive(compared, vp.spacing_um);
        o.dice_ok = dv.dice_ok, o.dice = dv.dice;
        o.distances_ok = dv.distances_ok, o.hausdorff_mm = dv.hausdorff_mm;
      }
      if (vp.measure) {  // the sidecar next to the planes; its text travels to rank 0 for the table
        o.measure_json = vp.measure_texture
                             ? golden::measure_volume_json(measured, vp.measure_intensity ? &intensity : nullptr,
                                                           vp.measure_lesions ? &lesions : nullptr, vp.measure_lesions, texture, v,
                                                           vp.pipe.apply_rescale, vp.measure_connectivity)
                         : vp.measure_intensity
                             ? golden::measure_volume_json(measured, intensity, vp.measure_lesions ? &lesions : nullptr,
                                                           vp.measure_lesions, v, vp.pipe.apply_rescale, vp.measure_connectivity)
                         : vp.measure_lesions
                             ? golden::measure_volume_json(measured, lesions, vp.measure_lesions, v, vp.pipe.apply_rescale,
                                                           vp.measure_connectivity)
                             : golden::measure_volume_json(measured, v, vp.pipe.apply_rescale, vp.measure_connectivity);
        if (vp.measure_thickness)  // after the global keys, before diameters_spacing_um / lesions_max
          o.measure_json = measure::insert_thickness_keys(std::move(o.measure_json), thickness, vp.spacing_um);
        if (vp.measure_diameters)  // last, so that diameters_spacing_um stands directly before lesions_max
          o.measure_json = measure::insert_diameter_keys(std::move(o.measure_json), diameters.data(), (int)diameters.size(),
                                                         vp.spacing_um);
        const std::string path = pp.out_dir + "/" + measure::volume_sidecar_name();
        std::ofstream f(path, std::ios::binary | std::ios::trunc);
        f.write(o.measure_json.data(), (std::streamsize)o.measure_json.size());
        if (!f) throw std::runtime_error("Cannot write " + path);
      }
      o.ok = 1;
    } catch (const std::exception& e) {
      o.message = e.what();
    }
    o.wall_s = wall_now() - t0;
    my_wall += o.wall_s;
    mine.push_back(std::move(o));
  }
  // ---- gather outcomes, rank 0 prints in patient order ---------------------------------------
  ByteWriter w;
  w.u32((uint32_t)mine.size());
  for (const auto& o : mine) {
    w.i32(o.ok);
    w.str(o.message);
    w.i32(o.sweeps);
    w.f64(o.gpu_s);
    w.f64(o.export_s);
    w.f64(o.wall_s);
    w.u64((uint64_t)o.slices);
    w.u64((uint64_t)o.fallbacks);
    w.i32(o.rounds);
    w.u64((uint64_t)o.exchanged);
    w.str(o.measure_json);
    w.f64(o.measure_s);
    w.i32(o.view_files);
    w.i32(o.mesh_files);
    w.u64((uint64_t)o.mesh_vertices);
    w.u64((uint64_t)o.mesh_quads);
    w.i32(o.mask_files);
    w.str(o.compare_status);
    w.str(o.compare_fields);
    w.i32(o.dice_ok);
    w.i32(o.distances_ok);
    w.f64(o.dice);
    w.f64(o.hausdorff_mm);
    w.f64(o.compare_s);
    w.str(o.lesion_rows);
    w.i32(o.lesion_f1_ok);
    w.f64(o.lesion_f1);
    w.f64(o.compare_lesions_s);
  }
  auto all = comm.allgather_bytes(w.b);
  double tot = wall_now() - t_start;
  comm.allreduce_max_f64(&tot, 1);
  std::vector<double> walls((size_t)size);
  comm.allgather(&my_wall, sizeof(double), walls.data());
  if (rank != 0) return 0;
  std::vector<VolOutcome> outs;
  for (auto& b : all) {
    ByteReader r(b.data(), b.size());
    const uint32_t k = r.u32();
    for (uint32_t i = 0; i < k; ++i) {
      VolOutcome o;
      o.ok = r.i32();
      o.message = r.str();
      o.sweeps = r.i32();
      o.gpu_s = r.f64();
      o.export_s = r.f64();
      o.wall_s = r.f64();
      o.slices = (int64_t)r.u64();
      o.fallbacks = (int64_t)r.u64();
      o.rounds = r.i32();
      o.exchanged = (int64_t)r.u64();
      o.measure_json = r.str();
      o.measure_s = r.f64();
      o.view_files = r.i32();
      o.mesh_files = r.i32();
      o.mesh_vertices = (int64_t)r.u64();
      o.mesh_quads = (int64_t)r.u64();
      o.mask_files = r.i32();
      o.compare_status = r.str();
      o.compare_fields = r.str();
      o.dice_ok = r.i32();
      o.distances_ok = r.i32();
      o.dice = r.f64();
      o.hausdorff_mm = r.f64();
      o.compare_s = r.f64();
      o.lesion_rows = r.str();
      o.lesion_f1_ok = r.i32();
      o.lesion_f1 = r.f64();
      o.compare_lesions_s = r.f64();
      outs.push_back(std::move(o));
    }
  }
  if (cfg.split_volume) {
    // Rank-major per-patient outcomes → one per patient: ok if every slab was, the first failure's
    // message, the slowest slab's times, the sum of planes and exchanged bytes.
    std::vector<VolOutcome> merged(plan.size());
    for (size_t i = 0; i < plan.size(); ++i) {
      VolOutcome& m = merged[i];
      m.ok = 1;
      for (int q = 0; q < size; ++q) {
        const VolOutcome& o = outs[(size_t)q * plan.size() + i];
        if (!o.ok) {
          if (m.ok || m.message == "failed on another rank") m.message = o.message;
          m.ok = 0;
        }
        m.sweeps = std::max(m.sweeps, o.sweeps);
        m.rounds = std::max(m.rounds, o.rounds);
        m.gpu_s = std::max(m.gpu_s, o.gpu_s);
        m.export_s = std::max(m.export_s, o.export_s);
        m.wall_s = std::max(m.wall_s, o.wall_s);
        m.slices += o.slices;
        m.fallbacks += o.fallbacks;
        m.exchanged += o.exchanged;
      }
    }
    outs = std::move(merged);
  }
  int successful = 0;
  int64_t slices = 0, fallbacks = 0;
  std::ostringstream pj;
  for (size_t i = 0; i < plan.size(); ++i) {
    const VolPatient& pp = plan[i];
    const VolOutcome& o = outs[i];
    std::cout << "\n=== Processing Patient: " << pp.id << " as a 3D volume ===\n" << std::endl;
    if (pp.setup_ok) std::cout << "Created output directory: " + pp.out_dir << std::endl;
    if (pp.listed) {
      std::cout << "Using series directory: " << pp.series_dir << std::endl;
      std::cout << "Found " << pp.files.size() << " DICOM files for patient " << pp.id << std::endl;
    }
    if (o.ok) {
      ++successful;
      slices += o.slices;
      fallbacks += o.fallbacks;
      if (cfg.cpu)
        std::cout << "\nPatient " << pp.id << " completed on the CPU golden model." << std::endl;
      else
        std::cout << "\nPatient " << pp.id << " completed. 3D region growing converged in " << o.sweeps
                  << " sweeps; GPU time " << o.gpu_s * 1e3 << " ms." << std::endl;
      if (cfg.split_volume)
        std::cout << "Split over " << size << " ranks: " << o.rounds << " exchange rounds, " << o.exchanged
                  << " bytes exchanged." << std::endl;
    } else {
      std::cerr << "Error processing patient " << pp.id << ": " << o.message << std::endl;
    }
    pj << (i ? ", " : "") << "{\"id\": \"" << pp.id << "\", \"ok\": " << (o.ok ? "true" : "false")
       << ", \"slices\": " << o.slices << ", \"sweeps\": " << o.sweeps << ", \"gpu_s\": " << o.gpu_s
       << ", \"export_s\": " << o.export_s << ", \"wall_s\": " << o.wall_s << ", \"rounds\": " << o.rounds
       << ", \"exchanged_bytes\": " << o.exchanged;
    if (cfg.measure_volume) pj << ", \"measure_s\": " << o.measure_s;
    if (!cfg.compare_to.empty()) pj << ", \"compare_s\": " << o.compare_s;
    if (cfg.compare_lesions) pj << ", \"compare_lesions_s\": " << o.compare_lesions_s;
    pj << "}";
  }
  std::cout << "\n=== All Processing Completed ===\n" << std::endl;
  std::cout << "Successfully processed " << successful << "/" << plan.size() << " patients." << std::endl;
  VolumeTotals volume_totals;
  if (cfg.measure_volume) {  // the cohort table, in plan order (an error is reported, not fatal)
    std::vector<VolumePatientRow> rows;
    for (size_t i = 0; i < plan.size(); ++i) rows.push_back({plan[i].id, outs[i].ok != 0, outs[i].measure_json});
    try {
      volume_totals = write_volumes_csv(cfg.out_dir, rows, cfg.measure_volume_intensity,
                                        cfg.measure_volume_texture ? cfg.engine.pipe.texture_levels : 0,
                                        cfg.measure_volume_thickness);
    } catch (const std::exception& e) {
      std::cerr << "Error writing volumes.csv: " << e.what() << std::endl;
    }
    if (cfg.measure_volume_lesions) {
      try {
        volume_totals.lesions = write_lesions_csv(cfg.out_dir, rows, cfg.measure_volume_diameters, &volume_totals);
      } catch (const std::exception& e) {
        std::cerr << "Error writing lesions.csv: " << e.what() << std::endl;
      }
    }
  }
  if (!cfg.compare_to.empty()) {  // the comparison table, in plan order (an error is reported, not fatal)
    try {
      std::string text = compare::csv_header(cfg.compare_lesions != 0) + "\n";
      const size_t commas = (size_t)std::count(text.begin(), text.end(), ',') - 1;  // after patient,status
      for (size_t i = 0; i < plan.size(); ++i) {
        const VolOutcome& o = outs[i];
        const bool ok = o.ok && o.compare_status == "ok";
        text += plan[i].id + "," + (o.ok ? o.compare_status : std::string("failed")) + "," +
                (ok ? o.compare_fields : std::string(commas - 1, ',')) + "\n";
      }
      write_bytes(cohort::with_slash(cfg.out_dir) + "comparisons.csv", text.data(), text.size());
      if (cfg.compare_lesions) {  // one row per reported lesion, side a before b, patients in plan order
        std::string rows = compare::lesions_table_header() + "\n";
        for (size_t i = 0; i < plan.size(); ++i)
          if (outs[i].ok && outs[i].compare_status == "ok") rows += outs[i].lesion_rows;
        write_bytes(cohort::with_slash(cfg.out_dir) + "compare_lesions.csv", rows.data(), rows.size());
      }
    } catch (const std::exception& e) {
      std::cerr << "Error writing comparisons.csv: " << e.what() << std::endl;
    }
  }
  if (!cfg.json.empty()) {
    std::ofstream f(cfg.json, std::ios::trunc);
    f << "{\"mode\": \"3d\", \"backend\": \"" << (cfg.cpu ? "cpu" : "gpu") << "\", \"gpus\": " << size
      << ", \"comm\": \"" << comm.backend() << "\", \"dilation_size\": " << vp.dilation_size;
    if (cfg.dilate_um >= 0) f << ", \"dilate_mm\": " << cfg.dilate_mm << ", \"dilate_um\": " << cfg.dilate_um;
    f << ", \"connectivity\": " << vp.connectivity << ", \"split_volume\": " << (cfg.split_volume ? "true" : "false")
      << ", \"wall_s\": " << tot << ", \"slices\": " << slices
      << ", \"jpeg_fallbacks\": " << fallbacks << ", \"per_rank_wall_s\": [";
    for (int r = 0; r < size; ++r) f << (r ? ", " : "") << walls[r];
    f << "], \"patients\": [" << pj.str() << "]";
    if (cfg.measure_volume) f << ", \"measure_volume\": " << volume_totals_json(volume_totals);
    if (cfg.volume_views) {
      int64_t vp_n = 0, vf_n = 0;
      for (const auto& o : outs) vp_n += o.ok && o.view_files > 0, vf_n += o.ok ? o.view_files : 0;
      f << ", \"volume_views\": {\"patients\": " << vp_n << ", \"files\": " << vf_n << ", \"at_mode\": \""
        << views::at_mode_name(cfg.volume_views_at.mode) << "\"}";
    }
    if (cfg.volume_mesh) {
      int64_t mp_n = 0, mv_n = 0, mq_n = 0;
      for (const auto& o : outs)
        if (o.ok && o.mesh_files > 0) ++mp_n, mv_n += o.mesh_vertices, mq_n += o.mesh_quads;
      f << ", \"volume_mesh\": {\"patients\": " << mp_n << ", \"vertices\": " << mv_n << ", \"quads\": " << mq_n
        << ", \"placement\": \"" << mesh::placement_name(cfg.volume_mesh_placement) << "\", \"format\": \""
        << mesh::format_name(cfg.volume_mesh_format) << "\"}";
    }
    if (cfg.volume_mask) {
      int64_t mk_n = 0;
      for (const auto& o : outs) mk_n += o.ok && o.mask_files > 0;
      f << ", \"volume_mask\": {\"patients\": " << mk_n << "}";
    }
    if (!cfg.compare_to.empty()) {
      int64_t cn = 0, dn = 0;
      double dice_sum = 0, hd_max = 0;
      bool any_hd = false;
      for (const auto& o : outs) {
        if (!o.ok || o.compare_status != "ok") continue;
        ++cn;
        if (o.dice_ok) ++dn, dice_sum += o.dice;
        if (o.distances_ok) any_hd = true, hd_max = std::max(hd_max, o.hausdorff_mm);
      }
      char buf[160];
      std::string dm = "null", hm = "null";
      if (dn) std::snprintf(buf, sizeof buf, "%.9g", dice_sum / (double)dn), dm = buf;
      if (any_hd) std::snprintf(buf, sizeof buf, "%.9g", hd_max), hm = buf;
      f << ", \"compare\": {\"volumes\": " << cn << ", \"dice_mean\": " << dm << ", \"hausdorff_mm_max\": " << hm;
      if (cfg.compare_lesions) {
        int64_t fn = 0;
        double f1_sum = 0;
        for (const auto& o : outs)
          if (o.ok && o.compare_status == "ok" && o.lesion_f1_ok) ++fn, f1_sum += o.lesion_f1;
        std::string fm = "null";
        if (fn) std::snprintf(buf, sizeof buf, "%.9g", f1_sum / (double)fn), fm = buf;
        f << ", \"lesions\": true, \"lesion_f1_mean\": " << fm;
      }
      f << "}";
    }
    f << "}\n";
  }
  return 0;
}

}  // namespace

int run_volume_cohort(const AppConfig& cfg) {
  // 3D variant of the cohort run (BASELINE config 5): each patient's series becomes one volume
  // (3D SRG + cube dilation on the GPU), exported per plane like the 2D run; patients are sharded
  // over the ranks (one process per MI355X) like the 2D work list.
  // Both backends take the GPU kernels' limits, so --cpu stays the oracle of the same command.
  try {
    const int c = cfg.engine.pipe.srg_connectivity;
    check_volume_params(c == 4 ? 6 : c, cfg.dilation_set ? cfg.engine.pipe.dilation_size : 7);
  } catch (const std::invalid_argument& e) {
    std::cerr << "--mode 3d: " << e.what() << std::endl;
    return 2;
  }
  LaunchOptions lo = LaunchOptions::from_env();
  int n = 1;
  if (cfg.cpu) {  // golden model: the ranks are CPU processes over the host comm (default 1)
    n = std::max(1, cfg.gpus);  // auto / all: 1
    lo.comm = "host";
  } else {
    n = resolve_gpus(cfg, lo);
  }
  return launch_ranks(n, [&](int rank, int size, Comm& comm) {
    const int dev = size > 1 ? lo.device_of(rank) : lo.device_override >= 0 ? lo.device_override : cfg.engine.device;
    return volume_rank(cfg, rank, size, comm, dev);
  }, lo);
}

}  // namespace app
}  // namespace nm03
