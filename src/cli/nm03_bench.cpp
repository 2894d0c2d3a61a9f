// nm03_bench — native benchmark driver: the BASELINE configs on the engine without the CLI's
// message catalogue. Prints one JSON line.
//   --config cohort  (2/3)   full synthetic T1+C cohort, end-to-end (read → GPU → JPEG files);
//                            with --host-only every load, pack and file write but no GPU
//   --config volume  (5)     one patient series as a volume, 3D SRG + cube dilation
//   --config cpu-reference   BASELINE.md protocol: the golden CPU model in the reference's
//                            structure — per patient, batches of ≤25 slices over 16 threads
//                            (#pragma omp parallel for, main_parallel.cpp:336), then a SERIAL
//                            export of the batch (render + JPEG + write, main_parallel.cpp:346)
//   --config volume-cpu      config 5 on the golden CPU model (per-slice preprocessing on the
//                            thread pool, then 3D SRG + cube dilation)
//   --config single          config 1: test_pipeline's single slice (all stages + 5 renders +
//                            5 JPEGs, test_pipeline.cpp:29-182) on the GPU, latency per slice
//   --config single-cpu      config 1 on the golden CPU model
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>

#include "nm03/app.h"
#include "nm03/cohort.h"
#include "nm03/engine.h"
#include "nm03/golden.h"
#include "nm03/jpeg.h"
#include "nm03/log.h"
#include "nm03/thread_pool.h"
#include "nm03/volume.h"

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
  nm03::install_crash_handler();
  nm03::app::arm_fast_exit();
  std::string config = "cohort", root = nm03::cohort::default_data_root(), out = "/tmp/nm03_bench_out";
  int steps = 10, warmup = 2;
  nm03::EngineConfig ec;
  int dil3d = 7;
  bool measure_volume = false;  // volume: also K8 (the volumetry of the dilated volume) per run
  int measure_volume_conn = 26;
  int measure_volume_lesions = 0;  // volume: also K10 (one record per lesion, the N largest) per run
  bool measure_volume_diameters = false;  // volume: also K13 (every reported lesion's diameters) per run
  bool diameters_brute_force = false;     // volume: K13 compares every tile pair (the same records; for comparison)
  bool measure_texture = false;    // cohort with --measure / volume with --measure-volume: also K12 (co-occurrence matrix)
  int texture_levels = 32;
  bool measure_intensity = false;  // cohort with --measure / volume with --measure-volume: also K11 (percentiles, sum of squares)
  bool volume_views = false;       // volume: also K14 and the render + encode of the twelve view files per run
  bool volume_mesh = false;        // volume: also K15 (the surface mesh of the dilated volume) per run
  int64_t dilate_um = -1;          // volume: the margin of --dilate-mm R (K16) in place of the cube / ball, inside kernels_s
  double dilate_mm = 0;
  bool measure_volume_thickness = false;  // volume with --measure-volume: also K16's thickness, inside measure_s
  int compare_lesions = 0;  // volume with --compare: also K18 with N reported lesions per side, outside compare_ms_per_volume
  bool compare = false;  // volume: also K17 (the dilated volume against the run's own undilated region), outside kernels_s and measure_s
  int mesh_placement = nm03::kMeshCorner;
  uint64_t mesh_max_mb = nm03::mesh::kDefaultMaxMb;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto v = [&] { return std::string(argv[++i]); };
    if (a == "--config") config = v();
    else if (a == "--data-root") root = nm03::cohort::with_slash(v());
    else if (a == "--out") out = v();
    else if (a == "--steps") steps = std::atoi(v().c_str());
    else if (a == "--warmup") warmup = std::atoi(v().c_str());
    else if (a == "--batch-size") ec.batch_size = std::atoi(v().c_str());
    else if (a == "--streams") ec.streams = std::atoi(v().c_str());
    else if (a == "--threads") ec.threads = std::atoi(v().c_str());
    else if (a == "--median-window") ec.pipe.median_window = std::atoi(v().c_str());
    else if (a == "--max-dim") ec.max_dim = std::atoi(v().c_str());
    else if (a == "--dilation-3d") dil3d = std::atoi(v().c_str());
    else if (a == "--device") ec.device = std::atoi(v().c_str());
    else if (a == "--host-only") ec.host_only = true;  // cohort: every load/pack/write, no GPU (sanitizer sweeps)
    // The FAST-unpinned choices (app.h flags of the CLIs) for timing their kernel paths.
    else if (a == "--jpeg-sampling") {
      const std::string s = v();
      ec.render.jpeg_sampling = s == "gray" ? 2 : s == "444" ? 1 : 0;
    }
    else if (a == "--overlay") ec.render.overlay = true;  // cohort: also the colour overlay per slice
    else if (a == "--measure") ec.pipe.measure = true;    // cohort: also K7 and the measurement sidecar per slice
    else if (a == "--measure-diameters") ec.pipe.measure = ec.pipe.measure_diameters = true;  // cohort: K7, K9 and the extended sidecar
    else if (a == "--measure-intensity") measure_intensity = true;
    else if (a == "--measure-texture") measure_texture = true;
    else if (a == "--texture-levels") texture_levels = std::min(64, std::max(2, std::atoi(v().c_str())));
    else if (a == "--measure-connectivity") ec.pipe.measure_connectivity = std::atoi(v().c_str()) == 4 ? 4 : 8;
    else if (a == "--measure-volume") measure_volume = true;
    else if (a == "--measure-volume-connectivity") measure_volume_conn = std::atoi(v().c_str()) == 6 ? 6 : 26;
    else if (a == "--measure-volume-lesions") {
      measure_volume_lesions = std::atoi(v().c_str());
      if (measure_volume_lesions < 1 || measure_volume_lesions > nm03::kMaxVolumeLesions) {
        std::cerr << "--measure-volume-lesions must be 1.." << nm03::kMaxVolumeLesions << std::endl;
        return 2;
      }
      measure_volume = true;
    }
    else if (a == "--measure-volume-diameters") measure_volume_diameters = true;
    else if (a == "--volume-diameters-brute-force") diameters_brute_force = true;
    else if (a == "--dilate-mm") {
      dilate_mm = std::atof(v().c_str());
      if (!(dilate_mm >= 0.0 && dilate_mm <= nm03::kMaxDilateMm)) {
        std::cerr << "--dilate-mm must be in [0, 1000]" << std::endl;
        return 2;
      }
      dilate_um = nm03::measure::dilate_mm_to_um(dilate_mm);
    }
    else if (a == "--measure-volume-thickness") measure_volume_thickness = true;
    else if (a == "--compare") compare = true;
    else if (a == "--compare-lesions") compare_lesions = std::stoi(v());
    else if (a == "--volume-views") volume_views = true;
    else if (a == "--volume-mesh") volume_mesh = true;
    else if (a == "--volume-mesh-placement") {
      if (!nm03::mesh::parse_placement(v(), &mesh_placement)) {
        std::cerr << "--volume-mesh-placement must be corner or nets" << std::endl;
        return 2;
      }
    }
    else if (a == "--volume-mesh-max-mb") mesh_max_mb = std::stoull(v());
    else if (a == "--se-shape") ec.pipe.se_shape = v() == "disc" ? nm03::kSeDisc : nm03::kSeSquare;
    else if (a == "--render-filter") ec.render.filter = v() == "nearest" ? nm03::kFilterNearest : nm03::kFilterBilinear;
    else {
      std::cerr << "unknown option " << a << std::endl;
      return 2;
    }
  }
  if ((measure_volume_diameters || diameters_brute_force) && !measure_volume_lesions) {
    std::cerr << "--measure-volume-diameters needs --measure-volume-lesions N" << std::endl;
    return 2;
  }
  if (diameters_brute_force) measure_volume_diameters = true;
  if ((dilate_um >= 0 || measure_volume_thickness) && (config != "volume" || ec.host_only)) {
    std::cerr << "--dilate-mm and --measure-volume-thickness need --config volume and the GPU (not --host-only)" << std::endl;
    return 2;
  }
  if (measure_volume_thickness) measure_volume = true;
  if (compare && (config != "volume" || ec.host_only)) {
    std::cerr << "--compare needs --config volume and the GPU (not --host-only)" << std::endl;
    return 2;
  }
  if (compare_lesions != 0 && !compare) {
    std::cerr << "--compare-lesions needs --compare" << std::endl;
    return 2;
  }
  if (compare_lesions < 0 || compare_lesions > nm03::kMaxVolumeLesions) {
    std::cerr << "--compare-lesions must be 1.." << nm03::kMaxVolumeLesions << std::endl;
    return 2;
  }
  if (volume_views && (config != "volume" || ec.host_only)) {
    std::cerr << "--volume-views needs --config volume and the GPU (not --host-only)" << std::endl;
    return 2;
  }
  if (volume_mesh && (config != "volume" || ec.host_only)) {
    std::cerr << "--volume-mesh needs --config volume and the GPU (not --host-only)" << std::endl;
    return 2;
  }
  // --measure-intensity implies the measurement it extends: --measure (cohort) or --measure-volume (volume).
  if (measure_intensity && config == "cohort") ec.pipe.measure = ec.pipe.measure_intensity = true;
  if (measure_intensity && config == "volume") measure_volume = true;
  // --measure-texture likewise.
  if (measure_texture && config == "cohort") ec.pipe.measure = ec.pipe.measure_texture = true, ec.pipe.texture_levels = texture_levels;
  if (measure_texture && config == "volume") measure_volume = true;
  try {
    const std::string base = nm03::cohort::cohort_dir(root);
    auto pids = nm03::cohort::find_patient_dirs(base);
    if (config == "cohort") {
      std::vector<nm03::WorkItem> items;
      for (const auto& p : pids) {
        auto s = nm03::cohort::list_patient_series(base, p);
        const std::string od = out + "/" + p;
        nm03::cohort::make_dirs(od);
        for (const auto& f : s.files) items.push_back({f, od});
      }
      nm03::Engine eng(ec);
      for (int w = 0; w < warmup; ++w) eng.run(items);
      nm03::StageTimes t, acc;
      const double t0 = now_s();
      for (int k = 0; k < steps; ++k) {
        eng.run(items, &t);
        acc.load_s += t.load_s;
        acc.kernels_s += t.kernels_s;
        acc.h2d_s += t.h2d_s;
        acc.write_s += t.write_s;
        acc.slices_ok += t.slices_ok;
      }
      const double dt = now_s() - t0;
      std::cout << "{\"config\": \"cohort\", \"slices_per_step\": " << items.size() << ", \"steps\": " << steps
                << ", \"ms_per_step\": " << dt * 1e3 / steps << ", \"slices_per_s\": " << acc.slices_ok / dt
                << ", \"load_s\": " << acc.load_s << ", \"h2d_s\": " << acc.h2d_s << ", \"kernels_s\": " << acc.kernels_s
                << ", \"write_s\": " << acc.write_s << "}" << std::endl;
    } else if (config == "cpu-reference") {
      nm03::ThreadPool pool(ec.threads);
      std::vector<std::pair<std::string, std::vector<std::string>>> pats;
      for (const auto& p : pids) {
        auto s = nm03::cohort::list_patient_series(base, p);
        const std::string od = out + "/" + p;
        nm03::cohort::make_dirs(od);
        pats.push_back({od, s.files});
      }
      auto one_pass = [&]() -> size_t {
        size_t ok = 0;
        for (auto& pp : pats) {
          const auto& files = pp.second;
          for (size_t b0 = 0; b0 < files.size(); b0 += (size_t)ec.batch_size) {
            const size_t nb = std::min((size_t)ec.batch_size, files.size() - b0);
            std::vector<nm03::golden::SliceInput> in(nb);
            std::vector<nm03::golden::SliceResult> res(nb);
            std::vector<char> good(nb, 0);
            {
              nm03::TaskGroup tg(pool);
              for (size_t i = 0; i < nb; ++i)
                tg.run([&, i] {
                  try {
                    in[i] = nm03::golden::load_slice(files[b0 + i], ec.pipe.min_dim);
                    res[i] = nm03::golden::run(in[i], ec.pipe, false);
                    good[i] = 1;
                  } catch (...) {
                  }
                });
              tg.wait();
            }
            for (size_t i = 0; i < nb; ++i) {  // serial export, like exportBatch
              if (!good[i]) continue;
              auto j = nm03::golden::export_jpegs(in[i], res[i], ec.pipe, ec.render);
              const std::string stem = pp.first + "/" + nm03::cohort::stem(files[b0 + i]);
              nm03::jpeg::write_jpeg_file(stem + "_original.jpg", {}, j.original.data(), j.original.size() - 2);
              nm03::jpeg::write_jpeg_file(stem + "_processed.jpg", {}, j.processed.data(), j.processed.size() - 2);
              ++ok;
            }
          }
        }
        return ok;
      };
      for (int w = 0; w < warmup; ++w) one_pass();
      size_t ok = 0;
      const double t0 = now_s();
      for (int k = 0; k < steps; ++k) ok += one_pass();
      const double dt = now_s() - t0;
      std::cout << "{\"config\": \"cpu-reference\", \"threads\": " << ec.threads << ", \"batch\": " << ec.batch_size
                << ", \"steps\": " << steps << ", \"ms_per_step\": " << dt * 1e3 / steps
                << ", \"slices_per_s\": " << ok / dt << "}" << std::endl;
    } else if (config == "volume") {
      if (pids.empty()) throw std::runtime_error("no patients");
      auto s = nm03::cohort::list_patient_series(base, pids[0]);
      nm03::VolumeInput v = nm03::load_volume(s.files);
      nm03::VolumeParams vp;
      vp.pipe = ec.pipe;
      vp.dilation_size = dil3d;
      vp.measure = measure_volume;
      vp.measure_connectivity = measure_volume_conn;
      vp.measure_lesions = measure_volume_lesions;
      vp.measure_diameters = measure_volume_diameters;
      vp.diameters_brute_force = diameters_brute_force;
      if (measure_volume_diameters) nm03::measure::volume_spacing_um((double)v.spacing_x, (double)v.spacing_y, v.spacing_z, vp.spacing_um);
      vp.measure_intensity = measure_intensity;
      vp.measure_texture = measure_texture;
      vp.texture_levels = texture_levels;
      vp.dilate_um = dilate_um;
      vp.measure_thickness = measure_volume_thickness;
      if (dilate_um >= 0 || measure_volume_thickness)
        nm03::measure::volume_spacing_um((double)v.spacing_x, (double)v.spacing_y, v.spacing_z, vp.spacing_um);
      nm03::VolumeRunner runner(ec.device);
      // --compare: the reference is this run's own undilated region, so no file is needed
      std::vector<uint8_t> compare_mask;
      nm03::VolumeReference compare_ref;
      if (compare) {
        compare_mask = runner.run(v, vp, true).region;
        compare_ref.mask = compare_mask.data();
        compare_ref.w = v.w, compare_ref.h = v.h, compare_ref.d = v.d;
        nm03::measure::volume_spacing_um((double)v.spacing_x, (double)v.spacing_y, v.spacing_z, vp.spacing_um);
        vp.compare = &compare_ref;
        vp.compare_lesions = compare_lesions;
      }
      for (int w = 0; w < warmup; ++w) runner.run(v, vp, false);
      double ks = 0, ms = 0, cs = 0, ls = 0;
      nm03::VolumeCompare vc = {};
      nm03::VolumeCompareLesions vl;
      int sweeps = 0;
      nm03::VolumeMeasure vm = {};
      size_t lesions = 0;
      uint64_t lesion0_vox = 0, lesion0_major_um2 = 0;
      nm03::IntensityStats vi = {};
      uint64_t glcm_pairs = 0;
      nm03::VolumeThickness vt = {};
      const double t0 = now_s();
      for (int k = 0; k < steps; ++k) {
        auto r = runner.run(v, vp, false);
        ks += r.kernels_s;
        ms += r.measure_s;
        cs += r.compare_s;
        vc = r.compare;
        ls += r.compare_lesions_s;
        if (compare_lesions) vl = std::move(r.compare_lesions);
        sweeps = r.sweeps;
        vm = r.measure;
        vi = r.intensity;
        glcm_pairs = r.texture.head.pairs;
        vt = r.thickness;
        lesions = r.lesions.size();
        lesion0_vox = lesions ? r.lesions[0].voxels : 0;
        lesion0_major_um2 = r.diameters.empty() ? 0 : r.diameters[0].major_um2;
      }
      const double dt = now_s() - t0;
      vp.compare = nullptr;  // the comparison is timed above alone
      vp.compare_lesions = 0;
      // + the GPU export of every plane (render + JPEG, both images), as the 3D CLI does
      nm03::VolumeExportStats xs;
      for (int w = 0; w < warmup; ++w) runner.export_jpegs(v, vp, ec.render);
      const double t1 = now_s();
      for (int k = 0; k < steps; ++k) {
        runner.run(v, vp, false);
        runner.export_jpegs(v, vp, ec.render, &xs);
      }
      const double dt2 = now_s() - t1;
      // + the views (K14, then borders + render + encode of the twelve files), as the 3D CLI does with --volume-views
      double views_ms = 0, k14_ms = 0, views_render_ms = 0;
      size_t view_bytes = 0;
      if (volume_views) {
        const nm03::ViewsAt at;  // mask
        for (int w = 0; w < warmup + 1; ++w) runner.export_views(v, vp, ec.render, at);
        const double t2 = now_s();
        for (int k = 0; k < steps; ++k) {
          const auto x = runner.export_views(v, vp, ec.render, at);
          k14_ms += x.k14_s * 1e3;
          views_render_ms += x.render_s * 1e3;
          view_bytes = 0;
          for (const auto& f : x.files) view_bytes += f.size();
        }
        views_ms = (now_s() - t2) * 1e3;
      }
      // + the surface mesh (K15) of the dilated volume the last run left on the device, as the 3D CLI does with
      // --volume-mesh: mesh_ms_per_volume from device events, outside kernels_s
      double mesh_ms = 0, mesh_wall_ms = 0;
      size_t mesh_v = 0, mesh_q = 0;
      if (volume_mesh) {
        for (int w = 0; w < warmup + 1; ++w) runner.export_mesh(v, vp, mesh_placement, mesh_max_mb << 20);
        const double t3 = now_s();
        for (int k = 0; k < steps; ++k) {
          const auto m = runner.export_mesh(v, vp, mesh_placement, mesh_max_mb << 20);
          mesh_ms += m.k15_s * 1e3;
          mesh_v = m.vertices();
          mesh_q = m.quad_count();
        }
        mesh_wall_ms = (now_s() - t3) * 1e3;
      }
      std::cout << "{\"config\": \"volume\", \"dims\": [" << v.w << ", " << v.h << ", " << v.d << "], \"steps\": " << steps
                << ", \"ms_per_volume\": " << dt * 1e3 / steps << ", \"gpu_ms_per_volume\": " << ks * 1e3 / steps
                << ", \"sweeps\": " << sweeps << ", \"ms_per_volume_with_export\": " << dt2 * 1e3 / steps
                << ", \"export_ms_per_volume\": " << xs.export_s * 1e3 / steps;
      if (measure_volume)
        std::cout << ", \"measure_ms_per_volume\": " << ms * 1e3 / steps << ", \"volume_vox\": " << vm.volume_vox
                  << ", \"components\": " << vm.components << ", \"cavities\": " << vm.cavities;
      if (measure_volume_lesions)
        std::cout << ", \"lesions_max\": " << measure_volume_lesions << ", \"lesions\": " << lesions
                  << ", \"largest_lesion_vox\": " << lesion0_vox;
      if (measure_volume_diameters)
        std::cout << ", \"diameters\": true, \"diameters_brute_force\": " << (diameters_brute_force ? "true" : "false")
                  << ", \"largest_lesion_major_um2\": " << lesion0_major_um2;
      if (volume_views)
        std::cout << ", \"views_ms_per_volume\": " << views_ms / steps << ", \"views_k14_ms\": " << k14_ms / steps
                  << ", \"views_render_encode_ms\": " << views_render_ms / steps << ", \"views_jpeg_bytes\": " << view_bytes;
      if (volume_mesh)
        std::cout << ", \"mesh_ms_per_volume\": " << mesh_ms / steps << ", \"mesh_wall_ms_per_volume\": " << mesh_wall_ms / steps
                  << ", \"mesh_placement\": \"" << nm03::mesh::placement_name(mesh_placement) << "\", \"mesh_vertices\": " << mesh_v
                  << ", \"mesh_quads\": " << mesh_q;
      if (measure_intensity) std::cout << ", \"intensity\": true, \"raw_p50\": " << vi.pct[2];
      if (measure_texture)
        std::cout << ", \"texture\": true, \"texture_levels\": " << texture_levels << ", \"glcm_pairs\": " << glcm_pairs;
      if (dilate_um >= 0) std::cout << ", \"dilate_mm\": " << dilate_mm << ", \"dilate_um\": " << dilate_um;
      if (compare) {
        const nm03::compare::Derived dv = nm03::compare::derive(vc, vp.spacing_um);
        std::cout << ", \"compare_ms_per_volume\": " << cs * 1e3 / steps << ", \"compare_surface_a\": " << vc.surface_a
                  << ", \"compare_surface_b\": " << vc.surface_b << ", \"compare_dice\": " << dv.dice
                  << ", \"compare_hausdorff_mm\": " << dv.hausdorff_mm << ", \"compare_hd95_mm\": " << dv.hd95_mm;
        if (compare_lesions)
          std::cout << ", \"compare_lesions\": " << compare_lesions << ", \"compare_lesions_ms_per_volume\": " << ls * 1e3 / steps
                    << ", \"compare_lesions_a\": " << vl.head.lesions_a << ", \"compare_lesions_b\": " << vl.head.lesions_b
                    << ", \"compare_hit_b\": " << vl.head.hit_b << ", \"compare_multi_a\": " << vl.head.multi_a;
      }
      if (measure_volume_thickness)
        std::cout << ", \"thickness\": true, \"inscribed_um2\": " << vt.inscribed_um2
                  << ", \"thickness_mm\": " << 2.0 * nm03::measure::inscribed_radius_mm(vt);
      std::cout << "}" << std::endl;
    } else if (config == "volume-cpu") {
      if (pids.empty()) throw std::runtime_error("no patients");
      auto s = nm03::cohort::list_patient_series(base, pids[0]);
      nm03::ThreadPool pool(ec.threads);
      auto one = [&]() -> size_t {
        nm03::VolumeInput v = nm03::load_volume(s.files);
        const size_t plane = (size_t)v.w * v.h;
        std::vector<uint8_t> band(plane * v.d);
        {
          nm03::TaskGroup tg(pool);
          for (int z = 0; z < v.d; ++z)
            tg.run([&, z] {
              nm03::golden::SliceInput si;
              si.w = v.w;
              si.h = v.h;
              si.type = v.type;
              si.stored_bits = v.stored_bits;
              si.slope = v.slope;
              si.intercept = v.intercept;
              si.raw.assign(v.raw.begin() + z * plane, v.raw.begin() + (z + 1) * plane);
              auto c = nm03::golden::norm_clip(si, ec.pipe);
              auto m = nm03::golden::median(c, v.w, v.h, ec.pipe.median_window);
              auto sh = nm03::golden::sharpen(m, v.w, v.h, ec.pipe.sharpen_gain, ec.pipe.sharpen_sigma,
                                              ec.pipe.sharpen_mask);
              auto b = nm03::golden::band(sh, ec.pipe.srg_min, ec.pipe.srg_max);
              std::copy(b.begin(), b.end(), band.begin() + z * plane);
            });
          tg.wait();
        }
        auto seeds = nm03::reference_seeds(v.w, v.h);
        for (auto& sd : seeds) sd.z = v.d / 2;
        auto region = nm03::golden::region_grow3d(band, v.w, v.h, v.d, seeds, 6);
        auto dil = nm03::golden::dilate3d(region, v.w, v.h, v.d, dil3d);
        size_t n = 0;
        for (uint8_t x : dil) n += x;
        return n;
      };
      for (int w = 0; w < warmup; ++w) one();
      const double t0 = now_s();
      size_t vox = 0;
      for (int k = 0; k < steps; ++k) vox = one();
      const double dt = now_s() - t0;
      std::cout << "{\"config\": \"volume-cpu\", \"threads\": " << ec.threads << ", \"slices\": " << s.files.size()
                << ", \"steps\": " << steps << ", \"ms_per_volume\": " << dt * 1e3 / steps
                << ", \"dilated_voxels\": " << vox << "}" << std::endl;
    } else if (config == "single" || config == "single-cpu") {
      const bool cpu = config == "single-cpu";
      const std::string f = nm03::cohort::test_slice_path(root);
      std::unique_ptr<nm03::Engine> eng;
      if (!cpu) {
        ec.streams = 1;
        eng = std::make_unique<nm03::Engine>(ec);
      }
      auto one = [&] {
        nm03::golden::SliceInput si = nm03::golden::load_slice(f, 0);
        size_t n = 0;
        if (cpu) {
          auto r = nm03::golden::test_pipeline_images(si, ec.pipe, ec.render);
          for (auto& j : r.jpegs) n += j.size();
          return n;
        }
        auto r = eng->run_single(si);
        for (auto& j : r.jpegs) n += j.size();
        return n;
      };
      for (int w = 0; w < warmup; ++w) one();
      const double t0 = now_s();
      size_t bytes = 0;
      for (int k = 0; k < steps; ++k) bytes = one();
      const double dt = now_s() - t0;
      std::cout << "{\"config\": \"" << config << "\", \"steps\": " << steps
                << ", \"ms_per_slice\": " << dt * 1e3 / steps << ", \"jpeg_bytes\": " << bytes << "}" << std::endl;
    } else {
      throw std::runtime_error("unknown config " + config);
    }
  } catch (const std::exception& e) {
    std::cerr << "Fatal error: " << e.what() << std::endl;
    return nm03::app::cli_exit(1);
  }
  // Like the CLIs: return from main (rocprofv3 writes its results when main returns), then the
  // handler armed at the start of main _exits before the shared libraries' destructors. Under
  // rocprofv3 a full teardown died with SIGSEGV inside libamdhip64's own static destructor, after
  // the tool's finalisation, with no nm03 frame on the stack
  // (profiles/r4/probe/c5_prof_segv_backtrace.txt); exiting from inside main lost the results.
  return nm03::app::cli_exit(0);
}
