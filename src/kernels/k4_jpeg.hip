// K4 — JPEG export on the GPU (replaces ImageFileExporter → Qt → libjpeg on the host,
// main_sequential.cpp:61-73). Output is byte-identical to libjpeg(-turbo) baseline q75 4:2:0
// (nm03/jpeg_common.h; golden encoder src/io/jpeg.cpp; tests/test_jpeg.py vs Pillow).
//
// One launch per batch (a batch of 64 slices = 128 canvases = 524k luma blocks), after a clear of
// the look-back records:
//    jpeg_fused_kernel   workgroup per 256 luma blocks (64 MCUs) of an image, thread per block.
//                        Pixels come from the canvas or — for an exact 2× fit, the common case —
//                        are rendered on the fly from the 6×6 source patch (render_core.h), so the
//                        256 KiB canvas never exists. The workgroup first stages its source rows
//                        in LDS (gray: rescaled f32, 18 × 258 for a 256² slice; labels: the label
//                        and border bit rows) with coalesced loads: 76 → 67 µs per 64-slice batch.
//                        islow FDCT as v_dot2_i32_i16 dot products (label waves of one flat colour
//                        skip FDCT, quantisation and coding), quantisation by exact reciprocal (umulhi
//                        by ceil(2^32/d): exact for |x|, d < 2^16),
//                        Huffman cost, workgroup scan, the workgroup's bit range assembled in LDS,
//                        its 0xFF-byte counts for all 8 byte alignments, a decoupled look-back
//                        over the image's earlier workgroups that resolves both the bit offset and
//                        the number of stuffing bytes before it, and the 0xFF-stuffed bytes it
//                        owns written straight into host-mapped pinned memory. (Earlier versions
//                        ORed the codes into an HBM stage and ran two more launches to count and
//                        insert the stuffing: 2.65 MB written + read back per batch, two launches.)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "device_util.h"
#include "jpeg_device.h"
#include "nm03/gpu_types.h"
#include "nm03/jpeg_common.h"
#include "nm03/kernels.h"
#include "render_core.h"

namespace nm03::gpu {

using namespace nm03::jpeg;


// Gray source staging: the raw rows a workgroup's 64 MCUs read (8 per MCU row + a 1-row halo each
// side, full width + 1-column halos, edge-clamped) are loaded once, coalesced, into LDS; the 6×6
// patches of the exact-2× render then come from LDS instead of 36 scattered global loads per
// block. Pixels are converted to f32 (rescale) once while staging, not once per patch use (2.25×).
// Staged gray rows are swizzled: source column c (0..W+1 with the halos) sits at c + c/4 of a row of
// stride ≡ 4 (mod 8) words. A half-wave's patch reads then hit distinct banks: its 16 blocks step
// 5 words apart (16 distinct banks mod 32) and its two block rows, 4 source rows apart, are offset
// by 16 banks (disjoint sets) — the plain layout's 4-byte stride put 4 addresses on each bank.
constexpr int kPatchLds = 5832;  // f32 elements (22.8 KiB; 256²: 18 × 324); larger footprints use global loads
__device__ __forceinline__ int swz_col(int c) { return c + (c >> 2); }
// One LDS region serves the render (source patch above) and then, once every block is rendered,
// the workgroup's assembled bit range followed by its staged stuffed output bytes.
constexpr int kUnionWords = kPatchLds + 1080;  // 27 KiB as before (4 workgroups per CU): bit ranges up to ~220 Kbit


// Single-pass encoder: workgroup with ticket L encodes blocks [256p, 256p+256) of image i.
//  1. render (fused 2×) or read the 8×8 block, islow FDCT, reciprocal quantisation;
//  2. Huffman cost of the block (DC needs the previous block's DC: LDS neighbour, and for the
//     first block of the workgroup a wave-0 recomputation of the preceding block's DC = Σ(x-128));
//  3. workgroup exclusive scan of the costs, then a decoupled look-back over the image's earlier
//     workgroups in ticket order (tickets are taken when a workgroup starts, so every workgroup
//     waited on is already resident). The spin is bounded anyway (an image whose look-back
//     times out is re-encoded on the CPU);
//  4. each thread writes its block's codes at its bit offset (atomicOr into the zeroed stage).
// The last workgroup of an image publishes the total (or the overflow marker).
// kOcc: target waves per SIMD (= workgroups per CU); kUnion: LDS words of the patch / bit-range
// union; kSamp: jpeg::Sampling — 4:2:0 scans MCUs of 2×2 luma blocks followed by the MCU's two
// all-zero chroma blocks; 4:4:4 scans the luma blocks in raster order, each followed by its two
// chroma blocks; gray scans them in raster order alone. (One instance per layout: the default
// 4:2:0 code is unchanged by the other two.) 5 workgroups per CU (31.7 KiB, ≤ 96 VGPRs with spills) measured no better than 4 once
// images were dealt round-robin (profiles/r3/jpeg_spread/split_and_occ5.txt).
template <int kOcc, int kUnion, int kSamp, bool kNearest>
__global__ __launch_bounds__(kJpegWG) __attribute__((amdgpu_waves_per_eu(kOcc))) void jpeg_fused_kernel(const uint8_t* __restrict__ canvas,
                                                             const JpegDesc* __restrict__ jd, int ncanvas, int out_w,
                                                             int out_h, QuantRecip q, JpegWork w, JpegRenderSrc rs,
                                                             uint8_t* __restrict__ out, int32_t* __restrict__ out_sizes,
                                                             int dbg) {
  // dbg: profiling variant (NM03_PROFILE_VARIANT=jpeg=N; output invalid), 0 = the real encoder.
  // kWG blocks (threads) per workgroup = kWG / 4 MCUs. (512-block workgroups, 8 waves and 2 per
  // CU, halve the per-workgroup fixed costs but measured no faster: 116.8–117.6 vs 119.2 µs per
  // 96-slice batch in the bench, profiles/r4/jpeg_wg512/.)
  constexpr int kWG = kJpegWG;
  constexpr int kPatch = kPatchLds;
  constexpr bool k420 = kSamp == kSampling420;
  // Scan units (MCUs) per workgroup and the canvas rows (source rows of the 2× render: half) of one
  // row of units.
  constexpr int kUnitBlocks = k420 ? 4 : 1, kUnitRows = k420 ? 16 : 8;
  static_assert(kPatch <= kUnion, "staging area exceeds the LDS union");
  __shared__ uint32_t actab[256];
  __shared__ uint32_t dctab[16];
  __shared__ int32_t sdc[kWG];
  __shared__ uint32_t spriv[kWG * kPrivWords];  // per-block AC Huffman bits
  __shared__ uint32_t s_ticket;
  __shared__ int32_t s_prevdc;
  __shared__ __attribute__((aligned(16))) float spatch[kUnion];  // render patch, then swg + output
  uint32_t* const swg = reinterpret_cast<uint32_t*>(spatch);             // the workgroup's bit range
  const int tid = threadIdx.x;
  // Records of the previous launch (the other half of the look area) are dead: clear them here
  // for the next launch instead of a separate memset launch.
  if (w.clear_words) {
    uint64_t* other = w.look + w.clear_base;
    for (size_t i = (size_t)blockIdx.x * kWG + tid; i < w.clear_words; i += (size_t)gridDim.x * kWG) other[i] = 0ull;
  }
  if (dbg == 8) {  // profiling variant: empty workgroup
    if (tid == 999) out_sizes[0] = 1;
    return;
  }
  const int bpi = (out_w >> 3) * (out_h >> 3);
  const int parts = (bpi + kWG - 1) / kWG;
  // The image is fixed by the dispatch index; only the part comes from the ticket. The ticket's
  // device-scope atomic is issued first, so its round trip overlaps the table and descriptor
  // loads below (issued after them it waited behind three dependent descriptor loads).
  // Images are dealt round-robin over the dispatch order (workgroup b encodes image b mod
  // ncanvas): consecutive workgroups hit different ticket counters instead of `parts` of them
  // queueing on one address, and an image's parts start one `ncanvas` stride apart, so a part's
  // predecessors have mostly finished encoding when it looks back (blocked order: 137.8–138.5 vs
  // 118.9–119.0 µs per 96-slice batch, profiles/r3/jpeg_spread/).
  const int img = (int)(blockIdx.x % (uint32_t)ncanvas);
  uint32_t ticket = 0;
  if (tid == 0) {
    // The address goes through a VGPR the compiler cannot prove uniform: a uniform-address atomic
    // is rewritten into a wave-aggregated one whose result is waited for on the spot.
    // (Kept in the global address space: a flat atomic would also count in lgkmcnt and hold up
    // the LDS waits behind it.)
    auto* tp = (__attribute__((address_space(1))) uint32_t*)&w.ticket[img];
    asm volatile("" : "+v"(tp));
    ticket = __hip_atomic_fetch_add(tp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  actab[tid] = kHuffAcLuma.e[tid];
  if (tid < 16) dctab[tid] = tid < 12 ? kHuffDcLuma.e[tid] : 0u;
  // JpegDesc::render is -1 or img itself, so the render descriptor loads alongside the JPEG one
  // (no dependent round trip); the render window (stats of the slice) is computed where the render
  // first needs it, so its load overlaps the staging below.
  const JpegDesc d = jd[img];
  RenderDesc rd;
  if (rs.rd) rd = rs.rd[img];
  RWindow win{0.f, 0.f};
  if (tid == 0) {
    // Ordered tickets per image: workgroup b encodes image b / parts and takes the next part of
    // that image from the image's counter, so it only ever waits on parts whose workgroups have
    // already started — progress is guaranteed even when other kernels (other streams, other
    // processes on the same GPU) share the CUs or the queue is preempted. (Using the dispatch
    // index as the part is ~5% faster, but two encoders interleaving on the same XCDs can starve
    // each other's predecessors: measured 2.3 s/step stalls with two ranks per GPU.) One counter per
    // image keeps the serialised atomics per address at `parts`.
    if (ticket == (uint32_t)parts - 1) atomicExch(&w.ticket[img], 0u);  // the image's last ticket
    s_ticket = ticket;
  }
  __syncthreads();
  // The part is workgroup-uniform: keep it in an SGPR.
  const int part = (int)__builtin_amdgcn_readfirstlane(s_ticket);
  if (dbg == 7) {  // profiling variant: tables + ticket only
    if (part == 0x7FFFFFF1) out_sizes[0] = 1;
    return;
  }
  // Profiling variants 40 / 41: only the gray (original) / only the label (processed) images are
  // encoded; the other kind's workgroups leave after taking their ticket (their images' output is
  // invalid). Splits the encoder's time by image kind.
  if ((dbg == 40 && d.render >= 0 && rd.kind == kRenderLabels) || (dbg == 41 && !(d.render >= 0 && rd.kind == kRenderLabels))) {
    if (part == 0x7FFFFFF1) out_sizes[0] = 1;
    return;
  }
  // Units (MCUs) per row: 16×16 (4:2:0) or 8×8 (4:4:4, gray) canvas pixels each.
  const int mcux = k420 ? out_w >> 4 : out_w >> 3;
  const Div16 dmx((uint32_t)mcux);
  // Scan block b → luma block column/row of the canvas.
  auto block_xy = [&](int bb, int& bx, int& by) {
    if (k420) {
      const int mcu = bb >> 2, sub = bb & 3;
      const int my = (int)dmx.q((uint32_t)mcu), mx = mcu - my * mcux;
      bx = 2 * mx + (sub & 1);
      by = 2 * my + (sub >> 1);
    } else {
      by = (int)dmx.q((uint32_t)bb);
      bx = bb - by * mcux;
    }
  };
  const int b = part * kWG + tid;
  const bool valid = b < bpi;
  // ---- 0. stage the source rows of this workgroup in LDS (workgroup-uniform decision) ----------
  int ys0 = 0, pcols = 0;
  bool staged = false, lstaged = false;
  // (A flat-label-workgroup shortcut — a workgroup whose label rows were all background or all
  // region filled its bit range with the repeating MCU pattern instead of coding — was removed in
  // round 5: its extra live state gave the kernel a 36-byte private segment, and the kernel without
  // it measured 105.2–105.8 vs 106.8–107.2 µs per 96-slice batch, profiles/r5/jpeg_flat/.)
  uint64_t* const slab = reinterpret_cast<uint64_t*>(spatch);  // label images reuse the area
  if (d.render >= 0 && rd.kind == kRenderLabels) {
    // Label render rows: 4by .. 4by+3 for the workgroup's block rows → 8 per MCU row (4:2:0).
    const int m0 = part * (kWG / kUnitBlocks), m1 = min(m0 + kWG / kUnitBlocks, bpi / kUnitBlocks) - 1;
    const int r0 = m0 / mcux, r1 = m1 / mcux;
    const int nrows = (kUnitRows / 2) * (r1 - r0 + 1), wpr = rd.wpr, nw = nrows * wpr;
    if (2 * nw * 2 <= kPatch) {  // two u64 planes in the f32 area
      lstaged = true;
      ys0 = (kUnitRows / 2) * r0;
      pcols = nw;  // offset of the border plane
      const Div16 dw((uint32_t)wpr);
      for (int i = tid; i < nw; i += kWG) {
        const int j = (int)dw.q((uint32_t)i), k = i - j * wpr;
        const size_t wi = (size_t)clampi(ys0 + j, 0, rd.src_h - 1) * wpr + k;
        slab[i] = rs.bits[rd.src_off + wi];
        slab[nw + i] = rs.bits[rd.border_off + wi];
      }
      __syncthreads();
    }
  }
  if (d.render >= 0 && rd.kind == kRenderRawGray) {
    const int m0 = part * (kWG / kUnitBlocks), m1 = min(m0 + kWG / kUnitBlocks, bpi / kUnitBlocks) - 1;
    const int r0 = m0 / mcux, r1 = m1 / mcux;
    const int nrows = (kUnitRows / 2) * (r1 - r0 + 1) + 2;
    pcols = swz_col(rd.src_w + 1) + 1;
    pcols += (4 - pcols % 8 + 8) % 8;  // row stride ≡ 4 (mod 8)
    if (nrows * pcols <= kPatch && !(rd.src_off & 1)) {
      staged = true;
      ys0 = (kUnitRows / 2) * r0 - 1;
      const int W = rd.src_w, H = rd.src_h, hw = W >> 1;  // W is a multiple of 8 (exact 2× fit)
      const uint16_t* src = rs.raw + rd.src_off;
      // Interior: 4-byte loads of pixel pairs, all issued before the LDS stores (one latency).
      const int nw = nrows * hw;
      const Div16 dh((uint32_t)hw);
      constexpr int kU = 12;  // ≥ 18 rows × 128 pairs / 256 threads for a 256² source: one round
      uint32_t v[kU];
#pragma unroll
      for (int t = 0; t < kU; ++t) {
        const int i = tid + t * kWG;
        v[t] = 0u;
        if (i < nw) {
          const int j = (int)dh.q((uint32_t)i), k = i - j * hw;
          v[t] = *reinterpret_cast<const uint32_t*>(src + (size_t)clampi(ys0 + j, 0, H - 1) * W + 2 * k);
        }
      }
      // rescaled_value(key_from_raw(r)) per staged pixel (pixel_math.h), without the key round
      // trip: the value is the low stored_bits bits of the sample, sign-extended for signed data —
      // one shift up and one arithmetic or logical shift down, selected as integers, then one
      // int → f32 conversion; the rescale only when the image has one (workgroup-uniform).
      // (Written with __builtin_amdgcn_sbfe / _ubfe and the select between the two conversions,
      // the compiler folded both into one unsigned conversion and signed slices rendered wrong:
      // profiles/r4/bfe_probe/, test_engine_norm_tables_vs_golden.)
      const bool sgn = rd.type == kI16, affine = rd.slope != 1.0f || rd.intercept != 0.0f;
      const uint32_t vsh = 32u - rd.stored_bits;
      auto value = [&](uint32_t r) {
        const uint32_t up = r << vsh;
        const int32_t xi = sgn ? (int32_t)up >> vsh : (int32_t)(up >> vsh);
        float x = (float)xi;
        if (affine) {
          const float t = x * rd.slope;
          x = t + rd.intercept;
        }
        return x;
      };
#pragma unroll
      for (int t = 0; t < kU; ++t) {
        const int i = tid + t * kWG;
        if (i < nw) {
          const int j = (int)dh.q((uint32_t)i), k = i - j * hw;
          spatch[j * pcols + swz_col(2 * k + 1)] = value(v[t] & 0xFFFFu);
          spatch[j * pcols + swz_col(2 * k + 2)] = value(v[t] >> 16);
        }
      }
      for (int i = tid + kU * kWG; i < nw; i += kWG) {  // larger footprints
        const int j = (int)dh.q((uint32_t)i), k = i - j * hw;
        const uint32_t u = *reinterpret_cast<const uint32_t*>(src + (size_t)clampi(ys0 + j, 0, H - 1) * W + 2 * k);
        spatch[j * pcols + swz_col(2 * k + 1)] = value(u & 0xFFFFu);
        spatch[j * pcols + swz_col(2 * k + 2)] = value(u >> 16);
      }
      // Clamped halo columns 0 and W+1.
      for (int i = tid; i < 2 * nrows; i += kWG) {
        const int j = i >> 1, right = i & 1;
        spatch[j * pcols + (right ? swz_col(W + 1) : 0)] =
            value(src[(size_t)clampi(ys0 + j, 0, H - 1) * W + (right ? W - 1 : 0)]);
      }
      __syncthreads();
    }
  }
  // ---- 1+2. block → DCT → quantisation fused with the AC Huffman coding ------------------------
  // The coefficients never leave registers: the zig-zag walk is unrolled, each coefficient is
  // quantised and — if non-zero in some lane of the wave (else the position is skipped) — coded
  // straight into the block's private bit buffer. The DC code depends on the previous block's DC,
  // so the AC stream is coded first and the DC code is prepended at assembly time.
  if (d.render >= 0 && rd.kind != kRenderLabels) win = render_window(rd, rs.stats);
  uint32_t* const pbuf = spriv + tid * kPrivWords;
  uint32_t* const pspill = w.spill + ((size_t)blockIdx.x * kWG + tid) * kSpillWords;
  int dc0 = 0;
  uint32_t acbits = 0;
  if (valid) {
    int bx, by;
    block_xy(b, bx, by);
    int32_t blk[64];
    // Label images are mostly background: when every block of the wave is one flat colour (76% of
    // the phantom cohort's label waves, 97.5% of its blocks) the islow FDCT of a constant block is
    // exactly DC = 64·x with every AC coefficient 0 (all butterfly differences vanish), so the
    // wave skips the FDCT, the quantisation and the zig-zag walk (wave-uniform branch).
    bool flat = false;
    if (dbg == 6) {  // profiling variant: no render
#pragma unroll
      for (int i = 0; i < 64; ++i) blk[i] = (i * 7 + bx + by) & 255;
    } else if (lstaged) {  // d.render ≥ 0: the fit is exactly 2× (render_is_exact_2x)
      const int wpr = rd.wpr;
      render_labels_exact2x(rd, [&](int y, int k, uint64_t& lab, uint64_t& brd) {
        const int i = (y - ys0) * wpr + k;
        lab = slab[i];
        brd = slab[pcols + i];
      }, bx, by, blk);
      bool same = true;
#pragma unroll
      for (int i = 1; i < 64; ++i) same = same && blk[i] == blk[0];  // 15 distinct cells after CSE
      flat = __ballot(!same) == 0;
    } else if (staged) {
      // Patch element (j, i) = source (4by-1+j, 4bx-1+i) = staged row 4by-1+j-ys0, column 4bx+i.
      // Patch column i = source column 4bx-1+i = staged column 4bx+i → swizzled 5bx + i + (i ≥ 4).
      const float* pp = spatch + (4 * by - 1 - ys0) * pcols + 5 * bx;
      auto fetch = [&](int j, int i) { return pp[j * pcols + i + (i >= 4 ? 1 : 0)]; };
      if (kNearest)  // --render-filter nearest: its own instance (launch_jpeg)
        render_patch_2x_nearest(fetch, win, blk);
      else
        render_patch_2x(fetch, win, blk);
    } else if (d.render >= 0) {
      render_block_2x<kNearest>(rd, rs.raw, rs.f32, rs.bits, win, bx, by, blk);
    } else {
      const uint8_t* src = canvas + d.canvas_off + (size_t)(by * 8) * out_w + bx * 8;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const uint2 v = *reinterpret_cast<const uint2*>(src + (size_t)r * out_w);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          blk[r * 8 + c] = (int32_t)((v.x >> (8 * c)) & 0xFF);
          blk[r * 8 + 4 + c] = (int32_t)((v.y >> (8 * c)) & 0xFF);
        }
      }
    }
    if (dbg == 1 || dbg == 6) {  // profiling variants: stop before the FDCT
      int acc = 0;
#pragma unroll
      for (int i = 0; i < 64; ++i) acc += blk[i] * (i + 1);
      if (acc == 0x7FFFFFF1) out_sizes[0] = 1;
      return;
    }
    LBitWriter lw(pbuf, pspill);
    int last = 0;
    if (flat) {
      dc0 = quant_recip(64 * (blk[0] - 128), q, 0);  // == fdct_islow's DC − 64·128 for a flat block
      if (dbg == 16) {  // profiling variant (below): every wave must stop here, or the look-back of
        // the flat waves would wait for records the stopped waves never publish
        if (dc0 == 0x7FFFFFF1) out_sizes[0] = 1;
        return;
      }
    } else {
      // Level shift (x − 128) folded into the DC term: the islow FDCT is linear and its only
      // rounding of the DC is a shift that divides the constant exactly, so fdct(x − 128) ==
      // fdct(x) with DC − 64·128 (checked for all-extreme and random blocks). Saves 64 VALU ops.
      // islow FDCT as 16-bit dot products (jpeg_common.h fdct_islow_dot): 63 fewer static VALU
      // instructions than the multiply/add form and no scratch spills (20 scratch instructions).
      fdct_islow_dot(blk);
      blk[0] -= 64 * 128;
      // Quantise into packed pairs first (frees the 64 int32 DCT registers), then walk the zig-zag
      // order from those registers. Sign-magnitude halves: |q| in bits 0–14 (16–30), the
      // coefficient's sign in bit 15 (31) — the coder needs |q| for the category and the sign only
      // to complement the magnitude bits, so the quotient is never negated back (|q| < 2^14: the
      // islow coefficients of 8-bit samples stay below 2^15 and every divisor is ≥ 2). Per pair:
      // 2 × (abs, add, mul_hi) + one byte permute for the signs + one bit-field insert.
      uint32_t zp[32];
#pragma unroll
      for (int k = 0; k < 64; k += 2) {
        const int32_t xa = blk[kNatural[k]], xc = blk[kNatural[k + 1]];
        const uint32_t mags = quant_mag(xa, q, kNatural[k]) | (quant_mag(xc, q, kNatural[k + 1]) << 16);
        const uint32_t signs = ((uint32_t)xa >> 16) | ((uint32_t)xc & 0xFFFF0000u);
        zp[k >> 1] = (mags & ~0x80008000u) | (signs & 0x80008000u);
      }
      {
        const int a0 = (int)(zp[0] & 0x7FFFu);
        dc0 = (zp[0] & 0x8000u) ? -a0 : a0;
      }
      if (dbg == 16) {  // profiling variant: stop after the FDCT and quantisation
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i) acc ^= zp[i] * (uint32_t)(2 * i + 1);
        if (acc == 0x7FFFFFF1u) out_sizes[0] = 1;
        return;
      }
      // Outer loop not unrolled: zp[j] is indexed by a wave-uniform counter (register indexing, no
      // scratch), keeping the code compact.
#pragma unroll 1
      for (int j = 0; j < 32; ++j) {
        const uint32_t word = zp[j];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = 2 * j + h;
          const uint32_t half = word >> (16 * h);
          const uint32_t av = half & 0x7FFFu;  // |q|; bit 15 of `half`: its sign
          if (k > 0 && __ballot(av != 0)) {
            if (av != 0) {
              int run = k - last - 1;
              while (run > 15) {
                lw.put_sym(actab[0xF0]);
                run -= 16;
              }
              const int nb = 32 - __builtin_clz(av);
              const uint32_t e = actab[(run << 4) + nb];  // symbol and magnitude in one put (≤ 27 bits)
              // Magnitude bits: q for q > 0, q − 1 = ~|q| for q < 0 (low nb bits).
              const uint32_t mag = (av ^ (0u - ((half >> 15) & 1u))) & ((1u << nb) - 1u);
              lw.put(((e & 0xFFFFu) << nb) | mag, (int)(e >> 16) + nb);
              last = k;
            }
          }
        }
      }
    }
    if (last < 63) lw.put_sym(actab[0x00]);
    if (kSamp == kSampling444 || (k420 && (b & 3) == 3)) {  // the MCU's Cb and Cr blocks of a gray image: DC diff 0 + EOB each
      lw.put_sym(kHuffDcChroma.e[0]);
      lw.put_sym(kHuffAcChroma.e[0]);
      lw.put_sym(kHuffDcChroma.e[0]);
      lw.put_sym(kHuffAcChroma.e[0]);
    }
    lw.finish();
    acbits = lw.bits;
  }
  if (dbg == 2) {  // profiling variant: stop after FDCT + quantisation + AC coding
    if (dc0 == 0x7FFFFFF1 || acbits == 0x7FFFFFF1u) out_sizes[0] = 1;
    return;
  }
  sdc[tid] = dc0;
  // DC of the block preceding this workgroup's first block (0 at the start of the image).
  if (tid < 64) {
    int dcp = 0;
    if (part > 0 && dbg != 17) {  // dbg 17: profiling variant without the predecessor's DC (output invalid)
      int pbx, pby;
      block_xy(part * kWG - 1, pbx, pby);
      const int u = 8 * pbx + (tid & 7);
      const int v = 8 * pby + (tid >> 3);
      const int px = d.render >= 0 ? (int)render_pixel(rd, rs.raw, rs.f32, rs.bits, win, u, v)
                                   : (int)canvas[d.canvas_off + (size_t)v * out_w + u];
      dcp = quant_recip(wave_sum_i32(px - 128), q, 0);
    }
    if (tid == 0) s_prevdc = dcp;
  }
  __syncthreads();
  // DC code (Huffman symbol + magnitude bits, ≤ 20 bits, right-aligned).
  const int diff = dc0 - (tid ? sdc[tid - 1] : s_prevdc);
  const int dn = mag_bits_fast(diff);
  const uint32_t dce = dctab[dn];
  const int dclen = valid ? (int)(dce >> 16) + dn : 0;
  const uint32_t dccode = ((dce & 0xFFFFu) << dn) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << dn) - 1u));
  // ---- 3–7. scan, bit range in LDS, look-back, stuffed bytes: jpeg_device.h (shared with k4_jpeg_rgb.hip)
  jpeg_emit_range<kWG, kUnion>(tid, img, part, parts, d, w, valid, dclen, dccode, acbits, pbuf, pspill, swg, out, out_sizes,
                               dbg);
}

bool render_is_exact_2x(const RenderDesc& r, int out_w, int out_h) {
  return r.invx == 0.5f && r.invy == 0.5f && r.ox == 0.0f && r.oy == 0.0f && 2 * r.src_w == out_w &&
         2 * r.src_h == out_h && (r.src_w % 4) == 0;
}

// Look-back bookkeeping of one encoder launch of `workgroups` workgroups (both encoders; jpeg_device.h).
void jpeg_look_begin(JpegWork& w, size_t workgroups, hipStream_t stream, const char* who) {
  if (w.look_base && w.look_base != 3 * w.look_cap) throw DeviceError(std::string(who) + ": look area state corrupt");
  if (workgroups > w.look_cap) throw DeviceError(std::string(who) + ": look-back capacity exceeded");
  w.look_used = workgroups;
  // The look-back records (3 words per workgroup) start unpublished. Eager launches alternate
  // between two halves of the look area, each launch clearing the half the previous one used
  // (stream order makes that safe); captured launches (hipGraph replay repeats the arguments)
  // clear their own half with a memset node instead.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(stream, &cap);
  const size_t words = workgroups * 3;
  if (cap != hipStreamCaptureStatusNone) {
    w.look_base = 0;
    w.clear_words = 0;
    check_hip(hipMemsetAsync(w.look, 0, words * sizeof(uint64_t), stream), "clear look-back");
  } else {
    const size_t half = 3 * w.look_cap;
    w.clear_base = w.look_base;
    w.clear_words = w.prev_words;
    w.look_base = w.look_base ? 0 : half;
    w.prev_words = words;
  }
}

void launch_jpeg(const uint8_t* canvas, const JpegDesc* jd, int ncanvas, int out_w, int out_h, const int32_t* div_luma,
                 JpegWork& w, uint8_t* out, int32_t* out_sizes, hipStream_t stream, const JpegRenderSrc* fused,
                 int sampling, bool nearest) {
  if (ncanvas <= 0) return;
  if (sampling < kSampling420 || sampling > kSamplingGray) throw DeviceError("launch_jpeg: unknown sampling");
  if (out_w % 16 || out_h % 16) throw DeviceError("GPU JPEG encoder needs canvas dims that are multiples of 16");
  if (!w.look || !w.ticket || !w.spill) throw DeviceError("launch_jpeg: JpegWork incomplete");
  QuantRecip q;
  for (int i = 0; i < 64; ++i) {
    const uint32_t dv = (uint32_t)div_luma[i];
    q.half[i] = dv >> 1;
    q.m[i] = (uint32_t)(((1ull << 32) + dv - 1) / dv);
  }
  JpegRenderSrc rs;
  if (fused) rs = *fused;
  const int bpi = (out_w / 8) * (out_h / 8);
  const int parts = (bpi + kJpegWG - 1) / kJpegWG;
  // NM03_PROFILE_VARIANT=jpeg=N selects truncated profiling variants (output invalid; time them
  // with rocprofv3 --kernel-trace --stats).
  static const int dbg = profile_variant("jpeg") & 0xFF;
  if (rs.rd && rs.nrd < ncanvas) throw DeviceError("launch_jpeg: fewer render descriptors than canvases");
  jpeg_look_begin(w, (size_t)parts * ncanvas, stream, "launch_jpeg");
  // Fused gray renders with --render-filter nearest have their own 4:2:0 instance; callers send the
  // other layouts' nearest renders through canvases (jpeg_fuses_nearest).
  if (nearest && sampling != kSampling420) throw DeviceError("launch_jpeg: fused nearest renders need 4:2:0");
  auto* kern = nearest                    ? &jpeg_fused_kernel<4, kUnionWords, kSampling420, true>
               : sampling == kSampling420 ? &jpeg_fused_kernel<4, kUnionWords, kSampling420, false>
               : sampling == kSampling444 ? &jpeg_fused_kernel<4, kUnionWords, kSampling444, false>
                                          : &jpeg_fused_kernel<4, kUnionWords, kSamplingGray, false>;
  kern<<<parts * ncanvas, kJpegWG, 0, stream>>>(canvas, jd, ncanvas, out_w, out_h, q, w, rs, out, out_sizes, dbg);
  check_launch("jpeg_fused_kernel");
}

void preload_kernels(bool with_volume) {
  // NM03_PRELOAD_TRACE=1: milliseconds per translation unit on stderr (what a cold start pays for
  // each code object).
  static const int trace = [] {
    const char* e = std::getenv("NM03_PRELOAD_TRACE");
    return e && *e ? std::atoi(e) : 0;  // 2: the same loads in reverse order (first-use cost vs size)
  }();
  auto t = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!trace) return;
    const auto n = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[nm03 preload] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  };
  if (trace == 2) {
    preload_render();
    lap("k3_render");
    preload_srg();
    lap("k2_srg_morph");
    preload_sharpen();
    lap("k1_sharpen");
  }
  preload_median();
  lap("k1_median");
  preload_sharpen();
  lap("k1_sharpen");
  preload_srg();
  lap("k2_srg_morph");
  preload_render();
  lap("k3_render");
  if (with_volume) {
    preload_volume();
    preload_threshold();
    lap("k5_volume+k6_threshold");
  }
  hipFuncAttributes a;
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&jpeg_fused_kernel<4, kUnionWords, kSampling420, false>)),
            "preload jpeg_fused_kernel");
  lap("k4_jpeg (first instance)");
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&jpeg_fused_kernel<4, kUnionWords, kSampling420, true>)),
            "preload jpeg_fused_kernel nearest");
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&jpeg_fused_kernel<4, kUnionWords, kSampling444, false>)),
            "preload jpeg_fused_kernel 4:4:4");
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&jpeg_fused_kernel<4, kUnionWords, kSamplingGray, false>)),
            "preload jpeg_fused_kernel gray");
  lap("k4_jpeg (other instances)");
}

}  // namespace nm03::gpu
