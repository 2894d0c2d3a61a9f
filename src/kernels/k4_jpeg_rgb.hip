// K4-RGB — true-colour JPEG export on the GPU (the --overlay output): an interleaved RGB canvas in
// device memory → the entropy-coded segment of a YCbCr 4:2:0 or 4:4:4 file, byte-identical to
// libjpeg(-turbo) (golden encoder jpeg::encode_scan_rgb; tests/test_jpeg_rgb.py vs Pillow).
//
// One launch per batch, the structure of k4_jpeg.hip: a workgroup per run of MCUs of an image, a
// thread per coded 8×8 block in scan order (4:2:0: Y00 Y01 Y10 Y11 Cb Cr per MCU; 4:4:4: Y Cb Cr),
// tickets, workgroup scan, bit range in LDS, decoupled look-back and the stuffed bytes into
// host-mapped memory (jpeg_device.h, shared with the gray encoder).
//
// Workgroup shape. 256 threads, as the gray encoder, coding 42 MCUs (252 blocks) of a 4:2:0 image or
// 85 MCUs (255 blocks) of a 4:4:4 one; the last 4 (1) threads idle. An MCU carries 6 (3) coded
// blocks against the gray encoder's 4 (1) with luma detail, so the per-block bit buffers are what
// grows with colour: at 256 blocks per workgroup they stay exactly the gray encoder's 5 KiB, and
// the LDS is 36.4 KiB (2 KiB of Huffman tables for two components instead of one, 1 KiB of
// quantisation reciprocals, which the lanes of a wave pick by component; the 27 KiB union holds
// first the converted samples — 42 × 384 B or 85 × 192 B ≈ 16 KiB — then the bit range). With
// ≤ 128 VGPRs (113 / 110, no scratch) a SIMD holds 4 waves, a CU 4 such workgroups, 146 of its 160 KiB LDS:
// the occupancy point the gray encoder was tuned at. 64 MCUs per workgroup (384 threads, 6 waves)
// would leave room for only 2 workgroups per CU (12 of 16 wave slots); 32 MCUs (192 threads) fit 5
// but pay the per-workgroup costs (tables, ticket, look-back) twice as often for the same LDS.
// MCU runs are not aligned to MCU rows (42 and 85 divide no canvas width used here), so nearly every
// workgroup starts mid-row and needs its predecessor MCU's last Y, Cb and Cr DC values: three waves
// recompute them from the predecessor's pixels (DC = quantised Σ(x − 128), one sample per lane), as
// the gray encoder's wave 0 does for its one luma predecessor. Nothing is serial across workgroups
// but the look-back.
//
// Cost, and a supposition about it. Per canvas this encoder measured 1.9× the gray encoder for 1.5×
// the coded blocks (docs/ARCHITECTURE.md §6). None of its waves are flat label waves, which is one
// reason; two access patterns here are likely the rest, though no counter run backs it: the 4:2:0
// conversion reads each 2×2 quad with 12 single-byte global loads at a 6-byte stride across lanes
// (the 4:4:4 one 3 at a 3-byte stride), and a thread fetches its 64-byte block from LDS with four
// 16-byte reads at a 64-byte stride across lanes, which lands the lanes of a wave on few banks.
// Wider loads of whole pixel rows and a padded block pitch are the things to try first, with
// counters, if this export becomes a default.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "jpeg_device.h"
#include "nm03/gpu_types.h"
#include "nm03/jpeg_common.h"
#include "nm03/kernels.h"

namespace nm03::gpu {

using namespace nm03::jpeg;

constexpr int kRgbUnionWords = 6912;  // 27 KiB: converted samples, then bit range + staged output (as k4_jpeg.hip)

constexpr int rgb_blocks_per_mcu(int samp) { return samp == kSampling420 ? 6 : 3; }
constexpr int rgb_mcus_per_wg(int samp) { return kJpegWG / rgb_blocks_per_mcu(samp); }

template <int kSamp>
__global__ __launch_bounds__(kJpegWG) __attribute__((amdgpu_waves_per_eu(4))) void jpeg_rgb_kernel(
    const uint8_t* __restrict__ canvas, const JpegDesc* __restrict__ jd, int ncanvas, int out_w, int out_h, QuantRecip ql,
    QuantRecip qc, JpegWork w, uint8_t* __restrict__ out, int32_t* __restrict__ out_sizes) {
  constexpr int kWG = kJpegWG;
  constexpr bool k420 = kSamp == kSampling420;
  constexpr int kBlk = rgb_blocks_per_mcu(kSamp), kMcuWG = rgb_mcus_per_wg(kSamp);
  constexpr int kMcuPx = k420 ? 16 : 8;  // MCU side in canvas pixels
  constexpr int kUnion = kRgbUnionWords;
  static_assert(kMcuWG * kBlk * 64 <= kUnion * 4, "converted samples exceed the LDS union");
  __shared__ uint32_t actab[2][256];
  __shared__ uint32_t dctab[2][16];
  __shared__ uint2 sq[2][64];  // (d/2, ceil(2^32 / d)) per component and coefficient
  __shared__ int32_t sdc[kWG];
  __shared__ uint32_t spriv[kWG * kPrivWords];  // per-block AC Huffman bits
  __shared__ uint32_t s_ticket;
  __shared__ int32_t s_prevdc[3];
  __shared__ __attribute__((aligned(16))) uint32_t sunion[kUnion];
  uint8_t* const samples = reinterpret_cast<uint8_t*>(sunion);  // block-major: 64 bytes per coded block
  const int tid = threadIdx.x;
  // Records of the previous launch (the other half of the look area) are dead: clear them here.
  if (w.clear_words) {
    uint64_t* other = w.look + w.clear_base;
    for (size_t i = (size_t)blockIdx.x * kWG + tid; i < w.clear_words; i += (size_t)gridDim.x * kWG) other[i] = 0ull;
  }
  const int mcux = out_w / kMcuPx, nmcu = mcux * (out_h / kMcuPx);
  const int parts = (nmcu + kMcuWG - 1) / kMcuWG;
  // Images dealt round-robin over the dispatch order, the part from the image's ticket counter
  // (ordered tickets: a workgroup only waits on parts that have already started), as in k4_jpeg.hip.
  const int img = (int)(blockIdx.x % (uint32_t)ncanvas);
  uint32_t ticket = 0;
  if (tid == 0) {
    auto* tp = (__attribute__((address_space(1))) uint32_t*)&w.ticket[img];
    asm volatile("" : "+v"(tp));
    ticket = __hip_atomic_fetch_add(tp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  actab[0][tid] = kHuffAcLuma.e[tid];
  actab[1][tid] = kHuffAcChroma.e[tid];
  if (tid < 32) dctab[tid >> 4][tid & 15] = (tid & 15) < 12 ? (tid < 16 ? kHuffDcLuma.e[tid] : kHuffDcChroma.e[tid & 15]) : 0u;
  // Waves 0 and 1 spread the luma / chroma reciprocals (kernel arguments: scalar registers) over
  // their lanes with constant indices — a lane-indexed read would copy the tables to scratch.
  auto spread = [&](const QuantRecip& q, int c) {
    const int lane = tid & 63;
    uint32_t hv = 0, mv = 0;
#pragma unroll
    for (int n = 0; n < 64; ++n) {
      hv = lane == n ? q.half[n] : hv;
      mv = lane == n ? q.m[n] : mv;
    }
    sq[c][lane] = make_uint2(hv, mv);
  };
  if (tid < 64)
    spread(ql, 0);
  else if (tid < 128)
    spread(qc, 1);
  const JpegDesc d = jd[img];
  if (tid == 0) {
    if (ticket == (uint32_t)parts - 1) atomicExch(&w.ticket[img], 0u);  // the image's last ticket
    s_ticket = ticket;
  }
  __syncthreads();
  const int part = (int)__builtin_amdgcn_readfirstlane(s_ticket);
  const Div16 dmx((uint32_t)mcux);
  const int g0 = part * kMcuWG;                  // first MCU of this workgroup
  const int nm = min(kMcuWG, nmcu - g0);         // its MCUs
  const uint8_t* const src = canvas + d.canvas_off;
  const size_t pitch = (size_t)out_w * 3;
  // ---- 0. colour conversion (and, 4:2:0, the 2×2 chroma mean) of the workgroup's MCUs into LDS ----
  if (k420) {
    // One 2×2 pixel quad per step: 4 luma samples and one Cb / Cr sample each.
    for (int i = tid; i < nm * 64; i += kWG) {
      const int m = i >> 6, qy = (i >> 3) & 7, qx = i & 7;
      const int g = g0 + m, my = (int)dmx.q((uint32_t)g), mx = g - my * mcux;
      const uint8_t* p = src + (size_t)(16 * my + 2 * qy) * pitch + (size_t)(16 * mx + 2 * qx) * 3;
      int cb[4], cr[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint8_t* q = p + (k >> 1) * pitch + (k & 1) * 3;
        const int r = q[0], gg = q[1], b = q[2];
        const int px = 2 * qx + (k & 1), py = 2 * qy + (k >> 1);
        samples[(m * 6 + (py >> 3) * 2 + (px >> 3)) * 64 + (py & 7) * 8 + (px & 7)] = (uint8_t)rgb_to_y(r, gg, b);
        cb[k] = rgb_to_cb(r, gg, b);
        cr[k] = rgb_to_cr(r, gg, b);
      }
      // The image's chroma column is 8·mx + qx: its parity is qx's.
      samples[(m * 6 + 4) * 64 + qy * 8 + qx] = (uint8_t)h2v2_sample(cb[0], cb[1], cb[2], cb[3], qx);
      samples[(m * 6 + 5) * 64 + qy * 8 + qx] = (uint8_t)h2v2_sample(cr[0], cr[1], cr[2], cr[3], qx);
    }
  } else {
    for (int i = tid; i < nm * 64; i += kWG) {
      const int m = i >> 6, py = (i >> 3) & 7, px = i & 7;
      const int g = g0 + m, my = (int)dmx.q((uint32_t)g), mx = g - my * mcux;
      const uint8_t* q = src + (size_t)(8 * my + py) * pitch + (size_t)(8 * mx + px) * 3;
      const int r = q[0], gg = q[1], b = q[2];
      samples[(m * 3 + 0) * 64 + (i & 63)] = (uint8_t)rgb_to_y(r, gg, b);
      samples[(m * 3 + 1) * 64 + (i & 63)] = (uint8_t)rgb_to_cb(r, gg, b);
      samples[(m * 3 + 2) * 64 + (i & 63)] = (uint8_t)rgb_to_cr(r, gg, b);
    }
  }
  __syncthreads();
  // ---- 1+2. block → FDCT → quantisation fused with the AC Huffman coding (as k4_jpeg.hip) --------
  const int m = tid / kBlk, k = tid - m * kBlk;     // MCU of the workgroup, block of the MCU
  const int comp = k420 ? (k < 4 ? 0 : k - 3) : k;  // 0 Y, 1 Cb, 2 Cr
  const bool chroma = comp != 0;
  const bool valid = m < nm;  // also false for the threads past the last whole MCU (m == kMcuWG)
  const uint32_t* const act = actab[chroma ? 1 : 0];
  uint32_t* const pbuf = spriv + tid * kPrivWords;
  uint32_t* const pspill = w.spill + ((size_t)blockIdx.x * kWG + tid) * kSpillWords;
  int dc0 = 0;
  uint32_t acbits = 0;
  if (valid) {
    int32_t blk[64];
    const uint4* sp = reinterpret_cast<const uint4*>(samples + tid * 64);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint4 v = sp[r];
      const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int c = 0; c < 16; ++c) blk[r * 16 + c] = (int32_t)((wv[c >> 2] >> (8 * (c & 3))) & 0xFFu);
    }
    LBitWriter lw(pbuf, pspill);
    int last = 0;
    // Level shift folded into the DC term; packed sign-magnitude pairs in zig-zag order; positions
    // that are zero in every lane of the wave are skipped (see k4_jpeg.hip for the derivations).
    fdct_islow_dot(blk);
    blk[0] -= 64 * 128;
    // The component's reciprocals come from LDS (sq, one ds_read_b64 per coefficient at a per-lane
    // base): a wave holds luma and chroma blocks side by side (scan order), so the gray encoder's
    // scalar operands would need a per-lane select between the two tables (120 bytes of scratch) or
    // a divergent branch per table (16 bytes, and the quantisation twice per wave).
    uint32_t zp[32];
    const uint2* const qt = sq[chroma ? 1 : 0];
    auto qmag = [&](int32_t x, int n) {
      const uint2 hm = qt[n];  // (d/2, ceil(2^32 / d))
      return __umulhi((uint32_t)(x < 0 ? -x : x) + hm.x, hm.y);
    };
#pragma unroll
    for (int j = 0; j < 64; j += 2) {
      const int32_t xa = blk[kNatural[j]], xc = blk[kNatural[j + 1]];
      const uint32_t mags = qmag(xa, kNatural[j]) | (qmag(xc, kNatural[j + 1]) << 16);
      const uint32_t signs = ((uint32_t)xa >> 16) | ((uint32_t)xc & 0xFFFF0000u);
      zp[j >> 1] = (mags & ~0x80008000u) | (signs & 0x80008000u);
    }
    {
      const int a0 = (int)(zp[0] & 0x7FFFu);
      dc0 = (zp[0] & 0x8000u) ? -a0 : a0;
    }
#pragma unroll 1
    for (int j = 0; j < 32; ++j) {
      const uint32_t word = zp[j];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int kk = 2 * j + h;
        const uint32_t half = word >> (16 * h);
        const uint32_t av = half & 0x7FFFu;  // |q|; bit 15 of `half`: its sign
        if (kk > 0 && __ballot(av != 0)) {
          if (av != 0) {
            int run = kk - last - 1;
            while (run > 15) {
              lw.put_sym(act[0xF0]);
              run -= 16;
            }
            const int nb = 32 - __builtin_clz(av);
            const uint32_t e = act[(run << 4) + nb];
            const uint32_t mag = (av ^ (0u - ((half >> 15) & 1u))) & ((1u << nb) - 1u);
            lw.put(((e & 0xFFFFu) << nb) | mag, (int)(e >> 16) + nb);
            last = kk;
          }
        }
      }
    }
    if (last < 63) lw.put_sym(act[0x00]);
    lw.finish();
    acbits = lw.bits;
  }
  sdc[tid] = dc0;
  // Last Y, Cb and Cr DC of the MCU preceding this workgroup's first one (0 at the start of the
  // image): wave c recomputes component c's block of that MCU, one sample per lane.
  if (tid < 192) {
    const int c = tid >> 6, lane = tid & 63, sx = lane & 7, sy = lane >> 3;
    int dcp = 0;
    if (part > 0) {
      const int g = g0 - 1, my = (int)dmx.q((uint32_t)g), mx = g - my * mcux;
      int s;
      if (k420 && c > 0) {
        const uint8_t* p = src + (size_t)(16 * my + 2 * sy) * pitch + (size_t)(16 * mx + 2 * sx) * 3;
        int v[4];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const uint8_t* q = p + (q4 >> 1) * pitch + (q4 & 1) * 3;
          v[q4] = c == 1 ? rgb_to_cb(q[0], q[1], q[2]) : rgb_to_cr(q[0], q[1], q[2]);
        }
        s = h2v2_sample(v[0], v[1], v[2], v[3], sx);
      } else {
        // 4:2:0 luma: Y11, the MCU's lower right block.
        const int x = kMcuPx * mx + (k420 ? 8 : 0) + sx, y = kMcuPx * my + (k420 ? 8 : 0) + sy;
        const uint8_t* q = src + (size_t)y * pitch + (size_t)x * 3;
        s = c == 0 ? rgb_to_y(q[0], q[1], q[2]) : c == 1 ? rgb_to_cb(q[0], q[1], q[2]) : rgb_to_cr(q[0], q[1], q[2]);
      }
      const int sum = wave_sum_i32(s - 128);
      dcp = c == 0 ? quant_recip(sum, ql, 0) : quant_recip(sum, qc, 0);
    }
    if (lane == 0) s_prevdc[c] = dcp;
  }
  __syncthreads();
  // DC code against the previous block of the same component: the preceding thread inside an MCU's
  // luma blocks, else the same component's last block of the preceding MCU (kBlk threads back, 3 for
  // Y00 ← Y11), else the recomputed predecessor.
  int prev;
  if (k420 && k >= 1 && k <= 3)
    prev = sdc[tid - 1];
  else if (m > 0)
    prev = sdc[tid - ((k420 && k == 0) ? 3 : kBlk)];
  else
    prev = s_prevdc[comp];
  const int diff = dc0 - prev;
  const int dn = mag_bits_fast(diff);
  const uint32_t dce = dctab[chroma ? 1 : 0][dn];
  const int dclen = valid ? (int)(dce >> 16) + dn : 0;
  const uint32_t dccode = ((dce & 0xFFFFu) << dn) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << dn) - 1u));
  // ---- 3–7. scan, bit range, look-back, stuffed bytes (jpeg_device.h) ---------------------------
  jpeg_emit_range<kWG, kUnion>(tid, img, part, parts, d, w, valid, dclen, dccode, acbits, pbuf, pspill, sunion, out,
                               out_sizes, 0);
}

size_t jpeg_rgb_parts(int out_w, int out_h, int sampling) {
  const int px = sampling == kSampling420 ? 16 : 8;
  const int nmcu = (out_w / px) * (out_h / px), per = rgb_mcus_per_wg(sampling);
  return (size_t)(nmcu + per - 1) / per;
}

void launch_jpeg_rgb(const uint8_t* canvas, const JpegDesc* jd, int ncanvas, int out_w, int out_h, const int32_t* div_luma,
                     const int32_t* div_chroma, JpegWork& w, uint8_t* out, int32_t* out_sizes, hipStream_t stream,
                     int sampling) {
  if (ncanvas <= 0) return;
  if (sampling != kSampling420 && sampling != kSampling444) throw DeviceError("launch_jpeg_rgb: a colour image needs 4:2:0 or 4:4:4");
  if (out_w <= 0 || out_h <= 0 || out_w % 16 || out_h % 16)
    throw DeviceError("GPU JPEG encoder needs canvas dims that are multiples of 16");
  if (!w.look || !w.ticket || !w.spill) throw DeviceError("launch_jpeg_rgb: JpegWork incomplete");
  QuantRecip q[2];
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 64; ++i) {
      const uint32_t dv = (uint32_t)(c ? div_chroma : div_luma)[i];
      q[c].half[i] = dv >> 1;
      q[c].m[i] = (uint32_t)(((1ull << 32) + dv - 1) / dv);
    }
  const size_t parts = jpeg_rgb_parts(out_w, out_h, sampling);
  jpeg_look_begin(w, parts * (size_t)ncanvas, stream, "launch_jpeg_rgb");
  auto* kern = sampling == kSampling420 ? &jpeg_rgb_kernel<kSampling420> : &jpeg_rgb_kernel<kSampling444>;
  kern<<<(unsigned)(parts * ncanvas), kJpegWG, 0, stream>>>(canvas, jd, ncanvas, out_w, out_h, q[0], q[1], w, out, out_sizes);
  check_launch("jpeg_rgb_kernel");
}

void preload_jpeg_rgb() {
  hipFuncAttributes a;
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&jpeg_rgb_kernel<kSampling420>)),
            "preload jpeg_rgb_kernel 4:2:0");
  check_hip(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&jpeg_rgb_kernel<kSampling444>)),
            "preload jpeg_rgb_kernel 4:4:4");
}

}  // namespace nm03::gpu
