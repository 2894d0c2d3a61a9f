// Device code shared by the two JPEG encoders (k4_jpeg.hip: gray canvases and fused renders;
// k4_jpeg_rgb.hip: RGB canvases): reciprocal quantisation, the per-block Huffman bit buffers, and
// the second half of an encoder workgroup — workgroup scan of the block costs, the bit range
// assembled in LDS, its 0xFF-byte counts for all 8 alignments, the decoupled look-back over the
// image's earlier workgroups and the stuffed bytes written to host-mapped memory.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"
#include "nm03/gpu_types.h"
#include "nm03/jpeg_common.h"
#include "nm03/kernels.h"

namespace nm03::gpu {

using namespace nm03::jpeg;

// Host side, internal to the two encoder launchers (defined in k4_jpeg.hip): the look-back bookkeeping
// of one launch of `workgroups` workgroups on `stream` — capacity check, and which half of the look
// area the launch uses and which it clears. It advances JpegWork's private state: nothing else calls it.
// `who` names the launcher in errors.
void jpeg_look_begin(JpegWork& w, size_t workgroups, hipStream_t stream, const char* who);


struct QuantRecip {
  uint32_t half[64];  // d/2
  uint32_t m[64];     // ceil(2^32 / d)
};

__device__ __forceinline__ int mag_bits_fast(int v) {
  const unsigned a = (unsigned)(v < 0 ? -v : v);
  return a ? 32 - __builtin_clz(a) : 0;
}
__device__ __forceinline__ uint32_t hlen(uint32_t e) { return e >> 16; }

__device__ __forceinline__ int16_t quant_recip(int32_t x, const QuantRecip& q, int n) {
  const uint32_t a = (uint32_t)(x < 0 ? -x : x) + q.half[n];
  const int32_t v = (int32_t)__umulhi(a, q.m[n]);
  return (int16_t)(x < 0 ? -v : v);
}

// i / d for 0 ≤ i < 2^16 and 1 ≤ d < 2^16 as one multiply-high by m = ceil(2^32 / d): with
// e = m·d − 2^32 < d, i·m / 2^32 = i/d + i·e / (d·2^32), and the error term stays below
// 2^-16 ≤ 1/d, so it never carries i/d past the next integer. The divisors here (staged row
// widths, MCUs per row) are workgroup-uniform: m is computed once instead of the compiler's
// ≈10-instruction float-reciprocal division per use (24 per thread in the gray staging alone).
struct Div16 {
  uint32_t d, m;
  __device__ __forceinline__ explicit Div16(uint32_t dv) : d(dv), m(dv > 1u ? 0xFFFFFFFFu / dv + 1u : 0u) {}
  __device__ __forceinline__ uint32_t q(uint32_t i) const { return d > 1u ? __umulhi(i, m) : i; }
};

// |quantised x| (the same quotient as quant_recip, without the sign).
__device__ __forceinline__ uint32_t quant_mag(int32_t x, const QuantRecip& q, int n) {
  const uint32_t a = (uint32_t)(x < 0 ? -x : x) + q.half[n];
  return __umulhi(a, q.m[n]);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}


// Look-back records: 3 words per workgroup, each tagged in its top 2 bits (0 = not yet, 1 =
// aggregate, 2 = inclusive; word 0 is rewritten with the inclusive record). Cleared (memset)
// before every launch.
// Relaxed agent-scope atomics: the word itself carries the value, nothing else is published
// through it (the stage bits are consumed by later kernels), and acquire/release would add an L2
// writeback (buffer_wbl2) per store and an L2 invalidate (buffer_inv) per poll on gfx950.
__device__ __forceinline__ uint64_t look_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void look_store64(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// `n` ≤ 8 bits at bit offset `o` of an MSB-first word buffer (right-aligned). Reads word o/32 + 1:
// the buffer is zeroed one word past its end.
__device__ __forceinline__ uint32_t lds_bits(const uint32_t* buf, uint32_t o, uint32_t n) {
  if (n == 0) return 0u;
  const uint32_t w = o >> 5, sh = o & 31u;
  uint32_t v = buf[w] << sh;
  if (sh) v |= buf[w + 1] >> (32u - sh);
  return v >> (32u - n);
}
__device__ __forceinline__ uint32_t lds_byte(const uint32_t* buf, uint32_t o) { return lds_bits(buf, o, 8); }

constexpr int kJpegWG = 256;     // luma blocks (threads) per workgroup = 64 MCUs

constexpr int kPrivWords = 5;    // per-block Huffman bits kept in LDS (160 bits, odd stride) ...
constexpr int kSpillWords = 56;  // ... the rest in the block's global spill slot (a block needs ≤ 1700)

// MSB-first bit writer for one block: words [0, kPrivWords) go to LDS, later words (noisy,
// high-detail blocks only) to global memory. Counts every bit.
struct LBitWriter {
  uint32_t* buf;
  uint32_t* spill;
  uint32_t bits = 0;
  uint64_t acc = 0;
  int nacc = 0;
  __device__ LBitWriter(uint32_t* b, uint32_t* s) : buf(b), spill(s) {}
  __device__ __forceinline__ void store(uint32_t wi, uint32_t v) {
    if (wi < (uint32_t)kPrivWords)
      buf[wi] = v;
    else
      spill[wi - kPrivWords] = v;
  }
  // `code` must fit in `len` bits (Huffman codes do; magnitudes are masked by the caller).
  __device__ __forceinline__ void put(uint32_t code, int len) {
    acc = (acc << len) | (uint64_t)code;
    nacc += len;
    bits += (uint32_t)len;
    if (nacc >= 32) {
      store((bits - (uint32_t)nacc) >> 5, (uint32_t)(acc >> (nacc - 32)));
      nacc -= 32;
      acc &= (1ull << nacc) - 1ull;
    }
  }
  __device__ __forceinline__ void put_sym(uint32_t e) { put(e & 0xFFFFu, (int)(e >> 16)); }
  __device__ __forceinline__ void finish() {
    if (nacc > 0) store(bits >> 5, (uint32_t)(acc << (32 - nacc)));
  }
};
__device__ __forceinline__ uint32_t priv_word(const uint32_t* pb, const uint32_t* spill, uint32_t i) {
  return i < (uint32_t)kPrivWords ? pb[i] : spill[i - kPrivWords];
}

// Steps 3–7 of an encoder workgroup (k4_jpeg.hip's kernel comment): thread `tid` owns one coded
// block of `part` of image `img` — its DC code (`dclen` bits of `dccode`, right-aligned) and the
// `acbits` bits behind it in pbuf/pspill (LBitWriter) — in scan order. `swg`: kUnion words of LDS
// free for the bit range and the staged output. Called by every thread of the workgroup, after a
// barrier; returns with the workgroup's stuffed bytes stored (or the image flagged).
template <int kWG, int kUnion>
__device__ __forceinline__ void jpeg_emit_range(const int tid, const int img, const int part, const int parts,
                                                const JpegDesc& d, const JpegWork& w, const bool valid, const int dclen,
                                                const uint32_t dccode, const uint32_t acbits, const uint32_t* const pbuf,
                                                const uint32_t* const pspill, uint32_t* const swg,
                                                uint8_t* __restrict__ out, int32_t* __restrict__ out_sizes, const int dbg) {
  __shared__ uint32_t sh[17];
  __shared__ uint32_t sff[(kWG / 64) * 8];
  __shared__ uint32_t s_obase, s_nown, s_strad_v, s_fin_v, s_f, s_nwords;
  __shared__ bool s_bad, s_strad, s_fin;
  uint32_t agg = 0, nlocal = 0;
  bool in_lds = true;
  const uint32_t bits = valid ? (uint32_t)dclen + acbits : 0u;
  // ---- 3. workgroup scan, bit range assembled in LDS ----------------------------------------
  const uint32_t excl = block_exclusive_scan(bits, sh, &agg);  // ends with a barrier
  // Each block's DC code, then its AC words shifted behind it, into the workgroup's contiguous
  // bit range (MSB-first words), in the LDS region the render patch used. A range too long for
  // it (> ~220 Kbit: pathological detail) poisons the image, which the host then re-encodes.
  nlocal = (agg + 31) >> 5;
  in_lds = nlocal + 2u <= (uint32_t)kUnion;  // workgroup-uniform
  const uint32_t nwp = (acbits + 31) >> 5;
  const uint32_t acpos = excl + (uint32_t)dclen;
  if (in_lds) {
    for (uint32_t i = tid; i <= nlocal; i += kWG) swg[i] = 0u;
    __syncthreads();
    if (valid) {
      const uint32_t dv = dclen ? dccode << (32 - dclen) : 0u, sh0 = excl & 31u, w0 = excl >> 5;
      atomicOr(&swg[w0], dv >> sh0);
      if (sh0) atomicOr(&swg[w0 + 1], dv << (32u - sh0));
      const uint32_t shf = acpos & 31u, wa = acpos >> 5;
      for (uint32_t i = 0; i < nwp; ++i) {
        const uint32_t v = priv_word(pbuf, pspill, i);
        atomicOr(&swg[wa + i], v >> shf);
        if (shf) atomicOr(&swg[wa + i + 1], v << (32u - shf));
      }
    }
  }
  __syncthreads();
  // ---- 4. this workgroup's stuffing record -------------------------------------------------
  // Output byte k (bits 8k..8k+7 of the image's segment) belongs to the workgroup holding its
  // last bit; its offset in the stuffed output is k + (0xFF bytes before k). Whether a byte is
  // 0xFF depends on where the workgroup's range starts inside a byte (a = start mod 8), known only
  // after the look-back — so the record carries, for all eight alignments, the number of 0xFF
  // bytes lying wholly inside the range (ff[a]), plus its leading-ones count and last 7 bits
  // (the byte that straddles two workgroups). Successors then resolve any chain of aggregates.
  const uint32_t A = agg;
  uint32_t ffc[8];
#pragma unroll
  for (int al = 0; al < 8; ++al) ffc[al] = 0;
  if (in_lds) {
    // All eight alignments in one pass over the range's 32-bit words: bit q (MSB first) of
    // `r` says whether the 8 bits starting at range bit 32j + q are all ones (three shift-ANDs on
    // the word and the next one); a byte of alignment `al` starts at f + 8i, f = (8 − al) & 7, and
    // must end within the range (p + 8 ≤ A), so its count is popcount(r & (0x80808080 >> f)) over
    // the valid positions — instead of one LDS byte extraction per byte and alignment.
    const uint32_t nw = (A + 31u) >> 5;  // the range buffer has ≥ 2 words of slack (in_lds)
    for (uint32_t j = tid; j < nw; j += kWG) {
      const int32_t lim = (int32_t)A - 8 - 32 * (int32_t)j;  // last q whose byte fits in the range
      if (lim < 0) continue;
      const uint64_t v = ((uint64_t)swg[j] << 32) | swg[j + 1];
      uint64_t run = v & (v << 1);
      run &= run << 2;
      run &= run << 4;  // bit k: bits k .. k−7 of v all set
      uint32_t r = (uint32_t)(run >> 32);
      if (lim < 31) r &= ~((1u << (31 - lim)) - 1u);
#pragma unroll
      for (int al = 0; al < 8; ++al) ffc[al] += (uint32_t)__popc(r & (0x80808080u >> ((8 - al) & 7)));
    }
  }
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int al = 0; al < 8; ++al) ffc[al] = (uint32_t)wave_sum_i32((int)ffc[al]);
  if (lane == 0) {
#pragma unroll
    for (int al = 0; al < 8; ++al) sff[wv * 8 + al] = ffc[al];
  }
  __syncthreads();
  uint64_t* look = w.look + w.look_base + (size_t)img * parts * 3;
  if (tid < 64) {
    uint32_t ff[8];
#pragma unroll
    for (int al = 0; al < 8; ++al) {
      ff[al] = 0;
#pragma unroll
      for (int wq = 0; wq < kWG / 64; ++wq) ff[al] += sff[wq * 8 + al];
    }
    const uint32_t w0 = in_lds ? swg[0] : 0u;
    const uint32_t lead = ~w0 ? (uint32_t)__builtin_clz(~w0) : 32u;
    const uint32_t head = min(min(lead, 8u), A);  // leading ones of the range
    const uint32_t tail = in_lds && A >= 7 ? lds_bits(swg, A - 7, 7) : (in_lds ? lds_bits(swg, 0, A) : 0u);
    const bool poison = !in_lds || A >= (1u << 20) || ff[0] > 0x7FFFu;
    // ---- 5. publish the aggregate (3 words), then the decoupled look-back ----------------------
    if (lane == 0 && part < parts - 1) {
      look_store64(&look[3 * part + 1], (1ull << 62) | ((uint64_t)(ff[2] & 0x7FFF) << 45) |
                                            ((uint64_t)(ff[3] & 0x7FFF) << 30) | ((uint64_t)(ff[4] & 0x7FFF) << 15) |
                                            (uint64_t)(ff[5] & 0x7FFF));
      look_store64(&look[3 * part + 2], (1ull << 62) | ((uint64_t)(ff[6] & 0x7FFF) << 15) | (uint64_t)(ff[7] & 0x7FFF));
      look_store64(&look[3 * part], (1ull << 62) | ((uint64_t)poison << 61) | ((uint64_t)(A & 0xFFFFF) << 41) |
                                        ((uint64_t)tail << 34) | ((uint64_t)head << 30) |
                                        ((uint64_t)(ff[0] & 0x7FFF) << 15) | (uint64_t)(ff[1] & 0x7FFF));
    }
    // Lane l looks at part (hi − l): the nearest inclusive record ends the window; the aggregates
    // after it are resolved in order (their start bits are the inclusive end plus a suffix sum of
    // aggregate lengths, which fixes every alignment). Part −1 is an inclusive (0, 0) sentinel.
    uint32_t p_start = 0, ff_before = 0, tail_prev = 0;
    bool bad = poison;
    if (part > 0) {
      const int hi = part - 1;
      uint32_t spins = 0;
      uint64_t r0 = 0, r1 = 0, r2 = 0;
      int stop;
      for (;;) {
        const int q = hi - lane;
        uint32_t tag = 2;
        r0 = 2ull << 62;
        r1 = r2 = 0;
        if (q >= 0) {
          r0 = look_load(&look[3 * q]);
          tag = (uint32_t)(r0 >> 62);
          if (tag == 1u) {
            r1 = look_load(&look[3 * q + 1]);
            r2 = look_load(&look[3 * q + 2]);
            if ((r1 >> 62) != 1u || (r2 >> 62) != 1u) tag = 0;  // words land one by one
          }
        }
        const uint64_t incl = __ballot(tag == 2u);
        stop = incl ? __builtin_ctzll(incl) : 64;
        const uint64_t need = stop >= 63 ? ~0ull : ((2ull << stop) - 1ull);
        if ((__ballot(tag == 0u) & need) || stop == 64) {  // a needed record is not published yet
          if (++spins > (1u << 26)) {  // cannot happen with ordered tickets; never hang the GPU
            bad = true;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          continue;
        }
        break;
      }
      if (!bad) {
        const bool isagg = lane < stop;
        const uint32_t alen = isagg ? (uint32_t)(r0 >> 41) & 0xFFFFFu : 0u;
        uint32_t suf = alen;  // inclusive suffix sum over lanes l..63
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t t = (uint32_t)__shfl_down((int)suf, o, 64);
          if (lane + o < 64) suf += t;
        }
        // Inclusive record at lane `stop`: end bit, 0xFF count, last 7 bits.
        const uint32_t iend = (uint32_t)__shfl((int)((uint32_t)(r0 >> 39) & 0x3FFFFFu), stop, 64);
        const uint32_t iff = (uint32_t)__shfl((int)((uint32_t)(r0 >> 19) & 0xFFFFFu), stop, 64);
        const uint32_t mytail = isagg ? (uint32_t)(r0 >> 34) & 0x7Fu : (uint32_t)(r0 >> 12) & 0x7Fu;
        const uint32_t prevtail = (uint32_t)__shfl_down((int)mytail, 1, 64);  // part q − 1's last bits
        const uint32_t qstart = iend + (suf - alen);
        const uint32_t al = qstart & 7u;
        uint32_t fq = 0;
        if (isagg) {
          const uint32_t sel = al < 2 ? (uint32_t)(r0 >> (al ? 0 : 15)) : al < 6 ? (uint32_t)(r1 >> (15 * (5 - al)))
                                                                                : (uint32_t)(r2 >> (15 * (7 - al)));
          fq = sel & 0x7FFFu;
          const uint32_t hq = (uint32_t)(r0 >> 30) & 0xFu, m = (1u << al) - 1u;
          if (al && (prevtail & m) == m && hq >= 8u - al) ++fq;  // the straddling byte
        }
        const bool pois = __ballot(lane <= stop && ((r0 >> 61) & 1ull)) != 0;
        bad = bad || pois;
        ff_before = iff + (uint32_t)wave_sum_i32((int)fq);
        p_start = iend + (uint32_t)__shfl((int)suf, 0, 64);
        tail_prev = (uint32_t)__shfl((int)mytail, 0, 64);
      }
    }
    // ---- 6. own 0xFF count, inclusive record ---------------------------------------------------
    const uint32_t al = p_start & 7u, f = (8u - al) & 7u;
    const bool last = part == parts - 1;
    uint32_t own = 0, nown = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) own = al == (uint32_t)k ? ff[k] : own;  // select: ff stays in VGPRs (no scratch)
    bool strad = false, fin = false;
    uint32_t strad_v = 0, fin_v = 0;
    if (al) {  // the byte shared with the previous workgroup
      strad = true;
      const uint32_t take = min(8u - al, A);
      strad_v = ((tail_prev & ((1u << al) - 1u)) << (8u - al)) | (lds_bits(swg, 0, take) << (8u - al - take));
      if (take < 8u - al) strad_v |= (1u << (8u - al - take)) - 1u;  // final byte: pad with ones
      own += strad_v == 0xFFu;
    }
    const uint32_t nfull = A >= f ? (A - f) >> 3 : 0u;
    const uint32_t rem = A >= f ? A - f - 8u * nfull : 0u;
    if (last && rem) {  // the image's final partial byte, padded with 1-bits
      fin = true;
      fin_v = (lds_bits(swg, f + 8u * nfull, rem) << (8u - rem)) | ((1u << (8u - rem)) - 1u);
      own += fin_v == 0xFFu;
    }
    nown = (uint32_t)strad + nfull + (uint32_t)fin;
    const uint32_t end = p_start + A;
    bad = bad || end >= (1u << 22) || ff_before + own >= (1u << 20);
    const uint32_t obase = (p_start >> 3) + ff_before;
    // Exact end of this workgroup's stuffed bytes (own = its 0xFF count). It must be exact, not a
    // bound: a later workgroup that saw this one only as an aggregate never learns its flag, so the
    // flag has to follow from positions alone (ends are monotone along the image: once one
    // workgroup's end passes the capacity every later start does, and the last part reports -1).
    // A conservative 2 × nown bound let a workgroup drop its bytes while the image still reported
    // a size (tests/test_gpu.py::test_engine_jpeg_d2h_identical, capacity 20000).
    bad = bad || obase + nown + own > d.out_cap;
    if (lane == 0) {
      look_store64(&look[3 * part], (2ull << 62) | ((uint64_t)bad << 61) | ((uint64_t)(end & 0x3FFFFF) << 39) |
                                        ((uint64_t)((ff_before + own) & 0xFFFFF) << 19) |
                                        ((uint64_t)(in_lds ? (A >= 7 ? lds_bits(swg, A - 7, 7) : 0u) : 0u) << 12));
      s_bad = bad;
      s_obase = obase;
      s_nown = nown;
      s_strad = strad;
      s_fin = fin;
      s_strad_v = strad_v;
      s_fin_v = fin_v;
      s_f = f;
      s_nwords = nlocal + 2u;
      if (last) out_sizes[img] = bad ? -1 : (int32_t)(((end + 7u) >> 3) + ff_before + own);
    }
  }
  __syncthreads();
  if (dbg == 4 || s_bad) return;
  // ---- 7. stuffed bytes straight into the host-mapped output --------------------------------
  // Thread t takes a contiguous run of the owned bytes; a block scan of (bytes + 0xFF count) gives
  // every run its output position; the stuffed bytes are staged in LDS behind the bit range and
  // copied out with consecutive lanes on consecutive bytes.
  const uint32_t nown = s_nown, f = s_f, hs = s_strad ? 1u : 0u;
  const uint32_t per = (nown + kWG - 1) / kWG;
  const uint32_t j0 = min(nown, tid * per), j1 = min(nown, j0 + per);
  auto owned = [&](uint32_t j) -> uint32_t {
    if (j < hs) return s_strad_v;
    const uint32_t i = j - hs;
    const uint32_t nfull = nown - hs - (s_fin ? 1u : 0u);
    return i < nfull ? lds_byte(swg, f + 8u * i) : s_fin_v;
  };
  uint32_t cnt = 0;
  for (uint32_t j = j0; j < j1; ++j) cnt += owned(j) == 0xFFu ? 2u : 1u;
  uint32_t tot = 0;
  uint32_t o = block_exclusive_scan(cnt, sh, &tot);
  uint8_t* dst = out + d.out_off + s_obase;
  // Staged bytes sit at the destination's 16-byte phase behind the bit range, so 16-byte chunks of
  // the output are 16-byte chunks of LDS (one ds_read_b128 + one dwordx4 host store per lane).
  const uint32_t phase = (uint32_t)((uintptr_t)dst & 15u);
  uint8_t* sbuf = reinterpret_cast<uint8_t*>(swg + ((s_nwords + 3u) & ~3u)) + phase;  // behind the bit range
  const bool staged_out = tot + phase <= (uint32_t)(kUnion - ((s_nwords + 3u) & ~3u)) * 4u;
  for (uint32_t j = j0; j < j1; ++j) {
    const uint32_t v = owned(j);
    if (staged_out) {
      sbuf[o++] = (uint8_t)v;
      if (v == 0xFFu) sbuf[o++] = 0;
    } else {
      dst[o++] = (uint8_t)v;
      if (v == 0xFFu) dst[o++] = 0;
    }
  }
  if (staged_out) {
    __syncthreads();
    if (dbg == 15) {  // profiling variant: staged, not stored
      if (tot == 0x7FFFFFF1u) out_sizes[0] = sbuf[tid];
      return;
    }
    // Chunk c covers destination bytes [16c − phase, 16c + 16 − phase) of the range; the first and
    // last chunks may be partial (byte stores), the rest move whole.
    const uint32_t nchunks = (phase + tot + 15u) >> 4;
    uint8_t* const dbase = dst - phase;  // 16-byte aligned
    const uint8_t* const lbase = sbuf - phase;
    for (uint32_t c = tid; c < nchunks; c += kWG) {
      const uint32_t b0 = 16u * c, lo = max(b0, phase), hi = min(b0 + 16u, phase + tot);
      if (lo == b0 && hi == b0 + 16u) {
        // Non-temporal: the bytes go to host memory over PCIe and are never read back on the GPU.
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(lbase + b0), reinterpret_cast<u32x4*>(dbase + b0));
      } else {
        for (uint32_t k = lo; k < hi; ++k) dbase[k] = lbase[k];
      }
    }
  }
}

}  // namespace nm03::gpu
