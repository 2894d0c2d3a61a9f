"""Inputs of the JPEG stream tests (CPU: test_jpeg_stream_cases.py, GPU: test_gpu_jpeg_streams.py; not
a conftest), and a baseline scan walker that says which branches of the encoders a stream takes.

Everything here is NumPy and plain Python on the CPU. The builders are deterministic; every parameter
that a search found (the amplitudes below) is a stored literal, found against the golden encoder
(native.jpeg_encode_gray / native.jpeg_encode_rgb), and test_jpeg_stream_cases.py re-establishes on
every run that each case still meets its condition — and that the golden bytes are libjpeg's. Two
colour images that only a long search finds (a part over the range limit) are data under tests/golden/.

What the cases reach (walker figures of the golden encoder's streams at gray sampling unless named,
all equal to Pillow's; part lengths in bits, `al` = a part's start bit mod 8, `ff` = share of 0xFF
bytes before stuffing; test_jpeg_stream_cases.py prints them all with -s):

  sparse_hf_a / _b 48×80 q50     ZRL symbols per block {1: 7, 2: 13, 3: 40} / {1: 6, 2: 14, 3: 40}; 5 / 2
                                 blocks without EOB; largest block 58 bits; ff 15.6 % / 13.5 %; one part of
                                 2970 / 2958 bits
  sparse_hf 272×400 q50          ZRL per block {1: 196, 2: 502, 3: 1002} (4206 symbols in 1700 blocks), 60
                                 blocks without EOB, ff 14.1 %, 7 parts of 12 160–12 503 bits (the last 7855),
                                 al 0 6 2 3 3 1 0 (4:2:0: 0 0 4 2 5 3 1)
  dc_checker(_shifted) 128×256   q100: DC category 11, diff ±2040 in every block but the first, 24 bits a
                                 block; block 256 (part 1's first) takes −2040 (+2040 shifted); ff 33.3 % (0 %)
  binary_noise 48×80 q100        AC category 10, largest block 982 bits (26 spill words), no EOB at all
  uniform_noise 128×128 q100     one part of 204 260 bits: under the range limit (221 120)
  binary_noise 128×128 q100      one part of 239 000 bits: over it (largest block 991 bits)
  flat_levels q10/50/90/100      DC divisors 80 / 16 / 3 / 1; q50: 128 exact halves, 64 of them negative
  straddle(al), al 1..7          parts [1639..1697, 1673]; part 1 at alignment al, its first byte 0xFF
  straddle3(al), al 1..7         three parts; part 1 at al and part 2 at al + 1, both on a 0xFF byte (al 7:
                                 part 2 is byte-aligned)
  final(rem), rem 1..7           the padded last byte 0xFF with rem stream bits in it
  rgb_sparse_hf 48×80, 64×256    q50, 4:2:0 / 4:4:4: one to three ZRL symbols a block in Y, Cb and Cr, 5–63
                                 blocks without EOB, ff 6–13 %; 64×256: 2 / 4 parts (al 0 3 / 0 5 6 3)
  rgb_binary_noise 48×80 q100    AC category 9, largest block 888 / 884 bits
  rgb_dc_checker 64×256 q100     Y, Cb and Cr DC category 11 (Cb and Cr diffs of ±2040)
  rgb_straddle / rgb_final       part 1 at alignment 2 on a 0xFF byte (behind a Cr block without EOB); the
                                 padded last byte 0xFF with 2 stream bits
  rgb_over_limit (tests/golden/) q100: part 0 of 223 491 bits at 4:2:0 and 222 132 at 4:4:4, over the range
                                 limit; found by search (the colour section below says how), since colour
                                 noise stays under it (207 447 bits at the most)

Against the figures first measured on Pillow's streams for these builders (another seed, so near but not
equal): sparse_hf 272×400 — about 4200 ZRL symbols, about 65 blocks without EOB, 14 % 0xFF: here 4206, 60
and 14.1 %; a binary_noise block of 996 bits: here 982 (48×80) and 991 (128×128); one part of binary noise
238 998 bits: here 239 000; uniform noise about 205 000: here 204 260. The edge amplitudes (EDGE_A and the
two tables of a) came out the same on the golden encoder as on Pillow.

Why a gray image at 4:2:0 or 4:4:4 cannot straddle: each of its MCUs ends in the two all-zero chroma
blocks, `00 00 00 00` (DC difference 0 and EOB are `00` each in the chroma tables), so the byte across
a part edge, and the padded last byte, hold zero bits and are never 0xFF. Those samplings still take
every case for byte equality.
"""
import os

import numpy as np

# ---- the kernels' part sizes (src/kernels/jpeg_device.h, k4_jpeg.hip, k4_jpeg_rgb.hip) --------------
K_JPEG_WG = 256                       # kJpegWG: coded blocks (threads) per workgroup
K_UNION_WORDS = 6912                  # kUnionWords = kRgbUnionWords: LDS words of the bit range
RANGE_LIMIT_BITS = (K_UNION_WORDS - 2) * 32   # in_lds = nlocal + 2 <= kUnion: 221 120 bits
GRAY_OUT_CAP = 512 * 1024             # ops.jpeg_encode's bytes per image


def gray_mcus_per_part(luma_blocks_per_mcu):
    """The gray encoder (k4_jpeg.hip) gives a workgroup kJpegWG luma blocks: 64 MCUs at 4:2:0, 256
    at 4:4:4 and gray (the all-zero chroma blocks ride on their MCU's last luma thread)."""
    return K_JPEG_WG // luma_blocks_per_mcu


def rgb_mcus_per_part(blocks_per_mcu):
    """The colour encoder (k4_jpeg_rgb.hip, rgb_mcus_per_wg) gives a workgroup kJpegWG / 6 = 42 MCUs
    at 4:2:0 and kJpegWG / 3 = 85 at 4:4:4: a thread per coded block, whole MCUs only."""
    return K_JPEG_WG // blocks_per_mcu


# ---- the walker -------------------------------------------------------------------------------------
class Stream:
    """One walked scan. Per coded block, in scan order: `pos` (bit position in the unstuffed stream),
    `bits`, `comp` (index into the frame's components), `zrl` (ZRL symbols), `dc_cat`, `dc_diff`,
    `ac_cat` (largest), `eob` (False: the block ends on coefficient 63). Per image: `total_bits`,
    `unstuffed` (bytes), `segment` (the stuffed bytes as found), `ff_bytes`, `blocks_per_mcu`,
    `luma_blocks_per_mcu`, `mcus`, `quant` ({table id: 64 divisors in zig-zag order})."""

    def zrl_histogram(self):
        h = {}
        for z in self.zrl:
            h[z] = h.get(z, 0) + 1
        return dict(sorted(h.items()))

    def ff_share(self):
        return self.ff_bytes / max(1, len(self.unstuffed))

    def summary(self):
        return (f"blocks {len(self.pos)} bits {self.total_bits} zrl {self.zrl_histogram()} dc_cat {max(self.dc_cat)} "
                f"ac_cat {max(self.ac_cat)} no_eob {self.eob.count(False)} largest {max(self.bits)} "
                f"ff {100 * self.ff_share():.1f}%")


def _huff_lookup(counts, symbols):
    """16-bit peek → (length << 8 | symbol) for one DHT table; 0 where no code matches."""
    lut = [0] * 65536
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            lo = code << (16 - length)
            v = (length << 8) | symbols[k]
            lut[lo:lo + (1 << (16 - length))] = [v] * (1 << (16 - length))
            code += 1
            k += 1
        code <<= 1
    return lut


def walk(jpeg):
    """Parse a baseline JFIF file (DQT, SOF0, DHT, SOS; no restart markers) of 1 or 3 components and
    Huffman-decode its scan block by block."""
    assert jpeg[:2] == b"\xff\xd8" and jpeg[-2:] == b"\xff\xd9"
    p = 2
    quant, dc_tabs, ac_tabs, comps, scan = {}, {}, {}, [], None
    while scan is None:
        assert jpeg[p] == 0xFF
        marker, n = jpeg[p + 1], (jpeg[p + 2] << 8) | jpeg[p + 3]
        body = jpeg[p + 4:p + 2 + n]
        if marker == 0xDB:
            q = 0
            while q < len(body):
                assert body[q] >> 4 == 0, "8-bit tables only"
                quant[body[q] & 15] = list(body[q + 1:q + 65])
                q += 65
        elif marker == 0xC0:
            assert body[0] == 8
            height, width = (body[1] << 8) | body[2], (body[3] << 8) | body[4]
            for c in range(body[5]):
                cid, hv, tq = body[6 + 3 * c:9 + 3 * c]
                comps.append({"id": cid, "h": hv >> 4, "v": hv & 15, "tq": tq})
        elif marker == 0xC4:
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                counts = list(body[q + 1:q + 17])
                syms = list(body[q + 17:q + 17 + sum(counts)])
                (ac_tabs if tc else dc_tabs)[th] = _huff_lookup(counts, syms)
                q += 17 + sum(counts)
        elif marker == 0xDA:
            assert body[0] == len(comps)
            for c in range(body[0]):
                cid, t = body[1 + 2 * c], body[2 + 2 * c]
                assert cid == comps[c]["id"]
                comps[c]["td"], comps[c]["ta"] = t >> 4, t & 15
            scan = p + 2 + n
        else:
            assert marker in (0xE0, 0xFE) or 0xE0 <= marker <= 0xEF, hex(marker)
        p += 2 + n
    assert len(comps) in (1, 3)
    segment = jpeg[scan:-2]
    data = segment.replace(b"\xff\x00", b"\xff")
    assert data.count(b"\xff") == segment.count(b"\xff\x00"), "a marker inside the scan"
    hmax, vmax = max(c["h"] for c in comps), max(c["v"] for c in comps)
    if len(comps) == 1:
        hmax = vmax = comps[0]["h"] = comps[0]["v"] = 1  # a one-component scan is not interleaved
    mcus = -(-width // (8 * hmax)) * -(-height // (8 * vmax))
    order = [ci for ci, c in enumerate(comps) for _ in range(c["h"] * c["v"])]
    buf = data + b"\xff\xff\xff\xff"

    def peek16(pos):
        i = pos >> 3
        return (((buf[i] << 16) | (buf[i + 1] << 8) | buf[i + 2]) >> (8 - (pos & 7))) & 0xFFFF

    s = Stream()
    s.pos, s.bits, s.comp, s.zrl, s.dc_cat, s.dc_diff, s.ac_cat, s.eob = [], [], [], [], [], [], [], []
    pos = 0
    luts = [(dc_tabs[c["td"]], ac_tabs[c["ta"]]) for c in comps]
    for _ in range(mcus):
        for ci in order:
            dlut, alut = luts[ci]
            start = pos
            v = dlut[peek16(pos)]
            assert v, "no DC code"
            pos += v >> 8
            cat = v & 255
            diff = 0
            if cat:
                m = peek16(pos) >> (16 - cat)
                diff = m if m >> (cat - 1) else m - (1 << cat) + 1
                pos += cat
            k, zrl, amax, eob = 1, 0, 0, False
            while k < 64:
                v = alut[peek16(pos)]
                assert v, "no AC code"
                pos += v >> 8
                rs = v & 255
                if rs == 0:
                    eob = True
                    break
                if rs == 0xF0:
                    zrl += 1
                    k += 16
                    continue
                size = rs & 15
                amax = max(amax, size)
                pos += size
                k += (rs >> 4) + 1
            assert k <= 64
            s.pos.append(start)
            s.bits.append(pos - start)
            s.comp.append(ci)
            s.zrl.append(zrl)
            s.dc_cat.append(cat)
            s.dc_diff.append(diff)
            s.ac_cat.append(amax)
            s.eob.append(eob)
    s.total_bits = pos
    s.unstuffed, s.segment = data, segment
    s.ff_bytes = data.count(b"\xff")
    s.blocks_per_mcu = len(order)
    s.luma_blocks_per_mcu = comps[0]["h"] * comps[0]["v"]
    s.mcus = mcus
    s.quant = {c["tq"]: quant[c["tq"]] for c in comps}
    s.components = len(comps)
    return s


def restuff(stream):
    """The walked bits, padded with ones and 0xFF-stuffed again: must reproduce the segment."""
    nbytes = (stream.total_bits + 7) >> 3
    assert nbytes == len(stream.unstuffed), "bit total vs unstuffed length"
    pad = 8 * nbytes - stream.total_bits
    if pad:
        assert stream.unstuffed[-1] & ((1 << pad) - 1) == (1 << pad) - 1, "padding is not all ones"
    return stream.unstuffed.replace(b"\xff", b"\xff\x00")


class Parts:
    """A stream cut into an encoder's parts: `start`, `length` (bits), `al` (start & 7), `straddle_ff`
    (the byte holding the part's first bit is 0xFF; only a part with al != 0 shares that byte with
    its predecessor) per part, and for the image `final_rem` (bits of the stream in the padded last
    byte, 0: none) and `final_ff` (that byte is 0xFF)."""


def parts(stream, encoder):
    """`encoder`: "gray" (ops.jpeg_encode) or "rgb" (ops.jpeg_encode_rgb)."""
    per = (gray_mcus_per_part(stream.luma_blocks_per_mcu) if encoder == "gray"
           else rgb_mcus_per_part(stream.blocks_per_mcu))
    if encoder == "rgb":
        assert stream.components == 3
    p = Parts()
    p.mcus_per_part = per
    firsts = list(range(0, stream.mcus, per))
    p.start = [stream.pos[m * stream.blocks_per_mcu] for m in firsts]
    ends = p.start[1:] + [stream.total_bits]
    p.length = [e - s for s, e in zip(p.start, ends)]
    p.al = [s & 7 for s in p.start]
    p.straddle_ff = [bool(s & 7) and stream.unstuffed[s >> 3] == 0xFF for s in p.start]
    p.final_rem = stream.total_bits & 7
    p.final_ff = bool(p.final_rem) and stream.unstuffed[-1] == 0xFF
    return p


# ---- a host model of the encoders' stuffing steps -------------------------------------------------
def _bits_value(bits):
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return v


def stuff_model(stream, cut, view, drop=None):
    """The stuffed segment as jpeg_emit_range (src/kernels/jpeg_device.h, steps 4–7) assembles it from the
    parts `cut` of `stream`: per part the 0xFF counts for all eight alignments, the leading ones and
    the last 7 bits; then each part's output position from its predecessors, seen either all as
    aggregates (`view` "aggregate": the look-back resolves their alignments and straddling bytes
    itself) or through the previous part's inclusive record ("inclusive"); then the owned bytes, stuffed.
    `drop` leaves one step out: "fq" (the look-back's `++fq`), "strad" (`own += strad_v == 0xFFu`) or
    "fin" (`own += fin_v == 0xFFu`). With nothing dropped both views give the stream's own segment;
    test_jpeg_stream_cases.py shows which named cases notice each dropped step."""
    bits = np.unpackbits(np.frombuffer(stream.unstuffed, np.uint8))[:stream.total_bits]
    out = bytearray(2 * len(stream.unstuffed) + 16)
    recs, incl_ff, size = [], 0, 0
    nparts = len(cut.start)
    for k in range(nparts):
        r = bits[cut.start[k]:cut.start[k] + cut.length[k]]
        n = len(r)
        ff = [sum(1 for i in range((8 - al) & 7, n - 7, 8) if r[i:i + 8].all()) for al in range(8)]
        head = 0
        while head < min(8, n) and r[head]:
            head += 1
        recs.append((n, ff, head, _bits_value(r[n - 7:] if n >= 7 else r)))
        start = cut.start[k]
        if view == "aggregate":
            ff_before, qstart = 0, 0
            for q in range(k):
                al = qstart & 7
                fq, m = recs[q][1][al], (1 << al) - 1
                if drop != "fq" and al and (recs[q - 1][3] & m) == m and recs[q][2] >= 8 - al:
                    fq += 1   # the byte that straddles parts q − 1 and q
                ff_before += fq
                qstart += recs[q][0]
        else:
            ff_before = incl_ff
        tail_prev = recs[k - 1][3] if k else 0
        al = start & 7
        f = (8 - al) & 7
        own, owned = ff[al], []
        if al:
            take = min(8 - al, n)
            sv = ((tail_prev & ((1 << al) - 1)) << (8 - al)) | (_bits_value(r[:take]) << (8 - al - take))
            if take < 8 - al:
                sv |= (1 << (8 - al - take)) - 1
            own += drop != "strad" and sv == 0xFF
            owned.append(sv)
        nfull = (n - f) >> 3 if n >= f else 0
        rem = n - f - 8 * nfull if n >= f else 0
        owned += [_bits_value(r[f + 8 * i:f + 8 * i + 8]) for i in range(nfull)]
        if k == nparts - 1 and rem:
            fv = (_bits_value(r[f + 8 * nfull:]) << (8 - rem)) | ((1 << (8 - rem)) - 1)
            own += drop != "fin" and fv == 0xFF
            owned.append(fv)
        o = (start >> 3) + ff_before
        for v in owned:
            out[o] = v
            o += 1
            if v == 0xFF:
                out[o] = 0
                o += 1
        incl_ff = ff_before + own
        size = ((start + n + 7) >> 3) + incl_ff
    return bytes(out[:size])


# ---- builders ---------------------------------------------------------------------------------------
def cos_basis(u, v):
    """[8, 8] float: cos((2x + 1)·u·π/16) · cos((2y + 1)·v·π/16), u horizontal, v vertical."""
    t = (2 * np.arange(8) + 1) * np.pi / 16
    return np.outer(np.cos(t * v), np.cos(t * u))


def _u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _blocks_to_image(blocks, h, w):
    """blocks [h/8 · w/8, 8, 8] in raster order → [h, w]."""
    return np.ascontiguousarray(blocks.reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w))


def sparse_hf_blocks(n, seed):
    """n blocks 128 + a·cos_basis(u, v): u, v from 3..7, |a| from 20..109, random sign (quality 50:
    one high coefficient behind a long zero run)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 8, 8))
    for i in range(n):
        u, v = rng.integers(3, 8, 2)
        a = int(rng.integers(20, 110)) * (1 if rng.integers(0, 2) else -1)
        out[i] = 128 + a * cos_basis(int(u), int(v))
    return out


def sparse_hf(h, w, seed):
    return _blocks_to_image(_u8(sparse_hf_blocks((h // 8) * (w // 8), seed)), h, w)


def dc_checker(h, w, shift=0):
    """Flat blocks alternating 0 and 255 along the raster order (block i is 255 where (i + shift) is
    odd): DC differences of ±2040 at quality 100. With 32 blocks a row and shift 0, block 255 is 255
    and block 256 is 0; shift 1 is the variant with block 255 = 0 and block 256 = 255."""
    i = np.arange((h // 8) * (w // 8)) + shift
    return _blocks_to_image(np.broadcast_to(((i & 1) * 255).astype(np.uint8)[:, None, None], (i.size, 8, 8)).copy(), h, w)


def binary_noise(h, w, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


BINARY_NOISE_SEED = 24   # the first seed whose 48×80 image reaches AC category 10 (1 in about 25 does)


def uniform_noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def flat_levels():
    """128×128: block i flat at level i."""
    return _blocks_to_image(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, 8, 8)).copy(), 128, 128)


FLAT_LEVEL_QUALITIES = (10, 50, 90, 100)

# Gray edge images (quality 100, gray sampling, 32 blocks a row): everything flat 128 except
#   block 0            128 + a·cos_basis(1, 0): its length moves every later bit position;
#   block 256·k − 1    64 + EDGE_A·cos_basis(7, 7): ends on coefficient 63 (no EOB) in EDGE_ONES one-bits;
#   block 256·k        flat 255: DC difference 1528, category 11, code 111111110;
#   the last block     64 + EDGE_A·cos_basis(7, 7).
EDGE_A = 31.5
EDGE_ONES = 9
# a per alignment of part 1's start (two parts, 128×256), and per remainder of the padded last byte.
STRADDLE_A = {1: 24, 2: 6, 3: 8, 4: 4, 5: 30, 6: 10, 7: 0}
FINAL_A = {1: 14, 2: 24, 3: 6, 4: 8, 5: 4, 6: 30, 7: 10}
# Three parts (192×256): part 1 starts at alignment al on a 0xFF byte and has a successor, which needs
# part 1's straddling byte in its own output position — from part 1's inclusive record, or, when it
# sees part 1 only as an aggregate, from the look-back's own straddle test.
STRADDLE3_A = dict(STRADDLE_A)


def edge_image(a, nparts=2):
    n = 256 * nparts
    b = np.full((n, 8, 8), 128.0)
    b[0] = 128 + a * cos_basis(1, 0)
    hf = 64 + EDGE_A * cos_basis(7, 7)
    for k in range(1, nparts):
        b[256 * k - 1] = hf
        b[256 * k] = 255
    b[n - 1] = hf
    return _blocks_to_image(_u8(b), 64 * nparts, 256)


def straddle(al):
    return edge_image(STRADDLE_A[al])


def straddle3(al):
    return edge_image(STRADDLE3_A[al], 3)


def final(rem):
    return edge_image(FINAL_A[rem])


# ---- gray cases: equally shaped images of one quality share a launch ------------------------------
def gray_cases():
    """{(quality, (h, w)): {name: uint8 [h, w]}}: one launch each in the GPU test."""
    c = {
        (50, (48, 80)): {"sparse_hf_a": sparse_hf(48, 80, 1), "sparse_hf_b": sparse_hf(48, 80, 2)},
        (50, (272, 400)): {"sparse_hf": sparse_hf(272, 400, 3)},
        (100, (128, 256)): {"dc_checker": dc_checker(128, 256), "dc_checker_shifted": dc_checker(128, 256, 1)},
        (100, (48, 80)): {"binary_noise": binary_noise(48, 80, BINARY_NOISE_SEED)},
        (100, (128, 128)): {"uniform_noise": uniform_noise(128, 128, 5), "flat_levels": flat_levels()},
    }
    for q in FLAT_LEVEL_QUALITIES:
        c.setdefault((q, (128, 128)), {})["flat_levels"] = flat_levels()
    return c


def edge_cases():
    """The seven straddle and seven final images of one gray-sampling launch at quality 100."""
    c = {f"straddle_{al}": straddle(al) for al in range(1, 8)}
    c.update({f"final_{rem}": final(rem) for rem in range(1, 8)})
    return c


def edge3_cases():
    return {f"straddle3_{al}": straddle3(al) for al in range(1, 8)}


LIMIT_SHAPES = ((128, 128), (128, 256))


def limit_launch(shape):
    """{name: image}, one launch at quality 100. 128×128: [uniform_noise, binary_noise, flat_levels],
    exactly one full part each at gray sampling — the uniform noise under the range limit, the binary
    noise over it. 128×256: [uniform_noise, binary_noise, straddle(3)], two parts each: both parts of the
    binary noise over the limit, both of the uniform noise under it."""
    h, w = shape
    third = {"flat_levels": flat_levels()} if shape == (128, 128) else {"straddle_3": straddle(3)}
    return {"uniform_noise": uniform_noise(h, w, 5), "binary_noise": binary_noise(h, w, 6), **third}


# ---- colour cases ----------------------------------------------------------------------------------
def ycc_to_rgb(y, cb, cr):
    """Float YCbCr planes → uint8 RGB (JFIF's inverse, rounded): what the encoders convert back."""
    r = y + 1.402 * (cr - 128)
    g = y - 0.344136 * (cb - 128) - 0.714136 * (cr - 128)
    b = y + 1.772 * (cb - 128)
    return _u8(np.stack([r, g, b], -1))


def rgb_sparse_hf(h, w, seed):
    return np.stack([sparse_hf(h, w, seed + c) for c in range(3)], -1)


def rgb_binary_noise(h, w, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


_SATURATED = np.array([[255, 0, 0], [0, 255, 255], [255, 0, 0], [0, 255, 255], [0, 0, 255], [255, 255, 0],
                       [0, 0, 255], [255, 255, 0], [0, 255, 0], [255, 0, 255], [0, 0, 0], [255, 255, 255]], np.uint8)


def rgb_dc_checker(h, w):
    """16×16 cells of saturated colours, each followed by its complement: red, cyan, red, cyan (Cr from
    255 to 0 and back), blue, yellow, blue, yellow (Cb likewise), green, magenta, black, white. Cb and Cr
    DC differences of ±2040 at quality 100."""
    ny, nx = h // 16, w // 16
    idx = (np.arange(ny * nx) % len(_SATURATED)).reshape(ny, nx)
    return np.ascontiguousarray(np.repeat(np.repeat(_SATURATED[idx], 16, 0), 16, 1))


# Colour edge images (quality 100), built as the gray ones: Y, Cb, Cr flat (128, 128, 128) except
#   MCU 0              Y = 128 + a·cos_basis(1, 0) in its first block: moves the bit positions;
#   MCU per − 1        Cr = 128 + RGB_EDGE_A·cos_basis(7, 7) (4:2:0: 2×2-replicated over the 16×16 MCU), with Y at
#                      RGB_EDGE_Y: the MCU's last block ends on coefficient 63;
#   MCU per            Y = 255 (white): a large luma DC step into the next part;
#   the last MCU       as MCU per − 1.
# RGB rounding leaves ±1 noise in all three components at quality 100, so the parameters were found by
# search over a (and the amplitude) on the golden encoder's stream.
RGB_EDGE_SHAPE = (64, 256)   # 4:2:0: 64 MCUs = 2 parts; 4:4:4: 256 MCUs = 4 parts
RGB_EDGE_A = 21.0
RGB_EDGE_Y = 100.0
# a, found with the amplitude and level above: part 1 starts at alignment 2 on a 0xFF byte; the padded
# last byte is 0xFF with 2 stream bits in it.
RGB_STRADDLE_A = {"420": 14, "444": 6}
RGB_FINAL_A = {"420": 30, "444": 30}


def rgb_edge_image(sampling, a):
    h, w = RGB_EDGE_SHAPE
    px = 16 if sampling == "420" else 8
    per = rgb_mcus_per_part(6 if sampling == "420" else 3)
    mx = w // px
    nmcu = mx * (h // px)
    y = np.full((h, w), 128.0)
    cb = np.full((h, w), 128.0)
    cr = np.full((h, w), 128.0)
    hf = RGB_EDGE_A * cos_basis(7, 7)
    if sampling == "420":
        hf = np.repeat(np.repeat(hf, 2, 0), 2, 1)

    def cell(m):
        return slice(px * (m // mx), px * (m // mx) + px), slice(px * (m % mx), px * (m % mx) + px)

    y[:8, :8] = 128 + a * cos_basis(1, 0)
    for m in (per - 1, nmcu - 1):
        ys, xs = cell(m)
        cr[ys, xs] = 128 + hf
        y[ys, xs] = RGB_EDGE_Y
    ys, xs = cell(per)
    y[ys, xs] = 255
    return ycc_to_rgb(y, cb, cr)


def rgb_cases(sampling):
    """{(quality, (h, w)): {name: uint8 [h, w, 3]}} for ops.jpeg_encode_rgb at `sampling`."""
    c = {
        (50, (48, 80)): {"rgb_sparse_hf": rgb_sparse_hf(48, 80, 11)},
        (50, (64, 256)): {"rgb_sparse_hf_parts": rgb_sparse_hf(64, 256, 14)},
        (100, (48, 80)): {"rgb_binary_noise": rgb_binary_noise(48, 80, 12)},
        (100, RGB_EDGE_SHAPE): {"rgb_dc_checker": rgb_dc_checker(*RGB_EDGE_SHAPE)},
    }
    c[(100, RGB_EDGE_SHAPE)]["rgb_straddle"] = rgb_edge_image(sampling, RGB_STRADDLE_A[sampling])
    c[(100, RGB_EDGE_SHAPE)]["rgb_final"] = rgb_edge_image(sampling, RGB_FINAL_A[sampling])
    return c


# The range limit in colour. A part of the colour encoder holds 252 (4:2:0) or 255 (4:4:4) coded blocks
# and must average about 870 bits a block in Y, Cb and Cr at once to pass RANGE_LIMIT_BITS. Noise does
# not get there: at quality 100 one full part of per-channel 0 / 255 noise is 195 472 (4:2:0) and
# 203 758 (4:4:4) bits, and the best of 18 palettes of saturated colours 199 926 (black, white, blue,
# yellow, red, cyan) and 207 447 (blue, yellow, red, cyan). The two images under tests/golden/ were
# searched for on the CPU, scored by the golden encoder's stream:
#   1. from that palette noise, 40 rounds of alternating projections: in the 8×8 DCT of Y, Cb and Cr
#      raise every AC magnitude below a floor to it, sign kept (4:4:4: floors 100 / 110 / 110; 4:2:0: 150
#      for Y and 75 for the 2×2-averaged chroma), convert back to RGB, clip and round — 218 415 bits at
#      4:4:4, 220 648 at 4:2:0;
#   2. a hill climb of single-sample steps of up to ±60, kept when the unstuffed stream of the sample's
#      few MCUs does not shrink — 222 132 bits at 4:4:4 and 223 491 at 4:2:0 after about 10⁷ steps.
# They are data, not built here: test_jpeg_stream_cases.py checks that each still has its part over the
# limit and is libjpeg's stream.
_PALETTE = {"k": (0, 0, 0), "w": (255, 255, 255), "r": (255, 0, 0), "c": (0, 255, 255), "b": (0, 0, 255),
            "y": (255, 255, 0), "g": (0, 255, 0), "m": (255, 0, 255)}
RGB_NEAR_LIMIT = {"420": ((48, 224), "kwbyrc"), "444": ((48, 128), "byrc")}   # one full part (42 / 85 MCUs)
RGB_LIMIT_OUT_CAP = 256 * 1024   # the longest stream here is 32 KB: capacity is not what fails


def rgb_palette_noise(h, w, seed, palette):
    cols = np.array([_PALETTE[c] for c in palette], np.uint8)
    return cols[np.random.default_rng(seed).integers(0, len(palette), (h, w))]


def rgb_over_limit(sampling):
    """uint8 [48, 224, 3] (4:2:0, one part) or [48, 128, 3] (4:4:4, a full part and one of 11 MCUs):
    part 0 is over the range limit."""
    img = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"jpeg_rgb_over_limit_{sampling}.npy"))
    assert img.dtype == np.uint8 and img.shape == RGB_NEAR_LIMIT[sampling][0] + (3,)
    return img


def rgb_limit_launch(sampling):
    """{name: image}, one launch at quality 100: the longest part of palette noise (90–94 % of the
    limit), the searched image over the limit, and an ordinary neighbour."""
    (h, w), palette = RGB_NEAR_LIMIT[sampling]
    return {"rgb_palette_noise": rgb_palette_noise(h, w, 22, palette),
            "rgb_over_limit": rgb_over_limit(sampling),
            "rgb_sparse_hf": rgb_sparse_hf(h, w, 23)}


# ---- engine ----------------------------------------------------------------------------------------
def engine_slices(native):
    """Three 512×512 slices for 512² canvases at quality 100: the middle one 0 / 4095 binary noise, whose
    original canvas is 0 / 255 (every part over the range limit); phantoms around it."""
    noise = (np.random.default_rng(31).integers(0, 2, (512, 512)) * 4095).astype(np.uint16)
    return {"phantom_a": native.phantom_slice(512, 512, 3, 12, 25, 7), "binary_noise": noise,
            "phantom_b": native.phantom_slice(512, 512, 2, 12, 25, 11)}


ENGINE_FALLBACKS = 1   # of the 6 exported images: the noise slice's original (test_jpeg_stream_cases.py)
ENGINE_OUT_CAP = 1 << 20
