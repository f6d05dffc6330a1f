// The per-lane bodies of the device Huffman coder (jpeg_huff_device.hip): plain functions of (unit or chunk index,
// buffers), usable from host and device, so that tools/jpeg_huff_device_check.cpp runs the very code the kernels run,
// serially and in a shuffled order, under a host sanitizer.
//
// A CODING UNIT is one 8x8 block in scan order: MCU raster, then component, then the v x h blocks of the component
// inside the MCU.  Its bits depend on its own 64 coefficients and on the DC of the previous unit of its component, whose
// index is arithmetic in the unit's own; no state is carried from unit to unit.  The passes over one frame:
//
//   size   one lane per unit     bits[u] = length of the unit's code; a value outside baseline JPEG marks the frame
//   scan   (kernel)              bits[] -> exclusive bit offsets, total_bits
//   pack   one lane per unit     the unit's code, OR-ed into the frame's zeroed, big-endian bit stream `area`
//   count  one lane per chunk    cnt[c] = FF bytes among the kChunk stream bytes of chunk c
//   scan   (kernel)              cnt[] -> exclusive, ff_total
//   emit   one lane per chunk    out[header_len + i + ff_before(i)] = stream byte i, 00 behind every FF; the header,
//                                EOI, length and status by the first lanes
//
// Bit offsets are 32-bit: the entry point refuses a geometry with kMaxBlockBits * units >= 2^32.  The stream area holds
// min(capacity, worst case) bytes (rounded up to whole chunks).  A frame whose stream is longer cannot fit its file into
// `capacity`; its bytes past the area are dropped by `pack`, and `count` re-derives them from the coefficients (the
// slow path) so that the reported length is still the exact one.  Every store into `out` is guarded by `capacity`.
#pragma once
#include "jpeg_geom.h"
#include "jpeg_huff_tables.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define VNF_HUFF_OR(p, v) atomicOr((p), (v))
#else
#define VNF_HUFF_OR(p, v) (*(p) |= (v))
#endif

namespace vnf {
namespace huff {

constexpr int kChunk = 128;   // stream bytes per lane of the count and emit passes; a multiple of 16
constexpr int kOk = 0, kInvalid = -1, kCapacity = -4;   // VNF_OK, VNF_E_INVALID, VNF_E_CAPACITY

struct alignas(16) Vec16 {
  uint32_t w[4];
};

struct Geom {
  int mx;             // MCUs per row
  int h0, v0;         // luma blocks per MCU, across and down
  int upm;            // units per MCU: h0 * v0 + 2
  int bw[3];          // blocks per row of each plane
  long long plane[3]; // first coefficient of each plane inside a frame
  unsigned units;     // per frame
};

// One frame's buffers.  bits: `units` entries (sizes, then exclusive offsets); cnt: one entry per chunk of the longest
// possible stream; area: area_bytes zeroed bytes, 16-byte aligned, a multiple of kChunk.
struct Frame {
  const int16_t* coefs;
  uint32_t* bits;
  uint32_t* cnt;
  uint32_t* area;
  long long area_bytes;
  int32_t* invalid;      // zeroed; set when a unit holds a value outside baseline JPEG
  uint32_t* total_bits;  // of the scan, before padding
  uint32_t* ff_total;
  const uint8_t* header;
  long long header_len;
  uint8_t* out;
  long long capacity;
  int64_t* length;
  int32_t* status;
};

VNF_HD inline long long stream_bytes(const Frame& f) { return ((long long)*f.total_bits + 7) >> 3; }

// unit -> its component and the first of its 64 coefficients
VNF_HD inline long long unit_block(const Geom& g, unsigned u, int* comp) {
  const unsigned m = u / g.upm, r = u % g.upm;
  const int luma = g.h0 * g.v0;
  const int x = m % g.mx, y = m / g.mx;
  if ((int)r < luma) {
    *comp = 0;
    const int by = r / g.h0, bx = r % g.h0;
    return g.plane[0] + ((long long)(y * g.v0 + by) * g.bw[0] + (x * g.h0 + bx)) * 64;
  }
  const int c = 1 + (int)r - luma;
  *comp = c;
  return g.plane[c] + ((long long)y * g.bw[c] + x) * 64;
}

// the previous unit of the same component in scan order; -1: none (the prediction is 0)
VNF_HD inline long long unit_pred(const Geom& g, unsigned u) {
  const unsigned m = u / g.upm, r = u % g.upm;
  const int luma = g.h0 * g.v0;
  if ((int)r < luma && r > 0) return (long long)u - 1;
  if (m == 0) return -1;
  return (int)r < luma ? (long long)(m - 1) * g.upm + luma - 1 : (long long)u - g.upm;
}

// Runs the walk of unit u into `put`.  The block is read with eight 16-byte loads.
template <class Put>
VNF_HD inline bool walk_unit(const Geom& g, const int16_t* coefs, const Tables& t, unsigned u, Put&& put) {
  int c;
  const long long at = unit_block(g, u, &c);
  const long long pu = unit_pred(g, u);
  int pc, pred = 0;
  if (pu >= 0) pred = coefs[unit_block(g, (unsigned)pu, &pc)];
  alignas(16) int16_t blk[64];
  const Vec16* src = reinterpret_cast<const Vec16*>(coefs + at);
  VNF_HUFF_UNROLL
  for (int i = 0; i < 8; ++i) {
    const Vec16 v = src[i];
    __builtin_memcpy(blk + 8 * i, &v, 16);
  }
  return encode_block(blk, pred, t.dc[c ? 1 : 0], t.ac[c ? 1 : 0], put);
}

// the last unit of a frame pads the stream to a whole byte with 1-bits; `pos` is the bit position behind the unit
template <class Put>
VNF_HD inline void pad_last(const Geom& g, unsigned u, long long pos, Put&& put) {
  const int pad = (int)(-pos & 7);
  if (u + 1 == g.units && pad) put((1u << pad) - 1u, pad);
}

// size pass ------------------------------------------------------------------------------------------------------------
VNF_HD inline void size_unit(const Geom& g, const Frame& f, const Tables& t, unsigned u) {
  uint32_t n = 0;
  if (!walk_unit(g, f.coefs, t, u, [&n](uint32_t, int k) { n += (uint32_t)k; }))
    *f.invalid = 1;   // every lane that sees one stores the same value
  f.bits[u] = n;      // of an invalid unit: what the walk put before it stopped, as the pack pass will
}

// pack pass ------------------------------------------------------------------------------------------------------------
// Big-endian 32-bit words of the stream.  A word that lies wholly inside the unit's bit range is stored; the first and
// the last one may be shared with the neighbours (up to eight units lie inside one word) and are OR-ed into the zeroed
// area.  Words past the area are dropped.
struct PackSink {
  uint32_t* words;
  long long nwords, w;
  uint64_t acc;   // the low n bits are pending; a unit that starts inside a word begins with that many zero bits
  int n;
  bool shared;    // the word being filled began before this unit

  VNF_HD void word(uint32_t x, bool merge) {
    if (w < nwords) {
      const uint32_t be = __builtin_bswap32(x);
      if (merge) VNF_HUFF_OR(words + w, be);
      else words[w] = be;
    }
    ++w;
  }
  VNF_HD void operator()(uint32_t v, int k) {
    acc = (acc << k) | (uint64_t)(v & ((1u << k) - 1u));   // k <= 26, n <= 31: 57 bits at most
    n += k;
    if (n >= 32) {
      word((uint32_t)(acc >> (n - 32)), shared);
      shared = false;
      n -= 32;
    }
  }
  VNF_HD void finish() {
    if (n > 0) word((uint32_t)(acc << (32 - n)), true);
  }
};

VNF_HD inline void pack_unit(const Geom& g, const Frame& f, const Tables& t, unsigned u) {
  const uint32_t off = f.bits[u];
  PackSink s{f.area, f.area_bytes >> 2, (long long)(off >> 5), 0, (int)(off & 31u), (off & 31u) != 0};
  walk_unit(g, f.coefs, t, u, s);
  pad_last(g, u, s.w * 32 + s.n, s);
  s.finish();
}

// count pass -----------------------------------------------------------------------------------------------------------
VNF_HD inline uint32_t ff_bytes(uint32_t w) {   // how many of the four bytes of w are FF (exact: no carry between bytes)
  const uint32_t x = ~w;
  const uint32_t y = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
  return (uint32_t)__builtin_popcount(y);
}

// the bits of the stream that fall into one chunk, rebuilt from the coefficients
struct WindowSink {
  uint32_t win[kChunk / 4];   // big-endian words as values: bit 31 of win[0] is the chunk's first bit
  long long lo, pos;
  VNF_HD void operator()(uint32_t v, int k) {
    for (int i = 0; i < k; ++i) {
      const long long rel = pos + i - lo;
      if (((v >> (k - 1 - i)) & 1u) && rel >= 0 && rel < (long long)kChunk * 8) win[rel >> 5] |= 1u << (31 - (int)(rel & 31));
    }
    pos += k;
  }
};

VNF_HD inline void count_chunk(const Geom& g, const Frame& f, const Tables& t, long long c) {
  const long long total = stream_bytes(f), c0 = c * kChunk;
  if (c0 >= total) return;
  uint32_t n = 0;
  if (c0 + kChunk <= f.area_bytes) {   // the bytes behind the stream's end are zero
    const Vec16* src = reinterpret_cast<const Vec16*>(reinterpret_cast<const uint8_t*>(f.area) + c0);
    for (int i = 0; i < kChunk / 16; ++i) {
      const Vec16 x = src[i];
      n += ff_bytes(x.w[0]) + ff_bytes(x.w[1]) + ff_bytes(x.w[2]) + ff_bytes(x.w[3]);
    }
  } else {
    // the units that reach into bits [lo, hi): from the last one that starts at or before lo
    const long long lo = c0 * 8, hi = lo + (long long)kChunk * 8;
    unsigned a = 0, b = g.units - 1;
    while (a < b) {
      const unsigned m = a + (b - a + 1) / 2;
      if ((long long)f.bits[m] <= lo) a = m;
      else b = m - 1;
    }
    WindowSink s;
    for (int i = 0; i < kChunk / 4; ++i) s.win[i] = 0;
    s.lo = lo;
    for (unsigned u = a; u < g.units && (long long)f.bits[u] < hi; ++u) {
      s.pos = f.bits[u];
      walk_unit(g, f.coefs, t, u, s);
      pad_last(g, u, s.pos, s);
    }
    for (int i = 0; i < kChunk / 4; ++i) n += ff_bytes(s.win[i]);
  }
  f.cnt[c] = n;
}

// emit pass ------------------------------------------------------------------------------------------------------------
VNF_HD inline void emit_header_byte(const Frame& f, long long i) {
  if (i < f.header_len && i < f.capacity) f.out[i] = f.header[i];
}

// EOI, the file's length and the frame's status
VNF_HD inline void emit_tail(const Frame& f) {
  const long long end = f.header_len + stream_bytes(f) + (long long)*f.ff_total;
  if (end < f.capacity) f.out[end] = 0xFF;
  if (end + 1 < f.capacity) f.out[end + 1] = 0xD9;
  *f.length = end + 2;
  *f.status = *f.invalid ? kInvalid : end + 2 > f.capacity ? kCapacity : kOk;
}

VNF_HD inline void emit_chunk(const Frame& f, long long c) {
  const long long total = stream_bytes(f), c0 = c * kChunk;
  if (c0 >= total || c0 + kChunk > f.area_bytes) return;   // past the area: the byte's place is past `capacity` too
  long long dst = f.header_len + c0 + (long long)f.cnt[c];
  const Vec16* src = reinterpret_cast<const Vec16*>(reinterpret_cast<const uint8_t*>(f.area) + c0);
  const int count = total - c0 < kChunk ? (int)(total - c0) : kChunk;
  for (int i = 0; i < count; i += 16) {
    const Vec16 x = src[i >> 4];
    for (int j = 0; j < 16 && i + j < count; ++j) {
      const uint32_t b = (x.w[j >> 2] >> (8 * (j & 3))) & 255u;   // memory order: the words are stored big-endian
      if (dst < f.capacity) f.out[dst] = (uint8_t)b;
      ++dst;
      if (b == 0xFF) {
        if (dst < f.capacity) f.out[dst] = 0;
        ++dst;
      }
    }
  }
}

// host side: geometry and workspace ------------------------------------------------------------------------------------
constexpr long long kHeaderLen = 623;   // SOI .. SOS header of the files the coder writes (vnf_jpeg_huff_header)

inline Geom make_geom(const vnf_jpeg_info& info, const JpegGeom& jg) {
  Geom g;
  g.mx = jg.bw[1];
  g.h0 = info.h[0];
  g.v0 = info.v[0];
  g.upm = g.h0 * g.v0 + 2;
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = jg.bw[c];
    g.plane[c] = jg.plane_off[c];
  }
  g.units = (unsigned)jg.blocks;
  return g;
}

inline long long round_up(long long v, long long m) { return (v + m - 1) / m * m; }

// the workspace of n frames: [area n x area_bytes | invalid n (the zeroed part ends here) | total_bits n | ff_total n |
// bits n x bits_stride | cnt n x cnt_stride], every part 16-byte aligned, the strides multiples of 4 entries
struct Layout {
  long long area_bytes, bits_stride, cnt_stride;
  long long invalid_at, total_at, ff_at, bits_at, cnt_at, bytes;
};

// false: the frame is too large for 32-bit bit offsets
inline bool layout(int n, const JpegGeom& jg, long long capacity, Layout* l) {
  const long long units = jg.blocks;
  if (units * kMaxBlockBits >= (1LL << 32)) return false;
  const long long worst = (units * kMaxBlockBits + 7) / 8;
  l->area_bytes = round_up(capacity < worst ? capacity : worst, kChunk);
  l->bits_stride = round_up(units, 4);
  l->cnt_stride = round_up((worst + kChunk - 1) / kChunk, 4);
  const long long per_n = round_up(4LL * n, 16);
  l->invalid_at = (long long)n * l->area_bytes;
  l->total_at = l->invalid_at + per_n;
  l->ff_at = l->total_at + per_n;
  l->bits_at = l->ff_at + per_n;
  l->cnt_at = l->bits_at + 4LL * n * l->bits_stride;
  l->bytes = l->cnt_at + 4LL * n * l->cnt_stride;
  return true;
}

}  // namespace huff
}  // namespace vnf
