// The device Huffman DEcoder of the JPEG frame decoder (jpeg_huff_decode.hip): the format of a prepared frame
// (vnf_jpeg_huff_prepare, jpeg_entropy.cpp) and the per-lane bodies of the passes, plain functions of (lane index,
// buffers, subseq_bits), usable from host and device, so that tools/jpeg_huff_decode_check.cpp runs the very code the
// kernels run, serially and in a shuffled order, under a host sanitizer.  Units and their blocks are those of
// jpeg_huff_device.h (`unit_block`).
//
// A Huffman stream has no index: where a symbol starts is known only after decoding everything before it.  It does
// re-synchronise, though (Weissenberger and Schmidt, "Massively parallel Huffman decoding on GPUs", ICPP 2018): a
// decoder started at a wrong bit usually falls into step with the right one after a few symbols.  The scan of a frame
// is cut into SEGMENTS at its RSTn markers (one segment without DRI) and every segment into SUBSEQUENCES of
// `subseq_bits` bits, one LANE each; a subsequence never crosses a segment.
//
// The STATE of a decoder at a symbol boundary is (bit position in the segment, unit index inside the MCU, zigzag index
// k; k = 0: a DC symbol is next).  Two decoders that agree on it agree on everything after it.  A lane's EXIT state is
// the first symbol boundary at or past its subsequence's end, packed into 32 bits with the position relative to that
// end (under 31: the longest symbol is a 16-bit code with 15 magnitude bits), or "dead" after an impossible code.
//
//   plan        one lane per segment   the segment's extent checked against the blob size the host passed; its lanes
//   scan        (kernel)               lanes per segment -> first lane of every segment
//   speculate   one lane per subseq.   decode from state (0, 0, 0) at the lane's own first bit: true for the first lane
//                                      of a segment (a HEAD), a guess for every other one -> exit state
//   synchronise level 1: a workgroup owns kLoad consecutive lanes (a LOAD).  Round: lane i decodes again from lane
//               i-1's exit state when that differs from the entry it used last; the load's first lane keeps the guess.
//               A fixed point within kLoad rounds: true-relative-to-the-load's-entry states spread one lane a round.
//               level 2: one lane per load, a workgroup owns kLoad loads.  Round: a load whose entry (the exit of the
//               load before it) changed walks its lanes from that entry until a lane's exit state comes out as
//               recorded, a head, or the load's end.  A fixed point within kLoad rounds.  Streams of more than
//               kLoad * kLoad lanes take one launch per group of kLoad loads, in order: the dependency is carried by
//               the stream, never by a flag.  Nothing here relies on the stream re-synchronising -- that only makes
//               the rounds few.
//               Worst case, a stream that never re-synchronises (flat picture areas, whose periodic bits hold a wrong
//               decoder in a cycle of its own, come close): the true states then advance one lane per level-1 round and
//               one load per level-2 round, and a level-2 lane decodes its whole load serially in every round -- up to
//               kLoad rounds x kLoad lanes x subseq_bits one-bit symbols by one thread (6.7e7 at the default, 5.4e8 at
//               8192).  It ends, but a frame then decodes no faster than one lane reads it.
//   count       one lane per subseq.   units that complete inside the lane, decoding from its TRUE entry
//   scan        (kernel)               -> units before every lane
//   write       one lane per subseq.   decode once more and store every non-zero coefficient at its natural position
//                                      in the zeroed frame; DC differences go to position 0 and to `dctmp`.  All the
//                                      checks of the host decoder sit here: an impossible code, a run past the block, a
//                                      unit that ends past the segment, a segment short of its share of units, 8 or more
//                                      bits left in a non-final segment.  Symbols past a segment's share are ignored.
//   scan        (kernel)               dctmp -> exclusive sums
//   dc          one lane per unit      DC value = sum of the differences since the restart interval began; a value
//                                      outside int16 marks the frame
//
// Every loop is bounded by bit counts: a symbol consumes at least one bit (a table entry of length 0 is an impossible
// code), a lane stops at its subsequence's end plus one symbol.  Speculative lanes read only inside their segment
// (bits past its end are zero) and write only their own state slot.
#pragma once
#include "jpeg_huff_device.h"

namespace vnf {
namespace hdec {

using huff::Geom;
using huff::kInvalid;
using huff::kOk;

constexpr int kLook = 10;                // bits of the one-step code lookup, as in jpeg_entropy.cpp
constexpr int kDefaultSubseqBits = 1024;
constexpr int kMinSubseqBits = 32;       // above the longest symbol (31 bits): an entry lies inside the lane's own subsequence
constexpr int kMaxSubseqBits = 8192;
constexpr int kLoad = 256;               // lanes per workgroup of the per-lane kernels = lanes per load
constexpr int kMaxTables = 6;            // a DC and an AC table per component
constexpr uint32_t kMagic = 0x31444856u; // "VHD1"
constexpr long long kMaxBlobBytes = 1LL << 28;   // bit positions are 32-bit

// ---- the prepared frame (position-independent; every offset is in bytes from the blob's first byte, which is 16-byte
// aligned wherever the blob lies) ----
//   BlobHeader | DTable x ntables | Seg x nseg | the segments' bytes, FF 00 unstuffed, each 16-byte aligned and
//   zero-padded to a multiple of 16
struct DTable {
  uint16_t look[1 << kLook];   // (length << 8) | symbol for codes of at most kLook bits, 0: longer
  int32_t maxcode[18];         // largest code of each length, -1: none; [17] closes the walk
  int32_t valoff[17];          // index of the first symbol of a length minus its first code
  int32_t nvals;
  uint8_t vals[256];
};
static_assert(sizeof(DTable) == 2448 && sizeof(DTable) % 16 == 0, "DTable is part of the blob format");

struct BlobHeader {
  uint32_t magic, total_bytes, nseg, restart_interval;
  uint32_t tables_at, ntables, seg_at, data_at;
  uint32_t ncomp;
  uint8_t dc_sel[4], ac_sel[4];   // per component: index into the blob's tables
  uint32_t pad[5];
};
static_assert(sizeof(BlobHeader) == 64, "BlobHeader is part of the blob format");

struct Seg {
  uint32_t at, bytes;   // of the unstuffed segment
};

inline long long round16(long long v) { return (v + 15) & ~15LL; }

// how many segments the scan of *info has
inline long long segments_of(const vnf_jpeg_info& info) {
  const long long mcus = (long long)(info.blocks_w[0] / info.h[0]) * (info.blocks_h[0] / info.v[0]);
  return info.restart_interval > 0 ? (mcus + info.restart_interval - 1) / info.restart_interval : 1;
}

// the longest blob a file of len bytes with *info's segments can give
inline long long prepared_bound(long long len, const vnf_jpeg_info& info) {
  const long long s = segments_of(info);
  return (long long)sizeof(BlobHeader) + kMaxTables * (long long)sizeof(DTable) + round16(8 * s) + round16(len) + 16 * s;
}

// ---- what the lanes work on ----
// per frame, written by the plan pass after it has checked the header against the blob size the host passed
struct alignas(16) Meta {
  int32_t invalid;       // zeroed by the entry point; set by plan, write and dc lanes (every one stores the same value)
  uint32_t nlanes, nseg, ri;
  uint32_t seg_at, tables_at, ntables, pad;
  uint8_t dc_sel[4], ac_sel[4];
  uint32_t pad2[6];
};
static_assert(sizeof(Meta) == 64, "Meta");

struct Frame {
  const uint8_t* blob;     // 16-byte aligned
  uint32_t blob_bytes;     // what the host passed: nothing past it is read
  Meta* meta;
  uint32_t* seg_lane0;     // seg_cap + 1 entries (and room for the scan's whole uint4s): first lane of every segment
  uint32_t* state;         // lane_cap exit states
  uint32_t* cnt;           // lane_cap: units completed in the lane, then units before it
  uint32_t* dctmp;         // `units` DC differences in component order, then their exclusive sums
  int16_t* coefs;
  long long coef_count;
  uint32_t lane_cap, seg_cap;
};

// what a lane needs of the geometry and the header
struct Sel {
  int upm, luma;
  uint8_t dc[3], ac[3];
};

VNF_HD inline Sel make_sel(const Geom& g, const Meta& m) {
  Sel s;
  s.upm = g.upm;
  s.luma = g.h0 * g.v0;
  for (int c = 0; c < 3; ++c) {
    s.dc[c] = m.dc_sel[c];
    s.ac[c] = m.ac_sel[c];
  }
  return s;
}

VNF_HD inline const DTable* tables_of(const Frame& f) {
  return reinterpret_cast<const DTable*>(f.blob + f.meta->tables_at);
}

// packed state
constexpr uint32_t kDead = 1u << 15, kOver = 1u << 16, kStateMask = (1u << 17) - 1u;
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;   // "decoded from nothing yet": equals no state
VNF_HD inline uint32_t pack_state(uint32_t past_end, int unit, int k) { return past_end | ((uint32_t)unit << 5) | ((uint32_t)k << 9); }

// plan pass ------------------------------------------------------------------------------------------------------------
// The header of the blob against blob_bytes and the geometry; fills *f.meta (but `invalid` on success).  One lane.
VNF_HD inline bool plan_header(const Frame& f, int ncomp, uint32_t mcus) {
  Meta& m = *f.meta;
  m.nlanes = 0;
  m.nseg = 0;
  if (f.blob_bytes < sizeof(BlobHeader)) return false;
  const BlobHeader& h = *reinterpret_cast<const BlobHeader*>(f.blob);
  const uint64_t size = f.blob_bytes;
  if (h.magic != kMagic || h.ncomp != (uint32_t)ncomp || h.ntables < 1 || h.ntables > (uint32_t)kMaxTables) return false;
  if ((h.tables_at & 15u) || h.tables_at > size || (uint64_t)h.ntables * sizeof(DTable) > size - h.tables_at) return false;
  if (h.nseg < 1 || h.nseg > f.seg_cap || (h.seg_at & 7u) || h.seg_at > size || (uint64_t)h.nseg * sizeof(Seg) > size - h.seg_at)
    return false;
  const uint32_t ri = h.restart_interval;
  if (h.nseg != (ri ? (mcus + ri - 1) / ri : 1u)) return false;
  for (int c = 0; c < ncomp; ++c)
    if (h.dc_sel[c] >= h.ntables || h.ac_sel[c] >= h.ntables) return false;
  const DTable* t = reinterpret_cast<const DTable*>(f.blob + h.tables_at);
  for (uint32_t i = 0; i < h.ntables; ++i)
    if (t[i].nvals < 0 || t[i].nvals > 256) return false;
  m.nseg = h.nseg;
  m.ri = ri;
  m.seg_at = h.seg_at;
  m.tables_at = h.tables_at;
  m.ntables = h.ntables;
  for (int c = 0; c < 4; ++c) {
    m.dc_sel[c] = c < ncomp ? h.dc_sel[c] : 0;
    m.ac_sel[c] = c < ncomp ? h.ac_sel[c] : 0;
  }
  return true;
}

VNF_HD inline const Seg* segs_of(const Frame& f) { return reinterpret_cast<const Seg*>(f.blob + f.meta->seg_at); }

// segment s -> its lanes into seg_lane0[s] (scanned afterwards); an extent outside the blob, or one that begins before
// the segment in front of it ends, marks the frame.  Segments that lie inside the blob one after another hold at most
// blob_bytes bytes together, so their lanes sum to at most lane_cap and the 32-bit total cannot wrap.
VNF_HD inline void plan_seg(const Frame& f, uint32_t s, int subseq_bits) {
  const Seg sg = segs_of(f)[s];
  const uint64_t size = f.blob_bytes, padded = ((uint64_t)sg.bytes + 15u) & ~(uint64_t)15u;
  bool ok = !(sg.at & 15u) && sg.at <= size && padded <= size - sg.at;
  if (ok && s > 0) {
    const Seg before = segs_of(f)[s - 1];
    ok = (uint64_t)sg.at >= (uint64_t)before.at + (((uint64_t)before.bytes + 15u) & ~(uint64_t)15u);
  }
  uint32_t lanes = 1;
  if (!ok) f.meta->invalid = 1;
  else if (sg.bytes) lanes = (uint32_t)(((uint64_t)sg.bytes * 8u + (uint32_t)subseq_bits - 1u) / (uint32_t)subseq_bits);
  f.seg_lane0[s] = lanes;
}

// after the scan: total lanes against the capacity the host sized the workspace for.  One lane.
VNF_HD inline void plan_finish(const Frame& f, uint32_t total) {
  Meta& m = *f.meta;
  f.seg_lane0[m.nseg] = total;
  if (total > f.lane_cap) m.invalid = 1;
  m.nlanes = m.invalid ? 0u : total;
}

// a lane's place -------------------------------------------------------------------------------------------------------
struct Lane {
  const uint32_t* words;   // of the segment
  uint32_t lenbits;        // of the segment
  uint32_t start, end;     // of the subsequence, in bits of the segment
  uint32_t seg, lane0;     // the segment and its first lane
  uint32_t next0;          // first lane of the next segment
};

VNF_HD inline uint32_t seg_of(const Frame& f, uint32_t lane) {   // the last segment whose first lane is at or before `lane`
  uint32_t a = 0, b = f.meta->nseg - 1;
  while (a < b) {
    const uint32_t m = a + (b - a + 1) / 2;
    if (f.seg_lane0[m] <= lane) a = m;
    else b = m - 1;
  }
  return a;
}

VNF_HD inline Lane lane_at(const Frame& f, uint32_t lane, int subseq_bits) {
  Lane l;
  l.seg = seg_of(f, lane);
  l.lane0 = f.seg_lane0[l.seg];
  l.next0 = f.seg_lane0[l.seg + 1];
  const Seg sg = segs_of(f)[l.seg];
  l.words = reinterpret_cast<const uint32_t*>(f.blob + sg.at);
  l.lenbits = sg.bytes * 8u;
  l.start = (lane - l.lane0) * (uint32_t)subseq_bits;
  l.end = l.lenbits - l.start < (uint32_t)subseq_bits ? l.lenbits : l.start + (uint32_t)subseq_bits;
  return l;
}

// MSB-first reader over one segment; bits at and past lenbits are zero and nothing past the segment is loaded
struct Reader {
  const uint32_t* w;
  uint32_t lenbits, pos, wi;
  uint64_t win;   // words wi and wi + 1

  VNF_HD uint32_t word(uint32_t i) const {
    const uint32_t b = i * 32u;
    if (b >= lenbits) return 0;
    uint32_t x = __builtin_bswap32(w[i]);
    if (lenbits - b < 32u) x &= ~0u << (32u - (lenbits - b));
    return x;
  }
  VNF_HD void seek(uint32_t p) {
    pos = p;
    wi = p >> 5;
    win = ((uint64_t)word(wi) << 32) | word(wi + 1);
  }
  VNF_HD uint32_t peek(int n) {   // n in 1..32
    const uint32_t at = pos >> 5;
    if (at == wi + 1u) {   // the common move: one word on, one load
      win = (win << 32) | word(at + 1u);
      wi = at;
    } else if (at != wi) {
      seek(pos);
    }
    return (uint32_t)((win << (pos & 31u)) >> (64 - n));
  }
  VNF_HD void drop(int n) { pos += (uint32_t)n; }
};

// -> symbol, or -1 for a code no table entry matches (or an entry that would consume no bit)
VNF_HD inline int decode_sym(Reader& r, const DTable& t) {
  const unsigned e = t.look[r.peek(kLook)];
  if (e) {
    const int len = (int)(e >> 8);
    if (len < 1 || len > kLook) return -1;
    r.drop(len);
    return (int)(e & 255u);
  }
  for (int l = kLook + 1; l <= 16; ++l) {
    const int code = (int)r.peek(l);
    if (code <= t.maxcode[l]) {
      const int idx = t.valoff[l] + code;
      if (idx < 0 || idx >= t.nvals) return -1;
      r.drop(l);
      return t.vals[idx];
    }
  }
  return -1;
}

VNF_HD inline int receive_extend(Reader& r, int s) {   // s in 1..15
  const int v = (int)r.peek(s);
  r.drop(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

enum Step { kSymbol = 0, kUnitDone = 1, kBad = 2 };

// One symbol of the unit `unit` (inside its MCU) at zigzag index k; put(k, value) receives a non-zero coefficient
// (k = 0: the DC difference).  At least one and at most 31 bits are consumed unless the result is kBad.
template <class Put>
VNF_HD inline Step step(Reader& r, const DTable* tabs, const Sel& sel, int& unit, int& k, Put&& put) {
  const int c = unit < sel.luma ? 0 : 1 + unit - sel.luma;
  if (k == 0) {
    const int s = decode_sym(r, tabs[sel.dc[c]]);
    if (s < 0 || s > 15) return kBad;
    if (s) put(0, receive_extend(r, s));
    k = 1;
    return kSymbol;
  }
  const int rs = decode_sym(r, tabs[sel.ac[c]]);
  if (rs < 0) return kBad;
  const int run = rs >> 4, s = rs & 15;
  if (s == 0) {
    if (run == 15) {
      k += 16;
      if (k > 64) return kBad;   // a run past the block
    } else {
      k = 64;                    // end of block
    }
  } else {
    k += run;
    if (k > 63) return kBad;
    put(k, receive_extend(r, s));
    ++k;
  }
  if (k < 64) return kSymbol;
  k = 0;
  unit = unit + 1 == sel.upm ? 0 : unit + 1;
  return kUnitDone;
}

// Decodes lane `l` from the packed state `entry` to the first symbol boundary at or past its end -> exit state.  Reads
// the segment, writes nothing.  Any 32-bit value is a harmless entry.
VNF_HD inline uint32_t run_lane(const Lane& l, const DTable* tabs, const Sel& sel, uint32_t entry) {
  entry &= kStateMask;
  int unit = (int)((entry >> 5) & 15u), k = (int)((entry >> 9) & 63u);
  if ((entry & kDead) || unit >= sel.upm) return kDead;
  Reader r{l.words, l.lenbits, 0, 0, 0};
  r.seek(l.start + (entry & 31u));
  while (r.pos < l.end)
    if (step(r, tabs, sel, unit, k, [](int, int) {}) == kBad) return kDead;
  return pack_state(r.pos - l.end, unit, k) | (r.pos > l.lenbits ? kOver : 0u);
}

// speculate pass -------------------------------------------------------------------------------------------------------
VNF_HD inline void speculate_lane(const Frame& f, const DTable* tabs, const Sel& sel, uint32_t lane, int subseq_bits) {
  f.state[lane] = run_lane(lane_at(f, lane, subseq_bits), tabs, sel, 0u);
}

// synchronise pass, level 1: one round of one lane.  entry: the exit state of the lane before it as the round began (0
// for the first lane of a load); used: the entry `st` was decoded from.  -> st changed
VNF_HD inline bool resync_lane(const Lane& l, const DTable* tabs, const Sel& sel, uint32_t entry, uint32_t* used, uint32_t* st) {
  if (entry == *used) return false;
  *used = entry;
  const uint32_t n = run_lane(l, tabs, sel, entry);
  const bool changed = n != *st;
  *st = n;
  return changed;
}

// synchronise pass, level 2: one round of the load [first, first + kLoad).  entry: the exit state of the load before it
// as the round began.  Walks the load's lanes from `entry` until one's exit state comes out as recorded.  Writes state
// slots of its own load only.  -> the load's exit state (that of its last lane)
VNF_HD inline uint32_t resync_load(const Frame& f, const DTable* tabs, const Sel& sel, uint32_t first, int subseq_bits,
                                   uint32_t entry, uint32_t* used) {
  const uint32_t nlanes = f.meta->nlanes, stop = nlanes - first < (uint32_t)kLoad ? nlanes : first + (uint32_t)kLoad;
  Lane l = lane_at(f, first, subseq_bits);
  if (entry != *used && first != l.lane0) {          // a load that begins with a head has its true entry already
    *used = entry;
    for (uint32_t i = first; i < stop && i != l.next0; ++i) {
      if (i != first) {
        l.start += (uint32_t)subseq_bits;
        l.end = l.lenbits - l.start < (uint32_t)subseq_bits ? l.lenbits : l.start + (uint32_t)subseq_bits;
      }
      const uint32_t n = run_lane(l, tabs, sel, entry);
      if (n == f.state[i]) break;                    // from here on the load is what it was
      f.state[i] = n;
      entry = n;
    }
  }
  return f.state[stop - 1];
}

// the true entry of a lane once the synchronise pass is through
VNF_HD inline uint32_t true_entry(const Frame& f, const Lane& l, uint32_t lane) { return lane == l.lane0 ? 0u : f.state[lane - 1]; }

// count pass -----------------------------------------------------------------------------------------------------------
VNF_HD inline void count_lane(const Frame& f, const DTable* tabs, const Sel& sel, uint32_t lane, int subseq_bits) {
  const Lane l = lane_at(f, lane, subseq_bits);
  const uint32_t entry = true_entry(f, l, lane) & kStateMask;
  uint32_t n = 0;
  int unit = (int)((entry >> 5) & 15u), k = (int)((entry >> 9) & 63u);
  if (!(entry & kDead) && unit < sel.upm) {
    Reader r{l.words, l.lenbits, 0, 0, 0};
    r.seek(l.start + (entry & 31u));
    while (r.pos < l.end) {
      const Step s = step(r, tabs, sel, unit, k, [](int, int) {});
      if (s == kBad) break;
      n += s == kUnitDone;
    }
  }
  f.cnt[lane] = n;
}

// write pass -----------------------------------------------------------------------------------------------------------
// where the DC difference of unit u sits in dctmp: the components one after another, each in scan order
VNF_HD inline uint32_t dc_index(const Geom& g, uint32_t mcus, uint32_t u) {
  const uint32_t m = u / (uint32_t)g.upm, r = u % (uint32_t)g.upm, luma = (uint32_t)(g.h0 * g.v0);
  return r < luma ? m * luma + r : mcus * luma + (r - luma) * mcus + m;
}

VNF_HD inline void write_lane(const Geom& g, const Frame& f, const DTable* tabs, const Sel& sel, uint32_t mcus, uint32_t lane,
                              int subseq_bits) {
  const Lane l = lane_at(f, lane, subseq_bits);
  const Meta& m = *f.meta;
  const uint32_t per_seg = m.ri * (uint32_t)g.upm, base = l.seg * per_seg;
  const bool final = l.seg + 1 == m.nseg;
  const uint32_t share = final ? g.units - base : per_seg;   // plan_header: nseg = ceil(mcus / ri), so base < units
  uint32_t local = f.cnt[lane] - f.cnt[l.lane0];              // units of the segment before this lane
  const uint32_t entry = true_entry(f, l, lane) & kStateMask;
  int unit = (int)((entry >> 5) & 15u), k = (int)((entry >> 9) & 63u);
  if ((entry & kDead) || unit >= sel.upm) {
    if (local < share) f.meta->invalid = 1;
    return;
  }
  Reader r{l.words, l.lenbits, 0, 0, 0};
  r.seek(l.start + (entry & 31u));
  while (r.pos < l.end && local < share) {
    const uint32_t u = base + local;
    int c;
    const long long at = huff::unit_block(g, u, &c);
    const Step s = step(r, tabs, sel, unit, k, [&](int kk, int v) {
      const long long o = at + huff::kZigzag[kk];
      if (o >= 0 && o < f.coef_count) f.coefs[o] = (int16_t)v;
      if (kk == 0) f.dctmp[dc_index(g, mcus, u)] = (uint32_t)v;
    });
    if (s == kBad) {
      f.meta->invalid = 1;
      return;
    }
    if (s == kUnitDone) {
      ++local;
      // the unit read invented bits; or a restart interval ends with a whole byte or more to spare
      if (r.pos > l.lenbits || (local == share && !final && l.lenbits - r.pos >= 8u)) {
        f.meta->invalid = 1;
        return;
      }
    }
  }
  if (lane + 1 == l.next0 && local < share) f.meta->invalid = 1;   // the segment ran out before its share
}

// dc pass --------------------------------------------------------------------------------------------------------------
// Sums are taken modulo 2^32 over all components at once and differenced at the restart interval's first unit.  That is
// exact: every difference is an int16, so while the values before it are int16 the next one is within +-65535 and
// shows as it is, and the first one outside int16 fails the frame.
VNF_HD inline void dc_unit(const Geom& g, const Frame& f, uint32_t mcus, uint32_t u) {
  const uint32_t luma = (uint32_t)(g.h0 * g.v0), m = u / (uint32_t)g.upm, r = u % (uint32_t)g.upm, ri = f.meta->ri;
  const uint32_t m0 = ri ? m / ri * ri : 0u;
  const uint32_t j = dc_index(g, mcus, u);
  const uint32_t j0 = r < luma ? m0 * luma : mcus * luma + (r - luma) * mcus + m0;
  int c;
  const long long at = huff::unit_block(g, u, &c);
  if (at < 0 || at >= f.coef_count) return;
  const int32_t v = (int32_t)(f.dctmp[j] - f.dctmp[j0]) + f.coefs[at];
  if (v < -32768 || v > 32767) f.meta->invalid = 1;
  f.coefs[at] = (int16_t)v;
}

// host side: geometry and workspace ------------------------------------------------------------------------------------
inline Geom make_geom(const vnf_jpeg_info& info, const JpegGeom& jg) {
  Geom g;
  g.h0 = info.components == 1 ? 1 : info.h[0];
  g.v0 = info.components == 1 ? 1 : info.v[0];
  g.mx = jg.bw[0] / g.h0;
  g.upm = info.components == 1 ? 1 : g.h0 * g.v0 + 2;
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = jg.bw[c];
    g.plane[c] = jg.plane_off[c];
  }
  g.units = (unsigned)jg.blocks;
  return g;
}

// the workspace of n frames: [meta n | dctmp n x dc_stride (the zeroed part ends here) | seg_lane0 n x seg_stride |
// state n x lane_cap | cnt n x lane_cap], every part 16-byte aligned, the strides multiples of 4 entries
struct Layout {
  long long lane_cap, seg_cap, seg_stride, dc_stride;
  long long dc_at, seg_lane_at, state_at, cnt_at, bytes;
};

// false: a geometry or a blob too large for 32-bit bit positions and unit indices
inline bool layout(int n, const JpegGeom& jg, const Geom& g, long long max_blob_bytes, int subseq_bits, Layout* l) {
  if (max_blob_bytes < 0 || max_blob_bytes > kMaxBlobBytes || jg.blocks >= (1LL << 28)) return false;
  l->seg_cap = jg.blocks / g.upm;   // one segment per MCU at the most
  l->lane_cap = huff::round_up((max_blob_bytes * 8 + subseq_bits - 1) / subseq_bits + l->seg_cap + 1, kLoad);
  l->seg_stride = huff::round_up(l->seg_cap + 1, 4) + 4;
  l->dc_stride = huff::round_up(jg.blocks, 4);
  l->dc_at = (long long)n * (long long)sizeof(Meta);
  l->seg_lane_at = l->dc_at + 4LL * n * l->dc_stride;
  l->state_at = l->seg_lane_at + 4LL * n * l->seg_stride;
  l->cnt_at = l->state_at + 4LL * n * l->lane_cap;
  l->bytes = l->cnt_at + 4LL * n * l->lane_cap;
  return true;
}

inline bool subseq_ok(int subseq_bits) {
  return subseq_bits >= kMinSubseqBits && subseq_bits <= kMaxSubseqBits && subseq_bits % 32 == 0;
}

}  // namespace hdec
}  // namespace vnf
