// Host half of the JPEG frame decoder: the marker walk and the Huffman (entropy) decode of a baseline frame, the part
// of a JPEG that is serial per frame.  Output: quantised coefficients in natural order, ready for the device kernels of
// jpeg_decode.hip (dequantisation, IDCT, upsampling, colour).
//
// Replaces, together with those kernels, the reference's cv2.VideoCapture.read (/root/reference/demo_video.py:78-110)
// for Motion-JPEG input.  Written from the JPEG standard (ITU-T T.81: B.2 marker segments, C Huffman table
// generation, F.2.2 decoding procedures); no HIP call and no dependency on the rest of the library but headers, so the
// file also compiles into stand-alone checkers (tools/jpeg_entropy_check.cpp, tools/jpeg_huff_decode_check.cpp).  For the
// device Huffman decoder (jpeg_huff_decode.hip) the same marker walk PREPARES a frame instead of decoding it
// (vnf_jpeg_huff_prepare, at the end of the file).  The input is a file from disk: every read is
// checked against `len`, every write against `capacity`, and no state is shared between calls (thread-safe).
#include <stdint.h>
#include <string.h>

#include <new>

#include "../../include/vnface.h"
#include "jpeg_huff_decode.h"

namespace {

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK = 10;  // bits of the one-step code lookup; longer codes walk maxcode[]

struct Huff {
  bool set = false;
  uint16_t look[1 << LOOK];  // (length << 8) | symbol for codes of at most LOOK bits, 0: longer
  int32_t fast[1 << LOOK];   // AC tables: (value << 8) | (run << 4) | bits when code AND magnitude fit LOOK bits, else 0
  int32_t maxcode[18];       // largest code of each length, -1: none
  int32_t valoff[17];        // index of the first symbol of a length minus its first code
  uint8_t vals[256];
  int nvals = 0;
};

struct Parsed {
  vnf_jpeg_info info;
  Huff dc[4], ac[4];
  int td[3], ta[3];
  int64_t scan;  // offset of the first entropy-coded byte
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// T.81 annex C: code lengths -> canonical codes.  false: the lengths over-subscribe the code space.
bool build_huff(Huff& h, const uint8_t counts[16], const uint8_t* syms, int nsyms) {
  memset(h.look, 0, sizeof(h.look));
  memcpy(h.vals, syms, nsyms);
  h.nvals = nsyms;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = counts[l - 1];
    h.valoff[l] = k - code;
    if (code + n > (1 << l)) return false;
    for (int i = 0; i < n; ++i, ++k, ++code) {
      if (l <= LOOK) {
        const int first = code << (LOOK - l), span = 1 << (LOOK - l);
        for (int j = 0; j < span; ++j) h.look[first + j] = (uint16_t)((l << 8) | syms[k]);
      }
    }
    h.maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
  h.maxcode[17] = 0x7fffffff;
  // a run/size symbol whose magnitude bits are inside the looked-up bits too: the coefficient in one step
  for (int i = 0; i < (1 << LOOK); ++i) {
    h.fast[i] = 0;
    const int e = h.look[i], len = e >> 8, run = (e >> 4) & 15, size = e & 15;
    if (!e || !size || len + size > LOOK) continue;
    int v = (i >> (LOOK - len - size)) & ((1 << size) - 1);
    if (v < (1 << (size - 1))) v -= (1 << size) - 1;
    h.fast[i] = v * 256 + (run << 4) + (len + size);
  }
  h.set = true;
  return true;
}

// Marker walk up to the first SOS.  VNF_OK / VNF_E_INVALID / VNF_JPEG_NOT_TAKEN.
int parse(const uint8_t* d, int64_t len, Parsed& P) {
  if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) return VNF_E_INVALID;
  vnf_jpeg_info& I = P.info;
  memset(&I, 0, sizeof(I));
  uint8_t qt[4][64];
  bool qset[4] = {false, false, false, false};
  int tq[3] = {0, 0, 0}, cid[3] = {0, 0, 0};
  bool sof = false, any_dht = false, adobe_rgb = false;
  int64_t p = 2;
  for (;;) {
    if (p + 2 > len) return VNF_E_INVALID;
    if (d[p] != 0xFF) return VNF_E_INVALID;
    while (p + 1 < len && d[p + 1] == 0xFF) ++p;  // fill bytes before a marker
    if (p + 2 > len) return VNF_E_INVALID;
    const int m = d[p + 1];
    p += 2;
    if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x00 || m == 0x01) return VNF_E_INVALID;
    if (p + 2 > len) return VNF_E_INVALID;
    const int L = be16(d + p);
    if (L < 2 || p + L > len) return VNF_E_INVALID;
    const uint8_t* s = d + p + 2;
    const int n = L - 2;
    if (m == 0xC0) {
      if (sof || n < 6) return VNF_E_INVALID;
      const int prec = s[0], nc = s[5];
      I.height = be16(s + 1);
      I.width = be16(s + 3);
      if (n != 6 + 3 * nc || nc < 1 || I.width < 1) return VNF_E_INVALID;
      if (prec != 8 || I.height < 1 || (nc != 1 && nc != 3)) return VNF_JPEG_NOT_TAKEN;  // 12-bit, DNL height, CMYK
      for (int c = 0; c < nc; ++c) {
        cid[c] = s[6 + 3 * c];
        I.h[c] = s[7 + 3 * c] >> 4;
        I.v[c] = s[7 + 3 * c] & 15;
        tq[c] = s[8 + 3 * c];
        if (I.h[c] < 1 || I.h[c] > 4 || I.v[c] < 1 || I.v[c] > 4 || tq[c] > 3) return VNF_E_INVALID;
      }
      I.components = nc;
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8) {
      return VNF_JPEG_NOT_TAKEN;  // extended, progressive, lossless, arithmetic (SOF1..15, DAC)
    } else if (m == 0xC4) {
      int q = 0;
      while (q < n) {
        if (q + 17 > n) return VNF_E_INVALID;
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return VNF_E_INVALID;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
        if (total > 256 || q + 17 + total > n) return VNF_E_INVALID;
        if (!build_huff(tc ? P.ac[th] : P.dc[th], s + q + 1, s + q + 17, total)) return VNF_E_INVALID;
        any_dht = true;
        q += 17 + total;
      }
    } else if (m == 0xDB) {
      int q = 0;
      while (q < n) {
        const int pq = s[q] >> 4, t = s[q] & 15;
        if (pq > 1 || t > 3) return VNF_E_INVALID;
        if (pq == 1) return VNF_JPEG_NOT_TAKEN;  // 16-bit table
        if (q + 65 > n) return VNF_E_INVALID;
        for (int k = 0; k < 64; ++k) qt[t][kZigzag[k]] = s[q + 1 + k];
        qset[t] = true;
        q += 65;
      }
    } else if (m == 0xEE) {
      // Adobe APP14, transform 0: the three components are RGB, not YCbCr
      if (n >= 12 && memcmp(s, "Adobe", 5) == 0 && s[11] == 0) adobe_rgb = true;
    } else if (m == 0xDD) {
      if (n != 2) return VNF_E_INVALID;
      I.restart_interval = be16(s);
    } else if (m == 0xDA) {
      if (!sof || n < 1) return VNF_E_INVALID;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * ns) return VNF_E_INVALID;
      if (ns != I.components) return VNF_JPEG_NOT_TAKEN;  // one component per scan: more than one scan
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != cid[c]) return VNF_JPEG_NOT_TAKEN;  // components out of frame order
        P.td[c] = s[2 + 2 * c] >> 4;
        P.ta[c] = s[2 + 2 * c] & 15;
        if (P.td[c] > 3 || P.ta[c] > 3) return VNF_E_INVALID;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return VNF_E_INVALID;  // Ss, Se, Ah/Al
      if (!any_dht) return VNF_JPEG_NOT_TAKEN;  // abbreviated frame: the tables live elsewhere
      if (ns == 3 && (adobe_rgb || (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B'))) return VNF_JPEG_NOT_TAKEN;
      for (int c = 0; c < ns; ++c) {
        if (!P.dc[P.td[c]].set || !P.ac[P.ta[c]].set || !qset[tq[c]]) return VNF_E_INVALID;
        memcpy(I.quant[c], qt[tq[c]], 64);
      }
      P.scan = p + L;
      break;
    }
    // APPn, COM and anything else with a length: skipped
    p += L;
  }
  // geometry
  if (I.components == 1) {
    I.h[0] = I.v[0] = 1;  // a single component is never interleaved: its factors do not shape the block grid
    I.sampling = VNF_JPEG_GRAY;
  } else {
    if (I.h[1] != 1 || I.v[1] != 1 || I.h[2] != 1 || I.v[2] != 1) return VNF_JPEG_NOT_TAKEN;
    if (I.h[0] == 1 && I.v[0] == 1) I.sampling = VNF_JPEG_444;
    else if (I.h[0] == 2 && I.v[0] == 1) I.sampling = VNF_JPEG_422;
    else if (I.h[0] == 2 && I.v[0] == 2) I.sampling = VNF_JPEG_420;
    else return VNF_JPEG_NOT_TAKEN;
  }
  const int mw = 8 * I.h[0], mh = 8 * I.v[0];
  const int mx = (I.width + mw - 1) / mw, my = (I.height + mh - 1) / mh;
  I.coef_count = 0;
  for (int c = 0; c < I.components; ++c) {
    I.blocks_w[c] = mx * I.h[c];
    I.blocks_h[c] = my * I.v[c];
    I.coef_count += (int64_t)64 * I.blocks_w[c] * I.blocks_h[c];
  }
  return VNF_OK;
}

// MSB-first bit reader over the entropy-coded segment.  It never moves past a marker (FF xx, xx != 00) or past `end`:
// from there on it supplies zero bits and counts them in `fake`, and a caller that has consumed one of them
// (`overrun()`) has a truncated stream.
struct Bits {
  const uint8_t* d;
  int64_t p, end;
  uint64_t acc = 0;
  int n = 0;     // valid bits in acc (the low n)
  int fake = 0;  // how many of them, at the low end, are invented zeros

  void fill() {
    if (n <= 32 && p + 8 <= end) {
      // eight bytes at once when none of them is FF (no stuffing, no marker): the common case
      uint64_t be = 0;
      for (int i = 0; i < 8; ++i) be = (be << 8) | d[p + i];
      const uint64_t x = ~be;
      if (!((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull)) {  // no zero byte in ~be
        const int k = (64 - n) >> 3;  // whole bytes that fit: 4..8
        acc = k == 8 ? be : (acc << (8 * k)) | (be >> (64 - 8 * k));
        n += 8 * k;
        p += k;
        return;
      }
    }
    while (n <= 56) {
      unsigned b = 0;
      bool real = false;
      while (p < end) {
        b = d[p];
        if (b != 0xFF) { ++p; real = true; break; }
        if (p + 1 >= end) break;                         // a lone FF at the end: truncated
        const unsigned nx = d[p + 1];
        if (nx == 0x00) { p += 2; real = true; break; }  // stuffed FF
        if (nx == 0xFF) { ++p; continue; }               // fill byte
        break;                                           // a marker: stay in front of it
      }
      acc = (acc << 8) | (real ? b : 0u);
      n += 8;
      if (!real && fake < (1 << 20)) fake += 8;  // p does not move again once it is stuck, so these stay the low bits
    }
  }
  bool overrun() const { return n < fake; }
  unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
  void drop(int k) { n -= k; }
  void reset() { acc = 0; n = 0; fake = 0; }
};

// -> symbol, or -1 for a code no table entry matches
inline int decode_sym(Bits& b, const Huff& h) {
  const unsigned e = h.look[b.peek(LOOK)];
  if (e) {
    b.drop(e >> 8);
    return e & 255;
  }
  for (int l = LOOK + 1; l <= 16; ++l) {
    const int code = (int)b.peek(l);
    if (code <= h.maxcode[l]) {
      const int idx = h.valoff[l] + code;
      if (idx < 0 || idx >= h.nvals) return -1;
      b.drop(l);
      return h.vals[idx];
    }
  }
  return -1;
}

inline int receive_extend(Bits& b, int s) {
  const int v = (int)b.peek(s);
  b.drop(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace

extern "C" int vnf_jpeg_probe(const uint8_t* data, int64_t len, vnf_jpeg_info* info) {
  if (!data || !info || len < 0) return VNF_E_INVALID;
  Parsed* P = new (std::nothrow) Parsed;
  if (!P) return VNF_E_INVALID;
  const int rc = parse(data, len, *P);
  if (rc == VNF_OK) *info = P->info;
  delete P;
  return rc;
}

extern "C" int vnf_jpeg_entropy_decode(const uint8_t* data, int64_t len, const vnf_jpeg_info* info, int16_t* coefs,
                                       int64_t capacity) {
  if (!data || !info || !coefs || len < 0 || capacity < 0) return VNF_E_INVALID;
  Parsed* P = new (std::nothrow) Parsed;
  if (!P) return VNF_E_INVALID;
  int rc = parse(data, len, *P);
  if (rc != VNF_OK) {
    delete P;
    return VNF_E_INVALID;
  }
  const vnf_jpeg_info& I = P->info;
  // the caller's info sized the buffers: it has to be the one these bytes give
  if (I.width != info->width || I.height != info->height || I.components != info->components ||
      I.sampling != info->sampling || I.coef_count != info->coef_count) {
    delete P;
    return VNF_E_INVALID;
  }
  if (I.coef_count > capacity) {
    delete P;
    return VNF_E_CAPACITY;
  }
  int64_t plane[3] = {0, 0, 0};
  for (int c = 1; c < I.components; ++c) plane[c] = plane[c - 1] + (int64_t)64 * I.blocks_w[c - 1] * I.blocks_h[c - 1];
  const int mx = I.blocks_w[0] / I.h[0], my = I.blocks_h[0] / I.v[0];
  Bits b{data, P->scan, len};
  int pred[3] = {0, 0, 0};
  int left = I.restart_interval, rst = 0;
  rc = VNF_OK;
  for (int y = 0; y < my && rc == VNF_OK; ++y) {
    for (int x = 0; x < mx && rc == VNF_OK; ++x) {
      if (I.restart_interval && left == 0) {
        // an interval ends on a byte boundary: under 8 padding bits may be left, then RSTn in sequence
        if (b.overrun() || b.n - b.fake >= 8 || b.p + 2 > len || data[b.p] != 0xFF || data[b.p + 1] != 0xD0 + (rst & 7)) {
          rc = VNF_E_INVALID;
          break;
        }
        b.p += 2;
        b.reset();
        rst++;
        pred[0] = pred[1] = pred[2] = 0;
        left = I.restart_interval;
      }
      for (int c = 0; c < I.components && rc == VNF_OK; ++c) {
        const Huff& hd = P->dc[P->td[c]];
        const Huff& ha = P->ac[P->ta[c]];
        for (int by = 0; by < I.v[c] && rc == VNF_OK; ++by) {
          for (int bx = 0; bx < I.h[c]; ++bx) {
            const int64_t off = plane[c] + ((int64_t)(y * I.v[c] + by) * I.blocks_w[c] + (x * I.h[c] + bx)) * 64;
            if (off < 0 || off + 64 > capacity) { rc = VNF_E_INVALID; break; }
            int16_t* blk = coefs + off;
            memset(blk, 0, 64 * sizeof(int16_t));
            if (b.n < 32) b.fill();
            int s = decode_sym(b, hd);
            if (s < 0 || s > 15) { rc = VNF_E_INVALID; break; }
            if (s) pred[c] += receive_extend(b, s);
            if (pred[c] < -32768 || pred[c] > 32767) { rc = VNF_E_INVALID; break; }
            blk[0] = (int16_t)pred[c];
            int k = 1;
            while (k < 64) {
              if (b.n < 32) b.fill();
              const int32_t f = ha.fast[b.peek(LOOK)];
              if (f) {
                k += (f >> 4) & 15;
                if (k > 63) { rc = VNF_E_INVALID; break; }
                blk[kZigzag[k]] = (int16_t)(f >> 8);
                b.drop(f & 15);
                ++k;
                continue;
              }
              const int rs = decode_sym(b, ha);
              if (rs < 0) { rc = VNF_E_INVALID; break; }
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;  // end of block
                k += 16;
                continue;
              }
              k += r;
              if (k > 63) { rc = VNF_E_INVALID; break; }
              blk[kZigzag[k]] = (int16_t)receive_extend(b, s);
              ++k;
            }
            if (rc == VNF_OK && (k > 64 || b.overrun())) rc = VNF_E_INVALID;  // a run past the block; invented bits
            if (rc != VNF_OK) break;
          }
        }
      }
      --left;
    }
  }
  delete P;
  return rc;
}

// ---- the frame prepared for the device Huffman decoder (the blob of jpeg_huff_decode.h) ----------------------------------

namespace {

using namespace vnf::hdec;

// writes into out[0, capacity) only; `ok` goes false at the first byte that does not fit
struct BlobOut {
  uint8_t* out;
  int64_t capacity, at = 0;
  bool ok = true;
  void put(const void* src, int64_t n) {
    if (!ok || n > capacity - at) { ok = false; return; }
    if (n) memcpy(out + at, src, (size_t)n);
    at += n;
  }
  void zeros(int64_t n) {
    if (!ok || n > capacity - at) { ok = false; return; }
    if (n) memset(out + at, 0, (size_t)n);
    at += n;
  }
};

void device_table(const Huff& h, DTable* t) {
  memset(t, 0, sizeof(*t));
  memcpy(t->look, h.look, sizeof(t->look));
  for (int l = 1; l <= 17; ++l) t->maxcode[l] = h.maxcode[l];   // [0] of both is never set and never read
  for (int l = 1; l <= 16; ++l) t->valoff[l] = h.valoff[l];
  t->nvals = h.nvals;
  memcpy(t->vals, h.vals, (size_t)h.nvals);
}

}  // namespace

extern "C" int64_t vnf_jpeg_huff_prepared_bound(int64_t len, const vnf_jpeg_info* info) {
  if (!info || len < 0 || info->components < 1 || info->components > 3 || info->h[0] < 1 || info->v[0] < 1 ||
      info->restart_interval < 0)
    return VNF_E_INVALID;
  return prepared_bound(len, *info);
}

extern "C" int vnf_jpeg_huff_prepare(const uint8_t* data, int64_t len, const vnf_jpeg_info* info, uint8_t* out,
                                     int64_t capacity, int64_t* len_out) {
  if (!data || !info || !out || !len_out || len < 0 || capacity < 0) return VNF_E_INVALID;
  Parsed* P = new (std::nothrow) Parsed;
  if (!P) return VNF_E_INVALID;
  int rc = parse(data, len, *P);
  const vnf_jpeg_info& I = P->info;
  if (rc != VNF_OK || I.width != info->width || I.height != info->height || I.components != info->components ||
      I.sampling != info->sampling || I.coef_count != info->coef_count) {
    delete P;
    return VNF_E_INVALID;
  }
  const int64_t nseg = segments_of(I);
  // the tables the scan's components select, each once: DC tables first
  BlobHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = kMagic;
  h.nseg = (uint32_t)nseg;
  h.restart_interval = (uint32_t)I.restart_interval;
  h.ncomp = (uint32_t)I.components;
  int slot_dc[4] = {-1, -1, -1, -1}, slot_ac[4] = {-1, -1, -1, -1};
  const Huff* used[kMaxTables];
  int nt = 0;
  for (int c = 0; c < I.components; ++c)
    if (slot_dc[P->td[c]] < 0) { slot_dc[P->td[c]] = nt; used[nt++] = &P->dc[P->td[c]]; }
  for (int c = 0; c < I.components; ++c)
    if (slot_ac[P->ta[c]] < 0) { slot_ac[P->ta[c]] = nt; used[nt++] = &P->ac[P->ta[c]]; }
  for (int c = 0; c < I.components; ++c) {
    h.dc_sel[c] = (uint8_t)slot_dc[P->td[c]];
    h.ac_sel[c] = (uint8_t)slot_ac[P->ta[c]];
  }
  h.ntables = (uint32_t)nt;
  h.tables_at = (uint32_t)sizeof(BlobHeader);
  h.seg_at = h.tables_at + (uint32_t)nt * (uint32_t)sizeof(DTable);
  const int64_t data_at = round16((int64_t)h.seg_at + nseg * (int64_t)sizeof(Seg));
  h.data_at = (uint32_t)data_at;
  rc = VNF_OK;
  if (data_at + round16(len) + 16 * nseg > kMaxBlobBytes) rc = VNF_E_INVALID;   // 32-bit bit positions on the device
  BlobOut o{out, capacity};
  if (rc == VNF_OK) {
    o.zeros(data_at);   // header, tables and segment table: filled in below, once they are known to fit
    if (o.ok) {
      DTable* t = new (std::nothrow) DTable;
      if (!t) rc = VNF_E_INVALID;
      for (int i = 0; i < nt && t; ++i) {
        device_table(*used[i], t);
        memcpy(out + h.tables_at + (int64_t)i * (int64_t)sizeof(DTable), t, sizeof(DTable));
      }
      delete t;
    }
  }
  // the scan: runs without FF are copied as they are; FF 00 -> FF, FF FF -> a fill byte, FF xx -> a marker
  int64_t p = P->scan;
  for (int64_t s = 0; s < nseg && rc == VNF_OK && o.ok; ++s) {
    const int64_t at = o.at;
    int marker = -1;
    while (o.ok) {
      const uint8_t* q = p < len ? (const uint8_t*)memchr(data + p, 0xFF, (size_t)(len - p)) : nullptr;
      const int64_t run = q ? q - (data + p) : len - p;
      o.put(data + p, run);
      p += run;
      if (!q || p + 1 >= len) { p = len; break; }       // the end of the data; a lone FF there is no data
      const int nx = data[p + 1];
      if (nx == 0x00) { o.put(data + p, 1); p += 2; }   // a stuffed FF
      else if (nx == 0xFF) ++p;                         // a fill byte
      else { marker = nx; break; }
    }
    if (!o.ok) break;
    const Seg sg = {(uint32_t)at, (uint32_t)(o.at - at)};
    memcpy(out + h.seg_at + s * (int64_t)sizeof(Seg), &sg, sizeof(sg));
    o.zeros(round16(o.at) - o.at);
    if (s + 1 < nseg) {
      if (marker != 0xD0 + (int)(s & 7)) rc = VNF_E_INVALID;   // a restart interval ends with RSTn in sequence
      p += 2;
    }
  }
  if (rc == VNF_OK && !o.ok) rc = VNF_E_CAPACITY;
  if (rc == VNF_OK) {
    h.total_bytes = (uint32_t)o.at;
    memcpy(out, &h, sizeof(h));
    *len_out = o.at;
  }
  delete P;
  return rc;
}
