// Host half of the JPEG frame encoder: quantisation tables, the geometry of a frame to be written, and the Huffman
// (entropy) pass that turns the quantised coefficients of jpeg_encode.hip into a complete baseline JFIF file -- the part
// of a JPEG that is serial per frame.  It is jpeg_entropy.cpp run backwards: the same coefficient layout goes in that
// vnf_jpeg_entropy_decode writes.
//
// Replaces, together with those kernels, the reference's cv2.VideoWriter (/root/reference/demo_video.py:25-43) for
// Motion-JPEG output.  Written from the JPEG standard (ITU-T T.81: B.2 marker segments, C Huffman table generation,
// F.1.2 encoding procedures, K.1 / K.3 the "typical" quantisation and Huffman tables) and the JFIF 1.01 APP0 layout; the
// quality scaling of the tables is libjpeg's public rule.  No HIP call and no dependency on the rest of the library, so
// the file also compiles into the stand-alone checkers (tools/jpeg_huff_encode_check.cpp, tools/jpeg_huff_device_check.cpp).  Every write is checked against
// `capacity`, and no state is shared between calls (thread-safe).
#include <stdint.h>
#include <string.h>

#include "../../include/vnface.h"
#include "jpeg_huff_tables.h"

namespace {

using namespace vnf::huff;   // zigzag order, annex K.3 tables and codes, the walk over a block

// T.81 K.1: luminance, chrominance, natural order
constexpr uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Byte sink over out[0, cap): a byte past the end is counted, not written.
struct Sink {
  uint8_t* out;
  int64_t cap, pos = 0;
  uint64_t acc = 0;  // bit accumulator of the scan, the low n bits are pending
  int n = 0;

  void byte(unsigned b) {
    if (pos < cap) out[pos] = (uint8_t)b;
    ++pos;
  }
  void be16(unsigned v) { byte(v >> 8); byte(v & 255); }
  void bytes(const uint8_t* p, int k) { for (int i = 0; i < k; ++i) byte(p[i]); }
  // scan bits, MSB first, k <= 32; FF is followed by a stuffed 00 (T.81 F.1.2.3)
  void bits(uint32_t v, int k) {
    acc = (acc << k) | (v & (uint32_t)((1ull << k) - 1ull));
    n += k;
    if (n < 32) return;
    // four bytes at once when none of them is FF and they fit: the common case
    const uint32_t w = (uint32_t)(acc >> (n - 32));
    if (pos + 4 <= cap && !((~w - 0x01010101u) & w & 0x80808080u)) {   // no zero byte in ~w
      out[pos] = (uint8_t)(w >> 24);
      out[pos + 1] = (uint8_t)(w >> 16);
      out[pos + 2] = (uint8_t)(w >> 8);
      out[pos + 3] = (uint8_t)w;
      pos += 4;
      n -= 32;
      return;
    }
    drain();
  }
  void drain() {
    while (n >= 8) {
      const unsigned b = (unsigned)(acc >> (n - 8)) & 255u;
      byte(b);
      if (b == 0xFF) byte(0);
      n -= 8;
    }
  }
  void flush() {
    drain();
    if (n) {                   // the last byte is padded with 1-bits
      bits(0x7F, 8 - n);
      drain();
    }
  }
};

bool geometry(int width, int height, int sampling, int* h0, int* v0, int bw[3], int bh[3], int64_t* count) {
  switch (sampling) {
    case VNF_JPEG_444: *h0 = 1; *v0 = 1; break;
    case VNF_JPEG_422: *h0 = 2; *v0 = 1; break;
    case VNF_JPEG_420: *h0 = 2; *v0 = 2; break;
    default: return false;
  }
  if (width < 1 || width > 65535 || height < 1 || height > 65535) return false;
  const int mx = (width + 8 * *h0 - 1) / (8 * *h0), my = (height + 8 * *v0 - 1) / (8 * *v0);
  *count = 0;
  for (int c = 0; c < 3; ++c) {
    bw[c] = mx * (c ? 1 : *h0);
    bh[c] = my * (c ? 1 : *v0);
    *count += (int64_t)64 * bw[c] * bh[c];
  }
  return true;
}

}  // namespace

extern "C" int vnf_jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
  if (quality < 1 || quality > 100 || !luma || !chroma) return VNF_E_INVALID;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t) {
    uint8_t* dst = t ? chroma : luma;
    for (int i = 0; i < 64; ++i) {
      int v = (kBaseQuant[t][i] * scale + 50) / 100;
      dst[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
  }
  return VNF_OK;
}

extern "C" int vnf_jpeg_encode_info(int width, int height, int sampling, int quality, vnf_jpeg_info* out) {
  if (!out) return VNF_E_INVALID;
  int h0, v0, bw[3], bh[3];
  int64_t count;
  if (!geometry(width, height, sampling, &h0, &v0, bw, bh, &count)) return VNF_E_INVALID;  // VNF_JPEG_GRAY too: frames are RGB
  memset(out, 0, sizeof(*out));
  if (vnf_jpeg_quant_tables(quality, out->quant[0], out->quant[1]) != VNF_OK) return VNF_E_INVALID;
  memcpy(out->quant[2], out->quant[1], 64);
  out->width = width;
  out->height = height;
  out->components = 3;
  out->sampling = sampling;
  for (int c = 0; c < 3; ++c) {
    out->h[c] = c ? 1 : h0;
    out->v[c] = c ? 1 : v0;
    out->blocks_w[c] = bw[c];
    out->blocks_h[c] = bh[c];
  }
  out->restart_interval = 0;
  out->coef_count = count;
  return VNF_OK;
}

namespace {

// what the Huffman pass accepts: three components, no restart interval, the geometry vnf_jpeg_encode_info gives for
// this size and sampling, one table for both chroma components, no zero quantiser
bool valid_info(const vnf_jpeg_info* info, int bw[3], int bh[3]) {
  int h0, v0;
  int64_t count;
  if (info->components != 3 || info->restart_interval != 0 ||
      !geometry(info->width, info->height, info->sampling, &h0, &v0, bw, bh, &count) || count != info->coef_count)
    return false;
  for (int c = 0; c < 3; ++c)
    if (info->blocks_w[c] != bw[c] || info->blocks_h[c] != bh[c] || info->h[c] != (c ? 1 : h0) || info->v[c] != (c ? 1 : v0))
      return false;
  // two tables are written: luma's and the one both chroma components share
  if (memcmp(info->quant[1], info->quant[2], 64) != 0) return false;
  for (int i = 0; i < 64; ++i)
    if (!info->quant[0][i] || !info->quant[1][i]) return false;
  return true;
}

// SOI .. the end of the SOS header
void write_header(Sink& s, const vnf_jpeg_info* info) {
  s.be16(0xFFD8);
  static const uint8_t app0[16] = {0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};  // JFIF 1.01, aspect 1:1
  s.be16(0xFFE0);
  s.bytes(app0, 16);
  for (int t = 0; t < 2; ++t) {
    s.be16(0xFFDB);
    s.be16(67);
    s.byte(t);
    for (int k = 0; k < 64; ++k) s.byte(info->quant[t][kZigzag[k]]);
  }
  s.be16(0xFFC0);
  s.be16(17);
  s.byte(8);
  s.be16(info->height);
  s.be16(info->width);
  s.byte(3);
  for (int c = 0; c < 3; ++c) {
    s.byte(c + 1);
    s.byte((info->h[c] << 4) | info->v[c]);
    s.byte(c ? 1 : 0);
  }
  for (int t = 0; t < 2; ++t) {  // DC 0, AC 0, DC 1, AC 1, each in a segment of its own
    s.be16(0xFFC4);
    s.be16(2 + 1 + 16 + 12);
    s.byte(t);
    s.bytes(kDcBits[t], 16);
    s.bytes(kDcVals, 12);
    s.be16(0xFFC4);
    s.be16(2 + 1 + 16 + 162);
    s.byte(0x10 | t);
    s.bytes(kAcBits[t], 16);
    s.bytes(kAcVals[t], 162);
  }
  s.be16(0xFFDA);
  s.be16(12);
  s.byte(3);
  for (int c = 0; c < 3; ++c) {
    s.byte(c + 1);
    s.byte(c ? 0x11 : 0x00);
  }
  s.byte(0);
  s.byte(63);
  s.byte(0);
}

}  // namespace

extern "C" int vnf_jpeg_huff_header(const vnf_jpeg_info* info, uint8_t* out, int64_t capacity, int64_t* len_out) {
  if (!info || !len_out || capacity < 0 || (!out && capacity > 0)) return VNF_E_INVALID;
  int bw[3], bh[3];
  if (!valid_info(info, bw, bh)) return VNF_E_INVALID;
  Sink s{out, capacity};
  write_header(s, info);
  *len_out = s.pos;
  return s.pos > capacity ? VNF_E_CAPACITY : VNF_OK;
}

extern "C" int vnf_jpeg_entropy_encode(const int16_t* coefs, const vnf_jpeg_info* info, uint8_t* out, int64_t capacity,
                                       int64_t* len_out) {
  if (!coefs || !info || !len_out || capacity < 0 || (!out && capacity > 0)) return VNF_E_INVALID;
  int bw[3], bh[3];
  if (!valid_info(info, bw, bh)) return VNF_E_INVALID;

  Sink s{out, capacity};
  write_header(s, info);
  auto put = [&s](uint32_t v, int k) { s.bits(v, k); };

  int64_t plane[3] = {0, 0, 0};
  for (int c = 1; c < 3; ++c) plane[c] = plane[c - 1] + (int64_t)64 * bw[c - 1] * bh[c - 1];
  const int mx = bw[1], my = bh[1];
  int pred[3] = {0, 0, 0};
  for (int y = 0; y < my; ++y) {
    for (int x = 0; x < mx; ++x) {
      for (int c = 0; c < 3; ++c) {
        const Codes& hd = kTables.dc[c ? 1 : 0];
        const Codes& ha = kTables.ac[c ? 1 : 0];
        for (int by = 0; by < info->v[c]; ++by) {
          for (int bx = 0; bx < info->h[c]; ++bx) {
            const int16_t* blk = coefs + plane[c] + ((int64_t)(y * info->v[c] + by) * bw[c] + (x * info->h[c] + bx)) * 64;
            if (!encode_block(blk, pred[c], hd, ha, put)) return VNF_E_INVALID;
            pred[c] = blk[0];
          }
        }
      }
    }
  }
  s.flush();
  s.be16(0xFFD9);
  *len_out = s.pos;  // on VNF_E_CAPACITY: the size that would have been enough
  return s.pos > capacity ? VNF_E_CAPACITY : VNF_OK;
}
