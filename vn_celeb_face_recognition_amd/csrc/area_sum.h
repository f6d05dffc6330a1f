// interpolate(mode="area") on 8-bit RGB frames (adaptive average pooling), the one statement of it for the pyramid, crop
// and extract kernels: which input rows / columns an output bin covers, and the integer sum of a bin's bytes per channel,
// gathered pixel by pixel or built from packed column sums of 16-byte pieces of the rows.
//
// Everything here returns integers; the caller finishes.  The sums are exact whatever order they are added in, so every
// kernel over this header gives the same bits for the same bin, and a sum below 2^24 (bins under 256 x 256 pixels)
// converts to fp32 exactly.  The cascade's finish is area_norm; face extraction has its own (extract.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace vnf {

// Output index o of `out` covers input [lo, hi) = [floor(o * in / out), ceil((o + 1) * in / out)) of `in`.
// With in = q * out + r the products stay in 32 bits: exact for every in < 2^31 with o < out <= 65535.
struct AreaBin { int lo, hi; };
__host__ __device__ __forceinline__ AreaBin area_bin(int o, int in, int out) {
  const unsigned uo = (unsigned)o, n = (unsigned)out, q = (unsigned)in / n, r = (unsigned)in - q * n;
  return AreaBin{(int)(uo * q + (uo * r) / n), (int)((uo + 1) * q + ((uo + 1) * r + n - 1) / n)};
}

// 16 bytes of a row: one dwordx4 load either way; ALIGNED promises a 16-byte boundary
template <bool ALIGNED>
__device__ __forceinline__ uint4 area_load16(const uint8_t* p) {
  if constexpr (ALIGNED) return *reinterpret_cast<const uint4*>(p);
  uint4 v;
  memcpy(&v, p, 16);
  return v;
}

// Packed per-byte sums of one 16-byte column over rows [h0, h1) of `pitch` bytes, p0 = the column in row 0.  Bytes 0,2
// and 1,3 of each dword add up in the two 16-bit halves of one register (5 VALU ops per dword instead of 11), so
// h1 - h0 <= 257 (257 x 255 = 65535).  A round is four independent loads: the row is clamped and its bytes masked
// instead of a branch, so the loads are not serialised behind their predicates.  ROUNDS of them are unrolled into one
// trip, 4 x ROUNDS loads in flight: the caller's choice, stated here so that it does not hang on an inlining heuristic.
template <bool ALIGNED, int ROUNDS>
__device__ __forceinline__ void area_colsum16(const uint8_t* p0, size_t pitch, int h0, int h1, unsigned (&pe)[4], unsigned (&po)[4]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) { pe[d] = 0u; po[d] = 0u; }
#pragma unroll ROUNDS
  for (int yy = h0; yy < h1; yy += 4) {
    uint4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = area_load16<ALIGNED>(p0 + (size_t)min(yy + j, h1 - 1) * pitch);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned msk = (yy + j < h1) ? 0x00FF00FFu : 0u;
      const unsigned wv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        pe[d] += wv[d] & msk;
        po[d] += (wv[d] >> 8) & msk;
      }
    }
  }
}

// the 16 per-byte sums of a packed pair, in byte order
__device__ __forceinline__ void area_unpack(const unsigned (&pe)[4], const unsigned (&po)[4], unsigned (&sum)[16]) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    sum[d * 4 + 0] = pe[d] & 0xFFFFu;
    sum[d * 4 + 1] = po[d] & 0xFFFFu;
    sum[d * 4 + 2] = pe[d] >> 16;
    sum[d * 4 + 3] = po[d] >> 16;
  }
}

// s[c] += channel c of n RGB pixels at px: bytes of a frame row, or the per-byte column sums of a bin row
template <typename T>
__device__ __forceinline__ void area_span(const T* px, int n, unsigned (&s)[3]) {
  for (int xx = 0; xx < 3 * n; xx += 3) { s[0] += px[xx]; s[1] += px[xx + 1]; s[2] += px[xx + 2]; }
}

// the bin rows [h0, h1) x columns [w0, w1), pixel by pixel; base = pixel (0, 0) of what the bins count from
__device__ __forceinline__ void area_gather(const uint8_t* base, size_t pitch, int h0, int h1, int w0, int w1, unsigned (&s)[3]) {
  s[0] = s[1] = s[2] = 0u;
  for (int yy = h0; yy < h1; ++yy) area_span(base + (size_t)yy * pitch + (size_t)w0 * 3, w1 - w0, s);
}

// detect_face.py:71-72, 113, 142: imresample then (x - 127.5) * 0.0078125; the mean as sum / kh / kw, two divisions,
// as ATen rounds it
__device__ __forceinline__ float area_norm(unsigned sum, int kh, int kw) {
  return (((float)sum / (float)kh) / (float)kw - 127.5f) * 0.0078125f;
}

}  // namespace vnf
