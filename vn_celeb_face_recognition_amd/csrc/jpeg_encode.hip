// Device half of the JPEG frame encoder: (n,H,W,3) u8 RGB in HBM -> quantised coefficients, in exactly the layout
// vnf_jpeg_entropy_decode writes (and jpeg_decode.hip reads), ready for the host Huffman pass of jpeg_huff_encode.cpp.
//
// Replaces, together with that pass, the reference's cv2.VideoWriter.write (/root/reference/demo_video.py:25-43) for
// Motion-JPEG output: jpeg_decode.hip run backwards.  The arithmetic is libjpeg's public baseline encoder, all integer,
// so the coefficients are the ones libjpeg and libjpeg-turbo (and with them Pillow) produce:
//   * RGB -> YCbCr with 16-bit fixed-point constants;
//   * chroma down-sampling by 2x1 / 2x2 box sums with the alternating rounding bias (0,1,.. / 1,2,..);
//   * edge replication: columns of the full-resolution rows out to the MCU-padded width BEFORE down-sampling; rows of
//     the source only to whole chroma samples, the DOWN-SAMPLED last row from there on;
//   * the "islow" 8x8 forward DCT (Loeffler-Ligtenberg-Moshytz, 13-bit constants, 2 extra bits kept between the
//     passes) on samples - 128: rows first, then columns; results are 8 x the true DCT;
//   * quantisation sign(x) * ((|x| + 4 q) / (8 q)) by integer division;
//   * the dummy blocks that pad the luma plane to whole MCUs: zero but for a DC copied from the QUANTISED DC of the
//     block to the left (right edge) or of the last block of the row above in the same MCU (bottom edge).
//
// Two launches, mirroring the decoder: the down-sampling sums cross the 4-pixel runs a lane can own with dword stores,
// and an 8x8 block of chroma covers 16x16 pixels, so a fused kernel would have one lane convert 768 bytes of RGB; the
// planes in between cost 1.5 bytes per pixel each way at 4:2:0 (DESIGN.md section 8 has the sums).
//   1. jpeg_enc_colour_kernel: a lane owns 4 neighbouring pixels of VF rows (VF the vertical luma factor): three dword
//      loads per row when the row allows it, one dword of luma per row, its chroma samples (4, 2 or 2 bytes per plane).
//   2. jpeg_fdct_kernel: a lane owns an 8x8 block -- eight 8-byte loads, both passes in registers, 64 divisions, eight
//      16-byte stores; neighbouring lanes own neighbouring blocks, so a wave writes 8 KB of consecutive coefficients.
//      A dummy block recomputes its source block's DC (exactly the sum of its 64 samples - 128) and quantises it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "jpeg_geom.h"

namespace vnf {

// pixels x0..x0+3 of source row `row` (already clamped into the frame), columns clamped to W-1
__device__ __forceinline__ void jpeg_enc_load4(const uint8_t* __restrict__ frame, int W, int row, int x0, int vec,
                                               int* r, int* g, int* b) {
  const uint8_t* p = frame + ((size_t)row * W + x0) * 3;
  if (vec && x0 + 4 <= W) {
    const unsigned* p4 = reinterpret_cast<const unsigned*>(p);
    const unsigned w0 = p4[0], w1 = p4[1], w2 = p4[2];
    r[0] = w0 & 255; g[0] = (w0 >> 8) & 255; b[0] = (w0 >> 16) & 255;
    r[1] = w0 >> 24; g[1] = w1 & 255; b[1] = (w1 >> 8) & 255;
    r[2] = (w1 >> 16) & 255; g[2] = w1 >> 24; b[2] = w2 & 255;
    r[3] = (w2 >> 8) & 255; g[3] = (w2 >> 16) & 255; b[3] = w2 >> 24;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = min(x0 + i, W - 1);
      const uint8_t* q = frame + ((size_t)row * W + x) * 3;
      r[i] = q[0]; g[i] = q[1]; b[i] = q[2];
    }
  }
}

__device__ __forceinline__ int jpeg_enc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int jpeg_enc_cb(int r, int g, int b) {
  return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int jpeg_enc_cr(int r, int g, int b) {
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// HF, VF: luma sampling factors.  A lane owns columns x0..x0+3 (x0 % 4 == 0) of plane rows yr*VF .. yr*VF+VF-1 of
// the MCU-padded luma plane and the chroma samples under them.
template <int HF, int VF>
__global__ void __launch_bounds__(256) jpeg_enc_colour_kernel(const uint8_t* __restrict__ frames, int n, int W, int H,
                                                              JpegGeom g, uint8_t* __restrict__ planes, int vec) {
  const int quads = g.bw[0] * 2;            // 4-pixel runs of a padded luma row
  const int rows = g.bh[0] * 8 / VF;        // row groups of a padded luma plane
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * rows * quads) return;
  const long long rg = t / quads;
  const int xq = (int)(t - rg * quads);
  const int f = (int)(rg / rows), yr = (int)(rg - (long long)f * rows);
  const int x0 = xq * 4;
  const uint8_t* frame = frames + (size_t)f * H * W * 3;
  uint8_t* fp = planes + (size_t)f * g.plane_frame;
  const size_t lpitch = (size_t)g.bw[0] * 8, cpitch = (size_t)g.bw[1] * 8;
  int r[VF][4], gg[VF][4], b[VF][4];
#pragma unroll
  for (int v = 0; v < VF; ++v) {
    const int y = yr * VF + v;
    jpeg_enc_load4(frame, W, min(y, H - 1), x0, vec, r[v], gg[v], b[v]);
    unsigned yw = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) yw |= (unsigned)jpeg_enc_y(r[v][i], gg[v][i], b[v][i]) << (8 * i);
    *reinterpret_cast<unsigned*>(fp + g.plane_off[0] + (size_t)y * lpitch + x0) = yw;
  }
  if (VF == 2) {
    // chroma row yr: source rows 2 cy, 2 cy + 1 with cy = min(yr, ch - 1) -- below the last real chroma row it is
    // that DOWN-SAMPLED row again, not the sum of two copies of the last source row
    const int cy = min(yr, g.chh - 1);
    if (cy != yr) {
      jpeg_enc_load4(frame, W, min(2 * cy, H - 1), x0, vec, r[0], gg[0], b[0]);
      jpeg_enc_load4(frame, W, min(2 * cy + 1, H - 1), x0, vec, r[1], gg[1], b[1]);
    }
  }
  if (HF == 1) {
    unsigned cbw = 0, crw = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      cbw |= (unsigned)jpeg_enc_cb(r[0][i], gg[0][i], b[0][i]) << (8 * i);
      crw |= (unsigned)jpeg_enc_cr(r[0][i], gg[0][i], b[0][i]) << (8 * i);
    }
    *reinterpret_cast<unsigned*>(fp + g.plane_off[1] + (size_t)yr * cpitch + x0) = cbw;
    *reinterpret_cast<unsigned*>(fp + g.plane_off[2] + (size_t)yr * cpitch + x0) = crw;
  } else {
    unsigned cbw = 0, crw = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {           // chroma columns x0/2 + j: the first is even
      int sb = 0, sr = 0;
#pragma unroll
      for (int v = 0; v < VF; ++v) {
#pragma unroll
        for (int i = 2 * j; i < 2 * j + 2; ++i) {
          sb += jpeg_enc_cb(r[v][i], gg[v][i], b[v][i]);
          sr += jpeg_enc_cr(r[v][i], gg[v][i], b[v][i]);
        }
      }
      const int bias = VF == 2 ? 1 + j : j, sh = VF == 2 ? 2 : 1;
      cbw |= (unsigned)((sb + bias) >> sh) << (8 * j);
      crw |= (unsigned)((sr + bias) >> sh) << (8 * j);
    }
    *reinterpret_cast<uint16_t*>(fp + g.plane_off[1] + (size_t)yr * cpitch + (x0 >> 1)) = (uint16_t)cbw;
    *reinterpret_cast<uint16_t*>(fp + g.plane_off[2] + (size_t)yr * cpitch + (x0 >> 1)) = (uint16_t)crw;
  }
}

__device__ __forceinline__ int jpeg_enc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one dimension of the islow forward DCT, in place.  FIRST: the row pass (outputs 0 and 4 scaled up by 2 bits, the
// others descaled by 11); else the column pass (descaled by 2 and by 15).
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int* d) {
  int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7];
  int tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5];
  int tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int SH = FIRST ? 11 : 15;
  d[0] = FIRST ? (tmp10 + tmp11) * 4 : jpeg_enc_descale(tmp10 + tmp11, 2);
  d[4] = FIRST ? (tmp10 - tmp11) * 4 : jpeg_enc_descale(tmp10 - tmp11, 2);
  int z1 = (tmp12 + tmp13) * 4433;
  d[2] = jpeg_enc_descale(z1 + tmp13 * 6270, SH);
  d[6] = jpeg_enc_descale(z1 + tmp12 * (-15137), SH);
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6;
  int z3 = tmp4 + tmp6;
  int z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  tmp4 *= 2446;
  tmp5 *= 16819;
  tmp6 *= 25172;
  tmp7 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 *= -16069;
  z4 *= -3196;
  z3 += z5;
  z4 += z5;
  d[7] = jpeg_enc_descale(tmp4 + z1 + z3, SH);
  d[5] = jpeg_enc_descale(tmp5 + z2 + z4, SH);
  d[3] = jpeg_enc_descale(tmp6 + z2 + z3, SH);
  d[1] = jpeg_enc_descale(tmp7 + z1 + z4, SH);
}

// sign(x) * ((|x| + q8 / 2) / q8), q8 = 8 * quant >= 8
__device__ __forceinline__ int jpeg_enc_quant(int x, int q8) {
  const unsigned a = (unsigned)abs(x);
  const int m = (int)((a + ((unsigned)q8 >> 1)) / (unsigned)q8);
  return x < 0 ? -m : m;
}

// wb, hb: the REAL luma blocks per row / column, ceil(W / 8) and ceil(H / 8); hf: the horizontal luma factor
__global__ void __launch_bounds__(256) jpeg_fdct_kernel(const uint8_t* __restrict__ planes,
                                                        const uint8_t* __restrict__ quant, int n, JpegGeom g, int wb,
                                                        int hb, int hf, int16_t* __restrict__ coefs) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * g.blocks) return;
  const int f = (int)(t / g.blocks);
  long long b = t - (long long)f * g.blocks;
  int c = 0;
  const long long n0 = (long long)g.bw[0] * g.bh[0], n1 = (long long)g.bw[1] * g.bh[1];
  if (b >= n0 + n1) { c = 2; b -= n0 + n1; }
  else if (b >= n0) { c = 1; b -= n0; }
  const int by = (int)(b / g.bw[c]), bx = (int)(b - (long long)by * g.bw[c]);
  const uint8_t* q = quant + (c ? 64 : 0);
  const size_t pitch = (size_t)g.bw[c] * 8;
  const uint8_t* plane = planes + (size_t)f * g.plane_frame + g.plane_off[c];
  int4* dst = reinterpret_cast<int4*>(coefs + (size_t)t * 64);
  if (c == 0 && (bx >= wb || by >= hb)) {
    // dummy block: the quantised DC of its source block, whose unquantised DC is the sum of its samples - 128
    const int sy = min(by, hb - 1);
    const int sx = by >= hb ? min((bx / hf) * hf + hf - 1, wb - 1) : wb - 1;
    const uint8_t* src = plane + ((size_t)sy * 8 * pitch + (size_t)sx * 8);
    int s = -128 * 64;
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      const uint2 w = *reinterpret_cast<const uint2*>(src + y * pitch);
#pragma unroll
      for (int i = 0; i < 4; ++i) s += (int)((w.x >> (8 * i)) & 255) + (int)((w.y >> (8 * i)) & 255);
    }
    const int dc = jpeg_enc_quant(s, 8 * (int)q[0]);
    dst[0] = make_int4(dc & 0xffff, 0, 0, 0);
#pragma unroll
    for (int y = 1; y < 8; ++y) dst[y] = make_int4(0, 0, 0, 0);
    return;
  }
  const uint8_t* src = plane + ((size_t)by * 8 * pitch + (size_t)bx * 8);
  int v[64];
  // pass 1: rows
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const uint2 w = *reinterpret_cast<const uint2*>(src + y * pitch);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[y * 8 + i] = (int)((w.x >> (8 * i)) & 255) - 128;
      v[y * 8 + 4 + i] = (int)((w.y >> (8 * i)) & 255) - 128;
    }
    jpeg_fdct8<true>(v + y * 8);
  }
  // pass 2: columns
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    int col[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) col[y] = v[y * 8 + x];
    jpeg_fdct8<false>(col);
#pragma unroll
    for (int y = 0; y < 8; ++y) v[y * 8 + x] = col[y];
  }
  const uint2* q2 = reinterpret_cast<const uint2*>(q);
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const uint2 qq = q2[y];
    int o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int qv = (int)(((i < 4 ? qq.x : qq.y) >> (8 * (i & 3))) & 255);
      o[i] = jpeg_enc_quant(v[y * 8 + i], 8 * max(qv, 1)) & 0xffff;   // a zero entry is no valid table: never divide by it
    }
    dst[y] = make_int4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
  }
}

}  // namespace vnf

using namespace vnf;

extern "C" int64_t vnf_jpeg_encode_workspace_bytes(int n, int width, int height, int sampling) {
  JpegGeom g;
  if (n < 0 || width < 1 || width > 65535 || height < 1 || height > 65535 || sampling == VNF_JPEG_GRAY ||
      !jpeg_geom(width, height, sampling, &g))
    return fail(VNF_E_INVALID, "vnf_jpeg_encode_workspace_bytes: bad argument");
  return (int64_t)n * g.plane_frame;
}

extern "C" int vnf_jpeg_encode_frames(const uint8_t* frames_dev, int n, int width, int height, int sampling,
                                      const uint8_t* quant_dev, int16_t* coefs_out, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  if (n == 0) return VNF_OK;
  JpegGeom g;
  if (n < 0 || width < 1 || width > 65535 || height < 1 || height > 65535 || !frames_dev || !quant_dev || !coefs_out ||
      !workspace)
    return fail(VNF_E_INVALID, "vnf_jpeg_encode_frames: bad argument");
  if (sampling == VNF_JPEG_GRAY || !jpeg_geom(width, height, sampling, &g))
    return fail(VNF_E_INVALID, "vnf_jpeg_encode_frames: sampling must be VNF_JPEG_444, _422 or _420 (frames are RGB)");
  // 16-byte stores of the coefficients (a frame is a multiple of 64 of them), 8-byte loads of the tables and of the
  // plane rows
  if (((uintptr_t)coefs_out & 15) || ((uintptr_t)quant_dev & 7) || ((uintptr_t)workspace & 15))
    return fail(VNF_E_INVALID, "vnf_jpeg_encode_frames: coefs_out and workspace must be 16-byte, quant_dev 8-byte aligned");
  if (workspace_bytes < (int64_t)n * g.plane_frame)
    return fail(VNF_E_CAPACITY, "vnf_jpeg_encode_frames: workspace_bytes is below vnf_jpeg_encode_workspace_bytes");
  const int hf = sampling == VNF_JPEG_444 ? 1 : 2, vf = sampling == VNF_JPEG_420 ? 2 : 1;
  const long long t1 = ((long long)n * (g.bh[0] * 8 / vf) * (g.bw[0] * 2) + 255) / 256;
  const long long t2 = ((long long)n * g.blocks + 255) / 256;
  if (t1 > 0x7fffffffLL || t2 > 0x7fffffffLL) return fail(VNF_E_CAPACITY, "vnf_jpeg_encode_frames: batch too large for one grid");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* planes = (uint8_t*)workspace;
  // three dwords per lane when every quad of every row starts on a dword: (row * W + x0) * 3 with x0 % 4 == 0
  const int vec = (width % 4 == 0 && ((uintptr_t)frames_dev & 3) == 0) ? 1 : 0;
  const dim3 grid((unsigned)t1), block(256);
  switch (sampling) {
    case VNF_JPEG_444:
      hipLaunchKernelGGL((jpeg_enc_colour_kernel<1, 1>), grid, block, 0, st, frames_dev, n, width, height, g, planes, vec);
      break;
    case VNF_JPEG_422:
      hipLaunchKernelGGL((jpeg_enc_colour_kernel<2, 1>), grid, block, 0, st, frames_dev, n, width, height, g, planes, vec);
      break;
    default:
      hipLaunchKernelGGL((jpeg_enc_colour_kernel<2, 2>), grid, block, 0, st, frames_dev, n, width, height, g, planes, vec);
      break;
  }
  VNF_HIP(hipGetLastError());
  hipLaunchKernelGGL(jpeg_fdct_kernel, dim3((unsigned)t2), dim3(256), 0, st, planes, quant_dev, n, g, (width + 7) / 8,
                     (height + 7) / 8, hf, coefs_out);
  VNF_HIP(hipGetLastError());
  return VNF_OK;
}
