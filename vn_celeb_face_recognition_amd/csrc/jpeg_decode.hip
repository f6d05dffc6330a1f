// Device half of the JPEG frame decoder: quantised coefficients (jpeg_entropy.cpp) -> (n,H,W,3) u8 RGB in HBM.
//
// Replaces, together with the host entropy decoder, cv2.VideoCapture.read of /root/reference/demo_video.py:78-110 for
// Motion-JPEG input.  The arithmetic is libjpeg's public baseline path, all integer, so the bytes are the ones libjpeg
// and libjpeg-turbo (and with them Pillow) produce:
//   * dequantisation coef * quant in int32 and the "islow" 8x8 inverse DCT (Loeffler-Ligtenberg-Moshytz, 13-bit
//     constants, 2 extra bits kept between the passes): columns first, descaled by 11 bits, then rows, descaled by 18,
//     each with rounding; + 128 and the 10-bit range-limit mask;
//   * "fancy" (triangle) chroma upsampling over the plane of ceil(W h / hmax) x ceil(H v / vmax) real samples, edges
//     replicated, MCU padding never read;
//   * YCbCr -> RGB with 16-bit fixed-point constants.
//
// Two launches.  The work is memory-bound byte shuffling and the second kernel's chroma taps cross 8x8 block borders
// (a 16x16 output tile of a 4:2:0 frame needs a one-sample ring of chroma from up to 8 neighbour blocks), so a fused
// kernel would run those neighbours' IDCTs again or exchange them between workgroups; the planes that two launches
// put in between cost 1.5 bytes per pixel each way (DESIGN.md section 8 has the sums).
//   1. jpeg_idct_kernel: a lane owns an 8x8 block -- eight 16-byte loads, both passes in registers (no exchange
//      between lanes: a lane that held one block ROW would have to transpose across 8 neighbours before the column
//      pass), eight 8-byte stores; neighbouring lanes own neighbouring blocks, so a wave's stores are 512-byte runs of
//      a plane row.
//   2. jpeg_colour_kernel: a lane owns 4 neighbouring pixels of a row: one 4-byte luma load, the chroma taps of its
//      two chroma columns, twelve output bytes as three dwords when the row allows it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine.h"
#include "jpeg_geom.h"

namespace vnf {

__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one dimension of the islow IDCT: in[0..7] -> out[0..7], descaled by `shift` bits with rounding
__device__ __forceinline__ void jpeg_idct8(const int* in, int* out, int shift) {
  int z2 = in[2], z3 = in[6];
  int z1 = (z2 + z3) * 4433;
  int tmp2 = z1 + z3 * (-15137);
  int tmp3 = z1 + z2 * 6270;
  z2 = in[0];
  z3 = in[4];
  int tmp0 = (z2 + z3) * 8192;
  int tmp1 = (z2 - z3) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446;
  tmp1 *= 16819;
  tmp2 *= 25172;
  tmp3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 *= -16069;
  z4 *= -3196;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0] = jpeg_descale(tmp10 + tmp3, shift);
  out[7] = jpeg_descale(tmp10 - tmp3, shift);
  out[1] = jpeg_descale(tmp11 + tmp2, shift);
  out[6] = jpeg_descale(tmp11 - tmp2, shift);
  out[2] = jpeg_descale(tmp12 + tmp1, shift);
  out[5] = jpeg_descale(tmp12 - tmp1, shift);
  out[3] = jpeg_descale(tmp13 + tmp0, shift);
  out[4] = jpeg_descale(tmp13 - tmp0, shift);
}

// libjpeg's range_limit[(x) & 1023] behind the + 128: the clamp on [-512, 511], and the same wrap outside it
__device__ __forceinline__ unsigned jpeg_range(int x) {
  int m = x & 1023;
  m = m >= 512 ? m - 1024 : m;
  return (unsigned)min(255, max(0, m + 128));
}

__global__ void __launch_bounds__(256) jpeg_idct_kernel(const int16_t* __restrict__ coefs,
                                                        const uint8_t* __restrict__ quant, int n, JpegGeom g,
                                                        uint8_t* __restrict__ planes) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * g.blocks) return;
  const int f = (int)(t / g.blocks);
  long long b = t - (long long)f * g.blocks;
  int c = 0;
  if (g.ncomp == 3) {
    const long long n0 = (long long)g.bw[0] * g.bh[0], n1 = (long long)g.bw[1] * g.bh[1];
    if (b >= n0 + n1) { c = 2; b -= n0 + n1; }
    else if (b >= n0) { c = 1; b -= n0; }
  }
  const int by = (int)(b / g.bw[c]), bx = (int)(b - (long long)by * g.bw[c]);
  // every block of every plane of every frame is 64 int16 of one dense array
  const int4* src = reinterpret_cast<const int4*>(coefs + (size_t)t * 64);
  const uint2* q = reinterpret_cast<const uint2*>(quant + ((size_t)f * 3 + c) * 64);
  int v[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int4 w = src[r];
    const uint2 qq = q[r];
    const int ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned qw = j < 2 ? qq.x : qq.y;
      const int qa = (qw >> (16 * (j & 1))) & 255, qb = (qw >> (16 * (j & 1) + 8)) & 255;
      v[r * 8 + 2 * j] = (int)(int16_t)(ww[j] & 0xffff) * qa;
      v[r * 8 + 2 * j + 1] = (ww[j] >> 16) * qb;
    }
  }
  // pass 1: columns
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    int in[8], out[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) in[y] = v[y * 8 + x];
    jpeg_idct8(in, out, 11);
#pragma unroll
    for (int y = 0; y < 8; ++y) v[y * 8 + x] = out[y];
  }
  // pass 2: rows, then the sample bytes of the row
  uint8_t* dst = planes + (size_t)f * g.plane_frame + g.plane_off[c] + ((size_t)by * 8 * g.bw[c] + bx) * 8;
  const size_t pitch = (size_t)g.bw[c] * 8;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    int out[8];
    jpeg_idct8(v + y * 8, out, 18);
    uint2 o;
    o.x = jpeg_range(out[0]) | (jpeg_range(out[1]) << 8) | (jpeg_range(out[2]) << 16) | (jpeg_range(out[3]) << 24);
    o.y = jpeg_range(out[4]) | (jpeg_range(out[5]) << 8) | (jpeg_range(out[6]) << 16) | (jpeg_range(out[7]) << 24);
    *reinterpret_cast<uint2*>(dst + y * pitch) = o;
  }
}

__device__ __forceinline__ unsigned jpeg_clamp8(int x) { return (unsigned)min(255, max(0, x)); }

// SAMPLING: VNF_JPEG_*.  A lane owns pixels x0 .. x0+3 (x0 % 4 == 0) of one output row.
template <int SAMPLING>
__global__ void __launch_bounds__(256) jpeg_colour_kernel(const uint8_t* __restrict__ planes, int n, int W, int H,
                                                          JpegGeom g, uint8_t* __restrict__ out, int vec) {
  const int quads = (W + 3) >> 2;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * H * quads) return;
  const long long row = t / quads;
  const int xq = (int)(t - row * quads);
  const int f = (int)(row / H), y = (int)(row - (long long)f * H);
  const int x0 = xq * 4;
  const uint8_t* fp = planes + (size_t)f * g.plane_frame;
  // luma: the plane's pitch is a multiple of 8, so the four bytes are there (padding past W) and aligned
  const unsigned yw = *reinterpret_cast<const unsigned*>(fp + g.plane_off[0] + (size_t)y * g.bw[0] * 8 + x0);
  int cb[4], cr[4];
  if (SAMPLING == VNF_JPEG_GRAY) {
#pragma unroll
    for (int i = 0; i < 4; ++i) cb[i] = cr[i] = 128;
  } else {
#pragma unroll
    for (int k = 1; k <= 2; ++k) {
      int* dstc = k == 1 ? cb : cr;
      const uint8_t* cp = fp + g.plane_off[k];
      const size_t pitch = (size_t)g.bw[k] * 8;
      if (SAMPLING == VNF_JPEG_444) {
        const unsigned w = *reinterpret_cast<const unsigned*>(cp + (size_t)y * pitch + x0);
#pragma unroll
        for (int i = 0; i < 4; ++i) dstc[i] = (w >> (8 * i)) & 255;
      } else {
        // chroma columns i0, i0+1 and their neighbours, clamped to the real samples (edge replication)
        const int i0 = x0 >> 1;
        int col[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) col[j] = min(max(i0 - 1 + j, 0), g.cw - 1);
        int s[4];
        if (SAMPLING == VNF_JPEG_422) {
          const uint8_t* r0 = cp + (size_t)y * pitch;
#pragma unroll
          for (int j = 0; j < 4; ++j) s[j] = r0[col[j]];
          dstc[0] = (3 * s[1] + s[0] + 1) >> 2;
          dstc[1] = (3 * s[1] + s[2] + 2) >> 2;
          dstc[2] = (3 * s[2] + s[1] + 1) >> 2;
          dstc[3] = (3 * s[2] + s[3] + 2) >> 2;
        } else {
          const int cy = y >> 1;
          const int far = min(max((y & 1) ? cy + 1 : cy - 1, 0), g.chh - 1);
          const uint8_t* rn = cp + (size_t)cy * pitch;
          const uint8_t* rf = cp + (size_t)far * pitch;
#pragma unroll
          for (int j = 0; j < 4; ++j) s[j] = 3 * rn[col[j]] + rf[col[j]];
          dstc[0] = (3 * s[1] + s[0] + 8) >> 4;
          dstc[1] = (3 * s[1] + s[2] + 7) >> 4;
          dstc[2] = (3 * s[2] + s[1] + 8) >> 4;
          dstc[3] = (3 * s[2] + s[3] + 7) >> 4;
        }
      }
    }
  }
  unsigned rgb[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int Y = (yw >> (8 * i)) & 255;
    if (SAMPLING == VNF_JPEG_GRAY) {
      rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = (unsigned)Y;
    } else {
      const int u = cb[i] - 128, w = cr[i] - 128;
      rgb[3 * i] = jpeg_clamp8(Y + ((91881 * w + 32768) >> 16));
      rgb[3 * i + 1] = jpeg_clamp8(Y + ((-22554 * u + 32768 - 46802 * w) >> 16));
      rgb[3 * i + 2] = jpeg_clamp8(Y + ((116130 * u + 32768) >> 16));
    }
  }
  uint8_t* o = out + ((size_t)row * W + x0) * 3;
  if (vec && x0 + 4 <= W) {
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
    for (int d = 0; d < 3; ++d)
      o4[d] = rgb[4 * d] | (rgb[4 * d + 1] << 8) | (rgb[4 * d + 2] << 16) | (rgb[4 * d + 3] << 24);
  } else {
    const int np = min(4, W - x0);
    for (int i = 0; i < np * 3; ++i) o[i] = (uint8_t)rgb[i];
  }
}

}  // namespace vnf

using namespace vnf;

extern "C" int64_t vnf_jpeg_workspace_bytes(int n, int width, int height, int sampling) {
  JpegGeom g;
  if (n < 0 || width < 1 || width > 65535 || height < 1 || height > 65535 || !jpeg_geom(width, height, sampling, &g))
    return fail(VNF_E_INVALID, "vnf_jpeg_workspace_bytes: bad argument");
  return (int64_t)n * g.plane_frame;
}

extern "C" int vnf_jpeg_decode_frames(const int16_t* coefs_dev, const uint8_t* quant_dev, int n, int width, int height,
                                      int sampling, uint8_t* frames_out, void* workspace, int64_t workspace_bytes,
                                      void* stream) {
  if (n == 0) return VNF_OK;
  JpegGeom g;
  if (n < 0 || width < 1 || width > 65535 || height < 1 || height > 65535 || !coefs_dev || !quant_dev || !frames_out ||
      !workspace)
    return fail(VNF_E_INVALID, "vnf_jpeg_decode_frames: bad argument");
  if (!jpeg_geom(width, height, sampling, &g)) return fail(VNF_E_INVALID, "vnf_jpeg_decode_frames: unknown sampling code");
  // 16-byte loads of the coefficients (a frame is a multiple of 64 of them), 8-byte loads of the tables and stores of
  // the plane rows
  if (((uintptr_t)coefs_dev & 15) || ((uintptr_t)quant_dev & 7) || ((uintptr_t)workspace & 15))
    return fail(VNF_E_INVALID, "vnf_jpeg_decode_frames: coefs_dev and workspace must be 16-byte, quant_dev 8-byte aligned");
  if (workspace_bytes < (int64_t)n * g.plane_frame)
    return fail(VNF_E_CAPACITY, "vnf_jpeg_decode_frames: workspace_bytes is below vnf_jpeg_workspace_bytes");
  const long long t1 = ((long long)n * g.blocks + 255) / 256;
  const long long t2 = ((long long)n * height * ((width + 3) / 4) + 255) / 256;
  if (t1 > 0x7fffffffLL || t2 > 0x7fffffffLL) return fail(VNF_E_CAPACITY, "vnf_jpeg_decode_frames: batch too large for one grid");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* planes = (uint8_t*)workspace;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)t1), dim3(256), 0, st, coefs_dev, quant_dev, n, g, planes);
  VNF_HIP(hipGetLastError());
  // three dwords per lane when every quad of every row starts on a dword: (row * W + x0) * 3 with x0 % 4 == 0
  const int vec = (width % 4 == 0 && ((uintptr_t)frames_out & 3) == 0) ? 1 : 0;
  const dim3 grid((unsigned)t2), block(256);
  switch (sampling) {
    case VNF_JPEG_GRAY:
      hipLaunchKernelGGL(jpeg_colour_kernel<VNF_JPEG_GRAY>, grid, block, 0, st, planes, n, width, height, g, frames_out, vec);
      break;
    case VNF_JPEG_444:
      hipLaunchKernelGGL(jpeg_colour_kernel<VNF_JPEG_444>, grid, block, 0, st, planes, n, width, height, g, frames_out, vec);
      break;
    case VNF_JPEG_422:
      hipLaunchKernelGGL(jpeg_colour_kernel<VNF_JPEG_422>, grid, block, 0, st, planes, n, width, height, g, frames_out, vec);
      break;
    default:
      hipLaunchKernelGGL(jpeg_colour_kernel<VNF_JPEG_420>, grid, block, 0, st, planes, n, width, height, g, frames_out, vec);
      break;
  }
  VNF_HIP(hipGetLastError());
  return VNF_OK;
}
