// Face extraction on the device: the integer crop rectangle of a detection, area-resampled to S x S, as
// bytes (n,S,S,3) and / or as the encoder's NCHW input (n,3,S,S), raw or (x - 127.5) / 128.
//
// Reference semantics (file:line under /root/reference):
//   models/mtcnn_utils/detect_face.py:317-322  crop = img[y1:y2, x1:x2]; imresample(crop.float(), (S,S)).byte()
//   models/mtcnn_utils/detect_face.py:304-306  imresample = interpolate(mode="area") = adaptive average pooling: the bin
//                                              of output (oy,ox) is rows [oy*ch//S, ceil((oy+1)*ch/S)), columns alike
//   models/mtcnn_utils/detect_face.py:376      F.to_tensor(np.float32(face)): float(byte), HWC -> CHW
//   models/mtcnn.py:516-518                    fixed_image_standardization: (x - 127.5) / 128
// The rectangle itself (detect_face.py:358-368, float32 margin arithmetic) is host work: detector.crop_rects.
//
// Memory-bound byte work over the bins and sums of area_sum.h, like the cascade's crop_resize_rows_kernel: a wave owns an
// output row; its lanes stream 16-byte pieces of the crop's byte span of every input row of the bin row, keep per-byte
// column sums in registers, park them in a wave-private LDS strip and then add the horizontal bin spans.  The finish is
// this file's own: one IEEE fp32 division of the exact sum (no reciprocal: s * (1 / (kh kw)) truncates constant bins to
// v - 1), so for bins under 2^15 pixels the byte is the reference's whatever order it adds in.  Unlike the cascade's
// kernel the pieces start at the crop's first byte, not at a 16-byte boundary of the frame, so one code path serves every
// x1 and every row pitch (W*3 % 16 != 0 moves the alignment from row to row, which chunk-aligned register sums cannot
// follow).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "area_sum.h"
#include "engine.h"

namespace vnf {

constexpr int EXT_STRIP = 2048;     // bytes of crop row a wave holds column sums for at a time (682 px); wider crops go in x-tiles
constexpr int EXT_MAXS = 1024;      // largest output side
constexpr int EXT_MAXBIN = 1 << 15; // pixels per bin, exclusive: below it every correctly rounded quotient truncates alike

struct ExtRect { int frame, x1, y1, cw, ch; bool ok; };

__device__ __forceinline__ ExtRect ext_rect(const int32_t* __restrict__ rects, int i, int B, int H, int W, int S) {
  const int32_t* r = rects + 5 * (size_t)i;
  ExtRect o;
  o.frame = r[0]; o.x1 = r[1]; o.y1 = r[2];
  const int x2 = r[3], y2 = r[4];
  o.ok = o.frame >= 0 && o.frame < B && o.x1 >= 0 && o.y1 >= 0 && x2 > o.x1 && y2 > o.y1 && x2 <= W && y2 <= H;
  o.cw = o.ok ? x2 - o.x1 : 0;
  o.ch = o.ok ? y2 - o.y1 : 0;
  if (o.ok && (long long)((o.ch + S - 1) / S + 1) * ((o.cw + S - 1) / S + 1) >= EXT_MAXBIN) o.ok = false;
  return o;
}

// dynamic LDS behind the strips: the bin table of the output columns, 2 * S ints, and -- only when the bytes are wanted --
// a staging row of S * 3 bytes per wave; sized by the S of the call, so that four workgroups share a CU at S = 160
__host__ __device__ inline int ext_tab_bytes(int S) { return (8 * S + 15) & ~15; }
__host__ __device__ inline int ext_row_bytes(int S) { return (3 * S + 3) & ~3; }

// grid (n faces, row groups): blockIdx.y splits the S output rows, so one large crop is spread over several workgroups
template <typename TO>
__global__ void __launch_bounds__(256) extract_faces_kernel(const uint8_t* __restrict__ frames, int B, int H, int W,
                                                            const int32_t* __restrict__ rects, int S, int standardize,
                                                            TO* __restrict__ x_out, uint8_t* __restrict__ u8_out) {
  __shared__ __attribute__((aligned(16))) unsigned strips[4][EXT_STRIP];
  extern __shared__ __attribute__((aligned(16))) uint8_t ext_dyn[];
  int* wtab0 = reinterpret_cast<int*>(ext_dyn);  // first and one-past-last input column of every output column's bin
  int* wtab1 = wtab0 + S;
  const int f = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const ExtRect t = ext_rect(rects, f, B, H, W, S);
  const int zrows = (S + (int)gridDim.y - 1) / (int)gridDim.y;
  const int oy_lo = (int)blockIdx.y * zrows, oy_hi = min(S, oy_lo + zrows);
  const size_t pitch = (size_t)W * 3;
  const uint8_t* fend = frames + (size_t)B * H * pitch;
  const uint8_t* base = frames + ((size_t)(t.ok ? t.frame : 0) * H + t.y1) * pitch + (size_t)t.x1 * 3;
  unsigned* cs = strips[wave];
  uint8_t* ob = ext_dyn + ext_tab_bytes(S) + wave * ext_row_bytes(S);  // only there (and only touched) with u8_out
  const int lim_px = (EXT_STRIP - 16) / 3;
  // a single bin wider than a strip (S tiny against the crop): per-pixel sums for this face
  const bool wide = t.ok && (t.cw + S - 1) / S + 1 > lim_px;
  const bool u8_vec = (S & 3) == 0 && ((uintptr_t)u8_out & 3) == 0;
  // the column bins are the same for every row: worked out once per workgroup, not per output value
  if (t.ok)
    for (int ox = threadIdx.x; ox < S; ox += blockDim.x) {
      const AreaBin bw = area_bin(ox, t.cw, S);
      wtab0[ox] = bw.lo;
      wtab1[ox] = bw.hi;
    }
  __syncthreads();

  for (int oy = oy_lo + wave; oy < oy_hi; oy += 4) {
    const AreaBin bh = area_bin(oy, t.ch, S);
    const int h0 = bh.lo, h1 = bh.hi;
    int ox_a = 0;
    while (ox_a < S) {
      int ox_b = S, px0 = 0;
      if (t.ok && !wide) {
        // x-tile [ox_a, ox_b): the most output columns whose input bytes fit the strip (all of them for crops up to 677 px)
        px0 = wtab0[ox_a];
        if (t.cw > lim_px) ox_b = (int)min((long long)S, ((long long)(px0 + lim_px) * S) / t.cw);
        const int px1 = wtab1[ox_b - 1];
        const int nct = ((px1 - px0) * 3 + 15) >> 4;
        const uint8_t* tb = base + (size_t)px0 * 3;
        for (int c = lane; c < nct; c += 64) {
          const uint8_t* p0 = tb + ((size_t)c << 4);
          uint4* dst = reinterpret_cast<uint4*>(cs + (c << 4));
          // the pieces start at the crop's first byte and run past its last one by up to 15 bytes: harmless inside the
          // frames (those sums are never read), but the last rows of the last frame would leave the buffer
          if (p0 + (size_t)(h1 - 1) * pitch + 16 > fend) {
#pragma nounroll
            for (int j = 0; j < 16; ++j) {
              unsigned sum = 0;
#pragma nounroll
              for (int yy = h0; yy < h1; ++yy) {
                const uint8_t* q = p0 + (size_t)yy * pitch + j;
                if (q < fend) sum += *q;
              }
              cs[(c << 4) + j] = sum;
            }
            continue;
          }
          // packed sums of at most 256 rows at a time, one round of four loads per trip, which then go to the lane's own
          // 32-bit sums in the strip (written by the first 256 rows, added to by deeper ones)
          for (int hb = h0; hb < h1; hb += 256) {
            unsigned pe[4], po[4], u[16];
            area_colsum16<false, 1>(p0, pitch, hb, min(h1, hb + 256), pe, po);
            area_unpack(pe, po, u);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              uint4 a = uint4{u[4 * d], u[4 * d + 1], u[4 * d + 2], u[4 * d + 3]};
              if (hb != h0) {
                const uint4 o = dst[d];
                a = uint4{a.x + o.x, a.y + o.y, a.z + o.z, a.w + o.w};
              }
              dst[d] = a;
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      // bins of this tile: a lane takes an output column and its three channels, so the lanes of each store run along x
      for (int ox = ox_a + lane; ox < ox_b; ox += 64) {
        unsigned byte[3] = {0u, 0u, 0u};
        if (t.ok) {
          const int w0 = wtab0[ox], w1 = wtab1[ox];
          unsigned sum[3] = {0u, 0u, 0u};
          if (!wide) area_span(cs + (w0 - px0) * 3, w1 - w0, sum);
          else area_gather(base, pitch, h0, h1, w0, w1, sum);
          // one IEEE division of the exact integer sum, truncated (.byte())
          const float area = (float)((h1 - h0) * (w1 - w0));
#pragma unroll
          for (int c = 0; c < 3; ++c) byte[c] = (unsigned)((float)sum[c] / area);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (u8_out) ob[ox * 3 + c] = (uint8_t)byte[c];
          if (x_out) {
            const float v = (float)byte[c];
            x_out[(((size_t)f * 3 + c) * S + oy) * S + ox] = (TO)((standardize && t.ok) ? (v - 127.5f) / 128.0f : v);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      ox_a = ox_b;
    }
    if (u8_out) {  // the finished row: S*3 contiguous bytes
      uint8_t* o = u8_out + ((size_t)f * S + oy) * (size_t)S * 3;
      if (u8_vec) {
        for (int q = lane; q < (S * 3) >> 2; q += 64) reinterpret_cast<unsigned*>(o)[q] = reinterpret_cast<const unsigned*>(ob)[q];
      } else {
        for (int q = lane; q < S * 3; q += 64) o[q] = ob[q];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace vnf

using namespace vnf;

extern "C" int vnf_extract_faces(const uint8_t* frames, int b, int height, int width, const int32_t* rects, int n, int s,
                                 int standardize, void* x_out, int out_dtype, uint8_t* u8_out, void* stream) {
  if (n == 0) return VNF_OK;
  if (n < 0 || s < 1 || s > EXT_MAXS || !frames || !rects || b < 1 || height < 1 || width < 1 || (!x_out && !u8_out))
    return fail(VNF_E_INVALID, "vnf_extract_faces: bad argument");
  if (x_out && out_dtype != VNF_F32 && out_dtype != VNF_BF16 && out_dtype != VNF_F16)
    return fail(VNF_E_INVALID, "vnf_extract_faces: bad out_dtype");
  hipStream_t st = (hipStream_t)stream;
  // row groups: about 1024 workgroups (four fit a CU: 123 VGPRs, 32 KB of strips), at least one output row per wave
  int z = (1024 + n - 1) / n;
  z = z < 1 ? 1 : z;
  const int zmax = (s + 3) / 4;
  z = z > zmax ? zmax : z;
  const dim3 grid(n, z), block(256);
  const size_t lds = ext_tab_bytes(s) + (u8_out ? 4 * ext_row_bytes(s) : 0);
  switch (x_out ? out_dtype : VNF_F32) {
    case VNF_F32:
      hipLaunchKernelGGL(extract_faces_kernel<float>, grid, block, lds, st, frames, b, height, width, rects, s, standardize,
                         (float*)x_out, u8_out);
      break;
    case VNF_BF16:
      hipLaunchKernelGGL(extract_faces_kernel<__bf16>, grid, block, lds, st, frames, b, height, width, rects, s, standardize,
                         (__bf16*)x_out, u8_out);
      break;
    default:
      hipLaunchKernelGGL(extract_faces_kernel<_Float16>, grid, block, lds, st, frames, b, height, width, rects, s, standardize,
                         (_Float16*)x_out, u8_out);
      break;
  }
  VNF_HIP(hipGetLastError());
  return VNF_OK;
}
