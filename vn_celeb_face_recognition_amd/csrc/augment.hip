// transforms_facenet_aug (data_loader/__init__.py:58-65) for a batch, in one launch: gather a face of the resident u8 data
// set, rotate it as Pillow's Image.rotate(angle, BICUBIC) does, zero-pad and crop (RandomCrop(T, padding=2,
// pad_if_needed=True)) by offset arithmetic, mirror by index (RandomHorizontalFlip), then np.float32, (v - 127.5) / 128
// and CHW (fix_std, to_tensor) in the encoder's input dtype.  The random draws are the host's (vnf_aug_param); nothing
// here is random.
//
// The rotation is libImaging/Geometry.c's ImagingGenericTransform with affine_transform and bicubic_filter32RGB, restated
// operation by operation in double so the bytes are Pillow's (the file is built with -ffp-contract=off: a contracted
// multiply-add rounds once where Pillow rounds twice):
//   xin = m0 (x + .5) + m1 (y + .5) + m2, yin likewise; outside [0,S) the pixel is the fill (0);
//   xin -= .5, yin -= .5; x0 = floor, d = frac; columns x0-1..x0+2 clamped to the image; row y0-1 clamped, and each of
//   the next three rows that lies outside the image REPEATS the value of the row before it;
//   the cubic is the a = -1 form p1 + d (p2 + d (p3 + d p4)), rows first, then the column of the four row values;
//   v <= 0 -> 0, v >= 255 -> 255, else (uint8)v: truncation.
//
// One thread = AUG_PX consecutive output pixels of one row (3 channels each), so a wave writes whole stretches of an
// NCHW row per channel with 16-byte (f32) / 8-byte (16-bit) stores.  Reads are the 16 taps per pixel of a 77 KB face,
// served by L2; the bound is the bytes written, n 3 T^2 es.
#include "kernels.h"

namespace vnf {

constexpr int AUG_PX = 4, AUG_BLOCK = 256;

__host__ __device__ inline double aug_cubic(double v1, double v2, double v3, double v4, double d) {
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

__host__ __device__ inline int aug_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The three bytes of output pixel (ox, oy) of the T x T crop of one sample.  face: (S,S,3) u8.
__host__ __device__ inline void aug_pixel(const uint8_t* __restrict__ face, int S, const vnf_aug_param& p, int T, int ox, int oy,
                                          uint8_t rgb[3]) {
  rgb[0] = rgb[1] = rgb[2] = 0;
  // flip mirrors the crop; the crop origin is in the padded image; the padding is p.pad per side
  const int rx = p.j + (p.flip ? T - 1 - ox : ox) - p.pad;
  const int ry = p.i + oy - p.pad;
  if (rx < 0 || rx >= S || ry < 0 || ry >= S) return;   // the zero border
  const double xc = rx + 0.5, yc = ry + 0.5;
  double xin = p.m[0] * xc + p.m[1] * yc + p.m[2];
  double yin = p.m[3] * xc + p.m[4] * yc + p.m[5];
  if (xin < 0.0 || xin >= S || yin < 0.0 || yin >= S) return;   // the rotation's fill
  xin -= 0.5;
  yin -= 0.5;
  const double fx = floor(xin), fy = floor(yin);
  const double dx = xin - fx, dy = yin - fy;
  const int x = (int)fx - 1, y = (int)fy - 1;
  const int c0 = aug_clampi(x, S - 1) * 3, c1 = aug_clampi(x + 1, S - 1) * 3, c2 = aug_clampi(x + 2, S - 1) * 3,
            c3 = aug_clampi(x + 3, S - 1) * 3;
  const uint8_t* r0 = face + (size_t)aug_clampi(y, S - 1) * S * 3;
  // rows y+1..y+3: aug_clampi keeps the address inside the image; `in` says whether the row is used at all
  const uint8_t* r1 = face + (size_t)aug_clampi(y + 1, S - 1) * S * 3;
  const uint8_t* r2 = face + (size_t)aug_clampi(y + 2, S - 1) * S * 3;
  const uint8_t* r3 = face + (size_t)aug_clampi(y + 3, S - 1) * S * 3;
  const bool in1 = y + 1 >= 0 && y + 1 < S, in2 = y + 2 >= 0 && y + 2 < S, in3 = y + 3 >= 0 && y + 3 < S;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const double v1 = aug_cubic(r0[c0 + b], r0[c1 + b], r0[c2 + b], r0[c3 + b], dx);
    const double v2 = in1 ? aug_cubic(r1[c0 + b], r1[c1 + b], r1[c2 + b], r1[c3 + b], dx) : v1;
    const double v3 = in2 ? aug_cubic(r2[c0 + b], r2[c1 + b], r2[c2 + b], r2[c3 + b], dx) : v2;
    const double v4 = in3 ? aug_cubic(r3[c0 + b], r3[c1 + b], r3[c2 + b], r3[c3 + b], dx) : v3;
    const double v = aug_cubic(v1, v2, v3, v4, dy);
    rgb[b] = v <= 0.0 ? (uint8_t)0 : (v >= 255.0 ? (uint8_t)255 : (uint8_t)v);
  }
}

template <typename TO>
struct AugVec;
template <>
struct AugVec<float> { typedef float __attribute__((ext_vector_type(4))) type; };
template <>
struct AugVec<_Float16> { typedef _Float16 __attribute__((ext_vector_type(4))) type; };
template <>
struct AugVec<__bf16> { typedef __bf16 __attribute__((ext_vector_type(4))) type; };

// grid (ceil(T * ceil(T / AUG_PX) / AUG_BLOCK), n); vec: T % AUG_PX == 0 and x_out is 16-byte aligned
template <typename TO>
__global__ void __launch_bounds__(AUG_BLOCK) augment_faces_kernel(const uint8_t* __restrict__ faces, int n_faces, int S,
                                                                  const int32_t* __restrict__ index,
                                                                  const vnf_aug_param* __restrict__ params, int T,
                                                                  TO* __restrict__ x_out, uint8_t* __restrict__ u8_out, int vec) {
  const int img = blockIdx.y;
  const int groups = (T + AUG_PX - 1) / AUG_PX;
  const int item = blockIdx.x * AUG_BLOCK + threadIdx.x;
  if (item >= T * groups) return;
  const int oy = item / groups, ox0 = (item - oy * groups) * AUG_PX;
  const int src = index ? index[img] : img;
  const vnf_aug_param p = params[img];
  // an index outside the data set or a crop outside the padded image writes the fill, never reads outside `faces`
  // (the host checks both where it can see them; these live in device memory)
  const int size = S + 2 * p.pad;
  const bool ok = src >= 0 && src < n_faces && p.pad >= 0 && p.pad <= T && p.i >= 0 && p.j >= 0 && p.i <= size - T && p.j <= size - T;
  const uint8_t* face = faces + (size_t)(ok ? src : 0) * S * S * 3;
  uint8_t px[AUG_PX][3];
#pragma unroll
  for (int k = 0; k < AUG_PX; ++k) {
    px[k][0] = px[k][1] = px[k][2] = 0;
    if (ok && ox0 + k < T) aug_pixel(face, S, p, T, ox0 + k, oy, px[k]);
  }
  if (u8_out) {
    uint8_t* o = u8_out + ((size_t)img * T * T + (size_t)oy * T + ox0) * 3;
#pragma unroll
    for (int k = 0; k < AUG_PX; ++k)
      if (ox0 + k < T) {
        o[k * 3 + 0] = px[k][0];
        o[k * 3 + 1] = px[k][1];
        o[k * 3 + 2] = px[k][2];
      }
  }
  if (x_out) {
    TO* o = x_out + (size_t)img * 3 * T * T + (size_t)oy * T + ox0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // np.float32(v), then (v - 127.5) / 128 in fp32 (fix_std on a float32 array), then the cast to the output dtype
      TO v[AUG_PX];
#pragma unroll
      for (int k = 0; k < AUG_PX; ++k) v[k] = (TO)(((float)px[k][c] - 127.5f) / 128.f);
      TO* oc = o + (size_t)c * T * T;
      if (vec) {
        typename AugVec<TO>::type w = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<typename AugVec<TO>::type*>(oc) = w;
      } else {
#pragma unroll
        for (int k = 0; k < AUG_PX; ++k)
          if (ox0 + k < T) oc[k] = v[k];
      }
    }
  }
}

hipError_t launch_augment_faces(const uint8_t* faces, int n_faces, int S, const int32_t* index, const vnf_aug_param* params,
                                int n, int T, void* x_out, int out_dtype, uint8_t* u8_out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n < 0 || n > 65535 || S < 1 || T < 1 || !faces || !params) return hipErrorInvalidValue;
  const int groups = (T + AUG_PX - 1) / AUG_PX;
  const dim3 grid((T * groups + AUG_BLOCK - 1) / AUG_BLOCK, n), block(AUG_BLOCK);
  const int vec = (T % AUG_PX == 0 && ((uintptr_t)x_out & 15) == 0) ? 1 : 0;
  switch (out_dtype) {
    case F32: hipLaunchKernelGGL(augment_faces_kernel<float>, grid, block, 0, s, faces, n_faces, S, index, params, T, (float*)x_out, u8_out, vec); break;
    case BF16: hipLaunchKernelGGL(augment_faces_kernel<__bf16>, grid, block, 0, s, faces, n_faces, S, index, params, T, (__bf16*)x_out, u8_out, vec); break;
    case F16: hipLaunchKernelGGL(augment_faces_kernel<_Float16>, grid, block, 0, s, faces, n_faces, S, index, params, T, (_Float16*)x_out, u8_out, vec); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace vnf
