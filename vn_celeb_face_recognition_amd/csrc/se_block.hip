// Squeeze-and-excitation tail of an IRBlock (models/resnet_encoder.py:98-113, 142-149), NHWC, two launches:
//     gate = sigmoid(W2 . prelu(W1 . mean_hw(t) + b1) + b2)        y = prelu(t * gate + res)
//   se_squeeze_kernel   per (image, pixel slice): fp32 channel sums of t.  A workgroup is (pixel lanes) x (storage units
//                       of a pixel), so a wave reads consecutive 16-byte chunks; every lane adds its pixels in order, the
//                       lanes of a unit are added in lane order through LDS.  No atomics: the slice sums land in
//                       part[image][slice][C] and depend on nothing but (HW, C, layout) -- the same bits in any batch.
//   se_apply_kernel     per (image, chunk): adds the slice sums in slice order, divides once by HW, recomputes the image's
//                       gate (<= 2 * C * C/16 MACs in fp32; every workgroup of an image gets the same bits), then streams
//                       y = prelu(t * gate + res) with one 16-byte access per storage unit, rounding once to the storage
//                       type (split-f16: re-split by Unit<pf16>::store).
#include "kernels.h"
#include "storage_unit.h"

namespace vnf {

constexpr int SE_THREADS = 256, SE_MAX_C = 1024, SE_MAX_SLICES = 16;
constexpr int SE_PIX_PER_LANE = 16;    // pixels a lane of the squeeze adds before another slice is opened
constexpr int SE_UNITS_PER_THREAD = 8;  // storage units a thread of the apply launch streams

static int unit_channels(int dtype) { return dtype_chan_align(dtype); }

int se_slices(int dtype, int HW, int C) {
  const int cu = C / unit_channels(dtype);
  if (cu < 1 || cu > SE_THREADS || HW < 1) return 0;
  const int lanes = SE_THREADS / cu;
  const int want = (HW + lanes * SE_PIX_PER_LANE - 1) / (lanes * SE_PIX_PER_LANE);
  return want < 1 ? 1 : want > SE_MAX_SLICES ? SE_MAX_SLICES : want;
}

template <typename T>
__global__ void __launch_bounds__(SE_THREADS) se_squeeze_kernel(const T* __restrict__ t, int HW, int C, int slices,
                                                                float* __restrict__ part, size_t part_stride) {
  typedef Unit<T> U;
  constexpr int N = U::N;
  __shared__ float sm[SE_THREADS * N];
  const int cu = C / N, lanes = SE_THREADS / cu;
  const int img = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
  const int u = tid % cu, pl = tid / cu;
  const int p0 = (int)((long long)HW * sl / slices), p1 = (int)((long long)HW * (sl + 1) / slices);
  float acc[N];
#pragma unroll
  for (int e = 0; e < N; ++e) acc[e] = 0.f;
  if (pl < lanes) {
    const T* base = t + (size_t)img * HW * C + (size_t)u * N;
    int p = p0 + pl;
    for (; p + lanes < p1; p += 2 * lanes) {   // two loads in flight, added in pixel order
      const typename U::Raw r0 = U::raw(base + (size_t)p * C), r1 = U::raw(base + (size_t)(p + lanes) * C);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] += U::at(r0, e);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] += U::at(r1, e);
    }
    if (p < p1) {
      const typename U::Raw r0 = U::raw(base + (size_t)p * C);
#pragma unroll
      for (int e = 0; e < N; ++e) acc[e] += U::at(r0, e);
    }
#pragma unroll
    for (int e = 0; e < N; ++e) sm[(pl * cu + u) * N + e] = acc[e];
  }
  __syncthreads();
  for (int c = tid; c < C; c += SE_THREADS) {   // channel c = value c % N of unit c / N: sm row pl holds it at index c
    float s = 0.f;
    for (int l = 0; l < lanes; ++l) s += sm[l * C + c];
    part[(size_t)img * part_stride + (size_t)sl * C + c] = s;
  }
}

struct SeGate { const float *w1, *b1, *w2, *b2; float slope_se, slope_out; };

template <typename T>
__global__ void __launch_bounds__(SE_THREADS) se_apply_kernel(const T* __restrict__ t, const T* __restrict__ res, T* __restrict__ y,
                                                              int HW, int C, int slices, const float* __restrict__ part,
                                                              size_t part_stride, SeGate g) {
  typedef Unit<T> U;
  constexpr int N = U::N;
  __shared__ float pooled[SE_MAX_C], gate[SE_MAX_C], hid[SE_MAX_C / 16];
  const int img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = C / 16;
  const float* pi = part + (size_t)img * part_stride;
  for (int c = tid; c < C; c += SE_THREADS) {
    float s = 0.f;
    for (int sl = 0; sl < slices; ++sl) s += pi[(size_t)sl * C + c];
    pooled[c] = s / (float)HW;
  }
  __syncthreads();
  for (int j = wave; j < R; j += SE_THREADS / 64) {   // one wave per hidden unit: lanes stride over c, butterfly sum
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += g.w1[(size_t)j * C + c] * pooled[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
      const float v = s + g.b1[j];
      hid[j] = v > 0.f ? v : v * g.slope_se;
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += SE_THREADS) {
    float z = g.b2[c];
    for (int j = 0; j < R; ++j) z += g.w2[(size_t)c * R + j] * hid[j];
    gate[c] = 1.f / (1.f + expf(-z));
  }
  __syncthreads();
  const int cu = C / N;
  const unsigned total = (unsigned)HW * cu;   // storage units of one image (< 2^31: the launcher checks)
  const size_t ibase = (size_t)img * HW * C;
  for (unsigned i = blockIdx.x * SE_THREADS + tid; i < total; i += gridDim.x * SE_THREADS) {
    const int c0 = (int)(i % cu) * N;
    const size_t off = ibase + (size_t)i * N;
    const typename U::Raw rt = U::raw(t + off), rr = U::raw(res + off);
    float v[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const float x = U::at(rt, e) * gate[c0 + e] + U::at(rr, e);
      v[e] = x > 0.f ? x : x * g.slope_out;
    }
    U::store(y + off, v);
  }
}

template <typename T>
static hipError_t se_go(const void* t, const void* res, void* y, int n, int HW, int C, int slices, const SeWeights& w, float* part,
                        size_t part_stride, hipStream_t s) {
  const size_t units = (size_t)HW * (C / Unit<T>::N);
  const size_t per_wg = (size_t)SE_THREADS * SE_UNITS_PER_THREAD;
  const int chunks = (int)((units + per_wg - 1) / per_wg < 64 ? (units + per_wg - 1) / per_wg : 64);
  hipLaunchKernelGGL(se_squeeze_kernel<T>, dim3(slices, n), dim3(SE_THREADS), 0, s, (const T*)t, HW, C, slices, part, part_stride);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(se_apply_kernel<T>, dim3(chunks, n), dim3(SE_THREADS), 0, s, (const T*)t, (const T*)res, (T*)y, HW, C, slices,
                     part, part_stride, SeGate{w.w1, w.b1, w.w2, w.b2, w.slope_se, w.slope_out});
  return hipGetLastError();
}

hipError_t launch_se_block(const void* t, const void* res, void* y, int dtype, int n, int HW, int C, const SeWeights& w, float* part,
                           size_t part_stride, hipStream_t s) {
  if (dtype != F32 && dtype != BF16 && dtype != F16 && dtype != F16P) return hipErrorInvalidValue;
  const int slices = se_slices(dtype, HW, C);
  if (C < 16 || C % 16 || C > SE_MAX_C || slices < 1 || part_stride < (size_t)slices * C) return hipErrorInvalidValue;
  if ((size_t)HW * C >= ((size_t)1 << 31) || n > 65535) return hipErrorInvalidValue;
  if (n <= 0) return hipSuccess;
  switch (dtype) {
    case BF16: return se_go<__bf16>(t, res, y, n, HW, C, slices, w, part, part_stride, s);
    case F16: return se_go<_Float16>(t, res, y, n, HW, C, slices, w, part, part_stride, s);
    case F32: return se_go<float>(t, res, y, n, HW, C, slices, w, part, part_stride, s);
    default: return se_go<pf16>(t, res, y, n, HW, C, slices, w, part, part_stride, s);
  }
}

}  // namespace vnf
