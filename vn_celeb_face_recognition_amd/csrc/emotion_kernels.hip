// Kernels around the ResNet-50 two-head emotion plan (plan_rn50.cpp build_rn50_2b): the Pillow-exact face transform
// (u8 faces -> bilinear 224x224 -> ToTensor -> Normalize) and the softmax top-k of the class head.  Both are streaming
// kernels: vector loads and stores along the contiguous axis, plain C++ stores.
#include <cmath>
#include <map>
#include <mutex>

#include "kernels.h"
#include "split_f16.h"

namespace vnf {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------- emotion_prep
// trans_emotion_inf (data_loader/__init__.py:74-81) on aligned (n,S,S,3) u8 faces: Resize(224) on a square PIL image is
// Image.resize((224,224), BILINEAR), then ToTensor (x / 255) and Normalize((x - mean) / std).  Pillow resamples in two
// separable 8-bit passes, horizontal first, with 22-bit fixed-point coefficients: acc = 2^21 + sum(pixel * k), result
// clip8(acc >> 22) after EACH pass.  The coefficients depend on S only; the host builds them once per S exactly as Pillow
// does (triangle filter, support max(S/224, 1), windows [int(center - support + 0.5), int(center + support + 0.5)) clamped,
// weights normalised in double, k = int(w * 2^22 + 0.5)) and hands them to the kernel BY VALUE (2.9 KB of kernel
// arguments: no device table, no allocation, nothing to order against the stream).
// One workgroup = PREP_ROWS output rows of one face: the horizontal pass of the source rows those need goes to LDS as
// bytes, the vertical pass reads it and writes the normalised pixels.
constexpr int PREP_OUT = 224, PREP_ROWS = 8, PREP_KS = 3, PREP_MAXR = 12, PREP_BITS = 22;

struct PrepTab {
  int k[PREP_OUT * PREP_KS];     // zero beyond a window's length
  unsigned char lo[PREP_OUT];    // first source index of the window
};

enum PrepForm { PREP_NCHW = 0, PREP_NHWC8 = 1 };

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <typename TO, int FORM>
__global__ void __launch_bounds__(256) emotion_prep_kernel(const uint8_t* __restrict__ faces, int S, TO* __restrict__ out, PrepTab tab) {
  __shared__ uint8_t hrow[PREP_MAXR][PREP_OUT * 3];
  const int img = blockIdx.y, y0 = blockIdx.x * PREP_ROWS;
  const uint8_t* src = faces + (size_t)img * S * S * 3;
  const int r0 = tab.lo[y0];
  int r1 = tab.lo[y0 + PREP_ROWS - 1] + PREP_KS;   // one past the last source row any of the band's windows may touch
  if (r1 > S) r1 = S;
  if (r1 > r0 + PREP_MAXR) r1 = r0 + PREP_MAXR;     // the host refuses an S whose bands need more (never for S <= 224)
  const int nrows = r1 - r0;
  // horizontal pass: (source row, output column, channel)
  for (int i = threadIdx.x; i < nrows * PREP_OUT * 3; i += 256) {
    const int r = i / (PREP_OUT * 3), rem = i - r * (PREP_OUT * 3), xo = rem / 3, c = rem - xo * 3;
    const uint8_t* row = src + (size_t)(r0 + r) * S * 3 + c;
    const int lo = tab.lo[xo];
    int acc = 1 << (PREP_BITS - 1);
#pragma unroll
    for (int t = 0; t < PREP_KS; ++t) {
      const int xi = lo + t < S ? lo + t : S - 1;   // a tap beyond the window has coefficient 0
      acc += (int)row[xi * 3] * tab.k[xo * PREP_KS + t];
    }
    hrow[r][rem] = (uint8_t)clip8(acc >> PREP_BITS);
  }
  __syncthreads();
  // vertical pass + ToTensor + Normalize: one output pixel (3 channels) per item
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  for (int i = threadIdx.x; i < PREP_ROWS * PREP_OUT; i += 256) {
    const int ry = i / PREP_OUT, xo = i - ry * PREP_OUT, yo = y0 + ry;
    const int lo = tab.lo[yo] - r0;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int acc = 1 << (PREP_BITS - 1);
#pragma unroll
      for (int t = 0; t < PREP_KS; ++t) {
        const int ri = lo + t < nrows ? lo + t : nrows - 1;
        acc += (int)hrow[ri][xo * 3 + c] * tab.k[yo * PREP_KS + t];
      }
      v[c] = ((float)clip8(acc >> PREP_BITS) / 255.f - mean[c]) / sd[c];
    }
    if constexpr (FORM == PREP_NCHW) {
      TO* o = out + (size_t)img * 3 * PREP_OUT * PREP_OUT + (size_t)yo * PREP_OUT + xo;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[(size_t)c * PREP_OUT * PREP_OUT] = (TO)v[c];
    } else if constexpr (__is_same(TO, pf16)) {
      f16x8_t h = {0, 0, 0, 0, 0, 0, 0, 0}, l = h;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const sf16 s(v[c]);
        h[c] = s.hi; l[c] = s.lo;
      }
      f16x8_t* o = reinterpret_cast<f16x8_t*>(out + ((size_t)img * PREP_OUT * PREP_OUT + (size_t)yo * PREP_OUT + xo) * 8);
      o[0] = h;
      o[1] = l;
    } else {
      TO o8[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) o8[c] = (TO)(c < 3 ? v[c] : 0.f);
      uint4* o = reinterpret_cast<uint4*>(out + ((size_t)img * PREP_OUT * PREP_OUT + (size_t)yo * PREP_OUT + xo) * 8);
#pragma unroll
      for (int q = 0; q < (int)(8 * sizeof(TO) / 16); ++q) o[q] = reinterpret_cast<const uint4*>(o8)[q];
    }
  }
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c) for in_size -> 224 with the bilinear filter
static bool build_prep_tab(int S, PrepTab* t) {
  const double scale = (double)S / PREP_OUT;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  if ((int)std::ceil(support) * 2 + 1 != PREP_KS) return false;
  for (int xx = 0; xx < PREP_OUT; ++xx) {
    const double center = (xx + 0.5) * scale, ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > S) xmax = S;
    xmax -= xmin;
    if (xmax > PREP_KS) return false;
    double k[PREP_KS] = {0, 0, 0}, ww = 0;
    for (int x = 0; x < xmax; ++x) {
      double a = (x + xmin - center + 0.5) * ss;
      if (a < 0) a = -a;
      k[x] = a < 1.0 ? 1.0 - a : 0.0;
      ww += k[x];
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = 0; x < PREP_KS; ++x)
      t->k[xx * PREP_KS + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << PREP_BITS)) : (int)(0.5 + k[x] * (1 << PREP_BITS));
    t->lo[xx] = (unsigned char)xmin;
  }
  for (int y0 = 0; y0 < PREP_OUT; y0 += PREP_ROWS) {   // every band's source rows fit the LDS strip
    int r1 = t->lo[y0 + PREP_ROWS - 1] + PREP_KS;
    if (r1 > S) r1 = S;
    if (r1 - t->lo[y0] > PREP_MAXR) return false;
  }
  return true;
}

static const PrepTab* prep_tab(int S) {
  static std::mutex mu;
  static std::map<int, PrepTab> cache;   // node addresses are stable
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find(S);
  if (it == cache.end()) {
    PrepTab t;
    if (!build_prep_tab(S, &t)) return nullptr;
    it = cache.emplace(S, t).first;
  }
  return &it->second;
}

hipError_t launch_emotion_prep(const uint8_t* faces, int n, int S, void* out, int out_dtype, bool packed, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (S < 1 || S > PREP_OUT || n < 0 || n > 65535) return hipErrorInvalidValue;
  const PrepTab* t = prep_tab(S);
  if (!t) return hipErrorInvalidValue;
  const dim3 grid(PREP_OUT / PREP_ROWS, n), block(256);
  if (packed) {
    switch (out_dtype) {
      case F32: hipLaunchKernelGGL((emotion_prep_kernel<float, PREP_NHWC8>), grid, block, 0, s, faces, S, (float*)out, *t); break;
      case BF16: hipLaunchKernelGGL((emotion_prep_kernel<__bf16, PREP_NHWC8>), grid, block, 0, s, faces, S, (__bf16*)out, *t); break;
      case F16: hipLaunchKernelGGL((emotion_prep_kernel<_Float16, PREP_NHWC8>), grid, block, 0, s, faces, S, (_Float16*)out, *t); break;
      case F16P: hipLaunchKernelGGL((emotion_prep_kernel<pf16, PREP_NHWC8>), grid, block, 0, s, faces, S, (pf16*)out, *t); break;
      default: return hipErrorInvalidValue;
    }
  } else {
    switch (out_dtype) {
      case F32: hipLaunchKernelGGL((emotion_prep_kernel<float, PREP_NCHW>), grid, block, 0, s, faces, S, (float*)out, *t); break;
      case BF16: hipLaunchKernelGGL((emotion_prep_kernel<__bf16, PREP_NCHW>), grid, block, 0, s, faces, S, (__bf16*)out, *t); break;
      case F16: hipLaunchKernelGGL((emotion_prep_kernel<_Float16, PREP_NCHW>), grid, block, 0, s, faces, S, (_Float16*)out, *t); break;
      default: return hipErrorInvalidValue;
    }
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------- softmax top-k
// find_emotion (demo_image.py:37-47): the k largest logits of a row in descending order and their softmax values.
// One wave per row; round j selects the largest (value, then LOWER index) pair that comes after round j-1's in that
// order, so exact ties come out lower index first (the pinned rule: numpy's argsort gives them no defined order).
// NaN logits are never selected; a row with fewer than k selectable logits pads with index -1, probability 0.  A row
// whose largest logit is -inf has no softmax (torch gives NaN): its indices still come out in order, probabilities 0.
__global__ void softmax_topk_kernel(const float* __restrict__ logits, int n, int C, int k, int32_t* __restrict__ idx,
                                    float* __restrict__ prob) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* x = logits + (size_t)row * C;
  float pv = INFINITY, top = 0.f, sum = 0.f;
  int pi = -1;
  for (int j = 0; j < k; ++j) {
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      const float v = x[c];
      const bool after = v < pv || (v == pv && c > pi);
      if (after && (v > m || (v == m && c < mi))) { m = v; mi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o);
      const int oi = __shfl_xor(mi, o);
      if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    if (j == 0) {
      top = m;
      for (int c = lane; c < C; c += 64) {
        const float e = expf(x[c] - top);
        sum += e == e ? e : 0.f;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    }
    const bool found = mi != 0x7fffffff;
    if (lane == 0) {
      idx[(size_t)row * k + j] = found ? mi : -1;
      prob[(size_t)row * k + j] = (found && sum > 0.f) ? expf(m - top) / sum : 0.f;
    }
    if (!found) { pv = -INFINITY; pi = 0x7fffffff; } else { pv = m; pi = mi; }
  }
}

hipError_t launch_softmax_topk(const float* logits, int n, int C, int k, int32_t* idx, float* prob, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (k < 1 || k > 16 || k > C) return hipErrorInvalidValue;
  hipLaunchKernelGGL(softmax_topk_kernel, dim3((n + 3) / 4), dim3(256), 0, s, logits, n, C, k, idx, prob);
  return hipGetLastError();
}

// rows of fp32 (n, C) from a pitched source to a pitched destination (the two heads out of the plan's logit buffer)
__global__ void copy_rows_f32_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd, int n, int C) {
  const size_t total = (size_t)n * C;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / C;
    const int c = (int)(i - r * C);
    dst[r * ldd + c] = src[r * lds + c];
  }
}

hipError_t launch_copy_rows_f32(const float* src, int lds, float* dst, int ldd, int n, int C, hipStream_t s) {
  const size_t total = (size_t)n * C;
  if (total == 0) return hipSuccess;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(copy_rows_f32_kernel, dim3(blocks), dim3(256), 0, s, src, lds, dst, ldd, n, C);
  return hipGetLastError();
}

}  // namespace vnf
