// HBM-bound helper kernels around the convolution core: layout packing, pooling, L2 norm.
// All are coalesced streaming kernels (16-byte accesses along the NHWC channel axis).
#include <cstdlib>
#include <algorithm>
#include <type_traits>
#include "conv_device.h"
#include "kernels.h"
#include "storage_unit.h"

namespace vnf {

template <typename T> __device__ __forceinline__ float to_f(T v) { return (float)v; }

// ---------------------------------------------------------------- NCHW (n,3,S,S) -> NHWC8
template <typename TI, typename TO>
__global__ void pack_input_kernel(const TI* __restrict__ x, TO* __restrict__ y, int n, int hw) {
  const size_t total = (size_t)n * hw;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / hw, p = i - img * hw;
    const TI* src = x + img * 3 * (size_t)hw + p;
    if constexpr (sizeof(TO) == sizeof(pf16) && __is_same(TO, pf16)) {
      const float v[8] = {to_f(src[0]), to_f(src[hw]), to_f(src[2 * (size_t)hw]), 0.f, 0.f, 0.f, 0.f, 0.f};
      Unit<pf16>::store(y + i * 8, v);
    } else {
      TO o[8];
      o[0] = (TO)to_f(src[0]);
      o[1] = (TO)to_f(src[hw]);
      o[2] = (TO)to_f(src[2 * (size_t)hw]);
#pragma unroll
      for (int c = 3; c < 8; ++c) o[c] = (TO)0.f;
      TO* dst = y + i * 8;
      if constexpr (sizeof(TO) == 2) {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
      } else {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(o);
        *reinterpret_cast<uint4*>(dst + 4) = *reinterpret_cast<const uint4*>(o + 4);
      }
    }
  }
}

template <typename TI>
static hipError_t pack_dispatch_out(const void* x, void* out, int dtype, int n, int hw, hipStream_t s) {
  const size_t total = (size_t)n * hw;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  if (blocks == 0) return hipSuccess;
  switch (dtype) {
    case BF16: hipLaunchKernelGGL((pack_input_kernel<TI, __bf16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (__bf16*)out, n, hw); break;
    case F16: hipLaunchKernelGGL((pack_input_kernel<TI, _Float16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (_Float16*)out, n, hw); break;
    case F32: hipLaunchKernelGGL((pack_input_kernel<TI, float>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (float*)out, n, hw); break;
    case F16P: hipLaunchKernelGGL((pack_input_kernel<TI, pf16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (pf16*)out, n, hw); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_pack_input(const void* x, int x_dtype, void* out, int dtype, int n, int hw, hipStream_t s) {
  switch (x_dtype) {
    case F32: return pack_dispatch_out<float>(x, out, dtype, n, hw, s);
    case BF16: return pack_dispatch_out<__bf16>(x, out, dtype, n, hw, s);
    case F16: return pack_dispatch_out<_Float16>(x, out, dtype, n, hw, s);
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------- IRv1 stem: NCHW input -> conv2d_1a, direct
// inception_resnet_v1.py:281 (BasicConv2d 3->32, 3x3 stride 2, folded BN, ReLU) straight from the caller's NCHW
// tensor: no NHWC8 staging pass (it wrote and re-read 105 MB per 256 images) and no 3->8 channel padding in an
// MFMA K of 72 that is 62 % zeros.  One thread per output pixel, 32 channels as 16 packed-FMA pairs in the
// reference's (c,kh,kw) order, fp32 weights [27][32] read as wave-uniform scalars, one 64/128-byte NHWC row out.
typedef float f2_t __attribute__((ext_vector_type(2)));

template <typename TI, typename TO>
__global__ void __launch_bounds__(256) stem_conv1a_kernel(const TI* __restrict__ x, TO* __restrict__ y, int ldy, int n,
                                                          const float* __restrict__ wt) {
  constexpr int S = 160, SO = 79;
  const unsigned total = (unsigned)n * SO * SO;
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const unsigned img = i / (SO * SO), p = i - img * (SO * SO);
  const int oy = (int)(p / SO), ox = (int)(p - (unsigned)oy * SO);
  const TI* src = x + (size_t)img * 3 * S * S + (size_t)(2 * oy) * S + 2 * ox;
  float in[27];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) in[(c * 3 + kh) * 3 + kw] = to_f(src[(size_t)c * S * S + kh * S + kw]);
  f2_t acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = f2_t{wt[27 * 32 + 2 * j], wt[27 * 32 + 2 * j + 1]};
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const f2_t v2 = {in[k], in[k]};
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = __builtin_elementwise_fma(v2, f2_t{wt[k * 32 + 2 * j], wt[k * 32 + 2 * j + 1]}, acc[j]);
  }
  if constexpr (__is_same(TO, pf16)) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[2 * j] = fmaxf(acc[4 * u + j][0], 0.f); v[2 * j + 1] = fmaxf(acc[4 * u + j][1], 0.f); }
      Unit<pf16>::store(y + (size_t)i * ldy + u * 8, v);
    }
  } else {
    TO o[32];
#pragma unroll
    for (int j = 0; j < 16; ++j) { o[2 * j] = (TO)fmaxf(acc[j][0], 0.f); o[2 * j + 1] = (TO)fmaxf(acc[j][1], 0.f); }
    uint4* dst = reinterpret_cast<uint4*>(y + (size_t)i * ldy);
#pragma unroll
    for (int q = 0; q < (int)(32 * sizeof(TO) / 16); ++q) dst[q] = reinterpret_cast<const uint4*>(o)[q];
  }
}

// Prologue and epilogue of the two MFMA forms below.  Lane (row col, k slot g) keeps w[k = 4t + g][channel 16 ct + col]
// of the 7 k-steps and both channel tiles, and the bias of the channels 16 ct + 4g .. + 3 its accumulators hold; cst is
// the first of the 8 channels it stores after the lane-row swap.  tap(t, k): the kernel's own set-up of k-step t, where
// its lane fetches tap k.
template <class Tap>
__device__ __forceinline__ void stem1a_lane(const float* __restrict__ wt, int col, int g, float (&wa)[2][7],
                                            float (&bias)[2][4], int& cst, Tap tap) {
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int k = 4 * t + g;
    wa[0][t] = k < 27 ? wt[k * 32 + col] : 0.f;
    wa[1][t] = k < 27 ? wt[k * 32 + 16 + col] : 0.f;
    tap(t, k);
  }
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int e = 0; e < 4; ++e) bias[ct][e] = wt[27 * 32 + 16 * ct + 4 * g + e];
  cst = (g & 1) * 16 + (g >> 1) * 8;
}
// ReLU, rounding to TO, lane-row swap and the 16-byte store(s) of one pixel's 8 channels at d (every lane calls; ok: this
// lane's pixel exists)
template <typename TO>
__device__ __forceinline__ void stem1a_store(TO* d, bool ok, const f32x4_t& a0, const f32x4_t& a1) {
  f32x4_t r0, r1;
#pragma unroll
  for (int e = 0; e < 4; ++e) { r0[e] = fmaxf(a0[e], 0.f); r1[e] = fmaxf(a1[e], 0.f); }
  swap_store<TO>(reinterpret_cast<char*>(d), ok, r0, r1);
}

// The same convolution on the f32 MFMA (v_mfma_f32_16x16x4_f32: the f32 vector rate, exact fmaf chain in k order, so
// bit-identical to the kernel above), for the 16-bit and planar split-f16 plans.  The VALU form reads its 27 x 32 weights
// as wave-uniform scalars at every tap -- 864 values do not fit the SGPR file, and the refetch, not the FMAs, set its
// time in the split-f16 plan (0.098 -> 0.07 ms; bf16: 0.062 -> 0.059, where the rest is index arithmetic and the two
// memory streams).  Here the weights are the A operand: lane (row r, k slot g) keeps
// w[k = 4t + g][channel 16 ct + r] for the 7 k-steps and both channel tiles in 14 VGPRs, loaded once; B = 16 output
// pixels, lane (pixel, g) fetching tap k = 4t + g of its pixel; D = channels 4g .. 4g+3 of the pixel per tile.  A lane-row
// swap between the two tiles gives every lane 8 channels = one 16-byte store (planar: one hi and one lo chunk).
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) stem_conv1a_mfma_kernel(const TI* __restrict__ x, TO* __restrict__ y, int ldy, int n,
                                                               const float* __restrict__ wt) {
  constexpr int S = 160, SO = 79, NPX = SO * SO, G = 4;   // G pixel groups of 16 per wave iteration
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const unsigned total = (unsigned)n * NPX;
  const unsigned ngroups = (total + 15) / 16;
  const unsigned nwaves = gridDim.x * 4, w0 = blockIdx.x * 4 + (threadIdx.x >> 6);
  float wa[2][7], bias[2][4];
  // koff: element offset of tap k = 4t + g from the pixel's first tap.  It is filled inside stem1a_lane's weight loop: in
  // a loop of its own the kernel holds every tap address at once (84 -> 104-108 registers, an occupancy step)
  int cst, koff[7];
  stem1a_lane(wt, col, g, wa, bias, cst,
              [&](int t, int k) { koff[t] = k < 27 ? (k / 9) * S * S + ((k % 9) / 3) * S + k % 3 : 0; });
  for (unsigned gi = w0 * G; gi < ngroups; gi += nwaves * G) {
    float xb[G][7];
#pragma unroll
    for (int q = 0; q < G; ++q) {
      const unsigned i = min((gi + q) * 16 + col, total - 1);
      const unsigned img = i / NPX, p = i - img * NPX;
      const int oy = (int)(p / SO), ox = (int)(p - (unsigned)oy * SO);
      const TI* src = x + (size_t)img * 3 * S * S + (size_t)(2 * oy) * S + 2 * ox;
#pragma unroll
      for (int t = 0; t < 7; ++t) xb[q][t] = to_f(src[koff[t]]);
    }
#pragma unroll
    for (int q = 0; q < G; ++q) {
      f32x4_t a0 = {bias[0][0], bias[0][1], bias[0][2], bias[0][3]};
      f32x4_t a1 = {bias[1][0], bias[1][1], bias[1][2], bias[1][3]};
#pragma unroll
      for (int t = 0; t < 7; ++t) {
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[0][t], xb[q][t], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[1][t], xb[q][t], a1, 0, 0, 0);
      }
      const unsigned i = (gi + q) * 16 + col;
      stem1a_store(y + (size_t)i * ldy + cst, gi + q < ngroups && i < total, a0, a1);
    }
  }
}

// The MFMA form fed from LDS-staged input rows.  Above, every lane gathers its 7 taps with 7 two-byte global loads per
// 16-pixel group: ~700 k divergent wave-level gathers per 256 images, every input element pulled 2.2 times, and a wave
// waits for its 28 loads before its 56 MFMAs.  Here a band is R = 4 output rows of one image, one row per wave: the
// 3 x 9 input rows it touches are contiguous per channel, so they arrive with coalesced 16-byte loads and sit in LDS
// as raw TI elements, [c][row][160] (8.6 KB for 2-byte crops, 17.3 KB for fp32 crops).  Workgroups are persistent
// (4 per CU, 5 bands each at 256 images) and the LDS is two such buffers: the next band's loads are issued before the
// current band's MFMAs and written to the other buffer after them, one barrier per band.
// A group is 16 consecutive pixels of the wave's row (5 per row, the last with 15): lane (pixel, g) reads its 7 taps
// from LDS -- the 16 pixels of a tap hit 16 different banks (2-byte crops; every other bank for fp32), kw neighbours
// share a dword, kh neighbours sit 80 dwords on.  With the row fixed per wave and the group and buffer unrolled, every
// tap address is one per-lane register (set once per kernel) plus an immediate: besides the MFMAs a group costs its 7
// conversions and the epilogue, which is what lets the vector issue of four waves fit under the MFMA pipe (with the
// addresses computed per group, 6 vector instructions per MFMA, the two added up: 46 us of which 18 us MFMA).
// MFMAs of 3 (then 2) groups are interleaved k-step by k-step, so no accumulator is needed within its 40-cycle latency.
// The arithmetic is the kernel above's, operand for operand: wa[ct][t] with k = 4t + g as A, bias as the initial
// accumulator, the padding slot k = 27 reading tap 0 against a zero weight, the same ReLU / conversion / lane-row swap /
// 16-byte store -- so the tensor is bit-identical.  Needs x 16-byte aligned (row and channel starts then are too); the
// launcher falls back to the gather form otherwise.
struct Stem1aRows { static constexpr int R = 4, NB = (79 + R - 1) / R; };   // output rows per band, bands per image

template <typename TI, typename TO>
__global__ void __launch_bounds__(256) stem_conv1a_rows_kernel(const TI* __restrict__ x, TO* __restrict__ y, int ldy, int n,
                                                               const float* __restrict__ wt) {
  constexpr int S = 160, SO = 79, NPX = SO * SO, R = Stem1aRows::R, NB = Stem1aRows::NB, ES = (int)sizeof(TI);
  static_assert(R == 4, "one output row per wave");
  constexpr int RI = 2 * R + 1, CS = RI * S;             // input rows of a full band; LDS channel stride in elements
  constexpr int RC = S * ES / 16, CSC = CS * ES / 16;    // 16-byte chunks per input row / per LDS channel
  constexpr int NLD = (3 * RI * RC + 255) / 256;         // chunks per thread
  // a buffer and 16 bytes: lane 15 of a row's last group (pixel 79, not stored) reads up to one element past the rows
  constexpr int BUFB = 3 * CS * ES + 16;
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) char sm[2 * BUFB];
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nbands = n * NB;
  u4 v[NLD];
  // band b = (image, rows oy0 .. oy0 + rows): its 2 rows + 1 input rows are contiguous per channel (cpc chunks), and
  // 2 oy0 + 2 rows <= 158, so every staged row is in the image
  auto fetch = [&](int b) {
    const int img = b / NB, oy0 = (b - img * NB) * R;
    const int cpc = (2 * min(R, SO - oy0) + 1) * RC;
    const u4* src = reinterpret_cast<const u4*>(x + (size_t)img * 3 * S * S + (size_t)(2 * oy0) * S);
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int q = min(tid + j * 256, 3 * cpc - 1);       // past the end: the last chunk again, not stored
      const int c = (q >= cpc) + (q >= 2 * cpc);
      v[j] = src[c * (S * S * ES / 16) + q - c * cpc];
    }
  };
  auto stash = [&](int b, int buf) {
    const int oy0 = (b % NB) * R;
    const int cpc = (2 * min(R, SO - oy0) + 1) * RC;
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int q = tid + j * 256;
      const int c = (q >= cpc) + (q >= 2 * cpc);
      if (q < 3 * cpc) reinterpret_cast<u4*>(sm + buf * BUFB)[c * CSC + q - c * cpc] = v[j];
    }
  };
  int band = blockIdx.x;
  if (band >= nbands) return;
  float wa[2][7], bias[2][4];
  // la: byte offset in a buffer of tap k = 4t + g of this lane's pixel in the wave's row, group 0; filled inside
  // stem1a_lane's weight loop like koff above, so that both kernels share one prologue
  int cst, la[7];
  stem1a_lane(wt, col, g, wa, bias, cst, [&](int t, int k) {
    la[t] = (2 * wave * S + 2 * col + (k < 27 ? (k / 9) * CS + ((k % 9) / 3) * S + k % 3 : 0)) * ES;
  });
  fetch(band);
  stash(band, 0);
  // nothing of the prologue is pending inside the band loop: the compiler would otherwise drain the vector-memory
  // counter in front of the MFMAs (which read wa) and with it the next band's loads
  __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)

  // groups J0 .. J0 + NJ of the wave's row, from buffer BUF
  auto groups = [&](auto buf_c, auto j0_c, auto nj_c, unsigned row0) {
    constexpr int BUF = decltype(buf_c)::value, J0 = decltype(j0_c)::value, NJ = decltype(nj_c)::value;
    float xb[NJ][7];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int t = 0; t < 7; ++t)
        xb[j][t] = to_f(*reinterpret_cast<const TI*>(sm + la[t] + (BUF * BUFB + (J0 + j) * 32 * ES)));
    f32x4_t a0[NJ], a1[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      a0[j] = f32x4_t{bias[0][0], bias[0][1], bias[0][2], bias[0][3]};
      a1[j] = f32x4_t{bias[1][0], bias[1][1], bias[1][2], bias[1][3]};
    }
#pragma unroll
    for (int t = 0; t < 7; ++t)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        a0[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[0][t], xb[j][t], a0[j], 0, 0, 0);
        a1[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[1][t], xb[j][t], a1[j], 0, 0, 0);
      }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      stem1a_store(y + (size_t)(row0 + (J0 + j) * 16 + col) * ldy + cst, (J0 + j + 1) * 16 <= SO || col < SO - (J0 + j) * 16,
                   a0[j], a1[j]);
  };
  // one band out of buffer BUF; false when it was this workgroup's last
  auto one_band = [&](auto buf_c) {
    constexpr int BUF = decltype(buf_c)::value;
    const int next = band + gridDim.x;
    if (next < nbands) fetch(next);            // in flight under this band's MFMAs
    // this band's rows are visible; every wave is past its reads of the other buffer (the band before)
    __syncthreads();
    const int img = band / NB, oy0 = (band - img * NB) * R;
    if (wave < min(R, SO - oy0)) {             // the image's last band has 3 rows
      const unsigned row0 = (unsigned)img * NPX + (unsigned)((oy0 + wave) * SO);
      groups(buf_c, std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{}, row0);
      groups(buf_c, std::integral_constant<int, 3>{}, std::integral_constant<int, 2>{}, row0);
    }
    if (next < nbands) stash(next, BUF ^ 1);   // visible after the next band's barrier
    band = next;
    return next < nbands;
  };
  while (one_band(std::integral_constant<int, 0>{}) && one_band(std::integral_constant<int, 1>{})) {}
}

// mode (VNF_STEM1A_MFMA): 2 = MFMA from LDS-staged rows, 1 = MFMA with per-lane gathers, 0 = VALU
template <typename TI>
static hipError_t stem_dispatch_out(const void* x, void* y, int ldy, int dtype, int n, const float* wt, int mode, hipStream_t s) {
  if (mode >= 2 && n > 0 && (dtype == BF16 || dtype == F16 || dtype == F16P) && ((uintptr_t)x & 15) == 0) {
    const int blocks = std::min(n * Stem1aRows::NB, 1024);   // 4 workgroups per CU walk the bands (5 each at 256 images)
    if (dtype == BF16) hipLaunchKernelGGL((stem_conv1a_rows_kernel<TI, __bf16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (__bf16*)y, ldy, n, wt);
    else if (dtype == F16) hipLaunchKernelGGL((stem_conv1a_rows_kernel<TI, _Float16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (_Float16*)y, ldy, n, wt);
    else hipLaunchKernelGGL((stem_conv1a_rows_kernel<TI, pf16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (pf16*)y, ldy, n, wt);
    return hipGetLastError();
  }
  if (mode != 0 && n > 0 && (dtype == BF16 || dtype == F16 || dtype == F16P)) {
    const unsigned ngroups = ((unsigned)n * 79 * 79 + 15) / 16;
    const int blocks = (int)((ngroups + 15) / 16 < 2048 ? (ngroups + 15) / 16 : 2048);   // 4 waves x 4 groups per block round
    if (dtype == BF16) hipLaunchKernelGGL((stem_conv1a_mfma_kernel<TI, __bf16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (__bf16*)y, ldy, n, wt);
    else if (dtype == F16) hipLaunchKernelGGL((stem_conv1a_mfma_kernel<TI, _Float16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (_Float16*)y, ldy, n, wt);
    else hipLaunchKernelGGL((stem_conv1a_mfma_kernel<TI, pf16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (pf16*)y, ldy, n, wt);
    return hipGetLastError();
  }
  const unsigned total = (unsigned)n * 79 * 79;
  const int blocks = (int)((total + 255) / 256);
  if (blocks == 0) return hipSuccess;
  switch (dtype) {
    case BF16: hipLaunchKernelGGL((stem_conv1a_kernel<TI, __bf16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (__bf16*)y, ldy, n, wt); break;
    case F16: hipLaunchKernelGGL((stem_conv1a_kernel<TI, _Float16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (_Float16*)y, ldy, n, wt); break;
    case F32: hipLaunchKernelGGL((stem_conv1a_kernel<TI, float>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (float*)y, ldy, n, wt); break;
    case F16P: hipLaunchKernelGGL((stem_conv1a_kernel<TI, pf16>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (pf16*)y, ldy, n, wt); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_stem_conv1a(const void* x, int x_dtype, void* y, int ldy, int dtype, int n, const float* wt, int mode,
                              hipStream_t s) {
  switch (x_dtype) {
    case F32: return stem_dispatch_out<float>(x, y, ldy, dtype, n, wt, mode, s);
    case BF16: return stem_dispatch_out<__bf16>(x, y, ldy, dtype, n, wt, mode, s);
    case F16: return stem_dispatch_out<_Float16>(x, y, ldy, dtype, n, wt, mode, s);
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------- max pool K x K stride 2
// One thread per (output pixel, storage unit), NHWC slice -> NHWC slice; padding and the part of a ceil-mode window that
// hangs over the border compare as -inf.  Every window the plans use has a tap inside the image, so -inf reaches the
// output only where all of a window's inputs are -inf.  Split-f16: the max of the recombined values is re-split, which
// reproduces the (hi, lo) pair of the largest value bit for bit.
// INSIDE: every tap of every window lies in the image (floor mode, no padding): no bounds tests, and with 16-byte units
// all K*K loads are in flight before the first fmaxf (kept as loaded: their fp32 values would double the registers).
template <typename T, int K, int PAD, bool INSIDE>
__global__ void maxpool_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, int n, int H, int W, int C,
                               int Ho, int Wo) {
  typedef Unit<T> U;
  constexpr int N = U::N;
  // the instances that are neither INSIDE nor padded are the ceil-mode windows (a few thousand MTCNN crops): their tap
  // loops stay rolled, one load at a time, as they always were (20 / 24 VGPRs; unrolled 24 / 27)
  constexpr bool kCeil = !INSIDE && PAD == 0;
  constexpr int TAPS = kCeil ? 1 : K;   // unroll factor of the tap loops
  const int cc = C / N;
  const unsigned total = (unsigned)n * Ho * Wo * cc;  // < 2^31, checked by the launcher: 32-bit index math
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned p = i / cc;
    const int c = (int)(i - p * cc) * N;
    const unsigned q = p / Wo;
    const int wo = (int)(p - q * Wo);
    const unsigned img = q / Ho;
    const int ho = (int)(q - img * Ho);
    float m[N];
#pragma unroll
    for (int e = 0; e < N; ++e) m[e] = -INFINITY;
    if constexpr (INSIDE && sizeof(typename U::Raw) == 16) {
      const T* xi = x + ((size_t)img * H * W + (size_t)(2 * ho) * W + 2 * wo) * ldx + c;
      typename U::Raw r[K * K];
#pragma unroll
      for (int dh = 0; dh < K; ++dh)
#pragma unroll
        for (int dw = 0; dw < K; ++dw) r[dh * K + dw] = U::raw(xi + (size_t)(dh * W + dw) * ldx);
#pragma unroll
      for (int t = 0; t < K * K; ++t)
#pragma unroll
        for (int e = 0; e < N; ++e) m[e] = fmaxf(m[e], U::at(r[t], e));
    } else {
      const T* xi = x + (size_t)img * H * W * ldx + c;
#pragma unroll TAPS
      for (int dh = 0; dh < K; ++dh)
#pragma unroll TAPS
        for (int dw = 0; dw < K; ++dw) {
          const int yy = 2 * ho - PAD + dh, xx = 2 * wo - PAD + dw;
          if (INSIDE || ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)) {
            float v[N];
            U::load(xi + (size_t)(yy * W + xx) * ldx, v);
#pragma unroll
            for (int e = 0; e < N; ++e) m[e] = fmaxf(m[e], v[e]);
          }
        }
    }
    U::store(y + (size_t)p * ldy + c, m);
  }
}

struct PoolArgs { const void* x; int ldx; void* y; int ldy, n, H, W, C, Ho, Wo, blocks; hipStream_t s; };

template <typename T, int K, int PAD, bool INSIDE>
static void maxpool_go(const PoolArgs& a) {
  hipLaunchKernelGGL((maxpool_kernel<T, K, PAD, INSIDE>), dim3(a.blocks), dim3(256), 0, a.s, (const T*)a.x, a.ldx, (T*)a.y, a.ldy,
                     a.n, a.H, a.W, a.C, a.Ho, a.Wo);
}

// the windows the plans use, each in the layouts that reach it
static const struct { PoolWindow w; int dtype; void (*go)(const PoolArgs&); } kPools[] = {
    // 3x3 floor: IRv1 (maxpool_3a, mixed_6a, mixed_7a)
    {{3, 0, false}, F32, maxpool_go<float, 3, 0, true>},     {{3, 0, false}, BF16, maxpool_go<__bf16, 3, 0, true>},
    {{3, 0, false}, F16, maxpool_go<_Float16, 3, 0, true>},  {{3, 0, false}, F16P, maxpool_go<pf16, 3, 0, true>},
    // 3x3 ceil: R-Net, O-Net pool2;  2x2 ceil: O-Net pool3
    {{3, 0, true}, F32, maxpool_go<float, 3, 0, false>},     {{3, 0, true}, F16X2, maxpool_go<sf16, 3, 0, false>},
    {{2, 0, true}, F32, maxpool_go<float, 2, 0, false>},     {{2, 0, true}, F16X2, maxpool_go<sf16, 2, 0, false>},
    // 3x3 pad 1: ResNet-50 stem, vnf_maxpool3s2p1
    {{3, 1, false}, F32, maxpool_go<float, 3, 1, false>},    {{3, 1, false}, BF16, maxpool_go<__bf16, 3, 1, false>},
    {{3, 1, false}, F16, maxpool_go<_Float16, 3, 1, false>}, {{3, 1, false}, F16X2, maxpool_go<sf16, 3, 1, false>},
    {{3, 1, false}, F16P, maxpool_go<pf16, 3, 1, false>},
    // 2x2 floor: SE-IR ResNet-101 stem
    {{2, 0, false}, F32, maxpool_go<float, 2, 0, true>},     {{2, 0, false}, BF16, maxpool_go<__bf16, 2, 0, true>},
    {{2, 0, false}, F16, maxpool_go<_Float16, 2, 0, true>},  {{2, 0, false}, F16P, maxpool_go<pf16, 2, 0, true>},
};

hipError_t launch_maxpool(const void* x, int ldx, void* y, int ldy, int dtype, int n, int H, int W, int C, PoolWindow w,
                          hipStream_t s) {
  const int Ho = pool_out_size(H, w), Wo = pool_out_size(W, w);
  const int ch = dtype_chan_align(dtype);
  if (H < 1 || W < 1 || Ho < 1 || Wo < 1 || C % ch || ldx % ch || ldy % ch) return hipErrorInvalidValue;
  const size_t total = (size_t)n * Ho * Wo * (C / ch);
  if (total == 0) return hipSuccess;
  if (total >= (1u << 31)) return hipErrorInvalidValue;
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  for (const auto& p : kPools)
    if (p.w.k == w.k && p.w.pad == w.pad && p.w.ceil == w.ceil && p.dtype == dtype) {
      p.go(PoolArgs{x, ldx, y, ldy, n, H, W, C, Ho, Wo, blocks, s});
      return hipGetLastError();
    }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------- global average pool
// one thread per (image, storage unit): every channel is summed over p = 0 .. HW-1 in that order and divided once
template <typename T>
__global__ void avgpool_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int n, int HW, int C) {
  constexpr int N = Unit<T>::N;
  const int cc = C / N;
  const size_t total = (size_t)n * cc;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t img = i / cc;
    const int c = (int)(i - img * cc) * N;
    float s[N], v[N];
#pragma unroll
    for (int e = 0; e < N; ++e) s[e] = 0.f;
    for (int p = 0; p < HW; ++p) {
      Unit<T>::load(x + (img * HW + p) * (size_t)ldx + c, v);
#pragma unroll
      for (int e = 0; e < N; ++e) s[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < N; ++e) s[e] = s[e] / (float)HW;
    Unit<T>::store(y + img * C + c, s);
  }
}

template <typename T>
static hipError_t avgpool_go(const void* x, int ldx, void* y, int n, int HW, int C, hipStream_t s) {
  const size_t total = (size_t)n * (C / Unit<T>::N);
  hipLaunchKernelGGL(avgpool_kernel<T>, dim3((int)((total + 255) / 256)), dim3(256), 0, s, (const T*)x, ldx, (T*)y, n, HW, C);
  return hipGetLastError();
}

hipError_t launch_avgpool(const void* x, int ldx, void* y, int dtype, int n, int HW, int C, hipStream_t s) {
  const int ch = dtype_chan_align(dtype);
  if (C % ch || ldx % ch) return hipErrorInvalidValue;
  if ((size_t)n * C == 0) return hipSuccess;
  switch (dtype) {
    case BF16: return avgpool_go<__bf16>(x, ldx, y, n, HW, C, s);
    case F16: return avgpool_go<_Float16>(x, ldx, y, n, HW, C, s);
    case F32: return avgpool_go<float>(x, ldx, y, n, HW, C, s);
    case F16P: return avgpool_go<pf16>(x, ldx, y, n, HW, C, s);
  }
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------- row-wise L2 normalisation
// one wave per row: F.normalize(x, p=2, dim=1) = x / max(||x||, 1e-12) (inception_resnet_v1.py:302)
__global__ void l2norm_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int C) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* xr = x + (size_t)row * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c] * xr[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float d = fmaxf(sqrtf(s), 1e-12f);
  for (int c = lane; c < C; c += 64) y[(size_t)row * C + c] = xr[c] / d;
}

hipError_t launch_l2norm(const float* x, float* y, int n, int C, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(l2norm_kernel, dim3((n + 3) / 4), dim3(256), 0, s, x, y, n, C);
  return hipGetLastError();
}

// ---------------------------------------------------------------- depthwise 3x3 (MobileNetV1 blocks of RetinaFace)
// HBM-bound: one thread per (pixel, 4 channels), nine 16-byte loads, taps in (kh, kw) order as the reference's
// grouped conv sums them
// SPLIT: the tensor holds split-f16 (hi, lo) pairs in its 32-bit elements (the F16X2 plans) instead of fp32
template <bool SPLIT> __device__ __forceinline__ float ldv(float raw) { return SPLIT ? (float)__builtin_bit_cast(sf16, raw) : raw; }
template <bool SPLIT> __device__ __forceinline__ float stv(float v) { return SPLIT ? __builtin_bit_cast(float, sf16(v)) : v; }

template <bool SPLIT>
__global__ void dwconv3x3_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int H, int W, int C, int stride,
                                 int Ho, int Wo, const float* __restrict__ w9c, const float* __restrict__ bias, float slope) {
  const int c4 = C >> 2;
  const size_t total = (size_t)n * Ho * Wo * c4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4) * 4;
    const size_t p = i / c4;
    const int wo = (int)(p % Wo);
    const size_t q = p / Wo;
    const int ho = (int)(q % Ho);
    const size_t img = q / Ho;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int hi = ho * stride - 1 + kh, wi = wo * stride - 1 + kw;
        if ((unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W) {
          const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + ((img * H + hi) * W + wi) * C + c);
          const f32x4_t ww = *reinterpret_cast<const f32x4_t*>(w9c + (kh * 3 + kw) * C + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = acc[e] + ldv<SPLIT>(v[e]) * ww[e];
        }
      }
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(bias + c);
    f32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = acc[e] + b[e];
      o[e] = stv<SPLIT>(v > 0.f ? v : v * slope);
    }
    *reinterpret_cast<f32x4_t*>(y + p * C + c) = o;
  }
}

hipError_t launch_dwconv3x3(const float* x, float* y, int n, int H, int W, int C, int stride, const float* w9c,
                            const float* bias, float slope, bool split, hipStream_t s) {
  if (C % 4 || (stride != 1 && stride != 2)) return hipErrorInvalidValue;
  const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
  const size_t total = (size_t)n * Ho * Wo * (C / 4);
  if (total == 0) return hipSuccess;
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  if (split) hipLaunchKernelGGL(dwconv3x3_kernel<true>, dim3(blocks), dim3(256), 0, s, x, y, n, H, W, C, stride, Ho, Wo, w9c, bias, slope);
  else hipLaunchKernelGGL(dwconv3x3_kernel<false>, dim3(blocks), dim3(256), 0, s, x, y, n, H, W, C, stride, Ho, Wo, w9c, bias, slope);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// RetinaFace / MobileNetV1-0.25 early layers on the MFMA lane layout (fp32, exact v_mfma_f32_16x16x4_f32).
//
// The first layers of that network are pure data movement (a 1080p frame is 33 MB as NHWC4 fp32, conv0's output 133 MB,
// the 8->16 pointwise output 265 MB per 8 frames ...), with channel counts (3, 8, 16, 32) far below what the tiled
// implicit-GEMM kernel is built for.  Two kernels replace them:
//   * retina_stem_kernel: u8 RGB frame -> (x - mean) -> 3x3 stride-2 pad-1 conv 3->8 + folded BN + LeakyReLU, straight
//     from the frame bytes (no NHWC4 fp32 staging tensor).  One wave = 16 output pixels: B = the 27 taps of a pixel
//     (k = (kh*3+kw)*3 + c, lane group = k mod 4), A = weights (7 VGPRs), one MFMA per 4 k.
//   * dwpw_kernel<CIN,COUT>: depthwise 3x3 (+BN+LeakyReLU) and the pointwise 1x1 (+BN+LeakyReLU) that follows it in
//     conv_dw (components.py:30-40) in one pass: lane (pixel l&15, group l>>4) computes the depthwise outputs of
//     channels {4s + group}, which is exactly the B operand of k-step s of the pointwise GEMM; the depthwise tensor
//     never reaches memory.  Depthwise arithmetic (mul, add, tap order) is that of dwconv3x3_kernel.
struct RetinaStemW { const float* wa; const float* bias; float slope; };   // wa: [7][64] lane table, bias[8]

template <bool SPLIT>
__global__ void __launch_bounds__(256) retina_stem_kernel(const uint8_t* __restrict__ frames, int n, int H, int W, int Ho, int Wo,
                                                           RetinaStemW w, float* __restrict__ y) {
  // (tried and slower: four tiles in flight per wave, 0.15 ms per 8 frames; rows staged as aligned dwords in a
  // wave-private LDS strip, 0.19 ms; this form: 0.13 ms against 0.46 ms for the staging pass + plan convolution)
  const int lane = threadIdx.x & 63, lg = lane >> 4, lm = lane & 15;
  float wa[7];
#pragma unroll
  for (int s = 0; s < 7; ++s) wa[s] = w.wa[s * 64 + lane];
  float b4[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) b4[e] = lg < 2 ? w.bias[lg * 4 + e] : 0.f;
  const int tiles_w = (Wo + 15) >> 4;
  const long long ntile = (long long)n * Ho * tiles_w;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = (gridDim.x * blockDim.x) >> 6;
  for (long long t = wave; t < ntile; t += nwave) {
    const int tw = (int)(t % tiles_w);
    const long long q = t / tiles_w;
    const int ho = (int)(q % Ho), img = (int)(q / Ho);
    const int wo = tw * 16 + lm;
    const uint8_t* fb = frames + (size_t)img * H * W * 3;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      const int k = 4 * s + lg, tap = k / 3, c = k - tap * 3, kh = tap / 3, kw = tap - kh * 3;
      const int hi = 2 * ho - 1 + kh, wi = 2 * wo - 1 + kw;
      // clamped address + select on the value: the seven byte loads issue back to back (a predicated load is a branch
      // and a wait per tap)
      const bool ok = k < 27 && (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
      const int hc = min(max(hi, 0), H - 1), wc = min(max(wi, 0), W - 1), cc = min(c, 2);
      const float raw = (float)fb[((size_t)hc * W + wc) * 3 + cc] - (cc == 0 ? 104.f : (cc == 1 ? 117.f : 123.f));
      const float v = ok ? raw : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], v, acc, 0, 0, 0);
    }
    if (lg < 2 && wo < Wo) {
      f32x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = acc[e] + b4[e];
        o[e] = stv<SPLIT>(v > 0.f ? v : v * w.slope);
      }
      *reinterpret_cast<f32x4_t*>(y + (((size_t)img * Ho + ho) * Wo + wo) * 8 + lg * 4) = o;
    }
  }
}

hipError_t launch_retina_stem(const uint8_t* frames, int n, int H, int W, const float* wa, const float* bias, float slope, float* y,
                              bool split, hipStream_t s) {
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const long long ntile = (long long)n * Ho * ((Wo + 15) / 16);
  if (ntile == 0) return hipSuccess;
  const int blocks = (int)std::min<long long>((ntile + 3) / 4, 8192);
  if (split) hipLaunchKernelGGL(retina_stem_kernel<true>, dim3(blocks), dim3(256), 0, s, frames, n, H, W, Ho, Wo, RetinaStemW{wa, bias, slope}, y);
  else hipLaunchKernelGGL(retina_stem_kernel<false>, dim3(blocks), dim3(256), 0, s, frames, n, H, W, Ho, Wo, RetinaStemW{wa, bias, slope}, y);
  return hipGetLastError();
}

struct DwPwW { const float *dw, *dbias, *pw, *pbias; float dslope, pslope; };   // dw [9][CIN], pw [COUT][CIN] (BN folded)

template <int CIN, int COUT, bool SPLIT>
__global__ void __launch_bounds__(256) dwpw_kernel(const float* __restrict__ x, int n, int H, int W, int stride, int Ho, int Wo, DwPwW w,
                                                    float* __restrict__ y) {
  // lane group g owns the CONTIGUOUS channels [g*KS, g*KS + KS): k-step s of the pointwise GEMM pairs channel g*KS + s of
  // every group (any consistent k permutation is a valid dot product), and a lane's depthwise inputs are vector loads
  constexpr int KS = CIN / 4, NT = COUT / 16, VL = KS < 4 ? KS : 4, NV = KS / VL;
  typedef float vec_t __attribute__((ext_vector_type(VL)));
  const int lane = threadIdx.x & 63, lg = lane >> 4, lm = lane & 15;
  float wd[9][KS], bd[KS], wp[NT][KS], bp[NT][4];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    bd[s] = w.dbias[lg * KS + s];
#pragma unroll
    for (int t = 0; t < 9; ++t) wd[t][s] = w.dw[t * CIN + lg * KS + s];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wp[nt][s] = w.pw[(size_t)(16 * nt + lm) * CIN + lg * KS + s];
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int e = 0; e < 4; ++e) bp[nt][e] = w.pbias[16 * nt + 4 * lg + e];
  const int tiles_w = (Wo + 15) >> 4;
  const long long ntile = (long long)n * Ho * tiles_w;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = (gridDim.x * blockDim.x) >> 6;
  for (long long t = wave; t < ntile; t += nwave) {
    const int tw = (int)(t % tiles_w);
    const long long q = t / tiles_w;
    const int ho = (int)(q % Ho), img = (int)(q / Ho);
    const int wo = min(tw * 16 + lm, Wo - 1);          // tail lanes recompute the last pixel and do not store
    const float* xb = x + (size_t)img * H * W * CIN + lg * KS;
    // all 9 x NV loads first (clamped addresses, no predicate), then the arithmetic in dwconv3x3_kernel's order
    vec_t in[9][NV];
    bool ok[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int hi = ho * stride - 1 + kh, wi = wo * stride - 1 + kw;
        ok[kh * 3 + kw] = (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
        const float* px = xb + ((size_t)min(max(hi, 0), H - 1) * W + min(max(wi, 0), W - 1)) * CIN;
#pragma unroll
        for (int v = 0; v < NV; ++v) in[kh * 3 + kw][v] = *reinterpret_cast<const vec_t*>(px + v * VL);
      }
    float d[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) d[s] = 0.f;
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float xv = ldv<SPLIT>(in[tp][s / VL][s % VL]);
        d[s] = ok[tp] ? d[s] + xv * wd[tp][s] : d[s];
      }
    f32x4_t acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      float v = d[s] + bd[s];
      v = v > 0.f ? v : v * w.dslope;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[nt][s], v, acc[nt], 0, 0, 0);
    }
    if (tw * 16 + lm < Wo) {
      float* o = y + (((size_t)img * Ho + ho) * Wo + wo) * COUT + 4 * lg;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4_t r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[nt][e] + bp[nt][e];
          r[e] = stv<SPLIT>(v > 0.f ? v : v * w.pslope);
        }
        *reinterpret_cast<f32x4_t*>(o + 16 * nt) = r;
      }
    }
  }
}

bool dwpw_supported(int cin, int cout) {
  return (cin == 8 && cout == 16) || (cin == 16 && cout == 32) || (cin == 32 && cout == 32) || (cin == 32 && cout == 64);
}

hipError_t launch_dwpw(const float* x, float* y, int n, int H, int W, int cin, int cout, int stride, const float* dw, const float* dbias,
                       float dslope, const float* pw, const float* pbias, float pslope, bool split, hipStream_t s) {
  const int Ho = stride == 2 ? (H - 1) / 2 + 1 : H, Wo = stride == 2 ? (W - 1) / 2 + 1 : W;
  const long long ntile = (long long)n * Ho * ((Wo + 15) / 16);
  if (ntile == 0) return hipSuccess;
  const int blocks = (int)std::min<long long>((ntile + 3) / 4, 8192);
  const DwPwW w{dw, dbias, pw, pbias, dslope, pslope};
#define VNF_DWPW(CI, CO)                                                                                                    \
  do {                                                                                                                      \
    if (split) hipLaunchKernelGGL((dwpw_kernel<CI, CO, true>), dim3(blocks), dim3(256), 0, s, x, n, H, W, stride, Ho, Wo, w, y); \
    else hipLaunchKernelGGL((dwpw_kernel<CI, CO, false>), dim3(blocks), dim3(256), 0, s, x, n, H, W, stride, Ho, Wo, w, y);      \
  } while (0)
  if (cin == 8 && cout == 16) VNF_DWPW(8, 16);
  else if (cin == 16 && cout == 32) VNF_DWPW(16, 32);
  else if (cin == 32 && cout == 32) VNF_DWPW(32, 32);
  else if (cin == 32 && cout == 64) VNF_DWPW(32, 64);
  else return hipErrorInvalidValue;
#undef VNF_DWPW
  return hipGetLastError();
}

template <bool SPLIT>
__global__ void upsample_add_kernel(const float* __restrict__ x, int Hs, int Ws, float* __restrict__ y, int H, int W, int C,
                                    int n, float sh, float sw) {
  const int c4 = C >> 2;
  const size_t total = (size_t)n * H * W * c4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4) * 4;
    const size_t p = i / c4;
    const int w = (int)(p % W);
    const size_t q = p / W;
    const int h = (int)(q % H);
    const size_t img = q / H;
    // ATen nearest: min(floor(dst * scale), in - 1) with scale = (float)in / out
    const int hs = min((int)floorf((float)h * sh), Hs - 1), ws = min((int)floorf((float)w * sw), Ws - 1);
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(y + p * C + c);
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(x + ((img * Hs + hs) * Ws + ws) * C + c);
    f32x4_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = stv<SPLIT>(ldv<SPLIT>(a[e]) + ldv<SPLIT>(b[e]));
    *reinterpret_cast<f32x4_t*>(y + p * C + c) = o;
  }
}

hipError_t launch_upsample_add(const float* x, int Hs, int Ws, float* y, int H, int W, int C, int n, bool split, hipStream_t s) {
  if (C % 4) return hipErrorInvalidValue;
  const size_t total = (size_t)n * H * W * (C / 4);
  if (total == 0) return hipSuccess;
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  if (split)
    hipLaunchKernelGGL(upsample_add_kernel<true>, dim3(blocks), dim3(256), 0, s, x, Hs, Ws, y, H, W, C, n, (float)Hs / (float)H,
                       (float)Ws / (float)W);
  else
    hipLaunchKernelGGL(upsample_add_kernel<false>, dim3(blocks), dim3(256), 0, s, x, Hs, Ws, y, H, W, C, n, (float)Hs / (float)H,
                       (float)Ws / (float)W);
  return hipGetLastError();
}

// ---------------------------------------------------------------- NHWC slice -> NCHW fp32 (taps)
// one thread per (image, storage unit, pixel), pixels fastest: N coalesced fp32 rows out
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ x, int ldx, float* __restrict__ y, int n, int HW, int C) {
  constexpr int N = Unit<T>::N;
  const int cc = C / N;
  const size_t total = (size_t)n * cc * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int p = (int)(i % HW);
    const size_t q = i / HW;
    const int c = (int)(q % cc) * N;
    const size_t img = q / cc;
    float v[N];
    Unit<T>::load(x + (img * HW + p) * (size_t)ldx + c, v);
#pragma unroll
    for (int e = 0; e < N; ++e) y[(img * C + c + e) * HW + p] = v[e];
  }
}

template <typename T>
static hipError_t nhwc_to_nchw_go(const void* x, int ldx, float* y, int n, int HW, int C, hipStream_t s) {
  const size_t total = (size_t)n * (C / Unit<T>::N) * HW;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)x, ldx, y, n, HW, C);
  return hipGetLastError();
}

hipError_t launch_nhwc_to_nchw_f32(const void* x, int ldx, int dtype, float* y, int n, int HW, int C, hipStream_t s) {
  const int ch = dtype_chan_align(dtype);
  if (C % ch || ldx % ch) return hipErrorInvalidValue;   // slices start and end on a unit boundary
  if ((size_t)n * HW * C == 0) return hipSuccess;
  switch (dtype) {
    case BF16: return nhwc_to_nchw_go<__bf16>(x, ldx, y, n, HW, C, s);
    case F16: return nhwc_to_nchw_go<_Float16>(x, ldx, y, n, HW, C, s);
    case F32: return nhwc_to_nchw_go<float>(x, ldx, y, n, HW, C, s);
    case F16P: return nhwc_to_nchw_go<pf16>(x, ldx, y, n, HW, C, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace vnf
