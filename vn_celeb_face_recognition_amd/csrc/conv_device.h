// Device-side building blocks shared by the implicit-GEMM convolution kernels (conv_igemm.hip: LDS-DMA ring kernel;
// conv_patch.hip: LDS-resident input patch kernel; conv_ws.hip: wave-specialised kernel and its persistent form): the MFMA
// wrappers per storage layout, the consumer K loop (conv_k_loop), the loaders' pixel-row set-up, the LDS-staged epilogue
// and the register epilogue's swap-and-store (also under the stem_conv1a kernels of aux_kernels.hip).
#pragma once
#include <atomic>
#include <type_traits>

#include "kernels.h"
#include "split_f16.h"

namespace vnf {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct KArgs {  // device-side copy of ConvArgs (POD)
  const char* x;
  const char* w;
  const float* bias;
  const int4* ktab;
  const char* res;
  const float* slope;
  const char* zero;  // >= 16 zero bytes
  int ldx, H, W, Ho, Wo, sh, sw, ph, pw;
  int K, Kpad, nkt;
  int wrs, wts;  // weight image strides in bytes: between output channels, between K tiles
  int ncls, cout_pad;
  int M, Cout, tiles_n, nblk;
  int ldres, act, out_f32;
  int nseg;
  int seg_c0[4], seg_c1[4], seg_ld[4];
  char* seg_ptr[4];
  // patch kernel (conv_patch.hip) geometry: taps, channels per tap, LDS pixel pitch in 16-byte
  // slots, padded row width, virtual (vertically padded) image height, patch bytes
  int KH, KW, Cin, pp, Wp, Hv, patch_bytes;
  int lds_bytes;  // patch kernel: dynamic LDS of the launch (what the epilogue may stage into)
  long long* dbg;  // in-kernel stamp buffer of the instrumented build (tools), else null
};

// Host side, in front of every launch that asks for more dynamic LDS than the default: opt `Kernel` in to `bytes`, once
// per (kernel instantiation, device).  Steady state: hipGetDevice and one atomic load, no lock; threads that race to be
// first on a device each set the attribute, which is harmless.  The attribute is advisory on this ROCm, so its status is
// dropped and the sticky error cleared: the launch error is what the callers check.
template <auto Kernel>
inline void allow_dynamic_lds(int bytes) {
  static std::atomic<unsigned> done{0};   // bit d: set on device d
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned bit = (unsigned)dev < 16 ? 1u << dev : 0;   // past 16 devices: set on every launch
  if (done.load(std::memory_order_acquire) & bit) return;
  (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  (void)hipGetLastError();
  done.fetch_or(bit, std::memory_order_release);
}

// the fused kernels: opt in to the launch's own dynamic LDS, launch, return the launch status
template <auto Kernel, class Args>
inline hipError_t launch_with_lds(dim3 grid, int block, int lds, hipStream_t s, const Args& a) {
  allow_dynamic_lds<Kernel>(lds);
  hipLaunchKernelGGL(Kernel, grid, dim3(block), lds, s, a);
  return hipGetLastError();
}
template <auto Kernel, class Args>
inline hipError_t launch_with_lds(int grid, int block, int lds, hipStream_t s, const Args& a) {
  return launch_with_lds<Kernel>(dim3(grid), block, lds, s, a);
}

template <typename T>
__device__ __forceinline__ void mma_chunk(f32x4_t& acc, const uint4& wf, const uint4& xf);

template <>
__device__ __forceinline__ void mma_chunk<__bf16>(f32x4_t& acc, const uint4& wf, const uint4& xf) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf), __builtin_bit_cast(bf16x8_t, xf),
                                                acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma_chunk<_Float16>(f32x4_t& acc, const uint4& wf, const uint4& xf) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, wf), __builtin_bit_cast(f16x8_t, xf),
                                               acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma_chunk<float>(f32x4_t& acc, const uint4& wf, const uint4& xf) {
  // lane group g holds k = 4g..4g+3 of this 16-deep block; MFMA j consumes element j of every
  // group, i.e. the k set {4g+j}.  Any consistent k permutation is a valid dot product.
  f32x4_t w4 = __builtin_bit_cast(f32x4_t, wf), x4 = __builtin_bit_cast(f32x4_t, xf);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[0], x4[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[1], x4[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[2], x4[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[3], x4[3], acc, 0, 0, 0);
}

template <>
__device__ __forceinline__ void mma_chunk<sf16>(f32x4_t& acc, const uint4& wf, const uint4& xf) {
  // each operand chunk is 4 k values as (hi, lo) halves: slots [h0 l0 h1 l1 h2 l2 h3 l3].  The first MFMA pairs
  // equal slots (sum hi*hi' + lo*lo'), the second pairs the weight chunk with the activation chunk's halves
  // swapped inside every dword (sum hi*lo' + lo*hi'): together the full product of the two split values.
  const uint4 xr = {(xf.x >> 16) | (xf.x << 16), (xf.y >> 16) | (xf.y << 16), (xf.z >> 16) | (xf.z << 16),
                    (xf.w >> 16) | (xf.w << 16)};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, wf), __builtin_bit_cast(f16x8_t, xf),
                                               acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, wf), __builtin_bit_cast(f16x8_t, xr),
                                               acc, 0, 0, 0);
}

// ---- planar split-f16 (pf16, split_f16.h): one K tile in LDS = [hi chunk of unit 0..3 | lo chunk of unit 0..3], so the
// fragment reads of "half" 0 / 1 of a K tile (chunk ks*4 + fgrp) return the hi / lo plane of the lane group's 8 k values
template <typename T> struct is_planar { static constexpr bool value = false; };
template <> struct is_planar<pf16> { static constexpr bool value = true; };

// channel (k) index of logical 16-byte chunk `lchunk` (0..7) inside a K tile, and the chunk's extra byte offset
// inside its 8-channel unit (planar: chunks 4..7 are the lo planes of units 0..3)
template <typename T> __device__ __forceinline__ int chunk_chan(int lchunk) {
  if constexpr (is_planar<T>::value) return (lchunk & 3) * 8;
  else return lchunk * (16 / (int)sizeof(T));
}
template <typename T> __device__ __forceinline__ int chunk_byte(int lchunk) {
  if constexpr (is_planar<T>::value) return (lchunk >> 2) * 16;
  else return 0;
}

__device__ __forceinline__ f32x4_t mfma_f16(const uint4& a, const uint4& b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
// planar split product of one K tile for one (weight tile, pixel tile): hi.hi' first, then the two cross terms
__device__ __forceinline__ void mma_hh(f32x4_t& acc, const uint4& wh, const uint4& xh) { acc = mfma_f16(wh, xh, acc); }
__device__ __forceinline__ void mma_cross(f32x4_t& acc, const uint4& wh, const uint4& wl, const uint4& xh, const uint4& xl) {
  acc = mfma_f16(wh, xl, acc);
  acc = mfma_f16(wl, xh, acc);
}
template <>
__device__ __forceinline__ void mma_chunk<pf16>(f32x4_t&, const uint4&, const uint4&) {}  // planar tiles go through mma_hh / mma_cross

template <typename T>
__device__ __forceinline__ void load8(const char* p, float (&v)[8]);
template <>
__device__ __forceinline__ void load8<__bf16>(const char* p, float (&v)[8]) {
  bf16x8_t r = *reinterpret_cast<const bf16x8_t*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)r[i];
}
template <>
__device__ __forceinline__ void load8<_Float16>(const char* p, float (&v)[8]) {
  f16x8_t r = *reinterpret_cast<const f16x8_t*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)r[i];
}
template <>
__device__ __forceinline__ void load8<float>(const char* p, float (&v)[8]) {
  f32x4_t a = *reinterpret_cast<const f32x4_t*>(p), b = *reinterpret_cast<const f32x4_t*>(p + 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
}

template <>
__device__ __forceinline__ void load8<sf16>(const char* p, float (&v)[8]) {
  f16x8_t a = *reinterpret_cast<const f16x8_t*>(p), b = *reinterpret_cast<const f16x8_t*>(p + 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = (float)a[2 * i] + (float)a[2 * i + 1];
    v[4 + i] = (float)b[2 * i] + (float)b[2 * i + 1];
  }
}

template <>
__device__ __forceinline__ void load8<pf16>(const char* p, float (&v)[8]) {
  f16x8_t h = *reinterpret_cast<const f16x8_t*>(p), l = *reinterpret_cast<const f16x8_t*>(p + 16);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)h[i] + (float)l[i];
}

template <typename T>
__device__ __forceinline__ void store8(char* p, const float (&v)[8]);
template <>
__device__ __forceinline__ void store8<__bf16>(char* p, const float (&v)[8]) {
  bf16x8_t r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = (__bf16)v[i];
  *reinterpret_cast<bf16x8_t*>(p) = r;
}
template <>
__device__ __forceinline__ void store8<_Float16>(char* p, const float (&v)[8]) {
  f16x8_t r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = (_Float16)v[i];
  *reinterpret_cast<f16x8_t*>(p) = r;
}
template <>
__device__ __forceinline__ void store8<float>(char* p, const float (&v)[8]) {
  f32x4_t a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
  *reinterpret_cast<f32x4_t*>(p) = a;
  *reinterpret_cast<f32x4_t*>(p + 16) = b;
}

template <>
__device__ __forceinline__ void store8<sf16>(char* p, const float (&v)[8]) {
  f16x8_t a, b;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const sf16 s0(v[i]), s1(v[4 + i]);
    a[2 * i] = s0.hi; a[2 * i + 1] = s0.lo;
    b[2 * i] = s1.hi; b[2 * i + 1] = s1.lo;
  }
  *reinterpret_cast<f16x8_t*>(p) = a;
  *reinterpret_cast<f16x8_t*>(p + 16) = b;
}

template <>
__device__ __forceinline__ void store8<pf16>(char* p, const float (&v)[8]) {
  f16x8_t h, l;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const sf16 s(v[i]);
    h[i] = s.hi; l[i] = s.lo;
  }
  *reinterpret_cast<f16x8_t*>(p) = h;
  *reinterpret_cast<f16x8_t*>(p + 16) = l;
}

// XCD-aware, bijective block -> tile map: blocks that share an XCD (same blockIdx % 8) walk
// consecutive tiles, so the BN-column siblings of one pixel tile hit the same L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// ---- epilogue shared by the conv kernels: fp32 accumulators -> LDS -> whole NHWC rows ------------
// Fast form (the stem / reduction convolutions of the 2-byte plans: bias + ReLU / PReLU, no residual, no border-class bias,
// output in T): bias and activation are applied in the accumulator layout, the tile is staged ALREADY ROUNDED to T --
// half the LDS bytes, so the whole tile fits one pass and one barrier -- and every global load (the bias) is issued
// before the first store: vmcnt counts loads and stores together in issue order, so a load behind a store waits for
// the store's acknowledgement (the staged fp32 form paid that once per pass: conv2d_4a's epilogue was 17 k of its
// workgroups' 59 k cycles, in-kernel stamps).  Same fp32 sum, bias add, max and rounding as the general form, so the
// results are bit-identical to it.
template <typename T, int BM, int BN>
__device__ __forceinline__ bool conv_epilogue_is_fast(const KArgs& a, int avail) {
  if constexpr (sizeof(T) != 2)
    return false;
  else
    return !a.res && a.ncls == 1 && !a.out_f32 && BM * (BN * 2 + 16) <= avail;
}

template <typename T, int BM, int BN, int WM, int WN, int LDS_BYTES>
__device__ __forceinline__ void conv_epilogue(const KArgs& a, f32x4_t (&acc)[BM / WM / 16][BN / WN / 16], char* smem,
                                              int m0, int n0, int avail = LDS_BYTES) {
  static_assert(BM % (WM * 16) == 0 && BN % (WN * 16) == 0, "wave tiles are whole 16x16 MFMA tiles");
  constexpr int ES = (int)sizeof(T);
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int NT = WM * WN * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN, frow = lane & 15, fgrp = lane >> 4;
  const int HoWo = a.Ho * a.Wo;
  if constexpr (sizeof(T) == 2) {
    if (conv_epilogue_is_fast<T, BM, BN>(a, avail)) {
      constexpr int PITCH = BN * 2 + 16;  // +16 B: the 16 rows of one ds_write_b64 land on different banks
      typedef T tx4 __attribute__((ext_vector_type(4)));
      f32x4_t bias[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int c = n0 + wn * WTN + j * 16 + fgrp * 4;
        bias[j] = c < a.Cout ? *reinterpret_cast<const f32x4_t*>(a.bias + c) : f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
      const bool relu = a.act == ACT_RELU, prelu = a.act == ACT_PRELU;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        f32x4_t slope = {0.f, 0.f, 0.f, 0.f};
        if (prelu) {
          const int c = n0 + wn * WTN + j * 16 + fgrp * 4;
          if (c < a.Cout) slope = *reinterpret_cast<const f32x4_t*>(a.slope + c);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          tx4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = acc[i][j][e] + bias[j][e];
            if (relu) v = fmaxf(v, 0.f);
            if (prelu) v = v > 0.f ? v : v * slope[e];
            o[e] = (T)v;
          }
          *reinterpret_cast<tx4*>(smem + (wm * WTM + i * 16 + frow) * PITCH + (wn * WTN + j * 16 + fgrp * 4) * 2) = o;
        }
      }
      __syncthreads();
      constexpr int CPR8 = BN / 8;
      for (int idx = tid; idx < BM * CPR8; idx += NT) {
        const int r = idx / CPR8, cc = idx - r * CPR8;
        const int m = m0 + r, c = n0 + cc * 8;
        if (m < a.M && c < a.Cout) {
          int sg = 0;
#pragma unroll
          for (int s = 1; s < 4; ++s)
            if (s < a.nseg && c >= a.seg_c0[s]) sg = s;
          *reinterpret_cast<uint4*>(a.seg_ptr[sg] + ((size_t)m * a.seg_ld[sg] + (c - a.seg_c0[sg])) * 2) =
              *reinterpret_cast<const uint4*>(smem + r * PITCH + cc * 16);
        }
      }
      return;
    }
  }
  float* sC = reinterpret_cast<float*>(smem);
  constexpr int CST = BN + 4;  // floats per staged row (+16 B pad: conflict-free float4 writes)
  constexpr int CPR = BN / 8;  // 8-channel chunks per row
  // as many wave rows per pass as the staging LDS holds
  constexpr int EPASS = (BM * CST * 4 <= LDS_BYTES) ? 1 : WM;
  constexpr int RPP = BM / EPASS;
  static_assert(RPP * CST * 4 <= LDS_BYTES, "epilogue staging does not fit");
  // Thread map of the store phase.  When the chunk count per row divides the thread count every
  // thread owns ONE 8-channel column chunk (bias loaded once, residual loads hoisted above the
  // barrier); tiles whose width is not a power of two (96, 192 channels) use the general map.
  constexpr bool FIXEDCOL = (NT % CPR == 0) && ((RPP * CPR) % NT == 0);
  constexpr int NIT = (RPP * CPR + NT - 1) / NT, RSTEP = NT / CPR;
  if constexpr (FIXEDCOL) {
    const int cc = tid % CPR, r0 = tid / CPR;
    const int c = n0 + cc * 8;
    const bool cok = c < a.Cout;
    const int cl = cok ? c : 0;  // in-range column for the loads of masked threads
    // destination tensor of this thread's 8-channel chunk (segment boundaries are multiples of 8, so a
    // tile may span several destinations: concat-free routing happens per chunk, not per tile)
    int sg = 0;
#pragma unroll
    for (int s = 1; s < 4; ++s)
      if (s < a.nseg && c >= a.seg_c0[s]) sg = s;
    char* const dptr = a.seg_ptr[sg];
    const int dld = a.seg_ld[sg], dc0 = a.seg_c0[sg];
    f32x4_t b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
    float slope[8];
    if (a.ncls == 1) {
      b0 = *reinterpret_cast<const f32x4_t*>(a.bias + cl);
      b1 = *reinterpret_cast<const f32x4_t*>(a.bias + cl + 4);
    }
    if (a.act == ACT_PRELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) slope[e] = a.slope[cl + e];
    }
    for (int pass = 0; pass < EPASS; ++pass) {
      float rv[NIT][8];
      if (a.res) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const int m = min(m0 + pass * RPP + r0 + it * RSTEP, a.M - 1);
          load8<T>(a.res + ((size_t)m * a.ldres + cl) * ES, rv[it]);
        }
      }
      if ((wm * WTM) / RPP == pass) {
        const int rbase = wm * WTM - pass * RPP;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            *reinterpret_cast<f32x4_t*>(sC + (rbase + i * 16 + frow) * CST + wn * WTN + j * 16 + fgrp * 4) = acc[i][j];
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int r = r0 + it * RSTEP;
        const int m = m0 + pass * RPP + r;
        float v[8];
        const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(sC + r * CST + cc * 8);
        const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(sC + r * CST + cc * 8 + 4);
        if (a.ncls == 9) {
          const int mm = min(m, a.M - 1);
          const int rr = mm % HoWo, ho = rr / a.Wo, wo = rr - ho * a.Wo;
          const int cls = (ho == 0 ? 0 : (ho == a.Ho - 1 ? 2 : 1)) * 3 + (wo == 0 ? 0 : (wo == a.Wo - 1 ? 2 : 1));
          const float* bp = a.bias + (size_t)cls * a.cout_pad + cl;
          b0 = *reinterpret_cast<const f32x4_t*>(bp);
          b1 = *reinterpret_cast<const f32x4_t*>(bp + 4);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = v0[e] + b0[e]; v[4 + e] = v1[e] + b1[e]; }
        if (a.res) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += rv[it][e];
        }
        if (a.act == ACT_RELU) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
        } else if (a.act == ACT_PRELU) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * slope[e];
        }
        if (m < a.M && cok) {
          if (a.out_f32)
            store8<float>(dptr + ((size_t)m * dld + (c - dc0)) * 4, v);
          else
            store8<T>(dptr + ((size_t)m * dld + (c - dc0)) * ES, v);
        }
      }
      __syncthreads();
    }
  } else {
    for (int pass = 0; pass < EPASS; ++pass) {
      if ((wm * WTM) / RPP == pass) {
        const int rbase = wm * WTM - pass * RPP;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            *reinterpret_cast<f32x4_t*>(sC + (rbase + i * 16 + frow) * CST + wn * WTN + j * 16 + fgrp * 4) = acc[i][j];
      }
      __syncthreads();
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int idx = tid + it * NT;
        const int r = idx / CPR, cc = idx - r * CPR;
        const int m = m0 + pass * RPP + r, c = n0 + cc * 8;
        if (idx < RPP * CPR && m < a.M && c < a.Cout) {
          int sg = 0;
#pragma unroll
          for (int s = 1; s < 4; ++s)
            if (s < a.nseg && c >= a.seg_c0[s]) sg = s;
          float v[8];
          const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(sC + r * CST + cc * 8);
          const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(sC + r * CST + cc * 8 + 4);
          int cls = 0;
          if (a.ncls == 9) {
            const int rr = m % HoWo, ho = rr / a.Wo, wo = rr - ho * a.Wo;
            cls = (ho == 0 ? 0 : (ho == a.Ho - 1 ? 2 : 1)) * 3 + (wo == 0 ? 0 : (wo == a.Wo - 1 ? 2 : 1));
          }
          const float* bp = a.bias + (size_t)cls * a.cout_pad + c;
          const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(bp), b1 = *reinterpret_cast<const f32x4_t*>(bp + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { v[e] = v0[e] + b0[e]; v[4 + e] = v1[e] + b1[e]; }
          if (a.res) {
            float rv[8];
            load8<T>(a.res + ((size_t)m * a.ldres + c) * ES, rv);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += rv[e];
          }
          if (a.act == ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
          } else if (a.act == ACT_PRELU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * a.slope[c + e];
          }
          char* const dptr = a.seg_ptr[sg];
          if (a.out_f32)
            store8<float>(dptr + ((size_t)m * a.seg_ld[sg] + (c - a.seg_c0[sg])) * 4, v);
          else
            store8<T>(dptr + ((size_t)m * a.seg_ld[sg] + (c - a.seg_c0[sg])) * ES, v);
        }
      }
      __syncthreads();
    }
  }
}

// One LDS-DMA piece: 64 lanes x 16 B -> lds_base + lane*16.  M0 carries the LDS base; it is
// compiler-reserved, so it is saved and restored inside the statement (cdna guide 5.7).
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_base)
      : "memory");
}

// Retire this wave's older DMA pieces (all but the N youngest), drain its own LDS reads of the
// stage about to be recycled, then meet the other waves.  One statement, so the compiler cannot
// move LDS accesses between the wait and the barrier.
template <int N>
__device__ __forceinline__ void wait_dma_and_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// ---- loader side: per-thread pixel-row bookkeeping of the im2col gather.  This thread's row p of the A tile is pixel
// m0 + row0 + RS * p (ring kernel: row0 = tid >> 3, RS rows per DMA pass of the workgroup; loader waves of conv_ws.hip:
// row0 = 8 * loader wave + lane >> 3, RS = 8 * loader waves).  Rows past M read the zero page (ahi far outside the image).
// EARLY: the geometry is read once, in front of the rows.  Read inside the `m < M` branch, as the ring kernel has it,
// every row fetches its kernel arguments again and waits for them; in the loader waves of conv_ws.hip that wait sits on
// the way to the first DMA of the workgroup (persistent form: of every tile) and cost 1.2 - 1.5 % of a launch, while the
// ring kernel's sf16 128x32 tiles lose an occupancy step when it is hoisted (profiles/conv_core_ab.txt).
struct RowGeom { int M, H, W, Wo, HoWo, ldx, sh, sw, ph, pw; };
template <int AP, int RS, bool EARLY = false>
__device__ __forceinline__ void row_setup(const KArgs& a, int m0, int row0, int (&abase)[AP], int (&ahi)[AP],
                                          int (&awi)[AP]) {
  auto geom = [&]() { return RowGeom{a.M, a.H, a.W, a.Wo, a.Ho * a.Wo, a.ldx, a.sh, a.sw, a.ph, a.pw}; };
  const int HoWo = a.Ho * a.Wo;
  RowGeom early = {};
  if constexpr (EARLY) early = geom();
#pragma unroll
  for (int p = 0; p < AP; ++p) {
    const int m = m0 + row0 + RS * p;
    if (m < (EARLY ? early.M : a.M)) {
      RowGeom g = early;
      if constexpr (!EARLY) { g = geom(); g.HoWo = HoWo; }
      const int n = m / g.HoWo, r = m - n * g.HoWo;
      const int ho = r / g.Wo, wo = r - ho * g.Wo;
      ahi[p] = ho * g.sh - g.ph;
      awi[p] = wo * g.sw - g.pw;
      abase[p] = ((n * g.H + ahi[p]) * g.W + awi[p]) * g.ldx;
    } else {
      ahi[p] = -(1 << 24);
      awi[p] = 0;
      abase[p] = 0;
    }
  }
}

// ---- consumer side: the K loop of every conv kernel --------------------------------------------------------------
// Fragments of half ks of a K tile from a swizzled [row][128 B] LDS image (physical 16-byte slot p of row r holds logical
// k-chunk p ^ (r & 7)): TR MFMA tiles of 16 rows from row0 on, lane (frow, fgrp) reading chunk ks * 4 + fgrp of its row.
template <int TR>
__device__ __forceinline__ void read_rows(const char* img, int row0, int frow, int fgrp, int ks, uint4 (&f)[TR]) {
#pragma unroll
  for (int i = 0; i < TR; ++i) {
    const int row = row0 + i * 16 + frow;
    f[i] = *reinterpret_cast<const uint4*>(img + row * 128 + (((ks * 4 + fgrp) ^ (row & 7)) << 4));
  }
}

// The loop over the nkt K tiles of one output tile: acc = the sums over K.
//   join(kt) makes K tile kt readable -- barrier, counted wait, issue of tile kt + S - 1, stamps: whatever the kernel's
//     ring needs;
//   rd(kt, ks, x, w) reads the pixel (x) and weight (w) fragments of its half ks;
//   ahead(kt), if given, runs behind the last fragment read of tile kt: what the kernel does for tile kt + 1 under the
//     MFMAs (the patch kernel's table look-up, the persistent kernel's stage advance).
// The MFMA takes the WEIGHT fragment as the A operand and the PIXEL fragment as B, so an accumulator quad holds 4
// consecutive output channels of one pixel.
//   2-byte and f32 layouts, PIPE: software-pipelined over half K tiles, the fragment reads of one half in flight under
//     the MFMAs of the previous half (also across the join), so a wave never idles on LDS latency even at one or two
//     waves per SIMD.  The second half of the last tile is K padding when K - kt * BKE <= BKE / 2 and is skipped.
//   planar split-f16: half 0 / 1 of a K tile is the hi / lo plane of the same 32 k values.  Per tile hi.hi' (needs the hi
//     fragments only) and the two cross terms; with PIPE the cross terms of tile kt - 1 run under the hi reads of tile kt,
//     so the hi fragments are double-buffered (static indices: the loop is unrolled by two).
//   !PIPE keeps ONE fragment set (wave tiles whose accumulators leave no room for two): read, multiply, read, multiply.
struct no_fetch_ahead { __device__ void operator()(int) const {} };
template <typename T, int TM, int TN, bool PIPE, class Join, class Rd, class Ahead = no_fetch_ahead>
__device__ __forceinline__ void conv_k_loop(int K, int nkt, f32x4_t (&acc)[TM][TN], Join&& join, Rd&& rd,
                                            Ahead&& ahead = Ahead{}) {
  constexpr int BKE = 128 / (int)sizeof(T);
  constexpr int NF = PIPE ? 2 : 1;
  // The sums are kept in a struct per MFMA tile and handed over at the end.  A bare f32x4_t[TM][TN] that is indexed here
  // directly is turned into ONE wide vector by the compiler (AMDGPU promote-alloca runs before the array is split), and
  // the small tiles then shuffle that vector in and out of the MFMA's registers at every K tile.  Nothing but the
  // generated code shows whether this still holds: after a compiler change, redo the per-instantiation table of
  // profiles/conv_core_ab.txt -- the 64x32 / 32x64 ring tiles must stay at 52 - 64 registers and occupancy 8.
  struct Sum { f32x4_t v; } c[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) c[i][j].v = f32x4_t{0.f, 0.f, 0.f, 0.f};
  if constexpr (is_planar<T>::value) {
    uint4 xh[NF][TM], wh[NF][TN], xl[TM], wl[TN];
    auto cross = [&](uint4 (&x)[TM], uint4 (&w)[TN]) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mma_cross(c[i][j].v, w[j], wl[j], x[i], xl[i]);
    };
    auto hh = [&](uint4 (&x)[TM], uint4 (&w)[TN]) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mma_hh(c[i][j].v, w[j], x[i]);
    };
    if constexpr (PIPE) {
      auto step = [&](auto P, int kt) {
        constexpr int b = decltype(P)::value;
        join(kt);
        rd(kt, 0, xh[b], wh[b]);
        if (kt > 0) cross(xh[b ^ 1], wh[b ^ 1]);
        rd(kt, 1, xl, wl);
        ahead(kt);
        hh(xh[b], wh[b]);
      };
      int kt = 0;
      for (; kt + 1 < nkt; kt += 2) {
        step(std::integral_constant<int, 0>{}, kt);
        step(std::integral_constant<int, 1>{}, kt + 1);
      }
      if (kt < nkt) {
        step(std::integral_constant<int, 0>{}, kt);
        cross(xh[0], wh[0]);
      } else {
        cross(xh[NF - 1], wh[NF - 1]);
      }
    } else {
      for (int kt = 0; kt < nkt; ++kt) {
        join(kt);
        rd(kt, 0, xh[0], wh[0]);
        rd(kt, 1, xl, wl);
        ahead(kt);
        hh(xh[0], wh[0]);
        cross(xh[0], wh[0]);
      }
    }
  } else {
    uint4 xf[NF][TM], wf[NF][TN];
    auto mma = [&](int ks) {
      const int fs = PIPE ? ks : 0;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mma_chunk<T>(c[i][j].v, wf[fs][j], xf[fs][i]);
    };
    bool pend = false;  // second half of the previous K tile read but not yet multiplied
    for (int kt = 0; kt < nkt; ++kt) {
      join(kt);
      if constexpr (PIPE) {
        rd(kt, 0, xf[0], wf[0]);
        if (pend) mma(1);
        pend = BKE / 2 < K - kt * BKE;
        if (pend) rd(kt, 1, xf[1], wf[1]);
        ahead(kt);
        mma(0);
      } else {
        rd(kt, 0, xf[0], wf[0]);
        mma(0);
        if (BKE / 2 < K - kt * BKE) {
          rd(kt, 1, xf[0], wf[0]);
          mma(1);
        }
        ahead(kt);
      }
    }
    if (pend) mma(1);
  }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = c[i][j].v;
}

// ---- register epilogue: swap and store -----------------------------------------------------------------------------
// A lane holds, of one pixel, channel quad fgrp of two neighbouring 16-channel MFMA tiles (v0: tile j, v1: tile j + 1).
// Rounded to T, the odd lane rows of tile j's quads are exchanged with the even lane rows of tile j + 1's
// (v_permlane16_swap): every lane then owns 8 consecutive channels, those of tile j + (fgrp & 1) from (fgrp >> 1) * 8
// on, one 16-byte store.  Every lane of the wave must call these (the swap is a cross-lane operation).
template <typename T>
__device__ __forceinline__ uint4 swap_quads(const f32x4_t& v0, const f32x4_t& v1) {
  static_assert(sizeof(T) == 2, "2-byte elements");
  typedef T tx4 __attribute__((ext_vector_type(4)));
  tx4 o0, o1;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o0[e] = (T)v0[e]; o1[e] = (T)v1[e]; }
  const uint2 p0 = __builtin_bit_cast(uint2, o0), p1 = __builtin_bit_cast(uint2, o1);
  const auto sx = __builtin_amdgcn_permlane16_swap(p0.x, p1.x, false, false);
  const auto sy = __builtin_amdgcn_permlane16_swap(p0.y, p1.y, false, false);
  return uint4{sx[0], sy[0], sx[1], sy[1]};
}
// planar split-f16: an 8-channel unit is [8 hi][8 lo], so the hi quads and the lo quads are exchanged separately
__device__ __forceinline__ void swap_quads_planar(const f32x4_t& v0, const f32x4_t& v1, uint4& hi, uint4& lo) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  h4 h0, l0, h1, l1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const sf16 s0(v0[e]), s1(v1[e]);
    h0[e] = s0.hi; l0[e] = s0.lo;
    h1[e] = s1.hi; l1[e] = s1.lo;
  }
  const uint2 ph0 = __builtin_bit_cast(uint2, h0), ph1 = __builtin_bit_cast(uint2, h1);
  const uint2 pl0 = __builtin_bit_cast(uint2, l0), pl1 = __builtin_bit_cast(uint2, l1);
  const auto hx = __builtin_amdgcn_permlane16_swap(ph0.x, ph1.x, false, false);
  const auto hy = __builtin_amdgcn_permlane16_swap(ph0.y, ph1.y, false, false);
  const auto lx = __builtin_amdgcn_permlane16_swap(pl0.x, pl1.x, false, false);
  const auto ly = __builtin_amdgcn_permlane16_swap(pl0.y, pl1.y, false, false);
  hi = uint4{hx[0], hy[0], hx[1], hy[1]};
  lo = uint4{lx[0], ly[0], lx[1], ly[1]};
}
// both forms behind one call: the swap in every lane, then this lane's 8-channel unit to d where ok
template <typename T>
__device__ __forceinline__ void swap_store(char* d, bool ok, const f32x4_t& v0, const f32x4_t& v1) {
  if constexpr (is_planar<T>::value) {
    uint4 hi, lo;
    swap_quads_planar(v0, v1, hi, lo);
    if (ok) {
      *reinterpret_cast<uint4*>(d) = hi;
      *reinterpret_cast<uint4*>(d + 16) = lo;
    }
  } else {
    const uint4 c = swap_quads<T>(v0, v1);
    if (ok) *reinterpret_cast<uint4*>(d) = c;
  }
}

// ---- conv_patch.hip (LDS-resident input patch kernel; tile configurations follow the ring kernel's ids)
// epilogue staging bytes of a patch configuration: the whole tile when it fits 64 KiB, else one wave row per pass
constexpr int patch_epi_bytes(int bm, int bn, int wm) {
  return bm * (bn + 4) * 4 <= 64 * 1024 ? bm * (bn + 4) * 4 : (bm / wm) * (bn + 4) * 4;
}
int patch_num_cfgs();
bool patch_cfg_ok(const ConvArgs& a, int pcfg);
bool patch_cfg_tile(int pcfg, ConvTile& t);
hipError_t launch_patch(const ConvArgs& a, const KArgs& k, int pcfg, hipStream_t s);

// ---- conv_ws.hip (wave-specialised big-tile kernel; configuration ids follow the patch kernel's)
int ws_num_cfgs();
bool ws_cfg_ok(const ConvArgs& a, int wcfg);
bool ws_cfg_tile(int wcfg, ConvTile& t);
hipError_t launch_ws(const ConvArgs& a, const KArgs& k, int wcfg, hipStream_t s);

}  // namespace vnf
