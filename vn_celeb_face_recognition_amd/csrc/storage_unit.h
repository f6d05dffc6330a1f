// Storage unit of an activation layout: the N consecutive channels a streaming kernel moves per thread -- one 16-byte
// chunk of float / __bf16 / _Float16 / sf16 values, or the 32-byte [8 hi][8 lo] unit of planar split-f16 (split_f16.h).
//   Raw                 the unit as loaded (what a kernel keeps while further loads are in flight)
//   raw(p)              one unit from memory
//   at(raw, e)          value e of it as fp32 (converted where it is used: N converted taps cost N registers each)
//   load(p, v)          all N values of the unit at p
//   store(p, v)         N fp32 values rounded to T (split-f16: re-split, which reproduces a recombined pair bit for bit)
#pragma once
#include <hip/hip_runtime.h>

#include "split_f16.h"

namespace vnf {

template <typename T>
struct Unit {
  static constexpr int N = 16 / (int)sizeof(T);
  struct alignas(16) Raw { T v[N]; };
  static __device__ __forceinline__ Raw raw(const T* p) {
    Raw r;
    *reinterpret_cast<uint4*>(r.v) = *reinterpret_cast<const uint4*>(p);
    return r;
  }
  static __device__ __forceinline__ float at(const Raw& r, int e) { return (float)r.v[e]; }
  static __device__ __forceinline__ void load(const T* p, float (&v)[N]) {
    const Raw r = raw(p);
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = at(r, e);
  }
  static __device__ __forceinline__ void store(T* p, const float (&v)[N]) {
    Raw r;
#pragma unroll
    for (int e = 0; e < N; ++e) r.v[e] = (T)v[e];
    *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(r.v);
  }
};

template <>
struct Unit<pf16> {
  static constexpr int N = 8;
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  struct Raw { h8 hi, lo; };
  static __device__ __forceinline__ Raw raw(const pf16* p) {
    return Raw{reinterpret_cast<const h8*>(p)[0], reinterpret_cast<const h8*>(p)[1]};
  }
  static __device__ __forceinline__ float at(const Raw& r, int e) { return (float)r.hi[e] + (float)r.lo[e]; }
  static __device__ __forceinline__ void load(const pf16* p, float (&v)[8]) {
    const Raw r = raw(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = at(r, e);
  }
  static __device__ __forceinline__ void store(pf16* p, const float (&v)[8]) {
    Raw r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const sf16 s(v[e]);
      r.hi[e] = s.hi; r.lo[e] = s.lo;
    }
    reinterpret_cast<h8*>(p)[0] = r.hi;
    reinterpret_cast<h8*>(p)[1] = r.lo;
  }
};

}  // namespace vnf
