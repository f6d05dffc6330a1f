// Launch interface of the persistent Block17 stack kernels: trunk17.hip (bf16 / f16) and its planar split-f16 twin
// trunk17s.hip (F16P: x / y are F16P tensors, 4 bytes per value, the pack's weights F16P-packed).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "kernels.h"

namespace vnf {

constexpr int T17_FRAGS = 168;   // (tile, k-step) weight fragments per wave per block: 56 reduce + 28 (1x7) + 28 (7x1) + 56 up
constexpr int T17_BIAS = 1408;   // fp32 biases per block: 256 reduce | 128 (1x7) | 128 (7x1) | 896 up
constexpr int T17_MAX_BLOCKS = 10;
constexpr int T17_RING = 8;      // weight fragments in flight per wave (divides T17_FRAGS)
#ifndef T17S_RING
#define T17S_RING 8              // ... of the planar twin (tools/micro/trunk17s_bench.hip builds it at other depths)
#endif

struct Trunk17Args {
  const void* x;        // (n, 64, ldx) NHWC input (first 896 channels of each pixel row)
  void* y;              // (n, 64, ldy) output
  int ldx, ldy, n, nblocks;
  const void* wstream;  // trunk17_repack output
  const float* bias;    // [nblocks][T17_BIAS]
};

// packed per-convolution weights [rows][kpad] of every block (engine layout, k = (kh, kw, c)), device pointers
struct Trunk17Pack {
  const void* w[T17_MAX_BLOCKS][4];   // reduce (256 rows, K 896), 1x7 (128, 896), 7x1 (128, 896), up (896, 256)
  int kpad[4];
  int nblocks;
};

// The weight stream: per wave (8 of them), per block, the wave's T17_FRAGS fragments in the order both kernels consume
// them, then the ring's zero fragments.  Fragment s of wave w is rows r0 .. r0 + 15, k = k0 .. k0 + 31 of convolution conv:
//   reduce : s = 2 ks + j,         ks in 0..27, j in 0..1    rows 128 j + 16 w    (56)
//   1x7    : s = 56 + ks,          ks in 0..27               rows 16 w            (28)
//   7x1    : s = 84 + ks,          ks in 0..27               rows 16 w            (28)
//   up     : s = 112 + 7 ks + j,   ks in 0..7, j in 0..6     rows 128 j + 16 w    (56)
// The 16-bit stream holds one 1-KiB fragment per s; the planar stream two, the hi plane then the lo plane.
struct Trunk17Frag { int conv, r0, k0; };
__host__ __device__ inline Trunk17Frag trunk17_frag(int s, int wave) {
  if (s < 56) return {0, 128 * (s & 1) + 16 * wave, 32 * (s >> 1)};
  if (s < 84) return {1, 16 * wave, 32 * (s - 56)};
  if (s < 112) return {2, 16 * wave, 32 * (s - 84)};
  return {3, 128 * ((s - 112) % 7) + 16 * wave, 32 * ((s - 112) / 7)};
}
// 1-KiB fragments of one wave's stream
inline size_t trunk17_wave_frags(int nblocks, int dtype) {
  return dtype == F16P ? (size_t)nblocks * T17_FRAGS * 2 + T17S_RING : (size_t)nblocks * T17_FRAGS + T17_RING;
}
inline size_t trunk17_stream_bytes(int nblocks, int dtype) { return 8 * trunk17_wave_frags(nblocks, dtype) * 1024; }

// dtype: BF16, F16 or F16P (anything else: hipErrorInvalidValue)
hipError_t trunk17_repack(const Trunk17Pack& p, int dtype, void* out, hipStream_t s);
hipError_t launch_trunk17(const Trunk17Args& a, int dtype, hipStream_t s);
hipError_t launch_trunk17s(const Trunk17Args& a, hipStream_t s);   // the twin's launcher, reached through launch_trunk17

}  // namespace vnf
