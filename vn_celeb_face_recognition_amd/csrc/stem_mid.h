// Launch interface of the fused conv2d_2a -> conv2d_2b -> maxpool_3a kernels: stem_mid.hip (bf16 / f16) and its planar
// split-f16 twin stem_mids.hip (F16P: x / y are F16P tensors, weights F16P-packed, conv2d_3b always fused).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "kernels.h"

namespace vnf {

// Weight fragments: 6 channel tiles x 9 taps in MFMA A order, tiles 0, 1 = conv2d_2a channels 0..31, tiles 2..5 =
// conv2d_2b channels 0..63; fragment (tile, tap) is rows 16 * tile' .. + 15, k = 32 * tap .. + 31.  1 KiB each in the 16-bit
// image; the planar image holds every one as a (hi, lo) pair.
constexpr int SM_FRAGS = 54;
inline size_t stem_mid_wfrag_bytes(int dtype) { return (size_t)SM_FRAGS * (dtype == F16P ? 2 : 1) * 1024; }
constexpr int SM_BIAS = 96;                 // fp32: 32 (conv2d_2a) | 64 (conv2d_2b)

struct StemMidArgs {
  const void* x;       // (n, 79, 79, ldx) NHWC conv2d_1a output (32 channels used)
  void* y;             // (n, 38, 38, ldy) pooled output, 64 channels
  int ldx, ldy, n;
  const void* wfrag;   // stem_mid_repack output
  const float* bias;   // [SM_BIAS]
  // optional: conv2d_3b (1x1, 64 -> 80, folded BN, ReLU) applied to every pooled row before it leaves the kernel; y is
  // then the (n, 38, 38, ldy) conv2d_3b output and the pooled tensor never reaches memory
  const void* w3b;     // packed engine weights [>= 80 rows][k3b_pad]; nullptr: no fusion
  const float* b3b;    // [80]
  int k3b_pad;
  long long* dbg = nullptr;   // in-kernel timer buffer of the instrumented launch (tools), else null
};

struct StemMidPack {    // packed engine weights [rows][kpad], k = (kh, kw, c): conv2d_2a (32 x 288), conv2d_2b (64 x 288)
  const void* w[2];
  int kpad[2];
};

// dtype: BF16, F16 or F16P (anything else: hipErrorInvalidValue)
hipError_t stem_mid_repack(const StemMidPack& p, int dtype, void* out, hipStream_t s);
hipError_t launch_stem_mid(const StemMidArgs& a, int dtype, hipStream_t s);
hipError_t launch_stem_mids(const StemMidArgs& a, hipStream_t s);   // the twin's launcher, reached through launch_stem_mid

}  // namespace vnf
