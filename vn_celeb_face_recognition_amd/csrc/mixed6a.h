// Launch interface of the mixed_6a branch-1 chain kernel (mixed6a.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace vnf {

constexpr int M6_BIAS = 640;     // fp32 biases: 192 (1x1) | 192 (3x3 p1) | 256 (3x3 s2)

struct Mixed6aArgs {
  const void* x;        // (n, 289, ldx) 16-bit NHWC block input (first 256 channels of each pixel row)
  void* y;              // (n, 64, ldy) the mixed_6a output; the kernel writes channels [coff, coff + 256)
  int ldx, ldy, coff, n;
  const void* wstream;  // mixed6a_repack output
  const float* bias;    // [M6_BIAS]
};

// packed per-convolution weights [rows][kpad] (engine layout, k = (kh, kw, c)), device pointers
struct Mixed6aPack {
  const void* w[3];     // 1x1 (192 rows, K 256), 3x3 p1 (192, 1728), 3x3 s2 (256, 1728)
  int kpad[3];
};

size_t mixed6a_stream_bytes();
hipError_t mixed6a_repack(const Mixed6aPack& p, void* out, hipStream_t s);
hipError_t launch_mixed6a(const Mixed6aArgs& a, int dtype, hipStream_t s);

}  // namespace vnf
