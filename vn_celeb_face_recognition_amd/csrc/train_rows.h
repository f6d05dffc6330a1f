// The row kernels of a classification training step, shared by the MLP trainer (mlp_train.hip) and the head trainer
// (head_train.hip): log_softmax + NLL + argmax match + dz per row, then the batch's loss mean and hit count.
// `static`: every translation unit that includes this gets kernels of its own (the library is built without
// relocatable device code).
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace vnf {

// one wave per row: log_softmax, NLL term, argmax match, dz = (softmax - onehot) / B
static __global__ void softmax_nll_kernel(const float* __restrict__ z, int C, int Bn, const int64_t* __restrict__ target,
                                   float* __restrict__ dz, float* __restrict__ loss_rows, int* __restrict__ hit_rows, float inv_b) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Bn) return;
  const float* x = z + (size_t)row * C;
  float m = -INFINITY;
  int mi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = x[c];
    if (v > m) { m = v; mi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o);
    const int oi = __shfl_xor(mi, o);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(x[c] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float ls = logf(s);
  // a label outside [0, C) (torch's NLLLoss asserts on it; the host layer raises before the launch) never indexes the
  // row: its loss term is NaN, so the step's loss shows it, and no out-of-range address is formed
  const long long tl = (long long)target[row];
  const bool tok = tl >= 0 && tl < (long long)C;
  const int t = tok ? (int)tl : -1;
  if (dz)
    for (int c = lane; c < C; c += 64) dz[(size_t)row * C + c] = (expf((x[c] - m) - ls) - (c == t ? 1.f : 0.f)) * inv_b;
  if (lane == 0) {
    loss_rows[row] = tok ? -((x[t] - m) - ls) : __builtin_nanf("");
    hit_rows[row] = mi == t ? 1 : 0;
  }
}

// loss = mean(loss_rows), hits = sum(hit_rows); one workgroup
static __global__ void reduce_rows_kernel(const float* __restrict__ loss_rows, const int* __restrict__ hit_rows, int Bn,
                                   float* __restrict__ loss_out, int* __restrict__ hits_out) {
  __shared__ float sl[256];
  __shared__ int sh[256];
  float l = 0.f;
  int h = 0;
  for (int i = threadIdx.x; i < Bn; i += 256) { l += loss_rows[i]; h += hit_rows[i]; }
  sl[threadIdx.x] = l; sh[threadIdx.x] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sh[threadIdx.x] += sh[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (loss_out) *loss_out = sl[0] / (float)Bn;
    if (hits_out) *hits_out = sh[0];
  }
}

}  // namespace vnf
