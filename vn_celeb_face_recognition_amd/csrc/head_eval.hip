// Evaluation of a classification head: logits (+ targets) -> per-row log-probabilities, prediction, probability, loss and
// hit, and the two batch sums a validation loop reads (mlp_model.py:14 log_softmax; demo_image.py:125-129 argmax, exp;
// trainer/classification_trainer.py:42-80: F.nll_loss on the log_softmax output, losses/metrics.py:3-7 accuracy;
// trainer/base_trainer.py:177-200 result.csv columns).
//   head_eval_rows_kernel   one wave per row; without targets it is vnf_classify's log_softmax + argmax + prob
//   head_eval_sums_kernel   one wave adds the rows' nll / hit in index order: no float atomics, the same bits every run
//   head_eval_sums_rows_kernel   the sums when the caller keeps no per-row nll / hit: one workgroup recomputes the rows
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels.h"

namespace vnf {

struct RowStat { float m, ls; int mi; };   // row maximum, log(sum exp(x - m)), index of the first maximum

// max-subtracted log-sum-exp and first-occurrence argmax of one row, by one wave; every lane returns the same values
__device__ __forceinline__ RowStat row_stat(const float* __restrict__ x, int C, int lane) {
  float m = -INFINITY;
  int mi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = x[c];
    if (v > m) { m = v; mi = c; }   // first occurrence within the lane's stride
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o);
    const int oi = __shfl_xor(mi, o);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }   // ties: the lowest index
  }
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(x[c] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return RowStat{m, logf(s), mi};
}

// -logp[t] and argmax == t; a target outside [0, C) is never an index: +inf and no hit
__device__ __forceinline__ void row_score(const float* __restrict__ x, int C, const RowStat& r, long long t, float* nll, int* hit) {
  const bool ok = t >= 0 && t < (long long)C;
  *nll = ok ? -((x[ok ? t : 0] - r.m) - r.ls) : INFINITY;
  *hit = (ok && (long long)r.mi == t) ? 1 : 0;
}

__global__ void head_eval_rows_kernel(const float* __restrict__ logits, int ld, int C, int n, const long long* __restrict__ target,
                                      float* __restrict__ logp, int32_t* __restrict__ amax, float* __restrict__ prob,
                                      float* __restrict__ nll, int32_t* __restrict__ hit) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* x = logits + (size_t)row * ld;
  const RowStat r = row_stat(x, C, lane);
  if (logp)
    for (int c = lane; c < C; c += 64) logp[(size_t)row * C + c] = (x[c] - r.m) - r.ls;
  if (lane == 0) {
    if (amax) amax[row] = r.mi;
    if (prob) prob[row] = expf(-r.ls);   // exp(logp[argmax]), logp[argmax] = 0 - log(sum)
    if (target && (nll || hit)) {
      float l;
      int h;
      row_score(x, C, r, target[row], &l, &h);
      if (nll) nll[row] = l;
      if (hit) hit[row] = h;
    }
  }
}

// one wave: 64 rows per step come in with one load, then every lane adds them in index order
__global__ void head_eval_sums_kernel(const float* __restrict__ nll, const int32_t* __restrict__ hit, int n, float* __restrict__ sums) {
  const int lane = threadIdx.x;
  float sl = 0.f, sh = 0.f;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const float vl = i < n ? nll[i] : 0.f;
    const float vh = i < n ? (float)hit[i] : 0.f;
    const int cnt = n - base < 64 ? n - base : 64;
    for (int j = 0; j < cnt; ++j) {
      sl += __shfl(vl, j);
      sh += __shfl(vh, j);
    }
  }
  if (lane == 0) { sums[0] = sl; sums[1] = sh; }
}

// 16 waves, 16 rows per step; thread 0 adds each step's rows in index order
__global__ void head_eval_sums_rows_kernel(const float* __restrict__ logits, int ld, int C, int n, const long long* __restrict__ target,
                                           float* __restrict__ sums) {
  __shared__ float s_nll[16];
  __shared__ int s_hit[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float sl = 0.f, sh = 0.f;
  for (int base = 0; base < n; base += 16) {
    const int row = base + wave;
    if (row < n) {
      const float* x = logits + (size_t)row * ld;
      const RowStat r = row_stat(x, C, lane);
      if (lane == 0) row_score(x, C, r, target[row], &s_nll[wave], &s_hit[wave]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = n - base < 16 ? n - base : 16;
      for (int j = 0; j < cnt; ++j) { sl += s_nll[j]; sh += (float)s_hit[j]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { sums[0] = sl; sums[1] = sh; }
}

hipError_t launch_head_eval(const float* logits, int ld, int C, int n, const int64_t* target, float* logp, int32_t* amax,
                            float* prob, float* nll, int32_t* hit, float* sums, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const long long* t = reinterpret_cast<const long long*>(target);
  if (logp || amax || prob || nll || hit)
    hipLaunchKernelGGL(head_eval_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, s, logits, ld, C, n, t, logp, amax, prob, nll, hit);
  if (sums) {
    if (nll && hit)
      hipLaunchKernelGGL(head_eval_sums_kernel, dim3(1), dim3(64), 0, s, (const float*)nll, (const int32_t*)hit, n, sums);
    else
      hipLaunchKernelGGL(head_eval_sums_rows_kernel, dim3(1), dim3(1024), 0, s, logits, ld, C, n, t, sums);
  }
  return hipGetLastError();
}

}  // namespace vnf
