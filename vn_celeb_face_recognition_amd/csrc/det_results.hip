#include "det_results.h"

#include <algorithm>
#include <cstring>

namespace vnf {

int count_results(const char* who, const int* cnt, int b, int32_t* counts, int max_out, int32_t* n_out, int* maxf) {
  int total = 0;
  *maxf = 0;
  for (int i = 0; i < b; ++i) { counts[i] = cnt[i]; total += cnt[i]; *maxf = std::max(*maxf, cnt[i]); }
  *n_out = total;
  if (total > max_out) return fail(VNF_E_CAPACITY, std::string(who) + ": more faces than max_out");
  return VNF_OK;
}

void scatter_rows(const float* rows, int maxf, const int* cnt, int b, float* boxes, float* probs, float* points) {
  int o = 0;
  for (int i = 0; i < b; ++i)
    for (int k = 0; k < cnt[i]; ++k, ++o) {
      const float* f = &rows[((size_t)i * maxf + k) * 15];
      if (boxes) memcpy(boxes + (size_t)o * 4, f, 16);
      if (probs) probs[o] = f[4];
      if (points) memcpy(points + (size_t)o * 10, f + 5, 40);
    }
}

// device-resident copy of the last detection, frames concatenated in order (the host arrays' layout)
__global__ void results_device_kernel(const float* __restrict__ fin, const int* __restrict__ fin_cnt, int max_out, int row_stride,
                                      int32_t* __restrict__ fidx, float* __restrict__ boxes, float* __restrict__ probs,
                                      float* __restrict__ points) {
  const int img = blockIdx.x;
  int off = 0;
  for (int i = 0; i < img; ++i) off += fin_cnt[i];
  const int c = fin_cnt[img];
  for (int k = threadIdx.x; k < c; k += blockDim.x) {
    const int o = off + k;
    if (o >= max_out) break;
    const float* f = fin + ((size_t)img * row_stride + k) * 15;
    if (fidx) fidx[o] = img;
    if (boxes) { boxes[o * 4] = f[0]; boxes[o * 4 + 1] = f[1]; boxes[o * 4 + 2] = f[2]; boxes[o * 4 + 3] = f[3]; }
    if (probs) probs[o] = f[4];
    if (points)
      for (int j = 0; j < 10; ++j) points[o * 10 + j] = f[5 + j];
  }
}

int results_device(const char* who, const float* fin, const int* fin_cnt, int last_b, int row_stride, int32_t* frame_idx,
                   float* boxes, float* probs, float* points, int max_out, void* stream) {
  if (max_out < 0) return fail(VNF_E_INVALID, std::string(who) + ": bad argument");
  if (last_b == 0 || max_out == 0) return VNF_OK;  // the last detection found nothing
  hipLaunchKernelGGL(results_device_kernel, dim3(last_b), dim3(64), 0, (hipStream_t)stream, fin, fin_cnt, max_out, row_stride,
                     frame_idx, boxes, probs, points);
  VNF_HIP(hipGetLastError());
  return VNF_OK;
}

}  // namespace vnf
