// What a set of Adam-trained tensors is, shared by the MLP trainer (mlp_train.hip) and the head trainer (head_train.hip):
// Adam's arithmetic on one element, the handle's table of named parameters with their moments, the bias-correction
// scalars of a step, and the launch of the loss rows (train_rows.h).  `static` / `__forceinline__` where device code or a
// kernel is named: every translation unit that includes this gets its own (the library is built without relocatable
// device code).
#pragma once
#include <cmath>
#include <cstring>
#include <string>

#include "engine.h"
#include "train_rows.h"

namespace vnf {

// torch.optim.Adam (no amsgrad, coupled weight decay) on one element, in the operation order of torch/optim/adam.py
// _single_tensor_adam:
//   g = g + wd*p ; m.lerp_(g, 1-b1) ; v = v*b2 + ((1-b2)*g)*g ; p += (-step_size) * (m / (sqrt(v)/bc2_sqrt + eps))
// step_size = lr / (1 - b1^t) and bc2_sqrt = sqrt(1 - b2^t) are formed on the host in double, as Python does
// (AdamTrainer::begin_step).
static __device__ __forceinline__ void adam_update(float grad, float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                   float b1, float b2, float eps, float wd, float step_size, float bc2_sqrt) {
  const float pi = *p;
  grad = grad + wd * pi;
  const float mi = *m + (1.f - b1) * (grad - *m);
  const float vi = *v * b2 + ((1.f - b2) * grad) * grad;
  *m = mi; *v = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  *p = pi + (-step_size) * (mi / denom);
}

// One trained tensor: its state_dict key, the parameter, Adam's exp_avg and exp_avg_sq, and the gradient when the
// trainer keeps gradients in memory (the MLP does, the head consumes them in registers).
struct AdamParam {
  const char* name = nullptr;
  size_t numel = 0;
  float *p = nullptr, *m = nullptr, *v = nullptr, *g = nullptr;
};

struct AdamTrainer : HandleBase {
  static constexpr HandleKind KINDS[2] = {HandleKind::MlpTrainer, HandleKind::HeadTrainer};   // handle_cast_base
  explicit AdamTrainer(HandleKind k) : HandleBase(k) {}
  AdamParam params[4];
  int n_params = 0, max_batch = 0;
  long long step = 0;
  float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f, wd = 0.f;
  float* loss_rows = nullptr;   // [max_batch], launch_loss_rows
  int* hit_rows = nullptr;

  // Parameter i = the state_dict tensor names[i] of numel[i] elements, uploaded; its moments zeroed.  Also the two row
  // buffers (max_batch is set by then).  `who`: the calling function, for the message.
  int init_params(WeightMap& wm, const std::string& who, const char* const* names, const size_t* numel, int n, bool with_grad) {
    (void)hipGetDevice(&device);
    for (n_params = 0; n_params < n; ++n_params) {
      AdamParam& a = params[n_params];
      a.name = names[n_params];
      a.numel = numel[n_params];
      const size_t bytes = a.numel * 4;
      const float* src = wm.get(a.name, (int64_t)a.numel);
      if (!src) return fail(VNF_E_MISSING, who + ": missing weight: " + wm.missing);
      a.p = (float*)upload(src, bytes);
      if (with_grad) a.g = (float*)dalloc(bytes);
      a.m = (float*)dalloc(bytes);
      a.v = (float*)dalloc(bytes);
      if (!a.p || (with_grad && !a.g) || !a.m || !a.v) return VNF_E_HIP;
      hipError_t me = hipMemset(a.m, 0, bytes);
      if (me == hipSuccess) me = hipMemset(a.v, 0, bytes);
      if (me != hipSuccess) return fail(VNF_E_HIP, who + ": hipMemset: " + hipGetErrorString(me));
    }
    loss_rows = (float*)dalloc((size_t)max_batch * 4);
    hit_rows = (int*)dalloc((size_t)max_batch * 4);
    return loss_rows && hit_rows ? VNF_OK : VNF_E_HIP;
  }

  // kind: 0 parameter, 1 Adam exp_avg, 2 Adam exp_avg_sq; name: one of the table's state_dict keys.  nullptr: neither.
  float* find(const char* name, int kind, size_t* numel) {
    for (int i = 0; i < n_params; ++i)
      if (name && !strcmp(name, params[i].name)) {
        *numel = params[i].numel;
        return kind == 0 ? params[i].p : kind == 1 ? params[i].m : kind == 2 ? params[i].v : nullptr;
      }
    return nullptr;
  }

  // Counts the step and forms its two bias-correction scalars, in double.
  void begin_step(float lr, float* step_size, float* bc2_sqrt) {
    step += 1;
    const double bc1 = 1.0 - std::pow((double)b1, (double)step), bc2 = 1.0 - std::pow((double)b2, (double)step);
    *step_size = (float)((double)lr / bc1);
    *bc2_sqrt = (float)std::sqrt(bc2);
  }
};

// Logits z (b,C) + targets -> loss_out / hits_out (device scalars), and dz (b,C) unless it is null: softmax_nll_kernel
// over the rows, then reduce_rows_kernel.  A free `static` function because it names this translation unit's kernels.
static hipError_t launch_loss_rows(const AdamTrainer& t, const float* z, int C, int b, const int64_t* target, float* dz, float* loss_out,
                                   int32_t* hits_out, hipStream_t s) {
  hipLaunchKernelGGL(softmax_nll_kernel, dim3((b + 3) / 4), dim3(256), 0, s, z, C, b, target, dz, t.loss_rows, t.hit_rows, 1.f / (float)b);
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(256), 0, s, t.loss_rows, t.hit_rows, b, loss_out, hits_out);
  return hipGetLastError();
}

}  // namespace vnf
