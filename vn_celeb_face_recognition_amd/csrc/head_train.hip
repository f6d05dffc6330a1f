// Training of the `logits` layer of a frozen encoder: the optimisation step of
// trainer/classification_trainer.py:9-40 for iresnet100(n_classes=..., freeze_weights=True) (models/iresnet_encoder.py:
// 174-179: every parameter but `logits` is frozen) with torch.optim.Adam, on the encoder's fp32 (b,512) features.  fp32
// end to end on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32 == an fp32 fma chain).
//
//   z  = feat W^T + bias ;  logp = log_softmax(z) ;  loss = -mean_b logp[b, t_b]          (losses/__init__.py: NLLLoss)
//   dz = (softmax(z) - onehot(t)) / b ;  dW = dz^T feat ;  dbias = sum_b dz ;  Adam with coupled weight decay
//
// A training step is four launches: head_logits_kernel, softmax_nll_kernel, reduce_rows_kernel (train_rows.h, shared with
// the MLP trainer) and head_update_kernel.  The gradient of W never reaches memory: head_update_kernel owns a tile of
// classes x inputs, accumulates dz^T feat over the batch in MFMA accumulators (the reduction dimension is the batch) and
// applies weight decay and Adam to W, exp_avg and exp_avg_sq straight from them.  dz (b,C) and feat (b,512) are both
// batch-major, which is the k-major form both 16x16x4 operands load in, so nothing is transposed.  No atomics, one fixed
// summation order: a step is bitwise repeatable.  Tails (b % 4, C % 16, C < 16) are masked in the loads and stores.
#include <memory>
#include <string>

#include "adam_params.h"

namespace vnf {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int HEAD_K = 512;   // width of the features every encoder's `logits` layer reads

// z[b][c] = sum_k feat[b][k] W[c][k] + bias[c].  One wave per 16 rows x 16 classes, 4 waves (64 classes) per workgroup.
// A lane reads 4 consecutive k of its row of feat and of W (16 bytes each) and feeds them to 4 MFMAs: MFMA j of a group of
// 16 k takes k = 4*(lane>>4) + j from both operands, a fixed permutation of the k order inside the group.
__global__ void __launch_bounds__(256) head_logits_kernel(const float* __restrict__ feat, const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ z, int Bn, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = (blockIdx.x * 4 + wave) * 16, b0 = blockIdx.y * 16;
  if (c0 >= C) return;
  const int ar = b0 + (lane & 15), br = c0 + (lane & 15), kq = 4 * (lane >> 4);
  const bool aok = ar < Bn, bok = br < C;
  const float* ap = feat + (size_t)(aok ? ar : 0) * HEAD_K + kq;
  const float* bp = W + (size_t)(bok ? br : 0) * HEAD_K + kq;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k0 = 0; k0 < HEAD_K; k0 += 16) {
    f32x4_t a = *reinterpret_cast<const f32x4_t*>(ap + k0), b = *reinterpret_cast<const f32x4_t*>(bp + k0);
    if (!aok) a = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (!bok) b = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
  }
  // D[row = 4*(lane>>4) + r][col = lane & 15]: row from A (batch), column from B (class)
  const int c = c0 + (lane & 15);
  if (c < C) {
    const float bv = bias[c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = b0 + 4 * (lane >> 4) + r;
      if (m < Bn) z[(size_t)m * C + c] = acc[r] + bv;
    }
  }
}

// dW[c][k] = sum_b dz[b][c] feat[b][k], consumed in registers.  A workgroup owns 16 classes x 128 inputs, a wave 16 x 32
// (two accumulators).  Per K step of 4 batch rows: A[lane&15][lane>>4] = dz[b0 + (lane>>4)][c0 + (lane&15)],
// B[lane>>4][lane&15] = feat[b0 + (lane>>4)][k0 + (lane&15)], rows of 16 consecutive floats.  The workgroups of the first
// input tile also own their 16 classes' bias: db = sum_b dz in batch order, then the same update.
__global__ void __launch_bounds__(256) head_update_kernel(const float* __restrict__ dz, const float* __restrict__ feat, int Bn, int C,
                                                          float* __restrict__ W, float* __restrict__ mW, float* __restrict__ vW,
                                                          float* __restrict__ bias, float* __restrict__ mB, float* __restrict__ vB,
                                                          float b1, float b2, float eps, float wd, float step_size, float bc2_sqrt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = blockIdx.y * 16, k0 = blockIdx.x * 128 + wave * 32;
  const int ca = c0 + (lane & 15), kr = lane >> 4;
  const bool cok = ca < C;
  f32x4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const float* fp = feat + k0 + (lane & 15);
  const int full = Bn & ~3;
  for (int r0 = 0; r0 < full; r0 += 4) {
    const size_t row = (size_t)(r0 + kr);
    const float a = cok ? dz[row * C + ca] : 0.f;
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, fp[row * HEAD_K], acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, fp[row * HEAD_K + 16], acc[1], 0, 0, 0);
  }
  if (full < Bn) {   // the last 1..3 rows: the K step's other rows are zero
    const size_t row = (size_t)(full + kr);
    const bool rok = full + kr < Bn;
    const float a = (rok && cok) ? dz[row * C + ca] : 0.f;
    const float f0 = rok ? fp[row * HEAD_K] : 0.f, f1 = rok ? fp[row * HEAD_K + 16] : 0.f;
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, f0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, f1, acc[1], 0, 0, 0);
  }
  // D[row = 4*(lane>>4) + r][col = lane & 15]: row from A (class), column from B (input)
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + 4 * (lane >> 4) + r;
      if (c < C) {
        const size_t i = (size_t)c * HEAD_K + k0 + 16 * j + (lane & 15);
        adam_update(acc[j][r], W + i, mW + i, vW + i, b1, b2, eps, wd, step_size, bc2_sqrt);
      }
    }
  if (blockIdx.x == 0 && threadIdx.x < 16) {
    const int c = c0 + threadIdx.x;
    if (c < C) {
      float g = 0.f;
      for (int r = 0; r < Bn; ++r) g += dz[(size_t)r * C + c];
      adam_update(g, bias + c, mB + c, vB + c, b1, b2, eps, wd, step_size, bc2_sqrt);
    }
  }
}

// params: logits.weight [C][512], logits.bias [C], no gradients in memory
struct HeadTrainer : AdamTrainer {
  static constexpr HandleKind KIND = HandleKind::HeadTrainer;
  HeadTrainer() : AdamTrainer(KIND) {}
  int C = 0;
  float *z = nullptr, *dz = nullptr;
};

static const char* const kHeadNames[2] = {"logits.weight", "logits.bias"};

}  // namespace vnf
using namespace vnf;

extern "C" int vnf_head_trainer_create(const vnf_tensor_desc* weights, int n_weights, int num_classes, int max_batch, float beta1,
                                       float beta2, float eps, float weight_decay, vnf_handle* out) {
  try {
    if (!out || !weights || num_classes <= 0 || num_classes > (1 << 20) || max_batch <= 0 || max_batch > 65535 * 16)
      return fail(VNF_E_INVALID, "vnf_head_trainer_create: bad argument");
    *out = nullptr;
    WeightMap wm(weights, n_weights);
    std::unique_ptr<HeadTrainer> t(new HeadTrainer());
    t->C = num_classes; t->max_batch = max_batch;
    t->b1 = beta1; t->b2 = beta2; t->eps = eps; t->wd = weight_decay;
    const size_t C = num_classes, B = max_batch;
    const size_t ne[2] = {C * HEAD_K, C};
    if (const int rc = t->init_params(wm, "vnf_head_trainer_create", kHeadNames, ne, 2, false)) return rc;
    t->z = (float*)t->dalloc(B * C * 4);
    t->dz = (float*)t->dalloc(B * C * 4);
    if (!t->z || !t->dz) return VNF_E_HIP;
    const hipError_t se = hipDeviceSynchronize();
    if (se != hipSuccess) return fail(VNF_E_HIP, std::string("vnf_head_trainer_create: ") + hipGetErrorString(se));
    *out = reinterpret_cast<vnf_handle>(static_cast<HandleBase*>(t.release()));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

// forward (+ loss / hits); train != 0: backward + Adam step with learning rate lr.  Checkpoint access: vnf_trainer_get /
// _set / _step_count (mlp_train.hip).
extern "C" int vnf_head_train_step(vnf_handle h, const float* feat, const int64_t* target, int b, float lr, int train, float* loss_out,
                                   int32_t* hits_out, void* stream) {
  try {
    HeadTrainer* t = handle_cast<HeadTrainer>(h);
    if (!t) return fail(VNF_E_INVALID, "not a head trainer handle");
    if (b <= 0 || b > t->max_batch) return fail(VNF_E_CAPACITY, "vnf_head_train_step: batch exceeds max_batch");
    if (!feat || !target) return fail(VNF_E_INVALID, "vnf_head_train_step: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int C = t->C;
    const AdamParam &W = t->params[0], &B = t->params[1];
    hipLaunchKernelGGL(head_logits_kernel, dim3((C + 63) / 64, (b + 15) / 16), dim3(256), 0, s, feat, W.p, B.p, t->z, b, C);
    VNF_HIP(launch_loss_rows(*t, t->z, C, b, target, train ? t->dz : nullptr, loss_out, hits_out, s));
    if (!train) return VNF_OK;
    float step_size, bc2s;
    t->begin_step(lr, &step_size, &bc2s);
    hipLaunchKernelGGL(head_update_kernel, dim3(HEAD_K / 128, (C + 15) / 16), dim3(256), 0, s, t->dz, feat, b, C, W.p, W.m, W.v, B.p, B.m, B.v,
                       t->b1, t->b2, t->eps, t->wd, step_size, bc2s);
    VNF_HIP(hipGetLastError());
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
