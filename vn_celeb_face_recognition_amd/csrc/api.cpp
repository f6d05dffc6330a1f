// extern "C" surface of libvnface.so (declared in include/vnface.h).  No exception crosses it.
#include <cstring>
#include <new>

#include "plan.h"

using namespace vnf;

#define API_GUARD_BEGIN try {
#define API_GUARD_END                                                  \
  }                                                                    \
  catch (const std::bad_alloc&) { return fail(VNF_E_INVALID, "host out of memory"); } \
  catch (const std::exception& ex) { return fail(VNF_E_INVALID, std::string("exception: ") + ex.what()); } \
  catch (...) { return fail(VNF_E_INVALID, "unknown exception"); }

// An encoder handle of `arch` on the plan `build` makes: what vnf_encoder_create and vnf_emotion_create share
template <class Build>
static int create_encoder(int arch, const vnf_tensor_desc* weights, int n_weights, int compute_dtype, int max_batch, vnf_handle* out,
                          Build build) {
  if (!out || !weights || n_weights <= 0 || max_batch <= 0) return fail(VNF_E_INVALID, "bad argument");
  if (compute_dtype != VNF_F32 && compute_dtype != VNF_BF16 && compute_dtype != VNF_F16 && compute_dtype != VNF_F16X2)
    return fail(VNF_E_INVALID, "compute_dtype must be VNF_F32, VNF_BF16, VNF_F16 or VNF_F16X2");
  *out = nullptr;
  Encoder* e = new Encoder();
  e->arch = arch;
  // VNF_F32/BF16/F16 == vnf::F32/BF16/F16; the encoders keep VNF_F16X2 tensors PLANAR (F16P: 8-channel units
  // [8 hi][8 lo], three MFMAs per product, split_f16.h)
  e->dtype = compute_dtype == VNF_F16X2 ? F16P : compute_dtype;
  e->max_batch = max_batch;
  (void)hipGetDevice(&e->device);
  WeightMap wm(weights, n_weights);
  int r = build(*e, wm);
  if (r == VNF_OK) r = e->finalize();
  if (r != VNF_OK) { delete e; return r; }
  VNF_HIP(hipDeviceSynchronize());
  *out = reinterpret_cast<vnf_handle>(static_cast<HandleBase*>(e));
  return VNF_OK;
}

extern "C" {

const char* vnf_last_error(void) { return last_error_cstr(); }
const char* vnf_version(void) { return "vnface 0.1 (gfx950)"; }

int vnf_init(int device_ordinal) {
  API_GUARD_BEGIN
  int n = 0;
  VNF_HIP(hipGetDeviceCount(&n));
  if (device_ordinal < 0 || device_ordinal >= n) return fail(VNF_E_INVALID, "no such device");
  VNF_HIP(hipSetDevice(device_ordinal));
  hipDeviceProp_t p;
  VNF_HIP(hipGetDeviceProperties(&p, device_ordinal));
  if (strncmp(p.gcnArchName, "gfx950", 6) != 0)
    return fail(VNF_E_INVALID, std::string("libvnface is built for gfx950 only, device is ") + p.gcnArchName);
  return VNF_OK;
  API_GUARD_END
}

int vnf_destroy(vnf_handle h) {
  API_GUARD_BEGIN
  delete reinterpret_cast<HandleBase*>(h);
  return VNF_OK;
  API_GUARD_END
}

int vnf_encoder_create(int arch, const vnf_tensor_desc* weights, int n_weights, int compute_dtype, int max_batch,
                       vnf_handle* out) {
  API_GUARD_BEGIN
  return create_encoder(arch, weights, n_weights, compute_dtype, max_batch, out, [&](Encoder& e, WeightMap& wm) {
    return arch == VNF_ARCH_IRV1    ? build_irv1(e, wm)
           : arch == VNF_ARCH_IR100 ? build_ir100(e, wm)
           : arch == VNF_ARCH_SEIR101 ? build_seir101(e, wm)
                                      : fail(VNF_E_INVALID, "unknown arch");
  });
  API_GUARD_END
}

// `logits` (num_classes, 512) + bias on the encoder's fp32 features: an exact-f32 linear plan of its own, whatever the
// encoder computes in (inception_resnet_v1.py:260-265,298-300; iresnet_encoder.py:100-103,155-157)
static int attach_head(Encoder& e, WeightMap& wm, int num_classes) {
  const float* w = wm.get("logits.weight", (int64_t)num_classes * 512);
  const float* b = wm.get("logits.bias", num_classes);
  if (!w || !b) return fail(VNF_E_MISSING, "vnf_encoder_create_classifier: missing weight: " + wm.missing);
  Encoder* hd = new Encoder();
  e.head = hd;   // owned from here on: ~Encoder deletes it
  e.head_classes = num_classes;
  const int cpad = (num_classes + 7) / 8 * 8;
  hd->dtype = F32; hd->max_batch = e.max_batch; hd->in_size = 1; hd->arch = ARCH_MLP; hd->device = e.device;
  hd->max_streams = 1;
  e.head_in = hd->add_buf(1, 1, 512);
  e.head_logit = hd->add_buf(1, 1, cpad);
  int r = add_linear(*hd, "logits", w, b, 512, num_classes, cpad, e.head_in, e.head_logit, ACT_NONE);
  if (r == VNF_OK) r = hd->finalize();
  if (r != VNF_OK) return r;
  e.head_emb = (float*)e.dalloc((size_t)e.max_batch * 512 * 4);
  return e.head_emb ? VNF_OK : VNF_E_HIP;
}

int vnf_encoder_create_classifier(int arch, const vnf_tensor_desc* weights, int n_weights, int compute_dtype, int max_batch,
                                  int num_classes, vnf_handle* out) {
  API_GUARD_BEGIN
  if (num_classes < 1 || num_classes > (1 << 20)) return fail(VNF_E_INVALID, "vnf_encoder_create_classifier: num_classes must be 1..2^20");
  if (arch == VNF_ARCH_SEIR101)
    return fail(VNF_E_INVALID, "vnf_encoder_create_classifier: the SE-IR ResNet-101 has no `logits` layer (models/resnet_encoder.py:154-222)");
  return create_encoder(arch, weights, n_weights, compute_dtype, max_batch, out, [&](Encoder& e, WeightMap& wm) {
    const int r = arch == VNF_ARCH_IRV1 ? build_irv1(e, wm) : arch == VNF_ARCH_IR100 ? build_ir100(e, wm) : fail(VNF_E_INVALID, "unknown arch");
    return r != VNF_OK ? r : attach_head(e, wm, num_classes);
  });
  API_GUARD_END
}

int vnf_encoder_logprobs(vnf_handle h, const void* x, int n, int x_dtype, float* logp_out, int32_t* amax_out, float* prob_out,
                         void* stream) {
  API_GUARD_BEGIN
  Encoder* e = handle_cast<Encoder>(h);
  if (!e) return fail(VNF_E_INVALID, "not an encoder handle");
  if (!e->head) return fail(VNF_E_INVALID, "vnf_encoder_logprobs: the handle has no classification head (vnf_encoder_create_classifier)");
  if (n < 0 || (n > 0 && !x)) return fail(VNF_E_INVALID, "bad argument");
  if (x_dtype != VNF_F32 && x_dtype != VNF_BF16 && x_dtype != VNF_F16) return fail(VNF_E_INVALID, "bad x_dtype");
  if (n > e->max_batch) return fail(VNF_E_CAPACITY, "batch exceeds max_batch");
  if (n == 0) return VNF_OK;
  hipStream_t s = (hipStream_t)stream;
  Encoder& hd = *e->head;
  if (e->head_done) VNF_HIP(hipStreamWaitEvent(s, e->head_done, 0));
  else VNF_HIP(hipEventCreateWithFlags(&e->head_done, hipEventDisableTiming));
  int r = e->run(x, n, x_dtype, e->head_emb, s);
  if (r != VNF_OK) return r;
  // emb_raw is the feature buffer of the activation context this run used: last_bn's output before the normalisation
  // (IRv1), `features` (IR-100)
  VNF_HIP(hipMemcpyAsync(hd.bufs[e->head_in].ptr, e->emb_raw, (size_t)n * 512 * 4, hipMemcpyDeviceToDevice, s));
  if (e->n_ctx > 1) {   // the context is free again only after this copy
    const int c = (e->next_ctx + e->n_ctx - 1) % e->n_ctx;
    VNF_HIP(hipEventRecord(e->ctx_ev[c], s));
  }
  r = hd.run(nullptr, n, VNF_F32, nullptr, s);
  if (r != VNF_OK) return r;
  VNF_HIP(launch_head_eval((const float*)hd.bufs[e->head_logit].ptr, hd.bufs[e->head_logit].C, e->head_classes, n, nullptr, logp_out,
                           amax_out, prob_out, nullptr, nullptr, nullptr, s));
  VNF_HIP(hipEventRecord(e->head_done, s));
  return VNF_OK;
  API_GUARD_END
}

int vnf_logits_eval(const float* logits, int n, int c, int ld, const int64_t* target, float* logp, int32_t* amax, float* prob,
                    float* nll, int32_t* hit, float* sums, void* stream) {
  API_GUARD_BEGIN
  if (n < 0 || c < 1 || ld < c) return fail(VNF_E_INVALID, "vnf_logits_eval: need n >= 0, c >= 1, ld >= c");
  if (n == 0) return VNF_OK;
  if (!logits) return fail(VNF_E_INVALID, "vnf_logits_eval: logits must not be NULL");
  if (!target && (nll || hit || sums)) return fail(VNF_E_INVALID, "vnf_logits_eval: nll, hit and sums need a target");
  VNF_HIP(launch_head_eval(logits, ld, c, n, target, logp, amax, prob, nll, hit, sums, (hipStream_t)stream));
  return VNF_OK;
  API_GUARD_END
}

int vnf_embed(vnf_handle h, const void* x, int n, int x_dtype, float* emb_out, void* stream) {
  API_GUARD_BEGIN
  Encoder* e = handle_cast<Encoder>(h);
  if (!e) return fail(VNF_E_INVALID, "not an encoder handle");
  if (e->arch == VNF_ARCH_RN50_2B) return fail(VNF_E_INVALID, "emotion handle: use vnf_emotion_forward");
  if (n < 0 || (n > 0 && (!x || !emb_out))) return fail(VNF_E_INVALID, "bad argument");
  if (x_dtype != VNF_F32 && x_dtype != VNF_BF16 && x_dtype != VNF_F16) return fail(VNF_E_INVALID, "bad x_dtype");
  return e->run(x, n, x_dtype, emb_out, (hipStream_t)stream);
  API_GUARD_END
}

int vnf_encoder_features(vnf_handle h, const void* x, int n, int x_dtype, float* feat_out, void* stream) {
  API_GUARD_BEGIN
  Encoder* e = handle_cast<Encoder>(h);
  if (!e) return fail(VNF_E_INVALID, "not an encoder handle");
  if (e->arch == VNF_ARCH_RN50_2B) return fail(VNF_E_INVALID, "emotion handle: use vnf_emotion_forward");
  if (n < 0 || (n > 0 && (!x || !feat_out))) return fail(VNF_E_INVALID, "bad argument");
  if (x_dtype != VNF_F32 && x_dtype != VNF_BF16 && x_dtype != VNF_F16) return fail(VNF_E_INVALID, "bad x_dtype");
  if (n > e->max_batch) return fail(VNF_E_CAPACITY, "batch exceeds max_batch");
  if (n == 0) return VNF_OK;
  hipStream_t s = (hipStream_t)stream;
  // the plan's last op writes the embeddings to feat_out; where those are not the features themselves (a normalising
  // plan), emb_raw of the activation context this run used then replaces them
  const int r = e->run(x, n, x_dtype, feat_out, s);
  if (r != VNF_OK || e->arch == VNF_ARCH_IR100) return r;
  VNF_HIP(hipMemcpyAsync(feat_out, e->emb_raw, (size_t)n * 512 * 4, hipMemcpyDeviceToDevice, s));
  if (e->n_ctx > 1) {   // the context is free again only after this copy
    const int c = (e->next_ctx + e->n_ctx - 1) % e->n_ctx;
    VNF_HIP(hipEventRecord(e->ctx_ev[c], s));
  }
  return VNF_OK;
  API_GUARD_END
}

int vnf_encoder_tap(vnf_handle h, const char* name, int n, float* host_out, int64_t capacity, int64_t shape_out[4]) {
  API_GUARD_BEGIN
  Encoder* e = handle_cast<Encoder>(h);
  if (!e || !name) return fail(VNF_E_INVALID, "not an encoder handle");
  auto it = e->taps.find(name);
  if (it == e->taps.end()) return fail(VNF_E_INVALID, std::string("no such tap: ") + name);
  if (it->second.buf == -2) {   // the fp32 features of the last call (emb_raw), as (n,C,1,1)
    const int C = it->second.C;
    if (shape_out) { shape_out[0] = n; shape_out[1] = C; shape_out[2] = 1; shape_out[3] = 1; }
    if (n > e->max_batch || (int64_t)n * C > capacity || !host_out) return fail(VNF_E_CAPACITY, "tap capacity");
    for (int i = 0; i < n; ++i)
      VNF_HIP(hipMemcpy(host_out + (size_t)i * C, e->emb_raw + (size_t)i * e->emb_ld + it->second.coff, (size_t)C * 4, hipMemcpyDeviceToHost));
    return VNF_OK;
  }
  if (!e->buf_materialised(it->second.buf))
    return fail(VNF_E_INVALID, std::string("tap '") + name + "' is computed inside a fused kernel and never reaches memory in this "
                "compute dtype: create the encoder under VNF_FUSE=0 (or use a dtype without fused stacks) to read it");
  const Buf& b = e->bufs[it->second.buf];
  const int C = it->second.C;
  const int64_t total = (int64_t)n * C * b.H * b.W;
  if (shape_out) { shape_out[0] = n; shape_out[1] = C; shape_out[2] = b.H; shape_out[3] = b.W; }
  if (n > e->max_batch || total > capacity || !host_out) return fail(VNF_E_CAPACITY, "tap capacity");
  float* tmp = nullptr;
  VNF_HIP(hipMalloc(&tmp, (size_t)total * 4));
  hipError_t err = launch_nhwc_to_nchw_f32(b.ptr + (size_t)it->second.coff * dtype_size(e->dtype), b.C, e->dtype, tmp, n,
                                           b.H * b.W, C, 0);
  if (err == hipSuccess) err = hipMemcpy(host_out, tmp, (size_t)total * 4, hipMemcpyDeviceToHost);
  (void)hipFree(tmp);
  if (err != hipSuccess) return fail(VNF_E_HIP, hipGetErrorString(err));
  return VNF_OK;
  API_GUARD_END
}

int vnf_encoder_profile(vnf_handle h, const void* x, int n, int x_dtype, float* emb_out, void* stream, char* report,
                        int64_t capacity) {
  API_GUARD_BEGIN
  Encoder* e = handle_cast<Encoder>(h);
  if (!e || !report || capacity <= 0) return fail(VNF_E_INVALID, "bad argument");
  std::string rep;
  int r = e->run(x, n, x_dtype, emb_out, (hipStream_t)stream, &rep);
  if (r != VNF_OK) return r;
  strncpy(report, rep.c_str(), (size_t)capacity - 1);
  report[capacity - 1] = 0;
  return VNF_OK;
  API_GUARD_END
}

int vnf_encoder_flops(vnf_handle h, double* algorithmic, double* executed) {
  API_GUARD_BEGIN
  Encoder* e = handle_cast<Encoder>(h);
  if (!e) return fail(VNF_E_INVALID, "not an encoder handle");
  if (algorithmic) *algorithmic = 2.0 * e->macs_alg;
  if (executed) *executed = 2.0 * e->macs_exec;
  return VNF_OK;
  API_GUARD_END
}

int vnf_encoder_set_streams(vnf_handle h, int max_streams) {
  API_GUARD_BEGIN
  Encoder* e = handle_cast<Encoder>(h);
  if (!e) return fail(VNF_E_INVALID, "not an encoder handle");
  if (max_streams < 1 || max_streams > 4) return fail(VNF_E_INVALID, "vnf_encoder_set_streams: 1..4");
  if (e->max_streams != max_streams) {
    e->max_streams = max_streams;
    e->tune_dirty = true;  // the part size the layers see changed: the next vnf_embed picks the tiles again
  }
  return VNF_OK;
  API_GUARD_END
}

int vnf_encoder_set_contexts(vnf_handle h, int n) {
  API_GUARD_BEGIN
  Encoder* e = handle_cast<Encoder>(h);
  if (!e) return fail(VNF_E_INVALID, "not an encoder handle");
  if (n < 1 || n > 4) return fail(VNF_E_INVALID, "vnf_encoder_set_contexts: 1..4");
  if (e->arch == VNF_ARCH_RN50_2B && n != 1) return fail(VNF_E_INVALID, "vnf_encoder_set_contexts: not for the emotion network");
  e->n_ctx = n;
  e->next_ctx = 0;
  if (e->tune_lanes != n) {
    e->tune_lanes = n;
    e->tune_dirty = true;  // the next vnf_embed picks the tiles for `n` kernels sharing the GPU
  }
  return VNF_OK;
  API_GUARD_END
}

// ---- emotion network (ResNet-50, two heads): an Encoder of arch VNF_ARCH_RN50_2B
int vnf_emotion_create(const vnf_tensor_desc* weights, int n_weights, int num_classes, int num_projections, int compute_dtype,
                       int max_batch, vnf_handle* out) {
  API_GUARD_BEGIN
  if (num_classes < 1 || num_projections < 1 || num_classes > 65536 || num_projections > 65536) return fail(VNF_E_INVALID, "bad argument");
  const int r = create_encoder(VNF_ARCH_RN50_2B, weights, n_weights, compute_dtype, max_batch, out, [&](Encoder& e, WeightMap& wm) {
    return build_rn50_2b(e, wm, num_classes, num_projections);
  });
  if (r != VNF_OK) return r;
  Encoder* e = handle_cast<Encoder>(*out);
  e->cls_buf = (float*)e->dalloc((size_t)max_batch * num_classes * 4);
  if (!e->cls_buf) { delete e; *out = nullptr; return VNF_E_HIP; }
  return VNF_OK;
  API_GUARD_END
}

static Encoder* as_emotion(vnf_handle h) {
  Encoder* e = handle_cast<Encoder>(h);
  return (e && e->arch == VNF_ARCH_RN50_2B) ? e : nullptr;
}

int vnf_emotion_forward(vnf_handle h, const void* x, int n, int x_dtype, float* cls_out, float* proj_out, void* stream) {
  API_GUARD_BEGIN
  Encoder* e = as_emotion(h);
  if (!e) return fail(VNF_E_INVALID, "not an emotion handle");
  if (n < 0 || (n > 0 && !x)) return fail(VNF_E_INVALID, "bad argument");
  if (x_dtype != VNF_F32 && x_dtype != VNF_BF16 && x_dtype != VNF_F16) return fail(VNF_E_INVALID, "bad x_dtype");
  RunExtra ex;
  ex.out2 = proj_out;
  return e->run(x, n, x_dtype, cls_out, (hipStream_t)stream, nullptr, &ex);
  API_GUARD_END
}

int vnf_emotion_recognize(vnf_handle h, const uint8_t* faces_u8, int n, int s, int k, int32_t* idx_out, float* prob_out,
                          float* cls_out, void* stream) {
  API_GUARD_BEGIN
  Encoder* e = as_emotion(h);
  if (!e) return fail(VNF_E_INVALID, "not an emotion handle");
  if (n < 0 || (n > 0 && (!faces_u8 || !idx_out || !prob_out))) return fail(VNF_E_INVALID, "bad argument");
  if (s < 1 || s > 224) return fail(VNF_E_INVALID, "face size must be 1..224");
  if (k < 1 || k > 16 || k > e->n_cls) return fail(VNF_E_INVALID, "k must be 1..16 and <= num_classes");
  if (n > e->max_batch) return fail(VNF_E_CAPACITY, "batch exceeds max_batch");
  if (n == 0) return VNF_OK;
  float* cls = cls_out ? cls_out : e->cls_buf;
  RunExtra ex;
  ex.prep_src = faces_u8;
  ex.prep_s = s;
  const int r = e->run(nullptr, n, VNF_F32, cls, (hipStream_t)stream, nullptr, &ex);
  if (r != VNF_OK) return r;
  VNF_HIP(launch_softmax_topk(cls, n, e->n_cls, k, idx_out, prob_out, (hipStream_t)stream));
  return VNF_OK;
  API_GUARD_END
}

int vnf_emotion_prep(const uint8_t* faces_u8, int n, int s, void* x_out, int out_dtype, void* stream) {
  API_GUARD_BEGIN
  if (n < 0 || (n > 0 && (!faces_u8 || !x_out))) return fail(VNF_E_INVALID, "bad argument");
  if (s < 1 || s > 224) return fail(VNF_E_INVALID, "face size must be 1..224");
  if (out_dtype != VNF_F32 && out_dtype != VNF_BF16 && out_dtype != VNF_F16) return fail(VNF_E_INVALID, "bad out_dtype");
  for (int n0 = 0; n0 < n; n0 += 32768) {
    const int nn = n - n0 < 32768 ? n - n0 : 32768;
    VNF_HIP(launch_emotion_prep(faces_u8 + (size_t)n0 * s * s * 3, nn, s,
                                (char*)x_out + (size_t)n0 * 3 * 224 * 224 * dtype_size(out_dtype), out_dtype, false,
                                (hipStream_t)stream));
  }
  return VNF_OK;
  API_GUARD_END
}

int vnf_augment_faces(const uint8_t* faces, int n_faces, int s, const int32_t* index, const vnf_aug_param* params, int n,
                      int t, void* x_out, int out_dtype, uint8_t* u8_out, void* stream) {
  API_GUARD_BEGIN
  if (n < 0) return fail(VNF_E_INVALID, "bad argument");
  if (s < 1 || s > 1024 || t < 1 || t > 1024) return fail(VNF_E_INVALID, "face size and target size must be 1..1024");
  if (out_dtype != VNF_F32 && out_dtype != VNF_BF16 && out_dtype != VNF_F16) return fail(VNF_E_INVALID, "bad out_dtype");
  if (n == 0) return VNF_OK;
  if (!faces || !params || n_faces < 1) return fail(VNF_E_INVALID, "faces and params must not be NULL");
  if (!index && n != n_faces) return fail(VNF_E_INVALID, "without an index there is one parameter set per face");
  for (int n0 = 0; n0 < n; n0 += 32768) {
    const int nn = n - n0 < 32768 ? n - n0 : 32768;
    // without an index row r reads face r: the chunk's faces start at n0
    VNF_HIP(launch_augment_faces(index ? faces : faces + (size_t)n0 * s * s * 3, index ? n_faces : nn, s,
                                 index ? index + n0 : nullptr, params + n0, nn, t,
                                 x_out ? (char*)x_out + (size_t)n0 * 3 * t * t * dtype_size(out_dtype) : nullptr, out_dtype,
                                 u8_out ? u8_out + (size_t)n0 * t * t * 3 : nullptr, (hipStream_t)stream));
  }
  return VNF_OK;
  API_GUARD_END
}

int vnf_softmax_topk(const float* logits, int n, int c, int k, int32_t* idx, float* prob, void* stream) {
  API_GUARD_BEGIN
  if (n < 0 || c < 1 || (n > 0 && (!logits || !idx || !prob))) return fail(VNF_E_INVALID, "bad argument");
  if (k < 1 || k > 16 || k > c) return fail(VNF_E_INVALID, "k must be 1..16 and <= c");
  VNF_HIP(launch_softmax_topk(logits, n, c, k, idx, prob, (hipStream_t)stream));
  return VNF_OK;
  API_GUARD_END
}

int vnf_maxpool3s2p1(const void* x, int dtype, int planar, int n, int h, int w, int c, void* y, void* stream) {
  API_GUARD_BEGIN
  if (n < 0 || h < 1 || w < 1 || c < 1 || (n > 0 && (!x || !y))) return fail(VNF_E_INVALID, "bad argument");
  if (dtype != VNF_F32 && dtype != VNF_BF16 && dtype != VNF_F16 && dtype != VNF_F16X2) return fail(VNF_E_INVALID, "bad dtype");
  const int dt = dtype == VNF_F16X2 ? (planar ? F16P : F16X2) : dtype;
  if (c % dtype_chan_align(dt)) return fail(VNF_E_INVALID, "channel count is not a multiple of the layout's 16-byte unit");
  const PoolWindow win = {3, 1, false};
  if ((size_t)n * pool_out_size(h, win) * pool_out_size(w, win) * (size_t)c >= ((size_t)1 << 31)) return fail(VNF_E_CAPACITY, "tensor too large");
  VNF_HIP(launch_maxpool(x, c, y, c, dt, n, h, w, c, win, (hipStream_t)stream));
  return VNF_OK;
  API_GUARD_END
}

int vnf_se_block(const void* t, const void* res, int dtype, int planar, int n, int h, int w, int c, const float* w1, const float* b1,
                 float slope_se, const float* w2, const float* b2, float slope_out, void* y, void* stream) {
  API_GUARD_BEGIN
  if (n < 0 || h < 1 || w < 1 || c < 1 || (n > 0 && (!t || !res || !y)) || !w1 || !b1 || !w2 || !b2) return fail(VNF_E_INVALID, "bad argument");
  if (dtype != VNF_F32 && dtype != VNF_BF16 && dtype != VNF_F16 && dtype != VNF_F16X2) return fail(VNF_E_INVALID, "bad dtype");
  if (dtype == VNF_F16X2 && !planar) return fail(VNF_E_INVALID, "vnf_se_block: split-f16 tensors in the planar layout only");
  const int dt = dtype == VNF_F16X2 ? F16P : dtype;
  if (c % 16 || c > 1024) return fail(VNF_E_INVALID, "vnf_se_block: c must be a multiple of 16, at most 1024");
  if ((size_t)h * w * (size_t)c >= ((size_t)1 << 31) || n > 65535) return fail(VNF_E_CAPACITY, "tensor too large");
  const int slices = se_slices(dt, h * w, c);
  if (slices < 1) return fail(VNF_E_INVALID, "vnf_se_block: unsupported shape");
  if (n == 0) return VNF_OK;
  hipStream_t s = (hipStream_t)stream;
  float* part = nullptr;
  VNF_HIP(hipMalloc(&part, (size_t)n * slices * c * 4));
  hipError_t err = launch_se_block(t, res, y, dt, n, h * w, c, SeWeights{w1, b1, w2, b2, slope_se, slope_out}, part, (size_t)slices * c, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);   // the scratch is freed here
  (void)hipFree(part);
  if (err != hipSuccess) return fail(VNF_E_HIP, hipGetErrorString(err));
  return VNF_OK;
  API_GUARD_END
}

}  // extern "C"
