/*
 * vnface.h -- C ABI of libvnface.so: the MI355X (gfx950) detect -> align -> embed -> classify
 * hot path of votnhan/VN_celeb_face_recognition, written from scratch in HIP.
 *
 * Each entry point replaces one reference interface (file:line under /root/reference):
 *
 *   vnf_encoder_create / vnf_embed   models/inception_resnet_v1.py:202,272-303
 *                                    (InceptionResnetV1.__init__ / forward) and
 *                                    models/iresnet_encoder.py:139-159,194-196 (iresnet100)
 *   vnf_mlp_create / vnf_classify    models/mlp_model.py:5-15 (MLPModel) +
 *                                    demo_image.py:113-137 (argmax / exp / threshold part of
 *                                    identify_person)
 *   vnf_mtcnn_create / vnf_mtcnn_detect
 *                                    models/mtcnn.py:200-227,318-361,511-513 (MTCNN.__init__,
 *                                    detect, inference) and
 *                                    models/mtcnn_utils/detect_face.py:25-185 (detect_face)
 *   vnf_align                        demo_image.py:174-199,236-239,283-295 +
 *                                    align_face.py:51-57 (crop, move landmarks, Umeyama,
 *                                    cv2.warpAffine) + data_loader/__init__.py:27-34,52-56
 *                                    (transforms_default, fused)
 *   vnf_emotion_create / vnf_emotion_forward
 *                                    models/resnet_2_branch.py:12-89 (ResNet2Branch, resnet_2branch_50)
 *   vnf_emotion_prep                 data_loader/__init__.py:74-81 (trans_emotion_inf)
 *   vnf_softmax_topk                 demo_image.py:37-47 (find_emotion, after the forward)
 *   vnf_emotion_recognize            demo_image.py:79-110 (recognize_emotion: transform, forward, top-k)
 *   vnf_augment_faces                data_loader/__init__.py:58-65 (transforms_facenet_aug) as
 *                                    trainer/online_aug_trainer.py:22-33 consumes it per batch
 *   vnf_extract_faces                models/mtcnn.py:458-509 (MTCNN.extract) +
 *                                    models/mtcnn_utils/detect_face.py:309-377 (crop_resize, extract_face)
 *   vnf_encoder_create_classifier / vnf_encoder_logprobs
 *                                    models/inception_resnet_v1.py:202-216,260-265,298-300 (classify=True) and
 *                                    models/iresnet_encoder.py:100-103,155-157,174-179 (n_classes)
 *   vnf_logits_eval                  trainer/classification_trainer.py:42-80 (_validate_epoch: nll_loss, accuracy,
 *                                    argmax / exp for the result rows) + trainer/base_trainer.py:177-200 (eval)
 *   vnf_encoder_features             what `logits` reads: models/inception_resnet_v1.py:296-298 (last_bn's output) and
 *                                    models/iresnet_encoder.py:153 (features)
 *   vnf_head_trainer_create / vnf_head_train_step
 *                                    trainer/classification_trainer.py:9-40 (one optimisation step) for
 *                                    models/iresnet_encoder.py:174-179 (freeze_weights: `logits` alone trains)
 *   vnf_jpeg_probe / vnf_jpeg_entropy_decode / vnf_jpeg_decode_frames
 *                                    cv2.VideoCapture.read as demo_video.py:78-110 calls it (a frame of a
 *                                    Motion-JPEG stream: bitstream walk on the host, pixels on the device)
 *   vnf_jpeg_huff_prepare / vnf_jpeg_huff_decode_frames
 *                                   (the Huffman pass of that decoder on the device: a compressed frame goes to HBM as it is)
 *   vnf_jpeg_encode_frames / vnf_jpeg_entropy_encode / vnf_overlay_draw
 *                                    demo_video.py:25-43,149-152 (cv2.rectangle / putText on the frame, cv2.imwrite,
 *                                    cv2.VideoWriter.write: the annotated frame is drawn and transformed on the
 *                                    device, the Huffman pass and the container stay on the host)
 *   vnf_overlay_draw_text            demo_image.py:161-171 (draw_emotions: cv2.putText per tag line) on frames in
 *                                    device memory, from a glyph atlas
 *
 * Conventions
 *   - every function returns 0 on success or a negative VNF_E_* code and never throws;
 *     vnf_last_error() returns a thread-local message for the last failure;
 *   - the caller owns all input/output buffers; the library owns handles, packed weights and
 *     workspaces (allocated at create time, sized by max_batch; nothing is allocated on the
 *     launch path -- the one exception is documented at vnf_encoder_set_contexts);
 *   - a handle is bound to the device that was current at create time and is NOT thread-safe
 *     (one host thread per GPU / rank);
 *   - all work is enqueued on the caller's hipStream_t (passed as void*); calls do not
 *     synchronise unless stated;
 *   - weights are handed over as host fp32 arrays keyed by their reference state_dict names
 *     (the Python side takes them from torch.load(...); a C caller fills the same table).
 */
#ifndef VNFACE_H
#define VNFACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VNF_OK 0
#define VNF_E_INVALID (-1)   /* bad argument / shape */
#define VNF_E_MISSING (-2)   /* a required weight tensor is absent */
#define VNF_E_HIP (-3)       /* HIP runtime error */
#define VNF_E_CAPACITY (-4)  /* batch / candidate count exceeds the handle's capacity */

/* element types */
#define VNF_F32 0
#define VNF_BF16 1
#define VNF_F16 2
#define VNF_I64 3
#define VNF_U8 4
#define VNF_F16X2 5 /* compute dtype only: fp32 values kept as (hi, lo) pairs of halves (split-f16) */

/* encoder architectures */
#define VNF_ARCH_IRV1 0   /* InceptionResnetV1, 160x160 input, L2-normalised 512-d output */
#define VNF_ARCH_IR100 1  /* IResNet-100 (ArcFace), 112x112 input, 512-d BN1d features */
#define VNF_ARCH_RN50_2B 2 /* ResNet-50 with class + projection heads (emotions), 224x224 input: vnf_emotion_create only */
#define VNF_ARCH_SEIR101 3 /* SE-IR ResNet-101 (resnet_encoder.py resnet101(use_se=True)), 112x112 input, L2-normalised 512-d output */

typedef struct vnf_handle_s* vnf_handle;

typedef struct {
  const char* name;  /* reference state_dict key, e.g. "repeat_1.0.branch0.conv.weight" */
  const void* data;  /* host pointer, contiguous */
  int32_t dtype;     /* VNF_F32 (VNF_I64 entries such as num_batches_tracked are ignored) */
  int32_t ndim;
  int64_t shape[4];
} vnf_tensor_desc;

/* library / device ------------------------------------------------------------------------- */
int vnf_init(int device_ordinal);          /* hipSetDevice + capability check (gfx950) */
const char* vnf_last_error(void);
const char* vnf_version(void);
int vnf_destroy(vnf_handle h);

/* encoders --------------------------------------------------------------------------------- */
/* compute_dtype: VNF_BF16 | VNF_F16 (MFMA 16x16x32 on 16-bit storage, fp32 accumulate);
 * VNF_F16X2 (split-f16: every weight and activation is an (hi, lo) pair of halves, products
 * expanded on the same 16-bit MFMA -- meets the <=1e-4 embedding gate at several times the
 * rate of the exact path); VNF_F32 (exact-f32 MFMA 16x16x4, bit-for-bit an fp32 fma chain). */
int vnf_encoder_create(int arch, const vnf_tensor_desc* weights, int n_weights, int compute_dtype,
                       int max_batch, vnf_handle* out);
/* x: device pointer, (N,3,S,S) NCHW, already normalised, dtype VNF_F32 | VNF_BF16 | VNF_F16.
 * emb_out: device pointer, (N,512) fp32. */
int vnf_embed(vnf_handle h, const void* x, int n, int x_dtype, float* emb_out, void* stream);
/* debugging / staged parity: copy an internal NHWC activation to a host fp32 NCHW array.
 * Synchronises the stream.  name is a reference module name ("conv2d_4b", "repeat_2", ...). */
int vnf_encoder_tap(vnf_handle h, const char* name, int n, float* host_out, int64_t capacity,
                    int64_t shape_out[4]);
/* vnf_embed with per-launch device timing (HIP events between ops; synchronises).  Writes a
 * text table (one line per plan op: shape, ms, TFLOP/s) into report. */
int vnf_encoder_profile(vnf_handle h, const void* x, int n, int x_dtype, float* emb_out, void* stream,
                        char* report, int64_t capacity);
/* FLOPs of one image through the loaded encoder as the kernels execute it (padded K / channels
 * included) and as the algorithm defines it; used by bench.py for the roofline line. */
int vnf_encoder_flops(vnf_handle h, double* algorithmic, double* executed);

/* vnf_embed cuts batches of >= 192 images over two internal HIP streams (one half each) to hide the small
 * layers' launch latencies.  A caller that already runs other work beside the encoder (the pipeline's detection
 * stream) sets 1: the forks then only take turns with that work.  Default 4 = the library decides. */
int vnf_encoder_set_streams(vnf_handle h, int max_streams);

/* Throughput mode for streams of independent batches (find_embedding.py's directory walk, the benchmark loop):
 * consecutive vnf_embed calls rotate over n (1..4) private activation-buffer sets, so calls the caller issues on
 * DIFFERENT streams overlap on the GPU; a set is re-used only after the event recorded at its previous use.
 * Each call stays ordered on the stream it was given.  Extra sets are allocated at first use (~2 GB for IRv1 at
 * max_batch 256).  Default 1. */
int vnf_encoder_set_contexts(vnf_handle h, int n);

/* encoders with their own classification head ----------------------------------------------- */
/* InceptionResnetV1(classify=True, num_classes=C) (inception_resnet_v1.py:202-216,260-265,298-300) and
 * iresnet100(n_classes=C) (iresnet_encoder.py:100-103,155-157): vnf_encoder_create plus the `logits` layer, so weights
 * must also hold logits.weight (num_classes,512) and logits.bias (num_classes); VNF_E_MISSING names the absent one.
 * (vnf_encoder_create ignores logits.* and builds no head.)  The head reads the fp32 features the plan leaves before its
 * last op -- last_bn's output before the L2 normalisation for IRv1, `features` for IR-100 -- and is one exact-f32
 * linear layer in every compute_dtype.  Everything else about the handle is as vnf_encoder_create makes it: vnf_embed
 * returns the same embeddings.  VNF_ARCH_SEIR101 is refused (VNF_E_INVALID): resnet_encoder.py has no `logits` layer. */
int vnf_encoder_create_classifier(int arch, const vnf_tensor_desc* weights, int n_weights, int compute_dtype,
                                  int max_batch, int num_classes, vnf_handle* out);
/* forward() of a classify model (inception_resnet_v1.py:298-300 F.log_softmax, iresnet_encoder.py:155-157): the plan,
 * the head, then vnf_logits_eval's row kernel, enqueued on `stream` with no host synchronisation.  x as for vnf_embed.
 * logp_out: device (N,num_classes) fp32; amax_out: device (N) int32; prob_out: device (N) fp32; each may be NULL.
 * N > max_batch: VNF_E_CAPACITY; a handle without a head: VNF_E_INVALID; N == 0: no-op. */
int vnf_encoder_logprobs(vnf_handle h, const void* x, int n, int x_dtype, float* logp_out, int32_t* amax_out,
                         float* prob_out, void* stream);
/* The fp32 (N,512) rows the handle's `logits` layer reads (or would read: the handle need not have a head): last_bn's
 * output before the L2 normalisation (InceptionResnetV1), `features` (IResNet-100).  x as for vnf_embed; feat_out: device
 * (N,512) fp32, written on `stream` with no host synchronisation.  N > max_batch: VNF_E_CAPACITY; the emotion handle:
 * VNF_E_INVALID; N == 0: no-op. */
int vnf_encoder_features(vnf_handle h, const void* x, int n, int x_dtype, float* feat_out, void* stream);
/* What a validation step does with a batch of logits (trainer/classification_trainer.py:42-80, losses/metrics.py:3-7):
 * logits device (n,c) fp32 with row stride ld >= c; target device (n) int64, may be NULL when nll, hit and sums are.
 * Outputs, all device, each may be NULL:
 *   logp (n,c)  log_softmax over the row (max-subtracted)      amax (n) int32  first index of the row maximum
 *   prob (n)    exp(logp[amax])                                nll (n)         -logp[target]
 *   hit (n) int32  amax == target                              sums (2)        {sum nll, sum hit}
 * sums are added in index order by a second launch, without float atomics: the same bits on every run, equal to the
 * fp32 sum of the nll / hit rows taken one after the other.  The call cannot see the targets: one outside [0, c) is
 * never used as an index, its row gets nll = +inf and hit = 0 (the host layer checks targets before it uploads them).
 * n == 0: no-op.  No workspace, nothing allocated, no synchronisation. */
int vnf_logits_eval(const float* logits, int n, int c, int ld, const int64_t* target, float* logp, int32_t* amax,
                    float* prob, float* nll, int32_t* hit, float* sums, void* stream);

/* emotion network --------------------------------------------------------------------------- */
/* models/resnet_2_branch.py:12-89: ResNet-50 (Bottleneck 3-4-6-3) on 224x224 inputs with two linear heads, fc
 * (2048 -> num_classes) and proj (2048 -> num_projections).  weights: the reference state_dict (conv1, bn1,
 * layer1..4, fc, proj; a DataParallel "module." prefix is stripped by the caller).  compute_dtype as for the
 * encoders.  The handle is an encoder handle: vnf_encoder_tap ("stem", "maxpool", "layer1".."layer4", "avgpool"),
 * vnf_encoder_profile (its emb_out is the (N,num_classes) class head), vnf_encoder_flops and
 * vnf_encoder_set_streams work on it; vnf_embed and vnf_encoder_set_contexts refuse it. */
int vnf_emotion_create(const vnf_tensor_desc* weights, int n_weights, int num_classes, int num_projections,
                       int compute_dtype, int max_batch, vnf_handle* out);
/* ResNet2Branch.forward (resnet_2_branch.py:55-70).  x: device (N,3,224,224) NCHW, already normalised, dtype
 * VNF_F32 | VNF_BF16 | VNF_F16.  cls_out: device (N,num_classes) fp32, proj_out: device (N,num_projections) fp32;
 * either may be NULL.  N > max_batch: VNF_E_CAPACITY; N == 0: no-op. */
int vnf_emotion_forward(vnf_handle h, const void* x, int n, int x_dtype, float* cls_out, float* proj_out,
                        void* stream);
/* recognize_emotion's device part (demo_image.py:79-110): aligned faces -> trans_emotion_inf -> network -> top-k in
 * one enqueue, nothing returns to the host in between.  faces_u8: device (N,S,S,3) RGB bytes, S <= 224; k in 1..16,
 * k <= num_classes.  idx_out: device (N,k) int32, prob_out: device (N,k) fp32 (see vnf_softmax_topk); cls_out:
 * device (N,num_classes) fp32 logits, may be NULL. */
int vnf_emotion_recognize(vnf_handle h, const uint8_t* faces_u8, int n, int s, int k, int32_t* idx_out,
                          float* prob_out, float* cls_out, void* stream);
/* trans_emotion_inf (data_loader/__init__.py:74-81) for square faces: Resize(224) with Pillow's bilinear resampling
 * (byte-exact: two 8-bit passes, 22-bit fixed-point coefficients), ToTensor, Normalize(ImageNet mean / std).
 * faces_u8: device (N,S,S,3), S <= 224; x_out: device (N,3,224,224) of out_dtype VNF_F32 | VNF_BF16 | VNF_F16. */
int vnf_emotion_prep(const uint8_t* faces_u8, int n, int s, void* x_out, int out_dtype, void* stream);
/* find_emotion after the forward (demo_image.py:41-47): per row of logits (N,C) fp32 the indices of the k largest
 * in descending order and their softmax values.  Exact ties come out lower index first (numpy's argsort leaves
 * their order undefined).  k in 1..16; k > C: VNF_E_INVALID.  idx: device (N,k) int32, prob: device (N,k) fp32. */
int vnf_softmax_topk(const float* logits, int n, int c, int k, int32_t* idx, float* prob, void* stream);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (resnet_2_branch.py:21) on its own, for staged parity of the
 * plan's pool: x device NHWC (N,H,W,C) -> y device NHWC (N,(H-1)/2+1,(W-1)/2+1,C) in one of the plans' storage
 * layouts: dtype VNF_F32 | VNF_BF16 | VNF_F16 (C % 4 / 8 / 8 == 0) or VNF_F16X2 (4-byte (hi, lo) pairs, C % 4 == 0;
 * planar != 0: 8-channel units [8 hi][8 lo], C % 8 == 0, what the encoders keep).  Padding compares as -inf. */
int vnf_maxpool3s2p1(const void* x, int dtype, int planar, int n, int h, int w, int c, void* y, void* stream);

/* The tail of an IRBlock of the SE-IR ResNet-101 (resnet_encoder.py:98-113,142-149) on its own, for parity of the
 * plan's squeeze-and-excitation kernels at their own shapes:
 *     y = prelu(t * gate + res, slope_out),   gate = sigmoid(w2 . prelu(w1 . mean_hw(t) + b1, slope_se) + b2)
 * t, res, y: device NHWC (N,H,W,C) in one of the encoders' storage layouts (dtype VNF_F32 | VNF_BF16 | VNF_F16, or
 * VNF_F16X2 with planar != 0: 8-channel units [8 hi][8 lo]); w1 (C/16,C), b1 (C/16), w2 (C,C/16), b2 (C): device fp32;
 * C % 16 == 0, C <= 1024.  Sums and the gate are fp32, the result is rounded once to the storage type.  The call is
 * bitwise repeatable, an image's result does not depend on N, and it returns after the work on `stream` is done. */
int vnf_se_block(const void* t, const void* res, int dtype, int planar, int n, int h, int w, int c, const float* w1,
                 const float* b1, float slope_se, const float* w2, const float* b2, float slope_out, void* y, void* stream);

/* classifier ------------------------------------------------------------------------------- */
int vnf_mlp_create(const vnf_tensor_desc* weights, int n_weights, int input_dim, int num_classes,
                   int max_batch, vnf_handle* out);
/* emb: device (F,input_dim) fp32.  logp_out: device (F,C) fp32 log-probabilities (may be NULL).
 * argmax_out: device (F,) int32; prob_out: device (F,) fp32 = exp(logp[argmax]) (may be NULL). */
int vnf_classify(vnf_handle h, const float* emb, int f, float* logp_out, int32_t* argmax_out,
                 float* prob_out, void* stream);

/* classifier training --------------------------------------------------- */
/* One optimisation step of trainer/classification_trainer.py:13-21 for models/mlp_model.py with
 * torch.optim.Adam semantics (coupled weight decay, no amsgrad): weights = the four MLPModel state_dict
 * tensors (initial values), fp32 end to end.  The handle owns parameters, gradients and Adam moments. */
int vnf_mlp_trainer_create(const vnf_tensor_desc* weights, int n_weights, int input_dim, int num_classes,
                           int max_batch, float beta1, float beta2, float eps, float weight_decay,
                           vnf_handle* out);
/* emb: device (b,input_dim) fp32; target: device (b,) int64; dropout_mask: device (b,2048) fp32 holding
 * F.dropout's factor per hidden unit (0 or 1/(1-p); NULL = no dropout; ignored when train == 0).
 * train != 0: forward, NLL loss, backward, Adam step with learning rate lr; train == 0: forward + loss only
 * (classification_trainer.py:48-56).  loss_out: device fp32 scalar (mean NLL of the batch); hits_out: device
 * int32 scalar (argmax == target count, losses/metrics.py:3-7).  Enqueued on `stream`, no synchronisation. */
int vnf_mlp_train_step(vnf_handle h, const float* emb, const int64_t* target, int b,
                       const float* dropout_mask, float lr, int train, float* loss_out,
                       int32_t* hits_out, void* stream);
/* checkpoint access of either trainer handle (trainer/base_trainer.py:83-105): name = a state_dict key of what the handle
 * trains (the four of MLPModel; logits.weight | logits.bias), kind 0 = parameter, 1 = Adam exp_avg, 2 = Adam exp_avg_sq;
 * host fp32 arrays of exactly numel elements.  Synchronise. */
int vnf_trainer_get(vnf_handle h, const char* name, int kind, float* host_out, int64_t numel);
int vnf_trainer_set(vnf_handle h, const char* name, int kind, const float* host_in, int64_t numel);
int vnf_trainer_step_count(vnf_handle h, int64_t* step_io, int set);  /* Adam's step counter */

/* training of a frozen encoder's `logits` layer ---------------------------- */
/* One optimisation step of trainer/classification_trainer.py:13-21 for nn.Linear(512, num_classes) + log_softmax on
 * precomputed features (vnf_encoder_features), torch.optim.Adam semantics (coupled weight decay, no amsgrad), fp32 end
 * to end.  weights: logits.weight (num_classes,512) and logits.bias (num_classes) (initial values; other entries are
 * ignored).  The handle owns the two parameters and their Adam moments; the gradient of the weight never exists in memory. */
int vnf_head_trainer_create(const vnf_tensor_desc* weights, int n_weights, int num_classes, int max_batch,
                            float beta1, float beta2, float eps, float weight_decay, vnf_handle* out);
/* feat: device (b,512) fp32; target: device (b,) int64 (a label outside [0,num_classes) is never used as an index: the
 * loss becomes NaN).  train != 0: forward, NLL loss, backward, Adam step with learning rate lr (four launches);
 * train == 0: forward + loss only, parameters, moments and step count untouched.  loss_out: device fp32 scalar (mean
 * NLL of the batch, rows summed in index order); hits_out: device int32 scalar (first argmax == target count).
 * Bitwise repeatable.  b > max_batch: VNF_E_CAPACITY.  Enqueued on `stream`, no synchronisation. */
int vnf_head_train_step(vnf_handle h, const float* feat, const int64_t* target, int b, float lr, int train,
                        float* loss_out, int32_t* hits_out, void* stream);

/* training-time augmentation --------------------------------------------- */
/* transforms_facenet_aug (data_loader/__init__.py:58-65) for the images VNCelebDataset serves
 * (data_loader/vn_celeb_dataset.py:12-47) to AugClassificationTrainer (trainer/online_aug_trainer.py:22-33): the random
 * state of one sample, drawn by the host.  m: the matrix Pillow's Image.rotate builds for the drawn angle (output pixel
 * centre -> input position); i, j: row and column of the crop origin in the zero-padded image; flip: mirror the crop;
 * pad: the zero border per side, 2 + max(0, T - (S + 4)) for RandomCrop(T, padding=2, pad_if_needed=True). */
typedef struct {
  double m[6];
  int32_t i, j, flip, pad;
} vnf_aug_param;

/* One launch: output row r = face index[r] (index NULL: face r, and then n == n_faces) rotated with Pillow's bicubic
 * resampling (byte-exact: double arithmetic in Pillow's operation order, truncation to u8), zero-padded, cropped at
 * (i, j), mirrored, then np.float32, (v - 127.5) / 128 and CHW (fix_std, to_tensor; data_loader/__init__.py:27-34).
 * With m the identity, i = j = pad and flip 0 this is transforms_default (:52-56).
 *   faces: device (n_faces,S,S,3) u8, the resident data set; index: device (n) int32 or NULL; params: device (n);
 *   x_out: device (n,3,T,T) of out_dtype VNF_F32 | VNF_BF16 | VNF_F16, may be NULL;
 *   u8_out: device (n,T,T,3) augmented bytes, may be NULL.
 * No workspace, nothing allocated, no synchronisation.  n == 0: no-op.  S or T outside 1..1024, a NULL faces / params
 * with n > 0, n_faces < 1, index NULL with n != n_faces or a bad out_dtype: VNF_E_INVALID.  index and params live in device memory, so the call cannot see their values: a row
 * whose index is outside 0..n_faces-1 or whose crop origin is outside [0, S + 2 pad - T] is written as the fill
 * (byte 0) and reads nothing; the host layer checks both before it uploads them. */
int vnf_augment_faces(const uint8_t* faces, int n_faces, int s, const int32_t* index, const vnf_aug_param* params,
                      int n, int t, void* x_out, int out_dtype, uint8_t* u8_out, void* stream);

/* detector --------------------------------------------------------------------------------- */
typedef struct {
  int32_t min_face_size;   /* mtcnn.py:201 */
  float thresholds[3];     /* mtcnn.py:202 */
  float factor;            /* mtcnn.py:202 */
  int32_t select_largest;  /* mtcnn.py:203: order boxes by area, descending */
  int32_t max_batch;       /* frames per call */
  int32_t max_height, max_width;
  int32_t max_candidates;  /* rows per frame of the stage-2 / stage-3 candidate tables (survivors of the cross-scale NMS,
                            * of the R-Net filter and of the O-Net filter): 0 or anything <= 2048 = 2048.  The reference
                            * has no cap (detect_face.py:79-93,203-218).  Here stage 1 is sized by the pyramid itself
                            * (every P-Net cell has a slot: it cannot overflow) and every NMS moves from LDS to
                            * global-memory scratch when a list outgrows the LDS tables, so this is the ONLY bound: a
                            * frame with more stage-1 survivors fails the call with VNF_E_CAPACITY (never a silent
                            * truncation) and the host layer re-creates the handle with a larger table and retries */
} vnf_mtcnn_cfg;

int vnf_mtcnn_create(const vnf_tensor_desc* pnet, int n_pnet, const vnf_tensor_desc* rnet, int n_rnet,
                     const vnf_tensor_desc* onet, int n_onet, const vnf_mtcnn_cfg* cfg, vnf_handle* out);
/* frames: device (B,H,W,3) uint8 RGB.  Results stay on the device for vnf_align and are also
 * copied to the caller's host arrays.  The reference synchronises at both stage boundaries to shape its tensors
 * (detect_face.py:96-146); this call synchronises the stream ONCE, at the end, for the results: stages 2 and 3 are
 * launched with the previous call's candidate counts (plus head room) as launch bounds, every kernel reads the true
 * counts from device memory, and the final read-back tells whether the bounds covered them.  If not -- or on the first
 * call of a frame size -- stage 1's counts are read and stages 2 / 3 run with exact bounds (one more synchronisation);
 * the results are identical either way (VNF_MTCNN_SPEC=0 always takes the second path):
 *   counts[B]            faces per frame
 *   boxes[max_out*4]     x1,y1,x2,y2 fp32, frames concatenated in order
 *   probs[max_out]
 *   points[max_out*10]   (5,2) landmarks
 * n_out receives the total number of faces; VNF_E_CAPACITY if it exceeds max_out. */
int vnf_mtcnn_detect(vnf_handle h, const uint8_t* frames, int b, int height, int width,
                     int32_t* counts, float* boxes, float* probs, float* points, int max_out,
                     int32_t* n_out, void* stream);

/* Device-resident copy of the LAST vnf_mtcnn_detect on this handle (same order as its host arrays): writes up to
 * max_out faces into caller-owned device buffers on `stream` (any of the four may be NULL).  This is what lets
 * vnf_align consume the detections without the host round trip of demo_image.py:283-295 (boxes and landmarks go
 * detector -> host -> OpenCV there).  Valid until the next vnf_mtcnn_detect on the handle. */
int vnf_mtcnn_results_device(vnf_handle h, int32_t* frame_idx, float* boxes, float* probs, float* points,
                             int max_out, void* stream);

/* measurement hook (bench.py roofline): one detection with HIP events between the cascade's stages on
 * `stream`; report receives one text line per stage, "name milliseconds algorithmic_bytes" (pyramid,
 * pnet_conv1_pool, pnet_conv2, pnet_conv3_heads, nms_stage1, host_sync_1, crop_resize_24, rnet, ...).
 * Synchronises. */
int vnf_mtcnn_stage_times(vnf_handle h, const uint8_t* frames, int b, int height, int width,
                          char* report, int64_t capacity, void* stream);

/* staged parity hook: runs the cascade on frame 0 and copies one pyramid level (3,Hs,Ws), its
 * P-Net face-probability map (oh,ow) and regression map (4,oh,ow) to host arrays.
 * dims receives {Hs, Ws, oh, ow}.  Synchronises. */
int vnf_mtcnn_debug_pnet(vnf_handle h, const uint8_t* frames, int height, int width, int level,
                         float* level_out, float* prob_out, float* reg_out, int32_t dims[4], void* stream);

/* staged parity hook for the O-stage decode alone (detect_face.py:148-169, mtcnn.py:334-340): threshold,
 * landmark decode, bbreg, "Min" NMS and the final area ordering on a caller-made single-frame table --
 * boxes (n,4) host fp32 (before bbreg), onet_out (n,15) host fp32 [prob, reg0..3, lm_x0..4, lm_y0..4];
 * fin_out (max_out,15) host rows [x1,y1,x2,y2,score, (x,y) x 5].  Lets a test inject exactly tied scores.
 * Synchronises. */
int vnf_mtcnn_debug_stage3(vnf_handle h, const float* boxes, const float* onet_out, int n, float* fin_out,
                           int max_out, int32_t* n_out, void* stream);

/* staged parity hook for R-Net (net 2) or O-Net (net 3) on their own (mtcnn.py:84-99 / 138-157 behind
 * detect_face.py:108-117 / 137-146): the caller's rectangles become the candidate table of stage 2 / stage 3 and the
 * cascade's own launch sequence runs on it -- prefix offsets, then per chunk of the dense batch the crop kernel, the
 * fused front (conv1 + pool1), the fused mid (conv2 + pool2) where the handle has it, the plan and the heads scatter.
 *   frames      device (b,H,W,3) uint8, as for vnf_mtcnn_detect
 *   rects       host int32 (total,4): y, ey, x, ex as pad() returns them (detect_face.py:277-289: 1-based, inclusive),
 *               frame 0's rows first; every value inside the frame (VNF_E_INVALID otherwise)
 *   counts      host int32 (b): rectangles per frame, each at most the rows per frame of the handle's tables
 *               (vnf_mtcnn_cfg.max_candidates) -- VNF_E_CAPACITY beyond, as for b above max_batch
 *   table_out   host fp32 (total,nf), frame-major: nf = 5 [prob, reg0..3] for R-Net, 15 [prob, reg0..3, lm0..9] for
 *               O-Net, the rows stage2_post / stage3_post read
 *   status_out  the kernels' status word (0: nothing flagged)
 * Reads no environment variable, allocates nothing that outlives the call, forgets the speculative launch sizes and the
 * last detection's results.  Synchronises. */
int vnf_mtcnn_debug_net(vnf_handle h, int net, const uint8_t* frames, int b, int height, int width,
                        const int32_t* rects, const int32_t* counts, float* table_out, int32_t* status_out, void* stream);

/* One buffer of the LAST chunk the previous vnf_mtcnn_debug_net on this handle and net processed, as its raw 32-bit
 * words: the n_last x H x W x C NHWC rows, no row padding.  dims receives {n_last, H, W, C, split, c0}: split 1 = a
 * word is a split-f16 (hi, lo) pair (hi in the low half), 0 = an fp32 value (the crops in every form); c0 = dense
 * index (frames concatenated) of the chunk's first candidate.  Names: crops (C = 4: RGB + 0), pool1, conv2, pool2,
 * conv3, pool3 and conv4 (O-Net), dense, heads.  raw_out NULL: dims only.  VNF_E_INVALID for an unknown name, without a
 * preceding debug call on that net, and for a buffer the handle's form never writes (conv2 under the fused mid
 * kernel); VNF_E_CAPACITY if the rows exceed capacity_bytes. */
int vnf_mtcnn_debug_net_tap(vnf_handle h, int net, const char* name, void* raw_out, int64_t capacity_bytes,
                            int32_t dims[6]);

/* RetinaFace detector (replaces /root/reference/models/retina_face.py:56-232, the mobilenet0.25 configuration of
 * cfg/detection/retina_face.json) ---------------------------------------------------------------------------------- */
typedef struct {
  int32_t height, width;  /* the exact frame size the handle serves (priors and the plan's buffers are sized for it;
                           * retina_face.py:180-183 rebuilds its PriorBox per image, here one handle per frame size) */
  int32_t max_batch;      /* frames per call */
  float conf_thres;       /* retina_face.py:191-195 (cfg 0.02) */
  int32_t topk_bf_nms;    /* :198-201 (cfg 5000) */
  float nms_thres;        /* :204-206 py_cpu_nms (cfg 0.4) */
  int32_t keep_top_k;     /* :209-210 (cfg 750; <= 768) */
  float vis_thres;        /* :213-216 (cfg 0.6) */
  int32_t compute_dtype;  /* VNF_F32 (0, default): the network on the exact-f32 MFMA; VNF_F16X2: split-f16 storage and
                           * products (~22 significant bits, ~15 % faster; scores move by up to ~3e-5) */
} vnf_retina_cfg;

/* weights: the RetinaFace state_dict (body.* / fpn.* / ssh{1,2,3}.* / ClassHead.* / BboxHead.* / LandmarkHead.*, without the
 * "module." prefix retina_face.py:117-127 strips), fp32 host arrays; BatchNorm is folded (eps 1e-5) at creation. */
int vnf_retina_create(const vnf_tensor_desc* weights, int n_weights, const vnf_retina_cfg* cfg, vnf_handle* out);
/* Same contract as vnf_mtcnn_detect: frames = device (B,H,W,3) uint8 RGB; per frame the rows that pass vis_thres in
 * descending score order.  VNF_E_CAPACITY when a frame has more than 16384 anchors above conf_thres or the total
 * exceeds max_out.  Synchronises the stream twice (counts, then rows). */
int vnf_retina_detect(vnf_handle h, const uint8_t* frames, int b, int height, int width,
                      int32_t* counts, float* boxes, float* probs, float* points, int max_out,
                      int32_t* n_out, void* stream);
int vnf_retina_results_device(vnf_handle h, int32_t* frame_idx, float* boxes, float* probs, float* points,
                              int max_out, void* stream);
/* staged parity hook: the raw head maps of pyramid level 0..2 of the last detection as a host (b,fh,fw,32) fp32
 * array, columns [class logits 2x2 | bbox 2x4 | landmarks 2x10]; dims receives {fh, fw}.  Synchronises. */
int vnf_retina_debug_heads(vnf_handle h, int level, int b, float* host_out, int64_t capacity, int32_t dims[2]);

/* alignment -------------------------------------------------------------------------------- */
/* For each of n faces: crop rectangle from its box (demo_image.py:179-182), landmarks moved by
 * the float box corner (236-239), Umeyama similarity landmarks -> template (align_face.py:52-54),
 * fixed-point bilinear warp into S x S (cv2.warpAffine, borderValue 0, the crop being the
 * source image), then optionally (x-127.5)/128 to NCHW.
 *   frames: device (B,H,W,3) u8; frame_idx: device (n,) int32; boxes: device (n,4) fp32;
 *   points: device (n,10) fp32; template5x2: host 10 floats.
 *   faces_u8: device (n,S,S,3) u8 or NULL; faces_norm: device (n,3,S,S) of norm_dtype or NULL. */
int vnf_align(const uint8_t* frames, int b, int height, int width, const int32_t* frame_idx,
              const float* boxes, const float* points, int n, const float* template5x2, int s,
              uint8_t* faces_u8, void* faces_norm, int norm_dtype, void* stream);

/* face extraction -------------------------------------------------------------------------- */
/* MTCNN.extract / extract_face (models/mtcnn.py:458-509, models/mtcnn_utils/detect_face.py:309-377, tensor path):
 * row r is the rectangle rects[r] = {frame, x1, y1, x2, y2} (pixels [y1,y2) x [x1,x2) of that frame; the margin
 * arithmetic of detect_face.py:358-368 is the caller's, detector.crop_rects) resampled to s x s as
 * interpolate(mode="area") does (detect_face.py:304-306,317-322: bin of output (oy,ox) = rows [oy*ch/s, ceil((oy+1)*ch/s)),
 * columns alike, also when up-sampling), truncated to a byte (.byte()): integer sums and one IEEE fp32 division.
 *   frames: device (B,H,W,3) u8; rects: device (n,5) int32;
 *   x_out: device (n,3,s,s) of out_dtype VNF_F32 | VNF_BF16 | VNF_F16 (the fp32 value rounded to nearest-even), may be
 *          NULL: float(byte) (detect_face.py:376), or (byte - 127.5) / 128 with standardize != 0 (mtcnn.py:516-518);
 *   u8_out: device (n,s,s,3) bytes, may be NULL.
 * One launch, no workspace, nothing allocated, no synchronisation.  n == 0: no-op.  s outside 1..1024, NULL frames or
 * rects with n > 0, a bad out_dtype or both outputs NULL: VNF_E_INVALID.  rects live in device memory, so the call
 * cannot see their values: a row whose frame index is outside 0..B-1, whose rectangle is empty or leaves the frame, or
 * whose bins reach 2^15 pixels ((ceil(ch/s)+1) * (ceil(cw/s)+1), the bound under which every correctly rounded
 * quotient truncates to the same byte) is written as zeros and reads nothing; the host layer checks all of it before it
 * uploads the table. */
int vnf_extract_faces(const uint8_t* frames, int b, int height, int width,
                      const int32_t* rects /* device (n,5): frame, x1, y1, x2, y2 */, int n, int s,
                      int standardize, void* x_out /* (n,3,s,s) */, int out_dtype /* VNF_F32|VNF_BF16|VNF_F16 */,
                      uint8_t* u8_out /* (n,s,s,3) */, void* stream);

/* JPEG video frames ------------------------------------------------------------------------ */
/* The reference reads its frames with cv2.VideoCapture.read (demo_video.py:78-110): a host decoder, one frame at a
 * time.  Here a baseline JPEG frame (a Motion-JPEG AVI chunk, a .jpg file) is split: the serial bitstream walk stays
 * on the host (vnf_jpeg_probe, vnf_jpeg_entropy_decode: plain C++, no HIP call, usable without a GPU, thread-safe,
 * one frame per call), everything after it -- dequantisation, 8x8 IDCT, chroma upsampling, YCbCr -> RGB -- runs on the
 * device (vnf_jpeg_decode_frames).  The arithmetic is libjpeg's public baseline path (islow IDCT, "fancy" triangle
 * upsampling, 16-bit fixed-point colour), all integer, so the bytes are those libjpeg / libjpeg-turbo produce. */
#define VNF_JPEG_NOT_TAKEN 1 /* the one positive status: a valid JPEG this decoder leaves to the host decoder */

/* sampling codes of a frame (luma factors; chroma is 1x1) */
#define VNF_JPEG_GRAY 0 /* one component */
#define VNF_JPEG_444 1  /* 1x1 */
#define VNF_JPEG_422 2  /* 2x1 */
#define VNF_JPEG_420 3  /* 2x2 */

typedef struct {
  int32_t width, height;
  int32_t components;       /* 1 or 3 */
  int32_t sampling;         /* VNF_JPEG_* */
  int32_t h[3], v[3];       /* sampling factors per component (1x1 for a single component) */
  int32_t restart_interval; /* MCUs between RSTn markers, 0: none */
  int32_t blocks_w[3], blocks_h[3]; /* 8x8 blocks per row / column of each component plane, MCU-padded */
  uint8_t quant[3][64];     /* the component's 8-bit quantisation table in natural (row-major) order */
  int64_t coef_count;       /* int16 coefficients of a frame: 64 * sum(blocks_w * blocks_h) */
} vnf_jpeg_info;

/* Walks the markers of data[0, len) up to the first scan (SOI; APPn / COM skipped; DQT, SOF0, DHT, DRI, SOS) and fills
 * *info.  VNF_OK: vnf_jpeg_entropy_decode takes this frame.  VNF_E_INVALID: not a JPEG / corrupt or truncated header.
 * VNF_JPEG_NOT_TAKEN: a JPEG outside this decoder -- any SOF but baseline SOF0, 12-bit samples, arithmetic coding,
 * 2 or 4 components, three components that are RGB (Adobe APP14 transform 0, ids 'R','G','B'), no DHT in the frame
 * (the abbreviated frames some cameras write), 16-bit quantisation tables, a scan that does not hold every component
 * (more than one scan), sampling other than 1x1 / 2x1 / 2x2 luma over 1x1 chroma. */
int vnf_jpeg_probe(const uint8_t* data, int64_t len, vnf_jpeg_info* info);
/* Huffman-decodes the one scan of a frame vnf_jpeg_probe accepted (info: what it filled, for the same bytes) into
 * coefs[0, info->coef_count): QUANTISED coefficients in natural order, 64 per block, the blocks of a component plane in
 * raster order (blocks_w per row), the planes one after another.  FF 00 stuffing, DC prediction and restart markers
 * (predictors reset, RSTn sequence checked) are undone here.  Every read is checked against len, every write against
 * capacity (in coefficients): VNF_E_CAPACITY when capacity < coef_count, VNF_E_INVALID for a truncated or
 * inconsistent stream or an info that does not belong to these bytes -- never a partial success (coefs then holds
 * unspecified values inside [0, capacity)).  A missing EOI after the last MCU is accepted. */
int vnf_jpeg_entropy_decode(const uint8_t* data, int64_t len, const vnf_jpeg_info* info, int16_t* coefs,
                            int64_t capacity);
/* bytes of device workspace vnf_jpeg_decode_frames needs for n frames of this geometry (the component planes between
 * its two launches), or a negative VNF_E_* code */
int64_t vnf_jpeg_workspace_bytes(int n, int width, int height, int sampling);
/* n frames of ONE geometry (width, height, sampling code), each with its own tables:
 *   coefs_dev: device (n, coef_count) int16 as vnf_jpeg_entropy_decode writes them; quant_dev: device (n,3,64) u8
 *   (vnf_jpeg_info.quant; rows 1..2 unused for VNF_JPEG_GRAY); frames_out: device (n,height,width,3) u8 RGB
 *   (R = G = B for VNF_JPEG_GRAY); workspace: device, 16-byte aligned.
 * Two launches (planes, then upsample + colour), nothing allocated, no synchronisation.  n == 0: no-op.
 * VNF_E_INVALID: n < 0, a NULL or misaligned pointer, width or height outside 1..65535, an unknown sampling code;
 * VNF_E_CAPACITY: workspace_bytes below vnf_jpeg_workspace_bytes(...). */
int vnf_jpeg_decode_frames(const int16_t* coefs_dev, const uint8_t* quant_dev, int n, int width, int height,
                           int sampling, uint8_t* frames_out, void* workspace, int64_t workspace_bytes, void* stream);

/* JPEG video frames, written --------------------------------------------------------------- */
/* The way out of the device: the reference draws on every frame with OpenCV and hands it to cv2.VideoWriter
 * (demo_video.py:25-43,149-152), one frame at a time on the host.  Here the annotated frame is drawn (vnf_overlay_draw),
 * colour-converted, down-sampled, DCT-transformed and quantised (vnf_jpeg_encode_frames) where it already lives; the
 * serial Huffman pass (vnf_jpeg_entropy_encode: plain C++, no HIP call, usable without a GPU, thread-safe, one frame per
 * call) writes the file.  The arithmetic is libjpeg's public baseline encoder (16-bit fixed-point colour, box
 * down-sampling with alternating bias, islow forward DCT, quantisation by division), all integer, so the coefficients --
 * and with the annex K Huffman tables the files -- are those libjpeg / libjpeg-turbo write without `optimize`. */

/* The annex K.1 tables scaled as libjpeg's jpeg_set_quality does (quality < 50: 5000 / quality, else 200 - 2 quality;
 * entry = (base * scale + 50) / 100 clamped to 1..255), natural (row-major) order.  Host only.  quality outside 1..100 or
 * a NULL pointer: VNF_E_INVALID. */
int vnf_jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);
/* What vnf_jpeg_probe fills for a width x height RGB frame written with this sampling and quality: factors, blocks_w/h
 * (MCU-padded), quant (rows 1 and 2 both the chroma table), coef_count, restart_interval 0.  Host only.  VNF_E_INVALID:
 * width or height outside 1..65535, quality outside 1..100, a sampling other than VNF_JPEG_444 / _422 / _420
 * (VNF_JPEG_GRAY is refused: frames are RGB). */
int vnf_jpeg_encode_info(int width, int height, int sampling, int quality, vnf_jpeg_info* out);
/* bytes of device workspace vnf_jpeg_encode_frames needs for n frames of this geometry (the component planes between
 * its two launches), or a negative VNF_E_* code */
int64_t vnf_jpeg_encode_workspace_bytes(int n, int width, int height, int sampling);
/* n frames of ONE geometry through colour conversion, down-sampling, forward DCT and quantisation with ONE pair of tables:
 *   frames_dev: device (n,height,width,3) u8 RGB; quant_dev: device (2,64) u8, luma then chroma, natural order, 8-byte
 *   aligned (a zero entry is read as 1); coefs_out: device (n, coef_count) int16, 16-byte aligned, in EXACTLY the layout
 *   vnf_jpeg_entropy_decode writes and vnf_jpeg_decode_frames reads: planes one after another, blocks in raster order,
 *   blocks_w per row, the dummy blocks that pad the luma plane to whole MCUs included (zero but for the DC libjpeg gives
 *   them); workspace: device, 16-byte aligned.
 * Two launches (planes, then DCT + quantisation), nothing allocated, no synchronisation.  n == 0: no-op.
 * VNF_E_INVALID: n < 0, a NULL or misaligned pointer, width or height outside 1..65535, a sampling other than
 * VNF_JPEG_444 / _422 / _420; VNF_E_CAPACITY: workspace_bytes below vnf_jpeg_encode_workspace_bytes(...). */
int vnf_jpeg_encode_frames(const uint8_t* frames_dev, int n, int width, int height, int sampling, const uint8_t* quant_dev,
                           int16_t* coefs_out, void* workspace, int64_t workspace_bytes, void* stream);
/* Huffman-encodes coefs[0, info->coef_count) (the layout above; info as vnf_jpeg_encode_info or vnf_jpeg_probe fill it:
 * three components, no restart interval, quant[1] == quant[2]) into a complete baseline JFIF file in out[0, capacity):
 * SOI, APP0, two DQT, SOF0, four DHT (the annex K.3 tables), SOS, one interleaved scan (FF bytes stuffed, the last byte
 * padded with 1-bits), EOI.  *len_out receives the file's length.  Host only, thread-safe, one frame per call.
 * VNF_E_CAPACITY: the file does not fit -- nothing was written outside [0, capacity) and *len_out is the length that
 * would have fitted; VNF_E_INVALID: a NULL pointer, an info outside the above, or a coefficient outside the baseline
 * range (an AC magnitude category above 10, a DC difference category above 11). */
int vnf_jpeg_entropy_encode(const int16_t* coefs, const vnf_jpeg_info* info, uint8_t* out, int64_t capacity,
                            int64_t* len_out);

/* The same Huffman pass on the device (csrc/jpeg_huff_device.hip): a second back end that writes the same files, so that
 * a frame's coefficients never cross to the host.  Sizes -> exclusive scan -> bit packing into a zeroed stream area ->
 * FF count -> scan -> byte emission with stuffing; kernel boundaries are the only synchronisation between workgroups,
 * and the result is bitwise repeatable. */
/* The bytes SOI .. end of the SOS header of the file vnf_jpeg_entropy_encode writes for *info (623 of them; this is the
 * code that call itself runs), into out[0, capacity); *len_out receives their count.  Host only, no HIP call.
 * VNF_E_INVALID: a NULL pointer or an info vnf_jpeg_entropy_encode refuses; VNF_E_CAPACITY: capacity below *len_out --
 * nothing was written outside [0, capacity). */
int vnf_jpeg_huff_header(const vnf_jpeg_info* info, uint8_t* out, int64_t capacity, int64_t* len_out);
/* bytes of device workspace vnf_jpeg_huff_encode_frames needs for n frames of *info with capacity_per_frame bytes of
 * output each (the stream areas hold min(capacity_per_frame, the longest possible scan) bytes), or a negative VNF_E_*
 * code (VNF_E_INVALID: n outside 0..65535, a negative capacity, an info vnf_jpeg_entropy_encode refuses, or a frame of
 * 1658 * blocks >= 2^32 bits: bit offsets are 32-bit) */
int64_t vnf_jpeg_huff_workspace_bytes(int n, const vnf_jpeg_info* info, int64_t capacity_per_frame);
/* n frames of ONE info: coefs_dev device (n, info->coef_count) int16 as vnf_jpeg_encode_frames writes them, 16-byte
 * aligned; header_dev: the bytes of vnf_jpeg_huff_header, on the device; out_dev: device (n, capacity_per_frame) u8;
 * lengths_dev: device (n) int64; status_dev: device (n) int32; workspace: device, 16-byte aligned.  Frame i's file is
 * out_dev[i * capacity_per_frame, + lengths_dev[i]) when status_dev[i] is VNF_OK; VNF_E_CAPACITY: the file does not fit
 * and lengths_dev[i] is the length that would (the number vnf_jpeg_entropy_encode reports); VNF_E_INVALID: a
 * coefficient outside the baseline range.  Bytes in [length, capacity) are unspecified; no byte at or past a frame's
 * capacity is written; a frame's status never affects another frame.  Enqueued on `stream` (one memset, six launches),
 * nothing allocated, no host synchronisation.  n == 0: no-op.
 * Returns VNF_E_INVALID: n outside 0..65535, a NULL or misaligned pointer, an info vnf_jpeg_entropy_encode refuses,
 * header_len other than vnf_jpeg_huff_header's; VNF_E_CAPACITY: workspace_bytes below
 * vnf_jpeg_huff_workspace_bytes(...); VNF_E_HIP: a launch error. */
int vnf_jpeg_huff_encode_frames(const int16_t* coefs_dev, int n, const vnf_jpeg_info* info, const uint8_t* header_dev,
                                int64_t header_len, uint8_t* out_dev, int64_t capacity_per_frame, int64_t* lengths_dev,
                                int32_t* status_dev, void* workspace, int64_t workspace_bytes, void* stream);

/* JPEG video frames, Huffman-decoded on the device ------------------------------------------ */
/* The Huffman pass of the frame DEcoder on the device (csrc/jpeg_huff_decode.hip): a second back end that writes the
 * coefficients vnf_jpeg_entropy_decode writes, so that a compressed frame crosses to HBM as it is and nothing
 * per-coefficient runs on the host.  The host PREPARES a frame (a memchr-speed pass: FF 00 unstuffed, the scan cut at its
 * RSTn markers, the decode tables laid out; no symbol decoded); the device decodes every segment in subsequences of
 * `subseq_bits` bits, one lane each, with the self-synchronising scheme of Weissenberger and Schmidt: speculate ->
 * synchronise (fixed points inside one workgroup, launch boundaries between workgroups) -> count -> scan -> write ->
 * DC prefix sums.  Kernel boundaries are the only synchronisation between workgroups, every loop is bounded by bit
 * counts, and the result is bitwise repeatable. */
/* The longest blob vnf_jpeg_huff_prepare writes for a file of len bytes whose probe gave *info (its restart interval
 * decides the number of segments), or VNF_E_INVALID for a NULL info or a negative len.  Host only. */
int64_t vnf_jpeg_huff_prepared_bound(int64_t len, const vnf_jpeg_info* info);
/* Prepares the one scan of a frame vnf_jpeg_probe accepted (info: what it filled, for the same bytes) into
 * out[0, capacity): one self-contained, position-independent blob -- a 64-byte header, the decode tables the scan's
 * components select with each component's selectors, a table of (offset, byte length) per segment, and the
 * entropy-coded bytes with FF 00 stuffing removed and fill bytes dropped, split at the RSTn markers (checked to come in
 * sequence, as vnf_jpeg_entropy_decode checks them; the scan ends at the first other marker or at len) into segments
 * that each start 16-byte aligned.  A scan without DRI is one segment.  *len_out receives the blob's length, a multiple
 * of 16.  Wherever the blob is copied to, its first byte must be 16-byte aligned.  Host only, no HIP call, thread-safe;
 * every read is checked against len, every write against capacity.  VNF_E_INVALID: a NULL pointer, a header
 * vnf_jpeg_probe does not accept or an info that does not belong to these bytes, a restart interval that does not end
 * with its RSTn; VNF_E_CAPACITY: the blob does not fit -- never a partial success (out then holds unspecified values
 * inside [0, capacity), *len_out is untouched). */
int vnf_jpeg_huff_prepare(const uint8_t* data, int64_t len, const vnf_jpeg_info* info, uint8_t* out, int64_t capacity,
                          int64_t* len_out);
/* bytes of device workspace vnf_jpeg_huff_decode_frames needs for n frames of *info's geometry whose blobs are at most
 * max_blob_bytes long, with this subseq_bits (0: the default, 1024), or a negative VNF_E_* code (VNF_E_INVALID: n
 * outside 0..65535, subseq_bits neither 0 nor a multiple of 32 in 32..8192, an info vnf_jpeg_probe does not fill,
 * max_blob_bytes outside 0..2^28) */
int64_t vnf_jpeg_huff_decode_workspace_bytes(int n, const vnf_jpeg_info* info, int64_t max_blob_bytes, int subseq_bits);
/* n prepared frames of ONE geometry (*info: width, height, components, sampling, coef_count; restart intervals and
 * tables are each frame's own): frame i's blob is blobs_dev[blob_offsets[i], + blob_bytes[i]) on the device, blobs_dev
 * and every offset 16-byte aligned; blob_offsets and blob_bytes are HOST arrays of n, read before the call returns.  The
 * kernels clamp every access by these sizes, never by a value a blob holds.  coefs_dev: device (n, coef_count) int16 in
 * exactly the layout vnf_jpeg_entropy_decode writes and vnf_jpeg_decode_frames reads; status_dev: device (n) int32;
 * workspace: device, 16-byte aligned.  status_dev[i] is VNF_OK and frame i's coefficients are those
 * vnf_jpeg_entropy_decode gives, or VNF_E_INVALID (a stream that call refuses, or a blob that does not fit its size):
 * the frame's coefficients are then unspecified, nothing outside its own coef_count was written, and the other frames
 * are unaffected.  subseq_bits: 0 for the default (1024), else a multiple of 32 in 32..8192 -- a tuning parameter; the
 * result does not depend on it.  Enqueued on `stream` (two memsets, nine launches and one more per 65536 lanes of the
 * longest frame, per group of 32 frames), nothing allocated, no host synchronisation.  n == 0: no-op.
 * Returns VNF_E_INVALID: n outside 0..65535, a NULL or misaligned pointer, a subseq_bits outside the above, an info
 * vnf_jpeg_probe does not fill, an offset or size outside the above; VNF_E_CAPACITY: workspace_bytes below
 * vnf_jpeg_huff_decode_workspace_bytes(n, info, max(blob_bytes), subseq_bits); VNF_E_HIP: a launch error. */
int vnf_jpeg_huff_decode_frames(const uint8_t* blobs_dev, const int64_t* blob_offsets, const int64_t* blob_bytes, int n,
                                const vnf_jpeg_info* info, int subseq_bits, int16_t* coefs_dev, int32_t* status_dev,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* frame overlay ---------------------------------------------------------------------------- */
#define VNF_OVERLAY_RECT 0
#define VNF_OVERLAY_LABEL 1
/* One drawing step on one frame of a batch.
 *   VNF_OVERLAY_RECT:  the outline, 2 pixels thick, of the rectangle with corners (x0,y0) and (x1,y1), both inside it
 *                      (ImageDraw.rectangle(width=2) for corners truncated toward zero; boxes of 3 pixels and more);
 *   VNF_OVERLAY_LABEL: (x0,y0) is where the top-left pixel of a coverage mask of x1 columns and y1 rows goes; the mask
 *                      is masks[mask_offset, mask_offset + x1 * y1), row-major, 255 = full colour.
 * rgb: the colour as r | g << 8 | b << 16. */
typedef struct {
  int32_t kind, frame;
  int32_t x0, y0, x1, y1;
  int32_t mask_offset;
  uint32_t rgb;
} vnf_overlay_op;
/* cli_utils.draw_boxes_on_image (demo_image.py:150-158) on frames in device memory, in place, one launch: frames_dev
 * device (b,height,width,3) u8; ops_dev device (n_ops) entries in DRAW ORDER (a later entry paints over an earlier one
 * of the same frame; the entries of different frames may interleave); masks_dev device u8 (masks_bytes of them, may be
 * NULL when that is 0).  A label pixel is blended per channel as v = bg (255 - m) + c m + 128, ((v >> 8) + v) >> 8.
 * Everything is clipped to the frame.  The table lives in device memory, so the call cannot see its values: an entry
 * whose frame is outside 0..b-1, whose kind is unknown or whose mask leaves [0, masks_bytes) paints nothing.
 * Nothing allocated, no synchronisation.  b == 0 or n_ops == 0: no-op.  VNF_E_INVALID: a negative count, height or
 * width outside 1..65535, a NULL frames_dev / ops_dev. */
int vnf_overlay_draw(uint8_t* frames_dev, int b, int height, int width, const vnf_overlay_op* ops_dev, int n_ops,
                     const uint8_t* masks_dev, int64_t masks_bytes, void* stream);

/* Text runs: lines that differ per face and per frame (cli_utils.draw_emotions, demo_image.py:161-171), composited on
 * the device from a glyph atlas instead of rendered on the host. */
#define VNF_TEXT_RUN_MAX 64   /* characters in one run */
#define VNF_TEXT_GLYPH_MAX 64 /* a glyph's width, height and advance, and the magnitude of its offsets */
/* One glyph: its coverage cut to the ink, w columns by h rows, row-major at coverage[offset, offset + w * h); (ox, oy)
 * is where its top-left pixel lies relative to the pen, advance what it moves the pen by. */
typedef struct {
  int32_t offset, w, h, ox, oy, advance;
} vnf_text_glyph;
/* The atlas in device memory: this header, n_glyphs vnf_text_glyph for the characters first_char .. first_char +
 * n_glyphs - 1, then the coverage bytes.  n_glyphs in 1..256. */
typedef struct {
  int32_t first_char, n_glyphs;
} vnf_text_atlas;
/* One ImageDraw.text((x, y), chars[first, first + length), fill=rgb) call on one frame; rgb as in vnf_overlay_op. */
typedef struct {
  int32_t frame, x, y;
  uint32_t rgb;
  int32_t first, length;
} vnf_text_run;
/* Paints the runs in place on frames_dev (b,height,width,3) u8, after whatever is on the frames already (call it
 * behind vnf_overlay_draw on the same stream): the glyphs of a run sit at pen positions equal to the sum of the
 * preceding advances, overlapping glyphs combine as dst += round(src (255 - dst) / 255), and the run's coverage is
 * blended with vnf_overlay_draw's label formula.  With an atlas of Pillow's default font (jpeg_encode.text_atlas) this
 * is ImageDraw.text byte for byte.  One workgroup per run, threads over the run's ink rectangle clipped to the frame.
 *   runs_dev: device, n_runs entries in DRAW ORDER; chars_dev: device bytes; atlas_dev: device, atlas_bytes in all.
 *   launch_ends: HOST array of n_launches ascending run counts, the last one n_runs, or NULL for one launch: runs
 *   [launch_ends[i-1], launch_ends[i]) go into launch i.  The runs of one launch must not intersect on a frame; a run
 *   that intersects an earlier one belongs to a later launch, which paints over it (jpeg_encode.text_runs orders them).
 * The tables live in device memory, so the call cannot see their values: a run whose frame is outside 0..b-1, whose
 * length is outside 1..VNF_TEXT_RUN_MAX or whose characters leave [0, chars_bytes) paints nothing; a character outside
 * the atlas or a glyph outside VNF_TEXT_GLYPH_MAX or the atlas's bytes has no ink and does not move the pen.
 * Nothing allocated, no synchronisation.  b == 0 or n_runs == 0: no-op.  VNF_E_INVALID: a negative count, height or
 * width outside 1..65535, a NULL or misaligned pointer, launch_ends not ascending or not ending at n_runs. */
int vnf_overlay_draw_text(uint8_t* frames_dev, int b, int height, int width, const vnf_text_run* runs_dev, int n_runs,
                          const int32_t* launch_ends, int n_launches, const uint8_t* chars_dev, int64_t chars_bytes,
                          const void* atlas_dev, int64_t atlas_bytes, void* stream);

/* Gallery identification ------------------------------------------------------------------------ */
/* A gallery is a device matrix of unit-norm fp32 rows (G, dim) with an int32 label per row; identification is an exact
 * cosine top-k search over it, so people are added without training.  dim: a multiple of 16 in 16..512 (else
 * VNF_E_INVALID).  capacity_rows is only the first allocation: vnf_gallery_add grows it (amortised doubling, device to
 * device copy).  Release with vnf_destroy. */
int vnf_gallery_create(int dim, int64_t capacity_rows, vnf_handle* out);
/* Appends n rows: rows_dev device (n,dim) fp32, 16-byte aligned, each stored as x / max(||x||_2, 1e-12) (F.normalize's
 * rule); labels_dev device (n) int32, copied as they are.  Enqueued on `stream`; a call that has to grow the matrix
 * synchronises that stream and the device once.  VNF_E_CAPACITY: more than 2^31 - 1 rows. */
int vnf_gallery_add(vnf_handle gallery, const float* rows_dev, const int32_t* labels_dev, int64_t n, void* stream);
int vnf_gallery_size(vnf_handle gallery, int64_t* rows);
/* The stored (unit) rows [first, first + n) copied to rows_out_dev (n,dim) fp32, device to device on `stream`: what a
 * gallery file keeps.  vnf_gallery_add_unit appends such rows as they are, without normalising them again, so a saved
 * gallery comes back bit for bit. */
int vnf_gallery_rows(vnf_handle gallery, float* rows_out_dev, int64_t first, int64_t n, void* stream);
int vnf_gallery_add_unit(vnf_handle gallery, const float* rows_dev, const int32_t* labels_dev, int64_t n, void* stream);
/* Enrolment of a centroid gallery: sums_inout_dev (num_classes,dim) fp32 += the normalised rows (same rule) whose label
 * is the class, counts_inout_dev (num_classes) int32 += their number.  The rows of a class are added in row order in
 * fp32, so the result repeats bitwise and appending later needs the sums alone.  A label outside [0, num_classes)
 * matches no class (the table lives in device memory; the host layer checks labels before they are uploaded).  One
 * wave per class walks every label: not a hot path. */
int vnf_gallery_class_sums(const float* rows_dev, const int32_t* labels_dev, int64_t n, int dim, float* sums_inout_dev,
                           int32_t* counts_inout_dev, int num_classes, void* stream);
/* Bytes of workspace vnf_gallery_search needs for F queries, k results, a gallery of G rows and this chunk_rows (0: the
 * library's default, which depends on F and G).  Negative VNF_E_INVALID on a bad argument. */
int64_t vnf_gallery_search_workspace_bytes(int F, int k, int64_t G, int64_t chunk_rows);
/* q_dev device (F,dim) fp32, 16-byte aligned, normalised by the kernel with the rule of vnf_gallery_add.
 * score = <q^, g^> in fp32 on v_mfma_f32_16x16x4_f32 with one k order per (query, row) pair: a score's bits depend on
 * the two vectors only, not on F, the row's position or chunk_rows.  Per query, idx_out / label_out / score_out (F,k)
 * receive the k best rows (1 <= k <= 16) under the total order (score descending, row index ascending); -0 ties with
 * +0, a NaN score (returned as the canonical quiet NaN) orders below every number, and the slots beyond G hold index
 * -1, label -1, score -inf.  Stage one: a wave takes chunk_rows gallery rows against 16 queries and writes a partial
 * top-k to the workspace; stage two merges the partial lists, exactly because the order is total.  No atomics, nothing
 * allocated, no synchronisation.  chunk_rows is public so that a test can put a chunk boundary anywhere.  F == 0:
 * no-op.  VNF_E_CAPACITY: workspace_bytes below vnf_gallery_search_workspace_bytes of the same arguments. */
int vnf_gallery_search(vnf_handle gallery, const float* q_dev, int F, int k, int32_t* idx_out, int32_t* label_out,
                       float* score_out, int64_t chunk_rows, void* workspace, int64_t workspace_bytes, void* stream);
/* Gallery calibration: the label-aware search.  q_dev (F,dim) fp32 probes as for vnf_gallery_search, qlabels_dev (F)
 * int32 their known labels, exclude_dev (F) int32 or NULL.  Per probe f, idx_out / label_out / score_out (F,2) receive
 *   column 0, the mate:     the best row g with labels[g] == qlabels[f] and g != exclude[f];
 *   column 1, the non-mate: the best row g with labels[g] != qlabels[f] (exclude plays no part);
 * "best" under vnf_gallery_search's total order, an absent candidate being index -1, label -1, score -inf.  exclude ==
 * NULL and exclude[f] == -1 exclude nothing (a gallery calibrated against itself passes each probe's own row); a probe
 * label that no row carries is legal and has no mate.  The scores come from the code vnf_gallery_search runs: the bits
 * of a (probe, row) score are the same in both.  Stage one keeps two keys per lane in registers (no LDS, no atomics) and
 * writes (chunk, 2F, 1) partials; stage two is the search's merge.  F == 0: no-op.  Errors as vnf_gallery_search:
 * VNF_E_INVALID for a null pointer, a q_dev not 16-byte or a workspace not 8-byte aligned; VNF_E_CAPACITY for
 * workspace_bytes below vnf_gallery_mated_search_workspace_bytes of the same arguments. */
int64_t vnf_gallery_mated_search_workspace_bytes(int F, int64_t G, int64_t chunk_rows);
int vnf_gallery_mated_search(vnf_handle gallery, const float* q_dev, const int32_t* qlabels_dev, const int32_t* exclude_dev, int F,
                             int32_t* idx_out, int32_t* label_out, float* score_out, int64_t chunk_rows, void* workspace,
                             int64_t workspace_bytes, void* stream);
/* Gallery clustering: DBSCAN over the gallery's own G stored rows, by an all-pairs self-join.  The result is a function
 * of the scores alone: neither scheduling nor chunk_rows nor the order in which edges are met changes a bit of it.
 *   score     s(i,j) = the fp32 dot of stored rows i and j on v_mfma_f32_16x16x4_f32 in the search's k order, the rows
 *             taken AS STORED (no second normalisation), so s(i,j) and s(j,i) have the same bits.  It is therefore NOT
 *             bit-equal to vnf_gallery_search's score of the same pair, which normalises its query once more.
 *   neighbour N(i) = { j != i : s(i,j) >= threshold }; a NaN score is never >= threshold.  degree_out[i] = |N(i)|.
 *   core      degree(i) + 1 >= min_samples (a row counts itself, as in scikit-learn's DBSCAN); min_samples 1 makes every
 *             row core, which gives plain connected components.
 *   cluster   the connected components of the core rows under s >= threshold, numbered 0, 1, ... in ascending order of
 *             each component's smallest row index.
 *   border    a non-core row with a core neighbour: it joins the cluster of its BEST core neighbour under
 *             vnf_gallery_search's total order (score descending, row index ascending).  Every other row is noise, -1.
 *   nearest   nn_idx_out[i] / nn_score_out[i]: the best OTHER row of row i under the same order, neighbour or not
 *             (-1, -inf when G == 1; a NaN score is returned as the canonical quiet NaN).
 * All pointers are device pointers; cluster_out, degree_out, nn_idx_out (int32) and nn_score_out (fp32) are (G) arrays,
 * n_clusters_out one int32.  Three stages on `stream`: degrees and nearest neighbours (the search's stream with a key
 * and a count per lane, the search's merge with k = 1, one integer atomic add per row and chunk); links (the same pairs
 * with the same scoring code, a lock-free union-find over the core rows that hooks the larger root under the smaller by
 * compare-and-swap, so the final root of a component is its smallest row whatever the arrival order); numbering (a scan
 * over the roots).  No float atomics, nothing allocated, no synchronisation.  chunk_rows as for vnf_gallery_search
 * (0: the library's default).  G == 0: a no-op that writes *n_clusters_out = 0.  VNF_E_INVALID: not a gallery handle,
 * a NaN threshold, min_samples < 1, a null pointer, a workspace not 16-byte aligned; VNF_E_CAPACITY: workspace_bytes
 * below vnf_gallery_cluster_workspace_bytes of the same G and chunk_rows. */
int64_t vnf_gallery_cluster_workspace_bytes(int64_t G, int64_t chunk_rows);
int vnf_gallery_cluster(vnf_handle gallery, float threshold, int min_samples, int32_t* cluster_out, int32_t* degree_out,
                        int32_t* nn_idx_out, float* nn_score_out, int32_t* n_clusters_out, int64_t chunk_rows, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* Face tracks: the G faces of a video, stored in a gallery IN FRAME ORDER, linked across frames.  A row's int32 label is
 * its frame ordinal f(i) -- its position among the processed frames --, non-decreasing in i; frame_first_dev is a device
 * int32 array of n_frames + 1 entries, the rows of frame p being [frame_first[p], frame_first[p + 1]), ascending from 0 to G;
 * boxes_dev is device (G,4) fp32 x1,y1,x2,y2, 16-byte aligned, or NULL.  The result is a function of these inputs alone:
 * neither scheduling nor the number of waves nor the order in which pairs are met changes a bit of it.
 *   score      s(i,j): vnf_gallery_cluster's, the fp32 dot of the two STORED rows, the same bits from either side.
 *   candidate  j is a forward candidate of i iff 0 < f(j) - f(i) <= max_gap (with j > i, which the order of the rows
 *              implies), s(i,j) >= threshold (a NaN score never), and, with min_iou > 0,  inter >= min_iou * union  where
 *              iw = max(0, min(x2) - max(x1)), ih likewise, inter = iw * ih, area = (x2 - x1) * (y2 - y1),
 *              union = area_i + area_j - inter: fp32, in this operation order, nothing contracted.  With min_iou <= 0 the
 *              boxes are not read.  Two faces of one frame are never candidates of each other.  i is a backward
 *              candidate of j exactly where j is a forward candidate of i.
 *   best       next(i): the best forward candidate of i under the total order (frame distance ascending, then score
 *              descending, then row index ascending -- the last two vnf_gallery_search's order); pred(j): the best backward
 *              candidate of j likewise.
 *   link       i -> j iff next(i) == j and pred(j) == i.  A row has at most one successor and one predecessor, so the
 *              links form chains through strictly increasing frames: the tracks.
 * Outputs, device arrays of G entries: prev_out / next_out (int32) the linked rows, -1 without one; link_score_out
 * (fp32) the score of the link to prev, -inf at the head of a track (-0 is returned as +0); track_out (int32) the
 * track of each row, tracks numbered 0, 1, ... in ascending order of each chain's first row; n_tracks_out one int32.
 * The work follows the window, not G^2: a wave takes 16 rows and streams the one contiguous row range frame_first gives
 * for the frames within max_gap of them, 32 rows a step, keeping a best forward and a best backward candidate per
 * lane; then mutual bests, then chains to tracks: ceil(log2(n_frames)) rounds of pointer jumping, and a scan over the
 * heads as vnf_gallery_cluster numbers its roots.
 * No float atomics, nothing allocated, no synchronisation.  G == 0: a no-op that writes *n_tracks_out = 0 and looks at
 * no other pointer.  VNF_E_INVALID: not a gallery handle, a NaN threshold or min_iou, max_gap outside 1..255,
 * n_frames < 0, a null pointer (boxes_dev only with min_iou > 0), a workspace or boxes_dev not 16-byte aligned;
 * VNF_E_CAPACITY: workspace_bytes below vnf_gallery_tracks_workspace_bytes(G).  frame_first and the labels live in
 * device memory and are the caller's to check: tables that break the rules above give tracks that mean nothing, but no
 * row outside [0, G) is read or written and every loop ends (the rounds are counted from n_frames). */
int64_t vnf_gallery_tracks_workspace_bytes(int64_t G);
int vnf_gallery_tracks(vnf_handle gallery, const int32_t* frame_first_dev, int n_frames, const float* boxes_dev, float threshold,
                       float min_iou, int max_gap, int32_t* prev_out, int32_t* next_out, float* link_score_out, int32_t* track_out,
                       int32_t* n_tracks_out, void* workspace, int64_t workspace_bytes, void* stream);
/* One pooled row per track: sums_out device (n_tracks,dim) fp32, 16-byte aligned, row k the sum of the stored rows of
 * track k IN ROW ORDER, s = s + x from 0 in fp32 per element (it repeats bitwise and equals a sequential fp32 sum on the
 * host); counts_out device (n_tracks) int32 their number.  prev_dev, next_dev, track_dev: vnf_gallery_tracks' outputs
 * for this gallery.  A wave per track starts at the track's head (the row without a prev) and walks next while it leads
 * to a later row of the gallery; a track number no head carries gets zeros and 0.  n_tracks == 0: no-op. */
int vnf_gallery_track_sums(vnf_handle gallery, const int32_t* prev_dev, const int32_t* next_dev, const int32_t* track_dev, int n_tracks,
                           float* sums_out, int32_t* counts_out, void* stream);

/* One-convolution probe (debug / test entry) -------------------------------------------------- */
/* Every convolution of every plan goes through one launcher that picks one of vnf_conv_probe_cfgs() tile
 * configurations (three kernel families, each compiled for five storage layouts).  A probe is a plan of exactly ONE
 * convolution of the caller's geometry, packed as the plans pack theirs, that runs one NAMED configuration on the
 * caller's device buffers, so that every instantiation can be compared with a reference of
 *     out[m][co] = store(act(sum_k x[pix(m) + tap(k)] * w[co][k] + bias[class(m)][co] + res[m][co]))
 * Nothing is tuned and nothing falls back.  Release with vnf_destroy. */
typedef struct {
  int32_t n, h, w, cin;          /* input: n images of h x w pixels, cin channels consumed */
  int32_t kh, kw, sh, sw, ph, pw;
  int32_t cout;                  /* multiple of 8 */
  int32_t x_coff, ldx;           /* the input is channels [x_coff, x_coff + cin) of an NHWC buffer ldx channels wide */
  int32_t nseg;                  /* 1..4: output channels [seg_c0[i], seg_c1[i]) go to channels [seg_coff[i], ...) of */
  int32_t seg_c0[4], seg_c1[4];  /*   buffer i, seg_ld[i] channels wide; the segments tile [0, cout), all four numbers */
  int32_t seg_ld[4], seg_coff[4];/*   multiples of 8 */
  int32_t has_res, ldres, res_coff; /* residual: channels [res_coff, res_coff + cout) of an (n,Ho,Wo,ldres) buffer */
  int32_t act;                   /* 0 none, 1 ReLU, 2 PReLU (per-channel slopes) */
  int32_t out_f32;               /* outputs are fp32 whatever the dtype */
  int32_t dtype, planar;         /* VNF_F32 | VNF_BF16 | VNF_F16 | VNF_F16X2; planar: with VNF_F16X2, the encoders'
                                    8-channel units [8 hi][8 lo] instead of interleaved (hi, lo) pairs */
} vnf_conv_probe_geom;
/* w: host fp32 [cout][cin][kh][kw]; bias, slope (with act 2, else NULL), pre_s / pre_t (a BatchNorm x * pre_s[c] +
 * pre_t[c] on the unpadded input, folded into the weights and nine border-class biases; both or neither): host fp32
 * per channel, may be NULL.  The persistent switch of the wave-specialised kernels is VNF_WS_PERSIST as it is now, as
 * for every handle.  VNF_E_INVALID: a geometry, alignment or layout the convolution core does not take. */
int vnf_conv_probe_create(const vnf_conv_probe_geom* geom, const float* w, const float* bias, const float* slope,
                          const float* pre_s, const float* pre_t, vnf_handle* out);
/* Returns the number of tile configurations (or a negative VNF_E_* code).  admitted (NULL, or `capacity` >= that number
 * of entries): 1 where the launcher admits configuration id for this convolution, else 0.  family_sizes (may be NULL):
 * how many of the ids are ring, patch and wave-specialised tiles, in id order. */
int vnf_conv_probe_cfgs(vnf_handle probe, int32_t* admitted, int capacity, int32_t family_sizes[3]);
/* The tile of configuration cfg, whatever the convolution: {family (0 ring, 1 patch, 2 wave-specialised), BM, BN, waves
 * along M, waves along N, ring stages}.  Host only.  VNF_E_INVALID: no such id. */
int vnf_conv_cfg_tile(int cfg, int32_t tile[6]);
/* One launch of configuration cfg (-1: the launcher's heuristic) and a synchronisation of `stream`.  x, out[0..nseg) and
 * res are device pointers to the WHOLE buffers of the geometry, in the storage layout; the call writes the output
 * slices' first n*Ho*Wo rows and nothing else.  VNF_E_INVALID when the configuration is not admitted (never another
 * one in its place); VNF_E_HIP with the error of that launch; no retry. */
int vnf_conv_probe_run(vnf_handle probe, int cfg, const void* x, void* const* out, const void* res, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VNFACE_H */
