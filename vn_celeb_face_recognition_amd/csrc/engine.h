// Host-side engine shared by the encoder / classifier / detector handles of libvnface.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/vnface.h"
#include "kernels.h"

namespace vnf {

void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
const char* last_error_cstr();   // the calling thread's last message (vnf_last_error)

#define VNF_HIP(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return ::vnf::fail(VNF_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
  } while (0)

enum class HandleKind { Encoder = 1, Mlp, Mtcnn, MlpTrainer, Retina, HeadTrainer, ConvProbe, Gallery };

struct HandleBase {
  const HandleKind kind;
  explicit HandleBase(HandleKind k) : kind(k) {}
  int device = 0;
  std::vector<void*> allocs;  // device allocations owned by the handle
  virtual ~HandleBase();
  void* dalloc(size_t bytes);  // hipMalloc + bookkeeping (nullptr on failure, error set)
  void* upload(const void* host, size_t bytes);
};

// The handle as a T, or nullptr when it is null or of another kind (every handle type names its kind as T::KIND).
template <class T>
T* handle_cast(vnf_handle h) {
  HandleBase* b = reinterpret_cast<HandleBase*>(h);
  return (b && b->kind == T::KIND) ? static_cast<T*>(b) : nullptr;
}

// The handle as T, the common base of several handle types (it names their kinds as T::KINDS), or nullptr.
template <class T>
T* handle_cast_base(vnf_handle h) {
  HandleBase* b = reinterpret_cast<HandleBase*>(h);
  if (b)
    for (HandleKind k : T::KINDS)
      if (b->kind == k) return static_cast<T*>(b);
  return nullptr;
}

// state_dict lookup -----------------------------------------------------------------------
struct WeightMap {
  std::unordered_map<std::string, const vnf_tensor_desc*> m;
  std::string missing;
  WeightMap(const vnf_tensor_desc* w, int n);
  const float* get(const std::string& name, int64_t numel);  // nullptr (+missing recorded) if absent / wrong size
  bool has(const std::string& name) const { return m.count(name) != 0; }
};

// host float -> storage dtype ----------------------------------------------------------------
void convert_to(int dtype, const float* src, void* dst, size_t n);

// ---------------------------------------------------------------------------------------------
// Encoder: a static plan of convolutions / pools over NHWC buffers.
struct Buf {
  int H, W, C;
  size_t elems_per_image() const { return (size_t)H * W * C; }
  char* ptr = nullptr;
};

struct ConvLayer {
  std::string name;
  int x_buf, x_coff, cin;  // cin = padded channels consumed
  int H, W, Ho, Wo, KH, KW, sh, sw, ph, pw;
  void* w = nullptr;
  float* bias = nullptr;
  float* slope = nullptr;
  int4* ktab = nullptr;
  int K, Kpad, cout, cout_pad, ncls = 1;
  int nseg = 0;
  struct { int c0, c1, buf, coff; } seg[4];
  int res_buf = -1, res_coff = 0;
  int act = ACT_NONE, out_f32 = 0;
  int cfg = -1;  // tile configuration chosen by Encoder::autotune (-1 = launcher heuristic)
  double macs_alg = 0, macs_exec = 0;  // per image
};

struct Op {
  enum Kind { PACK, CONV, MAXPOOL, AVGPOOL, L2NORM, COPYOUT, STEM1, DWCONV, UPADD, RSTEM, DWPW, HEADS, SE } kind;
  int src = -1;                   // source buffer
  int dst = -1, dst_coff = 0;     // destination buffer and the channel offset of the slice written in it
  int layer = -1;                 // index into Encoder::convs (CONV, STEM1), dws (DWCONV), dwpws (DWPW) or ses (SE)
  int res = -1;                   // SE: the residual buffer
  PoolWindow window = {0, 0, false};   // MAXPOOL: stride-2 window (launch_maxpool)
  int frame_h = 0, frame_w = 0;   // RSTEM: size of the u8 frames the caller passes as x
  int n_cls = 0, n_proj = 0, proj_col = 0;   // HEADS: widths of the two heads, first projection column of emb_raw

  static Op pack(int dst) { Op o{PACK}; o.dst = dst; return o; }   // the caller's NCHW tensor (or u8 faces) -> NHWC8 plan input
  static Op conv(int layer) { Op o{CONV}; o.layer = layer; return o; }
  static Op stem1(int layer, int dst) { Op o{STEM1}; o.layer = layer; o.dst = dst; return o; }   // PACK + CONV of conv2d_1a, direct
  static Op maxpool(int src, int dst, int dst_coff, PoolWindow w = {3, 0, false}) {   // 3x3 s2 into a channel slice of dst
    Op o{MAXPOOL}; o.src = src; o.dst = dst; o.dst_coff = dst_coff; o.window = w; return o;
  }
  static Op maxpool_ceil(int src, int dst, int k) { return maxpool(src, dst, 0, {k, 0, true}); }
  static Op maxpool_pad1(int src, int dst) { return maxpool(src, dst, 0, {3, 1, false}); }   // 3x3 s2 p1
  static Op avgpool(int src, int dst) { Op o{AVGPOOL}; o.src = src; o.dst = dst; return o; }
  static Op l2norm() { return Op{L2NORM}; }     // emb_raw -> out, rows normalised
  static Op copyout() { return Op{COPYOUT}; }   // emb_raw -> out
  static Op dwconv(int layer) { Op o{DWCONV}; o.layer = layer; return o; }
  static Op dwpw(int layer) { Op o{DWPW}; o.layer = layer; return o; }
  static Op upadd(int src, int dst) { Op o{UPADD}; o.src = src; o.dst = dst; return o; }   // dst += nearest-upsampled src
  static Op rstem(int frame_h, int frame_w, int dst) { Op o{RSTEM}; o.frame_h = frame_h; o.frame_w = frame_w; o.dst = dst; return o; }
  static Op se(int layer, int src, int res, int dst) { Op o{SE}; o.layer = layer; o.src = src; o.res = res; o.dst = dst; return o; }   // dst = prelu(src * gate + res)
  static Op heads(int n_cls, int n_proj, int proj_col) { Op o{HEADS}; o.n_cls = n_cls; o.n_proj = n_proj; o.proj_col = proj_col; return o; }
};

struct DwLayer {   // depthwise 3x3 pad 1 + folded BN + LeakyReLU (fp32 plans: RetinaFace's MobileNetV1)
  int x_buf, o_buf, C, stride;
  float *w = nullptr, *bias = nullptr;   // [9][C], [C]
  float slope = 0.f;
};

struct DwPwLayer {   // conv_dw in one kernel (launch_dwpw): depthwise 3x3 + BN + leaky, pointwise 1x1 + BN + leaky
  int x_buf, o_buf, cin, cout, stride;
  float *dw = nullptr, *dbias = nullptr, *pw = nullptr, *pbias = nullptr;
  float slope = 0.f;
  std::string name;
};

struct SeLayer {   // squeeze-and-excitation + residual + PReLU behind conv2 / bn2 of an IRBlock (launch_se_block)
  std::string name;
  int C, part_buf;   // part_buf: plan buffer that holds the squeeze launch's fp32 slice sums
  float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
  float slope_se = 0.f, slope_out = 0.f;
};

struct Group { int first, last, chunk; };

// A run of plan ops that fused kernels replace when the compute dtype allows it (16-bit operands): the 40 convolutions
// of repeat_2 become one launch of block17_trunk_kernel (trunk17.hip), the 25 of repeat_1 five launches of
// block35_kernel (block35.hip), reduce + 1x3 + 3x1 of each Block8 one launch of block8_chain_kernel (block8.hip), the
// three branch-1 convolutions of mixed_6a one launch of mixed6a_chain_kernel (mixed6a.hip).
struct FusedStack {
  // Block17: persistent Block17 stack (trunk17.hip); Block35: one fused launch per Block35 (block35.hip);
  // StemMid: conv2d_2a + conv2d_2b + maxpool_3a in one launch (stem_mid.hip);
  // Block8: reduce + branch1.1 + branch1.2 of one Block8 in one launch (block8.hip): conv0 = the reduce, out_buf = the
  // 384-channel concat; the block's up-projection stays a plan op behind the stack
  // Mixed6a: mixed_6a.branch1.0 + branch1.1 + branch1.2 in one launch (mixed6a.hip): conv0 = the 1x1, in_buf = the
  // repeat_1 output, out_buf = the mixed_6a output, of which the launch writes the last convolution's channel slice
  enum class Kind { StemMid, Block35, Block17, Block8, Mixed6a } kind = Kind::Block17;
  std::string label;           // Block8, Mixed6a: the profile row's label
  int first = 0, last = 0;     // op range
  int in_buf = -1, out_buf = -1;
  int nblocks = 0;
  int conv0 = 0;               // index of the first of the 4*nblocks convolutions (reduce, 1x7, 7x1, up per block)
  void* wstream = nullptr;
  float* bias = nullptr;
  void* wtail = nullptr;       // Block35 with ext: block35_tail_repack image of mixed_6a.branch1.0
  bool active = false;
  bool stack = false;          // Block35: the five blocks in ONE launch, x resident in registers (trunk35.hip; bf16 / f16)
  double macs_alg = 0;         // per image
  // StemMid: conv2d_3b (the op after the pool) folded into the stem kernel; Block35 (stack): mixed_6a.branch1.0 (the op
  // after the last block) computed from the register-resident output: ops [first, ext_last) become one launch
  int ext_last = 0, ext_conv = -1, ext_out_buf = -1;
  bool ext = false;
  int end() const { return ext ? ext_last : last; }   // one past the last op the stack's launch replaces
};  // ops [first,last) run per `chunk` images (L3 residency)

struct Tap { int buf, coff, C; };   // buf -2: columns [coff, coff + C) of emb_raw

// Every switch an encoder takes from the environment (VNF_<FIELD NAME>; INTEGRATION.md has the table), read once, when
// the Encoder is constructed.  Plans, fused stacks, the autotuner and the launchers take their values from here.
struct EncoderEnv {
  int fuse = 223, direct_stem = 1, stem1a_mfma = 2, retina_fuse = 3, ws_persist = 1;
  int stem_chunk = 0, ir100_chunk1 = 0, ir100_chunk2 = 0;   // sub-batch of the leading op groups (<= 0: the plan's default)
  int autotune = 1, force_cfg = -2, tune_lanes = 0, autotune_log = 0;
  bool tune_final = true;   // 0: no finalists pass
  std::string tune_cache;   // file; empty: none
  static EncoderEnv read();
};

// Per-call arguments of the two-head plan beyond run()'s x / out (`out` is the class head): the second output of
// Op::HEADS, and the u8 faces (n,S,S,3) Op::PACK transforms instead of packing the caller's tensor (emotion_prep
// straight into the plan input)
struct RunExtra {
  float* out2 = nullptr;
  const uint8_t* prep_src = nullptr;
  int prep_s = 0;
};

// arch of the internal sub-plans (the public VNF_ARCH_* values are >= 0)
constexpr int ARCH_MLP = -1, ARCH_RNET = -2, ARCH_ONET = -3, ARCH_RETINA = -5;

struct Encoder : HandleBase {
  static constexpr HandleKind KIND = HandleKind::Encoder;
  Encoder() : HandleBase(KIND) {}
  ~Encoder() override;  // side streams, fork/join and context events (device buffers: HandleBase)
  int arch, dtype, max_batch, in_size;
  std::vector<Buf> bufs;
  std::vector<ConvLayer> convs;
  std::vector<DwLayer> dws;
  std::vector<DwPwLayer> dwpws;
  std::vector<SeLayer> ses;
  float *rstem_wa = nullptr, *rstem_bias = nullptr;   // RetinaFace stem (Op::RSTEM): MFMA lane table [7][64], bias [8]
  std::vector<Op> ops;
  std::vector<Group> groups;
  std::vector<FusedStack> fused;
  std::vector<int> fused_at;   // per op: index of the ACTIVE fused stack that starts there, or -1 (finalize)
  int prepare_fused();  // build the weight streams of the fused stacks (finalize)
  int launch_fused(const FusedStack& f, int n0, int nn, hipStream_t s);   // images [n0, n0 + nn) through the stack's kernel
  std::unordered_map<std::string, Tap> taps;
  bool buf_materialised(int buf) const;  // false: only ops that an ACTIVE fused stack replaces would write it
  float* emb_raw = nullptr;  // (max_batch,emb_ld) fp32 before the final normalisation
  int emb_ld = 512;          // row length of emb_raw (the two-head plan: both heads side by side)
  // ResNet-50 two-head plan (build_rn50_2b): head widths and the logits of vnf_emotion_recognize
  int n_cls = 0, n_proj = 0;
  float* cls_buf = nullptr;
  double macs_alg = 0, macs_exec = 0;
  // classification head of an IRv1 / IR-100 handle (vnf_encoder_create_classifier): `logits`, one linear layer on the
  // fp32 features in emb_raw, as an exact-f32 plan of its own like the MLP's; nullptr: no head
  Encoder* head = nullptr;
  int head_classes = 0, head_in = -1, head_logit = -1;
  float* head_emb = nullptr;         // (max_batch,512): where vnf_encoder_logprobs lets the plan's last op write
  hipEvent_t head_done = nullptr;    // orders calls on different streams over the head's one buffer set

  int add_buf(int H, int W, int C);
  // image n0 of a buffer, at channel `coff` (at_f32: the fp32 / split-f16 pair plans, 4-byte elements)
  char* at(int buf, int n0, int coff = 0) const {
    return bufs[buf].ptr + ((size_t)n0 * bufs[buf].elems_per_image() + coff) * dtype_size(dtype);
  }
  float* at_f32(int buf, int n0) const { return (float*)at(buf, n0); }
  int finalize();  // allocate buffers, autotune tile configurations
  int autotune();
  ConvArgs conv_args(const ConvLayer& L, int n0, int nn) const;
  int run(const void* x, int n, int x_dtype, float* out, hipStream_t s, std::string* report = nullptr,
          const RunExtra* extra = nullptr);
  int run_range(const void* x, int i0, int i1, int x_dtype, float* out, hipStream_t s, std::string* report, const RunExtra* extra);
  int write_report(std::vector<hipEvent_t>& prof_ev, const std::vector<int>& prof_op, int n, hipStream_t s, std::string* report) const;
  float* stem_wt = nullptr;  // IRv1: fp32 folded conv2d_1a weights + biases for the direct stem kernel (Op::STEM1)
  // activation-buffer contexts: consecutive vnf_embed calls rotate over n_ctx private buffer sets, so calls issued
  // on DIFFERENT streams may overlap on the GPU (the latency-bound tail of one batch under the throughput-bound
  // stem of the next); a set is re-used only after the event of its previous use.  Extra sets are allocated lazily.
  int n_ctx = 1, next_ctx = 0;
  std::vector<std::vector<char*>> ctx_bufs;
  std::vector<float*> ctx_emb;
  std::vector<hipEvent_t> ctx_ev;
  int select_ctx(hipStream_t s, int* used);
  int max_streams = 4;  // cap on run()'s batch split (1: never fork side streams)
  bool tune_dirty = true;  // tiles are (re)picked lazily at the next run(): create, set_streams and set_contexts only mark
  int tune_lanes = 1;   // concurrent copies the autotuner times each candidate as (set with the context count)
  int tune_batch = 0;   // batch size the autotuner times at (0: the part size run() uses at max_batch)
  const EncoderEnv env = EncoderEnv::read();
  hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t join_ev[4] = {nullptr, nullptr, nullptr, nullptr}, fork_ev = nullptr;
};

// the two report strings of an active fused stack (vnf_encoder_profile)
const char* fused_label(const FusedStack& f);
const char* fused_detail(const FusedStack& f);

// the plan builders (plan_*.cpp)
int build_irv1(Encoder& e, WeightMap& wm);
int build_ir100(Encoder& e, WeightMap& wm);
// SE-IR ResNet-101 (models/resnet_encoder.py:116-222, use_se=True), 112 x 112 input, L2-normalised output
int build_seir101(Encoder& e, WeightMap& wm);
// ResNet-50 with a class head and a projection head (models/resnet_2_branch.py:12-70), 224 x 224 input
int build_rn50_2b(Encoder& e, WeightMap& wm, int num_classes, int num_projections);
// RetinaFace (mobilenet0.25) on the exact-f32 core for an H x W input: buffer 0 = NHWC4 mean-subtracted input (written by
// the caller), head_bufs[l] = (Hl, Wl, 32) fp32 [cls 4 | bbox 8 | landmark 20] of pyramid level l
int build_retina_mnet(Encoder& e, WeightMap& wm, int H, int W, int head_bufs[3]);
// MTCNN R-Net / O-Net as MFMA plans (exact-f32 or split-f16) over NHWC4 candidate crops.  The detector touches four of a
// plan's buffers, named in `nb`: `crops` is written by its crop kernel, `pooled1` (conv1 + pool1) by its net_front_kernel,
// with mid `pooled2` (conv2 + pool2) by its net_mid_kernel, and `heads` holds the outputs: 8 floats [a0,a1,reg0..3,-,-] /
// 16 floats [a0,a1,reg0..3,lm0..9]
struct NetBufs { int crops, pooled1, pooled2, heads; };
int build_rnet(Encoder& e, WeightMap& wm, bool mid, NetBufs& nb);
int build_onet(Encoder& e, WeightMap& wm, bool mid, NetBufs& nb);

}  // namespace vnf
