// Encoder engine: activations are NHWC slices of a small set of device buffers (concat-free inception branches); a
// static plan of convolution / pooling launches (plan_*.cpp build it, plan.cpp packs the weights) is replayed on the
// caller's stream.  Tiles: autotune.cpp; fused stacks: fused.cpp.
#include "engine.h"
#include "split_f16.h"

#include <cstdio>
#include <cstring>

namespace vnf {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
const char* last_error_cstr() { return g_err.c_str(); }

HandleBase::~HandleBase() {
  for (void* p : allocs) (void)hipFree(p);
}
void* HandleBase::dalloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    set_error(std::string("hipMalloc: ") + hipGetErrorString(e));
    return nullptr;
  }
  allocs.push_back(p);
  return p;
}
void* HandleBase::upload(const void* host, size_t bytes) {
  void* p = dalloc(bytes);
  if (!p) return nullptr;
  hipError_t e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error(std::string("hipMemcpy H2D: ") + hipGetErrorString(e));
    return nullptr;
  }
  return p;
}

WeightMap::WeightMap(const vnf_tensor_desc* w, int n) {
  for (int i = 0; i < n; ++i)
    if (w[i].name) m[w[i].name] = &w[i];
}
const float* WeightMap::get(const std::string& name, int64_t numel) {
  auto it = m.find(name);
  if (it == m.end() || it->second->dtype != VNF_F32 || !it->second->data) {
    if (missing.empty()) missing = name;
    return nullptr;
  }
  int64_t n = 1;
  for (int i = 0; i < it->second->ndim; ++i) n *= it->second->shape[i];
  if (n != numel) {
    if (missing.empty()) missing = name + " (unexpected size)";
    return nullptr;
  }
  return (const float*)it->second->data;
}

static inline uint16_t f2bf16(float f) {  // round to nearest even, NaN preserved
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
void convert_to(int dtype, const float* src, void* dst, size_t n) {
  if (dtype == F32) {
    memcpy(dst, src, n * 4);
  } else if (dtype == BF16) {
    uint16_t* d = (uint16_t*)dst;
    for (size_t i = 0; i < n; ++i) d[i] = f2bf16(src[i]);
  } else if (dtype == F16X2) {
    sf16* d = (sf16*)dst;
    for (size_t i = 0; i < n; ++i) d[i] = sf16(src[i]);
  } else if (dtype == F16P) {
    // planar split-f16 WEIGHTS: per K tile of 32 k values [32 hi][32 lo] -- the 128-byte LDS row of a K tile is its
    // four hi chunks followed by its four lo chunks (conv_device.h); n is a whole number of K tiles
    _Float16* d = (_Float16*)dst;
    for (size_t t = 0; t + 32 <= n; t += 32)
      for (int i = 0; i < 32; ++i) {
        const sf16 v(src[t + i]);
        d[2 * t + i] = v.hi;
        d[2 * t + 32 + i] = v.lo;
      }
  } else {
    _Float16* d = (_Float16*)dst;
    for (size_t i = 0; i < n; ++i) d[i] = (_Float16)src[i];
  }
}

// ---------------------------------------------------------------------------------------------
int Encoder::add_buf(int H, int W, int C) {
  bufs.push_back(Buf{H, W, C});
  return (int)bufs.size() - 1;
}

ConvArgs Encoder::conv_args(const ConvLayer& L, int n0, int nn) const {
  const int es = dtype_size(dtype);
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.dtype = dtype;
  a.x = at(L.x_buf, n0, L.x_coff);
  a.ldx = bufs[L.x_buf].C; a.H = L.H; a.W = L.W; a.Cin = L.cin; a.Ho = L.Ho; a.Wo = L.Wo;
  a.KH = L.KH; a.KW = L.KW; a.sh = L.sh; a.sw = L.sw; a.ph = L.ph; a.pw = L.pw;
  a.w = L.w; a.K = L.K; a.Kpad = L.Kpad; a.bias = L.bias; a.ncls = L.ncls; a.cout_pad = L.cout_pad;
  a.ktab = L.ktab; a.M = nn * L.Ho * L.Wo; a.Cout = L.cout; a.nseg = L.nseg;
  for (int i = 0; i < L.nseg; ++i) {
    a.seg[i].c0 = L.seg[i].c0; a.seg[i].c1 = L.seg[i].c1;
    if (L.seg[i].buf == -2) {
      a.seg[i].ptr = emb_raw + (size_t)n0 * emb_ld;
      a.seg[i].ld = emb_ld;
    } else {
      const Buf& ob = bufs[L.seg[i].buf];
      a.seg[i].ptr = ob.ptr + ((size_t)n0 * ob.elems_per_image() + L.seg[i].coff) * (L.out_f32 ? 4 : es);
      a.seg[i].ld = ob.C;
    }
  }
  if (L.res_buf >= 0) {
    a.res = at(L.res_buf, n0, L.res_coff);
    a.ldres = bufs[L.res_buf].C;
  }
  a.act = L.act; a.slope = L.slope; a.out_f32 = L.out_f32;
  a.cfg = L.cfg;
  a.ws_persist = env.ws_persist;
  return a;
}

int Encoder::finalize() {
  const int es = dtype_size(dtype);
  for (auto& b : bufs) {
    const size_t bytes = b.elems_per_image() * es * (size_t)max_batch;
    b.ptr = (char*)dalloc(bytes);
    if (!b.ptr) return VNF_E_HIP;
    VNF_HIP(hipMemset(b.ptr, 0, bytes));
  }
  emb_raw = (float*)dalloc((size_t)max_batch * emb_ld * 4);
  if (!emb_raw) return VNF_E_HIP;
  macs_alg = macs_exec = 0;
  for (auto& c : convs) { macs_alg += c.macs_alg; macs_exec += c.macs_exec; }
  if (groups.empty()) groups.push_back({0, (int)ops.size(), 1 << 30});
  const int rc = prepare_fused();
  if (rc != VNF_OK) return rc;
  fused_at.assign(ops.size(), -1);
  for (size_t i = 0; i < fused.size(); ++i)
    if (fused[i].active) fused_at[fused[i].first] = (int)i;
  tune_dirty = true;  // the first run() picks the tiles (after any set_streams / set_contexts of the caller)
  return VNF_OK;
}

// Images are independent, so a batch is cut into `nstreams` contiguous parts that run the whole plan
// concurrently on side streams (fork / join with events on the caller's stream): the small late
// layers (a few hundred workgroups, latency-bound) of one part fill the CUs the other leaves idle,
// and kernel-boundary drains overlap.
Encoder::~Encoder() {
  for (int i = 0; i < 4; ++i) {
    if (join_ev[i]) (void)hipEventDestroy(join_ev[i]);
    if (side[i]) (void)hipStreamDestroy(side[i]);
  }
  if (fork_ev) (void)hipEventDestroy(fork_ev);
  for (hipEvent_t ev : ctx_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (head_done) (void)hipEventDestroy(head_done);
  delete head;
}

int Encoder::select_ctx(hipStream_t s, int* used) {
  const int es = dtype_size(dtype);
  if (ctx_bufs.empty()) {  // context 0 = the buffers finalize() allocated
    ctx_bufs.emplace_back();
    for (auto& b : bufs) ctx_bufs[0].push_back(b.ptr);
    ctx_emb.push_back(emb_raw);
    ctx_ev.push_back(nullptr);
  }
  const int c = next_ctx % n_ctx;
  next_ctx = (c + 1) % n_ctx;
  while ((int)ctx_bufs.size() <= c) {
    std::vector<char*> set;
    for (auto& b : bufs) {
      const size_t bytes = b.elems_per_image() * es * (size_t)max_batch;
      char* p = (char*)dalloc(bytes);
      if (!p) return VNF_E_HIP;
      // on the caller's stream: ordered before this call's kernels (a null-stream hipMemset is not ordered against
      // non-blocking streams and may land after the first layers have written their outputs)
      VNF_HIP(hipMemsetAsync(p, 0, bytes, s));
      set.push_back(p);
    }
    float* er = (float*)dalloc((size_t)max_batch * emb_ld * 4);
    if (!er) return VNF_E_HIP;
    ctx_bufs.push_back(set);
    ctx_emb.push_back(er);
    ctx_ev.push_back(nullptr);
  }
  for (size_t i = 0; i < bufs.size(); ++i) bufs[i].ptr = ctx_bufs[c][i];
  emb_raw = ctx_emb[c];
  if (ctx_ev[c]) VNF_HIP(hipStreamWaitEvent(s, ctx_ev[c], 0));
  *used = c;
  return VNF_OK;
}

int Encoder::run(const void* x, int n, int x_dtype, float* out, hipStream_t s, std::string* report, const RunExtra* extra) {
  if (n < 0 || n > max_batch) return fail(VNF_E_CAPACITY, "batch exceeds max_batch");
  if (n == 0) return VNF_OK;
  if (tune_dirty) {
    tune_dirty = false;
    const int rc = autotune();
    if (rc != VNF_OK) return rc;
  }
  if (n_ctx > 1) {
    int c = 0;
    int rc = select_ctx(s, &c);
    if (rc != VNF_OK) return rc;
    const int keep = n_ctx;
    n_ctx = 1;  // the body below runs once on the selected set
    rc = run(x, n, x_dtype, out, s, report, extra);
    n_ctx = keep;
    if (rc != VNF_OK) return rc;
    if (!ctx_ev[c]) VNF_HIP(hipEventCreateWithFlags(&ctx_ev[c], hipEventDisableTiming));
    VNF_HIP(hipEventRecord(ctx_ev[c], s));
    return VNF_OK;
  }
  int ns = max_streams < 2 ? max_streams : 2;
  while (ns > 1 && n / ns < 96) --ns;  // below ~100 images a part no longer fills the chip: fixed per-launch latency dominates
  if (ns == 1 || report) return run_range(x, 0, n, x_dtype, out, s, report, extra);
  if (!side[0]) {
    for (int i = 0; i < 4; ++i) {
      VNF_HIP(hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
      VNF_HIP(hipEventCreateWithFlags(&join_ev[i], hipEventDisableTiming));
    }
    VNF_HIP(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
  }
  VNF_HIP(hipEventRecord(fork_ev, s));
  int rc = VNF_OK;
  for (int i = 0; i < ns && rc == VNF_OK; ++i) {
    const int i0 = (int)((long long)n * i / ns), i1 = (int)((long long)n * (i + 1) / ns);
    VNF_HIP(hipStreamWaitEvent(side[i], fork_ev, 0));
    rc = run_range(x, i0, i1, x_dtype, out, side[i], nullptr, extra);
    VNF_HIP(hipEventRecord(join_ev[i], side[i]));
    VNF_HIP(hipStreamWaitEvent(s, join_ev[i], 0));
  }
  return rc;
}

int Encoder::run_range(const void* x, int i0, int i1, int x_dtype, float* out, hipStream_t s, std::string* report,
                       const RunExtra* extra) {
  const RunExtra ex = extra ? *extra : RunExtra();
  const int n = i1 - i0;
  const bool f32_plan = dtype == F32 || dtype == F16X2;   // fp32 tensors, or split-f16 pairs in their 32-bit elements
  const size_t x_image = (size_t)3 * in_size * in_size * dtype_size(x_dtype);   // bytes per image of the caller's tensor
  std::vector<hipEvent_t> prof_ev;
  std::vector<int> prof_op;
  for (const Group& g : groups) {
    const int step = g.chunk < n ? g.chunk : n;
    for (int n0 = i0; n0 < i1; n0 += step) {
      const int nn = (i1 - n0) < step ? (i1 - n0) : step;
      for (int oi = g.first; oi < g.last; ++oi) {
        if (report) {
          hipEvent_t e0;
          VNF_HIP(hipEventCreate(&e0));
          VNF_HIP(hipEventRecord(e0, s));
          prof_ev.push_back(e0);
          prof_op.push_back(oi);
        }
        if (fused_at[oi] >= 0) {
          const FusedStack& f = fused[fused_at[oi]];
          const int rc = launch_fused(f, n0, nn, s);
          if (rc != VNF_OK) return rc;
          oi = f.end() - 1;
          continue;
        }
        const Op& op = ops[oi];
        const Buf* ib = op.src >= 0 ? &bufs[op.src] : nullptr;   // the source buffer of the ops that name one
        switch (op.kind) {
          case Op::PACK:
            if (ex.prep_src)   // vnf_emotion_recognize: the face transform writes the packed input itself
              VNF_HIP(launch_emotion_prep(ex.prep_src + (size_t)n0 * ex.prep_s * ex.prep_s * 3, nn, ex.prep_s, at(op.dst, n0), dtype, true, s));
            else
              VNF_HIP(launch_pack_input((const char*)x + n0 * x_image, x_dtype, at(op.dst, n0), dtype, nn, in_size * in_size, s));
            break;
          case Op::CONV: {
            const ConvLayer& L = convs[op.layer];
            hipError_t err = launch_conv(conv_args(L, n0, nn), s);
            if (err != hipSuccess) return fail(VNF_E_HIP, L.name + ": " + hipGetErrorString(err));
            break;
          }
          case Op::STEM1:
            VNF_HIP(launch_stem_conv1a((const char*)x + n0 * x_image, x_dtype, at(op.dst, n0), bufs[op.dst].C, dtype, nn, stem_wt,
                                       env.stem1a_mfma, s));
            break;
          case Op::MAXPOOL:
            VNF_HIP(launch_maxpool(at(op.src, n0), ib->C, at(op.dst, n0, op.dst_coff), bufs[op.dst].C, dtype, nn, ib->H, ib->W, ib->C,
                                   op.window, s));
            break;
          case Op::AVGPOOL:
            VNF_HIP(launch_avgpool(at(op.src, n0), ib->C, at(op.dst, n0), dtype, nn, ib->H * ib->W, ib->C, s));
            break;
          case Op::L2NORM:
            VNF_HIP(launch_l2norm(emb_raw + (size_t)n0 * 512, out + (size_t)n0 * 512, nn, 512, s));
            break;
          case Op::DWCONV: {
            if (!f32_plan) return fail(VNF_E_INVALID, "depthwise conv: fp32 / split-f16 plans only");
            const DwLayer& d = dws[op.layer];
            const Buf& xb = bufs[d.x_buf];
            VNF_HIP(launch_dwconv3x3(at_f32(d.x_buf, n0), at_f32(d.o_buf, n0), nn, xb.H, xb.W, d.C, d.stride, d.w, d.bias, d.slope,
                                     dtype == F16X2, s));
            break;
          }
          case Op::RSTEM:
            if (!f32_plan || !x) return fail(VNF_E_INVALID, "retina stem: fp32 / split-f16 plans on caller frames only");
            VNF_HIP(launch_retina_stem((const uint8_t*)x + (size_t)n0 * op.frame_h * op.frame_w * 3, nn, op.frame_h, op.frame_w, rstem_wa,
                                       rstem_bias, 0.1f, at_f32(op.dst, n0), dtype == F16X2, s));
            break;
          case Op::DWPW: {
            if (!f32_plan) return fail(VNF_E_INVALID, "dw+pw: fp32 / split-f16 plans only");
            const DwPwLayer& d = dwpws[op.layer];
            const Buf& xb = bufs[d.x_buf];
            VNF_HIP(launch_dwpw(at_f32(d.x_buf, n0), at_f32(d.o_buf, n0), nn, xb.H, xb.W, d.cin, d.cout, d.stride, d.dw, d.dbias, d.slope,
                                d.pw, d.pbias, d.slope, dtype == F16X2, s));
            break;
          }
          case Op::UPADD: {
            if (!f32_plan) return fail(VNF_E_INVALID, "upsample-add: fp32 / split-f16 plans only");
            const Buf& ob = bufs[op.dst];
            VNF_HIP(launch_upsample_add(at_f32(op.src, n0), ib->H, ib->W, at_f32(op.dst, n0), ob.H, ob.W, ob.C, nn, dtype == F16X2, s));
            break;
          }
          case Op::SE: {
            const SeLayer& L = ses[op.layer];
            const Buf& pb = bufs[L.part_buf];
            hipError_t err = launch_se_block(at(op.src, n0), at(op.res, n0), at(op.dst, n0), dtype, nn, ib->H * ib->W, L.C,
                                             SeWeights{L.w1, L.b1, L.w2, L.b2, L.slope_se, L.slope_out}, (float*)at(L.part_buf, n0),
                                             pb.elems_per_image() * dtype_size(dtype) / 4, s);
            if (err != hipSuccess) return fail(VNF_E_HIP, L.name + ": " + hipGetErrorString(err));
            break;
          }
          case Op::HEADS: {
            const float* raw = emb_raw + (size_t)n0 * emb_ld;
            if (out) VNF_HIP(launch_copy_rows_f32(raw, emb_ld, out + (size_t)n0 * op.n_cls, op.n_cls, nn, op.n_cls, s));
            if (ex.out2) VNF_HIP(launch_copy_rows_f32(raw + op.proj_col, emb_ld, ex.out2 + (size_t)n0 * op.n_proj, op.n_proj, nn, op.n_proj, s));
            break;
          }
          case Op::COPYOUT:
            VNF_HIP(hipMemcpyAsync(out + (size_t)n0 * 512, emb_raw + (size_t)n0 * 512, (size_t)nn * 512 * 4,
                                   hipMemcpyDeviceToDevice, s));
            break;
        }
      }
    }
  }
  return report ? write_report(prof_ev, prof_op, n, s, report) : VNF_OK;
}

// report label of the ops that have no line format of their own
static const char* op_label(const Op& op) {
  switch (op.kind) {
    case Op::PACK: return "pack";
    case Op::CONV: return "conv";
    case Op::MAXPOOL: return op.window.ceil ? "maxpool_ceil" : op.window.pad ? "maxpool_pad1" : "maxpool";
    case Op::AVGPOOL: return "avgpool";
    case Op::L2NORM: return "l2norm";
    case Op::COPYOUT: return "copyout";
    case Op::STEM1: return "stem1";
    case Op::DWCONV: return "dwconv3x3";
    case Op::UPADD: return "upsample_add";
    case Op::RSTEM: return "retina_stem (u8 frames -> conv0)";
    case Op::DWPW: return "dw3x3+pw1x1 fused";
    case Op::HEADS: return "heads";
    case Op::SE: return "se";
  }
  return "?";
}

// Per-op device time of one run_range (events between consecutive launches on the stream), summed over chunks: one line
// per op or fused stack, in plan order.  Takes the events over and destroys them.
int Encoder::write_report(std::vector<hipEvent_t>& prof_ev, const std::vector<int>& prof_op, int n, hipStream_t s,
                          std::string* report) const {
  hipEvent_t e_end;
  VNF_HIP(hipEventCreate(&e_end));
  VNF_HIP(hipEventRecord(e_end, s));
  VNF_HIP(hipEventSynchronize(e_end));
  prof_ev.push_back(e_end);
  std::vector<double> ms(ops.size(), 0.0);
  for (size_t i = 0; i + 1 < prof_ev.size(); ++i) {
    float t = 0;
    VNF_HIP(hipEventElapsedTime(&t, prof_ev[i], prof_ev[i + 1]));
    ms[prof_op[i]] += t;
  }
  for (auto ev : prof_ev) (void)hipEventDestroy(ev);
  char line[512];
  double total = 0;
  for (size_t oi = 0; oi < ops.size(); ++oi) {
    const Op& op = ops[oi];
    total += ms[oi];
    const double t = ms[oi];
    auto tflops = [t](double gf) { return t > 0 ? gf / t : 0.0; };
    if (fused_at[oi] >= 0) {   // the ops it replaces were never marked: no time, no line
      const FusedStack& f = fused[fused_at[oi]];
      const double gf = 2.0 * f.macs_alg * n / 1e9;
      snprintf(line, sizeof line, "%-28s %-60s %8.4f ms  %8.1f GFLOP %8.1f TFLOP/s\n", fused_label(f), fused_detail(f), t, gf, tflops(gf));
      oi = f.end() - 1;
    } else if (op.kind == Op::CONV) {
      const ConvLayer& L = convs[op.layer];
      const double gf = 2.0 * L.macs_alg * n / 1e9;
      snprintf(line, sizeof line, "%-28s conv M/img=%-6d N=%-5d K=%-5d %dx%d s%d cfg%-2d %8.4f ms  %8.1f GFLOP %8.1f TFLOP/s\n",
               L.name.c_str(), L.Ho * L.Wo, L.cout, L.K, L.KH, L.KW, L.sh, L.cfg, t, gf, tflops(gf));
    } else if (op.kind == Op::STEM1) {
      const double gf = 2.0 * convs[op.layer].macs_alg * n / 1e9;
      snprintf(line, sizeof line, "%-28s %-60s %8.4f ms  %8.1f GFLOP %8.1f TFLOP/s\n", "conv2d_1a (direct, NCHW in)",
               "3x3 s2 3->32 on the caller's tensor, exact f32 (MFMA / VALU)", t, gf, tflops(gf));
    } else if (op.kind == Op::SE) {
      // algorithmic traffic: t twice (mean, product), the residual once, the result once
      const Buf& b = bufs[op.src];
      const double mb = 4.0 * b.elems_per_image() * dtype_size(dtype) * n / 1e6;
      snprintf(line, sizeof line, "%-28s se %dx%dx%-4d squeeze + excite/apply %24s %8.4f ms  %8.1f MB    %8.3f TB/s\n",
               ses[op.layer].name.c_str(), b.H, b.W, b.C, "", t, mb, t > 0 ? mb / t / 1e3 : 0.0);
    } else {
      snprintf(line, sizeof line, "%-28s %-8s %60s %8.4f ms\n", "", op_label(op), "", t);
    }
    *report += line;
  }
  snprintf(line, sizeof line, "TOTAL %.4f ms for n=%d\n", total, n);
  *report += line;
  return VNF_OK;
}

}  // namespace vnf
