// MTCNN detector, host layer: the handle, its creation (weight packing, tables), one detection as a sequence of launches
// (mtcnn.h; the kernels are mtcnn.hip, the rest of R-Net / O-Net the plans of plan_mtcnn.cpp) and the C ABI.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "det_results.h"
#include "engine.h"
#include "mtcnn.h"
#include "split_f16.h"

namespace vnf {

// R-Net or O-Net behind a candidate table, filled at create time: what run_net needs to know about the net
struct NetStage {
  std::unique_ptr<Encoder> enc;   // the plan on the MFMA core (candidates = batch)
  NetBufs bufs{};                 // the plan buffers the detector's own kernels touch
  int cap = 0;                    // candidates per chunk of the dense batch
  int S = 0, hw = 0, nf = 0;      // crop size 24 / 48, head width 8 / 16, columns of the output table 5 / 15
  float* out = nullptr;           // output table [frame][keep][nf]
  FrontW fw{};                    // conv1 + PReLU + pool1 by net_front_kernel (the plan starts at conv2)
  MidW mw{};                      // conv2 + PReLU + pool2 by net_mid_kernel (Mtcnn::mid)
  const char *crop_name = "", *front_name = "", *net_name = "", *post_name = "";   // stages of vnf_mtcnn_stage_times
  float* buf(int i) const { return (float*)enc->bufs[i].ptr; }
};

struct Mtcnn : HandleBase {
  static constexpr HandleKind KIND = HandleKind::Mtcnn;
  Mtcnn() : HandleBase(KIND) {}
  vnf_mtcnn_cfg cfg;
  PNetW pw;
  LevelTable cap_table;  // geometry at (max_height, max_width): sizes the buffers
  float *lvl = nullptr, *p1 = nullptr, *c2 = nullptr;
  Cand* cand = nullptr;                       // stage-1 records, dense by cell: [frame][cap_out]
  int *cells = nullptr, *keep1c = nullptr;    // per (level, frame) compact cell lists: P-Net hits / per-scale NMS survivors
  int keep = KEEP;                            // rows per frame of the stage-2 / stage-3 tables (vnf_mtcnn_cfg.max_candidates)
  NmsScratch scratch{};                       // global-memory fallback of the NMS kernels
  int *cand_cnt = nullptr, *keep1_cnt = nullptr, *row_cnt = nullptr, *row3_cnt = nullptr, *fin_cnt = nullptr, *status = nullptr;
  Row *rows = nullptr, *rows3 = nullptr;
  float* fin = nullptr;
  float *prob_dbg = nullptr, *reg_dbg = nullptr;
  NetStage rnet, onet;
  int* row_order = nullptr;                   // pyramid dispatch order (device), rebuilt when the frame size changes
  int row_order_h = 0, row_order_w = 0, row_order_cap = 0;
  bool mid = false;                           // conv2 + PReLU + pool2 by net_mid_kernel (split-f16 plans start at conv3)
  int* offs = nullptr;                        // device: (max_batch + 1) compact-batch offsets
  // final read-back: counts block + the first FIN_FAST rows of every frame packed by one kernel into `stage`,
  // one D2H copy into pinned memory, one host synchronisation (a frame with more faces takes the 2-D copy)
  float* stage = nullptr;
  int* h_pin = nullptr;
  // switches of the environment, read once at create time so that every handle keeps the ones it was made with
  int fin_fast = FIN_FAST;                    // VNF_FIN_FAST
  bool spec_on = true;                        // VNF_MTCNN_SPEC: size stages 2 / 3 from the previous call's counts
  bool layers = false;                        // VNF_MTCNN_LAYERS (diagnostic): per-layer table of the plans on stderr
  int last_b = 0;  // frames of the last vnf_mtcnn_detect (vnf_mtcnn_results_device)
  struct Dbg { int net = 0, c0 = 0, n = 0; } dbg;   // last chunk of the last vnf_mtcnn_debug_net (net 0: none) for its taps
  struct Spec { bool valid = false; int b = 0, H = 0, W = 0, max2 = 0, total2 = 0, max3 = 0, total3 = 0; } spec;   // launch sizes of stages 2 / 3 from the previous call
  ~Mtcnn() override { if (h_pin) (void)hipHostFree(h_pin); }
  size_t cap_px = 0, cap_p1 = 0, cap_c2 = 0, cap_out = 0;
};

static LevelTable make_levels(int h, int w, int minsize, double factor) {
  // detect_face.py:50-60,71 in python-double arithmetic
  LevelTable t;
  memset(&t, 0, sizeof(t));
  const double m = 12.0 / minsize;
  double minl = std::min(h, w) * m, scale = m;
  int opx = 0, op1 = 0, oc2 = 0, oout = 0;
  while (minl >= 12 && t.n < MAX_LEVELS) {
    LevelDesc& L = t.l[t.n];
    L.Hs = (int)(h * scale + 1);
    L.Ws = (int)(w * scale + 1);
    L.Hp = (L.Hs - 2 + 1) / 2;  // ceil((Hs-2)/2)
    L.Wp = (L.Ws - 2 + 1) / 2;
    L.H2 = L.Hp - 2; L.W2 = L.Wp - 2;
    L.oh = L.H2 - 2; L.ow = L.W2 - 2;
    L.scale = (float)scale;
    L.off_px = opx; L.off_p1 = op1; L.off_c2 = oc2; L.off_out = oout;
    opx += L.Hs * L.Ws; op1 += L.Hp * L.Wp; oc2 += L.H2 * L.W2; oout += L.oh * L.ow;
    ++t.n;
    scale = scale * factor;
    minl = minl * factor;
  }
  t.tot_px = opx; t.tot_p1 = op1; t.tot_c2 = oc2; t.tot_out = oout;
  return t;
}

static const float* up_transposed(Mtcnn& m, const float* w, int cout, int cin, int k) {
  // [cout][cin][k][k] -> [cin][k][k][cout]
  std::vector<float> t((size_t)cout * cin * k * k);
  for (int co = 0; co < cout; ++co)
    for (int c = 0; c < cin; ++c)
      for (int i = 0; i < k * k; ++i) t[((size_t)c * k * k + i) * cout + co] = w[((size_t)co * cin + c) * k * k + i];
  return (const float*)m.upload(t.data(), t.size() * 4);
}

// conv1 weights [cout][3][3][3] -> [32][9 taps][4 channels (3 + zero)], bias and PReLU slopes padded to 32
static bool pack_front(Mtcnn& m, WeightMap& wm, int cout, FrontW& fw) {
  const float* c1 = wm.get("conv1.weight", (int64_t)cout * 27);
  const float* b1 = wm.get("conv1.bias", cout);
  const float* a1 = wm.get("prelu1.weight", cout);
  if (!c1 || !b1 || !a1) return false;
  std::vector<float> w(32 * 36, 0.f), b(32, 0.f), a(32, 0.f);
  for (int co = 0; co < cout; ++co) {
    for (int c = 0; c < 3; ++c)
      for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) w[(co * 9 + kh * 3 + kw) * 4 + c] = c1[((co * 3 + c) * 3 + kh) * 3 + kw];
    b[co] = b1[co]; a[co] = a1[co];
  }
  fw.w = (const float*)m.upload(w.data(), w.size() * 4);
  fw.b = (const float*)m.upload(b.data(), b.size() * 4);
  fw.a = (const float*)m.upload(a.data(), a.size() * 4);
  return fw.w && fw.b && fw.a;
}

// conv2 weights [cout][cin][3][3] -> MFMA A-fragments of interleaved split-f16: fragment (ct, kb = 2 tap + half),
// lane (row r, group g) = the 4 k values (channels 16 half + 4 g .. + 3 of the tap) of output channel 16 ct + r
// as (hi, lo) pairs; input channels beyond cin (R-Net: 28 of 32) are zero
static bool pack_mid(Mtcnn& m, WeightMap& wm, int cout, int cin, MidW& mw) {
  const float* c2 = wm.get("conv2.weight", (int64_t)cout * cin * 9);
  const float* b2 = wm.get("conv2.bias", cout);
  const float* a2 = wm.get("prelu2.weight", cout);
  if (!c2 || !b2 || !a2) return false;
  std::vector<uint32_t> w((size_t)(cout / 16) * 18 * 64 * 4, 0u);
  for (int ct = 0; ct < cout / 16; ++ct)
    for (int kb = 0; kb < 18; ++kb)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 4; ++e) {
          const int co = 16 * ct + (l & 15), c = 16 * (kb & 1) + 4 * (l >> 4) + e, tap = kb >> 1;
          const float v = c < cin ? c2[((size_t)(co * cin + c) * 3 + tap / 3) * 3 + tap % 3] : 0.f;
          const sf16 sv(v);
          uint32_t bits;
          memcpy(&bits, &sv, 4);
          w[(((size_t)ct * 18 + kb) * 64 + l) * 4 + e] = bits;
        }
  mw.w = (const uint4*)m.upload(w.data(), w.size() * 4);
  mw.b = (const float*)m.upload(b2, (size_t)cout * 4);
  mw.a = (const float*)m.upload(a2, (size_t)cout * 4);
  return mw.w && mw.b && mw.a;
}

#define GETW(dst, wmref, name, numel)                                                        \
  const float* dst = (wmref).get(name, numel);                                               \
  if (!dst) return fail(VNF_E_MISSING, std::string("mtcnn: missing weight ") + (wmref).missing);
#define UP(ptr, numel) (const float*)m->upload(ptr, (size_t)(numel) * 4)

}  // namespace vnf
using namespace vnf;

extern "C" int vnf_mtcnn_create(const vnf_tensor_desc* pnet, int n_pnet, const vnf_tensor_desc* rnet, int n_rnet,
                                const vnf_tensor_desc* onet, int n_onet, const vnf_mtcnn_cfg* cfg, vnf_handle* out) {
  try {
    if (!pnet || !rnet || !onet || !cfg || !out) return fail(VNF_E_INVALID, "vnf_mtcnn_create: bad argument");
    if (cfg->min_face_size < 1 || cfg->max_batch < 1 || cfg->max_height < 12 || cfg->max_width < 12 ||
        !(cfg->factor > 0.f && cfg->factor < 1.f))
      return fail(VNF_E_INVALID, "vnf_mtcnn_create: bad configuration");
    *out = nullptr;
    auto m = std::make_unique<Mtcnn>();
    m->cfg = *cfg;
    (void)hipGetDevice(&m->device);
    WeightMap wp(pnet, n_pnet), wr(rnet, n_rnet), wo(onet, n_onet);
    {
      GETW(c1, wp, "conv1.weight", 270) GETW(b1, wp, "conv1.bias", 10) GETW(a1, wp, "prelu1.weight", 10)
      GETW(c2, wp, "conv2.weight", 1440) GETW(b2, wp, "conv2.bias", 16) GETW(a2, wp, "prelu2.weight", 16)
      GETW(c3, wp, "conv3.weight", 4608) GETW(b3, wp, "conv3.bias", 32) GETW(a3, wp, "prelu3.weight", 32)
      GETW(c41, wp, "conv4_1.weight", 64) GETW(b41, wp, "conv4_1.bias", 2)
      GETW(c42, wp, "conv4_2.weight", 128) GETW(b42, wp, "conv4_2.bias", 4)
      m->pw.w1 = up_transposed(*m, c1, 10, 3, 3); m->pw.b1 = UP(b1, 10); m->pw.a1 = UP(a1, 10);
      m->pw.w2 = up_transposed(*m, c2, 16, 10, 3); m->pw.b2 = UP(b2, 16); m->pw.a2 = UP(a2, 16);
      m->pw.w3 = up_transposed(*m, c3, 32, 16, 3); m->pw.b3 = UP(b3, 32); m->pw.a3 = UP(a3, 32);
      m->pw.w41 = up_transposed(*m, c41, 2, 32, 1); m->pw.b41 = UP(b41, 2);
      m->pw.w42 = up_transposed(*m, c42, 4, 32, 1); m->pw.b42 = UP(b42, 4);
    }
    // switches of the environment: read here, once per handle
    auto env_int = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    // VNF_MTCNN_DTYPE=f32 keeps the R/O-Net plans (and conv1 in net_front_kernel) on the exact-f32 MFMA; the default is
    // split-f16 (two 16-bit MFMAs per product, ~22 significant bits) for every layer of both nets
    const bool plans_f32 = getenv("VNF_MTCNN_DTYPE") && !strcmp(getenv("VNF_MTCNN_DTYPE"), "f32");
    const bool mid_env = env_int("VNF_MTCNN_MID", 1) != 0;
    m->spec_on = env_int("VNF_MTCNN_SPEC", 1) != 0;
    m->layers = getenv("VNF_MTCNN_LAYERS") != nullptr;
    m->fin_fast = std::max(0, std::min(FIN_FAST, env_int("VNF_FIN_FAST", FIN_FAST)));
    NetStage &rn = m->rnet, &on = m->onet;
    {
      rn.S = 24; rn.hw = 8; rn.nf = 5;
      rn.crop_name = "crop_resize_24"; rn.front_name = "rnet_front"; rn.net_name = "rnet"; rn.post_name = "stage2_post";
      on.S = 48; on.hw = 16; on.nf = 15;
      on.crop_name = "crop_resize_48"; on.front_name = "onet_front"; on.net_name = "onet"; on.post_name = "stage3_post";
      rn.cap = std::min(cfg->max_batch * KEEP, 8192);
      on.cap = std::min(cfg->max_batch * KEEP, 2048);
      rn.enc = std::make_unique<Encoder>();
      rn.enc->max_streams = 1;  // the detector shares the GPU with the embedding stream: no forks of its own
      rn.enc->tune_batch = std::max(1, rn.cap / 2);  // typical stage-2 load, not the capacity
      rn.enc->arch = ARCH_RNET; rn.enc->dtype = plans_f32 ? F32 : F16X2; rn.enc->max_batch = rn.cap;
      if (!pack_front(*m, wr, 28, rn.fw) || !pack_front(*m, wo, 32, on.fw)) return fail(VNF_E_MISSING, "mtcnn: conv1 weights");
      m->mid = mid_env && rn.enc->dtype == F16X2;
      if (m->mid && (!pack_mid(*m, wr, 48, 28, rn.mw) || !pack_mid(*m, wo, 64, 32, on.mw)))
        return fail(VNF_E_MISSING, "mtcnn: conv2 weights");
      int rr = build_rnet(*rn.enc, wr, m->mid, rn.bufs);
      if (rr == VNF_OK) rr = rn.enc->finalize();
      on.enc = std::make_unique<Encoder>();
      on.enc->max_streams = 1;
      on.enc->tune_batch = std::max(1, on.cap / 4);
      on.enc->arch = ARCH_ONET; on.enc->dtype = rn.enc->dtype; on.enc->max_batch = on.cap;
      if (rr == VNF_OK) rr = build_onet(*on.enc, wo, m->mid, on.bufs);
      if (rr == VNF_OK) rr = on.enc->finalize();
      if (rr != VNF_OK) return rr;
    }
    const int B = cfg->max_batch;
    m->cap_table = make_levels(cfg->max_height, cfg->max_width, cfg->min_face_size, (double)cfg->factor);
    // other aspect ratios up to the same bounds can need slightly more: 10 % head-room
    m->cap_px = (size_t)(m->cap_table.tot_px * 1.1) + 4096; m->cap_p1 = (size_t)(m->cap_table.tot_p1 * 1.1) + 4096;
    m->cap_c2 = (size_t)(m->cap_table.tot_c2 * 1.1) + 4096; m->cap_out = (size_t)(m->cap_table.tot_out * 1.1) + 4096;
    {
      int rows_cap = 0;
      for (int l = 0; l < m->cap_table.n; ++l) rows_cap += m->cap_table.l[l].Hs;
      m->row_order_cap = (int)(rows_cap * 1.1) + 64;
      m->row_order = (int*)m->dalloc((size_t)m->row_order_cap * 4);
      if (!m->row_order) return VNF_E_HIP;
    }
    m->lvl = (float*)m->dalloc(m->cap_px * 3 * B * 4);
    m->p1 = (float*)m->dalloc(m->cap_p1 * 10 * B * 4);
    m->c2 = (float*)m->dalloc(m->cap_c2 * 16 * B * 4);
    const size_t nseg = (size_t)MAX_LEVELS * B;
    // rows per frame of the stage-2 / stage-3 tables: run-time (max_candidates), at least the LDS fast-path size
    m->keep = std::max(KEEP, cfg->max_candidates);
    const size_t KR = (size_t)m->keep;
    m->cand = (Cand*)m->dalloc((size_t)B * m->cap_out * sizeof(Cand));
    m->cells = (int*)m->dalloc((size_t)B * m->cap_out * 4);
    m->keep1c = (int*)m->dalloc((size_t)B * m->cap_out * 4);
    m->cand_cnt = (int*)m->dalloc((nseg * 2 + (size_t)B * 3 + 16) * 4);
    m->keep1_cnt = m->cand_cnt + nseg;
    m->row_cnt = m->keep1_cnt + nseg;
    m->row3_cnt = m->row_cnt + B;
    m->fin_cnt = m->row3_cnt + B;
    m->status = m->fin_cnt + B;
    m->rows = (Row*)m->dalloc((size_t)B * KR * sizeof(Row));
    m->rows3 = (Row*)m->dalloc((size_t)B * KR * sizeof(Row));
    rn.out = (float*)m->dalloc((size_t)B * KR * 5 * 4);
    on.out = (float*)m->dalloc((size_t)B * KR * 15 * 4);
    m->fin = (float*)m->dalloc((size_t)B * KR * 15 * 4);
    {
      // NMS scratch in global memory (lists longer than the LDS tables): per frame max(cells of the pyramid, rows)
      const size_t st = std::max(m->cap_out, KR);
      m->scratch.stride = (int)st;
      m->scratch.keys = (unsigned long long*)m->dalloc((size_t)B * st * 8);
      m->scratch.kbox = (float4*)m->dalloc((size_t)B * st * 16);
      m->scratch.keep = (int*)m->dalloc((size_t)B * st * 4);
      m->scratch.reg = (float4*)m->dalloc((size_t)B * st * 16);
      if (!m->scratch.keys || !m->scratch.kbox || !m->scratch.keep || !m->scratch.reg || !m->cells || !m->keep1c) return VNF_E_HIP;
    }
    {
      const size_t sb = ((size_t)B * 3 + 16) * 4 + (size_t)B * FIN_FAST * 15 * 4;
      m->stage = (float*)m->dalloc(sb);
      if (hipHostMalloc((void**)&m->h_pin, sb, hipHostMallocDefault) != hipSuccess) m->h_pin = nullptr;
      if (!m->stage || !m->h_pin) return fail(VNF_E_HIP, "mtcnn: read-back buffers");
    }
    m->offs = (int*)m->dalloc((size_t)(B + 1) * 4);
    if (!m->lvl || !m->p1 || !m->c2 || !m->cand || !m->cand_cnt || !m->rows || !m->rows3 ||
        !rn.out || !on.out || !m->fin || !m->pw.w1)
      return VNF_E_HIP;
    // The launchers opt their kernels in to the dynamic LDS they ask for (above 64 KiB this is needed; gfx950 has 160 KiB
    // per workgroup); a device that reports less than the largest request is refused here.
    {
      int lds_max = 0;
      VNF_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, m->device));
      if (lds_max < MTCNN_LDS_MAX)
        return fail(VNF_E_INVALID, "mtcnn: device reports " + std::to_string(lds_max) + " B of LDS per workgroup, need " + std::to_string(MTCNN_LDS_MAX));
    }
    VNF_HIP(hipDeviceSynchronize());
    *out = reinterpret_cast<vnf_handle>(static_cast<HandleBase*>(m.release()));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

// per-stage device time + algorithmic bytes of one call (vnf_mtcnn_stage_times): events between the stages' launches
struct StageProf {
  std::vector<std::string> name;
  std::vector<double> bytes;
  std::vector<hipEvent_t> ev;
  void mark(const char* n, double b, hipStream_t s) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, s);
    name.push_back(n); bytes.push_back(b); ev.push_back(e);
  }
  ~StageProf() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

// one detection: what every step of the cascade needs
struct RunCtx {
  Mtcnn* m;
  const uint8_t* frames;
  int B, H, W;
  LevelTable t;
  hipStream_t s;
  StageProf* prof;
  // a mark closes the stage named in it: its time is the span since the previous mark
  void mark(const char* n, double bytes = 0) const { if (prof) prof->mark(n, bytes, s); }
  int ncnt() const { return m->cfg.max_batch * 3 + 16; }   // the counts block: row_cnt, row3_cnt, fin_cnt, status
};

// dispatch order of pyramid_rows_kernel's workgroups, rebuilt when the frame size changes
static int order_rows(const RunCtx& c) {
  Mtcnn* m = c.m;
  const LevelTable& t = c.t;
  int rows = 0;
  for (int l = 0; l < t.n; ++l) rows += t.l[l].Hs;
  if (rows > m->row_order_cap) return fail(VNF_E_CAPACITY, "mtcnn: pyramid exceeds handle capacity");
  if (m->row_order_h == c.H && m->row_order_w == c.W) return VNF_OK;
  std::vector<std::pair<long long, int>> ord;     // (first input row, tall bins first) -> (level << 16 | row)
  for (int l = 0; l < t.n; ++l)
    for (int i = 0; i < t.l[l].Hs; ++i) {
      const long long h0 = ((long long)i * c.H) / t.l[l].Hs;
      ord.push_back({h0 * 64 + (63 - std::min(l, 63)), (l << 16) | i});
    }
  std::sort(ord.begin(), ord.end());
  std::vector<int> packed(ord.size());
  for (size_t k = 0; k < ord.size(); ++k) packed[k] = ord[k].second;
  VNF_HIP(hipMemcpyAsync(m->row_order, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, c.s));
  VNF_HIP(hipStreamSynchronize(c.s));              // the host vector goes away; happens once per frame size
  m->row_order_h = c.H; m->row_order_w = c.W;
  return VNF_OK;
}

// pyramid, P-Net and both NMS passes of stage 1 -> rows / row_cnt
static int stage1(const RunCtx& c) {
  Mtcnn* m = c.m;
  const LevelTable& t = c.t;
  const int B = c.B, cap_out = (int)m->cap_out;
  const bool by_rows = pyramid_by_rows(c.frames, c.W);
  if (by_rows) {
    const int r = order_rows(c);
    if (r != VNF_OK) return r;
  }
  VNF_HIP(launch_pyramid(c.frames, B, c.H, c.W, t, m->lvl, by_rows ? m->row_order : nullptr, c.s));
  // algorithmic bytes per launch: what each kernel must read + write once (SURVEY.md 8d terms, from the level table)
  const double fB = (double)B;
  c.mark("pyramid", fB * ((double)c.H * c.W * 3 + (double)t.tot_px * 12));
  VNF_HIP(launch_pnet_conv1_pool(m->lvl, B, t, m->pw, m->p1, c.s));
  c.mark("pnet_conv1_pool", fB * ((double)t.tot_px * 12 + (double)t.tot_p1 * 40));
  VNF_HIP(launch_pnet_conv2(m->p1, B, t, m->pw, m->c2, c.s));
  c.mark("pnet_conv2", fB * ((double)t.tot_p1 * 40 + (double)t.tot_c2 * 64));
  VNF_HIP(launch_pnet_conv3_heads(m->c2, B, t, m->pw, m->cfg.thresholds[0], cap_out, m->cand, m->cells, m->cand_cnt, m->prob_dbg,
                                  m->reg_dbg, c.s));
  c.mark("pnet_conv3_heads", fB * (double)t.tot_c2 * 64);
  VNF_HIP(launch_nms_stage1(m->cand, m->cells, m->cand_cnt, t, B, cap_out, c.H, c.W, m->keep, m->keep1c, m->keep1_cnt, m->rows,
                            m->row_cnt, m->status, m->scratch, c.s));
  c.mark("nms_stage1");
  return VNF_OK;
}

// after a read-back into h_pin: did a stage-1 list outgrow its table?
static int check_overflow(const Mtcnn* m) {
  const int st = m->h_pin[m->cfg.max_batch * 3];
  if (stage_tables_overflowed(st))
    return fail(VNF_E_CAPACITY, "mtcnn: candidate table overflow (status " + std::to_string(st) + "): a frame has more than " +
                                std::to_string(m->keep) + " stage-1 survivors; raise vnf_mtcnn_cfg.max_candidates");
  return VNF_OK;
}

// pinned h_pin: the copy is a true async DMA, the only wait is the stream synchronisation
static int read_counts(const RunCtx& c) {
  VNF_HIP(hipMemcpyAsync(c.m->h_pin, c.m->row_cnt, (size_t)c.ncnt() * 4, hipMemcpyDeviceToHost, c.s));
  VNF_HIP(hipStreamSynchronize(c.s));
  return check_overflow(c.m);
}

// ---- stages 2 and 3 as launch sequences sized by (largest per-frame candidate count, total candidates): every kernel
// reads the true counts from device memory and leaves early past them, so any UPPER bound gives the exact result (the
// nets then also run on the unused tail rows of the dense batch); an under-estimate leaves candidates out and is
// detected after the read-back.
// nets on the MFMA core: candidates of all frames form one dense batch, processed in chunks of `net.cap`
static int run_net(const RunCtx& c, const NetStage& net, const Row* rows, const int* cnt, int maxc, int total) {
  Mtcnn* m = c.m;
  const bool split = net.enc->dtype == F16X2;
  VNF_HIP(launch_prefix_offsets(cnt, c.B, m->offs, c.s));
  for (int c0 = 0; c0 < total; c0 += net.cap) {
    const int n = std::min(net.cap, total - c0);
    VNF_HIP(launch_crop_resize(c.frames, c.B, c.H, c.W, rows, cnt, maxc, net.S, net.buf(net.bufs.crops), m->status, m->offs, c0, n,
                               m->keep, c.s));
    c.mark(net.crop_name, (double)n * net.S * net.S * 16);  // output bytes only (NHWC4 fp32)
    VNF_HIP(launch_net_front(net.S, split, net.buf(net.bufs.crops), net.fw, net.buf(net.bufs.pooled1), n, c.s));
    c.mark(net.front_name);
    if (m->mid)   // conv2 + PReLU + pool2 (the plan starts at conv3)
      VNF_HIP(launch_net_mid(net.S, net.buf(net.bufs.pooled1), net.mw, net.buf(net.bufs.pooled2), n, c.s));
    std::string rep;
    const int rc = net.enc->run(nullptr, n, VNF_F32, nullptr, c.s, c.prof && m->layers ? &rep : nullptr);
    if (rc != VNF_OK) return rc;
    if (!rep.empty()) fprintf(stderr, "%s n=%d\n%s", net.net_name, n, rep.c_str());
    c.mark(net.net_name);
    VNF_HIP(launch_heads_scatter(net.buf(net.bufs.heads), net.hw, m->offs, cnt, maxc, c.B, c0, n, net.out, net.nf, split, m->keep, c.s));
  }
  return VNF_OK;
}

static int stage2(const RunCtx& c, int max2, int total2) {
  Mtcnn* m = c.m;
  const int rc = run_net(c, m->rnet, m->rows, m->row_cnt, max2, total2);
  if (rc != VNF_OK) return rc;
  VNF_HIP(launch_stage2_post(m->rows, m->row_cnt, m->rnet.out, m->cfg.thresholds[1], c.B, c.H, c.W, m->keep, m->rows3, m->row3_cnt,
                             m->status, m->scratch, c.s));
  c.mark(m->rnet.post_name);
  return VNF_OK;
}

// the result rows of this call, packed for the one-copy read-back
static int pack_results(const RunCtx& c) {
  Mtcnn* m = c.m;
  m->last_b = c.B;
  VNF_HIP(launch_pack_results(m->row_cnt, c.ncnt(), m->fin, m->fin_cnt, c.B, m->keep, m->stage, c.s));
  return VNF_OK;
}

static int stage3(const RunCtx& c, int max3, int total3) {
  Mtcnn* m = c.m;
  int rc = run_net(c, m->onet, m->rows3, m->row3_cnt, max3, total3);
  if (rc != VNF_OK) return rc;
  VNF_HIP(launch_stage3_post(m->rows3, m->row3_cnt, m->onet.out, m->cfg.thresholds[2], m->cfg.select_largest, c.B, m->keep, m->fin,
                             m->fin_cnt, m->status, m->scratch, c.s));
  rc = pack_results(c);
  if (rc != VNF_OK) return rc;
  c.mark(m->onet.post_name);
  return VNF_OK;
}

static int readback(const RunCtx& c) {
  VNF_HIP(hipMemcpyAsync(c.m->h_pin, c.m->stage, ((size_t)c.ncnt() + (size_t)c.B * FIN_FAST * 15) * 4, hipMemcpyDeviceToHost, c.s));
  VNF_HIP(hipStreamSynchronize(c.s));
  c.mark("readback");
  return check_overflow(c.m);
}

// largest per-frame count and total of the B counts at h_pin[base]
struct Counts { int max = 0, total = 0; };
static Counts counts_of(const RunCtx& c, int base) {
  Counts n;
  for (int i = 0; i < c.B; ++i) { n.max = std::max(n.max, c.m->h_pin[base + i]); n.total += c.m->h_pin[base + i]; }
  return n;
}

// an estimate with head room, in whole tiles of the nets' batch dimension
static int padded(int v, int limit) { return std::min(limit, ((v + v / 8 + 8 + 15) / 16) * 16); }

// Stages 2 / 3 and the read-back after stage 1 has been launched; leaves the counts block and the packed rows in h_pin.
static int stages23(const RunCtx& c) {
  Mtcnn* m = c.m;
  const int B = c.B, KR = m->keep, MB = m->cfg.max_batch;
  // Sizes of stages 2 / 3 WITHOUT asking the device (the reference synchronises at both stage boundaries to shape its
  // tensors, detect_face.py:96-146): a video stream's candidate counts move slowly, so the previous call's counts plus
  // head room size this call's launches, and the one read-back at the end tells whether they covered it.  If not (or on
  // the first call of a frame size) stage-1's counts are read and stages 2 / 3 run with exact bounds: stage 2 by its
  // own counts, stage 3 by stage 2's (it only filters stage-2 rows) -- never a second mid-cascade synchronisation.
  Mtcnn::Spec& sp = m->spec;
  int r = VNF_OK;
  bool exact_needed = true;
  if (m->spec_on && sp.valid && sp.b == B && sp.H == c.H && sp.W == c.W) {
    r = stage2(c, sp.max2, sp.total2);
    if (r == VNF_OK) r = stage3(c, sp.max3, sp.total3);
    if (r == VNF_OK) r = readback(c);
    if (r != VNF_OK) return r;
    const Counts n2 = counts_of(c, 0), n3 = counts_of(c, MB);
    exact_needed = n2.max > sp.max2 || n2.total > sp.total2 || n3.max > sp.max3 || n3.total > sp.total3;
  } else {
    r = read_counts(c);
    if (r != VNF_OK) return r;
    c.mark("host_sync_1");
  }
  if (exact_needed) {
    // h[0..B) = stage-1 counts (from read_counts, or from the read-back of the speculative pass: stage 1 is not re-run)
    const Counts n2 = counts_of(c, 0);
    if (n2.max > 0) {
      r = stage2(c, n2.max, n2.total);
      if (r == VNF_OK) r = stage3(c, n2.max, n2.total);      // stage-3 rows are a subset of stage-2 rows: exact upper bounds
    } else {
      r = pack_results(c);
    }
    if (r == VNF_OK) r = readback(c);
    if (r != VNF_OK) return r;
  }
  const Counts n2 = counts_of(c, 0), n3 = counts_of(c, MB);
  sp.valid = true; sp.b = B; sp.H = c.H; sp.W = c.W;
  sp.max2 = padded(n2.max, KR); sp.total2 = padded(n2.total, B * KR);
  sp.max3 = padded(n3.max, KR); sp.total3 = padded(n3.total, B * KR);
  return VNF_OK;
}

static int mtcnn_run(Mtcnn* m, const uint8_t* frames, int b, int H, int W, hipStream_t s, std::vector<int>& cnt,
                     std::vector<float>& fin, StageProf* prof = nullptr) {
  const vnf_mtcnn_cfg& cfg = m->cfg;
  if (b > cfg.max_batch || H > cfg.max_height || W > cfg.max_width) return fail(VNF_E_CAPACITY, "mtcnn: frame batch exceeds handle capacity");
  const RunCtx c{m, frames, b, H, W, make_levels(H, W, cfg.min_face_size, (double)cfg.factor), s, prof};
  const LevelTable& t = c.t;
  m->last_b = 0;
  cnt.assign(b, 0);
  fin.clear();
  if (t.n == 0) return VNF_OK;  // image smaller than one cell: no detections
  if ((size_t)t.tot_px > m->cap_px || (size_t)t.tot_p1 > m->cap_p1 || (size_t)t.tot_c2 > m->cap_c2 || (size_t)t.tot_out > m->cap_out)
    return fail(VNF_E_CAPACITY, "mtcnn: pyramid exceeds handle capacity");
  const size_t nseg = (size_t)MAX_LEVELS * cfg.max_batch;
  VNF_HIP(hipMemsetAsync(m->cand_cnt, 0, (nseg * 2 + (size_t)cfg.max_batch * 3 + 16) * 4, s));
  c.mark("begin");
  int r = stage1(c);
  if (r == VNF_OK) r = stages23(c);
  if (r != VNF_OK) return r;
  const int* h = m->h_pin;
  int maxf = 0;
  for (int i = 0; i < b; ++i) { cnt[i] = h[2 * cfg.max_batch + i]; maxf = std::max(maxf, cnt[i]); }
  if (maxf == 0) return VNF_OK;
  fin.resize((size_t)b * maxf * 15);
  if (maxf <= m->fin_fast) {
    const float* rows = reinterpret_cast<const float*>(h + c.ncnt());
    for (int i = 0; i < b; ++i)
      memcpy(&fin[(size_t)i * maxf * 15], rows + (size_t)i * FIN_FAST * 15, (size_t)maxf * 15 * 4);
    return VNF_OK;
  }
  VNF_HIP(hipMemcpy2DAsync(fin.data(), (size_t)maxf * 15 * 4, m->fin, (size_t)m->keep * 15 * 4, (size_t)maxf * 15 * 4, b,
                           hipMemcpyDeviceToHost, s));
  VNF_HIP(hipStreamSynchronize(s));
  return VNF_OK;
}

extern "C" int vnf_mtcnn_detect(vnf_handle h, const uint8_t* frames, int b, int height, int width, int32_t* counts,
                                float* boxes, float* probs, float* points, int max_out, int32_t* n_out, void* stream) {
  try {
    Mtcnn* m = handle_cast<Mtcnn>(h);
    if (!m) return fail(VNF_E_INVALID, "not an MTCNN handle");
    if (!frames || b <= 0 || !counts || !n_out) return fail(VNF_E_INVALID, "vnf_mtcnn_detect: bad argument");
    std::vector<int> cnt;
    std::vector<float> fin;
    int r = mtcnn_run(m, frames, b, height, width, (hipStream_t)stream, cnt, fin);
    if (r != VNF_OK) return r;
    int maxf = 0;
    r = count_results("vnf_mtcnn_detect", cnt.data(), b, counts, max_out, n_out, &maxf);
    if (r == VNF_OK && maxf > 0) scatter_rows(fin.data(), maxf, cnt.data(), b, boxes, probs, points);   // fin is (b, maxf, 15)
    return r;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

// One detection with HIP events between the cascade's stages (on the caller's stream): a text table, one line per
// stage "name ms algorithmic_bytes" (bytes 0 where the stage is not bandwidth-priced).  Synchronises.
extern "C" int vnf_mtcnn_stage_times(vnf_handle h, const uint8_t* frames, int b, int height, int width, char* report,
                                     int64_t capacity, void* stream) {
  try {
    Mtcnn* m = handle_cast<Mtcnn>(h);
    if (!m) return fail(VNF_E_INVALID, "not an MTCNN handle");
    if (!frames || b <= 0 || !report || capacity <= 0) return fail(VNF_E_INVALID, "vnf_mtcnn_stage_times: bad argument");
    std::vector<int> cnt;
    std::vector<float> fin;
    StageProf prof;
    int r = mtcnn_run(m, frames, b, height, width, (hipStream_t)stream, cnt, fin, &prof);
    if (r != VNF_OK) return r;
    VNF_HIP(hipStreamSynchronize((hipStream_t)stream));
    std::string rep;
    char line[160];
    for (size_t i = 1; i < prof.ev.size(); ++i) {
      float ms = 0;
      VNF_HIP(hipEventElapsedTime(&ms, prof.ev[i - 1], prof.ev[i]));
      snprintf(line, sizeof line, "%s %.6f %.0f\n", prof.name[i].c_str(), ms, prof.bytes[i]);
      rep += line;
    }
    strncpy(report, rep.c_str(), (size_t)capacity - 1);
    report[capacity - 1] = 0;
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

extern "C" int vnf_mtcnn_results_device(vnf_handle h, int32_t* frame_idx, float* boxes, float* probs, float* points,
                                        int max_out, void* stream) {
  Mtcnn* m = handle_cast<Mtcnn>(h);
  if (!m) return fail(VNF_E_INVALID, "not an MTCNN handle");
  return results_device("vnf_mtcnn_results_device", m->fin, m->fin_cnt, m->last_b, m->keep, frame_idx, boxes, probs, points, max_out, stream);
}

// Staged-parity hook for the O-stage decode alone (detect_face.py:148-169 + mtcnn.py:334-340): runs stage3_post_kernel
// on a caller-made candidate table of ONE frame -- boxes (n,4) before bbreg and the O-Net outputs (n,15: face
// probability, 4 regression values, 5 x-landmarks, 5 y-landmarks) -- so a test can inject exactly tied scores.
// fin_out receives up to max_out rows [x1,y1,x2,y2,score, 10 landmark coordinates].  Synchronises.
extern "C" int vnf_mtcnn_debug_stage3(vnf_handle h, const float* boxes, const float* onet_out, int n, float* fin_out,
                                      int max_out, int32_t* n_out, void* stream) {
  try {
    Mtcnn* m = handle_cast<Mtcnn>(h);
    if (!m) return fail(VNF_E_INVALID, "not an MTCNN handle");
    if (!boxes || !onet_out || n < 0 || !fin_out || !n_out) return fail(VNF_E_INVALID, "vnf_mtcnn_debug_stage3: bad argument");
    if (n > m->keep) return fail(VNF_E_CAPACITY, "vnf_mtcnn_debug_stage3: more rows than the handle's tables hold");
    hipStream_t s = (hipStream_t)stream;
    std::vector<Row> rows((size_t)std::max(n, 1));
    for (int i = 0; i < n; ++i) {
      Row r{};
      r.x1 = boxes[i * 4]; r.y1 = boxes[i * 4 + 1]; r.x2 = boxes[i * 4 + 2]; r.y2 = boxes[i * 4 + 3];
      rows[i] = r;
    }
    VNF_HIP(hipMemcpyAsync(m->rows3, rows.data(), (size_t)n * sizeof(Row), hipMemcpyHostToDevice, s));
    VNF_HIP(hipMemcpyAsync(m->onet.out, onet_out, (size_t)n * 15 * 4, hipMemcpyHostToDevice, s));
    VNF_HIP(hipMemcpyAsync(m->row3_cnt, &n, 4, hipMemcpyHostToDevice, s));
    VNF_HIP(hipMemsetAsync(m->status, 0, 4, s));
    VNF_HIP(launch_stage3_post(m->rows3, m->row3_cnt, m->onet.out, m->cfg.thresholds[2], m->cfg.select_largest, 1, m->keep, m->fin,
                               m->fin_cnt, m->status, m->scratch, s));
    int nk = 0;
    VNF_HIP(hipMemcpyAsync(&nk, m->fin_cnt, 4, hipMemcpyDeviceToHost, s));
    VNF_HIP(hipStreamSynchronize(s));
    *n_out = nk;
    if (nk > max_out) return fail(VNF_E_CAPACITY, "vnf_mtcnn_debug_stage3: more rows than max_out");
    VNF_HIP(hipMemcpy(fin_out, m->fin, (size_t)nk * 15 * 4, hipMemcpyDeviceToHost));
    m->last_b = 0;
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

// Staged-parity hook: dense P-Net maps of one pyramid level for frame 0 of a batch (test use).
extern "C" int vnf_mtcnn_debug_pnet(vnf_handle h, const uint8_t* frames, int height, int width, int level,
                                    float* level_out, float* prob_out, float* reg_out, int32_t dims[4], void* stream) {
  try {
    Mtcnn* m = handle_cast<Mtcnn>(h);
    if (!m) return fail(VNF_E_INVALID, "not an MTCNN handle");
    LevelTable t = make_levels(height, width, m->cfg.min_face_size, (double)m->cfg.factor);
    if (level < 0 || level >= t.n) return fail(VNF_E_INVALID, "no such level");
    // the dense maps live for this call only: on every way out they are freed and the handle forgets them
    struct Maps {
      Mtcnn* m;
      float *pd = nullptr, *rd = nullptr;
      ~Maps() { m->prob_dbg = m->reg_dbg = nullptr; (void)hipFree(pd); (void)hipFree(rd); }
    } maps{m};
    float *&pd = maps.pd, *&rd = maps.rd;
    VNF_HIP(hipMalloc(&pd, (size_t)t.tot_out * 4 * m->cfg.max_batch));
    VNF_HIP(hipMalloc(&rd, (size_t)t.tot_out * 16 * m->cfg.max_batch));
    m->prob_dbg = pd; m->reg_dbg = rd;
    std::vector<int> cnt;
    std::vector<float> fin;
    int r = mtcnn_run(m, frames, 1, height, width, (hipStream_t)stream, cnt, fin);
    if (r == VNF_OK) {
      const LevelDesc& L = t.l[level];
      dims[0] = L.Hs; dims[1] = L.Ws; dims[2] = L.oh; dims[3] = L.ow;
      hipError_t e = hipSuccess;
      if (level_out)
        for (int c = 0; c < 3 && e == hipSuccess; ++c)
          e = hipMemcpy(level_out + (size_t)c * L.Hs * L.Ws, m->lvl + (size_t)c * t.tot_px + L.off_px, (size_t)L.Hs * L.Ws * 4, hipMemcpyDeviceToHost);
      if (prob_out && e == hipSuccess) e = hipMemcpy(prob_out, pd + L.off_out, (size_t)L.oh * L.ow * 4, hipMemcpyDeviceToHost);
      if (reg_out)
        for (int c = 0; c < 4 && e == hipSuccess; ++c)
          e = hipMemcpy(reg_out + (size_t)c * L.oh * L.ow, rd + (size_t)c * t.tot_out + L.off_out, (size_t)L.oh * L.ow * 4, hipMemcpyDeviceToHost);
      if (e != hipSuccess) r = fail(VNF_E_HIP, hipGetErrorString(e));
    }
    return r;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

// the net a debug hook names: 2 = R-Net, 3 = O-Net
static NetStage* debug_net_of(Mtcnn* m, int net) { return net == 2 ? &m->rnet : net == 3 ? &m->onet : nullptr; }

// Staged-parity hook for R-Net / O-Net on their own: the caller's rectangles become the candidate table of stage 2
// (net 2) or stage 3 (net 3) and run_net -- the cascade's own launch sequence -- processes it.  vnface.h has the layout.
extern "C" int vnf_mtcnn_debug_net(vnf_handle h, int net, const uint8_t* frames, int b, int height, int width,
                                   const int32_t* rects, const int32_t* counts, float* table_out, int32_t* status_out,
                                   void* stream) {
  try {
    Mtcnn* m = handle_cast<Mtcnn>(h);
    if (!m) return fail(VNF_E_INVALID, "not an MTCNN handle");
    m->last_b = 0; m->spec.valid = false; m->dbg = {};   // whatever comes of this call, the taps and results of earlier ones are gone
    const NetStage* ns = debug_net_of(m, net);
    if (!ns) return fail(VNF_E_INVALID, "vnf_mtcnn_debug_net: net " + std::to_string(net) + " is neither 2 (R-Net) nor 3 (O-Net)");
    if (!frames || b <= 0 || height <= 0 || width <= 0 || !counts || !status_out)
      return fail(VNF_E_INVALID, "vnf_mtcnn_debug_net: bad argument");
    if (b > m->cfg.max_batch || height > m->cfg.max_height || width > m->cfg.max_width)
      return fail(VNF_E_CAPACITY, "vnf_mtcnn_debug_net: " + std::to_string(b) + " frames of " + std::to_string(height) + " x " +
                                  std::to_string(width) + " exceed the handle's capacity (max_batch " + std::to_string(m->cfg.max_batch) + ")");
    int total = 0, maxc = 0;
    for (int i = 0; i < b; ++i) {
      if (counts[i] < 0) return fail(VNF_E_INVALID, "vnf_mtcnn_debug_net: negative count");
      if (counts[i] > m->keep)
        return fail(VNF_E_CAPACITY, "vnf_mtcnn_debug_net: frame " + std::to_string(i) + " has " + std::to_string(counts[i]) +
                                    " rectangles, the handle's tables hold " + std::to_string(m->keep) + " rows per frame");
      total += counts[i]; maxc = std::max(maxc, counts[i]);
    }
    if (total > 0 && (!rects || !table_out)) return fail(VNF_E_INVALID, "vnf_mtcnn_debug_net: bad argument");
    // the crop kernel reads the frame wherever a rectangle points: pad() keeps 1 <= y, ey <= H and 1 <= x, ex <= W
    for (int k = 0; k < total; ++k) {
      const int32_t* r = rects + (size_t)k * 4;
      if (r[0] < 1 || r[0] > height || r[1] < 1 || r[1] > height || r[2] < 1 || r[2] > width || r[3] < 1 || r[3] > width)
        return fail(VNF_E_INVALID, "vnf_mtcnn_debug_net: rectangle " + std::to_string(k) + " leaves the frame");
    }
    hipStream_t s = (hipStream_t)stream;
    *status_out = 0;
    if (total == 0) return VNF_OK;
    Row* drows = net == 2 ? m->rows : m->rows3;
    int* dcnt = net == 2 ? m->row_cnt : m->row3_cnt;
    std::vector<Row> rows((size_t)total);
    for (int k = 0; k < total; ++k) {
      Row r{};
      r.y = rects[k * 4]; r.ey = rects[k * 4 + 1]; r.x = rects[k * 4 + 2]; r.ex = rects[k * 4 + 3];
      rows[k] = r;
    }
    for (int i = 0, o = 0; i < b; o += counts[i], ++i)
      if (counts[i]) VNF_HIP(hipMemcpyAsync(drows + (size_t)i * m->keep, rows.data() + o, (size_t)counts[i] * sizeof(Row), hipMemcpyHostToDevice, s));
    VNF_HIP(hipMemcpyAsync(dcnt, counts, (size_t)b * 4, hipMemcpyHostToDevice, s));
    VNF_HIP(hipMemsetAsync(m->status, 0, 4, s));
    const RunCtx c{m, frames, b, height, width, LevelTable{}, s, nullptr};
    const int rc = run_net(c, *ns, drows, dcnt, maxc, total);
    VNF_HIP(hipStreamSynchronize(s));   // also on failure: `rows` and `counts` are still being read
    if (rc != VNF_OK) return rc;
    for (int i = 0, o = 0; i < b; o += counts[i], ++i)
      if (counts[i]) VNF_HIP(hipMemcpy(table_out + (size_t)o * ns->nf, ns->out + (size_t)i * m->keep * ns->nf, (size_t)counts[i] * ns->nf * 4, hipMemcpyDeviceToHost));
    VNF_HIP(hipMemcpy(status_out, m->status, 4, hipMemcpyDeviceToHost));
    m->dbg.net = net; m->dbg.c0 = ((total - 1) / ns->cap) * ns->cap; m->dbg.n = total - m->dbg.c0;
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

// does the handle's launch sequence write plan buffer `buf` of the net?  The detector's kernels write crops, pooled1 and
// (fused mid) pooled2, the plan what its convolutions and pools name
static bool net_writes(const Mtcnn* m, const NetStage& ns, int buf) {
  if (buf == ns.bufs.crops || buf == ns.bufs.pooled1 || (m->mid && buf == ns.bufs.pooled2)) return true;
  for (const Op& op : ns.enc->ops) {
    if (op.kind == Op::MAXPOOL && op.dst == buf) return true;
    if (op.kind != Op::CONV) continue;
    const ConvLayer& L = ns.enc->convs[op.layer];
    for (int i = 0; i < L.nseg; ++i)
      if (L.seg[i].buf == buf) return true;
  }
  return false;
}

// One plan buffer of the LAST chunk the previous vnf_mtcnn_debug_net processed, as raw 32-bit words (vnface.h).
extern "C" int vnf_mtcnn_debug_net_tap(vnf_handle h, int net, const char* name, void* raw_out, int64_t capacity_bytes,
                                       int32_t dims[6]) {
  try {
    Mtcnn* m = handle_cast<Mtcnn>(h);
    if (!m) return fail(VNF_E_INVALID, "not an MTCNN handle");
    const NetStage* ns = debug_net_of(m, net);
    if (!ns || !name || !dims) return fail(VNF_E_INVALID, "vnf_mtcnn_debug_net_tap: bad argument");
    const auto it = ns->enc->taps.find(name);
    if (it == ns->enc->taps.end()) return fail(VNF_E_INVALID, std::string("vnf_mtcnn_debug_net_tap: no such tap: ") + name);
    if (m->dbg.net != net)
      return fail(VNF_E_INVALID, "vnf_mtcnn_debug_net_tap: no vnf_mtcnn_debug_net call on net " + std::to_string(net) +
                                 " with candidates precedes the tap");
    if (!net_writes(m, *ns, it->second.buf))
      return fail(VNF_E_INVALID, std::string("vnf_mtcnn_debug_net_tap: '") + name + "' is computed inside the fused conv2 + pool2 kernel and "
                  "never reaches memory on this handle: create the detector under VNF_MTCNN_MID=0 (or VNF_MTCNN_DTYPE=f32) to read it");
    const Buf& bf = ns->enc->bufs[it->second.buf];
    dims[0] = m->dbg.n; dims[1] = bf.H; dims[2] = bf.W; dims[3] = bf.C;
    dims[4] = ns->enc->dtype == F16X2 && it->second.buf != ns->bufs.crops ? 1 : 0;   // the crops stay fp32 in every form
    dims[5] = m->dbg.c0;
    if (!raw_out) return VNF_OK;   // a size query
    const int64_t bytes = (int64_t)m->dbg.n * (int64_t)bf.elems_per_image() * 4;
    if (bytes > capacity_bytes) return fail(VNF_E_CAPACITY, "vnf_mtcnn_debug_net_tap: the tap holds " + std::to_string(bytes) + " bytes");
    VNF_HIP(hipMemcpy(raw_out, bf.ptr, (size_t)bytes, hipMemcpyDeviceToHost));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
