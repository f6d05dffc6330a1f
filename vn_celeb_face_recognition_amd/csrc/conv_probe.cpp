// One-convolution probe (vnf_conv_probe_*): a plan of exactly one Op::CONV, built with add_buf / add_conv / finalize
// like every other plan, whose launch the caller drives one tile configuration at a time on its own device buffers.
// It exists for the tests: every instantiation behind launch_conv can be run on a geometry of the caller's choosing and
// compared with a reference, which the whole-network tests (one tuned tile per layer) cannot do.
#include "plan.h"

namespace vnf {

struct ConvProbe : HandleBase {
  static constexpr HandleKind KIND = HandleKind::ConvProbe;
  ConvProbe() : HandleBase(KIND) {}
  Encoder enc;  // owns the packed weights, bias classes, slopes and the gather table
  vnf_conv_probe_geom g;
};

static int probe_dtype(const vnf_conv_probe_geom& g) {
  if (g.dtype == VNF_F16X2) return g.planar ? F16P : F16X2;
  return (g.dtype == VNF_F32 || g.dtype == VNF_BF16 || g.dtype == VNF_F16) ? g.dtype : -1;
}

// the launch arguments of the probe's convolution on the caller's buffers
static ConvArgs probe_args(const ConvProbe& p, const void* x, void* const* out, const void* res) {
  const Encoder& e = p.enc;
  const vnf_conv_probe_geom& g = p.g;
  const int es = dtype_size(e.dtype), oes = g.out_f32 ? 4 : es;
  ConvArgs a = e.conv_args(e.convs[0], 0, g.n);
  a.x = (const char*)x + (size_t)g.x_coff * es;
  for (int i = 0; i < g.nseg; ++i) a.seg[i].ptr = (char*)out[i] + (size_t)g.seg_coff[i] * oes;
  if (g.has_res) a.res = (const char*)res + (size_t)g.res_coff * es;
  return a;
}

}  // namespace vnf
using namespace vnf;

extern "C" int vnf_conv_probe_create(const vnf_conv_probe_geom* gp, const float* w, const float* bias, const float* slope,
                                     const float* pre_s, const float* pre_t, vnf_handle* out) {
  try {
    if (!out || !gp || !w) return fail(VNF_E_INVALID, "vnf_conv_probe_create: bad argument");
    *out = nullptr;
    const vnf_conv_probe_geom& g = *gp;
    const int dt = probe_dtype(g);
    if (dt < 0) return fail(VNF_E_INVALID, "vnf_conv_probe_create: bad dtype");
    if (g.n < 1 || g.h < 1 || g.w < 1 || g.cin < 1 || g.cout < 1 || g.kh < 1 || g.kw < 1 || g.sh < 1 || g.sw < 1 || g.ph < 0 ||
        g.pw < 0 || g.ph >= g.kh || g.pw >= g.kw || g.h + 2 * g.ph < g.kh || g.w + 2 * g.pw < g.kw)
      return fail(VNF_E_INVALID, "vnf_conv_probe_create: bad geometry");
    if (g.act != ACT_NONE && g.act != ACT_RELU && g.act != ACT_PRELU) return fail(VNF_E_INVALID, "vnf_conv_probe_create: bad act");
    if ((g.act == ACT_PRELU) != (slope != nullptr)) return fail(VNF_E_INVALID, "vnf_conv_probe_create: slopes go with PReLU");
    if ((pre_s != nullptr) != (pre_t != nullptr)) return fail(VNF_E_INVALID, "vnf_conv_probe_create: pre_s and pre_t go together");
    // the epilogue moves 8-channel chunks with 16-byte (2-byte layouts) or 2 x 16-byte accesses: every output and
    // residual slice starts and ends on a chunk; the input slice on the layout's unit (add_conv checks that one)
    if (g.x_coff < 0 || g.x_coff + g.cin > g.ldx) return fail(VNF_E_INVALID, "vnf_conv_probe_create: input slice outside its buffer");
    if (g.nseg < 1 || g.nseg > 4) return fail(VNF_E_INVALID, "vnf_conv_probe_create: 1 to 4 output segments");
    for (int i = 0; i < g.nseg; ++i) {
      const int c0 = g.seg_c0[i], c1 = g.seg_c1[i];
      if (c0 != (i ? g.seg_c1[i - 1] : 0) || c1 <= c0 || (i == g.nseg - 1 && c1 != g.cout) || c0 % 8 || c1 % 8 || g.seg_ld[i] % 8 ||
          g.seg_coff[i] % 8 || g.seg_coff[i] < 0 || g.seg_coff[i] + (c1 - c0) > g.seg_ld[i])
        return fail(VNF_E_INVALID, "vnf_conv_probe_create: output segments tile [0, cout) in 8-channel chunks inside their buffers");
    }
    if (g.has_res && (g.ldres % 8 || g.res_coff % 8 || g.res_coff < 0 || g.res_coff + g.cout > g.ldres))
      return fail(VNF_E_INVALID, "vnf_conv_probe_create: residual slice outside its buffer or off the 8-channel chunks");
    const int Ho = (g.h + 2 * g.ph - g.kh) / g.sh + 1, Wo = (g.w + 2 * g.pw - g.kw) / g.sw + 1;
    const size_t lim = (size_t)1 << 31;
    if ((size_t)g.n * g.h * g.w * (size_t)g.ldx >= lim) return fail(VNF_E_CAPACITY, "vnf_conv_probe_create: tensor too large");
    for (int i = 0; i < g.nseg; ++i)
      if ((size_t)g.n * Ho * Wo * (size_t)g.seg_ld[i] >= lim) return fail(VNF_E_CAPACITY, "vnf_conv_probe_create: tensor too large");
    if (g.has_res && (size_t)g.n * Ho * Wo * (size_t)g.ldres >= lim) return fail(VNF_E_CAPACITY, "vnf_conv_probe_create: tensor too large");

    ConvProbe* p = new ConvProbe();
    p->g = g;
    (void)hipGetDevice(&p->device);
    Encoder& e = p->enc;
    e.dtype = dt; e.max_batch = 1; e.in_size = 1; e.arch = ARCH_MLP;   // the plan's own buffers are never launched on
    e.device = p->device;
    ConvSpec s;
    s.name = "conv_probe";
    s.x_buf = e.add_buf(g.h, g.w, g.ldx);
    s.x_coff = g.x_coff; s.cin = s.cin_pad = g.cin;
    s.KH = g.kh; s.KW = g.kw; s.sh = g.sh; s.sw = g.sw; s.ph = g.ph; s.pw = g.pw;
    s.pieces.resize(1);
    Piece& pc = s.pieces[0];
    pc.w = w; pc.cout = pc.cout_pad = g.cout;
    if (bias) pc.bias.assign(bias, bias + g.cout);
    if (slope) pc.slope.assign(slope, slope + g.cout);
    for (int i = 0; i < g.nseg; ++i) s.segs.push_back({g.seg_c0[i], g.seg_c1[i], e.add_buf(Ho, Wo, g.seg_ld[i]), g.seg_coff[i]});
    if (g.has_res) { s.res_buf = e.add_buf(Ho, Wo, g.ldres); s.res_coff = g.res_coff; }
    s.act = g.act; s.out_f32 = g.out_f32 ? 1 : 0;
    std::vector<float> ps, pt;
    if (pre_s) {
      ps.assign(pre_s, pre_s + g.cin); pt.assign(pre_t, pre_t + g.cin);
      s.pre_s = &ps; s.pre_t = &pt;
    }
    int r = add_conv(e, s);
    if (r == VNF_OK) r = e.finalize();
    if (r != VNF_OK) { delete p; return r; }
    VNF_HIP(hipDeviceSynchronize());
    *out = reinterpret_cast<vnf_handle>(static_cast<HandleBase*>(p));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

extern "C" int vnf_conv_probe_cfgs(vnf_handle h, int32_t* admitted, int capacity, int32_t family_sizes[3]) {
  try {
    ConvProbe* p = handle_cast<ConvProbe>(h);
    if (!p) return fail(VNF_E_INVALID, "not a conv probe handle");
    const int total = conv_num_cfgs();
    if (family_sizes) {
      int fs[3];
      conv_family_sizes(fs);
      for (int i = 0; i < 3; ++i) family_sizes[i] = fs[i];
    }
    if (admitted) {
      if (capacity < total) return fail(VNF_E_CAPACITY, "vnf_conv_probe_cfgs: capacity below the number of configurations");
      // conv_cfg_ok looks at the geometry, the dtype and the packed sizes only: no pointer of the launch matters
      void* const none[4] = {nullptr, nullptr, nullptr, nullptr};
      const ConvArgs a = probe_args(*p, nullptr, none, nullptr);
      for (int c = 0; c < total; ++c) admitted[c] = conv_cfg_ok(a, c) ? 1 : 0;
    }
    return total;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}

extern "C" int vnf_conv_cfg_tile(int cfg, int32_t tile[6]) {
  ConvTile t;
  if (!tile || !conv_cfg_tile(cfg, t)) return fail(VNF_E_INVALID, "vnf_conv_cfg_tile: no such configuration");
  tile[0] = t.family; tile[1] = t.bm; tile[2] = t.bn; tile[3] = t.wm; tile[4] = t.wn; tile[5] = t.stages;
  return VNF_OK;
}

extern "C" int vnf_conv_probe_run(vnf_handle h, int cfg, const void* x, void* const* out, const void* res, void* stream) {
  try {
    ConvProbe* p = handle_cast<ConvProbe>(h);
    if (!p) return fail(VNF_E_INVALID, "not a conv probe handle");
    if (!x || !out || (p->g.has_res && !res)) return fail(VNF_E_INVALID, "vnf_conv_probe_run: bad argument");
    for (int i = 0; i < p->g.nseg; ++i)
      if (!out[i]) return fail(VNF_E_INVALID, "vnf_conv_probe_run: bad argument");
    ConvArgs a = probe_args(*p, x, out, res);
    if (cfg != -1 && (cfg < 0 || cfg >= conv_num_cfgs() || !conv_cfg_ok(a, cfg)))
      return fail(VNF_E_INVALID, "vnf_conv_probe_run: configuration " + std::to_string(cfg) + " is not admitted for this convolution");
    a.cfg = cfg;
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = launch_conv(a, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) return fail(VNF_E_HIP, std::string("vnf_conv_probe_run: ") + hipGetErrorString(err));
    return VNF_OK;
  } catch (const std::exception& ex) {
    return fail(VNF_E_INVALID, std::string("exception: ") + ex.what());
  }
}
