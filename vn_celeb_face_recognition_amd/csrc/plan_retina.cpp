#include "plan.h"

namespace vnf {

// RetinaFace with the MobileNetV1-0.25 backbone (models/retina_face.py:56-152, retina_face_utils/components.py,
// config.py cfg_mnet) as a plan on the exact-f32 core.  LeakyReLU is the PReLU epilogue with a constant slope;
// relu(cat(...)) of SSH is a ReLU in each branch's last conv, written into its channel slice (concat-free).
int build_retina_mnet(Encoder& e, WeightMap& wm, int H, int W, int head_bufs[3]) {
  e.in_size = 0;
  const float EPS = 1e-5f;   // every BatchNorm of the network
  auto down = [](int v) { return (v + 2 - 3) / 2 + 1; };
  // VNF_RETINA_FUSE=0: the early layers as plan convolutions on an NHWC4 fp32 copy of the frames (buffer 0, written by
  // the caller); default: conv0 straight from the u8 frames (Op::RSTEM) and dw+pw blocks in one kernel (Op::DWPW)
  // (bit 0: stem, bit 1: dw+pw blocks)
  const int fuse_env = e.env.retina_fuse;
  const bool fused = fuse_env & 1, fused_dw = fuse_env & 2;
  int cur = e.add_buf(fused ? 1 : H, fused ? 1 : W, 4);   // input: NHWC4 (R-104, G-117, B-123, 0); a stub when fused
  int h = H, w = W;
  // conv (3x3 or 1x1) + BN + optional LeakyReLU / ReLU into (buf, channel offset)
  auto conv_bn = [&](const std::string& p, int xb, int cin, int cin_pad, int cout, int k, int stride, int ob, int ooff, int act,
                     float leaky) -> int {
    ConvSpec s;
    s.name = p; s.x_buf = xb; s.cin = cin; s.cin_pad = cin_pad; s.KH = s.KW = k; s.sh = s.sw = stride; s.ph = s.pw = k / 2;
    if (!single_piece(wm, s, p + ".0.weight", cout, ob, ooff, Epilogue::batchnorm(p + ".1", EPS)))
      return fail(VNF_E_MISSING, "retina: missing weight " + wm.missing);
    if (act == ACT_PRELU) s.pieces[0].slope.assign(cout, leaky);
    s.act = act;
    return add_conv(e, s);
  };
  // conv_dw(inp, oup, stride): depthwise 3x3 + BN + leaky 0.1, pointwise 1x1 + BN + leaky 0.1 (components.py:30-40)
  auto conv_dw = [&](const std::string& p, int inp, int oup, int stride) -> int {
    const float* dw = wm.get(p + ".0.weight", (int64_t)inp * 9);
    std::vector<float> sc, sh;
    if (!dw || !bn_fold(wm, p + ".1", inp, EPS, sc, sh)) return fail(VNF_E_MISSING, "retina: missing weight " + wm.missing);
    std::vector<float> w9c((size_t)9 * inp);
    for (int c = 0; c < inp; ++c)
      for (int t = 0; t < 9; ++t) w9c[(size_t)t * inp + c] = dw[(size_t)c * 9 + t] * sc[c];
    const int ho = stride == 2 ? down(h) : h, wo = stride == 2 ? down(w) : w;
    if (fused_dw && dwpw_supported(inp, oup)) {
      const float* pw = wm.get(p + ".3.weight", (int64_t)oup * inp);
      std::vector<float> ps, pb;
      if (!pw || !bn_fold(wm, p + ".4", oup, EPS, ps, pb)) return fail(VNF_E_MISSING, "retina: missing weight " + wm.missing);
      std::vector<float> pwf((size_t)oup * inp);
      for (int o = 0; o < oup; ++o)
        for (int c = 0; c < inp; ++c) pwf[(size_t)o * inp + c] = pw[(size_t)o * inp + c] * ps[o];
      DwPwLayer d;
      d.name = p; d.x_buf = cur; d.o_buf = e.add_buf(ho, wo, oup); d.cin = inp; d.cout = oup; d.stride = stride; d.slope = 0.1f;
      d.dw = (float*)e.upload(w9c.data(), w9c.size() * 4);
      d.dbias = (float*)e.upload(sh.data(), sh.size() * 4);
      d.pw = (float*)e.upload(pwf.data(), pwf.size() * 4);
      d.pbias = (float*)e.upload(pb.data(), pb.size() * 4);
      if (!d.dw || !d.dbias || !d.pw || !d.pbias) return VNF_E_HIP;
      e.dwpws.push_back(d);
      e.ops.push_back(Op::dwpw((int)e.dwpws.size() - 1));
      cur = d.o_buf; h = ho; w = wo;
      return VNF_OK;
    }
    DwLayer d;
    d.x_buf = cur; d.o_buf = e.add_buf(ho, wo, inp); d.C = inp; d.stride = stride; d.slope = 0.1f;
    d.w = (float*)e.upload(w9c.data(), w9c.size() * 4);
    d.bias = (float*)e.upload(sh.data(), sh.size() * 4);
    if (!d.w || !d.bias) return VNF_E_HIP;
    e.dws.push_back(d);
    e.ops.push_back(Op::dwconv((int)e.dws.size() - 1));
    h = ho; w = wo;
    const int ob = e.add_buf(h, w, oup);
    // the pointwise half: Sequential indices 3 (conv) and 4 (bn)
    ConvSpec s;
    s.name = p + ".3"; s.x_buf = d.o_buf; s.cin = s.cin_pad = inp;
    if (!single_piece(wm, s, p + ".3.weight", oup, ob, 0, Epilogue::batchnorm(p + ".4", EPS)))
      return fail(VNF_E_MISSING, "retina: missing weight " + wm.missing);
    s.pieces[0].slope.assign(oup, 0.1f);
    s.act = ACT_PRELU;
    TRY(add_conv(e, s));
    cur = ob;
    return VNF_OK;
  };
  // ---- body (components.py:100-121)
  {
    const int ho = down(h), wo = down(w);
    const int ob = e.add_buf(ho, wo, 8);
    if (fused) {
      const float* w0 = wm.get("body.stage1.0.0.weight", 8 * 27);
      std::vector<float> sc, sh;
      if (!w0 || !bn_fold(wm, "body.stage1.0.1", 8, EPS, sc, sh)) return fail(VNF_E_MISSING, "retina: missing weight " + wm.missing);
      std::vector<float> wa(7 * 64, 0.f);
      for (int s7 = 0; s7 < 7; ++s7)
        for (int lane = 0; lane < 64; ++lane) {
          const int lg = lane >> 4, lm = lane & 15, k = 4 * s7 + lg;
          if (lm < 8 && k < 27) {
            const int tap = k / 3, c = k % 3;
            wa[s7 * 64 + lane] = w0[(lm * 3 + c) * 9 + tap] * sc[lm];
          }
        }
      e.rstem_wa = (float*)e.upload(wa.data(), wa.size() * 4);
      e.rstem_bias = (float*)e.upload(sh.data(), 8 * 4);
      if (!e.rstem_wa || !e.rstem_bias) return VNF_E_HIP;
      e.ops.push_back(Op::rstem(H, W, ob));
    } else {
      TRY(conv_bn("body.stage1.0", cur, 3, 4, 8, 3, 2, ob, 0, ACT_PRELU, 0.1f));
    }
    cur = ob; h = ho; w = wo;
  }
  TRY(conv_dw("body.stage1.1", 8, 16, 1));
  TRY(conv_dw("body.stage1.2", 16, 32, 2));
  TRY(conv_dw("body.stage1.3", 32, 32, 1));
  TRY(conv_dw("body.stage1.4", 32, 64, 2));
  TRY(conv_dw("body.stage1.5", 64, 64, 1));
  const int c1 = cur, h1 = h, w1 = w;
  TRY(conv_dw("body.stage2.0", 64, 128, 2));
  for (int i = 1; i < 6; ++i) TRY(conv_dw("body.stage2." + std::to_string(i), 128, 128, 1));
  const int c2 = cur, h2 = h, w2 = w;
  TRY(conv_dw("body.stage3.0", 128, 256, 2));
  TRY(conv_dw("body.stage3.1", 256, 256, 1));
  const int c3 = cur, h3 = h, w3 = w;
  // ---- FPN (components.py:66-97; out_channels 64 -> leaky 0.1)
  const int o1 = e.add_buf(h1, w1, 64), o2 = e.add_buf(h2, w2, 64), o3 = e.add_buf(h3, w3, 64);
  TRY(conv_bn("fpn.output1", c1, 64, 64, 64, 1, 1, o1, 0, ACT_PRELU, 0.1f));
  TRY(conv_bn("fpn.output2", c2, 128, 128, 64, 1, 1, o2, 0, ACT_PRELU, 0.1f));
  TRY(conv_bn("fpn.output3", c3, 256, 256, 64, 1, 1, o3, 0, ACT_PRELU, 0.1f));
  e.ops.push_back(Op::upadd(o3, o2));
  const int m2 = e.add_buf(h2, w2, 64);
  TRY(conv_bn("fpn.merge2", o2, 64, 64, 64, 3, 1, m2, 0, ACT_PRELU, 0.1f));
  e.ops.push_back(Op::upadd(m2, o1));
  const int m1 = e.add_buf(h1, w1, 64);
  TRY(conv_bn("fpn.merge1", o1, 64, 64, 64, 3, 1, m1, 0, ACT_PRELU, 0.1f));
  // ---- SSH x3 + heads (components.py:42-64, retina_face.py:20-54,138-146)
  const int feat_in[3] = {m1, m2, o3}, fh[3] = {h1, h2, h3}, fw[3] = {w1, w2, w3};
  for (int l = 0; l < 3; ++l) {
    const std::string p = "ssh" + std::to_string(l + 1);
    const int cat = e.add_buf(fh[l], fw[l], 64), t5 = e.add_buf(fh[l], fw[l], 16), t7 = e.add_buf(fh[l], fw[l], 16);
    // convolutions that read the same tensor run as ONE GEMM whose column ranges go to different tensors (ReLU = a
    // PReLU slope of 0, LeakyReLU = 0.1 on the other range): conv3X3 | conv5X5_1 on the level's feature map,
    // conv5X5_2 | conv7X7_2 on conv5X5_1's output
    auto conv_pair = [&](const std::string& pa, int na, int ba, int oa, float sa, const std::string& pb, int nb, int bb, int ob2,
                         float sb, int xb, int cin) -> int {
      ConvSpec s;
      s.name = pa + "|" + pb.substr(pb.rfind('.') + 1); s.x_buf = xb; s.cin = s.cin_pad = cin; s.KH = s.KW = 3; s.ph = s.pw = 1;
      s.pieces.resize(2);
      const std::string nm[2] = {pa, pb};
      const int nn[2] = {na, nb};
      const float sl[2] = {sa, sb};
      for (int k = 0; k < 2; ++k) {
        if (!fill_piece(wm, s.pieces[k], nm[k] + ".0.weight", nn[k], cin * 9, Epilogue::batchnorm(nm[k] + ".1", EPS)))
          return fail(VNF_E_MISSING, "retina: missing weight " + wm.missing);
        s.pieces[k].slope.assign(nn[k], sl[k]);
      }
      s.segs.push_back({0, na, ba, oa});
      s.segs.push_back({na, na + nb, bb, ob2});
      s.act = ACT_PRELU;
      return add_conv(e, s);
    };
    TRY(conv_pair(p + ".conv3X3", 32, cat, 0, 0.f, p + ".conv5X5_1", 16, t5, 0, 0.1f, feat_in[l], 64));
    TRY(conv_pair(p + ".conv5X5_2", 16, cat, 32, 0.f, p + ".conv7X7_2", 16, t7, 0, 0.1f, t5, 16));
    TRY(conv_bn(p + ".conv7x7_3", t7, 16, 16, 16, 3, 1, cat, 48, ACT_RELU, 0.f));
    // the three 1x1 heads of the level as one GEMM: columns [class 4 | bbox 8 | landmark 20]
    const int hb = e.add_buf(fh[l], fw[l], 32);
    ConvSpec s;
    s.name = "heads" + std::to_string(l); s.x_buf = cat; s.cin = s.cin_pad = 64;
    s.pieces.resize(3);
    const char* hn[3] = {"ClassHead.", "BboxHead.", "LandmarkHead."};
    const int hc[3] = {4, 8, 20};
    for (int k = 0; k < 3; ++k) {
      const std::string q = std::string(hn[k]) + std::to_string(l) + ".conv1x1";
      if (!fill_piece(wm, s.pieces[k], q + ".weight", hc[k], 64, Epilogue::biased(q + ".bias")))
        return fail(VNF_E_MISSING, "retina: missing weight " + wm.missing);
    }
    s.segs.push_back({0, 32, hb, 0});
    s.act = ACT_NONE;
    TRY(add_conv(e, s));
    head_bufs[l] = hb;
  }
  return VNF_OK;
}

}  // namespace vnf
