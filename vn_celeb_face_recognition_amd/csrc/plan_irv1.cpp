// InceptionResnetV1 (models/inception_resnet_v1.py), 160 x 160 input: the plan of vnf_encoder_create(VNF_ARCH_IRV1).
#include "plan.h"

namespace vnf {

// BasicConv2d (inception_resnet_v1.py:12-33): conv(no bias) -> BN(eps 1e-3) -> ReLU
static bool basic_piece(WeightMap& wm, const std::string& p, int cin, int cout, int kh, int kw, Piece& out) {
  return fill_piece(wm, out, p + ".conv.weight", cout, cin * kh * kw, Epilogue::batchnorm(p + ".bn", 1e-3f));
}

int build_irv1(Encoder& e, WeightMap& wm) {
  e.in_size = 160;
  const int b_in = e.add_buf(160, 160, 8);
  const int b_1a = e.add_buf(79, 79, 32), b_2a = e.add_buf(77, 77, 32), b_2b = e.add_buf(77, 77, 64);
  const int b_3a = e.add_buf(38, 38, 64), b_3b = e.add_buf(38, 38, 80), b_4a = e.add_buf(36, 36, 192);
  const int x35[3] = {e.add_buf(17, 17, 256), e.add_buf(17, 17, 256), e.add_buf(17, 17, 256)};
  const int t35a = e.add_buf(17, 17, 64), t35b = e.add_buf(17, 17, 32), cat35 = e.add_buf(17, 17, 96);
  const int m6a = e.add_buf(17, 17, 192), m6b = e.add_buf(17, 17, 192);
  const int x17[3] = {e.add_buf(8, 8, 896), e.add_buf(8, 8, 896), e.add_buf(8, 8, 896)};
  const int t17a = e.add_buf(8, 8, 128), t17b = e.add_buf(8, 8, 128), cat17 = e.add_buf(8, 8, 256);
  const int m7a = e.add_buf(8, 8, 768), m7b = e.add_buf(8, 8, 256);
  const int x8[3] = {e.add_buf(3, 3, 1792), e.add_buf(3, 3, 1792), e.add_buf(3, 3, 1792)};
  const int t8a = e.add_buf(3, 3, 192), t8b = e.add_buf(3, 3, 192), cat8 = e.add_buf(3, 3, 384);
  const int pool = e.add_buf(1, 1, 1792);

  e.ops.push_back(Op::pack(b_in));

  auto simple = [&](const std::string& name, int xb, int xoff, int cin, int cin_pad, int cout, int kh, int kw, int st,
                    int ph, int pw, int ob, int ooff) -> int {
    ConvSpec s;
    s.name = name; s.x_buf = xb; s.x_coff = xoff; s.cin = cin; s.cin_pad = cin_pad;
    s.KH = kh; s.KW = kw; s.sh = s.sw = st; s.ph = ph; s.pw = pw;
    NEED(single_piece(wm, s, name + ".conv.weight", cout, ob, ooff, Epilogue::batchnorm(name + ".bn", 1e-3f)));
    return add_conv(e, s);
  };
  // fused 1x1 reducers of several branches reading the same input: one GEMM, columns routed
  auto fused1x1 = [&](const std::string& name, std::vector<std::string> prefixes, int xb, int cin, int cout_each,
                      std::vector<SegSpec> segs) -> int {
    ConvSpec s;
    s.name = name; s.x_buf = xb; s.cin = s.cin_pad = cin;
    s.pieces.resize(prefixes.size());
    for (size_t i = 0; i < prefixes.size(); ++i)
      NEED(basic_piece(wm, prefixes[i], cin, cout_each, 1, 1, s.pieces[i]));
    s.segs = segs;
    return add_conv(e, s);
  };
  // block-output 1x1 conv with bias, scaled residual and optional ReLU
  // (inception_resnet_v1.py:63-67): relu(conv(cat)*scale + x) == relu(conv_{w*scale} + b*scale + x)
  auto up = [&](const std::string& p, int cat, int cin, int cout, float scale, int xin, int xout, bool relu) -> int {
    ConvSpec s;
    s.name = p + ".conv2d"; s.x_buf = cat; s.cin = s.cin_pad = cin;
    NEED(single_piece(wm, s, p + ".conv2d.weight", cout, xout, 0, Epilogue::biased(p + ".conv2d.bias")));
    Piece& pc = s.pieces[0];
    pc.scale.assign(cout, scale);
    for (int i = 0; i < cout; ++i) pc.bias[i] = pc.bias[i] * scale;
    s.res_buf = xin;
    s.act = relu ? ACT_RELU : ACT_NONE;
    return add_conv(e, s);
  };

  // ---- stem (inception_resnet_v1.py:281-287)
  TRY(simple("conv2d_1a", b_in, 0, 3, 8, 32, 3, 3, 2, 0, 0, b_1a, 0));
  {
    // the first convolution runs as a direct kernel on the caller's NCHW tensor (aux_kernels.hip): the layer stays
    // in `convs` for the FLOP accounting, the PACK + CONV pair of ops becomes one STEM1 op
    const int direct = e.env.direct_stem;
    Piece pc;
    if (direct && basic_piece(wm, "conv2d_1a", 3, 32, 3, 3, pc)) {
      std::vector<float> wt(27 * 32 + 32);
      for (int co = 0; co < 32; ++co) {
        for (int k = 0; k < 27; ++k) wt[k * 32 + co] = pc.w[co * 27 + k] * pc.scale[co];
        wt[27 * 32 + co] = pc.bias[co];
      }
      e.stem_wt = (float*)e.upload(wt.data(), wt.size() * 4);
      if (!e.stem_wt) return VNF_E_HIP;
      e.ops.resize(e.ops.size() - 2);
      e.ops.push_back(Op::stem1((int)e.convs.size() - 1, b_1a));
    }
  }
  {
    FusedStack f;   // 16-bit compute dtypes: conv2d_2a + conv2d_2b + maxpool_3a as one rolling-row launch (stem_mid.hip)
    f.kind = FusedStack::Kind::StemMid;
    f.first = (int)e.ops.size(); f.conv0 = (int)e.convs.size();
    f.in_buf = b_1a; f.out_buf = b_3a; f.nblocks = 1;
    TRY(simple("conv2d_2a", b_1a, 0, 32, 32, 32, 3, 3, 1, 0, 0, b_2a, 0));
    TRY(simple("conv2d_2b", b_2a, 0, 32, 32, 64, 3, 3, 1, 1, 1, b_2b, 0));
    e.ops.push_back(Op::maxpool(b_2b, b_3a, 0));
    f.last = (int)e.ops.size();
    TRY(simple("conv2d_3b", b_3a, 0, 64, 64, 80, 1, 1, 1, 0, 0, b_3b, 0));
    f.ext_last = (int)e.ops.size(); f.ext_conv = (int)e.convs.size() - 1; f.ext_out_buf = b_3b;
    e.fused.push_back(f);
  }
  TRY(simple("conv2d_4a", b_3b, 0, 80, 80, 192, 3, 3, 1, 0, 0, b_4a, 0));
  TRY(simple("conv2d_4b", b_4a, 0, 192, 192, 256, 3, 3, 2, 0, 0, x35[0], 0));
  const int stem_end = (int)e.ops.size();
  e.taps["conv2d_1a"] = {b_1a, 0, 32}; e.taps["conv2d_2a"] = {b_2a, 0, 32}; e.taps["conv2d_2b"] = {b_2b, 0, 64};
  e.taps["maxpool_3a"] = {b_3a, 0, 64}; e.taps["conv2d_3b"] = {b_3b, 0, 80}; e.taps["conv2d_4a"] = {b_4a, 0, 192};
  e.taps["conv2d_4b"] = {x35[0], 0, 256};

  // ---- repeat_1: 5 x Block35 (36-67)
  int cur = 0;
  const int r1_first_op = (int)e.ops.size(), r1_first_conv = (int)e.convs.size();
  for (int i = 0; i < 5; ++i) {
    const std::string p = "repeat_1." + std::to_string(i);
    const int X = x35[cur], Y = x35[cur == 1 ? 2 : 1];
    TRY(fused1x1(p + ".reduce", {p + ".branch0", p + ".branch1.0", p + ".branch2.0"}, X, 256, 32,
                 {{0, 32, cat35, 0}, {32, 96, t35a, 0}}));
    TRY(simple(p + ".branch1.1", t35a, 0, 32, 32, 32, 3, 3, 1, 1, 1, cat35, 32));
    TRY(simple(p + ".branch2.1", t35a, 32, 32, 32, 32, 3, 3, 1, 1, 1, t35b, 0));
    TRY(simple(p + ".branch2.2", t35b, 0, 32, 32, 32, 3, 3, 1, 1, 1, cat35, 64));
    TRY(up(p, cat35, 96, 256, 0.17f, X, Y, true));
    cur = (cur == 1 ? 2 : 1);
  }
  e.taps["repeat_1"] = {x35[cur], 0, 256};
  {
    FusedStack f;   // 16-bit compute dtypes: one fused launch per block (block35.hip) or for the whole stack (trunk35.hip)
    f.kind = FusedStack::Kind::Block35;
    f.first = r1_first_op; f.last = (int)e.ops.size();
    f.nblocks = 5; f.conv0 = r1_first_conv;
    // mixed_6a.branch1.0 (137) reads the stack's output only: listed right behind it so the stack kernel can take it over
    TRY(simple("mixed_6a.branch1.0", x35[cur], 0, 256, 256, 192, 1, 1, 1, 0, 0, m6a, 0));
    f.ext_last = (int)e.ops.size(); f.ext_conv = (int)e.convs.size() - 1; f.ext_out_buf = m6a;
    e.fused.push_back(f);
  }
  // ---- mixed_6a (129-149)
  {
    const int X = x35[cur], O = x17[0];
    // bf16 / f16: the three branch-1 convolutions as one image-resident launch (mixed6a.hip), unless the Block35 stack
    // kernel has taken branch1.0.  They are listed in one run; branch0 and the pool write other channels of O
    FusedStack f;
    f.kind = FusedStack::Kind::Mixed6a;
    f.label = "mixed_6a.branch1.0-1.2 chain";
    f.first = (int)e.ops.size() - 1; f.conv0 = (int)e.convs.size() - 1;
    f.in_buf = X; f.out_buf = O; f.nblocks = 1;
    TRY(simple("mixed_6a.branch1.1", m6a, 0, 192, 192, 192, 3, 3, 1, 1, 1, m6b, 0));
    TRY(simple("mixed_6a.branch1.2", m6b, 0, 192, 192, 256, 3, 3, 2, 0, 0, O, 384));
    f.last = (int)e.ops.size();
    e.fused.push_back(f);
    TRY(simple("mixed_6a.branch0", X, 0, 256, 256, 384, 3, 3, 2, 0, 0, O, 0));
    e.ops.push_back(Op::maxpool(X, O, 640));
  }
  e.taps["mixed_6a"] = {x17[0], 0, 896};
  // ---- repeat_2: 10 x Block17 (70-95)
  cur = 0;
  const int r2_first_op = (int)e.ops.size(), r2_first_conv = (int)e.convs.size();
  for (int i = 0; i < 10; ++i) {
    const std::string p = "repeat_2." + std::to_string(i);
    const int X = x17[cur], Y = x17[cur == 1 ? 2 : 1];
    TRY(fused1x1(p + ".reduce", {p + ".branch0", p + ".branch1.0"}, X, 896, 128,
                 {{0, 128, cat17, 0}, {128, 256, t17a, 0}}));
    TRY(simple(p + ".branch1.1", t17a, 0, 128, 128, 128, 1, 7, 1, 0, 3, t17b, 0));
    TRY(simple(p + ".branch1.2", t17b, 0, 128, 128, 128, 7, 1, 1, 3, 0, cat17, 128));
    TRY(up(p, cat17, 256, 896, 0.10f, X, Y, true));
    cur = (cur == 1 ? 2 : 1);
  }
  e.taps["repeat_2"] = {x17[cur], 0, 896};
  {
    // 16-bit compute dtypes run the whole stack as one persistent kernel (trunk17.hip); the plan ops above stay as
    // the fp32 / split-f16 path, the FLOP accounting and the source of the packed weights
    FusedStack f;
    f.kind = FusedStack::Kind::Block17;
    f.first = r2_first_op; f.last = (int)e.ops.size();
    f.in_buf = x17[0]; f.out_buf = x17[cur];
    f.nblocks = 10; f.conv0 = r2_first_conv;
    e.fused.push_back(f);
  }
  // ---- mixed_7a (152-181)
  {
    const int X = x17[cur], O = x8[0];
    TRY(fused1x1("mixed_7a.reduce", {"mixed_7a.branch0.0", "mixed_7a.branch1.0", "mixed_7a.branch2.0"}, X, 896, 256,
                 {{0, 768, m7a, 0}}));
    TRY(simple("mixed_7a.branch0.1", m7a, 0, 256, 256, 384, 3, 3, 2, 0, 0, O, 0));
    TRY(simple("mixed_7a.branch1.1", m7a, 256, 256, 256, 256, 3, 3, 2, 0, 0, O, 384));
    TRY(simple("mixed_7a.branch2.1", m7a, 512, 256, 256, 256, 3, 3, 1, 1, 1, m7b, 0));
    TRY(simple("mixed_7a.branch2.2", m7b, 0, 256, 256, 256, 3, 3, 2, 0, 0, O, 640));
    e.ops.push_back(Op::maxpool(X, O, 896));
  }
  e.taps["mixed_7a"] = {x8[0], 0, 1792};
  // ---- repeat_3 (5 x Block8, scale 0.2) + block8 (scale 1, no ReLU) (98-126, 247-254)
  cur = 0;
  for (int i = 0; i < 6; ++i) {
    const std::string p = i < 5 ? "repeat_3." + std::to_string(i) : std::string("block8");
    const int X = x8[cur], Y = x8[cur == 1 ? 2 : 1];
    FusedStack f;   // bf16 / f16: reduce + 1x3 + 3x1 as one weight-streaming launch (block8.hip); the up-projection stays
    f.kind = FusedStack::Kind::Block8;
    f.label = p + " chain (reduce+1x3+3x1)";
    f.first = (int)e.ops.size(); f.conv0 = (int)e.convs.size();
    f.in_buf = X; f.out_buf = cat8; f.nblocks = 1;
    TRY(fused1x1(p + ".reduce", {p + ".branch0", p + ".branch1.0"}, X, 1792, 192,
                 {{0, 192, cat8, 0}, {192, 384, t8a, 0}}));
    TRY(simple(p + ".branch1.1", t8a, 0, 192, 192, 192, 1, 3, 1, 0, 1, t8b, 0));
    TRY(simple(p + ".branch1.2", t8b, 0, 192, 192, 192, 3, 1, 1, 1, 0, cat8, 192));
    f.last = (int)e.ops.size();
    e.fused.push_back(f);
    TRY(up(p, cat8, 384, 1792, i < 5 ? 0.20f : 1.0f, X, Y, i < 5));
    cur = (cur == 1 ? 2 : 1);
    if (i == 4) e.taps["repeat_3"] = {x8[cur], 0, 1792};
  }
  e.taps["block8"] = {x8[cur], 0, 1792};
  // ---- tail (294-302): avgpool -> last_linear (no bias) -> last_bn (eps 1e-3) -> L2 normalise
  e.ops.push_back(Op::avgpool(x8[cur], pool));
  e.taps["avgpool_1a"] = {pool, 0, 1792};
  {
    ConvSpec s;
    s.name = "last_linear"; s.x_buf = pool; s.cin = s.cin_pad = 1792;
    NEED(single_piece(wm, s, "last_linear.weight", 512, -2, 0, Epilogue::batchnorm("last_bn", 1e-3f)));
    s.act = ACT_NONE; s.out_f32 = 1;
    TRY(add_conv(e, s));
  }
  e.ops.push_back(Op::l2norm());

  // unfused, the stem runs in sub-batches of 128 images so its big producer -> consumer tensors stay inside the
  // Infinity Cache; with conv2d_2a/2b/maxpool fused (one workgroup per image, no big intermediate) a sub-batch would
  // only leave half the CUs without a workgroup
  const int fuse_mask = e.env.fuse;
  int chunk = ((fuse_mask & 4) && (e.dtype == BF16 || e.dtype == F16 || (e.dtype == F16P && (fuse_mask & 8)))) ? 256 : 128;
  if (e.env.stem_chunk > 0) chunk = e.env.stem_chunk;
  e.groups.push_back({0, stem_end, chunk});
  e.groups.push_back({stem_end, (int)e.ops.size(), 1 << 30});
  return VNF_OK;
}

}  // namespace vnf
