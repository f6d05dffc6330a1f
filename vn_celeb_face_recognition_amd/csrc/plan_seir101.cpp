// SE-IR ResNet-101 (models/resnet_encoder.py), 112 x 112 input: the plan of vnf_encoder_create(VNF_ARCH_SEIR101).
#include "plan.h"

namespace vnf {

// ResNet(IRBlock, [3, 4, 23, 3], use_se=True) (resnet_encoder.py:116-222).  Per IRBlock three launches (+ the downsample):
//   A: conv1(bn0(x)) -> bn1 -> PReLU.  bn0 sits before a zero-padded conv: scale into the weights, shift as one of 9
//      border-class biases (as IR-100's bn1).  conv1 keeps the INPUT width and resolution.
//   B: conv2 (stride) -> bn2, no activation and no residual: the SE gate multiplies before the add.
//   SE: gate from the spatial mean of B's output, then prelu(B * gate + residual) with the block's one PReLU again
//      (se_block.hip; the residual is x, or the 1x1 stride-2 downsample branch with its BN).
// Every nn.PReLU() here has ONE slope: it is broadcast over the channels of the convolution epilogue.
// The head (bn2 -> flatten (C,H,W) -> fc -> bn3) is one 7x7 "convolution" as in IR-100, then the L2 normalisation.
int build_seir101(Encoder& e, WeightMap& wm) {
  e.in_size = 112;
  const float EPS = 1e-5f;
  const int b_in = e.add_buf(112, 112, 8);
  e.ops.push_back(Op::pack(b_in));
  const int planes[4] = {64, 128, 256, 512}, nblk[4] = {3, 4, 23, 3};
  auto slope1 = [&](const std::string& name, float& out) {   // the single slope of an nn.PReLU()
    const float* a = wm.get(name, 1);
    if (a) out = a[0];
    return a != nullptr;
  };
  const int c1 = e.add_buf(110, 110, 64);
  int x = e.add_buf(55, 55, 64);
  {  // stem: conv1 3x3 no padding (3->64) -> bn1 -> PReLU -> MaxPool2d(2, 2) (resnet_encoder.py:205-208)
    ConvSpec s;
    s.name = "conv1"; s.x_buf = b_in; s.cin = 3; s.cin_pad = 8; s.KH = s.KW = 3;
    NEED(single_piece(wm, s, "conv1.weight", 64, c1, 0, Epilogue::batchnorm("bn1", EPS)));
    float a = 0.f;
    NEED(slope1("prelu.weight", a));
    s.pieces[0].slope.assign(64, a);
    s.act = ACT_PRELU;
    TRY(add_conv(e, s));
    e.ops.push_back(Op::maxpool(c1, x, 0, {2, 0, false}));
  }
  e.taps["conv1"] = {c1, 0, 64};
  e.taps["stem"] = {x, 0, 64};
  int cin = 64, H = 55;
  std::vector<int> stage_end;
  for (int li = 0; li < 4; ++li) {
    const int P = planes[li], Ho = li == 0 ? H : (H + 1) / 2;
    const int t_first = e.add_buf(H, H, cin);     // conv1 output of the first block: input width and resolution
    const int t_rest = e.add_buf(Ho, Ho, P);
    const int t2 = e.add_buf(Ho, Ho, P);          // conv2 + bn2, what the SE kernels read
    const int dsb = li == 0 ? -1 : e.add_buf(Ho, Ho, P);   // downsample branch
    const int y[2] = {e.add_buf(Ho, Ho, P), e.add_buf(Ho, Ho, P)};
    const int slices = se_slices(e.dtype, Ho * Ho, P);
    if (slices < 1) return fail(VNF_E_INVALID, "se: unsupported shape");
    const int part = e.add_buf(1, 1, slices * P * 4 / dtype_size(e.dtype));   // fp32 slice sums of the squeeze launch
    int cur = -1;
    for (int b = 0; b < nblk[li]; ++b) {
      const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
      const int xin = b == 0 ? x : y[cur];
      const int xout = b == 0 ? y[0] : y[cur ^ 1];
      const int ci = b == 0 ? cin : P, t1 = b == 0 ? t_first : t_rest, st = (b == 0 && li > 0) ? 2 : 1;
      const bool down = b == 0 && li > 0;
      float a = 0.f;
      NEED(slope1(p + ".prelu.weight", a));
      std::vector<float> s0, t0;
      NEED(bn_fold(wm, p + ".bn0", ci, EPS, s0, t0));
      {
        ConvSpec s;
        s.name = p + ".conv1"; s.x_buf = xin; s.cin = s.cin_pad = ci; s.KH = s.KW = 3; s.ph = s.pw = 1;
        NEED(single_piece(wm, s, p + ".conv1.weight", ci, t1, 0, Epilogue::batchnorm(p + ".bn1", EPS)));
        s.pieces[0].slope.assign(ci, a);
        s.pre_s = &s0; s.pre_t = &t0;
        s.act = ACT_PRELU;
        TRY(add_conv(e, s));
      }
      if (down) {
        ConvSpec s;
        s.name = p + ".downsample"; s.x_buf = xin; s.cin = s.cin_pad = ci; s.sh = s.sw = 2;
        NEED(single_piece(wm, s, p + ".downsample.0.weight", P, dsb, 0, Epilogue::batchnorm(p + ".downsample.1", EPS)));
        s.act = ACT_NONE;
        TRY(add_conv(e, s));
      }
      {
        ConvSpec s;
        s.name = p + ".conv2"; s.x_buf = t1; s.cin = s.cin_pad = ci; s.KH = s.KW = 3; s.ph = s.pw = 1; s.sh = s.sw = st;
        NEED(single_piece(wm, s, p + ".conv2.weight", P, t2, 0, Epilogue::batchnorm(p + ".bn2", EPS)));
        s.act = ACT_NONE;
        TRY(add_conv(e, s));
      }
      {
        const int R = P / 16;
        SeLayer L;
        L.name = p + ".se"; L.C = P; L.part_buf = part;
        const float* w1 = wm.get(p + ".se.fc.0.weight", (int64_t)R * P);
        const float* b1 = wm.get(p + ".se.fc.0.bias", R);
        const float* w2 = wm.get(p + ".se.fc.2.weight", (int64_t)P * R);
        const float* b2 = wm.get(p + ".se.fc.2.bias", P);
        NEED(w1 && b1 && w2 && b2 && slope1(p + ".se.fc.1.weight", L.slope_se));
        L.slope_out = a;
        L.w1 = (float*)e.upload(w1, (size_t)R * P * 4);
        L.b1 = (float*)e.upload(b1, (size_t)R * 4);
        L.w2 = (float*)e.upload(w2, (size_t)P * R * 4);
        L.b2 = (float*)e.upload(b2, (size_t)P * 4);
        if (!L.w1 || !L.b1 || !L.w2 || !L.b2) return VNF_E_HIP;
        e.ses.push_back(L);
        e.ops.push_back(Op::se((int)e.ses.size() - 1, t2, down ? dsb : xin, xout));
      }
      cur = b == 0 ? 0 : cur ^ 1;
    }
    x = y[cur];
    e.taps["layer" + std::to_string(li + 1)] = {x, 0, P};
    cin = P;
    H = Ho;
    stage_end.push_back((int)e.ops.size());
  }
  {  // bn2 -> (dropout: identity) -> flatten -> fc(+bias) -> bn3 (resnet_encoder.py:215-219)
    std::vector<float> s2, t2, s3, t3;
    NEED(bn_fold(wm, "bn2", 512, EPS, s2, t2) && bn_fold(wm, "bn3", 512, EPS, s3, t3));
    ConvSpec s;
    s.name = "fc"; s.x_buf = x; s.cin = s.cin_pad = 512; s.KH = s.KW = 7;
    NEED(single_piece(wm, s, "fc.weight", 512, -2, 0, Epilogue::biased("fc.bias")));
    Piece& pc = s.pieces[0];
    pc.scale = s3;
    for (int i = 0; i < 512; ++i) pc.bias[i] = pc.bias[i] * s3[i] + t3[i];
    s.pre_s = &s2; s.pre_t = &t2;
    s.act = ACT_NONE; s.out_f32 = 1;
    TRY(add_conv(e, s));
  }
  e.taps["bn3"] = {-2, 0, 512};   // emb_raw: the fp32 features before the normalisation
  e.ops.push_back(Op::l2norm());
  add_resnet_groups(e, stage_end[0], stage_end[1]);
  return VNF_OK;
}

}  // namespace vnf
