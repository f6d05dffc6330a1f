// IResNet-100 (models/iresnet_encoder.py), 112 x 112 input: the plan of vnf_encoder_create(VNF_ARCH_IR100).
#include "plan.h"

namespace vnf {

// IResNet-100 (models/iresnet_encoder.py:26-61, 64-159).  Per IBasicBlock two launches:
//   A: conv1(bn1(x)) -> bn2 -> PReLU.  bn1 sits BEFORE a zero-padded conv, so it cannot be folded
//      into a plain bias: its scale goes into the weights, and its shift becomes a bias that depends
//      on which taps fall inside the image -- one of 9 border classes, picked in the epilogue.
//      bn2 folds into per-output scale / bias, PReLU runs in the epilogue.
//   B: conv2 (stride) -> bn3, + identity (x, or the 1x1-stride-2 downsample branch with its BN).
// The head (bn2 -> flatten (C,H,W) -> fc -> features BN1d) is ONE 7x7 "convolution" over the
// NHWC map: fc.weight viewed as (512, 512, 7, 7) is exactly that conv's weight.
int build_ir100(Encoder& e, WeightMap& wm) {
  e.in_size = 112;
  const float EPS = 2e-5f;
  const int b_in = e.add_buf(112, 112, 8);
  e.ops.push_back(Op::pack(b_in));
  const int planes[4] = {64, 128, 256, 512}, nblk[4] = {3, 13, 30, 3};
  int H = 112;
  int x = e.add_buf(112, 112, 64);
  {  // stem: conv1 3x3 p1 (3->64) -> bn1 -> PReLU (iresnet_encoder.py:140-142)
    ConvSpec s;
    s.name = "conv1"; s.x_buf = b_in; s.cin = 3; s.cin_pad = 8; s.KH = s.KW = 3; s.ph = s.pw = 1;
    NEED(single_piece(wm, s, "conv1.weight", 64, x, 0, Epilogue::batchnorm("bn1", EPS, "prelu.weight")));
    s.act = ACT_PRELU;
    TRY(add_conv(e, s));
  }
  e.taps["stem"] = {x, 0, 64};
  int cin = 64;
  std::vector<int> stage_end;
  for (int li = 0; li < 4; ++li) {
    const int P = planes[li], Ho = H / 2;
    const int t_first = e.add_buf(H, H, P);      // conv1 output of the first block (input resolution)
    const int t_rest = e.add_buf(Ho, Ho, P);
    const int dsb = e.add_buf(Ho, Ho, P);        // downsample branch
    const int y[2] = {e.add_buf(Ho, Ho, P), e.add_buf(Ho, Ho, P)};
    int cur = -1;
    for (int b = 0; b < nblk[li]; ++b) {
      const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
      const int xin = b == 0 ? x : y[cur];
      const int xout = b == 0 ? y[0] : y[cur ^ 1];
      const int ci = b == 0 ? cin : P, t1 = b == 0 ? t_first : t_rest, st = b == 0 ? 2 : 1;
      std::vector<float> s1, t1v;
      NEED(bn_fold(wm, p + ".bn1", ci, EPS, s1, t1v));
      {
        ConvSpec s;
        s.name = p + ".conv1"; s.x_buf = xin; s.cin = s.cin_pad = ci; s.KH = s.KW = 3; s.ph = s.pw = 1;
        NEED(single_piece(wm, s, p + ".conv1.weight", P, t1, 0, Epilogue::batchnorm(p + ".bn2", EPS, p + ".prelu.weight")));
        s.pre_s = &s1; s.pre_t = &t1v;
        s.act = ACT_PRELU;
        TRY(add_conv(e, s));
      }
      if (b == 0) {
        ConvSpec s;
        s.name = p + ".downsample"; s.x_buf = xin; s.cin = s.cin_pad = ci; s.sh = s.sw = 2;
        NEED(single_piece(wm, s, p + ".downsample.0.weight", P, dsb, 0, Epilogue::batchnorm(p + ".downsample.1", EPS)));
        s.act = ACT_NONE;
        TRY(add_conv(e, s));
      }
      {
        ConvSpec s;
        s.name = p + ".conv2"; s.x_buf = t1; s.cin = s.cin_pad = P; s.KH = s.KW = 3; s.ph = s.pw = 1; s.sh = s.sw = st;
        NEED(single_piece(wm, s, p + ".conv2.weight", P, xout, 0, Epilogue::batchnorm(p + ".bn3", EPS)));
        s.res_buf = b == 0 ? dsb : xin;
        s.act = ACT_NONE;
        TRY(add_conv(e, s));
      }
      cur = b == 0 ? 0 : cur ^ 1;
    }
    x = y[cur];
    e.taps["layer" + std::to_string(li + 1)] = {x, 0, P};
    cin = P;
    H = Ho;
    stage_end.push_back((int)e.ops.size());
  }
  {  // bn2 -> flatten -> fc(+bias) -> features (iresnet_encoder.py:149-153)
    std::vector<float> s2, t2, sf, tf;
    NEED(bn_fold(wm, "bn2", 512, EPS, s2, t2) && bn_fold(wm, "features", 512, EPS, sf, tf));
    ConvSpec s;
    s.name = "fc"; s.x_buf = x; s.cin = s.cin_pad = 512; s.KH = s.KW = 7;
    NEED(single_piece(wm, s, "fc.weight", 512, -2, 0, Epilogue::biased("fc.bias")));
    Piece& pc = s.pieces[0];
    pc.scale = sf;
    for (int i = 0; i < 512; ++i) pc.bias[i] = pc.bias[i] * sf[i] + tf[i];
    s.pre_s = &s2; s.pre_t = &t2;
    s.act = ACT_NONE; s.out_f32 = 1;
    TRY(add_conv(e, s));
  }
  e.ops.push_back(Op::copyout());
  add_resnet_groups(e, stage_end[0], stage_end[1]);
  return VNF_OK;
}

}  // namespace vnf
