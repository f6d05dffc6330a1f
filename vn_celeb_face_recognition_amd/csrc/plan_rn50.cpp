#include "plan.h"

namespace vnf {

// ResNet-50 with two linear heads (models/resnet_2_branch.py:12-70; Bottleneck: resnet_2_branch_utils/resnet.py:68-104),
// the emotion network.  Every BatchNorm (eps 1e-5) follows its convolution, so all of them fold into scale and bias;
// per Bottleneck three launches (1x1 -> ReLU, 3x3 carrying the stride -> ReLU, 1x1 + residual -> ReLU) plus the 1x1
// stride-s downsample of the first block of each layer.  The stem is the generic convolution on the NHWC8 input
// (7x7x8 = 392 k values, 147 of them real: the channel padding adds ~5 % to the plan's executed MACs, 8.61 against
// 8.18 GFLOP per image; the stem as a whole is ~7 % of them), the heads are ONE GEMM over the pooled
// 2048 features whose columns [0, pad8(num_classes)) and [pad8(num_classes), ...) land side by side in emb_raw.
int build_rn50_2b(Encoder& e, WeightMap& wm, int num_classes, int num_projections) {
  e.in_size = 224;
  e.n_cls = num_classes; e.n_proj = num_projections;
  const float EPS = 1e-5f;
  const int b_in = e.add_buf(224, 224, 8);
  e.ops.push_back(Op::pack(b_in));
  auto conv_bn = [&](const std::string& name, const std::string& wname, const std::string& bn, int xb, int cin, int cin_pad, int cout,
                     int k, int st, int pad, int ob, int res, int act) -> int {
    ConvSpec s;
    s.name = name; s.x_buf = xb; s.cin = cin; s.cin_pad = cin_pad; s.KH = s.KW = k; s.sh = s.sw = st; s.ph = s.pw = pad;
    NEED(single_piece(wm, s, wname, cout, ob, 0, Epilogue::batchnorm(bn, EPS)));
    s.res_buf = res;
    s.act = act;
    return add_conv(e, s);
  };
  const int b_stem = e.add_buf(112, 112, 64), b_pool = e.add_buf(56, 56, 64);
  TRY(conv_bn("conv1", "conv1.weight", "bn1", b_in, 3, 8, 64, 7, 2, 3, b_stem, -1, ACT_RELU));
  e.ops.push_back(Op::maxpool_pad1(b_stem, b_pool));
  e.taps["stem"] = {b_stem, 0, 64};
  e.taps["maxpool"] = {b_pool, 0, 64};
  const int planes[4] = {64, 128, 256, 512}, nblk[4] = {3, 4, 6, 3};
  int x = b_pool, cin = 64, H = 56;
  std::vector<int> stage_end;
  for (int li = 0; li < 4; ++li) {
    const int P = planes[li], st0 = li == 0 ? 1 : 2, Ho = H / st0;
    const int t_first = e.add_buf(H, H, P);   // conv1 output of the first block (input resolution: the stride sits in conv2)
    const int t_rest = li == 0 ? t_first : e.add_buf(Ho, Ho, P);
    const int t2 = e.add_buf(Ho, Ho, P), dsb = e.add_buf(Ho, Ho, 4 * P);
    const int y[2] = {e.add_buf(Ho, Ho, 4 * P), e.add_buf(Ho, Ho, 4 * P)};
    int cur = -1;
    for (int b = 0; b < nblk[li]; ++b) {
      const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
      const int xin = b == 0 ? x : y[cur], xout = b == 0 ? y[0] : y[cur ^ 1];
      const int ci = b == 0 ? cin : 4 * P, t1 = b == 0 ? t_first : t_rest, st = b == 0 ? st0 : 1;
      TRY(conv_bn(p + ".conv1", p + ".conv1.weight", p + ".bn1", xin, ci, ci, P, 1, 1, 0, t1, -1, ACT_RELU));
      TRY(conv_bn(p + ".conv2", p + ".conv2.weight", p + ".bn2", t1, P, P, P, 3, st, 1, t2, -1, ACT_RELU));
      if (b == 0)
        TRY(conv_bn(p + ".downsample", p + ".downsample.0.weight", p + ".downsample.1", xin, ci, ci, 4 * P, 1, st, 0, dsb, -1, ACT_NONE));
      TRY(conv_bn(p + ".conv3", p + ".conv3.weight", p + ".bn3", t2, P, P, 4 * P, 1, 1, 0, xout, b == 0 ? dsb : xin, ACT_RELU));
      cur = b == 0 ? 0 : cur ^ 1;
    }
    x = y[cur];
    e.taps["layer" + std::to_string(li + 1)] = {x, 0, 4 * P};
    cin = 4 * P;
    H = Ho;
    stage_end.push_back((int)e.ops.size());
  }
  // AvgPool2d(7) on the 7x7 map -> fc (2048 -> num_classes) and proj (2048 -> num_projections), both with bias, fp32 out
  const int pool = e.add_buf(1, 1, 2048);
  e.ops.push_back(Op::avgpool(x, pool));
  e.taps["avgpool"] = {pool, 0, 2048};
  const int cls_pad = (num_classes + 7) / 8 * 8, proj_pad = (num_projections + 7) / 8 * 8;
  e.emb_ld = cls_pad + proj_pad;
  {
    ConvSpec s;
    s.name = "fc+proj"; s.x_buf = pool; s.cin = s.cin_pad = 2048;
    s.pieces.resize(2);
    const char* nm[2] = {"fc", "proj"};
    const int co[2] = {num_classes, num_projections}, cp[2] = {cls_pad, proj_pad};
    for (int i = 0; i < 2; ++i) {
      const std::string p = nm[i];
      NEED(fill_piece(wm, s.pieces[i], p + ".weight", co[i], 2048, Epilogue::biased(p + ".bias"), cp[i]));
    }
    s.segs.push_back({0, e.emb_ld, -2, 0});
    s.act = ACT_NONE; s.out_f32 = 1;
    TRY(add_conv(e, s));
  }
  e.ops.push_back(Op::heads(num_classes, num_projections, cls_pad));
  // the stem, the pool and layer1 work on the same 112x112x64 / 56x56x256 tensor sizes as IR-100's first stage, layer2 on
  // IR-100's second: the same sub-batches (and the same switches) keep producer -> consumer tensors in the Infinity Cache
  add_resnet_groups(e, stage_end[0], stage_end[1]);
  return VNF_OK;
}

}  // namespace vnf
