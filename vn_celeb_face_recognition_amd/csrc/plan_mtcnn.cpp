#include "plan.h"

namespace vnf {

// MTCNN R-Net (mtcnn.py:52-99) and O-Net (102-157) as plans on the exact-f32 MFMA convolution core.
// Candidates are the batch dimension; the crop kernel writes NHWC4 fp32 crops into the first buffer.
// dense4 / dense5 consume x.permute(0,3,2,1) flattened (feature (w*H + h)*C + c), i.e. they are a
// 3x3 "convolution" over the 3x3xC map with weight[o][c][kh=h][kw=w] = dense[o][(w*3 + h)*C + c].
static int mtcnn_conv(Encoder& e, WeightMap& wm, const std::string& name, const std::string& prelu, int xb, int cin,
                      int cin_pad, int cout, int cout_pad, int k, int ob) {
  ConvSpec s;
  s.name = name; s.x_buf = xb; s.cin = cin; s.cin_pad = cin_pad; s.KH = s.KW = k;
  if (!single_piece(wm, s, name + ".weight", cout, ob, 0, Epilogue::biased(name + ".bias", prelu + ".weight"), cout_pad))
    return fail(VNF_E_MISSING, "mtcnn: missing weight " + wm.missing);
  s.act = ACT_PRELU;
  return add_conv(e, s);
}

static int mtcnn_dense(Encoder& e, WeightMap& wm, const std::string& name, const std::string& prelu, int xb, int C,
                       int nout, int ob, std::vector<float>& keep) {
  ConvSpec s;
  s.name = name; s.x_buf = xb; s.cin = s.cin_pad = C; s.KH = s.KW = 3;
  if (!single_piece(wm, s, name + ".weight", nout, ob, 0, Epilogue::biased(name + ".bias", prelu + ".weight")))
    return fail(VNF_E_MISSING, "mtcnn: missing weight " + wm.missing);
  const float* d = s.pieces[0].w;
  keep.assign((size_t)nout * C * 9, 0.f);
  for (int o = 0; o < nout; ++o)
    for (int c = 0; c < C; ++c)
      for (int h = 0; h < 3; ++h)
        for (int w = 0; w < 3; ++w) keep[(((size_t)o * C + c) * 3 + h) * 3 + w] = d[(size_t)o * C * 9 + (w * 3 + h) * C + c];
  s.pieces[0].w = keep.data();
  s.act = ACT_PRELU;
  return add_conv(e, s);
}

static int mtcnn_heads(Encoder& e, WeightMap& wm, const std::vector<std::pair<std::string, int>>& heads, int xb, int nin,
                       int ob, int total_pad) {
  ConvSpec s;
  s.name = "heads"; s.x_buf = xb; s.cin = s.cin_pad = nin;
  s.pieces.resize(heads.size());
  int tot = 0;
  for (size_t i = 0; i < heads.size(); ++i) {
    const int n = heads[i].second, pad = (i + 1 == heads.size()) ? total_pad - tot : n;
    if (!fill_piece(wm, s.pieces[i], heads[i].first + ".weight", n, nin, Epilogue::biased(heads[i].first + ".bias"), pad))
      return fail(VNF_E_MISSING, "mtcnn: missing weight " + wm.missing);
    tot += pad;
  }
  s.segs.push_back({0, total_pad, ob, 0});
  s.act = ACT_NONE;
  return add_conv(e, s);
}

// conv1 + PReLU + pool1 are computed by the detector's own fused kernel (mtcnn.hip net_front_kernel), which reads
// nb.crops and writes nb.pooled1; the plan starts at conv2.  mid: conv2 + pool2 as well, from net_mid_kernel (mtcnn.hip:
// the plan starts at conv3 and reads nb.pooled2)
int build_rnet(Encoder& e, WeightMap& wm, bool mid, NetBufs& nb) {
  e.in_size = 24;
  const int x = e.add_buf(24, 24, 4), p1 = e.add_buf(11, 11, 32);
  const int c2 = e.add_buf(9, 9, 48), p2 = e.add_buf(4, 4, 48), c3 = e.add_buf(3, 3, 64), d4 = e.add_buf(1, 1, 128);
  const int hd = e.add_buf(1, 1, 8);
  nb = {x, p1, p2, hd};
  static thread_local std::vector<float> keep;
  if (!mid) {
    TRY(mtcnn_conv(e, wm, "conv2", "prelu2", p1, 28, 32, 48, 48, 3, c2));
    e.ops.push_back(Op::maxpool_ceil(c2, p2, 3));
  }
  TRY(mtcnn_conv(e, wm, "conv3", "prelu3", p2, 48, 48, 64, 64, 2, c3));
  TRY(mtcnn_dense(e, wm, "dense4", "prelu4", c3, 64, 128, d4, keep));
  TRY(mtcnn_heads(e, wm, {{"dense5_1", 2}, {"dense5_2", 4}}, d4, 128, hd, 8));
  // names of vnf_mtcnn_debug_net_tap (metadata only)
  e.taps["crops"] = {x, 0, 4}; e.taps["pool1"] = {p1, 0, 32}; e.taps["conv2"] = {c2, 0, 48}; e.taps["pool2"] = {p2, 0, 48};
  e.taps["conv3"] = {c3, 0, 64}; e.taps["dense"] = {d4, 0, 128}; e.taps["heads"] = {hd, 0, 8};
  return VNF_OK;
}

int build_onet(Encoder& e, WeightMap& wm, bool mid, NetBufs& nb) {
  e.in_size = 48;
  const int x = e.add_buf(48, 48, 4), p1 = e.add_buf(23, 23, 32);
  const int c2 = e.add_buf(21, 21, 64), p2 = e.add_buf(10, 10, 64), c3 = e.add_buf(8, 8, 64), p3 = e.add_buf(4, 4, 64);
  const int c4 = e.add_buf(3, 3, 128), d5 = e.add_buf(1, 1, 256);
  const int hd = e.add_buf(1, 1, 16);
  nb = {x, p1, p2, hd};
  static thread_local std::vector<float> keep;
  if (!mid) {
    TRY(mtcnn_conv(e, wm, "conv2", "prelu2", p1, 32, 32, 64, 64, 3, c2));
    e.ops.push_back(Op::maxpool_ceil(c2, p2, 3));
  }
  TRY(mtcnn_conv(e, wm, "conv3", "prelu3", p2, 64, 64, 64, 64, 3, c3));
  e.ops.push_back(Op::maxpool_ceil(c3, p3, 2));
  TRY(mtcnn_conv(e, wm, "conv4", "prelu4", p3, 64, 64, 128, 128, 2, c4));
  TRY(mtcnn_dense(e, wm, "dense5", "prelu5", c4, 128, 256, d5, keep));
  TRY(mtcnn_heads(e, wm, {{"dense6_1", 2}, {"dense6_2", 4}, {"dense6_3", 10}}, d5, 256, hd, 16));
  e.taps["crops"] = {x, 0, 4}; e.taps["pool1"] = {p1, 0, 32}; e.taps["conv2"] = {c2, 0, 64}; e.taps["pool2"] = {p2, 0, 64};
  e.taps["conv3"] = {c3, 0, 64}; e.taps["pool3"] = {p3, 0, 64}; e.taps["conv4"] = {c4, 0, 128}; e.taps["dense"] = {d5, 0, 256};
  e.taps["heads"] = {hd, 0, 16};
  return VNF_OK;
}

}  // namespace vnf
