// What the plan builders (plan_*.cpp) share: the description of one convolution launch in terms of the reference's
// layers, and the packer that turns it into a ConvLayer + Op::CONV of the plan.
#pragma once
#include "engine.h"

namespace vnf {

struct Piece {  // output channels contributed by one reference conv / linear
  const float* w;  // [cout][cin][KH][KW]
  int cout, cout_pad;
  std::vector<float> scale, bias;  // per logical output channel
  std::vector<float> slope;        // optional PReLU slopes
};

struct SegSpec { int c0, c1, buf, coff; };

struct ConvSpec {
  std::string name;
  int x_buf, x_coff = 0, cin, cin_pad;
  int KH = 1, KW = 1, sh = 1, sw = 1, ph = 0, pw = 0;
  std::vector<Piece> pieces;
  std::vector<SegSpec> segs;
  int res_buf = -1, res_coff = 0;
  int act = ACT_RELU, out_f32 = 0;
  // folded pre-conv BatchNorm (IR-100 bn1): x' = x*pre_s[c] + pre_t[c] on valid (unpadded) taps
  const std::vector<float>* pre_s = nullptr;
  const std::vector<float>* pre_t = nullptr;
};

// Packs the weights of `s` and appends its ConvLayer and Op::CONV to the plan.
int add_conv(Encoder& e, const ConvSpec& s);

// BatchNorm `p` (state_dict prefix) of C channels as y = x * s + t; false: a tensor is missing (wm.missing names it)
bool bn_fold(WeightMap& wm, const std::string& p, int C, float eps, std::vector<float>& s, std::vector<float>& t);

// What follows the convolution of a single-piece ConvSpec, by state_dict name ("": none): the BatchNorm prefix `bn`
// folded at `eps` into scale and bias, or the explicit `bias`; then PReLU with the slopes `prelu`.
struct Epilogue {
  std::string bn;
  float eps = 0.f;
  std::string bias, prelu;
  static Epilogue batchnorm(const std::string& bn, float eps, const std::string& prelu = "") { return {bn, eps, "", prelu}; }
  static Epilogue biased(const std::string& bias, const std::string& prelu = "") { return {"", 0.f, bias, prelu}; }
};

// One Piece of `cout` channels (padded to cout_pad if given): the weights wm[wname] ([cout][taps], taps = cin * KH * KW)
// with `ep` behind them.  false: a tensor is missing (wm.missing names it).
bool fill_piece(WeightMap& wm, Piece& pc, const std::string& wname, int cout, int taps, const Epilogue& ep, int cout_pad = 0);

// The usual ConvSpec, ONE Piece: fill_piece on the geometry the caller has set in `s`, every column written to
// (out_buf, out_coff).  The caller adjusts the piece if the layer needs more (a residual scale, constant slopes) and
// hands `s` to add_conv.
bool single_piece(WeightMap& wm, ConvSpec& s, const std::string& wname, int cout, int out_buf, int out_coff, const Epilogue& ep,
                  int cout_pad = 0);

// A linear layer as a 1x1 convolution over a 1x1 "image" (used by the MLP classifier).
int add_linear(Encoder& e, const std::string& name, const float* w, const float* b, int cin, int cout, int cout_pad,
               int x_buf, int o_buf, int act);

// The op groups of the two ResNets (IR-100, ResNet-50), whose first two stages end at ops end1 / end2 and work on the same
// tensor sizes: they run in sub-batches of 32 / 64 images (VNF_IR100_CHUNK1 / 2) so that producer -> consumer tensors stay
// in the Infinity Cache; the rest takes the whole batch
void add_resnet_groups(Encoder& e, int end1, int end2);

#define TRY(x) do { int _r = (x); if (_r != VNF_OK) return _r; } while (0)
#define NEED(x) do { if (!(x)) return fail(VNF_E_MISSING, "missing weight: " + wm.missing); } while (0)

}  // namespace vnf
