// Weight packing of the plans: BatchNorm folding, MFMA-ready weight images, gather tables.
#include "plan.h"
#include "split_f16.h"

#include <cmath>

namespace vnf {

int add_conv(Encoder& e, const ConvSpec& s) {
  const int es = dtype_size(e.dtype), ch = dtype_chan_align(e.dtype), bke = 128 / es;
  const bool planar = e.dtype == F16P;
  const Buf& xb = e.bufs[s.x_buf];
  ConvLayer L;
  L.name = s.name;
  L.x_buf = s.x_buf; L.x_coff = s.x_coff; L.cin = s.cin_pad;
  L.H = xb.H; L.W = xb.W;
  L.KH = s.KH; L.KW = s.KW; L.sh = s.sh; L.sw = s.sw; L.ph = s.ph; L.pw = s.pw;
  L.Ho = (L.H + 2 * s.ph - s.KH) / s.sh + 1;
  L.Wo = (L.W + 2 * s.pw - s.KW) / s.sw + 1;
  if (s.cin_pad % ch || s.x_coff % ch || xb.C % ch) return fail(VNF_E_INVALID, s.name + ": channel alignment");
  L.K = s.KH * s.KW * s.cin_pad;
  L.Kpad = (L.K + bke - 1) / bke * bke;
  int cout = 0, cout_logical = 0;
  for (auto& p : s.pieces) { cout += p.cout_pad; cout_logical += p.cout; }
  L.cout = cout;
  L.cout_pad = (cout + 127) / 128 * 128;
  L.ncls = s.pre_s ? 9 : 1;
  // The nine border-class biases below, and the epilogue that picks one by ho == 0 / ho == Ho - 1 (wo alike), hold where
  // row 0 loses exactly the ph top taps, row Ho - 1 exactly the ph bottom taps and no row between them any: stride 1,
  // at most one padding row / column, and a first and a last row / column that are two different ones.
  if (s.pre_s && (!s.pre_t || s.sh != 1 || s.sw != 1 || s.ph > 1 || s.pw > 1 || (s.ph > 0 && L.Ho < 2) || (s.pw > 0 && L.Wo < 2)))
    return fail(VNF_E_INVALID, s.name + ": a folded pre-conv BatchNorm needs stride 1, padding <= 1 and, where it pads, "
                               "at least two output rows / columns");
  if (cout % 8) return fail(VNF_E_INVALID, s.name + ": cout % 8");

  std::vector<float> wpk((size_t)L.cout_pad * L.Kpad, 0.f);
  std::vector<float> bias((size_t)L.ncls * L.cout_pad, 0.f), slope((size_t)L.cout_pad, 0.f);
  bool has_slope = false;
  int co0 = 0;
  for (auto& p : s.pieces) {
    if (!p.w) return fail(VNF_E_MISSING, s.name + ": weight missing");
    for (int co = 0; co < p.cout; ++co) {
      const float sc = p.scale.empty() ? 1.f : p.scale[co];
      float* dst = &wpk[(size_t)(co0 + co) * L.Kpad];
      for (int c = 0; c < s.cin; ++c) {
        const float ps = s.pre_s ? (*s.pre_s)[c] : 1.f;
        for (int kh = 0; kh < s.KH; ++kh)
          for (int kw = 0; kw < s.KW; ++kw) {
            const float wv = p.w[(((size_t)co * s.cin + c) * s.KH + kh) * s.KW + kw];
            dst[(kh * s.KW + kw) * s.cin_pad + c] = wv * sc * ps;
          }
      }
      const float b = p.bias.empty() ? 0.f : p.bias[co];
      if (!s.pre_s) {
        bias[co0 + co] = b;
      } else {
        // border classes: the BN shift only reaches the output through taps that land inside
        // the image; class (r,c) in {first, interior, last}^2 selects the valid tap set.
        for (int rc = 0; rc < 3; ++rc)
          for (int cc = 0; cc < 3; ++cc) {
            double acc = 0;
            for (int kh = 0; kh < s.KH; ++kh) {
              if ((rc == 0 && kh < s.ph) || (rc == 2 && kh >= s.KH - s.ph)) continue;
              for (int kw = 0; kw < s.KW; ++kw) {
                if ((cc == 0 && kw < s.pw) || (cc == 2 && kw >= s.KW - s.pw)) continue;
                for (int c = 0; c < s.cin; ++c)
                  acc += (double)p.w[(((size_t)co * s.cin + c) * s.KH + kh) * s.KW + kw] * (*s.pre_t)[c];
              }
            }
            bias[(size_t)(rc * 3 + cc) * L.cout_pad + co0 + co] = b + (float)(acc * sc);
          }
      }
      if (!p.slope.empty()) { slope[co0 + co] = p.slope[co]; has_slope = true; }
    }
    co0 += p.cout_pad;
  }
  std::vector<char> wdev((size_t)L.cout_pad * L.Kpad * es);
  convert_to(e.dtype, wpk.data(), wdev.data(), wpk.size());
  L.w = e.upload(wdev.data(), wdev.size());
  L.bias = (float*)e.upload(bias.data(), bias.size() * 4);
  if (has_slope) L.slope = (float*)e.upload(slope.data(), slope.size() * 4);
  // gather table: one entry per 16-byte chunk of the K-tile image, 8 per K tile.  Planar split-f16: chunk q of a tile
  // is the hi (q < 4) or lo (q >= 4) plane of the 8-channel unit q & 3, 16 bytes (4 elements) into the unit for lo.
  std::vector<int4> kt(L.Kpad / bke * 8);
  for (int kc = 0; kc < (int)kt.size(); ++kc) {
    const int q = kc & 7;
    const int k = planar ? (kc >> 3) * bke + (q & 3) * 8 : kc * (16 / es);
    if (k < L.K) {
      const int tap = k / s.cin_pad, c = k % s.cin_pad, kh = tap / s.KW, kw = tap % s.KW;
      kt[kc] = int4{(kh * L.W + kw) * xb.C + c + (planar ? (q >> 2) * 4 : 0), kh, kw, 1};
    } else {
      kt[kc] = int4{0, 0, 0, 0};
    }
  }
  L.ktab = (int4*)e.upload(kt.data(), kt.size() * sizeof(int4));
  if (!L.w || !L.bias || !L.ktab) return VNF_E_HIP;

  L.nseg = (int)s.segs.size();
  if (L.nseg < 1 || L.nseg > 4) return fail(VNF_E_INVALID, s.name + ": segments");
  for (int i = 0; i < L.nseg; ++i) {
    L.seg[i].c0 = s.segs[i].c0; L.seg[i].c1 = s.segs[i].c1;
    L.seg[i].buf = s.segs[i].buf; L.seg[i].coff = s.segs[i].coff;
    if (s.segs[i].buf >= 0) {
      const Buf& ob = e.bufs[s.segs[i].buf];
      if (ob.H != L.Ho || ob.W != L.Wo || s.segs[i].coff + (s.segs[i].c1 - s.segs[i].c0) > ob.C)
        return fail(VNF_E_INVALID, s.name + ": output buffer shape");
    }
  }
  L.res_buf = s.res_buf; L.res_coff = s.res_coff;
  L.act = s.act; L.out_f32 = s.out_f32;
  L.macs_alg = (double)L.Ho * L.Wo * cout_logical * (double)(s.KH * s.KW * s.cin);
  const int kstep = planar ? bke : bke / 2;   // k values one MFMA group consumes
  const int k32 = (L.K + kstep - 1) / kstep * kstep;
  L.macs_exec = (double)L.Ho * L.Wo * cout * (double)k32;
  e.convs.push_back(L);
  e.ops.push_back(Op::conv((int)e.convs.size() - 1));
  return VNF_OK;
}

bool bn_fold(WeightMap& wm, const std::string& p, int C, float eps, std::vector<float>& s, std::vector<float>& t) {
  const float* g = wm.get(p + ".weight", C);
  const float* b = wm.get(p + ".bias", C);
  const float* m = wm.get(p + ".running_mean", C);
  const float* v = wm.get(p + ".running_var", C);
  if (!g || !b || !m || !v) return false;
  s.resize(C); t.resize(C);
  for (int i = 0; i < C; ++i) {
    const double sc = (double)g[i] / std::sqrt((double)v[i] + (double)eps);
    s[i] = (float)sc;
    t[i] = (float)((double)b[i] - (double)m[i] * sc);
  }
  return true;
}

bool fill_piece(WeightMap& wm, Piece& pc, const std::string& wname, int cout, int taps, const Epilogue& ep, int cout_pad) {
  pc.w = wm.get(wname, (int64_t)cout * taps);
  pc.cout = cout;
  pc.cout_pad = cout_pad ? cout_pad : cout;
  const float* b = ep.bias.empty() ? nullptr : wm.get(ep.bias, cout);
  const float* a = ep.prelu.empty() ? nullptr : wm.get(ep.prelu, cout);
  bool ok = pc.w && (b || ep.bias.empty()) && (a || ep.prelu.empty());
  if (!ep.bn.empty()) ok = bn_fold(wm, ep.bn, cout, ep.eps, pc.scale, pc.bias) && ok;
  if (b) pc.bias.assign(b, b + cout);
  if (a) pc.slope.assign(a, a + cout);
  return ok;
}

bool single_piece(WeightMap& wm, ConvSpec& s, const std::string& wname, int cout, int out_buf, int out_coff, const Epilogue& ep,
                  int cout_pad) {
  s.pieces.resize(1);
  s.segs.push_back({0, cout_pad ? cout_pad : cout, out_buf, out_coff});
  return fill_piece(wm, s.pieces[0], wname, cout, s.cin * s.KH * s.KW, ep, cout_pad);
}

void add_resnet_groups(Encoder& e, int end1, int end2) {
  e.groups.push_back({0, end1, e.env.ir100_chunk1 > 0 ? e.env.ir100_chunk1 : 32});
  e.groups.push_back({end1, end2, e.env.ir100_chunk2 > 0 ? e.env.ir100_chunk2 : 64});
  e.groups.push_back({end2, (int)e.ops.size(), 1 << 30});
}

int add_linear(Encoder& e, const std::string& name, const float* w, const float* b, int cin, int cout, int cout_pad,
               int x_buf, int o_buf, int act) {
  ConvSpec s;
  s.name = name; s.x_buf = x_buf; s.cin = s.cin_pad = cin;
  s.pieces.resize(1);
  Piece& pc = s.pieces[0];
  pc.w = w; pc.cout = cout; pc.cout_pad = cout_pad;
  pc.bias.assign(b, b + cout);
  s.segs.push_back({0, cout_pad, o_buf, 0});
  s.act = act;
  return add_conv(e, s);
}

}  // namespace vnf
