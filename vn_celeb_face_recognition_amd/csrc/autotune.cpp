// Create-time choices of an encoder: the switches it takes from the environment and the tile configuration of each
// convolution.
#include "engine.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>

namespace vnf {

EncoderEnv EncoderEnv::read() {
  auto env_int = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
  EncoderEnv e;
  e.fuse = env_int("VNF_FUSE", e.fuse);
  e.direct_stem = env_int("VNF_DIRECT_STEM", e.direct_stem);
  e.stem1a_mfma = env_int("VNF_STEM1A_MFMA", e.stem1a_mfma);
  e.stem_chunk = env_int("VNF_STEM_CHUNK", e.stem_chunk);
  e.ir100_chunk1 = env_int("VNF_IR100_CHUNK1", e.ir100_chunk1);
  e.ir100_chunk2 = env_int("VNF_IR100_CHUNK2", e.ir100_chunk2);
  e.retina_fuse = env_int("VNF_RETINA_FUSE", e.retina_fuse);
  e.ws_persist = env_int("VNF_WS_PERSIST", e.ws_persist);
  e.autotune = env_int("VNF_AUTOTUNE", e.autotune);
  e.force_cfg = env_int("VNF_FORCE_CFG", e.force_cfg);
  e.tune_lanes = env_int("VNF_TUNE_LANES", e.tune_lanes);
  e.autotune_log = env_int("VNF_AUTOTUNE_LOG", e.autotune_log);
  e.tune_final = env_int("VNF_TUNE_FINAL", 1) != 0;
  if (const char* cache = getenv("VNF_TUNE_CACHE")) e.tune_cache = cache;
  return e;
}

// Pick each convolution's tile configuration by timing the candidates on this device at the
// batch size it will see (measure, don't guess: the best tile depends on M, N, K, the number of
// workgroups and where the operands sit in the cache hierarchy).  ~1 s at create time.
int Encoder::autotune() {
  const int enabled = env.autotune, force = env.force_cfg;   // the switches as they were when the handle was created
  if (!enabled && force < -1) return VNF_OK;
  // VNF_TUNE_CACHE=<file>: reuse the choices of an earlier create on this device (lines "key cfg"); lets a
  // profiled run show steady-state launches only and brings create time down to the weight upload
  std::map<std::string, int> cache;
  const char* cache_path = env.tune_cache.empty() ? nullptr : env.tune_cache.c_str();
  bool cache_dirty = false;
  if (cache_path && enabled) {
    if (FILE* f = fopen(cache_path, "r")) {
      char key[256];
      int c;
      while (fscanf(f, "%255s %d", key, &c) == 2) cache[key] = c;
      fclose(f);
    }
  }
  // tuning launches scribble over the activation buffers: nothing of an earlier vnf_embed may still be in flight,
  // and nothing of the tuner when the caller's launches start
  VNF_HIP(hipDeviceSynchronize());
  // the timing events and lane streams, released on every way out of this function
  struct Timers {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t lane_s[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t lane_e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Timers() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      for (int l = 0; l < 4; ++l) {
        if (lane_e[l]) (void)hipEventDestroy(lane_e[l]);
        if (lane_s[l]) (void)hipStreamDestroy(lane_s[l]);
      }
    }
  } tm;
  VNF_HIP(hipEventCreate(&tm.e0));
  VNF_HIP(hipEventCreate(&tm.e1));
  // tune_lanes > 1: every candidate is timed as `tune_lanes` concurrent copies on separate streams -- the state the
  // layer actually runs in when independent batches overlap (activation contexts): alone on the GPU a small tile with
  // many workgroups looks best, beside other kernels the tile that moves fewer bytes per FLOP does
  const int lanes = env.tune_lanes > 0 ? (env.tune_lanes > 4 ? 4 : env.tune_lanes) : (tune_lanes < 1 ? 1 : tune_lanes);
  if (lanes > 1)
    for (int l = 0; l < lanes; ++l) {
      VNF_HIP(hipStreamCreateWithFlags(&tm.lane_s[l], hipStreamNonBlocking));
      VNF_HIP(hipEventCreate(&tm.lane_e[l]));
    }
  for (const Group& g : groups) {
    int part = (max_batch >= 192 && max_streams > 1) ? (max_batch + 1) / 2 : max_batch;  // run() cuts the batch over 2 streams
    if (tune_batch > 0 && tune_batch < part) part = tune_batch;
    const int nn = g.chunk < part ? g.chunk : part;
    for (int oi = g.first; oi < g.last; ++oi) {
      if (fused_at[oi] >= 0) {  // replaced by a persistent kernel: nothing to tune
        oi = fused[fused_at[oi]].end() - 1;
        continue;
      }
      if (ops[oi].kind != Op::CONV) continue;
      ConvLayer& L = convs[ops[oi].layer];
      float best = 1e30f;
      int best_cfg = -1;
      char key[256];
      snprintf(key, sizeof key, "%s/d%d/n%d/M%d/K%d/N%d/v%d/L%d", L.name.c_str(), dtype, nn, nn * L.Ho * L.Wo, L.Kpad, L.cout,
               conv_num_cfgs(), lanes);
      const auto hit = cache.find(key);
      if (hit != cache.end()) {
        ConvArgs a = conv_args(L, 0, nn);
        if (hit->second == -1 || conv_cfg_ok(a, hit->second)) { L.cfg = hit->second; continue; }
      }
      std::vector<std::pair<float, int>> timed;   // (ms per 4 launches, cfg) of every candidate
      // time one candidate: the minimum over `trials` of `reps` back-to-back launches (per lane), scaled to 4 launches
      auto time_cfg = [&](const ConvArgs& a, int trials, int reps, float* out_ms) -> int {
        float ms = 1e30f;
        for (int trial = 0; trial < trials; ++trial) {
          float t = 0;
          if (lanes <= 1) {
            VNF_HIP(hipEventRecord(tm.e0, 0));
            for (int r = 0; r < reps; ++r) (void)launch_conv(a, 0);
            VNF_HIP(hipEventRecord(tm.e1, 0));
            VNF_HIP(hipEventSynchronize(tm.e1));
            VNF_HIP(hipEventElapsedTime(&t, tm.e0, tm.e1));
          } else {
            VNF_HIP(hipDeviceSynchronize());
            VNF_HIP(hipEventRecord(tm.e0, tm.lane_s[0]));
            for (int r = 0; r < reps; ++r)
              for (int l = 0; l < lanes; ++l) (void)launch_conv(a, tm.lane_s[l]);
            for (int l = 0; l < lanes; ++l) VNF_HIP(hipEventRecord(tm.lane_e[l], tm.lane_s[l]));
            for (int l = 0; l < lanes; ++l) {
              float tl = 0;
              VNF_HIP(hipEventSynchronize(tm.lane_e[l]));
              VNF_HIP(hipEventElapsedTime(&tl, tm.e0, tm.lane_e[l]));
              if (tl > t) t = tl;
            }
          }
          t *= 4.f / reps;
          if (t < ms) ms = t;
        }
        *out_ms = ms;
        return VNF_OK;
      };
      const int logit = env.autotune_log;
      for (int cfg = -1; enabled && cfg < conv_num_cfgs(); ++cfg) {
        ConvArgs a = conv_args(L, 0, nn);
        a.cfg = cfg;
        if (cfg >= 0 && !conv_cfg_ok(a, cfg)) continue;
        if (launch_conv(a, 0) != hipSuccess) { (void)hipGetLastError(); continue; }
        float ms = 1e30f;
        const int rc = time_cfg(a, 2, 4, &ms);
        if (rc != VNF_OK) return rc;
        timed.emplace_back(ms, cfg);
        if (ms < best) { best = ms; best_cfg = cfg; }
        if (logit) fprintf(stderr, "autotune %s cfg %d: %.4f ms\n", L.name.c_str(), cfg, ms / 4);
      }
      // finalists: the first pass is 8 launches per candidate and two candidates a few per cent apart change places from
      // run to run; the ones within 8 % of the best are timed again, longer (VNF_TUNE_FINAL=0: first pass only)
      if (env.tune_final && timed.size() > 1) {
        std::sort(timed.begin(), timed.end());
        float fbest = 1e30f;
        int fcfg = best_cfg, nfin = 0;
        for (const auto& tc : timed) {
          if (tc.first > timed[0].first * 1.08f || nfin == 4) break;
          ++nfin;
          ConvArgs a = conv_args(L, 0, nn);
          a.cfg = tc.second;
          float ms = 1e30f;
          const int rc = time_cfg(a, 3, 8, &ms);
          if (rc != VNF_OK) return rc;
          if (logit) fprintf(stderr, "autotune %s final cfg %d: %.4f ms\n", L.name.c_str(), tc.second, ms / 4);
          if (ms < fbest) { fbest = ms; fcfg = tc.second; }
        }
        if (nfin > 1) { best = fbest; best_cfg = fcfg; }
      }
      L.cfg = best_cfg;
      if (cache_path && enabled) { cache[key] = best_cfg; cache_dirty = true; }
      if (force >= -1) {
        ConvArgs a = conv_args(L, 0, nn);
        if (force == -1 || conv_cfg_ok(a, force)) L.cfg = force;
      }
    }
  }
  VNF_HIP(hipDeviceSynchronize());
  if (cache_dirty) {
    if (FILE* f = fopen(cache_path, "w")) {
      for (auto& kv : cache) fprintf(f, "%s %d\n", kv.first.c_str(), kv.second);
      fclose(f);
    }
  }
  return VNF_OK;
}

}  // namespace vnf
