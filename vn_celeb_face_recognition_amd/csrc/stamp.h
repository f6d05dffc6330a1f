// Host side of the in-kernel cycle stamps (tools/stamp_patch.py, tools/stamp_ws.py): only in a build with -DVNF_STAMPS
// (build.py --stamps).  Without it the DBG = true kernels are not instantiated and the VNF_*_STAMP variables are ignored.
#pragma once
#ifdef VNF_STAMPS
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace vnf {

// One stamped launch: `n` zeroed 64-bit slots on the current device, for this call only; launch(buf) enqueues the
// instrumented kernel on `s`; after the stream has drained, rows(f, host) appends to the file that `env` names.
template <class Launch, class Rows>
inline hipError_t stamped_launch(const char* env, int n, hipStream_t s, Launch launch, Rows rows) {
  long long* dbuf = nullptr;
  if (hipMalloc((void**)&dbuf, n * 8) != hipSuccess) return hipErrorOutOfMemory;
  (void)hipMemsetAsync(dbuf, 0, n * 8, s);
  launch(dbuf);
  const hipError_t e = hipStreamSynchronize(s);
  std::vector<long long> host(n);
  if (e == hipSuccess) (void)hipMemcpy(host.data(), dbuf, n * 8, hipMemcpyDeviceToHost);
  (void)hipFree(dbuf);
  if (e != hipSuccess) return e;
  if (FILE* f = fopen(getenv(env), "a")) {
    rows(f, host.data());
    fclose(f);
  }
  return hipSuccess;
}

}  // namespace vnf
#endif  // VNF_STAMPS
