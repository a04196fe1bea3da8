// Node topology probe: which local GPU pairs are joined by a direct xGMI link.
//
// The schedules of mp4x assume the MI355X node shape — 8 GPUs, every pair one xGMI hop apart
// (7 links per GPU), peer memory readable by kernels.  The reference has no counterpart (its
// topology is "hosts on 1 GbE", README.md:300); here the probe is evidence that a multi-GPU run
// really crossed xGMI (bench.py records it), and the device engine logs a warning when a pair is
// not a single xGMI hop (PCIe-only boxes still work: the autotuners choose from measurements).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mp4x/runtime.h"

extern "C" int mp4x_topology(int cap, int* link, int* hops, int* access, int* rank, int* atomics) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return -(int)e;
  if (n > cap) n = cap;
  for (int a = 0; a < n; ++a) {
    for (int b = 0; b < n; ++b) {
      const int i = a * n + b;
      link[i] = -1;
      hops[i] = 0;
      access[i] = a == b;
      rank[i] = 0;
      atomics[i] = a == b;
      if (a == b) continue;
      uint32_t lt = 0, hc = 0;
      if (hipExtGetLinkTypeAndHopCount(a, b, &lt, &hc) == hipSuccess) {
        link[i] = (int)lt;
        hops[i] = (int)hc;
      }
      int v = 0;
      if (hipDeviceGetP2PAttribute(&v, hipDevP2PAttrAccessSupported, a, b) == hipSuccess) access[i] = v;
      if (hipDeviceGetP2PAttribute(&v, hipDevP2PAttrPerformanceRank, a, b) == hipSuccess) rank[i] = v;
      if (hipDeviceGetP2PAttribute(&v, hipDevP2PAttrNativeAtomicSupported, a, b) == hipSuccess) atomics[i] = v;
    }
  }
  (void)hipGetLastError();   // a failed query must not poison the next kernel launch's error check
  return n;
}
