// lgar_host.hpp -- host-side helpers shared by the translation units of liblgar_hip.so: what needs the HIP API (the plans and
// argument blocks themselves are in lgar_plan.hpp)
#pragma once
#include <hip/hip_runtime.h>

#include "lgar_plan.hpp"

namespace lgar {

// wave slots of the chip for a kernel compiled for `waves` waves per SIMD
inline unsigned wave_slots(int waves) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  return (unsigned)cus * 4u * (unsigned)waves;
}

inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : LGAR_E_LAUNCH;
}

}  // namespace lgar
