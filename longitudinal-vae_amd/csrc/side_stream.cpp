// side_stream.cpp -- see side_stream.hpp.
#include "side_stream.hpp"

#include "lvae_hip.h"

namespace lvae {

namespace {
constexpr int kMaxDev = 64;
SideStream g_side[kMaxDev];
}  // namespace

std::recursive_mutex& side_mutex() {
  static std::recursive_mutex mu;
  return mu;
}

int side_stream(SideStream*& out) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return LVAE_ERR_LAUNCH;
  SideStream& sd = g_side[dev];
  if (!sd.s) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return LVAE_ERR_LAUNCH;
    sd.cus = prop.multiProcessorCount;
    // (the events first: sd.s, the "created" mark, is set last)
    for (hipEvent_t* e : {&sd.fork, &sd.prep, &sd.c, &sd.u2p[0], &sd.u2p[1], &sd.piv[0], &sd.piv[1], &sd.rbx, &sd.rb,
                          &sd.efork, &sd.edone})
      if (!*e && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return LVAE_ERR_LAUNCH;
    if (hipStreamCreateWithPriority(&sd.s, hipStreamNonBlocking, greatest) != hipSuccess) return LVAE_ERR_LAUNCH;
  }
  out = &sd;
  return 0;
}

}  // namespace lvae

extern "C" int lvae_set_early_stream(void* stream) {
  std::lock_guard<std::recursive_mutex> lock(lvae::side_mutex());
  lvae::SideStream* sd = nullptr;
  if (int rc = lvae::side_stream(sd)) return rc;
  sd->early = (hipStream_t)stream;
  return 0;
}
