// device_once.hpp -- what a unit does once per device, under a lock (one process may drive several GPUs from several
// threads): hipFuncSetAttribute applies to the current device only.  No HIP in here: internal.hpp's once_per_device supplies the
// current device and the refusal; host/test_device_once.cc drives this header alone.
#pragma once
#include <mutex>

namespace mlmcpi {

constexpr int kMaxDevices = 64;
constexpr int kDeviceOutOfRange = 1;  // (the statuses of the library are <= 0)

struct DeviceOnce {
  std::mutex mutex;
  bool done[kMaxDevices] = {false};
};

// init() for device `dev`, unless it has succeeded there before: its status, 0 (MLMCPI_OK) latches.  A failed init is
// run again by the next call.  dev outside [0, kMaxDevices): kDeviceOutOfRange, init not called.
template <class Init>
int device_once(DeviceOnce &once, int dev, Init init) {
  if (dev < 0 || dev >= kMaxDevices) return kDeviceOutOfRange;
  std::lock_guard<std::mutex> lock(once.mutex);
  if (once.done[dev]) return 0;
  const int rc = init();
  once.done[dev] = rc == 0;
  return rc;
}

}  // namespace mlmcpi
