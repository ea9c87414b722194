// test_device_once.cc -- the once-per-device guard of the library's LDS-heavy units (mlmcpathintegral_amd/csrc/device_once.hpp)
// on its own: no HIP, no library.  tests/test_device_once.py builds and runs it.
#include <stdio.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../mlmcpathintegral_amd/csrc/device_once.hpp"

using namespace mlmcpi;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);             \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

// 16 threads x 4 device indices x repeated calls: init runs exactly once per device, and every call returns its status
static void test_threads() {
  constexpr int kThreads = 16, kDevices = 4, kRepeats = 200;
  DeviceOnce once;
  int ran[kDevices] = {0, 0, 0, 0};  // written under the guard's lock only: a race here is a failure of the guard
  std::atomic<int> bad_status{0};
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([&, t] {
      for (int r = 0; r < kRepeats; ++r)
        for (int d = 0; d < kDevices; ++d) {
          const int dev = (d + t) % kDevices;  // (the threads do not walk the devices in step)
          if (device_once(once, dev, [&]() -> int { ++ran[dev]; return 0; }) != 0) ++bad_status;
        }
    });
  for (auto &th : threads) th.join();
  for (int d = 0; d < kDevices; ++d) CHECK(ran[d] == 1);
  CHECK(bad_status == 0);
  for (int d = 0; d < kMaxDevices; ++d) CHECK(once.done[d] == (d < kDevices));
}

// an init that fails is not latched: its status comes back, and the next call runs it again
static void test_failure_is_not_latched() {
  DeviceOnce once;
  int calls = 0;
  auto init = [&]() -> int { return ++calls < 3 ? -2 : 0; };
  CHECK(device_once(once, 5, init) == -2 && calls == 1 && !once.done[5]);
  CHECK(device_once(once, 5, init) == -2 && calls == 2 && !once.done[5]);
  CHECK(device_once(once, 5, init) == 0 && calls == 3 && once.done[5]);
  CHECK(device_once(once, 5, init) == 0 && calls == 3);
  CHECK(device_once(once, 6, [&]() -> int { ++calls; return 0; }) == 0 && calls == 4);  // another device: its own latch
  CHECK(device_once(once, 0, [&]() -> int { ++calls; return 0; }) == 0 && calls == 5);
  CHECK(device_once(once, kMaxDevices - 1, [&]() -> int { ++calls; return 0; }) == 0 && calls == 6 && once.done[kMaxDevices - 1]);
}

// indices outside [0, kMaxDevices) are refused without calling init
static void test_range() {
  DeviceOnce once;
  int calls = 0;
  auto init = [&]() -> int { ++calls; return 0; };
  CHECK(kMaxDevices == 64 && kDeviceOutOfRange > 0);
  CHECK(device_once(once, -1, init) == kDeviceOutOfRange);
  CHECK(device_once(once, 64, init) == kDeviceOutOfRange);
  CHECK(device_once(once, 1 << 30, init) == kDeviceOutOfRange);
  CHECK(calls == 0);
  for (int d = 0; d < kMaxDevices; ++d) CHECK(!once.done[d]);
}

int main() {
  test_threads();
  test_failure_is_not_latched();
  test_range();
  if (failures) printf("test_device_once: %d FAILED\n", failures);
  else printf("test_device_once OK\n");
  return failures ? 1 : 0;
}
