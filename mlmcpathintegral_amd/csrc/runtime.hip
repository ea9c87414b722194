// runtime.hip -- plumbing entry points of the C ABI: the error channel, the scratch pool, ABI version, device selection
// and memory.
#include <stdarg.h>
#include <stdio.h>

#include <vector>

#include "internal.hpp"

namespace mlmcpi {

static thread_local char g_err[512] = "";

int fail(int status, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return status;
}

int fail_hip(hipError_t e, const char *what) {
  snprintf(g_err, sizeof(g_err), "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
  return MLMCPI_ERR_HIP;
}

// Scratch for reduction partials: one buffer per (host thread, device, stream), grown on demand (the first call of a
// given size allocates; steady state does not).  A launch sequence that uses it (reduce -> finish) is issued by one
// thread on one stream, so neither another stream nor another host thread driving the same device can overwrite the
// partials in between.  The caller passes the stream it is about to launch on.
namespace {
struct ScratchSlot { int dev; hipStream_t stream; void *ptr; size_t bytes; };
struct ScratchPool {
  std::vector<ScratchSlot> slots;
  ~ScratchPool() {
    for (auto &s : slots)
      if (s.ptr) (void)hipFree(s.ptr);  // may fail at process teardown (runtime already gone): nothing to do about it
  }
};
thread_local ScratchPool t_scratch;
}  // namespace

int scratch(size_t bytes, void **d_ptr, hipStream_t stream) {
  int dev = 0;
  MLMCPI_HIP_TRY(hipGetDevice(&dev));
  ScratchSlot *slot = nullptr;
  for (auto &s : t_scratch.slots)
    if (s.dev == dev && s.stream == stream) slot = &s;
  if (!slot) {
    t_scratch.slots.push_back(ScratchSlot{dev, stream, nullptr, 0});
    slot = &t_scratch.slots.back();
  }
  if (slot->bytes < bytes) {
    if (slot->ptr) {
      MLMCPI_HIP_TRY(hipStreamSynchronize(stream));  // the only work that can still read it is on this stream
      MLMCPI_HIP_TRY(hipFree(slot->ptr));
      slot->ptr = nullptr;
      slot->bytes = 0;
    }
    const size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
    MLMCPI_HIP_TRY(hipMalloc(&slot->ptr, want));
    slot->bytes = want;
  }
  *d_ptr = slot->ptr;
  return MLMCPI_OK;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_abi_version(void) { return MLMCPI_ABI_VERSION; }
const char *mlmcpi_last_error(void) { return g_err; }

int mlmcpi_device_count(int *count) {
  MLMCPI_REQUIRE(count, "count is NULL");
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    fail_hip(e, "hipGetDeviceCount");
    return MLMCPI_ERR_NO_DEVICE;
  }
  return MLMCPI_OK;
}

int mlmcpi_set_device(int device) {
  MLMCPI_HIP_TRY(hipSetDevice(device));
  return MLMCPI_OK;
}

int mlmcpi_device_name(char *buf, size_t len) {
  MLMCPI_REQUIRE(buf && len > 0, "buf is NULL");
  int dev = 0;
  MLMCPI_HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  MLMCPI_HIP_TRY(hipGetDeviceProperties(&prop, dev));
  snprintf(buf, len, "%s (%s)", prop.name, prop.gcnArchName);
  return MLMCPI_OK;
}

int mlmcpi_malloc(void **d_ptr, size_t bytes) {
  MLMCPI_REQUIRE(d_ptr, "d_ptr is NULL");
  MLMCPI_HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 8));
  return MLMCPI_OK;
}
int mlmcpi_free(void *d_ptr) {
  if (d_ptr) MLMCPI_HIP_TRY(hipFree(d_ptr));
  return MLMCPI_OK;
}
int mlmcpi_memset(void *d_ptr, int value, size_t bytes, void *stream) {
  MLMCPI_HIP_TRY(hipMemsetAsync(d_ptr, value, bytes, as_stream(stream)));
  return MLMCPI_OK;
}
int mlmcpi_copy_h2d(void *d_dst, const void *src, size_t bytes, void *stream) {
  MLMCPI_HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, as_stream(stream)));
  MLMCPI_HIP_TRY(hipStreamSynchronize(as_stream(stream)));
  return MLMCPI_OK;
}
int mlmcpi_copy_d2h(void *dst, const void *d_src, size_t bytes, void *stream) {
  MLMCPI_HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
  MLMCPI_HIP_TRY(hipStreamSynchronize(as_stream(stream)));
  return MLMCPI_OK;
}
int mlmcpi_copy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream) {
  MLMCPI_HIP_TRY(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
  return MLMCPI_OK;
}
int mlmcpi_stream_synchronize(void *stream) {
  MLMCPI_HIP_TRY(hipStreamSynchronize(as_stream(stream)));
  return MLMCPI_OK;
}

}  // extern "C"
