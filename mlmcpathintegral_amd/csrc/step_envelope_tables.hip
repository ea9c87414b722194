// step_envelope_tables.hip -- the tables of the step-envelope heat-bath sampler (step_envelope.hpp), built on the host for an
// action's scale: the tables themselves (exported as mlmcpi_vs_table), their device image, and the cache of uploaded images
// per (device, scale).
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "internal.hpp"
#include "step_envelope.hpp"

namespace mlmcpi {

// For the action's scale (kappa = scale |cos(.)| <= scale <= kVsKappaMax) and each of the kVsClasses ranges of kappa: the
// proposal probabilities q_k / 64 of the eight bins, as a 64-entry selector, and log2 of the acceptance factors.
// q[c][k] selector values for bin k of class c, lw[c][k] = log2 of its acceptance factor
static void vs_build_tables(double scale, int *q_out, float *lw) {
  for (int c = 0; c < kVsClasses; ++c) {
    const double kmin = scale * sin(2.0 * kPi * c / 32.0);  // the smallest concentration of the class
    double hw[kVsBins], w[kVsBins], total = 0.0;
    for (int k = 0; k < kVsBins; ++k) {
      w[k] = vs_width16(k) * (kPi / 16.0);
      hw[k] = exp(kmin * (cos(vs_edge16(k) * (kPi / 16.0)) - 1.0)) * w[k];  // target at the bin's left edge (its maximum) x width
      total += hw[k];
    }
    int *q = q_out + c * kVsBins, sum = 0;
    for (int k = 0; k < kVsBins; ++k) {
      q[k] = (int)floor(hw[k] / total * kVsSel);
      if (q[k] < 1) q[k] = 1;
      sum += q[k];
    }
    while (sum < kVsSel) {  // the bin that binds the envelope constant gets the next selector value
      int j = 0;
      for (int k = 1; k < kVsBins; ++k)
        if (hw[k] / q[k] > hw[j] / q[j]) j = k;
      ++q[j];
      ++sum;
    }
    while (sum > kVsSel) {  // (many bins at the minimum of one value): take from the bin that stays lowest
      int j = -1;
      for (int k = 0; k < kVsBins; ++k)
        if (q[k] > 1 && (j < 0 || hw[k] / (q[k] - 1) < hw[j] / (q[j] - 1))) j = k;
      --q[j];
      --sum;
    }
    double M = 0.0;
    for (int k = 0; k < kVsBins; ++k) M = fmax(M, hw[k] / q[k]);
    for (int k = 0; k < kVsBins; ++k) {
      // acceptance factor (w_k / q_k) / M <= 1 / H_k, lowered by 4e-6 in log2 so that float rounding never lifts it above
      const double x = log2(w[k] / q[k] / M) - 4e-6;
      float f = (float)x;
      if ((double)f > x) f = nextafterf(f, -INFINITY);
      lw[c * kVsBins + k] = f;
    }
  }
}

// the device image (step_envelope.hpp, "Device image of the tables"): code | scr | lw | fin | consts
static void vs_device_image(double scale, uint32_t *image) {
  int q[kVsClasses * kVsBins];
  float lw[kVsClasses * kVsBins];
  vs_build_tables(scale, q, lw);
  memset(image, 0, kVsTableBytes);
  uint8_t *bytes = (uint8_t *)image;
  for (int c = 0; c < kVsClasses; ++c) {
    int pos = 0;
    for (int k = 0; k < kVsBins; ++k) {
      for (int i = 0; i < q[c * kVsBins + k]; ++i) bytes[kVsCodeOff + c * kVsSel + pos++] = (uint8_t)(8 * k);
      memcpy(bytes + kVsLwOff + c * kVsSel + 8 * k, &lw[c * kVsBins + k], 4);
    }
  }
  for (int k = 0; k < kVsBins; ++k) {
    const double e = vs_edge16(k), w = vs_width16(k);
    const float scr[2] = {(float)(0.5 * kPi - (kPi / 16.0) * e), (float)(-(kPi / 16.0) * w / 4294967296.0)};
    const double fin[2] = {64.0 * w, e - 64.0 * w};
    memcpy(bytes + kVsScrOff + 8 * k, scr, 8);
    memcpy(bytes + kVsFinOff + 16 * k, fin, 16);
  }
  const float band = vs_band_of_scale(scale);
  const float consts[4] = {4294967296.0f * (1.0f - band), 4294967296.0f * (1.0f + band), 0.f, 0.f};
  memcpy(bytes + kVsConstOff, consts, 16);
}

namespace {
struct VsTableEntry { int device; double scale; uint32_t *d_table; };
std::mutex g_vs_mutex;
std::vector<VsTableEntry> g_vs_tables;
}  // namespace

int vs_table_device(double scale, const uint32_t **d_table) {
  int dev = 0;
  MLMCPI_HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_vs_mutex);
  for (const VsTableEntry &e : g_vs_tables)
    if (e.device == dev && e.scale == scale) {
      *d_table = e.d_table;
      return MLMCPI_OK;
    }
  uint32_t host[kVsTableBytes / 4];
  vs_device_image(scale, host);
  uint32_t *d = nullptr;
  MLMCPI_HIP_TRY(hipMalloc((void **)&d, kVsTableBytes));
  MLMCPI_HIP_TRY(hipMemcpy(d, host, kVsTableBytes, hipMemcpyHostToDevice));  // first use of this scale on this device only
  g_vs_tables.push_back(VsTableEntry{dev, scale, d});
  *d_table = d;
  return MLMCPI_OK;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_vs_table(double scale, uint8_t *sel, float *lw) {
  MLMCPI_REQUIRE(sel && lw && scale >= 0.0 && scale <= kVsKappaMax, "bad arguments (0 <= scale <= %g)", kVsKappaMax);
  int q[kVsClasses * kVsBins];
  vs_build_tables(scale, q, lw);
  for (int c = 0; c < kVsClasses; ++c) {
    int pos = 0;
    for (int k = 0; k < kVsBins; ++k)
      for (int i = 0; i < q[c * kVsBins + k]; ++i) sel[c * kVsSel + pos++] = (uint8_t)k;
  }
  return MLMCPI_OK;
}

}  // extern "C"
