// test_hooks.hip -- test kernels of the RNG contract and of the heat-bath samplers, with their entry points.
#include "internal.hpp"
#include "step_envelope.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

__global__ void test_random_kernel(RngKey key, uint32_t purpose, uint32_t sub, uint32_t n, double *out) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double u0, u1, n0, n1;
  rng_uniforms(key, k, purpose, sub, u0, u1);
  rng_normals(key, k, purpose, sub, n0, n1);
  out[4 * k + 0] = u0;
  out[4 * k + 1] = u1;
  out[4 * k + 2] = n0;
  out[4 * k + 3] = n1;
}

__global__ void test_philox_kernel(U4 ctr, uint32_t k0, uint32_t k1, uint32_t *out) {
  U4 r = philox4x32_10(ctr.x, ctr.y, ctr.z, ctr.w, k0, k1);
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

__global__ void test_expcos_kernel(RngKey key, double beta, const double *xp, const double *xm, uint32_t n,
                                   double *out) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = expcos_draw(key, k, beta, xp[k], xm[k]);
}

__global__ void __launch_bounds__(256)
    test_vs_draw_kernel(RngKey key, double scale, const double *xp, const double *xm, uint32_t n, const uint32_t *d_table, double *out) {
  __shared__ uint32_t tab_lds[kVsTableBytes / 4];
  const VsTable tab = VsTable::stage(tab_lds, d_table);
  __syncthreads();
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = vs_draw(key, k, scale, xp[k], xm[k], tab);
}

__global__ void test_expsin2_kernel(RngKey key, const double *sigma, uint32_t n, double *out) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = expsin2_draw(key, k, sigma[k]);
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_test_philox(const uint32_t *ctr4, const uint32_t *key2, uint32_t *out4) {
  MLMCPI_REQUIRE(ctr4 && key2 && out4, "NULL argument");
  uint32_t *d = nullptr;
  MLMCPI_HIP_TRY(hipMalloc(&d, 16));
  hipLaunchKernelGGL(test_philox_kernel, dim3(1), dim3(1), 0, 0, U4{ctr4[0], ctr4[1], ctr4[2], ctr4[3]}, key2[0],
                     key2[1], d);
  MLMCPI_LAUNCH_CHECK("test_philox_kernel");
  MLMCPI_HIP_TRY(hipMemcpy(out4, d, 16, hipMemcpyDeviceToHost));
  MLMCPI_HIP_TRY(hipFree(d));
  return MLMCPI_OK;
}

int mlmcpi_test_random(uint64_t seed, uint32_t chain, uint32_t step, uint32_t purpose, uint32_t sub, uint32_t n,
                       double *d_out, void *stream) {
  MLMCPI_REQUIRE(d_out && n > 0, "bad arguments");
  hipLaunchKernelGGL(test_random_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream),
                     make_key(seed, chain, step), purpose, sub, n, d_out);
  MLMCPI_LAUNCH_CHECK("test_random_kernel");
  return MLMCPI_OK;
}

int mlmcpi_test_expcos(uint64_t seed, uint32_t chain, uint32_t step, double beta, const double *d_xp,
                       const double *d_xm, uint32_t n, double *d_out, void *stream) {
  MLMCPI_REQUIRE(d_xp && d_xm && d_out && n > 0, "bad arguments");
  hipLaunchKernelGGL(test_expcos_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream),
                     make_key(seed, chain, step), beta, d_xp, d_xm, n, d_out);
  MLMCPI_LAUNCH_CHECK("test_expcos_kernel");
  return MLMCPI_OK;
}

int mlmcpi_test_vs_draw(uint64_t seed, uint32_t chain, uint32_t step, double scale, const double *d_xp, const double *d_xm,
                        uint32_t n, double *d_out, void *stream) {
  MLMCPI_REQUIRE(d_xp && d_xm && d_out && n > 0 && scale >= 0.0 && scale <= kVsKappaMax, "bad arguments");
  const uint32_t *d_table = nullptr;
  if (int rc = vs_table_device(scale, &d_table)) return rc;
  hipLaunchKernelGGL(test_vs_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), make_key(seed, chain, step),
                     scale, d_xp, d_xm, n, d_table, d_out);
  MLMCPI_LAUNCH_CHECK("test_vs_draw_kernel");
  return MLMCPI_OK;
}

int mlmcpi_test_expsin2(uint64_t seed, uint32_t chain, uint32_t step, const double *d_sigma, uint32_t n,
                        double *d_out, void *stream) {
  MLMCPI_REQUIRE(d_sigma && d_out && n > 0, "bad arguments");
  hipLaunchKernelGGL(test_expsin2_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream),
                     make_key(seed, chain, step), d_sigma, n, d_out);
  MLMCPI_LAUNCH_CHECK("test_expsin2_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
