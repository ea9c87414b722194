// path1d.hip -- the standalone methods of the 1-D path actions (harmonic / quartic oscillator, topological rotor), batched
// over B chains laid out chain-major x[b*M + j]:
//   * Action::evaluate / Action::force / initialise_state   (drop-in methods)
//   * QoIXsquared / QoISusceptibility
//   * QMAction::copy_from_fine / copy_from_coarse
// and the reductions the other path units call (path_common.hpp, which also lists those units).
#include "path_common.hpp"

namespace mlmcpi {

// ---- standalone evaluate / force / QoI ------------------------------------------------------------

// grid (nsplit, B); partial[b*nsplit + s] = sum over the split's sites of the site term
template <int KIND, int OP>
__global__ void __launch_bounds__(256) path_reduce_kernel(PathP P, const double *__restrict__ x,
                                                          double *__restrict__ partial, double scale,
                                                          double *__restrict__ out) {
  __shared__ double red[4];
  const uint32_t b = blockIdx.y, M = P.M;
  const double *xb = x + (size_t)b * M;
  const uint32_t per = (M + gridDim.x - 1) / gridDim.x;
  const uint32_t lo = blockIdx.x * per, hi = min(M, lo + per);
  double acc[1] = {0.0};
  for (uint32_t j = lo + threadIdx.x; j < hi; j += blockDim.x) {
    const double xj = xb[j], xl = xb[j == 0 ? M - 1 : j - 1];
    if (OP == R_ENERGY) acc[0] += site_energy<KIND>(P, xj, xl);
    if (OP == R_XSQUARED) acc[0] += xj * xj;
    if (OP == R_WINDING) acc[0] += mod_2pi(xj - xl);
  }
  block_sum<1>(acc, red);
  if (threadIdx.x != 0) return;
  if (gridDim.x == 1)  // one workgroup per chain: the sum is complete, finish here (what path_finish_kernel does)
    out[b] = (OP == R_WINDING) ? (1. / (4. * kPi * kPi)) * (acc[0] * acc[0]) * scale : scale * acc[0];
  else
    partial[(size_t)b * gridDim.x + blockIdx.x] = acc[0];
}

// out[b] = finish(sum_s partial[b][s]); one thread per chain, fixed summation order
__global__ void path_finish_kernel(const double *__restrict__ partial, uint32_t nsplit, uint32_t B, int op,
                                   double scale, double *__restrict__ out, double *__restrict__ acc = nullptr) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (uint32_t k = 0; k < nsplit; ++k) s += partial[(size_t)b * nsplit + k];
  // R_WINDING: chi = Q^2 / (4 pi^2 T)  (qoisusceptibility.cc:20-22); others: scale * sum
  const double v = (op == R_WINDING) ? (1. / (4. * kPi * kPi)) * (s * s) * scale : scale * s;
  out[b] = v;
  if (acc) record_moments(acc + 5 * (size_t)b, v);  // stats->record_sample of the value as well (the recurrence of stats_accumulate_kernel)
}

template <int KIND>
__global__ void __launch_bounds__(256) path_force_kernel(PathP P, const double *__restrict__ x,
                                                         double *__restrict__ f) {
  const uint32_t b = blockIdx.y, M = P.M;
  const double *xb = x + (size_t)b * M;
  double *fb = f + (size_t)b * M;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < M; j += gridDim.x * blockDim.x) {
    const double xl = xb[j == 0 ? M - 1 : j - 1], xr = xb[j + 1 == M ? 0 : j + 1];
    fb[j] = site_force<KIND>(P, xl, xb[j], xr);
  }
}

__global__ void __launch_bounds__(256) path_init_kernel(int kind, uint32_t M, RngKey key0, double *__restrict__ x) {
  const uint32_t b = blockIdx.y;
  RngKey key = key0;
  key.chain += b;
  double *xb = x + (size_t)b * M;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < M; j += gridDim.x * blockDim.x) {
    if (kind == MLMCPI_ROTOR) {
      double u, v;
      rng_uniforms(key, j, P_INIT, 0, u, v);
      xb[j] = -kPi + 2.0 * kPi * u;
    } else {
      xb[j] = 0.0;
    }
  }
}

// QMAction::copy_from_fine / copy_from_coarse (action/qm/qmaction.cc:7-24): even sites of the fine path
__global__ void __launch_bounds__(256) path_transfer_kernel(uint32_t Mc, double *__restrict__ fine_all,
                                                            double *__restrict__ coarse_all, int to_coarse) {
  const uint32_t b = blockIdx.y;
  double *fine = fine_all + (size_t)b * 2 * Mc, *coarse = coarse_all + (size_t)b * Mc;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < Mc; j += gridDim.x * blockDim.x) {
    if (to_coarse) coarse[j] = fine[2 * j]; else fine[2 * j] = coarse[j];
  }
}

// ---- host dispatch ---------------------------------------------------------------------------------------
int check_action(const mlmcpi_path_action *act) {
  if (!act) return fail(MLMCPI_ERR_INVALID, "action is NULL");
  if (act->kind < MLMCPI_HARMONIC || act->kind > MLMCPI_ROTOR)
    return fail(MLMCPI_ERR_INVALID, "kind %d is not a 1-D path action", act->kind);
  if (act->M < 2) return fail(MLMCPI_ERR_INVALID, "M_lat = %u too small", act->M);
  if (!(act->T_final > 0.0)) return fail(MLMCPI_ERR_INVALID, "T_final must be positive");
  return MLMCPI_OK;
}

uint32_t choose_split(uint32_t sites, uint32_t B) {
  // enough workgroups to fill 256 CUs, at least ~1024 sites each
  uint32_t want = (2048 + B - 1) / B, cap = (sites + 1023) / 1024;
  uint32_t n = want < cap ? want : cap;
  return n ? n : 1;
}

template <int OP>
static int launch_reduce(const PathP &P, const double *d_x, uint32_t B, double scale, double *d_out, hipStream_t st) {
  const uint32_t nsplit = choose_split(P.M, B);
  void *ws = nullptr;
  int rc = scratch((size_t)B * nsplit * sizeof(double), &ws, st);
  if (rc) return rc;
  dim3 grid(nsplit, B), block(256);
  dispatch_kind(P.kind, [&](auto K) {
    hipLaunchKernelGGL((path_reduce_kernel<decltype(K)::value, OP>), grid, block, 0, st, P, d_x, (double *)ws, scale, d_out);
  });
  MLMCPI_LAUNCH_CHECK("path_reduce_kernel");
  if (nsplit == 1) return MLMCPI_OK;
  return path_finish((const double *)ws, nsplit, B, OP, scale, d_out, nullptr, st);
}

int path_reduce(int op, const PathP &P, const double *d_x, uint32_t B, double scale, double *d_out, hipStream_t st) {
  switch (op) {
    case R_ENERGY: return launch_reduce<R_ENERGY>(P, d_x, B, scale, d_out, st);
    case R_XSQUARED: return launch_reduce<R_XSQUARED>(P, d_x, B, scale, d_out, st);
    default: return launch_reduce<R_WINDING>(P, d_x, B, scale, d_out, st);
  }
}

int path_finish(const double *partial, uint32_t nsplit, uint32_t B, int op, double scale, double *d_out, double *d_acc, hipStream_t st) {
  hipLaunchKernelGGL(path_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, st, partial, nsplit, B, op, scale, d_out, d_acc);
  MLMCPI_LAUNCH_CHECK("path_finish_kernel");
  return MLMCPI_OK;
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

int mlmcpi_path_evaluate(const mlmcpi_path_action *act, const double *d_x, uint32_t B, double *d_S, void *stream) {
  if (int rc = check_action(act)) return rc;
  MLMCPI_REQUIRE(d_x && d_S && B > 0, "bad arguments");
  PathP P = make_params(*act);
  return path_reduce(R_ENERGY, P, d_x, B, energy_scale(P), d_S, as_stream(stream));
}

int mlmcpi_path_force(const mlmcpi_path_action *act, const double *d_x, double *d_f, uint32_t B, void *stream) {
  if (int rc = check_action(act)) return rc;
  MLMCPI_REQUIRE(d_x && d_f && B > 0 && d_x != d_f, "bad arguments");
  PathP P = make_params(*act);
  dim3 grid(choose_split(P.M, B) , B), block(256);
  hipStream_t st = as_stream(stream);
  dispatch_kind(P.kind, [&](auto K) { hipLaunchKernelGGL(path_force_kernel<decltype(K)::value>, grid, block, 0, st, P, d_x, d_f); });
  MLMCPI_LAUNCH_CHECK("path_force_kernel");
  return MLMCPI_OK;
}

int mlmcpi_path_initialise(const mlmcpi_path_action *act, double *d_x, uint32_t B, uint64_t seed, uint32_t chain0,
                           void *stream) {
  if (int rc = check_action(act)) return rc;
  MLMCPI_REQUIRE(d_x && B > 0, "bad arguments");
  dim3 grid(choose_split(act->M, B), B), block(256);
  hipLaunchKernelGGL(path_init_kernel, grid, block, 0, as_stream(stream), act->kind, act->M, make_key(seed, chain0, 0),
                     d_x);
  MLMCPI_LAUNCH_CHECK("path_init_kernel");
  return MLMCPI_OK;
}

int mlmcpi_qoi_xsquared(const double *d_x, uint32_t M, uint32_t B, double *d_out, void *stream) {
  MLMCPI_REQUIRE(d_x && d_out && B > 0 && M > 1, "bad arguments");
  PathP P = {};
  P.kind = MLMCPI_HARMONIC;
  P.M = M;
  return path_reduce(R_XSQUARED, P, d_x, B, 1.0 / M, d_out, as_stream(stream));
}

int mlmcpi_qoi_susceptibility(const double *d_x, uint32_t M, double T_final, uint32_t B, double *d_out,
                              void *stream) {
  MLMCPI_REQUIRE(d_x && d_out && B > 0 && M > 1 && T_final > 0, "bad arguments");
  PathP P = {};
  P.kind = MLMCPI_ROTOR;
  P.M = M;
  return path_reduce(R_WINDING, P, d_x, B, 1.0 / T_final, d_out, as_stream(stream));
}

int mlmcpi_path_copy_from_fine(const double *d_fine, double *d_coarse, uint32_t M_coarse, uint32_t B, void *stream) {
  MLMCPI_REQUIRE(d_fine && d_coarse && M_coarse > 0 && B > 0, "bad arguments");
  hipLaunchKernelGGL(path_transfer_kernel, dim3(choose_split(M_coarse, B), B), dim3(256), 0, as_stream(stream), M_coarse,
                     (double *)d_fine, d_coarse, 1);
  MLMCPI_LAUNCH_CHECK("path_transfer_kernel");
  return MLMCPI_OK;
}

int mlmcpi_path_copy_from_coarse(const double *d_coarse, double *d_fine, uint32_t M_coarse, uint32_t B, void *stream) {
  MLMCPI_REQUIRE(d_fine && d_coarse && M_coarse > 0 && B > 0, "bad arguments");
  hipLaunchKernelGGL(path_transfer_kernel, dim3(choose_split(M_coarse, B), B), dim3(256), 0, as_stream(stream), M_coarse,
                     d_fine, (double *)d_coarse, 0);
  MLMCPI_LAUNCH_CHECK("path_transfer_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
