// path_twolevel.hip -- the two-level Metropolis step of the 1-D paths, one launch per step.
#include "path_common.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

// ---- two-level Metropolis step (montecarlo/twolevelmetropolisstep.cc:35-89) ----------------------------------
// Conditioned-action quantities of the Gaussian fill-in (action/qm/gaussianconditionedfineaction.cc:7-43):
// HO  harmonicoscillatoraction.hh:163-189: W'' = 2 m0/a + a m0 mu2, x0 = (x- + x+) / (2 + a^2 mu2)
// quartic quarticoscillatoraction.hh:160-194: W'' = (2/a + a mu2) m0 + 3 lambda a (xbar - x0)^2, x0 by 4 fixed-point steps
template <int KIND>
__device__ __forceinline__ void w_conditioned(const PathP &P, double x_m, double x_p, double &w_min, double &w_curv) {
  if (KIND == MLMCPI_ROTOR) {  // rotoraction.hh:195-213
    double sm, cm, sp, cp;
    sincos(x_m, &sm, &cm);
    sincos(x_p, &sp, &cp);
    w_min = atan2(sp + sm, cp + cm);
    w_curv = 2.0 * P.m0 / P.a * fabs(cos(0.5 * (x_p - x_m)));
  } else if (KIND == MLMCPI_HARMONIC) {
    w_curv = (2. / P.a + P.a * P.mu2) * P.m0;
    w_min = (0.5 / (1. + 0.5 * P.a * P.a * P.mu2)) * (x_m + x_p);
  } else {
    const double xbar = 0.5 * (x_m + x_p);
    const double rho = 1. / (1. + 0.5 * P.a * P.a * P.mu2);
    double x = xbar;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double sh = x - P.x0;
      x = rho * (xbar - 0.5 * P.a * P.a * P.lambda / P.m0 * sh * sh * sh);
    }
    w_min = x;
    w_curv = (2. / P.a + P.a * P.mu2) * P.m0 + 3. * P.lambda * P.a * (xbar - P.x0) * (xbar - P.x0);
  }
}

// TwoLevelMetropolisStep::draw (montecarlo/twolevelmetropolisstep.cc:35-89) for one chain per workgroup, in ONE launch (r02:
// a propose kernel, four reductions of two launches each and an accept kernel -- ten launches for an O(M) streaming job,
// 27 % of the multilevel kernel time).  The thread of coarse site j builds theta'[2j] = x_c[j] and the fill-in
// theta'[2j+1] (Gaussian around Wminimum with Wcurvature, gaussianconditionedfineaction.cc:7-43; ExpSin2 for the rotor,
// rotorconditionedfineaction.cc:7-43; Philox normals / von Mises draws of site 2j+1) and adds up, for the sites 2j+1 and
// 2j+2 of the fine paths and for coarse site j+1, the six sums of the step:
//     S_f(theta'), S_f(theta), S_c(theta_C), S_c(x_c), S_cfa(theta'), S_cfa(theta).
// The workgroup reduces them in a fixed order, takes the decision (exp(-dS) against the chain's P_ACCEPT2 uniform) and,
// if accepted, copies theta' over theta -- every thread the entries it wrote itself.
template <int KIND>
__global__ void __launch_bounds__(KIND == MLMCPI_ROTOR ? 512 : 1024)  // the rotor's libm calls want more than 128 registers
    twolevel_fused_kernel(PathP Pf, PathP Pc, const double *__restrict__ x_coarse, double *__restrict__ theta,
                          double *__restrict__ theta_prime, int32_t *__restrict__ accept, double *__restrict__ terms, RngKey key0,
                          const int32_t *__restrict__ mask) {
  __shared__ double red[6 * 16];
  __shared__ int decision;
  const uint32_t b = blockIdx.x, M = Pf.M, Mc = M / 2;
  if (mask && mask[b] == 0) {  // hierarchicalsampler.cc:62-76: a chain rejected further down does not move on this level
    if (threadIdx.x == 0) {
      accept[b] = 0;
      if (terms) terms[3 * b + 0] = terms[3 * b + 1] = terms[3 * b + 2] = 0.0;
    }
    return;
  }
  const double *xc = x_coarse + (size_t)b * Mc;
  double *th = theta + (size_t)b * M, *tp = theta_prime + (size_t)b * M;
  RngKey key = key0;
  key.chain += b;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint32_t j = threadIdx.x; j < Mc; j += blockDim.x) {
    const uint32_t jn = (j + 1 == Mc) ? 0 : j + 1;
    const double x_m = xc[j], x_p = xc[jn];
    double w_min, w_curv;
    w_conditioned<KIND>(Pf, x_m, x_p, w_min, w_curv);
    double fill;
    if (KIND == MLMCPI_ROTOR) {
      const double sigma = 2. * w_curv;
      fill = mod_2pi(w_min + vonmises_draw(key, 2 * j + 1, 0.5 * sigma, kVmFillin));
      const double sh = sin(0.5 * (fill - w_min));
      acc[4] += sigma * sh * sh + log(two_pi_i0_scaled(0.5 * sigma));
    } else {
      const double sigma = 1. / sqrt(w_curv);
      fill = w_min + rng_normal0(key, 2 * j + 1, P_FILLIN, 0) * sigma;
      const double dxp = fill - w_min;
      acc[4] += 0.5 * w_curv * dxp * dxp - 0.5 * log(w_curv);
    }
    tp[2 * j] = x_m;
    tp[2 * j + 1] = fill;
    const double t_m = th[2 * j], t_o = th[2 * j + 1], t_p = th[2 * jn];
    w_conditioned<KIND>(Pf, t_m, t_p, w_min, w_curv);
    const double dx = t_o - w_min;
    if (KIND == MLMCPI_ROTOR) {
      const double sigma = 2. * w_curv, sh = sin(0.5 * dx);
      acc[5] += sigma * sh * sh + log(two_pi_i0_scaled(0.5 * sigma));
    } else {
      acc[5] += 0.5 * w_curv * dx * dx - 0.5 * log(w_curv);
    }
    // actions: sites 2j+1 and 2j+2 of the fine paths, site j+1 of the coarse ones (each site once over all j)
    acc[0] += site_energy<KIND>(Pf, fill, x_m) + site_energy<KIND>(Pf, x_p, fill);
    acc[1] += site_energy<KIND>(Pf, t_o, t_m) + site_energy<KIND>(Pf, t_p, t_o);
    acc[2] += site_energy<KIND>(Pc, t_p, t_m);
    acc[3] += site_energy<KIND>(Pc, x_p, x_m);
  }
  block_sum<6>(acc, red);
  if (threadIdx.x == 0) {
    const double dS_fine = energy_scale(Pf) * acc[0] - energy_scale(Pf) * acc[1];
    const double dS_coarse = energy_scale(Pc) * acc[2] - energy_scale(Pc) * acc[3];
    const double dS_trial = acc[5] - acc[4];
    const double dS = dS_fine + dS_coarse + dS_trial;
    bool ok = dS < 0.0;
    if (!ok) {
      double u, v;
      rng_uniforms(key, 0, P_ACCEPT2, 0, u, v);
      ok = u < exp(-dS);
    }
    decision = ok ? 1 : 0;
    accept[b] = decision;
    if (terms) {
      terms[3 * b + 0] = dS_fine; terms[3 * b + 1] = dS_coarse; terms[3 * b + 2] = dS_trial;
    }
  }
  __syncthreads();
  if (!decision) return;
  for (uint32_t j = threadIdx.x; j < Mc; j += blockDim.x) {  // the entries this thread wrote above
    th[2 * j] = tp[2 * j];
    th[2 * j + 1] = tp[2 * j + 1];
  }
}

}  // namespace mlmcpi

using namespace mlmcpi;

extern "C" {

// workspace: theta' [B*M] (the trial state; kept at the r02 size, which also held reduction partials)
static uint32_t twolevel_blocks(uint32_t M, uint32_t B) { return choose_split(M / 2, B); }

int mlmcpi_path_twolevel_workspace_bytes(const mlmcpi_path_action *fine, uint32_t B, size_t *bytes) {
  if (int rc = check_action(fine)) return rc;
  MLMCPI_REQUIRE(bytes && B > 0, "bad arguments");
  *bytes = align256((size_t)B * fine->M * 8) + align256((size_t)4 * B * 8) +
           align256((size_t)B * twolevel_blocks(fine->M, B) * 2 * 8);
  return MLMCPI_OK;
}

int mlmcpi_path_twolevel_draw(const mlmcpi_path_action *fine, const mlmcpi_path_action *coarse, const double *d_x_coarse,
                              double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step, void *d_work,
                              int32_t *d_accept, double *d_terms, void *stream) {
  return mlmcpi_path_twolevel_draw_masked(fine, coarse, d_x_coarse, d_theta, B, seed, chain0, step, d_work, nullptr, d_accept, d_terms,
                                          stream);
}

int mlmcpi_path_twolevel_draw_masked(const mlmcpi_path_action *fine, const mlmcpi_path_action *coarse, const double *d_x_coarse,
                                     double *d_theta, uint32_t B, uint64_t seed, uint32_t chain0, uint32_t step, void *d_work,
                                     const int32_t *d_mask, int32_t *d_accept, double *d_terms, void *stream) {
  if (int rc = check_action(fine)) return rc;
  if (int rc = check_action(coarse)) return rc;
  MLMCPI_REQUIRE(d_x_coarse && d_theta && d_work && d_accept && B > 0, "bad arguments");
  MLMCPI_REQUIRE(fine->M % 2 == 0 && coarse->M == fine->M / 2 && coarse->kind == fine->kind,
                 "coarse action must live on the lattice with half the sites (M %u vs %u)", coarse->M, fine->M);
  hipStream_t st = as_stream(stream);
  const PathP Pf = make_params(*fine), Pc = make_params(*coarse);
  double *theta_prime = (double *)d_work;
  const RngKey key = make_key(seed, chain0, step);
  // one workgroup per chain; as many threads as there are coarse sites, up to 1024 (then several sites per thread)
  uint32_t nt = 64;
  while (nt < (Pf.kind == MLMCPI_ROTOR ? 512u : 1024u) && nt < Pf.M / 2) nt *= 2;
  const dim3 grid(B), block(nt);
  dispatch_kind(Pf.kind, [&](auto K) {
    hipLaunchKernelGGL(twolevel_fused_kernel<decltype(K)::value>, grid, block, 0, st, Pf, Pc, d_x_coarse, d_theta, theta_prime, d_accept,
                       d_terms, key, d_mask);
  });
  MLMCPI_LAUNCH_CHECK("twolevel_fused_kernel");
  return MLMCPI_OK;
}

}  // extern "C"
