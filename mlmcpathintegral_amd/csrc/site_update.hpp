// site_update.hpp -- one heat-bath or overrelaxation update of one site of the 2-D actions (Schwinger, GFF), on a state that
// is read and written in place.  Included by lattice_sweep.hpp (lattice_site_update_kernel) and random_sweep.hip, whose
// kernels must agree on it.
#pragma once
#include "device_common.hpp"
#include "step_envelope.hpp"
#include "vonmises.hpp"

namespace mlmcpi {

// ---- Action::heatbath_update / overrelaxation_update(state, l) of the 2-D actions on a state that is read and written in
// place (gffaction.cc:33-42,68-77; quenchedschwingeraction.cc:25-65): the body of the site-at-a-time kernels
// (lattice_site_update_kernel) and of the random-order sweep (random_sweep.hip), which must agree
// `th` = the chain's links theta[2 (Mt j + i) + mu]; step = 2 coupling <= kVsKappaMax (the step-envelope sampler and its table)
__device__ __forceinline__ void schwinger_site_update(double *th, uint32_t Mt, uint32_t Mx, uint32_t l, bool heat, bool step,
                                                      double coupling, const RngKey &key, const VsTable &tab) {
  auto link = [&](uint32_t i, uint32_t j, uint32_t mu) -> double & { return th[2 * (Mt * j + i) + mu]; };
  const uint32_t mu = l & 1u, v = l >> 1, j = v / Mt, i = v - j * Mt;
  const uint32_t ip = i + 1 == Mt ? 0 : i + 1, im = i == 0 ? Mt - 1 : i - 1, jp = j + 1 == Mx ? 0 : j + 1, jm = j == 0 ? Mx - 1 : j - 1;
  double tp, tm;  // staple sums, unwrapped (quenchedschwingeraction.cc:25-43; same sums as schwinger_sweep_kernel)
  if (mu == 0) {
    tp = link(i, jp, 0) + link(i, j, 1) - link(ip, j, 1);
    tm = link(i, jm, 0) + link(ip, jm, 1) - link(i, jm, 1);
  } else {
    tp = link(i, j, 0) + link(ip, j, 1) - link(i, jp, 0);
    tm = link(im, jp, 0) + link(im, j, 1) - link(im, j, 0);
  }
  double &x = th[l];
  if (!heat) {
    x = mod_2pi_fast((tp + tm) - x);
  } else if (step) {
    x = vs_draw(key, l, 2. * coupling, tp, tm, tab);
  } else {
    double tau, centre;
    expcos_params(coupling, tp, tm, tau, centre);
    x = mod_2pi_fast(vonmises_draw(key, l, tau) + centre);
  }
}

// `phi` = the chain's field phi[Mt j + i]; inv_kappa = 1 / (4 + mu2), two_over_kappa = 2 / (4 + mu2), sigma = 1 / sqrt(4 + mu2)
__device__ __forceinline__ void gff_site_update(double *phi, uint32_t Mt, uint32_t Mx, uint32_t l, bool heat, double inv_kappa,
                                                double two_over_kappa, double sigma, const RngKey &key) {
  const uint32_t j = l / Mt, i = l - j * Mt;
  const uint32_t ip = i + 1 == Mt ? 0 : i + 1, im = i == 0 ? Mt - 1 : i - 1, jp = j + 1 == Mx ? 0 : j + 1, jm = j == 0 ? Mx - 1 : j - 1;
  double Delta = 0.0;  // the order of the reference's neighbour table: +i, -i, +j, -j
  Delta += phi[Mt * j + ip];
  Delta += phi[Mt * j + im];
  Delta += phi[Mt * jp + i];
  Delta += phi[Mt * jm + i];
  if (!heat) {
    phi[l] = fma(two_over_kappa, Delta, -phi[l]);
  } else {
    double n0, n1;
    rng_normals(key, l >> 1, P_GFF_NORMAL, 0, n0, n1);
    phi[l] = fma(Delta, inv_kappa, sigma * ((l & 1u) ? n1 : n0));
  }
}

}  // namespace mlmcpi
